"""A numpy restatement of the Gibbs-ringing removal that include/met2_hip.h states for met2_degibbs (local sub-voxel shifts: Kellner,
Dhital, Kiselev, Reisert, MRM 2016), with numpy.fft: the reference of tests/test_gpu_gibbs.py.  Written from the header, not from MRtrix;
not fast.  Besides the output and the chosen shifts it returns, per sample and axis, the margin of the choice: the gap between the best and
the second-best shift's min(TVL, TVR), divided by max|slice|.  A sample whose margin is below TIE is a tie: another correct evaluation
may choose another shift there (formulations of step 2 differ by 1e-14 to 1e-13 max|x|; TIE is four orders above that)."""
import numpy as np

TIE = 1e-9


def shift_table(nsh):
    """sh = [0, 1, ..., nsh, -1, ..., -nsh]"""
    return np.concatenate([np.arange(0, nsh + 1), -np.arange(1, nsh + 1)])


def shifted_lines_fft(x, nsh):
    """step 2 by Fourier interpolation: x [..., n] -> [..., 2 nsh + 1, n]"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    delta = shift_table(nsh) / (2.0 * nsh)
    k = np.fft.fftfreq(n, 1.0 / n)                                   # the signed frequency; -n / 2 at the Nyquist bin of even n
    ph = np.exp(2j * np.pi * k[None, :] * delta[:, None] / n)
    if n % 2 == 0:
        ph[:, n // 2] = 0.0
        ph[0, n // 2] = 1.0
    X = np.fft.fft(x, axis=-1)
    return np.real(np.fft.ifft(X[..., None, :] * ph, axis=-1))


def shift_kernels(n, nsh):
    """the circular-convolution kernels of step 2: c [2 nsh + 1, n]"""
    delta = shift_table(nsh) / (2.0 * nsh)
    K = (n - 1) // 2
    kp = np.arange(-K, K + 1)
    r = np.arange(n)
    c = np.cos(2.0 * np.pi * kp[None, None, :] * (r[None, :, None] + delta[:, None, None]) / n).sum(axis=-1) / n
    if n % 2 == 0:
        c[0] += np.cos(np.pi * r) / n
    return c


def shifted_lines_conv(x, nsh):
    """step 2 as a circular convolution: x_j[m] = sum_l c_j[(m - l) mod n] x[l]"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    c = shift_kernels(n, nsh)
    m = np.arange(n)
    C = c[:, (m[:, None] - m[None, :]) % n]                          # [j, m, l]
    return np.einsum("jml,...l->...jm", C, x)


def unring_lines(x, nsh=20, minW=1, maxW=3, route="fft"):
    """the operator U on the lines x [L, n] -> (out [L, n], shift [L, n] int8, gap [L, n]: second-best minus best min(TVL, TVR))"""
    x = np.asarray(x, dtype=np.float64)
    L, n = x.shape
    sh = shift_table(nsh)
    xs = (shifted_lines_fft if route == "fft" else shifted_lines_conv)(x, nsh)      # [L, J, n]
    d = np.abs(xs - np.roll(xs, 1, axis=-1))                         # d[m] = |x[m] - x[m - 1]|
    tvl = np.zeros_like(d)
    tvr = np.zeros_like(d)
    for t in range(minW, maxW + 1):                                  # formed directly, in increasing t
        tvl = tvl + np.roll(d, t, axis=-1)                           # d[l - t]
        tvr = tvr + np.roll(d, -(t + 1), axis=-1)                    # d[l + t + 1]
    J = sh.size
    cand = np.stack([tvl, tvr], axis=2).reshape(L, 2 * J, n)         # (j = 0, L), (j = 0, R), (j = 1, L), ...
    js = np.argmin(cand, axis=1) // 2                                # the first minimum
    v = np.sort(np.minimum(tvl, tvr), axis=1)
    gap = v[:, 1] - v[:, 0]
    pick = lambda a: np.take_along_axis(a, js[:, None, :], axis=1)[:, 0]
    a0, a1, a2 = pick(np.roll(xs, 1, axis=-1)), pick(xs), pick(np.roll(xs, -1, axis=-1))
    s = sh[js]
    dl = s / (2.0 * nsh)
    out = np.where(dl > 0, a1 * (1.0 - dl) + a0 * dl, a1 * (1.0 + dl) - a2 * dl)
    return out, s.astype(np.int8), gap


def split_weights(nx, ny):
    """Gx, Gy [nx, ny]"""
    cx = 1.0 + np.cos(2.0 * np.pi * np.arange(nx) / nx)
    cy = 1.0 + np.cos(2.0 * np.pi * np.arange(ny) / ny)
    if nx % 2 == 0:
        cx[nx // 2] = 0.0
    if ny % 2 == 0:
        cy[ny // 2] = 0.0
    den = cx[:, None] + cy[None, :]
    safe = np.where(den == 0.0, 1.0, den)
    gx = np.where(den == 0.0, 0.0, cy[None, :] / safe)
    gy = np.where(den == 0.0, 0.0, cx[:, None] / safe)
    return gx, gy


def split2d(S):
    """the 2-D split of a slice: (Ix, Iy)"""
    gx, gy = split_weights(*S.shape)
    F = np.fft.fft2(S)
    return np.real(np.fft.ifft2(F * gx)), np.real(np.fft.ifft2(F * gy))


def degibbs_slice(S, nsh=20, minW=1, maxW=3):
    """-> (out, shift_x, shift_y, margin_x, margin_y), all [nx, ny]"""
    if not np.isfinite(S).all():
        z = np.zeros(S.shape, dtype=np.int8)
        inf = np.full(S.shape, np.inf)
        return S.copy(), z, z.copy(), inf, inf.copy()
    ix, iy = split2d(S)
    ox, sx, gx = unring_lines(ix.T, nsh, minW, maxW)                 # the lines along x are the columns
    oy, sy, gy = unring_lines(iy, nsh, minW, maxW)
    scale = np.abs(S).max()
    scale = scale if scale > 0 else 1.0
    return ox.T + oy, sx.T, sy, gx.T / scale, gy / scale


def degibbs(data, nsh=20, minW=1, maxW=3):
    """data [nx, ny, nz, nt] -> dict(out, shift_x, shift_y, margin_x, margin_y), every (z, echo) slice on its own"""
    data = np.asarray(data, dtype=np.float64)
    nx, ny, nz, nt = data.shape
    if not (nsh >= 1 and 1 <= minW <= maxW and 2 * (maxW + 1) <= min(nx, ny)):
        raise ValueError("bad parameters")
    res = {"out": np.empty_like(data), "shift_x": np.zeros(data.shape, np.int8), "shift_y": np.zeros(data.shape, np.int8),
           "margin_x": np.empty_like(data), "margin_y": np.empty_like(data)}
    for z in range(nz):
        for e in range(nt):
            parts = degibbs_slice(data[:, :, z, e], nsh, minW, maxW)
            for name, p in zip(("out", "shift_x", "shift_y", "margin_x", "margin_y"), parts):
                res[name][:, :, z, e] = p
    return res


def ties(res):
    """the samples whose choice of shift, along either axis, this restatement itself calls a tie"""
    return (res["margin_x"] < TIE) | (res["margin_y"] < TIE)


# The volumes the GPU tests compare on: name -> (shape, seed, (nsh, minW, maxW)).  Every one is 100 + 5 N(0, 1) everywhere (no flat regions);
# tests/test_gibbs_host.py asserts that the restatement calls no sample of any of them a tie.
CASES = {
    "n8": ((8, 8, 1, 1), 1, (20, 1, 3)),              # the smallest shape: the windows wrap
    "odd": ((9, 15, 2, 3), 2, (20, 1, 3)),            # odd along both axes: no Nyquist bin
    "mixed": ((16, 12, 3, 2), 3, (20, 1, 3)),
    "wave": ((65, 64, 1, 2), 4, (20, 1, 3)),          # crosses a wave and a tile
    "long": ((128, 33, 2, 1), 5, (20, 1, 3)),
    "extreme": ((256, 8, 1, 1), 6, (20, 1, 3)),       # the largest against the smallest
    "params": ((16, 12, 1, 1), 7, (4, 2, 4)),
    "nsh32": ((16, 12, 1, 1), 8, (32, 1, 3)),
}


def case(name):
    """-> (data [nx, ny, nz, nt], (nsh, minW, maxW))"""
    shape, seed, params = CASES[name]
    return 100.0 + 5.0 * np.random.default_rng(seed).standard_normal(shape), params


def disc_phantom(n=64, N=512, inside=120.0, outside=20.0, radius=0.3, offset=(0.37, -0.21)):
    """A disc of `inside` on `outside`, radius `radius` N fine pixels, its centre `offset` coarse pixels off the image's, drawn on N x N and
    cropped in k-space to n x n: an image with truncation ringing.  -> (image [n, n], distance from the centre in coarse pixels [n, n])"""
    f = N // n
    c = N / 2.0 + np.asarray(offset) * f
    yy, xx = np.meshgrid(np.arange(N), np.arange(N))
    fine = np.where((xx - c[0]) ** 2 + (yy - c[1]) ** 2 <= (radius * N) ** 2, inside, outside)
    F = np.fft.fftshift(np.fft.fft2(fine))
    lo = N // 2 - n // 2
    Fc = F[lo:lo + n, lo:lo + n].copy()
    img = np.real(np.fft.ifft2(np.fft.ifftshift(Fc))) / f ** 2
    a = np.arange(n)
    # coarse sample a sits at fine position a f (both grids start at the origin)
    dist = np.sqrt((a[:, None] * f - c[0]) ** 2 + (a[None, :] * f - c[1]) ** 2) / f
    return img, dist


def driver_volume(shape=(12, 12, 2), nt=32, seed=21):
    """A two-pool decay with 2 % noise for the driver tests (compared between GPU runs only): (data [nx, ny, nz, nt], mask, TE)"""
    rng = np.random.default_rng(seed)
    te = 10.0 * np.arange(1, nt + 1)
    f = 0.1 + 0.1 * rng.random(shape)[..., None]
    s = 1000.0 * (f * np.exp(-te / 20.0) + (1.0 - f) * np.exp(-te / 80.0))
    data = s + 20.0 * rng.standard_normal(s.shape)
    mask = np.ones(shape, dtype=np.uint8)
    mask[0, 0, :] = 0
    return data, mask, te
