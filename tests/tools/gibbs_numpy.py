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


# The noise volumes the GPU tests compare on: name -> (shape, seed, (nsh, minW, maxW)).  Every one is 100 + 5 N(0, 1) everywhere (no flat regions);
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
    "full": ((256, 256, 1, 1), 9, (20, 1, 3)),        # one line per workgroup along both axes
    "lpb1": ((129, 10, 1, 2), 10, (20, 1, 3)),        # the first length with one line per workgroup
    "lpb2": ((128, 9, 1, 1), 11, (20, 1, 3)),         # the last with two
    "lpb23": ((86, 85, 1, 1), 12, (20, 1, 3)),        # two lines per workgroup along x, three along y
    "sq64": ((64, 64, 2, 1), 13, (20, 1, 3)),
    "n255": ((255, 8, 1, 1), 14, (20, 1, 3)),
    "tall": ((12, 20, 1, 3), 15, (20, 1, 3)),         # ny > nx, no multiple of the DFT kernels' row tile
    "wide7": ((16, 16, 1, 1), 16, (20, 1, 7)),        # the widest window that fits 16: every window index wraps
    "n9x8": ((9, 8, 1, 1), 17, (20, 1, 3)),
    "nsh1": ((16, 12, 1, 1), 18, (1, 1, 3)),          # 3 candidates: 4 of a pass's 7 lanes are padding
    "nsh3": ((16, 12, 1, 1), 19, (3, 2, 2)),          # exactly one pass, minW == maxW
    "seam37": ((8, 8, 37, 1), 20, (20, 1, 3)),        # the distinct slices of the 65537-slice seam volume
    "seam5": ((64, 64, 5, 1), 21, (20, 1, 3)),        # those of the 1025-slice one
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


def box_phantom(shape=(40, 24), seed=31):
    """noise inside a box, exactly 0.0 outside it"""
    nx, ny = shape
    img = np.zeros(shape)
    rng = np.random.default_rng(seed)
    img[nx // 4:3 * nx // 4, ny // 4:3 * ny // 4] = 100.0 + 5.0 * rng.standard_normal((3 * nx // 4 - nx // 4, 3 * ny // 4 - ny // 4))
    return img


SCALES = (1e-6, 1.0, 1e7)


def image_volume(name):
    """The volumes that are not noise all over, [nx, ny, nz, nt], default parameters: 'disc64', 'disc48' (disc_phantom), 'box' (box_phantom),
    'scales' (one noise slice times SCALES along the echoes), 'signed' (zero-mean noise)"""
    if name == "disc64":
        return disc_phantom()[0][:, :, None, None]
    if name == "disc48":
        return disc_phantom(n=48, N=384)[0][:, :, None, None]
    if name == "box":
        return box_phantom()[:, :, None, None]
    if name == "scales":
        S = 100.0 + 5.0 * np.random.default_rng(32).standard_normal((16, 12))
        return np.stack([S * f for f in SCALES], axis=-1)[:, :, None, :]
    if name == "signed":
        return 5.0 * np.random.default_rng(33).standard_normal((16, 12, 2, 1))
    raise KeyError(name)


IMAGES = ("disc64", "disc48", "box", "scales", "signed")


# ---- The stages in extended precision, formed directly from the header's formulas (a dense DFT and the cosine sums, no numpy.fft): the
# references of tests/test_gpu_gibbs_kernels.py.  np.longdouble is the x87 80-bit format where the platform has it (eps 1.1e-19); where it is
# float64 these are one more float64 route and the tests say so.
LD = np.longdouble
LD_IS_WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def ld_pi():
    return LD(4) * np.arctan(LD(1))


def ld_dft_matrix(n):
    """W[b][q] = exp(-2 pi i b q / n) -> (re, im), the angle reduced in integers"""
    k = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    ang = 2 * ld_pi() * k.astype(LD) / LD(n)
    return np.cos(ang), -np.sin(ang)


def ld_shift_kernels(n, nsh):
    """c[j][r] = (1 / n) sum_k' cos(2 pi k' (r + delta_j) / n), plus (1 / n) cos(pi r) for j = 0 and even n: [2 nsh + 1, n]"""
    sh = shift_table(nsh).astype(np.int64)
    r = np.arange(n, dtype=np.int64)
    num = r[None, :] * 2 * nsh + sh[:, None]                         # 2 pi k (r + delta) / n = pi k num / (nsh n)
    per = 2 * nsh * n
    c = np.ones((sh.size, n), dtype=LD)
    for k in range(1, (n - 1) // 2 + 1):
        c += 2 * np.cos(ld_pi() * ((k * num) % per).astype(LD) / LD(nsh * n))
    c /= LD(n)
    if n % 2 == 0:
        c[0] += np.where(r % 2 == 0, LD(1), LD(-1)) / LD(n)
    return c


def ld_split2d(S):
    """the 2-D split of a slice by dense DFTs -> (Ix, Iy, corner): corner the Nyquist-Nyquist term of even nx and ny, as an image (else 0)"""
    S = np.asarray(S, dtype=LD)
    nx, ny = S.shape
    xr, xi = ld_dft_matrix(nx)
    yr, yi = ld_dft_matrix(ny)
    tr, ti = S @ yr, S @ yi                                           # along y
    fr, fi = xr.T @ tr - xi.T @ ti, xr.T @ ti + xi.T @ tr             # along x
    cx = 1 + xr[1]
    cy = 1 + yr[1]
    if nx % 2 == 0:
        cx[nx // 2] = 0
    if ny % 2 == 0:
        cy[ny // 2] = 0
    den = cx[:, None] + cy[None, :]
    zero = den == 0
    gx = np.where(zero, LD(0), cy[None, :] / np.where(zero, LD(1), den))
    gy = np.where(zero, LD(0), cx[:, None] / np.where(zero, LD(1), den))
    corner = np.zeros_like(S)
    if nx % 2 == 0 and ny % 2 == 0:
        sign = np.where((np.arange(nx)[:, None] + np.arange(ny)[None, :]) % 2 == 0, LD(1), LD(-1))
        corner = fr[nx // 2, ny // 2] / LD(nx * ny) * sign

    def back(g):
        ar, ai = fr * g, fi * g
        br, bi = xr @ ar + xi @ ai, xr @ ai - xi @ ar                  # conj(W_x) F
        return (br @ yr.T + bi @ yi.T) / LD(nx * ny)                  # Re(. conj(W_y))
    return back(gx), back(gy), corner


def ld_shifted_lines(x, nsh, roll_of=None):
    """step 2 as the circular convolution with ld_shift_kernels: x [L, n] -> [L, 2 nsh + 1, n].  roll_of[l] = (l0, k) states that line l is
    line l0 rolled by k samples (np.roll(x[l0], k), checked); the convolution commutes with a roll, so its shifted lines are those of l0
    rolled by k: the same terms summed in another order, 1e-19 apart in this format, and n times less work at n steps of one shape."""
    x = np.asarray(x, dtype=LD)
    L, n = x.shape
    c = ld_shift_kernels(n, nsh)
    m = np.arange(n)
    out = np.empty((L, c.shape[0], n), dtype=LD)
    for l in range(L):
        if roll_of is not None and roll_of[l] is not None:
            l0, k = roll_of[l]
            assert l0 < l and roll_of[l0] is None and np.array_equal(x[l], np.roll(x[l0], k))
            out[l] = np.roll(out[l0], k, axis=-1)
        else:
            out[l] = c @ x[l][(m[None, :] - m[:, None]) % n]            # [r, m] = x[(m - r) mod n]
    return out


def ld_unring_lines(x, nsh=20, minW=1, maxW=3, roll_of=None):
    """the operator U in extended precision -> (out, shift int8, gap, best): unring_lines' three and the minimum of min(TVL, TVR)"""
    xs = ld_shifted_lines(x, nsh, roll_of)
    L, J, n = xs.shape
    sh = shift_table(nsh)
    d = np.abs(xs - np.roll(xs, 1, axis=-1))
    tvl = np.zeros_like(d)
    tvr = np.zeros_like(d)
    for t in range(minW, maxW + 1):
        tvl = tvl + np.roll(d, t, axis=-1)
        tvr = tvr + np.roll(d, -(t + 1), axis=-1)
    cand = np.stack([tvl, tvr], axis=2).reshape(L, 2 * J, n)
    js = np.argmin(cand, axis=1) // 2
    v = np.partition(np.minimum(tvl, tvr), 1, axis=1)[:, :2]         # the two smallest, in order
    pick = lambda a: np.take_along_axis(a, js[:, None, :], axis=1)[:, 0]
    a0, a1, a2 = pick(np.roll(xs, 1, axis=-1)), pick(xs), pick(np.roll(xs, -1, axis=-1))
    s = sh[js]
    dl = s.astype(LD) / LD(2 * nsh)
    out = np.where(dl > 0, a1 * (1 - dl) + a0 * dl, a1 * (1 + dl) - a2 * dl)
    return out, s.astype(np.int8), v[:, 1] - v[:, 0], v[:, 0]


# ---- The lines of the stage test of the operator U.
LINE_N = (8, 9, 16, 64, 65, 85, 86, 128, 129, 255, 256)
LINE_PARAMS = ((20, 1, 3), (1, 1, 3), (3, 2, 2), (4, 2, 4), (32, 1, 3))


def line_cases():
    """(n, (nsh, minW, maxW)) of every case of the stage test"""
    return [(n, p) for n in LINE_N for p in LINE_PARAMS if 2 * (p[2] + 1) <= n] + [(16, (20, 1, 7))]     # windows 2..4 need n >= 10


def noise_lines(n):
    """100 + 5 N(0, 1); two full workgroups of 256 / n lines and one line more"""
    return 100.0 + 5.0 * np.random.default_rng(1000 + n).standard_normal((2 * (256 // n) + 1, n))


def designed_lines(n):
    """-> (lines [L, n], index of the all-zero line, roll_of for ld_shifted_lines).  A step at every position m0 = 0..n-1 (x[m] = base + amp for the n // 2 samples from
    m0 on, periodically, base elsewhere: for m0 > n - n // 2 the plateau runs across the wrap; on a slow cosine of 3 % of the step and a second harmonic of 2 %, without
    which the line is mirror-symmetric and the two half-sample shifts tie exactly with shift 0 on the plateau), in enough copies with their own base and
    amplitude that the set holds at least 100 lines (so the all-zero line, a tie all along by definition, is under 1 % of the samples);
    then an impulse, a ramp with one jump, a step truncated in k-space to 3/4 of the band (it rings), and an all-zero line between two
    non-zero ones, all in one workgroup where a workgroup holds several lines; a last line so that L is no multiple of 256 / n."""
    m = np.arange(n)
    rows, roll_of = [], []
    reps = -(-100 // n)
    for k in range(reps):
        base, amp = 40.0 + 13.0 * k, (1.0 + 0.37 * k) * (-1.0) ** k
        for m0 in range(n):
            roll_of.append((k * n, m0) if m0 else None)
            rows.append(np.roll(base + amp * ((m < n // 2) + 0.03 * np.cos(2.0 * np.pi * m / n + 0.7 + k) + 0.02 * np.sin(4.0 * np.pi * m / n + 0.2)), m0))
    imp = 25.0 + 2.0 * np.cos(2.0 * np.pi * m / n + 0.3)            # not mirror-symmetric either
    imp[n // 3] += 80.0
    rows.append(imp)
    ramp = 10.0 + 0.75 * m + 30.0 * (m >= (2 * n) // 3)
    rows.append(ramp)
    step = 50.0 + 60.0 * ((m >= n // 4) & (m < n // 4 + n // 2)) + 3.0 * np.cos(2.0 * np.pi * m / n + 1.1)
    kk = np.abs(((m + n // 2) % n) - n // 2)                         # |signed frequency|
    X = np.fft.fft(step)
    X[kk > (3 * n) // 8] = 0.0
    rows.append(np.real(np.fft.ifft(X)))
    zero_at = len(rows)
    rows.append(np.zeros(n))
    rows.append(ramp[::-1].copy())
    lpb = 256 // n
    if len(rows) % lpb == 0 and lpb > 1:
        rows.append(imp[::-1] * 3.0)
    return np.array(rows), zero_at, roll_of + [None] * (len(rows) - len(roll_of))


import functools                                                   # noqa: E402


@functools.lru_cache(maxsize=None)
def line_reference(n, params, kind):
    """kind 'noise' or 'designed' -> dict(lines, zero_at (None for noise), out, shift, margin (the gap over max|line|, 1 for a zero line),
    best), extended precision, computed once per process and not to be written to"""
    if kind == "noise":
        lines, zero_at, roll_of = noise_lines(n), None, None
    else:
        lines, zero_at, roll_of = designed_lines(n)
    out, shift, gap, best = ld_unring_lines(lines, *params, roll_of=roll_of)
    scale = np.abs(lines).max(axis=1, keepdims=True)
    scale[scale == 0] = 1.0
    res = {"lines": lines, "out": out, "shift": shift, "margin": (gap / scale).astype(np.float64), "best": best, "scale": scale}
    for a in res.values():
        a.setflags(write=False)
    res["zero_at"] = zero_at
    return res


def record(name, figures):
    """with MET2_GIBBS_PARITY_JSON set, the GPU tests keep their measured deviations in that file (profiles/gibbs_parity.json was written
    this way)"""
    import json
    import os
    path = os.environ.get("MET2_GIBBS_PARITY_JSON")
    if not path:
        return
    table = json.load(open(path)) if os.path.exists(path) else {}
    table[name] = figures
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
