"""A numpy restatement of the 3-D Gibbs-ringing removal that include/met2_hip.h states for met2_degibbs3d (the 3-D split of Bautista,
O'Muircheartaigh, Hajnal, Tournier, ISMRM 2021, around the 1-D operator U of met2_degibbs), with numpy.fft.fftn: the reference of
tests/test_gpu_gibbs3d.py and tests/test_gibbs3d_host.py.  Written from the header, not from MRtrix; not fast.  U is gibbs_numpy's
unring_lines, unchanged.  Besides the output and the three shift maps it returns the three margin maps (the gap between the best and the
second-best shift's min(TVL, TVR) over max|echo volume|; below TIE another correct evaluation may choose another shift) and the split."""
import functools
import json
import os

import numpy as np

from gibbs_numpy import TIE, unring_lines, ld_dft_matrix, LD

AXES = ("x", "y", "z")


def axis_weights(n):
    """c = 1 + cos(2 pi p / n), exactly 0 at the Nyquist index of an even axis"""
    c = 1.0 + np.cos(2.0 * np.pi * np.arange(n) / n)
    if n % 2 == 0:
        c[n // 2] = 0.0
    return c


def weights_from(cx, cy, cz):
    """(Gx, Gy, Gz) [nx, ny, nz] from the three axes' c; where den == 0 the weight is shared evenly among the axes whose c is 0"""
    cx, cy, cz = cx[:, None, None], cy[None, :, None], cz[None, None, :]
    w = [cy * cz + 0 * cx, cx * cz + 0 * cy, cx * cy + 0 * cz]
    den = w[0] + w[1] + w[2]
    zero = den == 0
    safe = np.where(zero, 1, den)
    full = [np.broadcast_to(c == 0, den.shape) for c in (cx, cy, cz)]
    m = full[0].astype(int) + full[1].astype(int) + full[2].astype(int)
    one = den.dtype.type(1)
    return tuple(np.where(zero, np.where(f, one / np.maximum(m, 1).astype(den.dtype), 0), wa / safe) for f, wa in zip(full, w))


def split_weights3d(nx, ny, nz):
    return weights_from(axis_weights(nx), axis_weights(ny), axis_weights(nz))


def split3d(V):
    """the 3-D split of an echo volume: (Ix, Iy, Iz), each Re IDFT3(F Ga)"""
    F = np.fft.fftn(V)
    return tuple(np.real(np.fft.ifftn(F * g)) for g in split_weights3d(*V.shape))


def unring_axis(I, axis, nsh, minW, maxW, block=4096):
    """U along `axis` of I [nx, ny, nz] -> (out, shift int8, gap), the same shape; the lines in blocks to bound the memory"""
    moved = np.moveaxis(I, axis, -1)
    lines = np.ascontiguousarray(moved).reshape(-1, I.shape[axis])
    parts = [unring_lines(lines[i:i + block], nsh, minW, maxW) for i in range(0, lines.shape[0], block)]
    return tuple(np.moveaxis(np.concatenate([p[k] for p in parts]).reshape(moved.shape), -1, axis) for k in range(3))


def degibbs3d_volume(V, nsh=20, minW=1, maxW=3):
    """-> (out, shift_x, shift_y, shift_z, margin_x, margin_y, margin_z, Ix, Iy, Iz), all [nx, ny, nz]"""
    if not np.isfinite(V).all():
        z = np.zeros(V.shape, dtype=np.int8)
        inf = np.full(V.shape, np.inf)
        nan = np.full(V.shape, np.nan)
        return (V.copy(), z, z.copy(), z.copy(), inf, inf.copy(), inf.copy(), nan, nan.copy(), nan.copy())
    parts = split3d(V)
    done = [unring_axis(p, a, nsh, minW, maxW) for a, p in enumerate(parts)]
    scale = np.abs(V).max()
    scale = scale if scale > 0 else 1.0
    out = (done[0][0] + done[1][0]) + done[2][0]
    return (out,) + tuple(d[1] for d in done) + tuple(d[2] / scale for d in done) + parts


NAMES = ("out", "shift_x", "shift_y", "shift_z", "margin_x", "margin_y", "margin_z", "ix", "iy", "iz")


def degibbs3d(data, nsh=20, minW=1, maxW=3):
    """data [nx, ny, nz, nt] -> dict of NAMES, every echo volume on its own"""
    data = np.asarray(data, dtype=np.float64)
    nx, ny, nz, nt = data.shape
    if not (nsh >= 1 and 1 <= minW <= maxW and 2 * (maxW + 1) <= min(nx, ny, nz)):
        raise ValueError("bad parameters")
    res = {k: (np.zeros(data.shape, np.int8) if k.startswith("shift") else np.empty_like(data)) for k in NAMES}
    for e in range(nt):
        for k, p in zip(NAMES, degibbs3d_volume(data[..., e], nsh, minW, maxW)):
            res[k][..., e] = p
    return res


def ties(res):
    """the samples whose choice of shift, along any axis, this restatement itself calls a tie"""
    return (res["margin_x"] < TIE) | (res["margin_y"] < TIE) | (res["margin_z"] < TIE)


def min_margin(res):
    return float(min(res["margin_" + a].min() for a in AXES))


# The noise volumes: name -> (shape (nx, ny, nz, nt), seed, (nsh, minW, maxW)).  Every one is 100 + 5 N(0, 1) everywhere;
# tests/test_gibbs3d_host.py asserts that the restatement calls no sample of any of them a tie.
CASES = {
    "n8": ((8, 8, 8, 1), 101, (20, 1, 3)),             # the smallest shape: the windows wrap along all axes, every axis has a Nyquist bin
    "odd": ((9, 15, 11, 2), 102, (20, 1, 3)),          # no Nyquist bin; no axis, line count or plane a multiple of the kernels' tile of 8
    "mixed": ((16, 12, 10, 3), 103, (20, 1, 3)),
    "zwave": ((8, 9, 65, 2), 104, (20, 1, 3)),         # a z line crosses a wave; one even axis
    "z256": ((9, 8, 256, 1), 105, (20, 1, 3)),         # one z line per workgroup, the longest
    "z255": ((8, 8, 255, 1), 106, (20, 1, 3)),
    "x256": ((256, 8, 9, 1), 107, (20, 1, 3)),
    "y129": ((8, 129, 8, 1), 108, (20, 1, 3)),
    "cube33": ((33, 33, 33, 1), 109, (20, 1, 3)),
    "cube64": ((64, 64, 64, 1), 110, (20, 1, 3)),
    "params": ((16, 12, 10, 1), 111, (4, 2, 4)),
    "nsh32": ((12, 10, 16, 1), 112, (32, 1, 3)),       # nz = 16: the y pass's tiles of 8 z lines end with the axis
    "echoes37": ((8, 8, 8, 37), 113, (20, 1, 3)),      # more echoes than the gather's tile of 32; the distinct echoes of the seam volume
    # the tile edges of the passes along and across z
    "zlpb1": ((8, 9, 129, 1), 114, (20, 1, 3)),        # the first nz with one z line per workgroup of the line kernel
    "zlpb2": ((9, 8, 128, 1), 115, (20, 1, 3)),        # the last with two
    "zlpb23": ((8, 86, 85, 1), 116, (20, 1, 3)),       # two lines per workgroup along y, three along z
    "ztile17": ((8, 8, 17, 2), 117, (20, 1, 3)),       # one z line above two tiles of 8 in the DFT along y; ny nz = 136 = 17 tiles of the one along x
    "ztile15": ((8, 9, 15, 1), 118, (20, 1, 3)),       # one below; ny nz = 135, one short of 17 tiles
}


def case(name):
    """-> (data [nx, ny, nz, nt], (nsh, minW, maxW))"""
    shape, seed, params = CASES[name]
    return 100.0 + 5.0 * np.random.default_rng(seed).standard_normal(shape), params


@functools.lru_cache(maxsize=None)
def reference(name):
    """(data, (nsh, minW, maxW), the restatement's result) of a case: computed once per process, shared, not to be written to"""
    data, params = case(name)
    res = degibbs3d(data, *params)
    for a in (data,) + tuple(res.values()):
        a.setflags(write=False)
    return data, params, res


BALL_N, BALL_F, BALL_OFFSET = (40, 32, 24), 4, (0.31, -0.17, 0.23)


@functools.lru_cache(maxsize=None)
def ball_phantom():
    """A ball of 120 on 20, radius 0.3 of the field of view, drawn on a grid BALL_F times finer and cropped in k-space to BALL_N: a volume
    that rings along all three axes.  -> (image, truth, flat): the truth is the fine grid at the coarse positions; flat marks the voxels
    whose six periodic face neighbours equal them in the truth"""
    n, f, o = BALL_N, BALL_F, BALL_OFFSET
    N = tuple(f * k for k in n)
    ax = [(np.arange(Na) - Na / 2 - oa * f) / Na for Na, oa in zip(N, o)]
    r2 = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2
    fine = np.where(r2 <= 0.3 ** 2, 120.0, 20.0)
    F = np.fft.fftshift(np.fft.fftn(fine))
    lo = [Na // 2 - na // 2 for Na, na in zip(N, n)]
    block = F[lo[0]:lo[0] + n[0], lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]]
    img = np.real(np.fft.ifftn(np.fft.ifftshift(block))) / f ** 3
    truth = fine[::f, ::f, ::f].copy()
    flat = np.ones(n, dtype=bool)
    for a in range(3):
        for s in (1, -1):
            flat &= np.roll(truth, s, axis=a) == truth
    for a in (img, truth, flat):
        a.setflags(write=False)
    return img, truth, flat


@functools.lru_cache(maxsize=None)
def ball_reference():
    img, _, _ = ball_phantom()
    res = degibbs3d(img[..., None])
    for a in res.values():
        a.setflags(write=False)
    return res


def rms(a, b, where):
    return float(np.sqrt(np.mean((a[where] - b[where]) ** 2)))


def driver_volume3d():
    """gibbs_numpy's driver_volume enlarged to 8 along z"""
    from gibbs_numpy import driver_volume
    return driver_volume(shape=(12, 12, 8))


# ---- the split in extended precision, by dense DFTs built from gibbs_numpy's ld_dft_matrix (no numpy.fft)
def ld_apply(mr, mi, xr, xi, axis):
    """(mr + i mi) applied along `axis` of xr + i xi: out[.., q, ..] = sum_b m[b][q] x[.., b, ..]"""
    def along(m, x):
        return np.moveaxis(np.tensordot(m.T, x, axes=([1], [axis])), 0, axis)
    return along(mr, xr) - along(mi, xi), along(mr, xi) + along(mi, xr)


def ld_split3d(V):
    """-> (Ix, Iy, Iz) in np.longdouble"""
    V = np.asarray(V, dtype=LD)
    mats = [ld_dft_matrix(n) for n in V.shape]
    fr, fi = V, np.zeros_like(V)
    for a, (mr, mi) in enumerate(mats):
        fr, fi = ld_apply(mr, mi, fr, fi, a)
    cs = []
    for (mr, _), n in zip(mats, V.shape):
        c = 1 + mr[1]
        if n % 2 == 0:
            c[n // 2] = 0
        cs.append(c)
    parts = []
    for g in weights_from(*cs):
        br, bi = fr * g, fi * g
        for a, (mr, mi) in enumerate(mats):
            br, bi = ld_apply(mr, -mi, br, bi, a)
        parts.append(br / LD(V.size))
    return tuple(parts)


def record(name, figures):
    """with MET2_GIBBS3D_PARITY_JSON set, the GPU tests keep their measured deviations and smallest margins in that file
    (profiles/gibbs3d_parity.json is written this way)"""
    path = os.environ.get("MET2_GIBBS3D_PARITY_JSON")
    if not path:
        return
    table = json.load(open(path)) if os.path.exists(path) else {}
    table[name] = figures
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
