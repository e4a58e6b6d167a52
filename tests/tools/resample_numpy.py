"""The affine resampling of include/met2_hip.h (met2_resample, met2_resample_labels, met2_resample_prefilter), restated in numpy: vectorised,
in fp64 (dtype=np.float64: the operations of the header, each rounded once, in its order) or in long double (dtype=np.longdouble: the
reference the device is held against).  The coordinates, the inside test, the floors and the tap indices are fp64 in both -- they are the
contract, and the device reproduces them to the bit --; the weights, the sums and the prefilter run in `dtype`.
Volumes are [S, nx, ny, nz] (or [nx, ny, nz]); a transform is A [3, 4]: destination index -> continuous source coordinates."""
import numpy as np

Z1 = np.sqrt(3.0) - 2.0


def coords(A, shape):
    """-> c [3, mx, my, mz] fp64: c_a = ((A[a][3] + A[a][0] i) + A[a][1] j) + A[a][2] k"""
    A = np.asarray(A, dtype=np.float64)
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.stack([((A[a, 3] + A[a, 0] * i) + A[a, 1] * j) + A[a, 2] * k for a in range(3)])


def inside_map(A, src_shape, shape):
    c = coords(A, shape)
    ok = np.ones(tuple(shape), dtype=bool)
    for a in range(3):
        ok &= (c[a] >= 0.0) & (c[a] <= float(src_shape[a] - 1))
    return ok.astype(np.uint8)


def mirror(m, n):
    """taps m (ints) of a line of n samples, mirrored about the end samples by modulo"""
    m = np.asarray(m, dtype=np.int64)
    if n == 1:
        return np.zeros_like(m)
    P = 2 * (n - 1)
    m = np.mod(m, P)
    return np.where(m > n - 1, P - m, m)


def _axis(c, n, order, dtype):
    """per axis: (tap indices [N, ...], weights [N, ...]); c restricted to the inside voxels"""
    if order == 0:
        return [np.floor(c + 0.5).astype(np.int64)], [np.ones(c.shape, dtype=dtype)]
    f = np.floor(c)
    t = (c - f).astype(dtype)                     # exact in fp64
    f = f.astype(np.int64)
    one, three, four, six = dtype(1), dtype(3), dtype(4), dtype(6)
    if order == 1:
        return [f, mirror(f + 1, n)], [one - t, t]
    u = one - t
    w = [(u * u) * u / six, (((three * t - six) * t) * t + four) / six, (((three * u - six) * u) * u + four) / six, (t * t) * t / six]
    return [mirror(f - 1 + p, n) for p in range(4)], w


def prefilter(vol, dtype=np.float64):
    """the cubic B-spline coefficients of [..., nx, ny, nz], per axis x, y, z; a line of one sample is left as it is"""
    dtype = np.dtype(dtype).type
    c = np.array(vol, dtype=dtype)
    z = dtype(np.sqrt(dtype(3))) - dtype(2) if dtype is not np.float64 else np.float64(Z1)
    lam = (dtype(1) - z) * (dtype(1) - dtype(1) / z)
    for axis in (-3, -2, -1):
        n = c.shape[axis]
        if n == 1:
            continue
        x = np.moveaxis(c, axis, 0)                # a view: line samples along the first axis
        zn = z ** (n - 1) if dtype is not np.float64 else np.float64(float(z) ** (n - 1))
        s = lam * x                                # x_i = lambda s_i
        c0 = s[0] + zn * s[n - 1]
        p = z
        for i in range(1, n - 1):
            c0 = c0 + p * (s[i] + zn * s[n - 1 - i])
            p = p * z
        c0 = c0 / (dtype(1) - zn * zn)
        x[0] = c0
        for i in range(1, n):
            x[i] = s[i] + z * x[i - 1]
        x[n - 1] = (z * x[n - 2] + x[n - 1]) * (z / (z * z - dtype(1)))
        for i in range(n - 2, -1, -1):
            x[i] = z * (x[i + 1] - x[i])
    return c


def resample(vol, A, shape, order=1, cval=0.0, dtype=np.float64, return_inside=False):
    """vol [S, nx, ny, nz] or [nx, ny, nz] -> [S, mx, my, mz] or [mx, my, mz] in `dtype` (order 0: in vol's own dtype, so labels pass)"""
    dtype = np.dtype(dtype).type
    vol = np.asarray(vol)
    single = vol.ndim == 3
    v = vol[None] if single else vol
    src_shape = v.shape[1:]
    shape = tuple(int(n) for n in shape)
    c = coords(A, shape)
    ins = inside_map(A, src_shape, shape).astype(bool)
    out_dtype = vol.dtype if order == 0 else dtype
    out = np.full((v.shape[0],) + shape, cval, dtype=out_dtype)
    if ins.any():
        taps = [_axis(c[a][ins], src_shape[a], order, dtype) for a in range(3)]
        if order == 0:
            out[:, ins] = v[:, taps[0][0][0], taps[1][0][0], taps[2][0][0]]
        else:
            coef = prefilter(v, dtype) if order == 3 else v.astype(dtype)
            (ix, wx), (iy, wy), (iz, wz) = taps
            acc = None
            for p in range(len(ix)):
                for q in range(len(iy)):
                    wpq = wx[p] * wy[q]
                    for r in range(len(iz)):
                        term = (wpq * wz[r]) * coef[:, ix[p], iy[q], iz[r]]
                        acc = term if acc is None else acc + term
            out[:, ins] = acc
    out = out[0] if single else out
    return (out, ins.astype(np.uint8)) if return_inside else out


def resample_labels(labels, A, shape, fill=0):
    return resample(np.asarray(labels).astype(np.int32), A, shape, order=0, cval=fill)


# ---------------------------------------------------------------- the cases the tests share

SRC_DIMS = ((1, 1, 1), (2, 3, 4), (5, 1, 9), (9, 8, 7), (3, 4, 63), (3, 4, 64), (3, 4, 65), (4, 3, 129), (65, 4, 3), (4, 65, 3))
N_SERIES = (1, 3, 8, 9)
TRANSFORMS = ("identity", "shift", "flip", "half", "scale", "rotated", "outside")


def dst_dims(dims):
    """the destination grid the tests pair with a source grid: no multiple of a block, (1, 1, 1) once, larger than the source elsewhere
    but on one axis"""
    return {(1, 1, 1): (1, 1, 1), (2, 3, 4): (3, 2, 5)}.get(tuple(dims), (dims[0] + 2, max(dims[1] - 1, 1), dims[2] + 3))


def volume(rng, dims, n_series, vmax=100.0):
    """[S, nx, ny, nz]: smooth-ish random values of either sign, max |v| = vmax exactly"""
    v = rng.standard_normal((n_series,) + tuple(dims))
    return v * (vmax / np.abs(v).max())


def rotated(dims, shape):
    """a rotation with anisotropic scaling about the source's centre that takes the destination's centre there: part of the destination
    falls outside the source"""
    ax, ay = np.deg2rad(10.0), np.deg2rad(-7.0)
    Rz = np.array([[np.cos(ax), -np.sin(ax), 0], [np.sin(ax), np.cos(ax), 0], [0, 0, 1.0]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1.0, 0], [-np.sin(ay), 0, np.cos(ay)]])
    scale = np.array([(n - 1.0) / max(m - 1.0, 1.0) for n, m in zip(dims, shape)]) * np.array([1.1, 0.9, 1.05])
    M = Rz @ Ry @ np.diag(scale)
    cs, cd = (np.array(dims) - 1.0) / 2.0, (np.array(shape) - 1.0) / 2.0
    return np.column_stack([M, cs - M @ cd])


def transforms(dims, shape):
    """name -> A for a source of `dims` and a destination of `shape` (the transforms every GPU test runs)"""
    nx = dims[0]
    out = {
        "identity": np.column_stack([np.eye(3), np.zeros(3)]),
        "shift": np.column_stack([np.eye(3), np.array([1.0, 0.0, -2.0])]),
        "flip": np.column_stack([np.diag([-1.0, 1.0, 1.0]), np.array([nx - 1.0, 0.0, 0.0])]),
        "half": np.column_stack([np.eye(3), np.array([0.5, 0.5, 0.5])]),
        "scale": np.column_stack([0.5 * np.eye(3), np.zeros(3)]),
        "rotated": rotated(dims, shape),
        "outside": np.column_stack([np.eye(3), np.array([-1000.0, 0.0, 0.0])]),
    }
    return out


# ---------------------------------------------------------------- the cases of tests/test_gpu_resample_edges.py (and of its host checks)

EDGE_N_SERIES = (4, 5, 31, 32, 33, 48, 60, 64, 65, 120)          # echo data holds 32 or 48 series, spectra 60 or 120
EDGE_DIMS = ((9, 8, 7), (3, 4, 65))                               # 504 voxels: 7 voxel tiles of 64 and one of 56; a z line of the wave width plus one
EDGE_TRANSFORMS = ("rotated", "half")
GATHER_DIMS = ((2, 3, 4), (4, 4, 4), (5, 13, 1), (9, 8, 7))       # 24 voxels (one partial voxel tile), 64 (one full), 65 with nz = 1 (no z pass), 504
CHUNK_SERIES = (33, 40)                                           # order-3 chunks of 120 series: 33 + 33 + 33 + 21 and 40 + 40 + 40
STRIDE_N_SERIES = (5, 33)
LONG_AXES = (("nz512", (2, 2, 512), (1, 4)), ("nx512", (512, 2, 2), (1, 4)), ("ny512", (2, 512, 2), (1, 4)),
             ("nz125", (5, 13, 125), (1,)), ("nz126", (5, 13, 126), (1,)))
LONG_TRANSFORMS = ("half", "scale")
MIN_INSIDE = 200                                                  # inside voxels every resampling case must have (and one outside at least)

GATHER_TILE_V, GATHER_TILE_S, Z_LDS_DOUBLES = 64, 32, 8064        # RS_TILE_V, RS_TILE_S, RS_Z_LDS_DOUBLES of met2_resample.hip


def group_width(n_series):
    """lanes per voxel of rs_group_kernel: min(64, the next power of two >= max(n_series, 4))"""
    g = 4
    while g < 64 and g < n_series:
        g *= 2
    return g


def group_turns(n_series):
    """turns of rs_group_kernel's loop over the series"""
    return -(-n_series // group_width(n_series))


def series_tiles(n_series):
    """(series tiles of rs_gather_kernel<true>, series in the last one)"""
    n = -(-n_series // GATHER_TILE_S)
    return n, n_series - (n - 1) * GATHER_TILE_S


def z_tiles(nz, lines):
    """(lines of a tile of rs_prefilter_z_kernel, tiles, lines in the last one)"""
    t = min(64, Z_LDS_DOUBLES // (nz | 1))
    n = -(-lines // t)
    return t, n, lines - (n - 1) * t


def edge_volume(dims, n_series):
    """the source of an edge case: the same values wherever the case is computed"""
    return volume(np.random.default_rng(list(dims) + [n_series, 61]), dims, n_series)
