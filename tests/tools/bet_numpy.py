"""numpy restatement of the brain extraction (met2_brain_mask in include/met2_hip.h: the surface model of Smith, Fast robust automated brain
extraction, HBM 2002, without the self-intersection retry pass), written from the header's text step by step: the reference of
tests/test_gpu_bet.py, checked on its own by tests/test_bet_host.py.  dtype=np.longdouble runs the floating-point sums of the statistics and
the whole surface evolution in long double (the thresholds, which the header defines in fp64, and the fill stay fp64), to show how far
rounding moves a result.  Also the phantom the tests run on and the table of committed cases."""
import functools
import math

import numpy as np

NBINS = 1000
RMIN, RMAX = 3.33, 10.0
D1, D2 = 20, 10                       # depth in mm of the search for Imin and for Imax
L_EVERY = 50
STAT_KEYS = ("t2", "t", "t98", "tm", "cx", "cy", "cz", "r")


# ---------------------------------------------------------------- mesh
@functools.lru_cache(maxsize=None)
def icosphere(level):
    """-> (unit vertices [nv, 3], triangles [nt, 3] int32, ring [nv, 6] int32 padded with -1, deg [nv] int32)"""
    phi = (1.0 + math.sqrt(5.0)) / 2.0
    base = [(-1, phi, 0), (1, phi, 0), (-1, -phi, 0), (1, -phi, 0), (0, -1, phi), (0, 1, phi), (0, -1, -phi), (0, 1, -phi),
            (phi, 0, -1), (phi, 0, 1), (-phi, 0, -1), (-phi, 0, 1)]
    tris = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
            (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]

    def unit(p):
        x, y, z = float(p[0]), float(p[1]), float(p[2])
        n = math.sqrt((x * x + y * y) + z * z)
        return (x / n, y / n, z / n)

    verts = [unit(p) for p in base]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p, q = verts[key[0]], verts[key[1]]
                verts.append(unit(((p[0] + q[0]) * 0.5, (p[1] + q[1]) * 0.5, (p[2] + q[2]) * 0.5)))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in tris:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tris = out
    nv = len(verts)
    succ = [dict() for _ in range(nv)]
    for a, b, c in tris:
        succ[a][b] = c
        succ[b][c] = a
        succ[c][a] = b
    ring = np.full((nv, 6), -1, dtype=np.int32)
    deg = np.zeros(nv, dtype=np.int32)
    for i in range(nv):
        p = min(succ[i])
        for k in range(len(succ[i])):
            ring[i, k] = p
            p = succ[i][p]
        deg[i] = len(succ[i])
    out = (np.array(verts, dtype=np.float64), np.array(tris, dtype=np.int32), ring, deg)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- echo mean and statistics
def echo_mean(data):
    """[nx,ny,nz,nt] -> the echoes added one by one in ascending order from the first, divided by nt"""
    data = np.asarray(data, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        s = data[..., 0].copy()
        for e in range(1, data.shape[-1]):
            s = s + data[..., e]
        return s / float(data.shape[-1])


def stats(v, vox, dtype=np.float64):
    """-> dict of STAT_KEYS (float64), 'count' = |{v > t}|, 'n_tm' = the size of the set the median is taken of"""
    v = np.asarray(v, dtype=np.float64)
    fin = np.isfinite(v)
    N = int(fin.sum())
    if N == 0:
        raise ValueError("no finite voxel")
    vf = v[fin]
    lo, hi = float(vf.min()), float(vf.max())
    if not hi > lo:
        raise ValueError("empty v > t set")
    b = np.minimum(np.floor((vf - lo) / (hi - lo) * float(NBINS)).astype(np.int64), NBINS - 1)
    C = np.cumsum(np.bincount(b, minlength=NBINS))
    j2, j98 = int(np.argmax(100 * C >= 2 * N)), int(np.argmax(100 * C >= 98 * N))
    binw = (hi - lo) / float(NBINS)
    t2, t98 = lo + float(j2) * binw, lo + float(j98 + 1) * binw
    t = t2 + 0.1 * (t98 - t2)
    vv = np.where(fin, v, -np.inf)
    sel = vv > t
    count = int(sel.sum())
    if count == 0:
        raise ValueError("empty v > t set")
    ix, iy, iz = np.nonzero(sel)
    w = (np.minimum(v[sel], t98) - t2).astype(dtype)
    sw = w.sum()
    cog = [float((w * (i.astype(np.float64) * float(d)).astype(dtype)).sum() / sw) for i, d in zip((ix, iy, iz), vox)]
    vol = float(count) * ((float(vox[0]) * float(vox[1])) * float(vox[2]))
    r = float(np.cbrt(3.0 * vol / (4.0 * math.pi)))
    gx, gy, gz = np.meshgrid(*[np.arange(n, dtype=np.float64) * float(d) for n, d in zip(v.shape, vox)], indexing="ij", sparse=True)
    dx, dy, dz = gx - cog[0], gy - cog[1], gz - cog[2]
    inside = ((dx * dx + dy * dy) + dz * dz) <= r * r
    med = inside & (vv > t2) & (vv < t98)
    tm = float(np.median(v[med])) if med.any() else t
    return {"t2": t2, "t": t, "t98": t98, "tm": tm, "cx": cog[0], "cy": cog[1], "cz": cog[2], "r": r, "count": count, "n_tm": int(med.sum())}


def stats_vector(st):
    return np.array([st[k] for k in STAT_KEYS], dtype=np.float64)


# ---------------------------------------------------------------- surface evolution
def start_vertices(st, level):
    unit = icosphere(level)[0]
    c = np.array([st["cx"], st["cy"], st["cz"]])
    return c[None, :] + unit * (0.5 * st["r"])


def evolve(v, vox, st, verts, level, f=0.4, n_iter=1000, dtype=np.float64):
    """n_iter Jacobi steps from `verts` [nv, 3] -> the vertices in `dtype`"""
    v = np.asarray(v, dtype=np.float64)
    _, _, ring, deg = icosphere(level)
    T = dtype
    X = np.array(verts, dtype=T)
    nv = X.shape[0]
    valid = ring >= 0
    R = np.where(valid, ring, 0)
    nxt = (np.arange(6)[None, :] + 1) % deg[:, None]
    degT = deg.astype(T)
    vflat = np.where(np.isfinite(v), v, 0.0).reshape(-1)
    dims = [T(n) for n in v.shape]
    wT = (1.0 / np.array(vox, dtype=np.float64)).astype(T)            # the reciprocals are rounded to fp64
    t2, t, tm = T(st["t2"]), T(st["t"]), T(st["tm"])
    E = T((1.0 / RMIN + 1.0 / RMAX) / 2.0)
    F = T(6.0 / (1.0 / RMIN - 1.0 / RMAX))
    bt = T(float(f) ** 0.275)
    rows = np.arange(nv)
    depth = np.arange(1, D1 + 1).astype(T)
    l = T(0)
    for it in range(int(n_iter)):
        D = X[R] - X[:, None, :]                                   # [nv, 6, 3]
        if it % L_EVERY == 0:
            dist = np.sqrt((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2])
            l = np.where(valid, dist, T(0)).sum() / T(int(deg.sum()))
        nr = np.zeros((nv, 3), dtype=T)
        sm = np.zeros((nv, 3), dtype=T)
        a, b = D, D[rows[:, None], nxt, :]
        cr = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                       a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=2)
        cr = np.where(valid[..., None], cr, T(0))
        nb = np.where(valid[..., None], X[R], T(0))
        for k in range(6):                                          # in ring order
            nr = nr + cr[:, k, :]
            sm = sm + nb[:, k, :]
        nl = np.sqrt((nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2])
        n = np.where(nl[:, None] > 0, nr / np.where(nl > 0, nl, T(1))[:, None], T(0))
        s = sm / degT[:, None] - X
        sd = (s[:, 0] * n[:, 0] + s[:, 1] * n[:, 1]) + s[:, 2] * n[:, 2]
        sn = sd[:, None] * n
        st_ = s - sn
        f2 = (T(1) + np.tanh(F * (T(2) * np.abs(sd) / (l * l) - E))) * T(0.5)
        p = X[:, None, :] - depth[None, :, None] * n[:, None, :]    # [nv, 20, 3]: the points at d = 1 .. 20 mm
        fa = np.floor(p * wT + T(0.5))
        fx, fy, fz = fa[..., 0], fa[..., 1], fa[..., 2]
        inb = (fx >= 0) & (fx < dims[0]) & (fy >= 0) & (fy < dims[1]) & (fz >= 0) & (fz < dims[2])      # false for a NaN
        flat = np.where(inb, (fx * dims[1] + fy) * dims[2] + fz, T(0)).astype(np.int64)                  # exact: below 2^31
        I = np.where(inb, vflat[flat], 0.0).astype(T)
        imin = np.maximum(t2, np.minimum(tm, I.min(axis=1)))
        imax = np.minimum(tm, np.maximum(t, I[:, :D2].max(axis=1)))
        den = imax - t2
        tl = den * bt + t2
        f3 = np.where(den > 0, T(2) * (imin - tl) / np.where(den > 0, den, T(1)), T(0))
        X = ((X + T(0.5) * st_) + f2[:, None] * sn) + ((T(0.05) * f3) * l)[:, None] * n
    return X


# ---------------------------------------------------------------- fill
def fill(verts, tris, shape, vox, return_crossings=False):
    """-> uint8 mask [nx,ny,nz] (and the number of crossings of every column)"""
    verts = np.asarray(verts, dtype=np.float64)
    nx, ny, nz = shape
    dx, dy, dz = (float(d) for d in vox)
    tog = np.zeros((nx, ny, nz), dtype=np.int64)
    cross = np.zeros((nx, ny), dtype=np.int64)
    nv = verts.shape[0]
    for tri in np.asarray(tris):
        if tri.min() < 0 or tri.max() >= nv:
            continue
        P = verts[tri]
        if not np.all(np.isfinite(P)):
            x0, x1, y0, y1 = 0, nx - 1, 0, ny - 1
        else:
            x0, x1 = max(int(math.floor(P[:, 0].min() / dx)) - 1, 0), min(int(math.ceil(P[:, 0].max() / dx)) + 1, nx - 1)
            y0, y1 = max(int(math.floor(P[:, 1].min() / dy)) - 1, 0), min(int(math.ceil(P[:, 1].max() / dy)) + 1, ny - 1)
        if x0 > x1 or y0 > y1:
            continue
        px = (np.arange(x0, x1 + 1, dtype=np.float64) * dx)[:, None]
        py = np.arange(y0, y1 + 1, dtype=np.float64) * dy
        c, xs, zs = [], [], []
        for e in range(3):
            i, j = int(tri[e]), int(tri[(e + 1) % 3])
            p, q = (verts[i], verts[j]) if i < j else (verts[j], verts[i])
            ce = (p[1] <= py) != (q[1] <= py)
            den = np.where(ce, q[1] - p[1], 1.0)
            with np.errstate(invalid="ignore", over="ignore"):
                xs.append(p[0] + ((py - p[1]) * (q[0] - p[0])) / den)
                zs.append(p[2] + ((py - p[1]) * (q[2] - p[2])) / den)
            c.append(ce)
        any_ = c[0] | c[1] | c[2]
        xa, za = np.where(c[0], xs[0], xs[1]), np.where(c[0], zs[0], zs[1])
        xb, zb = np.where(c[2], xs[2], xs[1]), np.where(c[2], zs[2], zs[1])
        ra, rb = xa[None, :] > px, xb[None, :] > px
        ins = any_[None, :] & (ra != rb)
        if not ins.any():
            continue
        xl, zl = np.where(ra, xb[None, :], xa[None, :]), np.where(ra, zb[None, :], za[None, :])
        xr, zr = np.where(ra, xa[None, :], xb[None, :]), np.where(ra, za[None, :], zb[None, :])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            zc = zl + ((px - xl) * (zr - zl)) / np.where(ins, xr - xl, 1.0)
            m = np.ceil(zc / dz)
        gi, gj = np.nonzero(ins)
        mm = m[gi, gj]
        cross[gi + x0, gj + y0] += 1
        keep = mm >= 1.0                                            # a NaN keeps nothing
        k = np.minimum(mm[keep], float(nz)).astype(np.int64) - 1
        tog[gi[keep] + x0, gj[keep] + y0, k] += 1
    mask = (np.cumsum(tog[:, :, ::-1], axis=2)[:, :, ::-1] % 2).astype(np.uint8)
    return (mask, cross) if return_crossings else mask


def brain_mask(v, vox, f=0.4, level=4, n_iter=1000, dtype=np.float64):
    """the whole of met2_brain_mask -> dict(mask, vertices (dtype), stats)"""
    st = stats(v, vox, dtype)
    X = evolve(v, vox, st, start_vertices(st, level), level, f, n_iter, dtype)
    mask = fill(np.asarray(X, dtype=np.float64), icosphere(level)[1], np.shape(v), vox)
    return {"mask": mask, "vertices": X, "stats": st}


# ---------------------------------------------------------------- phantom and cases
def phantom(shape=(64, 72, 56), vox=(3.0, 3.0, 3.0), seed=0, shell=7.0, offset=(0.37, -0.41, 0.23)):
    """Nested ellipsoids about a centre `offset` voxels off the middle of the volume: brain about 1000 with a smooth +-15 % modulation, a dark
    gap of `shell` mm at 80, a scalp of `shell` mm at 700, nothing outside; Gaussian noise of sigma 15, folded.  The scalp's outer
    semi-axes are 0.88 of the volume's half extent.  -> (v, labels: 1 brain, 2 gap, 3 scalp, 0 outside)"""
    rng = np.random.default_rng(seed)
    half = [0.5 * (n - 1) * d for n, d in zip(shape, vox)]
    ctr = [h + o * d for h, o, d in zip(half, offset, vox)]
    g = np.meshgrid(*[np.arange(n) * float(d) - c for n, d, c in zip(shape, vox, ctr)], indexing="ij")
    q = lambda shrink: sum((x / (0.88 * h - shrink)) ** 2 for x, h in zip(g, half))
    lab = np.zeros(shape, dtype=np.uint8)
    lab[q(0.0) <= 1.0] = 3
    lab[q(shell) <= 1.0] = 2
    lab[q(2.0 * shell) <= 1.0] = 1
    mod = 0.15 * np.sin(2.0 * np.pi * g[0] / (4.0 * half[0]) + 0.7) * np.cos(2.0 * np.pi * g[1] / (3.0 * half[1])) * np.cos(2.0 * np.pi * g[2] / (5.0 * half[2]) - 0.4)
    v = np.select([lab == 1, lab == 2, lab == 3], [1000.0 * (1.0 + mod), 80.0, 700.0], 0.0)
    v = np.abs(v + 15.0 * rng.standard_normal(shape))
    return v, lab


# the whole filter: name -> phantom arguments and the filter's parameters ('default' runs the defaults: level 4, 1000 iterations, f = 0.4)
CASES = {
    "small": dict(shape=(40, 44, 36), vox=(3.0, 3.0, 3.0), seed=1, level=3, n_iter=300),
    "aniso": dict(shape=(45, 41, 23), vox=(3.0, 3.0, 5.0), seed=2, level=3, n_iter=200),
    "default": dict(shape=(64, 72, 56), vox=(3.0, 3.0, 3.0), seed=3, level=4, n_iter=1000),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (v, labels, vox, dict(level, n_iter, f))"""
    c = CASES[name]
    v, lab = phantom(c["shape"], c["vox"], c["seed"], c.get("shell", 7.0))
    v.setflags(write=False)
    lab.setflags(write=False)
    return v, lab, c["vox"], {"level": c["level"], "n_iter": c["n_iter"], "f": c.get("f", 0.4)}


# the evolution alone, from start vertices the caller chooses: name -> (volume, level, n_iter, start).  Volumes: 'small' and 'aniso' above,
# 'mm1' (1 mm voxels, shells of 2 mm), 'flat' (z spans 12 mm: every search leaves the volume).  start: None = the sphere (COG, r / 2);
# (cx, cy, cz, radius) in mm otherwise -- 'outside' puts 28 % of the sphere's vertices beyond the volume's x = 0 face
# (a start on round numbers, (8, 10, 100) mm with radius 30, put samples on rounding boundaries: fp64 and long double parted by 0.04 mm).
EVOLVE_VOLUMES = {
    "small": dict(shape=(40, 44, 36), vox=(3.0, 3.0, 3.0), seed=1),
    "aniso": dict(shape=(45, 41, 23), vox=(3.0, 3.0, 5.0), seed=2),
    "mm1": dict(shape=(48, 53, 44), vox=(1.0, 1.0, 1.0), seed=4, shell=2.0),
    "flat": dict(shape=(40, 44, 5), vox=(3.0, 3.0, 3.0), seed=5),
}
EVOLVE_CASES = {
    "l0_n1": ("small", 0, 1, None), "l0_n51": ("small", 0, 51, None),
    "l1_n50": ("aniso", 1, 50, None),
    "l3_n0": ("aniso", 3, 0, None), "l3_n1": ("aniso", 3, 1, None), "l3_n49": ("aniso", 3, 49, None), "l3_n50": ("aniso", 3, 50, None),
    "l3_n51": ("aniso", 3, 51, None),
    "l4_n0": ("small", 4, 0, None), "l4_n1": ("small", 4, 1, None), "l4_n51": ("small", 4, 51, None), "l4_aniso_n50": ("aniso", 4, 50, None),
    "mm1_l3_n51": ("mm1", 3, 51, None), "mm1_l4_n49": ("mm1", 4, 49, None),
    "flat_l3_n51": ("flat", 3, 51, None),
    "outside_l3_n51": ("small", 3, 51, (15.5, 60.2, 50.1, 35.0)),
}


@functools.lru_cache(maxsize=None)
def evolve_volume(name):
    c = EVOLVE_VOLUMES[name]
    v, _ = phantom(c["shape"], c["vox"], c["seed"], c.get("shell", 7.0))
    v.setflags(write=False)
    return v, c["vox"], stats(v, c["vox"])


@functools.lru_cache(maxsize=None)
def evolve_case(name):
    """-> (v, vox, stats, level, n_iter, start vertices)"""
    vol, level, n_iter, start = EVOLVE_CASES[name]
    v, vox, st = evolve_volume(vol)
    if start is None:
        X0 = start_vertices(st, level)
    else:
        X0 = np.array(start[:3])[None, :] + icosphere(level)[0] * start[3]
    X0.setflags(write=False)
    return v, vox, st, level, n_iter, X0


@functools.lru_cache(maxsize=None)
def evolve_reference(name):
    """-> (the restatement's vertices in fp64, max |fp64 - long double| over the vertices' coordinates)"""
    v, vox, st, level, n_iter, X0 = evolve_case(name)
    a = evolve(v, vox, st, X0, level, 0.4, n_iter)
    b = evolve(v, vox, st, X0, level, 0.4, n_iter, dtype=np.longdouble)
    a.setflags(write=False)
    return a, float(np.abs(a.astype(np.longdouble) - b).max())


# fill alone: name -> (vertices, triangles, shape, vox)
def fill_case(name):
    unit, tris, _, _ = icosphere(2)
    if name == "sphere":                                            # centre off the grid, radius 10.3 mm
        return unit * 10.3 + np.array([15.2, 14.9, 16.1]), tris, (31, 29, 33), (1.0, 1.0, 1.0)
    if name == "on_centre":                                         # vertex 0 moved onto the column of voxel (7, 9): x = 14 mm, y = 13.5 mm
        X = unit * 9.0 + np.array([15.0, 16.0, 20.0])
        X = X + (np.array([14.0, 13.5, X[0, 2]]) - X[0]) * (np.arange(X.shape[0]) == 0)[:, None]
        return X, tris, (17, 23, 14), (2.0, 1.5, 3.0)
    if name == "on_grid":                                           # an octahedron-like level 0 mesh with every vertex on voxel centres' columns
        X = np.round(icosphere(0)[0] * 6.0) + np.array([8.0, 8.0, 8.0])
        return X, icosphere(0)[1], (17, 17, 17), (1.0, 1.0, 1.0)
    if name == "nx1":
        return unit * 6.0 + np.array([0.2, 7.3, 6.6]), tris, (1, 15, 14), (1.0, 1.0, 1.0)
    if name == "ny1":
        return unit * 6.0 + np.array([7.3, -0.3, 6.6]), tris, (67, 1, 13), (0.25, 1.0, 1.0)
    if name == "nz1":
        return unit * 6.0 + np.array([7.3, 6.6, 0.4]), tris, (15, 14, 1), (1.0, 1.0, 1.0)
    if name == "nz65":
        return unit * 7.7 + np.array([4.1, 3.3, 8.2]), tris, (9, 7, 65), (1.0, 1.0, 0.25)
    if name == "outside":                                           # part of the surface beyond every face of the volume
        return unit * 14.0 + np.array([3.0, 18.0, 9.5]), tris, (13, 21, 19), (1.0, 1.0, 1.0)
    raise KeyError(name)


FILL_CASES = ("sphere", "on_centre", "on_grid", "nx1", "ny1", "nz1", "nz65", "outside")
