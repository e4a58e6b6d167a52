"""A numpy restatement of the partial-volume maps that include/met2_hip.h states for met2_partial_volume (the mixel model of Santago & Gage
1993 as Shattuck et al. 2001 and Tohka et al. 2004 use it: pure types and mixtures of rank-adjacent classes, the mixtures' likelihood
marginalised over a uniform fraction by a 64-node midpoint rule, a Potts-like prior over the six face neighbours, types by iterated
conditional modes, Tohka's closed-form fraction): the reference of tests/test_gpu_pve.py.  Written from the header, step by step; not fast.
Every function works in the dtype of what it is handed, so `dtype=np.longdouble` runs every step in extended precision.  The stage functions
take the constants (mu, a, h, live, table) as arguments, so a stage test can hand them the device's.  Types are uint8 volumes: 0..K-1 pure,
K + j the mixture of classes j and j + 1, OFF off the domain.  case(name) makes the seeded test inputs, phantom() a volume whose true tissue
fractions are known."""
import functools

import numpy as np

import seg_numpy as sn

OFF = 255
N_NODES = 64
CHUNK = 1024


def n_types(K):
    return 2 * int(K) - 1


# ---- step 1 ----

def chunk_sums(values):
    """seg.chunk_sums in the dtype of `values`: the sums over chunks of 1024 consecutive entries of values [..., N] -> [..., np], in the order
    a first-stage kernel adds them (include/met2_hip.h, met2_bias_em)"""
    values = np.asarray(values)
    lead, m = values.shape[:-1], values.shape[-1]
    npart = -(-max(m, 1) // CHUNK)
    p = np.zeros(lead + (npart * CHUNK,), dtype=values.dtype)
    p[..., :m] = values
    p = p.reshape(lead + (npart, 4, 256))
    a = np.zeros(lead + (npart, 256), dtype=values.dtype)
    for j in range(4):
        a = a + p[..., j, :]
    a = a.reshape(lead + (npart, 4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lane ^ o]
    w = a[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def partial_sum(part):
    """bias.partial_sum in the dtype of `part`: the second stage's sum of the partials part [..., np]"""
    part = np.asarray(part)
    lead, m = part.shape[:-1], part.shape[-1]
    rows = -(-max(m, 1) // 256)
    p = np.zeros(lead + (rows * 256,), dtype=part.dtype)
    p[..., :m] = part
    p = p.reshape(lead + (rows, 256))
    a = np.zeros(lead + (256,), dtype=part.dtype)
    for r in range(rows):
        a = a + p[..., r, :]
    a = a.reshape(lead + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lane ^ o]
    w = a[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def moments(v, seg, prob, dtype=np.float64):
    """step 1 -> dict(mu, var, pi [K]; part [3, K, np]: the chunks' sums of p_k, p_k v, (p_k d) d; N)"""
    om = np.asarray(seg) != 0
    u = np.asarray(v)[om].astype(dtype)                              # memory order
    p = np.asarray(prob)[:, om].astype(dtype)
    N = u.size
    zero = np.dtype(dtype).type(0.0)
    p01 = chunk_sums(np.stack([p, p * u[None, :]]))
    s, a = partial_sum(p01[0]), partial_sum(p01[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.where(s == 0, zero, a / s)
        d = u[None, :] - mu[:, None]
        p2 = chunk_sums((p * d) * d)
        q = partial_sum(p2)
        var = np.where(s == 0, zero, q / s)
        pi = np.where(s == 0, zero, s / np.dtype(dtype).type(max(N, 1)))
    return {"mu": mu, "var": var, "pi": pi, "part": np.concatenate([p01, p2[None]]), "N": N}


# ---- steps 2 and 3 ----

def consts(mu, var, pi, dtype=np.float64):
    """-> (a [K], h [K], live [2K-1] bool, table [K-1, 64, 3] = (m, a, h) per node); the entries of a dead class or mixture are 0"""
    dt = np.dtype(dtype).type
    mu, var, pi = (np.asarray(x).astype(dtype) for x in (mu, var, pi))
    K = len(mu)
    lk = (pi != 0) & np.isfinite(var) & (var > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(lk, dt(1.0) / (dt(2.0) * var), dt(0.0))
        h = np.where(lk, dt(0.5) * np.log(np.where(lk, var, dt(1.0))), dt(0.0))
    al = (np.arange(N_NODES).astype(dtype) + dt(0.5)) / dt(N_NODES)
    be = dt(1.0) - al
    live = np.zeros(n_types(K), dtype=bool)
    live[:K] = lk
    tab = np.zeros((max(K - 1, 0), N_NODES, 3), dtype=dtype)
    for j in range(K - 1):
        with np.errstate(invalid="ignore"):
            live[K + j] = lk[j] and lk[j + 1] and bool(mu[j + 1] - mu[j] > 0)
        if live[K + j]:
            s = (al * al) * var[j] + (be * be) * var[j + 1]
            tab[j, :, 0] = al * mu[j] + be * mu[j + 1]
            tab[j, :, 1] = dt(1.0) / (dt(2.0) * s)
            tab[j, :, 2] = dt(0.5) * np.log(s)
    return a, h, live, tab


# ---- steps 4 and 5 ----

def energies(v, om, mu, a, h, live, tab):
    """E [2K-1] + v.shape in v's dtype: 0 off the domain, +inf for a dead type; every operation rounded once, in the header's order"""
    K = len(mu)
    u = v[om]
    dt = v.dtype.type
    E = np.zeros((n_types(K),) + v.shape, dtype=v.dtype)
    for k in range(K):
        d = u - mu[k]
        E[k][om] = (d * d) * a[k] + h[k] if live[k] else np.inf
    for j in range(K - 1):
        if not live[K + j]:
            E[K + j][om] = np.inf
            continue
        d = u[:, None] - tab[j, :, 0][None, :]
        q = (d * d) * tab[j, :, 1][None, :] + tab[j, :, 2][None, :]
        qs = q.min(axis=1)
        S = np.zeros(u.shape, dtype=v.dtype)
        for m in range(N_NODES):                                     # m ascending
            S = S + np.exp(qs - q[:, m])
        E[K + j][om] = qs - np.log(S * dt(1.0 / N_NODES))
    return E


def init_types(E, om, live, seg):
    """step 5"""
    typ = np.full(om.shape, OFF, dtype=np.uint8)
    if not np.any(live):
        typ[om] = np.asarray(seg)[om] - 1
        return typ
    typ[om] = np.argmin(np.where(np.asarray(live)[:, None], E[:, om], np.inf), axis=0)
    return typ


# ---- step 6 ----

def member_sets(K):
    """bit k of entry t: class k is a member of type t"""
    return np.array([1 << t for t in range(K)] + [3 << j for j in range(K - 1)], dtype=np.int64)


def delta2_table(K):
    """[T, T]: 0 for equal types, 1 when their member sets intersect, 2 otherwise"""
    m = member_sets(K)
    d = np.where((m[:, None] & m[None, :]) != 0, 1, 2)
    d[np.arange(len(m)), np.arange(len(m))] = 0
    return d


def neighbour_counts(typ, K):
    """c [3, T] + typ.shape: per axis and type t the sum of delta2(t, the neighbour's type) over the domain neighbours inside the volume"""
    T = n_types(K)
    look = np.zeros((T, 256), dtype=np.int64)
    look[:, :T] = delta2_table(K)
    L = np.pad(typ, 1, constant_values=OFF)
    core = tuple(slice(1, -1) for _ in range(3))
    c = np.zeros((3, T) + typ.shape, dtype=np.int64)
    for ax in range(3):
        for sh in (-1, 1):
            nb = np.roll(L, sh, axis=ax)[core]
            c[ax] += look[:, nb]
    return c


def penalty(typ, K, w, beta_pv):
    """P_t = (beta_pv ((w_x c_x + w_y c_y) + w_z c_z)) 0.5, [T] + typ.shape, in w's dtype"""
    w = np.asarray(w)
    dt = w.dtype.type
    c = neighbour_counts(typ, K).astype(w.dtype)
    return (dt(beta_pv) * ((w[0] * c[0] + w[1] * c[1]) + w[2] * c[2])) * dt(0.5)


def _relative_gap(EP):
    """per voxel (s1 - s0) / max(|s0|, |s1|, 1) of the two lowest entries along axis 0 (an energy near zero is a difference of larger terms,
    so magnitudes below 1 count as 1); inf with fewer than two finite entries"""
    if EP.shape[0] < 2:
        return np.full(EP.shape[1:], np.inf)
    s = np.sort(EP, axis=0)
    with np.errstate(invalid="ignore"):
        g = (s[1] - s[0]) / np.maximum(np.maximum(np.abs(s[0]), np.abs(np.where(np.isfinite(s[1]), s[1], 0.0))), 1.0)
    return np.where(np.isfinite(s[1]), g, np.inf).astype(np.float64)


def icm_pass(typ, E, live, w, beta_pv, colour, gaps=None):
    """one colour pass -> the new types; gaps, an array shaped like typ, is lowered to the relative gap of every visit"""
    live = np.asarray(live)
    if not live.any():
        return typ.copy()
    K = (E.shape[0] + 1) // 2
    EP = np.where(live[(slice(None),) + (None,) * typ.ndim], E + penalty(typ, K, np.asarray(w).astype(E.dtype), beta_pv), np.inf)
    at = (typ != OFF) & (sn.colour_of(typ.shape) == colour)
    out = typ.copy()
    out[at] = np.argmin(EP[:, at], axis=0)
    if gaps is not None:
        gaps[at] = np.minimum(gaps[at], _relative_gap(EP[:, at]))
    return out


def icm(typ, E, live, w, beta_pv, n_sweeps, trace=None, gaps=None):
    for _ in range(n_sweeps):
        for colour in (0, 1):
            typ = icm_pass(typ, E, live, w, beta_pv, colour, gaps)
            if trace is not None:
                trace.append(typ)
    return typ


def energy_gap(E, om, live, seg, w, beta_pv, n_sweeps):
    """the smallest relative gap between the two lowest E + P of the live types that any visit of a voxel saw: the first argmin (P = 0) and
    every visit of every sweep -> (gap per voxel, inf off the domain or with one live type; the final types)"""
    gaps = np.full(om.shape, np.inf)
    lv = np.asarray(live)
    if lv.any():
        gaps[om] = _relative_gap(np.where(lv[:, None], E[:, om], np.inf))
    typ = icm(init_types(E, om, live, seg), E, live, w, beta_pv, n_sweeps, gaps=gaps)
    return gaps, typ


def total_energy(typ, E, w, beta_pv):
    """U = sum_Omega E_i(t_i) + (beta_pv / 2) sum over neighbouring domain pairs of w_a delta2(t_i, t_j): what no visit of the ICM may raise"""
    K = (E.shape[0] + 1) // 2
    om = typ != OFF
    u = np.take_along_axis(E, np.where(om, typ, 0).astype(np.int64)[None], axis=0)[0][om].sum()
    look = np.zeros((256, 256), dtype=np.int64)
    look[:n_types(K), :n_types(K)] = delta2_table(K)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        p, q = typ[tuple(lo)], typ[tuple(hi)]
        u += beta_pv * 0.5 * w[ax] * look[p, q][(p != OFF) & (q != OFF)].sum()
    return u


# ---- step 7 ----

def finish(v, typ, mu):
    """-> (pve [K] + v.shape in v's dtype, pveseg, mixeltype)"""
    K = len(mu)
    T = n_types(K)
    pve = np.zeros((K,) + v.shape, dtype=v.dtype)
    pveseg = np.zeros(v.shape, dtype=np.uint8)
    on = typ < T
    for k in range(K):
        at = typ == k
        pve[k][at] = 1.0
        pveseg[at] = k + 1
    for j in range(K - 1):
        at = typ == K + j
        with np.errstate(invalid="ignore", divide="ignore"):
            al = np.clip((mu[j + 1] - v[at]) / (mu[j + 1] - mu[j]), 0.0, 1.0)
        pve[j][at] = al
        pve[j + 1][at] = 1.0 - al
        pveseg[at] = np.where(al >= 1.0 - al, j + 1, j + 2)
    return pve, pveseg, np.where(on, typ, OFF).astype(np.uint8)


def partial_volume(v, seg, prob, voxel_size=(1.0, 1.0, 1.0), beta_pv=0.3, n_icm=8, dtype=np.float64):
    """-> dict(pve, pveseg, mixeltype, classes_lin [3 K], and what they were made with: mu, var, pi, a, h, live, table, E, types0, w, om)"""
    seg = np.asarray(seg)
    om = seg != 0
    vd = np.asarray(v, dtype=np.float64).astype(dtype)
    mo = moments(v, seg, prob, dtype)
    a, h, live, tab = consts(mo["mu"], mo["var"], mo["pi"], dtype)
    E = energies(vd, om, mo["mu"], a, h, live, tab)
    w = sn.axis_weights(voxel_size, dtype)
    t0 = init_types(E, om, live, seg)
    typ = icm(t0, E, live, w, beta_pv, n_icm)
    pve, pveseg, mixel = finish(vd, typ, mo["mu"])
    return {"pve": pve, "pveseg": pveseg, "mixeltype": mixel, "classes_lin": np.concatenate([mo["mu"], mo["var"], mo["pi"]]), "mu": mo["mu"],
            "var": mo["var"], "pi": mo["pi"], "a": a, "h": h, "live": live, "table": tab, "E": E, "types0": t0, "w": w, "om": om}


# ---- a volume with known fractions ----

def phantom(n=24, seed=1, noise=0.04, levels=sn.LEVELS, over=4):
    """three nested shells (the driest tissue innermost, so neighbouring tissues are rank-adjacent) on an n^3 grid: the tissue of every
    sub-voxel of an `over`-times finer grid, block-averaged -> (v = sum_k f_k level_k with multiplicative Gaussian noise, the true fractions
    f [3, n, n, n])"""
    rng = np.random.default_rng(seed)
    m = n * over
    ax = (np.arange(m) + 0.5) / m * 2.0 - 1.0
    x, y, z = np.meshgrid(ax, ax * 1.1, ax * 0.9, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    lab = (r > 0.85).astype(np.int64) + (r > 1.12)           # three tissues of about equal volume
    f = np.stack([(lab == k).reshape(n, over, n, over, n, over).mean(axis=(1, 3, 5)) for k in range(3)])
    clean = np.tensordot(np.asarray(levels, dtype=np.float64), f, axes=1)
    return clean * (1.0 + noise * rng.standard_normal(clean.shape)), f


# ---- the seeded inputs of tests/test_pve_host.py and tests/test_gpu_pve.py ----

def masked(shape, count, seed):
    """a mask with exactly `count` voxels in: a random choice, so it has holes everywhere"""
    rng = np.random.default_rng(seed)
    m = np.zeros(int(np.prod(shape)), dtype=np.uint8)
    m[rng.choice(m.size, size=count, replace=False)] = 1
    return m.reshape(shape)


def levels_for(K):
    return sn.LEVELS if K <= 3 else tuple(np.geomspace(400.0, 1600.0, K))


TILE = (4, 8, 16)                 # the tile of pve_icm_kernel (x, y, z)
# name: (shape, voxel size, K, the domain's size or None for every voxel, seed, index of a class made dead or None).  The seeds were picked on
# the CPU (tests/test_pve_host.py) so that the long-double restatement's smallest relative energy gap over all visits is >= 1e-9.
CASES = {
    "one": ((1, 1, 1), (1.0, 1.0, 1.0), 3, None, 1, None),
    "line": ((3, 1, 40), (1.0, 1.0, 1.0), 3, None, 2, None),
    "tile": ((4, 8, 16), (1.0, 1.0, 1.0), 3, None, 3, None),
    "tile+1": ((5, 9, 17), (1.0, 1.0, 1.0), 3, None, 4, None),
    "2tile+1": ((9, 17, 33), (1.0, 1.0, 1.0), 3, None, 5, None),
    "n1023": ((9, 17, 33), (1.0, 1.0, 1.0), 3, 1023, 6, None),
    "n1024": ((9, 17, 33), (1.0, 1.0, 1.0), 3, 1024, 7, None),
    "n1025": ((9, 17, 33), (1.0, 1.0, 1.0), 3, 1025, 8, None),
    "n2049": ((9, 17, 33), (1.0, 1.0, 1.0), 3, 2049, 9, None),
    "aniso": ((5, 9, 17), (2.0, 1.5, 4.0), 3, None, 10, None),
    "k1": ((5, 9, 17), (1.0, 1.0, 1.0), 1, None, 11, None),
    "k2": ((5, 9, 17), (1.0, 1.0, 1.0), 2, 600, 12, None),
    "k8": ((9, 17, 33), (1.0, 1.0, 1.0), 8, 2049, 13, None),
    "dead": ((5, 9, 17), (1.0, 2.0, 1.0), 3, None, 14, 1),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(v, seg, prob, voxel, K, om): the volume, and the labels and posteriors seg_numpy's restatement of the segmentation gives for it
    (n_outer = 2); a dead class has its row of prob zeroed.  Computed once; the arrays are read-only"""
    shape, vox, K, count, seed, dead = CASES[name]
    v, _, _ = sn.phantom(shape, 500 + seed, levels=levels_for(K))
    mask = None if count is None else masked(shape, count, 900 + seed)
    res = sn.tissue_segment(v, mask, vox, n_class=K, n_outer=2)
    seg, prob = res["seg"], np.array(res["prob"], dtype=np.float64)
    if dead is not None:
        prob[dead] = 0.0
    out = {"v": v, "seg": seg, "prob": prob, "voxel": vox, "K": K, "om": seg != 0, "dead": dead}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
