"""A numpy restatement of the tissue segmentation that include/met2_hip.h states for met2_tissue_segment (the hidden-Markov-random-field EM of
Zhang, Brady & Smith, IEEE TMI 2001: Gaussian classes in log intensity, a Potts prior over the six face neighbours, labels by iterated
conditional modes): the reference of tests/test_gpu_seg.py.  Written from the header, step by step; not fast.  Steps 1 and 7 (domain, log,
initial classes, plain EM, the M-step) are those of bias_numpy.  `dtype=np.longdouble` runs every step in extended precision
(tests/test_seg_host.py: the labels must not depend on it).  The stage functions take the class constants mu, a, h, live as arguments, so a
stage test can hand them the device's.  Labels are uint8 volumes: a class 0..K-1 on the domain, OFF off it.  case(name) makes the seeded
test volumes."""
import numpy as np

import bias_numpy as bn

OFF = 255


def axis_weights(voxel_size, dtype=np.float64):
    """step 4: w_a = d_min / d_a"""
    vox = np.asarray(voxel_size, dtype=np.float64).astype(dtype)
    return vox.min() / vox


def consts(var, pi, dtype=np.float64):
    """step 2 -> (a = 1 / (2 var), h = 0.5 log var, live = pi != 0)"""
    dt = np.dtype(dtype).type
    var = np.asarray(var).astype(dtype)
    return dt(1.0) / (dt(2.0) * var), dt(0.5) * np.log(var), np.asarray(pi) != 0


def data_term(y, mu, a, h):
    """D_k = ((y - mu_k)^2 a_k) + h_k, [K] + y.shape, every operation rounded once in y's dtype"""
    ex = (slice(None),) + (None,) * y.ndim
    d = y[None] - mu[ex]
    return (d * d) * a[ex] + h[ex]


def _argmin_live(E, live):
    """argmin over the live classes, ties to the lowest k"""
    E = np.where(np.asarray(live)[(slice(None),) + (None,) * (E.ndim - 1)], E, np.inf)
    return np.argmin(E, axis=0)


def init_labels(y, om, mu, a, h, live):
    """step 3 on the volume y with the domain om (bool) -> labels"""
    lab = np.full(y.shape, OFF, dtype=np.uint8)
    lab[om] = _argmin_live(data_term(y[om], mu, a, h), live)
    return lab


def differing(lab, K):
    """c [3, K] + lab.shape: per axis and class the number of domain neighbours, inside the volume, whose label differs from k"""
    L = np.pad(lab, 1, constant_values=OFF)
    core = tuple(slice(1, -1) for _ in range(3))
    c = np.zeros((3, K) + lab.shape, dtype=np.int64)
    for ax in range(3):
        for sh in (-1, 1):
            nb = np.roll(L, sh, axis=ax)[core]
            for k in range(K):
                c[ax, k] += (nb != OFF) & (nb != k)
    return c


def penalty(lab, K, w, beta):
    """P_k = beta ((w_x c_x + w_y c_y) + w_z c_z), [K] + lab.shape, in w's dtype"""
    dt = np.asarray(w).dtype
    c = differing(lab, K).astype(dt)
    return dt.type(beta) * ((w[0] * c[0] + w[1] * c[1]) + w[2] * c[2])


def energies(lab, y, mu, a, h, w, beta):
    """E_k = D_k + P_k, [K] + lab.shape (also off the domain, where it means nothing)"""
    return data_term(y, mu, a, h) + penalty(lab, len(mu), np.asarray(w).astype(y.dtype), beta)


def colour_of(shape):
    ix, iy, iz = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return (ix + iy + iz) & 1


def icm_pass(lab, y, mu, a, h, live, w, beta, colour):
    """one colour pass of step 5 -> the new labels"""
    E = energies(lab, y, mu, a, h, w, beta)
    at = (lab != OFF) & (colour_of(lab.shape) == colour)
    out = lab.copy()
    out[at] = _argmin_live(E[:, at], live)
    return out


def icm(lab, y, mu, a, h, live, w, beta, n_sweeps, trace=None):
    """n_sweeps sweeps; trace, a list, receives the labels after every colour pass"""
    for _ in range(n_sweeps):
        for colour in (0, 1):
            lab = icm_pass(lab, y, mu, a, h, live, w, beta, colour)
            if trace is not None:
                trace.append(lab)
    return lab


def posterior(lab, y, mu, a, h, live, w, beta):
    """step 6 -> p [K] + lab.shape, 0 off the domain and for dead classes"""
    om = lab != OFF
    E = energies(lab, y, mu, a, h, w, beta)[:, om]
    lv = np.asarray(live)
    E = np.where(lv[:, None], E, np.inf)
    with np.errstate(invalid="ignore"):
        e = np.where(lv[:, None], np.exp(E.min(axis=0)[None, :] - E), 0.0)
    p = np.zeros((len(mu),) + lab.shape, dtype=y.dtype)
    p[:, om] = e / e.sum(axis=0)[None, :]
    return p


def energy_gap(lab, y, mu, a, h, live, w, beta):
    """per voxel the distance from the lowest energy of a live class to the next one (inf with one live class): what a label hangs on"""
    E = np.where(np.asarray(live)[:, None, None, None], energies(lab, y, mu, a, h, w, beta), np.inf)
    if E.shape[0] < 2:
        return np.full(lab.shape, np.inf)
    s = np.sort(E, axis=0)
    with np.errstate(invalid="ignore"):
        return s[1] - s[0]


def total_energy(lab, y, mu, a, h, w, beta):
    """U = sum_Omega D_i(x_i) + beta sum over neighbouring domain pairs of w_a [x_i != x_j]: what no visit of the ICM may raise"""
    om = lab != OFF
    D = data_term(y, mu, a, h)
    u = np.take_along_axis(D, np.where(om, lab, 0).astype(np.int64)[None], axis=0)[0][om].sum()
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        p, q = lab[tuple(lo)], lab[tuple(hi)]
        u += beta * w[ax] * ((p != OFF) & (q != OFF) & (p != q)).sum()
    return u


def isolated(lab):
    """the number of domain voxels with six domain neighbours that all carry another label"""
    L = np.pad(lab, 1, constant_values=OFF)
    core = tuple(slice(1, -1) for _ in range(3))
    alone = lab != OFF
    for ax in range(3):
        for sh in (-1, 1):
            nb = np.roll(L, sh, axis=ax)[core]
            alone &= (nb != OFF) & (nb != lab)
    return int(alone.sum())


def ranks(mu):
    """rank_k = the number of j with mu_j < mu_k, or mu_j == mu_k and j < k"""
    r = np.empty(len(mu), dtype=np.int64)
    r[np.argsort(np.asarray(mu, dtype=np.float64), kind="stable")] = np.arange(len(mu))
    return r


def finish(lab, p, mu, var, pi):
    """-> (seg, prob in rank order or None, classes [3 K] in rank order)"""
    K = len(mu)
    r = ranks(mu)
    seg = np.zeros(lab.shape, dtype=np.uint8)
    on = lab < K
    seg[on] = r[lab[on]] + 1
    order = np.argsort(r)
    prob = None if p is None else np.where(on[None], p, 0.0)[order]
    return seg, prob, np.concatenate([np.asarray(mu)[order], np.asarray(var)[order], np.asarray(pi)[order]])


def tissue_segment(v, mask=None, voxel_size=(1.0, 1.0, 1.0), n_class=3, beta=0.1, n_outer=4, n_em=10, n_icm=8, dtype=np.float64):
    """-> dict(seg, prob [K, ...], classes [3 K], labels: the final labels before the ranking, mu, a, h, live: what they were made with, y, w)"""
    K = int(n_class)
    v64 = np.asarray(v, dtype=np.float64)
    y, om = bn.log_domain(v64, mask, dtype)
    ini = bn.init_classes(y[om], K, dtype)
    if ini["degenerate"]:
        prob = np.zeros((K,) + v64.shape, dtype=dtype)
        prob[0][om] = 1.0
        return {"seg": om.astype(np.uint8), "prob": prob, "classes": np.concatenate([ini["mu"], ini["var"], ini["pi"]]), "labels": None}
    mu, var, pi = ini["mu"], ini["var"], ini["pi"]
    u = y[om]
    for _ in range(n_em):
        bn.m_step(bn.e_step(u, mu, var, pi), u, mu, var, pi)
    w = axis_weights(voxel_size, dtype)
    a, h, live = consts(var, pi, dtype)
    lab = init_labels(y, om, mu, a, h, live)
    for _ in range(n_outer):
        lab = icm(lab, y, mu, a, h, live, w, beta, n_icm)
        p = posterior(lab, y, mu, a, h, live, w, beta)
        bn.m_step(p[:, om], u, mu, var, pi)
        a, h, live = consts(var, pi, dtype)
    lab = icm(lab, y, mu, a, h, live, w, beta, n_icm)
    p = posterior(lab, y, mu, a, h, live, w, beta)
    seg, prob, classes = finish(lab, p, mu, var, pi)
    return {"seg": seg, "prob": prob, "classes": classes, "labels": lab, "mu": mu.copy(), "a": a, "h": h, "live": live, "y": y, "w": w}


# ---- the seeded volumes of tests/test_seg_host.py and tests/test_gpu_seg.py ----

LEVELS = (500.0, 800.0, 1100.0)


def phantom(shape, seed, noise=0.08, levels=LEVELS, mask_kind="all"):
    """a piecewise-constant volume of len(levels) tissues (slabs across x, cut again across y) with multiplicative Gaussian noise
    -> (v, mask or None, the true labels).  mask_kind: 'all' (None); 'holes': a random 15 % of the voxels out, a slab of the volume cut off
    from the rest but for a one-voxel bridge; 'disc': bias_numpy's circular mask"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    ix, iy, iz = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    L = len(levels)
    lab = ((ix * L) // max(nx, 1) + (iy * 2) // max(ny, 1)) % L
    v = np.asarray(levels)[lab] * (1.0 + noise * rng.standard_normal(shape))
    mask = None
    if mask_kind == "holes":
        mask = (rng.random(shape) < 0.85).astype(np.uint8)
        cut = nx // 2
        mask[cut] = 0                                                 # a wall across x ...
        mask[cut, ny // 2, nz // 2] = 1                               # ... with a one-voxel bridge
        mask[cut - 1, ny // 2, nz // 2] = mask[min(cut + 1, nx - 1), ny // 2, nz // 2] = 1
    elif mask_kind == "disc":
        ax = [np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1) for n in shape]
        x, yy, _ = np.meshgrid(*ax, indexing="ij")
        mask = (np.sqrt(x * x + yy * yy) < 0.9).astype(np.uint8)
    return v, mask, lab


# name: (shape, voxel_size, seed, mask_kind, levels, kwargs of tissue_segment).  The seeds were picked on the CPU (tests/test_seg_host.py) so
# that the fp64 and the long-double restatement give the same labels: no label of these volumes hangs on a rounding.
CASES = {
    "block": ((24, 20, 18), (1.0, 1.0, 1.0), 1, "all", LEVELS, {}),
    "odd": ((17, 9, 5), (1.0, 1.0, 3.0), 2, "all", LEVELS, {}),
    "holes": ((24, 20, 18), (2.0, 2.0, 4.0), 3, "holes", LEVELS, {}),
    "flat": ((16, 16, 1), (1.0, 1.0, 1.0), 4, "all", LEVELS, {}),
    "line": ((1, 1, 64), (1.0, 1.0, 1.0), 5, "all", LEVELS, {"n_class": 2}),
    "k4": ((33, 1, 7), (1.0, 1.0, 1.0), 6, "all", (400.0, 650.0, 1000.0, 1500.0), {"n_class": 4}),
    "k1": ((17, 9, 5), (1.0, 1.0, 1.0), 7, "disc", LEVELS, {"n_class": 1}),
    "k8": ((24, 20, 18), (1.0, 1.0, 1.0), 8, "disc", LEVELS, {"n_class": 8, "n_outer": 2}),
    "beta0": ((17, 9, 5), (1.0, 1.0, 1.0), 9, "all", LEVELS, {"beta": 0.0}),
    "inverted": ((24, 20, 18), (1.0, 1.0, 1.0), 1, "all", LEVELS, {}),
}
INVERTED_OVER = 4.0e5             # 'inverted' is 'block' with v -> 4e5 / v: the wettest tissue becomes the driest


def case(name, seed=None):
    """-> (v, mask, voxel_size, kwargs of tissue_segment)"""
    shape, vox, s, kind, levels, kw = CASES[name]
    v, mask, _ = phantom(shape, s if seed is None else seed, levels=levels, mask_kind=kind)
    if name == "inverted":
        v = INVERTED_OVER / v
    return v, mask, vox, dict(kw)


def stage_input(name, K=None, seed=None):
    """the input of a stage test -> dict(v, mask, y, om, idx, classes = (mu, var, pi), w, K): the case's volume with classes that the
    restatement's first step leaves (n_em plain EM steps), K overriding the case's class number"""
    v, mask, vox, kw = case(name, seed)
    K = int(kw.get("n_class", 3) if K is None else K)
    y, om = bn.log_domain(v, mask)
    ini = bn.init_classes(y[om], K)
    mu, var, pi = ini["mu"], ini["var"], ini["pi"]
    u = y[om]
    for _ in range(3):
        bn.m_step(bn.e_step(u, mu, var, pi), u, mu, var, pi)
    return {"v": v, "mask": mask, "y": y, "om": om, "idx": np.flatnonzero(om.reshape(-1)).astype(np.int32), "classes": (mu, var, pi),
            "w": axis_weights(vox), "K": K}
