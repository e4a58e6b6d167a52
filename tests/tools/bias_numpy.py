"""A numpy restatement of the bias-field estimation that include/met2_hip.h states for met2_bias_field (the EM estimator of Wells et al.,
IEEE TMI 1996, and Guillemaud & Brady, 1997: class-posterior-weighted residual, low-pass filtered by a normalised Gaussian convolution;
FAST's iteration without its Markov random field term): the reference of tests/test_gpu_bias.py.  Written from the header, step by step;
not fast.  `dtype=np.longdouble` runs every step in extended precision (tests/test_bias_host.py: how far rounding moves the result).
case(name) makes the seeded test volumes, init_margin(...) says how far the initial class means are from depending on one sample."""
import numpy as np

VAR_FLOOR = 1e-6
NBINS = 256


def radius_weights(fwhm, d, dtype=np.float64):
    """step 1, one axis: (r, w[2 r + 1]): sigma = fwhm / (2 sqrt(2 ln 2)) / d voxels, r = int(4 sigma + 0.5), Gaussian weights of sum 1"""
    dt = np.dtype(dtype).type
    sigma = dt(fwhm) / (dt(2.0) * np.sqrt(dt(2.0) * np.log(dt(2.0)))) / dt(d)
    r = int(dt(4.0) * sigma + dt(0.5))
    t = np.arange(-r, r + 1).astype(dtype)
    w = np.exp(-(t * t) / (dt(2.0) * sigma * sigma))
    return r, w / w.sum()


def smooth_axis(a, w, axis):
    """out[i] = sum_t w[t] a[i + t], t ascending, a = 0 outside the volume"""
    r = (len(w) - 1) // 2
    n = a.shape[axis]
    out = np.zeros_like(a)
    for t in range(-r, r + 1):
        i0, i1 = max(0, -t), min(n, n - t)
        if i1 <= i0:
            continue
        dst = [slice(None)] * a.ndim
        src = [slice(None)] * a.ndim
        dst[axis] = slice(i0, i1)
        src[axis] = slice(i0 + t, i1 + t)
        out[tuple(dst)] += w[t + r] * a[tuple(src)]
    return out


def smooth(a, weights):
    for axis in range(3):
        a = smooth_axis(a, weights[axis], axis)
    return a


def domain(v, mask):
    v = np.asarray(v)
    ok = np.isfinite(v) & (np.where(np.isfinite(v), v, 0.0) > 0)
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def histogram(y, lo, hi):
    dt = y.dtype.type
    j = np.minimum(NBINS - 1, np.floor((y - lo) / (hi - lo) * dt(NBINS)).astype(np.int64))
    return np.bincount(j, minlength=NBINS)


def init_bins(c, K, N):
    """j_k: the first bin whose cumulative count reaches (2 k + 1) / (2 K) N"""
    return [int(np.argmax(c.astype(np.float64) >= (2 * k + 1) / (2.0 * K) * N)) for k in range(K)]


def e_step(u, mu, var, pi):
    with np.errstate(divide="ignore"):
        logc = np.log(pi) - 0.5 * np.log(var)
    l = logc[:, None] - (u[None, :] - mu[:, None]) ** 2 / (2.0 * var[:, None])
    e = np.exp(l - l.max(axis=0)[None, :])
    return e / e.sum(axis=0)[None, :]


# ---- the stages, each on the output of the one before it (tests/test_gpu_bias_stages.py runs them on the DEVICE's output of the stage before;
# ---- dtype=np.longdouble evaluates the same formulas in extended precision)

def log_domain(v, mask=None, dtype=np.float64):
    """step 1 -> (y: log v on Omega and 0 off it, shaped like v; Omega as a boolean array)"""
    v64 = np.asarray(v, dtype=np.float64)
    om = domain(v64, mask)
    y = np.zeros(v64.shape, dtype=dtype)
    y[om] = np.log(v64[om].astype(dtype))
    return y, om


def init_classes(y, K, dtype=np.float64):
    """step 2 on y [N], the domain's values in memory order -> dict(lo, hi, degenerate, and unless degenerate mean, ss = sum (y - mean)^2,
    hist [256], jk [K], mu, var, pi [K])"""
    dt = np.dtype(dtype).type
    y = np.asarray(y).astype(dtype)
    N = y.size
    lo, hi = (y.min(), y.max()) if N else (dt(0.0), dt(0.0))
    if N == 0 or hi == lo:
        return {"lo": lo, "hi": hi, "degenerate": True, "mu": np.full(K, lo).astype(dtype), "var": np.zeros(K, dtype=dtype),
                "pi": np.full(K, 1.0 / K).astype(dtype)}
    hist = histogram(y, lo, hi)
    jk = init_bins(np.cumsum(hist), K, N)
    mu = np.array([lo + (dt(j) + dt(0.5)) * (hi - lo) / dt(NBINS) for j in jk], dtype=dtype)
    mean = y.mean()
    return {"lo": lo, "hi": hi, "degenerate": False, "mean": mean, "ss": ((y - mean) ** 2).sum(), "hist": hist, "jk": jk, "mu": mu,
            "var": np.full(K, y.var() / dt(K * K), dtype=dtype), "pi": np.full(K, dt(1.0) / dt(K), dtype=dtype)}


def log_terms(u, mu, var, pi):
    """l_k = log pi_k - log(var_k) / 2 - (u - mu_k)^2 / (2 var_k), [K, N]; -inf for a class with pi_k = 0"""
    with np.errstate(divide="ignore"):
        logc = np.log(pi) - 0.5 * np.log(var)
    return logc[:, None] - (u[None, :] - mu[:, None]) ** 2 / (2.0 * var[:, None])


def m_step(p, u, mu, var, pi):
    """the M-step of step 3 in place on mu, var, pi (the variance about the NEW mean) -> s [K]"""
    dt = u.dtype.type
    s = p.sum(axis=1)
    for k in range(len(mu)):
        if s[k] == 0:
            pi[k] = 0.0
            continue
        mu[k] = (p[k] * u).sum() / s[k]
        var[k] = max((p[k] * (u - mu[k]) ** 2).sum() / s[k], dt(VAR_FLOOR))
        pi[k] = s[k] / dt(u.size)
    return s


def em_sums(p, u, mu):
    """the 3 K sums the kernels form, [3, K]: s_k = sum p_k, sum p_k u, sum p_k (u - m_k)^2 about the mean m_k the E-step ran with;
    and the sums of the terms' magnitudes, the scale their rounding is measured against"""
    d2 = (u[None, :] - mu[:, None]) ** 2
    return np.stack([p.sum(axis=1), (p * u[None, :]).sum(axis=1), (p * d2).sum(axis=1)]), \
        np.stack([p.sum(axis=1), (p * np.abs(u)[None, :]).sum(axis=1), (p * d2).sum(axis=1)])


def class_update(sums, mu, var, pi, N):
    """the M-step as the kernel states it, from the 3 K sums about the old means: mu' = a / s, var' = max(q / s - (mu' - mu)^2, 1e-6),
    pi' = s / N; a class with s = 0 keeps mu and var and gets pi = 0 -> (mu', var', pi')"""
    dt = sums.dtype.type
    mu, var, pi = mu.astype(sums.dtype), var.astype(sums.dtype), pi.astype(sums.dtype)
    for k in range(len(mu)):
        s, a, q = sums[0][k], sums[1][k], sums[2][k]
        if s == 0:
            pi[k] = 0.0
            continue
        mn = a / s
        var[k] = max(q / s - (mn - mu[k]) ** 2, dt(VAR_FLOOR))
        mu[k] = mn
        pi[k] = s / dt(N)
    return mu, var, pi


def residual_weights(p, u, mu, var):
    """R = sum_k p_k (u - mu_k) / var_k and W = sum_k p_k / var_k on the list, [N] each"""
    return (p * (u[None, :] - mu[:, None]) / var[:, None]).sum(axis=0), (p / var[:, None]).sum(axis=0)


def update_b(b, SR, SW, om):
    """b += S_R / S_W on D = {S_W > 0}, then b -= mean_Omega(b) on D, in place -> that mean"""
    D = SW > 0
    b[D] += SR[D] / SW[D]
    bmean = b[om].mean()
    b[D] -= bmean
    return bmean


def bias_field(v, mask=None, voxel_size=(1.0, 1.0, 1.0), n_class=3, n_outer=4, n_em=10, fwhm=20.0, dtype=np.float64, init_shift=None,
               trace=None):
    """-> dict(out, field, classes [3 K] = mu, var, pi, b, omega, support).  init_shift = (k, bins) moves the initial mean of class k by
    whole histogram bins (tests only); trace, a list, receives (outer, em, s) after every M-step.  Composed of the stage functions above."""
    dt = np.dtype(dtype).type
    K = int(n_class)
    v64 = np.asarray(v, dtype=np.float64)
    yv, om = log_domain(v64, mask, dtype)
    fin = np.isfinite(v64)
    field = np.ones(v64.shape, dtype=dtype)
    b = np.zeros(v64.shape, dtype=dtype)
    y = yv[om]
    ini = init_classes(y, K, dtype)
    if ini["degenerate"]:
        classes = np.concatenate([ini["mu"], ini["var"], ini["pi"]]).astype(dtype)
        return {"out": v64.astype(dtype), "field": field, "classes": classes, "b": b, "omega": om, "support": np.zeros(v64.shape, dtype=bool)}
    weights = [radius_weights(fwhm, d, dtype)[1] for d in voxel_size]
    lo, hi, mu, var, pi = ini["lo"], ini["hi"], ini["mu"], ini["var"], ini["pi"]
    if init_shift is not None:
        mu[init_shift[0]] += dt(init_shift[1]) * (hi - lo) / dt(NBINS)
    support = smooth(om.astype(dtype), weights) > 0
    for it in range(n_outer):
        u = y - b[om]
        for em in range(n_em):
            s = m_step(e_step(u, mu, var, pi), u, mu, var, pi)
            if trace is not None:
                trace.append((it, em, s.copy(), var.copy()))
        p = e_step(u, mu, var, pi)
        R = np.zeros(v64.shape, dtype=dtype)
        W = np.zeros(v64.shape, dtype=dtype)
        R[om], W[om] = residual_weights(p, u, mu, var)
        update_b(b, smooth(R, weights), smooth(W, weights), om)
    field = np.exp(b)
    out = v64.astype(dtype)
    out[fin] = out[fin] / field[fin]
    return {"out": out, "field": field, "classes": np.concatenate([mu, var, pi]), "b": b, "omega": om, "support": support}


def _bias_field_v0(v, mask=None, voxel_size=(1.0, 1.0, 1.0), n_class=3, n_outer=4, n_em=10, fwhm=20.0, dtype=np.float64, init_shift=None,
               trace=None):
    """bias_field() as it stood before it was composed of the stage functions above, kept for one test (tests/test_bias_host.py): the two
    must return the same bits"""
    dt = np.dtype(dtype).type
    K = int(n_class)
    v64 = np.asarray(v, dtype=np.float64)
    om = domain(v64, mask)
    N = int(om.sum())
    fin = np.isfinite(v64)
    field = np.ones(v64.shape, dtype=dtype)
    b = np.zeros(v64.shape, dtype=dtype)
    y = np.log(v64[om].astype(dtype))
    lo, hi = (y.min(), y.max()) if N else (dt(0.0), dt(0.0))
    if N == 0 or hi == lo:
        classes = np.concatenate([np.full(K, lo), np.zeros(K), np.full(K, 1.0 / K)]).astype(dtype)
        return {"out": v64.astype(dtype), "field": field, "classes": classes, "b": b, "omega": om, "support": np.zeros(v64.shape, dtype=bool)}
    weights = [radius_weights(fwhm, d, dtype)[1] for d in voxel_size]
    c = np.cumsum(histogram(y, lo, hi))
    jk = init_bins(c, K, N)
    mu = np.array([lo + (dt(j) + dt(0.5)) * (hi - lo) / dt(NBINS) for j in jk], dtype=dtype)
    if init_shift is not None:
        mu[init_shift[0]] += dt(init_shift[1]) * (hi - lo) / dt(NBINS)
    var = np.full(K, y.var() / dt(K * K), dtype=dtype)
    pi = np.full(K, dt(1.0) / dt(K), dtype=dtype)
    support = smooth(om.astype(dtype), weights) > 0
    for it in range(n_outer):
        u = y - b[om]
        for em in range(n_em):
            p = e_step(u, mu, var, pi)
            s = p.sum(axis=1)
            for k in range(K):
                if s[k] == 0:
                    pi[k] = 0.0
                    continue
                mu[k] = (p[k] * u).sum() / s[k]
                var[k] = max((p[k] * (u - mu[k]) ** 2).sum() / s[k], dt(VAR_FLOOR))
                pi[k] = s[k] / dt(N)
            if trace is not None:
                trace.append((it, em, s.copy(), var.copy()))
        p = e_step(u, mu, var, pi)
        R = np.zeros(v64.shape, dtype=dtype)
        W = np.zeros(v64.shape, dtype=dtype)
        R[om] = (p * (u[None, :] - mu[:, None]) / var[:, None]).sum(axis=0)
        W[om] = (p / var[:, None]).sum(axis=0)
        SR, SW = smooth(R, weights), smooth(W, weights)
        D = SW > 0
        b[D] += SR[D] / SW[D]
        b[D] -= b[om].mean()
    field = np.exp(b)
    out = v64.astype(dtype)
    out[fin] = out[fin] / field[fin]
    return {"out": out, "field": field, "classes": np.concatenate([mu, var, pi]), "b": b, "omega": om, "support": support}


def init_margin(v, mask=None, n_class=3):
    """per class k: (T_k - c[j_k - 1], c[j_k] - T_k) in samples, T_k = (2 k + 1) / (2 K) N the threshold that picks bin j_k: how many
    samples would have to change bins before another j_k is picked"""
    om = domain(np.asarray(v, dtype=np.float64), mask)
    y = np.log(np.asarray(v, dtype=np.float64)[om])
    N = y.size
    c = np.cumsum(histogram(y, y.min(), y.max()))
    out = []
    for k, j in enumerate(init_bins(c, n_class, N)):
        T = (2 * k + 1) / (2.0 * n_class) * N
        out.append((T - (c[j - 1] if j > 0 else 0), c[j] - T))
    return out


def true_log_field(shape):
    ax = [np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1) for n in shape]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    return 0.25 * x - 0.2 * y + 0.15 * x * y + 0.1 * z


def phantom(shape=(40, 36, 12), seed=7, noise=0.02, levels=(500.0, 800.0, 1100.0)):
    """three concentric tissue classes under a smooth multiplicative field, multiplicative noise, a circular mask
    -> (v, mask, true log field, labels)"""
    rng = np.random.default_rng(seed)
    ax = [np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1) for n in shape]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    rr = np.sqrt(x * x + y * y)
    lab = np.where(rr < 0.35, 0, np.where(rr < 0.65, 1, 2))
    logf = true_log_field(shape)
    v = np.asarray(levels)[lab] * np.exp(logf) * (1.0 + noise * rng.standard_normal(shape))
    mask = (rr < 0.9).astype(np.uint8)
    return v, mask, logf, lab


SEEDS = {"phantom": 1, "thin": 254, "wave": 6, "coarse": 63, "coarse80": 63, "k8floor": 2, "holes": 2, "k1": 1, "k8": 5, "outer0": 1,
         "seams": 3, "r64": 3, "big": 4, "bigall": 4}
CASES = tuple(SEEDS)
NEW_SHAPES = {"seams": ((9, 70, 131), (8.0, 3.0, 2.0)), "r64": ((130, 20, 3), (0.53, 2.0, 4.0)), "big": ((64, 64, 65), (8.0, 8.0, 8.0)),
              "bigall": ((64, 64, 65), (8.0, 8.0, 8.0))}
STRETCH = {"thin": (5.0, 1.0e5), "k8floor": (5.0, 1.0e5)}


def case(name, seed=None):
    """-> (v, mask, voxel_size, kwargs of bias_field): the seeded volumes of tests/test_bias_host.py and tests/test_gpu_bias.py
    phantom   40 x 36 x 12, voxels 2 x 2 x 4 mm (radii 17, 17, 8)
    thin      33 x 5 x 1 at 1 mm: r = 34 on every axis, two axes shorter than the half-width, one of length 1
    wave      65 x 3 x 7, voxels 1.25 x 2.5 x 3 mm (radii 27, 14, 11): a line longer than a wave and no multiple of a tile
    coarse    9 x 9 x 9 with 40 mm voxels: 4 sigma + 0.5 = 1.35, so r = 1 with outer weights of 1.5e-5
    coarse80  the same with 80 mm voxels: r = 0 on every axis, smoothing is the identity and b the raw ratio
    holes     the phantom with zeros, negatives, a NaN and an inf inside the mask; the mask a small disc and an island apart from it,
              so that the support D leaves part of the volume out
    k1, k8    the phantom with 1 and 8 classes;  outer0: n_outer = 0
    seams     the phantom at 9 x 70 x 131, voxels 8 x 3 x 2 mm (radii 4, 11, 17): tile seams of the smoothing on y and z, three tiles on z
    r64       the phantom at 130 x 20 x 3, voxels 0.53 x 2 x 4 mm (radii 64, 17, 8): the widest halo across two seams on x
    big       the phantom at 64 x 64 x 65 (260 chunks of 1024 voxels), 8 mm voxels (radius 4): the scan's second pass, a support short of the volume
    bigall    the same without a mask: 266 240 domain voxels, 260 partials in every second-stage sum"""
    seed = SEEDS[name] if seed is None else seed
    if name in NEW_SHAPES:
        shape, vox = NEW_SHAPES[name]
        v, mask, _, _ = phantom(shape=shape, seed=seed)
        return v, (None if name == "bigall" else mask), vox, {}
    if name in ("phantom", "k1", "k8", "outer0", "holes"):
        v, mask, _, _ = phantom(seed=seed)
        kw = {"k1": {"n_class": 1}, "k8": {"n_class": 8}, "outer0": {"n_outer": 0}}.get(name, {})
        if name == "holes":
            nx, ny, nz = v.shape
            ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
            disc = (ix - 10) ** 2 + (iy - 10) ** 2 <= 64
            mask = np.repeat(disc[:, :, None], nz, axis=2).astype(np.uint8)
            mask[14:17, 31:34, 2:4] = 1                                  # the island
            v[8, 9, 3] = 0.0
            v[12, 7, 5] = -3.0
            v[5, 10, 0] = -700.0
            v[10, 13, 6] = np.nan
            v[13, 12, 11] = np.inf
            v[30, 30, 4] = np.nan                                        # one outside the mask too
        return v, mask, (2.0, 2.0, 4.0), kw
    rng = np.random.default_rng(seed)
    shape, vox = {"thin": ((33, 5, 1), (1.0, 1.0, 1.0)), "wave": ((65, 3, 7), (1.25, 2.5, 3.0)), "coarse": ((9, 9, 9), (40.0, 40.0, 40.0)),
                  "coarse80": ((9, 9, 9), (80.0, 80.0, 80.0)), "k8floor": ((9, 9, 9), (40.0, 40.0, 40.0))}[name]
    lab = rng.integers(0, 3, size=shape)
    v = np.array([500.0, 800.0, 1100.0])[lab] * np.exp(true_log_field(shape)) * (1.0 + 0.02 * rng.standard_normal(shape))
    mask = (rng.random(shape) < 0.85).astype(np.uint8)
    if name in STRETCH:                                              # two outliers stretch [lo, hi]: wider bins, more samples in each
        v[0, 0, 0], v[-1, -1, -1] = STRETCH[name]
        mask[0, 0, 0] = mask[-1, -1, -1] = 1
    return v, mask, vox, {"n_class": 8} if name == "k8floor" else {}


# ---- the inputs of the stage tests (tests/test_gpu_bias_stages.py on the device, tests/test_bias_host.py for what rounding does to them) ----

def _levels(shape, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 3, size=shape)
    return np.array([500.0, 800.0, 1100.0])[lab] * (1.0 + 0.02 * rng.standard_normal(shape)), rng


def domain_input(name):
    """-> (v, mask).  odd: 1001 voxels, no multiple of 4 or of a chunk;  exact: two whole chunks;  gap: 6144 voxels whose mask is zero over
    voxels 1500..4699, so chunks 2 and 3 hold no domain voxel;  bad: NaN, +-inf, 0 and negatives inside the mask;  nomask: mask = None;
    scan2: 64 x 64 x 65, 260 chunks: bias_scan_kernel's second pass"""
    if name == "scan2":
        return case("big")[:2]
    shape = {"odd": (7, 11, 13), "exact": (8, 16, 16), "gap": (16, 16, 24), "bad": (7, 11, 13), "nomask": (7, 11, 13)}[name]
    v, rng = _levels(shape, 100 + len(name))
    mask = (rng.random(shape) < 0.8).astype(np.uint8)
    if name == "gap":
        mask = np.ones(shape, dtype=np.uint8)
        mask.reshape(-1)[1500:4700] = 0
    if name in ("bad", "nomask"):
        at = rng.choice(v.size, size=6, replace=False)
        v.reshape(-1)[at] = [np.nan, np.inf, -np.inf, 0.0, -3.0, -700.0]
        mask.reshape(-1)[at] = 1
    return v, (None if name == "nomask" else mask)


DOMAIN_INPUTS = ("odd", "exact", "gap", "bad", "nomask", "scan2")


def init_input(name):
    """-> (v, mask, K).  n2048, n2049, n1: that many domain voxels, picked by a mask out of 6144;  const: a constant volume (degenerate);
    big1, big3, big8: 266 240 domain voxels (260 partials in the second-stage sums) with K = 1, 3, 8"""
    if name.startswith("big"):
        v, mask, _, _ = case("bigall")
        return v, mask, int(name[3:])
    shape = (16, 16, 24)
    v, rng = _levels(shape, 7)
    if name == "const":
        return np.full(shape, 750.0), (rng.random(shape) < 0.5).astype(np.uint8), 3
    N = {"n2048": 2048, "n2049": 2049, "n1": 1}[name]
    mask = np.zeros(v.size, dtype=np.uint8)
    mask[rng.choice(v.size, size=N, replace=False)] = 1
    return v, mask.reshape(shape), 3


INIT_INPUTS = ("n2048", "n2049", "n1", "const", "big1", "big3", "big8")


def em_input(name):
    """-> dict(v, mask, b, classes = (mu, var, pi), floor).  plain, k8: the phantom with the initial classes, K = 3 and 8;  bfield: b = 0.3 of
    the phantom's true log field;  dying: u = log v in [6, 7.2] with one class at mu = 20, var = 1e-6, whose posteriors underflow to 0;
    floor: the same volume with a class at the variance floor inside the data, where the exponent reaches 1e5;  big: 266 240 domain voxels"""
    if name in ("plain", "k8", "bfield", "big"):
        v, mask = case("bigall")[:2] if name == "big" else phantom(seed=SEEDS["phantom"])[:2]
        y, om = log_domain(v, mask)
        ini = init_classes(y[om], 8 if name == "k8" else 3)
        b = 0.3 * true_log_field(v.shape) if name == "bfield" else np.zeros(v.shape)
        return {"v": v, "mask": mask, "b": b, "classes": (ini["mu"], ini["var"], ini["pi"]), "floor": False}
    rng = np.random.default_rng(11)
    shape = (12, 10, 9)
    v = np.exp(rng.uniform(6.0, 7.2, size=shape))
    mask = (rng.random(shape) < 0.9).astype(np.uint8)
    mu3, floor = (20.0, False) if name == "dying" else (6.6, True)
    return {"v": v, "mask": mask, "b": np.zeros(shape), "floor": floor,
            "classes": (np.array([6.3, 6.9, mu3]), np.array([0.04, 0.04, VAR_FLOOR]), np.array([0.4, 0.4, 0.2]))}


EM_INPUTS = ("plain", "k8", "bfield", "dying", "floor", "big")


def em_reference(y, b, idx, mu, var, pi, dtype=np.longdouble):
    """one EM step and the final E-step's R, W on u = (y - b)[idx], every quantity the stage tests compare, in `dtype` -> dict(sums [3, K],
    sums_abs, classes = the kernel's update from those sums, R, W, R_abs, W_abs [N], lmax = the largest finite |l_k|).  u is the fp64 difference,
    one correctly rounded subtraction that is the same number on the device, taken as the input: a voxel whose u falls within rounding of
    a class mean would otherwise have an R that no fp64 evaluation can give to 1e-13 of sum_k |p_k (u - mu_k) / var_k|."""
    u = (np.asarray(y, dtype=np.float64).reshape(-1)[idx] - np.asarray(b, dtype=np.float64).reshape(-1)[idx]).astype(dtype)
    mu, var, pi = (np.asarray(a).astype(dtype) for a in (mu, var, pi))
    l = log_terms(u, mu, var, pi)
    p = e_step(u, mu, var, pi)
    sums, sums_abs = em_sums(p, u, mu)
    t = p * (u[None, :] - mu[:, None]) / var[:, None]
    R, W = residual_weights(p, u, mu, var)
    return {"sums": sums, "sums_abs": sums_abs, "classes": class_update(sums, mu, var, pi, u.size), "R": R, "W": W,
            "R_abs": np.abs(t).sum(axis=0), "W_abs": W, "lmax": float(np.abs(l[np.isfinite(l)]).max())}


def smooth_input(name):
    """-> (a [nx, ny, nz, 2], radii, weights, axis).  'A<axis>_<length>': one pass along an axis of 64, 65, 128, 129 or 131 samples with the
    other extents 21 and 1, or 3 and 7, and a radius of 64, 63, 17, 1, 64 in that order;  all3: 70 x 5 x 67 with radii 63, 17, 1 (y is
    shorter than its radius);  flat: 3 x 66 x 1 with radii 64, 0, 17.  The weights are positive, sum to 1 and are NOT symmetric, so a
    reversed kernel shows; the two channels carry different data."""
    if name == "all3":
        shape, radii, axis = (70, 5, 67), (63, 17, 1), None
    elif name == "flat":
        shape, radii, axis = (3, 66, 1), (64, 0, 17), None
    else:
        axis, L = int(name[1]), int(name[3:])
        i = (64, 65, 128, 129, 131).index(L)
        other = (21, 1) if i % 2 == 0 else (3, 7)
        shape = list(other)
        shape.insert(axis, L)
        radii = [2, 3]
        radii.insert(axis, (64, 63, 17, 1, 64)[i])
    rng = np.random.default_rng(1000 + sum(shape) + sum(radii))
    weights = []
    for r in radii:
        w = rng.uniform(0.2, 1.0, size=2 * r + 1)
        weights.append(w / w.sum())
    return rng.standard_normal(tuple(shape) + (2,)), tuple(radii), weights, axis


SMOOTH_INPUTS = tuple("A%d_%d" % (a, L) for a in range(3) for L in (64, 65, 128, 129, 131)) + ("all3", "flat")


def smooth_reference(a, radii, weights, axis, dtype=np.longdouble):
    """-> (the smoothed array in `dtype`, the same passes on |a| with |w|: the scale sum_t |w_t x_t| of the rounding)"""
    axes = range(3) if axis is None else (axis,)
    out, mag = np.asarray(a).astype(dtype), np.abs(np.asarray(a)).astype(dtype)
    for ax in axes:
        w = np.asarray(weights[ax]).astype(dtype)
        out, mag = smooth_axis(out, w, ax), smooth_axis(mag, np.abs(w), ax)
    return out, mag


def update_input(name):
    """-> (b, S [.., 2] = (S_R, S_W), idx).  small: 13 x 17 x 19; S_W is 0 (with S_R = 0) on a block and positive elsewhere, the domain a random
    part of D, so D is larger than Omega;  big: 64 x 64 x 65 with 263 000 domain voxels, 257 partials in the mean"""
    shape, N = ((13, 17, 19), 1025) if name == "small" else ((64, 64, 65), 263000)
    rng = np.random.default_rng(5 + len(name))
    b = 0.2 * rng.standard_normal(shape)
    S = np.stack([rng.standard_normal(shape), rng.uniform(0.5, 2.0, size=shape)], axis=-1)
    S[:2, :2, :] = 0.0
    S[0, 5, 3] = (0.0, 0.0)
    D = np.flatnonzero(S[..., 1].reshape(-1) > 0)
    idx = np.sort(rng.choice(D, size=N, replace=False)).astype(np.int32)
    return b, S, idx


UPDATE_INPUTS = ("small", "big")


def update_reference(b, S, idx, dtype=np.longdouble):
    """-> (new b, bmean, the scale of new b's rounding: |b| + |S_R / S_W| + |bmean|)"""
    nb = np.asarray(b).astype(dtype)
    SR, SW = S[..., 0].astype(dtype), S[..., 1].astype(dtype)
    om = np.zeros(nb.size, dtype=bool)
    om[idx] = True
    bmean = update_b(nb, SR, SW, om.reshape(nb.shape))
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.abs(np.asarray(b)) + np.where(SW > 0, np.abs(SR / SW), 0.0) + abs(bmean)
    return nb, bmean, scale


def revive_input():
    """-> (u [4001] as a 4001 x 1 x 1 volume's log, classes): a class that dies in the first EM step and would come back in the second if its
    log coefficient stayed finite.  Two clusters of 2000 voxels at 6.3 and 6.9 (sd 0.01) and one voxel at 8; classes at 6.3 and 6.9 with
    variance 0.01, the third at 9.5237 with variance 1e-3.  Step 1: at the voxel at 8 the third class' exponent lies 1100 below the largest
    (class 2's, -59), at every other voxel further still: every posterior underflows to exactly 0 in fp64, s_3 = 0, the class is dead.
    The step shrinks class 2's variance to 7e-4, its exponent at the voxel at 8 falls to about -850, and the dead class' old exponent,
    -1159, would now be only 300 below the maximum: a posterior of 1e-133, not 0.  The header says the class has p = 0 from then on."""
    rng = np.random.default_rng(3)
    u = np.concatenate([6.3 + 0.01 * rng.standard_normal(2000), 6.9 + 0.01 * rng.standard_normal(2000), [8.0]])
    return u.reshape(-1, 1, 1), (np.array([6.3, 6.9, 9.5237]), np.array([0.01, 0.01, 1e-3]), np.array([0.4, 0.4, 0.2]))
