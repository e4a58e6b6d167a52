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


def bias_field(v, mask=None, voxel_size=(1.0, 1.0, 1.0), n_class=3, n_outer=4, n_em=10, fwhm=20.0, dtype=np.float64, init_shift=None,
               trace=None):
    """-> dict(out, field, classes [3 K] = mu, var, pi, b, omega, support).  init_shift = (k, bins) moves the initial mean of class k by
    whole histogram bins (tests only); trace, a list, receives (outer, em, s) after every M-step."""
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


SEEDS = {"phantom": 1, "thin": 254, "wave": 6, "coarse": 63, "coarse80": 63, "k8floor": 2, "holes": 2, "k1": 1, "k8": 5, "outer0": 1}
CASES = tuple(SEEDS)
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
    k1, k8    the phantom with 1 and 8 classes;  outer0: n_outer = 0"""
    seed = SEEDS[name] if seed is None else seed
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
