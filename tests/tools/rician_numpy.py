"""numpy / scipy.special restatement of the Rician noise-floor correction of include/met2_hip.h ("Rician noise floor"): the reference of
tests/test_gpu_rician.py, checked itself against mpmath in tests/test_rician_host.py.  Written from the header's formulas; not fast.

  mean(A, sigma)      m = sigma sqrt(pi / 2) [(1 + t) i0e(t / 2) + t i1e(t / 2)], t = A^2 / (2 sigma^2)
  bias(A, sigma)      m - A by plain subtraction (A < 0 reads as 0, sigma = 0 gives 0)
  step(...)           data - bias(model, sigma_v) with the fit's gate on the corrected row
  invert(M, sigma)    the root of mean(A, sigma) = M by bisection inside the bracket [sqrt(max(M^2 - 2 sigma^2, 0)), M]
  loop(...)           met2_fit_rician's passes around a fit the caller passes in
  mp_bias, mp_forward_residual   the yardsticks: the same from mpmath at 50 digits"""
import numpy as np
from scipy.special import i0e, i1e

FLOOR = np.sqrt(np.pi / 2.0)


def mean(A, sigma):
    A, sigma = np.broadcast_arrays(np.asarray(A, dtype=np.float64), np.asarray(sigma, dtype=np.float64))
    A = np.maximum(A, 0.0)
    ok = sigma > 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        t = np.where(ok, A * A / (2.0 * np.where(ok, sigma, 1.0) ** 2), 0.0)
        m = sigma * FLOOR * ((1.0 + t) * i0e(t / 2.0) + t * i1e(t / 2.0))
    return np.where(ok, m, A)


def bias(A, sigma):
    A, sigma = np.broadcast_arrays(np.asarray(A, dtype=np.float64), np.asarray(sigma, dtype=np.float64))
    return np.where(sigma > 0, mean(A, sigma) - np.maximum(A, 0.0), 0.0)


def step(data, model, sigma, mask=None, b=None):
    """data, model [nvox, n_te]; sigma, mask [nvox].  Returns (out, flag).  b: the bias to subtract when it comes from elsewhere (the device's
    own entry, for the bit-for-bit test); the gate's sum is np.sum over the row, so a row within rounding of the gate may differ."""
    data = np.asarray(data, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    live = sigma > 0 if mask is None else (sigma > 0) & (np.asarray(mask) != 0)
    if b is None:
        b = bias(model, sigma[:, None])
    out = np.where(live[:, None], data - b, data)
    bad = live & ~((out[:, 0] > 0) & (out.sum(axis=1) > 0))
    out[bad] = data[bad]
    return out, bad.astype(np.int32)


def invert(M, sigma, iters=200):
    M, sigma = np.broadcast_arrays(np.asarray(M, dtype=np.float64), np.asarray(sigma, dtype=np.float64))
    shape = M.shape
    M, sigma = M.reshape(-1), sigma.reshape(-1)
    out = M.copy()
    live = sigma > 0
    s = np.where(live, sigma, 1.0)
    mu = M / s
    above = live & (mu > FLOOR)
    out[live & ~above] = 0.0
    if above.any():
        u = mu[above]
        lo, hi = np.sqrt(np.maximum(u * u - 2.0, 0.0)), u.copy()
        for _ in range(iters):                                      # plain bisection: 200 halvings end at neighbouring doubles
            mid = 0.5 * (lo + hi)
            up = mean(mid, 1.0) > u
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
        a = 0.5 * (lo + hi)
        # of the bracket's ends and its midpoint, the one whose forward value lies nearest
        cand = np.stack([lo, a, hi])
        res = np.abs(mean(cand, 1.0) - u[None, :])
        a = cand[np.argmin(res, axis=0), np.arange(u.shape[0])]
        out[above] = a * s[above]
    return out.reshape(shape)


def loop(fit, data, sigma, n_iter, mask=None):
    """met2_fit_rician around fit(y) -> (fsol, sig, fitted [nvox] bool): y^0 = data; y^(k+1) = step(data, sig^k, sigma) on the voxels fitted in
    pass 0.  Returns (fsol, sig, flag, history of sig)."""
    data = np.asarray(data, dtype=np.float64)
    fsol, sig, fitted0 = fit(data)
    hist = [sig.copy()]
    flag = np.zeros(data.shape[0], dtype=np.int32)
    m0 = fitted0 if mask is None else fitted0 & (np.asarray(mask) != 0)
    for _ in range(n_iter):
        y, flag = step(data, sig, sigma, m0)
        fsol, sig, _ = fit(y)
        hist.append(sig.copy())
    return fsol, sig, flag, hist


def _mp_mean(mp, A, sigma):
    A, sigma = mp.mpf(float(A)), mp.mpf(float(sigma))
    A = max(A, mp.mpf(0))
    if sigma == 0:
        return A
    t = A * A / (2 * sigma * sigma)
    e = mp.exp(-t / 2)
    return sigma * mp.sqrt(mp.pi / 2) * ((1 + t) * e * mp.besseli(0, t / 2) + t * e * mp.besseli(1, t / 2))


def mp_bias(A, sigma, dps=50):
    """b(A, sigma) from mpmath at `dps` digits, rounded to float64 at the end"""
    import mpmath as mp
    with mp.workdps(dps):
        return float(_mp_mean(mp, A, sigma) - max(mp.mpf(float(A)), mp.mpf(0))) if sigma > 0 else 0.0


def mp_forward_residual(A, sigma, M, dps=50):
    """|m(A, sigma) - max(M, sigma sqrt(pi / 2))| from mpmath at `dps` digits: the inverse's figure of merit"""
    import mpmath as mp
    with mp.workdps(dps):
        target = max(mp.mpf(float(M)), mp.mpf(float(sigma)) * mp.sqrt(mp.pi / 2))
        return float(abs(_mp_mean(mp, A, sigma) - target))
