"""numpy restatements for the group statistics (include/met2_hip.h: met2_group_perm_stats; multicomponent-t2-toolbox_amd/group.py).

perm_stats      the entry, in the entry's order of summation, in any dtype: long double is the accuracy reference, float64 gives the entry's
                bits.  The order (the header states it, this restates it): every sum over the subjects starts from 0.0 and takes its terms one
                by one, a <- a + W[k][j][i] Y[i][v] for i = 0 .. n - 1, product and sum rounded separately; q = g_1 g_1, then q <- q + g_j g_j for
                j = 2 .. r; rss = s0 - q; t = rss > 0 ? b / sqrt(rss) : 0; two_sided: |t|.
batch_stat      perm_stats in float64 with randomise's batch_stat signature: the host stand-in for the device entry
freedman_lane_t an independent restatement that makes no use of the weight form: per permutation y* = (P R_z + H_z) y, the full model
                [x1 Z] fitted with lstsq, the textbook t of the first coefficient
ols_t           the textbook t of a contrast in the original design"""
import numpy as np

LD = np.longdouble


def perm_t(Y, s0, W, two_sided=False, dtype=np.float64, chunk=16):
    """t [K, V] and rss / s0 [K, V] in `dtype`, in the entry's order"""
    Y, s0, W = (np.asarray(a, dtype=dtype) for a in (Y, s0, W))
    n, V = Y.shape
    K, r1 = W.shape[0], W.shape[1]
    t, ratio = np.empty((K, V), dtype=dtype), np.empty((K, V), dtype=dtype)
    for k0 in range(0, K, chunk):
        w = W[k0:k0 + chunk]
        acc = np.zeros((w.shape[0], r1, V), dtype=dtype)
        for i in range(n):
            acc = acc + w[:, :, i, None] * Y[i][None, None, :]
        q = acc[:, 1] * acc[:, 1]
        for j in range(2, r1):
            q = q + acc[:, j] * acc[:, j]
        rss = s0[None, :] - q
        pos = rss > 0
        tt = np.where(pos, acc[:, 0] / np.sqrt(np.where(pos, rss, 1)), 0)
        t[k0:k0 + chunk] = np.abs(tt) if two_sided else tt
        ratio[k0:k0 + chunk] = rss / np.where(s0 != 0, s0, 1)[None, :]
    return t, ratio


def perm_stats(Y, s0, W, two_sided=False, t_ref=None, dtype=np.float64):
    """-> dict(t [K, V], ratio [K, V], kmax [K], count [V] uint32 or None): the entry's outputs (count: the increment)"""
    t, ratio = perm_t(Y, s0, W, two_sided, dtype)
    kmax = t.max(axis=1) if t.shape[1] else np.full(t.shape[0], -np.inf)
    count = None if t_ref is None else (t >= np.asarray(t_ref, dtype=dtype)[None, :]).sum(axis=0).astype(np.uint32)
    return {"t": t, "ratio": ratio, "kmax": kmax, "count": count}


def batch_stat(Y, s0, W, two_sided, t_ref, want_first):
    """randomise's batch_stat: the entry in float64 -> (kmax, count increment or None, t_first or None)"""
    s = perm_stats(Y, s0, W, two_sided, t_ref, np.float64)
    return s["kmax"], s["count"], (s["t"][0].copy() if want_first else None)


def perm_matrix(index, sign):
    """P with (P y)_i = sign[i] y[index[i]]"""
    n = len(index)
    P = np.zeros((n, n))
    P[np.arange(n), index] = sign
    return P


def freedman_lane_t(Y, x1, Z, index, sign):
    """t [P, V] of the coefficient of x1, for the signed permutations (index [P, n], sign [P, n]), by the scheme's own steps"""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    Hz = Z @ np.linalg.pinv(Z) if Z.shape[1] else np.zeros((n, n))
    Rz = np.eye(n) - Hz
    M = np.hstack([x1, Z])
    dof = n - np.linalg.matrix_rank(M)
    var_factor = np.linalg.inv(M.T @ M)[0, 0]
    out = np.empty((len(index), Y.shape[1]))
    for k in range(len(index)):
        ystar = (perm_matrix(index[k], sign[k]) @ Rz + Hz) @ Y
        beta = np.linalg.lstsq(M, ystar, rcond=None)[0]
        res = ystar - M @ beta
        sigma2 = np.sum(res * res, axis=0) / dof
        out[k] = beta[0] / np.sqrt(sigma2 * var_factor)
    return out


def ols_t(Y, X, c):
    """the textbook t of c' beta in Y = X beta + e -> (t [V], cope [V], dof)"""
    Y, X = np.asarray(Y, dtype=np.float64), np.asarray(X, dtype=np.float64)
    X = X[:, None] if X.ndim == 1 else X
    c = np.asarray(c, dtype=np.float64).ravel()
    beta = np.linalg.lstsq(X, Y, rcond=None)[0]
    res = Y - X @ beta
    dof = X.shape[0] - np.linalg.matrix_rank(X)
    sigma2 = np.sum(res * res, axis=0) / dof
    cope = c @ beta
    return cope / np.sqrt(sigma2 * (c @ np.linalg.inv(X.T @ X) @ c)), cope, dof


# ---------------------------------------------------------------- the cases the host and the device tests share

def two_group_design(n=12):
    """two groups of n / 2 and a centred age covariate; the contrast is group 1 minus group 2"""
    g = np.repeat([1.0, 0.0], n // 2)
    age = np.random.default_rng(5).uniform(20.0, 60.0, n)
    return np.stack([g, 1.0 - g, age - age.mean()], axis=1), np.array([1.0, -1.0, 0.0])


def one_sample_design(n=8):
    return np.ones((n, 1)), np.array([1.0])


def planted_case(n=12, V=500, n_planted=20, shift=3.0, seed=17):
    """one-sample data, unit normal noise, +shift sigma in the first n_planted voxels -> (Y [n, V], X, c, planted [V] bool)"""
    Y = np.random.default_rng(seed).standard_normal((n, V))
    Y[:, :n_planted] += shift
    X, c = one_sample_design(n)
    planted = np.zeros(V, dtype=bool)
    planted[:n_planted] = True
    return Y, X, c, planted


def null_case(n=12, V=500, seed=18):
    X, c = one_sample_design(n)
    return np.random.default_rng(seed).standard_normal((n, V)), X, c
