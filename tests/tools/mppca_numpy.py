"""Marchenko-Pastur PCA denoising (Veraart et al., NeuroImage 2016) restated with numpy.linalg.eigh: the specification of
met2_mppca (include/met2_hip.h), voxel by voxel, for the tests.  Nothing here is fast.

For every voxel v with mask != 0: the patch is the cube of side `window` centred on v, clipped at the volume's faces and restricted
to voxels with mask != 0 (N of them; v is one).  X [M, N] holds their decay curves, not centred; r = min(M, N), q = max(M, N).
C = X X^T, eigenvalues ascending, lambda_p = max(ev[M - r + p], 0) / q for p = 0..r-1.  The threshold loop

    clam = 0; cut = 0; sigma2 = 0
    for p in 0..r-1:  clam += lambda_p;  gamma = (p + 1) / q;  s1 = clam / (p + 1);  s2 = (lambda_p - lambda_0) / (4 sqrt(gamma))
                      if s2 < s1:  sigma2 = s1;  cut = p + 1

leaves k = r - cut signal components; out[v] = U_s (U_s^T x_v) with U_s the eigenvectors of the k largest eigenvalues,
sigma[v] = sqrt(sigma2), rank[v] = k.  mask == 0: zeros and rank 0.  N < 2: copied through, sigma 0, rank 1.  A non-finite value in
the patch: copied through, sigma 0, rank -1.

The rank is a discrete decision.  Two numbers say how close a voxel's decision is to a tie, so that a comparison of another
implementation against this one can tell a rounding-level flip from a fault:
    margin = min over p >= 1 of |s2 - s1| / s1     (p = 0 has s2 = 0 < s1 whenever lambda_0 > 0: no decision there)
    gap    = (lambda_cut - lambda_{cut-1}) / lambda_max  when 0 < k < r: the eigenvalue gap at the cut (the projector is
             ill-determined when it closes)
Both are inf where they do not apply."""
import numpy as np

TIE = 1e-6      # a voxel with margin < TIE or gap < TIE is a tie by this restatement's own account


def patch_indices(mask, x, y, z, window):
    """flat C-order indices of the voxels of v's patch, in memory order"""
    nx, ny, nz = mask.shape
    h = window // 2
    xs = np.arange(max(x - h, 0), min(x + h + 1, nx))
    ys = np.arange(max(y - h, 0), min(y + h + 1, ny))
    zs = np.arange(max(z - h, 0), min(z + h + 1, nz))
    idx = (xs[:, None, None] * ny + ys[None, :, None]) * nz + zs[None, None, :]
    idx = idx.reshape(-1)
    return idx[mask.reshape(-1)[idx] != 0]


def threshold(lam, q):
    """the loop above on the ascending spectrum lam [r] -> (cut, sigma2, margin)"""
    clam = 0.0
    cut = 0
    sigma2 = 0.0
    margin = np.inf
    for p in range(lam.shape[0]):
        clam += lam[p]
        gamma = (p + 1) / q
        s1 = clam / (p + 1)
        s2 = (lam[p] - lam[0]) / (4.0 * np.sqrt(gamma))
        if s2 < s1:
            sigma2 = s1
            cut = p + 1
        if p >= 1 and s1 > 0:
            margin = min(margin, abs(s2 - s1) / s1)
    return cut, sigma2, margin


def spectrum(X, route="eigh"):
    """X [M, N] -> (lam [r] ascending, U [M, r] the matching orthonormal vectors).  route='svd' takes the same quantities from the
    singular values of X (the check of the eigh route)."""
    M, N = X.shape
    r, q = min(M, N), max(M, N)
    if route == "eigh":
        ev, U = np.linalg.eigh(X @ X.T)
        return np.maximum(ev[M - r:], 0.0) / q, U[:, M - r:]
    U, s, _ = np.linalg.svd(X, full_matrices=False)              # descending
    return (s[::-1] ** 2) / q, U[:, ::-1]


def mppca_voxel(X, xv, route="eigh"):
    """one patch X [M, N] and the centre's curve xv [M] -> (out [M], sigma, rank, margin, gap)"""
    M, N = X.shape
    r, q = min(M, N), max(M, N)
    lam, U = spectrum(X, route)
    cut, sigma2, margin = threshold(lam, q)
    k = r - cut
    gap = np.inf
    if 0 < k < r and lam[-1] > 0:
        gap = (lam[cut] - lam[cut - 1]) / lam[-1]
    Us = U[:, r - k:]
    return Us @ (Us.T @ xv), np.sqrt(sigma2), k, margin, gap


def mppca(data, mask, window=5, route="eigh"):
    """data [nx, ny, nz, M], mask [nx, ny, nz] -> dict(out, sigma, rank, margin, gap, n): n is the patch's voxel count"""
    data = np.ascontiguousarray(data, dtype=np.float64)
    mask = np.ascontiguousarray(mask)
    if window < 3 or window % 2 == 0:
        raise ValueError("window must be odd and >= 3")
    nx, ny, nz, M = data.shape
    flat = data.reshape(-1, M)
    out = np.zeros_like(data)
    sigma = np.zeros((nx, ny, nz))
    rank = np.zeros((nx, ny, nz), dtype=np.int32)
    margin = np.full((nx, ny, nz), np.inf)
    gap = np.full((nx, ny, nz), np.inf)
    count = np.zeros((nx, ny, nz), dtype=np.int32)
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                if mask[x, y, z] == 0:
                    continue
                idx = patch_indices(mask, x, y, z, window)
                count[x, y, z] = idx.size
                X = flat[idx].T
                xv = data[x, y, z]
                if not np.isfinite(X).all():
                    out[x, y, z] = xv
                    rank[x, y, z] = -1
                elif idx.size < 2:
                    out[x, y, z] = xv
                    rank[x, y, z] = 1
                else:
                    out[x, y, z], sigma[x, y, z], rank[x, y, z], margin[x, y, z], gap[x, y, z] = mppca_voxel(X, xv, route)
    return {"out": out, "sigma": sigma, "rank": rank, "margin": margin, "gap": gap, "n": count}


def ties(res):
    """the voxels whose decision this restatement itself calls a tie"""
    return (res["margin"] < TIE) | (res["gap"] < TIE)


def two_pool_volume(shape, M, seed, peak=1000.0, noise=10.0, holes=2, edge_line=False):
    """A test volume: a two-pool decay with spatial gradients in the fractions and the T2s, Gaussian noise in both channels, magnitude
    taken; a mask with `holes` voxels cleared, and with edge_line the line [0, :, 0] too.  -> (data [nx, ny, nz, M], mask uint8)"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny), np.linspace(0, 1, nz), indexing="ij")
    te = 10.0 * (1 + np.arange(M))
    f = 0.1 + 0.15 * gx
    t2a = 15.0 + 10.0 * gy
    t2b = 70.0 + 30.0 * gz
    s = peak * (f[..., None] * np.exp(-te / t2a[..., None]) + (1 - f[..., None]) * np.exp(-te / t2b[..., None]))
    s = np.abs(s + noise * rng.standard_normal(s.shape) + 1j * noise * rng.standard_normal(s.shape))
    mask = np.ones(shape, dtype=np.uint8)
    for _ in range(holes):
        mask[rng.integers(nx), rng.integers(ny), rng.integers(nz)] = 0
    if edge_line:
        mask[0, :, 0] = 0
    return s * mask[..., None], mask


# The volumes the GPU tests compare on: name -> (shape, M, window, seed, edge_line).  tests/test_mppca_host.py asserts that the restatement
# calls no voxel of any of them a tie.
CASES = {
    "parity": ((9, 8, 7), 32, 5, 1, True),          # corner patches N = 27 < M, interior N = 125 > M
    "M2": ((5, 4, 3), 2, 3, 6, False),
    "M7": ((5, 4, 3), 7, 3, 7, False),
    "M16": ((5, 4, 3), 16, 3, 8, False),
    "M33": ((5, 4, 3), 33, 3, 5, False),            # N <= 27 < M
    "M63": ((5, 4, 3), 63, 3, 4, False),
    "M3": ((5, 4, 3), 3, 3, 24, False),             # G = 21 pairs' room, two pairs
    "M21": ((5, 4, 3), 21, 3, 20, False),           # G = 3
    "M22": ((5, 4, 3), 22, 3, 18, False),           # G = 2
    "M31": ((5, 4, 3), 31, 3, 26, False),           # odd: a dummy player, G = 2
    "M62": ((5, 4, 3), 62, 3, 14, False),           # the even maximum
    "W7M63": ((7, 7, 7), 63, 7, 54, False),         # the longest patch list (343 entries) beside the largest matrices
    "wide": ((3, 9, 2), 12, 7, 9, False),           # the window wider than the volume
    "tiny": ((2, 2, 2), 12, 3, 10, False),
    "driver": ((8, 8, 4), 32, 5, 12, False),
}


def case(name):
    """-> (data, mask, window)"""
    shape, M, w, seed, edge = CASES[name]
    data, mask = two_pool_volume(shape, M, seed, edge_line=edge)
    return data, mask, w


# ---- matrix cases: a cube of side w whose centre voxel's patch (window w) is the whole cube, so that the centre's C = X X^T is a matrix the
# test chose.  tests/test_gpu_mppca_stages.py looks at the centre voxel of each; tests/test_mppca_host.py at what eigh makes of them.

def cube(X, n2=False):
    """X [M, N] with N = w^3 (w = 3, 5, 7) -> (data [w, w, w, M], mask, w): voxel n of the cube, in memory order, holds column n.  n2: the mask
    keeps the centre and the voxel before it only (N = 2)."""
    M, N = X.shape
    w = int(round(N ** (1.0 / 3.0)))
    assert w ** 3 == N and w in (3, 5, 7)
    data = np.ascontiguousarray(X.T).reshape(w, w, w, M)
    mask = np.ones((w, w, w), dtype=np.uint8)
    if n2:
        mask[...] = 0
        mask[w // 2, w // 2, w // 2 - 1:w // 2 + 1] = 1
        data = data * mask[..., None]
    return data, mask, w


def from_spectrum(spec, N, seed):
    """X [M, N] = Q sqrt(diag(spec)) W^T with Q [M, M] and W [N, M] orthonormal (N >= M): X X^T = Q diag(spec) Q^T up to rounding"""
    spec = np.asarray(spec, dtype=np.float64)
    M = spec.size
    assert N >= M
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((M, M)))
    W, _ = np.linalg.qr(rng.standard_normal((N, M)))
    return (Q * np.sqrt(spec)) @ W.T


def two_pool_matrix(M, N, seed):
    """two-pool curves of N voxels as X [M, N]"""
    w = int(round(N ** (1.0 / 3.0)))
    data, _ = two_pool_volume((w, w, w), M, seed, holes=0)
    return np.ascontiguousarray(data.reshape(N, M).T)


def equal_diagonal(M, N, a):
    """voxel n holds a e_(n mod M): with M | N every echo is hit N / M times and C = (N / M) a^2 I exactly"""
    assert N % M == 0
    X = np.zeros((M, N))
    X[np.arange(N) % M, np.arange(N)] = a
    return X


TWO_POOL_M = (2, 3, 7, 21, 22, 31, 32, 33, 62, 63)          # the echo counts at which G = floor(64 / M) or the tournament's shape changes


def _special(name):
    rng = np.random.default_rng(100 + sorted(SPECIAL).index(name))
    if name == "noise":                                      # zero-mean Gaussian noise: the rule keeps nothing
        return rng.standard_normal((32, 125)) * 10.0
    if name == "rank1":
        return from_spectrum([0.0] * 31 + [5.0e6], 125, 21)
    if name == "rank2":
        return from_spectrum([0.0] * 30 + [3.0e4, 5.0e6], 125, 22)
    if name == "identical":                                  # every voxel the same curve
        return np.repeat(two_pool_matrix(32, 125, 23)[:, :1], 125, axis=1)
    if name == "constant":
        return np.full((32, 125), 37.0)
    if name == "zero":
        return np.zeros((32, 125))
    X = two_pool_matrix(32, 125, 24)
    if name == "zero_echoes":
        X[[5, 20]] = 0.0
    if name == "dup_echoes":
        X[17] = X[4]
    return X


SPECIAL = {"noise", "rank1", "rank2", "identical", "constant", "zero", "zero_echoes", "dup_echoes"}
SPECTRA = {
    "clustered": ([1.0] * 10 + [4.0] * 10 + [9.0] * 12, 125),
    "graded32": ([10.0 ** -p for p in range(32)], 125),
    "graded63": ([10.0 ** (-p / 4.0) for p in range(63)], 343),
}
EQUAL_DIAGONAL = {"eqdiag_M3": (3, 27, 3.0), "eqdiag_M25": (25, 125, 0.75)}


def matrix_case_names():
    names = ["tp_M%d_N%d" % (M, N) for M in TWO_POOL_M for N in (2, 27, 125)] + ["tp_M63_N343", "tp_M32_N343"]
    return names + sorted(SPECIAL) + sorted(SPECTRA) + sorted(EQUAL_DIAGONAL)


def matrix_case(name):
    """-> (data [w, w, w, M], mask, w): the centre voxel's patch is the whole cube (for ..._N2 the centre and one neighbour)"""
    if name.startswith("tp_"):
        M, N = (int(s[1:]) for s in name.split("_")[1:])
        return cube(two_pool_matrix(M, max(N, 27), 40 + M), n2=(N == 2))
    if name in SPECIAL:
        return cube(_special(name))
    if name in SPECTRA:
        spec, N = SPECTRA[name]
        return cube(from_spectrum(spec, N, 30 + len(spec)))
    M, N, a = EQUAL_DIAGONAL[name]
    return cube(equal_diagonal(M, N, a))


def centre(w):
    """the flat index of the cube's centre voxel"""
    return (w ** 3) // 2


def eig_figures(Cm, d, V):
    """how good (d, V) is as an eigensystem of the symmetric Cm, each figure relative to ||Cm||_2 (1 where Cm is zero): the residual
    ||Cm V - V diag(d)||_2, max |V^T V - I| (absolute: V has unit scale), max |sort(d) - eigvalsh(Cm)| and |tr Cm - sum d|.  The products are
    taken in long double so that the figures are those of (d, V) and not of this function."""
    Cm = np.asarray(Cm, dtype=np.float64)
    L = np.longdouble
    nrm = np.linalg.norm(Cm, 2)
    nrm = float(nrm) if nrm > 0 else 1.0
    R = Cm.astype(L) @ V.astype(L) - V.astype(L) * d.astype(L)[None, :]
    O = V.astype(L).T @ V.astype(L) - np.eye(V.shape[0], dtype=L)
    return {"residual": float(np.linalg.norm(R.astype(np.float64), 2)) / nrm,
            "orth": float(np.abs(O).max()),
            "eigval": float(np.abs(np.sort(d) - np.linalg.eigvalsh(Cm)).max()) / nrm,
            "trace": float(abs(np.trace(Cm.astype(L)) - d.astype(L).sum())) / nrm}


EIG_MARGIN = 50.0           # Jacobi applies some hundreds of rotations per column where LAPACK applies O(M) reflectors


def eig_bounds(Cm):
    """the bound of each figure for a solver under test: EIG_MARGIN times np.linalg.eigh's own figure on the same matrix, floored at M 2^-52"""
    d, V = np.linalg.eigh(Cm)
    own = eig_figures(Cm, d, V)
    floor = Cm.shape[0] * 2.0 ** -52
    return {k: max(EIG_MARGIN * v, floor) for k, v in own.items()}, own


def threshold_from_eigval(d, N):
    """the kernel's step 4 on the solver's unsorted diagonal d [M] with N patch voxels: the stable ascending order (ties by index), lambda =
    max(d, 0) / q of the top r, the threshold loop -> (k, sigma, order, lam): order[M - k:] are the indices of the kept eigenvectors"""
    d = np.asarray(d, dtype=np.float64)
    M = d.size
    r, q = min(M, N), max(M, N)
    order = np.argsort(d, kind="stable")
    lam = np.maximum(d[order][M - r:], 0.0) / float(q)
    cut, sigma2, _ = threshold(lam, q)
    return r - cut, np.sqrt(sigma2), order, lam
