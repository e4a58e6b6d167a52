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
    "wide": ((3, 9, 2), 12, 7, 9, False),           # the window wider than the volume
    "tiny": ((2, 2, 2), 12, 3, 10, False),
    "driver": ((8, 8, 4), 32, 5, 12, False),
}


def case(name):
    """-> (data, mask, window)"""
    shape, M, w, seed, edge = CASES[name]
    data, mask = two_pool_volume(shape, M, seed, edge_line=edge)
    return data, mask, w
