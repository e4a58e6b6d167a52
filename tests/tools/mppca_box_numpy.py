"""MP-PCA denoising with a box window and the average over the overlapping patches, restated with numpy: the specification of
met2_mppca_box (include/met2_hip.h), voxel by voxel, for the tests.  Nothing here is fast.  The decomposition of a patch (spectrum,
threshold) and the account of ties (TIE, margin, gap) are those of mppca_numpy.py, which states met2_mppca.

window = (wx, wy, wz), each odd and >= 1, at least 3 voxels.  The patch of a voxel c with mask != 0 is the box of half-widths
(wx // 2, wy // 2, wz // 2) around it, clipped at the volume's faces, restricted to mask != 0, in memory order; it gives k_c, sigma_c and U_c,
the eigenvectors of the k_c largest eigenvalues.  A centre is in a copy-through class if N < 2 (rank 1) or its patch holds a non-finite
value (rank -1).

average=False: out[v] = U_v (U_v^T x_v), sigma[v] = sigma_v, rank[v] = k_v, wsum[v] = 0.
average=True:  C(v) = the masked voxels of the same clipped box around v, in memory order; a centre votes unless it is in a copy-through
class, with weight w_c = 1 / (1 + k_c):  out[v] = sum_c w_c U_c (U_c^T x_v) / sum_c w_c,  sigma[v] = sum_c w_c sigma_c / sum_c w_c,
rank[v] = k_v, wsum[v] = sum_c w_c; no voting centre: out[v] = x_v, sigma[v] = 0, wsum[v] = 0.
mask == 0: zeros everywhere.

tie[v]: with average=False whether v's own decision is a tie (margin or gap below TIE); with average=True whether that of any centre of
C(v) is, since every one of them enters out[v]."""
import numpy as np

from mppca_numpy import TIE, spectrum, threshold


def box_indices(mask, x, y, z, window):
    """flat C-order indices of the masked voxels of the clipped box around (x, y, z), in memory order"""
    nx, ny, nz = mask.shape
    hx, hy, hz = (w // 2 for w in window)
    xs = np.arange(max(x - hx, 0), min(x + hx + 1, nx))
    ys = np.arange(max(y - hy, 0), min(y + hy + 1, ny))
    zs = np.arange(max(z - hz, 0), min(z + hz + 1, nz))
    idx = ((xs[:, None, None] * ny + ys[None, :, None]) * nz + zs[None, None, :]).reshape(-1)
    return idx[mask.reshape(-1)[idx] != 0]


def check_window(window):
    window = tuple(int(w) for w in window)
    if len(window) != 3 or any(w < 1 or w % 2 == 0 for w in window) or window[0] * window[1] * window[2] < 3:
        raise ValueError("window must be three odd sizes >= 1 holding at least 3 voxels")
    return window


def decompose(flat, idx):
    """the patch `idx` of the curves flat [nvox, M] -> (rank, sigma, Us [M, k] or None for a copy-through class, tie)"""
    X = flat[idx].T
    M, N = X.shape
    if not np.isfinite(X).all():
        return -1, 0.0, None, False
    if N < 2:
        return 1, 0.0, None, False
    r, q = min(M, N), max(M, N)
    lam, U = spectrum(X)
    cut, sigma2, margin = threshold(lam, q)
    k = r - cut
    gap = np.inf
    if 0 < k < r and lam[-1] > 0:
        gap = (lam[cut] - lam[cut - 1]) / lam[-1]
    return k, np.sqrt(sigma2), U[:, r - k:], bool(margin < TIE or gap < TIE)


def mppca_box(data, mask, window, average=False):
    """data [nx, ny, nz, M], mask [nx, ny, nz] -> dict(out, sigma, rank, n, wsum, tie)"""
    data = np.ascontiguousarray(data, dtype=np.float64)
    mask = np.ascontiguousarray(mask)
    window = check_window(window)
    nx, ny, nz, M = data.shape
    flat = data.reshape(-1, M)
    nvox = flat.shape[0]
    on = np.flatnonzero(mask.reshape(-1) != 0)
    coords = np.stack(np.unravel_index(np.arange(nvox), (nx, ny, nz)), axis=1)
    patch = {v: box_indices(mask, *coords[v], window) for v in on}
    dec = {v: decompose(flat, patch[v]) for v in on}
    out = np.zeros((nvox, M))
    sigma, wsum = np.zeros(nvox), np.zeros(nvox)
    rank, count = np.zeros(nvox, dtype=np.int32), np.zeros(nvox, dtype=np.int32)
    tie = np.zeros(nvox, dtype=bool)
    for v in on:
        k, s, Us, t = dec[v]
        rank[v], count[v] = k, patch[v].size
        if not average:
            out[v], sigma[v], tie[v] = (flat[v], 0.0, False) if Us is None else (Us @ (Us.T @ flat[v]), s, t)
            continue
        acc, ssum = np.zeros(M), 0.0
        for c in patch[v]:                                         # the box is symmetric: the patch of v lists the centres that hold v
            kc, sc, Uc, tc = dec[c]
            tie[v] |= tc
            if Uc is None:
                continue
            w = 1.0 / (1.0 + kc)
            acc += w * (Uc @ (Uc.T @ flat[v]))
            ssum += w * sc
            wsum[v] += w
        out[v], sigma[v] = (acc / wsum[v], ssum / wsum[v]) if wsum[v] > 0 else (flat[v], 0.0)
    shape = (nx, ny, nz)
    return {"out": out.reshape(data.shape), "sigma": sigma.reshape(shape), "rank": rank.reshape(shape), "n": count.reshape(shape),
            "wsum": wsum.reshape(shape), "tie": tie.reshape(shape)}


def holed_volume(shape, M, seed, isolated=True):
    """A test volume of mppca_numpy.two_pool_volume with holes in the mask and, with `isolated`, one masked voxel all of whose neighbours
    (within three voxels, as far as the volume reaches) are cleared: its patch is itself under every window up to 7.  Volumes too small to
    hold such a voxel and anything else get none.  -> (data, mask uint8)"""
    from mppca_numpy import two_pool_volume
    raw, mask = two_pool_volume(shape, M, seed, holes=4)          # (the curves are already multiplied by this mask)
    if isolated and min(shape) >= 2 and np.prod(shape) > 200:
        x, y, z = shape[0] - 1, shape[1] - 1, 0
        mask[max(x - 3, 0):, max(y - 3, 0):, :4] = 0
        mask[x, y, z] = 1
        raw = raw * mask[..., None]                                # the isolated voxel lies in none of the holes: it keeps its curve
    return raw, mask


# The volumes tests/test_gpu_mppca_box.py compares on: name -> (shape, echoes, window, seed of holed_volume).  tests/test_mppca_box_host.py
# asserts that the restatement calls no voxel of any of them a tie.
CASES = {
    "w331_M3": ((9, 8, 7), 3, (3, 3, 1), 1),
    "w133_M12": ((9, 8, 7), 12, (1, 3, 3), 1),
    "w551_M32": ((9, 8, 7), 32, (5, 5, 1), 1),
    "w357_M33": ((9, 8, 7), 33, (3, 5, 7), 1),
    "w773_M63": ((9, 8, 7), 63, (7, 7, 3), 1),
    "w555_M32": ((9, 8, 7), 32, (5, 5, 5), 1),
    "thin_z": ((9, 8, 1), 12, (3, 3, 3), 1),                       # nz = 1 under wz = 3
    "thin_x": ((2, 8, 7), 12, (5, 5, 1), 1),                       # nx = 2 under wx = 5
    "seams": ((12, 5, 4), 12, (3, 3, 3), 1),                       # long along x: many pieces at the smallest work space
}


def case(name):
    """-> (data, mask, window)"""
    shape, M, window, seed = CASES[name]
    data, mask = holed_volume(shape, M, seed)
    return data, mask, window
