"""Voxel-wise group statistics with permutation inference (csrc/met2_group.hip; include/met2_hip.h states the entry's contract).

A general linear model Y = X beta + e over n subjects, a t-contrast c (or an F-contrast: several at once, below), and the permutation
distribution of the statistic at every voxel:
uncorrected p-values from the voxel's own distribution, family-wise-error-corrected ones from the distribution of the maximum over the voxels
(Winkler et al., NeuroImage 92:381-397, 2014).  One form covers one-sample sign flipping, the permutation of group labels and the
Freedman-Lane scheme with nuisance regressors:

  partition(X, c)        the effect of interest x1 and the nuisance Z with x1' Z = 0 (Beckmann's form), so that the coefficient of x1 in
                         [x1 Z] is c' beta
  residualise(Y, X, c)   Yr = R_z Y with R_z = I - Z Z+, and s0 = sum_i Yr^2 per voxel
  permutation_set(...)   signed permutations P_k, row 0 the identity, unique by the x1 they produce, exhaustive where that is affordable
  weights(X, c, perms)   W [P][r + 1][n]: row 0 = sqrt(dof) P_k' x1 / sqrt(x1' x1), rows 1 .. r = P_k' q_j for an orthonormal basis q_j of [x1 Z]

Freedman-Lane fits the full model to y* = (P_k R_z + H_z) y.  H_z y lies in the model's column space and x1 is orthogonal to Z, so the
coefficient of x1 is x1' P_k Yr / (x1' x1), the residual sum of squares is |P_k Yr|^2 - sum_j (q_j' P_k Yr)^2 = s0 - sum_j ((P_k' q_j)' Yr)^2
(a signed permutation keeps the norm), and t = b / sqrt(rss) with b = (row 0)' Yr: the statistic of met2_group_perm_stats.  The V x P table of
statistics is never formed: the entry keeps the maximum per candidate and the count per voxel.

perm_stats is the entry on arrays; randomise batches the candidates through it (or through batch_stat, a numpy callable with the entry's
meaning: the loop then needs no device).

Spatial statistics (csrc/met2_tfce.hip; the header states the definitions): tfce and cluster_extent transform maps on a grid;
randomise(tfce=..., cluster_threshold=..., grid=, at=) tests them by permutation through met2_group_perm_tfce (perm_tfce on arrays), which
computes every candidate's t with met2_group_perm_stats's own kernel code, keeps a batch of dense maps on the device and returns, as the t
entry does, one maximum per candidate and one count per voxel.  dh defaults to a hundredth of the observed map's maximum and is the same for
every permutation; a level holds the voxels with t >= h (not >); a map is followed up to MET2_TFCE_MAX_STEPS = 1 024 levels, i.e. with the
default dh to 10.24 times the observed maximum, and treated above that as if it stopped there -- three places where FSL's randomise -T may
differ.  One-sided only: on |t| a positive and a negative blob would fuse into one cluster, so test c and -c.

F-contrasts (randomise(f_contrast=[s, p]); met2_group_perm_fstats, met2_group_perm_ftfce): partition, residualise and permutation_set take a
contrast matrix C [p, s] of rank s and give x1 [n, s]; weights_f gives W [P][r][n], rows P_k' q_j of the QR basis of [x1 Z], whose first s
span x1.  F = ((n - r) / s) qs / (s0 - q) with qs the sum of the first s squared sums and q of all r: the Freedman-Lane F of the full model
against the nuisance, by the argument above with |Q1' P_k Yr|^2 in the place of b^2.  perm_fstats and perm_ftfce are the entries on arrays.
TFCE and the cluster extent are taken on F itself, with the same E, H and dh rule.

Variance smoothing (randomise(variance_smoothing=sigma_vox); csrc/met2_group_vsm.hip; the header states the definitions): for small samples
the residual variance is pooled over a Gaussian neighbourhood inside the mask, sigma2 = S(rho) / S(mask) with rho = max(rss, 0) and S three
separable passes with the taps of smoothing_taps, and the statistic is the pseudo-t b / sqrt(sigma2) (Holmes et al. 1996; Nichols & Holmes
2002).  met2_group_perm_vsm (perm_vsm on arrays) computes b and rss with met2_group_perm_stats's own kernel code, smooths a batch of dense maps
on the device and then either gathers the pseudo-t (maximum per candidate, count per voxel) or hands the maps to the TFCE / extent machinery
above.  masked_smooth is the smoothing on its own.  Radii up to 16 voxels (sigma <= 16 / 3 voxels), batches of at most 32 candidates.
Where FSL's randomise -v may differ: the kernel is cut at 3 sigma here; FSL smooths its variance image with a kernel width of its own
choosing; and the normalisation by the smoothed mask is this project's definition.

Cluster mass (randomise(cluster_mass_threshold=h); cluster_mass on maps; MET2_TFCE_MODE_MASS, the header states the definition): where the
extent counts the voxels of a component of {t >= h}, the mass sums the statistic over them, so a compact, strongly altered region outweighs
a wide rim barely above the threshold.  The sum is taken in 64-bit fixed point: a member contributes rint(min(t, 16384) * 2^24), the
integers are added (integer atomics: the order does not matter) and the total is converted once, so the device reproduces an int64 numpy
sum to the bit and differs from the exact sum of the doubles by at most e * 2^-25 plus one rounding for a component of e voxels.  Every
permutation is quantised the same way: the test is a valid permutation test of the quantised statistic.  Grids of more than 2^24 voxels
(after the crop to the tested voxels' bounding box) are refused in this mode.  It works on t, on F and on the pseudo-t, one-sided.  FSL's
randomise -C / -S sums the raw doubles: the values may differ in the last bits, and, as for the extent, a level holds t >= h (not >).

Parity with FSL randomise (-T, -c, -C, -S, -f and -v included) is unpinned: FSL was not available.  Not provided: exchangeability
blocks, several devices, 2-D connectivity."""
import collections
import ctypes as C
import math

import numpy as np

from ._lib import check, lib

PermSet = collections.namedtuple("PermSet", "index sign exhaustive exchange")   # (P_k y)_i = sign[k, i] y[index[k, i]]
EXCHANGES = ("permute", "flip")
TINY = 1e-24                       # a voxel whose s0 <= TINY sum_i Y^2 is explained by the nuisance alone: t = 0, p = 1


def limits():
    """met2_group_limits -> dict(max_n, max_r, max_k, voxel_tile); needs no device"""
    v = [C.c_int32(-1) for _ in range(4)]
    check(lib().met2_group_limits(*[C.byref(x) for x in v]))
    return dict(zip(("max_n", "max_r", "max_k", "voxel_tile"), (x.value for x in v)))


# ---------------------------------------------------------------- the design

def _design(X, c):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    c = np.asarray(c, dtype=np.float64)
    if X.ndim != 2 or c.ndim != 2 or c.shape[0] != X.shape[1]:     # a t-contrast of p entries in any shape; a matrix is [p, s]
        c = c.reshape(-1, 1)
    if X.ndim != 2 or c.shape[0] != X.shape[1] or not (np.isfinite(X).all() and np.isfinite(c).all()):
        raise ValueError("X must be a finite [n, p] design and c a finite t-contrast of p entries or a contrast matrix [p, s]")
    if not c.any():
        raise ValueError("the contrast is zero")
    if c.shape[1] > c.shape[0] or np.linalg.matrix_rank(c) < c.shape[1]:
        raise ValueError("the contrast matrix is rank deficient: its %d columns must be linearly independent (s <= p)" % c.shape[1])
    if X.shape[0] <= X.shape[1] or np.linalg.matrix_rank(X) < X.shape[1]:
        raise ValueError("the design is rank deficient or leaves no degree of freedom: drop the redundant columns")
    return X, c


def partition(X, c):
    """The partition of a design X [n, p] and a t-contrast c [p] (or a contrast matrix C [p, s] of rank s: an F-contrast) into the effect of
    interest x1 [n, s] and the nuisance Z [n, p - s] with x1' Z = 0 (Winkler et al. 2014, appendix; Beckmann's form).  With D = (X'X)^-1 and
    Cu an orthonormal basis of null(c'): x1 = X D c (c'Dc)^-1, Cv = Cu - c (c'Dc)^-1 c' D Cu, Z = X D Cv (Cv'DCv)^-1.  A rank-deficient X
    or C is refused.  A 1-D c and a [p, 1] column give the same bits."""
    X, c = _design(X, c)
    p, s = X.shape[1], c.shape[1]
    D = np.linalg.inv(X.T @ X)
    cdc = np.linalg.inv(c.T @ D @ c)
    x1 = X @ D @ c @ cdc
    if p == s:
        return x1, np.zeros((X.shape[0], 0))
    Cu = np.linalg.svd(c, full_matrices=True)[0][:, s:]            # the left singular vectors beyond the first s span null(c')
    Cv = Cu - c @ cdc @ c.T @ D @ Cu
    Z = X @ D @ Cv @ np.linalg.inv(Cv.T @ D @ Cv)
    return x1, Z


def residualise(Y, X, c):
    """Yr = R_z Y [n, V] with R_z = I - Z Z+ of partition(X, c), and s0 [V] = sum_i Yr^2: a sum of squared residuals, not a difference"""
    Y = np.asarray(Y, dtype=np.float64)
    _, Z = partition(X, c)
    if Y.ndim != 2 or Y.shape[0] != Z.shape[0]:
        raise ValueError("Y must be [n, V] with one row per subject")
    Yr = Y - Z @ (np.linalg.pinv(Z) @ Y) if Z.shape[1] else Y.copy()
    return np.ascontiguousarray(Yr), np.sum(Yr * Yr, axis=0)


# ---------------------------------------------------------------- the permutations

def _labels(x1):
    """equal entries of x1 (to 1e-10 of its largest) get one label; of an x1 with several columns, equal rows"""
    x = np.asarray(x1, dtype=np.float64)
    if x.ndim == 2 and x.shape[1] > 1:
        scale = np.abs(x).max()
        return np.unique(np.round(x / (scale if scale > 0 else 1.0), 10), axis=0, return_inverse=True)[1].ravel()
    x = x.ravel()
    scale = np.abs(x).max()
    return np.unique(np.round(x / (scale if scale > 0 else 1.0), 10), return_inverse=True)[1].ravel()


def _arrangements(counts):
    """every distinct sequence with counts[l] copies of label l, in lexicographic order"""
    n = sum(counts)
    left, seq = list(counts), []

    def walk():
        if len(seq) == n:
            yield tuple(seq)
            return
        for lab in range(len(left)):
            if left[lab]:
                left[lab] -= 1
                seq.append(lab)
                yield from walk()
                seq.pop()
                left[lab] += 1
    return walk()


def _index_for(arrangement, labels):
    """the permutation that carries the labels onto `arrangement`: P' x1 has the label arrangement[m] at m; sources and targets of one label
    are matched in ascending order, so the labels' own arrangement gives the identity"""
    arrangement = np.asarray(arrangement)
    index = np.empty(labels.size, dtype=np.int64)
    for lab in np.unique(labels):
        index[np.flatnonzero(labels == lab)] = np.flatnonzero(arrangement == lab)
    return index


def permutation_set(X, c, n_perm, seed=0, exchange="permute"):
    """At most n_perm signed permutations for the test of c in X -> PermSet(index [P, n], sign [P, n], exhaustive, exchange), with
    (P_k y)_i = sign[k, i] y[index[k, i]].  Row 0 is the identity.  Rows are unique by the x1 they produce (P_k' x1), so swaps within a group
    count once.  The set is exhaustive when the number of distinct arrangements -- n! / prod(group sizes!) for 'permute', 2^n for 'flip' (2^m
    with m the entries of x1 that are not zero) -- is <= n_perm; otherwise it is drawn at random, deterministic in `seed`.
    c may be a contrast matrix [p, s] (an F-contrast): the labels are then those of the rows of x1 [n, s], by the same 1e-10 rule, and m counts
    the subjects whose row of x1 is not zero.  Under 'flip' a sign pattern and its negation give the same F; both are kept, since the rule
    stays "unique by P_k' x1": with the exhaustive set every F then appears twice, the identity's too, and no p-value changes."""
    if exchange not in EXCHANGES:
        raise ValueError("exchange must be one of %s" % (EXCHANGES,))
    if isinstance(n_perm, bool) or int(n_perm) != n_perm or int(n_perm) < 1:
        raise ValueError("n_perm must be a count >= 1")
    n_perm = int(n_perm)
    x1, _ = partition(X, c)
    n = x1.shape[0]
    rng = np.random.default_rng(seed)
    ident = np.arange(n, dtype=np.int64)
    if exchange == "flip":
        free = np.flatnonzero((x1 != 0.0).any(axis=1))
        total = 2 ** free.size
        sign = np.ones((min(total, n_perm), n))
        if total <= n_perm:
            for k in range(total):                                 # row 0: no flip
                sign[k, free] = 1.0 - 2.0 * ((k >> np.arange(free.size)) & 1)
        else:
            seen, k = {(0,) * free.size}, 1
            while k < n_perm:
                bits = rng.integers(0, 2, free.size)
                key = tuple(int(b) for b in bits)
                if key not in seen:
                    seen.add(key)
                    sign[k, free] = 1.0 - 2.0 * bits
                    k += 1
        return PermSet(np.tile(ident, (sign.shape[0], 1)), sign, total <= n_perm, exchange)
    labels = _labels(x1)
    counts = np.bincount(labels).tolist()
    if len(counts) < 2:
        raise ValueError("permuting the subjects cannot change the effect of interest (every entry of x1 is the same, as in a one-sample "
                         "test): use exchange='flip'")
    total = math.factorial(n)
    for m in counts:
        total //= math.factorial(m)
    own = tuple(int(l) for l in labels)
    if total <= n_perm:
        rows = [ident] + [_index_for(a, labels) for a in _arrangements(counts) if a != own]
    else:
        rows, seen = [ident], {own}
        while len(rows) < n_perm:
            index = rng.permutation(n)
            arrangement = np.empty(n, dtype=np.int64)
            arrangement[index] = labels                            # (P' x1)[index[i]] = x1[i]
            key = tuple(int(l) for l in arrangement)
            if key not in seen:
                seen.add(key)
                rows.append(index.astype(np.int64))
    index = np.stack(rows)
    return PermSet(index, np.ones(index.shape), total <= n_perm, exchange)


def _transposed(perms, x):
    """P_k' x for every k: x [n, m] -> [P, m, n]; (P' x)[index[i]] = sign[i] x[i]"""
    P, n = perms.index.shape
    out = np.empty((P, x.shape[1], n))
    rows = np.arange(P)[:, None]
    for j in range(x.shape[1]):
        out[rows, j, perms.index] = perms.sign * x[:, j][None, :]
    return out


def weights(X, c, perms):
    """The weight rows of met2_group_perm_stats for the signed permutations `perms` -> (W [P, r + 1, n], dof) with r = rank(X), dof = n - r:
    row 0 = sqrt(dof) P_k' x1 / sqrt(x1' x1), rows 1 .. r = P_k' q_j, q_j an orthonormal basis of [x1 Z] (see the module's docstring)."""
    x1, Z = partition(X, c)
    n = x1.shape[0]
    M = np.hstack([x1, Z])
    r = M.shape[1]
    dof = n - r
    if perms.index.shape[1] != n:
        raise ValueError("the permutations are not of the design's %d subjects" % n)
    Q = np.linalg.qr(M)[0]
    first = math.sqrt(dof) * x1 / math.sqrt(float(np.sum(x1 * x1)))
    return np.ascontiguousarray(_transposed(perms, np.hstack([first, Q]))), dof


def weights_f(X, C, perms):
    """The weight rows of met2_group_perm_fstats for the contrast matrix C [p, s] and the signed permutations `perms` -> (W [P, r, n], s, dof)
    with r = rank(X), dof = n - r: rows j = 1 .. r are P_k' q_j, q_j the orthonormal basis from np.linalg.qr([x1 Z]), so that q_1 .. q_s span
    x1.  There is no row 0.  The entry's scale is dof / s."""
    x1, Z = partition(X, C)
    n, s = x1.shape
    M = np.hstack([x1, Z])
    if perms.index.shape[1] != n:
        raise ValueError("the permutations are not of the design's %d subjects" % n)
    return np.ascontiguousarray(_transposed(perms, np.linalg.qr(M)[0])), s, n - M.shape[1]


# ---------------------------------------------------------------- the entry on arrays

def _launch(dev, Y, s0, r, W, two_sided, t_ref, t_first, kmax, count):
    """met2_group_perm_stats on tensors that are already on `dev`, contiguous and of the right type (count: int32, the bits of uint32)"""
    import torch
    n, V = Y.shape
    with torch.cuda.device(dev):
        check(lib().met2_group_perm_stats(dev.index or 0, n, V, Y.data_ptr(), s0.data_ptr(), r, W.shape[0], W.data_ptr(), 1 if two_sided else 0,
                                          None if t_ref is None else t_ref.data_ptr(), None if t_first is None else t_first.data_ptr(),
                                          kmax.data_ptr(), None if count is None else count.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))


def _check_batch(Y, s0, W, t_ref, count):
    if len(Y.shape) != 2 or tuple(s0.shape) != (Y.shape[1],):
        raise ValueError("Y must be [n, V] and s0 [V]")
    if len(W.shape) != 3 or W.shape[2] != Y.shape[0] or W.shape[1] < 2 or W.shape[0] < 1:
        raise ValueError("W must be [K, r + 1, n] with K >= 1 and r >= 1")
    if t_ref is not None and tuple(t_ref.shape) != (Y.shape[1],):
        raise ValueError("t_ref must be [V]")
    if count is not None and tuple(count.shape) != (Y.shape[1],):
        raise ValueError("count must be [V]")


def perm_stats(Y, s0, W, two_sided=False, t_ref=None, count=None, want_first=False, device=0):
    """met2_group_perm_stats on numpy arrays: Y [n, V], s0 [V], W [K, r + 1, n], t_ref [V] or None, count [V] uint32 to add to (zeros when None)
    -> (kmax [K], count [V] uint32 or None without t_ref, t_first [V] or None without want_first)"""
    import torch
    dev = torch.device("cuda", device)
    Y, s0, W = (np.ascontiguousarray(a, dtype=np.float64) for a in (Y, s0, W))
    _check_batch(Y, s0, W, t_ref, count)
    put = lambda a: torch.as_tensor(a, device=dev)
    V = Y.shape[1]
    kmax = torch.empty(W.shape[0], dtype=torch.float64, device=dev)
    ref = None if t_ref is None else put(np.ascontiguousarray(t_ref, dtype=np.float64))
    cnt = None
    if ref is not None:
        cnt = put(np.zeros(V, dtype=np.int32) if count is None else np.ascontiguousarray(count, dtype=np.uint32).view(np.int32))
    first = torch.empty(V, dtype=torch.float64, device=dev) if want_first else None
    _launch(dev, put(Y), put(s0), W.shape[1] - 1, put(W), two_sided, ref, first, kmax, cnt)
    return (kmax.cpu().numpy(), None if cnt is None else cnt.cpu().numpy().view(np.uint32), None if first is None else first.cpu().numpy())


def _launch_f(dev, Y, s0, W, s, scale, f_ref, f_first, kmax, count):
    """met2_group_perm_fstats on tensors that are already on `dev`, contiguous and of the right type (count: int32, the bits of uint32)"""
    import torch
    n, V = Y.shape
    with torch.cuda.device(dev):
        check(lib().met2_group_perm_fstats(dev.index or 0, n, V, Y.data_ptr(), s0.data_ptr(), W.shape[1], int(s), float(scale), W.shape[0],
                                           W.data_ptr(), None if f_ref is None else f_ref.data_ptr(),
                                           None if f_first is None else f_first.data_ptr(), kmax.data_ptr(),
                                           None if count is None else count.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))


def _check_fbatch(Y, s0, W, s, ref, count):
    if len(Y.shape) != 2 or tuple(s0.shape) != (Y.shape[1],):
        raise ValueError("Y must be [n, V] and s0 [V]")
    if len(W.shape) != 3 or W.shape[2] != Y.shape[0] or W.shape[1] < 1 or W.shape[0] < 1:
        raise ValueError("W must be [K, r, n] with K >= 1 and r >= 1")
    if isinstance(s, bool) or int(s) != s or not 1 <= int(s) <= W.shape[1]:
        raise ValueError("s must lie in 1 .. r = %d" % W.shape[1])
    if ref is not None and tuple(ref.shape) != (Y.shape[1],):
        raise ValueError("f_ref must be [V]")
    if count is not None and tuple(count.shape) != (Y.shape[1],):
        raise ValueError("count must be [V]")


def perm_fstats(Y, s0, W, s, scale, f_ref=None, count=None, want_first=False, device=0):
    """met2_group_perm_fstats on numpy arrays: Y [n, V], s0 [V], W [K, r, n] (weights_f), s the number of leading rows that span the effect,
    scale = dof / s, f_ref [V] or None, count [V] uint32 to add to (zeros when None)
    -> (kmax [K], count [V] uint32 or None without f_ref, f_first [V] or None without want_first)"""
    import torch
    dev = torch.device("cuda", device)
    Y, s0, W = (np.ascontiguousarray(a, dtype=np.float64) for a in (Y, s0, W))
    _check_fbatch(Y, s0, W, s, f_ref, count)
    put = lambda a: torch.as_tensor(a, device=dev)
    V = Y.shape[1]
    kmax = torch.empty(W.shape[0], dtype=torch.float64, device=dev)
    ref = None if f_ref is None else put(np.ascontiguousarray(f_ref, dtype=np.float64))
    cnt = None
    if ref is not None:
        cnt = put(np.zeros(V, dtype=np.int32) if count is None else np.ascontiguousarray(count, dtype=np.uint32).view(np.int32))
    first = torch.empty(V, dtype=torch.float64, device=dev) if want_first else None
    _launch_f(dev, put(Y), put(s0), put(W), s, scale, ref, first, kmax, cnt)
    return (kmax.cpu().numpy(), None if cnt is None else cnt.cpu().numpy().view(np.uint32), None if first is None else first.cpu().numpy())


# ---------------------------------------------------------------- the spatial statistics on arrays

MODES = {"tfce": 0, "extent": 1, "mass": 3}                        # MET2_TFCE_MODE_* (2 is the pseudo-t's voxel mode, below)
CONNECTIVITIES = (6, 18, 26)
TFCE_DEFAULTS = {"E": 0.5, "H": 2.0, "dh": None, "connectivity": 6}


def tfce_limits():
    """met2_tfce_limits -> dict(max_k, max_steps); needs no device"""
    v = [C.c_int32(-1) for _ in range(2)]
    check(lib().met2_tfce_limits(*[C.byref(x) for x in v]))
    return dict(zip(("max_k", "max_steps"), (x.value for x in v)))


def _dims(grid):
    g = tuple(int(x) for x in grid)
    if len(g) != 3 or min(g) < 1:
        raise ValueError("grid must be (nx, ny, nz) with every axis >= 1")
    return g


def tfce_work_bytes(K, grid, n_vox=0):
    """met2_tfce_work_bytes: the device work space of one call for K maps on `grid` (n_vox > 0: of met2_group_perm_tfce)"""
    out = C.c_int64(-1)
    check(lib().met2_tfce_work_bytes(int(K), (C.c_int32 * 3)(*_dims(grid)), int(n_vox), C.byref(out)))
    return out.value


def _batch_for(grid, n_vox, budget, most):
    """the largest K <= most (and <= max_k) whose work space stays within `budget` bytes"""
    K = max(1, min(int(most), tfce_limits()["max_k"]))
    while K > 1 and tfce_work_bytes(K, grid, n_vox) > budget:
        K -= 1
    if tfce_work_bytes(K, grid, n_vox) > budget:
        raise ValueError("one map on a grid of %s needs %d bytes of work space, more than work_bytes = %d" % (grid, tfce_work_bytes(1, grid, n_vox), budget))
    return K


def spatial(maps, mask=None, mode="tfce", dh=None, E=0.5, H=2.0, connectivity=6, device=0, work_bytes=2 ** 30):
    """met2_tfce on numpy arrays: maps [K, nx, ny, nz] (any K: batches of at most max_k maps, fewer if the work space would pass work_bytes),
    mask [nx, ny, nz] or None, mode 'tfce' | 'extent' | 'mass' (dh is then the threshold) -> (out [K, nx, ny, nz], kmax [K]).  dh is required."""
    import torch
    if mode not in MODES:
        raise ValueError("mode must be one of %s" % (tuple(MODES),))
    maps = np.ascontiguousarray(maps, dtype=np.float64)
    if maps.ndim != 4:
        raise ValueError("maps must be [K, nx, ny, nz]")
    grid = _dims(maps.shape[1:])
    if dh is None:
        raise ValueError("dh is required")
    dev = torch.device("cuda", device)
    m = None
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape != grid:
            raise ValueError("the mask does not lie on the grid of the maps")
        m = torch.as_tensor(mask, device=dev)
    out, kmax = np.empty_like(maps), np.empty(maps.shape[0])
    if not maps.shape[0]:
        return out, kmax
    step = _batch_for(grid, 0, work_bytes, maps.shape[0])
    dims = (C.c_int32 * 3)(*grid)
    with torch.cuda.device(dev):
        for k0 in range(0, maps.shape[0], step):
            src = torch.as_tensor(maps[k0:k0 + step], device=dev)
            dst, km = torch.empty_like(src), torch.empty(src.shape[0], dtype=torch.float64, device=dev)
            check(lib().met2_tfce(device, src.shape[0], dims, src.data_ptr(), None if m is None else m.data_ptr(), MODES[mode], float(dh), float(E),
                                  float(H), int(connectivity), dst.data_ptr(), km.data_ptr(), None, 0, torch.cuda.current_stream(dev).cuda_stream))
            out[k0:k0 + step], kmax[k0:k0 + step] = dst.cpu().numpy(), km.cpu().numpy()
    return out, kmax


def _inside(maps, mask):
    vals = maps if mask is None else maps[..., np.asarray(mask) != 0]
    vals = vals[np.isfinite(vals)]
    return float(vals.max()) if vals.size else 0.0


def tfce(maps, mask=None, dh=None, E=0.5, H=2.0, connectivity=6, device=0):
    """Threshold-free cluster enhancement of one map [nx, ny, nz] or several [K, nx, ny, nz] -> the same shape.  dh None: a hundredth of the
    largest finite value inside the mask over all the maps; when that is <= 0 every value is 0 and nothing is launched.  connectivity
    6 | 18 | 26.  E = 0.5, H = 2 reproduce a float64 numpy loop to the bit; other exponents go through pow."""
    a = np.asarray(maps, dtype=np.float64)
    one = a.ndim == 3
    a = a[None] if one else a
    if a.ndim != 4:
        raise ValueError("maps must be [nx, ny, nz] or [K, nx, ny, nz]")
    if dh is None:
        top = _inside(a, mask)
        if top <= 0.0:
            return np.zeros(a.shape[1:] if one else a.shape)
        dh = top / 100.0
    out = spatial(a, mask, "tfce", dh, E, H, connectivity, device)[0]
    return out[0] if one else out


def cluster_extent(maps, threshold, mask=None, connectivity=26, device=0):
    """The size of every voxel's connected component of {t >= threshold} (0 outside it), for one map [nx, ny, nz] or several [K, nx, ny, nz]"""
    a = np.asarray(maps, dtype=np.float64)
    one = a.ndim == 3
    out = spatial(a[None] if one else a, mask, "extent", threshold, 1.0, 1.0, connectivity, device)[0]
    return out[0] if one else out


def cluster_mass(maps, threshold, mask=None, connectivity=26, device=0):
    """The mass of every voxel's connected component of {t >= threshold}: the sum of t over the component in the header's 64-bit fixed point
    (0 outside it), for one map [nx, ny, nz] or several [K, nx, ny, nz].  At most 2^24 grid voxels."""
    a = np.asarray(maps, dtype=np.float64)
    one = a.ndim == 3
    out = spatial(a[None] if one else a, mask, "mass", threshold, 1.0, 1.0, connectivity, device)[0]
    return out[0] if one else out


def _launch_spatial(dev, Y, s0, r, W, dims, at, mode, dh, E, H, connectivity, ref, first, kmax, count, work):
    """met2_group_perm_tfce on tensors that are already on `dev` (at: int32; count: int32, the bits of uint32; work: a uint8 tensor or None)"""
    import torch
    n, V = Y.shape
    with torch.cuda.device(dev):
        check(lib().met2_group_perm_tfce(dev.index or 0, n, V, Y.data_ptr(), s0.data_ptr(), r, W.shape[0], W.data_ptr(), (C.c_int32 * 3)(*dims),
                                         at.data_ptr(), MODES[mode], float(dh), float(E), float(H), int(connectivity),
                                         None if ref is None else ref.data_ptr(), None if first is None else first.data_ptr(), kmax.data_ptr(),
                                         None if count is None else count.data_ptr(), None if work is None else work.data_ptr(),
                                         0 if work is None else work.numel(), torch.cuda.current_stream(dev).cuda_stream))


def perm_tfce(Y, s0, W, grid, at, mode="tfce", dh=None, E=0.5, H=2.0, connectivity=6, ref=None, count=None, want_first=False, device=0):
    """met2_group_perm_tfce on numpy arrays: perm_stats's Y, s0, W; grid (nx, ny, nz); at [V] the voxels' indices in the grid, strictly
    ascending; ref [V] or None; count [V] uint32 to add to -> (kmax [K], count or None without ref, first [V] or None without want_first)"""
    import torch
    if mode not in MODES:
        raise ValueError("mode must be one of %s" % (tuple(MODES),))
    dev = torch.device("cuda", device)
    Y, s0, W = (np.ascontiguousarray(a, dtype=np.float64) for a in (Y, s0, W))
    _check_batch(Y, s0, W, ref, count)
    put = lambda a: torch.as_tensor(a, device=dev)
    V = Y.shape[1]
    at = np.ascontiguousarray(at, dtype=np.int32)
    if at.shape != (V,):
        raise ValueError("at must be [V]")
    kmax = torch.empty(W.shape[0], dtype=torch.float64, device=dev)
    rf = None if ref is None else put(np.ascontiguousarray(ref, dtype=np.float64))
    cnt = None
    if rf is not None:
        cnt = put(np.zeros(V, dtype=np.int32) if count is None else np.ascontiguousarray(count, dtype=np.uint32).view(np.int32))
    first = torch.empty(V, dtype=torch.float64, device=dev) if want_first else None
    _launch_spatial(dev, put(Y), put(s0), W.shape[1] - 1, put(W), _dims(grid), put(at), mode, dh, E, H, connectivity, rf, first, kmax, cnt, None)
    return (kmax.cpu().numpy(), None if cnt is None else cnt.cpu().numpy().view(np.uint32), None if first is None else first.cpu().numpy())


def _launch_fspatial(dev, Y, s0, W, s, scale, dims, at, mode, dh, E, H, connectivity, ref, first, kmax, count, work):
    """met2_group_perm_ftfce on tensors that are already on `dev` (as _launch_spatial; W [K, r, n])"""
    import torch
    n, V = Y.shape
    with torch.cuda.device(dev):
        check(lib().met2_group_perm_ftfce(dev.index or 0, n, V, Y.data_ptr(), s0.data_ptr(), W.shape[1], int(s), float(scale), W.shape[0],
                                          W.data_ptr(), (C.c_int32 * 3)(*dims), at.data_ptr(), MODES[mode], float(dh), float(E), float(H),
                                          int(connectivity), None if ref is None else ref.data_ptr(), None if first is None else first.data_ptr(),
                                          kmax.data_ptr(), None if count is None else count.data_ptr(), None if work is None else work.data_ptr(),
                                          0 if work is None else work.numel(), torch.cuda.current_stream(dev).cuda_stream))


def perm_ftfce(Y, s0, W, s, scale, grid, at, mode="tfce", dh=None, E=0.5, H=2.0, connectivity=6, ref=None, count=None, want_first=False, device=0):
    """met2_group_perm_ftfce on numpy arrays: perm_fstats's Y, s0, W, s, scale; the rest as perm_tfce
    -> (kmax [K], count or None without ref, first [V] or None without want_first)"""
    import torch
    if mode not in MODES:
        raise ValueError("mode must be one of %s" % (tuple(MODES),))
    dev = torch.device("cuda", device)
    Y, s0, W = (np.ascontiguousarray(a, dtype=np.float64) for a in (Y, s0, W))
    _check_fbatch(Y, s0, W, s, ref, count)
    put = lambda a: torch.as_tensor(a, device=dev)
    V = Y.shape[1]
    at = np.ascontiguousarray(at, dtype=np.int32)
    if at.shape != (V,):
        raise ValueError("at must be [V]")
    kmax = torch.empty(W.shape[0], dtype=torch.float64, device=dev)
    rf = None if ref is None else put(np.ascontiguousarray(ref, dtype=np.float64))
    cnt = None
    if rf is not None:
        cnt = put(np.zeros(V, dtype=np.int32) if count is None else np.ascontiguousarray(count, dtype=np.uint32).view(np.int32))
    first = torch.empty(V, dtype=torch.float64, device=dev) if want_first else None
    _launch_fspatial(dev, put(Y), put(s0), put(W), s, scale, _dims(grid), put(at), mode, dh, E, H, connectivity, rf, first, kmax, cnt, None)
    return (kmax.cpu().numpy(), None if cnt is None else cnt.cpu().numpy().view(np.uint32), None if first is None else first.cpu().numpy())


def _crop(grid, at):
    """the grid cut to the bounding box of the voxels `at` -> (grid, at) there"""
    if not at.size:
        return (1, 1, 1), at.astype(np.int32)
    x, y, z = np.unravel_index(at, grid)
    lo = (x.min(), y.min(), z.min())
    box = (int(x.max() - lo[0] + 1), int(y.max() - lo[1] + 1), int(z.max() - lo[2] + 1))
    return box, np.ravel_multi_index((x - lo[0], y - lo[1], z - lo[2]), box).astype(np.int32)    # the order of the voxels is kept: still ascending


def _spatial_test(Yk, sk, W, r, grid, at, mode, dh, E, H, connectivity, device, batch_spatial, work_bytes, fstat=None):
    """the permutation distribution of one spatial statistic -> (observed [V], count [V] uint32, max_dist [P]); fstat = (s, scale): of F"""
    P, V = W.shape[0], Yk.shape[1]
    if fstat is not None:
        launch = lambda Wk, ref, first, km, cnt, work: _launch_fspatial(dev, Yt, st, Wk, fstat[0], fstat[1], grid, at_t, mode, dh, E, H,
                                                                        connectivity, ref, first, km, cnt, work)
        if batch_spatial is not None:
            f_spatial = batch_spatial
            batch_spatial = lambda Y_, s_, W_, *rest: f_spatial(Y_, s_, W_, fstat[0], fstat[1], *rest)
    else:
        launch = lambda Wk, ref, first, km, cnt, work: _launch_spatial(dev, Yt, st, r, Wk, grid, at_t, mode, dh, E, H, connectivity, ref, first,
                                                                       km, cnt, work)
    if batch_spatial is not None:
        _, _, obs = batch_spatial(Yk, sk, W[:1], grid, at, mode, dh, E, H, connectivity, None, True)
        obs = np.asarray(obs, dtype=np.float64)
        count, max_dist, K = np.zeros(V, dtype=np.uint32), np.empty(P), 32
        for k0 in range(0, P, K):
            km, inc, _ = batch_spatial(Yk, sk, W[k0:k0 + K], grid, at, mode, dh, E, H, connectivity, obs, False)
            max_dist[k0:k0 + K] = km
            count += np.asarray(inc, dtype=np.uint32)
        return obs, count, max_dist
    import torch
    dev = torch.device("cuda", device)
    put = lambda a: torch.as_tensor(a, device=dev)
    K = _batch_for(grid, V, work_bytes, P)
    work = torch.empty(tfce_work_bytes(K, grid, V), dtype=torch.uint8, device=dev)
    Yt, st, Wt, at_t = put(Yk), put(sk), put(W), put(at)
    obs_t = torch.empty(V, dtype=torch.float64, device=dev)
    cnt = torch.zeros(V, dtype=torch.int32, device=dev)
    md = torch.empty(P, dtype=torch.float64, device=dev)
    launch(Wt[:1], None, obs_t, md[:1], None, work)
    for k0 in range(0, P, K):
        launch(Wt[k0:k0 + K], obs_t, None, md[k0:k0 + K], cnt, work)
    return obs_t.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), md.cpu().numpy()


def _spatial_options(tfce, cluster_threshold, cluster_connectivity, two_sided, grid, at, V, batch_stat, batch_spatial, cluster_mass_threshold=None):
    """the checked options of randomise's spatial statistics -> (tfce dict or None, grid, at)"""
    if two_sided:
        raise ValueError("tfce, cluster_threshold and cluster_mass_threshold are one-sided: on |t| a positive and a negative blob would fuse into one cluster; "
                         "test c and -c instead of two_sided=True")
    if grid is None or at is None:
        raise ValueError("tfce, cluster_threshold and cluster_mass_threshold need grid=(nx, ny, nz) and at=[V], the columns' voxel indices in it")
    if batch_stat is not None and batch_spatial is None:
        raise ValueError("batch_stat together with tfce, cluster_threshold or cluster_mass_threshold needs batch_spatial, the numpy callable with met2_group_perm_tfce's meaning")
    if batch_spatial is not None and not callable(batch_spatial):
        raise ValueError("batch_spatial must be a callable with the entry's meaning")
    grid = _dims(grid)
    at = np.asarray(at, dtype=np.int64).ravel()
    if at.size != V or (at.size and (at[0] < 0 or at[-1] >= int(np.prod(grid)))) or (np.diff(at) <= 0).any():
        raise ValueError("at must hold one strictly ascending index into the grid per column of Y")
    if int(np.prod(grid)) >= 2 ** 31:
        raise ValueError("the grid must hold fewer than 2^31 voxels")
    opts = None
    if tfce is not None and tfce is not False:
        opts = dict(TFCE_DEFAULTS)
        if isinstance(tfce, dict):
            unknown = set(tfce) - set(opts)
            if unknown:
                raise ValueError("tfce takes E, H, dh and connectivity, not %s" % sorted(unknown))
            opts.update(tfce)
        elif tfce is not True:
            raise ValueError("tfce must be None, True or a dict of E, H, dh, connectivity")
        if opts["connectivity"] not in CONNECTIVITIES or not (np.isfinite(opts["E"]) and opts["E"] > 0 and np.isfinite(opts["H"]) and opts["H"] >= 0):
            raise ValueError("tfce: connectivity 6 | 18 | 26, E > 0, H >= 0")
        if opts["dh"] is not None and not (np.isfinite(opts["dh"]) and opts["dh"] > 0):
            raise ValueError("tfce: dh must be finite and > 0")
    if cluster_threshold is not None:
        if not (np.isfinite(cluster_threshold) and cluster_threshold > 0) or cluster_connectivity not in CONNECTIVITIES:
            raise ValueError("cluster_threshold must be finite and > 0, cluster_connectivity 6 | 18 | 26")
    if cluster_mass_threshold is not None:
        if not (np.isfinite(cluster_mass_threshold) and cluster_mass_threshold > 0) or cluster_connectivity not in CONNECTIVITIES:
            raise ValueError("cluster_mass_threshold must be finite and > 0, cluster_connectivity 6 | 18 | 26")
    return opts, grid, at


# ---------------------------------------------------------------- variance smoothing: the pseudo-t

VSM_MAX_RADIUS, VSM_MAX_K = 16, 32                                 # MET2_GROUP_VSM_MAX_RADIUS, MET2_GROUP_VSM_MAX_K (vsm_limits reports them)
VSM_MODES = dict(MODES, voxel=2)                                   # MET2_GROUP_VSM_MODE_VOXEL beside MET2_TFCE_MODE_*


def vsm_limits():
    """met2_group_vsm_limits -> dict(max_radius, max_k, tile_axis, tile_lines); needs no device"""
    v = [C.c_int32(-1) for _ in range(4)]
    check(lib().met2_group_vsm_limits(*[C.byref(x) for x in v]))
    return dict(zip(("max_radius", "max_k", "tile_axis", "tile_lines"), (x.value for x in v)))


def vsm_work_bytes(K, grid, n_vox=0, mode="voxel"):
    """met2_group_vsm_work_bytes: the device work space of one call for K maps on `grid` (n_vox = 0: of met2_masked_smooth; n_vox > 0: of
    met2_group_perm_vsm in `mode`, 'voxel' | 'tfce' | 'extent' | 'mass')"""
    if mode not in VSM_MODES:
        raise ValueError("mode must be one of %s" % (tuple(VSM_MODES),))
    out = C.c_int64(-1)
    check(lib().met2_group_vsm_work_bytes(int(K), (C.c_int32 * 3)(*_dims(grid)), int(n_vox), VSM_MODES[mode], C.byref(out)))
    return out.value


def _sigma3(sigma_vox):
    s = np.asarray(sigma_vox, dtype=np.float64).ravel()
    s = np.repeat(s, 3) if s.size == 1 else s
    if s.size != 3 or not np.isfinite(s).all() or (s < 0).any():
        raise ValueError("sigma_vox must be one finite value >= 0, in voxels, or one per axis (sx, sy, sz)")
    return tuple(float(x) for x in s)


def smoothing_taps(sigma_vox):
    """The taps of the variance smoothing for a Gaussian of sigma_vox voxels (a scalar, or one value per axis) -> (radius [3], taps [3]):
    per axis R = ceil(3 sigma) and tap_d = exp(-d^2 / (2 sigma^2)) / sum over d = -R .. R; sigma = 0 gives R = 0 and [1.0], no smoothing
    along that axis.  Formed here, on the host, so that no bit of a result depends on a device exp.  R may not exceed VSM_MAX_RADIUS."""
    radius, taps = [], []
    for s in _sigma3(sigma_vox):
        R = int(math.ceil(3.0 * s))
        if R > VSM_MAX_RADIUS:
            raise ValueError("sigma_vox = %g voxels needs a radius of %d voxels: at most %d, i.e. sigma_vox <= %g" %
                             (s, R, VSM_MAX_RADIUS, VSM_MAX_RADIUS / 3.0))
        d = np.arange(-R, R + 1, dtype=np.float64)
        w = np.exp(-(d * d) / (2.0 * s * s)) if R else np.ones(1)
        radius.append(R)
        taps.append(np.ascontiguousarray(w / w.sum()))
    return tuple(radius), tuple(taps)


def _checked_taps(taps):
    """three tap arrays of odd length -> (radius (3 ints), taps (3 contiguous float64 arrays)); the entry checks the values"""
    taps = tuple(np.ascontiguousarray(t, dtype=np.float64).ravel() for t in taps)
    if len(taps) != 3 or any(t.size % 2 == 0 for t in taps):
        raise ValueError("taps must hold three arrays of 2 R + 1 values, one per axis x, y, z")
    return tuple((t.size - 1) // 2 for t in taps), taps


def _taps_args(radius, taps):
    """the ctypes arguments radius[3], taps_x, taps_y, taps_z (host arrays; the tuple keeps them alive)"""
    dp = C.POINTER(C.c_double)
    return ((C.c_int32 * 3)(*radius),) + tuple(t.ctypes.data_as(dp) for t in taps)


def masked_smooth(maps, mask=None, sigma_vox=None, taps=None, device=0):
    """met2_masked_smooth on numpy arrays: the masked, separable smoothing S of one map [nx, ny, nz] or several [K, nx, ny, nz] (any K: batches
    of at most max_k maps), read as 0 where mask [nx, ny, nz] is 0 (None: no mask), with the taps of smoothing_taps(sigma_vox) or `taps`
    (three arrays) -> (S at every grid voxel, in the shape of maps; N [nx, ny, nz] = S of the mask's indicator).  The variance smoothing
    divides the two: S(m) / N on the mask."""
    import torch
    if (sigma_vox is None) == (taps is None):
        raise ValueError("give exactly one of sigma_vox and taps")
    radius, taps = _checked_taps(smoothing_taps(sigma_vox)[1] if taps is None else taps)
    a = np.ascontiguousarray(maps, dtype=np.float64)
    one = a.ndim == 3
    a = a[None] if one else a
    if a.ndim != 4:
        raise ValueError("maps must be [nx, ny, nz] or [K, nx, ny, nz]")
    grid = _dims(a.shape[1:])
    dev = torch.device("cuda", device)
    m = None
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape != grid:
            raise ValueError("the mask does not lie on the grid of the maps")
        m = torch.as_tensor(mask, device=dev)
    out = np.empty_like(a)
    norm = torch.empty(grid, dtype=torch.float64, device=dev)
    dims, targs = (C.c_int32 * 3)(*grid), _taps_args(radius, taps)
    with torch.cuda.device(dev):
        for k0 in range(0, max(a.shape[0], 1), VSM_MAX_K):
            src = torch.as_tensor(a[k0:k0 + VSM_MAX_K] if a.shape[0] else np.zeros((1,) + grid), device=dev)
            dst = torch.empty_like(src)
            check(lib().met2_masked_smooth(device, src.shape[0], dims, src.data_ptr(), None if m is None else m.data_ptr(), *targs, dst.data_ptr(),
                                           norm.data_ptr() if k0 == 0 else None, None, 0, torch.cuda.current_stream(dev).cuda_stream))
            if a.shape[0]:
                out[k0:k0 + VSM_MAX_K] = dst.cpu().numpy()
    return (out[0] if one else out), norm.cpu().numpy()


def _launch_vsm(dev, Y, s0, r, W, two_sided, dims, at, mode, dh, E, H, connectivity, radius, taps, ref, first, kmax, count, work):
    """met2_group_perm_vsm on tensors that are already on `dev` (as _launch_spatial; radius and taps: the host arrays of _checked_taps)"""
    import torch
    n, V = Y.shape
    with torch.cuda.device(dev):
        check(lib().met2_group_perm_vsm(dev.index or 0, n, V, Y.data_ptr(), s0.data_ptr(), r, W.shape[0], W.data_ptr(), 1 if two_sided else 0,
                                        (C.c_int32 * 3)(*dims), at.data_ptr(), VSM_MODES[mode], float(dh), float(E), float(H), int(connectivity),
                                        *_taps_args(radius, taps), None if ref is None else ref.data_ptr(),
                                        None if first is None else first.data_ptr(), kmax.data_ptr(), None if count is None else count.data_ptr(),
                                        None if work is None else work.data_ptr(), 0 if work is None else work.numel(),
                                        torch.cuda.current_stream(dev).cuda_stream))


def perm_vsm(Y, s0, W, grid, at, taps, mode="voxel", two_sided=False, dh=1.0, E=0.5, H=2.0, connectivity=6, ref=None, count=None, want_first=False,
             device=0):
    """met2_group_perm_vsm on numpy arrays: perm_tfce's Y, s0, W, grid, at; taps: three arrays (smoothing_taps(...)[1]); mode 'voxel' (the
    pseudo-t itself; two_sided allowed; dh, E, H, connectivity not read) | 'tfce' | 'extent' | 'mass' (on the pseudo-t, one-sided)
    -> (kmax [K], count or None without ref, first [V] or None without want_first)"""
    import torch
    if mode not in VSM_MODES:
        raise ValueError("mode must be one of %s" % (tuple(VSM_MODES),))
    radius, taps = _checked_taps(taps)
    dev = torch.device("cuda", device)
    Y, s0, W = (np.ascontiguousarray(a, dtype=np.float64) for a in (Y, s0, W))
    _check_batch(Y, s0, W, ref, count)
    put = lambda a: torch.as_tensor(a, device=dev)
    V = Y.shape[1]
    at = np.ascontiguousarray(at, dtype=np.int32)
    if at.shape != (V,):
        raise ValueError("at must be [V]")
    kmax = torch.empty(W.shape[0], dtype=torch.float64, device=dev)
    rf = None if ref is None else put(np.ascontiguousarray(ref, dtype=np.float64))
    cnt = None
    if rf is not None:
        cnt = put(np.zeros(V, dtype=np.int32) if count is None else np.ascontiguousarray(count, dtype=np.uint32).view(np.int32))
    first = torch.empty(V, dtype=torch.float64, device=dev) if want_first else None
    _launch_vsm(dev, put(Y), put(s0), W.shape[1] - 1, put(W), two_sided, _dims(grid), put(at), mode, dh, E, H, connectivity, radius, taps, rf, first,
                kmax, cnt, None)
    return (kmax.cpu().numpy(), None if cnt is None else cnt.cpu().numpy().view(np.uint32), None if first is None else first.cpu().numpy())


def _vsm_batch_for(grid, n_vox, mode, budget, most):
    """the largest K <= most (and <= max_k) whose work space stays within `budget` bytes"""
    K = max(1, min(int(most), VSM_MAX_K))
    while K > 1 and vsm_work_bytes(K, grid, n_vox, mode) > budget:
        K -= 1
    if vsm_work_bytes(K, grid, n_vox, mode) > budget:
        raise ValueError("one map on a grid of %s needs %d bytes of work space, more than work_bytes = %d" %
                         (grid, vsm_work_bytes(1, grid, n_vox, mode), budget))
    return K


def _vsm_test(Yk, sk, W, r, grid, at, mode, dh, E, H, connectivity, two_sided, radius, taps, device, batch_spatial, work_bytes):
    """the permutation distribution of the pseudo-t (mode 'voxel') or of a spatial statistic of it -> (observed [V], signed in voxel mode;
    ref [V], what the candidates are compared with: |observed| when two_sided; count [V] uint32; max_dist [P])"""
    P, V = W.shape[0], Yk.shape[1]
    if batch_spatial is not None:
        _, _, obs = batch_spatial(Yk, sk, W[:1], grid, at, mode, dh, E, H, connectivity, None, True, False, radius, taps)
        obs = np.asarray(obs, dtype=np.float64)
        ref = np.abs(obs) if two_sided else obs
        count, max_dist, K = np.zeros(V, dtype=np.uint32), np.empty(P), VSM_MAX_K
        for k0 in range(0, P, K):
            km, inc, _ = batch_spatial(Yk, sk, W[k0:k0 + K], grid, at, mode, dh, E, H, connectivity, ref, False, two_sided, radius, taps)
            max_dist[k0:k0 + K] = km
            count += np.asarray(inc, dtype=np.uint32)
        return obs, ref, count, max_dist
    import torch
    dev = torch.device("cuda", device)
    put = lambda a: torch.as_tensor(a, device=dev)
    K = _vsm_batch_for(grid, V, mode, work_bytes, P)
    work = torch.empty(vsm_work_bytes(K, grid, V, mode), dtype=torch.uint8, device=dev)
    Yt, st, Wt, at_t = put(Yk), put(sk), put(W), put(np.ascontiguousarray(at, dtype=np.int32))
    launch = lambda Wk, two, rf, first, km, cnt: _launch_vsm(dev, Yt, st, r, Wk, two, grid, at_t, mode, dh, E, H, connectivity, radius, taps, rf,
                                                             first, km, cnt, work)
    obs_t = torch.empty(V, dtype=torch.float64, device=dev)
    cnt = torch.zeros(V, dtype=torch.int32, device=dev)
    md = torch.empty(P, dtype=torch.float64, device=dev)
    launch(Wt[:1], False, None, obs_t, md[:1], None)
    ref_t = obs_t.abs() if two_sided else obs_t
    for k0 in range(0, P, K):
        launch(Wt[k0:k0 + K], two_sided, ref_t, None, md[k0:k0 + K], cnt)
    return obs_t.cpu().numpy(), ref_t.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), md.cpu().numpy()


def _randomise_vsm(Y, X, c, n_perm, seed, exchange, two_sided, device, batch_stat, tfce, cluster_threshold, cluster_connectivity, grid, at,
                   batch_spatial, work_bytes, variance_smoothing, cluster_mass_threshold=None):
    """randomise with variance_smoothing (its docstring states the results): every statistic is taken on the pseudo-t"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if Y.ndim != 2:
        raise ValueError("Y must be [n, V] with one row per subject")
    sigma = _sigma3(variance_smoothing)
    radius, taps = smoothing_taps(sigma)
    if grid is None or at is None:
        raise ValueError("variance_smoothing needs grid=(nx, ny, nz) and at=[V], the columns' voxel indices in it: the statistic is spatial")
    if batch_stat is not None and batch_spatial is None:
        raise ValueError("batch_stat together with variance_smoothing needs batch_spatial, the numpy callable with met2_group_perm_vsm's meaning")
    if batch_stat is not None and not callable(batch_stat):
        raise ValueError("batch_stat must be a callable with the entry's meaning")
    # two_sided is handed on only with a spatial statistic, which refuses it; the grid and `at` are checked either way
    tfce_opts, grid, at = _spatial_options(tfce, cluster_threshold, cluster_connectivity,
                                           two_sided and ((tfce is not None and tfce is not False) or cluster_threshold is not None
                                                          or cluster_mass_threshold is not None), grid, at,
                                           Y.shape[1], batch_stat, batch_spatial, cluster_mass_threshold)
    x1, _ = partition(X, c)
    perms = permutation_set(X, c, n_perm, seed, exchange)
    W, dof = weights(X, c, perms)
    P, r = W.shape[0], W.shape[1] - 1
    lim = limits() if batch_spatial is None else {"max_n": Y.shape[0], "max_r": r}
    if Y.shape[0] > lim["max_n"] or r > lim["max_r"]:
        raise ValueError("at most %d subjects and %d model columns" % (lim["max_n"], lim["max_r"]))
    Yr, s0 = residualise(Y, X, c)
    keep = np.flatnonzero((Yr != 0.0).any(axis=0) & (s0 > TINY * np.sum(Y * Y, axis=0)))
    Yk, sk = np.ascontiguousarray(Yr[:, keep]), np.ascontiguousarray(s0[keep])
    V, full = keep.size, Y.shape[1]
    # Cropping to the tested voxels' bounding box changes no bit: what is cut away holds zeros, and a sum skips a term or adds an exact zero
    box, at_box = _crop(grid, at[keep])
    test = lambda mode, dh, E, H, conn, two: _vsm_test(Yk, sk, W, r, box, at_box, mode, dh, E, H, conn, two, radius, taps, device, batch_spatial,
                                                      work_bytes)
    if V:
        t_obs, ref, count, max_dist = test("voxel", 1.0, 0.5, 2.0, 6, two_sided)
    else:
        t_obs, ref, count, max_dist = np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint32), np.full(P, -np.inf)
    out = {"tstat": np.zeros(full), "cope": np.zeros(full), "p_uncorrected": np.ones(full), "p_fwe": np.ones(full),
           "count": np.full(full, P, dtype=np.uint32)}
    out["tstat"][keep] = t_obs
    out["cope"][keep] = (x1.T @ Yk).ravel() / float(np.sum(x1 * x1))
    out["count"][keep] = count
    out["p_uncorrected"][keep] = count / float(P)
    out["p_fwe"][keep] = (P - np.searchsorted(np.sort(max_dist), ref, side="left")) / float(P)
    out.update(max_dist=max_dist, n_perm=P, exhaustive=bool(perms.exhaustive), dof=dof,
               t_crit=float(np.quantile(max_dist, 0.95)) if V else float("nan"),
               variance_smoothing={"sigma_vox": sigma, "radius": tuple(int(x) for x in radius)})

    def fill(prefix, stat_key, keys, obs, count_s, md):
        """one statistic's results, unfolded to the V columns: left-out voxels get 0 and p = 1"""
        stat, cnt = np.zeros(full), np.full(full, P, dtype=np.uint32)
        p_unc, p_fwe = np.ones(full), np.ones(full)
        stat[keep], cnt[keep] = obs, count_s
        p_unc[keep] = count_s / float(P)
        p_fwe[keep] = (P - np.searchsorted(np.sort(md), obs, side="left")) / float(P)
        out.update({stat_key: stat, keys[0]: p_unc, keys[1]: p_fwe, prefix + "_count": cnt, prefix + "_max_dist": md,
                    prefix + "_crit": float(np.quantile(md, 0.95))})

    nothing = lambda: (np.zeros(V), np.full(V, P, dtype=np.uint32), np.zeros(P))
    if tfce_opts is not None:
        dh = tfce_opts["dh"]
        if dh is None:
            top = float(np.max(t_obs)) if V else 0.0
            dh = top / 100.0 if top > 0.0 and np.isfinite(top) else None
        if dh is None or not V:                                    # nothing rises above zero: every value 0, every p 1, no launch
            obs, count_s, md = nothing()
        else:
            obs, _, count_s, md = test("tfce", dh, tfce_opts["E"], tfce_opts["H"], tfce_opts["connectivity"], False)
        fill("tfce", "tfce", ("p_tfce_uncorrected", "p_tfce_fwe"), obs, count_s, md)
        out.update(dh=dh if dh is not None else 0.0, tfce_options={"E": float(tfce_opts["E"]), "H": float(tfce_opts["H"]),
                                                                   "connectivity": int(tfce_opts["connectivity"])})
    if cluster_threshold is not None:
        if V:
            obs, _, count_s, md = test("extent", float(cluster_threshold), 1.0, 1.0, cluster_connectivity, False)
        else:
            obs, count_s, md = nothing()
        fill("cluster", "cluster_extent", ("p_cluster_uncorrected", "p_cluster_fwe"), obs, count_s, md)
        out.update(cluster_threshold=float(cluster_threshold), cluster_connectivity=int(cluster_connectivity))
    if cluster_mass_threshold is not None:
        if V:
            obs, _, count_s, md = test("mass", float(cluster_mass_threshold), 1.0, 1.0, cluster_connectivity, False)
        else:
            obs, count_s, md = nothing()
        fill("mass", "cluster_mass", ("p_mass_uncorrected", "p_mass_fwe"), obs, count_s, md)
        out.update(cluster_mass_threshold=float(cluster_mass_threshold), cluster_connectivity=int(cluster_connectivity))
    return out


# ---------------------------------------------------------------- the test

def _randomise_f(Y, X, f_contrast, n_perm, seed, exchange, device, batch_stat, tfce, cluster_threshold, cluster_connectivity, grid, at,
                 batch_spatial, work_bytes, cluster_mass_threshold=None):
    """randomise for an F-contrast (its docstring states the results)"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if Y.ndim != 2:
        raise ValueError("Y must be [n, V] with one row per subject")
    fc = np.asarray(f_contrast, dtype=np.float64)
    fc = fc[None, :] if fc.ndim == 1 else fc
    p = np.shape(X)[1] if np.ndim(X) == 2 else 1
    if fc.ndim != 2 or fc.shape[1] != p:
        raise ValueError("f_contrast must be [s, p]: one t-contrast of the design's %d columns per row" % p)
    Cm = np.ascontiguousarray(fc.T)                                # [p, s]
    want_spatial = (tfce is not None and tfce is not False) or cluster_threshold is not None or cluster_mass_threshold is not None
    if want_spatial:
        tfce_opts, grid, at = _spatial_options(tfce, cluster_threshold, cluster_connectivity, False, grid, at, Y.shape[1], batch_stat, batch_spatial,
                                               cluster_mass_threshold)
    if batch_stat is not None and not callable(batch_stat):
        raise ValueError("batch_stat must be a callable with the entry's meaning")
    perms = permutation_set(X, Cm, n_perm, seed, exchange)
    W, s, dof = weights_f(X, Cm, perms)
    P, r = W.shape[0], W.shape[1]
    scale = float(dof) / float(s)
    lim = limits() if batch_stat is None else {"max_n": Y.shape[0], "max_r": r, "max_k": 256}
    if Y.shape[0] > lim["max_n"] or r > lim["max_r"]:
        raise ValueError("at most %d subjects and %d model columns" % (lim["max_n"], lim["max_r"]))
    Yr, s0 = residualise(Y, X, Cm)
    keep = np.flatnonzero((Yr != 0.0).any(axis=0) & (s0 > TINY * np.sum(Y * Y, axis=0)))
    Yk, sk = np.ascontiguousarray(Yr[:, keep]), np.ascontiguousarray(s0[keep])
    V, K = keep.size, lim["max_k"]
    if batch_stat is not None:
        _, _, f_obs = batch_stat(Yk, sk, W[:1], s, scale, None, True)
        f_obs = np.asarray(f_obs, dtype=np.float64)
        count, max_dist = np.zeros(V, dtype=np.uint32), np.empty(P)
        for k0 in range(0, P, K):
            km, inc, _ = batch_stat(Yk, sk, W[k0:k0 + K], s, scale, f_obs, False)
            max_dist[k0:k0 + K] = km
            count += np.asarray(inc, dtype=np.uint32)
        n_ge = P - np.searchsorted(np.sort(max_dist), f_obs, side="left")
    else:
        import torch
        dev = torch.device("cuda", device)
        put = lambda a: torch.as_tensor(a, device=dev)
        Yt, st, Wt = put(Yk), put(sk), put(W)
        f_dev = torch.empty(V, dtype=torch.float64, device=dev)
        cnt = torch.zeros(V, dtype=torch.int32, device=dev)
        md = torch.empty(P, dtype=torch.float64, device=dev)
        _launch_f(dev, Yt, st, Wt[:1], s, scale, None, f_dev, md[:1], None)
        for k0 in range(0, P, K):
            _launch_f(dev, Yt, st, Wt[k0:k0 + K], s, scale, f_dev, None, md[k0:k0 + K], cnt)
        n_ge_t = P - torch.searchsorted(torch.sort(md)[0], f_dev.contiguous(), right=False)      # exact integers, on the device
        f_obs, count, max_dist, n_ge = f_dev.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), md.cpu().numpy(), n_ge_t.cpu().numpy()
    full = Y.shape[1]
    out = {"fstat": np.zeros(full), "p_uncorrected": np.ones(full), "p_fwe": np.ones(full), "count": np.full(full, P, dtype=np.uint32)}
    out["fstat"][keep] = f_obs
    out["count"][keep] = count
    out["p_uncorrected"][keep] = count / float(P)
    out["p_fwe"][keep] = n_ge / float(P)
    out.update(max_dist=max_dist, n_perm=P, exhaustive=bool(perms.exhaustive), dof=(int(s), int(dof)),
               f_crit=float(np.quantile(max_dist, 0.95)) if V else float("nan"))
    if not want_spatial:
        return out
    box, at_box = _crop(grid, at[keep])

    def fill(prefix, stat_key, keys, obs, count_s, md):
        """one statistic's results, unfolded to the V columns: left-out voxels get 0 and p = 1"""
        stat, cnt = np.zeros(full), np.full(full, P, dtype=np.uint32)
        p_unc, p_fwe = np.ones(full), np.ones(full)
        stat[keep], cnt[keep] = obs, count_s
        p_unc[keep] = count_s / float(P)
        p_fwe[keep] = (P - np.searchsorted(np.sort(md), obs, side="left")) / float(P)
        out.update({stat_key: stat, keys[0]: p_unc, keys[1]: p_fwe, prefix + "_count": cnt, prefix + "_max_dist": md,
                    prefix + "_crit": float(np.quantile(md, 0.95))})

    nothing = lambda: (np.zeros(V), np.full(V, P, dtype=np.uint32), np.zeros(P))
    if tfce_opts is not None:
        dh = tfce_opts["dh"]
        if dh is None:
            top = float(np.max(f_obs)) if V else 0.0
            dh = top / 100.0 if top > 0.0 and np.isfinite(top) else None
        if dh is None or not V:                                    # nothing rises above zero: every value 0, every p 1, no launch
            obs, count_s, md = nothing()
        else:
            obs, count_s, md = _spatial_test(Yk, sk, W, r, box, at_box, "tfce", dh, tfce_opts["E"], tfce_opts["H"], tfce_opts["connectivity"],
                                             device, batch_spatial, work_bytes, fstat=(s, scale))
        fill("tfce", "tfce", ("p_tfce_uncorrected", "p_tfce_fwe"), obs, count_s, md)
        out.update(dh=dh if dh is not None else 0.0, tfce_options={"E": float(tfce_opts["E"]), "H": float(tfce_opts["H"]),
                                                                   "connectivity": int(tfce_opts["connectivity"])})
    if cluster_threshold is not None:
        if V:
            obs, count_s, md = _spatial_test(Yk, sk, W, r, box, at_box, "extent", float(cluster_threshold), 1.0, 1.0, cluster_connectivity, device,
                                             batch_spatial, work_bytes, fstat=(s, scale))
        else:
            obs, count_s, md = nothing()
        fill("cluster", "cluster_extent", ("p_cluster_uncorrected", "p_cluster_fwe"), obs, count_s, md)
        out.update(cluster_threshold=float(cluster_threshold), cluster_connectivity=int(cluster_connectivity))
    if cluster_mass_threshold is not None:
        if V:
            obs, count_s, md = _spatial_test(Yk, sk, W, r, box, at_box, "mass", float(cluster_mass_threshold), 1.0, 1.0, cluster_connectivity, device,
                                             batch_spatial, work_bytes, fstat=(s, scale))
        else:
            obs, count_s, md = nothing()
        fill("mass", "cluster_mass", ("p_mass_uncorrected", "p_mass_fwe"), obs, count_s, md)
        out.update(cluster_mass_threshold=float(cluster_mass_threshold), cluster_connectivity=int(cluster_connectivity))
    return out


def randomise(Y, X, c=None, n_perm=5000, seed=0, exchange="permute", two_sided=False, device=0, batch_stat=None, tfce=None, cluster_threshold=None,
              cluster_connectivity=26, grid=None, at=None, batch_spatial=None, work_bytes=2 ** 30, f_contrast=None, variance_smoothing=None,
              cluster_mass_threshold=None):
    """The permutation test of the t-contrast c in the design X [n, p] at every voxel of Y [n, V] (one row per subject).
    batch_stat: None runs met2_group_perm_stats on `device`; a numpy callable with its meaning -- batch_stat(Y, s0, W, two_sided, t_ref,
    want_first) -> (kmax [K], count increment [V] or None, t_first [V] or None) -- replaces it, and the loop then needs no device.
    -> dict(tstat [V] (signed; two_sided tests |t|), cope [V] (c' beta), p_uncorrected [V] = count / P with count the permutations whose
    statistic at the voxel reaches the observed one, p_fwe [V] = #{k: max_dist[k] >= tstat(v)} / P, count [V], max_dist [P] (the maximum over
    the voxels per permutation), n_perm (the number actually used), exhaustive, dof, t_crit: np.quantile(max_dist, 0.95)).  Both p-values
    count the identity, so neither is below 1 / P.  A voxel whose residualised data are all zero, or whose s0 <= 1e-24 sum_i Y^2 (the
    nuisance explains it), is left out of the launch and gets t = 0, cope = 0, p = 1.
    Spatial statistics, one-sided: tfce = True or dict(E, H, dh, connectivity) (defaults 0.5, 2, a hundredth of the observed maximum of t, 6)
    and / or cluster_threshold = h with cluster_connectivity; both need grid = (nx, ny, nz) and at [V], the strictly ascending index of every
    column of Y in that grid (the grid is cropped to the tested voxels' bounding box before the launches).  batch_spatial: None runs
    met2_group_perm_tfce in batches whose work space stays within work_bytes; a numpy callable with its meaning -- batch_spatial(Y, s0, W, grid,
    at, mode, dh, E, H, connectivity, ref, want_first) -> (kmax [K], count increment [V] or None, first [V] or None), mode 'tfce' | 'extent' | 'mass' --
    replaces it, and is required when batch_stat is given.  Adds for tfce: tfce [V], p_tfce_uncorrected, p_tfce_fwe, tfce_count, tfce_max_dist
    [P], tfce_crit, dh, tfce_options; for the extent: cluster_extent [V], p_cluster_uncorrected, p_cluster_fwe, cluster_count,
    cluster_max_dist [P], cluster_crit -- each defined as its t counterpart.  cluster_mass_threshold = h (with cluster_connectivity, which
    it shares with cluster_threshold; under the rules of cluster_threshold for two_sided, grid, at and batch_spatial, whose stand-ins
    receive mode 'mass' through the same signatures) tests the cluster mass -- the sum of the statistic over a voxel's component of {t >= h}
    in the header's 64-bit fixed point -- on t, on F (f_contrast) or on the pseudo-t (variance_smoothing), and adds cluster_mass [V],
    p_mass_uncorrected, p_mass_fwe, mass_count, mass_max_dist [P], mass_crit and cluster_mass_threshold, each defined as its extent
    counterpart; left-out voxels get mass 0 and p = 1.  When the observed maximum of t is <= 0 (and dh is not given)
    every TFCE value is 0 and every p is 1, with no launch.  With none of the options the results and the launches are what they were.
    F-contrasts: exactly one of c and f_contrast.  f_contrast [s, p] holds one t-contrast per row, as the rows an FSL .fts line selects; the
    test is the F-test of all of them at once (met2_group_perm_fstats; the header states the statistic), one-sided by nature: two_sided=True
    is refused.  -> dict(fstat [V], p_uncorrected, p_fwe, count, max_dist, f_crit, dof = (s, n - r), n_perm, exhaustive); there is no cope.
    tfce (dh defaults to a hundredth of the observed maximum of F) and cluster_threshold (a threshold on F) go through met2_group_perm_ftfce
    and add the keys they add above.  batch_stat(Y, s0, W, s, scale, f_ref, want_first) and batch_spatial(Y, s0, W, s, scale, grid, at,
    mode, dh, E, H, connectivity, ref, want_first) keep their role, with s and scale = dof / s handed on.  Left-out voxels get F = 0, p = 1.
    Variance smoothing: variance_smoothing = sigma_vox or (sx, sy, sz), the Gaussian's sigma in VOXELS (randomise -v takes mm): the statistic
    is the pseudo-t of met2_group_perm_vsm, cope / sqrt(the residual variance pooled over the neighbourhood inside the tested voxels), with
    the taps of smoothing_taps.  It needs grid and at, as TFCE does (the grid is cropped to the tested voxels' bounding box and nothing more,
    which changes no bit: what is cut away holds zeros, and a sum skips a term or adds an exact zero).  tstat is then the pseudo-t, as
    randomise -v's _tstat is, and p_uncorrected, p_fwe, count, max_dist and t_crit are taken on it; cope and dof are unchanged; two_sided is
    allowed; tfce and cluster_threshold are taken on the pseudo-t (dh from its observed maximum; one-sided).  Adds variance_smoothing =
    {"sigma_vox": (sx, sy, sz), "radius": (Rx, Ry, Rz)}.  Batches are sized by vsm_work_bytes within work_bytes.  The stand-in, required when
    batch_stat is given and the only one called: batch_spatial(Y, s0, W, grid, at, mode, dh, E, H, connectivity, ref, want_first, two_sided,
    radius, taps) with mode 'voxel' | 'tfce' | 'extent' | 'mass'.  Together with f_contrast it is refused: FSL smooths the variance for t only, and a
    pseudo-F is not defined here.  Parity with randomise -v is unpinned (the module's docstring says where the definitions may differ)."""
    if (c is None) == (f_contrast is None):
        raise ValueError("give exactly one of c (a t-contrast) and f_contrast (an F-contrast [s, p])")
    if variance_smoothing is not None:
        if f_contrast is not None:
            raise ValueError("variance_smoothing together with f_contrast is refused: FSL randomise smooths the variance for t statistics only, "
                             "and a pseudo-F is not defined here")
        return _randomise_vsm(Y, X, c, n_perm, seed, exchange, two_sided, device, batch_stat, tfce, cluster_threshold, cluster_connectivity, grid,
                              at, batch_spatial, work_bytes, variance_smoothing, cluster_mass_threshold)
    if f_contrast is not None:
        if two_sided:
            raise ValueError("an F-contrast has no sides: two_sided=True is refused")
        return _randomise_f(Y, X, f_contrast, n_perm, seed, exchange, device, batch_stat, tfce, cluster_threshold, cluster_connectivity, grid, at,
                            batch_spatial, work_bytes, cluster_mass_threshold)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if Y.ndim != 2:
        raise ValueError("Y must be [n, V] with one row per subject")
    want_spatial = (tfce is not None and tfce is not False) or cluster_threshold is not None or cluster_mass_threshold is not None
    if want_spatial:
        tfce_opts, grid, at = _spatial_options(tfce, cluster_threshold, cluster_connectivity, two_sided, grid, at, Y.shape[1], batch_stat, batch_spatial,
                                               cluster_mass_threshold)
    if batch_stat is not None and not callable(batch_stat):
        raise ValueError("batch_stat must be a callable with the entry's meaning")
    x1, _ = partition(X, c)
    perms = permutation_set(X, c, n_perm, seed, exchange)
    W, dof = weights(X, c, perms)
    P, r = W.shape[0], W.shape[1] - 1
    lim = limits() if batch_stat is None else {"max_n": Y.shape[0], "max_r": r, "max_k": 256}
    if Y.shape[0] > lim["max_n"] or r > lim["max_r"]:
        raise ValueError("at most %d subjects and %d model columns" % (lim["max_n"], lim["max_r"]))
    Yr, s0 = residualise(Y, X, c)
    keep = np.flatnonzero((Yr != 0.0).any(axis=0) & (s0 > TINY * np.sum(Y * Y, axis=0)))
    Yk, sk = np.ascontiguousarray(Yr[:, keep]), np.ascontiguousarray(s0[keep])
    V, K = keep.size, lim["max_k"]
    if batch_stat is not None:
        _, _, t_obs = batch_stat(Yk, sk, W[:1], False, None, True)
        t_obs = np.asarray(t_obs, dtype=np.float64)
        ref = np.abs(t_obs) if two_sided else t_obs
        count, max_dist = np.zeros(V, dtype=np.uint32), np.empty(P)
        for k0 in range(0, P, K):
            km, inc, _ = batch_stat(Yk, sk, W[k0:k0 + K], two_sided, ref, False)
            max_dist[k0:k0 + K] = km
            count += np.asarray(inc, dtype=np.uint32)
        n_ge = P - np.searchsorted(np.sort(max_dist), ref, side="left")
    else:
        import torch
        dev = torch.device("cuda", device)
        put = lambda a: torch.as_tensor(a, device=dev)
        Yt, st, Wt = put(Yk), put(sk), put(W)
        t_dev = torch.empty(V, dtype=torch.float64, device=dev)
        cnt = torch.zeros(V, dtype=torch.int32, device=dev)
        md = torch.empty(P, dtype=torch.float64, device=dev)
        _launch(dev, Yt, st, r, Wt[:1], False, None, t_dev, md[:1], None)
        ref_t = t_dev.abs() if two_sided else t_dev
        for k0 in range(0, P, K):
            _launch(dev, Yt, st, r, Wt[k0:k0 + K], two_sided, ref_t, None, md[k0:k0 + K], cnt)
        n_ge_t = P - torch.searchsorted(torch.sort(md)[0], ref_t.contiguous(), right=False)      # exact integers, on the device
        t_obs, count, max_dist, n_ge = t_dev.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), md.cpu().numpy(), n_ge_t.cpu().numpy()
    full = Y.shape[1]
    out = {"tstat": np.zeros(full), "cope": np.zeros(full), "p_uncorrected": np.ones(full), "p_fwe": np.ones(full),
           "count": np.full(full, P, dtype=np.uint32)}
    out["tstat"][keep] = t_obs
    out["cope"][keep] = (x1.T @ Yk).ravel() / float(np.sum(x1 * x1))
    out["count"][keep] = count
    out["p_uncorrected"][keep] = count / float(P)
    out["p_fwe"][keep] = n_ge / float(P)
    out.update(max_dist=max_dist, n_perm=P, exhaustive=bool(perms.exhaustive), dof=dof,
               t_crit=float(np.quantile(max_dist, 0.95)) if V else float("nan"))
    if not want_spatial:
        return out
    box, at_box = _crop(grid, at[keep])
    spatial_fn = batch_spatial                                     # None: the device

    def fill(prefix, stat_key, keys, obs, count_s, md):
        """one statistic's results, unfolded to the V columns: left-out voxels get 0 and p = 1"""
        stat, cnt = np.zeros(full), np.full(full, P, dtype=np.uint32)
        p_unc, p_fwe = np.ones(full), np.ones(full)
        stat[keep], cnt[keep] = obs, count_s
        p_unc[keep] = count_s / float(P)
        p_fwe[keep] = (P - np.searchsorted(np.sort(md), obs, side="left")) / float(P)
        out.update({stat_key: stat, keys[0]: p_unc, keys[1]: p_fwe, prefix + "_count": cnt, prefix + "_max_dist": md,
                    prefix + "_crit": float(np.quantile(md, 0.95))})

    if tfce_opts is not None:
        dh = tfce_opts["dh"]
        if dh is None:
            top = float(np.max(t_obs)) if V else 0.0
            dh = top / 100.0 if top > 0.0 and np.isfinite(top) else None
        if dh is None or not V:                                    # nothing rises above zero: every value 0, every p 1, no launch
            obs, count_s, md = np.zeros(V), np.full(V, P, dtype=np.uint32), np.zeros(P)
        else:
            obs, count_s, md = _spatial_test(Yk, sk, W, r, box, at_box, "tfce", dh, tfce_opts["E"], tfce_opts["H"], tfce_opts["connectivity"],
                                             device, spatial_fn, work_bytes)
        fill("tfce", "tfce", ("p_tfce_uncorrected", "p_tfce_fwe"), obs, count_s, md)
        out.update(dh=dh if dh is not None else 0.0, tfce_options={"E": float(tfce_opts["E"]), "H": float(tfce_opts["H"]),
                                                                   "connectivity": int(tfce_opts["connectivity"])})
    if cluster_threshold is not None:
        if V:
            obs, count_s, md = _spatial_test(Yk, sk, W, r, box, at_box, "extent", float(cluster_threshold), 1.0, 1.0, cluster_connectivity, device,
                                             spatial_fn, work_bytes)
        else:
            obs, count_s, md = np.zeros(V), np.full(V, P, dtype=np.uint32), np.zeros(P)
        fill("cluster", "cluster_extent", ("p_cluster_uncorrected", "p_cluster_fwe"), obs, count_s, md)
        out.update(cluster_threshold=float(cluster_threshold), cluster_connectivity=int(cluster_connectivity))
    if cluster_mass_threshold is not None:
        if V:
            obs, count_s, md = _spatial_test(Yk, sk, W, r, box, at_box, "mass", float(cluster_mass_threshold), 1.0, 1.0, cluster_connectivity, device,
                                             spatial_fn, work_bytes)
        else:
            obs, count_s, md = np.zeros(V), np.full(V, P, dtype=np.uint32), np.zeros(P)
        fill("mass", "cluster_mass", ("p_mass_uncorrected", "p_mass_fwe"), obs, count_s, md)
        out.update(cluster_mass_threshold=float(cluster_mass_threshold), cluster_connectivity=int(cluster_connectivity))
    return out
