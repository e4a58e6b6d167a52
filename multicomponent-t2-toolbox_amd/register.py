"""Rigid and affine registration of two volumes: the estimate of the `world` matrix of resample.voxel_matrix (destination-world mm ->
source-world mm) that brings a MOVING volume (the source) onto a FIXED volume (the destination).  The similarity of the two under a batch
of candidate transforms is one launch on the device (met2_register_cost in include/met2_hip.h, which states the three measures and their
sums; csrc/met2_register.hip); the search that proposes the candidates is here, in numpy, and is deterministic: no random restarts.  Mutual
information and its normalised form ('mi', 'nmi') come from a joint histogram of both images (met2_register_joint_cost).

  params_to_world / world_to_params   the parametrisation, FLIRT's ordering: three rotations in degrees about `centre`, three translations in
                                      mm, then 1 (dof 7) or 3 scales, then 3 skews
  prepare, cost                       the stage wrappers of the device cost
  robust_range, scale_intensity, bin_intensity   the intensity rule (below)
  pyramid                             the levels, coarse to fine, on isotropic grids that cover the field of view
  register                            the coarse-to-fine direction-set search

Intensity rule.  Per pyramid level and per image, lo and hi are the 0.02 and 0.98 quantiles (np.quantile, 'linear') of the finite voxels (of the
fixed image: inside the mask); the image becomes clip((v - lo) / (hi - lo), 0, 1), all zeros where hi = lo, non-finite voxels 0.  The fixed
image's bin is min(floor(n_bins s), n_bins - 1) of its scaled value s; a voxel outside the mask, or not finite, gets -1 and takes no part.

Histogram rule ('mi', 'nmi').  The joint histogram is square, B x B, and B is set per pyramid level: B = min(n_bins, max(4, c)) with c the
integer cube root of n_included, the number of that level's fixed voxels that have a bin (level_bins).  A level of a few hundred voxels then
has a handful of samples per cell; with 64 x 64 cells there it has far more cells than samples, every placement scores alike, and the search
runs off (tests/test_register_mi_host.py keeps that case).  The moving image's bin is the library's: floor((y - lo) B / (hi - lo)) of the
interpolated value, clamped to 0 .. B - 1, with (lo, hi) the range of the scaled moving image.

Out of scope: Parzen-window or partial-volume histograms, a histogram that is not square in register, a mask or a weighting of the moving image, motion correction from echo to echo (non-linear warps: warp.py, which starts from this module's matrix).  Parity
with FSL's flirt is unpinned: FSL was not available; the measures are the published ones (Roche et al., MICCAI 1998; Jenkinson & Smith,
Med. Image Anal. 5:143-156, 2001; Jenkinson et al., NeuroImage 17:825-841, 2002)."""
import ctypes as C

import numpy as np

from . import resample
from ._lib import _dp, check, lib

KINDS = {"corratio": 0, "normcorr": 1, "leastsq": 2, "mi": 3, "nmi": 4}      # MET2_REGISTER_CORRATIO, _NORMCORR, _LEASTSQ, _MI, _NMI
JOINT_KINDS = ("mi", "nmi")                                   # scored from a joint histogram, by met2_register_joint_cost
DOFS = (6, 7, 9, 12)
MAX_AXIS, MAX_BINS, MAX_K = 512, 256, 256                     # MET2_REGISTER_MAX_AXIS, _MAX_BINS, _MAX_K
LEASTSQ_WORST = 1.0e300                                       # MET2_REGISTER_LEASTSQ_WORST
ROBUST_Q = (0.02, 0.98)


def worst(kind):
    """the value a candidate without enough overlap, or without variance (mi, nmi: with one occupied row or column), gets"""
    return {2: LEASTSQ_WORST, 3: 0.0, 4: -1.0}.get(_kind(kind), 1.0)


# ---------------------------------------------------------------- the parametrisation (numpy, no device)

def _dof(dof):
    if isinstance(dof, bool) or dof not in DOFS:
        raise ValueError("dof must be 6, 7, 9 or 12")
    return int(dof)


def _kind(kind):
    if kind not in KINDS:
        raise ValueError("cost must be 'corratio', 'normcorr', 'leastsq', 'mi' or 'nmi'")
    return KINDS[kind]


def _centre(centre):
    c = np.zeros(3) if centre is None else np.asarray(centre, dtype=np.float64).reshape(-1)
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError("centre must be three finite coordinates in mm")
    return c


def _full(p, dof):
    """the dof parameters -> all twelve: rotations (deg), translations (mm), three scales, three skews"""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    if p.shape != (_dof(dof),) or not np.isfinite(p).all():
        raise ValueError("a transform of %d degrees of freedom takes %d finite parameters" % (dof, dof))
    full = np.concatenate([np.zeros(6), np.ones(3), np.zeros(3)])
    full[:6] = p[:6]
    if dof == 7:
        full[6:9] = p[6]
    elif dof >= 9:
        full[6:dof] = p[6:dof]
    return full


def _rotation(deg):
    rx, ry, rz = np.deg2rad(deg)
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    return Rz @ Ry @ Rx


def params_to_world(p, dof, centre=None):
    """-> world [4, 4]: x -> centre + t + R K S (x - centre), with R = Rz Ry Rx of the rotations p[0:3] in degrees, t = p[3:6] in mm, S the
    diagonal of the scales (dof 7: p[6] three times; dof >= 9: p[6:9]; else 1) and K = [[1, k0, k1], [0, 1, k2], [0, 0, 1]] of the skews
    p[9:12] (dof 12).  `centre` in mm defaults to the origin; register passes the fixed image's centre of mass."""
    full = _full(p, dof)
    c = _centre(centre)
    K = np.array([[1.0, full[9], full[10]], [0.0, 1.0, full[11]], [0.0, 0.0, 1.0]])
    L = _rotation(full[:3]) @ K @ np.diag(full[6:9])
    w = np.eye(4)
    w[:3, :3] = L
    w[:3, 3] = c + full[3:6] - L @ c
    return w


def world_to_params(world, dof, centre=None):
    """the inverse of params_to_world for a matrix of that family (a determinant > 0, rotations about y inside +-90 degrees); of a matrix with
    more freedom than `dof` the surplus is dropped: scales and skews beyond dof, and at dof 7 the scale is the geometric mean of the three."""
    dof = _dof(dof)
    w = resample._affine44(world, "world")
    c = _centre(centre)
    L = w[:3, :3]
    if np.linalg.det(L) <= 0:
        raise ValueError("world must have a positive determinant (no reflection)")
    Q, U = np.linalg.qr(L)
    sgn = np.sign(np.diag(U))
    Q, U = Q * sgn, U * sgn[:, None]                               # L = Q U with a positive diagonal of U; det Q = +1 follows
    s = np.diag(U).copy()
    Kmat = U / s
    full = np.empty(12)
    full[0] = np.rad2deg(np.arctan2(Q[2, 1], Q[2, 2]))
    full[1] = np.rad2deg(-np.arcsin(np.clip(Q[2, 0], -1.0, 1.0)))
    full[2] = np.rad2deg(np.arctan2(Q[1, 0], Q[0, 0]))
    full[3:6] = w[:3, 3] - c + L @ c
    full[6:9] = s
    full[9:12] = Kmat[0, 1], Kmat[0, 2], Kmat[1, 2]
    return _reduce(full, dof)


def _reduce(full, dof):
    if dof == 7:
        return np.concatenate([full[:6], [np.prod(full[6:9]) ** (1.0 / 3.0)]])
    return full[:dof].copy()


# ---------------------------------------------------------------- intensities

def robust_range(vol, mask=None):
    """(lo, hi): the 0.02 and 0.98 quantiles of the finite voxels (inside the mask); (0, 0) where there is none"""
    v = np.asarray(vol, dtype=np.float64)
    ok = np.isfinite(v) if mask is None else np.isfinite(v) & (np.asarray(mask) != 0)
    if not ok.any():
        return 0.0, 0.0
    lo, hi = np.quantile(v[ok], ROBUST_Q)
    return float(lo), float(hi)


def scale_intensity(vol, mask=None):
    """clip((v - lo) / (hi - lo), 0, 1) with the robust range; zeros where hi = lo; non-finite voxels 0"""
    v = np.asarray(vol, dtype=np.float64)
    lo, hi = robust_range(v, mask)
    if not hi > lo:
        return np.zeros(v.shape)
    return np.clip((np.where(np.isfinite(v), v, lo) - lo) / (hi - lo), 0.0, 1.0)


def bin_intensity(scaled, n_bins, vol=None, mask=None):
    """int32 bins of a volume scaled to [0, 1]: min(floor(n_bins s), n_bins - 1); -1 outside the mask and where `vol` is not finite"""
    n_bins = _n_bins(n_bins)
    b = np.minimum(np.floor(np.asarray(scaled, dtype=np.float64) * n_bins), n_bins - 1).astype(np.int32)
    if mask is not None:
        b[np.asarray(mask) == 0] = -1
    if vol is not None:
        b[~np.isfinite(np.asarray(vol, dtype=np.float64))] = -1
    return b


def _n_bins(n_bins, what="n_bins"):
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or not 1 <= int(n_bins) <= MAX_BINS:
        raise ValueError("%s must lie in 1 .. %d" % (what, MAX_BINS))
    return int(n_bins)


def level_bins(n_bins, n_included):
    """the side B of the square joint histogram of 'mi' and 'nmi' on a level with n_included binned fixed voxels: min(n_bins, max(4, c)), c the
    integer cube root of n_included (the largest c with c^3 <= n_included), so that the mean cell occupancy grows with the level"""
    n = int(n_included)
    c = int(round(max(n, 0) ** (1.0 / 3.0)))
    while c ** 3 > n:
        c -= 1
    while (c + 1) ** 3 <= n:
        c += 1
    return min(_n_bins(n_bins), max(4, c))


def _min_overlap(x):
    x = float(x)
    if not 0.0 <= x <= 1.0:
        raise ValueError("min_overlap must lie in [0, 1]")
    return x


def _volume_dims(shape, what):
    d = tuple(int(n) for n in shape)
    if len(d) != 3 or any(n < 1 for n in d):
        raise ValueError("the %s volume must have three axes of at least one voxel" % what)
    if any(n > MAX_AXIS for n in d):
        raise ValueError("an axis of the %s volume may hold at most %d voxels" % (what, MAX_AXIS))
    return d


def _batch(A):
    a = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1:] != (3, 4) or not 1 <= a.shape[0] <= MAX_K or not np.isfinite(a).all():
        raise ValueError("A_batch must hold 1 .. %d finite 3 x 4 matrices (resample.voxel_matrix makes one)" % MAX_K)
    return a


def limits():
    """dict(run, max_axis, max_bins, max_k, leastsq_worst) of the library (met2_register_limits; no device needed)"""
    v = [C.c_int32(-1) for _ in range(4)]
    w = C.c_double(0.0)
    check(lib().met2_register_limits(*[C.byref(x) for x in v], C.byref(w)))
    return dict(zip(("run", "max_axis", "max_bins", "max_k"), (x.value for x in v)), leastsq_worst=w.value)


def work_bytes(fixed_shape, n_bins, K):
    """(index_bytes, cost_bytes) of met2_register_index and met2_register_cost (met2_register_work_bytes; no device needed)"""
    a, b = C.c_int64(-1), C.c_int64(-1)
    check(lib().met2_register_work_bytes(resample._i3(_volume_dims(fixed_shape, "fixed")), int(n_bins), int(K), C.byref(a), C.byref(b)))
    return a.value, b.value


def joint_work_bytes(fixed_shape, n_bins, moving_bins, K):
    """the bytes of met2_register_joint_cost's work space (met2_register_joint_work_bytes; no device needed)"""
    a = C.c_int64(-1)
    check(lib().met2_register_joint_work_bytes(resample._i3(_volume_dims(fixed_shape, "fixed")), int(n_bins), int(moving_bins), int(K), C.byref(a)))
    return a.value


# ---------------------------------------------------------------- the stage wrappers of the device cost

def prepare(fixed, fixed_bin, moving, kind="corratio", n_bins=64, min_overlap=0.25, device=0, moving_bins=None):
    """Everything of a cost that does not depend on the candidates, once per pair of volumes: the volumes on the device, the fixed voxels
    indexed by bin (met2_register_index), the ranges.  `fixed` and `moving` are used as they are (no scaling), `fixed_bin` int32 with -1 for
    voxels that take no part.  -> f(A_batch [K, 3, 4]) -> (n_inside [K] int64, cost [K]); numpy in, numpy out; device tensors in, tensors out.
    This is also the signature a `cost_fn` of register has.  'mi' and 'nmi' go to met2_register_joint_cost: the moving samples fall into
    `moving_bins` bins (default n_bins) over the moving volume's range, and f(A_batch, want_joint=True) -> (n_inside, cost, joint
    [K, n_bins, moving_bins] int32), the joint histograms the costs were formed from."""
    import torch
    k = _kind(kind)
    n_bins, min_overlap = _n_bins(n_bins), _min_overlap(min_overlap)
    joint_kind = kind in JOINT_KINDS
    moving_bins = n_bins if moving_bins is None else _n_bins(moving_bins, "moving_bins")
    as_numpy = not torch.is_tensor(fixed)
    fdims = _volume_dims(fixed.shape, "fixed")
    mdims = _volume_dims(moving.shape, "moving")
    if tuple(fixed_bin.shape) != fdims:
        raise ValueError("fixed_bin must have the shape of fixed")
    dev = torch.device("cuda", device) if as_numpy or not fixed.is_cuda else fixed.device
    f = torch.as_tensor(fixed, device=dev).to(torch.float64).contiguous()
    m = torch.as_tensor(moving, device=dev).to(torch.float64).contiguous()
    b = torch.as_tensor(fixed_bin, device=dev).to(torch.int32).contiguous()
    if not (bool(torch.isfinite(f).all()) and bool(torch.isfinite(m).all())):
        raise ValueError("fixed and moving must be finite")
    frange = (C.c_double * 2)(float(f.min()), float(f.max()))
    mrange = (C.c_double * 2)(float(m.min()), float(m.max()))
    index_bytes, _ = work_bytes(fdims, n_bins, 1)
    index = torch.empty(index_bytes // 4, dtype=torch.int32, device=dev)
    stream = resample._stream(dev)
    with torch.cuda.device(dev):
        check(lib().met2_register_index(dev.index or 0, resample._i3(fdims), b.data_ptr(), n_bins, index.data_ptr(), index_bytes, stream))
    work, pending = {}, []                                         # pending: (event, transforms) of calls that may still read their host array

    def evaluate(A_batch, want_joint=False):
        a = _batch(A_batch.cpu().numpy() if torch.is_tensor(A_batch) else A_batch)
        K = a.shape[0]
        if want_joint and not joint_kind:
            raise ValueError("only 'mi' and 'nmi' form a joint histogram")
        if K not in work:
            need = joint_work_bytes(fdims, n_bins, moving_bins, K) if joint_kind else work_bytes(fdims, n_bins, K)[1]
            work[K] = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        n_inside = torch.empty(K, dtype=torch.int64, device=dev)
        cost = torch.empty(K, dtype=torch.float64, device=dev)
        joint = torch.empty((K, n_bins, moving_bins), dtype=torch.int32, device=dev) if want_joint else None
        with torch.cuda.device(dev):
            if joint_kind:
                check(lib().met2_register_joint_cost(dev.index or 0, k, resample._i3(fdims), n_bins, index.data_ptr(), resample._i3(mdims), m.data_ptr(), mrange,
                                                     moving_bins, K, a.ctypes.data_as(_dp), min_overlap, work[K].data_ptr(), work[K].numel() * 8,
                                                     n_inside.data_ptr(), cost.data_ptr(), joint.data_ptr() if want_joint else None, resample._stream(dev)))
            else:
                check(lib().met2_register_cost(dev.index or 0, k, resample._i3(fdims), n_bins, index.data_ptr(), f.data_ptr(), frange, resample._i3(mdims),
                                               m.data_ptr(), mrange, K, a.ctypes.data_as(_dp), min_overlap, work[K].data_ptr(), work[K].numel() * 8,
                                               n_inside.data_ptr(), cost.data_ptr(), resample._stream(dev)))
        out = (n_inside, cost, joint) if want_joint else (n_inside, cost)
        if as_numpy:                                               # the copies wait for the stream: `a` has been read by then
            return tuple(x.cpu().numpy() for x in out)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        pending[:] = [(e, x) for e, x in pending if not e.query()] + [(done, a)]    # met2_register_cost: A stays valid until its call has run
        return out

    return evaluate


def cost(fixed, moving, A_batch, kind="corratio", n_bins=64, mask=None, min_overlap=0.25, device=0):
    """The cost of every candidate of A_batch [K, 3, 4] (fixed voxel indices -> continuous moving voxel coordinates) with the intensity rule of
    this module applied to both volumes (n_bins counts for 'corratio', and for 'mi' and 'nmi', which bin both volumes with it; 'normcorr' and
    'leastsq' use one bin).  -> (n_inside [K] int64, cost [K]).  numpy in, numpy out; device tensors in, tensors out."""
    import torch
    tens = torch.is_tensor(fixed)
    fx = fixed.cpu().numpy() if tens else np.asarray(fixed)
    mv = moving.cpu().numpy() if torch.is_tensor(moving) else np.asarray(moving)
    mk = None if mask is None else (mask.cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask))
    if mk is not None and mk.shape != fx.shape:
        raise ValueError("mask must have the shape of fixed")
    fs = scale_intensity(fx, mk)
    nb = _n_bins(n_bins) if kind == "corratio" or kind in JOINT_KINDS else 1
    n, c = prepare(fs, bin_intensity(fs, nb, fx, mk), scale_intensity(mv), kind, nb, min_overlap,
                   fixed.device.index if tens and fixed.is_cuda else device)(A_batch)
    if not tens:
        return n, c
    return torch.as_tensor(n, device=fixed.device), torch.as_tensor(c, device=fixed.device)


# ---------------------------------------------------------------- the pyramid

def _device_filters(device):
    from . import filters

    def smooth(vol, sigma):
        return filters.gaussian_smooth(np.ascontiguousarray(vol)[..., None], sigma, device=device)[..., 0]

    def resample_(vol, A, shape):
        return filters.resample_filter(np.ascontiguousarray(vol), A, shape, order=1, cval=0.0, device=device)

    return smooth, resample_


def voxel_sizes(affine):
    return np.sqrt((resample._affine44(affine, "affine")[:3, :3] ** 2).sum(axis=0))


def pyramid(vol, affine, scales_mm, device=0, filters=None):
    """-> [(volume, affine)] per scale, in the order given: the volume on an isotropic grid of that voxel size which keeps the image's axes and
    its centre and covers its field of view (ceil(n_a p_a / s) voxels along axis a of n_a voxels of p_a mm).  A level coarser than the image's
    smallest voxel p is smoothed first (gaussian_smooth, sigma = sqrt((s / p)^2 - 1) / 2 voxels: half the voxel size of the level in mm, less what
    the image's own voxel already averages) and then resampled by trilinear interpolation (resample_filter; zeros beyond the edge); a level
    that is the image's own grid is the image.  `filters` = (smooth(vol, sigma), resample(vol, A, shape)) replaces the two device filters."""
    v = np.asarray(vol, dtype=np.float64)
    dims = _volume_dims(v.shape, "pyramid")
    aff = resample._affine44(affine, "affine")
    pix = voxel_sizes(aff)
    smooth, resample_ = filters if filters is not None else _device_filters(device)
    levels = []
    for s in scales_mm:
        s = float(s)
        if not (np.isfinite(s) and s > 0):
            raise ValueError("a pyramid scale must be a positive voxel size in mm")
        if np.allclose(pix, s, rtol=1e-6, atol=0.0):
            levels.append((v, aff))
            continue
        shape = tuple(min(max(int(np.ceil(n * p / s - 1e-9)), 1), MAX_AXIS) for n, p in zip(dims, pix))
        step = np.eye(4)                                           # level voxel indices -> image voxel indices: the centres coincide
        step[:3, :3] = np.diag(s / pix)
        step[:3, 3] = (np.array(dims) - 1.0) / 2.0 - (s / pix) * (np.array(shape) - 1.0) / 2.0
        f = s / pix.min()
        src = smooth(v, 0.5 * np.sqrt(f * f - 1.0)) if f > 1.0 + 1e-6 else v
        levels.append((np.asarray(resample_(src, step[:3], shape), dtype=np.float64), aff @ step))
    return levels


# ---------------------------------------------------------------- the search

def centre_of_mass(vol, affine, mask=None):
    """the intensity-weighted mean position in world mm (weights: the volume scaled by the intensity rule); the grid's centre where all weights are 0"""
    w = scale_intensity(vol, mask)
    if mask is not None:
        w = w * (np.asarray(mask) != 0)
    aff = resample._affine44(affine, "affine")
    if w.sum() > 0:
        idx = [(w.sum(axis=tuple(b for b in range(3) if b != a)) * np.arange(w.shape[a])).sum() / w.sum() for a in range(3)]
    else:
        idx = [(n - 1) / 2.0 for n in w.shape]
    return aff[:3, :3] @ np.array(idx) + aff[:3, 3]


def _stages(dof, n_levels):
    """the degrees of freedom searched on every level, as flirt stages them: 6 on the coarsest, 7, 9, 12 (as far as `dof` goes) on the next,
    `dof` from there on; with one level, all of them there"""
    ladder = [d for d in DOFS if d <= dof]
    if n_levels == 1:
        return [ladder]
    return [[6]] + [ladder[1:] or [6]] + [[dof]] * (n_levels - 2)


def _basis(dof):
    """the directions of the twelve-parameter space a search of `dof` degrees of freedom moves along; dof 7 moves the three scales together"""
    B = np.eye(12)[:min(dof, 6)] if dof <= 7 else np.eye(12)[:dof]
    if dof == 7:
        B = np.vstack([B, [0.0] * 6 + [1.0] * 3 + [0.0] * 3])
    return B


def _line_factor(batch):
    return min(0.5, 3.0 / (batch - 1))


def register(fixed, fixed_affine, moving, moving_affine, dof=6, cost="corratio", n_bins=64, scales_mm=None, init="com", search_deg=None,
             mask=None, min_overlap=0.25, xtol=0.02, ftol=1e-7, max_sweeps=6, batch=16, device=0, cost_fn=None, filters=None):
    """Estimate `world` (fixed-world mm -> moving-world mm; resample.voxel_matrix(fixed_affine, moving_affine, world) then resamples `moving`
    onto the grid of `fixed`).  numpy volumes [nx,ny,nz] with their voxel-to-world affines.
    dof 6 (rigid), 7 (+ one scale), 9 (+ three scales) or 12 (+ skews); cost 'corratio' (images of different contrast; flirt's default),
    'normcorr' or 'leastsq' (the same contrast), 'mi' or 'nmi' (mutual information and Studholme's normalised mutual information, negated so
    that smaller is better: only a statistical dependence of the two contrasts is assumed; their joint histogram is square and sized per level,
    B = min(n_bins, max(4, integer cube root of the level's binned fixed voxels)) -- the histogram rule of this module); n_bins of the fixed image for corratio (normcorr and leastsq put every voxel that counts in one bin:
    the member list then runs in voxel order, and the reads of the fixed image are contiguous).  `mask` [nx,ny,nz] selects the fixed voxels that count.
    Levels: scales_mm, coarse to fine (default 4, 2 and 1 times the fixed image's smallest voxel size); both images go on isotropic grids of that
    voxel size (pyramid), are scaled and binned by the intensity rule of this module per level; the mask goes through the same interpolation and
    holds where it gives 0.5 or more.  Fixed voxels that are not finite take no part, moving ones count as 0.
    Degrees of freedom per level as flirt stages them: 6 on the coarsest level, 7 / 9 / 12 up to `dof` on the second, `dof` after that.
    init: 'com' (the translation that brings the centres of mass together), 'identity', or a 4 x 4 world matrix with a positive determinant.
    search_deg: angles in degrees; every triple of them (about x, y, z) is scored on the coarsest level with the centre-of-mass translation
    (whatever `init` is; scales and skews are those of `init`), in batches, and the best seeds the search when it beats `init` (ties: the
    lowest index, `init` first).
    Search: a direction-set (Powell) search over the parameters, in units in which one step moves a point at the edge of the field of view (half
    its diagonal from the centre) by about 1 mm: rotations in units of 1 / radius rad, scales and skews of 1 / radius.  A line search scores
    `batch` points spread evenly over [-span, +span] about the current point in ONE cost call and moves to the best if it is better than the current
    point (ties: the lowest index, the current point first); the span starts at two voxels of the level and shrinks by the fixed factor
    min(1 / 2, 3 / (batch - 1)) until it is below xtol voxels of the level.  A sweep searches every direction, then the sweep's displacement,
    which replaces the direction of the largest decrease; a stage ends after max_sweeps sweeps or when a sweep gains less than ftol.
    cost_fn(fixed, fixed_bin, moving, kind, n_bins, min_overlap) -> f(A_batch) -> (n_inside, cost) replaces the device cost (prepare has this
    signature; for 'mi' and 'nmi' n_bins is the level's B and fixed_bin has B bins), `filters` the device filters of pyramid: the search then needs no device.
    -> dict(world [4, 4], params [dof] (about `centre`), centre [3] = the fixed image's centre of mass, cost, n_inside, dof, levels: one entry
    per (level, stage) in the order they ran, dict(scale_mm, shape, dof: the stage's, cost: at the stage's end, n_eval and n_calls: the
    candidates scored and the cost calls made by that stage alone -- a level's first stage includes the level's first score and the
    search_deg grid --, so their sums over the entries are the totals of the registration))."""
    dof, kind = _dof(dof), cost
    _kind(kind)
    n_bins, min_overlap = _n_bins(n_bins), _min_overlap(min_overlap)
    if isinstance(batch, bool) or not 3 <= int(batch) <= MAX_K:
        raise ValueError("batch must lie in 3 .. %d" % MAX_K)
    batch = int(batch)
    if not (xtol > 0 and ftol >= 0 and int(max_sweeps) >= 1):
        raise ValueError("xtol must be positive, ftol not negative and max_sweeps at least 1")
    fx, mv = np.asarray(fixed, dtype=np.float64), np.asarray(moving, dtype=np.float64)
    _volume_dims(fx.shape, "fixed")
    _volume_dims(mv.shape, "moving")
    fa, ma = resample._affine44(fixed_affine, "fixed_affine"), resample._affine44(moving_affine, "moving_affine")
    mk = None if mask is None else (np.asarray(mask) != 0)
    if mk is not None and mk.shape != fx.shape:
        raise ValueError("mask must have the shape of fixed")
    if not np.isfinite(fx).all():                                  # a fixed voxel that is not finite takes no part; a moving one counts as 0
        mk = np.isfinite(fx) if mk is None else mk & np.isfinite(fx)
        fx = np.where(np.isfinite(fx), fx, 0.0)
    mv = np.where(np.isfinite(mv), mv, 0.0)
    if scales_mm is None:
        scales_mm = [m * voxel_sizes(fa).min() for m in (4.0, 2.0, 1.0)]
    scales_mm = [float(s) for s in scales_mm]
    if not scales_mm:
        raise ValueError("scales_mm must name one level at least")
    centre = centre_of_mass(fx, fa, mk)
    com_shift = centre_of_mass(mv, ma) - centre                    # the translation that brings the centres of mass together
    if isinstance(init, str):
        if init not in ("com", "identity"):
            raise ValueError("init must be 'com', 'identity' or a 4 x 4 world matrix")
        p = np.concatenate([np.zeros(6), np.ones(3), np.zeros(3)])
        if init == "com":
            p[3:6] = com_shift
    else:
        p = world_to_params(init, 12, centre)
    angles = [] if search_deg is None else [float(a) for a in np.asarray(search_deg, dtype=np.float64).reshape(-1)]
    if search_deg is not None and (not angles or not np.isfinite(angles).all()):
        raise ValueError("search_deg must hold finite angles in degrees")
    make = prepare if cost_fn is None else cost_fn
    kw = {"device": device} if cost_fn is None else {}
    filt = filters if filters is not None else (_device_filters(device) if cost_fn is None else None)
    if filt is None:
        raise ValueError("a cost_fn needs `filters` too: the pyramid would run on the device otherwise")
    f_levels = pyramid(fx, fa, scales_mm, filters=filt)
    m_levels = pyramid(mv, ma, scales_mm, filters=filt)
    corners = np.array([[i, j, k] for i in (0, fx.shape[0] - 1) for j in (0, fx.shape[1] - 1) for k in (0, fx.shape[2] - 1)], dtype=np.float64)
    radius = max(np.linalg.norm(corners @ fa[:3, :3].T + fa[:3, 3] - centre, axis=1).max(), voxel_sizes(fa).min())
    unit = np.concatenate([np.full(3, np.rad2deg(1.0 / radius)), np.ones(3), np.full(6, 1.0 / radius)])
    trace, f_best, n_best = [], None, 0
    for li, (scale, stage_dofs) in enumerate(zip(scales_mm, _stages(dof, len(scales_mm)))):
        (fv, faff), (mvol, maff) = f_levels[li], m_levels[li]
        lmask = None
        if mk is not None:
            own_grid = fv.shape == fx.shape and np.array_equal(faff, fa)
            lmask = mk if own_grid else filt[1](mk.astype(np.float64), (resample.invert(fa) @ faff)[:3], fv.shape) >= 0.5
        fs = scale_intensity(fv, lmask)
        nb = n_bins if kind == "corratio" else 1                    # normcorr and leastsq have no use for bins: one bin keeps the voxels in their order
        if kind in JOINT_KINDS:                                     # the histogram rule: the voxels that get a bin do not depend on the number of bins
            nb = level_bins(n_bins, int((bin_intensity(fs, 1, fv, lmask) >= 0).sum()))
        evaluate = make(fs, bin_intensity(fs, nb, fv, lmask), scale_intensity(mvol), kind, nb, min_overlap, **kw)
        count = {"n_eval": 0, "n_calls": 0}

        def score(points):
            A = np.stack([resample.voxel_matrix(faff, maff, params_to_world(q, 12, centre)) for q in points])
            n, c = evaluate(A)
            count["n_eval"] += len(points)
            count["n_calls"] += 1
            return np.asarray(n), np.asarray(c, dtype=np.float64)

        n0, c0 = score([p])                                        # the level's own cost of where the search stands; counted with its first stage
        n_best, f_best = int(n0[0]), float(c0[0])
        if li == 0 and angles:
            grid = [np.concatenate([[rx, ry, rz], com_shift, p[6:]]) for rx in angles for ry in angles for rz in angles]
            for g0 in range(0, len(grid), batch):
                n, c = score(grid[g0:g0 + batch])
                j = int(np.argmin(c))
                if c[j] < f_best:
                    p, f_best, n_best = grid[g0 + j], float(c[j]), int(n[j])
        for sd in stage_dofs:
            dirs = _basis(sd) * unit
            for _ in range(int(max_sweeps)):
                p_start, f_start, drops = p.copy(), f_best, []
                for d in list(dirs) + [None]:
                    if d is None:                                  # the sweep's displacement, in units
                        d = p - p_start
                        norm = np.linalg.norm(d / unit)
                        if norm == 0.0:
                            break
                        d = d / norm
                    f_before, span = f_best, 2.0 * scale
                    while span >= xtol * scale:
                        ts = np.linspace(-span, span, batch)
                        n, c = score([p + t * d for t in ts])
                        j = int(np.argmin(c))
                        if c[j] < f_best:
                            p, f_best, n_best = p + ts[j] * d, float(c[j]), int(n[j])
                        span *= _line_factor(batch)
                    drops.append(f_before - f_best)
                if len(drops) > len(dirs):                         # the displacement was searched: it takes the place of the best direction
                    dirs[int(np.argmax(drops[:len(dirs)]))] = d
                if f_start - f_best < ftol:
                    break
            trace.append({"scale_mm": scale, "shape": tuple(fv.shape), "dof": sd, "cost": f_best, "n_eval": count["n_eval"], "n_calls": count["n_calls"]})
            count["n_eval"] = count["n_calls"] = 0                 # the next stage of this level counts its own
    return {"world": params_to_world(p, 12, centre), "params": _reduce(p, dof), "centre": centre, "cost": f_best, "n_inside": n_best, "dof": dof,
            "levels": trace}
