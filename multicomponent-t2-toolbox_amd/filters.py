"""The whole-volume filters of the drivers, each one call into the C ABI (one translation unit under csrc/ per filter): nesma_filter,
mppca_filter (with mppca_window and mppca_work_bytes), gibbs_filter, brain_mask_filter, bias_field_filter, tissue_segment_filter, partial_volume_filter, label_stats_filter,
resample_filter, resample_labels_filter, register_filter, warp_register_filter, warp_filter, warp_labels_filter, atlas_stats_filter, group_stats_filter, tfce_filter and gaussian_smooth.  All take numpy arrays (and return numpy) or CUDA tensors (and return tensors on the same device); motor.py's drivers
call them and re-export the names."""
import numpy as np
import torch

from ._lib import _dp, check, lib


def _enter(x, device):
    """-> (x as a float64 contiguous tensor on the device, that device, whether the caller gave numpy)"""
    as_numpy = not torch.is_tensor(x)
    dev = torch.device("cuda", device) if as_numpy else x.device
    return torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous(), dev, as_numpy


def _voxel_size(voxel_size):
    vox = np.ascontiguousarray(np.asarray(voxel_size, dtype=np.float64).reshape(-1))
    if vox.shape != (3,):
        raise ValueError("voxel_size must be (dx, dy, dz)")
    return vox


def _mask_u8(mask, dev, chosen):
    """mask -> uint8 on the device, 1 where chosen(mask) holds; None stays None (every voxel)"""
    return None if mask is None else chosen(torch.as_tensor(mask, device=dev)).to(torch.uint8).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(dev, entry, *args):
    """one entry of the library on dev's current stream"""
    with torch.cuda.device(dev):
        check(getattr(lib(), entry)(dev.index or 0, *args, torch.cuda.current_stream(dev).cuda_stream))


def _leave(out, as_numpy):
    """a tensor or a tuple of tensors, as numpy when numpy came in"""
    if not as_numpy:
        return out
    return out.cpu().numpy() if torch.is_tensor(out) else tuple(t.cpu().numpy() for t in out)


def _nonzero(m):
    return m != 0


def nesma_filter(data, mask, device=0):
    """The NESMA filter of the driver (motor:305-333) on the device: `data` [nx,ny,nz,nt] as the driver holds it at
    that point (multiplied by the mask, negatives clipped), `mask` [nx,ny,nz]; voxels with mask == 1 become the
    mean of the similar voxels (relative L1 distance < 2.5 %) of their 12^3 window, all others zero.  Accepts numpy
    arrays (returns numpy) or CUDA tensors (returns a tensor on the same device)."""
    dd, dev, as_numpy = _enter(data, device)
    if dd.dim() != 4 or tuple(np.shape(mask)) != tuple(dd.shape[:3]):
        raise ValueError("data must be [nx,ny,nz,nt] and mask [nx,ny,nz]")
    mk = _mask_u8(mask, dev, lambda m: m == 1)
    out = torch.empty_like(dd)
    _call(dev, "met2_nesma", *dd.shape, dd.data_ptr(), mk.data_ptr(), out.data_ptr())
    return _leave(out, as_numpy)


def mppca_window(window, average=False):
    """an odd int w >= 3 (the cube) or three odd ints >= 1 holding at least 3 voxels -> (wx, wy, wz); ValueError otherwise, and for more
    than 343 voxels wherever met2_mppca_box would run (three ints, or average)"""
    a = np.atleast_1d(np.asarray(window))
    if a.dtype.kind not in "iu" or a.shape not in ((1,), (3,)):
        raise ValueError("the MP-PCA window must be an odd int >= 3 or three odd ints (wx, wy, wz)")
    w = tuple(int(x) for x in a) * (3 if a.size == 1 else 1)
    if any(x < 1 or x % 2 == 0 for x in w) or w[0] * w[1] * w[2] < 3:
        raise ValueError("the MP-PCA window must be an odd int >= 3 or (wx, wy, wz), each odd and >= 1, holding at least 3 voxels")
    if (a.size == 3 or average) and w[0] * w[1] * w[2] > 343:
        raise ValueError("an MP-PCA window (wx, wy, wz), and any window with averaging, must hold at most 343 voxels")
    return w


def mppca_work_bytes(shape, window, average=True):
    """(min_bytes, default_bytes) of mppca_filter's work space for data of `shape` [nx,ny,nz,nt] (met2_mppca_box_work_bytes; no device
    needed): max_work_bytes may lie anywhere from min_bytes up; both are 0 without averaging."""
    import ctypes as C
    nx, ny, nz, nt = (int(x) for x in shape)
    lo, dflt = C.c_int64(0), C.c_int64(0)
    check(lib().met2_mppca_box_work_bytes(nx, ny, nz, nt, (C.c_int32 * 3)(*mppca_window(window, True)), int(bool(average)), C.byref(lo), C.byref(dflt)))
    return lo.value, dflt.value


def mppca_filter(data, mask, window=5, average=False, device=0, return_maps=False, max_work_bytes=0):
    """Marchenko-Pastur PCA denoising (Veraart et al., NeuroImage 2016; met2_mppca in include/met2_hip.h states the algorithm) on the
    device: `data` [nx,ny,nz,nt], 2 <= nt <= 63, `mask` [nx,ny,nz]; every voxel with mask != 0 is projected on the signal subspace of
    the decay curves of its window^3 patch (masked voxels only), all others become zero.  The output is not clipped.
    window=(wx, wy, wz) (met2_mppca_box): a box patch, each side odd, for anisotropic voxels -- (5, 5, 1) keeps to the slice of a 2-D
    multi-slice acquisition.  average=True (met2_mppca_box, average = 1): every voxel becomes the weighted mean of the estimates of all the
    patches that hold it, weights 1 / (1 + rank) (Manjon et al., PLoS ONE 2013); sigma is the same mean of the patches' noise levels.  The
    patches' bases are held in a work space of at most max_work_bytes (0: the library's default, at most 1 GiB; mppca_work_bytes gives the
    minimum), the volume going through in as many pieces as that takes; the result does not depend on it.  The call then waits for the device.
    An int window without average is the call of met2_mppca it always was.  Pinned against its numpy restatement only (tests/tools).
    return_maps=True: (denoised, sigma [nx,ny,nz] the noise level, rank [nx,ny,nz] int32 the components kept by the voxel's own patch; -1
    where the patch holds a non-finite value and -2 where the eigen-solver gave up, both copied through -- with average=True only where no
    patch that holds the voxel has a say).  numpy in -> numpy out, CUDA tensor in -> tensors out."""
    import ctypes as C
    dd, dev, as_numpy = _enter(data, device)
    if dd.dim() != 4 or tuple(np.shape(mask)) != tuple(dd.shape[:3]):
        raise ValueError("data must be [nx,ny,nz,nt] and mask [nx,ny,nz]")
    mk = _mask_u8(mask, dev, _nonzero)
    out = torch.empty_like(dd)
    sigma = torch.empty(dd.shape[:3], dtype=torch.float64, device=dev) if return_maps else None
    rank = torch.empty(dd.shape[:3], dtype=torch.int32, device=dev) if return_maps else None
    if np.ndim(window) == 0 and not average:                       # the call of before, refusals included: a bad int window is the library's Met2Error
        _call(dev, "met2_mppca", *dd.shape, dd.data_ptr(), mk.data_ptr(), int(window), out.data_ptr(), _ptr(sigma), _ptr(rank))
    else:
        _call(dev, "met2_mppca_box", *dd.shape, dd.data_ptr(), mk.data_ptr(), (C.c_int32 * 3)(*mppca_window(window, True)), int(bool(average)),
              int(max_work_bytes), out.data_ptr(), _ptr(sigma), _ptr(rank), None, None)
    return _leave((out, sigma, rank) if return_maps else out, as_numpy)


def gibbs_filter(data, nshifts=20, minW=1, maxW=3, device=0, return_shifts=False, mode="2d"):
    """Removal of Gibbs (truncation) ringing by local sub-voxel shifts (Kellner et al., MRM 2016; met2_degibbs in include/met2_hip.h states
    the algorithm) on the device: every (z, echo) slice of `data` [nx,ny,nz,nt] is unrung along x and y, 8 <= nx, ny <= 256.  The defaults
    are those of MRtrix's mrdegibbs, which the reference's example script runs at this place; parity with mrdegibbs itself is unpinned.  A
    slice that holds a non-finite value is copied through.  The output is not clipped: it can undershoot zero next to an edge.
    mode='3d' (met2_degibbs3d; Bautista et al., ISMRM 2021), for 3-D Fourier-encoded acquisitions: every echo volume is unrung along x, y
    and z, 8 <= nx, ny, nz <= 256; an echo volume that holds a non-finite value is copied through.
    return_shifts=True: (unrung, shift_x, shift_y), the int8 shifts (in units of 1 / (2 nshifts) voxel) chosen per sample along each axis;
    with mode='3d' (unrung, shift_x, shift_y, shift_z).  numpy in -> numpy out, CUDA tensor in -> tensors out."""
    if mode not in ("2d", "3d"):
        raise ValueError("mode must be '2d' or '3d'")
    dd, dev, as_numpy = _enter(data, device)
    if dd.dim() != 4:
        raise ValueError("data must be [nx,ny,nz,nt]")
    out = torch.empty_like(dd)
    shifts = tuple(torch.empty(dd.shape, dtype=torch.int8, device=dev) if return_shifts else None for _ in range(3 if mode == "3d" else 2))
    _call(dev, "met2_degibbs3d" if mode == "3d" else "met2_degibbs", *dd.shape, dd.data_ptr(), int(nshifts), int(minW), int(maxW),
          out.data_ptr(), *map(_ptr, shifts))
    return _leave((out,) + shifts if return_shifts else out, as_numpy)

def brain_mask_filter(data, voxel_size, f=0.4, level=4, n_iter=1000, device=0, return_surface=False):
    """Brain extraction (met2_brain_mask in include/met2_hip.h states the algorithm: the surface model of Smith, HBM 2002, which FSL's bet
    runs, without bet's self-intersection retry pass and its -R / -S / -B variants) on the device: `data` [nx,ny,nz], or [nx,ny,nz,nt], which
    is averaged over the echoes first; `voxel_size` (dx, dy, dz) in mm.  The defaults are those of the reference's example script
    (bet -m -f 0.4; level 4 is bet's mesh of 2562 vertices); parity with bet itself is unpinned.  -> uint8 mask [nx,ny,nz], 1 inside the
    surface.  return_surface=True: (mask, vertices [nv, 3] in mm, triangles [nt, 3] int32, statistics: a dict of t2, t, t98, tm, cx, cy, cz,
    r).  numpy in -> numpy out, CUDA tensor in -> tensors out (the triangles and the statistics are host objects either way)."""
    from . import bet
    as_numpy = not torch.is_tensor(data)
    if (np.ndim(data) if as_numpy else data.dim()) not in (3, 4):
        raise ValueError("data must be [nx,ny,nz] or [nx,ny,nz,nt]")
    vox = _voxel_size(voxel_size)
    dd, dev, _ = _enter(data, device)
    if dd.dim() == 4:
        dd = bet.bet_mean(dd)
    mask = torch.empty(dd.shape, dtype=torch.uint8, device=dev)
    n = 4 ** min(max(int(level), 0), 4)
    verts = torch.empty((10 * n + 2, 3), dtype=torch.float64, device=dev) if return_surface else None
    st = np.zeros(8, dtype=np.float64)
    _call(dev, "met2_brain_mask", *dd.shape, dd.data_ptr(), vox.ctypes.data_as(_dp), float(f), int(level), int(n_iter), mask.data_ptr(),
          _ptr(verts), st.ctypes.data_as(_dp))
    if not return_surface:
        return _leave(mask, as_numpy)
    stats = {k: float(x) for k, x in zip(bet.STAT_KEYS, st)}
    return _leave((mask, verts), as_numpy) + (bet.bet_mesh(level)[1], stats)

def bias_field_filter(vol, mask=None, voxel_size=(1, 1, 1), n_class=3, n_outer=4, n_em=10, fwhm=20.0, device=0, return_field=False):
    """Bias-field correction of a 3-D map (met2_bias_field in include/met2_hip.h states the algorithm: the EM estimator of Wells et al. 1996
    and Guillemaud & Brady 1997, which FSL's fast iterates, without fast's Markov random field term) on the device: `vol` [nx,ny,nz], `mask`
    [nx,ny,nz] or None (every voxel), `voxel_size` (dx, dy, dz) in mm.  The defaults are those of the reference's example script
    (fast -n 3 -I 4 -l 20.0); parity with fast itself is unpinned.  The field is estimated on the masked voxels that are finite and positive
    and divided out wherever it is defined; non-finite voxels are copied through.
    return_field=True: (corrected, field, classes [3 n_class] = the final class means and variances of log(vol) and the class weights).
    numpy in -> numpy out, CUDA tensor in -> tensors out."""
    dd, dev, as_numpy = _enter(vol, device)
    if dd.dim() != 3 or (mask is not None and tuple(np.shape(mask)) != tuple(dd.shape)):
        raise ValueError("vol must be [nx,ny,nz] and mask the same shape")
    vox = _voxel_size(voxel_size)
    mk = _mask_u8(mask, dev, _nonzero)
    out = torch.empty_like(dd)
    field = torch.empty_like(dd) if return_field else None
    classes = torch.empty(3 * max(int(n_class), 0), dtype=torch.float64, device=dev) if return_field else None
    _call(dev, "met2_bias_field", *dd.shape, dd.data_ptr(), _ptr(mk), vox.ctypes.data_as(_dp), int(n_class), int(n_outer), int(n_em),
          float(fwhm), out.data_ptr(), _ptr(field), _ptr(classes))
    return _leave((out, field, classes) if return_field else out, as_numpy)

def tissue_segment_filter(vol, mask=None, voxel_size=(1, 1, 1), n_class=3, beta=0.1, n_outer=4, n_em=10, n_icm=8, device=0, return_prob=True):
    """Tissue segmentation of a 3-D map (met2_tissue_segment in include/met2_hip.h states the algorithm: the hidden-Markov-random-field EM of
    Zhang, Brady & Smith 2001, the model of FSL's fast: Gaussian classes in log intensity, a Potts prior of strength `beta` over the six face
    neighbours weighted by the voxel size, labels by iterated conditional modes) on the device: `vol` [nx,ny,nz] (the drivers pass the
    bias-corrected water-content map), `mask` [nx,ny,nz] or None (every voxel), `voxel_size` (dx, dy, dz) in mm.  The defaults are those of the
    reference's example script (fast -n 3 -H 0.1); parity with fast itself is unpinned.  The outputs are hard labels and class posteriors
    (fast's _seg and _prob_k); its _pve_k maps are partial_volume_filter's.  Voxels outside the mask, non-finite or not positive are left out.
    -> seg [nx,ny,nz] uint8: 0 where left out, otherwise 1..n_class by ascending class mean (1 the driest tissue of a water-content map);
    return_prob=True: (seg, prob [n_class,nx,ny,nz]: the class posteriors in that order, 0 where left out, classes [3 n_class]: the class
    means and variances of log(vol) and the class weights, in that order too).
    numpy in -> numpy out, CUDA tensor in -> tensors out."""
    dd, dev, as_numpy = _enter(vol, device)
    if dd.dim() != 3 or (mask is not None and tuple(np.shape(mask)) != tuple(dd.shape)):
        raise ValueError("vol must be [nx,ny,nz] and mask the same shape")
    vox = _voxel_size(voxel_size)
    mk = _mask_u8(mask, dev, _nonzero)
    K = max(int(n_class), 0)
    seg = torch.zeros(tuple(dd.shape), dtype=torch.uint8, device=dev)
    prob = torch.zeros((K,) + tuple(dd.shape), dtype=torch.float64, device=dev) if return_prob else None
    classes = torch.zeros(3 * K, dtype=torch.float64, device=dev) if return_prob else None
    _call(dev, "met2_tissue_segment", *dd.shape, dd.data_ptr(), _ptr(mk), vox.ctypes.data_as(_dp), int(n_class), float(beta), int(n_outer),
          int(n_em), int(n_icm), seg.data_ptr(), _ptr(prob), _ptr(classes))
    return _leave((seg, prob, classes) if return_prob else seg, as_numpy)


def partial_volume_filter(vol, mask=None, voxel_size=(1, 1, 1), n_class=3, beta=0.1, beta_pv=0.3, n_outer=4, n_em=10, n_icm=8, device=0,
                          seg=None, prob=None):
    """Partial-volume tissue maps of a 3-D map (met2_partial_volume in include/met2_hip.h states the algorithm: the mixel model of Santago &
    Gage 1993 as Shattuck et al. 2001 and Tohka et al. 2004 use it -- every voxel pure tissue or a mixture of two rank-adjacent tissues, a
    Potts-like prior of strength `beta_pv` over the six face neighbours, types by iterated conditional modes, the fraction of a mixed voxel
    in Tohka's closed form) on the device, after the tissue segmentation: `seg` [nx,ny,nz] and `prob` [n_class,nx,ny,nz] as
    tissue_segment_filter returns them, or None, and tissue_segment_filter runs first with `mask`, `beta`, `n_outer`, `n_em`, `n_icm`.  The
    defaults are those of the reference's example script (fast -n 3 -H 0.1, and fast's own -R 0.3); parity with fast itself is unpinned.
    -> (pve [n_class,nx,ny,nz]: the tissue fractions, summing to 1 on the segmented voxels and 0 elsewhere; pveseg [nx,ny,nz] uint8: 1 + the
    class of the largest fraction, 0 elsewhere; mixeltype uint8: 0..n_class-1 pure, n_class + j a mixture of classes j and j + 1, 255
    elsewhere; classes_lin [3 n_class]: the class means and variances of vol itself (not its log) and the class weights).
    numpy in -> numpy out, CUDA tensor in -> tensors out."""
    if (seg is None) != (prob is None):
        raise ValueError("seg and prob go together")
    vox = _voxel_size(voxel_size)
    dd, dev, as_numpy = _enter(vol, device)
    if dd.dim() != 3 or (mask is not None and tuple(np.shape(mask)) != tuple(dd.shape)):
        raise ValueError("vol must be [nx,ny,nz] and mask the same shape")
    K = max(int(n_class), 0)
    if seg is None:
        seg, prob, _ = tissue_segment_filter(dd, mask, vox, n_class, beta, n_outer, n_em, n_icm)
    sg = torch.as_tensor(seg, device=dev).to(torch.uint8).contiguous()
    pr = torch.as_tensor(prob, dtype=torch.float64, device=dev).contiguous()
    if tuple(sg.shape) != tuple(dd.shape) or tuple(pr.shape) != (K,) + tuple(dd.shape):
        raise ValueError("seg must have the shape of vol and prob must be [n_class] + that shape")
    pve = torch.zeros((K,) + tuple(dd.shape), dtype=torch.float64, device=dev)
    pveseg = torch.zeros(tuple(dd.shape), dtype=torch.uint8, device=dev)
    mixel = torch.full(tuple(dd.shape), 255, dtype=torch.uint8, device=dev)
    classes = torch.zeros(3 * K, dtype=torch.float64, device=dev)
    _call(dev, "met2_partial_volume", *dd.shape, dd.data_ptr(), sg.data_ptr(), pr.data_ptr(), vox.ctypes.data_as(_dp), int(n_class),
          float(beta_pv), int(n_icm), pve.data_ptr(), pveseg.data_ptr(), mixel.data_ptr(), classes.data_ptr())
    return _leave((pve, pveseg, mixel, classes), as_numpy)

STAT_QUANTITIES = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "reg_param")
STAT_KEYS = ("n", "mean", "std", "quantiles", "spectrum_mean", "spectrum_quantiles")


def label_stats_filter(res, labels, q=None, device=0):
    """Per-label statistics of a result dict of recon_met2_arrays (met2_label_stats in include/met2_hip.h states the definitions; stats.py
    holds the stages) on the device: `labels` is an integer volume shaped like the maps -- every distinct value > 0 is a label, mapped to
    dense indices the way recon_met2_rois does, so a tissue segmentation and an atlas ROI image are served alike; `q` the probabilities
    (stats.DEFAULT_Q).  Per label the sample of a quantity is its voxels that are not NaN.
    -> dict(labels [L], quantities = STAT_QUANTITIES, q, n, mean, std [L, 8], quantiles [L, 8, n_q] (np.quantile's 'linear', to the bit),
    spectrum_mean [L, n_t2]: the per-bin mean of fsol_4D over the label, normalised to sum 1 -- the reference's mean_T2_dist (motor:377) per
    label, its TO DO (2) of motor:376 --, spectrum_quantiles [L, n_t2, n_q]: the per-bin quantiles scaled by the same factor, the spatial
    band around it, T2s)."""
    from . import stats
    q = stats.DEFAULT_Q if q is None else tuple(float(x) for x in np.asarray(q, dtype=np.float64).reshape(-1))
    lab_in = labels if torch.is_tensor(labels) else np.asarray(labels)
    if (lab_in.dtype.is_floating_point if torch.is_tensor(lab_in) else lab_in.dtype.kind not in "iu"):
        raise ValueError("labels must be an integer volume")
    vol_shape = tuple(np.shape(res["MWF"]))
    if tuple(lab_in.shape) != vol_shape:
        raise ValueError("labels must have the shape of the maps")
    dev = torch.device("cuda", device)
    lab = torch.as_tensor(lab_in if torch.is_tensor(lab_in) else np.ascontiguousarray(lab_in).astype(np.int64), device=dev).to(torch.int64).reshape(-1)
    ids = torch.unique(lab)
    ids = ids[ids > 0]
    L = int(ids.numel())
    if L == 0:
        raise ValueError("no label > 0")
    pos = torch.searchsorted(ids, lab).clamp(max=L - 1)
    dense = torch.where(ids[pos] == lab, pos, torch.full_like(pos, -1)).to(torch.int32)
    maps = torch.stack([torch.as_tensor(np.ascontiguousarray(res[name], dtype=np.float64), device=dev).reshape(-1) for name in STAT_QUANTITIES])
    fsol = torch.as_tensor(np.ascontiguousarray(res["fsol_4D"], dtype=np.float64), device=dev)
    n_t2 = int(fsol.shape[-1])
    st = stats.label_stats(maps, dense, L, q, "series")
    sp = stats.label_stats(fsol.reshape(-1, n_t2), dense, L, q, "voxel")
    with np.errstate(invalid="ignore", divide="ignore"):
        tot = sp[:, :, 1].sum(axis=1)
        return {"labels": ids.cpu().numpy(), "quantities": STAT_QUANTITIES, "q": np.asarray(q), "n": st[:, :, 0], "mean": st[:, :, 1],
                "std": st[:, :, 2], "quantiles": st[:, :, 3:], "spectrum_mean": sp[:, :, 1] / tot[:, None],
                "spectrum_quantiles": sp[:, :, 3:] / tot[:, None, None], "T2s": np.asarray(res["T2s"])}

def resample_filter(vol, A, shape, order=1, cval=0.0, device=0, return_inside=False, max_work_bytes=0, series_axis=-1):
    """Affine resampling of a volume onto another grid (met2_resample in include/met2_hip.h states the algorithm:
    scipy.ndimage.affine_transform(vol, A[:, :3], offset=A[:, 3], output_shape=shape, order=order, mode='constant', cval=cval), restated) on the
    device: `vol` [nx,ny,nz], or 4-D -- [nx,ny,nz,S] as the drivers hold echo data and spectra (series_axis=-1), or [S,nx,ny,nz] as they hold
    stacked maps (series_axis=0) --, every series through the same transform and read in place; `A` [3, 4] takes a voxel index of the grid
    `shape` = (mx, my, mz) to continuous voxel coordinates of `vol` (resample.voxel_matrix makes it from two NIfTI affines).  order 0 is
    nearest neighbour, 1 trilinear, 3 the cubic B-spline; voxels that fall outside `vol` get `cval`.  Nothing is smoothed: a map that goes onto
    a coarser grid should pass gaussian_smooth first.  max_work_bytes bounds the work space of order 3 (resample.work_bytes gives the minimum;
    0: the library's default); the result does not depend on it.
    -> the resampled array in the layout of `vol`; return_inside=True: (array, inside [mx,my,mz] uint8, 1 where the voxel was interpolated).
    numpy in -> numpy out, CUDA tensor in -> tensors out."""
    from . import resample
    if series_axis not in (-1, 0, 3):
        raise ValueError("series_axis must be -1 ([nx,ny,nz,S]) or 0 ([S,nx,ny,nz])")
    return resample.resample(vol, A, shape, order=order, cval=cval, layout="series" if series_axis == 0 else "voxel", device=device,
                             return_inside=return_inside, max_work_bytes=max_work_bytes)


def resample_labels_filter(labels, A, shape, fill=0, device=0):
    """An integer label volume (an atlas ROI image, a parcellation) onto the grid `shape` through `A` (see resample_filter), nearest neighbour
    (met2_resample_labels); `fill` where a voxel falls outside the label image.  -> int32 [mx,my,mz].  numpy in -> numpy out, CUDA tensor in
    -> tensor out."""
    from . import resample
    return resample.resample_labels(labels, A, shape, fill=fill, device=device)


def register_filter(fixed, fixed_affine, moving, moving_affine, **options):
    """Rigid or affine registration of `moving` onto `fixed` (register.register states the search, met2_register_cost in include/met2_hip.h
    the similarity measures, which run on the device): numpy volumes [nx,ny,nz] with their voxel-to-world affines, `options` those of
    register.register (dof=6, cost='corratio' | 'normcorr' | 'leastsq' | 'mi' | 'nmi', n_bins, scales_mm, init, search_deg, mask, min_overlap, xtol,
    ftol, max_sweeps, batch, device).  'mi' and 'nmi' (mutual information and its normalised form, met2_register_joint_cost) assume only a
    statistical dependence between the two contrasts: the measures to fall back to where 'corratio' locks onto the wrong structure.
    -> world [4, 4], fixed-world mm -> moving-world mm: what resample.voxel_matrix(fixed_affine, moving_affine, world) takes to bring
    `moving`, or a label image that lies in its space, onto the grid of `fixed`."""
    from . import register
    return register.register(fixed, fixed_affine, moving, moving_affine, **options)["world"]


def warp_register_filter(fixed, fixed_affine, moving, moving_affine, world=None, **options):
    """Non-linear (deformable) registration of `moving` onto `fixed` after the rigid or affine `world` of register_filter (None: the
    identity): greedy registration with the squared local normalised cross-correlation, coarse to fine, its stages on the device (warp.register
    states the loop and the options: radius, step, sigma_fluid, sigma_elastic, iters, scales_mm, device; met2_warp_lncc in include/met2_hip.h
    the metric and its force).  The metric is that of ANTs' CC and of `greedy -m NCC`, the force their centre-voxel approximation of its
    gradient; parity with ANTs, greedy or fnirt is unpinned: none was available.
    -> dict(disp [nx, ny, nz, 3]: the displacement field on the grid of `fixed`, in its voxels -- what warp_filter and warp_labels_filter take
    together with resample.voxel_matrix(fixed_affine, moving_affine, world) --, world, levels: per level its shape, iterations and metric trace)."""
    from . import warp
    return warp.register(fixed, fixed_affine, moving, moving_affine, world, **options)


def warp_filter(vol, A, disp, order=1, cval=0.0, series_axis=-1, return_inside=False, device=0):
    """resample_filter through a displacement field (met2_warp): the grid is that of `disp` [mx, my, mz, 3], whose voxel x samples `vol` at
    A (x + disp(x)); order 0 or 1; `vol` 3-D or 4-D as in resample_filter.  -> the warped array in the layout of `vol`; return_inside=True:
    (array, inside [mx, my, mz] uint8).  numpy in -> numpy out, CUDA tensor in -> tensors out."""
    from . import warp
    if series_axis not in (-1, 0, 3):
        raise ValueError("series_axis must be -1 ([nx,ny,nz,S]) or 0 ([S,nx,ny,nz])")
    return warp.warp(vol, A, disp, order=order, cval=cval, layout="series" if series_axis == 0 else "voxel", device=device, return_inside=return_inside)


def warp_labels_filter(labels, A, disp, fill=0, device=0):
    """resample_labels_filter through a displacement field (met2_warp_labels): nearest neighbour, `fill` where a voxel falls outside the
    label image.  -> int32 on the grid of `disp`.  numpy in -> numpy out, CUDA tensor in -> tensor out."""
    from . import warp
    return warp.warp_labels(labels, A, disp, fill=fill, device=device)


def warp_invert_filter(disp, A, shape, n_iter=20, device=0):
    """The inverse of the transform (A, disp) of warp_filter -- voxel x of the grid of `disp` samples at A (x + disp(x)) -- in the same form, on
    the other grid: `shape` is that of the image A leads to.  Fixed-point iteration (Chen et al., Med. Phys. 35:81-88, 2008; warp.invert holds
    the loop, met2_warp_invert_step in include/met2_hip.h the step), `n_iter` steps, no convergence test: it converges only where the field
    is a contraction, so judge `residual` and warp_jacobian_filter's count.  Parity with antsApplyTransforms -i or invwarp is unpinned: none
    was available.
    -> dict(disp [shape + (3,)] in voxels of that grid, B [3, 4] = A^-1 -- what warp_filter and warp_labels_filter take to bring an image on
    the grid of the original field onto `shape` --, inside [shape] uint8: 1 where the last step sampled the original field within its grid,
    residual [n_iter]: the largest change of every step in voxels)."""
    from . import warp
    return warp.invert(disp, A, shape, n_iter=n_iter, device=device)


def warp_jacobian_filter(disp, scale=1.0, device=0):
    """The Jacobian determinant of x -> x + disp(x) on the grid of `disp` [nx, ny, nz, 3], times `scale` (met2_warp_jacobian: central
    differences, one-sided at the rim), and the number of voxels at which it is not > 0: there the field folds and has no inverse.
    -> (det [nx, ny, nz], n_nonpositive).  numpy in -> (numpy, int), CUDA tensor in -> tensors."""
    from . import warp
    return warp.jacobian(disp, scale=scale, device=device)


def maps_to_template_filter(res, affine, template_shape, template_affine, world=None, disp=None, order=1, n_iter=20, device=0):
    """The STAT_QUANTITIES maps of a result dict of recon_met2_arrays onto the grid of a template: the direction opposite to
    atlas_stats_filter, for voxel-wise comparison across subjects.  `affine` is the maps' voxel-to-world affine, template_shape and
    template_affine the template's grid, `world` [4, 4] the matrix of atlas_stats_filter (the maps' world mm -> the template's; None: both
    share scanner space), disp [nx, ny, nz, 3] the field of warp_register_filter on the maps' grid (applied after `world`).  With
    A = resample.voxel_matrix(affine, template_affine, world) and B = A^-1: without a field the maps go through resample_filter with B alone;
    with one its inverse is taken (warp_invert_filter, n_iter steps) and they go through warp_filter with (B, inverse field), order 0 or 1.
    Voxels of the template that fall outside the maps get 0.
    -> dict(the maps by name on the template grid, inside [template_shape] uint8, inverse_disp [template_shape + (3,)] (None without a
    field), residual [n_iter] (empty without a field), jacobian [nx, ny, nz] on the maps' grid: det(I + grad disp), the local volume change
    of the field alone in voxels (None without a field), n_nonpositive: the number of its voxels that are not > 0)."""
    from . import resample, warp
    shape = resample._dims(template_shape, "template", disp is not None)     # a field lives on grids of at most 512 voxels per axis
    A = resample.voxel_matrix(affine, template_affine, world)
    B = np.ascontiguousarray(resample.invert(A)[:3])
    maps_shape = tuple(np.shape(res[STAT_QUANTITIES[0]]))
    stack = np.stack([np.asarray(res[k].cpu() if torch.is_tensor(res[k]) else res[k], dtype=np.float64) for k in STAT_QUANTITIES])
    out = {"inverse_disp": None, "residual": np.zeros(0), "jacobian": None, "n_nonpositive": 0}
    if disp is None:
        on_tpl, inside = resample_filter(stack, B, shape, order=order, cval=0.0, device=device, return_inside=True, series_axis=0)
    else:
        if tuple(np.shape(disp)) != maps_shape + (3,):
            raise ValueError("disp must be [nx,ny,nz,3] on the grid of the maps")
        if isinstance(order, bool) or order not in (0, 1):
            raise ValueError("order must be 0 (nearest) or 1 (trilinear) through a field")
        disp = np.asarray(disp.cpu() if torch.is_tensor(disp) else disp, dtype=np.float64)
        inv = warp.invert(disp, A, shape, n_iter=n_iter, device=device)
        on_tpl, inside = warp_filter(stack, B, inv["disp"], order=order, cval=0.0, series_axis=0, return_inside=True, device=device)
        det, count = warp.jacobian(disp, 1.0, device=device)
        out.update(inverse_disp=inv["disp"], residual=inv["residual"], jacobian=det, n_nonpositive=count)
    out.update({k: on_tpl[i] for i, k in enumerate(STAT_QUANTITIES)}, inside=inside)
    return out


GROUP_VOLUMES = ("tstat", "cope", "p_uncorrected", "p_fwe")
GROUP_F_VOLUMES = ("fstat", "p_uncorrected", "p_fwe")              # of an F-contrast: no cope, no tstat
# the spatial statistics' maps (group.randomise(tfce=..., cluster_threshold=...)): the statistic is 0 outside the mask, a p-value 1
GROUP_SPATIAL_VOLUMES = ("tfce", "p_tfce_uncorrected", "p_tfce_fwe", "cluster_extent", "p_cluster_uncorrected", "p_cluster_fwe", "cluster_mass",
                         "p_mass_uncorrected", "p_mass_fwe")
GROUP_SPATIAL_COUNTS = ("tfce_count", "cluster_count", "mass_count")


def group_stats_filter(volumes, X, c=None, mask=None, tfce=None, cluster_threshold=None, cluster_connectivity=26, f_contrast=None, variance_smoothing=None,
                       cluster_mass_threshold=None, **options):
    """The permutation test of the t-contrast c in the design X [n, p] at every voxel of n subjects' volumes [n, x, y, z] on one grid (the
    <map>_in_template volumes of maps_to_template_filter): group.randomise on the voxels of `mask` (None: all), unfolded into volumes.
    options: n_perm, seed, exchange ('permute' | 'flip'), two_sided, device, batch_stat -- group.randomise's.
    tfce (True or a dict of E, H, dh, connectivity) and / or cluster_threshold (with cluster_connectivity) add the spatial statistics, for
    which the grid and the voxels' places in it are handed on (options then also: batch_spatial, work_bytes): tfce, p_tfce_uncorrected,
    p_tfce_fwe, tfce_count, cluster_extent, p_cluster_uncorrected, p_cluster_fwe and cluster_count as volumes too.  cluster_mass_threshold
    (with the same cluster_connectivity) adds the cluster mass in the same way: cluster_mass, p_mass_uncorrected, p_mass_fwe and mass_count.
    -> its dict with tstat, cope, p_uncorrected, p_fwe and count as [x, y, z] volumes (outside the mask t = 0, cope = 0, p = 1, count =
    n_perm) and mask [x, y, z] bool: the voxels that were tested.  Parity with FSL randomise is unpinned: FSL was not available.
    f_contrast [s, p] in the place of c: the F-test of its rows at once (group.randomise(f_contrast=...)), with fstat in the place of tstat and
    cope (outside the mask F = 0), dof = (s, n - r) and f_crit; the spatial statistics are then taken on F.
    variance_smoothing = sigma or (sx, sy, sz), in VOXELS (the filter has no affine): handed on to group.randomise with the grid and the
    voxels' places; tstat is then the pseudo-t and every p-value, and the spatial statistics, are taken on it."""
    from . import group
    vols = np.asarray(volumes.cpu() if torch.is_tensor(volumes) else volumes, dtype=np.float64)
    if vols.ndim != 4:
        raise ValueError("volumes must be [n, x, y, z]: one volume per subject")
    shape = vols.shape[1:]
    m = np.ones(shape, dtype=bool) if mask is None else np.asarray(mask.cpu() if torch.is_tensor(mask) else mask) != 0
    if m.shape != shape:
        raise ValueError("the mask does not lie on the grid of the volumes")
    at = np.flatnonzero(m.reshape(-1))
    if (tfce is not None and tfce is not False) or cluster_threshold is not None:
        options = dict(options, tfce=tfce, cluster_threshold=cluster_threshold, cluster_connectivity=cluster_connectivity, grid=shape, at=at)
    if f_contrast is not None:
        options = dict(options, f_contrast=f_contrast)
    if variance_smoothing is not None:
        options = dict(options, variance_smoothing=variance_smoothing, grid=shape, at=at)
    if cluster_mass_threshold is not None:
        options = dict(options, cluster_mass_threshold=cluster_mass_threshold, cluster_connectivity=cluster_connectivity, grid=shape, at=at)
    res = group.randomise(np.ascontiguousarray(vols.reshape(vols.shape[0], -1)[:, at]), X, c, **options)
    for key in (GROUP_VOLUMES if f_contrast is None else GROUP_F_VOLUMES) + tuple(k for k in GROUP_SPATIAL_VOLUMES if k in res):
        vol = np.full(int(np.prod(shape)), 1.0 if key.startswith("p_") else 0.0)
        vol[at] = res[key]
        res[key] = vol.reshape(shape)
    for key in ("count",) + tuple(k for k in GROUP_SPATIAL_COUNTS if k in res):
        count = np.full(int(np.prod(shape)), res["n_perm"], dtype=np.uint32)
        count[at] = res[key]
        res[key] = count.reshape(shape)
    res.update(mask=m)
    return res


def tfce_filter(vol, mask=None, dh=None, E=0.5, H=2.0, connectivity=6, device=0):
    """Threshold-free cluster enhancement of one volume [x, y, z] (group.tfce: csrc/met2_tfce.hip) -> the enhanced volume.  mask: the voxels that
    take part (None: all); dh None: a hundredth of the volume's largest finite value inside the mask; connectivity 6 | 18 | 26.  numpy in,
    numpy out; a CUDA tensor in, a tensor on its device out."""
    from . import group
    is_t = torch.is_tensor(vol)
    a = np.asarray(vol.cpu() if is_t else vol, dtype=np.float64)
    if a.ndim != 3:
        raise ValueError("vol must be [x, y, z]")
    m = None if mask is None else np.asarray(mask.cpu() if torch.is_tensor(mask) else mask) != 0
    out = group.tfce(a, m, dh=dh, E=E, H=H, connectivity=connectivity, device=vol.device.index or 0 if is_t and vol.is_cuda else device)
    return torch.as_tensor(out, device=vol.device) if is_t else out


def atlas_stats_filter(res, labels, labels_affine, affine, world=None, q=None, device=0, template=None, template_affine=None, register=None,
                       reference=None, nonlinear=None, disp=None):
    """label_stats_filter for a label image that does not lie on the grid of the maps: `labels` [lx,ly,lz] integers with the voxel-to-world
    affine `labels_affine`, `affine` the maps' own (both as nifti.load gives them), `world` [4, 4] taking the maps' world mm to the label
    image's (None: both share scanner space; resample.from_flirt reads a FLIRT matrix).  The labels are resampled onto the maps' grid
    (resample_labels_filter, nearest neighbour, 0 outside) and the statistics taken there.
    template [tx,ty,tz]: an intensity image in the label image's world space (template_affine; None: labels_affine), the atlas' anatomical
    image.  `world` is then estimated: the template is registered (register_filter, options `register`: a dict, e.g. {"cost": "nmi"}) to `reference`, a volume on the
    maps' grid (None: res['TWC']).  A template together with a world matrix is refused.
    nonlinear (with a template): True, or a dict of warp_register_filter's options -- after the affine registration the template is registered
    non-linearly to the reference from that `world`, and the labels go through the displacement field (warp_labels_filter).  disp
    [nx,ny,nz,3]: a field estimated before, on the maps' grid, applied after `world` (not together with nonlinear).
    -> the dict of label_stats_filter plus labels_resampled [nx,ny,nz] int32, with a template world [4, 4], and with nonlinear disp and
    warp_levels (the levels of warp_register_filter)."""
    from . import resample
    if template is None and (template_affine is not None or register is not None or reference is not None):
        raise ValueError("template_affine, register and reference go with a template")
    if nonlinear is not None and not (nonlinear is True or isinstance(nonlinear, dict)):
        raise ValueError("nonlinear must be None, True or a dict of warp_register_filter's options")
    if nonlinear is not None and template is None:
        raise ValueError("nonlinear goes with a template: the field is estimated from the template")
    if nonlinear is not None and disp is not None:
        raise ValueError("give nonlinear or a field estimated before, not both")
    if template is not None:
        if world is not None:
            raise ValueError("give a template or a world matrix, not both")
        ref = res["TWC"] if reference is None else reference
        ref = ref.cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
        tpl = template.cpu().numpy() if torch.is_tensor(template) else np.asarray(template)
        tpl_affine = labels_affine if template_affine is None else template_affine
        world = register_filter(ref, affine, tpl, tpl_affine, **dict(register or {}, device=device))
        if nonlinear is not None:
            nl = warp_register_filter(ref, affine, tpl, tpl_affine, world, **dict({"device": device}, **(nonlinear if isinstance(nonlinear, dict) else {})))
            disp = nl["disp"]
    A = resample.voxel_matrix(affine, labels_affine, world)
    shape = tuple(np.shape(res["MWF"]))
    if disp is None:
        lab = resample_labels_filter(labels, A, shape, fill=0, device=device)
    else:
        if tuple(np.shape(disp)) != shape + (3,):
            raise ValueError("disp must be [nx,ny,nz,3] on the grid of the maps")
        lab = warp_labels_filter(labels, A, disp, fill=0, device=device)
    out = label_stats_filter(res, lab, q=q, device=device)
    out["labels_resampled"] = lab.cpu().numpy() if torch.is_tensor(lab) else lab
    if template is not None:
        out["world"] = world
    if nonlinear is not None:
        out["disp"], out["warp_levels"] = disp, nl["levels"]
    return out


def gaussian_weights(sigma, truncate=4.0):
    """(radius, weights [2 radius + 1]) of scipy.ndimage.gaussian_filter1d: what met2_smooth_separable takes"""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return radius, np.ascontiguousarray(w / w.sum(), dtype=np.float64)


def gaussian_smooth(data, sigma=2.0, truncate=4.0, device=0):
    """The Gaussian pre-smoothing of the FA step (motor:337-343): every echo volume of data [nx,ny,nz,nt] through the
    equivalent of scipy.ndimage.gaussian_filter(volume, sigma) (mode 'reflect', truncate 4), on the device, bit-identical
    to scipy.  numpy in -> numpy out, CUDA tensor in -> tensor out."""
    dd, dev, as_numpy = _enter(data, device)
    if dd.dim() != 4:
        raise ValueError("data must be [nx,ny,nz,nt]")
    radius, w = gaussian_weights(sigma, truncate)
    out = torch.empty_like(dd)
    work = torch.empty_like(dd)
    _call(dev, "met2_smooth_separable", *dd.shape, radius, w.ctypes.data_as(_dp), dd.data_ptr(), out.data_ptr(), work.data_ptr())
    torch.cuda.current_stream(dev).synchronize()                     # `work` and the host weights stay alive until here
    return _leave(out, as_numpy)
