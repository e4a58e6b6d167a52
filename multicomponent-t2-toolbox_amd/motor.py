"""Drop-ins for motor/motor_recon_met2_real_data.py: create_Laplacian_matrix, fitting_slice_T2, the NESMA filter, the MP-PCA filter
(mppca_filter: an extension), the Gibbs-ringing filter (gibbs_filter: the mrdegibbs step of the reference's example script), recon_met2_arrays (the driver's steps 1-4 on in-memory arrays), motor_recon_met2 (the same with the on-disk
contract) and the ROI mode (recon_met2_rois, motor_recon_met2_ROIs).  Plots and the mean-spectrum PNG are not reproduced."""
import math

import numpy as np
import torch

from ._cache import plan_for
from ._lib import _dp, check, lib
from .plan import MAP_NAMES, Met2Plan


def create_Laplacian_matrix(Npc, order):
    """motor:86-111 -> dense [Npc, Npc]"""
    L = np.zeros((Npc, Npc))
    i = np.arange(Npc)
    if order == 2:
        L[i, i] = 2.0
        L[i[1:], i[1:] - 1] = -1.0
        L[i[:-1], i[:-1] + 1] = -1.0
        L[0, 0] = 1.0
        L[-1, -1] = 1.0
    elif order == 1:
        L[i, i] = 1.0
        L[i[1:], i[1:] - 1] = -1.0
    elif order == 0:
        L[i, i] = 1.0
    else:
        raise ValueError("order must be 0, 1 or 2")
    return L


def create_InvT2_matrix(T2s):
    """motor:263-269 (reg_matrix == 'InvT2')"""
    T2s = np.asarray(T2s, dtype=np.float64)
    d = T2s - np.concatenate(([T2s[0] - 1.0], T2s[:-1]))
    d[0] = d[1]
    return np.diag(1.0 / d)


def penalty_matrix(reg_matrix, Npc, T2s=None):
    """motor:254-273; unknown names raise (the reference calls sys.exit())."""
    if reg_matrix == "I":
        return create_Laplacian_matrix(Npc, 0)
    if reg_matrix == "L1":
        return create_Laplacian_matrix(Npc, 1)
    if reg_matrix == "L2":
        return create_Laplacian_matrix(Npc, 2)
    if reg_matrix == "InvT2":
        return create_InvT2_matrix(T2s)
    raise ValueError("Error: Wrong reg_matrix option!")


def fitting_slice_T2(mask_1d, data_1d, FA_index_1d, nx, Dic_3D, lambda_reg, T2dim, nEchoes, reg_method, Laplac, dist_x_prior=None):
    """motor:113-162 -> (f_sol[nx, T2dim], signal[nx, nEchoes], reg[nx])"""
    data = np.ascontiguousarray(data_1d, dtype=np.float64)
    if not np.isfinite(data[np.asarray(mask_1d) > 0]).all():
        raise ValueError("array must not contain infs or NaNs")     # algorithms.py:56
    plan = plan_for(Dic_3D, Laplac, lambda_reg)
    dev = plan.device
    out = plan.fit(reg_method, torch.as_tensor(data, device=dev), fa_index=torch.as_tensor(np.asarray(FA_index_1d, dtype=np.float64), device=dev),
                   mask=torch.as_tensor(np.asarray(mask_1d) > 0, device=dev), want_maps=False)
    return out["fsol"].cpu().numpy(), out["sig"].cpu().numpy(), out["reg"].cpu().numpy()


def nesma_filter(data, mask, device=0):
    """The NESMA filter of the driver (motor:305-333) on the device: `data` [nx,ny,nz,nt] as the driver holds it at
    that point (multiplied by the mask, negatives clipped), `mask` [nx,ny,nz]; voxels with mask == 1 become the
    mean of the similar voxels (relative L1 distance < 2.5 %) of their 12^3 window, all others zero.  Accepts numpy
    arrays (returns numpy) or CUDA tensors (returns a tensor on the same device)."""
    as_numpy = not torch.is_tensor(data)
    dev = torch.device("cuda", device) if as_numpy else data.device
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 4 or tuple(np.shape(mask)) != tuple(dd.shape[:3]):
        raise ValueError("data must be [nx,ny,nz,nt] and mask [nx,ny,nz]")
    mk = (torch.as_tensor(mask, device=dev) == 1).to(torch.uint8).contiguous()
    out = torch.empty_like(dd)
    nx, ny, nz, nt = dd.shape
    with torch.cuda.device(dev):
        check(lib().met2_nesma(dev.index or 0, nx, ny, nz, nt, dd.data_ptr(), mk.data_ptr(), out.data_ptr(),
                               torch.cuda.current_stream(dev).cuda_stream))
    return out.cpu().numpy() if as_numpy else out


def mppca_filter(data, mask, window=5, device=0, return_maps=False):
    """Marchenko-Pastur PCA denoising (Veraart et al., NeuroImage 2016; met2_mppca in include/met2_hip.h states the algorithm) on the
    device: `data` [nx,ny,nz,nt], 2 <= nt <= 63, `mask` [nx,ny,nz]; every voxel with mask != 0 is projected on the signal subspace of
    the decay curves of its window^3 patch (masked voxels only), all others become zero.  The output is not clipped.
    return_maps=True: (denoised, sigma [nx,ny,nz] the noise level, rank [nx,ny,nz] int32 the components kept; -1 where the patch holds
    a non-finite value and -2 where the eigen-solver gave up, both copied through).  numpy in -> numpy out, CUDA tensor in -> tensors out."""
    as_numpy = not torch.is_tensor(data)
    dev = torch.device("cuda", device) if as_numpy else data.device
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 4 or tuple(np.shape(mask)) != tuple(dd.shape[:3]):
        raise ValueError("data must be [nx,ny,nz,nt] and mask [nx,ny,nz]")
    mk = (torch.as_tensor(mask, device=dev) != 0).to(torch.uint8).contiguous()
    out = torch.empty_like(dd)
    nx, ny, nz, nt = dd.shape
    sigma = torch.empty((nx, ny, nz), dtype=torch.float64, device=dev) if return_maps else None
    rank = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev) if return_maps else None
    with torch.cuda.device(dev):
        check(lib().met2_mppca(dev.index or 0, nx, ny, nz, nt, dd.data_ptr(), mk.data_ptr(), int(window), out.data_ptr(),
                               sigma.data_ptr() if return_maps else None, rank.data_ptr() if return_maps else None,
                               torch.cuda.current_stream(dev).cuda_stream))
    if not return_maps:
        return out.cpu().numpy() if as_numpy else out
    return tuple(t.cpu().numpy() for t in (out, sigma, rank)) if as_numpy else (out, sigma, rank)


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
    as_numpy = not torch.is_tensor(data)
    dev = torch.device("cuda", device) if as_numpy else data.device
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 4:
        raise ValueError("data must be [nx,ny,nz,nt]")
    out = torch.empty_like(dd)
    nx, ny, nz, nt = dd.shape
    shifts = tuple(torch.empty(dd.shape, dtype=torch.int8, device=dev) for _ in range(3 if mode == "3d" else 2)) if return_shifts else ()
    entry = lib().met2_degibbs3d if mode == "3d" else lib().met2_degibbs
    ptrs = [s.data_ptr() for s in shifts] if return_shifts else [None] * (3 if mode == "3d" else 2)
    with torch.cuda.device(dev):
        check(entry(dev.index or 0, nx, ny, nz, nt, dd.data_ptr(), int(nshifts), int(minW), int(maxW), out.data_ptr(), *ptrs,
                    torch.cuda.current_stream(dev).cuda_stream))
    if not return_shifts:
        return out.cpu().numpy() if as_numpy else out
    return tuple(t.cpu().numpy() for t in (out,) + shifts) if as_numpy else (out,) + shifts


def _degibbs_first(data, degibbs, prepared, device):
    """degibbs='yes' or '3d' of the drivers: the raw volume through gibbs_filter, before anything else -> the volume to go on with"""
    if degibbs not in ("no", "yes", "3d"):
        raise ValueError("degibbs must be 'no', 'yes' or '3d'")
    if degibbs == "no":
        return data
    if prepared:
        raise ValueError("degibbs='%s' works on the raw volume and does not go with prepared=True" % degibbs)
    if np.ndim(data) != 4:
        raise ValueError("degibbs='%s' needs data [nx,ny,nz,nt]" % degibbs)
    return gibbs_filter(np.asarray(data, dtype=np.float64), device=device, mode="3d" if degibbs == "3d" else "2d")


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
    vox = np.ascontiguousarray(np.asarray(voxel_size, dtype=np.float64).reshape(-1))
    if vox.shape != (3,):
        raise ValueError("voxel_size must be (dx, dy, dz)")
    dev = torch.device("cuda", device) if as_numpy else data.device
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() == 4:
        dd = bet.bet_mean(dd)
    nx, ny, nz = dd.shape
    mask = torch.empty(dd.shape, dtype=torch.uint8, device=dev)
    n = 4 ** min(max(int(level), 0), 4)
    verts = torch.empty((10 * n + 2, 3), dtype=torch.float64, device=dev) if return_surface else None
    st = np.zeros(8, dtype=np.float64)
    with torch.cuda.device(dev):
        check(lib().met2_brain_mask(dev.index or 0, nx, ny, nz, dd.data_ptr(), vox.ctypes.data_as(_dp), float(f), int(level), int(n_iter),
                                    mask.data_ptr(), verts.data_ptr() if return_surface else None, st.ctypes.data_as(_dp),
                                    torch.cuda.current_stream(dev).cuda_stream))
    if not return_surface:
        return mask.cpu().numpy() if as_numpy else mask
    stats = {k: float(x) for k, x in zip(bet.STAT_KEYS, st)}
    return (mask.cpu().numpy() if as_numpy else mask, verts.cpu().numpy() if as_numpy else verts, bet.bet_mesh(level)[1], stats)


def _brain_mask_check(brain_mask, mask, data, voxel_size, prepared, distributed):
    """brain_mask of the drivers, checked before any device work -> True when the step is to run"""
    if brain_mask not in ("no", "yes"):
        raise ValueError("brain_mask must be 'no' or 'yes'")
    if brain_mask == "no":
        return False
    if mask is not None:
        raise ValueError("brain_mask='yes' makes the mask itself and does not go with a mask")
    if prepared:
        raise ValueError("brain_mask='yes' works on the raw volume and does not go with prepared=True")
    if distributed:
        raise ValueError("brain_mask='yes' does not go with distributed=True")
    if np.ndim(data) != 4:
        raise ValueError("brain_mask='yes' needs data [nx,ny,nz,nt]")
    if voxel_size is None or np.shape(voxel_size) != (3,):
        raise ValueError("brain_mask='yes' needs voxel_size=(dx, dy, dz) in mm")
    return True


def bias_field_filter(vol, mask=None, voxel_size=(1, 1, 1), n_class=3, n_outer=4, n_em=10, fwhm=20.0, device=0, return_field=False):
    """Bias-field correction of a 3-D map (met2_bias_field in include/met2_hip.h states the algorithm: the EM estimator of Wells et al. 1996
    and Guillemaud & Brady 1997, which FSL's fast iterates, without fast's Markov random field term) on the device: `vol` [nx,ny,nz], `mask`
    [nx,ny,nz] or None (every voxel), `voxel_size` (dx, dy, dz) in mm.  The defaults are those of the reference's example script
    (fast -n 3 -I 4 -l 20.0); parity with fast itself is unpinned.  The field is estimated on the masked voxels that are finite and positive
    and divided out wherever it is defined; non-finite voxels are copied through.
    return_field=True: (corrected, field, classes [3 n_class] = the final class means and variances of log(vol) and the class weights).
    numpy in -> numpy out, CUDA tensor in -> tensors out."""
    as_numpy = not torch.is_tensor(vol)
    dev = torch.device("cuda", device) if as_numpy else vol.device
    dd = torch.as_tensor(vol, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 3 or (mask is not None and tuple(np.shape(mask)) != tuple(dd.shape)):
        raise ValueError("vol must be [nx,ny,nz] and mask the same shape")
    vox = np.asarray(voxel_size, dtype=np.float64).reshape(-1)
    if vox.shape != (3,):
        raise ValueError("voxel_size must be (dx, dy, dz)")
    mk = None if mask is None else (torch.as_tensor(mask, device=dev) != 0).to(torch.uint8).contiguous()
    out = torch.empty_like(dd)
    nx, ny, nz = dd.shape
    field = torch.empty_like(dd) if return_field else None
    classes = torch.empty(3 * max(int(n_class), 0), dtype=torch.float64, device=dev) if return_field else None
    with torch.cuda.device(dev):
        check(lib().met2_bias_field(dev.index or 0, nx, ny, nz, dd.data_ptr(), None if mk is None else mk.data_ptr(),
                                    vox.ctypes.data_as(_dp), int(n_class), int(n_outer), int(n_em), float(fwhm), out.data_ptr(),
                                    field.data_ptr() if return_field else None, classes.data_ptr() if return_field else None,
                                    torch.cuda.current_stream(dev).cuda_stream))
    if not return_field:
        return out.cpu().numpy() if as_numpy else out
    return tuple(t.cpu().numpy() for t in (out, field, classes)) if as_numpy else (out, field, classes)


def _bias_check(bias_correct, vol_shape, voxel_size, distributed):
    """bias_correct of the drivers, checked before any device work -> True when the step is to run"""
    if bias_correct not in ("no", "yes"):
        raise ValueError("bias_correct must be 'no' or 'yes'")
    if bias_correct == "no":
        return False
    if distributed:
        raise ValueError("bias_correct='yes' does not go with distributed=True: the map is complete only after the gather")
    if len(vol_shape) != 3:
        raise ValueError("bias_correct='yes' needs data [nx,ny,nz,nt]")
    if voxel_size is None or np.shape(voxel_size) != (3,):
        raise ValueError("bias_correct='yes' needs voxel_size=(dx, dy, dz) in mm")
    return True


def _bias_last(res, mask, voxel_size, device):
    """bias_correct='yes' of the drivers: res['TWC'] through bias_field_filter with the driver's mask -> the corrected map, and 'TWC_bias'"""
    twc, field, _ = bias_field_filter(np.ascontiguousarray(res["TWC"], dtype=np.float64), np.asarray(mask) != 0, voxel_size, device=device,
                                      return_field=True)
    res["TWC"] = twc
    res["TWC_bias"] = field


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
    as_numpy = not torch.is_tensor(vol)
    dev = torch.device("cuda", device) if as_numpy else vol.device
    dd = torch.as_tensor(vol, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 3 or (mask is not None and tuple(np.shape(mask)) != tuple(dd.shape)):
        raise ValueError("vol must be [nx,ny,nz] and mask the same shape")
    vox = np.asarray(voxel_size, dtype=np.float64).reshape(-1)
    if vox.shape != (3,):
        raise ValueError("voxel_size must be (dx, dy, dz)")
    mk = None if mask is None else (torch.as_tensor(mask, device=dev) != 0).to(torch.uint8).contiguous()
    K = max(int(n_class), 0)
    seg = torch.zeros(tuple(dd.shape), dtype=torch.uint8, device=dev)
    prob = torch.zeros((K,) + tuple(dd.shape), dtype=torch.float64, device=dev) if return_prob else None
    classes = torch.zeros(3 * K, dtype=torch.float64, device=dev) if return_prob else None
    nx, ny, nz = dd.shape
    with torch.cuda.device(dev):
        check(lib().met2_tissue_segment(dev.index or 0, nx, ny, nz, dd.data_ptr(), None if mk is None else mk.data_ptr(), vox.ctypes.data_as(_dp),
                                        int(n_class), float(beta), int(n_outer), int(n_em), int(n_icm), seg.data_ptr(),
                                        prob.data_ptr() if return_prob else None, classes.data_ptr() if return_prob else None,
                                        torch.cuda.current_stream(dev).cuda_stream))
    if not return_prob:
        return seg.cpu().numpy() if as_numpy else seg
    return tuple(t.cpu().numpy() for t in (seg, prob, classes)) if as_numpy else (seg, prob, classes)


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
    vox = np.asarray(voxel_size, dtype=np.float64).reshape(-1)
    if vox.shape != (3,):
        raise ValueError("voxel_size must be (dx, dy, dz)")
    as_numpy = not torch.is_tensor(vol)
    dev = torch.device("cuda", device) if as_numpy else vol.device
    dd = torch.as_tensor(vol, dtype=torch.float64, device=dev).contiguous()
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
    nx, ny, nz = dd.shape
    with torch.cuda.device(dev):
        check(lib().met2_partial_volume(dev.index or 0, nx, ny, nz, dd.data_ptr(), sg.data_ptr(), pr.data_ptr(), vox.ctypes.data_as(_dp),
                                        int(n_class), float(beta_pv), int(n_icm), pve.data_ptr(), pveseg.data_ptr(), mixel.data_ptr(),
                                        classes.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    out = (pve, pveseg, mixel, classes)
    return tuple(t.cpu().numpy() for t in out) if as_numpy else out


def _segment_check(segment, bias_correct, distributed):
    """segment of the drivers, checked before any device work -> True when the step is to run"""
    if segment not in ("no", "yes", "pve"):
        raise ValueError("segment must be 'no', 'yes' or 'pve'")
    if segment == "no":
        return False
    if bias_correct != "yes":
        raise ValueError("segment='%s' needs bias_correct='yes': the bias-corrected map is what is segmented" % segment)
    if distributed:
        raise ValueError("segment='%s' does not go with distributed=True: the map is complete only after the gather" % segment)
    return True


def _segment_last(res, mask, voxel_size, device, segment="yes"):
    """segment='yes' of the drivers, after _bias_last: the corrected res['TWC'] through tissue_segment_filter -> 'TWC_seg', 'TWC_prob';
    segment='pve': those, then partial_volume_filter on them -> 'TWC_pve', 'TWC_pveseg', 'TWC_mixeltype'"""
    twc = np.ascontiguousarray(res["TWC"], dtype=np.float64)
    seg, prob, _ = tissue_segment_filter(twc, np.asarray(mask) != 0, voxel_size, device=device)
    res["TWC_seg"] = seg
    res["TWC_prob"] = prob
    if segment == "pve":
        res["TWC_pve"], res["TWC_pveseg"], res["TWC_mixeltype"], _ = partial_volume_filter(twc, None, voxel_size, device=device, seg=seg, prob=prob)


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


def _tissue_stats_check(tissue_stats, segment, distributed, pve_threshold=0.9):
    """tissue_stats of the drivers, checked before any device work -> True when the step is to run"""
    if tissue_stats not in ("no", "yes"):
        raise ValueError("tissue_stats must be 'no' or 'yes'")
    if tissue_stats == "no":
        return False
    if segment not in ("yes", "pve"):
        raise ValueError("tissue_stats='yes' needs segment='yes' or 'pve': the tissue classes are the labels")
    if distributed:
        raise ValueError("tissue_stats='yes' does not go with distributed=True: the maps are complete only after the gather")
    if not 0.5 <= float(pve_threshold) < 1.0:
        raise ValueError("pve_threshold must lie in [0.5, 1), so that no voxel carries two labels")
    return True


def tissue_labels(res, segment, pve_threshold=0.9):
    """the label volume tissue_stats='yes' uses: segment='yes' -> TWC_seg (1..3); 'pve' -> k + 1 where TWC_pve[k] > pve_threshold, else 0"""
    if segment != "pve":
        return np.asarray(res["TWC_seg"]).astype(np.int32)
    pve = np.asarray(res["TWC_pve"])
    lab = np.zeros(pve.shape[1:], dtype=np.int32)
    for k in range(pve.shape[0]):
        lab[pve[k] > pve_threshold] = k + 1
    return lab


def _tissue_stats_last(res, dd, plan, segment, pve_threshold, myelin_T2):
    """tissue_stats='yes' of the drivers, after _segment_last, on the plan's device: label_stats_filter on the tissue labels -> the dict
    res['tissue_stats'], plus 'all' (the same statistics, one row, of the whole segmented domain TWC_seg > 0) and 'mean_signal_fsol'
    [L + 1, n_t2] with 'mean_signal_<map>' [L + 1]: the X2 fit with penalty I and factor 1.01 of every label's mean signal on its mean
    kernel (motor:379-403's dist_T2_mean2, per tissue; the last row the whole domain), by recon_met2_rois on the prepared data `dd` and
    the run's flip-angle indices."""
    device = plan.device.index or 0
    lab = tissue_labels(res, segment, pve_threshold)
    whole = (np.asarray(res["TWC_seg"]) > 0).astype(np.int32)
    if not lab.any():
        raise ValueError("tissue_stats='yes': no voxel carries a tissue label")
    ts = label_stats_filter(res, lab, device=device)
    al = label_stats_filter(res, whole, device=device)
    ts["all"] = {k: al[k][0] for k in STAT_KEYS}
    Id = create_Laplacian_matrix(plan.n_t2, 0)
    data = torch.as_tensor(dd).to(plan.device)
    fits = [recon_met2_rois(data, torch.as_tensor(r, device=plan.device), res["FA_index"], None, res["T2s"], Id, factor=1.01, myelin_T2=myelin_T2,
                            plan=plan) for r in (lab, whole)]
    ts["mean_signal_fsol"] = np.concatenate([f["fsol"] for f in fits])
    for name in MAP_NAMES:
        ts["mean_signal_" + name] = np.concatenate([f[name] for f in fits])
    res["tissue_stats"] = ts


def tissue_stats_tables(ts):
    """the two tables motor_recon_met2 writes from res['tissue_stats'] -> (stats [(L + 1) * 8, 5 + n_q] of objects: label, quantity, n, mean,
    std, q...; spectra [1 + 2 (L + 1), n_t2] of floats: T2s, then per label the normalised mean spectrum and the mean-signal spectrum);
    the whole domain is the last label, 'all'"""
    names = [str(int(x)) for x in ts["labels"]] + ["all"]
    rows, spectra = [], [np.asarray(ts["T2s"], dtype=np.float64)]
    for i, name in enumerate(names):
        src = ts["all"] if name == "all" else {k: ts[k][i] for k in STAT_KEYS}
        for j, quantity in enumerate(ts["quantities"]):
            rows.append([name, quantity, src["n"][j], src["mean"][j], src["std"][j]] + list(src["quantiles"][j]))
        spectra += [src["spectrum_mean"], ts["mean_signal_fsol"][i]]
    return np.array(rows, dtype=object), np.array(spectra, dtype=np.float64)


def gaussian_smooth(data, sigma=2.0, truncate=4.0, device=0):
    """The Gaussian pre-smoothing of the FA step (motor:337-343): every echo volume of data [nx,ny,nz,nt] through the
    equivalent of scipy.ndimage.gaussian_filter(volume, sigma) (mode 'reflect', truncate 4), on the device, bit-identical
    to scipy.  numpy in -> numpy out, CUDA tensor in -> tensor out."""
    as_numpy = not torch.is_tensor(data)
    dev = torch.device("cuda", device) if as_numpy else data.device
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 4:
        raise ValueError("data must be [nx,ny,nz,nt]")
    radius = int(truncate * float(sigma) + 0.5)                      # scipy.ndimage.gaussian_filter1d
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    w = np.ascontiguousarray(w / w.sum(), dtype=np.float64)
    out = torch.empty_like(dd)
    work = torch.empty_like(dd)
    nx, ny, nz, nt = dd.shape
    import ctypes as C
    with torch.cuda.device(dev):
        check(lib().met2_smooth_separable(dev.index or 0, nx, ny, nz, nt, radius, w.ctypes.data_as(C.POINTER(C.c_double)), dd.data_ptr(),
                                          out.data_ptr(), work.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.current_stream(dev).synchronize()                 # `work` and the host weights stay alive until here
    return out.cpu().numpy() if as_numpy else out


def _prepare_volume(data, mask, dev, prepared, denoise, maps=None):
    """The driver's preparation (motor:180-182, :279, :293-333) on the device.  The volume keeps the memory order it
    arrives in (nibabel arrays are Fortran-ordered; the solver reads either order in place).  denoise='MPPCA' (an extension) leaves its
    noise map in maps['MPPCA_sigma'] when the caller hands a dict in."""
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev)
    mk = torch.as_tensor(mask, device=dev)
    if not prepared:
        dd = dd * mk.to(torch.float64).unsqueeze(-1)                # the mask VALUE multiplies (motor:180-182)
        dd = torch.where(dd < 0.0, torch.zeros((), dtype=torch.float64, device=dev), dd)      # motor:279
        if denoise == "NESMA":
            if dd.dim() != 4:
                raise ValueError("NESMA needs data [nx,ny,nz,nt]")
            dd = nesma_filter(dd, mk)
        elif denoise == "TV":
            if dd.dim() != 4:
                raise ValueError("TV denoising needs data [nx,ny,nz,nt]")
            from .tv import tv_denoise_volume
            dd = tv_denoise_volume(dd)
        elif denoise == "MPPCA":
            if dd.dim() != 4:
                raise ValueError("MPPCA needs data [nx,ny,nz,nt]")
            dd, sigma, _ = mppca_filter(dd, mk, return_maps=True)
            dd = torch.where(dd < 0.0, torch.zeros((), dtype=torch.float64, device=dev), dd)   # the projection can undershoot at late echoes
            if maps is not None:
                maps["MPPCA_sigma"] = sigma
    return dd, mk


def _estimate_fa(plan, dd_fa, mm, FA_method, fa_index, T2s, T1s, tau, TR, alpha_values, device):
    """Driver step 2 (motor:349-373) -> float64 FA-index tensor shaped like the volume (dd_fa.shape[:-1]); the smoothed
    volume the angles are estimated on may be laid out differently from the one the spectra are fitted on, so the result
    is handed on by logical voxel position, not in a memory order."""
    from .plan import unflatten, voxel_layout
    _, nvox, _, _, vol, order = voxel_layout(dd_fa, plan.n_te)
    if fa_index is not None:
        return torch.as_tensor(np.asarray(fa_index, dtype=np.float64), device=dd_fa.device).reshape(vol)
    if FA_method == "spline":
        alpha_values_spline = np.linspace(90.0, 180.0, 15)                                      # motor:237
        plan_lr = Met2Plan(plan.n_te, plan.n_t2, 15, device=device)
        try:
            plan_lr.build_dictionary_epg(T2s, T1s, tau, alpha_values_spline, TR, slice_profile=plan.slice_profile)
            fa, _, _ = plan.fa_spline(plan_lr, alpha_values_spline, alpha_values, dd_fa, mm, want_km=False)
        finally:
            plan_lr.close()
    else:
        fa, _, _ = plan.fa_bruteforce(dd_fa, mm)
    return unflatten(fa, vol, order)


def recon_met2_arrays(data, mask, TE_array, TR, reg_method="X2", reg_matrix="L2", FA_method="brute-force", myelin_T2=40.0,
                      fa_index=None, device=0, plan=None, denoise="None", prepared=False, FA_smooth="no", distributed=False,
                      return_prepared=False, devices=None, bootstrap=None, degibbs="no", bias_correct="no", voxel_size=None,
                      brain_mask="no", segment="no", tissue_stats="no", pve_threshold=0.9, rician="no", rician_sigma=None, rician_iters=3,
                      slice_profile=None):
    """Steps 1-4 of motor_recon_met2 (motor:293-373, 427-472) on arrays: data [nx,ny,nz,nt] (or
    [nvox, nt]), mask [nx,ny,nz].  Mirrors the driver's preparation: data *= mask (motor:180-182),
    negative values clipped to 0 (motor:279), optional NESMA / TV filter (motor:293-333, needs a 3-D volume) or denoise='MPPCA'
    (mppca_filter with window 5, an extension; what it leaves below zero is set to zero; return_prepared=True then adds 'MPPCA_sigma'),
    Npc = 60 (96 for T2SPARC, motor:207-213), T2 grid 10..2000 ms, T1 = 1000 ms, 91 flip angles for brute force.
    `prepared=True` says the caller already did that preparation (mask multiply, clip, denoise).
    degibbs='yes' (step 2 of the reference's example script, which runs MRtrix's mrdegibbs there): the raw volume goes through gibbs_filter
    first -- before the mask multiply, the clip and any denoise, so the clip also removes what the unringing leaves below zero; needs data
    [nx,ny,nz,nt]; ValueError with prepared=True; on the devices=[...] path it runs on devices[0], under distributed=True on every rank's own
    copy (it is deterministic).  MRtrix recommends MP-PCA denoising BEFORE unringing: a caller who wants that order calls mppca_filter and
    gibbs_filter themselves and passes prepared=True.  degibbs='3d': the same with gibbs_filter(mode='3d'), for 3-D Fourier-encoded acquisitions
    (every echo volume unrung along x, y and z; needs 8 <= nz <= 256 too).  degibbs='no' (default) changes nothing.
    bias_correct='yes' (step 5 of the reference's example script, which runs FSL's fast on the TWC map there): after everything else the
    total water content map goes through bias_field_filter with the driver's mask and voxel_size=(dx, dy, dz) in mm; 'TWC' becomes the
    corrected map and 'TWC_bias' the estimated field; the other outputs, the bootstrap's included, are not touched.  Needs data [nx,ny,nz,nt]
    and voxel_size; ValueError otherwise and with distributed=True; on the devices=[...] path it runs on devices[0], on the assembled map.
    Parity with fast itself is unpinned (no Markov random field term).  bias_correct='no' (default) changes nothing.
    segment='yes' (the other product of that fast call; needs bias_correct='yes'): the corrected TWC map then goes through
    tissue_segment_filter with the same mask and voxel_size (3 classes, beta 0.1: fast -n 3 -H 0.1) and the result gains 'TWC_seg' (uint8: 0
    outside, 1..3 by ascending water content) and 'TWC_prob' [3,nx,ny,nz] (the class posteriors); nothing else changes.  ValueError before
    any device work for a value other than 'no' / 'yes' / 'pve', without bias_correct='yes' and with distributed=True; on the devices=[...]
    path it runs on devices[0].  segment='pve': everything 'yes' gives, then partial_volume_filter on the map, the labels and the posteriors
    (beta_pv 0.3: fast's -R default) adds 'TWC_pve' [3,nx,ny,nz] (the tissue fractions, what fast writes as _pve_k: a white-matter mask
    for MWF statistics is TWC_pve[k] > 0.9, not a hard label), 'TWC_pveseg' and 'TWC_mixeltype' (uint8).  Parity with fast itself is
    unpinned.  segment='no' (default) changes no output and no launch.
    tissue_stats='yes' (an extension: the reference's TO DO (2) of motor:376 and its mean-spectrum numbers of motor:377-403, per tissue;
    needs segment='yes' or 'pve'): after the segmentation the result gains 'tissue_stats', the dict of label_stats_filter on the tissue labels
    -- TWC_seg with segment='yes'; with 'pve' label k + 1 where TWC_pve[k] > pve_threshold (in [0.5, 1), so that no voxel has two labels)
    -- plus 'all', the same statistics of the whole segmented domain (TWC_seg > 0), and 'mean_signal_fsol' [L + 1, n_t2] with
    'mean_signal_<map>' [L + 1]: the X2 fit (penalty I, factor 1.01) of every label's mean signal on its mean kernel, the last row the
    whole domain (recon_met2_rois on the prepared data and the run's FA_index).  ValueError before any device work for another value,
    without the segmentation, for a threshold outside [0.5, 1) and with distributed=True; on the devices=[...] path it runs on devices[0].
    tissue_stats='no' (default) changes no output and no launch.
    brain_mask='yes' (step 3 of the reference's example script, which runs FSL's fslmaths -Tmean and bet -m -f 0.4 there): `mask` is None
    and the mask is made by brain_mask_filter from the echo mean of the raw volume -- of the unrung one with degibbs='yes' -- with
    voxel_size=(dx, dy, dz) in mm, after degibbs and before the mask multiply; the result carries it as 'mask' (uint8).  Needs data
    [nx,ny,nz,nt] and voxel_size; ValueError otherwise, with a mask given, with prepared=True and with distributed=True, before any device
    work; on the devices=[...] path it runs on devices[0].  Parity with bet itself is unpinned (no self-intersection retry).
    brain_mask='no' (default) changes nothing.
    FA_smooth='yes' (the CLI default, motor:337-343): the flip angles are estimated on the Gaussian-smoothed volume
    (sigma = 2 voxels, every echo), the spectra on the unsmoothed one; needs a 3-D volume.
    C- and Fortran-ordered volumes (nibabel's) are both read in place.
    distributed=True (under torch.distributed.run, one rank per GPU): every rank holds the volume, runs the FA step and the
    fit on its own interleaved 4096-voxel blocks of the voxel list and the outputs meet on rank 0 in ONE gather
    (dist.fit_sharded); ranks other than 0 return None.
    devices=[d0, d1, ...]: ONE process drives several GPUs through the C ABI's host entry (met2_fit_host: one plan and one host thread per
    device inside the call, blocks of voxels dealt round-robin, outputs copied by every device into the same host arrays -- no
    torch.distributed); the whole-volume filters (TV / NESMA / MPPCA / FA smoothing) run on devices[0] first.  Same outputs bit for bit.
    bootstrap=dict(n_rep=100, seed=0): per-voxel bootstrap uncertainty of the metrics (Met2Plan.fit_bootstrap; an extension with no
    counterpart in the reference), on one device (devices[0]) with the pipeline's prepared data and FA indices; voxel_id is the voxel's flat
    index in the volume's C order, whatever the memory order.  Adds '<Q>_bootstrap' [vol..., 5] for Q in BOOT_QUANTITIES (BOOT_STATS along
    the last axis), 'sigma' and 'rep_status'; the ten outputs are those of the same run without it.  Two more keys (Met2Plan.fit_bootstrap's
    fa and want_spectrum): fa='fixed' (default) | 'brute-force' | 'spline' -- other than 'fixed' it must be the run's FA_method, every
    replicate then gets its own flip angle and 'FA_bootstrap' [vol..., 5] (degrees) is added; it does not go with FA_smooth='yes' (see
    _bootstrap_check).  spectrum=True adds 'fsol_bootstrap' [vol..., n_t2, 5], the per-bin band of the T2 spectrum.
    rician='iterative' | 'direct' (an extension: the Rician noise floor of the echo magnitudes, which the fit otherwise reads as a long-T2 pool;
    one device, through a plan).  'iterative': after the FA step the fit is Met2Plan.fit_rician with rician_iters passes (default 3) at the
    noise level rician_sigma (a number or a volume) or, without one, at the residual estimate of Met2Plan.noise_sigma; adds 'sigma', 'SNR'
    (first echo of the model signal over sigma, 0 where sigma = 0) and 'rician_flag'; 'Est_Signal' is then the noise-free signal estimate.
    'direct': the prepared volume goes through rician.invert before the FA step and the fit, which run once -- the one-shot correction of
    denoised magnitudes; it needs a sigma map, rician_sigma or the one denoise='MPPCA' leaves, and adds 'sigma' and 'data_rician' (the
    corrected volume).  It treats a denoised magnitude as the Rician mean, which it only approximates.  sigma is never re-estimated after a
    correction, and the residual estimate is biased low where many echoes sit in the floor; neither mode makes the fit a maximum-likelihood
    Rician fit.  ValueError before any device work for another value, for 'direct' without a sigma source, and with devices=[...],
    distributed=True or bootstrap=...  rician='no' (default) changes no output and no launch.
    slice_profile=<the dict of epg.slice_profile> (an extension, for 2-D multi-slice multi-echo spin echo: the flip angles vary across the
    slice and the decay is the integral of the echo trains over the profile, Lebel & Wilman 2010): every dictionary of the run -- the run's
    own plan, the coarse plan of FA_method='spline', and with them what tissue_stats and bootstrap=dict(fa='fixed') reuse -- is built by
    Met2Plan.build_dictionary_epg(slice_profile=...); one device, through a plan.  'FA' is then the nominal refocusing angle at the slice
    centre, on the unchanged 90..180 degree grid.  A caller's own plan= keeps the dictionary it has: ValueError if slice_profile is given
    too and differs from plan.slice_profile.  ValueError before any device work with devices=[...], distributed=True and a bootstrap whose
    fa is not 'fixed'.  slice_profile=None (default) changes no output and no launch.
    Returns a dict with the driver's ten outputs."""
    boot = _bootstrap_args(bootstrap)
    ric = _rician_check(rician, rician_sigma, rician_iters, denoise, prepared, devices, distributed, bootstrap)
    slice_profile = _slice_profile_check(slice_profile, plan, devices, distributed, boot)
    if boot is not None and distributed:
        raise ValueError("bootstrap runs on one device and does not go with distributed=True")
    _bootstrap_check(boot, FA_method, FA_smooth)
    if FA_method not in ("brute-force", "spline"):
        raise ValueError("FA_method must be 'spline' or 'brute-force'")
    if denoise not in ("None", None, "none", "NESMA", "TV", "MPPCA"):
        raise ValueError("denoise must be 'None', 'NESMA', 'TV' or 'MPPCA'")
    seg = _segment_check(segment, bias_correct, distributed)
    tstats = _tissue_stats_check(tissue_stats, segment, distributed, pve_threshold)
    bet = _brain_mask_check(brain_mask, mask, data, voxel_size, prepared, distributed)
    first_dev = devices[0] if devices else plan.device.index or 0 if plan is not None else device
    data = _degibbs_first(data, degibbs, prepared, first_dev)
    data = np.asarray(data, dtype=np.float64)
    vol_shape = data.shape[:-1]
    if bet:
        made = brain_mask_filter(np.ascontiguousarray(data), voxel_size, device=first_dev)
        res = recon_met2_arrays(data, made, TE_array, TR, reg_method, reg_matrix, FA_method, myelin_T2, fa_index, device, plan, denoise, False,
                                FA_smooth, False, return_prepared, devices, bootstrap, "no", bias_correct, voxel_size, "no", segment, tissue_stats,
                                pve_threshold, rician=rician, rician_sigma=rician_sigma, rician_iters=rician_iters, slice_profile=slice_profile)
        res["mask"] = made
        return res
    bias = _bias_check(bias_correct, vol_shape, voxel_size, distributed)
    nt = data.shape[-1]
    mask = np.asarray(mask).reshape(vol_shape)
    if devices is None and plan is None and not distributed and data.ndim >= 2 and not ric and slice_profile is None:
        devices = [device]                                       # the default: one device, through the C ABI's host entry (met2_fit_host: the block
                                                                 # pipeline inside the library; the torch pipeline of rounds 3-4 is retired to tests/tools)
    if devices is not None:
        if plan is not None or distributed:
            raise ValueError("devices=[...] builds its own plans and does not go with distributed=True")
        res = _recon_multi_device(data, mask, TE_array, TR, reg_method, reg_matrix, FA_method, myelin_T2, fa_index, list(devices), prepared,
                                  denoise, FA_smooth, return_prepared or boot is not None or tstats)
        dd = None
        if boot is not None or tstats:
            dd = res["data_prepared"] if return_prepared else res.pop("data_prepared")
            if not return_prepared:
                res.pop("MPPCA_sigma", None)
            TE_array = np.asarray(TE_array, dtype=np.float64)

        def device_plan():                                       # a plan with the run's dictionary on devices[0]: the host entry closed its own
            p = Met2Plan(nt, res["T2s"].shape[0], 91 * 3 if FA_method == "spline" else 91, device=devices[0], myelin_T2=myelin_T2)
            p.build_dictionary_epg(res["T2s"], 1000.0 * np.ones_like(res["T2s"]), float(TE_array[1] - TE_array[0]),
                                   np.linspace(90.0, 180.0, p.n_fa), TR)
            return p

        if boot is not None:
            plan = device_plan()
            try:
                plan.set_penalty("InvT2" if reg_method == "T2SPARC" else reg_matrix, res["T2s"])
                _bootstrap_into(res, plan, reg_method, torch.as_tensor(dd).to(plan.device), res["FA_index"], mask > 0, boot,
                                (res["T2s"], 1000.0 * np.ones_like(res["T2s"]), float(TE_array[1] - TE_array[0]), TR))
            finally:
                plan.close()
        if bias:
            _bias_last(res, mask, voxel_size, devices[0])
        if seg:
            _segment_last(res, mask, voxel_size, devices[0], segment)
        if tstats:
            plan = device_plan()
            try:
                _tissue_stats_last(res, dd, plan, segment, pve_threshold, myelin_T2)
            finally:
                plan.close()
        return res
    dev = plan.device if plan is not None else torch.device("cuda", device)
    # a caller's own plan, a distributed run, or a bare voxel list: the volume on the device in one piece
    extra = {}
    dd, mk = _prepare_volume(data, mask, dev, prepared, denoise, extra)
    mm = (mk > 0)
    sigma_vol = _rician_sigma(ric, rician_sigma, extra, vol_shape, dev)
    dd_prepared = dd
    if ric == "direct":
        from . import rician as _rician
        dd = _rician.invert(dd, sigma_vol, mm)
    dd_fa = dd
    if FA_smooth == "yes" and fa_index is None:
        if len(vol_shape) != 3:
            raise ValueError("FA_smooth='yes' needs data [nx,ny,nz,nt]")
        dd_fa = gaussian_smooth(dd, 2.0)
    TE_array = np.asarray(TE_array, dtype=np.float64)
    tau = float(TE_array[1] - TE_array[0])
    Npc = 96 if reg_method == "T2SPARC" else 60
    T2s = np.logspace(math.log10(10.0), math.log10(2000.0), num=Npc, endpoint=True, base=10.0)
    T1s = 1000.0 * np.ones_like(T2s)
    alpha_values = np.linspace(90.0, 180.0, 91 * 3 if FA_method == "spline" else 91)      # motor:231-244
    own = plan is None
    if own:
        plan = Met2Plan(nt, Npc, alpha_values.shape[0], device=device, myelin_T2=myelin_T2)
        plan.build_dictionary_epg(T2s, T1s, tau, alpha_values, TR, slice_profile=slice_profile)
        plan.set_penalty("InvT2" if reg_method == "T2SPARC" else reg_matrix, T2s)   # run_real_data_script.py:91-93
    try:
        if distributed:
            return _recon_sharded(plan, dd, dd_fa, mm, reg_method, FA_method, fa_index, T2s, T1s, tau, TR, alpha_values, device, vol_shape)
        fa_vol = _estimate_fa(plan, dd_fa, mm, FA_method, fa_index, T2s, T1s, tau, TR, alpha_values, device)
        if ric == "iterative":
            out = plan.fit_rician(reg_method, dd, n_iter=int(rician_iters), sigma=sigma_vol, fa_index=fa_vol, mask=mm)
        else:
            out = plan.fit(reg_method, dd, fa_index=fa_vol, mask=mm)
        tot_fa = dd_fa.sum(dim=-1)
        res = {"fsol_4D": out["fsol"].cpu().numpy(), "Est_Signal": out["sig"].cpu().numpy(), "reg_param": out["reg"].cpu().numpy(),
               "FA_index": fa_vol.cpu().numpy()}
        if ric == "iterative":
            sg = out["sigma"]
            res["sigma"] = sg.cpu().numpy()
            res["SNR"] = torch.where(sg > 0, out["sig"][..., 0] / torch.where(sg > 0, sg, torch.ones_like(sg)), torch.zeros_like(sg)).cpu().numpy()
            res["rician_flag"] = out["rician_flag"].cpu().numpy()
        elif ric == "direct":
            res["sigma"] = sigma_vol.cpu().numpy()
            res["data_rician"] = dd.cpu().numpy()
        fitted_fa = (mm & (tot_fa > 0)).cpu().numpy()      # gate of the FA step (fa_estimation.py:45)
        res["FA"] = np.where(fitted_fa, alpha_values[res["FA_index"].astype(int)], 0.0)
        maps = out["maps"].cpu().numpy()
        for i, name in enumerate(MAP_NAMES):
            res[name] = maps[i]
        res["T2s"] = T2s
        if return_prepared:
            res["data_prepared"] = dd_prepared.cpu().numpy()
            for name, t in extra.items():
                res[name] = t.cpu().numpy()
        if boot is not None:
            _bootstrap_into(res, plan, reg_method, dd, fa_vol, mm, boot, (T2s, T1s, tau, TR))
        if bias:
            _bias_last(res, mask, voxel_size, dev.index or 0)
        if seg:
            _segment_last(res, mask, voxel_size, dev.index or 0, segment)
        if tstats:
            _tissue_stats_last(res, dd, plan, segment, pve_threshold, myelin_T2)
        return res
    finally:
        if own:
            plan.close()


def _rician_check(rician, rician_sigma, rician_iters, denoise, prepared, devices, distributed, bootstrap):
    """rician of recon_met2_arrays -> None, 'iterative' or 'direct'; what it cannot be combined with is raised before any device work."""
    if rician not in ("no", "iterative", "direct"):
        raise ValueError("rician must be 'no', 'iterative' or 'direct'")
    if rician == "no":
        return None
    if devices is not None:
        raise ValueError("rician='%s' runs through one plan and does not go with devices=[...]" % rician)
    if distributed:
        raise ValueError("rician='%s' does not go with distributed=True" % rician)
    if bootstrap is not None:
        raise ValueError("rician='%s' does not go with bootstrap=...: the replicates would be drawn around a corrected fit" % rician)
    if not 0 <= int(rician_iters) <= 16:
        raise ValueError("rician_iters must lie in [0, 16]")
    if rician_sigma is not None and np.any(np.asarray(rician_sigma, dtype=np.float64) < 0):
        raise ValueError("rician_sigma must be >= 0")
    if rician == "direct" and rician_sigma is None and (denoise != "MPPCA" or prepared):
        raise ValueError("rician='direct' needs a sigma map: rician_sigma, or denoise='MPPCA' (not prepared=True), whose map it takes")
    return rician


def _slice_profile_check(slice_profile, plan, devices, distributed, boot):
    """slice_profile of recon_met2_arrays -> None or the validated profile dict; what it cannot be combined with is raised before any device work."""
    if slice_profile is None:
        return None
    from . import epg as _epg
    prof = _epg.check_profile(slice_profile["r_exc"], slice_profile["r_ref"], slice_profile["w"])        # the weights as given
    if devices is not None:
        raise ValueError("slice_profile runs through one plan and does not go with devices=[...]")
    if distributed:
        raise ValueError("slice_profile does not go with distributed=True")
    if boot is not None and boot["fa"] != "fixed":
        raise ValueError("slice_profile goes with bootstrap fa='fixed' only, not fa=%r" % (boot["fa"],))
    if plan is not None and not _epg.same_profile(prof, plan.slice_profile):
        raise ValueError("slice_profile differs from the one the caller's plan was built with (plan.slice_profile)")
    return prof


def _rician_sigma(ric, rician_sigma, extra, vol_shape, dev):
    """The noise level of the run as a device volume shaped like the voxels: rician_sigma (a number or a volume), MP-PCA's map for 'direct'
    without one, None for 'iterative' without one (the fit then estimates it)."""
    if not ric:
        return None
    if rician_sigma is None:
        return extra["MPPCA_sigma"].reshape(vol_shape) if ric == "direct" else None
    sg = np.asarray(rician_sigma, dtype=np.float64)
    sg = np.full(vol_shape, float(sg)) if sg.ndim == 0 else sg.reshape(vol_shape)
    return torch.as_tensor(sg, dtype=torch.float64, device=dev)


def _bootstrap_args(bootstrap):
    if bootstrap is None:
        return None
    extra = set(bootstrap) - {"n_rep", "seed", "fa", "spectrum"}
    if extra:
        raise ValueError("bootstrap takes n_rep, seed, fa and spectrum, not %s" % sorted(extra))
    fa = bootstrap.get("fa", "fixed")
    if fa not in ("fixed", "brute-force", "spline"):
        raise ValueError("bootstrap fa must be 'fixed', 'brute-force' or 'spline', got %r" % (fa,))
    return {"n_rep": int(bootstrap.get("n_rep", 100)), "seed": int(bootstrap.get("seed", 0)), "fa": fa, "spectrum": bool(bootstrap.get("spectrum", False))}


def _bootstrap_check(boot, FA_method, FA_smooth):
    """What a bootstrap with per-replicate flip angles cannot be combined with; raised before any device work."""
    if boot is None or boot["fa"] == "fixed":
        return
    if FA_smooth == "yes":
        raise ValueError("bootstrap fa=%r does not go with FA_smooth='yes': the point fit's flip angle would come from the Gaussian-smoothed "
                         "volume and every replicate's from its own unsmoothed row (replicates of different voxels are independent draws, "
                         "there is nothing to smooth over), so the spread would measure the difference between two estimators; "
                         "use FA_smooth='no' or fa='fixed'" % (boot["fa"],))
    if boot["fa"] != FA_method:
        raise ValueError("bootstrap fa=%r must be the run's FA_method (%r): the replicates are re-estimated the way the point fit was"
                         % (boot["fa"], FA_method))


def _bootstrap_into(res, plan, reg_method, dd, fa_vol, mask, boot, epg=None):
    """recon_met2_arrays(bootstrap=...): Met2Plan.fit_bootstrap on the prepared volume dd [vol..., nt] (a device tensor) with the run's FA
    indices and mask; the statistics go into res beside the ten outputs, which stay as the run made them.  epg = (T2s, T1s, tau, TR): what
    the coarse plan of fa='spline' is built from."""
    from .plan import BOOT_QUANTITIES
    vol = tuple(dd.shape[:-1])
    vid = np.arange(int(np.prod(vol)), dtype=np.int64).reshape(vol)       # the C-order flat index: independent of the memory order
    plan_lr = None
    try:
        if boot["fa"] == "spline":
            alpha_lr = np.linspace(90.0, 180.0, 15)                          # motor:237
            plan_lr = Met2Plan(plan.n_te, plan.n_t2, 15, device=plan.device.index or 0)
            plan_lr.build_dictionary_epg(epg[0], epg[1], epg[2], alpha_lr, epg[3], slice_profile=plan.slice_profile)
            plan.attach_fa_spline(plan_lr, alpha_lr)
        out = plan.fit_bootstrap(reg_method, dd, n_rep=boot["n_rep"], seed=boot["seed"], fa_index=fa_vol, mask=mask, voxel_id=vid,
                                 want_sig=True, want_status=False, fa=boot["fa"], want_spectrum=boot["spectrum"])
    finally:
        if plan_lr is not None:
            plan.attach_fa_spline(None, None)
            plan_lr.close()
    stats = out["stats"].cpu().numpy()                                    # [7, 5, vol...]
    for i, q in enumerate(BOOT_QUANTITIES):
        res[q + "_bootstrap"] = np.moveaxis(stats[i], 0, -1)
    res["sigma"] = out["sigma"].cpu().numpy()
    res["rep_status"] = out["rep_status"].cpu().numpy()
    if boot["fa"] != "fixed":
        res["FA_bootstrap"] = np.where((res["rep_status"] != 0)[..., None], np.moveaxis(out["fa_stats_deg"], 0, -1), 0.0)   # degrees; 0 where not fitted, like 'FA'
    if boot["spectrum"]:
        res["fsol_bootstrap"] = np.moveaxis(out["spec_stats"].cpu().numpy(), 0, -1)       # [vol..., n_t2, 5]


PIPELINE_CHUNK = 262144       # voxels per DMA block the driver asks met2_fit_host for (262 144: the library's own default; a test sets others)


def _match_layout(t, order):
    """the volume tensor t [..., nt] laid out in memory as `order` says ('C', or 'F': the reversed axes contiguous)"""
    rev = list(reversed(range(t.dim())))
    if order == "C":
        return t.contiguous()
    return t if t.permute(*rev).is_contiguous() else t.permute(*rev).contiguous().permute(*rev)


def _recon_multi_device(data, mask, TE_array, TR, reg_method, reg_matrix, FA_method, myelin_T2, fa_index, devices, prepared, denoise, FA_smooth,
                        return_prepared=False):
    """recon_met2_arrays(devices=[...]): one process, one plan per listed device, driven by met2_fit_host (host.fit_host).  The driver's
    preparation runs on the host for plain runs and, with a whole-volume filter (motor:293-343), on devices[0]; steps 2-4 then go through
    the host entry, which deals blocks of the voxel list to the devices."""
    from . import host as mhost
    if not devices:
        raise ValueError("devices is empty")
    vol_shape, nt = data.shape[:-1], data.shape[-1]
    filtered = denoise not in ("None", None, "none") or (FA_smooth == "yes" and fa_index is None)
    fa_vol = None
    mvals = None

    def to_pinned(t):                                            # device tensor -> numpy view of a pinned copy in the same memory order
        h = torch.empty_strided(tuple(t.shape), tuple(t.stride()), dtype=t.dtype, pin_memory=True)
        h.copy_(t)
        return h.numpy()

    keep_alive = None
    extra = {}                                                   # what a filter leaves beside the volume (MPPCA: its noise map)
    if filtered:
        dev0 = torch.device("cuda", devices[0])
        dd, _ = _prepare_volume(data, mask, dev0, prepared, denoise, extra)
        one_device = len(set(devices)) == 1                      # the filtered volume stays where it is: met2_fit_host copies its blocks device to device
        place = (lambda t: t) if one_device else to_pinned
        if FA_smooth == "yes" and fa_index is None:
            if len(vol_shape) != 3:
                raise ValueError("FA_smooth='yes' needs data [nx,ny,nz,nt]")
            fa_vol = place(_match_layout(gaussian_smooth(dd, 2.0), "C" if dd.is_contiguous() else "F"))     # laid out like the volume itself
        if not (dd.is_contiguous() or dd.permute(*reversed(range(dd.dim()))).is_contiguous()):
            dd = dd.contiguous()
        vol = place(dd)                                          # keeps the memory order the volume came in
        keep_alive = dd
        torch.cuda.current_stream(dev0).synchronize()            # the library's streams do not wait for torch's
    else:
        vol = data                                               # prepared inside the library, per block, on the device (mask_values)
        if not prepared:
            mvals = np.asarray(mask, dtype=np.float64)
    if not torch.is_tensor(vol) and not (vol.flags.c_contiguous or vol.flags.f_contiguous):
        vol = np.ascontiguousarray(vol)
    order = "C" if (vol.is_contiguous() if torch.is_tensor(vol) else vol.flags.c_contiguous) else "F"
    TE_array = np.asarray(TE_array, dtype=np.float64)
    tau = float(TE_array[1] - TE_array[0])
    Npc = 96 if reg_method == "T2SPARC" else 60
    T2s = np.logspace(math.log10(10.0), math.log10(2000.0), num=Npc, endpoint=True, base=10.0)
    T1s = 1000.0 * np.ones_like(T2s)
    alpha_values = np.linspace(90.0, 180.0, 91 * 3 if FA_method == "spline" else 91)      # motor:231-244
    plans, coarse = [], []
    try:
        for d in devices:
            p = Met2Plan(nt, Npc, alpha_values.shape[0], device=d, myelin_T2=myelin_T2)
            plans.append(p)
            p.build_dictionary_epg(T2s, T1s, tau, alpha_values, TR)
            p.set_penalty("InvT2" if reg_method == "T2SPARC" else reg_matrix, T2s)      # run_real_data_script.py:91-93
        mode = False
        if fa_index is None:
            mode = "brute-force"
            if FA_method == "spline":
                alpha_lr = np.linspace(90.0, 180.0, 15)                                    # motor:237
                for d in devices:
                    q = Met2Plan(nt, Npc, 15, device=d)
                    coarse.append(q)
                    q.build_dictionary_epg(T2s, T1s, tau, alpha_lr, TR)
                mhost.attach_fa_spline(plans, coarse, alpha_lr, alpha_values)
                mode = "spline"
        nvox = int(np.prod(vol_shape))
        pin = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, pin_memory=True).numpy()     # torch's caching host allocator: reused across calls
        bufs = {"fsol": pin((nvox, Npc)), "sig": pin((nvox, nt)), "reg": pin((nvox,)), "maps": pin((6, nvox)), "status": pin((nvox,), torch.int32),
                "fa_index": pin((nvox,)), "fa_gate": pin((nvox,))}
        out = mhost.fit_host(plans, reg_method, vol, fa_index=fa_index, mask=mask > 0, estimate_fa=mode, fa_data=fa_vol, mask_values=mvals, want_gate=True,
                             chunk=PIPELINE_CHUNK if PIPELINE_CHUNK != 262144 else 0, out=bufs)     # (0: the library's block size; a test that sets PIPELINE_CHUNK gets its chunks)
    finally:
        for p in plans + coarse:
            p.close()
    rv = tuple(reversed(vol_shape))
    nd = len(vol_shape)

    def unfold(a, lead=0):                                        # flat in the volume's memory order -> the volume's logical shape
        if order == "C":
            return a.reshape(a.shape[:lead] + vol_shape + a.shape[lead + 1:])
        u = a.reshape(a.shape[:lead] + rv + a.shape[lead + 1:])
        return u.transpose(list(range(lead)) + [lead + nd - 1 - i for i in range(nd)] + list(range(lead + nd, u.ndim)))

    res = {"fsol_4D": unfold(out["fsol"]), "Est_Signal": unfold(out["sig"]), "reg_param": unfold(out["reg"]), "FA_index": unfold(out["fa_index"])}
    fitted_fa = unfold(out["fa_gate"]) > 0                        # gate of the FA step (fa_estimation.py:45), formed on the device per block
    res["FA"] = np.where(fitted_fa, alpha_values[res["FA_index"].astype(int)], 0.0)
    maps = unfold(out["maps"], lead=1)
    for i, name in enumerate(MAP_NAMES):
        res[name] = maps[i]
    res["T2s"] = T2s
    if return_prepared:
        if mvals is not None:                                     # (plain runs prepare per block inside the library)
            vol = np.maximum(vol * mvals[..., None], 0.0)
        res["data_prepared"] = vol.cpu().numpy() if torch.is_tensor(vol) else vol
        for name, t in extra.items():
            res[name] = t.cpu().numpy()
    return res


def _recon_sharded(plan, dd, dd_fa, mm, reg_method, FA_method, fa_index, T2s, T1s, tau, TR, alpha_values, device, vol_shape):
    """The multi-GPU leg of recon_met2_arrays: this rank's interleaved blocks through FA estimation + fit, one gather."""
    from . import dist as mdist
    from .plan import unflatten_back
    nt, Npc = plan.n_te, plan.n_t2
    flat = unflatten_back(dd, "C")                          # [nvox, nt] views in C voxel order (rows are gathered per shard)
    flat_fa = unflatten_back(dd_fa, "C")
    mflat = mm.reshape(-1)
    faflat = None if fa_index is None else torch.as_tensor(np.asarray(fa_index, dtype=np.float64).reshape(-1), device=dd.device)

    def fit_fn(idx):
        d = flat[idx].contiguous()
        dfa = d if dd_fa is dd else flat_fa[idx].contiguous()
        m = mflat[idx]
        fa = _estimate_fa(plan, dfa, m, FA_method, None if faflat is None else faflat[idx].cpu().numpy(), T2s, T1s, tau, TR, alpha_values, device)
        out = plan.fit(reg_method, d, fa_index=fa, mask=m)
        out["fa"] = fa
        out["fa_gate"] = (m & (dfa.sum(dim=1) > 0)).to(torch.float64)
        return out

    nvox = flat.shape[0]
    _, full = mdist.fit_sharded(fit_fn, nvox, gather=("fsol", "sig", "reg", "maps", "fa", "fa_gate"))
    if full is None:
        return None
    res = {"fsol_4D": full["fsol"].cpu().numpy().reshape(vol_shape + (Npc,)), "Est_Signal": full["sig"].cpu().numpy().reshape(vol_shape + (nt,)),
           "reg_param": full["reg"].cpu().numpy().reshape(vol_shape), "FA_index": full["fa"].cpu().numpy().reshape(vol_shape)}
    res["FA"] = np.where(full["fa_gate"].cpu().numpy().reshape(vol_shape) > 0, alpha_values[res["FA_index"].astype(int)], 0.0)
    maps = full["maps"].cpu().numpy()
    for i, name in enumerate(MAP_NAMES):
        res[name] = maps[i].reshape(vol_shape)
    res["T2s"] = T2s
    return res


def motor_recon_met2(TE_array, path_to_data, path_to_mask, path_to_save_data, TR, reg_method, reg_matrix, denoise, FA_method,
                     FA_smooth, myelin_T2, num_cores=-1, device=0, devices=None, bootstrap=None, degibbs="no", bias_correct="no",
                     brain_mask="no", segment="no", tissue_stats="no", pve_threshold=0.9, rician="no", rician_sigma=None, rician_iters=3,
                     slice_profile=None):
    """Drop-in for motor_recon_met2 (motor:165-506) with the reference's on-disk contract: NIfTI in
    (data [nx,ny,nz,nt], mask [nx,ny,nz]), ten NIfTI volumes out (MWF, IEWF, FWF, T2_M, T2_IE, TWC, FA, fsol_4D,
    Est_Signal, reg_param .nii.gz at path_to_save_data, motor:475-503).  `num_cores` is accepted and ignored (one
    process drives the GPU; devices=[0, 1, ...]: that one process drives all the listed GPUs through met2_fit_host).  denoise: 'None',
    'NESMA' (motor:305-333), 'TV' (motor:293-304) or 'MPPCA' (an extension: mppca_filter; Data_denoised.nii.gz as for TV, and the noise
    map MPPCA_sigma.nii.gz).  degibbs='yes' or '3d' (see recon_met2_arrays): the raw volume is unrung first (gibbs_filter) and written as
    Data_degibbs.nii.gz.  bias_correct='yes' (see recon_met2_arrays): TWC.nii.gz is the bias-corrected map and TWC_bias.nii.gz the
    estimated field, as the example script leaves them; the voxel size is the data header's pixdim[1:4] (absolute values, 0 read as 1).
    segment='yes' (see recon_met2_arrays; needs bias_correct='yes'): TWC_seg.nii.gz (0 outside, 1..3 by ascending water content) and
    TWC_prob_0.nii.gz .. TWC_prob_2.nii.gz (the class posteriors), named after fast's _seg and _prob_k.  segment='pve' also writes
    TWC_pve_0.nii.gz .. TWC_pve_2.nii.gz (the tissue fractions), TWC_pveseg.nii.gz and TWC_mixeltype.nii.gz, after fast's _pve_k, _pveseg
    and _mixeltype.  Parity with fast itself is unpinned.
    brain_mask='yes' (see recon_met2_arrays): path_to_mask is None, the mask is made by brain_mask_filter from the echo mean (of the unrung
    volume with degibbs='yes') with the header's voxel size, and Data_avg.nii.gz (the echo mean) and mask.nii.gz are written beside the
    outputs, as the example script's step 3 leaves Data_avg and Data_mask.
    tissue_stats='yes' (see recon_met2_arrays; needs segment='yes' or 'pve'): table_tissue_stats.csv, one row per (label, quantity) with the
    columns label, quantity, n, mean, std and the quantiles 0.025, 0.25, 0.5, 0.75, 0.975 (the labels: the tissues 1..3, then 'all', the
    whole segmented domain), and table_tissue_spectra.csv: the T2 grid, then per label the normalised mean spectrum of its voxels and
    the spectrum fitted to its mean signal -- the numbers of the reference's mean-spectrum figure (motor:377-403), per tissue; written
    with np.savetxt like the ROI driver's tables (tissue_stats_tables makes them).
    Not reproduced: the mean-spectrum PNG of motor:404-424.
    bootstrap=dict(n_rep=..., seed=...) (an extension, see recon_met2_arrays) also writes <Q>_bootstrap.nii.gz [nx,ny,nz,5] for Q in
    BOOT_QUANTITIES (BOOT_STATS along the last axis) and sigma.nii.gz; with fa='brute-force' / 'spline' also FA_bootstrap.nii.gz [nx,ny,nz,5]
    (degrees), with spectrum=True also fsol_bootstrap_{mean,std,q025,q500,q975}.nii.gz [nx,ny,nz,n_t2] each.
    rician='iterative' | 'direct' with rician_sigma and rician_iters (an extension, see recon_met2_arrays; not with devices=[...] or bootstrap):
    also writes sigma.nii.gz; 'iterative' SNR.nii.gz and rician_flag.nii.gz, 'direct' Data_rician.nii.gz (the corrected volume).
    slice_profile=<the dict of epg.slice_profile> (an extension, see recon_met2_arrays; not with devices=[...] or a bootstrap whose fa is not
    'fixed'): the dictionaries are built over the slice profile; FA.nii.gz is then the nominal refocusing angle at the slice centre."""
    from . import nifti
    img = nifti.load(path_to_data)
    data = img.get_fdata().astype(np.float64, copy=False)           # Fortran-ordered, like nibabel's: read in place by the solver
    if brain_mask not in ("no", "yes"):
        raise ValueError("brain_mask must be 'no' or 'yes'")
    if brain_mask == "yes" and path_to_mask is not None:
        raise ValueError("brain_mask='yes' makes the mask itself and does not go with path_to_mask")
    _segment_check(segment, bias_correct, False)
    _tissue_stats_check(tissue_stats, segment, False, pve_threshold)
    if _rician_check(rician, rician_sigma, rician_iters, denoise, False, devices, False, bootstrap):
        rician_kw = {"rician": rician, "rician_sigma": rician_sigma, "rician_iters": rician_iters}
    else:
        rician_kw = {}
    profile_kw = {}
    if _slice_profile_check(slice_profile, None, devices, False, _bootstrap_args(bootstrap)) is not None:
        profile_kw = {"slice_profile": slice_profile}
    mask = None if brain_mask == "yes" else nifti.load(path_to_mask).get_fdata().astype(np.int64)
    if data.ndim != 4 or (mask is not None and mask.shape != data.shape[:3]):
        raise ValueError("data must be 4-D and mask must match its first three dimensions")
    bias_kw = {}
    if bias_correct != "no" or brain_mask == "yes":
        pixdim = img.header.get("pixdim", (1.0,) * 8)
        voxel_size = tuple(abs(float(p)) or 1.0 for p in pixdim[1:4])
    if bias_correct != "no":
        bias_kw = {"bias_correct": bias_correct, "voxel_size": voxel_size}
    if segment != "no":
        bias_kw["segment"] = segment
    if tissue_stats != "no":
        bias_kw["tissue_stats"] = tissue_stats
        bias_kw["pve_threshold"] = pve_threshold
    if degibbs != "no":
        data = _degibbs_first(data, degibbs, False, devices[0] if devices else device)
        nifti.save(nifti.NiftiImage(data, img.affine), path_to_save_data + "Data_degibbs.nii.gz")
    if brain_mask == "yes":
        from . import bet
        avg = bet.bet_mean(np.ascontiguousarray(data), device=devices[0] if devices else device)
        mask = brain_mask_filter(avg, voxel_size, device=devices[0] if devices else device)
        nifti.save(nifti.NiftiImage(avg, img.affine), path_to_save_data + "Data_avg.nii.gz")
        nifti.save(nifti.NiftiImage(mask, img.affine), path_to_save_data + "mask.nii.gz")
    res = recon_met2_arrays(data, mask, TE_array, TR, reg_method, reg_matrix, FA_method, myelin_T2, device=device, denoise=denoise,
                            FA_smooth=FA_smooth, return_prepared=(denoise in ("TV", "MPPCA")), devices=devices, bootstrap=bootstrap,
                            **bias_kw, **rician_kw, **profile_kw)
    if brain_mask == "yes":
        res["mask"] = mask
    if rician_kw:
        nifti.save(nifti.NiftiImage(res["sigma"], img.affine), path_to_save_data + "sigma.nii.gz")
        if rician == "iterative":
            nifti.save(nifti.NiftiImage(res["SNR"], img.affine), path_to_save_data + "SNR.nii.gz")
            nifti.save(nifti.NiftiImage(res["rician_flag"], img.affine), path_to_save_data + "rician_flag.nii.gz")
        else:
            nifti.save(nifti.NiftiImage(res.pop("data_rician"), img.affine), path_to_save_data + "Data_rician.nii.gz")
    if bias_kw:
        nifti.save(nifti.NiftiImage(res["TWC_bias"], img.affine), path_to_save_data + "TWC_bias.nii.gz")
    if "TWC_seg" in res:
        nifti.save(nifti.NiftiImage(res["TWC_seg"], img.affine), path_to_save_data + "TWC_seg.nii.gz")
        for k in range(res["TWC_prob"].shape[0]):
            nifti.save(nifti.NiftiImage(np.ascontiguousarray(res["TWC_prob"][k]), img.affine), path_to_save_data + "TWC_prob_%d.nii.gz" % k)
    if "TWC_pve" in res:
        for k in range(res["TWC_pve"].shape[0]):
            nifti.save(nifti.NiftiImage(np.ascontiguousarray(res["TWC_pve"][k]), img.affine), path_to_save_data + "TWC_pve_%d.nii.gz" % k)
        nifti.save(nifti.NiftiImage(res["TWC_pveseg"], img.affine), path_to_save_data + "TWC_pveseg.nii.gz")
        nifti.save(nifti.NiftiImage(res["TWC_mixeltype"], img.affine), path_to_save_data + "TWC_mixeltype.nii.gz")
    if "tissue_stats" in res:
        table, spectra = tissue_stats_tables(res["tissue_stats"])
        np.savetxt(path_to_save_data + "table_tissue_stats.csv", table, delimiter=",", fmt="%s")
        np.savetxt(path_to_save_data + "table_tissue_spectra.csv", spectra, delimiter=",", fmt="%s")
    if denoise in ("TV", "MPPCA"):                                  # motor:302-303
        nifti.save(nifti.NiftiImage(res.pop("data_prepared"), img.affine), path_to_save_data + "Data_denoised.nii.gz")
    if denoise == "MPPCA":
        nifti.save(nifti.NiftiImage(res.pop("MPPCA_sigma"), img.affine), path_to_save_data + "MPPCA_sigma.nii.gz")
    for name in ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param"):
        nifti.save(nifti.NiftiImage(res[name], img.affine), path_to_save_data + name + ".nii.gz")
    if bootstrap is not None:
        from .plan import BOOT_QUANTITIES
        for q in BOOT_QUANTITIES:
            nifti.save(nifti.NiftiImage(res[q + "_bootstrap"], img.affine), path_to_save_data + q + "_bootstrap.nii.gz")
        nifti.save(nifti.NiftiImage(res["sigma"], img.affine), path_to_save_data + "sigma.nii.gz")
        if "FA_bootstrap" in res:
            nifti.save(nifti.NiftiImage(res["FA_bootstrap"], img.affine), path_to_save_data + "FA_bootstrap.nii.gz")
        if "fsol_bootstrap" in res:
            from .plan import BOOT_STATS
            for i, st in enumerate(BOOT_STATS):
                nifti.save(nifti.NiftiImage(np.ascontiguousarray(res["fsol_bootstrap"][..., i]), img.affine),
                           path_to_save_data + "fsol_bootstrap_" + st + ".nii.gz")
    return res


def recon_met2_rois(data, rois, fa_index, Dic_3D, T2s, Laplac, factor=1.01, myelin_T2=40.0, device=0, plan=None):
    """ROI-mode estimation (motor/motor_recon_met2_real_data_ROI.py:405-443): for every ROI label > 0 the mean signal and the
    mean EPG kernel over its voxels (each voxel contributes the dictionary slice of its own flip angle), one X2 fit
    (factor 1.01 there) per ROI, then the spectrum metrics.  data [..., nt], rois [...] integer labels, fa_index [...]
    (indices into the FA axis of Dic_3D [nt, nT2, nFA], reference layout; or pass `plan`, a Met2Plan that already holds the
    dictionary).  The reduction runs on the device (met2_roi_reduce, deterministic).  numpy arrays or CUDA tensors.
    Returns dict(labels, count, fsol [nROI, nT2] normalised to sum 1 like the reference, MWF, IEWF, FWF, T2_M, T2_IE, TWC,
    reg_opt, k_est, mean_signal)."""
    from .plan import voxel_layout, _ptr
    src = plan if plan is not None else plan_for(Dic_3D, device=device)
    dev = src.device
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev)
    nt = dd.shape[-1]
    dd, nvox, vs, es, vol, order = voxel_layout(dd, nt)
    lab = src._per_voxel(torch.as_tensor(rois, device=dev).to(torch.int64), nvox, torch.int64, "rois", order)
    fa = src._per_voxel(torch.as_tensor(fa_index, device=dev), nvox, torch.float64, "fa_index", order)
    labels = torch.unique(lab)
    labels = labels[labels > 0]
    nroi = int(labels.numel())
    if nroi == 0:
        raise ValueError("no ROI label > 0")
    pos = torch.searchsorted(labels, lab).clamp(max=nroi - 1)
    ridx = torch.where(labels[pos] == lab, pos, torch.full_like(pos, -1)).to(torch.int32).contiguous()
    dst = Met2Plan(nt, src.n_t2, nroi, device=dev.index or 0, x2_factor=factor, myelin_T2=myelin_T2)
    try:
        dst.set_t2_grid(T2s).set_penalty(np.asarray(Laplac, dtype=np.float64))
        sig = torch.empty((nroi, nt), dtype=torch.float64, device=dev)
        cnt = torch.empty((nroi,), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            check(lib().met2_roi_reduce(src._h, dst._h, nvox, _ptr(dd), vs, es, _ptr(ridx), _ptr(fa), _ptr(sig), _ptr(cnt), dst._stream()))
        out = dst.fit("X2", sig, fa_index=torch.arange(nroi, dtype=torch.float64, device=dev), want_lambda=True)
        f = out["fsol"].cpu().numpy()
        maps = out["maps"].cpu().numpy()
        res = {"labels": labels.cpu().numpy(), "count": cnt.cpu().numpy(), "fsol": f / maps[5][:, None], "reg_opt": out["lam"].cpu().numpy(),
               "k_est": out["reg"].cpu().numpy(), "mean_signal": sig.cpu().numpy()}
        for i, name in enumerate(MAP_NAMES):
            res[name] = maps[i]
        return res
    finally:
        dst.close()


def motor_recon_met2_ROIs(TE_array, path_to_data, path_to_mask, path_to_ROIs, path_to_save_data, TR, reg_matrix, denoise, FA_method,
                          FA_smooth, myelin_T2, num_cores=-1, device=0, degibbs="no"):
    """Drop-in for motor_recon_met2_ROIs (motor/motor_recon_met2_real_data_ROI.py:152-498): NIfTI data, mask and ROI labels in;
    flip angles per voxel (step 2), then one X2 fit (factor 1.01, :417) per ROI on the ROI's mean signal and mean kernel.
    Writes the reference's tables: table_MWF.csv, table_Spectra.csv, ROI_labels.csv at path_to_save_data and
    ROI_<label>/table_values.csv per ROI (:476-498; the PNG plots and the tabulate text table are not reproduced).
    Labels are taken from the ROI volume before the mask is applied, as the reference does (:175-178); a label that lies
    entirely outside the mask has no voxels and the reference's nnls_x2 raises ValueError on its nan kernel -- so does this.
    degibbs='yes' or '3d': the raw volume is unrung first (gibbs_filter; see recon_met2_arrays)."""
    import os
    from . import nifti
    img = nifti.load(path_to_data)
    data = img.get_fdata().astype(np.float64, copy=False)
    mask = nifti.load(path_to_mask).get_fdata().astype(np.int64)
    rois = nifti.load(path_to_ROIs).get_fdata().astype(np.int64)
    if data.ndim != 4 or mask.shape != data.shape[:3] or rois.shape != mask.shape:
        raise ValueError("data must be 4-D; mask and ROIs must match its first three dimensions")
    if FA_method not in ("brute-force", "spline"):
        raise ValueError("FA_method must be 'spline' or 'brute-force'")
    nt = data.shape[-1]
    labels_all = np.unique(rois)
    labels_all = labels_all[labels_all != 0]
    rois = rois * mask                                              # :191
    dev = torch.device("cuda", device)
    data = _degibbs_first(data, degibbs, False, device)
    dd, mk = _prepare_volume(data, mask, dev, False, denoise)
    dd_fa = gaussian_smooth(dd, 2.0) if FA_smooth == "yes" else dd
    TE_array = np.asarray(TE_array, dtype=np.float64)
    tau = float(TE_array[1] - TE_array[0])
    Npc = 60
    T2s = np.logspace(math.log10(10.0), math.log10(2000.0), num=Npc, endpoint=True, base=10.0)
    T1s = 1000.0 * np.ones_like(T2s)
    alpha_values = np.linspace(90.0, 180.0, 91 * 3 if FA_method == "spline" else 91)
    Laplac = penalty_matrix(reg_matrix, Npc, T2s)
    plan = Met2Plan(nt, Npc, alpha_values.shape[0], device=device, myelin_T2=myelin_T2)
    try:
        plan.build_dictionary_epg(T2s, T1s, tau, alpha_values, TR)
        fa_vol = _estimate_fa(plan, dd_fa, mk > 0, FA_method, None, T2s, T1s, tau, TR, alpha_values, device)
        present = np.intersect1d(labels_all, np.unique(rois))
        if present.size != labels_all.size:
            raise ValueError("array must not contain infs or NaNs")  # a label without voxels inside the mask: 0/0 kernel (see docstring)
        res = recon_met2_rois(dd, torch.as_tensor(rois, device=dev), fa_vol, None, T2s, Laplac, factor=1.01, myelin_T2=myelin_T2,
                              device=device, plan=plan)
    finally:
        plan.close()
    np.savetxt(path_to_save_data + "table_MWF.csv", res["MWF"], delimiter=",", fmt="%s")
    np.savetxt(path_to_save_data + "table_Spectra.csv", res["fsol"], delimiter=",", fmt="%s")
    np.savetxt(path_to_save_data + "ROI_labels.csv", res["labels"], delimiter=",", fmt="%s")
    for i, lab in enumerate(res["labels"]):
        d = path_to_save_data + "ROI_%.0f/" % float(lab)
        os.makedirs(d, exist_ok=True)
        table = [["1. MWF       ", res["MWF"][i]], ["2. IEWF      ", res["IEWF"][i]], ["3. FWF       ", res["FWF"][i]],
                 ["4. T2M       ", res["T2_M"][i]], ["5. T2IE      ", res["T2_IE"][i]], ["6. TWC       ", res["TWC"][i]]]
        np.savetxt(d + "table_values.csv", np.array(table, dtype=object), delimiter=",", fmt="%s")
    return res
