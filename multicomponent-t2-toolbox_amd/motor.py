"""Drop-ins for motor/motor_recon_met2_real_data.py: create_Laplacian_matrix, fitting_slice_T2, recon_met2_arrays (the driver's steps 1-4
on in-memory arrays), motor_recon_met2 (the same with the on-disk contract), the ROI mode (recon_met2_rois, motor_recon_met2_ROIs) and the
atlas statistics of written maps (motor_atlas_stats), the written maps on a template's grid (motor_maps_to_template) and the voxel-wise
group statistics of several subjects' maps on that grid (motor_group_stats).
The whole-volume filters the drivers call (nesma_filter ... gaussian_smooth) are filters.py's, re-exported here; the drivers reach them
through this module's names.  Plots and the mean-spectrum PNG are not reproduced."""
import collections
import contextlib

import numpy as np
import torch

from ._cache import plan_for
from ._lib import check, lib
from .evaluate import study_t2_grid
from .filters import (STAT_KEYS, STAT_QUANTITIES, atlas_stats_filter, bias_field_filter, brain_mask_filter, gaussian_smooth,  # noqa: F401
                      gibbs_filter, group_stats_filter, label_stats_filter, maps_to_template_filter, mppca_filter, nesma_filter, partial_volume_filter,
                      register_filter, resample_filter, resample_labels_filter, tfce_filter, tissue_segment_filter, warp_filter, warp_invert_filter,
                      warp_jacobian_filter, warp_labels_filter, warp_register_filter)
from .plan import BOOT_QUANTITIES, BOOT_STATS, MAP_NAMES, Met2Plan


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


_Protocol = collections.namedtuple("_Protocol", "Npc T2s T1s tau TR alpha_values alpha_lr penalty")
_ALPHA_LR = np.linspace(90.0, 180.0, 15)                             # motor:237: the coarse grid of FA_method='spline'


def _protocol(reg_method, FA_method, TE_array, TR, reg_matrix=None):
    """The drivers' constants (motor:207-244): Npc = 60 T2 bins (96 for T2SPARC) on 10..2000 ms, T1 = 1000 ms, tau = the echo spacing, 91
    flip angles on 90..180 degrees (273 for the spline method, with its 15-angle coarse grid) and the penalty's name (InvT2 for T2SPARC,
    run_real_data_script.py:91-93)."""
    TE_array = np.asarray(TE_array, dtype=np.float64)
    Npc = 96 if reg_method == "T2SPARC" else 60
    T2s = study_t2_grid(Npc)
    alpha_values = np.linspace(90.0, 180.0, 91 * 3 if FA_method == "spline" else 91)
    return _Protocol(Npc, T2s, 1000.0 * np.ones_like(T2s), float(TE_array[1] - TE_array[0]), TR, alpha_values, _ALPHA_LR,
                     "InvT2" if reg_method == "T2SPARC" else reg_matrix)


def _fine_plan(proto, nt, device, myelin_T2, slice_profile=None, penalty=True):
    """a plan with the protocol's dictionary and, unless penalty=False, its penalty on `device`; the caller closes it"""
    plan = Met2Plan(nt, proto.Npc, proto.alpha_values.shape[0], device=device, myelin_T2=myelin_T2)
    plan.build_dictionary_epg(proto.T2s, proto.T1s, proto.tau, proto.alpha_values, proto.TR, slice_profile=slice_profile)
    if penalty:
        plan.set_penalty(proto.penalty, proto.T2s)
    return plan


@contextlib.contextmanager
def _coarse_plan(plan, T2s, T1s, tau, TR, device, attach=False):
    """The 15-angle plan of the spline FA method beside the fine `plan`, with the fine plan's slice profile, on `device`; attach=True
    attaches it to the fine plan for the block (fit_bootstrap(fa='spline')) and detaches it again; closed on exit."""
    plan_lr = Met2Plan(plan.n_te, plan.n_t2, _ALPHA_LR.shape[0], device=device)
    try:
        plan_lr.build_dictionary_epg(T2s, T1s, tau, _ALPHA_LR, TR, slice_profile=plan.slice_profile)
        if attach:
            plan.attach_fa_spline(plan_lr, _ALPHA_LR)
        yield plan_lr
    finally:
        if attach:
            plan.attach_fa_spline(None, None)
        plan_lr.close()


def _degibbs_first(data, degibbs, device):
    """degibbs='yes' or '3d' of the drivers: the raw volume through gibbs_filter, before anything else -> the volume to go on with"""
    if degibbs == "no":
        return data
    return gibbs_filter(np.asarray(data, dtype=np.float64), device=device, mode="3d" if degibbs == "3d" else "2d")


def _bias_last(res, mask, voxel_size, device):
    """bias_correct='yes' of the drivers: res['TWC'] through bias_field_filter with the driver's mask -> the corrected map, and 'TWC_bias'"""
    twc, field, _ = bias_field_filter(np.ascontiguousarray(res["TWC"], dtype=np.float64), np.asarray(mask) != 0, voxel_size, device=device,
                                      return_field=True)
    res["TWC"] = twc
    res["TWC_bias"] = field


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


def _prepare_volume(data, mask, dev, prepared, denoise, maps=None, mppca=(5, False)):
    """The driver's preparation (motor:180-182, :279, :293-333) on the device.  The volume keeps the memory order it
    arrives in (nibabel arrays are Fortran-ordered; the solver reads either order in place).  denoise='MPPCA' (an extension) leaves its
    noise map in maps['MPPCA_sigma'] when the caller hands a dict in; mppca = (window, average) as mppca_filter takes them."""
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
            dd, sigma, _ = mppca_filter(dd, mk, window=mppca[0], average=mppca[1], return_maps=True)
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
        with _coarse_plan(plan, T2s, T1s, tau, TR, device) as plan_lr:
            fa, _, _ = plan.fa_spline(plan_lr, _ALPHA_LR, alpha_values, dd_fa, mm, want_km=False)
    else:
        fa, _, _ = plan.fa_bruteforce(dd_fa, mm)
    return unflatten(fa, vol, order)


_Run = collections.namedtuple("_Run", "degibbs brain_mask denoise rician boot slice_profile bias segment tissue_stats pve_threshold first_dev mppca")


def _resolve_run(data_shape, mask, *, FA_method, FA_smooth, denoise, device, devices, bootstrap, degibbs, bias_correct, voxel_size, brain_mask,
                 segment, tissue_stats, pve_threshold, rician, rician_sigma, rician_iters, slice_profile, prepared=False, distributed=False,
                 plan=None, mask_name="a mask"):
    """The options of recon_met2_arrays and motor_recon_met2 as given -> the _Run record of the steps that run: degibbs ('no' | 'yes' |
    '3d'), brain_mask (bool), denoise (the method's name), rician (None | 'iterative' | 'direct'), boot (None or the dict with n_rep, seed, fa, spectrum),
    slice_profile (None or the validated dict), bias (bool), segment ('no' | 'yes' | 'pve'), tissue_stats (bool), pve_threshold,
    first_dev: devices[0], else the caller's plan's device, else `device`, and mppca: (window, average) as mppca_filter takes them.  Both drivers call it first, so every refusal is a ValueError
    before any device work.  The rules, in the order they are checked (the first bad option wins):
      bootstrap       takes the keys n_rep, seed, fa ('fixed' | 'brute-force' | 'spline') and spectrum only.
      rician          'no' | 'iterative' | 'direct'.  Runs through one plan: not with devices=[...], distributed=True or bootstrap=...;
                      rician_iters in [0, 16], rician_sigma >= 0; 'direct' needs a sigma map: rician_sigma or denoise='MPPCA' (not prepared).
      slice_profile   must pass epg.check_profile.  Runs through one plan: not with devices=[...] or distributed=True, only with a bootstrap
                      whose fa is 'fixed', and it must equal the profile a caller's plan= was built with.
      bootstrap       runs on one device: not with distributed=True.  An fa other than 'fixed' must be the run's FA_method and does not go
                      with FA_smooth='yes'.
      FA_method       'brute-force' | 'spline'.
      denoise         'None' | 'NESMA' | 'TV' | 'MPPCA', or a dict with the key method (one of those) and, optionally, mppca_window and
                      mppca_average and no other key.  mppca_window: an odd int >= 3 or (wx, wy, wz), each odd and >= 1, 3 to 343 voxels
                      (filters.mppca_window; default 5); mppca_average: 'no' | 'yes' (default 'no'; with 'yes' an int window holds at most
                      343 voxels too); either away from its default needs method 'MPPCA'.  (The two ride in `denoise` because the
                      drivers' argument lists are fixed.)
      segment         'no' | 'yes' | 'pve'; needs bias_correct='yes'; not with distributed=True.
      tissue_stats    'no' | 'yes'; needs segment='yes' or 'pve'; not with distributed=True; pve_threshold in [0.5, 1).
      brain_mask      'no' | 'yes'; makes the mask itself: `mask` is None; works on the raw volume: not with prepared=True; not with
                      distributed=True; needs data [nx,ny,nz,nt] and voxel_size=(dx, dy, dz).
      degibbs         'no' | 'yes' | '3d'; works on the raw volume: not with prepared=True; needs data [nx,ny,nz,nt].
      bias_correct    'no' | 'yes'; not with distributed=True; needs data [nx,ny,nz,nt] and voxel_size=(dx, dy, dz).
      devices=[...]   builds its own plans: not with plan= or distributed=True.
    On the devices=[...] leg degibbs, brain_mask, the whole-volume filters (denoise, FA smoothing), bootstrap, bias_correct, segment and
    tissue_stats all run on devices[0]; only the FA step and the fit are dealt over the list.  Under distributed=True degibbs runs on every
    rank's own copy (it is deterministic)."""
    boot = _bootstrap_args(bootstrap)
    denoise_given, mppca_window, mppca_average = denoise, 5, "no"
    if isinstance(denoise, dict):                                # what is wrong with the dict is said where denoise is checked, below
        denoise, mppca_window, mppca_average = denoise.get("method"), denoise.get("mppca_window", 5), denoise.get("mppca_average", "no")
    if rician not in ("no", "iterative", "direct"):
        raise ValueError("rician must be 'no', 'iterative' or 'direct'")
    if rician != "no":
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
    if slice_profile is not None:
        from . import epg as _epg
        slice_profile = _epg.check_profile(slice_profile["r_exc"], slice_profile["r_ref"], slice_profile["w"])        # the weights as given
        if devices is not None:
            raise ValueError("slice_profile runs through one plan and does not go with devices=[...]")
        if distributed:
            raise ValueError("slice_profile does not go with distributed=True")
        if boot is not None and boot["fa"] != "fixed":
            raise ValueError("slice_profile goes with bootstrap fa='fixed' only, not fa=%r" % (boot["fa"],))
        if plan is not None and not _epg.same_profile(slice_profile, plan.slice_profile):
            raise ValueError("slice_profile differs from the one the caller's plan was built with (plan.slice_profile)")
    if boot is not None and distributed:
        raise ValueError("bootstrap runs on one device and does not go with distributed=True")
    _bootstrap_check(boot, FA_method, FA_smooth)
    if FA_method not in ("brute-force", "spline"):
        raise ValueError("FA_method must be 'spline' or 'brute-force'")
    if isinstance(denoise_given, dict) and ("method" not in denoise_given or set(denoise_given) - {"method", "mppca_window", "mppca_average"}):
        raise ValueError("denoise as a dict takes method, mppca_window and mppca_average, and needs method; got %s" % sorted(denoise_given))
    if not isinstance(denoise, (str, type(None))) or denoise not in ("None", None, "none", "NESMA", "TV", "MPPCA"):
        raise ValueError("denoise must be 'None', 'NESMA', 'TV' or 'MPPCA'")
    if mppca_average not in ("no", "yes"):
        raise ValueError("mppca_average must be 'no' or 'yes'")
    from . import filters as _filters
    _filters.mppca_window(mppca_window, mppca_average == "yes")
    if denoise != "MPPCA" and (mppca_average != "no" or np.ndim(mppca_window) != 0 or mppca_window != 5):
        raise ValueError("mppca_window and mppca_average need the denoise method 'MPPCA'")
    mppca = (mppca_window if np.ndim(mppca_window) == 0 else tuple(int(w) for w in mppca_window), mppca_average == "yes")
    _segment_check(segment, bias_correct, distributed)
    tstats = _tissue_stats_check(tissue_stats, segment, distributed, pve_threshold)
    volume = len(data_shape) == 4
    has_voxel_size = voxel_size is not None and np.shape(voxel_size) == (3,)
    if brain_mask not in ("no", "yes"):
        raise ValueError("brain_mask must be 'no' or 'yes'")
    if brain_mask == "yes":
        if mask is not None:
            raise ValueError("brain_mask='yes' makes the mask itself and does not go with " + mask_name)
        if prepared:
            raise ValueError("brain_mask='yes' works on the raw volume and does not go with prepared=True")
        if distributed:
            raise ValueError("brain_mask='yes' does not go with distributed=True")
        if not volume:
            raise ValueError("brain_mask='yes' needs data [nx,ny,nz,nt]")
        if not has_voxel_size:
            raise ValueError("brain_mask='yes' needs voxel_size=(dx, dy, dz) in mm")
    if degibbs not in ("no", "yes", "3d"):
        raise ValueError("degibbs must be 'no', 'yes' or '3d'")
    if degibbs != "no":
        if prepared:
            raise ValueError("degibbs='%s' works on the raw volume and does not go with prepared=True" % degibbs)
        if not volume:
            raise ValueError("degibbs='%s' needs data [nx,ny,nz,nt]" % degibbs)
    if bias_correct not in ("no", "yes"):
        raise ValueError("bias_correct must be 'no' or 'yes'")
    if bias_correct == "yes":
        if distributed:
            raise ValueError("bias_correct='yes' does not go with distributed=True: the map is complete only after the gather")
        if not volume:
            raise ValueError("bias_correct='yes' needs data [nx,ny,nz,nt]")
        if not has_voxel_size:
            raise ValueError("bias_correct='yes' needs voxel_size=(dx, dy, dz) in mm")
    if devices is not None and (plan is not None or distributed):
        raise ValueError("devices=[...] builds its own plans and does not go with distributed=True")
    first_dev = devices[0] if devices else plan.device.index or 0 if plan is not None else device
    return _Run(degibbs, brain_mask == "yes", denoise, None if rician == "no" else rician, boot, slice_profile, bias_correct == "yes", segment,
                tstats, pve_threshold, first_dev, mppca)


def _finish(run, res, dd, mask, plan, proto, reg_method, voxel_size, myelin_T2):
    """The tail of every leg of recon_met2_arrays, on the result dict `res`, the prepared volume `dd` and a plan with the run's dictionary
    (None when neither the bootstrap nor the tissue statistics run): bootstrap, bias correction, segmentation, tissue statistics."""
    if run.boot is not None:
        _bootstrap_into(res, plan, reg_method, dd, res["FA_index"], mask > 0, run.boot, proto)
    if run.bias:
        _bias_last(res, mask, voxel_size, run.first_dev)
    if run.segment != "no":
        _segment_last(res, mask, voxel_size, run.first_dev, run.segment)
    if run.tissue_stats:
        _tissue_stats_last(res, dd, plan, run.segment, run.pve_threshold, myelin_T2)
    return res


def recon_met2_arrays(data, mask, TE_array, TR, reg_method="X2", reg_matrix="L2", FA_method="brute-force", myelin_T2=40.0,
                      fa_index=None, device=0, plan=None, denoise="None", prepared=False, FA_smooth="no", distributed=False,
                      return_prepared=False, devices=None, bootstrap=None, degibbs="no", bias_correct="no", voxel_size=None,
                      brain_mask="no", segment="no", tissue_stats="no", pve_threshold=0.9, rician="no", rician_sigma=None, rician_iters=3,
                      slice_profile=None):
    """Steps 1-4 of motor_recon_met2 (motor:293-373, 427-472) on arrays: data [nx,ny,nz,nt] (or
    [nvox, nt]), mask [nx,ny,nz].  Mirrors the driver's preparation: data *= mask (motor:180-182),
    negative values clipped to 0 (motor:279), optional NESMA / TV filter (motor:293-333, needs a 3-D volume) or denoise='MPPCA'
    (mppca_filter with window 5, an extension; what it leaves below zero is set to zero; return_prepared=True then adds 'MPPCA_sigma';
    denoise={'method': 'MPPCA', 'mppca_window': (wx, wy, wz), 'mppca_average': 'yes'} hands mppca_filter a box patch for anisotropic
    voxels, e.g. (5, 5, 1) for 2-D multi-slice data, and has it average the estimates of all patches that hold a voxel -- its window and
    average; either key may be left out; rician='direct' takes the noise map of whichever mode ran),
    and the constants of _protocol.  `prepared=True` says the caller already did that preparation (mask multiply, clip, denoise).
    Every option below defaults to a value that changes no output and no launch; what each refuses, always before any device work, and
    where it runs on the devices=[...] leg is stated once, in _resolve_run.
    degibbs='yes' (step 2 of the reference's example script, which runs MRtrix's mrdegibbs there): the raw volume goes through gibbs_filter
    first -- before the mask multiply, the clip and any denoise, so the clip also removes what the unringing leaves below zero.  MRtrix
    recommends MP-PCA denoising BEFORE unringing: a caller who wants that order calls mppca_filter and gibbs_filter themselves and passes
    prepared=True.  degibbs='3d': the same with gibbs_filter(mode='3d'), for 3-D Fourier-encoded acquisitions (every echo volume unrung
    along x, y and z; needs 8 <= nz <= 256 too).
    brain_mask='yes' (step 3 of that script, which runs FSL's fslmaths -Tmean and bet -m -f 0.4 there): `mask` is None and the mask is made
    by brain_mask_filter from the echo mean of the raw volume -- of the unrung one with degibbs -- with voxel_size=(dx, dy, dz) in mm, after
    degibbs and before the mask multiply; the result carries it as 'mask' (uint8).  Parity with bet itself is unpinned.
    bias_correct='yes' (step 5 of that script, which runs FSL's fast on the TWC map there): after everything else the total water content
    map goes through bias_field_filter with the driver's mask and voxel_size; 'TWC' becomes the corrected map and 'TWC_bias' the estimated
    field; the other outputs, the bootstrap's included, are not touched.  Parity with fast itself is unpinned (no Markov random field term).
    segment='yes' (the other product of that fast call): the corrected TWC map then goes through tissue_segment_filter with the same mask
    and voxel_size (3 classes, beta 0.1: fast -n 3 -H 0.1) and the result gains 'TWC_seg' (uint8: 0 outside, 1..3 by ascending water
    content) and 'TWC_prob' [3,nx,ny,nz] (the class posteriors).  segment='pve': everything 'yes' gives, then partial_volume_filter on the
    map, the labels and the posteriors (beta_pv 0.3: fast's -R default) adds 'TWC_pve' [3,nx,ny,nz] (the tissue fractions, what fast writes
    as _pve_k: a white-matter mask for MWF statistics is TWC_pve[k] > 0.9, not a hard label), 'TWC_pveseg' and 'TWC_mixeltype' (uint8).
    tissue_stats='yes' (an extension: the reference's TO DO (2) of motor:376 and its mean-spectrum numbers of motor:377-403, per tissue):
    after the segmentation the result gains 'tissue_stats', the dict of label_stats_filter on the tissue labels -- TWC_seg with
    segment='yes'; with 'pve' label k + 1 where TWC_pve[k] > pve_threshold (in [0.5, 1), so that no voxel has two labels) -- plus 'all', the
    same statistics of the whole segmented domain (TWC_seg > 0), and 'mean_signal_fsol' [L + 1, n_t2] with 'mean_signal_<map>' [L + 1]: the
    X2 fit (penalty I, factor 1.01) of every label's mean signal on its mean kernel, the last row the whole domain (recon_met2_rois on the
    prepared data and the run's FA_index).
    FA_smooth='yes' (the CLI default, motor:337-343): the flip angles are estimated on the Gaussian-smoothed volume
    (sigma = 2 voxels, every echo), the spectra on the unsmoothed one; needs a 3-D volume.
    C- and Fortran-ordered volumes (nibabel's) are both read in place.
    distributed=True (under torch.distributed.run, one rank per GPU): every rank holds the volume, runs the FA step and the
    fit on its own interleaved 4096-voxel blocks of the voxel list and the outputs meet on rank 0 in ONE gather
    (dist.fit_sharded); ranks other than 0 return None.
    devices=[d0, d1, ...]: ONE process drives several GPUs through the C ABI's host entry (met2_fit_host: one plan and one host thread per
    device inside the call, blocks of voxels dealt round-robin, outputs copied by every device into the same host arrays -- no
    torch.distributed).  Same outputs bit for bit.  Without devices, plan, distributed, rician and slice_profile a volume takes this leg
    with devices=[device].
    bootstrap=dict(n_rep=100, seed=0): per-voxel bootstrap uncertainty of the metrics (Met2Plan.fit_bootstrap; an extension with no
    counterpart in the reference), on one device with the pipeline's prepared data and FA indices; voxel_id is the voxel's flat
    index in the volume's C order, whatever the memory order.  Adds '<Q>_bootstrap' [vol..., 5] for Q in BOOT_QUANTITIES (BOOT_STATS along
    the last axis), 'sigma' and 'rep_status'; the ten outputs are those of the same run without it.  Two more keys (Met2Plan.fit_bootstrap's
    fa and want_spectrum): fa='fixed' (default) | 'brute-force' | 'spline' -- other than 'fixed' every replicate gets its own flip angle and
    'FA_bootstrap' [vol..., 5] (degrees) is added (see _bootstrap_check).  spectrum=True adds 'fsol_bootstrap' [vol..., n_t2, 5], the
    per-bin band of the T2 spectrum.
    rician='iterative' | 'direct' (an extension: the Rician noise floor of the echo magnitudes, which the fit otherwise reads as a long-T2
    pool).  'iterative': after the FA step the fit is Met2Plan.fit_rician with rician_iters passes (default 3) at the noise level
    rician_sigma (a number or a volume) or, without one, at the residual estimate of Met2Plan.noise_sigma; adds 'sigma', 'SNR' (first echo
    of the model signal over sigma, 0 where sigma = 0) and 'rician_flag'; 'Est_Signal' is then the noise-free signal estimate.  'direct':
    the prepared volume goes through rician.invert before the FA step and the fit, which run once -- the one-shot correction of denoised
    magnitudes; it takes rician_sigma or the map denoise='MPPCA' leaves, and adds 'sigma' and 'data_rician' (the corrected volume).  It
    treats a denoised magnitude as the Rician mean, which it only approximates.  sigma is never re-estimated after a correction, and the
    residual estimate is biased low where many echoes sit in the floor; neither mode makes the fit a maximum-likelihood Rician fit.
    slice_profile=<the dict of epg.slice_profile> (an extension, for 2-D multi-slice multi-echo spin echo: the flip angles vary across the
    slice and the decay is the integral of the echo trains over the profile, Lebel & Wilman 2010): every dictionary of the run -- the run's
    own plan, the coarse plan of FA_method='spline', and with them what tissue_stats and bootstrap=dict(fa='fixed') reuse -- is built by
    Met2Plan.build_dictionary_epg(slice_profile=...).  'FA' is then the nominal refocusing angle at the slice centre, on the unchanged
    90..180 degree grid.  A caller's own plan= keeps the dictionary it has.
    Returns a dict with the driver's ten outputs."""
    data = np.asarray(data, dtype=np.float64)
    run = _resolve_run(data.shape, mask, FA_method=FA_method, FA_smooth=FA_smooth, denoise=denoise, device=device, devices=devices,
                       bootstrap=bootstrap, degibbs=degibbs, bias_correct=bias_correct, voxel_size=voxel_size, brain_mask=brain_mask,
                       segment=segment, tissue_stats=tissue_stats, pve_threshold=pve_threshold, rician=rician, rician_sigma=rician_sigma,
                       rician_iters=rician_iters, slice_profile=slice_profile, prepared=prepared, distributed=distributed, plan=plan)
    data = _degibbs_first(data, run.degibbs, run.first_dev)
    made = brain_mask_filter(np.ascontiguousarray(data), voxel_size, device=run.first_dev) if run.brain_mask else None
    vol_shape, nt = data.shape[:-1], data.shape[-1]
    mask = np.asarray(made if run.brain_mask else mask).reshape(vol_shape)
    proto = _protocol(reg_method, FA_method, TE_array, TR, reg_matrix)
    if devices is None and plan is None and not distributed and data.ndim >= 2 and not run.rician and run.slice_profile is None:
        devices = [device]                                       # the default: one device, through the C ABI's host entry (met2_fit_host: the block
                                                                 # pipeline inside the library; the torch pipeline of rounds 3-4 is retired to tests/tools)
    needs_plan = run.boot is not None or run.tissue_stats
    own = None
    try:
        if devices is not None:
            res = _recon_multi_device(data, mask, proto, reg_method, FA_method, myelin_T2, fa_index, list(devices), prepared, run.denoise, FA_smooth,
                                      return_prepared=return_prepared or needs_plan, mppca=run.mppca)
            dd = None
            if needs_plan:                                       # a plan with the run's dictionary on devices[0]: the host entry closed its own
                dd = res["data_prepared"] if return_prepared else res.pop("data_prepared")
                if not return_prepared:
                    res.pop("MPPCA_sigma", None)
                plan = own = _fine_plan(proto, nt, devices[0], myelin_T2)
        else:                                                    # a caller's own plan, a distributed run, rician, slice_profile: the volume in one piece
            if plan is None:
                plan = own = _fine_plan(proto, nt, device, myelin_T2, run.slice_profile)
            res, dd = _recon_one_plan(run, plan, proto, data, mask, reg_method, FA_method, fa_index, prepared, FA_smooth, distributed,
                                      rician_sigma=rician_sigma, rician_iters=rician_iters, return_prepared=return_prepared, device=device)
            if distributed:
                return res
        if made is not None:
            res["mask"] = made
        return _finish(run, res, dd, mask, plan, proto, reg_method, voxel_size, myelin_T2)
    finally:
        if own is not None:
            own.close()


def _recon_one_plan(run, plan, proto, data, mask, reg_method, FA_method, fa_index, prepared, FA_smooth, distributed, rician_sigma, rician_iters,
                    return_prepared, device):
    """The plan and sharded legs of recon_met2_arrays: the volume on the plan's device in one piece -> (the result dict, the prepared
    volume the fit read); under distributed=True (what _recon_sharded returns, None)."""
    dev, vol_shape = plan.device, data.shape[:-1]
    extra = {}
    dd, mk = _prepare_volume(data, mask, dev, prepared, run.denoise, extra, run.mppca)
    mm = (mk > 0)
    sigma_vol = _rician_sigma(run.rician, rician_sigma, extra, vol_shape, dev)
    dd_prepared = dd
    if run.rician == "direct":
        from . import rician as _rician
        dd = _rician.invert(dd, sigma_vol, mm)
    dd_fa = dd
    if FA_smooth == "yes" and fa_index is None:
        if len(vol_shape) != 3:
            raise ValueError("FA_smooth='yes' needs data [nx,ny,nz,nt]")
        dd_fa = gaussian_smooth(dd, 2.0)
    if distributed:
        return _recon_sharded(plan, proto, dd, dd_fa, mm, reg_method, FA_method, fa_index, device, vol_shape), None
    fa_vol = _estimate_fa(plan, dd_fa, mm, FA_method, fa_index, proto.T2s, proto.T1s, proto.tau, proto.TR, proto.alpha_values, device)
    if run.rician == "iterative":
        out = plan.fit_rician(reg_method, dd, n_iter=int(rician_iters), sigma=sigma_vol, fa_index=fa_vol, mask=mm)
    else:
        out = plan.fit(reg_method, dd, fa_index=fa_vol, mask=mm)
    tot_fa = dd_fa.sum(dim=-1)
    res = {"fsol_4D": out["fsol"].cpu().numpy(), "Est_Signal": out["sig"].cpu().numpy(), "reg_param": out["reg"].cpu().numpy(),
           "FA_index": fa_vol.cpu().numpy()}
    if run.rician == "iterative":
        sg = out["sigma"]
        res["sigma"] = sg.cpu().numpy()
        res["SNR"] = torch.where(sg > 0, out["sig"][..., 0] / torch.where(sg > 0, sg, torch.ones_like(sg)), torch.zeros_like(sg)).cpu().numpy()
        res["rician_flag"] = out["rician_flag"].cpu().numpy()
    elif run.rician == "direct":
        res["sigma"] = sigma_vol.cpu().numpy()
        res["data_rician"] = dd.cpu().numpy()
    fitted_fa = (mm & (tot_fa > 0)).cpu().numpy()      # gate of the FA step (fa_estimation.py:45)
    res["FA"] = np.where(fitted_fa, proto.alpha_values[res["FA_index"].astype(int)], 0.0)
    maps = out["maps"].cpu().numpy()
    for i, name in enumerate(MAP_NAMES):
        res[name] = maps[i]
    res["T2s"] = proto.T2s
    if return_prepared:
        res["data_prepared"] = dd_prepared.cpu().numpy()
        for name, t in extra.items():
            res[name] = t.cpu().numpy()
    return res, dd


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


def _bootstrap_into(res, plan, reg_method, dd, fa_vol, mask, boot, proto):
    """recon_met2_arrays(bootstrap=...): Met2Plan.fit_bootstrap on the prepared volume dd [vol..., nt] with the run's FA indices and mask;
    the statistics go into res beside the ten outputs, which stay as the run made them.  proto: what the coarse plan of fa='spline' is
    built from."""
    dd = torch.as_tensor(dd).to(plan.device)
    vol = tuple(dd.shape[:-1])
    vid = np.arange(int(np.prod(vol)), dtype=np.int64).reshape(vol)       # the C-order flat index: independent of the memory order
    with contextlib.ExitStack() as coarse:
        if boot["fa"] == "spline":
            coarse.enter_context(_coarse_plan(plan, proto.T2s, proto.T1s, proto.tau, proto.TR, plan.device.index or 0, attach=True))
        out = plan.fit_bootstrap(reg_method, dd, n_rep=boot["n_rep"], seed=boot["seed"], fa_index=fa_vol, mask=mask, voxel_id=vid,
                                 want_sig=True, want_status=False, fa=boot["fa"], want_spectrum=boot["spectrum"])
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


def _recon_multi_device(data, mask, proto, reg_method, FA_method, myelin_T2, fa_index, devices, prepared, denoise, FA_smooth, return_prepared=False,
                        mppca=(5, False)):
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
        dd, _ = _prepare_volume(data, mask, dev0, prepared, denoise, extra, mppca)
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
    Npc, alpha_values = proto.Npc, proto.alpha_values
    plans = []
    with contextlib.ExitStack() as coarse:                       # closed after the fine plans: a coarse plan outlives its attachment
        try:
            for d in devices:
                plans.append(_fine_plan(proto, nt, d, myelin_T2))
            mode = False
            if fa_index is None:
                mode = "brute-force"
                if FA_method == "spline":
                    lr = [coarse.enter_context(_coarse_plan(p, proto.T2s, proto.T1s, proto.tau, proto.TR, d)) for p, d in zip(plans, devices)]
                    mhost.attach_fa_spline(plans, lr, proto.alpha_lr, alpha_values)
                    mode = "spline"
            nvox = int(np.prod(vol_shape))
            pin = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, pin_memory=True).numpy()     # torch's caching host allocator: reused across calls
            bufs = {"fsol": pin((nvox, Npc)), "sig": pin((nvox, nt)), "reg": pin((nvox,)), "maps": pin((6, nvox)), "status": pin((nvox,), torch.int32),
                    "fa_index": pin((nvox,)), "fa_gate": pin((nvox,))}
            out = mhost.fit_host(plans, reg_method, vol, fa_index=fa_index, mask=mask > 0, estimate_fa=mode, fa_data=fa_vol, mask_values=mvals, want_gate=True,
                                 chunk=PIPELINE_CHUNK if PIPELINE_CHUNK != 262144 else 0, out=bufs)     # (0: the library's block size; a test that sets PIPELINE_CHUNK gets its chunks)
        finally:
            for p in plans:
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
    res["T2s"] = proto.T2s
    if return_prepared:
        if mvals is not None:                                     # (plain runs prepare per block inside the library)
            vol = np.maximum(vol * mvals[..., None], 0.0)
        res["data_prepared"] = vol.cpu().numpy() if torch.is_tensor(vol) else vol
        for name, t in extra.items():
            res[name] = t.cpu().numpy()
    return res


def _recon_sharded(plan, proto, dd, dd_fa, mm, reg_method, FA_method, fa_index, device, vol_shape):
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
        fa = _estimate_fa(plan, dfa, m, FA_method, None if faflat is None else faflat[idx].cpu().numpy(), proto.T2s, proto.T1s, proto.tau, proto.TR,
                          proto.alpha_values, device)
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
    res["FA"] = np.where(full["fa_gate"].cpu().numpy().reshape(vol_shape) > 0, proto.alpha_values[res["FA_index"].astype(int)], 0.0)
    maps = full["maps"].cpu().numpy()
    for i, name in enumerate(MAP_NAMES):
        res[name] = maps[i].reshape(vol_shape)
    res["T2s"] = proto.T2s
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
    map MPPCA_sigma.nii.gz; the dict form with mppca_window and mppca_average as for recon_met2_arrays).  degibbs='yes' or '3d' (see recon_met2_arrays): the raw volume is unrung first (gibbs_filter) and written as
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
    voxel_size = tuple(abs(float(p)) or 1.0 for p in img.header.get("pixdim", (1.0,) * 8)[1:4])
    run = _resolve_run(data.shape, path_to_mask, FA_method=FA_method, FA_smooth=FA_smooth, denoise=denoise, device=device, devices=devices,
                       bootstrap=bootstrap, degibbs=degibbs, bias_correct=bias_correct, voxel_size=voxel_size, brain_mask=brain_mask,
                       segment=segment, tissue_stats=tissue_stats, pve_threshold=pve_threshold, rician=rician, rician_sigma=rician_sigma,
                       rician_iters=rician_iters, slice_profile=slice_profile, mask_name="path_to_mask")
    mask = None if run.brain_mask else nifti.load(path_to_mask).get_fdata().astype(np.int64)
    if data.ndim != 4 or (mask is not None and mask.shape != data.shape[:3]):
        raise ValueError("data must be 4-D and mask must match its first three dimensions")

    def save(a, stem):
        nifti.save(nifti.NiftiImage(a, img.affine), path_to_save_data + stem + ".nii.gz")

    if run.degibbs != "no":
        data = _degibbs_first(data, run.degibbs, run.first_dev)
        save(data, "Data_degibbs")
    if run.brain_mask:
        from . import bet
        avg = bet.bet_mean(np.ascontiguousarray(data), device=run.first_dev)
        mask = brain_mask_filter(avg, voxel_size, device=run.first_dev)
        save(avg, "Data_avg")
        save(mask, "mask")
    res = recon_met2_arrays(data, mask, TE_array, TR, reg_method=reg_method, reg_matrix=reg_matrix, FA_method=FA_method, myelin_T2=myelin_T2,
                            device=device, denoise=denoise, FA_smooth=FA_smooth, return_prepared=(run.denoise in ("TV", "MPPCA")), devices=devices,
                            bootstrap=bootstrap, bias_correct=bias_correct, voxel_size=voxel_size, segment=segment, tissue_stats=tissue_stats,
                            pve_threshold=pve_threshold, rician=rician, rician_sigma=rician_sigma, rician_iters=rician_iters,
                            slice_profile=slice_profile)
    if run.brain_mask:
        res["mask"] = mask
    for key, stem, pop, axis, names in _OUTPUT_FILES:
        if key not in res:
            continue
        a = res.pop(key) if pop else res[key]
        if axis is None:
            save(a, stem)
        else:
            for name, part in zip(names or range(a.shape[axis]), np.moveaxis(a, axis, 0)):
                save(np.ascontiguousarray(part), stem % name)
    if "tissue_stats" in res:
        table, spectra = tissue_stats_tables(res["tissue_stats"])
        np.savetxt(path_to_save_data + "table_tissue_stats.csv", table, delimiter=",", fmt="%s")
        np.savetxt(path_to_save_data + "table_tissue_spectra.csv", spectra, delimiter=",", fmt="%s")
    return res


def _file(key, stem=None, pop=False, axis=None, names=None):
    return key, stem or key, pop, axis, names


# The NIfTI files motor_recon_met2 writes of the result dict, in this order: (key, file stem, whether the key is popped from the returned
# dict, and for a stacked key the axis it is split along and the names that go into the stem: the index by default).  A key the options did
# not produce is skipped.  Data_degibbs, Data_avg and mask are written before the fit; the tissue statistics go to two CSV tables.
_OUTPUT_FILES = (
    (_file("sigma"), _file("SNR"), _file("rician_flag"), _file("data_rician", "Data_rician", pop=True), _file("TWC_bias"), _file("TWC_seg"),
     _file("TWC_prob", "TWC_prob_%d", axis=0), _file("TWC_pve", "TWC_pve_%d", axis=0), _file("TWC_pveseg"), _file("TWC_mixeltype"),
     _file("data_prepared", "Data_denoised", pop=True), _file("MPPCA_sigma", pop=True))           # Data_denoised: motor:302-303
    + tuple(_file(k) for k in ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param"))
    + tuple(_file(q + "_bootstrap") for q in BOOT_QUANTITIES)
    + (_file("FA_bootstrap"), _file("fsol_bootstrap", "fsol_bootstrap_%s", axis=-1, names=BOOT_STATS)))


def roi_stats_tables(st, names=None):
    """the two tables motor_atlas_stats writes from the dict of atlas_stats_filter, in the layout of tissue_stats_tables -> (stats
    [(L + 1) * 8, 5 + n_q] of objects: label, quantity, n, mean, std, q...; spectra [1 + (L + 1), n_t2] of floats: T2s, then per label the
    normalised mean spectrum); the last label, 'all', is every voxel that carries a label, where st['all'] is given.  `names` maps a label
    value to the name that stands in the label column (a dict, or a sequence indexed by label value); other labels keep their number.
    There is no mean-signal spectrum row: the echo data are not read."""
    def name_of(x):
        x = int(x)
        if isinstance(names, dict):
            return str(names.get(x, x))
        return str(names[x]) if names is not None and 0 <= x < len(names) else str(x)

    labels = [name_of(x) for x in st["labels"]] + (["all"] if "all" in st else [])
    rows, spectra = [], [np.asarray(st["T2s"], dtype=np.float64)]
    for i, name in enumerate(labels):
        src = st["all"] if i == len(st["labels"]) else {k: st[k][i] for k in STAT_KEYS}
        for j, quantity in enumerate(st["quantities"]):
            rows.append([name, quantity, src["n"][j], src["mean"][j], src["std"][j]] + list(src["quantiles"][j]))
        spectra.append(src["spectrum_mean"])
    return np.array(rows, dtype=object), np.array(spectra, dtype=np.float64)


def motor_atlas_stats(path_to_save_data, path_to_labels, path_to_world=None, names=None, path_to_template=None, register=None, nonlinear=None):
    """Per-ROI statistics of the maps motor_recon_met2 wrote at path_to_save_data (MWF ... reg_param and fsol_4D .nii.gz, found through
    _OUTPUT_FILES' naming), for an atlas or parcellation image that lies on a grid of its own: path_to_labels is its NIfTI, whose affine places it
    in world space; path_to_world an optional plain-text 4 x 4 matrix (np.loadtxt) taking the maps' world mm to the label image's (None: both
    share scanner space; resample.from_flirt turns a FLIRT matrix into one).  The labels go onto the maps' grid by nearest neighbour
    (atlas_stats_filter) and are written as ROIs_resampled.nii.gz with the maps' affine; table_roi_stats.csv holds one row per (label,
    quantity) -- label, quantity, n, mean, std and the quantiles 0.025 .. 0.975; the last label, 'all', is every labelled voxel --, and
    table_roi_spectra.csv the T2 grid and per label the normalised mean spectrum (roi_stats_tables; `names` as there).  Runs on device 0.
    path_to_template: the atlas' intensity image, a NIfTI in the label image's world space, instead of path_to_world (both: refused).  The world
    matrix is then estimated: the template is registered (register_filter; `register`: a dict of its options, e.g. {"cost": "nmi"} for normalised mutual information) to the maps' reference volume,
    Data_avg.nii.gz at path_to_save_data or, where that is absent, TWC.nii.gz.  template_to_maps_world.txt holds the matrix (np.savetxt; what
    path_to_world reads), template_to_maps_flirt.mat its FLIRT form (resample.to_flirt: `flirt -in <template> -ref <reference> -applyxfm
    -init` takes it), template_resampled.nii.gz the template on the maps' grid, trilinear, for a look.
    nonlinear (with path_to_template; None: nothing below happens and every file is what it was): True, or a dict of warp_register_filter's
    options.  After the affine registration the template is registered non-linearly to the reference from that matrix, and the labels go
    through the displacement field (warp_labels_filter).  template_to_maps_warp.nii.gz holds the field (4-D [x, y, z, 3], in voxels of the
    maps' grid, applied after the world matrix), template_warped.nii.gz the template through matrix and field, trilinear.
    -> the dict of atlas_stats_filter with 'all' added (and 'world' with a template; 'disp' and 'warp_levels' with nonlinear)."""
    import os
    from . import nifti, resample
    if path_to_template is not None and path_to_world is not None:
        raise ValueError("give path_to_template or path_to_world, not both")
    if path_to_template is None and register is not None:
        raise ValueError("register goes with path_to_template")
    if nonlinear is not None and not (nonlinear is True or isinstance(nonlinear, dict)):
        raise ValueError("nonlinear must be None, True or a dict of warp_register_filter's options")
    if nonlinear is not None and path_to_template is None:
        raise ValueError("nonlinear goes with path_to_template: the field is estimated from the template")
    stems = {key: stem for key, stem, _, _, _ in _OUTPUT_FILES}
    res, affine = {}, None
    for key in STAT_QUANTITIES + ("fsol_4D",):
        img = nifti.load(path_to_save_data + stems[key] + ".nii.gz")
        res[key] = img.get_fdata()
        affine = img.affine if affine is None else affine
    if res["fsol_4D"].ndim != 4 or any(res[k].shape != res["fsol_4D"].shape[:3] for k in STAT_QUANTITIES):
        raise ValueError("the maps at path_to_save_data do not share one grid")
    res["T2s"] = study_t2_grid(res["fsol_4D"].shape[-1])
    lab_img = nifti.load(path_to_labels)
    labels = lab_img.get_fdata()
    if labels.ndim != 3 or not np.array_equal(labels, np.round(labels)):
        raise ValueError("the label image must be a 3-D volume of integers")
    world = None if path_to_world is None else np.loadtxt(path_to_world, dtype=np.float64)
    if world is not None and world.shape != (4, 4):
        raise ValueError("path_to_world must hold a 4 x 4 matrix")
    if path_to_template is not None:
        tpl = nifti.load(path_to_template)
        template = tpl.get_fdata()
        if template.ndim != 3:
            raise ValueError("the template must be a 3-D volume")
        ref_path = path_to_save_data + "Data_avg.nii.gz"
        ref = nifti.load(ref_path if os.path.exists(ref_path) else path_to_save_data + stems["TWC"] + ".nii.gz").get_fdata()
        if ref.shape != res["MWF"].shape:
            raise ValueError("the reference volume does not lie on the grid of the maps")
        world = register_filter(ref, affine, template, tpl.affine, **dict(register or {}))
        np.savetxt(path_to_save_data + "template_to_maps_world.txt", world)
        np.savetxt(path_to_save_data + "template_to_maps_flirt.mat", resample.to_flirt(world, tpl.affine, template.shape, affine, ref.shape))
        on_maps = resample_filter(template, resample.voxel_matrix(affine, tpl.affine, world), ref.shape, order=1)
        nifti.save(nifti.NiftiImage(on_maps, affine), path_to_save_data + "template_resampled.nii.gz")
    nl = None
    if nonlinear is not None:
        nl = warp_register_filter(ref, affine, template, tpl.affine, world, **(nonlinear if isinstance(nonlinear, dict) else {}))
        nifti.save(nifti.NiftiImage(nl["disp"], affine), path_to_save_data + "template_to_maps_warp.nii.gz")
        warped = warp_filter(template, resample.voxel_matrix(affine, tpl.affine, world), nl["disp"], order=1)
        nifti.save(nifti.NiftiImage(warped, affine), path_to_save_data + "template_warped.nii.gz")
    st = atlas_stats_filter(res, labels.astype(np.int64), lab_img.affine, affine, world=world, **({} if nl is None else {"disp": nl["disp"]}))
    if path_to_template is not None:
        st["world"] = world
    if nl is not None:
        st["disp"], st["warp_levels"] = nl["disp"], nl["levels"]
    lab = st["labels_resampled"]
    al = label_stats_filter(res, (lab > 0).astype(np.int32), q=st["q"])
    st["all"] = {k: al[k][0] for k in STAT_KEYS}
    nifti.save(nifti.NiftiImage(lab, affine), path_to_save_data + "ROIs_resampled.nii.gz")
    table, spectra = roi_stats_tables(st, names)
    np.savetxt(path_to_save_data + "table_roi_stats.csv", table, delimiter=",", fmt="%s")
    np.savetxt(path_to_save_data + "table_roi_spectra.csv", spectra, delimiter=",", fmt="%s")
    return st


def motor_maps_to_template(path_to_save_data, path_to_template, path_to_world=None, path_to_warp=None, register=None, nonlinear=None, order=1,
                           n_iter=20):
    """The maps motor_recon_met2 wrote at path_to_save_data (MWF ... reg_param .nii.gz, found as motor_atlas_stats finds them) brought INTO
    template space, the direction opposite to motor_atlas_stats: for voxel-wise comparison and averaging across subjects.  path_to_template
    is the template's NIfTI.  The world matrix (the maps' world mm -> the template's) comes from path_to_world -- a plain-text 4 x 4 matrix,
    e.g. the template_to_maps_world.txt motor_atlas_stats wrote -- or is estimated as motor_atlas_stats estimates it: the template is
    registered (register_filter; `register`: a dict of its options) to Data_avg.nii.gz or, where that is absent, TWC.nii.gz.  The field
    comes from path_to_warp (4-D [x, y, z, 3] on the maps' grid, e.g. template_to_maps_warp.nii.gz), or is estimated after the registration
    (nonlinear: True or a dict of warp_register_filter's options), or there is none.  path_to_warp together with nonlinear is refused, and so
    are register or nonlinear together with path_to_world.  The field is inverted by `n_iter` fixed-point steps (warp_invert_filter: it
    converges only where the field is a contraction; the report holds what to judge it by) and the maps go through its inverse
    (maps_to_template_filter; order 0 or 1 with a field), 0 outside.  Runs on device 0.
    Written with the template's affine: <map>_in_template.nii.gz per map, maps_to_template_inside.nii.gz and, with a field,
    maps_to_template_warp.nii.gz (the inverse field, 4-D [x, y, z, 3], in voxels of the template's grid, applied after the inverse of the
    world matrix); with the maps' affine template_to_maps_jacobian.nii.gz (with a field); maps_to_template_report.txt: the residual per
    step, the number and share of voxels whose Jacobian determinant is not positive, and its smallest and largest value.
    -> the dict of maps_to_template_filter, with 'world' and 'disp' (the field on the maps' grid that was inverted; None without one)."""
    import os
    from . import nifti
    if path_to_world is not None and (register is not None or nonlinear is not None):
        raise ValueError("register and nonlinear estimate the world matrix: give them or path_to_world, not both")
    if path_to_warp is not None and nonlinear is not None:
        raise ValueError("give path_to_warp or nonlinear, not both")
    if nonlinear is not None and not (nonlinear is True or isinstance(nonlinear, dict)):
        raise ValueError("nonlinear must be None, True or a dict of warp_register_filter's options")
    stems = {key: stem for key, stem, _, _, _ in _OUTPUT_FILES}
    res, affine = {}, None
    for key in STAT_QUANTITIES:
        img = nifti.load(path_to_save_data + stems[key] + ".nii.gz")
        res[key] = img.get_fdata()
        affine = img.affine if affine is None else affine
    shape = res[STAT_QUANTITIES[0]].shape
    if len(shape) != 3 or any(res[k].shape != shape for k in STAT_QUANTITIES):
        raise ValueError("the maps at path_to_save_data do not share one grid")
    tpl = nifti.load(path_to_template)
    template = tpl.get_fdata()
    if template.ndim != 3:
        raise ValueError("the template must be a 3-D volume")
    disp = None
    if path_to_warp is not None:
        disp = nifti.load(path_to_warp).get_fdata()
        if disp.shape != shape + (3,):
            raise ValueError("the field at path_to_warp must be [x, y, z, 3] on the grid of the maps")
    if path_to_world is not None:
        world = np.loadtxt(path_to_world, dtype=np.float64)
        if world.shape != (4, 4):
            raise ValueError("path_to_world must hold a 4 x 4 matrix")
    else:
        ref_path = path_to_save_data + "Data_avg.nii.gz"
        ref = nifti.load(ref_path if os.path.exists(ref_path) else path_to_save_data + stems["TWC"] + ".nii.gz").get_fdata()
        if ref.shape != shape:
            raise ValueError("the reference volume does not lie on the grid of the maps")
        world = register_filter(ref, affine, template, tpl.affine, **dict(register or {}))
        if nonlinear is not None:
            disp = warp_register_filter(ref, affine, template, tpl.affine, world, **(nonlinear if isinstance(nonlinear, dict) else {}))["disp"]
    out = maps_to_template_filter(res, affine, template.shape, tpl.affine, world=world, disp=disp, order=order, n_iter=n_iter)
    out["world"], out["disp"] = world, disp
    for key in STAT_QUANTITIES:
        nifti.save(nifti.NiftiImage(out[key], tpl.affine), path_to_save_data + stems[key] + "_in_template.nii.gz")
    nifti.save(nifti.NiftiImage(out["inside"], tpl.affine), path_to_save_data + "maps_to_template_inside.nii.gz")
    lines = ["maps to template: %s" % ("the inverse of the world matrix alone, no field" if disp is None else "%d fixed-point steps" % len(out["residual"]))]
    if disp is not None:
        nifti.save(nifti.NiftiImage(out["inverse_disp"], tpl.affine), path_to_save_data + "maps_to_template_warp.nii.gz")
        nifti.save(nifti.NiftiImage(out["jacobian"], affine), path_to_save_data + "template_to_maps_jacobian.nii.gz")
        lines += ["step %d: residual %.6e voxels" % (k + 1, r) for k, r in enumerate(out["residual"])]
        n_vox = int(np.prod(shape))
        lines += ["Jacobian determinant of the field on the maps' grid: %d of %d voxels not positive (%.4f %%)"
                  % (out["n_nonpositive"], n_vox, 100.0 * out["n_nonpositive"] / n_vox),
                  "Jacobian determinant: min %.6e, max %.6e" % (np.nanmin(out["jacobian"]), np.nanmax(out["jacobian"]))]
    with open(path_to_save_data + "maps_to_template_report.txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    return out


def motor_group_stats(paths_to_save_data, quantity, X, c, path_to_out, path_to_mask=None, f_contrast=None, variance_smoothing_mm=None, **options):
    """Voxel-wise group statistics of one map over several subjects, after motor_maps_to_template brought every subject's maps onto one
    template grid.  paths_to_save_data: one path_to_save_data per subject, in the order of the rows of the design X [n, p]; `quantity`: one of
    STAT_QUANTITIES; c: the t-contrast.  Every subject's <stem>_in_template.nii.gz is loaded; differing shapes or affines are refused.  The
    test runs on the intersection of the subjects' maps_to_template_inside.nii.gz and, where given, the mask at path_to_mask (non-zero voxels,
    on the same grid).  options: group_stats_filter's (n_perm, seed, exchange, two_sided, device, batch_stat; tfce, cluster_threshold,
    cluster_mass_threshold, cluster_connectivity, batch_spatial, work_bytes).
    Written at path_to_out with the template's affine: <quantity>_tstat.nii.gz, <quantity>_cope.nii.gz, <quantity>_p_unc.nii.gz and
    <quantity>_p_fwe.nii.gz; <quantity>_max_dist.txt (the maximum statistic of every permutation, the identity first) and
    <quantity>_group_report.txt: n, dof, the number of permutations, whether the set was exhaustive, t_crit (the 0.95 quantile of the maximum
    statistic) and the number of voxels with p_fwe <= 0.05.  The p-value files hold p itself, NOT FSL randomise's 1 - p: small is significant,
    and no value is below 1 / n_perm.  Parity with FSL randomise is unpinned.
    With tfce=True | dict(E, H, dh, connectivity) (one-sided): also <quantity>_tfce.nii.gz, <quantity>_p_tfce_unc.nii.gz,
    <quantity>_p_tfce_fwe.nii.gz and <quantity>_tfce_max_dist.txt, and in the report dh, E, H, the connectivity, tfce_crit and the number of
    voxels with p_tfce_fwe <= 0.05.  With cluster_threshold=h (cluster_connectivity=26): <quantity>_cluster_extent.nii.gz and
    <quantity>_p_cluster_fwe.nii.gz, and their line in the report.  With cluster_mass_threshold=h (the same cluster_connectivity):
    <quantity>_cluster_mass.nii.gz, <quantity>_p_mass_fwe.nii.gz and <quantity>_mass_max_dist.txt, and a line with the threshold, the
    connectivity, mass_crit and the number of voxels with p_mass_fwe <= 0.05 (the mass is the fixed-point sum group.py describes).  Parity
    with randomise -T / -c / -C / -S is unpinned as well.
    f_contrast [s, p] with c = None: the F-test of its rows at once.  Written then: <quantity>_fstat.nii.gz, <quantity>_p_unc.nii.gz,
    <quantity>_p_fwe.nii.gz, <quantity>_max_dist.txt, the TFCE / cluster files under the names above (taken on F), and the report with s, the
    degrees of freedom (s, n - r), f_crit and the counts at p <= 0.05; no _tstat and no _cope file.  Parity with randomise -f is unpinned.
    variance_smoothing_mm = sigma in mm (randomise -v): the variance is smoothed with a Gaussian of sigma / (the voxel size along the axis)
    voxels per axis, the voxel sizes being the norms of the columns of the template's affine.  The same files are written; <quantity>_tstat
    then holds the pseudo-t, every p-value is taken on it, and the report gains sigma in mm and in voxels, the radii and a line that says so.
    Parity with randomise -v is unpinned.
    -> the dict of group_stats_filter."""
    from . import nifti
    if quantity not in STAT_QUANTITIES:
        raise ValueError("quantity must be one of %s" % (STAT_QUANTITIES,))
    paths = list(paths_to_save_data)
    if len(paths) != np.shape(X)[0]:
        raise ValueError("the design has %d rows for %d subjects" % (np.shape(X)[0], len(paths)))
    stem = {key: st for key, st, _, _, _ in _OUTPUT_FILES}[quantity]
    vols, inside, affine = [], None, None
    for path in paths:
        img = nifti.load(path + stem + "_in_template.nii.gz")
        ins = nifti.load(path + "maps_to_template_inside.nii.gz")
        vol = img.get_fdata()
        if affine is None:
            affine = img.affine
        if vol.ndim != 3 or (vols and vol.shape != vols[0].shape) or not np.allclose(img.affine, affine, rtol=0.0, atol=1e-6):
            raise ValueError("%s does not lie on the template grid of the first subject: run motor_maps_to_template with one template" % path)
        m = ins.get_fdata() != 0
        if m.shape != vol.shape:
            raise ValueError("maps_to_template_inside at %s does not lie on the grid of its maps" % path)
        inside = m if inside is None else inside & m
        vols.append(vol)
    if path_to_mask is not None:
        m = nifti.load(path_to_mask).get_fdata() != 0
        if m.shape != inside.shape:
            raise ValueError("the mask does not lie on the template grid")
        inside = inside & m
    if variance_smoothing_mm is not None:
        if not np.isfinite(variance_smoothing_mm) or variance_smoothing_mm < 0:
            raise ValueError("variance_smoothing_mm must be a finite sigma >= 0 in mm")
        voxel_mm = np.sqrt(np.sum(np.asarray(affine, dtype=np.float64)[:3, :3] ** 2, axis=0))
        options = dict(options, variance_smoothing=tuple(float(variance_smoothing_mm) / voxel_mm))
    out = group_stats_filter(np.stack(vols), X, c, mask=inside, f_contrast=f_contrast, **options)
    files = (("tstat", "tstat"), ("cope", "cope")) if f_contrast is None else (("fstat", "fstat"),)
    for key, name in files + (("p_uncorrected", "p_unc"), ("p_fwe", "p_fwe")):
        nifti.save(nifti.NiftiImage(out[key], affine), path_to_out + quantity + "_" + name + ".nii.gz")
    np.savetxt(path_to_out + quantity + "_max_dist.txt", out["max_dist"])
    n = len(paths)
    if f_contrast is None:
        head = ["group statistics of %s: n = %d subjects, dof = %d" % (quantity, n, out["dof"])]
        crit = "t_crit (0.95 quantile of the maximum statistic): %.6f" % out["t_crit"]
    else:
        head = ["group statistics of %s: n = %d subjects, F-contrast of s = %d rows, dof = (%d, %d)" % ((quantity, n, out["dof"][0]) + out["dof"])]
        crit = "f_crit (0.95 quantile of the maximum statistic): %.6f" % out["f_crit"]
    lines = head + ["permutations: %d (%s)" % (out["n_perm"], "exhaustive" if out["exhaustive"] else "drawn at random"),
                    "voxels tested: %d" % int(out["mask"].sum()), crit,
                    "voxels with p_fwe <= 0.05: %d" % int(((out["p_fwe"] <= 0.05) & out["mask"]).sum())]
    if "variance_smoothing" in out:
        v = out["variance_smoothing"]
        lines += ["variance smoothing: sigma = %.6g mm = (%.6g, %.6g, %.6g) voxels, radius = (%d, %d, %d) voxels" %
                  ((float(variance_smoothing_mm),) + tuple(v["sigma_vox"]) + tuple(v["radius"])),
                  "%s_tstat holds the pseudo-t (cope / sqrt(smoothed variance)); every p-value and critical value is taken on it" % quantity]
    if "tfce" in out:
        for key, name in (("tfce", "tfce"), ("p_tfce_uncorrected", "p_tfce_unc"), ("p_tfce_fwe", "p_tfce_fwe")):
            nifti.save(nifti.NiftiImage(out[key], affine), path_to_out + quantity + "_" + name + ".nii.gz")
        np.savetxt(path_to_out + quantity + "_tfce_max_dist.txt", out["tfce_max_dist"])
        o = out["tfce_options"]
        lines += ["tfce: dh = %.6g, E = %g, H = %g, connectivity = %d" % (out["dh"], o["E"], o["H"], o["connectivity"]),
                  "tfce_crit (0.95 quantile of the maximum TFCE): %.6f" % out["tfce_crit"],
                  "voxels with p_tfce_fwe <= 0.05: %d" % int(((out["p_tfce_fwe"] <= 0.05) & out["mask"]).sum())]
    if "cluster_extent" in out:
        for key, name in (("cluster_extent", "cluster_extent"), ("p_cluster_fwe", "p_cluster_fwe")):
            nifti.save(nifti.NiftiImage(out[key], affine), path_to_out + quantity + "_" + name + ".nii.gz")
        lines += ["cluster extent: threshold = %.6g, connectivity = %d, cluster_crit (0.95 quantile of the maximum extent): %.6f, "
                  "voxels with p_cluster_fwe <= 0.05: %d" % (out["cluster_threshold"], out["cluster_connectivity"], out["cluster_crit"],
                                                            int(((out["p_cluster_fwe"] <= 0.05) & out["mask"]).sum()))]
    if "cluster_mass" in out:
        for key, name in (("cluster_mass", "cluster_mass"), ("p_mass_fwe", "p_mass_fwe")):
            nifti.save(nifti.NiftiImage(out[key], affine), path_to_out + quantity + "_" + name + ".nii.gz")
        np.savetxt(path_to_out + quantity + "_mass_max_dist.txt", out["mass_max_dist"])
        lines += ["cluster mass: threshold = %.6g, connectivity = %d, mass_crit (0.95 quantile of the maximum mass): %.6f, "
                  "voxels with p_mass_fwe <= 0.05: %d" % (out["cluster_mass_threshold"], out["cluster_connectivity"], out["mass_crit"],
                                                         int(((out["p_mass_fwe"] <= 0.05) & out["mask"]).sum()))]
    with open(path_to_out + quantity + "_group_report.txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    return out


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
    if degibbs not in ("no", "yes", "3d"):
        raise ValueError("degibbs must be 'no', 'yes' or '3d'")
    dev = torch.device("cuda", device)
    data = _degibbs_first(data, degibbs, device)
    dd, mk = _prepare_volume(data, mask, dev, False, denoise)
    dd_fa = gaussian_smooth(dd, 2.0) if FA_smooth == "yes" else dd
    proto = _protocol("X2", FA_method, TE_array, TR)
    Laplac = penalty_matrix(reg_matrix, proto.Npc, proto.T2s)
    plan = _fine_plan(proto, nt, device, myelin_T2, penalty=False)
    try:
        fa_vol = _estimate_fa(plan, dd_fa, mk > 0, FA_method, None, proto.T2s, proto.T1s, proto.tau, proto.TR, proto.alpha_values, device)
        present = np.intersect1d(labels_all, np.unique(rois))
        if present.size != labels_all.size:
            raise ValueError("array must not contain infs or NaNs")  # a label without voxels inside the mask: 0/0 kernel (see docstring)
        res = recon_met2_rois(dd, torch.as_tensor(rois, device=dev), fa_vol, None, proto.T2s, Laplac, factor=1.01, myelin_T2=myelin_T2,
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
