"""ctypes binding of include/met2_hip.h.  There is no CPU fallback: if the HIP library is
missing or no MI355X is visible, every product entry point raises."""
import ctypes as C
import os

from . import _build

_LIB = None

_dp = C.POINTER(C.c_double)


class Met2Error(RuntimeError):
    pass


class Options(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("x2_factor", C.c_double), ("t2sparc_lambda", C.c_double),
                ("brent_xtol", C.c_double), ("brent_maxfun", C.c_int32), ("reserved0", C.c_int32), ("t2_myelin_cut", C.c_double),
                ("t2_ie_cut", C.c_double), ("x2_lo", C.c_double), ("x2_hi", C.c_double), ("gcv_lo", C.c_double), ("gcv_hi", C.c_double),
                ("bayes_lo", C.c_double), ("bayes_hi", C.c_double)]


class SynthParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved0", C.c_int32), ("te", C.c_double), ("TR", C.c_double), ("T1", C.c_double)] + [
        (k, C.c_double) for k in ("mwf_lo", "mwf_hi", "t2m_lo", "t2m_hi", "t2ie_lo", "t2ie_hi", "fa_lo", "fa_hi", "snr_lo", "snr_hi", "sm_lo", "sm_hi",
                                  "sie_lo", "sie_hi", "km")]


class TvGeometry(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("oy", "step1", "step2", "xlen", "nt1", "nt2", "nseg", "ntiles", "c0", "c1", "c2", "sigma_cap")] + [("nc", C.c_int64)]


# every symbol include/met2_hip.h declares
SYMBOLS = ["met2_default_options", "met2_abi_version", "met2_device_count", "met2_last_error", "met2_plan_create",
           "met2_plan_destroy", "met2_plan_set_options", "met2_plan_get_options", "met2_plan_build_dictionary_epg", "met2_plan_build_dictionary_epg_profile", "met2_plan_set_dictionary", "met2_plan_get_dictionary",
           "met2_plan_set_penalty", "met2_plan_set_penalty_dense", "met2_plan_get_penalty", "met2_plan_set_lambda_grid",
           "met2_plan_set_t2_grid", "met2_fit", "met2_fit_strided", "met2_fit_enqueue_strided", "met2_plan_finish", "met2_fa_bruteforce", "met2_fa_bruteforce_strided", "met2_fa_spline_select",
           "met2_fa_spline_select_strided", "met2_roi_reduce", "met2_nesma", "met2_tv_work_bytes", "met2_tv_chambolle", "met2_tv_last_timing", "met2_tv_launch_info", "met2_tv_detail", "met2_tv_sigma", "met2_smooth_separable", "met2_metrics", "met2_plan_last_kernel_ms", "met2_plan_last_second_pass_ms", "met2_plan_last_spill_count",
           "met2_plan_launch_info", "met2_plan_gcv_form", "met2_plan_get_shape", "met2_fit_host", "met2_plan_attach_fa_spline", "met2_host_trim",
           "met2_fit_bootstrap", "met2_fit_bootstrap_fa", "met2_bootstrap_replicates", "met2_bootstrap_series_stats", "met2_bootstrap_spectrum_stats",
           "met2_bootstrap_spec_launch_info", "met2_synth_two_lobe", "met2_eval_voxel_metrics", "met2_eval_reduce", "met2_refac_packed_calls", "met2_mppca", "met2_mppca_stages", "met2_mppca_box", "met2_mppca_box_work_bytes", "met2_degibbs", "met2_bias_field",
           "met2_bias_weights", "met2_bias_domain", "met2_bias_init", "met2_bias_em", "met2_bias_smooth", "met2_bias_update", "met2_bias_apply",
           "met2_gibbs_table_cols", "met2_gibbs_tables", "met2_gibbs_split", "met2_gibbs_lines", "met2_degibbs3d", "met2_gibbs_split3d",
           "met2_brain_mask", "met2_bet_stats", "met2_bet_evolve", "met2_bet_fill", "met2_bet_mesh", "met2_bet_mean",
           "met2_tissue_segment", "met2_seg_consts", "met2_seg_init", "met2_seg_icm", "met2_seg_posterior", "met2_seg_finish",
           "met2_partial_volume", "met2_pve_moments", "met2_pve_consts", "met2_pve_energy", "met2_pve_icm", "met2_pve_finish",
           "met2_label_stats_limits", "met2_label_index", "met2_label_moments", "met2_label_quantiles", "met2_label_stats",
           "met2_rician_bias", "met2_rician_step", "met2_rician_invert", "met2_noise_sigma", "met2_fit_rician",
           "met2_resample", "met2_resample_work_bytes", "met2_resample_labels", "met2_resample_prefilter",
           "met2_register_limits", "met2_register_work_bytes", "met2_register_index", "met2_register_cost",
           "met2_register_joint_work_bytes", "met2_register_joint_cost",
           "met2_warp", "met2_warp_labels", "met2_warp_compose", "met2_warp_max_norm2", "met2_warp_work_bytes", "met2_warp_lncc_sums",
           "met2_warp_lncc_force", "met2_warp_lncc", "met2_warp_invert_step", "met2_warp_jacobian",
           "met2_group_limits", "met2_group_perm_stats", "met2_group_perm_fstats",
           "met2_tfce_limits", "met2_tfce_work_bytes", "met2_tfce", "met2_group_perm_tfce", "met2_group_perm_ftfce",
           "met2_group_vsm_limits", "met2_group_vsm_work_bytes", "met2_masked_smooth", "met2_group_perm_vsm"]


def lib():
    global _LIB
    if _LIB is None:
        path = _build.LIB
        if not os.path.exists(path):
            raise Met2Error("HIP extension %s is not built (run __graft_entry__.build()); there is no CPU fallback" % path)
        L = C.CDLL(path)
        L.met2_last_error.restype = C.c_char_p
        vp = C.c_void_p
        L.met2_plan_create.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, C.c_int32, C.POINTER(Options)]
        L.met2_plan_destroy.argtypes = [vp]
        L.met2_plan_set_options.argtypes = [vp, C.POINTER(Options)]
        L.met2_plan_get_options.argtypes = [vp, C.POINTER(Options)]
        L.met2_plan_build_dictionary_epg.argtypes = [vp, _dp, _dp, C.c_double, _dp, C.c_double, vp]
        L.met2_plan_build_dictionary_epg_profile.argtypes = [vp, _dp, _dp, C.c_double, _dp, C.c_double, C.c_int32, _dp, _dp, _dp, vp]
        L.met2_plan_set_dictionary.argtypes = [vp, _dp]
        L.met2_plan_get_dictionary.argtypes = [vp, _dp]
        L.met2_plan_set_penalty.argtypes = [vp, C.c_int32, _dp]
        L.met2_plan_set_penalty_dense.argtypes = [vp, _dp]
        L.met2_plan_get_penalty.argtypes = [vp, _dp]
        L.met2_plan_set_lambda_grid.argtypes = [vp, _dp, C.c_int32]
        L.met2_plan_set_t2_grid.argtypes = [vp, _dp]
        L.met2_fit.argtypes = [vp, C.c_int32, C.c_int64] + [vp] * 10
        L.met2_fit_strided.argtypes = [vp, C.c_int32, C.c_int64, vp, C.c_int64, C.c_int64] + [vp] * 9
        L.met2_fit_enqueue_strided.argtypes = [vp, C.c_int32, C.c_int64, vp, C.c_int64, C.c_int64] + [vp] * 9
        L.met2_plan_finish.argtypes = [vp, vp]
        L.met2_fa_bruteforce.argtypes = [vp, C.c_int64] + [vp] * 6
        L.met2_fa_bruteforce_strided.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int64] + [vp] * 5
        L.met2_fa_spline_select_strided.argtypes = [C.c_int32, C.c_int64, C.c_int32, _dp, vp, C.c_int32, _dp, C.c_int32, vp, C.c_int64, C.c_int64,
                                                    vp, vp, vp, vp]
        L.met2_roi_reduce.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp]
        L.met2_fa_spline_select.argtypes = [C.c_int32, C.c_int64, C.c_int32, _dp, vp, C.c_int32, _dp, C.c_int32, vp, vp, vp, vp, vp]
        L.met2_nesma.argtypes = [C.c_int32] * 5 + [vp] * 4
        L.met2_mppca.argtypes = [C.c_int32] * 5 + [vp, vp, C.c_int32, vp, vp, vp, vp]
        L.met2_mppca_stages.argtypes = [C.c_int32] * 5 + [vp, vp, C.c_int32, vp, vp, vp, C.c_int32] + [vp] * 7
        L.met2_mppca_box.argtypes = [C.c_int32] * 5 + [vp, vp, C.POINTER(C.c_int32), C.c_int32, C.c_int64] + [vp] * 6
        L.met2_mppca_box_work_bytes.argtypes = [C.c_int32] * 4 + [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.met2_degibbs.argtypes = [C.c_int32] * 5 + [vp] + [C.c_int32] * 3 + [vp, vp, vp, vp]
        L.met2_gibbs_table_cols.argtypes = [C.c_int32]
        L.met2_gibbs_table_cols.restype = C.c_int32
        L.met2_gibbs_tables.argtypes = [C.c_int32] * 3 + [vp, vp, vp]
        L.met2_gibbs_split.argtypes = [C.c_int32] * 5 + [vp, vp, vp, vp]
        L.met2_gibbs_lines.argtypes = [C.c_int32] * 3 + [vp] + [C.c_int32] * 3 + [vp, vp, vp, vp]
        L.met2_degibbs3d.argtypes = [C.c_int32] * 5 + [vp] + [C.c_int32] * 3 + [vp, vp, vp, vp, vp]
        L.met2_gibbs_split3d.argtypes = [C.c_int32] * 5 + [vp, vp, vp, vp, vp]
        L.met2_bias_field.argtypes = [C.c_int32] * 4 + [vp, vp, _dp] + [C.c_int32] * 3 + [C.c_double, vp, vp, vp, vp]
        L.met2_bias_weights.argtypes = [C.c_double, _dp, C.POINTER(C.c_int32), _dp]
        L.met2_bias_domain.argtypes = [C.c_int32] * 4 + [vp, vp, vp, vp, C.POINTER(C.c_int64), vp]
        L.met2_bias_init.argtypes = [C.c_int32, C.c_int64, vp, vp, C.c_int64, C.c_int32, _dp, C.POINTER(C.c_uint32), _dp, _dp, vp]
        L.met2_bias_em.argtypes = [C.c_int32, C.c_int64, vp, vp, vp, C.c_int64, C.c_int32, _dp, C.c_int32, _dp, _dp, vp, vp]
        L.met2_bias_smooth.argtypes = [C.c_int32] * 4 + [vp, C.POINTER(C.c_int32), _dp, C.c_int32, vp, vp]
        L.met2_bias_update.argtypes = [C.c_int32, C.c_int64, vp, vp, vp, C.c_int64, _dp, vp]
        L.met2_bias_apply.argtypes = [C.c_int32, C.c_int64, vp, vp, vp, vp, vp]
        L.met2_brain_mask.argtypes = [C.c_int32] * 4 + [vp, _dp, C.c_double, C.c_int32, C.c_int32, vp, vp, _dp, vp]
        L.met2_bet_stats.argtypes = [C.c_int32] * 4 + [vp, _dp, _dp, C.POINTER(C.c_int64), vp]
        L.met2_bet_evolve.argtypes = [C.c_int32] * 4 + [vp, _dp, _dp, C.c_double, C.c_int32, C.c_int32, vp, vp, vp]
        L.met2_bet_fill.argtypes = [C.c_int32] * 4 + [_dp, C.c_int32, vp, C.c_int32, vp, vp, vp]
        L.met2_bet_mesh.argtypes = [C.c_int32, _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.met2_bet_mean.argtypes = [C.c_int32, C.c_int64, C.c_int32, vp, vp, vp]
        L.met2_tissue_segment.argtypes = [C.c_int32] * 4 + [vp, vp, _dp, C.c_int32, C.c_double] + [C.c_int32] * 3 + [vp, vp, vp, vp]
        L.met2_seg_consts.argtypes = [C.c_int32, C.c_int32, _dp, _dp, _dp, C.POINTER(C.c_int32), vp]
        L.met2_seg_init.argtypes = [C.c_int32, C.c_int64, vp, vp, C.c_int64, C.c_int32, _dp, vp, vp]
        L.met2_seg_icm.argtypes = [C.c_int32] * 4 + [vp, vp, C.c_int32, _dp, _dp, C.c_double, C.c_int32, C.c_int32, vp]
        L.met2_seg_posterior.argtypes = [C.c_int32] * 4 + [vp, vp, vp, C.c_int64, C.c_int32, _dp, _dp, C.c_double, vp, _dp, vp]
        L.met2_seg_finish.argtypes = [C.c_int32, C.c_int64, vp, vp, C.c_int32, _dp, vp, vp, _dp, vp]
        L.met2_partial_volume.argtypes = [C.c_int32] * 4 + [vp, vp, vp, _dp, C.c_int32, C.c_double, C.c_int32, vp, vp, vp, vp, vp]
        L.met2_pve_moments.argtypes = [C.c_int32, C.c_int64, vp, vp, vp, C.c_int32, C.POINTER(C.c_int64), _dp, _dp, vp]
        L.met2_pve_consts.argtypes = [C.c_int32, C.c_int32, _dp, _dp, _dp, C.POINTER(C.c_int32), _dp, vp]
        L.met2_pve_energy.argtypes = [C.c_int32, C.c_int64, vp, vp, C.c_int32, _dp, vp, vp, vp]
        L.met2_pve_icm.argtypes = [C.c_int32] * 4 + [vp, vp, C.c_int32, C.POINTER(C.c_int32), _dp, C.c_double, C.c_int32, C.c_int32, vp]
        L.met2_pve_finish.argtypes = [C.c_int32, C.c_int64, vp, vp, C.c_int32, _dp, vp, vp, vp, vp]
        L.met2_label_stats_limits.argtypes = [C.POINTER(C.c_int32)] * 5
        L.met2_label_index.argtypes = [C.c_int32, C.c_int64, vp, C.c_int32, vp, vp, vp]
        L.met2_label_moments.argtypes = [C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, C.c_int64, C.c_int64, vp, vp]
        L.met2_label_quantiles.argtypes = [C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, C.c_int64, C.c_int64, C.c_int32, _dp, vp, vp]
        L.met2_label_stats.argtypes = [C.c_int32, C.c_int64, vp, C.c_int32, C.c_int32, vp, C.c_int64, C.c_int64, C.c_int32, _dp, vp, vp]
        L.met2_tv_work_bytes.argtypes = [C.c_int32] * 5
        L.met2_tv_work_bytes.restype = C.c_int64
        L.met2_tv_chambolle.argtypes = [C.c_int32] * 5 + [vp, C.c_int32, _dp, C.c_double, C.c_double, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int64, vp]
        L.met2_tv_last_timing.argtypes = [_dp, C.POINTER(C.c_int32)]
        L.met2_tv_launch_info.argtypes = [C.c_int32] * 5 + [C.POINTER(TvGeometry)]
        L.met2_tv_detail.argtypes = [C.c_int32] * 5 + [vp, C.c_int32, vp, vp]
        L.met2_tv_sigma.argtypes = [C.c_int32, C.c_int32, C.c_int64, vp, _dp, C.c_double, vp, vp, vp, vp]
        L.met2_smooth_separable.argtypes = [C.c_int32] * 6 + [_dp] + [vp] * 4
        L.met2_metrics.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
        L.met2_plan_last_kernel_ms.argtypes = [vp, _dp]
        L.met2_plan_last_second_pass_ms.argtypes = [vp, _dp]
        L.met2_plan_last_spill_count.argtypes = [vp, C.POINTER(C.c_int64)]
        L.met2_plan_gcv_form.argtypes = [vp, C.POINTER(C.c_int32), _dp]
        L.met2_refac_packed_calls.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int32]
        L.met2_plan_launch_info.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.met2_plan_get_shape.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.met2_fit_host.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, C.c_int64, vp, vp, C.c_int64, C.c_int64, vp, vp, vp, C.c_int32] + [vp] * 8 + [C.c_int64, _dp]
        L.met2_host_trim.argtypes = []
        L.met2_plan_attach_fa_spline.argtypes = [vp, vp, C.c_int32, _dp, C.c_int32, _dp]
        L.met2_fit_bootstrap.argtypes = [vp, C.c_int32, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, C.c_int32, C.c_int64] + [vp] * 10
        L.met2_fit_bootstrap_fa.argtypes = [vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, C.c_int32, C.c_int64] + [vp] * 11
        L.met2_bootstrap_replicates.argtypes = [vp, C.c_int64, vp, vp, vp, C.c_int32, C.c_int64, vp, vp]
        L.met2_bootstrap_series_stats.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.met2_bootstrap_spectrum_stats.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.met2_bootstrap_spec_launch_info.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        L.met2_rician_bias.argtypes = [C.c_int32, C.c_int64, vp, vp, vp, vp]
        L.met2_rician_step.argtypes = [C.c_int32, C.c_int64, C.c_int32, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp]
        L.met2_rician_invert.argtypes = [C.c_int32, C.c_int64, C.c_int32, vp, C.c_int64, C.c_int64, vp, vp, vp, vp]
        L.met2_noise_sigma.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp]
        L.met2_fit_rician.argtypes = [vp, C.c_int32, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, vp, C.c_int32] + [vp] * 9
        i3 = C.POINTER(C.c_int32)
        L.met2_resample.argtypes = [C.c_int32, C.c_int32, i3, C.c_int32, vp, C.c_int64, C.c_int64, i3, _dp, C.c_double, vp, C.c_int64, C.c_int64, vp, C.c_int64, vp]
        L.met2_resample_work_bytes.argtypes = [C.c_int32, i3, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.met2_resample_labels.argtypes = [C.c_int32, i3, vp, i3, _dp, C.c_int32, vp, vp, vp]
        L.met2_resample_prefilter.argtypes = [C.c_int32, i3, C.c_int32, vp, C.c_int64, C.c_int64, vp, vp]
        L.met2_register_limits.argtypes = [i3] * 4 + [_dp]
        L.met2_register_work_bytes.argtypes = [i3, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.met2_register_index.argtypes = [C.c_int32, i3, vp, C.c_int32, vp, C.c_int64, vp]
        L.met2_register_cost.argtypes = [C.c_int32, C.c_int32, i3, C.c_int32, vp, vp, _dp, i3, vp, _dp, C.c_int32, _dp, C.c_double, vp, C.c_int64, vp, vp, vp]
        L.met2_register_joint_work_bytes.argtypes = [i3, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.met2_register_joint_cost.argtypes = [C.c_int32, C.c_int32, i3, C.c_int32, vp, i3, vp, _dp, C.c_int32, C.c_int32, _dp, C.c_double, vp, C.c_int64, vp, vp, vp, vp]
        L.met2_warp.argtypes = [C.c_int32, C.c_int32, i3, C.c_int32, vp, C.c_int64, C.c_int64, i3, _dp, vp, C.c_double, vp, C.c_int64, C.c_int64, vp, vp]
        L.met2_warp_labels.argtypes = [C.c_int32, i3, vp, i3, _dp, vp, C.c_int32, vp, vp, vp]
        L.met2_warp_compose.argtypes = [C.c_int32, i3, vp, i3, _dp, _dp, vp, C.c_double, vp, vp, vp]
        L.met2_warp_max_norm2.argtypes = [C.c_int32, C.c_int64, vp, vp, vp]
        L.met2_warp_work_bytes.argtypes = [i3, C.POINTER(C.c_int64)]
        L.met2_warp_lncc_sums.argtypes = [C.c_int32, i3, vp, vp, vp, C.c_int32, vp, vp, C.c_int64, vp]
        L.met2_warp_lncc_force.argtypes = [C.c_int32, i3, vp, vp, vp, vp, C.c_double, vp, vp, vp, C.c_int64, vp]
        L.met2_warp_lncc.argtypes = [C.c_int32, i3, vp, vp, vp, C.c_int32, C.c_double, vp, vp, vp, C.c_int64, vp]
        L.met2_warp_invert_step.argtypes = [C.c_int32, i3, vp, i3, _dp, _dp, vp, vp, vp, vp, vp]
        L.met2_warp_jacobian.argtypes = [C.c_int32, i3, vp, C.c_double, vp, vp, vp]
        L.met2_group_limits.argtypes = [i3] * 4
        L.met2_group_perm_stats.argtypes = [C.c_int32, C.c_int32, C.c_int64, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp]
        L.met2_tfce_limits.argtypes = [i3] * 2
        L.met2_tfce_work_bytes.argtypes = [C.c_int32, i3, C.c_int64, C.POINTER(C.c_int64)]
        L.met2_tfce.argtypes = [C.c_int32, C.c_int32, i3, vp, vp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, vp, vp, vp, C.c_int64, vp]
        L.met2_group_perm_tfce.argtypes = [C.c_int32, C.c_int32, C.c_int64, vp, vp, C.c_int32, C.c_int32, vp, i3, vp, C.c_int32, C.c_double, C.c_double,
                                           C.c_double, C.c_int32, vp, vp, vp, vp, vp, C.c_int64, vp]
        L.met2_group_perm_fstats.argtypes = [C.c_int32, C.c_int32, C.c_int64, vp, vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, vp, vp, vp, vp, vp, vp]
        L.met2_group_perm_ftfce.argtypes = [C.c_int32, C.c_int32, C.c_int64, vp, vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, vp, i3, vp, C.c_int32,
                                            C.c_double, C.c_double, C.c_double, C.c_int32, vp, vp, vp, vp, vp, C.c_int64, vp]
        L.met2_group_vsm_limits.argtypes = [i3] * 4
        L.met2_group_vsm_work_bytes.argtypes = [C.c_int32, i3, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.met2_masked_smooth.argtypes = [C.c_int32, C.c_int32, i3, vp, vp, i3, _dp, _dp, _dp, vp, vp, vp, C.c_int64, vp]
        L.met2_group_perm_vsm.argtypes = [C.c_int32, C.c_int32, C.c_int64, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, i3, vp, C.c_int32, C.c_double,
                                          C.c_double, C.c_double, C.c_int32, i3, _dp, _dp, _dp, vp, vp, vp, vp, vp, C.c_int64, vp]
        L.met2_synth_two_lobe.argtypes = [vp, C.POINTER(SynthParams), C.c_int64, C.c_int64, C.c_int64, vp, vp, vp, vp]
        L.met2_eval_voxel_metrics.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
        L.met2_eval_reduce.argtypes = [C.c_int64, vp, vp, vp, vp, vp, vp]
        _LIB = L
    return _LIB


def check(rc):
    if rc != 0:
        msg = lib().met2_last_error()
        raise Met2Error("met2_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
