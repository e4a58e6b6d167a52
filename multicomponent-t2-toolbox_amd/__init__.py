"""MI355X-native per-voxel regularised-NNLS T2-spectrum solver (drop-in for the hot path of
ejcanalesr/multicomponent-T2-toolbox).  Package layout:

  csrc/                     HIP kernels + the C ABI of include/met2_hip.h
  plan.py                   Met2Plan (ctypes face of the C ABI; torch for device memory only)
  intravoxel_algorithms.py  nnls, nnls_tik, nnls_x2, nnls_lcurve_wrapper, nnls_gcv, BayesReg_nnls
  epg.py                    create_Dic_3D, create_met2_design_matrix_epg; slice_profile / hann_sinc / pulse_profile / pulse_pair_profile: slice-profile-aware
                            dictionaries for 2-D multi-slice data (slice_profile=... of Met2Plan.build_dictionary_epg and the drivers)
  flip_angle_algorithms.py  compute_optimal_FA, fitting_slice_FA_brute_force
  motor.py                  create_Laplacian_matrix, fitting_slice_T2, the drivers: recon_met2_arrays (steps 1-4 on arrays; _resolve_run states what the options
                            refuse and where they run), motor_recon_met2 (the on-disk contract), the ROI mode, motor_atlas_stats, motor_maps_to_template, motor_group_stats; re-exports the filters
  filters.py                the whole-volume filters, one C ABI call each: nesma_filter, mppca_filter (MP-PCA denoising, cubic or box window, optional overlapping-patch averaging: csrc/met2_mppca.hip),
                            gibbs_filter (Gibbs-ringing removal, degibbs='yes' and '3d': csrc/met2_gibbs.hip),
                            bias_field_filter (bias-field correction of the TWC map, bias_correct='yes': csrc/met2_bias.hip),
                            brain_mask_filter (brain extraction, brain_mask='yes': csrc/met2_bet.hip),
                            tissue_segment_filter (tissue segmentation of the TWC map, segment='yes': csrc/met2_seg.hip),
                            partial_volume_filter (partial-volume tissue maps of the TWC map, segment='pve': csrc/met2_pve.hip),
                            label_stats_filter (per-tissue / per-ROI statistics of the maps and spectra, tissue_stats='yes': csrc/met2_stats.hip),
                            resample_filter / resample_labels_filter (affine resampling onto another grid) and atlas_stats_filter (label_stats_filter for an
                            atlas on a grid of its own, with template=... after registering the atlas' template to the maps): csrc/met2_resample.hip,
                            register_filter (rigid / affine registration of two volumes: register.py, csrc/met2_register.hip),
                            warp_register_filter / warp_filter / warp_labels_filter (non-linear registration and resampling through a displacement
                            field; atlas_stats_filter(nonlinear=...)), warp_invert_filter / warp_jacobian_filter / maps_to_template_filter (the
                            inverse of a field by fixed-point iteration, its Jacobian determinant, the maps onto a template's grid): warp.py, csrc/met2_warp.hip,
                            group_stats_filter (voxel-wise group statistics with permutation inference over subjects' maps on one grid: group.py, csrc/met2_group.hip;
                            tfce=... / cluster_threshold=...: TFCE and cluster-extent inference), tfce_filter (the TFCE of one volume: csrc/met2_tfce.hip),
                            gaussian_smooth
  tv.py                     tv_denoise_volume / tv_chambolle: denoise='TV' of the driver through met2_tv_chambolle (csrc/met2_tv.hip)
  gibbs.py                  gibbs_tables / gibbs_split / gibbs_split3d / gibbs_lines: the stages of the Gibbs-ringing filter one by one (tests and diagnostics)
  bet.py                    bet_mean / bet_stats / bet_mesh / bet_evolve / bet_fill: the stages of the brain extraction one by one (tests and diagnostics)
  bias.py                   bias_weights / bias_domain / bias_init / bias_em / bias_smooth / bias_update / bias_apply: the stages of the bias-field correction one by one (tests and diagnostics)
  seg.py                    seg_consts / seg_init / seg_icm / seg_posterior / seg_finish: the stages of the tissue segmentation one by one (tests and diagnostics)
  pve.py                    pve_moments / pve_consts / pve_energy / pve_icm / pve_finish: the stages of the partial-volume maps one by one (tests and diagnostics)
  stats.py                  label_index / label_moments / label_quantiles / label_stats: per-label n, mean, std and np.quantile-exact quantiles of any series (csrc/met2_stats.hip)
  resample.py               resample / resample_labels / prefilter / work_bytes: the affine resampling's entries (csrc/met2_resample.hip), and the transform
                            algebra in numpy: voxel_matrix, invert, from_flirt / to_flirt
  register.py               register: the coarse-to-fine direction-set search for the world matrix that brings a moving volume onto a fixed one, dof 6 / 7 / 9 / 12,
                            cost 'corratio' | 'normcorr' | 'leastsq' | 'mi' | 'nmi' (the last two from a joint histogram sized per level: level_bins); prepare / cost: a batch of candidate transforms scored in one launch (csrc/met2_register.hip);
                            params_to_world / world_to_params, pyramid, the intensity rule
  warp.py                   register: greedy deformable registration with the squared local normalised cross-correlation, coarse to fine, after the world
                            matrix of register.py; warp / warp_labels / compose / max_norm2 / lncc / lncc_sums / lncc_force: its stages one by one (csrc/met2_warp.hip);
                            invert: the inverse field by fixed-point iteration, invert_step / jacobian: its step and the determinant with the count of folded voxels
  group.py                  partition / residualise / permutation_set / weights: a design and a t-contrast as the weight rows of met2_group_perm_stats;
                            perm_stats: the entry on arrays; randomise: the permutation test (uncorrected and FWE-corrected p-values) (csrc/met2_group.hip);
                            tfce / cluster_extent / cluster_mass: the spatial statistics of maps; randomise(tfce=..., cluster_threshold=..., cluster_mass_threshold=...): their permutation test (csrc/met2_tfce.hip)
  rician.py                 bias / step / invert: the kernels of the Rician noise-floor correction one by one (csrc/met2_rician.hip; Met2Plan.fit_rician and
                            noise_sigma, rician='iterative' | 'direct' of the drivers)
  mppca.py                  mppca_stages: the MP-PCA denoiser with what each of its steps leaves (tests and diagnostics)
  nifti.py                  NIfTI-1 reader / writer for the driver's on-disk contract
  dist.py                   one-process-per-GPU voxel sharding + the single gather of output maps
  synth.py                  seeded synthetic volumes (the reference's Monte-Carlo recipe)

There is no CPU fallback: without the built HIP library and a visible GPU every call raises."""
from ._lib import Met2Error  # noqa: F401
from .plan import BOOT_QUANTITIES, BOOT_QUANTITIES_FA, BOOT_STATS, MAP_NAMES, METHODS, PENALTIES, Met2Plan  # noqa: F401


_LAZY = ("gibbs_filter", "bias_field_filter", "brain_mask_filter", "tissue_segment_filter", "partial_volume_filter", "tfce_filter")   # motor's, imported on first use


def __getattr__(name):
    if name in _LAZY:
        from . import motor
        return getattr(motor, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
