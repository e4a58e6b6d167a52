/*
 * met2_hip.h -- C ABI of libmet2_hip.so, the MI355X (gfx950) implementation of the
 * per-voxel regularised-NNLS T2-spectrum path of ejcanalesr/multicomponent-T2-toolbox.
 *
 * The reference has no FFI layer: its boundary is Python function calls inside one
 * process.  Each entry point below names the reference function (or
 * driver code) it replaces; INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add.  Plain pointers and sizes only -- no torch types.
 *
 * Conventions
 *   - all arithmetic is fp64 (fused multiply-adds; the factorisation's reciprocal square roots are v_rsq_f64 plus two
 *     Newton steps, ~1 ulp; the lambda search and its objective use IEEE division and square root);
 *   - "host" pointers are ordinary process memory (small parameter arrays);
 *     "device" pointers are HIP device memory on the plan's device (bulk voxel arrays);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are
 *     asynchronous with respect to the host unless stated otherwise;
 *   - every function returns 0 on success, a negative MET2_E_* code otherwise;
 *     met2_last_error() gives the message of the calling thread's last failure;
 *   - a plan may be used from one host thread at a time and serves one stream at a time (its sort scratch, error word and
 *     timing events are per plan: a fit or met2_plan_finish on another stream while enqueued fits are pending returns
 *     MET2_E_STATE); different plans may be used concurrently, on one device or on several;
 *   - multi-GPU: the library keeps no global state besides the calling thread's error message and
 *     what met2_fit_host parks with a plan, so "one plan per device (met2_options.device), each driven by its own host thread or
 *     process, all at once" works from any host language.  Two drivers are built on it:
 *       met2_fit_host (ABI 5, below)  ONE process, one host thread per plan inside the call, host arrays in and out -- what the
 *                                     reference's single Python process binds; no communicator, the outputs meet in host memory;
 *       dist.py                       one process per GPU under torch.distributed; the path's single collective -- the gather of
 *                                     the outputs to the root -- belongs to the host's communicator (RCCL).
 */
#ifndef MET2_HIP_H
#define MET2_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MET2_ABI_VERSION 6

/* reg_method of motor/motor_recon_met2_real_data.py:134-150 */
enum met2_method {
    MET2_NNLS = 0,      /* algorithms.py:55  nnls                      reg_param = 0      */
    MET2_T2SPARC = 1,   /* algorithms.py:262 nnls_tik, lambda = 1.8    reg_param = 1.8    */
    MET2_X2 = 2,        /* algorithms.py:211 nnls_x2, factor = 1.02    reg_param = k_est  */
    MET2_LCURVE = 3,    /* algorithms.py:88  nnls_lcurve_wrapper + nnls_tik, reg_param = lambda */
    MET2_GCV = 4,       /* algorithms.py:276 nnls_gcv                  reg_param = lambda */
    MET2_BAYESREG = 5   /* bayesian_interpolation.py:84 BayesReg_nnls  reg_param = lambda */
};

/* reg_matrix of motor:254-273 */
enum met2_penalty { MET2_PEN_I = 0, MET2_PEN_L1 = 1, MET2_PEN_L2 = 2, MET2_PEN_INVT2 = 3 };

/* per-voxel status bits written by met2_fit */
enum met2_status {
    MET2_ST_FITTED = 1,        /* passed the gates of motor:124,131 and was solved                 */
    MET2_ST_ITMAX = 2,         /* some inner NNLS hit the 3n iteration cap (reference ignores it)  */
    MET2_ST_NONFINITE = 4,     /* NaN/Inf in the voxel's echoes: outputs zero (reference: ValueError) */
    MET2_ST_CHOLFAIL = 8,      /* BayesReg: Cholesky of beta(B + lambda K) failed (reference: LinAlgError) */
    MET2_ST_BRENT_MAXFUN = 16, /* lambda search stopped on maxfun                                  */
    MET2_ST_KOVERFLOW = 32     /* passive set outgrew the wave's LDS region: set only transiently -- the fit kernel queues such a voxel and
                                  the spill-over kernel launched behind it (in every fit that runs at a reduced capacity) solves it again,
                                  so no voxel returned by met2_fit carries it */
};

enum met2_error {
    MET2_OK = 0,
    MET2_E_INVALID = -1,       /* bad argument (shape, NULL, enum)        */
    MET2_E_UNSUPPORTED = -2,   /* shape/penalty outside the built kernels */
    MET2_E_HIP = -3,           /* a HIP runtime call failed               */
    MET2_E_NODEVICE = -4,      /* no gfx950 device visible                */
    MET2_E_STATE = -5          /* plan not fully configured for this call, or fits pending on another stream */
};

typedef struct met2_plan met2_plan;

/* Constants the reference buries in its driver; defaults = reference values. */
typedef struct met2_options {
    int32_t struct_size;      /* sizeof(met2_options), for ABI growth                      */
    int32_t device;           /* HIP device ordinal                                        */
    double x2_factor;         /* motor:141            1.02                                 */
    double t2sparc_lambda;    /* motor:138            1.8                                  */
    double brent_xtol;        /* algorithms.py:219    1e-5                                 */
    int32_t brent_maxfun;     /* 0 = reference value: 300 (X2, GCV), 200 (BayesReg)        */
    int32_t reserved0;
    double t2_myelin_cut;     /* motor:216 (myelin_T2 CLI flag)   40.0                     */
    double t2_ie_cut;         /* motor:217            200.0                                */
    /* ABI 6: the intervals of the lambda searches (scipy.optimize.fminbound's x1, x2).  A caller that passes a shorter struct (struct_size of
     * ABI <= 5) gets the reference values.  0 <= lo < hi, finite.  The plan-level seeds and BayesReg's factor tables follow them.  */
    double x2_lo, x2_hi;      /* algorithms.py:219              0, 10     (the reference's evaluation scripts search wider grids: :215 of
                                                                          evaluate_all_methods_two_lobes_SNR50_150.py tops at 100)          */
    double gcv_lo, gcv_hi;    /* algorithms.py:280              1e-8, 10  */
    double bayes_lo, bayes_hi;/* bayesian_interpolation.py:101  1e-8, 2   */
} met2_options;

void met2_default_options(met2_options *opt);

int met2_abi_version(void);
int met2_device_count(void);
const char *met2_last_error(void);

/* ---- plan: the shared nTE x nT2 x nFA problem (dictionary, Gram matrices, penalty) ---- */
int met2_plan_create(met2_plan **out, int32_t n_te, int32_t n_t2, int32_t n_fa, const met2_options *opt);
int met2_plan_destroy(met2_plan *plan);
/* change x2_factor / t2sparc_lambda / Brent settings / metric windows of an existing plan
 * (the per-call arguments `factor` of nnls_x2 and `reg_opt` of nnls_tik, algorithms.py:211,262) */
int met2_plan_set_options(met2_plan *plan, const met2_options *opt);
int met2_plan_get_options(met2_plan *plan, met2_options *opt);
/* the shape the plan was created with (any of the three may be NULL) */
int met2_plan_get_shape(met2_plan *plan, int32_t *n_te, int32_t *n_t2, int32_t *n_fa);

/* epg/epg.py:155 create_Dic_3D -- EPG dictionary built on the device, one wave per
 * (T2, flip angle).  T2s/T1s [n_t2], alpha_deg [n_fa] are host arrays.  Also forms the
 * per-flip-angle Gram matrices D^T D used by the solver. */
int met2_plan_build_dictionary_epg(met2_plan *plan, const double *T2s, const double *T1s, double tau,
                                   const double *alpha_deg, double TR, void *stream);

/* The same dictionary for slice-selective pulses (2-D multi-slice multi-echo spin echo; an extension with no counterpart in the
 * reference): the excitation and refocusing angles vary across the slice and the decay is the integral of the echo trains over the slice
 * profile (Lebel & Wilman, Magn Reson Med 64:1005-1014, 2010).  The profile is three host arrays of length n_z, 1 <= n_z <= 64: r_exc[z] and
 * r_ref[z], the excitation and refocusing angles at position z relative to the nominal ones (1.0 at the centre of ideal pulses), and the
 * quadrature weights w[z], used as given (not normalised).  For a = alpha_deg[fa] and bin j, with H_z[e] echo e of the train of the plain
 * entry at alpha = (a * r_ref[z]) * pi/180 and alpha_exc = ((a / 2.0) * r_exc[z]) * pi/180 (operations in this order):
 *     acc = 0;  for z = 0 .. n_z-1 ascending:  acc = acc + (w[z] * H_z[e])       (product and sum rounded separately, no fma)
 *     D[fa][e][j] = acc * (1 - exp(-TR / T1s[j]))
 * The summation order is part of the definition: the result does not depend on the device or the launch.  With n_z = 1 and
 * r_exc = r_ref = w = {1.0} it is the plain entry's dictionary bit for bit, with one exception: an echo that is -0 in the plain
 * dictionary (a negative value that underflowed) comes back as +0, since 0 + (-0) = +0.  The TR factor stays the reference's: a steady state that
 * depends on the local excitation angle is out of scope, as are complex (phase) profiles.  Everything after the dictionary is the plain
 * entry's (Gram matrices, low-rank basis, seeds, T2 grid).  MET2_E_INVALID before any launch, the plan's dictionary untouched, for a NULL
 * pointer, n_z outside 1..64, a profile value that is not finite or negative, and weights that are all zero. */
int met2_plan_build_dictionary_epg_profile(met2_plan *plan, const double *T2s, const double *T1s, double tau, const double *alpha_deg, double TR,
                                           int32_t n_z, const double *r_exc, const double *r_ref, const double *w, void *stream);

/* Dictionary handed in by the caller, reference layout Dic_3D[n_te][n_t2][n_fa] (host).
 * Replaces the `Dic_3D` argument of fitting_slice_T2 (motor:113). */
int met2_plan_set_dictionary(met2_plan *plan, const double *dic3d_host);

/* Copies the dictionary back in the reference layout [n_te][n_t2][n_fa] (host, blocking). */
int met2_plan_get_dictionary(met2_plan *plan, double *dic3d_host);

/* motor:86 create_Laplacian_matrix / motor:263 InvT2.  T2s (host, [n_t2]) is needed for
 * InvT2 only.  The dense form takes any `Laplac` [n_t2][n_t2] (host) whose L^T L has
 * bandwidth <= 2 (true for I, L1, L2, InvT2); wider ones return MET2_E_UNSUPPORTED.
 * The plan-level seeds of the lambda searches are (re)built here and wherever the dictionary changes (these entries block);
 * they are used only if D^T D + lambda L^T L is positive definite (checked for flip angle 0) -- with a penalty whose null
 * space meets the dictionary's the minimiser is not unique and every voxel starts cold, as the reference does. */
int met2_plan_set_penalty(met2_plan *plan, int32_t which, const double *T2s);
int met2_plan_set_penalty_dense(met2_plan *plan, const double *laplac_host);
int met2_plan_get_penalty(met2_plan *plan, double *laplac_host);

/* motor:248-251 lambda_reg (host, [n]); default = the reference's 50-point grid */
int met2_plan_set_lambda_grid(met2_plan *plan, const double *lambda_reg, int32_t n);

/* motor:215-224 T2 grid for the metrics windows (host, [n_t2]); set automatically by
 * met2_plan_build_dictionary_epg */
int met2_plan_set_t2_grid(met2_plan *plan, const double *T2s);

/* ---- hot path ------------------------------------------------------------------------
 * motor:113 fitting_slice_T2 over a flat voxel list, fused with the step-4 metrics of
 * motor:443-472.  All array arguments are DEVICE pointers:
 *   data     [nvox][n_te]  echoes (un-normalised, as the driver passes them)
 *   fa_index [nvox]        float64 index into the dictionary's FA axis (motor:127), NULL = 0
 *   mask     [nvox]        uint8, voxel is fitted iff mask != 0 (motor:124), NULL = all ones
 *   fsol     [nvox][n_t2]  out: x * km                       (motor:154)
 *   sig      [nvox][n_te]  out: Kernel @ x * km              (motor:155), may be NULL
 *   reg      [nvox]        out: reg_param                    (motor:153)
 *   lam      [nvox]        out: the selected lambda (equals reg except for X2, where the driver
 *                               stores k_est in reg_param, motor:141-143), may be NULL
 *   maps     [6][nvox]     out: MWF, IEWF, FWF, T2_M, T2_IE, TWC (motor:455-468), may be NULL
 *   status   [nvox]        out: met2_status bits, may be NULL
 * Gated-out voxels get zeros (motor:115-117) and, if mask != 0, the all-zero-spectrum
 * metrics of motor:448-468. */
int met2_fit(met2_plan *plan, int32_t method, int64_t nvox, const double *data, const double *fa_index,
             const uint8_t *mask, double *fsol, double *sig, double *reg, double *lam, double *maps,
             int32_t *status, void *stream);

/* The same with an explicit layout of `data`: echo e of voxel v is read at data[v * voxel_stride + e * echo_stride]
 * (strides in doubles).  The driver loads its volume with nibabel (motor:167-173), whose arrays are Fortran-ordered:
 * for such an [nx][ny][nz][nt] array voxel_stride = 1 and echo_stride = nx*ny*nz, and voxel v is the voxel at
 * x + nx*(y + ny*z) -- the outputs then come out in that (Fortran) voxel order, i.e. fsol is the Fortran-ordered
 * [nx][ny][nz] volume of spectra.  met2_fit is the special case voxel_stride = n_te, echo_stride = 1.  The classify pass
 * and the solver read every echo exactly once either way; no transposed copy is made. */
int met2_fit_strided(met2_plan *plan, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride,
                     int64_t echo_stride, const double *fa_index, const uint8_t *mask, double *fsol, double *sig, double *reg,
                     double *lam, double *maps, int32_t *status, void *stream);

/* The same without waiting for the GPU: the launches are enqueued on `stream` and the call returns (the blocking entries above
 * wait only to report an FA index outside the dictionary, the reference's IndexError at motor:127-128).  A host pipeline --
 * H2D of the next chunk of a volume, this fit, D2H of the previous chunk's outputs, on separate streams (motor:167-182,
 * :427-503 are that loop in the reference, one image row at a time) -- enqueues chunk after chunk and calls met2_plan_finish
 * once: it waits for `stream` and returns MET2_E_INVALID if any fit enqueued since the last finish saw such an index.
 * One plan serves one stream at a time (its sort scratch is per plan): enqueueing on, or finishing, another stream while fits are pending
 * returns MET2_E_STATE. */
int met2_fit_enqueue_strided(met2_plan *plan, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride,
                             int64_t echo_stride, const double *fa_index, const uint8_t *mask, double *fsol, double *sig,
                             double *reg, double *lam, double *maps, int32_t *status, void *stream);
int met2_plan_finish(met2_plan *plan, void *stream);

/* ---- host to host, one or several devices (ABI 5; run-wise dealing since ABI 6) ----------
 * motor:349-373 + motor:427-472 for a voxel list that lives in HOST memory, as the reference's driver holds it (motor:167-182), from ONE
 * process: what a binding of the reference calls instead of its joblib loop over image rows (motor:427-441) -- numpy arrays in, numpy
 * arrays out, no device memory, stream or communicator on the caller's side.
 *   plans [n_plans]   1..64 distinct plans of one shape, configured alike (dictionary, penalty, options), each on the device of its
 *                     met2_options.device; several plans may share a device.  With several plans the voxel list is dealt in RUNS of
 *                     4 096 voxels, run j -> plan j mod n_plans (interleaved: tissue classes cluster in space and differ 10x in
 *                     iteration count; ABI 6 -- ABI 5 dealt whole blocks), and a plan's DMA block is `chunk`
 *                     voxels of ITS runs, moved by pitched copies; rows with a pitch (echo_stride 1, voxel_stride > n_te) and general
 *                     strides keep whole blocks, block b -> plan b mod n_plans.  Every plan is driven by its own host thread inside
 *                     the call (one plan: the calling thread) through three streams of its device: H2D of its block c + 1 |
 *                     [FA estimation and] fit of block c | D2H of block c - 1.  There is no exchange between devices.  The coarse plans
 *                     of estimate_fa = 2 must be distinct, one per plan, and none of them in plans[].
 *   ALL array arguments are HOST pointers (data and fa_data may ALSO be device pointers: the volume as met2_tv_chambolle / met2_nesma /
 *   met2_smooth_separable left it -- then copied block by block device to device); arrays in pinned memory (hipHostMalloc,
 *   hipHostRegister) are copied from / to in place, pageable ones are staged through pinned block buffers by the plan's thread while its
 *   device works:
 *   data              echo e of voxel v at data[v * voxel_stride + e * echo_stride] (strides in doubles, > 0): [nvox][n_te] rows
 *                     (echo_stride 1) and the Fortran-ordered volume of nibabel (voxel_stride 1, echo_stride nvox) are copied as they
 *                     lie and read in place on the device; any other layout is gathered on the host
 *   fa_data           NULL, or the same voxel list (same layout and strides) as the FA estimation shall see it: the Gaussian-smoothed
 *                     volume of motor:337-343 (FA_smooth='yes', the CLI default); needs estimate_fa != 0
 *   mask_values       NULL, or [nvox] float64: the driver's preparation on the device -- every echo of voxel v is multiplied by
 *                     mask_values[v] and negative values are clipped to 0 (motor:180-182, :279) before anything else sees the block
 *                     (fa_data, when given, is taken as prepared already)
 *   fa_index, mask    [nvox] float64 / uint8 as for met2_fit, NULL = flip angle 0 / all ones
 *   estimate_fa       0: the flip angles are given (fa_index, or angle 0);  fa_index must be NULL otherwise;
 *                     1: brute-force search over the plans' FA axis on every block (met2_fa_bruteforce, fa_estimation.py:74-111);
 *                     2: the spline method (fa_estimation.py:35-70, the CLI default): plain-NNLS residuals on the coarse grid of the
 *                        plan attached with met2_plan_attach_fa_spline, a cubic spline through them, its bounded minimum snapped to the
 *                        plans' own FA axis (met2_fa_bruteforce on the coarse plan + met2_fa_spline_select, per block)
 *   fsol [nvox][n_t2], sig [nvox][n_te], reg, lam [nvox], maps [6][nvox], status [nvox]   as for met2_fit (sig, lam, maps, status may be NULL)
 *   fa_out [nvox]     out, may be NULL: the FA index every voxel was fitted with
 *   fa_gate [nvox]    out, may be NULL: 1.0 where the FA step's gate holds (fa_estimation.py:45: mask and a positive echo sum of what
 *                     the FA step sees), else 0.0 -- the driver reports a flip angle only there (motor:366-370)
 *   chunk             voxels per DMA block (several plans: rounded up to whole runs of 4 096); 0 = a quarter of a plan's share, in multiples of
 *                     4 096, at most 262 144 and (unless the share itself is smaller) at least 65 536
 *   plan_ms [n_plans] out, may be NULL: wall-clock ms every plan's thread spent in the call
 * Blocking.  Every voxel is solved on its own, so the outputs are bit for bit those of one met2_fit over the whole list, whatever
 * n_plans, chunk and the devices (a voxel queued for the spill-over kernel gets the same bits in a short queue and a long one).  Returns the first failing plan's code (an FA index outside the dictionary: MET2_E_INVALID) after
 * ALL plans' streams have drained -- nothing writes to the caller's arrays after the return.  The block buffers (two slots of
 * chunk x ~8 (2 n_te + n_t2 + 10) bytes on the device, the same pinned when a pageable array takes part), three streams and six
 * events stay with each plan until met2_plan_destroy (and then wait for the next plan on that device: met2_host_trim). */
int met2_fit_host(met2_plan *const *plans, int32_t n_plans, int32_t method, int64_t nvox, const double *data, const double *fa_data,
                  int64_t voxel_stride, int64_t echo_stride, const double *mask_values, const double *fa_index, const uint8_t *mask,
                  int32_t estimate_fa, double *fsol, double *sig, double *reg, double *lam, double *maps, int32_t *status, double *fa_out,
                  double *fa_gate, int64_t chunk, double *plan_ms);
/* For estimate_fa = 2: `plan_lr` holds the coarse-grid dictionary (motor:237-238: 15 flip angles from 90 to 180 degrees), same n_te x n_t2
 * and device as `plan`; alpha_lr [n_lr = its flip angles] and alpha_hr [n_hr = the plan's flip angles] are the two grids in degrees (HOST
 * arrays, copied).  plan_lr must outlive the attachment; plan_lr = NULL detaches. */
int met2_plan_attach_fa_spline(met2_plan *plan, met2_plan *plan_lr, int32_t n_lr, const double *alpha_lr, int32_t n_hr, const double *alpha_hr);
/* met2_plan_destroy hands a plan's block buffers of met2_fit_host to the next plan created on the same device (at most two sets per device
 * wait; a driver that builds its plans per call then allocates and pins nothing per call); this frees the waiting ones. */
int met2_host_trim(void);

/* ---- bootstrap uncertainty maps (an extension: the reference has no counterpart) ----------
 * Monte-Carlo noise propagation per voxel.  The point fit is met2_fit_strided's, bit for bit (fsol, sig, reg, lam, maps, status as there; let
 * s_hat = sig[v]).  Then every voxel is refitted on n_rep = B Rician replicates of its fitted signal with the same method, plan, flip angle and
 * mask, and the statistics of the metrics over the replicates are returned.  The ingredients are the reference's:
 *   noise model   Rician at sigma around the signal, scripts_synthetic_data_evaluation/Paper_Comparison/
 *                 evaluate_all_methods_two_lobes_SNR50_150.py:387-391:  M_b[e] = sqrt((s_hat_e + sigma_v z1)^2 + (sigma_v z2)^2)
 *   sigma_v       sigma[v] when `sigma` is given; otherwise the estimate of intravoxel_algorithms/bayesian_interpolation.py:88-93 on the raw
 *                 echoes: a plain-NNLS pass (MET2_NNLS) at the voxel's flip angle gives fsol0, sig0 and
 *                 sigma_v = sqrt(sum_e (M_e - sig0_e)^2 / max(n_te - #{fsol0 > 0}, 1)); returned in sigma_out
 *   replicates    counter-based: (x0, x1, x2, x3) = Philox4x32-10(counter = (e, b, lo32(id_v), hi32(id_v)), key = (lo32(seed), hi32(seed))),
 *                 id_v = voxel_id[v] (NULL: v), u1 = ((x0 >> 5) 2^26 + (x1 >> 6) + 1) 2^-53 in (0, 1], u2 = ((x2 >> 5) 2^26 + (x3 >> 6)) 2^-53,
 *                 r = sqrt(-2 log u1), z1 = r cos(2 pi u2), z2 = r sin(2 pi u2).  A voxel's replicates depend on (seed, id_v, b, e) alone: not
 *                 on chunking, call splitting, voxel order or device.  Any 64-bit seed (its bits are taken as they are)
 *   fits          each replicate as met2_fit fits its echoes, at the voxel's FA index and mask; replicates of a voxel whose point status lacks
 *                 MET2_ST_FITTED are not fitted.  FA is not re-estimated per replicate (met2_fit_bootstrap_fa can)
 * DEVICE pointers: data (echo e of voxel v at data[v * voxel_stride + e * echo_stride], strides > 0), fa_index, mask, fsol, sig, reg, lam,
 * maps, status as for met2_fit_strided; voxel_id [nvox] int64 or NULL; sigma [nvox] (>= 0) or NULL; sigma_out [nvox]; out:
 *   stats       [7][5][nvox]  quantities MWF, IEWF, FWF, T2_M, T2_IE, TWC (the maps' order) and reg; statistics mean, std (ddof = 1; both in
 *                             two deterministic passes) and the 0.025, 0.5, 0.975 quantiles, bit-equal to np.quantile (method 'linear').
 *                             Zeros where the point status lacks MET2_ST_FITTED
 *   rep_status  [nvox]        OR of the replicates' status bits (0 where not fitted)
 * sig, lam, maps, status, sigma_out and rep_status may be NULL.  2 <= n_rep <= 1024.  The replicates are fitted in chunks of whole voxels
 * (262 144 rows; 4 096 for L-curve at n_t2 > 64) through met2_fit_enqueue_strided on scratch kept with the plan until met2_plan_destroy.
 * Blocking (one wait after the point fit, which reports an FA index outside the dictionary, and one at the end). */
int met2_fit_bootstrap(met2_plan *plan, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                       const double *fa_index, const uint8_t *mask, const int64_t *voxel_id, const double *sigma, int32_t n_rep,
                       int64_t seed, double *fsol, double *sig, double *reg, double *lam, double *maps, int32_t *status,
                       double *sigma_out, double *stats, int32_t *rep_status, void *stream);
/* The same with the flip angle re-estimated on every replicate, and with statistics of the replicates' spectra (additive; ABI stays 6).
 * met2_fit_bootstrap refits every replicate at the point fit's FA, so its spread holds only the noise that reaches the spectrum at a fixed
 * dictionary slice; a pipeline that estimates the FA per voxel (motor:349-373; evaluate_all_methods_two_lobes_SNR50_150.py:398 does so for
 * every noisy voxel) has a second estimation step, whose error this entry can put into the spread.  Everything not named here is as in
 * met2_fit_bootstrap: the point fit, sigma_v, the replicate generator (a replicate row is bit for bit met2_bootstrap_replicates') and the gating.
 *   fa_mode  MET2_BOOT_FA_FIXED       the replicates are fitted at the point fit's FA: rows 0..6 of stats, rep_status, sigma_out and all point
 *                                     outputs are bit for bit met2_fit_bootstrap's; row 7 holds the point FA index (mean and quantiles, std 0)
 *            MET2_BOOT_FA_BRUTEFORCE  every replicate row goes through the plan's brute-force walk exactly as met2_fa_bruteforce treats a row
 *                                     (un-normalised echoes, gate of fa_estimation.py:45) and is fitted at THAT index; the row's mask is the
 *                                     voxel's point-fit MET2_ST_FITTED bit
 *            MET2_BOOT_FA_SPLINE      the same with the coarse walk on the plan attached by met2_plan_attach_fa_spline followed by the
 *                                     spline selection (met2_fa_spline_select); MET2_E_STATE if nothing is attached
 *   fa_index still gives the POINT fit's FA: the caller estimated it, possibly on a smoothed volume.  A replicate's FA is estimated on the
 *            replicate row alone: the Gaussian pre-smoothing of motor:337-343 is spatial, and replicates of different voxels are independent
 *            draws, so it does not apply.  (With a point FA from a smoothed volume the spread would then measure the difference between two
 *            estimators; the Python drivers refuse that combination.)
 *   stats       [8][5][nvox]        the 7 quantities of met2_fit_bootstrap, then the FA index the replicates were fitted with
 *   spec_stats  [5][nvox][n_t2]     or NULL: mean, std (ddof = 1), q0.025, q0.5, q0.975 over the replicates of fsol[row][j] as the fit writes it
 *                                   (x * km, not normalised), per T2 bin, with the definitions of stats (two deterministic passes; quantiles
 *                                   bit-equal to np.quantile, method 'linear'); zeros where the point status lacks MET2_ST_FITTED.  Taken from
 *                                   the replicate spectra the fits have just written: no additional fits
 * The FA walk is enqueued per chunk in front of the chunk's fit on the caller's stream; its scratch stays with the plans.  Blocking like
 * met2_fit_bootstrap (the same two waits). */
enum met2_boot_fa { MET2_BOOT_FA_FIXED = 0, MET2_BOOT_FA_BRUTEFORCE = 1, MET2_BOOT_FA_SPLINE = 2 };
int met2_fit_bootstrap_fa(met2_plan *plan, int32_t method, int32_t fa_mode, int64_t nvox, const double *data, int64_t voxel_stride,
                          int64_t echo_stride, const double *fa_index, const uint8_t *mask, const int64_t *voxel_id, const double *sigma,
                          int32_t n_rep, int64_t seed, double *fsol, double *sig, double *reg, double *lam, double *maps, int32_t *status,
                          double *sigma_out, double *stats, double *spec_stats, int32_t *rep_status, void *stream);
/* Test/diagnostic entry: the replicates of met2_fit_bootstrap for given centres.  DEVICE pointers: center [nvox][n_te] (the s_hat), sigma
 * [nvox], voxel_id [nvox] or NULL; out [nvox][n_rep][n_te].  Every voxel gets replicates (no gating).  Asynchronous on `stream`. */
int met2_bootstrap_replicates(met2_plan *plan, int64_t nvox, const double *center, const double *sigma, const int64_t *voxel_id,
                              int32_t n_rep, int64_t seed, double *out, void *stream);
/* The statistics kernels of met2_fit_bootstrap and met2_fit_bootstrap_fa on values the caller supplies (additive; ABI stays 6): what summarises a quantity derived
 * from replicates, and what lets a test hand the kernels any series.  No plan: `device` and `stream` only.  DEVICE pointers.
 * A series is the n_rep consecutive values of one voxel; its statistics are those of stats above (mean, std with ddof = 1, the 0.025, 0.5
 * and 0.975 quantiles bit-equal to np.quantile, method 'linear').  status [nvox] or NULL: a voxel whose status lacks MET2_ST_FITTED gets
 * zeros and its values are not read; NULL counts every voxel (the call then allocates a status of its own and waits for `stream` before it
 * returns; with a status it is asynchronous on `stream`).  2 <= n_rep <= 1024.
 *   met2_bootstrap_series_stats     values [n_quant][nvox * n_rep], 1 <= n_quant <= 8  ->  stats [n_quant][5][nvox]   (bootstrap_stats_kernel)
 *   met2_bootstrap_spectrum_stats   fsol_r [nvox * n_rep][n_t2], 1 <= n_t2 <= 65536    ->  spec [5][nvox][n_t2]      (bootstrap_spec_stats_kernel,
 *                                   with the tile geometry and LDS size the fused entry launches it with).  Bin j of voxel v is the series
 *                                   fsol_r[(v n_rep + b) n_t2 + j], b = 0 .. n_rep - 1
 * Both give the same bits for the same series.  Input domain: finite values and NaN.  A series with a NaN gives five NaNs, as numpy does.
 * +-inf is outside the contract: the mean is taken from sums shifted by the series' first value, which turn an inf into NaN where numpy
 * gives inf.  The accuracy of mean and std against exact arithmetic (|mean error| <= 1e-14 max|v|, |std error| <= 1e-12 std + 1e-14 max|v|)
 * holds for nonzero magnitudes within [1e-150, 1e150]: outside, squares under- or overflow in float64, for numpy's std as well. */
int met2_bootstrap_series_stats(int32_t device, int64_t nvox, int32_t n_rep, int32_t n_quant, const double *values, const int32_t *status,
                                double *stats, void *stream);
int met2_bootstrap_spectrum_stats(int32_t device, int64_t nvox, int32_t n_rep, int32_t n_t2, const double *fsol_r, const int32_t *status,
                                  double *spec, void *stream);
/* Host only: how bootstrap_spec_stats_kernel is launched for series of n_rep values, by every entry that launches it -- T2 bins per tile,
 * doubles between two series of a tile, dynamic LDS in bytes (at most 65 536).  Any output may be NULL. */
int met2_bootstrap_spec_launch_info(int32_t n_rep, int32_t *tile_bins, int32_t *tile_stride, int64_t *lds_bytes);

/* ---- Rician noise floor (an extension: the reference has no counterpart; additive, ABI stays 6) ----------
 * The echoes are magnitudes, so their noise is Rician: with t = A^2 / (2 sigma^2) the mean of a magnitude with true amplitude A >= 0 and
 * noise sigma > 0 is
 *   m(A, sigma) = sigma sqrt(pi / 2) [(1 + t) i0e(t / 2) + t i1e(t / 2)],   i0e(x) = exp(-x) I0(x), i1e(x) = exp(-x) I1(x)
 * (the exponentially scaled modified Bessel functions: the unscaled ones overflow at A / sigma ~ 53).  The bias b(A, sigma) = m(A, sigma) - A
 * is >= 0, b(0, sigma) = sigma sqrt(pi / 2), b ~ sigma^2 / (2 A) for A >> sigma; b(A, 0) = 0 by definition and A < 0 is read as 0.  The
 * inverse A = m^-1(M, sigma) is the root of m(A, sigma) = M for M > sigma sqrt(pi / 2) and 0 otherwise (m is increasing in A).  A fit treats
 * the floor sigma sqrt(pi / 2) of the late echoes as signal -- a spurious long-T2 pool.  What is here:
 *   met2_rician_bias     b[i] = b(A[i], sigma[i]), i < n.  The device function every other kernel calls (float64 Chebyshev series of i0e and
 *                        i1e; from A / sigma = 1024 on the asymptotic series of b).  |b - exact| <= 1e-13 max(A, sigma) for A / sigma from 0 to 1e12
 *   met2_rician_step     out[v][e] = data[v][e] - b(model[v][e], sigma[v]); not clipped: the fit's gate reads the echo sum and the first echo
 *                        only, normalises by the first echo, and its NNLS does not need y >= 0.  A voxel that would fall out of that gate
 *                        afterwards (out[v][0] <= 0 or sum_e out[v][e] <= 0) is left uncorrected, out = data for all its echoes, and flag[v] = 1;
 *                        voxels with mask = 0 or sigma = 0 are copied, flag 0.  Several voxels per wave (one at n_te > 32); the sum is taken in a fixed order
 *   met2_rician_invert   out[v][e] = m^-1(data[v][e], sigma[v]) (mask = 0 or sigma = 0: copied).
 *                        |m(out, sigma) - max(data, sigma sqrt(pi / 2))| <= 1e-13 max(data, sigma): the condition is on the forward residual
 *                        because the inverse is ill-conditioned at A -> 0, where dm / dA = 0
 *   met2_noise_sigma     the estimate met2_fit_bootstrap makes when no sigma is given (bit for bit its sigma_out): a plain-NNLS pass at the
 *                        voxel's flip angle, then sqrt(sum_e residual_e^2 / max(n_te - #{x > 0}, 1)); sig0 [nvox][n_te] or NULL: that pass's
 *                        model signal.  Blocking (reports an FA index outside the dictionary); scratch stays with the plan
 *   met2_fit_rician      sigma_v = sigma[v], or met2_noise_sigma's on the raw data when sigma is NULL (returned in sigma_out either way).
 *                        y^0 = data; for k = 0 .. n_iter: fit y^k as met2_fit_strided does, giving the model signal s^k; if k < n_iter,
 *                        y^(k+1) = step(data, s^k, sigma): the correction is always applied to the RAW data, never accumulated.  The outputs
 *                        are the last fit's (sig is then the noise-free signal estimate); flag [nvox] is the last step's.  n_iter = 0 is
 *                        met2_fit_strided bit for bit; 0 <= n_iter <= 16.  A voxel whose status lacks MET2_ST_FITTED after pass 0 is never
 *                        corrected; the flip angle is fixed through the passes.  Passes 1 .. n_iter run in chunks of whole voxels (262 144;
 *                        4 096 for L-curve at n_t2 > 64) through met2_fit_enqueue_strided on scratch kept with the plan until
 *                        met2_plan_destroy.  Blocking (one wait after pass 0, which reports an FA index outside the dictionary, one at the end)
 * All pointers are DEVICE pointers.  data: echo e of voxel v at data[v * voxel_stride + e * echo_stride] (strides in doubles, > 0), as for
 * met2_fit_strided; model, out, sig0: [nvox][n_te] rows; sigma, sigma_out [nvox] (>= 0); mask [nvox] uint8 or NULL = all ones; flag [nvox]
 * int32, may be NULL; out must not overlap data.  fsol, sig, reg, lam, maps, status as for met2_fit_strided (sig, lam, maps, status, sigma_out,
 * flag may be NULL).  The three kernel entries take `device` and are asynchronous on `stream`.
 * What this is not: sigma is not re-estimated after a correction, and the residual estimate is biased low where many echoes sit in the
 * floor; met2_rician_invert treats its input as the Rician MEAN, which a denoised magnitude only approximates; nothing here makes the fit a
 * maximum-likelihood Rician fit. */
int met2_rician_bias(int32_t device, int64_t n, const double *A, const double *sigma, double *b, void *stream);
int met2_rician_step(int32_t device, int64_t nvox, int32_t n_te, const double *data, int64_t voxel_stride, int64_t echo_stride,
                     const double *model, const double *sigma, const uint8_t *mask, double *out, int32_t *flag, void *stream);
int met2_rician_invert(int32_t device, int64_t nvox, int32_t n_te, const double *data, int64_t voxel_stride, int64_t echo_stride,
                       const double *sigma, const uint8_t *mask, double *out, void *stream);
int met2_noise_sigma(met2_plan *plan, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride, const double *fa_index,
                     const uint8_t *mask, double *sigma_out, double *sig0, void *stream);
int met2_fit_rician(met2_plan *plan, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                    const double *fa_index, const uint8_t *mask, const double *sigma, int32_t n_iter, double *fsol, double *sig, double *reg,
                    double *lam, double *maps, int32_t *status, double *sigma_out, int32_t *flag, void *stream);

/* ---- Monte-Carlo accuracy study (scripts_synthetic_data_evaluation/Paper_Comparison/evaluate_all_methods_two_lobes_SNR*.py) -------
 * met2_synth_two_lobe draws n two-lobe voxels by the reference's recipe (:156-190, :376-428).  Per voxel, from counter-based Philox4x32-10
 * (philox.hpp) with key (lo32(seed), hi32(seed)) and counter (c0, stream, lo32(id), hi32(id)), id = voxel_offset + v:
 *   stream 1, c0 = 0..3   eight 53-bit uniforms u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 in [0, 1), taken in the order MWF, T2m, T2ie, FA |
 *                         SNR, sigma_m, sigma_ie; each value lo + (hi - lo) u.  FA is continuous (not snapped to a dictionary grid)
 *   pdf on linspace(1, 300, 1000): MWF N(T2m, sigma_m) + (1 - MWF) N(T2ie, sigma_ie), normalised to sum 1 (f_csf = 0)
 *   signal_e = km (1 - exp(-TR/T1)) sum_j EPG_e(T2_j; FA, FA/2, te, T1) pdf_j
 *   stream 2, c0 = e      Rician noise at sigma = signal_0 / SNR, Box-Muller as met2_bootstrap_replicates; none when snr_lo = +inf
 * DEVICE outputs: data [n][n_te]; true_dist [n][n_t2] the pdf re-binned onto the plan's T2 grid by the midpoint rule of :404-426
 * (normalised); truth [MET2_EVAL_NTRUTH][n] = MWF (sum of true_dist at T2 <= t2_myelin_cut), T2m, T2ie, km, FA, SNR (inf when noise-free),
 * the drawn MWF, sigma_m, sigma_ie.  n_te <= 64, n_t2 <= 128.  Asynchronous on `stream`. */
#define MET2_EVAL_NTRUTH 9
typedef struct met2_synth_params {
    int32_t struct_size;      /* sizeof(met2_synth_params)                                       */
    int32_t reserved0;
    double te, TR, T1;        /* echo spacing (ms), :186-189 10; TR :209 3000; T1 :181 1000     */
    double mwf_lo, mwf_hi;    /* :156  0.05, 0.25                                                */
    double t2m_lo, t2m_hi;    /* :158  15, 35                                                    */
    double t2ie_lo, t2ie_hi;  /* :160  60, 90                                                    */
    double fa_lo, fa_hi;      /* :162  90, 180 (degrees)                                         */
    double snr_lo, snr_hi;    /* :164  50, 150; snr_lo = +inf: no noise (the SNR_Inf script)     */
    double sm_lo, sm_hi;      /* :168  1, 3                                                      */
    double sie_lo, sie_hi;    /* :170  6, 12                                                     */
    double km;                /* :166  1000                                                      */
} met2_synth_params;
int met2_synth_two_lobe(met2_plan *plan, const met2_synth_params *params, int64_t n, int64_t seed, int64_t voxel_offset, double *data,
                        double *true_dist, double *truth, void *stream);
/* estimate_error_metrics (:59-74) per voxel from a fit's fsol [n][n_t2] (already multiplied by the first echo) and true_dist [n][n_t2]
 * (DEVICE).  km = sum fsol, x = fsol / km; out [MET2_EVAL_NFIELD][n] = fM (x at T2 <= t2_myelin_cut), fIE (t2_myelin_cut < T2 <= t2_ie_cut),
 * arithmetic-mean T2 of both (epsilon 1e-50), km, the number of scipy.signal.find_peaks(x, height = 1e-5 max x), mean |true_dist - x|,
 * scipy.spatial.distance.jensenshannon(true_dist, x) and scipy.stats.wasserstein_distance(true_dist, x) (the bin values as samples).
 * 3 <= n_t2 <= 128.  One wave per voxel; asynchronous on `stream`. */
#define MET2_EVAL_NFIELD 9
int met2_eval_voxel_metrics(met2_plan *plan, int64_t n, const double *fsol, const double *true_dist, double *out, void *stream);
/* compute_multi_metrics (:77-123) of one method over n voxels, and the lambda statistics.  DEVICE: per_voxel [MET2_EVAL_NFIELD][n] (of
 * met2_eval_voxel_metrics), truth [MET2_EVAL_NTRUTH][n] (of met2_synth_two_lobe), lam [n] or NULL (zeros), fie [n] or NULL: the fIE array
 * GMARE's second term reads (NULL: per_voxel's own; the reference reads its NNLS array for every method, :107).  out [MET2_EVAL_NAGG] = MAE,
 * MARE, RMSE, cRMSE, RMSRE, U95, MBE, R, GMARE, MAE-k, MAE-S, MJSD-S, MWD-S (the columns of table_errors.txt), mean and std (ddof 0) of
 * lambda.  Every aggregate is what its formula gives in IEEE arithmetic, NaN and Inf included: R is clamped to [-1, 1] only when it is a
 * number, so a constant column, n = 1 or a NaN voxel gives R = NaN (0/0), as scipy.stats.pearsonr does.  One workgroup in a fixed
 * reduction order: the same inputs give the same bits.  Runs on the current device; asynchronous. */
#define MET2_EVAL_NAGG 15
int met2_eval_reduce(int64_t n, const double *per_voxel, const double *truth, const double *lam, const double *fie, double *out, void *stream);

/* Test/diagnostic entry: `method` = 10 + MET2_X2 / MET2_GCV / MET2_BAYESREG passed to met2_fit
 * evaluates that method's lambda-selection objective (algorithms.py:226-233, :285-296,
 * bayesian_interpolation.py:107-126) on the plan's lambda grid (n <= n_t2 points) and stores the
 * values in fsol[v][0..n); sig, lam and maps are not written. */
#define MET2_OBJECTIVE_GRID 10

/* flip_angle_algorithms/fa_estimation.py:74-111 (brute force over the plan's FA axis).
 * DEVICE pointers: data [nvox][n_te] (un-normalised), mask [nvox] (NULL = ones);
 * out fa_index [nvox] float64 (0 where gated out), km [nvox] = sum(f) at the best FA
 * (may be NULL), resid [nvox][n_fa] NNLS residual norms (may be NULL). */
int met2_fa_bruteforce(met2_plan *plan, int64_t nvox, const double *data, const uint8_t *mask,
                       double *fa_index, double *km, double *resid, void *stream);

int met2_fa_bruteforce_strided(met2_plan *plan, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                               const uint8_t *mask, double *fa_index, double *km, double *resid, void *stream);

/* flip_angle_algorithms/fa_estimation.py:54-59, the selection step of the spline FA method (the CLI default,
 * run_real_data_script.py:34): given the plain-NNLS residual norms on a coarse FA grid (`resid` from
 * met2_fa_bruteforce on a plan built with the coarse grid, motor:237-238), interpolate them with a cubic
 * spline (scipy interp1d(kind='cubic')), minimise over [90, 180] with the bounded Brent of
 * scipy minimize_scalar(method='Bounded') and snap to the fine grid.  alpha_lr [n_lr] and alpha_hr [n_hr] are
 * host arrays; resid [nvox][n_lr], data [nvox][n_te], mask are DEVICE pointers (data/mask only gate voxels,
 * fa_estimation.py:45); out fa_index [nvox] float64 index into alpha_hr, xmin [nvox] the continuous minimiser
 * (may be NULL).  Blocking. */
int met2_fa_spline_select(int32_t device, int64_t nvox, int32_t n_lr, const double *alpha_lr, const double *resid,
                          int32_t n_hr, const double *alpha_hr, int32_t n_te, const double *data, const uint8_t *mask,
                          double *fa_index, double *xmin, void *stream);

int met2_fa_spline_select_strided(int32_t device, int64_t nvox, int32_t n_lr, const double *alpha_lr, const double *resid,
                                  int32_t n_hr, const double *alpha_hr, int32_t n_te, const double *data, int64_t voxel_stride,
                                  int64_t echo_stride, const uint8_t *mask, double *fa_index, double *xmin, void *stream);

/* motor:337-343, the Gaussian pre-smoothing of the FA step (FA_smooth='yes', the CLI default): the reference runs
 * scipy.ndimage.gaussian_filter(volume, 2.0) on every echo volume.  This is the separable filter behind it: one pass per
 * spatial axis with the symmetric kernel weights[0 .. 2 radius] (HOST array, weights[radius] the centre; for the
 * reference: radius = int(4 sigma + 0.5), weights = exp(-x^2 / (2 sigma^2)) normalised to sum 1), boundary mode 'reflect',
 * accumulated in scipy's order, so the result is bit-identical to gaussian_filter.  DEVICE pointers: data and out
 * [nx][ny][nz][n_te], work the same size (NULL: allocated and freed inside, which makes the call blocking); all distinct.
 * radius <= 32. */
int met2_smooth_separable(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, int32_t radius, const double *weights,
                          const double *data, double *out, double *work, void *stream);

/* motor:305-333, the NESMA filter (denoise='NESMA').  DEVICE pointers: data [nx][ny][nz][n_te] (already
 * multiplied by the mask and clipped at 0, motor:180-182 and :279), mask [nx][ny][nz] uint8 -- voxels with
 * mask == 1 are filtered (motor:317), all others get zeros (NULL = filter every voxel); out [nx][ny][nz][n_te],
 * must not alias data.  Each filtered voxel becomes the mean of the voxels in its half-open window
 * [x-6, x+6) x [y-6, y+6) x [z-6, z+6) (clipped to the volume) whose relative L1 distance to it is < 2.5 %
 * (nan when none qualifies, e.g. an all-zero signal, like np.mean of an empty selection).  n_te <= 128.
 * Asynchronous on `stream`. */
int met2_nesma(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const double *data,
               const uint8_t *mask, double *out, void *stream);

/* Marchenko-Pastur PCA denoising (denoise='MPPCA'; Veraart et al., NeuroImage 2016; an extension with no counterpart in the reference).
 * DEVICE pointers: data [nx][ny][nz][n_te] fp64 in C order, mask [nx][ny][nz] uint8 (NULL = every voxel), out [nx][ny][nz][n_te], must
 * not alias data; out, each may be NULL: sigma [nx][ny][nz] the estimated noise level, rank [nx][ny][nz] int32 the number of signal
 * components kept.  window = w, odd and >= 3.  For every voxel v with mask != 0:
 *   1. the patch is the cube of side w centred on v, clipped at the volume's faces and restricted to voxels with mask != 0; N = its
 *      voxel count (v is one of them), X = the n_te x N matrix of their decay curves, not centred; M = n_te, r = min(M, N), q = max(M, N);
 *   2. C = X X^T, eigenvalues ev ascending with orthonormal eigenvectors; lambda_p = max(ev[M - r + p], 0) / q for p = 0..r-1 (for N < M
 *      the lowest M - N eigenvalues are zero up to rounding and are dropped with their eigenvectors);
 *   3. clam = 0, cut = 0, sigma2 = 0; for p = 0..r-1: clam += lambda_p, gamma = (p + 1) / q, s1 = clam / (p + 1),
 *      s2 = (lambda_p - lambda_0) / (4 sqrt(gamma)); if s2 < s1: sigma2 = s1, cut = p + 1.  k = r - cut signal components;
 *   4. out[v] = U_s (U_s^T x_v) with U_s the eigenvectors of the k largest eigenvalues, sigma[v] = sqrt(sigma2), rank[v] = k.
 * mask == 0: out = 0, sigma = 0, rank = 0.  N < 2: the voxel is copied through, sigma = 0, rank = 1.  A non-finite value anywhere in the
 * patch: copied through, sigma = 0, rank = -1; so is a voxel whose data are finite but whose C overflows (a non-finite trace; |x| above
 * about 1e152).  The eigen-solver (a cyclic Jacobi, stopped when every |c_ij| <= 2^-52 sqrt(c_ii c_jj), the root taken so that it neither
 * overflows nor vanishes while C is finite) capped at its 30 sweeps: copied through, sigma = 0, rank = -2.  Scaling the data by a power of two
 * scales out and sigma by exactly that power while nothing over- or underflows.  Below |x| of about 1e-155 the entries of C are subnormal
 * and the accuracy degrades (a residual of 1e-10 ||C|| at 1e-160 in an emulation; unmeasured on the device).
 * The output is not clipped: the projection can undershoot zero at late echoes.
 * MET2_E_INVALID: window even or < 3, data or out NULL, out == data.  MET2_E_UNSUPPORTED: n_te < 2 or > 63; a window whose patch list
 * (4 w^3 bytes) does not fit in the 64 KB of LDS beside the two n_te x n_te matrices (w <= 7 fits at every n_te); more than 2^26 - 1 voxels.
 * An empty volume returns MET2_OK at once.  Deterministic; asynchronous on `stream`. */
int met2_mppca(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const double *data, const uint8_t *mask, int32_t window,
               double *out, double *sigma, int32_t *rank, void *stream);

/* met2_mppca with what each of its steps leaves, for tests and diagnostics (additive; ABI stays 6).  The same kernel code, instantiated a
 * second time; out, sigma and rank are bit for bit those of met2_mppca when max_sweeps = 30.  max_sweeps, 1..30 (else MET2_E_INVALID), is the
 * sweep cap of the eigen-solver; a voxel that has not converged by then gets rank -2.  DEVICE pointers, each may be NULL, nvox = nx ny nz:
 *   n_patch [nvox] int32            N, the patch's voxel count;
 *   patch   [nvox][w^3] int32       the patch list as the kernel holds it: the flat voxel offsets pv - v, in memory order; the first N are written;
 *   gram    [nvox][n_te][n_te]      C as stored after step 2;
 *   eigval  [nvox][n_te]            the diagonal of C after the solver, in index order (unsorted);
 *   eigvec  [nvox][n_te][n_te]      V after the solver: column i belongs to eigval[i];
 *   sweeps  [nvox] int32            the sweeps run, the last one that found nothing to rotate included.
 * A voxel with mask == 0 writes n_patch = 0 and nothing else.  A voxel copied through for N < 2 or for a non-finite value writes n_patch and
 * patch and nothing else.  A voxel whose C overflowed also writes gram, the diagonal and the identity it started from, and sweeps = 0.  A voxel
 * that hit the sweep cap writes everything, as it stood then.  What a voxel does not write is left as the caller had it. */
int met2_mppca_stages(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const double *data, const uint8_t *mask, int32_t window,
                      double *out, double *sigma, int32_t *rank, int32_t max_sweeps, int32_t *n_patch, int32_t *patch, double *gram,
                      double *eigval, double *eigvec, int32_t *sweeps, void *stream);

/* met2_mppca with a box window and, optionally, the average over the overlapping patches (mppca_filter's window= and average=; additive, ABI stays
 * 6; the averaging after Manjon et al., PLoS ONE 2013; pinned against its numpy restatement only, tests/tools/mppca_box_numpy.py -- parity
 * with MRtrix's dwidenoise or DIPY is unpinned).  DEVICE pointers as for met2_mppca, and out, each may be NULL: n_patch [nx][ny][nz] int32,
 * wsum [nx][ny][nz].  window (HOST) = (wx, wy, wz), each odd and >= 1, wx wy wz >= 3.
 *   Patch.  The patch of a voxel c with mask != 0 is the box of half-widths (wx / 2, wy / 2, wz / 2) around it, clipped at the volume's faces,
 *     restricted to voxels with mask != 0 and listed in memory order.  Steps 1-3 of met2_mppca run unchanged on it and give k_c, sigma_c and
 *     U_c, the eigenvectors of the k_c largest eigenvalues.  The copy-through classes are those of met2_mppca: N < 2 (rank 1), a non-finite
 *     value or an overflowing C (rank -1), the eigen-solver's give-up (rank -2).
 *   average = 0.  Step 4 of met2_mppca: out[v] = U_v (U_v^T x_v), sigma[v] = sigma_v, rank[v] = k_v, n_patch[v] = N_v, wsum[v] = 0.  With
 *     wx = wy = wz = w this is met2_mppca(window = w) bit for bit (the same kernel code).  One launch, no work space, asynchronous on `stream`.
 *   average = 1.  For a voxel v with mask != 0 let C(v) be the masked voxels of the same clipped box around v, in ascending memory order (the
 *     box is symmetric: these are the centres whose patch holds v).  A centre votes unless it is in a copy-through class; its weight is
 *     w_c = 1 / (1 + k_c).  out[v] = (sum_c w_c U_c (U_c^T x_v)) / (sum_c w_c), sigma[v] = (sum_c w_c sigma_c) / (sum_c w_c), both sums over
 *     the voting centres of C(v) in that order; rank[v] = v's own k_v (the negative codes included), n_patch[v] = N_v, wsum[v] = sum_c w_c.  No
 *     voting centre: out[v] = x_v, sigma[v] = 0, wsum[v] = 0.  A centre of rank 0 votes with weight 1 and a zero curve.
 *     The order of the arithmetic: per centre p = sum_j u_j (u_j . x_v) over the kept eigenvectors by ascending eigenvalue, one fused
 *     multiply-add per term; each dot product is a 64-lane tree (neighbouring lanes first: pairs, fours, eights, sixteens, then
 *     (row 0 + row 1) + (row 2 + row 3)) over the echoes; then acc = fma(w_c, p, acc), wsum += w_c, ssum = fma(w_c, sigma_c, ssum).
 *   mask == 0: out = 0, sigma = 0, rank = 0, n_patch = 0, wsum = 0.  Scaling the data by a power of two scales out and sigma by exactly that
 *   power while nothing over- or underflows; rank, n_patch and wsum do not change.
 *   Work space (average = 1).  Per centre a 24-byte head and its k_c kept eigenvectors, k_c n_te doubles taken from a pool by one atomic add
 *     (where a centre's vectors lie in the pool depends on the order of arrival, what they hold does not); 16 bytes hold the pool's count.
 *     With P = min(wx, nx) min(wy, ny) min(wz, nz), the largest patch of the volume and the most centres that hold one voxel, and
 *     K = min(n_te, P), the most vectors a centre keeps: c centres need at most 16 + c (24 + 8 n_te K) bytes, and are reckoned at
 *     16 + 24 c + 8 max(c n_te min(K, 8), P n_te K) bytes -- 8 vectors per centre (measured means at 32 echoes: 1.1 to 1.3), and never less
 *     than one voxel's centres need at most.  The volume is cut into boxes of output voxels whose centres -- the box widened by the
 *     half-widths, clipped -- fit as reckoned: whole (y, z) planes while one plane's centres fit, else whole z lines of one plane, else runs
 *     of one line; centres in the overlap of two boxes are decomposed again.  A box whose centres keep more vectors than the pool holds
 *     writes nothing past it, is halved along its longest side and run again; a box of one voxel always fits.  (The overfilled attempt's
 *     decomposition is thrown away: where most centres keep more than 8 vectors, every halving decomposes the box once more.  Unmeasured.)
 *     The entry allocates one
 *     device block of at most max_work_bytes (0: the default, which is the whole volume's largest need capped at 2^30 bytes = 1 GiB,
 *     whatever the volume), enqueues on `stream`, waits for it -- after every box that could have overfilled the pool, and at the end -- and
 *     frees the block: BLOCKING.  The result does not depend on the cut and repeats to the bit.  met2_mppca_box_work_bytes gives min_bytes
 *     (one voxel's centres at any rank: at most 343 of them, 10.9 MB at 63 echoes) and default_bytes for a shape without touching a device;
 *     both are 0 for average = 0 and for an empty volume.
 * MET2_E_INVALID: a negative dimension, window NULL, an entry even or < 1, wx wy wz < 3, average outside {0, 1}, max_work_bytes < 0, or
 * (average = 1) > 0 and below min_bytes -- the message names the minimum --, data or out NULL, out == data.  MET2_E_UNSUPPORTED: n_te < 2 or
 * > 63; wx wy wz > 343 (the patch list, 4 wx wy wz bytes, must fit in LDS beside the two n_te x n_te matrices at every n_te); more than
 * 2^26 - 1 voxels.  The checks of window, average and n_te come first; an empty volume then returns MET2_OK at once.  Deterministic. */
int met2_mppca_box(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const double *data, const uint8_t *mask,
                   const int32_t window[3], int32_t average, int64_t max_work_bytes, double *out, double *sigma, int32_t *rank,
                   int32_t *n_patch, double *wsum, void *stream);
int met2_mppca_box_work_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const int32_t window[3], int32_t average,
                              int64_t *min_bytes, int64_t *default_bytes);

/* Removal of Gibbs (truncation) ringing by local sub-voxel shifts (degibbs='yes'; Kellner, Dhital, Kiselev, Reisert, MRM 2016; step 2 of the
 * reference's example pipeline, example_script_run_MET2_preproc_and_recon.sh, which runs MRtrix's mrdegibbs there; stated here from the
 * paper, none of MRtrix's program text is used and parity with mrdegibbs itself is unpinned).
 * DEVICE pointers: data [nx][ny][nz][n_te] fp64 in C order; out the same shape, must not alias data; out, each may be NULL: shift_x, shift_y
 * [nx][ny][nz][n_te] int8, the signed shift sh[j*] chosen per sample along x and along y (a diagnostic).  nshifts = nsh (MRtrix: 20),
 * min_w = minW (1), max_w = maxW (3).  The unringing axes are x and y; every (z, echo) slice S[nx][ny] is processed on its own, in real fp64:
 *   2-D split.  F = DFT2(S); for the frequency indices (p, q): cx = 1 + cos(2 pi p / nx), cy = 1 + cos(2 pi q / ny), Gx = cy / (cx + cy),
 *     Gy = cx / (cx + cy), both 0 where cx + cy == 0 (the corner Nyquist term of even nx and ny).  Ix = Re IDFT2(F Gx), Iy = Re IDFT2(F Gy)
 *     (Ix + Iy = S less that corner term).  out = U(Ix along x) + U(Iy along y).
 *   U on a line x[0..n), indices periodic:
 *     1. sh = [0, 1, ..., nsh, -1, ..., -nsh] (2 nsh + 1 entries), delta_j = sh[j] / (2 nsh);
 *     2. x_j[m] = x(m + delta_j) by Fourier interpolation: x_j = IDFT(X[k] exp(2 pi i k' delta_j / n)), k' the signed frequency,
 *        |k'| <= (n - 1) / 2 (integer division); for even n the Nyquist bin is kept as it is for j = 0 and set to zero for every other j.
 *        In real form a circular convolution: x_j[m] = sum_l c_j[(m - l) mod n] x[l], c_j[r] = (1 / n) sum_k' cos(2 pi k' (r + delta_j) / n),
 *        plus (1 / n) cos(pi r) for j = 0 and even n;
 *     3. d_j[m] = |x_j[m] - x_j[m - 1]|;  TVL_j[l] = sum_{t = minW..maxW} d_j[l - t],  TVR_j[l] = sum_{t = minW..maxW} d_j[l + t + 1], each
 *        sum formed directly in increasing t (no running window);
 *     4. per sample l the candidates are scanned in the order (j = 0, L), (j = 0, R), (j = 1, L), (j = 1, R), ...; the first strict minimum
 *        gives j*;
 *     5. with delta = delta_j*, a0 = x_j*[l - 1], a1 = x_j*[l], a2 = x_j*[l + 1]:  out[l] = a1 (1 - delta) + a0 delta if delta > 0,
 *        a1 (1 + delta) - a2 delta otherwise.
 * A slice that holds a non-finite value is copied through unchanged (its shifts are 0); the other slices are not affected.
 * MET2_E_INVALID: a negative dimension, nshifts < 1, min_w < 1, min_w > max_w, data or out NULL, out == data.  MET2_E_UNSUPPORTED: nshifts > 32;
 * nx or ny outside 8..256; 2 (max_w + 1) > min(nx, ny) (at the smallest axis, 8, the default windows reach round the line and overlap); 2^31 samples or more.  All of them before any launch.  A volume with a zero-sized
 * dimension returns MET2_OK at once (after the checks of nshifts, min_w and max_w).  MRtrix accumulates the windows with running updates, so it
 * may pick another shift where two candidates tie within rounding.
 * Deterministic, slice by slice independent of the rest of the volume.  BLOCKING: the entry allocates its own work space (42 bytes per sample
 * of a chunk of at most 2^22 samples, or of one slice; plus the two axes' tables), enqueues on `stream`, waits for it and frees the space. */
int met2_degibbs(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const double *data, int32_t nshifts, int32_t min_w,
                 int32_t max_w, double *out, int8_t *shift_x, int8_t *shift_y, void *stream);

/* The stages of met2_degibbs one by one, for tests and diagnostics.  Each launches the kernels of met2_degibbs through the host code that
 * met2_degibbs itself runs; the argument checks and return codes are those of met2_degibbs where they apply.
 *
 * met2_gibbs_table_cols: the row length jp of the shift-kernel table at nshifts (2 nshifts + 1 rounded up to the kernel's pass width), or
 *   MET2_E_INVALID (nshifts < 1) / MET2_E_UNSUPPORTED (nshifts > 32).
 * met2_gibbs_tables: the two tables of one axis of length n, as the kernels read them.  DEVICE pointers: W [n][n][2], the DFT matrix
 *   W[b][q] = exp(-2 pi i b q / n) as (re, im) pairs; c [n][jp], c[r][j] = c_j[r] of step 2 of U for j < 2 nshifts + 1 and exactly 0 in the
 *   padding columns j >= 2 nshifts + 1.  8 <= n <= 256.  Asynchronous on `stream`.
 * met2_gibbs_split: the 2-D split alone.  DEVICE pointers: data [nx][ny][nz][n_te]; ix, iy the same shape, distinct from data and from each
 *   other: Ix and Iy of every (z, echo) slice.  A slice that holds a non-finite value gets what the arithmetic gives (not a copy).  The
 *   volume goes through the chunk loop of met2_degibbs.  BLOCKING.
 * met2_gibbs_lines: the operator U on nlines lines of n samples.  DEVICE pointers: lines [nlines][n]; out [nlines][n], must not alias lines;
 *   each may be NULL: shift [nlines][n] int8, the chosen sh[j*]; best [nlines][n], the winning candidate's total variation
 *   min(TVL_j*[l], TVR_j*[l]).  8 <= n <= 256, 2 (max_w + 1) <= n, nlines n < 2^31.  nlines == 0 or n == 0 returns MET2_OK at once (after
 *   the checks of nshifts, min_w and max_w).  A non-finite line is not treated specially here.  BLOCKING. */
int met2_gibbs_table_cols(int32_t nshifts);
int met2_gibbs_tables(int32_t device, int32_t n, int32_t nshifts, double *W, double *c, void *stream);
int met2_gibbs_split(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const double *data, double *ix, double *iy, void *stream);
int met2_gibbs_lines(int32_t device, int32_t n, int32_t nlines, const double *lines, int32_t nshifts, int32_t min_w, int32_t max_w, double *out,
                     int8_t *shift, double *best, void *stream);

/* Removal of Gibbs ringing along all three axes, for 3-D Fourier-encoded acquisitions whose partition axis is truncated in k-space like the
 * other two (degibbs='3d'; Bautista, O'Muircheartaigh, Hajnal, Tournier, "Removal of Gibbs ringing artefacts for 3D acquisitions using
 * subvoxel shifts", ISMRM 2021; stated here from the abstract, none of MRtrix's program text is used and parity with mrdegibbs is unpinned).
 * DEVICE pointers: data [nx][ny][nz][n_te] fp64 in C order; out the same shape, must not alias data; out, each may be NULL: shift_x, shift_y,
 * shift_z [nx][ny][nz][n_te] int8, the signed shift chosen per sample along each axis.  nshifts, min_w, max_w as for met2_degibbs.  Every echo
 * volume V[nx][ny][nz] is processed on its own, in real fp64:
 *   3-D split.  F = DFT3(V); for the frequency indices (p, q, r): cx = 1 + cos(2 pi p / nx), cy = 1 + cos(2 pi q / ny),
 *     cz = 1 + cos(2 pi r / nz), each exactly 0 at the Nyquist index of an even axis; wx = cy cz, wy = cx cz, wz = cx cy,
 *     den = wx + wy + wz; Ga = wa / den where den != 0.  den is 0 exactly where two or three of cx, cy, cz are 0 (three lines of k-space
 *     when all axes are even): there, with m the number of axes whose c is 0, Ga = 1 / m on those axes and 0 on the remaining one (the
 *     symmetric limit; NOT the rule of met2_degibbs, which drops its single corner term).  Gx + Gy + Gz = 1 everywhere.
 *     Ia = Re IDFT3(F Ga), so Ix + Iy + Iz = V; the kernels form Iz as (V - Ix) - Iy.
 *   out = (U(Ix along x) + U(Iy along y)) + U(Iz along z), U the operator of met2_degibbs, steps 1-5.
 * An echo volume that holds a non-finite value is copied through unchanged (its shifts are 0); the other echoes are not affected.
 * MET2_E_INVALID: a negative dimension, nshifts < 1, min_w < 1, min_w > max_w, data or out NULL, out == data.  MET2_E_UNSUPPORTED: nshifts > 32;
 * nx, ny or nz outside 8..256; 2 (max_w + 1) > min(nx, ny, nz); 2^31 samples or more.  All of them before any launch.  A volume with a
 * zero-sized dimension returns MET2_OK at once (after the checks of nshifts, min_w and max_w).
 * Deterministic, echo by echo independent of the rest of the volume.  BLOCKING: the entry allocates its own work space (67 bytes per sample
 * of a chunk of at most 2^22 samples, or of one echo volume; plus the three axes' tables), enqueues on `stream`, waits for it and frees the
 * space.
 * met2_gibbs_split3d: the 3-D split alone, through the host code and the chunk loop of met2_degibbs3d.  ix, iy, iz the shape of data, distinct
 * from data and from each other.  An echo that holds a non-finite value gets what the arithmetic gives (not a copy).  BLOCKING. */
int met2_degibbs3d(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const double *data, int32_t nshifts, int32_t min_w,
                   int32_t max_w, double *out, int8_t *shift_x, int8_t *shift_y, int8_t *shift_z, void *stream);
int met2_gibbs_split3d(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const double *data, double *ix, double *iy, double *iz,
                       void *stream);

/* Bias-field correction of a 3-D map (bias_correct='yes'; step 5 of the reference's example pipeline,
 * example_script_run_MET2_preproc_and_recon.sh, which runs FSL's `fast -t 3 -n 3 -H 0.1 -I 4 -l 20.0 -b` on the total water content map and
 * divides the estimated field out).  The EM bias-field estimation of Wells et al. (IEEE TMI 1996) and Guillemaud & Brady (IEEE TMI 1997): the
 * class-posterior-weighted residual, low-pass filtered by a normalised Gaussian convolution.  It is the estimator FAST iterates (Zhang, Brady,
 * Smith, IEEE TMI 2001) WITHOUT FAST's Markov random field term, and without partial-volume classes; stated here from the papers, none of
 * FSL's program text is used and parity with `fast` itself is unpinned.
 * DEVICE pointers: v [nx][ny][nz] fp64 in C order; mask [nx][ny][nz] uint8 or NULL (every voxel); out the same shape as v, must not alias it;
 * out, each may be NULL: field [nx][ny][nz], classes [3 K] = the final mu[K], var[K], pi[K].  HOST: voxel_mm[3] = (dx, dy, dz) in mm.
 * K = n_class (the script: 3), n_outer (-I 4), n_em (10), fwhm_mm (-l 20.0).
 *   1. Domain and log.  Omega = the voxels with mask != 0, v finite and v > 0; N = |Omega|; y = log v on Omega; lo = min y, hi = max y.
 *      Per axis a: sigma_a = fwhm / (2 sqrt(2 ln 2)) / d_a voxels, r_a = int(4 sigma_a + 0.5) (scipy's gaussian_filter1d truncation),
 *      w_a[t] = exp(-t^2 / (2 sigma_a^2)) for t = -r_a..r_a, divided by their sum (made on the host); r_a = 0 is the identity on that axis.
 *   2. Initial classes.  A 256-bin histogram of y over [lo, hi], bin = min(255, floor((y - lo) / (hi - lo) 256)); c its cumulative counts;
 *      mu_k = lo + (j_k + 0.5) (hi - lo) / 256 with j_k the first bin with c[j] >= (2 k + 1) / (2 K) N; var_k = Var_Omega(y) / K^2
 *      (population variance); pi_k = 1 / K; b = 0.
 *   3. n_outer times, with u = y - b on Omega:
 *      EM, n_em steps.  E: p_k proportional to pi_k var_k^(-1/2) exp(-(u - mu_k)^2 / (2 var_k)), formed in logs with the voxel's maximum
 *        subtracted, normalised over k.  M: s_k = sum p_k; mu_k = sum p_k u / s_k; var_k = max(sum p_k (u - mu_k)^2 / s_k, 1e-6) about the NEW
 *        mu_k; pi_k = s_k / N.  A class with s_k = 0 keeps mu_k and var_k, gets pi_k = 0 and has p_k = 0 from then on.  (The kernel sums
 *        p_k (u - m)^2 about the old mean m and takes s_k (mu_k - m)^2 off, which is the same number.)
 *      One more E-step; on Omega R = sum_k p_k (u - mu_k) / var_k, W = sum_k p_k / var_k; both 0 off Omega.
 *      S_R, S_W = R, W convolved with w_x, then w_y, then w_z; values outside the volume count as 0 (no reflection); taps added in
 *        ascending t.
 *      D = the voxels with S_W > 0 (it depends on Omega and the radii only).  b += S_R / S_W on D, then b -= mean_Omega(b) on D; b stays 0
 *        off D.
 *   4. field = exp(b) (1 off D); out = v / field where v is finite, a non-finite v is copied through.
 * N = 0 or hi == lo: field = 1 everywhere, out = v, classes mu = lo (0 for an empty domain), var = 0, pi = 1 / K; MET2_OK.
 * Properties of the estimator, not of this implementation: it needs classes that are separate in log intensity (three classes at 500 / 800 /
 * 1100 under a field of rms 0.16: correlation 0.965 with the true log field after 4 outer iterations, 0.997 after 8; at 700 / 830 / 1000
 * only 0.90), and with K = 1 it takes all smooth tissue contrast for bias.
 * MET2_E_INVALID: a negative dimension, K < 1, n_outer < 0, n_em < 1, voxel_mm NULL, a voxel size or fwhm that is not positive and finite, v or
 * out NULL, out == v.  MET2_E_UNSUPPORTED: K > 8, an r_a > 64, 2^31 voxels or more.  All of them before any launch.  A volume with a
 * zero-sized dimension returns MET2_OK at once (after the checks of the dimensions' signs, K, n_outer, n_em, voxel_mm and fwhm).
 * Deterministic: every fp64 sum over Omega is taken over Omega's voxels in memory order in a fixed tree, and the histogram counts are
 * integers, so the result is the same bits from run to run, does not depend on the launch geometry, and does not change when the volume is
 * embedded in a larger one with nothing in its mask within r_a of it.  The host reads nothing back during the call.  BLOCKING: the entry
 * allocates its own work space (53 bytes per voxel), enqueues every launch on `stream`, waits for it and frees the space. */
int met2_bias_field(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const uint8_t *mask, const double voxel_mm[3],
                    int32_t n_class, int32_t n_outer, int32_t n_em, double fwhm_mm, double *out, double *field, double *classes, void *stream);

/* The stages of met2_bias_field one by one, for tests and diagnostics.  Each launches the kernels of met2_bias_field through the host code
 * that met2_bias_field itself runs, on input the caller supplies; each allocates and frees what it needs and BLOCKS (it enqueues on `stream`,
 * waits for it and copies its small results to the host).  n = the voxels of the volume, N = n_domain, np = ceil(N / 1024), K = n_class.
 * DEVICE pointers: v, y, b, out, field [n] fp64; mask [n] uint8 or NULL; idx [n] int32; in, out of the smoothing, smoothed, rw_out [n][2].
 * HOST pointers: everything else.  idx[0..N) must hold voxel indices in [0, n): the kernels index y and b with them unchecked, as they do
 * with the list met2_bias_field makes for itself.  Additive: MET2_ABI_VERSION stays 6.
 *
 * met2_bias_weights (host only, no device): step 1's radii and weights as met2_bias_field makes them: radius_out [3]; weights_out, room for
 *   3 x 129 doubles, gets w_x[2 r_x + 1], w_y[2 r_y + 1], w_z[2 r_z + 1] one after the other, the layout met2_bias_smooth takes.
 * met2_bias_domain (log, scan, compact): y = log v on Omega and 0 off it, all n written; idx[0..N) = Omega's voxel indices in ascending order,
 *   idx[N..n) untouched; *n_domain = N.  A zero-sized volume: *n_domain = 0, MET2_OK, nothing written.
 * met2_bias_init (stat1, stat1_final, stat2, init), step 2 on the caller's y, idx, N (N = 0 is allowed).  Each out may be NULL:
 *   stats_out [4] = lo, hi, mean of y over idx[0..N), and 1.0 when N = 0 or hi == lo (degenerate), else 0.0;  hist_out [256] uint32, all 0 when
 *   degenerate;  ss_part_out [np]: the partial sums of (y - mean)^2 over the chunks of 1024 consecutive list entries, in the order of step-1's
 *   note below, untouched when degenerate (bias_init_kernel adds them up: var_k = (their sum) / N / K^2);  classes_out [3 K] = mu, var, pi, the
 *   degenerate classes (mu = lo, var = 0, pi = 1 / K) when degenerate.
 * met2_bias_em: classes_in [3 K] = mu, var, pi go into the device record, lc_k = -inf when pi_k == 0, otherwise log(pi_k) - 0.5 log(var_k) (the
 *   M-step's own rule, evaluated on the device); then n_em >= 0 times E-step and M-step with u = y - b; then, when rw_out is not NULL, the
 *   final E-step: rw_out[i] = (R, W) on idx[0..N) and (0, 0) elsewhere, all n pairs written.  Each may be NULL: part_out [3][K][np], the LAST
 *   E-step's partial sums per chunk of the list: [0] of p_k, [1] of p_k u, [2] of p_k (u - m_k)^2 about the mean m_k that E-step ran with;
 *   untouched when n_em = 0.  classes_out [3 K]: mu, var, pi after the last M-step (classes_in when n_em = 0).  The M-step adds the np
 *   partials of a sum in this order: thread h of 256 adds partials h, 256 + h, 512 + h, .. in that order, a butterfly (xor 32, 16, .. 1)
 *   adds the 64 lanes of a wave, the four waves add as (0 + 1) + (2 + 3) -- the order of every second-stage sum of the filter; within a chunk
 *   thread h adds entries h, 256 + h, 512 + h, 768 + h, then the same butterfly and the same four waves.  N >= 1, finite mu, finite var > 0,
 *   finite pi >= 0 (MET2_E_INVALID otherwise).
 * met2_bias_smooth: the three passes x, y, z (axis = -1) or the pass of one axis (axis = 0, 1, 2) on the two channels of `in`, with the
 *   caller's radii and weights: radius[3], each in 0..64; weights = w_x[2 r_x + 1], w_y[2 r_y + 1], w_z[2 r_z + 1] one after the other (all
 *   three even when one axis is asked for).  out[i] = sum_t w[t + r] in[i + t] along the axis, zeros outside the volume, t ascending, each
 *   tap a fused multiply-add.  out may be in.
 * met2_bias_update (update, bmean, bmean_final, recentre): b += S_R / S_W where S_W > 0 (smoothed[i] = (S_R, S_W)); *bmean_out = the mean of
 *   that b over idx[0..N) (NULL allowed; 0 when N = 0, and b is then not recentred); b -= that mean where S_W > 0.  b is updated in place and
 *   untouched elsewhere.
 * met2_bias_apply: field = exp(b) (NULL allowed), out = v / field where v is finite, a non-finite v copied through; out must not be v.
 * The checks and codes are those of met2_bias_field where they apply; n < 1 (but for met2_bias_domain and met2_bias_apply, which return
 * MET2_OK at once for n = 0), N outside 0..n and axis outside -1..2 are MET2_E_INVALID; all before any launch. */
int met2_bias_weights(double fwhm_mm, const double voxel_mm[3], int32_t *radius_out, double *weights_out);
int met2_bias_domain(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const uint8_t *mask, double *y, int32_t *idx,
                     int64_t *n_domain, void *stream);
int met2_bias_init(int32_t device, int64_t n, const double *y, const int32_t *idx, int64_t n_domain, int32_t n_class, double *stats_out,
                   uint32_t *hist_out, double *ss_part_out, double *classes_out, void *stream);
int met2_bias_em(int32_t device, int64_t n, const double *y, const double *b, const int32_t *idx, int64_t n_domain, int32_t n_class,
                 const double *classes_in, int32_t n_em, double *part_out, double *classes_out, double *rw_out, void *stream);
int met2_bias_smooth(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *in, const int32_t radius[3], const double *weights,
                     int32_t axis, double *out, void *stream);
int met2_bias_update(int32_t device, int64_t n, double *b, const double *smoothed, const int32_t *idx, int64_t n_domain, double *bmean_out,
                     void *stream);
int met2_bias_apply(int32_t device, int64_t n, const double *v, const double *b, double *out, double *field, void *stream);

/* Tissue segmentation of a 3-D map (segment='yes'; the second purpose of step 5 of the reference's example pipeline, whose
 * `fast -t 3 -n 3 -H 0.1 -I 4 -l 20.0 -b` also writes a segmentation of the total water content map).  The hidden-Markov-random-field EM of
 * Zhang, Brady & Smith (IEEE TMI 20:45-57, 2001): Gaussian classes in log intensity, a Potts prior over the six face neighbours, labels by
 * iterated conditional modes (ICM).  Stated here from the paper; none of FSL's program text is used and parity with `fast` itself is
 * unpinned.  The outputs are hard labels and class posteriors, fast's _seg and _prob_k; its _pve_k are met2_partial_volume's, below.
 * DEVICE pointers: v [nx][ny][nz] fp64 in C order (the driver passes the bias-corrected map); mask [nx][ny][nz] uint8 or NULL (every voxel);
 * out, each may be NULL: seg [nx][ny][nz] uint8, prob [K][nx][ny][nz] fp64, classes [3 K] fp64.  HOST: voxel_mm[3] = (dx, dy, dz) in mm.
 * K = n_class (the script: 3), beta (-H 0.1), n_outer (4), n_em (10), n_icm (8).
 *   1. Domain, log, initial classes: steps 1 and 2 of met2_bias_field (Omega, N, y = log v, the histogram initialisation), then n_em EM steps
 *      of its step 3 with b = 0.  The same kernels through the same host code.
 *   2. Class constants, on the device: a_k = 1 / (2 var_k) (2 var_k is exact, so one rounding), h_k = 0.5 log var_k.  A class with pi_k = 0 is
 *      dead: its energy is +inf, it is never chosen and its posterior is 0.
 *   3. Initial labels: x_i = argmin_k D_ik over the live classes, D_ik = ((y_i - mu_k)^2 a_k) + h_k; ties go to the lowest k; off Omega the
 *      label is 255.
 *   4. Neighbourhood: the six face neighbours that lie inside the volume and in Omega.  Axis weight w_a = d_min / d_a, d_min = min(dx, dy, dz)
 *      (thick slices couple less), made on the host.  P_ik = beta ((w_x c_x + w_y c_y) + w_z c_z), c_a in {0, 1, 2} the number of that axis'
 *      Omega-neighbours whose label differs from k.
 *   5. ICM, n_icm sweeps, always all of them (a converged sweep changes nothing; no counter is read back).  A sweep visits every voxel of
 *      Omega with (ix + iy + iz) even, then every one with it odd; a visit sets x_i = argmin_k (D_ik + P_ik) over the live classes, ties to the
 *      lowest k.  Voxels of one colour are not neighbours of each other: a colour pass is one launch and its result does not depend on the
 *      order of the threads.  Every operation of D_ik + P_ik rounds once, in the order written (d = y - mu; (d d) a; + h; the products w_a c_a;
 *      their sums left to right; beta times that; D + P), and none is fused into a multiply-add: given the device's mu_k, a_k, h_k, numpy
 *      gives every energy to the bit.
 *   6. Posterior given the labels: p_ik = exp(m_i - E_ik) / sum_k exp(m_i - E_ik) over the live classes, k ascending, E_ik = D_ik + P_ik,
 *      m_i = min_k E_ik.
 *   7. M-step with those p_ik: the formulas and the fixed summation tree of met2_bias_field's M-step (the same kernel) on the sums of p_k,
 *      p_k y and (p_k (y - mu_k)) (y - mu_k), each term rounded operation by operation, in the E-step's layout of entries and partials;
 *      pi_k = s_k / N.
 *   8. n_outer times: steps 2, 5, 6, 7; the labels carry over.  After the last M-step steps 2, 5 and 6 once more for the outputs.
 * Outputs: classes are numbered by ascending mu_k (rank_k = the number of j with mu_j < mu_k, or mu_j == mu_k and j < k; dead classes take
 * part with the mean they kept): seg = rank + 1 on Omega and 0 off it, so in a water-content map 1 is the driest tissue and K the wettest;
 * prob [rank] = the posteriors, 0 off Omega; classes = mu[K], var[K], pi[K], each in rank order.
 * N = 0 or hi == lo: seg = 1 on Omega, prob[0] = 1 on Omega and the other rows 0, classes as met2_bias_field's (mu = lo, var = 0,
 * pi = 1 / K); MET2_OK.
 * MET2_E_INVALID: a negative dimension, K < 1, n_outer < 0, n_em < 1, n_icm < 0, voxel_mm NULL, a voxel size that is not positive and finite,
 * beta negative or not finite, v NULL.  MET2_E_UNSUPPORTED: K > 8, 2^31 voxels or more.  All of them before any launch; the outputs are then
 * untouched.  A volume with a zero-sized dimension returns MET2_OK at once (after the checks of the dimensions' signs, K, n_outer, n_em,
 * n_icm, voxel_mm and beta).
 * Deterministic: the sums are those of met2_bias_field (memory order, fixed tree), a colour pass does not depend on the order of its threads,
 * and nothing else is shared between voxels; so the result is the same bits from run to run, does not depend on the launch geometry or the
 * tiling, and does not change when the volume is embedded in a larger one whose added voxels are outside the mask.  The host reads nothing
 * back during the call.  BLOCKING: the entry allocates its own work space (22 bytes per voxel, and 8 K more when prob is asked for),
 * enqueues every launch on `stream` -- 7 + 2 n_em + 2 + n_outer (2 n_icm + 3) + 2 n_icm + 2 of them -- waits and frees the space. */
int met2_tissue_segment(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const uint8_t *mask, const double voxel_mm[3],
                        int32_t n_class, double beta, int32_t n_outer, int32_t n_em, int32_t n_icm, uint8_t *seg, double *prob, double *classes,
                        void *stream);

/* The stages of met2_tissue_segment one by one, for tests and diagnostics, after the pattern of met2_bias_*: each launches the production
 * kernels through the host code met2_tissue_segment itself runs, on input the caller supplies, allocates and frees what it needs and BLOCKS.
 * Steps 1 and 7 are met2_bias_domain, met2_bias_init and met2_bias_em (b = 0) and the M-step's sum (met2_bias_em's note).  n = the voxels,
 * N = n_domain, np = ceil(N / 1024), K = n_class.  DEVICE pointers: y [n] fp64; idx [n] int32; labels [n] uint8 (a class 0..K-1 on Omega,
 * 255 off it); prob_out, prob_raw, prob [K][n] fp64; seg [n] uint8.  HOST pointers: everything else; classes_in [3 K] = mu, var, pi with
 * finite mu, finite var > 0 and finite pi >= 0.  idx[0..N) must hold voxel indices in [0, n), unchecked.  Additive: MET2_ABI_VERSION stays 6.
 *
 * met2_seg_consts: step 2; a_out [K], h_out [K], live_out [K] (1, or 0 for a dead class); each may be NULL.
 * met2_seg_init: step 3; labels: all n written, 255 off idx[0..N).
 * met2_seg_icm: step 5 in place on labels, with the caller's axis weights w[3] (finite, >= 0) and beta.  colour = -1: n_sweeps sweeps;
 *   colour = 0 or 1: that colour pass of one sweep (none when n_sweeps = 0).  Omega is where labels != 255: the stencil needs no list.
 * met2_seg_posterior: step 6 on idx[0..N), N >= 1; prob_out (NULL allowed) [k][i] = p_ik in the order of classes_in, all K n written, 0 off
 *   the list; part_out (NULL allowed) [3][K][np]: per chunk of 1024 list entries the sums of p_k, p_k y and (p_k d) d, d = y - mu_k, every
 *   operation rounded once, added in the order of met2_bias_em's note.
 * met2_seg_finish: the rank by mu, seg, prob (NULL allowed; needs prob_raw, the posteriors in the order of classes_in) and classes_out
 *   [3 K] in rank order (NULL allowed).  A label that is no class gives seg = 0 and prob = 0.
 * The checks and codes are those of met2_tissue_segment where they apply; a volume without a voxel, N outside 0..n (1..n for the posterior),
 * n_sweeps < 0, colour outside -1..1 and a bad weight are MET2_E_INVALID; all before any launch. */
int met2_seg_consts(int32_t device, int32_t n_class, const double *classes_in, double *a_out, double *h_out, int32_t *live_out, void *stream);
int met2_seg_init(int32_t device, int64_t n, const double *y, const int32_t *idx, int64_t n_domain, int32_t n_class, const double *classes_in,
                  uint8_t *labels, void *stream);
int met2_seg_icm(int32_t device, int32_t nx, int32_t ny, int32_t nz, uint8_t *labels, const double *y, int32_t n_class, const double *classes_in,
                 const double w[3], double beta, int32_t n_sweeps, int32_t colour, void *stream);
int met2_seg_posterior(int32_t device, int32_t nx, int32_t ny, int32_t nz, const uint8_t *labels, const double *y, const int32_t *idx,
                       int64_t n_domain, int32_t n_class, const double *classes_in, const double w[3], double beta, double *prob_out,
                       double *part_out, void *stream);
int met2_seg_finish(int32_t device, int64_t n, const uint8_t *labels, const double *prob_raw, int32_t n_class, const double *classes_in,
                    uint8_t *seg, double *prob, double *classes_out, void *stream);

/* Partial-volume tissue maps of a segmented 3-D map (segment='pve'; what the reference's `fast` call of step 5 writes by default: _pve_k,
 * _pveseg and _mixeltype).  The mixel model of Santago & Gage (Quantification of MR brain images by mixture density and partial volume
 * modeling, IEEE TMI 12:566-574, 1993) as Shattuck et al. (NeuroImage 13:856-876, 2001) and Tohka, Zijdenbos & Evans (NeuroImage 23:84-97,
 * 2004) use it: a voxel is pure tissue or a mixture of two tissues, a mixture's likelihood is the Gaussian of the mixed intensity
 * marginalised over a uniform fraction, a Potts-like prior over the six face neighbours couples the types, and the fraction of a mixed
 * voxel is Tohka's closed form.  Stated here from the papers; none of FSL's program text is used and parity with `fast` itself is unpinned.
 * It runs after met2_tissue_segment, on its outputs.
 * DEVICE pointers: v [nx][ny][nz] fp64 in C order (the map that was segmented); seg [n] uint8 and prob [K][n] fp64 exactly as
 * met2_tissue_segment writes them (rank order, 0 off Omega); out, each may be NULL: pve [K][n] fp64, pveseg [n] uint8, mixeltype [n] uint8,
 * classes_lin [3 K] fp64.  HOST: voxel_mm[3] = (dx, dy, dz) in mm.  K = n_class (the script: 3), beta_pv (fast's -R, default 0.3, which the
 * script leaves alone), n_icm (8).  n = nx ny nz; Omega = the voxels with seg != 0, N of them.
 *   1. Class moments in LINEAR intensity (partial volume mixes intensities, not their logs): s_k = sum p_ik, mu_k = (sum p_ik v_i) / s_k;
 *      then, in a second pass, var_k = (sum (p_ik d) d) / s_k with d = v_i - mu_k; pi_k = s_k / N.  The sums run over the compacted list of
 *      Omega in memory order, in the fixed tree of met2_bias_em's note (chunks of 1024 list entries, then the partials); every term is
 *      rounded operation by operation.  A class with s_k = 0 gets mu_k = var_k = pi_k = 0.  A class is DEAD when s_k = 0 or var_k is not
 *      finite and positive.
 *   2. Mixel types: t = 0..K-1 are pure; t = K + j (j = 0..K-2) is a mixture of the rank-adjacent classes j and j + 1; T = 2 K - 1 <= 15.
 *      A mixture is dead when either member is dead or mu_{j+1} - mu_j is not positive.
 *   3. Constants, on the device.  Pure: a_k = 1 / (2 var_k), h_k = 0.5 log var_k.  Every mixture has 64 midpoint nodes
 *      alpha_m = (m + 0.5) / 64: m_jm = alpha_m mu_j + (1 - alpha_m) mu_{j+1}, s_jm = alpha_m^2 var_j + (1 - alpha_m)^2 var_{j+1},
 *      a_jm = 1 / (2 s_jm), h_jm = 0.5 log s_jm: a table [K-1][64][3] = (m, a, h), the same for every voxel, which the energy kernel reads
 *      from LDS.  The entries of a dead class or mixture are 0.
 *   4. Energies, once, E [T][n].  Pure: E = ((d d) a_k) + h_k, d = v - mu_k.  Mixed: q_m = (((v - m_jm)^2) a_jm) + h_jm, q* = min_m q_m,
 *      S = sum_m exp(q* - q_m) with m ascending, E = q* - log(S / 64): minus the log of the likelihood marginalised over the fraction by the
 *      midpoint rule.  The common log(2 pi) / 2 is dropped.  No operation is fused into a multiply-add.  A dead type has E = +inf.
 *      The midpoint rule needs (mu_{j+1} - mu_j) / 64 small against the classes' standard deviations, which holds for any map whose classes
 *      can be told apart at all.
 *   5. Initial types: t_i = argmin_t E_it over the live types, ties to the lowest t; off Omega the type is 255.  When no type is live,
 *      t_i = seg_i - 1 and the sweeps change nothing.
 *   6. Prior and ICM.  The six face neighbours inside the volume and Omega, axis weights w_a = d_min / d_a made on the host, as in
 *      met2_tissue_segment.  The distance of two types, doubled so that it is an integer: delta2(t, u) = 0 for t = u, 1 when their member
 *      sets ({k} for pure k, {j, j + 1} for mixture j) intersect, 2 otherwise.  c_a = the sum of delta2(t, type of the neighbour) over that
 *      axis' Omega-neighbours, 0..4.  P_it = (beta_pv ((w_x c_x + w_y c_y) + w_z c_z)) 0.5, rounded in the order written.  n_icm checkerboard
 *      sweeps in met2_tissue_segment's schedule (step 5 there: all of them, nothing read back, one launch per colour): a visit sets
 *      t_i = argmin_t (E_it + P_it) over the live types, ties to the lowest t.  Given E, numpy gives every decision to the bit.
 *   7. Outputs.  Pure type k: pve_k = 1, the others 0.  Mixture j: alpha = min(max((mu_{j+1} - v) / (mu_{j+1} - mu_j), 0), 1), pve_j = alpha,
 *      pve_{j+1} = 1 - alpha (Tohka's estimator: the maximum-likelihood fraction for equal variances).  pve = 0 off Omega.
 *      pveseg = 1 + argmax_k pve_k, ties to the lowest k, 0 off Omega.  mixeltype = t, 255 off Omega.  classes_lin = mu[K], var[K], pi[K].
 * An empty Omega: pve = 0, pveseg = 0, mixeltype = 255, classes_lin = 0; MET2_OK.  A volume with a zero-sized dimension returns MET2_OK at
 * once (after the checks of the dimensions' signs, K >= 1, n_icm, voxel_mm and beta_pv) and writes nothing.
 * MET2_E_INVALID: a negative dimension, K < 1, n_icm < 0, voxel_mm NULL, a voxel size that is not positive and finite, beta_pv negative or
 * not finite, v, seg or prob NULL.  MET2_E_UNSUPPORTED: K > 8, 2^31 voxels or more.  All of them before any launch; the outputs are then
 * untouched.
 * Deterministic: the sums are taken in memory order in a fixed tree, a colour pass does not depend on the order of its threads and nothing
 * else is shared between voxels; so the result is the same bits from run to run, does not depend on the launch geometry or the tiling, and
 * does not change when the volume is embedded in a larger one whose added voxels have seg = 0, at an offset (ox, oy, oz) with ox + oy + oz
 * even (the colours of a sweep are those of the absolute coordinates: at an odd offset its two passes change places, which can settle a
 * few voxels differently).  The host reads nothing back during the call.  BLOCKING: the entry allocates its own work space
 * (8 (2 K - 1) + 5 bytes per voxel: E, the list and the types), enqueues every launch on `stream` -- 10 + 2 n_icm of them (3 for the list,
 * 4 for the moments, the constants, the energies, the passes, the outputs) -- waits and frees the space. */
int met2_partial_volume(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const uint8_t *seg, const double *prob,
                        const double voxel_mm[3], int32_t n_class, double beta_pv, int32_t n_icm, double *pve, uint8_t *pveseg,
                        uint8_t *mixeltype, double *classes_lin, void *stream);

/* The stages of met2_partial_volume one by one, for tests and diagnostics, after the pattern of met2_seg_*: each launches the production
 * kernels through the host code met2_partial_volume itself runs, on input the caller supplies, allocates and frees what it needs and BLOCKS.
 * n = the voxels, K = n_class, T = 2 K - 1, nch = ceil(n / 1024), N = the voxels with seg != 0, np = ceil(N / 1024).  DEVICE pointers: v [n]
 * fp64; seg, types, pveseg, mixeltype [n] uint8; prob, pve [K][n] fp64; E, E_out [T][n] fp64.  HOST pointers: everything else; classes_in
 * [3 K] = mu, var, pi in linear intensity, any values (step 1's rule says which classes are dead).  Additive: MET2_ABI_VERSION stays 6.
 *
 * met2_pve_moments: step 1 (the list of seg != 0, then the two passes).  Each may be NULL: *n_domain = N; part_out [3][K][nch], of which
 *   the first np of every row are written: per chunk of 1024 list entries the sums of p_k, p_k v and (p_k d) d, added in the order of
 *   met2_bias_em's note; classes_out [3 K] = mu, var, pi.
 * met2_pve_consts: steps 2 and 3; a_out [K], h_out [K], live_out [T] (1, or 0 for a dead type), table_out [K-1][64][3]; each may be NULL.
 * met2_pve_energy: steps 2 to 5 on the list of seg != 0; E_out: all T n written, 0 off the list; types_out (NULL allowed): all n written,
 *   255 off the list.
 * met2_pve_icm: step 6 in place on types, given E, the live flags live_in [T], the caller's axis weights w[3] (finite, >= 0) and beta_pv.
 *   colour = -1: n_sweeps sweeps; colour = 0 or 1: that colour pass of one sweep (none when n_sweeps = 0).  Omega is where types != 255; E
 *   is read there only.  A type must be 0..T-1 or 255.
 * met2_pve_finish: step 7 from types and the means of classes_in; pve, pveseg, mixeltype: each may be NULL.  A type that is none of 0..T-1
 *   counts as off Omega.
 * The checks and codes are those of met2_partial_volume where they apply; a volume without a voxel, a NULL input, n_sweeps < 0, colour
 * outside -1..1 and a bad weight are MET2_E_INVALID; all before any launch. */
int met2_pve_moments(int32_t device, int64_t n, const double *v, const uint8_t *seg, const double *prob, int32_t n_class, int64_t *n_domain,
                     double *part_out, double *classes_out, void *stream);
int met2_pve_consts(int32_t device, int32_t n_class, const double *classes_in, double *a_out, double *h_out, int32_t *live_out,
                    double *table_out, void *stream);
int met2_pve_energy(int32_t device, int64_t n, const double *v, const uint8_t *seg, int32_t n_class, const double *classes_in, double *E_out,
                    uint8_t *types_out, void *stream);
int met2_pve_icm(int32_t device, int32_t nx, int32_t ny, int32_t nz, uint8_t *types, const double *E, int32_t n_class, const int32_t *live_in,
                 const double w[3], double beta_pv, int32_t n_sweeps, int32_t colour, void *stream);
int met2_pve_finish(int32_t device, int64_t n, const double *v, const uint8_t *types, int32_t n_class, const double *classes_in, double *pve,
                    uint8_t *pveseg, uint8_t *mixeltype, void *stream);

/* Per-label statistics of maps and spectra (tissue_stats='yes'; additive, ABI stays 6): what turns the maps, a label volume (the tissue
 * classes of met2_tissue_segment, a thresholded met2_partial_volume map, an atlas ROI image) and the spectra into "MWF in white matter:
 * mean, SD, median, quartiles", and the per-tissue mean spectrum the reference leaves as a TO DO (motor/motor_recon_met2_real_data.py:
 * 375-376).  No plan: `device` and `stream` only.  DEVICE pointers except q_host.
 * Inputs.  label [nvox], int32: a value in [0, n_label) makes the voxel a member of that label, anything else a non-member.  Series s of
 * voxel v is values[v voxel_stride + s series_stride], fp64, strides in doubles and > 0: maps are series-major ([S][nvox]: voxel_stride 1,
 * series_stride nvox), spectra voxel-major ([nvox][n_t2]: voxel_stride n_t2, series_stride 1); both are read in place, along their
 * contiguous axis.
 * Per (label, series) the sample is the members' values that are not NaN (+-inf is outside the contract, as for
 * met2_bootstrap_series_stats):
 *   n            the sample size, as a double
 *   mean         the sample mean
 *   std          ddof = 1, two passes (the second around the mean); 0 for n = 1
 *   quantile[j]  np.quantile(sample, q[j], method='linear') to the bit: h = (n - 1) q, the order statistics floor(h) and floor(h) + 1,
 *                numpy's _lerp with its t >= 0.5 branch, no contraction (quantile.hpp, the implementation the bootstrap statistics use)
 * -0.0 counts as +0.0.  n = 0 gives n = 0 and NaN for everything else (a zero in a table would read as a measurement).  Nothing depends on
 * floating-point atomics: two runs give the same bits.  n and the quantiles do not depend on the order of the voxels either; the sums of
 * mean and std run in the order of the member list -- chunks of MET2_STATS_CHUNK members, in a chunk 256 chains of 64 additions and a
 * binary tree over them, the chunks of a label again by 256 chains (at most 512 long) and the tree -- so no chain is longer than 512
 * terms: |mean error| <= 1e-13 max|v|, |std error| <= 1e-12 std + 1e-13 max|v|.
 *   met2_label_index      the member list: order [nvox] holds the members' voxel indices grouped by ascending label, inside a label by
 *                         ascending voxel index; offset [n_label + 1] the start of every label's group, offset[n_label] the member
 *                         count.  A counting sort in integers (histogram, scan, stable scatter).
 *   met2_label_moments    out [n_label][n_series][3] = n, mean, std
 *   met2_label_quantiles  out [n_label][n_series][n_q]; q_host [n_q] on the HOST, 1 <= n_q.  The series are gathered tile by tile into
 *                         a dense matrix of sortable 64-bit keys (at most 256 MiB a tile, one series at least); labels of at most
 *                         MET2_STATS_SMALL_N members are sorted in LDS, the others selected by most-significant-digit radix, 8 levels of
 *                         8 bits, all ranks of all (label, series) segments of a tile per pass, the bookkeeping on the device.
 *   met2_label_stats      the three in one call: out [n_label][n_series][3 + n_q] = n, mean, std, quantiles; n_q = 0 is allowed.
 * Each allocates and frees what it needs and BLOCKS.  Limits: nvox < 2^31, n_label <= MET2_STATS_MAX_LABEL, n_series <=
 * MET2_STATS_MAX_SERIES, n_q <= MET2_STATS_MAX_Q (MET2_E_UNSUPPORTED beyond).  MET2_E_INVALID: n_label or n_series < 1, nvox < 0, a
 * stride that is not positive, a probability outside [0, 1] or NaN, a NULL required pointer, offsets that decrease or do not start at 0.
 * The parameter checks come before any read of device memory.  met2_label_stats_limits (host only) returns the five constants; any
 * output may be NULL. */
#define MET2_STATS_CHUNK 16384
#define MET2_STATS_SMALL_N 1024
#define MET2_STATS_MAX_LABEL 4096
#define MET2_STATS_MAX_SERIES 32768
#define MET2_STATS_MAX_Q 16
int met2_label_stats_limits(int32_t *chunk, int32_t *small_n, int32_t *max_label, int32_t *max_series, int32_t *max_q);
int met2_label_index(int32_t device, int64_t nvox, const int32_t *label, int32_t n_label, int32_t *offset, int32_t *order, void *stream);
int met2_label_moments(int32_t device, int32_t n_label, const int32_t *offset, const int32_t *order, int32_t n_series, const double *values,
                       int64_t voxel_stride, int64_t series_stride, double *out, void *stream);
int met2_label_quantiles(int32_t device, int32_t n_label, const int32_t *offset, const int32_t *order, int32_t n_series, const double *values,
                         int64_t voxel_stride, int64_t series_stride, int32_t n_q, const double *q_host, double *out, void *stream);
int met2_label_stats(int32_t device, int64_t nvox, const int32_t *label, int32_t n_label, int32_t n_series, const double *values,
                     int64_t voxel_stride, int64_t series_stride, int32_t n_q, const double *q_host, double *out, void *stream);

/* Affine resampling of volumes and label images (an extension; additive, ABI stays 6): what brings an atlas ROI image onto the grid of the
 * maps, or the maps into a template space, through a GIVEN transform (estimating one: met2_register_cost below scores candidates, register.py searches).  It is
 * scipy.ndimage.affine_transform(src, A[:, :3], offset=A[:, 3], output_shape=dst, mode='constant', cval=cval), restated; no plan: `device`
 * and `stream` only.  All arithmetic is fp64 and no product is fused into a sum: every operation below rounds once, in the order written.
 * Shapes.  The source grid is [nx][ny][nz] (src_dims), the destination grid [mx][my][mz] (dst_dims), both in C order, z fastest; series s
 * of source voxel v = (x ny + y) nz + z is src[v src_voxel_stride + s src_series_stride], of destination voxel w
 * dst[w dst_voxel_stride + s dst_series_stride], strides in elements and > 0: series-major maps [S][x][y][z] have voxel stride 1 and series
 * stride nvox, voxel-major echo data [x][y][z][S] voxel stride S and series stride 1; both are read and written in place.
 * Transform.  A [12] on the HOST, row-major 3 x 4, finite: destination voxel (i, j, k) lies at the continuous source coordinates
 *     c_a = ((A[a][3] + A[a][0] i) + A[a][1] j) + A[a][2] k,   a = x, y, z   (four roundings after the three products; i, j, k as doubles)
 *   Inside.  The voxel is inside when 0 <= c_a <= n_a - 1 on all three axes (a NaN coordinate is outside).  An outside voxel gets cval in
 *     every series (the fill label for labels) and inside = 0; nothing is extrapolated.  inside [mx][my][mz] uint8 may be NULL.
 *   Order 0.  The sample at floor(c_a + 0.5) per axis.
 *   Order 1.  f = floor(c), t = c - f (exact), weights w = (1 - t, t) for the taps f, f + 1 per axis;
 *     out = sum_p sum_q sum_r ((wx_p wy_q) wz_r) v[p][q][r], p outermost, each ascending, starting from the first term.
 *   Order 3.  The cubic B-spline on the coefficients of the prefilter below: taps f - 1 .. f + 2, weights, with u = 1 - t,
 *     (u u u / 6, ((3 t - 6) t t + 4) / 6, ((3 u - 6) u u + 4) / 6, t t t / 6); the 64 terms are added in the nesting of order 1.
 *   Taps off the line.  A tap m outside 0 .. n - 1 is mirrored about the end samples (whole-sample symmetric): m mod 2 (n - 1), and
 *     2 (n - 1) minus that where it exceeds n - 1; for n = 1 every tap is sample 0.  (Only orders 1 and 3 have such taps, and only next to a face.)
 *   Prefilter (order 3), per axis in the order x, y, z, every line of n > 1 samples on its own, a line of one sample left as it is:
 *     z1 = sqrt(3) - 2, lambda = (1 - z1)(1 - 1 / z1), zn = z1^(n - 1) (pow on the host); x_i = lambda s_i;
 *     c_0 = x_0 + zn x_(n-1); for i = 1 .. n - 2, p = z1^i by repeated multiplication: c_0 += p (x_i + zn x_(n-1-i)); c_0 /= 1 - zn zn
 *       (the sum over the mirrored, periodic line, exact: nothing is truncated);
 *     c_i = x_i + z1 c_(i-1), i = 1 .. n - 1;   c_(n-1) = (z1 c_(n-2) + c_(n-1)) z1 / (z1 z1 - 1);   c_i = z1 (c_(i+1) - c_i), i = n - 2 .. 0.
 *     This is Unser's recursive filter (IEEE TSP 41:821-848, 1993) as scipy.ndimage.spline_filter(mode='mirror') runs it.
 * Entries.  DEVICE pointers except A.
 *   met2_resample            order 0, 1 or 3.  For order 3 the coefficient volumes of a chunk of series live in a device block of at most
 *                            max_work_bytes (0: the default) that the entry allocates and frees; the series go through a chunk at a time,
 *                            and every (voxel, series) gets the same bits whatever the chunking.  BLOCKING for order 3; orders 0 and 1
 *                            allocate nothing and are asynchronous on `stream`.
 *   met2_resample_work_bytes (host only) min_bytes = one series' coefficients, 8 nx ny nz; default_bytes = all series', capped at 2^30 bytes
 *                            but never below min_bytes; both 0 for orders 0 and 1.
 *   met2_resample_labels     int32 labels, order 0, fill where outside.  Asynchronous on `stream`.
 *   met2_resample_prefilter  the stage entry: coef [n_series][nx][ny][nz] = the prefilter of every series, nothing else.  Asynchronous.
 * Limits.  Source axes 1 .. MET2_RESAMPLE_MAX_AXIS, destination axes >= 1 with at most 2^31 - 1 voxels in all, 1 <= n_series <=
 * MET2_RESAMPLE_MAX_SERIES (MET2_E_UNSUPPORTED beyond the upper ends).  MET2_E_INVALID: an axis or n_series < 1, an order other than 0, 1, 3,
 * a stride < 1, destination strides under which two (voxel, series) pairs share an element (neither dst_series_stride >= nvox
 * dst_voxel_stride nor dst_voxel_stride >= n_series dst_series_stride), a NULL required pointer, dst == src, an entry of A that is not
 * finite, max_work_bytes < 0 or (order 3) > 0 and below min_bytes.  Every check comes before any device work: the outputs are then untouched.
 * Deterministic: no atomics, one thread per output element. */
#define MET2_RESAMPLE_MAX_AXIS 512
#define MET2_RESAMPLE_MAX_SERIES 32768
int met2_resample(int32_t device, int32_t order, const int32_t src_dims[3], int32_t n_series, const double *src, int64_t src_voxel_stride,
                  int64_t src_series_stride, const int32_t dst_dims[3], const double A[12], double cval, double *dst, int64_t dst_voxel_stride,
                  int64_t dst_series_stride, uint8_t *inside, int64_t max_work_bytes, void *stream);
int met2_resample_work_bytes(int32_t order, const int32_t src_dims[3], int32_t n_series, int64_t *min_bytes, int64_t *default_bytes);
int met2_resample_labels(int32_t device, const int32_t src_dims[3], const int32_t *labels, const int32_t dst_dims[3], const double A[12],
                         int32_t fill, int32_t *out, uint8_t *inside, void *stream);
int met2_resample_prefilter(int32_t device, const int32_t src_dims[3], int32_t n_series, const double *src, int64_t src_voxel_stride,
                            int64_t src_series_stride, double *coef, void *stream);

/* The cost function of rigid / affine registration (an extension; additive, ABI stays 6): how well a MOVING volume, resampled through each of
 * K candidate transforms, matches a FIXED volume -- all K in one launch.  The search that proposes the candidates is register.py's; the
 * library only scores them.  No plan: `device` and `stream` only.  DEVICE pointers except the dims, the ranges and A.
 * Sampling.  Candidate k is A[k][12] on the HOST, in the convention of met2_resample with the fixed grid [mx][my][mz] as the destination and
 *   the moving grid [nx][ny][nz] as the source: fixed voxel (i, j, k) lies at c_a = ((A[a][3] + A[a][0] i) + A[a][1] j) + A[a][2] k, is
 *   inside when 0 <= c_a <= n_a - 1 on all three axes, and its moving value y is met2_resample's order 1 there, mirrored taps and n = 1 axes
 *   included, to the bit (the two share their device code).  fp64 throughout, no product fused into a sum.
 * Bins.  fixed_bin [mx my mz] int32: 0 .. n_bins - 1, anything else (use -1) excludes the voxel -- this is how a mask enters.  Only the fixed
 *   image is binned, once per image, by met2_register_index: the included voxels grouped by ascending bin, inside a bin by ascending voxel
 *   index (met2_label_index), and cut into RUNS of MET2_REGISTER_RUN consecutive members of one bin, the last run of a bin shorter.
 *   n_included is their number.  normcorr and leastsq take the same index; they read x = fixed[v] besides.
 * Sums.  Per candidate, over the included voxels that are inside (n_inside of them), of d = y - cy and e = x - cx, where the shifts
 *   cy = lo + (hi - lo) / 2 of moving_range = (lo, hi) and cx of fixed_range are fixed per call (the ranges are the caller's: the minimum and
 *   maximum of the volumes, or any finite lo <= hi; a shift only moves where cancellation sets in, in exact arithmetic the cost is the same):
 *   per run, slot t of the run's 256 (absent and outside members are zeros): within each group of 64 slots, for s = 32, 16, .., 1 slot t
 *   takes slot t + s, then the four groups as (g0 + g1) + (g2 + g3); per bin, the runs r = l, l + 64, l + 128, ... of the bin are added in
 *   ascending order for l = 0 .. 63, and the 64 chains go through the same group tree; over the bins, slot b of 256 (bins beyond n_bins are
 *   zeros) through the tree of a run.  No floating-point atomics; the counts are integers.  A candidate's n_inside and cost therefore have the
 *   same bits from call to call, whatever K is and wherever the candidate stands in A.
 *   C(q, s, n) = max(q - s s / n, 0) is n times a variance from the shifted sums.
 *   MET2_REGISTER_CORRATIO  per bin n_b, S_b = sum d, Q_b = sum d d; cost = min((sum_b C(Q_b, S_b, n_b)) / C(Q, S, n_inside), 1), the sum over
 *                           the bins with n_b > 0 by the tree: sum_b n_b Var_b(y) / (n_inside Var(y)), the correlation ratio (Roche et al.,
 *                           MICCAI 1998), flirt's default.  `fixed` and fixed_range may be NULL.
 *   MET2_REGISTER_NORMCORR  1 - r r, r r = min(c c / (vx vy), 1) with c = Sde - Se Sd / n, vx = C(See, Se, n), vy = C(Sdd, Sd, n); not below 0.
 *   MET2_REGISTER_LEASTSQ   (sum (x - y)(x - y)) / n_inside.  No shifts are taken; `fixed` is read, fixed_range may be NULL.  (moving_range is required for every
 *                           kind: the zero-variance rule and the shift come from it.)
 * Worst value.  A candidate with n_inside = 0 or n_inside < min_overlap n_included (as doubles, one product), or whose variance is zero where a
 *   ratio needs one -- C(..) <= n_inside 1e-24 m m with m = max(|lo|, |hi|) of that volume's range: a constant volume interpolates to itself up
 *   to rounding --, gets 1 (corratio, normcorr) or MET2_REGISTER_LEASTSQ_WORST (leastsq).  A cost is never NaN for finite volumes.
 * Entries.
 *   met2_register_limits      (host only) the five constants; any output may be NULL
 *   met2_register_work_bytes  (host only) index_bytes = 4 (2 (n_bins + 1) + mx my mz); cost_bytes = 96 K + 44 K (ceil(mx my mz / 256) + n_bins):
 *                             the transforms, and per (candidate, run) five sums and a count
 *   met2_register_index       fills `index` (index_bytes at least; 4-byte aligned) from fixed_bin.  BLOCKS (met2_label_index does).
 *   met2_register_cost        n_inside [K] int64 and cost [K] of the K candidates; `work` (cost_bytes at least, 8-byte aligned) is scratch that
 *                             must not be shared by calls on different streams.  Asynchronous on `stream`: the transforms go to the head of `work` by a copy enqueued on `stream`, so A
 *                             must stay valid and unchanged until the work this call enqueued has completed (wait for `stream`, or for
 *                             an event recorded after the call), like every host array of an asynchronous entry.
 * Limits.  Fixed and moving axes 1 .. MET2_REGISTER_MAX_AXIS, 1 <= n_bins <= MET2_REGISTER_MAX_BINS, 1 <= K <= MET2_REGISTER_MAX_K
 * (MET2_E_UNSUPPORTED beyond the upper ends).  MET2_E_INVALID: an axis, n_bins or K < 1, an unknown kind, a NULL required pointer, a range
 * that is not finite or has lo > hi, an entry of A that is not finite, min_overlap outside [0, 1] or NaN, a work space or index that is too
 * small or misaligned.  Every check comes before any device work: the outputs are then untouched.
 *
 * Mutual information (met2_register_joint_cost; additive, ABI stays 6): MET2_REGISTER_MI and MET2_REGISTER_NMI assume only a statistical
 * dependence between the two images' intensities.  They have an entry of their own; met2_register_cost keeps refusing them.  The index,
 * the sampling, the copy of A to the head of `work`, min_overlap and the checks are those above.
 * Moving bin.  With moving_range = (lo, hi) and scale = (double)moving_bins / (hi - lo), formed once on the host in fp64, a sample y falls in
 *   j = min(max(floor((y - lo) scale), 0), moving_bins - 1): the subtraction and the product are two roundings, not fused.  hi = lo (or a
 *   width so small that the quotient is not finite) gives scale = 0: every sample in bin 0.  The fixed bin b is the index's.
 * Counts.  Per candidate the joint histogram n[b][j] over the included voxels that are inside, its row sums n_b, its column sums m_j and
 *   N = n_inside: integers, formed with integer atomic adds only (per run into moving_bins counters on chip, then the non-zero counters
 *   into row b of the candidate's table in `work`, which every call zeroes on `stream` first).  Integer adds commute, so the histogram is the
 *   same whatever the order of arrival, whatever K is and wherever the candidate stands in A.  No floating-point atomics.
 * Cost.  T(c) = c log(c) for c > 0 and 0 for c = 0, in fp64, one product.  Sxy = sum of T(n[b][j]): the cells of the table, flat index
 *   b moving_bins + j, in 256 chains -- chain t adds the cells t, t + 256, t + 512, ... in ascending order -- and the chains through the tree
 *   of a run (above: groups of 64 with s = 32 .. 1, then (g0 + g1) + (g2 + g3)); Sx = sum of T(n_b) with slot b of 256 through the same
 *   tree (slots beyond n_bins are zeros), Sy = sum of T(m_j) likewise.  Hxy = log N - Sxy / N, Hx = log N - Sx / N, Hy = log N - Sy / N.
 *   MET2_REGISTER_MI   min(-((Hx + Hy) - Hxy), 0): minus the mutual information
 *   MET2_REGISTER_NMI  min(-((Hx + Hy) / Hxy), -1): minus Studholme's normalised mutual information (Pattern Recognition 32:71-86, 1999),
 *                      negated as flirt's normmi is, so that smaller is better
 *   A cost has the same bits from call to call.
 * Worst value.  MET2_REGISTER_MI_WORST = 0 and MET2_REGISTER_NMI_WORST = -1 (independent images): for n_inside = 0, for n_inside < min_overlap
 *   n_included, and where every inside voxel falls in one fixed bin or in one moving bin -- some n_b = N or some m_j = N, tested on the
 *   integers.  Never NaN for finite volumes.
 * Entries.
 *   met2_register_joint_work_bytes  (host only) work_bytes = 96 K + 4 K n_bins moving_bins: the transforms and the candidates' tables
 *   met2_register_joint_cost        n_inside [K] int64 and cost [K]; `joint`, where not NULL, receives the tables, int32 [K][n_bins][moving_bins]
 *                                   (4-byte aligned), by a copy on `stream` after the costs are formed.  `work` (work_bytes at least, 8-byte
 *                                   aligned) and A as for met2_register_cost.  Asynchronous on `stream`.
 * Limits and errors as above, with 1 <= moving_bins <= MET2_REGISTER_MAX_BINS (below: MET2_E_INVALID; beyond: MET2_E_UNSUPPORTED), a kind other
 * than the two (MET2_E_INVALID) and a misaligned `joint` (MET2_E_INVALID). */
#define MET2_REGISTER_CORRATIO 0
#define MET2_REGISTER_NORMCORR 1
#define MET2_REGISTER_LEASTSQ 2
#define MET2_REGISTER_MI 3
#define MET2_REGISTER_NMI 4
#define MET2_REGISTER_RUN 256
#define MET2_REGISTER_MAX_AXIS 512
#define MET2_REGISTER_MAX_BINS 256
#define MET2_REGISTER_MAX_K 256
#define MET2_REGISTER_LEASTSQ_WORST 1.0e300
int met2_register_limits(int32_t *run, int32_t *max_axis, int32_t *max_bins, int32_t *max_k, double *leastsq_worst);
int met2_register_work_bytes(const int32_t fixed_dims[3], int32_t n_bins, int32_t K, int64_t *index_bytes, int64_t *cost_bytes);
int met2_register_index(int32_t device, const int32_t fixed_dims[3], const int32_t *fixed_bin, int32_t n_bins, void *index, int64_t index_bytes,
                        void *stream);
int met2_register_cost(int32_t device, int32_t kind, const int32_t fixed_dims[3], int32_t n_bins, const void *index, const double *fixed,
                       const double fixed_range[2], const int32_t moving_dims[3], const double *moving, const double moving_range[2], int32_t K,
                       const double *A, double min_overlap, void *work, int64_t work_bytes, int64_t *n_inside, double *cost, void *stream);
#define MET2_REGISTER_MI_WORST 0.0
#define MET2_REGISTER_NMI_WORST -1.0
int met2_register_joint_work_bytes(const int32_t fixed_dims[3], int32_t n_bins, int32_t moving_bins, int32_t K, int64_t *work_bytes);
int met2_register_joint_cost(int32_t device, int32_t kind, const int32_t fixed_dims[3], int32_t n_bins, const void *index,
                             const int32_t moving_dims[3], const double *moving, const double moving_range[2], int32_t moving_bins, int32_t K,
                             const double *A, double min_overlap, void *work, int64_t work_bytes, int64_t *n_inside, double *cost,
                             int32_t *joint, void *stream);

/* Brain extraction (brain_mask='yes'; an extension: the reference's example pipeline makes the mask on the CPU, with FSL's
 * `fslmaths -Tmean` and `bet -m -f 0.4`, example_script_run_MET2_preproc_and_recon.sh step 3).  The surface model of Smith, Fast robust
 * automated brain extraction, HBM 17:143-155, 2002 -- the model bet runs -- WITHOUT bet's self-intersection retry pass, its skull and
 * scalp surfaces and its -R / -S / -B variants; parity with bet itself is unpinned.  All arithmetic is fp64 and no product is fused into a
 * sum: every expression below rounds operation by operation as written, products before sums, left to right.  v [nx][ny][nz] (z fastest);
 * voxel (ix, iy, iz) has its centre at (ix dx, iy dy, iz dz) mm, (dx, dy, dz) = voxel_mm.
 *  0 echo mean (met2_bet_mean): v = (((d_0 + d_1) + d_2) + ... + d_{n_te-1}) / n_te per voxel; a non-finite echo leaves a non-finite v.
 *  1 robust statistics over the FINITE voxels of v, N of them (met2_bet_stats):
 *      lo, hi = their min and max; bin(x) = min(999, floor((x - lo) / (hi - lo) * 1000)); C_j = the number of voxels in bins 0 .. j;
 *      j2 = the first j with 100 C_j >= 2 N, j98 = the first with 100 C_j >= 98 N (integers); w = (hi - lo) / 1000;
 *      t2 = lo + j2 w (the bin's lower edge), t98 = lo + (j98 + 1) w (the bin's upper edge), t = t2 + 0.1 (t98 - t2);
 *      S = the finite voxels with v > t, `count` of them; weight q = min(v, t98) - t2; COG_a = (sum_S q p_a) / (sum_S q), p_a = i_a d_a;
 *      r = cbrt(3 count ((dx dy) dz) / (4 pi));
 *      tm = the median (np.median's: the mean (a + b) / 2 of the two middle values for an even number) of the voxels with t2 < v < t98 and
 *      ((p_x - COG_x)^2 + (p_y - COG_y)^2) + (p_z - COG_z)^2 <= r r; tm = t when there is none.
 *      The histogram and the median's radix selection are integer atomics.  The four sums run over chunks of 1024 consecutive voxels in
 *      memory order: in a chunk thread h of 256 adds voxels h, 256 + h, 512 + h, 768 + h in that order, a butterfly (xor 32, 16, .. 1) adds the
 *      64 lanes of a wave, the four waves add as (0 + 1) + (2 + 3); the host adds the chunks' partials in ascending order.  No float atomics:
 *      a call gives the same bits every time.  MET2_E_INVALID when S is empty (no finite voxel, hi = lo, no voxel at all).
 *  2 mesh (met2_bet_mesh, built on the host): the icosahedron, phi = (1 + sqrt 5) / 2, every vertex divided by sqrt((x^2 + y^2) + z^2):
 *      vertices (-1,phi,0) (1,phi,0) (-1,-phi,0) (1,-phi,0) (0,-1,phi) (0,1,phi) (0,-1,-phi) (0,1,-phi) (phi,0,-1) (phi,0,1) (-phi,0,-1) (-phi,0,1);
 *      faces, counter-clockwise seen from outside: 0 11 5, 0 5 1, 0 1 7, 0 7 10, 0 10 11, 1 5 9, 5 11 4, 11 10 2, 10 7 6, 7 1 8, 3 9 4, 3 4 2,
 *      3 2 6, 3 6 8, 3 8 9, 4 9 5, 2 4 11, 6 2 10, 8 6 7, 9 8 1;  subdivided `level` times: every triangle (a, b, c), in
 *      order, becomes (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca); a midpoint is ((p + q) 0.5) / |.| and gets the next free index the
 *      first time its edge is met (edges ab, bc, ca in that order).  10 4^level + 2 vertices, 20 4^level triangles: 2562 and 5120 at level 4,
 *      bet's mesh.  ring[i][0 .. deg_i) = the neighbours of vertex i counter-clockwise seen from outside, starting at the one of the smallest
 *      index; deg is 5 at the twelve original vertices and 6 elsewhere.  Start: vertex = COG + unit vertex x (r / 2).
 *  3 surface evolution (met2_bet_evolve), n_iter Jacobi steps: every vertex x is computed from the previous step's positions.  With D_k =
 *      ring_k - x, k in ring order, sums started at 0 and added in that order:
 *      N = sum_k D_k x D_{k+1} (cyclic; (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x)), n = N / sqrt((N_x^2 + N_y^2) + N_z^2), 0 if N = 0;
 *      s = (sum_k ring_k) / deg - x;  sd = (s_x n_x + s_y n_y) + s_z n_z;  sn = sd n;  st = s - sn;
 *      u1 = 0.5 st;  u2 = f2 sn, f2 = (1 + tanh(F (2 |sd| / (l l) - E))) 0.5   [1 / rho = 2 |sn| / l^2],
 *      E = (1 / rmin + 1 / rmax) / 2, F = 6 / (1 / rmin - 1 / rmax), rmin = 3.33 mm, rmax = 10 mm;
 *      I(d) = v at voxel i_a = floor((x_a - d n_a) g_a + 0.5), g_a = 1 / d_a rounded to fp64, d = 1, 2, .. mm; 0 outside the volume and where v
 *      is not finite;  Imin = max(t2, min(tm, min_{d = 1..20} I(d)));  Imax = min(tm, max(t, max_{d = 1..10} I(d)));
 *      tl = (Imax - t2) b + t2, b = pow(f, 0.275);  f3 = 2 (Imin - tl) / (Imax - t2), 0 where Imax - t2 is not positive;
 *      u3 = ((0.05 f3) l) n;  x' = ((x + u1) + u2) + u3.
 *      l = the mean vertex-to-neighbour distance of the mesh, (sum_i sum_k |D_k|) / (sum_i deg_i), taken from the positions at the start of
 *      iterations 0, 50, 100, ..: per vertex the ring in order, per thread h of 1024 its vertices h, 1024 + h, 2048 + h in order, the
 *      butterfly over a wave, the 16 waves in ascending order.  tanh is the device library's (about an ulp).
 *      ONE workgroup of 1024 threads runs all n_iter steps in one launch: both position buffers and the rings in LDS (60 nv bytes: 153 720
 *      of the CU's 163 840 at level 4), one barrier per step.  level > 4 does not fit: MET2_E_UNSUPPORTED.  The volume needs one voxel at least.
 *  4 fill (met2_bet_fill): voxel (ix, iy, iz) is inside when the ray from its centre along +z crosses the surface an odd number of times.
 *      Per triangle, with (px, py) = (ix dx, iy dy): an edge (p, q) -- p the end of the SMALLER vertex index, so that both triangles of an
 *      edge compute the same bits -- meets the line y = py when (p_y <= py) != (q_y <= py) (half-open: an end on the line belongs to the
 *      side below), at x_e = p_x + ((py - p_y) (q_x - p_x)) / (q_y - p_y), z_e likewise.  None or two of a triangle's edges do; the ray crosses
 *      the triangle when exactly one of the two has x_e > px (half-open again).  With (xl, zl) the one with x_e <= px and (xr, zr) the other:
 *      zc = zl + ((px - xl) (zr - zl)) / (xr - xl), m = ceil(zc / dz): the crossing lies above the voxels iz < m (a voxel whose centre is on
 *      the surface counts as above it).  A voxel is inside when an odd number of crossings has m > iz.  Every edge is decided once for
 *      both of its triangles, so on a closed mesh every column has an even number of crossings and a ray through an edge or a vertex is
 *      counted once.  One thread per column, integers only.  A triangle with an index outside [0, n_vertices) is skipped; a crossing whose
 *      zc is NaN (non-finite vertices) is dropped.
 * DEVICE pointers: v, data, mask_out [nx][ny][nz] uint8 (1 inside), vertices [nv][3] (x, y, z in mm), triangles [nt][3] int32.
 * HOST: voxel_mm, stats and stats_out [8] = (t2, t, t98, tm, COG_x, COG_y, COG_z, r), count_out (may be NULL), met2_bet_mesh's outputs (each may be NULL):
 * unit_vertices [nv][3], triangles [nt][3], ring [nv][6] (-1 beyond deg), deg [nv].
 * met2_brain_mask runs 1-4 through the host code of the stage entries (which exist for tests and diagnostics); vertices_out (device,
 * [nv][3], the final surface) and stats_out (host, 8 doubles) may be NULL.  met2_bet_evolve takes the statistics and the start vertices
 * from the caller (vertices_out may be vertices_in), met2_bet_fill any mesh.  All but met2_bet_mean and met2_bet_fill BLOCK: the host reads
 * the statistics back between the stages, and the evolution waits for its kernel.  Additive: MET2_ABI_VERSION stays 6.
 * Limits: 0 < f < 1, n_iter >= 0, positive finite voxel sizes, level >= 0 (MET2_E_INVALID); level <= 4, fewer than 2^31 voxels
 * (MET2_E_UNSUPPORTED). */
int met2_brain_mask(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const double voxel_mm[3], double f, int32_t level,
                    int32_t n_iter, uint8_t *mask_out, double *vertices_out, double *stats_out, void *stream);
int met2_bet_mean(int32_t device, int64_t nvox, int32_t n_te, const double *data, double *out, void *stream);
int met2_bet_stats(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const double voxel_mm[3], double *stats_out,
                   int64_t *count_out, void *stream);
int met2_bet_mesh(int32_t level, double *unit_vertices, int32_t *triangles, int32_t *ring, int32_t *deg);
int met2_bet_evolve(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const double voxel_mm[3], const double stats[8], double f,
                    int32_t level, int32_t n_iter, const double *vertices_in, double *vertices_out, void *stream);
int met2_bet_fill(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double voxel_mm[3], int32_t n_vertices, const double *vertices,
                  int32_t n_triangles, const int32_t *triangles, uint8_t *mask_out, void *stream);

/* motor:293-304, TV denoising (denoise='TV'; the reference's example pipeline runs it, example_script_run_MET2_preproc_and_recon.sh:54):
 *     for every echo volume:  sigma_est = mean(estimate_sigma(vol));  vol <- denoise_tv_chambolle(vol, weight = 2 sigma_est, eps = 2e-4,
 *                                                                                                 max_num_iter = 200)
 * (scikit-image's functions, restated from the published algorithms: Donoho-Johnstone's db2 median estimator and Chambolle's
 * projection algorithm in 3-D).  ALL n_te echo volumes go through every step in the same launches; the stopping rule is applied
 * on the device per echo, the host reads nothing per iteration.
 * DEVICE pointers: data and out, both [nx][ny][nz][n_te] (echo_major = 0, the C-ordered array of the driver) or both [n_te][nz][ny][nx]
 * (echo_major = 1: the memory order of the Fortran-ordered array nibabel hands the driver, motor:167-173); out may alias data.
 * HOST: weight [n_te] = the `weight` of denoise_tv_chambolle per echo, or NULL: weight = weight_factor x the echo's estimated sigma
 * (the reference: weight_factor = 2).  An echo whose weight is not a positive finite number is copied through (an all-zero volume
 * has sigma = 0; scikit-image would return nan for it).
 * eps, max_num_iter: the reference passes 2e-4 and 200.  poll_every: 0 = every iteration of max_num_iter is enqueued and the call
 * returns without waiting (launches for echoes that have converged return at once); k > 0 = the host looks at the device's flags
 * every k iterations -- one batch of k behind the stream, so that the stream never waits for the host -- and stops enqueueing when
 * every echo has converged (the call then blocks until about that point; up to 2k launches that return at once are enqueued past it).
 * DEVICE out, may be NULL: sigma [n_te] the estimated noise level per echo (nan if the echo holds a nan or inf -- the reference's
 * finite check would raise), iters [n_te] int32 Chambolle iterations executed per echo.
 * work: DEVICE scratch of met2_tv_work_bytes() bytes (7 working copies of the volume), or NULL: allocated and freed inside, which
 * makes the call blocking.  n_te <= 127 for echo_major = 0. */
int64_t met2_tv_work_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t n_te, int32_t echo_major);
int met2_tv_chambolle(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const double *data, int32_t echo_major,
                      const double *weight, double weight_factor, double eps, int32_t max_num_iter, int32_t poll_every, double *out,
                      double *sigma, int32_t *iters, void *work, int64_t work_bytes, void *stream);
/* For reports: HIP-event time (ms) from the first to the last Chambolle launch of the calling thread's most recent
 * met2_tv_chambolle (blocks until they finished) and the number of iterations that were enqueued. */
int met2_tv_last_timing(double *iter_ms, int32_t *launches);
/* The noise estimate's kernels one by one, and the tile geometry of the iteration, for tests and diagnostics (additive; ABI stays 6).
 * met2_tv_chambolle launches tv_gather_kernel, tv_detail_kernel and tv_sigma_kernel through the same host helpers as these entries.
 *
 * Host only: how met2_tv_chambolle lays a shape out.  (n0, n1, n2) is one echo volume in memory order, slowest axis first: (nx, ny, nz)
 * for echo_major = 0, (nz, ny, nx) for echo_major = 1.  A workgroup of tv_iter_kernel has `oy` rows of 64 lanes and owns step1 rows
 * along n1 (oy when n1 <= oy, else oy - 1: the last row is a halo) and step2 lanes along n2; it marches over xlen planes along n0.
 * nt1, nt2, nseg = tiles along n1 and n2, segments along n0; ntiles = nt1 nt2 nseg per echo.  c0, c1, c2 = (n + 3) / 2 per memory axis:
 * the shape of the 'ddd' sub-band; nc = c0 c1 c2.  sigma_cap: tv_sigma_kernel counts on the whole array while more than this many keys
 * share the prefix found so far, and decides the remaining bits on a list in LDS after that.
 * met2_tv_work_bytes = the sum, each term rounded up to a multiple of 256, of: 8 vol n_te (echo-major copy), 2 x 24 vol n_te (the two
 * buffers of p), 8 nc n_te (coefficients), 16 ntiles n_te (energy partials), 56 n_te (per-echo state), 8 n_te (weights); vol = n0 n1 n2. */
typedef struct met2_tv_geometry {
    int32_t oy, step1, step2, xlen, nt1, nt2, nseg, ntiles, c0, c1, c2, sigma_cap;
    int64_t nc;
} met2_tv_geometry;
int met2_tv_launch_info(int32_t nx, int32_t ny, int32_t nz, int32_t n_te, int32_t echo_major, met2_tv_geometry *geom);
/* The finest all-detail ('ddd') db2 coefficients of every echo volume: the gather (echo_major = 0 only) and tv_detail_kernel.
 * DEVICE pointers: data as for met2_tv_chambolle (n_te <= 127 for echo_major = 0); coef [n_te][c0][c1][c2] in the volume's MEMORY axis
 * order: [n_te][(nx+3)/2][(ny+3)/2][(nz+3)/2] for echo_major = 0, [n_te][(nz+3)/2][(ny+3)/2][(nx+3)/2] for echo_major = 1.  The separable
 * passes run x first, then y, then z in either layout, products and sums rounded separately and added in tap order, so both layouts
 * give the same bits for the same volume.  Input domain: any float64, axis lengths >= 1 (inf and nan propagate as in IEEE arithmetic).
 * Allocates its echo-major copy inside and blocks until the coefficients are written. */
int met2_tv_detail(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t n_te, const double *data, int32_t echo_major, double *coef,
                   void *stream);
/* tv_sigma_kernel on coefficients the caller supplies.  DEVICE: coef [n_te][nc], nc >= 1; out, each may be NULL: sigma [n_te] =
 * median(|d|) / 0.6744897501960817 over the echo's non-zero d (-0.0 counts as zero), bit-equal to np.median -- the mean (a + b) / 2 of the
 * two middle values for an even count; 0 when every d is zero; nan when any d is inf or nan.  weight_out [n_te] = weight[t] if given, else
 * weight_factor x sigma; copy [n_te] int32 = 1 where that weight is not a positive finite number (met2_tv_chambolle copies such an echo
 * through).  HOST: weight [n_te] or NULL.  Input domain: any float64, denormals included.  Blocking. */
int met2_tv_sigma(int32_t device, int32_t n_te, int64_t nc, const double *coef, const double *weight, double weight_factor, double *sigma,
                  double *weight_out, int32_t *copy, void *stream);

/* motor/motor_recon_met2_real_data_ROI.py:405-420, the reduction of the ROI mode: for every ROI the mean signal over its
 * voxels and the mean EPG kernel, each voxel contributing the dictionary slice of its own flip angle
 * (total_signal / nv, total_Kernel / nv).  `src` holds the dictionary the flip angles index; `dst` is a plan of the same
 * n_te x n_t2 with n_fa = number of ROIs: its dictionary (and Gram matrices) become the per-ROI mean kernels, so that
 * met2_fit(dst, MET2_X2, nroi, mean_signal, fa_index = 0..nroi-1, ...) is the per-ROI fit of :419.
 * DEVICE pointers: data (echo e of voxel v at data[v * voxel_stride + e * echo_stride]), roi_index [nvox] int32 ROI
 * ordinal 0..nroi-1 (negative: voxel belongs to no ROI), fa_index [nvox] float64 (NULL = 0), out mean_signal
 * [nroi][n_te], out count [nroi] float64 voxels per ROI (0 -> that ROI's outputs are nan, as in the reference).
 * Deterministic (fixed summation order).  Blocking. */
int met2_roi_reduce(met2_plan *src, met2_plan *dst, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                    const int32_t *roi_index, const double *fa_index, double *mean_signal, double *count, void *stream);

/* motor:443-472 alone (fsol already on the device). */
int met2_metrics(met2_plan *plan, int64_t nvox, const double *fsol, const uint8_t *mask, double *maps,
                 void *stream);

/* Duration in ms of the solver kernel of the most recent met2_fit / met2_fa_bruteforce on
 * this plan, measured with HIP events on the launch stream (blocks until it finished). */
int met2_plan_last_kernel_ms(met2_plan *plan, double *ms);
/* NNLS/T2SPARC/X2/L-curve/GCV fits (and BayesReg at n_t2 > 64) give every wave an LDS region for a Cholesky factor of a reduced
 * passive-set capacity (the largest that lets 16 waves share a CU's LDS, never below 0.6 n_t2: 50 at n_t2 = 60; at two bins per
 * lane the largest that lets the 8 waves those kernels are compiled for share it: 71 at n_t2 = 120).  Such a fit runs two solver
 * kernels: the fit kernel queues a voxel whose set outgrows the capacity (~1 % at 32 x 60, 5-10 % at 48 x 120), and the spill-over
 * kernel launched behind it, with the same geometry, solves the queued voxels with the factor's columns beyond the capacity in a
 * per-wave slot in device memory (allocated by the first such fit on the plan: 18 MB at n_t2 = 60, 77 MB at 120).  A plan whose
 * options name non-default lambda-search intervals runs every voxel through the spill-over kernel.
 * met2_plan_last_spill_count: how many voxels of the most recent finished fit were queued (for reports and tests); under non-default
 * lambda-search intervals every fitted voxel goes through the spill-over kernel, and the count is theirs.
 * met2_plan_last_second_pass_ms: the spill-over kernel's duration in the most recent fit (0 if the fit ran none);
 * met2_plan_last_kernel_ms is then the fit kernel's alone, about 0 under non-default lambda-search intervals. */
int met2_plan_last_spill_count(met2_plan *plan, int64_t *count);
int met2_plan_last_second_pass_ms(met2_plan *plan, double *ms);

/* For tests: the number of warm re-factorisations that took the packed four-rows-per-step leg (one bin per lane, 4 <= k <= 32) in the fits
 * on the plan's device that ran with MET2_REFAC_COUNT set in the environment, since the last reset.  Waits for the device. */
int met2_refac_packed_calls(met2_plan *plan, uint64_t *calls, int32_t reset);

/* Launch geometry of the solver kernel (for reports): workgroups, threads per workgroup,
 * dynamic LDS bytes per workgroup. */
int met2_plan_launch_info(met2_plan *plan, int32_t method, int32_t *grid, int32_t *block, int32_t *lds_bytes);

/* Which form of the GCV trace (algorithms.py:285-296) met2_fit takes on this plan (for reports and tests): low_rank = 1 when every
 * flip angle's dictionary is of numerical rank <= 16 -- an orthonormal basis of 16 vectors leaves less than 1e-9 of its largest
 * column, `residual` = the largest such remainder over the flip angles -- and the trace is taken from the 17 x 17 matrix in that
 * basis (true for EPG dictionaries: ~1e-10 at 48 x 120, ~1e-12 at 32 x 60); 0: from the (n_te + 1) x (n_te + 1) matrix. */
int met2_plan_gcv_form(met2_plan *plan, int32_t *low_rank, double *residual);

/* Resampling through a displacement field, and the device stages of a greedy deformable (non-linear) registration with the squared local
 * normalised cross-correlation, LNCC (an extension; additive, ABI stays 6).  The loop around the stages is warp.py's: warp, force, fluid
 * smoothing of the force (met2_smooth_separable), its largest norm, composition, elastic smoothing of the field.  The metric is that of ANTs'
 * CC and of `greedy -m NCC` (Avants et al., Med. Image Anal. 12:26-41, 2008), and the force is their CENTRE-VOXEL approximation of its
 * gradient, not the sum over all windows that hold a voxel.  Parity with ANTs, greedy or fnirt is unpinned: none was available.  No plan:
 * `device` and `stream` only.  All arithmetic is fp64, no product is fused into a sum, every operation rounds once in the order written;
 * there are no floating-point atomics.  DEVICE pointers except the dims, A and gain.
 * Field.  disp [mx][my][mz][3] lives on the destination (fixed) grid, in voxels of that grid: the layout of echo data, so
 *   met2_smooth_separable smooths a field with n_te = 3.
 * met2_warp.  met2_resample with a field, orders 0 and 1: destination voxel x = (i, j, k) samples the source at c = A (x + u(x)):
 *     p_a = x_a + u_a (one rounding per axis);  c_a = ((A[a][3] + A[a][0] p_x) + A[a][1] p_y) + A[a][2] p_z;
 *   then the inside test, the taps, the weights and the tap sum of met2_resample.  A zero field reproduces met2_resample to the bit.  Strides,
 *   series, cval and inside as there.  Asynchronous.  disp == NULL is refused (met2_resample is that call).
 * met2_warp_labels.  int32 labels, order 0, `fill` where outside.  Asynchronous.
 * met2_warp_compose.  The one kernel for composition and for a change of grid.  u_src [nx][ny][nz][3] on its own grid, the destination grid
 *   [mx][my][mz], A[12] (destination voxel -> u_src's voxel), gain[3], v [mx][my][mz][3] or NULL, step, vmax2 (one double on the device) or NULL:
 *     s = step / sqrt(*vmax2), 0 where *vmax2 is not > 0, `step` itself where vmax2 is NULL;   w_a = s v_a(x) (0 where v is NULL);
 *     p_a = x_a + w_a;  c_a as above, then clamped into 0 .. n_a - 1 (a coordinate that is not a number: 0) -- there is never an outside;
 *     out_a(x) = w_a + gain_a t_a,  t_a = the order-1 tap sum of channel a of u_src at c.
 *   Composition phi <- phi o (id + w) is A = identity, gain = 1 on one grid; carrying a field to another pyramid level is v = NULL with A
 *   the level-to-level voxel matrix and gain the ratio of the voxel sizes.  The scale is read on the device: an iteration needs no host
 *   synchronisation.  out must not alias u_src or v.  Asynchronous.
 * met2_warp_max_norm2.  *vmax2 = max over the n_voxels voxels of (v_x v_x + v_y v_y) + v_z v_z (0 for a zero field; a norm that is not a
 *   number is passed over): per block, then one integer atomic max on the bit pattern, which orders as the non-negative values do.  Asynchronous.
 * met2_warp_lncc.  The metric force from fixed F, warped W and inside m (uint8), all [nx][ny][nz], a radius r in 1 .. MET2_WARP_MAX_RADIUS
 *   and eps >= 0:
 *     channels  c0 = m (1 or 0), c1 = F where m else 0, c2 = W where m else 0, c3 = c1 c1, c4 = c2 c2, c5 = c1 c2;
 *     box sums  over the (2 r + 1)^3 window clipped to the volume, separable, along x, then y, then z; every output is the direct sum of its
 *               <= 2 r + 1 terms in ascending order (no running sum): n, sF, sW, sFF, sWW, sFW;
 *     A = sFW - (sF sW) / n,  B = sFF - (sF sF) / n,  C = sWW - (sW sW) / n;
 *     a voxel is VALID when m and n >= 2 and B > eps and C > eps;   cc = (A A) / (B C);
 *     f = ((2 A) / (B C)) ((F - sF / n) - (A / C) (W - sW / n));
 *     g_a = (W(x+) - W(x-)) / 2, x+ and x- the face neighbours along a where they are in the grid AND inside, the centre voxel otherwise
 *       (a moving image with a background that is not zero would otherwise show a false edge at the rim of its field of view);
 *     force_a = f g_a at a valid voxel, 0 elsewhere;   metric[0] = the sum of cc over the valid voxels, metric[1] = their number.
 *   force [nx][ny][nz][3]; metric [2] at a device address of the caller's choice (a level's trace is read back once).  The sums of metric are
 *   taken per thread in ascending voxel order, per block by a tree, over the blocks in a fixed order: the same bits from call to call.
 *   Stage entries: met2_warp_lncc_sums (sums [6][nx][ny][nz], in the order above), met2_warp_lncc_force (from given sums).
 *   Work space: `work` of at least work_bytes = met2_warp_work_bytes (host only; enough for every one of the three entries) on the device,
 *   and the call is asynchronous; or NULL, and the entry allocates its own block and waits for the stream.
 * Limits.  Every axis 1 .. MET2_RESAMPLE_MAX_AXIS, series as met2_resample (MET2_E_UNSUPPORTED beyond).  MET2_E_INVALID: an axis < 1, an
 * order other than 0 or 1, bad strides (met2_resample's rule), a NULL required pointer, aliased outputs, an entry of A, gain or step that is
 * not finite, a radius outside 1 .. 4, eps < 0 or not finite, a work block that is too small.  Every check comes before any device work:
 * the outputs are then untouched. */
#define MET2_WARP_MAX_RADIUS 4
int met2_warp(int32_t device, int32_t order, const int32_t src_dims[3], int32_t n_series, const double *src, int64_t src_voxel_stride,
              int64_t src_series_stride, const int32_t dst_dims[3], const double A[12], const double *disp, double cval, double *dst,
              int64_t dst_voxel_stride, int64_t dst_series_stride, uint8_t *inside, void *stream);
int met2_warp_labels(int32_t device, const int32_t src_dims[3], const int32_t *labels, const int32_t dst_dims[3], const double A[12],
                     const double *disp, int32_t fill, int32_t *out, uint8_t *inside, void *stream);
int met2_warp_compose(int32_t device, const int32_t src_dims[3], const double *u_src, const int32_t dst_dims[3], const double A[12],
                      const double gain[3], const double *v, double step, const double *vmax2, double *out, void *stream);
int met2_warp_max_norm2(int32_t device, int64_t n_voxels, const double *v, double *vmax2, void *stream);
int met2_warp_work_bytes(const int32_t dims[3], int64_t *bytes);
int met2_warp_lncc_sums(int32_t device, const int32_t dims[3], const double *fixed, const double *warped, const uint8_t *inside, int32_t radius,
                        double *sums, void *work, int64_t work_bytes, void *stream);
int met2_warp_lncc_force(int32_t device, const int32_t dims[3], const double *fixed, const double *warped, const uint8_t *inside,
                         const double *sums, double eps, double *force, double *metric, void *work, int64_t work_bytes, void *stream);
int met2_warp_lncc(int32_t device, const int32_t dims[3], const double *fixed, const double *warped, const uint8_t *inside, int32_t radius,
                   double eps, double *force, double *metric, void *work, int64_t work_bytes, void *stream);

/* The inverse of a displacement field by fixed-point iteration, and the Jacobian determinant of a field (an extension; additive, ABI stays
 * 6).  With T(x) = A (x + u(x)) of met2_warp (u on the fixed grid, A: fixed voxel -> moving voxel, L its 3 x 3 part) the inverse is wanted
 * in the same form, so that met2_warp and met2_warp_labels apply it unchanged: v on the MOVING grid in its voxels, B = A^-1, moving voxel y
 * samples the fixed grid at B (y + v(y)).  That gives v(y) = -L u(B (y + v(y))), a fixed-point equation (Chen et al., Med. Phys. 35:81-88,
 * 2008) iterated as v_0 = 0, v_{k+1}(y) = -L u_tri(clamp(B (y + v_k(y)))).  It contracts where the Lipschitz constant of L u B is below 1
 * and nowhere else: the step returns the largest change, and met2_warp_jacobian counts the voxels at which u folds, for the user to judge.
 * The loop is warp.py's (a fixed number of steps, no host synchronisation inside).  Parity with ANTs, greedy or invwarp is unpinned: none
 * was available.  No plan, no work space: `device` and `stream` only.  All arithmetic is fp64, no product is fused into a sum, every
 * operation rounds once in the order written; there are no floating-point atomics.  DEVICE pointers except the dims, B, N and scale.
 * met2_warp_invert_step.  One step, general enough to be held against met2_warp_compose: u_src [nx][ny][nz][3] on its own grid, the
 *   destination grid [mx][my][mz], B[12] (destination voxel -> u_src's voxel), N[9] (row-major 3 x 3), v_in [mx][my][mz][3] or NULL,
 *   v_out [mx][my][mz][3], inside [mx][my][mz] uint8 or NULL, res2 (one double on the device) or NULL.  Per destination voxel y:
 *     p_a = y_a + v_in_a(y) (one rounding per axis; y_a where v_in is NULL, the bits v_in = 0 gives);
 *     c_a = ((B[a][3] + B[a][0] p_x) + B[a][1] p_y) + B[a][2] p_z                                   -- met2_warp's coordinates;
 *     inside(y) = met2_resample's inside test on c: 0 <= c_a <= n_a - 1 on every axis;
 *     c_a is then clamped into 0 .. n_a - 1 as met2_warp_compose clamps it (a coordinate that is not a number: 0);
 *     t_a = the order-1 tap sum of channel a of u_src at c (met2_resample's taps, weights and order of summation);
 *     v_out_a(y) = (N[a][0] t_x + N[a][1] t_y) + N[a][2] t_z;
 *     d_a = v_out_a - v_in_a (v_out_a - 0 where v_in is NULL);   *res2 = max over y of (d_x d_x + d_y d_y) + d_z d_z
 *   (0 where every voxel's is 0; a value that is not a number is passed over): per thread, per block by a tree, then one integer atomic max
 *   per block on the bit pattern, which orders as the non-negative values do (a block whose maximum does not exceed what *res2 holds by
 *   then leaves it out: the value only grows during the call).  The entry zeroes *res2 on the stream first.
 *   An inverse step is N = -L, B = A^-1, both formed by the caller on the host.  v_out must not alias u_src or v_in.  Asynchronous.
 * met2_warp_jacobian.  u [nx][ny][nz][3], scale, det [nx][ny][nz], n_nonpositive (one int64 on the device) or NULL:
 *     J_ab = delta_ab + D_b u_a;   D_b f = (f(x + e_b) - f(x - e_b)) / 2 where both neighbours are in the grid, f(x + e_b) - f(x) at the lower
 *     rim, f(x) - f(x - e_b) at the upper rim (an axis of length 2 has rims only), 0 on an axis of length 1;   J_aa = 1 + D_a u_a;
 *     m_0 = J_11 J_22 - J_12 J_21,  m_1 = J_10 J_22 - J_12 J_20,  m_2 = J_10 J_21 - J_11 J_20    (two products, then their difference);
 *     det(x) = scale ((J_00 m_0 - J_01 m_1) + J_02 m_2)                                          -- the expansion along the first row;
 *     *n_nonpositive = the number of voxels whose det is not > 0 (one that is not a number counts): per thread, per block by a tree of
 *     integers, then one integer atomic add per block.  The entry zeroes it on the stream first.
 *   With scale = 1 this is the local volume change of x -> x + u(x) in voxels; scale = det L makes it that of T.  det must not alias u.
 *   Asynchronous.
 * Limits.  Every axis 1 .. MET2_RESAMPLE_MAX_AXIS (MET2_E_UNSUPPORTED beyond).  MET2_E_INVALID: an axis < 1, a NULL required pointer,
 * aliased outputs, an entry of B or N, or a scale, that is not finite.  Every check comes before any device work: the outputs are then
 * untouched. */
int met2_warp_invert_step(int32_t device, const int32_t src_dims[3], const double *u_src, const int32_t dst_dims[3], const double B[12],
                          const double N[9], const double *v_in, double *v_out, uint8_t *inside, double *res2, void *stream);
int met2_warp_jacobian(int32_t device, const int32_t dims[3], const double *u, double scale, double *det, int64_t *n_nonpositive, void *stream);

/* Voxel-wise group statistics by permutation (an extension; additive, ABI stays 6).  One form covers one-sample sign flipping, the
 * permutation of group labels and the Freedman-Lane scheme with nuisance regressors (Winkler et al., NeuroImage 92:381-397, 2014): the
 * caller residualises the data against the nuisance once (Y, with s0 the residual sum of squares per voxel) and turns every candidate
 * permutation into r + 1 weight rows over the n subjects (group.py: partition, weights, residualise); the statistic is then
 * met2_group_perm_stats.  Y [n][n_vox] (series-major: one row per subject), s0 [n_vox], W [K][r + 1][n], two_sided 0 | 1, t_ref [n_vox] or
 *   NULL, t_first [n_vox] or NULL, kmax [K], count [n_vox] uint32 (required with t_ref).  For voxel v and candidate k:
 *     b   = sum_i W[k][0][i] Y[i][v]
 *     g_j = sum_i W[k][j][i] Y[i][v]                 j = 1 .. r
 *     q   = sum_j g_j g_j;   rss = s0[v] - q
 *     t   = rss > 0 ? b / sqrt(rss) : 0              (two_sided: t = |t|)
 *   Order.  All arithmetic is fp64; no product is fused into a sum; every operation rounds once.  A sum over i starts from 0.0 and takes
 *   its terms one by one, i = 0, 1, .. n - 1: a <- a + W[k][j][i] Y[i][v].  q = g_1 g_1, then q <- q + g_j g_j for j = 2 .. r.  The
 *   quotient and the square root are correctly rounded.  So the bits of t(k, v) depend on W[k], Y[:, v] and s0[v] alone -- not on K, not
 *   on where the candidate stands in W, not on n_vox or the voxel's place, not on the device -- and numpy reproduces them in float64 with
 *   the same loop (tests/tools/group_numpy.py).  That is what makes t >= t_obs exact for the identity permutation.
 *   Outputs.  kmax[k] = max over v of t(k, v), as a double; the entry sets it itself (per wave by comparisons, per block through LDS,
 *     then one integer atomic max per block and candidate on a key that orders as the doubles do, turned back into the double by a last
 *     launch; +0 orders above -0; a t that is not a number is passed over; -infinity when n_vox = 0 or every t is not a number).  No
 *     floating-point atomics, no scratch.
 *     count[v] += the number of candidates k with t(k, v) >= t_ref[v]: accumulated over launches, so the caller zeroes it once; the voxel's
 *     count is owned by one thread.  Skipped when t_ref is NULL.
 *     t_first[v] = t(0, v) when t_first is not NULL.
 *   DEVICE pointers throughout.  Asynchronous on `stream`.
 * met2_group_limits (host only; any output may be NULL): MET2_GROUP_MAX_N, MET2_GROUP_MAX_R, MET2_GROUP_MAX_K and MET2_GROUP_VOXEL_TILE, the
 *   number of consecutive voxels a block owns (what a test stands on the edges of).
 * Limits.  r < n <= MET2_GROUP_MAX_N, 1 <= r <= MET2_GROUP_MAX_R, 1 <= K <= MET2_GROUP_MAX_K per launch (MET2_E_UNSUPPORTED beyond the upper
 * ends).  MET2_E_INVALID: r or K < 1, n <= r, n_vox < 0, two_sided outside {0, 1}, W or kmax NULL, Y or s0 NULL with n_vox > 0, t_ref
 * without count.  n_vox = 0 is valid (Y and s0 are then not read and may be NULL).  Every check comes before any device work: the outputs
 * are then untouched. */
#define MET2_GROUP_MAX_N 128
#define MET2_GROUP_MAX_R 8
#define MET2_GROUP_MAX_K 256
#define MET2_GROUP_VOXEL_TILE 256
int met2_group_limits(int32_t *max_n, int32_t *max_r, int32_t *max_k, int32_t *voxel_tile);
int met2_group_perm_stats(int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t K, const double *W,
                          int32_t two_sided, const double *t_ref, double *t_first, double *kmax, uint32_t *count, void *stream);

/* F-contrasts: the same test for a contrast matrix C [p][s] of rank s, 1 <= s <= r (an extension; additive, ABI stays 6).  The caller
 * partitions the design into the effect X1 [n][s] and the nuisance Z with X1' Z = 0, residualises against Z (Y, s0 as above) and turns every
 * candidate into r weight rows W[k][j] = P_k' q_j, q_1 .. q_r the orthonormal basis from the QR factorisation of [X1 Z], so that q_1 .. q_s
 * span X1 (group.py: partition, weights_f).  There is no row 0: W [K][r][n].  scale = (n - r) / s.  For voxel v and candidate k:
 *     g_j = sum_i W[k][j][i] Y[i][v]                 j = 1 .. r
 *     qs  = g_1 g_1 + .. + g_s g_s;   q = qs + g_{s+1} g_{s+1} + .. + g_r g_r;   rss = s0[v] - q
 *     F   = rss > 0 ? (scale qs) / rss : 0
 *   the Freedman-Lane F of the full model against the nuisance: H_z y lies in the column space of Z, X1 is orthogonal to Z and a signed
 *   permutation keeps the norm, so the extra sum of squares is |Q1' P_k Y|^2 = qs and the residual one s0 - q.  For s = 1, F = t^2 up to
 *   rounding.
 *   Order.  All arithmetic is fp64; no product is fused into a sum; every operation rounds once.  Each g_j is a sum from 0.0 over
 *   i = 0, 1, .. n - 1: a <- a + W[k][j][i] Y[i][v].  q = g_1 g_1, then q <- q + g_j g_j for j = 2 .. r in ascending order; qs is the value q
 *   holds after the term j = s -- a prefix of the same sum, no addition of its own.  rss = s0 - q; num = scale qs; F = num / rss, correctly
 *   rounded.  So the bits of F(k, v) depend on W[k], Y[:, v], s0[v], s and scale alone, and numpy reproduces them in float64 with the same loop
 *   (tests/tools/group_f_numpy.py).  rss <= 0 gives F = 0; an rss that is not a number (a NaN in Y or s0) gives an F that is not a number, which
 *   the maximum passes over and which reaches no reference.
 * met2_group_perm_fstats: Y, s0, K, stream as for met2_group_perm_stats; s and scale are the same for every candidate of the launch; f_ref,
 *   f_first, kmax and count have the meaning of t_ref, t_first, kmax and count there, for F (kmax by the same integer atomic max on the same
 *   key, -infinity when n_vox = 0 or every F is not a number; count[v] += #{k: F(k, v) >= f_ref[v]}, one owner per voxel; no floating-point
 *   atomics, no scratch).  There is no two_sided: F does not see the sign (all weights negated give the same bits).
 * met2_group_perm_ftfce: met2_group_perm_tfce with F(k, v) in the place of t(k, v): computed by met2_group_perm_fstats's own kernel code -- the
 *   same bits -- scattered to the dense maps, then the same transform, gather, work space (met2_tfce_work_bytes with n_vox > 0) and late errors.
 *   TFCE is taken on F itself, with the same E, H and dh; the extent's threshold is one on F.
 * Limits.  1 <= s <= r <= MET2_GROUP_MAX_R, r < n <= MET2_GROUP_MAX_N, 1 <= K <= MET2_GROUP_MAX_K (MET2_TFCE_MAX_K for met2_group_perm_ftfce);
 * MET2_E_UNSUPPORTED beyond the upper ends.  MET2_E_INVALID: s < 1 or s > r, scale not finite or <= 0, and every case of the t entries (no
 * two_sided).  n_vox = 0 is valid for met2_group_perm_fstats.  Every check comes before any device work: the outputs are then untouched. */
int met2_group_perm_fstats(int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t s, double scale,
                           int32_t K, const double *W, const double *f_ref, double *f_first, double *kmax, uint32_t *count, void *stream);

/* Threshold-free cluster enhancement (Smith & Nichols, NeuroImage 44:83-98, 2009) and cluster extent of statistic maps, and both as the
 * statistic of the permutation test above (an extension; additive, ABI stays 6).  Written from the paper and from the statement below.
 * A map t lies on a grid dims = {nx, ny, nz}, the voxel (x, y, z) at (x ny + y) nz + z, with a mask (uint8, non-zero = inside; NULL: all).
 *   Level.    h_j = (double)j * dh (one rounding).  level(v) = the largest j in 1 .. MET2_TFCE_MAX_STEPS with h_j <= t(v), found by comparisons
 *             (a bisection over j; no division); 0 if there is none, if v lies outside the mask or if t(v) is not a number.  A map that rises
 *             above MET2_TFCE_MAX_STEPS dh is treated as if it stopped there (+infinity too).
 *   Support.  S_j = {v: level(v) >= j};  e_j(v) = the number of voxels of the connected component of S_j that holds v, under connectivity
 *             6 (faces), 18 (faces and edges) or 26 (faces, edges and corners).  Neighbours are found on (x, y, z): the grid does not wrap,
 *             and a voxel outside the mask joins nothing.
 *   MET2_TFCE_MODE_TFCE:    out(v) = dh * sum_j e_j(v)^E h_j^H, the sum from 0.0 over j = level(v), level(v) - 1, .. 1 in that order, every
 *             product and sum rounded once, nothing fused.  For E = 0.5 and H = 2 exactly, a term is sqrt((double)e) * (h * h), with a
 *             correctly rounded square root: numpy reproduces the bits in float64 (tests/tools/tfce_numpy.py).  Any other (E, H): a term is
 *             pow((double)e, E) * pow(h, H), held to an accuracy bound only.  out = 0 where level = 0.
 *   MET2_TFCE_MODE_EXTENT:  dh is THE threshold h: out(v) = the size of v's component of {t >= h} as a double, 0 outside it.  E and H are
 *             not read.
 *   MET2_TFCE_MODE_MASS:    cluster mass (an extension; additive, the ABI number stays).  dh is THE threshold h, as in extent mode; E and H
 *             are not read.  Membership is extent mode's: t(v) >= h, inside the mask, t a number.  A member contributes the integer
 *             q(v) = (int64) rint(min(t(v), MET2_TFCE_MASS_T_CAP) * 2^MET2_TFCE_MASS_FRAC_BITS), ties to even; the scaling is exact and
 *             +infinity saturates at the cap.  For a member, out(v) = (double)(the sum of q over v's component) * 2^-24: the sum is taken in
 *             64-bit integers (by integer atomic adds at the component's root, so it does not depend on the order), converted ONCE, round to
 *             nearest even, and the scaling is exact.  out(v) = 0 elsewhere.  The sum cannot overflow: q <= 2^38 and a grid of at most
 *             MET2_TFCE_MASS_MAX_G = 2^24 voxels give at most 2^62; a larger grid is MET2_E_UNSUPPORTED in mass mode only, before any device
 *             work (group.py crops the grid to the tested voxels' bounding box).  Consequence: as long as nothing saturates,
 *             |out - the exact sum of t over the component| <= e * 2^-25 + one rounding of the result, e the component's size (measured on the
 *             observed maps of the planted case of tests/tools/tfce_numpy.py against a long double sum: at worst 0.9995 of e * 2^-25).  An
 *             int64 numpy sum reproduces the bits (tests/tools/cluster_mass_numpy.py).  Every permutation is quantised the same way, so
 *             the test stays a valid permutation test -- of the quantised statistic.  Parity with randomise -C / -S is unpinned: FSL sums
 *             the raw doubles and was not available.
 * met2_tfce: maps [K][nx][ny][nz] -> out [K][nx][ny][nz] (must not overlap maps) and, when not NULL, kmax [K] = max over the grid of out
 *   (>= 0; by an integer atomic max per block and map on the key of met2_group_perm_stats).  A map's bits depend on that map, the mask and the
 *   parameters alone: not on K, its place in the batch or the other maps.
 * met2_group_perm_tfce: n, n_vox, Y, s0, r, K, W as for met2_group_perm_stats (one-sided); at [n_vox] int32, strictly ascending: voxel v's
 *   index in the grid.  For each candidate k, t(k, v) is computed by met2_group_perm_stats's own kernel code -- the same sums in the same
 *   order, hence the same bits -- and scattered to a dense map on the grid, with the mask {at[v]}; the maps are transformed as above, and
 *   s(k, v) = out_k(at[v]) gathered:  kmax[k] = max_v s(k, v);  first[v] = s(0, v) when first is not NULL;  count[v] += #{k: s(k, v) >=
 *   ref[v]} when ref is not NULL (count is then required; accumulated over launches; one thread owns a voxel).
 * How.  One union-find forest per map over the grid, kept across the levels, which are walked downward from the batch's top level (one
 *   4-byte device-to-host read per call; nothing per level): voxels of level j unite with their neighbours of level >= j by an integer
 *   atomic min on a parent array with parent[v] <= v; sizes are kept at the roots by integer atomic adds (a voxel adds itself once, at its own
 *   level; a root that stopped being one hands its size on); then every voxel of S_j adds its root's term to its own running sum.  Integer
 *   atomics only; results do not depend on the order of execution.  Every device loop is bounded (a chase or a retry by the voxel count, the
 *   levels by MET2_TFCE_MAX_STEPS); a bound that runs out, or an `at` that is not strictly ascending inside the grid, raises a device flag,
 *   read when the call's work is waited for: MET2_E_HIP, resp. MET2_E_INVALID, and kmax, first and count are then untouched for `at`.
 * Work space.  met2_tfce_work_bytes: the bytes a call needs for K maps on dims (n_vox = 0: met2_tfce, 10 bytes per map and grid voxel: level,
 *   parent, size; n_vox > 0: met2_group_perm_tfce, 18 bytes: the dense map, which becomes the running sum, as well).  work = NULL: the call
 *   allocates and frees it; else a device block of work_bytes >= that (MET2_E_INVALID if smaller).  Either way the call returns after its
 *   work is done.
 * DEVICE pointers throughout but dims.  met2_tfce_limits is host only.
 * Limits.  1 <= K <= MET2_TFCE_MAX_K, nx, ny, nz >= 1 and nx ny nz < 2^31, in mass mode <= 2^24 (MET2_E_UNSUPPORTED beyond the upper ends); the group entry's
 * n, r as above.  MET2_E_INVALID: a mode or connectivity other than those named, dh not finite or <= 0, in TFCE mode E not finite or <= 0 or
 * H not finite or < 0, K or an axis < 1, a NULL required pointer, ref without count.  Every such check comes before any device work: the
 * outputs are then untouched. */
#define MET2_TFCE_MAX_K 32
#define MET2_TFCE_MAX_STEPS 1024
#define MET2_TFCE_MODE_TFCE 0
#define MET2_TFCE_MODE_EXTENT 1
#define MET2_TFCE_MODE_MASS 3              /* 2 is MET2_GROUP_VSM_MODE_VOXEL, which met2_tfce refuses */
#define MET2_TFCE_MASS_FRAC_BITS 24
#define MET2_TFCE_MASS_T_CAP 16384.0
#define MET2_TFCE_MASS_MAX_G (1 << 24)
int met2_tfce_limits(int32_t *max_k, int32_t *max_steps);
int met2_tfce_work_bytes(int32_t K, const int32_t dims[3], int64_t n_vox, int64_t *bytes);
int met2_tfce(int32_t device, int32_t K, const int32_t dims[3], const double *maps, const uint8_t *mask, int32_t mode, double dh, double E,
              double H, int32_t connectivity, double *out, double *kmax, void *work, int64_t work_bytes, void *stream);
int met2_group_perm_tfce(int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t K, const double *W,
                         const int32_t dims[3], const int32_t *at, int32_t mode, double dh, double E, double H, int32_t connectivity,
                         const double *ref, double *first, double *kmax, uint32_t *count, void *work, int64_t work_bytes, void *stream);
/* the F counterpart (stated with met2_group_perm_fstats above) */
int met2_group_perm_ftfce(int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t s, double scale,
                          int32_t K, const double *W, const int32_t dims[3], const int32_t *at, int32_t mode, double dh, double E, double H,
                          int32_t connectivity, const double *ref, double *first, double *kmax, uint32_t *count, void *work, int64_t work_bytes,
                          void *stream);

/* ---- Variance smoothing: the pseudo-t of small-sample studies (csrc/met2_group_vsm.hip) ---------------------------------------------
 * With few degrees of freedom the residual variance of a voxel is noisy and the permutation distribution of the maximum t is driven by voxels
 * whose variance happens to be tiny.  The remedy of Holmes et al. (1996) and Nichols & Holmes (2002), FSL randomise's -v: pool the variance
 * over a Gaussian neighbourhood and test the pseudo-t, cope / sqrt(smoothed variance).
 * Grid, mask, at: as for met2_group_perm_tfce (dims = (nx, ny, nz), z contiguous; the mask of the group entry is {at[v]}).
 * Taps.  taps_a holds 2 R_a + 1 doubles for axis a in x, y, z, with R_a = radius[a], 0 <= R_a <= MET2_GROUP_VSM_MAX_RADIUS.  Every tap is
 *   finite and >= 0 and the centre tap is > 0.  HOST arrays, like dims and radius: the entries do not form them, so no result depends on a
 *   device exp (group.py: smoothing_taps).
 * Masked smoothing S(m) of a map m, which is read as 0 outside the mask.  Three passes in the order x, y, z, each complete over the WHOLE grid
 *   before the next starts: values outside the mask are computed and used in between.  One pass along axis a:
 *       out(p) = sum over d = -R_a .. +R_a, in ascending d, of taps_a[d + R_a] * in(p + d e_a),
 *   the sum from 0.0, a term whose source lies outside the grid skipped, product and sum rounded separately, nothing fused, fp64 throughout.
 *   N = S(the mask's indicator, 1.0 / 0.0), computed once per call.
 * Pseudo-t of candidate k at tested voxel v.  b, g_j, q and rss are met2_group_perm_stats's, by that entry's own kernel code: the same sums in
 *   the same order, the same bits.  rho(k, v) = rss > 0 ? rss : 0 (an rss that is not a number contributes 0 and does not spread);
 *   sigma2(k, v) = S(rho_k)(v) / N(v), one correctly rounded division (N > 0 on the mask since the centre taps are);
 *   pt(k, v) = sigma2 > 0 ? b / sqrt(sigma2) : 0, correctly rounded; two_sided: |pt|.  A b that is not a number gives a pt that is not one:
 *   the maximum passes over it and it reaches no reference.
 * Consequences.  The bits of pt(k, .) depend on W[k], Y, s0, the mask and the taps alone: not on K, the candidate's place, its batch mates,
 *   the tiling or the device; a float64 numpy loop in that order reproduces them (tests/tools/group_vsm_numpy.py).  With taps {[1.0], [1.0],
 *   [1.0]} the result is met2_group_perm_stats's t to the bit: rss * 1.0 / 1.0 is exact.  Cropping the grid to the mask's bounding box changes
 *   no bit: what is cut away holds zeros, and a sum skips a term or adds an exact zero.
 * met2_masked_smooth: maps [K][nx][ny][nz], read as 0 where mask [nx][ny][nz] (uint8; NULL: no mask) is 0 -> out [K][nx][ny][nz] = S at EVERY
 *   grid voxel (must not overlap maps) and, when not NULL, norm_out [nx][ny][nz] = N.  What lies outside the mask in maps (-0, infinities,
 *   values that are not numbers) is not read.
 * met2_group_perm_vsm: n, n_vox, Y, s0, r, K, W, dims, at, dh, E, H, connectivity, ref, first, kmax, count as for met2_group_perm_tfce.  Stages:
 *   b and rho of the batch to dense maps; the three passes; the pseudo-t into a dense map (0 off the mask); then by mode
 *   MET2_GROUP_VSM_MODE_VOXEL: s(k, v) = pt(k, at[v]):  kmax[k] = max_v s(k, v);  first[v] = s(0, v);  count[v] += #{k: s(k, v) >= ref[v]}, with
 *     the meaning they have for met2_group_perm_tfce; dh, E, H and connectivity are not read;
 *   MET2_TFCE_MODE_TFCE, MET2_TFCE_MODE_EXTENT, MET2_TFCE_MODE_MASS: met2_group_perm_tfce's transform and gather on the pseudo-t maps, unchanged.  One-sided:
 *     two_sided = 1 with a spatial mode is MET2_E_INVALID.
 *   Late errors as for met2_group_perm_tfce: an `at` that is not strictly ascending inside the grid is MET2_E_INVALID with kmax, first and
 *   count untouched; a bound of the union-find that ran out is MET2_E_HIP.
 * Work space.  met2_group_vsm_work_bytes(K, dims, n_vox, mode): n_vox = 0: met2_masked_smooth, 8 bytes per map and grid voxel and 8 per grid
 *   voxel; n_vox > 0: met2_group_perm_vsm: b and two maps that take turns (24 bytes per map and grid voxel), N and the mask (9 per grid voxel)
 *   and, in the spatial modes, the forest (10 per map and grid voxel).  work = NULL: the call allocates and frees it; else a device block of
 *   work_bytes >= that (MET2_E_INVALID if smaller).  Either way the call returns after its work is done.
 * DEVICE pointers throughout but dims, radius and the taps.  met2_group_vsm_limits and met2_group_vsm_work_bytes are host only;
 * met2_group_vsm_limits reports MET2_GROUP_VSM_MAX_RADIUS, MET2_GROUP_VSM_MAX_K and the smoothing kernel's tile: samples along the axis of a
 * pass, and lines across it (any output may be NULL).
 * Limits.  1 <= K <= MET2_GROUP_VSM_MAX_K and R_a <= MET2_GROUP_VSM_MAX_RADIUS (MET2_E_UNSUPPORTED beyond), the grid and n, r as for
 * met2_group_perm_tfce.  MET2_E_INVALID: a negative radius, a tap that is not finite or < 0, a centre tap <= 0, out overlapping maps, norm_out
 * overlapping either, a mode other than the four named, a NULL required pointer, ref without count, and what met2_group_perm_tfce refuses.
 * Every such check comes before any device work: the outputs are then untouched.
 * Parity with FSL randomise -v is unpinned (FSL was not available).  The definitions may differ from FSL's in the truncation of the kernel (the
 * caller's taps; group.py cuts at 3 sigma), in the width FSL gives the kernel it smooths its variance image with, and in the normalisation by
 * the smoothed mask. */
#define MET2_GROUP_VSM_MAX_RADIUS 16
#define MET2_GROUP_VSM_MAX_K 32
#define MET2_GROUP_VSM_MODE_VOXEL 2
int met2_group_vsm_limits(int32_t *max_radius, int32_t *max_k, int32_t *tile_axis, int32_t *tile_lines);
int met2_group_vsm_work_bytes(int32_t K, const int32_t dims[3], int64_t n_vox, int32_t mode, int64_t *bytes);
int met2_masked_smooth(int32_t device, int32_t K, const int32_t dims[3], const double *maps, const uint8_t *mask, const int32_t radius[3],
                       const double *taps_x, const double *taps_y, const double *taps_z, double *out, double *norm_out, void *work,
                       int64_t work_bytes, void *stream);
int met2_group_perm_vsm(int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t K, const double *W,
                        int32_t two_sided, const int32_t dims[3], const int32_t *at, int32_t mode, double dh, double E, double H,
                        int32_t connectivity, const int32_t radius[3], const double *taps_x, const double *taps_y, const double *taps_z,
                        const double *ref, double *first, double *kmax, uint32_t *count, void *work, int64_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MET2_HIP_H */
