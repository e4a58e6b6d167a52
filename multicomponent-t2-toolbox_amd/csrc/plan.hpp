// plan.hpp -- struct met2_plan and the hidden functions that cross translation units of libmet2_hip.so, each declared here ONCE.
// Internal (not installed).  Included by every unit that looks into a plan or calls across units, and by the solver headers for the two
// constants below; it includes none of them (nnls_wave.hpp, objectives.hpp, fit_kernel.hpp), so the units beside the fit stay quick to compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/met2_hip.h"

#ifndef MET2_BAYES_TABLE
#define MET2_BAYES_TABLE 10               // shared Brent abscissae with plan-level factors (0 disables the tables)
#endif
#define MET2_GCV_LR_RANK 16               // columns of GCV's low-rank basis per flip angle (objectives.hpp, "Round 4"; gcv_basis_kernel)

struct met2_plan {
    int n_te, n_t2, n_fa;
    met2_options opt;
    int cus;
    double *dD = nullptr;       // [nfa][nte][nt2]
    double *dB = nullptr;       // [nfa][nt2][nt2]
    double *dKband = nullptr;   // [5][64]
    double *dLband = nullptr;   // [5][64]
    double *dDt = nullptr;      // [n_fa][n_t2][n_te] transposed dictionary
    double *dKd = nullptr;      // [n_t2][n_t2] dense L^T L (row loads of the warm-start refactorisation)
    double *dLam = nullptr;     // [nlam]
    double *dT2 = nullptr;      // [nt2]
    int nlam = 0;
    bool have_dict = false, have_pen = false, have_t2 = false;
    std::vector<double> Lhost;  // dense penalty as given
    double log_detL = 0.0;      // log(det(L)) as bayesian_interpolation.py:100,123 uses it (-inf for L2)
    // sort buffers (grown on demand)
    int64_t cap_vox = 0;
    int *dKey = nullptr, *dPerm = nullptr, *dSmall = nullptr, *dOvf = nullptr;      // dSmall: hist|cursor|bucket_start|chunk_start|queue|err
    char *dSeed = nullptr;                                // seed_kernel's output: [4][nfa] SeedRec
    bool seeds_valid = false; double seeds_key[7] = {0};  // (t2sparc_lambda and the six interval ends the seeds and tables were built for)
    bool seeds_ok = false;                                // B + lambda K is positive definite at the seed lambdas (checked on the host for
                                                          // flip angle 0): only then is the seeded start the cold start's solution
    double *dH = nullptr; int64_t cap_h = 0;              // FA walk: h of every flip angle for one pass of voxels (fa_project_kernel), grown on demand
    double *dBtab = nullptr; int btab_stride = 0;         // BayesReg factor tables [nfa][MET2_BAYES_TABLE][btab_stride] (built with the seeds)
    double *dQt = nullptr;                                // [nfa][16][n_te]: the basis vectors themselves (lower bounds of the brute-force FA search)
    double *dAq = nullptr, *dAqRes = nullptr;             // GCV: [nfa][n_t2][16] = (Q^T D)^T in the flip angle's low-rank basis, [nfa] what the basis leaves of D
    double gcv_res = 0.0;                                 // the largest of dAqRes
    bool gcv_lr = false;                                  // every flip angle's dictionary is of numerical rank <= 16: the GCV trace takes the 17 x 17 form
    double *dChol = nullptr; int64_t cap_chol = 0;        // BayesReg at two bins per lane: one packed factor per resident wave (chol_lean), grown on demand
    double *dLcSave = nullptr; int64_t cap_lc = 0;        // L-curve at two bins per lane: the sweep states of queued voxels (fit_kernel.hpp: FitArgs::lc_save) and, behind them, lc_at
    double *dBig = nullptr; int64_t cap_big = 0;          // the waves' spill-over slots: factor columns beyond the LDS capacity (nnls_big.hpp), grown on demand
    int last_spill = 0;                                   // voxels of the last finished fit(s) that used them
    double blam[MET2_BAYES_TABLE > 0 ? MET2_BAYES_TABLE : 1];
    int *hErr = nullptr;                                  // pinned [4]: the FA-range error word of an enqueued fit lands here, and its spill-over queue's tail (= count) and head
    bool err_pending = false;
    hipStream_t err_stream = nullptr;                     // the stream the fits since the last finish were enqueued on (one plan serves one stream at a time)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    bool timed = false, timed2 = false;
};

namespace met2 {
// met2_hip.hip
__attribute__((visibility("hidden"))) int plan_reserve(met2_plan *plan, int64_t nvox);      // the plan's per-voxel scratch for blocks of nvox voxels, reserved before a block loop
__attribute__((visibility("hidden"))) int ensure_seeds(met2_plan *plan, hipStream_t s);     // the plan-level seeds and factor tables, rebuilt when dictionary, penalty or options changed; blocks
// met2_dictionary.hip
__attribute__((visibility("hidden"))) int build_gram(met2_plan *plan, hipStream_t s);       // everything derived from the dictionary alone; blocks
// met2_prefilter.hip
__attribute__((visibility("hidden"))) void spline_tables_release();                         // for host threads that end: frees the calling thread's FA spline tables
// met2_host.hip
__attribute__((visibility("hidden"))) void host_release(met2_plan *plan);                   // called by met2_plan_destroy: what met2_fit_host keeps with the plan
__attribute__((visibility("hidden"))) bool fa_spline_attachment(met2_plan *plan, met2_plan **plan_lr, std::vector<double> *alpha_lr,
                                                                std::vector<double> *alpha_hr);   // a copy of what met2_plan_attach_fa_spline left with the plan; false if nothing is attached
// met2_bootstrap.hip
__attribute__((visibility("hidden"))) void bootstrap_release(met2_plan *plan);              // called by met2_plan_destroy: what met2_fit_bootstrap keeps with the plan
__attribute__((visibility("hidden"))) int rician_scratch(met2_plan *plan, int device, size_t bytes, char **out);      // `bytes` of scratch kept with the plan until met2_plan_destroy
__attribute__((visibility("hidden"))) int noise_sigma_enqueue(met2_plan *plan, int nte, int nt2, int64_t nvox, const double *data, int64_t vs, int64_t es,
                                                              const double *fa_index, const uint8_t *mask, double *fsol0, double *sig0, double *reg0,
                                                              double *sigma_out, void *stream);   // the sigma estimate of met2_noise_sigma on scratch of the caller's
}  // namespace met2
