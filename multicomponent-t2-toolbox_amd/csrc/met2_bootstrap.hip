// met2_bootstrap.hip -- met2_fit_bootstrap / met2_bootstrap_replicates: per-voxel Monte-Carlo uncertainty of the metrics.
//
// An extension with no counterpart in the reference.  Its ingredients are the reference's own: the Rician noise model of its synthetic
// evaluation (scripts_synthetic_data_evaluation/Paper_Comparison/evaluate_all_methods_two_lobes_SNR50_150.py:387-391), the per-voxel noise
// estimate of BayesReg_nnls (intravoxel_algorithms/bayesian_interpolation.py:88-93: sigma from a plain NNLS fit with m - nnz degrees of
// freedom) and the library's fits.  Every voxel is refitted on B replicates M_b = |s_hat + sigma (z1 + i z2)| of its fitted signal; the
// replicate fits go through met2_fit_enqueue_strided on per-plan scratch, chunk after chunk on the caller's stream, and the statistics of every
// chunk's voxels are taken behind its fit.  Three kernels of this file:
//   bootstrap_sigma_kernel   sigma_v from the plain-NNLS pass (one thread per voxel)
//   bootstrap_gen_kernel     the replicate rows of a chunk (one thread per echo; counter-based Philox4x32-10, HBM-write-bound)
//   bootstrap_stats_kernel   mean, std and three quantiles of 7 quantities per voxel (one wave per voxel, bitonic sort in LDS)
// The replicates of a voxel depend on (seed, voxel_id, b, e) alone and every replicate is solved on its own, so the outputs do not depend on
// chunking, call splitting, voxel order or device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "philox.hpp"
#include "wave_ops.hpp"

namespace met2 {
__attribute__((visibility("hidden"))) int plan_reserve(met2_plan *plan, int64_t nvox);      // the plan's per-voxel scratch (met2_hip.hip)
}

namespace {

#define MET2_BOOT_MAX_REP 1024
#define MET2_BOOT_QUANT 7          // MWF, IEWF, FWF, T2_M, T2_IE, TWC, reg
#define MET2_BOOT_STATS 5          // mean, std (ddof 1), quantiles 0.025, 0.5, 0.975

struct GenArgs {
    int64_t nv, v0;                 // voxels of this launch, global index of the first
    int nrep, nte;
    uint32_t k0, k1;                // the seed's two halves
    const double *center;           // [..][nte] fitted signal s_hat of voxel v0 + lv
    const double *sigma;            // [..]
    const int64_t *vid;             // [..] or NULL = the voxel's index in the call
    const int32_t *pstatus;         // [..] point status, or NULL = every voxel gets replicates
    const double *fa;               // [..] or NULL
    double *out;                    // [nv * nrep][nte]
    double *fa_rows;                // [nv * nrep] or NULL
    uint8_t *mask_rows;             // [nv * nrep] or NULL
};

// row = lv * nrep + b; thread per (row, echo).  u1 in (0, 1], u2 in [0, 1) from 53 bits each, Box-Muller, Rician magnitude.
__global__ __launch_bounds__(256) void bootstrap_gen_kernel(GenArgs A)
{
    const int64_t total = A.nv * A.nrep * A.nte;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / A.nte;
        const int e = (int)(i - row * A.nte);
        const int64_t lv = row / A.nrep;
        const int b = (int)(row - lv * A.nrep);
        const int64_t v = A.v0 + lv;
        const bool live = !A.pstatus || (A.pstatus[v] & MET2_ST_FITTED);
        double x = 0.0;
        if (live) {
            const uint64_t id = A.vid ? (uint64_t)A.vid[v] : (uint64_t)v;
            uint32_t c0 = (uint32_t)e, c1 = (uint32_t)b, c2 = (uint32_t)id, c3 = (uint32_t)(id >> 32);
            met2::philox4x32_10(c0, c1, c2, c3, A.k0, A.k1);
            const double u1 = met2::u01_oc(c0, c1), u2 = met2::u01_co(c2, c3);
            const double r = sqrt(-2.0 * log(u1)), t = 6.283185307179586 * u2;
            const double sg = A.sigma[v];
            const double re = A.center[v * A.nte + e] + sg * (r * cos(t)), im = sg * (r * sin(t));
            x = sqrt(re * re + im * im);
        }
        A.out[i] = x;
        if (e == 0) {
            if (A.fa_rows) A.fa_rows[row] = A.fa ? A.fa[v] : 0.0;
            if (A.mask_rows) A.mask_rows[row] = live ? 1 : 0;      // a voxel gated out of its point fit has no replicate fits
        }
    }
}

// sigma_v = sqrt(sum_e (M_e - sig0_e)^2 / max(m - #{fsol0 > 0}, 1))  (bayesian_interpolation.py:88-93 on the plain-NNLS pass)
__global__ __launch_bounds__(256) void bootstrap_sigma_kernel(int64_t nvox, int nte, int nt2, const double *__restrict__ data, int64_t vs, int64_t es,
                                                              const double *__restrict__ fsol0, const double *__restrict__ sig0, double *__restrict__ sigma)
{
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
        double ss = 0.0;
        for (int e = 0; e < nte; ++e) { const double d = data[v * vs + e * es] - sig0[v * nte + e]; ss += d * d; }
        int nnz = 0;
        for (int j = 0; j < nt2; ++j) nnz += fsol0[v * nt2 + j] > 0.0;
        sigma[v] = sqrt(ss / (double)std::max(nte - nnz, 1));
    }
}

struct StatArgs {
    int64_t v0, nvox, rows;         // first voxel of the chunk, voxels of the call (stride of stats), replicate rows of the chunk
    int nrep, npow2;
    const double *maps_r;           // [6][rows]
    const double *reg_r;            // [rows]
    const int32_t *st_r;            // [rows]
    const int32_t *pstatus;         // [nvox]
    double *stats;                  // [7][5][nvox]
    int32_t *rep_status;            // [nvox] or NULL
};

// numpy's ordering for np.sort: nan last
__device__ __forceinline__ bool nan_last_gt(double a, double b) { return a > b || (a != a && b == b); }

// np.quantile(values, p) with method 'linear' on the sorted values: h = (n - 1) p and numpy's _lerp, including its t >= 0.5 branch.
// No contraction: a fused multiply-add would differ from numpy in the last bit.
__device__ double quantile_sorted(const double *s, int n, double p)
{
#pragma clang fp contract(off)
    if (s[n - 1] != s[n - 1]) return s[n - 1];                 // a nan among the values: numpy returns nan
    const double h = (double)(n - 1) * p;
    const double fl = floor(h);
    int i0 = (int)fl, i1 = i0 + 1;
    if (h >= (double)(n - 1)) i0 = i1 = n - 1;
    const double g = h - fl;
    const double a = s[i0], b = s[i1];
    const double d = b - a;
    return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

// one wave (one workgroup) per voxel: for each quantity the B values go to LDS; mean and std in two passes in a fixed order (lane-strided
// partial sums, then wave_sum); then a bitonic sort over the next power of two (nan padding sorts last) and the three quantiles
__global__ __launch_bounds__(64) void bootstrap_stats_kernel(StatArgs A)
{
    __shared__ double buf[MET2_BOOT_MAX_REP];
    const int lane = threadIdx.x;
    const int64_t lv = blockIdx.x, v = A.v0 + lv;
    const int B = A.nrep, P = A.npow2;
    if (!(A.pstatus[v] & MET2_ST_FITTED)) {
        for (int i = lane; i < MET2_BOOT_QUANT * MET2_BOOT_STATS; i += 64) A.stats[i * A.nvox + v] = 0.0;
        if (lane == 0 && A.rep_status) A.rep_status[v] = 0;
        return;
    }
    const int64_t base = lv * B;
    if (A.rep_status) {
        int st = 0;
        for (int b = lane; b < B; b += 64) st |= A.st_r[base + b];
        for (int off = 32; off > 0; off >>= 1) st |= __shfl_xor(st, off);
        if (lane == 0) A.rep_status[v] = st;
    }
    const double qp[3] = {0.025, 0.5, 0.975};
    for (int q = 0; q < MET2_BOOT_QUANT; ++q) {
        const double *src = (q < 6 ? A.maps_r + q * A.rows : A.reg_r) + base;
        for (int i = lane; i < P; i += 64) buf[i] = i < B ? src[i] : __builtin_nan("");
        __syncthreads();
        const double c = buf[0];                                   // shifted sums: identical values give a mean equal to them and std 0
        double s = 0.0;
        for (int b = lane; b < B; b += 64) s += buf[b] - c;
        const double mean = c + met2::wave_sum(s) / (double)B;
        double ss = 0.0;
        for (int b = lane; b < B; b += 64) { const double d = buf[b] - mean; ss += d * d; }
        const double sd = sqrt(met2::wave_sum(ss) / (double)(B - 1));
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = lane; i < P; i += 64) {
                    const int l = i ^ j;
                    if (l > i) {
                        const double x = buf[i], y = buf[l];
                        if ((i & k) == 0 ? nan_last_gt(x, y) : nan_last_gt(y, x)) { buf[i] = y; buf[l] = x; }
                    }
                }
                __syncthreads();
            }
        if (lane < MET2_BOOT_STATS) {
            const double r = lane == 0 ? mean : (lane == 1 ? sd : quantile_sorted(buf, B, qp[lane - 2]));
            A.stats[(q * MET2_BOOT_STATS + lane) * A.nvox + v] = r;
        }
        __syncthreads();
    }
}

// what this entry keeps with a plan: the point pass's scratch (for outputs the caller passes as NULL, and the plain-NNLS pass of the sigma
// estimate) and one chunk of replicate rows.  Grown on demand, freed by met2_plan_destroy (met2::bootstrap_release).
struct BootWork {
    int device = -1;
    int64_t cap_vox = 0, cap_rows = 0;
    char *vox = nullptr;            // sig | sig0 | fsol0 | sigma | reg0 | status
    char *rows = nullptr;           // data | fsol | maps | reg | fa | status | mask
};
std::mutex g_boot_mutex;
std::map<met2_plan *, BootWork> g_boot;

void free_boot(BootWork &w)
{
    if (w.device < 0) return;
    DevGuard dg(w.device);
    if (w.vox) (void)hipFree(w.vox);
    if (w.rows) (void)hipFree(w.rows);
    w = BootWork();
}

int grow(char *&buf, int64_t &cap, int64_t need, size_t bytes_per)
{
    if (need <= cap) return MET2_OK;
    if (buf) { HIPCHK(hipFree(buf)); buf = nullptr; cap = 0; }
    HIPCHK(hipMalloc(&buf, bytes_per * (size_t)need));
    cap = need;
    return MET2_OK;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int plan_shape(met2_plan *plan, int &nte, int &nt2, int &device)
{
    int32_t a = 0, b = 0;
    int rc = met2_plan_get_shape(plan, &a, &b, nullptr);
    if (rc) return rc;
    met2_options o;
    rc = met2_plan_get_options(plan, &o);
    if (rc) return rc;
    nte = a; nt2 = b; device = o.device;
    return MET2_OK;
}

int gen_grid(int64_t total) { return (int)std::min<int64_t>((total + 255) / 256, 65536); }

}  // namespace

namespace met2 {
// called by met2_plan_destroy
__attribute__((visibility("hidden"))) void bootstrap_release(met2_plan *plan)
{
    BootWork w;
    {
        std::lock_guard<std::mutex> lock(g_boot_mutex);
        auto it = g_boot.find(plan);
        if (it == g_boot.end()) return;
        w = it->second;
        g_boot.erase(it);
    }
    free_boot(w);
}
}  // namespace met2

extern "C" int met2_bootstrap_replicates(met2_plan *plan, int64_t nvox, const double *center, const double *sigma, const int64_t *voxel_id,
                                         int32_t n_rep, int64_t seed, double *out, void *stream)
{
    if (n_rep < 2 || n_rep > MET2_BOOT_MAX_REP) return fail(MET2_E_INVALID, "n_rep must lie in [2, 1024]");
    if (nvox < 0 || nvox > 0x7fffffff) return fail(MET2_E_INVALID, "nvox out of range");
    if (!plan) return fail(MET2_E_INVALID, "NULL plan");
    if (nvox == 0) return MET2_OK;
    if (!center || !sigma || !out) return fail(MET2_E_INVALID, "NULL argument");
    int nte, nt2, dev;
    int rc = plan_shape(plan, nte, nt2, dev);
    if (rc) return rc;
    USE_DEVICE(dev);
    GenArgs A;
    A.nv = nvox; A.v0 = 0; A.nrep = n_rep; A.nte = nte;
    A.k0 = (uint32_t)(uint64_t)seed; A.k1 = (uint32_t)((uint64_t)seed >> 32);
    A.center = center; A.sigma = sigma; A.vid = voxel_id; A.pstatus = nullptr; A.fa = nullptr;
    A.out = out; A.fa_rows = nullptr; A.mask_rows = nullptr;
    hipLaunchKernelGGL(bootstrap_gen_kernel, dim3(gen_grid(nvox * n_rep * nte)), dim3(256), 0, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_fit_bootstrap(met2_plan *plan, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                                  const double *fa_index, const uint8_t *mask, const int64_t *voxel_id, const double *sigma, int32_t n_rep,
                                  int64_t seed, double *fsol, double *sig, double *reg, double *lam, double *maps, int32_t *status,
                                  double *sigma_out, double *stats, int32_t *rep_status, void *stream)
{
    // argument checks first: nothing here touches a device
    if (n_rep < 2 || n_rep > MET2_BOOT_MAX_REP) return fail(MET2_E_INVALID, "n_rep must lie in [2, 1024]");
    if (nvox < 0 || nvox > 0x7fffffff) return fail(MET2_E_INVALID, "nvox out of range");
    if (voxel_stride <= 0 || echo_stride <= 0) return fail(MET2_E_INVALID, "strides must be positive");
    if (!plan) return fail(MET2_E_INVALID, "NULL plan");
    if (method < MET2_NNLS || method > MET2_BAYESREG) return fail(MET2_E_INVALID, "unknown method");
    if (nvox == 0) return MET2_OK;
    if (!data || !fsol || !reg || !stats) return fail(MET2_E_INVALID, "NULL argument");
    int nte, nt2, dev;
    int rc = plan_shape(plan, nte, nt2, dev);
    if (rc) return rc;
    USE_DEVICE(dev);
    hipStream_t s = (hipStream_t)stream;
    // replicate rows per internal fit: 262 144; L-curve at two bins per lane 4 096, where the spill-over kernel's record cap
    // (min(rows, max(4 096, rows / 16)), met2_hip.hip) covers every row -- past it the outcome would depend on arrival order.
    // A chunk holds whole voxels, so that their statistics follow its fit.
    const int64_t rmax = (method == MET2_LCURVE && nt2 > 64) ? 4096 : 262144;
    const int64_t vpc = std::min<int64_t>(nvox, std::max<int64_t>(1, rmax / n_rep));
    const int64_t rcap = vpc * n_rep;
    int npow2 = 1;
    while (npow2 < n_rep) npow2 <<= 1;
    BootWork *w;
    {
        std::lock_guard<std::mutex> lock(g_boot_mutex);
        w = &g_boot[plan];
    }
    w->device = dev;
    const size_t vox_bytes = align256(sizeof(double) * (2 * nte + nt2 + 2) + sizeof(int32_t));
    const size_t row_bytes = align256(sizeof(double) * (nte + nt2 + 8) + sizeof(int32_t) + 1);
    rc = grow(w->vox, w->cap_vox, nvox, vox_bytes);
    if (rc) return rc;
    rc = grow(w->rows, w->cap_rows, rcap, row_bytes);
    if (rc) return rc;
    rc = met2::plan_reserve(plan, std::max(nvox, rcap));       // the sort scratch is sized once, before anything is enqueued
    if (rc) return rc;
    double *v_sig = (double *)w->vox, *v_sig0 = v_sig + nvox * nte, *v_fsol0 = v_sig0 + nvox * nte, *v_sigma = v_fsol0 + nvox * nt2;
    double *v_reg0 = v_sigma + nvox;
    int32_t *v_st = (int32_t *)(v_reg0 + nvox);
    double *r_data = (double *)w->rows, *r_fsol = r_data + rcap * nte, *r_maps = r_fsol + rcap * nt2, *r_reg = r_maps + 6 * rcap, *r_fa = r_reg + rcap;
    int32_t *r_st = (int32_t *)(r_fa + rcap);
    uint8_t *r_mask = (uint8_t *)(r_st + rcap);

    // 1. the point fit, exactly met2_fit's
    double *psig = sig ? sig : v_sig;
    int32_t *pst = status ? status : v_st;
    rc = met2_fit_enqueue_strided(plan, method, nvox, data, voxel_stride, echo_stride, fa_index, mask, fsol, psig, reg, lam, maps, pst, stream);
    if (rc) return rc;
    // 2. sigma: given, or from a plain-NNLS pass on the raw echoes at the voxel's flip angle
    const double *sg = sigma;
    if (sigma) {
        if (sigma_out && sigma_out != sigma) HIPCHK(hipMemcpyAsync(sigma_out, sigma, sizeof(double) * (size_t)nvox, hipMemcpyDeviceToDevice, s));
    } else {
        rc = met2_fit_enqueue_strided(plan, MET2_NNLS, nvox, data, voxel_stride, echo_stride, fa_index, mask, v_fsol0, v_sig0, v_reg0, nullptr, nullptr,
                                      nullptr, stream);
        if (rc) return rc;
        double *so = sigma_out ? sigma_out : v_sigma;
        hipLaunchKernelGGL(bootstrap_sigma_kernel, dim3(gen_grid(nvox)), dim3(256), 0, s, nvox, nte, nt2, data, voxel_stride, echo_stride, v_fsol0, v_sig0, so);
        HIPCHK(hipGetLastError());
        sg = so;
    }
    // one wait: an FA index outside the dictionary is reported before any replicate is fitted
    rc = met2_plan_finish(plan, stream);
    if (rc) return rc;
    // 3.-5. chunk after chunk: replicate rows, their fits (enqueued, no wait), the statistics of the chunk's voxels
    GenArgs G;
    G.nrep = n_rep; G.nte = nte; G.k0 = (uint32_t)(uint64_t)seed; G.k1 = (uint32_t)((uint64_t)seed >> 32);
    G.center = psig; G.sigma = sg; G.vid = voxel_id; G.pstatus = pst; G.fa = fa_index;
    G.out = r_data; G.fa_rows = r_fa; G.mask_rows = r_mask;
    StatArgs S;
    S.nvox = nvox; S.nrep = n_rep; S.npow2 = npow2; S.maps_r = r_maps; S.reg_r = r_reg; S.st_r = r_st; S.pstatus = pst; S.stats = stats; S.rep_status = rep_status;
    for (int64_t v0 = 0; v0 < nvox; v0 += vpc) {
        const int64_t nv = std::min(vpc, nvox - v0), rows = nv * n_rep;
        G.nv = nv; G.v0 = v0;
        hipLaunchKernelGGL(bootstrap_gen_kernel, dim3(gen_grid(rows * nte)), dim3(256), 0, s, G);
        HIPCHK(hipGetLastError());
        rc = met2_fit_enqueue_strided(plan, method, rows, r_data, nte, 1, r_fa, r_mask, r_fsol, nullptr, r_reg, nullptr, r_maps, r_st, stream);
        if (rc) return rc;
        S.v0 = v0; S.rows = rows;
        hipLaunchKernelGGL(bootstrap_stats_kernel, dim3((unsigned)nv), dim3(64), 0, s, S);
        HIPCHK(hipGetLastError());
    }
    return met2_plan_finish(plan, stream);
}
