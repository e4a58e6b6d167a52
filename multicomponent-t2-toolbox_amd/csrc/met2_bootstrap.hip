// met2_bootstrap.hip -- met2_fit_bootstrap / met2_bootstrap_replicates: per-voxel Monte-Carlo uncertainty of the metrics.
//
// An extension with no counterpart in the reference.  Its ingredients are the reference's own: the Rician noise model of its synthetic
// evaluation (scripts_synthetic_data_evaluation/Paper_Comparison/evaluate_all_methods_two_lobes_SNR50_150.py:387-391), the per-voxel noise
// estimate of BayesReg_nnls (intravoxel_algorithms/bayesian_interpolation.py:88-93: sigma from a plain NNLS fit with m - nnz degrees of
// freedom) and the library's fits.  Every voxel is refitted on B replicates M_b = |s_hat + sigma (z1 + i z2)| of its fitted signal; the
// replicate fits go through met2_fit_enqueue_strided on per-plan scratch, chunk after chunk on the caller's stream, and the statistics of every
// chunk's voxels are taken behind its fit.  met2_fit_bootstrap_fa re-estimates the flip angle of every replicate row before its fit (the
// plan's brute-force walk, or the coarse walk and the spline selection) and can return the statistics of the replicates' spectra per T2 bin.
// met2_noise_sigma is that noise estimate on its own (noise_sigma_enqueue: the one copy the bootstrap and met2_fit_rician, met2_rician.hip, take it from).
// Four kernels of this file:
//   bootstrap_sigma_kernel        sigma_v from the plain-NNLS pass (one thread per voxel)
//   bootstrap_gen_kernel          the replicate rows of a chunk (one thread per echo; counter-based Philox4x32-10, HBM-write-bound)
//   bootstrap_stats_kernel        mean, std and three quantiles of 7 (8 with the FA index) quantities per voxel (one wave per voxel)
//   bootstrap_spec_stats_kernel   the same statistics of every T2 bin of the replicates' spectra (one workgroup per voxel, tiles of bins
//                                 transposed through LDS, one series per wave at a time)
// Both statistics kernels reduce and sort a series with series_stats: the bit-level contract has one implementation.
// met2_bootstrap_series_stats / met2_bootstrap_spectrum_stats launch the two on values of the caller's (no plan, no fit).
// The replicates of a voxel depend on (seed, voxel_id, b, e) alone and every replicate is solved on its own, so the outputs do not depend on
// chunking, call splitting, voxel order or device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_helpers.hpp"
#include "philox.hpp"
#include "plan.hpp"
#include "quantile.hpp"
#include "wave_ops.hpp"

namespace {

#define MET2_BOOT_MAX_REP 1024
#define MET2_BOOT_QUANT 7          // MWF, IEWF, FWF, T2_M, T2_IE, TWC, reg
#define MET2_BOOT_QUANT_FA 8       // ... and the FA index (met2_fit_bootstrap_fa)
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
    int nrep, npow2, nquant;        // nquant: 7, or 8 with the FA index
    const double *maps_r;           // [6][rows]
    const double *reg_r;            // [rows]
    const double *fa_r;             // [rows] (nquant = 8)
    const int32_t *st_r;            // [rows]
    const int32_t *pstatus;         // [nvox]
    double *stats;                  // [nquant][5][nvox]
    int32_t *rep_status;            // [nvox] or NULL
};

// np.quantile(values, p) with method 'linear' on the sorted values: quantile.hpp, shared with met2_stats.hip
using met2::quantile_sorted;

// The statistics of one series, by one wave: buf[0..B) holds the values and buf[B..P) nan (P = the next power of two), written by anyone
// and made visible to this wave before the call.  Mean and std in two passes in a fixed order (lane-strided partial sums, then wave_sum);
// then a bitonic sort over P (the nan padding sorts last) and the three quantiles.  Lane s < 5 returns statistic s; buf is left sorted.
// SKIP_EQUAL: a series of B identical finite values (bit patterns; not -0.0, whose sums and lerps give +0.0) needs no sort -- the long way
// gives mean = c + 0 / B = c, std = sqrt(0 / (B - 1)) = 0 and quantiles a + 0 g = b - 0 (1 - g) = c, the same bits.
template <bool SKIP_EQUAL>
__device__ __forceinline__ double series_stats(double *buf, int B, int P, int lane)
{
    const double qp[3] = {0.025, 0.5, 0.975};
    const double c = buf[0];                                   // shifted sums: identical values give a mean equal to them and std 0
    if (SKIP_EQUAL) {
        const long long cb = __double_as_longlong(c);
        bool same = cb != (long long)0x8000000000000000ull && c - c == 0.0;
        for (int b = lane; b < B; b += 64) same = same && __double_as_longlong(buf[b]) == cb;
        if (__all(same)) return lane == 1 ? 0.0 : c;
    }
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
            wave_lds_sync();
        }
    double r = 0.0;
    if (lane < MET2_BOOT_STATS) r = lane == 0 ? mean : (lane == 1 ? sd : quantile_sorted(buf, B, qp[lane - 2]));
    return r;
}

// one wave (one workgroup) per voxel: for each quantity the B values go to LDS (read with unit stride from the [q][rows] arrays) and
// through series_stats
__global__ __launch_bounds__(64) void bootstrap_stats_kernel(StatArgs A)
{
    __shared__ double buf[MET2_BOOT_MAX_REP];
    const int lane = threadIdx.x;
    const int64_t lv = blockIdx.x, v = A.v0 + lv;
    const int B = A.nrep, P = A.npow2;
    if (!(A.pstatus[v] & MET2_ST_FITTED)) {
        for (int i = lane; i < A.nquant * MET2_BOOT_STATS; i += 64) A.stats[i * A.nvox + v] = 0.0;
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
    for (int q = 0; q < A.nquant; ++q) {
        const double *src = (q < 6 ? A.maps_r + q * A.rows : (q == 6 ? A.reg_r : A.fa_r)) + base;
        for (int i = lane; i < P; i += 64) buf[i] = i < B ? src[i] : __builtin_nan("");
        __syncthreads();
        const double r = series_stats<false>(buf, B, P, lane);
        if (lane < MET2_BOOT_STATS) A.stats[(q * MET2_BOOT_STATS + lane) * A.nvox + v] = r;
        __syncthreads();
    }
}

struct SpecArgs {
    int64_t v0, nvox;               // first voxel of the chunk, voxels of the call
    int nrep, npow2, nt2;
    int w, lw, S;                   // bins per tile (a power of two, 2^lw), doubles between two series of the tile
    const double *fsol_r;           // [rows][nt2] the chunk's replicate spectra
    const int32_t *pstatus;         // [nvox]
    double *spec;                   // [5][nvox][nt2]
};

#define MET2_SPEC_WAVES 4
#ifndef MET2_BOOT_SPEC_SKIP_EQUAL
#define MET2_BOOT_SPEC_SKIP_EQUAL true     // series_stats' shortcut for constant series in the spectrum kernel (false: for measuring it)
#endif
// bins per tile for series of P sort slots: w P = 4 096 doubles (32 KiB) from P = 64 on, 64 bins below.  With the padding and the [5][w]
// staging of the results a workgroup takes 33 .. 36 KiB of LDS, so four workgroups (16 waves) share a CU's 160 KiB.
inline int spec_tile_bins(int P) { return P <= 64 ? 64 : 4096 / P; }
// A series is a row of the tile, S = P + pad doubles long.  The transposing store puts lane (j, b) at double j S + b with the bin j running
// fastest over min(w, 16) lanes; ds_write_b64 is served in groups of 16 consecutive lanes over 32 banks of 4 bytes = 16 doubles.  S odd
// spreads 16 bins over the 16 double-banks; with w < 16 a group holds 16 / w replicates of each bin, and S = 16 / w (mod 16) keeps
// (j S + b) mod 16 distinct.  The sort then reads and writes a series with unit stride, which is conflict-free at any S.
inline int spec_tile_pad(int w) { return w >= 16 ? 1 : 16 / w; }
// The launch geometry of bootstrap_spec_stats_kernel for series of n_rep values, the one copy every launch site and
// met2_bootstrap_spec_launch_info take it from: sort slots, tile shape and the dynamic LDS ([w][S] tile and [5][w] results) in bytes.
struct SpecGeom { int P, w, lw, S; size_t lds; };
inline SpecGeom spec_geometry(int n_rep)
{
    SpecGeom g;
    g.P = next_pow2(n_rep);
    g.w = spec_tile_bins(g.P);
    g.S = g.P + spec_tile_pad(g.w);
    g.lw = 0;
    while ((1 << g.lw) < g.w) ++g.lw;
    g.lds = sizeof(double) * ((size_t)g.w * g.S + MET2_BOOT_STATS * g.w);
    return g;
}
#define MET2_SPEC_LDS_MAX 65536     // the dynamic LDS a kernel gets without asking for more

// One workgroup of four waves per voxel.  The voxel's [B][nt2] block of the chunk's fsol is taken in tiles of w bins: loaded with the lanes
// along the bin axis (w consecutive doubles of a row; reading one bin's B values directly would fetch a 64-byte line for every 8 bytes),
// stored transposed, and then every wave takes whole series through series_stats.  The results of a tile are staged in LDS and written with
// the lanes along the bin axis again.
template <bool SKIP_EQUAL>
__global__ __launch_bounds__(64 * MET2_SPEC_WAVES) void bootstrap_spec_stats_kernel(SpecArgs A)
{
    extern __shared__ double spec_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t lv = blockIdx.x, v = A.v0 + lv;
    const int B = A.nrep, P = A.npow2, n = A.nt2, w = A.w, S = A.S;
    double *tile = spec_lds, *res = spec_lds + w * S;          // [w][S], [5][w]
    if (!(A.pstatus[v] & MET2_ST_FITTED)) {
        for (int i = tid; i < MET2_BOOT_STATS * n; i += 64 * MET2_SPEC_WAVES) {
            const int s = i / n, j = i - s * n;
            A.spec[((int64_t)s * A.nvox + v) * n + j] = 0.0;
        }
        return;
    }
    const double *src = A.fsol_r + lv * B * n;
    for (int j0 = 0; j0 < n; j0 += w) {
        const int wj = min(w, n - j0);
        for (int i = tid; i < P * w; i += 64 * MET2_SPEC_WAVES) {
            const int j = i & (w - 1), b = i >> A.lw;
            if (j < wj) tile[j * S + b] = b < B ? src[(int64_t)b * n + j0 + j] : __builtin_nan("");
        }
        __syncthreads();
        for (int j = wave; j < wj; j += MET2_SPEC_WAVES) {
            const double r = series_stats<SKIP_EQUAL>(tile + j * S, B, P, lane);
            if (lane < MET2_BOOT_STATS) res[lane * w + j] = r;
        }
        __syncthreads();
        for (int i = tid; i < MET2_BOOT_STATS * wj; i += 64 * MET2_SPEC_WAVES) {
            const int s = i / wj, j = i - s * wj;
            A.spec[((int64_t)s * A.nvox + v) * n + j0 + j] = res[s * w + j];
        }
        // the next tile's loads overwrite `tile`, which every wave has left behind the barrier above; `res` is written again only behind the
        // next tile's first barrier, which these reads precede
    }
}

// what this entry keeps with a plan: the point pass's scratch (for outputs the caller passes as NULL, and the plain-NNLS pass of the sigma
// estimate) and one chunk of replicate rows.  Grown on demand, freed by met2_plan_destroy (met2::bootstrap_release).
struct BootWork {
    int device = -1;
    int64_t cap_vox = 0, cap_rows = 0;
    char *vox = nullptr;            // sig | sig0 | fsol0 | sigma | reg0 | status
    char *rows = nullptr;           // data | fsol | maps | reg | fa | status | mask
    int64_t cap_aux = 0;            // bytes
    char *aux = nullptr;            // spline mode: the coarse walk's residuals [rows][n_lr]
    int64_t cap_ric = 0;            // bytes
    char *ric = nullptr;            // met2_fit_rician's scratch (met2_rician.hip lays it out)
};
std::mutex g_boot_mutex;
std::map<met2_plan *, BootWork> g_boot;

void free_boot(BootWork &w)
{
    if (w.device < 0) return;
    DevGuard dg(w.device);
    if (w.vox) (void)hipFree(w.vox);
    if (w.rows) (void)hipFree(w.rows);
    if (w.aux) (void)hipFree(w.aux);
    if (w.ric) (void)hipFree(w.ric);
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

// met2_fit_rician's scratch: `bytes` kept with the plan like the bootstrap's own
__attribute__((visibility("hidden"))) int rician_scratch(met2_plan *plan, int device, size_t bytes, char **out)
{
    BootWork *w;
    {
        std::lock_guard<std::mutex> lock(g_boot_mutex);
        w = &g_boot[plan];
    }
    w->device = device;
    const int rc = grow(w->ric, w->cap_ric, (int64_t)bytes, 1);
    *out = w->ric;
    return rc;
}

// The noise estimate of bayesian_interpolation.py:88-93 on the raw echoes, enqueued on `stream`: a plain-NNLS pass at the voxel's flip angle into
// fsol0 [nvox][nt2], sig0 [nvox][nte] and reg0 [nvox] (scratch of the caller's), then bootstrap_sigma_kernel.  The one copy that met2_fit_bootstrap,
// met2_noise_sigma and met2_fit_rician take sigma_v from.
__attribute__((visibility("hidden"))) int noise_sigma_enqueue(met2_plan *plan, int nte, int nt2, int64_t nvox, const double *data, int64_t vs, int64_t es,
                                                              const double *fa_index, const uint8_t *mask, double *fsol0, double *sig0, double *reg0,
                                                              double *sigma_out, void *stream)
{
    int rc = met2_fit_enqueue_strided(plan, MET2_NNLS, nvox, data, vs, es, fa_index, mask, fsol0, sig0, reg0, nullptr, nullptr, nullptr, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(bootstrap_sigma_kernel, dim3(gen_grid(nvox)), dim3(256), 0, (hipStream_t)stream, nvox, nte, nt2, data, vs, es, fsol0, sig0, sigma_out);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}
}  // namespace met2

extern "C" int met2_noise_sigma(met2_plan *plan, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride, const double *fa_index,
                                const uint8_t *mask, double *sigma_out, double *sig0, void *stream)
{
    if (nvox < 0 || nvox > 0x7fffffff) return fail(MET2_E_INVALID, "nvox out of range");
    if (voxel_stride <= 0 || echo_stride <= 0) return fail(MET2_E_INVALID, "strides must be positive");
    if (!plan) return fail(MET2_E_INVALID, "NULL plan");
    if (nvox == 0) return MET2_OK;
    if (!data || !sigma_out) return fail(MET2_E_INVALID, "NULL argument");
    int nte, nt2, dev;
    int rc = plan_shape(plan, nte, nt2, dev);
    if (rc) return rc;
    USE_DEVICE(dev);
    BootWork *w;
    {
        std::lock_guard<std::mutex> lock(g_boot_mutex);
        w = &g_boot[plan];
    }
    w->device = dev;
    rc = grow(w->vox, w->cap_vox, nvox, align256(sizeof(double) * (2 * nte + nt2 + 2) + sizeof(int32_t)));      // boot_impl's bytes per voxel
    if (rc) return rc;
    double *v_sig0 = (double *)w->vox, *v_fsol0 = v_sig0 + nvox * nte, *v_reg0 = v_fsol0 + nvox * nt2;
    rc = met2::noise_sigma_enqueue(plan, nte, nt2, nvox, data, voxel_stride, echo_stride, fa_index, mask, v_fsol0, sig0 ? sig0 : v_sig0, v_reg0, sigma_out,
                                   stream);
    if (rc) return rc;
    return met2_plan_finish(plan, stream);       // reports an FA index outside the dictionary
}

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

namespace {

// met2_fit_bootstrap (fa_mode FIXED, nquant 7, no spec_stats) and met2_fit_bootstrap_fa (nquant 8)
int boot_impl(met2_plan *plan, int32_t method, int32_t fa_mode, int nquant, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
              const double *fa_index, const uint8_t *mask, const int64_t *voxel_id, const double *sigma, int32_t n_rep, int64_t seed, double *fsol,
              double *sig, double *reg, double *lam, double *maps, int32_t *status, double *sigma_out, double *stats, double *spec_stats,
              int32_t *rep_status, void *stream)
{
    // argument checks first: nothing here touches a device
    if (n_rep < 2 || n_rep > MET2_BOOT_MAX_REP) return fail(MET2_E_INVALID, "n_rep must lie in [2, 1024]");
    if (nvox < 0 || nvox > 0x7fffffff) return fail(MET2_E_INVALID, "nvox out of range");
    if (voxel_stride <= 0 || echo_stride <= 0) return fail(MET2_E_INVALID, "strides must be positive");
    if (!plan) return fail(MET2_E_INVALID, "NULL plan");
    if (method < MET2_NNLS || method > MET2_BAYESREG) return fail(MET2_E_INVALID, "unknown method");
    if (fa_mode < MET2_BOOT_FA_FIXED || fa_mode > MET2_BOOT_FA_SPLINE) return fail(MET2_E_INVALID, "unknown fa_mode");
    met2_plan *plan_lr = nullptr;
    std::vector<double> alpha_lr, alpha_hr;
    if (fa_mode == MET2_BOOT_FA_SPLINE && !met2::fa_spline_attachment(plan, &plan_lr, &alpha_lr, &alpha_hr))
        return fail(MET2_E_STATE, "fa_mode = MET2_BOOT_FA_SPLINE needs met2_plan_attach_fa_spline on the plan first");
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
    const SpecGeom geo = spec_geometry(n_rep);
    const int npow2 = geo.P;
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
    const int n_lr = (int)alpha_lr.size();
    if (plan_lr) {                                             // the coarse walk's residuals, and the coarse plan's own scratch
        rc = grow(w->aux, w->cap_aux, (int64_t)sizeof(double) * rcap * n_lr, 1);
        if (rc) return rc;
        rc = met2::plan_reserve(plan_lr, rcap);
        if (rc) return rc;
    }
    double *v_sig = (double *)w->vox, *v_sig0 = v_sig + nvox * nte, *v_fsol0 = v_sig0 + nvox * nte, *v_sigma = v_fsol0 + nvox * nt2;
    double *v_reg0 = v_sigma + nvox;
    int32_t *v_st = (int32_t *)(v_reg0 + nvox);
    double *r_data = (double *)w->rows, *r_fsol = r_data + rcap * nte, *r_maps = r_fsol + rcap * nt2, *r_reg = r_maps + 6 * rcap, *r_fa = r_reg + rcap;
    int32_t *r_st = (int32_t *)(r_fa + rcap);
    uint8_t *r_mask = (uint8_t *)(r_st + rcap);
    double *r_res = (double *)w->aux;

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
        double *so = sigma_out ? sigma_out : v_sigma;
        rc = met2::noise_sigma_enqueue(plan, nte, nt2, nvox, data, voxel_stride, echo_stride, fa_index, mask, v_fsol0, v_sig0, v_reg0, so, stream);
        if (rc) return rc;
        sg = so;
    }
    // one wait: an FA index outside the dictionary is reported before any replicate is fitted
    rc = met2_plan_finish(plan, stream);
    if (rc) return rc;
    // 3.-5. chunk after chunk: replicate rows, [their flip angles,] their fits (enqueued, no wait), the statistics of the chunk's voxels
    GenArgs G;
    G.nrep = n_rep; G.nte = nte; G.k0 = (uint32_t)(uint64_t)seed; G.k1 = (uint32_t)((uint64_t)seed >> 32);
    G.center = psig; G.sigma = sg; G.vid = voxel_id; G.pstatus = pst; G.fa = fa_index;
    G.out = r_data; G.fa_rows = r_fa; G.mask_rows = r_mask;
    StatArgs S;
    S.nvox = nvox; S.nrep = n_rep; S.npow2 = npow2; S.nquant = nquant; S.maps_r = r_maps; S.reg_r = r_reg; S.fa_r = r_fa; S.st_r = r_st; S.pstatus = pst;
    S.stats = stats; S.rep_status = rep_status;
    SpecArgs Q;
    Q.nvox = nvox; Q.nrep = n_rep; Q.npow2 = npow2; Q.nt2 = nt2; Q.fsol_r = r_fsol; Q.pstatus = pst; Q.spec = spec_stats;
    Q.w = geo.w; Q.lw = geo.lw; Q.S = geo.S;
    const size_t spec_lds = geo.lds;
    for (int64_t v0 = 0; v0 < nvox; v0 += vpc) {
        const int64_t nv = std::min(vpc, nvox - v0), rows = nv * n_rep;
        G.nv = nv; G.v0 = v0;
        hipLaunchKernelGGL(bootstrap_gen_kernel, dim3(gen_grid(rows * nte)), dim3(256), 0, s, G);
        HIPCHK(hipGetLastError());
        // the rows' flip angles, as met2_fa_bruteforce / the spline method treat a row; the walks keep their scratch with their plans, sized by
        // the first (largest) chunk.  A row of a voxel without a point fit is masked out and keeps index 0
        if (fa_mode == MET2_BOOT_FA_BRUTEFORCE) {
            rc = met2_fa_bruteforce_strided(plan, rows, r_data, nte, 1, r_mask, r_fa, nullptr, nullptr, stream);
            if (rc) return rc;
        } else if (fa_mode == MET2_BOOT_FA_SPLINE) {
            rc = met2_fa_bruteforce_strided(plan_lr, rows, r_data, nte, 1, r_mask, r_fa, nullptr, r_res, stream);
            if (rc) return rc;
            rc = met2_fa_spline_select_strided(dev, rows, n_lr, alpha_lr.data(), r_res, (int32_t)alpha_hr.size(), alpha_hr.data(), nte, r_data, nte, 1,
                                               r_mask, r_fa, nullptr, stream);
            if (rc) return rc;
        }
        rc = met2_fit_enqueue_strided(plan, method, rows, r_data, nte, 1, r_fa, r_mask, r_fsol, nullptr, r_reg, nullptr, r_maps, r_st, stream);
        if (rc) return rc;
        S.v0 = v0; S.rows = rows;
        hipLaunchKernelGGL(bootstrap_stats_kernel, dim3((unsigned)nv), dim3(64), 0, s, S);
        HIPCHK(hipGetLastError());
        if (spec_stats) {
            Q.v0 = v0;
            hipLaunchKernelGGL(bootstrap_spec_stats_kernel<MET2_BOOT_SPEC_SKIP_EQUAL>, dim3((unsigned)nv), dim3(64 * MET2_SPEC_WAVES), spec_lds, s, Q);
            HIPCHK(hipGetLastError());
        }
    }
    return met2_plan_finish(plan, stream);
}

}  // namespace

extern "C" int met2_fit_bootstrap(met2_plan *plan, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                                  const double *fa_index, const uint8_t *mask, const int64_t *voxel_id, const double *sigma, int32_t n_rep,
                                  int64_t seed, double *fsol, double *sig, double *reg, double *lam, double *maps, int32_t *status,
                                  double *sigma_out, double *stats, int32_t *rep_status, void *stream)
{
    return boot_impl(plan, method, MET2_BOOT_FA_FIXED, MET2_BOOT_QUANT, nvox, data, voxel_stride, echo_stride, fa_index, mask, voxel_id, sigma, n_rep,
                     seed, fsol, sig, reg, lam, maps, status, sigma_out, stats, nullptr, rep_status, stream);
}

extern "C" int met2_fit_bootstrap_fa(met2_plan *plan, int32_t method, int32_t fa_mode, int64_t nvox, const double *data, int64_t voxel_stride,
                                     int64_t echo_stride, const double *fa_index, const uint8_t *mask, const int64_t *voxel_id, const double *sigma,
                                     int32_t n_rep, int64_t seed, double *fsol, double *sig, double *reg, double *lam, double *maps, int32_t *status,
                                     double *sigma_out, double *stats, double *spec_stats, int32_t *rep_status, void *stream)
{
    return boot_impl(plan, method, fa_mode, MET2_BOOT_QUANT_FA, nvox, data, voxel_stride, echo_stride, fa_index, mask, voxel_id, sigma, n_rep, seed,
                     fsol, sig, reg, lam, maps, status, sigma_out, stats, spec_stats, rep_status, stream);
}

namespace {

// status = NULL of the two entries below: every series counts.  The kernels read a status per voxel, so the call makes one, waits for the
// stream behind its launch and frees it.
struct AllFitted {
    int32_t *p = nullptr;
    ~AllFitted() { if (p) (void)hipFree(p); }
    int make(int64_t nvox, hipStream_t s)
    {
        HIPCHK(hipMalloc(&p, sizeof(int32_t) * (size_t)nvox));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)p, MET2_ST_FITTED, (size_t)nvox, s));
        return MET2_OK;
    }
};

int stats_entry_checks(int64_t nvox, int32_t n_rep)
{
    if (n_rep < 2 || n_rep > MET2_BOOT_MAX_REP) return fail(MET2_E_INVALID, "n_rep must lie in [2, 1024]");
    if (nvox < 0 || nvox > 0x7fffffff) return fail(MET2_E_INVALID, "nvox out of range");
    return MET2_OK;
}

}  // namespace

extern "C" int met2_bootstrap_series_stats(int32_t device, int64_t nvox, int32_t n_rep, int32_t n_quant, const double *values,
                                           const int32_t *status, double *stats, void *stream)
{
    int rc = stats_entry_checks(nvox, n_rep);
    if (rc) return rc;
    if (n_quant < 1 || n_quant > MET2_BOOT_QUANT_FA) return fail(MET2_E_INVALID, "n_quant must lie in [1, 8]");
    if (nvox == 0) return MET2_OK;
    if (!values || !stats) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    hipStream_t s = (hipStream_t)stream;
    AllFitted all;
    if (!status) { rc = all.make(nvox, s); if (rc) return rc; }
    const int64_t rows = nvox * n_rep;
    StatArgs S;
    S.v0 = 0; S.nvox = nvox; S.rows = rows; S.nrep = n_rep; S.npow2 = next_pow2(n_rep); S.nquant = n_quant;
    S.maps_r = values; S.reg_r = n_quant > 6 ? values + 6 * rows : nullptr; S.fa_r = n_quant > 7 ? values + 7 * rows : nullptr;
    S.st_r = nullptr; S.pstatus = status ? status : all.p; S.stats = stats; S.rep_status = nullptr;
    hipLaunchKernelGGL(bootstrap_stats_kernel, dim3((unsigned)nvox), dim3(64), 0, s, S);
    HIPCHK(hipGetLastError());
    if (all.p) HIPCHK(hipStreamSynchronize(s));
    return MET2_OK;
}

extern "C" int met2_bootstrap_spectrum_stats(int32_t device, int64_t nvox, int32_t n_rep, int32_t n_t2, const double *fsol_r,
                                             const int32_t *status, double *spec, void *stream)
{
    int rc = stats_entry_checks(nvox, n_rep);
    if (rc) return rc;
    if (n_t2 < 1 || n_t2 > 65536) return fail(MET2_E_INVALID, "n_t2 must lie in [1, 65536]");
    if (nvox == 0) return MET2_OK;
    if (!fsol_r || !spec) return fail(MET2_E_INVALID, "NULL argument");
    const SpecGeom geo = spec_geometry(n_rep);
    if (geo.lds > MET2_SPEC_LDS_MAX) return fail(MET2_E_UNSUPPORTED, "the tile of the spectrum statistics does not fit into LDS");
    USE_DEVICE(device);
    hipStream_t s = (hipStream_t)stream;
    AllFitted all;
    if (!status) { rc = all.make(nvox, s); if (rc) return rc; }
    SpecArgs Q;
    Q.v0 = 0; Q.nvox = nvox; Q.nrep = n_rep; Q.npow2 = geo.P; Q.nt2 = n_t2; Q.w = geo.w; Q.lw = geo.lw; Q.S = geo.S;
    Q.fsol_r = fsol_r; Q.pstatus = status ? status : all.p; Q.spec = spec;
    hipLaunchKernelGGL(bootstrap_spec_stats_kernel<MET2_BOOT_SPEC_SKIP_EQUAL>, dim3((unsigned)nvox), dim3(64 * MET2_SPEC_WAVES), geo.lds, s, Q);
    HIPCHK(hipGetLastError());
    if (all.p) HIPCHK(hipStreamSynchronize(s));
    return MET2_OK;
}

extern "C" int met2_bootstrap_spec_launch_info(int32_t n_rep, int32_t *tile_bins, int32_t *tile_stride, int64_t *lds_bytes)
{
    if (n_rep < 2 || n_rep > MET2_BOOT_MAX_REP) return fail(MET2_E_INVALID, "n_rep must lie in [2, 1024]");
    const SpecGeom geo = spec_geometry(n_rep);
    if (tile_bins) *tile_bins = geo.w;
    if (tile_stride) *tile_stride = geo.S;
    if (lds_bytes) *lds_bytes = (int64_t)geo.lds;
    return MET2_OK;
}
