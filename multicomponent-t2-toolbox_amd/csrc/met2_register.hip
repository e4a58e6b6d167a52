// met2_register.hip -- met2_register_index, met2_register_cost, met2_register_limits, met2_register_work_bytes: the similarity of a fixed and a
// moving volume under a whole batch of candidate affine transforms in one launch (include/met2_hip.h states the contract).  The optimiser that
// drives it lives in register.py; this file is its cost function.
//   met2_register_index  the fixed voxels grouped by bin (met2_label_index, the counting sort of the label statistics), and per bin the first
//                        of its runs: a run is RG_RUN consecutive members of ONE bin, the last run of a bin may be short
//   rg_runs_kernel       run_first[b] = sum over b' < b of ceil(n_b' / RG_RUN): one thread, at most 256 bins
//   rg_cost_kernel<KIND> one block per (run, candidate), one member per thread: the voxel's coordinates in the moving volume, the inside test
//                        and the trilinear sample through resample_taps.hpp (the bits met2_resample gives), then the run's sums by a fixed tree:
//                        __shfl_down over the 64 lanes of a wave, strides 32 .. 1, and the four waves as (w0 + w1) + (w2 + w3)
//   rg_final_kernel<KIND> one block per candidate: wave w takes the bins w, w + 4, ...; lane l adds the runs l, l + 64, ... of the bin in
//                        ascending order, the lanes go through the same wave tree; then the bins (slot b of 256, empty slots zero) through the
//                        block tree, and thread 0 forms the cost
//   rg_joint_kernel      met2_register_joint_cost (mutual information): the grid and the sampling of rg_cost_kernel; the run's samples are
//                        counted per moving bin in LDS (integer LDS atomics), and the counters that are not zero are added to row b of the
//                        candidate's table [n_bins][moving_bins] in `work` (integer global atomics: at most min(256, moving_bins) a block).
//                        Per-run histograms summed in a fixed order, as the other costs keep their sums, would take 4 moving_bins bytes per
//                        (run, candidate) -- 272 MB at 128 x 128 x 64, 64 bins and 256 candidates --; integer adds commute, so the table
//                        has the same value without that
//   rg_joint_final_kernel one block per candidate: the row and column sums of the table (integers, in LDS), the three sums of c log c in
//                        a fixed order (the header states it) and the cost
// No floating-point atomics and no dependence of a candidate's sums on K or on its place in the batch: candidate k reads A[k] and writes
// part[k] and nothing else.  The candidates of a run share its member list and the moving volume through the caches: at a pyramid level the
// moving volume is a few MiB at most, so the eight gathers per voxel are served by L2 and not by HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"

#pragma clang fp contract(off)

#include "resample_taps.hpp"

namespace {

#define RG_RUN MET2_REGISTER_RUN
#define RG_NP 5                            // doubles of a run's partial sums: the most any kind needs (normcorr)
static_assert(RG_RUN == 256, "a run is one block of four waves");

struct RgArgs {
    int nx, ny, nz;                        // moving
    int mx, my, mz;                        // fixed
    int n_bins, max_runs;
    const double *A;                       // [K][12]
    const int32_t *offset, *run_first, *order;
    const double *fixed, *moving;
    double cx, cy;                         // the shifts of the fixed and the moving values
    double tiny_x, tiny_y;                 // a sum of squares about the mean of n values counts as zero up to n times this
    double min_overlap;
    double *part;                          // [K][max_runs][RG_NP]
    int32_t *part_n;                       // [K][max_runs]
    int64_t *n_inside;                     // [K]
    double *cost;                          // [K]
};

__global__ void rg_runs_kernel(int n_bins, const int32_t *__restrict__ offset, int32_t *__restrict__ run_first)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int32_t acc = 0;
    for (int b = 0; b < n_bins; ++b) {
        run_first[b] = acc;
        acc += (offset[b + 1] - offset[b] + RG_RUN - 1) / RG_RUN;
    }
    run_first[n_bins] = acc;
}

// lane 0 of the wave gets slot l + slot (l + s) for s = 32, 16, .., 1
__device__ __forceinline__ double rg_wave_sum(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = rn_add(v, __shfl_down(v, s));
    return v;
}

__device__ __forceinline__ int rg_wave_sum(int v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s);
    return v;
}

// thread 0 gets the sum of the block's 256 slots: the wave tree, then (w0 + w1) + (w2 + w3).  lds holds 4 values; two barriers.
template <typename T>
__device__ __forceinline__ T rg_block_sum(T v, T *lds)
{
    v = rg_wave_sum(v);
    __syncthreads();                       // the last use of lds is over
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);   // integers, or doubles under contract(off): three roundings
}

template <int KIND>
struct RgKind {
    static constexpr int NP = KIND == MET2_REGISTER_CORRATIO ? 2 : KIND == MET2_REGISTER_NORMCORR ? 5 : 1;
};

template <int KIND>
__global__ void __launch_bounds__(RG_RUN) rg_cost_kernel(RgArgs P)
{
    constexpr int NP = RgKind<KIND>::NP;
    __shared__ double lds[NP][4];
    __shared__ int lds_n[4];
    const int r = blockIdx.x, k = blockIdx.y, n_bins = P.n_bins;
    if (r >= P.run_first[n_bins]) return;                          // the grid is sized by the upper bound ceil(nvox / RG_RUN) + n_bins
    int lo = 0, hi = n_bins;                                       // the bin b with run_first[b] <= r < run_first[b + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.run_first[mid] <= r) lo = mid; else hi = mid;
    }
    const int start = P.offset[lo] + (r - P.run_first[lo]) * RG_RUN;
    const int count = min(RG_RUN, P.offset[lo + 1] - start);
    const int t = threadIdx.x;
    double s[NP];
#pragma unroll
    for (int e = 0; e < NP; ++e) s[e] = 0.0;
    int n = 0;
    if (t < count) {
        RsGeom G;
        G.nx = P.nx; G.ny = P.ny; G.nz = P.nz;
        G.mx = P.mx; G.my = P.my; G.mz = P.mz;
#pragma unroll
        for (int e = 0; e < 12; ++e) G.A[e] = P.A[(size_t)k * 12 + e];
        const int v = P.order[start + t];
        const int kz = v % G.mz, rest = v / G.mz;
        RsTaps<1> T;
        if (rs_taps<1>(G, rest / G.my, rest % G.my, kz, T)) {
            const double y = rs_value<1, double>(T, P.moving, 1);
            n = 1;
            if constexpr (KIND == MET2_REGISTER_CORRATIO) {
                const double d = rn_sub(y, P.cy);
                s[0] = d;
                s[1] = rn_mul(d, d);
            } else if constexpr (KIND == MET2_REGISTER_NORMCORR) {
                const double dx = rn_sub(P.fixed[v], P.cx), dy = rn_sub(y, P.cy);
                s[0] = dx;
                s[1] = dy;
                s[2] = rn_mul(dx, dx);
                s[3] = rn_mul(dy, dy);
                s[4] = rn_mul(dx, dy);
            } else {
                const double d = rn_sub(P.fixed[v], y);
                s[0] = rn_mul(d, d);
            }
        }
    }
    n = rg_wave_sum(n);
#pragma unroll
    for (int e = 0; e < NP; ++e) s[e] = rg_wave_sum(s[e]);
    if ((t & 63) == 0) {
        lds_n[t >> 6] = n;
#pragma unroll
        for (int e = 0; e < NP; ++e) lds[e][t >> 6] = s[e];
    }
    __syncthreads();
    if (t == 0) {
        const size_t slot = (size_t)k * P.max_runs + r;
        P.part_n[slot] = (lds_n[0] + lds_n[1]) + (lds_n[2] + lds_n[3]);
#pragma unroll
        for (int e = 0; e < NP; ++e) P.part[slot * RG_NP + e] = rn_add(rn_add(lds[e][0], lds[e][1]), rn_add(lds[e][2], lds[e][3]));
    }
}

// sum of squares about the mean times n: q - s s / n, not below zero
__device__ __forceinline__ double rg_central(double q, double s, double n) { return fmax(rn_sub(q, rn_mul(s, s) / n), 0.0); }

template <int KIND>
__global__ void __launch_bounds__(RG_RUN) rg_final_kernel(RgArgs P)
{
    constexpr int NP = RgKind<KIND>::NP;
    __shared__ double bin_s[NP][RG_RUN];
    __shared__ int bin_n[RG_RUN];
    __shared__ double lds[4];
    __shared__ int lds_n[4];
    const int k = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, n_bins = P.n_bins;
    const double *part = P.part + (size_t)k * P.max_runs * RG_NP;
    const int32_t *part_n = P.part_n + (size_t)k * P.max_runs;
    bin_n[t] = 0;
#pragma unroll
    for (int e = 0; e < NP; ++e) bin_s[e][t] = 0.0;
    __syncthreads();
    for (int b = wave; b < n_bins; b += 4) {
        const int r1 = P.run_first[b + 1];
        double s[NP];
#pragma unroll
        for (int e = 0; e < NP; ++e) s[e] = 0.0;
        int n = 0;
        for (int r = P.run_first[b] + lane; r < r1; r += 64) {
            n += part_n[r];
#pragma unroll
            for (int e = 0; e < NP; ++e) s[e] = rn_add(s[e], part[(size_t)r * RG_NP + e]);
        }
        n = rg_wave_sum(n);
#pragma unroll
        for (int e = 0; e < NP; ++e) s[e] = rg_wave_sum(s[e]);
        if (lane == 0) {
            bin_n[b] = n;
#pragma unroll
            for (int e = 0; e < NP; ++e) bin_s[e][b] = s[e];
        }
    }
    __syncthreads();
    const int nb = bin_n[t];
    const int n_in = rg_block_sum(nb, lds_n);
    double tot[NP];
#pragma unroll
    for (int e = 0; e < NP; ++e) tot[e] = rg_block_sum(bin_s[e][t], lds);
    double within = 0.0;                                           // corratio: sum over the bins of n_b Var_b(y)
    if constexpr (KIND == MET2_REGISTER_CORRATIO) within = rg_block_sum(nb > 0 ? rg_central(bin_s[1][t], bin_s[0][t], (double)nb) : 0.0, lds);
    if (t != 0) return;
    const double N = (double)n_in;
    const bool enough = n_in > 0 && !(N < rn_mul(P.min_overlap, (double)P.offset[n_bins]));
    double cost = KIND == MET2_REGISTER_LEASTSQ ? MET2_REGISTER_LEASTSQ_WORST : 1.0;
    if (enough) {
        if constexpr (KIND == MET2_REGISTER_CORRATIO) {
            const double all = rg_central(tot[1], tot[0], N);
            if (all > rn_mul(N, P.tiny_y)) cost = fmin(within / all, 1.0);
        } else if constexpr (KIND == MET2_REGISTER_NORMCORR) {
            const double vx = rg_central(tot[2], tot[0], N), vy = rg_central(tot[3], tot[1], N);
            const double cxy = rn_sub(tot[4], rn_mul(tot[0], tot[1]) / N);
            if (vx > rn_mul(N, P.tiny_x) && vy > rn_mul(N, P.tiny_y)) cost = fmax(rn_sub(1.0, fmin(rn_mul(cxy, cxy) / rn_mul(vx, vy), 1.0)), 0.0);
        } else {
            cost = tot[0] / N;
        }
    }
    P.n_inside[k] = n_in;
    P.cost[k] = cost;
}

// ---------------------------------------------------------------- the joint histogram and the mutual-information costs
struct RgJointArgs {
    int nx, ny, nz;                        // moving
    int mx, my, mz;                        // fixed
    int n_bins, moving_bins, kind;
    const double *A;                       // [K][12]
    const int32_t *offset, *run_first, *order;
    const double *moving;
    double lo, scale;                      // moving bin = floor((y - lo) scale), clamped
    double min_overlap, worst;
    int32_t *table;                        // [K][n_bins][moving_bins], zero before rg_joint_kernel
    int64_t *n_inside;                     // [K]
    double *cost;                          // [K]
};

// one block per (run, candidate), the grid of rg_cost_kernel: the run's samples go into moving_bins counters in LDS, the counters that are
// not zero into row b of the candidate's table.  Integer adds commute: the table does not depend on the order of arrival.
__global__ void __launch_bounds__(RG_RUN) rg_joint_kernel(RgJointArgs P)
{
    __shared__ int hist[MET2_REGISTER_MAX_BINS];
    const int r = blockIdx.x, k = blockIdx.y, n_bins = P.n_bins, mb = P.moving_bins;
    if (r >= P.run_first[n_bins]) return;                          // the whole block leaves: no barrier is missed
    int lo = 0, hi = n_bins;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.run_first[mid] <= r) lo = mid; else hi = mid;
    }
    const int start = P.offset[lo] + (r - P.run_first[lo]) * RG_RUN;
    const int count = min(RG_RUN, P.offset[lo + 1] - start);
    const int t = threadIdx.x;
    hist[t] = 0;
    __syncthreads();
    if (t < count) {
        RsGeom G;
        G.nx = P.nx; G.ny = P.ny; G.nz = P.nz;
        G.mx = P.mx; G.my = P.my; G.mz = P.mz;
#pragma unroll
        for (int e = 0; e < 12; ++e) G.A[e] = P.A[(size_t)k * 12 + e];
        const int v = P.order[start + t];
        const int kz = v % G.mz, rest = v / G.mz;
        RsTaps<1> T;
        if (rs_taps<1>(G, rest / G.my, rest % G.my, kz, T)) {
            const double y = rs_value<1, double>(T, P.moving, 1);
            const double s = floor(rn_mul(rn_sub(y, P.lo), P.scale));
            const int j = (int)fmin(fmax(s, 0.0), (double)(mb - 1));       // clamped as a double: j lies in 0 .. mb - 1 whatever the range given
            atomicAdd(&hist[j], 1);
        }
    }
    __syncthreads();
    if (t < mb && hist[t] > 0) atomicAdd(P.table + ((size_t)k * n_bins + lo) * mb + t, hist[t]);
}

__device__ __forceinline__ double rg_clogc(int c) { return c > 0 ? rn_mul((double)c, log((double)c)) : 0.0; }

// one block per candidate: thread t takes the cells t, t + 256, ... of the table [n_bins moving_bins] in ascending order -- T(n_bj) added as
// it goes, the counts into the row and the column sums in LDS (integers) --, then the three sums of T through the block tree: the cells'
// chains, the rows as slot b of 256, the columns as slot j of 256
__global__ void __launch_bounds__(RG_RUN) rg_joint_final_kernel(RgJointArgs P)
{
    __shared__ int row[MET2_REGISTER_MAX_BINS], col[MET2_REGISTER_MAX_BINS];
    __shared__ double lds[4];
    __shared__ int lds_n[4];
    const int k = blockIdx.x, t = threadIdx.x, n_bins = P.n_bins, mb = P.moving_bins, cells = n_bins * mb;
    const int32_t *table = P.table + (size_t)k * cells;
    row[t] = 0;
    col[t] = 0;
    __syncthreads();
    double t_cell = 0.0;
    for (int c = t; c < cells; c += RG_RUN) {
        const int n = table[c];
        if (n > 0) {
            t_cell = rn_add(t_cell, rg_clogc(n));
            atomicAdd(&row[c / mb], n);
            atomicAdd(&col[c % mb], n);
        }
    }
    __syncthreads();
    const int nb = row[t], mj = col[t];
    const int n_in = rg_block_sum(nb, lds_n);
    const int single = rg_block_sum((int)(n_in > 0 && (nb == n_in || mj == n_in)), lds_n);    // every voxel in one fixed bin, or in one moving bin
    const double txy = rg_block_sum(t_cell, lds), tx = rg_block_sum(rg_clogc(nb), lds), ty = rg_block_sum(rg_clogc(mj), lds);
    if (t != 0) return;
    const double N = (double)n_in;
    double cost = P.worst;
    if (n_in > 0 && !(N < rn_mul(P.min_overlap, (double)P.offset[n_bins])) && single == 0) {
        const double logn = log(N);
        const double hx = rn_sub(logn, tx / N), hy = rn_sub(logn, ty / N), hxy = rn_sub(logn, txy / N);
        if (P.kind == MET2_REGISTER_MI) cost = fmin(-rn_sub(rn_add(hx, hy), hxy), 0.0);
        else cost = fmin(-(rn_add(hx, hy) / hxy), -1.0);
    }
    P.n_inside[k] = n_in;
    P.cost[k] = cost;
}

int rg_check_dims(const int32_t *d, const char *what)
{
    if (!d) return fail(MET2_E_INVALID, std::string("NULL ") + what + " dims");
    for (int a = 0; a < 3; ++a) {
        if (d[a] < 1) return fail(MET2_E_INVALID, std::string("every ") + what + " axis needs at least one voxel");
        if (d[a] > MET2_REGISTER_MAX_AXIS) return fail(MET2_E_UNSUPPORTED, std::string("a ") + what + " axis holds more than 512 voxels");
    }
    return MET2_OK;
}

int rg_check_counts(int32_t n_bins, int32_t K)
{
    if (n_bins < 1 || K < 1) return fail(MET2_E_INVALID, "n_bins and K must be positive");
    if (n_bins > MET2_REGISTER_MAX_BINS) return fail(MET2_E_UNSUPPORTED, "more than 256 bins");
    if (K > MET2_REGISTER_MAX_K) return fail(MET2_E_UNSUPPORTED, "more than 256 candidates in a batch");
    return MET2_OK;
}

int rg_check_range(const double *r, const char *what)
{
    if (!r) return fail(MET2_E_INVALID, std::string("NULL ") + what + " range");
    if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || r[0] > r[1]) return fail(MET2_E_INVALID, std::string("the ") + what + " range must be finite, lo <= hi");
    return MET2_OK;
}

int64_t rg_nvox(const int32_t *d) { return (int64_t)d[0] * d[1] * d[2]; }
int64_t rg_max_runs(const int32_t *d, int n_bins) { return (rg_nvox(d) + RG_RUN - 1) / RG_RUN + n_bins; }
int64_t rg_index_bytes(const int32_t *d, int n_bins) { return 4 * (2 * ((int64_t)n_bins + 1) + rg_nvox(d)); }
int64_t rg_part_offset(int K) { return (int64_t)K * 12 * 8; }
int64_t rg_cost_bytes(const int32_t *d, int n_bins, int K) { return rg_part_offset(K) + (int64_t)K * rg_max_runs(d, n_bins) * (RG_NP * 8 + 4); }

template <int KIND>
hipError_t rg_launch(const RgArgs &P, int K, hipStream_t st)
{
    hipLaunchKernelGGL(rg_cost_kernel<KIND>, dim3((unsigned)P.max_runs, (unsigned)K), dim3(RG_RUN), 0, st, P);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(rg_final_kernel<KIND>, dim3((unsigned)K), dim3(RG_RUN), 0, st, P);
    return hipGetLastError();
}

}  // namespace

extern "C" int met2_register_limits(int32_t *run, int32_t *max_axis, int32_t *max_bins, int32_t *max_k, double *leastsq_worst)
{
    if (run) *run = MET2_REGISTER_RUN;
    if (max_axis) *max_axis = MET2_REGISTER_MAX_AXIS;
    if (max_bins) *max_bins = MET2_REGISTER_MAX_BINS;
    if (max_k) *max_k = MET2_REGISTER_MAX_K;
    if (leastsq_worst) *leastsq_worst = MET2_REGISTER_LEASTSQ_WORST;
    return MET2_OK;
}

extern "C" int met2_register_work_bytes(const int32_t fixed_dims[3], int32_t n_bins, int32_t K, int64_t *index_bytes, int64_t *cost_bytes)
{
    int rc;
    if ((rc = rg_check_dims(fixed_dims, "fixed")) || (rc = rg_check_counts(n_bins, K))) return rc;
    if (index_bytes) *index_bytes = rg_index_bytes(fixed_dims, n_bins);
    if (cost_bytes) *cost_bytes = rg_cost_bytes(fixed_dims, n_bins, K);
    return MET2_OK;
}

extern "C" int met2_register_index(int32_t device, const int32_t fixed_dims[3], const int32_t *fixed_bin, int32_t n_bins, void *index,
                                   int64_t index_bytes, void *stream)
{
    int rc;
    if ((rc = rg_check_dims(fixed_dims, "fixed")) || (rc = rg_check_counts(n_bins, 1))) return rc;
    if (!fixed_bin || !index) return fail(MET2_E_INVALID, "NULL argument");
    if (index_bytes < rg_index_bytes(fixed_dims, n_bins))
        return fail(MET2_E_INVALID, "the index needs " + std::to_string(rg_index_bytes(fixed_dims, n_bins)) + " bytes");
    int32_t *offset = (int32_t *)index, *run_first = offset + n_bins + 1, *order = run_first + n_bins + 1;
    if ((rc = met2_label_index(device, rg_nvox(fixed_dims), fixed_bin, n_bins, offset, order, stream))) return rc;
    USE_DEVICE(device);
    hipLaunchKernelGGL(rg_runs_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, n_bins, offset, run_first);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_register_cost(int32_t device, int32_t kind, const int32_t fixed_dims[3], int32_t n_bins, const void *index, const double *fixed,
                                  const double fixed_range[2], const int32_t moving_dims[3], const double *moving, const double moving_range[2],
                                  int32_t K, const double *A, double min_overlap, void *work, int64_t work_bytes, int64_t *n_inside, double *cost,
                                  void *stream)
{
    int rc;
    if (kind != MET2_REGISTER_CORRATIO && kind != MET2_REGISTER_NORMCORR && kind != MET2_REGISTER_LEASTSQ)
        return fail(MET2_E_INVALID, "kind must be MET2_REGISTER_CORRATIO, _NORMCORR or _LEASTSQ");
    if ((rc = rg_check_dims(fixed_dims, "fixed")) || (rc = rg_check_dims(moving_dims, "moving")) || (rc = rg_check_counts(n_bins, K))) return rc;
    if (!index || !moving || !A || !work || !n_inside || !cost) return fail(MET2_E_INVALID, "NULL argument");
    if (kind != MET2_REGISTER_CORRATIO && !fixed) return fail(MET2_E_INVALID, "normcorr and leastsq need the fixed values");
    if ((rc = rg_check_range(moving_range, "moving"))) return rc;
    if (kind == MET2_REGISTER_NORMCORR && (rc = rg_check_range(fixed_range, "fixed"))) return rc;
    for (int64_t e = 0; e < (int64_t)K * 12; ++e)
        if (!std::isfinite(A[e])) return fail(MET2_E_INVALID, "every entry of every transform must be finite");
    if (!(min_overlap >= 0.0 && min_overlap <= 1.0)) return fail(MET2_E_INVALID, "min_overlap must lie in [0, 1]");
    if (work_bytes < rg_cost_bytes(fixed_dims, n_bins, K))
        return fail(MET2_E_INVALID, "the work space needs " + std::to_string(rg_cost_bytes(fixed_dims, n_bins, K)) + " bytes");
    if (((uintptr_t)work & 7) || ((uintptr_t)index & 3)) return fail(MET2_E_INVALID, "work must be aligned to 8 bytes and index to 4");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    RgArgs P;
    P.nx = moving_dims[0]; P.ny = moving_dims[1]; P.nz = moving_dims[2];
    P.mx = fixed_dims[0]; P.my = fixed_dims[1]; P.mz = fixed_dims[2];
    P.n_bins = n_bins;
    P.max_runs = (int)rg_max_runs(fixed_dims, n_bins);
    P.A = (const double *)work;
    P.offset = (const int32_t *)index;
    P.run_first = P.offset + n_bins + 1;
    P.order = P.run_first + n_bins + 1;
    P.fixed = fixed;
    P.moving = moving;
    const auto mid = [](const double *r) { return r[0] + (r[1] - r[0]) / 2.0; };
    const auto tiny = [](const double *r) { const double m = std::max(std::fabs(r[0]), std::fabs(r[1])); return 1e-24 * m * m; };
    P.cy = mid(moving_range);
    P.tiny_y = tiny(moving_range);
    P.cx = kind == MET2_REGISTER_NORMCORR ? mid(fixed_range) : 0.0;
    P.tiny_x = kind == MET2_REGISTER_NORMCORR ? tiny(fixed_range) : 0.0;
    P.min_overlap = min_overlap;
    P.part = (double *)((char *)work + rg_part_offset(K));
    P.part_n = (int32_t *)(P.part + (size_t)K * P.max_runs * RG_NP);
    P.n_inside = n_inside;
    P.cost = cost;
    HIPCHK(hipMemcpyAsync(work, A, (size_t)K * 12 * sizeof(double), hipMemcpyHostToDevice, st));       // A lives until the stream has run it: the header says so
    if (kind == MET2_REGISTER_CORRATIO) HIPCHK(rg_launch<MET2_REGISTER_CORRATIO>(P, K, st));
    if (kind == MET2_REGISTER_NORMCORR) HIPCHK(rg_launch<MET2_REGISTER_NORMCORR>(P, K, st));
    if (kind == MET2_REGISTER_LEASTSQ) HIPCHK(rg_launch<MET2_REGISTER_LEASTSQ>(P, K, st));
    return MET2_OK;
}

namespace {

int rg_check_joint_counts(int32_t n_bins, int32_t moving_bins, int32_t K)
{
    int rc;
    if ((rc = rg_check_counts(n_bins, K))) return rc;
    if (moving_bins < 1) return fail(MET2_E_INVALID, "moving_bins must be positive");
    if (moving_bins > MET2_REGISTER_MAX_BINS) return fail(MET2_E_UNSUPPORTED, "more than 256 moving bins");
    return MET2_OK;
}

int64_t rg_joint_bytes(int n_bins, int moving_bins, int K) { return rg_part_offset(K) + (int64_t)K * n_bins * moving_bins * 4; }

}  // namespace

extern "C" int met2_register_joint_work_bytes(const int32_t fixed_dims[3], int32_t n_bins, int32_t moving_bins, int32_t K, int64_t *work_bytes)
{
    int rc;
    if ((rc = rg_check_dims(fixed_dims, "fixed")) || (rc = rg_check_joint_counts(n_bins, moving_bins, K))) return rc;
    if (work_bytes) *work_bytes = rg_joint_bytes(n_bins, moving_bins, K);
    return MET2_OK;
}

extern "C" int met2_register_joint_cost(int32_t device, int32_t kind, const int32_t fixed_dims[3], int32_t n_bins, const void *index,
                                        const int32_t moving_dims[3], const double *moving, const double moving_range[2], int32_t moving_bins,
                                        int32_t K, const double *A, double min_overlap, void *work, int64_t work_bytes, int64_t *n_inside,
                                        double *cost, int32_t *joint, void *stream)
{
    int rc;
    if (kind != MET2_REGISTER_MI && kind != MET2_REGISTER_NMI) return fail(MET2_E_INVALID, "kind must be MET2_REGISTER_MI or MET2_REGISTER_NMI");
    if ((rc = rg_check_dims(fixed_dims, "fixed")) || (rc = rg_check_dims(moving_dims, "moving")) || (rc = rg_check_joint_counts(n_bins, moving_bins, K)))
        return rc;
    if (!index || !moving || !A || !work || !n_inside || !cost) return fail(MET2_E_INVALID, "NULL argument");
    if ((rc = rg_check_range(moving_range, "moving"))) return rc;
    for (int64_t e = 0; e < (int64_t)K * 12; ++e)
        if (!std::isfinite(A[e])) return fail(MET2_E_INVALID, "every entry of every transform must be finite");
    if (!(min_overlap >= 0.0 && min_overlap <= 1.0)) return fail(MET2_E_INVALID, "min_overlap must lie in [0, 1]");
    if (work_bytes < rg_joint_bytes(n_bins, moving_bins, K))
        return fail(MET2_E_INVALID, "the work space needs " + std::to_string(rg_joint_bytes(n_bins, moving_bins, K)) + " bytes");
    if (((uintptr_t)work & 7) || ((uintptr_t)index & 3) || ((uintptr_t)joint & 3))
        return fail(MET2_E_INVALID, "work must be aligned to 8 bytes, index and joint to 4");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    RgJointArgs P;
    P.nx = moving_dims[0]; P.ny = moving_dims[1]; P.nz = moving_dims[2];
    P.mx = fixed_dims[0]; P.my = fixed_dims[1]; P.mz = fixed_dims[2];
    P.n_bins = n_bins;
    P.moving_bins = moving_bins;
    P.kind = kind;
    P.A = (const double *)work;
    P.offset = (const int32_t *)index;
    P.run_first = P.offset + n_bins + 1;
    P.order = P.run_first + n_bins + 1;
    P.moving = moving;
    P.lo = moving_range[0];
    P.scale = moving_range[1] > moving_range[0] ? (double)moving_bins / (moving_range[1] - moving_range[0]) : 0.0;
    if (!std::isfinite(P.scale)) P.scale = 0.0;                    // a range so narrow that the quotient overflows counts as hi = lo
    P.min_overlap = min_overlap;
    P.worst = kind == MET2_REGISTER_MI ? MET2_REGISTER_MI_WORST : MET2_REGISTER_NMI_WORST;
    P.table = (int32_t *)((char *)work + rg_part_offset(K));
    P.n_inside = n_inside;
    P.cost = cost;
    const size_t table_bytes = (size_t)K * n_bins * moving_bins * 4;
    HIPCHK(hipMemcpyAsync(work, A, (size_t)K * 12 * sizeof(double), hipMemcpyHostToDevice, st));       // A lives until the stream has run it: the header says so
    HIPCHK(hipMemsetAsync(P.table, 0, table_bytes, st));           // in every call: the table of the call before is gone
    hipLaunchKernelGGL(rg_joint_kernel, dim3((unsigned)rg_max_runs(fixed_dims, n_bins), (unsigned)K), dim3(RG_RUN), 0, st, P);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(rg_joint_final_kernel, dim3((unsigned)K), dim3(RG_RUN), 0, st, P);
    HIPCHK(hipGetLastError());
    if (joint) HIPCHK(hipMemcpyAsync(joint, P.table, table_bytes, hipMemcpyDeviceToDevice, st));
    return MET2_OK;
}
