// met2_hip.hip -- the core of libmet2_hip.so: the plan, the sort, the fit and the brute-force flip-angle walk.
//
// Host code
//   error plumbing (met2_last_error), options, the plan's lifecycle (struct met2_plan itself: plan.hpp), the lambda grid
//   fit_geometry, fast_kmax, kernel_method, launch_*: the geometry and the instance of a fit launch
//   ensure_seeds            the plan-level seeds and BayesReg factor tables (seed_kernel, bayes_table_kernel: fit_kernel.hpp)
//   fit_impl                met2_fit / met2_fit_strided / met2_fit_enqueue_strided, met2_plan_finish
//   met2_fa_bruteforce[_strided], the timing and launch-info getters
// Kernels
//   reset_sort / classify / scan / scatter   gates of motor:124,131 + counting sort of voxels by FA index, so that
//                           neighbouring entries of the work list read the same D / B rows from L2
//   fit_kernel<METHOD>      (fit_kernel.hpp) motor:113-162 + motor:443-472: one voxel per wavefront; every wave of the
//                           persistent workgroups pulls its own voxels from per-XCD queue cursors over
//                           the FA-sorted list; D, D^T, B and K rows are read through L1/L2
//   finalize_unfitted       zeros / all-zero-spectrum metrics for gated-out voxels
//   fa_project_kernel, fa_kernel   fa_estimation.py:74-111: brute force over the plan's flip angles
// The walk lives here because it shares fit_geometry and the sort buffers with the fit, needs the solver headers, and in
// -DMET2_CYCSTATS builds reads the counters the fit writes (one copy per translation unit).
// The dictionary and the penalty: met2_dictionary.hip.  NESMA, the smoother, the FA spline selection: met2_prefilter.hip.
// The ROI reduction and the stand-alone metrics: met2_roi_metrics.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "plan.hpp"
#include "nnls_wave.hpp"
#include "objectives.hpp"
#include "fit_kernel.hpp"

using namespace met2;

#ifdef MET2_SPLIT_TU
// the fit kernels are instantiated in met2_fit_*.hip (fit_kernel.hpp)
extern template int launch_fit_nb<0, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<0, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<1, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<1, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<2, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<2, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<3, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<3, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<4, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<4, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<5, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<5, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<6, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<6, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<12, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<12, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<14, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<14, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<15, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<15, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<16, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<16, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<0, 1, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<0, 2, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<1, 1, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<1, 2, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<2, 1, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<2, 2, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<3, 1, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<3, 2, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<4, 1, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<4, 2, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<5, 1, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<5, 2, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<6, 1, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
extern template int launch_fit_nb<6, 2, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
#endif

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;
int met2::abi_fail(int code, const std::string &msg) { g_err = msg; return code; }

// ------------------------------------------------------------------------------------------
// voxel classification and counting sort by FA index
// ------------------------------------------------------------------------------------------

// counters and cursors of a fit start at zero: ONE launch instead of two or three fills (a fit over a block of a host pipeline starts while the previous
// block's download bursts, and every tiny launch then waits its turn: three fills stood 1.8 ms in a 5 ms gap between two blocks' solver kernels).
// keep_err: the error word keeps what earlier ENQUEUED fits may have set.
__global__ __launch_bounds__(256) void reset_sort_kernel(SortBufs sb, int nfa, int keep_err)
{
    const int e = 4 * (nfa + 1) + 1;                                  // index of the error word behind hist | cursor | bucket_start | chunk_start | queue
    for (int i = threadIdx.x; i < e + 15; i += blockDim.x)
        if (i != e || !keep_err) sb.hist[i] = 0;
}

#define MET2_SORT_BLOCK 1024
// The histogram and the cursors take ONE global atomic per (workgroup, flip angle): a wave adds its counts to a table in LDS first.  With one atomic
// per wave a single-angle fit sent 3 600 atomics per 230 000 voxels to one address -- 0.33 ms of classify and 0.75 ms of scatter were that queue.
__global__ __launch_bounds__(MET2_SORT_BLOCK) void classify_kernel(int64_t nvox, int nte, int nfa, const double *__restrict__ data,
                                                       int64_t vs, int64_t es,      // element strides of data: voxel, echo
                                                       const double *__restrict__ fa_index, const uint8_t *__restrict__ mask,
                                                       int require_first_echo, SortBufs sb, int32_t *__restrict__ status)
{
    extern __shared__ int sort_lds[];                                 // [nfa] counts of this workgroup
    const int lane = lane_id();
    for (int i = threadIdx.x; i < nfa; i += blockDim.x) sort_lds[i] = 0;
    __syncthreads();
    int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int key = -1, st = 0;
    if (v < nvox) {
        const double *M = data + v * vs;
        double sum = 0.0; bool finite = true;
        for (int e = 0; e < nte; ++e) { double t = M[e * es]; sum += t; finite = finite && isfinite(t); }
        bool mk = mask ? (mask[v] != 0) : true;
        if (!finite) st = MET2_ST_NONFINITE;
        else if (mk && sum > 0.0 && (!require_first_echo || M[0] > 0.0)) {
            int fi = fa_index ? (int)fa_index[v] : 0;
            if (fi < 0 || fi >= nfa) atomicOr(sb.err, 1);
            else { key = fi; st = MET2_ST_FITTED; }
        }
        sb.key[v] = key;
        if (status) status[v] = st;
    }
    // wave-aggregated histogram, into the workgroup's table
    u64 todo = ballot(key >= 0);
    while (todo) {
        int leader = first_lane(todo);
        int k0 = bcast_i(key, leader);
        u64 same = ballot(key == k0) & todo;
        if (lane == leader) atomicAdd(&sort_lds[k0], __popcll(same));
        todo &= ~same;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nfa; i += blockDim.x) { const int c = sort_lds[i]; if (c) atomicAdd(&sb.hist[i], c); }
}

// bucket and chunk offsets from the histogram.  The histogram comes in and the offsets go out in parallel; the running sums are taken over LDS (one
// thread walking 273 counters in global memory stood 0.13 ms per launch, two launches per fit).
__global__ __launch_bounds__(256) void scan_kernel(int nfa, int chunk, SortBufs sb)
{
    extern __shared__ int sort_lds[];                                 // [nfa + 1] bucket starts, [nfa + 1] chunk starts
    int *bs = sort_lds, *cs = sort_lds + nfa + 1;
    for (int f = threadIdx.x; f < nfa; f += blockDim.x) { const int c = sb.hist[f]; bs[f] = c; cs[f] = (c + chunk - 1) / chunk; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0, cacc = 0;
        for (int f = 0; f < nfa; ++f) { const int c = bs[f], cc = cs[f]; bs[f] = acc; cs[f] = cacc; acc += c; cacc += cc; }
        bs[nfa] = acc; cs[nfa] = cacc;
        sb.queue[0] = 0;
    }
    __syncthreads();
    for (int f = threadIdx.x; f <= nfa; f += blockDim.x) {
        sb.bucket_start[f] = bs[f]; sb.chunk_start[f] = cs[f];
        if (f < nfa) sb.cursor[f] = 0;
    }
}

__global__ __launch_bounds__(MET2_SORT_BLOCK) void scatter_kernel(int64_t nvox, int nfa, SortBufs sb)
{
    extern __shared__ int sort_lds[];                                 // [nfa] counts of this workgroup, then [nfa] its base in every bucket
    const int lane = lane_id();
    for (int i = threadIdx.x; i < nfa; i += blockDim.x) sort_lds[i] = 0;
    __syncthreads();
    int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int key = (v < nvox) ? sb.key[v] : -1;
    int off = 0;                                                      // this voxel's place among the workgroup's voxels of its flip angle
    u64 todo = ballot(key >= 0);
    while (todo) {
        int leader = first_lane(todo);
        int k0 = bcast_i(key, leader);
        u64 same = ballot(key == k0) & todo;
        int base = 0;
        if (lane == leader) base = atomicAdd(&sort_lds[k0], __popcll(same));
        base = bcast_i(base, leader);
        if (key == k0) off = base + __popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nfa; i += blockDim.x) { const int c = sort_lds[i]; if (c) sort_lds[nfa + i] = atomicAdd(&sb.cursor[i], c); }
    __syncthreads();
    if (key >= 0) sb.perm[sb.bucket_start[key] + sort_lds[nfa + key] + off] = (int)v;
}

// ------------------------------------------------------------------------------------------
// brute-force flip-angle estimation (flip_angle_algorithms/fa_estimation.py:74-111):
// for every flip angle of the dictionary one plain NNLS per voxel, argmin of the residual norm.
// Every wave keeps VPW voxels in registers and walks the FA axis on its own.
// ------------------------------------------------------------------------------------------
struct FaArgs {
    int n, m, nfa, kmax, waves, wave_doubles;
    const double *Dfa, *Bfa, *Dtfa;
    const double *Kd;         // [n][n], only multiplied by lambda = 0 here (the refactorisation reads its rows)
    const double *data;       // echo e of voxel v at data[v * vs + e * es]
    int64_t vs, es;
    const uint8_t *mask;
    double *fa_index, *km, *resid;
    int *queue;
    int64_t nvox;
    const double *Hq;         // [nvox of this pass][nfa * 16]: c_fa = Q_fa^T b in every flip angle's low-rank basis (fa_project_kernel on the stacked bases), or NULL: no pruning.
    double *Lb;               // [nvox of this pass][nfa]: the walk parks every angle's lower bound here (a voxel's row belongs to the one wave that walks it)
    const double *Aq;         // [nfa][n][16]: (Q_fa^T D_fa)^T -- with Hq, the walk forms h_fa = A_fa^T c_fa = D_fa^T (Q Q^T b) from it (round 5: no H then)
    const double *H;          // [nvox of this pass][nfa * n]: h = D_fa^T b of every flip angle (fa_project_kernel), or NULL: formed in the walk
    int64_t v0;               // first voxel of this pass (H row 0), voxels [v0, v0 + nvox_pass)
    int64_t v_end;            // one past the last voxel of this pass
};

// ------------------------------------------------------------------------------------------
// The batched contraction of the brute-force FA step on the matrix cores: every NNLS of fa_estimation.py:78-82 starts from
// h_fa = D_fa^T b, 91 dictionaries per voxel.  As ONE GEMM per pass of voxels,  H[v][fa * n + bin] = sum_e data[v][e] D^T[fa][bin][e]
// ([T x m] . [m x nfa n]) with v_mfma_f64_16x16x4: a wave keeps the echoes of 32 voxels in registers (two 16-voxel operand sets),
// walks the nfa * n rows of the stacked D^T in tiles of 16 -- each tile's operand is loaded once from L2 and used for both voxel
// sets -- and writes the 16 x 16 results voxel-major, so that the walk reads its h as one contiguous row per flip angle.
// The walk without it re-derives h per (voxel pair, flip angle) on the vector unit from D rows streamed through L2 (half of the
// 2.8 MB per voxel the FA walk pulls through L2 at 48 x 120).
// KS = ceil(m / 4) k-steps of four echoes (operands past m are zero).
// ------------------------------------------------------------------------------------------
struct FaGemmArgs {
    int n, m, nfa;
    const double *Dtfa;       // [nfa * n][m]
    const double *data; int64_t vs, es;
    double *H;                // [T][nfa * n]
    int64_t v0, v_end;
};

template <int KS>
__global__ __launch_bounds__(256) void fa_project_kernel(FaGemmArgs A)
{
    const int lane = lane_id(), li = lane & 15, lk = lane >> 4;
    const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t vA = A.v0 + wv * 32;
    if (vA >= A.v_end) return;
    const int M = A.nfa * A.n, m = A.m;
    // A operands: voxel vA + li (and vA + 16 + li), echoes 4 q + lk
    double a0[KS], a1[KS];
#pragma unroll
    for (int q = 0; q < KS; ++q) {
        const int e = 4 * q + lk;
        const int64_t v0 = vA + li, v1 = vA + 16 + li;
        a0[q] = (e < m && v0 < A.v_end) ? A.data[v0 * A.vs + e * A.es] : 0.0;
        a1[q] = (e < m && v1 < A.v_end) ? A.data[v1 * A.vs + e * A.es] : 0.0;
    }
    double *Hrow0[4], *Hrow1[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        Hrow0[v] = A.H + (size_t)(vA - A.v0 + lk + 4 * v) * M;
        Hrow1[v] = A.H + (size_t)(vA - A.v0 + 16 + lk + 4 * v) * M;
    }
    for (int r0 = 0; r0 < M; r0 += 16) {
        const int r = min(r0 + li, M - 1);
        const double *drow = A.Dtfa + (size_t)r * m;
        double bop[KS];
#pragma unroll
        for (int q = 0; q < KS; ++q) { const int e = 4 * q + lk; bop[q] = (e < m) ? drow[min(e, m - 1)] : 0.0; }
        met2_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < KS; ++q) {
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[q], bop[q], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[q], bop[q], acc1, 0, 0, 0);
        }
        if (r0 + li < M) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (vA + lk + 4 * v < A.v_end) Hrow0[v][r0 + li] = acc0[v];
                if (vA + 16 + lk + 4 * v < A.v_end) Hrow1[v][r0 + li] = acc1[v];
            }
        }
    }
}

// PRUNE: the walk skips flip angles by their lower bounds (A.Hq); a separate instantiation keeps the exhaustive walk (all residuals wanted: the
// spline path; few flip angles) free of the masks and the extra round
template <int VPW, int NB, int WAVES, bool PRUNE>
__global__ __launch_bounds__(64 * WAVES) void fa_kernel(FaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int n = A.n, m = A.m;
    double *sR = smem + (size_t)wave * A.wave_doubles;
    WaveShared S;
    S.R = sR; S.n = n; S.m = m; S.kmax = A.kmax; S.rcap = A.wave_doubles; S.K = A.Kd; S.kband = nullptr; S.Dt = nullptr; S.DtG = A.Dtfa; S.dtstride = m; S.buffer_rows = false; S.reorder = false; S.have_bdiag = true; S.bdiag[0] = S.bdiag[1] = 0.0;
    S.B = A.Bfa; S.D = A.Dfa; S.bstride = n; S.dstride = n;
    Band<NB> bd;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int d = 0; d < 5; ++d) bd.lb[b][d] = 0.0;
    // every wave pulls its own VPW voxels and walks the flip angles alone, reading D, D^T and B through L1/L2 -- no barrier,
    // so no wave waits for the slowest solve of a tile (a tile kernel with D and B staged in LDS per flip angle spent 48 % of
    // its wave time in its two barriers per flip angle; removed in round 3).
    const int64_t ntiles = (A.v_end - A.v0 + VPW - 1) / VPW;     // this pass: voxels [A.v0, A.v_end)
    const int Mh = A.nfa * n;
    for (int64_t round = 0; round <= ntiles; ++round) {
        int t32 = 0;
        if (lane == 0) t32 = atomicAdd(A.queue, 1);
        const int64_t tile = __builtin_amdgcn_readfirstlane(t32);
        if (tile >= ntiles) break;
        const int64_t v0 = A.v0 + tile * VPW;
        double b[VPW], best_r[VPW], best_km[VPW];
        int best_fa[VPW];
        bool act[VPW];
        // the passive set and x of a voxel carry over from one flip angle to the next (neighbouring dictionaries give
        // nearly the same support): each solve is a warm start -- re-factorise, secondary loop, dual check -- instead
        // of rebuilding the support bin by bin.  NNLS has one minimiser, so only the rounding differs from a cold start.
        NnlsState<NB> st[VPW];
#pragma unroll
        for (int vv = 0; vv < VPW; ++vv) {
            st[vv].itmax_hit = 0;
            MET2_CYC_INIT(st[vv]);
            nnls_reset<NB>(st[vv]);
            const int64_t v = v0 + vv;
            const bool in = v < A.v_end;
            b[vv] = (in && lane < m) ? A.data[v * A.vs + lane * A.es] : 0.0;
            double sum = wave_sum(b[vv]);
            bool mk = in && (A.mask ? (A.mask[v] != 0) : true);
            bool fin = (ballot(!isfinite(b[vv])) == 0ull);
            act[vv] = mk && fin && (sum > 0.0);
            best_r[vv] = INFINITY; best_km[vv] = 0.0; best_fa[vv] = 0;
        }
        // Lower bounds (A.Hq): the NNLS residual of a flip angle is at least the unconstrained least-squares residual on its dictionary's
        // column space, ||b||^2 - ||Q_fa^T b||^2 in the plan's low-rank basis (exact to 1e-18 ||b||^2 while the basis leaves < 1e-9 of D).
        // The angle with the smallest bound is solved first (round -1); in rounds 0 .. nfa - 1 an angle whose bound exceeds the best
        // residual found so far cannot be the argmin and is skipped -- on the reference's recipe 28 of 91 angles per voxel are solved
        // (median 24).  Lane f (and f + 64) forms the bound of angle f and parks it in the voxel's own row of Hq (no registers held
        // through the walk).
        double slack[VPW];
        int fa0[VPW];
        u64 cand[VPW][2];                      // flip angles whose bound does not exceed the best residual so far (wave-uniform masks; all ones: no pruning)
        // the masks are formed again whenever the best residual improves: lane f compares its angle's parked bound
        auto candidates = [&](int vv) {
            const double tb = fma(best_r[vv], 1.0 + 1e-6, slack[vv]);     // sqrt(lb) > best (1 + 1e-6) + 1e-7 ||b||, compared as squares
            const double thr = tb * tb;
            const double *q = A.Lb + (size_t)(v0 + vv - A.v0) * (size_t)A.nfa;
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                const int f = lane + 64 * sl;
                const double lb = q[min(f, A.nfa - 1)];
                cand[vv][sl] = ballot(f < A.nfa && !(lb > thr));
            }
        };
#pragma unroll
        for (int vv = 0; vv < VPW; ++vv) {
            slack[vv] = 0.0; fa0[vv] = -1; cand[vv][0] = cand[vv][1] = ~0ull;
            if (PRUNE && A.Hq && act[vv]) {
                const double bb2 = wave_sum(b[vv] * b[vv]);
                const double *q = A.Hq + (size_t)(v0 + vv - A.v0) * ((size_t)A.nfa * MET2_GCV_LR_RANK);
                double *qb = A.Lb + (size_t)(v0 + vv - A.v0) * (size_t)A.nfa;
                double l2[2];
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    const int f = lane + 64 * sl;
                    double cs = 0.0;
                    if (f < A.nfa)
                        for (int j = 0; j < MET2_GCV_LR_RANK; ++j) { const double c = q[(size_t)f * MET2_GCV_LR_RANK + j]; cs = fma(c, c, cs); }
                    l2[sl] = (f < A.nfa) ? bb2 - cs : INFINITY;
                    if (f < A.nfa) qb[f] = l2[sl];
                }
                // What the bound may be off by: the basis leaves E = (I - Q Q^T) D, ||E|| <= 1e-9 of the largest column, outside, and the residual
                // of ANY x is at least ||b_perp|| - ||E x||; with ||x||_1 <= a few ||b|| per unit column norm (x >= 0 and a dictionary of decaying
                // signals: the first echo alone bounds x) that is < 1e-8 ||b||.  1e-7 ||b|| covers it sixteen times over and the rounding of
                // the difference above (1e-16 ||b||^2, i.e. 1e-8 ||b|| at worst) as well; on noisy data it prunes nothing less.
                slack[vv] = 1e-7 * sqrt(bb2);
                const double mn = wave_min(fmin(l2[0], l2[1]));
                const u64 m0 = ballot(l2[0] == mn), m1 = ballot(l2[1] == mn);
                fa0[vv] = m0 ? first_lane(m0) : 64 + first_lane(m1);
            }
        }
        for (int i = (PRUNE && A.Hq) ? -1 : 0; i < A.nfa; ++i) {
#ifdef MET2_CYCSTATS
            const unsigned long long cv0 = __builtin_readcyclecounter();
#endif
            if (!A.H && !(PRUNE && A.Hq)) {    // few flip angles: no batched contraction; rows of D come from L2, each loaded once for all the wave's voxels
                const double *Bf = A.Bfa + (size_t)i * n * n;
                S.B = Bf; S.D = A.Dfa + (size_t)i * m * n; S.Dt = A.Dtfa + (size_t)i * m * n;
#pragma unroll
                for (int bb = 0; bb < NB; ++bb) { const int j = min(lane + 64 * bb, n - 1); S.bdiag[bb] = Bf[(size_t)j * n + j]; }
                double hh[VPW][NB];
                project_multi<NB, VPW>(S, b, lane, hh);
#pragma unroll
                for (int vv = 0; vv < VPW; ++vv)
#pragma unroll
                    for (int bb = 0; bb < NB; ++bb) st[vv].h[bb] = hh[vv][bb];
            }
#pragma unroll
            for (int vv = 0; vv < VPW; ++vv) {
                const int fa = (PRUNE && i < 0) ? fa0[vv] : i;
                if (!act[vv] || (PRUNE && (fa < 0 || (i >= 0 && fa == fa0[vv])))) continue;
                if (PRUNE && !((cand[vv][fa >> 6] >> (fa & 63)) & 1ull)) continue;   // its lower bound exceeds the best residual: cannot be the argmin
                if (A.H || (PRUNE && A.Hq)) {
                    const double *Bf = A.Bfa + (size_t)fa * n * n;
                    S.B = Bf; S.D = A.Dfa + (size_t)fa * m * n; S.Dt = A.Dtfa + (size_t)fa * m * n;
#pragma unroll
                    for (int bb = 0; bb < NB; ++bb) { const int j = min(lane + 64 * bb, n - 1); S.bdiag[bb] = Bf[(size_t)j * n + j]; }
                    if (PRUNE && A.Hq) {
                        // h = A_fa^T c_fa from the plan's low-rank basis: D_fa = Q_fa A_fa to 1e-10 of its largest column, so this is D_fa^T (Q Q^T b), and the
                        // NNLS against the projected data has the minimiser of the NNLS against b (b - Q Q^T b is orthogonal to everything D_fa x can
                        // reach): residuals equal to 1e-14 relative (numpy, both shapes).  16 FMAs per bin from a 128-byte row of a 1.4 MB table that
                        // stays in L2, where the batched contraction wrote 87 KB of H per voxel at 91 x 120 and the walk read a third of it back.
                        const double *cq = A.Hq + (size_t)(v0 + vv - A.v0) * ((size_t)A.nfa * MET2_GCV_LR_RANK) + (size_t)fa * MET2_GCV_LR_RANK;
                        const double cl = cq[lane & (MET2_GCV_LR_RANK - 1)];
                        const met2_d2 *aq = (const met2_d2 *)(A.Aq + (size_t)fa * n * MET2_GCV_LR_RANK);
#pragma unroll
                        for (int bb = 0; bb < NB; ++bb) {
                            const int j = min(lane + 64 * bb, n - 1);
                            met2_d2 av[MET2_GCV_LR_RANK / 2];
#pragma unroll
                            for (int t = 0; t < MET2_GCV_LR_RANK / 2; ++t) av[t] = aq[(size_t)j * (MET2_GCV_LR_RANK / 2) + t];
                            double h0 = 0.0, h1 = 0.0;
#pragma unroll
                            for (int t = 0; t < MET2_GCV_LR_RANK / 2; ++t) { h0 = fma(av[t].x, bcast(cl, 2 * t), h0); h1 = fma(av[t].y, bcast(cl, 2 * t + 1), h1); }
                            st[vv].h[bb] = (lane + 64 * bb < n) ? h0 + h1 : 0.0;
                        }
                    } else {                   // h of this flip angle from the batched MFMA contraction: one contiguous row per voxel
                        const double *hrow = A.H + (size_t)(v0 + vv - A.v0) * Mh + (size_t)fa * n;
#pragma unroll
                        for (int bb = 0; bb < NB; ++bb) { const int j = lane + 64 * bb; const double hv = hrow[min(j, n - 1)]; st[vv].h[bb] = (j < n) ? hv : 0.0; }
                    }
                }
                nnls_solve_warm<NB, (NB == 2 && VPW == 1)>(S, bd, st[vv], 0.0, false, lane);   // one position slot (k <= nTE); with two voxels per wave the second code path stops the voxel loop from unrolling
                const double rn = sqrt(sse_of<NB>(S, st[vv], b[vv], lane));
                if (A.resid && lane == 0) A.resid[(size_t)(v0 + vv) * A.nfa + fa] = rn;
                if (rn < best_r[vv] || (rn == best_r[vv] && fa < best_fa[vv])) {      // np.argmin: the first minimum wins, whatever order the angles are visited in
                    best_r[vv] = rn; best_fa[vv] = fa;
                    double t = 0.0;
#pragma unroll
                    for (int bb = 0; bb < NB; ++bb) t += (lane + 64 * bb < n) ? st[vv].x[bb] : 0.0;
                    best_km[vv] = wave_sum(t);
                    if (PRUNE && A.Hq) candidates(vv);
                }
            }
#ifdef MET2_CYCSTATS
            st[0].cyc[0] += __builtin_readcyclecounter() - cv0;
#endif
        }
#ifdef MET2_CYCSTATS
#pragma unroll
        for (int vv = 0; vv < VPW; ++vv) MET2_CYC_FLUSH(st[vv]);
#endif
#pragma unroll
        for (int vv = 0; vv < VPW; ++vv) {
            const int64_t v = v0 + vv;
            if (v < A.v_end && lane == 0) {
                A.fa_index[v] = act[vv] ? (double)best_fa[vv] : 0.0;
                if (A.km) A.km[v] = act[vv] ? best_km[vv] : 0.0;
            }
            if (v < A.v_end && A.resid && !act[vv]) for (int f = lane; f < A.nfa; f += 64) A.resid[(size_t)v * A.nfa + f] = 0.0;
        }
    }
}

// zeros for gated-out voxels (motor:115-117) and the metrics an all-zero spectrum gets at
// motor:448-468 when mask > 0 (T2_M = T2_IE = exp(0) = 1, TWC = 1e-16)
__global__ __launch_bounds__(256) void finalize_unfitted_kernel(int64_t nvox, int n, int m, const int *__restrict__ key,
                                                                const uint8_t *__restrict__ mask, double *__restrict__ fsol,
                                                                double *__restrict__ sig, double *__restrict__ reg,
                                                                double *__restrict__ lam, double *__restrict__ maps)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < nvox * n; i += stride) if (key[i / n] < 0) fsol[i] = 0.0;
    if (sig) for (int64_t i = t0; i < nvox * m; i += stride) if (key[i / m] < 0) sig[i] = 0.0;
    for (int64_t v = t0; v < nvox; v += stride) {
        if (key[v] >= 0) continue;
        reg[v] = 0.0;
        if (lam) lam[v] = 0.0;
        if (maps) {
            bool mk = mask ? (mask[v] != 0) : true;
            maps[0 * nvox + v] = 0.0; maps[1 * nvox + v] = 0.0; maps[2 * nvox + v] = 0.0;
            maps[3 * nvox + v] = mk ? 1.0 : 0.0; maps[4 * nvox + v] = mk ? 1.0 : 0.0;
            maps[5 * nvox + v] = mk ? 1.0e-16 : 0.0;
        }
    }
}

// ------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------
// re-factorisations that took the packed leg of refactor_rowwise, counted by fits under the test switch MET2_REFAC_COUNT (met2_refac_packed_calls)
__device__ unsigned long long g_refac_packed_calls;

static void default_lambda_grid(std::vector<double> &g)
{
    g.assign(50, 0.0);   // motor:248-251
    const double l0 = log10(1e-8), l1 = log10(10.0);
    for (int i = 0; i < 49; ++i) g[i + 1] = pow(10.0, l0 + (l1 - l0) * (double)i / 48.0);
    g[49] = 10.0;
}

static int ensure_sort_bufs(met2_plan *p, int64_t nvox)
{
    if (nvox <= p->cap_vox) return MET2_OK;
    if (p->dKey) HIPCHK(hipFree(p->dKey));
    if (p->dPerm) HIPCHK(hipFree(p->dPerm));
    if (p->dOvf) HIPCHK(hipFree(p->dOvf));
    HIPCHK(hipMalloc(&p->dKey, sizeof(int) * (size_t)nvox));
    HIPCHK(hipMalloc(&p->dPerm, sizeof(int) * (size_t)nvox));
    HIPCHK(hipMalloc(&p->dOvf, sizeof(int) * (size_t)nvox));
    p->cap_vox = nvox;
    return MET2_OK;
}

// met2_fit_host reserves a plan's per-voxel scratch for its largest block before the block loop (met2_host.hip)
int met2::plan_reserve(met2_plan *p, int64_t nvox)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    USE_DEVICE(p->opt.device);
    return ensure_sort_bufs(p, nvox);
}

static SortBufs sort_bufs(met2_plan *p)
{
    SortBufs sb;
    const int nf = p->n_fa + 1;
    sb.key = p->dKey; sb.perm = p->dPerm; sb.ovf = p->dOvf;
    sb.hist = p->dSmall; sb.cursor = p->dSmall + nf; sb.bucket_start = p->dSmall + 2 * nf; sb.chunk_start = p->dSmall + 3 * nf;
    sb.queue = p->dSmall + 4 * nf; sb.err = p->dSmall + 4 * nf + 1; sb.xq = p->dSmall + 4 * nf + 8;
    return sb;
}


// GCV's kernel variant: the trace from the 17 x 17 low-rank form when the plan's dictionary allows it, unless MET2_GCV_FULL is set (the one
// place fit_impl, met2_plan_gcv_form and met2_plan_launch_info take it from)
static int kernel_method(const met2_plan *p, int method)
{
    return (method == MET2_GCV && p->gcv_lr && !test_switch("MET2_GCV_FULL")) ? MET2_GCV_LR : method;
}

// kmax_cap > 0: capacity of the passive set for this launch (fast path); 0: full capacity n.
// `method` is the kernel's template method (10 + base for the objective-grid kernels), so that the waves per workgroup come from
// the same number as the kernel's __launch_bounds__.
static int fit_geometry(const met2_plan *p, int method, LaunchGeom &g, int kmax_cap = 0, int wave_cap = 0, int64_t nvox = -1)
{
    const int n = p->n_t2, m = p->n_te;
    const int base = method >= 10 ? method - 10 : method;
    g.nb = n > 64 ? 2 : 1;
    g.kmax = (kmax_cap > 0 && kmax_cap < n) ? kmax_cap : n;
    g.wave_doubles = col_base(g.kmax);                                 // the factor, packed by columns without padding (nnls_wave.hpp)
    if (base == MET2_GCV && gcv_lds_doubles(m, n) > g.wave_doubles) g.wave_doubles = gcv_lds_doubles(m, n);      // M ((m+1)^2) + vectors + support list
    if (base == MET2_GCV_LR && gcv_lds_doubles(MET2_GCV_LR_RANK, n) > g.wave_doubles) g.wave_doubles = gcv_lds_doubles(MET2_GCV_LR_RANK, n);
    if (method == MET2_BAYESREG && g.nb == 2 && chol_panel_doubles(n) > g.wave_doubles) g.wave_doubles = chol_panel_doubles(n);   // chol_lean's 16-row panel
    g.wave_doubles = (g.wave_doubles + 1) & ~1;                        // every wave's region starts 16-byte aligned
    // D, D^T, B and K are read through L1/L2: with warm starts a lambda evaluation reads only ~k rows of B, and the LDS is worth
    // more as room for resident waves (measured on X2/L2 in round 1: staged 8 waves 1.555 M voxels/s, unstaged 11 waves 1.821 M)
    const size_t per_wave = sizeof(double) * (size_t)g.wave_doubles;
    const size_t budget = 160 * 1024 - 64;
    if (per_wave > budget) return fail(MET2_E_UNSUPPORTED, "shape does not fit the LDS budget");
    int w = (int)(budget / per_wave);
    const int wmax = wave_cap > 0 ? wave_cap : method_max_waves(method, g.nb);     // (the FA kernels have their own launch bounds)
    if (w > wmax) w = wmax;
    // small voxel lists (every wave pulls single voxels): no more waves per CU than the list gives every CU, in whole
    // multiples of the four SIMDs -- with 16 waves per CU racing for 1 024 voxels the CUs that win run four voxels per SIMD while
    // others idle (configs[0]: 1.16 ms at 16 waves, 0.85 ms at 4)
    if (nvox >= 0) {
        const int cus = p->cus > 0 ? p->cus : 256;
        int64_t per_cu = (nvox + cus - 1) / cus;
        int ww = (int)(((per_cu + 3) / 4) * 4);
        if (ww < 4) ww = 4;
        if (ww < w) w = ww;
    }
    w = tuning_env("MET2_WAVES", 1, w, w);
    g.waves = w; g.block = 64 * w;
    g.lds = (int)(per_wave * w + 64);
    g.grid = p->cus > 0 ? p->cus : 256;
    return MET2_OK;
}

// Fast-path capacity: the passive set rarely exceeds ~0.75 n (X2/L2 at nT2=60 peaks at 42-45 on the first,
// large-lambda Brent points), and LDS per wave grows with kmax^2.  Methods whose second phase needs the
// full n x n region (BayesReg) or their own matrix (GCV) do not use it.
static int fast_kmax(const met2_plan *p, int method)
{
    if (method >= 10 || (method == MET2_BAYESREG && p->n_t2 <= 64)) return 0;     // (BayesReg at one bin per lane factorises n x n in the wave's region)
    { const int kk = test_value("MET2_KMAX", 8, p->n_t2 - 1, -1); if (kk > 0) return kk; }
    // the largest capacity that still lets 16 waves share the LDS, but not below 0.6 n.  The figures below were measured with the
    // capacity ladder of rounds 1-4, which solved the voxels that outgrew the capacity again in a clean-up launch at full capacity
    // (measured on X2/L2, nT2 = 60: kmax 48 -> 1.95 M voxels/s, 50 -> 2.10 M, 52 (14 waves) -> 2.03 M, 60 (11 waves) -> 1.84 M;
    //  nT2 = 120 with the per-wave queue, where the clean-up pass is cheap: kmax 56 / 64 / 72 / 80 / 96 ->
    //  320 / 464 / 583 / 534 / 391 k voxels/s at 12 / 9 / 7 / 6 / 4 waves per CU)
    int k16 = 8;
    while (16 * sizeof(double) * (size_t)col_base(k16 + 1) <= 160 * 1024 - 64) ++k16;
    int k = (3 * p->n_t2 + 4) / 5;
    if (k16 > k) k = k16;
    if (p->n_t2 > 64) {
        // two bins per lane: those kernels are compiled for 8 waves per CU (method_max_waves), so the capacity that still lets EIGHT
        // regions share the LDS -- 71 at nT2 = 120, where 0.6 n = 72 gave 7 (round 3, with the ladder, X2/L2 at 48 x 120 on 32 768 voxels: first pass
        // 26.1 -> 23.2 ms, clean-up 5.2 -> 6.4 ms; 64 -> 22.4 + 17.7 ms; 80 / 90 / 110 -> 29.0 / 41.4 / 53.3 ms with a clean-up pass
        // that stays at ~5 ms: a few voxels whose set at the first abscissae is nearly all of the grid.  A middle pass at capacity
        // 88 or 100 between the two made the clean-up slower, 6.7 -> 10 ms: those voxels outgrow it too and are solved three times) ...
        int k8 = 8;
        while (8 * sizeof(double) * (size_t)col_base(k8 + 1) <= 160 * 1024 - 64) ++k8;
        k = k8;
        // ... and GCV's region is set by its (m + 1)^2 matrix anyway: the largest factor that fits in it
        if (method == MET2_GCV) while (col_base(k + 1) <= gcv_lds_doubles(p->n_te, p->n_t2)) ++k;
    }
    return k < p->n_t2 ? k : 0;
}

template <int METHOD>
static int launch_fit(const FitArgs &A, const LaunchGeom &g, hipStream_t s, bool second = false)
{
    if (second) {      // the spill-over kernel (fit_kernel.hpp): every method but the objective grids
        if (METHOD >= 10) return fail(MET2_E_INVALID, "no spill-over kernel for this method");
        constexpr int M2 = METHOD >= 10 ? MET2_NNLS : METHOD;
        return g.nb == 2 ? launch_fit_nb<M2, 2, true>(A, g, s) : launch_fit_nb<M2, 1, true>(A, g, s);
    }
    return g.nb == 2 ? launch_fit_nb<METHOD, 2, false>(A, g, s) : launch_fit_nb<METHOD, 1, false>(A, g, s);
}

// -DMET2_ONLY=<method number> builds the fit kernel of that method only (plus plain NNLS): a development switch that
// cuts the compile time of an experiment from ~80 s to ~15 s; the shipped library is built without it
#ifdef MET2_ONLY
#define MET2_HAS(m) ((m) == MET2_ONLY || (m) == 0)
#else
#define MET2_HAS(m) 1
#endif

static int launch_method(int method, const FitArgs &A, const LaunchGeom &g, hipStream_t s, bool second = false)
{
    switch (method) {
#if MET2_HAS(2)
    case 10 + MET2_X2: return launch_fit<10 + MET2_X2>(A, g, s);
    case MET2_X2: return launch_fit<MET2_X2>(A, g, s, second);
#endif
#if MET2_HAS(4)
    case 10 + MET2_GCV: return launch_fit<10 + MET2_GCV>(A, g, s);
    case MET2_GCV: return launch_fit<MET2_GCV>(A, g, s, second);
    case 10 + MET2_GCV_LR: return launch_fit<10 + MET2_GCV_LR>(A, g, s);
    case MET2_GCV_LR: return launch_fit<MET2_GCV_LR>(A, g, s, second);
#endif
#if MET2_HAS(5)
    case 10 + MET2_BAYESREG: return launch_fit<10 + MET2_BAYESREG>(A, g, s);
    case MET2_BAYESREG: return launch_fit<MET2_BAYESREG>(A, g, s, second);
#endif
    case MET2_NNLS: return launch_fit<MET2_NNLS>(A, g, s, second);
#if MET2_HAS(1)
    case MET2_T2SPARC: return launch_fit<MET2_T2SPARC>(A, g, s, second);
#endif
#if MET2_HAS(3)
    case MET2_LCURVE: return launch_fit<MET2_LCURVE>(A, g, s, second);
#endif
    default: return fail(MET2_E_UNSUPPORTED, "method not built");
    }
}

// Plan-level seeds (seed_kernel) are built where the dictionary, the penalty or T2SPARC's lambda are SET -- entries that
// synchronise -- never inside a fit: a fit on another stream or thread only ever reads finished records.
// Seeded starts equal the cold-start solution only when B + lambda K is positive definite (one minimiser).  That holds for the
// reference's I / L1 / L2 / InvT2; met2_plan_set_penalty_dense takes any banded L, e.g. a pure second difference whose null
// space meets that of D.  Checked here on the host by a Cholesky factorisation of B_0 + lambda K (flip angle 0, the three seed
// lambdas) with a relative pivot threshold; when it fails the plan simply runs unseeded.
static bool host_posdef(int n, std::vector<double> G)
{
    double dmax = 0.0;
    for (int i = 0; i < n; ++i) dmax = std::max(dmax, fabs(G[(size_t)i * n + i]));
    for (int j = 0; j < n; ++j) {
        double d = G[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= G[(size_t)j * n + k] * G[(size_t)j * n + k];
        if (!(d > 1e-13 * dmax)) return false;
        d = sqrt(d);
        G[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double t = G[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) t -= G[(size_t)i * n + k] * G[(size_t)j * n + k];
            G[(size_t)i * n + j] = t / d;
        }
    }
    return true;
}

int met2::ensure_seeds(met2_plan *p, hipStream_t s)
{
    if (!p->have_dict || !p->have_pen) return MET2_OK;
    const double key[7] = {p->opt.t2sparc_lambda, p->opt.x2_lo, p->opt.x2_hi, p->opt.gcv_lo, p->opt.gcv_hi, p->opt.bayes_lo, p->opt.bayes_hi};
    if (p->seeds_valid && memcmp(key, p->seeds_key, sizeof(key)) == 0) return MET2_OK;
    const int n = p->n_t2;
    const double gm = 0.5 * (3.0 - sqrt(5.0));
    SeedArgs SA;
    SA.n = n; SA.m = p->n_te; SA.nfa = p->n_fa;
    SA.Dfa = p->dD; SA.Bfa = p->dB; SA.Dtfa = p->dDt; SA.kband = p->dKband; SA.lband = p->dLband; SA.Kd = p->dKd;
    // the first abscissa of scipy's bounded Brent on each method's interval, a + g (b - a); T2SPARC's fixed lambda
    SA.lam[0] = p->opt.x2_lo + gm * (p->opt.x2_hi - p->opt.x2_lo); SA.lam[1] = p->opt.bayes_lo + gm * (p->opt.bayes_hi - p->opt.bayes_lo);
    SA.lam[2] = p->opt.t2sparc_lambda; SA.lam[3] = p->opt.gcv_lo + gm * (p->opt.gcv_hi - p->opt.gcv_lo);
    SA.out = p->dSeed;
    {
        std::vector<double> B0((size_t)n * n), K((size_t)n * n);
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(B0.data(), p->dB, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(K.data(), p->dKd, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost));
        bool ok = true;
        for (int q = 0; q < 4 && ok; ++q) {
            std::vector<double> G((size_t)n * n);
            for (size_t i = 0; i < G.size(); ++i) G[i] = B0[i] + SA.lam[q] * K[i];
            ok = SA.lam[q] > 0.0 && host_posdef(n, G);
        }
        p->seeds_ok = ok;
    }
    const int lds = (int)sizeof(double) * col_base(n) + 64;
    if (n <= 64) {
        HIPCHK(hipFuncSetAttribute((const void *)seed_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL(seed_kernel<1>, dim3(p->n_fa, 4), dim3(64), lds, s, SA);
    } else {
        HIPCHK(hipFuncSetAttribute((const void *)seed_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL(seed_kernel<2>, dim3(p->n_fa, 4), dim3(64), lds, s, SA);
    }
    HIPCHK(hipGetLastError());
    if (MET2_BAYES_TABLE > 0) {
        // BayesReg's shared abscissae on its interval ([1e-8, 2] in the reference; fminbound_dev with an objective that decreases towards
        // the lower bound): a + g (b - a), one golden step up, then golden steps down
        const double a = p->opt.bayes_lo, b = p->opt.bayes_hi;
        BayesTabArgs TA;
        TA.n = n; TA.m = p->n_te; TA.nfa = p->n_fa; TA.nj = MET2_BAYES_TABLE;
        TA.Bfa = p->dB; TA.Kd = p->dKd; TA.kband = p->dKband; TA.lband = p->dLband;
        double t0 = a + gm * (b - a);
        for (int j = 0; j < MET2_BAYES_TABLE; ++j) {
            double t;
            if (j == 0) t = t0;
            else if (j == 1) t = t0 + gm * (b - t0);
            else { const double prev = (j == 2) ? t0 : p->blam[j - 1]; t = prev + gm * (a - prev); }
            p->blam[j] = t; TA.lam[j] = t;
        }
        p->btab_stride = col_base(n) + 1;
        if (!p->dBtab) HIPCHK(hipMalloc(&p->dBtab, sizeof(double) * (size_t)p->n_fa * MET2_BAYES_TABLE * p->btab_stride));
        TA.stride = p->btab_stride; TA.out = p->dBtab;
        if (n <= 64) {
            HIPCHK(hipFuncSetAttribute((const void *)bayes_table_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            hipLaunchKernelGGL(bayes_table_kernel<1>, dim3(p->n_fa, MET2_BAYES_TABLE), dim3(64), lds, s, TA);
        } else {
            HIPCHK(hipFuncSetAttribute((const void *)bayes_table_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            hipLaunchKernelGGL(bayes_table_kernel<2>, dim3(p->n_fa, MET2_BAYES_TABLE), dim3(64), lds, s, TA);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));
    p->seeds_valid = true; memcpy(p->seeds_key, key, sizeof(key));
    return MET2_OK;
}

extern "C" {

void met2_default_options(met2_options *o)
{
    memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(met2_options);
    o->device = 0;
    o->x2_factor = 1.02;
    o->t2sparc_lambda = 1.8;
    o->brent_xtol = 1e-5;
    o->brent_maxfun = 0;
    o->t2_myelin_cut = 40.0;
    o->t2_ie_cut = 200.0;
    o->x2_lo = 0.0; o->x2_hi = 10.0;             // algorithms.py:219
    o->gcv_lo = 1e-8; o->gcv_hi = 10.0;          // algorithms.py:280
    o->bayes_lo = 1e-8; o->bayes_hi = 2.0;       // bayesian_interpolation.py:101
}

// a caller's options struct may be shorter than ours (an earlier ABI): what it does not carry keeps the value already in `dst`
static int take_options(met2_options *dst, const met2_options *src)
{
    if (src->struct_size < (int32_t)(2 * sizeof(int32_t))) return fail(MET2_E_INVALID, "met2_options.struct_size not set");
    memcpy(dst, src, sizeof(met2_options) < (size_t)src->struct_size ? sizeof(met2_options) : (size_t)src->struct_size);
    dst->struct_size = (int32_t)sizeof(met2_options);
    const double iv[3][2] = {{dst->x2_lo, dst->x2_hi}, {dst->gcv_lo, dst->gcv_hi}, {dst->bayes_lo, dst->bayes_hi}};
    for (int q = 0; q < 3; ++q)
        if (!(iv[q][0] >= 0.0) || !(iv[q][1] > iv[q][0]) || !std::isfinite(iv[q][1])) return fail(MET2_E_INVALID, "lambda-search interval: 0 <= lo < hi (finite) required");
    return MET2_OK;
}

int met2_abi_version(void) { return MET2_ABI_VERSION; }

int met2_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *met2_last_error(void) { return g_err.c_str(); }

int met2_plan_create(met2_plan **out, int32_t n_te, int32_t n_t2, int32_t n_fa, const met2_options *opt)
{
    if (!out) return fail(MET2_E_INVALID, "out is NULL");
    if (n_te < 2 || n_t2 < 2 || n_fa < 1) return fail(MET2_E_INVALID, "bad shape");
    if (n_t2 > 128) return fail(MET2_E_UNSUPPORTED, "n_t2 > 128 unsupported (two T2 bins per lane)");
    if (n_te > 63) return fail(MET2_E_UNSUPPORTED, "n_te > 63 unsupported (EPG orders live on the 64 lanes)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MET2_E_NODEVICE, "no HIP device visible");
    met2_plan *p = new met2_plan();
    p->n_te = n_te; p->n_t2 = n_t2; p->n_fa = n_fa;
    met2_default_options(&p->opt);
    if (opt) { const int rco = take_options(&p->opt, opt); if (rco) { delete p; return rco; } }
    if (p->opt.device < 0 || p->opt.device >= ndev) { delete p; return fail(MET2_E_INVALID, "device ordinal out of range"); }
    DevGuard dev_guard_(p->opt.device);
    if (dev_guard_.err != hipSuccess) { delete p; return fail(MET2_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dev_guard_.err)); }
    struct Guard { met2_plan *p; ~Guard() { if (p) (void)met2_plan_destroy(p); } } guard{p};      // a failing return below releases the plan and what it holds by then
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, p->opt.device));
    p->cus = prop.multiProcessorCount;
    HIPCHK(hipMalloc(&p->dD, sizeof(double) * (size_t)n_fa * n_te * n_t2));
    HIPCHK(hipMalloc(&p->dB, sizeof(double) * (size_t)n_fa * n_t2 * n_t2));
    HIPCHK(hipMalloc(&p->dDt, sizeof(double) * (size_t)n_fa * n_te * n_t2));
    HIPCHK(hipMalloc(&p->dAq, sizeof(double) * (size_t)n_fa * n_t2 * MET2_GCV_LR_RANK));
    HIPCHK(hipMalloc(&p->dAqRes, sizeof(double) * (size_t)n_fa));
    HIPCHK(hipMalloc(&p->dQt, sizeof(double) * (size_t)n_fa * MET2_GCV_LR_RANK * n_te));
    HIPCHK(hipMalloc(&p->dKband, sizeof(double) * 5 * 128));
    HIPCHK(hipMalloc(&p->dLband, sizeof(double) * 5 * 128));
    HIPCHK(hipMalloc(&p->dKd, sizeof(double) * (size_t)n_t2 * n_t2));
    HIPCHK(hipMemset(p->dKd, 0, sizeof(double) * (size_t)n_t2 * n_t2));
    HIPCHK(hipMalloc(&p->dT2, sizeof(double) * 128));
    HIPCHK(hipMalloc(&p->dSmall, sizeof(int) * (4 * (size_t)(n_fa + 1) + 16)));
    HIPCHK(hipMalloc(&p->dSeed, sizeof(SeedRec) * 4 * (size_t)n_fa));
    HIPCHK(hipHostMalloc((void **)&p->hErr, 4 * sizeof(int), hipHostMallocDefault));
    p->hErr[0] = p->hErr[1] = p->hErr[2] = p->hErr[3] = 0;
    HIPCHK(hipEventCreate(&p->ev0));
    HIPCHK(hipEventCreate(&p->ev1));
    HIPCHK(hipEventCreate(&p->ev2));
    std::vector<double> g;
    default_lambda_grid(g);
    const int rc = met2_plan_set_lambda_grid(p, g.data(), (int)g.size());
    if (rc) return rc;
    guard.p = nullptr;
    *out = p;
    return MET2_OK;
}

int met2_plan_set_options(met2_plan *p, const met2_options *opt)
{
    if (!p || !opt) return fail(MET2_E_INVALID, "NULL argument");
    if (opt->device != p->opt.device) return fail(MET2_E_INVALID, "a plan cannot change device");
    {
        met2_options o = p->opt;
        const int rco = take_options(&o, opt);
        if (rco) return rco;
        if (o.device != p->opt.device) return fail(MET2_E_INVALID, "a plan stays on the device it was created on");
        p->opt = o;
    }
    USE_DEVICE(p->opt.device);
    return ensure_seeds(p, 0);       // T2SPARC's seed belongs to its lambda
}

int met2_plan_get_options(met2_plan *p, met2_options *opt)
{
    if (!p || !opt) return fail(MET2_E_INVALID, "NULL argument");
    *opt = p->opt;
    return MET2_OK;
}

int met2_plan_get_shape(met2_plan *p, int32_t *n_te, int32_t *n_t2, int32_t *n_fa)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    if (n_te) *n_te = p->n_te;
    if (n_t2) *n_t2 = p->n_t2;
    if (n_fa) *n_fa = p->n_fa;
    return MET2_OK;
}

int met2_plan_destroy(met2_plan *p)
{
    if (!p) return MET2_OK;
    met2::host_release(p);           // what met2_fit_host keeps with the plan (met2_host.hip)
    met2::bootstrap_release(p);      // what met2_fit_bootstrap keeps with the plan (met2_bootstrap.hip)
    DevGuard dev_guard_(p->opt.device);
    void *bufs[] = {p->dQt, p->dAq, p->dAqRes, p->dD, p->dB, p->dDt, p->dKband, p->dLband, p->dKd, p->dLam, p->dT2, p->dKey, p->dPerm, p->dOvf, p->dSmall, p->dSeed, p->dBtab, p->dH, p->dChol, p->dBig, p->dLcSave};
    for (void *b : bufs) (void)hipFree(b);
    if (p->hErr) (void)hipHostFree(p->hErr);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    if (p->ev2) (void)hipEventDestroy(p->ev2);
    delete p;
    return MET2_OK;
}

int met2_plan_set_lambda_grid(met2_plan *p, const double *lam, int32_t n)
{
    if (!p || !lam || n < 3) return fail(MET2_E_INVALID, "bad lambda grid");
    if (n > 64) return fail(MET2_E_UNSUPPORTED, "lambda grid longer than 64 points");
    USE_DEVICE(p->opt.device);
    if (p->dLam) HIPCHK(hipFree(p->dLam));
    HIPCHK(hipMalloc(&p->dLam, sizeof(double) * n));
    HIPCHK(hipMemcpy(p->dLam, lam, sizeof(double) * n, hipMemcpyHostToDevice));
    p->nlam = n;
    return MET2_OK;
}

int met2_fit(met2_plan *p, int32_t method, int64_t nvox, const double *data, const double *fa_index, const uint8_t *mask,
             double *fsol, double *sig, double *reg, double *lam, double *maps, int32_t *status, void *stream)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    return met2_fit_strided(p, method, nvox, data, p->n_te, 1, fa_index, mask, fsol, sig, reg, lam, maps, status, stream);
}

static int fit_impl(met2_plan *p, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                    const double *fa_index, const uint8_t *mask, double *fsol, double *sig, double *reg, double *lam, double *maps,
                    int32_t *status, void *stream, bool sync);

int met2_fit_strided(met2_plan *p, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                     const double *fa_index, const uint8_t *mask, double *fsol, double *sig, double *reg, double *lam, double *maps,
                     int32_t *status, void *stream)
{
    return fit_impl(p, method, nvox, data, voxel_stride, echo_stride, fa_index, mask, fsol, sig, reg, lam, maps, status, stream, true);
}

int met2_fit_enqueue_strided(met2_plan *p, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                             const double *fa_index, const uint8_t *mask, double *fsol, double *sig, double *reg, double *lam, double *maps,
                             int32_t *status, void *stream)
{
    return fit_impl(p, method, nvox, data, voxel_stride, echo_stride, fa_index, mask, fsol, sig, reg, lam, maps, status, stream, false);
}

int met2_plan_finish(met2_plan *p, void *stream)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    USE_DEVICE(p->opt.device);
    if (p->err_pending && p->err_stream != (hipStream_t)stream)
        return fail(MET2_E_STATE, "met2_plan_finish on another stream than the one the plan's fits were enqueued on");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (p->err_pending) {
        p->err_pending = false;
        const int herr = p->hErr[0];
        p->last_spill = p->hErr[1];
        p->hErr[0] = 0;
        if (herr & 1) return fail(MET2_E_INVALID, "FA index outside the dictionary's flip-angle axis");
    }
    return MET2_OK;
}

// MET2_DEBUG: waits for the fit kernels; libraries built with -DMET2_CYCSTATS, -DMET2_BIGSTATS or -DMET2_LOOPSTATS print their counters too
static int debug_counters(int method, hipStream_t s)
{
    (void)method;
    HIPCHK(hipStreamSynchronize(s)); fprintf(stderr, "[met2] fit kernel done\n");
#ifdef MET2_CYCSTATS
    unsigned long long cy[16];
    HIPCHK(hipMemcpyFromSymbol(cy, HIP_SYMBOL(met2::g_cyc), sizeof(cy)));
    fprintf(stderr, "[met2] gcv trace: gram(mfma)=%llu tridiag=%llu bisect=%llu weights=%llu\n", cy[8], cy[9], cy[10], cy[11]);
    fprintf(stderr, "[met2] calls: warm solves=%llu duals=%llu append rounds=%llu inner loops after an append=%llu\n", cy[12], cy[13], cy[14], cy[15]);
    fprintf(stderr, "[met2] wave cycles: voxel=%llu refactor=%llu inner=%llu dual=%llu append=%llu | slots 5-7 (x2: sse, removals, removal cycles; bayes: chol, upper_times, erf/log; gcv small path: cycles, evaluations, sweeps; append slot += sum k)=%llu %llu %llu\n",
            cy[0], cy[1], cy[2], cy[3], cy[4], cy[5], cy[6], cy[7]);
    {
        unsigned long long rk[4];
        HIPCHK(hipMemcpyFromSymbol(rk, HIP_SYMBOL(met2::g_refk), sizeof(rk)));
        fprintf(stderr, "[met2] row-by-row re-factorisations: calls=%llu row-terms=%llu | with k > 32: calls=%llu row-terms=%llu\n", rk[0], rk[1], rk[2], rk[3]);
    }
    if (method == MET2_X2) {
        static unsigned long long ev[40][12];
        HIPCHK(hipMemcpyFromSymbol(ev, HIP_SYMBOL(met2::g_ev), sizeof(ev)));
        fprintf(stderr, "[met2] X2 per Brent evaluation index: evals canonical | cycles per eval: refactor inner(incl. removal) dual append sse | removals/eval removal-cycles/eval | k start -> end\n");
        for (int e = 0; e < 40; ++e) {
            if (!ev[e][0]) continue;
            const double c = (double)ev[e][0];
            fprintf(stderr, "[met2]  ev %2d: %9llu %9llu | %8.0f %8.0f %8.0f %8.0f %8.0f | %5.2f %8.0f | %5.1f -> %5.1f\n", e, ev[e][0], ev[e][10], ev[e][1] / c, ev[e][2] / c,
                    ev[e][3] / c, ev[e][4] / c, ev[e][5] / c, ev[e][6] / c, ev[e][7] / c, ev[e][8] / c, ev[e][9] / c);
        }
    }
#endif
#ifdef MET2_BIGSTATS
    { unsigned long long bs[16]; HIPCHK(hipMemcpyFromSymbol(bs, HIP_SYMBOL(met2::g_bigstats), sizeof(bs)));
      fprintf(stderr, "[met2] spill-over voxels: solver calls=%llu, with spill-over legs=%llu | cycles plain=%llu spill=%llu (refactor in slot %llu) | appends=%llu removals=%llu refactors=%llu | k start sum=%llu end sum=%llu\n",
              bs[0], bs[1], bs[2], bs[3], bs[9], bs[4], bs[5], bs[6], bs[8], bs[7]); }
#endif
#ifdef MET2_LOOPSTATS
    int ls[8];
    HIPCHK(hipMemcpyFromSymbol(ls, HIP_SYMBOL(met2::g_loopstats), sizeof(ls)));
    fprintf(stderr, "[met2] loop maxima: tries=%d sweeps=%d outer=%d iter=%d taken=%d round=%d jacobi_sweeps=%d last_sweep_rotations=%d\n", ls[0], ls[1], ls[2], ls[3], ls[4], ls[5], ls[6], ls[7]);
#endif
    fflush(stderr);
    return MET2_OK;
}

// a scratch buffer of the plan's that a fit grows on demand: waits for the stream's work on the old one before it goes
static int grow_device(double *&buf, int64_t &cap, int64_t need, hipStream_t s)
{
    if (cap >= need) return MET2_OK;
    if (buf) { HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipFree(buf)); buf = nullptr; cap = 0; }
    HIPCHK(hipMalloc(&buf, sizeof(double) * (size_t)need));
    cap = need;
    return MET2_OK;
}

static int fit_impl(met2_plan *p, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                    const double *fa_index, const uint8_t *mask, double *fsol, double *sig, double *reg, double *lam, double *maps,
                    int32_t *status, void *stream, bool sync)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    if (voxel_stride == 0 || echo_stride == 0) return fail(MET2_E_INVALID, "zero stride");
    if (nvox == 0) return MET2_OK;                       // empty voxel list: nothing to do (pointers may be NULL)
    if (!data || !fsol || !reg) return fail(MET2_E_INVALID, "NULL argument");
    if (nvox < 0 || nvox > 0x7fffffff) return fail(MET2_E_INVALID, "nvox out of range");
    if (!p->have_dict) return fail(MET2_E_STATE, "no dictionary in the plan");
    if (method != MET2_NNLS && !p->have_pen) return fail(MET2_E_STATE, "no penalty matrix set");
    if (maps && !p->have_t2) return fail(MET2_E_STATE, "metrics requested but no T2 grid set");
    const bool objgrid = method >= 10;
    if (objgrid) { method -= 10; if (method != MET2_X2 && method != MET2_GCV && method != MET2_BAYESREG) return fail(MET2_E_INVALID, "no objective for this method"); }
    if (method < 0 || method > MET2_BAYESREG) return fail(MET2_E_INVALID, "unknown method");
    if (objgrid && p->nlam > p->n_t2) return fail(MET2_E_UNSUPPORTED, "objective grid longer than n_t2");
    USE_DEVICE(p->opt.device);
    hipStream_t s = (hipStream_t)stream;
    if (p->err_pending && p->err_stream != s)
        return fail(MET2_E_STATE, "fits are pending on another stream of this plan: call met2_plan_finish on it first (one plan serves one stream at a time)");
    int rc = ensure_sort_bufs(p, nvox);
    if (rc) return rc;
    // capacity scheme: the fit kernel runs at a passive-set capacity kfast < n (more waves per CU); the voxels whose set outgrows it
    // go on in the spill-over kernel behind it
    const int kmeth = kernel_method(p, method);
    const int kfast = objgrid ? 0 : fast_kmax(p, kmeth);
    LaunchGeom g;
    rc = fit_geometry(p, objgrid ? kmeth + 10 : kmeth, g, kfast, 0, nvox);
    if (rc) return rc;
    if (!p->have_pen) {   // plain NNLS never touches the bands, but the kernel loads them
        HIPCHK(hipMemsetAsync(p->dKband, 0, sizeof(double) * 5 * 128, s));
        HIPCHK(hipMemsetAsync(p->dLband, 0, sizeof(double) * 5 * 128, s));
        HIPCHK(hipMemsetAsync(p->dKd, 0, sizeof(double) * (size_t)p->n_t2 * p->n_t2, s));
    }
    if (!p->have_t2) HIPCHK(hipMemsetAsync(p->dT2, 0, sizeof(double) * 128, s));
    SortBufs sb = sort_bufs(p);
    // counters and cursors start at zero; the error word (index 4 (nfa + 1) + 1) keeps what earlier ENQUEUED fits may have set
    hipLaunchKernelGGL(reset_sort_kernel, dim3(1), dim3(256), 0, s, sb, p->n_fa, p->err_pending ? 1 : 0);
    const int nbs = (int)((nvox + MET2_SORT_BLOCK - 1) / MET2_SORT_BLOCK);          // classify / scatter: one global atomic per (workgroup, flip angle)
    const size_t sort_lds = sizeof(int) * 2 * ((size_t)p->n_fa + 1);                // per-flip-angle tables of the sort kernels in LDS
    if (sort_lds > 48 * 1024) {
        if (sort_lds > 150 * 1024) return fail(MET2_E_UNSUPPORTED, "more than 19 000 flip angles (or ROIs) in one plan");
        HIPCHK(hipFuncSetAttribute((const void *)classify_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds));
        HIPCHK(hipFuncSetAttribute((const void *)scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds));
        HIPCHK(hipFuncSetAttribute((const void *)scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds));
    }
    // work-queue granularity: every wave pulls
    // its own voxels -- one at a time for the methods that spend ~1 ms per voxel (X2/L2 on configs[1]: 1 / 2 / 4 / 8 / 16
    // voxels per pull -> 5.37 / 5.32 / 5.22 / 5.04 / 4.71 M voxels/s; HBM writes 1.01 / 0.93 / 0.88 / 0.89 GB because the
    // 8-byte per-voxel outputs of neighbouring voxels then leave from different XCDs), eight at a time for NNLS and
    // T2SPARC, where one atomic per voxel on the queue word would cap the kernel at 23 M voxels/s (8 -> 82 M)
    int chunk = (method <= MET2_T2SPARC) ? 8 : 1;
    chunk = tuning_env("MET2_CHUNK", 1, 1024, chunk);
    const bool dbg = test_switch("MET2_DEBUG");
    if (dbg) { HIPCHK(hipStreamSynchronize(s)); fprintf(stderr, "[met2] fit: nvox=%lld grid=%d block=%d lds=%d\n", (long long)nvox, g.grid, g.block, g.lds); fflush(stderr); }
    hipLaunchKernelGGL(classify_kernel, dim3(nbs), dim3(MET2_SORT_BLOCK), sort_lds, s, nvox, p->n_te, p->n_fa, data, voxel_stride, echo_stride, fa_index, mask, 1, sb, status);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(256), sort_lds, s, p->n_fa, chunk, sb);
    if (dbg) { HIPCHK(hipStreamSynchronize(s)); fprintf(stderr, "[met2] classify done\n"); fflush(stderr); }
    hipLaunchKernelGGL(scatter_kernel, dim3(nbs), dim3(MET2_SORT_BLOCK), sort_lds, s, nvox, p->n_fa, sb);
    HIPCHK(hipGetLastError());
    if (dbg) {
        HIPCHK(hipStreamSynchronize(s));
        std::vector<int> hs(4 * (size_t)(p->n_fa + 1) + 8);
        HIPCHK(hipMemcpy(hs.data(), p->dSmall, sizeof(int) * hs.size(), hipMemcpyDeviceToHost));
        fprintf(stderr, "[met2] sort done: fitted=%d chunks=%d\n", hs[2 * (p->n_fa + 1) + p->n_fa], hs[3 * (p->n_fa + 1) + p->n_fa]); fflush(stderr);
    }

    FitArgs A;
    A.n = p->n_t2; A.m = p->n_te; A.nfa = p->n_fa; A.kmax = g.kmax; A.waves = g.waves; A.chunk = chunk; A.wave_doubles = g.wave_doubles;
    A.method = method; A.nlam = p->nlam;
    A.maxfun = p->opt.brent_maxfun > 0 ? p->opt.brent_maxfun : (method == MET2_BAYESREG ? 200 : 300);
    A.x2_factor = p->opt.x2_factor; A.t2sparc_lambda = p->opt.t2sparc_lambda; A.xtol = p->opt.brent_xtol;
    A.cut_m = p->opt.t2_myelin_cut; A.cut_ie = p->opt.t2_ie_cut;
    A.lam_lo = method == MET2_GCV ? p->opt.gcv_lo : (method == MET2_BAYESREG ? p->opt.bayes_lo : p->opt.x2_lo);       // the lambda search's interval
    A.lam_hi = method == MET2_GCV ? p->opt.gcv_hi : (method == MET2_BAYESREG ? p->opt.bayes_hi : p->opt.x2_hi);
    A.log_detL = p->log_detL;
    A.Dfa = p->dD; A.Bfa = p->dB; A.Dtfa = p->dDt; A.Aq = p->dAq; A.kband = p->dKband; A.lband = p->dLband; A.Kd = p->dKd; A.lam_grid = p->dLam; A.t2s = p->dT2;
    A.data = data; A.vs = voxel_stride; A.es = echo_stride; A.sb = sb; A.fsol = fsol; A.sig = sig; A.reg = reg; A.lam = lam; A.maps = maps; A.status = status; A.nvox = nvox;

    A.test_switches = (test_switch("MET2_REFAC_PAIR") ? FitArgs::TEST_REFAC_PAIR : 0) | (test_switch("MET2_SUBST_REF") ? FitArgs::TEST_SUBST_REF : 0) |
                      (test_switch("MET2_ROWWALK_REF") ? FitArgs::TEST_ROWWALK_REF : 0) | (test_switch("MET2_DUAL_REF") ? FitArgs::TEST_DUAL_REF : 0);
    // dual()'s x table pays where other waves of the SIMD cover its LDS round trip.  A launch of at most one wave per SIMD (a short voxel list:
    // fit_geometry) is as long as its slowest voxel's chain of latencies, and there the table is slower than the lane reads (configs[0], 1 024 voxels
    // on 4 waves per CU: -0.7 %, profiles/dualx_ab.txt section 5c): such launches take the lane reads.  MET2_DUAL_TAB (tests) keeps the table.
    if (g.waves <= 4 && !test_switch("MET2_DUAL_TAB")) A.test_switches |= FitArgs::TEST_DUAL_REF;
    A.refac_count = nullptr;
    if (test_switch("MET2_REFAC_COUNT")) HIPCHK(hipGetSymbolAddress((void **)&A.refac_count, HIP_SYMBOL(g_refac_packed_calls)));
    A.seed = nullptr;
    if (!test_switch("MET2_NO_SEED") && !objgrid && p->have_pen && p->seeds_valid && p->seeds_ok && p->seeds_key[0] == p->opt.t2sparc_lambda &&
        (method == MET2_X2 || method == MET2_GCV || method == MET2_BAYESREG || method == MET2_T2SPARC)) {
        const int slot = method == MET2_BAYESREG ? 1 : (method == MET2_T2SPARC ? 2 : (method == MET2_GCV ? 3 : 0));      // records built by ensure_seeds() when the plan was configured
        A.seed = p->dSeed + sizeof(SeedRec) * (size_t)slot * p->n_fa;
    }
    A.btab = nullptr; A.nbtab = 0; A.btab_stride = p->btab_stride;
    A.chol = nullptr; A.chol_stride = 0;
    if (method == MET2_BAYESREG && !objgrid && g.nb == 2) {
        // chol_lean's scratch: one packed factor per wave of the launch (the spill-over kernel runs with the same geometry)
        const int stride = (col_base(p->n_t2) + 15) & ~15;
        const int64_t need = (int64_t)g.grid * g.waves * stride;
        rc = grow_device(p->dChol, p->cap_chol, need, s);
        if (rc) return rc;
        A.chol = p->dChol; A.chol_stride = stride;
    }
    // spill-over slots (nnls_big.hpp): a set that outgrows the LDS capacity of the launch goes on in the spill-over kernel, its columns beyond
    // the capacity in the wave's slot
    A.big = nullptr; A.big_stride = 0;
    if (kfast) {
        const int stride = (col_base(p->n_t2) - col_base(g.kmax) + 15) & ~15;
        LaunchGeom gw;                                                      // sized for the widest launch of this shape (a short voxel list runs fewer waves):
        rc = fit_geometry(p, kmeth, gw, kfast, 0, -1);                      // the slots are allocated once, not per block of a host pipeline
        if (rc) return rc;
        const int64_t need = (int64_t)gw.grid * gw.waves * stride;
        rc = grow_device(p->dBig, p->cap_big, need, s);
        if (rc) return rc;
        A.big = p->dBig; A.big_stride = stride;
    }
    A.lc_save = nullptr; A.lc_at = nullptr; A.lc_cap = 0;
    if (A.big && method == MET2_LCURVE && g.nb == 2 && !objgrid && !test_switch("MET2_LC_RESTART")) {
        // records for a sixteenth of the voxels (5 % of them overflow on measured spectra), between 4 096 and 262 144 (2.4 GB): entries beyond start over
        const int64_t cap = std::min<int64_t>(nvox, std::min<int64_t>(262144, std::max<int64_t>(4096, nvox / 16)));
        const int64_t need = cap * (LC_SAVE_DOUBLES * 64) + (cap + 1) / 2;
        rc = grow_device(p->dLcSave, p->cap_lc, need, s);
        if (rc) return rc;
        A.lc_save = p->dLcSave; A.lc_at = (int *)(p->dLcSave + cap * (LC_SAVE_DOUBLES * 64)); A.lc_cap = (int)cap;
    }
    for (int j = 0; j < (MET2_BAYES_TABLE > 0 ? MET2_BAYES_TABLE : 1); ++j) A.blam[j] = p->blam[j];
    if (MET2_BAYES_TABLE > 0 && method == MET2_BAYESREG && !objgrid && p->dBtab && p->seeds_valid && p->seeds_ok && !tuning_env("MET2_NO_BAYES_TABLE", 0, 1, 0)) {
        A.btab = p->dBtab; A.nbtab = MET2_BAYES_TABLE;
    }
    // The fit kernels carry the reference's lambda-search intervals as literals (fit_kernel.hpp: FitArgs::lam_lo); a plan whose options name other
    // intervals runs every voxel through the spill-over kernel, whose instance of the voxel routine reads them -- correct, and slower (the solver is
    // a function call there).
    const bool custom_iv = !objgrid && ((method == MET2_X2 && (p->opt.x2_lo != 0.0 || p->opt.x2_hi != 10.0)) || (method == MET2_GCV && (p->opt.gcv_lo != 1e-8 || p->opt.gcv_hi != 10.0)) ||
                                        (method == MET2_BAYESREG && (p->opt.bayes_lo != 1e-8 || p->opt.bayes_hi != 2.0)));
    A.all_queued = custom_iv ? 1 : 0;
    HIPCHK(hipEventRecord(p->ev0, s));
    if (objgrid) { A.sig = nullptr; A.maps = nullptr; A.lam = nullptr; }
    if (!custom_iv) {
        rc = launch_method(objgrid ? kmeth + 10 : kmeth, A, g, s);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(p->ev1, s));
    // the spill-over kernel: the voxels the first kernel queued (their passive set outgrew the LDS capacity; under custom intervals every fitted
    // voxel), same geometry, the solver with its spill-over legs -- no re-sort, no second capacity; it finds an empty queue in most launches at
    // one bin per lane
    const bool spill = A.big || custom_iv;
    if (spill) {
        rc = launch_method(kmeth, A, g, s, true);
        if (rc) return rc;
        HIPCHK(hipEventRecord(p->ev2, s));
    }
    p->timed = true; p->timed2 = spill;
    if (dbg) { rc = debug_counters(method, s); if (rc) return rc; }
    hipLaunchKernelGGL(finalize_unfitted_kernel, dim3(p->cus * 4), dim3(256), 0, s, nvox, p->n_t2, p->n_te, p->dKey, mask, fsol,
                       objgrid ? nullptr : sig, reg, objgrid ? nullptr : lam, objgrid ? nullptr : maps);
    HIPCHK(hipGetLastError());
    // FA index range errors (IndexError in the reference): the error word lands in the plan's pinned host word; the blocking entries
    // wait for it here, an enqueued fit leaves it to met2_plan_finish (errors of several enqueued fits accumulate: the kernel ORs)
    HIPCHK(hipMemcpyAsync(p->hErr, sb.err, 4 * sizeof(int), hipMemcpyDeviceToHost, s));      // the error word and the spill-over queue.s tail and head
    p->err_pending = true; p->err_stream = s;
    if (!sync) return MET2_OK;
    return met2_plan_finish(p, stream);
}

int met2_fa_bruteforce(met2_plan *p, int64_t nvox, const double *data, const uint8_t *mask, double *fa_index, double *km,
                       double *resid, void *stream)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    return met2_fa_bruteforce_strided(p, nvox, data, p->n_te, 1, mask, fa_index, km, resid, stream);
}

int met2_fa_bruteforce_strided(met2_plan *p, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                               const uint8_t *mask, double *fa_index, double *km, double *resid, void *stream)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    if (nvox == 0) return MET2_OK;                       // empty voxel list: nothing to do (pointers may be NULL)
    if (nvox < 0 || !data || !fa_index) return fail(MET2_E_INVALID, "NULL argument");
    if (voxel_stride == 0 || echo_stride == 0) return fail(MET2_E_INVALID, "zero stride");
    if (!p->have_dict) return fail(MET2_E_STATE, "no dictionary in the plan");
    USE_DEVICE(p->opt.device);
    hipStream_t s = (hipStream_t)stream;
    LaunchGeom g;
    // plain NNLS stops at min(n_t2, n_te) passive bins (Lawson-Hanson's k >= rows test), so the factor needs that
    // capacity only: 4 KB per wave at nTE = 32 instead of 14.6 KB; every wave walks the flip angles on its own, 16 waves per CU.
    const int kcap = p->n_te < p->n_t2 ? p->n_te : 0;
    int rc = fit_geometry(p, MET2_NNLS, g, kcap, 16);
    if (rc) return rc;
    const int fa_waves = g.waves >= 16 ? 16 : (g.waves >= 8 ? 8 : g.waves);
    if (g.waves != fa_waves) {
        g.waves = fa_waves; g.block = 64 * fa_waves;
        g.lds = (int)(sizeof(double) * (size_t)g.wave_doubles * fa_waves + 64);
    }
    SortBufs sb = sort_bufs(p);
    FaArgs A;
    A.n = p->n_t2; A.m = p->n_te; A.nfa = p->n_fa; A.kmax = g.kmax; A.waves = g.waves; A.wave_doubles = g.wave_doubles;
    A.Dfa = p->dD; A.Bfa = p->dB; A.Dtfa = p->dDt; A.Kd = p->dKd; A.data = data; A.vs = voxel_stride; A.es = echo_stride; A.mask = mask; A.fa_index = fa_index; A.km = km; A.resid = resid;
    A.queue = sb.queue; A.nvox = nvox;
    // h = D_fa^T b of all flip angles by one MFMA GEMM per pass of voxels (fa_project_kernel) when the plan has more than a handful
    // of flip angles; the pass size bounds the scratch (8 nfa n bytes per voxel: 87 KB at 91 x 120)
    // Mh: doubles of H per voxel -- h of every flip angle, and behind it (when the walk prunes) the 16 coefficients of the voxel in every
    // flip angle's low-rank basis.  Pruning needs the basis to span the dictionary (p->gcv_lr), all residuals NOT to be asked for, and the
    // bounds of all angles to fit two per lane; MET2_FA_NOPRUNE=1: test switch.
    const bool prune = p->gcv_lr && !resid && p->n_fa >= 8 && p->n_fa <= 128 && !test_switch("MET2_FA_NOPRUNE");      // (<= 128: the bounds are formed two per lane)
    // round 5: a pruning walk forms its h from the low-rank basis (fa_kernel), so its scratch is the 16 coefficients per angle and the bounds --
    // 12.4 KB per voxel at 91 angles where H took 87 KB more; the exhaustive walk (all residuals asked for; a dictionary the basis does not span) keeps H
    const int64_t Mh0 = prune ? 0 : (int64_t)p->n_fa * p->n_t2;
    const int64_t Mh = Mh0 + (prune ? (int64_t)p->n_fa * (MET2_GCV_LR_RANK + 1) : 0);
    const bool gemm = p->n_fa >= 8 && tuning_env("MET2_FA_GEMM", 0, 1, 1) != 0;
    int64_t pass = nvox;
    if (gemm) {
        // scratch: at most 6 GiB and at most a quarter of what the device has free right now (several plans or ranks may share it);
        // a failed allocation halves the pass instead of failing the call
        size_t mem_free = 0, mem_total = 0;
        HIPCHK(hipMemGetInfo(&mem_free, &mem_total));
        const int64_t budget = std::min<int64_t>((int64_t)6 << 30, (int64_t)(mem_free / 4) + (int64_t)sizeof(double) * p->cap_h);
        pass = std::max<int64_t>(32, std::min<int64_t>(nvox, (budget / (8 * Mh)) & ~(int64_t)31));
        if (p->cap_h >= 32 * Mh && p->cap_h < pass * Mh && p->cap_h >= std::min<int64_t>(nvox, 65536) * Mh)
            pass = (p->cap_h / Mh) & ~(int64_t)31;                                  // what the plan already holds serves 64 Ki voxels a pass: keep it
        if (p->cap_h < pass * Mh) {
            if (p->dH) { HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipFree(p->dH)); p->dH = nullptr; p->cap_h = 0; }
            for (;;) {
                const hipError_t e = hipMalloc(&p->dH, sizeof(double) * (size_t)(pass * Mh));
                if (e == hipSuccess) break;
                (void)hipGetLastError();
                p->dH = nullptr;
                if (pass <= 32) return fail(MET2_E_HIP, std::string("hipMalloc of the FA walk's scratch: ") + hipGetErrorString(e));
                pass = std::max<int64_t>(32, (pass / 2) & ~(int64_t)31);
            }
            p->cap_h = pass * Mh;
        }
    }
    HIPCHK(hipEventRecord(p->ev0, s));
#define MET2_FA_LAUNCH(VPW, NB, WAVES)                                                                                   \
    do {                                                                                                                \
        if (A.Hq) {                                                                                                     \
            HIPCHK(hipFuncSetAttribute((const void *)fa_kernel<VPW, NB, WAVES, true>, hipFuncAttributeMaxDynamicSharedMemorySize, g.lds)); \
            hipLaunchKernelGGL((fa_kernel<VPW, NB, WAVES, true>), dim3(g.grid), dim3(g.block), g.lds, s, A);              \
        } else {                                                                                                        \
            HIPCHK(hipFuncSetAttribute((const void *)fa_kernel<VPW, NB, WAVES, false>, hipFuncAttributeMaxDynamicSharedMemorySize, g.lds)); \
            hipLaunchKernelGGL((fa_kernel<VPW, NB, WAVES, false>), dim3(g.grid), dim3(g.block), g.lds, s, A);             \
        }                                                                                                               \
    } while (0)
    for (int64_t v0 = 0; v0 < nvox; v0 += pass) {
        A.v0 = v0; A.v_end = std::min<int64_t>(nvox, v0 + pass); A.H = nullptr; A.Hq = nullptr; A.Lb = nullptr; A.Aq = p->dAq;
        HIPCHK(hipMemsetAsync(sb.queue, 0, sizeof(int), s));
        if (gemm) {
            FaGemmArgs G;
            G.n = p->n_t2; G.m = p->n_te; G.nfa = p->n_fa; G.Dtfa = p->dDt; G.data = data; G.vs = voxel_stride; G.es = echo_stride; G.H = p->dH;
            G.v0 = v0; G.v_end = A.v_end;
            const int64_t waves = (A.v_end - v0 + 31) / 32;
            const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
            const int ks = (p->n_te + 3) / 4;
            if (prune) {                                                            // the contraction on the stacked bases: [T x m] . [m x nfa 16]
                G.n = MET2_GCV_LR_RANK; G.Dtfa = p->dQt;
                A.Hq = p->dH; A.Lb = p->dH + (size_t)pass * p->n_fa * MET2_GCV_LR_RANK;
            } else A.H = p->dH;
            if (ks <= 8)       hipLaunchKernelGGL(fa_project_kernel<8>, grid, block, 0, s, G);
            else if (ks <= 12) hipLaunchKernelGGL(fa_project_kernel<12>, grid, block, 0, s, G);
            else               hipLaunchKernelGGL(fa_project_kernel<16>, grid, block, 0, s, G);
            HIPCHK(hipGetLastError());
        }
        if (g.nb == 1) { if (g.waves == 16) MET2_FA_LAUNCH(2, 1, 16); else MET2_FA_LAUNCH(4, 1, 8); }
        else           { if (g.waves == 16) MET2_FA_LAUNCH(1, 2, 16); else MET2_FA_LAUNCH(2, 2, 8); }   // two voxels per wave at two bins per lane: same 57 ms (measured)
    }
#undef MET2_FA_LAUNCH
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->ev1, s));
#ifdef MET2_CYCSTATS
    if (test_switch("MET2_DEBUG")) {
        HIPCHK(hipStreamSynchronize(s));
        unsigned long long cy[8];
        HIPCHK(hipMemcpyFromSymbol(cy, HIP_SYMBOL(met2::g_cyc), sizeof(cy)));
        fprintf(stderr, "[met2] fa wave cycles: solves=%llu barrier-wait=%llu staging=%llu | refactor=%llu inner=%llu dual=%llu append=%llu\n", cy[0], cy[5], cy[6], cy[1], cy[2], cy[3], cy[4]);
    }
#endif
    p->timed = true;
    return MET2_OK;
}

int met2_plan_last_kernel_ms(met2_plan *p, double *ms)
{
    if (!p || !ms) return fail(MET2_E_INVALID, "NULL argument");
    if (!p->timed) return fail(MET2_E_STATE, "no timed launch yet");
    USE_DEVICE(p->opt.device);
    HIPCHK(hipEventSynchronize(p->ev1));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, p->ev0, p->ev1));
    *ms = (double)f;
    return MET2_OK;
}

int met2_plan_last_spill_count(met2_plan *p, int64_t *count)
{
    if (!p || !count) return fail(MET2_E_INVALID, "NULL argument");
    *count = p->last_spill;
    return MET2_OK;
}

int met2_plan_last_second_pass_ms(met2_plan *p, double *ms)
{
    if (!p || !ms) return fail(MET2_E_INVALID, "NULL argument");
    *ms = 0.0;
    if (!p->timed || !p->timed2) return MET2_OK;
    USE_DEVICE(p->opt.device);
    HIPCHK(hipEventSynchronize(p->ev2));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, p->ev1, p->ev2));
    *ms = (double)f;
    return MET2_OK;
}

int met2_plan_gcv_form(met2_plan *p, int32_t *low_rank, double *residual)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    if (!p->have_dict) return fail(MET2_E_STATE, "no dictionary in the plan");
    if (low_rank) *low_rank = kernel_method(p, MET2_GCV) == MET2_GCV_LR ? 1 : 0;
    if (residual) *residual = p->gcv_res;
    return MET2_OK;
}

int met2_refac_packed_calls(met2_plan *p, uint64_t *calls, int32_t reset)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    USE_DEVICE(p->opt.device);
    HIPCHK(hipDeviceSynchronize());
    unsigned long long v = 0;
    HIPCHK(hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_refac_packed_calls), sizeof(v)));
    if (calls) *calls = (uint64_t)v;
    if (reset) { v = 0; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_refac_packed_calls), &v, sizeof(v))); }
    return MET2_OK;
}

int met2_plan_launch_info(met2_plan *p, int32_t method, int32_t *grid, int32_t *block, int32_t *lds_bytes)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    LaunchGeom g;
    method = kernel_method(p, method);      // the variant fit_impl launches
    const int kf = fast_kmax(p, method);
    int rc = fit_geometry(p, method, g, kf);
    if (rc) return rc;
    if (grid) *grid = g.grid;
    if (block) *block = g.block;
    if (lds_bytes) *lds_bytes = g.lds;
    return MET2_OK;
}

} // extern "C"
