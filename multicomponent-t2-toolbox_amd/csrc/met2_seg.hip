// met2_seg.hip -- met2_tissue_segment: tissue segmentation of a 3-D map (segment='yes'; the second purpose of step 5 of the reference's example
// pipeline, which runs FSL's fast on the total water content map on the CPU).  The hidden-Markov-random-field EM of Zhang, Brady & Smith (IEEE
// TMI 20:45-57, 2001): Gaussian classes in log intensity, a Potts prior over the six face neighbours, labels by iterated conditional modes;
// include/met2_hip.h states the algorithm; no program text of FSL was used.  The domain, the log, the initial classes, the plain EM steps and
// the M-step are the kernels of the bias-field correction (bias_common.hpp), launched through its host code.  New here:
//   seg_consts_kernel     a_k = 1 / (2 var_k), h_k = log(var_k) / 2 and the live flags, from the class record
//   seg_init_kernel       the first labels: argmin_k D_k over the compacted list
//   seg_icm_kernel<C>     one colour pass of a checkerboard sweep: a tile of 4 x 8 x 16 labels with its one-voxel halo in LDS, one thread per
//                         z-adjacent pair of voxels, which updates the one of colour C
//   seg_posterior_kernel  the posteriors given the labels and the partials of the M-step's 3 K sums in bias_estep_kernel's layout
//   seg_finish_kernel     the rank of the classes by mean, the relabelling, seg and prob
// The host reads nothing back: every launch of the call is enqueued up front.  Every loop is bounded by a shape or a compile-time constant;
// fp64 throughout.  No energy is formed with a fused multiply-add: see rn_mul.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "bias_common.hpp"

namespace {

#define SEG_TX 4                          // the tile of seg_icm_kernel: 4 x 8 x 16 voxels, 256 z-adjacent pairs
#define SEG_TY 8
#define SEG_TZ 16
#define SEG_LZ (SEG_TZ + 2)               // its extents in LDS, with the halo
#define SEG_LY (SEG_TY + 2)
#define SEG_LX (SEG_TX + 2)
#define SEG_OFF 255                       // the label of a voxel off the domain

struct SegConsts {
    double a[BIAS_MAX_K], h[BIAS_MAX_K];
    int32_t live[BIAS_MAX_K];
};

struct SegGeom {
    int nx, ny, nz;
    double beta, wx, wy, wz;
};

// D_k = (y - mu_k)^2 a_k + h_k
__device__ __forceinline__ double seg_data_term(double yv, double mu, double a, double h)
{
    const double d = rn_sub(yv, mu);
    return rn_add(rn_mul(rn_mul(d, d), a), h);
}

// P_k = beta ((w_x c_x + w_y c_y) + w_z c_z)
__device__ __forceinline__ double seg_penalty(const SegGeom &G, int cx, int cy, int cz)
{
    return rn_mul(G.beta, rn_add(rn_add(rn_mul(G.wx, (double)cx), rn_mul(G.wy, (double)cy)), rn_mul(G.wz, (double)cz)));
}

__device__ __forceinline__ int seg_differs(int nb, int k) { return nb != SEG_OFF && nb != k ? 1 : 0; }

__global__ __launch_bounds__(64) void seg_consts_kernel(const BiasStats *__restrict__ st, SegConsts *__restrict__ sc, int K)
{
    const int k = threadIdx.x;
    if (k >= BIAS_MAX_K) return;
    const bool in = k < K;
    const double var = in ? st->var[k] : 1.0;
    sc->a[k] = 1.0 / (2.0 * var);                                     // 2 var is exact: one rounding
    sc->h[k] = 0.5 * log(var);
    sc->live[k] = in && st->pi[k] != 0.0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void seg_init_kernel(const double *__restrict__ y, const int32_t *__restrict__ idx,
                                                       const BiasStats *__restrict__ st, const SegConsts *__restrict__ sc, int K,
                                                       uint8_t *__restrict__ lab)
{
    const int N = st->N;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (st->degenerate || i >= N) return;
    const int32_t at = idx[i];
    const double yv = y[at];
    int best = -1;
    double be = INFINITY;
    for (int k = 0; k < K; ++k) {
        if (!sc->live[k]) continue;                                   // uniform
        const double e = seg_data_term(yv, st->mu[k], sc->a[k], sc->h[k]);
        if (best < 0 || e < be) { best = k; be = e; }
    }
    lab[at] = (uint8_t)best;                                          // a class is live: the weights sum to 1
}

// One colour pass.  Tiles are numbered along blockIdx.x, z fastest.  Thread t owns the voxels z0 + 2 (t & 7) and the next of line
// (x0 + (t >> 6), y0 + ((t >> 3) & 7)) and updates the one with (x + y + z) & 1 == COLOUR: the six neighbours of that voxel have the other
// colour, which no thread of this launch writes, so the pass does not depend on the order of the threads or on the tiling.
template <int COLOUR>
__global__ __launch_bounds__(256) void seg_icm_kernel(uint8_t *__restrict__ lab, const double *__restrict__ y, const BiasStats *__restrict__ st,
                                                      const SegConsts *__restrict__ sc, int K, SegGeom G)
{
    __shared__ uint8_t tile[SEG_LX * SEG_LY * SEG_LZ];
    __shared__ double cmu[BIAS_MAX_K], ca[BIAS_MAX_K], ch[BIAS_MAX_K];
    __shared__ int clive[BIAS_MAX_K];
    if (st->degenerate) return;
    const int t = threadIdx.x;
    const int ntz = (G.nz + SEG_TZ - 1) / SEG_TZ, nty = (G.ny + SEG_TY - 1) / SEG_TY;
    int bid = blockIdx.x;
    const int z0 = (bid % ntz) * SEG_TZ;
    bid /= ntz;
    const int y0 = (bid % nty) * SEG_TY, x0 = (bid / nty) * SEG_TX;
    if (t < BIAS_MAX_K) {
        cmu[t] = t < K ? st->mu[t] : 0.0;
        ca[t] = sc->a[t];
        ch[t] = sc->h[t];
        clive[t] = t < K ? sc->live[t] : 0;
    }
    for (int e = t; e < SEG_LX * SEG_LY * SEG_LZ; e += 256) {
        const int gz = z0 - 1 + e % SEG_LZ, gy = y0 - 1 + (e / SEG_LZ) % SEG_LY, gx = x0 - 1 + e / (SEG_LZ * SEG_LY);
        const bool in = gx >= 0 && gx < G.nx && gy >= 0 && gy < G.ny && gz >= 0 && gz < G.nz;
        tile[e] = in ? lab[((int64_t)gx * G.ny + gy) * G.nz + gz] : (uint8_t)SEG_OFF;
    }
    __syncthreads();
    const int tx = t >> 6, ty = (t >> 3) & 7;
    const int gx = x0 + tx, gy = y0 + ty;
    const int tz = 2 * (t & 7) + ((COLOUR + gx + gy + z0) & 1);
    const int gz = z0 + tz;
    if (gx >= G.nx || gy >= G.ny || gz >= G.nz) return;
    const uint8_t *c = tile + ((tx + 1) * SEG_LY + (ty + 1)) * SEG_LZ + (tz + 1);
    if (c[0] == SEG_OFF) return;
    const int xm = c[-SEG_LY * SEG_LZ], xp = c[SEG_LY * SEG_LZ], ym = c[-SEG_LZ], yp = c[SEG_LZ], zm = c[-1], zp = c[1];
    const int64_t at = ((int64_t)gx * G.ny + gy) * G.nz + gz;
    const double yv = y[at];
    int best = -1;
    double be = INFINITY;
    for (int k = 0; k < K; ++k) {
        if (!clive[k]) continue;                                      // uniform
        const double e = rn_add(seg_data_term(yv, cmu[k], ca[k], ch[k]),
                                seg_penalty(G, seg_differs(xm, k) + seg_differs(xp, k), seg_differs(ym, k) + seg_differs(yp, k),
                                            seg_differs(zm, k) + seg_differs(zp, k)));
        if (best < 0 || e < be) { best = k; be = e; }
    }
    lab[at] = (uint8_t)best;
}

// The posteriors given the labels, over chunk c of the compacted list, in bias_estep_kernel<false>'s layout of entries and partials: slot k,
// 8 + k, 16 + k at stride pstride hold the chunk's sums of p_k, p_k y and (p_k d) d, d = y - mu_k, each term rounded operation by operation.
// prob_raw (NULL allowed): p_k of voxel i at [k n + i], classes in the record's order.
__global__ __launch_bounds__(256) void seg_posterior_kernel(const double *__restrict__ y, const int32_t *__restrict__ idx,
                                                            const uint8_t *__restrict__ lab, const BiasStats *__restrict__ st,
                                                            const SegConsts *__restrict__ sc, int K, SegGeom G, int pstride,
                                                            double *__restrict__ part, double *__restrict__ prob_raw, int64_t n)
{
    __shared__ double red[4];
    const int N = st->N;
    const int64_t c0 = (int64_t)blockIdx.x * BIAS_CHUNK;
    if (st->degenerate || c0 >= N) return;
    double mu[BIAS_MAX_K], a[BIAS_MAX_K], h[BIAS_MAX_K];
    bool live[BIAS_MAX_K];
#pragma unroll
    for (int k = 0; k < BIAS_MAX_K; ++k) {
        mu[k] = k < K ? st->mu[k] : 0.0;
        a[k] = sc->a[k];
        h[k] = sc->h[k];
        live[k] = k < K && sc->live[k] != 0;
    }
    double s0[BIAS_MAX_K], s1[BIAS_MAX_K], s2[BIAS_MAX_K];
#pragma unroll
    for (int k = 0; k < BIAS_MAX_K; ++k) { s0[k] = 0.0; s1[k] = 0.0; s2[k] = 0.0; }
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < N) {
            const int32_t at = idx[i];
            const int gz = at % G.nz, r = at / G.nz, gy = r % G.ny, gx = r / G.ny;
            const int64_t sx = (int64_t)G.ny * G.nz;
            const int xm = gx > 0 ? lab[at - sx] : SEG_OFF, xp = gx + 1 < G.nx ? lab[at + sx] : SEG_OFF;
            const int ym = gy > 0 ? lab[at - G.nz] : SEG_OFF, yp = gy + 1 < G.ny ? lab[at + G.nz] : SEG_OFF;
            const int zm = gz > 0 ? lab[at - 1] : SEG_OFF, zp = gz + 1 < G.nz ? lab[at + 1] : SEG_OFF;
            const double u = y[at];
            double l[BIAS_MAX_K], m = INFINITY;
#pragma unroll
            for (int k = 0; k < BIAS_MAX_K; ++k) {
                l[k] = INFINITY;
                if (live[k]) {
                    l[k] = rn_add(seg_data_term(u, mu[k], a[k], h[k]),
                                  seg_penalty(G, seg_differs(xm, k) + seg_differs(xp, k), seg_differs(ym, k) + seg_differs(yp, k),
                                              seg_differs(zm, k) + seg_differs(zp, k)));
                    m = fmin(m, l[k]);
                }
            }
            double se = 0.0;
#pragma unroll
            for (int k = 0; k < BIAS_MAX_K; ++k) {
                l[k] = live[k] ? exp(rn_sub(m, l[k])) : 0.0;
                se += l[k];
            }
#pragma unroll
            for (int k = 0; k < BIAS_MAX_K; ++k) {
                if (k < K) {
                    const double p = l[k] / se, d = rn_sub(u, mu[k]);
                    s0[k] = rn_add(s0[k], p);
                    s1[k] = rn_add(s1[k], rn_mul(p, u));
                    s2[k] = rn_add(s2[k], rn_mul(rn_mul(p, d), d));
                    if (prob_raw) prob_raw[(int64_t)k * n + at] = p;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < BIAS_MAX_K; ++k) {
        if (k < K) {                                                  // uniform
            const double a0 = block_sum(s0[k], red), a1 = block_sum(s1[k], red), a2 = block_sum(s2[k], red);
            if (threadIdx.x == 0) {
                part[(int64_t)k * pstride + blockIdx.x] = a0;
                part[(int64_t)(BIAS_MAX_K + k) * pstride + blockIdx.x] = a1;
                part[(int64_t)(2 * BIAS_MAX_K + k) * pstride + blockIdx.x] = a2;
            }
        }
    }
}

// rank_k = the number of classes j with mu_j < mu_k, or mu_j == mu_k and j < k: class k becomes label rank_k + 1 and row rank_k of prob and
// of classes.  dom is read only when the record says degenerate (seg = 1 and prob_0 = 1 on the domain); prob_raw only when prob is asked for.
__global__ __launch_bounds__(256) void seg_finish_kernel(const uint8_t *__restrict__ lab, const uint8_t *__restrict__ dom,
                                                         const double *__restrict__ prob_raw, const BiasStats *__restrict__ st, int K, int64_t n,
                                                         uint8_t *__restrict__ seg, double *__restrict__ prob, double *__restrict__ classes)
{
    __shared__ int rank[BIAS_MAX_K];
    if (threadIdx.x < BIAS_MAX_K) {
        const int k = threadIdx.x;
        int r = 0;
        for (int j = 0; j < K; ++j)
            if (k < K && (st->mu[j] < st->mu[k] || (st->mu[j] == st->mu[k] && j < k))) ++r;
        rank[k] = r;
        if (classes && blockIdx.x == 0 && k < K) {
            classes[r] = st->mu[k];
            classes[K + r] = st->var[k];
            classes[2 * K + r] = st->pi[k];
        }
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (st->degenerate) {
        const bool on = dom[i] != 0;
        if (seg) seg[i] = on ? 1 : 0;
        if (prob)
            for (int k = 0; k < K; ++k) prob[(int64_t)k * n + i] = on && k == 0 ? 1.0 : 0.0;
        return;
    }
    const int l = lab[i];
    const bool on = l < K;                                            // SEG_OFF is not
    if (seg) seg[i] = on ? (uint8_t)(rank[l] + 1) : 0;
    if (prob)
        for (int k = 0; k < K; ++k) prob[(int64_t)rank[k] * n + i] = on ? prob_raw[(int64_t)k * n + i] : 0.0;
}

// ---- the host code of the stages: each enqueues its launches on st and reads nothing back.  met2_tissue_segment and the stage entries below
// ---- run these helpers and launch no kernel of the segmentation otherwise.

// step 4's axis weights
SegGeom seg_geom(int nx, int ny, int nz, const double voxel_mm[3], double beta)
{
    const double dmin = std::fmin(voxel_mm[0], std::fmin(voxel_mm[1], voxel_mm[2]));
    SegGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz;
    G.beta = beta;
    G.wx = dmin / voxel_mm[0]; G.wy = dmin / voxel_mm[1]; G.wz = dmin / voxel_mm[2];
    return G;
}

void enq_seg_consts(hipStream_t st, const BiasStats *S, SegConsts *SC, int K)
{
    hipLaunchKernelGGL(seg_consts_kernel, dim3(1), dim3(64), 0, st, S, SC, K);
}

// lab = SEG_OFF everywhere, then the first labels on the list
hipError_t enq_seg_init(hipStream_t st, const BiasGrid &g, const double *y, const int32_t *idx, const BiasStats *S, const SegConsts *SC, int K,
                        uint8_t *lab)
{
    const hipError_t e = hipMemsetAsync(lab, SEG_OFF, (size_t)g.n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(seg_init_kernel, dim3(g.nel), dim3(256), 0, st, y, idx, S, SC, K, lab);
    return hipSuccess;
}

void enq_seg_pass(hipStream_t st, int colour, uint8_t *lab, const double *y, const BiasStats *S, const SegConsts *SC, int K, const SegGeom &G)
{
    const int64_t tiles = (int64_t)((G.nx + SEG_TX - 1) / SEG_TX) * ((G.ny + SEG_TY - 1) / SEG_TY) * ((G.nz + SEG_TZ - 1) / SEG_TZ);   // <= n
    if (colour == 0)
        hipLaunchKernelGGL(seg_icm_kernel<0>, dim3((unsigned)tiles), dim3(256), 0, st, lab, y, S, SC, K, G);
    else
        hipLaunchKernelGGL(seg_icm_kernel<1>, dim3((unsigned)tiles), dim3(256), 0, st, lab, y, S, SC, K, G);
}

void enq_seg_icm(hipStream_t st, int n_sweeps, uint8_t *lab, const double *y, const BiasStats *S, const SegConsts *SC, int K, const SegGeom &G)
{
    for (int s = 0; s < n_sweeps; ++s) {
        enq_seg_pass(st, 0, lab, y, S, SC, K, G);
        enq_seg_pass(st, 1, lab, y, S, SC, K, G);
    }
}

void enq_seg_posterior(hipStream_t st, const BiasGrid &g, const double *y, const int32_t *idx, const uint8_t *lab, const BiasStats *S,
                       const SegConsts *SC, int K, const SegGeom &G, double *part, double *prob_raw)
{
    hipLaunchKernelGGL(seg_posterior_kernel, dim3(g.nch), dim3(256), 0, st, y, idx, lab, S, SC, K, G, g.nch, part, prob_raw, g.n);
}

void enq_seg_finish(hipStream_t st, const BiasGrid &g, const uint8_t *lab, const uint8_t *dom, const double *prob_raw, const BiasStats *S, int K,
                    uint8_t *seg, double *prob, double *classes)
{
    hipLaunchKernelGGL(seg_finish_kernel, dim3(g.nel), dim3(256), 0, st, lab, dom, prob_raw, S, K, g.n, seg, prob, classes);
}

int seg_check_beta(double beta)
{
    if (!(beta >= 0.0) || !std::isfinite(beta)) return fail(MET2_E_INVALID, "beta must be finite and not negative");
    return MET2_OK;
}

int seg_check_voxel(const double voxel_mm[3])
{
    if (!voxel_mm) return fail(MET2_E_INVALID, "NULL voxel size");
    for (int a = 0; a < 3; ++a)
        if (!(voxel_mm[a] > 0.0) || !std::isfinite(voxel_mm[a])) return fail(MET2_E_INVALID, "the voxel size must be positive and finite");
    return MET2_OK;
}

// the stage entries' class record from the caller's classes [3 K] = mu, var, pi
int seg_record(int64_t n_domain, int n_class, const double *classes_in, BiasStats *h)
{
    if (n_class < 1) return fail(MET2_E_INVALID, "segmentation needs at least one class");
    if (!classes_in) return fail(MET2_E_INVALID, "NULL argument");
    if (n_class > BIAS_MAX_K) return fail(MET2_E_UNSUPPORTED, "segmentation supports at most 8 classes");
    std::memset(h, 0, sizeof *h);
    h->N = (int32_t)n_domain;
    for (int k = 0; k < n_class; ++k) {
        h->mu[k] = classes_in[k]; h->var[k] = classes_in[n_class + k]; h->pi[k] = classes_in[2 * n_class + k];
        if (!std::isfinite(h->mu[k]) || !std::isfinite(h->var[k]) || !(h->var[k] > 0.0) || !std::isfinite(h->pi[k]) || h->pi[k] < 0.0)
            return fail(MET2_E_INVALID, "a class needs a finite mean, a positive finite variance and a finite weight >= 0");
    }
    return MET2_OK;
}

int seg_check_volume(int nx, int ny, int nz, int64_t *n)
{
    if (nx < 1 || ny < 1 || nz < 1) return fail(MET2_E_INVALID, "the segmentation stages need at least one voxel");
    *n = (int64_t)nx * ny * nz;
    if (*n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    return MET2_OK;
}

}  // namespace

extern "C" int met2_tissue_segment(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const uint8_t *mask,
                                   const double voxel_mm[3], int32_t n_class, double beta, int32_t n_outer, int32_t n_em, int32_t n_icm,
                                   uint8_t *seg, double *prob, double *classes, void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0) return fail(MET2_E_INVALID, "bad shape");
    if (n_class < 1) return fail(MET2_E_INVALID, "segmentation needs at least one class");
    if (n_outer < 0 || n_em < 1) return fail(MET2_E_INVALID, "segmentation needs n_outer >= 0 and n_em >= 1");
    if (n_icm < 0) return fail(MET2_E_INVALID, "n_icm must not be negative");
    if (int rc = seg_check_voxel(voxel_mm)) return rc;
    if (int rc = seg_check_beta(beta)) return rc;
    const int64_t n = (int64_t)nx * ny * nz;
    if (n == 0) return MET2_OK;
    if (!v) return fail(MET2_E_INVALID, "NULL argument");
    if (n_class > BIAS_MAX_K) return fail(MET2_E_UNSUPPORTED, "segmentation supports at most 8 classes");
    if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    const int K = n_class;
    const SegGeom G = seg_geom(nx, ny, nz, voxel_mm, beta);
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;

    const BiasGrid g = bias_grid(n);
    DeviceWork W(st);
    const auto y = W.take<double>(n), b = W.take<double>(n);
    const auto idx = W.take<int32_t>(n);
    const auto dom = W.take<uint8_t>(n), lab = W.take<uint8_t>(n);
    const auto cnt = W.take<int32_t>(g.nch), off = W.take<int32_t>(g.nch);
    const auto part = W.take<double>((size_t)g.nch * 3 * BIAS_MAX_K);
    const auto S = W.take<BiasStats>(1);
    const auto SC = W.take<SegConsts>(1);
    const auto praw = W.take<double>(prob ? (size_t)n * K : 0);
    if (!W.alloc()) return W.finish("met2_tissue_segment");
    double *prob_raw = prob ? (double *)praw : nullptr;

    W.ok(hipMemsetAsync(S, 0, S.bytes, st));
    W.ok(hipMemsetAsync(b, 0, b.bytes, st));                              // step 1's EM runs with b = 0
    if (W.ok()) {
        enq_domain(st, g, v, mask, y, dom, cnt, off, idx, S);
        enq_init(st, g, y, idx, S, part, K);
        for (int em = 0; em < n_em; ++em) enq_em_step(st, g, y, b, idx, S, K, part);
        enq_seg_consts(st, S, SC, K);
        W.ok(hipGetLastError());
    }
    if (W.ok()) W.ok(enq_seg_init(st, g, y, idx, S, SC, K, lab));
    for (int it = 0; it < n_outer && W.ok(); ++it) {
        enq_seg_icm(st, n_icm, lab, y, S, SC, K, G);
        enq_seg_posterior(st, g, y, idx, lab, S, SC, K, G, part, nullptr);
        hipLaunchKernelGGL(bias_mstep_kernel, dim3(1), dim3(256), 0, st, part, g.nch, S, K);
        enq_seg_consts(st, S, SC, K);
        W.ok(hipGetLastError());
    }
    if (W.ok()) {
        enq_seg_icm(st, n_icm, lab, y, S, SC, K, G);
        if (prob) enq_seg_posterior(st, g, y, idx, lab, S, SC, K, G, part, prob_raw);
        if (seg || prob || classes) enq_seg_finish(st, g, lab, dom, prob_raw, S, K, seg, prob, classes);
    }
    return W.finish("met2_tissue_segment");
}

// ---- the stages one by one, for tests and diagnostics (include/met2_hip.h) ----

extern "C" int met2_seg_consts(int32_t device, int32_t n_class, const double *classes_in, double *a_out, double *h_out, int32_t *live_out,
                               void *stream)
{
    BiasStats h;
    if (int rc = seg_record(1, n_class, classes_in, &h)) return rc;
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork W(st);
    const auto S = W.take<BiasStats>(1);
    const auto SC = W.take<SegConsts>(1);
    if (!W.alloc()) return W.finish("met2_seg_consts");
    SegConsts c;
    if (W.ok(hipMemcpyAsync(S, &h, sizeof h, hipMemcpyHostToDevice, st))) {               // h lives until the wait
        enq_seg_consts(st, S, SC, n_class);
        W.ok(hipGetLastError());
    }
    if (W.ok()) W.ok(hipMemcpyAsync(&c, SC, sizeof c, hipMemcpyDeviceToHost, st));
    const int rc = W.finish("met2_seg_consts");
    if (rc != MET2_OK) return rc;
    for (int k = 0; k < n_class; ++k) {
        if (a_out) a_out[k] = c.a[k];
        if (h_out) h_out[k] = c.h[k];
        if (live_out) live_out[k] = c.live[k];
    }
    return MET2_OK;
}

extern "C" int met2_seg_init(int32_t device, int64_t n, const double *y, const int32_t *idx, int64_t n_domain, int32_t n_class,
                             const double *classes_in, uint8_t *labels, void *stream)
{
    if (n < 1) return fail(MET2_E_INVALID, "the segmentation stages need at least one voxel");
    if (n_domain < 0 || n_domain > n) return fail(MET2_E_INVALID, "the domain's size must lie in 0..n");
    if (!y || !idx || !labels) return fail(MET2_E_INVALID, "NULL argument");
    BiasStats h;
    if (int rc = seg_record(n_domain, n_class, classes_in, &h)) return rc;
    if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork W(st);
    const auto S = W.take<BiasStats>(1);
    const auto SC = W.take<SegConsts>(1);
    if (!W.alloc()) return W.finish("met2_seg_init");
    if (W.ok(hipMemcpyAsync(S, &h, sizeof h, hipMemcpyHostToDevice, st))) {               // h lives until the wait
        enq_seg_consts(st, S, SC, n_class);
        W.ok(hipGetLastError());
    }
    if (W.ok()) W.ok(enq_seg_init(st, bias_grid(n), y, idx, S, SC, n_class, labels));
    return W.finish("met2_seg_init");
}

extern "C" int met2_seg_icm(int32_t device, int32_t nx, int32_t ny, int32_t nz, uint8_t *labels, const double *y, int32_t n_class,
                            const double *classes_in, const double w[3], double beta, int32_t n_sweeps, int32_t colour, void *stream)
{
    int64_t n = 0;
    if (int rc = seg_check_volume(nx, ny, nz, &n)) return rc;
    if (!labels || !y || !w) return fail(MET2_E_INVALID, "NULL argument");
    if (n_sweeps < 0) return fail(MET2_E_INVALID, "n_sweeps must not be negative");
    if (colour < -1 || colour > 1) return fail(MET2_E_INVALID, "colour must be 0, 1 or -1 for both");
    if (int rc = seg_check_beta(beta)) return rc;
    for (int a = 0; a < 3; ++a)
        if (!(w[a] >= 0.0) || !std::isfinite(w[a])) return fail(MET2_E_INVALID, "an axis weight must be finite and not negative");
    BiasStats h;
    if (int rc = seg_record(1, n_class, classes_in, &h)) return rc;
    SegGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.beta = beta; G.wx = w[0]; G.wy = w[1]; G.wz = w[2];
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork W(st);
    const auto S = W.take<BiasStats>(1);
    const auto SC = W.take<SegConsts>(1);
    if (!W.alloc()) return W.finish("met2_seg_icm");
    if (W.ok(hipMemcpyAsync(S, &h, sizeof h, hipMemcpyHostToDevice, st))) {               // h lives until the wait
        enq_seg_consts(st, S, SC, n_class);
        if (colour < 0)
            enq_seg_icm(st, n_sweeps, labels, y, S, SC, n_class, G);
        else if (n_sweeps > 0)
            enq_seg_pass(st, colour, labels, y, S, SC, n_class, G);
    }
    return W.finish("met2_seg_icm");
}

extern "C" int met2_seg_posterior(int32_t device, int32_t nx, int32_t ny, int32_t nz, const uint8_t *labels, const double *y, const int32_t *idx,
                                  int64_t n_domain, int32_t n_class, const double *classes_in, const double w[3], double beta, double *prob_out,
                                  double *part_out, void *stream)
{
    int64_t n = 0;
    if (int rc = seg_check_volume(nx, ny, nz, &n)) return rc;
    if (n_domain < 1 || n_domain > n) return fail(MET2_E_INVALID, "the domain's size must lie in 1..n");
    if (!labels || !y || !idx || !w) return fail(MET2_E_INVALID, "NULL argument");
    if (int rc = seg_check_beta(beta)) return rc;
    for (int a = 0; a < 3; ++a)
        if (!(w[a] >= 0.0) || !std::isfinite(w[a])) return fail(MET2_E_INVALID, "an axis weight must be finite and not negative");
    BiasStats h;
    if (int rc = seg_record(n_domain, n_class, classes_in, &h)) return rc;
    SegGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.beta = beta; G.wx = w[0]; G.wy = w[1]; G.wz = w[2];
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const BiasGrid g = bias_grid(n);
    const int np = (int)((n_domain + BIAS_CHUNK - 1) / BIAS_CHUNK);
    DeviceWork W(st);
    const auto part = W.take<double>((size_t)g.nch * 3 * BIAS_MAX_K);
    const auto S = W.take<BiasStats>(1);
    const auto SC = W.take<SegConsts>(1);
    if (!W.alloc()) return W.finish("met2_seg_posterior");
    std::vector<double> hp((size_t)3 * n_class * np);
    W.ok(hipMemcpyAsync(S, &h, sizeof h, hipMemcpyHostToDevice, st));                     // h lives until the wait
    if (W.ok() && prob_out) W.ok(hipMemsetAsync(prob_out, 0, (size_t)n * 8 * n_class, st));
    if (W.ok()) {
        enq_seg_consts(st, S, SC, n_class);
        enq_seg_posterior(st, g, y, idx, labels, S, SC, n_class, G, part, prob_out);
        W.ok(hipGetLastError());
    }
    if (part_out)
        for (int q = 0; q < 3; ++q)
            for (int k = 0; k < n_class && W.ok(); ++k)
                W.ok(hipMemcpyAsync(hp.data() + ((size_t)q * n_class + k) * np, part + (int64_t)(q * BIAS_MAX_K + k) * g.nch, (size_t)np * 8,
                                    hipMemcpyDeviceToHost, st));
    const int rc = W.finish("met2_seg_posterior");
    if (rc != MET2_OK) return rc;
    if (part_out) std::memcpy(part_out, hp.data(), hp.size() * 8);
    return MET2_OK;
}

extern "C" int met2_seg_finish(int32_t device, int64_t n, const uint8_t *labels, const double *prob_raw, int32_t n_class, const double *classes_in,
                               uint8_t *seg, double *prob, double *classes_out, void *stream)
{
    if (n < 1) return fail(MET2_E_INVALID, "the segmentation stages need at least one voxel");
    if (!labels) return fail(MET2_E_INVALID, "NULL argument");
    if (prob && !prob_raw) return fail(MET2_E_INVALID, "prob needs the posteriors it is made from");
    BiasStats h;
    if (int rc = seg_record(1, n_class, classes_in, &h)) return rc;
    if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork W(st);
    const auto S = W.take<BiasStats>(1);
    const auto cd = W.take<double>(3 * BIAS_MAX_K);
    if (!W.alloc()) return W.finish("met2_seg_finish");
    double hc[3 * BIAS_MAX_K];
    if (W.ok(hipMemcpyAsync(S, &h, sizeof h, hipMemcpyHostToDevice, st))) {               // h lives until the wait
        enq_seg_finish(st, bias_grid(n), labels, (const uint8_t *)nullptr, prob_raw, S, n_class, seg, prob, cd);
        W.ok(hipGetLastError());
    }
    if (W.ok()) W.ok(hipMemcpyAsync(hc, cd, (size_t)3 * n_class * 8, hipMemcpyDeviceToHost, st));
    const int rc = W.finish("met2_seg_finish");
    if (rc != MET2_OK) return rc;
    if (classes_out) std::memcpy(classes_out, hc, (size_t)3 * n_class * 8);
    return MET2_OK;
}
