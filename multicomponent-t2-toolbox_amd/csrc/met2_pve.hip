// met2_pve.hip -- met2_partial_volume: partial-volume tissue maps of a segmented 3-D map (segment='pve'; fast's _pve_k, _pveseg and _mixeltype of
// step 5 of the reference's example pipeline).  The mixel model of Santago & Gage (IEEE TMI 12:566-574, 1993) as Shattuck
// et al. (NeuroImage 13:856-876, 2001) and Tohka et al. (NeuroImage 23:84-97, 2004) use it: every voxel is pure tissue or a mixture of two
// rank-adjacent tissues, the mixtures' likelihood is the pure Gaussians' marginalised over a uniform fraction, a Potts-like prior over the six
// face neighbours couples the types, and the fraction of a mixed voxel is Tohka's closed form.  include/met2_hip.h states the algorithm; no
// program text of FSL was used.  The list of the domain is made by bias_common.hpp's scan and compaction.  New here:
//   pve_count_kernel      the chunks' counts of seg != 0
//   pve_moment_kernel<P>  the partials of sum p_k and sum p_k v (P = 0), of sum (p_k d) d (P = 1), in bias_estep_kernel's layout
//   pve_mean_kernel       s_k, mu_k;  pve_var_kernel  var_k, pi_k
//   pve_consts_kernel     the live flags, a_k, h_k and the node table [K - 1][64][3]
//   pve_energy_kernel     E [T][n] and the first types: one thread per voxel of the list, the node table in LDS
//   pve_icm_kernel<C>     one colour pass of a checkerboard sweep, on seg_icm_kernel's tile of 4 x 8 x 16 types with its halo in LDS
//   pve_finish_kernel     pve, pveseg, mixeltype, classes_lin
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

#define PVE_TX 4                          // the tile of pve_icm_kernel: seg_icm_kernel's, 4 x 8 x 16 voxels, 256 z-adjacent pairs
#define PVE_TY 8
#define PVE_TZ 16
#define PVE_LZ (PVE_TZ + 2)               // its extents in LDS, with the halo
#define PVE_LY (PVE_TY + 2)
#define PVE_LX (PVE_TX + 2)
#define PVE_OFF 255                       // the type of a voxel off the domain
#define PVE_NA 64                         // midpoint nodes of a mixture
#define PVE_MAX_T (2 * BIAS_MAX_K - 1)    // 15 types
#define PVE_TAB (PVE_NA * 3)              // doubles of one mixture's table: m, a, h per node

struct PveRec {
    double s[BIAS_MAX_K], mu[BIAS_MAX_K], var[BIAS_MAX_K], pi[BIAS_MAX_K];      // the moments in linear intensity
    double a[BIAS_MAX_K], h[BIAS_MAX_K];
    int32_t live[PVE_MAX_T + 1];          // per type; [15] = the number of live types
    double tab[(BIAS_MAX_K - 1) * PVE_TAB];
};

struct PveGeom {
    int nx, ny, nz;
    double beta, wx, wy, wz;
};

// ((v - m)^2 a) + h
__device__ __forceinline__ double pve_term(double v, double m, double a, double h)
{
    const double d = rn_sub(v, m);
    return rn_add(rn_mul(rn_mul(d, d), a), h);
}

__global__ __launch_bounds__(256) void pve_count_kernel(const uint8_t *__restrict__ seg, int64_t n, int32_t *__restrict__ cnt)
{
    __shared__ int sc[256];
    const int64_t base = (int64_t)blockIdx.x * BIAS_CHUNK + threadIdx.x * 4;
    int c = 0;
    for (int j = 0; j < 4; ++j)
        if (base + j < n && seg[base + j] != 0) ++c;
    const int tot = block_scan(c, sc);
    if (threadIdx.x == 255) cnt[blockIdx.x] = tot;
}

// Chunk c of the list.  PASS 0: slot k and 8 + k at stride pstride get the chunk's sums of p_k and p_k v; PASS 1: slot 16 + k that of
// (p_k d) d, d = v - mu_k.  Every term is rounded operation by operation; the sums are block_sum's fixed tree.
template <int PASS>
__global__ __launch_bounds__(256) void pve_moment_kernel(const double *__restrict__ v, const double *__restrict__ prob,
                                                         const int32_t *__restrict__ idx, const BiasStats *__restrict__ st,
                                                         const PveRec *__restrict__ R, int K, int64_t n, int pstride, double *__restrict__ part)
{
    __shared__ double red[4];
    const int N = st->N;
    const int64_t c0 = (int64_t)blockIdx.x * BIAS_CHUNK;
    if (c0 >= N) return;
    double mu[BIAS_MAX_K], s0[BIAS_MAX_K], s1[BIAS_MAX_K];
#pragma unroll
    for (int k = 0; k < BIAS_MAX_K; ++k) {
        mu[k] = PASS == 1 && k < K ? R->mu[k] : 0.0;
        s0[k] = 0.0;
        s1[k] = 0.0;
    }
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < N) {
            const int32_t at = idx[i];
            const double u = v[at];
#pragma unroll
            for (int k = 0; k < BIAS_MAX_K; ++k) {
                if (k < K) {
                    const double p = prob[(int64_t)k * n + at];
                    if (PASS == 0) {
                        s0[k] = rn_add(s0[k], p);
                        s1[k] = rn_add(s1[k], rn_mul(p, u));
                    } else {
                        const double d = rn_sub(u, mu[k]);
                        s0[k] = rn_add(s0[k], rn_mul(rn_mul(p, d), d));
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < BIAS_MAX_K; ++k) {
        if (k < K) {                                                  // uniform
            const double a0 = block_sum(s0[k], red);
            if (PASS == 0) {
                const double a1 = block_sum(s1[k], red);
                if (threadIdx.x == 0) {
                    part[(int64_t)k * pstride + blockIdx.x] = a0;
                    part[(int64_t)(BIAS_MAX_K + k) * pstride + blockIdx.x] = a1;
                }
            } else if (threadIdx.x == 0) {
                part[(int64_t)(2 * BIAS_MAX_K + k) * pstride + blockIdx.x] = a0;
            }
        }
    }
}

// s_k and mu_k = (sum p_k v) / s_k; a class without weight gets mu_k = 0
__global__ __launch_bounds__(256) void pve_mean_kernel(const double *__restrict__ part, int pstride, const BiasStats *__restrict__ st, PveRec *R,
                                                       int K)
{
    __shared__ double red[4];
    const int N = st->N;
    const int np = (int)(((int64_t)N + BIAS_CHUNK - 1) / BIAS_CHUNK);
    for (int k = 0; k < K; ++k) {
        const double s = partial_sum(part + (int64_t)k * pstride, np, red);
        const double a = partial_sum(part + (int64_t)(BIAS_MAX_K + k) * pstride, np, red);
        if (threadIdx.x == 0) {
            R->s[k] = s;
            R->mu[k] = s == 0.0 ? 0.0 : a / s;
        }
    }
}

// var_k = (sum (p_k d) d) / s_k and pi_k = s_k / N; a class without weight gets var_k = 0 and pi_k = 0
__global__ __launch_bounds__(256) void pve_var_kernel(const double *__restrict__ part, int pstride, const BiasStats *__restrict__ st, PveRec *R,
                                                      int K)
{
    __shared__ double red[4];
    const int N = st->N;
    const int np = (int)(((int64_t)N + BIAS_CHUNK - 1) / BIAS_CHUNK);
    for (int k = 0; k < K; ++k) {
        const double q = partial_sum(part + (int64_t)(2 * BIAS_MAX_K + k) * pstride, np, red);
        if (threadIdx.x == 0) {
            const double s = R->s[k];
            R->var[k] = s == 0.0 ? 0.0 : q / s;
            R->pi[k] = s == 0.0 ? 0.0 : s / (double)N;
        }
    }
}

// Step 3 from mu, var, pi of the record.  Thread m makes node m of every mixture; alpha_m, 1 - alpha_m and their squares are exact.
__global__ __launch_bounds__(64) void pve_consts_kernel(PveRec *R, int K)
{
    __shared__ int lv[BIAS_MAX_K];
    const int t = threadIdx.x;
    if (t < BIAS_MAX_K) {
        const bool in = t < K;
        const double var = in ? R->var[t] : 0.0;
        const bool live = in && R->pi[t] != 0.0 && isfinite(var) && var > 0.0;
        R->a[t] = live ? 1.0 / (2.0 * var) : 0.0;                     // 2 var is exact: one rounding
        R->h[t] = live ? 0.5 * log(var) : 0.0;
        lv[t] = live ? 1 : 0;
        if (in) R->live[t] = lv[t];
    }
    __syncthreads();
    const double al = ((double)t + 0.5) / (double)PVE_NA, be = 1.0 - al;
    int nlive = 0;
    for (int k = 0; k < K; ++k) nlive += lv[k];
    for (int j = 0; j + 1 < K; ++j) {
        const double m0 = R->mu[j], m1 = R->mu[j + 1];
        const bool live = lv[j] && lv[j + 1] && rn_sub(m1, m0) > 0.0;
        const double m = rn_add(rn_mul(al, m0), rn_mul(be, m1));
        const double s = rn_add(rn_mul(rn_mul(al, al), R->var[j]), rn_mul(rn_mul(be, be), R->var[j + 1]));
        double *tb = R->tab + j * PVE_TAB + 3 * t;
        tb[0] = live ? m : 0.0;
        tb[1] = live ? 1.0 / (2.0 * s) : 0.0;
        tb[2] = live ? 0.5 * log(s) : 0.0;
        if (t == 0) R->live[K + j] = live ? 1 : 0;
        nlive += live ? 1 : 0;
    }
    if (t >= 2 * K - 1 && t < PVE_MAX_T) R->live[t] = 0;
    if (t == 0) R->live[PVE_MAX_T] = nlive;
}

// Steps 4 and 5 for entry i of the list: E_t of its voxel at [t n + voxel] and its first type.  The mixtures' tables sit in LDS; every lane
// reads the same node at the same time (a broadcast).  Two passes over the nodes: the minimum, then the sum of exp(q* - q_m), m ascending.
__global__ __launch_bounds__(256) void pve_energy_kernel(const double *__restrict__ v, const uint8_t *__restrict__ seg,
                                                         const int32_t *__restrict__ idx, const BiasStats *__restrict__ st,
                                                         const PveRec *__restrict__ R, int K, int64_t n, double *__restrict__ E,
                                                         uint8_t *__restrict__ typ)
{
    __shared__ double tab[(BIAS_MAX_K - 1) * PVE_TAB];
    __shared__ double cmu[BIAS_MAX_K], ca[BIAS_MAX_K], ch[BIAS_MAX_K];
    __shared__ int clive[PVE_MAX_T + 1];
    const int N = st->N;
    const int t = threadIdx.x;
    if ((int64_t)blockIdx.x * 256 >= N) return;                       // uniform
    for (int e = t; e < (K - 1) * PVE_TAB; e += 256) tab[e] = R->tab[e];
    if (t < BIAS_MAX_K) {
        cmu[t] = R->mu[t];
        ca[t] = R->a[t];
        ch[t] = R->h[t];
    }
    if (t <= PVE_MAX_T) clive[t] = R->live[t];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + t;
    if (i >= N) return;
    const int32_t at = idx[i];
    const double u = v[at];
    int best = -1;
    double be = INFINITY;
    for (int k = 0; k < K; ++k) {
        const bool live = clive[k] != 0;                              // uniform
        const double e = live ? pve_term(u, cmu[k], ca[k], ch[k]) : INFINITY;
        E[(int64_t)k * n + at] = e;
        if (live && (best < 0 || e < be)) { best = k; be = e; }
    }
    for (int j = 0; j + 1 < K; ++j) {
        const bool live = clive[K + j] != 0;                          // uniform
        double e = INFINITY;
        if (live) {
            const double *tb = tab + j * PVE_TAB;
            double qs = INFINITY;
            for (int m = 0; m < PVE_NA; ++m) qs = fmin(qs, pve_term(u, tb[3 * m], tb[3 * m + 1], tb[3 * m + 2]));
            double S = 0.0;
            for (int m = 0; m < PVE_NA; ++m) S = rn_add(S, exp(rn_sub(qs, pve_term(u, tb[3 * m], tb[3 * m + 1], tb[3 * m + 2]))));
            e = rn_sub(qs, log(rn_mul(S, 1.0 / (double)PVE_NA)));     // S / 64 is exact
        }
        E[(int64_t)(K + j) * n + at] = e;
        if (live && (best < 0 || e < be)) { best = K + j; be = e; }
    }
    if (typ) typ[at] = best >= 0 ? (uint8_t)best : (uint8_t)(seg[at] - 1);
}

// delta2 of step 6 between a neighbour's type nb and type t with member set mt; msk: the member sets of the types, in LDS
__device__ __forceinline__ int pve_delta2(int nb, int t, int mt, const int *msk)
{
    if (nb == PVE_OFF || nb == t) return 0;
    return (msk[nb & 15] & mt) != 0 ? 1 : 2;
}

// One colour pass: seg_icm_kernel's tiling and ownership.  Tiles are numbered along blockIdx.x, z fastest; thread t owns the voxels
// z0 + 2 (t & 7) and the next of line (x0 + (t >> 6), y0 + ((t >> 3) & 7)) and updates the one with (x + y + z) & 1 == COLOUR, whose six
// neighbours have the other colour, which no thread of this launch writes.
template <int COLOUR>
__global__ __launch_bounds__(256) void pve_icm_kernel(uint8_t *__restrict__ typ, const double *__restrict__ E, const PveRec *__restrict__ R, int K,
                                                      int64_t n, PveGeom G)
{
    __shared__ uint8_t tile[PVE_LX * PVE_LY * PVE_LZ];
    __shared__ int clive[PVE_MAX_T + 1], cmsk[PVE_MAX_T + 1];
    const int t = threadIdx.x;
    const int T = 2 * K - 1;
    const int ntz = (G.nz + PVE_TZ - 1) / PVE_TZ, nty = (G.ny + PVE_TY - 1) / PVE_TY;
    int bid = blockIdx.x;
    const int z0 = (bid % ntz) * PVE_TZ;
    bid /= ntz;
    const int y0 = (bid % nty) * PVE_TY, x0 = (bid / nty) * PVE_TX;
    if (t <= PVE_MAX_T) {
        clive[t] = t < T ? R->live[t] : 0;
        cmsk[t] = t < K ? 1 << t : t < T ? 3 << (t - K) : 0;
    }
    for (int e = t; e < PVE_LX * PVE_LY * PVE_LZ; e += 256) {
        const int gz = z0 - 1 + e % PVE_LZ, gy = y0 - 1 + (e / PVE_LZ) % PVE_LY, gx = x0 - 1 + e / (PVE_LZ * PVE_LY);
        const bool in = gx >= 0 && gx < G.nx && gy >= 0 && gy < G.ny && gz >= 0 && gz < G.nz;
        tile[e] = in ? typ[((int64_t)gx * G.ny + gy) * G.nz + gz] : (uint8_t)PVE_OFF;
    }
    __syncthreads();
    const int tx = t >> 6, ty = (t >> 3) & 7;
    const int gx = x0 + tx, gy = y0 + ty;
    const int tz = 2 * (t & 7) + ((COLOUR + gx + gy + z0) & 1);
    const int gz = z0 + tz;
    if (gx >= G.nx || gy >= G.ny || gz >= G.nz) return;
    const uint8_t *c = tile + ((tx + 1) * PVE_LY + (ty + 1)) * PVE_LZ + (tz + 1);
    if (c[0] == PVE_OFF) return;
    const int xm = c[-PVE_LY * PVE_LZ], xp = c[PVE_LY * PVE_LZ], ym = c[-PVE_LZ], yp = c[PVE_LZ], zm = c[-1], zp = c[1];
    const int64_t at = ((int64_t)gx * G.ny + gy) * G.nz + gz;
    int best = -1;
    double be = INFINITY;
    for (int u = 0; u < T; ++u) {
        if (!clive[u]) continue;                                      // uniform
        const int mt = cmsk[u];
        const int cx = pve_delta2(xm, u, mt, cmsk) + pve_delta2(xp, u, mt, cmsk), cy = pve_delta2(ym, u, mt, cmsk) + pve_delta2(yp, u, mt, cmsk),
                  cz = pve_delta2(zm, u, mt, cmsk) + pve_delta2(zp, u, mt, cmsk);
        const double p = rn_mul(rn_mul(G.beta, rn_add(rn_add(rn_mul(G.wx, (double)cx), rn_mul(G.wy, (double)cy)), rn_mul(G.wz, (double)cz))), 0.5);
        const double e = rn_add(E[(int64_t)u * n + at], p);
        if (best < 0 || e < be) { best = u; be = e; }
    }
    if (best >= 0) typ[at] = (uint8_t)best;                           // no live type: the voxel keeps what it has
}

// Step 7.  A type that is none of 0..T-1 counts as off the domain.  Each output may be NULL.
__global__ __launch_bounds__(256) void pve_finish_kernel(const double *__restrict__ v, const uint8_t *__restrict__ typ,
                                                         const PveRec *__restrict__ R, int K, int64_t n, double *__restrict__ pve,
                                                         uint8_t *__restrict__ pveseg, uint8_t *__restrict__ mixel, double *__restrict__ classes)
{
    __shared__ double cmu[BIAS_MAX_K];
    if (threadIdx.x < BIAS_MAX_K) {
        const int k = threadIdx.x;
        cmu[k] = k < K ? R->mu[k] : 0.0;
        if (classes && blockIdx.x == 0 && k < K) {
            classes[k] = R->mu[k];
            classes[K + k] = R->var[k];
            classes[2 * K + k] = R->pi[k];
        }
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int t = typ[i];
    const bool on = t < 2 * K - 1;
    int k0 = -1, lab = 0;                                             // pve_{k0} = f0, pve_{k0 + 1} = f1
    double f0 = 0.0, f1 = 0.0;
    if (on && t < K) {
        k0 = t;
        f0 = 1.0;
        lab = t + 1;
    } else if (on) {
        k0 = t - K;
        const double m0 = cmu[k0], m1 = cmu[k0 + 1];
        const double al = fmin(fmax(rn_sub(m1, v[i]) / rn_sub(m1, m0), 0.0), 1.0);
        f0 = al;
        f1 = rn_sub(1.0, al);
        lab = f0 >= f1 ? k0 + 1 : k0 + 2;                             // ties to the lowest class
    }
    if (pve)
        for (int k = 0; k < K; ++k) pve[(int64_t)k * n + i] = k == k0 ? f0 : k == k0 + 1 && k0 >= 0 ? f1 : 0.0;
    if (pveseg) pveseg[i] = (uint8_t)lab;
    if (mixel) mixel[i] = on ? (uint8_t)t : (uint8_t)PVE_OFF;
}

// ---- the host code of the stages: each enqueues its launches on st and reads nothing back.  met2_partial_volume and the stage entries below
// ---- run these helpers and launch no kernel of the partial-volume stage otherwise.

PveGeom pve_geom(int nx, int ny, int nz, const double voxel_mm[3], double beta)
{
    const double dmin = std::fmin(voxel_mm[0], std::fmin(voxel_mm[1], voxel_mm[2]));
    PveGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz;
    G.beta = beta;
    G.wx = dmin / voxel_mm[0]; G.wy = dmin / voxel_mm[1]; G.wz = dmin / voxel_mm[2];
    return G;
}

// the list of seg != 0: the chunks' counts and offsets, idx[0..N), S->N
void enq_pve_domain(hipStream_t st, const BiasGrid &g, const uint8_t *seg, int32_t *cnt, int32_t *off, int32_t *idx, BiasStats *S)
{
    const dim3 T(256), GC(g.nch), G1(1);
    hipLaunchKernelGGL(pve_count_kernel, GC, T, 0, st, seg, g.n, cnt);
    hipLaunchKernelGGL(bias_scan_kernel, G1, T, 0, st, cnt, g.nch, off, S);
    hipLaunchKernelGGL(bias_compact_kernel, GC, T, 0, st, seg, g.n, off, idx);
}

// step 1; part is left holding the partials of the 3 K sums
void enq_pve_moments(hipStream_t st, const BiasGrid &g, const double *v, const double *prob, const int32_t *idx, const BiasStats *S, PveRec *R,
                     int K, double *part)
{
    const dim3 T(256), GC(g.nch), G1(1);
    hipLaunchKernelGGL(pve_moment_kernel<0>, GC, T, 0, st, v, prob, idx, S, R, K, g.n, g.nch, part);
    hipLaunchKernelGGL(pve_mean_kernel, G1, T, 0, st, part, g.nch, S, R, K);
    hipLaunchKernelGGL(pve_moment_kernel<1>, GC, T, 0, st, v, prob, idx, S, R, K, g.n, g.nch, part);
    hipLaunchKernelGGL(pve_var_kernel, G1, T, 0, st, part, g.nch, S, R, K);
}

void enq_pve_consts(hipStream_t st, PveRec *R, int K) { hipLaunchKernelGGL(pve_consts_kernel, dim3(1), dim3(64), 0, st, R, K); }

// typ (NULL allowed) = PVE_OFF everywhere, then E and the first types on the list
hipError_t enq_pve_energy(hipStream_t st, const BiasGrid &g, const double *v, const uint8_t *seg, const int32_t *idx, const BiasStats *S,
                          const PveRec *R, int K, double *E, uint8_t *typ)
{
    if (typ) {
        const hipError_t e = hipMemsetAsync(typ, PVE_OFF, (size_t)g.n, st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(pve_energy_kernel, dim3(g.nel), dim3(256), 0, st, v, seg, idx, S, R, K, g.n, E, typ);
    return hipSuccess;
}

void enq_pve_pass(hipStream_t st, int colour, uint8_t *typ, const double *E, const PveRec *R, int K, const PveGeom &G)
{
    const int64_t tiles = (int64_t)((G.nx + PVE_TX - 1) / PVE_TX) * ((G.ny + PVE_TY - 1) / PVE_TY) * ((G.nz + PVE_TZ - 1) / PVE_TZ);   // <= n
    const int64_t n = (int64_t)G.nx * G.ny * G.nz;
    if (colour == 0)
        hipLaunchKernelGGL(pve_icm_kernel<0>, dim3((unsigned)tiles), dim3(256), 0, st, typ, E, R, K, n, G);
    else
        hipLaunchKernelGGL(pve_icm_kernel<1>, dim3((unsigned)tiles), dim3(256), 0, st, typ, E, R, K, n, G);
}

void enq_pve_icm(hipStream_t st, int n_sweeps, uint8_t *typ, const double *E, const PveRec *R, int K, const PveGeom &G)
{
    for (int s = 0; s < n_sweeps; ++s) {
        enq_pve_pass(st, 0, typ, E, R, K, G);
        enq_pve_pass(st, 1, typ, E, R, K, G);
    }
}

void enq_pve_finish(hipStream_t st, const BiasGrid &g, const double *v, const uint8_t *typ, const PveRec *R, int K, double *pve, uint8_t *pveseg,
                    uint8_t *mixel, double *classes)
{
    hipLaunchKernelGGL(pve_finish_kernel, dim3(g.nel), dim3(256), 0, st, v, typ, R, K, g.n, pve, pveseg, mixel, classes);
}

int pve_check_beta(double beta)
{
    if (!(beta >= 0.0) || !std::isfinite(beta)) return fail(MET2_E_INVALID, "beta_pv must be finite and not negative");
    return MET2_OK;
}

// what every stage entry checks first: a voxel, no NULL among the pointers it needs (ok), 1 <= K <= 8, fewer than 2^31 voxels
int pve_check_stage(int64_t n, bool ok, int n_class)
{
    if (n < 1) return fail(MET2_E_INVALID, "the partial-volume stages need at least one voxel");
    if (n_class < 1) return fail(MET2_E_INVALID, "the partial-volume model needs at least one class");
    if (!ok) return fail(MET2_E_INVALID, "NULL argument");
    if (n_class > BIAS_MAX_K) return fail(MET2_E_UNSUPPORTED, "the partial-volume model supports at most 8 classes");
    if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    return MET2_OK;
}

// the stage entries' record from the caller's classes [3 K] = mu, var, pi in linear intensity (any values: a class may be dead)
void pve_record(int K, const double *classes_in, PveRec *h)
{
    std::memset(h, 0, sizeof *h);
    for (int k = 0; k < K; ++k) { h->mu[k] = classes_in[k]; h->var[k] = classes_in[K + k]; h->pi[k] = classes_in[2 * K + k]; }
}

}  // namespace

extern "C" int met2_partial_volume(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const uint8_t *seg, const double *prob,
                                   const double voxel_mm[3], int32_t n_class, double beta_pv, int32_t n_icm, double *pve, uint8_t *pveseg,
                                   uint8_t *mixeltype, double *classes_lin, void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0) return fail(MET2_E_INVALID, "bad shape");
    if (n_class < 1) return fail(MET2_E_INVALID, "the partial-volume model needs at least one class");
    if (n_icm < 0) return fail(MET2_E_INVALID, "n_icm must not be negative");
    if (!voxel_mm) return fail(MET2_E_INVALID, "NULL voxel size");
    for (int a = 0; a < 3; ++a)
        if (!(voxel_mm[a] > 0.0) || !std::isfinite(voxel_mm[a])) return fail(MET2_E_INVALID, "the voxel size must be positive and finite");
    if (int rc = pve_check_beta(beta_pv)) return rc;
    const int64_t n = (int64_t)nx * ny * nz;
    if (n == 0) return MET2_OK;
    if (!v || !seg || !prob) return fail(MET2_E_INVALID, "NULL argument");
    if (n_class > BIAS_MAX_K) return fail(MET2_E_UNSUPPORTED, "the partial-volume model supports at most 8 classes");
    if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    const int K = n_class, T = 2 * K - 1;
    const PveGeom G = pve_geom(nx, ny, nz, voxel_mm, beta_pv);
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;

    const BiasGrid g = bias_grid(n);
    DeviceWork W(st);
    const auto E = W.take<double>((size_t)n * T);
    const auto idx = W.take<int32_t>(n);
    const auto typ = W.take<uint8_t>(n);
    const auto cnt = W.take<int32_t>(g.nch), off = W.take<int32_t>(g.nch);
    const auto part = W.take<double>((size_t)g.nch * 3 * BIAS_MAX_K);
    const auto S = W.take<BiasStats>(1);
    const auto R = W.take<PveRec>(1);
    if (!W.alloc()) return W.finish("met2_partial_volume");

    enq_pve_domain(st, g, seg, cnt, off, idx, S);
    enq_pve_moments(st, g, v, prob, idx, S, R, K, part);
    enq_pve_consts(st, R, K);
    if (W.ok(hipGetLastError()) && W.ok(enq_pve_energy(st, g, v, seg, idx, S, R, K, E, typ))) {
        enq_pve_icm(st, n_icm, typ, E, R, K, G);
        if (pve || pveseg || mixeltype || classes_lin) enq_pve_finish(st, g, v, typ, R, K, pve, pveseg, mixeltype, classes_lin);
    }
    return W.finish("met2_partial_volume");
}

// ---- the stages one by one, for tests and diagnostics (include/met2_hip.h) ----

extern "C" int met2_pve_moments(int32_t device, int64_t n, const double *v, const uint8_t *seg, const double *prob, int32_t n_class,
                                int64_t *n_domain, double *part_out, double *classes_out, void *stream)
{
    if (int rc = pve_check_stage(n, v && seg && prob, n_class)) return rc;
    const int K = n_class;
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const BiasGrid g = bias_grid(n);
    DeviceWork W(st);
    const auto idx = W.take<int32_t>(n), cnt = W.take<int32_t>(g.nch), off = W.take<int32_t>(g.nch);
    const auto part = W.take<double>((size_t)g.nch * 3 * BIAS_MAX_K);
    const auto S = W.take<BiasStats>(1);
    const auto R = W.take<PveRec>(1);
    if (!W.alloc()) return W.finish("met2_pve_moments");
    BiasStats hs;
    PveRec hr;
    std::vector<double> hp((size_t)3 * BIAS_MAX_K * g.nch);
    enq_pve_domain(st, g, seg, cnt, off, idx, S);
    enq_pve_moments(st, g, v, prob, idx, S, R, K, part);
    W.ok(hipGetLastError());
    if (W.ok()) W.ok(hipMemcpyAsync(&hs, S, sizeof hs, hipMemcpyDeviceToHost, st));
    if (W.ok()) W.ok(hipMemcpyAsync(&hr, R, sizeof hr, hipMemcpyDeviceToHost, st));
    if (W.ok()) W.ok(hipMemcpyAsync(hp.data(), part, hp.size() * 8, hipMemcpyDeviceToHost, st));
    const int rc = W.finish("met2_pve_moments");
    if (rc != MET2_OK) return rc;
    const int64_t N = hs.N, np = (N + BIAS_CHUNK - 1) / BIAS_CHUNK;   // a chunk past np was never written
    if (n_domain) *n_domain = N;
    if (part_out)
        for (int q = 0; q < 3; ++q)
            for (int k = 0; k < K; ++k)
                for (int64_t c = 0; c < np; ++c) part_out[((int64_t)q * K + k) * g.nch + c] = hp[(size_t)(q * BIAS_MAX_K + k) * g.nch + c];
    if (classes_out)
        for (int k = 0; k < K; ++k) { classes_out[k] = hr.mu[k]; classes_out[K + k] = hr.var[k]; classes_out[2 * K + k] = hr.pi[k]; }
    return MET2_OK;
}

extern "C" int met2_pve_consts(int32_t device, int32_t n_class, const double *classes_in, double *a_out, double *h_out, int32_t *live_out,
                               double *table_out, void *stream)
{
    if (int rc = pve_check_stage(1, classes_in != nullptr, n_class)) return rc;
    const int K = n_class;
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork W(st);
    const auto R = W.take<PveRec>(1);
    if (!W.alloc()) return W.finish("met2_pve_consts");
    std::vector<PveRec> h(2);                                          // [0] in, [1] out; alive until the wait
    pve_record(K, classes_in, &h[0]);
    if (W.ok(hipMemcpyAsync(R, &h[0], sizeof(PveRec), hipMemcpyHostToDevice, st))) {
        enq_pve_consts(st, R, K);
        W.ok(hipGetLastError());
    }
    if (W.ok()) W.ok(hipMemcpyAsync(&h[1], R, sizeof(PveRec), hipMemcpyDeviceToHost, st));
    const int rc = W.finish("met2_pve_consts");
    if (rc != MET2_OK) return rc;
    for (int k = 0; k < K; ++k) {
        if (a_out) a_out[k] = h[1].a[k];
        if (h_out) h_out[k] = h[1].h[k];
    }
    if (live_out)
        for (int t = 0; t < 2 * K - 1; ++t) live_out[t] = h[1].live[t];
    if (table_out) std::memcpy(table_out, h[1].tab, (size_t)(K - 1) * PVE_TAB * 8);
    return MET2_OK;
}

extern "C" int met2_pve_energy(int32_t device, int64_t n, const double *v, const uint8_t *seg, int32_t n_class, const double *classes_in,
                               double *E_out, uint8_t *types_out, void *stream)
{
    if (int rc = pve_check_stage(n, v && seg && E_out && classes_in, n_class)) return rc;
    const int K = n_class;
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const BiasGrid g = bias_grid(n);
    DeviceWork W(st);
    const auto idx = W.take<int32_t>(n), cnt = W.take<int32_t>(g.nch), off = W.take<int32_t>(g.nch);
    const auto S = W.take<BiasStats>(1);
    const auto R = W.take<PveRec>(1);
    if (!W.alloc()) return W.finish("met2_pve_energy");
    std::vector<PveRec> h(1);                                          // alive until the wait
    pve_record(K, classes_in, &h[0]);
    W.ok(hipMemcpyAsync(R, &h[0], sizeof(PveRec), hipMemcpyHostToDevice, st));
    if (W.ok() && W.ok(hipMemsetAsync(E_out, 0, (size_t)n * 8 * (2 * K - 1), st))) {
        enq_pve_domain(st, g, seg, cnt, off, idx, S);
        enq_pve_consts(st, R, K);
        W.ok(hipGetLastError());
    }
    if (W.ok()) W.ok(enq_pve_energy(st, g, v, seg, idx, S, R, K, E_out, types_out));
    return W.finish("met2_pve_energy");
}

extern "C" int met2_pve_icm(int32_t device, int32_t nx, int32_t ny, int32_t nz, uint8_t *types, const double *E, int32_t n_class,
                            const int32_t *live_in, const double w[3], double beta_pv, int32_t n_sweeps, int32_t colour, void *stream)
{
    if (nx < 1 || ny < 1 || nz < 1) return fail(MET2_E_INVALID, "the partial-volume stages need at least one voxel");
    if (int rc = pve_check_stage((int64_t)nx * ny * nz, types && E && w && live_in, n_class)) return rc;
    if (n_sweeps < 0) return fail(MET2_E_INVALID, "n_sweeps must not be negative");
    if (colour < -1 || colour > 1) return fail(MET2_E_INVALID, "colour must be 0, 1 or -1 for both");
    if (int rc = pve_check_beta(beta_pv)) return rc;
    for (int a = 0; a < 3; ++a)
        if (!(w[a] >= 0.0) || !std::isfinite(w[a])) return fail(MET2_E_INVALID, "an axis weight must be finite and not negative");
    const int K = n_class;
    PveGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.beta = beta_pv; G.wx = w[0]; G.wy = w[1]; G.wz = w[2];
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork W(st);
    const auto R = W.take<PveRec>(1);
    if (!W.alloc()) return W.finish("met2_pve_icm");
    std::vector<PveRec> h(1);                                          // alive until the wait
    std::memset(&h[0], 0, sizeof(PveRec));
    for (int t = 0; t < 2 * K - 1; ++t) {
        h[0].live[t] = live_in[t] != 0 ? 1 : 0;
        h[0].live[PVE_MAX_T] += h[0].live[t];
    }
    if (W.ok(hipMemcpyAsync(R, &h[0], sizeof(PveRec), hipMemcpyHostToDevice, st))) {
        if (colour < 0)
            enq_pve_icm(st, n_sweeps, types, E, R, K, G);
        else if (n_sweeps > 0)
            enq_pve_pass(st, colour, types, E, R, K, G);
    }
    return W.finish("met2_pve_icm");
}

extern "C" int met2_pve_finish(int32_t device, int64_t n, const double *v, const uint8_t *types, int32_t n_class, const double *classes_in,
                               double *pve, uint8_t *pveseg, uint8_t *mixeltype, void *stream)
{
    if (int rc = pve_check_stage(n, v && types && classes_in, n_class)) return rc;
    const int K = n_class;
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork W(st);
    const auto R = W.take<PveRec>(1);
    if (!W.alloc()) return W.finish("met2_pve_finish");
    std::vector<PveRec> h(1);                                          // alive until the wait
    pve_record(K, classes_in, &h[0]);
    if (W.ok(hipMemcpyAsync(R, &h[0], sizeof(PveRec), hipMemcpyHostToDevice, st)))
        enq_pve_finish(st, bias_grid(n), v, types, R, K, pve, pveseg, mixeltype, (double *)nullptr);
    return W.finish("met2_pve_finish");
}
