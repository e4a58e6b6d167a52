// bias_common.hpp -- what met2_bias.hip (bias-field correction), met2_seg.hip (tissue segmentation) and met2_pve.hip (partial volume) share: the
// device record, the block scan, the kernels of the domain (log, scan, compact), of the initial classes (stat1, stat2, init) and of the EM step
// (E-step, M-step), and the host code that enqueues them.  The fixed-order sums come from device_helpers.hpp, the work space and the entries'
// common ending from device_work.hpp.  Everything sits in an unnamed namespace: each translation unit compiles its own copy from this one text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_helpers.hpp"
#include "device_work.hpp"

namespace {

#define BIAS_MAX_K 8
#define BIAS_MAX_R 64
#define BIAS_NBINS 256
#define BIAS_CHUNK 1024                   // entries per partial sum: 256 threads x 4
#define BIAS_TA 64                        // samples of a smoothing tile along the axis
#define BIAS_TC 16                        // lines of a smoothing tile
#define BIAS_VAR_FLOOR 1e-6

struct BiasStats {
    int32_t N, degenerate;                // |domain|; N == 0 or hi == lo
    double lo, hi, mean, bmean;
    double mu[BIAS_MAX_K], var[BIAS_MAX_K], pi[BIAS_MAX_K], lc[BIAS_MAX_K];     // lc = log pi - log(var) / 2
    uint32_t hist[BIAS_NBINS];
};

// inclusive scan over the 256 threads; sc: 256 ints of LDS
__device__ __forceinline__ int block_scan(int x, int *sc)
{
    const int t = threadIdx.x;
    __syncthreads();
    sc[t] = x;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int a = t >= d ? sc[t - d] : 0;
        __syncthreads();
        sc[t] += a;
        __syncthreads();
    }
    return sc[t];
}

// the second stage's fixed-order sum of np partials (stride 1), by one workgroup
__device__ __forceinline__ double partial_sum(const double *part, int np, double *red)
{
    double a = 0.0;
    for (int p = threadIdx.x; p < np; p += 256) a += part[p];
    return block_sum(a, red);
}

__global__ __launch_bounds__(256) void bias_log_kernel(const double *__restrict__ v, const uint8_t *__restrict__ mask, int64_t n,
                                                       double *__restrict__ y, uint8_t *__restrict__ dom, int32_t *__restrict__ cnt)
{
    __shared__ int sc[256];
    const int64_t base = (int64_t)blockIdx.x * BIAS_CHUNK + threadIdx.x * 4;
    int c = 0;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = base + j;
        if (i < n) {
            const double val = v[i];
            const bool ok = (!mask || mask[i] != 0) && isfinite(val) && val > 0.0;
            y[i] = ok ? log(val) : 0.0;
            dom[i] = ok ? 1 : 0;
            c += ok ? 1 : 0;
        }
    }
    const int tot = block_scan(c, sc);
    if (threadIdx.x == 255) cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void bias_scan_kernel(const int32_t *__restrict__ cnt, int nchunks, int32_t *__restrict__ off, BiasStats *st)
{
    __shared__ int sc[256];
    int running = 0;
    for (int b0 = 0; b0 < nchunks; b0 += 256) {
        const int p = b0 + threadIdx.x;
        const int x = p < nchunks ? cnt[p] : 0;
        const int inc = block_scan(x, sc);
        if (p < nchunks) off[p] = running + inc - x;
        running += sc[255];
    }
    if (threadIdx.x == 0) st->N = running;
}

__global__ __launch_bounds__(256) void bias_compact_kernel(const uint8_t *__restrict__ dom, int64_t n, const int32_t *__restrict__ off,
                                                           int32_t *__restrict__ idx)
{
    __shared__ int sc[256];
    const int64_t base = (int64_t)blockIdx.x * BIAS_CHUNK + threadIdx.x * 4;
    bool f[4];
    int c = 0;
    for (int j = 0; j < 4; ++j) {
        f[j] = base + j < n && dom[base + j] != 0;
        c += f[j] ? 1 : 0;
    }
    int pos = off[blockIdx.x] + block_scan(c, sc) - c;               // < N <= n: the counts are those bias_log_kernel made from the same flags
    for (int j = 0; j < 4; ++j)
        if (f[j]) idx[pos++] = (int32_t)(base + j);
}

// partials of chunk c of the compacted list: min, max and sum of y
__global__ __launch_bounds__(256) void bias_stat1_kernel(const double *__restrict__ y, const int32_t *__restrict__ idx, const BiasStats *st,
                                                         int pstride, double *__restrict__ part)
{
    __shared__ double red[4];
    const int N = st->N;
    const int64_t c0 = (int64_t)blockIdx.x * BIAS_CHUNK;
    if (c0 >= N) return;
    double mn = INFINITY, mx = -INFINITY, s = 0.0;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < N) {
            const double val = y[idx[i]];
            mn = fmin(mn, val);
            mx = fmax(mx, val);
            s += val;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o));
        mx = fmax(mx, __shfl_xor(mx, o));
    }
    __shared__ double rmn[4], rmx[4];
    if ((threadIdx.x & 63) == 0) { rmn[threadIdx.x >> 6] = mn; rmx[threadIdx.x >> 6] = mx; }
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = fmin(fmin(rmn[0], rmn[1]), fmin(rmn[2], rmn[3]));
        part[pstride + blockIdx.x] = fmax(fmax(rmx[0], rmx[1]), fmax(rmx[2], rmx[3]));
        part[2 * pstride + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void bias_stat1_final(const double *__restrict__ part, int pstride, BiasStats *st)
{
    __shared__ double red[4];
    __shared__ double rmn[256], rmx[256];
    const int N = st->N;
    const int np = (int)(((int64_t)N + BIAS_CHUNK - 1) / BIAS_CHUNK);
    double mn = INFINITY, mx = -INFINITY;
    for (int p = threadIdx.x; p < np; p += 256) {
        mn = fmin(mn, part[p]);
        mx = fmax(mx, part[pstride + p]);
    }
    rmn[threadIdx.x] = mn;
    rmx[threadIdx.x] = mx;
    const double s = partial_sum(part + 2 * pstride, np, red);
    if (threadIdx.x == 0) {
        for (int t = 1; t < 256; ++t) { mn = fmin(mn, rmn[t]); mx = fmax(mx, rmx[t]); }
        const bool deg = N == 0 || mx == mn;
        st->lo = N == 0 ? 0.0 : mn;
        st->hi = N == 0 ? 0.0 : mx;
        st->mean = N == 0 ? 0.0 : s / (double)N;
        st->bmean = 0.0;
        st->degenerate = deg ? 1 : 0;
    }
}

// the histogram of y over [lo, hi] and the partials of sum (y - mean)^2
__global__ __launch_bounds__(256) void bias_stat2_kernel(const double *__restrict__ y, const int32_t *__restrict__ idx, BiasStats *st,
                                                         double *__restrict__ part)
{
    __shared__ double red[4];
    __shared__ uint32_t lh[BIAS_NBINS];
    const int N = st->N;
    const int64_t c0 = (int64_t)blockIdx.x * BIAS_CHUNK;
    if (st->degenerate || c0 >= N) return;
    const double lo = st->lo, hi = st->hi, mean = st->mean;
    lh[threadIdx.x] = 0;
    __syncthreads();
    double ss = 0.0;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < N) {
            const double val = y[idx[i]];
            int bin = (int)floor((val - lo) / (hi - lo) * (double)BIAS_NBINS);
            bin = bin < 0 ? 0 : bin > BIAS_NBINS - 1 ? BIAS_NBINS - 1 : bin;
            atomicAdd(&lh[bin], 1u);
            const double d = val - mean;
            ss += d * d;
        }
    }
    ss = block_sum(ss, red);                                          // its barriers also close the LDS histogram
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
    if (lh[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], lh[threadIdx.x]);
}

__global__ __launch_bounds__(256) void bias_init_kernel(const double *__restrict__ part, BiasStats *st, int K)
{
    __shared__ double red[4];
    const int N = st->N;
    const int np = (int)(((int64_t)N + BIAS_CHUNK - 1) / BIAS_CHUNK);
    const bool deg = st->degenerate != 0;
    const double ss = deg ? 0.0 : partial_sum(part, np, red);        // deg is uniform
    if (threadIdx.x != 0) return;
    const double lo = st->lo, hi = st->hi;
    if (deg) {
        for (int k = 0; k < K; ++k) { st->mu[k] = lo; st->var[k] = 0.0; st->pi[k] = 1.0 / (double)K; st->lc[k] = 0.0; }
        return;
    }
    const double var = ss / (double)N / (double)(K * K);
    const double pi = 1.0 / (double)K;
    uint32_t c = 0;
    int k = 0;
    for (int j = 0; j < BIAS_NBINS && k < K; ++j) {
        c += st->hist[j];
        while (k < K && (double)c >= (double)(2 * k + 1) / (2.0 * (double)K) * (double)N) {
            st->mu[k] = lo + ((double)j + 0.5) * (hi - lo) / (double)BIAS_NBINS;
            st->var[k] = var;
            st->pi[k] = pi;
            st->lc[k] = log(pi) - 0.5 * log(var);
            ++k;
        }
    }
}

// E-step over chunk c of the compacted list.  FINAL = false: the partials of the M-step's 3 K sums, slot k, 8 + k, 16 + k at stride pstride.
// FINAL = true: R and W of the voxel instead.
template <bool FINAL>
__global__ __launch_bounds__(256) void bias_estep_kernel(const double *__restrict__ y, const double *__restrict__ b, const int32_t *__restrict__ idx,
                                                         const BiasStats *__restrict__ st, int K, int pstride, double *__restrict__ part,
                                                         double2 *__restrict__ RW)
{
    __shared__ double red[4];
    const int N = st->N;
    const int64_t c0 = (int64_t)blockIdx.x * BIAS_CHUNK;
    if (st->degenerate || c0 >= N) return;
    double mu[BIAS_MAX_K], var[BIAS_MAX_K], lc[BIAS_MAX_K];
#pragma unroll
    for (int k = 0; k < BIAS_MAX_K; ++k) {
        mu[k] = k < K ? st->mu[k] : 0.0;
        var[k] = k < K ? st->var[k] : 1.0;
        lc[k] = k < K ? st->lc[k] : -INFINITY;
    }
    double s0[BIAS_MAX_K], s1[BIAS_MAX_K], s2[BIAS_MAX_K];
#pragma unroll
    for (int k = 0; k < BIAS_MAX_K; ++k) { s0[k] = 0.0; s1[k] = 0.0; s2[k] = 0.0; }
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < N) {
            const int32_t at = idx[i];
            const double u = y[at] - b[at];
            double l[BIAS_MAX_K], m = -INFINITY;
#pragma unroll
            for (int k = 0; k < BIAS_MAX_K; ++k) {
                const double d = u - mu[k];
                l[k] = lc[k] - d * d / (2.0 * var[k]);                // -inf for a class that is not there or has pi = 0
                m = fmax(m, l[k]);
            }
            double se = 0.0;
#pragma unroll
            for (int k = 0; k < BIAS_MAX_K; ++k) {
                l[k] = k < K ? exp(l[k] - m) : 0.0;
                se += l[k];
            }
            double r = 0.0, w = 0.0;
#pragma unroll
            for (int k = 0; k < BIAS_MAX_K; ++k) {
                if (k < K) {
                    const double p = l[k] / se, d = u - mu[k];
                    if (FINAL) {
                        r += p * d / var[k];
                        w += p / var[k];
                    } else {
                        s0[k] += p;
                        s1[k] += p * u;
                        s2[k] += p * d * d;
                    }
                }
            }
            if (FINAL) RW[at] = make_double2(r, w);
        }
    }
    if (FINAL) return;
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

__global__ __launch_bounds__(256) void bias_mstep_kernel(const double *__restrict__ part, int pstride, BiasStats *st, int K)
{
    __shared__ double red[4];
    if (st->degenerate) return;
    const int N = st->N;
    const int np = (int)(((int64_t)N + BIAS_CHUNK - 1) / BIAS_CHUNK);
    for (int k = 0; k < K; ++k) {
        const double s = partial_sum(part + (int64_t)k * pstride, np, red);
        const double a = partial_sum(part + (int64_t)(BIAS_MAX_K + k) * pstride, np, red);
        const double q = partial_sum(part + (int64_t)(2 * BIAS_MAX_K + k) * pstride, np, red);
        if (threadIdx.x == 0) {
            if (s == 0.0) {                                           // the class keeps its mean and variance and is never seen again
                st->pi[k] = 0.0;
                st->lc[k] = -INFINITY;
            } else {
                const double mo = st->mu[k], mn = a / s, dm = mn - mo;
                const double var = fmax(q / s - dm * dm, BIAS_VAR_FLOOR);
                const double pi = s / (double)N;
                st->mu[k] = mn;
                st->var[k] = var;
                st->pi[k] = pi;
                st->lc[k] = log(pi) - 0.5 * log(var);
            }
        }
    }
}


// lc of classes the host wrote into the record, by bias_mstep_kernel's rule (met2_bias_em only; met2_bias_field never launches it)
__global__ __launch_bounds__(64) void bias_lc_kernel(BiasStats *st, int K)
{
    const int k = threadIdx.x;
    if (k < K) {
        const double pi = st->pi[k], var = st->var[k];
        st->lc[k] = pi == 0.0 ? -INFINITY : log(pi) - 0.5 * log(var);
    }
}

struct BiasGrid {
    int64_t n;                            // voxels
    int nch;                              // chunks of the volume; of the compacted list at most as many
    unsigned nel;                         // workgroups of the per-voxel kernels
};

BiasGrid bias_grid(int64_t n)
{
    BiasGrid g;
    g.n = n;
    g.nch = (int)((n + BIAS_CHUNK - 1) / BIAS_CHUNK);
    g.nel = (unsigned)((n + 255) / 256);
    return g;
}

// y, dom, the chunks' counts and offsets, idx[0..N), S->N
void enq_domain(hipStream_t st, const BiasGrid &g, const double *v, const uint8_t *mask, double *y, uint8_t *dom, int32_t *cnt, int32_t *off,
                int32_t *idx, BiasStats *S)
{
    const dim3 T(256), GC(g.nch), G1(1);
    hipLaunchKernelGGL(bias_log_kernel, GC, T, 0, st, v, mask, g.n, y, dom, cnt);
    hipLaunchKernelGGL(bias_scan_kernel, G1, T, 0, st, cnt, g.nch, off, S);
    hipLaunchKernelGGL(bias_compact_kernel, GC, T, 0, st, dom, g.n, off, idx);
}

// lo, hi, mean, degenerate, the histogram and the initial classes; part[0..np) is left holding the partials of sum (y - mean)^2
void enq_init(hipStream_t st, const BiasGrid &g, const double *y, const int32_t *idx, BiasStats *S, double *part, int K)
{
    const dim3 T(256), GC(g.nch), G1(1);
    hipLaunchKernelGGL(bias_stat1_kernel, GC, T, 0, st, y, idx, S, g.nch, part);
    hipLaunchKernelGGL(bias_stat1_final, G1, T, 0, st, part, g.nch, S);
    hipLaunchKernelGGL(bias_stat2_kernel, GC, T, 0, st, y, idx, S, part);
    hipLaunchKernelGGL(bias_init_kernel, G1, T, 0, st, part, S, K);
}

// one E-step and one M-step; part is left holding the partials of the 3 K sums
void enq_em_step(hipStream_t st, const BiasGrid &g, const double *y, const double *b, const int32_t *idx, BiasStats *S, int K, double *part)
{
    const dim3 T(256), GC(g.nch), G1(1);
    hipLaunchKernelGGL(bias_estep_kernel<false>, GC, T, 0, st, y, b, idx, S, K, g.nch, part, (double2 *)nullptr);
    hipLaunchKernelGGL(bias_mstep_kernel, G1, T, 0, st, part, g.nch, S, K);
}

}  // namespace
