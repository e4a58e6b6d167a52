// group_kernel.hpp -- the statistic kernel of the voxel-wise permutation test, stated once for the two units that launch it: met2_group.hip
// (met2_group_perm_stats: the maximum per candidate and the count per voxel fused in) and met2_tfce.hip (met2_group_perm_tfce: the same t, with
// the same sums in the same order, scattered into dense maps for the spatial statistics).  Also the order-preserving key of a double for
// integer atomic maxima.  Everything sits in an unnamed namespace: each unit compiles its own copy from this one text.
//   gp_stats_kernel<R1, KB, SCATTER>
//                              lanes = voxels: a block owns GP_TILE consecutive voxels, one per thread, for ALL candidates of the launch, so a
//                              voxel's count has one owner and is written once.  The candidates go through in groups of KB: the group's
//                              KB (r + 1) weight rows are staged in LDS transposed to [subject][row], so that for one subject every thread
//                              reads the same consecutive addresses (a broadcast, no bank conflict), and each thread carries KB (r + 1)
//                              running sums in registers while it walks its voxel's column of Y once per group (coalesced over the wave;
//                              the tile's columns stay in cache between groups).  R1 = r + 1 and KB are compile-time, so no register array
//                              is indexed at run time: KB = 8 up to r = 3 (16 .. 32 sums), 4 beyond (20 .. 36 sums).
//                              SCATTER = false: a candidate's maximum: per wave by an xor butterfly of comparisons, the four waves through LDS,
//                              then ONE integer atomic max per (block, candidate) on an order-preserving key, skipped when kmax already holds
//                              as much -- a maximum does not depend on the order, and no floating-point atomic is used.
//                              SCATTER = true: t(k, v) goes to dense[k][at[v]] (a grid of dense_stride voxels per candidate; an index outside
//                              the grid is passed over) and nothing else is written: no maximum, no count.
//   gp_fstats_kernel<R, KB, SCATTER>
//                              the F statistic of an F-contrast (met2_group_perm_fstats, met2_group_perm_ftfce): the same structure with R = r
//                              rows per candidate (no row 0) and both finishes; stated with the kernel below.  KB = 8 up to r = 4, 4 beyond.
//   gp_moments_kernel<R1, KB>  met2_group_perm_vsm's first stage: gp_stats_kernel's sums, with b and the clamped rss scattered in the place of t;
//                              stated with the kernel below.
//   gp_key_kernel              writes the key of -infinity into kmax before, and turns the keys into doubles in place after: no scratch
// A candidate beyond K in the last group has zero weights and is left out of every output; a thread beyond n_vox reads nothing and writes nothing.
// The including unit is compiled without contraction; every loop is bounded by a shape or a compile-time constant.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/met2_hip.h"
#include "device_helpers.hpp"

#pragma clang fp contract(off)

namespace {

#define GP_TILE MET2_GROUP_VOXEL_TILE      // voxels of a block, one per thread
#define GP_WAVES (GP_TILE / 64)

// the bit pattern of a double as an unsigned integer that orders as the values do (-inf lowest, -0 below +0, +inf highest)
__host__ __device__ __forceinline__ unsigned long long gp_key(unsigned long long bits)
{
    return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}
__device__ __forceinline__ unsigned long long gp_unkey(unsigned long long key)
{
    return (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
}

// decode = 0: every key the key of -infinity; decode = 1: every key back to the double it stands for
__global__ void __launch_bounds__(256) gp_key_kernel(int K, unsigned long long *__restrict__ kmax, int decode)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    kmax[k] = decode ? gp_unkey(kmax[k]) : gp_key(0xfff0000000000000ull);
}

template <int R1, int KB, bool SCATTER>
__global__ void __launch_bounds__(GP_TILE) gp_stats_kernel(int n, int64_t n_vox, const double *__restrict__ Y, const double *__restrict__ s0, int K,
                                                           const double *__restrict__ W, int two_sided, const double *__restrict__ t_ref,
                                                           double *__restrict__ t_first, unsigned long long *__restrict__ kmax, uint32_t *__restrict__ count,
                                                           const int32_t *__restrict__ at, int64_t dense_stride, double *__restrict__ dense)
{
    constexpr int ROWS = KB * R1;
    extern __shared__ double gp_lds[];
    double *wt = gp_lds;                                           // [n][ROWS]: the group's weights, subject-major
    double *wmax = gp_lds + (size_t)n * ROWS;                      // [GP_WAVES][KB]: the waves' maxima
    const int64_t v = (int64_t)blockIdx.x * GP_TILE + threadIdx.x;
    const bool live = v < n_vox;
    const double *y = Y + (live ? v : 0);
    const double s = live ? s0[v] : 0.0;
    const double ref = (t_ref && live) ? t_ref[v] : 0.0;
    int64_t cell = -1;                                             // SCATTER: the voxel's place in a dense map
    if constexpr (SCATTER) {
        if (live) cell = at[v];
        if (cell >= dense_stride) cell = -1;
    }
    uint32_t cnt = 0;
    for (int k0 = 0; k0 < K; k0 += KB) {
        __syncthreads();                                           // the previous group's readers of wt and wmax are done
        for (int e = threadIdx.x; e < ROWS * n; e += GP_TILE) {
            const int row = e / n, i = e - row * n;
            wt[i * ROWS + row] = k0 + row / R1 < K ? W[((int64_t)k0 * R1 + row) * n + i] : 0.0;
        }
        __syncthreads();
        double acc[KB][R1];
#pragma unroll
        for (int c = 0; c < KB; ++c)
#pragma unroll
            for (int j = 0; j < R1; ++j) acc[c][j] = 0.0;
        double y_next = live ? y[0] : 0.0;
#pragma unroll 1
        for (int i = 0; i < n; ++i) {                              // not unrolled: a second subject's weights in registers cost a wave per SIMD
            const double yi = y_next;
            y_next = live && i + 1 < n ? y[(int64_t)(i + 1) * n_vox] : 0.0;    // the next subject's value is on its way during this one's sums
            const double *w = wt + i * ROWS;
#pragma unroll
            for (int c = 0; c < KB; ++c)
#pragma unroll
                for (int j = 0; j < R1; ++j) acc[c][j] = rn_add(acc[c][j], rn_mul(w[c * R1 + j], yi));
        }
#pragma unroll
        for (int c = 0; c < KB; ++c) {
            double q = rn_mul(acc[c][1], acc[c][1]);
#pragma unroll
            for (int j = 2; j < R1; ++j) q = rn_add(q, rn_mul(acc[c][j], acc[c][j]));
            const double rss = rn_sub(s, q);
            double t = rss > 0.0 ? acc[c][0] / sqrt(rss) : 0.0;
            if (two_sided) t = fabs(t);
            const bool mine = live && k0 + c < K;
            if constexpr (SCATTER) {
                if (mine && cell >= 0) dense[(int64_t)(k0 + c) * dense_stride + cell] = t;
            } else {
                if (mine) {
                    if (t_ref && t >= ref) ++cnt;
                    if (t_first && k0 + c == 0) t_first[v] = t;
                }
                double m = mine && t == t ? t : -INFINITY;         // a statistic that is not a number is passed over
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double other = __shfl_xor(m, o);
                    if (other > m) m = other;
                }
                if ((threadIdx.x & 63) == 0) wmax[(threadIdx.x >> 6) * KB + c] = m;
            }
        }
        if constexpr (!SCATTER) {
            __syncthreads();
            if ((int)threadIdx.x < KB && k0 + (int)threadIdx.x < K) {
                double m = wmax[threadIdx.x];
#pragma unroll
                for (int wv = 1; wv < GP_WAVES; ++wv)
                    if (wmax[wv * KB + threadIdx.x] > m) m = wmax[wv * KB + threadIdx.x];
                // kmax[k] only grows during the launch, so a block whose maximum does not exceed what it reads there has nothing to add
                const unsigned long long key = gp_key((unsigned long long)__double_as_longlong(m));
                unsigned long long *dst = kmax + k0 + threadIdx.x;
                if (key > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, key);
            }
        }
    }
    if constexpr (!SCATTER)
        if (t_ref && live) count[v] += cnt;                        // this thread owns the voxel
}

template <int R1, bool SCATTER>
void gp_launch(int64_t n_vox, int n, int K, const double *Y, const double *s0, const double *W, int two_sided, const double *t_ref, double *t_first,
               double *kmax, uint32_t *count, const int32_t *at, int64_t dense_stride, double *dense, hipStream_t st)
{
    constexpr int KB = R1 <= 4 ? 8 : 4;
    const size_t lds = ((size_t)n * KB * R1 + GP_WAVES * KB) * sizeof(double);          // <= 128 * 36 * 8 + 256 = 37 120 bytes
    const unsigned blocks = (unsigned)((n_vox + GP_TILE - 1) / GP_TILE);
    hipLaunchKernelGGL((gp_stats_kernel<R1, KB, SCATTER>), dim3(blocks), dim3(GP_TILE), lds, st, n, n_vox, Y, s0, K, W, two_sided, t_ref, t_first,
                       (unsigned long long *)kmax, count, at, dense_stride, dense);
}

// the launch for r = 1 .. MET2_GROUP_MAX_R model columns (the caller has checked the range)
template <bool SCATTER>
void gp_launch_r(int r, int64_t n_vox, int n, int K, const double *Y, const double *s0, const double *W, int two_sided, const double *t_ref,
                 double *t_first, double *kmax, uint32_t *count, const int32_t *at, int64_t dense_stride, double *dense, hipStream_t st)
{
    switch (r) {
#define GP_CASE(R) case R: gp_launch<R + 1, SCATTER>(n_vox, n, K, Y, s0, W, two_sided, t_ref, t_first, kmax, count, at, dense_stride, dense, st); break
        GP_CASE(1); GP_CASE(2); GP_CASE(3); GP_CASE(4); GP_CASE(5); GP_CASE(6); GP_CASE(7); GP_CASE(8);
#undef GP_CASE
    }
}

// The numerator and the clamped residual sum of squares of the pseudo-t (met2_group_perm_vsm): gp_stats_kernel<R1, KB, true>'s text up to rss --
// the same sums in the same order, hence the same bits -- with b = acc[c][0] and rho = rss > 0 ? rss : 0 (an rss that is not a number gives 0)
// written to two dense maps in the place of t.  A sibling, not a third variant of gp_stats_kernel: that kernel's template arguments, and with
// them the names and registers of its instantiations, stay what they were.  Instantiated by met2_group_vsm.hip alone.
template <int R1, int KB>
__global__ void __launch_bounds__(GP_TILE) gp_moments_kernel(int n, int64_t n_vox, const double *__restrict__ Y, const double *__restrict__ s0, int K,
                                                             const double *__restrict__ W, const int32_t *__restrict__ at, int64_t dense_stride,
                                                             double *__restrict__ dense_b, double *__restrict__ dense_rho)
{
    constexpr int ROWS = KB * R1;
    extern __shared__ double gp_lds[];
    double *wt = gp_lds;                                           // [n][ROWS]: the group's weights, subject-major
    const int64_t v = (int64_t)blockIdx.x * GP_TILE + threadIdx.x;
    const bool live = v < n_vox;
    const double *y = Y + (live ? v : 0);
    const double s = live ? s0[v] : 0.0;
    int64_t cell = -1;                                             // the voxel's place in a dense map
    if (live) cell = at[v];
    if (cell >= dense_stride) cell = -1;
    for (int k0 = 0; k0 < K; k0 += KB) {
        __syncthreads();                                           // the previous group's readers of wt are done
        for (int e = threadIdx.x; e < ROWS * n; e += GP_TILE) {
            const int row = e / n, i = e - row * n;
            wt[i * ROWS + row] = k0 + row / R1 < K ? W[((int64_t)k0 * R1 + row) * n + i] : 0.0;
        }
        __syncthreads();
        double acc[KB][R1];
#pragma unroll
        for (int c = 0; c < KB; ++c)
#pragma unroll
            for (int j = 0; j < R1; ++j) acc[c][j] = 0.0;
        double y_next = live ? y[0] : 0.0;
#pragma unroll 1
        for (int i = 0; i < n; ++i) {                              // not unrolled, as in gp_stats_kernel
            const double yi = y_next;
            y_next = live && i + 1 < n ? y[(int64_t)(i + 1) * n_vox] : 0.0;
            const double *w = wt + i * ROWS;
#pragma unroll
            for (int c = 0; c < KB; ++c)
#pragma unroll
                for (int j = 0; j < R1; ++j) acc[c][j] = rn_add(acc[c][j], rn_mul(w[c * R1 + j], yi));
        }
#pragma unroll
        for (int c = 0; c < KB; ++c) {
            double q = rn_mul(acc[c][1], acc[c][1]);
#pragma unroll
            for (int j = 2; j < R1; ++j) q = rn_add(q, rn_mul(acc[c][j], acc[c][j]));
            const double rss = rn_sub(s, q);
            if (live && k0 + c < K && cell >= 0) {
                dense_b[(int64_t)(k0 + c) * dense_stride + cell] = acc[c][0];
                dense_rho[(int64_t)(k0 + c) * dense_stride + cell] = rss > 0.0 ? rss : 0.0;
            }
        }
    }
}

template <int R1>
void gp_moments_launch(int64_t n_vox, int n, int K, const double *Y, const double *s0, const double *W, const int32_t *at, int64_t dense_stride,
                       double *dense_b, double *dense_rho, hipStream_t st)
{
    constexpr int KB = R1 <= 4 ? 8 : 4;                            // gp_launch's groups
    const size_t lds = (size_t)n * KB * R1 * sizeof(double);       // <= 128 * 36 * 8 = 36 864 bytes
    const unsigned blocks = (unsigned)((n_vox + GP_TILE - 1) / GP_TILE);
    hipLaunchKernelGGL((gp_moments_kernel<R1, KB>), dim3(blocks), dim3(GP_TILE), lds, st, n, n_vox, Y, s0, K, W, at, dense_stride, dense_b, dense_rho);
}

// The F statistic over the first s of r orthonormal rows (met2_group_perm_fstats, met2_group_perm_ftfce): gp_stats_kernel's structure with R = r
// rows per candidate (there is no row 0), W [K][R][n].  s and scale are wave-uniform run-time arguments; the prefix qs of the sum of squares is
// taken by a compare on the compile-time row index inside the unrolled loop, so it costs no addition and no register is indexed at run time.
// An rss that is not a number gives an F that is not a number (the maximum passes it over); rss <= 0 gives 0.
template <int R, int KB, bool SCATTER>
__global__ void __launch_bounds__(GP_TILE) gp_fstats_kernel(int n, int64_t n_vox, const double *__restrict__ Y, const double *__restrict__ s0, int K,
                                                            const double *__restrict__ W, int s, double scale, const double *__restrict__ f_ref,
                                                            double *__restrict__ f_first, unsigned long long *__restrict__ kmax,
                                                            uint32_t *__restrict__ count, const int32_t *__restrict__ at, int64_t dense_stride,
                                                            double *__restrict__ dense)
{
    constexpr int ROWS = KB * R;
    extern __shared__ double gp_lds[];
    double *wt = gp_lds;                                           // [n][ROWS]: the group's weights, subject-major
    double *wmax = gp_lds + (size_t)n * ROWS;                      // [GP_WAVES][KB]: the waves' maxima
    const int64_t v = (int64_t)blockIdx.x * GP_TILE + threadIdx.x;
    const bool live = v < n_vox;
    const double *y = Y + (live ? v : 0);
    const double sv = live ? s0[v] : 0.0;
    const double ref = (f_ref && live) ? f_ref[v] : 0.0;
    int64_t cell = -1;                                             // SCATTER: the voxel's place in a dense map
    if constexpr (SCATTER) {
        if (live) cell = at[v];
        if (cell >= dense_stride) cell = -1;
    }
    uint32_t cnt = 0;
    for (int k0 = 0; k0 < K; k0 += KB) {
        __syncthreads();                                           // the previous group's readers of wt and wmax are done
        for (int e = threadIdx.x; e < ROWS * n; e += GP_TILE) {
            const int row = e / n, i = e - row * n;
            wt[i * ROWS + row] = k0 + row / R < K ? W[((int64_t)k0 * R + row) * n + i] : 0.0;
        }
        __syncthreads();
        double acc[KB][R];
#pragma unroll
        for (int c = 0; c < KB; ++c)
#pragma unroll
            for (int j = 0; j < R; ++j) acc[c][j] = 0.0;
        double y_next = live ? y[0] : 0.0;
#pragma unroll 1
        for (int i = 0; i < n; ++i) {                              // not unrolled, as in gp_stats_kernel
            const double yi = y_next;
            y_next = live && i + 1 < n ? y[(int64_t)(i + 1) * n_vox] : 0.0;
            const double *w = wt + i * ROWS;
#pragma unroll
            for (int c = 0; c < KB; ++c)
#pragma unroll
                for (int j = 0; j < R; ++j) acc[c][j] = rn_add(acc[c][j], rn_mul(w[c * R + j], yi));
        }
#pragma unroll
        for (int c = 0; c < KB; ++c) {
            double q = rn_mul(acc[c][0], acc[c][0]);
            double qs = q;                                         // the value q holds after the term j = s (1-based)
#pragma unroll
            for (int j = 1; j < R; ++j) {
                q = rn_add(q, rn_mul(acc[c][j], acc[c][j]));
                if (j < s) qs = q;
            }
            const double rss = rn_sub(sv, q);
            const double num = rn_mul(scale, qs);
            const double f = rss <= 0.0 ? 0.0 : num / rss;
            const bool mine = live && k0 + c < K;
            if constexpr (SCATTER) {
                if (mine && cell >= 0) dense[(int64_t)(k0 + c) * dense_stride + cell] = f;
            } else {
                if (mine) {
                    if (f_ref && f >= ref) ++cnt;
                    if (f_first && k0 + c == 0) f_first[v] = f;
                }
                double m = mine && f == f ? f : -INFINITY;         // a statistic that is not a number is passed over
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double other = __shfl_xor(m, o);
                    if (other > m) m = other;
                }
                if ((threadIdx.x & 63) == 0) wmax[(threadIdx.x >> 6) * KB + c] = m;
            }
        }
        if constexpr (!SCATTER) {
            __syncthreads();
            if ((int)threadIdx.x < KB && k0 + (int)threadIdx.x < K) {
                double m = wmax[threadIdx.x];
#pragma unroll
                for (int wv = 1; wv < GP_WAVES; ++wv)
                    if (wmax[wv * KB + threadIdx.x] > m) m = wmax[wv * KB + threadIdx.x];
                const unsigned long long key = gp_key((unsigned long long)__double_as_longlong(m));
                unsigned long long *dst = kmax + k0 + threadIdx.x;
                if (key > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, key);
            }
        }
    }
    if constexpr (!SCATTER)
        if (f_ref && live) count[v] += cnt;                        // this thread owns the voxel
}

#define GP_F_KB(R) ((R) <= 4 ? 8 : 4)      // candidates per group of the F kernel: 8 .. 32 sums up to r = 4, 20 .. 32 beyond (tests stand on it)

template <int R, bool SCATTER>
void gp_flaunch(int64_t n_vox, int n, int K, const double *Y, const double *s0, const double *W, int s, double scale, const double *f_ref,
                double *f_first, double *kmax, uint32_t *count, const int32_t *at, int64_t dense_stride, double *dense, hipStream_t st)
{
    constexpr int KB = GP_F_KB(R);
    const size_t lds = ((size_t)n * KB * R + GP_WAVES * KB) * sizeof(double);           // <= 128 * 32 * 8 + 256 = 33 024 bytes
    const unsigned blocks = (unsigned)((n_vox + GP_TILE - 1) / GP_TILE);
    hipLaunchKernelGGL((gp_fstats_kernel<R, KB, SCATTER>), dim3(blocks), dim3(GP_TILE), lds, st, n, n_vox, Y, s0, K, W, s, scale, f_ref, f_first,
                       (unsigned long long *)kmax, count, at, dense_stride, dense);
}

// the F launch for r = 1 .. MET2_GROUP_MAX_R model columns (the caller has checked the range, and 1 <= s <= r)
template <bool SCATTER>
void gp_flaunch_r(int r, int64_t n_vox, int n, int K, const double *Y, const double *s0, const double *W, int s, double scale, const double *f_ref,
                  double *f_first, double *kmax, uint32_t *count, const int32_t *at, int64_t dense_stride, double *dense, hipStream_t st)
{
    switch (r) {
#define GP_CASE(R) case R: gp_flaunch<R, SCATTER>(n_vox, n, K, Y, s0, W, s, scale, f_ref, f_first, kmax, count, at, dense_stride, dense, st); break
        GP_CASE(1); GP_CASE(2); GP_CASE(3); GP_CASE(4); GP_CASE(5); GP_CASE(6); GP_CASE(7); GP_CASE(8);
#undef GP_CASE
    }
}

}  // namespace
