// met2_warp.hip -- met2_warp, met2_warp_labels, met2_warp_compose, met2_warp_max_norm2, met2_warp_lncc (and its stage entries
// met2_warp_lncc_sums, met2_warp_lncc_force, met2_warp_work_bytes), met2_warp_invert_step, met2_warp_jacobian: resampling through a
// displacement field, the device stages of a greedy deformable registration with the squared local normalised cross-correlation, and the
// step of a field's fixed-point inverse with its Jacobian determinant (include/met2_hip.h states the contract; warp.py holds the loops).
// Written from that statement and from Avants et al. (Med. Image Anal. 12:26-41, 2008), whose centre-voxel force this is.
//   wp_voxel_kernel<ORDER, V>  met2_resample's rs_voxel_kernel with a field: one destination voxel per thread, threads along the destination's
//                              z; p = x + u(x) (one rounding per axis), then rs_coord, the inside test and the taps of resample_taps.hpp
//                              (rs_taps_at), then a loop over the series.  A zero field gives met2_resample's bits.
//   wp_compose_kernel          one destination voxel per thread: s from the device scalar, w = s v, the clamped coordinates, the three
//                              channels of the source field through one set of order-1 taps
//   wp_max_norm2_kernel        max |v|^2: per thread, per block (a tree in LDS), then ONE integer atomic max per block on the bit pattern of the
//                              non-negative double -- a max does not depend on the order, and no floating-point atomic is used
//   wp_invert_step_kernel      wp_compose_kernel's shape for one step of the fixed-point inverse: p = y + v_in(y), the coordinates before the clamp
//                              give `inside`, the three channels of the source field through one set of order-1 taps, a 3 x 3 product, and the
//                              largest squared change fused in (wp_max_norm2_kernel's tree and integer atomic max): a pass of its own would
//                              read both fields again.  Chen et al., Med. Phys. 35:81-88, 2008 is the iteration; warp.py holds the loop
//   wp_jacobian_kernel         one voxel per thread, threads along z: the six face neighbours' three channels straight from memory (the z
//                              neighbours are the wave's own lines, the x and y neighbours whole coalesced lines that L2 keeps between the
//                              blocks that share them; no LDS tile), the determinant along the first row, and the count of voxels whose
//                              determinant is not > 0 by a tree of integers and ONE integer atomic add per block
//   wp_box_line_kernel<R, FIRST>  the box sums along x or y, the volume seen as [outer][n][inner], lanes along `inner` (which ends in z, the
//                              contiguous axis): a thread owns WP_SEG consecutive outputs of one line and slides a window of 2 R + 1 values
//                              through registers, so it reads every input of its segment once (and 2 R of its neighbours'), coalesced over
//                              the wave, and every output is the direct sum of the window, left to right.  The shifts are unrolled: no
//                              register array is indexed at run time.  FIRST forms the channels from fixed, warped and inside on the way
//                              (three windows: m, mF, mW; the products are taken at the sum); the later pass runs one channel at a time.
//   wp_box_z_kernel<R>         the box sums along z, where the lines themselves are contiguous: 256 consecutive elements and R on either
//                              side go through LDS once (coalesced), every thread sums its 2 R + 1 from there; blockIdx.y is the channel
//   wp_force_kernel            one voxel per thread: the rule of the header from the six sums, the gradient of the warped image from its
//                              face neighbours, and the block's share of (sum cc, n valid) by a tree in LDS; wp_metric_kernel adds the
//                              blocks' shares in one block, in a fixed order
// A term of a window that lies beyond the volume is 0.0 and is added like the others: x + 0.0 = x, so the value is that of the clipped sum.
// The file is compiled without contraction; every loop is bounded by a shape or a compile-time constant.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_work.hpp"

#pragma clang fp contract(off)

#include "resample_taps.hpp"
#include "resample_checks.hpp"

namespace {

#define WP_SEG 16                          // wp_box_line_kernel: outputs of a line per thread
#define WP_Z_TILE 256                      // wp_box_z_kernel: elements of a tile (= the block)
#define WP_FORCE_GRID 1024                 // wp_force_kernel: blocks at the most; their shares are added by wp_metric_kernel
#define WP_INVERSE_GRID 2048               // wp_invert_step_kernel, wp_jacobian_kernel: blocks at the most, one atomic each

template <int ORDER, typename V>
__global__ void __launch_bounds__(RS_BLOCK) wp_voxel_kernel(RsGeom G, int n_series, const V *__restrict__ src, int64_t svs, int64_t sss,
                                                            const double *__restrict__ disp, V fill, V *__restrict__ dst, int64_t dvs, int64_t dss,
                                                            uint8_t *__restrict__ inside)
{
    const int64_t n_dst = (int64_t)G.mx * G.my * G.mz;
    for (int64_t w = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; w < n_dst; w += (int64_t)gridDim.x * RS_BLOCK) {
        int i, j, k;
        rs_split(w, G, i, j, k);
        const double *u = disp + 3 * w;
        const double px = rn_add((double)i, u[0]), py = rn_add((double)j, u[1]), pz = rn_add((double)k, u[2]);
        const double cx = rs_coord(G.A, px, py, pz), cy = rs_coord(G.A + 4, px, py, pz), cz = rs_coord(G.A + 8, px, py, pz);
        RsTaps<ORDER> T;
        const bool in = rs_taps_at<ORDER>(G, cx, cy, cz, T);
        if (inside) inside[w] = in ? 1 : 0;
        V *d = dst + w * dvs;
        if (in)
            for (int s = 0; s < n_series; ++s) d[s * dss] = rs_value<ORDER, V>(T, src + s * sss, svs);
        else
            for (int s = 0; s < n_series; ++s) d[s * dss] = fill;
    }
}

// a coordinate into 0 .. n - 1; one that is not a number goes to 0
__device__ __forceinline__ double wp_clamp(double c, int n)
{
    const double hi = (double)(n - 1);
    return !(c >= 0.0) ? 0.0 : (c > hi ? hi : c);
}

struct WpGain { double g[3]; };

__global__ void __launch_bounds__(RS_BLOCK) wp_compose_kernel(RsGeom G, WpGain gain, const double *__restrict__ u_src, const double *__restrict__ v, double step,
                                                              const double *__restrict__ vmax2, double *__restrict__ out)
{
    const int64_t n_dst = (int64_t)G.mx * G.my * G.mz;
    double s = step;
    if (vmax2) {
        const double m2 = *vmax2;
        s = m2 > 0.0 ? step / sqrt(m2) : 0.0;
    }
    for (int64_t w = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; w < n_dst; w += (int64_t)gridDim.x * RS_BLOCK) {
        int i, j, k;
        rs_split(w, G, i, j, k);
        double wx = 0.0, wy = 0.0, wz = 0.0;
        if (v) {
            wx = rn_mul(s, v[3 * w]);
            wy = rn_mul(s, v[3 * w + 1]);
            wz = rn_mul(s, v[3 * w + 2]);
        }
        const double px = rn_add((double)i, wx), py = rn_add((double)j, wy), pz = rn_add((double)k, wz);
        const double cx = wp_clamp(rs_coord(G.A, px, py, pz), G.nx), cy = wp_clamp(rs_coord(G.A + 4, px, py, pz), G.ny),
                     cz = wp_clamp(rs_coord(G.A + 8, px, py, pz), G.nz);
        RsTaps<1> T;
        (void)rs_taps_at<1>(G, cx, cy, cz, T);                     // always inside after the clamp
        out[3 * w] = rn_add(wx, rn_mul(gain.g[0], rs_value<1, double>(T, u_src, 3)));
        out[3 * w + 1] = rn_add(wy, rn_mul(gain.g[1], rs_value<1, double>(T, u_src + 1, 3)));
        out[3 * w + 2] = rn_add(wz, rn_mul(gain.g[2], rs_value<1, double>(T, u_src + 2, 3)));
    }
}

__global__ void __launch_bounds__(RS_BLOCK) wp_max_norm2_kernel(int64_t n, const double *__restrict__ v, unsigned long long *__restrict__ out)
{
    __shared__ double sh[RS_BLOCK];
    double mx = 0.0;
    for (int64_t w = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; w < n; w += (int64_t)gridDim.x * RS_BLOCK) {
        const double a = v[3 * w], b = v[3 * w + 1], c = v[3 * w + 2];
        const double q = rn_add(rn_add(rn_mul(a, a), rn_mul(b, b)), rn_mul(c, c));
        if (q > mx) mx = q;                                        // a norm that is not a number is passed over
    }
    sh[threadIdx.x] = mx;
    __syncthreads();
    for (int s = RS_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && sh[threadIdx.x + s] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(out, (unsigned long long)__double_as_longlong(sh[0]));   // >= 0: the bit patterns order as the values do
}

struct WpMat3 { double n[9]; };

// (N[a][0] x + N[a][1] y) + N[a][2] z
__device__ __forceinline__ double wp_row3(const double *row, double x, double y, double z)
{
    return rn_add(rn_add(rn_mul(row[0], x), rn_mul(row[1], y)), rn_mul(row[2], z));
}

__global__ void __launch_bounds__(RS_BLOCK) wp_invert_step_kernel(RsGeom G, WpMat3 N, const double *__restrict__ u_src, const double *__restrict__ v_in,
                                                                  double *__restrict__ v_out, uint8_t *__restrict__ inside, unsigned long long *__restrict__ res2)
{
    __shared__ double sh[RS_BLOCK];
    const int64_t n_dst = (int64_t)G.mx * G.my * G.mz;
    double mx = 0.0;
    for (int64_t w = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; w < n_dst; w += (int64_t)gridDim.x * RS_BLOCK) {
        int i, j, k;
        rs_split(w, G, i, j, k);
        double ax = 0.0, ay = 0.0, az = 0.0;
        if (v_in) {
            ax = v_in[3 * w];
            ay = v_in[3 * w + 1];
            az = v_in[3 * w + 2];
        }
        const double px = rn_add((double)i, ax), py = rn_add((double)j, ay), pz = rn_add((double)k, az);
        const double rx = rs_coord(G.A, px, py, pz), ry = rs_coord(G.A + 4, px, py, pz), rz = rs_coord(G.A + 8, px, py, pz);
        if (inside) inside[w] = rs_inside(rx, G.nx) && rs_inside(ry, G.ny) && rs_inside(rz, G.nz) ? 1 : 0;
        RsTaps<1> T;
        (void)rs_taps_at<1>(G, wp_clamp(rx, G.nx), wp_clamp(ry, G.ny), wp_clamp(rz, G.nz), T);     // always inside after the clamp
        const double tx = rs_value<1, double>(T, u_src, 3), ty = rs_value<1, double>(T, u_src + 1, 3), tz = rs_value<1, double>(T, u_src + 2, 3);
        const double ox = wp_row3(N.n, tx, ty, tz), oy = wp_row3(N.n + 3, tx, ty, tz), oz = wp_row3(N.n + 6, tx, ty, tz);
        v_out[3 * w] = ox;
        v_out[3 * w + 1] = oy;
        v_out[3 * w + 2] = oz;
        const double dx = rn_sub(ox, ax), dy = rn_sub(oy, ay), dz = rn_sub(oz, az);
        const double q = rn_add(rn_add(rn_mul(dx, dx), rn_mul(dy, dy)), rn_mul(dz, dz));
        if (q > mx) mx = q;                                        // a change that is not a number is passed over
    }
    if (!res2) return;                                             // the same for every thread of the launch
    sh[threadIdx.x] = mx;
    __syncthreads();
    for (int s = RS_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && sh[threadIdx.x + s] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // *res2 only grows during the launch, so a block whose maximum does not exceed what it reads there (0 is what the entry wrote) has
        // nothing to add: the atomics on the one address, which the memory side takes one after the other, fall from one per block to a few
        const unsigned long long m = (unsigned long long)__double_as_longlong(sh[0]);                      // >= 0: the bit patterns order as the values do
        if (m > __hip_atomic_load(res2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(res2, m);
    }
}

// D_b of the three channels at voxel e, which has the index `at` of `n` along an axis of `stride` voxels: the neighbours are taken at
// lo = max(at - 1, 0) and hi = min(at + 1, n - 1), so the difference is the central one where hi - lo = 2 and the one-sided one at a rim
__device__ __forceinline__ void wp_diff3(const double *__restrict__ u, int64_t e, int at, int n, int64_t stride, double *d)
{
    const int lo = at > 0 ? -1 : 0, hi = at < n - 1 ? 1 : 0;
    if (hi == lo) {                                                // an axis of length 1
        d[0] = d[1] = d[2] = 0.0;
        return;
    }
    const double *a = u + 3 * (e + hi * stride), *b = u + 3 * (e + lo * stride);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double df = rn_sub(a[c], b[c]);
        d[c] = hi - lo == 2 ? df / 2.0 : df;
    }
}

__global__ void __launch_bounds__(RS_BLOCK) wp_jacobian_kernel(int nx, int ny, int nz, const double *__restrict__ u, double scale, double *__restrict__ det,
                                                               unsigned long long *__restrict__ n_nonpositive)
{
    __shared__ int sh[RS_BLOCK];
    const int64_t nvox = (int64_t)nx * ny * nz;
    int cnt = 0;                                                   // a thread sees at most 2^31 / 256 voxels
    for (int64_t e = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; e < nvox; e += (int64_t)gridDim.x * RS_BLOCK) {
        const int z = (int)(e % nz);
        const int64_t rest = e / nz;
        const int y = (int)(rest % ny), x = (int)(rest / ny);
        double dx[3], dy[3], dz[3];                                // d?[a] = D_? u_a
        wp_diff3(u, e, x, nx, (int64_t)ny * nz, dx);
        wp_diff3(u, e, y, ny, nz, dy);
        wp_diff3(u, e, z, nz, 1, dz);
        const double j00 = rn_add(1.0, dx[0]), j01 = dy[0], j02 = dz[0];
        const double j10 = dx[1], j11 = rn_add(1.0, dy[1]), j12 = dz[1];
        const double j20 = dx[2], j21 = dy[2], j22 = rn_add(1.0, dz[2]);
        const double m0 = rn_sub(rn_mul(j11, j22), rn_mul(j12, j21)), m1 = rn_sub(rn_mul(j10, j22), rn_mul(j12, j20)),
                     m2 = rn_sub(rn_mul(j10, j21), rn_mul(j11, j20));
        const double d = rn_mul(scale, rn_add(rn_sub(rn_mul(j00, m0), rn_mul(j01, m1)), rn_mul(j02, m2)));
        det[e] = d;
        if (!(d > 0.0)) ++cnt;
    }
    if (!n_nonpositive) return;                                    // the same for every thread of the launch
    sh[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = RS_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0] > 0) atomicAdd(n_nonpositive, (unsigned long long)sh[0]);
}

// window <- window shifted by one, `x` coming in at the far end
template <int R>
__device__ __forceinline__ void wp_shift(double (&w)[2 * R + 1], double x)
{
#pragma unroll
    for (int q = 0; q < 2 * R; ++q) w[q] = w[q + 1];
    w[2 * R] = x;
}

template <int R, bool FIRST>
__global__ void __launch_bounds__(RS_BLOCK) wp_box_line_kernel(int64_t outer, int n, int64_t inner, int64_t nvox, const double *__restrict__ F,
                                                               const double *__restrict__ W, const uint8_t *__restrict__ m, const double *__restrict__ in,
                                                               double *__restrict__ out)
{
    const int nseg = (n + WP_SEG - 1) / WP_SEG;
    const int64_t items = outer * nseg * inner;
    for (int64_t item = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; item < items; item += (int64_t)gridDim.x * RS_BLOCK) {
        const int64_t r = item % inner, t = item / inner;
        const int sg = (int)(t % nseg);
        const int64_t base = (t / nseg) * n * inner + r;
        const int i0 = sg * WP_SEG, i1 = min(n, i0 + WP_SEG);
        if constexpr (FIRST) {
            double wm[2 * R + 1], wf[2 * R + 1], ww[2 * R + 1];
#pragma unroll
            for (int q = 0; q < 2 * R + 1; ++q) wm[q] = wf[q] = ww[q] = 0.0;
            // before the step of output i the windows hold the samples i - R - 1 .. i + R - 1
#pragma unroll
            for (int q = 1; q < 2 * R + 1; ++q) {
                const int e = i0 - R - 1 + q;
                if (e >= 0 && e < n) {
                    const int64_t g = base + e * inner;
                    const bool on = m[g] != 0;
                    wm[q] = on ? 1.0 : 0.0;
                    wf[q] = on ? F[g] : 0.0;
                    ww[q] = on ? W[g] : 0.0;
                }
            }
#pragma unroll 1
            for (int i = i0; i < i1; ++i) {
                const int e = i + R;
                double xm = 0.0, xf = 0.0, xw = 0.0;
                if (e < n) {
                    const int64_t g = base + e * inner;
                    const bool on = m[g] != 0;
                    xm = on ? 1.0 : 0.0;
                    xf = on ? F[g] : 0.0;
                    xw = on ? W[g] : 0.0;
                }
                wp_shift<R>(wm, xm);
                wp_shift<R>(wf, xf);
                wp_shift<R>(ww, xw);
                double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0;
#pragma unroll
                for (int q = 0; q < 2 * R + 1; ++q) {
                    s0 = rn_add(s0, wm[q]);
                    s1 = rn_add(s1, wf[q]);
                    s2 = rn_add(s2, ww[q]);
                    s3 = rn_add(s3, rn_mul(wf[q], wf[q]));
                    s4 = rn_add(s4, rn_mul(ww[q], ww[q]));
                    s5 = rn_add(s5, rn_mul(wf[q], ww[q]));
                }
                const int64_t g = base + i * inner;
                out[g] = s0;
                out[nvox + g] = s1;
                out[2 * nvox + g] = s2;
                out[3 * nvox + g] = s3;
                out[4 * nvox + g] = s4;
                out[5 * nvox + g] = s5;
            }
        } else {
#pragma unroll 1
            for (int c = 0; c < 6; ++c) {
                const double *src = in + c * nvox + base;
                double *dst = out + c * nvox + base;
                double w[2 * R + 1];
                w[0] = 0.0;
#pragma unroll
                for (int q = 1; q < 2 * R + 1; ++q) {
                    const int e = i0 - R - 1 + q;
                    w[q] = e >= 0 && e < n ? src[e * inner] : 0.0;
                }
#pragma unroll 1
                for (int i = i0; i < i1; ++i) {
                    const int e = i + R;
                    wp_shift<R>(w, e < n ? src[e * inner] : 0.0);
                    double s = 0.0;
#pragma unroll
                    for (int q = 0; q < 2 * R + 1; ++q) s = rn_add(s, w[q]);
                    dst[i * inner] = s;
                }
            }
        }
    }
}

template <int R>
__global__ void __launch_bounds__(WP_Z_TILE) wp_box_z_kernel(int64_t nvox, int nz, const double *__restrict__ in, double *__restrict__ out)
{
    __shared__ double tile[WP_Z_TILE + 2 * R];
    const double *src = in + blockIdx.y * nvox;
    double *dst = out + blockIdx.y * nvox;
    const int64_t n_tiles = (nvox + WP_Z_TILE - 1) / WP_Z_TILE;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t e0 = t * WP_Z_TILE;
        for (int j = threadIdx.x; j < WP_Z_TILE + 2 * R; j += WP_Z_TILE) {
            const int64_t g = e0 - R + j;
            tile[j] = g >= 0 && g < nvox ? src[g] : 0.0;
        }
        __syncthreads();
        const int64_t e = e0 + threadIdx.x;
        if (e < nvox) {
            const int z = (int)(e % nz);
            double s = 0.0;
#pragma unroll
            for (int q = -R; q <= R; ++q) s = rn_add(s, z + q >= 0 && z + q < nz ? tile[(int)threadIdx.x + R + q] : 0.0);
            dst[e] = s;
        }
        __syncthreads();
    }
}

// the neighbour of voxel e at distance `stride` along an axis on which it has the index `at` of `n`: its warped value where it is in the grid
// and inside, the centre voxel's otherwise
__device__ __forceinline__ double wp_neighbour(const double *__restrict__ W, const uint8_t *__restrict__ m, int64_t e, int at, int n, int64_t stride, int dir,
                                               double centre)
{
    const int p = at + dir;
    if (p < 0 || p >= n) return centre;
    const int64_t g = e + dir * stride;
    return m[g] ? W[g] : centre;
}

__global__ void __launch_bounds__(RS_BLOCK) wp_force_kernel(int nx, int ny, int nz, const double *__restrict__ F, const double *__restrict__ W,
                                                            const uint8_t *__restrict__ m, const double *__restrict__ sums, double eps,
                                                            double *__restrict__ force, double *__restrict__ partial)
{
    __shared__ double sh_cc[RS_BLOCK], sh_n[RS_BLOCK];
    const int64_t nvox = (int64_t)nx * ny * nz;
    double acc = 0.0, cnt = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; e < nvox; e += (int64_t)gridDim.x * RS_BLOCK) {
        const int z = (int)(e % nz);
        const int64_t rest = e / nz;
        const int y = (int)(rest % ny), x = (int)(rest / ny);
        double fx = 0.0, fy = 0.0, fz = 0.0;
        if (m[e]) {
            const double n = sums[e], sF = sums[nvox + e], sW = sums[2 * nvox + e], sFF = sums[3 * nvox + e], sWW = sums[4 * nvox + e],
                         sFW = sums[5 * nvox + e];
            if (n >= 2.0) {
                const double A = rn_sub(sFW, rn_mul(sF, sW) / n), B = rn_sub(sFF, rn_mul(sF, sF) / n), C = rn_sub(sWW, rn_mul(sW, sW) / n);
                if (B > eps && C > eps) {
                    const double BC = rn_mul(B, C), w0 = W[e];
                    acc = rn_add(acc, rn_mul(A, A) / BC);
                    cnt += 1.0;
                    const double f = rn_mul(rn_mul(2.0, A) / BC, rn_sub(rn_sub(F[e], sF / n), rn_mul(A / C, rn_sub(w0, sW / n))));
                    fx = rn_mul(f, rn_sub(wp_neighbour(W, m, e, x, nx, (int64_t)ny * nz, 1, w0), wp_neighbour(W, m, e, x, nx, (int64_t)ny * nz, -1, w0)) / 2.0);
                    fy = rn_mul(f, rn_sub(wp_neighbour(W, m, e, y, ny, nz, 1, w0), wp_neighbour(W, m, e, y, ny, nz, -1, w0)) / 2.0);
                    fz = rn_mul(f, rn_sub(wp_neighbour(W, m, e, z, nz, 1, 1, w0), wp_neighbour(W, m, e, z, nz, 1, -1, w0)) / 2.0);
                }
            }
        }
        force[3 * e] = fx;
        force[3 * e + 1] = fy;
        force[3 * e + 2] = fz;
    }
    sh_cc[threadIdx.x] = acc;
    sh_n[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = RS_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh_cc[threadIdx.x] = rn_add(sh_cc[threadIdx.x], sh_cc[threadIdx.x + s]);
            sh_n[threadIdx.x] = rn_add(sh_n[threadIdx.x], sh_n[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = sh_cc[0];
        partial[2 * blockIdx.x + 1] = sh_n[0];
    }
}

// metric[0..1] = the blocks' shares added up: thread t takes blocks t, t + 256, ... in that order, then the tree
__global__ void __launch_bounds__(RS_BLOCK) wp_metric_kernel(int n_blocks, const double *__restrict__ partial, double *__restrict__ metric)
{
    __shared__ double sh_cc[RS_BLOCK], sh_n[RS_BLOCK];
    double acc = 0.0, cnt = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += RS_BLOCK) {
        acc = rn_add(acc, partial[2 * b]);
        cnt = rn_add(cnt, partial[2 * b + 1]);
    }
    sh_cc[threadIdx.x] = acc;
    sh_n[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = RS_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh_cc[threadIdx.x] = rn_add(sh_cc[threadIdx.x], sh_cc[threadIdx.x + s]);
            sh_n[threadIdx.x] = rn_add(sh_n[threadIdx.x], sh_n[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        metric[0] = sh_cc[0];
        metric[1] = sh_n[0];
    }
}

// both grids of a warp obey the source limits of met2_resample: the field lives on the destination
int wp_check_dims(const int32_t *d, const char *what)
{
    int rc = rs_check_dims(d, what, false);
    if (rc) return rc;
    for (int a = 0; a < 3; ++a)
        if (d[a] > MET2_RESAMPLE_MAX_AXIS) return fail(MET2_E_UNSUPPORTED, std::string("a ") + what + " axis holds more than 512 voxels");
    return MET2_OK;
}

int wp_check_lncc(const int32_t *dims, int32_t radius, double eps)
{
    int rc = wp_check_dims(dims, "volume");
    if (rc) return rc;
    if (radius < 1 || radius > MET2_WARP_MAX_RADIUS) return fail(MET2_E_INVALID, "the radius must lie in 1 .. 4");
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(MET2_E_INVALID, "eps must be finite and not negative");
    return MET2_OK;
}

int wp_force_grid(int64_t nvox) { return (int)std::max<int64_t>(1, std::min<int64_t>((nvox + RS_BLOCK - 1) / RS_BLOCK, WP_FORCE_GRID)); }

template <int R>
hipError_t wp_sums_launch_r(const int32_t *d, const double *F, const double *W, const uint8_t *m, double *sums, double *tmp, hipStream_t st)
{
    const int nx = d[0], ny = d[1], nz = d[2];
    const int64_t nvox = (int64_t)nx * ny * nz, inner_x = (int64_t)ny * nz;
    const int seg_x = (nx + WP_SEG - 1) / WP_SEG, seg_y = (ny + WP_SEG - 1) / WP_SEG;
    // x: the inputs -> sums; y: sums -> tmp; z: tmp -> sums
    hipLaunchKernelGGL((wp_box_line_kernel<R, true>), dim3(rs_grid(seg_x * inner_x, RS_BLOCK)), dim3(RS_BLOCK), 0, st, (int64_t)1, nx, inner_x, nvox, F, W, m,
                       (const double *)nullptr, sums);
    hipLaunchKernelGGL((wp_box_line_kernel<R, false>), dim3(rs_grid((int64_t)nx * seg_y * nz, RS_BLOCK)), dim3(RS_BLOCK), 0, st, (int64_t)nx, ny, (int64_t)nz,
                       nvox, (const double *)nullptr, (const double *)nullptr, (const uint8_t *)nullptr, (const double *)sums, tmp);
    hipLaunchKernelGGL(wp_box_z_kernel<R>, dim3(rs_grid(nvox, WP_Z_TILE), 6), dim3(WP_Z_TILE), 0, st, nvox, nz, (const double *)tmp, sums);
    return hipGetLastError();
}

hipError_t wp_sums_launch(const int32_t *d, int radius, const double *F, const double *W, const uint8_t *m, double *sums, double *tmp, hipStream_t st)
{
    switch (radius) {
    case 1: return wp_sums_launch_r<1>(d, F, W, m, sums, tmp, st);
    case 2: return wp_sums_launch_r<2>(d, F, W, m, sums, tmp, st);
    case 3: return wp_sums_launch_r<3>(d, F, W, m, sums, tmp, st);
    default: return wp_sums_launch_r<4>(d, F, W, m, sums, tmp, st);
    }
}

hipError_t wp_force_launch(const int32_t *d, const double *F, const double *W, const uint8_t *m, const double *sums, double eps, double *force,
                           double *metric, double *partial, hipStream_t st)
{
    const int grid = wp_force_grid((int64_t)d[0] * d[1] * d[2]);
    hipLaunchKernelGGL(wp_force_kernel, dim3(grid), dim3(RS_BLOCK), 0, st, d[0], d[1], d[2], F, W, m, sums, eps, force, partial);
    hipLaunchKernelGGL(wp_metric_kernel, dim3(1), dim3(RS_BLOCK), 0, st, grid, (const double *)partial, metric);
    return hipGetLastError();
}

// the bytes of the pieces an entry takes, in DeviceWork's layout: `sums_volumes` blocks of six summed volumes, then (force) the blocks' shares
size_t wp_work_need(const int32_t *d, int sums_volumes, bool force)
{
    DeviceWork L(nullptr);
    size_t end = 0;
    for (int b = 0; b < sums_volumes; ++b) {
        const auto p = L.take<double>((size_t)6 * d[0] * d[1] * d[2]);
        end = p.off + p.bytes;
    }
    if (force) {
        const auto p = L.take<double>(2 * WP_FORCE_GRID);
        end = p.off + p.bytes;
    }
    return end;
}

// the caller's block must hold what the entry takes
int wp_check_work(const void *work, int64_t work_bytes, size_t need)
{
    if (work && (work_bytes < 0 || (uint64_t)work_bytes < need))
        return fail(MET2_E_INVALID, "the work block is smaller than the " + std::to_string(need) + " bytes this call takes (met2_warp_work_bytes)");
    return MET2_OK;
}

}  // namespace

extern "C" int met2_warp(int32_t device, int32_t order, const int32_t src_dims[3], int32_t n_series, const double *src, int64_t src_voxel_stride,
                         int64_t src_series_stride, const int32_t dst_dims[3], const double A[12], const double *disp, double cval, double *dst,
                         int64_t dst_voxel_stride, int64_t dst_series_stride, uint8_t *inside, void *stream)
{
    int rc;
    if (order != 0 && order != 1) return fail(MET2_E_INVALID, "the interpolation order of a warp must be 0 or 1");
    if ((rc = wp_check_dims(src_dims, "source")) || (rc = wp_check_dims(dst_dims, "destination")) || (rc = rs_check_series(n_series)) ||
        (rc = rs_check_transform(A)))
        return rc;
    if (!disp) return fail(MET2_E_INVALID, "NULL displacement field (met2_resample is the call without one)");
    if (!src || !dst) return fail(MET2_E_INVALID, "NULL argument");
    if (src == dst || disp == dst) return fail(MET2_E_INVALID, "dst must not alias src or disp");
    if (src_voxel_stride < 1 || src_series_stride < 1 || dst_voxel_stride < 1 || dst_series_stride < 1)
        return fail(MET2_E_INVALID, "the strides must be positive");
    const int64_t n_dst = (int64_t)dst_dims[0] * dst_dims[1] * dst_dims[2];
    if (n_series > 1 && n_dst > 1 && dst_series_stride < n_dst * dst_voxel_stride && dst_voxel_stride < (int64_t)n_series * dst_series_stride)
        return fail(MET2_E_INVALID, "the destination strides make two (voxel, series) pairs share an element");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const RsGeom G = rs_geom(src_dims, dst_dims, A);
    const dim3 grid(rs_grid(n_dst, RS_BLOCK));
    if (order == 0)
        hipLaunchKernelGGL((wp_voxel_kernel<0, double>), grid, dim3(RS_BLOCK), 0, st, G, n_series, src, src_voxel_stride, src_series_stride, disp, cval, dst,
                           dst_voxel_stride, dst_series_stride, inside);
    else
        hipLaunchKernelGGL((wp_voxel_kernel<1, double>), grid, dim3(RS_BLOCK), 0, st, G, n_series, src, src_voxel_stride, src_series_stride, disp, cval, dst,
                           dst_voxel_stride, dst_series_stride, inside);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_warp_labels(int32_t device, const int32_t src_dims[3], const int32_t *labels, const int32_t dst_dims[3], const double A[12],
                                const double *disp, int32_t fill, int32_t *out, uint8_t *inside, void *stream)
{
    int rc;
    if ((rc = wp_check_dims(src_dims, "source")) || (rc = wp_check_dims(dst_dims, "destination")) || (rc = rs_check_transform(A))) return rc;
    if (!disp) return fail(MET2_E_INVALID, "NULL displacement field (met2_resample_labels is the call without one)");
    if (!labels || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (labels == out) return fail(MET2_E_INVALID, "out must not alias labels");
    USE_DEVICE(device);
    const RsGeom G = rs_geom(src_dims, dst_dims, A);
    const int64_t n_dst = (int64_t)G.mx * G.my * G.mz;
    hipLaunchKernelGGL((wp_voxel_kernel<0, int32_t>), dim3(rs_grid(n_dst, RS_BLOCK)), dim3(RS_BLOCK), 0, (hipStream_t)stream, G, 1, labels, (int64_t)1,
                       (int64_t)1, disp, fill, out, (int64_t)1, (int64_t)1, inside);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_warp_compose(int32_t device, const int32_t src_dims[3], const double *u_src, const int32_t dst_dims[3], const double A[12],
                                 const double gain[3], const double *v, double step, const double *vmax2, double *out, void *stream)
{
    int rc;
    if ((rc = wp_check_dims(src_dims, "source")) || (rc = wp_check_dims(dst_dims, "destination")) || (rc = rs_check_transform(A))) return rc;
    if (!gain || !u_src || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (!(std::isfinite(gain[0]) && std::isfinite(gain[1]) && std::isfinite(gain[2]) && std::isfinite(step)))
        return fail(MET2_E_INVALID, "gain and step must be finite");
    if (out == u_src || out == v) return fail(MET2_E_INVALID, "out must not alias u_src or v");
    USE_DEVICE(device);
    const RsGeom G = rs_geom(src_dims, dst_dims, A);
    WpGain g;
    for (int a = 0; a < 3; ++a) g.g[a] = gain[a];
    const int64_t n_dst = (int64_t)G.mx * G.my * G.mz;
    hipLaunchKernelGGL(wp_compose_kernel, dim3(rs_grid(n_dst, RS_BLOCK)), dim3(RS_BLOCK), 0, (hipStream_t)stream, G, g, u_src, v, step, vmax2, out);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_warp_max_norm2(int32_t device, int64_t n_voxels, const double *v, double *vmax2, void *stream)
{
    if (n_voxels < 1 || n_voxels > 0x7fffffffLL) return fail(MET2_E_INVALID, "the field must hold 1 .. 2^31 - 1 voxels");
    if (!v || !vmax2) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(vmax2, 0, sizeof(double), st));
    hipLaunchKernelGGL(wp_max_norm2_kernel, dim3(std::min(rs_grid(n_voxels, RS_BLOCK), WP_FORCE_GRID)), dim3(RS_BLOCK), 0, st, n_voxels, v,
                       (unsigned long long *)vmax2);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_warp_invert_step(int32_t device, const int32_t src_dims[3], const double *u_src, const int32_t dst_dims[3], const double B[12],
                                     const double N[9], const double *v_in, double *v_out, uint8_t *inside, double *res2, void *stream)
{
    int rc;
    if ((rc = wp_check_dims(src_dims, "source")) || (rc = wp_check_dims(dst_dims, "destination")) || (rc = rs_check_transform(B))) return rc;
    if (!N || !u_src || !v_out) return fail(MET2_E_INVALID, "NULL argument");
    for (int e = 0; e < 9; ++e)
        if (!std::isfinite(N[e])) return fail(MET2_E_INVALID, "every entry of N must be finite");
    if (v_out == u_src || v_out == v_in) return fail(MET2_E_INVALID, "v_out must not alias u_src or v_in");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const RsGeom G = rs_geom(src_dims, dst_dims, B);
    WpMat3 M;
    for (int e = 0; e < 9; ++e) M.n[e] = N[e];
    if (res2) HIPCHK(hipMemsetAsync(res2, 0, sizeof(double), st));
    const int64_t n_dst = (int64_t)G.mx * G.my * G.mz;
    hipLaunchKernelGGL(wp_invert_step_kernel, dim3(std::min(rs_grid(n_dst, RS_BLOCK), WP_INVERSE_GRID)), dim3(RS_BLOCK), 0, st, G, M, u_src, v_in, v_out,
                       inside, (unsigned long long *)res2);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_warp_jacobian(int32_t device, const int32_t dims[3], const double *u, double scale, double *det, int64_t *n_nonpositive, void *stream)
{
    int rc = wp_check_dims(dims, "volume");
    if (rc) return rc;
    if (!u || !det) return fail(MET2_E_INVALID, "NULL argument");
    if (!std::isfinite(scale)) return fail(MET2_E_INVALID, "scale must be finite");
    if ((const void *)det == (const void *)u) return fail(MET2_E_INVALID, "det must not alias u");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    if (n_nonpositive) HIPCHK(hipMemsetAsync(n_nonpositive, 0, sizeof(int64_t), st));
    const int64_t nvox = (int64_t)dims[0] * dims[1] * dims[2];
    hipLaunchKernelGGL(wp_jacobian_kernel, dim3(std::min(rs_grid(nvox, RS_BLOCK), WP_INVERSE_GRID)), dim3(RS_BLOCK), 0, st, dims[0], dims[1], dims[2], u, scale,
                       det, (unsigned long long *)n_nonpositive);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_warp_work_bytes(const int32_t dims[3], int64_t *bytes)
{
    int rc = wp_check_dims(dims, "volume");
    if (rc) return rc;
    if (!bytes) return fail(MET2_E_INVALID, "NULL argument");
    *bytes = (int64_t)wp_work_need(dims, 2, true);
    return MET2_OK;
}

extern "C" int met2_warp_lncc_sums(int32_t device, const int32_t dims[3], const double *fixed, const double *warped, const uint8_t *inside,
                                   int32_t radius, double *sums, void *work, int64_t work_bytes, void *stream)
{
    int rc = wp_check_lncc(dims, radius, 0.0);
    if (rc) return rc;
    if (!fixed || !warped || !inside || !sums) return fail(MET2_E_INVALID, "NULL argument");
    if ((rc = wp_check_work(work, work_bytes, wp_work_need(dims, 1, false)))) return rc;
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork W(st);
    const auto tmp = W.take<double>((size_t)6 * dims[0] * dims[1] * dims[2]);
    if (!W.alloc(work)) return W.finish("met2_warp_lncc_sums");
    W.ok(wp_sums_launch(dims, radius, fixed, warped, inside, sums, tmp, st));
    return W.finish("met2_warp_lncc_sums");
}

extern "C" int met2_warp_lncc_force(int32_t device, const int32_t dims[3], const double *fixed, const double *warped, const uint8_t *inside,
                                    const double *sums, double eps, double *force, double *metric, void *work, int64_t work_bytes, void *stream)
{
    int rc = wp_check_lncc(dims, 1, eps);
    if (rc) return rc;
    if (!fixed || !warped || !inside || !sums || !force || !metric) return fail(MET2_E_INVALID, "NULL argument");
    if ((rc = wp_check_work(work, work_bytes, wp_work_need(dims, 0, true)))) return rc;
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork W(st);
    const auto partial = W.take<double>(2 * WP_FORCE_GRID);
    if (!W.alloc(work)) return W.finish("met2_warp_lncc_force");
    W.ok(wp_force_launch(dims, fixed, warped, inside, sums, eps, force, metric, partial, st));
    return W.finish("met2_warp_lncc_force");
}

extern "C" int met2_warp_lncc(int32_t device, const int32_t dims[3], const double *fixed, const double *warped, const uint8_t *inside, int32_t radius,
                              double eps, double *force, double *metric, void *work, int64_t work_bytes, void *stream)
{
    int rc = wp_check_lncc(dims, radius, eps);
    if (rc) return rc;
    if (!fixed || !warped || !inside || !force || !metric) return fail(MET2_E_INVALID, "NULL argument");
    if ((rc = wp_check_work(work, work_bytes, wp_work_need(dims, 2, true)))) return rc;
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork W(st);
    const size_t n6 = (size_t)6 * dims[0] * dims[1] * dims[2];
    const auto sums = W.take<double>(n6);
    const auto tmp = W.take<double>(n6);
    const auto partial = W.take<double>(2 * WP_FORCE_GRID);
    if (!W.alloc(work)) return W.finish("met2_warp_lncc");
    if (W.ok(wp_sums_launch(dims, radius, fixed, warped, inside, sums, tmp, st)))
        W.ok(wp_force_launch(dims, fixed, warped, inside, sums, eps, force, metric, partial, st));
    return W.finish("met2_warp_lncc");
}
