// met2_resample.hip -- met2_resample, met2_resample_labels, met2_resample_prefilter: affine resampling of volumes and label images through a
// given 3 x 4 voxel-to-voxel transform, nearest neighbour, trilinear or cubic B-spline (scipy.ndimage.affine_transform with mode='constant',
// restated; include/met2_hip.h states the contract).  Written from that statement and from Unser, Aldroubi & Eden (IEEE TSP 41:821-848, 1993).
//   rs_gather_kernel<VM>      a chunk of series, read through the caller's strides, into the series-major work space [chunk][nx][ny][nz]; for
//                             voxel-major sources (series stride 1) through a tile in LDS, so that reads run along the series and writes along z
//   rs_prefilter_lane_kernel  the recursive filter along x or y, in place: the volume seen as [outer][n][inner], one lane per line, lanes along
//                             `inner` (which ends in z, the contiguous axis), so every access of the wave is coalesced
//   rs_prefilter_z_kernel     the same along z, where the lines themselves are contiguous: a tile of lines is copied into LDS with coalesced
//                             accesses, rows padded to an odd stride in doubles (the 8-byte accesses of a half-wave then fall on distinct banks),
//                             one lane runs one line in LDS, and the tile is copied back
//   rs_voxel_kernel<ORDER, T> the interpolation, one destination voxel per thread, threads along the destination's z: coordinates, floor,
//                             weights and tap offsets once per voxel, then a loop over the series of the chunk.  Any strides.
//   rs_group_kernel<ORDER>    orders 0 and 1 when source and destination are both voxel-major (series stride 1) and hold at least 4 series: a group
//                             of 4 .. 64 lanes per voxel, lanes along the series, so that the gathers and the stores run along the contiguous axis.
//                             Order 3 reads its coefficients from the series-major work space and always takes rs_voxel_kernel.
// Both interpolation kernels call the same device functions for a (voxel, series) value, and the file is compiled without contraction, so the
// bits do not depend on the kernel, the chunking or the layout.  Every loop is bounded by a shape or a compile-time constant; no kernel
// indexes a register array with a run-time value (no scratch).
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

#define RS_TILE_V 64                       // rs_gather_kernel<true>: voxels x series of a tile
#define RS_TILE_S 32
#define RS_Z_LDS_DOUBLES 8064              // rs_prefilter_z_kernel: doubles of a tile in LDS (63 KiB), 15 lines at nz = 512

template <int ORDER, typename V>
__global__ void __launch_bounds__(RS_BLOCK) rs_voxel_kernel(RsGeom G, int n_series, const V *__restrict__ src, int64_t svs, int64_t sss, V fill,
                                                            V *__restrict__ dst, int64_t dvs, int64_t dss, uint8_t *__restrict__ inside)
{
    const int64_t n_dst = (int64_t)G.mx * G.my * G.mz;
    for (int64_t w = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; w < n_dst; w += (int64_t)gridDim.x * RS_BLOCK) {
        int i, j, k;
        rs_split(w, G, i, j, k);
        RsTaps<ORDER> T;
        const bool in = rs_taps<ORDER>(G, i, j, k, T);
        if (inside) inside[w] = in ? 1 : 0;
        V *d = dst + w * dvs;
        if (in)
            for (int s = 0; s < n_series; ++s) d[s * dss] = rs_value<ORDER, V>(T, src + s * sss, svs);
        else
            for (int s = 0; s < n_series; ++s) d[s * dss] = fill;
    }
}

// `group` lanes (a power of two, 4 .. 64) per destination voxel, lanes along the series; source and destination series strides are 1
template <int ORDER>
__global__ void __launch_bounds__(RS_BLOCK) rs_group_kernel(RsGeom G, int n_series, int group, const double *__restrict__ src, int64_t svs, double fill,
                                                            double *__restrict__ dst, int64_t dvs, uint8_t *__restrict__ inside)
{
    const int64_t n_dst = (int64_t)G.mx * G.my * G.mz;
    const int per_block = RS_BLOCK / group, lane = threadIdx.x % group;
    for (int64_t w = (int64_t)blockIdx.x * per_block + threadIdx.x / group; w < n_dst; w += (int64_t)gridDim.x * per_block) {
        int i, j, k;
        rs_split(w, G, i, j, k);
        RsTaps<ORDER> T;
        const bool in = rs_taps<ORDER>(G, i, j, k, T);
        if (inside && lane == 0) inside[w] = in ? 1 : 0;
        double *d = dst + w * dvs;
        if (in)
            for (int s = lane; s < n_series; s += group) d[s] = rs_value<ORDER, double>(T, src + s, svs);
        else
            for (int s = lane; s < n_series; s += group) d[s] = fill;
    }
}

// work [n_series][nvox] <- series s of voxel v at src[v svs + s sss].  VM = false: one thread per element, threads along the voxels.
// VM = true (sss == 1): a tile of RS_TILE_V voxels x RS_TILE_S series goes through LDS; blockIdx.x walks the voxel tiles, blockIdx.y the series tiles.
template <bool VM>
__global__ void __launch_bounds__(RS_BLOCK) rs_gather_kernel(int64_t nvox, int n_series, const double *__restrict__ src, int64_t svs, int64_t sss,
                                                             double *__restrict__ work)
{
    if (!VM) {
        const int64_t total = nvox * n_series;
        for (int64_t e = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * RS_BLOCK) {
            const int64_t s = e / nvox, v = e - s * nvox;
            work[e] = src[v * svs + s * sss];
        }
    } else {
        __shared__ double tile[RS_TILE_S * (RS_TILE_V + 1)];
        const int s0 = blockIdx.y * RS_TILE_S, ns = min(RS_TILE_S, n_series - s0);
        const int64_t n_tiles = (nvox + RS_TILE_V - 1) / RS_TILE_V;
        for (int64_t tv = blockIdx.x; tv < n_tiles; tv += gridDim.x) {
            const int64_t v0 = tv * RS_TILE_V;
            const int nv = (int)min((int64_t)RS_TILE_V, nvox - v0);
            for (int e = threadIdx.x; e < nv * ns; e += RS_BLOCK) {
                const int v = e / ns, s = e - v * ns;
                tile[s * (RS_TILE_V + 1) + v] = src[(v0 + v) * svs + (s0 + s)];
            }
            __syncthreads();
            for (int e = threadIdx.x; e < nv * ns; e += RS_BLOCK) {
                const int s = e / nv, v = e - s * nv;
                work[(int64_t)(s0 + s) * nvox + v0 + v] = tile[s * (RS_TILE_V + 1) + v];
            }
            __syncthreads();
        }
    }
}

struct RsPole {
    double z, lambda, zn, norm, last;       // z1, (1 - z1)(1 - 1 / z1), z1^(n-1), 1 - zn zn, z1 / (z1 z1 - 1)
};

// The recursive filter of one line of n >= 2 samples at c[0], c[stride], ..., in place (global memory or LDS).
template <typename P>
__device__ __forceinline__ void rs_filter_line(P c, int n, int64_t stride, const RsPole &K)
{
    double c0 = rn_add(rn_mul(K.lambda, c[0]), rn_mul(K.zn, rn_mul(K.lambda, c[(n - 1) * stride])));
    double p = K.z;
    for (int i = 1; i < n - 1; ++i) {
        c0 = rn_add(c0, rn_mul(p, rn_add(rn_mul(K.lambda, c[i * stride]), rn_mul(K.zn, rn_mul(K.lambda, c[(n - 1 - i) * stride])))));
        p = rn_mul(p, K.z);
    }
    c0 = c0 / K.norm;
    c[0] = c0;
    double prev = c0;
    for (int i = 1; i < n; ++i) {
        prev = rn_add(rn_mul(K.lambda, c[i * stride]), rn_mul(K.z, prev));
        c[i * stride] = prev;
    }
    prev = rn_mul(rn_add(rn_mul(K.z, c[(n - 2) * stride]), prev), K.last);
    c[(n - 1) * stride] = prev;
    for (int i = n - 2; i >= 0; --i) {
        prev = rn_mul(K.z, rn_sub(prev, c[i * stride]));
        c[i * stride] = prev;
    }
}

// the volume as [outer][n][inner]: line (o, r) holds c[(o n + i) inner + r], i = 0 .. n - 1; lanes along r
__global__ void __launch_bounds__(RS_BLOCK) rs_prefilter_lane_kernel(double *__restrict__ c, int64_t outer, int n, int64_t inner, RsPole K)
{
    const int64_t lines = outer * inner;
    for (int64_t l = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; l < lines; l += (int64_t)gridDim.x * RS_BLOCK) {
        const int64_t o = l / inner, r = l - o * inner;
        rs_filter_line(c + o * n * inner + r, n, inner, K);
    }
}

// contiguous lines of n samples; a tile of `tile_lines` of them in LDS at an odd row stride `ld`
__global__ void __launch_bounds__(RS_BLOCK) rs_prefilter_z_kernel(double *__restrict__ c, int64_t lines, int n, int tile_lines, int ld, RsPole K)
{
    extern __shared__ double rs_lds[];
    const int64_t n_tiles = (lines + tile_lines - 1) / tile_lines;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t l0 = t * tile_lines;
        const int nl = (int)min((int64_t)tile_lines, lines - l0);
        double *g = c + l0 * n;
        for (int e = threadIdx.x; e < nl * n; e += RS_BLOCK) {
            const int l = e / n, i = e - l * n;
            rs_lds[l * ld + i] = g[e];
        }
        __syncthreads();
        if ((int)threadIdx.x < nl) rs_filter_line(rs_lds + threadIdx.x * ld, n, 1, K);
        __syncthreads();
        for (int e = threadIdx.x; e < nl * n; e += RS_BLOCK) {
            const int l = e / n, i = e - l * n;
            g[e] = rs_lds[l * ld + i];
        }
        __syncthreads();
    }
}

RsPole rs_pole(int n)
{
    RsPole K;
    K.z = std::sqrt(3.0) - 2.0;
    K.lambda = (1.0 - K.z) * (1.0 - 1.0 / K.z);
    K.zn = std::pow(K.z, (double)(n - 1));
    K.norm = 1.0 - K.zn * K.zn;
    K.last = K.z / (K.z * K.z - 1.0);
    return K;
}

// the launches of the prefilter of n_series series: gather into work [n_series][nx][ny][nz], then x, y, z in place
hipError_t rs_prefilter_launch(const int32_t *sd, int n_series, const double *src, int64_t svs, int64_t sss, double *work, hipStream_t st)
{
    const int nx = sd[0], ny = sd[1], nz = sd[2];
    const int64_t nvox = (int64_t)nx * ny * nz;
    if (sss == 1 && n_series > 1) {
        const dim3 grid(rs_grid(nvox, RS_TILE_V), (n_series + RS_TILE_S - 1) / RS_TILE_S);
        hipLaunchKernelGGL(rs_gather_kernel<true>, grid, dim3(RS_BLOCK), 0, st, nvox, n_series, src, svs, sss, work);
    } else {
        hipLaunchKernelGGL(rs_gather_kernel<false>, dim3(rs_grid(nvox * n_series, RS_BLOCK)), dim3(RS_BLOCK), 0, st, nvox, n_series, src, svs, sss, work);
    }
    if (nx > 1) {
        const int64_t inner = (int64_t)ny * nz;
        hipLaunchKernelGGL(rs_prefilter_lane_kernel, dim3(rs_grid(n_series * inner, RS_BLOCK)), dim3(RS_BLOCK), 0, st, work, (int64_t)n_series, nx, inner,
                           rs_pole(nx));
    }
    if (ny > 1) {
        const int64_t outer = (int64_t)n_series * nx;
        hipLaunchKernelGGL(rs_prefilter_lane_kernel, dim3(rs_grid(outer * nz, RS_BLOCK)), dim3(RS_BLOCK), 0, st, work, outer, ny, (int64_t)nz, rs_pole(ny));
    }
    if (nz > 1) {
        const int ld = nz | 1;
        const int tile_lines = std::min(64, RS_Z_LDS_DOUBLES / ld);
        const int64_t lines = (int64_t)n_series * nx * ny;
        hipLaunchKernelGGL(rs_prefilter_z_kernel, dim3(rs_grid(lines, tile_lines)), dim3(RS_BLOCK), (size_t)tile_lines * ld * sizeof(double), st, work, lines,
                           nz, tile_lines, ld, rs_pole(nz));
    }
    return hipGetLastError();
}

template <int ORDER>
hipError_t rs_interp_launch(const RsGeom &G, int n_series, const double *src, int64_t svs, int64_t sss, double cval, double *dst, int64_t dvs, int64_t dss,
                            uint8_t *inside, hipStream_t st)
{
    const int64_t n_dst = (int64_t)G.mx * G.my * G.mz;
    bool grouped = false;
    if constexpr (ORDER != 3) {
        if (sss == 1 && dss == 1 && n_series >= 4) {
            int group = 4;
            while (group < 64 && group < n_series) group *= 2;
            hipLaunchKernelGGL(rs_group_kernel<ORDER>, dim3(rs_grid(n_dst, RS_BLOCK / group)), dim3(RS_BLOCK), 0, st, G, n_series, group, src, svs, cval, dst,
                               dvs, inside);
            grouped = true;
        }
    }
    if (!grouped)
        hipLaunchKernelGGL((rs_voxel_kernel<ORDER, double>), dim3(rs_grid(n_dst, RS_BLOCK)), dim3(RS_BLOCK), 0, st, G, n_series, src, svs, sss, cval, dst, dvs,
                           dss, inside);
    return hipGetLastError();
}

void rs_work_bytes(int order, const int32_t *sd, int n_series, int64_t *lo, int64_t *dflt)
{
    *lo = *dflt = 0;
    if (order != 3) return;
    *lo = 8LL * sd[0] * sd[1] * sd[2];
    *dflt = std::max(*lo, std::min<int64_t>(*lo * n_series, 1LL << 30));
}

int rs_check_order(int order)
{
    return order == 0 || order == 1 || order == 3 ? MET2_OK : fail(MET2_E_INVALID, "the interpolation order must be 0, 1 or 3");
}

}  // namespace

extern "C" int met2_resample_work_bytes(int32_t order, const int32_t src_dims[3], int32_t n_series, int64_t *min_bytes, int64_t *default_bytes)
{
    int rc;
    if ((rc = rs_check_order(order)) || (rc = rs_check_dims(src_dims, "source", true)) || (rc = rs_check_series(n_series))) return rc;
    int64_t lo, dflt;
    rs_work_bytes(order, src_dims, n_series, &lo, &dflt);
    if (min_bytes) *min_bytes = lo;
    if (default_bytes) *default_bytes = dflt;
    return MET2_OK;
}

extern "C" int met2_resample(int32_t device, int32_t order, const int32_t src_dims[3], int32_t n_series, const double *src, int64_t src_voxel_stride,
                             int64_t src_series_stride, const int32_t dst_dims[3], const double A[12], double cval, double *dst,
                             int64_t dst_voxel_stride, int64_t dst_series_stride, uint8_t *inside, int64_t max_work_bytes, void *stream)
{
    int rc;
    if ((rc = rs_check_order(order)) || (rc = rs_check_dims(src_dims, "source", true)) || (rc = rs_check_dims(dst_dims, "destination", false)) ||
        (rc = rs_check_series(n_series)) || (rc = rs_check_transform(A)))
        return rc;
    if (!src || !dst) return fail(MET2_E_INVALID, "NULL argument");
    if (src == dst) return fail(MET2_E_INVALID, "dst must not alias src");
    if (src_voxel_stride < 1 || src_series_stride < 1 || dst_voxel_stride < 1 || dst_series_stride < 1)
        return fail(MET2_E_INVALID, "the strides must be positive");
    const int64_t n_dst = (int64_t)dst_dims[0] * dst_dims[1] * dst_dims[2];
    if (n_series > 1 && n_dst > 1 && dst_series_stride < n_dst * dst_voxel_stride && dst_voxel_stride < (int64_t)n_series * dst_series_stride)
        return fail(MET2_E_INVALID, "the destination strides make two (voxel, series) pairs share an element");
    int64_t lo, dflt;
    rs_work_bytes(order, src_dims, n_series, &lo, &dflt);
    if (max_work_bytes < 0) return fail(MET2_E_INVALID, "max_work_bytes must not be negative");
    if (order == 3 && max_work_bytes > 0 && max_work_bytes < lo)
        return fail(MET2_E_INVALID, "max_work_bytes is below the minimum of " + std::to_string(lo) + " bytes (one series' coefficients)");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const RsGeom G = rs_geom(src_dims, dst_dims, A);
    if (order == 0) HIPCHK(rs_interp_launch<0>(G, n_series, src, src_voxel_stride, src_series_stride, cval, dst, dst_voxel_stride, dst_series_stride, inside, st));
    if (order == 1) HIPCHK(rs_interp_launch<1>(G, n_series, src, src_voxel_stride, src_series_stride, cval, dst, dst_voxel_stride, dst_series_stride, inside, st));
    if (order != 3) return MET2_OK;
    const int64_t budget = max_work_bytes > 0 ? max_work_bytes : dflt;
    const int chunk = (int)std::min<int64_t>(n_series, budget / lo);
    const int64_t nvox = lo / 8;
    DeviceWork W(st);
    const auto work = W.take<double>((size_t)chunk * nvox);
    if (!W.alloc()) return W.finish("met2_resample");
    for (int s0 = 0; s0 < n_series && W.ok(); s0 += chunk) {
        const int ns = std::min(chunk, n_series - s0);
        if (W.ok(rs_prefilter_launch(src_dims, ns, src + s0 * src_series_stride, src_voxel_stride, src_series_stride, work, st)))
            W.ok(rs_interp_launch<3>(G, ns, work, 1, nvox, cval, dst + s0 * dst_series_stride, dst_voxel_stride, dst_series_stride, s0 == 0 ? inside : nullptr, st));
    }
    return W.finish("met2_resample");
}

extern "C" int met2_resample_labels(int32_t device, const int32_t src_dims[3], const int32_t *labels, const int32_t dst_dims[3], const double A[12],
                                    int32_t fill, int32_t *out, uint8_t *inside, void *stream)
{
    int rc;
    if ((rc = rs_check_dims(src_dims, "source", true)) || (rc = rs_check_dims(dst_dims, "destination", false)) || (rc = rs_check_transform(A))) return rc;
    if (!labels || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (labels == out) return fail(MET2_E_INVALID, "out must not alias labels");
    USE_DEVICE(device);
    const RsGeom G = rs_geom(src_dims, dst_dims, A);
    const int64_t n_dst = (int64_t)G.mx * G.my * G.mz;
    hipLaunchKernelGGL((rs_voxel_kernel<0, int32_t>), dim3(rs_grid(n_dst, RS_BLOCK)), dim3(RS_BLOCK), 0, (hipStream_t)stream, G, 1, labels, (int64_t)1,
                       (int64_t)1, fill, out, (int64_t)1, (int64_t)1, inside);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_resample_prefilter(int32_t device, const int32_t src_dims[3], int32_t n_series, const double *src, int64_t src_voxel_stride,
                                       int64_t src_series_stride, double *coef, void *stream)
{
    int rc;
    if ((rc = rs_check_dims(src_dims, "source", true)) || (rc = rs_check_series(n_series))) return rc;
    if (!src || !coef) return fail(MET2_E_INVALID, "NULL argument");
    if (src == coef) return fail(MET2_E_INVALID, "coef must not alias src");
    if (src_voxel_stride < 1 || src_series_stride < 1) return fail(MET2_E_INVALID, "the strides must be positive");
    USE_DEVICE(device);
    HIPCHK(rs_prefilter_launch(src_dims, n_series, src, src_voxel_stride, src_series_stride, coef, (hipStream_t)stream));
    return MET2_OK;
}
