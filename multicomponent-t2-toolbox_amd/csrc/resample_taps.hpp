// resample_taps.hpp -- the sampling rule of include/met2_hip.h (affine resampling): coordinates, the inside test, mirrored taps, weights and
// the tap sum of one (voxel, series), as device functions.  met2_resample.hip interpolates through them and met2_register.hip evaluates its
// cost through them, so a registration samples the moving volume with the bits a resampling gives.  Include after
// `#pragma clang fp contract(off)`: every operation rounds once, in the order written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_helpers.hpp"     // rn_mul, rn_add, rn_sub: the file-scope pragma already forbids contraction; they name the intent where the order is the contract

namespace {

struct RsGeom {
    int nx, ny, nz;                        // source
    int mx, my, mz;                        // destination
    double A[12];
};

// tap m of a line of n samples, mirrored about the end samples
__device__ __forceinline__ int rs_mirror(int m, int n)
{
    if (n == 1) return 0;
    const int P = 2 * (n - 1);
    m %= P;
    if (m < 0) m += P;
    return m > n - 1 ? P - m : m;
}

// c_a = ((A[a][3] + A[a][0] i) + A[a][1] j) + A[a][2] k
__device__ __forceinline__ double rs_coord(const double *row, double i, double j, double k)
{
    return rn_add(rn_add(rn_add(row[3], rn_mul(row[0], i)), rn_mul(row[1], j)), rn_mul(row[2], k));
}

__device__ __forceinline__ bool rs_inside(double c, int n) { return c >= 0.0 && c <= (double)(n - 1); }

// what a destination voxel needs of the source, per axis: tap offsets (already multiplied by the axis' stride in voxels) and weights
template <int ORDER>
struct RsTaps {
    static constexpr int N = ORDER == 0 ? 1 : ORDER == 1 ? 2 : 4;
    int ox[N], oy[N], oz[N];
    double wx[N], wy[N], wz[N];
};

template <int ORDER>
__device__ __forceinline__ void rs_axis(double c, int n, int stride, int *o, double *w)
{
    if (ORDER == 0) {
        o[0] = (int)floor(rn_add(c, 0.5)) * stride;
        w[0] = 1.0;
    } else {
        const double fl = floor(c), t = rn_sub(c, fl);
        const int f = (int)fl;
        if (ORDER == 1) {
            o[0] = f * stride;
            o[1] = rs_mirror(f + 1, n) * stride;
            w[0] = rn_sub(1.0, t);
            w[1] = t;
        } else {
            const double u = rn_sub(1.0, t);
#pragma unroll
            for (int p = 0; p < 4; ++p) o[p] = rs_mirror(f - 1 + p, n) * stride;
            w[0] = rn_mul(rn_mul(u, u), u) / 6.0;
            w[1] = rn_add(rn_mul(rn_mul(rn_sub(rn_mul(3.0, t), 6.0), t), t), 4.0) / 6.0;
            w[2] = rn_add(rn_mul(rn_mul(rn_sub(rn_mul(3.0, u), 6.0), u), u), 4.0) / 6.0;
            w[3] = rn_mul(rn_mul(t, t), t) / 6.0;
        }
    }
}

// -> whether the source coordinates (cx, cy, cz) are inside; then T holds their taps (met2_warp.hip comes in here, with the coordinates of a
// displaced voxel)
template <int ORDER>
__device__ __forceinline__ bool rs_taps_at(const RsGeom &G, double cx, double cy, double cz, RsTaps<ORDER> &T)
{
    if (!(rs_inside(cx, G.nx) && rs_inside(cy, G.ny) && rs_inside(cz, G.nz))) return false;
    rs_axis<ORDER>(cx, G.nx, G.ny * G.nz, T.ox, T.wx);
    rs_axis<ORDER>(cy, G.ny, G.nz, T.oy, T.wy);
    rs_axis<ORDER>(cz, G.nz, 1, T.oz, T.wz);
    return true;
}

// -> whether destination voxel (i, j, k) is inside; then T holds its taps
template <int ORDER>
__device__ __forceinline__ bool rs_taps(const RsGeom &G, int i, int j, int k, RsTaps<ORDER> &T)
{
    const double di = (double)i, dj = (double)j, dk = (double)k;
    const double cx = rs_coord(G.A, di, dj, dk), cy = rs_coord(G.A + 4, di, dj, dk), cz = rs_coord(G.A + 8, di, dj, dk);
    return rs_taps_at<ORDER>(G, cx, cy, cz, T);
}

// the value of one series at the taps: sum_p sum_q sum_r ((wx_p wy_q) wz_r) v, p outermost, from the first term on
template <int ORDER, typename V>
__device__ __forceinline__ V rs_value(const RsTaps<ORDER> &T, const V *__restrict__ s, int64_t voxel_stride)
{
    if (ORDER == 0) return s[(int64_t)(T.ox[0] + T.oy[0] + T.oz[0]) * voxel_stride];
    constexpr int N = RsTaps<ORDER>::N;
    double acc = 0.0;
    if constexpr (ORDER == 3) {
        // The loop over p is kept a loop, its x tap rotating through four registers (after four turns they hold what they held), so that its
        // body is 16 taps and nothing in it is invariant over the series: unrolled 64-fold, the compiler hoists the 64 weight products and
        // offsets out of the series loop and takes 256 VGPRs, one wave per SIMD.  This way: 123 VGPRs, 4 waves, and the call at 8 series of
        // 128 x 128 x 64 went from 1.28 to 0.77 ms (profiles/resample_ab.json).  The arithmetic and its order are the same.
        double wx0 = T.wx[0], wx1 = T.wx[1], wx2 = T.wx[2], wx3 = T.wx[3];
        int ox0 = T.ox[0], ox1 = T.ox[1], ox2 = T.ox[2], ox3 = T.ox[3];
#pragma unroll 1
        for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double wpq = rn_mul(wx0, T.wy[q]);
                const int opq = ox0 + T.oy[q];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double term = rn_mul(rn_mul(wpq, T.wz[r]), (double)s[(int64_t)(opq + T.oz[r]) * voxel_stride]);
                    acc = (p | q | r) == 0 ? term : rn_add(acc, term);
                }
            }
            const double w = wx0;
            wx0 = wx1; wx1 = wx2; wx2 = wx3; wx3 = w;
            const int o = ox0;
            ox0 = ox1; ox1 = ox2; ox2 = ox3; ox3 = o;
        }
        return (V)acc;
    }
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const double wpq = rn_mul(T.wx[p], T.wy[q]);
            const int opq = T.ox[p] + T.oy[q];
#pragma unroll
            for (int r = 0; r < N; ++r) {
                const double term = rn_mul(rn_mul(wpq, T.wz[r]), (double)s[(int64_t)(opq + T.oz[r]) * voxel_stride]);
                acc = (p | q | r) == 0 ? term : rn_add(acc, term);
            }
        }
    return (V)acc;
}

}  // namespace
