// met2_group_vsm.hip -- met2_group_vsm_limits, met2_group_vsm_work_bytes, met2_masked_smooth, met2_group_perm_vsm: variance smoothing for
// the voxel-wise permutation test.  The residual variance of every candidate is pooled over a Gaussian neighbourhood inside the mask and the
// statistic is the pseudo-t, b / sqrt(smoothed variance) (Holmes et al., J. Cereb. Blood Flow Metab. 16:7-22, 1996; Nichols & Holmes, Hum.
// Brain Mapp. 15:1-25, 2002).  include/met2_hip.h states the definitions and the contract; group.py forms the taps and holds the loop over
// batches.  Written from that statement.  The stages of one call of the group entry:
//   tf_mask_kernel       (tfce_kernel.hpp) the mask from `at`, which it also checks
//   vs_pass_kernel       one axis of the separable sum over a batch of maps [K][grid], blockIdx.y the map: a tile of VS_TA samples along the
//                        axis by VS_TC lines with its halo of R samples either side in LDS; on the contiguous axis (z) the tile lies line by
//                        line, otherwise sample by sample, so that a wave's lanes touch consecutive addresses in both memories either way.
//                        Terms in ascending offset from 0.0, product and sum rounded separately; a term whose source lies outside the grid adds
//                        an exact +0.0, which leaves the bits of skipping it, so the sum is the stated one whatever the tiling.  A thread
//                        carries its four samples as four chains side by side.  The taps arrive by value
//                        in the kernel's arguments and are read by scalar loads.  The first pass reads its input through the mask (0 outside),
//                        or the mask's indicator itself when there is no input: that gives N.
//   gp_moments_kernel    (group_kernel.hpp) b and rho = max(rss, 0) of the batch into two dense maps
//   vs_combine_kernel    sigma^2 = S(rho) / N, pseudo-t = b / sqrt(sigma^2), |.| when two-sided, written over S(rho) at mask voxels, 0 elsewhere
//   vs_gather_kernel     voxel mode: tf_gather_kernel's first, count and maxima on the pseudo-t, unscaled, with a value that is not a number
//                        passed over by the maximum
//   tf_transform, tf_gather_kernel   (tfce_kernel.hpp) the spatial modes (TFCE, cluster extent, cluster mass), unchanged
// Three launches for the three axes: a pass must be complete over the whole grid before the next starts (what else was
// tried).  No floating-point atomic; every loop is bounded by a shape or a constant.  Compiled without contraction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_helpers.hpp"
#include "device_work.hpp"
#include "group_kernel.hpp"
#include "tfce_kernel.hpp"

#pragma clang fp contract(off)

namespace {

#define VS_TA 64                           // samples of a tile along the axis
#define VS_TC 16                           // lines of a tile
#define VS_MAX_R MET2_GROUP_VSM_MAX_RADIUS
static_assert(VS_TA * VS_TC % 256 == 0, "a tile is a whole number of rounds of the block");
static_assert(MET2_GROUP_VSM_MAX_K == MET2_TFCE_MAX_K, "the spatial modes hand the batch to tf_transform as it is");

struct VsTaps { double w[2 * VS_MAX_R + 1]; };     // one axis' taps, by value: 264 bytes of kernel arguments

struct VsPass {
    const double *src;                     // [K][G], or NULL: the mask's indicator
    double *dst;                           // [K][G]
    const uint8_t *mask;                   // [G] or NULL: src is read as 0 where mask is 0 (the first pass only)
    int r;
    int A, C, O;                           // the axis' length, the lines of one slab, the slabs
    int64_t sa, sc, so;                    // their strides
    int64_t G;                             // the stride of a map
};

template <bool AXIS_FAST>
__global__ __launch_bounds__(256) void vs_pass_kernel(VsPass P, VsTaps T)
{
    __shared__ double tile[(VS_TA + 2 * VS_MAX_R) * VS_TC];           // 12 288 bytes
    const int nta = (P.A + VS_TA - 1) / VS_TA, ntc = (P.C + VS_TC - 1) / VS_TC;
    int bid = blockIdx.x;
    const int ta = bid % nta;
    bid /= nta;
    const int tc = bid % ntc, o = bid / ntc;                          // o < P.O: the launch has nta ntc O blocks
    const int a0 = ta * VS_TA, c0 = tc * VS_TC;
    const int rows = VS_TA + 2 * P.r;                                 // <= VS_TA + 2 VS_MAX_R: r is checked by the entry
    const int64_t slab = (int64_t)o * P.so, map = (int64_t)blockIdx.y * P.G;
    // the tile with its halo; outside the grid and outside the mask it holds 0.0
    const auto fetch = [&](int ia, int ic) {
        const int a = a0 - P.r + ia, c = c0 + ic;
        double x = 0.0;
        if (a >= 0 && a < P.A && c < P.C) {
            const int64_t cell = slab + (int64_t)a * P.sa + (int64_t)c * P.sc;
            if (!P.mask || P.mask[cell]) x = P.src ? P.src[map + cell] : 1.0;
        }
        return x;
    };
    if (AXIS_FAST) {                                                  // a wave takes a line at a time: no division by the run-time row count
        for (int ic = threadIdx.x >> 6; ic < VS_TC; ic += 4)
            for (int ia = threadIdx.x & 63; ia < rows; ia += 64) tile[ic * rows + ia] = fetch(ia, ic);
    } else {
        for (int e = threadIdx.x; e < rows * VS_TC; e += 256) tile[e] = fetch(e / VS_TC, e % VS_TC);
    }
    __syncthreads();
    // A thread's VS_PER samples are VS_PER independent chains, taken side by side; each chain's terms stay in ascending order.  The taps that
    // reach outside the grid meet the tile's zeros: tap * 0.0 is +0.0 (taps are finite and >= 0) and s + 0.0 is s to the bit, since a sum
    // that starts from +0.0 is never -0.0 -- the same bits as skipping the term, with no test in the loop.
    constexpr int VS_PER = VS_TA * VS_TC / 256;
    const int step = AXIS_FAST ? 1 : VS_TC;
    const double *tp[VS_PER];
    double s[VS_PER];
#pragma unroll
    for (int j = 0; j < VS_PER; ++j) {
        const int e = threadIdx.x + 256 * j;
        const int ia = AXIS_FAST ? e % VS_TA : e / VS_TC, ic = AXIS_FAST ? e / VS_TA : e % VS_TC;
        tp[j] = tile + (AXIS_FAST ? ic * rows + ia : ia * VS_TC + ic);
        s[j] = 0.0;
    }
    for (int t = 0; t <= 2 * P.r; ++t) {                              // t is wave-uniform: the tap is a scalar load
        const double w = T.w[t];
#pragma unroll
        for (int j = 0; j < VS_PER; ++j) s[j] = rn_add(s[j], rn_mul(w, tp[j][t * step]));
    }
#pragma unroll
    for (int j = 0; j < VS_PER; ++j) {
        const int e = threadIdx.x + 256 * j;
        const int a = a0 + (AXIS_FAST ? e % VS_TA : e / VS_TC), c = c0 + (AXIS_FAST ? e / VS_TA : e % VS_TC);
        if (a < P.A && c < P.C) P.dst[map + slab + (int64_t)a * P.sa + (int64_t)c * P.sc] = s[j];
    }
}

__global__ __launch_bounds__(256) void vs_combine_kernel(int G, const uint8_t *__restrict__ mask, const double *__restrict__ bmap,
                                                         const double *__restrict__ norm, int two_sided, double *__restrict__ S)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= G) return;
    const int64_t cell = (int64_t)blockIdx.y * G + v;
    double t = 0.0;
    if (mask[v]) {
        const double s2 = S[cell] / norm[v];                          // N > 0 on the mask: the centre tap is > 0
        t = s2 > 0.0 ? bmap[cell] / sqrt(s2) : 0.0;
        if (two_sided) t = fabs(t);
    }
    S[cell] = t;
}

// tf_gather_kernel on the pseudo-t: unscaled, and a statistic that is not a number is passed over by the maximum (it still reaches `first`,
// and no reference: the comparison fails)
__global__ void __launch_bounds__(TF_BLOCK) vs_gather_kernel(int64_t n_vox, const int32_t *__restrict__ at, int G, int K, const double *__restrict__ stat,
                                                             const double *__restrict__ ref, double *__restrict__ first,
                                                             unsigned long long *__restrict__ kmax, uint32_t *__restrict__ count)
{
    __shared__ double wmax[TF_WAVES];
    const int64_t v = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    const bool live = v < n_vox;
    const int a = live ? at[v] : 0;
    const double rf = (ref && live) ? ref[v] : 0.0;
    uint32_t cnt = 0;
    for (int k = 0; k < K; ++k) {
        double m = -INFINITY;
        if (live) {
            const double s = stat[(int64_t)k * G + a];
            if (ref && s >= rf) ++cnt;
            if (first && k == 0) first[v] = s;
            if (s == s) m = s;
        }
        tf_block_max(m, wmax, kmax + k);
    }
    if (ref && live) count[v] += cnt;                              // this thread owns the voxel
}

// x: nx samples at stride ny nz, the lines are the ny nz contiguous voxels; y: per x a slab of nz lines; z: contiguous, one line per (x, y)
VsPass vs_pass_args(int a, const TfGrid &g, const double *src, double *dst, const uint8_t *mask, int r)
{
    VsPass P;
    P.src = src; P.dst = dst; P.mask = mask; P.r = r; P.G = g.G;
    const int64_t plane = (int64_t)g.ny * g.nz;
    if (a == 0) { P.A = g.nx; P.C = (int)plane; P.O = 1; P.sa = plane; P.sc = 1; P.so = 0; }
    else if (a == 1) { P.A = g.ny; P.C = g.nz; P.O = g.nx; P.sa = g.nz; P.sc = 1; P.so = plane; }
    else { P.A = g.nz; P.C = (int)((int64_t)g.nx * g.ny); P.O = 1; P.sa = 1; P.sc = g.nz; P.so = 0; }
    return P;
}

void vs_enq_pass(hipStream_t st, int a, int K, const VsPass &P, const VsTaps &T)
{
    const int64_t tiles = (int64_t)((P.A + VS_TA - 1) / VS_TA) * ((P.C + VS_TC - 1) / VS_TC) * P.O;      // <= G < 2^31
    const dim3 grid((unsigned)tiles, (unsigned)K);
    if (a == 2)
        hipLaunchKernelGGL(vs_pass_kernel<true>, grid, dim3(256), 0, st, P, T);
    else
        hipLaunchKernelGGL(vs_pass_kernel<false>, grid, dim3(256), 0, st, P, T);
}

// S of K maps: x: src (through the mask) -> pong, y: pong -> ping, z: ping -> pong.  src may be ping itself.  The result lies in pong.
void vs_smooth(hipStream_t st, const TfGrid &g, int K, const double *src, const uint8_t *mask, const int32_t radius[3], const VsTaps taps[3],
               double *ping, double *pong)
{
    vs_enq_pass(st, 0, K, vs_pass_args(0, g, src, pong, mask, radius[0]), taps[0]);
    vs_enq_pass(st, 1, K, vs_pass_args(1, g, pong, ping, nullptr, radius[1]), taps[1]);
    vs_enq_pass(st, 2, K, vs_pass_args(2, g, ping, pong, nullptr, radius[2]), taps[2]);
}

// the radii and taps of a call, checked and copied; the grid and K by tf_check
int vs_check(int K, const int32_t *dims, const int32_t *radius, const double *tx, const double *ty, const double *tz, TfGrid *g, VsTaps taps[3])
{
    TfParams p;
    if (!radius || !tx || !ty || !tz) return fail(MET2_E_INVALID, "NULL argument");
    const int rc = tf_check(K, dims, MET2_TFCE_MODE_EXTENT, 1.0, 1.0, 1.0, 6, g, &p);      // K, the axes and the grid's size
    if (rc != MET2_OK) return rc;
    const double *t[3] = {tx, ty, tz};
    for (int a = 0; a < 3; ++a)
        if (radius[a] > VS_MAX_R) return fail(MET2_E_UNSUPPORTED, "a smoothing radius of at most " + std::to_string(VS_MAX_R) + " voxels per axis");
    for (int a = 0; a < 3; ++a) {
        if (radius[a] < 0) return fail(MET2_E_INVALID, "a radius must be >= 0");
        for (int i = 0; i <= 2 * VS_MAX_R; ++i) taps[a].w[i] = 0.0;
        for (int i = 0; i <= 2 * radius[a]; ++i) {
            if (!std::isfinite(t[a][i]) || t[a][i] < 0.0) return fail(MET2_E_INVALID, "every tap must be finite and >= 0");
            taps[a].w[i] = t[a][i];
        }
        if (!(t[a][radius[a]] > 0.0)) return fail(MET2_E_INVALID, "the centre tap must be > 0");
    }
    return MET2_OK;
}

// the pieces of the work space, in one order for the size entry and the calls.  n_vox = 0: met2_masked_smooth (one map per map and one for N)
struct VsWork {
    DeviceWork::Piece<int> flags;
    DeviceWork::Piece<uint16_t> level;     // the spatial modes only, as are parent and size
    DeviceWork::Piece<int> parent;
    DeviceWork::Piece<unsigned> size;
    DeviceWork::Piece<double> bmap;        // the group entry only, as are pong and mask
    DeviceWork::Piece<double> ping;
    DeviceWork::Piece<double> pong;        // the pseudo-t, which becomes the running sum in the spatial modes
    DeviceWork::Piece<double> norm;
    DeviceWork::Piece<uint8_t> mask;
};
VsWork vs_take(DeviceWork &w, int K, int64_t G, bool group, bool forest)
{
    const size_t cells = (size_t)K * (size_t)G, fc = group && forest ? cells : 0, gc = group ? cells : 0;
    VsWork t{w.take<int>(2), w.take<uint16_t>(fc), w.take<int>(fc), w.take<unsigned>(fc), w.take<double>(gc), w.take<double>(cells),
             w.take<double>(gc), w.take<double>((size_t)G), w.take<uint8_t>(group ? (size_t)G : 0)};
    return t;
}
size_t vs_bytes(const VsWork &t) { return t.mask.off + t.mask.bytes; }

bool vs_mode_ok(int mode)
{
    return mode == MET2_TFCE_MODE_TFCE || mode == MET2_TFCE_MODE_EXTENT || mode == MET2_TFCE_MODE_MASS || mode == MET2_GROUP_VSM_MODE_VOXEL;
}

bool vs_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const char *p = (const char *)a, *q = (const char *)b;
    return p < q + nb && q < p + na;
}

// the launch of gp_moments_kernel for r = 1 .. MET2_GROUP_MAX_R model columns (the caller has checked the range)
void vs_moments(int r, int64_t n_vox, int n, int K, const double *Y, const double *s0, const double *W, const int32_t *at, int64_t dense_stride,
                double *dense_b, double *dense_rho, hipStream_t st)
{
    switch (r) {
#define GP_CASE(R) case R: gp_moments_launch<R + 1>(n_vox, n, K, Y, s0, W, at, dense_stride, dense_b, dense_rho, st); break
        GP_CASE(1); GP_CASE(2); GP_CASE(3); GP_CASE(4); GP_CASE(5); GP_CASE(6); GP_CASE(7); GP_CASE(8);
#undef GP_CASE
    }
}

}  // namespace

extern "C" int met2_group_vsm_limits(int32_t *max_radius, int32_t *max_k, int32_t *tile_axis, int32_t *tile_lines)
{
    if (max_radius) *max_radius = MET2_GROUP_VSM_MAX_RADIUS;
    if (max_k) *max_k = MET2_GROUP_VSM_MAX_K;
    if (tile_axis) *tile_axis = VS_TA;
    if (tile_lines) *tile_lines = VS_TC;
    return MET2_OK;
}

extern "C" int met2_group_vsm_work_bytes(int32_t K, const int32_t dims[3], int64_t n_vox, int32_t mode, int64_t *bytes)
{
    TfGrid g;
    TfParams p;
    const int rc = tf_check(K, dims, MET2_TFCE_MODE_EXTENT, 1.0, 1.0, 1.0, 6, &g, &p);
    if (rc != MET2_OK) return rc;
    if (!bytes || n_vox < 0) return fail(MET2_E_INVALID, "bytes is NULL or n_vox < 0");
    if (!vs_mode_ok(mode)) return fail(MET2_E_INVALID, "mode must be MET2_TFCE_MODE_TFCE, MET2_TFCE_MODE_EXTENT, MET2_TFCE_MODE_MASS or MET2_GROUP_VSM_MODE_VOXEL");
    DeviceWork w(nullptr);
    *bytes = (int64_t)vs_bytes(vs_take(w, K, g.G, n_vox > 0, mode != MET2_GROUP_VSM_MODE_VOXEL));
    return MET2_OK;
}

extern "C" int met2_masked_smooth(int32_t device, int32_t K, const int32_t dims[3], const double *maps, const uint8_t *mask, const int32_t radius[3],
                                  const double *taps_x, const double *taps_y, const double *taps_z, double *out, double *norm_out, void *work,
                                  int64_t work_bytes, void *stream)
{
    TfGrid g;
    VsTaps taps[3];
    const int rc = vs_check(K, dims, radius, taps_x, taps_y, taps_z, &g, taps);
    if (rc != MET2_OK) return rc;
    if (!maps || !out) return fail(MET2_E_INVALID, "NULL argument");
    const size_t map_bytes = (size_t)K * (size_t)g.G * sizeof(double), grid_bytes = (size_t)g.G * sizeof(double);
    if (vs_overlap(maps, map_bytes, out, map_bytes)) return fail(MET2_E_INVALID, "out overlaps maps");
    if (norm_out && (vs_overlap(norm_out, grid_bytes, out, map_bytes) || vs_overlap(norm_out, grid_bytes, maps, map_bytes)))
        return fail(MET2_E_INVALID, "norm_out overlaps maps or out");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork w(st);
    const VsWork t = vs_take(w, K, g.G, false, false);
    if (work && work_bytes < (int64_t)vs_bytes(t)) return fail(MET2_E_INVALID, "the work space is smaller than met2_group_vsm_work_bytes says");
    if (!w.alloc(work)) return w.finish("met2_masked_smooth");
    vs_smooth(st, g, K, maps, mask, radius, taps, t.ping, out);
    if (norm_out) vs_smooth(st, g, 1, nullptr, mask, radius, taps, t.norm, norm_out);
    return w.finish("met2_masked_smooth");
}

extern "C" int met2_group_perm_vsm(int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t K, const double *W,
                                   int32_t two_sided, const int32_t dims[3], const int32_t *at, int32_t mode, double dh, double E, double H,
                                   int32_t connectivity, const int32_t radius[3], const double *taps_x, const double *taps_y, const double *taps_z,
                                   const double *ref, double *first, double *kmax, uint32_t *count, void *work, int64_t work_bytes, void *stream)
{
    const char *who = "met2_group_perm_vsm";
    TfGrid g;
    TfParams p;
    VsTaps taps[3];
    if (r < 1 || n_vox < 1) return fail(MET2_E_INVALID, "r and n_vox must be >= 1");
    if (n <= r) return fail(MET2_E_INVALID, "n must exceed r: no degree of freedom is left");
    if (two_sided != 0 && two_sided != 1) return fail(MET2_E_INVALID, "two_sided must be 0 or 1");
    if (!vs_mode_ok(mode)) return fail(MET2_E_INVALID, "mode must be MET2_TFCE_MODE_TFCE, MET2_TFCE_MODE_EXTENT, MET2_TFCE_MODE_MASS or MET2_GROUP_VSM_MODE_VOXEL");
    const bool voxel = mode == MET2_GROUP_VSM_MODE_VOXEL;
    if (!voxel && two_sided)
        return fail(MET2_E_INVALID, "the spatial modes are one-sided: on |t| a positive and a negative blob would fuse into one cluster");
    int rc = vs_check(K, dims, radius, taps_x, taps_y, taps_z, &g, taps);
    if (rc != MET2_OK) return rc;
    if (!voxel && (rc = tf_check(K, dims, mode, dh, E, H, connectivity, &g, &p)) != MET2_OK) return rc;
    if (n > MET2_GROUP_MAX_N || r > MET2_GROUP_MAX_R)
        return fail(MET2_E_UNSUPPORTED, "n <= " + std::to_string(MET2_GROUP_MAX_N) + " and r <= " + std::to_string(MET2_GROUP_MAX_R));
    if (n_vox > g.G) return fail(MET2_E_INVALID, "more voxels than the grid holds");
    if (!Y || !s0 || !W || !at || !kmax) return fail(MET2_E_INVALID, "NULL argument");
    if (ref && !count) return fail(MET2_E_INVALID, "ref needs count");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork w(st);
    const VsWork t = vs_take(w, K, g.G, true, !voxel);
    if (work && work_bytes < (int64_t)vs_bytes(t)) return fail(MET2_E_INVALID, "the work space is smaller than met2_group_vsm_work_bytes says");
    if (!w.alloc(work)) return w.finish(who);
    int *flags = t.flags;
    uint8_t *mask = t.mask;
    w.ok(hipMemsetAsync(flags, 0, 2 * sizeof(int), st));
    w.ok(hipMemsetAsync(mask, 0, (size_t)g.G, st));
    const dim3 vgrid((unsigned)((n_vox + TF_BLOCK - 1) / TF_BLOCK));
    hipLaunchKernelGGL(tf_mask_kernel, vgrid, dim3(TF_BLOCK), 0, st, n_vox, at, g.G, mask, flags);
    vs_smooth(st, g, 1, nullptr, mask, radius, taps, t.ping, t.pong);                   // N, by way of the two maps' first grids
    w.ok(hipMemcpyAsync(t.norm, t.pong, (size_t)g.G * sizeof(double), hipMemcpyDeviceToDevice, st));
    vs_moments(r, n_vox, n, K, Y, s0, W, at, (int64_t)g.G, t.bmap, t.ping, st);         // rho lands at mask voxels; the first pass reads 0 elsewhere
    vs_smooth(st, g, K, t.ping, mask, radius, taps, t.ping, t.pong);
    const dim3 cgrid((unsigned)((g.G + 255) / 256), (unsigned)K);
    hipLaunchKernelGGL(vs_combine_kernel, cgrid, dim3(256), 0, st, g.G, (const uint8_t *)mask, (const double *)t.bmap, (const double *)t.norm, two_sided,
                       (double *)t.pong);
    const auto bad_at = [&]() {
        const int rc2 = w.finish(who);
        return rc2 != MET2_OK ? rc2 : fail(MET2_E_INVALID, "at must be strictly ascending indices into the grid");
    };
    if (voxel) {
        int host_flags[2] = {0, 0};                                // the gather indexes the maps by `at`: not before `at` is known to be good
        if (!w.ok(hipMemcpyAsync(host_flags, flags, sizeof host_flags, hipMemcpyDeviceToHost, st)) || !w.ok(hipStreamSynchronize(st))) return w.finish(who);
        if (host_flags[1] & TF_ERR_AT) return bad_at();
        hipLaunchKernelGGL(gp_key_kernel, dim3(1), dim3(256), 0, st, K, (unsigned long long *)kmax, 0);
        hipLaunchKernelGGL(vs_gather_kernel, vgrid, dim3(TF_BLOCK), 0, st, n_vox, at, g.G, K, (const double *)t.pong, ref, first,
                           (unsigned long long *)kmax, count);
        hipLaunchKernelGGL(gp_key_kernel, dim3(1), dim3(256), 0, st, K, (unsigned long long *)kmax, 1);
        return w.finish(who);
    }
    const TfForest f{t.level, t.parent, t.size, t.pong, flags};                         // the dense map of the statistic becomes the running sum
    int err = 0;
    if (tf_transform(w, g, K, p, t.pong, mask, f, st, &err) != MET2_OK) return w.finish(who);
    if (err & TF_ERR_AT) return bad_at();
    hipLaunchKernelGGL(gp_key_kernel, dim3(1), dim3(256), 0, st, K, (unsigned long long *)kmax, 0);
    hipLaunchKernelGGL(tf_gather_kernel, vgrid, dim3(TF_BLOCK), 0, st, n_vox, at, g.G, K, p.dh, p.mode == MET2_TFCE_MODE_TFCE ? 1 : 0, (const double *)t.pong,
                       ref, first, (unsigned long long *)kmax, count);
    hipLaunchKernelGGL(gp_key_kernel, dim3(1), dim3(256), 0, st, K, (unsigned long long *)kmax, 1);
    return tf_late_error(w, f.flags, st, who);
}
