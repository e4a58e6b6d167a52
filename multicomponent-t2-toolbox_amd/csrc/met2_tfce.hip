// met2_tfce.hip -- met2_tfce_limits, met2_tfce_work_bytes, met2_tfce, met2_group_perm_tfce, met2_group_perm_ftfce (the same on F): threshold-free cluster enhancement, cluster
// extent and cluster mass of a batch of statistic maps, and each as the statistic of the voxel-wise permutation test (include/met2_hip.h states the
// definitions and the contract; group.py holds the loop over batches).  The kernels, the work space's layout and the walk over the levels
// are tfce_kernel.hpp's, which met2_group_vsm.hip shares: that header describes them.  Compiled without contraction.
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

extern "C" int met2_tfce_limits(int32_t *max_k, int32_t *max_steps)
{
    if (max_k) *max_k = MET2_TFCE_MAX_K;
    if (max_steps) *max_steps = MET2_TFCE_MAX_STEPS;
    return MET2_OK;
}

extern "C" int met2_tfce_work_bytes(int32_t K, const int32_t dims[3], int64_t n_vox, int64_t *bytes)
{
    TfGrid g;
    TfParams p;
    const int rc = tf_check(K, dims, MET2_TFCE_MODE_EXTENT, 1.0, 1.0, 1.0, 6, &g, &p);
    if (rc != MET2_OK) return rc;
    if (!bytes || n_vox < 0) return fail(MET2_E_INVALID, "bytes is NULL or n_vox < 0");
    DeviceWork w(nullptr);
    *bytes = (int64_t)tf_bytes(tf_take(w, K, g.G, n_vox > 0));
    return MET2_OK;
}

extern "C" int met2_tfce(int32_t device, int32_t K, const int32_t dims[3], const double *maps, const uint8_t *mask, int32_t mode, double dh, double E,
                         double H, int32_t connectivity, double *out, double *kmax, void *work, int64_t work_bytes, void *stream)
{
    TfGrid g;
    TfParams p;
    const int rc = tf_check(K, dims, mode, dh, E, H, connectivity, &g, &p);
    if (rc != MET2_OK) return rc;
    if (!maps || !out) return fail(MET2_E_INVALID, "NULL argument");
    const int64_t cells = (int64_t)K * g.G;
    if (maps < out + cells && out < maps + cells) return fail(MET2_E_INVALID, "out overlaps maps");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork w(st);
    const TfWork t = tf_take(w, K, g.G, false);
    if (work && work_bytes < (int64_t)tf_bytes(t)) return fail(MET2_E_INVALID, "the work space is smaller than met2_tfce_work_bytes says");
    if (!w.alloc(work)) return w.finish("met2_tfce");
    const TfForest f{t.level, t.parent, t.size, out, t.flags};
    w.ok(hipMemsetAsync(f.flags, 0, 2 * sizeof(int), st));
    int err = 0;
    if (tf_transform(w, g, K, p, maps, mask, f, st, &err) != MET2_OK) return w.finish("met2_tfce");
    const dim3 grid((unsigned)((g.G + TF_BLOCK - 1) / TF_BLOCK), (unsigned)K);
    if (kmax) hipLaunchKernelGGL(gp_key_kernel, dim3(1), dim3(256), 0, st, K, (unsigned long long *)kmax, 0);
    hipLaunchKernelGGL(tf_finish_kernel, grid, dim3(TF_BLOCK), 0, st, g, p.dh, p.mode == MET2_TFCE_MODE_TFCE ? 1 : 0, out, (unsigned long long *)kmax);
    if (kmax) hipLaunchKernelGGL(gp_key_kernel, dim3(1), dim3(256), 0, st, K, (unsigned long long *)kmax, 1);
    return tf_late_error(w, f.flags, st, "met2_tfce");
}

namespace {

// the two group entries: s = 0 is the t statistic (W [K][r + 1][n]), s >= 1 the F statistic over the first s of r rows (W [K][r][n])
int tf_group_entry(const char *who, int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t s, double scale,
                   int32_t K, const double *W, const int32_t dims[3], const int32_t *at, int32_t mode, double dh, double E, double H,
                   int32_t connectivity, const double *ref, double *first, double *kmax, uint32_t *count, void *work, int64_t work_bytes, void *stream)
{
    TfGrid g;
    TfParams p;
    if (r < 1 || n_vox < 1) return fail(MET2_E_INVALID, "r and n_vox must be >= 1");
    if (n <= r) return fail(MET2_E_INVALID, "n must exceed r: no degree of freedom is left");
    const int rc = tf_check(K, dims, mode, dh, E, H, connectivity, &g, &p);
    if (rc != MET2_OK) return rc;
    if (n > MET2_GROUP_MAX_N || r > MET2_GROUP_MAX_R)
        return fail(MET2_E_UNSUPPORTED, "n <= " + std::to_string(MET2_GROUP_MAX_N) + " and r <= " + std::to_string(MET2_GROUP_MAX_R));
    if (n_vox > g.G) return fail(MET2_E_INVALID, "more voxels than the grid holds");
    if (!Y || !s0 || !W || !at || !kmax) return fail(MET2_E_INVALID, "NULL argument");
    if (ref && !count) return fail(MET2_E_INVALID, "ref needs count");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    DeviceWork w(st);
    const TfWork t = tf_take(w, K, g.G, true);
    if (work && work_bytes < (int64_t)tf_bytes(t)) return fail(MET2_E_INVALID, "the work space is smaller than met2_tfce_work_bytes says");
    if (!w.alloc(work)) return w.finish(who);
    const TfForest f{t.level, t.parent, t.size, t.dense, t.flags};                      // the dense map of the statistic becomes the running sum
    w.ok(hipMemsetAsync(f.flags, 0, 2 * sizeof(int), st));
    w.ok(hipMemsetAsync((uint8_t *)t.mask, 0, (size_t)g.G, st));
    const dim3 vgrid((unsigned)((n_vox + TF_BLOCK - 1) / TF_BLOCK));
    hipLaunchKernelGGL(tf_mask_kernel, vgrid, dim3(TF_BLOCK), 0, st, n_vox, at, g.G, (uint8_t *)t.mask, f.flags);
    if (s >= 1)
        gp_flaunch_r<true>(r, n_vox, n, K, Y, s0, W, s, scale, nullptr, nullptr, nullptr, nullptr, at, (int64_t)g.G, (double *)t.dense, st);
    else
        gp_launch_r<true>(r, n_vox, n, K, Y, s0, W, 0, nullptr, nullptr, nullptr, nullptr, at, (int64_t)g.G, (double *)t.dense, st);
    int err = 0;
    if (tf_transform(w, g, K, p, t.dense, t.mask, f, st, &err) != MET2_OK) return w.finish(who);
    if (err & TF_ERR_AT) {
        const int rc2 = w.finish(who);
        return rc2 != MET2_OK ? rc2 : fail(MET2_E_INVALID, "at must be strictly ascending indices into the grid");
    }
    hipLaunchKernelGGL(gp_key_kernel, dim3(1), dim3(256), 0, st, K, (unsigned long long *)kmax, 0);
    hipLaunchKernelGGL(tf_gather_kernel, vgrid, dim3(TF_BLOCK), 0, st, n_vox, at, g.G, K, p.dh, p.mode == MET2_TFCE_MODE_TFCE ? 1 : 0, (const double *)t.dense,
                       ref, first, (unsigned long long *)kmax, count);
    hipLaunchKernelGGL(gp_key_kernel, dim3(1), dim3(256), 0, st, K, (unsigned long long *)kmax, 1);
    return tf_late_error(w, f.flags, st, who);
}

}  // namespace

extern "C" int met2_group_perm_tfce(int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t K, const double *W,
                                    const int32_t dims[3], const int32_t *at, int32_t mode, double dh, double E, double H, int32_t connectivity,
                                    const double *ref, double *first, double *kmax, uint32_t *count, void *work, int64_t work_bytes, void *stream)
{
    return tf_group_entry("met2_group_perm_tfce", device, n, n_vox, Y, s0, r, 0, 1.0, K, W, dims, at, mode, dh, E, H, connectivity, ref, first, kmax,
                          count, work, work_bytes, stream);
}

extern "C" int met2_group_perm_ftfce(int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t s, double scale,
                                     int32_t K, const double *W, const int32_t dims[3], const int32_t *at, int32_t mode, double dh, double E, double H,
                                     int32_t connectivity, const double *ref, double *first, double *kmax, uint32_t *count, void *work,
                                     int64_t work_bytes, void *stream)
{
    if (s < 1 || s > r) return fail(MET2_E_INVALID, "s must lie in 1 .. r");
    if (!std::isfinite(scale) || scale <= 0.0) return fail(MET2_E_INVALID, "scale must be finite and > 0");
    return tf_group_entry("met2_group_perm_ftfce", device, n, n_vox, Y, s0, r, s, scale, K, W, dims, at, mode, dh, E, H, connectivity, ref, first,
                          kmax, count, work, work_bytes, stream);
}
