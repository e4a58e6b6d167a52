// met2_group.hip -- met2_group_limits, met2_group_perm_stats, met2_group_perm_fstats: the statistic (t of one contrast, F of several) of a
// voxel-wise permutation test for a batch of candidate permutations, with the maximum over the voxels per candidate and the count per voxel of
// the candidates that reach a reference fused in
// (include/met2_hip.h states the contract; group.py holds the partition of the design, the permutation set and the loop over batches).
// Written from that statement and from Winkler et al. (NeuroImage 92:381-397, 2014) and Freedman & Lane (J. Bus. Econ. Stat. 1:292-298, 1983).
// The kernels (gp_stats_kernel, gp_key_kernel) are group_kernel.hpp's, which met2_tfce.hip shares: that header describes them.
// The file is compiled without contraction; every loop is bounded by a shape or a compile-time constant.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_helpers.hpp"
#include "group_kernel.hpp"

#pragma clang fp contract(off)

extern "C" int met2_group_limits(int32_t *max_n, int32_t *max_r, int32_t *max_k, int32_t *voxel_tile)
{
    if (max_n) *max_n = MET2_GROUP_MAX_N;
    if (max_r) *max_r = MET2_GROUP_MAX_R;
    if (max_k) *max_k = MET2_GROUP_MAX_K;
    if (voxel_tile) *voxel_tile = MET2_GROUP_VOXEL_TILE;
    return MET2_OK;
}

extern "C" int met2_group_perm_stats(int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t K, const double *W,
                                     int32_t two_sided, const double *t_ref, double *t_first, double *kmax, uint32_t *count, void *stream)
{
    if (r < 1 || K < 1 || n_vox < 0) return fail(MET2_E_INVALID, "r and K must be >= 1 and n_vox >= 0");
    if (n <= r) return fail(MET2_E_INVALID, "n must exceed r: no degree of freedom is left");
    if (two_sided != 0 && two_sided != 1) return fail(MET2_E_INVALID, "two_sided must be 0 or 1");
    if (n > MET2_GROUP_MAX_N || r > MET2_GROUP_MAX_R || K > MET2_GROUP_MAX_K)
        return fail(MET2_E_UNSUPPORTED, "n <= " + std::to_string(MET2_GROUP_MAX_N) + ", r <= " + std::to_string(MET2_GROUP_MAX_R) + " and K <= " +
                                            std::to_string(MET2_GROUP_MAX_K) + " per launch");
    if (n_vox > (int64_t)0x7fffffff * GP_TILE) return fail(MET2_E_UNSUPPORTED, "too many voxels for one launch");
    if (!W || !kmax || (n_vox > 0 && (!Y || !s0))) return fail(MET2_E_INVALID, "NULL argument");
    if (t_ref && !count) return fail(MET2_E_INVALID, "t_ref needs count");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const dim3 kgrid((K + 255) / 256);
    hipLaunchKernelGGL(gp_key_kernel, kgrid, dim3(256), 0, st, K, (unsigned long long *)kmax, 0);
    if (n_vox > 0) gp_launch_r<false>(r, n_vox, n, K, Y, s0, W, two_sided, t_ref, t_first, kmax, count, nullptr, 0, nullptr, st);
    hipLaunchKernelGGL(gp_key_kernel, kgrid, dim3(256), 0, st, K, (unsigned long long *)kmax, 1);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_group_perm_fstats(int32_t device, int32_t n, int64_t n_vox, const double *Y, const double *s0, int32_t r, int32_t s, double scale,
                                      int32_t K, const double *W, const double *f_ref, double *f_first, double *kmax, uint32_t *count, void *stream)
{
    if (r < 1 || K < 1 || n_vox < 0) return fail(MET2_E_INVALID, "r and K must be >= 1 and n_vox >= 0");
    if (s < 1 || s > r) return fail(MET2_E_INVALID, "s must lie in 1 .. r");
    if (n <= r) return fail(MET2_E_INVALID, "n must exceed r: no degree of freedom is left");
    if (!std::isfinite(scale) || scale <= 0.0) return fail(MET2_E_INVALID, "scale must be finite and > 0");
    if (n > MET2_GROUP_MAX_N || r > MET2_GROUP_MAX_R || K > MET2_GROUP_MAX_K)
        return fail(MET2_E_UNSUPPORTED, "n <= " + std::to_string(MET2_GROUP_MAX_N) + ", r <= " + std::to_string(MET2_GROUP_MAX_R) + " and K <= " +
                                            std::to_string(MET2_GROUP_MAX_K) + " per launch");
    if (n_vox > (int64_t)0x7fffffff * GP_TILE) return fail(MET2_E_UNSUPPORTED, "too many voxels for one launch");
    if (!W || !kmax || (n_vox > 0 && (!Y || !s0))) return fail(MET2_E_INVALID, "NULL argument");
    if (f_ref && !count) return fail(MET2_E_INVALID, "f_ref needs count");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const dim3 kgrid((K + 255) / 256);
    hipLaunchKernelGGL(gp_key_kernel, kgrid, dim3(256), 0, st, K, (unsigned long long *)kmax, 0);
    if (n_vox > 0) gp_flaunch_r<false>(r, n_vox, n, K, Y, s0, W, s, scale, f_ref, f_first, kmax, count, nullptr, 0, nullptr, st);
    hipLaunchKernelGGL(gp_key_kernel, kgrid, dim3(256), 0, st, K, (unsigned long long *)kmax, 1);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}
