// resample_checks.hpp -- what the entries that sample through resample_taps.hpp share on the host side and around a launch: the argument
// checks of a grid and of a transform, the geometry they pass to a kernel, the launch width and the split of a destination index.
// met2_resample.hip and met2_warp.hip include it after resample_taps.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "resample_taps.hpp"

namespace {

#define RS_BLOCK 256
#define RS_MAX_GRID (1 << 20)              // blocks of a launch; the kernels stride over what is left

__device__ __forceinline__ void rs_split(int64_t w, const RsGeom &G, int &i, int &j, int &k)
{
    k = (int)(w % G.mz);
    const int64_t r = w / G.mz;
    j = (int)(r % G.my);
    i = (int)(r / G.my);
}

[[maybe_unused]] int rs_grid(int64_t items, int64_t per_block)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, RS_MAX_GRID));
}

[[maybe_unused]] int rs_check_dims(const int32_t *d, const char *what, bool source)
{
    if (!d) return fail(MET2_E_INVALID, std::string("NULL ") + what + " dims");
    int64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        if (d[a] < 1) return fail(MET2_E_INVALID, std::string("every ") + what + " axis needs at least one voxel");
        if (source && d[a] > MET2_RESAMPLE_MAX_AXIS) return fail(MET2_E_UNSUPPORTED, "a source axis holds more than 512 voxels");
        n *= d[a];
        if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "the destination holds more than 2^31 - 1 voxels");
    }
    return MET2_OK;
}

[[maybe_unused]] int rs_check_series(int32_t n_series)
{
    if (n_series < 1) return fail(MET2_E_INVALID, "resampling needs at least one series");
    if (n_series > MET2_RESAMPLE_MAX_SERIES) return fail(MET2_E_UNSUPPORTED, "more than 32768 series");
    return MET2_OK;
}

[[maybe_unused]] int rs_check_transform(const double *A)
{
    if (!A) return fail(MET2_E_INVALID, "NULL transform");
    for (int e = 0; e < 12; ++e)
        if (!std::isfinite(A[e])) return fail(MET2_E_INVALID, "every entry of the transform must be finite");
    return MET2_OK;
}

[[maybe_unused]] RsGeom rs_geom(const int32_t *sd, const int32_t *dd, const double *A)
{
    RsGeom G;
    G.nx = sd[0]; G.ny = sd[1]; G.nz = sd[2];
    G.mx = dd[0]; G.my = dd[1]; G.mz = dd[2];
    for (int e = 0; e < 12; ++e) G.A[e] = A[e];
    return G;
}

}  // namespace
