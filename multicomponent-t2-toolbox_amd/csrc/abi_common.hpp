// abi_common.hpp -- error plumbing and the environment switches shared by the translation units of libmet2_hip.so.  (The plan and the
// hidden functions that cross units: plan.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>

namespace met2 {
// records `msg` as the calling thread's last error (met2_last_error) and returns `code`; defined in met2_hip.hip
__attribute__((visibility("hidden"))) int abi_fail(int code, const std::string &msg);
}  // namespace met2

static inline int fail(int code, const std::string &msg) { return met2::abi_fail(code, msg); }

// The switches the shipped library reads from the environment, at every call (the tests flip them between fits on one plan); set means on:
//   MET2_NO_SEED      every voxel grows its first passive set from the lambda = 0 solution, not from the plan's seed (test_gpu_round2.py)
//   MET2_GCV_FULL     GCV's trace from the (m + 1) x (m + 1) form, never the low-rank one (test_round4.py)
//   MET2_FA_NOPRUNE   the brute-force FA walk visits every flip angle, no lower bounds (test_round4.py)
//   MET2_LC_RESTART   queued L-curve voxels start their sweep over in the spill-over kernel (test_round5.py)
//   MET2_HOST_BLOCKS  met2_fit_host gives its plans whole blocks, not runs of 4 096 voxels (test_round5.py)
//   MET2_REFAC_PAIR   the warm re-factorisation keeps to its pair loop, no packed leg (test_gpu_refactor_packed.py)
//   MET2_REFAC_COUNT  the fit kernels count the re-factorisations that took the packed leg (met2_refac_packed_calls; slow: one atomic per call)
//   MET2_SUBST_REF    the fit kernels' triangular substitutions at one bin per lane run their reference loops, not the lean ones (test_gpu_subst_lean.py)
//                     (fit_kernel and its spill-over kernels only: the plan's seed kernel, the Bayes table and the flip-angle walk keep the lean loops)
//   MET2_ROWWALK_REF  the fit kernels' model signal at one bin per lane runs on the whole wave with one lane read per passive position, not on two
//                     half waves (test_gpu_row_walk.py; same reach as MET2_SUBST_REF)
//   MET2_DUAL_REF     the fit kernels' dual at one bin per lane takes x by lane reads, never from its table in the wave's LDS region
//                     (test_gpu_dual_lds.py; the X2 and NNLS fit kernels: no other kernel has the table)
//   MET2_DUAL_TAB     launches of at most one wave per SIMD, which take the lane reads by default, keep the table (test_gpu_dual_lds.py: its
//                     1 024-voxel cases); MET2_DUAL_REF wins over it
//   MET2_KMAX=<k>     capacity of the fit kernels' passive set in LDS, 8 <= k < nT2 (test_value below; test_gpu_dual_lds.py: the capacity at
//                     which the table's validity limit lies inside the sets the solves reach)
//   MET2_DEBUG        synchronous launches with progress lines on stderr
static inline bool test_switch(const char *name) { return getenv(name) != nullptr; }
// a test variable that carries a number: its value if it lies in [lo, hi], else dflt
static inline int test_value(const char *name, int lo, int hi, int dflt)
{
    if (const char *e = getenv(name)) { const int v = atoi(e); if (v >= lo && v <= hi) return v; }
    return dflt;
}

// Development knobs (first-pass capacity, waves per CU, queue granularity, ...): read only by libraries built with -DMET2_TUNING, which take a
// value in [lo, hi]; every other build uses dflt.
static inline int tuning_env(const char *name, int lo, int hi, int dflt)
{
#ifdef MET2_TUNING
    if (const char *e = getenv(name)) { const int v = atoi(e); if (v >= lo && v <= hi) return v; }
#else
    (void)name; (void)lo; (void)hi;
#endif
    return dflt;
}

// makes `dev` current for the duration of a C-ABI call and puts the caller's device back afterwards
struct DevGuard {
    int prev = -1;
    hipError_t err;
    explicit DevGuard(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) err = hipSetDevice(dev); else if (err == hipSuccess) prev = -1;
    }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define USE_DEVICE(dev)                                                                                \
    DevGuard dev_guard_(dev);                                                                          \
    if (dev_guard_.err != hipSuccess) return fail(MET2_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dev_guard_.err))

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(MET2_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
