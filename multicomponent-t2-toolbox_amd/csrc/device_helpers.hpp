// device_helpers.hpp -- the small device functions that more than one unit needs, each stated once: contraction-free arithmetic, the wave's
// LDS hand-over, numpy's nan-last order, the next power of two, and the fixed-order sums over a wave (xor butterfly) and over 256 threads.
// Everything sits in an unnamed namespace and is inlined: each translation unit compiles its own copy from this one text.
// (met2::wave_sum of wave_ops.hpp adds in another order, DPP's; hence the butterfly's own name.)
#pragma once
#include <hip/hip_runtime.h>

namespace {

// One rounding each.  The toolchain's __dmul_rn, __dadd_rn and __dsub_rn are the plain operators, which the compiler may contract into a fused
// multiply-add once they are inlined; under this pragma it may not, so these are what those names promise.
__device__ __forceinline__ double rn_mul(double x, double y)
{
#pragma clang fp contract(off)
    return x * y;
}
__device__ __forceinline__ double rn_add(double x, double y)
{
#pragma clang fp contract(off)
    return x + y;
}
__device__ __forceinline__ double rn_sub(double x, double y)
{
#pragma clang fp contract(off)
    return x - y;
}

// The lanes of ONE wave exchange values through LDS: a wave's LDS accesses complete in program order, so what is needed is that the compiler
// keeps them in it (the fences) and that the wave is converged (the barrier, which emits no instruction).  A workgroup barrier would tie
// waves that work on series of their own to each other.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// numpy's ordering for np.sort: nan last
__device__ __forceinline__ bool nan_last_gt(double a, double b) { return a > b || (a != a && b == b); }

__host__ __device__ __forceinline__ int next_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// the sum over the wave's 64 lanes by xor butterfly: every lane adds the same two numbers, so all lanes hold the same bits, on every run
template <class T> __device__ __forceinline__ T wave_sum_xor(T v)      // double and int
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the sum over a workgroup of 256 threads in a fixed order, returned to every thread; red: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double *red)
{
    v = wave_sum_xor(v);
    __syncthreads();                                                  // the previous call's readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace
