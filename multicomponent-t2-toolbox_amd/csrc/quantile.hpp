// quantile.hpp -- np.quantile(values, p, method='linear') on order statistics: the one copy of the bit-level contract, shared by the bootstrap
// statistics (met2_bootstrap.hip, which sorts a series in LDS) and the label statistics (met2_stats.hip, which also selects the two order
// statistics by radix and never holds a sorted series).
#pragma once
#include <hip/hip_runtime.h>

namespace met2 {

// h = (n - 1) p  ->  the two order statistics i0 = floor(h), i1 = i0 + 1 (both n - 1 at the upper end) and the weight g = h - floor(h)
__device__ __forceinline__ void quantile_position(int n, double p, int &i0, int &i1, double &g)
{
#pragma clang fp contract(off)
    const double h = (double)(n - 1) * p;
    const double fl = floor(h);
    i0 = (int)fl;
    i1 = i0 + 1;
    if (h >= (double)(n - 1)) i0 = i1 = n - 1;
    g = h - fl;
}

// numpy's _lerp between the order statistics a <= b, including its t >= 0.5 branch.
// No contraction: a fused multiply-add would differ from numpy in the last bit.
__device__ __forceinline__ double quantile_lerp(double a, double b, double g)
{
#pragma clang fp contract(off)
    const double d = b - a;
    return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

// np.quantile(values, p) with method 'linear' on the sorted values (nan last)
__device__ __forceinline__ double quantile_sorted(const double *s, int n, double p)
{
    if (s[n - 1] != s[n - 1]) return s[n - 1];                 // a nan among the values: numpy returns nan
    int i0, i1;
    double g;
    quantile_position(n, p, i0, i1, g);
    return quantile_lerp(s[i0], s[i1], g);
}

}  // namespace met2
