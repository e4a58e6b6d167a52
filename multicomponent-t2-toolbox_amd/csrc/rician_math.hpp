// rician_math.hpp -- the Rician mean, its bias and its inverse in float64 (the contract of include/met2_hip.h, "Rician noise floor").
// Plain C++ without a device call in it, so that a host program can run the same text (RICIAN_HD is empty there).
//   i0e, i1e   exponentially scaled modified Bessel functions: Chebyshev series in x / 4 - 1 up to x = 8 and, behind a factor 1 / sqrt(x), in
//              16 / x - 1 above (rician_bessel.hpp, generated from mpmath); relative error below 1e-15 over x >= 0
//   mean1(r)   m(r, 1) = sqrt(pi / 2) [(1 + t) i0e(t / 2) + t i1e(t / 2)], t = r^2 / 2, for 0 <= r <= 1024
//   bias       b(A, sigma) = sigma mean1(A / sigma) - A up to A / sigma = 1024; above, the asymptotic series
//              b / sigma = 1 / (2 r) + 1 / (8 r^3) + 3 / (16 r^5) (next term 75 / (128 r^7) < 1e-21), which neither cancels nor overflows
//   inverse    the root of m(A, sigma) = M by Newton's method kept inside a bracket
#pragma once
#include <math.h>

#include "rician_bessel.hpp"

// Every kernel must give the same bits for the same arguments (met2_rician_step's output is checked against met2_rician_bias's), so the
// compiler fuses nothing on its own from here on: the multiply-adds that are wanted are written as fma().
#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifndef RICIAN_HD
#define RICIAN_HD __host__ __device__ __forceinline__
#endif

namespace met2 {

#define MET2_RICIAN_FLOOR 1.2533141373155002512      // sqrt(pi / 2): the mean of a Rayleigh magnitude at sigma = 1
#define MET2_RICIAN_ASYM 1024.0                      // A / sigma above which the bias is taken from its asymptotic series
#define MET2_RICIAN_NEWTON 64                        // iteration cap of the inverse (reached only on inputs that are not numbers)

// c[0] / 2 + sum_{k >= 1} c[k] T_k(y) by Clenshaw's recurrence
template <int N>
RICIAN_HD double cheb_eval(const double (&c)[N], double y)
{
    double b0 = 0.0, b1 = 0.0;
    const double y2 = 2.0 * y;
#pragma unroll
    for (int k = N - 1; k >= 1; --k) { const double t = fma(y2, b0, c[k] - b1); b1 = b0; b0 = t; }
    return fma(y, b0, 0.5 * c[0] - b1);
}

// i0e(x) and i1e(x), x >= 0
RICIAN_HD void bessel_i01e(double x, double &i0, double &i1)
{
    if (x <= 8.0) {
        constexpr double c0[MET2_I0S_N] = MET2_I0S_COEFFS;
        constexpr double c1[MET2_I1S_N] = MET2_I1S_COEFFS;
        const double y = 0.25 * x - 1.0;
        i0 = cheb_eval(c0, y);
        i1 = x * cheb_eval(c1, y);
    } else {
        constexpr double c0[MET2_I0L_N] = MET2_I0L_COEFFS;
        constexpr double c1[MET2_I1L_N] = MET2_I1L_COEFFS;
        const double y = 16.0 / x - 1.0, r = 1.0 / sqrt(x);
        i0 = cheb_eval(c0, y) * r;
        i1 = cheb_eval(c1, y) * r;
    }
}

// m(r, 1) for 0 <= r <= MET2_RICIAN_ASYM; *slope (may be NULL) gets dm / dr = sqrt(pi / 2) r (i0e + i1e) / 2
RICIAN_HD double rician_mean1(double r, double *slope)
{
    const double t = 0.5 * r * r;
    double i0, i1;
    bessel_i01e(0.5 * t, i0, i1);
    if (slope) *slope = MET2_RICIAN_FLOOR * r * 0.5 * (i0 + i1);
    return MET2_RICIAN_FLOOR * ((1.0 + t) * i0 + t * i1);
}

// b(A, sigma) = m(A, sigma) - A;  A < 0 reads as 0, sigma = 0 gives 0
RICIAN_HD double rician_bias(double A, double sigma)
{
    if (!(sigma > 0.0)) return 0.0;
    A = fmax(A, 0.0);
    const double r = A / sigma;
    if (r > MET2_RICIAN_ASYM) {
        const double q = 1.0 / r, q2 = q * q;
        return sigma * (q * (0.5 + q2 * (0.125 + q2 * 0.1875)));
    }
    return sigma * rician_mean1(r, nullptr) - A;
}

// A = m^-1(M, sigma): 0 for M <= sigma sqrt(pi / 2) (and for sigma = 0: M itself).  m is increasing in A and
// A <= m <= sqrt(A^2 + 2 sigma^2) (the mean lies below the root of the second moment), so in units of sigma the root lies in
// [sqrt(max(mu^2 - 2, 0)), mu]; a Newton step that leaves the bracket is replaced by the bracket's midpoint.  Stops at
// |m(a) - mu| <= 2^-47 max(mu, 1) -- float64 evaluation of m leaves about 2^-50 mu of rounding -- or at a step below two units of a.
RICIAN_HD double rician_inverse(double M, double sigma)
{
    if (!(sigma > 0.0)) return M;
    const double mu = M / sigma;
    if (!(mu > MET2_RICIAN_FLOOR)) return 0.0;
    if (mu > MET2_RICIAN_ASYM + 1.0) {
        // a + 1 / (2 a) + 1 / (8 a^3) + 3 / (16 a^5) = mu: a sweep of the fixed point gains a factor 2 a^2 > 2e6, three from a = mu are plenty
        double a = mu;
        for (int i = 0; i < 3; ++i) { const double q = 1.0 / a, q2 = q * q; a = mu - q * (0.5 + q2 * (0.125 + q2 * 0.1875)); }
        return sigma * a;
    }
    double lo = sqrt(fmax(mu * mu - 2.0, 0.0)), hi = mu;
    double a = sqrt(mu * mu - 1.0);                      // exact for a Gaussian magnitude; inside the bracket
    const double tol = 7.105427357601002e-15 * fmax(mu, 1.0);
    for (int it = 0; it < MET2_RICIAN_NEWTON; ++it) {
        double s;
        const double f = rician_mean1(a, &s) - mu;
        if (fabs(f) <= tol) break;
        if (f > 0.0) hi = a; else lo = a;
        double an = a - f / s;
        if (!(an > lo && an < hi)) an = 0.5 * (lo + hi);
        const bool still = fabs(an - a) <= 4.440892098500626e-16 * a;
        a = an;
        if (still) break;
    }
    return sigma * a;
}

}  // namespace met2
