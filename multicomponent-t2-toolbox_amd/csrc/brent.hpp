// brent.hpp -- scipy's bounded Brent search restated for the device.  Needs nothing but the compiler's builtins: the lambda searches of the
// fit kernels (fit_kernel.hpp) and the FA spline selection (met2_prefilter.hip) share it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// The searches run redundantly on all lanes, on wave-uniform doubles that the VALU computes into vector registers: eleven of them live across
// every objective evaluation (a whole NNLS solve), 22 VGPRs of the solver's budget.  uni() moves such a value into a scalar register pair
// (v_readfirstlane x 2); what the scalar file cannot hold the compiler keeps in the lanes of one VGPR (v_writelane), 64 scalars per register.
template <bool PIN>
__device__ __forceinline__ double uni(double v)
{
    if constexpr (PIN) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    } else return v;
}
#define MET2_UNI_PIN() do { a = uni<PIN>(a); b = uni<PIN>(b); fulc = uni<PIN>(fulc); nfc = uni<PIN>(nfc); xf = uni<PIN>(xf); rat = uni<PIN>(rat); e = uni<PIN>(e); \
                            x = uni<PIN>(x); fx = uni<PIN>(fx); ffulc = uni<PIN>(ffulc); fnfc = uni<PIN>(fnfc); } while (0)

// SciPy's bounded Brent (scipy.optimize.fminbound, called at algorithms.py:219,280 and
// bayesian_interpolation.py:101), restated; executed redundantly by all lanes on uniform values.
// on_best() is called whenever the abscissa just evaluated becomes Brent's best point xf (the value fminbound returns): callers
// keep the solver state of that evaluation and skip the solve scipy's callers repeat at the returned lambda.
template <bool PIN, class F, class G>
__device__ __forceinline__ double fminbound_dev(F &&fn, G &&on_best, double x1, double x2, double xatol, int maxfun, int &flag)
{
    const double sqrt_eps = sqrt(2.2e-16);
    const double golden_mean = 0.5 * (3.0 - sqrt(5.0));
    double a = x1, b = x2;
    double fulc = a + golden_mean * (b - a);
    double nfc = fulc, xf = fulc;
    double rat = 0.0, e = 0.0;
    double x = xf;
    double fx = fn(x);
    on_best();
    int num = 1;
    flag = 0;
    double fu = INFINITY;
    double ffulc = fx, fnfc = fx;
    double xm = 0.5 * (a + b);
    double tol1 = sqrt_eps * fabs(xf) + xatol / 3.0;
    double tol2 = 2.0 * tol1;
    while (fabs(xf - xm) > (tol2 - 0.5 * (b - a))) {
        bool golden = true;
        if (fabs(e) > tol1) {
            golden = false;
            double r = (xf - nfc) * (fx - ffulc);
            double q = (xf - fulc) * (fx - fnfc);
            double p = (xf - fulc) * q - (xf - nfc) * r;
            q = 2.0 * (q - r);
            if (q > 0.0) p = -p;
            q = fabs(q);
            r = e;
            e = rat;
            if ((fabs(p) < fabs(0.5 * q * r)) && (p > q * (a - xf)) && (p < q * (b - xf))) {
                rat = (p + 0.0) / q;
                x = xf + rat;
                if (((x - a) < tol2) || ((b - x) < tol2)) {
                    double d = xm - xf;
                    double si = (double)((d > 0.0) - (d < 0.0) + (d == 0.0));
                    rat = tol1 * si;
                }
            } else golden = true;
        }
        if (golden) {
            e = (xf >= xm) ? a - xf : b - xf;
            rat = golden_mean * e;
        }
        double si = (double)((rat > 0.0) - (rat < 0.0) + (rat == 0.0));
        double ar = fabs(rat);
        x = xf + si * (ar > tol1 ? ar : tol1);
        MET2_UNI_PIN();
        fu = fn(x);
        num++;
        if (fu <= fx) {
            if (x >= xf) a = xf; else b = xf;
            fulc = nfc; ffulc = fnfc;
            nfc = xf; fnfc = fx;
            xf = x; fx = fu;
            on_best();
        } else {
            if (x < xf) a = x; else b = x;
            if ((fu <= fnfc) || (nfc == xf)) {
                fulc = nfc; ffulc = fnfc;
                nfc = x; fnfc = fu;
            } else if ((fu <= ffulc) || (fulc == xf) || (fulc == nfc)) {
                fulc = x; ffulc = fu;
            }
        }
        xm = 0.5 * (a + b);
        tol1 = sqrt_eps * fabs(xf) + xatol / 3.0;
        tol2 = 2.0 * tol1;
        if (num >= maxfun) { flag = 1; break; }
    }
    if (isnan(xf) || isnan(fx) || isnan(fu)) flag = 2;
    return xf;
}
