// met2_eval.hip -- met2_synth_two_lobe / met2_eval_voxel_metrics / met2_eval_reduce: the reference's Monte-Carlo accuracy study on the GPU.
//
// scripts_synthetic_data_evaluation/Paper_Comparison/evaluate_all_methods_two_lobes_SNR{50_150,150_300,_Inf}.py draws two-lobe voxels,
// fits them with ten methods and scores every method on 13 error metrics and the mean / std of the selected lambda.  The fits are the
// library's (met2_fit); this file holds what surrounds them:
//   synth_two_lobe_kernel     the generator of :156-190, :376-428 (one wave per voxel; the wave's lanes carry the EPG states of one grid point)
//   eval_voxel_metrics_kernel estimate_error_metrics of :59-74 with scipy's find_peaks, jensenshannon and wasserstein_distance restated
//                             (one wave per voxel, bitonic sort in LDS)
//   eval_reduce_kernel        compute_multi_metrics of :77-123 and the lambda statistics (one workgroup, fixed reduction order)
// A voxel's draws depend on (seed, voxel id, stream) alone (counter-based Philox4x32-10), so the data do not depend on chunking, voxel
// order or call splitting.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_helpers.hpp"
#include "philox.hpp"
#include "plan.hpp"
#include "wave_ops.hpp"

namespace {

#define MET2_EVAL_NGRID 1000       // the high-resolution pdf grid, linspace(1, 300, 1000) (:179-180)
#define MET2_EVAL_MAX_T2 128
#define MET2_EVAL_MAX_TE 64
#define MET2_STREAM_PARAM 1u       // Philox counter word c1: the voxel's parameter draws
#define MET2_STREAM_NOISE 2u       //                          its Rician noise (c0 = echo)

struct SynthArgs {
    int64_t n, v0;                  // voxels of the call, absolute id of the first
    int nte, nt2;
    uint32_t k0, k1;                // the seed's two halves
    met2_synth_params P;
    bool noisy;
    const double *t2s;              // the plan's T2 grid [nt2]
    double cut_m;
    double *data;                   // [n][nte]
    double *dist2;                  // [n][nt2]
    double *truth;                  // [MET2_EVAL_NTRUTH][n]
};

// numpy's linspace(1, 300, 1000): j * step + start, the last point set to stop.  No contraction: the re-binning compares these values
// with the bin edges, so they must be numpy's to the bit.
__device__ __forceinline__ double hires_t2(int j, double step)
{
#pragma clang fp contract(off)
    return j == MET2_EVAL_NGRID - 1 ? 300.0 : (double)j * step + 1.0;
}

__device__ __forceinline__ double draw(const uint32_t w[8], int i, double lo, double hi) { return lo + (hi - lo) * met2::u01_co(w[2 * (i & 3)], w[2 * (i & 3) + 1]); }

// one wave (one workgroup) per voxel.  The pdf lives in LDS; the EPG train of each of the 1000 grid points runs with lane l holding the
// states (F+_k, F-_k, Z_k), k = l + 1 (the recursion of synth.epg_table / epg.py:64-153); lane e accumulates echo e of the signal.
__global__ __launch_bounds__(64) void synth_two_lobe_kernel(SynthArgs A)
{
    __shared__ double pdf[MET2_EVAL_NGRID];
    const int lane = threadIdx.x;
    const int64_t lv = blockIdx.x;
    const uint64_t id = (uint64_t)(A.v0 + lv);
    const met2_synth_params &P = A.P;
    // parameters: two Philox blocks of the parameter stream, eight 53-bit uniforms (the seventh and eighth unused)
    uint32_t w[2][8];
    for (int b = 0; b < 2; ++b)
        for (int h = 0; h < 2; ++h) {
            uint32_t c0 = (uint32_t)(2 * b + h), c1 = MET2_STREAM_PARAM, c2 = (uint32_t)id, c3 = (uint32_t)(id >> 32);
            met2::philox4x32_10(c0, c1, c2, c3, A.k0, A.k1);
            w[b][4 * h] = c0; w[b][4 * h + 1] = c1; w[b][4 * h + 2] = c2; w[b][4 * h + 3] = c3;
        }
    const double mwf = draw(w[0], 0, P.mwf_lo, P.mwf_hi), t2m = draw(w[0], 1, P.t2m_lo, P.t2m_hi), t2ie = draw(w[0], 2, P.t2ie_lo, P.t2ie_hi);
    const double fa = draw(w[0], 3, P.fa_lo, P.fa_hi), snr = A.noisy ? draw(w[1], 0, P.snr_lo, P.snr_hi) : INFINITY;
    const double sm = draw(w[1], 1, P.sm_lo, P.sm_hi), sie = draw(w[1], 2, P.sie_lo, P.sie_hi);
    const double iewf = 1.0 - mwf;                                 // f_csf = 0 (:175-176)
    const double step = 299.0 / 999.0;
    // pdf = MWF N(T2; T2m, sm) + IEWF N(T2; T2ie, sie) (scipy.stats.norm.pdf), normalised to sum 1 (:386-387)
    double part = 0.0;
    for (int j = lane; j < MET2_EVAL_NGRID; j += 64) {
        const double t = hires_t2(j, step);
        const double z1 = (t - t2m) / sm, z2 = (t - t2ie) / sie;
        const double p = mwf * (exp(-z1 * z1 / 2.0) / 2.5066282746310002 / sm) + iewf * (exp(-z2 * z2 / 2.0) / 2.5066282746310002 / sie);
        pdf[j] = p;
        part += p;
    }
    const double tot = met2::wave_sum(part);
    for (int j = lane; j < MET2_EVAL_NGRID; j += 64) pdf[j] /= tot;
    __syncthreads();

    // EPG at the voxel's own flip angle for every grid point; signal_e = Km (1 - exp(-TR/T1)) sum_j EPG_e(T2_j) dist_j (:40-56)
    const int nte = A.nte;
    const double a = fa * M_PI / 180.0, aexc = fa / 2.0 * M_PI / 180.0;
    const double ch = cos(a / 2), sh = sin(a / 2);
    const double c2 = ch * ch, s2 = sh * sh, sa = sin(a), ca = cos(a);
    const double F00 = sin(aexc), Fm0 = cos(aexc);
    const double E1 = exp(-(P.te / 2.0) / P.T1);
    const int up = lane > 0 ? lane - 1 : 0, dn = lane < 63 ? lane + 1 : 63;
    double acc = 0.0;
    for (int j = 0; j < MET2_EVAL_NGRID; ++j) {
        const double E2 = exp(-(P.te / 2.0) / hires_t2(j, step));
        double fp = 0.0, fm = lane == 0 ? Fm0 : 0.0, z = 0.0, F0 = F00;
        for (int e = 0; e < nte; ++e) {
            for (int half = 0; half < 2; ++half) {
                const double nF0 = met2::bcast(fm, 0);
                const double fpu = met2::gather(fp, up), fmd = met2::gather(fm, dn);
                fp = lane == 0 ? F0 : fpu;
                fm = lane < nte - 1 ? fmd : 0.0;
                F0 = nF0 * E2;
                fp *= E2; fm *= E2; z *= E1;
                if (half == 0) {
                    const double Ap = fp, Bm = fm, Zz = z;
                    fp = c2 * Ap + s2 * Bm + sa * Zz;
                    fm = s2 * Ap + c2 * Bm - sa * Zz;
                    z = -0.5 * sa * Ap + 0.5 * sa * Bm + ca * Zz;
                }
            }
            if (lane == e) acc += F0 * pdf[j];
        }
    }
    const double S = P.km * ((1.0 - exp(-P.TR / P.T1)) * acc);
    const double S0 = met2::bcast(S, 0);
    if (lane < nte) {
        double x = S;
        if (A.noisy) {                                             // Rician noise at sigma = S[0] / SNR (:390-393)
            uint32_t c0 = (uint32_t)lane, c1 = MET2_STREAM_NOISE, c2 = (uint32_t)id, c3 = (uint32_t)(id >> 32);
            met2::philox4x32_10(c0, c1, c2, c3, A.k0, A.k1);
            const double u1 = met2::u01_oc(c0, c1), u2 = met2::u01_co(c2, c3);
            const double r = sqrt(-2.0 * log(u1)), t = 6.283185307179586 * u2;
            const double sg = S0 / snr;
            const double re = S + sg * (r * cos(t)), im = sg * (r * sin(t));
            x = sqrt(re * re + im * im);
        }
        A.data[lv * nte + lane] = x;
    }

    // the pdf re-binned onto the plan's T2 grid by the midpoint rule (:404-426): bin i takes the grid points in [mid_{i-1}, mid_i),
    // the first everything below mid_0, the last everything from mid_{n-2} up; each weighted by dT2, then normalised
    const int nt2 = A.nt2;
    double bins[2] = {0.0, 0.0};
    for (int q = 0; q < 2; ++q) {
        const int i = lane + 64 * q;
        if (i >= nt2) continue;
        const double lo = i == 0 ? -INFINITY : A.t2s[i - 1] + (A.t2s[i] - A.t2s[i - 1]) / 2.0;
        const double hi = i == nt2 - 1 ? INFINITY : A.t2s[i] + (A.t2s[i + 1] - A.t2s[i]) / 2.0;
        double s = 0.0;
        for (int j = 0; j < MET2_EVAL_NGRID; ++j) {
            const double t = hires_t2(j, step);
            if (t >= lo && t < hi) s += pdf[j] * step;
        }
        bins[q] = s;
    }
    const double btot = met2::wave_sum(bins[0] + bins[1]);
    double fm_part = 0.0;
    for (int q = 0; q < 2; ++q) {
        const int i = lane + 64 * q;
        if (i >= nt2) continue;
        const double d = bins[q] / btot;
        A.dist2[lv * nt2 + i] = d;
        if (A.t2s[i] <= A.cut_m) fm_part += d;
    }
    const double mwf_true = met2::wave_sum(fm_part);
    if (lane < MET2_EVAL_NTRUTH) {
        const double tv[MET2_EVAL_NTRUTH] = {mwf_true, t2m, t2ie, P.km, fa, snr, mwf, sm, sie};
        double r = tv[0];
        for (int k = 1; k < MET2_EVAL_NTRUTH; ++k) r = lane == k ? tv[k] : r;
        A.truth[lane * A.n + lv] = r;
    }
}

__device__ void bitonic_sort(double *buf, int P, int lane)
{
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < P; i += 64) {
                const int l = i ^ j;
                if (l > i) {
                    const double x = buf[i], y = buf[l];
                    if ((i & k) == 0 ? nan_last_gt(x, y) : nan_last_gt(y, x)) { buf[i] = y; buf[l] = x; }
                }
            }
            __syncthreads();
        }
}

// scipy.special.rel_entr
__device__ __forceinline__ double rel_entr(double x, double y)
{
    if (x != x || y != y) return NAN;
    if (x > 0.0 && y > 0.0) return x * log(x / y);
    if (x == 0.0 && y >= 0.0) return 0.0;
    return INFINITY;
}

struct MetricArgs {
    int64_t n;
    int nt2, npow2;
    const double *t2s;
    double cut_m, cut_ie;
    const double *fsol, *dist2;     // [n][nt2]
    double *out;                    // [MET2_EVAL_NFIELD][n]
};

// one wave (one workgroup) per voxel: estimate_error_metrics (:59-74) from the fit's fsol (already multiplied by the first echo)
__global__ __launch_bounds__(64) void eval_voxel_metrics_kernel(MetricArgs A)
{
    __shared__ double xs[MET2_EVAL_MAX_T2], sa[MET2_EVAL_MAX_T2], sb[MET2_EVAL_MAX_T2];
    const int lane = threadIdx.x, n = A.nt2, P = A.npow2;
    const int64_t v = blockIdx.x;
    double f[2], d[2], t2[2];
    double s_f = 0.0, s_d = 0.0;
    for (int q = 0; q < 2; ++q) {
        const int i = lane + 64 * q;
        const bool in = i < n;
        f[q] = in ? A.fsol[v * n + i] : 0.0;
        d[q] = in ? A.dist2[v * n + i] : 0.0;
        t2[q] = in ? A.t2s[i] : 0.0;
        s_f += f[q]; s_d += d[q];
    }
    const double km = met2::wave_sum(s_f);
    double x[2], pm = 0.0, pie = 0.0, tm = 0.0, tie = 0.0, ae = 0.0, mx = -INFINITY, sx = 0.0;
    for (int q = 0; q < 2; ++q) {
        const int i = lane + 64 * q;
        x[q] = f[q] / km;
        if (i >= n) continue;
        xs[i] = x[q];
        if (t2[q] <= A.cut_m) { pm += x[q]; tm += x[q] * t2[q]; }
        if (t2[q] > A.cut_m && t2[q] <= A.cut_ie) { pie += x[q]; tie += x[q] * t2[q]; }
        ae += fabs(d[q] - x[q]);
        mx = (x[q] != x[q] || mx != mx) ? NAN : fmax(mx, x[q]);  // np.max propagates nan
        sx += x[q];
    }
    const double fM = met2::wave_sum(pm), fIE = met2::wave_sum(pie);
    const double T2m = met2::wave_sum(tm) / (fM + 1.0e-50), T2ie = met2::wave_sum(tie) / (fIE + 1.0e-50);
    const double mae = met2::wave_sum(ae) / (double)n;
    const double xmax = met2::wave_max(mx);
    const double xmax_nan = met2::wave_sum(mx != mx ? 1.0 : 0.0);
    const double hmin = 1e-5 * (xmax_nan > 0.0 ? NAN : xmax);
    const double sd = met2::wave_sum(s_d), sq = met2::wave_sum(sx);
    __syncthreads();
    // scipy.signal.find_peaks(x, height=hmin): a maximal run of equal values [a, b] with 1 <= a, b + 1 <= n - 1, x[a-1] < x[a] and x[b+1] <
    // x[a] (the run walk of _local_maxima_1d stops at n - 1), kept when x[a] >= hmin
    double pk = 0.0;
    for (int a = lane; a < n; a += 64) {
        if (a < 1 || a > n - 2 || !(xs[a - 1] < xs[a])) continue;
        int j = a + 1;
        while (j < n - 1 && xs[j] == xs[a]) ++j;
        if (xs[j] < xs[a] && hmin <= xs[a]) pk += 1.0;
    }
    const double npk = met2::wave_sum(pk);
    // scipy.spatial.distance.jensenshannon(dist2, x): both renormalised, m = (p + q) / 2, sqrt((sum rel_entr(p, m) + sum rel_entr(q, m)) / 2)
    double le = 0.0, ri = 0.0;
    for (int q = 0; q < 2; ++q) {
        if (lane + 64 * q >= n) continue;
        const double p = d[q] / sd, qq = x[q] / sq, m = (p + qq) / 2.0;
        le += rel_entr(p, m); ri += rel_entr(qq, m);
    }
    const double jsd = sqrt((met2::wave_sum(le) + met2::wave_sum(ri)) / 2.0);
    // scipy.stats.wasserstein_distance(dist2, x) with the bin values as samples: mean |sort(dist2) - sort(x)| for equal sizes
    for (int i = lane; i < P; i += 64) {
        sa[i] = i < n ? A.dist2[v * n + i] : NAN;
        sb[i] = i < n ? xs[i] : NAN;
    }
    __syncthreads();
    bitonic_sort(sa, P, lane);
    bitonic_sort(sb, P, lane);
    double wd = 0.0;
    for (int i = lane; i < n; i += 64) wd += fabs(sa[i] - sb[i]);
    const double wdist = met2::wave_sum(wd) / (double)n;
    if (lane < MET2_EVAL_NFIELD) {
        const double r[MET2_EVAL_NFIELD] = {fM, fIE, T2m, T2ie, km, npk, mae, jsd, wdist};
        double o = r[0];
        for (int k = 1; k < MET2_EVAL_NFIELD; ++k) o = lane == k ? r[k] : o;
        A.out[lane * A.n + v] = o;
    }
}

#define RED_THREADS 256
#define RED_S1 16
#define RED_S2 6

// sums over LDS in a fixed tree: the same inputs give the same bits
__device__ void block_reduce(double (*buf)[RED_THREADS], int nsum, int tid)
{
    for (int s = RED_THREADS / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s)
            for (int k = 0; k < nsum; ++k) buf[k][tid] += buf[k][tid + s];
    }
    __syncthreads();
}

struct ReduceArgs {
    int64_t n;
    const double *pv;               // [MET2_EVAL_NFIELD][n]
    const double *truth;            // [MET2_EVAL_NTRUTH][n]
    const double *lam;              // [n] or NULL
    const double *fie;              // [n] the fIE GMARE reads, or NULL = pv's
    double *out;                    // [MET2_EVAL_NAGG]
};

// one workgroup: compute_multi_metrics (:77-123) and mean / std (ddof 0) of lambda, in two passes (sums, then sums about the means)
__global__ __launch_bounds__(RED_THREADS) void eval_reduce_kernel(ReduceArgs A)
{
    __shared__ double buf[RED_S1][RED_THREADS];
    const int tid = threadIdx.x;
    const int64_t n = A.n;
    const double *M = A.pv, *FIE = A.fie ? A.fie : A.pv + n, *T2M = A.pv + 2 * n, *T2IE = A.pv + 3 * n, *KM = A.pv + 4 * n;
    const double *NPK = A.pv + 5 * n, *MAES = A.pv + 6 * n, *JSD = A.pv + 7 * n, *WD = A.pv + 8 * n;
    const double *T = A.truth, *VT2M = A.truth + n, *VT2IE = A.truth + 2 * n, *VKM = A.truth + 3 * n;
    double s[RED_S1];
    for (int k = 0; k < RED_S1; ++k) s[k] = 0.0;
    for (int64_t i = tid; i < n; i += RED_THREADS) {
        const double r = M[i] - T[i], rr = r / T[i];
        s[0] += r; s[1] += fabs(r); s[2] += fabs(rr); s[3] += r * r; s[4] += rr * rr; s[5] += M[i]; s[6] += T[i];
        s[7] += fabs(FIE[i] - (1.0 - T[i])) / (1.0 - T[i]);
        s[8] += fabs(T2M[i] - VT2M[i]) / VT2M[i];
        s[9] += fabs(T2IE[i] - VT2IE[i]) / VT2IE[i];
        s[10] += fabs(KM[i] - VKM[i]) / VKM[i];
        s[11] += fabs(NPK[i] - 2.0); s[12] += MAES[i]; s[13] += JSD[i]; s[14] += WD[i]; s[15] += A.lam ? A.lam[i] : 0.0;
    }
    for (int k = 0; k < RED_S1; ++k) buf[k][tid] = s[k];
    block_reduce(buf, RED_S1, tid);
    const double dn = (double)n;
    double m[RED_S1];
    for (int k = 0; k < RED_S1; ++k) m[k] = buf[k][0] / dn;
    __syncthreads();
    const double mr = m[0], mM = m[5], mT = m[6], ml = m[15];
    double c[RED_S2] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = tid; i < n; i += RED_THREADS) {
        const double xm = M[i] - mM, ym = T[i] - mT, dr = (M[i] - T[i]) - mr, dl = (A.lam ? A.lam[i] : 0.0) - ml;
        c[0] += (xm - ym) * (xm - ym); c[1] += dr * dr; c[2] += xm * ym; c[3] += xm * xm; c[4] += ym * ym; c[5] += dl * dl;
    }
    for (int k = 0; k < RED_S2; ++k) buf[k][tid] = c[k];
    block_reduce(buf, RED_S2, tid);
    if (tid == 0) {
        const double rmse = sqrt(m[3]), sdd = sqrt(buf[1][0] / dn);
        // fmin / fmax return the operand that is a number: a NaN quotient (a constant column, n = 1, a NaN voxel) stays NaN, as pearsonr's does
        const double q = buf[2][0] / (sqrt(buf[3][0]) * sqrt(buf[4][0]));
        const double R = q != q ? q : fmax(fmin(q, 1.0), -1.0);
        const double o[MET2_EVAL_NAGG] = {m[1], m[2], rmse, sqrt(buf[0][0] / dn), sqrt(m[4]), 1.96 * sqrt(sdd * sdd + rmse * rmse), m[0], R,
                                          m[2] + m[7] + m[8] + m[9] + m[10], m[11], m[12], m[13], m[14], ml, sqrt(buf[5][0] / dn)};
        for (int k = 0; k < MET2_EVAL_NAGG; ++k) A.out[k] = o[k];
    }
}

int plan_info(met2_plan *plan, int &nte, int &nt2, met2_options &o, const double *&t2s)
{
    int32_t a = 0, b = 0;
    int rc = met2_plan_get_shape(plan, &a, &b, nullptr);
    if (rc) return rc;
    rc = met2_plan_get_options(plan, &o);
    if (rc) return rc;
    t2s = plan->have_t2 ? plan->dT2 : nullptr;
    if (!t2s) return fail(MET2_E_STATE, "no T2 grid set");
    nte = a; nt2 = b;
    return MET2_OK;
}

}  // namespace

extern "C" int met2_synth_two_lobe(met2_plan *plan, const met2_synth_params *params, int64_t n, int64_t seed, int64_t voxel_offset, double *data,
                                   double *true_dist, double *truth, void *stream)
{
    if (!plan || !params) return fail(MET2_E_INVALID, "NULL argument");
    if (params->struct_size < (int32_t)sizeof(met2_synth_params)) return fail(MET2_E_INVALID, "met2_synth_params.struct_size too small");
    if (n < 0 || n > 0x7fffffff) return fail(MET2_E_INVALID, "n out of range");
    if (voxel_offset < 0) return fail(MET2_E_INVALID, "voxel_offset must be >= 0");
    const met2_synth_params &P = *params;
    const double lo[8] = {P.mwf_lo, P.t2m_lo, P.t2ie_lo, P.fa_lo, P.sm_lo, P.sie_lo, P.snr_lo, P.km};
    const double hi[8] = {P.mwf_hi, P.t2m_hi, P.t2ie_hi, P.fa_hi, P.sm_hi, P.sie_hi, std::isinf(P.snr_lo) ? INFINITY : P.snr_hi, P.km};
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || hi[k] < lo[k]) return fail(MET2_E_INVALID, "parameter range must be finite with lo <= hi");
    if (!std::isinf(P.snr_lo) && !(std::isfinite(P.snr_hi) && P.snr_lo > 0.0 && P.snr_hi >= P.snr_lo))
        return fail(MET2_E_INVALID, "SNR band must be 0 < lo <= hi, or lo = inf (no noise)");
    if (!(P.te > 0.0 && P.TR > 0.0 && P.T1 > 0.0 && std::isfinite(P.km))) return fail(MET2_E_INVALID, "te, TR, T1 must be positive, km finite");
    if (!(P.t2m_lo > 0.0 && P.t2ie_lo > 0.0 && P.sm_lo > 0.0 && P.sie_lo > 0.0)) return fail(MET2_E_INVALID, "T2 centres and widths must be positive");
    if (n == 0) return MET2_OK;
    if (!data || !true_dist || !truth) return fail(MET2_E_INVALID, "NULL argument");
    int nte, nt2;
    met2_options o;
    const double *t2s;
    int rc = plan_info(plan, nte, nt2, o, t2s);
    if (rc) return rc;
    if (nte > MET2_EVAL_MAX_TE || nt2 > MET2_EVAL_MAX_T2 || nt2 < 2) return fail(MET2_E_UNSUPPORTED, "synthesis needs n_te <= 64 and 2 <= n_t2 <= 128");
    USE_DEVICE(o.device);
    SynthArgs A;
    A.n = n; A.v0 = voxel_offset; A.nte = nte; A.nt2 = nt2;
    A.k0 = (uint32_t)(uint64_t)seed; A.k1 = (uint32_t)((uint64_t)seed >> 32);
    A.P = P; A.noisy = !std::isinf(P.snr_lo); A.t2s = t2s; A.cut_m = o.t2_myelin_cut;
    A.data = data; A.dist2 = true_dist; A.truth = truth;
    hipLaunchKernelGGL(synth_two_lobe_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_eval_voxel_metrics(met2_plan *plan, int64_t n, const double *fsol, const double *true_dist, double *out, void *stream)
{
    if (!plan) return fail(MET2_E_INVALID, "NULL plan");
    if (n < 0 || n > 0x7fffffff) return fail(MET2_E_INVALID, "n out of range");
    if (n == 0) return MET2_OK;
    if (!fsol || !true_dist || !out) return fail(MET2_E_INVALID, "NULL argument");
    int nte, nt2;
    met2_options o;
    const double *t2s;
    int rc = plan_info(plan, nte, nt2, o, t2s);
    if (rc) return rc;
    if (nt2 > MET2_EVAL_MAX_T2 || nt2 < 3) return fail(MET2_E_UNSUPPORTED, "metrics need 3 <= n_t2 <= 128");
    USE_DEVICE(o.device);
    MetricArgs A;
    A.n = n; A.nt2 = nt2;
    A.npow2 = 1;
    while (A.npow2 < nt2) A.npow2 <<= 1;
    A.t2s = t2s; A.cut_m = o.t2_myelin_cut; A.cut_ie = o.t2_ie_cut;
    A.fsol = fsol; A.dist2 = true_dist; A.out = out;
    hipLaunchKernelGGL(eval_voxel_metrics_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_eval_reduce(int64_t n, const double *per_voxel, const double *truth, const double *lam, const double *fie, double *out, void *stream)
{
    if (n <= 0) return fail(MET2_E_INVALID, "n must be positive");
    if (!per_voxel || !truth || !out) return fail(MET2_E_INVALID, "NULL argument");
    ReduceArgs A;
    A.n = n; A.pv = per_voxel; A.truth = truth; A.lam = lam; A.fie = fie; A.out = out;
    hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}
