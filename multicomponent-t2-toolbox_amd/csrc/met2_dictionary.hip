// met2_dictionary.hip -- what a plan derives from its dictionary and its penalty matrix: met2_plan_build_dictionary_epg[_profile],
// met2_plan_set_dictionary / _get_dictionary, met2_plan_set_t2_grid and met2_plan_set_penalty[_dense] / _get_penalty.
//
// Kernels
//   epg_dictionary_kernel   epg/epg.py:47-162      one wavefront per (T2, flip angle); the EPG
//                                                  coherence orders live on the lanes, the
//                                                  shift operator is a lane shuffle
//   epg_profile_dictionary_kernel                  the same trains summed over a slice profile: one workgroup per
//                                                  (T2, flip angle), its waves share the profile's points
//   gram_kernel            B_fa = D_fa^T D_fa, D_fa^T   (once per plan)
//   relayout_kernel        reference layout [te][t2][fa] <-> device layout [fa][te][t2]
//   gcv_basis_kernel       GCV's low-rank basis per flip angle (also the lower bounds of the brute-force FA walk)
// build_gram (plan.hpp) runs the two that follow every change of the dictionary; met2_roi_reduce (met2_roi_metrics.hip) calls it too.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_work.hpp"
#include "plan.hpp"
#include "wave_ops.hpp"

using namespace met2;

// ------------------------------------------------------------------------------------------
// EPG dictionary  (epg/epg.py:64-153).  Lane k holds order k: Fp = F_k (lane 0: F_0),
// Fm = F_-k, Z = Z_k.  One inter-echo period = P T P, P = shift then relax over tau/2.
// ------------------------------------------------------------------------------------------
// One echo train on one wave: the state after the excitation (the reference's: sin(aexc) in F_0, cos(aexc) in F_-1) and the
// constants of the refocusing pulse alpha (radians) and of the relaxation over tau/2.  Both dictionary kernels run this recursion.
struct EpgTrain { double E2, E1, c2, s2, sa, ca, Fp, Fm, Z; };

__device__ __forceinline__ EpgTrain epg_train_begin(int lane, double alpha, double aexc, double tau, double T2, double T1)
{
    EpgTrain t;
    const double th = tau / 2.0;
    const double R2 = 1.0 / T2, R1 = 1.0 / T1;
    t.E2 = exp(-th * R2); t.E1 = exp(-th * R1);
    const double ca2 = cos(alpha / 2.0), sa2 = sin(alpha / 2.0);
    t.c2 = ca2 * ca2; t.s2 = sa2 * sa2; t.sa = sin(alpha); t.ca = cos(alpha);
    t.Fp = (lane == 0) ? sin(aexc) : 0.0;
    t.Fm = (lane == 1) ? cos(aexc) : 0.0;
    t.Z = 0.0;
    return t;
}

// one inter-echo period of an n-echo train; afterwards lane 0's Fp is the echo amplitude
__device__ __forceinline__ void epg_train_period(EpgTrain &t, int lane, int n)
{
    for (int half = 0; half < 2; ++half) {
        double up = gather(t.Fp, (lane + 63) & 63);   // F_{k-1}
        double dn = gather(t.Fm, (lane + 1) & 63);    // F_-(k+1)
        dn = (lane < n) ? dn : 0.0;                   // F_-n <- 0
        t.Fp = (lane == 0) ? dn : up;                 // F_0 <- F_-1 ; F_k <- F_{k-1}
        t.Fm = (lane == 0) ? 0.0 : dn;
        t.Fp *= t.E2; t.Fm *= t.E2; t.Z *= t.E1;
        if (lane > n) { t.Fp = 0.0; t.Fm = 0.0; t.Z = 0.0; }
        if (half == 0 && lane >= 1) {
            // c2 a + s2 b + sa z,  s2 a + c2 b - sa z,  -sa/2 a + sa/2 b + ca z: the fused multiply-adds are written out, in the grouping the
            // dictionary kernel has always been compiled to, so that both kernels round alike and no compiler's choice of what to contract
            // changes a dictionary
            #pragma clang fp contract(off)
            const double a = t.Fp, b = t.Fm, z = t.Z, hs = 0.5 * t.sa;
            t.Fp = fma(t.sa, z, fma(t.c2, a, t.s2 * b));
            t.Fm = fma(-t.sa, z, fma(t.s2, a, t.c2 * b));
            t.Z = fma(t.ca, z, fma(hs, b, -(hs * a)));
        }
    }
}

__global__ __launch_bounds__(256) void epg_dictionary_kernel(int nte, int nt2, int nfa, const double *__restrict__ T2s,
                                                             const double *__restrict__ T1s, double tau,
                                                             const double *__restrict__ alpha_deg, double TR,
                                                             double *__restrict__ D /* [nfa][nte][nt2] */)
{
    const int lane = lane_id();
    const int gw = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (gw >= nfa * nt2) return;
    const int fa = gw / nt2, j = gw - fa * nt2;
    const double rad = M_PI / 180.0;
    const double alpha = alpha_deg[fa] * rad, aexc = alpha_deg[fa] / 2.0 * rad;
    EpgTrain t = epg_train_begin(lane, alpha, aexc, tau, T2s[j], T1s[j]);
    const double scale = 1.0 - exp(-TR / T1s[j]);
    for (int e = 0; e < nte; ++e) {
        epg_train_period(t, lane, nte);
        if (lane == 0) D[((size_t)fa * nte + e) * nt2 + j] = t.Fp * scale;
    }
}

// The dictionary of a slice profile (met2_plan_build_dictionary_epg_profile): D[fa][e][j] = scale_j * sum_z w[z] H_z[e], H_z the train above
// at the refocusing angle (a * r_ref[z]) and the excitation angle ((a / 2) * r_exc[z]).  One workgroup of four waves per (fa, t2) column:
// wave v runs the points z = v, v + 4, ...; lane e keeps echo e (in lane 0 after each period), so a finished point is one row of the LDS tile
// [n_z][64].  Then lanes e < nte of wave 0 sum their column over z in ascending order, product and sum rounded separately: the order is
// part of the entry's definition and no launch geometry enters it.
__global__ __launch_bounds__(256) void epg_profile_dictionary_kernel(int nte, int nt2, int nz, const double *__restrict__ T2s,
                                                                     const double *__restrict__ T1s, double tau,
                                                                     const double *__restrict__ alpha_deg, double TR,
                                                                     const double *__restrict__ r_exc, const double *__restrict__ r_ref,
                                                                     const double *__restrict__ w, double *__restrict__ D /* [nfa][nte][nt2] */)
{
    extern __shared__ double epg_tile[];                  // [nz][64]
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int fa = (int)blockIdx.x / nt2, j = (int)blockIdx.x - fa * nt2;
    const double rad = M_PI / 180.0;
    const double a = alpha_deg[fa], T2 = T2s[j], T1 = T1s[j];
    for (int z = wave; z < nz; z += 4) {
        const double alpha = (a * r_ref[z]) * rad, aexc = ((a / 2.0) * r_exc[z]) * rad;
        EpgTrain t = epg_train_begin(lane, alpha, aexc, tau, T2, T1);
        double keep = 0.0;
        for (int e = 0; e < nte; ++e) {
            epg_train_period(t, lane, nte);
            const double h = bcast(t.Fp, 0);
            keep = (lane == e) ? h : keep;
        }
        epg_tile[z * 64 + lane] = keep;
    }
    __syncthreads();
    if (wave == 0 && lane < nte) {
        #pragma clang fp contract(off)
        double acc = 0.0;
        for (int z = 0; z < nz; ++z) {
            const double term = w[z] * epg_tile[z * 64 + lane];
            acc = acc + term;
        }
        const double scale = 1.0 - exp(-TR / T1);
        D[((size_t)fa * nte + lane) * nt2 + j] = acc * scale;
    }
}

__global__ __launch_bounds__(256) void gram_kernel(int nte, int nt2, const double *__restrict__ D, double *__restrict__ B,
                                                   double *__restrict__ Dt)
{
    const double *Df = D + (size_t)blockIdx.x * nte * nt2;
    double *Bf = B + (size_t)blockIdx.x * nt2 * nt2;
    double *Dtf = Dt + (size_t)blockIdx.x * nte * nt2;          // [t2][te]: the model signal D x reads columns of D
    for (int idx = threadIdx.x; idx < nt2 * nte; idx += blockDim.x) {
        int a = idx / nte, e = idx - a * nte;
        Dtf[idx] = Df[e * nt2 + a];
    }
    for (int idx = threadIdx.x; idx < nt2 * nt2; idx += blockDim.x) {
        int a = idx / nt2, b = idx - a * nt2;
        double t = 0.0;
        for (int e = 0; e < nte; ++e) t = fma(Df[e * nt2 + a], Df[e * nt2 + b], t);
        Bf[idx] = t;
    }
}

// reference layout [te][t2][fa]  <->  device layout [fa][te][t2]
__global__ void relayout_kernel(int nte, int nt2, int nfa, const double *__restrict__ src, double *__restrict__ dst, int to_device)
{
    size_t total = (size_t)nte * nt2 * nfa;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t f = i / ((size_t)nte * nt2), r = i - f * nte * nt2;     // i indexes [fa][te][t2]
        size_t ref = r * nfa + f;
        if (to_device) dst[i] = src[ref]; else dst[ref] = src[i];
    }
}

// ------------------------------------------------------------------------------------------
// GCV's low-rank basis (objectives.hpp, "Round 4"): per flip angle an orthonormal Q (m x 16) of the dominant column space of D by
// pivoted Gram-Schmidt (the column of largest remaining norm, orthogonalised twice against the vectors found so far), then
// A = Q^T D from the ORIGINAL dictionary, stored transposed ([bin][16]: a support bin's 16 coefficients are one 128-byte line).
// res[fa] = largest remaining column norm / largest column norm: what the basis leaves of D.  One wave per flip angle; the
// remainder R (m x n) lives in LDS, lane <-> column for the sweeps over columns, lane <-> echo for the basis vectors.
// ------------------------------------------------------------------------------------------
#define MET2_GCV_LR_TOL 1e-9
__global__ __launch_bounds__(64) void gcv_basis_kernel(int m, int n, const double *__restrict__ D, double *__restrict__ Aq, double *__restrict__ Qt,
                                                       double *__restrict__ res)
{
    extern __shared__ double basis_lds[];
    double *R = basis_lds, *Q = basis_lds + (size_t)m * n;             // R[m][n], Q[16][64]
    const int fa = blockIdx.x, lane = threadIdx.x;
    const double *Df = D + (size_t)fa * m * n;
    for (int i = lane; i < m * n; i += 64) R[i] = Df[i];
    for (int i = lane; i < MET2_GCV_LR_RANK * 64; i += 64) Q[i] = 0.0;
    __syncthreads();
    auto colnorm2 = [&](int j) { double sum = 0.0; for (int e = 0; e < m; ++e) { const double v = R[e * n + j]; sum = fma(v, v, sum); } return sum; };
    double nrm0 = 0.0;
    for (int s = 0; s < MET2_GCV_LR_RANK; ++s) {
        const double c0 = lane < n ? colnorm2(lane) : -1.0, c1 = lane + 64 < n ? colnorm2(lane + 64) : -1.0;
        const double mx = wave_max(fmax(c0, c1));
        if (s == 0) nrm0 = mx;
        if (!(mx > nrm0 * 1e-30)) break;                                // nothing left above rounding: the dictionary has rank s
        const u64 b0 = ballot(c0 == mx), b1 = ballot(c1 == mx);
        const int piv = b0 ? first_lane(b0) : 64 + first_lane(b1);
        double q = lane < m ? R[lane * n + piv] : 0.0;
        for (int pass = 0; pass < 2; ++pass)
            for (int t = 0; t < s; ++t) { const double qt = Q[t * 64 + lane]; const double d = wave_sum(q * qt); q = fma(-d, qt, q); }
        q = q / sqrt(wave_sum(q * q));
        Q[s * 64 + lane] = q;
        __syncthreads();
        for (int j = lane; j < n; j += 64) {                            // R -= q (q^T R)
            double a = 0.0;
            for (int e = 0; e < m; ++e) a = fma(Q[s * 64 + e], R[e * n + j], a);
            for (int e = 0; e < m; ++e) R[e * n + j] = fma(-a, Q[s * 64 + e], R[e * n + j]);
        }
        __syncthreads();
    }
    {
        const double c0 = lane < n ? colnorm2(lane) : -1.0, c1 = lane + 64 < n ? colnorm2(lane + 64) : -1.0;
        const double mx = wave_max(fmax(c0, c1));
        if (lane == 0) res[fa] = nrm0 > 0.0 ? sqrt(fmax(mx, 0.0) / nrm0) : 0.0;
    }
    for (int j = lane; j < n; j += 64)
        for (int s = 0; s < MET2_GCV_LR_RANK; ++s) {
            double a = 0.0;
            for (int e = 0; e < m; ++e) a = fma(Q[s * 64 + e], Df[e * n + j], a);
            Aq[((size_t)fa * n + j) * MET2_GCV_LR_RANK + s] = a;
        }
    // the basis itself, one vector per row ([fa][16][m]): the FA walk's lower bounds project the voxel's signal on it (fa_kernel)
    for (int s = 0; s < MET2_GCV_LR_RANK; ++s)
        if (lane < m) Qt[((size_t)fa * MET2_GCV_LR_RANK + s) * m + lane] = Q[s * 64 + lane];
}

// determinant by LU with partial pivoting (scipy.linalg.det at bayesian_interpolation.py:100)
static double det_lu(int n, const double *Ain)
{
    std::vector<double> A(Ain, Ain + (size_t)n * n);
    double det = 1.0;
    for (int c = 0; c < n; ++c) {
        int piv = c; double mx = fabs(A[(size_t)c * n + c]);
        for (int r = c + 1; r < n; ++r) if (fabs(A[(size_t)r * n + c]) > mx) { mx = fabs(A[(size_t)r * n + c]); piv = r; }
        if (mx == 0.0) return 0.0;
        if (piv != c) { for (int j = 0; j < n; ++j) std::swap(A[(size_t)c * n + j], A[(size_t)piv * n + j]); det = -det; }
        double d = A[(size_t)c * n + c];
        det *= d;
        for (int r = c + 1; r < n; ++r) {
            double l = A[(size_t)r * n + c] / d;
            if (l != 0.0) for (int j = c + 1; j < n; ++j) A[(size_t)r * n + j] -= l * A[(size_t)c * n + j];
        }
    }
    return det;
}

// Everything that is derived from the dictionary alone: Gram matrices, the transposed copy, GCV's low-rank basis.  Blocks (its callers do).
int met2::build_gram(met2_plan *p, hipStream_t s)
{
    hipLaunchKernelGGL(gram_kernel, dim3(p->n_fa), dim3(256), 0, s, p->n_te, p->n_t2, p->dD, p->dB, p->dDt);
    HIPCHK(hipGetLastError());
    const int lds = (int)sizeof(double) * (p->n_te * p->n_t2 + MET2_GCV_LR_RANK * 64);
    HIPCHK(hipFuncSetAttribute((const void *)gcv_basis_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(gcv_basis_kernel, dim3(p->n_fa), dim3(64), lds, s, p->n_te, p->n_t2, p->dD, p->dAq, p->dQt, p->dAqRes);
    HIPCHK(hipGetLastError());
    std::vector<double> res(p->n_fa);
    HIPCHK(hipMemcpyAsync(res.data(), p->dAqRes, sizeof(double) * p->n_fa, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    bool ok = true;
    p->gcv_res = 0.0;
    for (double r : res) { ok = ok && (r <= MET2_GCV_LR_TOL); p->gcv_res = (r > p->gcv_res || r != r) ? r : p->gcv_res; }      // (nan: not low rank)
    p->gcv_lr = ok;
    p->have_dict = true; p->seeds_valid = false;
    return MET2_OK;
}

extern "C" {

int met2_plan_set_t2_grid(met2_plan *p, const double *T2s)
{
    if (!p || !T2s) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(p->opt.device);
    HIPCHK(hipMemcpy(p->dT2, T2s, sizeof(double) * p->n_t2, hipMemcpyHostToDevice));
    p->have_t2 = true;
    return MET2_OK;
}

int met2_plan_build_dictionary_epg(met2_plan *p, const double *T2s, const double *T1s, double tau, const double *alpha_deg,
                                   double TR, void *stream)
{
    if (!p || !T2s || !T1s || !alpha_deg) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(p->opt.device);
    hipStream_t s = (hipStream_t)stream;
    size_t nb = sizeof(double) * (size_t)(2 * p->n_t2 + p->n_fa);
    DeviceWork W(s);
    const auto tmp = W.take<double>(nb / sizeof(double));
    if (!W.alloc()) return W.finish("met2_plan_build_dictionary_epg");
    std::vector<double> h(2 * p->n_t2 + p->n_fa);
    memcpy(h.data(), T2s, sizeof(double) * p->n_t2);
    memcpy(h.data() + p->n_t2, T1s, sizeof(double) * p->n_t2);
    memcpy(h.data() + 2 * p->n_t2, alpha_deg, sizeof(double) * p->n_fa);
    int waves = p->n_fa * p->n_t2;
    int blocks = (waves + 3) / 4;
    int rc = MET2_OK;
    if (W.ok(hipMemcpy(tmp, h.data(), nb, hipMemcpyHostToDevice))) {
        hipLaunchKernelGGL(epg_dictionary_kernel, dim3(blocks), dim3(256), 0, s, p->n_te, p->n_t2, p->n_fa, tmp, tmp + p->n_t2, tau,
                           tmp + 2 * p->n_t2, TR, p->dD);
        if (W.ok(hipGetLastError())) rc = build_gram(p, s);
    }
    if (int e = W.finish("met2_plan_build_dictionary_epg")) return e;
    if (rc) return rc;
    rc = ensure_seeds(p, s);
    if (rc) return rc;
    return met2_plan_set_t2_grid(p, T2s);
}

int met2_plan_build_dictionary_epg_profile(met2_plan *p, const double *T2s, const double *T1s, double tau, const double *alpha_deg,
                                           double TR, int32_t n_z, const double *r_exc, const double *r_ref, const double *w, void *stream)
{
    if (!p || !T2s || !T1s || !alpha_deg || !r_exc || !r_ref || !w) return fail(MET2_E_INVALID, "NULL argument");
    if (n_z < 1 || n_z > 64) return fail(MET2_E_INVALID, "slice profile: n_z must lie in 1..64");
    double wsum = 0.0;
    for (int z = 0; z < n_z; ++z) {
        if (!std::isfinite(r_exc[z]) || !std::isfinite(r_ref[z]) || !std::isfinite(w[z]) || r_exc[z] < 0.0 || r_ref[z] < 0.0 || w[z] < 0.0)
            return fail(MET2_E_INVALID, "slice profile: r_exc, r_ref and w must be finite and >= 0");
        wsum += w[z];
    }
    if (!(wsum > 0.0)) return fail(MET2_E_INVALID, "slice profile: the weights are all zero");
    USE_DEVICE(p->opt.device);
    hipStream_t s = (hipStream_t)stream;
    const size_t n0 = (size_t)(2 * p->n_t2 + p->n_fa);
    std::vector<double> h(n0 + 3 * (size_t)n_z);
    memcpy(h.data(), T2s, sizeof(double) * p->n_t2);
    memcpy(h.data() + p->n_t2, T1s, sizeof(double) * p->n_t2);
    memcpy(h.data() + 2 * p->n_t2, alpha_deg, sizeof(double) * p->n_fa);
    memcpy(h.data() + n0, r_exc, sizeof(double) * n_z);
    memcpy(h.data() + n0 + n_z, r_ref, sizeof(double) * n_z);
    memcpy(h.data() + n0 + 2 * n_z, w, sizeof(double) * n_z);
    DeviceWork W(s);
    const auto tmp = W.take<double>(h.size());
    if (!W.alloc()) return W.finish("met2_plan_build_dictionary_epg_profile");
    int rc = MET2_OK;
    if (W.ok(hipMemcpy(tmp, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice))) {
        hipLaunchKernelGGL(epg_profile_dictionary_kernel, dim3(p->n_fa * p->n_t2), dim3(256), sizeof(double) * 64 * (size_t)n_z, s, p->n_te, p->n_t2,
                           n_z, tmp, tmp + p->n_t2, tau, tmp + 2 * p->n_t2, TR, tmp + n0, tmp + n0 + n_z, tmp + n0 + 2 * n_z, p->dD);
        if (W.ok(hipGetLastError())) rc = build_gram(p, s);
    }
    if (int e = W.finish("met2_plan_build_dictionary_epg_profile")) return e;
    if (rc) return rc;
    rc = ensure_seeds(p, s);
    if (rc) return rc;
    return met2_plan_set_t2_grid(p, T2s);
}

int met2_plan_set_dictionary(met2_plan *p, const double *dic)
{
    if (!p || !dic) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(p->opt.device);
    size_t nb = sizeof(double) * (size_t)p->n_fa * p->n_te * p->n_t2;
    DeviceWork W(0);
    const auto tmp = W.take<double>(nb / sizeof(double));
    if (!W.alloc()) return W.finish("met2_plan_set_dictionary");
    int rc = MET2_OK;
    if (W.ok(hipMemcpy(tmp, dic, nb, hipMemcpyHostToDevice))) {
        hipLaunchKernelGGL(relayout_kernel, dim3(256), dim3(256), 0, 0, p->n_te, p->n_t2, p->n_fa, tmp, p->dD, 1);
        if (W.ok(hipGetLastError())) rc = build_gram(p, 0);
        W.ok(hipDeviceSynchronize());
    }
    if (int e = W.finish("met2_plan_set_dictionary")) return e;
    if (rc) return rc;
    return ensure_seeds(p, 0);
}

int met2_plan_get_dictionary(met2_plan *p, double *dic)
{
    if (!p || !dic) return fail(MET2_E_INVALID, "NULL argument");
    if (!p->have_dict) return fail(MET2_E_STATE, "no dictionary in the plan");
    USE_DEVICE(p->opt.device);
    size_t nb = sizeof(double) * (size_t)p->n_fa * p->n_te * p->n_t2;
    DeviceWork W(0);
    const auto tmp = W.take<double>(nb / sizeof(double));
    if (!W.alloc()) return W.finish("met2_plan_get_dictionary");
    hipLaunchKernelGGL(relayout_kernel, dim3(256), dim3(256), 0, 0, p->n_te, p->n_t2, p->n_fa, p->dD, tmp, 0);
    if (W.ok(hipGetLastError())) W.ok(hipMemcpy(dic, tmp, nb, hipMemcpyDeviceToHost));
    return W.finish("met2_plan_get_dictionary");
}

int met2_plan_set_penalty_dense(met2_plan *p, const double *L)
{
    if (!p || !L) return fail(MET2_E_INVALID, "NULL argument");
    const int n = p->n_t2;
    for (int i = 0; i < n * n; ++i) if (!std::isfinite(L[i])) return fail(MET2_E_INVALID, "non-finite penalty matrix");
    std::vector<double> K((size_t)n * n, 0.0);
    for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) {
        double t = 0.0;
        for (int i = 0; i < n; ++i) t += L[(size_t)i * n + a] * L[(size_t)i * n + b];
        K[(size_t)a * n + b] = t;
    }
    for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) if (abs(a - b) > 2) {
        if (K[(size_t)a * n + b] != 0.0) return fail(MET2_E_UNSUPPORTED, "L^T L has bandwidth > 2");
        if (L[(size_t)a * n + b] != 0.0) return fail(MET2_E_UNSUPPORTED, "penalty matrix has bandwidth > 2");
    }
    std::vector<double> kb(5 * 128, 0.0), lb(5 * 128, 0.0);
    for (int j = 0; j < n; ++j) for (int d = 0; d < 5; ++d) {
        int c = j + d - 2;
        if (c < 0 || c >= n) continue;
        kb[d * 128 + j] = K[(size_t)j * n + c];
        lb[d * 128 + j] = L[(size_t)j * n + c];
    }
    USE_DEVICE(p->opt.device);
    HIPCHK(hipMemcpy(p->dKband, kb.data(), sizeof(double) * 5 * 128, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->dLband, lb.data(), sizeof(double) * 5 * 128, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->dKd, K.data(), sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice));
    p->Lhost.assign(L, L + (size_t)n * n);
    p->log_detL = log(det_lu(n, L));
    p->have_pen = true; p->seeds_valid = false;
    return ensure_seeds(p, 0);
}

int met2_plan_set_penalty(met2_plan *p, int32_t which, const double *T2s)
{
    if (!p) return fail(MET2_E_INVALID, "NULL plan");
    const int n = p->n_t2;
    std::vector<double> L((size_t)n * n, 0.0);
    switch (which) {   // motor:86-111, 263-269
    case MET2_PEN_I: for (int i = 0; i < n; ++i) L[(size_t)i * n + i] = 1.0; break;
    case MET2_PEN_L1: for (int i = 0; i < n; ++i) { L[(size_t)i * n + i] = 1.0; if (i > 0) L[(size_t)i * n + i - 1] = -1.0; } break;
    case MET2_PEN_L2:
        for (int i = 0; i < n; ++i) {
            L[(size_t)i * n + i] = 2.0;
            if (i > 0) L[(size_t)i * n + i - 1] = -1.0;
            if (i < n - 1) L[(size_t)i * n + i + 1] = -1.0;
        }
        L[0] = 1.0; L[(size_t)(n - 1) * n + n - 1] = 1.0;
        break;
    case MET2_PEN_INVT2:
        if (!T2s) return fail(MET2_E_INVALID, "InvT2 needs the T2 grid");
        for (int i = 0; i < n; ++i) {
            double prev = (i == 0) ? T2s[0] - 1.0 : T2s[i - 1];
            double d = T2s[i] - prev;
            if (i == 0) d = T2s[1] - T2s[0];
            L[(size_t)i * n + i] = 1.0 / d;
        }
        break;
    default: return fail(MET2_E_INVALID, "unknown penalty");
    }
    return met2_plan_set_penalty_dense(p, L.data());
}

int met2_plan_get_penalty(met2_plan *p, double *L)
{
    if (!p || !L) return fail(MET2_E_INVALID, "NULL argument");
    if (!p->have_pen) return fail(MET2_E_STATE, "no penalty set");
    memcpy(L, p->Lhost.data(), sizeof(double) * p->Lhost.size());
    return MET2_OK;
}

} // extern "C"
