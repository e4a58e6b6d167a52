// met2_rician.hip -- Rician noise-floor correction of the echo magnitudes: met2_rician_bias / _step / _invert and met2_fit_rician.
//
// An extension with no counterpart in the reference, whose fits treat the floor sigma sqrt(pi / 2) of the late echoes as signal (its own
// synthetic study draws Rician noise: evaluate_all_methods_two_lobes_SNR50_150.py:387-391).  The cure is the standard one: the mean of a
// Rician magnitude with amplitude A is m(A, sigma) = A + b(A, sigma), the fit's model signal s_hat estimates A, so the raw echoes minus
// b(s_hat, sigma) are refitted, a few times over.  The math is rician_math.hpp's, one text for every kernel here.  Three kernels:
//   rician_bias_kernel     b(A, sigma) elementwise (the test entry)
//   rician_step_kernel     out = data - b(model, sigma_v), 64 / G voxels per wave (G lanes each): the fit's gate (classify_kernel, met2_hip.hip: a
//                          positive echo sum and a positive first echo) is checked on the corrected row -- partial sums per lane, then a
//                          butterfly over the group, a fixed order -- and a voxel that would fall out of it keeps its raw echoes (flag 1)
//   rician_invert_kernel   out = m^-1(data, sigma_v) per sample (the one-shot correction of a denoised magnitude)
// met2_fit_rician drives fits and steps chunk after chunk on the caller's stream, on scratch kept with the plan (met2_bootstrap.hip owns it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "plan.hpp"
#include "rician_math.hpp"
#include "wave_ops.hpp"

namespace {

#define MET2_RICIAN_MAX_ITER 16

__global__ __launch_bounds__(256) void rician_bias_kernel(int64_t n, const double *__restrict__ A, const double *__restrict__ sigma, double *__restrict__ b)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) b[i] = met2::rician_bias(A[i], sigma[i]);
}

struct StepArgs {
    int64_t nvox, vs, es;
    int nte, group;                 // group: lanes per voxel, a power of two in [1, 64] (step_launch sets it)
    const double *data;             // echo e of voxel v at data[v vs + e es]
    const double *model;            // [nvox][nte]
    const double *sigma;            // [nvox]
    const uint8_t *mask;            // [nvox] or NULL
    const int32_t *pstatus;         // [nvox] or NULL: a voxel whose status lacks MET2_ST_FITTED is copied (met2_fit_rician)
    double *out;                    // [nvox][nte]
    int32_t *flag;                  // [nvox] or NULL
};

// A voxel is taken by a group of G lanes of one wave, G = the power of two from min(n_te, 64) up (StepArgs::group): 64 / G voxels per wave, so
// that at 32 echoes no lane idles and a wave reads 64 consecutive doubles of [nvox][n_te] rows.  Lane l of the group takes echoes l, l + G,
// ... in order, then the group's partial sums meet in a butterfly over lane distances G / 2 .. 1: the same association in every lane and for
// every launch.  The voxel loop is wave-uniform; lanes past the last voxel carry zeros through the exchanges and touch no memory.
__global__ __launch_bounds__(256) void rician_step_kernel(StepArgs S)
{
    const int lane = met2::lane_id(), G = S.group, per = 64 / G, l = lane & (G - 1);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t vb = wave * per; vb < S.nvox; vb += nwaves * per) {
        const int64_t v = vb + lane / G;
        const bool in = v < S.nvox;
        const double sg = in ? S.sigma[v] : 0.0;
        const bool live = in && (S.mask ? S.mask[v] != 0 : true) && sg > 0.0 && (S.pstatus ? (S.pstatus[v] & MET2_ST_FITTED) != 0 : true);
        const double *d = S.data + v * S.vs, *mo = S.model + v * S.nte;
        double *o = S.out + v * S.nte;
        double sum = 0.0, first = 0.0;
        if (in)
            for (int e = l; e < S.nte; e += G) {
                const double x = d[e * S.es];
                const double y = live ? x - met2::rician_bias(mo[e], sg) : x;
                o[e] = y;
                sum += y;
                if (e == 0) first = y;
            }
        for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        first = __shfl(first, lane & ~(G - 1));
        const bool back = live && !(first > 0.0 && sum > 0.0);      // NaN fails the gate as well: the fit reports the voxel's raw echoes then
        if (back)
            for (int e = l; e < S.nte; e += G) o[e] = d[e * S.es];
        if (in && l == 0 && S.flag) S.flag[v] = back ? 1 : 0;
    }
}

struct InvArgs {
    int64_t nvox, vs, es;
    int nte;
    const double *data;
    const double *sigma;
    const uint8_t *mask;
    double *out;
};

// one thread per sample, consecutive threads along the echoes of a row of `out`
__global__ __launch_bounds__(256) void rician_invert_kernel(InvArgs I)
{
    const int64_t total = I.nvox * I.nte;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = i / I.nte;
        const int e = (int)(i - v * I.nte);
        const double x = I.data[v * I.vs + e * I.es], sg = I.sigma[v];
        const bool live = (I.mask ? I.mask[v] != 0 : true) && sg > 0.0;
        I.out[i] = live ? met2::rician_inverse(x, sg) : x;
    }
}

int grid_1d(int64_t total) { return (int)std::min<int64_t>((total + 255) / 256, 65536); }

int step_launch(StepArgs S, hipStream_t s)
{
    S.group = 1;
    while (S.group < 64 && S.group < S.nte) S.group <<= 1;
    hipLaunchKernelGGL(rician_step_kernel, dim3(grid_1d(S.nvox * S.group)), dim3(256), 0, s, S);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

int layout_checks(int64_t nvox, int32_t n_te, int64_t voxel_stride, int64_t echo_stride)
{
    if (nvox < 0 || nvox > 0x7fffffff) return fail(MET2_E_INVALID, "nvox out of range");
    if (n_te < 1 || n_te > 65536) return fail(MET2_E_INVALID, "n_te must lie in [1, 65536]");
    if (voxel_stride <= 0 || echo_stride <= 0) return fail(MET2_E_INVALID, "strides must be positive");
    return MET2_OK;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" int met2_rician_bias(int32_t device, int64_t n, const double *A, const double *sigma, double *b, void *stream)
{
    if (n < 0) return fail(MET2_E_INVALID, "n out of range");
    if (n == 0) return MET2_OK;
    if (!A || !sigma || !b) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    hipLaunchKernelGGL(rician_bias_kernel, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, n, A, sigma, b);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_rician_step(int32_t device, int64_t nvox, int32_t n_te, const double *data, int64_t voxel_stride, int64_t echo_stride,
                                const double *model, const double *sigma, const uint8_t *mask, double *out, int32_t *flag, void *stream)
{
    int rc = layout_checks(nvox, n_te, voxel_stride, echo_stride);
    if (rc) return rc;
    if (nvox == 0) return MET2_OK;
    if (!data || !model || !sigma || !out) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    StepArgs S;
    S.nvox = nvox; S.vs = voxel_stride; S.es = echo_stride; S.nte = n_te; S.data = data; S.model = model; S.sigma = sigma; S.mask = mask;
    S.pstatus = nullptr; S.out = out; S.flag = flag;
    return step_launch(S, (hipStream_t)stream);
}

extern "C" int met2_rician_invert(int32_t device, int64_t nvox, int32_t n_te, const double *data, int64_t voxel_stride, int64_t echo_stride,
                                  const double *sigma, const uint8_t *mask, double *out, void *stream)
{
    int rc = layout_checks(nvox, n_te, voxel_stride, echo_stride);
    if (rc) return rc;
    if (nvox == 0) return MET2_OK;
    if (!data || !sigma || !out) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    InvArgs I;
    I.nvox = nvox; I.vs = voxel_stride; I.es = echo_stride; I.nte = n_te; I.data = data; I.sigma = sigma; I.mask = mask; I.out = out;
    hipLaunchKernelGGL(rician_invert_kernel, dim3(grid_1d(nvox * n_te)), dim3(256), 0, (hipStream_t)stream, I);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_fit_rician(met2_plan *plan, int32_t method, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                               const double *fa_index, const uint8_t *mask, const double *sigma, int32_t n_iter, double *fsol, double *sig,
                               double *reg, double *lam, double *maps, int32_t *status, double *sigma_out, int32_t *flag, void *stream)
{
    // argument checks first: nothing here touches a device
    if (n_iter < 0 || n_iter > MET2_RICIAN_MAX_ITER) return fail(MET2_E_INVALID, "n_iter must lie in [0, 16]");
    if (nvox < 0 || nvox > 0x7fffffff) return fail(MET2_E_INVALID, "nvox out of range");
    if (voxel_stride <= 0 || echo_stride <= 0) return fail(MET2_E_INVALID, "strides must be positive");
    if (!plan) return fail(MET2_E_INVALID, "NULL plan");
    if (method < MET2_NNLS || method > MET2_BAYESREG) return fail(MET2_E_INVALID, "unknown method");
    if (nvox == 0) return MET2_OK;
    if (!data || !fsol || !reg) return fail(MET2_E_INVALID, "NULL argument");
    int32_t nte = 0, nt2 = 0;
    int rc = met2_plan_get_shape(plan, &nte, &nt2, nullptr);
    if (rc) return rc;
    met2_options opt;
    rc = met2_plan_get_options(plan, &opt);
    if (rc) return rc;
    const int dev = opt.device;
    USE_DEVICE(dev);
    hipStream_t s = (hipStream_t)stream;
    // voxels per pass of the loop: met2_fit_bootstrap's row limits (L-curve at two bins per lane: the spill-over kernel's record cap covers every row)
    const int64_t vmax = (method == MET2_LCURVE && nt2 > 64) ? 4096 : 262144;
    const int64_t cap = n_iter > 0 ? std::min<int64_t>(nvox, vmax) : 0;
    // scratch: what the caller passed as NULL, the plain-NNLS pass of the sigma estimate, the status of pass 0, one chunk of corrected rows and maps
    size_t off = 0;
    auto take = [&off](bool wanted, size_t bytes) { const size_t o = off; if (wanted) off += align256(bytes); return wanted ? o : (size_t)-1; };
    const size_t nv = (size_t)nvox;
    const size_t o_sig = take(!sig, sizeof(double) * nv * nte), o_sigma = take(!sigma && !sigma_out, sizeof(double) * nv);
    const size_t o_f0 = take(!sigma, sizeof(double) * nv * nt2), o_s0 = take(!sigma, sizeof(double) * nv * nte), o_r0 = take(!sigma, sizeof(double) * nv);
    const size_t o_st0 = take(true, sizeof(int32_t) * nv);
    const size_t o_y = take(cap > 0, sizeof(double) * (size_t)cap * nte), o_maps = take(cap > 0 && maps, sizeof(double) * 6 * (size_t)cap);
    char *w = nullptr;
    rc = met2::rician_scratch(plan, dev, off, &w);
    if (rc) return rc;
    rc = met2::plan_reserve(plan, nvox);                       // the sort scratch is sized once, before anything is enqueued
    if (rc) return rc;
    auto at = [w](size_t o) { return o == (size_t)-1 ? nullptr : w + o; };
    double *psig = sig ? sig : (double *)at(o_sig);
    int32_t *st0 = (int32_t *)at(o_st0);
    double *y = (double *)at(o_y), *maps_c = (double *)at(o_maps);

    // pass 0: exactly met2_fit_strided's fit
    int32_t *pst = status ? status : st0;
    rc = met2_fit_enqueue_strided(plan, method, nvox, data, voxel_stride, echo_stride, fa_index, mask, fsol, psig, reg, lam, maps, pst, stream);
    if (rc) return rc;
    if (status && n_iter > 0) HIPCHK(hipMemcpyAsync(st0, status, sizeof(int32_t) * nv, hipMemcpyDeviceToDevice, s));
    // sigma: given, or met2_noise_sigma's estimate on the raw echoes
    const double *sg = sigma;
    if (sigma) {
        if (sigma_out && sigma_out != sigma) HIPCHK(hipMemcpyAsync(sigma_out, sigma, sizeof(double) * nv, hipMemcpyDeviceToDevice, s));
    } else {
        double *so = sigma_out ? sigma_out : (double *)at(o_sigma);
        rc = met2::noise_sigma_enqueue(plan, nte, nt2, nvox, data, voxel_stride, echo_stride, fa_index, mask, (double *)at(o_f0), (double *)at(o_s0),
                                       (double *)at(o_r0), so, stream);
        if (rc) return rc;
        sg = so;
    }
    if (flag) HIPCHK(hipMemsetAsync(flag, 0, sizeof(int32_t) * nv, s));
    // one wait: an FA index outside the dictionary is reported before any correction pass
    rc = met2_plan_finish(plan, stream);
    if (rc || n_iter == 0) return rc;

    // passes 1 .. n_iter, chunk after chunk: the raw echoes minus the bias at the previous pass's model signal, then the fit of that
    StepArgs S;
    S.vs = voxel_stride; S.es = echo_stride; S.nte = nte; S.out = y;
    for (int64_t v0 = 0; v0 < nvox; v0 += cap) {
        const int64_t n = std::min(cap, nvox - v0);
        S.nvox = n; S.data = data + v0 * voxel_stride; S.model = psig + v0 * nte; S.sigma = sg + v0; S.mask = mask ? mask + v0 : nullptr;
        S.pstatus = st0 + v0; S.flag = flag ? flag + v0 : nullptr;
        for (int k = 1; k <= n_iter; ++k) {
            const bool last = k == n_iter;
            rc = step_launch(S, s);
            if (rc) return rc;
            rc = met2_fit_enqueue_strided(plan, method, n, y, nte, 1, fa_index ? fa_index + v0 : nullptr, S.mask, fsol + v0 * nt2, psig + v0 * nte, reg + v0,
                                          lam && last ? lam + v0 : nullptr, maps && last ? maps_c : nullptr, status ? status + v0 : nullptr, stream);
            if (rc) return rc;
        }
        if (maps)                                              // the chunk's [6][n] maps into the caller's [6][nvox]
            for (int q = 0; q < 6; ++q) HIPCHK(hipMemcpyAsync(maps + q * nvox + v0, maps_c + q * n, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
    }
    return met2_plan_finish(plan, stream);
}
