// met2_bias.hip -- met2_bias_field: bias-field correction of a 3-D map (bias_correct='yes'; step 5 of the reference's example pipeline, which
// runs FSL's fast on the total water content map on the CPU).  The EM estimator of Wells et al. (IEEE TMI 1996) and Guillemaud & Brady
// (1997), the one FAST iterates, without FAST's Markov random field term; include/met2_hip.h states the algorithm; no program text of FSL was
// used.  The host reads nothing back: every launch of the call is enqueued up front, and the domain's size, the histogram, the class
// parameters and the mean of b stay in a small device record (BiasStats) that the kernels read.
//   bias_log_kernel       y = log v on the domain, the domain flags, the number of domain voxels per chunk of 1024 voxels
//   bias_scan_kernel      exclusive scan of those counts (one workgroup) -> N
//   bias_compact_kernel   the domain's voxel indices in memory order: idx[0..N)
// Every fp64 sum over the domain runs over that compacted list, BIAS_CHUNK entries per workgroup in a fixed order (a thread's four entries,
// a butterfly over the wave, the four waves), one partial per chunk; a one-workgroup second stage adds the partials in a fixed order.  So a
// sum depends on the domain's values in memory order alone: not on the grid, and not on where the domain lies in the volume.
//   bias_stat1_kernel / bias_stat1_final    lo, hi, mean of y
//   bias_stat2_kernel / bias_init_kernel    256-bin histogram (integer atomics, LDS then global), variance -> the initial classes
//   bias_estep_kernel<false> / bias_mstep_kernel   posteriors and the 3 K sums of the M-step (s, sum p u, sum p (u - mu)^2 about the OLD mean;
//                         the second stage moves it to the new one: sum p (u - mu')^2 = sum p (u - mu)^2 - s (mu' - mu)^2)
//   bias_estep_kernel<true>   the posteriors once more, R and W written as one (R, W) pair per voxel
//   bias_smooth_kernel    one axis of the separable Gaussian on both channels: a tile of 64 samples along the axis by 16 lines with its halo
//                         of r samples either side in LDS, zeros outside the volume, taps in ascending order, weights from scalar loads
//   bias_update_kernel, bias_bmean_kernel / bias_bmean_final, bias_recentre_kernel, bias_apply_kernel
// Every loop is bounded by a shape or a compile-time constant; fp64 throughout.  The record, the fixed-order sums, the kernels from
// bias_log_kernel to bias_mstep_kernel and the host code that enqueues them are in bias_common.hpp, which met2_seg.hip (the tissue
// segmentation, FAST's Markov random field labelling on the same classes) includes too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "bias_common.hpp"

namespace {

struct SmoothArgs {
    const double2 *src;
    double2 *dst;
    const double *w;                      // [2 r + 1]
    int r;
    int A, C, O;                          // the axis' length, the lines of one slab, the slabs
    int64_t sa, sc, so;                   // their strides
};

// AXIS_FAST: the axis is the contiguous one (z); the tile then lies in LDS line by line, otherwise sample by sample, so that a wave's lanes
// read and write consecutive addresses in both memories either way.  Tiles are numbered along blockIdx.x: at most one per voxel.
template <bool AXIS_FAST>
__global__ __launch_bounds__(256) void bias_smooth_kernel(SmoothArgs P)
{
    __shared__ double2 tile[(BIAS_TA + 2 * BIAS_MAX_R) * BIAS_TC];
    const int nta = (P.A + BIAS_TA - 1) / BIAS_TA, ntc = (P.C + BIAS_TC - 1) / BIAS_TC;
    int bid = blockIdx.x;
    const int ta = bid % nta;
    bid /= nta;
    const int tc = bid % ntc, o = bid / ntc;
    const int a0 = ta * BIAS_TA, c0 = tc * BIAS_TC;
    const int rows = BIAS_TA + 2 * P.r;                               // <= BIAS_TA + 2 BIAS_MAX_R: r is checked by the entry
    const double2 *src = P.src + (int64_t)o * P.so;
    double2 *dst = P.dst + (int64_t)o * P.so;
    for (int e = threadIdx.x; e < rows * BIAS_TC; e += 256) {
        const int ia = AXIS_FAST ? e % rows : e / BIAS_TC, ic = AXIS_FAST ? e / rows : e % BIAS_TC;
        const int a = a0 - P.r + ia, c = c0 + ic;
        tile[e] = a >= 0 && a < P.A && c < P.C ? src[(int64_t)a * P.sa + (int64_t)c * P.sc] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    const int step = AXIS_FAST ? 1 : BIAS_TC;
    for (int e = threadIdx.x; e < BIAS_TA * BIAS_TC; e += 256) {
        const int ia = AXIS_FAST ? e % BIAS_TA : e / BIAS_TC, ic = AXIS_FAST ? e / BIAS_TA : e % BIAS_TC;
        const int a = a0 + ia, c = c0 + ic;
        if (a < P.A && c < P.C) {
            const double2 *tp = tile + (AXIS_FAST ? ic * rows + ia : ia * BIAS_TC + ic);
            double sr = 0.0, sw = 0.0;
            for (int t = 0; t <= 2 * P.r; ++t) {
                const double w = P.w[t];
                const double2 x = tp[t * step];
                sr = fma(w, x.x, sr);
                sw = fma(w, x.y, sw);
            }
            dst[(int64_t)a * P.sa + (int64_t)c * P.sc] = make_double2(sr, sw);
        }
    }
}

__global__ __launch_bounds__(256) void bias_update_kernel(const double2 *__restrict__ S, int64_t n, double *__restrict__ b)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const double2 s = S[i];
        if (s.y > 0.0) b[i] += s.x / s.y;
    }
}

__global__ __launch_bounds__(256) void bias_bmean_kernel(const double *__restrict__ b, const int32_t *__restrict__ idx, const BiasStats *st,
                                                         double *__restrict__ part)
{
    __shared__ double red[4];
    const int N = st->N;
    const int64_t c0 = (int64_t)blockIdx.x * BIAS_CHUNK;
    if (st->degenerate || c0 >= N) return;
    double s = 0.0;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < N) s += b[idx[i]];
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void bias_bmean_final(const double *__restrict__ part, BiasStats *st)
{
    __shared__ double red[4];
    if (st->degenerate) return;
    const int N = st->N;
    const double s = partial_sum(part, (int)(((int64_t)N + BIAS_CHUNK - 1) / BIAS_CHUNK), red);
    if (threadIdx.x == 0) st->bmean = s / (double)N;
}

__global__ __launch_bounds__(256) void bias_recentre_kernel(const double2 *__restrict__ S, int64_t n, const BiasStats *st, double *__restrict__ b)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && S[i].y > 0.0) b[i] -= st->bmean;
}

__global__ __launch_bounds__(256) void bias_apply_kernel(const double *__restrict__ v, const double *__restrict__ b, int64_t n, const BiasStats *st,
                                                         int K, double *__restrict__ out, double *__restrict__ field, double *__restrict__ classes)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const double f = exp(b[i]);                                   // exp(0) = 1 off the support
        const double val = v[i];
        if (field) field[i] = f;
        out[i] = isfinite(val) ? val / f : val;
    }
    if (classes && blockIdx.x == 0 && threadIdx.x < K) {
        classes[threadIdx.x] = st->mu[threadIdx.x];
        classes[K + threadIdx.x] = st->var[threadIdx.x];
        classes[2 * K + threadIdx.x] = st->pi[threadIdx.x];
    }
}

// ---- the host code of the stages: each enqueues its launches on st and reads nothing back.  met2_bias_field and the stage entries below
// ---- (met2_bias_domain .. met2_bias_apply) run these helpers and launch no kernel of the filter otherwise.
// step 1's radii and weights on the host: hw[a][2 BIAS_MAX_R + 1], axis a's 2 rad[a] + 1 weights first in its row
int bias_weights(double fwhm_mm, const double voxel_mm[3], int rad[3], double *hw)
{
    for (int a = 0; a < 3; ++a) {
        const double sigma = fwhm_mm / (2.0 * std::sqrt(2.0 * std::log(2.0))) / voxel_mm[a];
        if (4.0 * sigma + 0.5 >= (double)(BIAS_MAX_R + 1)) return fail(MET2_E_UNSUPPORTED, "the smoothing kernel reaches further than 64 voxels");
        rad[a] = (int)(4.0 * sigma + 0.5);
        double *w = hw + a * (2 * BIAS_MAX_R + 1), sum = 0.0;
        for (int t = -rad[a]; t <= rad[a]; ++t) {
            w[t + rad[a]] = rad[a] == 0 ? 1.0 : std::exp(-((double)t * (double)t) / (2.0 * sigma * sigma));
            sum += w[t + rad[a]];
        }
        for (int t = 0; t <= 2 * rad[a]; ++t) w[t] /= sum;
    }
    return MET2_OK;
}

// RW = (R, W) on the domain and 0 off it; rw_bytes of it are cleared first
hipError_t enq_rw(hipStream_t st, const BiasGrid &g, const double *y, const double *b, const int32_t *idx, const BiasStats *S, int K, double2 *RW,
                  size_t rw_bytes)
{
    const hipError_t e = hipMemsetAsync(RW, 0, rw_bytes, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bias_estep_kernel<true>, dim3(g.nch), dim3(256), 0, st, y, b, idx, S, K, g.nch, (double *)nullptr, RW);
    return hipSuccess;
}

// x: nx samples at stride ny nz, the lines are the ny nz contiguous voxels; y: per x a slab of nz lines; z: contiguous, one line per (x, y)
SmoothArgs smooth_args(int a, int nx, int ny, int nz, const double2 *src, double2 *dst, const double *w, int r)
{
    SmoothArgs P;
    P.src = src; P.dst = dst; P.w = w; P.r = r;
    if (a == 0) { P.A = nx; P.C = (int)((int64_t)ny * nz); P.O = 1; P.sa = (int64_t)ny * nz; P.sc = 1; P.so = 0; }
    else if (a == 1) { P.A = ny; P.C = nz; P.O = nx; P.sa = nz; P.sc = 1; P.so = (int64_t)ny * nz; }
    else { P.A = nz; P.C = (int)((int64_t)nx * ny); P.O = 1; P.sa = 1; P.sc = nz; P.so = 0; }
    return P;
}

void enq_smooth(hipStream_t st, int a, const SmoothArgs &P)
{
    const int64_t tiles = (int64_t)((P.A + BIAS_TA - 1) / BIAS_TA) * ((P.C + BIAS_TC - 1) / BIAS_TC) * P.O;      // <= n
    if (a == 2)
        hipLaunchKernelGGL(bias_smooth_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, st, P);
    else
        hipLaunchKernelGGL(bias_smooth_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, st, P);
}

// b += S_R / S_W on D, S->bmean = mean_Omega(b), b -= bmean on D
void enq_update(hipStream_t st, const BiasGrid &g, const double2 *SRW, const int32_t *idx, BiasStats *S, double *part, double *b)
{
    const dim3 T(256), GC(g.nch), GE(g.nel), G1(1);
    hipLaunchKernelGGL(bias_update_kernel, GE, T, 0, st, SRW, g.n, b);
    hipLaunchKernelGGL(bias_bmean_kernel, GC, T, 0, st, b, idx, S, part);
    hipLaunchKernelGGL(bias_bmean_final, G1, T, 0, st, part, S);
    hipLaunchKernelGGL(bias_recentre_kernel, GE, T, 0, st, SRW, g.n, S, b);
}

void enq_apply(hipStream_t st, const BiasGrid &g, const double *v, const double *b, const BiasStats *S, int K, double *out, double *field,
               double *classes)
{
    hipLaunchKernelGGL(bias_apply_kernel, dim3(g.nel), dim3(256), 0, st, v, b, g.n, S, K, out, field, classes);
}

}  // namespace

extern "C" int met2_bias_field(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const uint8_t *mask, const double voxel_mm[3],
                               int32_t n_class, int32_t n_outer, int32_t n_em, double fwhm_mm, double *out, double *field, double *classes,
                               void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0) return fail(MET2_E_INVALID, "bad shape");
    if (n_class < 1) return fail(MET2_E_INVALID, "bias field needs at least one class");
    if (n_outer < 0 || n_em < 1) return fail(MET2_E_INVALID, "bias field needs n_outer >= 0 and n_em >= 1");
    if (!voxel_mm) return fail(MET2_E_INVALID, "NULL voxel size");
    if (!(fwhm_mm > 0.0) || !std::isfinite(fwhm_mm)) return fail(MET2_E_INVALID, "the smoothing width must be positive and finite");
    for (int a = 0; a < 3; ++a)
        if (!(voxel_mm[a] > 0.0) || !std::isfinite(voxel_mm[a])) return fail(MET2_E_INVALID, "the voxel size must be positive and finite");
    const int64_t n = (int64_t)nx * ny * nz;
    if (n == 0) return MET2_OK;
    if (!v || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (v == out) return fail(MET2_E_INVALID, "the bias field cannot be removed in place");
    if (n_class > BIAS_MAX_K) return fail(MET2_E_UNSUPPORTED, "bias field supports at most 8 classes");
    if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    int rad[3];
    std::vector<double> hw(3 * (2 * BIAS_MAX_R + 1), 0.0);
    if (int rc = bias_weights(fwhm_mm, voxel_mm, rad, hw.data())) return rc;
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;

    const BiasGrid g = bias_grid(n);
    const int nch = g.nch;
    DeviceWork W(st);
    const auto y = W.take<double>(n), b = W.take<double>(n);
    const auto RA = W.take<double2>(n), RB = W.take<double2>(n);
    const auto idx = W.take<int32_t>(n);
    const auto dom = W.take<uint8_t>(n);
    const auto cnt = W.take<int32_t>(nch), off = W.take<int32_t>(nch);
    const auto part = W.take<double>((size_t)nch * 3 * BIAS_MAX_K);
    const auto S = W.take<BiasStats>(1);
    const auto wd = W.take<double>(hw.size());
    if (!W.alloc()) return W.finish("met2_bias_field");

    W.ok(hipMemsetAsync(S, 0, S.bytes, st));
    W.ok(hipMemsetAsync(b, 0, b.bytes, st));
    W.ok(hipMemcpyAsync(wd, hw.data(), hw.size() * 8, hipMemcpyHostToDevice, st));    // hw lives until the wait below
    if (W.ok()) {
        enq_domain(st, g, v, mask, y, dom, cnt, off, idx, S);
        enq_init(st, g, y, idx, S, part, n_class);
        W.ok(hipGetLastError());
    }
    SmoothArgs P[3];
    P[0] = smooth_args(0, nx, ny, nz, RA, RB, wd, rad[0]);
    P[1] = smooth_args(1, nx, ny, nz, RB, RA, wd + (2 * BIAS_MAX_R + 1), rad[1]);
    P[2] = smooth_args(2, nx, ny, nz, RA, RB, wd + 2 * (2 * BIAS_MAX_R + 1), rad[2]);
    for (int it = 0; it < n_outer && W.ok(); ++it) {
        for (int em = 0; em < n_em; ++em) enq_em_step(st, g, y, b, idx, S, n_class, part);
        if (!W.ok(enq_rw(st, g, y, b, idx, S, n_class, RA, RA.bytes))) break;  // R = W = 0 off the domain; the y pass of the last round wrote here
        for (int a = 0; a < 3; ++a) enq_smooth(st, a, P[a]);
        enq_update(st, g, RB, idx, S, part, b);
        W.ok(hipGetLastError());
    }
    if (W.ok()) enq_apply(st, g, v, b, S, n_class, out, field, classes);
    return W.finish("met2_bias_field");
}

// ---- the stages one by one, for tests and diagnostics (include/met2_hip.h) ----

static int bias_check_list(int64_t n, const void *idx, int64_t N)
{
    if (n < 1) return fail(MET2_E_INVALID, "the bias stages need at least one voxel");
    if (N < 0 || N > n) return fail(MET2_E_INVALID, "the domain's size must lie in 0..n");
    if (!idx) return fail(MET2_E_INVALID, "NULL argument");
    if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    return MET2_OK;
}

extern "C" int met2_bias_weights(double fwhm_mm, const double voxel_mm[3], int32_t *radius_out, double *weights_out)
{
    if (!voxel_mm || !radius_out || !weights_out) return fail(MET2_E_INVALID, "NULL argument");
    if (!(fwhm_mm > 0.0) || !std::isfinite(fwhm_mm)) return fail(MET2_E_INVALID, "the smoothing width must be positive and finite");
    for (int a = 0; a < 3; ++a)
        if (!(voxel_mm[a] > 0.0) || !std::isfinite(voxel_mm[a])) return fail(MET2_E_INVALID, "the voxel size must be positive and finite");
    int rad[3];
    std::vector<double> hw(3 * (2 * BIAS_MAX_R + 1), 0.0);
    if (int rc = bias_weights(fwhm_mm, voxel_mm, rad, hw.data())) return rc;
    for (int a = 0; a < 3; ++a) {
        radius_out[a] = rad[a];
        for (int t = 0; t <= 2 * rad[a]; ++t) *weights_out++ = hw[a * (2 * BIAS_MAX_R + 1) + t];
    }
    return MET2_OK;
}

extern "C" int met2_bias_domain(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const uint8_t *mask, double *y, int32_t *idx,
                                int64_t *n_domain, void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0) return fail(MET2_E_INVALID, "bad shape");
    if (!n_domain) return fail(MET2_E_INVALID, "NULL argument");
    const int64_t n = (int64_t)nx * ny * nz;
    *n_domain = 0;
    if (n == 0) return MET2_OK;
    if (!v || !y || !idx) return fail(MET2_E_INVALID, "NULL argument");
    if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const BiasGrid g = bias_grid(n);
    DeviceWork W(st);
    const auto dom = W.take<uint8_t>(n);
    const auto cnt = W.take<int32_t>(g.nch), off = W.take<int32_t>(g.nch);
    const auto S = W.take<BiasStats>(1);
    if (!W.alloc()) return W.finish("met2_bias_domain");
    int32_t N = 0;
    if (W.ok(hipMemsetAsync(S, 0, S.bytes, st))) {
        enq_domain(st, g, v, mask, y, dom, cnt, off, idx, S);
        W.ok(hipGetLastError());
    }
    if (W.ok()) W.ok(hipMemcpyAsync(&N, &S->N, sizeof N, hipMemcpyDeviceToHost, st));
    const int rc = W.finish("met2_bias_domain");
    if (rc == MET2_OK) *n_domain = N;
    return rc;
}

extern "C" int met2_bias_init(int32_t device, int64_t n, const double *y, const int32_t *idx, int64_t n_domain, int32_t n_class, double *stats_out,
                              uint32_t *hist_out, double *ss_part_out, double *classes_out, void *stream)
{
    if (n_class < 1) return fail(MET2_E_INVALID, "bias field needs at least one class");
    if (int rc = bias_check_list(n, idx, n_domain)) return rc;
    if (!y) return fail(MET2_E_INVALID, "NULL argument");
    if (n_class > BIAS_MAX_K) return fail(MET2_E_UNSUPPORTED, "bias field supports at most 8 classes");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const BiasGrid g = bias_grid(n);
    const int np = (int)((n_domain + BIAS_CHUNK - 1) / BIAS_CHUNK);
    DeviceWork W(st);
    const auto part = W.take<double>((size_t)g.nch * 3 * BIAS_MAX_K);
    const auto S = W.take<BiasStats>(1);
    if (!W.alloc()) return W.finish("met2_bias_init");
    BiasStats h;
    std::vector<double> hp((size_t)np);
    const int32_t N = (int32_t)n_domain;
    if (W.ok(hipMemsetAsync(S, 0, S.bytes, st)) && W.ok(hipMemcpyAsync(&S->N, &N, sizeof N, hipMemcpyHostToDevice, st))) {
        enq_init(st, g, y, idx, S, part, n_class);
        W.ok(hipGetLastError());
    }
    if (W.ok()) W.ok(hipMemcpyAsync(&h, S, sizeof h, hipMemcpyDeviceToHost, st));
    if (W.ok() && np > 0) W.ok(hipMemcpyAsync(hp.data(), part, (size_t)np * 8, hipMemcpyDeviceToHost, st));
    const int rc = W.finish("met2_bias_init");
    if (rc != MET2_OK) return rc;
    if (stats_out) { stats_out[0] = h.lo; stats_out[1] = h.hi; stats_out[2] = h.mean; stats_out[3] = (double)h.degenerate; }
    if (hist_out) for (int j = 0; j < BIAS_NBINS; ++j) hist_out[j] = h.hist[j];
    if (ss_part_out && !h.degenerate) for (int p = 0; p < np; ++p) ss_part_out[p] = hp[p];
    if (classes_out)
        for (int k = 0; k < n_class; ++k) { classes_out[k] = h.mu[k]; classes_out[n_class + k] = h.var[k]; classes_out[2 * n_class + k] = h.pi[k]; }
    return MET2_OK;
}

extern "C" int met2_bias_em(int32_t device, int64_t n, const double *y, const double *b, const int32_t *idx, int64_t n_domain, int32_t n_class,
                            const double *classes_in, int32_t n_em, double *part_out, double *classes_out, double *rw_out, void *stream)
{
    if (n_class < 1) return fail(MET2_E_INVALID, "bias field needs at least one class");
    if (n_em < 0) return fail(MET2_E_INVALID, "n_em must not be negative");
    if (int rc = bias_check_list(n, idx, n_domain)) return rc;
    if (!y || !b || !classes_in) return fail(MET2_E_INVALID, "NULL argument");
    if (n_domain < 1) return fail(MET2_E_INVALID, "the EM step needs a domain voxel");
    if (n_class > BIAS_MAX_K) return fail(MET2_E_UNSUPPORTED, "bias field supports at most 8 classes");
    BiasStats h;
    std::memset(&h, 0, sizeof h);
    h.N = (int32_t)n_domain;
    for (int k = 0; k < n_class; ++k) {
        h.mu[k] = classes_in[k]; h.var[k] = classes_in[n_class + k]; h.pi[k] = classes_in[2 * n_class + k];
        if (!std::isfinite(h.mu[k]) || !std::isfinite(h.var[k]) || !(h.var[k] > 0.0) || !std::isfinite(h.pi[k]) || h.pi[k] < 0.0)
            return fail(MET2_E_INVALID, "a class needs a finite mean, a positive finite variance and a finite weight >= 0");
    }
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const BiasGrid g = bias_grid(n);
    const int np = (int)((n_domain + BIAS_CHUNK - 1) / BIAS_CHUNK);
    DeviceWork W(st);
    const auto part = W.take<double>((size_t)g.nch * 3 * BIAS_MAX_K);
    const auto S = W.take<BiasStats>(1);
    if (!W.alloc()) return W.finish("met2_bias_em");
    std::vector<double> hp((size_t)3 * n_class * np);
    if (W.ok(hipMemcpyAsync(S, &h, sizeof h, hipMemcpyHostToDevice, st))) {               // h lives until the wait
        hipLaunchKernelGGL(bias_lc_kernel, dim3(1), dim3(64), 0, st, S, n_class);
        for (int em = 0; em < n_em; ++em) enq_em_step(st, g, y, b, idx, S, n_class, part);
        W.ok(hipGetLastError());
    }
    if (W.ok() && rw_out) W.ok(enq_rw(st, g, y, b, idx, S, n_class, (double2 *)rw_out, (size_t)n * 16));
    if (part_out && n_em > 0)
        for (int q = 0; q < 3; ++q)
            for (int k = 0; k < n_class && W.ok(); ++k)
                W.ok(hipMemcpyAsync(hp.data() + ((size_t)q * n_class + k) * np, part + (int64_t)(q * BIAS_MAX_K + k) * g.nch, (size_t)np * 8,
                                    hipMemcpyDeviceToHost, st));
    if (W.ok()) W.ok(hipMemcpyAsync(&h, S, sizeof h, hipMemcpyDeviceToHost, st));
    const int rc = W.finish("met2_bias_em");
    if (rc != MET2_OK) return rc;
    if (part_out && n_em > 0) std::memcpy(part_out, hp.data(), hp.size() * 8);
    if (classes_out)
        for (int k = 0; k < n_class; ++k) { classes_out[k] = h.mu[k]; classes_out[n_class + k] = h.var[k]; classes_out[2 * n_class + k] = h.pi[k]; }
    return MET2_OK;
}

extern "C" int met2_bias_smooth(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *in, const int32_t radius[3], const double *weights,
                                int32_t axis, double *out, void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0) return fail(MET2_E_INVALID, "bad shape");
    if (axis < -1 || axis > 2) return fail(MET2_E_INVALID, "axis must be 0, 1, 2 or -1 for all three");
    if (!radius || !weights) return fail(MET2_E_INVALID, "NULL argument");
    for (int a = 0; a < 3; ++a)
        if (radius[a] < 0) return fail(MET2_E_INVALID, "a radius must not be negative");
    const int64_t n = (int64_t)nx * ny * nz;
    if (n == 0) return MET2_OK;
    if (!in || !out) return fail(MET2_E_INVALID, "NULL argument");
    for (int a = 0; a < 3; ++a)
        if (radius[a] > BIAS_MAX_R) return fail(MET2_E_UNSUPPORTED, "the smoothing kernel reaches further than 64 voxels");
    if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> hw(3 * (2 * BIAS_MAX_R + 1), 0.0);                                // the filter's layout of the three weight vectors
    const double *w = weights;
    for (int a = 0; a < 3; ++a) {
        for (int t = 0; t <= 2 * radius[a]; ++t) hw[a * (2 * BIAS_MAX_R + 1) + t] = w[t];
        w += 2 * radius[a] + 1;
    }
    DeviceWork W(st);
    const auto RA = W.take<double2>(n), RB = W.take<double2>(n);
    const auto wd = W.take<double>(hw.size());
    if (!W.alloc()) return W.finish("met2_bias_smooth");
    W.ok(hipMemcpyAsync(wd, hw.data(), hw.size() * 8, hipMemcpyHostToDevice, st));              // hw lives until the wait
    if (W.ok()) W.ok(hipMemcpyAsync(RA, in, (size_t)n * 16, hipMemcpyDeviceToDevice, st));
    double2 *res = RB;
    if (W.ok()) {
        if (axis < 0) {                                               // RA -> RB -> RA -> RB, as the filter
            enq_smooth(st, 0, smooth_args(0, nx, ny, nz, RA, RB, wd, radius[0]));
            enq_smooth(st, 1, smooth_args(1, nx, ny, nz, RB, RA, wd + (2 * BIAS_MAX_R + 1), radius[1]));
            enq_smooth(st, 2, smooth_args(2, nx, ny, nz, RA, RB, wd + 2 * (2 * BIAS_MAX_R + 1), radius[2]));
        } else {
            enq_smooth(st, axis, smooth_args(axis, nx, ny, nz, RA, RB, wd + axis * (2 * BIAS_MAX_R + 1), radius[axis]));
        }
        W.ok(hipGetLastError());
    }
    if (W.ok()) W.ok(hipMemcpyAsync(out, res, (size_t)n * 16, hipMemcpyDeviceToDevice, st));
    return W.finish("met2_bias_smooth");
}

extern "C" int met2_bias_update(int32_t device, int64_t n, double *b, const double *smoothed, const int32_t *idx, int64_t n_domain, double *bmean_out,
                                void *stream)
{
    if (int rc = bias_check_list(n, idx, n_domain)) return rc;
    if (!b || !smoothed) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const BiasGrid g = bias_grid(n);
    DeviceWork W(st);
    const auto part = W.take<double>(g.nch);
    const auto S = W.take<BiasStats>(1);
    if (!W.alloc()) return W.finish("met2_bias_update");
    BiasStats h;
    std::memset(&h, 0, sizeof h);
    h.N = (int32_t)n_domain;
    h.degenerate = n_domain == 0 ? 1 : 0;                             // an empty domain is degenerate in the filter too: b is not recentred
    if (W.ok(hipMemcpyAsync(S, &h, sizeof h, hipMemcpyHostToDevice, st))) {               // h lives until the wait
        enq_update(st, g, (const double2 *)smoothed, idx, S, part, b);
        W.ok(hipGetLastError());
    }
    double bmean = 0.0;
    if (W.ok()) W.ok(hipMemcpyAsync(&bmean, &S->bmean, 8, hipMemcpyDeviceToHost, st));
    const int rc = W.finish("met2_bias_update");
    if (rc == MET2_OK && bmean_out) *bmean_out = bmean;
    return rc;
}

extern "C" int met2_bias_apply(int32_t device, int64_t n, const double *v, const double *b, double *out, double *field, void *stream)
{
    if (n < 0) return fail(MET2_E_INVALID, "bad shape");
    if (n == 0) return MET2_OK;
    if (!v || !b || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (v == out) return fail(MET2_E_INVALID, "the bias field cannot be removed in place");
    if (n > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    enq_apply(st, bias_grid(n), v, b, (const BiasStats *)nullptr, 0, out, field, (double *)nullptr);    // no classes: the record is not read
    return DeviceWork(st).finish("met2_bias_apply");
}
