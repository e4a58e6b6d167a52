// met2_roi_metrics.hip -- met2_roi_reduce and met2_metrics.
//
// Kernels
//   roi_partial_kernel, roi_finish_kernel   motor_recon_met2_real_data_ROI.py:405-420: per-ROI mean signal and mean kernel
//   metrics_kernel                          motor:443-472 standalone
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
#include "metrics.hpp"
#include "plan.hpp"
#include "wave_ops.hpp"

using namespace met2;

// motor:443-472 standalone: one wavefront per voxel
template <int NB>
__global__ __launch_bounds__(256) void metrics_kernel(int64_t nvox, int n, const double *__restrict__ t2s, double cut_m, double cut_ie,
                                                      const double *__restrict__ fsol, const uint8_t *__restrict__ mask,
                                                      double *__restrict__ maps)
{
    const int lane = lane_id();
    MetricLanes<NB> ml;
    metric_lanes<NB>(ml, t2s, n, cut_m, cut_ie, lane);
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t v = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; v < nvox; v += nw) {
        const bool mk = mask ? (mask[v] != 0) : true;
        double xs[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) xs[b] = (lane + 64 * b < n && mk) ? fsol[(size_t)v * n + lane + 64 * b] : 0.0;
        write_metrics<NB>(ml, xs, mk, maps, nvox, v, lane);
    }
}

// ------------------------------------------------------------------------------------------
// ROI mode (motor/motor_recon_met2_real_data_ROI.py:405-420): per ROI the mean signal over its voxels and the mean
// EPG kernel (every voxel contributes the dictionary slice of its own flip angle).  Deterministic two-level
// reduction: a wave per (slice of the voxel list, ROI) accumulates the echoes of its matching voxels in voxel order
// (lane <-> echo) and a flip-angle histogram; one workgroup per ROI then adds the slices in order and forms
// mean kernel = sum_fa count[fa] D[fa] / nv.
// ------------------------------------------------------------------------------------------
struct RoiArgs {
    int nte, nt2, nfa, nroi, nslice;
    int64_t nvox, vs, es;
    const double *data;
    const int32_t *roi;        // [nvox] ROI ordinal 0..nroi-1, negative = none
    const double *fa_index;    // [nvox] or NULL
    double *part_sig;          // [nroi][nslice][64]
    int *part_cnt;             // [nroi][nslice][nfa]
    const double *Dsrc;        // [nfa][nte][nt2]
    double *Ddst;              // [nroi][nte][nt2]
    double *mean_sig;          // [nroi][nte]
    double *count;             // [nroi] voxels per ROI
    int *err;
};

__global__ __launch_bounds__(64) void roi_partial_kernel(RoiArgs A)
{
    extern __shared__ int roi_hist[];
    const int lane = lane_id();
    const int sl = (int)blockIdx.x, r = (int)blockIdx.y;
    for (int f = lane; f < A.nfa; f += 64) roi_hist[f] = 0;
    __builtin_amdgcn_wave_barrier();
    const int64_t per = (A.nvox + A.nslice - 1) / A.nslice;
    const int64_t lo = sl * per, hi = min(A.nvox, lo + per);
    double acc = 0.0;
    for (int64_t base = lo; base < hi; base += 64) {
        const int64_t v = base + lane;
        u64 hit = ballot(v < hi && A.roi[v] == r);
        while (hit) {
            const int bit = first_lane(hit);
            hit &= hit - 1ull;
            const int64_t vv = base + bit;
            if (lane < A.nte) acc += A.data[vv * A.vs + lane * A.es];
            const int fa = A.fa_index ? (int)A.fa_index[vv] : 0;
            if (fa < 0 || fa >= A.nfa) { if (lane == 0) atomicOr(A.err, 1); }
            else if (lane == 0) roi_hist[fa] += 1;
        }
    }
    __builtin_amdgcn_wave_barrier();
    A.part_sig[((size_t)r * A.nslice + sl) * 64 + lane] = acc;
    for (int f = lane; f < A.nfa; f += 64) A.part_cnt[((size_t)r * A.nslice + sl) * A.nfa + f] = roi_hist[f];
}

__global__ __launch_bounds__(256) void roi_finish_kernel(RoiArgs A)
{
    extern __shared__ int roi_tot[];           // [nfa]
    __shared__ double s_nv;
    const int r = (int)blockIdx.x;
    for (int f = threadIdx.x; f < A.nfa; f += blockDim.x) {
        int c = 0;
        for (int sl = 0; sl < A.nslice; ++sl) c += A.part_cnt[((size_t)r * A.nslice + sl) * A.nfa + f];
        roi_tot[f] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long nv = 0;
        for (int f = 0; f < A.nfa; ++f) nv += roi_tot[f];
        s_nv = (double)nv;
        A.count[r] = (double)nv;
    }
    __syncthreads();
    const double nv = s_nv;
    if ((int)threadIdx.x < A.nte) {
        double t = 0.0;
        for (int sl = 0; sl < A.nslice; ++sl) t += A.part_sig[((size_t)r * A.nslice + sl) * 64 + threadIdx.x];
        A.mean_sig[(size_t)r * A.nte + threadIdx.x] = t / nv;
    }
    const int sz = A.nte * A.nt2;
    for (int i = threadIdx.x; i < sz; i += blockDim.x) {
        double t = 0.0;
        for (int f = 0; f < A.nfa; ++f) { const int c = roi_tot[f]; if (c) t = fma((double)c, A.Dsrc[(size_t)f * sz + i], t); }
        A.Ddst[(size_t)r * sz + i] = t / nv;
    }
}

extern "C" {

int met2_roi_reduce(met2_plan *src, met2_plan *dst, int64_t nvox, const double *data, int64_t voxel_stride, int64_t echo_stride,
                    const int32_t *roi_index, const double *fa_index, double *mean_signal, double *count, void *stream)
{
    if (!src || !dst || !data || !roi_index || !mean_signal || !count) return fail(MET2_E_INVALID, "NULL argument");
    if (!src->have_dict) return fail(MET2_E_STATE, "no dictionary in the source plan");
    if (src->n_te != dst->n_te || src->n_t2 != dst->n_t2) return fail(MET2_E_INVALID, "source and destination plans differ in shape");
    if (src->opt.device != dst->opt.device) return fail(MET2_E_INVALID, "source and destination plans live on different devices");
    if (voxel_stride == 0 || echo_stride == 0) return fail(MET2_E_INVALID, "zero stride");
    if (nvox <= 0) return fail(MET2_E_INVALID, "empty voxel list");
    USE_DEVICE(src->opt.device);
    hipStream_t s = (hipStream_t)stream;
    RoiArgs A;
    A.nte = src->n_te; A.nt2 = src->n_t2; A.nfa = src->n_fa; A.nroi = dst->n_fa;
    A.nslice = (int)std::min<int64_t>(256, (nvox + 4095) / 4096);
    A.nvox = nvox; A.vs = voxel_stride; A.es = echo_stride; A.data = data; A.roi = roi_index; A.fa_index = fa_index;
    A.Dsrc = src->dD; A.Ddst = dst->dD; A.mean_sig = mean_signal; A.count = count;
    void *scratch = nullptr;
    const size_t nsig = sizeof(double) * (size_t)A.nroi * A.nslice * 64, ncnt = sizeof(int) * (size_t)A.nroi * A.nslice * A.nfa;
    HIPCHK(hipMalloc(&scratch, nsig + ncnt + 16));
    A.part_sig = (double *)scratch; A.part_cnt = (int *)((char *)scratch + nsig); A.err = (int *)((char *)scratch + nsig + ncnt);
    HIPCHK(hipMemsetAsync(A.err, 0, sizeof(int), s));
    hipLaunchKernelGGL(roi_partial_kernel, dim3(A.nslice, A.nroi), dim3(64), sizeof(int) * A.nfa, s, A);
    hipLaunchKernelGGL(roi_finish_kernel, dim3(A.nroi), dim3(256), sizeof(int) * A.nfa, s, A);
    HIPCHK(hipGetLastError());
    int rc = build_gram(dst, s);
    int herr = 0;
    HIPCHK(hipMemcpyAsync(&herr, A.err, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipFree(scratch));
    if (rc) return rc;
    rc = ensure_seeds(dst, s);
    if (rc) return rc;
    if (herr & 1) return fail(MET2_E_INVALID, "FA index outside the dictionary's flip-angle axis");
    return MET2_OK;
}

int met2_metrics(met2_plan *p, int64_t nvox, const double *fsol, const uint8_t *mask, double *maps, void *stream)
{
    if (!p || !fsol || !maps) return fail(MET2_E_INVALID, "NULL argument");
    if (!p->have_t2) return fail(MET2_E_STATE, "no T2 grid set");
    if (nvox <= 0) return MET2_OK;
    USE_DEVICE(p->opt.device);
    int blocks = (int)((nvox + 3) / 4);
    if (blocks > p->cus * 16) blocks = p->cus * 16;
    if (p->n_t2 <= 64)
        hipLaunchKernelGGL(metrics_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, nvox, p->n_t2, p->dT2, p->opt.t2_myelin_cut,
                           p->opt.t2_ie_cut, fsol, mask, maps);
    else
        hipLaunchKernelGGL(metrics_kernel<2>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, nvox, p->n_t2, p->dT2, p->opt.t2_myelin_cut,
                           p->opt.t2_ie_cut, fsol, mask, maps);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

} // extern "C"
