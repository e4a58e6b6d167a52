// metrics.hpp -- the metrics of one spectrum (motor:443-472) on a wave: the epilogue of the fit kernels (fit_kernel.hpp) and the stand-alone
// metrics_kernel (met2_roi_metrics.hip) share it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wave_ops.hpp"

using namespace met2;

// Per-lane constants of the metrics windows (motor:221-224, 444)
template <int NB>
struct MetricLanes {
    double logt2[NB];
    bool isM[NB], isIE[NB], isCSF[NB];
};

template <int NB>
__device__ __forceinline__ void metric_lanes(MetricLanes<NB> &ml, const double *t2s, int n, double cut_m, double cut_ie, int lane)
{
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = lane + 64 * b;
        const double t2 = (j < n) ? t2s[j] : 1.0;
        ml.logt2[b] = (j < n) ? log(t2) : 0.0;
        ml.isM[b] = (j < n) && (t2 <= cut_m);
        ml.isIE[b] = (j < n) && (t2 > cut_m) && (t2 <= cut_ie);
        ml.isCSF[b] = (j < n) && (t2 >= cut_ie);
    }
}

// motor:448-468 for one voxel held bin-indexed in xs (already un-normalised); lane 0 writes the six maps
template <int NB>
__device__ __forceinline__ void write_metrics(const MetricLanes<NB> &ml, const double (&xs)[NB], bool mk, double *maps, int64_t nvox,
                                              int64_t v, int lane)
{
    const double epsilon = 1.0e-16;
    double tot = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) tot += xs[b];
    const double vt = wave_sum(tot) + epsilon;
    double fm = 0.0, fie = 0.0, fcsf = 0.0, lm = 0.0, lie = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const double xn = xs[b] / vt;
        fm += ml.isM[b] ? xn : 0.0;
        fie += ml.isIE[b] ? xn : 0.0;
        fcsf += ml.isCSF[b] ? xn : 0.0;
        lm += ml.isM[b] ? xn * ml.logt2[b] : 0.0;
        lie += ml.isIE[b] ? xn * ml.logt2[b] : 0.0;
    }
    fcsf = wave_sum(fcsf);
    wave_sum2(fm, fie);
    wave_sum2(lm, lie);
    if (lane == 0) {
        maps[0 * nvox + v] = mk ? fm : 0.0;
        maps[1 * nvox + v] = mk ? fie : 0.0;
        maps[2 * nvox + v] = mk ? fcsf : 0.0;
        maps[3 * nvox + v] = mk ? exp(lm / (fm + epsilon)) : 0.0;
        maps[4 * nvox + v] = mk ? exp(lie / (fie + epsilon)) : 0.0;
        maps[5 * nvox + v] = mk ? vt : 0.0;
    }
}
