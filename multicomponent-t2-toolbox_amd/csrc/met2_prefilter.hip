// met2_prefilter.hip -- the steps of the driver that run before the fit and take a device ordinal, not a plan: met2_nesma,
// met2_smooth_separable and met2_fa_spline_select[_strided].
//
// Kernels
//   nesma_kernel            motor:305-333
//   nesma_one_echo_kernel   motor:305-333 at one echo
//   smooth_axis_kernel      motor:337-343
//   fa_spline_kernel        fa_estimation.py:54-59
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
#include "brent.hpp"
#include "device_work.hpp"
#include "plan.hpp"
#include "wave_ops.hpp"

using namespace met2;

// ------------------------------------------------------------------------------------------
// NESMA filter (motor:305-333): every voxel with mask == 1 becomes the mean of the voxels of its
// [x-6, x+6) x [y-6, y+6) x [z-6, z+6) window (clipped to the volume) whose relative L1 distance
// 100 * sum|s_nb - s_c| / sum(s_c) is below 2.5 %.  One wave per output voxel, lane <-> echo; the
// window is walked in batches of 8 neighbours: |s_nb - s_c| goes through the wave's LDS strip so
// that lane group q (8 lanes) can sum neighbour q in the order of numpy's pairwise sum (8 running
// sums, tree combine, tail in order), which keeps the 2.5 % test and the running mean bit-identical
// to the reference's np.sum / np.mean.  The four waves of a workgroup take consecutive z, so their
// windows overlap by 11/12 and the re-reads hit L1/L2.
// ------------------------------------------------------------------------------------------
#define MET2_NESMA_HW 6
#define MET2_NESMA_MAX_NT 128
struct NesmaArgs {
    int nx, ny, nz, nt;
    const double *data;       // [nx][ny][nz][nt]
    const uint8_t *mask;      // [nx][ny][nz], filtered where == 1 (NULL = everywhere)
    double *out;              // [nx][ny][nz][nt]
    int64_t nvox;
    int srow;                 // LDS row stride in doubles: >= nt, = 8 mod 32
};

// numpy pairwise sum of S[q][0..nt) for the lane's group q = lane / 8 (nt <= 128): valid on every lane of the group
__device__ __forceinline__ double np_rowsum_group(const double *Sq, int nt, int j)
{
    double r;
    if (nt < 8) {
        r = 0.0;
        for (int i = 0; i < nt; ++i) r += Sq[i];
        return r;
    }
    const int n8 = nt - (nt & 7);
    r = Sq[j];
    for (int i = 8; i < n8; i += 8) r += Sq[i + j];
    r = r + dpp_mov<0xB1>(r);       // r0+r1 | r2+r3 | ...
    r = r + dpp_mov<0x4E>(r);       // (r0+r1)+(r2+r3) | (r4+r5)+(r6+r7)
    r = r + dpp_mov<0x141>(r);      // both halves of the group
    for (int i = n8; i < nt; ++i) r += Sq[i];
    return r;
}

// RE < 2.5 with RE = fl(fl(100 S) / sumc), decided without the division whenever 100 S is clear of 2.5 sumc by
// more than the rounding of both sides (the exact quotient is only formed for the voxels inside that band)
struct NesmaTest {
    double sumc, lo, hi;
    bool fast;
    __device__ __forceinline__ void init(double sc)
    {
        sumc = sc; fast = sc > 0.0 && sc < 1e300;
        lo = 2.5 * sc * (1.0 - 1e-15); hi = 2.5 * sc * (1.0 + 1e-15);
    }
    __device__ __forceinline__ u64 similar(double S) const
    {
        const double t = 100.0 * S;
        const bool yes = t < lo, no = !(t <= hi);
        if (fast && ballot(!yes && !no) == 0ull) return ballot(yes);
        return ballot(t / sumc < 2.5);
    }
};

// the value the lane 32 above holds (v_permlane32_swap: upper half of one operand <-> lower half of the other)
__device__ __forceinline__ double from_upper_half(double v)
{
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double((int)b[1], (int)a[1]);
}

// One batch = the z-run of one (x, y) of the window: up to 12 neighbours that are contiguous in memory, so the
// window walk is two nested loops with a pointer bump and the batch geometry (run length L) is fixed per voxel.
// PACK = 1: lane <-> echo (NE echoes per lane), one neighbour per load.  PACK = 2 (nt <= 32): the two halves of the
// wave load two consecutive neighbours at once; the running sum lives in the lower half and takes the odd neighbours
// through v_permlane32_swap so that the additions keep the reference's order.  LDS rows are padded to a stride of
// 8 mod 32 doubles, which spreads the 8 lane groups of a row-sum read over all banks.
// NT > 0 fixes the echo count at compile time (row sums fully unrolled); NT = 0 reads it from the arguments.
template <int NE, int PACK, int NT>
__global__ __launch_bounds__(256) void nesma_kernel(NesmaArgs A)
{
    extern __shared__ double nesma_lds[];
    constexpr int STEPS = 2 * MET2_NESMA_HW / PACK;
    const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
    const int nt = NT > 0 ? NT : A.nt, SR = NT > 0 ? ((NT + 23) / 32) * 32 + 8 : A.srow;
    double *S = nesma_lds + (size_t)w * 2 * MET2_NESMA_HW * SR;
    // workgroups are dealt round-robin to the 8 XCDs: give XCD i the i-th contiguous eighth of the volume so that
    // the windows its CUs walk at the same time overlap in its own L2
    const unsigned nb = gridDim.x, per = (nb + 7u) / 8u;
    const unsigned bid = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    const int64_t v = (int64_t)bid * 4 + w;
    if (bid >= nb || v >= A.nvox) return;                      // wave-uniform
    const int h = PACK == 2 ? lane >> 5 : 0;
    const int e0 = PACK == 2 ? (lane & 31) : lane, e1 = lane + 64;
    const bool has0 = e0 < nt, has1 = NE > 1 && e1 < nt;
    const bool writer = h == 0;
    double *orow = A.out + v * nt;
    if (A.mask && A.mask[v] != 1) {
        if (has0 && writer) orow[e0] = 0.0;
        if (has1) orow[e1] = 0.0;
        return;
    }
    const int z = (int)(v % A.nz), y = (int)((v / A.nz) % A.ny), x = (int)(v / ((int64_t)A.nz * A.ny));
    const int x0 = max(x - MET2_NESMA_HW, 0), x1 = min(x + MET2_NESMA_HW, A.nx);
    const int y0 = max(y - MET2_NESMA_HW, 0), y1 = min(y + MET2_NESMA_HW, A.ny);
    const int z0 = max(z - MET2_NESMA_HW, 0), z1 = min(z + MET2_NESMA_HW, A.nz);
    const int L = z1 - z0;                                     // 1..12 neighbours per batch
    const int q = lane >> 3, j = lane & 7;
    const double *crow = A.data + v * nt;
    const double c0 = has0 ? crow[e0] : 0.0, c1 = has1 ? crow[e1] : 0.0;
    if (has0 && writer) S[e0] = c0;
    if (has1) S[e1] = c1;
    __builtin_amdgcn_wave_barrier();
    NesmaTest T;
    T.init(bcast(np_rowsum_group(S, nt, j), 0));
    __builtin_amdgcn_wave_barrier();
    const double *S0 = S + min(q, L - 1) * SR, *S1 = S + min(8 + (q & 3), L - 1) * SR;
    const int64_t ystride = (int64_t)A.nz * nt, xstride = ystride * A.ny;
    unsigned off0[STEPS], off1[STEPS];                         // the lane's element of each row of a run
#pragma unroll
    for (int t = 0; t < STEPS; ++t) {
        const int r = min(PACK * t + h, L - 1);
        off0[t] = (unsigned)(r * nt + min(e0, nt - 1));
        off1[t] = (unsigned)(r * nt + min(e1, nt - 1));
    }
    u64 live0 = 0, live1 = 0;                                  // bit 8 r set for the rows a run has
    for (int r = 0; r < L; ++r) { if (r < 8) live0 |= 1ull << (8 * r); else live1 |= 1ull << (8 * (r - 8)); }
    double acc0 = 0.0, acc1 = 0.0;
    int cnt = 0;
    for (int i = x0; i < x1; ++i) {
        const double *strip = A.data + i * xstride + y0 * ystride + (int64_t)z0 * nt;
        for (int jj = y0; jj < y1; ++jj, strip += ystride) {
            // all loads of the run first (rows past the run re-read its last row; they are never summed), then the
            // |difference| rows into LDS
            double nb0[STEPS], nb1[STEPS];
#pragma unroll
            for (int t = 0; t < STEPS; ++t) {
                nb0[t] = strip[off0[t]];
                nb1[t] = NE > 1 ? strip[off1[t]] : 0.0;
            }
#pragma unroll
            for (int t = 0; t < STEPS; ++t) {
                const int r = PACK * t + h;
                if (has0) S[r * SR + e0] = fabs(nb0[t] - c0);
                if (NE > 1 && has1) S[r * SR + e1] = fabs(nb1[t] - c1);
            }
            __builtin_amdgcn_wave_barrier();
            const u64 ok0 = T.similar(np_rowsum_group(S0, nt, j));           // 8 identical bits per lane group
            const u64 ok1 = L > 8 ? T.similar(np_rowsum_group(S1, nt, j)) : 0ull;
            __builtin_amdgcn_wave_barrier();
            const u64 v0 = ok0 & live0, v1 = ok1 & live1;                    // bit 8 r: neighbour r (8 + r) of the run is similar
            cnt += __builtin_popcountll(v0) + __builtin_popcountll(v1);
#pragma unroll
            for (int t = 0; t < STEPS; ++t) {
                if (PACK == 1) {
                    if (((t < 8 ? v0 : v1) >> (8 * (t & 7))) & 1ull) { acc0 += nb0[t]; if (NE > 1) acc1 += nb1[t]; }
                } else {
                    const int ra = 2 * t, rb = 2 * t + 1;
                    if (((ra < 8 ? v0 : v1) >> (8 * (ra & 7))) & 1ull) acc0 += nb0[t];
                    if (((rb < 8 ? v0 : v1) >> (8 * (rb & 7))) & 1ull) acc0 += from_upper_half(nb0[t]);
                }
            }
        }
    }
    const double dc = (double)cnt;                             // empty set -> 0/0 = nan, as np.mean of nothing
    if (has0 && writer) orow[e0] = acc0 / dc;
    if (has1) orow[e1] = acc1 / dc;
}

// One echo (nt == 1): np.mean(rows[similar], axis=0) of an [n, 1] array is a contiguous reduction, which numpy sums pairwise (8 running
// sums on blocks of at most 128 values, longer vectors halved recursively) and not in window order as it does the rows of nt >= 2.
// numpy's pairwise sum of a[0..n), n <= 128
__device__ __forceinline__ double np_pairwise_block(const double *a, int n)
{
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    const int n8 = n - (n & 7);
    for (int i = 8; i < n8; i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = n8; i < n; ++i) res += a[i];
    return res;
}

// numpy's pairwise sum of a[0..n), n <= 12^3, on one lane: the recursion pw(a, n) = pw(a, n2) + pw(a + n2, n - n2), n2 = n / 2 rounded
// down to a multiple of 8, walked with an explicit stack (at most 5 levels: 1728 -> 871 -> 442 -> 228 -> 121)
__device__ double np_pairwise_serial(const double *a, int n)
{
    int off[8], len[8], stage[8], sp = 0;
    double left[8], ret = 0.0;
    off[0] = 0; len[0] = n; stage[0] = 0;
    while (sp >= 0) {
        if (len[sp] <= 128) { ret = np_pairwise_block(a + off[sp], len[sp]); --sp; continue; }
        int n2 = len[sp] / 2; n2 -= n2 % 8;
        if (stage[sp] == 0)      { stage[sp] = 1; off[sp + 1] = off[sp]; len[sp + 1] = n2; stage[sp + 1] = 0; ++sp; }
        else if (stage[sp] == 1) { stage[sp] = 2; left[sp] = ret; off[sp + 1] = off[sp] + n2; len[sp + 1] = len[sp] - n2; stage[sp + 1] = 0; ++sp; }
        else                     { ret = left[sp] + ret; --sp; }
    }
    return ret;
}

// One wave per voxel: the similar neighbours go into LDS in window order, lane 0 sums them as numpy does.  (A one-echo series has no
// decay to fit; the path is here so that the entry is the reference's filter at every echo count it accepts.)
__global__ __launch_bounds__(64) void nesma_one_echo_kernel(NesmaArgs A)
{
    __shared__ double sel[8 * MET2_NESMA_HW * MET2_NESMA_HW * MET2_NESMA_HW];
    const int lane = lane_id();
    const int64_t v = blockIdx.x;
    if (A.mask && A.mask[v] != 1) {                            // workgroup-uniform
        if (lane == 0) A.out[v] = 0.0;
        return;
    }
    const int z = (int)(v % A.nz), y = (int)((v / A.nz) % A.ny), x = (int)(v / ((int64_t)A.nz * A.ny));
    const int x0 = max(x - MET2_NESMA_HW, 0), x1 = min(x + MET2_NESMA_HW, A.nx);
    const int y0 = max(y - MET2_NESMA_HW, 0), y1 = min(y + MET2_NESMA_HW, A.ny);
    const int z0 = max(z - MET2_NESMA_HW, 0), z1 = min(z + MET2_NESMA_HW, A.nz);
    const int L = z1 - z0, wy = y1 - y0, n = (x1 - x0) * wy * L;          // n <= 12^3
    const double c = A.data[v], sumc = 0.0 + c;
    int cnt = 0;
    for (int b = 0; b < n; b += 64) {
        const int k = b + lane;
        bool ok = false;
        double nb = 0.0;
        if (k < n) {
            const int i = x0 + k / (wy * L), jj = y0 + (k / L) % wy, kk = z0 + k % L;
            nb = A.data[((int64_t)i * A.ny + jj) * A.nz + kk];
            ok = 100.0 * (0.0 + fabs(nb - c)) / sumc < 2.5;
        }
        const u64 m = ballot(ok);
        if (ok) sel[cnt + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = nb;
        cnt += __builtin_popcountll(m);
    }
    __syncthreads();
    if (lane == 0) A.out[v] = np_pairwise_serial(sel, cnt) / (double)cnt;    // empty set -> 0/0 = nan
}

// ------------------------------------------------------------------------------------------
// Gaussian pre-smoothing of the FA step (motor:337-343: scipy.ndimage.gaussian_filter(vol, 2.0) on every echo volume):
// one separable pass per axis over the whole [nx][ny][nz][nt] array (nt innermost: all echoes at once, coalesced for
// every axis), 'reflect' boundary, accumulation in the order of scipy's correlate1d for symmetric kernels (centre, then
// the pairs from the outermost inwards) with separate multiply and add roundings, so the result is bit-identical.
// ------------------------------------------------------------------------------------------
#define MET2_SMOOTH_MAX_RADIUS 32
struct SmoothArgs {
    int n, radius;
    int64_t stride, total;
    const double *src;
    double *dst;
    double w[2 * MET2_SMOOTH_MAX_RADIUS + 1];
};

__device__ __forceinline__ int reflect_index_dev(int i, int n)
{
    if (n == 1) return 0;
    const int period = 2 * n;
    i %= period; if (i < 0) i += period;
    return i < n ? i : period - 1 - i;
}

__global__ __launch_bounds__(256) void smooth_axis_kernel(SmoothArgs A)
{
#pragma clang fp contract(off)                                      // scipy's C loop rounds the product and the sum separately
    const int r = A.radius, n = A.n;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < A.total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)((idx / A.stride) % n);
        const double *base = A.src + (idx - (int64_t)i * A.stride);
        double t = A.src[idx] * A.w[r];
        if (i >= r && i + r < n) {                                  // interior: no reflection
            for (int j = -r; j < 0; ++j) {
                const double pr = (base[(int64_t)(i + j) * A.stride] + base[(int64_t)(i - j) * A.stride]) * A.w[j + r];
                t = t + pr;
            }
        } else {
            for (int j = -r; j < 0; ++j) {
                const double pr = (base[(int64_t)reflect_index_dev(i + j, n) * A.stride] + base[(int64_t)reflect_index_dev(i - j, n) * A.stride]) * A.w[j + r];
                t = t + pr;
            }
        }
        A.dst[idx] = t;
    }
}

// ------------------------------------------------------------------------------------------
// spline flip-angle selection (flip_angle_algorithms/fa_estimation.py:54-59): cubic (not-a-knot)
// interpolation of the coarse-grid NNLS residuals, bounded Brent over [90, 180] (scipy
// minimize_scalar(method='Bounded'): xatol 1e-5, maxiter 500), snap to the fine FA grid.
// One thread per voxel; the residuals come from fa_kernel on the coarse dictionary.
// ------------------------------------------------------------------------------------------
#define MET2_MAX_LR 32
struct SplineArgs {
    int nlr, nhr, nte;
    const double *alpha_lr;   // [nlr] device
    const double *W;          // [nlr][nlr] device: knot slopes = W y
    const double *alpha_hr;   // [nhr] device
    const double *resid;      // [nvox][nlr]
    const double *data;       // echo e of voxel v at data[v * vs + e * es]
    int64_t vs, es;
    const uint8_t *mask;
    double *fa_index, *xmin;
    int64_t nvox;
};

__device__ __forceinline__ double spline_eval_dev(int n, const double *x, const double *y, const double *s, double xx)
{
    int i = 0;
    while (i < n - 2 && xx >= x[i + 1]) ++i;
    const double h = x[i + 1] - x[i], t = (xx - x[i]) / h;
    const double h00 = (1.0 + 2.0 * t) * (1.0 - t) * (1.0 - t), h10 = t * (1.0 - t) * (1.0 - t);
    const double h01 = t * t * (3.0 - 2.0 * t), h11 = t * t * (t - 1.0);
    return h00 * y[i] + h10 * h * s[i] + h01 * y[i + 1] + h11 * h * s[i + 1];
}

__global__ __launch_bounds__(128) void fa_spline_kernel(SplineArgs A)
{
    __shared__ double sx[MET2_MAX_LR];
    for (int i = threadIdx.x; i < A.nlr; i += blockDim.x) sx[i] = A.alpha_lr[i];
    __syncthreads();
    const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (v >= A.nvox) return;
    double sum = 0.0;
    for (int e = 0; e < A.nte; ++e) sum += A.data[v * A.vs + e * A.es];
    const bool mk = A.mask ? (A.mask[v] != 0) : true;
    if (!(mk && sum > 0.0)) { A.fa_index[v] = 0.0; if (A.xmin) A.xmin[v] = 0.0; return; }
    double y[MET2_MAX_LR], s[MET2_MAX_LR];
    const int n = A.nlr;
    for (int i = 0; i < n; ++i) y[i] = A.resid[(size_t)v * n + i];
    for (int i = 0; i < n; ++i) {
        double t = 0.0;
        for (int j = 0; j < n; ++j) t = fma(A.W[i * n + j], y[j], t);
        s[i] = t;
    }
    int flag;
    const double xs = fminbound_dev<false>([&](double x) { return spline_eval_dev(n, sx, y, s, x); }, []() {}, 90.0, 180.0, 1e-5, 500, flag);
    int best = 0; double dbest = fabs(A.alpha_hr[0] - xs);            // np.argmin(|alpha - x|): first minimum
    for (int a = 1; a < A.nhr; ++a) { double d = fabs(A.alpha_hr[a] - xs); if (d < dbest) { dbest = d; best = a; } }
    A.fa_index[v] = (double)best;
    if (A.xmin) A.xmin[v] = xs;
}

// slope weights of the not-a-knot cubic spline: knot slopes = W y (the system depends on the knots only)
static void spline_weights_host(int n, const double *x, std::vector<double> &W)
{
    std::vector<double> A((size_t)n * n, 0.0), Rm((size_t)n * n, 0.0);   // A s = Rm y
    auto h = [&](int i) { return x[i + 1] - x[i]; };
    {   // not-a-knot at x[1]
        const double h0 = h(0), h1 = h(1);
        A[0] = h1; A[1] = h0 + h1;
        // rhs = ((3h0+2h1) h1 d0 + h0^2 d1)/(h0+h1), d0 = (y1-y0)/h0, d1 = (y2-y1)/h1
        const double c0 = (3.0 * h0 + 2.0 * h1) * h1 / (h0 + h1) / h0, c1 = h0 * h0 / (h0 + h1) / h1;
        Rm[0] += -c0; Rm[1] += c0 - c1; Rm[2] += c1;
    }
    for (int i = 1; i < n - 1; ++i) {
        const double hm = h(i - 1), hp = h(i);
        A[(size_t)i * n + i - 1] = hp; A[(size_t)i * n + i] = 2.0 * (hm + hp); A[(size_t)i * n + i + 1] = hm;
        const double cm = 3.0 * hp / hm, cp = 3.0 * hm / hp;               // rhs = 3 (hp dm + hm dp)
        Rm[(size_t)i * n + i - 1] += -cm; Rm[(size_t)i * n + i] += cm - cp; Rm[(size_t)i * n + i + 1] += cp;
    }
    {   // not-a-knot at x[n-2]
        const double ha = h(n - 3), hb = h(n - 2);
        A[(size_t)(n - 1) * n + n - 2] = ha + hb; A[(size_t)(n - 1) * n + n - 1] = ha;
        const double ca = hb * hb / (ha + hb) / ha, cb = (2.0 * ha + 3.0 * hb) * ha / (ha + hb) / hb;
        Rm[(size_t)(n - 1) * n + n - 3] += -ca; Rm[(size_t)(n - 1) * n + n - 2] += ca - cb; Rm[(size_t)(n - 1) * n + n - 1] += cb;
    }
    // W = A^-1 Rm by Gaussian elimination with partial pivoting on [A | Rm]
    for (int c = 0; c < n; ++c) {
        int p = c; double mx = fabs(A[(size_t)c * n + c]);
        for (int r = c + 1; r < n; ++r) if (fabs(A[(size_t)r * n + c]) > mx) { mx = fabs(A[(size_t)r * n + c]); p = r; }
        if (p != c) for (int j = 0; j < n; ++j) { std::swap(A[(size_t)c * n + j], A[(size_t)p * n + j]); std::swap(Rm[(size_t)c * n + j], Rm[(size_t)p * n + j]); }
        for (int r = c + 1; r < n; ++r) {
            const double l = A[(size_t)r * n + c] / A[(size_t)c * n + c];
            if (l == 0.0) continue;
            for (int j = c; j < n; ++j) A[(size_t)r * n + j] -= l * A[(size_t)c * n + j];
            for (int j = 0; j < n; ++j) Rm[(size_t)r * n + j] -= l * Rm[(size_t)c * n + j];
        }
    }
    W.assign((size_t)n * n, 0.0);
    for (int c = n - 1; c >= 0; --c)
        for (int j = 0; j < n; ++j) {
            double t = Rm[(size_t)c * n + j];
            for (int q = c + 1; q < n; ++q) t -= A[(size_t)c * n + q] * W[(size_t)q * n + j];
            W[(size_t)c * n + j] = t / A[(size_t)c * n + c];
        }
}

extern "C" int met2_smooth_separable(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t nt, int32_t radius, const double *weights,
                                     const double *data, double *out, double *work, void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0 || nt < 1) return fail(MET2_E_INVALID, "bad shape");
    if (radius < 0 || radius > MET2_SMOOTH_MAX_RADIUS) return fail(MET2_E_UNSUPPORTED, "kernel radius must be 0..32");
    const int64_t total = (int64_t)nx * ny * nz * nt;
    if (total == 0) return MET2_OK;
    if (!weights || !data || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (data == out || work == out || work == data) return fail(MET2_E_INVALID, "data, out and work must be distinct");
    USE_DEVICE(device);
    hipStream_t s = (hipStream_t)stream;
    DeviceWork W(s);                                                // the caller's work is neither waited for nor freed
    const auto piece = W.take<double>((size_t)total);
    if (!W.alloc(work)) return W.finish("met2_smooth_separable");
    double *tmp = piece;
    SmoothArgs A;
    A.radius = radius; A.total = total;
    for (int i = 0; i < 2 * radius + 1; ++i) A.w[i] = weights[i];
    const int dims[3] = {nx, ny, nz};
    const int64_t strides[3] = {(int64_t)ny * nz * nt, (int64_t)nz * nt, (int64_t)nt};
    const double *src = data;
    double *dst = out;                                              // x: data -> out, y: out -> work, z: work -> out
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 64);
    for (int ax = 0; ax < 3; ++ax) {
        A.n = dims[ax]; A.stride = strides[ax]; A.src = src; A.dst = dst;
        hipLaunchKernelGGL(smooth_axis_kernel, dim3(grid), dim3(256), 0, s, A);
        src = dst;
        dst = (dst == out) ? tmp : out;
    }
    return W.finish("met2_smooth_separable");
}

extern "C" int met2_nesma(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t nt, const double *data,
                          const uint8_t *mask, double *out, void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0 || nt < 1) return fail(MET2_E_INVALID, "bad shape");
    if (nt > MET2_NESMA_MAX_NT) return fail(MET2_E_UNSUPPORTED, "NESMA supports at most 128 echoes");
    const int64_t nvox = (int64_t)nx * ny * nz;
    if (nvox == 0) return MET2_OK;
    if (!data || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (data == out) return fail(MET2_E_INVALID, "NESMA cannot run in place");
    if ((nvox + 3) / 4 > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large for one launch");
    USE_DEVICE(device);
    hipStream_t s = (hipStream_t)stream;
    NesmaArgs A;
    A.nx = nx; A.ny = ny; A.nz = nz; A.nt = nt; A.data = data; A.mask = mask; A.out = out; A.nvox = nvox;
    const dim3 grid((unsigned)((((nvox + 3) / 4 + 7) / 8) * 8)), block(256);      // a multiple of 8 for the XCD remap
    A.srow = ((nt + 23) / 32) * 32 + 8;
    const size_t lds = sizeof(double) * 4 * 2 * MET2_NESMA_HW * (size_t)A.srow;
    if (nt == 1) {
        if (nvox > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large for one launch");
        hipLaunchKernelGGL(nesma_one_echo_kernel, dim3((unsigned)nvox), dim3(64), 0, s, A);
    }
    else if (nt == 32) hipLaunchKernelGGL((nesma_kernel<1, 2, 32>), grid, block, lds, s, A);
    else if (nt < 32)  hipLaunchKernelGGL((nesma_kernel<1, 2, 0>), grid, block, lds, s, A);
    else if (nt == 48) hipLaunchKernelGGL((nesma_kernel<1, 1, 48>), grid, block, lds, s, A);
    else if (nt <= 64) hipLaunchKernelGGL((nesma_kernel<1, 1, 0>), grid, block, lds, s, A);
    else               hipLaunchKernelGGL((nesma_kernel<2, 1, 0>), grid, block, lds, s, A);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

struct SplineTables { int device = -1; double *d = nullptr; size_t cap = 0; std::vector<double> last; };
static thread_local SplineTables g_spline_tables;
// for host threads that end (met2_fit_host's per-plan threads): frees the calling thread's tables
void met2::spline_tables_release()
{
    SplineTables &T = g_spline_tables;
    if (T.d) { DevGuard g(T.device); (void)hipDeviceSynchronize(); (void)hipFree(T.d); }
    T.d = nullptr; T.cap = 0; T.device = -1; T.last.clear();
}

extern "C" int met2_fa_spline_select_strided(int32_t device, int64_t nvox, int32_t n_lr, const double *alpha_lr, const double *resid,
                                             int32_t n_hr, const double *alpha_hr, int32_t n_te, const double *data, int64_t voxel_stride,
                                             int64_t echo_stride, const uint8_t *mask, double *fa_index, double *xmin, void *stream)
{
    if (nvox == 0) return MET2_OK;
    if (!alpha_lr || !resid || !alpha_hr || !data || !fa_index) return fail(MET2_E_INVALID, "NULL argument");
    if (n_lr < 4 || n_lr > MET2_MAX_LR) return fail(MET2_E_UNSUPPORTED, "coarse FA grid must have 4..32 points");
    if (n_hr < 1 || n_te < 1) return fail(MET2_E_INVALID, "bad shape");
    for (int i = 1; i < n_lr; ++i) if (!(alpha_lr[i] > alpha_lr[i - 1])) return fail(MET2_E_INVALID, "coarse FA grid must increase");
    if (nvox <= 0) return MET2_OK;
    USE_DEVICE(device);
    hipStream_t s = (hipStream_t)stream;
    std::vector<double> W;
    spline_weights_host(n_lr, alpha_lr, W);
    const size_t nd = (size_t)n_lr + (size_t)n_lr * n_lr + (size_t)n_hr;
    std::vector<double> hb(nd);
    memcpy(hb.data(), alpha_lr, sizeof(double) * n_lr);
    memcpy(hb.data() + n_lr, W.data(), sizeof(double) * n_lr * n_lr);
    memcpy(hb.data() + n_lr + (size_t)n_lr * n_lr, alpha_hr, sizeof(double) * n_hr);
    // The tables (two grids and the spline's weight matrix, a few KB) live in a per-thread device buffer that is written only when they
    // CHANGE: a driver calls this once per chunk with the same grids, and an allocation + blocking wait + hipFree per call stood in the
    // way of its pipeline (hipFree waits for the whole device).  Changing them waits for the device first (a kernel of an earlier call may
    // still read the old ones).
    SplineTables &T = g_spline_tables;
    if (T.device != device || T.cap < nd) {
        if (T.d) { DevGuard old(T.device); HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(T.d)); T.d = nullptr; T.cap = 0; T.last.clear(); }
        HIPCHK(hipMalloc((void **)&T.d, sizeof(double) * std::max<size_t>(nd, 2048)));
        T.cap = std::max<size_t>(nd, 2048); T.device = device;
    }
    if (T.last != hb) {
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(T.d, hb.data(), sizeof(double) * nd, hipMemcpyHostToDevice));
        T.last = hb;
    }
    double *dbuf = T.d;
    SplineArgs A;
    A.nlr = n_lr; A.nhr = n_hr; A.nte = n_te;
    A.alpha_lr = dbuf; A.W = dbuf + n_lr; A.alpha_hr = dbuf + n_lr + (size_t)n_lr * n_lr;
    A.resid = resid; A.data = data; A.vs = voxel_stride; A.es = echo_stride; A.mask = mask; A.fa_index = fa_index; A.xmin = xmin; A.nvox = nvox;
    hipLaunchKernelGGL(fa_spline_kernel, dim3((unsigned)((nvox + 127) / 128)), dim3(128), 0, s, A);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_fa_spline_select(int32_t device, int64_t nvox, int32_t n_lr, const double *alpha_lr, const double *resid,
                                     int32_t n_hr, const double *alpha_hr, int32_t n_te, const double *data, const uint8_t *mask,
                                     double *fa_index, double *xmin, void *stream)
{
    return met2_fa_spline_select_strided(device, nvox, n_lr, alpha_lr, resid, n_hr, alpha_hr, n_te, data, n_te, 1, mask, fa_index, xmin, stream);
}
