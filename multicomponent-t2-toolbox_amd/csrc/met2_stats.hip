// met2_stats.hip -- met2_label_stats and its stages: per-label (tissue class, atlas ROI) statistics of maps and spectra.
//
// include/met2_hip.h states the contract.  The stages and their kernels:
//   met2_label_index      the member list, a counting sort of the voxels by label that keeps the voxel order inside a label:
//                         label_index_kernel<false> (per-block label counts, one wave per block of voxels), label_scan_blocks_kernel and
//                         label_scan_labels_kernel (the two exclusive scans), label_index_kernel<true> (the scatter, ranks inside a wave by
//                         ballot).  Integer arithmetic only, so the list does not depend on timing.
//   met2_label_moments    n, mean, std (ddof 1, around the mean): label_moment_kernel<0|1> sums chunks of MET2_STATS_CHUNK members of a label
//                         (a tile of 8 series at a time, staged through LDS so that series-major and voxel-major input are both read along
//                         their contiguous axis; per thread a chain of CHUNK / 256 = 64 additions, then a fixed tree over the 256 threads),
//                         label_moment_combine_kernel<0|1> adds the chunks of a (label, series) in a fixed order (a chain of at most 512
//                         per thread up to 2^31 members, then the same tree).  No floating-point atomics.
//   met2_label_quantiles  label_key_kernel gathers a tile of series into the dense key matrix [series][member position] (sortable 64-bit
//                         keys); labels of at most MET2_STATS_SMALL_N members are sorted in LDS (label_small_kernel, one workgroup per
//                         (label, series)) and go through quantile_sorted; the others by most-significant-digit radix selection, eight
//                         levels of label_select_hist_kernel (256-bin integer histograms in LDS per distinct prefix of the segment's
//                         ranks, flushed with integer atomics) and label_select_step_kernel (per rank: the bucket it falls in and the
//                         rank inside it), then label_select_finish_kernel (quantile_lerp on the two selected order statistics).
//                         The launches per tile are a constant; nothing returns to the host between them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_helpers.hpp"
#include "device_work.hpp"
#include "quantile.hpp"

namespace {

#define STATS_CHUNK MET2_STATS_CHUNK
#define STATS_SMALL_N MET2_STATS_SMALL_N
#define STATS_MAX_Q MET2_STATS_MAX_Q
#define STATS_MAX_R (2 * MET2_STATS_MAX_Q)      // ranks per segment: two order statistics per probability
#define STATS_TS 8                              // series per tile of the moment and key kernels
#define STATS_IDX_BLOCKS 1024                   // blocks of voxels of the counting sort, at most
#define STATS_KEY_BYTES ((size_t)256 << 20)     // the key matrix of a tile of series stays under this (one series at least)
#define STATS_HIST_BYTES ((size_t)64 << 20)     // and its global histograms under this

// ---------------------------------------------------------------------------------------------------------------- member list

// One wave per block of `per` consecutive voxels.  SCATTER = false: cnt[block][label] = the block's members per label.  SCATTER = true: cnt
// holds the exclusive prefix over the blocks before this one, offset[label] the label's start, and the block writes its members' voxel
// indices: tile after tile of 64 voxels, inside a tile the rank of a lane among the lanes of its label by ballot.
template <bool SCATTER>
__global__ __launch_bounds__(64) void label_index_kernel(int64_t nvox, int64_t per, const int32_t *__restrict__ label, int n_label, int32_t *cnt,
                                                         const int32_t *__restrict__ offset, int32_t *__restrict__ order)
{
    extern __shared__ int32_t run[];                           // [n_label] the next free slot (SCATTER) or the count so far
    const int lane = threadIdx.x;
    int32_t *my = cnt + (size_t)blockIdx.x * n_label;
    for (int i = lane; i < n_label; i += 64) run[i] = SCATTER ? my[i] + offset[i] : 0;
    wave_lds_sync();
    const int64_t v0 = (int64_t)blockIdx.x * per, v1 = std::min<int64_t>(nvox, v0 + per);
    for (int64_t base = v0; base < v1; base += 64) {
        const int64_t v = base + lane;
        int l = -1;
        if (v < v1) {
            l = label[v];
            if (l < 0 || l >= n_label) l = -1;
        }
        bool todo = l >= 0;
        for (;;) {                                             // one turn per distinct label of the tile
            const unsigned long long act = __ballot(todo);
            if (!act) break;
            const int leader = __ffsll(act) - 1;
            const int ll = __shfl(l, leader);
            const bool mine = todo && l == ll;
            const unsigned long long same = __ballot(mine);
            if (mine) {
                if (SCATTER) order[run[ll] + __popcll(same & ((1ull << lane) - 1ull))] = (int32_t)v;
                todo = false;
            }
            wave_lds_sync();
            if (lane == leader) run[ll] += __popcll(same);
            wave_lds_sync();
        }
    }
    if (!SCATTER) {
        wave_lds_sync();
        for (int i = lane; i < n_label; i += 64) my[i] = run[i];
    }
}

// per label: counts per block -> their exclusive prefix over the blocks, and the label's total
__global__ __launch_bounds__(256) void label_scan_blocks_kernel(int nblocks, int n_label, int32_t *cnt, int32_t *__restrict__ total)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_label) return;
    int32_t acc = 0;
    for (int b = 0; b < nblocks; ++b) {
        const int32_t t = cnt[(size_t)b * n_label + l];
        cnt[(size_t)b * n_label + l] = acc;
        acc += t;
    }
    total[l] = acc;
}

// one workgroup: offset[0 .. n_label] = the exclusive scan of total
__global__ __launch_bounds__(256) void label_scan_labels_kernel(int n_label, const int32_t *__restrict__ total, int32_t *__restrict__ offset)
{
    __shared__ int32_t part[257];
    const int tid = threadIdx.x, per = (n_label + 255) / 256;
    const int a = std::min(tid * per, n_label), b = std::min(a + per, n_label);
    int32_t s = 0;
    for (int i = a; i < b; ++i) s += total[i];
    part[tid + 1] = s;
    __syncthreads();
    if (tid == 0) {
        part[0] = 0;
        for (int i = 1; i <= 256; ++i) part[i] += part[i - 1];
    }
    __syncthreads();
    s = part[tid];
    for (int i = a; i < b; ++i) { offset[i] = s; s += total[i]; }
    if (tid == 255) offset[n_label] = part[256];
}

// ---------------------------------------------------------------------------------------------------------------- shared pieces

// sum over the 256 threads of a workgroup in a fixed order: xor tree inside a wave, then the four waves in turn (not device_helpers.hpp's
// block_sum, which adds the waves in pairs: other bits).  Every thread gets the sum.
__device__ __forceinline__ double block_sum_chain(double x, double *red4, int tid)
{
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    __syncthreads();                                           // red4 may still be read from the call before
    if ((tid & 63) == 0) red4[tid >> 6] = x;
    __syncthreads();
    return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

__device__ __forceinline__ long long block_sum_int(long long x, long long *red4, int tid)
{
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    __syncthreads();
    if ((tid & 63) == 0) red4[tid >> 6] = x;
    __syncthreads();
    return red4[0] + red4[1] + red4[2] + red4[3];
}

struct TileSrc {
    const int32_t *order;           // the member list
    const double *values;
    int64_t vs, ss;                 // strides of a voxel and of a series, in doubles
    int series_fast;                // ss < vs: the lanes of a load run along the series axis
};

// Tile element i of 8 x 256 (series x members) in the order the lanes load it: along the contiguous axis of the input.
__device__ __forceinline__ void tile_coords(int i, int series_fast, int &s, int &m)
{
    if (series_fast) { s = i & (STATS_TS - 1); m = i >> 3; }
    else { m = i & 255; s = i >> 8; }
}

// ---------------------------------------------------------------------------------------------------------------- moments

struct MomArgs {
    TileSrc src;
    const int32_t *chunk_label, *chunk_begin, *chunk_len;     // per chunk: its label, its first position in the member list, its members
    int n_series;
    double *part;                   // [nchunks][n_series] partial sums
    int32_t *part_n;                // [nchunks][n_series] values that are not NaN (PASS 0)
    const double *out;              // PASS 1 reads the means
    int64_t out_stride;             // doubles between two (label, series) records of out
};

// PASS 0: sum and count of the values that are not NaN; PASS 1: sum of the squared distances to the mean.  Workgroup = (chunk, 8 series).
template <int PASS>
__global__ __launch_bounds__(256) void label_moment_kernel(MomArgs A)
{
    __shared__ double tile[STATS_TS][257];
    __shared__ double red4[4];
    __shared__ long long red4i[4];
    const int tid = threadIdx.x, c = blockIdx.x, s0 = blockIdx.y * STATS_TS, ns = std::min(STATS_TS, A.n_series - s0);
    const int l = A.chunk_label[c], begin = A.chunk_begin[c], len = A.chunk_len[c];
    double acc[STATS_TS], mu[STATS_TS];
    int cnt[STATS_TS];
#pragma unroll
    for (int s = 0; s < STATS_TS; ++s) {
        acc[s] = 0.0;
        cnt[s] = 0;
        mu[s] = (PASS == 1 && s < ns) ? A.out[((int64_t)l * A.n_series + s0 + s) * A.out_stride + 1] : 0.0;
    }
    for (int m0 = 0; m0 < len; m0 += 256) {
        for (int i = tid; i < STATS_TS * 256; i += 256) {
            int s, m;
            tile_coords(i, A.src.series_fast, s, m);
            double x = __builtin_nan("");
            if (s < ns && m0 + m < len) x = A.src.values[(int64_t)A.src.order[begin + m0 + m] * A.src.vs + (int64_t)(s0 + s) * A.src.ss];
            tile[s][m] = x;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < STATS_TS; ++s) {
            const double x = tile[s][tid];
            if (x == x) {
                if (PASS == 0) { acc[s] += x; ++cnt[s]; }
                else { const double d = x - mu[s]; acc[s] += d * d; }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < STATS_TS; ++s) {
        const double t = block_sum_chain(acc[s], red4, tid);
        long long n = 0;
        if (PASS == 0) n = block_sum_int(cnt[s], red4i, tid);
        if (tid == 0 && s < ns) {
            A.part[(int64_t)c * A.n_series + s0 + s] = t;
            if (PASS == 0) A.part_n[(int64_t)c * A.n_series + s0 + s] = (int32_t)n;
        }
    }
}

struct CombArgs {
    const int32_t *label_chunk0, *label_nchunks;
    int n_series;
    const double *part;
    const int32_t *part_n;
    double *out;
    int64_t out_stride;
};

// workgroup = (label, series): the chunks' partial sums, thread t the chunks t, t + 256, ..., then the tree.
// PASS 0 -> n, mean; PASS 1 -> std.  A sample without a value gets n = 0 and NaN.
template <int PASS>
__global__ __launch_bounds__(256) void label_moment_combine_kernel(CombArgs A)
{
    __shared__ double red4[4];
    __shared__ long long red4i[4];
    const int tid = threadIdx.x, l = blockIdx.x, s = blockIdx.y;
    const int c0 = A.label_chunk0[l], nc = A.label_nchunks[l];
    double acc = 0.0;
    long long n = 0;
    for (int c = tid; c < nc; c += 256) {
        acc += A.part[(int64_t)(c0 + c) * A.n_series + s];
        if (PASS == 0) n += A.part_n[(int64_t)(c0 + c) * A.n_series + s];
    }
    acc = block_sum_chain(acc, red4, tid);
    double *o = A.out + ((int64_t)l * A.n_series + s) * A.out_stride;
    if (PASS == 0) {
        n = block_sum_int(n, red4i, tid);
        if (tid == 0) {
            o[0] = (double)n;
            o[1] = n > 0 ? acc / (double)n : __builtin_nan("");
        }
    } else if (tid == 0) {
        const double nn = o[0];
        o[2] = nn > 1.0 ? sqrt(acc / (nn - 1.0)) : (nn == 1.0 ? 0.0 : __builtin_nan(""));
    }
}

// ---------------------------------------------------------------------------------------------------------------- quantiles

// sortable key of a double: ascending keys = ascending values, -0.0 is +0.0, every NaN the largest key
// (not sort_key of met2_bet.hip, which keeps -0.0 apart and gives NaN no place, or tv_key of met2_tv.hip, which orders magnitudes)
__device__ __forceinline__ uint64_t to_key(double x)
{
    if (x != x) return ~0ull;
    uint64_t b = (uint64_t)__double_as_longlong(x);
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double from_key(uint64_t k)
{
    const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// keys[s][p] of the tile's series s0 .. s0 + ns - 1 and every member position p.  Workgroup = (256 positions, 8 series), through LDS so that
// the loads run along the input's contiguous axis and the stores along p.
__global__ __launch_bounds__(256) void label_key_kernel(TileSrc src, int64_t M, int s0, int ns, uint64_t *__restrict__ keys)
{
    __shared__ uint64_t tile[STATS_TS][257];
    const int tid = threadIdx.x, sb = blockIdx.y * STATS_TS, nsb = std::min(STATS_TS, ns - sb);
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    for (int i = tid; i < STATS_TS * 256; i += 256) {
        int s, m;
        tile_coords(i, src.series_fast, s, m);
        if (s < nsb && p0 + m < M) tile[s][m] = to_key(src.values[(int64_t)src.order[p0 + m] * src.vs + (int64_t)(s0 + sb + s) * src.ss]);
    }
    __syncthreads();
    if (p0 + tid < M)
        for (int s = 0; s < nsb; ++s) keys[(int64_t)(sb + s) * M + p0 + tid] = tile[s][tid];
}

struct QArgs {
    const uint64_t *keys;           // [ns][M]
    int64_t M;
    const int32_t *offset;          // [n_label + 1]
    int n_label, ns, s0, n_series;  // the tile's series are s0 .. s0 + ns - 1 of n_series
    int n_q, R;                     // R = 2 n_q ranks per segment; segment = s * n_label + label
    const double *q;                // [n_q] on the device
    double *out;
    int64_t out_stride;
    int out_col;                    // the quantiles start at this column of a record
    // radix selection
    const int32_t *chunk_label, *chunk_begin, *chunk_len;     // the chunks of the labels above SMALL_N members
    int level;
    uint32_t *ghist;                // [nseg][R][256]
    int32_t *nan_count;             // [nseg]
    const uint64_t *prefix_in;      // [nseg][R] the leading `level` digits of every rank's key
    uint64_t *prefix_out;
    uint32_t *krank;                // [nseg][R] the rank among the keys that share the prefix
};


// labels of at most SMALL_N members: workgroup = (label, series), bitonic sort of the keys in LDS, then quantile_sorted
__global__ __launch_bounds__(256) void label_small_kernel(QArgs A)
{
    __shared__ uint64_t buf[STATS_SMALL_N];
    __shared__ int nan_s;
    const int tid = threadIdx.x, l = blockIdx.x, s = blockIdx.y;
    const int begin = A.offset[l], len = A.offset[l + 1] - begin;
    if (len > STATS_SMALL_N) return;
    double *o = A.out + ((int64_t)l * A.n_series + A.s0 + s) * A.out_stride + A.out_col;
    if (tid == 0) nan_s = 0;
    __syncthreads();
    const int P = next_pow2(len);
    const uint64_t *k = A.keys + (int64_t)s * A.M + begin;
    int nan = 0;
    for (int i = tid; i < P; i += 256) {
        const uint64_t key = i < len ? k[i] : ~0ull;
        nan += (i < len && key == ~0ull);
        buf[i] = key;
    }
    if (nan) atomicAdd(&nan_s, nan);
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int p = i ^ j;
                if (p > i) {
                    const uint64_t x = buf[i], y = buf[p];
                    if ((i & kk) == 0 ? x > y : y > x) { buf[i] = y; buf[p] = x; }
                }
            }
            __syncthreads();
        }
    const int n = len - nan_s;
    double *sorted = reinterpret_cast<double *>(buf);
    for (int i = tid; i < n; i += 256) sorted[i] = from_key(buf[i]);        // in place: slot i is read and written by one thread
    __syncthreads();
    for (int j = tid; j < A.n_q; j += 256) o[j] = n > 0 ? met2::quantile_sorted(sorted, n, A.q[j]) : __builtin_nan("");
}

// +1 in bin `digit` of h for every active lane; the lanes that share the first active lane's digit add once (long tie runs -- the exact zeros
// of a myelin water fraction -- put a whole wave into one bin)
__device__ __forceinline__ void hist_add(uint32_t *h, int digit, bool active, int lane)
{
    const unsigned long long act = __ballot(active);
    if (!act) return;
    const int leader = __ffsll(act) - 1;
    const int d0 = __shfl(digit, leader);
    const unsigned long long same = __ballot(active && digit == d0);
    if (active) {
        if (digit != d0) atomicAdd(&h[digit], 1u);
        else if (lane == leader) atomicAdd(&h[d0], (uint32_t)__popcll(same));
    }
}

// One digit level of the selection: workgroup = (chunk of a label, series).  The segment's ranks carry the leading digits found so far;
// each run of equal prefixes among them (its first rank the run's leader) gets one 256-bin histogram of the next digit over the keys
// that share the prefix.  Level 0 has the empty prefix and one histogram, and counts the NaN keys.
__global__ __launch_bounds__(256) void label_select_hist_kernel(QArgs A)
{
    __shared__ uint32_t hist[STATS_MAX_R * 256];
    __shared__ uint64_t pre[STATS_MAX_R];
    __shared__ int lead[STATS_MAX_R];
    __shared__ int nd_s, nan_s;
    const int tid = threadIdx.x, lane = tid & 63, c = blockIdx.x, s = blockIdx.y;
    const int l = A.chunk_label[c], begin = A.chunk_begin[c], len = A.chunk_len[c];
    const int64_t seg = (int64_t)s * A.n_label + l;
    if (tid == 0) {
        int nd = 0;
        if (A.level == 0) { lead[0] = 0; pre[0] = 0; nd = 1; }
        else {
            const uint64_t *p = A.prefix_in + seg * A.R;
            for (int r = 0; r < A.R; ++r)
                if (r == 0 || p[r] != p[r - 1]) { lead[nd] = r; pre[nd] = p[r]; ++nd; }
        }
        nd_s = nd;
        nan_s = 0;
    }
    __syncthreads();
    const int nd = nd_s;
    for (int i = tid; i < nd * 256; i += 256) hist[i] = 0;
    __syncthreads();
    const uint64_t *k = A.keys + (int64_t)s * A.M + begin;
    const int dshift = 56 - 8 * A.level, pshift = 64 - 8 * A.level;
    int nan = 0;
    for (int i0 = 0; i0 < len; i0 += 256) {                    // the whole wave walks together: hist_add ballots
        const int i = i0 + tid;
        const bool valid = i < len;
        const uint64_t key = valid ? k[i] : 0;
        const int digit = (int)((key >> dshift) & 255);
        if (A.level == 0) {
            nan += (valid && key == ~0ull);
            hist_add(hist, digit, valid, lane);
        } else {
            const uint64_t hi = key >> pshift;
            for (int d = 0; d < nd; ++d) hist_add(hist + d * 256, digit, valid && hi == pre[d], lane);
        }
    }
    if (A.level == 0 && nan) atomicAdd(&nan_s, nan);
    __syncthreads();
    for (int i = tid; i < nd * 256; i += 256) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(&A.ghist[(seg * A.R + lead[i >> 8]) * 256 + (i & 255)], v);
    }
    if (A.level == 0 && tid == 0 && nan_s) atomicAdd(&A.nan_count[seg], nan_s);
}

// The bookkeeping between two levels, a thread per (segment, rank): from the histogram of the rank's run, the bucket the rank falls in and
// the rank inside that bucket.  Level 0 first turns the probabilities into ranks (n = members - NaN keys).
__global__ __launch_bounds__(256) void label_select_step_kernel(QArgs A)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)A.ns * A.n_label * A.R) return;
    const int64_t seg = idx / A.R;
    const int r = (int)(idx - seg * A.R), l = (int)(seg % A.n_label);
    const int len = A.offset[l + 1] - A.offset[l];
    if (len <= STATS_SMALL_N) return;
    uint32_t k = 0;
    uint64_t p = 0;
    int ld = 0;
    if (A.level == 0) {
        const int n = len - A.nan_count[seg];
        if (n > 0) {
            int i0, i1;
            double g;
            met2::quantile_position(n, A.q[r >> 1], i0, i1, g);
            k = (uint32_t)((r & 1) ? i1 : i0);
        }
    } else {
        k = A.krank[idx];
        p = A.prefix_in[idx];
        ld = r;
        while (ld > 0 && A.prefix_in[seg * A.R + ld - 1] == p) --ld;
    }
    const uint32_t *h = A.ghist + (seg * A.R + ld) * 256;
    uint32_t cum = 0;
    int b = 0;
    for (; b < 255; ++b) {
        const uint32_t cb = h[b];
        if (cum + cb > k) break;
        cum += cb;
    }
    A.prefix_out[idx] = (p << 8) | (uint64_t)b;
    A.krank[idx] = k - cum;
}

// after eight levels a rank's prefix is its key: thread per (segment, probability), numpy's lerp between the two order statistics
__global__ __launch_bounds__(256) void label_select_finish_kernel(QArgs A)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)A.ns * A.n_label * A.n_q) return;
    const int64_t seg = idx / A.n_q;
    const int j = (int)(idx - seg * A.n_q), l = (int)(seg % A.n_label), s = (int)(seg / A.n_label);
    const int len = A.offset[l + 1] - A.offset[l];
    if (len <= STATS_SMALL_N) return;
    const int n = len - A.nan_count[seg];
    double v = __builtin_nan("");
    if (n > 0) {
        int i0, i1;
        double g;
        met2::quantile_position(n, A.q[j], i0, i1, g);
        v = met2::quantile_lerp(from_key(A.prefix_in[seg * A.R + 2 * j]), from_key(A.prefix_in[seg * A.R + 2 * j + 1]), g);
    }
    A.out[((int64_t)l * A.n_series + A.s0 + s) * A.out_stride + A.out_col + j] = v;
}

// ---------------------------------------------------------------------------------------------------------------- host side

// h into its piece d of the work space W
template <class T> bool upload(DeviceWork &W, void *d, const std::vector<T> &h, hipStream_t s)
{
    if (!h.empty()) W.ok(hipMemcpyAsync(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, s));
    return W.ok(hipStreamSynchronize(s));                      // h may go away behind the call
}

int common_checks(int32_t n_label, int32_t n_series, const double *values, int64_t voxel_stride, int64_t series_stride)
{
    if (n_label < 1 || n_series < 1) return fail(MET2_E_INVALID, "n_label and n_series must be positive");
    if (voxel_stride <= 0 || series_stride <= 0) return fail(MET2_E_INVALID, "strides must be positive");
    if (!values) return fail(MET2_E_INVALID, "NULL argument");
    if (n_label > MET2_STATS_MAX_LABEL) return fail(MET2_E_UNSUPPORTED, "more labels than MET2_STATS_MAX_LABEL");
    if (n_series > MET2_STATS_MAX_SERIES) return fail(MET2_E_UNSUPPORTED, "more series than MET2_STATS_MAX_SERIES");
    return MET2_OK;
}

int q_checks(int32_t n_q, const double *q_host, int min_q)
{
    if (n_q < min_q) return fail(MET2_E_INVALID, "n_q too small");
    if (n_q > 0 && !q_host) return fail(MET2_E_INVALID, "NULL argument");
    if (n_q > MET2_STATS_MAX_Q) return fail(MET2_E_UNSUPPORTED, "more probabilities than MET2_STATS_MAX_Q");
    for (int j = 0; j < n_q; ++j)
        if (!(q_host[j] >= 0.0 && q_host[j] <= 1.0)) return fail(MET2_E_INVALID, "a probability must lie in [0, 1]");
    return MET2_OK;
}

// the offsets on the host, checked: 0 = offset[0] <= offset[1] <= ...
int fetch_offsets(const int32_t *offset, int n_label, std::vector<int32_t> &h, hipStream_t s)
{
    h.resize((size_t)n_label + 1);
    HIPCHK(hipMemcpyAsync(h.data(), offset, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h[0] != 0) return fail(MET2_E_INVALID, "offset[0] must be 0");
    for (int l = 0; l < n_label; ++l)
        if (h[l + 1] < h[l]) return fail(MET2_E_INVALID, "offset must not decrease");
    return MET2_OK;
}

// the chunks of at most CHUNK members of the labels with more than `above` members
struct Chunks {
    std::vector<int32_t> label, begin, len, chunk0, nchunks;
    void build(const std::vector<int32_t> &off, int n_label, int above)
    {
        chunk0.assign(n_label, 0);
        nchunks.assign(n_label, 0);
        for (int l = 0; l < n_label; ++l) {
            const int32_t n = off[l + 1] - off[l];
            chunk0[l] = (int32_t)label.size();
            if (n <= above) continue;
            for (int32_t a = 0; a < n; a += STATS_CHUNK) {
                label.push_back(l);
                begin.push_back(off[l] + a);
                len.push_back(std::min<int32_t>(STATS_CHUNK, n - a));
            }
            nchunks[l] = (int32_t)label.size() - chunk0[l];
        }
    }
};

int index_impl(int64_t nvox, const int32_t *label, int n_label, int32_t *offset, int32_t *order, hipStream_t s)
{
    const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(STATS_IDX_BLOCKS, (nvox + 1023) / 1024));
    const int64_t per = ((std::max<int64_t>(nvox, 1) + nb - 1) / nb + 63) / 64 * 64;
    const int nblocks = (int)std::max<int64_t>(1, (nvox + per - 1) / per);
    const char *who = "met2_label_index";
    DeviceWork W(s);
    const auto cnt = W.take<int32_t>((size_t)nblocks * n_label), total = W.take<int32_t>(n_label);
    if (!W.alloc()) return W.finish(who);
    const size_t lds = sizeof(int32_t) * (size_t)n_label;
    hipLaunchKernelGGL(label_index_kernel<false>, dim3(nblocks), dim3(64), lds, s, nvox, per, label, n_label, cnt, (const int32_t *)nullptr,
                       (int32_t *)nullptr);
    if (!W.ok(hipGetLastError())) return W.finish(who);
    hipLaunchKernelGGL(label_scan_blocks_kernel, dim3((n_label + 255) / 256), dim3(256), 0, s, nblocks, n_label, cnt, total);
    if (!W.ok(hipGetLastError())) return W.finish(who);
    hipLaunchKernelGGL(label_scan_labels_kernel, dim3(1), dim3(256), 0, s, n_label, (const int32_t *)total, offset);
    if (!W.ok(hipGetLastError())) return W.finish(who);
    hipLaunchKernelGGL(label_index_kernel<true>, dim3(nblocks), dim3(64), lds, s, nvox, per, label, n_label, cnt, (const int32_t *)offset, order);
    return W.finish(who);
}

TileSrc tile_src(const int32_t *order, const double *values, int64_t vs, int64_t ss)
{
    TileSrc t;
    t.order = order; t.values = values; t.vs = vs; t.ss = ss; t.series_fast = ss < vs;
    return t;
}

int moments_impl(const std::vector<int32_t> &off, int n_label, const int32_t *order, int n_series, const double *values, int64_t vs, int64_t ss,
                 double *out, int64_t out_stride, hipStream_t s)
{
    Chunks ch;
    ch.build(off, n_label, 0);
    const size_t nch = ch.label.size();
    const char *who = "met2_label_moments";
    DeviceWork W(s);
    const auto d_label = W.take<int32_t>(nch), d_begin = W.take<int32_t>(nch), d_len = W.take<int32_t>(nch);
    const auto d_c0 = W.take<int32_t>(n_label), d_nc = W.take<int32_t>(n_label);
    const auto part = W.take<double>(nch * n_series);
    const auto part_n = W.take<int32_t>(nch * n_series);
    if (!W.alloc()) return W.finish(who);
    if (!upload(W, d_label, ch.label, s) || !upload(W, d_begin, ch.begin, s) || !upload(W, d_len, ch.len, s) || !upload(W, d_c0, ch.chunk0, s) ||
        !upload(W, d_nc, ch.nchunks, s))
        return W.finish(who);
    MomArgs M;
    M.src = tile_src(order, values, vs, ss);
    M.chunk_label = d_label; M.chunk_begin = d_begin; M.chunk_len = d_len;
    M.n_series = n_series; M.part = part; M.part_n = part_n; M.out = out; M.out_stride = out_stride;
    CombArgs Cb;
    Cb.label_chunk0 = d_c0; Cb.label_nchunks = d_nc; Cb.n_series = n_series; Cb.part = part;
    Cb.part_n = part_n; Cb.out = out; Cb.out_stride = out_stride;
    const dim3 gm((unsigned)nch, (unsigned)((n_series + STATS_TS - 1) / STATS_TS)), gc((unsigned)n_label, (unsigned)n_series);
    if (nch) {
        hipLaunchKernelGGL(label_moment_kernel<0>, gm, dim3(256), 0, s, M);
        if (!W.ok(hipGetLastError())) return W.finish(who);
    }
    hipLaunchKernelGGL(label_moment_combine_kernel<0>, gc, dim3(256), 0, s, Cb);
    if (!W.ok(hipGetLastError())) return W.finish(who);
    if (nch) {
        hipLaunchKernelGGL(label_moment_kernel<1>, gm, dim3(256), 0, s, M);
        if (!W.ok(hipGetLastError())) return W.finish(who);
    }
    hipLaunchKernelGGL(label_moment_combine_kernel<1>, gc, dim3(256), 0, s, Cb);
    return W.finish(who);
}

int quantiles_impl(const std::vector<int32_t> &off, int n_label, const int32_t *offset, const int32_t *order, int n_series, const double *values,
                   int64_t vs, int64_t ss, int n_q, const double *q_host, double *out, int64_t out_stride, int out_col, hipStream_t s)
{
    const int64_t M = off[n_label];
    const int R = 2 * n_q;
    Chunks ch;
    ch.build(off, n_label, STATS_SMALL_N);
    const size_t nch = ch.label.size();
    bool any_small = false;
    for (int l = 0; l < n_label; ++l) any_small = any_small || off[l + 1] - off[l] <= STATS_SMALL_N;
    // series per tile: the key matrix and the histograms within their budgets, the grids within 65 535 rows
    int64_t ts = n_series;
    ts = std::min<int64_t>(ts, std::max<int64_t>(1, (int64_t)(STATS_KEY_BYTES / (sizeof(uint64_t) * (size_t)std::max<int64_t>(M, 1)))));
    ts = std::min<int64_t>(ts, std::max<int64_t>(1, (int64_t)(STATS_HIST_BYTES / ((size_t)n_label * R * 256 * sizeof(uint32_t)))));
    ts = std::min<int64_t>(ts, 32768);
    const int64_t nseg = ts * n_label;
    const char *who = "met2_label_quantiles";
    DeviceWork W(s);
    const size_t sel = nch ? (size_t)nseg : 0;                 // the selection's pieces are empty without a large label: its kernels are not launched
    const auto d_q = W.take<double>(n_q);
    const auto d_label = W.take<int32_t>(nch), d_begin = W.take<int32_t>(nch), d_len = W.take<int32_t>(nch);
    const auto keys = W.take<uint64_t>((size_t)ts * (size_t)M);
    const auto ghist = W.take<uint32_t>(sel * R * 256);
    const auto nanc = W.take<int32_t>(sel);
    const auto pre_a = W.take<uint64_t>(sel * R), pre_b = W.take<uint64_t>(sel * R);
    const auto krank = W.take<uint32_t>(sel * R);
    if (!W.alloc()) return W.finish(who);
    std::vector<double> qv(q_host, q_host + n_q);
    if (!upload(W, d_q, qv, s) || !upload(W, d_label, ch.label, s) || !upload(W, d_begin, ch.begin, s) || !upload(W, d_len, ch.len, s))
        return W.finish(who);
    QArgs Q;
    Q.keys = keys; Q.M = M; Q.offset = offset; Q.n_label = n_label; Q.n_series = n_series; Q.n_q = n_q; Q.R = R; Q.q = d_q;
    Q.out = out; Q.out_stride = out_stride; Q.out_col = out_col;
    Q.chunk_label = d_label; Q.chunk_begin = d_begin; Q.chunk_len = d_len;
    Q.ghist = ghist; Q.nan_count = nanc; Q.krank = krank;
    const TileSrc src = tile_src(order, values, vs, ss);
    for (int64_t s0 = 0; s0 < n_series; s0 += ts) {
        const int ns = (int)std::min<int64_t>(ts, n_series - s0);
        Q.s0 = (int)s0; Q.ns = ns;
        if (M > 0) {
            hipLaunchKernelGGL(label_key_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)((ns + STATS_TS - 1) / STATS_TS)), dim3(256), 0, s, src, M,
                               (int)s0, ns, keys);
            if (!W.ok(hipGetLastError())) return W.finish(who);
        }
        if (any_small) {
            hipLaunchKernelGGL(label_small_kernel, dim3((unsigned)n_label, (unsigned)ns), dim3(256), 0, s, Q);
            if (!W.ok(hipGetLastError())) return W.finish(who);
        }
        if (!nch) continue;
        if (!W.ok(hipMemsetAsync(nanc, 0, sizeof(int32_t) * (size_t)nseg, s))) return W.finish(who);
        const unsigned step_grid = (unsigned)(((int64_t)ns * n_label * R + 255) / 256);
        for (int level = 0; level < 8; ++level) {
            Q.level = level;
            Q.prefix_in = (level & 1) ? pre_a : pre_b;
            Q.prefix_out = (level & 1) ? pre_b : pre_a;
            if (!W.ok(hipMemsetAsync(ghist, 0, sizeof(uint32_t) * (size_t)ns * n_label * R * 256, s))) return W.finish(who);
            hipLaunchKernelGGL(label_select_hist_kernel, dim3((unsigned)nch, (unsigned)ns), dim3(256), 0, s, Q);
            if (!W.ok(hipGetLastError())) return W.finish(who);
            hipLaunchKernelGGL(label_select_step_kernel, dim3(step_grid), dim3(256), 0, s, Q);
            if (!W.ok(hipGetLastError())) return W.finish(who);
        }
        Q.prefix_in = pre_b;                                   // level 7 wrote pre_b
        hipLaunchKernelGGL(label_select_finish_kernel, dim3((unsigned)(((int64_t)ns * n_label * n_q + 255) / 256)), dim3(256), 0, s, Q);
        if (!W.ok(hipGetLastError())) return W.finish(who);
    }
    return W.finish(who);
}

}  // namespace

extern "C" int met2_label_stats_limits(int32_t *chunk, int32_t *small_n, int32_t *max_label, int32_t *max_series, int32_t *max_q)
{
    if (chunk) *chunk = MET2_STATS_CHUNK;
    if (small_n) *small_n = MET2_STATS_SMALL_N;
    if (max_label) *max_label = MET2_STATS_MAX_LABEL;
    if (max_series) *max_series = MET2_STATS_MAX_SERIES;
    if (max_q) *max_q = MET2_STATS_MAX_Q;
    return MET2_OK;
}

extern "C" int met2_label_index(int32_t device, int64_t nvox, const int32_t *label, int32_t n_label, int32_t *offset, int32_t *order, void *stream)
{
    if (nvox < 0 || n_label < 1) return fail(MET2_E_INVALID, "nvox must not be negative and n_label must be positive");
    if (!offset || (nvox > 0 && (!label || !order))) return fail(MET2_E_INVALID, "NULL argument");
    if (nvox > 0x7fffffff) return fail(MET2_E_UNSUPPORTED, "2^31 voxels or more");
    if (n_label > MET2_STATS_MAX_LABEL) return fail(MET2_E_UNSUPPORTED, "more labels than MET2_STATS_MAX_LABEL");
    USE_DEVICE(device);
    return index_impl(nvox, label, n_label, offset, order, (hipStream_t)stream);
}

extern "C" int met2_label_moments(int32_t device, int32_t n_label, const int32_t *offset, const int32_t *order, int32_t n_series, const double *values,
                                  int64_t voxel_stride, int64_t series_stride, double *out, void *stream)
{
    int rc = common_checks(n_label, n_series, values, voxel_stride, series_stride);
    if (rc) return rc;
    if (!offset || !order || !out) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    std::vector<int32_t> off;
    if ((rc = fetch_offsets(offset, n_label, off, (hipStream_t)stream))) return rc;
    return moments_impl(off, n_label, order, n_series, values, voxel_stride, series_stride, out, 3, (hipStream_t)stream);
}

extern "C" int met2_label_quantiles(int32_t device, int32_t n_label, const int32_t *offset, const int32_t *order, int32_t n_series,
                                    const double *values, int64_t voxel_stride, int64_t series_stride, int32_t n_q, const double *q_host, double *out,
                                    void *stream)
{
    int rc = common_checks(n_label, n_series, values, voxel_stride, series_stride);
    if (rc) return rc;
    if ((rc = q_checks(n_q, q_host, 1))) return rc;
    if (!offset || !order || !out) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    std::vector<int32_t> off;
    if ((rc = fetch_offsets(offset, n_label, off, (hipStream_t)stream))) return rc;
    return quantiles_impl(off, n_label, offset, order, n_series, values, voxel_stride, series_stride, n_q, q_host, out, n_q, 0, (hipStream_t)stream);
}

extern "C" int met2_label_stats(int32_t device, int64_t nvox, const int32_t *label, int32_t n_label, int32_t n_series, const double *values,
                                int64_t voxel_stride, int64_t series_stride, int32_t n_q, const double *q_host, double *out, void *stream)
{
    if (nvox < 0) return fail(MET2_E_INVALID, "nvox must not be negative");
    int rc = common_checks(n_label, n_series, values, voxel_stride, series_stride);
    if (rc) return rc;
    if ((rc = q_checks(n_q, q_host, 0))) return rc;
    if (!out || (nvox > 0 && !label)) return fail(MET2_E_INVALID, "NULL argument");
    if (nvox > 0x7fffffff) return fail(MET2_E_UNSUPPORTED, "2^31 voxels or more");
    USE_DEVICE(device);
    hipStream_t s = (hipStream_t)stream;
    DeviceWork W(s);                                           // every stage below waits for the stream before it returns
    const auto offset = W.take<int32_t>((size_t)n_label + 1), order = W.take<int32_t>(nvox);
    if (!W.alloc()) return W.finish("met2_label_stats");
    if ((rc = index_impl(nvox, label, n_label, offset, order, s))) return rc;
    std::vector<int32_t> off;
    if ((rc = fetch_offsets(offset, n_label, off, s))) return rc;
    const int64_t stride = 3 + n_q;
    if ((rc = moments_impl(off, n_label, order, n_series, values, voxel_stride, series_stride, out, stride, s))) return rc;
    if (n_q == 0) return MET2_OK;
    return quantiles_impl(off, n_label, offset, order, n_series, values, voxel_stride, series_stride, n_q, q_host, out, stride, 3, s);
}
