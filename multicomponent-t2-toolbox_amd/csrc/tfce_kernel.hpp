// tfce_kernel.hpp -- the kernels and host helpers of the spatial statistics (threshold-free cluster enhancement, cluster extent and mass), stated once
// for the two units that run them: met2_tfce.hip (met2_tfce, met2_group_perm_tfce, met2_group_perm_ftfce) and met2_group_vsm.hip
// (met2_group_perm_vsm: the same transform and gather on the pseudo-t).  include/met2_hip.h states the definitions.  Written from that
// statement and from Smith & Nichols (NeuroImage 44:83-98, 2009); the lock-free union is the atomic-min hooking of Playne & Hawick's and
// Komura's label-equivalence kernels.  Everything sits in an unnamed namespace: each unit compiles its own copy from this one text.
// Components only merge as the threshold falls, so one union-find forest per map (parent[v] <= v, a root is its component's lowest index)
// persists while the levels are walked downward from the batch's top level; blockIdx.y is the map, a thread is a grid voxel.
//   tf_mask_kernel     the group entry's mask from `at`, which it also checks (inside the grid, strictly ascending)
//   tf_level_kernel    level(v) by a bisection of comparisons h_j <= t; parent = v, size = 0, sum = 0; the batch's top level: per block a
//                      butterfly and LDS, then one integer atomic max per block
//   tf_union_kernel    level j: a voxel of level j unites with every neighbour (tested on x, y, z) of level > j, and of level j below it
//   tf_count_kernel    level j: a voxel of level j adds 1 at its root; a voxel of a higher level that holds a size and is no root any more
//                      hands it to its root.  Integer adds at roots, which this kernel does not change: the sums do not depend on the order;
//                      the lanes of a wave that add to one root are summed by a butterfly first and make one atomic
//   tf_sum_kernel      level j: a voxel of level >= j adds its root's term e^E h_j^H to its own sum (it alone writes it) and points at its root
//   tf_mass_*_kernel   cluster mass: the level kernel's sibling that keeps q(v), the add at the roots, the spread and the roots' own conversion
//                      (described where they stand)
//   tf_finish_kernel   met2_tfce: out = dh * sum in place, and the map's maximum: one integer atomic max per (block, map) on gp_key
//   tf_gather_kernel   the group entry: a thread owns a masked voxel for all K maps: first, count, and the maxima as above
// Three launches per level and no host round trip between them; the level loop is the host's, bounded by MET2_TFCE_MAX_STEPS.  Every device
// loop is bounded (tf_find, tf_unite: the voxel count; the bisection: 11 steps); a bound that runs out raises flags[1] and the thread gives
// up, which the entry reports.  Integer atomics only.  A thread beyond the grid reads and writes nothing.  Compiled without contraction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_helpers.hpp"
#include "device_work.hpp"
#include "group_kernel.hpp"

#pragma clang fp contract(off)

namespace {

#define TF_BLOCK 256
#define TF_WAVES (TF_BLOCK / 64)
#define TF_BISECT 11                       // 2^11 > MET2_TFCE_MAX_STEPS + 1 candidates
static_assert((1 << TF_BISECT) > MET2_TFCE_MAX_STEPS + 1, "the bisection must cover every level");
static_assert(MET2_TFCE_MAX_STEPS < 65536, "levels are stored in 16 bits");
enum { TF_ERR_CHASE = 1, TF_ERR_RETRY = 2, TF_ERR_AT = 4 };

struct TfGrid { int nx, ny, nz, G; };      // G = nx ny nz < 2^31
struct TfForest {                          // per map and grid voxel
    uint16_t *level;
    int *parent;
    unsigned *size;
    double *sum;
    int *flags;                            // [0] the batch's top level, [1] TF_ERR_*
};

__device__ __forceinline__ int tf_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x, or -1 (and the flag) when more than G steps do not reach one; parent only ever falls, so a value read late is still an ancestor
__device__ __forceinline__ int tf_find(const int *parent, int x, int G, int *flags)
{
    for (int i = 0; i <= G; ++i) {
        const int p = tf_load(parent + x);
        if (p == x) return x;
        x = p;
    }
    atomicOr(flags + 1, TF_ERR_CHASE);
    return -1;
}

// joins the trees of a and b: the higher root is hooked under the lower by an atomic min; if it was no root any more, its former parent takes
// its place.  The pair only falls, hence the loop ends; the bound is the voxel count all the same.
__device__ __forceinline__ void tf_unite(int *parent, int a, int b, int G, int *flags)
{
    for (int it = 0; it <= G; ++it) {
        a = tf_find(parent, a, G, flags);
        b = tf_find(parent, b, G, flags);
        if (a < 0 || b < 0 || a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
    atomicOr(flags + 1, TF_ERR_RETRY);
}

__global__ void __launch_bounds__(TF_BLOCK) tf_mask_kernel(int64_t n_vox, const int32_t *__restrict__ at, int G, uint8_t *__restrict__ mask, int *flags)
{
    const int64_t v = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    if (v >= n_vox) return;
    const int a = at[v];
    if (a < 0 || a >= G || (v > 0 && at[v - 1] >= a)) { atomicOr(flags + 1, TF_ERR_AT); return; }
    mask[a] = 1;
}

__global__ void __launch_bounds__(TF_BLOCK) tf_level_kernel(TfGrid g, const double *__restrict__ maps, const uint8_t *__restrict__ mask, int max_level,
                                                            double dh, TfForest f)
{
    __shared__ int wtop[TF_WAVES];
    const int64_t v64 = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    const bool live = v64 < g.G;
    const int v = live ? (int)v64 : 0;
    const int64_t cell = (int64_t)blockIdx.y * g.G + v;
    int lo = 0;
    if (live && (!mask || mask[v])) {
        const double t = maps[cell];
        int hi = max_level;                                        // h_lo <= t (or lo = 0); h_j > t for j > hi.  Not a number: every test fails, lo stays 0
        for (int it = 0; it < TF_BISECT && lo < hi; ++it) {
            const int mid = (lo + hi + 1) >> 1;
            if (rn_mul((double)mid, dh) <= t) lo = mid; else hi = mid - 1;
        }
    }
    if (live) {
        f.level[cell] = (uint16_t)lo;
        f.parent[cell] = v;
        f.size[cell] = 0u;
        f.sum[cell] = 0.0;
    }
    int m = lo;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(m, o);
        if (other > m) m = other;
    }
    if ((threadIdx.x & 63) == 0) wtop[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TF_WAVES; ++w)
            if (wtop[w] > m) m = wtop[w];
        if (m > 0 && m > tf_load(f.flags)) atomicMax(f.flags, m);
    }
}

__global__ void __launch_bounds__(TF_BLOCK) tf_union_kernel(TfGrid g, int j, int reach, TfForest f)
{
    const int64_t v64 = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    if (v64 >= g.G) return;
    const int v = (int)v64;
    const int64_t base = (int64_t)blockIdx.y * g.G;
    const uint16_t *level = f.level + base;
    if (level[v] != j) return;
    int *parent = f.parent + base;
    const int z = v % g.nz, xy = v / g.nz, y = xy % g.ny, x = xy / g.ny;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz) {
                const int steps = (dx != 0) + (dy != 0) + (dz != 0);       // 1: a face, 2: an edge, 3: a corner
                if (steps == 0 || steps > reach) continue;
                const int X = x + dx, Y = y + dy, Z = z + dz;
                if (X < 0 || X >= g.nx || Y < 0 || Y >= g.ny || Z < 0 || Z >= g.nz) continue;
                const int u = (X * g.ny + Y) * g.nz + Z;
                const int lu = level[u];
                if (lu > j || (lu == j && u < v)) tf_unite(parent, v, u, g.G, f.flags);    // an equal neighbour above v does it from its side
            }
}

__global__ void __launch_bounds__(TF_BLOCK) tf_count_kernel(TfGrid g, int j, TfForest f)
{
    const int64_t v64 = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    const int64_t base = (int64_t)blockIdx.y * g.G;
    const int *parent = f.parent + base;
    unsigned *size = f.size + base;
    unsigned give = 0u;
    int root = -1;                                                 // -1: nothing to add.  No lane leaves before the wave's exchange below
    if (v64 < g.G) {
        const int v = (int)v64;
        const int lv = f.level[base + v];
        if (lv == j) {
            give = 1u;                                             // a voxel of this level brings itself
        } else if (lv > j && tf_load(parent + v) != v) {           // an earlier one: only a root of the level above that was hooked at this one
            give = size[v];                                        // nobody adds here: adds go to roots, and the forest is fixed in this kernel
            if (give != 0u) size[v] = 0u;
        }
        if (give != 0u) root = tf_find(parent, v, g.G, f.flags);
    }
    // The wave's lanes that add to one root do it in ONE atomic (at the lower levels thousands of voxels join the same few components): a
    // round per distinct root, 64 at the most.  Integer sums: the total does not depend on how the lanes are grouped.
    const int lane = threadIdx.x & 63;
    for (int round = 0; round < 64; ++round) {
        const unsigned long long todo = __ballot(root >= 0);
        if (todo == 0ull) break;
        const int lead = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(root, lead);
        const bool mine = root == r0;
        const unsigned part = wave_sum_xor(mine ? give : 0u);
        if (lane == lead) atomicAdd(size + r0, part);
        if (mine) root = -1;
    }
}

template <int MODE, bool HALF_TWO>
__global__ void __launch_bounds__(TF_BLOCK) tf_sum_kernel(TfGrid g, int j, double dh, double E, double H, TfForest f)
{
    const int64_t v64 = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    if (v64 >= g.G) return;
    const int v = (int)v64;
    const int64_t base = (int64_t)blockIdx.y * g.G;
    if (f.level[base + v] < j) return;
    int *parent = f.parent + base;
    const int root = tf_find(parent, v, g.G, f.flags);
    if (root < 0) return;
    if (root != v) __hip_atomic_store(parent + v, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // a shorter way next time; still an ancestor
    const double e = (double)f.size[base + root];
    double term;
    if (MODE == MET2_TFCE_MODE_EXTENT) {
        term = e;
    } else {
        const double h = rn_mul((double)j, dh);
        term = HALF_TWO ? rn_mul(sqrt(e), rn_mul(h, h)) : rn_mul(pow(e, E), pow(h, H));
    }
    f.sum[base + v] = rn_add(f.sum[base + v], term);
}

// ---- cluster mass (MET2_TFCE_MODE_MASS): the sum of the statistic over a voxel's component of {t >= h}, in 64-bit fixed point ------------
// A voxel's 8-byte sum cell holds, in turn: the integer q(v) (tf_mass_level_kernel); at a root, the component's integer total
// (tf_mass_add_kernel); the double out(v) (tf_mass_spread_kernel for the others, tf_mass_root_kernel for the roots).  Integer adds only, so
// the total does not depend on the order; the one conversion to double rounds to nearest even and the scaling by 2^-24 is exact.

__device__ __forceinline__ double tf_mass_value(unsigned long long total)
{
    return rn_mul((double)(long long)total, 1.0 / (double)(1 << MET2_TFCE_MASS_FRAC_BITS));
}

// tf_level_kernel with one level (dh is the threshold), but the sum cell takes the bits of q(v) = rint(min(t, cap) 2^24), 0 for a non-member
__global__ void __launch_bounds__(TF_BLOCK) tf_mass_level_kernel(TfGrid g, const double *__restrict__ maps, const uint8_t *__restrict__ mask, double dh, TfForest f)
{
    __shared__ int wtop[TF_WAVES];
    const int64_t v64 = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    const bool live = v64 < g.G;
    const int v = live ? (int)v64 : 0;
    const int64_t cell = (int64_t)blockIdx.y * g.G + v;
    int lo = 0;
    long long q = 0;
    if (live && (!mask || mask[v])) {
        const double t = maps[cell];
        if (rn_mul(1.0, dh) <= t) {                                 // not a number: the test fails
            lo = 1;
            const double c = t < MET2_TFCE_MASS_T_CAP ? t : MET2_TFCE_MASS_T_CAP;       // +infinity saturates
            q = __double2ll_rn(rn_mul(c, (double)(1 << MET2_TFCE_MASS_FRAC_BITS)));      // the product is exact; ties to even; <= 2^38
        }
    }
    if (live) {
        f.level[cell] = (uint16_t)lo;
        f.parent[cell] = v;
        f.size[cell] = 0u;
        ((long long *)f.sum)[cell] = q;                            // after t was read: maps may be the sum buffer itself
    }
    int m = lo;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(m, o);
        if (other > m) m = other;
    }
    if ((threadIdx.x & 63) == 0) wtop[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TF_WAVES; ++w)
            if (wtop[w] > m) m = wtop[w];
        if (m > 0 && m > tf_load(f.flags)) atomicMax(f.flags, m);
    }
}

// every member that is not its own root adds its q to its root's cell.  The forest is fixed here; a cell that is no root's is read by its owner
// alone, and the adds go to roots only.  As in tf_count_kernel the wave's lanes that share a root make ONE atomic: a round per distinct root.
__global__ void __launch_bounds__(TF_BLOCK) tf_mass_add_kernel(TfGrid g, TfForest f)
{
    const int64_t v64 = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    const int64_t base = (int64_t)blockIdx.y * g.G;
    unsigned long long *cells = (unsigned long long *)f.sum + base;
    unsigned long long give = 0ull;
    int root = -1;                                                 // -1: nothing to add.  No lane leaves before the wave's exchange below
    if (v64 < g.G) {
        const int v = (int)v64;
        if (f.level[base + v] == 1) {
            const int r = tf_find(f.parent + base, v, g.G, f.flags);
            if (r >= 0 && r != v) {
                root = r;
                give = cells[v];
            }
        }
    }
    const int lane = threadIdx.x & 63;
    for (int round = 0; round < 64; ++round) {
        const unsigned long long todo = __ballot(root >= 0);
        if (todo == 0ull) break;
        const int lead = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(root, lead);
        const bool mine = root == r0;
        const unsigned long long part = wave_sum_xor(mine ? give : 0ull);      // 64 lanes of at most 2^38: no overflow
        if (lane == lead) atomicAdd(cells + r0, part);
        if (mine) root = -1;
    }
}

// every member that is not its own root takes its root's integer total and writes the double over its own cell; roots write nothing here,
// so no cell is read and rewritten in one launch
__global__ void __launch_bounds__(TF_BLOCK) tf_mass_spread_kernel(TfGrid g, TfForest f)
{
    const int64_t v64 = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    if (v64 >= g.G) return;
    const int v = (int)v64;
    const int64_t base = (int64_t)blockIdx.y * g.G;
    if (f.level[base + v] != 1) return;
    const int root = tf_find(f.parent + base, v, g.G, f.flags);
    if (root < 0 || root == v) return;
    f.sum[base + v] = tf_mass_value(((const unsigned long long *)f.sum)[base + root]);
}

// the roots convert their own totals in place
__global__ void __launch_bounds__(TF_BLOCK) tf_mass_root_kernel(TfGrid g, TfForest f)
{
    const int64_t v64 = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    if (v64 >= g.G) return;
    const int v = (int)v64;
    const int64_t cell = (int64_t)blockIdx.y * g.G + v;
    if (f.level[cell] != 1 || f.parent[cell] != v) return;
    f.sum[cell] = tf_mass_value(((const unsigned long long *)f.sum)[cell]);
}

// the block's maximum of m for map k -> kmax[k], one atomic at the most; wmax: TF_WAVES doubles of LDS
__device__ __forceinline__ void tf_block_max(double m, double *wmax, unsigned long long *dst)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(m, o);
        if (other > m) m = other;
    }
    __syncthreads();                                               // the previous call's reader is done
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TF_WAVES; ++w)
            if (wmax[w] > m) m = wmax[w];
        const unsigned long long key = gp_key((unsigned long long)__double_as_longlong(m));
        if (key > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, key);
    }
}

__global__ void __launch_bounds__(TF_BLOCK) tf_finish_kernel(TfGrid g, double scale, int scaled, double *__restrict__ out, unsigned long long *__restrict__ kmax)
{
    __shared__ double wmax[TF_WAVES];
    const int64_t v = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    const bool live = v < g.G;
    double s = -INFINITY;
    if (live) {
        const int64_t cell = (int64_t)blockIdx.y * g.G + v;
        s = out[cell];
        if (scaled) out[cell] = s = rn_mul(scale, s);
    }
    if (kmax) tf_block_max(s, wmax, kmax + blockIdx.y);
}

__global__ void __launch_bounds__(TF_BLOCK) tf_gather_kernel(int64_t n_vox, const int32_t *__restrict__ at, int G, int K, double scale, int scaled,
                                                             const double *__restrict__ sum, const double *__restrict__ ref, double *__restrict__ first,
                                                             unsigned long long *__restrict__ kmax, uint32_t *__restrict__ count)
{
    __shared__ double wmax[TF_WAVES];
    const int64_t v = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    const bool live = v < n_vox;
    const int a = live ? at[v] : 0;
    const double rf = (ref && live) ? ref[v] : 0.0;
    uint32_t cnt = 0;
    for (int k = 0; k < K; ++k) {
        double s = -INFINITY;
        if (live) {
            s = sum[(int64_t)k * G + a];
            if (scaled) s = rn_mul(scale, s);
            if (ref && s >= rf) ++cnt;
            if (first && k == 0) first[v] = s;
        }
        tf_block_max(s, wmax, kmax + k);
    }
    if (ref && live) count[v] += cnt;                              // this thread owns the voxel
}

struct TfParams { int mode; double dh, E, H; int reach; };

int tf_check(int K, const int32_t *dims, int mode, double dh, double E, double H, int connectivity, TfGrid *g, TfParams *p)
{
    if (!dims) return fail(MET2_E_INVALID, "NULL argument");
    if (K < 1 || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return fail(MET2_E_INVALID, "K and every axis must be >= 1");
    if (mode != MET2_TFCE_MODE_TFCE && mode != MET2_TFCE_MODE_EXTENT && mode != MET2_TFCE_MODE_MASS)
        return fail(MET2_E_INVALID, "mode must be MET2_TFCE_MODE_TFCE, MET2_TFCE_MODE_EXTENT or MET2_TFCE_MODE_MASS");
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return fail(MET2_E_INVALID, "connectivity must be 6, 18 or 26");
    if (!std::isfinite(dh) || dh <= 0.0) return fail(MET2_E_INVALID, "dh (the threshold in extent and mass mode) must be finite and > 0");
    if (mode == MET2_TFCE_MODE_TFCE && (!std::isfinite(E) || E <= 0.0 || !std::isfinite(H) || H < 0.0))
        return fail(MET2_E_INVALID, "E must be finite and > 0, H finite and >= 0");
    if (K > MET2_TFCE_MAX_K) return fail(MET2_E_UNSUPPORTED, "K <= " + std::to_string(MET2_TFCE_MAX_K) + " maps per call");
    if ((double)dims[0] * (double)dims[1] * (double)dims[2] >= 2147483648.0) return fail(MET2_E_UNSUPPORTED, "the grid must hold fewer than 2^31 voxels");
    const int64_t G = (int64_t)dims[0] * dims[1] * dims[2];
    if (mode == MET2_TFCE_MODE_MASS && G > (int64_t)MET2_TFCE_MASS_MAX_G)
        return fail(MET2_E_UNSUPPORTED, "in mass mode the grid must hold at most 2^24 voxels: the 64-bit sum of the fixed-point statistic must not overflow");
    *g = TfGrid{dims[0], dims[1], dims[2], (int)G};
    *p = TfParams{mode, dh, E, H, connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3};
    return MET2_OK;
}

// the pieces of the work space, in one order for the size entry and the calls
struct TfWork {
    DeviceWork::Piece<int> flags;
    DeviceWork::Piece<uint16_t> level;
    DeviceWork::Piece<int> parent;
    DeviceWork::Piece<unsigned> size;
    DeviceWork::Piece<double> dense;       // the group entry only
    DeviceWork::Piece<uint8_t> mask;       // the group entry only
};
TfWork tf_take(DeviceWork &w, int K, int64_t G, bool group)
{
    const size_t cells = (size_t)K * (size_t)G;
    TfWork t{w.take<int>(2), w.take<uint16_t>(cells), w.take<int>(cells), w.take<unsigned>(cells), w.take<double>(group ? cells : 0),
             w.take<uint8_t>(group ? (size_t)G : 0)};
    return t;
}
size_t tf_bytes(const TfWork &t) { return t.mask.off + t.mask.bytes; }

// levels, then the walk down from the top level.  *top_out: the batch's top level; *err_out: the flags read with it.
// Returns without the walk when the flags already hold an error.
int tf_transform(DeviceWork &w, const TfGrid &g, int K, const TfParams &p, const double *maps, const uint8_t *mask, TfForest f, hipStream_t st, int *err_out)
{
    const dim3 grid((unsigned)((g.G + TF_BLOCK - 1) / TF_BLOCK), (unsigned)K), block(TF_BLOCK);
    const bool mass = p.mode == MET2_TFCE_MODE_MASS;
    const int max_level = p.mode == MET2_TFCE_MODE_TFCE ? MET2_TFCE_MAX_STEPS : 1;
    if (mass)
        hipLaunchKernelGGL(tf_mass_level_kernel, grid, block, 0, st, g, maps, mask, p.dh, f);
    else
        hipLaunchKernelGGL(tf_level_kernel, grid, block, 0, st, g, maps, mask, max_level, p.dh, f);
    int host_flags[2] = {0, 0};
    if (!w.ok(hipMemcpyAsync(host_flags, f.flags, sizeof host_flags, hipMemcpyDeviceToHost, st)) || !w.ok(hipStreamSynchronize(st))) return MET2_E_HIP;
    *err_out = host_flags[1];
    if (host_flags[1]) return MET2_OK;
    const int top = host_flags[0] < max_level ? host_flags[0] : max_level;
    if (mass) {                                                    // one level: the union, then the three passes over the sum cells
        if (top >= 1) {
            hipLaunchKernelGGL(tf_union_kernel, grid, block, 0, st, g, 1, p.reach, f);
            hipLaunchKernelGGL(tf_mass_add_kernel, grid, block, 0, st, g, f);
            hipLaunchKernelGGL(tf_mass_spread_kernel, grid, block, 0, st, g, f);
            hipLaunchKernelGGL(tf_mass_root_kernel, grid, block, 0, st, g, f);
        }
        return MET2_OK;
    }
    const bool half_two = p.E == 0.5 && p.H == 2.0;
    for (int j = top; j >= 1; --j) {                               // <= MET2_TFCE_MAX_STEPS
        hipLaunchKernelGGL(tf_union_kernel, grid, block, 0, st, g, j, p.reach, f);
        hipLaunchKernelGGL(tf_count_kernel, grid, block, 0, st, g, j, f);
        if (p.mode == MET2_TFCE_MODE_EXTENT)
            hipLaunchKernelGGL((tf_sum_kernel<MET2_TFCE_MODE_EXTENT, false>), grid, block, 0, st, g, j, p.dh, p.E, p.H, f);
        else if (half_two)
            hipLaunchKernelGGL((tf_sum_kernel<MET2_TFCE_MODE_TFCE, true>), grid, block, 0, st, g, j, p.dh, p.E, p.H, f);
        else
            hipLaunchKernelGGL((tf_sum_kernel<MET2_TFCE_MODE_TFCE, false>), grid, block, 0, st, g, j, p.dh, p.E, p.H, f);
    }
    return MET2_OK;
}

// the flags after the walk: read with the wait that gives the work space back
int tf_late_error(DeviceWork &w, const int *flags, hipStream_t st, const char *who)
{
    int host_flags[2] = {0, 0};
    if (!w.ok(hipMemcpyAsync(host_flags, flags, sizeof host_flags, hipMemcpyDeviceToHost, st)) || !w.ok(hipStreamSynchronize(st))) return w.finish(who);
    const int rc = w.finish(who);
    if (rc != MET2_OK) return rc;
    if (host_flags[1]) return fail(MET2_E_HIP, std::string(who) + ": a bounded loop of the union-find ran out (flags " + std::to_string(host_flags[1]) + ")");
    return MET2_OK;
}

}  // namespace
