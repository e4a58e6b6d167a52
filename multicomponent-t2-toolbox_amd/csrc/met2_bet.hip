// met2_bet.hip -- met2_brain_mask: brain extraction of a 3-D volume (brain_mask='yes'; step 3 of the reference's example pipeline, which runs
// FSL's bet on the echo mean on the CPU).  The surface model of Smith (Fast robust automated brain extraction, HBM 2002) without bet's
// self-intersection retry pass; include/met2_hip.h states the algorithm; no program text of FSL was used.
//   bet_mean_kernel       the echo mean
//   bet_range_kernel      min, max and number of the finite voxels, one partial per chunk of 1024 voxels
//   bet_hist_kernel       the 1000-bin histogram (integer atomics, LDS then global)
//   bet_cog_kernel        count of v > t and the partial sums of w, w x, w y, w z per chunk, in a fixed order; the host adds the partials in
//                         ascending order
//   bet_select_kernel     one 8-bit digit of the radix selection of the median: a 256-bin histogram of the keys that share the prefix found so
//                         far (integer atomics); bet_upper_kernel finds the next larger key for an even count (integer atomics)
//   bet_evolve_kernel     ALL iterations of the surface in ONE workgroup of 1024 threads: both position buffers (2 x 3 nv doubles: 123 KB at level
//                         4) and the neighbour rings (int16 [nv][6]: 31 KB) in LDS, up to three vertices per thread, one after the other; the
//                         intensity samples of a vertex are loaded ten at a time; one barrier per iteration and one more at every refresh of
//                         l.  Every thread reaches every barrier: the trip count is a kernel argument.
//   bet_fill_kernel       one thread per (x, y) column walks the triangles, toggles one flag per crossing in its own column of the mask and
//                         turns the flags into the parity from the top: no atomics, nothing depends on scheduling
// The statistics come back to the host between the stages (the host builds the start mesh from them).  fp64 throughout; no product is fused
// into a sum in this file (fp contract off), so that every expression rounds as it is written in the header.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_helpers.hpp"
#include "device_work.hpp"

#pragma clang fp contract(off)

namespace {

#define BET_NBINS 1000
#define BET_CHUNK 1024                    // voxels per partial: 256 threads x 4
#define BET_T 1024                        // threads of the evolution's one workgroup
#define BET_MAX_LEVEL 4
#define BET_D1 20                         // depth of the search for Imin, mm
#define BET_D2 10                         // and for Imax
#define BET_BATCH 10                     // samples in flight per vertex: divides BET_D1
#define BET_L_EVERY 50
#define BET_RMIN 3.33
#define BET_RMAX 10.0

__global__ __launch_bounds__(256) void bet_mean_kernel(const double *__restrict__ data, int64_t n, int nt, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *d = data + i * nt;
    double s = d[0];
    for (int e = 1; e < nt; ++e) s += d[e];
    out[i] = s / (double)nt;
}

__global__ __launch_bounds__(256) void bet_range_kernel(const double *__restrict__ v, int64_t n, double *__restrict__ pmin, double *__restrict__ pmax,
                                                        int32_t *__restrict__ pcnt)
{
    __shared__ double rmn[4], rmx[4];
    __shared__ int rc[4];
    const int64_t c0 = (int64_t)blockIdx.x * BET_CHUNK;
    double mn = INFINITY, mx = -INFINITY;
    int c = 0;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < n) {
            const double val = v[i];
            if (isfinite(val)) {
                mn = fmin(mn, val);
                mx = fmax(mx, val);
                ++c;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o));
        mx = fmax(mx, __shfl_xor(mx, o));
        c += __shfl_xor(c, o);
    }
    if ((threadIdx.x & 63) == 0) { rmn[threadIdx.x >> 6] = mn; rmx[threadIdx.x >> 6] = mx; rc[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        pmin[blockIdx.x] = fmin(fmin(rmn[0], rmn[1]), fmin(rmn[2], rmn[3]));
        pmax[blockIdx.x] = fmax(fmax(rmx[0], rmx[1]), fmax(rmx[2], rmx[3]));
        pcnt[blockIdx.x] = rc[0] + rc[1] + rc[2] + rc[3];
    }
}

__global__ __launch_bounds__(256) void bet_hist_kernel(const double *__restrict__ v, int64_t n, double lo, double hi, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t lh[BET_NBINS];
    for (int b = threadIdx.x; b < BET_NBINS; b += 256) lh[b] = 0;
    __syncthreads();
    const int64_t c0 = (int64_t)blockIdx.x * BET_CHUNK;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < n) {
            const double val = v[i];
            if (isfinite(val)) {
                int bin = (int)floor((val - lo) / (hi - lo) * (double)BET_NBINS);        // lo <= val <= hi: 0 .. 1000
                bin = bin < 0 ? 0 : bin > BET_NBINS - 1 ? BET_NBINS - 1 : bin;
                atomicAdd(&lh[bin], 1u);
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < BET_NBINS; b += 256)
        if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

struct Grid {
    int nx, ny, nz;
    double dx, dy, dz;
};

// partials of chunk c: part[q * nch + c], q = 0 .. 3 for w, w x, w y, w z; a thread adds its four voxels in ascending order
__global__ __launch_bounds__(256) void bet_cog_kernel(const double *__restrict__ v, int64_t n, Grid g, double t, double t2, double t98, int nch,
                                                      double *__restrict__ part, int32_t *__restrict__ pcnt)
{
    __shared__ double red[4];
    __shared__ int rc[4];
    const int64_t c0 = (int64_t)blockIdx.x * BET_CHUNK;
    double sw = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    int c = 0;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < n) {
            const double val = v[i];
            if (isfinite(val) && val > t) {
                const int iz = (int)(i % g.nz), iy = (int)((i / g.nz) % g.ny), ix = (int)(i / ((int64_t)g.nz * g.ny));
                const double w = fmin(val, t98) - t2;
                sw += w;
                sx += w * ((double)ix * g.dx);
                sy += w * ((double)iy * g.dy);
                sz += w * ((double)iz * g.dz);
                ++c;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) rc[threadIdx.x >> 6] = c;
    sw = block_sum(sw, red);
    sx = block_sum(sx, red);
    sy = block_sum(sy, red);
    sz = block_sum(sz, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = sw;
        part[nch + blockIdx.x] = sx;
        part[2 * nch + blockIdx.x] = sy;
        part[3 * nch + blockIdx.x] = sz;
        pcnt[blockIdx.x] = rc[0] + rc[1] + rc[2] + rc[3];
    }
}

// keys in the order of the values they stand for
// (not to_key of met2_stats.hip or tv_key of met2_tv.hip: the median set holds finite values only, and -0.0 keeps its own key below +0.0's)
__device__ __forceinline__ uint64_t sort_key(double x)
{
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : b | 0x8000000000000000ULL;
}

struct Sphere {
    double cx, cy, cz, r2, t2, t98;
};

// is voxel i one of those the median is taken of?
__device__ __forceinline__ bool in_median_set(double val, int64_t i, const Grid &g, const Sphere &s)
{
    if (!(val > s.t2 && val < s.t98)) return false;                   // false for a NaN
    const int iz = (int)(i % g.nz), iy = (int)((i / g.nz) % g.ny), ix = (int)(i / ((int64_t)g.nz * g.ny));
    const double ex = (double)ix * g.dx - s.cx, ey = (double)iy * g.dy - s.cy, ez = (double)iz * g.dz - s.cz;
    return (ex * ex + ey * ey) + ez * ez <= s.r2;
}

// histogram of the digit at `shift` over the keys with (key & decided) == prefix
__global__ __launch_bounds__(256) void bet_select_kernel(const double *__restrict__ v, int64_t n, Grid g, Sphere s, uint64_t decided, uint64_t prefix,
                                                         int shift, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t lh[256];
    lh[threadIdx.x] = 0;
    __syncthreads();
    const int64_t c0 = (int64_t)blockIdx.x * BET_CHUNK;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < n) {
            const double val = v[i];
            if (in_median_set(val, i, g, s)) {
                const uint64_t key = sort_key(val);
                if ((key & decided) == prefix) atomicAdd(&lh[(int)((key >> shift) & 255u)], 1u);
            }
        }
    }
    __syncthreads();
    if (lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], lh[threadIdx.x]);
}

// res[0] += the number of keys <= key, res[1] = min(res[1], the smallest key above key)
__global__ __launch_bounds__(256) void bet_upper_kernel(const double *__restrict__ v, int64_t n, Grid g, Sphere s, uint64_t key,
                                                        unsigned long long *__restrict__ res)
{
    const int64_t c0 = (int64_t)blockIdx.x * BET_CHUNK;
    unsigned long long le = 0, up = ~0ULL;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = c0 + j * 256 + threadIdx.x;
        if (i < n) {
            const double val = v[i];
            if (in_median_set(val, i, g, s)) {
                const uint64_t k = sort_key(val);
                if (k <= key) ++le; else up = k < up ? k : up;
            }
        }
    }
    if (le) atomicAdd(&res[0], le);
    if (up != ~0ULL) atomicMin(&res[1], up);
}

struct EvolveArgs {
    const double *v;
    Grid g;
    double wx, wy, wz;                    // 1 / voxel size
    double t2, t, tm, E, F, bt;
    int nv, n_iter, degsum;
    const double *xin;                    // [nv][3]
    double *xout;
    const int16_t *ring;                  // [nv][6], -1 beyond the degree
};

// the flat index of the voxel nearest to (px, py, pz) mm, or -1 outside the volume (and for a NaN)
__device__ __forceinline__ int nearest_voxel(const EvolveArgs &A, double px, double py, double pz)
{
    const double fx = floor(px * A.wx + 0.5), fy = floor(py * A.wy + 0.5), fz = floor(pz * A.wz + 0.5);
    const bool in = fx >= 0.0 && fx < (double)A.g.nx && fy >= 0.0 && fy < (double)A.g.ny && fz >= 0.0 && fz < (double)A.g.nz;
    return in ? ((int)fx * A.g.ny + (int)fy) * A.g.nz + (int)fz : -1;                    // fewer than 2^31 voxels
}

// a vertex' ring from the table in LDS: the neighbours' indices (0 beyond the degree) -> the degree
__device__ __forceinline__ int load_ring(const int16_t *ring, int i, int nb[6])
{
    int dg = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int r = ring[i * 6 + k];
        nb[k] = r < 0 ? 0 : r;
        dg += r >= 0 ? 1 : 0;                                           // the host's table fills a ring from the front
    }
    return dg;
}

__global__ __launch_bounds__(BET_T) void bet_evolve_kernel(EvolveArgs A)
{
    extern __shared__ double pos[];                                    // two buffers of x[nv], y[nv], z[nv], then the rings: int16 [nv][6]
    __shared__ double red[BET_T / 64];
    const int nv = A.nv, tid = threadIdx.x;
    double *cur = pos, *nxt = pos + 3 * nv;
    int16_t *ring = (int16_t *)(pos + 6 * nv);
    for (int e = tid; e < 6 * nv; e += BET_T) {
        const int r = A.ring[e];
        ring[e] = (int16_t)(r >= 0 && r < nv ? r : -1);                // the host's table holds nothing else
    }
    for (int i = tid; i < nv; i += BET_T) {
        cur[i] = A.xin[3 * i];
        cur[nv + i] = A.xin[3 * i + 1];
        cur[2 * nv + i] = A.xin[3 * i + 2];
    }
    __syncthreads();
    double l = 0.0;
    for (int it = 0; it < A.n_iter; ++it) {                            // uniform: every thread reaches every barrier
        if (it % BET_L_EVERY == 0) {
            double s = 0.0;
#pragma unroll 1
            for (int i = tid; i < nv; i += BET_T) {
                int nb[6];
                const int dg = load_ring(ring, i, nb);
                const double x = cur[i], y = cur[nv + i], z = cur[2 * nv + i];
                double sv = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    if (k < dg) {
                        const int p = nb[k];
                        const double ex = cur[p] - x, ey = cur[nv + p] - y, ez = cur[2 * nv + p] - z;
                        sv += sqrt((ex * ex + ey * ey) + ez * ez);
                    }
                }
                s += sv;
            }
            s = wave_sum_xor(s);
            if ((tid & 63) == 0) red[tid >> 6] = s;                    // the last readers of red are a barrier behind
            __syncthreads();
            double tot = 0.0;
            for (int w = 0; w < BET_T / 64; ++w) tot += red[w];
            l = tot / (double)A.degsum;
        }
#pragma unroll 1
        for (int i = tid; i < nv; i += BET_T) {                        // one vertex at a time: its registers are all that is live
            int nb[6];
            const int dg = load_ring(ring, i, nb);
            const double x = cur[i], y = cur[nv + i], z = cur[2 * nv + i];
            double ex[6], ey[6], ez[6];
            double mx = 0.0, my = 0.0, mz = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int p = nb[k];
                const double qx = cur[p], qy = cur[nv + p], qz = cur[2 * nv + p];
                ex[k] = qx - x; ey[k] = qy - y; ez[k] = qz - z;
                if (k < dg) { mx += qx; my += qy; mz += qz; }
            }
            double nx = 0.0, ny = 0.0, nz = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                if (k < dg) {
                    const bool last = k + 1 == dg;                         // the ring closes on its first entry
                    const double bx = last ? ex[0] : ex[k + 1 < 6 ? k + 1 : 0], by = last ? ey[0] : ey[k + 1 < 6 ? k + 1 : 0],
                                 bz = last ? ez[0] : ez[k + 1 < 6 ? k + 1 : 0];
                    nx += ey[k] * bz - ez[k] * by;
                    ny += ez[k] * bx - ex[k] * bz;
                    nz += ex[k] * by - ey[k] * bx;
                }
            }
            const double nl = sqrt((nx * nx + ny * ny) + nz * nz);
            if (nl > 0.0) { nx /= nl; ny /= nl; nz /= nl; } else { nx = 0.0; ny = 0.0; nz = 0.0; }
            const double dgd = (double)dg;
            const double sx = mx / dgd - x, sy = my / dgd - y, sz = mz / dgd - z;
            const double sd = (sx * nx + sy * ny) + sz * nz;
            const double snx = sd * nx, sny = sd * ny, snz = sd * nz;
            const double f2 = (1.0 + tanh(A.F * (2.0 * fabs(sd) / (l * l) - A.E))) * 0.5;
            // I(d), BET_BATCH depths at a time: the addresses first, then the loads with no branch between them (outside the volume voxel 0
            // is read and dropped), so that a wave waits for memory once per batch and not once per sample
            double imin = INFINITY, imax = -INFINITY;
#pragma unroll
            for (int d0 = 1; d0 <= BET_D1; d0 += BET_BATCH) {
                int at[BET_BATCH];
                double val[BET_BATCH];
#pragma unroll
                for (int b = 0; b < BET_BATCH; ++b) {
                    const double dd = (double)(d0 + b);
                    at[b] = nearest_voxel(A, x - dd * nx, y - dd * ny, z - dd * nz);
                }
#pragma unroll
                for (int b = 0; b < BET_BATCH; ++b) val[b] = A.v[at[b] < 0 ? 0 : at[b]];
#pragma unroll
                for (int b = 0; b < BET_BATCH; ++b) {
                    const double I = at[b] >= 0 && isfinite(val[b]) ? val[b] : 0.0;
                    imin = fmin(imin, I);
                    if (d0 + b <= BET_D2) imax = fmax(imax, I);
                }
            }
            imin = fmax(A.t2, fmin(A.tm, imin));
            imax = fmin(A.tm, fmax(A.t, imax));
            const double den = imax - A.t2;
            const double tl = den * A.bt + A.t2;
            const double f3 = den > 0.0 ? 2.0 * (imin - tl) / den : 0.0;
            const double u3 = (0.05 * f3) * l;
            nxt[i] = ((x + 0.5 * (sx - snx)) + f2 * snx) + u3 * nx;
            nxt[nv + i] = ((y + 0.5 * (sy - sny)) + f2 * sny) + u3 * ny;
            nxt[2 * nv + i] = ((z + 0.5 * (sz - snz)) + f2 * snz) + u3 * nz;
        }
        __syncthreads();                                               // nxt is complete and cur is read no more
        double *sw = cur; cur = nxt; nxt = sw;
    }
    for (int i = tid; i < nv; i += BET_T) {
        A.xout[3 * i] = cur[i];
        A.xout[3 * i + 1] = cur[nv + i];
        A.xout[3 * i + 2] = cur[2 * nv + i];
    }
}

// where the edge between vertices i and j (walked from the one of the smaller index, so that both triangles of an edge compute the same
// bits) meets the line y = py: -> does it (half-open in y), and x and z there
__device__ __forceinline__ bool edge_cross(const double *__restrict__ X, int i, int j, double py, double &x, double &z)
{
    const double *p = X + 3 * (i < j ? i : j), *q = X + 3 * (i < j ? j : i);
    if ((p[1] <= py) == (q[1] <= py)) return false;
    const double h = q[1] - p[1];
    x = p[0] + ((py - p[1]) * (q[0] - p[0])) / h;
    z = p[2] + ((py - p[1]) * (q[2] - p[2])) / h;
    return true;
}

__global__ __launch_bounds__(256) void bet_fill_kernel(const double *__restrict__ X, int nv, const int32_t *__restrict__ tri, int ntri, Grid g,
                                                       uint8_t *__restrict__ mask)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= g.nx * g.ny) return;                                    // no barrier in this kernel
    const int ix = col / g.ny, iy = col % g.ny;
    const double px = (double)ix * g.dx, py = (double)iy * g.dy;
    uint8_t *m = mask + (int64_t)col * g.nz;                           // this thread's own column
    for (int k = 0; k < g.nz; ++k) m[k] = 0;
    for (int t = 0; t < ntri; ++t) {                                   // uniform over the wave: the triangle comes through scalar loads
        const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) continue;
        const bool fa = X[3 * a + 1] <= py, fb = X[3 * b + 1] <= py, fc = X[3 * c + 1] <= py;
        if (fa == fb && fb == fc) continue;
        double x0 = 0.0, z0 = 0.0, x1 = 0.0, z1 = 0.0, x2 = 0.0, z2 = 0.0;
        const bool c0 = edge_cross(X, a, b, py, x0, z0), c1 = edge_cross(X, b, c, py, x1, z1), c2 = edge_cross(X, c, a, py, x2, z2);
        if (!(c0 || c1 || c2)) continue;
        const double xa = c0 ? x0 : x1, za = c0 ? z0 : z1, xb = c2 ? x2 : x1, zb = c2 ? z2 : z1;
        const bool ra = xa > px, rb = xb > px;
        if (ra == rb) continue;
        const double xl = ra ? xb : xa, zl = ra ? zb : za, xr = ra ? xa : xb, zr = ra ? za : zb;
        const double zc = zl + ((px - xl) * (zr - zl)) / (xr - xl);
        const double mz = ceil(zc / g.dz);
        if (mz >= 1.0) {                                               // false for a NaN
            const int k = (mz >= (double)g.nz ? g.nz : (int)mz) - 1;   // 0 .. nz - 1
            m[k] ^= 1;
        }
    }
    uint8_t run = 0;
    for (int k = g.nz - 1; k >= 0; --k) {
        run ^= m[k];
        m[k] = run;
    }
}

// ---- host side ----

struct Mesh {
    std::vector<double> unit;             // [nv][3]
    std::vector<int32_t> tri;             // [nt][3]
    std::vector<int32_t> ring;            // [nv][6], -1 beyond the degree
    std::vector<int32_t> deg;
    int nv() const { return (int)deg.size(); }
    int nt() const { return (int)tri.size() / 3; }
};

void push_unit(std::vector<double> &u, double x, double y, double z)
{
    const double n = std::sqrt((x * x + y * y) + z * z);
    u.push_back(x / n);
    u.push_back(y / n);
    u.push_back(z / n);
}

Mesh build_mesh(int level)
{
    Mesh M;
    const double phi = (1.0 + std::sqrt(5.0)) / 2.0;
    const double base[12][3] = {{-1, phi, 0}, {1, phi, 0}, {-1, -phi, 0}, {1, -phi, 0}, {0, -1, phi}, {0, 1, phi}, {0, -1, -phi}, {0, 1, -phi},
                                {phi, 0, -1}, {phi, 0, 1}, {-phi, 0, -1}, {-phi, 0, 1}};
    const int32_t faces[20][3] = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4}, {11, 10, 2}, {10, 7, 6}, {7, 1, 8},
                                  {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8}, {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
    for (auto &p : base) push_unit(M.unit, p[0], p[1], p[2]);
    for (auto &f : faces) M.tri.insert(M.tri.end(), f, f + 3);
    for (int s = 0; s < level; ++s) {
        std::map<std::pair<int32_t, int32_t>, int32_t> mid;
        std::vector<int32_t> out;
        auto midpoint = [&](int32_t a, int32_t b) {
            const std::pair<int32_t, int32_t> key(std::min(a, b), std::max(a, b));
            auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            const double *p = &M.unit[3 * key.first], *q = &M.unit[3 * key.second];
            const double x = (p[0] + q[0]) * 0.5, y = (p[1] + q[1]) * 0.5, z = (p[2] + q[2]) * 0.5;
            push_unit(M.unit, x, y, z);
            const int32_t id = (int32_t)(M.unit.size() / 3) - 1;
            mid[key] = id;
            return id;
        };
        for (size_t t = 0; t < M.tri.size(); t += 3) {
            const int32_t a = M.tri[t], b = M.tri[t + 1], c = M.tri[t + 2];
            const int32_t ab = midpoint(a, b), bc = midpoint(b, c), ca = midpoint(c, a);
            const int32_t four[12] = {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca};
            out.insert(out.end(), four, four + 12);
        }
        M.tri.swap(out);
    }
    const int nv = (int)(M.unit.size() / 3);
    std::vector<std::array<std::pair<int32_t, int32_t>, 6>> succ(nv);
    M.deg.assign(nv, 0);
    auto link = [&](int32_t i, int32_t p, int32_t q) { succ[i][M.deg[i]++] = std::make_pair(p, q); };      // a vertex of this mesh has 5 or 6
    for (size_t t = 0; t < M.tri.size(); t += 3) {
        const int32_t a = M.tri[t], b = M.tri[t + 1], c = M.tri[t + 2];
        link(a, b, c);
        link(b, c, a);
        link(c, a, b);
    }
    M.ring.assign((size_t)nv * 6, -1);
    for (int i = 0; i < nv; ++i) {
        int32_t p = succ[i][0].first;
        for (int k = 1; k < M.deg[i]; ++k) p = std::min(p, succ[i][k].first);
        for (int k = 0; k < M.deg[i]; ++k) {
            M.ring[(size_t)i * 6 + k] = p;
            for (int e = 0; e < M.deg[i]; ++e)
                if (succ[i][e].first == p) { p = succ[i][e].second; break; }
        }
    }
    return M;
}

int check_volume(int32_t nx, int32_t ny, int32_t nz, const double voxel_mm[3])
{
    if (nx < 0 || ny < 0 || nz < 0) return fail(MET2_E_INVALID, "bad shape");
    if (!voxel_mm) return fail(MET2_E_INVALID, "NULL voxel size");
    for (int a = 0; a < 3; ++a)
        if (!(voxel_mm[a] > 0.0) || !std::isfinite(voxel_mm[a])) return fail(MET2_E_INVALID, "the voxel size must be positive and finite");
    if ((int64_t)nx * ny * nz > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    return MET2_OK;
}

int check_surface(double f, int32_t level, int32_t n_iter)
{
    if (!(f > 0.0 && f < 1.0)) return fail(MET2_E_INVALID, "brain extraction needs 0 < f < 1");
    if (level < 0) return fail(MET2_E_INVALID, "the mesh level must not be negative");
    if (level > BET_MAX_LEVEL) return fail(MET2_E_UNSUPPORTED, "brain extraction supports mesh levels 0 to 4");
    if (n_iter < 0) return fail(MET2_E_INVALID, "the number of iterations must not be negative");
    return MET2_OK;
}

// the statistics of v (device) -> st[8] = t2, t, t98, tm, cog[3], r and the number of voxels above t; blocking
int stats_host(const double *v, const Grid &g, double st[8], int64_t *count, hipStream_t s)
{
    const int64_t n = (int64_t)g.nx * g.ny * g.nz;
    if (n == 0) return fail(MET2_E_INVALID, "brain extraction: the set v > t is empty (no voxel)");
    const int nch = (int)((n + BET_CHUNK - 1) / BET_CHUNK);
    DeviceWork W(s);
    const auto part = W.take<double>((size_t)4 * nch);                 // four rows of partials, which the kernels address at stride nch: one piece serves
    const auto pcnt = W.take<int32_t>(nch);
    const auto hist = W.take<uint32_t>(BET_NBINS);
    const auto res = W.take<unsigned long long>(2);
    if (!W.alloc()) return W.finish("met2_bet_stats");
    std::vector<double> hp((size_t)4 * nch);
    std::vector<int32_t> hc(nch);
    std::vector<uint32_t> hh(BET_NBINS);
    const dim3 T(256), GC(nch);

    hipLaunchKernelGGL(bet_range_kernel, GC, T, 0, s, v, n, part, part + nch, pcnt);
    W.ok(hipGetLastError());
    W.ok(hipMemcpyAsync(hp.data(), part, (size_t)2 * nch * 8, hipMemcpyDeviceToHost, s));
    W.ok(hipMemcpyAsync(hc.data(), pcnt, (size_t)nch * 4, hipMemcpyDeviceToHost, s));
    if (!W.ok(hipStreamSynchronize(s))) return W.finish("met2_bet_stats");
    double lo = INFINITY, hi = -INFINITY;
    int64_t N = 0;
    for (int c = 0; c < nch; ++c) {
        lo = std::fmin(lo, hp[c]);
        hi = std::fmax(hi, hp[nch + c]);
        N += hc[c];
    }
    if (N == 0 || !(hi > lo)) return fail(MET2_E_INVALID, "brain extraction: the set v > t is empty (no finite voxel, or a constant volume)");

    W.ok(hipMemsetAsync(hist, 0, hist.bytes, s));
    hipLaunchKernelGGL(bet_hist_kernel, GC, T, 0, s, v, n, lo, hi, hist);
    W.ok(hipGetLastError());
    W.ok(hipMemcpyAsync(hh.data(), hist, BET_NBINS * 4, hipMemcpyDeviceToHost, s));
    if (!W.ok(hipStreamSynchronize(s))) return W.finish("met2_bet_stats");
    int j2 = -1, j98 = -1;
    int64_t C = 0;
    for (int j = 0; j < BET_NBINS; ++j) {
        C += hh[j];
        if (j2 < 0 && 100 * C >= 2 * N) j2 = j;
        if (j98 < 0 && 100 * C >= 98 * N) j98 = j;
    }
    const double binw = (hi - lo) / (double)BET_NBINS;
    const double t2 = lo + (double)j2 * binw, t98 = lo + (double)(j98 + 1) * binw;
    const double t = t2 + 0.1 * (t98 - t2);

    hipLaunchKernelGGL(bet_cog_kernel, GC, T, 0, s, v, n, g, t, t2, t98, nch, part, pcnt);
    W.ok(hipGetLastError());
    W.ok(hipMemcpyAsync(hp.data(), part, (size_t)4 * nch * 8, hipMemcpyDeviceToHost, s));
    W.ok(hipMemcpyAsync(hc.data(), pcnt, (size_t)nch * 4, hipMemcpyDeviceToHost, s));
    if (!W.ok(hipStreamSynchronize(s))) return W.finish("met2_bet_stats");
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t cnt = 0;
    for (int c = 0; c < nch; ++c) {
        for (int q = 0; q < 4; ++q) sum[q] += hp[(size_t)q * nch + c];
        cnt += hc[c];
    }
    if (cnt == 0 || !(sum[0] > 0.0)) return fail(MET2_E_INVALID, "brain extraction: the set v > t is empty");
    Sphere sp;
    sp.cx = sum[1] / sum[0];
    sp.cy = sum[2] / sum[0];
    sp.cz = sum[3] / sum[0];
    const double vol = (double)cnt * ((g.dx * g.dy) * g.dz);
    const double r = std::cbrt(3.0 * vol / (4.0 * M_PI));
    sp.r2 = r * r;
    sp.t2 = t2;
    sp.t98 = t98;

    // the median by radix selection, one byte of the key at a time from the top; rank = the lower middle, counted from 0
    uint64_t decided = 0, prefix = 0;
    int64_t n_tm = 0, rank = 0;
    uint32_t h256[256];
    for (int shift = 56; shift >= 0 && W.ok(); shift -= 8) {
        W.ok(hipMemsetAsync(hist, 0, 256 * 4, s));
        hipLaunchKernelGGL(bet_select_kernel, GC, T, 0, s, v, n, g, sp, decided, prefix, shift, hist);
        W.ok(hipGetLastError());
        W.ok(hipMemcpyAsync(h256, hist, 256 * 4, hipMemcpyDeviceToHost, s));
        if (!W.ok(hipStreamSynchronize(s))) break;
        if (shift == 56) {
            for (int b = 0; b < 256; ++b) n_tm += h256[b];
            if (n_tm == 0) break;
            rank = (n_tm - 1) / 2;
        }
        int b = 0;
        while (b < 255 && rank >= (int64_t)h256[b]) rank -= h256[b++];
        prefix |= (uint64_t)b << shift;
        decided |= 0xffULL << shift;
    }
    double tm = t;                                                     // nothing to take the median of
    if (W.ok() && n_tm > 0) {
        auto value = [](uint64_t key) {
            const uint64_t bits = (key >> 63) ? key & 0x7fffffffffffffffULL : ~key;
            double x;
            std::memcpy(&x, &bits, 8);
            return x;
        };
        const double a = value(prefix);
        tm = a;
        if (n_tm % 2 == 0) {
            unsigned long long init[2] = {0ULL, ~0ULL}, got[2] = {0ULL, ~0ULL};
            W.ok(hipMemcpyAsync(res, init, 16, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(bet_upper_kernel, GC, T, 0, s, v, n, g, sp, prefix, res);
            W.ok(hipGetLastError());
            W.ok(hipMemcpyAsync(got, res, 16, hipMemcpyDeviceToHost, s));
            W.ok(hipStreamSynchronize(s));
            const int64_t k1 = (n_tm - 1) / 2 + 1;                     // the upper middle's rank
            const double b = (int64_t)got[0] > k1 ? a : value(got[1]);
            tm = (a + b) / 2.0;
        }
    }
    if (int rc = W.finish("met2_bet_stats")) return rc;
    st[0] = t2; st[1] = t; st[2] = t98; st[3] = tm; st[4] = sp.cx; st[5] = sp.cy; st[6] = sp.cz; st[7] = r;
    if (count) *count = cnt;
    return MET2_OK;
}

// n_iter steps from xin to xout (both device, [nv][3]; may be the same array); the mesh's tables go up and the call waits for the kernel
int evolve_host(const double *v, const Grid &g, const double st[8], double f, const Mesh &M, int32_t n_iter, const double *xin, double *xout,
                hipStream_t s)
{
    const int nv = M.nv();
    std::vector<int16_t> ring((size_t)nv * 6);
    int degsum = 0;
    for (int i = 0; i < nv; ++i) {
        degsum += M.deg[i];
        for (int k = 0; k < 6; ++k) ring[(size_t)i * 6 + k] = (int16_t)M.ring[(size_t)i * 6 + k];
    }
    DeviceWork W(s);
    const auto dring = W.take<int16_t>((size_t)nv * 6);
    if (!W.alloc()) return W.finish("met2_bet_evolve");
    EvolveArgs A;
    A.v = v;
    A.g = g;
    A.wx = 1.0 / g.dx; A.wy = 1.0 / g.dy; A.wz = 1.0 / g.dz;
    A.t2 = st[0]; A.t = st[1]; A.tm = st[3];
    A.E = (1.0 / BET_RMIN + 1.0 / BET_RMAX) / 2.0;
    A.F = 6.0 / (1.0 / BET_RMIN - 1.0 / BET_RMAX);
    A.bt = std::pow(f, 0.275);
    A.nv = nv; A.n_iter = n_iter; A.degsum = degsum;
    A.xin = xin; A.xout = xout;
    A.ring = dring;
    const int lds = 2 * 3 * nv * 8 + nv * 12;                          // positions and rings: 153 720 bytes at level 4, of the CU's 160 KiB
    W.ok(hipMemcpyAsync(dring, ring.data(), (size_t)nv * 12, hipMemcpyHostToDevice, s));
    W.ok(hipFuncSetAttribute((const void *)bet_evolve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    if (W.ok()) hipLaunchKernelGGL(bet_evolve_kernel, dim3(1), dim3(BET_T), lds, s, A);
    return W.finish("met2_bet_evolve");                                // waits: the host tables live until here
}

int fill_host(const Grid &g, int nv, const double *X, int ntri, const int32_t *tri, uint8_t *mask, hipStream_t s)
{
    const int64_t cols = (int64_t)g.nx * g.ny;
    if (cols == 0 || g.nz == 0) return MET2_OK;
    hipLaunchKernelGGL(bet_fill_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, X, nv, tri, ntri, g, mask);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

Grid make_grid(int32_t nx, int32_t ny, int32_t nz, const double voxel_mm[3])
{
    Grid g;
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.dx = voxel_mm[0]; g.dy = voxel_mm[1]; g.dz = voxel_mm[2];
    return g;
}

}  // namespace

extern "C" int met2_bet_mesh(int32_t level, double *unit_vertices, int32_t *triangles, int32_t *ring, int32_t *deg)
{
    if (level < 0) return fail(MET2_E_INVALID, "the mesh level must not be negative");
    if (level > BET_MAX_LEVEL) return fail(MET2_E_UNSUPPORTED, "brain extraction supports mesh levels 0 to 4");
    const Mesh M = build_mesh(level);
    if (unit_vertices) std::copy(M.unit.begin(), M.unit.end(), unit_vertices);
    if (triangles) std::copy(M.tri.begin(), M.tri.end(), triangles);
    if (ring) std::copy(M.ring.begin(), M.ring.end(), ring);
    if (deg) std::copy(M.deg.begin(), M.deg.end(), deg);
    return MET2_OK;
}

extern "C" int met2_bet_mean(int32_t device, int64_t nvox, int32_t n_te, const double *data, double *out, void *stream)
{
    if (nvox < 0 || n_te < 1) return fail(MET2_E_INVALID, "bad shape");
    if (nvox == 0) return MET2_OK;
    if (!data || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (nvox > 0x7fffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large");
    USE_DEVICE(device);
    hipLaunchKernelGGL(bet_mean_kernel, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, (hipStream_t)stream, data, nvox, n_te, out);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_bet_stats(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const double voxel_mm[3], double *stats_out,
                              int64_t *count_out, void *stream)
{
    if (int rc = check_volume(nx, ny, nz, voxel_mm)) return rc;
    if (!stats_out) return fail(MET2_E_INVALID, "NULL argument");
    if (!v && (int64_t)nx * ny * nz > 0) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    return stats_host(v, make_grid(nx, ny, nz, voxel_mm), stats_out, count_out, (hipStream_t)stream);
}

extern "C" int met2_bet_evolve(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const double voxel_mm[3], const double stats[8],
                               double f, int32_t level, int32_t n_iter, const double *vertices_in, double *vertices_out, void *stream)
{
    if (int rc = check_volume(nx, ny, nz, voxel_mm)) return rc;
    if (int rc = check_surface(f, level, n_iter)) return rc;
    if (!stats || !vertices_in || !vertices_out || !v) return fail(MET2_E_INVALID, "NULL argument");
    if ((int64_t)nx * ny * nz == 0) return fail(MET2_E_INVALID, "the surface evolution needs a volume of at least one voxel");
    USE_DEVICE(device);
    return evolve_host(v, make_grid(nx, ny, nz, voxel_mm), stats, f, build_mesh(level), n_iter, vertices_in, vertices_out, (hipStream_t)stream);
}

extern "C" int met2_bet_fill(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double voxel_mm[3], int32_t n_vertices, const double *vertices,
                             int32_t n_triangles, const int32_t *triangles, uint8_t *mask_out, void *stream)
{
    if (int rc = check_volume(nx, ny, nz, voxel_mm)) return rc;
    if (n_vertices < 0 || n_triangles < 0) return fail(MET2_E_INVALID, "bad mesh size");
    if ((int64_t)nx * ny * nz == 0) return MET2_OK;
    if (!mask_out || (n_triangles > 0 && (!triangles || !vertices))) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    return fill_host(make_grid(nx, ny, nz, voxel_mm), n_vertices, vertices, n_triangles, triangles, mask_out, (hipStream_t)stream);
}

extern "C" int met2_brain_mask(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double *v, const double voxel_mm[3], double f, int32_t level,
                               int32_t n_iter, uint8_t *mask_out, double *vertices_out, double *stats_out, void *stream)
{
    if (int rc = check_volume(nx, ny, nz, voxel_mm)) return rc;
    if (int rc = check_surface(f, level, n_iter)) return rc;
    if ((!v || !mask_out) && (int64_t)nx * ny * nz > 0) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    hipStream_t s = (hipStream_t)stream;
    const Grid g = make_grid(nx, ny, nz, voxel_mm);
    double st[8];
    if (int rc = stats_host(v, g, st, nullptr, s)) return rc;
    const Mesh M = build_mesh(level);
    const int nv = M.nv(), nt = M.nt();
    std::vector<double> x0((size_t)nv * 3);
    const double half = 0.5 * st[7];
    for (int i = 0; i < nv; ++i)
        for (int a = 0; a < 3; ++a) x0[(size_t)3 * i + a] = st[4 + a] + M.unit[(size_t)3 * i + a] * half;
    DeviceWork W(s);
    const auto X = W.take<double>((size_t)nv * 3);
    const auto tri = W.take<int32_t>((size_t)nt * 3);
    if (!W.alloc()) return W.finish("met2_brain_mask");
    W.ok(hipMemcpyAsync(X, x0.data(), (size_t)nv * 24, hipMemcpyHostToDevice, s));
    W.ok(hipMemcpyAsync(tri, M.tri.data(), (size_t)nt * 12, hipMemcpyHostToDevice, s));
    int rc = MET2_OK;
    if (W.ok()) rc = evolve_host(v, g, st, f, M, n_iter, X, X, s);                   // waits: x0 lives until here
    if (W.ok() && rc == MET2_OK) rc = fill_host(g, nv, X, nt, tri, mask_out, s);
    if (rc != MET2_OK) return rc;                                      // (the work space goes back behind a wait on this return too)
    if (W.ok() && vertices_out) W.ok(hipMemcpyAsync(vertices_out, X, (size_t)nv * 24, hipMemcpyDeviceToDevice, s));
    if (int e = W.finish("met2_brain_mask")) return e;
    if (stats_out) std::copy(st, st + 8, stats_out);
    return MET2_OK;
}
