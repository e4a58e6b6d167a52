// met2_gibbs.hip -- met2_degibbs: removal of Gibbs (truncation) ringing by local sub-voxel shifts (Kellner, Dhital, Kiselev, Reisert, MRM 2016;
// degibbs='yes'; step 2 of the reference's example pipeline, which runs MRtrix's mrdegibbs on the CPU).  include/met2_hip.h states the
// algorithm; no program text of MRtrix was used.  The volume is worked on in chunks of whole (z, echo) slices, slice-major [slice][nx][ny]:
//   gibbs_tables_kernel   per axis of length n: the DFT matrix W[b][q] = exp(-2 pi i b q / n) and the 2 nsh + 1 circular-convolution kernels
//                         c_j[r] of the sub-voxel shifts, laid out [r][j] (j padded to a multiple of GIBBS_JB with zeros) so that a wave reads
//                         the GIBBS_JB coefficients of one r with scalar loads;
//   gibbs_gather_kernel   caller's [nx][ny][slices] -> [slice][nx][ny] through a 32 x 32 LDS tile; flags the slices that hold a non-finite value;
//   gibbs_dft_rows_kernel T = S W_y               (real -> complex; GIBBS_LB rows per workgroup in LDS, one thread per output frequency)
//   gibbs_dft_cols_kernel T <- conj(W_x) ((W_x T) . Gx)   in place, GIBBS_LB columns per workgroup in LDS; keeps the corner Nyquist term of the slice
//   gibbs_idft_rows_kernel Ix = Re(T conj(W_y)) / (nx ny),  Iy = S - corner term - Ix     (Gx + Gy = 1 except at the corner, where both are 0)
//   gibbs_unring_kernel   the 1-D operator U on every line of one axis: the line twice over in LDS, each thread one sample; the shifted
//                         lines GIBBS_JB at a time as circular convolutions in registers (one LDS read per GIBBS_JB FMAs), handed to the
//                         neighbours through LDS for the windowed total variation; the running strict minimum with its three samples stays
//                         in registers; the y-pass adds into the x-pass's result;
//   gibbs_scatter_kernel  back to the caller's layout, non-finite slices copied through from the gathered input.
// met2_degibbs3d (degibbs='3d'; Bautista, O'Muircheartaigh, Hajnal, Tournier, ISMRM 2021) works in chunks of whole echo volumes, echo-major
// [echo][nx][ny][nz], with the same gather, tables, forward rows kernel (along z) and line kernel (along x, y and z by its strides), and
//   gibbs_dft_axis_kernel  the complex DFT along y or x, forward or back, in place;
//   gibbs_filter3d_kernel  F Gx and F Gy, the weight shared evenly where two or three axes sit at their Nyquist index;
//   gibbs_idft_z_kernel    back along z, real part, scaled; the third part as Iz = (V - Ix) - Iy;
//   gibbs_scatter3d_kernel gibbs_scatter_kernel with a third shift map.
// Every loop is bounded by a shape or a compile-time constant; fp64 throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_work.hpp"

namespace {

#define GIBBS_MIN_N 8
#define GIBBS_MAX_N 256
#define GIBBS_MAX_NSH 32
#define GIBBS_JB 7                        // shifted lines per pass of the convolution: 41 = 6 * 7 - 1 at the default nsh = 20
#define GIBBS_LB 8                        // lines per workgroup of the DFT kernels
#define GIBBS_CHUNK_ELEMS (1 << 22)       // samples per chunk of slices: 40 B of work space each

__global__ __launch_bounds__(256) void gibbs_tables_kernel(int n, int nsh, int jp, double2 *W, double *ct)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * n) {
        const int b = i / n, q = i - b * n;
        const int k = (b * q) % n;                                   // < 2^16
        double s, c;
        sincospi(2.0 * (double)k / (double)n, &s, &c);
        W[i] = make_double2(c, -s);
    }
    if (i < n * jp) {
        const int r = i / jp, j = i - r * jp;
        double v = 0.0;
        if (j < 2 * nsh + 1) {
            const int sh = j <= nsh ? j : nsh - j;
            const int64_t num = (int64_t)r * 2 * nsh + sh;           // (r + delta_j) 2 nsh;  2 pi k' (r + delta_j) / n = pi k' num / (nsh n)
            const int64_t per = (int64_t)2 * nsh * n;                // the cosine's period in k' num
            double sum = 0.0;
            for (int k = 1; k <= (n - 1) / 2; ++k) {
                int64_t a = ((int64_t)k * num) % per;
                if (a < 0) a += per;
                sum += cospi((double)a / (double)(nsh * n));
            }
            v = (1.0 + 2.0 * sum) / (double)n;
            if (j == 0 && n % 2 == 0) v += ((r & 1) ? -1.0 : 1.0) / (double)n;
        }
        ct[i] = v;
    }
}

__global__ __launch_bounds__(256) void gibbs_gather_kernel(const double *__restrict__ data, int64_t P, int64_t ns, int64_t s0, int sc,
                                                           double *__restrict__ W, int32_t *flag)
{
    __shared__ double tile[32][33];
    const int64_t p0 = (int64_t)blockIdx.x * 32;
    const int sb = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int64_t p = p0 + i;
        const int s = sb + threadIdx.x;
        if (p < P && s < sc) {
            const double v = data[p * ns + s0 + s];
            tile[i][threadIdx.x] = v;
            if (!isfinite(v)) flag[s] = 1;                            // every writer writes the same value
        }
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int s = sb + i;
        const int64_t p = p0 + threadIdx.x;
        if (s < sc && p < P) W[(int64_t)s * P + p] = tile[threadIdx.x][i];
    }
}

__global__ __launch_bounds__(256) void gibbs_scatter_kernel(const double *__restrict__ R, const double *__restrict__ W, const int8_t *__restrict__ sx,
                                                            const int8_t *__restrict__ sy, const int32_t *__restrict__ flag, int64_t P, int64_t ns,
                                                            int64_t s0, int sc, double *__restrict__ out, int8_t *__restrict__ ox,
                                                            int8_t *__restrict__ oy)
{
    __shared__ double tile[32][33];
    __shared__ int8_t tx8[32][33], ty8[32][33];
    const int64_t p0 = (int64_t)blockIdx.x * 32;
    const int sb = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int s = sb + i;
        const int64_t p = p0 + threadIdx.x;
        if (s < sc && p < P) {
            const bool copy = flag[s] != 0;                           // a slice with a non-finite value goes through unchanged
            const int64_t at = (int64_t)s * P + p;
            tile[i][threadIdx.x] = copy ? W[at] : R[at];
            if (ox) tx8[i][threadIdx.x] = copy ? (int8_t)0 : sx[at];
            if (oy) ty8[i][threadIdx.x] = copy ? (int8_t)0 : sy[at];
        }
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int64_t p = p0 + i;
        const int s = sb + threadIdx.x;
        if (p < P && s < sc) {
            const int64_t at = p * ns + s0 + s;
            out[at] = tile[threadIdx.x][i];
            if (ox) ox[at] = tx8[threadIdx.x][i];
            if (oy) oy[at] = ty8[threadIdx.x][i];
        }
    }
}

// T[g][q] = sum_b S[g][b] Wy[b][q] for the rows g of all slices of the chunk; blockDim.x >= ny
__global__ __launch_bounds__(256) void gibbs_dft_rows_kernel(const double *__restrict__ S, const double2 *__restrict__ Wy, int ny, int nrows,
                                                             double2 *__restrict__ T)
{
    __shared__ double xr[GIBBS_LB][GIBBS_MAX_N];
    const int g0 = blockIdx.x * GIBBS_LB;
    for (int i = threadIdx.x; i < GIBBS_LB * ny; i += blockDim.x) {
        const int l = i / ny, b = i - l * ny;
        xr[l][b] = g0 + l < nrows ? S[(int64_t)(g0 + l) * ny + b] : 0.0;
    }
    __syncthreads();
    const int q = threadIdx.x;
    if (q >= ny) return;
    double re[GIBBS_LB], im[GIBBS_LB];
#pragma unroll
    for (int l = 0; l < GIBBS_LB; ++l) { re[l] = 0.0; im[l] = 0.0; }
    for (int b = 0; b < ny; ++b) {
        const double2 w = Wy[b * ny + q];
#pragma unroll
        for (int l = 0; l < GIBBS_LB; ++l) {
            const double v = xr[l][b];
            re[l] = fma(v, w.x, re[l]);
            im[l] = fma(v, w.y, im[l]);
        }
    }
#pragma unroll
    for (int l = 0; l < GIBBS_LB; ++l)
        if (g0 + l < nrows) T[(int64_t)(g0 + l) * ny + q] = make_double2(re[l], im[l]);
}

// per slice and GIBBS_LB columns: F = W_x T, F *= Gx, T <- conj(W_x) F; blockDim.x >= nx; grid (ceil(ny / LB), slices)
__global__ __launch_bounds__(256) void gibbs_dft_cols_kernel(double2 *__restrict__ T, const double2 *__restrict__ Wx, const double2 *__restrict__ Wy,
                                                             int nx, int ny, double *__restrict__ corner)
{
    __shared__ double2 tc[GIBBS_LB][GIBBS_MAX_N];
    const int q0 = blockIdx.x * GIBBS_LB;
    const int s = blockIdx.y;
    double2 *Ts = T + (int64_t)s * nx * ny;
    for (int i = threadIdx.x; i < GIBBS_LB * nx; i += blockDim.x) {
        const int a = i / GIBBS_LB, l = i - a * GIBBS_LB;
        tc[l][a] = q0 + l < ny ? Ts[a * ny + q0 + l] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    const int p = threadIdx.x;
    const bool mine = p < nx;
    double re[GIBBS_LB], im[GIBBS_LB];
#pragma unroll
    for (int l = 0; l < GIBBS_LB; ++l) { re[l] = 0.0; im[l] = 0.0; }
    if (mine) {
        for (int a = 0; a < nx; ++a) {
            const double2 w = Wx[a * nx + p];
#pragma unroll
            for (int l = 0; l < GIBBS_LB; ++l) {
                const double2 t = tc[l][a];
                re[l] = fma(t.x, w.x, fma(-t.y, w.y, re[l]));
                im[l] = fma(t.x, w.y, fma(t.y, w.x, im[l]));
            }
        }
        const double cx = 1.0 + Wx[nx + p].x;                          // 1 + cos(2 pi p / nx); exactly 0 at p = nx / 2
#pragma unroll
        for (int l = 0; l < GIBBS_LB; ++l) {
            const int q = q0 + l;
            if (q < ny) {
                const double cy = 1.0 + Wy[ny + q].x;
                const double den = cx + cy;
                const double gx = den == 0.0 ? 0.0 : cy / den;
                if (2 * p == nx && 2 * q == ny) corner[s] = re[l];
                re[l] *= gx;
                im[l] *= gx;
            }
        }
    }
    __syncthreads();
    if (mine) {
#pragma unroll
        for (int l = 0; l < GIBBS_LB; ++l) tc[l][p] = make_double2(re[l], im[l]);
    }
    __syncthreads();
    if (!mine) return;
    const int a = p;
#pragma unroll
    for (int l = 0; l < GIBBS_LB; ++l) { re[l] = 0.0; im[l] = 0.0; }
    for (int pp = 0; pp < nx; ++pp) {
        const double2 w = Wx[pp * nx + a];                            // conjugated below
#pragma unroll
        for (int l = 0; l < GIBBS_LB; ++l) {
            const double2 t = tc[l][pp];
            re[l] = fma(t.x, w.x, fma(t.y, w.y, re[l]));
            im[l] = fma(t.y, w.x, fma(-t.x, w.y, im[l]));
        }
    }
#pragma unroll
    for (int l = 0; l < GIBBS_LB; ++l)
        if (q0 + l < ny) Ts[a * ny + q0 + l] = make_double2(re[l], im[l]);
}

// Ix[g][b] = Re sum_q T[g][q] conj(Wy[q][b]) / (nx ny);  Iy = S - corner / (nx ny) (-1)^(a + b) - Ix
__global__ __launch_bounds__(256) void gibbs_idft_rows_kernel(const double2 *__restrict__ T, const double2 *__restrict__ Wy, const double *__restrict__ S,
                                                              const double *__restrict__ corner, int nx, int ny, int nrows, double *__restrict__ Ix,
                                                              double *__restrict__ Iy)
{
    __shared__ double2 vr[GIBBS_LB][GIBBS_MAX_N];
    const int g0 = blockIdx.x * GIBBS_LB;
    for (int i = threadIdx.x; i < GIBBS_LB * ny; i += blockDim.x) {
        const int l = i / ny, q = i - l * ny;
        vr[l][q] = g0 + l < nrows ? T[(int64_t)(g0 + l) * ny + q] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    const int b = threadIdx.x;
    if (b >= ny) return;
    double re[GIBBS_LB];
#pragma unroll
    for (int l = 0; l < GIBBS_LB; ++l) re[l] = 0.0;
    for (int q = 0; q < ny; ++q) {
        const double2 w = Wy[q * ny + b];
#pragma unroll
        for (int l = 0; l < GIBBS_LB; ++l) {
            const double2 t = vr[l][q];
            re[l] = fma(t.x, w.x, fma(t.y, w.y, re[l]));
        }
    }
    const double scale = 1.0 / ((double)nx * (double)ny);
#pragma unroll
    for (int l = 0; l < GIBBS_LB; ++l) {
        const int g = g0 + l;
        if (g < nrows) {
            const int s = g / nx, a = g - s * nx;
            const int64_t at = (int64_t)g * ny + b;
            const double ix = re[l] * scale;
            const double cn = corner[s] * scale;
            Ix[at] = ix;
            Iy[at] = S[at] - (((a + b) & 1) ? -cn : cn) - ix;
        }
    }
}

struct UnringArgs {
    const double *src;        // [slices][nx][ny]
    const double *ct;         // [n][jp]
    double *dst;              // [slices][nx][ny]
    int8_t *shift;            // [slices][nx][ny] or NULL
    int n;                    // the line's length
    int nlines;               // lines in the chunk
    int per_slice;            // lines per slice
    int64_t slice_stride;     // nx ny
    int line_stride;          // between the first samples of a slice's consecutive lines
    int stride;               // between a line's samples
    int nsh, jp, min_w, max_w;
    int accumulate;           // dst += U(src) instead of dst = U(src)
    double *best;             // [slices][nx][ny] or NULL: the winning candidate's total variation (met2_gibbs_lines)
};

// one sample per thread, 256 / n lines per workgroup (one at n > 128)
__global__ __launch_bounds__(256) void gibbs_unring_kernel(UnringArgs A)
{
    __shared__ double xl[2 * GIBBS_MAX_N];                              // every line twice over: x[(m - r) mod n] = xl[base + m + n - r]
    __shared__ double xs[GIBBS_JB][GIBBS_MAX_N];                         // the pass's shifted lines, by thread
    const int n = A.n;
    const int lpb = 256 / n;
    const int t = threadIdx.x;
    const int li = t / n, m = t - li * n;
    const int line = blockIdx.x * lpb + li;
    const bool active = li < lpb && line < A.nlines;
    int64_t base = 0;
    if (active) {
        const int s = line / A.per_slice, o = line - s * A.per_slice;
        base = (int64_t)s * A.slice_stride + (int64_t)o * A.line_stride + (int64_t)m * A.stride;
    }
    const int lb = active ? li * 2 * n : 0;                             // an idle thread walks line 0's copy and writes nothing
    const int tb = active ? li * n : 0;
    if (active) {
        const double v = A.src[base];
        xl[lb + m] = v;
        xl[lb + n + m] = v;
    }
    __syncthreads();

    const int nj = 2 * A.nsh + 1;
    double best = INFINITY, a0 = 0.0, a1 = 0.0, a2 = 0.0;
    int jbest = 0;
    const int mm = active ? m : 0;
    const int ml = mm == 0 ? n - 1 : mm - 1, mr = mm == n - 1 ? 0 : mm + 1;
    const double *xp = xl + lb + mm + n;
    for (int j0 = 0; j0 < nj; j0 += GIBBS_JB) {
        double acc[GIBBS_JB];
#pragma unroll
        for (int jj = 0; jj < GIBBS_JB; ++jj) acc[jj] = 0.0;
        const double *__restrict__ cr = A.ct + j0;
#pragma unroll 4
        for (int r = 0; r < n; ++r) {
            const double xv = xp[-r];
#pragma unroll
            for (int jj = 0; jj < GIBBS_JB; ++jj) acc[jj] = fma(cr[r * A.jp + jj], xv, acc[jj]);
        }
        __syncthreads();                                              // the previous pass's readers are done
#pragma unroll
        for (int jj = 0; jj < GIBBS_JB; ++jj) xs[jj][t] = acc[jj];
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < GIBBS_JB; ++jj) {
            if (j0 + jj < nj) {                                        // uniform
                const double *xj = xs[jj] + tb;
                double tvl = 0.0, tvr = 0.0;
                for (int w = A.min_w; w <= A.max_w; ++w) {             // 2 (max_w + 1) <= n: one wrap at most
                    int i1 = mm - w, i0 = mm - w - 1, k0 = mm + w, k1 = mm + w + 1;
                    if (i1 < 0) i1 += n;
                    if (i0 < 0) i0 += n;
                    if (k0 >= n) k0 -= n;
                    if (k1 >= n) k1 -= n;
                    tvl += fabs(xj[i1] - xj[i0]);
                    tvr += fabs(xj[k1] - xj[k0]);
                }
                if (tvl < best) { best = tvl; jbest = j0 + jj; a0 = xj[ml]; a1 = acc[jj]; a2 = xj[mr]; }
                if (tvr < best) { best = tvr; jbest = j0 + jj; a0 = xj[ml]; a1 = acc[jj]; a2 = xj[mr]; }
            }
        }
    }
    if (!active) return;
    const int sh = jbest <= A.nsh ? jbest : A.nsh - jbest;
    const double d = (double)sh / (double)(2 * A.nsh);
    const double o = d > 0.0 ? a1 * (1.0 - d) + a0 * d : a1 * (1.0 + d) - a2 * d;
    A.dst[base] = A.accumulate ? A.dst[base] + o : o;
    if (A.shift) A.shift[base] = (int8_t)sh;
    if (A.best) A.best[base] = best;                                    // uniform
}

// ---- met2_degibbs3d: the 3-D split.  The work layout is echo-major [echo][nx][ny][nz], z fastest: gibbs_gather_kernel makes it from the
// caller's [nx ny nz][echoes] as it is (its "slice" is then an echo volume), the z lines are contiguous, gibbs_dft_rows_kernel is the forward
// DFT along z and gibbs_unring_kernel runs along all three axes by its strides.

// The DFT along an axis whose samples lie `stride` apart, in place and unscaled: T[o][a][i], o < nouter, a < n, i < stride; inverse != 0 takes
// the conjugate matrix.  GIBBS_LB adjacent i per workgroup, through LDS both ways so that global memory is touched 128 B at a time;
// blockDim.x >= n; grid nouter * ceil(stride / GIBBS_LB), the tile of i fastest
__global__ __launch_bounds__(256) void gibbs_dft_axis_kernel(double2 *__restrict__ T, const double2 *__restrict__ Wa, int n, int stride, int inverse)
{
    __shared__ double2 tc[GIBBS_LB][GIBBS_MAX_N + 1];                    // the odd row keeps the tile's GIBBS_LB lines on different banks
    const int tiles = (stride + GIBBS_LB - 1) / GIBBS_LB;
    const int o = blockIdx.x / tiles;
    const int i0 = (blockIdx.x - o * tiles) * GIBBS_LB;
    double2 *To = T + (int64_t)o * n * stride + i0;
    for (int i = threadIdx.x; i < GIBBS_LB * n; i += blockDim.x) {
        const int a = i / GIBBS_LB, l = i - a * GIBBS_LB;
        tc[l][a] = i0 + l < stride ? To[(int64_t)a * stride + l] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    const int p = threadIdx.x;
    const bool mine = p < n;
    double re[GIBBS_LB], im[GIBBS_LB];
#pragma unroll
    for (int l = 0; l < GIBBS_LB; ++l) { re[l] = 0.0; im[l] = 0.0; }
    if (mine) {
        for (int a = 0; a < n; ++a) {
            const double2 w = Wa[a * n + p];
            const double wy = inverse ? -w.y : w.y;
#pragma unroll
            for (int l = 0; l < GIBBS_LB; ++l) {
                const double2 t = tc[l][a];
                re[l] = fma(t.x, w.x, fma(-t.y, wy, re[l]));
                im[l] = fma(t.x, wy, fma(t.y, w.x, im[l]));
            }
        }
    }
    __syncthreads();
    if (mine) {
#pragma unroll
        for (int l = 0; l < GIBBS_LB; ++l) tc[l][p] = make_double2(re[l], im[l]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < GIBBS_LB * n; i += blockDim.x) {
        const int a = i / GIBBS_LB, l = i - a * GIBBS_LB;
        if (i0 + l < stride) To[(int64_t)a * stride + l] = tc[l][a];
    }
}

// A = F Gx, F <- F Gy over the chunk's [echo][p][q][r]; where two or three of cx, cy, cz are 0 the weight is shared evenly among those axes
__global__ __launch_bounds__(256) void gibbs_filter3d_kernel(double2 *__restrict__ F, double2 *__restrict__ A, const double2 *__restrict__ Wx,
                                                             const double2 *__restrict__ Wy, const double2 *__restrict__ Wz, int nx, int ny, int nz,
                                                             int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int r = (int)(i % nz);
    const int64_t g = i / nz;
    const int q = (int)(g % ny);
    const int p = (int)((g / ny) % nx);
    const double cx = 2 * p == nx ? 0.0 : 1.0 + Wx[nx + p].x;              // 1 + cos(2 pi p / nx)
    const double cy = 2 * q == ny ? 0.0 : 1.0 + Wy[ny + q].x;
    const double cz = 2 * r == nz ? 0.0 : 1.0 + Wz[nz + r].x;
    const double wx = cy * cz, wy = cx * cz;
    const double den = wx + wy + cx * cy;
    double gx, gy;
    if (den != 0.0) {
        gx = wx / den;
        gy = wy / den;
    } else {
        const double share = 1.0 / (double)((cx == 0.0) + (cy == 0.0) + (cz == 0.0));
        gx = cx == 0.0 ? share : 0.0;
        gy = cy == 0.0 ? share : 0.0;
    }
    const double2 f = F[i];
    A[i] = make_double2(f.x * gx, f.y * gx);
    F[i] = make_double2(f.x * gy, f.y * gy);
}

// I[g][b] = scale Re sum_r T[g][r] conj(Wz[r][b]) for the z lines g of the chunk; with Iz, also Iz = (V - Ix) - I; blockDim.x >= nz
__global__ __launch_bounds__(256) void gibbs_idft_z_kernel(const double2 *__restrict__ T, const double2 *__restrict__ Wz, int nz, int nrows,
                                                           double scale, double *__restrict__ I, const double *__restrict__ V,
                                                           const double *__restrict__ Ix, double *__restrict__ Iz)
{
    __shared__ double2 vr[GIBBS_LB][GIBBS_MAX_N];
    const int g0 = blockIdx.x * GIBBS_LB;
    for (int i = threadIdx.x; i < GIBBS_LB * nz; i += blockDim.x) {
        const int l = i / nz, r = i - l * nz;
        vr[l][r] = g0 + l < nrows ? T[(int64_t)(g0 + l) * nz + r] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    const int b = threadIdx.x;
    if (b >= nz) return;
    double re[GIBBS_LB];
#pragma unroll
    for (int l = 0; l < GIBBS_LB; ++l) re[l] = 0.0;
    for (int r = 0; r < nz; ++r) {
        const double2 w = Wz[r * nz + b];
#pragma unroll
        for (int l = 0; l < GIBBS_LB; ++l) {
            const double2 t = vr[l][r];
            re[l] = fma(t.x, w.x, fma(t.y, w.y, re[l]));
        }
    }
#pragma unroll
    for (int l = 0; l < GIBBS_LB; ++l) {
        if (g0 + l < nrows) {
            const int64_t at = (int64_t)(g0 + l) * nz + b;
            const double v = re[l] * scale;
            I[at] = v;
            if (Iz) Iz[at] = (V[at] - Ix[at]) - v;                       // uniform
        }
    }
}

// gibbs_scatter_kernel with a third shift map: [echo][P] back to the caller's [P][echoes]; a flagged echo volume is copied through from W
__global__ __launch_bounds__(256) void gibbs_scatter3d_kernel(const double *__restrict__ R, const double *__restrict__ W, const int8_t *__restrict__ sx,
                                                              const int8_t *__restrict__ sy, const int8_t *__restrict__ sz,
                                                              const int32_t *__restrict__ flag, int64_t P, int64_t ns, int64_t s0, int sc,
                                                              double *__restrict__ out, int8_t *__restrict__ ox, int8_t *__restrict__ oy,
                                                              int8_t *__restrict__ oz)
{
    __shared__ double tile[32][33];
    __shared__ int8_t tx8[32][33], ty8[32][33], tz8[32][33];
    const int64_t p0 = (int64_t)blockIdx.x * 32;
    const int sb = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int s = sb + i;
        const int64_t p = p0 + threadIdx.x;
        if (s < sc && p < P) {
            const bool copy = flag[s] != 0;
            const int64_t at = (int64_t)s * P + p;
            tile[i][threadIdx.x] = copy ? W[at] : R[at];
            if (ox) tx8[i][threadIdx.x] = copy ? (int8_t)0 : sx[at];
            if (oy) ty8[i][threadIdx.x] = copy ? (int8_t)0 : sy[at];
            if (oz) tz8[i][threadIdx.x] = copy ? (int8_t)0 : sz[at];
        }
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int64_t p = p0 + i;
        const int s = sb + threadIdx.x;
        if (p < P && s < sc) {
            const int64_t at = p * ns + s0 + s;
            out[at] = tile[threadIdx.x][i];
            if (ox) ox[at] = tx8[threadIdx.x][i];
            if (oy) oy[at] = ty8[threadIdx.x][i];
            if (oz) oz[at] = tz8[threadIdx.x][i];
        }
    }
}

inline int round64(int n) { return (n + 63) / 64 * 64; }

inline int table_cols(int nshifts) { return (2 * nshifts + 1 + GIBBS_JB - 1) / GIBBS_JB * GIBBS_JB; }

// the checks on an axis' tables and on the operator U that every entry shares; MET2_OK or the code already recorded by fail()
int check_shifts(int32_t nshifts)
{
    if (nshifts < 1) return fail(MET2_E_INVALID, "degibbs needs at least one sub-voxel shift");
    if (nshifts > GIBBS_MAX_NSH) return fail(MET2_E_UNSUPPORTED, "degibbs supports at most 32 sub-voxel shifts to a side");
    return MET2_OK;
}

int check_windows(int32_t min_w, int32_t max_w)
{
    if (min_w < 1 || min_w > max_w) return fail(MET2_E_INVALID, "degibbs needs 1 <= minW <= maxW");
    return MET2_OK;
}

void launch_tables(hipStream_t st, int n, int nshifts, int jp, double2 *W, double *ct)
{
    const int big = n * (n > jp ? n : jp);
    hipLaunchKernelGGL(gibbs_tables_kernel, dim3((big + 255) / 256), dim3(256), 0, st, n, nshifts, jp, W, ct);
}

void launch_unring(hipStream_t st, const UnringArgs &A)
{
    hipLaunchKernelGGL(gibbs_unring_kernel, dim3((A.nlines + 256 / A.n - 1) / (256 / A.n)), dim3(256), 0, st, A);
}

// The volume in chunks of whole slices.  split_x == NULL: the filter (out, shift_x, shift_y as met2_degibbs takes them).  Otherwise the 2-D
// split alone: Ix and Iy of every slice go to split_x and split_y, whatever the slice holds.  The shapes and parameters have been checked.
int run_volume(int32_t device, int32_t nx, int32_t ny, int64_t ns, const double *data, int32_t nshifts, int32_t min_w, int32_t max_w, double *out,
               int8_t *shift_x, int8_t *shift_y, double *split_x, double *split_y, void *stream, const char *who)
{
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;

    const int64_t P = (int64_t)nx * ny;
    int64_t scl = GIBBS_CHUNK_ELEMS / P;
    if (scl < 1) scl = 1;
    if (scl > ns) scl = ns;
    if (scl > 65535) scl = 65535;                                      // the column kernel's grid.y
    const int sc_max = (int)scl;
    const int jp = table_cols(nshifts);
    const size_t ce = (size_t)sc_max * (size_t)P;                      // samples of a chunk
    DeviceWork work(st);
    const auto W = work.take<double>(ce);
    const auto T = work.take<double2>(ce);
    const auto Ix = work.take<double>(ce), Iy = work.take<double>(ce);
    const auto sx = work.take<int8_t>(ce), sy = work.take<int8_t>(ce);
    const auto corner = work.take<double>(sc_max);
    const auto flag = work.take<int32_t>((size_t)sc_max * 2);           // sc_max flags in a piece as large as the corner terms': one memset clears both
    const auto Wx = work.take<double2>((size_t)nx * nx), Wy = work.take<double2>((size_t)ny * ny);
    const auto cx = work.take<double>((size_t)nx * jp), cy = work.take<double>((size_t)ny * jp);
    if (!work.alloc()) return work.finish(who);

    launch_tables(st, nx, nshifts, jp, Wx, cx);
    launch_tables(st, ny, nshifts, jp, Wy, cy);
    work.ok(hipGetLastError());
    for (int64_t s0 = 0; s0 < ns && work.ok(); s0 += sc_max) {
        const int sc = (int)(ns - s0 < sc_max ? ns - s0 : sc_max);
        const int nrows = sc * nx;
        if (!work.ok(hipMemsetAsync(corner, 0, 2 * corner.bytes, st))) break;    // the corner terms and the flags lie side by side
        const dim3 tg((unsigned)((P + 31) / 32), (unsigned)((sc + 31) / 32));
        hipLaunchKernelGGL(gibbs_gather_kernel, tg, dim3(32, 8), 0, st, data, P, ns, s0, sc, W, flag);
        hipLaunchKernelGGL(gibbs_dft_rows_kernel, dim3((nrows + GIBBS_LB - 1) / GIBBS_LB), dim3(round64(ny)), 0, st, W, Wy, ny, nrows, T);
        hipLaunchKernelGGL(gibbs_dft_cols_kernel, dim3((ny + GIBBS_LB - 1) / GIBBS_LB, sc), dim3(round64(nx)), 0, st, T, Wx, Wy, nx, ny, corner);
        hipLaunchKernelGGL(gibbs_idft_rows_kernel, dim3((nrows + GIBBS_LB - 1) / GIBBS_LB), dim3(round64(ny)), 0, st, T, Wy, W, corner, nx, ny,
                           nrows, Ix, Iy);
        if (split_x) {                                                  // source and copy-through source the same: the flags change nothing
            hipLaunchKernelGGL(gibbs_scatter_kernel, tg, dim3(32, 8), 0, st, Ix, Ix, sx, sy, flag, P, ns, s0, sc, split_x, (int8_t *)nullptr,
                               (int8_t *)nullptr);
            hipLaunchKernelGGL(gibbs_scatter_kernel, tg, dim3(32, 8), 0, st, Iy, Iy, sx, sy, flag, P, ns, s0, sc, split_y, (int8_t *)nullptr,
                               (int8_t *)nullptr);
            work.ok(hipGetLastError());
            continue;
        }
        UnringArgs A;
        A.nsh = nshifts; A.jp = jp; A.min_w = min_w; A.max_w = max_w; A.slice_stride = P; A.best = nullptr;
        // along x: the lines are a slice's columns; the result overwrites Ix
        A.src = Ix; A.dst = Ix; A.ct = cx; A.shift = shift_x ? (int8_t *)sx : nullptr; A.n = nx; A.nlines = sc * ny; A.per_slice = ny; A.line_stride = 1;
        A.stride = ny; A.accumulate = 0;
        launch_unring(st, A);
        // along y: the rows; added to the x-pass's result
        A.src = Iy; A.dst = Ix; A.ct = cy; A.shift = shift_y ? (int8_t *)sy : nullptr; A.n = ny; A.nlines = nrows; A.per_slice = nx; A.line_stride = ny;
        A.stride = 1; A.accumulate = 1;
        launch_unring(st, A);
        hipLaunchKernelGGL(gibbs_scatter_kernel, tg, dim3(32, 8), 0, st, Ix, W, sx, sy, flag, P, ns, s0, sc, out, shift_x, shift_y);
        work.ok(hipGetLastError());
    }
    return work.finish(who);
}

// the checks on the volume's shape that met2_degibbs and met2_gibbs_split share, after those of the parameters; *empty: nothing to do
int check_volume(int32_t nx, int32_t ny, int32_t nz, int32_t nt, int64_t min_axis, bool *empty)
{
    const int64_t ns = (int64_t)nz * nt;
    *empty = nx == 0 || ny == 0 || ns == 0;
    if (*empty) return MET2_OK;
    if (nx < GIBBS_MIN_N || nx > GIBBS_MAX_N || ny < GIBBS_MIN_N || ny > GIBBS_MAX_N)
        return fail(MET2_E_UNSUPPORTED, "degibbs supports 8 to 256 samples along x and y");
    if (min_axis > (nx < ny ? nx : ny)) return fail(MET2_E_UNSUPPORTED, "the total-variation window is too wide for the axis");
    return MET2_OK;
}

// The volume in chunks of whole echo volumes, [echo][nx][ny][nz].  split_x == NULL: the 3-D filter (out and the three shift maps as
// met2_degibbs3d takes them).  Otherwise the 3-D split alone: Ix, Iy, Iz of every echo go to split_x, split_y, split_z, whatever the echo
// holds.  The shapes and parameters have been checked.
int run_volume3d(int32_t device, int32_t nx, int32_t ny, int32_t nz, int64_t nt, const double *data, int32_t nshifts, int32_t min_w, int32_t max_w,
                 double *out, int8_t *shift_x, int8_t *shift_y, int8_t *shift_z, double *split_x, double *split_y, double *split_z, void *stream,
                 const char *who)
{
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;

    const int64_t P = (int64_t)nx * ny * nz;
    int64_t ecl = GIBBS_CHUNK_ELEMS / P;
    if (ecl < 1) ecl = 1;
    if (ecl > nt) ecl = nt;
    const int ec_max = (int)ecl;                                       // at most 2^22 / 8^3 echoes
    const int jp = table_cols(nshifts);
    const size_t ce = (size_t)ec_max * (size_t)P;                      // samples of a chunk
    const int32_t na[3] = {nx, ny, nz};
    DeviceWork work(st);
    const auto W = work.take<double>(ce);
    const auto T = work.take<double2>(ce), T2 = work.take<double2>(ce);
    const auto Ix = work.take<double>(ce), Iy = work.take<double>(ce), Iz = work.take<double>(ce);
    const auto sx = work.take<int8_t>(ce), sy = work.take<int8_t>(ce), sz = work.take<int8_t>(ce);
    const auto flag = work.take<int32_t>(ec_max);
    DeviceWork::Piece<double2> Wa[3];
    DeviceWork::Piece<double> ca[3];
    for (int a = 0; a < 3; ++a) {
        Wa[a] = work.take<double2>((size_t)na[a] * na[a]);
        ca[a] = work.take<double>((size_t)na[a] * jp);
    }
    if (!work.alloc()) return work.finish(who);

    for (int a = 0; a < 3; ++a) launch_tables(st, na[a], nshifts, jp, Wa[a], ca[a]);
    work.ok(hipGetLastError());
    const int yz = ny * nz;                                            // <= 2^16
    const int tiles_x = (yz + GIBBS_LB - 1) / GIBBS_LB, tiles_y = (nz + GIBBS_LB - 1) / GIBBS_LB;
    const double scale = 1.0 / ((double)nx * (double)ny * (double)nz);
    for (int64_t e0 = 0; e0 < nt && work.ok(); e0 += ec_max) {
        const int ec = (int)(nt - e0 < ec_max ? nt - e0 : ec_max);
        const int64_t cs = (int64_t)ec * P;                            // < 2^31
        const int nrows = (int)(cs / nz);                              // the chunk's z lines
        if (!work.ok(hipMemsetAsync(flag, 0, flag.bytes, st))) break;
        const dim3 tg((unsigned)((P + 31) / 32), (unsigned)((ec + 31) / 32));
        const dim3 rows((unsigned)((nrows + GIBBS_LB - 1) / GIBBS_LB));
        const dim3 gx((unsigned)((int64_t)ec * tiles_x)), gy((unsigned)((int64_t)ec * nx * tiles_y));    // <= 2^22 / 8 + ec and 2^22 / 64 + ec nx
        hipLaunchKernelGGL(gibbs_gather_kernel, tg, dim3(32, 8), 0, st, data, P, nt, e0, ec, W, flag);
        hipLaunchKernelGGL(gibbs_dft_rows_kernel, rows, dim3(round64(nz)), 0, st, W, Wa[2], nz, nrows, T);
        hipLaunchKernelGGL(gibbs_dft_axis_kernel, gy, dim3(round64(ny)), 0, st, T, Wa[1], ny, nz, 0);
        hipLaunchKernelGGL(gibbs_dft_axis_kernel, gx, dim3(round64(nx)), 0, st, T, Wa[0], nx, yz, 0);
        hipLaunchKernelGGL(gibbs_filter3d_kernel, dim3((unsigned)((cs + 255) / 256)), dim3(256), 0, st, T, T2, Wa[0], Wa[1], Wa[2], nx, ny, nz, cs);
        hipLaunchKernelGGL(gibbs_dft_axis_kernel, gx, dim3(round64(nx)), 0, st, T2, Wa[0], nx, yz, 1);
        hipLaunchKernelGGL(gibbs_dft_axis_kernel, gy, dim3(round64(ny)), 0, st, T2, Wa[1], ny, nz, 1);
        hipLaunchKernelGGL(gibbs_idft_z_kernel, rows, dim3(round64(nz)), 0, st, T2, Wa[2], nz, nrows, scale, Ix, (const double *)nullptr,
                           (const double *)nullptr, (double *)nullptr);
        hipLaunchKernelGGL(gibbs_dft_axis_kernel, gx, dim3(round64(nx)), 0, st, T, Wa[0], nx, yz, 1);
        hipLaunchKernelGGL(gibbs_dft_axis_kernel, gy, dim3(round64(ny)), 0, st, T, Wa[1], ny, nz, 1);
        hipLaunchKernelGGL(gibbs_idft_z_kernel, rows, dim3(round64(nz)), 0, st, T, Wa[2], nz, nrows, scale, Iy, W, Ix, Iz);
        if (split_x) {                                                  // source and copy-through source the same: the flags change nothing
            double *src[3] = {Ix, Iy, Iz}, *dst[3] = {split_x, split_y, split_z};
            for (int a = 0; a < 3; ++a)
                hipLaunchKernelGGL(gibbs_scatter_kernel, tg, dim3(32, 8), 0, st, src[a], src[a], sx, sy, flag, P, nt, e0, ec, dst[a],
                                   (int8_t *)nullptr, (int8_t *)nullptr);
            work.ok(hipGetLastError());
            continue;
        }
        UnringArgs A;
        A.nsh = nshifts; A.jp = jp; A.min_w = min_w; A.max_w = max_w; A.best = nullptr; A.dst = Ix;
        // along x: per echo, the ny nz lines start side by side; the result overwrites Ix
        A.src = Ix; A.ct = ca[0]; A.shift = shift_x ? (int8_t *)sx : nullptr; A.n = nx; A.nlines = ec * yz; A.per_slice = yz; A.slice_stride = P;
        A.line_stride = 1; A.stride = yz; A.accumulate = 0;
        launch_unring(st, A);
        // along y: per (echo, x), the nz lines start side by side; added to the x pass's result
        A.src = Iy; A.ct = ca[1]; A.shift = shift_y ? (int8_t *)sy : nullptr; A.n = ny; A.nlines = ec * nx * nz; A.per_slice = nz; A.slice_stride = yz;
        A.line_stride = 1; A.stride = nz; A.accumulate = 1;
        launch_unring(st, A);
        // along z: the lines are contiguous, one after the other through the chunk
        A.src = Iz; A.ct = ca[2]; A.shift = shift_z ? (int8_t *)sz : nullptr; A.n = nz; A.nlines = nrows; A.per_slice = nrows; A.slice_stride = 0;
        A.line_stride = nz; A.stride = 1; A.accumulate = 1;
        launch_unring(st, A);
        hipLaunchKernelGGL(gibbs_scatter3d_kernel, tg, dim3(32, 8), 0, st, Ix, W, sx, sy, sz, flag, P, nt, e0, ec, out, shift_x, shift_y, shift_z);
        work.ok(hipGetLastError());
    }
    return work.finish(who);
}

// the checks on the volume's shape that met2_degibbs3d and met2_gibbs_split3d share, after those of the parameters; *empty: nothing to do
int check_volume3d(int32_t nx, int32_t ny, int32_t nz, int32_t nt, int64_t min_axis, bool *empty)
{
    *empty = nx == 0 || ny == 0 || nz == 0 || nt == 0;
    if (*empty) return MET2_OK;
    const int32_t lo = nx < ny ? (nx < nz ? nx : nz) : (ny < nz ? ny : nz), hi = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
    if (lo < GIBBS_MIN_N || hi > GIBBS_MAX_N) return fail(MET2_E_UNSUPPORTED, "degibbs in 3-D supports 8 to 256 samples along x, y and z");
    if (min_axis > lo) return fail(MET2_E_UNSUPPORTED, "the total-variation window is too wide for the axis");
    return MET2_OK;
}

}  // namespace

extern "C" int met2_degibbs3d(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t nt, const double *data, int32_t nshifts, int32_t min_w,
                              int32_t max_w, double *out, int8_t *shift_x, int8_t *shift_y, int8_t *shift_z, void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0 || nt < 0) return fail(MET2_E_INVALID, "bad shape");
    if (nshifts < 1) return fail(MET2_E_INVALID, "degibbs needs at least one sub-voxel shift");
    if (int rc = check_windows(min_w, max_w)) return rc;
    if (int rc = check_shifts(nshifts)) return rc;
    bool empty;
    if (int rc = check_volume3d(nx, ny, nz, nt, 2 * ((int64_t)max_w + 1), &empty)) return rc;
    if (empty) return MET2_OK;
    if (!data || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (data == out) return fail(MET2_E_INVALID, "degibbs cannot run in place");
    if (nt > 0x7fffffffLL / ((int64_t)nx * ny * nz)) return fail(MET2_E_UNSUPPORTED, "volume too large");
    return run_volume3d(device, nx, ny, nz, nt, data, nshifts, min_w, max_w, out, shift_x, shift_y, shift_z, nullptr, nullptr, nullptr, stream,
                        "met2_degibbs3d");
}

extern "C" int met2_gibbs_split3d(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t nt, const double *data, double *ix, double *iy,
                                  double *iz, void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0 || nt < 0) return fail(MET2_E_INVALID, "bad shape");
    bool empty;
    if (int rc = check_volume3d(nx, ny, nz, nt, GIBBS_MIN_N, &empty)) return rc;
    if (empty) return MET2_OK;
    if (!data || !ix || !iy || !iz) return fail(MET2_E_INVALID, "NULL argument");
    if (data == ix || data == iy || data == iz || ix == iy || ix == iz || iy == iz) return fail(MET2_E_INVALID, "the split cannot run in place");
    if (nt > 0x7fffffffLL / ((int64_t)nx * ny * nz)) return fail(MET2_E_UNSUPPORTED, "volume too large");
    return run_volume3d(device, nx, ny, nz, nt, data, 1, 1, 1, nullptr, nullptr, nullptr, nullptr, ix, iy, iz, stream, "met2_gibbs_split3d");
}

extern "C" int met2_degibbs(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t nt, const double *data, int32_t nshifts, int32_t min_w,
                            int32_t max_w, double *out, int8_t *shift_x, int8_t *shift_y, void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0 || nt < 0) return fail(MET2_E_INVALID, "bad shape");
    if (nshifts < 1) return fail(MET2_E_INVALID, "degibbs needs at least one sub-voxel shift");
    if (int rc = check_windows(min_w, max_w)) return rc;
    if (int rc = check_shifts(nshifts)) return rc;
    bool empty;
    if (int rc = check_volume(nx, ny, nz, nt, 2 * ((int64_t)max_w + 1), &empty)) return rc;
    if (empty) return MET2_OK;
    if (!data || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (data == out) return fail(MET2_E_INVALID, "degibbs cannot run in place");
    const int64_t ns = (int64_t)nz * nt;
    if (ns > 0x7fffffffLL / ((int64_t)nx * ny)) return fail(MET2_E_UNSUPPORTED, "volume too large");
    return run_volume(device, nx, ny, ns, data, nshifts, min_w, max_w, out, shift_x, shift_y, nullptr, nullptr, stream, "met2_degibbs");
}

extern "C" int met2_gibbs_table_cols(int32_t nshifts)
{
    if (int rc = check_shifts(nshifts)) return rc;
    return table_cols(nshifts);
}

extern "C" int met2_gibbs_tables(int32_t device, int32_t n, int32_t nshifts, double *W, double *c, void *stream)
{
    if (int rc = check_shifts(nshifts)) return rc;
    if (n < GIBBS_MIN_N || n > GIBBS_MAX_N) return fail(MET2_E_UNSUPPORTED, "degibbs supports 8 to 256 samples along x and y");
    if (!W || !c) return fail(MET2_E_INVALID, "NULL argument");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    launch_tables(st, n, nshifts, table_cols(nshifts), (double2 *)W, c);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_gibbs_split(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t nt, const double *data, double *ix, double *iy,
                                void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0 || nt < 0) return fail(MET2_E_INVALID, "bad shape");
    bool empty;
    if (int rc = check_volume(nx, ny, nz, nt, GIBBS_MIN_N, &empty)) return rc;
    if (empty) return MET2_OK;
    if (!data || !ix || !iy) return fail(MET2_E_INVALID, "NULL argument");
    if (data == ix || data == iy || ix == iy) return fail(MET2_E_INVALID, "the split cannot run in place");
    const int64_t ns = (int64_t)nz * nt;
    if (ns > 0x7fffffffLL / ((int64_t)nx * ny)) return fail(MET2_E_UNSUPPORTED, "volume too large");
    return run_volume(device, nx, ny, ns, data, 1, 1, 1, nullptr, nullptr, nullptr, ix, iy, stream, "met2_gibbs_split");
}

extern "C" int met2_gibbs_lines(int32_t device, int32_t n, int32_t nlines, const double *lines, int32_t nshifts, int32_t min_w, int32_t max_w,
                                double *out, int8_t *shift, double *best, void *stream)
{
    if (n < 0 || nlines < 0) return fail(MET2_E_INVALID, "bad shape");
    if (int rc = check_shifts(nshifts)) return rc;
    if (int rc = check_windows(min_w, max_w)) return rc;
    if (n == 0 || nlines == 0) return MET2_OK;
    if (n < GIBBS_MIN_N || n > GIBBS_MAX_N) return fail(MET2_E_UNSUPPORTED, "degibbs supports 8 to 256 samples along x and y");
    if (2 * ((int64_t)max_w + 1) > n) return fail(MET2_E_UNSUPPORTED, "the total-variation window is too wide for the axis");
    if (!lines || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (lines == out) return fail(MET2_E_INVALID, "degibbs cannot run in place");
    if (nlines > 0x7fffffffLL / n) return fail(MET2_E_UNSUPPORTED, "volume too large");
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const int jp = table_cols(nshifts);
    DeviceWork work(st);
    const auto W = work.take<double2>((size_t)n * n);
    const auto ct = work.take<double>((size_t)n * jp);
    if (!work.alloc()) return work.finish("met2_gibbs_lines");
    launch_tables(st, n, nshifts, jp, W, ct);
    UnringArgs A;
    A.nsh = nshifts; A.jp = jp; A.min_w = min_w; A.max_w = max_w; A.slice_stride = 0; A.best = best;
    A.src = lines; A.dst = out; A.ct = ct; A.shift = shift; A.n = n; A.nlines = nlines; A.per_slice = nlines; A.line_stride = n;
    A.stride = 1; A.accumulate = 0;
    launch_unring(st, A);
    return work.finish("met2_gibbs_lines");
}
