// met2_mppca.hip -- met2_mppca: Marchenko-Pastur PCA denoising of a multi-echo volume (Veraart et al., NeuroImage 2016; denoise='MPPCA').
// An extension: the reference has no such filter.  include/met2_hip.h states the algorithm; this file holds
//   mppca_kernel   one wave (one workgroup of 64 lanes) per voxel, voxels in memory order so that neighbouring patches meet in L2:
//     1. the patch list: the lanes test the mask of the window's positions, 64 at a time, and the set ones are compacted into LDS in
//        memory order (ballot + prefix count);
//     2. the Gram matrix C = X X^T by rank-1 updates in registers: lane j owns column j, acc[i] += x_i x_j with x_i read from lane i
//        (v_readlane); C[i][j] and C[j][i] see the same products in the same order, so C is symmetric to the bit;
//     3. a parallel-ordered (round-robin) cyclic Jacobi on C with the eigenvectors V accumulated, both in the wave's LDS region: each of
//        the n - 1 steps of a sweep rotates the floor(M / 2) disjoint pairs of a tournament round -- lane k forms pair k's rotation, then
//        the rows, then the columns of C and V are rotated with the lanes over the columns / rows, floor(64 / M) pairs side by side.
//        A pair with |c_pq| <= eps sqrt(c_pp c_qq) is left alone (the root is taken of the product while that is finite and normal, of the
//        factors otherwise, so that the test holds at every scale at which C is finite); a sweep that rotates nothing ends the solver,
//        MET2_MPPCA_MAX_SWEEPS ends it otherwise (rank -2);
//     4. the ascending order of the eigenvalues by counting (lane i counts the eigenvalues before its own), the threshold rule with the
//        cumulative sum taken in the stated order, and the projection on the kept eigenvectors.
// Every loop is bounded by a shape or a compile-time constant.  fp64 throughout; division and square root are IEEE.
// mppca_kernel<true> (met2_mppca_stages) is the same code that also copies what each step leaves to global memory, and takes its sweep cap
// from the caller; mppca_kernel<false> is what met2_mppca launches.
// mppca_kernel<false, 1> (met2_mppca_box, average = 0) is the same code once more with the window's three half-widths in place of the cube's
// one, over a box of centres (there: the whole volume).  mppca_kernel<false, 2> (average = 1) writes nothing of the outputs: per centre it leaves a 24-byte head
// (rank, N, sigma, where its vectors are) and the k kept eigenvectors, k n_te doubles taken from a pool by one atomic add per centre, vector j
// (ascending eigenvalue) at doubles [j n_te, (j + 1) n_te) of them -- where a centre's vectors lie depends on the order the waves arrive in,
// what they hold does not --, and
//   mppca_average_kernel   one wave per output voxel, lanes along the echoes: it walks the masked centres of the voxel's clipped box in memory
//     order, and for every centre that votes forms p = sum_j u_j (u_j . x_v), j ascending, each dot product by wave_ops.hpp's wave_sum (the DPP
//     row reduction, then rows (0 + 1) + (2 + 3)), and acc = fma(w_c, p, acc), wsum += w_c, ssum = fma(w_c, sigma_c, ssum).  No atomics, no
//     scatter: a voxel's result depends on the heads and vectors it reads and on nothing else, so it is the same for every tiling.
// The host side cuts the volume into boxes of output voxels whose centres (the box widened by the half-widths, clipped) fit the work space:
// whole (y, z) planes while one fits, else whole z lines of one plane, else runs of one line.  The fit is reckoned at MET2_MPPCA_RANK_GUESS
// vectors per centre; a box whose centres keep more than the pool holds (the kernel writes nothing past it, the host reads the count) is
// halved and run again, down to one voxel, whose centres fit at any rank.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
#include "device_helpers.hpp"
#include "device_work.hpp"
#include "wave_ops.hpp"

namespace {

#define MET2_MPPCA_MAX_TE 63        // one echo per lane, and a dummy player for odd n_te
#define MET2_MPPCA_MAX_SWEEPS 30    // 7-8 sweeps at 32 echoes with more patch voxels than echoes, 10-14 with fewer (a null space to clean up)
#define MET2_MPPCA_LDS_MAX 65536    // dynamic LDS a launch may ask for without opting in to more

struct MppcaArgs {
    int nx, ny, nz, nt, win;
    int ld;                         // leading dimension of C and V in LDS: odd, so that a column walk is free of bank conflicts
    const double *data;
    const uint8_t *mask;
    double *out, *sigma;
    int32_t *rank;
};

struct MppcaStageArgs : MppcaArgs {  // what mppca_kernel<true> writes beside; each may be NULL
    int max_sweeps;
    int32_t *n_patch, *patch, *sweeps;
    double *gram, *eigval, *eigvec;
};

struct MppcaHead {                   // what averaging mode keeps of a centre beside its vectors; a centre votes if rank >= 0 and n >= 2
    int32_t rank, n;
    double sigma;
    int64_t at;                      // its vectors start at this double of the pool (rank > 0 only; -1: the pool was full)
};

struct MppcaBoxArgs : MppcaArgs {    // mppca_kernel<false, 1> and <false, 2>: win is unused
    int hx, hy, hz;                  // the window's half-widths
    int cx0, cy0, cz0, cny, cnz;     // the box of centres the launch covers: block b is the centre at (b / (cny cnz), (b / cnz) % cny, b % cnz) of it
    int32_t *n_patch;                // may be NULL
    MppcaHead *head;                 // <false, 2> only: [centres of the box]; out, sigma, rank and n_patch are then not written
    double *basis;                   // the pool of `pool` doubles, `used` counts what the centres of this launch have taken
    int64_t pool;
    unsigned long long *used;
};

template <bool STAGES, int BOX = 0> struct mppca_args { typedef MppcaArgs type; };      // BOX: 0 the cube, 1 a box, 2 a box whose centres are kept
template <> struct mppca_args<true, 0> { typedef MppcaStageArgs type; };
template <> struct mppca_args<false, 1> { typedef MppcaBoxArgs type; };
template <> struct mppca_args<false, 2> { typedef MppcaBoxArgs type; };

// pair k of round t of the round-robin tournament over n players (n even): player n - 1 stays, the others turn
__device__ __forceinline__ void rr_pair(int n, int t, int k, int &p, int &q)
{
    const int m = n - 1;
    int a = t + k;  if (a >= m) a -= m;
    int b = t - k;  if (b < 0) b += m;
    p = k == 0 ? m : a;
    q = b;
}

template <bool STAGES, int BOX> __device__ __forceinline__ int sweep_cap(const typename mppca_args<STAGES, BOX>::type &A)
{
    if constexpr (STAGES) return A.max_sweeps;
    else return MET2_MPPCA_MAX_SWEEPS;
}

// the voxel a block works on: block b in memory order, or the centre at b of a box launch
template <int BOX, class Args> __device__ __forceinline__ int64_t centre_voxel(const Args &A)
{
    if constexpr (BOX != 0) {
        const int b = (int)blockIdx.x;
        const int lz = b % A.cnz, ly = (b / A.cnz) % A.cny, lx = b / (A.cnz * A.cny);
        return ((int64_t)(A.cx0 + lx) * A.ny + (A.cy0 + ly)) * A.nz + (A.cz0 + lz);
    } else return blockIdx.x;
}

size_t aux_bytes(size_t wtot)
{
    const size_t list = wtot * sizeof(int32_t);
    const size_t need = list > 1024 ? list : 1024;       // the patch list, then the rotations' (c, s) [32 + 32], then the sorted spectrum [64]
    return (need + 15) / 16 * 16;
}

template <bool STAGES, int BOX = 0>
__global__ __launch_bounds__(64) void mppca_kernel(typename mppca_args<STAGES, BOX>::type A)
{
    extern __shared__ __attribute__((aligned(16))) double mppca_lds[];
    const int M = A.nt, LD = A.ld;
    double *C = mppca_lds;
    double *V = C + (size_t)M * LD;
    double *aux = V + (size_t)M * LD;
    int32_t *list = reinterpret_cast<int32_t *>(aux);
    const int lane = met2::lane_id();
    const int64_t v = centre_voxel<BOX>(A);
    const bool mine = lane < M;
    double *ov = A.out + v * M;

    if (A.mask && A.mask[v] == 0) {
        if constexpr (BOX == 2) {
            if (lane == 0) A.head[blockIdx.x] = MppcaHead{0, 0, 0.0, 0};
            return;
        }
        if (mine) ov[lane] = 0.0;
        if (lane == 0) { if (A.sigma) A.sigma[v] = 0.0; if (A.rank) A.rank[v] = 0; }
        if constexpr (STAGES || BOX == 1) { if (A.n_patch && lane == 0) A.n_patch[v] = 0; }
        return;
    }
    const int vz = (int)(v % A.nz), vy = (int)((v / A.nz) % A.ny), vx = (int)(v / ((int64_t)A.nz * A.ny));
    int hx, hy, hz;
    if constexpr (BOX != 0) { hx = A.hx; hy = A.hy; hz = A.hz; }
    else hx = hy = hz = A.win / 2;
    const int x0 = max(vx - hx, 0), y0 = max(vy - hy, 0), z0 = max(vz - hz, 0);
    const int wx = min(vx + hx + 1, A.nx) - x0, wy = min(vy + hy + 1, A.ny) - y0, wz = min(vz + hz + 1, A.nz) - z0;
    const int wtot = wx * wy * wz;                                   // <= the window's voxel count: the list's room

    // 1. the patch list, in memory order
    int N = 0;
    for (int base = 0; base < wtot; base += 64) {
        const int i = base + lane;
        int64_t pv = 0;
        bool in = false;
        if (i < wtot) {
            const int dz = i % wz, dy = (i / wz) % wy, dx = i / (wz * wy);
            pv = ((int64_t)(x0 + dx) * A.ny + (y0 + dy)) * A.nz + (z0 + dz);
            in = !A.mask || A.mask[pv] != 0;
        }
        const met2::u64 b = met2::ballot(in);
        if (in) list[N + __popcll(b & ((1ull << lane) - 1ull))] = (int32_t)(pv - v);      // |offset| < 2^31: the host checks the volume
        N += __popcll(b);
    }
    wave_lds_sync();
    if constexpr (STAGES) {                                           // the list as it stands, before aux is taken for anything else
        if (A.n_patch && lane == 0) A.n_patch[v] = N;
        if (A.patch)
            for (int i = lane; i < N; i += 64) A.patch[v * ((int64_t)A.win * A.win * A.win) + i] = list[i];
    }
    if constexpr (BOX == 1) { if (A.n_patch && lane == 0) A.n_patch[v] = N; }
    const double xc = mine ? A.data[v * M + lane] : 0.0;

    // 2. the Gram matrix, column `lane` in registers
    double acc[MET2_MPPCA_MAX_TE];
#pragma unroll
    for (int i = 0; i < MET2_MPPCA_MAX_TE; ++i) acc[i] = 0.0;
    bool finite = true;
    for (int n = 0; n < N; n += 2) {                                  // two patch voxels per trip: their loads are in flight together
        const int o0 = __builtin_amdgcn_readfirstlane(list[n]);
        const int o1 = __builtin_amdgcn_readfirstlane(list[n + 1 < N ? n + 1 : n]);
        const double xa = mine ? A.data[(v + o0) * M + lane] : 0.0;
        double xb = mine ? A.data[(v + o1) * M + lane] : 0.0;
        finite = finite && isfinite(xa) && isfinite(xb);
        if (n + 1 >= N) xb = 0.0;
#pragma unroll
        for (int i = 0; i < MET2_MPPCA_MAX_TE; ++i)
            if (i < M) {
                acc[i] = fma(met2::bcast(xa, i), xa, acc[i]);
                acc[i] = fma(met2::bcast(xb, i), xb, acc[i]);
            }
    }
    int rank = 0;
    int64_t at = 0;                                                   // (<false, 2> only)
    double sig = 0.0, res = xc;                                       // the copy-through cases leave the voxel as it is
    if (met2::ballot(!finite) != 0ull) rank = -1;
    else if (N < 2) rank = 1;
    else {
#pragma unroll
        for (int i = 0; i < MET2_MPPCA_MAX_TE; ++i)
            if (i < M && mine) { C[i * LD + lane] = acc[i]; V[i * LD + lane] = i == lane ? 1.0 : 0.0; }
        wave_lds_sync();
        if constexpr (STAGES) {
            if (A.gram && mine)
                for (int i = 0; i < M; ++i) A.gram[(v * M + i) * M + lane] = C[i * LD + lane];
        }

        // 3. Jacobi
        const int n = M + (M & 1), np = n / 2;
        const int G = 64 / M;                                          // pairs rotated side by side
        const int g = lane / M, j = lane - g * M;
        const bool work = g < G;
        double *cc = aux, *ss = aux + 32;
        const double dsum = met2::wave_sum(mine ? C[lane * LD + lane] : 0.0);
        const double floor_abs = dsum * 0x1p-80;                       // below this an entry is rounding dust of forming C
        // The rotation test's threshold is eps sqrt(|c_pp c_qq|) while that product is finite and normal, eps sqrt|c_pp| sqrt|c_qq| otherwise: it
        // neither overflows nor vanishes while C is finite.  Every |c_pp| is at most the trace (C is positive semidefinite), so below a trace of
        // 2^500 no product overflows; and from a trace of 2^-480 on, a product below DBL_MIN has eps times its root (by either formula, at most
        // 2^-563) below floor_abs (at least 2^-560), so that `off > floor_abs` decides alone.  Between the two the plain root is the whole test.
        const bool extreme = __builtin_amdgcn_readfirstlane(!(dsum >= 0x1p-480 && dsum < 0x1p500) ? 1 : 0) != 0;
        bool converged = false;
        const int max_sweeps = sweep_cap<STAGES, BOX>(A);
        int sweep = 0;
        if (!(dsum <= DBL_MAX)) { rank = -1; converged = true; }      // C overflowed on finite data: wave-uniform, copied through
        for (; sweep < max_sweeps && !converged; ++sweep) {
            int nrot = 0;
            for (int t = 0; t < n - 1; ++t) {
                int p = 0, q = 0;
                bool rot = false;
                double app = 0.0, aqq = 0.0, apq = 0.0, tt = 0.0;
                if (lane < np) {
                    rr_pair(n, t, lane, p, q);
                    if (p < M && q < M) {
                        app = C[p * LD + p]; aqq = C[q * LD + q]; apq = C[p * LD + q];
                        const double off = fabs(apq);
                        const double pr = fabs(app * aqq);
                        double gm = sqrt(pr);
                        if (__builtin_expect(extreme, 0) && !(pr <= DBL_MAX && pr >= DBL_MIN)) gm = sqrt(fabs(app)) * sqrt(fabs(aqq));
                        rot = !(off <= DBL_EPSILON * gm) && off > floor_abs;
                    }
                    double c = 1.0, s = 0.0;
                    if (rot) {
                        const double th = (aqq - app) / (2.0 * apq);
                        tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                        c = 1.0 / sqrt(tt * tt + 1.0);
                        s = tt * c;
                    }
                    cc[lane] = c; ss[lane] = s;
                }
                const met2::u64 rm = met2::ballot(rot);
                if (rm == 0ull) continue;                              // wave-uniform
                nrot += __popcll(rm);
                wave_lds_sync();
                // rows p, q of C: lanes over the columns
                for (int kk = 0; kk < np; kk += G) {
                    const int k = kk + g;
                    if (work && k < np && ((rm >> k) & 1ull)) {
                        int pp, qq;
                        rr_pair(n, t, k, pp, qq);
                        const double c = cc[k], s = ss[k];
                        const double a = C[pp * LD + j], b = C[qq * LD + j];
                        C[pp * LD + j] = c * a - s * b;
                        C[qq * LD + j] = s * a + c * b;
                    }
                }
                wave_lds_sync();
                // columns p, q of C and of V: lanes over the rows
                for (int kk = 0; kk < np; kk += G) {
                    const int k = kk + g;
                    if (work && k < np && ((rm >> k) & 1ull)) {
                        int pp, qq;
                        rr_pair(n, t, k, pp, qq);
                        const double c = cc[k], s = ss[k];
                        const double a = C[j * LD + pp], b = C[j * LD + qq];
                        const double va = V[j * LD + pp], vb = V[j * LD + qq];
                        C[j * LD + pp] = c * a - s * b;
                        C[j * LD + qq] = s * a + c * b;
                        V[j * LD + pp] = c * va - s * vb;
                        V[j * LD + qq] = s * va + c * vb;
                    }
                }
                wave_lds_sync();
                if (rot) {                                             // the rotated pair's 2 x 2 block in closed form: the off-diagonal is zero
                    C[p * LD + p] = app - tt * apq;
                    C[q * LD + q] = aqq + tt * apq;
                    C[p * LD + q] = 0.0;
                    C[q * LD + p] = 0.0;
                }
                wave_lds_sync();
            }
            converged = nrot == 0;
        }
        if constexpr (STAGES) {
            if (A.sweeps && lane == 0) A.sweeps[v] = sweep;
            if (A.eigval && mine) A.eigval[v * M + lane] = C[lane * LD + lane];
            if (A.eigvec && mine)
                for (int i = 0; i < M; ++i) A.eigvec[(v * M + i) * M + lane] = V[i * LD + lane];
        }
        if (!converged) rank = -2;
        else if (rank == 0) {
            // 4. order, threshold, projection
            const int r = min(M, N), qn = max(M, N);
            const double d = mine ? C[lane * LD + lane] : 0.0;
            int pos = 0;                                               // eigenvalues before this lane's in ascending order (ties by index)
            for (int i = 0; i < M; ++i) {
                const double di = met2::bcast(d, i);
                pos += (di < d || (di == d && i < lane)) ? 1 : 0;
            }
            wave_lds_sync();                                           // (cc, ss are dead: the spectrum takes their room)
            double *lamv = aux;
            if (mine && pos >= M - r) lamv[pos - (M - r)] = fmax(d, 0.0) / (double)qn;
            wave_lds_sync();
            const double lam = lane < r ? lamv[lane] : 0.0;
            const double lam0 = met2::bcast(lam, 0);
            double clam = 0.0, run = 0.0;
            for (int i = 0; i < r; ++i) {                              // the cumulative sum in the stated order
                run += met2::bcast(lam, i);
                if (i == lane) clam = run;
            }
            const double gamma = (double)(lane + 1) / (double)qn;
            const double s1 = clam / (double)(lane + 1);
            const double s2 = (lam - lam0) / (4.0 * sqrt(gamma));
            const met2::u64 below = met2::ballot(lane < r && s2 < s1);
            const int cut = below ? 64 - __builtin_clzll(below) : 0;
            const double sigma2 = cut ? met2::bcast(s1, cut - 1) : 0.0;
            const int k = r - cut;
            if constexpr (BOX == 2) {
                if (k > 0) {                                // the kept eigenvectors, ascending, where the pool has room for them
                    unsigned long long got = 0;
                    if (lane == 0) got = atomicAdd(A.used, (unsigned long long)(k * M));
                    at = (int64_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(got >> 32)) << 32) |
                                   (unsigned)__builtin_amdgcn_readfirstlane((int)got));
                    if (at + k * M <= A.pool) {
                        double *B = A.basis + at;
                        for (int jv = 0; jv < k; ++jv) {
                            const int src = met2::first_lane(met2::ballot(mine && pos == M - k + jv));
                            if (mine) B[jv * M + lane] = V[lane * LD + src];
                        }
                    } else at = -1;
                }
            }
            if constexpr (BOX != 2) {                       // (the averaging kernel projects on the exported vectors instead)
                // coefficients on the kept eigenvectors (lane = eigenvector), then the expansion (lane = echo)
                double coef = 0.0;
                for (int e = 0; e < M; ++e) {
                    const double xe = met2::bcast(xc, e);
                    if (mine) coef = fma(V[e * LD + lane], xe, coef);
                }
                if (!(mine && pos >= M - k)) coef = 0.0;
                double o = 0.0;
                for (int c = 0; c < M; ++c) {
                    const double cf = met2::bcast(coef, c);
                    if (mine) o = fma(V[lane * LD + c], cf, o);
                }
                res = o;
            }
            sig = sqrt(sigma2);
            rank = k;
        }
    }
    if constexpr (BOX == 2) {
        if (lane == 0) A.head[blockIdx.x] = MppcaHead{rank, N, sig, at};
        return;
    }
    if (mine) ov[lane] = res;
    if (lane == 0) { if (A.sigma) A.sigma[v] = sig; if (A.rank) A.rank[v] = rank; }
}

struct MppcaAvgArgs {
    int nx, ny, nz, nt;
    int hx, hy, hz;
    int ox0, oy0, oz0, ony, onz;     // the box of output voxels: block b is the voxel at (b / (ony onz), (b / onz) % ony, b % onz) of it
    int cx0, cy0, cz0, cny, cnz;     // the box of centres head and basis hold: the output box widened by the half-widths, clipped
    const double *data;
    const uint8_t *mask;
    const MppcaHead *head;
    const double *basis;
    double *out, *sigma, *wsum;
    int32_t *rank, *n_patch;
};

__global__ __launch_bounds__(64) void mppca_average_kernel(MppcaAvgArgs A)
{
    const int M = A.nt;
    const int lane = met2::lane_id();
    const bool mine = lane < M;
    const int b = (int)blockIdx.x;
    const int vx = A.ox0 + b / (A.onz * A.ony), vy = A.oy0 + (b / A.onz) % A.ony, vz = A.oz0 + b % A.onz;
    const int64_t v = ((int64_t)vx * A.ny + vy) * A.nz + vz;
    double *ov = A.out + v * M;
    if (A.mask && A.mask[v] == 0) {
        if (mine) ov[lane] = 0.0;
        if (lane == 0) {
            if (A.sigma) A.sigma[v] = 0.0;
            if (A.rank) A.rank[v] = 0;
            if (A.n_patch) A.n_patch[v] = 0;
            if (A.wsum) A.wsum[v] = 0.0;
        }
        return;
    }
    const double x = mine ? A.data[v * M + lane] : 0.0;
    const int x0 = max(vx - A.hx, 0), y0 = max(vy - A.hy, 0), z0 = max(vz - A.hz, 0);
    const int x1 = min(vx + A.hx + 1, A.nx), y1 = min(vy + A.hy + 1, A.ny), z1 = min(vz + A.hz + 1, A.nz);
    double acc = 0.0, wsum = 0.0, ssum = 0.0;
    for (int cx = x0; cx < x1; ++cx)
        for (int cy = y0; cy < y1; ++cy)
            for (int cz = z0; cz < z1; ++cz) {                         // everything that steers this loop is wave-uniform
                if (A.mask && __builtin_amdgcn_readfirstlane((int)A.mask[((int64_t)cx * A.ny + cy) * A.nz + cz]) == 0) continue;
                const int64_t lc = ((int64_t)(cx - A.cx0) * A.cny + (cy - A.cy0)) * A.cnz + (cz - A.cz0);
                const MppcaHead hd = A.head[lc];
                const int k = __builtin_amdgcn_readfirstlane(hd.rank), n = __builtin_amdgcn_readfirstlane(hd.n);
                if (k < 0 || n < 2) continue;                          // a copy-through class: no vote
                const double w = 1.0 / (double)(1 + k);
                const double *B = A.basis + (((int64_t)__builtin_amdgcn_readfirstlane((int)(hd.at >> 32)) << 32) |
                                             (unsigned)__builtin_amdgcn_readfirstlane((int)hd.at));
                double p = 0.0;
                for (int j = 0; j < k; ++j) {
                    const double u = mine ? B[j * M + lane] : 0.0;
                    const double d = met2::wave_sum(u * x);
                    p = fma(u, d, p);
                }
                acc = fma(w, p, acc);
                wsum += w;
                ssum = fma(w, hd.sigma, ssum);
            }
    const int64_t lv = ((int64_t)(vx - A.cx0) * A.cny + (vy - A.cy0)) * A.cnz + (vz - A.cz0);
    const MppcaHead own = A.head[lv];
    const bool voted = wsum > 0.0;
    if (mine) ov[lane] = voted ? acc / wsum : x;
    if (lane == 0) {
        if (A.sigma) A.sigma[v] = voted ? ssum / wsum : 0.0;
        if (A.rank) A.rank[v] = own.rank;
        if (A.n_patch) A.n_patch[v] = own.n;
        if (A.wsum) A.wsum[v] = wsum;
    }
}

}  // namespace

template <bool STAGES>
static int mppca_launch(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t nt, const double *data, const uint8_t *mask, int32_t window,
                        double *out, double *sigma, int32_t *rank, void *stream, typename mppca_args<STAGES>::type A)
{
    if (nx < 0 || ny < 0 || nz < 0) return fail(MET2_E_INVALID, "bad shape");
    if (window < 3 || window % 2 == 0) return fail(MET2_E_INVALID, "the MP-PCA window must be odd and at least 3");
    if (nt < 2 || nt > MET2_MPPCA_MAX_TE) return fail(MET2_E_UNSUPPORTED, "MP-PCA supports 2 to 63 echoes");
    const int ld = nt | 1;
    const size_t wcap = window > 63 ? 63 : window;
    const size_t lds = 2 * sizeof(double) * (size_t)nt * ld + aux_bytes(wcap * wcap * wcap);
    if (window > 63 || lds > MET2_MPPCA_LDS_MAX) return fail(MET2_E_UNSUPPORTED, "the MP-PCA window's patch list does not fit in LDS beside the two matrices");
    const int64_t nvox = (int64_t)nx * ny * nz;
    if (nvox == 0) return MET2_OK;
    if (!data || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (data == out) return fail(MET2_E_INVALID, "MP-PCA cannot run in place");
    if (nvox > 0x3ffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large for one launch");
    USE_DEVICE(device);
    A.nx = nx; A.ny = ny; A.nz = nz; A.nt = nt; A.win = window; A.ld = ld;
    A.data = data; A.mask = mask; A.out = out; A.sigma = sigma; A.rank = rank;
    hipLaunchKernelGGL(mppca_kernel<STAGES>, dim3((unsigned)nvox), dim3(64), lds, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return MET2_OK;
}

extern "C" int met2_mppca(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t nt, const double *data, const uint8_t *mask,
                          int32_t window, double *out, double *sigma, int32_t *rank, void *stream)
{
    return mppca_launch<false>(device, nx, ny, nz, nt, data, mask, window, out, sigma, rank, stream, MppcaArgs());
}

extern "C" int met2_mppca_stages(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t nt, const double *data, const uint8_t *mask,
                                 int32_t window, double *out, double *sigma, int32_t *rank, int32_t max_sweeps, int32_t *n_patch,
                                 int32_t *patch, double *gram, double *eigval, double *eigvec, int32_t *sweeps, void *stream)
{
    if (max_sweeps < 1 || max_sweeps > MET2_MPPCA_MAX_SWEEPS) return fail(MET2_E_INVALID, "max_sweeps must be 1 to 30");
    MppcaStageArgs A;
    A.max_sweeps = max_sweeps;
    A.n_patch = n_patch; A.patch = patch; A.sweeps = sweeps;
    A.gram = gram; A.eigval = eigval; A.eigvec = eigvec;
    return mppca_launch<true>(device, nx, ny, nz, nt, data, mask, window, out, sigma, rank, stream, A);
}

// ---- met2_mppca_box

#define MET2_MPPCA_BOX_MAX 343                      // the window's voxel count: its patch list fits beside the matrices at every n_te
#define MET2_MPPCA_WORK_CAP (1LL << 30)             // what the default work space never exceeds (the header states it)
#define MET2_MPPCA_RANK_GUESS 8                     // vectors per centre the cut is reckoned at (measured means: 1.1 to 1.3 at 32 echoes)

namespace {

struct BoxShape {
    int nx, ny, nz, nt, hx, hy, hz;
    int64_t largest, worst, guess;                  // the largest patch; doubles of vectors a centre can keep at most, and is reckoned at
    static const int64_t fixed = 16;                // the pool's counter
    int64_t centres(int bx, int by, int bz) const   // of a box of bx x by x bz output voxels, at most
    {
        auto along = [](int b, int h, int n) { return (int64_t)(b + 2 * h < n ? b + 2 * h : n); };
        return along(bx, hx, nx) * along(by, hy, ny) * along(bz, hz, nz);
    }
    int64_t all_bytes(int64_t c) const { return fixed + c * ((int64_t)sizeof(MppcaHead) + worst * 8); }      // c centres at any rank
    // c centres as reckoned; never less than one voxel's centres at any rank, so that a box halved down to one voxel always runs
    int64_t guess_bytes(int64_t c) const
    {
        const int64_t pool = c * guess > largest * worst ? c * guess : largest * worst;
        return fixed + c * (int64_t)sizeof(MppcaHead) + pool * 8;
    }
    int64_t min_bytes() const { return guess_bytes(largest); }
    int64_t default_bytes() const
    {
        const int64_t all = all_bytes(centres(nx, ny, nz)), floor = min_bytes();
        const int64_t capped = all < MET2_MPPCA_WORK_CAP ? all : MET2_MPPCA_WORK_CAP;
        return capped > floor ? capped : floor;
    }
    // the largest box within `bytes` (>= min_bytes): whole planes while one fits, else whole lines of one plane, else a run of one line
    void tile(int64_t bytes, int &bx, int &by, int &bz) const
    {
        auto fits = [&](int x, int y, int z) { return guess_bytes(centres(x, y, z)) <= bytes; };
        by = ny; bz = nz;
        for (bx = nx; bx >= 1 && !fits(bx, by, bz); --bx) {}
        if (bx >= 1) return;
        bx = 1;
        for (by = ny; by >= 1 && !fits(bx, by, bz); --by) {}
        if (by >= 1) return;
        by = 1;
        for (bz = nz; bz > 1 && !fits(bx, by, bz); --bz) {}
    }
};

// the argument checks both entries share; on MET2_OK `S` is set
int box_shape(int32_t nx, int32_t ny, int32_t nz, int32_t nt, const int32_t window[3], int32_t average, BoxShape &S)
{
    if (nx < 0 || ny < 0 || nz < 0) return fail(MET2_E_INVALID, "bad shape");
    if (!window) return fail(MET2_E_INVALID, "NULL window");
    for (int a = 0; a < 3; ++a)
        if (window[a] < 1 || window[a] % 2 == 0) return fail(MET2_E_INVALID, "every entry of the MP-PCA window must be odd and at least 1");
    const int64_t wtot = (int64_t)window[0] * window[1] * window[2];
    if (wtot < 3) return fail(MET2_E_INVALID, "the MP-PCA window must hold at least 3 voxels");
    if (average != 0 && average != 1) return fail(MET2_E_INVALID, "average must be 0 or 1");
    if (nt < 2 || nt > MET2_MPPCA_MAX_TE) return fail(MET2_E_UNSUPPORTED, "MP-PCA supports 2 to 63 echoes");
    if (wtot > MET2_MPPCA_BOX_MAX) return fail(MET2_E_UNSUPPORTED, "the MP-PCA window's patch list does not fit in LDS beside the two matrices (more than 343 voxels)");
    S.nx = nx; S.ny = ny; S.nz = nz; S.nt = nt;
    S.hx = window[0] / 2; S.hy = window[1] / 2; S.hz = window[2] / 2;
    S.largest = S.centres(1, 1, 1);                 // the largest patch a voxel of this volume can have, and the most centres that hold a voxel
    const int64_t kmax = nt < S.largest ? nt : S.largest;
    S.worst = (int64_t)nt * kmax;
    S.guess = (int64_t)nt * (kmax < MET2_MPPCA_RANK_GUESS ? kmax : MET2_MPPCA_RANK_GUESS);
    return MET2_OK;
}

struct OutBox { int x, y, z, nx, ny, nz; };

}  // namespace

extern "C" int met2_mppca_box_work_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t nt, const int32_t window[3], int32_t average,
                                         int64_t *min_bytes, int64_t *default_bytes)
{
    BoxShape S;
    const int rc = box_shape(nx, ny, nz, nt, window, average, S);
    if (rc != MET2_OK) return rc;
    const bool none = average == 0 || (int64_t)nx * ny * nz == 0;
    if (min_bytes) *min_bytes = none ? 0 : S.min_bytes();
    if (default_bytes) *default_bytes = none ? 0 : S.default_bytes();
    return MET2_OK;
}

extern "C" int met2_mppca_box(int32_t device, int32_t nx, int32_t ny, int32_t nz, int32_t nt, const double *data, const uint8_t *mask,
                              const int32_t window[3], int32_t average, int64_t max_work_bytes, double *out, double *sigma, int32_t *rank,
                              int32_t *n_patch, double *wsum, void *stream)
{
    BoxShape S;
    const int rc0 = box_shape(nx, ny, nz, nt, window, average, S);
    if (rc0 != MET2_OK) return rc0;
    const int ld = nt | 1;
    const size_t lds = 2 * sizeof(double) * (size_t)nt * ld + aux_bytes((size_t)window[0] * window[1] * window[2]);
    if (lds > MET2_MPPCA_LDS_MAX) return fail(MET2_E_UNSUPPORTED, "the MP-PCA window's patch list does not fit in LDS beside the two matrices");
    const int64_t nvox = (int64_t)nx * ny * nz;
    if (max_work_bytes < 0) return fail(MET2_E_INVALID, "max_work_bytes must be >= 0");
    if (nvox == 0) return MET2_OK;
    if (!data || !out) return fail(MET2_E_INVALID, "NULL argument");
    if (data == out) return fail(MET2_E_INVALID, "MP-PCA cannot run in place");
    if (nvox > 0x3ffffffLL) return fail(MET2_E_UNSUPPORTED, "volume too large for one launch");
    int64_t budget = 0;
    if (average) {
        budget = max_work_bytes ? max_work_bytes : S.default_bytes();
        if (budget < S.min_bytes())
            return fail(MET2_E_INVALID, "max_work_bytes is below the " + std::to_string(S.min_bytes()) + " bytes this volume and window need at least");
    }
    USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    MppcaBoxArgs A = MppcaBoxArgs();
    A.nx = nx; A.ny = ny; A.nz = nz; A.nt = nt; A.win = 0; A.ld = ld;
    A.data = data; A.mask = mask;
    A.hx = S.hx; A.hy = S.hy; A.hz = S.hz;
    if (!average) {                                                     // one launch over the whole volume, nothing held
        A.out = out; A.sigma = sigma; A.rank = rank; A.n_patch = n_patch;
        A.cx0 = A.cy0 = A.cz0 = 0; A.cny = ny; A.cnz = nz;
        hipLaunchKernelGGL((mppca_kernel<false, 1>), dim3((unsigned)nvox), dim3(64), lds, st, A);
        HIPCHK(hipGetLastError());
        if (wsum) HIPCHK(hipMemsetAsync(wsum, 0, (size_t)nvox * sizeof(double), st));
        return MET2_OK;
    }
    int bx, by, bz;
    S.tile(budget, bx, by, bz);
    const int64_t cmax = S.centres(bx, by, bz);
    const int64_t bytes = S.all_bytes(cmax) < budget ? S.all_bytes(cmax) : budget;      // more than every centre at any rank is never needed
    DeviceWork W(st);
    const auto piece = W.take<char>((size_t)bytes);                     // one piece: BoxShape's byte counts, which the budget is held against, lay it out
    if (!W.alloc()) return W.finish("met2_mppca_box");
    char *work = piece;
    A.used = (unsigned long long *)work;
    A.head = (MppcaHead *)(work + BoxShape::fixed);
    A.basis = (double *)(work + BoxShape::fixed + cmax * (int64_t)sizeof(MppcaHead));
    A.pool = (bytes - BoxShape::fixed - cmax * (int64_t)sizeof(MppcaHead)) / 8;         // >= largest * worst: see guess_bytes
    MppcaAvgArgs G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.nt = nt; G.hx = S.hx; G.hy = S.hy; G.hz = S.hz;
    G.data = data; G.mask = mask; G.head = A.head; G.basis = A.basis;
    G.out = out; G.sigma = sigma; G.wsum = wsum; G.rank = rank; G.n_patch = n_patch;
    auto lo = [](int o, int h) { return o - h > 0 ? o - h : 0; };
    auto hi = [](int o, int b, int h, int n) { return o + b + h < n ? o + b + h : n; };
    std::vector<OutBox> todo;                                           // a stack: the boxes of the cut in reverse, so that they run in memory order
    for (int ox = (nx - 1) / bx * bx; ox >= 0; ox -= bx)
        for (int oy = (ny - 1) / by * by; oy >= 0; oy -= by)
            for (int oz = (nz - 1) / bz * bz; oz >= 0; oz -= bz)
                todo.push_back(OutBox{ox, oy, oz, ox + bx < nx ? bx : nx - ox, oy + by < ny ? by : ny - oy, oz + bz < nz ? bz : nz - oz});
    while (!todo.empty() && W.ok()) {
        const OutBox b = todo.back();
        todo.pop_back();
        A.cx0 = lo(b.x, S.hx); A.cy0 = lo(b.y, S.hy); A.cz0 = lo(b.z, S.hz);
        const int cnx = hi(b.x, b.nx, S.hx, nx) - A.cx0;
        A.cny = hi(b.y, b.ny, S.hy, ny) - A.cy0; A.cnz = hi(b.z, b.nz, S.hz, nz) - A.cz0;
        const int64_t nc = (int64_t)cnx * A.cny * A.cnz;                // <= cmax: the box is at most bx x by x bz
        if (nc > cmax) { W.ok(hipErrorInvalidValue); break; }
        if (!W.ok(hipMemsetAsync(A.used, 0, sizeof(unsigned long long), st))) break;
        hipLaunchKernelGGL((mppca_kernel<false, 2>), dim3((unsigned)nc), dim3(64), lds, st, A);
        if (!W.ok(hipGetLastError())) break;
        if (nc * S.worst > A.pool) {                                    // the centres may have kept more than the pool holds: look
            unsigned long long used = 0;
            if (!W.ok(hipMemcpyAsync(&used, A.used, sizeof(used), hipMemcpyDeviceToHost, st)) || !W.ok(hipStreamSynchronize(st))) break;
            if (used > (unsigned long long)A.pool) {                    // halve the box along its longest side and run the halves (one voxel never gets here)
                OutBox p = b, q = b;
                if (b.nx >= b.ny && b.nx >= b.nz) { p.nx = b.nx / 2; q.x = b.x + p.nx; q.nx = b.nx - p.nx; }
                else if (b.ny >= b.nz) { p.ny = b.ny / 2; q.y = b.y + p.ny; q.ny = b.ny - p.ny; }
                else { p.nz = b.nz / 2; q.z = b.z + p.nz; q.nz = b.nz - p.nz; }
                if ((int64_t)b.nx * b.ny * b.nz < 2) { W.ok(hipErrorInvalidValue); break; }
                todo.push_back(q);
                todo.push_back(p);
                continue;
            }
        }
        G.ox0 = b.x; G.oy0 = b.y; G.oz0 = b.z; G.ony = b.ny; G.onz = b.nz;
        G.cx0 = A.cx0; G.cy0 = A.cy0; G.cz0 = A.cz0; G.cny = A.cny; G.cnz = A.cnz;
        hipLaunchKernelGGL(mppca_average_kernel, dim3((unsigned)((int64_t)b.nx * b.ny * b.nz)), dim3(64), 0, st, G);
        W.ok(hipGetLastError());
    }
    return W.finish("met2_mppca_box");
}
