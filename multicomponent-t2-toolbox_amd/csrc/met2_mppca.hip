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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>
#include <cmath>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"
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

template <bool STAGES> struct mppca_args { typedef MppcaArgs type; };
template <> struct mppca_args<true> { typedef MppcaStageArgs type; };

// the lanes of one wave exchange values through LDS: a wave's LDS accesses complete in program order, the fences keep the compiler to it
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// pair k of round t of the round-robin tournament over n players (n even): player n - 1 stays, the others turn
__device__ __forceinline__ void rr_pair(int n, int t, int k, int &p, int &q)
{
    const int m = n - 1;
    int a = t + k;  if (a >= m) a -= m;
    int b = t - k;  if (b < 0) b += m;
    p = k == 0 ? m : a;
    q = b;
}

template <bool STAGES> __device__ __forceinline__ int sweep_cap(const typename mppca_args<STAGES>::type &A)
{
    if constexpr (STAGES) return A.max_sweeps;
    else return MET2_MPPCA_MAX_SWEEPS;
}

size_t aux_bytes(int win)
{
    const size_t list = (size_t)win * win * win * sizeof(int32_t);
    const size_t need = list > 1024 ? list : 1024;       // the patch list, then the rotations' (c, s) [32 + 32], then the sorted spectrum [64]
    return (need + 15) / 16 * 16;
}

template <bool STAGES>
__global__ __launch_bounds__(64) void mppca_kernel(typename mppca_args<STAGES>::type A)
{
    extern __shared__ __attribute__((aligned(16))) double mppca_lds[];
    const int M = A.nt, LD = A.ld;
    double *C = mppca_lds;
    double *V = C + (size_t)M * LD;
    double *aux = V + (size_t)M * LD;
    int32_t *list = reinterpret_cast<int32_t *>(aux);
    const int lane = met2::lane_id();
    const int64_t v = blockIdx.x;
    const bool mine = lane < M;
    double *ov = A.out + v * M;

    if (A.mask && A.mask[v] == 0) {
        if (mine) ov[lane] = 0.0;
        if (lane == 0) { if (A.sigma) A.sigma[v] = 0.0; if (A.rank) A.rank[v] = 0; }
        if constexpr (STAGES) { if (A.n_patch && lane == 0) A.n_patch[v] = 0; }
        return;
    }
    const int vz = (int)(v % A.nz), vy = (int)((v / A.nz) % A.ny), vx = (int)(v / ((int64_t)A.nz * A.ny));
    const int h = A.win / 2;
    const int x0 = max(vx - h, 0), y0 = max(vy - h, 0), z0 = max(vz - h, 0);
    const int wx = min(vx + h + 1, A.nx) - x0, wy = min(vy + h + 1, A.ny) - y0, wz = min(vz + h + 1, A.nz) - z0;
    const int wtot = wx * wy * wz;                                   // <= win^3: the list's room

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
        const int max_sweeps = sweep_cap<STAGES>(A);
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
            sig = sqrt(sigma2);
            rank = k;
        }
    }
    if (mine) ov[lane] = res;
    if (lane == 0) { if (A.sigma) A.sigma[v] = sig; if (A.rank) A.rank[v] = rank; }
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
    const size_t lds = 2 * sizeof(double) * (size_t)nt * ld + aux_bytes(window > 63 ? 63 : window);
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
