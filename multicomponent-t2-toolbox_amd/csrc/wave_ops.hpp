// wave_ops.hpp -- wave64 cross-lane primitives for gfx950 (CDNA4).
// One wavefront = 64 lanes; every helper here must be called under full EXEC
// (wave-uniform control flow).
#pragma once
#include <hip/hip_runtime.h>

// The row-walk changes -- the half-wave model_signal() (nnls_wave.hpp) and the DPP cross-row stage of the wave reductions below -- are taken
// by the translation units that set MET2_ROWWALK (met2_fit_x2_nb1.hip, met2_fit_nnls_lcurve.hip: X2 at one bin per lane, L-curve, NNLS and
// T2SPARC) and by the development builds in one translation unit.  Every other translation unit compiles the code of before: with the
// cross-row stage's result in a scalar pair the compiler allocates several other kernels differently -- the X2 kernel at two bins per lane
// keeps 472 B of solver state in scratch (36 B before), the BayesReg spill-over kernel gains a spilled VGPR (profiles/rowwalk_ab.txt,
// section 3).  -DMET2_ROWWALK_PARTS=<mask> (development: the A/B builds of that file): bit 1 the half waves, bit 2 the cross-row stage.
#if !defined(MET2_ROWWALK) && !defined(MET2_SPLIT_TU)
#define MET2_ROWWALK 1
#endif
#ifndef MET2_ROWWALK
#define MET2_ROWWALK 0
#endif
#ifndef MET2_ROWWALK_PARTS
#define MET2_ROWWALK_PARTS 6
#endif
#define MET2_ROWWALK_ON(bit) (MET2_ROWWALK && (MET2_ROWWALK_PARTS & (bit)))

namespace met2 {

typedef unsigned long long u64;

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

// The lane number again, but opaque to the optimiser.  Per-lane constants of an inlined routine (column bases, byte offsets,
// tile coordinates) are loop-invariant in the voxel loop: the compiler hoists them out of it, runs out of registers and spills
// them (BayesReg at 168 VGPRs: 32 such 64-bit values, reloaded from scratch in the inner loops -- 110 KB of fetches per voxel).
// Derived from this value they are recomputed in place: a few integer instructions per call.
__device__ __forceinline__ int lane_opaque(int lane) { asm volatile("" : "+v"(lane)); return lane; }

// broadcast lane `l` (wave-uniform) of v to all lanes (v_readlane_b32 x2 -> SGPR pair)
__device__ __forceinline__ double bcast(double v, int l)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int bcast_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// per-lane gather from lane `src` (ds_bpermute_b32 x2)
__device__ __forceinline__ double gather(double v, int src)
{
    int lo = __builtin_amdgcn_ds_bpermute(src << 2, __double2loint(v));
    int hi = __builtin_amdgcn_ds_bpermute(src << 2, __double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int gather_i(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }

template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v)
{
    int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// DPP controls: quad_perm[1,0,3,2]=0xB1, quad_perm[2,3,0,1]=0x4E, row_half_mirror=0x141, row_mirror=0x140
#define MET2_ROW_REDUCE(v, OP)                 \
    v = OP(v, dpp_mov<0xB1>(v));               \
    v = OP(v, dpp_mov<0x4E>(v));               \
    v = OP(v, dpp_mov<0x141>(v));              \
    v = OP(v, dpp_mov<0x140>(v));

__device__ __forceinline__ double op_add(double a, double b) { return a + b; }
__device__ __forceinline__ double op_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ double op_min(double a, double b) { return fmin(a, b); }

// The cross-row stage.  Every lane of a row holds its row's result r0, r16, r32, r48 after MET2_ROW_REDUCE.  Two DPP row broadcasts combine
// them in the pairing (r0 o r16) o (r32 o r48) that four lane reads and three operations gave before: row_bcast:15 (0x142) hands lane 15 of
// each row to the row behind it -- rows 1 and 3 form OP(row before, own) = r0 o r16 and r32 o r48 -- and row_bcast:31 (0x143) hands lane 31 to
// rows 2 and 3 -- row 3 forms OP(lane 31, own) = (r0 o r16) o (r32 o r48), the operands in the order the lane reads had them.  Rows 0 to 2 end
// with values nobody reads (a row without a source lane reads zero: bound_ctrl); lane 63 is broadcast.  Six cross-lane moves and two
// operations, where the lane reads cost eight moves, the copies of one operand of each pair out of the scalar file, and three operations.
#if MET2_ROWWALK_ON(4)
#define MET2_CROSS_ROW(v, OP)                  \
    v = OP(dpp_mov<0x142>(v), v);              \
    v = OP(dpp_mov<0x143>(v), v);              \
    v = bcast(v, 63);
#else
#define MET2_CROSS_ROW(v, OP) v = OP(OP(bcast(v, 0), bcast(v, 16)), OP(bcast(v, 32), bcast(v, 48)));
#endif

__device__ __forceinline__ double wave_sum(double v)
{
    MET2_ROW_REDUCE(v, op_add)
    MET2_CROSS_ROW(v, op_add)
    return v;
}
// two sums at once (independent chains interleave)
__device__ __forceinline__ void wave_sum2(double &a, double &b)
{
    MET2_ROW_REDUCE(a, op_add)
    MET2_ROW_REDUCE(b, op_add)
    MET2_CROSS_ROW(a, op_add)
    MET2_CROSS_ROW(b, op_add)
}
__device__ __forceinline__ double wave_max(double v)
{
    MET2_ROW_REDUCE(v, op_max)
    MET2_CROSS_ROW(v, op_max)
    return v;
}
__device__ __forceinline__ double wave_min(double v)
{
    MET2_ROW_REDUCE(v, op_min)
    MET2_CROSS_ROW(v, op_min)
    return v;
}

__device__ __forceinline__ u64 ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ int first_lane(u64 m) { return __builtin_ctzll(m); }

} // namespace met2
