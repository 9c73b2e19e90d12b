// Device helpers every matrix and sweep kernel file uses (softattn*.hip, gausslogp*.hip, gaussup.hip, convgemm.hip,
// conv_bwd.hip, forwardsum.hip, mobo.hip, pausepath.hip, maxpath.hip; segments.h takes its clamp from here): the MFMA
// operand vector types, the branch-free mask, the fp32 -> bf16 pair split, the LDS-only barrier, the XCD-aware block
// map, the clamps of the utterance lengths with the "either length 0: empty" rule, and the buffer resource over an
// utterance's block.  Each exists here once (the clamp in its two orders): a fix reaches every kernel that uses it.
#pragma once
#include <hip/hip_runtime.h>

namespace aligner {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;     // one lane's A or B fragment of a bf16 MFMA (16 bytes)
typedef __attribute__((ext_vector_type(16))) float f32x16;     // one lane's 32 x 32 accumulator tile

// v or +0.0 without a select on the loaded value (a select fed by a load is turned back into a
// branch around the load, which serialises the loads)
__device__ __forceinline__ float and_mask(float v, unsigned m) {
    return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & m);
}

// ReLU that keeps NaN, as torch.relu does (fmaxf(NaN, 0) is 0: a NaN activation would vanish after one layer and the
// loss of a diverged run stay finite).  IEEE 754-2019 maximum: one v_maximum3_f32 on gfx950, where the select
// v < 0 ? 0 : v is a compare and a v_cndmask per element (C3's step 214 -> 216 us)
__device__ __forceinline__ float relu_nan(float v) { return __builtin_elementwise_maximum(v, 0.f); }

// v = hi + lo in two bf16 halves (lo: the rounding error of hi, itself rounded): a product of two such pairs as
// hi*hi + hi*lo + lo*hi with fp32 accumulation is ~2^-16 relative, at the bf16 MFMA rate
__device__ __forceinline__ void split_bf16(float v, __bf16 &hi, __bf16 &lo) {
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);
}

// Workgroup barrier for LDS traffic only: __syncthreads() also waits for vmcnt(0), which puts a memory round trip
// (the loads in flight for the next tile or row, the result stores of this one) on every barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Workgroup `bid` of a 1-D grid of per_b workgroups x B utterances -> (utterance b, workgroup `inner` of it).
// Workgroups are dealt round-robin over the 8 XCDs (observed, speed only): with B a multiple of 8 the per_b workgroups
// that re-read one utterance's operand are kept on the same XCD, so its L2 fetches that operand once instead of once
// per XCD.
// (softattn.hip keeps this text written out in its two kernels: called as a function it rewrites their prologues, and
// with that and the minimum-first clamp the row-tile kernel measured 14.0-14.3 us against the 13.6-13.9 us of three runs
// of the code as it was: profiles/device_helpers_times_first.txt)
__device__ __forceinline__ void xcd_block_map(int B, int per_b, unsigned bid, int &b, int &inner) {
    if ((B & 7) == 0) {
        const int xcd = bid & 7, slot = bid >> 3;
        inner = slot % per_b;
        b = (slot / per_b) * 8 + xcd;
    } else {
        b = bid / per_b;
        inner = bid % per_b;
    }
}

// utterance b's length within [0, T]; T where the caller gave no lengths
__device__ inline int clamp_len(const int *__restrict__ t, int b, int T) {
    int v = t ? t[b] : T;
    v = v < T ? v : T;
    return v > 0 ? v : 0;
}

// The same interval tested "below 0" first.  The compiler does not know that T >= 0, so the two orders are different
// code: the similarity and Gaussian kernels keep the order they were written in (taking the minimum first changes the
// register allocation of gb_prep_col_kernel and gb_finish_kernel and rewrites the similarity kernels' prologues).
__device__ __forceinline__ int clamp_len_lo(const int *t, int b, int T) {
    int v = T;
    if (t) {
        v = t[b];
        v = v < 0 ? 0 : (v > T ? T : v);
    }
    return v;
}

// both lengths of utterance b; an utterance with either length 0 is empty: tx = ty = 0
__device__ __forceinline__ void utterance_lengths(const int *t_xs, const int *t_ys, int b, int Tx, int Ty, int &tx, int &ty) {
    tx = clamp_len_lo(t_xs, b, Tx);
    ty = clamp_len_lo(t_ys, b, Ty);
    if (tx <= 0 || ty <= 0) tx = ty = 0;
}

// `bytes` from `base` (an utterance's block of a tensor) as a buffer resource: per-lane 32-bit byte offsets plus a
// scalar offset address it, reads past the block return 0 and stores past it are dropped by the hardware instead of
// faulting -- a lane whose cell does not exist carries an offset beyond any block
__device__ __forceinline__ __amdgpu_buffer_rsrc_t utterance_rsrc(const void *base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
}

}  // namespace aligner
