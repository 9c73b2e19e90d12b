// The per-cell arithmetic of Soft-DTW, shared by the dense kernels (softdtw.hip) and the band-storage kernels
// (banddtw.hip): a cell is a function of its operands only, so the two compute the same bits from the same operands,
// and the bounds of tests/softdtw_oracle.py (derived from exactly these operations) hold for both.
//
// Base-2 logs with log2(e) / gamma folded into the costs on their way in, "+inf" the finite SD_BIG (it absorbs every
// addend, nothing computes inf - inf), every cell's result clamped to [-SD_BIG, SD_BIG].  Backward is pushed: a cell
// hands its E times the softmin's own weights 2^(mn - pred) / sum to its three predecessors.
//
// DtwSoft is this arithmetic as the cell policy of the forward kernels (dtw_forward.h).
#pragma once
#include <hip/hip_runtime.h>

#include "dtw_schedule.h"

namespace aligner {

// lane i <- src[lane i-1], lane 0 gets `edge` (wave_shr:1); lane i <- src[lane i+1], lane 63 gets `edge` (wave_shl:1)
__device__ __forceinline__ float sd_from_below(float edge, float src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge),
                                                                 __builtin_bit_cast(int, src), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float sd_from_above(float edge, float src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge),
                                                                 __builtin_bit_cast(int, src), 0x130, 0xf, 0xf, false));
}
__device__ __forceinline__ float sd_lane(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
// a wave's own LDS traffic in program order, for the compiler as well (lanes read what other lanes of the wave wrote)
__device__ __forceinline__ void sd_wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// a cost on its way in: scaled, clamped to the sentinel
__device__ __forceinline__ float sd_cost_in(float d, float scale) { return fminf(fmaxf(d * scale, -SD_BIG), SD_BIG); }

// the three softmin weights 2^(mn - x), mn the smallest operand (so one of them is 1 and the sum is in [1, 3])
__device__ __forceinline__ float sd_weights(float a, float b, float c, float &wa, float &wb, float &wc) {
    const float mn = fminf(fminf(a, b), c);
    wa = __builtin_amdgcn_exp2f(mn - a);
    wb = __builtin_amdgcn_exp2f(mn - b);
    wc = __builtin_amdgcn_exp2f(mn - c);
    return mn;
}

// R[i,j] from R[i-1,j-1], R[i-1,j], R[i,j-1] (scaled), the scaled penalty and the scaled cost
__device__ __forceinline__ float sd_cell(float diag, float up, float left, float pen, float d) {
    float wa, wb, wc;
    const float mn = sd_weights(diag, up + pen, left + pen, wa, wb, wc);
    const float cur = d + (mn - __builtin_amdgcn_logf((wa + wb) + wc));
    return __builtin_amdgcn_fmed3f(cur, -SD_BIG, SD_BIG);
}

// what cell (i,j) with E[i,j] = e hands to (i-1,j-1), (i-1,j) and (i,j-1), from their stored R values
__device__ __forceinline__ void sd_push(float diag, float up, float left, float pen, float e, float &cd, float &cu, float &cl) {
    float wa, wb, wc;
    sd_weights(diag, up + pen, left + pen, wa, wb, wc);
    const float inv = __builtin_amdgcn_rcpf((wa + wb) + wc);
    const float q = e * inv;
    cd = q * wa;
    cu = q * wb;
    cl = q * wc;
}

// The soft cell for dtw_forward.h: R (scaled) is what a cell keeps, in the tile and in the table; R[n-1,m-1] goes to the
// workspace for the backward kernel and, unscaled, to the value.
struct DtwSoft {
    using Out = float;
    static constexpr bool TILE_HOLDS_VALUE = true;
    static __device__ __forceinline__ float none() { return SD_BIG; }
    static __device__ __forceinline__ float in(const DtwParams &p, float d) { return sd_cost_in(d, p.scale); }
    static __device__ __forceinline__ float cell(const DtwParams &p, float diag, float up, float left, float d, int &k) {
        k = 0;
        return sd_cell(diag, up, left, p.pen, d);
    }
    static __device__ __forceinline__ float keep(float cur, int) { return cur; }
    static __device__ __forceinline__ float *table(const DtwParams &p) { return p.grad; }
    static __device__ __forceinline__ float out(float x) { return x; }
    static __device__ __forceinline__ void finish(const DtwParams &p, int b, float fin) {
        p.fin[b] = fin;
        p.value[b] = fin < 0.5f * SD_BIG ? fin * p.unscale : __builtin_huge_valf();
    }
};

}  // namespace aligner
