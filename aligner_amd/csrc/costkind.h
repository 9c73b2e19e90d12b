// The kinds of the pairwise cost table (l1cost.hip: dense; banddtw.hip: band storage).  A kind is three pieces, and the
// kernels are written once per (layout, direction) over them:
//
//     term(t, p, acc)      one channel of one cell added to the cell's running sum, channels in order
//     finish(acc, scale)   the finished sum -> the stored cost
//     back(p, t, g, acc)   one cell's share of d cost / d pred[c,i] times G added to the running sum; g is G already
//                          masked by "the cell exists" (device.h: and_mask), so it is +0 where there is none
//     factor(scale, g)     what multiplies the finished backward sum once (dtarget takes its negative)
//
// The build has -ffp-contract=off: a fused multiply-add happens exactly where __builtin_fmaf is written.
//
//     L1       |t - p| added                        back: G, -G or 0 selected by sign(p - t), sign(0) = 0      k = scale g
//     L2       d = t - p, acc = fma(d, d, acc)      back: d = p - t, acc = fma(G, d, acc)                       k = (2 scale) g
//     L2Root   L2's sum, sqrt(acc) scale            no gradient (it needs the finished table and is singular at 0)
//
// Along a warping path only the path's own distances are needed, and there the root has a gradient too: pathcost.hip
// runs these pieces on the pairs of a path and keeps the root's backward pieces (PathRootGrad) to itself.
//
// L1 and L2 are two vector instructions per cell and channel.  A masked G of +0 times a finite d is 0, so the backward
// kernels take their pred rows and target columns from inside the utterance's lengths (a NaN in the padding past
// n[b] or m[b] would otherwise ride in on 0 * NaN); the selection of L1 never needed that and is unchanged by it.
#pragma once

namespace aligner {

struct CostL1 {
    static constexpr bool has_backward = true;
    static __device__ __forceinline__ float term(float t, float p, float acc) { return acc + __builtin_fabsf(t - p); }
    static __device__ __forceinline__ float finish(float acc, float scale) { return acc * scale; }
    // (0 for a tie, and for a NaN, which compares false both ways)
    static __device__ __forceinline__ float back(float p, float t, float g, float acc) {
        return acc + (p > t ? g : (p < t ? -g : 0.f));
    }
    static __device__ __forceinline__ float factor(float scale, float g) { return scale * g; }
};

struct CostL2 {
    static constexpr bool has_backward = true;
    static __device__ __forceinline__ float term(float t, float p, float acc) {
        const float d = t - p;
        return __builtin_fmaf(d, d, acc);
    }
    static __device__ __forceinline__ float finish(float acc, float scale) { return acc * scale; }
    static __device__ __forceinline__ float back(float p, float t, float g, float acc) {
        const float d = p - t;
        return __builtin_fmaf(g, d, acc);
    }
    static __device__ __forceinline__ float factor(float scale, float g) { return (2.f * scale) * g; }
};

struct CostL2Root : CostL2 {
    static constexpr bool has_backward = false;
    // (the compiler expands this to the correctly rounded square root, denormal operands included: DESIGN.md 5.13)
    static __device__ __forceinline__ float finish(float acc, float scale) { return __builtin_sqrtf(acc) * scale; }
};

}  // namespace aligner
