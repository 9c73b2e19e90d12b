// Vector-Jacobian product of gausslogp.hip's value tensor on MI355X (gfx950).  With G = dL/dvalue [B,Tx,ld] (read as
// grad_scale[b] G[b] when a scale is given; cells outside the lengths and the pad columns contribute nothing and are
// never read into a result) and w = exp(-2 s):
//
//   R[i]   = sum_j G[i,j]            P[c,i] = sum_j G[i,j] z[c,j]       Q[c,i] = sum_j G[i,j] z[c,j]^2
//   U[c,j] = sum_i G[i,j] w[c,i]     V[c,j] = sum_i G[i,j] (m w)[c,i]
//   dz[c,j] = V - z U        dm[c,i] = w (P - m R)        ds[c,i] = w (Q - 2 m P + m^2 R) - R
//
// U, V, P and Q are contractions with the forward's operand shapes and run on the bf16 matrix cores the forward's way:
// every fp32 operand split x = hi + lo, three v_mfma_f32_32x32x16_bf16 per product (lo*hi, hi*lo, hi*hi; fp32
// accumulate).  G is split as it is read.  R is an fp32 sum on the vector unit (it rides on registers G is in anyway).
//
//  * gb_prep_col_kernel / gb_prep_row_kernel: the operands that are not G, masked by the lengths, split and laid out in
//    A-fragment order in the workspace: (w, m w) over 16-token k-steps for the contraction over tokens, (z, z^2) over
//    32-frame chunks for the one over frames.  Channel tiles (32 channels) are padded with zeros to a whole number of
//    channel groups.
//  * gb_col_kernel<NCT> (dz): one wave = one 32-frame strip of one utterance and one group of NCT <= 3 channel tiles:
//    2 NCT accumulator tiles (U, V).  A k-step is 16 tokens: the B fragment is G[16 rows][32 frames] (each load two whole
//    128-byte row segments), asked for one k-step ahead of the MFMAs that consume it (two register sets); the A
//    fragments of the step are asked for in front of that, so waiting for them does not wait for the newer G loads.
//    Epilogue: dz = V - z U, 32 consecutive frames of a channel per half wave.
//  * gb_row_kernel<NCT> (P, Q, R): one wave = one 32-token tile, one channel group and one SPLIT of the frame range
//    (gb_plan(): a function of the shape alone, so that small batches fill the chip).  A chunk is 32 frames = two
//    k-steps in a permuted frame order (a lane reads 16 consecutive frames of its token's row: a lane pair one 128-byte
//    line; the z fragments are laid out in the same order), the next chunk's G asked for during the second k-step.
//    Partial P, Q, R go to the workspace per split.
//  * gb_finish_kernel: sums the partials in split order and forms dm and ds.
//  * No LDS, no barriers, no atomics; every sum in a fixed order: the same bits on every call and every stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "aligner_amd.h"
#include "common.h"
#include "device.h"

namespace aligner {

constexpr int GB_MAX_NCT = 3;                     // channel tiles per wave: 6 accumulator tiles
constexpr int GB_TARGET_WAVES = 1536;             // the row kernel splits the frame sweep until it has about this many waves
constexpr int GB_MIN_CHUNKS = 4;                  // ... but a split keeps at least 128 frames

struct GbPlan {
    int CT, NG, NCT, CTP;                         // channel tiles; groups; tiles per group; NG * NCT
    int KSI;                                      // 16-token k-steps
    int NS;                                       // 32-frame strips = chunks
    int RT;                                       // 32-token tiles
    int per, nsplit;                              // chunks per frame split, frame splits
    size_t col_off, row_off, part_off, rpart_off, total;
};

// Everything here is a function of the shape alone (determinism: the split count never depends on the device or the data).
static GbPlan gb_plan(int B, int C, int Tx, int Ty) {
    GbPlan L;
    L.CT = (C + 31) / 32;
    L.NG = (L.CT + GB_MAX_NCT - 1) / GB_MAX_NCT;
    L.NCT = (L.CT + L.NG - 1) / L.NG;
    L.CTP = L.NG * L.NCT;
    L.KSI = (Tx + 15) / 16;
    L.NS = (Ty + 31) / 32;
    L.RT = (Tx + 31) / 32;
    const long long waves = (long long)B * L.RT * L.NG;
    long long want = waves > 0 ? GB_TARGET_WAVES / waves : 1;
    const int most = (L.NS + GB_MIN_CHUNKS - 1) / GB_MIN_CHUNKS;
    if (want > most) want = most;
    if (want < 1) want = 1;
    L.per = (L.NS + (int)want - 1) / (int)want;
    L.nsplit = (L.NS + L.per - 1) / L.per;
    const size_t colb = (size_t)B * L.CTP * L.KSI * 4 * 64 * sizeof(uint4);
    const size_t rowb = (size_t)B * L.CTP * L.NS * 2 * 4 * 64 * sizeof(uint4);
    const size_t partb = (size_t)L.nsplit * B * L.RT * L.CTP * 2 * 1024 * sizeof(float);
    const size_t rpartb = (size_t)L.nsplit * B * L.RT * 32 * sizeof(float);
    L.col_off = 0;
    L.row_off = align_up(colb, 256);
    L.part_off = L.row_off + align_up(rowb, 256);
    L.rpart_off = L.part_off + align_up(partb, 256);
    L.total = L.rpart_off + align_up(rpartb, 256);
    return L;
}

struct GbParams {
    const float *g;         // [B,Tx,ld]
    const float *gscale;    // [B], nullable
    const float *z;         // [B,C,Ty]
    const float *mean;      // [B,C,Tx]
    const float *logstd;    // [B,C,Tx]
    const int *t_xs;        // nullable
    const int *t_ys;        // nullable
    float *dz;              // [B,C,Ty], nullable
    float *dmean;           // [B,C,Tx], nullable
    float *dlogstd;         // [B,C,Tx], nullable
    uint4 *colA;            // [B][CTP][KSI][w hi, w lo, mw hi, mw lo][64]
    uint4 *rowA;            // [B][CTP][NS][2][z hi, z lo, z^2 hi, z^2 lo][64]
    float *part;            // [nsplit][B][RT][CTP][P, Q][32 channels][32 tokens]
    float *rpart;           // [nsplit][B][RT][32 tokens]
    int NG, CTP, KSI, NS, RT, per, nsplit;
    int B, C, Tx, Ty, ld;
};

// Lane (channel 32 ct + lane&31, half lane>>5) of k-step ks holds tokens 16 ks + 8 half + jj: A[c][k] of the MFMA.
__global__ __launch_bounds__(64) void gb_prep_col_kernel(GbParams p) {
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    const int ks = blockIdx.x, ct = blockIdx.y, b = blockIdx.z;
    int tx, ty;
    utterance_lengths(p.t_xs, p.t_ys, b, p.Tx, p.Ty, tx, ty);
    const int c = 32 * ct + l31, cc = c < p.C ? c : p.C - 1;
    const float *Mb = p.mean + ((size_t)b * p.C + cc) * p.Tx;
    const float *Sb = p.logstd + ((size_t)b * p.C + cc) * p.Tx;
    float mv[8], sv[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {              // unconditional loads (clamped address, masked value)
        const int i = 16 * ks + 8 * half + jj, ic = i < p.Tx ? i : p.Tx - 1;
        mv[jj] = Mb[ic];
        sv[jj] = Sb[ic];
    }
    bf16x8 wh, wl, mh, ml;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const int i = 16 * ks + 8 * half + jj;
        const unsigned ok = (c < p.C && i < tx) ? ~0u : 0u;
        const float w = and_mask(expf(-2.0f * sv[jj]), ok);
        const float mw = and_mask(mv[jj] * w, ok);
        __bf16 h, l;
        split_bf16(w, h, l);
        wh[jj] = h;
        wl[jj] = l;
        split_bf16(mw, h, l);
        mh[jj] = h;
        ml[jj] = l;
    }
    uint4 *F = p.colA + ((((size_t)b * p.CTP + ct) * p.KSI + ks) * 4) * 64 + lane;
    F[0] = __builtin_bit_cast(uint4, wh);
    F[64] = __builtin_bit_cast(uint4, wl);
    F[128] = __builtin_bit_cast(uint4, mh);
    F[192] = __builtin_bit_cast(uint4, ml);
}

// Lane (channel, half) of k-step u of chunk ch holds frames 32 ch + 16 half + 8 u + jj: the order gb_row_kernel reads G in.
__global__ __launch_bounds__(128) void gb_prep_row_kernel(GbParams p) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5, u = threadIdx.x >> 6;
    const int ch = blockIdx.x, ct = blockIdx.y, b = blockIdx.z;
    int tx, ty;
    utterance_lengths(p.t_xs, p.t_ys, b, p.Tx, p.Ty, tx, ty);
    const int c = 32 * ct + l31, cc = c < p.C ? c : p.C - 1;
    const float *Zb = p.z + ((size_t)b * p.C + cc) * p.Ty;
    float v[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const int j = 32 * ch + 16 * half + 8 * u + jj, jc = j < p.Ty ? j : p.Ty - 1;
        v[jj] = Zb[jc];
    }
    bf16x8 zh, zl, qh, ql;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const int j = 32 * ch + 16 * half + 8 * u + jj;
        const float x = and_mask(v[jj], (c < p.C && j < ty) ? ~0u : 0u);
        __bf16 h, l;
        split_bf16(x, h, l);
        zh[jj] = h;
        zl[jj] = l;
        split_bf16(x * x, h, l);
        qh[jj] = h;
        ql[jj] = l;
    }
    uint4 *F = p.rowA + (((((size_t)b * p.CTP + ct) * p.NS + ch) * 2 + u) * 4) * 64 + lane;
    F[0] = __builtin_bit_cast(uint4, zh);
    F[64] = __builtin_bit_cast(uint4, zl);
    F[128] = __builtin_bit_cast(uint4, qh);
    F[192] = __builtin_bit_cast(uint4, ql);
}

// acc0 += a[0..1] x b, acc1 += a[2..3] x b, the three split products, the small terms first
template <int NCT>
__device__ __forceinline__ void gb_products(const uint4 (&a)[NCT][4], bf16x8 bh, bf16x8 bl, f32x16 (&acc0)[NCT], f32x16 (&acc1)[NCT]) {
#pragma unroll
    for (int t = 0; t < NCT; ++t) {
        acc0[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[t][1]), bh, acc0[t], 0, 0, 0);
        acc1[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[t][3]), bh, acc1[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < NCT; ++t) {
        acc0[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[t][0]), bl, acc0[t], 0, 0, 0);
        acc1[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[t][2]), bl, acc1[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < NCT; ++t) {
        acc0[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[t][0]), bh, acc0[t], 0, 0, 0);
        acc1[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[t][2]), bh, acc1[t], 0, 0, 0);
    }
}

template <int NCT>
__global__ __launch_bounds__(64, 2) void gb_col_kernel(GbParams p) {
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    int b, inner;
    xcd_block_map(p.B, p.NS * p.NG, blockIdx.x, b, inner);
    const int st = inner % p.NS, cg = inner / p.NS;
    int tx, ty;
    utterance_lengths(p.t_xs, p.t_ys, b, p.Tx, p.Ty, tx, ty);
    const int j0 = 32 * st;
    const int col = j0 + l31, colc = col < p.Ty ? col : p.Ty - 1;      // (j0 < Ty: the strip exists)

    f32x16 U[NCT], V[NCT];
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) U[t][e] = V[t][e] = 0.f;

    if (j0 < ty) {                                // (wave-uniform) a strip past t_y stores zeros only
        const float sc = p.gscale ? p.gscale[b] : 1.0f;
        const float *Gb = p.g + (size_t)b * p.Tx * p.ld + colc;
        const uint4 *A = p.colA + (((size_t)b * p.CTP + (size_t)cg * NCT) * p.KSI) * 256 + lane;
        const size_t tstep = (size_t)p.KSI * 256;         // one channel tile
        const int ksn = (tx + 15) / 16;
        const unsigned colok = col < ty ? ~0u : 0u;
        float g0[8], g1[8];
        auto load_g = [&](float (&g)[8], int ks) {
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int i = 16 * ks + 8 * half + jj;
                g[jj] = Gb[(size_t)(i < p.Tx ? i : p.Tx - 1) * p.ld];
            }
        };
        auto kstep = [&](const float (&g)[8], float (&gn)[8], int ks) __attribute__((always_inline)) {
            uint4 a[NCT][4];
#pragma unroll
            for (int t = 0; t < NCT; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) a[t][q] = A[t * tstep + (size_t)ks * 256 + q * 64];
            load_g(gn, ks + 1 < ksn ? ks + 1 : ks);       // (past the last k-step: the last one again, never used)
            __builtin_amdgcn_sched_barrier(0);
            bf16x8 bh, bl;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int i = 16 * ks + 8 * half + jj;
                const float v = and_mask(g[jj], i < tx ? colok : 0u) * sc;
                __bf16 h, l;
                split_bf16(v, h, l);
                bh[jj] = h;
                bl[jj] = l;
            }
            gb_products<NCT>(a, bh, bl, U, V);
            __builtin_amdgcn_sched_barrier(0);
        };
        load_g(g0, 0);
        for (int ks = 0; ks < ksn; ks += 2) {
            kstep(g0, g1, ks);
            if (ks + 1 < ksn) kstep(g1, g0, ks + 1);
        }
    }
    // C/D layout: col = lane&31 (frame), row = (e&3) + 8*(e>>2) + 4*(lane>>5) (channel of the tile)
    const float *Zb = p.z + (size_t)b * p.C * p.Ty;
    float *Db = p.dz + (size_t)b * p.C * p.Ty;
#pragma unroll
    for (int t = 0; t < NCT; ++t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int c = 32 * (cg * NCT + t) + (e & 3) + 8 * (e >> 2) + 4 * half;
            const size_t o = (size_t)(c < p.C ? c : p.C - 1) * p.Ty + colc;
            const float zv = Zb[o];
            const float r = col < ty ? V[t][e] - zv * U[t][e] : 0.f;
            if (c < p.C && col < p.Ty) Db[o] = r;
        }
    }
}

template <int NCT>
__global__ __launch_bounds__(64, 2) void gb_row_kernel(GbParams p) {
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    int b, inner;
    xcd_block_map(p.B, p.RT * p.nsplit * p.NG, blockIdx.x, b, inner);
    const int rt = inner % p.RT, sp = (inner / p.RT) % p.nsplit, cg = inner / (p.RT * p.nsplit);
    int tx, ty;
    utterance_lengths(p.t_xs, p.t_ys, b, p.Tx, p.Ty, tx, ty);
    if (32 * rt >= tx) return;                    // (wave-uniform) gb_finish_kernel never reads a tile past t_x
    const int i = 32 * rt + l31, ic = i < p.Tx ? i : p.Tx - 1;
    const int ch0 = sp * p.per;
    int ch1 = ch0 + p.per;
    ch1 = ch1 < p.NS ? ch1 : p.NS;
    ch1 = ch1 < (ty + 31) / 32 ? ch1 : (ty + 31) / 32;

    f32x16 P[NCT], Q[NCT];
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) P[t][e] = Q[t][e] = 0.f;
    float r = 0.f;

    if (ch0 < ch1) {
        const float sc = p.gscale ? p.gscale[b] : 1.0f;
        const float *Gr = p.g + ((size_t)b * p.Tx + ic) * p.ld;
        const uint4 *A = p.rowA + ((((size_t)b * p.CTP + (size_t)cg * NCT) * p.NS) * 2) * 256 + lane;
        const size_t tstep = (size_t)p.NS * 2 * 256;      // one channel tile
        const bool vec = (p.ld & 3) == 0 && (reinterpret_cast<uintptr_t>(p.g) & 15) == 0;     // rows on 16-byte boundaries
        const unsigned rowok = i < tx ? ~0u : 0u;
        float g0[16], g1[16];
        auto load_g = [&](float (&g)[16], int ch) {
            const int jb = 32 * ch + 16 * half;
            if (vec && 32 * ch + 32 <= p.Ty) {            // (wave-uniform) a whole chunk inside the row
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 x = *reinterpret_cast<const float4 *>(Gr + jb + 4 * q);
                    g[4 * q] = x.x;
                    g[4 * q + 1] = x.y;
                    g[4 * q + 2] = x.z;
                    g[4 * q + 3] = x.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) g[k] = Gr[jb + k < p.Ty ? jb + k : p.Ty - 1];
            }
        };
        auto chunk = [&](const float (&g)[16], float (&gn)[16], int ch) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                uint4 a[NCT][4];
#pragma unroll
                for (int t = 0; t < NCT; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) a[t][q] = A[t * tstep + ((size_t)ch * 2 + u) * 256 + q * 64];
                if (u == 1) load_g(gn, ch + 1 < ch1 ? ch + 1 : ch);   // behind this step's fragments: their wait leaves it in flight
                __builtin_amdgcn_sched_barrier(0);
                bf16x8 bh, bl;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const int j = 32 * ch + 16 * half + 8 * u + jj;
                    const float v = and_mask(g[8 * u + jj], j < ty ? rowok : 0u) * sc;
                    r += v;
                    __bf16 h, l;
                    split_bf16(v, h, l);
                    bh[jj] = h;
                    bl[jj] = l;
                }
                gb_products<NCT>(a, bh, bl, P, Q);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        load_g(g0, ch0);
        for (int ch = ch0; ch < ch1; ch += 2) {
            chunk(g0, g1, ch);
            if (ch + 1 < ch1) chunk(g1, g0, ch + 1);
        }
    }
    // C/D layout: col = lane&31 (token), row = (e&3) + 8*(e>>2) + 4*(lane>>5) (channel of the tile)
    const size_t tile = ((size_t)sp * p.B + b) * p.RT + rt;
#pragma unroll
    for (int t = 0; t < NCT; ++t) {
        float *Pp = p.part + ((tile * p.CTP + (size_t)cg * NCT + t) * 2) * 1024 + l31;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int cl = (e & 3) + 8 * (e >> 2) + 4 * half;
            Pp[cl * 32] = P[t][e];
            Pp[1024 + cl * 32] = Q[t][e];
        }
    }
    r += __shfl_xor(r, 32);                       // the two frame halves of a token (both lanes get the same bits)
    if (cg == 0 && half == 0) p.rpart[tile * 32 + l31] = r;
}

// dm and ds from the partials, summed in split order.  A workgroup = 32 tokens x 8 channels.
__global__ __launch_bounds__(256) void gb_finish_kernel(GbParams p) {
    const int rt = blockIdx.x, b = blockIdx.z;
    const int l31 = threadIdx.x & 31;
    const int i = 32 * rt + l31, c = 8 * blockIdx.y + (threadIdx.x >> 5);
    if (c >= p.C || i >= p.Tx) return;
    int tx, ty;
    utterance_lengths(p.t_xs, p.t_ys, b, p.Tx, p.Ty, tx, ty);
    float dm = 0.f, ds = 0.f;
    if (i < tx) {
        float R = 0.f, P = 0.f, Q = 0.f;
        for (int sp = 0; sp < p.nsplit; ++sp) {
            const size_t tile = ((size_t)sp * p.B + b) * p.RT + rt;
            const float *Pp = p.part + ((tile * p.CTP + (c >> 5)) * 2) * 1024 + (c & 31) * 32 + l31;
            R += p.rpart[tile * 32 + l31];
            P += Pp[0];
            Q += Pp[1024];
        }
        const size_t o = ((size_t)b * p.C + c) * p.Tx + i;
        const float m = p.mean[o];
        const float w = expf(-2.0f * p.logstd[o]);
        dm = w * (P - m * R);
        ds = w * ((Q - 2.0f * m * P) + (m * m) * R) - R;
    }
    const size_t o = ((size_t)b * p.C + c) * p.Tx + i;
    if (p.dmean) p.dmean[o] = dm;
    if (p.dlogstd) p.dlogstd[o] = ds;
}

template <int NCT>
static void gb_launch(const GbParams &p, bool col, bool row, hipStream_t s) {
    if (col)
        hipLaunchKernelGGL(gb_col_kernel<NCT>, dim3((unsigned)p.NS * p.NG * p.B), dim3(64), 0, s, p);
    if (row)
        hipLaunchKernelGGL(gb_row_kernel<NCT>, dim3((unsigned)p.RT * p.nsplit * p.NG * p.B), dim3(64), 0, s, p);
}

}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_gauss_logp_backward_workspace_bytes(int B, int C, int Tx, int Ty) {
    if (B < 1 || C < 1 || Tx < 1 || Ty < 1 || C > 256 || Tx > 1024 || B > 65535) return 0;
    return gb_plan(B, C, Tx, Ty).total;
}

int aligner_gauss_logp_backward_f32(const float *grad_value, int ld_grad, const float *grad_scale, const float *z,
                                    const float *mean, const float *logstd, const int32_t *t_xs, const int32_t *t_ys,
                                    float *dz, float *dmean, float *dlogstd, void *workspace, size_t workspace_bytes,
                                    int B, int C, int Tx, int Ty, void *stream) {
    if (!grad_value || !z || !mean || !logstd || !workspace) return fail(ALIGNER_EINVAL, "null pointer");
    if (!dz && !dmean && !dlogstd) return fail(ALIGNER_EINVAL, "no output: dz, dmean and dlogstd are all null");
    if (B < 0 || C < 1 || Tx < 1 || Ty < 1) return fail(ALIGNER_EINVAL, "bad shape B=%d C=%d Tx=%d Ty=%d", B, C, Tx, Ty);
    if (ld_grad < Ty) return fail(ALIGNER_EINVAL, "ld_grad=%d < Ty=%d", ld_grad, Ty);
    if (ld_grad != Ty && ((size_t)ld_grad * sizeof(float)) % 16 != 0)
        return fail(ALIGNER_EINVAL, "ld_grad=%d: rows must start on 16-byte boundaries", ld_grad);
    if (C > 256) return fail(ALIGNER_EDOM, "C=%d exceeds 256 channels", C);
    if (Tx > 1024) return fail(ALIGNER_EDOM, "Tx=%d exceeds 1024 text rows", Tx);
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if (B == 0) return ALIGNER_OK;
    const GbPlan L = gb_plan(B, C, Tx, Ty);
    const unsigned long long colw = (unsigned long long)L.NS * L.NG * B, roww = (unsigned long long)L.RT * L.nsplit * L.NG * B;
    if (colw >= (1ull << 31) || roww >= (1ull << 31))
        return fail(ALIGNER_EDOM, "Ty=%d: %llu workgroups exceed 2^31", Ty, colw > roww ? colw : roww);
    if (workspace_bytes < L.total) return fail(ALIGNER_ENOSPC, "workspace %zu < %zu bytes", workspace_bytes, L.total);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    GbParams p{grad_value, grad_scale, z, mean, logstd, t_xs, t_ys, dz, dmean, dlogstd,
               reinterpret_cast<uint4 *>(ws + L.col_off), reinterpret_cast<uint4 *>(ws + L.row_off),
               reinterpret_cast<float *>(ws + L.part_off), reinterpret_cast<float *>(ws + L.rpart_off),
               L.NG, L.CTP, L.KSI, L.NS, L.RT, L.per, L.nsplit, B, C, Tx, Ty, ld_grad};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool col = dz != nullptr, row = dmean != nullptr || dlogstd != nullptr;
    if (col) {
        hipLaunchKernelGGL(gb_prep_col_kernel, dim3(L.KSI, L.CTP, B), dim3(64), 0, s, p);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    if (row) {
        hipLaunchKernelGGL(gb_prep_row_kernel, dim3(L.NS, L.CTP, B), dim3(128), 0, s, p);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    if (L.NCT == 1) gb_launch<1>(p, col, row, s);
    else if (L.NCT == 2) gb_launch<2>(p, col, row, s);
    else gb_launch<3>(p, col, row, s);
    ALIGNER_HIP_CHECK(hipGetLastError());
    if (row) {
        hipLaunchKernelGGL(gb_finish_kernel, dim3(L.RT, (C + 7) / 8, B), dim3(256), 0, s, p);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

}  // extern "C"
