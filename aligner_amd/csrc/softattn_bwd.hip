// Backward of the soft-attention front end (softattn.hip) on MI355X (gfx950).
//
// Given the cotangents G_l = dL/dlogp and (optionally) G_s = dL/dsoft, [B,Tx,Ty] fp32:
//   G      = G_l + soft (G_s - sum_i soft G_s)          (soft = softmax_i(logp) = softmax_i(logit + log(prior + 1e-8)))
//   p      = softmax_i(logit)                           (the prior is an additive constant of the log-probs)
//   dlogit = G - p sum_i G                              (0 on rows i >= t_x)
//   L2 : dK[c,i] = 2T (sum_j dlogit q[c,j] - k[c,i] sum_j dlogit),  dQ[c,j] = 2T (sum_i dlogit k[c,i] - q[c,j] sum_i dlogit)
//   dot: dK[c,i] =  T  sum_j dlogit q[c,j],                         dQ[c,j] =  T  sum_i dlogit k[c,i]
// (sum_i G = sum_i G_l: the soft term sums to S - S sum_i soft = 0.)
//
// The logits are recomputed, never read: a saved logp would be as many bytes again as G.  Two kernels:
//  * softattn_bwd_col_kernel: a workgroup owns 128 frames (a wave 32) and every text row of its utterance, as the
//    forward's exact-product kernel does.  A first sweep over the row tiles forms each frame's column statistics (the
//    log-sum-exp of the logits, sum_i G_l and, with G_s, the log-sum-exp of logit + log prior and sum_i soft G_s) and
//    stores them (workspace, 16 bytes a frame); a second sweep forms dlogit in the MFMA accumulator layout and
//    contracts it with the text operand straight from registers into dQ (dQ finishes inside the workgroup).
//  * softattn_bwd_row_kernel: a workgroup owns one 32-row text tile; its four waves take every fourth 32-frame strip,
//    recompute the tile's logits and dlogit from the stored statistics and accumulate dK^T partials in registers over
//    their strips.  The four partials are summed in LDS in wave order: no atomics, the same bits on every call.
// Products: fp32 MFMA (v_mfma_f32_32x32x2f32), i.e. exact fp32 products at every temperature; DESIGN.md 4.2 has the
// numbers and what a faster form would take.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "aligner_amd.h"
#include "common.h"
#include "device.h"

namespace aligner {

constexpr float SB_NEG_INF = -__builtin_huge_valf();
constexpr int SB_THREADS = 256;                 // 4 waves
constexpr int SB_LDS_BUDGET = 64 * 1024;        // column kernel: text rows staged per group

struct SaBwdParams {
    const float *keys;      // [B,C,Tx]
    const float *queries;   // [B,C,Ty]
    const int *t_xs;        // nullable
    const float *prior;     // nullable [B,Tx,Ty]
    const float *gl;        // [B,Tx,Ty]
    const float *gs;        // nullable [B,Tx,Ty]
    float *dk;              // nullable [B,C,Tx]
    float *dq;              // nullable [B,C,Ty]
    float *stats;           // [B][4][Ty]: lse(logit), sum_i G_l, lse(logit + log prior), sum_i soft G_s
    int B, C, Tx, Ty;
    float temperature;
    int l2;
    int GE;                 // column kernel: 32-row tiles staged per group
};

// the two halves of a wave hold the same frames (rows 4h + ...): combine in a fixed order so both get the same bits
__device__ __forceinline__ float sb_sum_halves(float v, int half) {
    const float o = __shfl_xor(v, 32);
    return half ? o + v : v + o;
}

// online log-sum-exp (m, l) with a weighted sum w riding along, merged across the halves in a fixed order
__device__ __forceinline__ void sb_merge_halves(float &m, float &l, float &w, int half) {
    const float mo = __shfl_xor(m, 32), lo = __shfl_xor(l, 32), wo = __shfl_xor(w, 32);
    const float ma = half ? mo : m, la = half ? lo : l, wa = half ? wo : w;
    const float mb = half ? m : mo, lb = half ? l : lo, wb = half ? w : wo;
    const float mn = fmaxf(ma, mb);
    if (mn == SB_NEG_INF) {
        m = SB_NEG_INF; l = 0.f; w = 0.f;
        return;
    }
    const float fa = ma == SB_NEG_INF ? 0.f : __expf(ma - mn), fb = mb == SB_NEG_INF ? 0.f : __expf(mb - mn);
    m = mn;
    l = la * fa + lb * fb;
    w = wa * fa + wb * fb;
}

// dlogit of one valid element from its logit, cotangents and its frame's statistics
__device__ __forceinline__ float sb_dlogit(float lg, float gl, float gs, float lpr, const float (&st)[4], bool has_gs) {
    float g = gl;
    if (has_gs) g = fmaf(__expf(lg + lpr - st[2]), gs - st[3], g);
    return fmaf(-__expf(lg - st[0]), st[1], g);
}

// mel operand of a 32-frame strip: B fragment k = 2s + half, column = this lane's frame.  Held in registers up to 128
// channels; above, read again where it is used (registers: the operand and the dQ / dK accumulators would not fit)
template <int NCT>
struct SbMel {
    static constexpr int S2 = 16 * NCT;
    static constexpr bool REG = NCT <= 4;
    float qx[REG ? S2 : 1];
    const float *Qb;
    int col, C, Ty, half;
    bool ok;
    float qn;                 // |q_j|^2
    __device__ __forceinline__ float load(int s) const {
        const int c = 2 * s + half;
        return (c < C && ok) ? Qb[c * Ty + col] : 0.f;
    }
    __device__ __forceinline__ float operator[](int s) const {
        if constexpr (REG) return qx[s];
        else return load(s);
    }
    __device__ __forceinline__ void init(const SaBwdParams &p, const float *Qb_, int col_, bool ok_, int half_) {
        Qb = Qb_; col = col_; C = p.C; Ty = p.Ty; half = half_; ok = ok_;
        float n = 0.f;
#pragma unroll
        for (int s = 0; s < S2; ++s) {
            const float v = load(s);
            if constexpr (REG) qx[s] = v;
            n = fmaf(v, v, n);
        }
        qn = sb_sum_halves(n, half);
    }
};

// C/D layout of v_mfma_f32_32x32x2f32: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int sb_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }

template <int NCT>
__global__ __launch_bounds__(SB_THREADS) void softattn_bwd_col_kernel(SaBwdParams p) {
    constexpr int S2 = 16 * NCT, CP = 32 * NCT;
    extern __shared__ __attribute__((aligned(16))) float sb_smem[];
    const int GE = p.GE, PK = 32 * GE + 1;
    float *Ks = sb_smem;                              // [CP][PK]: K[c][32 GE g + il], zero beyond C and t_x
    float *kn = Ks + (size_t)CP * PK;                 // [32 GE]: T |k_i|^2 scaled (L2), 0 (dot)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int NJ = (p.Ty + 127) / 128;
    const int b = blockIdx.x / NJ;
    const int col = (blockIdx.x % NJ) * 128 + wave * 32 + (lane & 31);
    const bool col_ok = col < p.Ty;
    const int tx = clamp_len_lo(p.t_xs, b, p.Tx);
    const float scale = p.l2 ? -p.temperature : p.temperature;
    const float *Kb = p.keys + (size_t)b * p.C * p.Tx;
    const float *Qb = p.queries + (size_t)b * p.C * p.Ty;
    const bool has_gs = p.gs != nullptr;
    SbMel<NCT> qx;
    qx.init(p, Qb, col, col_ok, half);
    const float qn = qx.qn;
    const int RT = (tx + 31) / 32, NG = (RT + GE - 1) / GE;      // rows >= t_x have dlogit = 0: never visited
    auto stage = [&](int g) {
        const int W = 32 * GE, i0 = W * g;
        for (int idx = tid; idx < CP * W; idx += SB_THREADS) {
            const int c = idx / W, il = idx - c * W, i = i0 + il;
            Ks[c * PK + il] = (c < p.C && i < tx) ? Kb[(size_t)c * p.Tx + i] : 0.f;
        }
        __syncthreads();
        for (int il = tid; il < W; il += SB_THREADS) {
            float n = 0.f;
            if (p.l2)
                for (int c = 0; c < p.C; ++c) n = fmaf(Ks[c * PK + il], Ks[c * PK + il], n);
            kn[il] = scale * n;
        }
        __syncthreads();
    };
    auto logits = [&](float (&lg)[16], int r) {
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        const float *A = Ks + half * PK + 32 * r + (lane & 31);
#pragma unroll
        for (int s = 0; s < S2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[2 * s * PK], qx[s], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int il = 32 * r + sb_row(e, half);
            lg[e] = p.l2 ? fmaf(acc[e], -2.0f * scale, kn[il] + scale * qn) : acc[e] * scale;
        }
    };
    // per-utterance bases (uniform) + 32-bit lane offsets (Tx Ty < 2^29): one VGPR an address
    const size_t ub = (size_t)b * p.Tx * p.Ty;
    const float *glb = p.gl + ub, *gsb = p.gs ? p.gs + ub : nullptr, *prb = p.prior ? p.prior + ub : nullptr;

    // sweep 1: column statistics
    float m1 = SB_NEG_INF, l1 = 0.f, gsum = 0.f, m2 = SB_NEG_INF, l2s = 0.f, w2 = 0.f;
    for (int g = 0; g < NG; ++g) {
        if (g > 0) __syncthreads();
        stage(g);
        const int nt = (RT - GE * g < GE) ? RT - GE * g : GE;
        for (int r = 0; r < nt; ++r) {
            float lg[16];
            logits(lg, r);
            const int ib = 32 * (GE * g + r);
            float tm = m1;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (col_ok && ib + sb_row(e, half) < tx) tm = fmaxf(tm, lg[e]);
            if (tm != SB_NEG_INF) {
                float ls = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (col_ok && ib + sb_row(e, half) < tx) ls += __expf(lg[e] - tm);
                l1 = (m1 == SB_NEG_INF ? 0.f : l1 * __expf(m1 - tm)) + ls;
                m1 = tm;
            }
            if (col_ok) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int i = ib + sb_row(e, half);
                    if (i < tx) gsum += glb[i * p.Ty + col];
                }
            }
            if (col_ok && has_gs) {
                float x[16];
                float tm2 = m2;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int i = ib + sb_row(e, half);
                    x[e] = SB_NEG_INF;
                    if (i < tx) {
                        x[e] = lg[e] + (prb ? __logf(prb[i * p.Ty + col] + 1e-8f) : 0.f);
                        tm2 = fmaxf(tm2, x[e]);
                    }
                }
                if (tm2 != SB_NEG_INF) {
                    float ls = 0.f, ws = 0.f;
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int i = ib + sb_row(e, half);
                        if (i < tx) {
                            const float ex = __expf(x[e] - tm2);
                            ls += ex;
                            ws = fmaf(ex, gsb[i * p.Ty + col], ws);
                        }
                    }
                    const float f = m2 == SB_NEG_INF ? 0.f : __expf(m2 - tm2);
                    l2s = l2s * f + ls;
                    w2 = w2 * f + ws;
                    m2 = tm2;
                }
            }
        }
    }
    float st[4];
    {
        float dummy = 0.f;
        sb_merge_halves(m1, l1, dummy, half);
        sb_merge_halves(m2, l2s, w2, half);
        st[0] = m1 == SB_NEG_INF ? SB_NEG_INF : m1 + __logf(l1);
        st[1] = sb_sum_halves(gsum, half);
        st[2] = m2 == SB_NEG_INF ? SB_NEG_INF : m2 + __logf(l2s);
        st[3] = l2s > 0.f ? w2 / l2s : 0.f;
        if (col_ok && half == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) p.stats[((size_t)b * 4 + k) * p.Ty + col] = st[k];
        }
    }
    if (!p.dq) return;

    // sweep 2: dlogit, dQ = K dlogit (the accumulator is the B operand as it stands: k-step s <-> element s)
    f32x16 aq[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) aq[ct][e] = 0.f;
    float dsum = 0.f;
    for (int g = 0; g < NG; ++g) {
        if (NG > 1) {
            __syncthreads();
            stage(g);
        }
        const int nt = (RT - GE * g < GE) ? RT - GE * g : GE;
        for (int r = 0; r < nt; ++r) {
            float lg[16], d[16];
            logits(lg, r);
            const int ib = 32 * (GE * g + r);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = ib + sb_row(e, half);
                d[e] = 0.f;
                if (col_ok && i < tx) {
                    const int idx = i * p.Ty + col;
                    const float gs = has_gs ? gsb[idx] : 0.f;
                    const float lpr = (has_gs && prb) ? __logf(prb[idx] + 1e-8f) : 0.f;
                    d[e] = sb_dlogit(lg[e], glb[idx], gs, lpr, st, has_gs);
                }
                dsum += d[e];
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const float *A = Ks + (32 * ct + (lane & 31)) * PK + 32 * r + 4 * half;
#pragma unroll
                for (int s = 0; s < 16; ++s)
                    aq[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[(s & 3) + 8 * (s >> 2)], d[s], aq[ct], 0, 0, 0);
            }
        }
    }
    dsum = sb_sum_halves(dsum, half);
    if (!col_ok) return;
    const float f = p.l2 ? 2.0f * p.temperature : p.temperature;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int c = 32 * ct + sb_row(e, half);
            if (c < p.C) {
                float v = aq[ct][e];
                if (p.l2 && tx > 0) v = fmaf(-Qb[(size_t)c * p.Ty + col], dsum, v);   // t_x = 0: exactly 0, whatever q holds
                p.dq[((size_t)b * p.C + c) * p.Ty + col] = f * v;
            }
        }
}

template <int NCT>
__global__ __launch_bounds__(SB_THREADS) void softattn_bwd_row_kernel(SaBwdParams p) {
    // NCT = 8: the dK accumulators of 2 channel tiles a workgroup (blockIdx.y picks them); the logits need all channels
    constexpr int S2 = 16 * NCT, CP = 32 * NCT, WP = 33, NCTO = NCT <= 4 ? NCT : 2;
    const int ct0 = NCT <= 4 ? 0 : blockIdx.y * NCTO, cend = 32 * (ct0 + NCTO) < p.C ? 32 * (ct0 + NCTO) : p.C;
    extern __shared__ __attribute__((aligned(16))) float sb_smem[];
    float *Ka = sb_smem;                  // [CP][32]: K[c][i0 + il], zero beyond C and t_x
    float *kn = Ka + CP * 32;             // [32]
    float *rsw = kn + 32;                 // [4 waves][32]: sum_j dlogit of each row, per wave
    float *Wv = rsw + 4 * 32;             // per wave [2][32][WP] (Q of one channel tile, dlogit), later [4][1024] partials
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int RT = (p.Tx + 31) / 32;
    const int b = blockIdx.x / RT, i0 = 32 * (blockIdx.x % RT);
    const int tx = clamp_len_lo(p.t_xs, b, p.Tx);
    float *dkb = p.dk + (size_t)b * p.C * p.Tx;
    if (i0 >= tx) {                       // a tile of masked rows: dK = 0 exactly
        for (int idx = 32 * 32 * ct0 + tid; idx < cend * 32; idx += SB_THREADS) {
            const int c = idx >> 5, i = i0 + (idx & 31);
            if (i < p.Tx) dkb[(size_t)c * p.Tx + i] = 0.f;
        }
        return;
    }
    const float scale = p.l2 ? -p.temperature : p.temperature;
    const float *Kb = p.keys + (size_t)b * p.C * p.Tx;
    const float *Qb = p.queries + (size_t)b * p.C * p.Ty;
    const bool has_gs = p.gs != nullptr;
    for (int idx = tid; idx < CP * 32; idx += SB_THREADS) {
        const int c = idx >> 5, i = i0 + (idx & 31);
        Ka[idx] = (c < p.C && i < tx) ? Kb[(size_t)c * p.Tx + i] : 0.f;
    }
    __syncthreads();
    if (tid < 32) {
        float n = 0.f;
        if (p.l2)
            for (int c = 0; c < p.C; ++c) n = fmaf(Ka[c * 32 + tid], Ka[c * 32 + tid], n);
        kn[tid] = scale * n;
    }
    __syncthreads();
    float *wq = Wv + wave * 2 * 32 * WP, *wd = wq + 32 * WP;
    const size_t ub = (size_t)b * p.Tx * p.Ty;
    const float *glb = p.gl + ub, *gsb = p.gs ? p.gs + ub : nullptr, *prb = p.prior ? p.prior + ub : nullptr;
    f32x16 ak[NCTO];
#pragma unroll
    for (int ct = 0; ct < NCTO; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) ak[ct][e] = 0.f;
    float rs = 0.f;
    const int NS = (p.Ty + 31) / 32;
    for (int sp = wave; sp < NS; sp += 4) {
        const int col = 32 * sp + (lane & 31);
        const bool col_ok = col < p.Ty;
        SbMel<NCT> qx;
        qx.init(p, Qb, col, col_ok, half);
        const float qn = qx.qn;
        float st[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) st[k] = col_ok ? p.stats[((size_t)b * 4 + k) * p.Ty + col] : 0.f;
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        if constexpr (SbMel<NCT>::REG) {
#pragma unroll
            for (int s = 0; s < S2; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ka[(2 * s + half) * 32 + (lane & 31)], qx[s], acc, 0, 0, 0);
        } else {
#pragma unroll 1
            for (int s0 = 0; s0 < S2; s0 += 16)
#pragma unroll
                for (int s = s0; s < s0 + 16; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ka[(2 * s + half) * 32 + (lane & 31)], qx.load(s), acc, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int il = sb_row(e, half), i = i0 + il;
            float d = 0.f;
            if (col_ok && i < tx) {
                const float lg = p.l2 ? fmaf(acc[e], -2.0f * scale, kn[il] + scale * qn) : acc[e] * scale;
                const int idx = i * p.Ty + col;
                const float gs = has_gs ? gsb[idx] : 0.f;
                const float lpr = (has_gs && prb) ? __logf(prb[idx] + 1e-8f) : 0.f;
                d = sb_dlogit(lg, glb[idx], gs, lpr, st, has_gs);
            }
            wd[il * WP + (lane & 31)] = d;                  // dlogit[i][j], read back transposed
        }
        float bd[16];                                       // B operand: k = frame 2s + half, n = row lane & 31
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            bd[s] = wd[(lane & 31) * WP + 2 * s + half];
            rs += bd[s];
        }
#pragma unroll
        for (int ct = 0; ct < NCTO; ++ct) {
#pragma unroll
            for (int s = 0; s < 16; ++s) wq[(2 * s + half) * WP + (lane & 31)] = qx[16 * (ct0 + ct) + s];
#pragma unroll
            for (int s = 0; s < 16; ++s)      // A operand: m = channel 32 ct + lane & 31, k = frame 2s + half
                ak[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wq[(lane & 31) * WP + 2 * s + half], bd[s], ak[ct], 0, 0, 0);
        }
    }
    rs = sb_sum_halves(rs, half);
    __syncthreads();
    if (half == 0) rsw[wave * 32 + lane] = rs;
    const float f = p.l2 ? 2.0f * p.temperature : p.temperature;
#pragma unroll
    for (int ct = 0; ct < NCTO; ++ct) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) Wv[wave * 1024 + e * 64 + lane] = ak[ct][e];
        __syncthreads();
        for (int idx = tid; idx < 1024; idx += SB_THREADS) {
            const int e = idx >> 6, ln = idx & 63, il = ln & 31;
            const int c = 32 * (ct0 + ct) + sb_row(e, ln >> 5), i = i0 + il;
            if (c >= p.C || i >= p.Tx) continue;
            float v = 0.f;
            if (i < tx) {
                v = ((Wv[idx] + Wv[1024 + idx]) + Wv[2048 + idx]) + Wv[3072 + idx];
                if (p.l2) {
                    const float rsum = ((rsw[il] + rsw[32 + il]) + rsw[64 + il]) + rsw[96 + il];
                    v = fmaf(-Ka[c * 32 + il], rsum, v);
                }
                v *= f;
            }
            dkb[(size_t)c * p.Tx + i] = v;
        }
    }
}

static int sb_nct(int C) { return C <= 32 ? 1 : C <= 64 ? 2 : C <= 96 ? 3 : C <= 128 ? 4 : 8; }

static size_t sb_col_lds(int NCT, int GE) { return ((size_t)32 * NCT * (32 * GE + 1) + 32 * GE) * sizeof(float); }
static size_t sb_row_lds(int NCT) { return ((size_t)32 * NCT * 32 + 32 + 4 * 32 + 4 * 2 * 32 * 33) * sizeof(float); }

template <int NCT>
static int sb_launch(const SaBwdParams &p0, hipStream_t s) {
    SaBwdParams p = p0;
    const int RT = (p.Tx + 31) / 32;
    int GE = 1;
    while (GE < RT && sb_col_lds(NCT, GE + 1) <= (size_t)SB_LDS_BUDGET) ++GE;
    p.GE = GE;
    const size_t lc = sb_col_lds(NCT, GE), lr = sb_row_lds(NCT);
    auto kc = softattn_bwd_col_kernel<NCT>;
    auto kr = softattn_bwd_row_kernel<NCT>;
    ALIGNER_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void *>(kc), lc));
    ALIGNER_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void *>(kr), lr));
    hipLaunchKernelGGL(kc, dim3((unsigned)((p.Ty + 127) / 128) * (unsigned)p.B), dim3(SB_THREADS), lc, s, p);
    ALIGNER_HIP_CHECK(hipGetLastError());
    if (p.dk) {
        hipLaunchKernelGGL(kr, dim3((unsigned)RT * (unsigned)p.B, NCT <= 4 ? 1 : NCT / 2), dim3(SB_THREADS), lr, s, p);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_softattn_backward_workspace_bytes(int B, int C, int Tx, int Ty) {
    if (B < 0 || C < 1 || Tx < 1 || Ty < 1) return 0;
    return align_up((size_t)B * 4 * Ty * sizeof(float), 256) + 256;
}

int aligner_softattn_backward_f32(const float *keys, const float *queries, const int32_t *t_xs, const float *prior,
                                  const float *grad_logp, const float *grad_soft, float *grad_keys_out,
                                  float *grad_queries_out, void *workspace, size_t workspace_bytes, int B, int C, int Tx,
                                  int Ty, float temperature, int sim, void *stream) {
    if (!grad_keys_out && !grad_queries_out) return fail(ALIGNER_EINVAL, "null pointer: both gradient outputs are NULL");
    if (!keys || !queries || !grad_logp || !workspace) return fail(ALIGNER_EINVAL, "null pointer");
    if (B < 0 || C < 1 || Tx < 1 || Ty < 1) return fail(ALIGNER_EINVAL, "bad shape B=%d C=%d Tx=%d Ty=%d", B, C, Tx, Ty);
    if (sim != ALIGNER_SIM_L2 && sim != ALIGNER_SIM_DOT) return fail(ALIGNER_EINVAL, "bad sim %d", sim);
    if (C > 256) return fail(ALIGNER_EDOM, "C=%d exceeds 256 attention channels", C);
    if (Tx > 512) return fail(ALIGNER_EDOM, "Tx=%d exceeds 512 text rows", Tx);
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if ((unsigned long long)B * ((Ty + 127) / 128) >= (1ull << 31)) return fail(ALIGNER_EDOM, "grid too large");
    if ((size_t)Tx * Ty >= (1u << 29) || (size_t)C * Ty >= (1u << 29)) return fail(ALIGNER_EDOM, "Tx*Ty=%zu exceeds 2^29", (size_t)Tx * Ty);
    const size_t need = aligner_softattn_backward_workspace_bytes(B, C, Tx, Ty);
    if (workspace_bytes < need) return fail(ALIGNER_ENOSPC, "workspace %zu < %zu bytes", workspace_bytes, need);
    if (B == 0) return ALIGNER_OK;
    SaBwdParams p{};
    p.keys = keys;
    p.queries = queries;
    p.t_xs = t_xs;
    p.prior = prior;
    p.gl = grad_logp;
    p.gs = grad_soft;
    p.dk = grad_keys_out;
    p.dq = grad_queries_out;
    p.stats = static_cast<float *>(workspace);
    p.B = B;
    p.C = C;
    p.Tx = Tx;
    p.Ty = Ty;
    p.temperature = temperature;
    p.l2 = sim == ALIGNER_SIM_L2;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (sb_nct(C)) {
        case 1: return sb_launch<1>(p, s);
        case 2: return sb_launch<2>(p, s);
        case 3: return sb_launch<3>(p, s);
        case 4: return sb_launch<4>(p, s);
        default: return sb_launch<8>(p, s);
    }
}

}  // extern "C"
