// Glow-TTS / VITS log-likelihood front end on MI355X (gfx950): the `value` tensor those models hand to
// monotonic_align.maximum_path -- the log-density of every latent frame under every token's diagonal Gaussian:
//
//   value[b,i,j] = sum_c ( -1/2 ln 2pi - s[b,c,i] - 1/2 (z[b,c,j] - m[b,c,i])^2 exp(-2 s[b,c,i]) )
//
// m, s [B,C,Tx] (the text encoder's mean and log-std), z [B,C,Ty] (the flow's output), value [B,Tx,Ty].  No softmax, no
// gradient (both models compute it under no_grad).  Cells outside an utterance's lengths are written as 0.0.
//
// The sum is a contraction of depth 2C plus a per-token constant:
//
//   value[i,j] = sum_c w[c,i] (-1/2 z[c,j]^2) + sum_c (m w)[c,i] z[c,j] + k[i]
//   w = exp(-2 s),   k[i] = sum_c ( -1/2 ln 2pi - s - 1/2 m^2 w )
//
// so it runs on the bf16 matrix cores the way softattn.hip's and convgemm.hip's products do: every fp32 operand is
// split x = hi + lo into two bf16 halves and a product is three v_mfma_f32_32x32x16_bf16 (hi*hi + hi*lo + lo*hi, fp32
// accumulate, ~2^-16 relative per product).  The terms cancel where z ~ m and sigma is small; the error is bounded
// against the magnitude of what is summed (tests/gausslogp_oracle.py), and no per-channel shift is applied.
//
//  * gauss_prep_kernel, once per call: w, m w and k[i]; the [Tx, 2C] operand split into bf16 halves in A-fragment order
//    (k-steps 0 .. KSc-1 hold w, KSc .. 2 KSc - 1 hold m w, channels padded with zeros to a multiple of 16, row tiles to
//    an even count), into the workspace.
//  * gauss_logp_kernel: a workgroup = 4 waves = 64 frames of one utterance and ALL its text rows.  It reads its
//    [C, 64] block of z once, forms -1/2 z^2 and z, splits them and keeps the B fragments in LDS.  A wave then owns a
//    pair of row tiles at a time: 2 x 2 accumulator tiles (64 rows x 64 frames), A fragments from the workspace (they stay
//    in L2: with B a multiple of 8 an utterance's workgroups share an XCD), one k-step ahead of their MFMAs, 12 MFMAs
//    per k-step for 8 fragments read.  There is no statistic across rows or frames: tiles are independent, one barrier a
//    workgroup.  Row tiles past t_x and frame blocks past t_y skip the contraction and store zeros.
//  * Stores: k[i] added, lengths applied, 32 consecutive frames of a row per half wave, through a buffer resource over
//    the utterance's [Tx, ld] block (sc1: written through, nothing of the output is read again here).
//  * No atomics, fixed summation order: the same bits on every call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "aligner_amd.h"
#include "common.h"
#include "device.h"

namespace aligner {

struct GaussParams {
    const float *z;         // [B,C,Ty]
    const float *mean;      // [B,C,Tx]
    const float *logstd;    // [B,C,Tx]
    const int *t_xs;        // nullable
    const int *t_ys;        // nullable
    void *out;              // [B,Tx,ld] fp32 or bf16
    uint4 *frag_hi;         // [B][RTP][2 KSc][64] A fragments, bf16 high halves
    uint4 *frag_lo;         // same, low halves
    float *kc;              // [B][RTP*32] per-token constant
    int RTP;                // row tiles of 32 text rows, rounded up to an even count
    int KSc;                // k-steps of 16 channels per half of the contraction
    int NQ;                 // frame blocks per utterance
    int B, C, Tx, Ty, ld;
};

constexpr int GL_STRIPS = 2;                      // 32-frame strips per workgroup
constexpr int GL_WAVES = 4;
constexpr int GL_THREADS = GL_WAVES * 64;
constexpr int GL_ST_AUX = 16;                     // sc1
constexpr float HALF_LN_2PI = 0.91893853320467274178f;

// One workgroup per (row tile, utterance).  Lane (row i = 32 r + lane&31, channel half lane>>5) of k-step s holds channels
// 16 s + 8 (lane>>5) + jj: A[i][k] of v_mfma_f32_32x32x16_bf16.
__global__ __launch_bounds__(256) void gauss_prep_kernel(GaussParams p) {
    __shared__ float part[32][33];                // [row][2 KSc partial sums of k], KSc <= 16
    const int tid = threadIdx.x;
    const int r = blockIdx.x, b = blockIdx.y;
    const int KSc = p.KSc, KS = 2 * KSc;
    const float *Mb = p.mean + (size_t)b * p.C * p.Tx;
    const float *Sb = p.logstd + (size_t)b * p.C * p.Tx;
    for (int idx = tid; idx < KSc * 64; idx += 256) {
        const int ln = idx & 63, s = idx >> 6;
        const int i = 32 * r + (ln & 31);
        const int c0 = 16 * s + 8 * (ln >> 5);
        bf16x8 wh, wl, mh, ml;
        float acc = 0.f;
        // all 16 loads first, unconditional (clamped address): a guarded load is waited for before the next one is issued
        const int ic = i < p.Tx ? i : p.Tx - 1;
        float mv[8], sv[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int c = c0 + jj < p.C ? c0 + jj : p.C - 1;
            mv[jj] = Mb[(size_t)c * p.Tx + ic];
            sv[jj] = Sb[(size_t)c * p.Tx + ic];
        }
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const unsigned ok = (i < p.Tx && c0 + jj < p.C) ? ~0u : 0u;      // padding: w = m w = 0, nothing added to k
            const float m = mv[jj], sd = sv[jj];
            const float w = and_mask(expf(-2.0f * sd), ok);
            const float mw = and_mask(m * w, ok);
            acc += and_mask((-HALF_LN_2PI - sd) - 0.5f * (m * mw), ok);
            __bf16 h, l;
            split_bf16(w, h, l);
            wh[jj] = h;
            wl[jj] = l;
            split_bf16(mw, h, l);
            mh[jj] = h;
            ml[jj] = l;
        }
        const size_t o = ((size_t)(b * p.RTP + r) * KS + s) * 64 + ln;
        p.frag_hi[o] = __builtin_bit_cast(uint4, wh);
        p.frag_lo[o] = __builtin_bit_cast(uint4, wl);
        p.frag_hi[o + (size_t)KSc * 64] = __builtin_bit_cast(uint4, mh);
        p.frag_lo[o + (size_t)KSc * 64] = __builtin_bit_cast(uint4, ml);
        part[ln & 31][2 * s + (ln >> 5)] = acc;
    }
    __syncthreads();
    if (tid < 32) {
        float acc = 0.f;
        for (int j = 0; j < 2 * KSc; ++j) acc += part[tid][j];       // fixed order: deterministic
        p.kc[(size_t)(b * p.RTP + r) * 32 + tid] = acc;
    }
}

template <bool OUT16>
__global__ __launch_bounds__(GL_THREADS) void gauss_logp_kernel(GaussParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gl_smem[];
    uint4 *frg = reinterpret_cast<uint4 *>(gl_smem);      // [GL_STRIPS][KS][hi, lo][64] B fragments

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int KSc = p.KSc, KS = 2 * KSc;
    int b, fq;
    xcd_block_map(p.B, p.NQ, blockIdx.x, b, fq);  // the workgroups of one utterance on one XCD: its A fragments stay in that L2
    const int f0 = 32 * GL_STRIPS * fq;
    int tx, ty;
    utterance_lengths(p.t_xs, p.t_ys, b, p.Tx, p.Ty, tx, ty);
    const bool live = f0 < ty;                    // (workgroup-uniform) any cell of this frame block inside the lengths

    if (live) {
        // z block -> B fragments: lane (frame l31 of strip st, channel half) takes channels 16 kc + 8 half + jj; -1/2 z^2 is
        // k-step kc, z is k-step KSc + kc.  Loads are unconditional (clamped address, masked value).
        const float *Zb = p.z + (size_t)b * p.C * p.Ty;
        for (int idx = tid; idx < GL_STRIPS * KSc * 64; idx += GL_THREADS) {
            const int ln = idx & 63, t = idx >> 6;
            const int st = t % GL_STRIPS, kc = t / GL_STRIPS;
            const int col = f0 + 32 * st + (ln & 31);
            const int colc = col < p.Ty ? col : p.Ty - 1;
            const int c0 = 16 * kc + 8 * (ln >> 5);
            float v[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int c = c0 + jj;
                const float x = Zb[(size_t)(c < p.C ? c : p.C - 1) * p.Ty + colc];
                v[jj] = and_mask(x, (c < p.C && col < p.Ty) ? ~0u : 0u);
            }
            bf16x8 qh, ql, zh, zl;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                __bf16 h, l;
                split_bf16(-0.5f * (v[jj] * v[jj]), h, l);
                qh[jj] = h;
                ql[jj] = l;
                split_bf16(v[jj], h, l);
                zh[jj] = h;
                zl[jj] = l;
            }
            uint4 *F = frg + (size_t)(st * KS + kc) * 128 + ln;
            F[0] = __builtin_bit_cast(uint4, qh);
            F[64] = __builtin_bit_cast(uint4, ql);
            F[(size_t)KSc * 128] = __builtin_bit_cast(uint4, zh);
            F[(size_t)KSc * 128 + 64] = __builtin_bit_cast(uint4, zl);
        }
    }
    __syncthreads();

    // the utterance's [Tx, ld] block as a buffer resource; a lane whose cell does not exist carries an offset beyond it
    constexpr unsigned esz = OUT16 ? 2u : 4u;
    const __amdgpu_buffer_rsrc_t out_rs =
        utterance_rsrc(static_cast<unsigned char *>(p.out) + (size_t)b * p.Tx * p.ld * esz, (unsigned)p.Tx * (unsigned)p.ld * esz);

    for (int pr = wave; 2 * pr < p.RTP; pr += GL_WAVES) {
        f32x16 acc[2][GL_STRIPS];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < GL_STRIPS; ++u)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t][u][e] = 0.f;
        if (live && 64 * pr < tx) {
            const uint4 *Ah = p.frag_hi + ((size_t)(b * p.RTP + 2 * pr) * KS) * 64 + lane;
            const uint4 *Al = p.frag_lo + ((size_t)(b * p.RTP + 2 * pr) * KS) * 64 + lane;
            const size_t tstep = (size_t)KS * 64;         // one row tile
            // Two register sets of A fragments, the loop unrolled by two (KS is even): the set of k-step s + 1 is asked for
            // in front of k-step s's MFMAs and not touched before they are through -- no copies, and the scheduler cannot
            // sink a load to just before its use (an L2 round trip exposed per fragment) across the barriers.
            uint4 a0[4], a1[4];
            auto load_a = [&](uint4 (&a)[4], int s) {
                const size_t so = (size_t)(s < KS ? s : KS - 1) * 64;         // (past the last k-step: the last one again)
                a[0] = Ah[so];
                a[1] = Al[so];
                a[2] = Ah[tstep + so];
                a[3] = Al[tstep + so];
            };
            auto kstep = [&](const uint4 (&a)[4], uint4 (&an)[4], int s) __attribute__((always_inline)) {
                bf16x8 ah[2], al[2], bh[GL_STRIPS], bl[GL_STRIPS];
                load_a(an, s + 1);
#pragma unroll
                for (int u = 0; u < GL_STRIPS; ++u) {
                    const uint4 *F = frg + (size_t)(u * KS + s) * 128 + lane;
                    bh[u] = __builtin_bit_cast(bf16x8, F[0]);
                    bl[u] = __builtin_bit_cast(bf16x8, F[64]);
                }
                __builtin_amdgcn_sched_barrier(0);
                ah[0] = __builtin_bit_cast(bf16x8, a[0]);
                al[0] = __builtin_bit_cast(bf16x8, a[1]);
                ah[1] = __builtin_bit_cast(bf16x8, a[2]);
                al[1] = __builtin_bit_cast(bf16x8, a[3]);
                // the small terms first; consecutive MFMAs write different accumulators
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int u = 0; u < GL_STRIPS; ++u)
                        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[t], bh[u], acc[t][u], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int u = 0; u < GL_STRIPS; ++u)
                        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bl[u], acc[t][u], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int u = 0; u < GL_STRIPS; ++u)
                        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bh[u], acc[t][u], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            };
            load_a(a0, 0);
            for (int s = 0; s < KS; s += 2) {
                kstep(a0, a1, s);
                kstep(a1, a0, s + 1);
            }
        }
        // C/D layout: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int tile = 2 * pr + t;
            if (32 * tile >= p.Tx) continue;              // (wave-uniform) the padding tile of an odd count
            const float *kp = p.kc + (size_t)(b * p.RTP + tile) * 32 + 4 * half;
            float4 kq[4];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) kq[gq] = *reinterpret_cast<const float4 *>(kp + 8 * gq);
#pragma unroll
            for (int u = 0; u < GL_STRIPS; ++u) {
                const int col = f0 + 32 * u + l31;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = 32 * tile + (e & 3) + 8 * (e >> 2) + 4 * half;
                    const float kv = (e & 3) == 0 ? kq[e >> 2].x : (e & 3) == 1 ? kq[e >> 2].y : (e & 3) == 2 ? kq[e >> 2].z : kq[e >> 2].w;
                    const float v = (row < tx && col < ty) ? acc[t][u][e] + kv : 0.f;
                    const unsigned off = (row < p.Tx && col < p.Ty) ? ((unsigned)row * (unsigned)p.ld + (unsigned)col) * esz : 0x80000000u;
                    if (!OUT16) {
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), out_rs, off, 0, GL_ST_AUX);
                    } else {
                        const __bf16 hv = (__bf16)v;
                        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, hv), out_rs, off, 0, GL_ST_AUX);
                    }
                }
            }
        }
    }
}

struct GlLayout { size_t hi_off, lo_off, kc_off, total; int RTP, KSc; };

static GlLayout gl_layout(int B, int C, int Tx) {
    GlLayout L;
    L.RTP = ((Tx + 31) / 32 + 1) & ~1;
    L.KSc = (C + 15) / 16;
    const size_t frag = (size_t)B * L.RTP * (2 * L.KSc) * 64 * sizeof(uint4);
    L.hi_off = 0;
    L.lo_off = align_up(frag, 256);
    L.kc_off = L.lo_off + align_up(frag, 256);
    L.total = L.kc_off + align_up((size_t)B * L.RTP * 32 * sizeof(float), 256);
    return L;
}

}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_gauss_logp_workspace_bytes(int B, int C, int Tx) {
    if (B < 1 || C < 1 || Tx < 1 || C > 256 || Tx > 1024) return 0;
    return gl_layout(B, C, Tx).total;
}

int aligner_gauss_logp(const float *z, const float *mean, const float *logstd, const int32_t *t_xs, const int32_t *t_ys,
                       void *value_out, int value_dtype, int ld_value, void *workspace, size_t workspace_bytes,
                       int B, int C, int Tx, int Ty, void *stream) {
    if (!z || !mean || !logstd || !value_out || !workspace) return fail(ALIGNER_EINVAL, "null pointer");
    if (B < 0 || C < 1 || Tx < 1 || Ty < 1) return fail(ALIGNER_EINVAL, "bad shape B=%d C=%d Tx=%d Ty=%d", B, C, Tx, Ty);
    if (ld_value < Ty) return fail(ALIGNER_EINVAL, "ld_value=%d < Ty=%d", ld_value, Ty);
    if (value_dtype != ALIGNER_DT_F32 && value_dtype != ALIGNER_DT_BF16)
        return fail(ALIGNER_EINVAL, "value dtype %d not supported (F32 or BF16)", value_dtype);
    const int esz = value_dtype == ALIGNER_DT_BF16 ? 2 : 4;
    if (ld_value != Ty && ((size_t)ld_value * esz) % 16 != 0)
        return fail(ALIGNER_EINVAL, "ld_value=%d: rows must start on 16-byte boundaries", ld_value);
    if (C > 256) return fail(ALIGNER_EDOM, "C=%d exceeds 256 channels", C);
    if (Tx > 1024) return fail(ALIGNER_EDOM, "Tx=%d exceeds 1024 text rows", Tx);
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if ((size_t)Tx * (size_t)ld_value >= (1ull << 29))    // an utterance's block is one buffer resource (32-bit offsets)
        return fail(ALIGNER_EDOM, "Tx*ld=%zu exceeds 2^29", (size_t)Tx * ld_value);
    const int NQ = (Ty + 32 * GL_STRIPS - 1) / (32 * GL_STRIPS);
    if ((unsigned long long)NQ * (unsigned long long)B >= (1ull << 31))
        return fail(ALIGNER_EDOM, "B*ceil(Ty/%d)=%llu workgroups exceed 2^31", 32 * GL_STRIPS, (unsigned long long)NQ * B);
    if (B == 0) return ALIGNER_OK;
    const GlLayout L = gl_layout(B, C, Tx);
    if (workspace_bytes < L.total) return fail(ALIGNER_ENOSPC, "workspace %zu < %zu bytes", workspace_bytes, L.total);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    GaussParams p{z, mean, logstd, t_xs, t_ys, value_out,
                  reinterpret_cast<uint4 *>(ws + L.hi_off), reinterpret_cast<uint4 *>(ws + L.lo_off),
                  reinterpret_cast<float *>(ws + L.kc_off), L.RTP, L.KSc, NQ, B, C, Tx, Ty, ld_value};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gauss_prep_kernel, dim3(L.RTP, B), dim3(256), 0, s, p);
    ALIGNER_HIP_CHECK(hipGetLastError());
    const size_t lds = (size_t)GL_STRIPS * (2 * L.KSc) * 2 * 64 * sizeof(uint4);      // <= 128 KiB (C = 256)
    auto kern = value_dtype == ALIGNER_DT_BF16 ? gauss_logp_kernel<true> : gauss_logp_kernel<false>;
    ALIGNER_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)NQ * (unsigned)B), dim3(GL_THREADS), lds, s, p);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

}  // extern "C"
