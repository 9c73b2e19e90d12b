// Gaussian upsampling (JETS, Non-Attentive Tacotron, Parallel Tacotron, ESPnet's GaussianUpsampling): the differentiable
// length regulator.  Frame y of utterance b sits at tau_y = y + frame_offset and takes a softmax-weighted mix of the token
// encodings, the weights Gaussians in the distance to each token's centre:
//
//   e[y,x]   = g[x] - a[x] (tau_y - c[x])^2            x < t_x
//   p[y,.]   = softmax over those x
//   out[:,y] = sum_x p[y,x] h[:,x]                      y < t_y; +0.0 beyond, and everywhere when t_x = 0
//
// and backward, with G = dL/dout (a frame that does not count contributes nothing),
//
//   q[y,x] = sum_c G[c,y] h[c,x]    r[y] = sum_x p q    de = p (q - r)
//   dh[c,x] = sum_y p[y,x] G[c,y]   dg[x] = sum_y de    da[x] = -sum_y de (tau_y - c_x)^2    dc[x] = sum_y de 2 a_x (tau_y - c_x)
//
// The weights are never stored.  ALIGNER_GAUSS_UP_CUT (aligner_amd.h) is the contract that makes a band legal: a token
// whose energy is more than CUT below the frame's maximum may count as zero, every other token is included.
//
// Kernels:
//   gauss_up_band_kernel     per tile of 64 frames the token interval [lo,hi) it needs.  With the centres non-decreasing over
//                            x < t_x: L = the smallest, over the tile's frames, of the energy of a token next to the frame
//                            (a lower bound of every frame's maximum); a token at distance D from the tile has energy at most
//                            gmax - amin D^2 on all of its frames, so it may go when that is below L - CUT: the interval of
//                            the centres within R = sqrt((gmax - L + CUT) / amin) of the tile, by two binary searches.
//                            Centres out of order, a precision that is not positive, anything not finite: [0, t_x).
//   gauss_up_mix_kernel      dst[c,i] = sum_j w(i,j) src[c,j], the lane owning i (64 per workgroup, stores coalesced along
//                            i), a wave 16 of the workgroup's 64 channels, j in chunks of 32: src transposed into LDS and
//                            read back as broadcast 16-byte rows, each weight computed once per workgroup and shared
//                            through LDS.  Forward: i a frame, j the band's tokens, w = exp(e - max) and one division by
//                            the denominator (summed in double) at the end.  dh: i a token, j the frames of every tile whose
//                            band reaches the token tile, w = exp(e - max_j) / den_j with the frame's max and 1/den from
//                            the workspace: a token owns its row of dh, nothing is reduced across workgroups.
//   gauss_up_frames_kernel   backward, a workgroup per frame tile: the frame's max and 1/den into the workspace; then q over
//                            ALL channels for the band's tokens (32 at a time in registers, the channels split over the
//                            waves and added through LDS in a fixed order), the sums over the tile's frames of p q, p q d,
//                            p q d^2 by wave reductions, r[y], and in a second sweep those of p r, p r d, p r d^2: six
//                            partials per (tile, band token) into the workspace.
//   gauss_up_finish_kernel   a thread per token adds the tiles' partials in tile order: dg, dc, da.
// No floating-point atomics anywhere: the same bits on every call.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "aligner_amd.h"
#include "common.h"
#include "device.h"

namespace aligner {

constexpr int GU_THREADS = 256;
constexpr int GU_WAVES = GU_THREADS / 64;
constexpr int GU_TILE = 64;                  // owned indices (frames, or tokens in the dh form) per workgroup: one per lane
constexpr int GU_CS = 64;                    // channels per workgroup of the mix kernel, GU_CS / GU_WAVES per wave
constexpr int GU_CPW = GU_CS / GU_WAVES;
constexpr int GU_JC = 32;                    // contracted indices per chunk
constexpr int GU_SRC_LD = GU_CS + 4;         // LDS row pitch of the transposed source chunk (16-byte rows stay aligned)
constexpr int GU_H_LD = GU_JC + 4;           // ... of the frames kernel's [channel][token] chunk
constexpr int GU_MAX_TX = 2048;

// the one statement of the energy: every kernel, and the tests' restatement, round it this way
__device__ inline float gu_energy(float tau, float c, float a, float g) {
    const float d = tau - c;
    return g - (a * d) * d;
}

__device__ inline float gu_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ inline float gu_wave_min(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

// band[(b * ntiles + tile) * 2 + {0,1}] = lo, hi.  Grid (ceil(ntiles / 4), B): a wave per tile, the lane a frame.
__global__ __launch_bounds__(GU_THREADS) void gauss_up_band_kernel(const float *__restrict__ cen,
                                                                   const float *__restrict__ prec,
                                                                   const float *__restrict__ lw,
                                                                   const int *__restrict__ t_xs,
                                                                   const int *__restrict__ t_ys, float off,
                                                                   int *__restrict__ band, int Tx, int Ty, int ntiles,
                                                                   int force_full) {
    __shared__ float s_c[GU_MAX_TX];
    __shared__ float s_amin[GU_WAVES], s_gmax[GU_WAVES];
    __shared__ int s_bad[GU_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int tx = clamp_len(t_xs, b, Tx), ty = clamp_len(t_ys, b, Ty);
    const float *cb = cen + (size_t)b * Tx, *ab = prec + (size_t)b * Tx;
    const float *gb = lw ? lw + (size_t)b * Tx : nullptr;
    float amin = INFINITY, gmax = -INFINITY;
    int bad = 0;
    for (int x = tid; x < tx; x += GU_THREADS) {
        const float cx = cb[x], ax = ab[x], gx = gb ? gb[x] : 0.f;
        s_c[x] = cx;
        bad |= !(ax > 0.f) || !(fabsf(ax) < INFINITY) || !(fabsf(cx) < INFINITY) || !(fabsf(gx) < INFINITY);
        if (x + 1 < tx) bad |= !(cx <= cb[x + 1]);
        amin = fminf(amin, ax);
        gmax = fmaxf(gmax, gx);
    }
    for (int o = 32; o > 0; o >>= 1) {
        amin = fminf(amin, __shfl_xor(amin, o));
        gmax = fmaxf(gmax, __shfl_xor(gmax, o));
        bad |= __shfl_xor(bad, o);
    }
    if (lane == 0) {
        s_amin[wave] = amin;
        s_gmax[wave] = gmax;
        s_bad[wave] = bad;
    }
    __syncthreads();
    for (int w = 0; w < GU_WAVES; ++w) {
        amin = fminf(amin, s_amin[w]);
        gmax = fmaxf(gmax, s_gmax[w]);
        bad |= s_bad[w];
    }
    const int tile = blockIdx.x * GU_WAVES + wave;
    if (tile >= ntiles) return;
    int lo = 0, hi = tx;
    const int y0 = tile * GU_TILE;
    if (tx == 0 || y0 >= ty) {
        hi = 0;                                               // nothing counts in this tile
    } else if (!bad && !force_full) {
        const int y = y0 + lane;
        const float tau = (float)y + off;
        float L = INFINITY;
        if (y < ty) {
            int l = 0, h = tx;                                // first x with c[x] >= tau
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (s_c[mid] >= tau) h = mid; else l = mid + 1;
            }
            const int x1 = l < tx ? l : tx - 1, x0 = l > 0 ? l - 1 : 0;
            const float e0 = gu_energy(tau, s_c[x0], ab[x0], gb ? gb[x0] : 0.f);
            const float e1 = gu_energy(tau, s_c[x1], ab[x1], gb ? gb[x1] : 0.f);
            L = fmaxf(e0, e1);
        }
        L = gu_wave_min(L);
        const int ylast = (y0 + GU_TILE - 1 < ty ? y0 + GU_TILE - 1 : ty - 1);
        const float tau0 = (float)y0 + off, tau1 = (float)ylast + off;
        // (the margins: the kernels' energies carry a few ulps of their magnitude, the centres one of theirs)
        const float span = (gmax - L) + ALIGNER_GAUSS_UP_CUT;
        const float R2 = (span + 1.f + 1e-5f * (fabsf(gmax) + fabsf(L))) / amin;
        const float R = sqrtf(R2) * 1.0001f + 1e-6f * (fabsf(tau0) + fabsf(tau1)) + 0.01f;
        if (R2 >= 0.f && R < INFINITY) {
            const float left = tau0 - R, right = tau1 + R;
            int l = 0, h = tx;                                // first x with c[x] >= left
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (s_c[mid] >= left) h = mid; else l = mid + 1;
            }
            lo = l;
            l = lo;
            h = tx;                                           // first x with c[x] > right
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (s_c[mid] > right) h = mid; else l = mid + 1;
            }
            hi = l;
        }
    }
    if (lane == 0) {
        band[((size_t)b * ntiles + tile) * 2] = lo;
        band[((size_t)b * ntiles + tile) * 2 + 1] = hi;
    }
}

// The frame's maximum energy over the tokens [jlo, jhi), the tokens dealt over the waves; every thread gets the result.
// s_red: GU_WAVES * 64 floats.  (Ends with a barrier; s_red may be reused after the next one.)
__device__ inline float gu_frame_max(const float *__restrict__ cb, const float *__restrict__ ab,
                                     const float *__restrict__ gb, float tau, int jlo, int jhi, int wave, int lane,
                                     float *s_red) {
    float m = -INFINITY;
    for (int j = jlo + wave; j < jhi; j += GU_WAVES) m = fmaxf(m, gu_energy(tau, cb[j], ab[j], gb ? gb[j] : 0.f));
    s_red[wave * 64 + lane] = m;
    __syncthreads();
    m = s_red[lane];
    for (int w = 1; w < GU_WAVES; ++w) m = fmaxf(m, s_red[w * 64 + lane]);
    return m;
}

// TOK false: forward.  src = h [B,C,Tx], dst = out [B,C,Ty]; grid (ntiles, ceil(C / 64), B).
// TOK true:  dh.       src = G [B,C,Ty], dst = dh  [B,C,Tx]; grid (ceil(Tx / 64), ceil(C / 64), B); fmax / finv [B,Ty] from
//                      gauss_up_frames_kernel.
template <bool TOK>
__global__ __launch_bounds__(GU_THREADS) void gauss_up_mix_kernel(const float *__restrict__ src,
                                                                  const float *__restrict__ cen,
                                                                  const float *__restrict__ prec,
                                                                  const float *__restrict__ lw,
                                                                  const int *__restrict__ t_xs,
                                                                  const int *__restrict__ t_ys, float off,
                                                                  const int *__restrict__ band,
                                                                  const float *__restrict__ fmax,
                                                                  const float *__restrict__ finv,
                                                                  float *__restrict__ dst, int C, int Tx, int Ty,
                                                                  int ntiles) {
    __shared__ __attribute__((aligned(16))) float s_src[GU_JC * GU_SRC_LD];
    __shared__ float s_w[GU_JC * GU_TILE];
    __shared__ float s_red[GU_WAVES * 64];
    __shared__ int s_rng[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x, c0 = blockIdx.y * GU_CS, b = blockIdx.z;
    const int tx = clamp_len(t_xs, b, Tx), ty = clamp_len(t_ys, b, Ty);
    const int I = TOK ? Tx : Ty, J = TOK ? Ty : Tx;
    const int i = tile * GU_TILE + lane;
    const bool valid = i < (TOK ? tx : ty);
    const float *cb = cen + (size_t)b * Tx, *ab = prec + (size_t)b * Tx;
    const float *gb = lw ? lw + (size_t)b * Tx : nullptr;
    int jlo, jhi;
    if constexpr (!TOK) {
        jlo = band[((size_t)b * ntiles + tile) * 2];
        jhi = band[((size_t)b * ntiles + tile) * 2 + 1];
    } else {
        // the frames of every tile whose band reaches this token tile (integer min / max: any order, the same result)
        if (tid == 0) {
            s_rng[0] = INT_MAX;
            s_rng[1] = 0;
        }
        __syncthreads();
        const int x0 = tile * GU_TILE, x1 = x0 + GU_TILE < tx ? x0 + GU_TILE : tx;
        for (int t = tid; t < ntiles; t += GU_THREADS) {
            const int lo = band[((size_t)b * ntiles + t) * 2], hi = band[((size_t)b * ntiles + t) * 2 + 1];
            if (hi > lo && lo < x1 && hi > x0) {
                atomicMin(&s_rng[0], t * GU_TILE);
                atomicMax(&s_rng[1], (t + 1) * GU_TILE);
            }
        }
        __syncthreads();
        jlo = s_rng[0];
        jhi = s_rng[1] < ty ? s_rng[1] : ty;
        if (jlo == INT_MAX) jlo = jhi = 0;
    }
    // the owned index's own operands
    float tau_i = 0.f, ci = 0.f, ai = 0.f, gi = 0.f, ref = 0.f;
    if constexpr (TOK) {
        const int xi = valid ? i : 0;                         // (valid: i < tx <= Tx; otherwise nothing of it is used)
        if (valid) {
            ci = cb[xi];
            ai = ab[xi];
            gi = gb ? gb[xi] : 0.f;
        }
    } else {
        tau_i = (float)i + off;
        ref = gu_frame_max(cb, ab, gb, tau_i, jlo, jhi, wave, lane, s_red);
    }
    float acc[GU_CPW];
#pragma unroll
    for (int k = 0; k < GU_CPW; ++k) acc[k] = 0.f;
    double den = 0.0;
    const float *sb = src + (size_t)b * C * J;
    for (int jc = jlo; jc < jhi; jc += GU_JC) {
        // the chunk of src, transposed: s_src[j][channel]
#pragma unroll
        for (int k = 0; k < GU_JC * GU_CS / GU_THREADS; ++k) {
            const int idx = tid + GU_THREADS * k;
            const int jj = idx & (GU_JC - 1), cc = idx / GU_JC;
            const int j = jc + jj, c = c0 + cc;
            s_src[jj * GU_SRC_LD + cc] = (j < jhi && c < C) ? sb[(size_t)c * J + j] : 0.f;
        }
        // the chunk's weights, each once: this wave's quarter of the chunk, the lane's owned index
#pragma unroll
        for (int k = 0; k < GU_JC / GU_WAVES; ++k) {
            const int jj = wave * (GU_JC / GU_WAVES) + k;
            const int j = jc + jj;
            float w = 0.f;
            if (j < jhi) {
                if constexpr (TOK) {
                    const float e = gu_energy((float)j + off, ci, ai, gi);
                    w = expf(e - fmax[(size_t)b * Ty + j]) * finv[(size_t)b * Ty + j];
                } else {
                    w = expf(gu_energy(tau_i, cb[j], ab[j], gb ? gb[j] : 0.f) - ref);
                }
            }
            s_w[jj * GU_TILE + lane] = valid ? w : 0.f;
        }
        __syncthreads();
        const int n = jhi - jc < GU_JC ? jhi - jc : GU_JC;
        for (int jj = 0; jj < n; ++jj) {
            const float w = s_w[jj * GU_TILE + lane];
            den += (double)w;
            const float4 *hp = reinterpret_cast<const float4 *>(&s_src[jj * GU_SRC_LD + wave * GU_CPW]);
#pragma unroll
            for (int k = 0; k < GU_CPW / 4; ++k) {
                const float4 v = hp[k];
                acc[4 * k + 0] = fmaf(w, v.x, acc[4 * k + 0]);
                acc[4 * k + 1] = fmaf(w, v.y, acc[4 * k + 1]);
                acc[4 * k + 2] = fmaf(w, v.z, acc[4 * k + 2]);
                acc[4 * k + 3] = fmaf(w, v.w, acc[4 * k + 3]);
            }
        }
        __syncthreads();
    }
    if (i >= I) return;
    const float fden = (float)den;
    const bool live = valid && (TOK || fden > 0.f);
#pragma unroll
    for (int k = 0; k < GU_CPW; ++k) {
        const int c = c0 + wave * GU_CPW + k;
        if (c < C) {
            float v = 0.f;
            if (live) v = TOK ? acc[k] : acc[k] / fden;
            __builtin_nontemporal_store(v, dst + ((size_t)b * C + c) * I + i);
        }
    }
}

// Backward, a workgroup per frame tile; grid (ntiles, B).  fmax / finv [B,Ty]: every frame below Ty is written.
// PARAMS: also part[((b * ntiles + tile) * 6 + k) * Tx + x] for the band's tokens x, k = 0..2: the sums over the tile's
// frames of p q, p q d, p q d^2; k = 3..5: of p r, p r d, p r d^2 (d = tau_y - c_x).
template <bool PARAMS>
__global__ __launch_bounds__(GU_THREADS) void gauss_up_frames_kernel(const float *__restrict__ gout,
                                                                     const float *__restrict__ h,
                                                                     const float *__restrict__ cen,
                                                                     const float *__restrict__ prec,
                                                                     const float *__restrict__ lw,
                                                                     const int *__restrict__ t_xs,
                                                                     const int *__restrict__ t_ys, float off,
                                                                     const int *__restrict__ band,
                                                                     float *__restrict__ fmax, float *__restrict__ finv,
                                                                     float *__restrict__ part, int C, int Tx, int Ty,
                                                                     int ntiles) {
    __shared__ __attribute__((aligned(16))) float s_h[PARAMS ? GU_CS * GU_H_LD : 4];
    __shared__ float s_q[PARAMS ? GU_WAVES * GU_JC * 64 : 1];
    __shared__ float s_red[GU_WAVES * 64];
    __shared__ double s_den[GU_WAVES * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x, b = blockIdx.y;
    const int ty = clamp_len(t_ys, b, Ty);
    const int y = tile * GU_TILE + lane;
    const bool valid = y < ty;
    const float tau = (float)y + off;
    const float *cb = cen + (size_t)b * Tx, *ab = prec + (size_t)b * Tx;
    const float *gb = lw ? lw + (size_t)b * Tx : nullptr;
    const int jlo = band[((size_t)b * ntiles + tile) * 2], jhi = band[((size_t)b * ntiles + tile) * 2 + 1];

    const float m = gu_frame_max(cb, ab, gb, tau, jlo, jhi, wave, lane, s_red);
    double dpart = 0.0;
    for (int j = jlo + wave; j < jhi; j += GU_WAVES)
        dpart += (double)expf(gu_energy(tau, cb[j], ab[j], gb ? gb[j] : 0.f) - m);
    s_den[wave * 64 + lane] = dpart;
    __syncthreads();
    const float fden = (float)(((s_den[lane] + s_den[64 + lane]) + s_den[128 + lane]) + s_den[192 + lane]);
    const float invl = (valid && fden > 0.f) ? 1.f / fden : 0.f;
    if (wave == 0 && y < Ty) {
        fmax[(size_t)b * Ty + y] = (valid && jhi > jlo) ? m : 0.f;
        finv[(size_t)b * Ty + y] = invl;
    }
    if constexpr (PARAMS) {
        const float *hb = h + (size_t)b * C * Tx;
        const float *grow = gout + (size_t)b * C * Ty + (y < Ty ? y : 0);
        float *pb = part + ((size_t)b * ntiles + tile) * 6 * Tx;
        float r = 0.f;                                        // this wave's tokens' share of r[y]
        for (int jc = jlo; jc < jhi; jc += GU_JC) {
            float q[GU_JC];
#pragma unroll
            for (int jj = 0; jj < GU_JC; ++jj) q[jj] = 0.f;
            for (int cc0 = 0; cc0 < C; cc0 += GU_CS) {
#pragma unroll
                for (int k = 0; k < GU_JC * GU_CS / GU_THREADS; ++k) {
                    const int idx = tid + GU_THREADS * k;
                    const int jj = idx & (GU_JC - 1), cc = idx / GU_JC;
                    const int j = jc + jj, c = cc0 + cc;
                    s_h[cc * GU_H_LD + jj] = (j < jhi && c < C) ? hb[(size_t)c * Tx + j] : 0.f;
                }
                __syncthreads();
#pragma unroll 4
                for (int k = 0; k < GU_CPW; ++k) {
                    const int c = cc0 + wave * GU_CPW + k;
                    const float gv = (valid && c < C) ? grow[(size_t)c * Ty] : 0.f;
                    const float4 *row = reinterpret_cast<const float4 *>(&s_h[(wave * GU_CPW + k) * GU_H_LD]);
#pragma unroll
                    for (int v4 = 0; v4 < GU_JC / 4; ++v4) {
                        const float4 v = row[v4];
                        q[4 * v4 + 0] = fmaf(gv, v.x, q[4 * v4 + 0]);
                        q[4 * v4 + 1] = fmaf(gv, v.y, q[4 * v4 + 1]);
                        q[4 * v4 + 2] = fmaf(gv, v.z, q[4 * v4 + 2]);
                        q[4 * v4 + 3] = fmaf(gv, v.w, q[4 * v4 + 3]);
                    }
                }
                __syncthreads();
            }
#pragma unroll
            for (int jj = 0; jj < GU_JC; ++jj) s_q[(wave * GU_JC + jj) * 64 + lane] = q[jj];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < GU_JC / GU_WAVES; ++k) {
                const int jj = wave * (GU_JC / GU_WAVES) + k;
                const int j = jc + jj;
                if (j < jhi) {                                // (wave-uniform)
                    const float qq = ((s_q[jj * 64 + lane] + s_q[(GU_JC + jj) * 64 + lane]) +
                                      s_q[(2 * GU_JC + jj) * 64 + lane]) + s_q[(3 * GU_JC + jj) * 64 + lane];
                    const float cj = cb[j], aj = ab[j], gj = gb ? gb[j] : 0.f;
                    const float d = tau - cj;
                    const float p = valid ? expf(gu_energy(tau, cj, aj, gj) - m) * invl : 0.f;
                    const float t0 = p * qq, t1 = t0 * d, t2 = t1 * d;
                    r += t0;
                    const float s0 = gu_wave_sum(t0), s1 = gu_wave_sum(t1), s2 = gu_wave_sum(t2);
                    if (lane == 0) {
                        pb[j] = s0;
                        pb[(size_t)Tx + j] = s1;
                        pb[(size_t)2 * Tx + j] = s2;
                    }
                }
            }
            __syncthreads();
        }
        s_red[wave * 64 + lane] = r;
        __syncthreads();
        r = ((s_red[lane] + s_red[64 + lane]) + s_red[128 + lane]) + s_red[192 + lane];
        for (int j = jlo + wave; j < jhi; j += GU_WAVES) {
            const float cj = cb[j], aj = ab[j], gj = gb ? gb[j] : 0.f;
            const float d = tau - cj;
            const float p = valid ? expf(gu_energy(tau, cj, aj, gj) - m) * invl : 0.f;
            const float u0 = p * r, u1 = u0 * d, u2 = u1 * d;
            const float s0 = gu_wave_sum(u0), s1 = gu_wave_sum(u1), s2 = gu_wave_sum(u2);
            if (lane == 0) {
                pb[(size_t)3 * Tx + j] = s0;
                pb[(size_t)4 * Tx + j] = s1;
                pb[(size_t)5 * Tx + j] = s2;
            }
        }
    }
}

// dg, dc, da: a thread per token, the tiles whose band holds it in tile order.  Grid (ceil(Tx / 256), B).
__global__ __launch_bounds__(GU_THREADS) void gauss_up_finish_kernel(const float *__restrict__ part,
                                                                     const int *__restrict__ band,
                                                                     const float *__restrict__ prec,
                                                                     const int *__restrict__ t_xs,
                                                                     float *__restrict__ dcen, float *__restrict__ dprec,
                                                                     float *__restrict__ dlw, int Tx, int ntiles) {
    const int b = blockIdx.y, x = blockIdx.x * GU_THREADS + threadIdx.x;
    if (x >= Tx) return;
    const int tx = clamp_len(t_xs, b, Tx);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (x < tx) {
        for (int t = 0; t < ntiles; ++t) {
            const int lo = band[((size_t)b * ntiles + t) * 2], hi = band[((size_t)b * ntiles + t) * 2 + 1];
            if (x >= lo && x < hi) {
                const float *pb = part + ((size_t)b * ntiles + t) * 6 * Tx + x;
                s0 += pb[0] - pb[(size_t)3 * Tx];
                s1 += pb[(size_t)Tx] - pb[(size_t)4 * Tx];
                s2 += pb[(size_t)2 * Tx] - pb[(size_t)5 * Tx];
            }
        }
    }
    const size_t o = (size_t)b * Tx + x;
    const bool live = x < tx;
    if (dlw) dlw[o] = live ? s0 : 0.f;
    if (dcen) dcen[o] = live ? (2.f * prec[o]) * s1 : 0.f;
    if (dprec) dprec[o] = live ? 0.f - s2 : 0.f;
}

static int gu_ntiles(int Ty) { return (Ty + GU_TILE - 1) / GU_TILE; }
static bool gu_shape_ok(int B, int C, int Tx, int Ty) {
    return B >= 1 && C >= 1 && Tx >= 1 && Ty >= 1 && B <= 65535 && Tx <= GU_MAX_TX && C <= 65535 * GU_CS;
}
static size_t gu_band_bytes(int B, int Ty) { return align_up((size_t)B * gu_ntiles(Ty) * 2 * sizeof(int), 256); }
static size_t gu_frame_bytes(int B, int Ty) { return align_up((size_t)B * Ty * sizeof(float), 256); }

static int gu_check_shape(int B, int C, int Tx, int Ty) {
    if (B < 1 || C < 1 || Tx < 1 || Ty < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if (Tx > GU_MAX_TX) return fail(ALIGNER_EDOM, "Tx=%d too large (<= %d)", Tx, GU_MAX_TX);
    if (C > 65535 * GU_CS) return fail(ALIGNER_EDOM, "C=%d too large", C);
    return ALIGNER_OK;
}

}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_gauss_upsample_workspace_bytes(int B, int C, int Tx, int Ty) {
    if (!gu_shape_ok(B, C, Tx, Ty)) return 0;
    return gu_band_bytes(B, Ty);
}

int aligner_gauss_upsample_f32(const float *h, const float *centre, const float *precision, const float *log_weight,
                               const int32_t *t_xs, const int32_t *t_ys, float frame_offset, float *out, void *workspace,
                               size_t workspace_bytes, int B, int C, int Tx, int Ty, void *stream) {
    if (!h || !centre || !precision || !out || !workspace) return fail(ALIGNER_EINVAL, "null pointer");
    const int rc = gu_check_shape(B, C, Tx, Ty);
    if (rc != ALIGNER_OK) return rc;
    const size_t need = aligner_gauss_upsample_workspace_bytes(B, C, Tx, Ty);
    if (workspace_bytes < need)
        return fail(ALIGNER_ENOSPC, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ntiles = gu_ntiles(Ty);
    int *band = static_cast<int *>(workspace);
    hipLaunchKernelGGL(gauss_up_band_kernel, dim3((ntiles + GU_WAVES - 1) / GU_WAVES, B), dim3(GU_THREADS), 0, s, centre,
                       precision, log_weight, t_xs, t_ys, frame_offset, band, Tx, Ty, ntiles, g_opt_gaussup_full_range);
    ALIGNER_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((gauss_up_mix_kernel<false>), dim3(ntiles, (C + GU_CS - 1) / GU_CS, B), dim3(GU_THREADS), 0, s, h,
                       centre, precision, log_weight, t_xs, t_ys, frame_offset, band, nullptr, nullptr, out, C, Tx, Ty,
                       ntiles);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

size_t aligner_gauss_upsample_backward_workspace_bytes(int B, int C, int Tx, int Ty) {
    if (!gu_shape_ok(B, C, Tx, Ty)) return 0;
    return gu_band_bytes(B, Ty) + 2 * gu_frame_bytes(B, Ty) +
           align_up((size_t)B * gu_ntiles(Ty) * 6 * Tx * sizeof(float), 256);
}

int aligner_gauss_upsample_backward_f32(const float *h, const float *centre, const float *precision,
                                        const float *log_weight, const int32_t *t_xs, const int32_t *t_ys,
                                        float frame_offset, const float *g_out, float *dh, float *dcentre,
                                        float *dprecision, float *dlog_weight, void *workspace, size_t workspace_bytes,
                                        int B, int C, int Tx, int Ty, void *stream) {
    if (!h || !centre || !precision || !g_out || !workspace) return fail(ALIGNER_EINVAL, "null pointer");
    if (!dh && !dcentre && !dprecision && !dlog_weight) return fail(ALIGNER_EINVAL, "no output requested");
    const int rc = gu_check_shape(B, C, Tx, Ty);
    if (rc != ALIGNER_OK) return rc;
    const size_t need = aligner_gauss_upsample_backward_workspace_bytes(B, C, Tx, Ty);
    if (workspace_bytes < need)
        return fail(ALIGNER_ENOSPC, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ntiles = gu_ntiles(Ty);
    char *ws = static_cast<char *>(workspace);
    int *band = reinterpret_cast<int *>(ws);
    float *fmax = reinterpret_cast<float *>(ws + gu_band_bytes(B, Ty));
    float *finv = reinterpret_cast<float *>(ws + gu_band_bytes(B, Ty) + gu_frame_bytes(B, Ty));
    float *part = reinterpret_cast<float *>(ws + gu_band_bytes(B, Ty) + 2 * gu_frame_bytes(B, Ty));
    const bool params = dcentre || dprecision || dlog_weight;
    hipLaunchKernelGGL(gauss_up_band_kernel, dim3((ntiles + GU_WAVES - 1) / GU_WAVES, B), dim3(GU_THREADS), 0, s, centre,
                       precision, log_weight, t_xs, t_ys, frame_offset, band, Tx, Ty, ntiles, g_opt_gaussup_full_range);
    ALIGNER_HIP_CHECK(hipGetLastError());
    if (params) {
        hipLaunchKernelGGL((gauss_up_frames_kernel<true>), dim3(ntiles, B), dim3(GU_THREADS), 0, s, g_out, h, centre,
                           precision, log_weight, t_xs, t_ys, frame_offset, band, fmax, finv, part, C, Tx, Ty, ntiles);
        ALIGNER_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(gauss_up_finish_kernel, dim3((Tx + GU_THREADS - 1) / GU_THREADS, B), dim3(GU_THREADS), 0, s,
                           part, band, precision, t_xs, dcentre, dprecision, dlog_weight, Tx, ntiles);
        ALIGNER_HIP_CHECK(hipGetLastError());
    } else {
        hipLaunchKernelGGL((gauss_up_frames_kernel<false>), dim3(ntiles, B), dim3(GU_THREADS), 0, s, g_out, h, centre,
                           precision, log_weight, t_xs, t_ys, frame_offset, band, fmax, finv, part, C, Tx, Ty, ntiles);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    if (dh) {
        hipLaunchKernelGGL((gauss_up_mix_kernel<true>), dim3((Tx + GU_TILE - 1) / GU_TILE, (C + GU_CS - 1) / GU_CS, B),
                           dim3(GU_THREADS), 0, s, g_out, centre, precision, log_weight, t_xs, t_ys, frame_offset, band,
                           fmax, finv, dh, C, Tx, Ty, ntiles);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

}  // extern "C"
