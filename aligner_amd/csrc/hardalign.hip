// The hard half of an OTA-style training step (not in the reference snapshot -- README.md:21-25,50 only points at the
// OTA paper -- so the spec is build-defined; parity with published code is unpinned):
//
//   segment reduction    tokens[b,c,x] = sum (or mean) of frames[b,c,y] over the frames token x owns under the
//                        durations: the adjoint of the length regulator (prior.hip: regulate_kernel, the same
//                        segments) and the per-token pitch / energy averaging
//   binarization loss    nll[b] = -sum over the frames of max(logp[b, tok[b,y], y], min_logp), and its gradient,
//                        which lives on the path's cells only: written as a whole tensor, or scattered into a
//                        gradient that is already there (the forward-sum one)
//
// The segment reduction is the hot one: it reads [B,C,Ty] once and writes [B,C,Tx].  A workgroup owns whole
// (utterance, channel) rows, so no segment is ever split between workgroups and nothing is combined through
// global memory: no atomics, one fixed summation order, the same bits on every run.  The work per frame does not
// depend on the durations: every wave streams 1 KiB runs of a row, reduces them with a segmented scan over the
// lanes keyed by the token, and only the lanes at a segment's end touch the wave's own per-token accumulators in LDS.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "aligner_amd.h"
#include "common.h"
#include "segments.h"

namespace aligner {

constexpr int SR_THREADS = DUR_SCAN_THREADS;    // (scan_durations, segments.h)
constexpr int SR_WAVES = SR_THREADS / 64;

// VEC frames per lane (4: 16-byte loads, rows 16-byte aligned; 1: any Ty / pointer), CW rows per wave and pass.
// LDS: ends[Tx] | wave_tot[4] | acc[SR_WAVES][CW][Tx] fp32.
// Keys, joins and the accumulation into acc: segments.h.
template <int VEC, int CW>
__global__ __launch_bounds__(SR_THREADS) void segment_reduce_kernel(const float *__restrict__ frames,
                                                                    const int *__restrict__ dur,
                                                                    float *__restrict__ tokens, int C, int Tx, int Ty,
                                                                    int mean) {
    extern __shared__ int sr_lds[];
    int *ends = sr_lds;
    int *wave_tot = ends + Tx;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *acc = reinterpret_cast<float *>(wave_tot + SR_WAVES) + (size_t)wave * CW * Tx;
    scan_durations(dur + (size_t)b * Tx, ends, wave_tot, Tx);
    for (int i = lane; i < CW * Tx; i += 64) acc[i] = 0.f;
    __builtin_amdgcn_wave_barrier();

    const int ngroups = (C + SR_WAVES * CW - 1) / (SR_WAVES * CW);
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int c0 = (grp * SR_WAVES + wave) * CW;          // this wave's rows: c0 .. c0+CW-1 (those below C)
        if (c0 >= C) continue;
        const float *row0 = frames + ((size_t)b * C + c0) * Ty;
        for (int base = 0; base < Ty; base += 64 * VEC) {
            const int y0 = base + lane * VEC;
            // the loads first (addresses clamped into the row: what a frame without an owner holds is never used)
            float v[CW][1][VEC];                              // (one quantity per frame)
            {
                const int yl = (y0 + VEC <= Ty) ? y0 : 0;
#pragma unroll
                for (int r = 0; r < CW; ++r) {
                    // a row past C (C not a multiple of CW) repeats row c0: loaded, scanned and accumulated like the
                    // others, into an accumulator row that is neither written out nor cleared -- which is safe
                    // because such a wave has no later group (grp only grows, so its next c0 is >= C)
                    const int c = (c0 + r < C) ? c0 + r : c0;
                    const float *p = row0 + (size_t)(c - c0) * Ty + yl;
                    if constexpr (VEC == 4) {
                        const float4 q = *reinterpret_cast<const float4 *>(p);
                        v[r][0][0] = q.x; v[r][0][1] = q.y; v[r][0][2] = q.z; v[r][0][3] = q.w;
                    } else {
                        v[r][0][0] = *p;
                    }
                }
            }
            int k[VEC];                                       // keys, joins: once per run, for the CW rows
            seg_keys<VEC>(ends, Tx, Ty, y0, k);
            const SegJoin join = seg_join<VEC>(k, lane);
#pragma unroll
            for (int r = 0; r < CW; ++r) seg_accumulate<VEC, 1>(v[r], k, Tx, acc + r * Tx, 0, join);
        }
        // write the rows out along x and clear the accumulators for the next pass
        for (int r = 0; r < CW && c0 + r < C; ++r) {
            float *a = acc + r * Tx;
            float *o = tokens + ((size_t)b * C + c0 + r) * Tx;
            for (int x = lane; x < Tx; x += 64) {
                float s = a[x];
                a[x] = 0.f;
                if (mean) {
                    int lo = x > 0 ? ends[x - 1] : 0, hi = ends[x];
                    lo = lo < Ty ? lo : Ty;
                    hi = hi < Ty ? hi : Ty;
                    s = hi > lo ? s / (float)(hi - lo) : 0.f;
                }
                o[x] = s;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__device__ inline float load_logp(const void *p, int dtype, size_t i) {
    if (dtype == ALIGNER_DT_F32) return static_cast<const float *>(p)[i];
    const unsigned short h = static_cast<const unsigned short *>(p)[i];
    if (dtype == ALIGNER_DT_BF16) return __builtin_bit_cast(float, (unsigned)h << 16);
    return (float)__builtin_bit_cast(_Float16, h);
}

// does frame (b, y) count, and is its cell above the floor?  returns the clamped log-prob
__device__ inline bool path_cell(const void *logp, int dtype, int ld, const int *tok, int b, int y, int Tx, int Ty,
                                 int ty, int *x_out, float *lp_out) {
    if (y >= ty) return false;
    const int x = tok[(size_t)b * Ty + y];
    if (x < 0 || x >= Tx) return false;
    *x_out = x;
    *lp_out = load_logp(logp, dtype, ((size_t)b * Tx + x) * ld + y);
    return true;
}

// One workgroup per utterance; thread t sums the frames t, t+256, ... in order, then a fixed tree over the lanes
// and the four waves in order: one summation order, whatever the machine does.
__global__ __launch_bounds__(256) void bin_loss_kernel(const void *__restrict__ logp, int dtype, int ld,
                                                       const int *__restrict__ tok, const int *__restrict__ t_ys,
                                                       float min_logp, float *__restrict__ nll,
                                                       int *__restrict__ count, int Tx, int Ty) {
    __shared__ float wsum[4];
    __shared__ int wcnt[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ty = clamp_len(t_ys, b, Ty);
    float s = 0.f;
    int n = 0;
    for (int y = tid; y < Ty; y += 256) {
        int x;
        float lp;
        if (path_cell(logp, dtype, ld, tok, b, y, Tx, Ty, ty, &x, &lp)) {
            s += (lp > min_logp) ? lp : min_logp;             // (NaN: the floor, like -inf)
            ++n;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o);
        n += __shfl_down(n, o);
    }
    if ((tid & 63) == 0) { wsum[tid >> 6] = s; wcnt[tid >> 6] = n; }
    __syncthreads();
    if (tid == 0) {
        nll[b] = -(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
        count[b] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
}

// accumulate: a thread per frame adds -scale[b] to its cell, touches nothing else
__global__ __launch_bounds__(256) void bin_grad_scatter_kernel(const void *__restrict__ logp, int dtype, int ld,
                                                               const int *__restrict__ tok,
                                                               const int *__restrict__ t_ys, float min_logp,
                                                               const float *__restrict__ scale,
                                                               float *__restrict__ grad, int Tx, int Ty) {
    const int b = blockIdx.y, y = blockIdx.x * 256 + threadIdx.x;
    if (y >= Ty) return;
    const int ty = clamp_len(t_ys, b, Ty);
    int x;
    float lp;
    if (path_cell(logp, dtype, ld, tok, b, y, Tx, Ty, ty, &x, &lp) && lp > min_logp)
        grad[((size_t)b * Tx + x) * Ty + y] -= scale[b];
}

// write: the whole [B,Tx,Ty] tensor, a streaming store.  A thread owns VEC frames and a slice of the rows
// (gridDim.z slices); it looks its cells up only where the token falls into its slice.
template <int VEC>
__global__ __launch_bounds__(256) void bin_grad_write_kernel(const void *__restrict__ logp, int dtype, int ld,
                                                             const int *__restrict__ tok,
                                                             const int *__restrict__ t_ys, float min_logp,
                                                             const float *__restrict__ scale,
                                                             float *__restrict__ grad, int Tx, int Ty) {
    const int b = blockIdx.y, y0 = (blockIdx.x * 256 + threadIdx.x) * VEC;
    if (y0 >= Ty) return;
    const int xpz = (Tx + gridDim.z - 1) / gridDim.z;
    const int x0 = blockIdx.z * xpz, x1 = (x0 + xpz < Tx) ? x0 + xpz : Tx;
    const int ty = clamp_len(t_ys, b, Ty);
    const float g = -scale[b];
    int hot[VEC];                                             // the row that gets g in this column, -1: none here
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        hot[j] = -1;
        const int y = y0 + j;
        if (y < ty) {
            const int x = tok[(size_t)b * Ty + y];
            if (x >= x0 && x < x1) {
                const float lp = load_logp(logp, dtype, ((size_t)b * Tx + x) * ld + y);
                if (lp > min_logp) hot[j] = x;
            }
        }
    }
    float *out = grad + (size_t)b * Tx * Ty + y0;
    for (int x = x0; x < x1; ++x) {
        if constexpr (VEC == 4) {
            float4 q;
            q.x = hot[0] == x ? g : 0.f;
            q.y = hot[1] == x ? g : 0.f;
            q.z = hot[2] == x ? g : 0.f;
            q.w = hot[3] == x ? g : 0.f;
            *reinterpret_cast<float4 *>(out + (size_t)x * Ty) = q;
        } else {
            out[(size_t)x * Ty] = hot[0] == x ? g : 0.f;
        }
    }
}

static int segment_reduce_rows_per_wave(int Tx) { return Tx <= 512 ? 4 : (Tx <= 1024 ? 2 : 1); }

template <int VEC, int CW>
static int launch_segment_reduce(const float *frames, const int32_t *dur, float *tokens, int B, int C, int Tx, int Ty,
                                 int mean, hipStream_t stream) {
    const size_t lds = segment_lds_bytes(Tx, SR_WAVES, CW);
    const int gx = segment_grid_x(B, (C + SR_WAVES * CW - 1) / (SR_WAVES * CW));
    hipLaunchKernelGGL((segment_reduce_kernel<VEC, CW>), dim3(gx, B), dim3(SR_THREADS), lds, stream, frames, dur,
                       tokens, C, Tx, Ty, mean);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

static bool logp_dtype_ok(int dt) { return dt == ALIGNER_DT_F32 || dt == ALIGNER_DT_BF16 || dt == ALIGNER_DT_F16; }

}  // namespace aligner

using namespace aligner;

extern "C" {

int aligner_segment_reduce_f32(const float *frames, const int32_t *durations, float *tokens_out, int B, int C, int Tx,
                               int Ty, int mean, void *stream) {
    if (!frames || !durations || !tokens_out) return fail(ALIGNER_EINVAL, "null pointer");
    if (B < 0 || C < 0 || Tx < 1 || Ty < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if (Tx > 2048) return fail(ALIGNER_EDOM, "Tx=%d too large (<= 2048)", Tx);
    if (B == 0 || C == 0) return ALIGNER_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool vec = (Ty % 4 == 0) && (reinterpret_cast<uintptr_t>(frames) % 16 == 0);
    switch (segment_reduce_rows_per_wave(Tx)) {
        case 4: return vec ? launch_segment_reduce<4, 4>(frames, durations, tokens_out, B, C, Tx, Ty, mean, s)
                           : launch_segment_reduce<1, 4>(frames, durations, tokens_out, B, C, Tx, Ty, mean, s);
        case 2: return vec ? launch_segment_reduce<4, 2>(frames, durations, tokens_out, B, C, Tx, Ty, mean, s)
                           : launch_segment_reduce<1, 2>(frames, durations, tokens_out, B, C, Tx, Ty, mean, s);
        default: return vec ? launch_segment_reduce<4, 1>(frames, durations, tokens_out, B, C, Tx, Ty, mean, s)
                            : launch_segment_reduce<1, 1>(frames, durations, tokens_out, B, C, Tx, Ty, mean, s);
    }
}

int aligner_bin_loss(const void *logp, int logp_dtype, int ld_logp, const int32_t *tok, const int32_t *t_ys,
                     float min_logp, float *nll_out, int32_t *count_out, int B, int Tx, int Ty, void *stream) {
    if (!logp || !tok || !nll_out || !count_out) return fail(ALIGNER_EINVAL, "null pointer");
    if (B < 0 || Tx < 1 || Ty < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (!logp_dtype_ok(logp_dtype)) return fail(ALIGNER_EINVAL, "logp_dtype %d (F32, BF16 or F16)", logp_dtype);
    if (ld_logp < Ty) return fail(ALIGNER_EINVAL, "ld_logp=%d < Ty=%d", ld_logp, Ty);
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if (Tx > 2048) return fail(ALIGNER_EDOM, "Tx=%d too large (<= 2048)", Tx);
    if (B == 0) return ALIGNER_OK;
    hipLaunchKernelGGL(bin_loss_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), logp, logp_dtype,
                       ld_logp, tok, t_ys, min_logp, nll_out, count_out, Tx, Ty);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

int aligner_bin_loss_grad_f32(const void *logp, int logp_dtype, int ld_logp, const int32_t *tok, const int32_t *t_ys,
                              float min_logp, const float *scale, float *grad, int accumulate, int B, int Tx, int Ty,
                              void *stream) {
    if (!logp || !tok || !scale || !grad) return fail(ALIGNER_EINVAL, "null pointer");
    if (B < 0 || Tx < 1 || Ty < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (!logp_dtype_ok(logp_dtype)) return fail(ALIGNER_EINVAL, "logp_dtype %d (F32, BF16 or F16)", logp_dtype);
    if (ld_logp < Ty) return fail(ALIGNER_EINVAL, "ld_logp=%d < Ty=%d", ld_logp, Ty);
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if (Tx > 2048) return fail(ALIGNER_EDOM, "Tx=%d too large (<= 2048)", Tx);
    if (B == 0) return ALIGNER_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (accumulate) {
        hipLaunchKernelGGL(bin_grad_scatter_kernel, dim3((Ty + 255) / 256, B), dim3(256), 0, s, logp, logp_dtype,
                           ld_logp, tok, t_ys, min_logp, scale, grad, Tx, Ty);
    } else {
        const bool vec = (Ty % 4 == 0) && (reinterpret_cast<uintptr_t>(grad) % 16 == 0);
        const int per = vec ? 4 : 1;
        const int gx = (Ty + 256 * per - 1) / (256 * per);
        int nz = 1;                                           // row slices: ~8 workgroups per CU, >= 4 rows each (a rule of thumb, as
                                                              // for the regulator's channel slices; no other split was timed)
        while (nz < 64 && (long)gx * B * nz < 2048 && Tx / (nz * 2) >= 4) nz *= 2;
        if (vec)
            hipLaunchKernelGGL(bin_grad_write_kernel<4>, dim3(gx, B, nz), dim3(256), 0, s, logp, logp_dtype, ld_logp,
                               tok, t_ys, min_logp, scale, grad, Tx, Ty);
        else
            hipLaunchKernelGGL(bin_grad_write_kernel<1>, dim3(gx, B, nz), dim3(256), 0, s, logp, logp_dtype, ld_logp,
                               tok, t_ys, min_logp, scale, grad, Tx, Ty);
    }
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

}  // extern "C"
