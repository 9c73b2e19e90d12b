// Weight / bias gradient of the encoders' convolution (convgemm.hip) on MI355X (gfx950).
//
// For y = act(conv1d(x, w, b)) with "same" padding, K in {1, 3, 5}, act = ReLU or none:
//   dYpre       = 0 where y <= 0, dY elsewhere -- torch.relu's rule: a NaN y passes its cotangent  (dY without an activation)
//   db[o]       = sum_{b,t} dYpre[b,o,t]
//   dW[o,i,tap] = sum_{b,t} dYpre[b,o,t] x[b,i,t+tap-K/2]
// A GEMM M = Cout, N = Cin K over the reduction index (b, t), both operands with t contiguous.  The input gradient is the
// forward convolution of dYpre with the transposed weights (aligner_conv1d_prepare_transposed_f32); the ReLU mask is
// applied while dY is read, and the masked cotangent is written once (by the workgroups of the first column tile) for it.
//
// conv_bwd_w_kernel: 4 waves, a 128 x 128 output tile (64 x 64 a wave), the reduction in chunks of 32 frames of one
// utterance staged through LDS (the next chunk's loads in flight during this one's MFMAs), exact fp32 products
// (v_mfma_f32_32x32x2f32).  The reduction is split over
// `nsplit` workgroups per tile (a function of the shape only); their partials go to the workspace and
// conv_bwd_reduce_kernel sums them in split order: no atomics, the same bits on every call.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "aligner_amd.h"
#include "common.h"
#include "device.h"

namespace aligner {

constexpr int CW_TILE = 128, CW_CHUNK = 32, CW_P = CW_CHUNK + 1, CW_PER = CW_TILE * CW_CHUNK / 256;

struct ConvBwdParams {
    const float *x;      // [B,Cin,T]
    const float *y;      // [B,Cout,T] (relu only)
    const float *gy;     // [B,Cout,T]
    float *gyp;          // nullable [B,Cout,T]: dYpre
    float *part;         // [nsplit][Cout][Cin K]
    float *dbpart;       // nullable [nsplit][Cout]
    int B, Cin, Cout, T, K, relu, N, nsplit, NTt;
};

__device__ __forceinline__ float cw_gy(const ConvBwdParams &p, size_t idx) {
    const float g = p.gy[idx];
    return (p.relu && p.y[idx] <= 0.f) ? 0.f : g;
}

// one chunk (utterance b, frames t0 .. t0 + 31) of both operands into registers: element j of a thread is
// row (tid + 256 j) >> 5, frame (tid + 256 j) & 31 of the 128-row tile (A: output channels, B: (input channel, tap))
struct CwChunk {
    float a[CW_PER], m[CW_PER], bx[CW_PER];
};

__device__ __forceinline__ void cw_load(const ConvBwdParams &p, CwChunk &r, int b, int t0, int o0, int n0, int tid) {
    const int hk = p.K / 2;
    // per-utterance bases (uniform) + 32-bit offsets (Cout T, Cin T < 2^31): one VGPR an address
    const float *gyb = p.gy + (size_t)b * p.Cout * p.T, *yb = p.relu ? p.y + (size_t)b * p.Cout * p.T : nullptr;
    const float *xb = p.x + (size_t)b * p.Cin * p.T;
#pragma unroll
    for (int j = 0; j < CW_PER; ++j) {
        const int idx = tid + 256 * j, rl = idx >> 5, t = t0 + (idx & 31);
        const int o = o0 + rl, n = n0 + rl;
        r.a[j] = 0.f;
        r.m[j] = 1.f;
        if (o < p.Cout && t < p.T) {
            r.a[j] = gyb[o * p.T + t];
            if (yb) r.m[j] = yb[o * p.T + t];
        }
        r.bx[j] = 0.f;
        if (n < p.N && t < p.T) {
            const int i = n / p.K, ts = t + (n - i * p.K) - hk;
            if (ts >= 0 && ts < p.T) r.bx[j] = xb[i * p.T + ts];
        }
    }
}

__global__ __launch_bounds__(256) void conv_bwd_w_kernel(ConvBwdParams p) {
    __shared__ float As[CW_TILE * CW_P];     // dYpre[o0 + ol][t0 + tt]
    __shared__ float Bs[CW_TILE * CW_P];     // x[i][t0 + tt + tap - K/2], n = i K + tap
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;             // a wave: 64 x 64 of the 128 x 128 tile, 2 x 2 MFMA tiles
    const int o0 = blockIdx.x * CW_TILE, n0 = blockIdx.y * CW_TILE, sp = blockIdx.z;
    const bool first_col = blockIdx.y == 0;
    const long long U = (long long)p.B * p.NTt;
    const long long u0 = U * sp / p.nsplit, u1 = U * (sp + 1) / p.nsplit;
    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;
    float dbacc = 0.f;
    CwChunk r;
    if (u0 < u1) cw_load(p, r, (int)(u0 / p.NTt), CW_CHUNK * (int)(u0 % p.NTt), o0, n0, tid);
    for (long long u = u0; u < u1; ++u) {
        const int b = (int)(u / p.NTt), t0 = CW_CHUNK * (int)(u % p.NTt);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CW_PER; ++j) {
            const int idx = tid + 256 * j, rl = idx >> 5, tt = idx & 31;
            const float v = (p.relu && r.m[j] <= 0.f) ? 0.f : r.a[j];
            As[rl * CW_P + tt] = v;
            Bs[rl * CW_P + tt] = r.bx[j];
            const int o = o0 + rl, t = t0 + tt;
            if (first_col && p.gyp && o < p.Cout && t < p.T) p.gyp[((size_t)b * p.Cout + o) * p.T + t] = v;
        }
        __syncthreads();
        if (u + 1 < u1) cw_load(p, r, (int)((u + 1) / p.NTt), CW_CHUNK * (int)((u + 1) % p.NTt), o0, n0, tid);   // in flight below
        if (first_col && tid < CW_TILE) {
#pragma unroll 8
            for (int tt = 0; tt < CW_CHUNK; ++tt) dbacc += As[tid * CW_P + tt];
        }
        const float *A = As + (64 * wm + (lane & 31)) * CW_P + half;
        const float *Bv = Bs + (64 * wn + (lane & 31)) * CW_P + half;
#pragma unroll
        for (int s = 0; s < CW_CHUNK / 2; ++s) {
            const float a0 = A[2 * s], a1 = A[32 * CW_P + 2 * s], b0 = Bv[2 * s], b1 = Bv[32 * CW_P + 2 * s];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int n = n0 + 64 * wn + 32 * ni + (lane & 31);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int o = o0 + 64 * wm + 32 * mi + (e & 3) + 8 * (e >> 2) + 4 * half;
                if (o < p.Cout && n < p.N) p.part[((size_t)sp * p.Cout + o) * p.N + n] = acc[mi][ni][e];
            }
        }
    if (first_col && p.dbpart && tid < CW_TILE && o0 + tid < p.Cout) p.dbpart[(size_t)sp * p.Cout + o0 + tid] = dbacc;
}

// dW = sum of the partials in split order; db likewise (elements >= Cout N)
__global__ __launch_bounds__(256) void conv_bwd_reduce_kernel(const float *__restrict__ part, const float *__restrict__ dbpart,
                                                              float *__restrict__ dw, float *__restrict__ db, int nsplit,
                                                              size_t nw, int Cout) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < nw) {
        if (!dw) return;
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) v += part[(size_t)s * nw + idx];
        dw[idx] = v;
    } else if (idx < nw + (size_t)Cout) {
        if (!db) return;
        const size_t o = idx - nw;
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) v += dbpart[(size_t)s * Cout + o];
        db[o] = v;
    }
}

// dYpre alone (the input gradient without the weight gradient)
__global__ __launch_bounds__(256) void conv_bwd_mask_kernel(ConvBwdParams p, size_t n) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n) p.gyp[idx] = cw_gy(p, idx);
}

static int cw_nsplit(int B, int Cin, int Cout, int T, int K) {
    const long long tiles = (long long)((Cout + CW_TILE - 1) / CW_TILE) * ((Cin * K + CW_TILE - 1) / CW_TILE);
    const long long units = (long long)B * ((T + CW_CHUNK - 1) / CW_CHUNK);
    long long ns = (512 + tiles - 1) / tiles;            // about two workgroups a CU in all
    if (ns > 32) ns = 32;
    if (ns > units) ns = units;
    return ns < 1 ? 1 : (int)ns;
}

}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_conv1d_backward_workspace_bytes(int B, int Cin, int Cout, int T, int K) {
    if (B < 1 || Cin < 1 || Cout < 1 || T < 1 || (K != 1 && K != 3 && K != 5)) return 0;
    const size_t ns = cw_nsplit(B, Cin, Cout, T, K);
    return align_up(ns * Cout * (size_t)Cin * K * sizeof(float), 256) + align_up(ns * Cout * sizeof(float), 256);
}

int aligner_conv1d_backward_weight_f32(const float *x, const float *y, const float *grad_y, float *grad_ypre_out,
                                       float *grad_w_out, float *grad_b_out, void *workspace, size_t workspace_bytes,
                                       int B, int Cin, int Cout, int T, int K, int relu, void *stream) {
    if (!grad_w_out && !grad_b_out && !grad_ypre_out) return fail(ALIGNER_EINVAL, "null pointer: no output requested");
    if (!x || !grad_y) return fail(ALIGNER_EINVAL, "null pointer");
    if (relu && !y) return fail(ALIGNER_EINVAL, "null pointer: relu needs the layer's output y");
    if (relu != 0 && relu != 1) return fail(ALIGNER_EINVAL, "relu must be 0 or 1");
    if (B < 0 || Cin < 1 || Cout < 1 || T < 1) return fail(ALIGNER_EINVAL, "bad shape B=%d Cin=%d Cout=%d T=%d", B, Cin, Cout, T);
    if (K != 1 && K != 3 && K != 5) return fail(ALIGNER_EDOM, "kernel size %d not supported (1, 3, 5)", K);
    if ((long long)Cin * K >= (1ll << 30) || (long long)Cin * T >= (1ll << 31) || (long long)Cout * T >= (1ll << 31) || (Cout + CW_TILE - 1) / CW_TILE > 65535 || (Cin * K + CW_TILE - 1) / CW_TILE > 65535)
        return fail(ALIGNER_EDOM, "layer too large");
    const bool need_w = grad_w_out || grad_b_out;
    if (B == 0) return ALIGNER_OK;
    const size_t need = aligner_conv1d_backward_workspace_bytes(B, Cin, Cout, T, K);
    if (need_w && !workspace) return fail(ALIGNER_EINVAL, "null pointer: workspace");
    if (need_w && workspace_bytes < need) return fail(ALIGNER_ENOSPC, "workspace %zu < %zu bytes", workspace_bytes, need);
    ConvBwdParams p{};
    p.x = x;
    p.y = y;
    p.gy = grad_y;
    p.gyp = grad_ypre_out;
    p.B = B;
    p.Cin = Cin;
    p.Cout = Cout;
    p.T = T;
    p.K = K;
    p.relu = relu;
    p.N = Cin * K;
    p.NTt = (T + CW_CHUNK - 1) / CW_CHUNK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!need_w) {
        const size_t n = (size_t)B * Cout * T;
        hipLaunchKernelGGL(conv_bwd_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n);
        ALIGNER_HIP_CHECK(hipGetLastError());
        return ALIGNER_OK;
    }
    p.nsplit = cw_nsplit(B, Cin, Cout, T, K);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const size_t nw = (size_t)Cout * p.N;
    p.part = reinterpret_cast<float *>(ws);
    p.dbpart = reinterpret_cast<float *>(ws + align_up(p.nsplit * nw * sizeof(float), 256));
    dim3 grid((unsigned)((Cout + CW_TILE - 1) / CW_TILE), (unsigned)((p.N + CW_TILE - 1) / CW_TILE), (unsigned)p.nsplit);
    hipLaunchKernelGGL(conv_bwd_w_kernel, grid, dim3(256), 0, s, p);
    ALIGNER_HIP_CHECK(hipGetLastError());
    const size_t tot = nw + Cout;
    hipLaunchKernelGGL(conv_bwd_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p.part, p.dbpart,
                       grad_w_out, grad_b_out, p.nsplit, nw, Cout);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

}  // extern "C"
