// The cost kinds of costkind.h on the pairs of a warping path instead of on a table, forward and backward (DESIGN.md
// 5.14; include/aligner_amd.h has the definitions).  A path is a pair list [B,L,2] with a length per utterance, as
// dtw_path() / dtw_path_banded() report it; nothing here knows whether it came from a dense or a banded table, or
// whether it is optimal.
//
//     runs       one workgroup per utterance: pass 1 tests length, bounds and steps and reduces `valid`; pass 2 writes the
//                index of the first pair of every row and of every column (the pair whose predecessor has another row /
//                column writes it), -1 / 0 outside the rows and columns the path covers; after a barrier a row's count
//                is the next row's start (the length for the last row) minus its own.  A valid path covers a contiguous
//                range of rows and of columns, so every element has one writer.  Nothing is stored through an index
//                before pass 1 has found every pair inside [0,N) x [0,M).
//     pair cost  a lane per pair: Kind::term over the channels in order from 0, then Kind::finish -- the cell's
//                arithmetic of lc_cost_kernel / bc_cost_kernel, so the table's bits.  Consecutive pairs differ by at most
//                1 in i and in j: a wave's loads of one channel fall into one to three 128-byte lines of each operand.
//                The same body writes the root kind's backward coefficient w_k / dist_k instead (0 at dist_k == 0).
//     total      one workgroup per utterance adds the pair costs in a fixed order (strided partial sums, then a tree in
//                LDS): no atomics, the same bits on every call.
//     gradient   a lane owns a row i (dpred) or a column j (dtarget) and PC_CC channels, and walks its run: the pairs of
//                row i are (i, j0 .. j0 + count - 1) at k = start .. start + count - 1.  The run is accumulated first and
//                multiplied by the kind's factor once.  One owner per output element.
//
// The root kind's gradient is the squared kind's arithmetic with the coefficient in place of the weight and the L1
// factor: d / dist is at most 1 in magnitude, and dist, the root of an fp32 sum, is 0 or at least 2^-74.5, so
// w / dist is finite for |w| < 2^53 and 1 / dist is never formed unguarded.
#include "common.h"
#include "device.h"
#include "costkind.h"

namespace aligner {

constexpr int PC_CC = 8;                    // channels per lane (gradient)
constexpr int PC_MAX_C = 4096;
constexpr int PC_MAX_L = 1 << 24;

// The gradient pieces of the root kind along a path: fma(coefficient, pred - target, acc), finished by scale g.
struct PathRootGrad {
    static __device__ __forceinline__ float back(float p, float t, float g, float acc) { return CostL2::back(p, t, g, acc); }
    static __device__ __forceinline__ float factor(float scale, float g) { return CostL1::factor(scale, g); }
};

__device__ __forceinline__ int pc_clamp_length(const int *__restrict__ length, int b, int L) {
    const int v = length[b];
    return v < 0 ? 0 : (v > L ? L : v);
}

__global__ __launch_bounds__(256) void pc_runs_kernel(
        const int *__restrict__ path, const int *__restrict__ length, int *row_start, int *row_count, int *col_start,
        int *col_count, int *__restrict__ valid, int L, int N, int M) {
    __shared__ int any_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int *p = path + (size_t)b * L * 2;
    int *rs = row_start + (size_t)b * N, *rc = row_count + (size_t)b * N;
    int *cs = col_start + (size_t)b * M, *cc = col_count + (size_t)b * M;
    const int len = length[b];
    if (tid == 0) any_bad = 0;
    __syncthreads();
    bool bad = len < 0 || len > L;
    if (!bad) {
        for (int k = tid; k < len; k += 256) {
            const unsigned i = (unsigned)p[2 * k], j = (unsigned)p[2 * k + 1];
            bad |= i >= (unsigned)N || j >= (unsigned)M;
            if (k > 0) {                                                   // (unsigned: a difference of anything wraps)
                const unsigned di = i - (unsigned)p[2 * k - 2], dj = j - (unsigned)p[2 * k - 1];
                bad |= !((di == 1u && dj <= 1u) || (di == 0u && dj == 1u));
            }
        }
    }
    if (bad) any_bad = 1;
    __syncthreads();
    const bool ok = any_bad == 0;
    if (tid == 0) valid[b] = ok ? 1 : 0;
    // the rows and columns the path covers: [ifirst, ilast], [jfirst, jlast]; none without pairs
    int ifirst = 0, ilast = -1, jfirst = 0, jlast = -1;
    if (ok && len > 0) {
        ifirst = p[0], jfirst = p[1];
        ilast = p[2 * (len - 1)], jlast = p[2 * (len - 1) + 1];
    }
    for (int i = tid; i < N; i += 256)
        if (i < ifirst || i > ilast) rs[i] = -1, rc[i] = 0;
    for (int j = tid; j < M; j += 256)
        if (j < jfirst || j > jlast) cs[j] = -1, cc[j] = 0;
    if (!(ok && len > 0)) return;                                         // (uniform)
    for (int k = tid; k < len; k += 256) {
        const int i = p[2 * k], j = p[2 * k + 1];
        const int pi = k > 0 ? p[2 * k - 2] : -1, pj = k > 0 ? p[2 * k - 1] : -1;
        if (i != pi) rs[i] = k;
        if (j != pj) cs[j] = k;
    }
    __syncthreads();                                                      // (the starts are read back below)
    for (int i = ifirst + tid; i <= ilast; i += 256) rc[i] = (i < ilast ? rs[i + 1] : len) - rs[i];
    for (int j = jfirst + tid; j <= jlast; j += 256) cc[j] = (j < jlast ? cs[j + 1] : len) - cs[j];
}

// COEF: out[b,k] = w_k / sqrt(sum) (0 where the sum is 0, the pair is outside the lengths or k is past the length)
// instead of the cost; `weight` may be null (all 1) and is not read at k >= length[b].
template <class Kind, bool COEF>
__global__ __launch_bounds__(256) void pc_pair_kernel(
        const float *__restrict__ pred, const float *__restrict__ target, const int *__restrict__ path,
        const int *__restrict__ length, const int *__restrict__ ns, const int *__restrict__ ms, float scale,
        const float *__restrict__ weight, float *__restrict__ out, int C, int N, int M, int L) {
    const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= L) return;
    const int len = pc_clamp_length(length, b, L);
    const size_t at = (size_t)b * L + k;
    if (k >= len) {
        out[at] = 0.f;
        return;
    }
    const int n = clamp_len(ns, b, N), m = clamp_len(ms, b, M);
    const int i = path[at * 2], j = path[at * 2 + 1];
    if ((unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)m) {       // nothing is read for it
        out[at] = COEF ? 0.f : __builtin_huge_valf();
        return;
    }
    const float *p = pred + (size_t)b * C * N + i, *t = target + (size_t)b * C * M + j;
    float acc = 0.f;
#pragma unroll 4
    for (int c = 0; c < C; ++c) acc = Kind::term(t[(size_t)c * M], p[(size_t)c * N], acc);
    if constexpr (COEF) {
        const float dist = __builtin_sqrtf(acc), w = weight ? weight[at] : 1.f;
        out[at] = dist > 0.f ? w / dist : 0.f;
    } else {
        out[at] = Kind::finish(acc, scale);
    }
}

__global__ __launch_bounds__(256) void pc_total_kernel(const float *__restrict__ pair_cost, const int *__restrict__ length,
                                                       float *__restrict__ total, int L) {
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = pc_clamp_length(length, b, L);
    const float *pc = pair_cost + (size_t)b * L;
    float sum = 0.f;
    for (int k = tid; k < len; k += 256) sum = sum + pc[k];
    red[tid] = sum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    if (tid == 0) total[b] = len > 0 ? red[0] : __builtin_huge_valf();
}

// ROWS: out = dpred [B,C,N], a lane owns row x, `own` is pred and `other` target; else out = dtarget [B,C,M], a lane owns
// column x.  wk [B,L]: the pairs' weights (null: 1), or the root kind's coefficients.
template <class Kind, bool ROWS>
__global__ __launch_bounds__(64) void pc_run_kernel(
        const float *__restrict__ wk, const float *__restrict__ pred, const float *__restrict__ target,
        const int *__restrict__ path, const int *__restrict__ ns, const int *__restrict__ ms,
        const int *__restrict__ start, const int *__restrict__ count, float scale, const float *__restrict__ row_scale,
        float *__restrict__ out, int C, int N, int M, int L) {
    const int b = blockIdx.z, x = blockIdx.x * 64 + threadIdx.x, c0 = blockIdx.y * PC_CC;
    const int T = ROWS ? N : M, To = ROWS ? M : N;                        // the owner's extent and the other operand's
    if (x >= T) return;
    const int cmax = (c0 + PC_CC < C ? c0 + PC_CC : C) - 1 - c0;          // channels past C repeat the last one (never stored)
    const int n = clamp_len(ns, b, N), m = clamp_len(ms, b, M);
    const int own_len = ROWS ? n : m, other_len = ROWS ? m : n;
    const float *own = (ROWS ? pred : target) + ((size_t)b * C + c0) * T + x;
    const float *other = (ROWS ? target : pred) + ((size_t)b * C + c0) * To;
    const int s = start[(size_t)b * T + x];
    const int cnt = x < own_len ? count[(size_t)b * T + x] : 0;
    float acc[PC_CC];
#pragma unroll
    for (int cc = 0; cc < PC_CC; ++cc) acc[cc] = 0.f;
    int used = 0;                                                         // pairs inside the lengths
    if (cnt > 0) {
        float ov[PC_CC];
#pragma unroll
        for (int cc = 0; cc < PC_CC; ++cc) ov[cc] = own[(size_t)(cc < cmax ? cc : cmax) * T];
        const int y0 = path[((size_t)b * L + s) * 2 + (ROWS ? 1 : 0)];
        const float *w = wk ? wk + (size_t)b * L + s : nullptr;
        for (int r = 0; r < cnt; ++r) {
            const int y = y0 + r;                                         // the run's pairs are (x, y0 + r) at k = s + r
            if ((unsigned)y >= (unsigned)other_len) continue;
            const float wv = w ? w[r] : 1.f;
#pragma unroll
            for (int cc = 0; cc < PC_CC; ++cc) {
                const float v = other[(size_t)(cc < cmax ? cc : cmax) * To + y];
                acc[cc] = ROWS ? Kind::back(ov[cc], v, wv, acc[cc]) : Kind::back(v, ov[cc], wv, acc[cc]);
            }
            ++used;
        }
    }
    const float f = Kind::factor(scale, row_scale ? row_scale[b] : 1.f);
    const float k = ROWS ? f : -f;
    float *o = out + ((size_t)b * C + c0) * T + x;
#pragma unroll
    for (int cc = 0; cc < PC_CC; ++cc)
        if (cc <= cmax) o[(size_t)cc * T] = used > 0 ? acc[cc] * k : 0.f;
}

static bool pc_kind_ok(int kind) { return kind == ALIGNER_COST_L1 || kind == ALIGNER_COST_L2 || kind == ALIGNER_COST_L2_ROOT; }

static int pc_check(int kind, int B, int C, int N, int M, int L, float scale) {
    if (B < 1 || C < 1 || N < 1 || M < 1 || L < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (!pc_kind_ok(kind)) return fail(ALIGNER_EINVAL, "kind must be ALIGNER_COST_L1, _L2 or _L2_ROOT");
    if (!(scale == scale) || !(scale < __builtin_huge_valf()) || !(scale > -__builtin_huge_valf()))
        return fail(ALIGNER_EINVAL, "scale must be finite");
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if (C > PC_MAX_C) return fail(ALIGNER_EDOM, "C=%d too large (<= %d)", C, PC_MAX_C);
    if (L >= PC_MAX_L) return fail(ALIGNER_EDOM, "L=%d too large (< 2^24)", L);
    return ALIGNER_OK;
}

// the backward call's workspace: row_start, row_count [B,N] | col_start, col_count [B,M] | valid [B] | coefficients [B,L]
// (the coefficients for the root kind only)
static size_t pc_workspace_bytes(int kind, int B, int N, int M, int L) {
    return 4 * (2 * (size_t)B * N + 2 * (size_t)B * M + B + (kind == ALIGNER_COST_L2_ROOT ? (size_t)B * L : 0));
}

struct PcWorkspace {
    int32_t *row_start, *row_count, *col_start, *col_count, *valid;
    float *coef;
    PcWorkspace(void *ws, int B, int N, int M) {
        int32_t *w = static_cast<int32_t *>(ws);
        const size_t bn = (size_t)B * N, bm = (size_t)B * M;
        row_start = w, row_count = w + bn, col_start = w + 2 * bn, col_count = w + 2 * bn + bm, valid = w + 2 * bn + 2 * bm;
        coef = reinterpret_cast<float *>(w + 2 * bn + 2 * bm + B);
    }
};

template <class Kind>
static int pc_forward(const float *pred, const float *target, const int32_t *path, const int32_t *length, const int32_t *n_dev,
                      const int32_t *m_dev, float scale, float *pair_cost, int B, int C, int N, int M, int L, hipStream_t s) {
    hipLaunchKernelGGL((pc_pair_kernel<Kind, false>), dim3((L + 255) / 256, B), dim3(256), 0, s, pred, target, path, length,
                       n_dev, m_dev, scale, (const float *)nullptr, pair_cost, C, N, M, L);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

template <class Kind>
static int pc_backward(const float *wk, const float *pred, const float *target, const int32_t *path, const int32_t *n_dev,
                       const int32_t *m_dev, const PcWorkspace &w, float scale, const float *row_scale, float *dpred,
                       float *dtarget, int B, int C, int N, int M, int L, hipStream_t s) {
    const int nchunks = (C + PC_CC - 1) / PC_CC;
    if (dpred) {
        hipLaunchKernelGGL((pc_run_kernel<Kind, true>), dim3((N + 63) / 64, nchunks, B), dim3(64), 0, s, wk, pred, target, path,
                           n_dev, m_dev, w.row_start, w.row_count, scale, row_scale, dpred, C, N, M, L);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    if (dtarget) {
        hipLaunchKernelGGL((pc_run_kernel<Kind, false>), dim3((M + 63) / 64, nchunks, B), dim3(64), 0, s, wk, pred, target, path,
                           n_dev, m_dev, w.col_start, w.col_count, scale, row_scale, dtarget, C, N, M, L);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

}  // namespace aligner

using namespace aligner;

extern "C" {

int aligner_path_runs(const int32_t *path, const int32_t *length, int32_t *row_start, int32_t *row_count, int32_t *col_start,
                      int32_t *col_count, int32_t *valid, int B, int L, int N, int M, void *stream) {
    if (!path || !length || !row_start || !row_count || !col_start || !col_count || !valid)
        return fail(ALIGNER_EINVAL, "null pointer");
    if (B < 1 || L < 1 || N < 1 || M < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if (L >= PC_MAX_L) return fail(ALIGNER_EDOM, "L=%d too large (< 2^24)", L);
    hipLaunchKernelGGL(pc_runs_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), path, length, row_start,
                       row_count, col_start, col_count, valid, L, N, M);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

int aligner_path_cost_f32(const float *pred, const float *target, const int32_t *path, const int32_t *length,
                          const int32_t *n_dev, const int32_t *m_dev, int kind, float scale, float *pair_cost, float *total,
                          int B, int C, int N, int M, int L, void *stream) {
    if (!pred || !target || !path || !length || !pair_cost) return fail(ALIGNER_EINVAL, "null pointer");
    if (const int rc = pc_check(kind, B, C, N, M, L, scale)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    if (kind == ALIGNER_COST_L1) rc = pc_forward<CostL1>(pred, target, path, length, n_dev, m_dev, scale, pair_cost, B, C, N, M, L, s);
    else if (kind == ALIGNER_COST_L2) rc = pc_forward<CostL2>(pred, target, path, length, n_dev, m_dev, scale, pair_cost, B, C, N, M, L, s);
    else rc = pc_forward<CostL2Root>(pred, target, path, length, n_dev, m_dev, scale, pair_cost, B, C, N, M, L, s);
    if (rc) return rc;
    if (total) {
        hipLaunchKernelGGL(pc_total_kernel, dim3(B), dim3(256), 0, s, pair_cost, length, total, L);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

size_t aligner_path_cost_backward_workspace_bytes(int kind, int B, int N, int M, int L) {
    if (!pc_kind_ok(kind) || B < 1 || N < 1 || M < 1 || L < 1 || B > 65535 || L >= PC_MAX_L) return 0;
    return pc_workspace_bytes(kind, B, N, M, L);
}

int aligner_path_cost_backward_f32(const float *pair_weight, const float *pred, const float *target, const int32_t *path,
                                   const int32_t *length, const int32_t *n_dev, const int32_t *m_dev, int kind, float scale,
                                   const float *row_scale, float *dpred, float *dtarget, void *ws, size_t ws_bytes,
                                   int B, int C, int N, int M, int L, void *stream) {
    if (!pred || !target || !path || !length || !ws) return fail(ALIGNER_EINVAL, "null pointer");
    if (!dpred && !dtarget) return fail(ALIGNER_EINVAL, "null pointer: no output");
    if (const int rc = pc_check(kind, B, C, N, M, L, scale)) return rc;
    const size_t need = pc_workspace_bytes(kind, B, N, M, L);
    if (ws_bytes < need) return fail(ALIGNER_ENOSPC, "workspace too small: %zu < %zu bytes", ws_bytes, need);
    const PcWorkspace w(ws, B, N, M);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pc_runs_kernel, dim3(B), dim3(256), 0, s, path, length, w.row_start, w.row_count, w.col_start,
                       w.col_count, w.valid, L, N, M);
    ALIGNER_HIP_CHECK(hipGetLastError());
    if (kind == ALIGNER_COST_L1)
        return pc_backward<CostL1>(pair_weight, pred, target, path, n_dev, m_dev, w, scale, row_scale, dpred, dtarget, B, C, N, M, L, s);
    if (kind == ALIGNER_COST_L2)
        return pc_backward<CostL2>(pair_weight, pred, target, path, n_dev, m_dev, w, scale, row_scale, dpred, dtarget, B, C, N, M, L, s);
    hipLaunchKernelGGL((pc_pair_kernel<CostL2, true>), dim3((L + 255) / 256, B), dim3(256), 0, s, pred, target, path, length,
                       n_dev, m_dev, 1.f, pair_weight, w.coef, C, N, M, L);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return pc_backward<PathRootGrad>(w.coef, pred, target, path, n_dev, m_dev, w, scale, row_scale, dpred, dtarget, B, C, N, M, L, s);
}

}  // extern "C"
