// The L1 cost table of Soft-DTW and its gradient (include/aligner_amd.h has the definition):
//
//     cost[b,i,j] = scale sum_c |pred[b,c,i] - target[b,c,j]|        on the cells soft_dtw() calls existing
//
// +inf outside the band, 0 at and past the lengths.  Channels come first, so a lane owns a column j (target[b,c,j..]
// loads coalesced) and a wave keeps a block of rows of pred[b,c,.] as wave-uniform values: one target load feeds
// LC_RB cells, and each cell is one subtraction and one add of the magnitude, summed over c in order.  Work is done
// where cells exist: a wave whose 16 x 64 tile has none only stores the fill.
//
// Backward, with G = grad_cost and s = sign(pred - target) (sign(0) = 0), one kernel per output and one owner per
// output element, so no atomics and the same bits on every call:
//     dtarget[b,c,j] = -k sum_i G[i,j] s      a wave owns 64 columns x LC_CC channels and walks the rows of the band
//     dpred[b,c,i]   =  k sum_j G[i,j] s      a wave owns LC_PR rows x LC_CC channels, every lane sums its own columns
//                                             of the band and the 64 lanes' sums meet in LDS, added in lane order
// k = scale g[b] is rounded once and multiplies the finished sum.  G is selected, never multiplied, by "the cell
// exists", so whatever stands in G outside the cells reaches nothing.
//
// The kernels are written once over the cost kind (costkind.h): the same tiles, loads and order of summation give the
// squared Euclidean cost sum_c (pred - target)^2 with its gradient 2 k sum G (pred - target), and the root of that
// sum, which is forward only.
#include "common.h"
#include "device.h"
#include "costkind.h"

namespace aligner {

constexpr int LC_RB = 16;                   // rows per wave tile (forward)
constexpr int LC_TR = 8;                    // rows per step of a wave (dtarget): LC_TR * LC_CC pred values fit the scalar registers
constexpr int LC_PF = 4;                    // channels per pass of the forward loop, loaded a pass ahead
constexpr int LC_WAVES = 4;                // waves per workgroup (forward: row blocks; dtarget: channel chunks)
constexpr int LC_CC = 8;                    // channels per wave (backward)
constexpr int LC_PR = 8;                    // rows per wave (dpred): LC_PR * LC_CC == 64 sums, one per lane at the end
constexpr int LC_PITCH = 65;                // odd: the 64 lanes of the reduction read 64 banks
constexpr int LC_MAX_C = 4096;
constexpr int LC_NO_BAND = 1 << 30;

__device__ __forceinline__ float lc_lane(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

template <class Kind>
__global__ __launch_bounds__(64 * LC_WAVES) void lc_cost_kernel(
        const float *__restrict__ pred, const float *__restrict__ target, const int *__restrict__ ns,
        const int *__restrict__ ms, int band, float scale, float *__restrict__ cost, int C, int N, int M, int nct) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // Workgroups are dealt round-robin over the 8 XCDs (observed, speed only; device.h).  Neighbouring column tiles
    // share the 128-byte lines at their common edge (a row starts wherever i M falls), and lines written half by one
    // XCD and half by another cannot be merged in either L2.  With B a multiple of 8 the workgroups of 8 utterances
    // are therefore re-dealt, one utterance per XCD: 8 z-planes of gridDim.x workgroups, linear number l8 within them
    // (the planes before them hold a multiple of 8 workgroups, so the XCD is l8 & 7).  Any B: a bijection.
    int b = blockIdx.z, inner = blockIdx.x;
    if ((gridDim.z & 7) == 0) {
        const unsigned l8 = (b & 7) * gridDim.x + inner;
        b = (b & ~7) | (l8 & 7);
        inner = l8 >> 3;
    }
    const int ct = inner % nct, rb = inner / nct;
    const int i0 = (rb * LC_WAVES + w) * LC_RB, j0 = ct * 64, j = j0 + lane;
    if (i0 >= N) return;
    const int n = clamp_len(ns, b, N), m = clamp_len(ms, b, M);
    const int ilast = (i0 + LC_RB < n ? i0 + LC_RB : n) - 1;              // the tile's last row inside the utterance
    const bool some = i0 < n && j0 < m && j0 <= ilast + band && j0 + 63 >= i0 - band;
    float acc[LC_RB];
#pragma unroll
    for (int r = 0; r < LC_RB; ++r) acc[r] = 0.f;
    if (some) {
        const float *t = target + (size_t)b * C * M + (j < M ? j : M - 1);
        const float *p = pred + (size_t)b * C * N + i0;
        if (i0 + LC_RB <= N) {
            // LC_PF channels a pass, the target values of the next pass loaded while this one computes (a wave has
            // 32 instructions per channel to hide a load behind; channels past C repeat the last one and are not added)
            float tn[LC_PF];
#pragma unroll
            for (int k = 0; k < LC_PF; ++k) tn[k] = t[(size_t)(k < C ? k : C - 1) * M];
            for (int c = 0; c < C; c += LC_PF) {
                float tc[LC_PF];
#pragma unroll
                for (int k = 0; k < LC_PF; ++k) {
                    tc[k] = tn[k];
                    const int cn = c + LC_PF + k;
                    tn[k] = t[(size_t)(cn < C ? cn : C - 1) * M];
                }
#pragma unroll
                for (int k = 0; k < LC_PF; ++k) {
                    if (c + k >= C) break;
                    const float *pk = p + (size_t)(c + k) * N;
#pragma unroll
                    for (int r = 0; r < LC_RB; ++r) acc[r] = Kind::term(tc[k], pk[r], acc[r]);
                }
            }
        } else {                                                          // the last row block: rows past N repeat row N - 1
            const int rl = lane < N - 1 - i0 ? lane : N - 1 - i0;
            for (int c = 0; c < C; ++c, t += M, p += N) {
                const float tv = *t, pl = p[rl];
#pragma unroll
                for (int r = 0; r < LC_RB; ++r) acc[r] = Kind::term(tv, lc_lane(pl, r), acc[r]);
            }
        }
    }
    if (j >= M) return;
    float *out = cost + ((size_t)b * N + i0) * M + j;
#pragma unroll
    for (int r = 0; r < LC_RB; ++r) {
        const int i = i0 + r;
        if (i >= N) break;
        const int dist = i > j ? i - j : j - i;
        float v = dist <= band ? Kind::finish(acc[r], scale) : __builtin_huge_valf();
        v = (i < n && j < m) ? v : 0.f;
        out[(size_t)r * M] = v;
    }
}

template <class Kind>
__global__ __launch_bounds__(64 * LC_WAVES) void lc_dtarget_kernel(
        const float *__restrict__ G, const float *__restrict__ pred, const float *__restrict__ target,
        const int *__restrict__ ns, const int *__restrict__ ms, int band, float scale, const float *__restrict__ row_scale,
        float *__restrict__ dtarget, int C, int N, int M) {
    const int b = blockIdx.z, lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c0 = (blockIdx.y * LC_WAVES + w) * LC_CC, j0 = blockIdx.x * 64, j = j0 + lane;
    if (c0 >= C) return;
    const int n = clamp_len(ns, b, N), m = clamp_len(ms, b, M);
    const int cmax = (c0 + LC_CC < C ? c0 + LC_CC : C) - 1 - c0;          // channels past C repeat the last one (never stored)
    float acc[LC_CC];
#pragma unroll
    for (int cc = 0; cc < LC_CC; ++cc) acc[cc] = 0.f;
    // the rows with a cell in these 64 columns: [ilo, ihi)
    const int jlast = (j0 + 64 < m ? j0 + 64 : m) - 1;
    const int ilo = j0 - band > 0 ? j0 - band : 0;
    const int ihi = jlast + band + 1 < n ? jlast + band + 1 : n;
    if (j0 < m && ilo < ihi) {
        const float *t = target + ((size_t)b * C + c0) * M + (j < M ? j : M - 1);
        const float *p = pred + ((size_t)b * C + c0) * N;
        const float *g = G + (size_t)b * N * M + (j < M ? j : M - 1);
        float tv[LC_CC];
#pragma unroll
        for (int cc = 0; cc < LC_CC; ++cc) tv[cc] = t[(size_t)(cc < cmax ? cc : cmax) * M];
        // G of rows ib .. ib + LC_TR - 1, loaded from a row inside the tensor and then masked; a step ahead of its use
        auto load_g = [&](int ib, float (&out)[LC_TR]) {
#pragma unroll
            for (int r = 0; r < LC_TR; ++r) {
                const int i = ib + r;
                const int dist = i > j ? i - j : j - i;
                out[r] = and_mask(g[(size_t)(i < N ? i : N - 1) * M], (i < ihi && j < m && dist <= band) ? ~0u : 0u);
            }
        };
        float gn[LC_TR];
        load_g(ilo, gn);
        for (int ib = ilo; ib < ihi; ib += LC_TR) {
            float gv[LC_TR];
#pragma unroll
            for (int r = 0; r < LC_TR; ++r) gv[r] = gn[r];
            load_g(ib + LC_TR, gn);
            if (ib + LC_TR <= ihi && cmax == LC_CC - 1) {                  // (all LC_TR rows inside the utterance)
#pragma unroll
                for (int cc = 0; cc < LC_CC; ++cc)
#pragma unroll
                    for (int r = 0; r < LC_TR; ++r)
                        acc[cc] = Kind::back(p[(size_t)cc * N + ib + r], tv[cc], gv[r], acc[cc]);
            } else {                                                      // the last rows or channels: repeat the last one
                const int rl = ib + lane < ihi ? ib + lane : ihi - 1;     // (a row of the utterance: costkind.h)
#pragma unroll
                for (int cc = 0; cc < LC_CC; ++cc) {
                    const float pl = p[(size_t)(cc < cmax ? cc : cmax) * N + rl];
#pragma unroll
                    for (int r = 0; r < LC_TR; ++r) acc[cc] = Kind::back(lc_lane(pl, r), tv[cc], gv[r], acc[cc]);
                }
            }
        }
    }
    if (j >= M) return;
    const float k = -Kind::factor(scale, row_scale ? row_scale[b] : 1.f);
    float *out = dtarget + ((size_t)b * C + c0) * M + j;
#pragma unroll
    for (int cc = 0; cc < LC_CC; ++cc)
        if (cc <= cmax) out[(size_t)cc * M] = j < m && n > 0 ? acc[cc] * k : 0.f;
}

// (three waves a SIMD, 168 VGPRs: left to itself the compiler takes 229 for the loads a step ahead, and two waves)
template <class Kind>
__global__ __launch_bounds__(64, 3) void lc_dpred_kernel(
        const float *__restrict__ G, const float *__restrict__ pred, const float *__restrict__ target,
        const int *__restrict__ ns, const int *__restrict__ ms, int band, float scale, const float *__restrict__ row_scale,
        float *__restrict__ dpred, int C, int N, int M) {
    __shared__ float red[64 * LC_PITCH];
    const int b = blockIdx.z, lane = threadIdx.x;
    const int i0 = blockIdx.x * LC_PR, c0 = blockIdx.y * LC_CC;
    const int n = clamp_len(ns, b, N), m = clamp_len(ms, b, M);
    const int cmax = (c0 + LC_CC < C ? c0 + LC_CC : C) - 1 - c0;
    // this lane's output at the end: channel c0 + lane / LC_PR, row i0 + lane % LC_PR
    const int oc = lane / LC_PR, oi = i0 + lane % LC_PR;
    float *out = dpred + ((size_t)b * C + c0 + oc) * N + oi;
    const bool stored = oc <= cmax && oi < N;
    // the columns with a cell in these rows: [jlo, jhi)
    const int ilast = (i0 + LC_PR < n ? i0 + LC_PR : n) - 1;
    const int jlo = i0 - band > 0 ? i0 - band : 0;
    const int jhi = ilast + band + 1 < m ? ilast + band + 1 : m;
    if (i0 >= n || jlo >= jhi) {                                          // (wave-uniform)
        if (stored) *out = 0.f;
        return;
    }
    // The wave's 64 pred values, read once.  They are wave-uniform, and 64 of them are more than the scalar registers
    // hold: the zero the compiler cannot see keeps them in vector registers, one copy per lane.
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    float pv[LC_CC][LC_PR];
#pragma unroll
    for (int cc = 0; cc < LC_CC; ++cc)
#pragma unroll
        for (int r = 0; r < LC_PR; ++r)
            pv[cc][r] = pred[((size_t)b * C + c0 + (cc < cmax ? cc : cmax)) * N + (i0 + r < N ? i0 + r : N - 1) + vzero];
    float acc[LC_CC][LC_PR];
#pragma unroll
    for (int cc = 0; cc < LC_CC; ++cc)
#pragma unroll
        for (int r = 0; r < LC_PR; ++r) acc[cc][r] = 0.f;
    const float *tb = target + ((size_t)b * C + c0) * M;
    const float *gb = G + ((size_t)b * N + i0) * M;
    // target and G of columns jt .. jt + 63 (G from a cell inside the tensor, then masked), a step ahead of their use
    auto load_tile = [&](int jt, float (&tout)[LC_CC], float (&gout)[LC_PR]) {
        const int j = jt + lane;
        const int jc = j < jhi ? j : jhi - 1;                             // (a column of the utterance: costkind.h)
#pragma unroll
        for (int cc = 0; cc < LC_CC; ++cc) tout[cc] = tb[(size_t)(cc < cmax ? cc : cmax) * M + jc];
#pragma unroll
        for (int r = 0; r < LC_PR; ++r) {
            const int i = i0 + r;
            const int dist = i > j ? i - j : j - i;
            gout[r] = and_mask(gb[(size_t)(i < N ? r : N - 1 - i0) * M + jc], (i < n && j < m && dist <= band) ? ~0u : 0u);
        }
    };
    float tn[LC_CC], gn[LC_PR];
    load_tile(jlo & ~63, tn, gn);
    for (int jt = jlo & ~63; jt < jhi; jt += 64) {
        float tv[LC_CC], gv[LC_PR];
#pragma unroll
        for (int cc = 0; cc < LC_CC; ++cc) tv[cc] = tn[cc];
#pragma unroll
        for (int r = 0; r < LC_PR; ++r) gv[r] = gn[r];
        load_tile(jt + 64, tn, gn);
#pragma unroll
        for (int cc = 0; cc < LC_CC; ++cc)
#pragma unroll
            for (int r = 0; r < LC_PR; ++r) acc[cc][r] = Kind::back(pv[cc][r], tv[cc], gv[r], acc[cc][r]);
    }
    // sum number q = cc LC_PR + r of every lane to lane q, added in lane order
#pragma unroll
    for (int cc = 0; cc < LC_CC; ++cc)
#pragma unroll
        for (int r = 0; r < LC_PR; ++r) red[(cc * LC_PR + r) * LC_PITCH + lane] = acc[cc][r];
    __syncthreads();
    float sum = 0.f;
#pragma unroll 8
    for (int x = 0; x < 64; ++x) sum = sum + red[lane * LC_PITCH + x];
    const float k = Kind::factor(scale, row_scale ? row_scale[b] : 1.f);
    if (stored) *out = oi < n ? sum * k : 0.f;
}

static int lc_check(int B, int C, int N, int M, float scale, int bandwidth) {
    if (B < 1 || C < 1 || N < 1 || M < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (!(scale == scale) || !(scale < __builtin_huge_valf()) || !(scale > -__builtin_huge_valf()))
        return fail(ALIGNER_EINVAL, "scale must be finite");
    if (bandwidth < -1) return fail(ALIGNER_EINVAL, "bandwidth must be -1 (none) or at least 0");
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if (C > LC_MAX_C) return fail(ALIGNER_EDOM, "C=%d too large (<= %d)", C, LC_MAX_C);
    if ((long long)N * M >= (1ll << 29)) return fail(ALIGNER_EDOM, "N*M=%lld too large (< 2^29)", (long long)N * M);
    return ALIGNER_OK;
}
static int lc_band(int bandwidth) { return (bandwidth < 0 || bandwidth > LC_NO_BAND) ? LC_NO_BAND : bandwidth; }

template <class Kind>
static int lc_forward(const float *pred, const float *target, const int32_t *n_dev, const int32_t *m_dev, int bandwidth,
                      float scale, float *cost_out, int B, int C, int N, int M, void *stream) {
    if (!pred || !target || !cost_out) return fail(ALIGNER_EINVAL, "null pointer");
    if (const int rc = lc_check(B, C, N, M, scale, bandwidth)) return rc;
    const int nct = (M + 63) / 64, nrb = (N + LC_RB * LC_WAVES - 1) / (LC_RB * LC_WAVES);      // nct nrb <= N M / 64 + N + M
    hipLaunchKernelGGL(lc_cost_kernel<Kind>, dim3((unsigned)nct * nrb, 1, B), dim3(64 * LC_WAVES), 0, static_cast<hipStream_t>(stream),
                       pred, target, n_dev, m_dev, lc_band(bandwidth), scale, cost_out, C, N, M, nct);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

template <class Kind>
static int lc_backward(const float *grad_cost, const float *pred, const float *target, const int32_t *n_dev,
                       const int32_t *m_dev, int bandwidth, float scale, const float *row_scale,
                       float *dpred_out, float *dtarget_out, int B, int C, int N, int M, void *stream) {
    static_assert(Kind::has_backward, "this kind has no gradient");
    if (!grad_cost || !pred || !target) return fail(ALIGNER_EINVAL, "null pointer");
    if (!dpred_out && !dtarget_out) return fail(ALIGNER_EINVAL, "null pointer: no output");
    if (const int rc = lc_check(B, C, N, M, scale, bandwidth)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int band = lc_band(bandwidth), nchunks = (C + LC_CC - 1) / LC_CC;
    if (dpred_out) {
        hipLaunchKernelGGL(lc_dpred_kernel<Kind>, dim3((N + LC_PR - 1) / LC_PR, nchunks, B), dim3(64), 0, s,
                           grad_cost, pred, target, n_dev, m_dev, band, scale, row_scale, dpred_out, C, N, M);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    if (dtarget_out) {
        hipLaunchKernelGGL(lc_dtarget_kernel<Kind>, dim3((M + 63) / 64, (nchunks + LC_WAVES - 1) / LC_WAVES, B), dim3(64 * LC_WAVES), 0, s,
                           grad_cost, pred, target, n_dev, m_dev, band, scale, row_scale, dtarget_out, C, N, M);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

}  // namespace aligner

using namespace aligner;

extern "C" {

int aligner_l1_cost_f32(const float *pred, const float *target, const int32_t *n_dev, const int32_t *m_dev, int bandwidth,
                        float scale, float *cost_out, int B, int C, int N, int M, void *stream) {
    return lc_forward<CostL1>(pred, target, n_dev, m_dev, bandwidth, scale, cost_out, B, C, N, M, stream);
}

int aligner_l1_cost_backward_f32(const float *grad_cost, const float *pred, const float *target, const int32_t *n_dev,
                                 const int32_t *m_dev, int bandwidth, float scale, const float *row_scale,
                                 float *dpred_out, float *dtarget_out, int B, int C, int N, int M, void *stream) {
    return lc_backward<CostL1>(grad_cost, pred, target, n_dev, m_dev, bandwidth, scale, row_scale, dpred_out, dtarget_out,
                               B, C, N, M, stream);
}

int aligner_l2_cost_f32(const float *pred, const float *target, const int32_t *n_dev, const int32_t *m_dev, int bandwidth,
                        float scale, int squared, float *cost_out, int B, int C, int N, int M, void *stream) {
    if (squared) return lc_forward<CostL2>(pred, target, n_dev, m_dev, bandwidth, scale, cost_out, B, C, N, M, stream);
    return lc_forward<CostL2Root>(pred, target, n_dev, m_dev, bandwidth, scale, cost_out, B, C, N, M, stream);
}

int aligner_l2_cost_backward_f32(const float *grad_cost, const float *pred, const float *target, const int32_t *n_dev,
                                 const int32_t *m_dev, int bandwidth, float scale, const float *row_scale,
                                 float *dpred_out, float *dtarget_out, int B, int C, int N, int M, void *stream) {
    return lc_backward<CostL2>(grad_cost, pred, target, n_dev, m_dev, bandwidth, scale, row_scale, dpred_out, dtarget_out,
                               B, C, N, M, stream);
}

}  // extern "C"
