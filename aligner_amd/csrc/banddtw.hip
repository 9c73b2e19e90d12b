// Soft-DTW in band storage (include/aligner_amd.h has the definition): cost, R and E are [B,N,W],
// W = 2w + 1, element [i,d] is cell (i, j = i + d - w).  Memory is O(N w) and N has no limit of its own; the cell
// arithmetic is softdtw_cell.h's, shared with the dense kernels.
//
// Forward is dtw_forward.h's band-storage kernel with the soft cell; the walk along the anti-diagonals, the columns and
// slots of a lane and the staging of a tile are described there.
//
// Backward never reads the costs: it sweeps the tiles in reverse over the stored R (two tiles resident in an LDS
// ring, since a cell needs R one and two steps back, columns c - 1 .. c + 1 read straight from LDS, off the chain),
// and pushes E with the softmin's own weights; the chain is two additions, a DPP move and two products a step.
// E overwrites R in place.  Waves 1 .. 3 of the backward workgroup only write the exact zeros of the elements
// without a cell and leave; wave 0 sweeps.
//
// The L1 cost and its gradient in the same layout follow the kernels of l1cost.hip: formulas, sign(0) = 0, one owner
// per output element, a fixed order of summation, G selected (never multiplied) by "the cell exists".  Like them they
// are written once over the cost kind (costkind.h) and add the channels in the same order with the same operations:
// on the cells that exist the band table has the bits of the dense one, whatever the kind.
#include "common.h"
#include "device.h"
#include "softdtw_cell.h"
#include "costkind.h"
#include "dtw_schedule.h"
#include "dtw_forward.h"

namespace aligner {

constexpr int BD_BWD_WAVES = 4;             // backward: wave 0 sweeps, the others write zeros
constexpr int BD_MAX_C = 4096;
constexpr int BC_RB = 16;                   // rows per wave tile of the cost kernel
constexpr int BC_CC = 8;                    // channels per wave (gradients)
constexpr int BC_TR = 8;                    // rows per step (dtarget)
constexpr int BC_PR = 8;                    // rows per wave (dpred): BC_PR * BC_CC == 64 sums
constexpr int BC_PITCH = 65;

template <int NC>
__global__ __launch_bounds__(64 * BD_BWD_WAVES) void banddtw_backward_kernel(DtwParams p) {
    constexpr int PITCH = NC + 16, NP = NC / 64, NK = BdMover<NC>::NK;
    static_assert(NC + 2 <= PITCH, "columns -1 and NC");
    __shared__ float ring[2 * BD_T * PITCH];                  // [step & 63][column + 1]
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int n, m;
    const bool some = bd_lengths(p, b, n, m) && p.fin[b] < 0.5f * SD_BIG;
    const int w = p.w, W = 2 * w + 1, wp = w + (w & 1);
    float *E = p.grad + (size_t)b * p.N * W;
    if (wv > 0 || !some) {
        // exact zeros where no cell exists (the sweep writes every cell that does), everywhere without an alignment
        for (int r = some ? wv - 1 : wv; r < p.N; r += some ? BD_BWD_WAVES - 1 : BD_BWD_WAVES) {
            int lo = 0, hi = 0;                               // the row's cells: d in [lo, hi)
            if (some && r < n) {
                lo = w - r > 0 ? w - r : 0;
                hi = m - r + w < W ? m - r + w : W;
                hi = hi > lo ? hi : lo;
            }
            for (int d = lane; d < W; d += 64)
                if (d < lo || d >= hi) E[r * W + d] = 0.f;
        }
        return;
    }
    const int slast = n + m - 2, ntl = slast / BD_T + 1;
    for (int k = lane; k < 2 * BD_T * PITCH; k += 64) ring[k] = SD_BIG;
    BdSlot sl[NP][2];
    int finrel[NP][2];                                        // the slot's row n - 1 from ia where it is cell (n-1, m-1)
    float pd[NP][2], pu[NP][2], pl[NP][2];                    // what the slot's last cell handed to (i-1,j-1), (i-1,j), (i,j-1)
    const int ddfin = wp - (n - m);
#pragma unroll
    for (int a = 0; a < NP; ++a)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            sl[a][q] = bd_slot(64 * a + lane, q, w, wp, n, m);
            finrel[a][q] = 2 * (64 * a + lane) + q == ddfin ? n - 1 - sl[a][q].ia : -0x40000000;
            pd[a][q] = pu[a][q] = pl[a][q] = 0.f;
        }
    float v[NK];
    auto load = [&](int tl) {
        const BdMover<NC> mv(tl * BD_T, w, wp, lane);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            int off;
            float r = (mv.row(k) == -1 && mv.d(k) == w) ? 0.f : SD_BIG;       // R[-1,-1] = 0
            if (mv.cell(k, n, m, w, off)) r = E[off];
            v[k] = r;
        }
    };
    auto stage = [&](int tl) {
        const BdMover<NC> mv(tl * BD_T, w, wp, lane);
        float *half = ring + (tl & 1) * BD_T * PITCH + 1;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (mv.staged(k)) half[mv.lds(k, PITCH)] = v[k];
        }
    };
    sd_wave_lds_sync();
    load(ntl - 1);
    stage(ntl - 1);
    load(ntl - 2);
    stage(ntl - 2);
    sd_wave_lds_sync();
    for (int tl = ntl - 1; tl >= 0; --tl) {
        if (tl - 2 >= -1) load(tl - 2);
        float *cur = ring + (tl & 1) * BD_T * PITCH + 1, *oth = ring + ((tl & 1) ^ 1) * BD_T * PITCH + 1;
        const int hb = (tl * BD_T + wp) >> 1;
        int rel[NP][2];
#pragma unroll
        for (int a = 0; a < NP; ++a)
#pragma unroll
            for (int q = 0; q < 2; ++q) rel[a][q] = hb - (64 * a + lane) - sl[a][q].ia;
#pragma unroll 1
        for (int t4 = BD_T - 4; t4 >= 0; t4 -= 4) {
            // the three stored predecessors of each cell, read up front: rows t-1 and t-2 of the ring (the other
            // half's last rows for t = 0, 1), not yet overwritten by E
            float rd[4][NP], ru[4][NP], rl[4][NP];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int t = t4 + tt, q = tt & 1;
                const float *r1 = t >= 1 ? cur + (t - 1) * PITCH : oth + (BD_T - 1) * PITCH;
                const float *r2 = t >= 2 ? cur + (t - 2) * PITCH : oth + (BD_T - 2 + t) * PITCH;
#pragma unroll
                for (int a = 0; a < NP; ++a) {
                    const int c = 64 * a + lane;
                    rd[tt][a] = r2[c];
                    ru[tt][a] = r1[q == 0 ? c : c + 1];
                    rl[tt][a] = r1[q == 0 ? c - 1 : c];
                }
            }
#pragma unroll
            for (int tt = 3; tt >= 0; --tt) {
                const int t = t4 + tt, q = tt & 1, u = t >> 1;
                float nb[NP];                                 // the neighbour column's push of the step before
                if (q == 0) {                                 // from (c-1, 1) = (i+1, j): its push upwards
                    nb[0] = sd_from_below(0.f, pu[0][1]);
                    if (NP == 2) nb[NP - 1] = sd_from_below(sd_lane(pu[0][1], 63), pu[NP - 1][1]);
                } else {                                      // from (c+1, 0) = (i, j+1): its push to the left
                    nb[NP - 1] = sd_from_above(0.f, pl[NP - 1][0]);
                    if (NP == 2) nb[0] = sd_from_above(sd_lane(pl[NP - 1][0], 0), pl[0][0]);
                }
#pragma unroll
                for (int a = 0; a < NP; ++a) {
                    const float inl = q == 0 ? pl[a][1] : nb[a], inu = q == 0 ? nb[a] : pu[a][0];
                    float e = inl + (inu + pd[a][q]);
                    const int r = rel[a][q] + u;
                    if (r == finrel[a][q]) e = 1.f;
                    e = (unsigned)r < sl[a][q].len ? e : 0.f;
                    sd_push(rd[tt][a], ru[tt][a], rl[tt][a], p.pen, e, pd[a][q], pu[a][q], pl[a][q]);
                    cur[t * PITCH + 64 * a + lane] = e;
                }
            }
        }
        sd_wave_lds_sync();
        {
            const BdMover<NC> mv(tl * BD_T, w, wp, lane);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                int off;
                if (mv.cell(k, n, m, w, off)) E[off] = cur[mv.lds(k, PITCH)];
            }
        }
        sd_wave_lds_sync();
        if (tl - 2 >= -1) {
            stage(tl - 2);
            sd_wave_lds_sync();
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the cost of a kind (costkind.h) in band storage and its gradient

__device__ __forceinline__ float bc_lane(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// A wave owns rows i0 .. i0 + 15 and the 64 columns j = i0 - w + 64 ct + lane: one target load per channel feeds
// 16 cells, and row i0 + r stores d = 64 ct + lane - r, contiguous over the lanes.
template <class Kind>
__global__ __launch_bounds__(256) void bc_cost_kernel(
        const float *__restrict__ pred, const float *__restrict__ target, const int *__restrict__ ns,
        const int *__restrict__ ms, int w, float scale, float *__restrict__ cost, int C, int N, int M, int nch) {
    const int b = blockIdx.z, lane = threadIdx.x & 63;
    const int inner = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ct = inner % nch, i0 = (inner / nch) * BC_RB, W = 2 * w + 1;
    if (i0 >= N) return;
    const int n = clamp_len(ns, b, N);
    int m = clamp_len(ms, b, M);
    m = m < N + w ? m : N + w;
    const int j = i0 - w + 64 * ct + lane;
    float acc[BC_RB];
#pragma unroll
    for (int r = 0; r < BC_RB; ++r) acc[r] = 0.f;
    // (wave-uniform) the tile has a cell: a row below n, a column in [0, m)
    const int jfirst = i0 - w + 64 * ct;
    if (i0 < n && jfirst < m && jfirst + 63 >= 0) {
        const float *t = target + (size_t)b * C * M + (j < 0 ? 0 : (j < M ? j : M - 1));
        const float *p = pred + (size_t)b * C * N + (i0 + lane < N ? i0 + lane : N - 1);
        for (int c = 0; c < C; ++c, t += M, p += N) {
            const float tv = *t, pl = *p;
#pragma unroll
            for (int r = 0; r < BC_RB; ++r) acc[r] = Kind::term(tv, bc_lane(pl, r), acc[r]);
        }
    }
    float *out = cost + ((size_t)b * N + i0) * W;
#pragma unroll
    for (int r = 0; r < BC_RB; ++r) {
        const int i = i0 + r, d = 64 * ct + lane - r;
        if (i < N && d >= 0 && d < W) out[r * W + d] = (i < n && j >= 0 && j < m) ? Kind::finish(acc[r], scale) : 0.f;
    }
}

// dtarget: a wave owns 64 columns and BC_CC channels and walks the rows j0 - w .. j0 + 63 + w; lane j reads
// G[i, j - i + w], contiguous over the lanes.
template <class Kind>
__global__ __launch_bounds__(256) void bc_dtarget_kernel(
        const float *__restrict__ G, const float *__restrict__ pred, const float *__restrict__ target,
        const int *__restrict__ ns, const int *__restrict__ ms, int w, float scale, const float *__restrict__ row_scale,
        float *__restrict__ dtarget, int C, int N, int M) {
    const int b = blockIdx.z, lane = threadIdx.x & 63, W = 2 * w + 1;
    const int c0 = (blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * BC_CC;
    const int j0 = blockIdx.x * 64, j = j0 + lane;
    if (c0 >= C) return;
    const int n = clamp_len(ns, b, N);
    int m = clamp_len(ms, b, M);
    m = m < N + w ? m : N + w;
    const int cmax = (c0 + BC_CC < C ? c0 + BC_CC : C) - 1 - c0;
    float acc[BC_CC];
#pragma unroll
    for (int cc = 0; cc < BC_CC; ++cc) acc[cc] = 0.f;
    const int jlast = (j0 + 64 < m ? j0 + 64 : m) - 1;
    const int ilo = j0 - w > 0 ? j0 - w : 0;
    const int ihi = jlast + w + 1 < n ? jlast + w + 1 : n;
    if (j0 < m && ilo < ihi) {
        const float *t = target + ((size_t)b * C + c0) * M + (j < M ? j : M - 1);
        const float *p = pred + ((size_t)b * C + c0) * N;
        const float *g = G + (size_t)b * N * W;
        float tv[BC_CC];
#pragma unroll
        for (int cc = 0; cc < BC_CC; ++cc) tv[cc] = t[(size_t)(cc < cmax ? cc : cmax) * M];
        for (int ib = ilo; ib < ihi; ib += BC_TR) {
            float gv[BC_TR];
#pragma unroll
            for (int r = 0; r < BC_TR; ++r) {
                const int i = ib + r, d = j - i + w;
                const bool ok = i < ihi && j < m && d >= 0 && d < W;
                gv[r] = and_mask(g[(i < N ? i : N - 1) * W + (d < 0 ? 0 : (d < W ? d : W - 1))], ok ? ~0u : 0u);
            }
            const int rl = ib + lane < ihi ? ib + lane : ihi - 1;         // (a row of the utterance: costkind.h)
#pragma unroll
            for (int cc = 0; cc < BC_CC; ++cc) {
                const float pl = p[(size_t)(cc < cmax ? cc : cmax) * N + rl];
#pragma unroll
                for (int r = 0; r < BC_TR; ++r) acc[cc] = Kind::back(bc_lane(pl, r), tv[cc], gv[r], acc[cc]);
            }
        }
    }
    if (j >= M) return;
    const float k = -Kind::factor(scale, row_scale ? row_scale[b] : 1.f);
    float *out = dtarget + ((size_t)b * C + c0) * M + j;
#pragma unroll
    for (int cc = 0; cc < BC_CC; ++cc)
        if (cc <= cmax) out[(size_t)cc * M] = j < m && n > 0 ? acc[cc] * k : 0.f;
}

// dpred: a wave owns BC_PR rows and BC_CC channels; lane l sums the cells d = l, l + 64, ... of each row (G and
// target both contiguous over the lanes), and the 64 lanes' sums meet in LDS, added in lane order.
template <class Kind>
__global__ __launch_bounds__(64) void bc_dpred_kernel(
        const float *__restrict__ G, const float *__restrict__ pred, const float *__restrict__ target,
        const int *__restrict__ ns, const int *__restrict__ ms, int w, float scale, const float *__restrict__ row_scale,
        float *__restrict__ dpred, int C, int N, int M) {
    __shared__ float red[64 * BC_PITCH];
    const int b = blockIdx.z, lane = threadIdx.x, W = 2 * w + 1;
    const int i0 = blockIdx.x * BC_PR, c0 = blockIdx.y * BC_CC;
    const int n = clamp_len(ns, b, N);
    int m = clamp_len(ms, b, M);
    m = m < N + w ? m : N + w;
    const int cmax = (c0 + BC_CC < C ? c0 + BC_CC : C) - 1 - c0;
    const int oc = lane / BC_PR, oi = i0 + lane % BC_PR;
    float *out = dpred + ((size_t)b * C + c0 + oc) * N + oi;
    const bool stored = oc <= cmax && oi < N;
    if (i0 >= n || m < 1) {                                               // (wave-uniform)
        if (stored) *out = 0.f;
        return;
    }
    float acc[BC_CC][BC_PR];
#pragma unroll
    for (int cc = 0; cc < BC_CC; ++cc)
#pragma unroll
        for (int r = 0; r < BC_PR; ++r) acc[cc][r] = 0.f;
    const float *tb = target + ((size_t)b * C + c0) * M;
    const float *pb = pred + ((size_t)b * C + c0) * N;
    const float *gb = G + (size_t)b * N * W;
    for (int dc = 0; dc < W; dc += 64) {
        const int d = dc + lane;
#pragma unroll
        for (int r = 0; r < BC_PR; ++r) {
            const int i = i0 + r, j = i + d - w;
            const bool ok = i < n && d < W && j >= 0 && j < m;
            const float gv = and_mask(gb[(i < N ? i : N - 1) * W + (d < W ? d : W - 1)], ok ? ~0u : 0u);
            const int jc = j < 0 ? 0 : (j < m ? j : m - 1);               // (a column of the utterance: costkind.h)
#pragma unroll
            for (int cc = 0; cc < BC_CC; ++cc) {
                const int ch = cc < cmax ? cc : cmax;
                const float pv = pb[(size_t)ch * N + (i < N ? i : N - 1)];
                acc[cc][r] = Kind::back(pv, tb[(size_t)ch * M + jc], gv, acc[cc][r]);
            }
        }
    }
#pragma unroll
    for (int cc = 0; cc < BC_CC; ++cc)
#pragma unroll
        for (int r = 0; r < BC_PR; ++r) red[(cc * BC_PR + r) * BC_PITCH + lane] = acc[cc][r];
    __syncthreads();
    float sum = 0.f;
#pragma unroll 8
    for (int x = 0; x < 64; ++x) sum = sum + red[lane * BC_PITCH + x];
    const float k = Kind::factor(scale, row_scale ? row_scale[b] : 1.f);
    if (stored) *out = oi < n ? sum * k : 0.f;
}

static int bc_check(int B, int C, int N, int M, float scale, int bandwidth) {
    if (B < 1 || C < 1 || N < 1 || M < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (!(scale == scale) || !(scale < __builtin_huge_valf()) || !(scale > -__builtin_huge_valf()))
        return fail(ALIGNER_EINVAL, "scale must be finite");
    if (bandwidth < 0) return fail(ALIGNER_EINVAL, "bandwidth must be at least 0");
    if (C > BD_MAX_C) return fail(ALIGNER_EDOM, "C=%d too large (<= %d)", C, BD_MAX_C);
    return dtw_band_domain(B, N, bandwidth);
}

template <class Kind>
static int bc_forward(const float *pred, const float *target, const int32_t *n_dev, const int32_t *m_dev, int bandwidth,
                      float scale, float *cost_band_out, int B, int C, int N, int M, void *stream) {
    if (!pred || !target || !cost_band_out) return fail(ALIGNER_EINVAL, "null pointer");
    if (const int rc = bc_check(B, C, N, M, scale, bandwidth)) return rc;
    const int W = 2 * bandwidth + 1, nch = (W + BC_RB - 1 + 63) / 64, nrb = (N + BC_RB - 1) / BC_RB;
    hipLaunchKernelGGL(bc_cost_kernel<Kind>, dim3((unsigned)(nch * nrb + 3) / 4, 1, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       pred, target, n_dev, m_dev, bandwidth, scale, cost_band_out, C, N, M, nch);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

template <class Kind>
static int bc_backward(const float *grad_band, const float *pred, const float *target, const int32_t *n_dev,
                       const int32_t *m_dev, int bandwidth, float scale, const float *row_scale,
                       float *dpred_out, float *dtarget_out, int B, int C, int N, int M, void *stream) {
    static_assert(Kind::has_backward, "this kind has no gradient");
    if (!grad_band || !pred || !target) return fail(ALIGNER_EINVAL, "null pointer");
    if (!dpred_out && !dtarget_out) return fail(ALIGNER_EINVAL, "null pointer: no output");
    if (const int rc = bc_check(B, C, N, M, scale, bandwidth)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nchunks = (C + BC_CC - 1) / BC_CC;
    if (dpred_out) {
        hipLaunchKernelGGL(bc_dpred_kernel<Kind>, dim3((N + BC_PR - 1) / BC_PR, nchunks, B), dim3(64), 0, s,
                           grad_band, pred, target, n_dev, m_dev, bandwidth, scale, row_scale, dpred_out, C, N, M);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    if (dtarget_out) {
        hipLaunchKernelGGL(bc_dtarget_kernel<Kind>, dim3((M + 63) / 64, (nchunks + 3) / 4, B), dim3(256), 0, s,
                           grad_band, pred, target, n_dev, m_dev, bandwidth, scale, row_scale, dtarget_out, C, N, M);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_soft_dtw_banded_workspace_bytes(int B, int N, int bandwidth, int want_grad) {
    (void)want_grad;                                          // R lives in the gradient buffer: one float per utterance either way
    if (!bd_shape_ok(B, N, bandwidth)) return 0;
    return align_up((size_t)B * sizeof(float), 256);
}

int aligner_soft_dtw_banded_f32(const float *cost_band, const int32_t *n_dev, const int32_t *m_dev, float gamma,
                                float warp_penalty, int bandwidth, float *value_out, float *grad_band_out, void *workspace,
                                size_t workspace_bytes, int B, int N, void *stream) {
    if (!cost_band || !value_out || !workspace) return fail(ALIGNER_EINVAL, "null pointer");
    if (B < 1 || N < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (!(gamma > 0.f) || !(gamma < __builtin_huge_valf())) return fail(ALIGNER_EINVAL, "gamma must be positive and finite");
    if (const int rc = dtw_check_penalty(warp_penalty)) return rc;
    if (bandwidth < 0) return fail(ALIGNER_EINVAL, "bandwidth must be at least 0");
    if (const int rc = dtw_band_domain(B, N, bandwidth)) return rc;
    const size_t need = aligner_soft_dtw_banded_workspace_bytes(B, N, bandwidth, grad_band_out != nullptr);
    if (workspace_bytes < need)
        return fail(ALIGNER_ENOSPC, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DtwParams p = {};
    p.cost = cost_band; p.ns = n_dev; p.ms = m_dev;
    dtw_soft_scaling(p, gamma, warp_penalty);
    p.band = bandwidth; p.w = bandwidth;
    p.value = value_out; p.grad = grad_band_out; p.fin = static_cast<float *>(workspace);
    p.B = B; p.N = N; p.M = N + bandwidth;
    if (bandwidth <= 63) hipLaunchKernelGGL((dtw_band_forward_kernel<DtwSoft, 64>), dim3(B), dim3(64), 0, s, p);
    else hipLaunchKernelGGL((dtw_band_forward_kernel<DtwSoft, 128>), dim3(B), dim3(64), 0, s, p);
    ALIGNER_HIP_CHECK(hipGetLastError());
    if (grad_band_out) {
        if (bandwidth <= 63) hipLaunchKernelGGL(banddtw_backward_kernel<64>, dim3(B), dim3(64 * BD_BWD_WAVES), 0, s, p);
        else hipLaunchKernelGGL(banddtw_backward_kernel<128>, dim3(B), dim3(64 * BD_BWD_WAVES), 0, s, p);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

int aligner_l1_cost_banded_f32(const float *pred, const float *target, const int32_t *n_dev, const int32_t *m_dev, int bandwidth,
                               float scale, float *cost_band_out, int B, int C, int N, int M, void *stream) {
    return bc_forward<CostL1>(pred, target, n_dev, m_dev, bandwidth, scale, cost_band_out, B, C, N, M, stream);
}

int aligner_l1_cost_banded_backward_f32(const float *grad_band, const float *pred, const float *target, const int32_t *n_dev,
                                        const int32_t *m_dev, int bandwidth, float scale, const float *row_scale,
                                        float *dpred_out, float *dtarget_out, int B, int C, int N, int M, void *stream) {
    return bc_backward<CostL1>(grad_band, pred, target, n_dev, m_dev, bandwidth, scale, row_scale, dpred_out, dtarget_out,
                               B, C, N, M, stream);
}

int aligner_l2_cost_banded_f32(const float *pred, const float *target, const int32_t *n_dev, const int32_t *m_dev, int bandwidth,
                               float scale, int squared, float *cost_band_out, int B, int C, int N, int M, void *stream) {
    if (squared) return bc_forward<CostL2>(pred, target, n_dev, m_dev, bandwidth, scale, cost_band_out, B, C, N, M, stream);
    return bc_forward<CostL2Root>(pred, target, n_dev, m_dev, bandwidth, scale, cost_band_out, B, C, N, M, stream);
}

int aligner_l2_cost_banded_backward_f32(const float *grad_band, const float *pred, const float *target, const int32_t *n_dev,
                                        const int32_t *m_dev, int bandwidth, float scale, const float *row_scale,
                                        float *dpred_out, float *dtarget_out, int B, int C, int N, int M, void *stream) {
    return bc_backward<CostL2>(grad_band, pred, target, n_dev, m_dev, bandwidth, scale, row_scale, dpred_out, dtarget_out,
                               B, C, N, M, stream);
}

}  // extern "C"
