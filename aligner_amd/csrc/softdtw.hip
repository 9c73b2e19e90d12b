// Soft-DTW (Cuturi & Blondel 2017) between two frame sequences of different lengths, and its expected alignment
// matrix E = d value / d cost (Mensch & Blondel 2018); DESIGN.md 5.7.  Build-defined: include/aligner_amd.h has the
// definition (band |i - j| <= w, warp penalty on the two stalling moves, +inf costs as forbidden cells).
//
//     R[i,j] = D[i,j] + softmin_gamma(R[i-1,j-1], R[i-1,j] + p, R[i,j-1] + p)        value = R[n-1,m-1]
//
// Forward is dtw_forward.h's dense kernel (one workgroup per utterance, a lane per row on the skewed pipeline, a wave
// per 64 rows) with the soft cell of softdtw_cell.h; R (for the gradient) leaves through its tile.
//
// Arithmetic: base-2 logs with log2(e) / gamma folded into the costs on their way in, "+inf" the finite SD_BIG
// (it absorbs every addend, nothing computes inf - inf), every cell's result clamped to [-SD_BIG, SD_BIG].
//
// Backward never reads the costs.  It sweeps the same skew in reverse with E[n-1,m-1] = 1: cell (i,j) takes the three
// stored predecessor values, forms the softmin's own weights 2^(mn - pred) / sum (mn their minimum) and pushes
// E[i,j] times each to that predecessor.  Two of the three go to the lane below, added up and moved by one wave_shl a
// step.  Only differences of neighbouring R values enter, so the flow is conserved (E[0,0] = 1 up to rounding) where
// the textbook recursion exp((R[succ] - R[i,j] - D[succ]) / gamma) loses it to cancellation.  R[i,j] is dead once
// (i,j) and its three successors are done: E overwrites R in place in the gradient buffer.
#include "common.h"
#include "device.h"
#include "softdtw_cell.h"
#include "dtw_schedule.h"
#include "dtw_forward.h"

namespace aligner {

__global__ __launch_bounds__(SD_MAX_N) void softdtw_backward_kernel(DtwParams p) {
    extern __shared__ __attribute__((aligned(16))) float sd_smem[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), NW = blockDim.x >> 6;
    int n, m;
    const bool some = sd_lengths(p, b, n, m) && p.fin[b] < 0.5f * SD_BIG;
    const size_t ubase = (size_t)b * p.N * p.M;
    float *E = p.grad + ubase;
    // exact zeros outside the utterance (the sweep below writes every cell inside it), everywhere without an alignment
    for (int r = w; r < p.N; r += NW)
        for (int c = ((some && r < n) ? m : 0) + lane; c < p.M; c += 64) E[r * p.M + c] = 0.f;
    if (!some) return;
    const int nw = (n + 63) >> 6;
    const bool active = w < nw;
    float *tile = sd_smem + w * 65 * SD_PITCH;                // [65][SD_PITCH]: row 0 is the row above the wave's first
    float *ring = sd_smem + NW * 65 * SD_PITCH;               // [NW][SD_RING] what a wave's first row sends up, by column
    const int ntl = (m + 64 + SD_TW - 1) / SD_TW;             // one step beyond the forward sweep's: the look-ahead below
    const int nph = ntl + SD_LAG * (nw - 1) + 1;
    const int i = 64 * w + lane;
    int jlo, jhi;
    sd_row_span(i, n, m, p.band, jlo, jhi);
    const int r0 = lane / SD_TW, c0 = lane % SD_TW, row0 = 64 * w + r0, col0 = c0 - r0;         // (as in the forward kernel)
    const int off0 = row0 * p.M + col0, kstride = SD_RS * (p.M - 1), lds0 = r0 * SD_PITCH + c0;
    float rm1 = SD_BIG, xprev = SD_BIG;                       // R[i,j-1], R[i-1,j]
    float cl = 0.f, cdprev = 0.f, send = 0.f;                 // flow to (i,j-1); to (i-1,j-1) from the step before; to the lane below
    for (int ph = 0; ph < nph; ++ph) {
        const int t = ntl - 1 - (ph - SD_LAG * (nw - 1 - w) - 1);      // tiles from the last to the first
        const bool ldnext = active && t - 1 >= 0 && t - 1 < ntl;
        float v[SD_TW + 1];
        if (ldnext) {
            // position c of row r (-1 .. 63) of tile t-1 is R[64 w + r, (t-1) SD_TW + c - 2 - r]: two columns ahead of
            // the cell the lane is on, since a cell's weights need R[i,j-1] and the lane above R[i,j-2]
#pragma unroll
            for (int k = 0; k < SD_TW + 1; ++k) {
                const int row = row0 - 1 + SD_RS * k, col = (t - 1) * SD_TW - 1 + col0 - SD_RS * k;
                float x = SD_BIG;
                if (k < SD_TW || lane < SD_TW) {
                    if (row < 0) x = col == -1 ? 0.f : SD_BIG;                        // R[-1,-1] = 0
                    else if (row < n && col >= 0 && col < m) x = E[off0 - p.M - 1 + (t - 1) * SD_TW + k * kstride];
                }
                v[k] = x;
            }
        }
        if (active && t >= 0 && t < ntl) {
            float rv = 0.f;                                   // what the wave below sends to this wave's last row
            if (w + 1 < nw && lane < SD_TW) {
                const int col = t * SD_TW + lane - 63;
                if (col >= 0 && col < m) rv = ring[(w + 1) * SD_RING + (col & (SD_RING - 1))];
            }
            // Four steps at a time (unrolled whole, the kernel spills), their operands read up front: behind the stores
            // of E below, each read would wait in its own step.  The row above the wave's first: one entry per lane.
            const float above = tile[lane & (SD_TW - 1)];
#pragma unroll 1
            for (int c4 = SD_TW - 4; c4 >= 0; c4 -= 4) {
                float r2v[4];
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) r2v[cc] = tile[(lane + 1) * SD_PITCH + c4 + cc];
#pragma unroll
                for (int cc = 3; cc >= 0; --cc) {
                    const int c = c4 + cc;
                    const int j = t * SD_TW + c - lane;
                    const float r2 = r2v[cc];                                             // R[i,j-2]
                    const float x = sd_from_below(sd_lane(above, c), r2);                 // R[i-1,j-1]
                    float e = cl + sd_from_above(sd_lane(rv, c), send);
                    if (j == m - 1 && i == n - 1) e = 1.f;
                    e = (j >= jlo && j <= jhi) ? e : 0.f;
                    float cd, cu;
                    sd_push(x, xprev, rm1, p.pen, e, cd, cu, cl);
                    send = cu + cdprev;                                                   // both land on (i-1,j)
                    cdprev = cd;
                    tile[(lane + 1) * SD_PITCH + c] = e;
                    if (lane == 0) ring[w * SD_RING + (j & (SD_RING - 1))] = send;
                    xprev = x;
                    rm1 = r2;
                }
            }
            sd_wave_lds_sync();
#pragma unroll
            for (int k = 0; k < SD_TW; ++k) {
                const int row = row0 + SD_RS * k, col = t * SD_TW + col0 - SD_RS * k;
                if (row < n && col >= 0 && col < m) E[off0 + t * SD_TW + k * kstride] = tile[lds0 + (k * SD_RS + 1) * SD_PITCH];
            }
            sd_wave_lds_sync();
        }
        if (ldnext) {
#pragma unroll
            for (int k = 0; k < SD_TW + 1; ++k)
                if (k < SD_TW || lane < SD_TW) tile[lds0 + k * SD_RS * SD_PITCH] = v[k];
        }
        lds_barrier();
    }
}

}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_soft_dtw_workspace_bytes(int B, int N, int M, int want_grad) {
    (void)want_grad;                                          // R lives in the gradient buffer: one float per utterance either way
    if (!sd_shape_ok(B, N, M)) return 0;
    return align_up((size_t)B * sizeof(float), 256);
}

int aligner_soft_dtw_f32(const float *cost, const int32_t *n_dev, const int32_t *m_dev, float gamma, float warp_penalty,
                         int bandwidth, float *value_out, float *grad_out, void *workspace, size_t workspace_bytes,
                         int B, int N, int M, void *stream) {
    if (!cost || !value_out || !workspace) return fail(ALIGNER_EINVAL, "null pointer");
    if (B < 1 || N < 1 || M < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (!(gamma > 0.f) || !(gamma < __builtin_huge_valf())) return fail(ALIGNER_EINVAL, "gamma must be positive and finite");
    if (const int rc = dtw_check_penalty(warp_penalty)) return rc;
    if (bandwidth < -1) return fail(ALIGNER_EINVAL, "bandwidth must be -1 (none) or at least 0");
    if (const int rc = dtw_dense_domain(B, N, M)) return rc;
    const size_t need = aligner_soft_dtw_workspace_bytes(B, N, M, grad_out != nullptr);
    if (workspace_bytes < need)
        return fail(ALIGNER_ENOSPC, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DtwParams p = {};
    p.cost = cost; p.ns = n_dev; p.ms = m_dev;
    dtw_soft_scaling(p, gamma, warp_penalty);
    p.band = (bandwidth < 0 || bandwidth > SD_NO_BAND) ? SD_NO_BAND : bandwidth;
    p.value = value_out; p.grad = grad_out; p.fin = static_cast<float *>(workspace);
    p.B = B; p.N = N; p.M = M;
    const int NW = (N + 63) / 64;
    ALIGNER_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void *>(dtw_dense_forward_kernel<DtwSoft>), sd_lds_bytes(NW, false)));
    hipLaunchKernelGGL(dtw_dense_forward_kernel<DtwSoft>, dim3(B), dim3(64 * NW), sd_lds_bytes(NW, false), s, p);
    ALIGNER_HIP_CHECK(hipGetLastError());
    if (grad_out) {
        ALIGNER_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void *>(softdtw_backward_kernel), sd_lds_bytes(NW, true)));
        hipLaunchKernelGGL(softdtw_backward_kernel, dim3(B), dim3(64 * NW), sd_lds_bytes(NW, true), s, p);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

}  // extern "C"
