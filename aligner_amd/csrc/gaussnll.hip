// The likelihood half of a Glow-TTS / VITS training step on the hard path: the negative log-likelihood of every latent
// frame under the diagonal Gaussian of the token that owns it, and its gradient with respect to the flow's output z and
// the text encoder's mean m and log-std s.  For utterance b, with the segments of the length regulator (prior.hip,
// hardalign.hip: negative durations count as 0, a sum past T_mel is clipped) and x = x(y) the owner of frame y,
//
//   w = exp(-2 s[b,c,x]),  d = z[b,c,y] - m[b,c,x]
//   nll[b]    = sum over the counting frames y and the channels c of ( 1/2 ln 2pi + s[b,c,x] + 1/2 d^2 w )
//   dz[b,c,y] =  scale[b] d w                       (+0.0 on a frame that does not count)
//   dm[b,c,x] = -scale[b] sum_{y of x} d w          (+0.0 for a token without a counting frame)
//   ds[b,c,x] =  scale[b] ( n_x - w sum_{y of x} d^2 )
//
// A frame counts when a token owns it, y < T_mel and y < t_y[b].  What a caller composes this from otherwise is two
// regulate() calls, an elementwise chain over [B,C,T_mel], a reduction, the chain again in backward and two segment
// reductions; the data-dependent part needs one read of z and one write of dz.
//
// Ownership is segment_reduce_kernel's (hardalign.hip): a workgroup owns whole (utterance, channel) rows, a wave streams
// runs of 64 * VEC frames of its rows and reduces d w and d^2 per token with a segmented scan over the lanes keyed by the
// token; only the lanes at a segment's end touch the wave's per-token accumulators in LDS.  No atomics, one summation
// order: the same bits on every run.  m and s are read through the cache at the frame's token (neighbouring lanes read
// the same or the next token: a run of 256 frames touches a few cache lines of each), not staged: staging them would
// double the LDS per row and the accumulators already decide how many rows a wave can take.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "aligner_amd.h"
#include "common.h"
#include "segments.h"

namespace aligner {

constexpr int GN_THREADS = DUR_SCAN_THREADS;
constexpr int GN_WAVES = GN_THREADS / 64;
typedef float __attribute__((ext_vector_type(4))) gn_f32x4;
constexpr float GN_HALF_LN_2PI = 0.91893853320467274178f;

// VEC frames per lane (4: 16-byte loads and stores, rows 16-byte aligned; 1: any T_mel / pointer), CW rows per wave and
// pass, GRAD: the gradients as well.  LDS: ends[Tx] | wave_tot[4] | GRAD only: acc[GN_WAVES][CW][2][Tx] fp32.
// The key of a frame is its token, Tx for a frame that does not count.  part[b*C + c] receives the row's share of nll[b].
template <int VEC, int CW, bool GRAD>
__global__ __launch_bounds__(GN_THREADS) void gauss_nll_kernel(const float *__restrict__ z,
                                                               const float *__restrict__ mean,
                                                               const float *__restrict__ logstd,
                                                               const int *__restrict__ dur,
                                                               const int *__restrict__ t_ys,
                                                               const float *__restrict__ scale,
                                                               float *__restrict__ dz, float *__restrict__ dm,
                                                               float *__restrict__ ds, float *__restrict__ part,
                                                               int C, int Tx, int Ty) {
    extern __shared__ int gn_lds[];
    int *ends = gn_lds;
    int *wave_tot = ends + Tx;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *acc = reinterpret_cast<float *>(wave_tot + GN_WAVES) + (size_t)wave * CW * 2 * Tx;
    scan_durations(dur + (size_t)b * Tx, ends, wave_tot, Tx);
    const int ty = clamp_len(t_ys, b, Ty);
    float sc = 1.f;
    if constexpr (GRAD) {
        if (scale) sc = scale[b];
        for (int i = lane; i < CW * 2 * Tx; i += 64) acc[i] = 0.f;
        __builtin_amdgcn_wave_barrier();
    }

    const int ngroups = (C + GN_WAVES * CW - 1) / (GN_WAVES * CW);
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int c0 = (grp * GN_WAVES + wave) * CW;          // this wave's rows: c0 .. c0+CW-1 (those below C)
        if (c0 >= C) continue;
        const size_t row0 = (size_t)b * C + c0;
        float q[CW];                                          // the lane's sum of d^2 w per row
#pragma unroll
        for (int r = 0; r < CW; ++r) q[r] = 0.f;
        for (int base = 0; base < Ty; base += 64 * VEC) {
            const int y0 = base + lane * VEC;
            const bool in_row = y0 + VEC <= Ty;               // (VEC == 4: Ty % 4 == 0, so all four frames or none)
            const int yl = in_row ? y0 : 0;
            // the loads first (addresses clamped into the row: what a frame that does not count holds is never used)
            float zv[CW][VEC];
#pragma unroll
            for (int r = 0; r < CW; ++r) {
                const int cr = (c0 + r < C) ? r : 0;          // a row past C repeats row c0; nothing of it is written
                const float *p = z + (row0 + cr) * Ty + yl;
                if constexpr (VEC == 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(p);
                    zv[r][0] = v.x; zv[r][1] = v.y; zv[r][2] = v.z; zv[r][3] = v.w;
                } else {
                    zv[r][0] = *p;
                }
            }
            int k[VEC];                                       // keys (segments.h), once per run for the CW rows
            seg_keys<VEC>(ends, Tx, ty, y0, k);
            SegJoin join = {};
            if constexpr (GRAD) join = seg_join<VEC>(k, lane);
#pragma unroll
            for (int r = 0; r < CW; ++r) {
                const int cr = (c0 + r < C) ? r : 0;
                const float *mrow = mean + (row0 + cr) * Tx;
                const float *srow = logstd + (row0 + cr) * Tx;
                // m and w of the lane's frames: the first and the last frame's token are read, the two between only
                // where they have a token of their own
                float mj[VEC], wj[VEC];
                {
                    const int x = k[0] < Tx ? k[0] : 0;
                    mj[0] = mrow[x];
                    wj[0] = expf(-2.f * srow[x]);
                }
                if constexpr (VEC == 4) {
                    {
                        const int x = k[3] < Tx ? k[3] : 0;
                        mj[3] = mrow[x];
                        wj[3] = expf(-2.f * srow[x]);
                    }
#pragma unroll
                    for (int j = 1; j < 3; ++j) {
                        if (k[j] == k[0]) {
                            mj[j] = mj[0];
                            wj[j] = wj[0];
                        } else if (k[j] == k[3]) {
                            mj[j] = mj[3];
                            wj[j] = wj[3];
                        } else {
                            mj[j] = mrow[k[j]];               // (between two tokens: a token itself, < Tx)
                            wj[j] = expf(-2.f * srow[k[j]]);
                        }
                    }
                }
                float v[2][VEC], o[VEC];                      // v: d w and d^2, what the tokens sum
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const bool counts = k[j] < Tx;
                    const float d = zv[r][j] - mj[j];
                    const float dw = d * wj[j];
                    v[0][j] = counts ? dw : 0.f;
                    v[1][j] = counts ? d * d : 0.f;
                    o[j] = counts ? sc * dw : 0.f;
                    q[r] += counts ? d * dw : 0.f;
                }
                if constexpr (GRAD) {
                    if (in_row && c0 + r < C) {
                        float *p = dz + (row0 + r) * Ty + y0;
                        if constexpr (VEC == 4) {
                            const gn_f32x4 v = {o[0], o[1], o[2], o[3]};
                            __builtin_nontemporal_store(v, reinterpret_cast<gn_f32x4 *>(p));
                        } else {
                            __builtin_nontemporal_store(o[0], p);
                        }
                    }
                    seg_accumulate<VEC, 2>(v, k, Tx, acc + r * 2 * Tx, Tx, join);
                }
            }
        }
        // along x: the per-token part of the loss, the token gradients, and the accumulators cleared for the next pass
        for (int r = 0; r < CW && c0 + r < C; ++r) {
            const float *srow = logstd + (row0 + r) * Tx;
            float *a = acc + r * 2 * Tx;
            float p = 0.f;
            for (int x = lane; x < Tx; x += 64) {
                int lo = x > 0 ? ends[x - 1] : 0, hi = ends[x];
                lo = lo < ty ? lo : ty;
                hi = hi < ty ? hi : ty;
                const int n = hi - lo;                        // counting frames of token x
                const float sx = srow[x];
                if (n > 0) p += (float)n * (GN_HALF_LN_2PI + sx);
                if constexpr (GRAD) {
                    const float a1 = a[x], a2 = a[Tx + x];
                    a[x] = 0.f;
                    a[Tx + x] = 0.f;
                    const float w = expf(-2.f * sx);
                    dm[(row0 + r) * Tx + x] = n > 0 ? -(sc * a1) : 0.f;
                    ds[(row0 + r) * Tx + x] = n > 0 ? sc * ((float)n - w * a2) : 0.f;
                }
            }
            float t = p + 0.5f * q[r];
            for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
            if (lane == 0) part[row0 + r] = t;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// One wave per utterance: lane l adds the rows l, l+64, ... in order, then a fixed tree over the lanes.
__global__ __launch_bounds__(64) void gauss_nll_finish_kernel(const float *__restrict__ part,
                                                              const int *__restrict__ dur,
                                                              const int *__restrict__ t_ys, float *__restrict__ nll,
                                                              int *__restrict__ count, int C, int Tx, int Ty) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += part[(size_t)b * C + c];
    long long n = 0;
    for (int x = lane; x < Tx; x += 64) {
        const int d = dur[(size_t)b * Tx + x];
        n += d > 0 ? d : 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o);
        n += __shfl_down(n, o);
    }
    if (lane == 0) {
        const int ty = clamp_len(t_ys, b, Ty);
        if (nll) nll[b] = s;
        if (count) count[b] = n < ty ? (int)n : ty;
    }
}

// Rows per wave and pass.  The two accumulator rows per channel row bound it (about 34 KiB of LDS at most up to
// T_text = 512, 74 KiB at 2048); below that it is halved while the launch would have fewer than 2048 workgroups, so
// that a batch of few channels still fills the device (a rule of thumb, as the segment reduction's grid is).
static int gauss_nll_rows_per_wave(int B, int C, int Tx) {
    int cw = Tx <= 256 ? 4 : (Tx <= 512 ? 2 : 1);
    if (g_opt_gaussnll_rows > 0) {                            // pinned (A-B, tests): never above what LDS allows
        const int want = g_opt_gaussnll_rows >= 4 ? 4 : (g_opt_gaussnll_rows >= 2 ? 2 : 1);
        return want < cw ? want : cw;
    }
    while (cw > 1 && (long long)B * ((C + GN_WAVES * cw - 1) / (GN_WAVES * cw)) < 2048) cw /= 2;
    return cw;
}

// one call's operands (scale, dz, dm, ds: null without the gradient)
struct GaussNllArgs {
    const float *z, *mean, *logstd;
    const int32_t *dur, *t_ys;
    const float *scale;
    float *dz, *dm, *ds, *part;
    int B, C, Tx, Ty;
    hipStream_t stream;
};

template <int VEC, int CW, bool GRAD>
static int launch_gauss_nll(const GaussNllArgs &a) {
    const size_t lds = segment_lds_bytes(a.Tx, GN_WAVES, GRAD ? 2 * CW : 0);
    ALIGNER_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void *>(&gauss_nll_kernel<VEC, CW, GRAD>), lds));
    const int gx = segment_grid_x(a.B, (a.C + GN_WAVES * CW - 1) / (GN_WAVES * CW), g_opt_gaussnll_grid);
    hipLaunchKernelGGL((gauss_nll_kernel<VEC, CW, GRAD>), dim3(gx, a.B), dim3(GN_THREADS), lds, a.stream, a.z, a.mean,
                       a.logstd, a.dur, a.t_ys, a.scale, a.dz, a.dm, a.ds, a.part, a.C, a.Tx, a.Ty);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

template <int VEC, bool GRAD>
static int launch_gauss_nll_cw(int cw, const GaussNllArgs &a) {
    switch (cw) {
        case 4: return launch_gauss_nll<VEC, 4, GRAD>(a);
        case 2: return launch_gauss_nll<VEC, 2, GRAD>(a);
        default: return launch_gauss_nll<VEC, 1, GRAD>(a);
    }
}

static bool gauss_nll_shape_ok(int B, int C, int Tx) { return B >= 1 && C >= 1 && Tx >= 1 && B <= 65535 && Tx <= 2048; }

}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_gauss_nll_workspace_bytes(int B, int C, int Tx) {
    if (!gauss_nll_shape_ok(B, C, Tx)) return 0;
    return align_up((size_t)B * C * sizeof(float), 256);
}

int aligner_gauss_nll_f32(const float *z, const float *mean, const float *logstd, const int32_t *durations,
                          const int32_t *t_ys, const float *scale, float *nll_out, int32_t *count_out, float *grad_z,
                          float *grad_mean, float *grad_logstd, void *workspace, size_t workspace_bytes, int B, int C,
                          int Tx, int Ty, void *stream) {
    if (!z || !mean || !logstd || !durations || !workspace) return fail(ALIGNER_EINVAL, "null pointer");
    if (B < 1 || C < 1 || Tx < 1 || Ty < 1) return fail(ALIGNER_EINVAL, "bad shape");
    const int ngrad = (grad_z != nullptr) + (grad_mean != nullptr) + (grad_logstd != nullptr);
    if (ngrad != 0 && ngrad != 3)
        return fail(ALIGNER_EINVAL, "grad_z, grad_mean and grad_logstd go together: all three or none");
    if (ngrad == 0 && !nll_out && !count_out) return fail(ALIGNER_EINVAL, "no output requested");
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if (Tx > 2048) return fail(ALIGNER_EDOM, "Tx=%d too large (<= 2048)", Tx);
    if ((long long)B * C * Ty > INT32_MAX || (long long)B * C * Tx > INT32_MAX)
        return fail(ALIGNER_EDOM, "B*C*max(Tx,Ty) past 2^31 - 1: 32-bit frame indexing");
    const size_t need = aligner_gauss_nll_workspace_bytes(B, C, Tx);
    if (workspace_bytes < need)
        return fail(ALIGNER_ENOSPC, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *part = static_cast<float *>(workspace);
    const int cw = gauss_nll_rows_per_wave(B, C, Tx);
    const bool grad = ngrad == 3;
    const bool vec = (Ty % 4 == 0) && (reinterpret_cast<uintptr_t>(z) % 16 == 0) &&
                     (!grad || reinterpret_cast<uintptr_t>(grad_z) % 16 == 0);
    const GaussNllArgs a = {z, mean, logstd, durations, t_ys, grad ? scale : nullptr, grad_z, grad_mean, grad_logstd, part,
                            B, C, Tx, Ty, s};
    const int rc = grad ? (vec ? launch_gauss_nll_cw<4, true>(cw, a) : launch_gauss_nll_cw<1, true>(cw, a))
                        : (vec ? launch_gauss_nll_cw<4, false>(cw, a) : launch_gauss_nll_cw<1, false>(cw, a));
    if (rc != ALIGNER_OK) return rc;
    if (nll_out || count_out) {
        hipLaunchKernelGGL(gauss_nll_finish_kernel, dim3(B), dim3(64), 0, s, part, durations, t_ys, nll_out, count_out,
                           C, Tx, Ty);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

}  // extern "C"
