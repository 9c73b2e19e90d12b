// Hard alignment search with optional pauses between tokens (aligner_pausepath, include/aligner_amd.h).
//
// A Viterbi search over the CTC topology of an utterance's token sequence: states s = 0 .. 2 t_x, s = 2g the pause in
// gap g (the place before token g; gap t_x trails), s = 2x+1 token x.  A token takes at least one frame, a pause
// zero or more, and a gap whose mask is 0 holds no pause.  Build-defined spec (the reference snapshot has no code for
// it), restated in numpy by tests/pausepath_oracle.py, which the kernel equals bit for bit:
//
//   T[x,y] = best(T[x,y-1], P[x,y-1], T[x-1,y-1]) + value[x,y]          (stay, advance out of the pause, skip the gap)
//   P[g,y] = best(P[g,y-1], T[g-1,y-1])           + pause[y]            (stay, advance out of token g-1)
//
// `best` takes the first candidate that EXISTS at frame y-1 and replaces it by a later one only when that one is
// strictly greater (a NaN never replaces anything); a state exists inside its band only (token x: x <= y <= t_y - t_x + x,
// pause g: g <= y <= t_y - 1 - t_x + g and its gap allowed).  Absent candidates are excluded, never scored, so the
// backtrack is a legal path whatever the scores hold.  Only the band's lower edge needs a test in the sweep: an in-band
// cell's candidates are never above their own band's upper edge, and a cell outside its band (whose registers then
// hold garbage) is never a candidate of an in-band one.
//
// One workgroup of 256 threads per utterance.  A thread owns token x and gap x for x = tid + 256 r, r < R (Tx <= 1024,
// as maxpath_generic_kernel); the owner of token t_x-1 also keeps the trailing gap, whose only foreign operand is that
// token.  The two states of a thread need one foreign value per frame, T[x-1,y-1]: a DPP shift inside a wave, an LDS slot
// between waves, one barrier per frame.  Scores are register-resident 32 / 16 / 8 frames ahead of the sweep (1 / 2 / 4 row groups: at most 48 loads in
// flight, which the load counter can tell apart; each element is re-loaded right after the frame that consumed it: pitched rows and 16-bit scores are read in place, any
// alignment, up-cast where they are consumed), so a frame waits only for a load issued that many frames earlier.  A cell's decision takes 3 bits (2 token, 1 pause), packed per 32-frame
// tile into three words per row; the words stay in LDS when they fit, else they go to the caller's workspace and come
// back window by window for the walk.  The backtrack runs in the same launch on one wave: per tile the 33 rows the
// walk can reach are read into lanes once, then every frame is a v_readlane away -- no dependent LDS round trip per
// frame.  Durations are the run lengths of the walked states (one writer, no atomics): deterministic.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "aligner_amd.h"
#include "common.h"
#include "device.h"

namespace aligner {
namespace {

constexpr int PP_THREADS = 256;
constexpr int PP_TC = 32;                       // frames per tile == decision bits per word
constexpr int PP_MAX_R = 4;                     // row groups per thread: Tx <= 1024
constexpr int PP_BND_LD = 20;                   // floats per parity of the wave-boundary slots (4 * R + 1 used)
constexpr size_t PP_LDS_BUDGET = 160 * 1024;    // gfx950: one workgroup may own the CU's whole LDS

enum { PP_F32 = 0, PP_BF16 = 1, PP_F16 = 2 };

typedef __attribute__((address_space(3))) unsigned pp_lds_u32;
typedef __attribute__((address_space(1))) unsigned pp_global_u32;

struct PauseParams {
    const void *value;            // [B,Tx,ld] scores
    const float *pause;           // [B,Ty] or null (then pause_score)
    const unsigned char *gap_mask;   // [B,Tx+1] or null
    const int *t_xs, *t_ys;
    int *tok, *dur, *pauses, *sdur;
    float *score;
    unsigned *gbits;              // workspace: [B][NT][3][Tx+1] decision words (used when they do not fit LDS)
    unsigned long long *stamps;   // debug (aligner_debug_set_stamps): [B][16 waves][16]; 0 entry, 1 sweep done, 3 walk done, 5 end, 6 / 7 wall clock
    float pause_score;
    int ld, B, Tx, Ty, NT;
    int WT;                       // tiles per LDS window of decision words (>= the utterance's tiles when in_lds)
    int in_lds;
    int lds_dec_off;              // byte offset of the decision words in LDS
};

#define PP_STAMP(k)                                                                                     \
    do {                                                                                                \
        if (p.stamps && (threadIdx.x & 63) == 0)                                                        \
            p.stamps[((size_t)blockIdx.x * 16 + (threadIdx.x >> 6)) * 16 + (k)] =                        \
                ((k) == 6 || (k) == 7) ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime();   \
    } while (0)

// A score travels through its prefetch register as the bits that were loaded (16 of them for bf16 / fp16: widening them
// at the load is an instruction on the load's result as well) and is up-cast where the sweep consumes it: a cast at the
// load sits in the frame that issues the load and makes that frame wait for it.
template <int VT> struct pp_raw { typedef unsigned short type; };
template <> struct pp_raw<PP_F32> { typedef float type; };
template <int VT> __device__ __forceinline__ typename pp_raw<VT>::type pp_load(const void *base, size_t idx) {
    return static_cast<const typename pp_raw<VT>::type *>(base)[idx];
}
template <int VT> __device__ __forceinline__ float pp_cast16(unsigned short raw) {
    if (VT == PP_BF16) return __builtin_bit_cast(float, (unsigned)raw << 16);
    return (float)__builtin_bit_cast(_Float16, raw);
}

__device__ __forceinline__ float pp_wave_shr1(float lane0, float src) {
    // lane i <- src[lane i-1]; lane 0 keeps `lane0`
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, lane0), __builtin_bit_cast(int, src),
                                                                 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

// Every element of every requested output of an utterance without a path.
__device__ __forceinline__ void pp_write_infeasible(const PauseParams &p, int b) {
    const int tid = threadIdx.x;
    if (p.dur) for (int i = tid; i < p.Tx; i += PP_THREADS) p.dur[(size_t)b * p.Tx + i] = 0;
    if (p.pauses) for (int i = tid; i <= p.Tx; i += PP_THREADS) p.pauses[(size_t)b * (p.Tx + 1) + i] = 0;
    if (p.sdur) for (int i = tid; i <= 2 * p.Tx; i += PP_THREADS) p.sdur[(size_t)b * (2 * p.Tx + 1) + i] = 0;
    if (p.tok) for (int i = tid; i < p.Ty; i += PP_THREADS) p.tok[(size_t)b * p.Ty + i] = -1;
    if (p.score && tid == 0) p.score[b] = -__builtin_inff();
}

template <int R, int VT, bool HASP>
__global__ __launch_bounds__(PP_THREADS) void pausepath_kernel(PauseParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    PP_STAMP(6);
    PP_STAMP(0);
    const int tx = p.t_xs[b], ty = p.t_ys[b];
    if (!(tx >= 1 && ty >= 1 && tx <= ty && tx <= p.Tx && ty <= p.Ty)) {     // uniform
        pp_write_infeasible(p, b);
        return;
    }
    int *durL = reinterpret_cast<int *>(smem);                       // [2 Tx + 2] frames per state
    float *endL = reinterpret_cast<float *>(durL + 2 * p.Tx + 2);    // [0] the path's last state, [1] its score
    float *bnd = endL + 2;                                           // [2][PP_BND_LD] last lane of every wave, by frame parity; [256 + PP_BND_LD] dummies
    unsigned *dec = reinterpret_cast<unsigned *>(smem + p.lds_dec_off);
    const int RP = tx + 1;                                           // rows of a decision plane: tokens / gaps 0 .. t_x
    const int nt = (ty + PP_TC - 1) / PP_TC;
    unsigned *gdec = p.in_lds ? nullptr : p.gbits + (size_t)b * p.NT * 3 * (p.Tx + 1);

    for (int i = tid; i < 2 * p.Tx + 2; i += PP_THREADS) durL[i] = 0;

    const unsigned char *gm = p.gap_mask ? p.gap_mask + (size_t)b * (p.Tx + 1) : nullptr;
    const bool allow_trail = !gm || gm[tx] != 0;
    const float *pz = p.pause ? p.pause + (size_t)b * p.Ty : nullptr;
    const int rt = (tx - 1) >> 8;                                    // row group of the last token
    const bool trail_owner = tid == ((tx - 1) & 255);

    // Frames the scores (PF) and the pause row (PFP) are loaded ahead of the sweep.  vmcnt counts 63 loads: with more in
    // flight the wait for the oldest one is a wait for younger ones too, so R * PF + PFP stays at 48.
    constexpr int PF = R == 1 ? 32 : R == 2 ? 16 : 8, PFP = 16;
    float T[R], P[R], pv[PFP];
    typename pp_raw<VT>::type v[R][PF];
    unsigned tlo[R], thi[R], pb[R];
    bool allow[R];
    size_t rowoff[R];
    float PT = 0.0f;                                                 // trailing pause (meaningful in its owner)
    unsigned ptb = 0u;
    // a zero the compiler cannot see through: the pause row is read with vector loads (a scalar load would share its
    // counter with the LDS traffic, and the per-frame barrier's lgkmcnt(0) would wait for memory)
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    const float *pzv = HASP ? pz + vzero : nullptr;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int x = tid + 256 * r;
        allow[r] = x < tx && (!gm || gm[x] != 0);
        const int xr = x < tx ? x : tx - 1;                          // clamped: every load stays in the utterance's block
        rowoff[r] = ((size_t)b * p.Tx + xr) * (size_t)p.ld;
        T[r] = P[r] = 0.0f;
        tlo[r] = thi[r] = pb[r] = 0u;
#pragma unroll
        for (int j = 0; j < PF; ++j) v[r][j] = pp_load<VT>(p.value, rowoff[r] + (j < ty ? j : ty - 1));
    }
#pragma unroll
    for (int j = 0; j < PFP; ++j) pv[j] = HASP ? pzv[j < ty ? j : ty - 1] : p.pause_score;
    // y = 0 takes the general step: nothing of the thread's own exists at y-1, so both states take `up` -- which for
    // x = 0 is the slot nobody writes, preset to -0.0f, the one value with (-0.0f) + s == s for every s, bit for bit
    if (tid < 2) bnd[tid * PP_BND_LD] = -0.0f;
    const int bslot = lane == 63 ? wave + 1 : 2 * PP_BND_LD + tid;   // (the dummies: [256] behind the two parities)
    __syncthreads();

    // One tile of the sweep.  FULL: all 32 frames exist -- straight-line code, so that the compiler counts the loads in
    // flight (behind a branch per frame it waits for all of them); the utterance's last, partial tile takes the branches.
    auto sweep_tile = [&](const int t, auto full) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full)::value;
#pragma unroll
        for (int j = 0; j < PP_TC; ++j) {
            const int y = PP_TC * t + j;
            if (FULL || y < ty) {                                    // uniform
                const float ps = HASP ? pv[j % PFP] : p.pause_score;
                const float *bsrc = bnd + ((y + 1) & 1) * PP_BND_LD; // frame y-1's
                float Tt = 0.0f;                                     // T[t_x-1, y-1] in the trailing gap's owner
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int x = tid + 256 * r;
                    const float Tp = T[r], Pp = P[r];
                    const float up = pp_wave_shr1(bsrc[4 * r + wave], Tp);      // T[x-1, y-1]
                    const bool below = y > x;                        // the thread's own states exist at y-1
                    const bool has_up = x >= 1;
                    // pause x: stay, advance out of token x-1
                    const bool pa = !below || (has_up && up > Pp);
                    P[r] = (pa ? up : Pp) + ps;
                    pb[r] |= (pa ? 1u : 0u) << j;
                    // token x: stay, advance out of pause x, skip from token x-1
                    const bool t1 = allow[r] && Pp > Tp;
                    const float b1 = t1 ? Pp : Tp;
                    const bool t2 = !below || (has_up && up > b1);
                    float sc;
                    if constexpr (VT == PP_F32) sc = v[r][j % PF]; else sc = pp_cast16<VT>(v[r][j % PF]);
                    T[r] = (t2 ? up : b1) + sc;
                    tlo[r] |= ((t1 && !t2) ? 1u : 0u) << j;
                    thi[r] |= (t2 ? 1u : 0u) << j;
                    Tt = (R == 1 || r == rt) ? Tp : Tt;
                }
                // trailing pause t_x: stay, advance out of token t_x-1
                const bool ta = !(y > tx) || Tt > PT;
                PT = (ta ? Tt : PT) + ps;
                ptb |= (ta ? 1u : 0u) << j;
                // the wave's last lane publishes its tokens; the other lanes store into a slot of their own that nobody
                // reads -- a branch here would end the basic block, and the compiler then sinks the packing of the decision
                // bits to the end of the tile, with every frame's three lane masks alive until then
#pragma unroll
                for (int r = 0; r < R; ++r) bnd[bslot + (y & 1) * PP_BND_LD + (lane == 63 ? 4 * r : 0)] = T[r];
                // the element just consumed makes room for the one PF frames on
                const int yn = (y + PF < ty) ? y + PF : ty - 1;
#pragma unroll
                for (int r = 0; r < R; ++r) v[r][j % PF] = pp_load<VT>(p.value, rowoff[r] + yn);
                if (HASP) pv[j % PFP] = pzv[(y + PFP < ty) ? y + PFP : ty - 1];
                lds_barrier();                      // (LDS traffic only: the score loads in flight stay in flight across it)
                __builtin_amdgcn_sched_barrier(0);                   // a frame's instructions stay in their frame (registers)
            }
        }
    };

    // the tile's decision words
    auto store_words = [&](const int t) __attribute__((always_inline)) {
        // (a use in the sweep's own basic block, ahead of the first branch: with the stores below as their only use, the
        // compiler sinks the packing of the bits into those branches and keeps every frame's lane masks alive until then)
        asm volatile("" :: "v"(ptb));
#pragma unroll
        for (int r = 0; r < R; ++r) asm volatile("" :: "v"(tlo[r]), "v"(thi[r]), "v"(pb[r]));
        // (two address spaces, stated: the compiler otherwise merges the two branches into flat stores through one pointer,
        // and behind a flat store it no longer counts the score loads in flight -- vmcnt(0) once per tile)
        if (p.in_lds) {
            pp_lds_u32 *d0 = (pp_lds_u32 *)(dec + (size_t)t * 3 * RP);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int x = tid + 256 * r;
                if (x < tx) { d0[x] = tlo[r]; d0[RP + x] = thi[r]; d0[2 * RP + x] = pb[r]; }
            }
            if (trail_owner) d0[2 * RP + tx] = ptb;
        } else {
            pp_global_u32 *d0 = (pp_global_u32 *)(gdec + (size_t)t * 3 * RP);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int x = tid + 256 * r;
                if (x < tx) { d0[x] = tlo[r]; d0[RP + x] = thi[r]; d0[2 * RP + x] = pb[r]; }
            }
            if (trail_owner) d0[2 * RP + tx] = ptb;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) tlo[r] = thi[r] = pb[r] = 0u;
        ptb = 0u;
    };
    // whole tiles in a loop of their own: its only way in is from itself, so the loads of the tile before are the only
    // ones the compiler has to count behind a frame's operands
    int t = 0;
    for (; PP_TC * t + PP_TC <= ty; ++t) {
        sweep_tile(t, std::true_type{});
        store_words(t);
    }
    if (t < nt) {
        sweep_tile(t, std::false_type{});
        store_words(t);
    }
    // the path ends in the last token unless the trailing pause exists at t_y-1 and is strictly greater
    if (trail_owner) {
        float Tl = 0.0f;
#pragma unroll
        for (int r = 0; r < R; ++r) if (r == rt) Tl = T[r];
        const bool trail = allow_trail && tx <= ty - 1 && PT > Tl;
        endL[0] = __builtin_bit_cast(float, trail ? 2 * tx : 2 * tx - 1);
        endL[1] = trail ? PT : Tl;
    }
    __threadfence_block();
    __syncthreads();
    PP_STAMP(1);

    // ---- backtrack: wave 0, state in SGPRs ----
    int s = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, endL[0]));
    int run = 0;
    const int WT = p.in_lds ? nt : p.WT;
    for (int whi = nt; whi > 0; whi -= WT) {
        const int wlo = whi - WT > 0 ? whi - WT : 0;
        if (!p.in_lds) {
            __syncthreads();                                         // the previous window is consumed
            const unsigned *src = gdec + (size_t)wlo * 3 * RP;
            const int n = (whi - wlo) * 3 * RP;
            for (int i = tid; i < n; i += PP_THREADS) dec[i] = src[i];
            __syncthreads();
        }
        if (wave == 0) {
            for (int t = whi - 1; t >= wlo; --t) {
                const unsigned *D = dec + (size_t)(t - wlo) * 3 * RP;
                // a frame moves the walk up by one token at most: rows xt-32 .. xt are all this tile can reach
                const int xt = s >> 1;
                const int xr = xt - lane > 0 ? xt - lane : 0;
                const unsigned w0 = D[xr], w1 = D[RP + xr], w2 = D[2 * RP + xr];
                const int jhi = (ty - 1 - PP_TC * t) < PP_TC - 1 ? (ty - 1 - PP_TC * t) : PP_TC - 1;
                int tokv = -1;
                for (int j = jhi; j >= 0; --j) {
                    const int l = xt - (s >> 1);
                    int d;
                    if (s & 1) {
                        const unsigned a = __builtin_amdgcn_readlane(w0, l), c = __builtin_amdgcn_readlane(w1, l);
                        d = (int)(((a >> j) & 1u) | (((c >> j) & 1u) << 1));
                        tokv = lane == j ? s >> 1 : tokv;
                    } else {
                        d = (int)((__builtin_amdgcn_readlane(w2, l) >> j) & 1u);
                        tokv = lane == j ? -2 - (s >> 1) : tokv;
                    }
                    ++run;
                    if ((t | j) == 0) d = 0;                          // frame 0 has no predecessor
                    if (d != 0) {
                        if (lane == 0) durL[s] = run;
                        run = 0;
                        s -= d;
                    }
                }
                if (p.tok && lane <= jhi) p.tok[(size_t)b * p.Ty + PP_TC * t + lane] = tokv;
            }
        }
    }
    if (wave == 0 && lane == 0) durL[s] = run;                       // the state of frame 0
    PP_STAMP(3);
    __syncthreads();

    if (p.dur) for (int i = tid; i < p.Tx; i += PP_THREADS) p.dur[(size_t)b * p.Tx + i] = i < tx ? durL[2 * i + 1] : 0;
    if (p.pauses) for (int i = tid; i <= p.Tx; i += PP_THREADS) p.pauses[(size_t)b * (p.Tx + 1) + i] = i <= tx ? durL[2 * i] : 0;
    if (p.sdur) for (int i = tid; i <= 2 * p.Tx; i += PP_THREADS) p.sdur[(size_t)b * (2 * p.Tx + 1) + i] = i <= 2 * tx ? durL[i] : 0;
    if (p.tok) for (int i = ty + tid; i < p.Ty; i += PP_THREADS) p.tok[(size_t)b * p.Ty + i] = -1;
    if (p.score && tid == 0) p.score[b] = endL[1];
    PP_STAMP(5);
    PP_STAMP(7);
}

size_t pp_fixed_lds(int Tx) { return align_up((size_t)(2 * Tx + 2 + 2 + 2 * PP_BND_LD + PP_THREADS + PP_BND_LD) * 4, 16); }
size_t pp_tile_bytes(int Tx) { return (size_t)3 * (Tx + 1) * 4; }
int pp_tiles(int Ty) { return (Ty + PP_TC - 1) / PP_TC; }
bool pp_fits_lds(int Tx, int Ty, size_t budget) { return pp_fixed_lds(Tx) + pp_tiles(Ty) * pp_tile_bytes(Tx) <= budget; }

template <int R>
int pp_launch(const PauseParams &p, int vt, size_t lds, hipStream_t s) {
    void (*k)(PauseParams);
    if (p.pause) k = vt == PP_F32 ? pausepath_kernel<R, PP_F32, true> : vt == PP_BF16 ? pausepath_kernel<R, PP_BF16, true> : pausepath_kernel<R, PP_F16, true>;
    else k = vt == PP_F32 ? pausepath_kernel<R, PP_F32, false> : vt == PP_BF16 ? pausepath_kernel<R, PP_BF16, false> : pausepath_kernel<R, PP_F16, false>;
    ALIGNER_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void *>(k), lds));
    hipLaunchKernelGGL(k, dim3(p.B), dim3(PP_THREADS), lds, s, p);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

}  // namespace
}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_pausepath_workspace_bytes(int B, int Tx, int Ty) {
    if (B < 1 || Tx < 1 || Ty < 1 || Tx > 256 * PP_MAX_R) return 0;
    if (pp_fits_lds(Tx, Ty, PP_LDS_BUDGET)) return 0;
    return (size_t)B * pp_tiles(Ty) * pp_tile_bytes(Tx);
}

int aligner_pausepath(const void *value, int value_dtype, int ld_value, const float *pause, float pause_score,
                      const uint8_t *gap_mask, const int32_t *t_xs, const int32_t *t_ys, int32_t *tok_out,
                      int32_t *durations_out, int32_t *pauses_out, int32_t *state_durations_out, float *score_out,
                      void *workspace, size_t workspace_bytes, int B, int Tx, int Ty, void *stream) {
    if (!value || !t_xs || !t_ys) return fail(ALIGNER_EINVAL, "null pointer");
    if (!tok_out && !durations_out && !pauses_out && !state_durations_out && !score_out)
        return fail(ALIGNER_EINVAL, "no output requested");
    if (B < 0 || Tx < 1 || Ty < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (ld_value < Ty) return fail(ALIGNER_EINVAL, "ld_value=%d < Ty=%d", ld_value, Ty);
    int vt;
    switch (value_dtype) {
        case ALIGNER_DT_F32: vt = PP_F32; break;
        case ALIGNER_DT_BF16: vt = PP_BF16; break;
        case ALIGNER_DT_F16: vt = PP_F16; break;
        default: return fail(ALIGNER_EINVAL, "value_dtype %d (F32, BF16 or F16)", value_dtype);
    }
    if (Tx > 256 * PP_MAX_R) return fail(ALIGNER_EDOM, "Tx=%d too large (<= %d)", Tx, 256 * PP_MAX_R);
    if (B == 0) return ALIGNER_OK;

    PauseParams p{};
    p.value = value; p.pause = pause; p.gap_mask = gap_mask; p.t_xs = t_xs; p.t_ys = t_ys;
    p.tok = tok_out; p.dur = durations_out; p.pauses = pauses_out; p.sdur = state_durations_out; p.score = score_out;
    p.stamps = g_debug_stamps;
    p.pause_score = pause_score;
    p.ld = ld_value; p.B = B; p.Tx = Tx; p.Ty = Ty; p.NT = pp_tiles(Ty);
    p.lds_dec_off = (int)pp_fixed_lds(Tx);
    // the same predicate as aligner_pausepath_workspace_bytes: a caller who was told "0 bytes" is never asked for more
    const size_t budget = PP_LDS_BUDGET;
    size_t lds;
    if (pp_fits_lds(Tx, Ty, budget)) {
        p.in_lds = 1;
        p.WT = p.NT;
        lds = pp_fixed_lds(Tx) + p.NT * pp_tile_bytes(Tx);
    } else {
        const size_t need = (size_t)B * p.NT * pp_tile_bytes(Tx);
        if (!workspace || workspace_bytes < need)
            return fail(ALIGNER_ENOSPC, "workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, need);
        const size_t wt = (budget - pp_fixed_lds(Tx)) / pp_tile_bytes(Tx);
        if (wt < 1) return fail(ALIGNER_EDOM, "no LDS for one tile of decision words (Tx=%d)", Tx);
        p.in_lds = 0;
        p.WT = (int)(wt < (size_t)p.NT ? wt : (size_t)p.NT);
        p.gbits = static_cast<unsigned *>(workspace);
        lds = pp_fixed_lds(Tx) + p.WT * pp_tile_bytes(Tx);
    }
    if ((size_t)device_lds_limit() < lds)
        return fail(ALIGNER_EDOM, "the device gives a workgroup %d bytes of LDS, %zu are needed (built for gfx950)", device_lds_limit(), lds);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (Tx <= 256) return pp_launch<1>(p, vt, lds, s);
    if (Tx <= 512) return pp_launch<2>(p, vt, lds, s);
    return pp_launch<4>(p, vt, lds, s);
}

}  // extern "C"
