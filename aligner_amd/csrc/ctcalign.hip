// CTC forced alignment from emissions (aligner_ctc_align, include/aligner_amd.h).
//
// The Viterbi path of a transcript through the frame scores of a CTC acoustic model: emissions e[y, v] = log_probs[b, y, v]
// (frame-major, one column per vocabulary entry), labels lab[0 .. t_x-1].  States s = 0 .. 2 t_x: s = 2g is the blank in
// gap g (the place before token g; gap t_x trails) and scores e[y, blank], s = 2x+1 is token x and scores e[y, lab[x]].
// A token takes at least one frame, a blank zero or more.  Build-defined spec, restated in numpy by
// tests/ctcalign_oracle.py, which the kernel equals bit for bit:
//
//   T[x,y] = best(T[x,y-1], P[x,y-1], T[x-1,y-1] if lab[x] != lab[x-1]) + e[y, lab[x]]     (stay, advance, skip)
//   P[g,y] = best(P[g,y-1], T[g-1,y-1])                                 + e[y, blank]      (stay, advance)
//
// `best` is aligner_pausepath's: the first candidate that EXISTS at frame y-1, replaced by a later one only when that
// one is strictly greater (a NaN never replaces anything); absent candidates are excluded, never scored.  Between two
// equal labels the blank is mandatory, so the bands depend on the repeats: with r[x] = (x >= 1 and lab[x] == lab[x-1]),
// R[x] = r[0] + .. + r[x] and Rt = R[t_x-1],
//   token x exists at y iff  x + R[x] <= y          and  t_y-1-y >= (t_x-1-x) + (Rt - R[x]),
//   blank g exists at y iff  g + R[g-1] <= y        and  t_y-1-y >= (t_x-g) + (Rt - R[g])      (R[-1] = 0, R[t_x] = Rt)
// and an utterance has a path iff t_x + Rt <= t_y.
//
// Only the lower edges are tested in the sweep (lob = x + R[x] - r[x] for blank x, lot = x + R[x] for token x), by
// pausepath.hip's argument restated with repeats.  Write hi_t[x], hi_b[g] for the upper edges above.  Then
// hi_b[x] = hi_t[x] - 1 and hi_t[x-1] = hi_b[x] - r[x], so for a cell inside its band at frame y every candidate at y-1
// is at or below its own upper edge: stay trivially; blank x under token x since y-1 <= hi_t[x]-1 = hi_b[x]; token x-1
// under blank x since y-1 <= hi_b[x]-1 <= hi_t[x-1]; and the skip from token x-1 into token x, legal only when r[x] = 0,
// since then hi_t[x-1] = hi_b[x] = hi_t[x]-1.  A candidate that passes its lower-edge test is therefore inside its band,
// and a cell outside its band (whose registers hold garbage) is never a candidate of an in-band one; the walk starts on
// an in-band cell and follows recorded choices, so it never reads a garbage decision either.
//
// Layout: pausepath.hip's.  One workgroup of 256 threads per utterance; a thread owns token x and gap x for
// x = tid + 256 r, r < R (L <= 1024); the owner of token t_x-1 keeps the trailing gap.  One foreign value per frame,
// T[x-1,y-1]: a DPP shift inside a wave, an LDS slot between waves, one barrier per frame.  3 decision bits per cell,
// packed per 32-frame tile, in LDS when they fit and else in the caller's workspace, walked back window by window on
// wave 0 with its state in SGPRs; durations are run lengths written by that one walker.
// What differs:
//   * loads: the emissions are frame-major, so a thread keeps lab[x] in a register and reads e[y * stride_t + lab[x]]:
//     a uniform row base (scalar registers) plus a per-lane column.  The same register ring as the pause kernel's, 32 /
//     16 / 8 frames ahead; the blank column is one more such row, 16 frames ahead, read through a column index the
//     compiler cannot prove uniform (a scalar load would share its counter with the LDS traffic and put a memory wait
//     on every frame's barrier).
//   * the skip candidate is gated by a per-thread bit, lab[x] != lab[x-1]; lab[x-1] comes through LDS once at start-up.
//   * R comes from a workgroup scan of r at start-up (segments.h: scan_durations).
//   * the labels are checked as they are loaded: one outside [0, V) makes the utterance infeasible before any emission
//     is read, so no load leaves a row of V.
//   * two more outputs from the walk, a lane per frame like tok: labels (lab[x] / blank) and frame_scores (the emission
//     at that cell, loaded again; the load of a tile is consumed one tile later, so the walk does not wait for it).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "aligner_amd.h"
#include "common.h"
#include "device.h"
#include "segments.h"

namespace aligner {
namespace {

constexpr int CA_THREADS = 256;
constexpr int CA_TC = 32;                       // frames per tile == decision bits per word
constexpr int CA_MAX_R = 4;                     // row groups per thread: L <= 1024
constexpr int CA_BND_LD = 20;                   // floats per parity of the wave-boundary slots (4 * R + 1 used)
constexpr size_t CA_LDS_BUDGET = 160 * 1024;    // gfx950: one workgroup may own the CU's whole LDS

enum { CA_F32 = 0, CA_BF16 = 1, CA_F16 = 2 };

typedef __attribute__((address_space(3))) unsigned ca_lds_u32;
typedef __attribute__((address_space(1))) unsigned ca_global_u32;

struct CtcParams {
    const void *lp;               // [B,T,V] emissions at stride_b / stride_t elements
    const int *targets;           // [B,L]
    const int *t_xs, *t_ys;
    int *tok, *labels, *dur, *pauses, *sdur;
    float *fscore, *score;
    unsigned *gbits;              // workspace: [B][NT][3][L+1] decision words (used when they do not fit LDS)
    long long stride_b;
    unsigned stride_t;            // (T-1) * stride_t + V <= 2^31: a frame's row offset fits 32 bits
    int V, blank, B, L, T, NT;
    int WT;                       // tiles per LDS window of decision words (>= the utterance's tiles when in_lds)
    int in_lds;
    int lds_dec_off;              // byte offset of the decision words in LDS
};

// An emission travels through its prefetch register as the bits that were loaded and is up-cast where the sweep
// consumes it (pausepath.hip: a cast at the load makes the frame that issues the load wait for it).
template <int VT> struct ca_raw { typedef unsigned short type; };
template <> struct ca_raw<CA_F32> { typedef float type; };
// row: the utterance's block plus a uniform frame offset in elements; colb: the lane's vocabulary entry as a byte offset.
// (The compiler keeps base + colb as a 64-bit vector address per row and adds the frame's scalar offset with one
// v_lshl_add_u64 per load.  Stating the row address as scalar with readfirstlane did not turn the loads into the
// scalar-base form and cost 8% more instructions per tile, so the plain form stays.)
template <int VT> __device__ __forceinline__ typename ca_raw<VT>::type ca_load(const void *base, unsigned rowoff, unsigned colb) {
    const char *row = reinterpret_cast<const char *>(static_cast<const typename ca_raw<VT>::type *>(base) + rowoff);
    return *reinterpret_cast<const typename ca_raw<VT>::type *>(row + colb);
}
template <int VT> __device__ __forceinline__ float ca_cast(typename ca_raw<VT>::type raw) {
    if constexpr (VT == CA_F32) return raw;
    else if constexpr (VT == CA_BF16) return __builtin_bit_cast(float, (unsigned)raw << 16);
    else return (float)__builtin_bit_cast(_Float16, raw);
}

__device__ __forceinline__ float ca_wave_shr1(float lane0, float src) {
    // lane i <- src[lane i-1]; lane 0 keeps `lane0`
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, lane0), __builtin_bit_cast(int, src),
                                                                 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

// Every element of every requested output of an utterance without a path.
__device__ __forceinline__ void ca_write_infeasible(const CtcParams &p, int b) {
    const int tid = threadIdx.x;
    if (p.dur) for (int i = tid; i < p.L; i += CA_THREADS) p.dur[(size_t)b * p.L + i] = 0;
    if (p.pauses) for (int i = tid; i <= p.L; i += CA_THREADS) p.pauses[(size_t)b * (p.L + 1) + i] = 0;
    if (p.sdur) for (int i = tid; i <= 2 * p.L; i += CA_THREADS) p.sdur[(size_t)b * (2 * p.L + 1) + i] = 0;
    if (p.tok) for (int i = tid; i < p.T; i += CA_THREADS) p.tok[(size_t)b * p.T + i] = -1;
    if (p.labels) for (int i = tid; i < p.T; i += CA_THREADS) p.labels[(size_t)b * p.T + i] = -1;
    if (p.fscore) for (int i = tid; i < p.T; i += CA_THREADS) p.fscore[(size_t)b * p.T + i] = 0.0f;
    if (p.score && tid == 0) p.score[b] = -__builtin_inff();
}

template <int R, int VT>
__global__ __launch_bounds__(CA_THREADS) void ctcalign_kernel(CtcParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef typename ca_raw<VT>::type raw_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int tx = p.t_xs[b], ty = p.t_ys[b];
    if (!(tx >= 1 && ty >= 1 && tx <= p.L && ty <= p.T)) {            // uniform
        ca_write_infeasible(p, b);
        return;
    }
    int *durL = reinterpret_cast<int *>(smem);                       // [2 L + 2] frames per state
    float *endL = reinterpret_cast<float *>(durL + 2 * p.L + 2);     // [0] the path's last state, [1] its score
    float *bnd = endL + 2;                                           // [2][CA_BND_LD] last lane of every wave, by frame parity; [256 + CA_BND_LD] dummies
    int *labL = reinterpret_cast<int *>(bnd + 2 * CA_BND_LD + CA_THREADS + CA_BND_LD);   // [L] the labels, for the walk
    unsigned *dec = reinterpret_cast<unsigned *>(smem + p.lds_dec_off);
    const int RP = tx + 1;                                           // rows of a decision plane: tokens / gaps 0 .. t_x
    const int nt = (ty + CA_TC - 1) / CA_TC;
    unsigned *gdec = p.in_lds ? nullptr : p.gbits + (size_t)b * p.NT * 3 * (p.L + 1);

    // ---- start-up: labels, repeats and their prefix sums (the scratch lies where the decision words go later) ----
    int *repL = reinterpret_cast<int *>(dec), *RL = repL + p.L, *wtot = RL + p.L;     // [L], [L], [4]: 2 L + 4 <= 3 (L + 1)
    const int *tg = p.targets + (size_t)b * p.L;
    int lab[R], lob[R], lot[R];
    unsigned labb[R];                                                // lab[x] as a byte offset into a frame's row
    bool skip[R];
    int bad = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int x = tid + 256 * r;
        lab[r] = x < tx ? tg[x] : 0;
        bad |= (unsigned)lab[r] >= (unsigned)p.V ? 1 : 0;
        if (x < tx) labL[x] = lab[r];
    }
    if (__syncthreads_or(bad)) {                                     // uniform; nothing of the emissions has been read
        ca_write_infeasible(p, b);
        return;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int x = tid + 256 * r;
        const bool rep = x >= 1 && x < tx && labL[x - 1] == lab[r];
        skip[r] = x >= 1 && !rep;
        lot[r] = rep ? 1 : 0;                                        // (r[x] for now)
        if (x < tx) repL[x] = lot[r];
    }
    __syncthreads();
    scan_durations(repL, RL, wtot, tx);                              // RL[x] = R[x]
    const int Rt = RL[tx - 1];
    if (tx + Rt > ty) {                                              // uniform
        ca_write_infeasible(p, b);
        return;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int x = tid + 256 * r;
        const int rx = lot[r];
        lot[r] = x + (x < tx ? RL[x] : 0);
        lob[r] = lot[r] - rx;
        if (x >= tx) lab[r] = labL[tx - 1];                          // clamped: every load stays in a row of V
        labb[r] = (unsigned)lab[r] * (unsigned)sizeof(raw_t);
    }
    for (int i = tid; i < 2 * p.L + 2; i += CA_THREADS) durL[i] = 0;

    const raw_t *base = static_cast<const raw_t *>(p.lp) + (size_t)b * p.stride_b;
    const unsigned st = p.stride_t;
    const int lobT = tx + Rt;                                        // first frame of the trailing gap
    const int rt = (tx - 1) >> 8;                                    // row group of the last token
    const bool trail_owner = tid == ((tx - 1) & 255);

    // Frames the token columns (PF) and the blank column (PFP) are loaded ahead of the sweep.  vmcnt counts 63 loads: with
    // more in flight the wait for the oldest one is a wait for younger ones too, so R * PF + PFP stays at 48.
    constexpr int PF = R == 1 ? 32 : R == 2 ? 16 : 8, PFP = 16;
    float T[R], P[R];
    raw_t v[R][PF], pv[PFP];
    unsigned tlo[R], thi[R], pb[R];
    float PT = 0.0f;                                                 // trailing blank (meaningful in its owner)
    unsigned ptb = 0u;
    // a zero the compiler cannot see through: the blank column is read with vector loads
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    const unsigned blankv = (unsigned)(p.blank + vzero) * (unsigned)sizeof(raw_t);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        T[r] = P[r] = 0.0f;
        tlo[r] = thi[r] = pb[r] = 0u;
    }
    // The rings are filled in the order in which a tile leaves them to the next one: a slot's load is followed by as
    // many younger loads as it is in the loop.  The counted waits of the loop's first frames are the worse of the two
    // ways in; with the token columns first and the blank column after them the blank of frame 0 had 6 loads behind
    // it, and every tile began with a wait for all but 6.
#pragma unroll
    for (int f = 0; f < CA_TC; ++f) {
        if (f >= CA_TC - PF) {
            const int j = f - (CA_TC - PF);
#pragma unroll
            for (int r = 0; r < R; ++r) v[r][j] = ca_load<VT>(base, (unsigned)(j < ty ? j : ty - 1) * st, labb[r]);
        }
        if (f >= CA_TC - PFP) {
            const int j = f - (CA_TC - PFP);
            pv[j] = ca_load<VT>(base, (unsigned)(j < ty ? j : ty - 1) * st, blankv);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // y = 0 takes the general step: nothing of the thread's own exists at y-1, so both states take `up` -- which for
    // x = 0 is the slot nobody writes, preset to -0.0f, the one value with (-0.0f) + s == s for every s, bit for bit
    if (tid < 2) bnd[tid * CA_BND_LD] = -0.0f;
    const int bslot = lane == 63 ? wave + 1 : 2 * CA_BND_LD + tid;   // (the dummies: [256] behind the two parities)
    __syncthreads();                                                 // (also: the scan's scratch is consumed)

    // One tile of the sweep.  FULL: all 32 frames exist -- straight-line code, so that the compiler counts the loads in
    // flight (behind a branch per frame it waits for all of them); the utterance's last, partial tile takes the branches.
    auto sweep_tile = [&](const int t, auto full) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full)::value;
#pragma unroll
        for (int j = 0; j < CA_TC; ++j) {
            const int y = CA_TC * t + j;
            if (FULL || y < ty) {                                    // uniform
                const float ps = ca_cast<VT>(pv[j % PFP]);
                const float *bsrc = bnd + ((y + 1) & 1) * CA_BND_LD; // frame y-1's
                float Tt = 0.0f;                                     // T[t_x-1, y-1] in the trailing gap's owner
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int x = tid + 256 * r;
                    const float Tp = T[r], Pp = P[r];
                    const float up = ca_wave_shr1(bsrc[4 * r + wave], Tp);      // T[x-1, y-1]
                    const bool below_b = y > lob[r];                 // blank x exists at y-1
                    const bool below_t = y > lot[r];                 // token x exists at y-1 (one frame later behind a repeat)
                    const bool has_up = x >= 1;
                    // blank x: stay, advance out of token x-1
                    const bool pa = !below_b | (has_up & (up > Pp));
                    P[r] = (pa ? up : Pp) + ps;
                    pb[r] |= (pa ? 1u : 0u) << j;
                    // token x: stay, advance out of blank x, skip from token x-1 unless the labels are equal
                    // (on a repeat's first frame only the blank exists; elsewhere !below_t implies !below_b, and t2 wins)
                    const bool t1 = !below_t | (Pp > Tp);
                    const float b1 = t1 ? Pp : Tp;
                    const bool t2 = !below_b | (skip[r] & (up > b1));
                    const float sc = ca_cast<VT>(v[r][j % PF]);
                    T[r] = (t2 ? up : b1) + sc;
                    tlo[r] |= ((t1 & !t2) ? 1u : 0u) << j;
                    thi[r] |= (t2 ? 1u : 0u) << j;
                    Tt = (R == 1 || r == rt) ? Tp : Tt;
                }
                // trailing blank t_x: stay, advance out of token t_x-1
                const bool ta = !(y > lobT) | (Tt > PT);
                PT = (ta ? Tt : PT) + ps;
                ptb |= (ta ? 1u : 0u) << j;
                // the wave's last lane publishes its tokens; the other lanes store into a slot of their own that nobody
                // reads (pausepath.hip: a branch here would end the basic block)
#pragma unroll
                for (int r = 0; r < R; ++r) bnd[bslot + (y & 1) * CA_BND_LD + (lane == 63 ? 4 * r : 0)] = T[r];
                // the elements just consumed make room for the ones PF / PFP frames on
                const unsigned yn = (unsigned)((y + PF < ty) ? y + PF : ty - 1) * st;
#pragma unroll
                for (int r = 0; r < R; ++r) v[r][j % PF] = ca_load<VT>(base, yn, labb[r]);
                pv[j % PFP] = ca_load<VT>(base, (unsigned)((y + PFP < ty) ? y + PFP : ty - 1) * st, blankv);
                lds_barrier();                      // (LDS traffic only: the loads in flight stay in flight across it)
                __builtin_amdgcn_sched_barrier(0);                   // a frame's instructions stay in their frame (registers)
            }
        }
    };

    // the tile's decision words
    auto store_words = [&](const int t) __attribute__((always_inline)) {
        // (a use in the sweep's own basic block, and two stated address spaces: pausepath.hip says why)
        asm volatile("" :: "v"(ptb));
#pragma unroll
        for (int r = 0; r < R; ++r) asm volatile("" :: "v"(tlo[r]), "v"(thi[r]), "v"(pb[r]));
        if (p.in_lds) {
            ca_lds_u32 *d0 = (ca_lds_u32 *)(dec + (size_t)t * 3 * RP);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int x = tid + 256 * r;
                if (x < tx) { d0[x] = tlo[r]; d0[RP + x] = thi[r]; d0[2 * RP + x] = pb[r]; }
            }
            if (trail_owner) d0[2 * RP + tx] = ptb;
        } else {
            ca_global_u32 *d0 = (ca_global_u32 *)(gdec + (size_t)t * 3 * RP);
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
    for (; CA_TC * t + CA_TC <= ty; ++t) {
        sweep_tile(t, std::true_type{});
        store_words(t);
    }
    if (t < nt) {
        sweep_tile(t, std::false_type{});
        store_words(t);
    }
    // the path ends in the last token unless the trailing blank exists at t_y-1 and is strictly greater
    if (trail_owner) {
        float Tl = 0.0f;
#pragma unroll
        for (int r = 0; r < R; ++r) if (r == rt) Tl = T[r];
        const bool trail = lobT <= ty - 1 && PT > Tl;
        endL[0] = __builtin_bit_cast(float, trail ? 2 * tx : 2 * tx - 1);
        endL[1] = trail ? PT : Tl;
    }
    __threadfence_block();
    __syncthreads();

    // ---- backtrack: wave 0, state in SGPRs ----
    int s = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, endL[0]));
    int run = 0;
    raw_t fs_raw = 0;                                                // the emissions of tile fs_t's frames, stored one tile later
    int fs_t = -1, fs_jhi = -1;
    const int WT = p.in_lds ? nt : p.WT;
    for (int whi = nt; whi > 0; whi -= WT) {
        const int wlo = whi - WT > 0 ? whi - WT : 0;
        if (!p.in_lds) {
            __syncthreads();                                         // the previous window is consumed
            const unsigned *src = gdec + (size_t)wlo * 3 * RP;
            const int n = (whi - wlo) * 3 * RP;
            for (int i = tid; i < n; i += CA_THREADS) dec[i] = src[i];
            __syncthreads();
        }
        if (wave == 0) {
            for (int t = whi - 1; t >= wlo; --t) {
                const unsigned *D = dec + (size_t)(t - wlo) * 3 * RP;
                // a frame moves the walk up by one token at most: rows xt-32 .. xt are all this tile can reach
                const int xt = s >> 1;
                const int xr = xt - lane > 0 ? xt - lane : 0;
                const unsigned w0 = D[xr], w1 = D[RP + xr], w2 = D[2 * RP + xr];
                const int jhi = (ty - 1 - CA_TC * t) < CA_TC - 1 ? (ty - 1 - CA_TC * t) : CA_TC - 1;
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
                // the frame's vocabulary entry and its emission: lane j holds frame 32 t + j
                const bool mine = lane <= jhi;
                const int lbl = tokv >= 0 ? labL[tokv >= 0 ? tokv : 0] : p.blank;    // (lanes past jhi hold -1)
                const size_t o = (size_t)b * p.T + CA_TC * t + lane;
                if (p.tok && mine) p.tok[o] = tokv;
                if (p.labels && mine) p.labels[o] = lbl;
                if (p.fscore) {
                    raw_t cur = 0;
                    if (mine) cur = base[(size_t)((unsigned)(CA_TC * t + lane) * st) + (unsigned)lbl];
                    if (fs_t >= 0 && lane <= fs_jhi) p.fscore[(size_t)b * p.T + CA_TC * fs_t + lane] = ca_cast<VT>(fs_raw);
                    fs_raw = cur;
                    fs_t = t;
                    fs_jhi = jhi;
                }
            }
        }
    }
    if (wave == 0) {
        if (lane == 0) durL[s] = run;                                // the state of frame 0
        if (p.fscore && fs_t >= 0 && lane <= fs_jhi) p.fscore[(size_t)b * p.T + CA_TC * fs_t + lane] = ca_cast<VT>(fs_raw);
    }
    __syncthreads();

    if (p.dur) for (int i = tid; i < p.L; i += CA_THREADS) p.dur[(size_t)b * p.L + i] = i < tx ? durL[2 * i + 1] : 0;
    if (p.pauses) for (int i = tid; i <= p.L; i += CA_THREADS) p.pauses[(size_t)b * (p.L + 1) + i] = i <= tx ? durL[2 * i] : 0;
    if (p.sdur) for (int i = tid; i <= 2 * p.L; i += CA_THREADS) p.sdur[(size_t)b * (2 * p.L + 1) + i] = i <= 2 * tx ? durL[i] : 0;
    if (p.tok) for (int i = ty + tid; i < p.T; i += CA_THREADS) p.tok[(size_t)b * p.T + i] = -1;
    if (p.labels) for (int i = ty + tid; i < p.T; i += CA_THREADS) p.labels[(size_t)b * p.T + i] = -1;
    if (p.fscore) for (int i = ty + tid; i < p.T; i += CA_THREADS) p.fscore[(size_t)b * p.T + i] = 0.0f;
    if (p.score && tid == 0) p.score[b] = endL[1];
}

size_t ca_fixed_lds(int L) { return align_up((size_t)(2 * L + 2 + 2 + 2 * CA_BND_LD + CA_THREADS + CA_BND_LD + L) * 4, 16); }
size_t ca_tile_bytes(int L) { return (size_t)3 * (L + 1) * 4; }
int ca_tiles(int T) { return (T + CA_TC - 1) / CA_TC; }
bool ca_fits_lds(int L, int T, size_t budget) { return ca_fixed_lds(L) + ca_tiles(T) * ca_tile_bytes(L) <= budget; }

template <int R>
int ca_launch(const CtcParams &p, int vt, size_t lds, hipStream_t s) {
    void (*k)(CtcParams) = vt == CA_F32 ? ctcalign_kernel<R, CA_F32> : vt == CA_BF16 ? ctcalign_kernel<R, CA_BF16> : ctcalign_kernel<R, CA_F16>;
    ALIGNER_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void *>(k), lds));
    hipLaunchKernelGGL(k, dim3(p.B), dim3(CA_THREADS), lds, s, p);
    ALIGNER_HIP_CHECK(hipGetLastError());
    return ALIGNER_OK;
}

}  // namespace
}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_ctc_align_workspace_bytes(int B, int L, int T) {
    if (B < 1 || L < 1 || T < 1 || L > 256 * CA_MAX_R) return 0;
    if (ca_fits_lds(L, T, CA_LDS_BUDGET)) return 0;
    return (size_t)B * ca_tiles(T) * ca_tile_bytes(L);
}

int aligner_ctc_align(const void *log_probs, int dtype, long long stride_b, long long stride_t, int V, int blank,
                      const int32_t *targets, const int32_t *t_xs, const int32_t *t_ys, int32_t *tok_out,
                      int32_t *labels_out, float *frame_scores_out, int32_t *durations_out, int32_t *pauses_out,
                      int32_t *state_durations_out, float *score_out, void *workspace, size_t workspace_bytes,
                      int B, int L, int T, void *stream) {
    if (!log_probs || !targets || !t_xs || !t_ys) return fail(ALIGNER_EINVAL, "null pointer");
    if (!tok_out && !labels_out && !frame_scores_out && !durations_out && !pauses_out && !state_durations_out && !score_out)
        return fail(ALIGNER_EINVAL, "no output requested");
    if (B < 0 || L < 1 || T < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (V < 1) return fail(ALIGNER_EINVAL, "V=%d < 1", V);
    if (blank < 0 || blank >= V) return fail(ALIGNER_EINVAL, "blank=%d outside [0, V=%d)", blank, V);
    if (stride_t < V) return fail(ALIGNER_EINVAL, "stride_t=%lld < V=%d", stride_t, V);
    if (stride_b < 0) return fail(ALIGNER_EINVAL, "stride_b=%lld < 0", stride_b);
    int vt;
    switch (dtype) {
        case ALIGNER_DT_F32: vt = CA_F32; break;
        case ALIGNER_DT_BF16: vt = CA_BF16; break;
        case ALIGNER_DT_F16: vt = CA_F16; break;
        default: return fail(ALIGNER_EINVAL, "dtype %d (F32, BF16 or F16)", dtype);
    }
    if (L > 256 * CA_MAX_R) return fail(ALIGNER_EDOM, "L=%d too large (<= %d)", L, 256 * CA_MAX_R);
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large (<= 65535)", B);
    // an utterance's frames are addressed by 32-bit element offsets
    const unsigned long long extent = (unsigned long long)(T - 1) * (unsigned long long)stride_t + (unsigned long long)V;
    if (extent > (1ull << 31))
        return fail(ALIGNER_EDOM, "(T-1)*stride_t+V=%llu too large (<= 2^31 elements per utterance)", extent);
    const unsigned long long words = (unsigned long long)(B > 0 ? B : 1) * ca_tiles(T) * 3ull * (unsigned long long)(L + 1);
    if (words > (1ull << 31)) return fail(ALIGNER_EDOM, "%llu decision words, too many (<= 2^31)", words);
    if (B == 0) return ALIGNER_OK;

    CtcParams p{};
    p.lp = log_probs; p.targets = targets; p.t_xs = t_xs; p.t_ys = t_ys;
    p.tok = tok_out; p.labels = labels_out; p.fscore = frame_scores_out; p.dur = durations_out; p.pauses = pauses_out;
    p.sdur = state_durations_out; p.score = score_out;
    p.stride_b = stride_b;
    p.stride_t = T > 1 ? (unsigned)stride_t : (unsigned)V;          // (a single frame: the pitch is never used)
    p.V = V; p.blank = blank; p.B = B; p.L = L; p.T = T; p.NT = ca_tiles(T);
    p.lds_dec_off = (int)ca_fixed_lds(L);
    // the same predicate as aligner_ctc_align_workspace_bytes: a caller who was told "0 bytes" is never asked for more
    const size_t budget = CA_LDS_BUDGET;
    size_t lds;
    if (ca_fits_lds(L, T, budget)) {
        p.in_lds = 1;
        p.WT = p.NT;
        lds = ca_fixed_lds(L) + p.NT * ca_tile_bytes(L);
    } else {
        const size_t need = (size_t)B * p.NT * ca_tile_bytes(L);
        if (!workspace || workspace_bytes < need)
            return fail(ALIGNER_ENOSPC, "workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, need);
        const size_t wt = (budget - ca_fixed_lds(L)) / ca_tile_bytes(L);
        if (wt < 1) return fail(ALIGNER_EDOM, "no LDS for one tile of decision words (L=%d)", L);
        p.in_lds = 0;
        p.WT = (int)(wt < (size_t)p.NT ? wt : (size_t)p.NT);
        p.gbits = static_cast<unsigned *>(workspace);
        lds = ca_fixed_lds(L) + p.WT * ca_tile_bytes(L);
    }
    if ((size_t)device_lds_limit() < lds)
        return fail(ALIGNER_EDOM, "the device gives a workgroup %d bytes of LDS, %zu are needed (built for gfx950)", device_lds_limit(), lds);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (L <= 256) return ca_launch<1>(p, vt, lds, s);
    if (L <= 512) return ca_launch<2>(p, vt, lds, s);
    return ca_launch<4>(p, vt, lds, s);
}

}  // extern "C"
