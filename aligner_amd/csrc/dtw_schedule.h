// The two DP schedules of the warping kernels, shared by the soft forms (softdtw.hip, banddtw.hip) and the hard form
// (dtwpath.hip): the parameter struct of all their kernels, tile sizes, the utterance's lengths, the cells a row or a
// band slot owns, the movers' element maps, and the host side the entry points share (argument checks, the soft forms'
// scaling, the dense forward kernel's LDS size).  The forward kernels of both schedules are in dtw_forward.h, written
// once for the soft and the hard cell; the backward kernels and the backtrack are where they were.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace aligner {

constexpr float SD_BIG = 1e30f;                           // "+inf" in the soft kernels' scaled units (softdtw_cell.h)

// One struct for every kernel of the three files.  A soft call leaves dec, path, length and L null / 0; a hard call
// leaves scale, unscale, grad and fin.  (The soft fields stand last: between the others they cost the hard band kernel of
// 128 columns, which has no register to spare, 60 more scalars parked in vector lanes.  The band kernels' code follows
// the fields' offsets: DESIGN.md 5.12 has what each order was seen to do.)
struct DtwParams {
    const float *cost;      // [B,N,M], in band storage [B,N,W]
    const int   *ns, *ms;   // [B] or null
    float pen;              // warp penalty (soft: scaled)
    int   band;             // dense: SD_NO_BAND for none
    int   w;                // band storage
    float *value;           // [B]
    unsigned char *dec;     // hard, shaped like cost: decisions; null: value only
    int   *path;            // hard: [B,L,2]
    int   *length;          // hard: [B]
    int B, N, M, L;         // band storage: M = N + w; hard: L = N + M - 1 or 2 N + w - 1
    float scale;            // soft: log2(e) / gamma
    float unscale;          // soft: gamma ln 2
    float *grad;            // soft, shaped like cost: R (scaled) after forward, E after backward; null: value only
    float *fin;             // soft, workspace [B]: R[n-1,m-1] scaled, SD_BIG without an alignment
};

// ---- dense: one lane per row, skewed; a wave per 64 rows ---------------------------------------------------------------
constexpr int   SD_TW = 16;                               // steps (and staged floats per row) per tile
constexpr int   SD_PITCH = SD_TW + 1;                     // odd: a step's 64 lanes read 64 banks
constexpr int   SD_LAG = (63 + SD_TW - 1) / SD_TW + 1;    // tiles between neighbouring waves
constexpr int   SD_RS = 64 / SD_TW;                       // rows a wave moves per pass of a tile
constexpr int   SD_RING = 64;                             // hand-off ring of a wave, entries (a column each)
constexpr int   SD_MAX_N = 1024;
constexpr int   SD_NO_BAND = 1 << 30;

// utterance b's lengths within the block; false: no alignment (a length below 1, or the corner outside the band)
__device__ __forceinline__ bool sd_lengths(const DtwParams &p, int b, int &n, int &m) {
    n = p.ns ? p.ns[b] : p.N;
    m = p.ms ? p.ms[b] : p.M;
    n = n < p.N ? n : p.N;
    m = m < p.M ? m : p.M;
    if (n < 1 || m < 1) return false;
    const int d = n > m ? n - m : m - n;
    return d <= p.band;
}

// the columns of row i that exist: [jlo, jhi], empty for a row past the utterance
__device__ __forceinline__ void sd_row_span(int i, int n, int m, int band, int &jlo, int &jhi) {
    jlo = i - band > 0 ? i - band : 0;
    jhi = i + band < m - 1 ? i + band : m - 1;
    if (i >= n) { jlo = 1; jhi = 0; }
}

// ---- band storage: one wave walks the anti-diagonals of [N, 2w+1] ------------------------------------------------------
constexpr int BD_T = 32;                    // steps per tile
constexpr int BD_MAX_W = 127;

__device__ __forceinline__ bool bd_lengths(const DtwParams &p, int b, int &n, int &m) {
    n = p.ns ? p.ns[b] : p.N;
    m = p.ms ? p.ms[b] : p.N;
    n = n < p.N ? n : p.N;
    m = m < p.N + p.w ? m : p.N + p.w;
    if (n < 1 || m < 1) return false;
    const int d = n > m ? n - m : m - n;
    return d <= p.w;
}

// A lane's view of one of its cells (column c, slot q): the rows [ia, ia + len) on which the cell exists
struct BdSlot { int ia; unsigned len; };
__device__ __forceinline__ BdSlot bd_slot(int c, int q, int w, int wp, int n, int m) {
    const int d = 2 * c + q - (wp - w);
    const int e = wp - 2 * c - q;                             // i - j
    int ia = e > 0 ? e : 0;                                   // j >= 0
    int ib = m + e < n ? m + e : n;                           // j < m
    if (d < 0 || d > 2 * w || ib < ia) ib = ia;
    BdSlot s;
    s.ia = ia;
    s.len = (unsigned)(ib - ia);
    return s;
}

// The movers' element k of tile s0: row rtop + 2 k + (lane >> 5), step t = lane & 31; column c, band index d.
// NC columns and BD_T steps: every (t, c) of the tile belongs to exactly one (k, lane).
template <int NC> struct BdMover {
    static constexpr int NK = (NC + BD_T / 2) / 2;
    int row0, c0, d0, t;
    __device__ __forceinline__ BdMover(int s0, int w, int wp, int lane) {
        const int hb = (s0 + wp) >> 1;                        // (s0 + wp is even; arithmetic shift for tile -1)
        t = lane & 31;
        row0 = hb - (NC - 1) + (lane >> 5);
        c0 = hb - row0 + (t >> 1);
        d0 = 2 * c0 + (t & 1) - (wp - w);
    }
    __device__ __forceinline__ int row(int k) const { return row0 + 2 * k; }
    __device__ __forceinline__ int col(int k) const { return c0 - 2 * k; }
    __device__ __forceinline__ int d(int k) const { return d0 - 4 * k; }
    // element k is a cell that exists (then its column is in [0, NC) as well); off: its place in the utterance's block
    __device__ __forceinline__ bool cell(int k, int n, int m, int w, int &off) const {
        const int r = row(k), dk = d(k), j = r + dk - w;
        off = r * (2 * w + 1) + dk;
        return r >= 0 && r < n && dk >= 0 && dk <= 2 * w && j >= 0 && j < m;
    }
    __device__ __forceinline__ bool staged(int k) const { return col(k) >= 0 && col(k) < NC; }
    __device__ __forceinline__ int lds(int k, int pitch) const { return t * pitch + col(k); }
};

// ---- host side: what the entry points of the three files check and compute alike -------------------------------------
inline int dtw_check_penalty(float warp_penalty) {
    if (!(warp_penalty >= 0.f) || !(warp_penalty < __builtin_huge_valf()))
        return fail(ALIGNER_EINVAL, "warp_penalty must be finite and not negative");
    return ALIGNER_OK;
}

// the dense table: what a workspace size of 0 stands for, and the same limits with their messages
inline bool sd_shape_ok(int B, int N, int M) {
    return B >= 1 && N >= 1 && M >= 1 && B <= 65535 && N <= SD_MAX_N && (long long)N * M < (1ll << 29);
}
inline int dtw_dense_domain(int B, int N, int M) {
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if (N > SD_MAX_N) return fail(ALIGNER_EDOM, "N=%d too large (<= %d)", N, SD_MAX_N);
    if ((long long)N * M >= (1ll << 29)) return fail(ALIGNER_EDOM, "N*M=%lld too large (< 2^29)", (long long)N * M);
    return ALIGNER_OK;
}

// band storage, likewise; `dense`: what the message says takes a wider band
inline bool bd_shape_ok(int B, int N, int bandwidth) {
    return B >= 1 && N >= 1 && bandwidth >= 0 && bandwidth <= BD_MAX_W && B <= 65535 &&
           (long long)N * (2 * bandwidth + 1) < (1ll << 29);
}
inline int dtw_band_domain(int B, int N, int bandwidth, const char *dense = "the dense calls take any band") {
    if (bandwidth > BD_MAX_W) return fail(ALIGNER_EDOM, "bandwidth=%d too large (<= %d; %s)", bandwidth, BD_MAX_W, dense);
    if (B > 65535) return fail(ALIGNER_EDOM, "B=%d too large", B);
    if ((long long)N * (2 * bandwidth + 1) >= (1ll << 29))
        return fail(ALIGNER_EDOM, "N*W=%lld too large (< 2^29)", (long long)N * (2 * bandwidth + 1));
    return ALIGNER_OK;
}

// the soft forms work in base-2 logs: log2(e) / gamma folded into the costs and the penalty, gamma ln 2 into the value
inline void dtw_soft_scaling(DtwParams &p, float gamma, float warp_penalty) {
    const double scale = 1.4426950408889634 / (double)gamma;
    p.scale = (float)scale;
    const double pen = (double)warp_penalty * scale;
    p.pen = pen < (double)SD_BIG ? (float)pen : SD_BIG;
    p.unscale = (float)((double)gamma * 0.6931471805599453);
}

// dynamic LDS of the dense kernels: a tile of 64 rows a wave (backward: and the row above them) and its ring
inline size_t sd_lds_bytes(int NW, bool backward) {
    return (size_t)NW * ((backward ? 65 : 64) * SD_PITCH + SD_RING) * sizeof(float);
}

}  // namespace aligner
