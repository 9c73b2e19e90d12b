// The two DP schedules of the warping kernels, shared by the soft forms (softdtw.hip, banddtw.hip) and the hard form
// (dtwpath.hip): tile sizes, the utterance's lengths, the cells a row or a band slot owns, and the movers' element
// maps.  The schedules themselves are described where the kernels are (softdtw.hip: the skewed pipeline of the dense
// table; banddtw.hip: the anti-diagonal walk of band storage).
#pragma once
#include <hip/hip_runtime.h>

namespace aligner {

// ---- dense: one lane per row, skewed; a wave per 64 rows ---------------------------------------------------------------
constexpr int   SD_TW = 16;                               // steps (and staged floats per row) per tile
constexpr int   SD_PITCH = SD_TW + 1;                     // odd: a step's 64 lanes read 64 banks
constexpr int   SD_LAG = (63 + SD_TW - 1) / SD_TW + 1;    // tiles between neighbouring waves
constexpr int   SD_RS = 64 / SD_TW;                       // rows a wave moves per pass of a tile
constexpr int   SD_RING = 64;                             // hand-off ring of a wave, entries (a column each)
constexpr int   SD_MAX_N = 1024;
constexpr int   SD_NO_BAND = 1 << 30;

// utterance b's lengths within the block; false: no alignment (a length below 1, or the corner outside the band)
// P: ns, ms, N, M, band
template <class P> __device__ __forceinline__ bool sd_lengths(const P &p, int b, int &n, int &m) {
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

inline bool sd_shape_ok(int B, int N, int M) {
    return B >= 1 && N >= 1 && M >= 1 && B <= 65535 && N <= SD_MAX_N && (long long)N * M < (1ll << 29);
}

// ---- band storage: one wave walks the anti-diagonals of [N, 2w+1] ------------------------------------------------------
constexpr int BD_T = 32;                    // steps per tile
constexpr int BD_MAX_W = 127;

// P: ns, ms, N, w
template <class P> __device__ __forceinline__ bool bd_lengths(const P &p, int b, int &n, int &m) {
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

}  // namespace aligner
