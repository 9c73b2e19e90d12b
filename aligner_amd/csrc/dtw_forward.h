// The forward kernels of the warping DP, one per schedule, for the soft cell (softdtw.hip, banddtw.hip) and the hard cell
// (dtwpath.hip).  What differs between the two is the cell policy Alg (DtwSoft: softdtw_cell.h; DtwHard: dtwpath.hip),
// a struct of static functions:
//
//     none()                          the value of a cell that does not exist (SD_BIG / +inf)
//     in(p, d)                        a cost on its way in
//     cell(p, diag, up, left, d, k)   the cell's value; k: the move it came by, where the policy has one
//     keep(cur, k)                    what the cell leaves in the LDS tile, as a float: R / the decision
//     Out, table(p), out(x)           the table that is written from the tile (null: value only) and its element
//     finish(p, b, fin)               the utterance's results from R[n-1,m-1]
//     TILE_HOLDS_VALUE                the tile's floats are R: it is written whether or not a table is wanted, and the band
//                                     kernel reads R[n-1,m-1] back from it; otherwise the owning lane tracks it in a register
//
// Dense: one workgroup per utterance, one lane per row, a wave per 64 rows, and nothing shared between
// workgroups.  The lanes are skewed: at its local step s wave w's lane l sits on column s - l of row 64 w + l, so
// R[i-1,j] is what the lane below computed in the step before (one wave_shr per step), R[i-1,j-1] what it handed over
// the step before that, and R[i,j-1] the lane's own register.  A wave's last row reaches the next wave through a ring in
// LDS; the waves run SD_LAG tiles of SD_TW steps apart (the skew makes a wave's last row 63 steps late) with one barrier
// per tile.  Costs come through LDS in the skewed order -- position c of row r of tile t is column t SD_TW + c - r, a
// 64-byte segment of the row in memory -- at a pitch of SD_TW + 1 floats, so the 64 lanes of a step read 64 banks; the
// table leaves through the same tile.
//
// Band storage: cost and table are [B,N,W], W = 2w + 1, element [i,d] is cell (i, j = i + d - w).
// One workgroup per utterance, and one wave of it walks the anti-diagonals s = i + j, one a step.  With
// o = w & 1 and dd = d + o, a cell sits in column c = dd >> 1 (0 .. w) and slot q = dd & 1 of the band, and on
// anti-diagonal s exactly the cells with q = s & 1 are present: one per column.  Lane l owns column l, and for
// w > 63 column 64 + l as well -- two independent cells a step in one wave, which fill each other's latencies,
// where two waves would need a hand-off and a barrier a step.  The predecessors of (c,q) are (c,q) itself two steps
// back, and one step back (c,1) and (c-1,1) for q = 0, (c,0) and (c+1,0) for q = 1: the lane's own registers and
// one DPP move from a neighbour lane (column 63 <-> 64: a readlane into the move's edge value).  No LDS, no barrier
// and no other wave on the dependent chain.
//
// Staging.  A tile is BD_T = 32 steps.  In memory the cells of a tile are, for each row i, the BD_T consecutive
// floats d = s0 + w - 2 i + t (t = 0 .. 31): 128-byte segments, two rows per wave load, issued for the next tile
// before the current tile's steps.  In LDS the tile is [t][column] at a pitch of PITCH = NC + 16 floats
// (NC = 64 or 128 columns), so a step reads lane-linear addresses.  The movers' store has lane t of a row at
// t PITCH + c0 + (t >> 1); PITCH = 16 (mod 32), so even t = 2k fall on bank c0 + k and odd t = 2k + 1 on bank
// c0 + k + 16: the 32 lanes of a row (an LDS store is served 32 lanes at a time, on 32 banks) hit 32 banks.
// The table leaves through the same tile.
#pragma once
#include "device.h"
#include "softdtw_cell.h"
#include "dtw_schedule.h"

namespace aligner {

template <class Alg>
__global__ __launch_bounds__(SD_MAX_N) void dtw_dense_forward_kernel(DtwParams p) {
    extern __shared__ __attribute__((aligned(16))) float dtw_smem[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), NW = blockDim.x >> 6;
    int n, m;
    if (!sd_lengths(p, b, n, m)) {
        if (tid == 0) Alg::finish(p, b, Alg::none());
        return;
    }
    const int nw = (n + 63) >> 6;                             // waves that own rows of this utterance
    const bool active = w < nw;
    float *tile = dtw_smem + w * 64 * SD_PITCH;               // [64][SD_PITCH] this wave's costs, then what its cells keep
    float *ring = dtw_smem + NW * 64 * SD_PITCH;              // [NW][SD_RING] each wave's last row, by column
    const int ntl = (m + 64 + SD_TW - 1) / SD_TW;             // steps 0 .. m + 62 reach every cell of 64 skewed rows
    const int nph = ntl + SD_LAG * (nw - 1) + 1;
    const size_t ubase = (size_t)b * p.N * p.M;
    const float *cost = p.cost + ubase;
    typename Alg::Out *T = Alg::table(p) ? Alg::table(p) + ubase : nullptr;
    const int i = 64 * w + lane;
    int jlo, jhi;
    sd_row_span(i, n, m, p.band, jlo, jhi);
    // the movers' element k of a tile: row r0 + SD_RS k of the wave at position c0, SD_RS rows a pass (a 64-byte segment
    // of a row per 16 lanes); its column at tile t is t SD_TW + col0 - SD_RS k and its place in memory moves by kstride
    const int r0 = lane / SD_TW, c0 = lane % SD_TW, row0 = 64 * w + r0, col0 = c0 - r0;
    const int off0 = row0 * p.M + col0, kstride = SD_RS * (p.M - 1), lds0 = r0 * SD_PITCH + c0;
    float prev = Alg::none();                                 // R[i,j-1]
    float upprev = i == 0 ? 0.f : Alg::none();                // R[i-1,j-1]; R[-1,-1] = 0
    float fin = Alg::none();
    for (int ph = 0; ph < nph; ++ph) {
        const int t = ph - SD_LAG * w - 1;                    // (the phase before a wave's first tile stages that tile)
        const bool ldnext = active && t + 1 >= 0 && t + 1 < ntl;
        float v[SD_TW];
        if (ldnext) {
#pragma unroll
            for (int k = 0; k < SD_TW; ++k) {
                const int row = row0 + SD_RS * k, col = (t + 1) * SD_TW + col0 - SD_RS * k;
                float d = Alg::none();
                if (row < n && col >= 0 && col < m) d = cost[off0 + (t + 1) * SD_TW + k * kstride];
                v[k] = Alg::in(p, d);
            }
        }
        if (active && t >= 0 && t < ntl) {
            float bv = Alg::none();                           // the row above this wave's first, columns of this tile
            if (w > 0 && lane < SD_TW) {
                const int col = t * SD_TW + lane;
                if (col < m) bv = ring[(w - 1) * SD_RING + (col & (SD_RING - 1))];
            }
            float dv[SD_TW];                                  // (read up front: behind the stores to the tile below, the compiler
#pragma unroll                                                //  keeps each read in its own step and waits for it there)
            for (int c = 0; c < SD_TW; ++c) dv[c] = tile[lane * SD_PITCH + c];
#pragma unroll
            for (int c = 0; c < SD_TW; ++c) {
                const int j = t * SD_TW + c - lane;
                const float d = dv[c];
                const float up = sd_from_below(sd_lane(bv, c), prev);
                int k;
                float cur = Alg::cell(p, upprev, up, prev, d, k);
                const bool valid = j >= jlo && j <= jhi;
                cur = valid ? cur : Alg::none();
                if (T) tile[lane * SD_PITCH + c] = Alg::keep(cur, k);
                // (columns below 0 land on entries nobody reads yet: the next wave starts SD_LAG tiles later and masks them)
                if (lane == 63) ring[w * SD_RING + (j & (SD_RING - 1))] = cur;
                if (valid && j == m - 1 && i == n - 1) fin = cur;
                upprev = up;
                prev = cur;
            }
            if (T) {
                sd_wave_lds_sync();
#pragma unroll
                for (int k = 0; k < SD_TW; ++k) {
                    const int row = row0 + SD_RS * k, col = t * SD_TW + col0 - SD_RS * k;
                    if (row < n && col >= 0 && col < m) T[off0 + t * SD_TW + k * kstride] = Alg::out(tile[lds0 + k * SD_RS * SD_PITCH]);
                }
            }
        }
        if (ldnext) {
#pragma unroll
            for (int k = 0; k < SD_TW; ++k) tile[lds0 + k * SD_RS * SD_PITCH] = v[k];
        }
        lds_barrier();
    }
    if (i == n - 1) Alg::finish(p, b, fin);
}

template <class Alg, int NC>
__global__ __launch_bounds__(64) void dtw_band_forward_kernel(DtwParams p) {
    constexpr int PITCH = NC + 16, NP = NC / 64, NK = BdMover<NC>::NK;
    __shared__ float tile[BD_T * PITCH];
    const int b = blockIdx.x, lane = threadIdx.x;
    int n, m;
    if (!bd_lengths(p, b, n, m)) {
        if (lane == 0) Alg::finish(p, b, Alg::none());
        return;
    }
    const int w = p.w, W = 2 * w + 1, wp = w + (w & 1);
    const size_t ubase = (size_t)b * p.N * W;
    const float *cost = p.cost + ubase;
    typename Alg::Out *T = Alg::table(p) ? Alg::table(p) + ubase : nullptr;
    const int slast = n + m - 2, ntl = slast / BD_T + 1;
    const int ddfin = wp - (n - m);                           // cell (n-1, m-1): column ddfin >> 1, slot ddfin & 1
    BdSlot sl[NP][2];
    int finrel[NP][2];                                        // the slot's row n - 1 from ia where it is that cell
    float x[NP][2];                                           // the lane's cells as of their last step
    bool own = false;
#pragma unroll
    for (int a = 0; a < NP; ++a)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            sl[a][q] = bd_slot(64 * a + lane, q, w, wp, n, m);
            if constexpr (!Alg::TILE_HOLDS_VALUE) {
                const bool last = 2 * (64 * a + lane) + q == ddfin;
                finrel[a][q] = last ? n - 1 - sl[a][q].ia : -0x40000000;
                own = own || last;
            }
            x[a][q] = (q == 0 && 2 * (64 * a + lane) == wp) ? 0.f : Alg::none();       // R[-1,-1] = 0, two steps before (0,0)
        }
    float fin = Alg::none();
    float v[NK];
    auto load = [&](int tl) {
        const BdMover<NC> mv(tl * BD_T, w, wp, lane);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            int off;
            float c = Alg::none();
            if (mv.cell(k, n, m, w, off)) c = cost[off];
            v[k] = Alg::in(p, c);
        }
    };
    auto stage = [&](int tl) {
        const BdMover<NC> mv(tl * BD_T, w, wp, lane);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (mv.staged(k)) tile[mv.lds(k, PITCH)] = v[k];
        }
    };
    load(0);
    stage(0);
    sd_wave_lds_sync();
    for (int tl = 0; tl < ntl; ++tl) {
        if (tl + 1 < ntl) load(tl + 1);
        const int hb = (tl * BD_T + wp) >> 1;
        int rel[NP][2];                                       // row of the slot's cell at t = 0 or 1, from ia
#pragma unroll
        for (int a = 0; a < NP; ++a)
#pragma unroll
            for (int q = 0; q < 2; ++q) rel[a][q] = hb - (64 * a + lane) - sl[a][q].ia;
#pragma unroll 1
        for (int t8 = 0; t8 < BD_T; t8 += 8) {
            float dv[8][NP];
#pragma unroll
            for (int tt = 0; tt < 8; ++tt)
#pragma unroll
                for (int a = 0; a < NP; ++a) dv[tt][a] = tile[(t8 + tt) * PITCH + 64 * a + lane];
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) {
                const int q = tt & 1, u = (t8 + tt) >> 1;
                float nb[NP];                                 // the neighbour column's cell of the step before
                if (q == 0) {                                 // (c-1, 1)
                    nb[0] = sd_from_below(Alg::none(), x[0][1]);
                    if (NP == 2) nb[NP - 1] = sd_from_below(sd_lane(x[0][1], 63), x[NP - 1][1]);
                } else {                                      // (c+1, 0)
                    nb[NP - 1] = sd_from_above(Alg::none(), x[NP - 1][0]);
                    if (NP == 2) nb[0] = sd_from_above(sd_lane(x[NP - 1][0], 0), x[0][0]);
                }
#pragma unroll
                for (int a = 0; a < NP; ++a) {
                    const float up = q == 0 ? x[a][1] : nb[a], left = q == 0 ? nb[a] : x[a][0];
                    int k;
                    float cur = Alg::cell(p, x[a][q], up, left, dv[tt][a], k);
                    const int r = rel[a][q] + u;
                    cur = (unsigned)r < sl[a][q].len ? cur : Alg::none();
                    if constexpr (!Alg::TILE_HOLDS_VALUE) fin = r == finrel[a][q] ? cur : fin;
                    x[a][q] = cur;
                    if (Alg::TILE_HOLDS_VALUE || T) tile[(t8 + tt) * PITCH + 64 * a + lane] = Alg::keep(cur, k);
                }
            }
        }
        sd_wave_lds_sync();
        if constexpr (Alg::TILE_HOLDS_VALUE) {
            if (tl == ntl - 1) {                              // cell (n-1, m-1): step slast
                const float last = tile[(slast - tl * BD_T) * PITCH + (ddfin >> 1)];
                if (lane == 0) Alg::finish(p, b, last);
            }
        }
        if (T) {
            const BdMover<NC> mv(tl * BD_T, w, wp, lane);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                int off;
                if (mv.cell(k, n, m, w, off)) T[off] = Alg::out(tile[mv.lds(k, PITCH)]);
            }
            sd_wave_lds_sync();
        }
        if (tl + 1 < ntl) {
            stage(tl + 1);
            sd_wave_lds_sync();
        }
    }
    if constexpr (!Alg::TILE_HOLDS_VALUE) {
        if (own) Alg::finish(p, b, fin);
    }
}

}  // namespace aligner
