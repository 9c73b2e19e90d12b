// Device code for the kernels that work on the segments the durations cut out of the mel axis (prior.hip:
// regulate_kernel, hardalign.hip: segment_reduce_kernel and the binarization kernels, gaussnll.hip: gauss_nll_kernel):
// the durations' prefix sums and the owner lookup on them, the clamp of t_y, and the segmented reduction of a wave's run
// of frames into per-token accumulators in LDS.  That reduction uses no atomics and has one summation order -- the same
// bits on every run -- and exists here once: a change to it reaches every kernel that reduces over segments.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "device.h"

namespace aligner {

constexpr int DUR_SCAN_THREADS = 256;

// ends[x] = sum(max(dur[b,i],0), i <= x) for one utterance, by the whole workgroup (256 threads): a thread sums
// `per` consecutive tokens, the wave scans its 64 partial sums in registers, four wave totals go through LDS.
__device__ inline void scan_durations(const int *__restrict__ dur_b, int *ends, int *wave_tot, int Tx) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (Tx + DUR_SCAN_THREADS - 1) / DUR_SCAN_THREADS;
    const int x0 = tid * per;
    int s = 0;
    for (int i = 0; i < per; ++i) {
        const int x = x0 + i;
        int d = (x < Tx) ? dur_b[x] : 0;
        d = d < 0 ? 0 : d;
        s += d;
        if (x < Tx) ends[x] = s;                             // local inclusive sum for now
    }
    int incl = s;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int base = incl - s;
    for (int w = 0; w < wave; ++w) base += wave_tot[w];
    for (int i = 0; i < per; ++i)
        if (x0 + i < Tx) ends[x0 + i] += base;
    __syncthreads();
}

// first x in [lo, Tx) with ends[x] > y; Tx when there is none (a frame past the durations' sum)
__device__ inline int owner_of(const int *ends, int lo, int Tx, int y) {
    int hi = Tx;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ends[mid] > y) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Keys of the lane's VEC frames y0 .. y0+VEC-1.  The key of a frame is its token, Tx for a frame that does not count
// (no token owns it: past the durations' sum, or at or past `limit`): keys never decrease along a row, so "same key as
// the lane o below" is all a segmented scan needs.  The first and the last frame are looked up, the two between only
// where those differ.  (Scalar locals, and every k[j] stored once at a constant index: conditional stores into the
// array are merged into one store with a variable index when this is optimised on its own, before it is inlined, and
// the array then lives in scratch.)
template <int VEC>
__device__ __forceinline__ void seg_keys(const int *ends, int Tx, int limit, int y0, int (&k)[VEC]) {
    const int k0 = (y0 < limit) ? owner_of(ends, 0, Tx, y0) : Tx;
    if constexpr (VEC == 4) {
        const int k3 = (y0 + 3 < limit) ? owner_of(ends, k0, Tx, y0 + 3) : Tx;
        int k1, k2;
        if (k3 == k0) {
            k1 = k2 = k0;
        } else {
            k1 = (y0 + 1 < limit) ? owner_of(ends, k0, Tx, y0 + 1) : Tx;
            k2 = (y0 + 2 < limit) ? owner_of(ends, k1, Tx, y0 + 2) : Tx;
        }
        k[1] = k1;
        k[2] = k2;
        k[3] = k3;
    }
    k[0] = k0;
}

// How the lanes' last runs join in the segmented scan.  Keys are per run of frames, not per row: this is made once and
// used for every row a wave carries.
struct SegJoin {
    unsigned mask;                                           // bit i: the lane 2^i below ends in the same key
    bool has_head;                                           // a run that ends inside this lane's frames
    bool head_joins;                                         // ... and continues the last run of the lane below
    bool tail_ends;                                          // no lane above continues this lane's last run
};

template <int VEC>
__device__ __forceinline__ SegJoin seg_join(const int (&k)[VEC], int lane) {
    const int kt = k[VEC - 1];                               // key of the lane's last run
    SegJoin j;
    j.mask = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int pk = __shfl_up(kt, 1 << i);
        if (lane >= (1 << i) && pk == kt) j.mask |= 1u << i;
    }
    const int k_prev = __shfl_up(kt, 1);                     // (lane 0: its own, masked below)
    const int k_next = __shfl_down(k[0], 1);
    j.tail_ends = (lane == 63) || (k_next != kt);
    j.has_head = (k[0] != kt);
    j.head_joins = j.has_head && lane > 0 && k_prev == k[0];
    return j;
}

// One row's share of a run: the lane's VEC values of each of NQ quantities go into the row's per-token accumulators in
// LDS, acc[q * qstride + token].  The lane's own frames in order: its head run | the runs wholly inside the lane
// (flushed at once: a run between two others, nobody else holds its key) | its last run, which a segmented inclusive
// scan joins with the lanes below.  Then the head add, then the tail add: the lanes that add hold distinct tokens, so
// each is a plain read-add-write, and the wave barriers keep the three in program order.
// Q... = 0 .. NQ-1: every step is written as a fold over the quantities, not as a loop.  A loop's head[q] / run[q] stay
// in memory until the loop is unrolled, which is after the passes that turn the short branches below into selects; the
// kernels then come out with more branches and up to three more VGPRs, one of them across an occupancy step.
template <int VEC, int NQ, int... Q>
__device__ __forceinline__ void seg_accumulate_q(const float (&v)[NQ][VEC], const int (&k)[VEC], int Tx, float *acc,
                                                 int qstride, const SegJoin &join, std::integer_sequence<int, Q...>) {
    const int kh = k[0], kt = k[VEC - 1];
    float head[NQ], run[NQ];
    ((head[Q] = 0.f), ...);
    ((run[Q] = v[Q][0]), ...);
    if constexpr (VEC == 4) {
        int rk = kh;
        bool head_done = false;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            if (k[j] == rk) {
                ((run[Q] += v[Q][j]), ...);
            } else {
                if (!head_done) {
                    ((head[Q] = run[Q]), ...);
                    head_done = true;
                } else if (rk < Tx) {
                    ((acc[Q * qstride + rk] += run[Q]), ...);
                }
                rk = k[j];
                ((run[Q] = v[Q][j]), ...);
            }
        }
    }
    float s[NQ], below[NQ];                                  // segmented inclusive scan of the last runs over the lanes
    ((s[Q] = run[Q]), ...);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float p[NQ];
        ((p[Q] = __shfl_up(s[Q], 1 << i)), ...);
        if (join.mask & (1u << i)) ((s[Q] += p[Q]), ...);
    }
    ((below[Q] = __shfl_up(s[Q], 1)), ...);
    __builtin_amdgcn_wave_barrier();
    if (join.has_head && kh < Tx) ((acc[Q * qstride + kh] += join.head_joins ? below[Q] + head[Q] : head[Q]), ...);
    __builtin_amdgcn_wave_barrier();
    if (join.tail_ends && kt < Tx) ((acc[Q * qstride + kt] += s[Q]), ...);
    __builtin_amdgcn_wave_barrier();
}

template <int VEC, int NQ>
__device__ __forceinline__ void seg_accumulate(const float (&v)[NQ][VEC], const int (&k)[VEC], int Tx, float *acc,
                                               int qstride, const SegJoin &join) {
    seg_accumulate_q<VEC, NQ>(v, k, Tx, acc, qstride, join, std::make_integer_sequence<int, NQ>{});
}

}  // namespace aligner
