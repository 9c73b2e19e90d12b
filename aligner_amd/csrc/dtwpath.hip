// Hard DTW: the minimum-cost warping path between two frame sequences and its backtrack (DESIGN.md 5.11;
// include/aligner_amd.h has the definition).  The hard counterpart of softdtw.hip / banddtw.hip, on their schedules.
//
//     a = R[i-1,j-1]   b = R[i-1,j] + p   c = R[i,j-1] + p        best = a, k = 0; b < best: k = 1; c < best: k = 2
//     R[i,j] = best + cost[i,j]    (+inf: no cell, a +inf or NaN cost, best = +inf)             value = R[n-1,m-1]
//
// Two additions and two strict comparisons per cell in fp32, true infinities, no scaling: the result is a function of
// the costs' bits and the same on every schedule, so the dense and the band kernel agree with each other and with the
// NumPy float32 restatement of tests/dtwpath_oracle.py bit for bit.
//
// Forward: the two kernels of dtw_forward.h -- dense, the skewed pipeline (a lane per row, a wave per 64 rows, the LDS
// ring between waves, costs staged in the skewed order); band storage, the walk along the anti-diagonals (one wave, a
// lane per band column or two, neighbours by DPP) -- with the hard cell DtwHard below.  Instead of R both write the
// decision k of every cell that exists, one byte a cell, through the LDS tile the costs came in by, so the stores stay
// row segments; without a path nothing but the value is written.  The value leaves from the register of the lane that
// owns (n-1, m-1).
//
// Backtrack: one wave per utterance.  It stages the 64 rows that end at the current cell -- their 64 columns that end
// there (dense), or all W band elements (band storage, contiguous in memory) -- into LDS; a path cannot leave such a
// window in fewer than 64 steps.  Lane 0 follows the decisions inside LDS and notes the cells; the wave stores them
// from the back of the utterance's path block and goes on to the next window -- in band storage, where a walk can
// only leave by the window's first row, that window was loaded during the walk.  With the length K known the wave
// moves the K pairs to the front in ascending chunks (a chunk's source lies wholly beyond the chunks already written)
// and fills the tail with -1.  The dependent chain of a step is one LDS read; global loads are one batch per window.
#include "common.h"
#include "device.h"
#include "softdtw_cell.h"
#include "dtw_schedule.h"
#include "dtw_forward.h"

namespace aligner {

constexpr int DP_WIN = 64;                  // rows (and, dense, columns) of a backtrack window
constexpr int DP_STEPS = 512;               // cells noted per window: 64 + 63 + 2 w + 1 <= 382 at w = 127
constexpr int DP_BATCH = 32;                // words a lane has in flight while a band window is staged
static_assert(64 * DP_BATCH * 4 >= DP_WIN * 127 + 3 && 2 * 64 * DP_BATCH * 4 >= DP_WIN * (2 * BD_MAX_W + 1) + 3,
              "a band window fits one batch of words a lane at w <= 63, two beyond");
constexpr int DP_SHIFT = 4;                 // chunks of 64 pairs the move to the front has in flight

// The hard cell for dtw_forward.h: true infinities, costs unchanged; a cell keeps the move it came by (0: diagonal,
// 1: from the row above, 2: from the column before), a byte in the table, and the value alone leaves the kernel
struct DtwHard {
    using Out = unsigned char;
    static constexpr bool TILE_HOLDS_VALUE = false;
    static __device__ __forceinline__ float none() { return __builtin_huge_valf(); }
    static __device__ __forceinline__ float in(const DtwParams &, float d) { return d; }
    static __device__ __forceinline__ float cell(const DtwParams &p, float diag, float up, float left, float d, int &k) {
        const float inf = __builtin_huge_valf();
        const float b = up + p.pen, c = left + p.pen;
        float best = diag;
        k = 0;
        if (b < best) { best = b; k = 1; }
        if (c < best) { best = c; k = 2; }
        return (d < inf && best < inf) ? best + d : inf;      // (d < inf is false for a NaN as well)
    }
    static __device__ __forceinline__ float keep(float, int k) { return __int_as_float(k); }
    static __device__ __forceinline__ unsigned char *table(const DtwParams &p) { return p.dec; }
    static __device__ __forceinline__ unsigned char out(float x) { return (unsigned char)__float_as_int(x); }
    static __device__ __forceinline__ void finish(const DtwParams &p, int b, float fin) { p.value[b] = fin; }
};

// The index maps of the backtrack: where a window's decisions are in memory and in LDS.  A window is aimed at the cell
// it ends at, loaded into registers (every load in flight before the first is waited for: no branch around a load, a
// register a load) and stored to LDS in a second step, so that the next window can be in flight during a walk.
struct DpDenseMap {
    static constexpr bool BAND = false;
    static constexpr int LDS_BYTES = DP_WIN * DP_WIN;
    struct Regs { unsigned k[DP_WIN]; };
    int M, r0, c0;
    __device__ __forceinline__ DpDenseMap(const DtwParams &p) : M(p.M), r0(0), c0(0) {}
    __device__ __forceinline__ size_t block(const DtwParams &p, int b) const { return (size_t)b * p.N * p.M; }
    // the window whose last cell is (i, j): rows i - 63 .. i, columns j - 63 .. j
    __device__ __forceinline__ void aim(const unsigned char *, int i, int j) {
        r0 = i - (DP_WIN - 1);
        c0 = j - (DP_WIN - 1);
    }
    // (a row or column below 0 reads row or column 0 instead; the walk never looks at such an element)
    __device__ __forceinline__ void load(const unsigned char *dec, Regs &v, int lane) const {
        const int col = c0 + lane, colc = col > 0 ? col : 0;
#pragma unroll
        for (int r = 0; r < DP_WIN; ++r) {
            const int row = r0 + r;
            v.k[r] = dec[(row > 0 ? row : 0) * M + colc];
        }
    }
    __device__ __forceinline__ void store(const Regs &v, unsigned char *win, int lane) const {
#pragma unroll
        for (int r = 0; r < DP_WIN; ++r) win[r * DP_WIN + lane] = (unsigned char)v.k[r];
    }
    // where a walk leaves a dense window depends on the path: nothing to load ahead
    __device__ __forceinline__ bool ahead(DpDenseMap &, const unsigned char *) const { return false; }
    __device__ __forceinline__ bool holds(int, int) const { return false; }
    // a cell's place in LDS; a step (di, dj) back moves it by -(di pitch() + dj); left(): that place is outside the window
    __device__ __forceinline__ int at(int i, int j) const { return (i - r0) * DP_WIN + (j - c0); }
    __device__ __forceinline__ int pitch() const { return DP_WIN; }
    __device__ __forceinline__ bool left(int at, int j) const { return at < 0 || j < c0; }
    __device__ __forceinline__ bool valid(int i, int j) const { return i >= 0 && j >= 0; }
};

// NB batches of DP_BATCH words a lane: 1 holds 64 rows of W <= 127 elements, 2 of W <= 255
template <int NB> struct DpBandMap {
    static constexpr bool BAND = true;
    static constexpr int LDS_BYTES = NB * 64 * DP_BATCH * 4;
    struct Regs { unsigned v[NB][DP_BATCH]; };
    int w, W, r0, last, skew;
    __device__ __forceinline__ DpBandMap(const DtwParams &p) : w(p.w), W(2 * p.w + 1), r0(0), last(0), skew(0) {}
    __device__ __forceinline__ size_t block(const DtwParams &p, int b) const { return (size_t)b * p.N * W; }
    // the window whose last row is i: rows max(i - 63, 0) .. i, whole: (i - r0 + 1) W contiguous bytes, moved as the
    // aligned words that hold them (the table's base is word-aligned and its size a multiple of 256); `skew` bytes of
    // the first word lie before the window
    __device__ __forceinline__ void aim(const unsigned char *dec, int i, int) {
        last = i;
        r0 = i - (DP_WIN - 1) > 0 ? i - (DP_WIN - 1) : 0;
        skew = (int)(reinterpret_cast<size_t>(dec + r0 * W) & 3);
    }
    // (a word past the window reads the window's last word, and lands in LDS past it)
    __device__ __forceinline__ void load(const unsigned char *dec, Regs &v, int lane) const {
        const unsigned *src = reinterpret_cast<const unsigned *>(dec + r0 * W - skew);
        const int nwords = ((last - r0 + 1) * W + skew + 3) >> 2;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            if (nb > 0 && 64 * DP_BATCH * nb >= nwords) break;
#pragma unroll
            for (int c = 0; c < DP_BATCH; ++c) {
                const int x = 64 * (DP_BATCH * nb + c) + lane;
                v.v[nb][c] = src[x < nwords ? x : nwords - 1];
            }
        }
    }
    __device__ __forceinline__ void store(const Regs &v, unsigned char *win, int lane) const {
        unsigned *dst = reinterpret_cast<unsigned *>(win);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int c = 0; c < DP_BATCH; ++c) dst[64 * (DP_BATCH * nb + c) + lane] = v.v[nb][c];
    }
    // a walk leaves a band window by its first row, whatever the path: the next window is the 64 rows above
    __device__ __forceinline__ bool ahead(DpBandMap &next, const unsigned char *dec) const {
        if (r0 == 0) return false;
        next.aim(dec, r0 - 1, 0);
        return true;
    }
    __device__ __forceinline__ bool holds(int i, int) const { return i == last; }
    // (a row back is W bytes back and one band element forward)
    __device__ __forceinline__ int at(int i, int j) const { return skew + (i - r0) * W + (j - i + w); }
    __device__ __forceinline__ int pitch() const { return W - 1; }
    __device__ __forceinline__ bool left(int at, int) const { return at < skew; }
    __device__ __forceinline__ bool valid(int i, int j) const { return i >= 0 && j >= 0 && (unsigned)(j - i + w) < (unsigned)W; }
};

template <class Map>
__global__ __launch_bounds__(64) void dtwpath_backtrack_kernel(DtwParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char win[Map::LDS_BYTES];
    __shared__ int note[2 * DP_STEPS];                        // the cells of this window's piece of the path, last first
    const int b = blockIdx.x, lane = threadIdx.x, L = p.L;
    int *path = p.path + (size_t)b * L * 2;
    int n, m;
    bool some;
    if (Map::BAND) some = bd_lengths(p, b, n, m);
    else some = sd_lengths(p, b, n, m);
    some = some && p.value[b] < __builtin_huge_valf();
    if (!some) {
        for (int x = lane; x < 2 * L; x += 64) path[x] = -1;
        if (lane == 0) p.length[b] = 0;
        return;
    }
    Map map(p);
    typename Map::Regs regs;
    const unsigned char *dec = p.dec + map.block(p, b);
    int i = n - 1, j = m - 1, total = 0, done = 0;
    map.aim(dec, i, j);
    map.load(dec, regs, lane);
    // (one wave: its LDS traffic is in program order, sd_wave_lds_sync() is all the synchronisation the loop needs, and
    // it does not wait for the loads in flight)
    while (!done) {
        map.store(regs, win, lane);
        sd_wave_lds_sync();
        Map next(map);
        const bool ahead = map.ahead(next, dec);              // the window after this one, in flight during the walk
        if (ahead) next.load(dec, regs, lane);
        int cnt = 0;
        if (lane == 0) {
            const int room = L - total < DP_STEPS ? L - total : DP_STEPS;       // (n + m - 1 <= L: a path never runs out)
            const int pitch = map.pitch();
            int at = map.at(i, j);
            for (;;) {
                note[2 * cnt] = i;
                note[2 * cnt + 1] = j;
                ++cnt;
                if ((i | j) == 0) { done = 1; break; }
                const int k = __builtin_amdgcn_readfirstlane(win[at]);    // (one lane: the walk stays in scalar registers)
                const int di = k != 2, dj = k != 1;
                i -= di;
                j -= dj;
                at -= (di ? pitch : 0) + dj;
                if (cnt == room) { done = total + cnt == L; break; }
                if (map.left(at, j)) break;                   // the next window ends at (i, j)
            }
            // (Outside the table: a forward kernel's decisions never lead there; the walk ends rather than stage a
            // window around such a cell.  Inside a window `at` only falls, so no read leaves the staged bytes.)
            if (!map.valid(i, j)) done = 1;
        }
        i = __builtin_amdgcn_readlane(i, 0);
        j = __builtin_amdgcn_readlane(j, 0);
        cnt = __builtin_amdgcn_readlane(cnt, 0);
        done = __builtin_amdgcn_readlane(done, 0);
        sd_wave_lds_sync();
        for (int s = lane; s < cnt; s += 64) {
            const int pos = L - 1 - (total + s);
            path[2 * pos] = note[2 * s];
            path[2 * pos + 1] = note[2 * s + 1];
        }
        total += cnt;
        sd_wave_lds_sync();
        if (!done) {
            if (ahead && next.holds(i, j)) {
                map = next;
            } else {                                          // (a full note buffer ended the window early)
                map.aim(dec, i, j);
                map.load(dec, regs, lane);
            }
        }
    }
    __syncthreads();
    // the K = total pairs sit at the back, ascending: to the front, DP_SHIFT chunks at a time (their sources lie beyond
    // every chunk written so far, and a group's loads are complete before its stores: the stores carry their data)
    const int K = total, shift = L - K;
    __threadfence_block();
    if (shift > 0) {
        for (int base = 0; base < K; base += 64 * DP_SHIFT) {
            int vi[DP_SHIFT], vj[DP_SHIFT];
#pragma unroll
            for (int c = 0; c < DP_SHIFT; ++c) {
                const int x = base + 64 * c + lane;
                vi[c] = vj[c] = -1;
                if (x < K) { vi[c] = path[2 * (x + shift)]; vj[c] = path[2 * (x + shift) + 1]; }
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < DP_SHIFT; ++c) {
                const int x = base + 64 * c + lane;
                if (x < K) { path[2 * x] = vi[c]; path[2 * x + 1] = vj[c]; }
            }
            __syncthreads();
        }
        for (int x = 2 * K + lane; x < 2 * L; x += 64) path[x] = -1;
    }
    if (lane == 0) p.length[b] = K;
}

}  // namespace aligner

using namespace aligner;

extern "C" {

size_t aligner_dtw_path_workspace_bytes(int B, int N, int M) {
    if (!sd_shape_ok(B, N, M)) return 0;
    return align_up((size_t)B * N * M, 256);                  // a decision a byte
}

int aligner_dtw_path_f32(const float *cost, const int32_t *n_dev, const int32_t *m_dev, float warp_penalty, int bandwidth,
                         float *value_out, int32_t *path_out, int32_t *length_out, void *workspace, size_t workspace_bytes,
                         int B, int N, int M, void *stream) {
    if (!cost || !value_out) return fail(ALIGNER_EINVAL, "null pointer");
    if ((path_out == nullptr) != (length_out == nullptr)) return fail(ALIGNER_EINVAL, "null pointer: path_out and length_out go together");
    if (path_out && !workspace) return fail(ALIGNER_EINVAL, "null pointer: a path needs the workspace");
    if (B < 1 || N < 1 || M < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (const int rc = dtw_check_penalty(warp_penalty)) return rc;
    if (bandwidth < -1) return fail(ALIGNER_EINVAL, "bandwidth must be -1 (none) or at least 0");
    if (const int rc = dtw_dense_domain(B, N, M)) return rc;
    const size_t need = aligner_dtw_path_workspace_bytes(B, N, M);
    if (path_out && workspace_bytes < need)
        return fail(ALIGNER_ENOSPC, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DtwParams p = {};
    p.cost = cost; p.ns = n_dev; p.ms = m_dev;
    p.pen = warp_penalty;
    p.band = (bandwidth < 0 || bandwidth > SD_NO_BAND) ? SD_NO_BAND : bandwidth;
    p.w = 0;
    p.value = value_out;
    p.dec = path_out ? static_cast<unsigned char *>(workspace) : nullptr;
    p.path = path_out; p.length = length_out;
    p.B = B; p.N = N; p.M = M; p.L = N + M - 1;
    const int NW = (N + 63) / 64;
    ALIGNER_HIP_CHECK(ensure_dynamic_lds(reinterpret_cast<const void *>(dtw_dense_forward_kernel<DtwHard>), sd_lds_bytes(NW, false)));
    hipLaunchKernelGGL(dtw_dense_forward_kernel<DtwHard>, dim3(B), dim3(64 * NW), sd_lds_bytes(NW, false), s, p);
    ALIGNER_HIP_CHECK(hipGetLastError());
    if (path_out) {
        hipLaunchKernelGGL(dtwpath_backtrack_kernel<DpDenseMap>, dim3(B), dim3(64), 0, s, p);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

size_t aligner_dtw_path_banded_workspace_bytes(int B, int N, int bandwidth) {
    if (!bd_shape_ok(B, N, bandwidth)) return 0;
    return align_up((size_t)B * N * (2 * bandwidth + 1), 256);
}

int aligner_dtw_path_banded_f32(const float *cost_band, const int32_t *n_dev, const int32_t *m_dev, float warp_penalty,
                                int bandwidth, float *value_out, int32_t *path_out, int32_t *length_out, void *workspace,
                                size_t workspace_bytes, int B, int N, void *stream) {
    if (!cost_band || !value_out) return fail(ALIGNER_EINVAL, "null pointer");
    if ((path_out == nullptr) != (length_out == nullptr)) return fail(ALIGNER_EINVAL, "null pointer: path_out and length_out go together");
    if (path_out && !workspace) return fail(ALIGNER_EINVAL, "null pointer: a path needs the workspace");
    if (reinterpret_cast<size_t>(workspace) & 3) return fail(ALIGNER_EINVAL, "the workspace must be 4-byte aligned");
    if (B < 1 || N < 1) return fail(ALIGNER_EINVAL, "bad shape");
    if (const int rc = dtw_check_penalty(warp_penalty)) return rc;
    if (bandwidth < 0) return fail(ALIGNER_EINVAL, "bandwidth must be at least 0");
    if (const int rc = dtw_band_domain(B, N, bandwidth, "the dense call takes any band")) return rc;
    const size_t need = aligner_dtw_path_banded_workspace_bytes(B, N, bandwidth);
    if (path_out && workspace_bytes < need)
        return fail(ALIGNER_ENOSPC, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DtwParams p = {};
    p.cost = cost_band; p.ns = n_dev; p.ms = m_dev;
    p.pen = warp_penalty;
    p.band = bandwidth; p.w = bandwidth;
    p.value = value_out;
    p.dec = path_out ? static_cast<unsigned char *>(workspace) : nullptr;
    p.path = path_out; p.length = length_out;
    p.B = B; p.N = N; p.M = N + bandwidth; p.L = 2 * N + bandwidth - 1;
    if (bandwidth <= 63) hipLaunchKernelGGL((dtw_band_forward_kernel<DtwHard, 64>), dim3(B), dim3(64), 0, s, p);
    else hipLaunchKernelGGL((dtw_band_forward_kernel<DtwHard, 128>), dim3(B), dim3(64), 0, s, p);
    ALIGNER_HIP_CHECK(hipGetLastError());
    if (path_out) {
        if (bandwidth <= 63) hipLaunchKernelGGL(dtwpath_backtrack_kernel<DpBandMap<1>>, dim3(B), dim3(64), 0, s, p);
        else hipLaunchKernelGGL(dtwpath_backtrack_kernel<DpBandMap<2>>, dim3(B), dim3(64), 0, s, p);
        ALIGNER_HIP_CHECK(hipGetLastError());
    }
    return ALIGNER_OK;
}

}  // extern "C"
