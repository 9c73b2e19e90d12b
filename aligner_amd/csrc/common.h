// Shared host-side helpers for libaligner_amd.so (error reporting, HIP checks, launch shapes) and the debug options.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>

#include "aligner_amd.h"

namespace aligner {

// thread-local message behind aligner_last_error()
char *error_buffer();
int   fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define ALIGNER_HIP_CHECK(expr)                                                        \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess)                                                          \
            return ::aligner::fail(ALIGNER_EHIP, "%s failed: %s (%s:%d)", #expr,       \
                                   hipGetErrorString(_e), __FILE__, __LINE__);         \
    } while (0)

inline int dtype_size(int dt) {
    switch (dt) {
        case ALIGNER_DT_F32: return 4;
        case ALIGNER_DT_F16: return 2;
        case ALIGNER_DT_BF16: return 2;
        case ALIGNER_DT_F64: return 8;
        case ALIGNER_DT_I32: return 4;
        case ALIGNER_DT_U8: return 1;
        case ALIGNER_DT_I64: return 8;
        default: return 0;
    }
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a driver call: do it once per kernel and size,
// not on every launch (returns hipSuccess when nothing had to be done)
hipError_t ensure_dynamic_lds(const void *kernel, size_t bytes);   // cached per (device, kernel)

// LDS bytes one workgroup may own on the current device (160 KiB on gfx950), cached per device
int device_lds_limit();
int device_cu_count();                // compute units of the current device (cached per device)

// development aid shared by the kernel files (aligner_debug_set_stamps)
extern unsigned long long *g_debug_stamps;
// The debug options (aligner_debug_set_option), one line each: name, default, what it does.  The declarations below,
// the definitions (api.cpp: the only place that evaluates the defaults; env_flag reads the environment once) and the
// lookup by name in aligner_debug_set_option are all generated from this list.
#define ALIGNER_DEBUG_OPTIONS(X) \
    X(softattn_exact, env_flag("ALIGNER_SOFTATTN_EXACT"), "always the exact-product similarity kernel") \
    X(mobo_start_lag, 0, "rows a position segment lets its predecessor get ahead before it starts (default 0)") \
    X(mobo_stamp_wave, 0, "development, the wave whose first lane takes the gradient chain's stamps") \
    X(mobo_full_chain, 0, "testing, the search without log_alpha on the full (sum + max) chain kernel") \
    X(conv_narrow_ft, 0, "testing, frame tiles (8, 4, 2) per workgroup of the narrow conv kernel (0: the plan's choice)") \
    X(conv_no_ring, 0, "A-B / testing, a k = 1 layer with many input chunks stages them all at once (conv_narrow_kernel)") \
    X(maxpath_no_optimistic_mask, 0, "A-B / testing, the strict mask is verified by a pass in front of the search, not by the zero workgroups beside it") \
    X(maxpath_no_mask_verify, 0, "A-B / testing, a strict mask is always multiplied in (no verification pass)") \
    X(maxpath_zero_blocks, 0, "development, zero workgroups of the two-workgroup search launch (0: all idle CUs)") \
    X(maxpath_no_split_walk, 0, "A-B / testing, the two-workgroup search with one walker (the second half) for all rows") \
    X(maxpath_log_launch, 0, "development, every launch of the search and of the expand entry point as one line on stderr: kernel, grid, block, LDS, MaxpathParams (tools/maxpath_launches.py)") \
    X(conv_no_fuse, 0, "testing / A-B, a stack's trailing narrow layers as separate kernels instead of conv_narrow_fused_kernel") \
    X(conv_split_always, env_flag("ALIGNER_CONV_SPLIT_ALWAYS"), "narrow layers never stage fp32 themselves (A/B, tests)") \
    X(softattn_split, 0, "development, waves per strip of the row-group form (2, 4; 1: at most 2; 0: the launch's choice)") \
    X(softattn_strips, env_flag("ALIGNER_SOFTATTN_STRIPS"), "A/B / testing, the one-row-group similarity kernel in its strip-per-wave form (softattn_kernel) instead of the row-tile form") \
    X(softattn_rt_drop_merge, 0, "testing, the row-tile similarity kernel's loader never publishes a strip's normaliser") \
    X(softattn_no_pair, 0, "testing, the similarity kernel's row-group form with one wave per strip only") \
    X(mobo_bwd_general, 0, "testing, the gradient's chain in its general (one exp2 per term) form") \
    X(mobo_lanes, 0, "development, lanes per position in the split form (0: the plan's choice)") \
    X(mobo_drop_segment, -1, "testing, that position segment never publishes (-1: off)") \
    X(gaussnll_rows, 0, "A-B / testing, rows per wave and pass of gauss_nll_kernel (1, 2, 4; never above what LDS allows at the T_text; 0: the launch's choice)") \
    X(gaussnll_grid, 0, "testing, at most this many workgroups per utterance in gauss_nll_kernel's launch, so that a workgroup takes several row groups (0: the launch's choice)") \
    X(gaussup_full_range, 0, "A-B / testing, every frame tile of the Gaussian upsampling kernels takes the full token range [0, t_x) (the path of centres that are out of order)") \
    X(fwdsum_no_grad_stager, 0, "A-B / testing, the gradient-making backward kernel with its compiler-scheduled stager") \
    X(fwdsum_serial, env_flag("ALIGNER_FWDSUM_SERIAL"), "forward then backward sweep, never side by side (A/B, tests)") \
    X(fwdsum_one_wave, env_flag("ALIGNER_FWDSUM_ONE_WAVE"), "A/B / testing, always the one-sweeping-wave forward-sum kernels (the systolic ones never)")
#define ALIGNER_DECLARE_OPTION(name, initial, what) extern int g_opt_##name;
ALIGNER_DEBUG_OPTIONS(ALIGNER_DECLARE_OPTION)
#undef ALIGNER_DECLARE_OPTION

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Launch shape of the kernels in which a workgroup owns whole (utterance, channel) rows of the duration segments
// (hardalign.hip: segment_reduce_kernel, gaussnll.hip: gauss_nll_kernel).
// Workgroups per utterance for `ngroups` row groups: about SEGMENT_GRID_WORKGROUPS in all (256 CUs, eight resident each,
// two rounds), a rule of thumb for streaming kernels, not a tuned value -- no other grid was timed.  Beyond it a
// workgroup takes several row groups and pays the duration scan once for them.  cap > 0: at most that many.
constexpr int SEGMENT_GRID_WORKGROUPS = 4096;
inline int segment_grid_x(int B, int ngroups, int cap = 0) {
    int gx = (SEGMENT_GRID_WORKGROUPS + B - 1) / B;
    gx = gx < ngroups ? gx : ngroups;
    return (cap > 0 && gx > cap) ? cap : gx;
}

// their dynamic LDS: ends[Tx] | wave_tot[waves] | acc[waves][rows][Tx] fp32, `rows` accumulator rows per wave
inline size_t segment_lds_bytes(int Tx, int waves, int rows) {
    return ((size_t)Tx + waves + (size_t)waves * rows * Tx) * sizeof(int);
}

}  // namespace aligner
