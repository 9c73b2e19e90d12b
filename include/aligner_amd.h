/*
 * aligner_amd.h -- C ABI of libaligner_amd.so (MI355X / gfx950).
 *
 * Drop-in boundary for the TTS alignment hot path of xiaozhah/Aligner:
 *   monotonic_align.maximum_path(value, mask)      reference __init__.py:6-21
 *   monotonic_align.core.maximum_path_c(...)       reference core.pyx:38-45
 *   (per-utterance DP maximum_path_each)           reference core.pyx:7-35
 * plus the soft-attention front end that produces `value` (build-defined spec,
 * SURVEY.md 7.4; the reference snapshot only links the paper, README.md:50).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in any signature.
 *     `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - every *_dev pointer is device memory on the current HIP device; tensors
 *     are C-contiguous, [B, Tx, Ty] with the mel axis (Ty) contiguous, exactly
 *     the layout the reference's memoryviews demand (core.pyx:9,40).
 *   - all device entry points are asynchronous on `stream`, never allocate,
 *     never synchronise, and are hipGraph-capturable.
 *   - return 0 on success or a negative ALIGNER_E* code; aligner_last_error()
 *     returns a thread-local message for the last failure on this thread.
 *   - the library contains NO CPU implementation of the path: without a GPU the
 *     device entry points fail with ALIGNER_EHIP.
 */
#ifndef ALIGNER_AMD_H
#define ALIGNER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: aligner_maxpath_workspace_bytes grew (per-utterance mask verdicts), aligner_fused_align_f32 left the library,
 *    the prepared-weights image of round 4 (old image + the GEMM form's) and the forward-sum / search workspaces of round 4
 *    are what the *_bytes functions of THIS version return: size every buffer with them, never with constants;
 *    new entry points aligner_softattn_ld / aligner_maxpath_ld (a row pitch for the pipeline's own intermediate) and the
 *    test flag ALIGNER_F_TEST_IMPATIENT_FIRST_HALF.
 * 5: the convolution on raw (unprepared) weights left the library: prepare the weights once.
 *    Added within 5 (additive, nothing existing changed): the backward of the front end --
 *    aligner_softattn_backward_f32 / aligner_softattn_backward_workspace_bytes, aligner_conv1d_prepare_transposed_f32,
 *    aligner_conv1d_backward_weight_f32 / aligner_conv1d_backward_workspace_bytes; and the hard half of the training
 *    objective -- aligner_segment_reduce_f32, aligner_bin_loss, aligner_bin_loss_grad_f32; and the hard search with
 *    optional pauses between tokens -- aligner_pausepath / aligner_pausepath_workspace_bytes; and the Glow-TTS / VITS
 *    log-likelihood front end -- aligner_gauss_logp / aligner_gauss_logp_workspace_bytes, its gradient
 *    aligner_gauss_logp_backward_f32 / aligner_gauss_logp_backward_workspace_bytes; and their likelihood loss on
 *    the hard path -- aligner_gauss_nll_f32 / aligner_gauss_nll_workspace_bytes; and Gaussian upsampling with its
 *    gradient -- aligner_gauss_upsample_f32 / aligner_gauss_upsample_backward_f32 and their *_workspace_bytes; and
 *    Soft-DTW with its expected alignment matrix -- aligner_soft_dtw_f32 / aligner_soft_dtw_workspace_bytes; and its
 *    banded L1 cost table with the gradient -- aligner_l1_cost_f32 / aligner_l1_cost_backward_f32; the three in band
 *    storage, O(N w) memory and any N -- aligner_soft_dtw_banded_f32 / aligner_l1_cost_banded_f32 /
 *    aligner_l1_cost_banded_backward_f32; and hard DTW, the minimum-cost warping path with its backtrack, in both
 *    storage forms -- aligner_dtw_path_f32 / aligner_dtw_path_banded_f32 and their *_workspace_bytes; and the
 *    Euclidean cost tables, squared (with the gradient) and root, in both storage forms -- aligner_l2_cost_f32 /
 *    aligner_l2_cost_backward_f32 / aligner_l2_cost_banded_f32 / aligner_l2_cost_banded_backward_f32; and the cost
 *    kinds along a path, forward and backward -- aligner_path_runs / aligner_path_cost_f32 /
 *    aligner_path_cost_backward_f32 / aligner_path_cost_backward_workspace_bytes. */
#define ALIGNER_ABI_VERSION 5

/* error codes */
#define ALIGNER_OK       0
#define ALIGNER_EINVAL (-22) /* null pointer / bad shape / bad dtype / bad flag */
#define ALIGNER_EDOM   (-33) /* shape outside what the kernels support          */
#define ALIGNER_ENOSPC (-28) /* workspace too small                             */
#define ALIGNER_EHIP    (-5) /* HIP runtime failure (message has the detail)    */

/* element types for mask / path buffers */
#define ALIGNER_DT_F32  0
#define ALIGNER_DT_F16  1
#define ALIGNER_DT_BF16 2
#define ALIGNER_DT_F64  3
#define ALIGNER_DT_I32  4
#define ALIGNER_DT_U8   5   /* also torch.bool */
#define ALIGNER_DT_I64  6

/* flags for aligner_maxpath_* */
#define ALIGNER_F_STRICT_MASK   1  /* multiply value by mask element-wise first
                                      (__init__.py:11) instead of using the mask
                                      for lengths only.  The result is that of
                                      the multiply, bit for bit; the multiply
                                      itself happens only for the utterances whose
                                      mask is not ONE on every score the search
                                      reads (the rectangle [0,t_x) x [0,t_y)):
                                      that is checked on the device, per
                                      utterance -- by the workgroups that write
                                      the dense path beside an optimistic search
                                      (a second launch redoes the others), or by
                                      a pass over the mask in front of it.      */
#define ALIGNER_F_COMPAT_TXGTTY 2  /* t_x > t_y: reproduce the reference's
                                      result -- its forward band is empty, so
                                      its backtrack (core.pyx:32-35) walks up
                                      from row t_x-1 on the RAW scores --
                                      instead of an all-zero path and
                                      ALIGNER_ST_BAD_LENGTHS                   */
#define ALIGNER_F_FORCE_GENERIC 4  /* use the generic (barrier-per-frame) kernel */

#define ALIGNER_F_NO_PREV_TABLE 16 /* testing: do not keep the backtrack's second LDS table (the walk then
                                      takes the flag-and-retry steps it uses for long utterances)   */
#define ALIGNER_F_STREAM_PATH  128 /* the dense path is written with non-temporal stores: a large output that
                                      nothing on the GPU reads back soon then does not displace the score
                                      tensors of other batches in flight from the caches (three batches in
                                      flight: 39.9 -> 33.8 us per step at [64,200,1000]; one batch alone is
                                      2 us slower).  The caller's choice; off by default                */
#define ALIGNER_F_ONE_CU       256 /* never split an utterance over two workgroups.  By default text of 253..504
                                      rows over 1792 or more mel frames, in a batch of at most an eighth of the
                                      CU count (B <= 32 on MI355X), runs as two workgroups per utterance, each on its
                                      own CU: same results, the sweep bound by two CUs' vector units instead of
                                      one's (long-form [8,500,4000]: 134 -> 106 us).  The boundary row between the
                                      halves travels through the workspace, which is why the call then starts
                                      with a small fill kernel on the same stream.  Only taken when all 2B workgroups
                                      fit the chip at once; the second half's waits are bounded, and if the first half
                                      did not deliver in time (other work kept it off the GPU for ~0.3 s) the
                                      utterance comes back with an all-zero path, zero durations and
                                      ALIGNER_ST_INTERNAL in the status word -- check it (aligner_maxpath_read_status;
                                      aligner_maxpath_host_f32 does and fails with ALIGNER_EHIP) */
#define ALIGNER_F_TWO_CUS      512 /* take the two-workgroup form whenever the text has 253..504 rows, whatever
                                      the batch size and mel length (testing; a short sweep loses by it) */
#define ALIGNER_F_PATH_PREZEROED 2048 /* aligner_maxpath*: path_out_dev already holds zeros (aligner_maxpath_zero_path, on another
                                      stream or graph branch, BEFORE this call starts): the search kernel writes the
                                      path's ones itself -- core.pyx:33 on the np.zeros of __init__.py:15 -- and no
                                      expand kernel follows.  The dense path costs the step's serial chain nothing
                                      (bench.py, one batch at a time: 65.9 -> see DESIGN 5).  A path that is NOT all
                                      zero keeps its stale ones: the caller's contract                        */
#define ALIGNER_F_SEPARATE_EXPAND 4096 /* aligner_maxpath*: always write the dense path with the expand kernel behind the search.
                                      By default, where the batch leaves at least 32 CUs idle and the one-workgroup-
                                      per-utterance kernel runs, the search launch carries extra workgroups that write
                                      the path's zeros on those CUs while the others search, and every utterance's
                                      workgroup writes its ones at the end: one launch, nothing of the 4*B*Tx*Ty-byte
                                      write left on the serial chain (same bits; A/B switch for measurements)  */
#define ALIGNER_F_TEST_DROP_FIRST_HALF 1024 /* testing: in the two-workgroup form the first half of every utterance leaves
                                      without delivering, so the second gives up after its bounded wait: all-zero
                                      path, zero durations, ALIGNER_ST_INTERNAL -- the defined failure of that form */
#define ALIGNER_F_TEST_IMPATIENT_FIRST_HALF 16384 /* testing: in the two-workgroup form the first half gives up waiting for the
                                      backtrack's hand-over at once (as it would after its bounded wait on a contended
                                      chip): ALIGNER_ST_INTERNAL is set, and the second half, finding that, walks
                                      every row itself -- the answer is late, not lost */
#define ALIGNER_F_TEST_DROP_ZERO_REPORTS 8192 /* testing: the zero workgroups of the one-launch dense path (above) write their
                                      zeros but never report, so every utterance's workgroup gives up after a (here
                                      shortened) bounded wait -- the defined failure of that form: no 1 in the path
                                      (all zeros), zero durations, no token on any frame, ALIGNER_ST_INTERNAL */
#define ALIGNER_F_WRITE_Q       64 /* also overwrite the fp32 score block with the running scores Q inside
                                      the band, in place, exactly as the reference does (core.pyx:18,30:
                                      `value[x, y] = max(v_cur, v_prev) + value[x, y]`).  Takes the
                                      barrier-per-frame kernel (the fast one never materialises Q); the
                                      score pointer must be writable                                 */

/* bits of the device status word (aligner_maxpath_read_status) */
#define ALIGNER_ST_BAD_LENGTHS  1  /* some utterance had t_x < 1 or t_x > t_y
                                      (undefined behaviour in the reference,
                                      core.pyx:15,33-34); its path is all zero */
#define ALIGNER_ST_CLAMPED      2  /* some t_x > Tx or t_y > Ty was clamped     */
#define ALIGNER_ST_INTERNAL     4  /* internal consistency check failed         */

int         aligner_abi_version(void);
const char *aligner_last_error(void);

/* Number of visible HIP devices (0 when there is no GPU); never fails. */
int         aligner_device_count(void);

/* ---- monotonic alignment search ---------------------------------------- */

/* Bytes of device workspace aligner_maxpath_f32 needs for this shape. */
size_t aligner_maxpath_workspace_bytes(int B, int Tx, int Ty);

/* Replaces __init__.py:18-19: t_x[b] = sum_x mask[b,x,0], t_y[b] = sum_y mask[b,0,y]
 * (float sum truncated to int32, like ndarray.astype(np.int32)). */
int aligner_lengths_from_mask(const void *mask_dev, int mask_dtype,
                              int B, int Tx, int Ty,
                              int32_t *t_xs_dev, int32_t *t_ys_dev, void *stream);

/*
 * Replaces maximum_path_c (core.pyx:40-45) + the wrapper's marshalling
 * (__init__.py:11-21) with everything resident in HBM.
 *
 *   value_dev   [B,Tx,Ty] fp32, NOT modified (the reference mutates its private
 *               host copy; the caller's tensor is untouched there too).
 *   mask_dev    optional [B,Tx,Ty] of mask_dtype (F32, BF16, F16, U8 or I32).  Used (a) to derive
 *               lengths when t_xs_dev/t_ys_dev are NULL and (b) for the
 *               element-wise multiply when ALIGNER_F_STRICT_MASK is set.
 *   t_xs_dev,t_ys_dev  optional [B] int32 lengths; when NULL they are derived
 *               from mask_dev into the workspace.
 *   path_out_dev optional [B,Tx,Ty] of path_dtype (F32,F16,BF16,F64,I32,U8,I64),
 *               fully written (zeros and ones): the reference's return value.
 *   tok_out_dev optional [B,Ty] int32: text-token index per mel frame, -1 for
 *               frames >= t_y.
 *   dur_out_dev optional [B,Tx] int32: frames per token (= path.sum(2)).
 *   max_neg_val core.pyx:40 (default -1e9 in the reference).
 */
/* The same for scores of `value_dtype` F32, BF16 or F16: 16-bit scores are up-cast to fp32 (exactly) inside the
 * kernels' loaders -- no conversion pass, half the read traffic -- and the DP runs in fp32 like the reference
 * (__init__.py:14).  With ALIGNER_F_STRICT_MASK the mask must have the scores' dtype: the product is rounded in
 * that dtype, as torch's `value * mask` (__init__.py:11) is.  16-byte aligned pointers and Ty % 8 == 0 take the
 * fast kernels, anything else the generic one. */
int aligner_maxpath(const void *value_dev, int value_dtype,
                    const void *mask_dev, int mask_dtype,
                    const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                    void *path_out_dev, int path_dtype,
                    int32_t *tok_out_dev, int32_t *dur_out_dev,
                    void *workspace_dev, size_t workspace_bytes,
                    int B, int Tx, int Ty,
                    float max_neg_val, int flags, void *stream);
/* aligner_maxpath for scores with a ROW PITCH of their own: element [b,x,y] at ((b*Tx + x)*ld_value + y), ld_value >= Ty --
 * what aligner_softattn_ld writes (rows that start on whole 128-byte lines).  Lengths are given, there is no
 * mask (ALIGNER_F_STRICT_MASK, ALIGNER_F_WRITE_Q: ALIGNER_EINVAL); path / tok / dur are the contiguous outputs of
 * aligner_maxpath.  The columns Ty .. ld_value-1 are never read into a result. */
int aligner_maxpath_ld(const void *value_dev, int value_dtype, int ld_value,
                       const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                       void *path_out_dev, int path_dtype, int32_t *tok_out_dev, int32_t *dur_out_dev,
                       void *workspace_dev, size_t workspace_bytes, int B, int Tx, int Ty,
                       float max_neg_val, int flags, void *stream);
int aligner_maxpath_forward(const void *value_dev, int value_dtype,
                            const void *mask_dev, int mask_dtype,
                            const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                            int32_t *tok_out_dev, int32_t *dur_out_dev,
                            void *workspace_dev, size_t workspace_bytes,
                            int B, int Tx, int Ty,
                            float max_neg_val, int flags, void *stream);

/* fp32 scores (value_dtype = ALIGNER_DT_F32). */
int aligner_maxpath_f32(const float *value_dev,
                        const void *mask_dev, int mask_dtype,
                        const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                        void *path_out_dev, int path_dtype,
                        int32_t *tok_out_dev, int32_t *dur_out_dev,
                        void *workspace_dev, size_t workspace_bytes,
                        int B, int Tx, int Ty,
                        float max_neg_val, int flags, void *stream);

/* The two stages of aligner_maxpath_f32 as separate launches (profiling and
 * callers that only want durations): forward sweep + backtrack -> token starts in
 * the workspace (+ optional tok/dur), and workspace -> dense 0/1 path. */
int aligner_maxpath_forward_f32(const float *value_dev,
                                const void *mask_dev, int mask_dtype,
                                const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                                int32_t *tok_out_dev, int32_t *dur_out_dev,
                                void *workspace_dev, size_t workspace_bytes,
                                int B, int Tx, int Ty,
                                float max_neg_val, int flags, void *stream);
int aligner_maxpath_expand(const void *workspace_dev, void *path_out_dev, int path_dtype,
                           int B, int Tx, int Ty, void *stream);
int aligner_maxpath_expand_ex(const void *workspace_dev, void *path_out_dev, int path_dtype,
                           int B, int Tx, int Ty, int flags /* ALIGNER_F_STREAM_PATH */, void *stream);

/* The dense path in the reference's own two steps -- zeros (__init__.py:15), then one 1 per frame (core.pyx:33) -- for
 * callers with a second stream or a graph branch: aligner_maxpath_zero_path does not depend on the search and can
 * run BESIDE aligner_maxpath_forward*; aligner_maxpath_scatter_path (after both) then writes t_y elements per
 * utterance instead of the whole tensor.  Together they equal aligner_maxpath_expand, bit for bit, for every path
 * dtype; flags: ALIGNER_F_STREAM_PATH (non-temporal zeros).  bench.py's one-batch-at-a-time step is built this way. */
int aligner_maxpath_zero_path(void *path_out_dev, int path_dtype, int B, int Tx, int Ty, int flags, void *stream);
int aligner_maxpath_scatter_path(const void *workspace_dev, void *path_out_dev, int path_dtype,
                                 int B, int Tx, int Ty, void *stream);

/* Blocking read-and-clear of the workspace's status word (ALIGNER_ST_* bits).  The
 * word is sticky: kernels only OR bits into it, so the first 256 bytes of a fresh
 * workspace must be zero (hipMemset once at allocation; no per-call memset). */
int aligner_maxpath_read_status(void *workspace_dev, int32_t *status_host, void *stream);

/* Development aid: install (or clear with NULL) a device buffer of B*16*8 uint64 that
 * the forward kernels fill with shader-clock stamps per wave (see maxpath.hip). */
void aligner_debug_set_stamps(void *stamps_dev);

/* Development switches, process-wide (0/1; defaults from the environment variables ALIGNER_FWDSUM_ONE_WAVE /
 * ALIGNER_SOFTATTN_EXACT, read once at load): "fwdsum_one_wave" forces the one-sweeping-wave forward-sum
 * kernels, "softattn_exact" the exact-product similarity kernel; "mobo_drop_segment" (a segment index, -1 = off)
 * makes that position segment of every utterance withhold its rows from the next one, which then gives up after a
 * short wait: the test of the boundary search's defined failure; "mobo_start_lag" (rows a position segment lets the
 * one before it get ahead before it starts, default 0) and "mobo_lanes" (lanes per position of the split form: 1, 2, 4; 0 = the plan's
 * choice) are the boundary search's measurement knobs (tools/mobo_time.py).  ALIGNER_EINVAL for an unknown name. */
int aligner_debug_set_option(const char *name, int value);

/*
 * Host-buffer form with exactly maximum_path_c's contract (core.pyx:40):
 * paths[B,Tx,Ty] int32 receives the path (fully overwritten), values[B,Tx,Ty]
 * fp32 holds the scores; with ALIGNER_F_WRITE_Q in `flags` it comes back as the
 * running score Q inside every utterance's band, bit for bit what the reference
 * leaves there (without the flag it is only read), t_xs/t_ys[B] int32.  Stages
 * through device memory it allocates and frees; blocking.  Returns ALIGNER_EDOM
 * if any t_x < 1 or t_x > t_y.
 */
int aligner_maxpath_host_f32(int32_t *paths, float *values,
                             const int32_t *t_xs, const int32_t *t_ys,
                             int B, int Tx, int Ty, float max_neg_val, int flags);

/* ---- soft-attention front end (build-defined spec) ------- */

#define ALIGNER_SIM_L2   0  /* logit = -temperature * sum_c (q - k)^2 */
#define ALIGNER_SIM_DOT  1  /* logit = temperature * sum_c q*k        */

/*
 * logp[b,i,j] = log_softmax_i( logit[b,i,j] ) (+ log(prior[b,i,j] + 1e-8))
 *   keys_dev    [B,C,Tx] fp32  encoded text  (channel-major, as Conv1d emits)
 *   queries_dev [B,C,Ty] fp32  encoded mel
 *   t_xs_dev    optional [B] int32 (clamped to [0, Tx]): text rows >= t_x are excluded from the
 *               softmax and written as -inf (0 in soft_out_dev); NULL = all Tx rows valid.
 *   prior_dev   optional [B,Tx,Ty] fp32
 *   logp_out_dev [B,Tx,Ty] fp32; soft_out_dev optional [B,Tx,Ty] fp32 = softmax_i(logp)
 *   workspace_dev  aligner_softattn_workspace_bytes(B,C,Tx) bytes: the text operand split
 *               to bf16 halves in MFMA fragment order, prepared once per call.
 * Arithmetic: the contraction runs on the bf16 matrix cores with every fp32 operand split in two bf16 halves
 * (hi*hi + hi*lo + lo*hi, fp32 accumulate).  What that delivers, against the formula evaluated exactly on the fp32 inputs:
 *     |logp[b,i,j] - exact| <= 2^-16 Scol[b,j] + 2^-23 |logp| + 6.5e-6      (C >= 80; 3 * 2^-15 Scol below)
 *   Scol[b,j] = max over the rows i < t_x of S[b,i,j], the magnitude of what the logit adds up:
 *     L2 : S = T (2 sum_c |k_ci| |q_cj| + sum_c k_ci^2 + sum_c q_cj^2)        dot: S = T sum_c |k_ci| |q_cj|
 *   (an error in any row's logit moves the column's log-sum); 6.5e-6 is the log-sum-exp in fp32, whatever the logits.
 * The absolute consequence, per similarity, at the sharpest temperature these kernels are given:
 *   L2,  temperature <= 0.002: |logp - exact| < 1e-4 on encodings of a few units per channel (the error is multiplied
 *        by 2T <= 0.004; C = 256 at 3 units per channel: about 1e-5);
 *   dot, temperature <= 0.2:   |logp - exact| < 1e-4 on encodings of about ONE unit per channel only (the error is
 *        multiplied by T: at 3 units per channel, or a common offset of 3, the three products alone are 7e-4 to 8e-4
 *        off at T = 0.2 and 4e-4 at T = 0.11, C = 80 to 256); the bound above is what holds there.
 * Sharper temperatures (L2 > 0.002, dot > 0.2) take an exact-product kernel (fp32 MFMA, about a quarter of the matrix
 * rate) automatically: the same bound with 2^-16 replaced by 4 * 2^-24 e(C), e(C) = 9.5 at C = 80, 16 at C = 256 (an fp32
 * sum over C channels).  tests/test_softattn_host.py derives every figure, tests/test_softattn_inputs_gpu.py holds the
 * kernels to them.
 * An utterance with t_x <= 0 (no valid row): logp is -inf and soft is 0 throughout, never NaN.
 */
size_t aligner_softattn_workspace_bytes(int B, int C, int Tx);
/* logp_out_dev of logp_dtype F32 or BF16 (round to nearest even; the layout aligner_maxpath reads directly:
 * BASELINE config 5, "bf16 similarity + int32 path"); everything else as aligner_softattn_f32. */
int aligner_softattn(const float *keys_dev, const float *queries_dev,
                     const int32_t *t_xs_dev, const float *prior_dev,
                     void *logp_out_dev, int logp_dtype, float *soft_out_dev,
                     void *workspace_dev, size_t workspace_bytes,
                     int B, int C, int Tx, int Ty,
                     float temperature, int sim, void *stream);
int aligner_softattn_f32(const float *keys_dev, const float *queries_dev,
                         const int32_t *t_xs_dev, const float *prior_dev,
                         float *logp_out_dev, float *soft_out_dev,
                         void *workspace_dev, size_t workspace_bytes,
                         int B, int C, int Tx, int Ty,
                         float temperature, int sim, void *stream);
/* aligner_softattn with a ROW PITCH for logp_out_dev: element [b,i,j] at ((b*Tx + i)*ld_logp + j), ld_logp >= Ty, rows on
 * 16-byte boundaries.  For the pipeline's own intermediate (similarity -> alignment search: aligner_maxpath_ld reads it):
 * with ld_logp a multiple of 32 (fp32) every 32-frame run a wave stores is one whole 128-byte line -- rows of 4000 bytes
 * (T_mel = 1000) cut three quarters of those runs in two.  Only the columns < Ty are written.  The row-tile
 * form only (Tx <= 224, C = 80 or 128, Ty % 4 == 0, no prior, no soft output): ALIGNER_EDOM otherwise. */
int aligner_softattn_ld(const float *keys_dev, const float *queries_dev,
                        const int32_t *t_xs_dev, const float *prior_dev,
                        void *logp_out_dev, int logp_dtype, int ld_logp, float *soft_out_dev,
                        void *workspace_dev, size_t workspace_bytes,
                        int B, int C, int Tx, int Ty,
                        float temperature, int sim, void *stream);

/*
 * Backward of aligner_softattn_f32.  Given grad_logp_dev = dL/dlogp and (optional) grad_soft_dev = dL/dsoft, [B,Tx,Ty]
 * fp32, contiguous, and the forward's own keys / queries / t_xs / prior / temperature / sim:
 *   G      = G_l + soft (G_s - sum_i soft G_s)     (sums over the valid rows i < t_x)
 *   dlogit = G - softmax_i(logit) sum_i G          (0 on rows i >= t_x)
 *   L2 : dK[c,i] = 2T (sum_j dlogit q[c,j] - k[c,i] sum_j dlogit)   dQ[c,j] = 2T (sum_i dlogit k[c,i] - q[c,j] sum_i dlogit)
 *   dot: dK[c,i] =  T  sum_j dlogit q[c,j]                          dQ[c,j] =  T  sum_i dlogit k[c,i]
 * grad_keys_out_dev [B,C,Tx], grad_queries_out_dev [B,C,Ty]: either may be NULL, not both.  The prior gets no gradient.
 * t_xs_dev, prior_dev, grad_soft_dev may be NULL.  Masked rows get dK = 0 exactly; an utterance with t_x <= 0 gets zeros.
 * The logits are recomputed (fp32 products); the result is the same bits on every call (no atomics).
 * C <= 256 and Tx <= 512 (ALIGNER_EDOM beyond); workspace aligner_softattn_backward_workspace_bytes(B,C,Tx,Ty) bytes.
 */
size_t aligner_softattn_backward_workspace_bytes(int B, int C, int Tx, int Ty);
int aligner_softattn_backward_f32(const float *keys_dev, const float *queries_dev, const int32_t *t_xs_dev,
                                  const float *prior_dev, const float *grad_logp_dev, const float *grad_soft_dev,
                                  float *grad_keys_out_dev, float *grad_queries_out_dev,
                                  void *workspace_dev, size_t workspace_bytes,
                                  int B, int C, int Tx, int Ty, float temperature, int sim, void *stream);

/* ---- Glow-TTS / VITS log-likelihood front end --------------------------- */

/*
 * The `value` tensor Glow-TTS and VITS hand to monotonic_align.maximum_path: the log-density of every latent frame under
 * every token's diagonal Gaussian,
 *   value[b,i,j] = sum_c ( -1/2 ln 2pi - logstd[b,c,i] - 1/2 (z[b,c,j] - mean[b,c,i])^2 exp(-2 logstd[b,c,i]) )
 *   z_dev       [B,C,Ty] fp32  the flow's output    (channel-major, as both models hold it)
 *   mean_dev    [B,C,Tx] fp32  the text encoder's mean
 *   logstd_dev  [B,C,Tx] fp32  its log standard deviation
 *   t_xs_dev, t_ys_dev  optional [B] int32 lengths; NULL = the full extent (Tx / Ty)
 *   value_out_dev  element [b,i,j] at ((b*Tx + i)*ld_value + j), of value_dtype F32, or BF16 as the round-to-nearest-even
 *               of the fp32 result (aligner_maxpath / aligner_maxpath_ld read either as it is).  ld_value == Ty
 *               (contiguous), or a row pitch ld_value > Ty with rows on 16-byte boundaries -- the pipeline's own
 *               intermediate in front of aligner_maxpath_ld.  Only the columns < Ty are written.
 *   workspace_dev  aligner_gauss_logp_workspace_bytes(B,C,Tx) bytes (0 for a shape that is not supported): the [Tx,2C]
 *               operand (exp(-2 logstd), mean exp(-2 logstd)) split to bf16 halves in MFMA fragment order and the
 *               per-token constant, prepared once per call.
 * Masked cells: a cell with i >= t_x[b] or j >= t_y[b] is written as 0.0 -- what Glow-TTS's `logp * attn_mask` and the
 * reference's `value * mask` hold there; an utterance with t_x <= 0 or t_y <= 0 is all zeros.
 * Arithmetic: the sum is expanded into one contraction of depth 2C plus a per-token constant and runs on the bf16 matrix
 * cores with every fp32 operand split in two bf16 halves (hi*hi + hi*lo + lo*hi, fp32 accumulate: ~2^-16 relative per
 * product).  The expanded terms cancel where z ~ mean and the deviation is small, so the error is relative to the
 * magnitude of what is summed, S = sum_c (1/2 z^2 w + |z mean| w + 1/2 mean^2 w + |logstd| + 1/2 ln 2pi), w = exp(-2
 * logstd): |value - exact| <= 2^-14 S.  No atomics: the same bits on every call.  Its gradient:
 * aligner_gauss_logp_backward_f32.
 * Domain: 1 <= C <= 256 (any C: the contraction is padded with zeros inside the kernel), Tx <= 1024, any Ty, B <= 65535,
 * Tx*ld_value < 2^29: ALIGNER_EDOM beyond; ALIGNER_EINVAL for a null pointer, a shape below 1, ld_value < Ty or a dtype
 * other than F32 / BF16.  Arguments are validated before any HIP call.  Two launches (prepare, main), asynchronous.
 */
size_t aligner_gauss_logp_workspace_bytes(int B, int C, int Tx);
int aligner_gauss_logp(const float *z_dev, const float *mean_dev, const float *logstd_dev,
                       const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                       void *value_out_dev, int value_dtype, int ld_value,
                       void *workspace_dev, size_t workspace_bytes,
                       int B, int C, int Tx, int Ty, void *stream);

/*
 * The vector-Jacobian product of aligner_gauss_logp: with G = grad_value (the gradient of a loss with respect to value,
 * e.g. aligner_forward_sum_f32's gradient tensor), cells with i >= t_x[b] or j >= t_y[b] contributing nothing, and
 * w = exp(-2 logstd),
 *   R[i] = sum_j G[i,j]   P[c,i] = sum_j G[i,j] z[c,j]   Q[c,i] = sum_j G[i,j] z[c,j]^2
 *   U[c,j] = sum_i G[i,j] w[c,i]   V[c,j] = sum_i G[i,j] (mean w)[c,i]
 *   dz = V - z U      dmean = w (P - mean R)      dlogstd = w (Q - 2 mean P + mean^2 R) - R
 *   grad_value_dev  element [b,i,j] at ((b*Tx + i)*ld_grad + j), fp32; ld_grad == Ty or a row pitch > Ty with rows on
 *               16-byte boundaries.  Neither a cell outside the lengths nor a pad column is read into any result (a NaN
 *               there is harmless).
 *   grad_scale_dev  optional [B] fp32: G[b] is read as grad_scale[b] * G[b] (the cotangent of a per-utterance loss,
 *               without a scaling pass over G)
 *   z_dev, mean_dev, logstd_dev, t_xs_dev, t_ys_dev  as for aligner_gauss_logp (the same clamping of the lengths)
 *   dz_out_dev [B,C,Ty], dmean_out_dev [B,C,Tx], dlogstd_out_dev [B,C,Tx]  fp32, each fully written (frames >= t_y,
 *               tokens >= t_x and empty utterances: +0.0); each may be NULL, not all three.  A NULL dz skips the
 *               contraction over tokens, NULL dmean and dlogstd the one over frames.
 *   workspace_dev  aligner_gauss_logp_backward_workspace_bytes(B,C,Tx,Ty) bytes (0 for a shape that is not supported)
 * Arithmetic: U, V, P, Q with the forward's three split bf16 products per fp32 product, R in fp32.  Per element
 * |got - exact| <= 2^-14 S with S the magnitude of what the expanded sums add up.  No atomics, the frame
 * sweep is split over workgroups by the shape alone and summed in split order: the same bits on every call.
 * Domain: 1 <= C <= 256, Tx <= 1024, B <= 65535: ALIGNER_EDOM beyond; ALIGNER_EINVAL for a null pointer, no output, a
 * shape below 1 or a bad ld_grad; ALIGNER_ENOSPC for a workspace that is too small.  Validated before any HIP call.
 */
size_t aligner_gauss_logp_backward_workspace_bytes(int B, int C, int Tx, int Ty);
int aligner_gauss_logp_backward_f32(const float *grad_value_dev, int ld_grad, const float *grad_scale_dev,
                                    const float *z_dev, const float *mean_dev, const float *logstd_dev,
                                    const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                                    float *dz_out_dev, float *dmean_out_dev, float *dlogstd_out_dev,
                                    void *workspace_dev, size_t workspace_bytes,
                                    int B, int C, int Tx, int Ty, void *stream);

/*
 * The loss those models train on once the alignment is found: the negative log-likelihood of every latent frame under
 * the Gaussian of the token that owns it, and its gradient.  With ends[x] = sum(max(durations[b,i],0), i <= x) -- the
 * segments of aligner_regulate_f32 / aligner_segment_reduce_f32 -- token x owns the frames ends[x-1] <= y < ends[x]; a
 * frame counts when it has an owner, y < Ty and, with t_ys_dev given, y < t_ys[b].  For a counting frame
 * w = exp(-2 logstd[b,c,x]), d = z[b,c,y] - mean[b,c,x], and n_x is the number of counting frames of token x:
 *   nll_out[b]        = sum over the counting frames and the channels of ( 1/2 ln 2pi + logstd[b,c,x] + 1/2 d^2 w )
 *   count_out[b]      = number of counting frames (nll / (C count) is the Glow-TTS loss; a VITS KL term is nll minus
 *                       quantities that do not depend on the alignment)
 *   grad_z[b,c,y]     =  scale[b] d w                       (+0.0 on a frame that does not count)
 *   grad_mean[b,c,x]  = -scale[b] sum_{y of x} d w          (+0.0 for a token without a counting frame)
 *   grad_logstd[b,c,x] = scale[b] ( n_x - w sum_{y of x} d^2 )       (likewise)
 *   z_dev [B,C,Ty], mean_dev and logstd_dev [B,C,Tx] fp32; durations_dev [B,Tx] int32; t_ys_dev optional [B] int32;
 *   scale_dev optional [B] fp32 on the device, the upstream gradient of nll[b] (NULL: 1);
 *   nll_out_dev optional [B] fp32; count_out_dev optional [B] int32;
 *   grad_z_dev [B,C,Ty], grad_mean_dev and grad_logstd_dev [B,C,Tx] fp32: all three or none; every element is written;
 *   workspace_dev  aligner_gauss_nll_workspace_bytes(B,C,Tx) bytes (0 for a shape that is not supported): one loss
 *               partial per (utterance, channel) row.
 * One streaming kernel reads z once (and writes grad_z once); a workgroup owns whole (utterance, channel) rows, the
 * per-token sums are a segmented scan over the lanes into per-token accumulators in LDS; a second small kernel adds an
 * utterance's C partials in a fixed order.  No atomics: the same bits on every call.  Ty % 4 == 0 with 16-byte aligned
 * z_dev (and grad_z_dev) takes the 16-byte loads and stores.  fp32 throughout; a sum of n terms carries an error of at
 * most (n + 8) 2^-24 times the sum of the terms' magnitudes.
 * ALIGNER_EINVAL: a null z / mean / logstd / durations / workspace pointer, a shape below 1, one or two of the three
 * gradient pointers, or no output at all.  ALIGNER_EDOM: Tx > 2048 (the segment reduction's limit), B > 65535, or
 * B*C*max(Tx,Ty) past 2^31 - 1 (32-bit frame indexing).  ALIGNER_ENOSPC: workspace_bytes too small.  Arguments are
 * validated before any HIP call.  One or two launches, asynchronous.
 */
size_t aligner_gauss_nll_workspace_bytes(int B, int C, int Tx);
int aligner_gauss_nll_f32(const float *z_dev, const float *mean_dev, const float *logstd_dev,
                          const int32_t *durations_dev, const int32_t *t_ys_dev, const float *scale_dev,
                          float *nll_out_dev, int32_t *count_out_dev,
                          float *grad_z_dev, float *grad_mean_dev, float *grad_logstd_dev,
                          void *workspace_dev, size_t workspace_bytes,
                          int B, int C, int Tx, int Ty, void *stream);

/*
 * Gaussian upsampling, the differentiable length regulator of JETS, Non-Attentive Tacotron, Parallel Tacotron and
 * ESPnet's GaussianUpsampling.  Frame y sits at tau_y = y + frame_offset; with tx = clamp(t_xs[b], 0, Tx) and
 * ty = clamp(t_ys[b], 0, Ty) (NULL: the full extent),
 *   e[b,y,x]   = log_weight[b,x] - precision[b,x] (tau_y - centre[b,x])^2        x < tx
 *   p[b,y,.]   = softmax over those x
 *   out[b,:,y] = sum_x p[b,y,x] h[b,:,x]                                          y < ty; +0.0 beyond, and everywhere
 *                                                                                 when tx = 0
 * and backward, with G = g_out (a frame y >= ty contributes nothing, whatever g_out holds there),
 *   q[y,x] = sum_c G[c,y] h[c,x]     r[y] = sum_x p q     de[y,x] = p (q - r)
 *   dh[c,x] = sum_y p[y,x] G[c,y]    dlog_weight[x] = sum_y de    dprecision[x] = -sum_y de (tau_y - centre_x)^2
 *   dcentre[x] = sum_y de 2 precision_x (tau_y - centre_x)
 *   h_dev [B,C,Tx], out_dev / g_out_dev [B,C,Ty] fp32; centre_dev, precision_dev [B,Tx] fp32 (precision >= 0: a negative
 *   one is the caller's error and is not checked); log_weight_dev optional [B,Tx] fp32 (NULL: 0); t_xs_dev, t_ys_dev
 *   optional [B] int32; dh_dev [B,C,Tx], dcentre_dev / dprecision_dev / dlog_weight_dev [B,Tx]: each may be NULL (not
 *   wanted; at least one is), every element of a given one is written, +0.0 for a token x >= tx and everywhere for an
 *   utterance with tx = 0 or ty = 0.
 * Truncation is part of the contract: a kernel may treat as zero any token whose energy is more than
 * ALIGNER_GAUSS_UP_CUT below the frame's largest energy, and includes every other token (e^-30 = 9.4e-14: nothing against
 * 2^-24 for Tx <= 2048).  With the centres non-decreasing over x < tx a tile of 64 frames then needs one contiguous token
 * interval, found from the centres, the utterance's smallest precision and largest log-weight; an utterance whose centres
 * are out of order, or whose precision is not positive everywhere, or that holds a value that is not finite, takes the
 * full token range: slower, the same definition.  The weights are never stored; the backward pass recomputes them and
 * does not need out.  fp32 arithmetic, exact products (no matrix cores), the denominator summed in double; no
 * floating-point atomics: the same bits on every call.  Forward: two launches; backward: three or four.
 *   workspace_dev  aligner_gauss_upsample_workspace_bytes / aligner_gauss_upsample_backward_workspace_bytes (B,C,Tx,Ty)
 *               bytes (0 for a shape that is not supported): the tiles' token intervals; backward also the frames'
 *               maxima and denominators and six partial sums per (frame tile, token).
 * ALIGNER_EINVAL: a null required pointer, a shape below 1, no output requested.  ALIGNER_EDOM: Tx > 2048 (the duration
 * kernels' limit), B > 65535.  ALIGNER_ENOSPC: workspace_bytes too small.  Arguments are validated before any HIP call.
 */
#define ALIGNER_GAUSS_UP_CUT 30.0f
size_t aligner_gauss_upsample_workspace_bytes(int B, int C, int Tx, int Ty);
int aligner_gauss_upsample_f32(const float *h_dev, const float *centre_dev, const float *precision_dev,
                               const float *log_weight_dev, const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                               float frame_offset, float *out_dev,
                               void *workspace_dev, size_t workspace_bytes,
                               int B, int C, int Tx, int Ty, void *stream);
size_t aligner_gauss_upsample_backward_workspace_bytes(int B, int C, int Tx, int Ty);
int aligner_gauss_upsample_backward_f32(const float *h_dev, const float *centre_dev, const float *precision_dev,
                                        const float *log_weight_dev, const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                                        float frame_offset, const float *g_out_dev,
                                        float *dh_dev, float *dcentre_dev, float *dprecision_dev, float *dlog_weight_dev,
                                        void *workspace_dev, size_t workspace_bytes,
                                        int B, int C, int Tx, int Ty, void *stream);

/*
 * y[b,o,t] = act( bias[o] + sum_{i,k} w[o,i,k] * x[b,i,t+k-K/2] ), zero padded
 * ("same"), K odd; the 1-D conv of the text / mel encoders. relu: 0 or 1.
 * Weights prepared once (split into bf16 halves, in the matrix cores'
 * fragment order): aligner_conv1d_prepare_f32 writes aligner_conv1d_prepared_bytes(Cout,Cin,K) bytes,
 * aligner_conv1d_prepared_f32 consumes them.  Products are hi*hi + hi*lo + lo*hi in fp32 accumulators
 * (~2^-16 relative per product).  This is the fast path of the encoders: prepare per weight update.
 *
 * Numerics, the same for every entry point and kernel form of this section, per layer and per output element:
 *   |y - exact| <= (3 * 2^-16 + accumulation) * (|bias[o]| + sum_{i,k} |w[o,i,k]| |x[b,i,t+k-K/2]|)
 * 3 * 2^-16 is the worst case of one split product (the dropped lo*lo and the two rounding terms), whatever the input's
 * scale, offset or dynamic range and whatever the fan-in; the accumulation term is that of an fp32 sum over the
 * Cin * K products in the matrix cores' order (a few 2^-24 to a few 10 * 2^-24: tests/conv_oracle.py tabulates it).
 * A stack carries each layer's error through the next layer's |w| (ReLU is 1-Lipschitz).
 * Non-finite activations: a NaN gives NaN in its receptive field, in every output channel, and PASSES THROUGH ReLU
 * (as torch.relu; every other element keeps the bits it would have had).  +-Inf activations come out as NaN, not as
 * +-Inf (the split takes lo = v - hi = inf - inf), in the same receptive field.
 * The result never depends on what the workspace held before the call.
 */
size_t aligner_conv1d_prepared_bytes(int Cout, int Cin, int K);
int aligner_conv1d_prepare_f32(const float *w_dev, void *prepared_dev, size_t prepared_bytes,
                               int Cout, int Cin, int K, void *stream);
int aligner_conv1d_prepared_f32(const float *x_dev, const void *prepared_dev, const float *bias_dev,
                                float *y_dev, int B, int Cin, int Cout, int T, int K,
                                int relu, void *stream);
/*
 * ... and with a workspace, which the fast form needs (csrc/convgemm.hip): the activations are split into bf16 halves
 * and transposed to channels-last fragments by a streaming pass into the workspace
 * (aligner_conv1d_workspace_bytes(B,Cin,Cout,T,K) bytes, 16-byte aligned; 0 = this layer has no such form and takes the
 * kernel of aligner_conv1d_prepared_f32), then a GEMM-structured kernel multiplies them with the prepared weights --
 * activations global -> LDS by LDS-DMA, the weights' fragments straight into registers, nothing waited for inside the
 * loop.  Same numerics as above.
 */
size_t aligner_conv1d_workspace_bytes(int B, int Cin, int Cout, int T, int K);
int aligner_conv1d_prepared_ws_f32(const float *x_dev, const void *prepared_dev, const float *bias_dev,
                                   float *y_dev, void *workspace_dev, size_t workspace_bytes,
                                   int B, int Cin, int Cout, int T, int K, int relu, void *stream);

/*
 * A whole encoder stack y = conv_n(...act(conv_1(x))) in one call (the text / mel encoders of SURVEY.md 7.4): the first
 * layer's input is split once, every k = 1 layer reads the split image its producer's epilogue wrote (no fp32 round trip
 * between layers), the last layer writes fp32 [B, Cout_n, T].  layers[i].prepared = that layer's
 * aligner_conv1d_prepare_f32 image; workspace aligner_conv_stack_workspace_bytes(...) bytes, 16-byte aligned
 * (0: some layer has no GEMM form -- run the layers one by one through aligner_conv1d_prepared_ws_f32 instead).
 */
typedef struct aligner_conv_layer {
    const void *prepared;       /* device: aligner_conv1d_prepare_f32(w, ..., Cout, Cin, K) */
    const float *bias;          /* device, [Cout], nullable */
    int Cin, Cout, K, relu;
} aligner_conv_layer;
size_t aligner_conv_stack_workspace_bytes(const aligner_conv_layer *layers, int n_layers, int B, int T);
int aligner_conv_stack_f32(const float *x_dev, const aligner_conv_layer *layers, int n_layers, float *y_dev,
                           void *workspace_dev, size_t workspace_bytes, int B, int T, void *stream);

/*
 * Backward of y = act(conv1d(x, w, b)) (act: ReLU when relu = 1, none when 0):
 *   dYpre = 0 where y <= 0, dY elsewhere (torch.relu's rule: y = +0, -0 and y < 0 mask, a NaN y passes its cotangent;
 *   dY when relu = 0), db[o] = sum_{b,t} dYpre[b,o,t], dW[o,i,k] = sum_{b,t} dYpre[b,o,t] x[b,i,t+k-K/2]
 *   dX = conv1d(dYpre, w') with w'[i,o,k] = w[o,i,K-1-k]: aligner_conv1d_prepare_transposed_f32 writes the prepared image
 *   of w' straight from w [Cout,Cin,K] (aligner_conv1d_prepared_bytes(Cin, Cout, K) bytes), then
 *   aligner_conv1d_prepared_ws_f32(dYpre, image, NULL bias, dX, ..., Cin = Cout, Cout = Cin, K, relu = 0).
 * aligner_conv1d_backward_weight_f32: x_dev [B,Cin,T], y_dev [B,Cout,T] (relu = 1 only; may be NULL otherwise),
 *   grad_y_dev [B,Cout,T]; outputs, each nullable but not all: grad_ypre_out_dev [B,Cout,T] (dYpre, for the dX call),
 *   grad_w_out_dev [Cout,Cin,K], grad_b_out_dev [Cout].  fp32 products, the reduction split over workgroups and summed in
 *   a fixed order (the same bits on every call); workspace aligner_conv1d_backward_workspace_bytes(B,Cin,Cout,T,K) bytes
 *   (not needed when only grad_ypre_out_dev is asked for).
 */
int aligner_conv1d_prepare_transposed_f32(const float *w_dev, void *prepared_dev, size_t prepared_bytes,
                                          int Cout, int Cin, int K, void *stream);
size_t aligner_conv1d_backward_workspace_bytes(int B, int Cin, int Cout, int T, int K);
int aligner_conv1d_backward_weight_f32(const float *x_dev, const float *y_dev, const float *grad_y_dev,
                                       float *grad_ypre_out_dev, float *grad_w_out_dev, float *grad_b_out_dev,
                                       void *workspace_dev, size_t workspace_bytes,
                                       int B, int Cin, int Cout, int T, int K, int relu, void *stream);

/* ---- the callers either side of the path (build-defined specs) ---- */

/*
 * Forward-sum alignment objective: loss[b] = -log of the summed likelihood of ALL monotonic
 * alignments of logp[b] -- the column recurrence of maximum_path_each (core.pyx:17-30) with
 * log-sum-exp in place of max -- and, when grad_out_dev is not NULL, its gradient
 * d loss / d logp = -(posterior occupancy of each cell), 0 outside [0,t_x) x [0,t_y).
 *   logp_dev [B,Tx,Ty] fp32 (Tx <= 1024), t_xs_dev/t_ys_dev [B] int32, loss_out_dev [B] fp32
 *   (+inf where t_x < 1 or t_x > t_y), grad_out_dev optional [B,Tx,Ty] fp32,
 *   workspace_dev aligner_forward_sum_workspace_bytes(B,Tx,Ty) bytes (the alpha tiles).
 * -inf log-probs are legal (log 0: a hard mask, the padding rows of soft_attention).  An utterance whose EVERY alignment
 * crosses such a cell -- log Z below half the kernels' finite "log 0" of -1e30 -- has no alignment either: loss +inf and an
 * all-zero gradient, exactly as for t_x > t_y; the other utterances of the batch are not affected.
 * With the gradient, batches of at most half the CU count run the alpha and the beta sweep side by side in one launch
 * (beta travels through grad_out_dev) and a combining pass writes the gradient in place; larger batches run forward, then
 * backward.  Same results up to fp32 rounding of the exponent sum (tests/test_objective.py).  T_mel % 4 == 0 and 16-byte
 * aligned logp / grad pointers take the faster tile movers.
 */
size_t aligner_forward_sum_workspace_bytes(int B, int Tx, int Ty);
int aligner_forward_sum_f32(const float *logp_dev, const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                            float *loss_out_dev, float *grad_out_dev,
                            void *workspace_dev, size_t workspace_bytes,
                            int B, int Tx, int Ty, void *stream);

/*
 * The CTC form of the same objective -- the published one (OTA's forward-sum loss, README.md:21-25,50): a blank column
 * of log-prob `blank_logprob` (-1 in the paper's code) is put before the text rows, every frame is renormalised over
 * blank + the utterance's t_x text rows (log_softmax), and loss[b] = CTC loss of the token sequence 1..t_x over the
 * t_y frames = torch.nn.functional.ctc_loss(log_softmax(pad(scores)), targets = 1..t_x, reduction = "none") -- which
 * is what tests/test_objective.py checks it against, in float64.  grad_out_dev (optional) = d loss / d scores
 * = softmax over blank + text of the frame - posterior occupancy of the token, 0 outside [0,t_x) x [0,t_y).
 * scores_dev [B,Tx,Ty] fp32 (Tx <= 1023); loss +inf where t_x < 1 or t_x > t_y (no labelling exists; gradient 0).
 */
size_t aligner_forward_sum_ctc_workspace_bytes(int B, int Tx, int Ty);
int aligner_forward_sum_ctc_f32(const float *scores_dev, const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                                float blank_logprob, float *loss_out_dev, float *grad_out_dev,
                                void *workspace_dev, size_t workspace_bytes,
                                int B, int Tx, int Ty, void *stream);

/* prior[b,x,y] = BetaBinomial(n = t_x, a = scaling*(y+1), b = scaling*(t_y-y)).pmf(x) for x < t_x,
 * y < t_y, 0 elsewhere; [B,Tx,Ty] fp32, the `prior_dev` operand of aligner_softattn_f32.
 * t_x = t_xs[b] clamped to [0,Tx] and t_y = t_ys[b] clamped to [0,Ty]: a longer utterance gets the prior of the
 * container's extent, one with t_x < 1 is all zero.  `scaling` is used at its fp32 value.  Tx <= 7679 (ALIGNER_EDOM
 * beyond); scaling <= 0 or NaN is ALIGNER_EINVAL. */
int aligner_beta_binomial_prior_f32(const int32_t *t_xs_dev, const int32_t *t_ys_dev, float *prior_out_dev,
                                    int B, int Tx, int Ty, float scaling, void *stream);

/* Length regulator: out[b,c,y] = h[b,c,x(y)] where x(y) is the token whose duration interval holds
 * frame y (durations as aligner_maxpath_f32 writes them, negative values count as 0); frames past
 * sum(durations[b]) are 0.  h_dev [B,C,Tx], durations_dev [B,Tx] int32, out_dev optional [B,C,Ty],
 * tok_out_dev optional [B,Ty] int32 (-1 past the end). */
int aligner_regulate_f32(const float *h_dev, const int32_t *durations_dev, float *out_dev, int32_t *tok_out_dev,
                         int B, int C, int Tx, int Ty, void *stream);

/*
 * Segment reduction over the durations, frames -> tokens: the inverse direction of the length regulator.  With
 * s_x = sum(max(durations[b,i],0), i < x) and e_x = s_x + max(durations[b,x],0) -- exactly the segments
 * aligner_regulate_f32 defines: negative durations count as 0, a sum that runs past Ty is clipped --
 *   tokens_out[b,c,x] = sum of frames[b,c,y] over y in [s_x, e_x) and [0, Ty)
 * and with mean != 0 that sum divided by the number of frames actually summed.  A token without a frame gets 0; every
 * element of tokens_out is written.  mean = 0 is the adjoint of aligner_regulate_f32 (the regulator's gradient with
 * respect to h: pass the gradient of its output as `frames`); mean = 1 is the per-token averaging of pitch / energy.
 *   frames_dev [B,C,Ty] fp32, durations_dev [B,Tx] int32, tokens_out_dev [B,C,Tx] fp32; Tx <= 2048 (ALIGNER_EDOM beyond).
 * Deterministic: a workgroup owns whole (utterance, channel) rows, a wave sums a row's frames in one fixed order
 * (segmented scan over the lanes, per-token accumulators in LDS), no atomics -- the same bits on every run, and a run
 * time that does not depend on how the frames are distributed over the tokens.  Ty % 4 == 0 and a 16-byte aligned
 * frames pointer take the 16-byte loads.
 */
int aligner_segment_reduce_f32(const float *frames_dev, const int32_t *durations_dev, float *tokens_out_dev,
                               int B, int C, int Tx, int Ty, int mean, void *stream);

/*
 * Binarization loss of the OTA aligner: minus the summed log soft-probability at the cells of the hard path (the
 * published form is log(clamp(soft, 1e-12)) at the path's cells, averaged over them; neither the reference snapshot
 * nor SNIPPETS.md holds that code: parity unpinned, like the other OTA pieces).
 * A frame (b,y) counts when 0 <= tok[b,y] < Tx and, with t_ys_dev given, y < t_ys[b].
 *   nll_out[b]   = -sum over the counting frames of max(logp[b, tok[b,y], y], min_logp)
 *   count_out[b] = number of counting frames
 * A cell below min_logp (-inf and NaN included) contributes min_logp to the loss and nothing to the gradient.
 *   logp_dev [B,Tx,*] of logp_dtype F32, BF16 or F16 at a row pitch of ld_logp >= Ty elements (as aligner_maxpath_ld:
 *   the pipeline's pitched log-probs are read in place); tok_dev [B,Ty] int32 as aligner_maxpath / aligner_regulate_f32
 *   write it; t_ys_dev optional [B] int32; nll_out_dev [B] fp32; count_out_dev [B] int32; Tx <= 2048 (ALIGNER_EDOM).
 * One workgroup per utterance and a fixed summation order: deterministic.
 */
int aligner_bin_loss(const void *logp_dev, int logp_dtype, int ld_logp, const int32_t *tok_dev,
                     const int32_t *t_ys_dev, float min_logp, float *nll_out_dev, int32_t *count_out_dev,
                     int B, int Tx, int Ty, void *stream);

/*
 * Its gradient, d sum_b(scale[b] * nll[b]) / d logp: -scale[b] at every counting cell with logp > min_logp, 0 elsewhere.
 *   scale_dev [B] fp32 on the device (so a normaliser such as 1 / sum(count) never visits the host);
 *   grad_dev [B,Tx,Ty] fp32, contiguous.
 * accumulate = 0: the whole tensor is written (+0 off the path).  accumulate = 1: -scale[b] is added to those cells
 * and nothing else is touched -- the way to put the binarization term into a gradient that is already there
 * (aligner_forward_sum_ctc_f32's) without a zero-fill or a dense add.
 */
int aligner_bin_loss_grad_f32(const void *logp_dev, int logp_dtype, int ld_logp, const int32_t *tok_dev,
                              const int32_t *t_ys_dev, float min_logp, const float *scale_dev, float *grad_dev,
                              int accumulate, int B, int Tx, int Ty, void *stream);

/*
 * Hard alignment search with optional pauses between tokens: the Viterbi path over the CTC topology of the token
 * sequence, the decoding counterpart of aligner_forward_sum_ctc_f32's blank (build-defined spec: neither the reference
 * snapshot nor SNIPPETS.md holds code for it; stated in full in csrc/pausepath.hip and tests/pausepath_oracle.py).
 * States s = 0 .. 2 t_x per utterance: s = 2g is the pause in gap g (the place before token g; gap 0 leads, gap t_x
 * trails) and scores pause[y] on frame y, s = 2x+1 is token x and scores value[x,y].  A token takes at least one frame,
 * a pause zero or more; a path moves from a state to itself, to the next state, or from a token straight to the next
 * token.  Arithmetic is fp32, one add per cell; among the predecessors that exist (stay, advance, skip -- in this order)
 * a later one replaces an earlier one only when strictly greater, so ties keep the earlier and a NaN never wins; the path
 * ends in the last token unless the trailing pause exists on the last frame and is strictly greater.  Predecessors
 * outside the band are excluded, not scored: the result is a legal path (monotone, every token at least one frame,
 * durations summing to t_y) for any scores, -inf and NaN included.
 *   value_dev [B,Tx,*] of value_dtype F32, BF16 or F16 at a row pitch of ld_value >= Ty elements (read in place)
 *   pause_dev optional [B,Ty] fp32 pause score per frame; NULL: pause_score on every frame
 *   gap_mask_dev optional [B,Tx+1] uint8: a gap whose entry is 0 holds no pause; NULL: every gap may
 *   t_xs_dev, t_ys_dev [B] int32
 * Outputs, each optional, at least one; every element of a requested one is written:
 *   tok_out [B,Ty] int32: x on a frame of token x, -2-g on a pause frame of gap g, -1 for y >= t_y (negative means
 *                 "no token": aligner_bin_loss skips such frames)
 *   durations_out [B,Tx] int32 frames per token; pauses_out [B,Tx+1] int32 frames per gap
 *   state_durations_out [B,2*Tx+1] int32: the same numbers interleaved (even entries gaps, odd entries tokens) -- what
 *                 aligner_regulate_f32 takes for text encodings interleaved with a pause embedding
 *   score_out [B] fp32: the path's running score on its last frame
 * An utterance with t_x < 1, t_y < 1, t_x > t_y or a length outside [0,Tx] / [0,Ty] has no path: durations and pauses
 * 0, tok -1, score -inf; the others of the batch are unaffected.
 * One launch (sweep, backtrack and outputs), one workgroup per utterance, no atomics: deterministic.  Tx <= 1024
 * (ALIGNER_EDOM beyond).  The workspace holds decision words only, for shapes whose words do not fit LDS:
 * aligner_pausepath_workspace_bytes(B,Tx,Ty) bytes, 0 when they fit -- and 0 for a shape that is not supported.  Both
 * functions decide "fits" against gfx950's 160 KiB of LDS per workgroup, so a caller who is told 0 bytes is never asked
 * for more; on a device that gives a workgroup less than the launch needs the call fails with ALIGNER_EDOM.
 */
size_t aligner_pausepath_workspace_bytes(int B, int Tx, int Ty);
int aligner_pausepath(const void *value_dev, int value_dtype, int ld_value, const float *pause_dev, float pause_score,
                      const uint8_t *gap_mask_dev, const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                      int32_t *tok_out_dev, int32_t *durations_out_dev, int32_t *pauses_out_dev,
                      int32_t *state_durations_out_dev, float *score_out_dev,
                      void *workspace_dev, size_t workspace_bytes, int B, int Tx, int Ty, void *stream);

/*
 * CTC forced alignment from emissions: the Viterbi path of a transcript through the frame scores of a CTC acoustic
 * model (what torchaudio.functional.forced_align computes, for a whole batch and with repeated labels; build-defined
 * spec, stated in full in csrc/ctcalign.hip and tests/ctcalign_oracle.py).  Per utterance b: t_y = t_ys[b] frames,
 * t_x = t_xs[b] labels lab[x] = targets[b,x], emissions e[y,v] = log_probs[b,y,v] -- any scores, they need not be
 * normalised; read as fp32, 16-bit inputs up-cast exactly.
 * States s = 0 .. 2 t_x: s = 2g is the blank in gap g (the place before token g; gap 0 leads, gap t_x trails) and scores
 * e[y,blank]; s = 2x+1 is token x and scores e[y,lab[x]].  Moves: stay s -> s, advance s-1 -> s, and skip s-2 -> s only
 * into a token x >= 1 with lab[x] != lab[x-1]: between two equal labels the blank is mandatory.  A token takes at
 * least one frame, a blank zero or more.
 * Band: a state exists at frame y iff it lies on a legal path.  With r[x] = 1 if x >= 1 and lab[x] == lab[x-1] else 0,
 * R[x] = r[0] + .. + r[x] and Rt = R[t_x-1]:
 *   token x iff x + R[x] <= y and t_y-1-y >= (t_x-1-x) + (Rt - R[x]);
 *   blank g iff g + (g >= 1 ? R[g-1] : 0) <= y and t_y-1-y >= (t_x-g) + (g < t_x ? Rt - R[g] : 0).
 * Recurrence, ties and end are aligner_pausepath's: Q[s,0] = score(s,0) for the states 0 and 1 that exist;
 * Q[s,y] = Q[pred,y-1] + score(s,y), one fp32 add; pred among the candidates that exist at y-1 in the order stay,
 * advance, skip, a later one replacing an earlier one only when strictly greater (a NaN never wins); the path ends in
 * 2 t_x - 1 unless the trailing blank exists at t_y-1 and is strictly greater.  Absent candidates are excluded, not
 * scored: the result is a legal path for any scores, -inf and NaN included.
 *   log_probs_dev [B,T,V] of dtype F32, BF16 or F16; stride_b, stride_t in elements, the vocabulary axis contiguous
 *                 (stride_t >= V; any stride_b >= 0: a [T,B,V] tensor is read in place with stride_b = V, stride_t = B V)
 *   blank in [0,V).  A label equal to blank is an ordinary label that happens to score the blank column.
 *   targets_dev [B,L] int32; t_xs_dev (target lengths), t_ys_dev (input lengths) [B] int32
 * Outputs, each optional, at least one; every element of a requested one is written:
 *   tok_out [B,T] int32: x on a frame of token x, -2-g on a blank frame of gap g, -1 for y >= t_y (aligner_pausepath's)
 *   labels_out [B,T] int32: the vocabulary entry of the frame's state, lab[x] or blank; -1 for y >= t_y
 *   frame_scores_out [B,T] fp32: the emission at that state (the input's bits, up-cast); 0 for y >= t_y
 *   durations_out [B,L], pauses_out [B,L+1], state_durations_out [B,2L+1] int32, score_out [B] fp32: as aligner_pausepath's
 * No path: t_x < 1, t_y < 1, t_x + Rt > t_y, a length outside [0,L] / [0,T], or a label outside [0,V) (checked as the
 * labels are loaded, before any emission is read: no load leaves a row of V).  Such an utterance gets durations and
 * pauses 0, tok and labels -1, frame_scores 0 and score -inf; the others of the batch are unaffected.
 * One launch, one workgroup per utterance, no atomics: deterministic.  ALIGNER_EINVAL: a null input, no output, a bad
 * shape (B < 0, L < 1 or T < 1; B = 0 is an empty batch and succeeds), V < 1, blank outside [0,V), stride_t < V,
 * stride_b < 0, a dtype other than the three.  ALIGNER_EDOM: L > 1024, B > 65535,
 * (T-1)*stride_t + V or the number of decision words beyond 2^31.  The workspace holds decision words only, for shapes
 * whose words do not fit LDS: aligner_ctc_align_workspace_bytes(B,L,T) bytes, 0 when they fit and 0 for an unsupported
 * shape, decided against gfx950's 160 KiB as aligner_pausepath_workspace_bytes does; ALIGNER_ENOSPC for a short one.
 */
size_t aligner_ctc_align_workspace_bytes(int B, int L, int T);
int aligner_ctc_align(const void *log_probs_dev, int dtype, long long stride_b, long long stride_t, int V, int blank,
                      const int32_t *targets_dev, const int32_t *t_xs_dev, const int32_t *t_ys_dev,
                      int32_t *tok_out_dev, int32_t *labels_out_dev, float *frame_scores_out_dev,
                      int32_t *durations_out_dev, int32_t *pauses_out_dev, int32_t *state_durations_out_dev,
                      float *score_out_dev, void *workspace_dev, size_t workspace_bytes, int B, int L, int T,
                      void *stream);

/*
 * MoBoAligner monotonic boundary search (BASELINE config 5; build-defined spec from the paper the reference
 * links at README.md:49 -- its code is on a branch that is not in the snapshot; stated in full in
 * oracle/mobo_oracle.py and aligner_amd/csrc/mobo.hip).  Boundaries 0 = b_-1 < b_0 < ... < b_{t_x-1} = t_y,
 * token durations 1..max_duration, P(b_i = j | b_{i-1} = k) = softmax over the feasible j in (k, k+max_duration]
 * of energies[b,i,j-1].
 *   energies_dev   [B,Tx,Ty] of energy_dtype F32, BF16 or F16 (the alignment layout, mel axis contiguous).  Domain: -inf
 *                      and NaN are masked frames (no boundary there, log_alpha -inf, gradient 0; a NaN fails every "is it
 *                      live" comparison of the kernels exactly as -inf does).  Finite energies must stay far below 2^24
 *                      base-2 units in magnitude (|e| log2(e) << 1.6e7; anything at or below -1e7 of those units counts as
 *                      log 0: MB_DEADF in mobo.hip) -- a per-token offset of a hundred nats is well inside, and changes no
 *                      result beyond rounding (the model only sees a token's energies up to a shift).  +inf and larger
 *                      finite values are outside the domain: results undefined.  tests/mobo_cases.py pins this domain.
 *   boundaries_out_dev [B,Tx] int32: b_i of the most probable boundary sequence (rows >= t_x: t_y); NULL (with
 *                      durations_out_dev and map_score_out_dev NULL as well) when only log_alpha / gamma are wanted
 *                      (masked energies that leave no boundary sequence are then not reported: log_alpha of the last
 *                      token's row is -inf everywhere, gamma 0)
 *   durations_out_dev  optional [B,Tx] int32; map_score_out_dev optional [B] fp32 (its log-probability)
 *   log_alpha_out_dev  optional [B,Tx,Ty] fp32: log P(b_i = j) at [i, j-1], -inf where impossible
 *   gamma_out_dev      optional [B,Tx,Ty] fp32 soft alignment P(b_{i-1} <= y < b_i); needs log_alpha_out_dev
 *   workspace_dev      aligner_boundary_search_workspace_bytes_ex(B,Tx,Ty,max_duration) bytes (the form without
 *                      max_duration is an upper bound for every window), first 256 zeroed once (status word as for
 *                      aligner_maxpath: ALIGNER_ST_BAD_LENGTHS for an utterance without any segmentation -- not
 *                      t_x <= t_y <= t_x*max_duration, or masked (-inf) energies that leave no boundary sequence a
 *                      positive probability; its boundaries / durations are 0 and its score -inf, and for such lengths
 *                      log_alpha is -inf and gamma 0 everywhere).  It holds the normalisers
 *                      [B,Tx,Ty] fp32, the per-(token, position) durations [B,Tx,Ty+1] u16 and the ring through
 *                      which the position segments of an utterance hand their last max_duration entries on.
 * Only the chain that is asked for runs: the max-product one alone without log_alpha_out_dev (the MAP sequence: 0.47 ms at
 * [8,500,4000], max_duration 32), the sum-product one alone without boundaries_out_dev (log_alpha, gamma: a training
 * step's forward pass), both in one kernel otherwise (0.70 ms) -- with identical results.
 * Three launches: normalisers of every (utterance, token, position) on the whole chip; the token chain with an
 * utterance's positions cut into segments, one workgroup each (as many as fit the CUs: [8,500,4000] runs 32 per
 * utterance), a segment waiting only for the one before it -- ALIGNER_ST_INTERNAL and all-zero boundaries /
 * durations for an utterance whose segment gave up waiting (only possible when other work keeps its predecessor
 * off the GPU for seconds); the MAP backtrack.  Ty is limited to 8192 positions per segment and by LDS
 * (24 bytes per position and per window entry); ALIGNER_EDOM beyond.
 */
size_t aligner_boundary_search_workspace_bytes(int B, int Tx, int Ty);
size_t aligner_boundary_search_workspace_bytes_ex(int B, int Tx, int Ty, int max_duration);
int aligner_boundary_search(const void *energies_dev, int energy_dtype,
                            const int32_t *t_xs_dev, const int32_t *t_ys_dev, int max_duration,
                            int32_t *boundaries_out_dev, int32_t *durations_out_dev, float *map_score_out_dev,
                            float *log_alpha_out_dev, float *gamma_out_dev,
                            void *workspace_dev, size_t workspace_bytes,
                            int B, int Tx, int Ty, void *stream);

/*
 * Gradient of the boundary search: d loss / d energies for a loss that reads log_alpha and / or gamma (what a
 * MoBoAligner training step needs behind the soft alignment; build-defined like the search, pinned in
 * oracle/mobo_oracle.py::boundary_search_backward to autograd over a float64 restatement of the forward pass).
 *   energies_dev, t_xs_dev, t_ys_dev, max_duration: as given to aligner_boundary_search
 *   log_alpha_dev       [B,Tx,Ty] fp32: that call's log_alpha_out_dev
 *   grad_log_alpha_dev  optional [B,Tx,Ty] fp32 cotangent of log_alpha (entries where log_alpha is -inf are ignored)
 *   grad_gamma_dev      optional [B,Tx,Ty] fp32 cotangent of gamma; at least one of the two
 *   grad_energies_out_dev [B,Tx,Ty] fp32 (0 outside an utterance's lengths and for an utterance without a
 *                       segmentation)
 *   workspace_dev       aligner_boundary_search_backward_workspace_bytes(...) bytes, first 256 zeroed once (status
 *                       word as above).  Five [B,Tx,Ty] fp32 planes and the hand-off ring.
 * The MAP outputs (boundaries, durations, map_score) are not differentiated.  Four launches: the normalisers, the
 * per-cell operands, the chain over the token rows from the last to the first (the search's position segments,
 * handing their first max_duration entries to the left), the gradient of every cell.  Same limits and the same
 * defined failure (ALIGNER_ST_INTERNAL, all-zero gradient for that utterance) as the search.
 */
size_t aligner_boundary_search_backward_workspace_bytes(int B, int Tx, int Ty, int max_duration);
int aligner_boundary_search_backward(const void *energies_dev, int energy_dtype,
                                     const int32_t *t_xs_dev, const int32_t *t_ys_dev, int max_duration,
                                     const float *log_alpha_dev, const float *grad_log_alpha_dev,
                                     const float *grad_gamma_dev, float *grad_energies_out_dev,
                                     void *workspace_dev, size_t workspace_bytes,
                                     int B, int Tx, int Ty, void *stream);

/*
 * Soft-DTW (Cuturi & Blondel 2017) between two frame sequences, and its expected alignment matrix (Mensch & Blondel
 * 2018): the loss Parallel Tacotron 2 trains on.  Build-defined (the reference snapshot has no such code).  For
 * utterance b take D = the first n rows and m columns of cost[b], gamma > 0, a warp penalty p >= 0, a band w:
 *
 *     softmin_g(a,b,c) = -gamma log(exp(-a/gamma) + exp(-b/gamma) + exp(-c/gamma))
 *     R[i,j] = D[i,j] + softmin_g(R[i-1,j-1], R[i-1,j] + p, R[i,j-1] + p)     R[-1,-1] = 0, every other border cell +inf
 *     value  = R[n-1,m-1]            E[i,j] = d value / d D[i,j]
 *
 * Cell (i,j) exists iff |i - j| <= w (bandwidth -1: no band).  A +inf cost is a forbidden cell; an utterance without a
 * finite path (|n - m| > w, a length below 1, +inf costs across every path) has value +inf and an all-zero E.  A NaN
 * cost leaves that utterance's outputs undefined and no other's.  No gradient for gamma or p.
 *   cost_dev      [B,N,M] fp32, last axis contiguous; n_dev / m_dev optional [B] int32 (null: N / M; clamped from above)
 *   value_out_dev [B] fp32
 *   grad_out_dev  optional [B,N,M] fp32: E, exactly 0 at and past n or m and outside the band.  Between the two
 *                 launches it holds R: E overwrites it in place, so the call's peak memory is the two tensors.
 *   ws_dev        aligner_soft_dtw_workspace_bytes(B,N,M,want_grad) bytes (0: shape outside the domain)
 * One workgroup per utterance and no communication between workgroups; the same bits on every call.  Domain: N <= 1024,
 * B <= 65535, N*M < 2^29: ALIGNER_EDOM beyond; ALIGNER_EINVAL for a null pointer, a shape below 1, a gamma that is
 * not positive and finite, a penalty that is negative or not finite, a bandwidth below -1; ALIGNER_ENOSPC for a
 * workspace that is too small.  Validated before any HIP call.  Asynchronous on the stream, capturable.
 */
size_t aligner_soft_dtw_workspace_bytes(int B, int N, int M, int want_grad);
int aligner_soft_dtw_f32(const float *cost_dev, const int32_t *n_dev, const int32_t *m_dev,
                         float gamma, float warp_penalty, int bandwidth,
                         float *value_out_dev, float *grad_out_dev,
                         void *ws_dev, size_t ws_bytes, int B, int N, int M, void *hip_stream);

/*
 * The L1 cost table Soft-DTW runs on, built where soft_dtw's cells exist, and its gradient.  Build-defined.  With
 * n = n_dev[b], m = m_dev[b] (null: N / M; clamped to [0,N] / [0,M]) and the band w of aligner_soft_dtw_f32:
 *
 *     cost[b,i,j] = scale sum_c |pred[b,c,i] - target[b,c,j]|      i < n, j < m, |i - j| <= w     (an existing cell)
 *                 = +inf                                           i < n, j < m, |i - j| >  w     (soft_dtw's forbidden cell)
 *                 = 0                                              at or past n or m
 *
 *     dpred[b,c,i]   =  k sum_j G[b,i,j] sign(pred[b,c,i] - target[b,c,j])      k = scale row_scale[b], rounded once
 *     dtarget[b,c,j] = -k sum_i G[b,i,j] sign(pred[b,c,i] - target[b,c,j])      (row_scale null: k = scale)
 *
 * summed over existing cells only, sign(0) = 0 (torch.cdist's subgradient), both 0 at and past the lengths.  G is
 * never read as a value where no cell exists: a NaN there reaches nothing.  Every element of each output is written.
 *   pred_dev [B,C,N], target_dev [B,C,M], cost_out_dev / grad_cost_dev [B,N,M], dpred_out_dev [B,C,N],
 *   dtarget_out_dev [B,C,M] (either may be null, not both), row_scale_dev optional [B]: all fp32, contiguous.
 * Sums run in fp32 in a fixed order, one owner per output element, no atomics: the same bits on every call.  Neither
 * call needs a workspace.  Domain: B <= 65535, C <= 4096, N*M < 2^29 (no limit on N alone: that one is the DP's):
 * ALIGNER_EDOM beyond; ALIGNER_EINVAL for a null pointer, a shape below 1, a scale that is not finite, a bandwidth
 * below -1.  Validated before any HIP call.  Asynchronous on the stream, capturable.
 */
int aligner_l1_cost_f32(const float *pred_dev, const float *target_dev, const int32_t *n_dev, const int32_t *m_dev,
                        int bandwidth, float scale, float *cost_out_dev, int B, int C, int N, int M, void *hip_stream);
int aligner_l1_cost_backward_f32(const float *grad_cost_dev, const float *pred_dev, const float *target_dev,
                                 const int32_t *n_dev, const int32_t *m_dev, int bandwidth, float scale,
                                 const float *row_scale_dev, float *dpred_out_dev, float *dtarget_out_dev,
                                 int B, int C, int N, int M, void *hip_stream);

/*
 * Soft-DTW, its L1 cost and the cost's gradient in band storage: O(N w) memory and no limit on N.  Build-defined.
 * Band storage of bandwidth w is a contiguous fp32 tensor [B,N,W], W = 2 w + 1, 0 <= w <= 127; element [b,i,d] is
 * cell (i,j) with j = i + d - w, so |i - j| <= w by construction.  With n = n_dev[b] clamped to [0,N] and m = m_dev[b]
 * clamped to [0,N+w] (null: N; no larger column can be stored), a cell exists iff i < n and 0 <= j < m.
 *
 * R, value and E are those of aligner_soft_dtw_f32 on the dense image with band w: the same recurrence, penalty,
 * forbidden +inf cells and "no alignment" convention (value +inf and an all-zero E when |n - m| > w, a length is
 * below 1, or +inf costs cross every path), from the same per-cell arithmetic.  An element whose cell does not exist
 * is never read as a value, by the DP or by the cost gradient (a NaN there reaches nothing), and every output writes
 * it as exactly 0, the cost table included (band storage has no "outside the band" to mark with +inf).
 *   cost_band_dev     [B,N,W] fp32 contiguous; value_out_dev [B] fp32
 *   grad_band_out_dev optional [B,N,W] fp32: E.  Between the two launches it holds R; E overwrites it in place.
 *   ws_dev            aligner_soft_dtw_banded_workspace_bytes(B,N,bandwidth,want_grad) bytes (0: outside the domain)
 * The cost calls take pred [B,C,N] and target [B,C,M] as aligner_l1_cost_f32 does, with m additionally clamped to M
 * (columns j >= M have no target), the same formulas, sign(0) = 0 and row_scale; either of dpred_out_dev [B,C,N] and
 * dtarget_out_dev [B,C,M] may be null, not both, and each has the same bits whether or not the other is asked for.
 * One workgroup per utterance in the DP (one wave walks the anti-diagonals of the band), one owner per output element
 * and a fixed order of summation in the cost calls, no atomics: the same bits on every call.  Domain:
 * 0 <= bandwidth <= 127, B <= 65535, C <= 4096, N*W < 2^29, no other limit on N or M: ALIGNER_EDOM beyond (a negative
 * bandwidth: ALIGNER_EINVAL); ALIGNER_EINVAL and ALIGNER_ENOSPC as in the dense calls.  Validated before any HIP call.
 * No allocation and no synchronisation inside; asynchronous on the stream, capturable.
 */
size_t aligner_soft_dtw_banded_workspace_bytes(int B, int N, int bandwidth, int want_grad);
int aligner_soft_dtw_banded_f32(const float *cost_band_dev, const int32_t *n_dev, const int32_t *m_dev,
                                float gamma, float warp_penalty, int bandwidth,
                                float *value_out_dev, float *grad_band_out_dev,
                                void *ws_dev, size_t ws_bytes, int B, int N, void *hip_stream);
int aligner_l1_cost_banded_f32(const float *pred_dev, const float *target_dev, const int32_t *n_dev, const int32_t *m_dev,
                               int bandwidth, float scale, float *cost_band_out_dev,
                               int B, int C, int N, int M, void *hip_stream);
int aligner_l1_cost_banded_backward_f32(const float *grad_band_dev, const float *pred_dev, const float *target_dev,
                                        const int32_t *n_dev, const int32_t *m_dev, int bandwidth, float scale,
                                        const float *row_scale_dev, float *dpred_out_dev, float *dtarget_out_dev,
                                        int B, int C, int N, int M, void *hip_stream);

/*
 * The Euclidean cost tables, dense and in band storage: the four L1 cost calls above with another cost in the cells.
 * Build-defined.  Existing cells, fill values (+inf / 0 dense, 0 in band storage), lengths and their clamps, band,
 * layouts, row_scale, domains, error codes and their order are those of the L1 call of the same storage form.
 *
 *     squared != 0:  cost[b,i,j] = scale      sum_c (pred[b,c,i] - target[b,c,j])^2        (Soft-DTW's own cost)
 *     squared == 0:  cost[b,i,j] = scale sqrt(sum_c (pred[b,c,i] - target[b,c,j])^2)       (the distance MCD-DTW averages)
 *
 *     dpred[b,c,i]   =  k sum_j G[b,i,j] (pred[b,c,i] - target[b,c,j])      k = (2 scale) row_scale[b], rounded once
 *     dtarget[b,c,j] = -k sum_i G[b,i,j] (pred[b,c,i] - target[b,c,j])      (row_scale null: k = 2 scale)
 *
 * The backward calls are those of the squared cost; the root has none (it needs the finished table and is singular at
 * distance 0).  Per cell d = target - pred and acc = fma(d, d, acc) over the channels in order, the direct form on the
 * vector ALU: the error is relative to the distance itself, not to the norms.  The dense and the band call run the
 * same operations in the same order, so the band table has the dense table's bits on the cells that exist.  G is
 * masked by "the cell exists" before it is multiplied, and pred rows / target columns are taken from inside the
 * lengths: a NaN in G where no cell exists, or in pred / target past the lengths, reaches nothing.  pred and target
 * inside the lengths must be such that their differences are finite.  No atomics, no workspace; the same bits on
 * every call, and each gradient has the bits it has beside the other.
 */
int aligner_l2_cost_f32(const float *pred_dev, const float *target_dev, const int32_t *n_dev, const int32_t *m_dev,
                        int bandwidth, float scale, int squared, float *cost_out_dev,
                        int B, int C, int N, int M, void *hip_stream);
int aligner_l2_cost_backward_f32(const float *grad_cost_dev, const float *pred_dev, const float *target_dev,
                                 const int32_t *n_dev, const int32_t *m_dev, int bandwidth, float scale,
                                 const float *row_scale_dev, float *dpred_out_dev, float *dtarget_out_dev,
                                 int B, int C, int N, int M, void *hip_stream);
int aligner_l2_cost_banded_f32(const float *pred_dev, const float *target_dev, const int32_t *n_dev, const int32_t *m_dev,
                               int bandwidth, float scale, int squared, float *cost_band_out_dev,
                               int B, int C, int N, int M, void *hip_stream);
int aligner_l2_cost_banded_backward_f32(const float *grad_band_dev, const float *pred_dev, const float *target_dev,
                                        const int32_t *n_dev, const int32_t *m_dev, int bandwidth, float scale,
                                        const float *row_scale_dev, float *dpred_out_dev, float *dtarget_out_dev,
                                        int B, int C, int N, int M, void *hip_stream);

/*
 * Hard DTW: the minimum-cost warping path between two frame sequences, with its backtrack -- the hard counterpart of
 * aligner_soft_dtw_f32 / aligner_soft_dtw_banded_f32 (the gamma -> 0 limit, which those calls cannot take), and what an
 * MCD-DTW or L1-along-the-path evaluation needs.  Build-defined.  For utterance b take n = n_dev[b], m = m_dev[b],
 * clamped as the soft calls clamp them, a warp penalty p (finite, >= 0) and a band w.  Cell (i,j) exists iff i < n,
 * j < m and |i - j| <= w.  All in fp32, in exactly this order:
 *
 *     a = R[i-1,j-1]                 (R[-1,-1] = 0; every other border cell +inf)
 *     b = R[i-1,j] + p
 *     c = R[i,j-1] + p
 *     best = a, k = 0;  if (b < best) { best = b; k = 1 }   if (c < best) { best = c; k = 2 }
 *     d = cost[i,j]
 *     R[i,j] = +inf            if the cell does not exist, or d is +inf or NaN, or best is +inf
 *            = best + d        otherwise
 *     value = R[n-1,m-1]
 *
 * Both comparisons are strict: a tie prefers the diagonal, then the move that advances the row, then the move that
 * advances the column.  A -inf cost is legal and propagates; nothing computes inf - inf.  The path starts at
 * (n-1,m-1), follows k until (0,0) and is reported in ascending order; its length K satisfies
 * max(n,m) <= K <= n+m-1.  An utterance without an alignment (a length below 1, |n - m| > w, a +inf value) has
 * value +inf, length 0 and a path of all -1.  No scaling and no sentinel: two additions and two comparisons per cell,
 * so value, path and length are functions of the costs' bits, the same in both storage forms.
 *   cost_dev       [B,N,M] fp32 contiguous (dense), or cost_band_dev [B,N,W] in band storage (above; m null: N)
 *   value_out_dev  [B] fp32
 *   path_out_dev   optional [B,L,2] int32, L = N+M-1 (dense) or 2N+w-1 (band storage): the K pairs (i,j), then -1
 *   length_out_dev [B] int32: K; null iff path_out_dev is
 *   ws_dev         aligner_dtw_path_workspace_bytes(B,N,M) / aligner_dtw_path_banded_workspace_bytes(B,N,bandwidth)
 *                  bytes (0: outside the domain): the decisions k, a byte a cell.  Needed (and written) only with a path;
 *                  without one only the forward kernel runs, and ws_dev may be null.
 * One workgroup per utterance in each launch (forward, then the backtrack: one wave follows the decisions through
 * windows of 64 rows staged in LDS), no atomics: the same bits on every call.  Domain: that of the soft call of the
 * same storage form (dense: N <= 1024, B <= 65535, N*M < 2^29; band storage: 0 <= bandwidth <= 127, B <= 65535,
 * N*W < 2^29): ALIGNER_EDOM beyond; ALIGNER_EINVAL for a null pointer, a shape below 1, a penalty that is negative or
 * not finite, a bandwidth below -1 (band storage: below 0); ALIGNER_ENOSPC for a workspace that is too small.
 * Validated before any HIP call.  Asynchronous on the stream, capturable.
 */
size_t aligner_dtw_path_workspace_bytes(int B, int N, int M);
int aligner_dtw_path_f32(const float *cost_dev, const int32_t *n_dev, const int32_t *m_dev,
                         float warp_penalty, int bandwidth,
                         float *value_out_dev, int32_t *path_out_dev, int32_t *length_out_dev,
                         void *ws_dev, size_t ws_bytes, int B, int N, int M, void *hip_stream);
size_t aligner_dtw_path_banded_workspace_bytes(int B, int N, int bandwidth);
int aligner_dtw_path_banded_f32(const float *cost_band_dev, const int32_t *n_dev, const int32_t *m_dev,
                                float warp_penalty, int bandwidth,
                                float *value_out_dev, int32_t *path_out_dev, int32_t *length_out_dev,
                                void *ws_dev, size_t ws_bytes, int B, int N, void *hip_stream);

/*
 * The cost kinds along a path: the cells of the cost tables above evaluated on the pairs of a warping path instead of
 * on a table, forward and backward -- what makes the hard path a loss (the gamma -> 0 limit of the soft losses) and an
 * evaluation along the path one call for the batch, with no cost table kept.  Build-defined.
 *   pred_dev [B,C,N], target_dev [B,C,M] fp32 contiguous, channels first; n_dev / m_dev optional [B] int32, clamped to
 *   N / M; path_dev [B,L,2] int32 and length_dev [B] int32 as aligner_dtw_path_f32 / aligner_dtw_path_banded_f32 write
 *   them (pairs ascending, L whatever the buffer has).  The features need not be those the path was found on.
 *   kind: ALIGNER_COST_L1, ALIGNER_COST_L2 (squared) or ALIGNER_COST_L2_ROOT.
 *
 * aligner_path_cost_f32.  pair_cost[b,k], k < length[b] (a length outside [0,L] is clamped), is the cell (i_k,j_k) of
 * aligner_l1_cost_f32 / aligner_l2_cost_f32 with the same scale, bit for bit: the same operations over the channels in
 * order.  A pair with i outside [0,n) or j outside [0,m) costs +inf and nothing is read for it; pair_cost[b,k] = 0 for
 * k >= length[b].  total_out_dev (optional [B]): the sum of the length[b] pair costs in a fixed order by one workgroup
 * per utterance, +inf for a length below 1.  No atomics: the same bits on every call.
 *
 * aligner_path_runs.  The pairs of a warping path with row i are consecutive in k, and so are those with column j.
 * row_start[b,i] is the index k of the first pair with row i and row_count[b,i] how many follow with that row (-1 and 0
 * for a row not on the path); col_start / col_count [B,M] alike; all int32.  valid[b] = 1 iff 0 <= length[b] <= L,
 * every pair k < length[b] lies in [0,N) x [0,M) and every step is (1,1), (1,0) or (0,1); an utterance that is not
 * valid has every count 0 and every start -1, and causes no access outside a buffer.  Every element is written, by one
 * writer.
 *
 * aligner_path_cost_backward_f32.  With the weights w_k = pair_weight_dev[b,k] ([B,L], null: all 1; not read at
 * k >= length[b]), g = row_scale_dev[b] (null: 1) and d_k,c = pred[b,c,i_k] - target[b,c,j_k]:
 *
 *     dpred[b,c,i]   =  factor sum over the pairs k of row i's run     of  w_k s(d_k,c)
 *     dtarget[b,c,j] = -factor sum over the pairs k of column j's run  of  w_k s(d_k,c)
 *     L1:       s = sign(d), sign(0) = 0                      factor = scale g
 *     L2:       s = d                                         factor = (2 scale) g
 *     L2_ROOT:  s = d / dist_k, dist_k = sqrt(sum_c d_k,c^2) as the forward computes it, s = 0 for every channel when
 *               dist_k == 0                                   factor = scale g
 *
 * The run is accumulated in k order and multiplied by the factor once.  The root kind forms the coefficient w_k / dist_k
 * per pair first (dist_k is 0 or at least 2^-74.5: finite for |w_k| < 2^53) and then runs L2's arithmetic with it.  Pairs
 * are read only inside [0,n) x [0,m), a pair outside contributes 0; rows, columns and utterances without pairs -- an
 * utterance aligner_path_runs calls not valid among them -- are written exactly 0 whatever row_scale holds.  One owner
 * per output element and no atomics: the same bits on every call, and each of dpred_out_dev [B,C,N] / dtarget_out_dev
 * [B,C,M] (either may be null, not both) has the bits it has beside the other.  ws_dev:
 * aligner_path_cost_backward_workspace_bytes(kind,B,N,M,L) bytes (0: outside the domain), 4-byte aligned: the runs and
 * the root kind's coefficients.
 *
 * Domain: B <= 65535, C <= 4096, L < 2^24: ALIGNER_EDOM beyond; ALIGNER_EINVAL for a null pointer, a shape below 1, an
 * unknown kind, a scale that is not finite; ALIGNER_ENOSPC for a workspace that is too small.  Validated before any HIP
 * call.  Asynchronous on the stream, capturable.
 */
#define ALIGNER_COST_L1      0
#define ALIGNER_COST_L2      1
#define ALIGNER_COST_L2_ROOT 2
int aligner_path_runs(const int32_t *path_dev, const int32_t *length_dev,
                      int32_t *row_start_out_dev, int32_t *row_count_out_dev,
                      int32_t *col_start_out_dev, int32_t *col_count_out_dev, int32_t *valid_out_dev,
                      int B, int L, int N, int M, void *hip_stream);
int aligner_path_cost_f32(const float *pred_dev, const float *target_dev, const int32_t *path_dev, const int32_t *length_dev,
                          const int32_t *n_dev, const int32_t *m_dev, int kind, float scale,
                          float *pair_cost_out_dev, float *total_out_dev,
                          int B, int C, int N, int M, int L, void *hip_stream);
size_t aligner_path_cost_backward_workspace_bytes(int kind, int B, int N, int M, int L);
int aligner_path_cost_backward_f32(const float *pair_weight_dev, const float *pred_dev, const float *target_dev,
                                   const int32_t *path_dev, const int32_t *length_dev,
                                   const int32_t *n_dev, const int32_t *m_dev, int kind, float scale,
                                   const float *row_scale_dev, float *dpred_out_dev, float *dtarget_out_dev,
                                   void *ws_dev, size_t ws_bytes, int B, int C, int N, int M, int L, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNER_AMD_H */
