/*
 * asr_hip.h — C ABI of libasr_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for
 * the seq2seq-ASR training hot path of jjery2243542/semi-supervised-ASR.
 *
 * The reference has no FFI: the path sits behind torch modules (model.py) that dispatch
 * stock operators.  Each entry point below names the reference operator call it replaces
 * (file:line into the reference) — that is the "interface" a maintainer would bind.
 *
 * Conventions (all entry points):
 *   - plain device pointers + explicit sizes; contiguous row-major fp32; int32 lengths;
 *     base pointers 16-byte aligned;
 *   - the CALLER allocates every buffer (outputs and workspaces); nothing is allocated,
 *     freed or synchronised inside; work is enqueued on `stream` (a hipStream_t);
 *   - return 0 on success, a negative ASR_E_* code for a bad argument, or a positive
 *     hipError_t if a launch failed.  Nothing throws across the ABI;
 *   - re-entrant; no global mutable state.
 *
 * Layout vocabulary:
 *   time-major      activations are [T][B][...] so one time step is one contiguous slab;
 *   gate-interleave the 4H gate axis is ordered unit-major: index = unit*4 + gate, gate in
 *                   (i,f,g,o) (torch order).  Host code permutes W_ih/W_hh/bias
 *                   rows once per step; a 4-unit slice of all four gates is 16 contiguous
 *                   floats (64 B).
 */
#ifndef ASR_HIP_H
#define ASR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASR_ABI_VERSION 8

#define ASR_E_ARG    (-1)  /* null pointer / non-positive size */
#define ASR_E_SHAPE  (-2)  /* size not supported by the kernel (see each function) */
#define ASR_E_ALIGN  (-3)  /* pointer or leading dimension not 16-byte aligned */

typedef void* asr_stream_t; /* hipStream_t */

int asr_abi_version(void);

/* Product arithmetic of the MFMA kernels: an explicit argument (`arith`) of asr_gemm_f32 and of the persistent LSTM
 * recurrences - there is no process-wide switch.  All operands, accumulators and results are fp32 in every mode; what
 * the mode selects is how a product x * y of two fp32 operands is formed:
 *   ASR_ARITH_F32     on the fp32-input MFMA (v_mfma_f32_32x32x2_f32 / 4x4x1): the exact fp32 product, 157 TF peak.
 *                     (In the persistent recurrences the RECURRENT operand - h_{t-1}, the exchanged partial sums - crosses
 *                     CUs as fp32 words whose mantissa LSB carries the hand-off's validity tag (csrc/persist.h): the
 *                     product is exact, that operand has 23 mantissa bits.  Worst cfg-2 / cfg-5 gradient element under
 *                     this mode: 1.7e-4 / 4.6e-5 of its tensor's scale.  asr_dec_seq_bwd_persist* take no arith argument: the
 *                     decoder kernels are exact fp32 throughout except the embedding part of dX, dgates W_cat[:, D+O:],
 *                     which they always form with bf16x6 products.)
 *   ASR_ARITH_BF16X6  fp32-equivalent on the bf16 MFMA: each operand is re-encoded LOSSLESSLY as three bf16 terms
 *                     (x = a + b + c exactly: 3 x 8 significand bits, every split rounded to nearest) and the six products
 *                     aa' + ab' + ba' + ac' + ca' + bb' are accumulated in fp32.  Dropped: bc' + cb' + cc' <= 2^-24 |x y|,
 *                     below the rounding of the fp32 product itself.  2.7x the fp32 pipe's MAC rate.  The host code's
 *                     default (hip_backend.ARITH).
 *   ASR_ARITH_BF16X3  two terms (16 significand bits), three products: <= 2^-15 relative per product.  Fastest, and NOT a
 *                     precision the reference has: OUTSIDE the 1e-3 parity gate on long recurrences (2.2e-3 on a sampled
 *                     layer-0 dW_ih element at cfg-5, 6.8e-4 at cfg-2; tests/test_big_configs_gpu.py holds it to 5e-3) -
 *                     never the default.
 * Flags OR-ed into `arith` select a kernel where several implement the same arithmetic (tests, measurements):
 *   ASR_GEMM_TILE_NARROW / ASR_GEMM_TILE_WIDE / ASR_GEMM_TILE_SP   asr_gemm_f32: only the 128 x 128 kernel / the 256 x 128
 *                     LDS-DMA kernel / the 256 x 128 one-wave-per-SIMD kernel for every conforming shape; by default
 *                     each is used for the shapes it pays on (csrc/gemm.hip: asr_gemm_f32);
 *   ASR_GEMM_TILE_SMALL   asr_gemm_f32: 64 x 64 tiles on the 128 x 128 kernel's code (by default for products whose large tiles,
 *                     K split included, would be at most one workgroup per CU: decoder-side projections, output layer);
 *   ASR_GEMM_C_ZEROED     asr_gemm_f32 / asr_gemm_drop_f32: a promise, not a selector - C holds zeros already (a slice of a
 *                     buffer the caller zeroes once per step), so a product the library splits over K needs no zero pass
 *                     of its own in front of the atomics.  Ignored with accumulate != 0.
 *   ASR_LSTM_BWD_GATHER   asr_lstm_seq_bwd_persist: the gathered-dG kernel instead of the one with exchanged partials.
 *   ASR_DEBUG_FAULT       asr_lstm_seq_fwd_persist (ASR_ARITH_BF16X6, H = 512 only; ASR_E_SHAPE otherwise): TESTS ONLY - the
 *                         FAULT instantiation of the kernel: slice 1 of group 0 stops publishing after its first step and
 *                         every wait gives up after 4 096 attempts, so the launch runs the kernels' own abort path (bounded
 *                         spin expires -> abort word + latch + code -> NaN poison -> every workgroup drains) in a
 *                         millisecond.  asr_dec_seq_fwd_persist_fault is the decoder's. */
#define ASR_ARITH_F32        0
#define ASR_ARITH_BF16X6     1
#define ASR_ARITH_BF16X3     2
#define ASR_ARITH_MASK       0xff
#define ASR_GEMM_TILE_NARROW 0x100
#define ASR_GEMM_TILE_WIDE   0x200
#define ASR_GEMM_TILE_SP     0x800
#define ASR_GEMM_TILE_SMALL  0x1000
#define ASR_GEMM_C_ZEROED    0x2000
#define ASR_LSTM_BWD_GATHER  0x400
#define ASR_DEBUG_FAULT      0x10000

/* ---------------------------------------------------------------------------------------
 * Dense fp32 GEMM on the MFMA (product arithmetic: `arith`, see above).
 *   C[M,N] (ldc) = op(A)[M,K] * op(B)[K,N]  (+ bias[N]) (relu) (+ C if accumulate)
 * Row-major.  transA=0: A is [M][K] (lda>=K); transA=1: A is [K][M] (lda>=M).
 *             transB=0: B is [K][N] (ldb>=N); transB=1: B is [N][K] (ldb>=K).
 * batch>1 runs `batch` independent GEMMs with element strides sA,sB,sC.
 * split_k <= 0: the library chooses a K split; split_k == 1: unsplit (no atomics: run-to-run deterministic);
 * split_k > 1 splits K over grid.z and accumulates with fp32 atomics (C is zero-filled on
 * the stream first unless accumulate!=0); with a K split, bias/relu are applied by a second
 * pass over C (not combinable with accumulate).  batch * split_k is grid.y: ASR_E_SHAPE above 65 535.
 * Replaces torch.nn.Linear / mm / bmm on the path: the LSTM input-gate product inside
 * torch.nn.LSTM (model.py:67-68,80), project_layer (model.py:93-94), mlp_enc
 * (model.py:144), output_layer (model.py:293) and every autograd mm behind them.
 * ------------------------------------------------------------------------------------- */
int asr_gemm_f32(int transA, int transB, int64_t M, int64_t N, int64_t K,
                 const float* A, int64_t lda, const float* B, int64_t ldb,
                 float* C, int64_t ldc, const float* bias, int relu, int accumulate,
                 int batch, int64_t sA, int64_t sB, int64_t sC, int split_k, int arith,
                 asr_stream_t stream);
/* C = dropout(act(op(A) op(B) + bias)): asr_gemm_f32 (batch 1, no accumulate) followed by the seeded mask of
 * asr_dropout_seeded_f32 over the element index m N + n of C (project_layer -> relu -> dropout, model.py:93-95): in the
 * bias / ReLU pass where the product was split over K, in a pass of its own otherwise. */
int asr_gemm_drop_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                      const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, int relu, int split_k,
                      int arith, uint64_t seed, float p, asr_stream_t stream);

/* What asr_gemm_f32 / asr_gemm_drop_f32 decide for a call before they launch anything (csrc/gemm.hip: plan_gemm): the kernel
 * family and its template choices, the K split as it will run, the grid, and the passes in front of and behind the product.
 * tests/golden/gemm_plan.json.gz pins it per call. */
#define ASR_GEMM_FAMILY_F32 0 /* gemm_f32_kernel<AKC, BKC> */
#define ASR_GEMM_FAMILY_BF3 1 /* gemm_bf3_kernel<AKC, BKC, terms, tile, queue>: 128 x 128 or 64 x 64 tiles */
#define ASR_GEMM_FAMILY_BFW 2 /* gemm_bf6w_kernel (terms 3) / gemm_bf3w_kernel (terms 2) <AKC, BKC>: 256 x 128, LDS-DMA */
#define ASR_GEMM_FAMILY_BFS 3 /* gemm_bfs_kernel<AKC, BKC, terms, kt>: 256 x 128, one wave per SIMD */
#define ASR_GEMM_FAMILY_BFK 4 /* gemm_bfk_kernel<terms, 5, plain>: K = 80, weights stationary */
#define ASR_GEMM_BEHIND_EPILOGUE 1 /* the pass behind the product applies bias / ReLU (a product split over K) */
#define ASR_GEMM_BEHIND_DROPOUT  2 /* ... and / or the seeded dropout mask */
typedef struct {
  int family;              /* ASR_GEMM_FAMILY_* */
  int terms;               /* bf16 terms per operand: 3 (ASR_ARITH_BF16X6), 2 (ASR_ARITH_BF16X3), 0 (ASR_ARITH_F32) */
  int tile;                /* rows of an output tile: 128, 64, or 256 for the 256 x 128 kernels */
  int akc, bkc;            /* operand layouts: k contiguous (A: !transA, B: transB) */
  int kt, plain, queue;    /* template choices: masked K tail (BFS), branch-free epilogue (BFK), ticket queue (asr_gemm_side_f32) */
  int split_k;             /* K slices as they will run */
  int tiles_m, tiles_n, groups;      /* (groups: workgroups that walk down the M tiles of one column of tiles, BFK) */
  unsigned grid[3], block;           /* the product's launch, in workgroups / threads */
  unsigned pass_grid[3];             /* the zero pass and the pass behind (256 threads) */
  int zero_pass;           /* zero_rows_kernel runs in front of the product */
  int behind;              /* ASR_GEMM_BEHIND_* carried by bias_act_kernel behind it; 0: no such pass */
} asr_gemm_plan_t;
/* Arguments as asr_gemm_f32, without the stream; has_drop: the call is asr_gemm_drop_f32 with p > 0.  Returns what that call
 * would return before it launches (0, ASR_E_ARG, ASR_E_SHAPE).  The pointers are looked at for NULL and 16-byte alignment
 * only, never dereferenced: no GPU is needed. */
int asr_gemm_plan(int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B,
                  int64_t ldb, const float* C, int64_t ldc, const float* bias, int relu, int accumulate, int batch,
                  int64_t sA, int64_t sB, int64_t sC, int split_k, int arith, int has_drop, asr_gemm_plan_t* plan);

/* C[b] += op(A[b]) op(B[b]) on the XCDs of `xcd_mask` only (bit x = XCC id x), by workgroups built to run BESIDE the
 * persistent XCD-local kernels below: a batch of <= 8 utterances keeps the LSTM / decoder recurrences on four of the eight
 * XCDs (group g of a persistent launch = XCC id g; groups without rows leave at once), and the weight-gradient products
 * (the autograd mm's of torch.nn.LSTM / Linear behind model.py:67-68,93-94,262-263 - off the backward's critical path) run
 * on the other four, issued on a side stream under the recurrence of the layer below.  64 x 64 tiles, <= 128 VGPRs and 30 KB
 * of LDS (a workgroup fits next to a persistent one on a CU, so no persistent launch waits for room), one (tile, K slice)
 * per workgroup drawn from the ticket counter `queue` (ONE zeroed 32-bit word of the caller's, consumed by the call).  The
 * K slices are ADDED to C with atomics: C holds zeros for a plain product.  Arguments as asr_gemm_f32 (strides in elements,
 * negative batch strides allowed); arith: ASR_ARITH_BF16X6 / _BF16X3 (ASR_E_SHAPE for ASR_ARITH_F32: the caller runs
 * asr_gemm_f32 instead).  The result does not depend on where the hardware places workgroups (a second, unmasked launch
 * draws whatever tickets the masked one left).  ASR_E_SHAPE when batch * K slices exceeds 65 535 (grid.y) or the masked
 * launch would have 2^32 workgroups or more. */
int asr_gemm_side_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                      const float* B, int64_t ldb, float* C, int64_t ldc, int batch, int64_t sA, int64_t sB, int64_t sC,
                      int arith, unsigned xcd_mask, unsigned* queue, asr_stream_t stream);

/* Skinny GEMM for the sequential chains (M = batch rows, tens not thousands):
 *   C[M,N] (ldc) (+)= A[M,K] (lda) * Bt[N,K]^T (ldb)  (+ bias[N]) (* mask[M,N] from col mask_from)
 * 16 output columns per workgroup, K split over the 4 waves, 16x16x4 f32 MFMA.
 * K % 16 == 0, lda/ldb % 4 == 0.  Replaces mlp_dec (model.py:163), output_layer per step
 * (model.py:293) and the dX products of LSTMCell/mlp_dec backward. */
int asr_gemm_skinny_f32(int64_t M, int64_t N, int64_t K,
                        const float* A, int64_t lda, const float* Bt, int64_t ldb,
                        float* C, int64_t ldc, const float* bias, int accumulate,
                        const float* mask, int64_t ldmask, int64_t mask_from,
                        asr_stream_t stream);

/* Column sums: out[N] (+)= sum_m X[m][n]   (bias gradients). */
int asr_colsum_f32(int64_t M, int64_t N, const float* X, int64_t ldx, float* out,
                   int accumulate, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Fused LSTM sequence, all time steps of one layer, both directions in one call.
 * Replaces torch.nn.LSTM(bidirectional) on a PackedSequence + pad_packed_sequence
 * (model.py:79-81) and the 2-layer judge LSTM (model.py:466-467,515-519) — restated as a
 * masked recurrence on the padded time-major tensor: at t >= lens[b] the
 * state and the output are 0.
 *
 *   gates [T][B][ndir][4H]  in : x_t W_ih^T + b_ih + b_hh, gate-interleaved
 *                           out: activated gates (i,f,g,o) — saved for backward
 *   w_hh  [ndir][4H][H]     rows gate-interleaved
 *   lens  [B] int32 (device)
 *   y     [T][B][ndir*H]    hidden states; direction d occupies columns [d*H,(d+1)*H)
 *   c     [T][B][ndir*H]    cell states (saved for backward)
 * B is the batch STRIDE of the buffers, nb <= B the number of rows this call processes: utterances are
 * independent, so a caller may run disjoint row groups (pointers pre-offset to the group's first row)
 * concurrently on different streams to overlap the latency-bound chains.
 * Direction 0 runs t = 0..T-1, direction 1 (if ndir==2) runs t = T-1..0.
 * One kernel launch per time step covers both directions: workgroup = (4 hidden units x
 * 4 gates = 16 gate rows) x (<=32 batch rows); h_{t-1} W_hh^T on the 16x16x4 f32 MFMA
 * with K split over the 4 waves, partials reduced through LDS, then sigmoid/tanh/state
 * update.  H % 16 == 0.
 *
 * PACKED ROWS (ABI 4; rowbase / rowext, both NULL = the time-major layout above).  pack_padded_sequence spares the
 * reference's LSTM the padded frames (model.py:79-81); here the whole encoder runs without them: batch row b owns the
 * rows rowbase[b] .. rowbase[b] + rowext[b] - 1 of gates / y / c / dy (then [R][ndir][4H] and [R][ndir*H], R = the sum
 * of the extents), time t at row rowbase[b] + t.  lens[b] < rowext[b]: the rows lens[b] .. rowext[b] - 1 are padding
 * INSIDE the block - the kernels write y = c = 0 (forward) and dG = 0 (backward) there, as they do for the padded times
 * of the time-major layout, also behind the T steps of the call (T >= max lens suffices) - and times >= rowext[b] do not
 * exist (nothing is read into a result or written).  With at
 * least one padding row behind every utterance the products that pair a row with its time neighbour (dW_hh = sum_t
 * dG_t^T h_{t-1}) stay ONE row-shifted GEMM over all R rows: the neighbour across a block boundary is a zero row.
 * Blocks whose extents halve from layer to layer (rowext_l = 2 rowext_{l+1}) make the pyramid's pair-concat the
 * B = 1 case of asr_pyramid_concat_* over the R rows.  rowbase / rowext: int32 [B] on the device.
 * ------------------------------------------------------------------------------------- */
int asr_lstm_seq_fwd(int T, int B, int nb, int H, int ndir, float* gates, const float* w_hh,
                     const int32_t* lens, const int32_t* rowbase, const int32_t* rowext, float* y, float* c,
                     asr_stream_t stream);

/* Persistent fast path of asr_lstm_seq_fwd (same arguments and results; csrc/lstm_persist.hip): ONE launch runs
 * all T steps, each XCD owns a (direction, 8- or 4-row) group, W_hh stays in registers, h_t is exchanged inside the
 * XCD as LSB-tagged fp32 words.  Applies when H is 128, 256, 320, 512 (or 640 with a bf16 arithmetic) on an 8 x 32-CU
 * device, any nb (row blocks of 32 * (8 / ndir) run as consecutive launches; at H = 512 under the bf16 arithmetics every
 * block of 64 * (8 / ndir) rows runs 16 rows per group in one launch); otherwise returns ASR_E_SHAPE and the
 * caller uses asr_lstm_seq_fwd.  `arith`: product arithmetic of h W_hh^T (ASR_ARITH_*, see above).
 * xch and ctrl are caller-allocated scratch shared by ALL persistent entry points (LSTM and decoder): at least
 * asr_persist_scratch_bytes() says (10 MB of exchange - the H = 640 backward's partial sums are the largest user - and a
 * 128-byte control block); smaller buffers are silently overrun by the pre-launch zero fill and the kernels' atomics.
 * ctrl = [16 latch words | 16 per-launch words]: the
 * per-launch words and the used part of xch are zeroed on the stream before every launch (one fill when ctrl sits exactly
 * 128 bytes in front of xch, else two).  A kernel that aborts (bounded spin expired / unexpected placement) poisons its
 * outputs with NaN and sets per-launch word 8 (code in word 9) AND latch word 0 (code in latch word 1).  The library
 * never clears the latch words: a sequence operator is several launches, and the caller looks once, after the last
 * one, and clears the latch itself. */
int asr_persist_scratch_bytes(int64_t* xch_bytes, int64_t* ctrl_bytes);   /* minimum sizes of the scratch pair; returns 0 */
/* rowbase / rowext: packed rows (see asr_lstm_seq_fwd), NULL = time-major.  With packed rows T is the number of STEPS to
 * run, at least the longest of the nb rows (it may be less than their extents: the kernels zero a block's padding rows
 * behind the last step themselves).  lens_host: optional HOST copy of lens (packed rows only): every row block then runs
 * max(lens of its rows) steps instead of T (a batch of 256 length-sorted utterances on one GPU: the later blocks are
 * shorter). */
int asr_lstm_seq_fwd_persist(int T, int B, int nb, int H, int ndir, float* gates, const float* w_hh,
                             const int32_t* lens, const int32_t* rowbase, const int32_t* rowext,
                             const int32_t* lens_host, float* y, float* c, void* xch, void* ctrl, int arith,
                             asr_stream_t stream);

/* Backward through the same recurrence.
 *   gates [T][B][ndir][4H]  in : activated gates from the forward; out: dL/d(pre-activation)
 *                           (= gradient of the x-projection, gate-interleaved)
 *   w_hhT [ndir][H][4H]     transpose of the gate-interleaved w_hh
 *   dy    [T][B][ndir*H]    upstream gradient of y
 *   c     forward cell states;  dcarry [B][ndir*H] zero-initialised scratch (dL/dc carry)
 * dW_hh is NOT produced here: the caller forms sum_t dG_t^T h_{t-1} with one asr_gemm_f32
 * (transA=1) over the whole sequence after this call. */
int asr_lstm_seq_bwd(int T, int B, int nb, int H, int ndir, float* gates, const float* w_hhT,
                     const int32_t* lens, const int32_t* rowbase, const int32_t* rowext, const float* dy, const float* c,
                     float* dcarry, asr_stream_t stream);
/* Persistent fast path of asr_lstm_seq_bwd (same conditions / scratch / abort convention as asr_lstm_seq_fwd_persist;
 * H in {128, 256, 320, 512}, and 640 under ASR_ARITH_BF16X6).  With a bf16 arithmetic and H in {128, 256, 512} - and
 * H = 320 (10 units per CU in 12 slots) / H = 640 (20 units per CU, its own kernel) under ASR_ARITH_BF16X6 - the CUs of a
 * group exchange partial sums of dh_rec, laid out [8 groups][2][32 dest][32 src]
 * [8 rows][slots per CU] floats in xch (8 MB at H = 512); otherwise (H = 320 with two terms, ASR_ARITH_F32,
 * ASR_LSTM_BWD_GATHER) every CU gathers the step's dG tile: one kernel, lstm_persist_bwd_kernel, whose product dG W_hh
 * takes fp32 operands or operands split in two / three bf16 terms.  Exchanged words carry a 1-bit tag in the
 * mantissa LSB; the in-place dG is what the pointwise update produced.  `arith` selects the product arithmetic of
 * dG W_hh and of the fused dW_hh (the gathered-dG kernel always forms dW_hh on the fp32 MFMA).
 * If y (forward hidden states) and dw_hh ([ndir][4H][H], gate-interleaved, zero-filled or holding a running sum)
 * are given, the recurrent weight gradient sum_t dG_t^T h_{t-1} is accumulated into dw_hh inside the kernel
 * (fp32 atomics across the row groups) and the caller skips that GEMM.  If db ([ndir][4H], gate-interleaved,
 * zero-filled) is given, the bias gradient sum_{t,b} dG is accumulated into it as well.
 * With packed rows (rowbase / rowext / lens_host as in asr_lstm_seq_fwd_persist) y / dw_hh are ignored: dW_hh is the
 * caller's row-shifted product over all R rows. */
int asr_lstm_seq_bwd_persist(int T, int B, int nb, int H, int ndir, float* gates, const float* w_hhT,
                             const int32_t* lens, const int32_t* rowbase, const int32_t* rowext,
                             const int32_t* lens_host, const float* dy, const float* c, const float* y,
                             float* dw_hh, float* db, void* xch, void* ctrl, int arith, asr_stream_t stream);
/* Does asr_lstm_seq_bwd_persist(_w) with this (H, arith) accumulate dW_hh itself when given y and dw_hh?  1 yes; 0 no -
 * the ASR_ARITH_BF16X6 exchanged-partials kernels (H in {128, 256, 320, 512, 640}) leave dW_hh = sum_t dG_t^T h_{t-1} to the caller
 * (one batched asr_gemm_f32 over the two directions: with six products per product the fused form costs more time on the
 * kernel's serial chain than the GEMM does) and ignores y / dw_hh; -1 no persistent backward for this H / arith.  The
 * bias gradient db is accumulated by every persistent backward kernel. */
int asr_lstm_bwd_persist_fuses_dw(int H, int arith);
/* asr_lstm_seq_bwd_persist with W_hh in the FORWARD layout (w_hh_il [ndir][4H][H], gate-interleaved: the array
 * asr_lstm_seq_fwd_persist consumed) instead of its transpose: the exchanged-partials kernel reads its slice once per
 * launch.  Returns ASR_E_SHAPE where that kernel does not apply; the caller then forms w_hhT and calls
 * asr_lstm_seq_bwd_persist / asr_lstm_seq_bwd. */
int asr_lstm_seq_bwd_persist_w(int T, int B, int nb, int H, int ndir, float* gates, const float* w_hh_il,
                               const int32_t* lens, const int32_t* rowbase, const int32_t* rowext,
                               const int32_t* lens_host, const float* dy, const float* c, const float* y, float* dw_hh,
                               float* db, void* xch, void* ctrl, int arith, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The two ends of the packed-row encoder (csrc/rows.hip).  C % 4 == 0; lens / rowbase / rowext int32 [B] on the device;
 * ext_max = max_b rowext[b] (host).
 *   asr_rows_pack_f32        x [B][T][C], the collated batch (dataloader.py:6-12) -> rows [R][C]: row rowbase[b] + t =
 *                            x[b][t] for t < lens[b], zeros for lens[b] <= t < rowext[b]
 *   asr_rows_unpack_fwd_f32  rows [R][C] -> out [B][T][C] (the encoder output the decoder reads, model.py:109-112):
 *                            out[b][t] = rows[rowbase[b] + t] for t < lens[b]; the frames behind an utterance hold what the
 *                            reference's last projection makes of an all-zero frame, dropout(relu(bias)) (model.py:93-95,
 *                            SURVEY F2): fill [C] (NULL = zeros) times the dropout mask - `mask` [B][T][C] given, or
 *                            regenerated from (seed, p) over the element index of out (asr_dropout_seeded_f32; p = 0: none).
 *                            fill_relu != 0: `fill` is the projection's bias itself and the kernel takes relu(fill)
 *   asr_rows_unpack_bwd_f32  drows[rowbase[b] + t] = dout[b][t] for t < lens[b], zeros on the block's padding rows;
 *                            dfill [C] (NULL, or zero-filled by the caller) += sum of dout * mask over the padded frames
 *                            (relu_of != NULL: only where relu_of[c] > 0 - the gradient of the bias behind that relu)
 * ------------------------------------------------------------------------------------- */
int asr_rows_pack_f32(int B, int T, int C, const float* x, const int32_t* lens, const int32_t* rowbase,
                      const int32_t* rowext, int ext_max, float* rows, asr_stream_t stream);
int asr_rows_unpack_fwd_f32(int B, int T, int C, const float* rows, const int32_t* lens, const int32_t* rowbase,
                            const float* fill, int fill_relu, const float* mask, uint64_t seed, float p, float* out,
                            asr_stream_t stream);
int asr_rows_unpack_bwd_f32(int B, int T, int C, const float* dout, const int32_t* lens, const int32_t* rowbase,
                            const int32_t* rowext, int ext_max, const float* mask, uint64_t seed, float p, float* drows,
                            float* dfill, const float* relu_of, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Pyramidal pair-concat (model.py:85-92), time-major:
 *   in [T][B][C] -> out [ceil(T/2)][B][2C], out[t'] = [in[2t'] | in[2t'+1]]; for odd T the
 *   missing last frame replicates in[T-1].  Optional elementwise mask (dropout, already
 *   scaled by 1/(1-p)) of the input shape is applied on the fly.  float4 coalesced.
 * Backward: din[t] = dout[t/2][.., (t%2)*C ..] (* mask), the replicated frame's gradient
 * folded into din[T-1].
 * ------------------------------------------------------------------------------------- */
int asr_pyramid_concat_fwd(int T, int B, int C, const float* in, const float* mask,
                           float* out, asr_stream_t stream);
int asr_pyramid_concat_bwd(int T, int B, int C, const float* dout, const float* mask,
                           float* din, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Counter-based dropout (the shared torch.nn.Dropout of model.py:73,82,95): inverted dropout whose mask is a pure
 * function of (seed, flat element index), mask(i) = [hash(seed, i) >= p * 2^32] / (1 - p), so nothing is stored
 * between forward and backward.  p in [0, 1); n % 4 == 0; pointers 16-byte aligned.
 *   asr_dropout_seeded_f32      x[i] *= mask(i), in place (after relu(x W^T + b), model.py:94-95)
 *   asr_relu_dropout_bwd_f32    out[i] = grad[i] * mask(i) * (y[i] > 0), y = the dropped-out relu output
 *   asr_dropout_mask_f32        mask[i] = mask(i) (tests; the decoder's [L][B][O+E] operand mask)
 *   asr_pyramid_concat_*_seeded the pair-concat kernels with mask(i) over the [T][B][C] input regenerated in flight
 * ------------------------------------------------------------------------------------- */
int asr_dropout_seeded_f32(int64_t n, float* x, uint64_t seed, float p, asr_stream_t stream);
int asr_relu_dropout_bwd_f32(int64_t n, const float* grad, const float* y, uint64_t seed, float p, float* out,
                             asr_stream_t stream);
int asr_dropout_mask_f32(int64_t n, float* mask, uint64_t seed, float p, asr_stream_t stream);
int asr_pyramid_concat_fwd_seeded(int T, int B, int C, const float* in, uint64_t seed, float p, float* out,
                                  asr_stream_t stream);
int asr_pyramid_concat_bwd_seeded(int T, int B, int C, const float* dout, uint64_t seed, float p, float* din,
                                  asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Decoder step = LSTMCell + location-aware attention (Decoder.forward_step model.py:283-294,
 * AttLoc.forward model.py:139-173).  Per-sequence constants:
 *   P   [B][Tp][A]   mlp_enc(enc_h)                     (model.py:144)
 *   Q   [B][Tp][O]   enc_h W_o^T  — mlp_o hoisted out of the step loop by linearity:
 *                    mlp_o(sum_t w_t h_t) = sum_t w_t (W_o h_t) + b_o   (model.py:171-172)
 *   X   [L+1][B][KX] step inputs, KX = D + O + E: X[s] = [ z_{s-1} | ctx_{s-1} | emb_s ]
 *                    (cell_inp of model.py:284 plus the recurrent z); the step writes z_s
 *                    and ctx_s into X[s+1].
 *   wcat [4D][KX]    [W_hh | W_ih(ctx cols) | W_ih(emb cols)], rows gate-interleaved
 *   bcat [4D]        b_ih + b_hh, gate-interleaved
 * asr_dec_step_fwd(s) enqueues: fused cell (skinny MFMA gate GEMM + activations), mlp_dec
 * skinny GEMM, attention score kernel (201-tap location conv, tanh energy), softmax +
 * context kernel.  Softmax runs over ALL Tp frames with temperature `scaling` (SURVEY
 * F1/F4).  w_prev for s==0 is the caller-provided uniform-over-valid-frames row block.
 * Saved for backward: gates[s], cstate[s], S[s] (tanh values), fconv[s], ws[s], energies.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  int B, nb, Tp, A, D, O, E, C, K; /* B = batch stride of every buffer, nb <= B rows processed by this call
                                       (pointers pre-offset to the group's first row); K = conv half width */
  int L;                        /* number of steps buffers are sized for */
  float scaling;
  /* per-sequence inputs */
  const float* P;     /* [B][Tp][A] */
  const float* Q;     /* [B][Tp][O] */
  const float* bo;    /* [O] mlp_o bias */
  const float* wcat;  /* [4D][KX] */
  const float* bcat;  /* [4D] */
  const float* wdec;  /* [A][D]  mlp_dec.weight */
  const float* convw; /* [C][2K+1] loc_conv.weight */
  const float* watt;  /* [A][C]  mlp_att.weight */
  const float* wattT; /* [C][A]  its transpose (prepared by the caller once per sequence) */
  const float* gvec;  /* [A] */
  const float* w0;    /* [B][Tp] initial attention weights (model.py:151-153) */
  const float* xmask; /* [L][B][O+E] dropout mask for the (ctx|emb) part of X[s], or NULL */
  /* state / saved buffers */
  float* X;       /* [L+1][B][KX] */
  float* Xd;      /* [L+1][B][KX] dropout-masked copy of X (the cell's operand) when xmask != NULL, else NULL;
                     the caller fills its emb columns, the kernels fill z and ctx*mask */
  float* gates;   /* [L][B][4D] */
  float* cstate;  /* [L][B][D] */
  float* Dproj;   /* [L][B][A]   mlp_dec(z_s) */
  float* fconv;   /* [L][B][C][Tp] */
  float* S;       /* [L][B][Tp][A] */
  float* energy;  /* [L][B][Tp] */
  float* ws;      /* [L][B][Tp] attention weights */
} asr_dec_fwd_t;

int asr_dec_step_fwd(const asr_dec_fwd_t* p, int s, asr_stream_t stream);
/* attention part of step s only (AttLoc.forward model.py:139-173): z is read from X[s+1][:,0:D]; writes
 * mlp_o(context) to X[s+1][:,D:D+O] and the weights to ws[s] */
int asr_att_step_fwd(const asr_dec_fwd_t* p, int s, asr_stream_t stream);
int asr_dec_seq_fwd(const asr_dec_fwd_t* p, int s_begin, int s_end, asr_stream_t stream);
/* Persistent fast path of asr_dec_seq_fwd(p, 0, L): all L teacher-forced steps in one launch per 32 rows (each XCD
 * owns 4 utterances; W_cat, W_dec and the P slice stay in registers, exchanges stay in the XCD's L2).  Same results
 * except that Dproj is not written.  Returns ASR_E_SHAPE (-2) when it does not apply (see the table; not an 8 x 32-CU
 * device): use asr_dec_seq_fwd.
 * xch and ctrl: the scratch pair of asr_lstm_seq_fwd_persist (sizes: asr_persist_scratch_bytes(); the decoder kernels
 * zero up to 3.6 MB of xch and use all 128 bytes of ctrl); abort convention as asr_lstm_seq_fwd_persist.
 *
 * ACCEPTED RANGES of the decoder sequence entry points.  C = conv channels, K = conv half width (2K + 1 taps), T' = Tp =
 * encoder frames, T'p = T' rounded up to a multiple of 4, V = vocabulary; every persistent entry point also wants
 * (D,A,O,E) = (512,512,512,128) or (320,320,320,128).  Outside its range a persistent entry point returns ASR_E_SHAPE
 * and the caller takes the per-step one; tests/test_decoder_shapes_gpu.py runs both sides of every limit below.
 *
 *   entry point                         C        K        T'                                   V
 *   asr_dec_step/seq_fwd (per step)     1..16    >= 0     any                                  -
 *   asr_dec_step/seq_bwd (per step)     1..16    >= 0     any                                  -
 *   asr_dec_feedback_fwd / _bwd         -        -        -                                    1..128
 *   asr_dec_seq_fwd_persist             1..12    0..100   4 rows per group (32 per launch): T' <= 128 and C T'p <= 1024;
 *                                                         else 2 rows per group (16 per launch): T' <= 256 and
 *                                                         C T'p <= 3072                        -
 *   asr_dec_seq_fwd_persist_free        as asr_dec_seq_fwd_persist                             1..64
 *   asr_dec_seq_fwd_persist_fault       as asr_dec_seq_fwd_persist, (512,512,512,128) and the 4-row geometry only
 *   asr_dec_seq_bwd_persist             1..16    0..100   4 rows per group: T' <= 128 and C T'p <= 1024; else 2 rows per
 *                                                         group: T' <= 256, C T'p <= 2560 and an LDS plan (a function of
 *                                                         T', C, K and V) of at most 160 KB    -
 *   asr_dec_seq_bwd_persist_free        as asr_dec_seq_bwd_persist, E = 128                    1..36
 *
 * At 10 channels the 4-row geometry ends at T' = 100 and the 2-row one at T' = 256 in both directions; at 8 or fewer the
 * 4-row geometry reaches its full T' = 128.  At 12 channels the forward is persistent up to T' = 256 and the backward up
 * to T' = 212; at 13..16 channels only the backward is persistent (4 rows up to C T'p = 1024, 2 rows up to 2560).  With
 * V = 37..64 a free-running smooth sequence has a persistent forward and the per-step backward + asr_dec_feedback_bwd. */
int asr_dec_seq_fwd_persist(const asr_dec_fwd_t* p, void* xch, void* ctrl, asr_stream_t stream);
/* TESTS ONLY: asr_dec_seq_fwd_persist on the FAULT instantiation of its kernel (see ASR_DEBUG_FAULT): the launch aborts by
 * itself within a millisecond.  cfg-2 widths (512, 512, 512, 128) in the 4-row geometry (T' <= 128 and C T'p <= 1024:
 * T' <= 100 at 10 conv channels); ASR_E_SHAPE otherwise. */
int asr_dec_seq_fwd_persist_fault(const asr_dec_fwd_t* p, void* xch, void* ctrl, asr_stream_t stream);
/* Free-running variant (greedy / smooth-embedding decode, model.py:334-341; solver.py:230-231,466-470): the embedding
 * input of step s >= 1 is made inside the kernel from the logits of step s-1: mode 1 = emb[argmax], mode 2 =
 * softmax(scaling * logits) @ emb.  The caller fills X[0] / Xd[0] (embedding columns of <BOS>) and fed[0].  Written:
 * logits[s] [B][V] and pred[s] [B] (int64) for s < L-1; fed[s] [B] (int64, -1 in mode 2) and the embedding columns of
 * X[s] / Xd[s] for 1 <= s < L; probs[s] [B][V] for s < L-1 (mode 2, for the backward).  The last step's logits / pred
 * come from asr_dec_feedback_fwd(mode 3) on X[L].  V <= 64.  Same applicability rule, scratch and abort convention as
 * asr_dec_seq_fwd_persist. */
typedef struct {
  int mode;
  int V;
  int eos;             /* >= 0: a group of 4 utterances stops once each has emitted this token (decoding without a
                          backward: solver.py:212-242 strips everything after the first <EOS> anyway); the caller
                          pre-fills pred / logits of the steps that are then not run.  -1: run all L steps. */
  float scaling;
  const float* w_out;  /* [V][D+O] */
  const float* b_out;  /* [V] or NULL */
  const float* emb;    /* [V][E] */
  float* logits;       /* [L][B][V] */
  float* probs;        /* [L-1][B][V], mode 2 */
  int64_t* pred;       /* [L][B] */
  int64_t* fed;        /* [L][B] */
  /* scheduled sampling (mode 1, eos = -1; Decoder.forward with ys and tf_rate < 1, model.py:328-333): step s >= 1 is fed
   * tokens[b][s] where teacher[s] != 0 (the host's per-step draw) and its own argmax elsewhere; NULL: never the teacher */
  const int64_t* tokens;        /* [B][ld_tokens], ld_tokens >= L, or NULL */
  int64_t ld_tokens;
  const unsigned char* teacher; /* [L] */
} asr_dec_feedback_t;
int asr_dec_seq_fwd_persist_free(const asr_dec_fwd_t* p, const asr_dec_feedback_t* f, void* xch, void* ctrl,
                                 asr_stream_t stream);

/* Backward of one decoder step (reverse order s = L-1..0).
 *   G     [L+1][B][KX]  gradient wrt X; on entry G[s+1][:, 0:D+O] holds every other
 *                       contribution to d(z_s, ctx_s) (output layer); the step adds its own
 *                       and accumulates dX[s] into G[s].
 *   dwext [C][B][Tp]    partial d(w_s) coming from step s+1's location conv (in: consumed,
 *                       out: overwritten with step s's partials for step s-1).  Zero it
 *                       before the first (s = L-1) call.
 *   dws   [L][B][Tp]    optional upstream gradient of the returned attention weights
 *   dP    [B][Tp][A]    accumulated (+=);  dQw: dQ is formed by the caller as a batched
 *                       GEMM of ws and dctx after the loop.
 *   dgates[L][B][4D], dD [L][B][A]  saved per step for the deferred weight-gradient GEMMs
 *   dgvec_part [B][A], dwatt_part [B][A][C], dconv_part [B][C][2K+1]: per-utterance
 *                       partial sums accumulated over steps (caller zero-fills, reduces
 *                       over B afterwards).
 *   wcatT [KX][4D], wdecT [D][A]: transposes prepared by the caller.
 */
typedef struct {
  asr_dec_fwd_t f;
  const float* wcatT;
  const float* wdecT;
  const float* dws;   /* may be NULL */
  float* G;
  float* dwext;
  float* dwraw;       /* [B][Tp] scratch */
  float* dfpart;      /* [A/64 tiles][B][C][Tp] scratch */
  float* dP;
  float* dgates;
  float* dD;
  float* dcell;       /* [B][D] carry of dL/dc, zero-filled by the caller */
  float* dgvec_part;
  float* dwatt_part;
  float* dconv_part;
} asr_dec_bwd_t;

int asr_dec_step_bwd(const asr_dec_bwd_t* p, int s, asr_stream_t stream);
int asr_dec_seq_bwd(const asr_dec_bwd_t* p, int s_begin, int s_end, asr_stream_t stream);
/* Persistent fast path of asr_dec_seq_bwd(p, 0, L) (same applicability rule and scratch convention as
 * asr_dec_seq_fwd_persist; the sequence must have been teacher-forced).  mbuf: caller-allocated scratch
 * [L][B][C][Tp].  Results as the per-step path in G[:, :, D:], dgates, dD, dP; dgvec_part / dwatt_part / dconv_part
 * receive the same totals over rows (placed in other rows: reduce over B as usual); dwext, dwraw, dfpart and dcell
 * are not used.  The embedding part of dX is formed by one batched GEMM after the recurrence. */
int asr_dec_seq_bwd_persist(const asr_dec_bwd_t* p, float* mbuf, void* xch, void* ctrl, asr_stream_t stream);

/* Persistent backward of a FREE-RUNNING sequence with the smooth-embedding feedback (forward:
 * asr_dec_seq_fwd_persist_free, mode 2; Decoder.forward with ys=None, smooth=True: model.py:334-341 - the unlabeled
 * decode of the semi-supervised generator step, solver.py:465-470).  Step s's embedding input is
 * softmax(scaling * logit_{s-1}) @ emb, so d(emb_s) flows into logit_{s-1} and from there into [z_{s-1}, ctx_{s-1}]:
 * the kernel carries that path inside the recurrence (two more XCD-local hand-offs per step).
 *   probs [L-1][B][V]  the probabilities the forward saved;  w_out [V][D+O];  emb [V][E]
 *   dlfb  [L][B][V]    out (zero-filled by the caller): gradient reaching logit_s through the feedback; the caller adds
 *                      it to the upstream d(logits) before forming the output-layer weight gradients
 * On return G[s][:, D+O:] holds d(emb_s) (dropout-masked) for every step.  V <= 36, E = 128, both geometries of
 * asr_dec_seq_bwd_persist (4 rows per group up to T' = 100 at 10 conv channels, 2 rows per group up to T' = 256: the
 * table at asr_dec_seq_fwd_persist); otherwise ASR_E_SHAPE (per-step kernels + asr_dec_feedback_bwd). */
typedef struct {
  int V;
  float scaling;
  const float* w_out;
  const float* emb;
  const float* probs;
  float* dlfb;
} asr_dec_feedback_bwd_t;
int asr_dec_seq_bwd_persist_free(const asr_dec_bwd_t* p, const asr_dec_feedback_bwd_t* fb, float* mbuf, void* xch,
                                 void* ctrl, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Parameter layout conversion: torch layout of nn.LSTM / nn.LSTMCell (gate-major rows i,f,g,o; model.py:67-68,262)
 * <-> the kernels' gate-interleaved rows (unit*4+gate).  w_ih/w_hh/b_ih/b_hh: arrays of `ndir` device pointers.
 *   asr_lstm_pack_f32    -> w_ih_cat [ndir*4H][I], w_hh_il [ndir][4H][H], bias [ndir*4H] = b_ih + b_hh
 *   asr_lstm_unpack_f32  gradients in the interleaved layout -> per-direction torch-layout dw_ih [4H][I],
 *                        dw_hh [4H][H], db [4H] (the gradient of b_ih and of b_hh)
 *   asr_cell_pack_f32    decoder cell: wcat [4D][D+O+E] = [w_hh | w_ih[:, E:E+O] | w_ih[:, :E]] interleaved, bcat
 *   asr_cell_unpack_f32  dwcat, db (interleaved) -> dw_ih [4D][E+O], dw_hh [4D][D], db [4D] (+ db2: a second copy, or NULL)
 *   asr_dec_pack_f32     asr_cell_pack_f32 + the transposed images the decoder kernels read, one launch: wcatT [D+O+E][4D]
 *                        (the backward's dX product), wdecT [D][A] of mlp_dec.weight [A][D], wattT [C][A] of mlp_att.weight
 *                        [A][C] (each output NULL = not wanted)
 *   asr_lstm_pack_multi_f32 / asr_lstm_unpack_multi_f32   asr_lstm_pack_f32 / asr_lstm_unpack2_f32 for up to
 *                        ASR_PACK_MAX_LAYERS layers in one launch (the encoder's three, the judge's two)
 *   asr_colsum_parts_f32 dst[i][j] = sum_r src[i][r * n[i] + j], r < rows, for up to four matrices: the decoder backward's
 *                        per-utterance partial gradients (gvec, mlp_att.weight, loc_conv.weight) in one launch
 * ------------------------------------------------------------------------------------- */
#define ASR_PACK_MAX_LAYERS 4
typedef struct {
  int H, I, ndir;
  const float* w_ih[2];
  const float* w_hh[2];
  const float* b_ih[2];
  const float* b_hh[2];
  float* w_ih_cat;
  float* w_hh_il;
  float* bias;
} asr_lstm_pack_job_t;
typedef struct {
  int H, I, ndir;
  const float* dw_ih_cat;
  const float* dw_hh_il;
  const float* db_il;
  float* dw_ih[2];
  float* dw_hh[2];
  float* db[2];
  float* db2[2];   /* second copy of the bias gradient (b_hh), or NULL */
} asr_lstm_unpack_job_t;
int asr_lstm_pack_multi_f32(int nlayers, const asr_lstm_pack_job_t* jobs, asr_stream_t stream);
int asr_lstm_unpack_multi_f32(int nlayers, const asr_lstm_unpack_job_t* jobs, asr_stream_t stream);
int asr_dec_pack_f32(int D, int O, int E, int A, int C, const float* w_ih, const float* w_hh, const float* b_ih,
                     const float* b_hh, const float* wdec, const float* watt, float* wcat, float* bcat, float* wcatT,
                     float* wdecT, float* wattT, asr_stream_t stream);
int asr_colsum_parts_f32(int nparts, int rows, const float* const* src, const int32_t* n, float* const* dst,
                         asr_stream_t stream);
int asr_lstm_pack_f32(int H, int I, int ndir, const float* const* w_ih, const float* const* w_hh,
                      const float* const* b_ih, const float* const* b_hh, float* w_ih_cat, float* w_hh_il,
                      float* bias, asr_stream_t stream);
int asr_lstm_unpack_f32(int H, int I, int ndir, const float* dw_ih_cat, const float* dw_hh_il, const float* db_il,
                        float* const* dw_ih, float* const* dw_hh, float* const* db, asr_stream_t stream);
/* as asr_lstm_unpack_f32, with an optional second set of bias-gradient outputs (db2[d], may be NULL): nn.LSTM has two
 * bias vectors per direction that receive the same gradient, and autograd would otherwise copy the shared tensor. */
int asr_lstm_unpack2_f32(int H, int I, int ndir, const float* dw_ih_cat, const float* dw_hh_il, const float* db_il,
                         float* const* dw_ih, float* const* dw_hh, float* const* db, float* const* db2,
                         asr_stream_t stream);

/* Teacher-forced decoder input in one launch (model.py:301-306,337: pad_list + embedding + dropout of the decoder input):
 * X [L+1][B][D+O+E] = [0 | 0 | emb_w[tokens[b][s]]] (slab L all zero), Xd (nullable) the same with xmask
 * [L][B][O+E] applied to the embedding part, fed [L][B] = tokens[b][s].  tokens: int64, element (b, s) at
 * tokens[b * tok_row_stride + s].  (D+O) % 4 == 0, E % 4 == 0, 16-byte aligned buffers. */
int asr_dec_prepare_f32(int L, int B, int D, int O, int E, const long long* tokens, int64_t tok_row_stride,
                        const float* emb_w, const float* xmask, float* X, float* Xd, long long* fed, asr_stream_t stream);
/* The gradient of those embedding rows (autograd of nn.Embedding, model.py:337): demb [V][E] (caller-zeroed or accumulating)
 * += grad[r][0..E) for every r < rows with 0 <= tokens[r] < V (a step that was not fed a token carries -1); grad row-strided
 * (ldg floats: the embedding columns of the decoder's dX buffer, read where they lie).  E % 4 == 0, ldg % 4 == 0, V * E * 4 <=
 * 64 KB (the table a workgroup folds its rows into: label matrices are skewed towards <EOS>); ASR_E_SHAPE otherwise - the
 * caller then takes its own index_add. */
int asr_embedding_grad_f32(int64_t rows, int E, int V, const long long* tokens, const float* grad, int64_t ldg,
                           float* demb, asr_stream_t stream);
int asr_cell_pack_f32(int D, int O, int E, const float* w_ih, const float* w_hh, const float* b_ih,
                      const float* b_hh, float* wcat, float* bcat, asr_stream_t stream);
int asr_cell_unpack_f32(int D, int O, int E, const float* dwcat, const float* db_il, float* dw_ih, float* dw_hh,
                        float* db, float* db2, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Label log-probabilities with label smoothing (Decoder.forward, model.py:354-366):
 *   out[r] = (1-ls) * log_softmax(logits[r])[index[r]] + ls * sum_v labeldist[v] * log_softmax(logits[r])[v]
 * (labeldist NULL: plain gather of the log-softmax).  rows = L*B; index is int64 (torch long).  total (NULL, or one float
 * the caller zeroed) += total_scale * sum_r out[r]: the training loss -mean(log_probs) (solver.py:377) is that sum times a
 * constant, so with total_scale = -1 / (B L) `total` IS the loss and neither a reduction nor a multiply follows.  argmax
 * (NULL, or int64 [rows]) receives argmax_v logits[r][v] (lowest index on ties: the `prediction` output of model.py:346).
 * The backward writes d(logits) for an upstream gradient grad_scale * grad_out[r * grad_stride] (grad_stride 0: ONE device
 * scalar for every row - the gradient of `total`, grad_scale = the forward's total_scale).
 * ------------------------------------------------------------------------------------- */
int asr_label_logprob_fwd(int64_t rows, int V, const float* logits, int64_t ld, const int64_t* index,
                          const float* labeldist, float ls_weight, float* out, float* total, float total_scale,
                          int64_t* argmax, asr_stream_t stream);
int asr_label_logprob_bwd(int64_t rows, int V, const float* logits, int64_t ld, const int64_t* index,
                          const float* labeldist, float ls_weight, const float* grad_out, int64_t grad_stride,
                          float grad_scale, float* dlogits, int64_t lddz, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Free-running decoder feedback (Decoder.forward loop, model.py:329-351): one launch per decoder step each way for
 * what sits between two steps when the next input is not a stored teacher token.
 *   forward : logits[b] = w_out [z_s, c_s] + b_out (x: row-strided [B, DO] slice of the step-input buffer, ldx);
 *             pred[b] = argmax (int64, lowest index on ties); then the embedding input of step s+1 into x_emb_next
 *             (same buffer layout, ldx) by mode:  0 = emb[pred[b]]  (greedy, model.py:336-337)
 *                                                 1 = softmax(scaling * logits[b]) @ emb  (smooth, model.py:341), the
 *                                                     probabilities are kept in probs [B, V] for the backward
 *                                                 2 = emb[tok[b * tok_stride]]  (teacher token of a tf draw, 331-333)
 *                                                 3 = nothing (last step).
 *             fed[b] = the token used (-1 for mode 1); xd_emb_next (optional) = x_emb_next * mask (dropout
 *             multipliers [B, ldm] of the embedding columns).  V <= 128.
 *   backward (mode 1 only): with demb = d loss / d x_emb of step s (row-strided, ldg) and p = probs of step s-1:
 *             dl = scaling * p * (demb emb^T - sum_v p_v (demb emb^T)_v);  dlog[b] += dl  (gradient of logits_{s-1},
 *             from which the caller takes dW_out, db_out once per sequence);  gtop[b] += dl w_out  (gradient of
 *             [z_{s-1}, c_{s-1}], same buffer layout as demb).
 * ------------------------------------------------------------------------------------- */
int asr_dec_feedback_fwd(int B, int V, int E, int DO, const float* x, int64_t ldx, const float* w_out,
                         const float* b_out, const float* emb, float* logits, int64_t* pred, int mode, float scaling,
                         const int64_t* tok, int64_t tok_stride, int64_t* fed, float* probs, float* x_emb_next,
                         float* xd_emb_next, const float* mask, int64_t ldm, asr_stream_t stream);
int asr_dec_feedback_bwd(int B, int V, int E, int DO, const float* demb, float* gtop, int64_t ldg, const float* probs,
                         const float* emb, const float* w_out, float scaling, float* dlog, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Beam search between two decoder steps (Decoder.recognize_beams, model.py:369-406 - a stub in the reference that this
 * library completes; the semantics are DESIGN 4.8's).  Per step the caller runs asr_dec_step_fwd and
 * asr_gemm_skinny_f32 on the B*K beam rows (row b*K + k), then asr_beam_select_f32 and asr_beam_reorder_f32; after the
 * last step asr_beam_backtrack.  Every buffer is caller-owned device memory; K > ASR_BEAM_KMAX, V < 2 or an eos outside
 * [0, V) returns ASR_E_SHAPE.
 *   asr_beam_select_f32   step t (0 <= t < L), one workgroup per utterance that is not done: logp = log_softmax(logits)
 *                         of each live beam (score > -inf); candidates score[k] + logp[v] ranked by score, then by the
 *                         lower flat index k*V + v; of the first 2K, an <EOS> at rank < K is finished (step t, source
 *                         beam k, length t+1), other <EOS> are skipped, the rest fill the live slots j in rank order
 *                         (tok_hist[t][b][j], bp_hist[t][b][j] = k, scores[b][j]); empty slots get <EOS>, 0, -inf.  At
 *                         t = L-1 the live beams are finished as they stand unless K are finished already.  An utterance
 *                         with K finished hypotheses (or at t = L-1, or with no live beam left) sets done[b] and adds 1
 *                         to *ndone; done utterances are not touched again.
 *   asr_beam_reorder_f32  step t (`logits` is not read): for every beam row of an utterance that is not done, row
 *                         b*K+j of the destination slot gathers row b*K + bp_hist[t][b][j] of the source slot - x[:, 0:D+O] (z, ctx), the cell
 *                         state and the attention weights - and x[:, D+O:] = emb[tok_hist[t][b][j]].  A gather: source
 *                         and destination are different buffers (ASR_E_ARG otherwise).
 *   asr_beam_backtrack    ranks each utterance's finished hypotheses by score / length^length_penalty (ties: the one
 *                         finished first) and writes the first K as tokens [B][K][L] (padded with <EOS>), scores [B][K]
 *                         (the ranking key; -inf for a rank without a hypothesis) and lengths [B][K] (counting <EOS>).
 * ------------------------------------------------------------------------------------- */
#define ASR_BEAM_KMAX 16
#define ASR_BEAM_FCAP 48    /* finished entries per utterance the caller provides (at most 2K - 1 are ever written) */
typedef struct {
  int B, K, V, L;         /* utterances, beam width (1..16), vocabulary, max_dec_timesteps */
  int eos;
  const float* logits;    /* [B*K][V] this step's output-layer logits */
  float* scores;          /* [B][K] running scores: 0 for beam 0 and -inf for the others at the start */
  int32_t* tok_hist;      /* [L][B][K] token of live slot j after step t */
  int32_t* bp_hist;       /* [L][B][K] its predecessor slot at step t-1 */
  int32_t* fin;           /* [B][ASR_BEAM_FCAP][4] finished hypotheses: (step, slot, length, ends with <EOS>) */
  float* fin_score;       /* [B][ASR_BEAM_FCAP] their scores (sum of log-probabilities) */
  int32_t* nfin;          /* [B] number of finished hypotheses, 0 at the start */
  int32_t* done;          /* [B] 0 at the start */
  int32_t* ndone;         /* one word: number of done utterances, 0 at the start (the host polls it) */
} asr_beam_t;
typedef struct {
  int D, O, E, Tp;
  int64_t ldx;            /* row stride of x_src / x_dst (>= D + O + E) */
  const float* x_src;     /* [B*K][ldx] step output slot: z, ctx */
  float* x_dst;           /* [B*K][ldx] next step's input slot */
  const float* c_src;     /* [B*K][D] cell state */
  float* c_dst;
  const float* w_src;     /* [B*K][Tp] attention weights */
  float* w_dst;
  const float* emb;       /* [V][E] embedding */
} asr_beam_state_t;
int asr_beam_select_f32(const asr_beam_t* p, int t, asr_stream_t stream);
int asr_beam_reorder_f32(const asr_beam_t* p, int t, const asr_beam_state_t* s, asr_stream_t stream);
int asr_beam_backtrack(const asr_beam_t* p, float length_penalty, int32_t* tokens, float* scores, int32_t* lengths,
                       asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Shallow fusion: the beam search rescored by the judge LM on the device.  Three entries added to ABI
 * version 6 WITHOUT a version change: they are additive - no existing entry, structure or constant changes, and a
 * caller that does not use them sees the library it saw before.
 * Every beam row carries the LM's state: per layer l an input row [x_l | h_l] of In_l + H floats (x_0: the LM embedding
 * of the consumed token, x_l: layer l-1's new h) and a cell state of H floats, each in two step slots.  Per step the
 * caller runs asr_lm_step_f32 once per layer (input slot -> output slot), asr_gemm_skinny_f32 for the LM's output layer,
 * asr_beam_select_lm_f32 in place of asr_beam_select_f32 and asr_beam_reorder_lm_f32 in place of asr_beam_reorder_f32.
 *   asr_lm_step_f32         one LSTM layer step for R rows (1 .. ASR_LM_MAX_ROWS), one launch, no gates in memory:
 *                           gates = xin[r][0 : In+H] W_cat^T + b with W_cat [4H][In+H] = [W_ih | W_hh] and b = b_ih + b_hh,
 *                           both gate-interleaved (row = unit*4 + gate, gates (i,f,g,o)); c_out = f c_prev + i g;
 *                           h = o tanh(c_out) goes to h_out[r*ldh + unit] and, if h_out2 != NULL, to h_out2[r*ldh2 +
 *                           unit] (the x part of the next layer's input row).  fp32-input MFMA: exact fp32 products.
 *                           H, In multiples of 16 up to ASR_LM_MAX_WIDTH, R <= ASR_LM_MAX_ROWS: ASR_E_SHAPE otherwise.
 *                           xin (row stride ldx >= In + H, a multiple of 4), W_cat and b 16-byte aligned.  A step reads
 *                           one slot and writes another: c_out == c_prev or an output equal to xin is ASR_E_ARG.
 *   asr_beam_select_lm_f32  asr_beam_select_f32 on the fused candidate score
 *                           (score[k] + log_softmax(logits_k)[v]) + lm_weight * log_softmax(lm_logits_k)[v] - fp32, each
 *                           operation rounded on its own, in this order; lm_logits [B*K][V] like p->logits.  Everything
 *                           else (ranking, ties, <EOS>, finishing, done) as asr_beam_select_f32; with lm_weight = 0 and
 *                           finite lm_logits every output word equals that entry's.
 *   asr_beam_reorder_lm_f32 the gather of asr_beam_reorder_f32 (s; NULL: skipped) and, in the same launch, for every LM
 *                           layer l and every beam row b*K+j of an utterance that is not done: the h part
 *                           x_dst[l][row][In_l : In_l+H] and c_dst[l][row] from row b*K + bp_hist[t][b][j] of x_src[l] /
 *                           c_src[l], and x_dst[0][row][0 : In_0] = emb[tok_hist[t][b][j]] (emb [V][In_0]: the LM's own
 *                           table).  The x parts of layers l > 0 are not touched (the next step writes them).  Source
 *                           and destination of a layer must differ (ASR_E_ARG); 1 .. ASR_LM_MAX_LAYERS layers.
 * ------------------------------------------------------------------------------------- */
#define ASR_LM_MAX_LAYERS 4
#define ASR_LM_MAX_ROWS 512
#define ASR_LM_MAX_WIDTH 1024
typedef struct {
  int n_layers, H;
  int in_dim[ASR_LM_MAX_LAYERS];          /* In_l: E of the LM for layer 0, H above */
  const float* x_src[ASR_LM_MAX_LAYERS];  /* [B*K][In_l + H] the step's output slot (only the h part is read) */
  float* x_dst[ASR_LM_MAX_LAYERS];        /* [B*K][In_l + H] the next step's input slot */
  const float* c_src[ASR_LM_MAX_LAYERS];  /* [B*K][H] */
  float* c_dst[ASR_LM_MAX_LAYERS];
  const float* emb;                       /* [V][In_0] */
} asr_beam_lm_state_t;
int asr_lm_step_f32(int R, int H, int In, const float* xin, int64_t ldx, const float* wcat, const float* bcat,
                    const float* c_prev, float* c_out, float* h_out, int64_t ldh, float* h_out2, int64_t ldh2,
                    asr_stream_t stream);
int asr_beam_select_lm_f32(const asr_beam_t* p, const float* lm_logits, float lm_weight, int t, asr_stream_t stream);
int asr_beam_reorder_lm_f32(const asr_beam_t* p, int t, const asr_beam_state_t* s, const asr_beam_lm_state_t* lm,
                            asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Scoring: batched edit distance on token ids (utils.py:222-228: editdistance.eval per utterance).  One entry
 * added to ABI version 6 WITHOUT a version change: it is additive, like the beam entries.
 *   asr_edit_distance_i32   for every pair p < n_pairs: dist[p] = the Levenshtein distance (unit costs) between
 *                           filter(cut(hypothesis row p)) and filter(reference row r), r = p or ref_of_pair[p] (a valid
 *                           row of `ref`: K hypotheses may share one reference).
 *                           hyp: rows of hyp_cols tokens, row stride ldh elements, int32 (hyp_elem_bytes 4: beam tokens)
 *                           or int64 (8: the greedy prediction; the ids must fit int32); row p runs to hyp_len[p]
 *                           (clamped to 0 .. hyp_cols; NULL: to hyp_cols).  ref: int32 rows of stride ldr, row r runs to
 *                           ref_len[r] (clamped to 0 .. ldr).
 *                           cut: the hypothesis ends before its first `eos` (eos < 0: no cut); references are never cut.
 *                           filter: a token t with 0 <= t < V and skip[t] != 0 is dropped from BOTH sides (skip NULL or
 *                           V <= 0: nothing is dropped); ids outside [0, V) are ordinary tokens, the table is never read
 *                           out of range.  Empty sides are legal: the distance is the other side's filtered length.
 *                           hyp_n[p], ref_n[p] (each may be NULL): the two filtered lengths.  totals (may be NULL):
 *                           totals[0] += sum of dist, totals[1] += sum of ref_n, 64-bit integer atomics (the caller zeroes
 *                           them; integer sums do not depend on the order, so the result is deterministic).
 *                           Limits: hyp_cols and ldr (the bound of a reference's length) at most ASR_ED_MAX_COLS, which
 *                           also bounds both filtered lengths: ASR_E_SHAPE beyond.  n_pairs <= 0, a NULL hyp / ref /
 *                           ref_len / dist, an element size other than 4 or 8, ldh < hyp_cols: ASR_E_ARG.
 *                           One launch, no host synchronisation, no allocation.
 * ------------------------------------------------------------------------------------- */
#define ASR_ED_MAX_COLS 4096
int asr_edit_distance_i32(int n_pairs, const void* hyp, int hyp_elem_bytes, int64_t ldh, int hyp_cols,
                          const int32_t* hyp_len, const int32_t* ref, int64_t ldr, const int32_t* ref_len,
                          const int32_t* ref_of_pair, int eos, const uint8_t* skip, int V, int32_t* dist, int32_t* hyp_n,
                          int32_t* ref_n, long long* totals, asr_stream_t stream);
/*   asr_word_edit_distance_i32   the same call with `space`, on WORDS (the scoring half of WER).  Added to ABI
 *                           version 8 WITHOUT a version change: additive.  Each side is cut and filtered as above; a word is
 *                           a maximal run of the kept tokens that are not `space` - str.split() of the rendered text:
 *                           leading, trailing and repeated spaces make no words, and a dropped token between two letters
 *                           joins them into one word.  Two words are equal iff their token sequences are equal (a hash
 *                           only pre-filters; the tokens decide).  dist[p] = the Levenshtein distance (unit costs) between
 *                           the two word sequences; hyp_n[p], ref_n[p] = the word counts; totals[0] += sum of dist,
 *                           totals[1] += sum of ref_n.  Empty sides are legal.  A `space` that the skip table drops is never
 *                           seen: each side is then at most one word.
 *                           Limits and refusals as above (a side holds at most ASR_ED_MAX_COLS / 2 words); space < 0:
 *                           ASR_E_ARG.  One launch, no host synchronisation, no allocation. */
int asr_word_edit_distance_i32(int n_pairs, const void* hyp, int hyp_elem_bytes, int64_t ldh, int hyp_cols,
                               const int32_t* hyp_len, const int32_t* ref, int64_t ldr, const int32_t* ref_len,
                               const int32_t* ref_of_pair, int eos, const uint8_t* skip, int V, int space, int32_t* dist,
                               int32_t* hyp_n, int32_t* ref_n, long long* totals, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Optimiser on a flat fp32 buffer (solver.py:152-153,384-385: clip_grad_norm_ + Adam(amsgrad,
 * weight_decay).step).  asr_sumsq_f32 adds sum(g^2) into the device scalar out[0] (caller zeroes
 * it); asr_adam_clip_f32 scales g by min(1, max_norm/(sqrt(*gnorm_sq)+1e-6)) (skipped when
 * gnorm_sq is NULL), folds weight_decay*p into g, updates m, v, the AMSGrad max (skipped when vmax
 * is NULL) and p.  bias_c1 = 1-beta1^t, bias_c2 = 1-beta2^t are passed by the host.  skip_if_nonzero (may be
 * NULL): a 4-byte device word; when it is not zero at the time the kernel runs, nothing is updated - the abort latch
 * of the persistent kernels (or its all-reduced sum), so that the step can be enqueued before the host has read it.
 * zero_word (may be NULL): one float the kernel sets to zero whether or not the update is skipped - the accumulator the
 * NEXT step's asr_sumsq_f32 adds into (a caller that alternates between two words needs no fill launch per step).
 * ------------------------------------------------------------------------------------- */
int asr_sumsq_f32(int64_t n, const float* g, float* out, asr_stream_t stream);
/* The gradient gather in front of them in a one-process step: flat[dst_offset[j] .. + count[j]) = src[j][0 .. count[j]) for
 * njobs contiguous tensors (what autograd left in the parameters' .grad) and, if sumsq != NULL, sumsq[0] += the sum of their
 * squares - torch._foreach_copy_ and asr_sumsq_f32 in one pass over the gradients (the norm of clip_grad_norm_,
 * solver.py:384, is taken where they are read anyway).  Jobs beyond ASR_GATHER_MAX_JOBS take further launches. */
#define ASR_GATHER_MAX_JOBS 64
int asr_gather_sumsq_f32(int njobs, const float* const* src, const int64_t* dst_offset, const int64_t* count, float* flat,
                         float* sumsq, asr_stream_t stream);
int asr_adam_clip_f32(int64_t n, float* p, const float* g, float* m, float* v, float* vmax,
                      const float* gnorm_sq, float max_norm, float lr, float beta1, float beta2, float eps,
                      float weight_decay, float bias_c1, float bias_c2, const void* skip_if_nonzero, float* zero_word,
                      asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Deterministic mode (csrc/reduce_det.hip).  Ten entries added to ABI version 8 WITHOUT a version change, like
 * the beam and scoring entries: they are additive - no existing entry, structure or constant changes, and a caller that does
 * not use them sees the library it saw before.  Every entry above that adds fp32 partial sums with
 * atomics - a K split of asr_gemm_f32 / asr_gemm_skinny_f32, asr_colsum_f32, asr_embedding_grad_f32, the dfill of
 * asr_rows_unpack_bwd_f32, asr_sumsq_f32 / asr_gather_sumsq_f32, the `total` of asr_label_logprob_fwd - gives results
 * that differ in the last bits from run to run: the order of the adds is the order in which workgroups happen to arrive.
 * The entries below compute the same quantities as functions of the inputs and the shapes ONLY.  There is no switch
 * inside the library: a caller that wants reproducible results calls these instead (hip_backend.DETERMINISTIC routes the
 * host code).  Workspaces are the caller's, like every other buffer; no entry waits for the host or fills memory.
 * One scheme throughout: partial sums are written by their one owner with plain stores, a second launch adds them in index
 * order.  No float atomics, in global memory or LDS.
 *
 *   asr_colsum_det_f32         replaces asr_colsum_f32.  Rows in chunks of 256 (N, ldx multiples of 4 and X 16-byte
 *                              aligned: the float4 path) or 512 rows.  Column n of a chunk: row group r sums its rows
 *                              m0 + r, m0 + r + G, ... in ascending order (G = 16 / 4 row groups), the groups are added
 *                              (((l_0 + l_1) + l_2) + ...) (G = 16) resp. (l_0 + l_1) + (l_2 + l_3) (G = 4); the chunk sums
 *                              are added in ascending chunk order; out = that, or out + that with accumulate.
 *                              ws: ceil(M / 256) * N floats (not touched when M fits one chunk); ASR_E_ARG if smaller.
 *   asr_gemm_det_f32           replaces asr_gemm_f32 wherever that would split K.  Arguments as asr_gemm_f32 plus the
 *                              workspace.  K is cut into S ranges: S = split_k when split_k >= 1 (tests, measurements),
 *                              else the library's rule, a function of M, N and K alone - 1 when K < 1 024 or the
 *                              ceil(M / 128) ceil(N / 128) output tiles are 256 or more, else min(16, 256 / tiles,
 *                              K / 512).  A range is ceil(K / S) long, rounded up to a multiple of 32 when that is at
 *                              least 32; the last range takes what is left, and S becomes the number of ranges that exist.
 *                              Slab s = op(A)[:, range s] op(B)[range s, :] is an UNSPLIT product (asr_gemm_f32 with
 *                              split_k = 1, the ranges as its batch: stride = the range's offset in A and B, M N in ws; a
 *                              shorter last range is a second launch), then one kernel forms
 *                                C = (((ws[0] + ws[1]) + ...) + ws[S-1]) (+ bias) (+ C if accumulate) (relu)
 *                              one rounded fp32 add per step, in exactly this order (bias, accumulate, relu: the order of
 *                              the unsplit asr_gemm_f32 epilogue, so S = 1 and S > 1 are one function).  S = 1: asr_gemm_f32 with
 *                              split_k = 1 and nothing else (ws may be NULL).  batch > 1 with S > 1: the products run one
 *                              after the other through the same workspace.  ASR_GEMM_C_ZEROED is ignored.
 *   asr_gemm_det_ws_bytes      the bytes asr_gemm_det_f32 needs for these arguments (0, or S M N 4), S and the range
 *                              length; returns what the call would return before it launches (0, ASR_E_ARG, ASR_E_SHAPE -
 *                              the refusals of asr_gemm_f32).  Pointers are looked at for NULL and alignment only.
 *   asr_embedding_grad_det_f32 replaces asr_embedding_grad_f32 (same limits).  One owner per (token id v, 4 columns):
 *                              a = 0; for r = 0 .. rows - 1 in order: a += grad[r] if tokens[r] == v; demb[v] += a.
 *   asr_rows_fill_grad_det_f32 replaces the dfill half of asr_rows_unpack_bwd_f32 (call that with dfill = NULL, then this).
 *                              Utterance b: frame lane f of FL = min(8, 512 / (C / 4)) sums dout * mask over the padded
 *                              frames len + f, len + f + FL, ... in ascending order, the lanes are added
 *                              ((l_0 + l_1) + ...); dfill[c] += ((p_0 + p_1) + ... + p_{B-1}) in ascending b, only where
 *                              relu_of[c] > 0 when relu_of is given.  ws: B * C floats.
 *   asr_sumsq_det_f32          replaces asr_sumsq_f32: out[0] = out[0] + sum(g^2).  min(1 024, ceil(n / 1 024)) workgroups
 *                              store one partial each (a thread's elements in ascending order; lanes by the xor butterfly
 *                              32, 16, .. 1; waves (w_0 + w_1) + (w_2 + w_3)); ONE workgroup of a second launch adds the
 *                              partials the same way (thread t: partials t, t + 256, ...).  Adding to the word keeps the
 *                              protocol of asr_adam_clip_f32's zero_word: no fill launch.  ws: ASR_SUMSQ_DET_WS_BYTES.
 *   asr_gather_sumsq_det_f32   replaces asr_gather_sumsq_f32 (same jobs, chunks and copies): a partial per 8 192-element
 *                              chunk, combined as above after each launch.  ws: sum_j ceil(count[j] / 8 192) floats.
 *   asr_sum_det_f32            out[0] = out[0] + scale * sum_i x[i], one workgroup, order as the second launch above:
 *                              the `total` of asr_label_logprob_fwd (call that with total = NULL, then this on its `out`
 *                              with scale = total_scale).
 *   asr_dec_step_bwd_det / asr_dec_seq_bwd_det   replace asr_dec_step_bwd / asr_dec_seq_bwd: the same kernels, the two
 *                              skinny products that add into G without their K split (csrc/gemm.hip: skinny_kernel adds
 *                              the slices with atomics).  The per-utterance partial sums of these kernels have one owner.
 * ------------------------------------------------------------------------------------- */
#define ASR_SUMSQ_DET_WS_BYTES 4096
int asr_colsum_det_f32(int64_t M, int64_t N, const float* X, int64_t ldx, float* out, int accumulate, float* ws,
                       int64_t ws_bytes, asr_stream_t stream);
int asr_gemm_det_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B,
                     int64_t ldb, float* C, int64_t ldc, const float* bias, int relu, int accumulate, int batch, int64_t sA,
                     int64_t sB, int64_t sC, int split_k, int arith, float* ws, int64_t ws_bytes, asr_stream_t stream);
int asr_gemm_det_ws_bytes(int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                          const float* B, int64_t ldb, const float* C, int64_t ldc, const float* bias, int relu,
                          int accumulate, int batch, int64_t sA, int64_t sB, int64_t sC, int split_k, int arith,
                          int64_t* ws_bytes, int* split, int64_t* k_range);
int asr_embedding_grad_det_f32(int64_t rows, int E, int V, const long long* tokens, const float* grad, int64_t ldg,
                               float* demb, asr_stream_t stream);
int asr_rows_fill_grad_det_f32(int B, int T, int C, const float* dout, const int32_t* lens, const float* mask, uint64_t seed,
                               float p, float* dfill, const float* relu_of, float* ws, int64_t ws_bytes, asr_stream_t stream);
int asr_sumsq_det_f32(int64_t n, const float* g, float* out, float* ws, int64_t ws_bytes, asr_stream_t stream);
int asr_gather_sumsq_det_f32(int njobs, const float* const* src, const int64_t* dst_offset, const int64_t* count, float* flat,
                             float* sumsq, float* ws, int64_t ws_bytes, asr_stream_t stream);
int asr_sum_det_f32(int64_t n, const float* x, float scale, float* out, asr_stream_t stream);
int asr_dec_step_bwd_det(const asr_dec_bwd_t* p, int s, asr_stream_t stream);
int asr_dec_seq_bwd_det(const asr_dec_bwd_t* p, int s_begin, int s_end, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * CTC loss on the encoder output (csrc/ctc.hip): the CTC branch of joint CTC-attention training,
 * (1 - w) L_att + w L_ctc.  Not a reference operator - the reference has no CTC branch.  Three entries added to ABI version 8
 * WITHOUT a version change, like the deterministic entries: additive.
 *   logits        [B][T][V] fp32 RAW logits, row stride ld >= V floats; the log-softmax over V is taken inside (one
 *                 log-sum-exp per frame is all that is stored of it).  Frames t >= frame_lens[b] are never read.
 *   frame_lens    int32 [B] on the device (clamped to 0 .. T).
 *   labels        ONE packed int64 tensor on the device; utterance b owns labels[label_offsets[b] .. label_offsets[b + 1]),
 *                 label_offsets int32 [B + 1] on the device.  Blank = index 0, which is never a label: a label outside
 *                 [1, V), or more than max_label_len labels, makes the utterance infeasible.
 *   max_label_len an upper bound of every utterance's label count, known to the host (it sizes the workspace and picks the
 *                 kernel: one wave per utterance up to 2 max_label_len + 1 = 64 states, one 256-thread workgroup beyond,
 *                 states strided over the threads above 256).  At most ASR_CTC_MAX_LABELS; V >= 2: ASR_E_SHAPE otherwise.
 *   asr_ctc_ws_bytes   the bytes of the workspace for these sizes: 4 ( B T (2 max_label_len + 2) + B (max_label_len + V + 1) ),
 *                 each of the five parts rounded up to 64 words.  The forward fills it (log-sum-exps, alpha, the raw nll, the
 *                 label-sorted position list of every utterance), the backward reads it and overwrites alpha with
 *                 alpha + beta: one backward per forward, same arguments.
 *   asr_ctc_loss_fwd   nll[b] = -log p(labels_b | logits_b), alpha in log space.  An utterance with no alignment (frames <
 *                 labels + adjacent equal labels) has nll = +inf; with zero_infinity != 0 the output is 0 instead (the
 *                 workspace keeps the raw value).  Two launches.
 *   asr_ctc_loss_bwd   dlogits[b][t][k] = grad_nll[b] (softmax_k - exp(logsum_{s : l'_s = k} (alpha_t(s) + beta_t(s)) - logp_k
 *                 + nll_b)), row stride lddz >= V; exact zeros for t >= frame_lens[b] and, with zero_infinity, for an
 *                 infeasible utterance (without it: grad_nll[b] softmax_k).  Two launches.
 * No floating-point atomics: the sum over the states of a label is taken by ONE lane in ascending position order (the blank's
 * by the wave: lane-strided ascending, then the xor butterfly), so both calls are functions of their inputs and shapes only -
 * the same bits in every run, in and outside deterministic mode.  No host synchronisation, no allocation.
 * ------------------------------------------------------------------------------------- */
#define ASR_CTC_MAX_LABELS 1023
int asr_ctc_ws_bytes(int B, int T, int V, int max_label_len, int64_t* ws_bytes);
int asr_ctc_loss_fwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens, const int64_t* labels,
                     const int32_t* label_offsets, int max_label_len, int zero_infinity, float* nll, void* ws,
                     int64_t ws_bytes, asr_stream_t stream);
int asr_ctc_loss_bwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens, const int64_t* labels,
                     const int32_t* label_offsets, int max_label_len, int zero_infinity, const float* grad_nll, void* ws,
                     int64_t ws_bytes, float* dlogits, int64_t lddz, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Star CTC: the CTC loss for transcripts with missing words (csrc/ctc_star.hip; after Star Temporal
 * Classification, Pratap et al. 2022, and its relatives W-CTC and OTC).  Three entries added to ABI version 8 WITHOUT a
 * version change, like the CTC loss entries: additive - no existing entry, constant or kernel changes.
 * The arguments and conventions are asr_ctc_loss_fwd's (raw logits [B][T][V] with row stride ld, blank = 0, frame_lens int32
 * [B] on the device, one packed int64 label tensor with int32 offsets, x[t][v] = z[t][v] - logsumexp_v z[t]), plus
 *   penalty       fp32 [B] on the device: the price of one frame in a star state, <= 0 or -inf (the caller's to check).
 * Per frame nb[t] = logsumexp_{v >= 1} z[t][v] - lse[t], a direct log-sum-exp over the non-blank entries (never
 * log(1 - p_0)).  For labels l_1 .. l_L the lattice has S = 3 L + 2 states: b_0, s_0, then (l_g, b_g, s_g) for g = 1 .. L.
 *   emission      b_g: x[t][0]    l_g: x[t][l_g]    s_g: nb[t] + penalty[b]   ("any token", at a price)
 *   b_g comes from b_g, s_g, and l_g if g >= 1;   s_g comes from s_g, b_g, and l_g if g >= 1;
 *   l_g comes from l_g, b_{g-1}, s_{g-1}, and l_{g-1} if g >= 2 and l_g != l_{g-1};  every transition takes one frame.
 *   Frame 0 sits in b_0, s_0 or l_1; the path ends in l_L, b_L or s_L (L = 0: b_0 or s_0).
 *   nll[b] = -logsumexp over all state paths of the summed emissions: the path sum of this automaton, NOT a normalised
 *   probability (a star frame and a label frame may both count the same token) - it may be negative when the penalty is near
 *   0, and nll_star <= nll_ctc always.  penalty = -inf leaves the star states unreachable: the plain CTC lattice.
 * A row is infeasible when frames < labels + adjacent equal labels, when a label lies outside [1, V) or there are more than
 * max_label_len of them, or when it has no frame (T_b = 0, whatever L): nll = +inf, or 0 with zero_infinity.
 *   max_label_len at most ASR_CTC_STAR_MAX_LABELS (3 L + 2 states fit the LDS rows of the CTC chains); V >= 2: ASR_E_SHAPE
 *                 otherwise.  It picks the kernel by 3 max_label_len + 2 states: one wave per utterance up to 64 states
 *                 (max_label_len <= 20), one 256-thread workgroup with a state per thread up to 256 (<= 84), states strided
 *                 over the threads beyond (>= 85).
 *   asr_ctc_star_ws_bytes   4 ( B T (3 max_label_len + 4) + B (max_label_len + V + 1) ), each of the six parts rounded up to
 *                 64 words: lse, nb, the raw nll, alpha, the label-sorted position list, its heads.  The workspace is 4-byte
 *                 aligned (ASR_E_ARG otherwise, and when it is too small); the forward fills it, the backward overwrites
 *                 alpha with the log occupancy of every (t, s): one backward per forward, same arguments.
 *   asr_ctc_star_loss_fwd   three launches (lse and nb per frame; alpha).
 *   asr_ctc_star_loss_bwd   dlogits[b][t][k] = grad_nll[b] (softmax_k - occ_k), with gamma_t(s) the state occupancy,
 *                 occ_k = sum_{s : label k} gamma_t(s) + [k >= 1] (sum_g gamma_t(s_g)) exp(x[t][k] - nb[t]);
 *                 row stride lddz >= V; exact zeros for t >= frame_lens[b] and, with zero_infinity, for an infeasible
 *                 utterance (without it: grad_nll[b] softmax_k).  No gradient flows to penalty.  Two launches.
 * No floating-point atomics: the blank's and the star's sums are taken by the wave (lane-strided ascending, then the xor
 * butterfly), each label's by ONE lane along the sorted position list - the same bits in every run, in and outside
 * deterministic mode, whatever the rest of the batch.  No host synchronisation, no allocation.
 * ------------------------------------------------------------------------------------- */
#define ASR_CTC_STAR_MAX_LABELS 681
int asr_ctc_star_ws_bytes(int B, int T, int V, int max_label_len, int64_t* ws_bytes);
int asr_ctc_star_loss_fwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                          const int64_t* labels, const int32_t* label_offsets, int max_label_len, const float* penalty,
                          int zero_infinity, float* nll, void* ws, int64_t ws_bytes, asr_stream_t stream);
int asr_ctc_star_loss_bwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                          const int64_t* labels, const int32_t* label_offsets, int max_label_len, const float* penalty,
                          int zero_infinity, const float* grad_nll, void* ws, int64_t ws_bytes, float* dlogits, int64_t lddz,
                          asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Graph CTC (GTC; Moritz et al. 2021): a CTC loss over a label graph, for n-best pseudo-labels, confusion networks and any
 * other supervision that is a weighted set of label sequences (csrc/gtc.hip; the graphs are built and
 * validated on the host, gtc.py).  Three entries added to ABI version 8 WITHOUT a version change: additive - no existing
 * entry, constant or kernel changes.  The arguments and conventions are asr_ctc_loss_fwd's (raw logits [B][T][V] with row
 * stride ld, blank = 0, frame_lens int32 [B] on the device, x[t][v] = z[t][v] - logsumexp_v z[t]), with a graph table and
 * graph_of int32 [B] on the device (the graph of every row, in 0 .. G-1; rows may share a graph) in place of the labels.
 * Definition.  Per utterance there is a graph with N nodes.  Node n has a token lab[n] in [0, V) (0 = blank), a start
 * weight start[n] and a final weight fin[n], fp32, finite or -inf.  Arcs (m -> n, w) carry an fp32 weight w, finite.
 * Self-loops are ordinary arcs and are never implied; there are no parallel arcs.  With T the row's frame count a path is
 * n_0 .. n_{T-1} along arcs, its score
 *   start[n_0] + sum_t x[t][lab[n_t]] + sum_{t >= 1} w(n_{t-1}, n_t) + fin[n_{T-1}]
 * and nll = -logsumexp over all paths: a PATH SUM, not a normalised probability (the weights are any log numbers; two paths
 * may spell the same tokens).  dlogits[b][t][k] = grad_nll[b] (softmax_k - occ_k), occ_k = sum_{n : lab[n] = k} gamma_t(n),
 * gamma the node occupancy, normalised over the frame's nodes.  A row with no path of finite score, or with T = 0, is
 * infeasible: nll = +inf, or 0 with zero_infinity, and a zero gradient either way.  No gradient flows to arc, start or
 * final weights.
 * The table (asr_gtc_graphs_t; every pointer on the device, no array empty; its contents are trusted on the device and
 * validated on the host, like the context and n-gram tables).  G graphs concatenated, NN nodes and A arcs in all:
 *   node_off int32 [G + 1]     the nodes of graph g are node_off[g] .. node_off[g + 1] - 1; arcs name nodes by their index
 *                              inside the graph
 *   lab int32 [NN], start, fin fp32 [NN]
 *   in_ptr int32 [NN + 1], in_src int32 [A], in_w fp32 [A]       arcs by destination (CSR over all nodes), sources ascending
 *   out_ptr int32 [NN + 1], out_dst int32 [A], out_w fp32 [A]    arcs by source, destinations ascending
 *   order int32 [NN]           per graph its nodes sorted by (token, node)
 *   head int32 [G][V]          (first index in the graph's order << 12) | run length of the token's nodes; 0: no node
 *   V, G; max_nodes, max_arcs  the largest graph's, at most ASR_GTC_MAX_NODES (the CTC chains' 2 * 1023 + 1 states, so their
 *                              LDS rows serve) and ASR_GTC_MAX_ARCS (65 536: both arc lists of a graph, 1 MiB, stay in a
 *                              quarter of one XCD's L2 while a chain re-reads them every frame); V >= 2: ASR_E_SHAPE otherwise.
 *                              max_nodes picks the kernel: one wave per utterance up to 64 nodes, a node per thread up to
 *                              256, nodes strided over 256 threads beyond.
 *   asr_gtc_ws_bytes   plain integers: 4 (B T (max_nodes + 1) + B), each of the three parts rounded up to 64 words: lse, the
 *                      raw nll, alpha.  The workspace is 4-byte aligned (ASR_E_ARG otherwise, and when it is too small); the
 *                      forward fills it, the backward overwrites alpha with the occupancy of every (t, n): one backward
 *                      per forward, same arguments.
 *   asr_gtc_loss_fwd   two launches (lse per frame; alpha).     asr_gtc_loss_bwd   two launches (the backward chain - the
 *                      occupancies gamma_t(m) = sum over arcs (m -> n, w) of gamma_{t+1}(n) exp(alpha_t(m) + w - in_{t+1}(n)),
 *                      in the log-sum-exp over n's incoming arcs, in linear space from the forward's own shares -; the gradient); row
 *                      stride lddz >= V, exact zeros for t >= frame_lens[b] and for an infeasible row.
 * A thread sums the arcs of its node with an online log-sum-exp in the table's order (-inf (+) x = x exactly; unreachable
 * nodes stay -inf); the first four arcs of a node ride in registers, the rest are read from global memory every frame.  No
 * floating-point atomics, every sum in an order fixed by the graph and the shapes: the same bits in every run, in and
 * outside deterministic mode, whatever the rest of the batch.  No host synchronisation, no allocation.
 * ------------------------------------------------------------------------------------- */
#define ASR_GTC_MAX_NODES 2047
#define ASR_GTC_MAX_ARCS 65536
typedef struct {
  int32_t V, G;                   /* tokens, graphs */
  int32_t max_nodes, max_arcs;    /* of the largest graph */
  const int32_t* node_off;
  const int32_t* lab;
  const float* start;
  const float* fin;
  const int32_t* in_ptr;
  const int32_t* in_src;
  const float* in_w;
  const int32_t* out_ptr;
  const int32_t* out_dst;
  const float* out_w;
  const int32_t* order;
  const int32_t* head;
} asr_gtc_graphs_t;
int asr_gtc_ws_bytes(int B, int T, int V, int max_nodes, int64_t* ws_bytes);
int asr_gtc_loss_fwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                     const asr_gtc_graphs_t* graphs, const int32_t* graph_of, int zero_infinity, float* nll, void* ws,
                     int64_t ws_bytes, asr_stream_t stream);
int asr_gtc_loss_bwd(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                     const asr_gtc_graphs_t* graphs, const int32_t* graph_of, int zero_infinity, const float* grad_nll,
                     void* ws, int64_t ws_bytes, float* dlogits, int64_t lddz, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Graph CTC, the n-best graph builder: the list asr_ctc_beam_f32 leaves on the device compiled into an asr_gtc_graphs_t
 * table on the device, one prefix-tree graph per row (csrc/gtc_nbest.hip).  Two entries added to ABI version 8
 * WITHOUT a version change: additive - no existing entry, constant or kernel changes.
 * Inputs: hyp int32 [B][K][L] (padded with -1), hyp_len int32 [B][K] (-1: a dead slot), score fp32 [B][K] (-inf: a dead
 * slot), temperature (finite, >= 0), V.  1 <= K <= ASR_BEAM_KMAX, L >= 1, 2 <= V <= 2^20; otherwise ASR_E_SHAPE, as when
 * B times a capacity would pass INT_MAX / 2.  Trust: the tokens of live hypotheses lie in 1 .. V-1 (they come from the
 * search); like the contents of the other tables they are not checked on the device.  A token outside is copied into lab
 * as it stands; no index of the builder itself is formed from a token.
 * Output: the complete table, G = B graphs, graph_of[b] = b.  For every row it is, element for element, what
 * gtc.Graph.from_nbest and gtc._concat (gtc.py) make of the same list:
 *   weights     a slot is live iff hyp_len >= 0 and score > -inf.  log w_k = the log-softmax of temperature * score over the
 *               row's admitted live slots (below), in float64; log_weights fp64 [B][K] holds it, -inf in every other slot.
 *   duplicates  equal hypotheses join their weights by logaddexp in float64, in ascending slot order.
 *   no slot     a row without an admitted slot gets the graph of the empty hypothesis at weight 0.
 *   numbering   node 0 is the root's blank; trie node u (breadth first, children in token order, u = 1, 2, ..) gives the
 *               token node 2u - 1 and the blank node 2u.
 *   arcs        l_u -> l_u, l_u -> b_u, b_u -> b_u, b_u -> l_c for each child c of u, and l_u -> l_c where the tokens differ,
 *               all at weight 0; out lists by (source, destination), in lists by (destination, source).  Start weight 0 on
 *               the root's blank and the root's children, -inf elsewhere; final weight = the joined weight of the
 *               hypotheses that end in u on l_u and b_u, -inf elsewhere (rounded to fp32 once).
 *   order, head as in the table's definition above.   node_off, in_ptr, out_ptr: running offsets over the rows.
 * The node limit.  Hypotheses are admitted in slot order while the tree stays within (ASR_GTC_MAX_NODES - 1) / 2 = 1023 trie
 * nodes beyond the root: hypothesis k adds len_k - max over the admitted j < k of lcp(j, k) nodes.  The first live
 * hypothesis that does not fit and every live slot behind it are dropped; the weights are the log-softmax over the admitted
 * slots only; dropped int32 [B] counts the live slots a row lost.
 * Capacity.  Nothing is read back, so the caller sizes the arrays by bounds (asr_nbest_gtc_bytes): cap_nodes =
 * min(2 K L + 1, ASR_GTC_MAX_NODES) per row, cap_arcs = 3 cap_nodes; lab, start, fin, order [B cap_nodes]; in_ptr, out_ptr
 * [B cap_nodes + 1]; the arc arrays [B cap_arcs]; node_off [B + 1]; head [B][V].  The table's max_nodes and max_arcs are these
 * bounds (ASR_E_ARG otherwise): the loss kernels dispatch by them and guard every row's own N, which moves thread ownership
 * only, never the order of a sum.  Everything behind the counts actually written is undefined.
 *   asr_nbest_gtc_bytes  plain integers, no GPU: the two capacities and the workspace (8 B bytes: a node and an arc count
 *                        per row), 4-byte aligned.
 *   asr_nbest_gtc_f32    two launches, one workgroup per row each: the counts; then every array of the row, the workgroup
 *                        summing the counts of the rows in front itself.  The pointers of `table` name the caller's arrays,
 *                        which the call WRITES.  Integer work and float64 weights: bit-reproducible, a row's graph (its
 *                        nodes and arcs numbered inside the graph, lab, start, fin, order, its head row) a function of that
 *                        row alone.  No host synchronisation, no allocation.
 * ------------------------------------------------------------------------------------- */
int asr_nbest_gtc_bytes(int B, int K, int L, int V, int32_t* cap_nodes, int32_t* cap_arcs, int64_t* ws_bytes);
int asr_nbest_gtc_f32(int B, int K, int L, int V, const int32_t* hyp, const int32_t* hyp_len, const float* score,
                      double temperature, const asr_gtc_graphs_t* table, int32_t* graph_of, double* log_weights,
                      int32_t* dropped, void* ws, int64_t ws_bytes, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Joint CTC-attention decoding: the CTC prefix score inside the beam search (csrc/ctc_prefix.hip, the CTC variants of the
 * select kernel in csrc/beam.hip).  Four entries added to ABI version 8 WITHOUT a version change, like the CTC
 * loss entries: additive - no existing entry, structure or constant changes, and asr_beam_select_f32 /
 * asr_beam_select_lm_f32 launch the kernels they launched before.
 * With x[t][v] = logits[b][t][v] - logsumexp_v logits[b][t] over the T_b = frame_lens[b] valid frames (frames behind T_b are
 * never read), every beam row b*K+k carries, for its prefix g: r_n[t], r_b[t] (log-probability of g ending at frame t in a
 * non-blank / a blank) as pairs state[slot][row][t][2], last[slot][row] (g's last token; -1: g is empty) and
 * psi_prev[row] = psi(g).  (+) is log(exp a + exp b) with (-inf) (+) (-inf) = -inf.
 *   asr_ctc_prefix_init_f32     once per search, one launch: lse [B][Tp], and for all B*K rows slot 0 = the empty prefix:
 *                               r_n[t] = -inf, r_b[t] = sum_{tau <= t} x[tau][blank] (a wave scan: 64 frames per round,
 *                               the earlier rounds' total added behind it - an order fixed by T_b), last = -1, psi_prev = 0.
 *                               host_lens (may be NULL): the caller's host copy of frame_lens where it has one - a length
 *                               < 1 or > Tp is ASR_E_SHAPE.  The kernels clamp the device value to 0 .. Tp: an utterance
 *                               without frames scores every candidate -inf.
 *   asr_ctc_prefix_score_f32    per step, before the select: for every row with score > -inf of an utterance that is not
 *                               done (p: the search; other rows of psi are left as they are), from `slot`:
 *                                 phi[t] = r_b[t] if c == last, else r_n[t] (+) r_b[t]
 *                                 psi[row][c] = p0 (+) (+)_{t = 1 .. T_b-1} (phi[t-1] + x[t][c]),  p0 = x[0][c] if g is empty
 *                                 else -inf;  psi[row][eos] = r_n[T_b-1] (+) r_b[T_b-1];  psi[row][blank] = -inf.
 *                               A reduction over the frames, no state per candidate: memory is 2 R Tp 2 floats of state,
 *                               R V of psi and B Tp of lse, whatever L is.
 *   asr_beam_select_ctc_f32     asr_beam_select_f32 / asr_beam_select_lm_f32 (lm_logits NULL: no LM) on the candidate score
 *                                 c = score[k] + (1 - ctc_weight) * logp[v];  c = c + ctc_weight * (psi[k][v] - psi_prev[k]);
 *                                 with an LM: c = c + lm_weight * logp_lm[v]
 *                               fp32, each operation (1 - ctc_weight and the difference included) rounded on its own, in
 *                               this order.  A candidate that comes out -inf or NaN never enters, so a blank is never
 *                               emitted.  ctc_weight must lie in [0, 1] (ASR_E_ARG); with ctc_weight = 0 psi is not read:
 *                               the launch IS asr_beam_select_f32's (asr_beam_select_lm_f32's), the same kernel.
 *   asr_ctc_prefix_advance_f32  per step, after the select: for every row b*K+j with score > -inf of an utterance that is
 *                               not done, with src = b*K + bp_hist[t][b][j], c = tok_hist[t][b][j], phi of src_slot's row
 *                               src as above: dst_slot's row gets n[0] = p0, b[0] = -inf,
 *                                 n[t] = (n[t-1] (+) phi[t-1]) + x[t][c],  b[t] = (n[t-1] (+) b[t-1]) + x[t][blank],
 *                               last = c, and psi_prev[row] = psi[src][c].  Out of place: src_slot == dst_slot (or state[0]
 *                               == state[1]) is ASR_E_ARG.  One launch.
 * K > ASR_BEAM_KMAX, V < 3, eos or blank outside [0, V), eos == blank, B*K > 65 535: ASR_E_SHAPE.  B, K, V, eos must be
 * the search's (ASR_E_ARG).  No atomics, no host synchronisation, no allocation.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  int B, K, V, Tp;           /* utterances, beam width, vocabulary, padded encoder frames */
  int blank, eos;
  const float* logits;       /* [B][Tp] rows of ld >= V floats: RAW CTC logits */
  int64_t ld;
  const int32_t* frame_lens; /* [B] on the device */
  float* lse;                /* [B][Tp] */
  float* state[2];           /* [B*K][Tp][2] (r_n, r_b), two slots, 8-byte aligned (ASR_E_ALIGN) */
  int32_t* last[2];          /* [B*K] last token of the prefix, -1 while it is empty */
  float* psi;                /* [B*K][V] */
  float* psi_prev;           /* [B*K] */
} asr_ctc_prefix_t;
int asr_ctc_prefix_init_f32(const asr_ctc_prefix_t* c, const int32_t* host_lens, asr_stream_t stream);
int asr_ctc_prefix_score_f32(const asr_ctc_prefix_t* c, const asr_beam_t* p, int slot, asr_stream_t stream);
int asr_beam_select_ctc_f32(const asr_beam_t* p, const float* lm_logits, float lm_weight, const float* psi,
                            const float* psi_prev, float ctc_weight, int t, asr_stream_t stream);
int asr_ctc_prefix_advance_f32(const asr_ctc_prefix_t* c, const asr_beam_t* p, int t, int src_slot, int dst_slot,
                               asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * CTC forced alignment and best-path decoding (csrc/ctc_align.hip): the Viterbi (max-product) companions of
 * the CTC loss on the same head.  Not reference operators - the reference has no CTC branch.  Three entries added to ABI
 * version 8 WITHOUT a version change, like the CTC loss and prefix entries: additive.
 * logits, ld, frame_lens, labels, label_offsets, max_label_len are asr_ctc_loss_fwd's: RAW logits [B][T][V] fp32 with row
 * stride ld >= V, frame_lens int32 [B] on the device (clamped to 0 .. T; frames t >= frame_lens[b] are never read and may
 * hold NaN), ONE packed int64 label tensor with int32 offsets [B + 1], blank = index 0.  x[t][v] = logits[b][t][v] -
 * logsumexp_v logits[b][t]; l' = (0, l_1, 0, ..., l_L, 0), S = 2L + 1 states.
 *   asr_ctc_align_f32   v[0][0] = x[0][0], v[0][1] = x[0][l_1], -inf elsewhere;
 *                       v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if s is odd, s >= 3 and l'_s != l'_{s-2}) + x[t][l'_s];
 *                       score[b] = max(v[T_b-1][S-1], v[T_b-1][S-2]), and the path that attains it.
 *                       TIE RULE (it makes the path a function of the inputs): a predecessor replaces the current best only
 *                       when it is STRICTLY greater, tried in the order stay, s-1, s-2; at the end S-1 is taken unless
 *                       v[S-2] is strictly greater.
 *                         path       int32 [B][T]   the token of frame t (0 = blank); -1 for t >= T_b and for every frame of
 *                                                   an infeasible utterance
 *                         score      fp32 [B]       the log-probability of the best alignment
 *                         first,last int32, packed like labels: the inclusive encoder frames label i occupies
 *                         token_logp fp32, packed like labels: sum_{t = first .. last} x[t][l_i], summed by ONE lane in
 *                                                   ascending frame order
 *                       INFEASIBLE (T_b = 0, a label outside [1, V), more than max_label_len labels, v = -inf at the end:
 *                       frames < labels + adjacent equal labels): score = -inf, first = last = -1, token_logp = -inf,
 *                       path = -1.  An empty transcript with T_b >= 1 is feasible: all frames blank, score = sum_t x[t][0].
 *                       Two launches: the frame log-sum-exps; then one workgroup per utterance (one wave up to 2
 *                       max_label_len + 1 = 64 states, 256 threads beyond, states strided over the threads above 256) runs
 *                       the chain, the backtrace (one lane) and the output passes.  Each state's choice is two bits; per
 *                       (frame, 64 states) a pair of 64-bit words.  They stay in LDS when T_b ceil(S / 64) 16 bytes <=
 *                       ASR_CTC_ALIGN_LDS_BYTES and go to the workspace otherwise.
 *   asr_ctc_align_ws_bytes   the bytes of the workspace (8-byte aligned: ASR_E_ALIGN): with R = B T rounded up to 64,
 *                       W = ceil((2 max_label_len + 1) / 64):  8 R  (log-sum-exps, the state of every frame)
 *                       + 16 B T W  if T W 16 > ASR_CTC_ALIGN_LDS_BYTES (the back-pointers), + 0 otherwise.
 *   asr_ctc_greedy_f32  best path: frame_tok[b][t] = argmax_v logits[b][t][v] over the RAW logits (no log-softmax is
 *                       needed; NaN never wins, ties to the lowest index, a frame of NaN / -inf only gives 0), -1 for
 *                       t >= T_b.  Frame t is kept when frame_tok[t] != 0 and (t == 0 or frame_tok[t] != frame_tok[t-1]);
 *                       ids int32 [B][T] = the kept tokens in frame order, padded with -1; n int32 [B] their count.  One
 *                       launch, one workgroup per utterance.  No arithmetic: exact.
 * V < 2 or max_label_len > ASR_CTC_MAX_LABELS: ASR_E_SHAPE.  No floating-point atomics, no host synchronisation, no
 * allocation; functions of their inputs and shapes only - the same bits in every run, in and outside deterministic mode.
 * ------------------------------------------------------------------------------------- */
#define ASR_CTC_ALIGN_LDS_BYTES 40960
int asr_ctc_align_ws_bytes(int B, int T, int V, int max_label_len, int64_t* ws_bytes);
int asr_ctc_align_f32(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens, const int64_t* labels,
                      const int32_t* label_offsets, int max_label_len, int32_t* path, float* score, int32_t* first,
                      int32_t* last, float* token_logp, void* ws, int64_t ws_bytes, asr_stream_t stream);
int asr_ctc_greedy_f32(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens, int32_t* ids,
                       int32_t* n, int32_t* frame_tok, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * CTC segmentation (csrc/ctc_segment.hip; Kuerzinger et al. 2020): asr_ctc_align_f32 for a long recording and a
 * transcript of several utterances.  Not a reference operator.  Two entries added to ABI version 8 WITHOUT a version change,
 * like the other CTC entries: additive.
 * logits, ld, frame_lens, labels, label_offsets, max_label_len are asr_ctc_align_f32's, with its conventions.  One batch row
 * is a recording; its labels are the concatenation of its utterances:
 *   utt_offsets int32 [N + 1]  ascending label indices into the packed labels, over all recordings
 *   rec_utts    int32 [B + 1]  recording b owns the utterances rec_utts[b] .. rec_utts[b + 1] - 1, whose label ranges tile
 *                              [label_offsets[b], label_offsets[b + 1]) exactly (the caller's duty; not checked on the device)
 *   asr_ctc_segment_f32  asr_ctc_align_f32's recurrence, predecessors, skip rule and TIE RULE.  With free_ends != 0 the
 *                       emission of state 0 and of state S - 1 is 0 instead of x[t][0], at every frame: audio before the first
 *                       and after the last label costs nothing, score[b] is the log-probability of the text over the stretch
 *                       of frames it picks for itself, and the frames whose state is 0 or S - 1 get path = -2 (outside the
 *                       text); t >= T_b gets -1 as before.  L = 0 with free ends: score 0, every valid frame -2.
 *                       With free_ends = 0: path, score, first, last and token_logp are asr_ctc_align_f32's, bit for bit
 *                       (lse from the same kernel, one fp32 subtraction per emission, one fp32 add per cell, token_logp
 *                       summed by one lane in ascending frame order), here up to ASR_CTC_SEG_MAX_LABELS labels.
 *                       Per utterance u, packed [N]:
 *                         utt_begin int32   first of the utterance's first label
 *                         utt_end   int32   last of its last label
 *                         utt_logp  fp32    sum_{t = begin .. end} x[t][path[t]], by ONE lane in ascending frame order
 *                         utt_conf  fp32    the minimum, over the consecutive blocks of `window` frames from begin (the last
 *                                           may be shorter), of the block's mean of x[t][path[t]]: each block summed in
 *                                           ascending order, then divided once by its count in fp32
 *                       An utterance without labels: -1 / -1 / 0 / 0.  INFEASIBLE recordings (asr_ctc_align_f32's kinds) get
 *                       that entry's -inf / -1 pattern, and all their utterances -1 / -1 / -inf / -inf.
 *                       Two launches: the frame log-sum-exps; then one workgroup per recording.  Thread i owns K CONTIGUOUS
 *                       states (K = 4 up to 2 max_label_len + 1 = 1 024 states, on 64 .. 256 threads; K = 16 beyond, on 128 ..
 *                       1 024 threads) and keeps them in registers; K is even, so the one value a thread needs from its
 *                       neighbour - that thread's top state of the frame before - goes through LDS, one barrier per frame.
 *                       Static LDS only (41 KB: the labels and the exchange line); no dynamic LDS is asked for.  Each
 *                       state's choice is two bits, formed in the owning thread's registers (contiguous states leave no
 *                       ballot to take) and stored to the workspace: a frame's back-pointers are a bit row with state s at
 *                       bits 2 s, 2 s + 1.  The backtrace is one wave that fetches the candidate words of 32 frames at once
 *                       (the state falls by at most 2 per frame) and walks them in registers; the output passes are
 *                       parallel over frames, labels and utterances.
 *   asr_ctc_segment_ws_bytes   the bytes of the workspace (8-byte aligned: ASR_E_ALIGN; too small: ASR_E_ARG): with R = B T
 *                       rounded up to 64, W = ceil((2 max_label_len + 1) / 32):
 *                       8 B T W  (the back-pointers) + 12 R  (log-sum-exps, the state and x[t][path[t]] of every frame).
 * V < 2 or max_label_len > ASR_CTC_SEG_MAX_LABELS: ASR_E_SHAPE.  window < 1: ASR_E_ARG.  No floating-point atomics, no host
 * synchronisation, no allocation; a function of its inputs and shapes only - the same bits in every run, in and outside
 * deterministic mode, and a recording's results do not depend on the rest of the batch.
 * ------------------------------------------------------------------------------------- */
#define ASR_CTC_SEG_MAX_LABELS 8191
int asr_ctc_segment_ws_bytes(int B, int T, int V, int max_label_len, int64_t* ws_bytes);
int asr_ctc_segment_f32(int B, int T, int V, const float* logits, int64_t ld, const int32_t* frame_lens, const int64_t* labels,
                        const int32_t* label_offsets, int max_label_len, int free_ends, int N, const int32_t* utt_offsets,
                        const int32_t* rec_utts, int window, int32_t* path, float* score, int32_t* first, int32_t* last,
                        float* token_logp, int32_t* utt_begin, int32_t* utt_end, float* utt_logp, float* utt_conf, void* ws,
                        int64_t ws_bytes, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * CTC prefix beam search (csrc/ctc_beam.hip): the K best label sequences of the CTC head, the first pass of
 * two-pass decoding.  Not a reference operator.  Two entries added to ABI version 8 WITHOUT a version change, like the other
 * CTC entries: additive.
 * logits, ld, frame_lens are asr_ctc_align_f32's: RAW logits [B][T][V] fp32 with row stride ld >= V, frame_lens int32 [B] on
 * the device (clamped to 0 .. T; frames t >= T_b = frame_lens[b] are never read and may hold NaN), blank = index 0,
 * x[t][v] = logits[b][t][v] - logsumexp_v logits[b][t].  (+) is log(exp a + exp b) with (-inf) (+) x = x.
 *   The beam of an utterance holds at most K prefixes (token sequences), each with pb / pnb - the log-mass of its paths that
 *   end in blank / in a non-blank - and tot = pb (+) pnb; it starts as the empty prefix at (0, -inf).  Frame t's candidates:
 *     stay    of entry k (prefix p), flat index k:  pb' = tot + x[t][0];  pnb' = pnb + x[t][last(p)] (-inf for the empty p)
 *     extend  entry k by c in 1 .. V-1, flat index K + k (V - 1) + (c - 1):  pb' = -inf,
 *             pnb' = pb + x[t][c] if c == last(p), tot + x[t][c] otherwise
 *     merge   where p.c IS the prefix of entry k' (as token sequences) the extension is no candidate: its pnb' is added with
 *             (+) to the pnb' of the stay candidate of k' (entries in ascending order; at most one can match)
 *   The new beam: the K candidates of greatest tot', ties to the lower flat index, -inf never selected (fewer than K entries
 *   may be live), in that order.  No vocabulary pruning, no blank threshold.  After frame T_b - 1 the beam is the result:
 *     hyp      int32 [B][K][T]  the tokens of rank r, padded with -1 (at most T_b tokens)
 *     hyp_len  int32 [B][K]     their count; -1 in an unused slot
 *     score    fp32 [B][K]      tot, descending; -inf in an unused slot
 *   An utterance with T_b = 0 gets the empty hypothesis at score 0 in slot 0.
 *   Prefix identity inside the kernel: a 64-bit hash of the token sequence (h' = mix(h + token), the splitmix64 finaliser),
 *   with the length - p.c and q are taken as equal when hash, length and last token agree.
 *   Two launches: the frame log-sum-exps; then one workgroup per utterance (one wave when K V <= ASR_CTC_BEAM_ONE_WAVE_KV,
 *   256 threads beyond) runs every frame, the ranking and the backtrace.  The per-frame history (parent slot, token) stays
 *   in LDS when T K <= ASR_CTC_BEAM_LDS_ENTRIES and goes to the workspace otherwise.
 *   asr_ctc_beam_ws_bytes  the bytes of the workspace (8-byte aligned: ASR_E_ALIGN):  4 R with R = B T rounded up to 64 (the
 *   log-sum-exps) + 8 B T K if T K > ASR_CTC_BEAM_LDS_ENTRIES.
 * V < 2, K outside 1 .. ASR_BEAM_KMAX, K V > INT_MAX / 2: ASR_E_SHAPE.  No floating-point atomics, no host synchronisation, no
 * allocation; a function of its inputs and shapes only - the same bits in every run, in and outside deterministic mode.
 * ------------------------------------------------------------------------------------- */
#define ASR_CTC_BEAM_ONE_WAVE_KV 1024
#define ASR_CTC_BEAM_LDS_ENTRIES 4096
int asr_ctc_beam_ws_bytes(int B, int T, int V, int K, int64_t* ws_bytes);
int asr_ctc_beam_f32(int B, int T, int V, int K, const float* logits, int64_t ld, const int32_t* frame_lens, int32_t* hyp,
                     int32_t* hyp_len, float* score, void* ws, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A backoff n-gram LM on the device (csrc/ngram.hip, csrc/ctc_beam.hip).  Not reference operators.  Two entries
 * added to ABI version 8 WITHOUT a version change, like the other additive groups: callers pin the number.
 * The LM arrives compiled (ngram.py, NgramLM.compile): a deterministic automaton over S states with every backoff resolved,
 *     lm_logp  fp32  [S][V]  ln p(c | state); column 0 (the CTC blank) holds 0 and is never read; every value is finite
 *     lm_next  int32 [S][V]  the state after c, in 0 .. S-1
 *     lm_start               the state of the context <s>
 * S V <= INT_MAX, lm_start in 0 .. S-1: ASR_E_SHAPE otherwise.  The CONTENTS of the table are trusted - the host validates them
 * when it compiles the model - so a successor outside 0 .. S-1 is the caller's error.
 *
 *   asr_ngram_score_f32   N padded id sequences ids int32 [N][ld >= L] with lens int32 [N] (clamped to L; < 0: an unused slot,
 *       score -inf) -> score fp32 [N]: the sum over the tokens IN ORDER of lm_logp[state][id], state walking the automaton
 *       from lm_start, plus lm_logp[state][eos] behind the last token when eos >= 0 (eos < 0: no end term; eos >= V:
 *       ASR_E_SHAPE) - an fp32 sum, one thread per sequence.  tok_score fp32 [N][L] or NULL: the term of every token, 0
 *       behind the sequence.  An id outside 0 .. V-1 inside the length makes that sequence's score (and its tok_score from
 *       there to the length) NaN; nothing is indexed with it.  One launch, no atomics: the same bits in every run.
 *
 *   asr_ctc_beam_lm_f32   asr_ctc_beam_f32 with the LM inside the search.  An entry of the beam additionally carries its
 *       automaton state and lm, the fp32 sum of lm_logp[state][c] over its tokens in order (functions of the token sequence:
 *       equal prefixes hold equal bits, prefix identity and the merge are unchanged).  pb, pnb and tot stay the CTC masses of
 *       asr_ctc_beam_f32, operation for operation.  Every candidate ranks by
 *           rank = (tot' + alpha lm') + beta len'        fp32, each of the four operations rounded on its own (no fma)
 *       - the stay candidate with the entry's lm and len, an extension by c with lm + lm_logp[state][c] and len + 1.  Candidate
 *       order and tie rule are asr_ctc_beam_f32's.  After the last frame, with lm_eos >= 0, lm += lm_logp[state][lm_eos], the
 *       rank is formed again from (tot, lm, len) and the entries are ranked once more, ties to the search's order.  Outputs:
 *           hyp, hyp_len   as asr_ctc_beam_f32
 *           score      fp32 [B][K]  the rank, descending; -inf in an unused slot
 *           ctc_score  fp32 [B][K]  tot;  -inf in an unused slot
 *           lm_score   fp32 [B][K]  lm, the end term included when it is on;  -inf in an unused slot
 *       An utterance of no frames gets the empty hypothesis in slot 0 (ctc_score 0, lm_score the end term or 0).  With
 *       alpha = beta = 0 and no end term, hyp, hyp_len and ctc_score are asr_ctc_beam_f32's bits.  alpha and beta must be
 *       finite (ASR_E_ARG).  The workspace, the launches (two), the limits on K and V and the LDS history are those of
 *       asr_ctc_beam_f32 (asr_ctc_beam_ws_bytes); the LM rows are read through L2 where a candidate is formed, so memory
 *       does not depend on the LM's order.  No atomics, no host synchronisation, no allocation.
 * ------------------------------------------------------------------------------------- */
int asr_ngram_score_f32(int N, int L, int S, int V, const float* lm_logp, const int32_t* lm_next, int lm_start, int eos,
                        const int32_t* ids, int64_t ld, const int32_t* lens, float* score, float* tok_score, asr_stream_t stream);
int asr_ctc_beam_lm_f32(int B, int T, int V, int K, const float* logits, int64_t ld, const int32_t* frame_lens, int S,
                        const float* lm_logp, const int32_t* lm_next, int lm_start, int lm_eos, float alpha, float beta,
                        int32_t* hyp, int32_t* hyp_len, float* score, float* ctc_score, float* lm_score, void* ws,
                        asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A word-level backoff n-gram LM behind a lexicon (csrc/word_lm.h, csrc/word_lm.hip, csrc/ctc_beam.hip).  Not
 * reference operators.  Two entries added to ABI version 8 WITHOUT a version change: additive.
 * The LM arrives compiled (word_lm.py, WordLM.compile, which validates every index and value: the kernels trust the tables).
 * All arrays are device memory:
 *     trie_next int32 [N][V]  the lexicon's trie over token ids: the child node, or -1; node 0 is the root
 *     trie_word int32 [N]     the word id (0 .. W-1) that ends at the node, or -1
 *     arc_off   int32 [S+1]   the arcs of word state s are arc_off[s] .. arc_off[s+1]-1
 *     arc_word  int32 [A]     ascending inside a state;   arc_logp fp32 [A];   arc_next int32 [A] the state after the word
 *     bo_logp   fp32  [S]     the backoff weight of the state;   bo_state int32 [S] the state backed off to
 *     uni_logp  fp32  [W]     the empty context, direct-indexed;   uni_next int32 [W] the state after the word from there,
 *                             or -1: the word has no unigram and scores uni_logp[w] (the LM's oov_logp) from every context,
 *                             the state going to `empty`
 *     space: the token id words are split at;  start: the state of <s>;  empty: the state of the empty context;  eos, unk:
 *     the word ids of </s> and <unk>
 * The words of a token row: split at `space`; a run of spaces is one boundary; leading and trailing spaces make no word.  A
 * word is spelled down the trie from the root; one that leaves the trie or stops at a node with trie_word < 0 is `unk`.
 * The lookup (state s, word w) -> (lp, next), fp32, every addition rounded on its own:  uni_next[w] < 0: (uni_logp[w], empty).
 * Otherwise acc = 0; while s != empty: binary search for w among the arcs of s - found: (acc + arc_logp, arc_next); not
 * found: acc += bo_logp[s], s = bo_state[s]; at empty: (acc + uni_logp[w], uni_next[w]).
 *   asr_word_lm_score_f32   N padded TOKEN id rows ids int32 [N][ld >= L] with lens int32 [N] (clamped to L; < 0: an unused
 *       slot: score -inf, n_words 0) -> score fp32 [N]: the fp32 sum in word order of the lookups of the row's words from
 *       `start`, plus the lookup of `eos` from the final state when eos_term != 0;  n_words int32 [N]: the number of words;
 *       word_score fp32 [N][L] or NULL: the term of word j at column j, 0 behind the last word.  An id outside 0 .. V-1 inside
 *       the length makes the row's score NaN; the id is never used as an index.  One thread per row, one launch, no atomics.
 *   asr_ctc_beam_wlm_f32    asr_ctc_beam_f32 with the lexicon and the word LM inside the search.  An entry additionally
 *       carries its trie node (-1: off the trie), its word state, lm (the fp32 sum over its COMPLETED words) and nw (their
 *       count) - functions of the token sequence, so prefix identity and the merge are unchanged, and pb, pnb, tot are
 *       asr_ctc_beam_f32's operation for operation.  A candidate ranks by (tot' + alpha lm') + beta nw', fp32, each of the four
 *       operations rounded on its own; an extension by `space` from a node that is not the root has lm' = lm + lp and
 *       nw' = nw + 1 with (lp, state') the lookup of the pending word, every other candidate keeps lm and nw.  After the last
 *       frame a pending word closes, with eos_term != 0 the lookup of `eos` joins lm, and the entries are ranked once more.
 *       lexicon_only != 0: an extension that leaves the trie, and a `space` at a node that ends no word, are no candidates; an
 *       entry whose pending node ends no word after the last frame becomes an unused slot.  Outputs as asr_ctc_beam_lm_f32
 *       (score: the rank; ctc_score: tot; lm_score: lm) and n_words int32 [B][K] (-1 in an unused slot).  With alpha = beta =
 *       0, no end term and lexicon_only off, hyp, hyp_len and ctc_score are asr_ctc_beam_f32's bits.  lm->V must be V
 *       (ASR_E_SHAPE); alpha and beta finite (ASR_E_ARG).  Workspace, launches (two) and limits are asr_ctc_beam_f32's.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  int32_t V, N, S, W;     /* tokens, trie nodes, word states, word ids */
  int64_t A;              /* arcs */
  int32_t space, start, empty, eos, unk;
  const int32_t* trie_next;
  const int32_t* trie_word;
  const int32_t* arc_off;
  const int32_t* arc_word;
  const float* arc_logp;
  const int32_t* arc_next;
  const float* bo_logp;
  const int32_t* bo_state;
  const float* uni_logp;
  const int32_t* uni_next;
} asr_word_lm_t;
int asr_word_lm_score_f32(int N, int L, const asr_word_lm_t* lm, int eos_term, const int32_t* ids, int64_t ld,
                          const int32_t* lens, float* score, int32_t* n_words, float* word_score, asr_stream_t stream);
int asr_ctc_beam_wlm_f32(int B, int T, int V, int K, const float* logits, int64_t ld, const int32_t* frame_lens,
                         const asr_word_lm_t* lm, float alpha, float beta, int eos_term, int lexicon_only, int32_t* hyp,
                         int32_t* hyp_len, float* score, float* ctc_score, float* lm_score, int32_t* n_words, void* ws,
                         asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Contextual biasing: per-utterance phrase lists inside the CTC prefix beam search (csrc/context.h, csrc/context.hip,
 * csrc/ctc_beam.hip).  Not reference operators.  Two entries added to ABI version 8 WITHOUT a version change:
 * additive.
 * The graphs arrive compiled (context.py, ContextGraph / ContextBatch .compile, which validates every index: the kernels trust
 * the tables).  One table holds G graphs over N states in one numbering; all arrays are device memory:
 *     arc_off  int32 [N+1]    the arcs of state s are arc_off[s] .. arc_off[s+1]-1: its transitions that differ from its
 *                             default row
 *     arc_tok  int32 [A]      ascending inside a state;   arc_next int32 [A] the state after the token
 *     drow     int32 [N]      the default row of the state, in 0 .. R-1
 *     dflt     int32 [R][V]   next(s, c) = dflt[drow[s]][c] where no arc of s lists c
 *     credit   fp32  [N], pending fp32 [N]      root int32 [G]  the root of graph g
 * graph_of int32 [rows] (device) names the graph of every row; a value outside 0 .. G-1 (-1 by convention) means no biasing
 * for that row: bias 0, no state.  (The host layer refuses an index outside -1 .. G-1 before any launch; the kernels only
 * guard their reads.)
 * The bias of a token row: state = root; per token c in order  n = next(state, c), delta = credit[n] - pending[state] (one
 * fp32 subtraction), bias = bias + delta (one fp32 addition), state = n;  behind the last token bias = bias - pending[state].
 *   asr_context_score_f32   N padded TOKEN id rows ids int32 [N][ld >= L] with lens int32 [N] (clamped to L; < 0: an unused
 *       slot, score -inf) -> score fp32 [N], the bias of the row under graph graph_of[n];  tok_score fp32 [N][L] or NULL: the
 *       delta of every token, 0 behind the row.  An id outside 1 .. V-1 inside the length makes the row's score (and its
 *       tok_score from there to the length) NaN; nothing is indexed with it.  One thread per row, one launch, no atomics.
 *   asr_ctc_beam_ctx_f32    asr_ctc_beam_f32 (S = 0: lm_logp, lm_next and lm_score NULL) or asr_ctc_beam_lm_f32 (S > 0) with
 *       the context inside the search.  An entry additionally carries its context state and bias - functions of the token
 *       sequence, so prefix identity and the merge are unchanged, and pb, pnb, tot (and lm) are the search's without a
 *       context, operation for operation.  A candidate ranks by
 *           rank = r + ctx_weight bias'        r = tot' (S = 0) or (tot' + alpha lm') + beta len' (S > 0)
 *       fp32, the product and the sum rounded on their own, as the last operations: ctx_weight = 0, or graph_of = -1, gives the
 *       bits of the search without a context.  After the last frame bias = bias - pending[state] (and, S > 0 with lm_eos >= 0,
 *       the end term joins lm), the rank is formed again and the entries are ranked once more, ties to the search's order.
 *       Outputs: hyp, hyp_len as asr_ctc_beam_f32; score fp32 [B][K] the rank; ctc_score fp32 [B][K] tot; lm_score fp32 [B][K]
 *       (S > 0) lm; ctx_score fp32 [B][K] bias - asr_context_score_f32 of the hypothesis bit for bit; -inf in unused slots.
 *       An utterance of no frames gets the empty hypothesis in slot 0 with ctx_score 0.  c->V must be V, S V <= INT_MAX,
 *       lm_start in 0 .. S-1 (ASR_E_SHAPE); ctx_weight, alpha, beta finite (ASR_E_ARG).  Workspace, launches (two) and limits
 *       are asr_ctc_beam_f32's.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  int32_t V, N, G, R;     /* tokens, states, graphs, default rows */
  int64_t A;              /* arcs */
  const int32_t* arc_off;
  const int32_t* arc_tok;
  const int32_t* arc_next;
  const int32_t* drow;
  const int32_t* dflt;
  const float* credit;
  const float* pending;
  const int32_t* root;
} asr_context_t;
int asr_context_score_f32(int N, int L, const asr_context_t* c, const int32_t* graph_of, const int32_t* ids, int64_t ld,
                          const int32_t* lens, float* score, float* tok_score, asr_stream_t stream);
int asr_ctc_beam_ctx_f32(int B, int T, int V, int K, const float* logits, int64_t ld, const int32_t* frame_lens,
                         const asr_context_t* c, const int32_t* graph_of, float ctx_weight, int S, const float* lm_logp,
                         const int32_t* lm_next, int lm_start, int lm_eos, float alpha, float beta, int32_t* hyp,
                         int32_t* hyp_len, float* score, float* ctc_score, float* lm_score, float* ctx_score, void* ws,
                         asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The front end (csrc/frontend.hip): packed waveforms -> the [B][T][D] features the encoder reads.  Not
 * reference operators - the reference reads features that Kaldi computed.  Five entries added to ABI version 8 WITHOUT a
 * version change: additive.
 *   asr_fbank_num_frames  host integer arithmetic, no GPU: T = 1 + (n_samples - frame_length) / frame_shift when
 *                       n_samples >= frame_length, else 0 (Kaldi's snip-edges).
 *   asr_fbank_plan_bytes  the bytes of the table buffer ("plan") of asr_fbank_f32 for n_fft in {256, 512} (else ASR_E_SHAPE):
 *                       4 (7 n_fft / 2 + 3 ASR_FBANK_MAX_MELS).  The CALLER fills it (float64 arithmetic, rounded to fp32),
 *                       4-byte words in this order, M = n_fft / 2:
 *                         window  fp32 [n_fft]    (0.5 - 0.5 cos(2 pi n / (L - 1)))^0.85 for n < L, 0 behind
 *                         tw      fp32 [M/2][2]   (cos, -sin)(2 pi j / M)         the FFT's twiddles
 *                         ut      fp32 [M][2]     (cos, -sin)(2 pi k / n_fft)     the untangle pass's
 *                         start, len, woff  int32 [ASR_FBANK_MAX_MELS] each: mel bin j sums FFT bins start[j] .. start[j] +
 *                                                 len[j] - 1 (all < M: the Nyquist bin is unused, as in Kaldi) with the weights
 *                                                 w[woff[j] ..]; entries behind n_mels are ignored
 *                         w       fp32 [n_fft]    the packed weights (a bin lies in at most two triangles)
 *                       The kernel clamps start / len / woff into the buffer: a wrong plan gives wrong numbers, no fault.
 *   asr_fbank_f32       Kaldi-convention filterbank energies, dither off.  samples: ONE packed buffer of int16
 *                       (ASR_SAMPLES_I16) or fp32 (ASR_SAMPLES_F32; values in int16 range, as Kaldi expects), utterance b =
 *                       samples[offsets[b] .. offsets[b + 1]), offsets int64 [B + 1] on the device.  Only the natural
 *                       alignment of a sample is assumed (an int16 utterance may start at an odd element); no sample at or
 *                       behind offsets[B] and none outside a frame is read.  T_b = asr_fbank_num_frames(N_b), clamped to
 *                       T_max.  Per frame: subtract the frame mean; x[i] -= preemph x[i-1] (x[0] -= preemph x[0]); window;
 *                       zero-pad to n_fft; power spectrum; E[j] = sum_i w[woff[j] + i] P[start[j] + i] in ascending i;
 *                       out = E, or with use_log: logf(E) where E > FLT_EPSILON and the fp32 nearest to ln(FLT_EPSILON)
 *                       elsewhere.  Row (b, t) is written at out[(b T_max + t) ld + col0 .. + n_mels); rows t >= T_b are not
 *                       touched.  n_fft in {256, 512}, frame_length <= n_fft, 1 <= n_mels <= ASR_FBANK_MAX_MELS, B <= 65535:
 *                       ASR_E_SHAPE otherwise.  One launch: a workgroup of four waves per tile of ASR_FBANK_FRAME_TILE
 *                       consecutive frames of one utterance, one wave per frame.  The real FFT is a complex FFT of half the
 *                       size on z[n] = x[2n] + i x[2n+1] (radix 2, decimation in frequency, in LDS) and an untangle pass.
 *   asr_feat_cmvn_stats_f32  x fp32 [B][T] rows of ld >= n_mels floats, frame_lens int32 [B] on the device (clamped to 0 .. T)
 *                       -> stats fp32 [B][2][n_mels]: the mean over the utterance's frames, and 1 / sqrt(max(var, 1e-10))
 *                       with the biased variance taken about that mean (two passes).  One workgroup per utterance; four row
 *                       groups (t mod 4) per bin, summed in ascending t and combined as (g0 + g1) + (g2 + g3).
 *   asr_feat_finish_f32 one pass, x as above -> out fp32 [B][T][n_mels (1 + order)], contiguous.  In this order:
 *                         CMVN of the static features y = (x - mean) istd: ASR_CMVN_NONE; ASR_CMVN_GLOBAL (stats fp32
 *                           [2][n_mels]: mean, istd); ASR_CMVN_UTTERANCE (stats of asr_feat_cmvn_stats_f32);
 *                         deltas, order in {0, 1, 2} (Kaldi add-deltas, window 2): block k = sum_d s_k[d] y[clamp(t + d, 0,
 *                           T_b - 1)], s_1 = (-2, -1, 0, 1, 2) / 10 over d = -2 .. 2, s_2 = s_1 * s_1 (9 taps, d = -4 .. 4) -
 *                           each order a filter over the STATIC rows, summed in ascending d;
 *                         masks int32 [B][n_freq_masks + n_time_masks][2] of (start, width), frequency masks first: a
 *                           frequency mask zeroes bins [f0, f0 + w) of every block, a time mask frames [t0, t0 + w); width 0
 *                           masks nothing; masks may be null when both counts are 0;
 *                         exact zeros in rows t >= T_b.
 * No floating-point atomics, no host synchronisation, no allocation; functions of their inputs and shapes only - the same
 * bits in every run, in and outside deterministic mode.
 * ------------------------------------------------------------------------------------- */
#define ASR_FBANK_FRAME_TILE 8
#define ASR_FBANK_MAX_MELS 128
#define ASR_SAMPLES_I16 0
#define ASR_SAMPLES_F32 1
#define ASR_CMVN_NONE 0
#define ASR_CMVN_GLOBAL 1
#define ASR_CMVN_UTTERANCE 2
int asr_fbank_num_frames(int64_t n_samples, int frame_length, int frame_shift, int64_t* n_frames);
int asr_fbank_plan_bytes(int n_fft, int64_t* bytes);
int asr_fbank_f32(int B, int T_max, const void* samples, int sample_dtype, const int64_t* offsets, int frame_length,
                  int frame_shift, int n_fft, int n_mels, float preemph, int use_log, const void* plan, float* out, int64_t ld,
                  int64_t col0, asr_stream_t stream);
int asr_feat_cmvn_stats_f32(int B, int T, int n_mels, const float* x, int64_t ld, const int32_t* frame_lens, float* stats,
                            asr_stream_t stream);
int asr_feat_finish_f32(int B, int T, int n_mels, int order, const float* x, int64_t ldx, const int32_t* frame_lens,
                        int cmvn_mode, const float* stats, const int32_t* masks, int n_freq_masks, int n_time_masks, float* out,
                        asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Minimum error rate training on an n-best list (csrc/mwer.hip): the expected number of edit errors under the
 * model's sequence probabilities renormalised over the K hypotheses of an utterance (Prabhavalkar et al. 2018).  Not a
 * reference operator.  Two entries added to ABI version 8 WITHOUT a version change, like the beam and edit-distance entries:
 * additive.  Rows are r = b K + k (utterance b, hypothesis k), R = B K.
 *   logits   [L][R][V] fp32 RAW logits, time-major, row stride ld >= V floats (what the decoder sequence returns).
 *   tokens   int64 [L][R]: the hypothesis with its <EOS>, <EOS>-padded.  A value outside [0, V) is read as the nearest
 *            valid token: no access leaves the row.
 *   npos     int32 [R]: the scored positions n_r = len_r + 1, clamped to 1 .. L; <= 0 marks an unused slot.
 *   err      int32 [R]: the edit distance of hypothesis r to its utterance's reference.
 *   scale    the caller passes 1 / B.
 *   asr_mwer_fwd_f32
 *       s_r    = sum_{l < n_r} (logits[l][r][tokens[l][r]] - logsumexp_v logits[l][r][:]), summed in increasing l;
 *       over the live slots of utterance b, with m_b their maximum of s and Wbar_b their mean of err:
 *       phat_r = exp(s_r - m_b) / sum_j exp(s_j - m_b)            (the sum in increasing j)
 *       risk_b = sum_k phat_k (err_k - Wbar_b)                    (in increasing k)
 *       coef_r = phat_r (err_r - Wbar_b - risk_b)                 (= d risk_b / d s_r)
 *       loss   = scale sum_b risk_b                               (in increasing b)
 *       An unused slot gets s = phat = coef = 0; an utterance with no live slot has risk_b = 0.
 *       Outputs seq_logp [R], post [R] (phat), coef [R], risk [B], loss [1].  ws: L R floats (ASR_E_ARG when ws_bytes is
 *       smaller) that take the per-position log-probabilities; positions l >= n_r are neither read nor written.  Two launches:
 *       a wave per (l, r) row, then ONE workgroup - a thread per row for the sum over l, a thread per utterance for the K
 *       slots, one thread for the B risks.
 *   asr_mwer_bwd_f32   grad_loss: one device scalar g, the gradient of loss; grad_scale = the forward's scale; coef the
 *       forward's.  dlogits[l][r][v] = g grad_scale coef_r (1[v = tokens[l][r]] - softmax(logits[l][r][:])_v) for l < n_r,
 *       row stride lddz >= V; exact zeros for l >= n_r and for unused rows, whose logits are not read (nor are those of a row
 *       whose coef is 0).  One launch, a wave per (l, r) row.
 * B, K, L, V <= 0, a NULL pointer, ld or lddz < V: ASR_E_ARG.  K > ASR_BEAM_KMAX, or L B K above 4 INT_MAX: ASR_E_SHAPE.
 * Both are answered before anything is launched.  No floating-point atomics and no sum across lanes other than the
 * log-softmax's xor butterfly: functions of their inputs and shapes only - the same bits in every run, in and outside
 * deterministic mode.  No host synchronisation, no allocation.
 * ------------------------------------------------------------------------------------- */
int asr_mwer_fwd_f32(int B, int K, int L, int V, const float* logits, int64_t ld, const int64_t* tokens, const int32_t* npos,
                     const int32_t* err, float scale, float* seq_logp, float* post, float* coef, float* risk, float* loss,
                     float* ws, int64_t ws_bytes, asr_stream_t stream);
int asr_mwer_bwd_f32(int B, int K, int L, int V, const float* logits, int64_t ld, const int64_t* tokens, const int32_t* npos,
                     const float* coef, const float* grad_loss, float grad_scale, float* dlogits, int64_t lddz,
                     asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Speed perturbation (csrc/resample.hip): a polyphase resampler over packed waveforms, in front of
 * asr_fbank_f32.  Not a reference operator.  Two entries added to ABI version 8 WITHOUT a version change, like the front
 * end's: additive.
 * A speed factor s at sample rate sr is the rational orig / new = round(s sr) / sr in lowest terms (0.9 -> 9 / 10); the
 * result is read at sr again, so tempo and pitch change together (sox `speed`).  With lpw = 6, rolloff = 0.99:
 *   base = min(orig, new) rolloff, width = ceil(lpw orig / base), taps = 2 width + orig,
 *   t = clip(((k - width) / orig - j / new) base, -lpw, lpw),  h[j][k] = sinc(pi t) cos^2(pi t / (2 lpw)) base / orig,
 *   out[i new + j] = sum_k h[j][k] x[i orig + k - width] (k ascending, one fp32 running sum, fmaf), x zero outside [0, n),
 *   ceil(new n / orig) output samples for n input samples.
 * geometry: HOST int32 [n_factors][5] = (orig, new, width, taps, table offset in floats); tables: DEVICE fp32, factor f's
 * bank h[new][taps] at its offset, filled by the CALLER (float64 arithmetic, rounded to fp32 once).
 *   asr_resample_plan_bytes  no GPU: 4 * max_f (offset_f + new_f taps_f), the bytes the tables need.
 *   asr_resample_f32    samples: ONE packed buffer of in_count int16 (ASR_SAMPLES_I16) or fp32 (ASR_SAMPLES_F32) elements,
 *                       utterance b = samples[in_offsets[b] .. in_offsets[b + 1]) filtered with factor factor_index[b]
 *                       (int32 [B], clamped into the plan) into out[out_offsets[b] ..): ONE packed fp32 buffer of out_count
 *                       elements.  All three index arrays are on the device.  A row's length is ceil(new n / orig), clamped to
 *                       out_offsets[b + 1] - out_offsets[b]; what the host leaves between rows is not touched.  Offsets are
 *                       clamped into the two buffers: nothing at or behind in_offsets[B] is read, nothing at or behind
 *                       out_offsets[B] written, a neighbour in the packed buffer is not an utterance's padding.  A factor with
 *                       orig == new == 1 copies by value (int16 -> fp32 exactly, fp32 bit for bit).  max_out: the longest
 *                       row's output length (an upper bound will do: it sizes the grid).  One launch, grid (ceil(max_out /
 *                       ASR_RESAMPLE_TILE), B): a workgroup stages its tile's input span and the factor's bank in LDS once.
 * n_factors > ASR_RESAMPLE_MAX_FACTORS, new > ASR_RESAMPLE_MAX_PHASES, taps > ASR_RESAMPLE_MAX_TAPS, a tile span
 * ((ASR_RESAMPLE_TILE - 1) / new + 1) orig + taps above ASR_RESAMPLE_MAX_SPAN (speed factors above 2), B > 65535, a
 * sample_dtype that is neither of the two: ASR_E_SHAPE.  taps != 2 width + orig, tables smaller than the geometry addresses,
 * a NULL pointer: ASR_E_ARG.  Both before anything is launched.  No atomics, no host synchronisation, no allocation; a
 * function of its inputs only - the same bits in every run, in and outside deterministic mode.
 * ------------------------------------------------------------------------------------- */
#define ASR_RESAMPLE_TILE 1024
#define ASR_RESAMPLE_MAX_FACTORS 8
#define ASR_RESAMPLE_MAX_PHASES 32
#define ASR_RESAMPLE_MAX_TAPS 64
#define ASR_RESAMPLE_MAX_SPAN 2176
int asr_resample_plan_bytes(int n_factors, const int32_t* geometry, int64_t* bytes);
int asr_resample_f32(int B, int64_t max_out, const void* samples, int sample_dtype, int64_t in_count,
                     const int64_t* in_offsets, const int32_t* factor_index, const int64_t* out_offsets, int n_factors,
                     const int32_t* geometry, const void* tables, int64_t table_bytes, float* out, int64_t out_count,
                     asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Reverberation and additive noise (csrc/augment.hip): two passes over packed waveforms between
 * asr_resample_f32 and asr_fbank_f32.  Not reference operators.  Two entries added to ABI version 8 WITHOUT a version
 * change, like the resampler's: additive.  Both keep every row's length: the output is packed by the SAME offsets as the
 * input, so sample counts and frame counts stay host arithmetic.
 *   asr_reverb_f32      utterance b = samples[offsets[b] .. offsets[b + 1]) (int16 or fp32, as asr_resample_f32) with
 *                       r = rir_index[b] (DEVICE int32 [B]):  r < 0 copies the row by value (int16 -> fp32 exactly, fp32 bit
 *                       for bit);  otherwise  y[n] = sum_{k = 0}^{L - 1} h[k] x[n + d - k]  for n in [0, N), x zero outside
 *                       [0, N): the row convolved with RIR r and shifted back by the RIR's direct-path index d, so the output
 *                       is not delayed (Kaldi wav-reverberate --shift-output=true).  geometry: HOST int64 [n_rirs][3] =
 *                       (offset into bank in floats, taps L, d), checked here; geometry_dev: the same array on the DEVICE,
 *                       read by the kernel (clamped into the bank, so a copy that differs gives wrong numbers, not a wrong
 *                       access); bank: DEVICE fp32 [bank_count], filled by the CALLER (cut, scaled to unit energy in
 *                       float64, rounded once).  One launch, grid (ceil(max_len / ASR_REVERB_TILE), B), max_len = the
 *                       longest row (an upper bound will do).  A wave of the workgroup forms 1024 outputs as one 32 x 32
 *                       accumulator of v_mfma_f32_32x32x2_f32 - a banded matrix product, an exact fp32 fmaf chain per
 *                       output - over the taps in chunks of ASR_REVERB_CHUNK; input span and band are staged in LDS per
 *                       chunk (33 KB whatever L), so ASR_REVERB_MAX_TAPS bounds the work of a tile, not the LDS.
 *                       out must not alias samples.
 *   asr_noise_mix_f32   z[n] = y[n] + g v[n],  v[n] = clip[(start[b] + n) mod len(clip)],  clip = clip_index[b] (DEVICE int32
 *                       [B]; < 0: no clip),  g = scale[b] sqrt(P_y / P_v)  with P_y = sum y[n]^2, P_v = sum v[n]^2 over the
 *                       row's N samples in float64 (per-tile partials of ASR_NOISE_TILE samples in ws, added in tile order),
 *                       g formed in float64 and rounded once; g = 0 when either sum is 0.  scale[b] = 10^(-snr_db / 20)
 *                       comes from the host (DEVICE fp32 [B]); start: DEVICE int64 [B], taken mod len.  clip_offsets: HOST
 *                       int64 [n_clips + 1] into bank (DEVICE fp32 [bank_count]), checked here; clip_offsets_dev: the same
 *                       on the DEVICE.  ws: at least 16 B ceil(max_len / ASR_NOISE_TILE) bytes, 8-byte aligned.  out may be
 *                       the fp32 samples buffer itself (in place): rows without a clip and rows with g = 0 are then not
 *                       written at all; into another buffer they are copied by value.  gains: NULL or DEVICE fp32 [B] = g.
 *                       Two launches (sums, then mix) on the same grid.
 * Offsets are clamped into the buffers as in asr_resample_f32; nothing at or behind offsets[B] is read or written, nothing
 * behind a RIR or a clip is read.  A RIR of more than ASR_REVERB_MAX_TAPS taps, B > 65535, a sample_dtype that is neither of
 * the two: ASR_E_SHAPE.  A NULL pointer, geometry or clip offsets outside the bank, d outside [0, L), an empty clip, too small
 * a workspace, reverb in place, an int16 mix in place: ASR_E_ARG.  Both before anything is launched.  No atomics, no host
 * synchronisation, no allocation; the same bits in every run, in and outside deterministic mode.
 * ------------------------------------------------------------------------------------- */
#define ASR_REVERB_TILE 4096
#define ASR_REVERB_CHUNK 2048
#define ASR_REVERB_MAX_TAPS 8192
#define ASR_NOISE_TILE 4096
int asr_reverb_f32(int B, int64_t max_len, const void* samples, int sample_dtype, int64_t in_count, const int64_t* offsets,
                   const int32_t* rir_index, int n_rirs, const int64_t* geometry, const int64_t* geometry_dev,
                   const float* bank, int64_t bank_count, float* out, int64_t out_count, asr_stream_t stream);
int asr_noise_mix_f32(int B, int64_t max_len, const void* samples, int sample_dtype, int64_t in_count,
                      const int64_t* offsets, const int32_t* clip_index, const int64_t* start, const float* scale, int n_clips,
                      const int64_t* clip_offsets, const int64_t* clip_offsets_dev, const float* bank, int64_t bank_count,
                      void* ws, int64_t ws_bytes, float* out, int64_t out_count, float* gains, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Transducer (RNN-T) head (csrc/rnnt.hip).  Blank = 0, never a label.  B utterances, T_b >= 1 frames
 * (frame_lens, DEVICE int32 [B]), U_b >= 0 labels (label_offsets, DEVICE int32 [B + 1] into the packed DEVICE int64 labels, as
 * asr_ctc_loss_fwd takes them), T = max T_b, U = max U_b given by the caller.  A node is (b, t, u), t < T_b, u <= U_b; the node
 * matrices are [B][T][U + 1][.] row-major.  Nodes with t >= T_b or u > U_b are padding: never read, written as EXACT ZEROS
 * in z, dlogits, dpe and dpp (no prior fill needed).
 *   asr_rnnt_ws_bytes        plain integers, no GPU: 4 (3 B T (U + 1) + B) bytes rounded up per region (lse, alpha, beta,
 *                            log P).  ASR_E_SHAPE for V < 2, J not a multiple of 4, U > ASR_RNNT_MAX_LABELS (the chains
 *                            keep a diagonal in LDS), or a node matrix the launch grids cannot cover: offsets are 64-bit,
 *                            the bound is B T (U + 1) max(J, V) <= 2^40 elements and B T (U + 1) / 4 workgroups <= 2^31 - 1.
 *   asr_rnnt_joint_fwd_f32   z[b][t][u][:] = tanh(pe[b][t][:] + pp[b][u][:]); pe [B][T][J], pp [B][U + 1][J], z [B][T][U + 1][J],
 *                            all contiguous and 16-byte aligned (ASR_E_ALIGN).  One launch.
 *   asr_rnnt_joint_bwd_f32   dz (1 - z^2) summed over u = 0 .. U_b in ascending order into dpe [B][T][J] and over t = 0 ..
 *                            T_b - 1 in ascending order into dpp [B][U + 1][J]; reads valid nodes only.  One launch.
 *   asr_rnnt_loss_fwd_f32    RAW logits [B][T][U + 1][V] with row stride ld >= V (the log-softmax is the kernel's): the
 *                            node log-sum-exps, then alpha by anti-diagonals in log space, one workgroup per utterance:
 *                              alpha(0,0) = 0, alpha(t,u) = logaddexp(alpha(t-1,u) + lp_0(t-1,u), alpha(t,u-1) + lp_{y_u}(t,u-1))
 *                              nll[b] = -(alpha(T_b-1,U_b) + lp_0(T_b-1,U_b))
 *                            Every utterance with T_b >= 1 has an alignment; +inf only for a label outside [1, V), more than U
 *                            labels or no frame (the gradient of such an utterance is zero).  Two launches.
 *   asr_rnnt_loss_bwd_f32    behind a loss_fwd with the same arguments and workspace: beta from the far corner, then
 *                              dlogits[b][t][u][k] = grad_nll[b] (softmax_k gamma - [k = 0] exp(alpha + lp_0 + beta(t+1,u) - log P)
 *                                                   - [k = y_{u+1}] exp(alpha + lp_k + beta(t,u+1) - log P)),
 *                              gamma = exp(alpha + beta - log P), beta(T_b, U_b) = 0 for the closing blank, a term off the
 *                            lattice absent.  dlogits has row stride lddz >= V.  Two launches.
 *   asr_rnnt_greedy_step_f32 ONE iteration of greedy decoding for all rows; all state on the DEVICE: t_cur, n_out, n_frame,
 *                            last int32 [B], out int32 [B][L], score fp32 [B], advance int32 [B].  A row with t_cur == T_b
 *                            or n_out == L does nothing (advance = 0).  A row that has emitted max_symbols tokens at this
 *                            frame moves on: t_cur += 1, n_frame = 0, advance = 0.  Otherwise logits = w_out tanh(pe[b][t_cur]
 *                            + pp[b]) + b_out (pp [B][J]: the row's current prediction-network projection; w_out [V][J];
 *                            b_out [V] or NULL) and their argmax - GREATER VALUE FIRST, THE LOWER INDEX ON TIES: blank ->
 *                            t_cur += 1, n_frame = 0, advance = 0; a token k -> out[b][n_out++] = k, last[b] = k, n_frame += 1,
 *                            score[b] += log softmax_k, advance = 1.  (J + V) floats of LDS: ASR_E_SHAPE above 64 KB, for
 *                            V < 2 or J not a multiple of 4.  One launch.
 * No floating-point atomics, every sum in an order fixed by the shapes: the same bits in every run, in and outside
 * deterministic mode.  No host synchronisation, no allocation.
 * ------------------------------------------------------------------------------------- */
#define ASR_RNNT_MAX_LABELS 1023
int asr_rnnt_ws_bytes(int B, int T, int U, int J, int V, int64_t* ws_bytes);
int asr_rnnt_joint_fwd_f32(int B, int T, int U, int J, const float* pe, const float* pp, const int32_t* frame_lens,
                           const int32_t* label_offsets, float* z, asr_stream_t stream);
int asr_rnnt_joint_bwd_f32(int B, int T, int U, int J, const float* dz, const float* z, const int32_t* frame_lens,
                           const int32_t* label_offsets, float* dpe, float* dpp, asr_stream_t stream);
int asr_rnnt_loss_fwd_f32(int B, int T, int U, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                          const int64_t* labels, const int32_t* label_offsets, float* nll, void* ws, int64_t ws_bytes,
                          asr_stream_t stream);
int asr_rnnt_loss_bwd_f32(int B, int T, int U, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                          const int64_t* labels, const int32_t* label_offsets, const float* grad_nll, void* ws,
                          int64_t ws_bytes, float* dlogits, int64_t lddz, asr_stream_t stream);
int asr_rnnt_greedy_step_f32(int B, int T, int J, int V, int L, int max_symbols, const float* pe, const float* pp,
                             const float* w_out, const float* b_out, const int32_t* frame_lens, int32_t* t_cur,
                             int32_t* n_out, int32_t* n_frame, int32_t* out, int32_t* last, float* score, int32_t* advance,
                             asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Transducer forced alignment (csrc/rnnt_align.hip): the Viterbi (max-product) companion of asr_rnnt_loss_fwd_f32
 * on the same inputs - where in the audio each label of a transcript sits.  Not a reference operator.  Two entries added to
 * ABI version 8 WITHOUT a version change: additive, like the groups above (and named asr_transducer_* like the beam
 * search's: the asr_rnnt_* group stays the six entries of csrc/rnnt.hip).
 * B, T, U, V, logits, ld, frame_lens, labels, label_offsets are asr_rnnt_loss_fwd_f32's: RAW logits [B][T][U + 1][V] fp32 with
 * row stride ld >= V, frame_lens DEVICE int32 [B], ONE packed DEVICE int64 label tensor with DEVICE int32 offsets [B + 1],
 * blank = 0.  lp_k(t,u) = logits[b][t][u][k] - logsumexp_v logits[b][t][u]; nodes with t >= T_b or u > U_b are never read and
 * may hold NaN.
 *   asr_transducer_align_f32       v(0,0) = 0, v(t,u) = max(v(t-1,u) + lp_0(t-1,u), v(t,u-1) + lp_{y_u}(t,u-1)), a term off the
 *                            lattice absent; score[b] = v(T_b-1,U_b) + lp_0(T_b-1,U_b), and the path that attains it.
 *                            TIE RULE (it makes the path a function of the inputs): when the two candidates compare equal the
 *                            BLANK predecessor (t-1,u) wins - on an all-equal lattice every label is emitted at frame 0.
 *                              score        fp32 [B]      the log-probability of the best alignment
 *                              emit_frame   int32, packed like labels: the frame t on whose arc (t,i-1) -> (t,i) label i
 *                                                         (1-based) is emitted
 *                              token_logp   fp32, packed like labels: lp_{y_i}(emit_frame_i, i-1)
 *                              frame_labels int32 [B][T]  the u at which frame t's blank is taken: the labels emitted up to
 *                                                         and including frame t; -1 for t >= T_b
 *                              blank_logp   fp32 [B][T]   lp_0(t, frame_labels[t]); EXACT 0 for t >= T_b
 *                            so that score = sum_i token_logp_i + sum_t blank_logp_t up to the order of the additions.
 *                            NOT ALIGNED (T_b = 0, a label outside [1, V), more than U labels): score = -inf, emit_frame = -1,
 *                            token_logp = -inf, frame_labels = -1, blank_logp = 0, for that row alone.  Every other utterance
 *                            has an alignment.  Every output element is written (no prior fill needed).
 *                            Two launches: a wave per node writes the node's two emissions lp_0 and lp_{y_{u+1}} (no
 *                            [.., V] log-prob tensor exists); then one workgroup per utterance (one wave up to U + 1 = 64
 *                            label positions, 256 threads beyond, positions strided over the workgroup above 256) runs the
 *                            chain by anti-diagonals t + u = d, the backtrace (one wave) and the output passes.  Each node's
 *                            choice is one bit, a 64-bit word per (diagonal, 64 label positions), in the workspace.
 *   asr_transducer_align_ws_bytes  plain integers, no GPU: the bytes of the workspace (8-byte aligned: ASR_E_ALIGN): with N =
 *                            B T (U + 1) rounded up to 64 and W = ceil((U + 1) / 64):  8 N  (the two emissions of every
 *                            node) + 8 B (T + U) W  (the back-pointers).  ASR_E_SHAPE for V < 2, U > ASR_RNNT_MAX_LABELS, or a
 *                            node matrix beyond asr_rnnt_ws_bytes's bounds (B T (U + 1) max(4, V) <= 2^40 elements and
 *                            B T (U + 1) / 4 workgroups <= 2^31 - 1).
 * No floating-point atomics, adds and compares only behind the row log-sum-exp, 64-bit offsets, no host synchronisation, no
 * allocation; a function of the inputs and shapes only - the same bits in every run, in and outside deterministic mode, and
 * for a row alone or inside a batch.
 * ------------------------------------------------------------------------------------- */
int asr_transducer_align_ws_bytes(int B, int T, int U, int V, int64_t* ws_bytes);
int asr_transducer_align_f32(int B, int T, int U, int V, const float* logits, int64_t ld, const int32_t* frame_lens,
                       const int64_t* labels, const int32_t* label_offsets, float* score, int32_t* emit_frame,
                       float* token_logp, int32_t* frame_labels, float* blank_logp, void* ws, int64_t ws_bytes,
                       asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Beam search over the transducer head, with an n-gram LM inside when one is given (csrc/rnnt_beam.hip).  Not a
 * reference operator.  Five entries added to ABI version 8 WITHOUT a version change: additive, like the groups above.
 * The search is alignment-length synchronous: at iteration i every entry of an utterance's beam (at most K, 1 <= K <=
 * ASR_BEAM_KMAX) has t + u = i (u its label count, at most L; t its frame).  Each iteration every live entry proposes its
 * blank (same sequence, node (t + 1, u)) and, while u < L, its V - 1 labels (node (t, u + 1)); the blank of entry h and the
 * label candidate (h', k) with seq(h') . k = seq(h) are one candidate with the logaddexp of the two masses (sequences compare
 * by a 64-bit hash and their length; collisions are accepted), which keeps the flat index and the prediction state of its
 * BLANK parent.  The best K candidates by rank (greater first, the lower flat index parent V + token on ties) are the next
 * beam; rank = tot, or with an LM (tot + lm_alpha lm) + lm_beta u, every operation rounded on its own.  A blank taken at
 * t = T_b - 1 is a final: it leaves the beam for the utterance's final list, the best K finals by rank (the earlier one
 * first on ties); with lm_eos >= 0 the LM's end-of-sentence term joins a final's lm.  T + L iterations finish every row.
 * One iteration is four launches: asr_transducer_beam_step_f32, the gate product gates = xh [w_ih | w_hh]^T + (b_ih + b_hh)
 * (asr_gemm_f32, the caller's), asr_transducer_beam_cell_f32, and the projection pp = h w_pred^T (asr_gemm_f32, the caller's).
 *   asr_transducer_beam_t              the call: sizes, the head's tensors, the caller's state h, c [B K][P] and xh [B K][E + P],
 *                                pp [B K][J] (the projection of h), the LM (lm_logp NULL: none; logp fp32 / next int32
 *                                [lm_states][V] as asr_ctc_beam_lm_f32 takes them), the workspace (8-byte aligned)
 *   asr_transducer_beam_ws_bytes       plain integers, no GPU.  ASR_E_SHAPE for K outside 1 .. ASR_BEAM_KMAX, V < 2, J not a
 *                                multiple of 4, K (J + V) * 4 bytes of LDS above ASR_RNNT_BEAM_LDS_BYTES, or (T + L) B K or
 *                                B K (E + 4 P) above INT_MAX
 *   asr_transducer_beam_init_f32       the empty sequence at (0, 0) for every utterance with a frame; xh = [emb[bos] | 0] and
 *                                advance = 1 for its slot, zeros elsewhere.  The caller then runs gate product, cell, projection.
 *   asr_transducer_beam_step_f32       iteration `it` (0 .. T + L - 1, in order): reads pp, h, c; writes the beam, a history record
 *                                per slot, the finals, xh = [emb[token] | h[parent]], c[parent] and the advance flags
 *   asr_transducer_beam_cell_f32       h, c [B K][P] from gates [B K][4 P] (i, f, g, o) where advance is set; the parent's elsewhere
 *   asr_transducer_beam_backtrace_f32  hyp int32 [B][K][L] padded with -1, hyp_len int32 [B][K] (-1: unused), score fp32 [B][K]
 *                                (the rank, descending, -inf: unused); rnnt_score (tot) and lm_score fp32 [B][K] or NULL.
 *                                An utterance without a frame gives the empty hypothesis at tot 0 and nothing else.
 * No floating-point atomics, sums in an order fixed by the shapes, 64-bit offsets, no host synchronisation, no allocation;
 * frames t >= T_b, slots that are not live and workspace words the call has not written are never read.
 * ------------------------------------------------------------------------------------- */
#define ASR_RNNT_BEAM_LDS_BYTES (56 * 1024)
typedef struct {
  int B, T, J, V, K, L, E, P;
  const float* pe;            /* [B][T][J] */
  const float* pp;            /* [B K][J] */
  const float* w_out;         /* [V][J] */
  const float* b_out;         /* [V] or NULL */
  const float* emb;           /* [V][E] */
  const int32_t* frame_lens;  /* [B] */
  const float* h;             /* [B K][P] */
  const float* c;             /* [B K][P] */
  float* xh;                  /* [B K][E + P] */
  int lm_states, lm_start, lm_eos;
  float lm_alpha, lm_beta;
  const float* lm_logp;
  const int32_t* lm_next;
  void* ws;
  int64_t ws_bytes;
} asr_transducer_beam_t;
int asr_transducer_beam_ws_bytes(int B, int T, int J, int V, int K, int L, int E, int P, int64_t* ws_bytes);
int asr_transducer_beam_init_f32(const asr_transducer_beam_t* a, int bos, asr_stream_t stream);
int asr_transducer_beam_step_f32(const asr_transducer_beam_t* a, int it, asr_stream_t stream);
int asr_transducer_beam_cell_f32(const asr_transducer_beam_t* a, const float* gates, float* h, float* c, asr_stream_t stream);
int asr_transducer_beam_backtrace_f32(const asr_transducer_beam_t* a, int32_t* hyp, int32_t* hyp_len, float* score, float* rnnt_score,
                                float* lm_score, asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The transducer beam search with a lexicon and a word-level n-gram LM inside (csrc/rnnt_beam.hip, csrc/word_lm.h; DESIGN
 * 4.30).  Not reference operators.  Four entries added to ABI version 8 WITHOUT a version change: additive.  The search is
 * the group's above, entry for entry - the walk, the merge, the blank parent's slot, K, the T + L iterations, the finals -
 * and asr_transducer_beam_t, asr_transducer_beam_ws_bytes, asr_transducer_beam_cell_f32 and the two products are used as they
 * are; the LM is an asr_word_lm_t with its lookup as defined there, and a->lm_logp must be NULL (ASR_E_ARG).
 * An entry additionally carries node (its lexicon trie node: 0 the root, -1 off the trie), wstate (its word-LM state), lm
 * (the fp32 sum over its COMPLETED words) and nw (their count): functions of the token sequence, so a merge touches tot
 * alone.  The blank candidate keeps all four.  A label k != space: node' = node >= 0 ? trie_next[node][k] : -1, the rest
 * unchanged; with lexicon_only node' < 0 is no candidate.  The label `space` from the root changes nothing; elsewhere the
 * pending word w = trie_word[node] (unk when node < 0 or trie_word[node] < 0) closes: (lp, s') the lookup (wstate, w),
 * lm' = lm + lp, nw' = nw + 1, wstate' = s', node' = the root; with lexicon_only a `space` at a node that ends no word is
 * no candidate.  A candidate ranks by (tot + alpha lm) + beta nw, the four operations rounded on their own.  A final closes
 * its pending word the same way (with lexicon_only an entry whose pending node ends no word is no final), with eos_term the
 * lookup of eos from the resulting state joins lm, and the final ranks by those values; the earlier final first on ties.
 * With alpha = beta = 0, eos_term and lexicon_only off, hyp, hyp_len and rnnt_score are the plain search's bits; lm_score of
 * a hypothesis is asr_word_lm_score_f32 of its tokens with the same eos_term.
 *   asr_transducer_wbeam_ws_bytes       the EXTRA workspace in bytes, plain integers, no GPU: 4 * 7 * round64(B K) - node,
 *                                 wstate and nw of two generations of the beam and the finals' nw (round64: up to a
 *                                 multiple of 64).  B <= 0: ASR_E_ARG; K outside 1 .. ASR_BEAM_KMAX: ASR_E_SHAPE
 *   asr_transducer_wbeam_init_f32       asr_transducer_beam_init_f32, and the root, lm->start and 0 words for the empty sequence
 *   asr_transducer_wbeam_step_f32       asr_transducer_beam_step_f32 with the semantics above: one thread per live entry looks up
 *                                 the entry's close pair (and a final's end term), the candidate walk reads them
 *   asr_transducer_wbeam_backtrace_f32  asr_transducer_beam_backtrace_f32 and n_words int32 [B][K] (-1: unused).  An utterance
 *                                 without a frame gives the empty hypothesis at tot 0, lm 0 (the lookup of eos from
 *                                 lm->start with eos_term) and 0 words
 * Each takes the call `a`, the LM, alpha, beta (finite, else ASR_E_ARG), eos_term, lexicon_only and the extra workspace wws
 * (4-byte aligned, at least asr_transducer_wbeam_ws_bytes; else ASR_E_ARG); lm->V != a->V: ASR_E_SHAPE.  An iteration stays
 * four launches, a search 4 (T + L) + 2.  What is read back from the workspace to index the LM's tables is clamped to them;
 * no floating-point atomics, no host synchronisation, no allocation; a slot that is not live is never read.
 * ------------------------------------------------------------------------------------- */
int asr_transducer_wbeam_ws_bytes(int B, int K, int64_t* ws_bytes);
int asr_transducer_wbeam_init_f32(const asr_transducer_beam_t* a, const asr_word_lm_t* lm, float alpha, float beta, int eos_term,
                                  int lexicon_only, void* wws, int64_t wws_bytes, int bos, asr_stream_t stream);
int asr_transducer_wbeam_step_f32(const asr_transducer_beam_t* a, const asr_word_lm_t* lm, float alpha, float beta, int eos_term,
                                  int lexicon_only, void* wws, int64_t wws_bytes, int it, asr_stream_t stream);
int asr_transducer_wbeam_backtrace_f32(const asr_transducer_beam_t* a, const asr_word_lm_t* lm, float alpha, float beta,
                                       int eos_term, int lexicon_only, void* wws, int64_t wws_bytes, int32_t* hyp,
                                       int32_t* hyp_len, float* score, float* rnnt_score, float* lm_score, int32_t* n_words,
                                       asr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * An n-gram LM or a lexicon with a word-level LM inside the attention beam search (csrc/beam.hip, csrc/word_lm.h; DESIGN
 * 4.31).  Not reference operators.  Four entries added to ABI version 8 WITHOUT a version change: additive - asr_beam_t, the
 * select, reorder and backtrack entries above and the kernels they launch are unchanged.
 * The search is the one of asr_beam_select_f32 / _lm_f32 / _ctc_f32 with one more term.  Every beam row carries, beside its
 * running score, the position of its token sequence in the LM - held in the caller's extra workspace, like the parts of the
 * finished entries:
 *     p->scores   base: the score the search carries without this LM (attention, CTC prefix and judge terms)
 *     n-gram      the automaton state (lm_start for the empty sequence), lm - the fp32 sum of lm_logp[state][c] over the tokens
 *                 in order, every addition rounded on its own - and len, the tokens that are not <EOS>
 *     word LM     the trie node of the pending word, the word state, lm over the COMPLETED words and their number nw, moving
 *                 as asr_word_lm_score_f32's walk does (a <space> behind a pending word closes it)
 * A candidate (k, v): base' is the candidate expression of the variant (plain, LM, CTC) operation for operation; lm', len' /
 * nw' are those of the extended sequence, <EOS> taking the end term (n-gram: lm + lm_logp[state][eos]; word LM: the pending
 * word closes, then the lookup of the LM's `eos` word).  It ranks by
 *     (base' + weight lm') + bonus len'      (word LM: bonus nw')       fp32, each of the four operations rounded on its own
 * and with lexicon_only (word LM) a token that leaves the trie, and a <space> or <EOS> whose pending node ends no word, rank
 * -inf.  The first 2K by rank (ties: the lower flat index), the <EOS> rule, the finishing at t = L-1 and the done flags are
 * asr_beam_select_f32's on the rank; live beams that finish as they stand at t = L-1 take the end term, but no <EOS> token (and
 * with lexicon_only are dropped where the pending node ends no word).  fin_score holds the rank of a finished entry.
 * weight = bonus = 0 (lexicon_only off): rank = base', and every output word of the search equals the one without this LM.
 * lm_score of a hypothesis is asr_ngram_score_f32 (eos = p->eos) / asr_word_lm_score_f32 (eos_term 1) of its tokens, bit for
 * bit, n_words the latter's count.
 *   asr_beam_tlm_t           the LM of the call: kind, its tables (n-gram: lm_logp / lm_next [lm_states][V] as
 *                            asr_ctc_beam_lm_f32 takes them; word LM: an asr_word_lm_t with V = p->V), weight, bonus (finite:
 *                            ASR_E_ARG), lexicon_only, and the extra workspace ws (4-byte aligned, at least
 *                            asr_beam_tlm_ws_bytes; else ASR_E_ARG).  lm_states V > INT_MAX, lm_start outside the states, or a
 *                            word LM over another vocabulary: ASR_E_SHAPE.  All checks come before any launch.
 *   asr_beam_tlm_ws_bytes    plain integers, no GPU: 4 (4 round64(B K) + 3 round64(B ASR_BEAM_FCAP)) - independent of L.
 *   asr_beam_tlm_init_f32    the position of the empty sequence in every beam row.  One launch, before step 0.
 *   asr_beam_select_tlm_f32  the select of step t: lm_logits NULL: no judge LM; ctc_weight 0: no CTC term (psi is not read),
 *                            as asr_beam_select_ctc_f32.  One thread per live entry looks up its close pair and end term up
 *                            front (LDS); the candidate loop reads LDS and the entry's table row / trie_next row; the thread
 *                            that walks the ranked candidates writes the new positions in place from the staged copies, so
 *                            asr_beam_reorder_f32 / _lm_f32 and asr_ctc_prefix_advance_f32 are used as they are.  One launch.
 *   asr_beam_backtrack_tlm   asr_beam_backtrack, and in the same order att_score fp32 [B][K] (base), lm_score fp32 [B][K] and
 *                            n int32 [B][K] (len / n_words); -inf, -inf, -1 for a rank without a hypothesis.
 * No floating-point atomics, no host synchronisation, no allocation: the same bits in every run.
 * ------------------------------------------------------------------------------------- */
#define ASR_BEAM_TLM_NGRAM 1
#define ASR_BEAM_TLM_WORD 2
typedef struct {
  int kind;                       /* ASR_BEAM_TLM_NGRAM or ASR_BEAM_TLM_WORD */
  int lm_states, lm_start;        /* n-gram */
  const float* lm_logp;
  const int32_t* lm_next;
  const asr_word_lm_t* word_lm;   /* word LM */
  float weight, bonus;
  int lexicon_only;
  void* ws;
  int64_t ws_bytes;
} asr_beam_tlm_t;
int asr_beam_tlm_ws_bytes(int B, int K, int64_t* ws_bytes);
int asr_beam_tlm_init_f32(const asr_beam_t* p, const asr_beam_tlm_t* lm, asr_stream_t stream);
int asr_beam_select_tlm_f32(const asr_beam_t* p, const asr_beam_tlm_t* lm, const float* lm_logits, float lm_weight,
                            const float* psi, const float* psi_prev, float ctc_weight, int t, asr_stream_t stream);
int asr_beam_backtrack_tlm(const asr_beam_t* p, const asr_beam_tlm_t* lm, float length_penalty, int32_t* tokens, float* scores,
                           int32_t* lengths, float* att_score, float* lm_score, int32_t* n, asr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ASR_HIP_H */
