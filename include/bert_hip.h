/*
 * bert_hip.h — MI355X extensions of the bert.h ABI (libbert.so).
 *
 * Not part of the reference interface: these entry points exist for callers
 * that keep their data in HBM (zero-copy integration, bench.py), for live
 * per-kernel timing, for the native quantizer, and for per-kernel parity
 * tests.  Plain C types only (no torch / HIP types in the signatures); a
 * `stream` argument is a hipStream_t passed as void* (NULL = the context's own
 * stream for that device).
 */
#ifndef BERT_HIP_H
#define BERT_HIP_H

#include "bert.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * bert_load_from_file with an activation mode.  0: f16 activations into the
 * matrix cores, the default path (it tracks the f32-activation arithmetic).  1:
 * the reference's own arithmetic for q4_0 / q4_1 / q8_0 files: every projection
 * re-quantizes its input rows to q8_0 / q8_1 per 32-element block and takes
 * integer block dots (ggml through bert.cpp:995-1016, 1040, 1059, 1066), for
 * embeddings comparable with a CPU deployment of the reference; slower.  f16 and
 * f32 files have no q8 arithmetic in the reference: mode 1 loads them in mode 0.
 * Any other act_mode returns NULL.  The plain bert_load_from_file takes its mode
 * from the environment, BERT_ACT=f16|q8 (unset: f16; anything else: NULL).
 * bertx_activation_mode: the mode the context actually runs.
 */
BERT_API struct bert_ctx *bertx_load_from_file(const char *fname, int32_t act_mode);
BERT_API int32_t bertx_activation_mode(struct bert_ctx *ctx);

/* Number of GPUs the context drives, and the HIP ordinal of slot i. */
BERT_API int32_t bertx_num_devices(struct bert_ctx *ctx);
BERT_API int32_t bertx_device_ordinal(struct bert_ctx *ctx, int32_t slot);

/* hparams {n_vocab, n_max_tokens, n_embd, n_intermediate, n_head, n_layer, ftype}. */
BERT_API void bertx_hparams(struct bert_ctx *ctx, int32_t *out7);

/*
 * Device-resident forward on GPU `slot`.  d_ids: int32[total_tokens] packed
 * sentences back to back; d_cu: int32[n_seqs+1] prefix offsets (d_cu[0] = 0,
 * d_cu[n_seqs] = total_tokens); d_out: float[n_seqs][n_embd].  All three are
 * device pointers on that GPU.  max_len must be >= every sentence length and
 * <= n_max_tokens.  Asynchronous on `stream`; returns 0 or a negative error.
 */
BERT_API int32_t bertx_forward_device(struct bert_ctx *ctx, int32_t slot,
                                      const int32_t *d_ids, const int32_t *d_cu,
                                      int32_t n_seqs, int32_t max_len, int32_t total_tokens,
                                      float *d_out, void *stream);

/*
 * Pooling of the sentence embeddings, a per-context runtime setting that every
 * entry producing them follows (bert_encode, bert_encode_batch, bert_forward,
 * bert_forward_batch, bert_forward_fake_batch, bertx_forward_device) on every
 * replica.  MEAN (the default; bert.cpp:1087-1095): masked mean of the final
 * LayerNorm rows, divided by its L2 norm.  CLS: the final LayerNorm row of the
 * sentence's first token, divided by its L2 norm (how the BGE family is trained and
 * published).  Output sizes never change.  bertx_set_pooling returns 0, or -1 for
 * an unknown mode (nothing changes).  bert_load_from_file and bertx_load_from_file
 * take the initial mode from the environment, BERT_POOL=mean|cls (unset: mean;
 * anything else: NULL).  Tokenizer-only contexts accept and report the mode.
 *
 * bertx_set_cls_pruning (default 1): under CLS pooling the f16-activation chain
 * runs the last layer's attention, O-proj and FFN on the sentences' first rows only
 * (one row per sentence is ever read); 0 runs the full layer (A/B and tests).  The
 * f32 and q8-activation chains always run the full layer.  Returns 0.
 */
enum { BERTX_POOL_MEAN = 0, BERTX_POOL_CLS = 1 };
BERT_API int32_t bertx_set_pooling(struct bert_ctx *ctx, int32_t pool);
BERT_API int32_t bertx_pooling(struct bert_ctx *ctx);
BERT_API int32_t bertx_set_cls_pruning(struct bert_ctx *ctx, int32_t on);

/*
 * Per-token output: the final LayerNorm row of every token, un-normalised f32,
 * whatever the pooling mode.  Host form: out[i] receives float[n_tokens[i]][n_embd];
 * the refusals of bert_forward_batch (an input longer than n_max_tokens, a
 * tokenizer-only context: a message, outputs untouched) with a negative return;
 * the whole call runs on the least-loaded replica.  Device form: as
 * bertx_forward_device with d_out float[total_tokens][n_embd], rows packed as d_ids.
 */
BERT_API int32_t bertx_forward_tokens(struct bert_ctx *ctx, int32_t n, bert_vocab_id **batch_tokens,
                                      int32_t *n_tokens, float **out);
BERT_API int32_t bertx_forward_tokens_device(struct bert_ctx *ctx, int32_t slot, const int32_t *d_ids,
                                             const int32_t *d_cu, int32_t n_seqs, int32_t max_len,
                                             int32_t total_tokens, float *d_out, void *stream);

/* Make sure the workspace of `slot` can hold total_tokens (so a timed region
 * never allocates).  Returns 0 or a negative error. */
BERT_API int32_t bertx_reserve(struct bert_ctx *ctx, int32_t slot, int32_t total_tokens, int32_t n_seqs);

/*
 * Live kernel timing: when enabled, every launch is bracketed by hipEvents on
 * its stream and accumulated per kernel class.  bertx_kernel_stats fills the
 * class name, launch count, summed device milliseconds and summed algorithmic
 * work (FLOP for GEMM/attention classes, bytes for the memory-bound ones) for
 * class `idx` (returns 0, or -1 past the last class).  Stats cover launches
 * whose events have completed (call after a device synchronize).
 */
BERT_API void bertx_set_profiling(struct bert_ctx *ctx, int32_t on);
BERT_API void bertx_reset_stats(struct bert_ctx *ctx);
BERT_API int32_t bertx_kernel_stats(struct bert_ctx *ctx, int32_t idx, const char **name,
                                    int64_t *launches, double *total_ms, double *work,
                                    int32_t *work_is_flops);

/*
 * Multi-GPU balance of the last host-driven call that ran on GPU `slot`
 * (bert_forward_batch / bert_encode_batch, which route or shard sentences over the
 * context's GPUs by FLOP cost, reference entry point bert.cpp:1374-1444): its host
 * wall time for its share (staging, H2D, forward, D2H), its sentence and token
 * counts.  Returns 0, or -1 for a bad slot.
 */
BERT_API int32_t bertx_device_last_call(struct bert_ctx *ctx, int32_t slot, double *wall_ms, int32_t *n_seqs,
                                        int64_t *n_tokens);

/*
 * Number of host-driven calls (bert_forward_batch / bert_encode_batch shares) that
 * have run on replica `slot` since load, or -1 for a bad slot.  Routing rule of
 * those calls (bert_abi.cpp run_forward): a call of T tokens uses
 * k = clamp(min(idle replicas, T / 4096), 1, ...) replicas, the k least-loaded by the
 * work still in flight on them (ties rotate), split by cost; so a large batch
 * spreads over the idle replicas and a call that finds none idle (a concurrent
 * caller) goes whole to the least-loaded replica.
 */
BERT_API int64_t bertx_device_calls(struct bert_ctx *ctx, int32_t slot);

/* Native quantizer (mirrors models/quantize.cpp): f32/f16 file -> itype
 * 2 (q4_0), 3 (q4_1) or 8 (q8_0, extension).  Returns 0 on success. */
BERT_API int32_t bertx_quantize_file(const char *fname_in, const char *fname_out, int32_t itype);

/* Native converter (mirrors models/convert-to-ggml.py:1-113): a local HF
 * BERT directory (config.json, vocab.txt, model.safetensors or a sharded
 * model.safetensors.index.json) -> model file, ftype 0 (f32) or 1 (f16:
 * 2-D weights only).  Same bytes as the reference script writes.  Returns 0
 * on success. */
BERT_API int32_t bertx_convert_hf(const char *dir_model, const char *fname_out, int32_t ftype);

/*
 * Per-kernel parity hooks (host buffers in/out, run synchronously on device 0).
 * w_rows: the weight exactly as the model file stores it (N rows of K elements
 * in format `fmt` = 0,1,2,3,8).  x: f16 bits [M][K].  epi: 0 = +bias -> f16,
 * 1 = +bias, era GELU -> f16, 2 = +bias +res -> f16 (res f16 [M][N], the
 * residual-stream form; sum in f32, computed in place over res).  cfg: GEMM tile
 * config (0 = the production heuristic, 2 = 4 waves 256x128, 11 = the same with
 * the X pieces in one burst, 3 = 4 waves 128x128, 4 = 2 waves 64x64, 16 = 4 waves
 * 64x64 with wave-private X rings); a tile that does not divide the padded M falls
 * back to the next smaller one — bertx_test_gemm_ran() reports what ran.
 * Reference interface these kernels replace: ggml_mul_mat + ggml_add (+ ggml_gelu)
 * at bert.cpp:994-1016, 1040-1045, 1059-1072.
 */
BERT_API int32_t bertx_test_gemm(int32_t fmt, int32_t N, int32_t K, const void *w_rows,
                                 const float *bias, int32_t M, const uint16_t *x,
                                 int32_t epi, const void *res, void *out, int32_t cfg);

/*
 * The same GEMM with the LayerNorm bookkeeping of the forward (the "LN fold",
 * DESIGN.md §2; LayerNorm = bert.cpp:977-984, 1048-1056, 1074-1082):
 *  - in_stats (epi 0/1): x holds z = y * in_g of rows y with in_stats[M] =
 *    (mean, 1/sigma) float pairs; the result is LN(y) W^T + bias with LN's gamma
 *    in_g, beta in_b [K] (else NULL: plain x W^T + bias);
 *  - epi 2: res holds z = y * res_g with res_stats [M] (the residual is LN(y) with
 *    gamma res_g, beta res_b [N]), or the plain residual when res_stats is NULL;
 *    with g_next [N] the output is f16(y' * g_next) of the new stream y' =
 *    residual + x W^T + bias and st_out [M] receives y''s (mean, 1/sigma) as the
 *    forward computes them (epilogue partials + the statistics kernel).
 */
BERT_API int32_t bertx_test_gemm_ln(int32_t fmt, int32_t N, int32_t K, const void *w_rows, const float *bias,
                                    int32_t M, const uint16_t *x, const float *in_stats, const float *in_g,
                                    const float *in_b, int32_t epi, const uint16_t *res, const float *res_stats,
                                    const float *res_g, const float *res_b, const float *g_next, uint16_t *out,
                                    float *st_out, int32_t cfg);

/*
 * The statistics-fold form of the input-LN GEMM (epi 0/1; small batches, where the
 * forward drops the ln_stats launches): part holds the residual GEMM's partials of
 * the input rows, float pairs [K/32][M] (sum, squared deviations from the group
 * mean); the GEMM combines them per row with the statistics kernel's arithmetic
 * and then runs as bertx_test_gemm_ln with those in_stats; st_out [M] (mean,
 * 1/sigma) receives the combined statistics (the column-0 tiles' store), st_kernel
 * [M] (if not NULL) the statistics kernel's combine of the same partials.  Returns
 * -2 when the tile config has no fold form for this shape.
 */
BERT_API int32_t bertx_test_gemm_fold(int32_t fmt, int32_t N, int32_t K, const void *w_rows, const float *bias,
                                      int32_t M, const uint16_t *x, const float *part, const float *in_g,
                                      const float *in_b, int32_t epi, uint16_t *out, float *st_out, float *st_kernel,
                                      int32_t cfg);

/*
 * The two hooks above with the launched row count given: `rows` (a multiple of 64,
 * rows >= M) is the M that launch_gemm gets, so the 64-, 128-, 192- and 320-row
 * launches of the small-batch forward and the tile fallbacks can be reached
 * (bertx_test_gemm_ln and bertx_test_gemm_fold are these with rows = M rounded up
 * to 256, returning the first M rows).  Rows M .. rows-1 of x, res, the statistics
 * and the partials are filled by the hook with finite non-zero values and are
 * computed and stored like any other row.  out [rows][N], st_out [rows] (and
 * st_kernel [rows]) come back whole; every buffer the kernels write starts as 0xFF
 * bytes (NaN bits; the in-place residual as the residual), so an element left
 * unwritten shows, and carries 64 guard rows behind row `rows`.
 * bertx_test_gemm_rows: part_out (or NULL), float pairs [N/32][rows]: the per-group
 * (sum, squared deviations from the group mean) the g_next form's epilogue wrote;
 * out_of_place != 0 gives the epi-2 forms an output buffer of their own (res is
 * read, out is written), 0 runs them in place as the forward does.
 * Return 0; -1 bad arguments or a runtime error; -2 (fold) no fold form for the
 * shape; -5 a guard row behind row `rows` of a written buffer was stored to.
 */
BERT_API int32_t bertx_test_gemm_rows(int32_t fmt, int32_t N, int32_t K, const void *w_rows, const float *bias,
                                      int32_t M, int32_t rows, const uint16_t *x, const float *in_stats,
                                      const float *in_g, const float *in_b, int32_t epi, const uint16_t *res,
                                      const float *res_stats, const float *res_g, const float *res_b,
                                      const float *g_next, int32_t out_of_place, uint16_t *out, float *st_out,
                                      float *part_out, int32_t cfg);
BERT_API int32_t bertx_test_gemm_fold_rows(int32_t fmt, int32_t N, int32_t K, const void *w_rows,
                                           const float *bias, int32_t M, int32_t rows, const uint16_t *x,
                                           const float *part, const float *in_g, const float *in_b, int32_t epi,
                                           uint16_t *out, float *st_out, float *st_kernel, int32_t cfg);

/* Compute units of device 0 as the GEMM launch code counts them (tile heuristic,
 * persistent grids); -1 without a device. */
BERT_API int32_t bertx_test_cu_count(void);

/* The tile config the calling thread's last GEMM launch dispatched (after the
 * fallbacks above), so a test can assert which kernel it exercised. */
BERT_API int32_t bertx_test_gemm_ran(void);

/*
 * The f32 chain's GEMM (ftype 0 files: f32 activations x f32 weights on
 * v_mfma_f32_16x16x4_f32, reference ggml_mul_mat f32 x f32, bert.cpp:995):
 * w f32 [N][K] (file rows), x f32 [M][K], out f32 [M][N] = epi(x w^T):
 * epi 0 = bias + acc, 1 = era GELU(bias + acc) (fp16-table semantics), 2 =
 * (bias + acc) + res (res f32 [M][N]).  K % 32 == 0.  Returns 0 or -1.
 */
BERT_API int32_t bertx_test_gemm_f32(int32_t N, int32_t K, const float *w, const float *bias, int32_t M,
                                     const float *x, int32_t epi, const float *res, float *out);

/*
 * The q8-activation mode's two kernels (activation mode 1 above).
 * bertx_test_quantize_act: ggml's activation quantizer on x f32 [M][K] (K % 32 ==
 * 0): q int8 [M][K], d f32 [M][K/32] and, kind 1, s f32 [M][K/32].  kind 0 = q8_0
 * (d = the f16-rounded scale as f32, the value the dot uses; s may be NULL), kind 1
 * = q8_1 (d = the f32 scale, s = (float)(sum q) * d).
 * bertx_test_gemm_q8: one projection as the forward runs it, the quantizer (q8_1
 * for fmt 3, else q8_0) and then the block-integer GEMM: fmt 2, 3 or 8, w_rows as
 * bertx_test_gemm, x f32 [M][K] (K % 64 == 0), out f32 [M][N] (N % 32 == 0) =
 * epi(sum over blocks, ascending, of (wd xd) (float)sumi [+ wm xs]), epi as
 * bertx_test_gemm_f32 (res f32 [M][N]).  Return 0 or -1.
 */
BERT_API int32_t bertx_test_quantize_act(int32_t kind, int32_t M, int32_t K, const float *x, int8_t *q, float *d,
                                         float *s);
BERT_API int32_t bertx_test_gemm_q8(int32_t fmt, int32_t N, int32_t K, const void *w_rows, const float *bias,
                                    int32_t M, const float *x, int32_t epi, const float *res, float *out);

/*
 * GEMM micro-benchmark on random operands (device 0): average device time of
 * `iters` launches of the GEMM for fmt / N / K / M / epi / cfg (as
 * bertx_test_gemm), in the forward's own forms: the LN fold on the input of
 * epi 0/1, the residual LN + next gamma + partial statistics for epi 2
 * (cfg | 0x100: the plain forms, for A/B).
 */
BERT_API int32_t bertx_bench_gemm(int32_t fmt, int32_t N, int32_t K, int32_t M, int32_t epi, int32_t cfg,
                                  int32_t iters, float *avg_us);

/*
 * Attention micro-benchmark on random operands (device 0): average device time
 * of `iters` launches for n_seqs sentences of `len` tokens, n_head heads of size
 * dh; variant 0 = the production kernels (attention_pp for 64 < L <= 512 at dh
 * 64, attention_short for L <= 64), 8 = attention_lds3 (the persistent 16-wave
 * kernel, bitwise the same), 7 = lds3 on at most 7 workgroups (many ragged items
 * per workgroup).
 */
BERT_API int32_t bertx_bench_attention(int32_t n_seqs, int32_t len, int32_t n_head, int32_t dh, int32_t variant,
                                       int32_t iters, float *avg_us);

/*
 * Attention parity hook (host buffers, device 0): qkv f16 bits [T][3d] as the
 * QKV GEMM writes it (packed tokens of n_seqs sentences, cu[n_seqs + 1] the
 * token offsets), out f16 [T][d] = per (sentence, head) softmax(Q K^T / sqrt(dh)) V
 * over the sentence's own keys (bert.cpp:1018-1036).  variant as
 * bertx_bench_attention; -1 = the streaming kernel (sentences > 512), which a batch
 * holding such a sentence takes by itself.  The device output starts as NaN bits
 * (0xffff) with ATT_QT spare rows behind it, so a row the kernel left unwritten comes
 * back as NaN.  Returns 0; -1 bad arguments; -3 the runtime refused the launch; -4
 * the synchronise after it reported an error; -5 a spare row behind row T was
 * written.
 */
BERT_API int32_t bertx_test_attention(const uint16_t *qkv, const int32_t *cu, int32_t n_seqs, int32_t n_head,
                                      int32_t d, int32_t variant, uint16_t *out);

/* The kernel the calling thread's last attention launch ran: 0 attention_short,
 * 1 attention_pp, 2 attention_lds3, 3 attention_lds<32>, 4 the streaming kernel
 * (-1: none yet).  BERT_ATT_PP=0 / BERT_ATT_SHORT=0 in the environment take variant
 * 0 off the first two. */
BERT_API int32_t bertx_test_attention_ran(void);

/*
 * Parity hook of the pruned last layer's attention (CLS pooling; host buffers,
 * device 0): qkv and cu as bertx_test_attention, out f16 [n_seqs][d], row b = the
 * attention output of the sentence's first token (row cu[b]) over the sentence's
 * own keys.  dh 32 or 64, any sentence length.  -5: the kernel left a padding row
 * of its compact output unwritten.
 */
BERT_API int32_t bertx_test_attention_cls(const uint16_t *qkv, const int32_t *cu, int32_t n_seqs, int32_t n_head,
                                          int32_t d, uint16_t *out);

/*
 * The same launch with its residual gather, on Mc >= n_seqs compact rows: out f16
 * [Mc][d] comes back whole.  With z f16 [T][d] and st f32 [T][2] (all four of z, st,
 * zc, stc, or none): zc f16 [Mc][d] and stc f32 [Mc][2] come back whole too, zc[b] =
 * z[cu[b]], stc[b] = st[cu[b]].  All three device buffers start as NaN bits (0xff
 * bytes), so the zeros of rows n_seqs <= row < Mc are the kernel's.  Returns as
 * bertx_test_attention (no -5: the caller sees every row).
 */
BERT_API int32_t bertx_test_attention_cls_gather(const uint16_t *qkv, const int32_t *cu, int32_t n_seqs,
                                                 int32_t n_head, int32_t d, int32_t Mc, uint16_t *out,
                                                 const uint16_t *z, const float *st, uint16_t *zc, float *stc);

/*
 * Parity hooks of the memory-bound row kernels (norm.hip, f32.hip and their table
 * readers; host buffers, device 0, one launch each).  Common rules: every output
 * buffer has out_rows rows (at least the rows the kernel writes), is uploaded
 * before the launch and copied back whole after it, so rows the caller pre-filled
 * with a sentinel show whether the kernel touched them.  Returns 0; -1 for bad
 * arguments or the launcher's own refusal (outputs still copied back); -3 when the
 * runtime refused the launch; -4 when the synchronise after it reported an error.
 * cu: int32 [n_seqs + 1] token offsets, cu[0] = 0, every sentence of 1 .. max_len
 * tokens; widths d % 64 == 0, 64 <= d <= 1024.
 *
 * bertx_test_embed_ln: the three embedding tables as file-format rows (word
 * [rows_word][d] in fmt_word, type [2][d], pos [rows_pos][d]; formats may differ),
 * repacked as at load.  mode 0: the f16 chain's kernel, out f16 [out_rows][d] = z =
 * f16((pos[i] + (type[0] + word[id])) * ln_w) and stats f32 [out_rows][2] = (mean,
 * 1/sigma) of the f32 sum.  mode 1 / 2: the f32 chain's kernel (2: its exact form),
 * out f32 [out_rows][d] = LayerNorm of the sum; stats unused.
 *
 * bertx_test_ln_stats: part f32 pairs [G][stride] -> stats f32 [stats_rows][2] for
 * rows < rows; the launcher's return value (-1: refused, nothing launched).
 *
 * bertx_test_pool: z f16 [T][d] with stats f32 [T][2] (the LN fold's stream).  kind
 * 0: mean pool + L2 (max_len picks the one- or two-launch form), out [out_rows][d],
 * rows < n_seqs; 1: [CLS] pool of rows cu[b]; 2: [CLS] pool of the compact rows b
 * (cu unused); 3: per-token LN output, rows < T.
 *
 * bertx_test_f32_rows: the f32 chain.  kind 0: LayerNorm of x [n][d] (flag: exact),
 * out [out_rows][d] rows < n; 1: mean pool of x [cu[n]][d] over n sentences (flag:
 * the era summation order); 2: [CLS] pool.  g, b: gamma, beta (kind 0).
 *
 * bertx_test_attention_f32: qkv f32 [T][3d] -> out f32 [out_rows][d], rows < T; era:
 * the era summation order.  Returns launch_f32_attention's value (-1: refused).
 */
BERT_API int32_t bertx_test_embed_ln(int32_t mode, int32_t fmt_word, int32_t fmt_type, int32_t fmt_pos,
                                     int32_t rows_word, int32_t rows_pos, int32_t d, const void *word_rows,
                                     const void *type_rows, const void *pos_rows, const float *ln_w,
                                     const float *ln_b, const int32_t *ids, const int32_t *cu, int32_t n_seqs,
                                     int32_t max_len, void *out, float *stats, int32_t out_rows);
BERT_API int32_t bertx_test_ln_stats(const float *part, int32_t G, int32_t stride, int32_t rows, int32_t d,
                                     float *stats, int32_t stats_rows);
BERT_API int32_t bertx_test_pool(int32_t kind, const uint16_t *z, const float *stats, const float *ln_w,
                                 const float *ln_b, const int32_t *cu, int32_t n_seqs, int32_t max_len, int32_t T,
                                 int32_t d, float *out, int32_t out_rows);
BERT_API int32_t bertx_test_f32_rows(int32_t kind, const float *x, const int32_t *cu, int32_t n, int32_t d,
                                     const float *g, const float *b, int32_t flag, float *out, int32_t out_rows);
BERT_API int32_t bertx_test_attention_f32(const float *qkv, const int32_t *cu, int32_t n_seqs, int32_t max_len,
                                          int32_t n_head, int32_t d, int32_t era, float *out, int32_t out_rows);

/*
 * The tokenization stage of bert_encode_batch on its own (bert.cpp:1402-1406 runs
 * it sequentially; here on n_threads threads of the library's persistent pool):
 * texts[i] -> ids[i * n_max .. + min(n_tokens[i], n_max)), n_tokens[i] =
 * bert_tokenize's count (which can exceed n_max, bert.cpp:386-387).  The same
 * function bert_encode_batch calls; for timing and bulk tokenization.  Returns 0
 * or -1.
 */
BERT_API int32_t bertx_tokenize_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts,
                                      int32_t n_max, int32_t *ids, int32_t *n_tokens);

/*
 * Embedding index: an append-only matrix of rows x n_embd embeddings resident in the
 * HBM of one of the context's GPUs, stored as f16, with a fused top-k search (what
 * the reference's sample clients do on the host after bert_encode_batch,
 * examples/sample_dylib.py:84-94).  Row ids are int32 insertion order from 0.
 *
 * bertx_index_create: an index of fixed capacity on GPU `slot`, or NULL after a
 * message (bad slot, capacity < 1, allocation failure, a tokenizer-only context).
 * Its width is the context's n_embd.  The index keeps only the device ordinal and
 * the width: it may outlive the context.  Its buffers never move.
 * bertx_index_clear sets the row count back to 0.
 *
 * bertx_index_add / _add_device: rows float[n][d] (host / device, the layout
 * bertx_forward_device writes) are rounded to f16, nearest even, and appended; the
 * id of the first new row is returned, or a negative error with nothing changed (-2:
 * size + n > capacity).  bertx_index_rows: the stored values of rows first ..
 * first + n - 1, the exact f16 values widened to f32, into out float[n][d].
 *
 * bertx_index_search / _search_device: for each of the B queries float[B][d], the k
 * highest scores into scores float[B][k] with their row ids into ids int32[B][k].
 * A score is the dot product of the f16-rounded query with the stored f16 row,
 * accumulated in f32 (for the library's unit-length embeddings: the cosine, within
 * 2^-10).  Scores descend; equal scores come by ascending id; with fewer than k
 * rows the remaining slots are (-inf, -1).  1 <= k <= 128, B >= 1; anything else
 * returns a negative error and leaves the outputs untouched.  The score of a
 * (query, row) pair does not depend on the row's id, the row count or the other
 * queries of the call, bit for bit.
 *
 * The device forms take device pointers on the index's GPU and a hipStream_t (NULL:
 * the index's own stream); they are asynchronous, allocate nothing and never
 * synchronise, so they can be captured into a HIP graph.  A search sees the rows
 * added by the calls made before it.  Calls on one stream are ordered by the stream;
 * on different streams each operation waits on the device for the previous one's
 * completion event (a stream being captured waits for and records nothing outside
 * its graph).  Host calls on one index are serialised; the caller's current HIP
 * device is left as it was.
 *
 * The text forms encode with bert_encode_batch (the context's pooling mode) and
 * then add or search; if the encoder refuses an input (longer than n_max_tokens)
 * the whole call fails (-4) with nothing added.  The context's n_embd must be the
 * index's width.
 *
 * Storage kinds.  bertx_index_create_ex takes the kind: BERTX_INDEX_F16 (0) is exactly
 * bertx_index_create, everything above; BERTX_INDEX_I8 (1) stores a row as d int8 values
 * and one f32 scale, half the bytes; any other value returns NULL after a message.
 * bertx_index_storage returns the kind, -1 for NULL.  Every other entry follows the
 * index's kind with the same signature, refusals, ordering rules and capturability.
 * The int8 arithmetic, each named operation rounded once to f32 (IEEE, nearest even),
 * one quantizer for stored rows and for queries:
 *   amax = max_i |x_i|;  amax == 0: scale = 0 and every q_i = 0;  otherwise
 *   inv = 127 / amax,  q_i = clamp(rint(x_i * inv), -127, 127) (rint: nearest even),
 *   scale = amax / 127;
 *   score(query, row) = (float)isum * (scale_query * scale_row),  isum = sum_i qq_i qr_i
 * in int32, which is exact (|isum| <= 127 * 127 * 1024 < 2^24) and does not depend on
 * the order of the sum.  So the score of a (query, row) pair depends on that query and
 * that row only, bit for bit, with no accumulation-order caveat; ordering and fill are
 * as above.  Non-finite inputs give unspecified values within the clamp.  Against the
 * f32 dot of the unquantized vectors x (scale s_x) and y (scale s_y):
 *   |x.y - score| <= (s_y |x|_1 + s_x |y|_1) / 2 + d s_x s_y / 4
 * plus the two roundings of the final multiplies.  bertx_index_rows on an int8 index
 * returns the dequantized values (float)q * scale (one f32 multiply);
 * bertx_index_rows_i8 returns the stored bytes q int8[n][d] and scales float[n] of rows
 * first .. first + n - 1, or -1 on an f16 index or a bad range with the outputs
 * untouched.
 *
 * Binary storage.  BERTX_INDEX_BIN (8; the embedding index only, bertx_mvindex_create_ex
 * refuses it) stores a row as its d sign bits, d / 8 bytes: one sixteenth of f16.  One
 * rule for stored rows and for queries:
 *   bit_i = 1 iff x_i > 0: +0, -0, negative values and NaN give 0; a positive subnormal
 *   and +inf give 1 (sentence-transformers' `embeddings > 0`);
 *   score(query, row) = d - 2 * popcount(bits_query xor bits_row), returned as f32.
 * The score is an exact integer with |score| <= 1024, the dot product of the two +-1
 * vectors, and depends on that query's and that row's bits only: not on the row's id, the
 * row count or the other queries.  Ordering, fill and limits are those of the other kinds:
 * scores descend, equal scores (the normal case here: at most d + 1 distinct values) come
 * by ascending id, (-inf, -1) fill, 1 <= k <= 128, B >= 1, widths as above.  What the
 * score is not: it is no cosine and carries no error bound against one.  For random sign
 * patterns E[score / d] = 1 - 2 theta / pi, theta the angle of the two vectors; how well it
 * ranks a model's embeddings is a property of the model.  Every bertx_index_* entry
 * follows the kind with the same signature, refusals, ordering rules and capturability.
 * bertx_index_rows returns +1.0 / -1.0, bertx_index_rows_i8 returns -1 as on f16, and
 * bertx_index_rows_bits returns the stored bits uint8[n][d / 8] of rows first ..
 * first + n - 1 in np.packbits order (element i is bit 7 - i % 8 of byte i / 8), or -1 on
 * another kind or a bad range with the output untouched.
 *
 * Listed rows.  bertx_index_score_ids / _score_ids_device (every kind): queries
 * float[B][d], ids int32[B][n], 1 <= n <= 128 -> scores float[B][n], scores[b][j] = the
 * score of (query b, row ids[b][j]) with exactly the bits bertx_index_search gives that
 * pair, -inf for an id outside [0, size); so the id output of a search, -1 fill included,
 * can be passed as it is.  Refusals return a negative error with the output untouched.
 * The device form follows bertx_index_search_device word for word.
 *
 * Two-stage search.  bertx_index_search_rescored / _device (coarse, fine, queries, B, k,
 * n_cand, scores, ids), k <= n_cand <= 128, stated through the entries above:
 *   cand = the ids of bertx_index_search(coarse, queries, n_cand);
 *   s    = bertx_index_score_ids(fine, queries, cand);
 *   a pair whose id is -1 or one fine does not hold (s = -inf for that reason) is the fill
 *   (-inf, -1); the result is the k best (s, id) pairs in the order of the results, the
 *   fill last.
 * The result is that composition bit for bit; with n_cand >= size(coarse) it is
 * bertx_index_search(fine, k) restricted to the rows coarse holds.  coarse and fine are
 * different indexes of one width on one GPU, else -1 after a message; coarse may be of
 * any kind (binary is the point), and so may fine.  Row ids correspond by insertion
 * order: keeping the two in step is the caller's job.  The call is ordered behind the
 * earlier operations on both indexes; the candidates lie in a buffer coarse got when it
 * was created, so the device form allocates nothing, never synchronises and can be
 * captured; two concurrent calls on the same coarse index are serialised.
 * bertx_index_search_rescored_texts encodes as bertx_index_search_texts does.
 *
 * Deleting rows and filtered search.  Two masks over row ids, both packed 32 rows to a
 * uint32_t word: row r is bit r % 32 of word r / 32 (np.packbits(x, bitorder="little") viewed
 * as uint32).  Tombstones belong to the index, lie on its device, cover the capacity and start
 * as zeros; bit 1 = deleted.  Filters are the caller's, per call; bit 1 = the row may be
 * returned.  A row is admissible for query b iff id < size, its tombstone is 0 and, when a
 * filter is given, its bit in query b's filter is 1.
 * bertx_index_remove / _remove_device (ids int32[n], host / device; n >= 1, anything else a
 * negative error with nothing changed): sets the tombstones of the listed ids and returns 0.
 * Ids outside [0, size), size being the row count when the call is made, are ignored;
 * repeated ids are harmless; the bits are set by atomic OR, so no order matters.  The device
 * form is asynchronous, allocates nothing, never synchronises, can be captured, and is
 * ordered as bertx_index_add_device is.  Ids are never reused: bertx_index_size does not
 * change, and bertx_index_rows / _rows_i8 / _rows_bits still return a deleted row's stored
 * values.  bertx_index_clear also zeroes the tombstones (ordered on the index's stream), so a
 * clear followed by adds starts clean.
 * bertx_index_live: size minus the deleted rows in [0, size); a host call that synchronises.
 * bertx_index_deleted: out uint8[n] = 0 or 1 for rows first .. first + n - 1; -1 on a bad
 * range with the output untouched.
 * bertx_index_search_filtered / _device: bertx_index_search over the admissible rows.
 * filters uint32[n_filters][words] (host / device); n_filters is 1 (one filter for every
 * query) or B (query b uses filter b); words >= ceil(size / 32) is also the stride between
 * filters; bits of rows >= size are ignored, whatever they hold.  filters == NULL with
 * n_filters == 0 is exactly bertx_index_search.  The result is the k best admissible rows
 * with the scorer's bits, the same order (score descending, id ascending) and the same
 * (-inf, -1) fill when fewer than k rows are admissible.  1 <= k <= 128, B >= 1; every
 * refusal (a null pointer, n_filters not 0, 1 or B, too few words, a filter pointer without
 * a count or the reverse) returns a negative error with the outputs untouched.  The device
 * form allocates nothing; the host form allocates and frees a staging buffer for the filters
 * per call.  The filter is read when the kernel runs: a captured search sees the bits the
 * buffer holds at replay.
 * On an index with deletions the entries above follow: bertx_index_search / _search_device
 * return admissible rows only; bertx_index_score_ids gives -inf for a deleted id (and the
 * rescored search's kept-id -1), exactly as for an id outside [0, size); the text forms call
 * these.  The composition that defines the two-stage search stays literally true: coarse's
 * tombstones (and the filter) limit the candidates, a candidate fine has deleted becomes the
 * fill.  bertx_index_search_rescored_filtered / _device is that composition with
 * bertx_index_search_filtered(coarse, queries, n_cand, filters) as its first line.
 * An index from which nothing was removed since creation or the last clear, searched without
 * a filter, launches the kernels it launched before masks existed, with the same arguments:
 * the masked kernels are other instantiations, chosen at launch time by a host flag that any
 * accepted remove sets and clear resets (the rule the row count follows in captured graphs:
 * a graph captured before the first removal keeps launching the unmasked kernels).
 *
 * Not provided: an index sharded over several GPUs, compaction (reclaiming deleted rows'
 * bytes or renumbering), skipping the loads of fully masked groups, a gather path for very
 * selective filters, saving and loading (the mask layout above is what a file would carry;
 * the token store's masks: "Deleting documents and filtered search" below), f32 storage, f16 queries against int8 rows, 4-bit storage,
 * binary rows against unbinarized queries (asymmetric scores), a fine copy kept in host
 * memory.
 */
enum { BERTX_INDEX_F16 = 0, BERTX_INDEX_I8 = 1 };
enum { BERTX_INDEX_BIN = 8 };   /* the embedding index only: "Binary storage" above */
struct bertx_index;
BERT_API struct bertx_index *bertx_index_create(struct bert_ctx *ctx, int32_t slot, int32_t capacity_rows);
BERT_API struct bertx_index *bertx_index_create_ex(struct bert_ctx *ctx, int32_t slot, int32_t capacity_rows,
                                                   int32_t storage);
BERT_API int32_t bertx_index_storage(struct bertx_index *idx);
BERT_API void bertx_index_free(struct bertx_index *idx);
BERT_API int32_t bertx_index_clear(struct bertx_index *idx);
BERT_API int32_t bertx_index_size(struct bertx_index *idx);
BERT_API int32_t bertx_index_capacity(struct bertx_index *idx);
BERT_API int32_t bertx_index_dim(struct bertx_index *idx);
BERT_API int32_t bertx_index_add(struct bertx_index *idx, const float *rows, int32_t n);
BERT_API int32_t bertx_index_add_device(struct bertx_index *idx, const float *d_rows, int32_t n, void *stream);
BERT_API int32_t bertx_index_rows(struct bertx_index *idx, int32_t first, int32_t n, float *out);
BERT_API int32_t bertx_index_rows_i8(struct bertx_index *idx, int32_t first, int32_t n, int8_t *q, float *scale);
BERT_API int32_t bertx_index_search(struct bertx_index *idx, const float *queries, int32_t B, int32_t k,
                                    float *scores, int32_t *ids);
BERT_API int32_t bertx_index_search_device(struct bertx_index *idx, const float *d_queries, int32_t B, int32_t k,
                                           float *d_scores, int32_t *d_ids, void *stream);
BERT_API int32_t bertx_index_add_texts(struct bertx_index *idx, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                       const char **texts);
BERT_API int32_t bertx_index_search_texts(struct bertx_index *idx, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                          const char **texts, int32_t k, float *scores, int32_t *ids);
BERT_API int32_t bertx_index_rows_bits(struct bertx_index *idx, int32_t first, int32_t n, uint8_t *out);
BERT_API int32_t bertx_index_score_ids(struct bertx_index *idx, const float *queries, int32_t B, const int32_t *ids,
                                       int32_t n, float *scores);
BERT_API int32_t bertx_index_score_ids_device(struct bertx_index *idx, const float *d_queries, int32_t B,
                                              const int32_t *d_ids, int32_t n, float *d_scores, void *stream);
BERT_API int32_t bertx_index_search_rescored(struct bertx_index *coarse, struct bertx_index *fine, const float *queries,
                                             int32_t B, int32_t k, int32_t n_cand, float *scores, int32_t *ids);
BERT_API int32_t bertx_index_search_rescored_device(struct bertx_index *coarse, struct bertx_index *fine,
                                                    const float *d_queries, int32_t B, int32_t k, int32_t n_cand,
                                                    float *d_scores, int32_t *d_ids, void *stream);
BERT_API int32_t bertx_index_search_rescored_texts(struct bertx_index *coarse, struct bertx_index *fine,
                                                   struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts,
                                                   int32_t k, int32_t n_cand, float *scores, int32_t *ids);
BERT_API int32_t bertx_index_remove(struct bertx_index *idx, const int32_t *ids, int32_t n);
BERT_API int32_t bertx_index_remove_device(struct bertx_index *idx, const int32_t *d_ids, int32_t n, void *stream);
BERT_API int32_t bertx_index_live(struct bertx_index *idx);
BERT_API int32_t bertx_index_deleted(struct bertx_index *idx, int32_t first, int32_t n, uint8_t *out);
BERT_API int32_t bertx_index_search_filtered(struct bertx_index *idx, const float *queries, int32_t B, int32_t k,
                                             const uint32_t *filters, int32_t n_filters, int32_t words, float *scores,
                                             int32_t *ids);
BERT_API int32_t bertx_index_search_filtered_device(struct bertx_index *idx, const float *d_queries, int32_t B, int32_t k,
                                                    const uint32_t *d_filters, int32_t n_filters, int32_t words,
                                                    float *d_scores, int32_t *d_ids, void *stream);
BERT_API int32_t bertx_index_search_rescored_filtered(struct bertx_index *coarse, struct bertx_index *fine,
                                                      const float *queries, int32_t B, int32_t k, int32_t n_cand,
                                                      const uint32_t *filters, int32_t n_filters, int32_t words,
                                                      float *scores, int32_t *ids);
BERT_API int32_t bertx_index_search_rescored_filtered_device(struct bertx_index *coarse, struct bertx_index *fine,
                                                             const float *d_queries, int32_t B, int32_t k, int32_t n_cand,
                                                             const uint32_t *d_filters, int32_t n_filters, int32_t words,
                                                             float *d_scores, int32_t *d_ids, void *stream);

/*
 * Token store: late interaction (ColBERT's MaxSim) over per-token vectors.  An
 * append-only set of documents resident in the HBM of one of the context's GPUs; a
 * document is len >= 1 token vectors of the store's width, each stored as a unit-length
 * f16 row; a query of Lq <= 64 token vectors scores a list of documents in one launch.
 * Document ids are int32 insertion order from 0.  The conventions are the embedding
 * index's: plain C types, a message and a negative return on refusal with the outputs
 * untouched, the caller's HIP device left as it was, host calls on one store
 * serialised, and the stream ordering rules of the index (above) word for word.
 *
 * bertx_mvindex_create: a store of `width` (a multiple of 64 in 64 .. 1024; it need not
 * be n_embd, so a caller can store vectors it projected itself) on GPU `slot`, for at
 * most capacity_docs documents in at most capacity_token_slots token slots, or NULL
 * after a message (bad slot, width or capacity, allocation failure, a tokenizer-only
 * context).  A document of len tokens takes 16 ceil(len / 16) slots: every document
 * starts on a 16-row group of the search kernel's f16 fragment order.  The store keeps
 * only the device ordinal and the width: it may outlive the context.  Its buffers never
 * move.  _clear sets both counts back to 0; _docs and _token_slots return what is used.
 *
 * The arithmetic, one normaliser for stored rows and for queries, every named operation
 * rounded once to f32 (IEEE, nearest even):
 *   ss = sum_i x_i * x_i, summed in an order that depends on the width only;
 *   ss == 0: the row is stored as zeros;  otherwise rinv = 1 / sqrt(ss) (sqrt, then the
 *   division) and v_i = f16(x_i * rinv), nearest even;
 *   sim(q, c) = the f16 search score of the embedding index: both operands f16, products
 *   accumulated in f32 from 0 in ascending blocks of 32 elements;
 *   score(doc) = sum_{i < Lq} max_{j < len} sim(q_i, c_j): the max is exact, the sum over
 *   i is f32 in an order that depends on Lq only.
 * The slots of a document's last group past len are never counted, whatever they hold
 * (a similarity can be negative, so they count as -inf, not 0).  A document's score
 * depends on the query and on that document's rows only, bit for bit: not on its id,
 * the other documents, the candidate list, its length or its order.  Against the exact
 * value v = x_i / |x| a stored element is within |v| (2^-11 + (w + 8) 2^-24) + 2^-24;
 * against the exact MaxSim of the stored f16 values a score is within
 * Lq (2 w + Lq) 2^-24.
 *
 * bertx_mvindex_add / _add_device: n documents, their token rows float[T][width]
 * consecutive (host / device), T = sum lens, with lens int32[n] always on the host;
 * returns the id of the first new document, or a negative error with nothing changed
 * (-2: over either capacity; -1: a len < 1 or bad arguments).  One call of several
 * documents stores the bits that one call per document stores.  _doc_len: a document's
 * len (-1: no such id).  _doc: its stored f16 values widened, into out float[len][width].
 *
 * bertx_mvindex_score / _score_device: out[c] = score(document ids[c]) for c < n; ids
 * NULL: document c (pass n = _docs for all).  An id outside [0, docs) scores -inf and
 * disturbs nothing else, so the id output of bertx_index_search with its -1 fill slots
 * can be passed unchanged.  Only out[0 .. n) is written.  The host form refuses (-1) Lq
 * outside 1 .. 64 and n < 1.  The device form takes device pointers on the store's GPU
 * and a hipStream_t (NULL: the store's own stream); it is asynchronous, allocates
 * nothing and never synchronises, so it can be captured into a HIP graph (a captured
 * score keeps the document count of its capture).  The add forms are asynchronous on
 * the stream but are not meant for capture.
 *
 * The text forms need width == n_embd and a replica of the context on the store's GPU
 * (-1 otherwise).  _add_texts tokenises with bert_tokenize's rule, runs the per-token
 * forward (bertx_forward_tokens_device) on the store's GPU in chunks of at most 2^17
 * tokens and 4,096 texts, and packs the final hidden states from the forward's device
 * output: one document per text, len = the text's token count ([CLS] and [SEP]
 * included).  An input over n_max_tokens fails the whole call (-4) with nothing added.
 * _score_text does the same for one query; a query over 64 tokens (or over
 * n_max_tokens) fails with -4.
 *
 * bertx_bench_maxsim (device 0, no context): a store of n_docs documents of doc_len
 * random unit rows each (doc_len 0: ragged, 16 .. 512 by a hash of the id), a random
 * query of Lq rows, n_cand candidate ids spread over the store by a multiplicative
 * hash; average device time of `iters` calls of bertx_mvindex_score_device after 3
 * warm-up calls.
 *
 * Storage kinds.  bertx_mvindex_create_ex takes the kind: BERTX_INDEX_F16 (0) is exactly
 * bertx_mvindex_create, everything above; BERTX_INDEX_I8 (1) stores a token row as `width`
 * int8 values and one f32, width + 4 bytes instead of 2 width (the store allocates
 * slots * width bytes and slots * 4 bytes of scales); BERTX_INDEX_RES2 (4) and _RES4 (5)
 * are the kinds of "Residual codes" below (2 and 3 are no kinds); any other value returns NULL after
 * a message.  bertx_mvindex_storage returns the kind, -1 for NULL.  Every other entry
 * (_add, _add_device, _score, _score_device, _clear, _add_texts, _score_text and the two
 * _colbert text forms) follows the store's kind with the same signature, refusals,
 * stream ordering and capturability.  The int8 arithmetic, one quantizer for stored rows
 * and for query rows, every named operation rounded once to f32 (IEEE, nearest even):
 *   (q, _) = the embedding index's quantizer on the raw row x ("Storage kinds" above:
 *            amax = max_i |x_i|; amax == 0: all q_i = 0; else inv = 127 / amax,
 *            q_i = clamp(rint(x_i * inv), -127, 127)); its scale output is not kept;
 *   n2     = sum_i q_i * q_i in int32: exact, n2 <= 127 * 127 * 1024 < 2^24, so (float)n2
 *            is exact;
 *   n2 == 0: u = 0;  otherwise u = 1 / sqrt((float)n2) (sqrt, then the division);
 *   stored: the `width` bytes q and the one f32 u; the dequantized row q_i * u has unit
 *            length to f32 rounding;
 *   sim(a, c)  = (float)isum * (u_a * u_c), isum = sum_i qa_i * qc_i in int32 (exact);
 *   score(doc) = sum_{i < Lq} max_{j < len} sim(q_i, c_j): the max is exact; the sum over
 *            i is the f16 scorer's order, spelled out: lane c (0 .. 15) adds m[c],
 *            m[16 + c], ... in ascending order from +0 (a query index >= Lq adds +0),
 *            then s += shfl_xor(s, o) for o = 8, 4, 2, 1 (lane l adds lane l ^ o's value
 *            of the step before); lane 0 is the score.
 * Nothing in this depends on a summation order the caller cannot reproduce (normalising
 * after quantizing makes the norm an exact integer), so a restatement in float32 gives
 * the bytes, the scales and the scores bit for bit.  The invariances of the f16 store
 * hold word for word: a score depends on the query and on that document's rows only, not
 * on its id, the other documents, the candidate list or its order.  Slots of a
 * document's last group past len, and their scale slots, are never counted whatever they
 * hold: they become -inf through a select.  Non-finite input, or an amax so small that
 * 127 / amax overflows, gives unspecified values inside the clamp.
 * Accuracy against the exact cosine: with x' = 127 x / amax in real arithmetic and
 * e_x = |q - x'|_2 / |x'|_2 the relative quantization error of a row, the unit vectors
 * differ by at most 2 e_x, so
 *   |sim - cos(x, y)| <= 2 (e_x + e_y) + 2^-21,
 * the 2^-21 covering the sqrt, the division, the two multiplies and the f32 rounding of
 * (float)isum * (u_a * u_c).  int8 is the less precise kind: about 1e-2 per similarity
 * on rows with a few channels 20 times larger than the rest.
 * bertx_mvindex_doc on an int8 store returns (float)q * u (one f32 multiply);
 * bertx_mvindex_doc_i8 returns the stored bytes q int8[len][width] and scales
 * u float[len], or -1 on an f16 store or a bad id with the outputs untouched.
 * bertx_bench_maxsim_ex is bertx_bench_maxsim over a store of the given kind.
 *
 * Full-scan search: the k best documents of the whole store, several queries per call.
 * bertx_mvindex_search / _search_device: q is float[B][Lq][width], B >= 1 queries of
 * exactly Lq rows each, 1 <= Lq <= 64, 1 <= k <= 128; scores is float[B][k] and ids
 * int32[B][k].  Per query the entries come best first, equal scores by ascending id; with
 * fewer than k documents the remaining slots are (-inf, -1), so an empty store gives all
 * fill.  score(query, doc) is, bit for bit, what bertx_mvindex_score returns for that
 * query and document on the same store, f16 and int8 alike: it does not depend on the
 * other queries of the call, B, k, the document count or where the document sits.
 * A shorter query is padded by the caller with all-zero rows: a zero row normalises to
 * zeros (u = 0 on an int8 store), its similarity to every stored row is +0, so it adds
 * +0 to the sum exactly as a query index >= Lq does in the scorer, and the padded query's
 * scores are the bits of the unpadded one's.  That is why one Lq per call suffices.
 * Queries of ceil(Lq / 16) = 1, 2, 3, 4 tiles share one pass over the stored bytes 4, 2,
 * 1, 1 at a time; a call runs ceil(B / that) passes.  A refusal (B, Lq or k out of range,
 * a NULL pointer) returns -1 after a message with the outputs untouched.  The device form
 * follows bertx_mvindex_score_device word for word: device pointers on the store's GPU
 * and a hipStream_t (NULL: the store's own stream), asynchronous, ordered after the
 * store's previous operation, allocating nothing (the partial lists, 128 pairs of 8 B
 * for 4 queries and up to 1,024 + 32 lists = 4.1 MiB, belong to the store) and never synchronising,
 * so it can be captured into a HIP graph; a captured search keeps the document count of
 * its capture.  The host form stages through the store's stream.
 * bertx_mvindex_search_texts: n queries tokenised as _score_text tokenises one, one
 * batched per-token forward on the store's GPU per 1,024 queries, the rows laid out
 * [n][Lmax][width] on the device with zero rows behind the shorter queries, then the
 * search; needs what _score_text needs.  A query over 64 tokens (or over n_max_tokens)
 * fails the whole call with -4 and the outputs untouched.
 * bertx_mvindex_search_texts_colbert ("Projection" below): the same over the augmented
 * queries of query_maxlen tokens each, through the projector; refusals as
 * _score_text_colbert.
 * bertx_bench_maxsim_search: the store of bertx_bench_maxsim_ex, B random queries of Lq
 * rows; average device time of `iters` calls of bertx_mvindex_search_device after 3
 * warm-up calls.
 *
 * Centroid codes.  A store can keep C centroids and one uint16 code per token slot: the
 * index of the centroid nearest to the slot's stored row.  Without centroids every entry
 * above does what it did; with them the add forms also code the rows they store, in the
 * same stream order.
 * bertx_mvindex_set_centroids(mv, cent float[C][width] on the host, C): C a multiple of 16
 * in 16 .. 65,536 (-1 otherwise).  The rows are packed by the store's own row packer (the
 * arithmetic above, f16 or int8), so a centroid holds exactly the bits that a one-token
 * document added from the same f32 row would hold.  The call (re)assigns the code of every
 * stored token; a second call replaces the centroids and assigns every code again; _clear
 * keeps the centroids.  The buffers (the centroids, codes for capacity_token_slots, the
 * table scratch of 256 C bytes, the candidate lists of 64 queries) are allocated by the
 * first call and reallocated only when C grows; an allocation failure returns -3 with
 * nothing changed.  The call synchronises with the store's stream.  A HIP graph captured
 * before a set_centroids call must not be replayed after it: it holds the old buffers'
 * addresses and the old C.
 * The code of a stored row is a contract in terms of the entries above.  Let S_c be a
 * store of the same kind and width whose documents are the centroids, one row each, added
 * from the same f32 rows, and x what bertx_mvindex_doc returns for the row (the stored
 * values widened; q * u on int8).  Then
 *   code = the id that bertx_mvindex_search(S_c, x, B = 1, Lq = 1, k = 1) returns:
 * the centroid of highest sim in the scorer's arithmetic, x going through the query packer
 * (the normaliser runs again; on f16 it is not idempotent), equal similarities to the
 * lower index.  A row stored as zeros gets code 0.  The slots of a document's last group
 * past len hold code 0, so that a lookup is always in range; they never count towards a
 * score.
 * _centroids: the count, 0 if none.  _centroid(mv, c, out float[width]): the stored values
 * of centroid c widened, as _doc.  _doc_codes(mv, id, codes uint16[len]): a document's codes
 * (-1 without centroids or for a bad id, outputs untouched).
 * bertx_mvindex_train_centroids(mv, C, iters, seed): spherical k-means, reproducible from
 * the entries above.  Number the valid token rows 0 .. T - 1 in (document, token) order;
 * the sample is every stride-th of them from row seed % stride on, stride =
 * max(1, ceil(T / 2^18)), n_sample rows, their values _doc's.  The initial centroid c is
 * sample row floor(c n_sample / C).  Each of the `iters` iterations calls _set_centroids
 * (which codes the whole store on the GPU), reads the sample's codes, and replaces centroid
 * c by the sum of its members, in f64, added one after the other in ascending sample order,
 * divided by the count (f64) and rounded to f32; a centroid without a member keeps its f32
 * row.  A final _set_centroids leaves the store coded.  The update runs on the host without
 * atomics, so two runs give the same bits.  -1: C out of range or above n_sample, an empty
 * store, iters < 0.
 *
 * Pruned search: centroid interaction first, the exact scorer on the survivors.
 * bertx_mvindex_candidates / _candidates_device(mv, q float[B][Lq][width], B, Lq, n_cand,
 * approx float[B][n_cand], ids int32[B][n_cand]), 1 <= Lq <= 64, 1 <= n_cand <= 128:
 *   T[i][c]        = sim(q_i, centroid c) in the store's sim, the query packed as the
 *                    scorers pack it;
 *   approx(q, doc) = sum_{i < Lq} max_{j < len} T[i][code_j]: the max is exact, the sum in
 *                    the scorer's order (lane c adds m[c], m[16 + c], ... from +0, then the
 *                    four-step butterfly).
 * So approx(q, doc) is, bit for bit, what bertx_mvindex_score returns for q on a store in
 * which that document's rows were added from the caller's f32 centroid rows cent[code_j].
 * Per query the n_cand best documents by (approx, then ascending id) come first to last,
 * (-inf, -1) where the store has fewer.  A result does not depend on B, the other queries,
 * n_cand, the document count or where the document sits.  A pass of 4, 2, 1 or 1 queries (1,
 * 2, 3 or 4 tiles of 16 rows) runs a table kernel on the matrix cores, a scan that reads
 * only the 2-byte codes, and a selection that merges the workgroups' sorted lists.  The
 * scan copies the table into LDS when its 64 * tiles * C bytes (three tiles take the line of
 * four) fit beside the lists in 160 KiB (C up to about 512 at four tiles, 2,048 at one) and
 * reads it from global memory otherwise; both give the same bits;
 * bertx_test_approx_ran reports which ran (bit 0: LDS, bit 1: global; a non-zero argument
 * also resets it).
 * bertx_mvindex_search_pruned / _search_pruned_device(mv, q, B, Lq, k, n_cand, scores
 * float[B][k], ids int32[B][k]), 1 <= k <= n_cand <= 128: per query the n_cand candidates,
 * their exact scores by the scorer kernel, then the k best by (score, ascending id), (-inf,
 * -1) fill.  The scores are the scorer's bits; with n_cand >= docs the result is
 * bertx_mvindex_search's, bit for bit.  The candidate scratch belongs to the store.  The
 * device forms follow _search_device word for word (asynchronous, ordered after the store's
 * previous operation, allocating nothing, never synchronising, capturable).
 * bertx_mvindex_search_pruned_texts: _search_texts (colbert_query_maxlen 0) or
 * _search_texts_colbert (the augmented queries of that many tokens) with the pruned search
 * in place of the full scan; their refusals.
 * Refusals, a message and the outputs untouched: -1 for arguments out of range, for a store
 * without centroids and for a C that is not a multiple of 16; -4 for over-long texts.
 * bertx_bench_maxsim_pruned: the store of bertx_bench_maxsim_ex with C hash-chosen stored
 * rows as centroids; avg_us[0 .. 2] = the table kernels, the scans with their selections,
 * and the whole pruned search of B queries, each the average of `iters` calls after 3.
 *
 * Residual codes (ColBERTv2's compression).  BERTX_INDEX_RES2 (4) and BERTX_INDEX_RES4 (5)
 * for bertx_mvindex_create_ex keep no token row: per token slot the uint16 centroid code
 * (the `codes` of "Centroid codes"), NB = 2 or 4 bits per element (width * NB / 8 bytes of
 * bucket indices) and one f32 u, width * NB / 8 + 6 bytes in all (38 at width 128, NB 2,
 * against 256 + 2 in f16 and 132 + 2 in int8).  Widths as above.  bertx_index_create_ex, the
 * embedding index, refuses both kinds.  The centroids of a residual store are packed by the
 * f16 row packer: they hold exactly the bits that an f16 store given the same `cent` rows
 * holds.
 * bertx_mvindex_set_residual_buckets(mv, cutoffs float[2^NB - 1], weights float[2^NB]): the
 * codec.  Cutoffs finite and non-decreasing, weights finite (-1 otherwise).  The store keeps
 * cut_k as f32 and wt_k = f16(weights[k]), nearest even.  Refused (-1, a message, nothing
 * changed) on an f16 or int8 store and on a residual store that holds documents; _clear
 * keeps centroids and buckets.
 * The arithmetic, every named operation rounded once.  For a source row x let F be an f16
 * store of the same width with the same centroids (the "twin"):
 *   v    = the unit f16 row of pack_row_f16, the bits F stores and bertx_mvindex_doc(F)
 *          returns;
 *   code = the code F assigns ("Centroid codes" above); c = that centroid's stored f16 values;
 *   r_i  = f32(v_i) - f32(c_i), one f32 subtraction;
 *   b_i  = #{k : cut_k < r_i}, in 0 .. 2^NB - 1;
 *   e_i  = c_i + wt[b_i], ONE IEEE f16 addition, nearest even, f16 subnormals kept (what
 *          v_pk_add_f16 computes, and what np.float16 + np.float16 computes: numpy adds in
 *          f32 and rounds again, which is innocuous because 24 >= 2 * 11 + 2);
 *   ss   = sum_i e_i^2 taken exactly: every finite f16 is a multiple of 2^-24, every square
 *          a multiple of 2^-48, so an f64 accumulation in any order is exact while ss < 32
 *          (a unit centroid plus a small residual keeps ss near 1); ss >= 32 or a non-finite
 *          e gives unspecified values;
 *   s    = (float)ss;  u = 1 / sqrtf(s) (sqrt, then the division) if ss > 0, else 0;
 *   stored: code, the b_i and u;
 *   sim(q, tok) = acc * u, one f32 multiply; acc is the f16 scorer's accumulation of q16 . e:
 *          the query through pack_row_f16, the width / 32 v_mfma_f32_16x16x32_f16 in
 *          ascending k from a zero accumulator;
 *   score(doc)  = sum_i max_j sim(q_i, tok_j): the max exact, slots past len -inf through a
 *          select whatever bits, code and u they hold, the sum in the scorer's order (lane c
 *          adds m[c], m[16 + c], ... from +0, then the butterfly 8, 4, 2, 1).
 * Nothing stored depends on an order the caller cannot reproduce, so a restatement in numpy
 * gives code, bits and u bit for bit; acc is an MFMA sum, so scores are checked as the f16
 * store's are, against the float64 MaxSim of (q16, e, u).  The bound: |q16| and |e u| are
 * at most 1 + 2^-10 each, the accumulation of `width` products adds at most width * 2^-24
 * per similarity as in the f16 store (an |e| of 1 / u scales acc and its error alike, and u
 * scales both back), |acc * u| < 2 so its one extra rounding adds at most 2^-24 per
 * similarity, once per query row after the exact max, and the f32 sum of the Lq maxima is
 * the f16 store's (u itself is the same f32 on both sides of the comparison):
 *   |score - exact| <= Lq (2 width + Lq) 2^-24 + Lq 2^-24.
 * The invariances of the f16 store hold word for word (id, the other documents, the
 * candidate list and its order).  One add call of n documents stores the bits that n calls
 * of one document store.
 * An add (_add, _add_device and the text forms) is refused (-1) without centroids or without
 * buckets.  It packs the call's rows into a staging image of the store's own (2 * width
 * bytes per token slot of the largest call so far), codes them with the f16 assign kernel
 * and encodes; slots past len get code 0.
 * Readback: bertx_mvindex_doc returns (float)e_i * u.  bertx_mvindex_doc_residual(mv, id,
 * codes uint16[len], bits uint8[len][width * NB / 8], u float[len]): element i sits in byte
 * i * NB / 8 at bit offset NB * (i mod (8 / NB)), low bits first; -1 on another kind or a bad
 * id, outputs untouched.  _doc_i8 stays -1.
 * _score / _score_device, _candidates* and _search_pruned* (and _search_pruned_texts) work
 * as on the other kinds, with the same signatures, stream ordering and capturability: the
 * candidates from the f16 table kernel and the code scan, the exact stage by a scorer that
 * gathers each candidate row's centroid chunks by its code and decodes them straight into
 * the MFMA fragments.  Refused on a residual store (-1, a message, outputs untouched):
 * _search, _search_device, _search_texts and _search_texts_colbert (the full scan of a
 * residual store is not provided); _train_centroids (no rows to train from); _set_centroids
 * once documents are stored (no rows to code again).
 * bertx_mvindex_train_residual_buckets(src, nbits, cutoffs, weights): ColBERTv2's quantile
 * rule on the host, deterministic.  src is an f16 store with centroids and documents (-1
 * otherwise; nbits 2 or 4).  The valid token rows in (document, token) order, every
 * stride-th from row 0, stride = max(1, ceil(T / 2^16)); all n = rows * width residuals r as
 * above (v, code and c from _doc, _doc_codes and _centroid), sorted ascending;
 *   cutoffs[k - 1] = sorted[min(n - 1, floor(k n / 2^NB))],  k = 1 .. 2^NB - 1;
 *   weights[k]     = sorted[min(n - 1, floor((2k + 1) n / 2^(NB + 1)))];  no interpolation.
 * The workflow: fill an f16 store with a sample; _train_centroids on it; read the centroids
 * back with _centroid; train the buckets; create the residual store; _set_centroids and
 * _set_residual_buckets; add the corpus.
 * bertx_bench_maxsim_res: the documents of bertx_bench_maxsim_ex in a residual store, C
 * hash-chosen rows of the f16 twin as centroids and buckets trained from it; avg_us[0] =
 * bertx_mvindex_score_device over n_cand candidates, avg_us[1] = the pruned search of one
 * query for the 10 best of min(n_cand, 128) candidates; each the average of `iters` calls
 * after 3.
 *
 * Deleting documents and filtered search.  The embedding index's section word for word, a
 * document in the place of a row.  Two masks over document ids, both packed 32 documents to a
 * uint32_t word: document i is bit i % 32 of word i / 32 (np.packbits(x, bitorder="little")
 * viewed as uint32).  Tombstones belong to the store, lie on its device, cover capacity_docs
 * and are allocated and zeroed at creation; bit 1 = deleted.  Filters are the caller's, per
 * call; bit 1 = the document may be returned.  A document is admissible for query b iff
 * id < docs, its tombstone is 0 and, when a filter is given, its bit in query b's filter is 1.
 * bertx_mvindex_remove / _remove_device (ids int32[n], host / device; n >= 1, anything else a
 * negative error with nothing changed): sets the tombstones of the listed ids and returns 0.
 * Ids outside [0, docs), docs being the document count when the call is made, are ignored;
 * repeated ids are harmless; the bits are set by atomic OR, so no order matters.  The device
 * form is asynchronous, allocates nothing, never synchronises, can be captured, and is
 * ordered as bertx_mvindex_add_device is.  Ids are never reused: bertx_mvindex_docs and
 * _token_slots do not change, and _doc, _doc_len, _doc_i8, _doc_codes and _doc_residual still
 * return a deleted document's stored values.  bertx_mvindex_clear also zeroes the tombstones
 * (ordered on the store's stream), so a clear followed by adds starts clean.
 * bertx_mvindex_live: docs minus the deleted documents in [0, docs); a host call that
 * synchronises.  bertx_mvindex_deleted: out uint8[n] = 0 or 1 for documents first .. first +
 * n - 1; -1 on a bad range with the output untouched.
 * bertx_mvindex_search_filtered / _device(mv, q, B, Lq, k, filters, n_filters, words, scores,
 * ids[, stream]): bertx_mvindex_search over the admissible documents.  filters
 * uint32[n_filters][words] (host / device); n_filters is 1 (one filter for every query) or B
 * (query b uses filter b); words >= ceil(docs / 32) is also the stride between filters; bits
 * of documents >= docs are ignored, whatever they hold.  filters == NULL with n_filters == 0
 * is exactly bertx_mvindex_search.  The result is the k best admissible documents with the
 * scorer's score bits, the same order (score descending, id ascending) and the same (-inf,
 * -1) fill when fewer than k documents are admissible; a deleted or filtered document never
 * appears, not even as (-inf, id).  Every refusal (a null pointer, n_filters not 0, 1 or B,
 * too few words, a filter pointer without a count or the reverse, and the refusals of
 * _search) returns a negative error with the outputs untouched.  The device form allocates
 * nothing and can be captured; the host form allocates and frees a staging buffer for the
 * filters per call.  The filter is read when the kernel runs: a captured search sees the bits
 * the buffer holds at replay.  A filter is not read while the store is empty.
 * bertx_mvindex_candidates_filtered / _device and bertx_mvindex_search_pruned_filtered /
 * _device take the same three filter arguments, for all four storage kinds: the candidates are
 * the n_cand best admissible documents by (approx, ascending id), and the pruned search is
 * literally the composition stated under "Pruned search" with that as its first line; the
 * exact stage takes the store's tombstones.  With n_cand >= the number of admissible documents
 * it equals _search_filtered, bit for bit.
 * On a store with deletions the entries above follow: _search, _candidates, _search_pruned,
 * their device forms and the text forms (_search_texts, _search_texts_colbert,
 * _search_pruned_texts) return admissible documents only; _score / _score_device /
 * _score_text (and _score_text_colbert) give -inf for a deleted id, exactly as for an id
 * outside [0, docs), on the f16, int8 and residual scorers alike.  Training ignores
 * tombstones: _train_centroids, _train_residual_buckets and _set_centroids keep numbering and
 * coding every stored token row, deleted documents' rows included, so their contracts above
 * stay true word for word.
 * A store from which nothing was removed since creation or the last clear, searched without a
 * filter, launches the kernels it launched before masks existed, with the same arguments: the
 * masked kernels are other instantiations, chosen at launch time by a host flag that any
 * accepted remove sets and clear resets (a graph captured before the first removal keeps
 * launching the unmasked kernels).
 *
 * Not provided: int8 queries against f16 rows; the full scan of a residual store, 1-bit
 * codes; candidate lists longer than 128; per-query lengths on the device; sharding over
 * GPUs; compaction (reclaiming deleted documents' slots or renumbering); skipping the loads of
 * masked documents; a gather path for very selective filters (bertx_mvindex_score over listed
 * ids already serves those); filtered text forms in C; saving and loading.  (ColBERT
 * checkpoints: "Projection" below.)
 */
enum { BERTX_INDEX_RES2 = 4, BERTX_INDEX_RES4 = 5 };   /* token stores only: "Residual codes" above */
struct bertx_mvindex;
BERT_API struct bertx_mvindex *bertx_mvindex_create(struct bert_ctx *ctx, int32_t slot, int32_t width,
                                                    int32_t capacity_docs, int64_t capacity_token_slots);
BERT_API struct bertx_mvindex *bertx_mvindex_create_ex(struct bert_ctx *ctx, int32_t slot, int32_t width,
                                                       int32_t capacity_docs, int64_t capacity_token_slots,
                                                       int32_t storage);
BERT_API int32_t bertx_mvindex_storage(struct bertx_mvindex *mv);
BERT_API int32_t bertx_mvindex_doc_i8(struct bertx_mvindex *mv, int32_t id, int8_t *q, float *u);
BERT_API int32_t bertx_bench_maxsim_ex(int32_t w, int32_t n_docs, int32_t doc_len, int32_t Lq, int32_t n_cand,
                                       int32_t storage, int32_t iters, float *avg_us);
BERT_API void bertx_mvindex_free(struct bertx_mvindex *mv);
BERT_API int32_t bertx_mvindex_clear(struct bertx_mvindex *mv);
BERT_API int32_t bertx_mvindex_docs(struct bertx_mvindex *mv);
BERT_API int64_t bertx_mvindex_token_slots(struct bertx_mvindex *mv);
BERT_API int32_t bertx_mvindex_capacity_docs(struct bertx_mvindex *mv);
BERT_API int64_t bertx_mvindex_capacity_token_slots(struct bertx_mvindex *mv);
BERT_API int32_t bertx_mvindex_dim(struct bertx_mvindex *mv);
BERT_API int32_t bertx_mvindex_add(struct bertx_mvindex *mv, const float *rows, const int32_t *lens, int32_t n);
BERT_API int32_t bertx_mvindex_add_device(struct bertx_mvindex *mv, const float *d_rows, const int32_t *lens, int32_t n,
                                          void *stream);
BERT_API int32_t bertx_mvindex_doc_len(struct bertx_mvindex *mv, int32_t id);
BERT_API int32_t bertx_mvindex_doc(struct bertx_mvindex *mv, int32_t id, float *out);
BERT_API int32_t bertx_mvindex_score(struct bertx_mvindex *mv, const float *q, int32_t Lq, const int32_t *ids, int32_t n,
                                     float *out);
BERT_API int32_t bertx_mvindex_score_device(struct bertx_mvindex *mv, const float *d_q, int32_t Lq, const int32_t *d_ids,
                                            int32_t n, float *d_out, void *stream);
BERT_API int32_t bertx_mvindex_add_texts(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                         const char **texts);
BERT_API int32_t bertx_mvindex_score_text(struct bertx_mvindex *mv, struct bert_ctx *ctx, const char *query,
                                          const int32_t *ids, int32_t n, float *out);
BERT_API int32_t bertx_bench_maxsim(int32_t w, int32_t n_docs, int32_t doc_len, int32_t Lq, int32_t n_cand,
                                    int32_t iters, float *avg_us);
BERT_API int32_t bertx_mvindex_search(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t k,
                                      float *scores, int32_t *ids);
BERT_API int32_t bertx_mvindex_search_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq, int32_t k,
                                             float *d_scores, int32_t *d_ids, void *stream);
BERT_API int32_t bertx_mvindex_search_texts(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                            const char **texts, int32_t k, float *scores, int32_t *ids);
BERT_API int32_t bertx_bench_maxsim_search(int32_t w, int32_t n_docs, int32_t doc_len, int32_t Lq, int32_t B, int32_t k,
                                           int32_t storage, int32_t iters, float *avg_us);
BERT_API int32_t bertx_mvindex_set_centroids(struct bertx_mvindex *mv, const float *cent, int32_t C);
BERT_API int32_t bertx_mvindex_train_centroids(struct bertx_mvindex *mv, int32_t C, int32_t iters, uint32_t seed);
BERT_API int32_t bertx_mvindex_centroids(struct bertx_mvindex *mv);
BERT_API int32_t bertx_mvindex_centroid(struct bertx_mvindex *mv, int32_t c, float *out);
BERT_API int32_t bertx_mvindex_doc_codes(struct bertx_mvindex *mv, int32_t id, uint16_t *codes);
BERT_API int32_t bertx_mvindex_candidates(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t n_cand,
                                          float *approx, int32_t *ids);
BERT_API int32_t bertx_mvindex_candidates_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq,
                                                 int32_t n_cand, float *d_approx, int32_t *d_ids, void *stream);
BERT_API int32_t bertx_mvindex_search_pruned(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t k,
                                             int32_t n_cand, float *scores, int32_t *ids);
BERT_API int32_t bertx_mvindex_search_pruned_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq,
                                                    int32_t k, int32_t n_cand, float *d_scores, int32_t *d_ids,
                                                    void *stream);
BERT_API int32_t bertx_mvindex_search_pruned_texts(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads,
                                                   int32_t n, const char **texts, int32_t k, int32_t n_cand,
                                                   int32_t colbert_query_maxlen, float *scores, int32_t *ids);
BERT_API int32_t bertx_bench_maxsim_pruned(int32_t w, int32_t n_docs, int32_t doc_len, int32_t C, int32_t Lq, int32_t B,
                                           int32_t k, int32_t n_cand, int32_t storage, int32_t iters, float *avg_us);
BERT_API int32_t bertx_mvindex_set_residual_buckets(struct bertx_mvindex *mv, const float *cutoffs, const float *weights);
BERT_API int32_t bertx_mvindex_train_residual_buckets(struct bertx_mvindex *src, int32_t nbits, float *cutoffs,
                                                      float *weights);
BERT_API int32_t bertx_mvindex_doc_residual(struct bertx_mvindex *mv, int32_t id, uint16_t *codes, uint8_t *bits, float *u);
BERT_API int32_t bertx_bench_maxsim_res(int32_t w, int32_t n_docs, int32_t doc_len, int32_t C, int32_t Lq, int32_t n_cand,
                                        int32_t storage, int32_t iters, float *avg_us);
/* "Deleting documents and filtered search" above. */
BERT_API int32_t bertx_mvindex_remove(struct bertx_mvindex *mv, const int32_t *ids, int32_t n);
BERT_API int32_t bertx_mvindex_remove_device(struct bertx_mvindex *mv, const int32_t *d_ids, int32_t n, void *stream);
BERT_API int32_t bertx_mvindex_live(struct bertx_mvindex *mv);
BERT_API int32_t bertx_mvindex_deleted(struct bertx_mvindex *mv, int32_t first, int32_t n, uint8_t *out);
BERT_API int32_t bertx_mvindex_search_filtered(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t k,
                                               const uint32_t *filters, int32_t n_filters, int32_t words, float *scores,
                                               int32_t *ids);
BERT_API int32_t bertx_mvindex_search_filtered_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq,
                                                      int32_t k, const uint32_t *d_filters, int32_t n_filters,
                                                      int32_t words, float *d_scores, int32_t *d_ids, void *stream);
BERT_API int32_t bertx_mvindex_candidates_filtered(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq,
                                                   int32_t n_cand, const uint32_t *filters, int32_t n_filters,
                                                   int32_t words, float *approx, int32_t *ids);
BERT_API int32_t bertx_mvindex_candidates_filtered_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq,
                                                          int32_t n_cand, const uint32_t *d_filters, int32_t n_filters,
                                                          int32_t words, float *d_approx, int32_t *d_ids, void *stream);
BERT_API int32_t bertx_mvindex_search_pruned_filtered(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq,
                                                      int32_t k, int32_t n_cand, const uint32_t *filters, int32_t n_filters,
                                                      int32_t words, float *scores, int32_t *ids);
BERT_API int32_t bertx_mvindex_search_pruned_filtered_device(struct bertx_mvindex *mv, const float *d_q, int32_t B,
                                                             int32_t Lq, int32_t k, int32_t n_cand,
                                                             const uint32_t *d_filters, int32_t n_filters, int32_t words,
                                                             float *d_scores, int32_t *d_ids, void *stream);
/* bertx_bench_maxsim_masked: bertx_bench_maxsim_search (C == 0; avg_us[0]) or
 * bertx_bench_maxsim_pruned (C > 0; avg_us[0 .. 2]) of the same store under a mask pattern:
 * 0 none (the unmasked kernels); 1 one all-ones filter for every query; 2 an all-ones filter
 * per query; 3 a shared filter that admits a hashed 1 / 16 of the documents; 4 a shared
 * filter that admits the contiguous first 1 / 16; 5 no filter, a hashed 1 / 16 of the
 * documents removed.  -1 for another pattern. */
BERT_API int32_t bertx_bench_maxsim_masked(int32_t w, int32_t n_docs, int32_t doc_len, int32_t C, int32_t Lq, int32_t B,
                                           int32_t k, int32_t n_cand, int32_t storage, int32_t pattern, int32_t iters,
                                           float *avg_us);
/* Test hooks: which table placement the candidate scans took; the host half of training
 * (kmeans_update.h): one update in place, returning the centroids without a member; the
 * sample rule, out3 = {stride, start, n_sample}. */
BERT_API int32_t bertx_test_approx_ran(int32_t reset);
/* Test hooks: a cap on the grids of one store's scans.  The scorers, the full scan and the
 * centroid scan size their grids by the device's CU count, so at a test's store a wave sees
 * a handful of documents where production gives it hundreds.  max_wg > 0 bounds the
 * workgroups of every scan kernel launched for this store from then on (score, search,
 * candidates, search_pruned, their _device and text forms), applied after the launcher's
 * own rule and before the selection levels that follow from it; 0 removes the cap.  Returns
 * the previous value, or -1 for a negative max_wg (or a null store) with nothing changed.
 * A capped scan returns what the uncapped one returns, bit for bit: a score depends on the
 * query and the document alone.
 * bertx_test_mvindex_last_grid: the workgroups of the scan kernel (not of the selection
 * behind it) at the store's most recent scan launch, 0 before the first.
 * bertx_test_mvindex_last_masked: 1 if the store's most recent scan or scorer launch was a
 * masked instantiation ("Deleting documents and filtered search"), 0 otherwise, including
 * before the first launch. */
BERT_API int32_t bertx_test_mvindex_grid(struct bertx_mvindex *mv, int32_t max_wg);
BERT_API int32_t bertx_test_mvindex_last_grid(struct bertx_mvindex *mv);
BERT_API int32_t bertx_test_mvindex_last_masked(struct bertx_mvindex *mv);
BERT_API int32_t bertx_test_kmeans_update(const float *sample, const uint16_t *codes, int32_t n, int32_t w, int32_t C,
                                          float *cent);
BERT_API int32_t bertx_test_kmeans_sample(int64_t T, uint32_t seed, int64_t *out3);

/*
 * Cross-encoder reranking: token types and a classification head.
 *
 * Model file.  Four optional records behind the encoder's: pooler.dense.weight
 * [d][d] in the header ftype (the quantizer quantizes it), pooler.dense.bias [d] f32,
 * classifier.weight ne = {d, n_labels}, always 2-D and f32 in every ftype (the
 * quantizer copies it through), classifier.bias [n_labels] f32; 1 <= n_labels <= 16.
 * All four or none: a partial head is a load error.  A file without them loads and
 * runs as before.  bertx_convert_hf_head is bertx_convert_hf followed by the four
 * records, from a BertForSequenceClassification directory (pooler.dense.* or
 * bert.pooler.dense.*, un-prefixed classifier.*); it refuses (message, non-zero) a
 * checkpoint without a classifier or a pooler.  bertx_n_labels: the head's label
 * count, 0 for a file without one; works on tokenizer-only contexts.
 *
 * bertx_tokenize_pair: one (A, B) pair as [CLS] A [SEP] B [SEP], types 0 for [CLS] A
 * [SEP] and 1 for B [SEP] (an empty B keeps its [SEP]).  The WordPiece ids of each
 * text are bert_tokenize's for that text alone.  The pieces share m = n_max - 3.
 * truncate 0: a pair over budget is refused ("Too many tokens"), -4, *n_tokens the
 * full count, ids / types untouched.  truncate 1: Hugging Face's longest_first in
 * closed form; with s the shorter side, 2 s <= m keeps it whole and m - s pieces of
 * the longer, otherwise A keeps ceil(m / 2) and B floor(m / 2); pieces drop from the
 * end of a side.  Returns 0 with *n_tokens <= n_max ids and types stored; -1 for bad
 * arguments (n_max < 3).  Works on tokenizer-only contexts.
 *
 * bertx_forward_device_ex: bertx_forward_device with token types and a named output.
 * d_types: int32[total_tokens] on that GPU, packed as d_ids, or NULL for all 0 (then
 * POOLED and TOKENS give the bits of bertx_forward_device and
 * bertx_forward_tokens_device).  The device entry trusts every type to be 0 or 1:
 * the type table has two rows and another value reads outside it; the host entries
 * below check.  BERTX_OUT_LOGITS writes float[n_seqs][n_labels], the raw logits
 * classifier(tanh(pooler(final LayerNorm row of [CLS]))): no sigmoid or softmax is
 * applied.  Under the f16-activation chain with CLS pruning on (bertx_set_cls_pruning)
 * the last layer runs on the sentences' first rows only, whatever the pooling mode.
 * A sentence's logits depend on its own ids and types only, bit for bit: not on its
 * place in the batch, the other sentences or n_seqs.  Returns as bertx_forward_device;
 * -6 for LOGITS on a file without a head, -1 for an unknown out_kind.
 *
 * Host entries (routing, chunking and replicas as bert_forward_batch; outputs at the
 * caller's indices; on any refusal a message, a negative return and logits
 * untouched): bertx_score_ids takes pre-tokenised pairs (types outside {0, 1}: -1; an
 * input over n_max_tokens: -4) into logits float[n][n_labels]; bertx_score_pairs
 * tokenises texts_a[i] / texts_b[i] with bertx_tokenize_pair's rule at n_max_tokens
 * on n_threads threads of the library's pool; bertx_rerank is bertx_score_pairs with
 * the query as every A, tokenised once.  -6 for a file without a head.
 */
enum { BERTX_OUT_POOLED = 0, BERTX_OUT_TOKENS = 1, BERTX_OUT_LOGITS = 2 };
BERT_API int32_t bertx_convert_hf_head(const char *dir_model, const char *fname_out, int32_t ftype);
BERT_API int32_t bertx_n_labels(struct bert_ctx *ctx);
BERT_API int32_t bertx_tokenize_pair(struct bert_ctx *ctx, const char *text_a, const char *text_b, int32_t truncate,
                                     bert_vocab_id *ids, int32_t *types, int32_t *n_tokens, int32_t n_max);
BERT_API int32_t bertx_forward_device_ex(struct bert_ctx *ctx, int32_t slot, const int32_t *d_ids,
                                         const int32_t *d_types, const int32_t *d_cu, int32_t n_seqs, int32_t max_len,
                                         int32_t total_tokens, int32_t out_kind, float *d_out, void *stream);
BERT_API int32_t bertx_score_ids(struct bert_ctx *ctx, int32_t n, bert_vocab_id **ids, int32_t **types,
                                 int32_t *n_tokens, float *logits);
BERT_API int32_t bertx_score_pairs(struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts_a,
                                   const char **texts_b, int32_t truncate, float *logits);
BERT_API int32_t bertx_rerank(struct bert_ctx *ctx, int32_t n_threads, const char *query, int32_t n_docs,
                              const char **docs, int32_t truncate, float *logits);

/*
 * Parity hooks of the head and of the typed embedding kernels (host buffers, device
 * 0; the rules of the row-kernel hooks above).  bertx_test_head: x f32 [n][d] (the
 * [CLS] rows), wp f32 [d][d], bp [d], wc f32 [n_labels][d], bc [n_labels] -> out f32
 * [out_rows][n_labels], rows < n = wc tanh(x wp^T + bp) + bc as the forward computes
 * it.  The device output starts as the caller's bytes (pre-fill NaN bits: rows n ..
 * out_rows - 1 must come back untouched) with guard rows of NaN bits behind it; -5: a
 * guard row was written.  bertx_test_embed_ln_types: bertx_test_embed_ln with types
 * int32 [T] (values 0 or 1, checked), or NULL for the kernel without types.
 */
BERT_API int32_t bertx_test_head(const float *x, int32_t n, int32_t d, const float *wp, const float *bp,
                                 const float *wc, const float *bc, int32_t n_labels, float *out, int32_t out_rows);
BERT_API int32_t bertx_test_embed_ln_types(int32_t mode, int32_t fmt_word, int32_t fmt_type, int32_t fmt_pos,
                                           int32_t rows_word, int32_t rows_pos, int32_t d, const void *word_rows,
                                           const void *type_rows, const void *pos_rows, const float *ln_w,
                                           const float *ln_b, const int32_t *ids, const int32_t *types,
                                           const int32_t *cu, int32_t n_seqs, int32_t max_len, void *out,
                                           float *stats, int32_t out_rows);

/*
 * Search micro-benchmark (device 0, no context): an index of N random unit rows of
 * width d, B random unit queries; average device time of `iters` calls of
 * bertx_index_search_device for the k best, after 3 warm-up calls.
 * bertx_bench_search_add_rate: rows per second of bertx_index_add_device filling an
 * index of N rows from device rows, 65,536 rows per call (device time).
 * The _ex forms take the index's storage kind; the plain forms are BERTX_INDEX_F16.
 */
BERT_API int32_t bertx_bench_search(int32_t d, int32_t N, int32_t B, int32_t k, int32_t iters, float *avg_us);
BERT_API int32_t bertx_bench_search_add_rate(int32_t d, int32_t N, double *add_rows_per_s);
BERT_API int32_t bertx_bench_search_ex(int32_t d, int32_t N, int32_t B, int32_t k, int32_t storage, int32_t iters,
                                       float *avg_us);
BERT_API int32_t bertx_bench_search_add_rate_ex(int32_t d, int32_t N, int32_t storage, double *add_rows_per_s);
/*
 * The two-stage search on the same data: a binary index and an index of kind `fine`
 * (BERTX_INDEX_F16 or _I8) of the same N rows.  avg_us[0]: bertx_index_search_rescored_device
 * (binary, fine, B, k, n_cand); avg_us[1]: bertx_index_score_ids_device on the fine index
 * over the binary search's n_cand ids alone; avg_us[2]: the binary search for n_cand alone.
 * Each the average device time of `iters` calls after 3 warm-up calls.
 */
BERT_API int32_t bertx_bench_search_rescored(int32_t d, int32_t N, int32_t B, int32_t k, int32_t n_cand, int32_t fine,
                                             int32_t iters, float *avg_us);

/*
 * Projection: ColBERT checkpoints (the `linear` record, the [Q] / [D] markers, [MASK]
 * query augmentation, the punctuation skiplist, a fused projector).
 *
 * Model file.  One optional record linear.weight, ne = {n_embd, dim}, in the header
 * ftype like any 2-D weight (bertx_quantize_file quantizes it by its general rule);
 * ColBERT's projection has no bias.  dim % 32 == 0 and 32 <= dim <= 256, else a load
 * error.  A file without the record loads and runs exactly as before; a file may carry
 * the record and the classification head.  bertx_convert_hf_colbert is bertx_convert_hf
 * followed by the record, from an HF_ColBERT directory (encoder tensors bert.*, the
 * projection the un-prefixed linear.weight [dim][hidden]); it refuses (message,
 * non-zero) a checkpoint without linear.weight, with a linear.bias, or with a shape the
 * loader would refuse, and prints one line when the directory's artifact.metadata says
 * attend_to_mask_tokens is false (see "Key counts").  bertx_proj_dim: the record's
 * dim, 0 for a file without one; bertx_proj_width = 64 ceil(dim / 64): the width of
 * every projected row and a legal bertx_mvindex_create width (a 96-dim checkpoint gives
 * 128-wide rows whose last 32 columns are +0, which changes no dot product).  Both work
 * on tokenizer-only contexts.
 *
 * Arithmetic of a projected row, every named operation rounded once to f32, nearest even:
 *   x     = the row's final-LayerNorm values, the bits BERTX_OUT_TOKENS gives for that row
 *   a_k   = f16(x_k), nearest even
 *   w_jk  = f16(W_jk), at load, from the library's own dequantized f32 values
 *   p_j   = sum_k a_k w_jk, f32 from 0 in ascending blocks of 32 k
 *           (v_mfma_f32_16x16x32_f16; the order inside a block is the instruction's)
 *   ss    = sum_{j < dim} p_j p_j, f32, in an order that depends on dim only
 *   ss == 0: the row is +0; else rinv = 1 / sqrt(ss) (sqrt, then the division),
 *   out_j = p_j * rinv;  out_j = +0 for dim <= j < width.
 * The same arithmetic runs under all three chains (the LayerNorm row is rounded to f16
 * in registers; no fold constants are involved).  A row's output depends on that row's
 * x and on W only, bit for bit: not on the batch, the row's position or the other rows.
 *
 * BERTX_OUT_PROJ (bertx_forward_device_ex): d_out is float[total_tokens][proj_width],
 * unit rows, what bertx_mvindex_add_device takes.  It follows no pooling mode and is
 * never pruned.  On a file without the record bertx_forward_device_ex knows no such kind
 * and returns -1, as it did before the record existed; the entries below, which exist
 * only for the projection, return -6 on such a file.
 * bertx_forward_project_device: the same with a row map d_rows int32[n_rows] on that
 * GPU (every value in [0, total_tokens), trusted): d_out is float[n_rows][proj_width],
 * row i the projection of token d_rows[i]; only mapped rows are computed.  d_rows NULL:
 * BERTX_OUT_PROJ (n_rows is ignored).  -6 on a file without the record.
 * bertx_forward_project: the host form, with the routing and refusals of
 * bertx_forward_tokens; out[i] receives float[n_tokens[i]][proj_width].
 *
 * bertx_tokenize_colbert (works on tokenizer-only contexts): the pieces are
 * bert_tokenize's for the text alone; ids 1 ([unused0], the [Q] marker), 2 ([unused1],
 * the [D] marker) and 103 ([MASK]) are hard-coded as the tokenizer hard-codes 100 / 101
 * / 102.  kind 0, a query: [CLS] [unused0] pieces[: maxlen - 3] [SEP], then [MASK] up
 * to maxlen; *n_tokens = maxlen; every keep 1.  kind 1, a document: [CLS] [unused1]
 * pieces[: maxlen - 3] [SEP]; keep[i] is 0 exactly where the token's vocab string is
 * one ASCII punctuation character (the 32 of Python's string.punctuation).  ids and
 * keep hold maxlen entries.  maxlen < 4 or > n_max_tokens, or another kind: -1.
 *
 * Store, text forms (both need bertx_mvindex_dim == bertx_proj_width, -1 otherwise, and
 * the record, -6 otherwise; a replica on the store's GPU as the plain text forms).
 * bertx_mvindex_add_texts_colbert: tokenises as documents at doc_maxlen, runs the
 * forward on the store's GPU in the chunks of _add_texts and projects only the kept
 * rows through the row map, so punctuation tokens attend and are attended to but are
 * not stored; a document's len is its kept count (at least 3); returns as _add (-2
 * with nothing added when the kept rows do not fit).
 * bertx_mvindex_score_text_colbert: the augmented query of query_maxlen tokens, all of
 * whose rows score; query_maxlen > 64 (or < 4, or > n_max_tokens): -1.
 *
 * bertx_test_project (parity hook; host buffers, device 0, the rules of the row-kernel
 * hooks): mode 0: src = z f16 [T][d] with stats float [T][2] (mean, 1/sigma), g, b f32
 * [d]; mode 1: src = x f32 [T][d] (stats, g, b ignored).  W f32 [dim][d]; rows int32
 * [n_out] (values in [0, T), checked) or NULL for the identity with n_out = T.  out
 * f32 [out_rows][proj_width]: the device output starts as the caller's bytes and is
 * copied back whole, with guard rows of NaN bits behind it; -5: a guard row was
 * written; -1: a shape the kernel refuses or out_rows < n_out.
 * bertx_bench_project (device 0, no context): mode 0 on T random rows; average device
 * time of `iters` launches after 3 warm-up launches.
 *
 * Key counts: [MASK] rows that are not attention keys (ColBERT's attend_to_mask_tokens =
 * false, the setting colbertv2.0 was trained with).  A sentence of len rows may carry one
 * number keys, 1 <= keys <= len: all len rows are queries and produce output rows, only
 * the first keys rows are keys and values of every layer's attention -- HF's
 * attention_mask of a right-padded row, on the packed layout.  In every attention
 * kernel of the three chains a key j >= keys scores -inf through the mask that handles
 * j >= len (its P is exactly 0); K / V loads and the 64-key block loops run over
 * ceil(keys / 64) blocks, an excluded block is neither loaded nor multiplied; the query
 * rows, the Q loads and the stores stay bounded by len.  Nothing else of the forward
 * changes.  A sentence's rows depend on its ids, its types and its key count only, bit
 * for bit: not on the batch, the order, or the kernel the batch selects.  With
 * keys == len the rows are those of the same call without counts.
 * bertx_forward_device_kv: bertx_forward_device_ex / bertx_forward_project_device with
 * d_keys int32[n_seqs] on that GPU (trusted: 1 <= d_keys[b] <= the sentence's length).
 * out_kind BERTX_OUT_TOKENS or BERTX_OUT_PROJ, any other -1 (the pooled and logits
 * outputs take no counts, so a forward with counts never runs the pruned last layer);
 * d_rows / n_rows: the row map of bertx_forward_project_device, used with PROJ only
 * (NULL: every row).  d_keys NULL: exactly the launches and bits of those two entries.
 * Asynchronous and capturable as they are; the pointer is part of a captured forward's
 * key.  -6: PROJ on a file without the record.
 * bertx_forward_tokens_kv / bertx_forward_project_kv: the host forms with n_keys int32[n],
 * one count per sentence, which travels with its sentence through the routing and the
 * chunks; a count outside 1 .. n_tokens[i] returns -1 with every output untouched;
 * n_keys NULL is bertx_forward_tokens / bertx_forward_project.
 * bertx_tokenize_colbert_ex: bertx_tokenize_colbert plus *n_keys: for a query the rows up
 * to and including [SEP], 3 + min(pieces, maxlen - 3); for a document *n_tokens.
 * bertx_set_mask_keys(ctx, on) / bertx_mask_keys: whether the ColBERT query forms of the
 * store keep the [MASK] rows as keys.  1 (the default): they do, no counts are passed;
 * 0: bertx_mvindex_score_text_colbert and bertx_mvindex_search_texts_colbert pass each
 * query's count to the forward.  One value per context, for all its replicas;
 * BERT_MASK_KEYS=0|1 is read at every load as BERT_POOL is (another value: a load
 * error); a value other than 0 / 1: -1.  The document forms and every other entry
 * ignore it.
 * bertx_test_attention_kv / bertx_test_attention_f32_kv (parity hooks): the hooks
 * without _kv plus keys, host int32[n_seqs] (NULL: the plain hook), with their
 * NaN-filled output, guard rows and return codes; a count outside 1 .. len: -1.
 * bertx_bench_attention_kv: bertx_bench_attention with the one count n_keys for every
 * sentence (1 .. len, else -1).
 * (The ColBERT text forms follow the store's kind: an int8 store takes them unchanged.)
 */
enum { BERTX_OUT_PROJ = 3 };
BERT_API int32_t bertx_convert_hf_colbert(const char *dir_model, const char *fname_out, int32_t ftype);
BERT_API int32_t bertx_proj_dim(struct bert_ctx *ctx);
BERT_API int32_t bertx_proj_width(struct bert_ctx *ctx);
BERT_API int32_t bertx_tokenize_colbert(struct bert_ctx *ctx, const char *text, int32_t kind, int32_t maxlen,
                                        bert_vocab_id *ids, int32_t *keep, int32_t *n_tokens);
BERT_API int32_t bertx_forward_project_device(struct bert_ctx *ctx, int32_t slot, const int32_t *d_ids,
                                              const int32_t *d_types, const int32_t *d_cu, int32_t n_seqs,
                                              int32_t max_len, int32_t total_tokens, const int32_t *d_rows,
                                              int32_t n_rows, float *d_out, void *stream);
BERT_API int32_t bertx_forward_project(struct bert_ctx *ctx, int32_t n, bert_vocab_id **batch_tokens, int32_t *n_tokens,
                                       float **out);
BERT_API int32_t bertx_mvindex_add_texts_colbert(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads,
                                                 int32_t n, const char **texts, int32_t doc_maxlen);
BERT_API int32_t bertx_mvindex_score_text_colbert(struct bertx_mvindex *mv, struct bert_ctx *ctx, const char *query,
                                                  int32_t query_maxlen, const int32_t *ids, int32_t n, float *out);
BERT_API int32_t bertx_mvindex_search_texts_colbert(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads,
                                                    int32_t n, const char **texts, int32_t query_maxlen, int32_t k,
                                                    float *scores, int32_t *ids);
BERT_API int32_t bertx_test_project(int32_t mode, const void *src, const float *stats, const float *g, const float *b,
                                    int32_t T, int32_t d, const float *W, int32_t dim, const int32_t *rows,
                                    int32_t n_out, float *out, int32_t out_rows);
BERT_API int32_t bertx_bench_project(int32_t d, int32_t dim, int32_t T, int32_t iters, float *avg_us);
BERT_API int32_t bertx_forward_device_kv(struct bert_ctx *ctx, int32_t slot, const int32_t *d_ids, const int32_t *d_types,
                                         const int32_t *d_cu, const int32_t *d_keys, int32_t n_seqs, int32_t max_len,
                                         int32_t total_tokens, int32_t out_kind, const int32_t *d_rows, int32_t n_rows,
                                         float *d_out, void *stream);
BERT_API int32_t bertx_forward_tokens_kv(struct bert_ctx *ctx, int32_t n, bert_vocab_id **batch_tokens,
                                         int32_t *n_tokens, const int32_t *n_keys, float **out);
BERT_API int32_t bertx_forward_project_kv(struct bert_ctx *ctx, int32_t n, bert_vocab_id **batch_tokens,
                                          int32_t *n_tokens, const int32_t *n_keys, float **out);
BERT_API int32_t bertx_tokenize_colbert_ex(struct bert_ctx *ctx, const char *text, int32_t kind, int32_t maxlen,
                                           bert_vocab_id *ids, int32_t *keep, int32_t *n_tokens, int32_t *n_keys);
BERT_API int32_t bertx_set_mask_keys(struct bert_ctx *ctx, int32_t on);
BERT_API int32_t bertx_mask_keys(struct bert_ctx *ctx);
BERT_API int32_t bertx_test_attention_kv(const uint16_t *qkv, const int32_t *cu, const int32_t *keys, int32_t n_seqs,
                                         int32_t n_head, int32_t d, int32_t variant, uint16_t *out);
BERT_API int32_t bertx_test_attention_f32_kv(const float *qkv, const int32_t *cu, const int32_t *keys, int32_t n_seqs,
                                             int32_t max_len, int32_t n_head, int32_t d, int32_t era, float *out,
                                             int32_t out_rows);
BERT_API int32_t bertx_bench_attention_kv(int32_t n_seqs, int32_t len, int32_t n_keys, int32_t n_head, int32_t dh,
                                          int32_t variant, int32_t iters, float *avg_us);

BERT_API const char *bertx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BERT_HIP_H */
