// Device-side data layouts and kernel launchers (HIP, gfx950).
//
// HBM layout of one model replica (built by repack.cpp and engine.cpp build_model_image at load):
//   linear weights [N][K] ("lane order", gemm.hip): per K-step (64 k = quant
//            blocks 2ks, 2ks+1) and 32-feature group, 64 lane records; lane
//            l = 16g + f holds the four 16x16x32 A fragments u = 2a + s
//            (feature 32grp + 16a + f, block 2ks + s, elements 8g .. 8g+7):
//              q4_0/q4_1: 16 B (word u, element i at bit 4(i/2) + 16(i%2), so
//                    a mask and an OR with the f16 magic 0x6400 give an f16 pair)
//              q8_0: 32 B (8 B per u, (q ^ 0x80) in order e0 e2 e1 e3 per 4-group)
//              f16:  64 B; f32 files as f16 (hi, lo) pairs along a doubled K
//                    (hi = f16(w), lo = f16(w - hi)), X read twice
//            d (and m) f16 [ks][grp][f][u].  N % 32 == 0, K % 64 == 0.
//   QKV      the three projections are one [3d][d] weight (one GEMM, N = 3d)
//   tables   word/type/pos embeddings in the file's format; q blocks split
//            into an aligned 16/32 B plane + f16 d (+ m) planes.
// Activations (per device workspace, rows = packed tokens of all sentences,
// padded to whole GEMM tiles):
//   Z  [T][d] f16: the residual stream y kept PRE-LayerNorm and scaled by the
//      gamma of the LN that follows it, z = y * gamma ("LN fold", below), with
//      ST [T] (mean, 1/sigma) of y; QKV [T][3d], ATT [T][d], FFN [T][f] f16.
//
// LN fold.  Every consumer of a LayerNorm'd row LN(y) = gamma (y - mean) r + beta
// (r = 1/sigma) reads z = y * gamma and the row's (mean, r):
//   * a projection of it: LN(y) W^T + b = r (z W^T - mean c1) + c2 with the
//     per-feature constants c1 = W gamma, c2 = b + W beta (computed at load), so
//     the GEMM runs on z itself and applies r, mean in its epilogue;
//   * a residual add: LN(y) = r z - r mean gamma + beta, elementwise;
//   * the mean pool: the same expression per token.
// The statistics of a new stream y' come from the residual GEMM that produces
// it: each wave's 32 features of a row give (sum, squared deviations from their
// own mean) in its epilogue, and ln_stats combines them per row (Chan et al.).
// No kernel reads y' to normalise it.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emb {

struct DevWeight {
    int32_t fmt = 0;   // FMT_F16, FMT_Q4_0, FMT_Q4_1, FMT_Q8_0
    int32_t N = 0, K = 0;
    int32_t kx = 0;    // 0: X has K columns; else X has kx = K/2 columns, read twice
                       // (f32 files: [hi | lo] f16 weight rows, repack.cpp repack_linear_f32)
    const void *qs = nullptr;       // values / nibbles / int8, lane order
    const uint16_t *d = nullptr;    // f16 scales
    const uint16_t *m = nullptr;    // f16 mins (q4_1)
};

struct DevTable {
    int32_t fmt = 0;   // FMT_F32, FMT_F16, FMT_Q4_0, FMT_Q4_1, FMT_Q8_0
    int32_t rows = 0, cols = 0;
    const void *qs = nullptr;       // f32/f16 values, or per-block 16 B (q4) / 32 B (q8) planes
    const uint16_t *d = nullptr;    // [rows][cols/32]
    const uint16_t *m = nullptr;
};

enum Epi : int32_t { EPI_BIAS_F16 = 0, EPI_BIAS_GELU_F16 = 1, EPI_BIAS_RES = 2 };

constexpr int GEMM_BM = 256;          // largest token tile: batches of >= GEMM_PAD_BIG tokens pad to it
constexpr int GEMM_PAD_BIG = 4096;
constexpr int GEMM_BM_MIN = 64;       // smaller batches pad to the 64-row tile
inline int gemm_rows(int T) { const int a = T >= GEMM_PAD_BIG ? GEMM_BM : GEMM_BM_MIN; return (T + a - 1) / a * a; }
constexpr int ATT_QT = 128;           // queries per attention workgroup (sentences > ATT_LDS_MAX)
constexpr int ATT_LDS_MAX = 512;      // sentences up to this length: whole K/V of a head in LDS

// LayerNorm bookkeeping of a GEMM epilogue (the LN fold above).
struct LnFold {
    // Input side (EPI_BIAS_F16 / EPI_BIAS_GELU_F16): X holds z of a LayerNorm'd
    // stream with per-row in_stats (mean, r); the result is r (acc - mean c1[n])
    // + bias[n], where the caller passes c2 as `bias`.  Null: plain acc + bias.
    const float2 *in_stats = nullptr;
    const float *c1 = nullptr;
    // Statistics fold (instead of in_stats; small batches): the residual GEMM's
    // partials of the input stream, in_part[g * in_part_stride + row] for its
    // in_G = d / 32 groups, combined by the GEMM itself (ln_stats_kernel's
    // arithmetic); the column-0 tiles store the rows' (mean, 1/sigma) to st_out.
    // Only where gemm_fold_ok says the chosen tile config has the LDS for it.
    const float2 *in_part = nullptr;
    int32_t in_part_stride = 0, in_G = 0;
    float2 *st_out = nullptr;
    // Residual side (EPI_BIAS_RES): `res` holds z of the previous LN (res_stats,
    // gamma res_g, beta res_b), the residual being LN(y) = r z - r mean gamma +
    // beta; res_stats null: the residual as stored.  With g_next the new stream
    // y' = residual + acc + bias is stored as f16(y' * g_next) and per (32-feature
    // group, row) partials (sum y', sum (y' - group mean)^2) go to
    // part[group * part_stride + row]; without it the output is f16(y').
    const float2 *res_stats = nullptr;
    const float *res_g = nullptr, *res_b = nullptr;
    const float *g_next = nullptr;
    float2 *part = nullptr;
    int32_t part_stride = 0;
};

// Y[m][n] = epi( sum_k X[m][k] W[n][k] ), X f16 [M][K] with M % 64 == 0 (tiles of
// 256, 128 or 64 rows: every row of every tile is computed and stored), Y f16 [M][N].
// EPI_BIAS_RES: Y = residual + acc + bias (f32 math), res may alias out (in place,
// element-wise).  Returns 0, or -1 for an unsupported shape.
int launch_gemm(const DevWeight &W, const uint16_t *X, int32_t M, const float *bias, int32_t epi,
                const void *res, void *out, hipStream_t s, const LnFold &ln = LnFold());
// Tests/benches: tile config (0 = heuristic; the shipped configs are listed at
// gemm.hip launch_fmt: 2, 11, 3, 4, 16).  Per calling thread, so a test hook never
// changes a forward running on another thread.  g_gemm_ran: the config the
// calling thread's last launch_gemm actually dispatched (after fallbacks).
extern thread_local int g_gemm_cfg;
extern thread_local int g_gemm_ran;
// Whether launch_gemm of W over M rows can take the statistics fold (LnFold::in_part)
// for G partial groups: the tile config it will choose has the LDS for them.
bool gemm_fold_ok(const DevWeight &W, int32_t M, int32_t G);

// CU count of the calling thread's current HIP device (cached per ordinal).
int device_cu_count();

// z = f16((pos[i] + (type[ty] + word[id])) * gamma) and the (mean, 1/sigma) of
// the f32 sum, for every valid token (bert.cpp:963-984).  types (both embedding
// launchers): int32 [T] token type ids packed as ids, every value 0 or 1 (trusted:
// the table has two rows), ty = types[t]; null: ty = 0, the kernel without the load.
void launch_embed_ln(const DevTable &word, const DevTable &type, const DevTable &pos, const float *ln_w,
                     const int32_t *ids, const int32_t *cu, int32_t n_seqs, int32_t max_len, int32_t d, uint16_t *z,
                     float2 *stats, hipStream_t s, const int32_t *types = nullptr);

// stats[t] = (mean, 1/sqrt(var + 1e-5)) of rows t < rows from the G = d/32 group
// partials part[g * stride + t] a residual GEMM wrote (ggml_norm, bert.cpp:1048-1056).
// Returns -1 (nothing launched) unless d == 32 G with G <= 32.
int launch_ln_stats(const float2 *part, int32_t G, int32_t stride, int32_t rows, int32_t d, float2 *stats,
                     hipStream_t s);

// Benches only: attention kernel variant (bertx_bench_attention).
extern thread_local int g_att_variant;
// The kernel the calling thread's last launch_attention chose (attention.hip AttKernel:
// 0 short, 1 pp, 2 lds3, 3 lds<32>, 4 streaming; -1 before the first launch).
extern thread_local int g_att_ran;

// Per (sentence, head) softmax(Q K^T / sqrt(dh)) V over the sentence's own keys.
// keys (device int32 [n_seqs], or null): sentence b's first keys[b] rows are its
// keys and values, 1 <= keys[b] <= len, every row stays a query (both attention
// launchers).  Null is the plain launch: the same kernels, none reads a count.
// (No default: every caller says whether it has counts.)
void launch_attention(const uint16_t *qkv, const int32_t *cu, int32_t n_seqs, int32_t max_len, int32_t n_head,
                      int32_t d, uint16_t *out, hipStream_t s, const int32_t *keys);

// out[b] = mean_{i<len} LN(y[start+i]) / ||.||  (bert.cpp:1087-1095), from z and
// the row statistics (LN fold).  Two stages: per-64-token-chunk partial sums into
// partial[n_seqs][pool_chunks][d], then sum + normalise.
int32_t pool_chunks(int32_t max_len);
void launch_pool_l2(const uint16_t *z, const float2 *stats, const float *ln_w, const float *ln_b, const int32_t *cu,
                    int32_t n_seqs, int32_t max_len, int32_t d, float *partial, float *out, hipStream_t s);

// [CLS] pooling: out[b] = LN(y[row]) / ||.|| of the sentence's first token, from z
// and the row statistics (the expression of the mean pool, per token).  row =
// cu[b], or b when cu is null (the compact rows of the pruned last layer).
void launch_cls_l2(const uint16_t *z, const float2 *stats, const float *ln_w, const float *ln_b, const int32_t *cu,
                   int32_t n_seqs, int32_t d, float *out, hipStream_t s);
// Per-token output: out[t] = LN(y[t]) as f32 for rows t < T (un-normalised).
void launch_tokens_f32(const uint16_t *z, const float2 *stats, const float *ln_w, const float *ln_b, int32_t T,
                       int32_t d, float *out, hipStream_t s);

// The pruned last layer under [CLS] pooling (attention_cls.hip): per (sentence,
// head) the one query of row cu[b] against the sentence's own keys, f32 scores,
// softmax and P V, f16 into the compact attc [Mc][d] (row b).  With z (else null)
// the same launch gathers the residual of the compact rows, zc[b] = z[cu[b]] and
// stc[b] = st[cu[b]]; rows n_seqs <= row < Mc of attc, zc and stc are written as
// zeros.  dh 32 or 64, any sentence length; returns -1 otherwise.
int launch_attention_cls(const uint16_t *qkv, const int32_t *cu, int32_t n_seqs, int32_t n_head, int32_t d, int32_t Mc,
                         uint16_t *attc, const uint16_t *z, const float2 *st, uint16_t *zc, float2 *stc, hipStream_t s);

// ---- the f32 chain (ftype 0 files, f32.hip): every activation f32 [rows][width] ----
// x = LN(pos + (type + word)) with gamma/beta (bert.cpp:963-984).
void launch_f32_embed_ln(const DevTable &word, const DevTable &type, const DevTable &pos, const float *ln_w,
                         const float *ln_b, const int32_t *ids, const int32_t *cu, int32_t n_seqs, int32_t max_len,
                         int32_t d, float *x, hipStream_t s, bool exact = false, const int32_t *types = nullptr);
// In-place LayerNorm of rows [0, rows) (ggml_norm, f64 sums, eps 1e-5).  exact (both
// LayerNorm launchers; the q8-activation chain): scale, gamma and beta as three
// operations the compiler cannot contract, the reference's roundings bit for bit.
void launch_f32_ln(float *x, int32_t rows, int32_t d, const float *g, const float *b, hipStream_t s,
                   bool exact = false);
// Y[M][N] = epi(X[M][K] W[N][K]^T): 0 bias + acc, 1 era GELU(bias + acc) through the
// f16-indexed table gelu_tab [65536] (host_common.h era_tables, uploaded to the
// device), 2 (bias + acc) + res.  M % 64 == 0, K % 32 == 0; returns -1 otherwise.
int launch_f32_gemm(const float *X, int32_t M, const float *W, int32_t N, int32_t K, const float *bias, int32_t epi,
                    const float *res, float *Y, hipStream_t s, const uint16_t *gelu_tab);
// Per (sentence, head) softmax(Q K^T / sqrt(dh)) V with the era's fp16-table exp
// (exp_tab [65536] on the device), qkv f32 [T][3d] -> out f32 [T][d]; dh 32 or 64
// and the 16 score rows of max_len keys within the device's LDS, else -1.
// era_order (the q8-activation chain): Q K^T and P V summed in ggml_vec_dot_f32's own
// order (eight lanes, rounded multiply and add, pairwise horizontal sum).
int launch_f32_attention(const float *qkv, const int32_t *cu, int32_t n_seqs, int32_t max_len, int32_t n_head,
                         int32_t d, float *out, hipStream_t s, const uint16_t *exp_tab, bool era_order,
                         const int32_t *keys);
// out[b] = mean_{i<len} x[start + i] / ||.|| (bert.cpp:1087-1095); era_order: the token
// sum in ggml_vec_dot_f32's order.
void launch_f32_pool(const float *x, const int32_t *cu, int32_t n_seqs, int32_t d, float *out, hipStream_t s,
                     bool era_order = false);
// [CLS] pooling of the f32 / q8 chains: out[b] = x[cu[b]] / ||.|| (x holds the final LayerNorm output).
void launch_f32_cls(const float *x, const int32_t *cu, int32_t n_seqs, int32_t d, float *out, hipStream_t s);

// ---- the q8-activation chain (q4_0 / q4_1 / q8_0 files in activation mode 1, q8act.hip):
// the f32 chain's kernels around projections in the reference's block arithmetic ----
// ggml's activation quantizer (era_quantize_row_q8_0 / _q8_1): X f32 [>= T][K] ->
// q int8 [M][K], d f32 [K/32][M] (kind 0, q8_0: the f16-rounded scale as f32; kind 1,
// q8_1: the f32 scale) and, kind 1, s f32 [K/32][M] = (float)(sum q) * d.  Rows
// T <= row < M (tile padding) are quantized as zeros and never read.  M % 64 == 0,
// K % 32 == 0; returns -1 otherwise.
int launch_q8_quantize(const float *X, int32_t T, int32_t M, int32_t K, int32_t kind, int8_t *q, float *d, float *s,
                       hipStream_t st);
// Y f32 [M][N] = epi(sum over blocks b, ascending, of (wd xd) (float)sumi [+ wm xs]) with
// the exact integer block dot sumi on the i8 matrix cores; W in the lane-order layout
// above (q4_0 / q4_1 / q8_0), xq / xd / xs as launch_q8_quantize wrote them for the
// same M (q8_1 for q4_1 weights, else q8_0).  epi as launch_f32_gemm.  Returns -1 for
// an unsupported format or shape.
int launch_q8_gemm(const DevWeight &W, const int8_t *xq, const float *xd, const float *xs, int32_t M,
                   const float *bias, int32_t epi, const float *res, float *Y, hipStream_t s,
                   const uint16_t *gelu_tab);

// ---- the embedding index (search.hip, index.cpp): rows in fragment order, groups of
// 16 rows, a group's blocks of 1 KiB consecutive.  SEARCH_F16: a block = 16 rows x 32 k,
// lane 16g + f = row f, elements 8g .. 8g + 7.  SEARCH_I8: a block = 16 rows x 64 k,
// lane 16g + f = row f, bytes 16g .. 16g + 15, and a second buffer of one f32 scale per
// row (the arithmetic: bert_hip.h, search.hip quantize_row_i8 / score_i8) ----
enum { SEARCH_F16 = 0, SEARCH_I8 = 1 };   // = BERTX_INDEX_F16 / _I8
// The row masks of a masked search (index_mask.hip; bert_hip.h "Deleting rows and filtered
// search"): 32 rows to a uint32_t word, row r = bit r % 32 of word r / 32.  A row is offered
// iff it is < n_rows, its bit in tomb is 0 and its bit in the query's filter is 1.
struct SearchMask {
    const uint32_t *tomb;    // the index's tombstones, index_mask_words(capacity) words
    const uint32_t *filt;    // null: no filter; else at least ceil(n_rows / 32) words per filter
    int64_t stride;          // words from one query's filter to the next; 0: one filter for all
};
// (the masked kernels take the mask as a template parameter pack of none or one)
constexpr const SearchMask &first_mask(const SearchMask &m) { return m; }
constexpr const uint32_t *first_tomb(const uint32_t *t) { return t; }
// The mask of the pass of a token-store scan that starts at query q0 of the call: its own
// filters (a shared filter has stride 0).
inline SearchMask pass_mask(SearchMask m, int64_t q0)
{
    if (m.filt) m.filt += q0 * m.stride;
    return m;
}
// Once per process and device (the calling thread's current one) before the first
// launch_search: lets the search kernels use the CU's whole LDS.  Returns 0 or -1.
int search_prepare_device();
// Queries one search launch takes at width d and list length k (16, 32, 48 or 64:
// what the queries' fragments, the lists and the score tile leave room for in LDS;
// always 64 for SEARCH_I8, whose queries take d + 4 bytes).
int search_group_queries(int d, int k, int storage);
// The most workgroups a search over an index of this capacity uses (current device);
// the scratch of launch_search holds 64 * that * 128 (score, id) pairs of 8 B.
int64_t search_max_workgroups(int64_t capacity_rows);
// Converts rows f32 [n][d] (device) into rows first .. first + n - 1 of the index image:
// to f16, round to nearest even, or to int8 with the rows' scales into scales[first ..].
// d % 64 == 0, 64 <= d <= 1024; returns -1 otherwise.
int launch_index_add(const float *d_rows, int64_t n, int d, int64_t first, int storage, void *corpus, float *scales,
                     hipStream_t s);
// scores f32 [B][k], ids i32 [B][k]: per query the k highest scores over rows < n_rows
// (f16: the dot product of the f16-rounded query with the row; int8: the query quantized
// as the rows are, score_i8), descending, equal scores by ascending id, (-inf, -1) where
// the index has fewer than k rows.  One streaming kernel and one merge kernel per group
// of search_group_queries queries.  scales: the int8 rows' scales (not read for f16).
// 1 <= k <= 128, B >= 1; returns -1 for bad arguments (nothing launched), -3 when a
// launch was refused.
// mask (may be null): the masked kernels, which offer a row only when it is admissible as
// well; null launches the unmasked instantiations with the arguments above and nothing else.
int launch_search(const void *corpus, const float *scales, int storage, int64_t n_rows, int d, const float *d_queries,
                  int B, int k, void *scratch, float *d_scores, int32_t *d_ids, hipStream_t s,
                  const SearchMask *mask = nullptr);
// The second half of launch_search on its own, for the other scans that keep lists in its
// layout: partial (score, id) pairs of 8 B, [nq][P][k], every list in the order of the
// results with (-inf, -1) fill -> d_scores / d_ids [nq][k].  One workgroup per query.
int launch_search_merge(const void *partial, int nq, int P, int k, float *d_scores, int32_t *d_ids, hipStream_t s);
// Benches: out f32 [n][d] (device) = unit rows of hashed values.
int launch_unit_rows(float *d_out, int64_t n, int d, uint32_t seed, hipStream_t s);

// ---- binary storage of the embedding index (search_bin.hip; the layout, the binarizer
// and the score: bin_bits.h; the contract: bert_hip.h "Binary storage") ----
enum { SEARCH_BIN = 8 };   // = BERTX_INDEX_BIN
// Once per process and device before the first launch_search_bin (the LDS attribute).
int search_bin_prepare_device();
// Bytes of the image of an index of this capacity: ceil(capacity / 64) groups of
// ceil(d / 128) KiB.
size_t search_bin_image_bytes(int64_t capacity_rows, int d);
// The most workgroups a scan over an index of this capacity uses (current device); the
// scratch of launch_search_bin holds 64 * that * 128 (score, id) pairs of 8 B.
int64_t search_bin_max_workgroups(int64_t capacity_rows);
// rows f32 [n][d] (device) -> the sign bits of rows first .. first + n - 1 of the image.
int launch_index_add_bin(const float *d_rows, int64_t n, int d, int64_t first, void *corpus, hipStream_t s);
// launch_search over a binary image: the score is d - 2 popcount(bits_q xor bits_row).
// One scan kernel and the merge (launch_search_merge) per 64 queries.
int launch_search_bin(const void *corpus, int64_t n_rows, int d, const float *d_queries, int B, int k, void *scratch,
                      float *d_scores, int32_t *d_ids, hipStream_t s, const SearchMask *mask = nullptr);

// ---- scores of listed rows of the embedding index (search_rescore.hip), all three kinds ----
// d_scores [B][n] = the score of (query b, row d_ids[b][n]) with the bits launch_search /
// launch_search_bin give that pair, -inf for an id outside [0, n_rows).  d_ids_out (may be
// null) [B][n]: the id, or -1 where the score is -inf for that reason.  1 <= n <= 128,
// B >= 1; -1 otherwise (nothing launched), -3: launch refused.
// tomb (may be null): the index's tombstones; a row whose bit is 1 scores as an id outside
// [0, n_rows) does.  null launches the unmasked instantiation.
int launch_index_score_ids(const void *corpus, const float *scales, int storage, int64_t n_rows, int d,
                           const float *d_queries, int B, const int32_t *d_ids, int n, float *d_scores,
                           int32_t *d_ids_out, hipStream_t s, const uint32_t *tomb = nullptr);

// ---- the tombstones of the embedding index (index_mask.hip) ----
// Words of an index's tombstones: whole 64-row pairs over the capacity (the binary scan reads
// a pair per group).
int64_t index_mask_words(int64_t capacity_rows);
// Sets the tombstones of d_ids int32 [n] (device); ids outside [0, n_rows) are ignored.
int launch_index_remove(const int32_t *d_ids, int n, int64_t n_rows, uint32_t *tomb, hipStream_t s);
// *d_count = the tombstones set among rows [0, n_rows) (a memset and one kernel).
int launch_index_count_deleted(const uint32_t *tomb, int64_t n_rows, int32_t *d_count, hipStream_t s);
// d_out uint8 [n] = the tombstones of rows first .. first + n - 1, 0 or 1.
int launch_index_deleted_flags(const uint32_t *tomb, int64_t first, int n, uint8_t *d_out, hipStream_t s);

// ---- the token store of late interaction (maxsim.hip, mvindex.cpp): documents of len
// token rows in the SEARCH_F16 fragment order, every document on a group boundary, and
// a device table of int32 pairs (first group, len) per document (the arithmetic:
// bert_hip.h, maxsim.hip pack_row_f16) ----
// Once per process and device before the first launch_maxsim (the LDS attribute).
int maxsim_prepare_device();
// Source rows t0 .. t0 + count - 1 of one add call, d_rows = row t0, f32 [count][w], each
// normalised to unit length, rounded to f16 and written to its slot.  d_src_off int32
// [n_new]: the first source row of the call's i-th document (ascending from 0);
// d_table: the (first group, len) pairs of those n_new documents.  -1: bad arguments.
int launch_mv_pack(const float *d_rows, int64_t t0, int64_t count, int w, const int32_t *d_src_off,
                   const void *d_table, int n_new, void *store, hipStream_t s);
// d_out[c] = sum_{i < Lq} max_{j < len} sim(q_i, row j of document id), id = d_ids[c] (or c
// when d_ids is null), for c < n; -inf for an id outside [0, n_docs).  d_q f32 [Lq][w]
// is normalised as the rows are.  1 <= Lq <= 64, n >= 1; -1 otherwise, -3: launch refused.
// tomb (here and on the other two scorers; may be null): the store's tombstones, one bit per
// document as index_mask.hip packs them; a document whose bit is 1 scores -inf as an id outside
// [0, n_docs) does.  null launches the unmasked instantiation with the arguments above.
// max_wg, ran_wg (here and on every scan of the store below; bert_hip.h bertx_test_mvindex_grid):
// max_wg > 0 bounds the scan kernel's workgroups after the launcher's own rule and before
// anything derived from them; *ran_wg, when given, receives the workgroups it launched.
int launch_maxsim(const void *store, const void *d_table, int n_docs, int w, const float *d_q, int Lq,
                  const int32_t *d_ids, int n, float *d_out, hipStream_t s, int max_wg = 0, int *ran_wg = nullptr,
                  const uint32_t *tomb = nullptr);
// The same two over an int8 store (maxsim_i8.hip): rows in the SEARCH_I8 fragment order,
// each the embedding index's int8 quantization q of the raw row, and scales f32 [token
// slots], u = 1 / sqrt(sum q_i^2) per slot (0 for a zero row), so that q u has unit
// length; sim = score_i8(isum, u_query, u_row).  maxsim_prepare_device covers both kinds.
int maxsim_i8_prepare_device();
int launch_mv_pack_i8(const float *d_rows, int64_t t0, int64_t count, int w, const int32_t *d_src_off,
                      const void *d_table, int n_new, void *store, float *scales, hipStream_t s);
int launch_maxsim_i8(const void *store, const float *scales, const void *d_table, int n_docs, int w, const float *d_q,
                     int Lq, const int32_t *d_ids, int n, float *d_out, hipStream_t s, int max_wg = 0,
                     int *ran_wg = nullptr, const uint32_t *tomb = nullptr);
// The full scan (maxsim_search.hip): d_scores f32 [B][k], d_ids i32 [B][k] = per query the
// k best documents of all n_docs by the scorers' score, bit for bit, best first, equal
// scores by ascending id, (-inf, -1) where the store has fewer than k documents.  d_q f32
// [B][Lq][w]: B queries of exactly Lq rows (an all-zero row adds +0, as a query index
// >= Lq does).  used_groups: the store's used token slots / 16; the documents lie
// contiguous from group 0 in id order.  floor(4 / ceil(Lq / 16)) queries share one pass
// over the store; per pass one streaming kernel and one or two selection kernels.  scratch:
// maxsim_search_scratch_bytes() (sized by the current device's CU count and k = 128).
// 1 <= Lq <= 64, 1 <= k <= 128, B >= 1; -1 otherwise (nothing launched), -3: launch refused.
// mask (here and on launch_maxsim_candidates; may be null): a SearchMask over documents, tomb
// the store's tombstones and filt the call's filters, one for all (stride 0) or one per query
// of d_q; the masked kernels list a document for a query only when it is admissible (bert_hip.h
// "Deleting documents and filtered search").  null launches the unmasked instantiations with
// the arguments above and nothing else.
int maxsim_search_prepare_device();
size_t maxsim_search_scratch_bytes();
int launch_maxsim_search(const void *store, const float *scales, int storage, const void *d_table, int n_docs,
                         int64_t used_groups, int w, const float *d_q, int B, int Lq, int k, void *scratch,
                         float *d_scores, int32_t *d_ids, hipStream_t s, int max_wg = 0, int *ran_wg = nullptr,
                         const SearchMask *mask = nullptr);

// ---- centroid codes of the token store (maxsim_codes.hip; bert_hip.h "Centroid codes") ----
// The centroids are C rows (a multiple of 16) packed as one document of C tokens from group
// 0 of their own buffer (launch_mv_pack / launch_mv_pack_i8), cent_u their f32 (int8).
// codes uint16 [token slots]: for every slot of groups g0 .. g1 - 1 of the store the index of
// the centroid of highest sim to the slot's row, the row re-packed from its stored values in
// the query role, equal sims to the lower index.  Then the slots of documents d0 .. d1 - 1
// past their len are set to 0.  Once per device: maxsim_codes_prepare_device.
int maxsim_codes_prepare_device();
int launch_mv_assign(const void *store, const float *scales, int storage, const void *d_table, int64_t g0, int64_t g1,
                     int d0, int d1, int w, const void *cent, const float *cent_u, int C, uint16_t *codes,
                     hipStream_t s);

// ---- centroid interaction (maxsim_approx.hip; bert_hip.h "Pruned search") ----
// One pass of nq queries of ceil(Lq / 16) tiles each (at most four tiles), d_q f32
// [nq][Lq][w]: the table T f32 [C][16 tiles] = sim(query row, centroid) into tscratch
// (256 C bytes), the scan of every document's codes and the selection: d_approx / d_ids
// [nq][n_cand] by `better` with (-inf, -1) fill.  scratch: the search's.  *form: 1 the
// table went to LDS, 2 it stayed in global memory.  stages: 1 the table kernel, 2 the scan and
// the selection, 3 both (the benches time them apart).  -1: bad arguments, -3: launch refused.
int maxsim_approx_prepare_device();
int launch_maxsim_candidates(const uint16_t *codes, const void *d_table, int n_docs, int64_t used_groups, int storage,
                             int w, const void *cent, const float *cent_u, int C, const float *d_q, int nq, int Lq,
                             int n_cand, float *tscratch, void *scratch, float *d_approx, int32_t *d_ids, int stages,
                             int *form, hipStream_t s, int max_wg = 0, int *ran_wg = nullptr,
                             const SearchMask *mask = nullptr);
// out_s / out_i [nq][k] = the k best by `better` of each query's n_cand (exact[j], ids[j])
// pairs; a pair whose id is -1 counts as the fill.
int launch_maxsim_rerank_select(const float *exact, const int32_t *ids, int nq, int n_cand, int k, float *out_s,
                                int32_t *out_i, hipStream_t s);

// ---- residual-coded token storage (maxsim_res.hip; bert_hip.h "Residual codes") ----
// A slot keeps its code, nbits = 2 or 4 bits per element (the layout: maxsim_res.hip) and
// one f32 u.  An add packs its rows into a staging image in the f16 store layout whose
// table is the call's entries counted from the call's first group (launch_res_rel_table:
// d_rel[i] = (d_table_new[i].first - g0, len)), codes it with launch_mv_assign, and encodes:
// bits and u of `groups` groups from the staging image, their codes, the f16 centroid image,
// cuts f32 [2^nbits - 1] and wts f16 [2^nbits] on the device.  bits, u and codes point at the
// call's first group.  launch_maxsim_res is launch_maxsim over such a store: pair uint32
// [2^(2 nbits)] on the device, pair[b0 | b1 << nbits] = wts[b0] | wts[b1] << 16.
int maxsim_res_prepare_device();
int launch_res_rel_table(const void *d_table_new, int n_new, int64_t g0, void *d_rel, hipStream_t s);
int launch_res_encode(const void *staging, int64_t groups, int w, int nbits, const uint16_t *codes, const void *cent,
                      const float *cuts, const uint16_t *wts, uint32_t *bits, float *u, hipStream_t s);
int launch_maxsim_res(const uint32_t *bits, const float *u, const uint16_t *codes, const void *cent, const uint32_t *pair,
                      int nbits, const void *d_table, int n_docs, int w, const float *d_q, int Lq, const int32_t *d_ids, int n,
                      float *d_out, hipStream_t s, int max_wg = 0, int *ran_wg = nullptr, const uint32_t *tomb = nullptr);

// ---- the classification head (head.hip): pooler dense + tanh + classifier on the
// sentences' [CLS] rows, all f32, one form for the three chains ----
constexpr int HEAD_MAX_LABELS = 16;
// x f32 [n_seqs][d] = the final-LayerNorm row of each sentence's first token, not
// normalised.  f16 chain: LN(y[row]) by the LN-fold expression of launch_cls_l2 /
// launch_tokens_f32 from z and the row statistics, row = cu[b], or b when cu is null
// (the compact rows of the pruned last layer).  f32 / q8 chains: row cu[b] of x32.
void launch_head_gather(const uint16_t *z, const float2 *stats, const float *ln_w, const float *ln_b, const int32_t *cu,
                        int32_t n_seqs, int32_t d, float *x, hipStream_t s);
void launch_head_gather_f32(const float *x32, const int32_t *cu, int32_t n_seqs, int32_t d, float *x, hipStream_t s);
// logits f32 [n_seqs][n_labels] = wc tanh(x wp^T + bp) + bc: wp f32 [d][d] (rows =
// output features), wc f32 [n_labels][d]; p f32 [n_seqs][d] receives the pooler
// output.  Two launches: the pooler GEMM on v_mfma_f32_16x16x4_f32 over (16 feature,
// 16 sentence) tiles (wp is read once per 16 sentences), then one wave per sentence
// for the classifier.  Every sum runs in an order fixed by d alone, so a sentence's
// logits do not depend on n_seqs, its row or the other rows, bit for bit.
// d % 64 == 0, d <= 1024, 1 <= n_labels <= HEAD_MAX_LABELS; returns -1 otherwise.
int launch_head(const float *x, int32_t n_seqs, int32_t d, const float *wp, const float *bp, const float *wc,
                const float *bc, int32_t n_labels, float *p, float *logits, hipStream_t s);

// ---- the ColBERT projector (project.hip; the arithmetic: bert_hip.h "Projection") ----
// out f32 [n_out][width], width = 64 ceil(dim / 64): output row i = the unit-length
// projection of source row d_rows[i] (d_rows int32 [n_out] on the device; null: row i),
// columns dim .. width - 1 exactly +0.  The source is the final-LayerNorm row, rounded
// to f16 in registers: either z f16 [>= rows][d] with stats / ln_w / ln_b (the f16
// chain's stream, the expression of launch_tokens_f32) or x32 f32 [rows][d] (the f32 /
// q8 chains' final buffer); exactly one of z, x32 is non-null.  wimg: the weight as
// build_proj_image (engine.h) lays it out.  Only mapped rows are read, only n_out rows
// are stored.  d % 64 == 0, 64 <= d <= 1024, dim % 32 == 0, 32 <= dim <= 256, n_out >= 1;
// returns -1 otherwise (nothing launched), -3 when the launch was refused.
int launch_project(const uint16_t *z, const float2 *stats, const float *ln_w, const float *ln_b, const float *x32,
                   int32_t d, const void *wimg, int32_t dim, const int32_t *d_rows, int32_t n_out, float *out,
                   hipStream_t s);

// Diagnostics: *cnt += number of non-finite values in p[0..n) (f32, or f16 if f16).
void launch_count_nonfinite(const void *p, size_t n, int f16, unsigned *cnt, hipStream_t s);

}  // namespace emb
