// Per-GPU engine: one weight replica, one workspace, one stream, one mutex.
// The forward is the reference's bert_forward_batch graph (bert.cpp:876-1097)
// as a fixed sequence of HIP launches over a packed (un-padded) token batch.
#pragma once

#include "host_common.h"
#include "kernels.h"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

struct bertx_index;
struct bertx_mvindex;

namespace emb {

enum KClass : int32_t {
    K_EMBED_LN = 0, K_GEMM_QKV, K_ATTENTION, K_GEMM_O, K_LN_STATS, K_GEMM_FFN_UP, K_GEMM_FFN_DOWN, K_POOL_L2,
    K_NUM_CLASSES
};
const char *kclass_name(int k);

struct KStats {
    int64_t launches = 0;
    double ms = 0.0;
    double work = 0.0;     // FLOP (GEMM/attention) or bytes (memory-bound classes)
};

struct DevLayer {
    DevWeight qkv, o, up, down;
    float *b_o = nullptr, *b_down = nullptr;
    // LN fold (kernels.h) of the projections that read a LayerNorm'd stream:
    // c1 = W gamma, c2 = b + W beta of the LN in front (QKV: the previous layer's
    // output LN or the embedding LN; FFN-up: this layer's attention-output LN)
    float *c1_qkv = nullptr, *c2_qkv = nullptr, *c1_up = nullptr, *c2_up = nullptr;
    float *ln1_w = nullptr, *ln1_b = nullptr, *ln2_w = nullptr, *ln2_b = nullptr;
    // f32 files (the f32 chain, f32.hip): weights as the file rows [N][K] f32, QKV
    // fused [3d][d] with its bias [3d]; the q8-activation chain uses the two biases
    // with the lane-order weights above
    const float *w32_qkv = nullptr, *w32_o = nullptr, *w32_up = nullptr, *w32_down = nullptr;
    const float *b_qkv = nullptr, *b_up = nullptr;
};

// Sets the calling thread's current HIP device for a scope and restores the
// previous one on exit (library calls must not move a host application's device).
class DeviceGuard {
public:
    explicit DeviceGuard(int ordinal)
    {
        if (hipGetDevice(&prev_) != hipSuccess) { (void)hipGetLastError(); prev_ = -1; }
        st_ = prev_ == ordinal ? hipSuccess : hipSetDevice(ordinal);
        if (prev_ == ordinal) prev_ = -1;
    }
    ~DeviceGuard() { if (prev_ >= 0) (void)hipSetDevice(prev_); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
    bool ok() const { return st_ == hipSuccess; }
    hipError_t status() const { return st_; }

private:
    int prev_ = -1;
    hipError_t st_ = hipSuccess;
};

// A model's device image: every weight plane in its device layout (lane-order
// linear weights, LN-fold constants, embedding-table planes, the f32 chain's
// rows and tables), laid out at 256-B aligned offsets of one arena.  Built once
// on the host by build_model_image and uploaded to every replica, so N replicas
// cost one repack (reference: one read of the tensors, bert.cpp:650-766).
struct ModelImage {
    static constexpr size_t kNone = ~(size_t)0;
    struct Tab { size_t q = kNone, d = kNone, m = kNone; int fmt = 0, rows = 0, cols = 0; };
    struct Lin { size_t q = kNone, d = kNone, m = kNone; int N = 0, K = 0; };
    struct Layer {
        Lin qkv, o, up, down;
        size_t bo = kNone, bdown = kNone, c1q = kNone, c2q = kNone, c1u = kNone, c2u = kNone;
        size_t l1w = kNone, l1b = kNone, l2w = kNone, l2b = kNone;
        size_t w32q = kNone, w32o = kNone, w32u = kNone, w32d = kNone, bq = kNone, bu = kNone;
    };
    HParams hp;
    int wfmt = FMT_F16;
    bool f32 = false;
    bool q8 = false;   // activation mode 1 on a q4_0 / q4_1 / q8_0 file: the q8-activation chain (q8act.hip)
    Tab word, type, pos;
    size_t gelu = kNone, exp = kNone, lnw = kNone, lnb = kNone;
    // the classification head (files that carry one): the pooler rows dequantized to
    // f32 [d][d], its bias, the classifier rows f32 [n_labels][d] and bias
    size_t head_wp = kNone, head_bp = kNone, head_wc = kNone, head_bc = kNone;
    int n_labels = 0;
    // the ColBERT projection (files that carry one): build_proj_image of the dequantized rows
    size_t proj = kNone;
    int proj_dim = 0;
    std::vector<Layer> layers;
    // piece i: bytes [off[i], off[i] + len[i]) of the image (len 0: absent plane)
    std::vector<size_t> off, len;
    size_t total = 0;
    const uint8_t *bytes() const { return pinned_ ? pinned_ : host_.data(); }
    bool pinned() const { return pinned_ != nullptr; }

    ModelImage() = default;
    ~ModelImage();
    ModelImage(const ModelImage &) = delete;
    ModelImage &operator=(const ModelImage &) = delete;

private:
    friend bool build_model_image(const HostModel &m, ModelImage &img, std::string &err, bool pin, int act_mode);
    std::vector<uint8_t> host_;       // pageable image (when pinning failed or no device)
    uint8_t *pinned_ = nullptr;       // page-locked image (hipHostMalloc): async uploads
};

// Host work of a load, once per context: checks the shape, repacks every plane
// and concatenates them into the image (page-locked when `pin`).  False with a
// message in err; never throws (a bad_alloc becomes false).  act_mode 1 (the
// reference's q8 activations, quantized files only: act_mode_effective): the
// image carries the raw QKV / FFN-up biases and the era tables, as for f32 files,
// and no LN-fold constants.
bool build_model_image(const HostModel &m, ModelImage &img, std::string &err, bool pin, int act_mode = 0);
// The projector's weight image (project.hip, kernels.h launch_project): W f32 [dim][d]
// rounded to f16, nearest even, zero-padded to width = 64 ceil(dim / 64) rows, in the
// SEARCH_F16 block order: block (kb, t) of 16 features x 32 k at (kb * width / 16 + t)
// KiB, lane 16g + f = feature 16t + f, elements 32kb + 8g .. + 7.
void build_proj_image(const float *W, int dim, int d, std::vector<uint8_t> &bytes);
// The activation mode a file of format `ftype` runs when `act_mode` is asked for:
// 1 only for q4_0 / q4_1 / q8_0 (f16 and f32 files have no q8 arithmetic in the reference).
inline int act_mode_effective(int ftype, int act_mode)
{
    return act_mode == 1 && (ftype == FMT_Q4_0 || ftype == FMT_Q4_1 || ftype == FMT_Q8_0) ? 1 : 0;
}

class Device {
public:
    // Creates the replica's stream and completion event, allocates the weight
    // arena and issues the image upload on the replica's stream (async from a
    // page-locked image).  Call finish_load() before the first use.  All HIP calls
    // of a load are made by the loading thread (bert_load_from_file).
    Device(int ordinal, const ModelImage &img);
    ~Device();
    bool finish_load();   // waits for the upload; ok() from then on
    bool ok() const { return ok_; }
    int ordinal() const { return ordinal_; }
    hipStream_t stream() const { return stream_; }
    std::mutex &mutex() { return mu_; }

    // Grow the workspace so one forward of `tokens` packed tokens / `seqs`
    // sentences of at most `max_len` tokens fits (never called inside a timed
    // forward).  Waits for the replica's last forward, on whatever stream it ran.
    bool reserve(int64_t tokens, int64_t seqs, int max_len);

    // Device-resident forward (ids, cu, out on this GPU); async on `s`.  When
    // profiling is off and `s` is not the null stream, the launch sequence is
    // captured once per (pointers, shape, stream) into a HIP graph and replayed.
    // The workspace is shared by every forward of the replica: a forward on a
    // stream other than the previous forward's first waits (on the device) for
    // that forward's completion event, so calls on different streams never
    // overlap in the workspace.
    // len2_sum: sum of the squared sentence lengths when the caller knows them
    // (attention FLOP of the per-kernel stats), else -1.
    // tokens: d_out is float[total_tokens][n_embd] and receives every token's final
    // LayerNorm output (un-normalised) instead of the pooled sentence embeddings.
    int forward(const int32_t *d_ids, const int32_t *d_cu, int n_seqs, int max_len, int total_tokens, float *d_out,
                hipStream_t s, double len2_sum = -1.0, bool tokens = false)
    {
        return forward_ex(d_ids, nullptr, d_cu, n_seqs, max_len, total_tokens, tokens ? KIND_TOKENS : KIND_POOLED, d_out,
                          s, len2_sum);
    }
    // The same with token types and the kind of output (bert_hip.h BERTX_OUT_*).
    // d_types: int32[total_tokens] on this GPU, every value 0 or 1 (trusted), or null
    // for all 0.  KIND_LOGITS: d_out is float[n_seqs][n_labels], the raw logits of the
    // file's classification head on each sentence's [CLS] row; -6 without a head.  The
    // f16 chain runs the last layer on the compact rows when CLS pruning is on.
    // KIND_PROJ: d_out is float[n_rows][proj_width], row i the unit-length ColBERT
    // projection of token d_rows[i] (d_rows int32 [n_rows] on this GPU, every value in
    // [0, total_tokens), trusted), or with d_rows null float[total_tokens][proj_width],
    // every token in order; -6 on a file without the record.  Never pruned.
    // d_keys (KIND_TOKENS and KIND_PROJ only, -1 with another kind; null: none): int32
    // [n_seqs] on this GPU, sentence b's first d_keys[b] rows are the keys and values of
    // its attention, 1 <= d_keys[b] <= its length (trusted); every row stays a query and
    // an output row.  Those kinds never run the pruned last layer.
    enum OutKind : int { KIND_POOLED = 0, KIND_TOKENS = 1, KIND_LOGITS = 2, KIND_PROJ = 3 };
    int forward_ex(const int32_t *d_ids, const int32_t *d_types, const int32_t *d_cu, int n_seqs, int max_len,
                   int total_tokens, int out_kind, float *d_out, hipStream_t s, double len2_sum = -1.0,
                   const int32_t *d_rows = nullptr, int n_rows = 0, const int32_t *d_keys = nullptr);
    int n_labels() const { return n_labels_; }
    int proj_dim() const { return proj_dim_; }
    int proj_width() const { return proj_width_of(proj_dim_); }

    // Host-driven forward: packs tokens, H2D, forward, D2H, synchronous.
    // tokens[i] has lens[i] ids; out[i] receives n_embd floats, or with tok_out
    // lens[i] x n_embd floats (the per-token output).  types (or null: all 0): the
    // token type ids, types[i] beside tokens[i].  logits: out[i] receives the
    // n_labels logits of sentence i instead.  proj (with tok_out): out[i] receives
    // lens[i] x proj_width floats, the projected rows (KIND_PROJ).  keys (with tok_out;
    // null: none): keys[i] is sentence i's key count, 1 .. lens[i] (checked by the caller).
    int forward_host(const int32_t *const *tokens, const int32_t *lens, int n, float *const *out, bool tok_out = false,
                     const int32_t *const *types = nullptr, bool logits = false, bool proj = false,
                     const int32_t *keys = nullptr);

    // Pooling of the sentence embeddings (bert_hip.h): BERTX_POOL_MEAN / BERTX_POOL_CLS,
    // and whether CLS pooling runs the last layer on the sentences' first rows only
    // (f16 chain).  Both are part of a captured graph's key.  Call under mutex().
    void set_pooling(int pool) { pool_ = pool; }
    void set_cls_pruning(bool on) { prune_ = on; }

    // profiling
    void set_profiling(bool on) { profiling_ = on; }
    void collect_stats();
    void reset_stats();
    const KStats &stats(int k) const { return stats_[k]; }

    const HParams &hp() const { return hp_; }

    // the last bert_forward_batch / bert_encode_batch call that ran on this replica
    // (bertx_device_last_call): host wall time of its forwards, sentences, tokens;
    // calls() counts the host-driven calls that ran here (bertx_device_calls)
    void set_last_call(double ms, int seqs, int64_t tokens)
    {
        lc_ms_ = ms; lc_seqs_ = seqs; lc_tokens_ = tokens; ++calls_;
    }
    int64_t calls() const { return calls_; }
    double last_call_ms() const { return lc_ms_; }
    int last_call_seqs() const { return lc_seqs_; }
    int64_t last_call_tokens() const { return lc_tokens_; }

private:
    struct PendingEv { int cls; hipEvent_t a, b; double work; };
    struct GraphKey {
        const void *ids, *cu, *out;
        hipStream_t s;
        int n_seqs, max_len, T;
        int mode;   // OutMode: a graph of one pooling mode is never replayed for another
        const void *types;   // the token types pointer (null: all 0) is baked into the embedding launch
        const void *rows;    // OUT_PROJ: the row map (null: every token) and its length
        int n_rows;
        const void *keys;    // the key counts pointer (null: none) is baked into the attention launches
        bool operator==(const GraphKey &o) const
        {
            return ids == o.ids && cu == o.cu && out == o.out && s == o.s && n_seqs == o.n_seqs &&
                   max_len == o.max_len && T == o.T && mode == o.mode && types == o.types && rows == o.rows &&
                   n_rows == o.n_rows && keys == o.keys;
        }
    };
    // what the launch sequence ends in (and, for CLS and the logits, how its last layer runs)
    enum OutMode : int { OUT_MEAN = 0, OUT_CLS, OUT_CLS_PRUNED, OUT_TOKENS, OUT_LOGITS, OUT_LOGITS_PRUNED, OUT_PROJ };
    bool pruned_last() const { return out_mode_ == OUT_CLS_PRUNED || out_mode_ == OUT_LOGITS_PRUNED; }
    struct GraphEntry { GraphKey key; hipGraphExec_t exec; };
    int forward_ordered(const int32_t *d_ids, const int32_t *d_cu, int n_seqs, int max_len, int T, float *d_out,
                        hipStream_t s);
    void order_after_last(hipStream_t s);   // stream s waits for the last forward (any stream)
    void mark_done(hipStream_t s);          // records the completion event of a forward on s
    // The launch schedules (forward.cpp): launch_all runs the replica's chain through
    // a Launcher (timed launches, the optional finite check, the closing error report).
    struct Launcher;
    // The rows a layer tail of the f16 chain runs on: all the packed tokens, or the
    // compact rows (one per sentence) of the pruned last layer under CLS pooling.
    struct RowSet {
        int M;                      // GEMM rows (whole tiles)
        double flop_rows;           // rows that count as work
        size_t valid;               // rows the finite check reads
        uint16_t *z;
        float2 *st, *part;
        int32_t part_stride;
        uint16_t *att, *ffn;
        bool fold;                  // the statistics fold applies (gemm_fold_ok on these rows)
        bool last;                  // the last layer: its statistics feed the output stage
        const char *tag;            // suffix of the kernel names in the finite check
        LnFold input(bool fold_in, int G, const float *c1) const;
    };
    int launch_all(const int32_t *d_ids, const int32_t *d_cu, int n_seqs, int max_len, int T, float *d_out,
                   hipStream_t s, bool check);
    int chain_f16(Launcher &run, const int32_t *d_ids, const int32_t *d_cu, int n_seqs, int max_len, int T, float *d_out);
    int layer_tail(Launcher &run, const DevLayer &L, int l, const RowSet &r, const float *&gz, const float *&bz);
    int head(Launcher &run, int n_seqs, float *d_out);
    int chain_32(Launcher &run, const int32_t *d_ids, const int32_t *d_cu, int n_seqs, int max_len, int T, float *d_out);
    void drop_graphs();
    void bind(const ModelImage &img);   // device pointers of the image's planes
    bool uploading_ = false;
    void begin(int cls, hipStream_t s, hipEvent_t &a);
    void end(int cls, hipStream_t s, hipEvent_t a, double work);
    hipEvent_t get_event();

    bool ok_ = false;
    int ordinal_ = 0;
    HParams hp_;
    hipStream_t stream_ = nullptr;
    std::mutex mu_;

    // weights
    char *arena_ = nullptr;
    size_t arena_size_ = 0, arena_used_ = 0;
    DevTable word_, type_, pos_;
    float *ln_e_w_ = nullptr, *ln_e_b_ = nullptr;
    std::vector<DevLayer> layers_;
    int wfmt_ = FMT_F16;
    bool f32_ = false;              // ftype 0 file: the f32 chain (f32.hip)
    bool q8_ = false;               // activation mode 1: the q8-activation chain (q8act.hip + f32.hip)
    const uint16_t *gelu_tab_ = nullptr, *exp_tab_ = nullptr;   // f32 / q8 chains: the era's fp16 tables (host-built)
    // the classification head, f32 (null / 0: the file has none)
    const float *head_wp_ = nullptr, *head_bp_ = nullptr, *head_wc_ = nullptr, *head_bc_ = nullptr;
    int n_labels_ = 0;
    const void *proj_w_ = nullptr;   // the projector's weight image (null / 0: the file has none)
    int proj_dim_ = 0;

    // workspace
    int64_t cap_tokens_ = 0, cap_seqs_ = 0, cap_pool_ = 0;   // cap_pool_: pool partial rows (seqs x chunks)
    hipEvent_t done_ev_ = nullptr;          // completion of the last forward
    hipStream_t last_stream_ = nullptr;     // ... and the stream it ran on
    bool any_forward_ = false;
    char *ws_ = nullptr;
    uint16_t *z_ = nullptr;         // residual stream as z = y * gamma of its LN (f16, kernels.h)
    float2 *st_ = nullptr;          // (mean, 1/sigma) of y
    float2 *part_ = nullptr;        // [d/32][rows] group partials of the residual GEMMs
    int64_t rows_ = 0;              // workspace rows (part_ stride)
    uint16_t *qkv_ = nullptr, *att_ = nullptr, *ffn_ = nullptr;
    float *x32_ = nullptr, *z32_ = nullptr, *qkv32_ = nullptr, *att32_ = nullptr, *ffn32_ = nullptr;   // f32 / q8 chains
    int8_t *xq_ = nullptr;          // q8 chain: the quantized input of the next projection [rows][max(d, f)]
    float *xd_ = nullptr, *xs_ = nullptr;   // ... its block scales and q8_1 sums [max(d, f) / 32][M]
    int32_t *d_ids_ = nullptr, *d_cu_ = nullptr, *d_types_ = nullptr;
    float *d_out_ = nullptr;
    float *head_x_ = nullptr, *head_p_ = nullptr;   // the head's [CLS] rows and pooler output [seqs][d] (files with a head)
    float *pool_part_ = nullptr;
    // the pruned last layer of CLS pooling (f16 chain): compact rows, one per sentence
    uint16_t *zc_ = nullptr, *attc_ = nullptr, *ffnc_ = nullptr;
    float2 *stc_ = nullptr, *partc_ = nullptr;
    int64_t rows_c_ = 0;            // compact workspace rows (partc_ stride)
    float *tok_out_ = nullptr;      // per-token output staging of forward_host [cap_tok_out_][max(d, proj_width)], grown on demand
    int64_t cap_tok_out_ = 0;
    int pool_ = 0;                  // BERTX_POOL_MEAN / BERTX_POOL_CLS
    bool prune_ = true;
    int out_mode_ = OUT_MEAN;       // of the forward being launched
    const int32_t *types_ = nullptr;   // ... and its token types (null: all 0)
    const int32_t *map_ = nullptr;     // ... and, OUT_PROJ, its row map (null: every token) of n_map_ rows
    int n_map_ = 0;
    const int32_t *keys_ = nullptr;    // ... and its key counts (null: every row of a sentence is a key)
    int32_t *d_keys_ = nullptr;        // forward_host's counts on the device [cap_seqs_]
    int32_t *h_ids_ = nullptr, *h_cu_ = nullptr, *h_types_ = nullptr, *h_keys_ = nullptr;   // pinned staging
    float *h_out_ = nullptr;

    // HIP graphs of the launch sequence (cleared when the workspace moves)
    std::vector<GraphEntry> graphs_;
    std::vector<GraphKey> seen_once_;   // a shape is captured on its second use
    bool use_graphs_ = true;

    // profiling
    double lc_ms_ = 0.0;
    int lc_seqs_ = 0;
    int64_t lc_tokens_ = 0;
    int64_t calls_ = 0;

    bool profiling_ = false;
    double att_flop_ = 0.0;         // attention FLOP of the forward being launched
    std::vector<PendingEv> pending_;
    std::vector<hipEvent_t> free_events_;
    KStats stats_[K_NUM_CLASSES];
};

// HIP device count (0 when no runtime / no GPU); never throws.
int hip_device_count();

// An embedding index (index.cpp, bert_hip.h bertx_index_*) of `capacity` rows of width
// d on device `ordinal`, stored as BERTX_INDEX_F16 or _I8, without a context
// (bertx_index_create_ex, the search bench).  NULL after a message.
::bertx_index *index_create_on(int ordinal, int d, int64_t capacity, int storage);

// A token store (mvindex.cpp, bert_hip.h bertx_mvindex_*) of width w for cap_docs
// documents in cap_slots token slots on device `ordinal`, without a context
// (bertx_mvindex_create_ex, the MaxSim bench); storage BERTX_INDEX_F16 or _I8.  NULL
// after a message.
::bertx_mvindex *mvindex_create_on(int ordinal, int w, int64_t cap_docs, int64_t cap_slots, int storage);

}  // namespace emb
