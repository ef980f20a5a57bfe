// The forward of one replica: ordering against the previous forward, graph
// capture / replay, and the launch schedules of the three chains (f16, f32, q8).
#include "engine.h"
#include "hip_check.h"
#include "repack.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace emb {

// The launches of one forward on stream s.  run() puts a launch between the two
// profiling events of its class (work: the class's FLOP or bytes, bertx_kernel_stats)
// and, under BERT_CHECK_FINITE=1, counts the non-finite values of its output over
// the valid rows, reporting the first kernel that produced any (diagnostics).
struct Device::Launcher {
    struct Out {
        const char *what = nullptr, *tag = "";   // kernel name (+ "_cls" on the compact rows)
        int layer = -1;
        const void *p = nullptr;
        size_t n = 0;
        int f16 = 1;
    };
    Device &dev;
    hipStream_t s;
    unsigned *cnt = nullptr;   // the check's device counter; null: check off
    bool bad = false;

    Launcher(Device &d, hipStream_t st, bool check) : dev(d), s(st)
    {
        if (check) (void)hipMalloc((void **)&cnt, sizeof(unsigned));
    }
    ~Launcher() { if (cnt) (void)hipFree(cnt); }
    Launcher(const Launcher &) = delete;
    Launcher &operator=(const Launcher &) = delete;

    // launch: returns void, or non-zero for a refused launch (run() is then false)
    template <class F> bool run(int cls, double work, F &&launch, const Out &o = Out())
    {
        hipEvent_t ev;
        dev.begin(cls, s, ev);
        if constexpr (std::is_void_v<decltype(launch())>) {
            launch();
        } else if (launch() != 0) {
            if (ev) dev.free_events_.push_back(ev);
            return false;
        }
        dev.end(cls, s, ev, work);
        finite(o);
        return true;
    }

    void finite(const Out &o)
    {
        if (!cnt || bad || !o.p) return;
        (void)hipMemsetAsync(cnt, 0, sizeof(unsigned), s);
        launch_count_nonfinite(o.p, o.n, o.f16, cnt, s);
        unsigned h = 0;
        (void)hipMemcpyAsync(&h, cnt, sizeof(unsigned), hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        if (h) {
            bad = true;
            errorf("libbert: BERT_CHECK_FINITE: %u non-finite values after %s%s (layer %d)\n", h, o.what, o.tag, o.layer);
        }
    }

    // after the last launch of a chain
    int finish()
    {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return 0;
        errorf("libbert: kernel launch failed: %s\n", hipGetErrorString(e));
        return -1;
    }
};

int Device::forward_ex(const int32_t *d_ids, const int32_t *d_types, const int32_t *d_cu, int n_seqs, int max_len, int T,
                       int out_kind, float *d_out, hipStream_t s, double len2_sum, const int32_t *d_rows, int n_rows,
                       const int32_t *d_keys)
{
    if (out_kind != KIND_POOLED && out_kind != KIND_TOKENS && out_kind != KIND_LOGITS && out_kind != KIND_PROJ) return -1;
    // key counts come with the per-token outputs only (which never take the pruned last layer)
    if (d_keys && out_kind != KIND_TOKENS && out_kind != KIND_PROJ) return -1;
    if (out_kind == KIND_LOGITS && n_labels_ <= 0) return -6;
    if (out_kind == KIND_PROJ && proj_dim_ <= 0) return -6;
    const bool mapped = out_kind == KIND_PROJ && d_rows != nullptr;
    if (mapped && n_rows < 0) return -1;
    map_ = mapped ? d_rows : nullptr;
    n_map_ = mapped ? n_rows : 0;
    const bool can_prune = prune_ && !f32_ && !q8_;
    out_mode_ = out_kind == KIND_TOKENS   ? OUT_TOKENS
                : out_kind == KIND_PROJ   ? OUT_PROJ
                : out_kind == KIND_LOGITS ? (can_prune ? OUT_LOGITS_PRUNED : OUT_LOGITS)
                : pool_ != 1              ? OUT_MEAN
                                          : can_prune ? OUT_CLS_PRUNED : OUT_CLS;
    types_ = d_types;
    keys_ = d_keys;
    // attention work for the per-kernel stats: exact from the host's lengths when
    // known, else T max_len (exact for equal lengths, an upper bound otherwise)
    att_flop_ = 4.0 * hp_.n_embd * (len2_sum >= 0 ? len2_sum : (double)T * max_len);
    if (!ok_) return -3;
    if (T > cap_tokens_ || n_seqs > cap_seqs_ || (int64_t)n_seqs * pool_chunks(max_len) > cap_pool_) return -2;
    if (T <= 0 || n_seqs <= 0) return 0;
    order_after_last(s);
    const int rc = forward_ordered(d_ids, d_cu, n_seqs, max_len, T, d_out, s);
    mark_done(s);
    return rc;
}

int Device::forward_ordered(const int32_t *d_ids, const int32_t *d_cu, int n_seqs, int max_len, int T, float *d_out,
                            hipStream_t s)
{
    // BERT_CHECK_FINITE=1 (Launcher): eager launches, never captured
    static const bool check = [] { const char *e = std::getenv("BERT_CHECK_FINITE"); return e && *e == '1'; }();
    static const bool graphs_env = [] { const char *e = std::getenv("BERT_GRAPHS"); return !(e && *e == '0'); }();
    if (profiling_ || check || !use_graphs_ || !graphs_env || s == nullptr)
        return launch_all(d_ids, d_cu, n_seqs, max_len, T, d_out, s, check);
    const GraphKey key{d_ids, d_cu, d_out, s, n_seqs, max_len, T, out_mode_, types_, map_, n_map_, keys_};
    for (auto &g : graphs_)
        if (g.key == key) return hipGraphLaunch(g.exec, s) == hipSuccess ? 0 : -1;
    // a shape seen for the first time runs eagerly (one-off batches never pay
    // for a capture); on its second use the sequence is captured and replayed
    bool seen = false;
    for (auto &k : seen_once_) seen = seen || (k == key);
    if (!seen) {
        if (seen_once_.size() >= 32) seen_once_.erase(seen_once_.begin());
        seen_once_.push_back(key);
        return launch_all(d_ids, d_cu, n_seqs, max_len, T, d_out, s, false);
    }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        use_graphs_ = false;   // this runtime / stream cannot capture: stay eager
        return launch_all(d_ids, d_cu, n_seqs, max_len, T, d_out, s, false);
    }
    const int rc = launch_all(d_ids, d_cu, n_seqs, max_len, T, d_out, s, false);
    const hipError_t ec = hipStreamEndCapture(s, &graph);
    if (rc != 0 || ec != hipSuccess || hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (graph) (void)hipGraphDestroy(graph);
        use_graphs_ = false;
        return launch_all(d_ids, d_cu, n_seqs, max_len, T, d_out, s, false);
    }
    (void)hipGraphDestroy(graph);
    if (graphs_.size() >= 8) {
        (void)hipGraphExecDestroy(graphs_.front().exec);
        graphs_.erase(graphs_.begin());
    }
    graphs_.push_back({key, exec});
    return hipGraphLaunch(exec, s) == hipSuccess ? 0 : -1;
}

int Device::launch_all(const int32_t *d_ids, const int32_t *d_cu, int n_seqs, int max_len, int T, float *d_out,
                       hipStream_t s, bool check)
{
    Launcher run(*this, s, check);
    const int rc = f32_ || q8_ ? chain_32(run, d_ids, d_cu, n_seqs, max_len, T, d_out)
                               : chain_f16(run, d_ids, d_cu, n_seqs, max_len, T, d_out);
    return rc != 0 ? rc : run.finish();
}

// The f16 chain (f16 and quantized files): the residual stream as z with its row
// statistics (kernels.h LN fold), every GEMM on the f16 MFMA path.
int Device::chain_f16(Launcher &run, const int32_t *d_ids, const int32_t *d_cu, int n_seqs, int max_len, int T,
                      float *d_out)
{
    using Out = Launcher::Out;
    hipStream_t s = run.s;
    const int d = hp_.n_embd;
    const int M = gemm_rows(T);   // GEMM rows: T padded to whole tiles
    const double t = (double)T;
    const size_t Td = (size_t)T * d;

    run.run(K_EMBED_LN, t * (4.0 + 3.0 * d * 2.0 + 2.0 * d + 8.0),
            [&] { launch_embed_ln(word_, type_, pos_, ln_e_w_, d_ids, d_cu, n_seqs, max_len, d, z_, st_, s, types_); },
            Out{"embed_ln", "", -1, z_, Td});
    // z_ holds the stream as z = y * gamma of the LN in front of the next
    // projection, st_ its (mean, 1/sigma) (kernels.h LN fold); (gz, bz) is that LN
    const float *gz = ln_e_w_, *bz = ln_e_b_;
    const int G = d / 32;
    // Small batches: the projections combine their input's LN statistics from the
    // residual GEMM's partials themselves (LnFold::in_part; the column-0 tiles store
    // them for the residual GEMM after), so only the last ln_stats launch (for the
    // pool) remains: 2 n_layer - 1 fewer launches, the same bits (the combine is
    // ln_stats_kernel's arithmetic).  Where the tile config has no LDS for it (the
    // large-batch tiles, d > 768 on 64-row tiles), the statistics launches stay.
    static const bool fold_env = [] { const char *e = std::getenv("BERT_STATS_FOLD"); return !(e && *e == '0'); }();
    const bool fold = fold_env && !layers_.empty() && gemm_fold_ok(layers_[0].qkv, M, G) && gemm_fold_ok(layers_[0].up, M, G);
    const double att_flop = att_flop_;   // sum over sentences of 4 d len^2 (QK^T and PV), set by the caller

    for (int l = 0; l < hp_.n_layer; ++l) {
        const DevLayer &L = layers_[(size_t)l];
        const bool last = l + 1 == hp_.n_layer;
        RowSet r{M, t, (size_t)T, z_, st_, part_, (int32_t)rows_, att_, ffn_, fold, last, ""};
        // fold, past layer 0: the stream of the previous FFN-down comes with its partials
        // (layer 0 reads the embedding's statistics)
        const LnFold in = r.input(fold && l > 0, G, L.c1_qkv);
        if (!run.run(K_GEMM_QKV, 2.0 * t * 3.0 * d * d,
                     [&] { return launch_gemm(L.qkv, z_, M, L.c2_qkv, EPI_BIAS_F16, nullptr, qkv_, s, in); },
                     Out{"gemm_qkv", "", l, qkv_, Td * 3}))
            return -1;

        if (pruned_last() && last) {
            // CLS pooling and the head read one row per sentence of this layer: attention of the
            // sentences' first rows only (its launch gathers their residual rows into
            // zc_ / stc_), then the rest of the layer on Mc compact rows
            const int Mc = gemm_rows(n_seqs);
            r = RowSet{Mc, (double)n_seqs, (size_t)Mc, zc_, stc_, partc_, (int32_t)rows_c_, attc_, ffnc_,
                       fold_env && gemm_fold_ok(L.up, Mc, G), true, "_cls"};
            if (!run.run(K_ATTENTION, 4.0 * d * t,   // one query per sentence: 4 d len FLOP each
                         [&] { return launch_attention_cls(qkv_, d_cu, n_seqs, hp_.n_head, d, Mc, attc_, z_, st_, zc_, stc_, s); },
                         Out{"attention", "_cls", l, attc_, (size_t)Mc * d}))
                return -1;
            run.finite(Out{"gather", "_cls", l, zc_, (size_t)Mc * d});
        } else {
            run.run(K_ATTENTION, att_flop, [&] { launch_attention(qkv_, d_cu, n_seqs, max_len, hp_.n_head, d, att_, s, keys_); },
                    Out{"attention", "", l, att_, Td});
        }
        if (layer_tail(run, L, l, r, gz, bz) != 0) return -1;
    }

    if (out_mode_ == OUT_LOGITS || out_mode_ == OUT_LOGITS_PRUNED) {
        // the head's [CLS] rows: of the compact last layer, or of the full one
        run.run(K_POOL_L2, (double)n_seqs * (d * 6.0 + 8.0), [&] {
            if (out_mode_ == OUT_LOGITS_PRUNED) launch_head_gather(zc_, stc_, gz, bz, nullptr, n_seqs, d, head_x_, s);
            else launch_head_gather(z_, st_, gz, bz, d_cu, n_seqs, d, head_x_, s);
        }, Out{"head_gather", "", -1, head_x_, (size_t)n_seqs * d, 0});
        return head(run, n_seqs, d_out);
    }
    if (out_mode_ == OUT_PROJ) {
        // the projector reads z and the statistics as the token output does and writes
        // proj_width floats per mapped row (a row map of 0 rows: nothing to do)
        const int n_out = map_ ? n_map_ : T, width = proj_width();
        if (n_out == 0) return 0;
        const bool ok = run.run(K_POOL_L2, (double)n_out * (d * 2.0 + 8.0 + width * 4.0), [&] {
            return launch_project(z_, st_, gz, bz, nullptr, d, proj_w_, proj_dim_, map_, n_out, d_out, s);
        }, Out{"project", "", -1, d_out, (size_t)n_out * width, 0});
        return ok ? 0 : -1;
    }
    const Out out{"pool_l2", "", -1, d_out, (out_mode_ == OUT_TOKENS ? (size_t)T : (size_t)n_seqs) * d, 0};
    if (out_mode_ == OUT_MEAN) {
        run.run(K_POOL_L2, t * d * 2.0 + t * 8.0 + (double)n_seqs * d * 4.0,
                [&] { launch_pool_l2(z_, st_, gz, bz, d_cu, n_seqs, max_len, d, pool_part_, d_out, s); }, out);
    } else if (out_mode_ == OUT_TOKENS) {
        run.run(K_POOL_L2, t * d * 6.0 + t * 8.0, [&] { launch_tokens_f32(z_, st_, gz, bz, T, d, d_out, s); }, out);
    } else {
        // the sentences' first rows: of the compact last layer, or of the full one
        run.run(K_POOL_L2, (double)n_seqs * (d * 6.0 + 8.0), [&] {
            if (out_mode_ == OUT_CLS_PRUNED) launch_cls_l2(zc_, stc_, gz, bz, nullptr, n_seqs, d, d_out, s);
            else launch_cls_l2(z_, st_, gz, bz, d_cu, n_seqs, d, d_out, s);
        }, out);
    }
    return 0;
}

// The classification head on head_x_ (the sentences' final-LayerNorm [CLS] rows): the
// pooler GEMM + tanh and the classifier (head.hip), timed in the output-stage class.
// Work: the bytes of the pooler rows, read once per 16 sentences.
int Device::head(Launcher &run, int n_seqs, float *d_out)
{
    const int d = hp_.n_embd;
    const double tiles = (double)((n_seqs + 15) / 16);
    const bool ok = run.run(K_POOL_L2, tiles * d * d * 4.0 + (double)n_seqs * d * 12.0, [&] {
        return launch_head(head_x_, n_seqs, d, head_wp_, head_bp_, head_wc_, head_bc_, n_labels_, head_p_, d_out, run.s);
    }, Launcher::Out{"head", "", -1, d_out, (size_t)n_seqs * n_labels_, 0});
    return ok ? 0 : -1;
}

// The LN side of a projection that reads the rows' stream (c1 = W gamma): with the
// fold, the partials of the residual GEMM before it, which the projection combines
// itself, leaving the rows' statistics in st for the residual GEMM after; else st.
LnFold Device::RowSet::input(bool fold_in, int G, const float *c1) const
{
    LnFold in;
    if (fold_in) {
        in.in_part = part; in.in_part_stride = part_stride; in.in_G = G; in.st_out = st;
    } else {
        in.in_stats = st;
    }
    in.c1 = c1;
    return in;
}

// A layer of the f16 chain after its attention, on the rows of r: O-proj residual,
// FFN-up, FFN-down residual.  The residual GEMMs write the new stream's partials;
// with r.fold the projection after combines them itself, else an ln_stats launch
// does -- and always after the last layer, for the output stage.  (gz, bz): the LN
// in front of the stream, moved on to this layer's output LN.
int Device::layer_tail(Launcher &run, const DevLayer &L, int l, const RowSet &r, const float *&gz, const float *&bz)
{
    using Out = Launcher::Out;
    hipStream_t s = run.s;
    const int d = hp_.n_embd, f = hp_.n_intermediate, G = d / 32;
    auto ln_stats = [&] {
        return run.run(K_LN_STATS, (double)r.M * (G + 1) * 8.0,
                       [&] { return launch_ln_stats(r.part, G, r.part_stride, r.M, d, r.st, s); });
    };
    // the residual GEMM into z (in place; refused: z would be stale)
    auto residual = [&](int cls, double work, const DevWeight &W, const uint16_t *X, const float *bias,
                        const float *g_next, const char *what) {
        LnFold res;
        res.res_stats = r.st; res.res_g = gz; res.res_b = bz;
        res.g_next = g_next; res.part = r.part; res.part_stride = r.part_stride;
        return run.run(cls, work,
                       [&] { return launch_gemm(W, X, r.M, bias, EPI_BIAS_RES, r.z, r.z, s, res); },
                       Out{what, r.tag, l, r.z, r.valid * d});
    };

    // y1 = LN(y) + ATT W_o^T + b_o, stored as z = y1 * gamma_1 with its partials
    if (!residual(K_GEMM_O, 2.0 * r.flop_rows * d * d, L.o, r.att, L.b_o, L.ln1_w, "gemm_o")) return -1;
    if (!r.fold && !ln_stats()) return -1;
    gz = L.ln1_w; bz = L.ln1_b;
    const LnFold in = r.input(r.fold, G, L.c1_up);
    if (!run.run(K_GEMM_FFN_UP, 2.0 * r.flop_rows * d * f,
                 [&] { return launch_gemm(L.up, r.z, r.M, L.c2_up, EPI_BIAS_GELU_F16, nullptr, r.ffn, s, in); },
                 Out{"gemm_up", r.tag, l, r.ffn, r.valid * f}))
        return -1;
    if (!residual(K_GEMM_FFN_DOWN, 2.0 * r.flop_rows * d * f, L.down, r.ffn, L.b_down, L.ln2_w, "gemm_down")) return -1;
    if ((!r.fold || r.last) && !ln_stats()) return -1;   // (fold: only the output stage's statistics)
    gz = L.ln2_w; bz = L.ln2_b;
    return 0;
}

// The f32 chain (ftype 0 files, f32.hip): bert.cpp:963-1095 with every tensor in
// f32, the reference's own op order (QKV + bias, attention, (bias + O) + x, LN,
// GELU(bias + FFN-up), z + (bias + FFN-down), LN; mean pool, divide by the norm).
// The q8-activation chain (q4_0 / q4_1 / q8_0 files in activation mode 1) is the same
// schedule with `exact` kernels (the reference's roundings and summation orders) and
// every projection in the reference's block arithmetic: its input re-quantized to
// q8_0 / q8_1 (bert.cpp:995 through ggml; rows T <= row < M, tile padding, enter as
// zeros), then the integer block GEMM (q8act.hip), both timed in the projection's class.
int Device::chain_32(Launcher &run, const int32_t *d_ids, const int32_t *d_cu, int n_seqs, int max_len, int T,
                     float *d_out)
{
    using Out = Launcher::Out;
    hipStream_t s = run.s;
    const int d = hp_.n_embd, f = hp_.n_intermediate;
    const int M = gemm_rows(T);
    const double t = (double)T;
    const size_t Td = (size_t)T * d, nd = (size_t)n_seqs * d;
    const bool exact = q8_;
    const int kind = wfmt_ == FMT_Q4_1 ? 1 : 0;   // q8_1 activations for q4_1 weights, else q8_0
    // Y [M][N] = epi(X W^T): W the lane-order weight (q8 chain) or the f32 rows w32; 2 T N K FLOP
    auto proj = [&](int cls, const char *what, int l, const DevWeight &W, const float *w32, int N, int K,
                    const float *X, const float *bias, int epi, const float *res, float *Y) {
        return run.run(cls, 2.0 * t * N * K, [&] {
            if (!q8_) return launch_f32_gemm(X, M, w32, N, K, bias, epi, res, Y, s, gelu_tab_);
            if (launch_q8_quantize(X, T, M, W.K, kind, xq_, xd_, xs_, s)) return -1;
            return launch_q8_gemm(W, xq_, xd_, xs_, M, bias, epi, res, Y, s, gelu_tab_);
        }, Out{what, "", l, Y, (size_t)T * N, 0});
    };
    auto ln = [&](int l, float *x, const float *g, const float *b) {
        run.run(K_LN_STATS, (double)M * d * 8.0, [&] { launch_f32_ln(x, M, d, g, b, s, exact); }, Out{"ln", "", l, x, Td, 0});
    };
    run.run(K_EMBED_LN, t * (4.0 + 3.0 * d * 4.0 + 4.0 * d), [&] {
        launch_f32_embed_ln(word_, type_, pos_, ln_e_w_, ln_e_b_, d_ids, d_cu, n_seqs, max_len, d, x32_, s, exact, types_);
    }, Out{"embed_ln", "", -1, x32_, Td, 0});
    for (int l = 0; l < hp_.n_layer; ++l) {
        const DevLayer &L = layers_[(size_t)l];
        if (!proj(K_GEMM_QKV, "gemm_qkv", l, L.qkv, L.w32_qkv, 3 * d, d, x32_, L.b_qkv, 0, nullptr, qkv32_)) return -1;
        if (!run.run(K_ATTENTION, att_flop_, [&] {
                return launch_f32_attention(qkv32_, d_cu, n_seqs, max_len, hp_.n_head, d, att32_, s, exp_tab_, exact, keys_);
            }, Out{"attention", "", l, att32_, Td, 0}))
            return -1;
        if (!proj(K_GEMM_O, "gemm_o", l, L.o, L.w32_o, d, d, att32_, L.b_o, 2, x32_, z32_)) return -1;
        ln(l, z32_, L.ln1_w, L.ln1_b);
        if (!proj(K_GEMM_FFN_UP, "gemm_up", l, L.up, L.w32_up, f, d, z32_, L.b_up, 1, nullptr, ffn32_)) return -1;
        if (!proj(K_GEMM_FFN_DOWN, "gemm_down", l, L.down, L.w32_down, d, f, ffn32_, L.b_down, 2, z32_, x32_)) return -1;
        ln(l, x32_, L.ln2_w, L.ln2_b);
    }
    // x32_ holds the final LayerNorm output: the mean pool; CLS, a gather + normalise;
    // the token output, a copy
    bool ok;
    if (out_mode_ == OUT_LOGITS) {
        run.run(K_POOL_L2, (double)n_seqs * d * 8.0, [&] { launch_head_gather_f32(x32_, d_cu, n_seqs, d, head_x_, s); },
                Out{"head_gather", "", -1, head_x_, nd, 0});
        return head(run, n_seqs, d_out);
    }
    if (out_mode_ == OUT_PROJ) {
        const int n_out = map_ ? n_map_ : T, width = proj_width();
        if (n_out == 0) return 0;
        ok = run.run(K_POOL_L2, (double)n_out * (d * 4.0 + width * 4.0), [&] {
            return launch_project(nullptr, nullptr, nullptr, nullptr, x32_, d, proj_w_, proj_dim_, map_, n_out, d_out, s);
        }, Out{"project", "", -1, d_out, (size_t)n_out * width, 0});
        return ok ? 0 : -1;
    }
    if (out_mode_ == OUT_MEAN)
        ok = run.run(K_POOL_L2, t * d * 4.0 + (double)n_seqs * d * 4.0,
                     [&] { launch_f32_pool(x32_, d_cu, n_seqs, d, d_out, s, exact); }, Out{"pool_l2", "", -1, d_out, nd, 0});
    else if (out_mode_ == OUT_TOKENS)
        ok = run.run(K_POOL_L2, (double)T * d * 8.0,
                     [&] { return hipMemcpyAsync(d_out, x32_, sizeof(float) * Td, hipMemcpyDeviceToDevice, s); });
    else
        ok = run.run(K_POOL_L2, (double)n_seqs * d * 8.0, [&] { launch_f32_cls(x32_, d_cu, n_seqs, d, d_out, s); },
                     Out{"pool_l2", "", -1, d_out, nd, 0});
    return ok ? 0 : -1;
}

int Device::forward_host(const int32_t *const *tokens, const int32_t *lens, int n, float *const *out, bool tok_out,
                         const int32_t *const *types, bool logits, bool proj, const int32_t *keys)
{
    if (!ok_) return -3;
    if (keys && !tok_out) return -1;
    if (logits && n_labels_ <= 0) return -6;
    if (proj && proj_dim_ <= 0) return -6;
    if (n <= 0) return 0;
    int64_t T = 0;
    int max_len = 0;
    double len2 = 0.0;
    for (int i = 0; i < n; ++i) {
        T += lens[i];
        max_len = std::max(max_len, (int)lens[i]);
        len2 += (double)lens[i] * lens[i];
    }
    DeviceGuard g(ordinal_);
    HIP_RC(g.status());
    if (!reserve(T, n, max_len)) return -1;
    order_after_last(stream_);   // the previous forward may have run on a caller stream
    h_cu_[0] = 0;
    for (int i = 0; i < n; ++i) {
        std::memcpy(h_ids_ + h_cu_[i], tokens[i], sizeof(int32_t) * (size_t)lens[i]);
        h_cu_[i + 1] = h_cu_[i] + lens[i];
    }
    HIP_RC(hipMemcpyAsync(d_ids_, h_ids_, sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, stream_));
    HIP_RC(hipMemcpyAsync(d_cu_, h_cu_, sizeof(int32_t) * (size_t)(n + 1), hipMemcpyHostToDevice, stream_));
    if (types) {
        for (int i = 0; i < n; ++i) std::memcpy(h_types_ + h_cu_[i], types[i], sizeof(int32_t) * (size_t)lens[i]);
        HIP_RC(hipMemcpyAsync(d_types_, h_types_, sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, stream_));
    }
    const int32_t *dty = types ? d_types_ : nullptr;
    if (keys) {
        std::memcpy(h_keys_, keys, sizeof(int32_t) * (size_t)n);
        HIP_RC(hipMemcpyAsync(d_keys_, h_keys_, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, stream_));
    }
    const size_t d = (size_t)hp_.n_embd;
    if (tok_out) {
        // per-token output: a device buffer of its own, grown on demand, and plain
        // copies into the caller's buffers (not a hot path)
        if (T > cap_tok_out_) {
            HIP_RC(hipStreamSynchronize(stream_));
            if (tok_out_) { (void)hipFree(tok_out_); tok_out_ = nullptr; }
            cap_tok_out_ = 0;
            drop_graphs();   // captured token forwards hold the old pointer
            const int64_t cap = (int64_t)align_up((size_t)T, 4096);
            HIP_RC(hipMalloc((void **)&tok_out_, sizeof(float) * std::max(d, (size_t)proj_width()) * (size_t)cap));
            cap_tok_out_ = cap;
        }
        const size_t tw = proj ? (size_t)proj_width() : d;   // floats per row of this output
        const int rc = forward_ex(d_ids_, dty, d_cu_, n, max_len, (int)T, proj ? KIND_PROJ : KIND_TOKENS, tok_out_, stream_,
                                  len2, nullptr, 0, keys ? d_keys_ : nullptr);
        if (rc != 0) return rc;
        HIP_RC(hipStreamSynchronize(stream_));
        for (int i = 0; i < n; ++i)
            HIP_RC(hipMemcpy(out[i], tok_out_ + tw * (size_t)h_cu_[i], sizeof(float) * tw * (size_t)lens[i],
                             hipMemcpyDeviceToHost));
        return 0;
    }
    // (the staging rows are n_embd wide; the logits, n_labels <= 16 per sentence, fit in them)
    const size_t w = logits ? (size_t)n_labels_ : d;
    const int rc = forward_ex(d_ids_, dty, d_cu_, n, max_len, (int)T, logits ? KIND_LOGITS : KIND_POOLED, d_out_, stream_, len2);
    if (rc != 0) return rc;
    HIP_RC(hipMemcpyAsync(h_out_, d_out_, sizeof(float) * w * (size_t)n, hipMemcpyDeviceToHost, stream_));
    HIP_RC(hipStreamSynchronize(stream_));
    for (int i = 0; i < n; ++i) std::memcpy(out[i], h_out_ + w * (size_t)i, sizeof(float) * w);
    return 0;
}

}  // namespace emb
