// The drop-in C ABI (include/bert.h, reference bert.h:18-90) and the MI355X
// extensions (include/bert_hip.h): context lifetime, tokenization, batching,
// multi-GPU sharding of encode calls.  No CPU compute path: every forward runs
// on the HIP kernels, and fails loudly when no device is present.
#include "bert.h"
#include "bert_hip.h"
#include "ggml.h"

#include "chunk_rule.h"
#include "engine.h"
#include "task_pool.h"
#include "tokenizer.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

using emb::Device;

namespace {

// A persistent host thread per replica (multi-replica contexts): run_forward posts
// a replica's share of a call to it instead of creating a std::thread per call.
class ReplicaWorker {
public:
    ReplicaWorker() : th_([this] { loop(); }) {}
    ~ReplicaWorker()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_one();
        th_.join();
    }
    void post(std::function<void()> f)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            q_.push_back(std::move(f));
        }
        cv_.notify_one();
    }

private:
    void loop()
    {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;   // stop_ with nothing queued
                f = std::move(q_.front());
                q_.pop_front();
            }
            // nothing may leave the worker thread (std::terminate); run_forward's
            // tasks catch their own failures, this is the last line
            try { f(); } catch (...) { emb::errorf("libbert: replica worker task failed\n"); }
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    bool stop_ = false;
    std::thread th_;
};

}  // namespace

struct bert_ctx {
    emb::HParams hp;
    emb::Vocab vocab;
    std::vector<std::unique_ptr<Device>> devices;
    bool host_only = false;
    int act_mode = 0;   // the activation mode the context runs (bertx_activation_mode)
    int pool = 0;       // BERTX_POOL_MEAN / BERTX_POOL_CLS (bertx_set_pooling), mirrored on every replica
    int n_labels = 0;   // logits per sentence of the file's classification head; 0: none (bertx_n_labels)
    int proj_dim = 0;   // rows of the file's ColBERT projection; 0: none (bertx_proj_dim)
    // whether a ColBERT query's [MASK] rows are attention keys (bertx_set_mask_keys).  One value
    // for the context: the replicas hold no copy, the counts travel with each forward.
    std::atomic<int> mask_keys{1};
    // routing state of run_forward: the cost of the work routed to each replica and
    // not yet finished, and the rotation that breaks ties between equal loads
    std::mutex route_mu;
    std::vector<double> inflight;
    unsigned rr = 0;
    // declared after `devices`: destroyed (joined) before the replicas they drive
    std::vector<std::unique_ptr<ReplicaWorker>> workers;
};

namespace {

// A call is split only over replicas that are idle (no routed work in flight), and
// only while each share keeps at least kMinShareTokens.  The choice, from the
// measured per-share latency on one replica (scripts/share_curve.py,
// profiles/r05_share_curve.jsonl: bge-base q4_0, 128-token sentences through
// bert_forward_batch): the cost per token is 4.7x the large-batch asymptote at 128
// tokens, 1.8x at 4,096, 1.26x at 8,192 and 1.07x at 16,384.  The curve's own knee
// criterion (within 1.25x of the asymptote) gives 16,384; 8,192 is the smallest
// share for which a 2-way split still pays: a 16,384-token call takes 3.63 ms on one
// replica and 2.14 ms as two 8,192-token shares, while at 4,096 tokens per share
// (1.52 ms) the two half-size forwards buy 0.6 ms for a whole second replica.  A
// call that finds no idle replica goes whole to the least-loaded one, so concurrent
// callers (the server's batchers) land on different replicas instead of all
// splitting over all of them in lockstep.
constexpr int64_t kMinShareTokens = 8192;

std::vector<int> parse_device_list(int n_visible)
{
    std::vector<int> out;
    const char *env = std::getenv("BERT_DEVICES");
    if (!env || !*env) {
        for (int i = 0; i < n_visible; ++i) out.push_back(i);
        return out;
    }
    std::string s(env);
    size_t p = 0;
    while (p <= s.size()) {
        size_t q = s.find(',', p);
        if (q == std::string::npos) q = s.size();
        const std::string tok = s.substr(p, q - p);
        if (!tok.empty()) {
            const int v = std::atoi(tok.c_str());
            // a repeated ordinal is a second replica (own stream + workspace) on that device
            if (v >= 0 && v < n_visible) out.push_back(v);
        }
        p = q + 1;
    }
    return out;
}

// FLOP-proportional cost of one sentence of length L (GEMMs + attention).
double sentence_cost(const emb::HParams &hp, int L)
{
    const double d = hp.n_embd, f = hp.n_intermediate;
    return (double)L * (8.0 * d * d + 4.0 * d * f) + 4.0 * (double)L * L * d;
}

// Runs n sentences on the context's GPUs.  Routing (kMinShareTokens): the call
// uses k = min(idle replicas, sentences, tokens / kMinShareTokens) (at least 1)
// replicas, the k least-loaded by the cost still in flight on them (ties rotate,
// so consecutive small calls spread over the replicas too); its sentences are split over those k
// by cost, longest first to the least-loaded share (LPT).  Each replica walks its
// sentences in chunks (chunk_rule.h) on its persistent worker thread (the
// caller runs one share itself).  Results are independent of the routing and the
// split: every kernel computes a sentence from its own tokens only.
// types (or null) ride along with the ids; logits: outs[i] receives the n_labels raw
// logits of the file's head instead of an embedding (-6 without a head).
int run_forward(bert_ctx *ctx, const int32_t *const *toks, const int32_t *lens, float *const *outs, int n,
                const int32_t *const *types = nullptr, bool logits = false)
{
    if (ctx->devices.empty()) {
        emb::errorf("libbert: no HIP device in this context (BERT_HOST_ONLY); forward unavailable\n");
        return -1;
    }
    if (n <= 0) return 0;
    const int nd = (int)ctx->devices.size();
    std::vector<int> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lens[a] > lens[b]; });
    int64_t tokens = 0;
    for (int i = 0; i < n; ++i) tokens += lens[i];
    std::vector<std::vector<int>> assign((size_t)nd);
    std::vector<double> load((size_t)nd, 0.0);
    std::vector<int> chosen((size_t)nd);
    {
        std::lock_guard<std::mutex> lk(ctx->route_mu);
        int64_t idle = 0;
        for (double w : ctx->inflight) idle += w == 0.0 ? 1 : 0;
        const int k = (int)std::max<int64_t>(1, std::min<int64_t>({idle, (int64_t)n, tokens / kMinShareTokens}));
        std::iota(chosen.begin(), chosen.end(), 0);
        const unsigned rot = ctx->rr;
        std::stable_sort(chosen.begin(), chosen.end(), [&](int a, int b) {
            if (ctx->inflight[(size_t)a] != ctx->inflight[(size_t)b]) return ctx->inflight[(size_t)a] < ctx->inflight[(size_t)b];
            return (unsigned)(a - (int)rot + nd) % nd < (unsigned)(b - (int)rot + nd) % nd;
        });
        chosen.resize((size_t)k);
        ctx->rr = (rot + (unsigned)k) % (unsigned)nd;
        for (int idx : order) {
            int best = chosen[0];
            for (int dv : chosen) if (load[(size_t)dv] < load[(size_t)best]) best = dv;
            assign[(size_t)best].push_back(idx);
            load[(size_t)best] += sentence_cost(ctx->hp, lens[idx]);
        }
        for (int dv : chosen) ctx->inflight[(size_t)dv] += load[(size_t)dv];
    }
    std::vector<int> rcs((size_t)nd, 0);
    auto work = [&](int dv) {
        Device &D = *ctx->devices[(size_t)dv];
        std::lock_guard<std::mutex> lk(D.mutex());
        const std::vector<int> &mine = assign[(size_t)dv];
        const auto t0 = std::chrono::steady_clock::now();
        int64_t toks_done = 0;
        struct Stamp {   // this call's share of the device: wall time, sentences, tokens
            Device &D; const std::chrono::steady_clock::time_point &t0; const std::vector<int> &mine; int64_t &toks;
            ~Stamp()
            {
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                D.set_last_call(ms, (int)mine.size(), toks);
            }
        } stamp{D, t0, mine, toks_done};
        std::vector<const int32_t *> tp, yp;
        std::vector<int32_t> lp;
        std::vector<float *> op;
        size_t i = 0;
        while (i < mine.size()) {
            tp.clear(); lp.clear(); op.clear(); yp.clear();
            int64_t tok = 0;
            for (const size_t e = emb::chunk_end([&](size_t j) { return lens[mine[j]]; }, i, mine.size()); i < e;) {
                const int idx = mine[i++];
                tp.push_back(toks[idx]); lp.push_back(lens[idx]); op.push_back(outs[idx]);
                if (types) yp.push_back(types[idx]);
                tok += lens[idx];
            }
            const int rc = D.forward_host(tp.data(), lp.data(), (int)tp.size(), op.data(), false,
                                          types ? yp.data() : nullptr, logits);
            if (rc != 0) { rcs[(size_t)dv] = rc; return; }
            toks_done += tok;
        }
    };
    auto finish = [&](int dv) {
        std::lock_guard<std::mutex> lk(ctx->route_mu);
        ctx->inflight[(size_t)dv] -= load[(size_t)dv];
        if (ctx->inflight[(size_t)dv] < 0.5) ctx->inflight[(size_t)dv] = 0.0;   // idle again (no float drift)
    };
    // One share, exception-safe: a failure (bad_alloc staging the chunk, a throwing
    // forward) becomes that share's rc, and `finish` always runs, so the replica
    // counts as idle again and no task outlives this frame with an exception.
    auto run_share = [&](int dv) noexcept {
        try {
            work(dv);
        } catch (const std::exception &ex) {
            emb::errorf("libbert: replica %d share failed: %s\n", dv, ex.what());
            rcs[(size_t)dv] = -1;
        } catch (...) {
            emb::errorf("libbert: replica %d share failed\n", dv);
            rcs[(size_t)dv] = -1;
        }
        finish(dv);
    };
    std::vector<int> used;
    for (int dv : chosen) if (!assign[(size_t)dv].empty()) used.push_back(dv);
    if (used.size() <= 1 || ctx->workers.size() != (size_t)nd) {
        for (int dv : used) run_share(dv);
    } else {
        // the other shares on their replicas' persistent workers, the first on this
        // thread; `left` counts only the tasks actually posted (a post that throws
        // runs its share here), and this frame outlives every posted task
        std::mutex mu;
        std::condition_variable cv;
        size_t left = 0;
        for (size_t i = 1; i < used.size(); ++i) {
            const int dv = used[i];
            {
                std::lock_guard<std::mutex> lk(mu);
                ++left;
            }
            try {
                ctx->workers[(size_t)dv]->post([&, dv] {
                    run_share(dv);
                    std::lock_guard<std::mutex> lk(mu);
                    if (--left == 0) cv.notify_one();
                });
            } catch (...) {
                {
                    std::lock_guard<std::mutex> lk(mu);
                    --left;
                }
                run_share(dv);
            }
        }
        run_share(used[0]);
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return left == 0; });
    }
    for (int rc : rcs) if (rc != 0) {
        emb::errorf("libbert: forward failed (%d)\n", rc);
        return rc;
    }
    return 0;
}

// Tokenize n texts into ids[i * n_max ..] (lens[i] = bert_tokenize's count, which
// may exceed n_max: bert.cpp:386-387) on up to n_threads threads of the persistent
// pool; the stage bert_encode_batch runs first (bert.cpp:1402-1406, sequential in
// the reference).  Blocks of 8 texts per task.  False (after a message) when a
// task threw (e.g. bad_alloc growing a scratch buffer): nothing may unwind out of
// the C ABI, and the caller leaves its outputs untouched, as on every refusal.
bool tokenize_all(const bert_ctx *ctx, int n_threads, int n, const char *const *texts, int32_t n_max, int32_t *ids,
                  int32_t *lens)
{
    const int64_t n_blocks = ((int64_t)n + 7) / 8;
    try {
        emb::TaskPool::instance().run(n_blocks, n_threads, [&](int64_t blk) {
            const int e = (int)std::min<int64_t>(n, 8 * blk + 8);
            for (int i = (int)(8 * blk); i < e; ++i)
                lens[i] = ctx->vocab.tokenize(texts[i], n_max, ids + (size_t)i * n_max, n_max);
        });
    } catch (const std::exception &ex) {
        emb::errorf("libbert: tokenization failed: %s\n", ex.what());
        return false;
    } catch (...) {
        emb::errorf("libbert: tokenization failed\n");
        return false;
    }
    return true;
}

void print_usage(char **argv, const bert_params &p)
{
    std::fprintf(stderr, "usage: %s [options]\n\noptions:\n", argv[0]);
    std::fprintf(stderr, "  -h, --help            show this help message and exit\n");
    std::fprintf(stderr, "  -t N, --threads N     host threads (tokenizer pool) (default: %d)\n", p.n_threads);
    std::fprintf(stderr, "  -p PROMPT, --prompt PROMPT\n                        prompt text (default: %s)\n", p.prompt);
    std::fprintf(stderr, "  --port p              port to bind in server mode (default: %d)\n", p.port);
    std::fprintf(stderr, "  -m FNAME, --model FNAME\n                        model path (default: %s)\n", p.model);
    std::fprintf(stderr, "  environment: BERT_DEVICES=0,1,... (GPUs to use), BERT_HOST_ONLY=1\n\n");
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// ggml time shims (examples/main.cpp, test_batch_encode.cpp call these)
// ---------------------------------------------------------------------------
static std::chrono::steady_clock::time_point g_t0 = std::chrono::steady_clock::now();
void ggml_time_init(void) { g_t0 = std::chrono::steady_clock::now(); }
int64_t ggml_time_us(void)
{
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - g_t0).count();
}
int64_t ggml_time_ms(void) { return ggml_time_us() / 1000; }

// ---------------------------------------------------------------------------
// bert.h
// ---------------------------------------------------------------------------

bool bert_params_parse(int argc, char **argv, bert_params &params)
{
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has_val = i + 1 < argc;
        if ((a == "-t" || a == "--threads") && has_val) params.n_threads = std::stoi(argv[++i]);
        else if ((a == "-p" || a == "--prompt") && has_val) params.prompt = argv[++i];
        else if (a == "--port" && has_val) params.port = std::stoi(argv[++i]);
        else if ((a == "-m" || a == "--model") && has_val) params.model = argv[++i];
        else if (a == "-h" || a == "--help") { print_usage(argv, params); std::exit(0); }
        else {
            std::fprintf(stderr, "error: unknown argument: %s\n", a.c_str());
            print_usage(argv, params);
            std::exit(0);
        }
    }
    return true;
}

// The reference's loader reports and returns nullptr on every failure
// (bert.cpp:423-443, 684-750); so does this one: nothing thrown inside (a
// bad_alloc of the host repack, a std::system_error starting a worker thread)
// leaves the C ABI, and every partly built replica is released on the way out.
// All HIP calls of the load run on this thread, one replica after another; the
// weight uploads still overlap (async copies from one page-locked image on each
// replica's stream).  DESIGN §11 has the round-5 abort this replaces.
// act_mode: 0 (f16 activations) or 1 (the reference's q8 activations, bert_hip.h).
static bert_ctx *load_context(const char *fname, int act_mode)
{
    if (act_mode != 0 && act_mode != 1) {
        emb::errorf("bertx_load_from_file: act_mode %d is not an activation mode (0 = f16, 1 = q8)\n", act_mode);
        return nullptr;
    }
    emb::infof("bert_load_from_file: loading model from '%s' - please wait ...\n", fname);
    if (emb::fault_inject("load")) throw std::runtime_error("BERT_FAULT_INJECT=load");
    emb::HostModel m;
    std::string err;
    if (!emb::load_model_file(fname, m, err, true)) {
        emb::errorf("bert_load_from_file: %s\n", err.c_str());
        return nullptr;
    }
    // declared before ctx: on a failure the replicas (ctx) are released first, and
    // each waits for its upload from the page-locked image before the image goes
    emb::ModelImage img;
    std::unique_ptr<bert_ctx> ctx(new bert_ctx);
    ctx->hp = m.hp;
    ctx->vocab.build(m.vocab);
    ctx->act_mode = emb::act_mode_effective(m.hp.ftype, act_mode);
    ctx->n_labels = m.n_labels;
    ctx->proj_dim = m.proj_dim;
    if (act_mode == 1 && ctx->act_mode == 0)
        emb::infof("bert_load_from_file: q8 activations asked for a file of ftype %d: the reference has no q8 "
                   "arithmetic for f16 / f32 files, running the default mode\n", m.hp.ftype);
    const char *ho = std::getenv("BERT_HOST_ONLY");
    const bool host_only = ho && *ho && std::strcmp(ho, "0") != 0;
    if (host_only) {
        ctx->host_only = true;
        emb::infof("bert_load_from_file: host-only context (tokenizer only, no forward)\n");
        return ctx.release();
    }
    const std::vector<int> devs = parse_device_list(emb::hip_device_count());
    // the host half of the load, once for all replicas: repack into one image
    if (!emb::build_model_image(m, img, err, !devs.empty(), ctx->act_mode)) {
        emb::errorf("bert_load_from_file: %s\n", err.c_str());
        return nullptr;
    }
    emb::trace("bert_load_from_file: '%s': image %zu bytes (%s), %zu replica(s)\n", fname, img.total,
               img.pinned() ? "page-locked" : "pageable", devs.size());
    { emb::HostModel none; std::swap(m.layers, none.layers); }   // the file tensors are no longer needed
    if (devs.empty()) {
        emb::errorf("bert_load_from_file: no HIP (gfx950) device available -- libbert.so has no CPU "
                    "compute path (set BERT_HOST_ONLY=1 for a tokenizer-only context)\n");
        return nullptr;
    }
    ctx->devices.reserve(devs.size());
    for (size_t i = 0; i < devs.size(); ++i) {
        if (devs.size() > 1) emb::trace("bert_load_from_file: replica %zu on device %d: create + upload\n", i, devs[i]);
        if (i == 1 && emb::fault_inject("replica1")) throw std::runtime_error("BERT_FAULT_INJECT=replica1");
        std::unique_ptr<Device> d(new Device(devs[i], img));   // owned before anything else can throw
        ctx->devices.push_back(std::move(d));
    }
    bool ok = true;
    for (auto &d : ctx->devices) {
        if (!d->finish_load()) {
            emb::errorf("bert_load_from_file: device %d initialisation failed\n", d->ordinal());
            ok = false;
        }
    }
    if (!ok) return nullptr;
    emb::trace("bert_load_from_file: %zu replica(s) uploaded\n", ctx->devices.size());
    ctx->inflight.assign(ctx->devices.size(), 0.0);
    if (ctx->devices.size() > 1) {
        if (emb::fault_inject("worker")) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again), "BERT_FAULT_INJECT=worker");
        ctx->workers.reserve(ctx->devices.size());
        for (size_t i = 0; i < ctx->devices.size(); ++i) {
            std::unique_ptr<ReplicaWorker> w(new ReplicaWorker());   // joined by its destructor on any unwind
            ctx->workers.push_back(std::move(w));
        }
    }
    emb::infof("bert_load_from_file: MI355X engine on %zu HIP device(s)\n", ctx->devices.size());
    if (m.hp.ftype == emb::FMT_F32)
        emb::infof("bert_load_from_file: f32 file: f32 activations x f32 weights on the f32 MFMA chain "
                   "(as the reference multiplies them, bert.cpp:499-503)\n");
    if (ctx->act_mode == 1)
        emb::infof("bert_load_from_file: q8 activations: every projection re-quantizes its input per 32-block and "
                   "takes integer block dots (as the reference, bert.cpp:995)\n");
    return ctx.release();
}

static bert_ctx *load_guarded(const char *fname, int act_mode)
{
    // the initial pooling mode, BERT_POOL=mean|cls, read at every load (unset: mean)
    const char *ep = std::getenv("BERT_POOL");
    int pool = BERTX_POOL_MEAN;
    if (ep && *ep && std::strcmp(ep, "mean") != 0) {
        if (std::strcmp(ep, "cls") != 0) {
            emb::errorf("bert_load_from_file: BERT_POOL='%s' is not a pooling mode (mean or cls)\n", ep);
            return nullptr;
        }
        pool = BERTX_POOL_CLS;
    }
    // whether ColBERT queries keep their [MASK] rows as keys, BERT_MASK_KEYS=0|1 (unset: 1)
    const char *em = std::getenv("BERT_MASK_KEYS");
    int mask_keys = 1;
    if (em && *em) {
        if (std::strcmp(em, "0") != 0 && std::strcmp(em, "1") != 0) {
            emb::errorf("bert_load_from_file: BERT_MASK_KEYS='%s' is not 0 or 1\n", em);
            return nullptr;
        }
        mask_keys = em[0] - '0';
    }
    try {
        bert_ctx *ctx = load_context(fname, act_mode);
        if (ctx && pool != BERTX_POOL_MEAN) bertx_set_pooling(ctx, pool);
        if (ctx) bertx_set_mask_keys(ctx, mask_keys);
        return ctx;
    } catch (const std::bad_alloc &) {
        emb::errorf("bert_load_from_file: out of host memory\n");
    } catch (const std::exception &ex) {
        emb::errorf("bert_load_from_file: load failed: %s\n", ex.what());
    } catch (...) {
        emb::errorf("bert_load_from_file: load failed\n");
    }
    return nullptr;
}

// The reference's entry point has no mode argument: its unmodified clients choose
// with the environment, BERT_ACT=f16|q8, read at every load (unset: f16).
struct bert_ctx *bert_load_from_file(const char *fname)
{
    const char *ea = std::getenv("BERT_ACT");
    int act_mode = 0;
    if (ea && *ea && std::strcmp(ea, "f16") != 0) {
        if (std::strcmp(ea, "q8") != 0) {
            emb::errorf("bert_load_from_file: BERT_ACT='%s' is not an activation mode (f16 or q8)\n", ea);
            return nullptr;
        }
        act_mode = 1;
    }
    return load_guarded(fname, act_mode);
}

struct bert_ctx *bertx_load_from_file(const char *fname, int32_t act_mode) { return load_guarded(fname, act_mode); }

int32_t bertx_activation_mode(struct bert_ctx *ctx) { return ctx->act_mode; }

void bert_free(bert_ctx *ctx) { delete ctx; }

int32_t bert_n_embd(bert_ctx *ctx) { return ctx->hp.n_embd; }
int32_t bert_n_max_tokens(bert_ctx *ctx) { return ctx->hp.n_max_tokens; }
const char *bert_vocab_id_to_token(bert_ctx *ctx, bert_vocab_id id) { return ctx->vocab.id_to_token(id); }

void bert_tokenize(struct bert_ctx *ctx, const char *text, bert_vocab_id *tokens, int32_t *n_tokens,
                   int32_t n_max_tokens)
{
    *n_tokens = ctx->vocab.tokenize(text, n_max_tokens, tokens, n_max_tokens > 0 ? n_max_tokens : 0);
}

void bert_forward_batch(bert_ctx *ctx, int32_t n_threads, int32_t n_batch_size, bert_vocab_id **batch_tokens,
                        int32_t *n_tokens, float **batch_embeddings)
{
    (void)n_threads;
    if (!batch_embeddings || n_batch_size <= 0) return;   // reference memory-measurement mode: no output
    int32_t mx = 0;
    for (int i = 0; i < n_batch_size; ++i) mx = std::max(mx, n_tokens[i]);
    if (mx > ctx->hp.n_max_tokens) {
        emb::errorf("Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens);
        return;
    }
    run_forward(ctx, batch_tokens, n_tokens, batch_embeddings, n_batch_size);
}

void bert_forward(struct bert_ctx *ctx, int32_t n_threads, bert_vocab_id *tokens, int32_t n_tokens, float *embeddings)
{
    bert_forward_batch(ctx, n_threads, 1, &tokens, &n_tokens, embeddings ? &embeddings : nullptr);
}

void bert_forward_fake_batch(bert_ctx *ctx, int32_t n_threads, int32_t n_batch_size, bert_vocab_id **batch_tokens,
                             int32_t *n_tokens, float **batch_embeddings)
{
    (void)n_threads;
    std::printf("using function bert_forward_fake_batch\n");
    if (!batch_embeddings || n_batch_size <= 0) return;
    // the reference stops at the first over-long input, after writing the ones before it
    int n_ok = 0;
    while (n_ok < n_batch_size && n_tokens[n_ok] <= ctx->hp.n_max_tokens) ++n_ok;
    run_forward(ctx, batch_tokens, n_tokens, batch_embeddings, n_ok);
    if (n_ok < n_batch_size) emb::errorf("Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens);
}

void bert_encode_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_batch_size, int32_t n_inputs,
                       const char **texts, float **embeddings)
{
    if (n_inputs <= 0) return;
    const int32_t N = ctx->hp.n_max_tokens;
    std::vector<int32_t> ids((size_t)n_inputs * N);
    std::vector<int32_t> lens((size_t)n_inputs);
    if (!tokenize_all(ctx, n_threads > 0 ? n_threads : 1, n_inputs, texts, N, ids.data(), lens.data())) return;
    // which inputs the reference's chunking refuses (bert.cpp:1408-1443)
    std::vector<char> ok((size_t)n_inputs, 1);
    if (n_batch_size == n_inputs || n_batch_size <= 0) {
        if (*std::max_element(lens.begin(), lens.end()) > N) {
            emb::errorf("Too many tokens, maximum is %d\n", N);
            return;
        }
    } else {
        std::vector<int> idx((size_t)n_inputs);
        std::iota(idx.begin(), idx.end(), 0);
        std::sort(idx.begin(), idx.end(), [&](int a, int b) { return lens[(size_t)a] < lens[(size_t)b]; });
        for (int s = 0; s < n_inputs; s += n_batch_size) {
            const int e = std::min(n_inputs, s + n_batch_size);
            if (lens[(size_t)idx[(size_t)e - 1]] > N) {
                emb::errorf("Too many tokens, maximum is %d\n", N);
                for (int j = s; j < e; ++j) ok[(size_t)idx[(size_t)j]] = 0;
            }
        }
    }
    std::vector<const int32_t *> tp;
    std::vector<int32_t> lp;
    std::vector<float *> op;
    for (int i = 0; i < n_inputs; ++i) {
        if (!ok[(size_t)i]) continue;
        tp.push_back(ids.data() + (size_t)i * N);
        lp.push_back(lens[(size_t)i]);
        op.push_back(embeddings[i]);
    }
    run_forward(ctx, tp.data(), lp.data(), op.data(), (int)tp.size());
}

void bert_encode(struct bert_ctx *ctx, int32_t n_threads, const char *texts, float *embeddings)
{
    bert_encode_batch(ctx, n_threads, 1, 1, &texts, &embeddings);
}

// ---------------------------------------------------------------------------
// bert_hip.h
// ---------------------------------------------------------------------------

int32_t bertx_num_devices(struct bert_ctx *ctx) { return (int32_t)ctx->devices.size(); }

int32_t bertx_device_ordinal(struct bert_ctx *ctx, int32_t slot)
{
    return (slot >= 0 && slot < (int32_t)ctx->devices.size()) ? ctx->devices[(size_t)slot]->ordinal() : -1;
}

void bertx_hparams(struct bert_ctx *ctx, int32_t *o)
{
    o[0] = ctx->hp.n_vocab; o[1] = ctx->hp.n_max_tokens; o[2] = ctx->hp.n_embd; o[3] = ctx->hp.n_intermediate;
    o[4] = ctx->hp.n_head; o[5] = ctx->hp.n_layer; o[6] = ctx->hp.ftype;
}

int32_t bertx_reserve(struct bert_ctx *ctx, int32_t slot, int32_t total_tokens, int32_t n_seqs)
{
    if (slot < 0 || slot >= (int32_t)ctx->devices.size()) return -1;
    Device &D = *ctx->devices[(size_t)slot];
    std::lock_guard<std::mutex> lk(D.mutex());
    emb::DeviceGuard g(D.ordinal());
    return D.reserve(total_tokens, n_seqs, ctx->hp.n_max_tokens) ? 0 : -1;
}

int32_t bertx_forward_device(struct bert_ctx *ctx, int32_t slot, const int32_t *d_ids, const int32_t *d_cu,
                             int32_t n_seqs, int32_t max_len, int32_t total_tokens, float *d_out, void *stream)
{
    if (slot < 0 || slot >= (int32_t)ctx->devices.size()) return -1;
    if (max_len > ctx->hp.n_max_tokens || max_len <= 0) return -4;
    Device &D = *ctx->devices[(size_t)slot];
    std::lock_guard<std::mutex> lk(D.mutex());
    emb::DeviceGuard g(D.ordinal());
    return D.forward(d_ids, d_cu, n_seqs, max_len, total_tokens, d_out, stream ? (hipStream_t)stream : D.stream());
}

int32_t bertx_set_pooling(struct bert_ctx *ctx, int32_t pool)
{
    if (!ctx || (pool != BERTX_POOL_MEAN && pool != BERTX_POOL_CLS)) return -1;
    // under each replica's mutex: no forward of that replica is being launched; the
    // mode is part of a captured graph's key, so graphs of the other mode stay unreachable
    for (auto &d : ctx->devices) {
        std::lock_guard<std::mutex> lk(d->mutex());
        d->set_pooling(pool);
    }
    ctx->pool = pool;
    return 0;
}

int32_t bertx_pooling(struct bert_ctx *ctx) { return ctx ? ctx->pool : -1; }

int32_t bertx_set_mask_keys(struct bert_ctx *ctx, int32_t on)
{
    if (!ctx || (on != 0 && on != 1)) return -1;
    ctx->mask_keys.store(on);
    return 0;
}

int32_t bertx_mask_keys(struct bert_ctx *ctx) { return ctx ? ctx->mask_keys.load() : -1; }

int32_t bertx_set_cls_pruning(struct bert_ctx *ctx, int32_t on)
{
    if (!ctx) return -1;
    for (auto &d : ctx->devices) {
        std::lock_guard<std::mutex> lk(d->mutex());
        d->set_cls_pruning(on != 0);
    }
    return 0;
}

int32_t bertx_forward_tokens_device(struct bert_ctx *ctx, int32_t slot, const int32_t *d_ids, const int32_t *d_cu,
                                    int32_t n_seqs, int32_t max_len, int32_t total_tokens, float *d_out, void *stream)
{
    if (slot < 0 || slot >= (int32_t)ctx->devices.size()) return -1;
    if (max_len > ctx->hp.n_max_tokens || max_len <= 0) return -4;
    Device &D = *ctx->devices[(size_t)slot];
    std::lock_guard<std::mutex> lk(D.mutex());
    emb::DeviceGuard g(D.ordinal());
    return D.forward(d_ids, d_cu, n_seqs, max_len, total_tokens, d_out, stream ? (hipStream_t)stream : D.stream(), -1.0,
                     true);
}

// The per-token host forms: every token's final-LayerNorm row, or (proj) its projection.
// n_keys (or null): sentence i's key count, which travels with it into its chunk.
static int32_t forward_rows(struct bert_ctx *ctx, int32_t n, bert_vocab_id **batch_tokens, int32_t *n_tokens,
                            float **out, bool proj, const int32_t *n_keys = nullptr)
{
    if (!ctx || n < 0 || (n > 0 && (!batch_tokens || !n_tokens || !out))) return -1;
    if (proj && ctx->proj_dim <= 0) {
        emb::errorf("libbert: this model file has no projection (linear.weight)\n");
        return -6;
    }
    if (ctx->devices.empty()) {
        emb::errorf("libbert: no HIP device in this context (BERT_HOST_ONLY); forward unavailable\n");
        return -1;
    }
    for (int i = 0; i < n; ++i) {
        if (n_tokens[i] > ctx->hp.n_max_tokens) {
            emb::errorf("Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens);
            return -4;
        }
        if (n_tokens[i] <= 0) return -1;
        if (n_keys && (n_keys[i] < 1 || n_keys[i] > n_tokens[i])) return -1;   // before any output is written
    }
    if (n == 0) return 0;
    // the whole call on the least-loaded replica, in chunks the workspace holds
    int dv = 0;
    double cost = 0.0;
    for (int i = 0; i < n; ++i) cost += sentence_cost(ctx->hp, n_tokens[i]);
    {
        std::lock_guard<std::mutex> lk(ctx->route_mu);
        for (int i = 1; i < (int)ctx->devices.size(); ++i)
            if (ctx->inflight[(size_t)i] < ctx->inflight[(size_t)dv]) dv = i;
        ctx->inflight[(size_t)dv] += cost;
    }
    int rc = 0;
    try {
        Device &D = *ctx->devices[(size_t)dv];
        std::lock_guard<std::mutex> lk(D.mutex());
        std::vector<const int32_t *> tp;
        std::vector<int32_t> lp, kp;
        std::vector<float *> op;
        int i = 0;
        while (i < n && rc == 0) {
            tp.clear(); lp.clear(); op.clear(); kp.clear();
            for (const int e = (int)emb::chunk_end([&](size_t j) { return n_tokens[j]; }, (size_t)i, (size_t)n); i < e; ++i) {
                tp.push_back(batch_tokens[i]); lp.push_back(n_tokens[i]); op.push_back(out[i]);
                if (n_keys) kp.push_back(n_keys[i]);
            }
            rc = D.forward_host(tp.data(), lp.data(), (int)tp.size(), op.data(), true, nullptr, false, proj,
                                n_keys ? kp.data() : nullptr);
        }
    } catch (...) {
        rc = -1;
    }
    {
        std::lock_guard<std::mutex> lk(ctx->route_mu);
        ctx->inflight[(size_t)dv] -= cost;
        if (ctx->inflight[(size_t)dv] < 0.5) ctx->inflight[(size_t)dv] = 0.0;
    }
    if (rc != 0) emb::errorf("libbert: forward failed (%d)\n", rc);
    return rc;
}

int32_t bertx_forward_tokens(struct bert_ctx *ctx, int32_t n, bert_vocab_id **batch_tokens, int32_t *n_tokens,
                             float **out)
{
    return forward_rows(ctx, n, batch_tokens, n_tokens, out, false);
}

int32_t bertx_forward_project(struct bert_ctx *ctx, int32_t n, bert_vocab_id **batch_tokens, int32_t *n_tokens,
                              float **out)
{
    return forward_rows(ctx, n, batch_tokens, n_tokens, out, true);
}

int32_t bertx_forward_tokens_kv(struct bert_ctx *ctx, int32_t n, bert_vocab_id **batch_tokens, int32_t *n_tokens,
                                const int32_t *n_keys, float **out)
{
    return forward_rows(ctx, n, batch_tokens, n_tokens, out, false, n_keys);
}

int32_t bertx_forward_project_kv(struct bert_ctx *ctx, int32_t n, bert_vocab_id **batch_tokens, int32_t *n_tokens,
                                 const int32_t *n_keys, float **out)
{
    return forward_rows(ctx, n, batch_tokens, n_tokens, out, true, n_keys);
}

int32_t bertx_proj_dim(struct bert_ctx *ctx) { return ctx ? ctx->proj_dim : 0; }
int32_t bertx_proj_width(struct bert_ctx *ctx) { return ctx ? emb::proj_width_of(ctx->proj_dim) : 0; }

int32_t bertx_forward_project_device(struct bert_ctx *ctx, int32_t slot, const int32_t *d_ids, const int32_t *d_types,
                                     const int32_t *d_cu, int32_t n_seqs, int32_t max_len, int32_t total_tokens,
                                     const int32_t *d_rows, int32_t n_rows, float *d_out, void *stream)
{
    if (!ctx || slot < 0 || slot >= (int32_t)ctx->devices.size() || (d_rows && n_rows < 0)) return -1;
    if (ctx->proj_dim <= 0) return -6;
    if (max_len > ctx->hp.n_max_tokens || max_len <= 0) return -4;
    Device &D = *ctx->devices[(size_t)slot];
    std::lock_guard<std::mutex> lk(D.mutex());
    emb::DeviceGuard g(D.ordinal());
    return D.forward_ex(d_ids, d_types, d_cu, n_seqs, max_len, total_tokens, Device::KIND_PROJ, d_out,
                        stream ? (hipStream_t)stream : D.stream(), -1.0, d_rows, n_rows);
}

int32_t bertx_tokenize_colbert(struct bert_ctx *ctx, const char *text, int32_t kind, int32_t maxlen, bert_vocab_id *ids,
                               int32_t *keep, int32_t *n_tokens)
{
    int32_t n_keys = 0;
    return bertx_tokenize_colbert_ex(ctx, text, kind, maxlen, ids, keep, n_tokens, &n_keys);
}

int32_t bertx_tokenize_colbert_ex(struct bert_ctx *ctx, const char *text, int32_t kind, int32_t maxlen,
                                  bert_vocab_id *ids, int32_t *keep, int32_t *n_tokens, int32_t *n_keys)
{
    if (!ctx || !text || !ids || !keep || !n_tokens || !n_keys || (kind != 0 && kind != 1)) return -1;
    if (maxlen < 4 || maxlen > ctx->hp.n_max_tokens) return -1;
    try {
        thread_local std::vector<int32_t> p;
        ctx->vocab.pieces(text, p);
        const int32_t t = ctx->vocab.colbert_layout(p.data(), (int32_t)p.size(), kind, maxlen, ids, keep);
        if (t < 0) return -1;
        *n_tokens = t;
        // a query's rows up to and including [SEP]; the [MASK] rows behind it are not counted
        *n_keys = kind == 0 ? 3 + std::min<int32_t>((int32_t)p.size(), maxlen - 3) : t;
        return 0;
    } catch (...) {
        emb::errorf("libbert: tokenization failed\n");
        return -1;
    }
}

int32_t bertx_convert_hf_colbert(const char *dir_model, const char *fname_out, int32_t ftype)
{
    return emb::convert_hf_dir(dir_model, fname_out, ftype, false, true);
}

void bertx_set_profiling(struct bert_ctx *ctx, int32_t on)
{
    for (auto &d : ctx->devices) d->set_profiling(on != 0);
}

void bertx_reset_stats(struct bert_ctx *ctx)
{
    for (auto &d : ctx->devices) d->reset_stats();
}

int32_t bertx_kernel_stats(struct bert_ctx *ctx, int32_t idx, const char **name, int64_t *launches, double *total_ms,
                           double *work, int32_t *work_is_flops)
{
    if (idx < 0 || idx >= emb::K_NUM_CLASSES) return -1;
    int64_t l = 0;
    double ms = 0, w = 0;
    for (auto &d : ctx->devices) {
        d->collect_stats();
        l += d->stats(idx).launches;
        ms += d->stats(idx).ms;
        w += d->stats(idx).work;
    }
    if (name) *name = emb::kclass_name(idx);
    if (launches) *launches = l;
    if (total_ms) *total_ms = ms;
    if (work) *work = w;
    if (work_is_flops)
        *work_is_flops = (idx == emb::K_EMBED_LN || idx == emb::K_LN_STATS || idx == emb::K_POOL_L2) ? 0 : 1;
    return 0;
}

int32_t bertx_device_last_call(struct bert_ctx *ctx, int32_t slot, double *wall_ms, int32_t *n_seqs,
                               int64_t *n_tokens)
{
    if (!ctx || slot < 0 || slot >= (int32_t)ctx->devices.size()) return -1;
    Device &D = *ctx->devices[(size_t)slot];
    std::lock_guard<std::mutex> lk(D.mutex());   // the stamps are written under it (run_forward)
    if (wall_ms) *wall_ms = D.last_call_ms();
    if (n_seqs) *n_seqs = D.last_call_seqs();
    if (n_tokens) *n_tokens = D.last_call_tokens();
    return 0;
}

int64_t bertx_device_calls(struct bert_ctx *ctx, int32_t slot)
{
    if (!ctx || slot < 0 || slot >= (int32_t)ctx->devices.size()) return -1;
    Device &D = *ctx->devices[(size_t)slot];
    std::lock_guard<std::mutex> lk(D.mutex());
    return D.calls();
}

int32_t bertx_quantize_file(const char *fin, const char *fout, int32_t itype)
{
    return emb::quantize_file(fin, fout, itype, false);
}

int32_t bertx_convert_hf(const char *dir_model, const char *fname_out, int32_t ftype)
{
    return emb::convert_hf_dir(dir_model, fname_out, ftype);
}

int32_t bertx_convert_hf_head(const char *dir_model, const char *fname_out, int32_t ftype)
{
    return emb::convert_hf_dir(dir_model, fname_out, ftype, true);
}

int32_t bertx_n_labels(struct bert_ctx *ctx) { return ctx ? ctx->n_labels : 0; }

int32_t bertx_forward_device_ex(struct bert_ctx *ctx, int32_t slot, const int32_t *d_ids, const int32_t *d_types,
                                const int32_t *d_cu, int32_t n_seqs, int32_t max_len, int32_t total_tokens,
                                int32_t out_kind, float *d_out, void *stream)
{
    if (slot < 0 || slot >= (int32_t)ctx->devices.size()) return -1;
    if (out_kind != BERTX_OUT_POOLED && out_kind != BERTX_OUT_TOKENS && out_kind != BERTX_OUT_LOGITS &&
        out_kind != BERTX_OUT_PROJ)
        return -1;
    if (out_kind == BERTX_OUT_LOGITS && ctx->n_labels <= 0) return -6;
    // (a file without the projection record has no fourth output kind: -1 as before the
    // record existed; the entries that exist only for the projection answer -6)
    if (out_kind == BERTX_OUT_PROJ && ctx->proj_dim <= 0) return -1;
    if (max_len > ctx->hp.n_max_tokens || max_len <= 0) return -4;
    Device &D = *ctx->devices[(size_t)slot];
    std::lock_guard<std::mutex> lk(D.mutex());
    emb::DeviceGuard g(D.ordinal());
    return D.forward_ex(d_ids, d_types, d_cu, n_seqs, max_len, total_tokens, out_kind, d_out,
                        stream ? (hipStream_t)stream : D.stream());
}

int32_t bertx_forward_device_kv(struct bert_ctx *ctx, int32_t slot, const int32_t *d_ids, const int32_t *d_types,
                                const int32_t *d_cu, const int32_t *d_keys, int32_t n_seqs, int32_t max_len,
                                int32_t total_tokens, int32_t out_kind, const int32_t *d_rows, int32_t n_rows,
                                float *d_out, void *stream)
{
    if (!ctx || slot < 0 || slot >= (int32_t)ctx->devices.size()) return -1;
    if (out_kind != BERTX_OUT_TOKENS && out_kind != BERTX_OUT_PROJ) return -1;
    const bool mapped = out_kind == BERTX_OUT_PROJ && d_rows != nullptr;
    if (mapped && n_rows < 0) return -1;
    if (out_kind == BERTX_OUT_PROJ && ctx->proj_dim <= 0) return -6;
    if (max_len > ctx->hp.n_max_tokens || max_len <= 0) return -4;
    Device &D = *ctx->devices[(size_t)slot];
    std::lock_guard<std::mutex> lk(D.mutex());
    emb::DeviceGuard g(D.ordinal());
    return D.forward_ex(d_ids, d_types, d_cu, n_seqs, max_len, total_tokens, out_kind, d_out,
                        stream ? (hipStream_t)stream : D.stream(), -1.0, mapped ? d_rows : nullptr, mapped ? n_rows : 0,
                        d_keys);
}

int32_t bertx_tokenize_pair(struct bert_ctx *ctx, const char *text_a, const char *text_b, int32_t truncate,
                            bert_vocab_id *ids, int32_t *types, int32_t *n_tokens, int32_t n_max)
{
    if (!ctx || !text_a || !text_b || !ids || !types || !n_tokens || n_max < 3) return -1;
    try {
        thread_local std::vector<int32_t> pa, pb;
        ctx->vocab.pieces(text_a, pa);
        ctx->vocab.pieces(text_b, pb);
        const int32_t rc = emb::Vocab::pair_layout(pa.data(), (int32_t)pa.size(), pb.data(), (int32_t)pb.size(),
                                                   truncate != 0, n_max, ids, types, n_tokens);
        if (rc == -4) emb::errorf("Too many tokens, maximum is %d\n", n_max);
        return rc;
    } catch (...) {
        emb::errorf("libbert: tokenization failed\n");
        return -1;
    }
}

// The refusals the three scoring entries share, before any work: -1 bad arguments, -6
// a file without a head, -1 (after the usual message) a tokenizer-only context.
static int32_t score_refusal(struct bert_ctx *ctx, int32_t n, bool ptrs_ok, const float *logits)
{
    if (!ctx || n < 0 || (n > 0 && (!ptrs_ok || !logits))) return -1;
    if (ctx->n_labels <= 0) {
        emb::errorf("libbert: this model file has no classification head (pooler.dense.* + classifier.*)\n");
        return -6;
    }
    if (ctx->devices.empty()) {
        emb::errorf("libbert: no HIP device in this context (BERT_HOST_ONLY); forward unavailable\n");
        return -1;
    }
    return 0;
}

int32_t bertx_score_ids(struct bert_ctx *ctx, int32_t n, bert_vocab_id **ids, int32_t **types, int32_t *n_tokens,
                        float *logits)
{
    if (const int32_t rc = score_refusal(ctx, n, ids && types && n_tokens, logits)) return rc;
    for (int i = 0; i < n; ++i) {
        if (n_tokens[i] > ctx->hp.n_max_tokens) {
            emb::errorf("Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens);
            return -4;
        }
        if (n_tokens[i] <= 0 || !ids[i] || !types[i]) return -1;
        for (int t = 0; t < n_tokens[i]; ++t)
            if (types[i][t] != 0 && types[i][t] != 1) {
                emb::errorf("libbert: token type %d of input %d is not 0 or 1\n", types[i][t], i);
                return -1;
            }
    }
    if (n == 0) return 0;
    try {
        // results in staging rows first: a failed call leaves the caller's logits untouched
        const size_t nl = (size_t)ctx->n_labels;
        std::vector<float> stage((size_t)n * nl);
        std::vector<float *> op((size_t)n);
        for (int i = 0; i < n; ++i) op[(size_t)i] = stage.data() + nl * (size_t)i;
        const int rc = run_forward(ctx, ids, n_tokens, op.data(), n, types, true);
        if (rc != 0) return rc;
        std::memcpy(logits, stage.data(), stage.size() * sizeof(float));
        return 0;
    } catch (...) {
        emb::errorf("libbert: scoring failed\n");
        return -1;
    }
}

// n pairs: texts_a[i] (or the one query's pieces, tokenised once) against texts_b[i]
static int32_t score_texts(struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char *query,
                           const char *const *texts_a, const char *const *texts_b, int32_t truncate, float *logits)
{
    if (n == 0) return 0;
    try {
        const int32_t N = ctx->hp.n_max_tokens;
        std::vector<int32_t> ids((size_t)n * N), types((size_t)n * N), lens((size_t)n), rcs((size_t)n, 0), qp;
        if (query) ctx->vocab.pieces(query, qp);
        emb::TaskPool::instance().run(((int64_t)n + 7) / 8, n_threads > 0 ? n_threads : 1, [&](int64_t blk) {
            thread_local std::vector<int32_t> pa, pb;
            const int e = (int)std::min<int64_t>(n, 8 * blk + 8);
            for (int i = (int)(8 * blk); i < e; ++i) {
                if (!query) ctx->vocab.pieces(texts_a[i], pa);
                ctx->vocab.pieces(texts_b[i], pb);
                const std::vector<int32_t> &A = query ? qp : pa;
                rcs[(size_t)i] = emb::Vocab::pair_layout(A.data(), (int32_t)A.size(), pb.data(), (int32_t)pb.size(),
                                                         truncate != 0, N, ids.data() + (size_t)i * N,
                                                         types.data() + (size_t)i * N, &lens[(size_t)i]);
            }
        });
        for (int i = 0; i < n; ++i)
            if (rcs[(size_t)i] != 0) {
                if (rcs[(size_t)i] == -4) emb::errorf("Too many tokens, maximum is %d\n", N);
                return rcs[(size_t)i];
            }
        std::vector<int32_t *> ip((size_t)n), tp((size_t)n);
        for (int i = 0; i < n; ++i) {
            ip[(size_t)i] = ids.data() + (size_t)i * N;
            tp[(size_t)i] = types.data() + (size_t)i * N;
        }
        return bertx_score_ids(ctx, n, ip.data(), tp.data(), lens.data(), logits);
    } catch (const std::exception &ex) {
        emb::errorf("libbert: tokenization failed: %s\n", ex.what());
    } catch (...) {
        emb::errorf("libbert: tokenization failed\n");
    }
    return -1;
}

int32_t bertx_score_pairs(struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts_a,
                          const char **texts_b, int32_t truncate, float *logits)
{
    if (const int32_t rc = score_refusal(ctx, n, texts_a && texts_b, logits)) return rc;
    for (int i = 0; i < n; ++i)
        if (!texts_a[i] || !texts_b[i]) return -1;
    return score_texts(ctx, n_threads, n, nullptr, texts_a, texts_b, truncate, logits);
}

int32_t bertx_rerank(struct bert_ctx *ctx, int32_t n_threads, const char *query, int32_t n_docs, const char **docs,
                     int32_t truncate, float *logits)
{
    if (const int32_t rc = score_refusal(ctx, n_docs, query && docs, logits)) return rc;
    for (int i = 0; i < n_docs; ++i)
        if (!docs[i]) return -1;
    return score_texts(ctx, n_threads, n_docs, query, nullptr, docs, truncate, logits);
}

int32_t bertx_tokenize_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts,
                             int32_t n_max, int32_t *ids, int32_t *n_tokens)
{
    if (!ctx || n_inputs < 0 || n_max <= 0 || (n_inputs > 0 && (!texts || !ids || !n_tokens))) return -1;
    return tokenize_all(ctx, n_threads > 0 ? n_threads : 1, n_inputs, texts, n_max, ids, n_tokens) ? 0 : -1;
}

const char *bertx_version(void) { return "embeddings.cpp_amd 0.1 (gfx950)"; }

}  // extern "C"
