// The token store of late interaction (bert_hip.h bertx_mvindex_*): an append-only set
// of documents, each a run of unit-length token rows in the search kernel's fragment
// order, f16 (kernels.h, maxsim.hip) or int8 with one f32 per token slot (maxsim_i8.hip),
// the fused MaxSim scorer over it, and the text forms on top of the per-token forward.
// After creation a store knows only its device ordinal, its width and its storage kind.
// The ordering rules are the embedding index's (index.cpp).
#include "bert.h"
#include "bert_hip.h"

#include "engine.h"
#include "hip_check.h"
#include "task_pool.h"

#include <algorithm>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <vector>

struct bertx_mvindex {
    int ordinal = 0;
    int w = 0;
    int storage = BERTX_INDEX_F16;
    int64_t cap_docs = 0, cap_slots = 0;   // as given at creation
    int64_t n_docs = 0, used_slots = 0;    // used_slots: whole groups, 16 per group
    void *store = nullptr;                 // f16 or int8, ceil(cap_slots / 16) groups in fragment order
    float *scales = nullptr;               // int8: one f32 per token slot
    int32_t *table = nullptr;              // device: (first group, len) per document
    int32_t *src_off = nullptr;            // device: per document, its first source row in the add call that brought it
    // page-locked host images of both, written per add at the new documents' own entries
    // (an entry is rewritten only after a clear, which waits for the device first)
    int32_t *h_table = nullptr, *h_src = nullptr;
    // staging of the host forms
    float *st_rows = nullptr, *st_q = nullptr, *st_out = nullptr;
    int32_t *st_ids = nullptr, *st_tok = nullptr;
    void *search_scratch = nullptr;        // the partial lists of the full-scan search (maxsim_search_scratch_bytes)
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;             // completion of the last device operation on the store
    hipStream_t last_stream = nullptr;
    bool any = false;
    std::mutex mu;
    ~bertx_mvindex()
    {
        emb::DeviceGuard g(ordinal);
        if (stream) (void)hipStreamSynchronize(stream);
        if (any && done) (void)hipEventSynchronize(done);
        for (void *p : {store, (void *)scales, (void *)table, (void *)src_off, (void *)st_rows, (void *)st_q, (void *)st_out,
                        (void *)st_ids, (void *)st_tok, search_scratch})
            if (p) (void)hipFree(p);
        if (h_table) (void)hipHostFree(h_table);
        if (h_src) (void)hipHostFree(h_src);
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace emb {
namespace {

constexpr int kStageRows = 2048;    // token rows per staged chunk of the host add
constexpr int kStageIds = 65536;    // candidates per staged chunk of the host score
constexpr int kMaxLq = 64;
constexpr int kMaxK = 128;
constexpr int kSearchTexts = 1024;  // queries per forward of the search text forms (at most 2^16 tokens)
constexpr int64_t kChunkTokens = 1 << 17;   // per device forward of add_texts, as run_forward chunks
constexpr int kChunkSeqs = 4096;

bool capturing(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

// Orders an operation on `s` after the store's previous one and records it as the new
// previous one (index.cpp Ordered; a capturing stream waits for and records nothing).
struct Ordered {
    bertx_mvindex &mv;
    hipStream_t s;
    const bool cap;
    Ordered(bertx_mvindex &m, hipStream_t st) : mv(m), s(st), cap(capturing(st))
    {
        if (!cap && mv.any && mv.last_stream != s) (void)hipStreamWaitEvent(s, mv.done, 0);
    }
    ~Ordered()
    {
        if (cap) return;
        (void)hipEventRecord(mv.done, s);
        mv.last_stream = s;
        mv.any = true;
    }
};

// The first half of an add: checks the lens and both capacities and writes the new
// documents' entries into the host images.  Returns 0 with *T the source rows and
// *slots the slots they take; -1 / -2 as bertx_mvindex_add.
int32_t plan_add(bertx_mvindex &mv, const int32_t *lens, int32_t n, int64_t *T, int64_t *slots)
{
    if (!lens || n < 1) return -1;
    int64_t t = 0, g = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (lens[i] < 1) {
            errorf("bertx_mvindex_add: document %d has %d tokens\n", i, lens[i]);
            return -1;
        }
        t += lens[i];
        g += (lens[i] + 15) / 16;
    }
    if (mv.n_docs + n > mv.cap_docs || mv.used_slots + 16 * g > mv.cap_slots) {
        errorf("bertx_mvindex_add: %d documents of %lld token slots do not fit (%lld of %lld documents, %lld of %lld "
               "slots used)\n", n, (long long)(16 * g), (long long)mv.n_docs, (long long)mv.cap_docs,
               (long long)mv.used_slots, (long long)mv.cap_slots);
        return -2;
    }
    if (t > 0x7fffffffll) return -1;   // source rows are indexed in int32 (src_off)
    int64_t grp = mv.used_slots / 16, off = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t id = mv.n_docs + i;
        mv.h_table[2 * id] = (int32_t)grp;
        mv.h_table[2 * id + 1] = lens[i];
        mv.h_src[id] = (int32_t)off;
        grp += (lens[i] + 15) / 16;
        off += lens[i];
    }
    *T = t;
    *slots = 16 * g;
    return 0;
}

// The new documents' entries to the device (asynchronous, from page-locked memory).
int32_t upload_entries(bertx_mvindex &mv, int32_t n, hipStream_t s)
{
    const int64_t id = mv.n_docs;
    HIP_RC(hipMemcpyAsync(mv.table + 2 * id, mv.h_table + 2 * id, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_RC(hipMemcpyAsync(mv.src_off + id, mv.h_src + id, (size_t)n * 4, hipMemcpyHostToDevice, s));
    return 0;
}

int32_t pack(bertx_mvindex &mv, const float *d_rows, int64_t t0, int64_t count, int32_t n, hipStream_t s)
{
    if (mv.storage == BERTX_INDEX_I8)
        return launch_mv_pack_i8(d_rows, t0, count, mv.w, mv.src_off + mv.n_docs, mv.table + 2 * mv.n_docs, n, mv.store,
                                 mv.scales, s);
    return launch_mv_pack(d_rows, t0, count, mv.w, mv.src_off + mv.n_docs, mv.table + 2 * mv.n_docs, n, mv.store, s);
}

int32_t commit(bertx_mvindex &mv, int32_t n, int64_t slots)
{
    const int32_t first = (int32_t)mv.n_docs;
    mv.n_docs += n;
    mv.used_slots += slots;
    return first;
}

int32_t add_device_locked(bertx_mvindex &mv, const float *d_rows, const int32_t *lens, int32_t n, hipStream_t s)
{
    if (!d_rows) return -1;
    int64_t T = 0, slots = 0;
    int32_t rc = plan_add(mv, lens, n, &T, &slots);
    if (rc != 0) return rc;
    {
        Ordered o(mv, s);
        rc = upload_entries(mv, n, s);
        if (rc == 0) rc = pack(mv, d_rows, 0, T, n, s);
    }
    if (rc != 0) {
        (void)hipStreamSynchronize(s);   // the entries may be rewritten by the next add
        return rc;
    }
    return commit(mv, n, slots);
}

int32_t score_device_locked(bertx_mvindex &mv, const float *d_q, int32_t Lq, const int32_t *d_ids, int32_t n,
                            float *d_out, hipStream_t s)
{
    if (!d_q || !d_out || Lq < 1 || Lq > kMaxLq || n < 1) return -1;
    Ordered o(mv, s);
    if (mv.storage == BERTX_INDEX_I8)
        return launch_maxsim_i8(mv.store, mv.scales, mv.table, (int)mv.n_docs, mv.w, d_q, Lq, d_ids, n, d_out, s);
    return launch_maxsim(mv.store, mv.table, (int)mv.n_docs, mv.w, d_q, Lq, d_ids, n, d_out, s);
}

bool search_args_ok(const char *who, int32_t B, int32_t Lq, int32_t k)
{
    if (B >= 1 && Lq >= 1 && Lq <= kMaxLq && k >= 1 && k <= kMaxK) return true;
    errorf("%s: B = %d, Lq = %d, k = %d are not in B >= 1, 1 <= Lq <= %d, 1 <= k <= %d\n", who, B, Lq, k, kMaxLq, kMaxK);
    return false;
}

int32_t search_device_locked(bertx_mvindex &mv, const float *d_q, int32_t B, int32_t Lq, int32_t k, float *d_scores,
                             int32_t *d_ids, hipStream_t s)
{
    if (!d_q || !d_scores || !d_ids || !search_args_ok("bertx_mvindex_search", B, Lq, k)) return -1;
    Ordered o(mv, s);
    return launch_maxsim_search(mv.store, mv.scales, mv.storage, mv.table, (int)mv.n_docs, mv.used_slots / 16, mv.w, d_q, B,
                                Lq, k, mv.search_scratch, d_scores, d_ids, s);
}

// The query already on the device (mv.st_q or a caller's buffer on the store's stream):
// scores of the host ids (or of all documents) into the host out, which is written
// only when every chunk succeeded.
int32_t score_host_ids(bertx_mvindex &mv, const float *d_q, int32_t Lq, const int32_t *ids, int32_t n, float *out)
{
    std::vector<float> hs((size_t)n);
    std::vector<int32_t> all;
    if (!ids) {
        all.resize((size_t)n);
        for (int32_t i = 0; i < n; ++i) all[(size_t)i] = i;
        ids = all.data();
    }
    for (int32_t i = 0; i < n; i += kStageIds) {
        const int32_t m = std::min(kStageIds, n - i);
        HIP_RC(hipMemcpyAsync(mv.st_ids, ids + i, (size_t)m * 4, hipMemcpyHostToDevice, mv.stream));
        const int32_t rc = score_device_locked(mv, d_q, Lq, mv.st_ids, m, mv.st_out, mv.stream);
        if (rc != 0) return rc;
        HIP_RC(hipMemcpyAsync(hs.data() + i, mv.st_out, (size_t)m * 4, hipMemcpyDeviceToHost, mv.stream));
        HIP_RC(hipStreamSynchronize(mv.stream));
    }
    std::memcpy(out, hs.data(), hs.size() * 4);
    return 0;
}

// The stored bytes q [len][w] and scales u [len] of document id of an int8 store (the
// caller holds the lock, has checked the id and has selected the device).
int32_t read_doc_i8(bertx_mvindex &mv, int32_t id, int8_t *q, float *u)
{
    const int w = mv.w, KB = w / 64;
    const int64_t first = mv.h_table[2 * (size_t)id], len = mv.h_table[2 * (size_t)id + 1];
    const size_t group_bytes = (size_t)16 * w, groups = (size_t)((len + 15) / 16);
    std::vector<int8_t> raw(groups * group_bytes);
    std::vector<float> us(groups * 16);
    if (mv.any) HIP_RC(hipEventSynchronize(mv.done));
    HIP_RC(hipMemcpy(raw.data(), (const int8_t *)mv.store + (size_t)first * group_bytes, raw.size(),
                     hipMemcpyDeviceToHost));
    HIP_RC(hipMemcpy(us.data(), mv.scales + (size_t)first * 16, us.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < len; ++r) {
        const int8_t *grp = raw.data() + (size_t)(r / 16) * group_bytes;
        for (int kb = 0; kb < KB; ++kb)
            for (int g = 0; g < 4; ++g)
                std::memcpy(q + (size_t)r * w + 64 * kb + 16 * g, grp + ((size_t)kb * 64 + 16 * g + (r & 15)) * 16, 16);
        u[r] = us[(size_t)r];
    }
    return 0;
}

// The context's replica on the store's GPU, or -1.
int32_t slot_on(struct bert_ctx *ctx, int ordinal)
{
    for (int32_t s = 0; s < bertx_num_devices(ctx); ++s)
        if (bertx_device_ordinal(ctx, s) == ordinal) return s;
    return -1;
}

int32_t text_ctx_ok(bertx_mvindex *mv, struct bert_ctx *ctx, const char *who, int32_t *slot)
{
    if (!mv || !ctx) return -1;
    if (bertx_num_devices(ctx) == 0 || bert_n_embd(ctx) != mv->w) {
        errorf("%s: the context cannot produce token rows of width %d\n", who, mv->w);
        return -1;
    }
    *slot = slot_on(ctx, mv->ordinal);
    if (*slot < 0) {
        errorf("%s: the context has no replica on the store's device %d\n", who, mv->ordinal);
        return -1;
    }
    return 0;
}

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// B queries f32 [B][Lq][w] already on the device, on the store's stream: their results
// into host vectors (the caller copies them out when the whole call succeeded).
int32_t search_to_host(bertx_mvindex &mv, const float *d_q, int32_t B, int32_t Lq, int32_t k, float *scores, int32_t *ids)
{
    DevBuf d_s, d_i;
    HIP_RC(hipMalloc(&d_s.p, (size_t)B * k * 4));
    HIP_RC(hipMalloc(&d_i.p, (size_t)B * k * 4));
    const int32_t rc = search_device_locked(mv, d_q, B, Lq, k, (float *)d_s.p, (int32_t *)d_i.p, mv.stream);
    if (rc != 0) {
        (void)hipStreamSynchronize(mv.stream);
        return rc;
    }
    HIP_RC(hipMemcpyAsync(scores, d_s.p, (size_t)B * k * 4, hipMemcpyDeviceToHost, mv.stream));
    HIP_RC(hipMemcpyAsync(ids, d_i.p, (size_t)B * k * 4, hipMemcpyDeviceToHost, mv.stream));
    HIP_RC(hipStreamSynchronize(mv.stream));
    return 0;
}

// The refusals of the ColBERT text forms: -6 a file without the projection record, -1 a
// store of another width than the projected rows', then as text_ctx_ok.
int32_t colbert_ctx_ok(bertx_mvindex *mv, struct bert_ctx *ctx, const char *who, int32_t *slot)
{
    if (!mv || !ctx) return -1;
    if (bertx_proj_dim(ctx) <= 0) {
        errorf("%s: this model file has no projection (linear.weight)\n", who);
        return -6;
    }
    if (bertx_num_devices(ctx) == 0 || bertx_proj_width(ctx) != mv->w) {
        errorf("%s: the context projects to rows of width %d, the store holds width %d\n", who, bertx_proj_width(ctx),
               mv->w);
        return -1;
    }
    *slot = slot_on(ctx, mv->ordinal);
    if (*slot < 0) {
        errorf("%s: the context has no replica on the store's device %d\n", who, mv->ordinal);
        return -1;
    }
    return 0;
}

}  // namespace

bertx_mvindex *mvindex_create_on(int ordinal, int w, int64_t cap_docs, int64_t cap_slots, int storage)
{
    if (storage != BERTX_INDEX_F16 && storage != BERTX_INDEX_I8) {
        errorf("bertx_mvindex_create: storage %d is neither BERTX_INDEX_F16 nor BERTX_INDEX_I8\n", storage);
        return nullptr;
    }
    if (w % 64 || w < 64 || w > 1024) {
        errorf("bertx_mvindex_create: width %d is not a multiple of 64 in 64 .. 1024\n", w);
        return nullptr;
    }
    if (cap_docs < 1 || cap_docs > 0x7ffffff0ll || cap_slots < 16 || cap_slots > (0x7ffffff0ll << 4)) {
        errorf("bertx_mvindex_create: capacity of %lld documents / %lld token slots is not in 1 .. 2^31 - 16 / "
               "16 .. 2^35 - 256\n", (long long)cap_docs, (long long)cap_slots);
        return nullptr;
    }
    DeviceGuard g(ordinal);
    if (!g.ok()) {
        errorf("bertx_mvindex_create: cannot select device %d\n", ordinal);
        return nullptr;
    }
    bertx_mvindex *mv = new (std::nothrow) bertx_mvindex();
    if (!mv) return nullptr;
    mv->ordinal = ordinal;
    mv->w = w;
    mv->storage = storage;
    mv->cap_docs = cap_docs;
    mv->cap_slots = cap_slots;
    const size_t slots16 = (size_t)((cap_slots + 15) / 16) * 16;
    const bool i8 = storage == BERTX_INDEX_I8;
    const size_t store_bytes = slots16 * (size_t)w * (i8 ? 1 : 2);
    const bool ok = maxsim_prepare_device() == 0 && maxsim_search_prepare_device() == 0 &&
                    hipMalloc(&mv->search_scratch, maxsim_search_scratch_bytes()) == hipSuccess &&
                    hipStreamCreateWithFlags(&mv->stream, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&mv->done, hipEventDisableTiming) == hipSuccess &&
                    hipMalloc(&mv->store, store_bytes) == hipSuccess &&
                    (!i8 || hipMalloc((void **)&mv->scales, slots16 * 4) == hipSuccess) &&
                    hipMalloc((void **)&mv->table, (size_t)cap_docs * 8) == hipSuccess &&
                    hipMalloc((void **)&mv->src_off, (size_t)cap_docs * 4) == hipSuccess &&
                    hipHostMalloc((void **)&mv->h_table, (size_t)cap_docs * 8, hipHostMallocDefault) == hipSuccess &&
                    hipHostMalloc((void **)&mv->h_src, (size_t)cap_docs * 4, hipHostMallocDefault) == hipSuccess &&
                    hipMalloc((void **)&mv->st_rows, (size_t)kStageRows * w * 4) == hipSuccess &&
                    hipMalloc((void **)&mv->st_q, (size_t)kMaxLq * w * 4) == hipSuccess &&
                    hipMalloc((void **)&mv->st_out, (size_t)kStageIds * 4) == hipSuccess &&
                    hipMalloc((void **)&mv->st_ids, (size_t)kStageIds * 4) == hipSuccess &&
                    hipMalloc((void **)&mv->st_tok, (size_t)(kMaxLq + 3) * 4) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        errorf("bertx_mvindex_create: device %d could not allocate %zu bytes of token rows (+ %lld table entries)\n",
               ordinal, store_bytes + (i8 ? slots16 * 4 : 0), (long long)cap_docs);
        delete mv;
        return nullptr;
    }
    return mv;
}

}  // namespace emb

using emb::DeviceGuard;

extern "C" {

struct bertx_mvindex *bertx_mvindex_create_ex(struct bert_ctx *ctx, int32_t slot, int32_t width, int32_t capacity_docs,
                                              int64_t capacity_token_slots, int32_t storage)
{
    if (!ctx) {
        emb::errorf("bertx_mvindex_create: no context\n");
        return nullptr;
    }
    if (bertx_num_devices(ctx) == 0) {
        emb::errorf("bertx_mvindex_create: tokenizer-only context (BERT_HOST_ONLY): no device to hold a token store\n");
        return nullptr;
    }
    const int ordinal = bertx_device_ordinal(ctx, slot);
    if (ordinal < 0) {
        emb::errorf("bertx_mvindex_create: slot %d is not one of the context's %d device(s)\n", slot,
                    bertx_num_devices(ctx));
        return nullptr;
    }
    return emb::mvindex_create_on(ordinal, width, capacity_docs, capacity_token_slots, storage);
}

struct bertx_mvindex *bertx_mvindex_create(struct bert_ctx *ctx, int32_t slot, int32_t width, int32_t capacity_docs,
                                           int64_t capacity_token_slots)
{
    return bertx_mvindex_create_ex(ctx, slot, width, capacity_docs, capacity_token_slots, BERTX_INDEX_F16);
}

int32_t bertx_mvindex_storage(struct bertx_mvindex *mv) { return mv ? mv->storage : -1; }

void bertx_mvindex_free(struct bertx_mvindex *mv) { delete mv; }

int32_t bertx_mvindex_clear(struct bertx_mvindex *mv)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    // the host images' entries are about to be reused: no copy of them may be in flight
    if (mv->any) HIP_RC(hipEventSynchronize(mv->done));
    mv->n_docs = 0;
    mv->used_slots = 0;
    return 0;
}

int32_t bertx_mvindex_docs(struct bertx_mvindex *mv)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    return (int32_t)mv->n_docs;
}

int64_t bertx_mvindex_token_slots(struct bertx_mvindex *mv)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    return mv->used_slots;
}

int32_t bertx_mvindex_capacity_docs(struct bertx_mvindex *mv) { return mv ? (int32_t)mv->cap_docs : -1; }
int64_t bertx_mvindex_capacity_token_slots(struct bertx_mvindex *mv) { return mv ? mv->cap_slots : -1; }
int32_t bertx_mvindex_dim(struct bertx_mvindex *mv) { return mv ? mv->w : -1; }

int32_t bertx_mvindex_add_device(struct bertx_mvindex *mv, const float *d_rows, const int32_t *lens, int32_t n,
                                 void *stream)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    return emb::add_device_locked(*mv, d_rows, lens, n, stream ? (hipStream_t)stream : mv->stream);
}

int32_t bertx_mvindex_add(struct bertx_mvindex *mv, const float *rows, const int32_t *lens, int32_t n)
{
    if (!mv || !rows) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    int64_t T = 0, slots = 0;
    int32_t rc = emb::plan_add(*mv, lens, n, &T, &slots);
    if (rc != 0) return rc;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    {
        emb::Ordered o(*mv, mv->stream);
        rc = emb::upload_entries(*mv, n, mv->stream);
        for (int64_t t = 0; t < T && rc == 0; t += emb::kStageRows) {
            const int64_t m = std::min<int64_t>(emb::kStageRows, T - t);
            if (hipMemcpyAsync(mv->st_rows, rows + (size_t)t * mv->w, (size_t)m * mv->w * 4, hipMemcpyHostToDevice,
                               mv->stream) != hipSuccess)
                rc = -1;
            if (rc == 0) rc = emb::pack(*mv, mv->st_rows, t, m, n, mv->stream);
            if (rc == 0 && hipStreamSynchronize(mv->stream) != hipSuccess) rc = -1;   // the staging buffer is reused
        }
    }
    if (rc != 0) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(mv->stream);
        emb::errorf("bertx_mvindex_add: device %d failed while adding (%d)\n", mv->ordinal, rc);
        return rc;
    }
    return emb::commit(*mv, n, slots);
}

int32_t bertx_mvindex_doc_len(struct bertx_mvindex *mv, int32_t id)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (id < 0 || id >= mv->n_docs) return -1;
    return mv->h_table[2 * (size_t)id + 1];
}

int32_t bertx_mvindex_doc(struct bertx_mvindex *mv, int32_t id, float *out)
{
    if (!mv || !out) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (id < 0 || id >= mv->n_docs) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    if (mv->storage == BERTX_INDEX_I8) {
        try {
            const int w = mv->w;
            const int64_t len = mv->h_table[2 * (size_t)id + 1];
            std::vector<int8_t> q((size_t)len * w);
            std::vector<float> u((size_t)len);
            const int32_t rc = emb::read_doc_i8(*mv, id, q.data(), u.data());
            if (rc != 0) return rc;
            for (int64_t r = 0; r < len; ++r)
                for (int i = 0; i < w; ++i) out[(size_t)r * w + i] = (float)q[(size_t)r * w + i] * u[(size_t)r];
        } catch (const std::bad_alloc &) {
            emb::errorf("bertx_mvindex_doc: out of host memory\n");
            return -1;
        }
        return 0;
    }
    try {
        const int w = mv->w, KB = w / 32;
        const int64_t first = mv->h_table[2 * (size_t)id], len = mv->h_table[2 * (size_t)id + 1];
        const size_t group_halfs = (size_t)16 * w;
        std::vector<uint16_t> raw((size_t)((len + 15) / 16) * group_halfs);
        if (mv->any) HIP_RC(hipEventSynchronize(mv->done));
        HIP_RC(hipMemcpy(raw.data(), (const uint16_t *)mv->store + (size_t)first * group_halfs, raw.size() * 2,
                         hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < len; ++r) {
            const uint16_t *grp = raw.data() + (size_t)(r / 16) * group_halfs;
            float *o = out + (size_t)r * w;
            for (int kb = 0; kb < KB; ++kb)
                for (int q = 0; q < 4; ++q)
                    for (int j = 0; j < 8; ++j)
                        o[32 * kb + 8 * q + j] = emb::f16_to_f32(grp[((size_t)kb * 64 + 16 * q + (r & 15)) * 8 + j]);
        }
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_doc: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_mvindex_doc_i8(struct bertx_mvindex *mv, int32_t id, int8_t *q, float *u)
{
    if (!mv || !q || !u) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (mv->storage != BERTX_INDEX_I8 || id < 0 || id >= mv->n_docs) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    try {
        // through buffers of its own: a failed copy leaves the outputs untouched
        const int64_t len = mv->h_table[2 * (size_t)id + 1];
        std::vector<int8_t> hq((size_t)len * mv->w);
        std::vector<float> hu((size_t)len);
        const int32_t rc = emb::read_doc_i8(*mv, id, hq.data(), hu.data());
        if (rc != 0) return rc;
        std::memcpy(q, hq.data(), hq.size());
        std::memcpy(u, hu.data(), hu.size() * 4);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_doc_i8: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_mvindex_score_device(struct bertx_mvindex *mv, const float *d_q, int32_t Lq, const int32_t *d_ids,
                                   int32_t n, float *d_out, void *stream)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    return emb::score_device_locked(*mv, d_q, Lq, d_ids, n, d_out, stream ? (hipStream_t)stream : mv->stream);
}

int32_t bertx_mvindex_score(struct bertx_mvindex *mv, const float *q, int32_t Lq, const int32_t *ids, int32_t n,
                            float *out)
{
    if (!mv || !q || !out || Lq < 1 || Lq > emb::kMaxLq || n < 1) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    try {
        HIP_RC(hipMemcpyAsync(mv->st_q, q, (size_t)Lq * mv->w * 4, hipMemcpyHostToDevice, mv->stream));
        return emb::score_host_ids(*mv, mv->st_q, Lq, ids, n, out);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_score: out of host memory\n");
        return -1;
    }
}

int32_t bertx_mvindex_add_texts(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                const char **texts)
{
    int32_t slot = -1;
    if (!texts || n < 1) return -1;
    if (emb::text_ctx_ok(mv, ctx, "bertx_mvindex_add_texts", &slot) != 0) return -1;
    try {
        const int32_t n_max = bert_n_max_tokens(ctx);
        std::vector<int32_t> ids((size_t)n * n_max), lens((size_t)n);
        if (bertx_tokenize_batch(ctx, n_threads, n, texts, n_max, ids.data(), lens.data()) != 0) return -1;
        for (int32_t i = 0; i < n; ++i)
            if (lens[(size_t)i] > n_max) {
                emb::errorf("Too many tokens, maximum is %d\n", n_max);
                emb::errorf("bertx_mvindex_add_texts: text %d has %d tokens; nothing was added\n", i, lens[(size_t)i]);
                return -4;
            }
        std::lock_guard<std::mutex> lk(mv->mu);
        int64_t T = 0, slots = 0;
        int32_t rc = emb::plan_add(*mv, lens.data(), n, &T, &slots);
        if (rc != 0) return rc;
        DeviceGuard g(mv->ordinal);
        HIP_RC(g.status());
        // chunks of whole texts as run_forward cuts them; each chunk's token rows go from
        // the forward's device output straight into the pack kernel on the store's stream
        std::vector<int32_t> flat, cu;
        emb::DevBuf d_ids, d_cu, d_rows;
        int64_t cap_tok = 0, cap_seq = 0;
        {
            emb::Ordered o(*mv, mv->stream);
            rc = emb::upload_entries(*mv, n, mv->stream);
            int32_t i = 0;
            int64_t t0 = 0;
            while (i < n && rc == 0) {
                flat.clear();
                cu.assign(1, 0);
                int max_len = 0;
                while (i < n && (cu.size() == 1 || ((int64_t)flat.size() + lens[(size_t)i] <= emb::kChunkTokens &&
                                                    (int)cu.size() - 1 < emb::kChunkSeqs))) {
                    const int32_t *p = ids.data() + (size_t)i * n_max;
                    flat.insert(flat.end(), p, p + lens[(size_t)i]);
                    cu.push_back((int32_t)flat.size());
                    max_len = std::max(max_len, (int)lens[(size_t)i]);
                    ++i;
                }
                const int64_t tok = (int64_t)flat.size(), seqs = (int64_t)cu.size() - 1;
                if (tok > cap_tok || seqs > cap_seq) {
                    HIP_RC(hipStreamSynchronize(mv->stream));
                    for (emb::DevBuf *b : {&d_ids, &d_cu, &d_rows})
                        if (b->p) { (void)hipFree(b->p); b->p = nullptr; }
                    cap_tok = std::max(tok, cap_tok);
                    cap_seq = std::max(seqs, cap_seq);
                    HIP_RC(hipMalloc(&d_ids.p, (size_t)cap_tok * 4));
                    HIP_RC(hipMalloc(&d_cu.p, (size_t)(cap_seq + 1) * 4));
                    HIP_RC(hipMalloc(&d_rows.p, (size_t)cap_tok * mv->w * 4));
                }
                if (bertx_reserve(ctx, slot, (int32_t)tok, (int32_t)seqs) != 0) { rc = -1; break; }
                HIP_RC(hipMemcpyAsync(d_ids.p, flat.data(), (size_t)tok * 4, hipMemcpyHostToDevice, mv->stream));
                HIP_RC(hipMemcpyAsync(d_cu.p, cu.data(), (size_t)(seqs + 1) * 4, hipMemcpyHostToDevice, mv->stream));
                rc = bertx_forward_tokens_device(ctx, slot, (const int32_t *)d_ids.p, (const int32_t *)d_cu.p,
                                                 (int32_t)seqs, max_len, (int32_t)tok, (float *)d_rows.p, mv->stream);
                if (rc == 0) rc = emb::pack(*mv, (const float *)d_rows.p, t0, tok, n, mv->stream);
                // the chunk's host and device buffers are reused by the next one
                if (rc == 0 && hipStreamSynchronize(mv->stream) != hipSuccess) rc = -1;
                t0 += tok;
            }
        }
        if (rc != 0) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(mv->stream);
            emb::errorf("bertx_mvindex_add_texts: device %d failed while adding (%d)\n", mv->ordinal, rc);
            return rc < 0 ? rc : -1;
        }
        return emb::commit(*mv, n, slots);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_mvindex_add_texts: %s\n", ex.what());
        return -1;
    }
}

int32_t bertx_mvindex_score_text(struct bertx_mvindex *mv, struct bert_ctx *ctx, const char *query, const int32_t *ids,
                                 int32_t n, float *out)
{
    int32_t slot = -1;
    if (!query || !out || n < 1) return -1;
    if (emb::text_ctx_ok(mv, ctx, "bertx_mvindex_score_text", &slot) != 0) return -1;
    try {
        const int32_t n_max = bert_n_max_tokens(ctx);
        std::vector<int32_t> tok((size_t)n_max + 2);
        int32_t L = 0;
        bert_tokenize(ctx, query, tok.data(), &L, n_max);
        if (L > n_max || L > emb::kMaxLq) {
            emb::errorf("bertx_mvindex_score_text: the query has %d tokens, maximum is %d\n", L,
                        std::min<int32_t>(n_max, emb::kMaxLq));
            return -4;
        }
        if (L < 1) return -1;
        std::lock_guard<std::mutex> lk(mv->mu);
        DeviceGuard g(mv->ordinal);
        HIP_RC(g.status());
        // ids [L] and cu {0, L} in one staging buffer, the token rows into the query staging
        std::vector<int32_t> h((size_t)emb::kMaxLq + 2, 0);
        std::memcpy(h.data(), tok.data(), (size_t)L * 4);
        h[(size_t)emb::kMaxLq] = 0;
        h[(size_t)emb::kMaxLq + 1] = L;
        if (bertx_reserve(ctx, slot, L, 1) != 0) return -1;
        int32_t rc = 0;
        {
            emb::Ordered o(*mv, mv->stream);
            HIP_RC(hipMemcpyAsync(mv->st_tok, h.data(), h.size() * 4, hipMemcpyHostToDevice, mv->stream));
            HIP_RC(hipStreamSynchronize(mv->stream));   // h is pageable and leaves scope
            rc = bertx_forward_tokens_device(ctx, slot, mv->st_tok, mv->st_tok + emb::kMaxLq, 1, L, L, mv->st_q,
                                             mv->stream);
        }
        if (rc != 0) return rc < 0 ? rc : -1;
        return emb::score_host_ids(*mv, mv->st_q, L, ids, n, out);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_mvindex_score_text: %s\n", ex.what());
        return -1;
    }
}

int32_t bertx_mvindex_add_texts_colbert(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                        const char **texts, int32_t doc_maxlen)
{
    int32_t slot = -1;
    if (!texts || n < 1) return -1;
    if (const int32_t rc = emb::colbert_ctx_ok(mv, ctx, "bertx_mvindex_add_texts_colbert", &slot)) return rc;
    if (doc_maxlen < 4 || doc_maxlen > bert_n_max_tokens(ctx)) return -1;
    for (int32_t i = 0; i < n; ++i)
        if (!texts[i]) return -1;
    try {
        const size_t N = (size_t)doc_maxlen;
        std::vector<int32_t> ids((size_t)n * N), keep((size_t)n * N), lens((size_t)n), kept((size_t)n), rcs((size_t)n, 0);
        emb::TaskPool::instance().run(((int64_t)n + 7) / 8, n_threads > 0 ? n_threads : 1, [&](int64_t blk) {
            const int e = (int)std::min<int64_t>(n, 8 * blk + 8);
            for (int i = (int)(8 * blk); i < e; ++i) {
                rcs[(size_t)i] = bertx_tokenize_colbert(ctx, texts[i], 1, doc_maxlen, ids.data() + i * N,
                                                        keep.data() + i * N, &lens[(size_t)i]);
                int32_t c = 0;
                for (int32_t t = 0; rcs[(size_t)i] == 0 && t < lens[(size_t)i]; ++t) c += keep[i * N + t];
                kept[(size_t)i] = c;
            }
        });
        for (int32_t i = 0; i < n; ++i)
            if (rcs[(size_t)i] != 0) return -1;
        std::lock_guard<std::mutex> lk(mv->mu);
        int64_t T = 0, slots = 0;
        int32_t rc = emb::plan_add(*mv, kept.data(), n, &T, &slots);   // (a document keeps [CLS], [D] and [SEP]: >= 3)
        if (rc != 0) return rc;
        DeviceGuard g(mv->ordinal);
        HIP_RC(g.status());
        // the chunks of _add_texts; per chunk the kept tokens' packed rows are the row map,
        // and the projector's device output goes straight into the pack kernel
        std::vector<int32_t> flat, cu, map;
        emb::DevBuf d_ids, d_cu, d_map, d_rows;
        int64_t cap_tok = 0, cap_seq = 0;
        {
            emb::Ordered o(*mv, mv->stream);
            rc = emb::upload_entries(*mv, n, mv->stream);
            int32_t i = 0;
            int64_t t0 = 0;
            while (i < n && rc == 0) {
                flat.clear();
                map.clear();
                cu.assign(1, 0);
                int max_len = 0;
                while (i < n && (cu.size() == 1 || ((int64_t)flat.size() + lens[(size_t)i] <= emb::kChunkTokens &&
                                                    (int)cu.size() - 1 < emb::kChunkSeqs))) {
                    const int32_t *p = ids.data() + i * N, *kp = keep.data() + i * N;
                    for (int32_t t = 0; t < lens[(size_t)i]; ++t)
                        if (kp[t]) map.push_back((int32_t)flat.size() + t);
                    flat.insert(flat.end(), p, p + lens[(size_t)i]);
                    cu.push_back((int32_t)flat.size());
                    max_len = std::max(max_len, (int)lens[(size_t)i]);
                    ++i;
                }
                const int64_t tok = (int64_t)flat.size(), seqs = (int64_t)cu.size() - 1, rows = (int64_t)map.size();
                if (tok > cap_tok || seqs > cap_seq) {
                    HIP_RC(hipStreamSynchronize(mv->stream));
                    for (emb::DevBuf *b : {&d_ids, &d_cu, &d_map, &d_rows})
                        if (b->p) { (void)hipFree(b->p); b->p = nullptr; }
                    cap_tok = std::max(tok, cap_tok);
                    cap_seq = std::max(seqs, cap_seq);
                    HIP_RC(hipMalloc(&d_ids.p, (size_t)cap_tok * 4));
                    HIP_RC(hipMalloc(&d_cu.p, (size_t)(cap_seq + 1) * 4));
                    HIP_RC(hipMalloc(&d_map.p, (size_t)cap_tok * 4));
                    HIP_RC(hipMalloc(&d_rows.p, (size_t)cap_tok * mv->w * 4));
                }
                if (bertx_reserve(ctx, slot, (int32_t)tok, (int32_t)seqs) != 0) { rc = -1; break; }
                HIP_RC(hipMemcpyAsync(d_ids.p, flat.data(), (size_t)tok * 4, hipMemcpyHostToDevice, mv->stream));
                HIP_RC(hipMemcpyAsync(d_cu.p, cu.data(), (size_t)(seqs + 1) * 4, hipMemcpyHostToDevice, mv->stream));
                HIP_RC(hipMemcpyAsync(d_map.p, map.data(), (size_t)rows * 4, hipMemcpyHostToDevice, mv->stream));
                rc = bertx_forward_project_device(ctx, slot, (const int32_t *)d_ids.p, nullptr, (const int32_t *)d_cu.p,
                                                  (int32_t)seqs, max_len, (int32_t)tok, (const int32_t *)d_map.p,
                                                  (int32_t)rows, (float *)d_rows.p, mv->stream);
                if (rc == 0) rc = emb::pack(*mv, (const float *)d_rows.p, t0, rows, n, mv->stream);
                // the chunk's host and device buffers are reused by the next one
                if (rc == 0 && hipStreamSynchronize(mv->stream) != hipSuccess) rc = -1;
                t0 += rows;
            }
        }
        if (rc != 0) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(mv->stream);
            emb::errorf("bertx_mvindex_add_texts_colbert: device %d failed while adding (%d)\n", mv->ordinal, rc);
            return rc < 0 ? rc : -1;
        }
        return emb::commit(*mv, n, slots);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_mvindex_add_texts_colbert: %s\n", ex.what());
        return -1;
    }
}

int32_t bertx_mvindex_score_text_colbert(struct bertx_mvindex *mv, struct bert_ctx *ctx, const char *query,
                                         int32_t query_maxlen, const int32_t *ids, int32_t n, float *out)
{
    int32_t slot = -1;
    if (!query || !out || n < 1) return -1;
    if (const int32_t rc = emb::colbert_ctx_ok(mv, ctx, "bertx_mvindex_score_text_colbert", &slot)) return rc;
    if (query_maxlen < 4 || query_maxlen > emb::kMaxLq || query_maxlen > bert_n_max_tokens(ctx)) return -1;
    try {
        // ids [L], cu {0, L} and the key count in one staging buffer, as _score_text; L = query_maxlen
        std::vector<int32_t> h((size_t)emb::kMaxLq + 3, 0), keep((size_t)emb::kMaxLq);
        int32_t L = 0, nk = 0;
        if (bertx_tokenize_colbert_ex(ctx, query, 0, query_maxlen, h.data(), keep.data(), &L, &nk) != 0 ||
            L != query_maxlen)
            return -1;
        h[(size_t)emb::kMaxLq] = 0;
        h[(size_t)emb::kMaxLq + 1] = L;
        h[(size_t)emb::kMaxLq + 2] = nk;
        // the context's setting: [MASK] rows as keys (no counts), or the rows up to [SEP] only
        const bool counted = bertx_mask_keys(ctx) == 0;
        std::lock_guard<std::mutex> lk(mv->mu);
        DeviceGuard g(mv->ordinal);
        HIP_RC(g.status());
        if (bertx_reserve(ctx, slot, L, 1) != 0) return -1;
        int32_t rc = 0;
        {
            emb::Ordered o(*mv, mv->stream);
            HIP_RC(hipMemcpyAsync(mv->st_tok, h.data(), h.size() * 4, hipMemcpyHostToDevice, mv->stream));
            HIP_RC(hipStreamSynchronize(mv->stream));   // h is pageable and leaves scope
            rc = bertx_forward_device_kv(ctx, slot, mv->st_tok, nullptr, mv->st_tok + emb::kMaxLq,
                                         counted ? mv->st_tok + emb::kMaxLq + 2 : nullptr, 1, L, L, BERTX_OUT_PROJ,
                                         nullptr, 0, mv->st_q, mv->stream);
        }
        if (rc != 0) return rc < 0 ? rc : -1;
        return emb::score_host_ids(*mv, mv->st_q, L, ids, n, out);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_mvindex_score_text_colbert: %s\n", ex.what());
        return -1;
    }
}

int32_t bertx_mvindex_search_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq, int32_t k,
                                    float *d_scores, int32_t *d_ids, void *stream)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    return emb::search_device_locked(*mv, d_q, B, Lq, k, d_scores, d_ids, stream ? (hipStream_t)stream : mv->stream);
}

int32_t bertx_mvindex_search(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t k, float *scores,
                             int32_t *ids)
{
    if (!mv || !q || !scores || !ids || !emb::search_args_ok("bertx_mvindex_search", B, Lq, k)) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    try {
        const size_t nq = (size_t)B * Lq * mv->w, nr = (size_t)B * k;
        std::vector<float> hs(nr);
        std::vector<int32_t> hi(nr);
        emb::DevBuf d_q;
        HIP_RC(hipMalloc(&d_q.p, nq * 4));
        HIP_RC(hipMemcpyAsync(d_q.p, q, nq * 4, hipMemcpyHostToDevice, mv->stream));
        const int32_t rc = emb::search_to_host(*mv, (const float *)d_q.p, B, Lq, k, hs.data(), hi.data());
        if (rc != 0) return rc;
        std::memcpy(scores, hs.data(), nr * 4);
        std::memcpy(ids, hi.data(), nr * 4);
        return 0;
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_search: out of host memory\n");
        return -1;
    }
}

int32_t bertx_mvindex_search_texts(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                   const char **texts, int32_t k, float *scores, int32_t *ids)
{
    int32_t slot = -1;
    if (!texts || !scores || !ids || n < 1) return -1;
    if (emb::text_ctx_ok(mv, ctx, "bertx_mvindex_search_texts", &slot) != 0) return -1;
    if (!emb::search_args_ok("bertx_mvindex_search_texts", n, 1, k)) return -1;
    try {
        const int32_t n_max = bert_n_max_tokens(ctx), lim = std::min<int32_t>(n_max, emb::kMaxLq);
        const int w = mv->w;
        std::vector<int32_t> tok((size_t)n * n_max), lens((size_t)n);
        if (bertx_tokenize_batch(ctx, n_threads, n, texts, n_max, tok.data(), lens.data()) != 0) return -1;
        for (int32_t i = 0; i < n; ++i) {
            if (lens[(size_t)i] > lim) {
                emb::errorf("bertx_mvindex_search_texts: query %d has %d tokens, maximum is %d\n", i, lens[(size_t)i], lim);
                return -4;
            }
            if (lens[(size_t)i] < 1) return -1;
        }
        std::vector<float> hs((size_t)n * k);
        std::vector<int32_t> hi((size_t)n * k), flat, cu;
        std::lock_guard<std::mutex> lk(mv->mu);
        DeviceGuard g(mv->ordinal);
        HIP_RC(g.status());
        const int32_t cap = std::min<int32_t>(n, emb::kSearchTexts);
        emb::DevBuf d_tok, d_cu, d_rows, d_q;
        HIP_RC(hipMalloc(&d_tok.p, (size_t)cap * emb::kMaxLq * 4));
        HIP_RC(hipMalloc(&d_cu.p, (size_t)(cap + 1) * 4));
        HIP_RC(hipMalloc(&d_rows.p, (size_t)cap * emb::kMaxLq * w * 4));
        HIP_RC(hipMalloc(&d_q.p, (size_t)cap * emb::kMaxLq * w * 4));
        // chunks of whole queries: one per-token forward, the rows laid out [m][Lmax][w] with
        // zero rows behind the shorter queries (device-to-device), then the search
        for (int32_t i0 = 0; i0 < n; i0 += cap) {
            const int32_t m = std::min(cap, n - i0);
            flat.clear();
            cu.assign(1, 0);
            int32_t Lmax = 0;
            for (int32_t i = i0; i < i0 + m; ++i) {
                const int32_t *p = tok.data() + (size_t)i * n_max;
                flat.insert(flat.end(), p, p + lens[(size_t)i]);
                cu.push_back((int32_t)flat.size());
                Lmax = std::max(Lmax, lens[(size_t)i]);
            }
            const int32_t T = (int32_t)flat.size();
            if (bertx_reserve(ctx, slot, T, m) != 0) return -1;
            int32_t rc = 0;
            {
                emb::Ordered o(*mv, mv->stream);
                HIP_RC(hipMemcpyAsync(d_tok.p, flat.data(), (size_t)T * 4, hipMemcpyHostToDevice, mv->stream));
                HIP_RC(hipMemcpyAsync(d_cu.p, cu.data(), (size_t)(m + 1) * 4, hipMemcpyHostToDevice, mv->stream));
                rc = bertx_forward_tokens_device(ctx, slot, (const int32_t *)d_tok.p, (const int32_t *)d_cu.p, m, Lmax, T,
                                                 (float *)d_rows.p, mv->stream);
                if (rc == 0) {
                    HIP_RC(hipMemsetAsync(d_q.p, 0, (size_t)m * Lmax * w * 4, mv->stream));
                    for (int32_t j = 0; j < m; ++j)
                        HIP_RC(hipMemcpyAsync((float *)d_q.p + (size_t)j * Lmax * w, (const float *)d_rows.p + (size_t)cu[(size_t)j] * w,
                                              (size_t)lens[(size_t)(i0 + j)] * w * 4, hipMemcpyDeviceToDevice, mv->stream));
                }
            }
            if (rc == 0)
                rc = emb::search_to_host(*mv, (const float *)d_q.p, m, Lmax, k, hs.data() + (size_t)i0 * k,
                                         hi.data() + (size_t)i0 * k);
            if (rc != 0) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(mv->stream);
                return rc < 0 ? rc : -1;
            }
        }
        std::memcpy(scores, hs.data(), hs.size() * 4);
        std::memcpy(ids, hi.data(), hi.size() * 4);
        return 0;
    } catch (const std::exception &ex) {
        emb::errorf("bertx_mvindex_search_texts: %s\n", ex.what());
        return -1;
    }
}

int32_t bertx_mvindex_search_texts_colbert(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                           const char **texts, int32_t query_maxlen, int32_t k, float *scores,
                                           int32_t *ids)
{
    int32_t slot = -1;
    if (!texts || !scores || !ids || n < 1) return -1;
    if (const int32_t rc = emb::colbert_ctx_ok(mv, ctx, "bertx_mvindex_search_texts_colbert", &slot)) return rc;
    if (query_maxlen < 4 || query_maxlen > emb::kMaxLq || query_maxlen > bert_n_max_tokens(ctx)) return -1;
    if (!emb::search_args_ok("bertx_mvindex_search_texts_colbert", n, query_maxlen, k)) return -1;
    for (int32_t i = 0; i < n; ++i)
        if (!texts[i]) return -1;
    try {
        // every augmented query has L = query_maxlen tokens, all kept: the projector's output
        // is the [n][L][w] layout itself
        const size_t L = (size_t)query_maxlen;
        const int w = mv->w;
        std::vector<int32_t> tok((size_t)n * L), lens((size_t)n), nks((size_t)n), rcs((size_t)n, 0);
        emb::TaskPool::instance().run(((int64_t)n + 7) / 8, n_threads > 0 ? n_threads : 1, [&](int64_t blk) {
            const int e = (int)std::min<int64_t>(n, 8 * blk + 8);
            std::vector<int32_t> keep(L);
            for (int i = (int)(8 * blk); i < e; ++i)
                rcs[(size_t)i] = bertx_tokenize_colbert_ex(ctx, texts[i], 0, query_maxlen, tok.data() + i * L, keep.data(),
                                                           &lens[(size_t)i], &nks[(size_t)i]);
        });
        // the context's setting: [MASK] rows as keys (no counts), or each query's rows up to [SEP] only
        const bool counted = bertx_mask_keys(ctx) == 0;
        for (int32_t i = 0; i < n; ++i)
            if (rcs[(size_t)i] != 0 || lens[(size_t)i] != query_maxlen) return -1;
        std::vector<float> hs((size_t)n * k);
        std::vector<int32_t> hi((size_t)n * k), cu;
        std::lock_guard<std::mutex> lk(mv->mu);
        DeviceGuard g(mv->ordinal);
        HIP_RC(g.status());
        const int32_t cap = std::min<int32_t>(n, emb::kSearchTexts);
        emb::DevBuf d_tok, d_cu, d_q, d_nk;
        HIP_RC(hipMalloc(&d_tok.p, (size_t)cap * L * 4));
        HIP_RC(hipMalloc(&d_cu.p, (size_t)(cap + 1) * 4));
        HIP_RC(hipMalloc(&d_q.p, (size_t)cap * L * w * 4));
        if (counted) HIP_RC(hipMalloc(&d_nk.p, (size_t)cap * 4));
        cu.resize((size_t)cap + 1);
        for (int32_t j = 0; j <= cap; ++j) cu[(size_t)j] = j * query_maxlen;
        for (int32_t i0 = 0; i0 < n; i0 += cap) {
            const int32_t m = std::min(cap, n - i0), T = m * query_maxlen;
            if (bertx_reserve(ctx, slot, T, m) != 0) return -1;
            int32_t rc = 0;
            {
                emb::Ordered o(*mv, mv->stream);
                HIP_RC(hipMemcpyAsync(d_tok.p, tok.data() + (size_t)i0 * L, (size_t)T * 4, hipMemcpyHostToDevice, mv->stream));
                HIP_RC(hipMemcpyAsync(d_cu.p, cu.data(), (size_t)(m + 1) * 4, hipMemcpyHostToDevice, mv->stream));
                if (counted)
                    HIP_RC(hipMemcpyAsync(d_nk.p, nks.data() + i0, (size_t)m * 4, hipMemcpyHostToDevice, mv->stream));
                rc = bertx_forward_device_kv(ctx, slot, (const int32_t *)d_tok.p, nullptr, (const int32_t *)d_cu.p,
                                             (const int32_t *)d_nk.p, m, query_maxlen, T, BERTX_OUT_PROJ, nullptr, 0,
                                             (float *)d_q.p, mv->stream);
            }
            if (rc == 0)
                rc = emb::search_to_host(*mv, (const float *)d_q.p, m, query_maxlen, k, hs.data() + (size_t)i0 * k,
                                         hi.data() + (size_t)i0 * k);
            if (rc != 0) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(mv->stream);
                return rc < 0 ? rc : -1;
            }
        }
        std::memcpy(scores, hs.data(), hs.size() * 4);
        std::memcpy(ids, hi.data(), hi.size() * 4);
        return 0;
    } catch (const std::exception &ex) {
        emb::errorf("bertx_mvindex_search_texts_colbert: %s\n", ex.what());
        return -1;
    }
}

}  // extern "C"

// The MaxSim micro-benchmarks (bert_hip.h): device 0, no context.  B == 0: the scorer over
// n_cand candidates; B >= 1: the full-scan search of B queries for the k best.
static int32_t bench_store(int32_t w, int32_t n_docs, int32_t doc_len, int32_t Lq, int32_t n_cand, int32_t B, int32_t k,
                           int32_t storage, int32_t iters, float *avg_us)
{
    using namespace emb;
    if (n_docs < 1 || doc_len < 0 || doc_len > 4096 || n_cand < 1 || iters < 1 || !avg_us || hip_device_count() == 0)
        return -1;
    if (B > 0 && !search_args_ok("bertx_bench_maxsim_search", B, Lq, k)) return -1;
    const int32_t nq = std::max(B, 1);
    try {
        // ragged (doc_len 0): 16 .. 512 tokens by a hash of the id
        std::vector<int32_t> lens((size_t)n_docs), ids((size_t)n_cand);
        int64_t slots = 0;
        for (int32_t i = 0; i < n_docs; ++i) {
            uint32_t h = (uint32_t)i * 2654435761u + 99u;
            h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
            lens[(size_t)i] = doc_len ? doc_len : 16 + (int32_t)(h % 497u);
            slots += (lens[(size_t)i] + 15) / 16 * 16;
        }
        for (int32_t c = 0; c < n_cand; ++c) ids[(size_t)c] = (int32_t)(((uint64_t)c * 2654435761ull + 12345ull) % (uint64_t)n_docs);
        DeviceGuard guard(0);
        HIP_RC(guard.status());
        struct Holder {
            bertx_mvindex *mv = nullptr;
            hipStream_t s = nullptr;
            hipEvent_t a = nullptr, b = nullptr;
            DevBuf rows, q, id, out, oid;
            ~Holder()
            {
                if (s) (void)hipStreamSynchronize(s);
                if (a) (void)hipEventDestroy(a);
                if (b) (void)hipEventDestroy(b);
                if (s) (void)hipStreamDestroy(s);
                bertx_mvindex_free(mv);
            }
        } H;
        H.mv = mvindex_create_on(0, w, n_docs, slots, storage);
        if (!H.mv) return -1;
        HIP_RC(hipStreamCreateWithFlags(&H.s, hipStreamNonBlocking));
        HIP_RC(hipEventCreate(&H.a));
        HIP_RC(hipEventCreate(&H.b));
        constexpr int64_t kFillRows = 1 << 18;
        HIP_RC(hipMalloc(&H.rows.p, (size_t)(kFillRows + 4096) * w * 4));
        HIP_RC(hipMalloc(&H.q.p, (size_t)nq * kMaxLq * w * 4));
        HIP_RC(hipMalloc(&H.id.p, (size_t)n_cand * 4));
        HIP_RC(hipMalloc(&H.out.p, (size_t)std::max(n_cand, nq * kMaxK) * 4));
        HIP_RC(hipMalloc(&H.oid.p, (size_t)nq * kMaxK * 4));
        for (int32_t i = 0; i < n_docs;) {
            int32_t j = i;
            int64_t rows = 0;
            while (j < n_docs && (j == i || rows + lens[(size_t)j] <= kFillRows)) rows += lens[(size_t)j++];
            if (launch_unit_rows((float *)H.rows.p, rows, w, 12345u + (uint32_t)i, H.s) != 0) return -1;
            if (bertx_mvindex_add_device(H.mv, (const float *)H.rows.p, lens.data() + i, j - i, H.s) < 0) return -1;
            HIP_RC(hipStreamSynchronize(H.s));   // the fill buffer is reused
            i = j;
        }
        if (Lq < 1 || Lq > kMaxLq || launch_unit_rows((float *)H.q.p, (int64_t)nq * Lq, w, 777u, H.s) != 0) return -1;
        HIP_RC(hipMemcpyAsync(H.id.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, H.s));
        HIP_RC(hipStreamSynchronize(H.s));
        auto run = [&] {
            if (B > 0)
                return bertx_mvindex_search_device(H.mv, (const float *)H.q.p, B, Lq, k, (float *)H.out.p,
                                                   (int32_t *)H.oid.p, H.s);
            return bertx_mvindex_score_device(H.mv, (const float *)H.q.p, Lq, (const int32_t *)H.id.p, n_cand,
                                              (float *)H.out.p, H.s);
        };
        for (int i = 0; i < 3; ++i)
            if (run() != 0) return -1;
        HIP_RC(hipEventRecord(H.a, H.s));
        for (int i = 0; i < iters; ++i)
            if (run() != 0) return -1;
        HIP_RC(hipEventRecord(H.b, H.s));
        HIP_RC(hipEventSynchronize(H.b));
        float ms = 0.f;
        HIP_RC(hipEventElapsedTime(&ms, H.a, H.b));
        *avg_us = ms * 1000.f / (float)iters;
        return 0;
    } catch (const std::exception &ex) {
        emb::errorf("bertx_bench_maxsim: %s\n", ex.what());
        return -1;
    }
}

extern "C" {

int32_t bertx_bench_maxsim_ex(int32_t w, int32_t n_docs, int32_t doc_len, int32_t Lq, int32_t n_cand, int32_t storage,
                              int32_t iters, float *avg_us)
{
    return bench_store(w, n_docs, doc_len, Lq, n_cand, 0, 0, storage, iters, avg_us);
}

int32_t bertx_bench_maxsim_search(int32_t w, int32_t n_docs, int32_t doc_len, int32_t Lq, int32_t B, int32_t k,
                                  int32_t storage, int32_t iters, float *avg_us)
{
    if (B < 1) return -1;
    return bench_store(w, n_docs, doc_len, Lq, 1, B, k, storage, iters, avg_us);
}

int32_t bertx_bench_maxsim(int32_t w, int32_t n_docs, int32_t doc_len, int32_t Lq, int32_t n_cand, int32_t iters,
                           float *avg_us)
{
    return bertx_bench_maxsim_ex(w, n_docs, doc_len, Lq, n_cand, BERTX_INDEX_F16, iters, avg_us);
}

}  // extern "C"
