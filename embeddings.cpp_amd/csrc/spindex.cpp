// The sparse index (bert_hip.h bertx_spindex_*): an append-only, device-
// resident set of sparse documents and the fused top-k scan over it.  A document is a run
// of postings (uint32 = term | f16 weight << 16, ascending term) padded to whole units of 16;
// the documents lie contiguous in id order and a device table holds (first unit, postings)
// per document.  Dense rows become documents on the device: top-n selection, f16 rounding,
// padding and the offsets (a prefix sum of the counts the host never sees).  The host knows
// the used units only as an upper bound and asks the device when the bound stops an add.
// The ordering rules are the other two stores' (store_common.h).  Beside the forward store an
// inverted image (block-local term lists) is built on request and covers
// inverted_docs documents; the inverted search refuses to run while that is not all of them.
// Tombstones (index_mask.hip) and the callers' filters limit every search to the admissible
// documents (bert_hip.h "Sparse index", "Deleting documents and filtered search").
// Listed documents are scored by a gather (sparse_gather.hip), and the hybrid search (bert_hip.h
// "Hybrid search") stacks that scorer, the embedding index's and the two first
// stages around the union and fusion kernels (hybrid.hip); its scratch belongs to this store.
#include "bert.h"
#include "bert_hip.h"

#include "chunk_rule.h"
#include "engine.h"
#include "hip_check.h"
#include "kernels.h"
#include "store_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

namespace {
constexpr int kStage = 64;   // dense rows of the host forms' staging (an add chunk, a search's queries)
}

struct bertx_spindex {
    int ordinal = 0;
    int V = 0, n_top = 0;
    int64_t cap_docs = 0, cap_units = 0;
    int64_t n_docs = 0, used_bound = 0;    // used_bound >= the device's used units (d_used)
    uint32_t *store = nullptr;             // cap_units * 16 postings
    int32_t *table = nullptr;              // device: (first unit, postings) per document
    int32_t *d_used = nullptr;             // device: the used units
    // the selection's output for one chunk of kSparseAddRows rows
    int32_t *sel_terms = nullptr, *sel_count = nullptr;
    float *sel_weights = nullptr;
    float *st_rows = nullptr;              // f32 [kStage][V]
    float *st_scores = nullptr;            // [64][128]
    int32_t *st_ids = nullptr;
    void *qtab = nullptr, *partial = nullptr;
    // sparse queries: the host forms' staging int32 / f32 [kStage][1024], the passes' images
    int32_t *st_qterms = nullptr;
    float *st_qweights = nullptr;
    void *qimage = nullptr;
    int grid_cap = 0, last_grid = 0;       // bertx_test_spindex_grid
    int last_passes = 0;                   // bertx_test_spindex_last_passes
    // the inverted image (sparse_invert.hip), allocated by the first build
    int inv_block = emb::kSparseInvBlock;
    int64_t inverted_docs = 0;
    uint32_t *inv = nullptr, *inv_rows = nullptr;   // cap_units * 16 postings; offset rows of every block
    size_t inv_rows_bytes = 0;
    // the tombstones (index_mask.hip): bit d % 32 of word d / 32 is 1 once document d was
    // removed; `removed`: some remove was accepted since creation or the last clear, so the
    // searches take their masked instantiations.  last_masked (test hook
    // bertx_test_spindex_last_masked): the latest scan launch was a masked one
    uint32_t *tomb = nullptr;
    int64_t tomb_words = 0;
    bool removed = false;
    int last_masked = 0;
    // the hybrid search's scratch, allocated by the first hybrid call: cd, cs, U, rd, rs, sd, ss,
    // [64][128] words each
    int32_t *hyb = nullptr;
    hipStream_t stream = nullptr;
    emb::StoreOrder ord;
    std::mutex mu;
    ~bertx_spindex()
    {
        emb::DeviceGuard g(ordinal);
        if (stream) (void)hipStreamSynchronize(stream);
        if (ord.done) (void)ord.wait();
        for (void *p : {(void *)store, (void *)table, (void *)d_used, (void *)sel_terms, (void *)sel_count,
                        (void *)sel_weights, (void *)st_rows, (void *)st_scores, (void *)st_ids, qtab, partial,
                        (void *)st_qterms, (void *)st_qweights, qimage, (void *)inv, (void *)inv_rows,
                        (void *)tomb, (void *)hyb})
            if (p) (void)hipFree(p);
        if (ord.done) (void)hipEventDestroy(ord.done);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace emb {
namespace {

int64_t units_of(int64_t postings) { return (postings + 15) / 16; }

// The device's used units (the store locked, its device current); waits for the store.
int32_t read_used(bertx_spindex &sp, int64_t *used)
{
    HIP_RC(sp.ord.wait());
    int32_t u = 0;
    HIP_RC(hipMemcpy(&u, sp.d_used, 4, hipMemcpyDeviceToHost));
    *used = sp.used_bound = u;
    return 0;
}

// Room for n more documents of at most `worst` units in all: by the bound, else by the
// device's own count.
int32_t room_for(bertx_spindex &sp, const char *who, int64_t n, int64_t worst)
{
    if (sp.n_docs + n > sp.cap_docs) {
        errorf("%s: %lld documents do not fit (%lld of %lld used)\n", who, (long long)n, (long long)sp.n_docs,
               (long long)sp.cap_docs);
        return -2;
    }
    if (sp.used_bound + worst <= sp.cap_units) return 0;
    int64_t used = 0;
    if (const int32_t rc = read_used(sp, &used)) return rc;
    if (used + worst <= sp.cap_units) return 0;
    errorf("%s: up to %lld postings do not fit (%lld of %lld used)\n", who, (long long)worst * 16, (long long)used * 16,
           (long long)sp.cap_units * 16);
    return -2;
}

// n dense rows on the device -> documents n_docs .. n_docs + n - 1, on s.  Returns the first new id.
int32_t add_device_locked(bertx_spindex &sp, const float *d_rows, int32_t n, hipStream_t s, const char *who)
{
    if (!d_rows || n < 1) return -1;
    const int64_t worst = (int64_t)n * units_of(sp.n_top);
    if (const int32_t rc = room_for(sp, who, n, worst)) return rc;
    int rc = 0;
    {
        Ordered o(sp.ord, s);
        for (int32_t i = 0; i < n && rc == 0; i += kSparseAddRows) {
            const int m = std::min<int32_t>(kSparseAddRows, n - i);
            rc = launch_sparse_select(d_rows + (size_t)i * sp.V, m, sp.V, sp.n_top, sp.sel_terms, sp.sel_weights,
                                      sp.sel_count, s);
            if (rc == 0)
                rc = launch_sparse_pack(sp.sel_terms, sp.sel_weights, sp.sel_count, m, sp.n_top,
                                        sp.table + 2 * (size_t)(sp.n_docs + i), sp.d_used, sp.store, s);
        }
    }
    if (rc != 0) {
        errorf("%s: device %d refused a launch (%d)\n", who, sp.ordinal, rc);
        return rc;
    }
    const int32_t first = (int32_t)sp.n_docs;
    sp.n_docs += n;
    sp.used_bound += worst;
    return first;
}

// The mask of a search (sp locked): none while nothing was removed and no filter is given, which
// launches the unmasked kernels with the arguments they always had; else the store's
// tombstones with the call's filters (not read on an empty store).
struct ScanMask {
    SearchMask m;
    bool on;
    ScanMask(bertx_spindex &sp, const Filters &f)
        : m{sp.tomb, sp.n_docs > 0 ? f.d : nullptr, f.stride}, on(sp.removed || f.d)
    {
        sp.last_masked = on;
    }
    const SearchMask *get() const { return on ? &m : nullptr; }
};

constexpr int32_t kStageIds = 64 * 128;   // int32 entries of st_ids, the staging of remove / deleted

int32_t remove_device_locked(bertx_spindex &sp, const int32_t *d_ids, int32_t n, hipStream_t s)
{
    if (!d_ids || n < 1) return -1;
    Ordered o(sp.ord, s);
    const int rc = launch_index_remove(d_ids, n, sp.n_docs, sp.tomb, s);
    if (rc == 0) sp.removed = true;
    return rc;
}

int32_t search_device_locked(bertx_spindex &sp, const float *d_q, int32_t B, int32_t k, float *d_scores, int32_t *d_ids,
                             hipStream_t s, const Filters &f = Filters())
{
    if (!d_q || !d_scores || !d_ids || B < 1 || B > 64 || k < 1 || k > 128) {
        errorf("bertx_spindex_search: B = %d, k = %d are not in 1 <= B <= 64, 1 <= k <= 128\n", B, k);
        return -1;
    }
    Ordered o(sp.ord, s);
    const int NQ = sparse_scan_pair(sp.V, k);
    sp.last_passes = (B + NQ - 1) / NQ;
    const ScanMask mask(sp, f);
    return launch_sparse_scan(sp.store, sp.table, sp.d_used, (int)sp.n_docs, sp.V, d_q, B, k, sp.qtab, sp.partial, d_scores,
                              d_ids, s, sp.grid_cap, &sp.last_grid, mask.get());
}

int32_t search_sparse_device_locked(bertx_spindex &sp, const int32_t *d_terms, const float *d_weights, int32_t B,
                                    int32_t q_top, int32_t k, float *d_scores, int32_t *d_ids, hipStream_t s,
                                    const Filters &f = Filters())
{
    const int NQ = sparse_batch_queries(sp.V, q_top, k);
    if (!d_terms || !d_weights || !d_scores || !d_ids || B < 1 || B > 64 || NQ == 0) {
        errorf("bertx_spindex_search_sparse: B = %d, q_top = %d, k = %d are not in 1 <= B <= 64, 1 <= q_top <= 1024, "
               "1 <= k <= 128 with four queries' image in LDS\n", B, q_top, k);
        return -1;
    }
    Ordered o(sp.ord, s);
    sp.last_passes = (B + NQ - 1) / NQ;
    const ScanMask mask(sp, f);
    return launch_sparse_scan_batch(sp.store, sp.table, sp.d_used, (int)sp.n_docs, sp.V, d_terms, d_weights, B, q_top, k,
                                    sp.qimage, sp.partial, d_scores, d_ids, s, sp.grid_cap, &sp.last_grid, mask.get());
}

// Inverts the blocks that are not yet inverted, or have grown, on s.  The first call
// allocates the image for the store's whole capacity.
int32_t build_inverted_locked(bertx_spindex &sp, hipStream_t s)
{
    if (sp.inverted_docs == sp.n_docs) return 0;
    const size_t need = sparse_inv_rows_bytes(sp.cap_docs, sp.V, sp.inv_block);
    if (!sp.inv || sp.inv_rows_bytes < need) {
        HIP_RC(sp.ord.wait());   // inv_block changes only while nothing is inverted: no row is lost
        if (sp.inv_rows) (void)hipFree(sp.inv_rows);
        sp.inv_rows = nullptr;
        sp.inv_rows_bytes = 0;
        if (hipMalloc((void **)&sp.inv_rows, need) != hipSuccess ||
            (!sp.inv && hipMalloc((void **)&sp.inv, (size_t)sp.cap_units * 64) != hipSuccess)) {
            (void)hipGetLastError();
            errorf("bertx_spindex_build_inverted: device %d could not allocate %zu bytes\n", sp.ordinal,
                   need + (size_t)sp.cap_units * 64);
            return -2;
        }
        sp.inv_rows_bytes = need;
    }
    const int64_t d0 = sp.inverted_docs / sp.inv_block * sp.inv_block;
    Ordered o(sp.ord, s);
    const int rc = launch_sparse_invert(sp.store, sp.table, (int)d0, (int)sp.n_docs, sp.V, sp.inv_block, sp.inv_rows, sp.inv, s);
    if (rc != 0) {
        errorf("bertx_spindex_build_inverted: device %d refused a launch (%d)\n", sp.ordinal, rc);
        return rc;
    }
    sp.inverted_docs = sp.n_docs;
    return 0;
}

int32_t search_inverted_device_locked(bertx_spindex &sp, const int32_t *d_terms, const float *d_weights, int32_t B,
                                      int32_t q_top, int32_t k, float *d_scores, int32_t *d_ids, hipStream_t s,
                                      const Filters &f = Filters())
{
    if (!d_terms || !d_weights || !d_scores || !d_ids || B < 1 || B > 64 || q_top < 1 || q_top > 1024 || k < 1 || k > 128) {
        errorf("bertx_spindex_search_inverted: B = %d, q_top = %d, k = %d are not in 1 <= B <= 64, 1 <= q_top <= 1024, "
               "1 <= k <= 128\n", B, q_top, k);
        return -1;
    }
    if (sp.inverted_docs != sp.n_docs) {
        errorf("bertx_spindex_search_inverted: %lld of %lld documents are inverted; call bertx_spindex_build_inverted\n",
               (long long)sp.inverted_docs, (long long)sp.n_docs);
        return -1;
    }
    Ordered o(sp.ord, s);
    sp.last_passes = 1;
    const ScanMask mask(sp, f);
    if (sp.n_docs == 0) {   // nothing was ever built: the scan of an empty store gives the fill
        return launch_sparse_scan_batch(sp.store, sp.table, sp.d_used, 0, sp.V, d_terms, d_weights, B, q_top, k, sp.qimage,
                                        sp.partial, d_scores, d_ids, s, sp.grid_cap, &sp.last_grid, mask.get());
    }
    return launch_sparse_inv_search(sp.inv, sp.inv_rows, sp.table, (int)sp.n_docs, sp.V, sp.inv_block, d_terms, d_weights, B,
                                    q_top, k, sp.partial, d_scores, d_ids, s, sp.grid_cap, &sp.last_grid, mask.get());
}

// The scorer of listed documents on s: a deleted document as an id the store does not hold.
int32_t score_ids_device_locked(bertx_spindex &sp, const int32_t *d_terms, const float *d_weights, int32_t B, int32_t q_top,
                                const int32_t *d_ids, int32_t n, float *d_scores, hipStream_t s)
{
    if (!d_terms || !d_weights || !d_ids || !d_scores || B < 1 || B > 64 || q_top < 1 || q_top > 1024 || n < 1 || n > 128) {
        errorf("bertx_spindex_score_ids: B = %d, q_top = %d, n = %d are not in 1 <= B <= 64, 1 <= q_top <= 1024, "
               "1 <= n <= 128\n", B, q_top, n);
        return -1;
    }
    Ordered o(sp.ord, s);
    sp.last_masked = sp.removed;
    return launch_sparse_score_ids(sp.store, sp.table, (int)sp.n_docs, sp.V, d_terms, d_weights, B, q_top, d_ids, n,
                                   d_scores, s, sp.removed ? sp.tomb : nullptr);
}

constexpr size_t kHybWords = 64 * 128;   // words of one of the hybrid search's seven buffers

// The hybrid search on s (sp locked, its device current; ix is locked by each of its entries):
// every refusal comes before the first launch.
int32_t hybrid_device_locked(bertx_index *ix, bertx_spindex &sp, const float *d_q, const int32_t *d_terms,
                             const float *d_weights, int32_t B, int32_t q_top, int32_t k, int32_t n_cand, int32_t mode,
                             float a, float b, float *d_scores, int32_t *d_ids, hipStream_t s)
{
    const int32_t fusion = mode & ~BERTX_HYBRID_INVERTED;
    const bool inverted = (mode & BERTX_HYBRID_INVERTED) != 0, rrf = fusion == BERTX_FUSE_RRF;
    if (!ix || !d_q || !d_terms || !d_weights || !d_scores || !d_ids || B < 1 || B > 64 || q_top < 1 || q_top > 1024 ||
        n_cand < 1 || n_cand > 64 || k < 1 || k > 2 * n_cand || (fusion != BERTX_FUSE_LINEAR && !rrf) ||
        (!inverted && sparse_batch_queries(sp.V, q_top, n_cand) == 0)) {
        errorf("bertx_hybrid_search: B = %d, q_top = %d, k = %d, n_cand = %d, mode = %d are not in 1 <= B <= 64, "
               "1 <= q_top <= 1024, 1 <= n_cand <= 64, 1 <= k <= 2 n_cand, BERTX_FUSE_LINEAR or _RRF\n", B, q_top, k, n_cand,
               mode);
        return -1;
    }
    if (index_ordinal(ix) != sp.ordinal) {
        errorf("bertx_hybrid_search: the embedding index lies on device %d, the sparse index on device %d\n",
               index_ordinal(ix), sp.ordinal);
        return -1;
    }
    if (inverted && sp.inverted_docs != sp.n_docs) {
        errorf("bertx_hybrid_search: %lld of %lld documents are inverted; call bertx_spindex_build_inverted\n",
               (long long)sp.inverted_docs, (long long)sp.n_docs);
        return -1;
    }
    if (!sp.hyb) {
        if (capturing(s) || hipMalloc((void **)&sp.hyb, 7 * kHybWords * 4) != hipSuccess) {
            (void)hipGetLastError();
            sp.hyb = nullptr;
            errorf("bertx_hybrid_search: the first call on a sparse index allocates %zu bytes and cannot be captured\n",
                   7 * kHybWords * 4);
            return -2;
        }
    }
    int32_t *cd = sp.hyb, *cs = cd + kHybWords, *U = cs + kHybWords, *rd = U + kHybWords, *rs = rd + kHybWords;
    float *sd = (float *)(rs + kHybWords), *ss = sd + kHybWords;   // (first the stages' own scores)
    Ordered o(sp.ord, s);
    int32_t rc = bertx_index_search_device(ix, d_q, B, n_cand, sd, cd, s);
    if (rc == 0)
        rc = (inverted ? search_inverted_device_locked : search_sparse_device_locked)(sp, d_terms, d_weights, B, q_top, n_cand,
                                                                                      ss, cs, s, Filters());
    if (rc == 0) rc = launch_hybrid_union(cd, cs, B, n_cand, U, rd, rs, s);
    if (rc == 0 && !rrf) rc = bertx_index_score_ids_device(ix, d_q, B, U, 2 * n_cand, sd, s);
    if (rc == 0 && !rrf) rc = score_ids_device_locked(sp, d_terms, d_weights, B, q_top, U, 2 * n_cand, ss, s);
    if (rc == 0) rc = launch_hybrid_fuse(U, rd, rs, sd, ss, B, n_cand, k, rrf, a, b, d_scores, d_ids, s);
    return rc;
}

// The results of a search launched on the store's stream into st_scores / st_ids (rc: its
// return value) -> the host.
int32_t results_to_host(bertx_spindex &sp, int32_t rc, int32_t B, int32_t k, float *scores, int32_t *ids)
{
    if (rc != 0) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(sp.stream);
        return rc;
    }
    HIP_RC(hipMemcpyAsync(scores, sp.st_scores, (size_t)B * k * 4, hipMemcpyDeviceToHost, sp.stream));
    HIP_RC(hipMemcpyAsync(ids, sp.st_ids, (size_t)B * k * 4, hipMemcpyDeviceToHost, sp.stream));
    HIP_RC(hipStreamSynchronize(sp.stream));
    return 0;
}

// B dense queries on the device, on the store's stream -> host results.
int32_t search_to_host(bertx_spindex &sp, const float *d_q, int32_t B, int32_t k, float *scores, int32_t *ids,
                       const Filters &f = Filters())
{
    return results_to_host(sp, search_device_locked(sp, d_q, B, k, sp.st_scores, sp.st_ids, sp.stream, f), B, k, scores, ids);
}

// The refusals of the text forms: -6 a file without the MLM records, -1 another vocabulary or
// no replica on the store's device.
int32_t text_ctx_ok(bertx_spindex *sp, struct bert_ctx *ctx, const char *who, int32_t *slot)
{
    if (!sp || !ctx) return -1;
    if (bertx_sparse_width(ctx) <= 0) {
        errorf("%s: this model file has no masked-LM head (cls.predictions.*)\n", who);
        return -6;
    }
    if (bertx_num_devices(ctx) == 0 || bertx_sparse_width(ctx) != sp->V) {
        errorf("%s: the context gives rows of %d terms, the store holds %d\n", who, bertx_sparse_width(ctx), sp->V);
        return -1;
    }
    for (int32_t s = 0; s < bertx_num_devices(ctx); ++s)
        if (bertx_device_ordinal(ctx, s) == sp->ordinal) {
            *slot = s;
            return 0;
        }
    errorf("%s: the context has no replica on the store's device %d\n", who, sp->ordinal);
    return -1;
}

struct Texts {
    std::vector<int32_t> ids, lens;
    size_t stride = 0;
};

int32_t tokenize(struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts, Texts &t)
{
    t.stride = (size_t)bert_n_max_tokens(ctx);
    t.ids.resize((size_t)n * t.stride);
    t.lens.resize((size_t)n);
    return bertx_tokenize_batch(ctx, n_threads, n, texts, (int32_t)t.stride, t.ids.data(), t.lens.data()) != 0 ? -1 : 0;
}

// Texts i0 .. i1 - 1 (at most kStage) through one sparse forward on `stream` into d_out f32
// [i1 - i0][n_vocab]; d_tok: the call's device buffer of ids and offsets, grown as needed.
int32_t forward_chunk(hipStream_t stream, float *d_out, struct bert_ctx *ctx, int32_t slot, const Texts &t, size_t i0,
                      size_t i1, std::vector<int32_t> &flat, DevBuf &d_tok, size_t *cap)
{
    flat.clear();
    std::vector<int32_t> cu(1, 0);
    int32_t max_len = 0;
    for (size_t i = i0; i < i1; ++i) {
        const int32_t *p = t.ids.data() + i * t.stride, len = t.lens[i];
        flat.insert(flat.end(), p, p + len);
        cu.push_back((int32_t)flat.size());
        max_len = std::max(max_len, len);
    }
    const size_t tok = flat.size(), seqs = i1 - i0;
    flat.insert(flat.end(), cu.begin(), cu.end());
    if (flat.size() > *cap) {
        if (d_tok.p) {
            HIP_RC(hipStreamSynchronize(stream));
            (void)hipFree(d_tok.p);
            d_tok.p = nullptr;
        }
        HIP_RC(hipMalloc(&d_tok.p, flat.size() * 4));
        *cap = flat.size();
    }
    if (bertx_reserve(ctx, slot, (int32_t)tok, (int32_t)seqs) != 0) return -1;
    HIP_RC(hipMemcpyAsync(d_tok.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_RC(hipStreamSynchronize(stream));   // flat is pageable and reused
    const int32_t *d = (const int32_t *)d_tok.p;
    return bertx_forward_sparse_device(ctx, slot, d, nullptr, d + tok, (int32_t)seqs, max_len, (int32_t)tok, d_out,
                                       stream);
}

}  // namespace

bertx_spindex *spindex_create_on(int ordinal, int V, int n_top, int64_t cap_docs, int64_t cap_postings)
{
    if (V < 1 || V > 65536 || n_top < 1 || n_top > 1024) {
        errorf("bertx_spindex_create: n_vocab %d / n_top %d are not in 1 .. 65536 / 1 .. 1024\n", V, n_top);
        return nullptr;
    }
    if (cap_docs < 1 || cap_docs > 0x7ffffff0ll || cap_postings < 16 || cap_postings > (0x7ffffff0ll << 4)) {
        errorf("bertx_spindex_create: capacity of %lld documents / %lld postings is not in 1 .. 2^31 - 16 / "
               "16 .. 2^35 - 256\n", (long long)cap_docs, (long long)cap_postings);
        return nullptr;
    }
    DeviceGuard g(ordinal);
    if (!g.ok()) {
        errorf("bertx_spindex_create: cannot select device %d\n", ordinal);
        return nullptr;
    }
    bertx_spindex *sp = new (std::nothrow) bertx_spindex();
    if (!sp) return nullptr;
    sp->ordinal = ordinal;
    sp->V = V;
    sp->n_top = n_top;
    sp->cap_docs = cap_docs;
    sp->cap_units = units_of(cap_postings);
    sp->tomb_words = index_mask_words(cap_docs);
    const size_t sel = (size_t)kSparseAddRows * n_top * 4;
    const size_t stq = (size_t)kStage * 1024 * 4;
    const bool ok = sparse_scan_prepare_device() == 0 && sparse_batch_prepare_device() == 0 &&
                    sparse_inv_prepare_device() == 0 &&
                    hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&sp->ord.done, hipEventDisableTiming) == hipSuccess &&
                    hipMalloc((void **)&sp->store, (size_t)sp->cap_units * 64) == hipSuccess &&
                    hipMalloc((void **)&sp->table, (size_t)cap_docs * 8) == hipSuccess &&
                    hipMalloc((void **)&sp->d_used, 16) == hipSuccess &&
                    hipMalloc((void **)&sp->sel_terms, sel) == hipSuccess &&
                    hipMalloc((void **)&sp->sel_weights, sel) == hipSuccess &&
                    hipMalloc((void **)&sp->sel_count, (size_t)kSparseAddRows * 4) == hipSuccess &&
                    hipMalloc((void **)&sp->st_rows, (size_t)kStage * V * 4) == hipSuccess &&
                    hipMalloc((void **)&sp->st_scores, 64 * 128 * 4) == hipSuccess &&
                    hipMalloc((void **)&sp->st_ids, 64 * 128 * 4) == hipSuccess &&
                    hipMalloc(&sp->qtab, sparse_scan_table_bytes(V)) == hipSuccess &&
                    hipMalloc(&sp->partial, std::max({sparse_scan_partial_bytes(), sparse_batch_partial_bytes(),
                                                     sparse_inv_partial_bytes()})) == hipSuccess &&
                    hipMalloc((void **)&sp->st_qterms, stq) == hipSuccess &&
                    hipMalloc((void **)&sp->st_qweights, stq) == hipSuccess &&
                    hipMalloc(&sp->qimage, sparse_batch_image_bytes()) == hipSuccess &&
                    hipMalloc((void **)&sp->tomb, (size_t)sp->tomb_words * 4) == hipSuccess &&
                    hipMemsetAsync(sp->tomb, 0, (size_t)sp->tomb_words * 4, sp->stream) == hipSuccess &&
                    hipMemsetAsync(sp->d_used, 0, 16, sp->stream) == hipSuccess &&
                    hipStreamSynchronize(sp->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        errorf("bertx_spindex_create: device %d could not allocate %zu bytes of postings (+ %lld table entries)\n", ordinal,
               (size_t)sp->cap_units * 64, (long long)cap_docs);
        delete sp;
        return nullptr;
    }
    return sp;
}

}  // namespace emb

using emb::DeviceGuard;

extern "C" {

struct bertx_spindex *bertx_spindex_create(struct bert_ctx *ctx, int32_t slot, int32_t n_vocab, int32_t n_top,
                                           int32_t capacity_docs, int64_t capacity_postings)
{
    if (!ctx || bertx_num_devices(ctx) == 0) {
        emb::errorf("bertx_spindex_create: no context with a device to hold a sparse index\n");
        return nullptr;
    }
    const int ordinal = bertx_device_ordinal(ctx, slot);
    if (ordinal < 0) {
        emb::errorf("bertx_spindex_create: slot %d is not one of the context's %d device(s)\n", slot,
                    bertx_num_devices(ctx));
        return nullptr;
    }
    return emb::spindex_create_on(ordinal, n_vocab, n_top, capacity_docs, capacity_postings);
}

void bertx_spindex_free(struct bertx_spindex *sp) { delete sp; }

int32_t bertx_spindex_clear(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    {
        emb::Ordered o(sp->ord, sp->stream);
        HIP_RC(hipMemsetAsync(sp->d_used, 0, 4, sp->stream));
        if (sp->removed) {   // the tombstones back to zero, ordered behind every operation so far
            HIP_RC(hipMemsetAsync(sp->tomb, 0, (size_t)sp->tomb_words * 4, sp->stream));
            sp->removed = false;
        }
    }
    sp->n_docs = 0;
    sp->used_bound = 0;
    sp->inverted_docs = 0;
    return 0;
}

int32_t bertx_spindex_docs(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    return (int32_t)sp->n_docs;
}

int64_t bertx_spindex_postings(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    int64_t used = 0;
    if (emb::read_used(*sp, &used) != 0) return -1;
    return used * 16;
}

int32_t bertx_spindex_capacity_docs(struct bertx_spindex *sp) { return sp ? (int32_t)sp->cap_docs : -1; }
int64_t bertx_spindex_capacity_postings(struct bertx_spindex *sp) { return sp ? sp->cap_units * 16 : -1; }
int32_t bertx_spindex_vocab(struct bertx_spindex *sp) { return sp ? sp->V : -1; }
int32_t bertx_spindex_top(struct bertx_spindex *sp) { return sp ? sp->n_top : -1; }

int32_t bertx_spindex_add_device(struct bertx_spindex *sp, const float *d_rows, int32_t n, void *stream)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    return emb::add_device_locked(*sp, d_rows, n, stream ? (hipStream_t)stream : sp->stream, "bertx_spindex_add_device");
}

int32_t bertx_spindex_add(struct bertx_spindex *sp, const float *rows, int32_t n)
{
    if (!sp || !rows || n < 1) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    if (const int32_t rc = emb::room_for(*sp, "bertx_spindex_add", n, (int64_t)n * emb::units_of(sp->n_top))) return rc;
    const int32_t first = (int32_t)sp->n_docs;
    for (int32_t i = 0; i < n; i += kStage) {
        const int32_t m = std::min<int32_t>(kStage, n - i);
        {
            emb::Ordered o(sp->ord, sp->stream);
            HIP_RC(hipMemcpyAsync(sp->st_rows, rows + (size_t)i * sp->V, (size_t)m * sp->V * 4, hipMemcpyHostToDevice,
                                  sp->stream));
        }
        const int32_t rc = emb::add_device_locked(*sp, sp->st_rows, m, sp->stream, "bertx_spindex_add");
        if (hipStreamSynchronize(sp->stream) != hipSuccess || rc < 0) {   // the staging buffer is reused
            (void)hipGetLastError();
            return rc < 0 ? rc : -1;
        }
    }
    return first;
}

int32_t bertx_spindex_add_postings(struct bertx_spindex *sp, const int32_t *terms, const float *weights,
                                   const int32_t *lens, int32_t n)
{
    if (!sp || !lens || n < 1) return -1;
    int64_t total = 0, units = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (lens[i] < 0 || lens[i] > sp->n_top) {
            emb::errorf("bertx_spindex_add_postings: document %d has %d postings, not 0 .. n_top = %d\n", i, lens[i], sp->n_top);
            return -1;
        }
        total += lens[i];
        units += emb::units_of(lens[i]);
    }
    if (total > 0 && (!terms || !weights)) return -1;
    // the postings as the device packs them
    std::vector<uint32_t> img((size_t)units * 16, 0u);
    std::vector<int32_t> tab((size_t)n * 2);
    int64_t j0 = 0, u0 = 0;
    for (int32_t i = 0; i < n; ++i) {
        for (int32_t j = 0; j < lens[i]; ++j) {
            const int32_t t = terms[j0 + j];
            const float w = weights[j0 + j];
            const uint16_t h = std::isfinite(w) && w >= 0.f ? emb::f32_to_f16(w) : (uint16_t)0x7c00;
            if (t < 0 || t >= sp->V || (j > 0 && t <= terms[j0 + j - 1]) || h >= 0x7c00) {
                emb::errorf("bertx_spindex_add_postings: document %d, posting %d: terms ascend without repeats below "
                            "n_vocab = %d, weights are finite in f16 and not negative\n", i, j, sp->V);
                return -1;
            }
            img[(size_t)u0 * 16 + (size_t)j] = (uint32_t)t | (uint32_t)h << 16;
        }
        tab[2 * (size_t)i] = (int32_t)u0;   // relative to the call's first unit
        tab[2 * (size_t)i + 1] = lens[i];
        j0 += lens[i];
        u0 += emb::units_of(lens[i]);
    }
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    if (const int32_t rc = emb::room_for(*sp, "bertx_spindex_add_postings", n, units)) return rc;
    int64_t used = 0;
    if (emb::read_used(*sp, &used) != 0) return -1;   // a host form: the exact offset, read from the device
    for (int32_t i = 0; i < n; ++i) tab[2 * (size_t)i] += (int32_t)used;
    const int32_t new_used = (int32_t)(used + units);
    {
        emb::Ordered o(sp->ord, sp->stream);
        if (units) HIP_RC(hipMemcpyAsync(sp->store + (size_t)used * 16, img.data(), img.size() * 4, hipMemcpyHostToDevice, sp->stream));
        HIP_RC(hipMemcpyAsync(sp->table + 2 * (size_t)sp->n_docs, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, sp->stream));
        HIP_RC(hipMemcpyAsync(sp->d_used, &new_used, 4, hipMemcpyHostToDevice, sp->stream));
    }
    HIP_RC(hipStreamSynchronize(sp->stream));   // the images are pageable and leave scope
    const int32_t first = (int32_t)sp->n_docs;
    sp->n_docs += n;
    sp->used_bound = new_used;
    return first;
}

int32_t bertx_spindex_doc_len(struct bertx_spindex *sp, int32_t id)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (id < 0 || id >= sp->n_docs) return -1;
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    HIP_RC(sp->ord.wait());
    int32_t e[2] = {0, 0};
    HIP_RC(hipMemcpy(e, sp->table + 2 * (size_t)id, 8, hipMemcpyDeviceToHost));
    return e[1];
}

int32_t bertx_spindex_doc(struct bertx_spindex *sp, int32_t id, int32_t *terms, float *weights)
{
    if (!sp || !terms || !weights) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (id < 0 || id >= sp->n_docs) return -1;
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    HIP_RC(sp->ord.wait());
    int32_t e[2] = {0, 0};
    HIP_RC(hipMemcpy(e, sp->table + 2 * (size_t)id, 8, hipMemcpyDeviceToHost));
    std::vector<uint32_t> p((size_t)e[1]);
    if (e[1]) HIP_RC(hipMemcpy(p.data(), sp->store + (size_t)e[0] * 16, p.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t j = 0; j < e[1]; ++j) {
        terms[j] = (int32_t)(p[(size_t)j] & 0xffffu);
        weights[j] = emb::f16_to_f32((uint16_t)(p[(size_t)j] >> 16));
    }
    return e[1];
}

int32_t bertx_spindex_search_filtered_device(struct bertx_spindex *sp, const float *d_queries, int32_t B, int32_t k,
                                             const uint32_t *d_filters, int32_t n_filters, int32_t words, float *d_scores,
                                             int32_t *d_ids, void *stream)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (!emb::filters_fit(sp->n_docs, d_filters, n_filters, words, B)) return -1;
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    return emb::search_device_locked(*sp, d_queries, B, k, d_scores, d_ids, stream ? (hipStream_t)stream : sp->stream,
                                     emb::filters_of(d_filters, n_filters, words));
}

int32_t bertx_spindex_search_device(struct bertx_spindex *sp, const float *d_queries, int32_t B, int32_t k, float *d_scores,
                                    int32_t *d_ids, void *stream)
{
    return bertx_spindex_search_filtered_device(sp, d_queries, B, k, nullptr, 0, 0, d_scores, d_ids, stream);
}

int32_t bertx_spindex_search_filtered(struct bertx_spindex *sp, const float *queries, int32_t B, int32_t k,
                                      const uint32_t *filters, int32_t n_filters, int32_t words, float *scores, int32_t *ids)
{
    if (!sp || !queries || !scores || !ids || B < 1 || B > kStage) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (!emb::filters_fit(sp->n_docs, filters, n_filters, words, B)) return -1;
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    emb::DevBuf fbuf;   // (freed after the call's synchronise)
    {
        emb::Ordered o(sp->ord, sp->stream);
        HIP_RC(hipMemcpyAsync(sp->st_rows, queries, (size_t)B * sp->V * 4, hipMemcpyHostToDevice, sp->stream));
        HIP_RC(emb::stage_filters(sp->stream, filters, n_filters, words, fbuf));
    }
    HIP_RC(hipStreamSynchronize(sp->stream));   // the caller's rows are pageable
    return emb::search_to_host(*sp, sp->st_rows, B, k, scores, ids,
                               emb::filters_of((const uint32_t *)fbuf.p, n_filters, words));
}

int32_t bertx_spindex_search(struct bertx_spindex *sp, const float *queries, int32_t B, int32_t k, float *scores,
                             int32_t *ids)
{
    return bertx_spindex_search_filtered(sp, queries, B, k, nullptr, 0, 0, scores, ids);
}

int32_t bertx_spindex_remove_device(struct bertx_spindex *sp, const int32_t *d_ids, int32_t n, void *stream)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    return emb::remove_device_locked(*sp, d_ids, n, stream ? (hipStream_t)stream : sp->stream);
}

int32_t bertx_spindex_remove(struct bertx_spindex *sp, const int32_t *ids, int32_t n)
{
    if (!sp || !ids || n < 1) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    for (int32_t i = 0; i < n; i += emb::kStageIds) {
        const int32_t m = std::min(emb::kStageIds, n - i);
        {
            emb::Ordered o(sp->ord, sp->stream);
            HIP_RC(hipMemcpyAsync(sp->st_ids, ids + i, (size_t)m * 4, hipMemcpyHostToDevice, sp->stream));
        }
        const int32_t rc = emb::remove_device_locked(*sp, sp->st_ids, m, sp->stream);
        if (rc != 0) return rc;
        HIP_RC(hipStreamSynchronize(sp->stream));   // the staging buffer is reused
    }
    return 0;
}

int32_t bertx_spindex_live(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    int32_t dead = 0;
    {
        emb::Ordered o(sp->ord, sp->stream);
        const int rc = emb::launch_index_count_deleted(sp->tomb, sp->n_docs, sp->st_ids, sp->stream);
        if (rc != 0) return rc;
        HIP_RC(hipMemcpyAsync(&dead, sp->st_ids, 4, hipMemcpyDeviceToHost, sp->stream));
    }
    HIP_RC(hipStreamSynchronize(sp->stream));
    return (int32_t)sp->n_docs - dead;
}

int32_t bertx_spindex_deleted(struct bertx_spindex *sp, int32_t first, int32_t n, uint8_t *out)
{
    if (!sp || !out || first < 0 || n < 1) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    if ((int64_t)first + n > sp->n_docs) return -1;
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    // the caller's output is written only once every chunk has succeeded
    std::vector<uint8_t> flags((size_t)n);
    constexpr int32_t kChunk = emb::kStageIds * 4;   // bytes of the id staging buffer, one flag each
    for (int32_t i = 0; i < n; i += kChunk) {
        const int32_t m = std::min(kChunk, n - i);
        {
            emb::Ordered o(sp->ord, sp->stream);
            const int rc = emb::launch_index_deleted_flags(sp->tomb, (int64_t)first + i, m, (uint8_t *)sp->st_ids, sp->stream);
            if (rc != 0) return rc;
            HIP_RC(hipMemcpyAsync(flags.data() + i, sp->st_ids, (size_t)m, hipMemcpyDeviceToHost, sp->stream));
        }
        HIP_RC(hipStreamSynchronize(sp->stream));
    }
    std::memcpy(out, flags.data(), flags.size());
    return 0;
}

int32_t bertx_spindex_add_texts(struct bertx_spindex *sp, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                const char **texts)
{
    int32_t slot = -1;
    if (const int32_t rc = emb::text_ctx_ok(sp, ctx, "bertx_spindex_add_texts", &slot)) return rc;
    if (!texts || n < 1) return -1;
    emb::Texts t;
    if (emb::tokenize(ctx, n_threads, n, texts, t) != 0) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    if (const int32_t rc = emb::room_for(*sp, "bertx_spindex_add_texts", n, (int64_t)n * emb::units_of(sp->n_top))) return rc;
    const int32_t first = (int32_t)sp->n_docs;
    std::vector<int32_t> flat;
    emb::DevBuf d_tok;
    size_t cap = 0;
    for (size_t i = 0; i < (size_t)n;) {
        const size_t e = emb::chunk_end([&](size_t j) { return t.lens[j]; }, i, (size_t)n, emb::kChunkTokens, kStage);
        int32_t rc = 0;
        {
            emb::Ordered o(sp->ord, sp->stream);
            rc = emb::forward_chunk(sp->stream, sp->st_rows, ctx, slot, t, i, e, flat, d_tok, &cap);
        }
        if (rc == 0) rc = emb::add_device_locked(*sp, sp->st_rows, (int32_t)(e - i), sp->stream, "bertx_spindex_add_texts");
        if (hipStreamSynchronize(sp->stream) != hipSuccess || rc < 0) {   // st_rows is reused by the next chunk
            (void)hipGetLastError();
            emb::errorf("bertx_spindex_add_texts: device %d failed while adding (%d)\n", sp->ordinal, rc);
            return rc < 0 ? rc : -1;
        }
        i = e;
    }
    return first;
}

int32_t bertx_spindex_search_sparse_filtered_device(struct bertx_spindex *sp, const int32_t *d_terms,
                                                    const float *d_weights, int32_t B, int32_t q_top, int32_t k,
                                                    const uint32_t *d_filters, int32_t n_filters, int32_t words,
                                                    float *d_scores, int32_t *d_ids, void *stream)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (!emb::filters_fit(sp->n_docs, d_filters, n_filters, words, B)) return -1;
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    return emb::search_sparse_device_locked(*sp, d_terms, d_weights, B, q_top, k, d_scores, d_ids,
                                            stream ? (hipStream_t)stream : sp->stream,
                                            emb::filters_of(d_filters, n_filters, words));
}

int32_t bertx_spindex_search_sparse_device(struct bertx_spindex *sp, const int32_t *d_terms, const float *d_weights,
                                           int32_t B, int32_t q_top, int32_t k, float *d_scores, int32_t *d_ids, void *stream)
{
    return bertx_spindex_search_sparse_filtered_device(sp, d_terms, d_weights, B, q_top, k, nullptr, 0, 0, d_scores, d_ids,
                                                       stream);
}

namespace {
// What the host forms accept as sparse queries; a message otherwise.
bool queries_ok(int32_t V, const int32_t *terms, const float *weights, int32_t B, int32_t q_top)
{
    if (!terms || !weights || B < 1 || B > kStage || q_top < 1 || q_top > 1024) return false;
    std::vector<int32_t> seen((size_t)V, -1);   // the query that last held the term
    for (int32_t b = 0; b < B; ++b)
        for (int32_t j = 0; j < q_top; ++j) {
            const int32_t t = terms[(size_t)b * q_top + j];
            if (t < 0) continue;   // an empty slot
            if (t >= V || seen[(size_t)t] == b || !std::isfinite(weights[(size_t)b * q_top + j])) {
                emb::errorf("bertx_spindex_search_sparse: query %d, slot %d: terms are below n_vocab = %d and distinct "
                            "within a query, weights are finite\n", b, j, V);
                return false;
            }
            seen[(size_t)t] = b;
        }
    return true;
}

// The sparse queries of a host form into the staging buffers, on the store's stream (sp locked; the
// caller orders the copies and synchronises before its arrays leave scope).
hipError_t stage_queries(struct bertx_spindex *sp, const int32_t *terms, const float *weights, int32_t B, int32_t q_top)
{
    const hipError_t e = hipMemcpyAsync(sp->st_qterms, terms, (size_t)B * q_top * 4, hipMemcpyHostToDevice, sp->stream);
    return e != hipSuccess ? e : hipMemcpyAsync(sp->st_qweights, weights, (size_t)B * q_top * 4, hipMemcpyHostToDevice, sp->stream);
}

// The host forms of the two sparse-query searches: the refusals, the staging, the search
// (inverted: over the inverted lists, built first when stale) and the results.
int32_t search_sparse_host(struct bertx_spindex *sp, const int32_t *terms, const float *weights, int32_t B, int32_t q_top,
                           int32_t k, const uint32_t *filters, int32_t n_filters, int32_t words, float *scores, int32_t *ids,
                           bool inverted)
{
    if (!sp || !scores || !ids || !queries_ok(sp->V, terms, weights, B, q_top)) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (!emb::filters_fit(sp->n_docs, filters, n_filters, words, B)) return -1;
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    emb::DevBuf fbuf;   // (freed after the call's synchronise)
    {
        emb::Ordered o(sp->ord, sp->stream);
        HIP_RC(stage_queries(sp, terms, weights, B, q_top));
        HIP_RC(emb::stage_filters(sp->stream, filters, n_filters, words, fbuf));
    }
    HIP_RC(hipStreamSynchronize(sp->stream));   // the caller's arrays are pageable
    const emb::Filters f = emb::filters_of((const uint32_t *)fbuf.p, n_filters, words);
    int32_t rc = inverted ? emb::build_inverted_locked(*sp, sp->stream) : 0;
    if (rc == 0)
        rc = (inverted ? emb::search_inverted_device_locked : emb::search_sparse_device_locked)(
            *sp, sp->st_qterms, sp->st_qweights, B, q_top, k, sp->st_scores, sp->st_ids, sp->stream, f);
    return emb::results_to_host(*sp, rc, B, k, scores, ids);
}
}  // namespace

int32_t bertx_spindex_search_sparse_filtered(struct bertx_spindex *sp, const int32_t *terms, const float *weights, int32_t B,
                                             int32_t q_top, int32_t k, const uint32_t *filters, int32_t n_filters,
                                             int32_t words, float *scores, int32_t *ids)
{
    return search_sparse_host(sp, terms, weights, B, q_top, k, filters, n_filters, words, scores, ids, false);
}

int32_t bertx_spindex_search_sparse(struct bertx_spindex *sp, const int32_t *terms, const float *weights, int32_t B,
                                    int32_t q_top, int32_t k, float *scores, int32_t *ids)
{
    return search_sparse_host(sp, terms, weights, B, q_top, k, nullptr, 0, 0, scores, ids, false);
}

int32_t bertx_spindex_search_inverted_filtered(struct bertx_spindex *sp, const int32_t *terms, const float *weights,
                                               int32_t B, int32_t q_top, int32_t k, const uint32_t *filters,
                                               int32_t n_filters, int32_t words, float *scores, int32_t *ids)
{
    return search_sparse_host(sp, terms, weights, B, q_top, k, filters, n_filters, words, scores, ids, true);
}

int32_t bertx_spindex_search_inverted(struct bertx_spindex *sp, const int32_t *terms, const float *weights, int32_t B,
                                      int32_t q_top, int32_t k, float *scores, int32_t *ids)
{
    return search_sparse_host(sp, terms, weights, B, q_top, k, nullptr, 0, 0, scores, ids, true);
}

int32_t bertx_spindex_search_inverted_filtered_device(struct bertx_spindex *sp, const int32_t *d_terms,
                                                      const float *d_weights, int32_t B, int32_t q_top, int32_t k,
                                                      const uint32_t *d_filters, int32_t n_filters, int32_t words,
                                                      float *d_scores, int32_t *d_ids, void *stream)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (!emb::filters_fit(sp->n_docs, d_filters, n_filters, words, B)) return -1;
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    return emb::search_inverted_device_locked(*sp, d_terms, d_weights, B, q_top, k, d_scores, d_ids,
                                              stream ? (hipStream_t)stream : sp->stream,
                                              emb::filters_of(d_filters, n_filters, words));
}

int32_t bertx_spindex_search_inverted_device(struct bertx_spindex *sp, const int32_t *d_terms, const float *d_weights,
                                             int32_t B, int32_t q_top, int32_t k, float *d_scores, int32_t *d_ids,
                                             void *stream)
{
    return bertx_spindex_search_inverted_filtered_device(sp, d_terms, d_weights, B, q_top, k, nullptr, 0, 0, d_scores, d_ids,
                                                         stream);
}

int32_t bertx_spindex_score_ids_device(struct bertx_spindex *sp, const int32_t *d_terms, const float *d_weights, int32_t B,
                                       int32_t q_top, const int32_t *d_ids, int32_t n, float *d_scores, void *stream)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    return emb::score_ids_device_locked(*sp, d_terms, d_weights, B, q_top, d_ids, n, d_scores,
                                        stream ? (hipStream_t)stream : sp->stream);
}

int32_t bertx_spindex_score_ids(struct bertx_spindex *sp, const int32_t *terms, const float *weights, int32_t B,
                                int32_t q_top, const int32_t *ids, int32_t n, float *scores)
{
    if (!sp || !ids || !scores || n < 1 || n > 128 || !queries_ok(sp->V, terms, weights, B, q_top)) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    {
        emb::Ordered o(sp->ord, sp->stream);
        HIP_RC(stage_queries(sp, terms, weights, B, q_top));
        HIP_RC(hipMemcpyAsync(sp->st_ids, ids, (size_t)B * n * 4, hipMemcpyHostToDevice, sp->stream));
    }
    HIP_RC(hipStreamSynchronize(sp->stream));
    const int32_t rc = emb::score_ids_device_locked(*sp, sp->st_qterms, sp->st_qweights, B, q_top, sp->st_ids, n,
                                                    sp->st_scores, sp->stream);
    if (rc == 0) HIP_RC(hipMemcpyAsync(scores, sp->st_scores, (size_t)B * n * 4, hipMemcpyDeviceToHost, sp->stream));
    HIP_RC(hipStreamSynchronize(sp->stream));
    return rc;
}

int32_t bertx_hybrid_search_device(struct bertx_index *ix, struct bertx_spindex *sp, const float *d_queries,
                                   const int32_t *d_terms, const float *d_weights, int32_t B, int32_t q_top, int32_t k,
                                   int32_t n_cand, int32_t mode, float a, float b, float *d_scores, int32_t *d_ids,
                                   void *stream)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    return emb::hybrid_device_locked(ix, *sp, d_queries, d_terms, d_weights, B, q_top, k, n_cand, mode, a, b, d_scores, d_ids,
                                     stream ? (hipStream_t)stream : sp->stream);
}

namespace {
// The host form's second half (sp locked, the sparse queries staged): the dense queries f32 [B][d]
// to a buffer of the call's own, the search on the store's stream, the results.
int32_t hybrid_to_host(struct bertx_index *ix, struct bertx_spindex *sp, const float *queries, int32_t B, int32_t q_top,
                       int32_t k, int32_t n_cand, int32_t mode, float a, float b, float *scores, int32_t *ids)
{
    const size_t qbytes = (size_t)B * (size_t)bertx_index_dim(ix) * 4;
    emb::DevBuf d_q;   // (freed after the call's synchronise)
    HIP_RC(hipMalloc(&d_q.p, qbytes));
    HIP_RC(hipMemcpyAsync(d_q.p, queries, qbytes, hipMemcpyHostToDevice, sp->stream));
    HIP_RC(hipStreamSynchronize(sp->stream));   // the caller's rows are pageable
    int32_t rc = (mode & BERTX_HYBRID_INVERTED) ? emb::build_inverted_locked(*sp, sp->stream) : 0;
    if (rc == 0)
        rc = emb::hybrid_device_locked(ix, *sp, (const float *)d_q.p, sp->st_qterms, sp->st_qweights, B, q_top, k, n_cand,
                                       mode, a, b, sp->st_scores, sp->st_ids, sp->stream);
    return emb::results_to_host(*sp, rc, B, k, scores, ids);
}
}  // namespace

int32_t bertx_hybrid_search(struct bertx_index *ix, struct bertx_spindex *sp, const float *queries, const int32_t *terms,
                            const float *weights, int32_t B, int32_t q_top, int32_t k, int32_t n_cand, int32_t mode,
                            float a, float b, float *scores, int32_t *ids)
{
    if (!ix || !sp || !queries || !scores || !ids || n_cand < 1 || n_cand > 64 || k < 1 || k > 2 * n_cand ||
        !queries_ok(sp->V, terms, weights, B, q_top))
        return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    {
        emb::Ordered o(sp->ord, sp->stream);
        HIP_RC(stage_queries(sp, terms, weights, B, q_top));
    }
    return hybrid_to_host(ix, sp, queries, B, q_top, k, n_cand, mode, a, b, scores, ids);
}

int32_t bertx_hybrid_search_texts(struct bertx_index *ix, struct bert_ctx *ctx_dense, struct bertx_spindex *sp,
                                  struct bert_ctx *ctx_sparse, int32_t n_threads, int32_t n, const char **texts,
                                  int32_t q_top, int32_t k, int32_t n_cand, int32_t mode, float a, float b, float *scores,
                                  int32_t *ids)
{
    int32_t slot = -1;
    if (const int32_t rc = emb::text_ctx_ok(sp, ctx_sparse, "bertx_hybrid_search_texts", &slot)) return rc;
    if (!ix || !ctx_dense || !texts || !scores || !ids || n < 1 || q_top < 1 || q_top > 1024 || n_cand < 1 || n_cand > 64 ||
        k < 1 || k > 2 * n_cand)
        return -1;
    const int32_t d = bertx_index_dim(ix);
    if (bertx_num_devices(ctx_dense) == 0 || bert_n_embd(ctx_dense) != d) {
        emb::errorf("bertx_hybrid_search_texts: the dense context cannot produce rows of width %d\n", d);
        return -1;
    }
    // the dense rows as bertx_index_search_texts makes them: one batch, refused as a whole
    std::vector<float> rows((size_t)n * d, 0.f);
    std::vector<float *> ptr((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        ptr[(size_t)i] = rows.data() + (size_t)i * d;
        *ptr[(size_t)i] = std::nanf("");
    }
    bert_encode_batch(ctx_dense, n_threads, n, n, texts, ptr.data());
    for (int32_t i = 0; i < n; ++i)
        if (std::isnan(*ptr[(size_t)i])) {
            emb::errorf("bertx_hybrid_search_texts: the encoder refused the texts; nothing was searched\n");
            return -4;
        }
    emb::Texts t;
    if (emb::tokenize(ctx_sparse, n_threads, n, texts, t) != 0) return -1;
    std::vector<float> hs((size_t)n * k);
    std::vector<int32_t> hi((size_t)n * k);
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    std::vector<int32_t> flat;
    emb::DevBuf d_tok;
    size_t cap = 0;
    for (size_t i = 0; i < (size_t)n;) {
        const size_t e = emb::chunk_end([&](size_t j) { return t.lens[j]; }, i, (size_t)n, emb::kChunkTokens, kStage);
        const int32_t m = (int32_t)(e - i);
        int32_t rc = 0;
        {
            emb::Ordered o(sp->ord, sp->stream);
            rc = emb::forward_chunk(sp->stream, sp->st_rows, ctx_sparse, slot, t, i, e, flat, d_tok, &cap);
            if (rc == 0)
                rc = emb::launch_sparse_select(sp->st_rows, m, sp->V, q_top, sp->st_qterms, sp->st_qweights, sp->sel_count,
                                               sp->stream);
        }
        if (rc == 0)
            rc = hybrid_to_host(ix, sp, rows.data() + i * d, m, q_top, k, n_cand, mode, a, b, hs.data() + i * k,
                                hi.data() + i * k);
        if (rc != 0) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(sp->stream);
            return rc < 0 ? rc : -1;
        }
        i = e;
    }
    std::memcpy(scores, hs.data(), hs.size() * 4);
    std::memcpy(ids, hi.data(), hi.size() * 4);
    return 0;
}

int32_t bertx_spindex_build_inverted(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    return emb::build_inverted_locked(*sp, sp->stream);
}

int32_t bertx_spindex_inverted_docs(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    return (int32_t)sp->inverted_docs;
}

int32_t bertx_spindex_inv_block(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    return sp->inv_block;
}

int64_t bertx_spindex_inverted_bytes(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    return sp->inv ? (int64_t)((size_t)sp->cap_units * 64 + sp->inv_rows_bytes) : 0;
}

int32_t bertx_test_spindex_inv_block(struct bertx_spindex *sp, int32_t docs)
{
    if (!sp || docs < 64 || docs > emb::kSparseInvBlock || docs % 64 != 0) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->inverted_docs != 0) return -1;
    sp->inv_block = docs;
    return 0;
}

namespace {
// The text searches: q_top == 0 searches the forward's dense rows, q_top > 0 selects the
// q_top largest weights of each row on the device and searches those (inverted: over the
// inverted lists, built first when stale).
int32_t search_texts(struct bertx_spindex *sp, struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts,
                     int32_t q_top, int32_t k, float *scores, int32_t *ids, const char *who, bool inverted = false)
{
    int32_t slot = -1;
    if (const int32_t rc = emb::text_ctx_ok(sp, ctx, who, &slot)) return rc;
    if (!texts || !scores || !ids || n < 1 || k < 1 || k > 128) return -1;
    emb::Texts t;
    if (emb::tokenize(ctx, n_threads, n, texts, t) != 0) return -1;
    std::vector<float> hs((size_t)n * k);
    std::vector<int32_t> hi((size_t)n * k);
    std::lock_guard<std::mutex> lk(sp->mu);
    DeviceGuard g(sp->ordinal);
    HIP_RC(g.status());
    std::vector<int32_t> flat;
    emb::DevBuf d_tok;
    size_t cap = 0;
    if (inverted)
        if (const int32_t rc = emb::build_inverted_locked(*sp, sp->stream)) return rc;
    const auto sparse_search = inverted ? emb::search_inverted_device_locked : emb::search_sparse_device_locked;
    for (size_t i = 0; i < (size_t)n;) {
        const size_t e = emb::chunk_end([&](size_t j) { return t.lens[j]; }, i, (size_t)n, emb::kChunkTokens, kStage);
        const int32_t m = (int32_t)(e - i);
        int32_t rc = 0;
        {
            emb::Ordered o(sp->ord, sp->stream);
            rc = emb::forward_chunk(sp->stream, sp->st_rows, ctx, slot, t, i, e, flat, d_tok, &cap);
            if (rc == 0 && q_top > 0)
                rc = emb::launch_sparse_select(sp->st_rows, m, sp->V, q_top, sp->st_qterms, sp->st_qweights, sp->sel_count,
                                               sp->stream);
        }
        if (rc == 0 && q_top > 0)
            rc = emb::results_to_host(*sp, sparse_search(*sp, sp->st_qterms, sp->st_qweights, m, q_top, k, sp->st_scores,
                                                         sp->st_ids, sp->stream, emb::Filters()),
                                      m, k, hs.data() + i * k, hi.data() + i * k);
        else if (rc == 0)
            rc = emb::search_to_host(*sp, sp->st_rows, m, k, hs.data() + i * k, hi.data() + i * k);
        if (rc != 0) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(sp->stream);
            return rc < 0 ? rc : -1;
        }
        i = e;
    }
    std::memcpy(scores, hs.data(), hs.size() * 4);
    std::memcpy(ids, hi.data(), hi.size() * 4);
    return 0;
}
}  // namespace

int32_t bertx_spindex_search_texts(struct bertx_spindex *sp, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                   const char **texts, int32_t k, float *scores, int32_t *ids)
{
    return search_texts(sp, ctx, n_threads, n, texts, 0, k, scores, ids, "bertx_spindex_search_texts");
}

int32_t bertx_spindex_search_texts_top(struct bertx_spindex *sp, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                       const char **texts, int32_t q_top, int32_t k, float *scores, int32_t *ids)
{
    if (q_top < 1 || q_top > 1024) return -1;
    return search_texts(sp, ctx, n_threads, n, texts, q_top, k, scores, ids, "bertx_spindex_search_texts_top");
}

int32_t bertx_spindex_search_texts_inverted(struct bertx_spindex *sp, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                            const char **texts, int32_t q_top, int32_t k, float *scores, int32_t *ids)
{
    if (q_top < 1 || q_top > 1024) return -1;
    return search_texts(sp, ctx, n_threads, n, texts, q_top, k, scores, ids, "bertx_spindex_search_texts_inverted", true);
}

int32_t bertx_spindex_batch_queries(struct bertx_spindex *sp, int32_t q_top, int32_t k)
{
    return sp ? emb::sparse_batch_queries(sp->V, q_top, k) : 0;
}

int32_t bertx_forward_sparse_top(struct bert_ctx *ctx, int32_t slot, int32_t n, bert_vocab_id **batch_tokens,
                                 int32_t *n_tokens, int32_t n_top, int32_t *terms, float *weights, int32_t *counts)
{
    if (!ctx || !batch_tokens || !n_tokens || !terms || !weights || !counts || n < 1 || n_top < 1 || n_top > 1024) return -1;
    const int32_t V = bertx_sparse_width(ctx);
    if (V <= 0) {
        emb::errorf("bertx_forward_sparse_top: this model file has no masked-LM head (cls.predictions.*)\n");
        return -6;
    }
    const int ordinal = bertx_num_devices(ctx) > 0 ? bertx_device_ordinal(ctx, slot) : -1;
    if (ordinal < 0 || V > 65536) return -1;
    emb::Texts t;
    t.lens.assign(n_tokens, n_tokens + n);
    for (int32_t i = 0; i < n; ++i) {
        if (n_tokens[i] < 1 || n_tokens[i] > bert_n_max_tokens(ctx)) return -1;
        t.stride = std::max(t.stride, (size_t)n_tokens[i]);
    }
    t.ids.assign((size_t)n * t.stride, 0);
    for (int32_t i = 0; i < n; ++i) std::memcpy(t.ids.data() + (size_t)i * t.stride, batch_tokens[i], (size_t)n_tokens[i] * 4);
    DeviceGuard g(ordinal);
    HIP_RC(g.status());
    struct Str {
        hipStream_t s = nullptr;
        ~Str() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    } S;
    HIP_RC(hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking));
    emb::DevBuf d_tok, d_rows, d_t, d_w, d_c;
    HIP_RC(hipMalloc(&d_rows.p, (size_t)kStage * V * 4));
    HIP_RC(hipMalloc(&d_t.p, (size_t)kStage * n_top * 4));
    HIP_RC(hipMalloc(&d_w.p, (size_t)kStage * n_top * 4));
    HIP_RC(hipMalloc(&d_c.p, (size_t)kStage * 4));
    std::vector<int32_t> flat;
    size_t cap = 0;
    for (size_t i = 0; i < (size_t)n;) {
        const size_t e = emb::chunk_end([&](size_t j) { return t.lens[j]; }, i, (size_t)n, emb::kChunkTokens, kStage);
        const int m = (int)(e - i);
        int32_t rc = emb::forward_chunk(S.s, (float *)d_rows.p, ctx, slot, t, i, e, flat, d_tok, &cap);
        if (rc == 0)
            rc = emb::launch_sparse_select((const float *)d_rows.p, m, V, n_top, (int32_t *)d_t.p, (float *)d_w.p,
                                           (int32_t *)d_c.p, S.s);
        if (rc != 0) return rc < 0 ? rc : -1;
        HIP_RC(hipMemcpyAsync(terms + i * n_top, d_t.p, (size_t)m * n_top * 4, hipMemcpyDeviceToHost, S.s));
        HIP_RC(hipMemcpyAsync(weights + i * n_top, d_w.p, (size_t)m * n_top * 4, hipMemcpyDeviceToHost, S.s));
        HIP_RC(hipMemcpyAsync(counts + i, d_c.p, (size_t)m * 4, hipMemcpyDeviceToHost, S.s));
        HIP_RC(hipStreamSynchronize(S.s));
        i = e;
    }
    return 0;
}

int32_t bertx_test_spindex_grid(struct bertx_spindex *sp, int32_t max_wg)
{
    if (!sp || max_wg < 0) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    sp->grid_cap = max_wg;
    return 0;
}

int32_t bertx_test_spindex_last_grid(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    return sp->last_grid;
}

int32_t bertx_test_spindex_last_passes(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    return sp->last_passes;
}

int32_t bertx_test_spindex_last_masked(struct bertx_spindex *sp)
{
    if (!sp) return -1;
    std::lock_guard<std::mutex> lk(sp->mu);
    return sp->last_masked;
}

}  // extern "C"
