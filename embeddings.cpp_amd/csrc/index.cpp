// The device-resident embedding index (bert_hip.h bertx_index_*): an append-only
// matrix of f16, int8 or binary rows in HBM in the search kernels' order (kernels.h),
// the fused top-k search over it, the scorer of listed rows, the two-stage search over
// two indexes, and the text forms on top of bert_encode_batch.
// After creation an index knows only its device ordinal, its width and its storage.
// The ordering of its device operations and the unpackers of the read-back forms are
// shared with the token store (store_common.h).
#include "bert.h"
#include "bert_hip.h"

#include "engine.h"
#include "hip_check.h"
#include "kmeans_update.h"
#include "store_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <vector>

struct bertx_index {
    int ordinal = 0;
    int d = 0;
    int storage = BERTX_INDEX_F16;
    int64_t cap = 0, n = 0;
    void *rows = nullptr;        // f16 or int8: ceil(cap / 16) groups in fragment order; binary: ceil(cap / 64) in bit order
    float *scales = nullptr;     // int8: one per row of the padded capacity
    // the tombstones (index_mask.hip): bit r % 32 of word r / 32 is 1 once row r was removed;
    // `removed`: some remove was accepted since creation or the last clear, so searches take
    // the masked kernels (read at launch time, as n is)
    uint32_t *tomb = nullptr;
    int64_t tomb_words = 0;
    bool removed = false;
    void *scratch = nullptr;     // partial lists of one search launch
    // the rescored search's candidates, kStage queries at a time, [kStage][128] each: what this
    // index (as the coarse one) found, and what the fine index made of it
    float *cand_s = nullptr, *cand_exact = nullptr;
    int32_t *cand_i = nullptr, *cand_kept = nullptr;
    // staging of the host forms, kStage rows or queries at a time
    float *st_rows = nullptr, *st_scores = nullptr;
    int32_t *st_ids = nullptr;
    // the lists (search_lists.hip; bert_hip.h "Lists and probed search"), n_lists == 0: none.
    // The clustered image covers rows [0, listed) in list_groups of its list_cap_groups groups.
    int32_t n_lists = 0;
    int64_t listed = 0, list_groups = 0, list_cap_groups = 0;
    void *cent = nullptr, *cent_scratch = nullptr;      // the centroids' f16 image, their search's partial lists
    uint32_t *goff = nullptr, *lcount = nullptr;        // [n_lists + 1] in groups, [n_lists]
    void *probe_partial = nullptr;                      // [64][min(n_lists, 128)][128] pairs
    int32_t *row_list = nullptr;                        // [cap]: the list of every covered row
    void *limage = nullptr;                             // the clustered image, its scales and row ids
    float *lscales = nullptr;
    int32_t *slot_id = nullptr;
    int32_t *probe_ids = nullptr, *item_n = nullptr;    // one pass of the probed search: [64][128] each
    float *probe_scores = nullptr;
    uint32_t *pair_sorted = nullptr;
    hipStream_t stream = nullptr;
    emb::StoreOrder ord;
    std::mutex mu;
    ~bertx_index()
    {
        emb::DeviceGuard g(ordinal);
        // (no wait for ord.done, unlike the token store: an operation in flight on a caller's
        // stream reads device memory only, and hipFree waits for the device itself)
        if (stream) (void)hipStreamSynchronize(stream);
        for (void *p : {cent, cent_scratch, (void *)goff, (void *)lcount, probe_partial, (void *)row_list, limage,
                        (void *)lscales, (void *)slot_id, (void *)probe_ids, (void *)item_n, (void *)probe_scores,
                        (void *)pair_sorted})
            if (p) (void)hipFree(p);
        if (rows) (void)hipFree(rows);
        if (scales) (void)hipFree(scales);
        if (tomb) (void)hipFree(tomb);
        if (scratch) (void)hipFree(scratch);
        if (st_rows) (void)hipFree(st_rows);
        if (st_scores) (void)hipFree(st_scores);
        if (st_ids) (void)hipFree(st_ids);
        if (cand_s) (void)hipFree(cand_s);
        if (cand_exact) (void)hipFree(cand_exact);
        if (cand_i) (void)hipFree(cand_i);
        if (cand_kept) (void)hipFree(cand_kept);
        if (ord.done) (void)hipEventDestroy(ord.done);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace emb {
namespace {

constexpr int kStage = 256;   // rows / queries per staged chunk of the host forms
constexpr int kMaxK = 128;
constexpr int kStageIds = kStage * kMaxK;   // int32 values the id staging buffer holds

// What bertx_index_search_filtered accepts (idx locked; store_common.h filters_fit, which
// the token store shares with the Filters themselves).
bool filters_ok(const bertx_index &ix, const void *filters, int32_t n_filters, int32_t words, int32_t B)
{
    return filters_fit(ix.n, filters, n_filters, words, B);
}

bool kind_known(int storage)
{
    return storage == BERTX_INDEX_F16 || storage == BERTX_INDEX_I8 || storage == BERTX_INDEX_BIN;
}

void refuse_kind(int storage)
{
    errorf("bertx_index_create: storage %d is none of BERTX_INDEX_F16 (0), BERTX_INDEX_I8 (1), BERTX_INDEX_BIN (8)\n",
           storage);
}

int32_t add_device_locked(bertx_index &ix, const float *d_rows, int32_t n, hipStream_t s)
{
    if (!d_rows || n < 1) return -1;
    if (ix.n + n > ix.cap) {
        errorf("bertx_index_add: %d rows do not fit (%lld of %lld used)\n", n, (long long)ix.n, (long long)ix.cap);
        return -2;
    }
    {
        Ordered o(ix.ord, s);
        const int rc = ix.storage == BERTX_INDEX_BIN
                           ? launch_index_add_bin(d_rows, n, ix.d, ix.n, ix.rows, s)
                           : launch_index_add(d_rows, n, ix.d, ix.n, ix.storage, ix.rows, ix.scales, s);
        if (rc != 0) return rc;
    }
    const int32_t first = (int32_t)ix.n;
    ix.n += n;
    return first;
}

// the search of the index's kind on s (idx locked; the caller orders it): the unmasked
// kernels while nothing was removed and no filter is given, else the masked ones
int search_launch(bertx_index &ix, const float *d_q, int32_t B, int32_t k, float *d_scores, int32_t *d_ids, hipStream_t s,
                  const Filters &f)
{
    const SearchMask mask{ix.tomb, f.d, f.stride};
    const SearchMask *m = ix.removed || f.d ? &mask : nullptr;
    if (ix.storage == BERTX_INDEX_BIN)
        return launch_search_bin(ix.rows, ix.n, ix.d, d_q, B, k, ix.scratch, d_scores, d_ids, s, m);
    return launch_search(ix.rows, ix.scales, ix.storage, ix.n, ix.d, d_q, B, k, ix.scratch, d_scores, d_ids, s, m);
}

// the scorer of listed rows on s (idx locked; the caller orders it): a deleted row as an id the index does not hold
int score_ids_launch(bertx_index &ix, const float *d_q, int32_t B, const int32_t *d_ids, int32_t n, float *d_scores,
                     int32_t *d_kept, hipStream_t s)
{
    return launch_index_score_ids(ix.rows, ix.scales, ix.storage, ix.n, ix.d, d_q, B, d_ids, n, d_scores, d_kept, s,
                                  ix.removed ? ix.tomb : nullptr);
}

int32_t search_device_locked(bertx_index &ix, const float *d_q, int32_t B, int32_t k, float *d_scores, int32_t *d_ids,
                             hipStream_t s, const Filters &f = Filters())
{
    if (!d_q || !d_scores || !d_ids || B < 1 || k < 1 || k > kMaxK) return -1;
    Ordered o(ix.ord, s);
    return search_launch(ix, d_q, B, k, d_scores, d_ids, s, f);
}

int32_t remove_device_locked(bertx_index &ix, const int32_t *d_ids, int32_t n, hipStream_t s)
{
    if (!d_ids || n < 1) return -1;
    Ordered o(ix.ord, s);
    const int rc = launch_index_remove(d_ids, n, ix.n, ix.tomb, s);
    if (rc == 0) ix.removed = true;
    return rc;
}

int32_t score_ids_device_locked(bertx_index &ix, const float *d_q, int32_t B, const int32_t *d_ids, int32_t n,
                                float *d_scores, hipStream_t s)
{
    if (!d_q || !d_ids || !d_scores || B < 1 || n < 1 || n > kMaxK) return -1;
    Ordered o(ix.ord, s);
    return score_ids_launch(ix, d_q, B, d_ids, n, d_scores, nullptr, s);
}

// What the two indexes of a rescored search must be to each other; a message otherwise.
bool rescored_pair_ok(const bertx_index *coarse, const bertx_index *fine, const char *who)
{
    if (!coarse || !fine) return false;
    if (coarse == fine) {
        errorf("%s: coarse and fine are the same index\n", who);
        return false;
    }
    if (coarse->d != fine->d || coarse->ordinal != fine->ordinal) {
        errorf("%s: coarse (width %d, device %d) and fine (width %d, device %d) do not match\n", who, coarse->d,
               coarse->ordinal, fine->d, fine->ordinal);
        return false;
    }
    return true;
}

// Both indexes locked.  B walks in chunks of kStage: the coarse search for n_cand (its
// tombstones and the filters limit the candidates), the fine index's scores of those ids (an
// id the fine index does not hold, or has deleted, becomes the fill), the k best of them.
// The candidates lie in the coarse index's buffers.
int32_t search_rescored_device_locked(bertx_index &coarse, bertx_index &fine, const float *d_q, int32_t B, int32_t k,
                                      int32_t n_cand, float *d_scores, int32_t *d_ids, hipStream_t s,
                                      const Filters &f = Filters())
{
    if (!d_q || !d_scores || !d_ids || B < 1 || k < 1 || k > n_cand || n_cand > kMaxK) return -1;
    Ordered oc(coarse.ord, s), of(fine.ord, s);
    for (int32_t b0 = 0; b0 < B; b0 += kStage) {
        const int32_t m = std::min(kStage, B - b0);
        const float *q = d_q + (size_t)b0 * coarse.d;
        int rc = search_launch(coarse, q, m, n_cand, coarse.cand_s, coarse.cand_i, s, f.from(b0));
        if (rc == 0) rc = score_ids_launch(fine, q, m, coarse.cand_i, n_cand, coarse.cand_exact, coarse.cand_kept, s);
        if (rc == 0)
            rc = launch_maxsim_rerank_select(coarse.cand_exact, coarse.cand_kept, m, n_cand, k, d_scores + (size_t)b0 * k,
                                             d_ids + (size_t)b0 * k, s);
        if (rc != 0) return rc;
    }
    return 0;
}

// ---- lists and the probed search (bert_hip.h "Lists and probed search") ----
constexpr int kMaxLists = 65536, kMaxProbe = 128, kProbePass = 64;

bool lists_kind_ok(const bertx_index &ix, const char *who)
{
    if (ix.storage != BERTX_INDEX_BIN) return true;
    errorf("%s: a binary index keeps no lists\n", who);
    return false;
}

// hipMalloc into an owned buffer; false (and no HIP error left behind) when it fails
bool dev_alloc(DevBuf &b, size_t bytes)
{
    if (hipMalloc(&b.p, bytes ? bytes : 4) == hipSuccess) return true;
    (void)hipGetLastError();
    b.p = nullptr;
    return false;
}

// new takes old's place; old's memory is freed when `fresh` goes out of scope
template <class T> void install(T *&field, DevBuf &fresh)
{
    void *old = (void *)field;
    field = (T *)fresh.p;
    fresh.p = old;
}

// Every operation in flight on the index has finished (before buffers it may read are freed).
int32_t lists_quiesce(bertx_index &ix)
{
    HIP_RC(ix.ord.wait());
    HIP_RC(hipStreamSynchronize(ix.stream));
    return 0;
}

struct ImageBufs {
    DevBuf image, scales, ids;
    int64_t groups = 0;
    bool alloc(const bertx_index &ix, int64_t n_rows, int C)
    {
        groups = lists_max_groups(n_rows, C);
        const size_t slots = (size_t)groups * 16;
        return dev_alloc(image, slots * (size_t)ix.d * (ix.storage == BERTX_INDEX_I8 ? 1 : 2)) && dev_alloc(ids, slots * 4) &&
               (ix.storage != BERTX_INDEX_I8 || dev_alloc(scales, slots * 4));
    }
    void install_in(bertx_index &ix)
    {
        install(ix.limage, image);
        install(ix.lscales, scales);
        install(ix.slot_id, ids);
        ix.list_cap_groups = groups;
    }
};

// Covers rows [listed, n) (idx locked, its device current, lists set): their lists by the
// centroid search, kStage rows at a time through the row staging buffer, then the layout of
// the whole image; nothing to do when every row is covered, unless the lists are new.  -2 with
// nothing changed when a larger image cannot be allocated.
int32_t build_lists_locked(bertx_index &ix, bool fresh_lists = false)
{
    if (!fresh_lists && ix.listed == ix.n && ix.limage) return 0;
    if (!ix.limage || lists_max_groups(ix.n, ix.n_lists) > ix.list_cap_groups) {
        ImageBufs fresh;
        if (!fresh.alloc(ix, ix.n, ix.n_lists)) {
            errorf("bertx_index_build_lists: device %d could not allocate the image of %lld rows in %d lists\n", ix.ordinal,
                   (long long)ix.n, ix.n_lists);
            return -2;
        }
        const int32_t rc = lists_quiesce(ix);
        if (rc != 0) return rc;
        fresh.install_in(ix);   // (the covered rows keep their lists; the whole image is laid out below)
    }
    uint32_t total = 0;
    {
        Ordered o(ix.ord, ix.stream);
        for (int64_t r0 = ix.listed; r0 < ix.n; r0 += kStage) {
            const int m = (int)std::min<int64_t>(kStage, ix.n - r0);
            int rc = launch_index_widen(ix.rows, ix.scales, ix.storage, r0, m, ix.d, ix.st_rows, ix.stream);
            if (rc == 0)
                rc = launch_search(ix.cent, nullptr, SEARCH_F16, ix.n_lists, ix.d, ix.st_rows, m, 1, ix.cent_scratch, ix.st_scores,
                                   ix.row_list + r0, ix.stream);
            if (rc != 0) return rc;
        }
        const int rc = launch_lists_layout(ix.rows, ix.scales, ix.storage, ix.n, ix.d, ix.row_list, ix.n_lists, ix.lcount, ix.goff,
                                           ix.limage, ix.lscales, ix.slot_id, ix.list_cap_groups, ix.stream);
        if (rc != 0) return rc;
        HIP_RC(hipMemcpyAsync(&total, ix.goff + ix.n_lists, 4, hipMemcpyDeviceToHost, ix.stream));
    }
    HIP_RC(hipStreamSynchronize(ix.stream));
    ix.list_groups = total;
    ix.listed = ix.n;
    return 0;
}

int32_t set_lists_locked(bertx_index &ix, const float *cent, int32_t C)
{
    if (!lists_kind_ok(ix, "bertx_index_set_lists")) return -1;
    if (!cent || C < 1 || C > kMaxLists) {
        errorf("bertx_index_set_lists: C = %d is not in 1 .. %d\n", C, kMaxLists);
        return -1;
    }
    // everything the new lists need, before anything of the old ones is touched
    DevBuf ncent, nscratch, ngoff, ncount, npartial, nrow, nids, nitem, nscores, nsorted;
    ImageBufs img;
    const bool need_img = !ix.limage || lists_max_groups(ix.n, C) > ix.list_cap_groups;
    const bool ok = dev_alloc(ncent, (size_t)((C + 15) / 16) * 16 * ix.d * 2) &&
                    dev_alloc(nscratch, (size_t)64 * (size_t)search_max_workgroups(C) * kMaxK * 8) &&
                    dev_alloc(ngoff, (size_t)(C + 1) * 4) && dev_alloc(ncount, (size_t)C * 4) &&
                    dev_alloc(npartial, probed_partial_bytes(C)) && (ix.row_list || dev_alloc(nrow, (size_t)ix.cap * 4)) &&
                    (ix.probe_ids || (dev_alloc(nids, (size_t)kProbePass * kMaxProbe * 4) &&
                                      dev_alloc(nitem, (size_t)kProbePass * kMaxProbe * 4) &&
                                      dev_alloc(nscores, (size_t)kProbePass * kMaxProbe * 4) &&
                                      dev_alloc(nsorted, (size_t)kProbePass * kMaxProbe * 4))) &&
                    (!need_img || img.alloc(ix, ix.n, C));
    if (!ok) {
        errorf("bertx_index_set_lists: device %d could not allocate %d lists over %lld rows\n", ix.ordinal, C, (long long)ix.n);
        return -2;
    }
    for (int32_t c0 = 0; c0 < C; c0 += kStage) {
        const int32_t m = std::min(kStage, C - c0);
        HIP_RC(hipMemcpyAsync(ix.st_rows, cent + (size_t)c0 * ix.d, (size_t)m * ix.d * 4, hipMemcpyHostToDevice, ix.stream));
        const int rc = launch_index_add(ix.st_rows, m, ix.d, c0, SEARCH_F16, ncent.p, nullptr, ix.stream);
        if (rc != 0) return rc;
        HIP_RC(hipStreamSynchronize(ix.stream));   // the staging buffer is reused
    }
    const int32_t rc = lists_quiesce(ix);
    if (rc != 0) return rc;
    install(ix.cent, ncent);
    install(ix.cent_scratch, nscratch);
    install(ix.goff, ngoff);
    install(ix.lcount, ncount);
    install(ix.probe_partial, npartial);
    if (!ix.row_list) install(ix.row_list, nrow);
    if (!ix.probe_ids) {
        install(ix.probe_ids, nids);
        install(ix.item_n, nitem);
        install(ix.probe_scores, nscores);
        install(ix.pair_sorted, nsorted);
    }
    if (need_img) img.install_in(ix);
    ix.n_lists = C;
    ix.listed = 0;
    ix.list_groups = 0;
    return build_lists_locked(ix, true);   // (an empty index too: the offsets must be written)
}

// The probed search on s (idx locked, its device current): passes of 64 queries, each the
// centroid search for the probes and launch_search_probed over the clustered image.
int32_t search_probed_device_locked(bertx_index &ix, const float *d_q, int32_t B, int32_t k, int32_t n_probe, float *d_scores,
                                    int32_t *d_ids, hipStream_t s, const Filters &f)
{
    if (!d_q || !d_scores || !d_ids || B < 1 || k < 1 || k > kMaxK) return -1;
    if (ix.n_lists == 0) {
        errorf("bertx_index_search_probed: the index has no lists (bertx_index_set_lists / _train_lists)\n");
        return -1;
    }
    if (n_probe < 1 || n_probe > std::min(ix.n_lists, kMaxProbe)) {
        errorf("bertx_index_search_probed: n_probe = %d is not in 1 .. %d\n", n_probe, std::min(ix.n_lists, kMaxProbe));
        return -1;
    }
    if (ix.listed != ix.n) {
        errorf("bertx_index_search_probed: the lists cover %lld of %lld rows (bertx_index_build_lists)\n", (long long)ix.listed,
               (long long)ix.n);
        return -1;
    }
    Ordered o(ix.ord, s);
    for (int32_t b0 = 0; b0 < B; b0 += kProbePass) {
        const int32_t nq = std::min(kProbePass, B - b0);
        const float *q = d_q + (size_t)b0 * ix.d;
        int rc = launch_search(ix.cent, nullptr, SEARCH_F16, ix.n_lists, ix.d, q, nq, n_probe, ix.cent_scratch, ix.probe_scores,
                               ix.probe_ids, s);
        if (rc != 0) return rc;
        const Filters fp = f.from(b0);
        const SearchMask mask{ix.tomb, fp.d, fp.stride};
        rc = launch_search_probed(ix.limage, ix.lscales, ix.slot_id, ix.goff, ix.storage, ix.n_lists, ix.d, q, nq, k, n_probe,
                                  ix.probe_ids, ix.pair_sorted, ix.item_n, ix.probe_partial, d_scores + (size_t)b0 * k,
                                  d_ids + (size_t)b0 * k, s, ix.removed || f.d ? &mask : nullptr);
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace

int index_ordinal(const bertx_index *ix) { return ix->ordinal; }

bertx_index *index_create_on(int ordinal, int d, int64_t capacity, int storage)
{
    if (!kind_known(storage)) {
        refuse_kind(storage);
        return nullptr;
    }
    if (capacity < 1 || capacity > 0x7ffffff0ll) {
        errorf("bertx_index_create: capacity %lld is not in 1 .. 2^31 - 16\n", (long long)capacity);
        return nullptr;
    }
    if (d % 64 || d < 64 || d > 1024) {
        errorf("bertx_index_create: width %d is not a multiple of 64 in 64 .. 1024\n", d);
        return nullptr;
    }
    DeviceGuard g(ordinal);
    if (!g.ok()) {
        errorf("bertx_index_create: cannot select device %d\n", ordinal);
        return nullptr;
    }
    bertx_index *ix = new (std::nothrow) bertx_index();
    if (!ix) return nullptr;
    ix->ordinal = ordinal;
    ix->d = d;
    ix->cap = capacity;
    ix->storage = storage;
    const size_t padded = (size_t)((capacity + 15) / 16) * 16;
    const bool bin = storage == BERTX_INDEX_BIN;
    const size_t row_bytes = bin ? search_bin_image_bytes(capacity, d) : padded * (size_t)d * (storage == BERTX_INDEX_I8 ? 1 : 2);
    const size_t scratch_bytes =
        (size_t)64 * (size_t)(bin ? search_bin_max_workgroups(capacity) : search_max_workgroups(capacity)) * kMaxK * 8;
    const size_t cand_bytes = (size_t)kStage * kMaxK * 4;
    ix->tomb_words = index_mask_words(capacity);
    const bool ok = (bin ? search_bin_prepare_device() : search_prepare_device()) == 0 && hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&ix->ord.done, hipEventDisableTiming) == hipSuccess &&
                    hipMalloc(&ix->rows, row_bytes) == hipSuccess && hipMalloc(&ix->scratch, scratch_bytes) == hipSuccess &&
                    (storage != BERTX_INDEX_I8 || hipMalloc((void **)&ix->scales, padded * 4) == hipSuccess) &&
                    hipMalloc((void **)&ix->st_rows, (size_t)kStage * d * 4) == hipSuccess &&
                    hipMalloc((void **)&ix->st_scores, (size_t)kStage * kMaxK * 4) == hipSuccess &&
                    hipMalloc((void **)&ix->st_ids, (size_t)kStage * kMaxK * 4) == hipSuccess &&
                    hipMalloc((void **)&ix->cand_s, cand_bytes) == hipSuccess &&
                    hipMalloc((void **)&ix->cand_exact, cand_bytes) == hipSuccess &&
                    hipMalloc((void **)&ix->cand_i, cand_bytes) == hipSuccess &&
                    hipMalloc((void **)&ix->cand_kept, cand_bytes) == hipSuccess &&
                    hipMalloc((void **)&ix->tomb, (size_t)ix->tomb_words * 4) == hipSuccess &&
                    hipMemsetAsync(ix->tomb, 0, (size_t)ix->tomb_words * 4, ix->stream) == hipSuccess &&
                    hipStreamSynchronize(ix->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        errorf("bertx_index_create: device %d could not allocate %zu bytes of rows (+ %zu of scratch)\n", ordinal,
               row_bytes, scratch_bytes);
        delete ix;
        return nullptr;
    }
    return ix;
}

}  // namespace emb

using emb::DeviceGuard;

extern "C" {

struct bertx_index *bertx_index_create(struct bert_ctx *ctx, int32_t slot, int32_t capacity_rows)
{
    return bertx_index_create_ex(ctx, slot, capacity_rows, BERTX_INDEX_F16);
}

struct bertx_index *bertx_index_create_ex(struct bert_ctx *ctx, int32_t slot, int32_t capacity_rows, int32_t storage)
{
    if (!ctx) {
        emb::errorf("bertx_index_create: no context\n");
        return nullptr;
    }
    if (!emb::kind_known(storage)) {
        emb::refuse_kind(storage);
        return nullptr;
    }
    if (bertx_num_devices(ctx) == 0) {
        emb::errorf("bertx_index_create: tokenizer-only context (BERT_HOST_ONLY): no device to hold an index\n");
        return nullptr;
    }
    const int ordinal = bertx_device_ordinal(ctx, slot);
    if (ordinal < 0) {
        emb::errorf("bertx_index_create: slot %d is not one of the context's %d device(s)\n", slot, bertx_num_devices(ctx));
        return nullptr;
    }
    return emb::index_create_on(ordinal, bert_n_embd(ctx), capacity_rows, storage);
}

void bertx_index_free(struct bertx_index *idx) { delete idx; }

int32_t bertx_index_clear(struct bertx_index *idx)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    // (no wait for the device, unlike the token store's clear: the index keeps no host image
    // that a copy in flight could still read, and the next add is ordered behind every search)
    if (idx->removed) {
        // the tombstones back to zero, ordered behind every operation so far
        DeviceGuard g(idx->ordinal);
        HIP_RC(g.status());
        emb::Ordered o(idx->ord, idx->stream);
        HIP_RC(hipMemsetAsync(idx->tomb, 0, (size_t)idx->tomb_words * 4, idx->stream));
        idx->removed = false;
    }
    idx->n = 0;
    // the lists go with the rows (their buffers stay until the next set_lists or the index's end)
    idx->n_lists = 0;
    idx->listed = 0;
    idx->list_groups = 0;
    return 0;
}

int32_t bertx_index_size(struct bertx_index *idx)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    return (int32_t)idx->n;
}

int32_t bertx_index_capacity(struct bertx_index *idx) { return idx ? (int32_t)idx->cap : -1; }
int32_t bertx_index_dim(struct bertx_index *idx) { return idx ? idx->d : -1; }
int32_t bertx_index_storage(struct bertx_index *idx) { return idx ? idx->storage : -1; }

int32_t bertx_index_add_device(struct bertx_index *idx, const float *d_rows, int32_t n, void *stream)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    return emb::add_device_locked(*idx, d_rows, n, stream ? (hipStream_t)stream : idx->stream);
}

int32_t bertx_index_add(struct bertx_index *idx, const float *rows, int32_t n)
{
    if (!idx || !rows || n < 1) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (idx->n + n > idx->cap) {
        emb::errorf("bertx_index_add: %d rows do not fit (%lld of %lld used)\n", n, (long long)idx->n, (long long)idx->cap);
        return -2;
    }
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    const int64_t n0 = idx->n;
    for (int32_t i = 0; i < n; i += emb::kStage) {
        const int32_t m = std::min(emb::kStage, n - i);
        hipError_t e = hipMemcpyAsync(idx->st_rows, rows + (size_t)i * idx->d, (size_t)m * idx->d * 4,
                                      hipMemcpyHostToDevice, idx->stream);
        int32_t rc = e == hipSuccess ? emb::add_device_locked(*idx, idx->st_rows, m, idx->stream) : -1;
        if (rc >= 0 && hipStreamSynchronize(idx->stream) != hipSuccess) rc = -1;   // the staging buffer is reused
        if (rc < 0) {
            (void)hipGetLastError();
            emb::errorf("bertx_index_add: device %d failed while adding (%d)\n", idx->ordinal, rc);
            idx->n = n0;
            return rc;
        }
    }
    return (int32_t)n0;
}

// The int8 image of rows first .. first + n - 1 (idx locked, the range checked) out of
// i8 fragment order: q int8 [n][d], scale f32 [n].
static int32_t read_rows_i8(struct bertx_index *idx, int32_t first, int32_t n, std::vector<int8_t> &q,
                            std::vector<float> &scale)
{
    const int d = idx->d;
    const int64_t g0 = first / 16, g1 = ((int64_t)first + n + 15) / 16;
    const size_t group_bytes = (size_t)16 * d;
    std::vector<int8_t> raw((size_t)(g1 - g0) * group_bytes);
    q.resize((size_t)n * d);
    scale.resize((size_t)n);
    HIP_RC(idx->ord.wait());
    HIP_RC(hipMemcpy(raw.data(), (const int8_t *)idx->rows + (size_t)g0 * group_bytes, raw.size(), hipMemcpyDeviceToHost));
    HIP_RC(hipMemcpy(scale.data(), idx->scales + first, (size_t)n * 4, hipMemcpyDeviceToHost));
    emb::unpack_i8_rows(raw.data(), 16 * g0, first, n, d, q.data());
    return 0;
}

// The bits of rows first .. first + n - 1 of a binary index (idx locked, the range checked)
// out of bit order: bits uint8 [n][d / 8] in np.packbits order.
static int32_t read_rows_bits(struct bertx_index *idx, int32_t first, int32_t n, std::vector<uint8_t> &bits)
{
    const int d = idx->d;
    const int64_t g0 = first / 64, g1 = ((int64_t)first + n + 63) / 64;
    const size_t group_words = (size_t)((d + 127) / 128) * 256;
    std::vector<uint32_t> raw((size_t)(g1 - g0) * group_words);
    bits.resize((size_t)n * (d / 8));
    HIP_RC(idx->ord.wait());
    HIP_RC(hipMemcpy(raw.data(), (const uint32_t *)idx->rows + (size_t)g0 * group_words, raw.size() * 4,
                     hipMemcpyDeviceToHost));
    emb::unpack_bin_rows(raw.data(), 64 * g0, first, n, d, bits.data());
    return 0;
}

int32_t bertx_index_rows(struct bertx_index *idx, int32_t first, int32_t n, float *out)
{
    if (!idx || !out || first < 0 || n < 1) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if ((int64_t)first + n > idx->n) return -1;
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    try {
        if (idx->storage == BERTX_INDEX_BIN) {
            std::vector<uint8_t> bits;
            const int32_t rc = read_rows_bits(idx, first, n, bits);
            if (rc != 0) return rc;
            const size_t total = (size_t)n * idx->d;
            for (size_t i = 0; i < total; ++i) out[i] = (bits[i >> 3] >> (7 - (i & 7))) & 1 ? 1.0f : -1.0f;
            return 0;
        }
        if (idx->storage == BERTX_INDEX_I8) {
            std::vector<int8_t> q;
            std::vector<float> scale;
            const int32_t rc = read_rows_i8(idx, first, n, q, scale);
            if (rc != 0) return rc;
            for (size_t r = 0; r < (size_t)n; ++r)
                for (int i = 0; i < idx->d; ++i) out[r * idx->d + i] = (float)q[r * idx->d + i] * scale[r];
            return 0;
        }
        const int d = idx->d;
        const int64_t g0 = first / 16, g1 = ((int64_t)first + n + 15) / 16;
        const size_t group_halfs = (size_t)16 * d;
        std::vector<uint16_t> raw((size_t)(g1 - g0) * group_halfs);
        HIP_RC(idx->ord.wait());
        HIP_RC(hipMemcpy(raw.data(), (const uint16_t *)idx->rows + (size_t)g0 * group_halfs, raw.size() * 2,
                         hipMemcpyDeviceToHost));
        emb::unpack_f16_rows(raw.data(), 16 * g0, first, n, d, out);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_rows: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_index_rows_i8(struct bertx_index *idx, int32_t first, int32_t n, int8_t *q, float *scale)
{
    if (!idx || !q || !scale || first < 0 || n < 1) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (idx->storage != BERTX_INDEX_I8 || (int64_t)first + n > idx->n) return -1;
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    try {
        // the caller's outputs are written only once both copies have succeeded
        std::vector<int8_t> hq;
        std::vector<float> hs;
        const int32_t rc = read_rows_i8(idx, first, n, hq, hs);
        if (rc != 0) return rc;
        std::memcpy(q, hq.data(), hq.size());
        std::memcpy(scale, hs.data(), hs.size() * 4);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_rows_i8: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_index_rows_bits(struct bertx_index *idx, int32_t first, int32_t n, uint8_t *out)
{
    if (!idx || !out || first < 0 || n < 1) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (idx->storage != BERTX_INDEX_BIN || (int64_t)first + n > idx->n) return -1;
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    try {
        // the caller's output is written only once the copy has succeeded
        std::vector<uint8_t> bits;
        const int32_t rc = read_rows_bits(idx, first, n, bits);
        if (rc != 0) return rc;
        std::memcpy(out, bits.data(), bits.size());
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_rows_bits: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_index_score_ids_device(struct bertx_index *idx, const float *d_queries, int32_t B, const int32_t *d_ids,
                                     int32_t n, float *d_scores, void *stream)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    return emb::score_ids_device_locked(*idx, d_queries, B, d_ids, n, d_scores, stream ? (hipStream_t)stream : idx->stream);
}

int32_t bertx_index_score_ids(struct bertx_index *idx, const float *queries, int32_t B, const int32_t *ids, int32_t n,
                              float *scores)
{
    if (!idx || !queries || !ids || !scores || B < 1 || n < 1 || n > emb::kMaxK) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    try {
        // the caller's output is written only once every chunk has succeeded
        std::vector<float> hs((size_t)B * n);
        for (int32_t i = 0; i < B; i += emb::kStage) {
            const int32_t m = std::min(emb::kStage, B - i);
            HIP_RC(hipMemcpyAsync(idx->st_rows, queries + (size_t)i * idx->d, (size_t)m * idx->d * 4, hipMemcpyHostToDevice,
                                  idx->stream));
            HIP_RC(hipMemcpyAsync(idx->st_ids, ids + (size_t)i * n, (size_t)m * n * 4, hipMemcpyHostToDevice, idx->stream));
            const int32_t rc = emb::score_ids_device_locked(*idx, idx->st_rows, m, idx->st_ids, n, idx->st_scores, idx->stream);
            if (rc != 0) return rc;
            HIP_RC(hipMemcpyAsync(hs.data() + (size_t)i * n, idx->st_scores, (size_t)m * n * 4, hipMemcpyDeviceToHost,
                                  idx->stream));
            HIP_RC(hipStreamSynchronize(idx->stream));
        }
        std::memcpy(scores, hs.data(), hs.size() * 4);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_score_ids: out of host memory\n");
        return -1;
    }
    return 0;
}

// store_common.h stage_filters on the index's stream (idx locked, its device current)
static int32_t stage_filters(struct bertx_index *idx, const uint32_t *filters, int32_t n_filters, int32_t words,
                             emb::DevBuf &buf)
{
    HIP_RC(emb::stage_filters(idx->stream, filters, n_filters, words, buf));
    return 0;
}

int32_t bertx_index_search_rescored_filtered_device(struct bertx_index *coarse, struct bertx_index *fine,
                                                    const float *d_queries, int32_t B, int32_t k, int32_t n_cand,
                                                    const uint32_t *d_filters, int32_t n_filters, int32_t words,
                                                    float *d_scores, int32_t *d_ids, void *stream)
{
    if (!emb::rescored_pair_ok(coarse, fine, "bertx_index_search_rescored")) return -1;
    std::scoped_lock lk(coarse->mu, fine->mu);   // both, in an order that cannot deadlock against the reverse pair
    if (!emb::filters_ok(*coarse, d_filters, n_filters, words, B)) return -1;
    DeviceGuard g(coarse->ordinal);
    HIP_RC(g.status());
    return emb::search_rescored_device_locked(*coarse, *fine, d_queries, B, k, n_cand, d_scores, d_ids,
                                              stream ? (hipStream_t)stream : coarse->stream,
                                              emb::filters_of(d_filters, n_filters, words));
}

int32_t bertx_index_search_rescored_device(struct bertx_index *coarse, struct bertx_index *fine, const float *d_queries,
                                           int32_t B, int32_t k, int32_t n_cand, float *d_scores, int32_t *d_ids,
                                           void *stream)
{
    return bertx_index_search_rescored_filtered_device(coarse, fine, d_queries, B, k, n_cand, nullptr, 0, 0, d_scores, d_ids,
                                                       stream);
}

int32_t bertx_index_search_rescored_filtered(struct bertx_index *coarse, struct bertx_index *fine, const float *queries,
                                             int32_t B, int32_t k, int32_t n_cand, const uint32_t *filters,
                                             int32_t n_filters, int32_t words, float *scores, int32_t *ids)
{
    if (!queries || !scores || !ids || B < 1 || k < 1 || k > n_cand || n_cand > emb::kMaxK) return -1;
    if (!emb::rescored_pair_ok(coarse, fine, "bertx_index_search_rescored")) return -1;
    std::scoped_lock lk(coarse->mu, fine->mu);
    if (!emb::filters_ok(*coarse, filters, n_filters, words, B)) return -1;
    DeviceGuard g(coarse->ordinal);
    HIP_RC(g.status());
    emb::DevBuf fbuf;   // (freed after the last chunk's synchronise)
    try {
        const int32_t frc = stage_filters(coarse, filters, n_filters, words, fbuf);
        if (frc != 0) return frc;
        const emb::Filters f = emb::filters_of((const uint32_t *)fbuf.p, n_filters, words);
        // the caller's outputs are written only once every chunk has succeeded
        std::vector<float> hs((size_t)B * k);
        std::vector<int32_t> hi((size_t)B * k);
        hipStream_t s = coarse->stream;
        for (int32_t i = 0; i < B; i += emb::kStage) {
            const int32_t m = std::min(emb::kStage, B - i);
            HIP_RC(hipMemcpyAsync(coarse->st_rows, queries + (size_t)i * coarse->d, (size_t)m * coarse->d * 4,
                                  hipMemcpyHostToDevice, s));
            const int32_t rc = emb::search_rescored_device_locked(*coarse, *fine, coarse->st_rows, m, k, n_cand,
                                                                  coarse->st_scores, coarse->st_ids, s, f.from(i));
            if (rc != 0) return rc;
            HIP_RC(hipMemcpyAsync(hs.data() + (size_t)i * k, coarse->st_scores, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
            HIP_RC(hipMemcpyAsync(hi.data() + (size_t)i * k, coarse->st_ids, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
            HIP_RC(hipStreamSynchronize(s));
        }
        std::memcpy(scores, hs.data(), hs.size() * 4);
        std::memcpy(ids, hi.data(), hi.size() * 4);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_search_rescored: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_index_search_rescored(struct bertx_index *coarse, struct bertx_index *fine, const float *queries, int32_t B,
                                    int32_t k, int32_t n_cand, float *scores, int32_t *ids)
{
    return bertx_index_search_rescored_filtered(coarse, fine, queries, B, k, n_cand, nullptr, 0, 0, scores, ids);
}

int32_t bertx_index_search_filtered_device(struct bertx_index *idx, const float *d_queries, int32_t B, int32_t k,
                                           const uint32_t *d_filters, int32_t n_filters, int32_t words, float *d_scores,
                                           int32_t *d_ids, void *stream)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (!emb::filters_ok(*idx, d_filters, n_filters, words, B)) return -1;
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    return emb::search_device_locked(*idx, d_queries, B, k, d_scores, d_ids, stream ? (hipStream_t)stream : idx->stream,
                                     emb::filters_of(d_filters, n_filters, words));
}

int32_t bertx_index_search_device(struct bertx_index *idx, const float *d_queries, int32_t B, int32_t k,
                                  float *d_scores, int32_t *d_ids, void *stream)
{
    return bertx_index_search_filtered_device(idx, d_queries, B, k, nullptr, 0, 0, d_scores, d_ids, stream);
}

int32_t bertx_index_search_filtered(struct bertx_index *idx, const float *queries, int32_t B, int32_t k,
                                    const uint32_t *filters, int32_t n_filters, int32_t words, float *scores, int32_t *ids)
{
    if (!idx || !queries || !scores || !ids || B < 1 || k < 1 || k > emb::kMaxK) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (!emb::filters_ok(*idx, filters, n_filters, words, B)) return -1;
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    emb::DevBuf fbuf;   // (freed after the last chunk's synchronise)
    try {
        const int32_t frc = stage_filters(idx, filters, n_filters, words, fbuf);
        if (frc != 0) return frc;
        const emb::Filters f = emb::filters_of((const uint32_t *)fbuf.p, n_filters, words);
        // the caller's outputs are written only once every chunk has succeeded
        std::vector<float> hs((size_t)B * k);
        std::vector<int32_t> hi((size_t)B * k);
        for (int32_t i = 0; i < B; i += emb::kStage) {
            const int32_t m = std::min(emb::kStage, B - i);
            HIP_RC(hipMemcpyAsync(idx->st_rows, queries + (size_t)i * idx->d, (size_t)m * idx->d * 4, hipMemcpyHostToDevice,
                                  idx->stream));
            const int32_t rc = emb::search_device_locked(*idx, idx->st_rows, m, k, idx->st_scores, idx->st_ids, idx->stream,
                                                         f.from(i));
            if (rc != 0) return rc;
            HIP_RC(hipMemcpyAsync(hs.data() + (size_t)i * k, idx->st_scores, (size_t)m * k * 4, hipMemcpyDeviceToHost,
                                  idx->stream));
            HIP_RC(hipMemcpyAsync(hi.data() + (size_t)i * k, idx->st_ids, (size_t)m * k * 4, hipMemcpyDeviceToHost,
                                  idx->stream));
            HIP_RC(hipStreamSynchronize(idx->stream));
        }
        std::memcpy(scores, hs.data(), hs.size() * 4);
        std::memcpy(ids, hi.data(), hi.size() * 4);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_search: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_index_search(struct bertx_index *idx, const float *queries, int32_t B, int32_t k, float *scores,
                           int32_t *ids)
{
    return bertx_index_search_filtered(idx, queries, B, k, nullptr, 0, 0, scores, ids);
}

int32_t bertx_index_remove_device(struct bertx_index *idx, const int32_t *d_ids, int32_t n, void *stream)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    return emb::remove_device_locked(*idx, d_ids, n, stream ? (hipStream_t)stream : idx->stream);
}

int32_t bertx_index_remove(struct bertx_index *idx, const int32_t *ids, int32_t n)
{
    if (!idx || !ids || n < 1) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    for (int32_t i = 0; i < n; i += emb::kStageIds) {
        const int32_t m = std::min(emb::kStageIds, n - i);
        HIP_RC(hipMemcpyAsync(idx->st_ids, ids + i, (size_t)m * 4, hipMemcpyHostToDevice, idx->stream));
        const int32_t rc = emb::remove_device_locked(*idx, idx->st_ids, m, idx->stream);
        if (rc != 0) return rc;
        HIP_RC(hipStreamSynchronize(idx->stream));   // the staging buffer is reused
    }
    return 0;
}

int32_t bertx_index_live(struct bertx_index *idx)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    int32_t dead = 0;
    {
        emb::Ordered o(idx->ord, idx->stream);
        const int rc = emb::launch_index_count_deleted(idx->tomb, idx->n, idx->st_ids, idx->stream);
        if (rc != 0) return rc;
        HIP_RC(hipMemcpyAsync(&dead, idx->st_ids, 4, hipMemcpyDeviceToHost, idx->stream));
    }
    HIP_RC(hipStreamSynchronize(idx->stream));
    return (int32_t)idx->n - dead;
}

int32_t bertx_index_deleted(struct bertx_index *idx, int32_t first, int32_t n, uint8_t *out)
{
    if (!idx || !out || first < 0 || n < 1) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if ((int64_t)first + n > idx->n) return -1;
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    try {
        // the caller's output is written only once every chunk has succeeded
        std::vector<uint8_t> flags((size_t)n);
        constexpr int32_t kChunk = emb::kStageIds * 4;   // bytes of the id staging buffer, one flag each
        for (int32_t i = 0; i < n; i += kChunk) {
            const int32_t m = std::min(kChunk, n - i);
            {
                emb::Ordered o(idx->ord, idx->stream);
                const int rc = emb::launch_index_deleted_flags(idx->tomb, (int64_t)first + i, m, (uint8_t *)idx->st_ids,
                                                               idx->stream);
                if (rc != 0) return rc;
                HIP_RC(hipMemcpyAsync(flags.data() + i, idx->st_ids, (size_t)m, hipMemcpyDeviceToHost, idx->stream));
            }
            HIP_RC(hipStreamSynchronize(idx->stream));
        }
        std::memcpy(out, flags.data(), flags.size());
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_deleted: out of host memory\n");
        return -1;
    }
    return 0;
}

// ---- lists and the probed search ----

int32_t bertx_index_set_lists(struct bertx_index *idx, const float *cent, int32_t C)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    return emb::set_lists_locked(*idx, cent, C);
}

int32_t bertx_index_build_lists(struct bertx_index *idx)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (!emb::lists_kind_ok(*idx, "bertx_index_build_lists")) return -1;
    if (idx->n_lists == 0) {
        emb::errorf("bertx_index_build_lists: the index has no lists\n");
        return -1;
    }
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    return emb::build_lists_locked(*idx);
}

int32_t bertx_index_lists(struct bertx_index *idx)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    return idx->n_lists;
}

int32_t bertx_index_listed_rows(struct bertx_index *idx)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    return idx->n_lists ? (int32_t)idx->listed : 0;
}

int64_t bertx_index_lists_bytes(struct bertx_index *idx)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (idx->n_lists == 0) return 0;
    const int64_t slot_bytes = (int64_t)idx->d * (idx->storage == BERTX_INDEX_I8 ? 1 : 2) + 4 + (idx->storage == BERTX_INDEX_I8 ? 4 : 0);
    return idx->list_groups * 16 * slot_bytes;
}

int32_t bertx_index_list_centroid(struct bertx_index *idx, int32_t c, float *out)
{
    if (!idx || !out) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (c < 0 || c >= idx->n_lists) return -1;
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    try {
        const size_t group_halfs = (size_t)16 * idx->d;
        std::vector<uint16_t> raw(group_halfs);
        HIP_RC(idx->ord.wait());
        HIP_RC(hipMemcpy(raw.data(), (const uint16_t *)idx->cent + (size_t)(c / 16) * group_halfs, group_halfs * 2,
                         hipMemcpyDeviceToHost));
        emb::unpack_f16_rows(raw.data(), c / 16 * 16, c, 1, idx->d, out);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_list_centroid: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_index_row_lists(struct bertx_index *idx, int32_t first, int32_t n, int32_t *out)
{
    if (!idx || !out || first < 0 || n < 1) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (idx->n_lists == 0 || (int64_t)first + n > idx->listed) return -1;
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    try {
        // the caller's output is written only once the copy has succeeded
        std::vector<int32_t> h((size_t)n);
        HIP_RC(idx->ord.wait());
        HIP_RC(hipMemcpy(h.data(), idx->row_list + first, (size_t)n * 4, hipMemcpyDeviceToHost));
        std::memcpy(out, h.data(), h.size() * 4);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_row_lists: out of host memory\n");
        return -1;
    }
    return 0;
}

// The stored rows first, first + stride, ... (n of them) widened into out [n][d] (idx locked,
// its device current): bertx_index_rows' values, kStage consecutive rows at a time.
static int32_t sample_rows(struct bertx_index *idx, const emb::KmeansSample &sm, float *out)
{
    const int d = idx->d;
    std::vector<float> chunk((size_t)emb::kStage * d);
    int64_t have0 = -1;   // the first row the chunk holds
    for (int64_t i = 0; i < sm.n; ++i) {
        const int64_t r = sm.start + i * sm.stride;
        if (have0 < 0 || r >= have0 + emb::kStage) {
            have0 = r;
            const int m = (int)std::min<int64_t>(emb::kStage, idx->n - r);
            {
                emb::Ordered o(idx->ord, idx->stream);
                const int rc = emb::launch_index_widen(idx->rows, idx->scales, idx->storage, r, m, d, idx->st_rows, idx->stream);
                if (rc != 0) return rc;
                HIP_RC(hipMemcpyAsync(chunk.data(), idx->st_rows, (size_t)m * d * 4, hipMemcpyDeviceToHost, idx->stream));
            }
            HIP_RC(hipStreamSynchronize(idx->stream));
        }
        std::memcpy(out + (size_t)i * d, chunk.data() + (size_t)(r - have0) * d, (size_t)d * 4);
    }
    return 0;
}

int32_t bertx_index_train_lists(struct bertx_index *idx, int32_t C, int32_t iters, uint32_t seed)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (!emb::lists_kind_ok(*idx, "bertx_index_train_lists")) return -1;
    if (C < 1 || C > emb::kMaxLists || iters < 0 || idx->n < 1) {
        emb::errorf("bertx_index_train_lists: C = %d, iters = %d, %lld rows: nothing to train\n", C, iters, (long long)idx->n);
        return -1;
    }
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    try {
        const int d = idx->d;
        const emb::KmeansSample sm = emb::kmeans_sample(idx->n, seed);
        if (C > sm.n) {
            emb::errorf("bertx_index_train_lists: C = %d exceeds the sample of %lld rows\n", C, (long long)sm.n);
            return -1;
        }
        std::vector<float> sample((size_t)sm.n * d), cent((size_t)C * d);
        int32_t rc = sample_rows(idx, sm, sample.data());
        if (rc != 0) return rc;
        for (int64_t c = 0; c < C; ++c)
            std::memcpy(cent.data() + (size_t)c * d, sample.data() + (size_t)emb::kmeans_initial_row(c, sm.n, C) * d, (size_t)d * 4);
        std::vector<int32_t> all((size_t)idx->n);
        std::vector<uint16_t> codes((size_t)sm.n);
        for (int32_t it = 0; it < iters; ++it) {
            rc = emb::set_lists_locked(*idx, cent.data(), C);
            if (rc != 0) return rc;
            HIP_RC(idx->ord.wait());
            HIP_RC(hipMemcpy(all.data(), idx->row_list, all.size() * 4, hipMemcpyDeviceToHost));
            // (a row without a list, whose scores were not numbers, takes part in no centroid)
            for (int64_t j = 0; j < sm.n; ++j) codes[(size_t)j] = (uint16_t)std::min<uint32_t>((uint32_t)all[(size_t)(sm.start + j * sm.stride)], 0xffffu);
            (void)emb::kmeans_update(sample.data(), codes.data(), sm.n, d, C, cent.data());
        }
        return emb::set_lists_locked(*idx, cent.data(), C);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_train_lists: out of host memory\n");
        return -1;
    }
}

int32_t bertx_index_search_probed_device(struct bertx_index *idx, const float *d_queries, int32_t B, int32_t k,
                                         int32_t n_probe, const uint32_t *d_filters, int32_t n_filters, int32_t words,
                                         float *d_scores, int32_t *d_ids, void *stream)
{
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (!emb::lists_kind_ok(*idx, "bertx_index_search_probed")) return -1;
    if (!emb::filters_ok(*idx, d_filters, n_filters, words, B)) return -1;
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    return emb::search_probed_device_locked(*idx, d_queries, B, k, n_probe, d_scores, d_ids,
                                            stream ? (hipStream_t)stream : idx->stream,
                                            emb::filters_of(d_filters, n_filters, words));
}

int32_t bertx_index_search_probed(struct bertx_index *idx, const float *queries, int32_t B, int32_t k, int32_t n_probe,
                                  const uint32_t *filters, int32_t n_filters, int32_t words, float *scores, int32_t *ids)
{
    if (!idx || !queries || !scores || !ids || B < 1 || k < 1 || k > emb::kMaxK) return -1;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (!emb::lists_kind_ok(*idx, "bertx_index_search_probed")) return -1;
    if (!emb::filters_ok(*idx, filters, n_filters, words, B)) return -1;
    DeviceGuard g(idx->ordinal);
    HIP_RC(g.status());
    if (idx->n_lists && idx->listed != idx->n) {   // the host form covers the new rows first
        const int32_t rc = emb::build_lists_locked(*idx);
        if (rc != 0) return rc;
    }
    emb::DevBuf fbuf;   // (freed after the last chunk's synchronise)
    try {
        const int32_t frc = stage_filters(idx, filters, n_filters, words, fbuf);
        if (frc != 0) return frc;
        const emb::Filters f = emb::filters_of((const uint32_t *)fbuf.p, n_filters, words);
        // the caller's outputs are written only once every chunk has succeeded
        std::vector<float> hs((size_t)B * k);
        std::vector<int32_t> hi((size_t)B * k);
        for (int32_t i = 0; i < B; i += emb::kStage) {
            const int32_t m = std::min(emb::kStage, B - i);
            HIP_RC(hipMemcpyAsync(idx->st_rows, queries + (size_t)i * idx->d, (size_t)m * idx->d * 4, hipMemcpyHostToDevice,
                                  idx->stream));
            const int32_t rc = emb::search_probed_device_locked(*idx, idx->st_rows, m, k, n_probe, idx->st_scores, idx->st_ids,
                                                                idx->stream, f.from(i));
            if (rc != 0) return rc;
            HIP_RC(hipMemcpyAsync(hs.data() + (size_t)i * k, idx->st_scores, (size_t)m * k * 4, hipMemcpyDeviceToHost,
                                  idx->stream));
            HIP_RC(hipMemcpyAsync(hi.data() + (size_t)i * k, idx->st_ids, (size_t)m * k * 4, hipMemcpyDeviceToHost,
                                  idx->stream));
            HIP_RC(hipStreamSynchronize(idx->stream));
        }
        std::memcpy(scores, hs.data(), hs.size() * 4);
        std::memcpy(ids, hi.data(), hi.size() * 4);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_index_search_probed: out of host memory\n");
        return -1;
    }
    return 0;
}

// texts -> rows through bert_encode_batch as one batch (it refuses the whole call
// when any input is longer than n_max_tokens and then writes nothing: the NaN
// planted in every row's first element is still there)
static int32_t encode_texts(struct bertx_index *idx, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                            const char **texts, std::vector<float> &rows, const char *who)
{
    if (!idx || !ctx || !texts || n < 1) return -1;
    if (bertx_num_devices(ctx) == 0 || bert_n_embd(ctx) != idx->d) {
        emb::errorf("%s: the context cannot produce rows of width %d\n", who, idx->d);
        return -1;
    }
    rows.assign((size_t)n * idx->d, 0.f);
    std::vector<float *> ptr((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        ptr[(size_t)i] = rows.data() + (size_t)i * idx->d;
        *ptr[(size_t)i] = std::numeric_limits<float>::quiet_NaN();
    }
    bert_encode_batch(ctx, n_threads, n, n, texts, ptr.data());
    for (int32_t i = 0; i < n; ++i)
        if (std::isnan(*ptr[(size_t)i])) {
            emb::errorf("%s: the encoder refused the texts; nothing was added or searched\n", who);
            return -4;
        }
    return 0;
}

int32_t bertx_index_add_texts(struct bertx_index *idx, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                              const char **texts)
{
    try {
        if (idx && n >= 1 && bertx_index_size(idx) + (int64_t)n > bertx_index_capacity(idx)) {
            emb::errorf("bertx_index_add_texts: %d rows do not fit\n", n);
            return -2;
        }
        std::vector<float> rows;
        const int32_t rc = encode_texts(idx, ctx, n_threads, n, texts, rows, "bertx_index_add_texts");
        return rc != 0 ? rc : bertx_index_add(idx, rows.data(), n);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_index_add_texts: %s\n", ex.what());
        return -1;
    }
}

int32_t bertx_index_search_texts(struct bertx_index *idx, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                 const char **texts, int32_t k, float *scores, int32_t *ids)
{
    try {
        if (!scores || !ids || k < 1 || k > emb::kMaxK) return -1;
        std::vector<float> rows;
        const int32_t rc = encode_texts(idx, ctx, n_threads, n, texts, rows, "bertx_index_search_texts");
        return rc != 0 ? rc : bertx_index_search(idx, rows.data(), n, k, scores, ids);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_index_search_texts: %s\n", ex.what());
        return -1;
    }
}

int32_t bertx_index_search_probed_texts(struct bertx_index *idx, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                        const char **texts, int32_t k, int32_t n_probe, float *scores, int32_t *ids)
{
    try {
        if (!scores || !ids || k < 1 || k > emb::kMaxK) return -1;
        std::vector<float> rows;
        const int32_t rc = encode_texts(idx, ctx, n_threads, n, texts, rows, "bertx_index_search_probed_texts");
        return rc != 0 ? rc : bertx_index_search_probed(idx, rows.data(), n, k, n_probe, nullptr, 0, 0, scores, ids);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_index_search_probed_texts: %s\n", ex.what());
        return -1;
    }
}

int32_t bertx_index_search_rescored_texts(struct bertx_index *coarse, struct bertx_index *fine, struct bert_ctx *ctx,
                                          int32_t n_threads, int32_t n, const char **texts, int32_t k, int32_t n_cand,
                                          float *scores, int32_t *ids)
{
    try {
        if (!scores || !ids || k < 1 || k > n_cand || n_cand > emb::kMaxK) return -1;
        if (!emb::rescored_pair_ok(coarse, fine, "bertx_index_search_rescored_texts")) return -1;
        std::vector<float> rows;
        const int32_t rc = encode_texts(coarse, ctx, n_threads, n, texts, rows, "bertx_index_search_rescored_texts");
        return rc != 0 ? rc : bertx_index_search_rescored(coarse, fine, rows.data(), n, k, n_cand, scores, ids);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_index_search_rescored_texts: %s\n", ex.what());
        return -1;
    }
}

}  // extern "C"
