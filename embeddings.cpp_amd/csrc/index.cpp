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
    hipStream_t stream = nullptr;
    emb::StoreOrder ord;
    std::mutex mu;
    ~bertx_index()
    {
        emb::DeviceGuard g(ordinal);
        // (no wait for ord.done, unlike the token store: an operation in flight on a caller's
        // stream reads device memory only, and hipFree waits for the device itself)
        if (stream) (void)hipStreamSynchronize(stream);
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

}  // namespace

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
