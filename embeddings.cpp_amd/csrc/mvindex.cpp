// The token store of late interaction (bert_hip.h bertx_mvindex_*): an append-only set
// of documents, each a run of unit-length token rows in the search kernel's fragment
// order, f16 (kernels.h, maxsim.hip) or int8 with one f32 per token slot (maxsim_i8.hip),
// the fused MaxSim scorer over it, and the text forms on top of the per-token forward.
// A residual store (maxsim_res.hip) keeps no rows: per slot the centroid code, 2 or 4 bits
// per element and one f32; its adds go through a staging image in the f16 store layout.
// After creation a store knows only its device ordinal, its width and its storage kind.
// The ordering rules and the unpackers are shared with the embedding index
// (store_common.h).  A text form is an entry point's argument checks, one of two
// tokenizers that describe the call's texts as a TextRows, and one body per verb (add,
// score, search); the bodies do not know which tokenizer ran.
#include "bert.h"
#include "bert_hip.h"

#include "chunk_rule.h"
#include "engine.h"
#include "hip_check.h"
#include "kmeans_update.h"
#include "store_common.h"
#include "task_pool.h"

#include <algorithm>
#include <atomic>
#include <cmath>
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
    // test hook (bertx_test_mvindex_grid): a positive grid_cap bounds the workgroups of every scan
    // launched for this store; last_grid: the scan kernel's workgroups at the latest such launch
    int grid_cap = 0, last_grid = 0;
    // the tombstones (index_mask.hip): bit d % 32 of word d / 32 is 1 once document d was
    // removed; `removed`: some remove was accepted since creation or the last clear, so the
    // scans and the scorers take their masked instantiations.  last_masked (test hook
    // bertx_test_mvindex_last_masked): the latest scan or scorer launch was a masked one
    uint32_t *tomb = nullptr;
    int64_t tomb_words = 0;
    bool removed = false;
    int last_masked = 0;
    void *search_scratch = nullptr;        // the partial lists of the full-scan search (maxsim_search_scratch_bytes)
    // centroid codes (set_centroids; all null / 0 before): the C centroids packed as one
    // document of their own buffer, their f32 (int8), one code per token slot, the table of
    // a candidates pass (256 C bytes), and the candidate lists of kCandQueries queries
    int32_t C = 0, cap_C = 0;
    void *cent = nullptr;
    float *cent_u = nullptr;
    uint16_t *codes = nullptr;
    float *tscratch = nullptr;
    float *cand_approx = nullptr, *cand_exact = nullptr;
    int32_t *cand_ids = nullptr;
    int32_t *cent_entry = nullptr;         // device: (0, C) the centroids' table entry, then their source offset 0
    // residual kinds (store stays null): the slots' bits and u; the codec on the device (cutoffs
    // f32, weights f16, the scorer's pair table), the weights on the host; the staging image of an add
    // (f16 store layout) with its table, both grown by the add that needs more
    uint32_t *res_bits = nullptr;
    float *res_u = nullptr, *res_cuts = nullptr;
    uint16_t *res_wts = nullptr;
    uint32_t *res_pair = nullptr;
    bool has_buckets = false;
    uint16_t h_wts[16] = {};
    void *stage_img = nullptr;
    int32_t *stage_tab = nullptr;
    int64_t stage_slots = 0, stage_docs = 0;
    hipStream_t stream = nullptr;
    emb::StoreOrder ord;
    std::mutex mu;
    ~bertx_mvindex()
    {
        emb::DeviceGuard g(ordinal);
        if (stream) (void)hipStreamSynchronize(stream);
        // (unlike the embedding index: an add on a caller's stream copies from the page-locked
        // images freed below)
        if (ord.done) (void)ord.wait();
        for (void *p : {store, (void *)scales, (void *)table, (void *)src_off, (void *)st_rows, (void *)st_q, (void *)st_out,
                        (void *)st_ids, (void *)st_tok, search_scratch, cent, (void *)cent_u, (void *)codes,
                        (void *)tscratch, (void *)cand_approx, (void *)cand_exact, (void *)cand_ids, (void *)cent_entry,
                        (void *)res_bits, (void *)res_u, (void *)res_cuts, (void *)res_wts, (void *)res_pair, stage_img,
                        (void *)stage_tab, (void *)tomb})
            if (p) (void)hipFree(p);
        if (h_table) (void)hipHostFree(h_table);
        if (h_src) (void)hipHostFree(h_src);
        if (ord.done) (void)hipEventDestroy(ord.done);
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
constexpr int kCandQueries = 64;    // queries whose candidate lists the store's scratch holds at a time

std::atomic<int> g_approx_forms{0};   // bertx_test_approx_ran: 1 the table went to LDS, 2 global memory

// Bits per element of a residual store, 0 for the kinds that keep rows.
int res_nbits(const bertx_mvindex &mv)
{
    return mv.storage == BERTX_INDEX_RES2 ? 2 : mv.storage == BERTX_INDEX_RES4 ? 4 : 0;
}

// The kind whose table and assign kernels serve the store's centroids: a residual store's
// centroids are an f16 store's.
int cent_kind(const bertx_mvindex &mv) { return res_nbits(mv) ? (int)BERTX_INDEX_F16 : mv.storage; }

// A residual store encodes against its centroids and buckets: an add without either is refused.
bool add_refused(const bertx_mvindex &mv, const char *who)
{
    if (!res_nbits(mv) || (mv.C > 0 && mv.has_buckets)) return false;
    errorf("%s: a residual store needs centroids (bertx_mvindex_set_centroids) and buckets "
           "(bertx_mvindex_set_residual_buckets) before documents\n", who);
    return true;
}

bool full_scan_refused(const bertx_mvindex &mv, const char *who)
{
    if (!res_nbits(mv)) return false;
    errorf("%s: the full scan of a residual store is not provided (bertx_mvindex_search_pruned)\n", who);
    return true;
}

// The codes of the documents first_doc .. first_doc + n - 1, which take the groups from g0 on
// (a store without centroids keeps none).
int32_t assign_codes(bertx_mvindex &mv, int64_t g0, int64_t g1, int32_t d0, int32_t d1, hipStream_t s)
{
    if (mv.C == 0 || g1 <= g0) return 0;
    return launch_mv_assign(mv.store, mv.scales, mv.storage, mv.table, g0, g1, d0, d1, mv.w, mv.cent, mv.cent_u, mv.C,
                            mv.codes, s);
}

// After the rows of an add are packed, on the same stream: the new documents' codes.
int32_t assign_new(bertx_mvindex &mv, int32_t n, int64_t slots, hipStream_t s)
{
    if (const int nb = res_nbits(mv)) {
        // the staging image is an f16 store of the call's documents alone, whose codes, bits and
        // u are the real arrays from the call's first group on
        const size_t g0 = (size_t)(mv.used_slots / 16), per_group = (size_t)mv.w * nb / 2;   // dwords of bits per group
        uint16_t *codes = mv.codes + g0 * 16;
        const int32_t rc = launch_mv_assign(mv.stage_img, nullptr, BERTX_INDEX_F16, mv.stage_tab, 0, slots / 16, 0, n, mv.w,
                                            mv.cent, nullptr, mv.C, codes, s);
        if (rc != 0) return rc;
        return launch_res_encode(mv.stage_img, slots / 16, mv.w, nb, codes, mv.cent, mv.res_cuts, mv.res_wts,
                                 mv.res_bits + g0 * per_group, mv.res_u + g0 * 16, s);
    }
    return assign_codes(mv, mv.used_slots / 16, (mv.used_slots + slots) / 16, (int32_t)mv.n_docs, (int32_t)mv.n_docs + n, s);
}

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

// Before the first pack of an add, inside its stream order: the new documents' entries go to
// the device; a residual store also grows its staging image to the call's size (waiting for
// whatever still reads the old one) and writes the staging table.
int32_t begin_add(bertx_mvindex &mv, int32_t n, int64_t slots, hipStream_t s)
{
    if (const int32_t rc = upload_entries(mv, n, s)) return rc;
    if (!res_nbits(mv)) return 0;
    if (slots > mv.stage_slots || n > mv.stage_docs) {
        const int64_t ns = std::max(slots, mv.stage_slots), nd = std::max<int64_t>(n, mv.stage_docs);
        HIP_RC(mv.ord.wait());
        if (mv.stage_img) (void)hipFree(mv.stage_img);
        if (mv.stage_tab) (void)hipFree(mv.stage_tab);
        mv.stage_img = nullptr;
        mv.stage_tab = nullptr;
        mv.stage_slots = mv.stage_docs = 0;
        if (hipMalloc(&mv.stage_img, (size_t)ns * mv.w * 2) != hipSuccess ||
            hipMalloc((void **)&mv.stage_tab, (size_t)nd * 8) != hipSuccess) {
            (void)hipGetLastError();
            errorf("bertx_mvindex_add: device %d could not allocate the staging image of %lld token slots\n", mv.ordinal,
                   (long long)ns);
            return -3;
        }
        mv.stage_slots = ns;
        mv.stage_docs = nd;
    }
    return launch_res_rel_table(mv.table + 2 * mv.n_docs, n, mv.used_slots / 16, mv.stage_tab, s);
}

int32_t pack(bertx_mvindex &mv, const float *d_rows, int64_t t0, int64_t count, int32_t n, hipStream_t s)
{
    if (res_nbits(mv))
        return launch_mv_pack(d_rows, t0, count, mv.w, mv.src_off + mv.n_docs, mv.stage_tab, n, mv.stage_img, s);
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
    if (!d_rows || add_refused(mv, "bertx_mvindex_add_device")) return -1;
    int64_t T = 0, slots = 0;
    int32_t rc = plan_add(mv, lens, n, &T, &slots);
    if (rc != 0) return rc;
    {
        Ordered o(mv.ord, s);
        rc = begin_add(mv, n, slots, s);
        if (rc == 0) rc = pack(mv, d_rows, 0, T, n, s);
        if (rc == 0) rc = assign_new(mv, n, slots, s);
    }
    if (rc != 0) {
        (void)hipStreamSynchronize(s);   // the entries may be rewritten by the next add
        return rc;
    }
    return commit(mv, n, slots);
}

// The scorer of the store's kind; the caller orders the stream.  (On a residual store without
// documents every id is out of range, and neither codes nor centroids are read.)
// Once a document was removed the masked scorers run, with the store's tombstones: a deleted
// id scores as one outside [0, docs).
int32_t score_launch(bertx_mvindex &mv, const float *d_q, int32_t Lq, const int32_t *d_ids, int32_t n, float *d_out,
                     hipStream_t s)
{
    const uint32_t *tomb = mv.removed ? mv.tomb : nullptr;
    mv.last_masked = tomb != nullptr;
    if (mv.storage == BERTX_INDEX_I8)
        return launch_maxsim_i8(mv.store, mv.scales, mv.table, (int)mv.n_docs, mv.w, d_q, Lq, d_ids, n, d_out, s,
                                mv.grid_cap, &mv.last_grid, tomb);
    if (const int nb = res_nbits(mv))
        return launch_maxsim_res(mv.res_bits, mv.res_u, mv.codes, mv.cent, mv.res_pair, nb, mv.table, (int)mv.n_docs, mv.w,
                                 d_q, Lq, d_ids, n, d_out, s, mv.grid_cap, &mv.last_grid, tomb);
    return launch_maxsim(mv.store, mv.table, (int)mv.n_docs, mv.w, d_q, Lq, d_ids, n, d_out, s, mv.grid_cap,
                         &mv.last_grid, tomb);
}

// The mask of a scan (mv locked): none while nothing was removed and no filter is given, which
// launches the unmasked kernels with the arguments they always had; else the store's
// tombstones with the call's filters (not read on an empty store).
struct ScanMask {
    SearchMask m;
    bool on;
    ScanMask(bertx_mvindex &mv, const Filters &f)
        : m{mv.tomb, mv.n_docs > 0 ? f.d : nullptr, f.stride}, on(mv.removed || f.d)
    {
        mv.last_masked = on;
    }
    const SearchMask *get() const { return on ? &m : nullptr; }
};

int32_t score_device_locked(bertx_mvindex &mv, const float *d_q, int32_t Lq, const int32_t *d_ids, int32_t n,
                            float *d_out, hipStream_t s)
{
    if (!d_q || !d_out || Lq < 1 || Lq > kMaxLq || n < 1) return -1;
    Ordered o(mv.ord, s);
    return score_launch(mv, d_q, Lq, d_ids, n, d_out, s);
}

bool search_args_ok(const char *who, int32_t B, int32_t Lq, int32_t k)
{
    if (B >= 1 && Lq >= 1 && Lq <= kMaxLq && k >= 1 && k <= kMaxK) return true;
    errorf("%s: B = %d, Lq = %d, k = %d are not in B >= 1, 1 <= Lq <= %d, 1 <= k <= %d\n", who, B, Lq, k, kMaxLq, kMaxK);
    return false;
}

int32_t search_device_locked(bertx_mvindex &mv, const float *d_q, int32_t B, int32_t Lq, int32_t k, float *d_scores,
                             int32_t *d_ids, hipStream_t s, const Filters &f = Filters())
{
    if (!d_q || !d_scores || !d_ids || !search_args_ok("bertx_mvindex_search", B, Lq, k)) return -1;
    if (full_scan_refused(mv, "bertx_mvindex_search")) return -1;
    Ordered o(mv.ord, s);
    const ScanMask mask(mv, f);
    return launch_maxsim_search(mv.store, mv.scales, mv.storage, mv.table, (int)mv.n_docs, mv.used_slots / 16, mv.w, d_q, B,
                                Lq, k, mv.search_scratch, d_scores, d_ids, s, mv.grid_cap, &mv.last_grid, mask.get());
}

int32_t remove_device_locked(bertx_mvindex &mv, const int32_t *d_ids, int32_t n, hipStream_t s)
{
    if (!d_ids || n < 1) return -1;
    Ordered o(mv.ord, s);
    const int rc = launch_index_remove(d_ids, n, mv.n_docs, mv.tomb, s);
    if (rc == 0) mv.removed = true;
    return rc;
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
    const int64_t first = mv.h_table[2 * (size_t)id], len = mv.h_table[2 * (size_t)id + 1];
    const size_t group_bytes = (size_t)16 * mv.w, groups = (size_t)((len + 15) / 16);
    std::vector<int8_t> raw(groups * group_bytes);
    std::vector<float> us(groups * 16);
    HIP_RC(mv.ord.wait());
    HIP_RC(hipMemcpy(raw.data(), (const int8_t *)mv.store + (size_t)first * group_bytes, raw.size(),
                     hipMemcpyDeviceToHost));
    HIP_RC(hipMemcpy(us.data(), mv.scales + (size_t)first * 16, us.size() * 4, hipMemcpyDeviceToHost));
    unpack_i8_rows(raw.data(), 0, 0, len, mv.w, q);
    std::memcpy(u, us.data(), (size_t)len * 4);
    return 0;
}

// The stored state of document id of a residual store in the canonical order of
// bertx_mvindex_doc_residual: codes [len], bits [len][w NB / 8], u [len] (the caller holds
// the lock, has checked the id and has selected the device).
int32_t read_doc_res(bertx_mvindex &mv, int32_t id, uint16_t *codes, uint8_t *bits, float *u)
{
    const int nb = res_nbits(mv), w = mv.w, UG = w / 64, DW = nb / 2;
    const int64_t first = mv.h_table[2 * (size_t)id], len = mv.h_table[2 * (size_t)id + 1];
    const size_t groups = (size_t)((len + 15) / 16), group_dw = (size_t)UG * 64 * DW, row_bytes = (size_t)w * nb / 8;
    std::vector<uint32_t> raw(groups * group_dw);
    HIP_RC(mv.ord.wait());
    HIP_RC(hipMemcpy(raw.data(), mv.res_bits + (size_t)first * group_dw, raw.size() * 4, hipMemcpyDeviceToHost));
    HIP_RC(hipMemcpy(codes, mv.codes + (size_t)first * 16, (size_t)len * 2, hipMemcpyDeviceToHost));
    HIP_RC(hipMemcpy(u, mv.res_u + (size_t)first * 16, (size_t)len * 4, hipMemcpyDeviceToHost));
    // lane 16g + f of unit un holds row f's elements 8g .. 8g + 7 of blocks 2 un, 2 un + 1:
    // 2 (NB 2) or 4 (NB 4) canonical bytes per block, little-endian
    for (int64_t r = 0; r < len; ++r) {
        uint8_t *o = bits + (size_t)r * row_bytes;
        for (int kb = 0; kb < w / 32; ++kb)
            for (int g = 0; g < 4; ++g) {
                const uint32_t *at = raw.data() + (size_t)(r / 16) * group_dw + ((size_t)(kb / 2) * 64 + 16 * g + (r & 15)) * DW;
                const uint32_t v = nb == 2 ? (at[0] >> (16 * (kb & 1))) & 0xffffu : at[kb & 1];
                for (int b = 0; b < nb; ++b) o[((size_t)4 * kb + g) * nb + b] = (uint8_t)(v >> (8 * b));
            }
    }
    return 0;
}

// The f32 values of every centroid of a store whose centroids are f16 rows.
int32_t read_centroids_f16(bertx_mvindex &mv, std::vector<float> &out)
{
    std::vector<uint16_t> raw((size_t)mv.C * mv.w);
    out.resize(raw.size());
    HIP_RC(mv.ord.wait());
    HIP_RC(hipMemcpy(raw.data(), mv.cent, raw.size() * 2, hipMemcpyDeviceToHost));
    unpack_f16_rows(raw.data(), 0, 0, mv.C, mv.w, out.data());
    return 0;
}

// bertx_mvindex_doc under the caller's lock, the id checked and the device selected.
int32_t doc_locked(bertx_mvindex *mv, int32_t id, float *out)
{
    if (const int nb = emb::res_nbits(*mv)) {
        try {
            const int w = mv->w;
            const int64_t len = mv->h_table[2 * (size_t)id + 1];
            std::vector<uint16_t> codes((size_t)len);
            std::vector<uint8_t> bits((size_t)len * w * nb / 8);
            std::vector<float> u((size_t)len), c((size_t)w);
            if (const int32_t rc = read_doc_res(*mv, id, codes.data(), bits.data(), u.data())) return rc;
            std::vector<uint16_t> raw((size_t)16 * w);
            for (int64_t r = 0; r < len; ++r) {
                const size_t cg = codes[(size_t)r] / 16;
                HIP_RC(hipMemcpy(raw.data(), (const uint16_t *)mv->cent + cg * raw.size(), raw.size() * 2, hipMemcpyDeviceToHost));
                unpack_f16_rows(raw.data(), (int64_t)cg * 16, codes[(size_t)r], 1, w, c.data());
                const uint8_t *b = bits.data() + (size_t)r * w * nb / 8;
                for (int i = 0; i < w; ++i) {
                    const int k = (b[(size_t)i * nb / 8] >> (nb * (i % (8 / nb)))) & ((1 << nb) - 1);
                    // e = c + wt in f16: the f32 sum of two f16 values rounded once more gives the same bits
                    const float e = f16_to_f32(f32_to_f16(c[(size_t)i] + f16_to_f32(mv->h_wts[k])));
                    out[(size_t)r * w + i] = e * u[(size_t)r];
                }
            }
        } catch (const std::bad_alloc &) {
            emb::errorf("bertx_mvindex_doc: out of host memory\n");
            return -1;
        }
        return 0;
    }
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
        const int64_t first = mv->h_table[2 * (size_t)id], len = mv->h_table[2 * (size_t)id + 1];
        const size_t group_halfs = (size_t)16 * mv->w;
        std::vector<uint16_t> raw((size_t)((len + 15) / 16) * group_halfs);
        HIP_RC(mv->ord.wait());
        HIP_RC(hipMemcpy(raw.data(), (const uint16_t *)mv->store + (size_t)first * group_halfs, raw.size() * 2,
                         hipMemcpyDeviceToHost));
        emb::unpack_f16_rows(raw.data(), 0, 0, len, mv->w, out);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_doc: out of host memory\n");
        return -1;
    }
    return 0;
}

// The context's replica on the store's GPU, or -1 with a message.
int32_t slot_on(struct bert_ctx *ctx, int ordinal, const char *who)
{
    for (int32_t s = 0; s < bertx_num_devices(ctx); ++s)
        if (bertx_device_ordinal(ctx, s) == ordinal) return s;
    errorf("%s: the context has no replica on the store's device %d\n", who, ordinal);
    return -1;
}

int32_t text_ctx_ok(bertx_mvindex *mv, struct bert_ctx *ctx, const char *who, int32_t *slot)
{
    if (!mv || !ctx) return -1;
    if (bertx_num_devices(ctx) == 0 || bert_n_embd(ctx) != mv->w) {
        errorf("%s: the context cannot produce token rows of width %d\n", who, mv->w);
        return -1;
    }
    return (*slot = slot_on(ctx, mv->ordinal, who)) < 0 ? -1 : 0;
}

bool pruned_args_ok(const bertx_mvindex &mv, const char *who, int32_t B, int32_t Lq, int32_t k, int32_t n_cand)
{
    if (B < 1 || Lq < 1 || Lq > kMaxLq || k < 1 || k > n_cand || n_cand > kMaxK) {
        errorf("%s: B = %d, Lq = %d, k = %d, n_cand = %d are not in B >= 1, 1 <= Lq <= %d, 1 <= k <= n_cand <= %d\n", who, B,
               Lq, k, n_cand, kMaxLq, kMaxK);
        return false;
    }
    if (mv.C == 0) {
        errorf("%s: no centroids set (bertx_mvindex_set_centroids / _train_centroids)\n", who);
        return false;
    }
    return true;
}

// The candidate lists of B queries, floor(4 / ceil(Lq / 16)) per pass; the caller orders the
// stream.
int32_t candidates_launch(bertx_mvindex &mv, const float *d_q, int32_t B, int32_t Lq, int32_t n_cand, float *d_approx,
                          int32_t *d_ids, hipStream_t s, const Filters &f)
{
    const int32_t per_pass = 4 / ((Lq + 15) / 16);
    const ScanMask mask(mv, f);
    for (int32_t b0 = 0; b0 < B; b0 += per_pass) {
        int form = 0;
        const SearchMask pm = pass_mask(mask.m, b0);
        const int32_t rc = launch_maxsim_candidates(mv.codes, mv.table, (int)mv.n_docs, mv.used_slots / 16, cent_kind(mv), mv.w,
                                                    mv.cent, mv.cent_u, mv.C, d_q + (size_t)b0 * Lq * mv.w,
                                                    std::min(per_pass, B - b0), Lq, n_cand, mv.tscratch, mv.search_scratch,
                                                    d_approx + (size_t)b0 * n_cand, d_ids + (size_t)b0 * n_cand, 3, &form, s,
                                                    mv.grid_cap, &mv.last_grid, mask.on ? &pm : nullptr);
        if (rc != 0) return rc;
        g_approx_forms.fetch_or(form);
    }
    return 0;
}

int32_t candidates_device_locked(bertx_mvindex &mv, const float *d_q, int32_t B, int32_t Lq, int32_t n_cand,
                                 float *d_approx, int32_t *d_ids, hipStream_t s, const Filters &f = Filters())
{
    if (!d_q || !d_approx || !d_ids || !pruned_args_ok(mv, "bertx_mvindex_candidates", B, Lq, 1, n_cand)) return -1;
    Ordered o(mv.ord, s);
    return candidates_launch(mv, d_q, B, Lq, n_cand, d_approx, d_ids, s, f);
}

// kCandQueries queries at a time through the store's candidate scratch: their candidates
// (admissible documents only: the tombstones and the filters limit them), the scorer over each
// query's candidate ids (a fill id -1 scores -inf; the rerank takes the store's tombstones and
// no filter, which no candidate could fail), the k best.
int32_t search_pruned_device_locked(bertx_mvindex &mv, const float *d_q, int32_t B, int32_t Lq, int32_t k, int32_t n_cand,
                                    float *d_scores, int32_t *d_ids, hipStream_t s, const Filters &f = Filters())
{
    if (!d_q || !d_scores || !d_ids || !pruned_args_ok(mv, "bertx_mvindex_search_pruned", B, Lq, k, n_cand)) return -1;
    Ordered o(mv.ord, s);
    for (int32_t c0 = 0; c0 < B; c0 += kCandQueries) {
        const int32_t m = std::min(kCandQueries, B - c0);
        const float *Q = d_q + (size_t)c0 * Lq * mv.w;
        int32_t rc = candidates_launch(mv, Q, m, Lq, n_cand, mv.cand_approx, mv.cand_ids, s, f.from(c0));
        for (int32_t b = 0; b < m && rc == 0; ++b) {
            const float *qb = Q + (size_t)b * Lq * mv.w;
            const int32_t *ib = mv.cand_ids + (size_t)b * n_cand;
            float *ob = mv.cand_exact + (size_t)b * n_cand;
            rc = score_launch(mv, qb, Lq, ib, n_cand, ob, s);
        }
        if (rc == 0)
            rc = launch_maxsim_rerank_select(mv.cand_exact, mv.cand_ids, m, n_cand, k, d_scores + (size_t)c0 * k,
                                             d_ids + (size_t)c0 * k, s);
        if (rc != 0) return rc;
    }
    return 0;
}

// B queries f32 [B][Lq][w] already on the device, on the store's stream: their results
// into host vectors (the caller copies them out when the whole call succeeded).  n_cand > 0:
// by the pruned search.
int32_t search_to_host(bertx_mvindex &mv, const float *d_q, int32_t B, int32_t Lq, int32_t k, float *scores, int32_t *ids,
                       int32_t n_cand = 0)
{
    DevBuf d_s, d_i;
    HIP_RC(hipMalloc(&d_s.p, (size_t)B * k * 4));
    HIP_RC(hipMalloc(&d_i.p, (size_t)B * k * 4));
    const int32_t rc = n_cand > 0 ? search_pruned_device_locked(mv, d_q, B, Lq, k, n_cand, (float *)d_s.p, (int32_t *)d_i.p,
                                                                mv.stream)
                                  : search_device_locked(mv, d_q, B, Lq, k, (float *)d_s.p, (int32_t *)d_i.p, mv.stream);
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
    return (*slot = slot_on(ctx, mv->ordinal, who)) < 0 ? -1 : 0;
}

// How a call's texts became rows: filled by one of the two tokenizers before the store's
// lock is taken, read by the bodies below.
struct TextRows {
    std::vector<int32_t> ids;    // text i's ids at ids[i * stride]
    size_t stride = 0;
    std::vector<int32_t> lens;   // tokens per text
    std::vector<int32_t> keep;   // empty: every token's row is kept; else beside ids, 1: the token's row is kept
    std::vector<int32_t> kept;   // rows per text
    std::vector<int32_t> keys;   // empty: every token is an attention key; else the key count per text
    int32_t out_kind = BERTX_OUT_TOKENS;
    int32_t slot = -1;           // the context's replica on the store's GPU
};

// The plain form: every token's final hidden state (the callers check the lens against
// their own limits).
int32_t tokenize_plain(struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts, int32_t slot, TextRows &t)
{
    const int32_t n_max = bert_n_max_tokens(ctx);
    t.slot = slot;
    t.stride = (size_t)n_max;
    t.ids.resize((size_t)n * t.stride);
    t.lens.resize((size_t)n);
    if (bertx_tokenize_batch(ctx, n_threads, n, texts, n_max, t.ids.data(), t.lens.data()) != 0) return -1;
    t.kept = t.lens;
    return 0;
}

// The ColBERT form, kind 1 documents (punctuation rows dropped), kind 0 queries ([MASK]-
// augmented to maxlen, every row kept): the projected rows.  The context's mask_keys
// setting is read here, once per call: a query's [MASK] rows are keys (no counts), or its
// rows up to [SEP] only.
int32_t tokenize_colbert(struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts, int32_t kind,
                         int32_t maxlen, int32_t slot, TextRows &t)
{
    const size_t N = (size_t)maxlen;
    const bool doc = kind == 1;
    t.slot = slot;
    t.out_kind = BERTX_OUT_PROJ;
    t.stride = N;
    t.ids.resize((size_t)n * N);
    t.lens.resize((size_t)n);
    t.kept.resize((size_t)n);
    t.keys.resize((size_t)n);
    if (doc) t.keep.resize((size_t)n * N);
    std::vector<int32_t> rcs((size_t)n, 0);
    TaskPool::instance().run(((int64_t)n + 7) / 8, n_threads > 0 ? n_threads : 1, [&](int64_t blk) {
        const int e = (int)std::min<int64_t>(n, 8 * blk + 8);
        std::vector<int32_t> all(doc ? 0 : N);   // a query's mask: all ones
        for (int i = (int)(8 * blk); i < e; ++i) {
            int32_t *kp = doc ? t.keep.data() + i * N : all.data();
            rcs[(size_t)i] = bertx_tokenize_colbert_ex(ctx, texts[i], kind, maxlen, t.ids.data() + i * N, kp,
                                                       &t.lens[(size_t)i], &t.keys[(size_t)i]);
            int32_t c = 0;
            for (int32_t j = 0; rcs[(size_t)i] == 0 && j < t.lens[(size_t)i]; ++j) c += kp[j];
            t.kept[(size_t)i] = doc ? c : t.lens[(size_t)i];
        }
    });
    if (doc || bertx_mask_keys(ctx) != 0) t.keys.clear();
    for (int32_t i = 0; i < n; ++i)
        if (rcs[(size_t)i] != 0 || (!doc && t.lens[(size_t)i] != maxlen)) return -1;
    return 0;
}

// The host and device buffers of a call's forwards, reused from chunk to chunk.
struct ChunkBufs {
    std::vector<int32_t> flat, cu, map;
    DevBuf d_ids, d_cu, d_map, d_keys, d_rows;
    int64_t cap_tok = 0, cap_seq = 0;
};

// Grow-only: room for a chunk of tok tokens in seqs texts.
int32_t grow(bertx_mvindex &mv, const TextRows &t, ChunkBufs &b, int64_t tok, int64_t seqs)
{
    if (tok <= b.cap_tok && seqs <= b.cap_seq) return 0;
    if (b.d_rows.p) HIP_RC(hipStreamSynchronize(mv.stream));   // the previous chunk may still read them
    for (DevBuf *d : {&b.d_ids, &b.d_cu, &b.d_map, &b.d_keys, &b.d_rows})
        if (d->p) { (void)hipFree(d->p); d->p = nullptr; }
    b.cap_tok = std::max(tok, b.cap_tok);
    b.cap_seq = std::max(seqs, b.cap_seq);
    HIP_RC(hipMalloc(&b.d_ids.p, (size_t)b.cap_tok * 4));
    HIP_RC(hipMalloc(&b.d_cu.p, (size_t)(b.cap_seq + 1) * 4));
    if (!t.keep.empty()) HIP_RC(hipMalloc(&b.d_map.p, (size_t)b.cap_tok * 4));
    if (!t.keys.empty()) HIP_RC(hipMalloc(&b.d_keys.p, (size_t)b.cap_seq * 4));
    HIP_RC(hipMalloc(&b.d_rows.p, (size_t)b.cap_tok * mv.w * 4));
    return 0;
}

// Texts i0 .. i1 - 1 through one forward on the store's stream: their kept rows, in
// order, f32 [*n_rows][w] at *d_rows (a buffer of b: the next chunk reuses it).  With a
// keep mask the kept tokens' packed positions are the forward's row map.
int32_t forward_chunk(bertx_mvindex &mv, struct bert_ctx *ctx, const TextRows &t, size_t i0, size_t i1, ChunkBufs &b,
                      const float **d_rows, int64_t *n_rows)
{
    const bool mapped = !t.keep.empty(), counted = !t.keys.empty();
    b.flat.clear();
    b.map.clear();
    b.cu.assign(1, 0);
    int32_t max_len = 0;
    for (size_t i = i0; i < i1; ++i) {
        const int32_t *p = t.ids.data() + i * t.stride, len = t.lens[i];
        for (int32_t j = 0; mapped && j < len; ++j)
            if (t.keep[i * t.stride + (size_t)j]) b.map.push_back((int32_t)b.flat.size() + j);
        b.flat.insert(b.flat.end(), p, p + len);
        b.cu.push_back((int32_t)b.flat.size());
        max_len = std::max(max_len, len);
    }
    const int64_t tok = (int64_t)b.flat.size(), seqs = (int64_t)(i1 - i0), rows = mapped ? (int64_t)b.map.size() : tok;
    if (const int32_t rc = grow(mv, t, b, tok, seqs)) return rc;
    if (bertx_reserve(ctx, t.slot, (int32_t)tok, (int32_t)seqs) != 0) return -1;
    HIP_RC(hipMemcpyAsync(b.d_ids.p, b.flat.data(), (size_t)tok * 4, hipMemcpyHostToDevice, mv.stream));
    HIP_RC(hipMemcpyAsync(b.d_cu.p, b.cu.data(), (size_t)(seqs + 1) * 4, hipMemcpyHostToDevice, mv.stream));
    if (mapped) HIP_RC(hipMemcpyAsync(b.d_map.p, b.map.data(), (size_t)rows * 4, hipMemcpyHostToDevice, mv.stream));
    if (counted) HIP_RC(hipMemcpyAsync(b.d_keys.p, t.keys.data() + i0, (size_t)seqs * 4, hipMemcpyHostToDevice, mv.stream));
    *d_rows = (const float *)b.d_rows.p;
    *n_rows = rows;
    return bertx_forward_device_kv(ctx, t.slot, (const int32_t *)b.d_ids.p, nullptr, (const int32_t *)b.d_cu.p,
                                   (const int32_t *)b.d_keys.p, (int32_t)seqs, max_len, (int32_t)tok, t.out_kind,
                                   (const int32_t *)b.d_map.p, (int32_t)rows, (float *)b.d_rows.p, mv.stream);
}

// One document per text.  Chunks of whole texts as run_forward cuts them; each chunk's
// rows go from the forward's device output straight into the pack kernel on the store's
// stream.  who: the entry point, for the messages.
int32_t add_texts(bertx_mvindex &mv, struct bert_ctx *ctx, const TextRows &t, int32_t n, const char *who)
{
    std::lock_guard<std::mutex> lk(mv.mu);
    if (add_refused(mv, who)) return -1;
    int64_t T = 0, slots = 0;
    int32_t rc = plan_add(mv, t.kept.data(), n, &T, &slots);   // (a ColBERT document keeps [CLS], [D] and [SEP]: >= 3)
    if (rc != 0) return rc;
    DeviceGuard g(mv.ordinal);
    HIP_RC(g.status());
    ChunkBufs b;
    {
        Ordered o(mv.ord, mv.stream);
        rc = begin_add(mv, n, slots, mv.stream);
        int64_t t0 = 0;
        for (size_t i = 0; i < (size_t)n && rc == 0;) {
            const size_t e = chunk_end([&](size_t j) { return t.lens[j]; }, i, (size_t)n);
            const float *d_rows = nullptr;
            int64_t rows = 0;
            rc = forward_chunk(mv, ctx, t, i, e, b, &d_rows, &rows);
            if (rc == 0) rc = pack(mv, d_rows, t0, rows, n, mv.stream);
            // the chunk's host and device buffers are reused by the next one
            if (rc == 0 && hipStreamSynchronize(mv.stream) != hipSuccess) rc = -1;
            t0 += rows;
            i = e;
        }
        if (rc == 0) rc = assign_new(mv, n, slots, mv.stream);
    }
    if (rc != 0) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(mv.stream);   // the entries may be rewritten by the next add
        errorf("%s: device %d failed while adding (%d)\n", who, mv.ordinal, rc);
        return rc < 0 ? rc : -1;
    }
    return commit(mv, n, slots);
}

// The one query of t against the host ids.  Ids [L], cu {0, L} and the key count travel
// in the store's token staging and the rows land in its query staging: no device memory
// is allocated per call.
int32_t score_text(bertx_mvindex &mv, struct bert_ctx *ctx, const TextRows &t, const int32_t *ids, int32_t n, float *out)
{
    const int32_t L = t.lens[0];
    std::vector<int32_t> h((size_t)kMaxLq + 3, 0);
    std::memcpy(h.data(), t.ids.data(), (size_t)L * 4);
    h[(size_t)kMaxLq + 1] = L;
    if (!t.keys.empty()) h[(size_t)kMaxLq + 2] = t.keys[0];
    std::lock_guard<std::mutex> lk(mv.mu);
    DeviceGuard g(mv.ordinal);
    HIP_RC(g.status());
    if (bertx_reserve(ctx, t.slot, L, 1) != 0) return -1;
    int32_t rc = 0;
    {
        Ordered o(mv.ord, mv.stream);
        HIP_RC(hipMemcpyAsync(mv.st_tok, h.data(), h.size() * 4, hipMemcpyHostToDevice, mv.stream));
        HIP_RC(hipStreamSynchronize(mv.stream));   // h is pageable and leaves scope
        rc = bertx_forward_device_kv(ctx, t.slot, mv.st_tok, nullptr, mv.st_tok + kMaxLq,
                                     t.keys.empty() ? nullptr : mv.st_tok + kMaxLq + 2, 1, L, L, t.out_kind, nullptr, 0,
                                     mv.st_q, mv.stream);
    }
    if (rc != 0) return rc < 0 ? rc : -1;
    return score_host_ids(mv, mv.st_q, L, ids, n, out);
}

// The n queries of t, kSearchTexts per forward.  The search reads [m][Lmax][w]: a
// forward whose queries all have Lmax rows (the ColBERT form) hands its output over as
// it is; otherwise the rows are laid out with zero rows behind the shorter queries
// (device-to-device) first.  The outputs are written when every chunk succeeded.
int32_t search_texts(bertx_mvindex &mv, struct bert_ctx *ctx, const TextRows &t, int32_t n, int32_t k, float *scores,
                     int32_t *ids, int32_t n_cand = 0)
{
    const size_t w = (size_t)mv.w;
    std::vector<float> hs((size_t)n * k);
    std::vector<int32_t> hi((size_t)n * k);
    std::lock_guard<std::mutex> lk(mv.mu);
    DeviceGuard g(mv.ordinal);
    HIP_RC(g.status());
    const int32_t cap = std::min<int32_t>(n, kSearchTexts);
    const int64_t cap_tok = (int64_t)cap * std::min<int64_t>((int64_t)t.stride, kMaxLq);
    ChunkBufs b;
    DevBuf d_pad;
    if (const int32_t rc = grow(mv, t, b, cap_tok, cap)) return rc;   // once: no chunk is larger
    for (int32_t i0 = 0; i0 < n; i0 += cap) {
        const int32_t m = std::min(cap, n - i0);
        const int32_t Lmax = *std::max_element(t.kept.begin() + i0, t.kept.begin() + i0 + m);
        const float *d_q = nullptr;
        int64_t rows = 0;
        int32_t rc = 0;
        {
            Ordered o(mv.ord, mv.stream);
            rc = forward_chunk(mv, ctx, t, (size_t)i0, (size_t)(i0 + m), b, &d_q, &rows);
            if (rc == 0 && rows != (int64_t)m * Lmax) {
                if (!d_pad.p) HIP_RC(hipMalloc(&d_pad.p, (size_t)cap_tok * w * 4));
                HIP_RC(hipMemsetAsync(d_pad.p, 0, (size_t)m * Lmax * w * 4, mv.stream));
                for (int32_t j = 0; j < m; ++j) {
                    const size_t len = (size_t)t.kept[(size_t)(i0 + j)];
                    HIP_RC(hipMemcpyAsync((float *)d_pad.p + (size_t)j * Lmax * w, d_q, len * w * 4, hipMemcpyDeviceToDevice,
                                          mv.stream));
                    d_q += len * w;
                }
                d_q = (const float *)d_pad.p;
            }
        }
        if (rc == 0)
            rc = search_to_host(mv, d_q, m, Lmax, k, hs.data() + (size_t)i0 * k, hi.data() + (size_t)i0 * k, n_cand);
        if (rc != 0) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(mv.stream);
            return rc < 0 ? rc : -1;
        }
    }
    std::memcpy(scores, hs.data(), hs.size() * 4);
    std::memcpy(ids, hi.data(), hi.size() * 4);
    return 0;
}

bool centroid_count_ok(const char *who, int32_t C)
{
    if (C >= 16 && C <= 65536 && C % 16 == 0) return true;
    errorf("%s: C = %d is not a multiple of 16 in 16 .. 65536\n", who, C);
    return false;
}

// bertx_mvindex_set_centroids under the caller's lock with the device selected.  The
// buffers grow first, all or none; then the rows are packed through the add's staging by
// the store's own pack kernel, as one document of C tokens, and every stored token is coded.
int32_t set_centroids_locked(bertx_mvindex &mv, const float *cent, int32_t C)
{
    if (!cent || !centroid_count_ok("bertx_mvindex_set_centroids", C)) return -1;
    const bool i8 = mv.storage == BERTX_INDEX_I8;
    if (C > mv.cap_C) {
        const size_t slots16 = (size_t)((mv.cap_slots + 15) / 16) * 16;
        DevBuf n_cent, n_u, n_t, n_codes, n_a, n_x, n_i, n_e;
        const bool ok = hipMalloc(&n_cent.p, (size_t)C * mv.w * (i8 ? 1 : 2)) == hipSuccess &&
                        (!i8 || hipMalloc(&n_u.p, (size_t)C * 4) == hipSuccess) &&
                        hipMalloc(&n_t.p, (size_t)256 * C) == hipSuccess &&
                        (mv.codes || (hipMalloc(&n_codes.p, slots16 * 2) == hipSuccess &&
                                      hipMalloc(&n_a.p, (size_t)kCandQueries * kMaxK * 4) == hipSuccess &&
                                      hipMalloc(&n_x.p, (size_t)kCandQueries * kMaxK * 4) == hipSuccess &&
                                      hipMalloc(&n_i.p, (size_t)kCandQueries * kMaxK * 4) == hipSuccess &&
                                      hipMalloc(&n_e.p, 16) == hipSuccess));
        if (!ok) {
            (void)hipGetLastError();
            errorf("bertx_mvindex_set_centroids: device %d could not allocate the buffers of %d centroids\n", mv.ordinal, C);
            return -3;
        }
        HIP_RC(mv.ord.wait());   // the old buffers may still be read
        std::swap(mv.cent, n_cent.p);
        void *u = mv.cent_u, *t = mv.tscratch;
        mv.cent_u = (float *)n_u.p;
        mv.tscratch = (float *)n_t.p;
        n_u.p = u;
        n_t.p = t;
        if (!mv.codes) {
            mv.codes = (uint16_t *)n_codes.p;
            mv.cand_approx = (float *)n_a.p;
            mv.cand_exact = (float *)n_x.p;
            mv.cand_ids = (int32_t *)n_i.p;
            mv.cent_entry = (int32_t *)n_e.p;
            n_codes.p = n_a.p = n_x.p = n_i.p = n_e.p = nullptr;
        }
        mv.cap_C = C;
    }
    mv.C = 0;   // until every step below has been queued
    const int32_t entry[4] = {0, C, 0, 0};
    int32_t rc = 0;
    {
        Ordered o(mv.ord, mv.stream);
        if (hipMemcpyAsync(mv.cent_entry, entry, sizeof entry, hipMemcpyHostToDevice, mv.stream) != hipSuccess) rc = -1;
        for (int64_t t = 0; t < C && rc == 0; t += kStageRows) {
            const int64_t m = std::min<int64_t>(kStageRows, C - t);
            if (hipMemcpyAsync(mv.st_rows, cent + (size_t)t * mv.w, (size_t)m * mv.w * 4, hipMemcpyHostToDevice, mv.stream) !=
                hipSuccess)
                rc = -1;
            if (rc == 0)
                rc = i8 ? launch_mv_pack_i8(mv.st_rows, t, m, mv.w, mv.cent_entry + 2, mv.cent_entry, 1, mv.cent, mv.cent_u,
                                            mv.stream)
                        : launch_mv_pack(mv.st_rows, t, m, mv.w, mv.cent_entry + 2, mv.cent_entry, 1, mv.cent, mv.stream);
            if (rc == 0 && hipStreamSynchronize(mv.stream) != hipSuccess) rc = -1;   // the staging buffer is reused
        }
        if (rc == 0) {
            mv.C = C;
            rc = assign_codes(mv, 0, mv.used_slots / 16, 0, (int32_t)mv.n_docs, mv.stream);
        }
    }
    if (rc != 0) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(mv.stream);
        mv.C = 0;
        errorf("bertx_mvindex_set_centroids: device %d failed (%d); the store has no centroids now\n", mv.ordinal, rc);
    }
    return rc;
}

// B queries on the host through the device form `run`, per results of each: staged through
// buffers of the call, the outputs written when everything succeeded.
template <class Run>
int32_t queries_to_host(bertx_mvindex &mv, const float *q, int32_t B, int32_t Lq, int32_t per, Run run, float *scores,
                        int32_t *ids)
{
    const size_t nq = (size_t)B * Lq * mv.w, nr = (size_t)B * per;
    std::vector<float> hs(nr);
    std::vector<int32_t> hi(nr);
    DevBuf d_q, d_s, d_i;
    HIP_RC(hipMalloc(&d_q.p, nq * 4));
    HIP_RC(hipMalloc(&d_s.p, nr * 4));
    HIP_RC(hipMalloc(&d_i.p, nr * 4));
    HIP_RC(hipMemcpyAsync(d_q.p, q, nq * 4, hipMemcpyHostToDevice, mv.stream));
    const int32_t rc = run((const float *)d_q.p, (float *)d_s.p, (int32_t *)d_i.p);
    if (rc != 0) {
        (void)hipStreamSynchronize(mv.stream);
        return rc;
    }
    HIP_RC(hipMemcpyAsync(hs.data(), d_s.p, nr * 4, hipMemcpyDeviceToHost, mv.stream));
    HIP_RC(hipMemcpyAsync(hi.data(), d_i.p, nr * 4, hipMemcpyDeviceToHost, mv.stream));
    HIP_RC(hipStreamSynchronize(mv.stream));
    std::memcpy(scores, hs.data(), nr * 4);
    std::memcpy(ids, hi.data(), nr * 4);
    return 0;
}

}  // namespace

bertx_mvindex *mvindex_create_on(int ordinal, int w, int64_t cap_docs, int64_t cap_slots, int storage)
{
    if (storage != BERTX_INDEX_F16 && storage != BERTX_INDEX_I8 && storage != BERTX_INDEX_RES2 &&
        storage != BERTX_INDEX_RES4) {
        errorf("bertx_mvindex_create: storage %d is none of BERTX_INDEX_F16, _I8, _RES2, _RES4\n", storage);
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
    const int nb = res_nbits(*mv);
    mv->tomb_words = index_mask_words(cap_docs);
    // a residual store keeps no rows: w nb / 8 bytes of bits and one f32 per slot, and the codec
    const size_t store_bytes = nb ? slots16 * (size_t)w * nb / 8 + slots16 * 4 : slots16 * (size_t)w * (i8 ? 1 : 2);
    const bool ok = maxsim_prepare_device() == 0 && maxsim_search_prepare_device() == 0 &&
                    maxsim_codes_prepare_device() == 0 && maxsim_approx_prepare_device() == 0 &&
                    hipMalloc(&mv->search_scratch, maxsim_search_scratch_bytes()) == hipSuccess &&
                    hipStreamCreateWithFlags(&mv->stream, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&mv->ord.done, hipEventDisableTiming) == hipSuccess &&
                    (nb ? maxsim_res_prepare_device() == 0 &&
                              hipMalloc((void **)&mv->res_bits, slots16 * (size_t)w * nb / 8) == hipSuccess &&
                              hipMalloc((void **)&mv->res_u, slots16 * 4) == hipSuccess &&
                              hipMalloc((void **)&mv->res_cuts, 64) == hipSuccess &&
                              hipMalloc((void **)&mv->res_wts, 32) == hipSuccess &&
                              hipMalloc((void **)&mv->res_pair, 1024) == hipSuccess
                        : hipMalloc(&mv->store, store_bytes) == hipSuccess) &&
                    (!i8 || hipMalloc((void **)&mv->scales, slots16 * 4) == hipSuccess) &&
                    hipMalloc((void **)&mv->table, (size_t)cap_docs * 8) == hipSuccess &&
                    hipMalloc((void **)&mv->src_off, (size_t)cap_docs * 4) == hipSuccess &&
                    hipHostMalloc((void **)&mv->h_table, (size_t)cap_docs * 8, hipHostMallocDefault) == hipSuccess &&
                    hipHostMalloc((void **)&mv->h_src, (size_t)cap_docs * 4, hipHostMallocDefault) == hipSuccess &&
                    hipMalloc((void **)&mv->st_rows, (size_t)kStageRows * w * 4) == hipSuccess &&
                    hipMalloc((void **)&mv->st_q, (size_t)kMaxLq * w * 4) == hipSuccess &&
                    hipMalloc((void **)&mv->st_out, (size_t)kStageIds * 4) == hipSuccess &&
                    hipMalloc((void **)&mv->st_ids, (size_t)kStageIds * 4) == hipSuccess &&
                    hipMalloc((void **)&mv->st_tok, (size_t)(kMaxLq + 3) * 4) == hipSuccess &&
                    hipMalloc((void **)&mv->tomb, (size_t)mv->tomb_words * 4) == hipSuccess &&
                    hipMemsetAsync(mv->tomb, 0, (size_t)mv->tomb_words * 4, mv->stream) == hipSuccess &&
                    hipStreamSynchronize(mv->stream) == hipSuccess;
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
    // (the embedding index keeps no such images and does not wait)
    HIP_RC(mv->ord.wait());
    if (mv->removed) {
        // the tombstones back to zero, ordered behind every operation so far
        emb::Ordered o(mv->ord, mv->stream);
        HIP_RC(hipMemsetAsync(mv->tomb, 0, (size_t)mv->tomb_words * 4, mv->stream));
        mv->removed = false;
    }
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
    if (emb::add_refused(*mv, "bertx_mvindex_add")) return -1;
    int64_t T = 0, slots = 0;
    int32_t rc = emb::plan_add(*mv, lens, n, &T, &slots);
    if (rc != 0) return rc;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    {
        emb::Ordered o(mv->ord, mv->stream);
        rc = emb::begin_add(*mv, n, slots, mv->stream);
        for (int64_t t = 0; t < T && rc == 0; t += emb::kStageRows) {
            const int64_t m = std::min<int64_t>(emb::kStageRows, T - t);
            if (hipMemcpyAsync(mv->st_rows, rows + (size_t)t * mv->w, (size_t)m * mv->w * 4, hipMemcpyHostToDevice,
                               mv->stream) != hipSuccess)
                rc = -1;
            if (rc == 0) rc = emb::pack(*mv, mv->st_rows, t, m, n, mv->stream);
            if (rc == 0 && hipStreamSynchronize(mv->stream) != hipSuccess) rc = -1;   // the staging buffer is reused
        }
        if (rc == 0) rc = emb::assign_new(*mv, n, slots, mv->stream);
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
    return emb::doc_locked(mv, id, out);
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
        emb::TextRows t;
        if (emb::tokenize_plain(ctx, n_threads, n, texts, slot, t) != 0) return -1;
        const int32_t n_max = bert_n_max_tokens(ctx);
        for (int32_t i = 0; i < n; ++i)
            if (t.lens[(size_t)i] > n_max) {
                emb::errorf("Too many tokens, maximum is %d\n", n_max);
                emb::errorf("bertx_mvindex_add_texts: text %d has %d tokens; nothing was added\n", i, t.lens[(size_t)i]);
                return -4;
            }
        return emb::add_texts(*mv, ctx, t, n, "bertx_mvindex_add_texts");
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
        emb::TextRows t;
        if (emb::tokenize_plain(ctx, 1, 1, &query, slot, t) != 0) return -1;
        const int32_t n_max = bert_n_max_tokens(ctx), L = t.lens[0];
        if (L > n_max || L > emb::kMaxLq) {
            emb::errorf("bertx_mvindex_score_text: the query has %d tokens, maximum is %d\n", L,
                        std::min<int32_t>(n_max, emb::kMaxLq));
            return -4;
        }
        if (L < 1) return -1;
        return emb::score_text(*mv, ctx, t, ids, n, out);
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
        emb::TextRows t;
        if (emb::tokenize_colbert(ctx, n_threads, n, texts, 1, doc_maxlen, slot, t) != 0) return -1;
        return emb::add_texts(*mv, ctx, t, n, "bertx_mvindex_add_texts_colbert");
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
        emb::TextRows t;
        if (emb::tokenize_colbert(ctx, 1, 1, &query, 0, query_maxlen, slot, t) != 0) return -1;
        return emb::score_text(*mv, ctx, t, ids, n, out);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_mvindex_score_text_colbert: %s\n", ex.what());
        return -1;
    }
}

int32_t bertx_mvindex_search_filtered_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq, int32_t k,
                                             const uint32_t *d_filters, int32_t n_filters, int32_t words, float *d_scores,
                                             int32_t *d_ids, void *stream)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (!emb::filters_fit(mv->n_docs, d_filters, n_filters, words, B)) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    return emb::search_device_locked(*mv, d_q, B, Lq, k, d_scores, d_ids, stream ? (hipStream_t)stream : mv->stream,
                                     emb::filters_of(d_filters, n_filters, words));
}

int32_t bertx_mvindex_search_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq, int32_t k,
                                    float *d_scores, int32_t *d_ids, void *stream)
{
    return bertx_mvindex_search_filtered_device(mv, d_q, B, Lq, k, nullptr, 0, 0, d_scores, d_ids, stream);
}

int32_t bertx_mvindex_search_filtered(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t k,
                                      const uint32_t *filters, int32_t n_filters, int32_t words, float *scores, int32_t *ids)
{
    if (!mv || !q || !scores || !ids || !emb::search_args_ok("bertx_mvindex_search", B, Lq, k)) return -1;
    if (emb::full_scan_refused(*mv, "bertx_mvindex_search")) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (!emb::filters_fit(mv->n_docs, filters, n_filters, words, B)) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    emb::DevBuf fbuf;   // (freed after the call's synchronise)
    try {
        HIP_RC(emb::stage_filters(mv->stream, filters, n_filters, words, fbuf));
        const emb::Filters f = emb::filters_of((const uint32_t *)fbuf.p, n_filters, words);
        return emb::queries_to_host(*mv, q, B, Lq, k, [&](const float *dq, float *ds, int32_t *di) {
            return emb::search_device_locked(*mv, dq, B, Lq, k, ds, di, mv->stream, f);
        }, scores, ids);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_search: out of host memory\n");
        return -1;
    }
}

int32_t bertx_mvindex_search(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t k, float *scores,
                             int32_t *ids)
{
    return bertx_mvindex_search_filtered(mv, q, B, Lq, k, nullptr, 0, 0, scores, ids);
}

int32_t bertx_mvindex_remove_device(struct bertx_mvindex *mv, const int32_t *d_ids, int32_t n, void *stream)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    return emb::remove_device_locked(*mv, d_ids, n, stream ? (hipStream_t)stream : mv->stream);
}

int32_t bertx_mvindex_remove(struct bertx_mvindex *mv, const int32_t *ids, int32_t n)
{
    if (!mv || !ids || n < 1) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    for (int32_t i = 0; i < n; i += emb::kStageIds) {
        const int32_t m = std::min(emb::kStageIds, n - i);
        HIP_RC(hipMemcpyAsync(mv->st_ids, ids + i, (size_t)m * 4, hipMemcpyHostToDevice, mv->stream));
        const int32_t rc = emb::remove_device_locked(*mv, mv->st_ids, m, mv->stream);
        if (rc != 0) return rc;
        HIP_RC(hipStreamSynchronize(mv->stream));   // the staging buffer is reused
    }
    return 0;
}

int32_t bertx_mvindex_live(struct bertx_mvindex *mv)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    int32_t dead = 0;
    {
        emb::Ordered o(mv->ord, mv->stream);
        const int rc = emb::launch_index_count_deleted(mv->tomb, mv->n_docs, mv->st_ids, mv->stream);
        if (rc != 0) return rc;
        HIP_RC(hipMemcpyAsync(&dead, mv->st_ids, 4, hipMemcpyDeviceToHost, mv->stream));
    }
    HIP_RC(hipStreamSynchronize(mv->stream));
    return (int32_t)mv->n_docs - dead;
}

int32_t bertx_mvindex_deleted(struct bertx_mvindex *mv, int32_t first, int32_t n, uint8_t *out)
{
    if (!mv || !out || first < 0 || n < 1) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if ((int64_t)first + n > mv->n_docs) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    try {
        // the caller's output is written only once every chunk has succeeded
        std::vector<uint8_t> flags((size_t)n);
        constexpr int32_t kChunk = emb::kStageIds * 4;   // bytes of the id staging buffer, one flag each
        for (int32_t i = 0; i < n; i += kChunk) {
            const int32_t m = std::min(kChunk, n - i);
            {
                emb::Ordered o(mv->ord, mv->stream);
                const int rc = emb::launch_index_deleted_flags(mv->tomb, (int64_t)first + i, m, (uint8_t *)mv->st_ids,
                                                               mv->stream);
                if (rc != 0) return rc;
                HIP_RC(hipMemcpyAsync(flags.data() + i, mv->st_ids, (size_t)m, hipMemcpyDeviceToHost, mv->stream));
            }
            HIP_RC(hipStreamSynchronize(mv->stream));
        }
        std::memcpy(out, flags.data(), flags.size());
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_deleted: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_mvindex_search_texts(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                   const char **texts, int32_t k, float *scores, int32_t *ids)
{
    int32_t slot = -1;
    if (!texts || !scores || !ids || n < 1) return -1;
    if (emb::text_ctx_ok(mv, ctx, "bertx_mvindex_search_texts", &slot) != 0) return -1;
    if (emb::full_scan_refused(*mv, "bertx_mvindex_search_texts")) return -1;
    if (!emb::search_args_ok("bertx_mvindex_search_texts", n, 1, k)) return -1;
    try {
        emb::TextRows t;
        if (emb::tokenize_plain(ctx, n_threads, n, texts, slot, t) != 0) return -1;
        const int32_t lim = std::min<int32_t>(bert_n_max_tokens(ctx), emb::kMaxLq);
        for (int32_t i = 0; i < n; ++i) {
            if (t.lens[(size_t)i] > lim) {
                emb::errorf("bertx_mvindex_search_texts: query %d has %d tokens, maximum is %d\n", i, t.lens[(size_t)i], lim);
                return -4;
            }
            if (t.lens[(size_t)i] < 1) return -1;
        }
        return emb::search_texts(*mv, ctx, t, n, k, scores, ids);
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
    if (emb::full_scan_refused(*mv, "bertx_mvindex_search_texts_colbert")) return -1;
    if (query_maxlen < 4 || query_maxlen > emb::kMaxLq || query_maxlen > bert_n_max_tokens(ctx)) return -1;
    if (!emb::search_args_ok("bertx_mvindex_search_texts_colbert", n, query_maxlen, k)) return -1;
    for (int32_t i = 0; i < n; ++i)
        if (!texts[i]) return -1;
    try {
        emb::TextRows t;
        if (emb::tokenize_colbert(ctx, n_threads, n, texts, 0, query_maxlen, slot, t) != 0) return -1;
        return emb::search_texts(*mv, ctx, t, n, k, scores, ids);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_mvindex_search_texts_colbert: %s\n", ex.what());
        return -1;
    }
}

int32_t bertx_mvindex_set_centroids(struct bertx_mvindex *mv, const float *cent, int32_t C)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (!cent || !emb::centroid_count_ok("bertx_mvindex_set_centroids", C)) return -1;
    if (emb::res_nbits(*mv) && mv->n_docs > 0) {
        emb::errorf("bertx_mvindex_set_centroids: a residual store with documents keeps no rows to code again\n");
        return -1;
    }
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    return emb::set_centroids_locked(*mv, cent, C);
}

int32_t bertx_mvindex_set_residual_buckets(struct bertx_mvindex *mv, const float *cutoffs, const float *weights)
{
    if (!mv || !cutoffs || !weights) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    const int nb = emb::res_nbits(*mv);
    if (!nb || mv->n_docs > 0) {
        emb::errorf("bertx_mvindex_set_residual_buckets: %s\n",
                    nb ? "the store holds documents encoded with its buckets" : "not a residual store");
        return -1;
    }
    const int nw = 1 << nb;
    for (int k = 0; k < nw; ++k)
        if (!std::isfinite(weights[k]) || (k < nw - 1 && !std::isfinite(cutoffs[k])) ||
            (k > 0 && k < nw - 1 && cutoffs[k] < cutoffs[k - 1])) {
            emb::errorf("bertx_mvindex_set_residual_buckets: cutoffs must be finite and non-decreasing, weights finite\n");
            return -1;
        }
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    float cuts[15] = {};
    uint16_t wts[16] = {};
    uint32_t pair[256] = {};
    for (int k = 0; k < nw - 1; ++k) cuts[k] = cutoffs[k];
    for (int k = 0; k < nw; ++k) wts[k] = emb::f32_to_f16(weights[k]);
    for (int b1 = 0; b1 < nw; ++b1)
        for (int b0 = 0; b0 < nw; ++b0) pair[b0 | (b1 << nb)] = (uint32_t)wts[b0] | ((uint32_t)wts[b1] << 16);
    HIP_RC(mv->ord.wait());   // an empty store's scorer still copies the pair table
    HIP_RC(hipMemcpy(mv->res_cuts, cuts, sizeof cuts, hipMemcpyHostToDevice));
    HIP_RC(hipMemcpy(mv->res_wts, wts, sizeof wts, hipMemcpyHostToDevice));
    HIP_RC(hipMemcpy(mv->res_pair, pair, sizeof pair, hipMemcpyHostToDevice));
    std::memcpy(mv->h_wts, wts, sizeof wts);
    mv->has_buckets = true;
    return 0;
}

int32_t bertx_mvindex_doc_residual(struct bertx_mvindex *mv, int32_t id, uint16_t *codes, uint8_t *bits, float *u)
{
    if (!mv || !codes || !bits || !u) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    const int nb = emb::res_nbits(*mv);
    if (!nb || id < 0 || id >= mv->n_docs) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    try {
        // through buffers of its own: a failed copy leaves the outputs untouched
        const int64_t len = mv->h_table[2 * (size_t)id + 1];
        std::vector<uint16_t> hc((size_t)len);
        std::vector<uint8_t> hb((size_t)len * mv->w * nb / 8);
        std::vector<float> hu((size_t)len);
        const int32_t rc = emb::read_doc_res(*mv, id, hc.data(), hb.data(), hu.data());
        if (rc != 0) return rc;
        std::memcpy(codes, hc.data(), hc.size() * 2);
        std::memcpy(bits, hb.data(), hb.size());
        std::memcpy(u, hu.data(), hu.size() * 4);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_doc_residual: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_mvindex_train_residual_buckets(struct bertx_mvindex *src, int32_t nbits, float *cutoffs, float *weights)
{
    if (!src || !cutoffs || !weights) return -1;
    std::lock_guard<std::mutex> lk(src->mu);
    if (src->storage != BERTX_INDEX_F16 || src->C == 0 || src->n_docs < 1 || (nbits != 2 && nbits != 4)) {
        emb::errorf("bertx_mvindex_train_residual_buckets: needs an f16 store with centroids and documents, and 2 or 4 "
                    "bits\n");
        return -1;
    }
    DeviceGuard g(src->ordinal);
    HIP_RC(g.status());
    try {
        const int w = src->w;
        int64_t T = 0;
        for (int64_t d = 0; d < src->n_docs; ++d) T += src->h_table[2 * (size_t)d + 1];
        const int64_t stride = std::max<int64_t>(1, (T + 65535) / 65536);
        std::vector<float> cent, rows, res;
        if (const int32_t rc = emb::read_centroids_f16(*src, cent)) return rc;
        std::vector<uint16_t> codes((size_t)src->used_slots);
        HIP_RC(hipMemcpy(codes.data(), src->codes, codes.size() * 2, hipMemcpyDeviceToHost));
        res.reserve((size_t)((T + stride - 1) / stride) * w);
        int64_t t0 = 0, next = 0;
        for (int32_t d = 0; d < src->n_docs; ++d) {
            const int64_t first = src->h_table[2 * (size_t)d], len = src->h_table[2 * (size_t)d + 1];
            if (next < t0 + len) {
                rows.resize((size_t)len * w);
                if (const int32_t rc = emb::doc_locked(src, d, rows.data())) return rc;
                for (; next < t0 + len; next += stride) {
                    const float *v = rows.data() + (size_t)(next - t0) * w;
                    const float *c = cent.data() + (size_t)codes[(size_t)(first * 16 + (next - t0))] * w;
                    for (int i = 0; i < w; ++i) res.push_back(v[i] - c[i]);
                }
            }
            t0 += len;
        }
        std::sort(res.begin(), res.end());
        const int64_t n = (int64_t)res.size(), nw = (int64_t)1 << nbits;
        std::vector<float> hc((size_t)nw - 1), hw((size_t)nw);
        for (int64_t k = 1; k < nw; ++k) hc[(size_t)k - 1] = res[(size_t)std::min(n - 1, k * n / nw)];
        for (int64_t k = 0; k < nw; ++k) hw[(size_t)k] = res[(size_t)std::min(n - 1, (2 * k + 1) * n / (2 * nw))];
        std::memcpy(cutoffs, hc.data(), hc.size() * 4);
        std::memcpy(weights, hw.data(), hw.size() * 4);
        return 0;
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_train_residual_buckets: out of host memory\n");
        return -1;
    }
}

int32_t bertx_mvindex_centroids(struct bertx_mvindex *mv)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    return mv->C;
}

int32_t bertx_mvindex_centroid(struct bertx_mvindex *mv, int32_t c, float *out)
{
    if (!mv || !out) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (c < 0 || c >= mv->C) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    try {
        const int w = mv->w;
        const size_t grp = (size_t)(c / 16);
        HIP_RC(mv->ord.wait());
        if (mv->storage == BERTX_INDEX_I8) {
            std::vector<int8_t> raw((size_t)16 * w), q((size_t)w);
            float u = 0.f;
            HIP_RC(hipMemcpy(raw.data(), (const int8_t *)mv->cent + grp * raw.size(), raw.size(), hipMemcpyDeviceToHost));
            HIP_RC(hipMemcpy(&u, mv->cent_u + c, 4, hipMemcpyDeviceToHost));
            emb::unpack_i8_rows(raw.data(), (int64_t)grp * 16, c, 1, w, q.data());
            for (int i = 0; i < w; ++i) out[i] = (float)q[(size_t)i] * u;
        } else {
            std::vector<uint16_t> raw((size_t)16 * w);
            std::vector<float> row((size_t)w);
            HIP_RC(hipMemcpy(raw.data(), (const uint16_t *)mv->cent + grp * raw.size(), raw.size() * 2, hipMemcpyDeviceToHost));
            emb::unpack_f16_rows(raw.data(), (int64_t)grp * 16, c, 1, w, row.data());
            std::memcpy(out, row.data(), row.size() * 4);
        }
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_centroid: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_mvindex_doc_codes(struct bertx_mvindex *mv, int32_t id, uint16_t *codes)
{
    if (!mv || !codes) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (mv->C == 0 || id < 0 || id >= mv->n_docs) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    try {
        const int64_t first = mv->h_table[2 * (size_t)id], len = mv->h_table[2 * (size_t)id + 1];
        std::vector<uint16_t> h((size_t)len);
        HIP_RC(mv->ord.wait());
        HIP_RC(hipMemcpy(h.data(), mv->codes + (size_t)first * 16, h.size() * 2, hipMemcpyDeviceToHost));
        std::memcpy(codes, h.data(), h.size() * 2);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_doc_codes: out of host memory\n");
        return -1;
    }
    return 0;
}

int32_t bertx_mvindex_train_centroids(struct bertx_mvindex *mv, int32_t C, int32_t iters, uint32_t seed)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (!emb::centroid_count_ok("bertx_mvindex_train_centroids", C)) return -1;
    if (emb::res_nbits(*mv)) {
        emb::errorf("bertx_mvindex_train_centroids: a residual store keeps no rows to train from (train on an f16 store)\n");
        return -1;
    }
    if (iters < 0 || mv->n_docs < 1) {
        emb::errorf("bertx_mvindex_train_centroids: iters = %d, %lld documents: nothing to train on\n", iters,
                    (long long)mv->n_docs);
        return -1;
    }
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    try {
        const int w = mv->w;
        int64_t T = 0;
        for (int64_t d = 0; d < mv->n_docs; ++d) T += mv->h_table[2 * (size_t)d + 1];
        const emb::KmeansSample sm = emb::kmeans_sample(T, seed);
        if (C > sm.n) {
            emb::errorf("bertx_mvindex_train_centroids: C = %d exceeds the sample of %lld token rows\n", C, (long long)sm.n);
            return -1;
        }
        // the sample's rows (bertx_mvindex_doc's values) and the slots their codes sit in
        std::vector<float> sample((size_t)sm.n * w), rows;
        std::vector<int64_t> slot((size_t)sm.n);
        int64_t t0 = 0, next = sm.start, i = 0;
        for (int32_t d = 0; d < mv->n_docs; ++d) {
            const int64_t first = mv->h_table[2 * (size_t)d], len = mv->h_table[2 * (size_t)d + 1];
            if (next < t0 + len) {
                rows.resize((size_t)len * w);
                const int32_t rc = emb::doc_locked(mv, d, rows.data());
                if (rc != 0) return rc;
                for (; next < t0 + len; next += sm.stride, ++i) {
                    std::memcpy(sample.data() + (size_t)i * w, rows.data() + (size_t)(next - t0) * w, (size_t)w * 4);
                    slot[(size_t)i] = first * 16 + (next - t0);
                }
            }
            t0 += len;
        }
        std::vector<float> cent((size_t)C * w);
        for (int64_t c = 0; c < C; ++c)
            std::memcpy(cent.data() + (size_t)c * w, sample.data() + (size_t)emb::kmeans_initial_row(c, sm.n, C) * w,
                        (size_t)w * 4);
        std::vector<uint16_t> all((size_t)mv->used_slots), codes((size_t)sm.n);
        for (int32_t it = 0; it < iters; ++it) {
            const int32_t rc = emb::set_centroids_locked(*mv, cent.data(), C);
            if (rc != 0) return rc;
            HIP_RC(mv->ord.wait());
            HIP_RC(hipMemcpy(all.data(), mv->codes, all.size() * 2, hipMemcpyDeviceToHost));
            for (int64_t j = 0; j < sm.n; ++j) codes[(size_t)j] = all[(size_t)slot[(size_t)j]];
            (void)emb::kmeans_update(sample.data(), codes.data(), sm.n, w, C, cent.data());
        }
        return emb::set_centroids_locked(*mv, cent.data(), C);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_train_centroids: out of host memory\n");
        return -1;
    }
}

int32_t bertx_test_kmeans_update(const float *sample, const uint16_t *codes, int32_t n, int32_t w, int32_t C, float *cent)
{
    if (!sample || !codes || !cent || n < 0 || w < 1 || C < 1) return -1;
    return (int32_t)emb::kmeans_update(sample, codes, n, w, C, cent);
}

int32_t bertx_test_kmeans_sample(int64_t T, uint32_t seed, int64_t *out3)
{
    if (!out3 || T < 0) return -1;
    const emb::KmeansSample s = emb::kmeans_sample(T, seed);
    out3[0] = s.stride;
    out3[1] = s.start;
    out3[2] = s.n;
    return 0;
}

int32_t bertx_test_approx_ran(int32_t reset)
{
    return reset ? emb::g_approx_forms.exchange(0) : emb::g_approx_forms.load();
}

int32_t bertx_test_mvindex_grid(struct bertx_mvindex *mv, int32_t max_wg)
{
    if (!mv || max_wg < 0) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    const int32_t before = mv->grid_cap;
    mv->grid_cap = max_wg;
    return before;
}

int32_t bertx_test_mvindex_last_grid(struct bertx_mvindex *mv)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    return mv->last_grid;
}

int32_t bertx_test_mvindex_last_masked(struct bertx_mvindex *mv)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    return mv->last_masked;
}

int32_t bertx_mvindex_candidates_filtered_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq,
                                                 int32_t n_cand, const uint32_t *d_filters, int32_t n_filters, int32_t words,
                                                 float *d_approx, int32_t *d_ids, void *stream)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (!emb::filters_fit(mv->n_docs, d_filters, n_filters, words, B)) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    return emb::candidates_device_locked(*mv, d_q, B, Lq, n_cand, d_approx, d_ids, stream ? (hipStream_t)stream : mv->stream,
                                         emb::filters_of(d_filters, n_filters, words));
}

int32_t bertx_mvindex_candidates_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq, int32_t n_cand,
                                        float *d_approx, int32_t *d_ids, void *stream)
{
    return bertx_mvindex_candidates_filtered_device(mv, d_q, B, Lq, n_cand, nullptr, 0, 0, d_approx, d_ids, stream);
}

int32_t bertx_mvindex_candidates_filtered(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t n_cand,
                                          const uint32_t *filters, int32_t n_filters, int32_t words, float *approx,
                                          int32_t *ids)
{
    if (!mv || !q || !approx || !ids) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (!emb::pruned_args_ok(*mv, "bertx_mvindex_candidates", B, Lq, 1, n_cand)) return -1;
    if (!emb::filters_fit(mv->n_docs, filters, n_filters, words, B)) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    emb::DevBuf fbuf;   // (freed after the call's synchronise)
    try {
        HIP_RC(emb::stage_filters(mv->stream, filters, n_filters, words, fbuf));
        const emb::Filters f = emb::filters_of((const uint32_t *)fbuf.p, n_filters, words);
        return emb::queries_to_host(*mv, q, B, Lq, n_cand, [&](const float *dq, float *ds, int32_t *di) {
            return emb::candidates_device_locked(*mv, dq, B, Lq, n_cand, ds, di, mv->stream, f);
        }, approx, ids);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_candidates: out of host memory\n");
        return -1;
    }
}

int32_t bertx_mvindex_candidates(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t n_cand,
                                 float *approx, int32_t *ids)
{
    return bertx_mvindex_candidates_filtered(mv, q, B, Lq, n_cand, nullptr, 0, 0, approx, ids);
}

int32_t bertx_mvindex_search_pruned_filtered_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq,
                                                    int32_t k, int32_t n_cand, const uint32_t *d_filters, int32_t n_filters,
                                                    int32_t words, float *d_scores, int32_t *d_ids, void *stream)
{
    if (!mv) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (!emb::filters_fit(mv->n_docs, d_filters, n_filters, words, B)) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    return emb::search_pruned_device_locked(*mv, d_q, B, Lq, k, n_cand, d_scores, d_ids,
                                            stream ? (hipStream_t)stream : mv->stream,
                                            emb::filters_of(d_filters, n_filters, words));
}

int32_t bertx_mvindex_search_pruned_device(struct bertx_mvindex *mv, const float *d_q, int32_t B, int32_t Lq, int32_t k,
                                           int32_t n_cand, float *d_scores, int32_t *d_ids, void *stream)
{
    return bertx_mvindex_search_pruned_filtered_device(mv, d_q, B, Lq, k, n_cand, nullptr, 0, 0, d_scores, d_ids, stream);
}

int32_t bertx_mvindex_search_pruned_filtered(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t k,
                                             int32_t n_cand, const uint32_t *filters, int32_t n_filters, int32_t words,
                                             float *scores, int32_t *ids)
{
    if (!mv || !q || !scores || !ids) return -1;
    std::lock_guard<std::mutex> lk(mv->mu);
    if (!emb::pruned_args_ok(*mv, "bertx_mvindex_search_pruned", B, Lq, k, n_cand)) return -1;
    if (!emb::filters_fit(mv->n_docs, filters, n_filters, words, B)) return -1;
    DeviceGuard g(mv->ordinal);
    HIP_RC(g.status());
    emb::DevBuf fbuf;   // (freed after the call's synchronise)
    try {
        HIP_RC(emb::stage_filters(mv->stream, filters, n_filters, words, fbuf));
        const emb::Filters f = emb::filters_of((const uint32_t *)fbuf.p, n_filters, words);
        return emb::queries_to_host(*mv, q, B, Lq, k, [&](const float *dq, float *ds, int32_t *di) {
            return emb::search_pruned_device_locked(*mv, dq, B, Lq, k, n_cand, ds, di, mv->stream, f);
        }, scores, ids);
    } catch (const std::bad_alloc &) {
        emb::errorf("bertx_mvindex_search_pruned: out of host memory\n");
        return -1;
    }
}

int32_t bertx_mvindex_search_pruned(struct bertx_mvindex *mv, const float *q, int32_t B, int32_t Lq, int32_t k,
                                    int32_t n_cand, float *scores, int32_t *ids)
{
    return bertx_mvindex_search_pruned_filtered(mv, q, B, Lq, k, n_cand, nullptr, 0, 0, scores, ids);
}

int32_t bertx_mvindex_search_pruned_texts(struct bertx_mvindex *mv, struct bert_ctx *ctx, int32_t n_threads, int32_t n,
                                          const char **texts, int32_t k, int32_t n_cand, int32_t colbert_query_maxlen,
                                          float *scores, int32_t *ids)
{
    int32_t slot = -1;
    const char *who = "bertx_mvindex_search_pruned_texts";
    if (!texts || !scores || !ids || n < 1) return -1;
    const bool colbert = colbert_query_maxlen != 0;
    if (colbert) {
        if (const int32_t rc = emb::colbert_ctx_ok(mv, ctx, who, &slot)) return rc;
        if (colbert_query_maxlen < 4 || colbert_query_maxlen > emb::kMaxLq || colbert_query_maxlen > bert_n_max_tokens(ctx))
            return -1;
    } else if (emb::text_ctx_ok(mv, ctx, who, &slot) != 0) {
        return -1;
    }
    {
        std::lock_guard<std::mutex> lk(mv->mu);
        if (!emb::pruned_args_ok(*mv, who, n, colbert ? colbert_query_maxlen : 1, k, n_cand)) return -1;
    }
    for (int32_t i = 0; i < n; ++i)
        if (!texts[i]) return -1;
    try {
        emb::TextRows t;
        if (colbert) {
            if (emb::tokenize_colbert(ctx, n_threads, n, texts, 0, colbert_query_maxlen, slot, t) != 0) return -1;
        } else {
            if (emb::tokenize_plain(ctx, n_threads, n, texts, slot, t) != 0) return -1;
            const int32_t lim = std::min<int32_t>(bert_n_max_tokens(ctx), emb::kMaxLq);
            for (int32_t i = 0; i < n; ++i) {
                if (t.lens[(size_t)i] > lim) {
                    emb::errorf("%s: query %d has %d tokens, maximum is %d\n", who, i, t.lens[(size_t)i], lim);
                    return -4;
                }
                if (t.lens[(size_t)i] < 1) return -1;
            }
        }
        return emb::search_texts(*mv, ctx, t, n, k, scores, ids, n_cand);
    } catch (const std::exception &ex) {
        emb::errorf("%s: %s\n", who, ex.what());
        return -1;
    }
}

}  // extern "C"

namespace {

// What the MaxSim micro-benchmarks share (bench_store, bench_res; bert_hip.h): device 0
// selected, no context; the documents' lens and the candidates' ids from hashes; a stream
// with two events; the fill, query and result buffers; the stores, released with the rest.
struct MaxsimBench {
    static constexpr int64_t kFillRows = 1 << 18;
    const int32_t w, n_docs, iters;
    std::vector<int32_t> lens, ids;
    int64_t slots = 0;
    emb::DeviceGuard guard{0};
    bertx_mvindex *mv = nullptr, *aux = nullptr;   // the store that is timed; bench_res: the f16 store that trains the codec
    hipStream_t s = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    emb::DevBuf rows, q, id, out, oid;

    // ragged (doc_len 0): 16 .. 512 tokens by a hash of the id
    MaxsimBench(int32_t w_, int32_t n_docs_, int32_t doc_len, int32_t n_cand, int32_t iters_)
        : w(w_), n_docs(n_docs_), iters(iters_), lens((size_t)n_docs_), ids((size_t)n_cand)
    {
        for (int32_t i = 0; i < n_docs; ++i) {
            uint32_t h = (uint32_t)i * 2654435761u + 99u;
            h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
            lens[(size_t)i] = doc_len ? doc_len : 16 + (int32_t)(h % 497u);
            slots += (lens[(size_t)i] + 15) / 16 * 16;
        }
        for (int32_t c = 0; c < n_cand; ++c) ids[(size_t)c] = (int32_t)(((uint64_t)c * 2654435761ull + 12345ull) % (uint64_t)n_docs);
    }
    ~MaxsimBench()
    {
        if (s) (void)hipStreamSynchronize(s);
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        if (s) (void)hipStreamDestroy(s);
        bertx_mvindex_free(aux);
        bertx_mvindex_free(mv);
    }

    // the stream, the events and the buffers of nq queries
    int32_t init(int32_t nq)
    {
        using namespace emb;
        HIP_RC(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        HIP_RC(hipEventCreate(&a));
        HIP_RC(hipEventCreate(&b));
        HIP_RC(hipMalloc(&rows.p, (size_t)(kFillRows + 4096) * w * 4));
        HIP_RC(hipMalloc(&q.p, (size_t)nq * kMaxLq * w * 4));
        HIP_RC(hipMalloc(&id.p, ids.size() * 4));
        HIP_RC(hipMalloc(&out.p, (size_t)std::max((int32_t)ids.size(), nq * kMaxK) * 4));
        HIP_RC(hipMalloc(&oid.p, (size_t)nq * kMaxK * 4));
        return 0;
    }

    // every document into `store`, up to kFillRows unit rows per add (seed 12345 + first id)
    int32_t fill(bertx_mvindex *store)
    {
        for (int32_t i = 0; i < n_docs;) {
            int32_t j = i;
            int64_t n = 0;
            while (j < n_docs && (j == i || n + lens[(size_t)j] <= kFillRows)) n += lens[(size_t)j++];
            if (emb::launch_unit_rows((float *)rows.p, n, w, 12345u + (uint32_t)i, s) != 0) return -1;
            if (bertx_mvindex_add_device(store, (const float *)rows.p, lens.data() + i, j - i, s) < 0) return -1;
            HIP_RC(hipStreamSynchronize(s));   // the fill buffer is reused
            i = j;
        }
        return 0;
    }

    // nq queries of Lq unit rows (seed 777) and the candidates' ids, on the device
    int32_t queries(int32_t nq, int32_t Lq)
    {
        if (emb::launch_unit_rows((float *)q.p, (int64_t)nq * Lq, w, 777u, s) != 0) return -1;
        HIP_RC(hipMemcpyAsync(id.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, s));
        HIP_RC(hipStreamSynchronize(s));
        return 0;
    }

    // the mean of `iters` calls of fn after three, by the events
    template <class F>
    int32_t timed(F &&fn, float *us)
    {
        for (int i = 0; i < 3; ++i)
            if (fn() != 0) return -1;
        HIP_RC(hipEventRecord(a, s));
        for (int i = 0; i < iters; ++i)
            if (fn() != 0) return -1;
        HIP_RC(hipEventRecord(b, s));
        HIP_RC(hipEventSynchronize(b));
        float ms = 0.f;
        HIP_RC(hipEventElapsedTime(&ms, a, b));
        *us = ms * 1000.f / (float)iters;
        return 0;
    }

    // C hash-chosen rows of `store` (row c mod len of a hashed document) as centroids
    int32_t pick_centroids(bertx_mvindex *store, int32_t C, std::vector<float> &cent)
    {
        std::vector<float> doc;
        cent.resize((size_t)C * w);
        for (int32_t c = 0; c < C; ++c) {
            const int32_t d = (int32_t)(((uint64_t)c * 2654435761ull + 777ull) % (uint64_t)n_docs);
            doc.resize((size_t)lens[(size_t)d] * w);
            if (bertx_mvindex_doc(store, d, doc.data()) != 0) return -1;
            std::memcpy(cent.data() + (size_t)c * w, doc.data() + (size_t)(c % lens[(size_t)d]) * w, (size_t)w * 4);
        }
        return 0;
    }
};

// B == 0: the scorer over n_cand candidates; B >= 1: the full-scan search of B queries for
// the k best.  C > 0 (with B >= 1): C hash-chosen stored rows become the centroids and
// avg_us[3] gets the table kernels, the scans with their selections, and the whole pruned
// search of n_cand candidates.  pattern (with B >= 1): the mask of bertx_bench_maxsim_masked.
int32_t bench_store(int32_t w, int32_t n_docs, int32_t doc_len, int32_t Lq, int32_t n_cand, int32_t B, int32_t k,
                    int32_t storage, int32_t iters, float *avg_us, int32_t C = 0, int32_t pattern = 0)
{
    using namespace emb;
    if (pattern < 0 || pattern > 5 || (pattern && B < 1)) return -1;
    if (n_docs < 1 || doc_len < 0 || doc_len > 4096 || n_cand < 1 || iters < 1 || !avg_us || hip_device_count() == 0)
        return -1;
    if (B > 0 && !search_args_ok("bertx_bench_maxsim_search", B, Lq, k)) return -1;
    if (C > 0 && (B < 1 || k > n_cand || n_cand > kMaxK || !centroid_count_ok("bertx_bench_maxsim_pruned", C))) return -1;
    const int32_t nq = std::max(B, 1);
    try {
        MaxsimBench F(w, n_docs, doc_len, n_cand, iters);
        HIP_RC(F.guard.status());
        F.mv = mvindex_create_on(0, w, n_docs, F.slots, storage);
        if (!F.mv || F.init(nq) != 0 || F.fill(F.mv) != 0) return -1;
        if (Lq < 1 || Lq > kMaxLq || F.queries(nq, Lq) != 0) return -1;
        const float *Q = (const float *)F.q.p;
        float *out = (float *)F.out.p;
        int32_t *oid = (int32_t *)F.oid.p;
        // the mask: nf filters of `words` words on the device, or a hashed sixteenth removed
        const int32_t words = (n_docs + 31) / 32, nf = pattern == 2 ? B : pattern >= 1 && pattern <= 4 ? 1 : 0;
        auto sixteenth = [](int32_t i) {
            uint32_t h = (uint32_t)i * 2654435761u + 4242u;
            h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
            return (h & 15u) == 0;
        };
        DevBuf filt;
        if (nf) {
            std::vector<uint32_t> fw((size_t)nf * words, pattern <= 2 ? ~0u : 0u);
            for (int32_t i = 0; i < n_docs; ++i)
                if ((pattern == 3 && sixteenth(i)) || (pattern == 4 && i < n_docs / 16)) fw[(size_t)(i >> 5)] |= 1u << (i & 31);
            HIP_RC(hipMalloc(&filt.p, fw.size() * 4));
            HIP_RC(hipMemcpy(filt.p, fw.data(), fw.size() * 4, hipMemcpyHostToDevice));
        }
        if (pattern == 5) {
            std::vector<int32_t> gone;
            for (int32_t i = 0; i < n_docs; ++i)
                if (sixteenth(i)) gone.push_back(i);
            if (!gone.empty() && bertx_mvindex_remove(F.mv, gone.data(), (int32_t)gone.size()) != 0) return -1;
        }
        const uint32_t *df = (const uint32_t *)filt.p;
        if (C > 0) {
            std::vector<float> cent;
            if (F.pick_centroids(F.mv, C, cent) != 0 || bertx_mvindex_set_centroids(F.mv, cent.data(), C) != 0) return -1;
            HIP_RC(F.mv->ord.wait());
            bertx_mvindex &mv = *F.mv;
            const int32_t per_pass = 4 / ((Lq + 15) / 16);
            const SearchMask sm{mv.tomb, df, nf > 1 ? words : 0};
            auto stage = [&](int st) -> int32_t {
                for (int32_t b0 = 0; b0 < B; b0 += per_pass) {
                    const SearchMask pm = pass_mask(sm, b0);
                    const int32_t rc = launch_maxsim_candidates(
                        mv.codes, mv.table, (int)mv.n_docs, mv.used_slots / 16, mv.storage, mv.w, mv.cent, mv.cent_u, mv.C,
                        Q + (size_t)b0 * Lq * w, std::min(per_pass, B - b0), Lq, n_cand, mv.tscratch, mv.search_scratch,
                        out + (size_t)b0 * n_cand, oid + (size_t)b0 * n_cand, st, nullptr, F.s, 0, nullptr,
                        pattern ? &pm : nullptr);
                    if (rc != 0) return rc;
                }
                return 0;
            };
            if (F.timed([&] { return stage(1); }, avg_us) != 0) return -1;
            if (F.timed([&] { return stage(2); }, avg_us + 1) != 0) return -1;
            return F.timed([&] {
                return bertx_mvindex_search_pruned_filtered_device(F.mv, Q, B, Lq, k, n_cand, df, nf, nf ? words : 0, out, oid,
                                                                   F.s);
            }, avg_us + 2);
        }
        return F.timed([&] {
            if (B > 0) return bertx_mvindex_search_filtered_device(F.mv, Q, B, Lq, k, df, nf, nf ? words : 0, out, oid, F.s);
            return bertx_mvindex_score_device(F.mv, Q, Lq, (const int32_t *)F.id.p, n_cand, out, F.s);
        }, avg_us);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_bench_maxsim: %s\n", ex.what());
        return -1;
    }
}

// bertx_bench_maxsim_res: bench_store's documents (the same lens and fill seeds) twice: in an
// f16 store, whose C hash-chosen rows become the centroids and which trains the buckets, then
// in the residual store.
int32_t bench_res(int32_t w, int32_t n_docs, int32_t doc_len, int32_t C, int32_t Lq, int32_t n_cand, int32_t storage,
                  int32_t iters, float *avg_us)
{
    using namespace emb;
    if (n_docs < 1 || doc_len < 0 || doc_len > 4096 || n_cand < 1 || iters < 1 || !avg_us || Lq < 1 || Lq > kMaxLq ||
        (storage != BERTX_INDEX_RES2 && storage != BERTX_INDEX_RES4) || hip_device_count() == 0 ||
        !centroid_count_ok("bertx_bench_maxsim_res", C))
        return -1;
    try {
        MaxsimBench F(w, n_docs, doc_len, n_cand, iters);
        HIP_RC(F.guard.status());
        if (F.init(1) != 0) return -1;
        F.aux = mvindex_create_on(0, w, n_docs, F.slots, BERTX_INDEX_F16);
        if (!F.aux || F.fill(F.aux) != 0) return -1;
        std::vector<float> cent;
        float cuts[15], wts[16];
        if (F.pick_centroids(F.aux, C, cent) != 0 || bertx_mvindex_set_centroids(F.aux, cent.data(), C) != 0) return -1;
        if (bertx_mvindex_train_residual_buckets(F.aux, storage == BERTX_INDEX_RES2 ? 2 : 4, cuts, wts) != 0) return -1;
        bertx_mvindex_free(F.aux);
        F.aux = nullptr;
        F.mv = mvindex_create_on(0, w, n_docs, F.slots, storage);
        if (!F.mv || bertx_mvindex_set_centroids(F.mv, cent.data(), C) != 0 ||
            bertx_mvindex_set_residual_buckets(F.mv, cuts, wts) != 0 || F.fill(F.mv) != 0)
            return -1;
        if (F.queries(1, Lq) != 0) return -1;
        const float *Q = (const float *)F.q.p;
        float *out = (float *)F.out.p;
        if (F.timed([&] { return bertx_mvindex_score_device(F.mv, Q, Lq, (const int32_t *)F.id.p, n_cand, out, F.s); },
                    avg_us) != 0)
            return -1;
        const int32_t nc = std::min(n_cand, kMaxK), k = std::min(nc, 10);
        return F.timed([&] { return bertx_mvindex_search_pruned_device(F.mv, Q, 1, Lq, k, nc, out, (int32_t *)F.oid.p, F.s); },
                       avg_us + 1);
    } catch (const std::exception &ex) {
        emb::errorf("bertx_bench_maxsim_res: %s\n", ex.what());
        return -1;
    }
}

}  // namespace

extern "C" {

int32_t bertx_bench_maxsim_res(int32_t w, int32_t n_docs, int32_t doc_len, int32_t C, int32_t Lq, int32_t n_cand,
                               int32_t storage, int32_t iters, float *avg_us)
{
    return bench_res(w, n_docs, doc_len, C, Lq, n_cand, storage, iters, avg_us);
}

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

int32_t bertx_bench_maxsim_pruned(int32_t w, int32_t n_docs, int32_t doc_len, int32_t C, int32_t Lq, int32_t B, int32_t k,
                                  int32_t n_cand, int32_t storage, int32_t iters, float *avg_us)
{
    if (B < 1 || C < 1) return -1;
    return bench_store(w, n_docs, doc_len, Lq, n_cand, B, k, storage, iters, avg_us, C);
}

int32_t bertx_bench_maxsim_masked(int32_t w, int32_t n_docs, int32_t doc_len, int32_t C, int32_t Lq, int32_t B, int32_t k,
                                  int32_t n_cand, int32_t storage, int32_t pattern, int32_t iters, float *avg_us)
{
    if (B < 1 || C < 0) return -1;
    return bench_store(w, n_docs, doc_len, Lq, C > 0 ? n_cand : 1, B, k, storage, iters, avg_us, C, pattern);
}

int32_t bertx_bench_maxsim(int32_t w, int32_t n_docs, int32_t doc_len, int32_t Lq, int32_t n_cand, int32_t iters,
                           float *avg_us)
{
    return bertx_bench_maxsim_ex(w, n_docs, doc_len, Lq, n_cand, BERTX_INDEX_F16, iters, avg_us);
}

}  // extern "C"
