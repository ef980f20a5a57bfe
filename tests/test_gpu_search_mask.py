"""Row deletion and filtered search of the embedding index on the GPU (bertx_index_remove,
bertx_index_search_filtered, index_mask.hip and the masked variants of search.hip,
search_bin.hip and search_rescore.hip).  Every comparison is exact equality of ids and of
score bits.  The expected result of a masked call is search_mask_refs.select() over the score
matrix that bertx_index_score_ids gives for all ids (in chunks of 128) before any removal:
the existing contract makes those the search's bits.  One test uses another oracle: a fresh
index that holds the live rows only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import search_mask_refs as M
import search_refs as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

KINDS = ["f16", "int8", "binary"]


@pytest.fixture(scope="module", autouse=True)
def _one_device():
    os.environ.pop("BERT_HOST_ONLY", None)
    os.environ["BERT_DEVICES"] = "0"


_models = {}


@pytest.fixture(scope="module")
def model_of_width(tmp_path_factory):
    """A context whose n_embd is d: tiny64 for 64, else a one-layer synthetic f16 model."""
    def get(d):
        if d not in _models:
            if d == 64:
                path = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
            else:
                path = str(tmp_path_factory.mktemp("maskw%d" % d) / "m.bin")
                hp = dict(n_vocab=256, n_max_tokens=32, n_embd=d, n_intermediate=128, n_head=d // 64, n_layer=1)
                bertpy.synthetic_model(path, hp, "f16")
            _models[d] = bertpy.BertModel(path)
        return _models[d]
    yield get
    _models.clear()


def make(model, kind, capacity):
    if kind == "binary":
        return bertpy.BertBinaryIndex(model, capacity)
    return bertpy.BertIndex(model, capacity, storage=kind)


def filled(model, kind, rows, capacity=None):
    ix = make(model, kind, capacity or max(len(rows), 1))
    assert ix.add(rows) == 0 and len(ix) == len(rows)
    return ix


def score_matrix(ix, queries):
    """S f32 [B][size]: every pair's score from bertx_index_score_ids, 128 ids at a time."""
    B, N = len(queries), len(ix)
    S = np.zeros((B, N), np.float32)
    for i in range(0, N, 128):
        ids = np.arange(i, min(i + 128, N), dtype=np.int32)
        S[:, i:i + len(ids)] = ix.score_ids(queries, np.tile(ids, (B, 1)))
    return S


def filtered(ix, queries, k, words, n_filters=None):
    """bertx_index_search_filtered through the C ABI with packed words of the test's own."""
    q = np.ascontiguousarray(queries, np.float32)
    words = np.ascontiguousarray(words, np.uint32)
    nf = (1 if words.ndim == 1 else words.shape[0]) if n_filters is None else n_filters
    scores, ids = np.zeros((len(q), k), np.float32), np.zeros((len(q), k), np.int32)
    rc = ix.lib.bertx_index_search_filtered(ix.idx, q.ctypes.data, len(q), k, words.ctypes.data, nf, words.shape[-1],
                                            scores.ctypes.data, ids.ctypes.data)
    assert rc == 0
    return scores, ids


# ---- device buffers through the HIP runtime libbert.so is linked against ----
def _hip():
    h = ctypes.CDLL("libamdhip64.so.7")
    vp = ctypes.c_void_p
    h.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    h.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    h.hipFree.argtypes = [vp]
    h.hipStreamCreate.argtypes = [ctypes.POINTER(vp)]
    h.hipStreamSynchronize.argtypes = [vp]
    h.hipStreamDestroy.argtypes = [vp]
    h.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
    h.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
    h.hipGraphInstantiate.argtypes = [ctypes.POINTER(vp), vp, vp, vp, ctypes.c_size_t]
    h.hipGraphLaunch.argtypes = [vp, vp]
    h.hipGraphExecDestroy.argtypes = [vp]
    h.hipGraphDestroy.argtypes = [vp]
    return h


class DeviceArrays:
    def __init__(self):
        self.hip = _hip()
        self.ptrs = []

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), max(nbytes, 16)) == 0
        self.ptrs.append(p)
        return p

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        self.put(p, a)
        return p

    def put(self, p, a):
        a = np.ascontiguousarray(a)
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0

    def down(self, p, shape, dtype):
        out = np.zeros(shape, dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def close(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


@pytest.fixture
def dev():
    d = DeviceArrays()
    yield d
    d.close()


@pytest.fixture
def stream(dev):
    s = ctypes.c_void_p()
    assert dev.hip.hipStreamCreate(ctypes.byref(s)) == 0
    yield s
    dev.hip.hipStreamDestroy(s)


# ---- 1. remove / live / deleted ----
@pytest.mark.parametrize("kind", KINDS)
def test_remove_live_deleted_and_clear(model_of_width, kind):
    d, N, cap, k = 64, 150, 200, 10
    rng = np.random.default_rng(1)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 3, d)
    ix = filled(model_of_width(d), kind, rows, cap)
    assert ix.live() == N and not ix.deleted(0, N).any()
    stored = ix.rows(0, N)
    S = score_matrix(ix, queries)
    gone = [0, 15, 16, 31, 32, 63, 64, 149, 149, -1, 150, 2 ** 31 - 1]
    ix.remove(gone)
    dead = M.tombstones(N, gone)
    assert ix.live() == 142 and len(ix) == N
    assert np.array_equal(ix.deleted(0, N), dead)
    assert np.array_equal(np.flatnonzero(ix.deleted(0, N)), [0, 15, 16, 31, 32, 63, 64, 149])
    assert np.array_equal(ix.deleted(15, 2), [True, True]) and np.array_equal(ix.deleted(148, 2), [False, True])
    assert np.array_equal(ix.rows(0, N).view(np.uint32), stored.view(np.uint32))      # a deleted row's values stay
    assert M.same(ix.search(queries, k), M.select(S, ~dead, k))
    # score_ids: a deleted id as an id outside the index
    ids = np.tile(np.arange(128, dtype=np.int32), (3, 1))
    want = S[:, :128].copy()
    want[:, dead[:128]] = -np.inf
    assert np.array_equal(M.bits(ix.score_ids(queries, ids)), M.bits(want))
    # a bad range: -1, the output untouched
    out = np.full(4, 7, np.uint8)
    for first, n in ((-1, 2), (N - 1, 2), (0, 0), (N, 1)):
        assert ix.lib.bertx_index_deleted(ix.idx, first, n, out.ctypes.data) == -1
    assert np.all(out == 7)
    # clear, then a shorter add: no flag, no stale id, and an all-ones filter wider than needed admits no id >= size
    ix.clear()
    assert len(ix) == 0 and ix.live() == 0
    few = R.unit_rows(rng, 70, d)
    assert ix.add(few) == 0 and ix.live() == 70 and not ix.deleted(0, 70).any()
    S2 = score_matrix(ix, queries)
    got = ix.search(queries, 128)
    assert M.same(got, M.select(S2, np.ones(70, bool), 128)) and got[1].max() == 69
    assert np.array_equal(np.sort(got[1][:, :70], axis=1), np.tile(np.arange(70), (3, 1)))
    ones = np.full(7, 0xFFFFFFFF, np.uint32)                   # 224 bits for 70 rows (capacity 200)
    assert M.same(filtered(ix, queries, 128, ones), got)
    ix.remove([69])
    assert ix.live() == 69
    assert M.same(filtered(ix, queries, 128, ones), M.select(S2, np.arange(70) < 69, 128))


# ---- 2. the grid after a removal ----
@pytest.mark.parametrize("N", [1, 16, 17, 33, 64, 65, 300, 4099])
@pytest.mark.parametrize("d", [64, 192, 768])
def test_grid_after_removal(model_of_width, d, N):
    B, k = 5, 10
    rng = np.random.default_rng(100 * d + N)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    m = model_of_width(d)
    for kind in KINDS:
        ix = filled(m, kind, rows)
        S = score_matrix(ix, queries)
        assert M.same(ix.search(queries, k), M.select(S, np.ones(N, bool), k)), kind
        for name, gone in M.removal_patterns(N, rng).items():
            ix.clear()
            assert ix.add(rows) == 0
            ix.remove(gone)
            dead = M.tombstones(N, gone)
            assert ix.live() == N - dead.sum(), (kind, name)
            got = ix.search(queries, k)
            assert M.same(got, M.select(S, ~dead, k)), (kind, name)
            if name == "every row":
                assert np.all(got[1] == -1) and np.all(np.isneginf(got[0]))


@pytest.mark.parametrize("kind", KINDS)
def test_deletions_equal_a_fresh_index_of_the_live_rows(model_of_width, kind):
    """The oracle that does not use score_ids: scores do not depend on id or row count."""
    d, N, B, k = 192, 300, 5, 10
    rng = np.random.default_rng(7)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    m = model_of_width(d)
    ix = filled(m, kind, rows)
    live = rng.random(N) < 0.6
    live[[0, N - 1]] = [False, True]
    ix.remove(np.flatnonzero(~live))
    fs, fi = filled(m, kind, rows[live]).search(queries, k)
    got = ix.search(queries, k)
    assert np.array_equal(M.bits(got[0]), M.bits(fs))
    assert np.array_equal(got[1], np.flatnonzero(live)[fi].astype(np.int32))


# ---- 3. filters ----
@pytest.mark.parametrize("kind", KINDS)
def test_filters(model_of_width, kind):
    d, N, k = 192, 4099, 10
    rng = np.random.default_rng(11)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 261, d)
    ix = filled(model_of_width(d), kind, rows)
    S = score_matrix(ix, queries)
    plain = ix.search(queries, k)
    for B in (65, 261):                                        # across a 64-query group; across the 256-query stage
        q = queries[:B]
        shared = rng.random(N) < 0.3
        each = rng.random((B, N)) < 0.3
        # the Python interface, both shapes of allow=
        assert M.same(ix.search(q, k, allow=shared), M.select(S[:B], shared, k)), B
        assert M.same(ix.search(q, k, allow=each), M.select(S[:B], each, k)), B
        # all ones, shared and per query: the unfiltered search bit for bit
        assert M.same(ix.search(q, k, allow=np.ones(N, bool)), (plain[0][:B], plain[1][:B]))
        assert M.same(ix.search(q, k, allow=np.ones((B, N), bool)), (plain[0][:B], plain[1][:B]))
        # words beyond the needed ones, and garbage in the bits of rows >= size
        wide = M.pack_bits(each, words=M.words_for(N) + 3)
        wide[:, M.words_for(N):] = 0xFFFFFFFF
        wide[:, M.words_for(N) - 1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
        got = filtered(ix, q, k, wide)
        assert M.same(got, M.select(S[:B], each, k)) and got[1].max() < N
    # k 128 with 100 admissible rows: the fill
    B = 65
    q = queries[:B]
    hundred = np.zeros(N, bool)
    hundred[rng.permutation(N)[:100]] = True
    hundred_each = np.zeros((B, N), bool)
    for b in range(B):
        hundred_each[b, rng.permutation(N)[:100]] = True
    for allow in (hundred, hundred_each):
        s, i = ix.search(q, 128, allow=allow)
        assert M.same((s, i), M.select(S[:B], allow, 128))
        assert np.all(i[:, :100] >= 0) and np.all(i[:, 100:] == -1) and np.all(np.isneginf(s[:, 100:]))
    # per-query filters that admit disjoint sets return disjoint ids
    part = np.zeros((B, N), bool)
    part[np.arange(N) % B, np.arange(N)] = True
    s, i = ix.search(q, k, allow=part)
    assert M.same((s, i), M.select(S[:B], part, k))
    assert np.array_equal(i % B, np.tile(np.arange(B)[:, None], (1, k))) and len(np.unique(i)) == B * k
    # a filter and tombstones together
    gone = np.concatenate([plain[1][:B, 0], np.arange(4032, 4099)])      # every best row, and the end of the index
    ix.remove(gone)
    dead = M.tombstones(N, gone)
    assert M.same(ix.search(q, k), M.select(S[:B], ~dead, k))
    assert M.same(ix.search(q, k, allow=shared), M.select(S[:B], M.admissible(N, B, dead, shared), k))
    assert M.same(ix.search(q, k, allow=each[:B]), M.select(S[:B], M.admissible(N, B, dead, each[:B]), k))
    assert M.same(ix.search(q, 128, allow=hundred_each), M.select(S[:B], M.admissible(N, B, dead, hundred_each), 128))


# ---- 4. many steps per workgroup ----
@pytest.mark.parametrize("kind,N", [("f16", 66000), ("int8", 66000), ("binary", 300000)])
def test_masks_where_a_workgroup_walks_many_groups(model_of_width, dev, kind, N):
    d, B, k = 64, 3, 10
    rows, queries, planted = R.planted(d, N, B, k)
    ix = make(model_of_width(d), kind, N)
    assert ix.lib.bertx_index_add_device(ix.idx, dev.up(rows), N, None) == 0 and len(ix) == N
    s128, i128 = ix.search(queries, 128)                       # before any removal
    if kind == "f16":
        assert np.array_equal(i128[:, :k], planted)
    # delete every query's five best rows: the next best come up, with the bits they had
    gone = i128[:, :5].ravel()
    ix.remove(gone)
    assert ix.live() == N - len(set(gone.tolist()))
    want_s, want_i = np.zeros((B, k), np.float32), np.zeros((B, k), np.int32)
    for b in range(B):
        keep = ~np.isin(i128[b], gone)
        assert keep.sum() >= k
        want_s[b], want_i[b] = s128[b][keep][:k], i128[b][keep][:k]
    assert M.same(ix.search(queries, k), (want_s, want_i))
    # a filter that admits one row in each of five far-apart groups (one of them deleted)
    picks = np.array([5, N // 4 + 17, N // 2 + 33, 3 * N // 4 + 63, N - 1], np.int64)
    ix.remove([int(picks[2])])
    allow = np.zeros(N, bool)
    allow[picks] = True
    left = np.delete(picks, 2)
    sc = ix.score_ids(queries, np.tile(left.astype(np.int32), (B, 1)))
    want = M.select(sc, np.ones(4, bool), k)
    want = (want[0], np.where(want[1] >= 0, left[np.clip(want[1], 0, 3)], -1).astype(np.int32))
    got = ix.search(queries, k, allow=allow)
    assert M.same(got, want) and np.all(got[1][:, 4:] == -1)
    per = np.zeros((B, N), bool)
    per[np.arange(B), picks[[0, 3, 4]]] = True
    got = ix.search(queries, k, allow=per)
    assert np.array_equal(got[1][:, 0], picks[[0, 3, 4]]) and np.all(got[1][:, 1:] == -1)
    assert np.array_equal(M.bits(got[0][:, 0]), M.bits(sc[np.arange(B), [0, 2, 3]]))


# ---- 5. the two-stage search ----
@pytest.mark.parametrize("fine_kind", ["f16", "int8"])
def test_search_rescored_filtered_is_the_composition(model_of_width, fine_kind):
    d, N, B, k, n_cand = 192, 300, 5, 10, 40
    rng = np.random.default_rng(21)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    m = model_of_width(d)
    coarse, fine = filled(m, "binary", rows), filled(m, fine_kind, rows)
    S_fine = score_matrix(fine, queries)

    def composition(allow, fine_dead):
        _, cand = coarse.search(queries, n_cand, allow=allow)
        s = fine.score_ids(queries, cand)
        out_s, out_i = np.full((B, k), -np.inf, np.float32), np.full((B, k), -1, np.int32)
        for b in range(B):
            keep = (cand[b] >= 0) & ~fine_dead[np.clip(cand[b], 0, N - 1)]
            assert np.all(np.isneginf(s[b][~keep]))                       # what fine does not hold scores -inf
            assert np.array_equal(M.bits(s[b][keep]), M.bits(S_fine[b, cand[b][keep]]))
            o = np.lexsort((cand[b][keep], -s[b][keep].astype(np.float64)))[:k]
            out_s[b, :len(o)], out_i[b, :len(o)] = s[b][keep][o], cand[b][keep][o]
        return out_s, out_i

    none = np.zeros(N, bool)
    shared = rng.random(N) < 0.5
    each = rng.random((B, N)) < 0.5
    for allow in (None, shared, each):
        assert M.same(coarse.search_rescored(queries, k, fine, n_cand, allow=allow), composition(allow, none))
    coarse.remove(np.flatnonzero(shared)[:30])                 # the coarse index's tombstones limit the candidates
    for allow in (None, shared, each):
        got = coarse.search_rescored(queries, k, fine, n_cand, allow=allow)
        assert M.same(got, composition(allow, none))
        assert not np.isin(got[1], np.flatnonzero(shared)[:30]).any()
    # twenty admitted rows, fifteen of them deleted in the fine index only: five results and the fill
    twenty = np.zeros(N, bool)
    twenty[200:220] = True
    fine.remove(np.arange(205, 220))
    fine_dead = M.tombstones(N, np.arange(205, 220))
    got = coarse.search_rescored(queries, k, fine, n_cand, allow=twenty)
    assert M.same(got, composition(twenty, fine_dead))
    assert np.array_equal(np.sort(got[1][:, :5], axis=1), np.tile(np.arange(200, 205), (B, 1)))
    assert np.all(got[1][:, 5:] == -1) and np.all(np.isneginf(got[0][:, 5:]))


# ---- 6. the device forms ----
@pytest.mark.parametrize("kind", KINDS)
def test_remove_and_filtered_search_in_one_graph(model_of_width, dev, stream, kind):
    d, N, B, k = 768, 1025, 17, 10
    rng = np.random.default_rng(31)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    ix = filled(model_of_width(d), kind, rows)
    S = score_matrix(ix, queries)
    gone = np.array([0, 16, 1024, 500, 500, -3, N], np.int32)
    dead = M.tombstones(N, gone)
    f1, f2 = rng.random((B, N)) < 0.5, rng.random((B, N)) < 0.2
    words = M.words_for(N)
    dq, dg, df = dev.up(queries), dev.up(gone), dev.up(M.pack_bits(f1))
    ds, di = dev.alloc(B * k * 4), dev.alloc(B * k * 4)
    hip, vp = dev.hip, ctypes.c_void_p
    graph, ex = vp(), vp()
    assert hip.hipStreamBeginCapture(stream, 1) == 0           # thread-local mode
    rc1 = ix.lib.bertx_index_remove_device(ix.idx, dg, len(gone), stream)
    rc2 = ix.lib.bertx_index_search_filtered_device(ix.idx, dq, B, k, df, B, words, ds, di, stream)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0 and rc1 == 0 and rc2 == 0
    assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, 0) == 0
    assert not ix.deleted(0, N).any()                          # captured, not run
    for f in (f1, f2):
        dev.put(df, M.pack_bits(f))                            # the filter buffer overwritten in place
        dev.put(ds, np.full((B, k), 3, np.float32))
        dev.put(di, np.full((B, k), 3, np.int32))
        assert hip.hipGraphLaunch(ex, stream) == 0 and hip.hipStreamSynchronize(stream) == 0
        got = (dev.down(ds, (B, k), np.float32), dev.down(di, (B, k), np.int32))
        assert M.same(got, M.select(S, M.admissible(N, B, dead, f), k))
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    assert np.array_equal(ix.deleted(0, N), dead) and ix.live() == N - 4
    # outside a graph, a shared filter on the stream
    dev.put(df, M.pack_bits(f1[0]))
    assert ix.lib.bertx_index_search_filtered_device(ix.idx, dq, B, k, df, 1, words, ds, di, stream) == 0
    assert hip.hipStreamSynchronize(stream) == 0
    got = (dev.down(ds, (B, k), np.float32), dev.down(di, (B, k), np.int32))
    assert M.same(got, M.select(S, M.admissible(N, B, dead, f1[0]), k))


# ---- 7. refusals ----
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_the_outputs_untouched(model_of_width, kind):
    d, N, B, k = 64, 100, 3, 5
    rng = np.random.default_rng(41)
    rows, q = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    m = model_of_width(d)
    ix, other = filled(m, kind, rows), filled(m, "f16" if kind == "binary" else "binary", rows)
    lib = ix.lib
    scores, ids = np.full((B, 129), 7.0, np.float32), np.full((B, 129), 7, np.int32)
    words = M.words_for(N)
    f = np.full((B, words), 0xFFFFFFFF, np.uint32)
    Q, F, S, I = q.ctypes.data, f.ctypes.data, scores.ctypes.data, ids.ctypes.data

    def call(queries=Q, B_=B, k_=k, filters=F, nf=B, w=words, s=S, i=I):
        return lib.bertx_index_search_filtered(ix.idx, queries, B_, k_, filters, nf, w, s, i)

    def call2(queries=Q, k_=k, n_cand=20, filters=F, nf=B, w=words, s=S, i=I):
        return lib.bertx_index_search_rescored_filtered(other.idx, ix.idx, queries, B, k_, n_cand, filters, nf, w, s, i)

    for c in (call, call2):
        assert c(queries=None) < 0 and c(s=None) < 0 and c(i=None) < 0
        assert c(filters=None) < 0                             # a count without a pointer
        assert c(nf=0) < 0                                     # a pointer without a count
        assert c(nf=2) < 0 and c(nf=B + 1) < 0 and c(nf=-1) < 0
        assert c(w=words - 1) < 0 and c(w=0) < 0
        assert c(k_=129) < 0 and c(k_=0) < 0
    assert call(B_=0) < 0
    assert lib.bertx_index_search_filtered(None, Q, B, k, F, B, words, S, I) < 0
    assert np.all(scores == 7.0) and np.all(ids == 7)
    # remove: n 0, null ids, a null index: negative, nothing changed
    g = np.array([1, 2], np.int32)
    assert lib.bertx_index_remove(ix.idx, g.ctypes.data, 0) < 0 and lib.bertx_index_remove(ix.idx, None, 2) < 0
    assert lib.bertx_index_remove(None, g.ctypes.data, 2) < 0 and lib.bertx_index_remove_device(ix.idx, None, 2, None) < 0
    assert lib.bertx_index_remove_device(ix.idx, g.ctypes.data, 0, None) < 0
    assert ix.live() == N and not ix.deleted(0, N).any()
    assert lib.bertx_index_live(None) < 0
    with pytest.raises(ValueError):
        ix.search(q, k, allow=np.ones(N + 1, bool))
    # the accepted forms next to them: (NULL, 0) is the plain search
    assert call(filters=None, nf=0, w=0) == 0
    plain = ix.search(q, k)
    assert M.same((scores.reshape(-1)[:B * k].reshape(B, k), ids.reshape(-1)[:B * k].reshape(B, k)), plain)
    assert call(nf=1) == 0 and call() == 0 and call2() == 0


# ---- 8. the tool ----
def test_the_tool_deletes_rows(tmp_path):
    path = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
    texts = ["the cat sat on the mat", "a dog ran in the park", "rain fell on the town"]
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(texts) + "\n")
    tool = [os.path.join(ROOT, "build", "bin", "search"), "-m", path, "-f", str(corpus), "-k", "3"]
    m = bertpy.BertModel(path)
    ix = bertpy.BertIndex(m, 3)
    assert ix.add_texts(texts) == 0
    query = texts[1]
    before = ix.search_texts([query], 3)
    ix.remove([1, 7])
    after = ix.search_texts([query], 3)
    assert before[1][0, 0] == 1 and 1 not in after[1] and after[1][0, 2] == -1
    stdin = "%s\n:del 1 7\n%s\n:del 1\n:del 0 2\n%s\nq\n" % (query, query, query)

    def run(args):
        r = subprocess.run(tool + args, input=stdin, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        # (the loader's own lines share stdout: the hits and the answers to :del are kept)
        return [ln for ln in r.stdout.splitlines()
                if "deleted" in ln or (len(ln.split("\t")) == 4 and ln.split("\t")[0].isdigit())]

    def hit_lines(scores, ids):
        return ["%d\t%d\t%.4f\t%s" % (j + 1, i, s, texts[i]) for j, (s, i) in enumerate(zip(scores, ids)) if i >= 0]

    want = hit_lines(before[0][0], before[1][0]) + ["deleted 1"] + hit_lines(after[0][0], after[1][0]) + \
        ["deleted 0", "deleted 2"]
    assert run([]) == want
    for args in (["-s", "int8"], ["-s", "binary"], ["-s", "binary", "-R", "f16"]):
        out = run(args)
        assert [ln for ln in out if ln.startswith("deleted")] == ["deleted 1", "deleted 0", "deleted 2"]
        at = out.index("deleted 1")
        assert at == 3 and len(out) == 3 + 1 + 2 + 2
        assert all(ln.split("\t")[1] != "1" for ln in out[at + 1:at + 3])
    out = run(["-l", "-a"])                                    # no embedding index: answered and ignored
    assert len([ln for ln in out if "nothing deleted" in ln]) == 3 and not any(ln.startswith("deleted") for ln in out)
    assert len([ln for ln in out if ln.split("\t")[0].isdigit()]) == 9
