"""Residual-coded token stores on the GPU (BERTX_INDEX_RES2 / _RES4, maxsim_res.hip) against
the numpy restatement (maxsim_res_refs.py).  The reference of a residual store is its twin,
an f16 store of the same width with the same centroids: codes, bits and u are restated from
the twin's _doc, _doc_codes and _centroid bit for bit; scores are held to the float64 MaxSim
of the reproducible operands (q16, e, u) within the contract's bound; everything else is on
bits."""
import ctypes
import os

import numpy as np
import pytest

import bertpy
import maxsim_pruned_refs as PR
import maxsim_refs as M
import maxsim_res_refs as RR
from conftest import GOLDEN
from test_gpu_maxsim_i8 import DeviceArrays, same, slots_of, store_of
from test_gpu_maxsim_search import COLBERT_TEXTS, colbert_model, corpus_texts, corpus_words, tool_lines  # noqa: F401

pytestmark = pytest.mark.gpu

TINY64 = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
KINDS = ("res2", "res4")


@pytest.fixture(scope="module", autouse=True)
def _one_device():
    os.environ.pop("BERT_HOST_ONLY", None)
    os.environ["BERT_DEVICES"] = "0"


@pytest.fixture(scope="module")
def model():
    return bertpy.BertModel(TINY64)


@pytest.fixture
def dev():
    d = DeviceArrays()
    yield d
    d.close()


def make_centroids(w, C):
    return M.unit_rows(np.random.default_rng(77 * w + C), C, w)


def near_centroids(rng, cent, n, sigma=0.4):
    """n un-normalised rows: a random centroid plus noise of norm about sigma, at a random scale."""
    w = cent.shape[1]
    x = cent[rng.integers(0, len(cent), n)] + (sigma / np.sqrt(w)) * rng.standard_normal((n, w))
    return (x * rng.choice([1e-3, 1.0, 30.0], n)[:, None]).astype(np.float32)


def make_docs(w, C, lens, seed):
    rng = np.random.default_rng(seed)
    cent = make_centroids(w, C)
    return [near_centroids(rng, cent, n) for n in lens]


def twin_of(model, docs, w, cent, extra_docs=0, extra_slots=0):
    t = store_of(model, docs, w, storage="f16", extra_docs=extra_docs, extra_slots=extra_slots)
    t.set_centroids(cent)
    return t


def empty_res(model, w, kind, cent, buckets, n_docs, slots):
    ix = bertpy.BertTokenIndex(model, n_docs, slots, width=w, storage=kind)
    ix.set_centroids(cent)
    ix.set_residual_buckets(*buckets)
    return ix


def res_of(model, docs, w, kind, cent, buckets, extra_docs=0, extra_slots=0):
    ix = empty_res(model, w, kind, cent, buckets, len(docs) + extra_docs, slots_of(docs) + extra_slots)
    assert ix.add(docs) == 0 and len(ix) == len(docs) and ix.token_slots == slots_of(docs)
    return ix


def restate(twin, i, buckets):
    """(codes, b, e float16, u) of document i from the twin's read-back values."""
    codes = twin.doc_codes(i)
    cent = np.stack([twin.centroid(int(c)) for c in codes])
    b, e, u = RR.encode(twin.doc(i), cent, *buckets)
    return codes, b, e, u


def assert_state(ix, twin, buckets, ids=None):
    nb = RR.NBITS[ix.storage]
    for i in (range(len(ix)) if ids is None else ids):
        codes, b, e, u = restate(twin, i, buckets)
        gc, gb, gu = ix.doc_residual(i)
        assert gc.dtype == np.uint16 and np.array_equal(gc, codes), i
        assert np.array_equal(gb, RR.pack_bits(b, nb)), i
        assert same(gu, u), i
        assert same(ix.doc(i), e.astype(np.float32) * u[:, None]), i


def f16_of(model, q):
    """The query's f16 values: it is added to an f16 store as a document, one normaliser serves both."""
    return store_of(model, [q], q.shape[1], storage="f16").doc(0)


# the parity stores: per (w, kind, C) the twin, the residual store, the buckets and the float64
# references of every document's (e, u); built once, never changed
_parity = {}


@pytest.fixture(scope="module")
def parity(model):
    def get(w, kind, C):
        key = (w, kind, C)
        if key not in _parity:
            cent = make_centroids(w, C)
            docs = make_docs(w, C, M.DOC_LENS, 2000 + w + C)
            docs[2] = docs[2].copy()
            docs[2][7] = 0.0                                               # a row stored as zeros
            twin = twin_of(model, docs, w, cent)
            buckets = twin.train_residual_buckets(RR.NBITS[kind])
            ix = res_of(model, docs, w, kind, cent, buckets)
            decoded = [restate(twin, i, buckets)[2:] for i in range(len(docs))]
            _parity[key] = (ix, twin, buckets, decoded, cent)
        return _parity[key]
    yield get
    _parity.clear()


# ---- 1. the stored state ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", RR.CENTROID_COUNTS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_stored_state_bit_for_bit(model, w, C, kind):
    cent = make_centroids(w, C)
    docs = make_docs(w, C, M.PACK_LENS, 1000 + w + C)
    docs[2] = docs[2].copy()
    docs[2][7] = 0.0
    twin = twin_of(model, docs, w, cent)
    buckets = twin.train_residual_buckets(RR.NBITS[kind])
    ix = res_of(model, docs, w, kind, cent, buckets, extra_docs=len(docs), extra_slots=slots_of(docs))
    assert model.lib.bertx_mvindex_storage(ix.mv) == bertpy.BertTokenIndex.STORAGE[kind]
    assert ix.n_centroids == C
    for c in (0, C - 1):                                                   # the centroids are the f16 packer's bits
        assert same(ix.centroid(c), twin.centroid(c))
    assert_state(ix, twin, buckets)
    assert all(np.array_equal(ix.doc_codes(i), twin.doc_codes(i)) for i in range(len(docs)))
    used = np.concatenate([RR.unpack_bits(ix.doc_residual(i)[1], RR.NBITS[kind]).ravel() for i in range(len(docs))])
    assert set(used.tolist()) == set(range(1 << RR.NBITS[kind]))            # every bucket occurs
    for j, d in enumerate(docs):                                           # one call per document: the same bits
        assert ix.add([d]) == len(docs) + j
    for j in range(len(docs)):
        for a, b in zip(ix.doc_residual(j), ix.doc_residual(len(docs) + j)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), j
    q = np.zeros(4, np.int8)
    assert model.lib.bertx_mvindex_doc_i8(ix.mv, 0, q.ctypes.data, q.ctypes.data) == -1 and np.all(q == 0)


# ---- 2. scores ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", RR.CENTROID_COUNTS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_scores_within_the_bound(model, parity, w, C, kind):
    ix, twin, buckets, decoded, cent = parity(w, kind, C)
    rng = np.random.default_rng(50 + w)
    for Lq in M.QUERY_LENS:
        q = near_centroids(rng, cent, Lq)
        q16 = f16_of(model, q)
        got = ix.score(q)
        tol = RR.score_tol(Lq, w)
        for i, (e, u) in enumerate(decoded):
            ref = RR.maxsim(q16, e, u)
            assert abs(float(got[i]) - ref) <= tol, (Lq, i, float(got[i]), ref, tol)
        assert same(ix.score(q, np.arange(len(ix), dtype=np.int32)), got)   # ids = NULL: the same


# ---- 3. planted rows ----
def planted_store(model, w, kind, doc, q):
    """A residual store (and its twin) of one document whose centroids include the query's
    direction, so that the planted row decodes to nearly the query."""
    cent = make_centroids(w, 16)
    cent[3] = q[0] / np.linalg.norm(q[0])
    twin = twin_of(model, [doc], w, cent)
    buckets = twin.train_residual_buckets(RR.NBITS[kind])
    return res_of(model, [doc], w, kind, cent, buckets), twin, buckets


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", (64, 768))
def test_planted_row_in_every_position(model, w, kind):
    # The other rows lie near centroids other than the query's and have their component along
    # the query removed: their decoded similarity is the quantization error alone (below 0.5),
    # the planted row decodes to its centroid plus one bucket weight per element (above 0.9).
    n = 37
    rng = np.random.default_rng(3000 + w)
    q = M.unit_rows(rng, 1, w)
    others = near_centroids(rng, np.delete(make_centroids(w, 16), 3, axis=0), n, sigma=0.3)
    others = (others - (others @ q[0])[:, None] * q[0][None, :]).astype(np.float32)
    q16 = f16_of(model, q)
    tol = RR.score_tol(1, w)
    for p in (0, 14, 15, 16, 17, 31, 32, n - 1):                           # rows 15 and 16, and the last valid row
        doc = others.copy()
        doc[p] = q[0]
        ix, twin, buckets = planted_store(model, w, kind, doc, q)
        _, _, e, u = restate(twin, 0, buckets)
        sims = (q16.astype(np.float64) @ e.astype(np.float64).T)[0] * u
        assert int(sims.argmax()) == p and sims[p] > 0.9 and np.delete(sims, p).max() < 0.5
        got = float(ix.score(q)[0])
        assert abs(got - sims[p]) <= tol, (p, got, sims[p])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Lq", (1, 17))
def test_all_negative_similarities(model, kind, Lq):
    """Every similarity is about -1: padding rows counted as 0 would give 0, not about -Lq."""
    w = 192
    q, doc = M.planted_negative(w, Lq)
    ix, twin, buckets = planted_store(model, w, kind, doc, -q)
    _, _, e, u = restate(twin, 0, buckets)
    ref = RR.maxsim(f16_of(model, q), e, u)
    got = float(ix.score(q)[0])
    assert ref < -0.9 * Lq and abs(got - ref) <= RR.score_tol(Lq, w), (got, ref)


# ---- 4. stale padding ----
@pytest.mark.parametrize("kind", KINDS)
def test_stale_slots_behind_shorter_documents(model, kind):
    w, C = 192, 16
    cent = make_centroids(w, C)
    long_docs = make_docs(w, C, (100, 33, 32), 61)
    short_docs = make_docs(w, C, (1, 15, 17, 3, 16), 62)
    twin = twin_of(model, short_docs, w, cent)
    buckets = twin.train_residual_buckets(RR.NBITS[kind])
    ix = res_of(model, long_docs, w, kind, cent, buckets, extra_docs=8)
    ix.clear()
    assert len(ix) == 0 and ix.n_centroids == C                            # clear keeps centroids and buckets
    assert ix.add(short_docs) == 0
    fresh = res_of(model, short_docs, w, kind, cent, buckets)
    assert_state(ix, twin, buckets)
    q = near_centroids(np.random.default_rng(63), cent, 17)
    assert same(ix.score(q), fresh.score(q))


# ---- 5. invariance ----
@pytest.mark.parametrize("kind", KINDS)
def test_score_is_invariant_bit_for_bit(model, parity, kind):
    w, C = 192, 48
    ix, twin, buckets, decoded, cent = parity(w, kind, C)
    docs = make_docs(w, C, M.DOC_LENS, 2000 + w + C)
    docs[2] = docs[2].copy()
    docs[2][7] = 0.0
    q = near_centroids(np.random.default_rng(70), cent, 17)
    base = ix.score(q)
    order = [5, 0, 8, 3, 2, 7, 1, 6, 4]                                    # other ids, other neighbours
    other = res_of(model, [docs[i] for i in order] + make_docs(w, C, (40, 2), 71), w, kind, cent, buckets)
    assert same(other.score(q)[:len(order)], base[order])
    ids = np.array([4, -1, 4, 8, 99, 0, 2 ** 31 - 1, -2 ** 31, 4], np.int32)   # a list, its order, repeats, bad ids
    got = ix.score(q, ids)
    good = (ids >= 0) & (ids < len(ix))
    assert same(got[good], base[ids[good]]) and np.all(np.isneginf(got[~good]))
    assert same(ix.score(q, ids[::-1]), got[::-1])
    assert same(ix.score(q), base)                                         # and nothing was disturbed


# ---- 6. candidates and the pruned search ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", (64, 192))
def test_candidates_equal_the_twins(model, parity, w, kind):
    ix, twin, buckets, decoded, cent = parity(w, kind, 48)
    for Lq, B, n_cand in ((1, 5, 4), (17, 3, 9), (64, 2, 128)):
        rng = np.random.default_rng(80 + Lq)
        qs = [near_centroids(rng, cent, Lq) for _ in range(B)]
        want_s, want_i = twin.candidates(qs, n_cand)
        got_s, got_i = ix.candidates(qs, n_cand)
        assert np.array_equal(got_i, want_i) and same(got_s, want_s)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", (64, 768))
def test_pruned_search(model, parity, w, kind):
    ix, twin, buckets, decoded, cent = parity(w, kind, 16)
    n = len(ix)
    for Lq, B, k, n_cand in ((17, 3, 4, 6), (64, 2, 1, 1), (1, 5, 12, 128), (16, 9, 9, 9)):
        rng = np.random.default_rng(90 + Lq)
        qs = [near_centroids(rng, cent, Lq) for _ in range(B)]
        got_s, got_i = ix.search_pruned(qs, k, n_cand)
        cs, ci = ix.candidates(qs, n_cand)
        for b, q in enumerate(qs):
            exact = ix.score(q, ci[b])                                     # the scorer's bits
            want_s, want_i = PR.compose(exact, ci[b], k)
            assert np.array_equal(got_i[b], want_i) and same(got_s[b], want_s)
            if n_cand >= n:                                                # every document, ranked by (score, id)
                full = ix.score(q)
                order = np.lexsort((np.arange(n), -full.astype(np.float64)))[:k]
                m = min(k, n)
                assert np.array_equal(got_i[b, :m], order[:m]) and same(got_s[b, :m], full[order[:m]])
                assert np.all(got_i[b, m:] == -1) and np.all(np.isneginf(got_s[b, m:]))


# ---- 7. the device form, captured ----
@pytest.mark.parametrize("kind", KINDS)
def test_score_device_captured_graph(model, parity, dev, kind):
    w, Lq = 192, 33
    ix, twin, buckets, decoded, cent = parity(w, kind, 16)
    q = near_centroids(np.random.default_rng(95), cent, Lq)
    ids = np.array([3, 8, -1, 0, 8, 42], np.int32)
    want = ix.score(q, ids)
    hip, vp, lib = dev.hip, ctypes.c_void_p, model.lib
    s = vp()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    dq, di, do = dev.up(q), dev.up(ids), dev.alloc(len(ids) * 4)
    assert lib.bertx_mvindex_score_device(ix.mv, dq, Lq, di, len(ids), do, s) == 0
    assert hip.hipStreamSynchronize(s) == 0 and same(dev.down(do, len(ids), np.float32), want)
    graph, ex = vp(), vp()
    assert hip.hipStreamBeginCapture(s, 1) == 0   # thread-local mode
    rc = lib.bertx_mvindex_score_device(ix.mv, dq, Lq, di, len(ids), do, s)
    assert hip.hipStreamEndCapture(s, ctypes.byref(graph)) == 0 and rc == 0
    assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, 0) == 0
    zeros = np.zeros(len(ids) * 4, np.uint8)
    assert hip.hipMemcpy(do, zeros.ctypes.data, zeros.nbytes, 1) == 0
    assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
    assert same(dev.down(do, len(ids), np.float32), want)
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    hip.hipStreamDestroy(s)


# ---- 8. the trainer ----
@pytest.mark.parametrize("nb", (2, 4))
def test_trainer_is_the_quantile_rule(model, nb):
    w, C = 64, 16
    cent = make_centroids(w, C)
    docs = make_docs(w, C, (1, 15, 16, 17, 33, 100), 110)
    twin = twin_of(model, docs, w, cent)
    rows = np.concatenate([twin.doc(i) for i in range(len(docs))])
    codes = np.concatenate([twin.doc_codes(i) for i in range(len(docs))])
    cents = np.stack([twin.centroid(c) for c in range(C)])
    want_c, want_w = RR.train_buckets(rows, codes, cents, nb)
    got_c, got_w = twin.train_residual_buckets(nb)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_w, want_w)
    assert np.all(np.diff(got_c) >= 0) and got_w[0] <= got_c[0] <= got_w[1]
    again = twin.train_residual_buckets(nb)
    assert same(again[0], got_c) and same(again[1], got_w)


def test_trainer_stride(model):
    """70,000 rows: every second row from row 0."""
    w, C = 64, 16
    cent = make_centroids(w, C)
    docs = make_docs(w, C, (1000,) * 70, 111)
    twin = twin_of(model, docs, w, cent)
    rows = np.concatenate([twin.doc(i) for i in range(len(docs))])
    codes = np.concatenate([twin.doc_codes(i) for i in range(len(docs))])
    cents = np.stack([twin.centroid(c) for c in range(C)])
    assert len(rows) == 70000 and RR.sample_stride(len(rows)) == 2
    want_c, want_w = RR.train_buckets(rows, codes, cents, 4)
    got_c, got_w = twin.train_residual_buckets(4)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_w, want_w)


# ---- 9. refusals ----
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_everything_alone(model, dev, kind):
    w, C, nb = 64, 16, RR.NBITS[kind]
    L = model.lib
    cent = make_centroids(w, C)
    docs = make_docs(w, C, (5, 17), 120)
    twin = twin_of(model, docs, w, cent)
    i8 = store_of(model, docs, w, storage="int8")
    cut, wts = twin.train_residual_buckets(nb)
    # the buckets: not on f16 or int8 stores, not with bad values
    assert L.bertx_mvindex_set_residual_buckets(twin.mv, cut.ctypes.data, wts.ctypes.data) == -1
    assert L.bertx_mvindex_set_residual_buckets(i8.mv, cut.ctypes.data, wts.ctypes.data) == -1
    ix = bertpy.BertTokenIndex(model, 8, 256, width=w, storage=kind)
    rows = np.ascontiguousarray(np.concatenate(docs))
    lens = np.array([len(d) for d in docs], np.int32)

    def add():
        return L.bertx_mvindex_add(ix.mv, rows.ctypes.data, lens.ctypes.data, len(docs))

    assert add() == -1                                                     # no centroids, no buckets
    ix.set_residual_buckets(cut, wts)
    assert add() == -1 and len(ix) == 0                                    # no centroids
    other = bertpy.BertTokenIndex(model, 8, 256, width=w, storage=kind)
    other.set_centroids(cent)
    assert L.bertx_mvindex_add(other.mv, rows.ctypes.data, lens.ctypes.data, len(docs)) == -1 and len(other) == 0   # no buckets
    assert cut[0] < cut[-1]
    for bad_c, bad_w in ((cut[::-1].copy(), wts), (np.where(np.arange(len(cut)) == 0, np.nan, cut).astype(np.float32), wts),
                         (cut, np.where(np.arange(len(wts)) == 1, np.inf, wts).astype(np.float32))):
        assert L.bertx_mvindex_set_residual_buckets(other.mv, bad_c.ctypes.data, bad_w.ctypes.data) == -1
    assert L.bertx_mvindex_add(other.mv, rows.ctypes.data, lens.ctypes.data, len(docs)) == -1   # still none
    assert L.bertx_mvindex_add_device(other.mv, dev.up(rows), lens.ctypes.data, len(docs), None) == -1
    assert L.bertx_mvindex_add_texts(other.mv, model.ctx, 1, 1, bertpy.BertIndex._texts(["stone bridge"])) == -1
    assert len(other) == 0 and other.token_slots == 0
    assert L.bertx_mvindex_train_centroids(ix.mv, C, 1, 0) == -1           # no rows to train from
    ix.set_centroids(cent)
    assert add() == 0 and len(ix) == 2
    before = [ix.doc_residual(i) for i in range(2)]
    assert L.bertx_mvindex_set_residual_buckets(ix.mv, cut.ctypes.data, wts.ctypes.data) == -1   # documents are stored
    assert L.bertx_mvindex_set_centroids(ix.mv, cent.ctypes.data, C) == -1
    assert L.bertx_mvindex_train_centroids(ix.mv, C, 1, 0) == -1
    # the full scan
    q = np.ascontiguousarray(near_centroids(np.random.default_rng(121), cent, 8)[None])
    s = np.full((1, 2), 7.0, np.float32)
    i = np.full((1, 2), 7, np.int32)
    assert L.bertx_mvindex_search(ix.mv, q.ctypes.data, 1, 8, 2, s.ctypes.data, i.ctypes.data) == -1
    assert L.bertx_mvindex_search_device(ix.mv, q.ctypes.data, 1, 8, 2, s.ctypes.data, i.ctypes.data, None) == -1
    texts = bertpy.BertIndex._texts(["stone bridge"])
    assert L.bertx_mvindex_search_texts(ix.mv, model.ctx, 1, 1, texts, 2, s.ctypes.data, i.ctypes.data) == -1
    assert np.all(s == 7.0) and np.all(i == 7)
    # the readback of another kind, a bad id; the trainer on anything but an f16 store with centroids
    c = np.full(40, 9, np.uint16)
    b = np.full((40, w * nb // 8), 9, np.uint8)
    u = np.full(40, 9.0, np.float32)
    for mv, id_ in ((twin.mv, 0), (i8.mv, 0), (ix.mv, 2), (ix.mv, -1)):
        assert L.bertx_mvindex_doc_residual(mv, id_, c.ctypes.data, b.ctypes.data, u.ctypes.data) == -1
    assert np.all(c == 9) and np.all(b == 9) and np.all(u == 9.0)
    oc, ow = np.full(15, 9.0, np.float32), np.full(16, 9.0, np.float32)
    plain = store_of(model, docs, w, storage="f16")                        # no centroids
    for mv, bits in ((ix.mv, nb), (i8.mv, nb), (plain.mv, nb), (twin.mv, 1), (twin.mv, 3)):
        assert L.bertx_mvindex_train_residual_buckets(mv, bits, oc.ctypes.data, ow.ctypes.data) == -1
    assert np.all(oc == 9.0) and np.all(ow == 9.0)
    assert not L.bertx_index_create_ex(model.ctx, 0, 16, bertpy.BertTokenIndex.STORAGE[kind])   # the embedding index refuses
    after = [ix.doc_residual(i) for i in range(2)]
    for old, new in zip(before, after):
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(old, new))
    assert_state(ix, twin, (cut, wts))


def test_colbert_full_scan_refused(lib, tmp_path):
    import colbert_refs as CR
    m = bertpy.BertModel(CR.make_proj_models(lib, GOLDEN, str(tmp_path))[("tiny32", "f16")])
    ix = bertpy.BertTokenIndex(m, 4, 64, width=m.proj_width, storage="res2")
    s, i = np.full((1, 2), 7.0, np.float32), np.full((1, 2), 7, np.int32)
    rc = m.lib.bertx_mvindex_search_texts_colbert(ix.mv, m.ctx, 1, 1, bertpy.BertIndex._texts(["stone"]), 16, 2,
                                                  s.ctypes.data, i.ctypes.data)
    assert rc == -1 and np.all(s == 7.0) and np.all(i == 7)
    texts = bertpy.BertIndex._texts(["the stone bridge."])
    assert m.lib.bertx_mvindex_add_texts_colbert(ix.mv, m.ctx, 1, 1, texts, 32) == -1 and len(ix) == 0   # no centroids, no buckets


# ---- 10. the accuracy ordering ----
@pytest.mark.parametrize("sigma", (0.3, 0.6))
@pytest.mark.parametrize("w", (64, 128, 192))
def test_accuracy_ordering(model, w, sigma):
    """A condition, not a measurement: over all (query, row) pairs the mean |sim - sim of the
    f16 twin| is smaller with 4 bits than with 2, and smaller with 2 than with the centroid alone."""
    cent, rows, queries = RR.accuracy_case(w, sigma)
    docs = [r[None, :] for r in rows]                                      # one row per document: a score is a sim
    twin = twin_of(model, docs, w, cent)
    codes = [twin.doc_codes(i) for i in range(len(docs))]
    stores = [res_of(model, docs, w, kind, cent, twin.train_residual_buckets(RR.NBITS[kind])) for kind in ("res4", "res2")]
    stores.append(store_of(model, PR.substitute(cent, codes), w, storage="f16"))   # the centroid alone
    base = np.stack([twin.score(q[None, :]) for q in queries])
    err = [float(np.abs(np.stack([s.score(q[None, :]) for q in queries]).astype(np.float64) - base).mean()) for s in stores]
    print("w %d sigma %.1f: res4 %.5f res2 %.5f centroid %.5f" % (w, sigma, *err))
    assert 0 < err[0] < err[1] < err[2], err


# ---- 11. the text forms and the tool ----
def text_codec(model, texts, nb, colbert=None, width=None, C=16):
    """Centroids and buckets as the workflow trains them, on an f16 store of the texts, and the
    twin: an f16 store of the texts that is given the rows the residual store is given (the
    read-back centroids go through the packer once more)."""
    f = bertpy.BertTokenIndex(model, len(texts), len(texts) * 192, width=width)
    assert f.add_texts(texts, colbert=colbert) == 0
    f.train_centroids(C, iters=8, seed=0)
    cent = np.stack([f.centroid(c) for c in range(C)])
    twin = bertpy.BertTokenIndex(model, len(texts), len(texts) * 192, width=width)
    assert twin.add_texts(texts, colbert=colbert) == 0
    twin.set_centroids(cent)
    return twin, cent, f.train_residual_buckets(nb)


@pytest.mark.parametrize("kind", KINDS)
def test_text_path_equals_the_manual_path(model, tok_golden, kind):
    words = corpus_words(tok_golden)
    texts = corpus_texts(words, 12)
    twin, cent, buckets = text_codec(model, texts, RR.NBITS[kind])
    ids = [np.array(model.tokenize(t)[0], np.int32) for t in texts]
    cap = sum((len(t) + 15) // 16 * 16 for t in ids)
    a = empty_res(model, 64, kind, cent, buckets, 12, cap)
    assert a.add_texts(texts[:5]) == 0 and a.add_texts(texts[5:]) == 5 and len(a) == 12
    b = empty_res(model, 64, kind, cent, buckets, 12, cap)
    assert b.add(model.forward_tokens(ids)) == 0
    for i in range(12):
        for x, y in zip(a.doc_residual(i), b.doc_residual(i)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), i
    assert_state(a, twin, buckets)
    for query in (texts[3], " ".join(words[200:204])):
        qt = model.forward_tokens([np.array(model.tokenize(query)[0], np.int32)])[0]
        got = a.score_text(query)
        assert same(got, b.score(qt)) and same(got, a.score(qt))
        sub = [5, -1, 11, 5]
        assert same(a.score_text(query, sub), b.score(qt, sub))
        s, i = a.search_texts([query], 3, n_cand=12)
        ps, pi = b.search_pruned([qt], 3, 12)
        assert np.array_equal(i, pi) and same(s, ps)
    assert a.search_texts([texts[3]], 1, n_cand=12)[1][0, 0] == 3          # every token finds itself


def test_colbert_text_forms_on_a_residual_store(lib, tmp_path):
    import colbert_refs as CR
    m = bertpy.BertModel(CR.make_proj_models(lib, GOLDEN, str(tmp_path))[("tiny32", "f16")])
    texts = ["the stone bridge over the river.", "a, b; c!", "", "one two three four five six seven",
             " ".join(["stone", "river,", "x.y", "42", "bridge!"] * 12)]
    doc_maxlen, query_maxlen = 32, 16
    twin, cent, buckets = text_codec(m, texts, 2, colbert=doc_maxlen, width=m.proj_width)
    toks = [m.tokenize_colbert(t, "doc", doc_maxlen) for t in texts]
    rows = m.forward_project([i for i, _ in toks])
    docs = [r[k == 1] for r, (_, k) in zip(rows, toks)]
    a = empty_res(m, m.proj_width, "res2", cent, buckets, 8, 8 * 32)
    b = empty_res(m, m.proj_width, "res2", cent, buckets, 8, 8 * 32)
    assert a.add_texts(texts, colbert=doc_maxlen) == 0 and b.add(docs) == 0
    assert len(a) == len(b) == len(texts) and a.token_slots == b.token_slots
    for i in range(len(texts)):
        for x, y in zip(a.doc_residual(i), b.doc_residual(i)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), i
    assert_state(a, twin, buckets)
    ids = np.array([3, -1, 0, 99, 4, 4], np.int32)
    for q in ("stone bridge", "a, b."):
        qi, qk = m.tokenize_colbert(q, "query", query_maxlen)
        qrows = m.forward_project([qi])[0]
        for sel in (ids, None):
            assert same(a.score_text(q, sel, colbert=query_maxlen), b.score(qrows, sel))
        s, i = a.search_texts([q], 2, colbert=query_maxlen, n_cand=5)
        ps, pi = b.search_pruned([qrows], 2, 5)
        assert np.array_equal(i, pi) and same(s, ps)


def test_search_tool_residual_store(model, tmp_path):
    """search -l -a -C 16 -S res2 prints the pruned search's ranking of a residual store built
    by the documented workflow; -S res2 without -C is a usage error."""
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(COLBERT_TEXTS) + "\n")
    queries = ["stone bridge", "one two", "marks, words"]
    k = 3
    base = ["-m", TINY64, "-f", str(corpus), "-k", str(k)]
    r, got = tool_lines(base + ["-l", "-a", "-C", "16", "-c", "5", "-S", "res2"], queries)
    assert r.returncode == 0, r.stderr
    f = bertpy.BertTokenIndex(model, 10, 10 * 32)
    assert f.add_texts(COLBERT_TEXTS) == 0
    f.train_centroids(16, iters=8, seed=0)
    cent = np.stack([f.centroid(c) for c in range(16)])
    ix = empty_res(model, 64, "res2", cent, f.train_residual_buckets(2), 10, 10 * 32)
    assert ix.add_texts(COLBERT_TEXTS) == 0
    s, i = ix.search_texts(queries, k, n_cand=5)
    want = ["%d\t%d\t%.4f\t%s" % (j + 1, i[b, j], s[b, j], COLBERT_TEXTS[i[b, j]]) for b in range(3) for j in range(k)]
    assert got == want
    for bad in (["-l", "-a", "-S", "res2"], ["-l", "-S", "res4"], ["-S", "res2"]):
        r, _ = tool_lines(base + bad, [])
        assert r.returncode == 2 and "usage" in r.stderr, bad


@pytest.mark.parametrize("storage", (4, 5))
def test_bench_hook(model, storage):
    us = (ctypes.c_float * 2)(0, 0)
    assert model.lib.bertx_bench_maxsim_res(64, 300, 0, 16, 32, 200, storage, 2, us) == 0
    assert min(us) > 0
    assert model.lib.bertx_bench_maxsim_res(64, 300, 0, 16, 32, 200, 0, 2, us) < 0      # not a residual kind
    assert model.lib.bertx_bench_maxsim_res(64, 300, 0, 24, 32, 200, storage, 2, us) < 0     # C = 24
