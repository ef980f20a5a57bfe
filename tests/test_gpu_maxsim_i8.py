"""The int8 token store on the GPU (bertx_mvindex_create_ex with BERTX_INDEX_I8,
maxsim_i8.hip) against the numpy reference (maxsim_i8_refs.py): bytes, scales and scores
bit for bit, and the contract's accuracy bound against the exact cosine.  A store takes
its width from the caller, so the golden tiny model serves every width; only the text
forms need its own 64."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import maxsim_i8_refs as R
import maxsim_refs as M
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

TINY64 = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")


@pytest.fixture(scope="module", autouse=True)
def _one_device():
    os.environ.pop("BERT_HOST_ONLY", None)
    os.environ["BERT_DEVICES"] = "0"


@pytest.fixture(scope="module")
def model():
    return bertpy.BertModel(TINY64)


def slots_of(docs):
    return sum((len(d) + 15) // 16 * 16 for d in docs)


def store_of(model, docs, w, storage="int8", extra_docs=0, extra_slots=0):
    ix = bertpy.BertTokenIndex(model, len(docs) + extra_docs, slots_of(docs) + extra_slots, width=w, storage=storage)
    assert ix.add(docs) == 0 and len(ix) == len(docs) and ix.token_slots == slots_of(docs)
    return ix


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# the references, computed once per width and left unchanged
_packed, _refs = {}, {}


def packed_parity(w):
    if w not in _packed:
        docs, queries = M.parity_case(w)
        _packed[w] = (docs, queries, [R.pack(d) for d in docs])
    return _packed[w]


def parity_ref(w, Lq):
    if (w, Lq) not in _refs:
        _, queries, dp = packed_parity(w)
        qp = R.pack(queries[Lq])
        ref = np.array([R.score(qp, d) for d in dp], np.float32)
        ref.setflags(write=False)
        _refs[(w, Lq)] = ref
    return _refs[(w, Lq)]


_stores = {}


@pytest.fixture(scope="module")
def parity_store(model):
    def get(w):
        if w not in _stores:
            _stores[w] = store_of(model, packed_parity(w)[0], w)
        return _stores[w]
    yield get
    _stores.clear()


# ---- device buffers through the HIP runtime libbert.so is linked against ----
class DeviceArrays:
    def __init__(self):
        h = self.hip = ctypes.CDLL("libamdhip64.so.7")
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
        self.ptrs = []

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), max(nbytes, 16)) == 0
        self.ptrs.append(p)
        return p

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

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


# ---- 1. the pack kernel ----
@pytest.mark.parametrize("w", R.WIDTHS)
def test_pack_parity(model, dev, w):
    docs = M.pack_case(w)
    ix = store_of(model, docs, w)
    assert ix.storage == "int8" and model.lib.bertx_mvindex_storage(ix.mv) == 1
    one = bertpy.BertTokenIndex(model, len(docs), slots_of(docs), width=w, storage="int8")
    for i, d in enumerate(docs):
        assert one.add([d]) == i
    devf = bertpy.BertTokenIndex(model, len(docs), slots_of(docs), width=w, storage="int8")
    lens = np.array([len(d) for d in docs], np.int32)
    assert model.lib.bertx_mvindex_add_device(devf.mv, dev.up(np.concatenate(docs)), lens.ctypes.data, len(docs), None) == 0
    for i, d in enumerate(docs):
        q, u = ix.doc_i8(i)
        rq, ru = R.pack(d)
        assert q.dtype == np.int8 and np.array_equal(q, rq), i
        assert same(u, ru), i
        assert same(ix.doc(i), q.astype(np.float32) * u[:, None]), i           # one f32 multiply
        for other in (one, devf):                                              # one add per document; the device form
            oq, ou = other.doc_i8(i)
            assert np.array_equal(oq, q) and same(ou, u), i
    q, u = ix.doc_i8(2)
    assert not q[7].any() and u[7] == 0 and q[6].any() and u[6] > 0             # the zero row, and its neighbour
    assert not ix.doc(2)[7].any()
    # an f16 store has no bytes to return; a bad id
    f16 = store_of(model, docs, w, storage="f16")
    assert f16.storage == "f16" and model.lib.bertx_mvindex_storage(f16.mv) == 0
    bq, bu = np.full((33, w), 7, np.int8), np.full(33, 7.5, np.float32)
    for mv, i in ((f16.mv, 0), (ix.mv, len(docs)), (ix.mv, -1)):
        assert model.lib.bertx_mvindex_doc_i8(mv, i, bq.ctypes.data, bu.ctypes.data) == -1
        assert np.all(bq == 7) and np.all(bu == 7.5)


# ---- 2. score parity ----
@pytest.mark.parametrize("Lq", M.QUERY_LENS)
@pytest.mark.parametrize("w", R.WIDTHS)
def test_score_parity(model, parity_store, w, Lq):
    ix, ref = parity_store(w), parity_ref(w, Lq)
    q = packed_parity(w)[1][Lq]
    n = len(ix)
    rng = np.random.default_rng(100 * w + Lq)
    ids = np.concatenate([rng.permutation(n), rng.integers(0, n, 7), [-1, n]]).astype(np.int32)   # every document, repeats, bad ids
    ids = ids[rng.permutation(len(ids))]
    want = np.where((ids >= 0) & (ids < n), ref[np.clip(ids, 0, n - 1)], np.float32(-np.inf)).astype(np.float32)
    out = np.full(len(ids) + 8, 7.5, np.float32)
    assert model.lib.bertx_mvindex_score(ix.mv, q.ctypes.data, Lq, ids.ctypes.data, len(ids), out.ctypes.data) == 0
    assert same(out[:len(ids)], want), (out[:len(ids)], want)
    assert np.all(out[len(ids):] == 7.5)
    assert same(ix.score(q), ref)                                              # ids = NULL


# ---- 3. accuracy against the exact cosine ----
@pytest.mark.parametrize("w", R.WIDTHS)
def test_accuracy_against_the_exact_maxsim(parity_store, w):
    ix = parity_store(w)
    docs, queries, _ = packed_parity(w)
    worst = 0.0
    for Lq, q in queries.items():
        got = ix.score(q)
        for d, s in zip(docs, got):
            bound = Lq * float(R.sim_bound(q, d).max())
            err = abs(float(s) - R.exact_maxsim(q, d))
            worst = max(worst, err / bound)
            assert err <= bound, (w, Lq, len(d), err, bound)
    print("worst |score - exact MaxSim| / bound at w = %d: %.3f" % (w, worst))


# ---- 4. padding: stale bytes and stale scales ----
@pytest.mark.parametrize("w", R.WIDTHS)
def test_stale_bytes_and_scales_in_the_padding(model, parity_store, w):
    docs, queries, _ = packed_parity(w)
    Lq = 17
    q = queries[Lq]
    fill = [np.ascontiguousarray(np.resize(q, (512, w)))] * 2                  # every slot: a copy of a query token
    assert slots_of(fill) >= slots_of(docs)
    ix = bertpy.BertTokenIndex(model, len(docs), slots_of(fill), width=w, storage="int8")
    assert ix.add(fill) == 0
    assert np.all(ix.score(q) > 0.99 * Lq)
    ix.clear()
    assert len(ix) == 0 and ix.token_slots == 0
    assert ix.add(docs) == 0
    assert same(ix.score(q), parity_store(w).score(q)) and same(ix.score(q), parity_ref(w, Lq))


@pytest.mark.parametrize("w", R.WIDTHS)
def test_planted_rows(model, w):
    for n in (17, 33):
        q, doc = M.planted_last(w, n)
        got = store_of(model, [doc, doc[:-1]], w).score(q)
        assert same(got, [R.score(R.pack(q), R.pack(d)) for d in (doc, doc[:-1])])
        assert abs(float(got[0]) - 1.0) <= 2.0 ** -22 and abs(float(got[1])) < 0.01, got
    for Lq in (1, 17):
        q, doc = M.planted_negative(w, Lq)
        got = store_of(model, [doc], w).score(q)
        assert same(got, [R.score(R.pack(q), R.pack(doc))])
        assert abs(float(got[0]) + Lq) <= Lq * 2.0 ** -22, got


# ---- 5. independence ----
def test_score_is_independent_bit_for_bit(model):
    w, Lq = 192, 17
    rng = np.random.default_rng(70)
    q = M.token_rows(rng, Lq, w)
    x = M.token_rows(rng, 37, w)
    others_a = [M.token_rows(rng, int(n), w) for n in rng.integers(1, 70, 8)]
    others_b = [M.token_rows(rng, int(n), w) for n in rng.integers(1, 70, 8)]
    ref = store_of(model, [x], w).score(q)                                      # alone
    assert same(ref, [R.score(R.pack(q), R.pack(x))])
    a = store_of(model, [x] + others_a[:4] + [x] + others_a[4:], w, extra_docs=1, extra_slots=48)
    b = store_of(model, others_b[:3] + [x] + others_b[3:], w)                   # other neighbours (id 3)
    sa = a.score(q)
    assert same(sa[0:1], ref) and same(sa[5:6], ref) and same(b.score(q)[3:4], ref)
    n = len(a)
    many = rng.integers(0, n, 1000).astype(np.int32)                            # any list: 1,000 candidates, repeats
    assert same(a.score(q, many), sa[many])
    assert same(a.score(q, np.arange(n)[::-1]), sa[::-1]) and same(a.score(q, [5, 5, 0, 5]), np.repeat(ref, 4))
    assert a.add([x]) == n                                                      # after more documents are added
    assert same(a.score(q), np.concatenate([sa, ref]))


# ---- 6. ranking ----
@pytest.mark.parametrize("w,Lq,N,seed", M.RANKING_CASES)
def test_rerank_order_is_the_planted_order(model, w, Lq, N, seed):
    q, docs, order = M.ranking_corpus(w, Lq, N, seed)
    ix = store_of(model, docs, w)
    cand = np.random.default_rng(seed).permutation(N).astype(np.int32)
    ids, scores = ix.rerank(q, cand)
    assert np.array_equal(ids, order) and np.all(np.diff(scores) < 0)


# ---- 7. plumbing ----
def test_score_device_captured_graph(model, dev):
    w, Lq = 192, 33
    docs = packed_parity(w)[0]
    rng = np.random.default_rng(90)
    q = M.token_rows(rng, Lq, w)
    ix = store_of(model, docs, w, extra_docs=2, extra_slots=64)
    ids = np.array([3, -1, 8, 0, 8, 5], np.int32)
    want = ix.score(q, ids)
    qp = R.pack(q)
    assert same(want[[0, 2]], [R.score(qp, R.pack(docs[3])), R.score(qp, R.pack(docs[8]))]) and np.isneginf(want[1])
    hip, vp, lib = dev.hip, ctypes.c_void_p, model.lib
    s = vp()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    dq, di, do = dev.up(q), dev.up(ids), dev.alloc(len(ids) * 4)
    assert lib.bertx_mvindex_score_device(ix.mv, dq, Lq, di, len(ids), do, s) == 0
    assert hip.hipStreamSynchronize(s) == 0
    assert same(dev.down(do, len(ids), np.float32), want)
    graph, ex = vp(), vp()
    assert hip.hipStreamBeginCapture(s, 1) == 0   # thread-local mode
    rc = lib.bertx_mvindex_score_device(ix.mv, dq, Lq, di, len(ids), do, s)
    assert hip.hipStreamEndCapture(s, ctypes.byref(graph)) == 0 and rc == 0
    assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, 0) == 0
    zeros = np.zeros(len(ids), np.float32)
    for round_ in range(3):
        if round_ == 2:                           # a later add to the store
            assert ix.add([M.token_rows(rng, 20, w)]) == len(docs)
        assert hip.hipMemcpy(do, zeros.ctypes.data, zeros.nbytes, 1) == 0
        assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
        assert same(dev.down(do, len(ids), np.float32), want)
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    hip.hipStreamDestroy(s)


def test_text_path_equals_the_manual_path(model, tok_golden):
    words = [w for w in tok_golden["vocab"][104:] if w.isascii() and w.isalpha() and len(w) > 2]
    W = len(words)
    texts = [" ".join(words[(7 * i + 13 * j + j * j) % W] for j in range(3 + (5 * i) % 28)) for i in range(12)]
    ids = [np.array(model.tokenize(t)[0], np.int32) for t in texts]
    cap = sum((len(t) + 15) // 16 * 16 for t in ids)
    a = bertpy.BertTokenIndex(model, 12, cap, storage="int8")
    assert a.add_texts(texts[:5]) == 0 and a.add_texts(texts[5:]) == 5 and len(a) == 12
    b = bertpy.BertTokenIndex(model, 12, cap, storage="int8")
    rows = model.forward_tokens(ids)
    assert b.add(rows) == 0
    for i in range(12):
        (aq, au), (bq, bu) = a.doc_i8(i), b.doc_i8(i)
        assert np.array_equal(aq, bq) and same(au, bu), i
        rq, ru = R.pack(rows[i])
        assert np.array_equal(aq, rq) and same(au, ru), i
    for query in (texts[3], " ".join(words[200:204])):
        qt = model.forward_tokens([np.array(model.tokenize(query)[0], np.int32)])[0]
        got = a.score_text(query)
        assert same(got, b.score(qt)) and same(got, a.score(qt))
        sub = [5, -1, 11, 5]
        assert same(a.score_text(query, sub), b.score(qt, sub))
    assert a.rerank(texts[3], np.arange(12))[0][0] == 3                        # every token finds itself


def test_colbert_text_forms_on_an_int8_store(lib, tmp_path):
    """add_texts_colbert / score_text_colbert on an int8 store == the manual route through
    tokenize_colbert, forward_project, add() and score(), bit for bit."""
    import colbert_refs as CR
    m = bertpy.BertModel(CR.make_proj_models(lib, GOLDEN, str(tmp_path))[("tiny32", "f16")])
    texts = ["the stone bridge over the river.", "a, b; c!", "", "one two three four five six seven",
             " ".join(["stone", "river,", "x.y", "42", "bridge!"] * 12)]
    doc_maxlen, query_maxlen = 32, 16
    toks = [m.tokenize_colbert(t, "doc", doc_maxlen) for t in texts]
    rows = m.forward_project([i for i, _ in toks])
    docs = [r[k == 1] for r, (_, k) in zip(rows, toks)]
    assert any((k == 0).any() for _, k in toks)                                # the skiplist drops rows
    a = bertpy.BertTokenIndex(m, 8, 8 * 32, width=m.proj_width, storage="int8")
    b = bertpy.BertTokenIndex(m, 8, 8 * 32, width=m.proj_width, storage="int8")
    assert a.add_texts(texts, colbert=doc_maxlen) == 0 and b.add(docs) == 0
    assert len(a) == len(b) == len(texts) and a.token_slots == b.token_slots
    for i, d in enumerate(docs):
        (aq, au), (bq, bu), (rq, ru) = a.doc_i8(i), b.doc_i8(i), R.pack(d)
        assert np.array_equal(aq, bq) and same(au, bu) and np.array_equal(aq, rq) and same(au, ru), i
    ids = np.array([3, -1, 0, 99, 4, 4], np.int32)
    for q in ("stone bridge", "a, b."):
        qi, qk = m.tokenize_colbert(q, "query", query_maxlen)
        assert len(qi) == query_maxlen and np.all(qk == 1)
        qrows = m.forward_project([qi])[0]
        for sel in (ids, None):
            assert same(a.score_text(q, sel, colbert=query_maxlen), b.score(qrows, sel))
        got = a.score_text(q, colbert=query_maxlen)
        assert same(got, [R.score(R.pack(qrows), R.pack(d)) for d in docs])
        assert np.isneginf(a.score_text(q, ids, colbert=query_maxlen)[[1, 3]]).all()


def test_search_tool_int8_token_store(model, tok_golden, tmp_path):
    """search -l -S int8 prints the int8 store's rerank; -S without a token store is refused."""
    words = [w for w in tok_golden["vocab"][104:] if w.isascii() and w.isalpha() and len(w) > 2]
    W = len(words)
    texts = [" ".join(words[(7 * i + 13 * j + j * j) % W] for j in range(3 + (5 * i) % 28)) for i in range(40)]
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(texts) + "\n")
    queries = [texts[3], texts[22]]
    k, cand = 4, 12
    tool = [os.path.join(ROOT, "build", "bin", "search"), "-m", TINY64, "-f", str(corpus), "-k", str(k)]
    r = subprocess.run(tool + ["-l", "-c", str(cand), "-S", "int8"], input="\n".join(queries) + "\nq\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [ln for ln in r.stdout.splitlines() if "\t" in ln]
    ix = bertpy.BertIndex(model, 40)
    assert ix.add_texts(texts) == 0
    mv = bertpy.BertTokenIndex(model, 40, 40 * 32, storage="int8")
    assert mv.add_texts(texts) == 0
    want = []
    for query in queries:
        rid, rsc = mv.rerank(query, ix.search_texts([query], cand)[1][0], top_k=k)
        want += ["%d\t%d\t%.4f\t%s" % (j + 1, rid[j], rsc[j], texts[rid[j]]) for j in range(k)]
    assert got == want
    assert got[0].split("\t")[1] == "3" and got[k].split("\t")[1] == "22"
    r = subprocess.run(tool + ["-S", "int8"], input="q\n", capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "usage" in r.stderr


def test_create_ex_f16_is_create(model):
    w, Lq = 192, 17
    docs, queries, _ = packed_parity(w)
    lib = model.lib
    a = bertpy.BertTokenIndex(model, len(docs), slots_of(docs), width=w)                   # create_ex(.., F16)
    plain = lib.bertx_mvindex_create(model.ctx, 0, w, len(docs), slots_of(docs))
    assert plain and lib.bertx_mvindex_storage(plain) == 0 and lib.bertx_mvindex_storage(a.mv) == 0
    try:
        assert a.add(docs) == 0
        rows = np.ascontiguousarray(np.concatenate(docs))
        lens = np.array([len(d) for d in docs], np.int32)
        assert lib.bertx_mvindex_add(plain, rows.ctypes.data, lens.ctypes.data, len(docs)) == 0
        out = np.zeros(len(docs), np.float32)
        q = queries[Lq]
        assert lib.bertx_mvindex_score(plain, q.ctypes.data, Lq, None, len(docs), out.ctypes.data) == 0
        assert same(out, a.score(q))
        assert not same(out, parity_ref(w, Lq))                                # and int8 is another arithmetic
    finally:
        lib.bertx_mvindex_free(plain)
    assert not lib.bertx_mvindex_create_ex(model.ctx, 0, w, 4, 64, 2)          # no such kind
    assert not lib.bertx_mvindex_create_ex(model.ctx, 0, w, 4, 64, -1)
