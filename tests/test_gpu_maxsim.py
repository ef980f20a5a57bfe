"""The token store and its fused MaxSim scorer on the GPU (bertx_mvindex_*, maxsim.hip)
against the numpy reference (maxsim_refs.py).  Tolerances are the contract's: a stored
element within elem_tol of the exact x_i / |x|, a score within score_tol of the float64
MaxSim of the read-back f16 values (the query's f16 values are read back too: it is added
as a document, one normaliser serves both).  Everything else is bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import maxsim_refs as M
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

TINY64 = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")


@pytest.fixture(scope="module", autouse=True)
def _one_device():
    os.environ.pop("BERT_HOST_ONLY", None)
    os.environ["BERT_DEVICES"] = "0"


_models = {}


@pytest.fixture(scope="module")
def model_of_width(tmp_path_factory):
    """A context of n_embd d: tiny64 for 64, else a one-layer synthetic f16 model."""
    def get(d):
        if d not in _models:
            if d == 64:
                path = TINY64
            else:
                path = str(tmp_path_factory.mktemp("mvw%d" % d) / "m.bin")
                hp = dict(n_vocab=256, n_max_tokens=32, n_embd=d, n_intermediate=128, n_head=d // 64, n_layer=1)
                bertpy.synthetic_model(path, hp, "f16")
            _models[d] = bertpy.BertModel(path)
        return _models[d]
    yield get
    _models.clear()


def slots_of(docs):
    return sum((len(d) + 15) // 16 * 16 for d in docs)


def store_of(model, docs, extra_docs=0, extra_slots=0, width=None):
    ix = bertpy.BertTokenIndex(model, len(docs) + extra_docs, slots_of(docs) + extra_slots, width=width)
    assert ix.add(docs) == 0 and len(ix) == len(docs) and ix.token_slots == slots_of(docs)
    return ix


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def f16_of(ix, rows):
    """The f16 values the store keeps of `rows`: added to a scratch store and read back."""
    tmp = bertpy.BertTokenIndex(ix.model, 1, slots_of([rows]), width=ix.dim)
    assert tmp.add([rows]) == 0
    return tmp.doc(0)


def check_scores(ix, q, ids, got):
    q16 = f16_of(ix, q)
    worst = 0.0
    for i, s in zip(ids, got):
        ref = M.maxsim(q16, ix.doc(int(i)))
        err, tol = abs(float(s) - ref), M.score_tol(len(q), ix.dim)
        worst = max(worst, err / tol)
        assert err <= tol, (int(i), float(s), ref, err, tol)
    return worst


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
@pytest.mark.parametrize("w", M.WIDTHS)
def test_pack_parity(model_of_width, dev, w):
    m = model_of_width(w)
    docs = M.pack_case(w)
    ix = store_of(m, docs)
    worst = 0.0
    for i, d in enumerate(docs):
        got = ix.doc(i)
        assert ix.doc_len(i) == len(d) and got.shape == d.shape
        assert same(got.astype(np.float16).astype(np.float32), got)      # f16 values
        want = M.normalise(d)
        ratio = np.abs(got.astype(np.float64) - want) / M.elem_tol(want, w)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (i, float(ratio.max()))
    print("worst element error / bound at w = %d: %.3f" % (w, worst))
    assert not ix.doc(2)[7].any() and ix.doc(2)[6].any()                # the zero row, and its neighbour
    # one add of several documents == the same documents one by one == the device form
    one = bertpy.BertTokenIndex(m, len(docs), slots_of(docs))
    for i, d in enumerate(docs):
        assert one.add([d]) == i
    devf = bertpy.BertTokenIndex(m, len(docs), slots_of(docs))
    lens = np.array([len(d) for d in docs], np.int32)
    assert m.lib.bertx_mvindex_add_device(devf.mv, dev.up(np.concatenate(docs)), lens.ctypes.data, len(docs), None) == 0
    for i in range(len(docs)):
        assert same(one.doc(i), ix.doc(i)) and same(devf.doc(i), ix.doc(i))
    assert one.token_slots == ix.token_slots == devf.token_slots


def test_add_refusals_change_nothing(model_of_width):
    w = 64
    m = model_of_width(w)
    docs = M.pack_case(w)
    ix = store_of(m, docs, extra_docs=1, extra_slots=16)
    before = [ix.doc(i) for i in range(len(docs))]
    lib, rng = m.lib, np.random.default_rng(5)

    def add_rc(ds):
        rows = np.ascontiguousarray(np.concatenate(ds))
        lens = np.array([len(d) for d in ds], np.int32)
        return lib.bertx_mvindex_add(ix.mv, rows.ctypes.data, lens.ctypes.data, len(ds))

    def unchanged():
        assert len(ix) == len(docs) and ix.token_slots == slots_of(docs)
        assert all(same(ix.doc(i), b) for i, b in enumerate(before))

    assert add_rc([M.token_rows(rng, 3, w), M.token_rows(rng, 3, w)]) == -2     # one document too many
    unchanged()
    assert add_rc([M.token_rows(rng, 17, w)]) == -2                              # one group too many
    unchanged()
    rows, lens = M.token_rows(rng, 4, w), np.array([4, 0], np.int32)
    assert lib.bertx_mvindex_add(ix.mv, rows.ctypes.data, lens.ctypes.data, 2) == -1   # a len of 0
    unchanged()
    assert add_rc([M.token_rows(rng, 16, w)]) == len(docs)                        # what fits still does
    assert len(ix) == len(docs) + 1 and all(same(ix.doc(i), b) for i, b in enumerate(before))


# ---- 2. score parity ----
_parity = {}


@pytest.fixture(scope="module")
def parity_store(model_of_width):
    def get(w):
        if w not in _parity:
            docs, queries = M.parity_case(w)
            _parity[w] = (store_of(model_of_width(w), docs), queries)
        return _parity[w]
    yield get
    _parity.clear()


@pytest.mark.parametrize("Lq", M.QUERY_LENS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_score_parity(parity_store, w, Lq):
    ix, queries = parity_store(w)
    ids = np.arange(len(ix), dtype=np.int32)
    got = ix.score(queries[Lq], ids)
    worst = check_scores(ix, queries[Lq], ids, got)
    print("worst score error / bound at w = %d, Lq = %d: %.4f" % (w, Lq, worst))


# ---- 3. planted rows ----
@pytest.mark.parametrize("n", (17, 33))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_planted_last_token_counts(model_of_width, w, n):
    q, doc = M.planted_last(w, n)
    ix = store_of(model_of_width(w), [doc, doc[:-1]])
    got = ix.score(q)
    check_scores(ix, q, [0, 1], got)
    assert got[0] > 0.99 and abs(got[1]) < 0.01, got


@pytest.mark.parametrize("Lq", (1, 17))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_planted_all_negative(model_of_width, w, Lq):
    q, doc = M.planted_negative(w, Lq)
    assert len(doc) == 5
    ix = store_of(model_of_width(w), [doc])
    got = ix.score(q)
    check_scores(ix, q, [0], got)
    assert abs(got[0] + Lq) < 2e-3 * Lq, got


# ---- 4. stale rows ----
@pytest.mark.parametrize("w", (64, 768))
def test_stale_rows_behind_short_documents(model_of_width, w):
    m = model_of_width(w)
    rng = np.random.default_rng(60 + w)
    Lq, n = 16, 6
    q = M.unit_rows(rng, Lq, w)
    short = [M.orthogonal_to(rng, 3, q) for _ in range(n)]
    fresh = store_of(m, short)
    want = fresh.score(q)
    ix = bertpy.BertTokenIndex(m, n, 16 * n)
    assert ix.add([q] * n) == 0                        # every slot of every group: a copy of a query token
    assert np.all(ix.score(q) > 0.99 * Lq)
    ix.clear()
    assert len(ix) == 0 and ix.token_slots == 0
    assert ix.add(short) == 0
    got = ix.score(q)
    assert same(got, want), (got, want)
    assert np.all(np.abs(got) < 0.01 * Lq)


# ---- 5. invariance ----
def test_score_is_invariant_bit_for_bit(model_of_width):
    w, Lq = 192, 17
    m = model_of_width(w)
    rng = np.random.default_rng(70)
    q = M.token_rows(rng, Lq, w)
    x = M.token_rows(rng, 37, w)
    others_a = [M.token_rows(rng, int(n), w) for n in rng.integers(1, 70, 8)]
    others_b = [M.token_rows(rng, int(n), w) for n in rng.integers(1, 70, 8)]
    a = store_of(m, [x] + others_a[:4] + [x] + others_a[4:] + [x])      # id 0, the middle (5), the last (10)
    b = store_of(m, others_b[:3] + [x] + others_b[3:])                  # other neighbours (id 3)
    sa, sb = a.score(q), b.score(q)
    ref = sa[0:1]
    assert same(sa[5:6], ref) and same(sa[10:11], ref) and same(sb[3:4], ref)
    n = len(a)
    all_ids = np.arange(n, dtype=np.int32)
    assert same(a.score(q, all_ids), sa)                                # ids = NULL and the explicit list
    assert same(a.score(q, [5]), ref)                                   # a list of 1
    assert same(a.score(q, all_ids[::-1]), sa[::-1])                    # reversed
    many = rng.integers(0, n, 1000).astype(np.int32)                    # 1,000 candidates, repeated ids
    assert same(a.score(q, many), sa[many])
    assert same(a.score(q, [5, 5, 0, 5]), np.repeat(ref, 4))


# ---- 6. bad ids, the output guard ----
def test_bad_ids_score_minus_infinity(model_of_width):
    w = 64
    ix, q = store_of(model_of_width(w), M.pack_case(w)), M.token_rows(np.random.default_rng(80), 5, w)
    n = len(ix)
    want = ix.score(q)
    got = ix.score(q, [-1, 0, n, 1, -5, 2, n + 1000, 3, 2 ** 31 - 1, 4, -2 ** 31])
    assert np.all(np.isneginf(got[0::2])) and same(got[1::2], want)


def test_only_n_outputs_are_written(model_of_width, dev):
    w = 64
    m = model_of_width(w)
    ix, q = store_of(m, M.pack_case(w)), M.token_rows(np.random.default_rng(81), 17, w)
    want = ix.score(q)
    n = len(ix)
    ids = np.arange(n, dtype=np.int32)
    out = np.full(n + 8, 7.5, np.float32)
    assert m.lib.bertx_mvindex_score(ix.mv, q.ctypes.data, len(q), ids.ctypes.data, n - 1, out.ctypes.data) == 0
    assert same(out[:n - 1], want[:n - 1]) and np.all(out[n - 1:] == 7.5)
    d_out = dev.up(np.full(n + 8, 7.5, np.float32))
    assert m.lib.bertx_mvindex_score_device(ix.mv, dev.up(q), len(q), dev.up(ids), n - 1, d_out, None) == 0
    ix.doc(0)                                     # a host call on the store returns after everything before it
    got = dev.down(d_out, n + 8, np.float32)
    assert same(got[:n - 1], want[:n - 1]) and np.all(got[n - 1:] == 7.5)


# ---- 7. the device form, captured ----
def test_score_device_and_captured_graph(model_of_width, dev):
    w, Lq = 192, 33
    m = model_of_width(w)
    docs, _ = M.parity_case(w)
    rng = np.random.default_rng(90)
    q = M.token_rows(rng, Lq, w)
    ix = store_of(m, docs, extra_docs=2, extra_slots=64)
    ids = np.array([3, -1, 8, 0, 8, 5], np.int32)
    want = ix.score(q, ids)
    check_scores(ix, q, ids[ids >= 0], want[ids >= 0])
    hip, vp, lib = dev.hip, ctypes.c_void_p, m.lib
    s = vp()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    dq, di, do = dev.up(q), dev.up(ids), dev.alloc(len(ids) * 4)
    assert lib.bertx_mvindex_score_device(ix.mv, dq, Lq, di, len(ids), do, s) == 0
    assert hip.hipStreamSynchronize(s) == 0
    assert same(dev.down(do, len(ids), np.float32), want)
    do_all = dev.alloc(len(ix) * 4)                                       # ids = NULL
    assert lib.bertx_mvindex_score_device(ix.mv, dq, Lq, None, len(ix), do_all, s) == 0
    assert hip.hipStreamSynchronize(s) == 0
    assert same(dev.down(do_all, len(ix), np.float32), ix.score(q))
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


# ---- 8. refusals ----
def test_refusals(model_of_width, capfd):
    w = 64
    m = model_of_width(w)
    lib = m.lib
    for slot, width, cd, cs in ((1, 64, 4, 64), (-1, 64, 4, 64), (0, 32, 4, 64), (0, 96, 4, 64), (0, 1088, 4, 64 * 17),
                                (0, 64, 0, 64), (0, 64, 4, 0), (0, 64, 4, 15)):
        assert not lib.bertx_mvindex_create(m.ctx, slot, width, cd, cs), (slot, width, cd, cs)
    ix = store_of(m, M.pack_case(w))
    q = M.token_rows(np.random.default_rng(95), 65, w)
    ids = np.arange(len(ix), dtype=np.int32)
    out = np.full(len(ix), 7.5, np.float32)
    for Lq, n in ((0, 3), (65, 3), (-1, 3), (5, 0), (5, -1)):
        assert lib.bertx_mvindex_score(ix.mv, q.ctypes.data, Lq, ids.ctypes.data, n, out.ctypes.data) == -1
    assert lib.bertx_mvindex_score(ix.mv, None, 5, ids.ctypes.data, 3, out.ctypes.data) == -1
    assert np.all(out == 7.5)
    assert ix.doc_len(-1) == -1 and ix.doc_len(len(ix)) == -1
    row = np.full((1, w), 7.5, np.float32)
    assert lib.bertx_mvindex_doc(ix.mv, len(ix), row.ctypes.data) == -1 and np.all(row == 7.5)
    # the text forms need width == n_embd
    wide = bertpy.BertTokenIndex(m, 4, 64, width=128)
    assert wide.dim == 128
    t = (ctypes.c_char_p * 1)(b"hello")
    assert lib.bertx_mvindex_add_texts(wide.mv, m.ctx, 1, 1, t) == -1 and len(wide) == 0
    one = np.full(1, 7.5, np.float32)
    assert lib.bertx_mvindex_score_text(wide.mv, m.ctx, b"hello", None, 1, one.ctypes.data) == -1 and one[0] == 7.5
    # a store of a foreign width scores what the caller projected itself
    rng = np.random.default_rng(96)
    docs = [M.token_rows(rng, n, 128) for n in (3, 20)]
    assert wide.add(docs) == 0
    qq = M.token_rows(rng, 4, 128)
    check_scores(wide, qq, [0, 1], wide.score(qq))


# ---- 9. texts ----
def corpus_texts(tok_golden):
    """40 distinct texts of whole words of the golden vocabulary, of 3 .. 30 words."""
    words = [w for w in tok_golden["vocab"][104:] if w.isascii() and w.isalpha() and len(w) > 2]
    W = len(words)
    assert W > 300
    texts = [" ".join(words[(7 * i + 13 * j + j * j) % W] for j in range(3 + (5 * i) % 28)) for i in range(40)]
    assert len(set(texts)) == 40
    return texts, words


def test_text_path_equals_the_manual_path(tok_golden):
    m = bertpy.BertModel(TINY64)
    texts, words = corpus_texts(tok_golden)
    toks = [m.tokenize(t) for t in texts]
    assert all(n <= m.n_max_tokens for _, n in toks)
    ids = [np.array(t, np.int32) for t, _ in toks]
    cap = sum((len(t) + 15) // 16 * 16 for t in ids)
    a = bertpy.BertTokenIndex(m, 41, cap + 16)
    assert a.add_texts(texts[:7]) == 0 and a.add_texts(texts[7:]) == 7 and len(a) == 40
    assert [a.doc_len(i) for i in range(40)] == [n for _, n in toks]
    b = bertpy.BertTokenIndex(m, 40, cap)
    assert b.add(m.forward_tokens(ids)) == 0
    for i in range(40):
        assert same(a.doc(i), b.doc(i)), i
    for query in (texts[3], " ".join(words[200:204]), words[17]):
        qt = m.forward_tokens([np.array(m.tokenize(query)[0], np.int32)])[0]
        got = a.score_text(query)
        assert same(got, b.score(qt)) and same(got, a.score(qt))
        sub = [5, -1, 39, 5]
        assert same(a.score_text(query, sub), b.score(qt, sub))
    best = a.rerank(texts[3], np.arange(40))
    assert best[0][0] == 3 and abs(best[1][0] - toks[3][1]) < 0.01 * toks[3][1]   # every token finds itself
    # an over-long text: the whole call fails with -4 and adds nothing
    long_text = " ".join(words[i % 300] for i in range(m.n_max_tokens + 8))
    arr = bertpy.BertIndex._texts([texts[0], long_text])
    assert m.lib.bertx_mvindex_add_texts(a.mv, m.ctx, 2, 2, arr) == -4 and len(a) == 40
    # a query over 64 tokens
    long_q = " ".join(words[i % 300] for i in range(70))
    one = np.full(40, 7.5, np.float32)
    assert m.lib.bertx_mvindex_score_text(a.mv, m.ctx, long_q.encode(), None, 40, one.ctypes.data) == -4
    assert np.all(one == 7.5)
    # the 41st document over the slots that are left
    with pytest.raises(RuntimeError):
        a.add_texts([texts[20], texts[21]])
    assert len(a) == 40


# ---- 9b. the chunk boundaries of the text and host forms, bit for bit ----
def check_docs_against_the_manual_path(m, a, ids, picks):
    """Documents `picks` of store a (filled by add_texts) against a store filled by
    add(forward_tokens(.)) of those documents' ids."""
    b = bertpy.BertTokenIndex(m, len(picks), sum((len(ids[i]) + 15) // 16 * 16 for i in picks))
    assert b.add(m.forward_tokens([ids[i] for i in picks])) == 0
    for j, i in enumerate(picks):
        assert a.doc_len(i) == b.doc_len(j) == len(ids[i]), i
        assert same(a.doc(i), b.doc(j)), i


def test_add_texts_across_the_sentence_limit(tok_golden):
    """4,097 texts in one call: a device forward takes at most 4,096 sentences, so the last
    text is a chunk of its own."""
    m = bertpy.BertModel(TINY64)
    _, words = corpus_texts(tok_golden)
    W, n = len(words), 4097
    texts = [" ".join(words[(i + 97 * j) % W] for j in range(2 + i % 2)) for i in range(n)]
    ids = [np.array(m.tokenize(t)[0], np.int32) for t in texts]
    lens = [len(t) for t in ids]
    assert set(lens) == {4, 5} and sum(lens) < 2 ** 17              # the sentence limit alone cuts
    a = bertpy.BertTokenIndex(m, n, 16 * n)
    assert a.add_texts(texts) == 0
    assert len(a) == n and a.token_slots == 16 * n
    assert [a.doc_len(i) for i in range(n)] == lens
    check_docs_against_the_manual_path(m, a, ids, [0, 1, 4094, 4095, 4096])


def test_add_texts_across_the_token_limit(tok_golden):
    """Texts of 512 tokens each: 256 of them are 2^17 tokens, one device forward; the 257th
    opens the second chunk."""
    m = bertpy.BertModel(TINY64)
    _, words = corpus_texts(tok_golden)
    W, L = len(words), m.n_max_tokens
    assert L == 512
    texts = [" ".join(words[(i + 31 * j + j * j) % W] for j in range(L - 2)) for i in range(257)]
    ids = [np.array(m.tokenize(t)[0], np.int32) for t in texts]
    lens = [len(t) for t in ids]
    assert lens == [L] * 257
    assert sum(lens[:256]) <= 131072 < sum(lens[:257]) and len(lens) <= 4096   # the token limit alone cuts
    a = bertpy.BertTokenIndex(m, 257, 257 * L)
    assert a.add_texts(texts) == 0
    assert len(a) == 257 and a.token_slots == 257 * L
    assert [a.doc_len(i) for i in range(257)] == lens
    check_docs_against_the_manual_path(m, a, ids, [0, 255, 256])


def test_host_score_across_the_staging_chunk(model_of_width):
    """65,537 candidates: the host form stages 65,536 ids at a time."""
    w = 64
    ix, q = store_of(model_of_width(w), M.pack_case(w)), M.token_rows(np.random.default_rng(82), 17, w)
    n, N = len(ix), 65537
    want = ix.score(q)
    ids = (np.arange(N) % n).astype(np.int32)
    ids[65535] = ids[65536] = -1
    assert ids[65534] >= 0 and N - 65536 == 1
    got = ix.score(q, ids)
    exp = np.where(ids >= 0, want[np.maximum(ids, 0)], np.float32(-np.inf)).astype(np.float32)
    assert got.shape == (N,) and same(got, exp)


@pytest.mark.parametrize("storage", ("f16", "int8"))
def test_host_add_across_the_staging_chunk(model_of_width, storage):
    """One host add of 4,200 rows is staged 2,048 source rows at a time: documents 1 and 4
    straddle source rows 2,048 and 4,096, document 2 begins at row 2,057 of the call."""
    w = 64
    m = model_of_width(w)
    rng = np.random.default_rng(83)
    lens = [2040, 17, 2030, 1, 33, 79]
    starts = np.concatenate([[0], np.cumsum(lens)])
    assert starts[1] < 2048 < starts[2] and starts[4] < 4096 < starts[5] and starts[-1] == 4200
    docs = [M.token_rows(rng, n, w) for n in lens]
    ix = bertpy.BertTokenIndex(m, len(docs), slots_of(docs), storage=storage)
    assert ix.add(docs) == 0 and len(ix) == len(docs) and ix.token_slots == slots_of(docs)
    for i, d in enumerate(docs):                                      # alone, every document starts at source row 0
        one = bertpy.BertTokenIndex(m, 1, slots_of([d]), storage=storage)
        assert one.add([d]) == 0
        assert ix.doc_len(i) == len(d) and same(ix.doc(i), one.doc(0)), i


# ---- 10. rerank ----
@pytest.mark.parametrize("w,Lq,N,seed", M.RANKING_CASES)
def test_rerank_order_is_the_reference_order(model_of_width, w, Lq, N, seed):
    q, docs, order = M.ranking_corpus(w, Lq, N, seed)
    ix = store_of(model_of_width(w), docs)
    cand = np.random.default_rng(seed).permutation(N).astype(np.int32)
    ids, scores = ix.rerank(q, cand)
    assert np.array_equal(ids, order)
    assert np.all(np.diff(scores) < 0)
    check_scores(ix, q, ids, scores)
    ids5, scores5 = ix.rerank(q, cand, top_k=5)
    assert np.array_equal(ids5, order[:5]) and same(scores5, scores[:5])
    # equal scores come by ascending id; an id that is no document sorts last
    twice = np.array([order[1], -1, order[0], order[1]], np.int32)
    ids2, sc2 = ix.rerank(q, twice)
    assert ids2.tolist() == [order[0], order[1], order[1], -1] and np.isneginf(sc2[3])


# ---- 11. the tool ----
def test_search_tool_late_interaction(tok_golden, tmp_path):
    m = bertpy.BertModel(TINY64)
    texts, words = corpus_texts(tok_golden)
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(texts) + "\n")
    queries = [texts[3], texts[22], " ".join(words[200:204])]
    k, cand = 4, 12
    tool = [os.path.join(ROOT, "build", "bin", "search"), "-m", TINY64, "-f", str(corpus), "-k", str(k)]
    feed = "\n".join(queries) + "\nq\n"
    ix = bertpy.BertIndex(m, 40)
    assert ix.add_texts(texts) == 0
    # without -l: the lines of the index's own search, as before
    r = subprocess.run(tool, input=feed, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = []
    for query in queries:                                # one query per call, as the tool asks
        sc, ids = ix.search_texts([query], k)
        want += ["%d\t%d\t%.4f\t%s" % (j + 1, ids[0, j], sc[0, j], texts[ids[0, j]]) for j in range(k)]
    assert [ln for ln in r.stdout.splitlines() if "\t" in ln] == want
    # with -l: the index's `cand` best reranked by MaxSim
    r = subprocess.run(tool + ["-l", "-c", str(cand)], input=feed, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [ln for ln in r.stdout.splitlines() if "\t" in ln]
    mv = bertpy.BertTokenIndex(m, 40, 40 * 32)
    assert mv.add_texts(texts) == 0
    want = []
    for query in queries:
        rid, rsc = mv.rerank(query, ix.search_texts([query], cand)[1][0], top_k=k)
        want += ["%d\t%d\t%.4f\t%s" % (j + 1, rid[j], rsc[j], texts[rid[j]]) for j in range(k)]
    assert got == want
    assert got[0].split("\t")[1] == "3" and got[k].split("\t")[1] == "22"     # the planted best lines first
    # -l and -r exclude each other
    r = subprocess.run(tool + ["-l", "-r", TINY64], input="q\n", capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "usage" in r.stderr
