"""Full-scan MaxSim top-k over the token store (bertx_mvindex_search*, maxsim_search.hip).
The reference of every assertion is the existing scorer: per query, taken alone,
ix.score over every document, ordered by (-score, id) with (-inf, -1) fill
(maxsim_search_refs.expected).  The search must return the same score bits and the same
ids; no tolerance is involved anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import maxsim_refs as M
import maxsim_search_refs as SR
from conftest import GOLDEN, ROOT
from test_gpu_maxsim_i8 import DeviceArrays, same, slots_of, store_of

pytestmark = pytest.mark.gpu

TINY64 = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
STORAGES = ("f16", "int8")
DOC_LENS = (1, 15, 16, 17, 33, 100)


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


def make_docs(w, n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.choice(DOC_LENS, n)
    rows = M.token_rows(rng, int(lens.sum()), w) if n else np.zeros((0, w), np.float32)
    return np.split(rows, np.cumsum(lens)[:-1]) if n else []


def make_queries(w, Lq, B, seed=5):
    rng = np.random.default_rng(1000 * seed + 10 * Lq + w)
    return [M.token_rows(rng, Lq, w) for _ in range(B)]


_stores = {}


@pytest.fixture(scope="module")
def stores(model):
    """Stores by (storage, w, n): built once, never changed."""
    def get(storage, w, n):
        key = (storage, w, n)
        if key not in _stores:
            docs = make_docs(w, n, 7 * w + n)
            if n:
                _stores[key] = store_of(model, docs, w, storage=storage)
            else:
                _stores[key] = bertpy.BertTokenIndex(model, 4, 64, width=w, storage=storage)
        return _stores[key]
    yield get
    _stores.clear()


def check(ix, queries, k):
    want_s, want_i = SR.expected(ix, queries, k)
    got_s, got_i = ix.search(queries, k)
    assert got_i.dtype == np.int32 and np.array_equal(got_i, want_i), (got_i, want_i)
    assert same(got_s, want_s)
    return got_s, got_i


# (Lq, B, k): every Lq of 1, 16, 17, 32, 33, 64 (1, 2, 3 and 4 tiles), every B of 1, 2, 3, 4,
# 5, 9 (a full pass, an odd remainder, several passes for each packing factor) and every k
# of 1, 10, 64, 65, 128
COMBOS = [(1, 9, 10), (16, 5, 128), (16, 4, 1), (17, 3, 65), (32, 5, 64), (32, 2, 128), (32, 1, 10), (33, 2, 1),
          (33, 3, 10), (64, 2, 10), (64, 1, 65), (1, 1, 64), (16, 9, 10)]
# (w, documents): 130 documents leave some waves of the grid without a document; about 5,000
# at width 64 give every wave of a full grid documents, with range boundaries inside and
# between documents
SHAPES = [(64, 5000), (64, 130), (192, 130), (768, 130)]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("w,n", SHAPES)
def test_search_equals_the_scorer(stores, storage, w, n):
    ix = stores(storage, w, n)
    for Lq, B, k in (COMBOS if n == 130 and w == 192 or n == 5000 else COMBOS[::3]):
        check(ix, make_queries(w, Lq, B), k)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("k", (10, 128))
def test_document_counts_around_k(model, storage, k):
    w = 192
    for n in (0, 1, 3, k - 1, k, k + 1):
        docs = make_docs(w, n, 31 * n + k)
        ix = bertpy.BertTokenIndex(model, max(n, 1), max(slots_of(docs), 16), width=w, storage=storage)
        if n:
            assert ix.add(docs) == 0
        s, i = check(ix, make_queries(w, 17, 3), k)
        assert np.all(i[:, min(n, k):] == -1) and np.all(np.isneginf(s[:, min(n, k):]))
        assert np.all(i[:, :min(n, k)] >= 0)


@pytest.mark.parametrize("storage", STORAGES)
def test_ties_come_by_ascending_id(model, storage):
    """One one-token document planted at six neighbouring ids (at about three groups per
    wave, some of them share a wave's range) and at three ids far apart (other waves, other
    workgroups); every query row is that token, so the copies tie for the best score."""
    w, n = 64, 5000
    docs = make_docs(w, n, 7 * w + n)
    v = M.token_rows(np.random.default_rng(3), 1, w)
    planted = [100, 101, 102, 103, 104, 105, 2000, 4000, 4999]
    for p in planted:
        docs[p] = v
    ix = store_of(model, docs, w, storage=storage)
    for Lq in (1, 17):
        q = np.repeat(v, Lq, axis=0)
        for k in (4, 9, 10, 128):
            s, i = check(ix, [q, make_queries(w, Lq, 1)[0]], k)
            m = min(k, len(planted))
            assert i[0, :m].tolist() == planted[:m]                            # k cuts the run: the lower ids survive
            assert len(set(s[0, :m].view(np.uint32).tolist())) == 1
            if k > len(planted):
                assert s[0, len(planted)] < s[0, 0]


@pytest.mark.parametrize("storage", STORAGES)
def test_a_query_is_independent_of_the_call(stores, storage):
    ix = stores(storage, 192, 130)
    for Lq, B in ((16, 9), (32, 5), (64, 3)):
        qs = make_queries(192, Lq, B, seed=9)
        s, i = ix.search(qs, 128)
        for b in range(B):
            s1, i1 = ix.search([qs[b]], 128)                                   # alone
            assert same(s1[0], s[b]) and np.array_equal(i1[0], i[b])
        sr, ir = ix.search(qs[::-1], 128)                                      # at every other position
        assert same(sr[::-1], s) and np.array_equal(ir[::-1], i)
        for k in (1, 10, 65):                                                  # another k: a prefix
            sk, ik = ix.search(qs, k)
            assert same(sk, s[:, :k]) and np.array_equal(ik, i[:, :k])


@pytest.mark.parametrize("storage", STORAGES)
def test_zero_row_padding(stores, storage):
    ix = stores(storage, 192, 130)
    q5 = make_queries(192, 5, 1)[0]
    want_s, want_i = SR.topk(ix.score(q5), 10)
    for Lq in (5, 16, 17, 64):
        s, i = ix.search(SR.pad_rows(q5, Lq), 10)
        assert same(s[0], want_s) and np.array_equal(i[0], want_i), Lq
    # a ragged list is padded by the binding
    s, i = ix.search([q5, make_queries(192, 33, 1)[0]], 10)
    assert same(s[0], want_s) and np.array_equal(i[0], want_i)
    with pytest.raises(ValueError):
        ix.search(np.zeros((65, 192), np.float32), 10)


@pytest.mark.parametrize("storage", STORAGES)
def test_clear_leaves_no_stale_id(model, storage):
    w = 64
    docs = make_docs(w, 130, 1)
    ix = store_of(model, docs, w, storage=storage)
    qs = make_queries(w, 17, 2)
    check(ix, qs, 128)
    ix.clear()
    s, i = check(ix, qs, 10)
    assert np.all(i == -1)
    assert ix.add(make_docs(w, 20, 2)) == 0
    s, i = check(ix, qs, 128)
    assert i.max() == 19 and np.all(i[:, 20:] == -1)


@pytest.mark.parametrize("storage", STORAGES)
def test_search_device_and_captured_graph(model, dev, storage):
    w, Lq, B, k = 192, 32, 3, 10
    docs = make_docs(w, 130, 4)
    ix = store_of(model, docs, w, storage=storage, extra_docs=2, extra_slots=64)
    qs = make_queries(w, Lq, B)
    want_s, want_i = SR.expected(ix, qs, k)
    hip, vp, lib = dev.hip, ctypes.c_void_p, model.lib
    s = vp()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    dq, ds, di = dev.up(np.stack(qs)), dev.alloc(B * k * 4), dev.alloc(B * k * 4)
    assert lib.bertx_mvindex_search_device(ix.mv, dq, B, Lq, k, ds, di, s) == 0
    assert hip.hipStreamSynchronize(s) == 0
    assert same(dev.down(ds, (B, k), np.float32), want_s) and np.array_equal(dev.down(di, (B, k), np.int32), want_i)
    graph, ex = vp(), vp()
    assert hip.hipStreamBeginCapture(s, 1) == 0   # thread-local mode
    rc = lib.bertx_mvindex_search_device(ix.mv, dq, B, Lq, k, ds, di, s)
    assert hip.hipStreamEndCapture(s, ctypes.byref(graph)) == 0 and rc == 0
    assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, 0) == 0
    zeros = np.zeros(B * k, np.int32)
    for round_ in range(3):
        if round_ == 2:                           # a later add: a copy of query 0's rows would win, were it seen
            assert ix.add([qs[0]]) == len(docs)
        for p in (ds, di):
            assert hip.hipMemcpy(p, zeros.ctypes.data, zeros.nbytes, 1) == 0
        assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
        assert same(dev.down(ds, (B, k), np.float32), want_s)
        assert np.array_equal(dev.down(di, (B, k), np.int32), want_i)
    assert ix.search(qs, k)[1][0, 0] == len(docs)                              # the direct call sees it
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    hip.hipStreamDestroy(s)


@pytest.mark.parametrize("storage", STORAGES)
def test_refusals_leave_the_outputs_untouched(stores, model, storage):
    ix, lib = stores(storage, 64, 130), model.lib
    q = np.stack(make_queries(64, 64, 2) + [np.zeros((64, 64), np.float32)])   # room for Lq 65 to read
    nan_bits = np.uint32(0x7fc01234)
    for B, Lq, k in ((1, 16, 0), (1, 16, 129), (1, 0, 10), (1, 65, 10), (0, 16, 10), (-1, 16, 10)):
        s = np.full(2 * 129, nan_bits, np.uint32)
        i = np.full(2 * 129, nan_bits, np.uint32)
        assert lib.bertx_mvindex_search(ix.mv, q.ctypes.data, B, Lq, k, s.ctypes.data, i.ctypes.data) < 0
        assert np.all(s == nan_bits) and np.all(i == nan_bits)
    s = np.full(10, nan_bits, np.uint32)
    assert lib.bertx_mvindex_search(ix.mv, None, 1, 16, 10, s.ctypes.data, s.ctypes.data) < 0
    assert lib.bertx_mvindex_search(ix.mv, q.ctypes.data, 1, 16, 10, None, s.ctypes.data) < 0
    assert lib.bertx_mvindex_search(ix.mv, q.ctypes.data, 1, 16, 10, s.ctypes.data, None) < 0
    assert lib.bertx_mvindex_search_device(ix.mv, None, 1, 16, 10, None, None, None) < 0
    assert np.all(s == nan_bits)


def corpus_words(tok_golden):
    return [w for w in tok_golden["vocab"][104:] if w.isascii() and w.isalpha() and len(w) > 2]


def corpus_texts(words, n):
    W = len(words)
    return [" ".join(words[(7 * i + 13 * j + j * j) % W] for j in range(3 + (5 * i) % 28)) for i in range(n)]


@pytest.mark.parametrize("storage", STORAGES)
def test_search_texts_equals_score_text(model, tok_golden, storage):
    words = corpus_words(tok_golden)
    texts = corpus_texts(words, 40)
    ix = bertpy.BertTokenIndex(model, 40, 40 * 48, storage=storage)
    assert ix.add_texts(texts) == 0
    queries = [texts[3], " ".join(words[200:204]), words[5], texts[22]]        # ragged: 3 .. 30 tokens
    for k in (3, 64):
        s, i = ix.search_texts(queries, k)
        for b, q in enumerate(queries):
            ws, wi = SR.topk(ix.score_text(q), k)
            assert same(s[b], ws) and np.array_equal(i[b], wi), (b, k)
    assert i[0, 0] == 3 and i[3, 0] == 22                                      # every token finds itself
    # one query of 70 tokens fails the whole call
    long_q = " ".join(words[j] for j in range(70))
    assert len(model.tokenize(long_q)[0]) > 64
    nan_bits = np.uint32(0x7fc01234)
    s, i = np.full(3 * 5, nan_bits, np.uint32), np.full(3 * 5, nan_bits, np.uint32)
    rc = model.lib.bertx_mvindex_search_texts(ix.mv, model.ctx, 2, 3, bertpy.BertIndex._texts([texts[0], long_q, texts[1]]),
                                              5, s.ctypes.data, i.ctypes.data)
    assert rc == -4 and np.all(s == nan_bits) and np.all(i == nan_bits)


@pytest.fixture(scope="module")
def colbert_model(lib, tmp_path_factory):
    import colbert_refs as CR
    return CR.make_proj_models(lib, GOLDEN, str(tmp_path_factory.mktemp("proj")))[("tiny32", "f16")]


COLBERT_TEXTS = ["stone river, bridge. water!", "plain words without any marks", "one, two, three.",
                 "a.b,c;d (e) [f] stone", "river water bridge stone river", "the stone bridge over the river.",
                 "a, b; c!", "one two three four five six seven", "water under the bridge", "marks and words, again"]


@pytest.mark.parametrize("storage", STORAGES)
def test_search_texts_colbert_equals_score_text_colbert(colbert_model, storage):
    c = bertpy.BertModel(colbert_model)
    ix = bertpy.BertTokenIndex(c, 16, 16 * 32, width=c.proj_width, storage=storage)
    assert ix.add_texts(COLBERT_TEXTS, colbert=32) == 0
    queries = ["stone bridge", "one two", "marks, words"]
    for k in (2, 16):
        s, i = ix.search_texts(queries, k, colbert=32)
        for b, q in enumerate(queries):
            ws, wi = SR.topk(ix.score_text(q, colbert=32), k)
            assert same(s[b], ws) and np.array_equal(i[b], wi), (b, k)
    out = np.zeros(4, np.float32)
    texts = bertpy.BertIndex._texts(queries)
    L = c.lib
    assert L.bertx_mvindex_search_texts_colbert(ix.mv, c.ctx, 2, 3, texts, 65, 1, out.ctypes.data, out.ctypes.data) == -1
    plain = bertpy.BertModel(TINY64)
    assert L.bertx_mvindex_search_texts_colbert(ix.mv, plain.ctx, 2, 3, texts, 32, 1, out.ctypes.data, out.ctypes.data) == -6


def check_rows_alone(ix, queries, k, colbert=None):
    """1,025 queries in one call are two forwards (1,024 per forward): the rows on both sides
    of the cut, and the first, are the bits of the same query searched alone."""
    assert len(queries) == 1025
    s, i = ix.search_texts(queries, k, colbert=colbert)
    assert s.shape == i.shape == (1025, k)
    for r in (0, 1023, 1024):
        s1, i1 = ix.search_texts([queries[r]], k, colbert=colbert)
        assert same(s[r], s1[0]) and np.array_equal(i[r], i1[0]), r
    return s, i


@pytest.mark.parametrize("storage", STORAGES)
def test_search_texts_across_the_query_chunk(model, tok_golden, storage):
    words = corpus_words(tok_golden)
    W = len(words)
    ix = bertpy.BertTokenIndex(model, 20, 20 * 48, storage=storage)
    assert ix.add_texts(corpus_texts(words, 20)) == 0
    # 1 .. 30 words: the first forward pads to 32 rows per query, the second, query 1024 alone, to 7
    queries = [" ".join(words[(3 * i + 11 * j) % W] for j in range(1 + i % 30)) for i in range(1025)]
    lens = [len(model.tokenize(q)[0]) for q in queries]
    assert max(lens[:1024]) == 32 and lens[1024] == 7 and lens[1023] == 6 and lens[0] == 3
    s, i = check_rows_alone(ix, queries, 3)
    assert np.all(i >= 0) and np.all(i < 20)


@pytest.mark.parametrize("storage", STORAGES)
def test_search_texts_colbert_across_the_query_chunk(colbert_model, storage):
    c = bertpy.BertModel(colbert_model)
    ix = bertpy.BertTokenIndex(c, 20, 20 * 32, width=c.proj_width, storage=storage)
    assert ix.add_texts(COLBERT_TEXTS + [t + " " + u for t, u in zip(COLBERT_TEXTS, COLBERT_TEXTS[1:] + COLBERT_TEXTS[:1])],
                        colbert=32) == 0 and len(ix) == 20
    vocab = ["stone", "river", "bridge", "water", "plain", "words", "marks", "one", "two", "three", "a,", "b."]
    queries = [" ".join(vocab[(i + 5 * j + i // 12) % 12] for j in range(1 + i % 7)) for i in range(1025)]
    s, i = check_rows_alone(ix, queries, 3, colbert=32)
    assert np.all(i >= 0) and np.all(i < 20)


def tool_lines(args, queries):
    r = subprocess.run([os.path.join(ROOT, "build", "bin", "search")] + args, input="\n".join(queries) + "\nq\n",
                       capture_output=True, text=True, timeout=120)
    return r, [ln for ln in r.stdout.splitlines() if "\t" in ln]


def test_search_tool_full_scan(model, colbert_model, tmp_path):
    """search -l -a and search -L MODEL -a on a ten-line corpus print the ids and scores of
    the Python call; -a with -c, and -a without a token store, are usage errors."""
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(COLBERT_TEXTS) + "\n")
    queries = ["stone bridge", "one two", "marks, words"]
    k = 3
    base = ["-m", TINY64, "-f", str(corpus), "-k", str(k)]
    r, got = tool_lines(base + ["-l", "-a"], queries)
    assert r.returncode == 0, r.stderr
    ix = bertpy.BertTokenIndex(model, 10, 10 * 32)
    assert ix.add_texts(COLBERT_TEXTS) == 0
    s, i = ix.search_texts(queries, k)
    want = ["%d\t%d\t%.4f\t%s" % (j + 1, i[b, j], s[b, j], COLBERT_TEXTS[i[b, j]]) for b in range(3) for j in range(k)]
    assert got == want
    r, got = tool_lines(base + ["-L", colbert_model, "-a", "-S", "int8"], queries)
    assert r.returncode == 0, r.stderr
    c = bertpy.BertModel(colbert_model)
    cx = bertpy.BertTokenIndex(c, 10, 10 * 192, width=c.proj_width, storage="int8")
    assert cx.add_texts(COLBERT_TEXTS, colbert=min(180, c.n_max_tokens)) == 0
    s, i = cx.search_texts(queries, k, colbert=32)
    want = ["%d\t%d\t%.4f\t%s" % (j + 1, i[b, j], s[b, j], COLBERT_TEXTS[i[b, j]]) for b in range(3) for j in range(k)]
    assert got == want
    for bad in (["-l", "-a", "-c", "5"], ["-a"], ["-r", TINY64, "-a"]):
        r, _ = tool_lines(base + bad, [])
        assert r.returncode == 2 and "usage" in r.stderr, bad


@pytest.mark.parametrize("storage", (0, 1))
def test_bench_hook(model, storage):
    us = ctypes.c_float(0)
    assert model.lib.bertx_bench_maxsim_search(64, 300, 0, 32, 2, 10, storage, 2, ctypes.byref(us)) == 0
    assert us.value > 0
    assert model.lib.bertx_bench_maxsim_search(64, 300, 0, 32, 0, 10, storage, 2, ctypes.byref(us)) < 0
