"""The device-resident embedding index on the GPU (bertx_index_*, search.hip): top-k
results against the float64 reference of the stored f16 rows (search_refs.py), exact
ids on planted corpora, ties, bitwise invariances, graph capture, refusals and the
text forms end to end."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import search_refs as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _one_device():
    os.environ.pop("BERT_HOST_ONLY", None)
    os.environ["BERT_DEVICES"] = "0"


_models = {}


@pytest.fixture(scope="module")
def model_of_width(tmp_path_factory):
    """A context whose n_embd is d (an index takes its width from the context): tiny64
    for 64, else a one-layer synthetic f16 model."""
    def get(d):
        if d not in _models:
            if d == 64:
                path = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
            else:
                path = str(tmp_path_factory.mktemp("w%d" % d) / "m.bin")
                hp = dict(n_vocab=256, n_max_tokens=32, n_embd=d, n_intermediate=128, n_head=d // 64, n_layer=1)
                bertpy.synthetic_model(path, hp, "f16")
            _models[d] = bertpy.BertModel(path)
        return _models[d]
    yield get
    _models.clear()


def filled(model, rows, capacity=None):
    ix = bertpy.BertIndex(model, capacity or len(rows))
    assert ix.add(rows) == 0 and len(ix) == len(rows)
    return ix


def check_all(ix, queries, scores, ids, k):
    stored = ix.rows(0, len(ix))
    ref, tol = R.ref_scores(queries, stored), R.tolerances(queries, stored)
    for b in range(len(queries)):
        R.check_topk(ref[b], scores[b], ids[b], k, tol[b])
    return ref, tol


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


def search_device(ix, dev, queries, k, stream=None):
    B = len(queries)
    dq = dev.up(np.asarray(queries, np.float32))
    ds, di = dev.alloc(B * k * 4), dev.alloc(B * k * 4)
    assert ix.lib.bertx_index_search_device(ix.idx, dq, B, k, ds, di, stream) == 0
    assert dev.hip.hipStreamSynchronize(stream) == 0 if stream else True
    if not stream:   # the index's own stream: a host-form call on it returns after everything before it
        ix.rows(0, 1)
    return dev.down(ds, (B, k), np.float32), dev.down(di, (B, k), np.int32)


RANDOM_SHAPES = [(64, 1, 1, 1), (64, 7, 3, 10), (64, 15, 1, 10), (128, 257, 16, 10), (384, 1025, 17, 64),
                 (768, 4099, 65, 10), (1024, 513, 5, 128)]


@pytest.mark.parametrize("d,N,B,k", RANDOM_SHAPES)
def test_random_rows(model_of_width, dev, d, N, B, k):
    rng = np.random.default_rng(d + N)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    ix = filled(model_of_width(d), rows)
    scores, ids = ix.search(queries, k)
    check_all(ix, queries, scores, ids, k)
    # the device forms: rows added from device memory, searched into device memory
    ix2 = bertpy.BertIndex(model_of_width(d), N)
    assert ix.lib.bertx_index_add_device(ix2.idx, dev.up(rows), N, None) == 0
    s2, i2 = search_device(ix2, dev, queries, k)
    assert np.array_equal(ix2.rows(0, N), ix.rows(0, N))
    assert np.array_equal(s2.view(np.uint32), scores.view(np.uint32)) and np.array_equal(i2, ids)


@pytest.mark.parametrize("d,N,B,k", R.PLANTED_SHAPES)
def test_planted_rows_exact_ids(model_of_width, d, N, B, k):
    rows, queries, want = R.planted(d, N, B, k)
    ix = filled(model_of_width(d), rows)
    scores, ids = ix.search(queries, k)
    check_all(ix, queries, scores, ids, k)
    assert np.array_equal(ids, want)


def test_ties_by_ascending_id(model_of_width):
    d, N = 64, 1025
    rng = np.random.default_rng(11)
    rows = R.unit_rows(rng, N, d)
    v = R.unit_rows(rng, 1, d)[0]
    for i in (3, 300, N - 1):
        rows[i] = v
    ix = filled(model_of_width(d), rows)
    scores, ids = ix.search(v[None, :], 10)
    check_all(ix, v[None, :], scores, ids, 10)
    assert list(ids[0, :3]) == [3, 300, N - 1]
    assert len(set(scores[0, :3].view(np.uint32).tolist())) == 1


def test_query_composition_invariance(model_of_width):
    d, N, k = 768, 4099, 10
    rng = np.random.default_rng(12)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 65, d)
    ix = filled(model_of_width(d), rows)
    s_all, i_all = ix.search(queries, k)
    for b in (37, 64):   # a member of the first 64-query group, and the one past it
        s1, i1 = ix.search(queries[b:b + 1], k)
        assert np.array_equal(s1[0].view(np.uint32), s_all[b].view(np.uint32)) and np.array_equal(i1[0], i_all[b])


def test_incremental_adds_and_clear(model_of_width):
    d, N, k = 128, 600, 10
    rng = np.random.default_rng(13)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 5, d)
    m = model_of_width(d)
    one = filled(m, rows)
    want = one.search(queries, k)
    ix = bertpy.BertIndex(m, N)
    assert ix.add(rows[:1]) == 0
    assert ix.add(rows[1:18]) == 1
    # a search between adds sees only the rows present
    s18, i18 = ix.search(queries, k)
    assert i18.max() < 18
    ref18 = check_all(ix, queries, s18, i18, k)[0]
    assert ref18.shape[1] == 18
    assert ix.add(rows[18:]) == 18 and len(ix) == N
    got = ix.search(queries, k)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    ix.clear()
    assert len(ix) == 0
    s0, i0 = ix.search(queries, k)
    assert np.all(i0 == -1) and np.all(np.isneginf(s0))
    assert ix.add(rows) == 0
    got = ix.search(queries, k)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


def test_subnormal_rows_are_not_flushed(model_of_width):
    d = 64
    rng = np.random.default_rng(14)
    rows = R.unit_rows(rng, 40, d) * np.float32(1e-6)   # far smaller scores than the planted row's
    rows[21] = np.float32(3e-5)                          # every entry an f16 subnormal
    q = np.full((1, d), 1.0 / np.sqrt(d), np.float32)
    ix = filled(model_of_width(d), rows)
    assert np.all(ix.rows(21, 1) == np.float32(np.float16(3e-5)))
    scores, ids = ix.search(q, 1)
    ref, tol = check_all(ix, q, scores, ids, 1)
    assert ids[0, 0] == 21 and abs(scores[0, 0] - 2.4e-4) < 1e-5 and tol[0] < 1e-8


def test_storage_bound_against_f32(model_of_width):
    d, N, k = 768, 1025, 16
    rng = np.random.default_rng(15)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 9, d)
    ix = filled(model_of_width(d), rows)
    scores, ids = ix.search(queries, k)
    _, tol = check_all(ix, queries, scores, ids, k)
    exact = queries.astype(np.float64) @ rows.astype(np.float64).T
    err = np.abs(scores - np.take_along_axis(exact, ids.astype(np.int64), axis=1))
    bound = 2.0 ** -10 + np.sqrt(d) * 2.0 ** -24 + tol.max()
    print("storage error", err.max(), "bound", bound)
    assert err.max() <= bound


def test_search_device_in_a_captured_graph(model_of_width, dev):
    d, N, B, k = 384, 1025, 17, 10
    rng = np.random.default_rng(16)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    ix = filled(model_of_width(d), rows)
    hip, vp = dev.hip, ctypes.c_void_p
    s = vp()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    eager = search_device(ix, dev, queries, k, s)
    check_all(ix, queries, eager[0], eager[1], k)
    dq = dev.up(queries)
    ds, di = dev.alloc(B * k * 4), dev.alloc(B * k * 4)
    graph, ex = vp(), vp()
    assert hip.hipStreamBeginCapture(s, 1) == 0   # thread-local mode
    rc = ix.lib.bertx_index_search_device(ix.idx, dq, B, k, ds, di, s)
    assert hip.hipStreamEndCapture(s, ctypes.byref(graph)) == 0 and rc == 0
    assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, 0) == 0
    zeros = np.zeros((B, k), np.float32)
    for _ in range(2):
        assert hip.hipMemcpy(ds, zeros.ctypes.data, zeros.nbytes, 1) == 0
        assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
        got = dev.down(ds, (B, k), np.float32), dev.down(di, (B, k), np.int32)
        assert np.array_equal(got[0].view(np.uint32), eager[0].view(np.uint32)) and np.array_equal(got[1], eager[1])
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    hip.hipStreamDestroy(s)


def test_refusals_change_nothing(model_of_width):
    d = 64
    rng = np.random.default_rng(17)
    rows, q = R.unit_rows(rng, 20, d), R.unit_rows(rng, 2, d)
    ix = filled(model_of_width(d), rows, capacity=24)
    lib = ix.lib
    before = ix.rows(0, 20)
    scores, ids = np.full((2, 129), 7.0, np.float32), np.full((2, 129), 7, np.int32)
    for B, k in ((2, 0), (2, 129), (0, 5)):
        assert lib.bertx_index_search(ix.idx, q.ctypes.data, B, k, scores.ctypes.data, ids.ctypes.data) < 0
    assert lib.bertx_index_search(None, q.ctypes.data, 2, 5, scores.ctypes.data, ids.ctypes.data) < 0
    assert np.all(scores == 7.0) and np.all(ids == 7)
    more = R.unit_rows(rng, 5, d)
    assert lib.bertx_index_add(ix.idx, more.ctypes.data, 5) < 0        # 20 + 5 > 24
    assert lib.bertx_index_add(None, more.ctypes.data, 1) < 0
    assert len(ix) == 20 and np.array_equal(ix.rows(0, 20), before)
    assert ix.add(more[:4]) == 20 and len(ix) == 24                      # what fits still does


def corpus_texts(tok_golden):
    """40 distinct four-word texts and 3 new ones, of whole words of the golden vocabulary."""
    words = [w for w in tok_golden["vocab"][104:] if w.isascii() and w.isalpha() and len(w) > 2]
    W = len(words)
    assert W > 300
    texts = [" ".join(words[j % W] for j in (3 * i + 1, 5 * i + 2, 7 * i + 3, 11 * i + 150)) for i in range(40)]
    assert len(set(texts)) == 40
    new = [" ".join(words[j] for j in js) for js in ((301, 302), (17, 310, 311, 312, 313), (320,))]
    return texts, new, words


@pytest.mark.parametrize("fmt", ["f16", "q4_0"])
@pytest.mark.parametrize("pool", ["mean", "cls"])
def test_texts_end_to_end(quant_models, tok_golden, tmp_path, fmt, pool):
    TEXTS, NEW_TEXTS, words = corpus_texts(tok_golden)
    path = quant_models[("tiny64", fmt)]
    m = bertpy.BertModel(path)
    m.set_pooling(pool)
    ix = bertpy.BertIndex(m, 64)
    assert ix.add_texts(TEXTS) == 0 and len(ix) == 40
    queries = TEXTS[3:40:8] + NEW_TEXTS
    k = 5
    scores, ids = ix.search_texts(queries, k)
    emb = m.encode(queries, batch_size=len(queries))
    check_all(ix, emb, scores, ids, k)
    # the stored rows are the encoder's rows, rounded to f16
    assert np.array_equal(ix.rows(0, 40), m.encode(TEXTS, batch_size=40).astype(np.float16).astype(np.float32))
    for j, t in enumerate(TEXTS[3:40:8]):
        assert ids[j, 0] == 3 + 8 * j and scores[j, 0] >= 1 - 2.0 ** -10
    # an over-long text: the whole call fails, nothing is added
    long_text = " ".join(words[i % 300] for i in range(m.n_max_tokens + 8))
    with pytest.raises(RuntimeError):
        ix.add_texts([TEXTS[0], long_text])
    assert len(ix) == 40
    if pool == "mean":
        # the tool on the same corpus prints the same ids
        corpus = tmp_path / "corpus.txt"
        corpus.write_text("\n".join(TEXTS) + "\n")
        r = subprocess.run([os.path.join(ROOT, "build", "bin", "search"), "-m", path, "-f", str(corpus), "-k", str(k)],
                           input="\n".join(queries) + "\nq\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        hits = [ln.split("\t") for ln in r.stdout.splitlines() if re_hit(ln)]
        assert len(hits) == len(queries) * k
        got = np.array([int(h[1]) for h in hits]).reshape(len(queries), k)
        assert np.array_equal(got, ids)
        assert all(h[3] == TEXTS[int(h[1])] for h in hits)


def re_hit(line):
    p = line.split("\t")
    return len(p) == 4 and p[0].isdigit() and p[1].isdigit()


def test_tool_refuses_empty_corpus(quant_models, tmp_path):
    empty = tmp_path / "empty.txt"
    empty.write_text("\n")
    r = subprocess.run([os.path.join(ROOT, "build", "bin", "search"), "-m", quant_models[("tiny64", "f16")], "-f",
                        str(empty)], input="", capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "no text" in r.stderr
