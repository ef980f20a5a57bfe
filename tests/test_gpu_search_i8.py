"""The int8 embedding index on the GPU (bertx_index_create_ex(..., BERTX_INDEX_I8),
search.hip).  An int8 score is an exact integer sum times two f32 scales, so the device
must equal the numpy restatement (search_i8_refs.py) bit for bit: the stored bytes and
scales equal quantize(rows), and a search equals expected_topk(ref_scores_i8(...)) of
the read-back bytes and the numpy-quantized queries.  No tolerance anywhere but in the
storage-error test, whose bound is the contract's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import search_i8_refs as Q
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
                path = str(tmp_path_factory.mktemp("i8w%d" % d) / "m.bin")
                hp = dict(n_vocab=256, n_max_tokens=32, n_embd=d, n_intermediate=128, n_head=d // 64, n_layer=1)
                bertpy.synthetic_model(path, hp, "f16")
            _models[d] = bertpy.BertModel(path)
        return _models[d]
    yield get
    _models.clear()


def filled(model, rows, capacity=None):
    ix = bertpy.BertIndex(model, capacity or len(rows), storage="int8")
    assert ix.storage == "int8" and ix.lib.bertx_index_storage(ix.idx) == 1
    assert ix.add(rows) == 0 and len(ix) == len(rows)
    return ix


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """(scores, ids) pairs equal bit for bit."""
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def check_all(ix, queries, scores, ids, k):
    """The core check: against the numpy reference on the index's own bytes."""
    rq, rs = ix.rows_i8(0, len(ix)) if len(ix) else (np.zeros((0, ix.dim), np.int8), np.zeros(0, np.float32))
    qq, qs = Q.quantize(queries)
    ref = Q.ref_scores_i8(qq, qs, rq, rs)
    want = Q.expected_topk(ref, k)
    assert np.array_equal(ids, want[1])
    assert np.array_equal(bits(scores), bits(want[0]))
    for b in range(len(ref)):
        R.check_topk(ref[b], scores[b], ids[b], k, 0.0)
    return ref


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


# ---- 1. the quantizer ----
QUANT_SHAPES = [(64, 1), (64, 15), (64, 17), (192, 257), (320, 33), (768, 4099), (1024, 513)]


@pytest.mark.parametrize("d,N", QUANT_SHAPES)
def test_quantizer_bytes_and_scales(model_of_width, dev, d, N):
    rng = np.random.default_rng(7 * d + N)
    rows = R.unit_rows(rng, N, d) * rng.uniform(0.25, 4.0, (N, 1)).astype(np.float32)
    special = {}
    special["zero"] = N // 2
    rows[special["zero"]] = 0.0
    if N >= 15:
        special["spike"], special["first"], special["last"] = 3, 9, N - 2
        rows[3] = 0.0
        rows[3, d // 3] = -5.0                      # one spike: every other byte is 0
        rows[9, 0] = 3.0 * np.abs(rows[9]).max()    # amax at element 0
        rows[N - 2, d - 1] = -3.0 * np.abs(rows[N - 2]).max()   # amax at element d - 1
    ix = filled(model_of_width(d), rows)
    q, s = ix.rows_i8(0, N)
    wq, ws = Q.quantize(rows)
    assert np.array_equal(q, wq)
    assert np.array_equal(bits(s), bits(ws))
    assert s[special["zero"]] == 0.0 and not q[special["zero"]].any()
    if N >= 15:
        assert q[3, d // 3] == -127 and np.count_nonzero(q[3]) == 1
        assert q[9, 0] == 127 and q[N - 2, d - 1] == -127
    # rows(): the dequantized values, one f32 multiply
    assert np.array_equal(bits(ix.rows(0, N)), bits(q.astype(np.float32) * s[:, None]))
    # a sub-range that starts and ends inside groups
    if N > 20:
        q2, s2 = ix.rows_i8(5, 14)
        assert np.array_equal(q2, wq[5:19]) and np.array_equal(bits(s2), bits(ws[5:19]))
    # the device form stores the same bytes
    ix2 = bertpy.BertIndex(model_of_width(d), N, storage="int8")
    assert ix.lib.bertx_index_add_device(ix2.idx, dev.up(rows), N, None) == 0
    q3, s3 = ix2.rows_i8(0, N)
    assert np.array_equal(q3, wq) and np.array_equal(bits(s3), bits(ws))


# ---- 2. random rows ----
RANDOM_SHAPES = [(64, 1, 1, 1), (64, 7, 3, 10), (64, 15, 1, 10), (192, 257, 16, 10), (320, 1025, 17, 64),
                 (768, 4099, 65, 10), (1024, 513, 5, 128)]


@pytest.mark.parametrize("d,N,B,k", RANDOM_SHAPES)
def test_random_rows(model_of_width, dev, d, N, B, k):
    rng = np.random.default_rng(d + N)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    ix = filled(model_of_width(d), rows)
    got = ix.search(queries, k)
    check_all(ix, queries, got[0], got[1], k)
    # the device forms: rows added from device memory, searched into device memory
    ix2 = bertpy.BertIndex(model_of_width(d), N, storage="int8")
    assert ix.lib.bertx_index_add_device(ix2.idx, dev.up(rows), N, None) == 0
    assert same(search_device(ix2, dev, queries, k), got)


# ---- 3. planted rows ----
@pytest.mark.parametrize("d,N,B,k", R.PLANTED_SHAPES)
def test_planted_rows_exact_ids(model_of_width, d, N, B, k):
    rows, queries, want = R.planted(d, N, B, k)
    ix = filled(model_of_width(d), rows)
    scores, ids = ix.search(queries, k)
    check_all(ix, queries, scores, ids, k)
    assert np.array_equal(ids, want)


# ---- 4. ties ----
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
    assert len(set(bits(scores[0, :3]).tolist())) == 1


# ---- 5. composition ----
def test_query_composition_invariance(model_of_width):
    d, N, k = 768, 4099, 10
    rng = np.random.default_rng(12)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 65, d)
    ix = filled(model_of_width(d), rows)
    s_all, i_all = ix.search(queries, k)
    for b in (37, 64):   # a member of the first 64-query group, and the one past it
        s1, i1 = ix.search(queries[b:b + 1], k)
        assert np.array_equal(bits(s1[0]), bits(s_all[b])) and np.array_equal(i1[0], i_all[b])


# ---- 6. incremental adds ----
def test_incremental_adds_and_clear(model_of_width):
    d, N, k = 192, 600, 10
    rng = np.random.default_rng(13)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 5, d)
    m = model_of_width(d)
    one = filled(m, rows)
    want = one.search(queries, k)
    check_all(one, queries, want[0], want[1], k)
    ix = bertpy.BertIndex(m, N, storage="int8")
    assert ix.add(rows[:1]) == 0
    assert ix.add(rows[1:18]) == 1
    # a search between adds sees only the rows present, with the bits one add of them gives
    got18 = ix.search(queries, k)
    assert got18[1].max() < 18
    assert check_all(ix, queries, got18[0], got18[1], k).shape[1] == 18
    assert same(got18, filled(m, rows[:18]).search(queries, k))
    assert ix.add(rows[18:]) == 18 and len(ix) == N
    assert same(ix.search(queries, k), want)
    assert np.array_equal(ix.rows_i8(0, N)[0], one.rows_i8(0, N)[0])
    ix.clear()
    assert len(ix) == 0
    s0, i0 = ix.search(queries, k)
    assert np.all(i0 == -1) and np.all(np.isneginf(s0))
    # the stale bytes and scales past the row count are never offered: after a clear,
    # 5 rows scaled up 1000 times less than what lies behind them
    few = rows[100:105] * np.float32(1e-3)
    assert ix.add(few) == 0
    got5 = ix.search(queries, k)
    assert got5[1].max() < 5 and np.all(got5[1][:, 5:] == -1)
    check_all(ix, queries, got5[0], got5[1], k)
    ix.clear()
    assert ix.add(rows) == 0
    assert same(ix.search(queries, k), want)


# ---- 7. storage error ----
def test_storage_error_within_the_bound(model_of_width):
    d, N, k = 768, 1025, 16
    rng = np.random.default_rng(15)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 9, d)
    ix = filled(model_of_width(d), rows)
    scores, ids = ix.search(queries, k)
    check_all(ix, queries, scores, ids, k)
    _, rs = ix.rows_i8(0, N)
    _, qs = Q.quantize(queries)
    exact = queries.astype(np.float64) @ rows.astype(np.float64).T
    worst = 0.0
    for b in range(len(queries)):
        for j in range(k):
            i = int(ids[b, j])
            err = abs(float(scores[b, j]) - exact[b, i])
            bound = Q.error_bound(queries[b], rows[i], qs[b], rs[i]) + 3 * 2.0 ** -24 * abs(float(scores[b, j]))
            worst = max(worst, err / bound)
            assert err <= bound, (b, j, err, bound)
    print("worst storage error / bound", worst)


# ---- 8. captured graph ----
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
        assert same((dev.down(ds, (B, k), np.float32), dev.down(di, (B, k), np.int32)), eager)
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    hip.hipStreamDestroy(s)


# ---- 9. refusals ----
def test_refusals_change_nothing(model_of_width):
    d = 64
    rng = np.random.default_rng(17)
    rows, q = R.unit_rows(rng, 20, d), R.unit_rows(rng, 2, d)
    m = model_of_width(d)
    ix = filled(m, rows, capacity=24)
    lib = ix.lib
    before = ix.rows_i8(0, 20)
    scores, ids = np.full((2, 129), 7.0, np.float32), np.full((2, 129), 7, np.int32)
    for B, k in ((2, 0), (2, 129), (0, 5)):
        assert lib.bertx_index_search(ix.idx, q.ctypes.data, B, k, scores.ctypes.data, ids.ctypes.data) < 0
    assert np.all(scores == 7.0) and np.all(ids == 7)
    more = R.unit_rows(rng, 5, d)
    assert lib.bertx_index_add(ix.idx, more.ctypes.data, 5) < 0        # 20 + 5 > 24
    after = ix.rows_i8(0, 20)
    assert len(ix) == 20 and np.array_equal(after[0], before[0]) and np.array_equal(bits(after[1]), bits(before[1]))
    assert ix.add(more[:4]) == 20 and len(ix) == 24                      # what fits still does
    # rows_i8: a bad range, and an f16 index, with the outputs untouched
    qb, sb = np.full((2, d), 5, np.int8), np.full(2, 5.0, np.float32)
    assert lib.bertx_index_rows_i8(ix.idx, 23, 2, qb.ctypes.data, sb.ctypes.data) == -1
    f16 = bertpy.BertIndex(m, 24)
    assert f16.storage == "f16" and lib.bertx_index_storage(f16.idx) == 0
    assert f16.add(rows) == 0
    assert lib.bertx_index_rows_i8(f16.idx, 0, 2, qb.ctypes.data, sb.ctypes.data) == -1
    assert np.all(qb == 5) and np.all(sb == 5.0)
    with pytest.raises(RuntimeError):
        f16.rows_i8(0, 2)
    assert not lib.bertx_index_create_ex(m.ctx, 0, 24, 2)


def test_create_ex_f16_is_create(model_of_width):
    d, N, k = 128, 600, 10
    rng = np.random.default_rng(18)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 5, d)
    m = model_of_width(d)
    a = bertpy.BertIndex(m, N, storage="f16")        # bertx_index_create_ex(..., 0)
    b = bertpy.BertIndex.__new__(bertpy.BertIndex)   # bertx_index_create
    b.model, b.lib, b.storage = m, m.lib, "f16"
    b.idx = m.lib.bertx_index_create(m.ctx, 0, N)
    assert b.idx
    b.dim, b.capacity = d, N
    assert a.add(rows) == 0 and b.add(rows) == 0
    assert np.array_equal(bits(a.rows(0, N)), bits(b.rows(0, N)))
    assert same(a.search(queries, k), b.search(queries, k))


# ---- 10. texts end to end ----
def corpus_texts(tok_golden):
    """40 distinct four-word texts and 3 new ones, of whole words of the golden vocabulary."""
    words = [w for w in tok_golden["vocab"][104:] if w.isascii() and w.isalpha() and len(w) > 2]
    W = len(words)
    assert W > 300
    texts = [" ".join(words[j % W] for j in (3 * i + 1, 5 * i + 2, 7 * i + 3, 11 * i + 150)) for i in range(40)]
    assert len(set(texts)) == 40
    new = [" ".join(words[j] for j in js) for js in ((301, 302), (17, 310, 311, 312, 313), (320,))]
    return texts, new, words


def re_hit(line):
    p = line.split("\t")
    return len(p) == 4 and p[0].isdigit() and p[1].isdigit()


@pytest.mark.parametrize("fmt", ["f16", "q4_0"])
@pytest.mark.parametrize("pool", ["mean", "cls"])
def test_texts_end_to_end(quant_models, tok_golden, tmp_path, fmt, pool):
    TEXTS, NEW_TEXTS, words = corpus_texts(tok_golden)
    path = quant_models[("tiny64", fmt)]
    m = bertpy.BertModel(path)
    m.set_pooling(pool)
    ix = bertpy.BertIndex(m, 64, storage="int8")
    assert ix.add_texts(TEXTS) == 0 and len(ix) == 40
    queries = TEXTS[3:40:8] + NEW_TEXTS
    k = 5
    scores, ids = ix.search_texts(queries, k)
    check_all(ix, m.encode(queries, batch_size=len(queries)), scores, ids, k)
    # the stored bytes are the encoder's rows, quantized
    q, s = ix.rows_i8(0, 40)
    wq, ws = Q.quantize(m.encode(TEXTS, batch_size=40))
    assert np.array_equal(q, wq) and np.array_equal(bits(s), bits(ws))
    # an over-long text: the whole call fails, nothing is added
    long_text = " ".join(words[i % 300] for i in range(m.n_max_tokens + 8))
    with pytest.raises(RuntimeError):
        ix.add_texts([TEXTS[0], long_text])
    assert len(ix) == 40
    if pool == "mean":
        # the tool on the same corpus prints the same ids
        corpus = tmp_path / "corpus.txt"
        corpus.write_text("\n".join(TEXTS) + "\n")
        tool = [os.path.join(ROOT, "build", "bin", "search"), "-m", path, "-f", str(corpus), "-k", str(k)]
        r = subprocess.run(tool + ["-s", "int8"], input="\n".join(queries) + "\nq\n", capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        hits = [ln.split("\t") for ln in r.stdout.splitlines() if re_hit(ln)]
        assert len(hits) == len(queries) * k
        got = np.array([int(h[1]) for h in hits]).reshape(len(queries), k)
        assert np.array_equal(got, ids)
        assert all(h[3] == TEXTS[int(h[1])] for h in hits)
        if fmt == "f16":
            r = subprocess.run(tool + ["-s", "bogus"], input="q\n", capture_output=True, text=True, timeout=120)
            assert r.returncode != 0 and "usage" in r.stderr
