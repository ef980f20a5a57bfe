"""Binary storage of the embedding index on the GPU (BERTX_INDEX_BIN, search_bin.hip), the
scorer of listed rows (bertx_index_score_ids, search_rescore.hip) and the two-stage search
(bertx_index_search_rescored).  Binary scores are integers, so everything binary must
equal the numpy restatement (search_bin_refs.py) bit for bit; the scorer must reproduce
the bits of the search of its index's kind; the two-stage search must be the composition
of the two and the order of the results.  No tolerance anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import search_bin_refs as BR
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
                path = str(tmp_path_factory.mktemp("binw%d" % d) / "m.bin")
                hp = dict(n_vocab=256, n_max_tokens=32, n_embd=d, n_intermediate=128, n_head=d // 64, n_layer=1)
                bertpy.synthetic_model(path, hp, "f16")
            _models[d] = bertpy.BertModel(path)
        return _models[d]
    yield get
    _models.clear()


def make(model, kind, capacity):
    if kind == "binary":
        ix = bertpy.BertBinaryIndex(model, capacity)
        assert ix.lib.bertx_index_storage(ix.idx) == 8
        return ix
    return bertpy.BertIndex(model, capacity, storage=kind)


def filled(model, kind, rows, capacity=None):
    ix = make(model, kind, capacity or max(len(rows), 1))
    if len(rows):
        assert ix.add(rows) == 0
    assert len(ix) == len(rows)
    return ix


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """(scores, ids) pairs equal bit for bit."""
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def stored_bits(ix):
    return ix.rows_bits(0, len(ix)) if len(ix) else np.zeros((0, ix.dim // 8), np.uint8)


def check_search(ix, queries, got, k):
    """The core check: ids and score bits against the integer reference on the read-back bits."""
    ref = BR.ref_scores_bin(BR.binarize(queries), stored_bits(ix), ix.dim)
    want = BR.expected_topk(ref, k)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(bits(got[0]), bits(want[0]))
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

    def fill(self, p, shape, dtype, value):
        a = np.full(shape, value, dtype)
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0

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


def replay_twice(dev, stream, launch, outputs, want):
    """Captures launch() on `stream` into a graph and replays it twice; after each replay the
    outputs [(pointer, shape, dtype)], wiped before it, equal `want` bit for bit."""
    hip, vp = dev.hip, ctypes.c_void_p
    graph, ex = vp(), vp()
    assert hip.hipStreamBeginCapture(stream, 1) == 0   # thread-local mode
    rc = launch()
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0 and rc == 0
    assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, 0) == 0
    for _ in range(2):
        for p, shape, dtype in outputs:
            dev.fill(p, shape, dtype, 3)
        assert hip.hipGraphLaunch(ex, stream) == 0 and hip.hipStreamSynchronize(stream) == 0
        for (p, shape, dtype), w in zip(outputs, want):
            assert np.array_equal(dev.down(p, shape, dtype).view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)


WIDTHS = [64, 192, 768, 1024]


# ---- 1. the stored bits ----
@pytest.mark.parametrize("d", WIDTHS)
def test_stored_bits(model_of_width, dev, d):
    N = 150                                              # three groups of 64, the last partly filled
    rng = np.random.default_rng(d)
    rows = BR.special_rows(rng, N, d)
    m = model_of_width(d)
    ix = filled(m, "binary", rows)
    with np.errstate(invalid="ignore"):
        want = np.packbits(rows > 0, axis=1)
    assert np.array_equal(want, BR.binarize(rows))
    got = ix.rows_bits(0, N)
    assert np.array_equal(got, want)
    assert not got[1].any()                              # the all-negative row
    assert np.array_equal(ix.rows(0, N), np.unpackbits(want, axis=1)[:, :d].astype(np.float32) * 2 - 1)
    # a sub-range that starts and ends inside groups
    assert np.array_equal(ix.rows_bits(61, 70), want[61:131])
    assert np.array_equal(ix.rows(63, 2), BR.signs(want[63:65], d).astype(np.float32))
    # the device form stores the same bits
    ix2 = make(m, "binary", N)
    assert ix.lib.bertx_index_add_device(ix2.idx, dev.up(rows), N, None) == 0
    assert np.array_equal(ix2.rows_bits(0, N), want)
    # adds of 1, 15, 16, 17 and 63 + 2 rows across group boundaries equal one add
    ix3 = make(m, "binary", N)
    at = 0
    for n in (1, 15, 16, 17, 63, 2, N - 114):
        assert ix3.add(rows[at:at + n]) == at
        at += n
    assert at == N and np.array_equal(ix3.rows_bits(0, N), want)
    # rows_i8 and rows_bits on the wrong kind, and a bad range: -1, the outputs untouched
    out = np.full((2, d // 8), 5, np.uint8)
    qb, sb = np.full((2, d), 5, np.int8), np.full(2, 5.0, np.float32)
    assert ix.lib.bertx_index_rows_i8(ix.idx, 0, 2, qb.ctypes.data, sb.ctypes.data) == -1
    assert ix.lib.bertx_index_rows_bits(ix.idx, N - 1, 2, out.ctypes.data) == -1
    f16 = filled(m, "f16", rows[3:5])
    assert ix.lib.bertx_index_rows_bits(f16.idx, 0, 2, out.ctypes.data) == -1
    assert np.all(out == 5) and np.all(qb == 5) and np.all(sb == 5.0)


def test_clear_then_a_shorter_add_returns_no_stale_id(model_of_width):
    d, k = 192, 128
    rng = np.random.default_rng(5)
    rows, queries = BR.special_rows(rng, 300, d), BR.special_rows(rng, 3, d)
    ix = filled(model_of_width(d), "binary", rows)
    check_search(ix, queries, ix.search(queries, k), k)
    ix.clear()
    assert len(ix) == 0
    s0, i0 = ix.search(queries, k)
    assert np.all(i0 == -1) and np.all(np.isneginf(s0))
    # 70 rows that are the negation of the queries' signs: every stale row behind them scores higher
    few = np.tile(-queries[0], (70, 1))
    assert ix.add(few) == 0
    got = ix.search(queries, k)
    assert got[1].max() < 70 and np.all(got[1][:, 70:] == -1) and np.all(np.isneginf(got[0][:, 70:]))
    check_search(ix, queries, got, k)


# ---- 2. the search ----
@pytest.mark.parametrize("N", [0, 1, 16, 17, 64, 65, 300, 4099])
@pytest.mark.parametrize("d", WIDTHS)
def test_search_grid(model_of_width, d, N):
    rng = np.random.default_rng(1000 * d + N)
    rows = BR.special_rows(rng, N, d) if N else np.zeros((0, d), np.float32)
    queries = BR.special_rows(rng, 65, d)
    ix = filled(model_of_width(d), "binary", rows)
    rb = stored_bits(ix)
    assert np.array_equal(rb, BR.binarize(rows) if N else rb)
    ref = BR.ref_scores_bin(BR.binarize(queries), rb, d)
    for B in (1, 17, 65):
        for k in (1, 10, 128):
            got = ix.search(queries[:B], k)
            want = BR.expected_topk(ref[:B], k)
            assert np.array_equal(got[1], want[1]), (B, k)
            assert np.array_equal(bits(got[0]), bits(want[0])), (B, k)
            if N == 0 or k > N:
                assert np.all(got[1][:, N:] == -1) and np.all(np.isneginf(got[0][:, N:]))
    if N:
        print("d", d, "N", N, "distinct scores of query 0:", len(np.unique(ref[0])))
        R.check_topk(ref[0], *[a[0] for a in ix.search(queries[:1], 10)], 10, 0.0)


@pytest.mark.parametrize("d,N", [(64, 300000), (768, 66000)])
def test_search_where_a_workgroup_walks_many_groups(model_of_width, dev, d, N):
    """More 64-row groups than a scan has workgroups (at most four per CU), so a workgroup
    walks several and its prefetch ring (eight groups at d 64, two at d 768) goes round:
    the smaller indexes of the other tests give every workgroup a single group."""
    rng = np.random.default_rng(d)
    rows = rng.integers(0, 2, (N, d)).astype(np.float32) * 2 - 1
    queries = rng.integers(0, 2, (17, d)).astype(np.float32) * 2 - 1
    rows[N - 3] = queries[0]                               # the best row of query 0 in the last, partly filled group
    ix = make(model_of_width(d), "binary", N)
    assert ix.lib.bertx_index_add_device(ix.idx, dev.up(rows), N, None) == 0 and len(ix) == N
    ref = BR.ref_scores_bin(BR.binarize(queries), BR.binarize(rows), d)
    for B, k in ((1, 10), (2, 128), (17, 10)):
        got = ix.search(queries[:B], k)
        want = BR.expected_topk(ref[:B], k)
        assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0])), (B, k)
    assert ix.search(queries[:1], 1)[1][0, 0] == N - 3
    for first in (0, 64 * 1000 + 5, N - 70):
        assert np.array_equal(ix.rows_bits(first, 70), BR.binarize(rows[first:first + 70]))


def test_query_composition_invariance(model_of_width):
    d, N, k = 768, 4099, 10
    rng = np.random.default_rng(12)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 65, d)
    ix = filled(model_of_width(d), "binary", rows)
    s_all, i_all = ix.search(queries, k)
    check_search(ix, queries, (s_all, i_all), k)
    for b in (37, 64):   # a member of the first 64-query group, and the one past it
        s1, i1 = ix.search(queries[b:b + 1], k)
        assert np.array_equal(bits(s1[0]), bits(s_all[b])) and np.array_equal(i1[0], i_all[b])


def test_identical_rows_come_by_ascending_id(model_of_width):
    d, N = 192, 300
    rng = np.random.default_rng(13)
    v = R.unit_rows(rng, 1, d)
    ix = filled(model_of_width(d), "binary", np.tile(v, (N, 1)))
    queries = np.concatenate([v, R.unit_rows(rng, 2, d)])
    for k in (10, 128):
        scores, ids = ix.search(queries, k)
        assert np.array_equal(ids, np.tile(np.arange(k, dtype=np.int32), (3, 1)))
        assert np.all(scores == scores[:, :1]) and np.all(scores[0] == d)
        check_search(ix, queries, (scores, ids), k)


def test_search_device_on_a_stream_and_in_a_graph(model_of_width, dev, stream):
    d, N, B, k = 768, 1025, 17, 10
    rng = np.random.default_rng(16)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    ix = filled(model_of_width(d), "binary", rows)
    host = ix.search(queries, k)
    check_search(ix, queries, host, k)
    dq = dev.up(queries)
    ds, di = dev.alloc(B * k * 4), dev.alloc(B * k * 4)
    assert ix.lib.bertx_index_search_device(ix.idx, dq, B, k, ds, di, stream) == 0
    assert dev.hip.hipStreamSynchronize(stream) == 0
    assert same((dev.down(ds, (B, k), np.float32), dev.down(di, (B, k), np.int32)), host)
    replay_twice(dev, stream, lambda: ix.lib.bertx_index_search_device(ix.idx, dq, B, k, ds, di, stream),
                 [(ds, (B, k), np.float32), (di, (B, k), np.int32)], host)


# ---- 3. listed rows ----
KINDS = ["f16", "int8", "binary"]


@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("kind", KINDS)
def test_score_ids_reproduces_every_pair(model_of_width, kind, d):
    N, B = 100, 5
    rng = np.random.default_rng(20 + d)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    ix = filled(model_of_width(d), kind, rows)
    s_all, i_all = ix.search(queries, N)                  # every pair's score
    assert np.array_equal(np.sort(i_all, axis=1), np.tile(np.arange(N), (B, 1)))
    by_id = np.zeros((B, N), np.float32)
    np.put_along_axis(by_id, i_all.astype(np.int64), s_all, axis=1)
    ids = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int32)
    for n in (1, 15, 16, 17, 100):
        got = ix.score_ids(queries, ids[:, :n])
        assert np.array_equal(bits(got), bits(np.take_along_axis(by_id, ids[:, :n].astype(np.int64), axis=1))), n
    # ids outside the index: -inf, the others untouched by them
    odd = ids[:, :20].copy()
    odd[:, 3], odd[:, 16], odd[:, 19] = -1, N, 2 ** 31 - 1
    got = ix.score_ids(queries, odd)
    want = np.take_along_axis(by_id, np.clip(odd, 0, N - 1).astype(np.int64), axis=1)
    want[:, [3, 16, 19]] = -np.inf
    assert np.array_equal(bits(got), bits(want))
    # refusals leave the output untouched
    out = np.full((B, 129), 7.0, np.float32)
    big = np.zeros((B, 129), np.int32)
    for n in (0, 129):
        assert ix.lib.bertx_index_score_ids(ix.idx, queries.ctypes.data, B, big.ctypes.data, n, out.ctypes.data) < 0
    assert ix.lib.bertx_index_score_ids(ix.idx, queries.ctypes.data, 0, big.ctypes.data, 4, out.ctypes.data) < 0
    assert np.all(out == 7.0)


@pytest.mark.parametrize("kind", KINDS)
def test_score_ids_at_a_large_index(model_of_width, kind):
    d, N, k = 768, 4099, 128
    rng = np.random.default_rng(30)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, 65, d)
    m = model_of_width(d)
    ix = filled(m, kind, rows)
    s_top, i_top = ix.search(queries, k)
    # ids at fragment and group edges, two of one group, the last row: their scores from an index
    # of these rows alone (a score does not depend on the row's id or the row count)
    extra = np.array([0, 15, 16, N - 1, 130, 141], np.int32)
    s_x, i_x = filled(m, kind, rows[extra]).search(queries, len(extra))
    by_extra = np.zeros((65, len(extra)), np.float32)
    np.put_along_axis(by_extra, i_x.astype(np.int64), s_x, axis=1)
    ids = np.concatenate([i_top[:, :k - len(extra)], np.tile(extra, (65, 1))], axis=1)
    want = np.concatenate([s_top[:, :k - len(extra)], by_extra], axis=1)
    for B in (1, 65):
        got = ix.score_ids(queries[:B], ids[:B])
        assert np.array_equal(bits(got), bits(want[:B])), B


def test_score_ids_device_on_a_stream_and_in_a_graph(model_of_width, dev, stream):
    d, N, B, n = 192, 300, 9, 40
    rng = np.random.default_rng(31)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    m = model_of_width(d)
    ids = np.stack([rng.permutation(N)[:n] for _ in range(B)]).astype(np.int32)
    ids[:, 7] = -1
    dq, di, ds = dev.up(queries), dev.up(ids), dev.alloc(B * n * 4)
    for kind in KINDS:
        ix = filled(m, kind, rows)
        host = ix.score_ids(queries, ids)
        assert np.all(np.isneginf(host[:, 7])) and np.all(np.isfinite(np.delete(host, 7, axis=1)))
        assert ix.lib.bertx_index_score_ids_device(ix.idx, dq, B, di, n, ds, stream) == 0
        assert dev.hip.hipStreamSynchronize(stream) == 0
        assert np.array_equal(bits(dev.down(ds, (B, n), np.float32)), bits(host))
        replay_twice(dev, stream, lambda: ix.lib.bertx_index_score_ids_device(ix.idx, dq, B, di, n, ds, stream),
                     [(ds, (B, n), np.float32)], [host])


# ---- 4. the two-stage search ----
def composition(coarse, fine, queries, k, n_cand):
    """search -> score_ids -> the order of the results, in Python."""
    _, cand = coarse.search(queries, n_cand)
    return BR.select(fine.score_ids(queries, cand), cand, len(fine), k)


@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("fine_kind", ["f16", "int8"])
def test_search_rescored_is_the_composition(model_of_width, fine_kind, d):
    N, B, k = 4099, 17, 10
    rng = np.random.default_rng(40 + d)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    m = model_of_width(d)
    coarse, fine = filled(m, "binary", rows), filled(m, fine_kind, rows)
    exact = fine.search(queries, k)
    for n_cand in (10, 40, 128):
        got = coarse.search_rescored(queries, k, fine, n_cand)
        assert same(got, composition(coarse, fine, queries, k, n_cand)), n_cand
        shared = np.mean([len(set(got[1][b]) & set(exact[1][b])) for b in range(B)])
        print("d", d, fine_kind, "n_cand", n_cand, "ids shared with the full", fine_kind, "search:", shared, "of", k)
    assert same(coarse.search_rescored(queries, k, fine), coarse.search_rescored(queries, k, fine, 40))   # the default, 4 k


@pytest.mark.parametrize("fine_kind", ["f16", "int8"])
def test_search_rescored_over_every_row_is_the_fine_search(model_of_width, fine_kind):
    d, N, B, k = 192, 100, 261, 10                         # B: two chunks of the staged queries
    rng = np.random.default_rng(41)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    m = model_of_width(d)
    coarse, fine = filled(m, "binary", rows), filled(m, fine_kind, rows)
    assert same(coarse.search_rescored(queries, k, fine, 128), fine.search(queries, k))
    # any kind may be the coarse one
    assert same(filled(m, "int8", rows).search_rescored(queries, k, fine, 128), fine.search(queries, k))


@pytest.mark.parametrize("d,N,B,k", R.PLANTED_SHAPES)
def test_search_rescored_finds_the_planted_rows(model_of_width, d, N, B, k):
    rows, queries, want = R.planted(d, N, B, k)
    m = model_of_width(d)
    coarse = filled(m, "binary", rows)
    for fine_kind in ("f16", "int8"):
        fine = filled(m, fine_kind, rows)
        got = coarse.search_rescored(queries, k, fine, 4 * k)
        assert same(got, fine.search(queries, k)), fine_kind
        assert np.array_equal(got[1], want)


def test_search_rescored_with_a_shorter_fine_index(model_of_width):
    d, N, B, k = 192, 300, 5, 10
    rng = np.random.default_rng(42)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    m = model_of_width(d)
    coarse, fine = filled(m, "binary", rows), filled(m, "f16", rows[:40], capacity=N)
    full = coarse.search_rescored(queries, k, fine, 128)
    assert same(full, composition(coarse, fine, queries, k, 128)) and full[1].max() < 40 and full[1].min() >= 0
    got = coarse.search_rescored(queries, k, fine, 40)
    assert same(got, composition(coarse, fine, queries, k, 40))
    assert got[1].max() < 40
    held = (coarse.search(queries, 40)[1] < 40).sum(axis=1)
    assert held.max() < k                                  # (3 .. 6 here) fewer than k candidates that fine holds
    for b in range(B):
        n = min(k, held[b])
        assert np.all(got[1][b, :n] >= 0) and np.all(got[1][b, n:] == -1) and np.all(np.isneginf(got[0][b, n:]))


def test_search_rescored_refusals(model_of_width, capfd):
    rng = np.random.default_rng(43)
    rows64, rows192, q = R.unit_rows(rng, 50, 64), R.unit_rows(rng, 50, 192), R.unit_rows(rng, 2, 64)
    coarse, fine = filled(model_of_width(64), "binary", rows64), filled(model_of_width(64), "int8", rows64)
    wide = filled(model_of_width(192), "f16", rows192)
    lib = coarse.lib
    scores, ids = np.full((2, 128), 7.0, np.float32), np.full((2, 128), 7, np.int32)

    def call(c, f, k, n_cand):
        return lib.bertx_index_search_rescored(c.idx, f.idx, q.ctypes.data, 2, k, n_cand, scores.ctypes.data, ids.ctypes.data)

    capfd.readouterr()
    assert call(coarse, wide, 5, 20) == -1
    assert "do not match" in capfd.readouterr().err
    assert call(coarse, coarse, 5, 20) == -1
    assert "same index" in capfd.readouterr().err
    assert call(coarse, fine, 21, 20) == -1               # n_cand < k
    assert call(coarse, fine, 5, 129) == -1
    assert call(coarse, fine, 0, 20) == -1
    assert np.all(scores == 7.0) and np.all(ids == 7)
    with pytest.raises(RuntimeError):
        coarse.search_rescored(q, 5, fine, 4)
    assert call(coarse, fine, 5, 20) == 0 and np.all(ids[:, :5] >= 0)


def test_search_rescored_device_on_a_stream_and_in_a_graph(model_of_width, dev, stream):
    d, N, B, k, n_cand = 768, 1025, 17, 10, 40
    rng = np.random.default_rng(44)
    rows, queries = R.unit_rows(rng, N, d), R.unit_rows(rng, B, d)
    m = model_of_width(d)
    coarse, fine = filled(m, "binary", rows), filled(m, "int8", rows)
    host = coarse.search_rescored(queries, k, fine, n_cand)
    assert same(host, composition(coarse, fine, queries, k, n_cand))
    dq = dev.up(queries)
    ds, di = dev.alloc(B * k * 4), dev.alloc(B * k * 4)

    def launch():
        return coarse.lib.bertx_index_search_rescored_device(coarse.idx, fine.idx, dq, B, k, n_cand, ds, di, stream)

    assert launch() == 0 and dev.hip.hipStreamSynchronize(stream) == 0
    assert same((dev.down(ds, (B, k), np.float32), dev.down(di, (B, k), np.int32)), host)
    replay_twice(dev, stream, launch, [(ds, (B, k), np.float32), (di, (B, k), np.int32)], host)


# ---- 5. texts and the tool ----
def re_hit(line):
    p = line.split("\t")
    return len(p) == 4 and p[0].isdigit() and p[1].isdigit()


def test_texts_and_the_tool(tok_golden, tmp_path):
    words = [w for w in tok_golden["vocab"][104:] if w.isascii() and w.isalpha() and len(w) > 2]
    W = len(words)
    texts = [" ".join(words[j % W] for j in (3 * i + 1, 5 * i + 2, 7 * i + 3, 11 * i + 150)) for i in range(40)]
    queries = texts[3:40:8] + [" ".join(words[j] for j in (301, 302)), words[320]]
    path = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
    m = bertpy.BertModel(path)
    k = 5
    coarse, fine = bertpy.BertBinaryIndex(m, 64), bertpy.BertIndex(m, 64, storage="int8")
    assert coarse.add_texts(texts) == 0 and fine.add_texts(texts) == 0 and len(coarse) == len(fine) == 40
    emb = m.encode(texts, batch_size=40)
    assert np.array_equal(coarse.rows_bits(0, 40), BR.binarize(emb))
    qemb = m.encode(queries, batch_size=len(queries))
    ham = coarse.search_texts(queries, k)
    check_search(coarse, qemb, ham, k)
    got = coarse.search_rescored_texts(queries, k, fine)
    assert same(got, composition(coarse, fine, qemb, k, 20))
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(texts) + "\n")
    tool = [os.path.join(ROOT, "build", "bin", "search"), "-m", path, "-f", str(corpus), "-k", str(k)]
    stdin = "\n".join(queries) + "\nq\n"

    def hits(args):
        r = subprocess.run(tool + args, input=stdin, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        h = [ln.split("\t") for ln in r.stdout.splitlines() if re_hit(ln)]
        assert len(h) == len(queries) * k and all(x[3] == texts[int(x[1])] for x in h)
        return (np.array([int(x[1]) for x in h]).reshape(len(queries), k), np.array([x[2] for x in h]).reshape(len(queries), k))

    ids, printed = hits(["-s", "binary", "-R", "int8"])
    assert np.array_equal(ids, got[1])
    assert np.array_equal(printed, np.array([["%.4f" % s for s in row] for row in got[0]]))
    ids, printed = hits(["-s", "binary"])                  # the Hamming scores themselves
    assert np.array_equal(ids, ham[1])
    assert np.array_equal(printed, np.array([["%.4f" % s for s in row] for row in ham[0]]))
    for bad in (["-R", "int8"], ["-s", "int8", "-R", "f16"], ["-s", "binary", "-B", "20"], ["-s", "f16", "-B", "20"],
                ["-s", "binary", "-R", "int8", "-B", "4"], ["-s", "binary", "-R", "int8", "-B", "129"]):
        r = subprocess.run(tool + bad, input="q\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "usage" in r.stderr, bad
