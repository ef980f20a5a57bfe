"""Document deletion and filtered search of the token store (bertx_mvindex_remove / _live /
_deleted, _search_filtered, _candidates_filtered, _search_pruned_filtered; bert_hip.h "Deleting
documents and filtered search").

Every comparison is exact, on ids and on score bits.  The expected result is
maxsim_mask_refs.expected: search_mask_refs.select over the admissible documents of the score
matrix that score(q, ids=None) returned before any removal (the approx matrix for the
candidates); one oracle, the fresh store of the live documents, does not use score at all."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import maxsim_mask_refs as MM
import maxsim_pruned_refs as PR
import maxsim_refs as M
import maxsim_res_refs as RR
import maxsim_search_refs as SR
import search_mask_refs as SM
import test_gpu_maxsim_res as RES
from conftest import GOLDEN, ROOT
from test_gpu_maxsim_i8 import store_of
from test_gpu_search_mask import dev, stream  # noqa: F401

pytestmark = pytest.mark.gpu

TINY64 = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
SCAN = ("f16", "int8")                   # the kinds with a full scan
ALL = ("f16", "int8", "res2", "res4")


@pytest.fixture(scope="module", autouse=True)
def _one_device():
    os.environ.pop("BERT_HOST_ONLY", None)
    os.environ["BERT_DEVICES"] = "0"


@pytest.fixture(scope="module")
def model():
    return bertpy.BertModel(TINY64)


def lens_of(n, seed):
    """Ragged lens of the suite with one-token documents and documents of exactly 16, 17 and 32
    tokens at the front."""
    lens = SR.suite_lens(n, seed)
    front = [1, 16, 17, 32, 1]
    lens[:min(n, 5)] = front[:min(n, 5)]
    return lens


_buckets = {}


def store(model, kind, w, docs, cent):
    """A store of `kind` holding docs, coded by cent: f16 and int8 directly, the residual kinds
    by the workflow of test_gpu_maxsim_res.py (an f16 twin trains the buckets, once per shape)."""
    if kind in SCAN:
        ix = store_of(model, docs, w, storage=kind)
        ix.set_centroids(cent)
        return ix
    key = (kind, w, len(cent))
    if key not in _buckets:
        _buckets[key] = RES.twin_of(model, docs, w, cent).train_residual_buckets(RR.NBITS[kind])
    return RES.res_of(model, docs, w, kind, cent, _buckets[key])


def build(model, kind, w, lens, seed, C=16):
    cent = RES.make_centroids(w, C)
    docs = RES.make_docs(w, C, lens, seed)
    return store(model, kind, w, docs, cent), docs, cent


def refill(ix, docs):
    ix.clear()
    assert ix.add(docs) == 0 and len(ix) == len(docs) and ix.live() == len(docs)


def queries_of(w, Lq, B, seed):
    rng = np.random.default_rng(1000 * seed + 10 * Lq + w)
    return [M.token_rows(rng, Lq, w) for _ in range(B)]


def score_matrix(ix, queries):
    S = np.stack([ix.score(q) for q in queries])
    S.setflags(write=False)
    return S


def approx_matrix(model, ix, cent, queries):
    """The centroid-interaction score of every (query, document): candidates(q, docs) where the
    store has at most 128 documents, else the scores of the substituted store (every row replaced
    by the centroid of its code: the contract of the candidates)."""
    N = len(ix)
    if N <= 128:
        A = MM.scatter(*ix.candidates(queries, N), N)
    else:
        codes = [ix.doc_codes(i) for i in range(N)]
        sub = store_of(model, PR.substitute(cent, codes), ix.dim, storage="int8" if ix.storage == "int8" else "f16")
        A = score_matrix(sub, queries)
    A.setflags(write=False)
    return A


def check(ix, S, A, queries, k, dead=None, allow=None, allow_arg=None):
    """search (the kinds that have it), candidates and, where n_cand covers the admissible
    documents, search_pruned against the expected selection.  allow_arg: what is passed as
    allow= when it is not the bool array itself (packed words)."""
    N, B = S.shape[1], len(queries)
    arg = allow if allow_arg is None else allow_arg
    adm = SM.admissible(N, B, dead, allow)
    want = SM.select(S, adm, k)
    if ix.storage in SCAN:
        got = ix.search(queries, k, allow=arg)
        assert SM.same(got, want), (got, want)
    if A is not None:
        for n_cand in (min(k, 128), 128):
            got = ix.candidates(queries, n_cand, allow=arg)
            assert SM.same(got, SM.select(A, adm, n_cand)), n_cand
        if adm.sum(axis=1).max() <= 128:
            got = ix.search_pruned(queries, min(k, 128), 128, allow=arg)
            assert SM.same(got, SM.select(S, adm, min(k, 128))), (got, want)
    return want


# ---- 1. remove / live / deleted / clear ----
@pytest.mark.parametrize("kind", ALL)
def test_remove_live_deleted_and_clear(model, kind):
    w, N, k = 64, 40, 12
    ix, docs, cent = build(model, kind, w, lens_of(N, 1), 11)
    lib = ix.lib
    qs = queries_of(w, 8, 3, 1)
    S, A = score_matrix(ix, qs), approx_matrix(model, ix, cent, qs)
    slots, doc5 = ix.token_slots, ix.doc(5)
    assert ix.live() == N and not ix.deleted(0, N).any()
    gone = np.array([0, 5, 5, 39, -3, N, 1000, 5], np.int32)              # out of range and repeated ids
    ix.remove(gone)
    dead = SM.tombstones(N, gone)
    assert dead.sum() == 3 and ix.live() == N - 3 and np.array_equal(ix.deleted(0, N), dead)
    assert np.array_equal(ix.deleted(5, 1), [True]) and np.array_equal(ix.deleted(38, 2), [False, True])
    assert len(ix) == N and ix.token_slots == slots                        # ids are never reused
    assert ix.doc_len(5) == len(docs[5]) and np.array_equal(ix.doc(5), doc5)
    g = np.array([1, 2], np.int32)
    for n in (0, -1):
        assert lib.bertx_mvindex_remove(ix.mv, g.ctypes.data, n) < 0
        assert lib.bertx_mvindex_remove_device(ix.mv, g.ctypes.data, n, None) < 0
    assert lib.bertx_mvindex_remove(ix.mv, None, 2) < 0 and lib.bertx_mvindex_remove(None, g.ctypes.data, 2) < 0
    out = np.full(N + 1, 9, np.uint8)
    for first, n in ((0, N + 1), (-1, 2), (N, 1), (0, 0)):
        assert lib.bertx_mvindex_deleted(ix.mv, first, n, out.ctypes.data) == -1
    assert np.all(out == 9) and lib.bertx_mvindex_live(None) < 0
    assert ix.live() == N - 3
    check(ix, S, A, qs, k, dead)
    check(ix, S, A, qs, N, dead)                                           # k beyond the live documents: fill
    for b, q in enumerate(qs):                                             # score: -inf, the neighbours unchanged
        assert SM.same((ix.score(q), 0), (MM.scores_with_deleted(S[b], np.arange(N), dead), 0))
    ix.remove(np.arange(N))
    assert ix.live() == 0
    want = check(ix, S, A, qs, 4, np.ones(N, bool))
    assert np.all(want[1] == -1)
    ix.clear()
    assert len(ix) == 0 and ix.live() == 0
    assert ix.add(docs) == 0 and ix.live() == N and not ix.deleted(0, N).any()
    check(ix, S, A, qs, k)                                                 # clear, then add, starts clean


# ---- 2. mask word boundaries ----
# every count at both widths for the kinds with a full scan; the residual kinds share the
# candidate scan and differ in the scorer alone: four of the shapes
WORD_CASES = [(kind, w, N) for kind in SCAN for w in (64, 128) for N in (1, 31, 32, 33, 64, 65, 300)] + \
             [(kind, w, N) for kind in ("res2", "res4") for w, N in ((128, 1), (64, 33), (128, 65), (64, 300))]


@pytest.mark.parametrize("kind,w,N", WORD_CASES)
def test_mask_word_boundaries(model, kind, w, N):
    rng = np.random.default_rng(100 * N + w)
    ix, docs, cent = build(model, kind, w, lens_of(N, N), N + w)
    qs = queries_of(w, 5, 2, N)
    S, A = score_matrix(ix, qs), approx_matrix(model, ix, cent, qs)
    k = min(N + 2, 128)
    first = True
    for name, ids in SM.removal_patterns(N, rng).items():
        if not first:
            refill(ix, docs)
        first = False
        ix.remove(ids)
        dead = SM.tombstones(N, ids)
        assert ix.live() == N - dead.sum(), name
        want = check(ix, S, A, qs, k, dead)
        if name == "every row":
            assert np.all(want[1] == -1) and np.all(np.isneginf(want[0]))
    # the same patterns as filters (the complement is admitted), on the clean store
    refill(ix, docs)
    for name, ids in SM.removal_patterns(N, rng).items():
        check(ix, S, A, qs, k, allow=~SM.tombstones(N, ids))


# ---- 3. wave boundaries ----
@pytest.mark.parametrize("kind", ALL)
@pytest.mark.parametrize("cap", (1, 2))
def test_wave_boundaries(model, kind, cap):
    w, N, k = 64, 128, 128
    lens = lens_of(N, 3)
    ix, docs, cent = build(model, kind, w, lens, 33)
    lib = ix.lib
    qs = queries_of(w, 8, 2, 3)
    S, A = score_matrix(ix, qs), approx_matrix(model, ix, cent, qs)
    assert lib.bertx_test_mvindex_grid(ix.mv, cap) == 0
    table, G = SR.table_of(lens)
    patterns = []
    for W in (SR.FULL_WAVES * cap, SR.CENTROID_WAVES * cap):
        patterns.append(sorted({i for _, _, i in SR.edge_ids(lens, W)}))   # first and last document of every wave
        ranges = [r for r in SR.wave_ranges(table, G, W) if r[0] < r[1]]
        assert len(ranges) == W
        dA, dB = ranges[1]
        patterns.append(list(range(dA, dB)))                               # one whole wave's range
    for n, ids in enumerate(patterns):
        if n:
            refill(ix, docs)
        ix.remove(ids)
        check(ix, S, A, qs, k, SM.tombstones(N, ids))
        assert lib.bertx_test_mvindex_last_grid(ix.mv) == cap
    refill(ix, docs)
    for ids in patterns:
        check(ix, S, A, qs, k, allow=~SM.tombstones(N, ids))
    assert lib.bertx_test_mvindex_grid(ix.mv, 0) == cap


# ---- 4. pending-lane flushes ----
@pytest.mark.parametrize("kind", ALL)
def test_pending_lane_flushes(model, kind):
    w, N, k = 64, 600, 128
    rng = np.random.default_rng(44)
    lens = rng.choice((1, 15, 16, 17), N)
    ix, docs, cent = build(model, kind, w, lens, 44)
    qs = queries_of(w, 8, 5, 4)                                            # a pass of four queries and a pass of one
    S, A = score_matrix(ix, qs), approx_matrix(model, ix, cent, qs)
    assert ix.lib.bertx_test_mvindex_grid(ix.mv, 1) == 0
    for v, (dA, dB, g) in enumerate(SR.wave_load(lens, SR.FULL_WAVES)):
        assert dB - dA > 64
        if kind in SCAN:
            assert len(SR.full_scan_flushes(g, w, kind)) >= 1              # the unmasked wave flushes mid-stream
    half = rng.random(N) < 0.5
    sparse = np.arange(N) % 61 == 0
    per_query = MM.per_query_filters(len(qs), N, rng)
    for allow in (half, sparse, per_query):
        check(ix, S, A, qs, k, allow=allow)
    gone = np.flatnonzero(rng.random(N) < 0.4)
    ix.remove(gone)
    dead = SM.tombstones(N, gone)
    for allow in (None, half, sparse, per_query):
        check(ix, S, A, qs, k, dead, allow)
    assert ix.lib.bertx_test_mvindex_last_grid(ix.mv) == 1


# ---- 5. per-query filters inside one pass; 8. both table placements ----
_shared = {}


@pytest.fixture(scope="module")
def shared(model):
    """(ix, docs, cent) by (kind, C): 100 documents of width 128, built once and never changed
    (the tests that use them filter and do not remove)."""
    def get(kind, C):
        if (kind, C) not in _shared:
            _shared[(kind, C)] = build(model, kind, 128, lens_of(100, 5), 55, C)
        return _shared[(kind, C)]
    yield get
    _shared.clear()


def placements(Lq, B, C, n_cands):
    """What bertx_test_approx_ran reports for candidate scans of B queries of Lq rows over C
    centroids (bit 0: the table in LDS, bit 1: in global memory): the launcher's rule restated.
    A pass of nq queries has ceil(Lq / 16) nq tiles; its table, C lines of 16 floats per tile
    (three tiles take a line of four), goes to LDS when it fits the 160 KiB beside the lists of
    the eight waves."""
    QT = (Lq + 15) // 16
    per, ran = 4 // QT, 0
    for b0 in range(0, B, per):
        nq = min(per, B - b0)
        line = 64 if QT * nq == 3 else 16 * QT * nq
        for n_cand in n_cands:
            lists = (8 * nq * n_cand * 8 + 15) // 16 * 16
            ran |= 1 if lists + 4 * line * C <= 160 * 1024 else 2
    return ran


@pytest.mark.parametrize("kind", ALL)
@pytest.mark.parametrize("Lq,B", ((8, 5), (32, 3), (40, 2), (64, 2)))
def test_per_query_filters_inside_one_pass(model, shared, kind, Lq, B):
    N, k = 100, 40
    rng = np.random.default_rng(10 * Lq + B)
    f = MM.per_query_filters(B, N, rng)
    words = SM.words_for(N) + 3                                            # more words than needed ...
    packed = SM.pack_bits(f, words).copy()
    packed[:, SM.words_for(N):] = 0xFFFFFFFF                               # ... and garbage beyond docs
    packed[:, SM.words_for(N) - 1] |= np.uint32(0xFFFFFFFF) << np.uint32(N % 32)
    # C 16: every table in LDS; C 1,040: a pass of three or four tiles (266 KB) reads it from global
    # memory, the last pass of Lq 8 B 5 and of Lq 32 B 3 (one query: 67 and 133 KB) from LDS
    for C in (16, 1040):
        form = placements(Lq, B, C, (k, 128))
        assert form == 1 if C == 16 else form & 2
        ix, docs, cent = shared(kind, C)
        qs = queries_of(128, Lq, B, C)
        S, A = score_matrix(ix, qs), approx_matrix(model, ix, cent, qs)
        ix.lib.bertx_test_approx_ran(1)
        check(ix, S, A, qs, k, allow=f, allow_arg=packed)
        assert ix.lib.bertx_test_approx_ran(1) == form
        check(ix, S, A, qs, k, allow=f)
        check(ix, S, A, qs, k, allow=f[0])                                 # one filter for every query
        ix.candidates(qs, 5, allow=f[0])
        assert ix.lib.bertx_test_mvindex_last_masked(ix.mv) == 1
        check(ix, S, A, qs, k)
        ix.candidates(qs, 5)
        assert ix.lib.bertx_test_mvindex_last_masked(ix.mv) == 0


@pytest.mark.parametrize("kind", ALL)
@pytest.mark.parametrize("C,form", ((16, 1), (1040, 2)))
def test_candidates_and_pruned_search_in_both_placements(model, kind, C, form):
    w, N, k = 64, 100, 20
    rng = np.random.default_rng(C)
    ix, docs, cent = build(model, kind, w, lens_of(N, 8), 88, C)
    qs = queries_of(w, 8, 4, 8)                                            # one pass of four tiles: one placement
    S, A = score_matrix(ix, qs), approx_matrix(model, ix, cent, qs)
    gone = np.flatnonzero(rng.random(N) < 0.3)
    ix.remove(gone)
    dead = SM.tombstones(N, gone)
    ix.lib.bertx_test_approx_ran(1)
    for allow in (None, rng.random(N) < 0.5, MM.per_query_filters(len(qs), N, rng)):
        check(ix, S, A, qs, k, dead, allow)
        if kind in SCAN:                                                   # n_cand covers the admissible documents
            assert SM.same(ix.search_pruned(qs, k, 128, allow=allow), ix.search(qs, k, allow=allow))
    assert ix.lib.bertx_test_approx_ran(1) == form


# ---- 6. ties ----
@pytest.mark.parametrize("kind", ALL)
def test_ties_come_by_ascending_id(model, kind):
    w, N = 64, 60
    lens = lens_of(N, 6)
    copies, gone = [3, 10, 17, 40, 47, 55], [10, 47, 20]
    cent = RES.make_centroids(w, 16)
    docs = RES.make_docs(w, 16, lens, 66)
    for i in copies:
        docs[i] = docs[copies[0]]                                          # byte-identical documents: equal score bits
    lens = np.array([len(d) for d in docs])
    ix = store(model, kind, w, docs, cent)
    assert ix.lib.bertx_test_mvindex_grid(ix.mv, 1) == 0
    table, G = SR.table_of(lens)
    for W in (SR.FULL_WAVES, SR.CENTROID_WAVES):
        ranges = SR.wave_ranges(table, G, W)
        assert len({v for v, (dA, dB) in enumerate(ranges) for i in copies if dA <= i < dB}) >= 2
    qs = [docs[3][:8].copy(), M.token_rows(np.random.default_rng(6), 8, w)]
    S, A = score_matrix(ix, qs), approx_matrix(model, ix, cent, qs)
    assert len({S[0, i].tobytes() for i in copies}) == 1
    ix.remove(gone)
    want = check(ix, S, A, qs, 10, SM.tombstones(N, gone))
    assert want[1][0, :4].tolist() == [3, 17, 40, 55]                      # the survivors, ascending


# ---- 7. a fresh store of the live documents ----
@pytest.mark.parametrize("kind", ALL)
def test_deletions_equal_a_fresh_store_of_the_live_documents(model, kind):
    w, N, k = 128, 90, 70
    rng = np.random.default_rng(7)
    ix, docs, cent = build(model, kind, w, lens_of(N, 7), 77)
    gone = np.flatnonzero(rng.random(N) < 0.35)
    dead = SM.tombstones(N, gone)
    fresh = store(model, kind, w, [docs[i] for i in np.flatnonzero(~dead)], cent)
    ix.remove(gone)
    assert ix.live() == len(fresh)
    qs = queries_of(w, 17, 3, 7)
    if kind in SCAN:
        assert SM.same(ix.search(qs, k), MM.map_live(fresh.search(qs, k), dead))
    assert SM.same(ix.search_pruned(qs, k, 128), MM.map_live(fresh.search_pruned(qs, k, 128), dead))
    assert SM.same(ix.candidates(qs, 128), MM.map_live(fresh.candidates(qs, 128), dead))


# ---- 9. score ----
@pytest.mark.parametrize("kind", ALL)
def test_score_of_deleted_ids(model, kind):
    w, N = 64, 50
    rng = np.random.default_rng(9)
    ix, docs, cent = build(model, kind, w, lens_of(N, 9), 99)
    qs = queries_of(w, 33, 2, 9)
    S = score_matrix(ix, qs)
    gone = [0, 1, 17, 31, 32, 49]
    ix.remove(gone)
    dead = SM.tombstones(N, gone)
    for b, q in enumerate(qs):
        assert SM.same((ix.score(q), 0), (MM.scores_with_deleted(S[b], np.arange(N), dead), 0))
        ids = np.array([49, 48, -1, 0, N, 2, 17, 16, 18, 2], np.int32)
        assert SM.same((ix.score(q, ids), 0), (MM.scores_with_deleted(S[b], ids, dead), 0))
    # the embedding index's ids passed straight through: a deletion made in the store alone
    emb = bertpy.BertIndex(model, N)
    rows = M.unit_rows(rng, N, 64)
    assert emb.add(rows) == 0
    _, ids = emb.search(rows[:2], N + 2)                                   # every row, then the fill
    assert sorted(ids[0].tolist()) == [-1, -1] + list(range(N))
    for b, q in enumerate(qs):
        assert SM.same((ix.score(q, ids[b]), 0), (MM.scores_with_deleted(S[b], ids[b], dead), 0))


# ---- 10. the launch rule ----
@pytest.mark.parametrize("kind", ALL)
def test_launch_rule(model, kind):
    w, N = 64, 40
    ix, docs, cent = build(model, kind, w, lens_of(N, 10), 10)
    last = lambda: ix.lib.bertx_test_mvindex_last_masked(ix.mv)       # noqa: E731
    q = queries_of(w, 8, 1, 10)
    assert last() == 0                                                     # before the first launch

    def calls(expect, allow=None):
        if kind in SCAN:
            ix.search(q, 5, allow=allow)
            assert last() == expect
        ix.candidates(q, 5, allow=allow)
        assert last() == expect
        ix.search_pruned(q, 5, 10, allow=allow)
        assert last() == (expect if allow is None else 0)                 # its last launch is the scorer: tombstones only

    calls(0)
    ix.score(q[0])
    assert last() == 0
    calls(1, allow=np.ones(N, bool))
    calls(0)
    ix.remove([N, -1])                                                     # accepted, though it names no document
    calls(1)
    ix.score(q[0])
    assert last() == 1
    assert ix.lib.bertx_test_mvindex_last_masked(None) == -1
    refill(ix, docs)
    calls(0)
    ix.score(q[0])
    assert last() == 0


# ---- 11. graph capture ----
@pytest.mark.parametrize("kind", ALL)
def test_remove_and_filtered_search_in_one_graph(model, dev, stream, kind):  # noqa: F811
    w, N, B, Lq, k = 64, 100, 5, 8, 10
    rng = np.random.default_rng(31)
    ix, docs, cent = build(model, kind, w, lens_of(N, 12), 12)
    qs = queries_of(w, Lq, B, 12)
    S = score_matrix(ix, qs)
    gone = np.array([0, 16, 99, 50, 50, -3, N], np.int32)
    dead = SM.tombstones(N, gone)
    f1, f2 = rng.random((B, N)) < 0.5, rng.random((B, N)) < 0.2
    words = SM.words_for(N)
    dq, dg, df = dev.up(np.stack(qs)), dev.up(gone), dev.up(SM.pack_bits(f1))
    ds, di, ps, pi = (dev.alloc(B * k * 4) for _ in range(4))
    hip, vp, lib = dev.hip, ctypes.c_void_p, ix.lib
    graph, ex = vp(), vp()
    assert hip.hipStreamBeginCapture(stream, 1) == 0                       # thread-local mode
    rcs = [lib.bertx_mvindex_remove_device(ix.mv, dg, len(gone), stream)]
    if kind in SCAN:
        rcs.append(lib.bertx_mvindex_search_filtered_device(ix.mv, dq, B, Lq, k, df, B, words, ds, di, stream))
    rcs.append(lib.bertx_mvindex_search_pruned_filtered_device(ix.mv, dq, B, Lq, k, 128, df, B, words, ps, pi, stream))
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0 and not any(rcs)
    assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, 0) == 0
    assert not ix.deleted(0, N).any()                                      # captured, not run
    for f in (f1, f2):
        dev.put(df, SM.pack_bits(f))                                       # the filter buffer overwritten in place
        for p, fill in ((ds, np.float32), (di, np.int32), (ps, np.float32), (pi, np.int32)):
            dev.put(p, np.full((B, k), 3, fill))
        assert hip.hipGraphLaunch(ex, stream) == 0 and hip.hipStreamSynchronize(stream) == 0
        want = MM.expected(S, k, dead, f)
        if kind in SCAN:
            assert SM.same((dev.down(ds, (B, k), np.float32), dev.down(di, (B, k), np.int32)), want)
        assert SM.same((dev.down(ps, (B, k), np.float32), dev.down(pi, (B, k), np.int32)), want)
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    assert np.array_equal(ix.deleted(0, N), dead) and ix.live() == N - 4
    # outside a graph, a shared filter on the stream
    dev.put(df, SM.pack_bits(f1[0]))
    assert lib.bertx_mvindex_candidates_filtered_device(ix.mv, dq, B, Lq, k, df, 1, words, ps, pi, stream) == 0
    assert hip.hipStreamSynchronize(stream) == 0
    got = (dev.down(ps, (B, k), np.float32), dev.down(pi, (B, k), np.int32))
    assert SM.same(got, ix.candidates(qs, k, allow=f1[0]))


# ---- 12. refusals ----
@pytest.mark.parametrize("kind", ("f16", "res2"))
def test_refusals_leave_the_outputs_untouched(model, kind):
    w, N, B, Lq, k = 64, 70, 3, 8, 5
    ix, docs, cent = build(model, kind, w, lens_of(N, 13), 13)
    lib = ix.lib
    q = np.ascontiguousarray(np.stack(queries_of(w, Lq, B, 13)))
    scores, ids = np.full((B, 129), 7.0, np.float32), np.full((B, 129), 7, np.int32)
    words = SM.words_for(N)
    f = np.full((B, words), 0xFFFFFFFF, np.uint32)
    Q, F, S, I = q.ctypes.data, f.ctypes.data, scores.ctypes.data, ids.ctypes.data

    def search(queries=Q, B_=B, k_=k, filters=F, nf=B, w_=words, s=S, i=I):
        return lib.bertx_mvindex_search_filtered(ix.mv, queries, B_, Lq, k_, filters, nf, w_, s, i)

    def cands(queries=Q, B_=B, k_=k, filters=F, nf=B, w_=words, s=S, i=I):
        return lib.bertx_mvindex_candidates_filtered(ix.mv, queries, B_, Lq, k_, filters, nf, w_, s, i)

    def pruned(queries=Q, B_=B, k_=k, filters=F, nf=B, w_=words, s=S, i=I):
        return lib.bertx_mvindex_search_pruned_filtered(ix.mv, queries, B_, Lq, k_, 20, filters, nf, w_, s, i)

    for c in (search, cands, pruned):
        assert c(queries=None) < 0 and c(s=None) < 0 and c(i=None) < 0
        assert c(filters=None) < 0                                         # a count without a pointer
        assert c(nf=0) < 0                                                 # a pointer without a count
        assert c(nf=2) < 0 and c(nf=B + 1) < 0 and c(nf=-1) < 0
        assert c(w_=words - 1) < 0 and c(w_=0) < 0
        assert c(k_=129) < 0 and c(k_=0) < 0 and c(B_=0) < 0
    assert lib.bertx_mvindex_search_filtered(None, Q, B, Lq, k, F, B, words, S, I) < 0
    if kind == "res2":
        assert search() < 0 and search(filters=None, nf=0, w_=0) < 0       # no full scan of a residual store
    assert np.all(scores == 7.0) and np.all(ids == 7)
    with pytest.raises(ValueError):
        ix.candidates(list(q), k, allow=np.ones(N + 1, bool))
    # the accepted forms next to them: (NULL, 0) is the plain call
    for c, plain in ((search, ix.search), (cands, ix.candidates)) if kind == "f16" else ((cands, ix.candidates),):
        assert c(filters=None, nf=0, w_=0) == 0
        got = (scores.reshape(-1)[:B * k].reshape(B, k), ids.reshape(-1)[:B * k].reshape(B, k))
        assert SM.same(got, plain(list(q), k))
        assert c(nf=1) == 0 and c() == 0
    assert pruned() == 0 and pruned(filters=None, nf=0, w_=0) == 0
    # a filter is not read when the store is empty: a pointer that must not be followed
    ix.clear()
    assert lib.bertx_mvindex_candidates_filtered(ix.mv, Q, B, Lq, k, ctypes.c_void_p(16), 1, 0, S, I) == 0
    assert np.all(ids.reshape(-1)[:B * k] == -1)


# ---- 13. the tool ----
def test_the_tool_drops_documents(model, tmp_path):
    texts = ["the cat sat on the mat", "a dog ran in the park", "rain fell on the town", "the town has a park"]
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(texts) + "\n")
    tool = [os.path.join(ROOT, "build", "bin", "search"), "-m", TINY64, "-f", str(corpus), "-k", "4"]
    ix = bertpy.BertTokenIndex(model, 4, 4 * 16)
    assert ix.add_texts(texts) == 0
    query = texts[1]
    before = ix.search_texts([query], 4)
    ix.remove([1, 9])
    after = ix.search_texts([query], 4)
    assert before[1][0, 0] == 1 and 1 not in after[1] and after[1][0, 3] == -1
    stdin = "%s\n:drop 1 9\n%s\n:drop 1\n:del 0\n:drop 0 2\n%s\nq\n" % (query, query, query)

    def run(args):
        r = subprocess.run(tool + args, input=stdin, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        # (the loader's own lines share stdout: the hits and the answers are kept)
        return [ln for ln in r.stdout.splitlines()
                if "dropped" in ln or "deleted" in ln or (len(ln.split("\t")) == 4 and ln.split("\t")[0].isdigit())]

    def hit_lines(scores, ids):
        return ["%d\t%d\t%.4f\t%s" % (j + 1, i, s, texts[i]) for j, (s, i) in enumerate(zip(scores, ids)) if i >= 0]

    out = run(["-l", "-a"])                                                # the full scan: the Python call's lines
    assert out[:4] == hit_lines(before[0][0], before[1][0]) and out[4] == "dropped 1"
    assert out[5:8] == hit_lines(after[0][0], after[1][0])
    assert out[8:11] == ["dropped 0", "no embedding index (-a): nothing deleted", "dropped 2"]
    assert [ln.split("\t")[1] for ln in out[11:]] == ["3"] and len(out) == 12
    out = run(["-l"])                                                      # the second stage behind the embedding index
    assert [ln for ln in out if "dropped" in ln or "deleted" in ln] == ["dropped 1", "dropped 0", "deleted 1", "dropped 2"]
    at = out.index("dropped 1")
    assert at == 4 and all(ln.split("\t")[1] != "1" for ln in out[at + 1:] if "\t" in ln)
    assert [ln.split("\t")[1] for ln in out[out.index("dropped 2") + 1:]] == ["3"]
    out = run([])                                                          # no token store: answered and ignored
    assert len([ln for ln in out if ln == "no token store: nothing dropped"]) == 3
    assert not any(ln.startswith("dropped") for ln in out)
