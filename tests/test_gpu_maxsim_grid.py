"""The token store's scans with many documents per wave (maxsim.hip, maxsim_i8.hip,
maxsim_res.hip, maxsim_search.hip, maxsim_approx.hip).  The scans size their grids by the
device's CU count, so at a test's store a wave sees one to four documents; a search over a
million documents gives it hundreds.  bertx_test_mvindex_grid caps the workgroups of one
store's scans, and a store of 1,200 documents (2,957 groups) under caps of 1, 2, 5 and 33
workgroups then runs what production runs: the mid-stream flushes of the pending scores,
the second and later chunks of codes, documents that follow one another inside a ring pass
at every width, lists that take more than k offers, the scorers' second and later
candidates per wave, a second selection level of one list.  maxsim_search_refs.py restates
what a wave of such a grid sees, and test_cpu_maxsim_search.py pins it for these shapes.

Every expected value comes from the uncapped scorer (or the uncapped call) and is computed
before the cap is set; every comparison is on ids and score bits."""
import contextlib
import os

import numpy as np
import pytest

import bertpy
import maxsim_i8_refs as R8
import maxsim_pruned_refs as PR
import maxsim_refs as M
import maxsim_res_refs as RR
import maxsim_search_refs as SR
from conftest import GOLDEN
from test_gpu_maxsim import f16_of
from test_gpu_maxsim_i8 import same, store_of
from test_gpu_maxsim_pruned import make_centroids
from test_gpu_maxsim_res import make_centroids as res_centroids, near_centroids, res_of, twin_of
from test_gpu_maxsim_search import make_queries

pytestmark = pytest.mark.gpu

TINY64 = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
STORAGES = ("f16", "int8")
KINDS = ("res2", "res4")
LENS = SR.grid_lens()
N = len(LENS)
CAPS = (1, 2, 5, 33)
RES_C = 48


@pytest.fixture(scope="module", autouse=True)
def _one_device():
    os.environ.pop("BERT_HOST_ONLY", None)
    os.environ["BERT_DEVICES"] = "0"


@pytest.fixture(scope="module")
def model():
    return bertpy.BertModel(TINY64)


def set_cap(ix, cap):
    return ix.lib.bertx_test_mvindex_grid(ix.mv, cap)


def last_grid(ix):
    return ix.lib.bertx_test_mvindex_last_grid(ix.mv)


@contextlib.contextmanager
def capped(ix, cap):
    """The store's scans under `cap` workgroups; uncapped before and after."""
    assert set_cap(ix, cap) == 0
    try:
        yield
    finally:
        assert set_cap(ix, 0) == cap


def ran_grid(ix, cap):
    """The scan just launched took the cap's workgroups; uncapped, its own rule's, which lie above every cap."""
    g = last_grid(ix)
    return g == cap if cap else g > max(CAPS)


# the documents per width, the stores per (storage, width), the coded stores with their
# substituted twins per (storage, width, C), the residual stores per (kind, width): built once
_docs, _stores, _coded, _res = {}, {}, {}, {}


def docs_of(w):
    if w not in _docs:
        rows = M.token_rows(np.random.default_rng(7 * w + N), int(LENS.sum()), w)
        _docs[w] = np.split(rows, np.cumsum(LENS)[:-1])
    return _docs[w]


@pytest.fixture(scope="module")
def stores(model):
    def get(storage, w):
        if (storage, w) not in _stores:
            _stores[(storage, w)] = store_of(model, docs_of(w), w, storage=storage)
        return _stores[(storage, w)]
    yield get
    _stores.clear()
    _docs.clear()


@pytest.fixture(scope="module")
def coded(model):
    """(ix, sub): a store with C centroids and the uncapped store of its rows' centroids (PR.substitute)."""
    def get(storage, w, C):
        key = (storage, w, C)
        if key not in _coded:
            ix = store_of(model, docs_of(w), w, storage=storage)
            cent = make_centroids(w, C)
            ix.set_centroids(cent)
            sub = store_of(model, PR.substitute(cent, [ix.doc_codes(i) for i in range(N)]), w, storage=storage)
            _coded[key] = (ix, sub)
        return _coded[key]
    yield get
    _coded.clear()


@pytest.fixture(scope="module")
def residual(model):
    """(ix, cent): a residual store of documents near RES_C centroids, its buckets trained on the f16 twin."""
    def get(kind, w):
        if (kind, w) not in _res:
            cent = res_centroids(w, RES_C)
            rng = np.random.default_rng(9 * w + N)
            docs = [near_centroids(rng, cent, int(n)) for n in LENS]
            twin = twin_of(model, docs, w, cent)
            _res[(kind, w)] = (res_of(model, docs, w, kind, cent, twin.train_residual_buckets(RR.NBITS[kind])), cent)
        return _res[(kind, w)]
    yield get
    _res.clear()


def natural_grids(lib):
    """The uncapped workgroups of the scorer over all documents, the full scan and the centroid
    scan of this store where the LDS leaves four workgroups per CU (width 64)."""
    cus = lib.bertx_test_cu_count()
    G = SR.table_of(LENS)[1]
    return min(4 * cus, (N + 3) // 4), SR.natural_waves(G, 4, cus) // 4, SR.natural_waves(G, 8, cus) // 8


# ---- 1. the hook ----
@pytest.mark.parametrize("storage", STORAGES)
def test_hook_semantics(model, coded, storage):
    ix, sub = coded(storage, 64, 16)
    nat_score, nat_search, nat_cand = natural_grids(model.lib)
    qs = make_queries(64, 17, 2)
    k, n_cand = 10, 32
    nat_rerank = n_cand // 4                                               # the pruned search's last scan: the scorer over n_cand ids

    def run(grids):
        out = [ix.score(qs[0])]
        assert last_grid(ix) == grids[0]
        out += ix.search(qs, k)
        assert last_grid(ix) == grids[1]
        out += ix.candidates(qs, n_cand)
        assert last_grid(ix) == grids[2]
        out += ix.search_pruned(qs, k, n_cand)
        assert last_grid(ix) == grids[3]
        return out

    def equal(a, b):
        return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))

    other, _ = coded(storage, 64, 1040)
    try:
        assert set_cap(ix, 0) == 0
        base = run((nat_score, nat_search, nat_cand, nat_rerank))
        before = 0
        for cap in CAPS + (nat_search + 7,):                                   # the last one lies above every natural grid
            assert set_cap(ix, cap) == before
            before = cap
            assert equal(run((min(cap, nat_score), min(cap, nat_search), min(cap, nat_cand), min(cap, nat_rerank))), base)
        assert set_cap(ix, -1) == -1 and set_cap(ix, -2 ** 31) == -1           # refused: the cap stays
        ix.score(qs[0])
        assert last_grid(ix) == nat_score
        assert set_cap(ix, 3) == before and set_cap(ix, -1) == -1
        ix.score(qs[0])
        assert last_grid(ix) == 3
        assert set_cap(ix, 0) == 3
        assert equal(run((nat_score, nat_search, nat_cand, nat_rerank)), base)
        # the cap is the store's own
        assert set_cap(ix, 2) == 0 and set_cap(other, 0) == 0
        other.score(qs[0])
        assert last_grid(other) == nat_score
        assert set_cap(ix, 0) == 2
    finally:                                                               # the stores are shared: leave them uncapped
        set_cap(ix, 0)
        set_cap(other, 0)


# ---- 2. the scorers ----
def store_and_query(stores, residual, storage, w):
    if storage in KINDS:
        ix, cent = residual(storage, w)
        return ix, lambda Lq: near_centroids(np.random.default_rng(50 + w + Lq), cent, Lq)
    return stores(storage, w), lambda Lq: make_queries(w, Lq, 1)[0]


@pytest.mark.parametrize("w", (64, 192, 768))
@pytest.mark.parametrize("storage", STORAGES + KINDS)
def test_scorers_under_a_cap(stores, residual, storage, w):
    ix, query = store_and_query(stores, residual, storage, w)
    rng = np.random.default_rng(w)
    ids = np.concatenate([[5, 5, -1, N, 2 ** 31 - 1, 0, N - 1, 7, 600, 7, -2 ** 31], rng.integers(0, N, 40)]).astype(np.int32)
    good = (ids >= 0) & (ids < N)
    for Lq in (1, 17, 64):
        q = query(Lq)
        assert set_cap(ix, 0) == 0
        want_all, want_ids = ix.score(q), ix.score(q, ids)
        assert same(want_ids[good], want_all[ids[good]]) and np.all(np.isneginf(want_ids[~good]))
        assert np.all(np.isfinite(want_all)) and len(set(want_all.tolist())) > N // 2
        for cap in (1, 5):
            with capped(ix, cap):
                got_all = ix.score(q)
                assert last_grid(ix) == cap
                got_ids = ix.score(q, ids)
                assert last_grid(ix) == cap
            assert same(got_all, want_all), (Lq, cap)
            assert same(got_ids, want_ids), (Lq, cap)


def test_capped_f16_scorer_against_numpy(stores):
    """One workgroup scores all 1,200 documents at width 768 with four query tiles: within
    score_tol of the float64 MaxSim of the stored values, as test_gpu_maxsim.py holds the uncapped scorer."""
    w, Lq = 768, 64
    ix = stores("f16", w)
    q = make_queries(w, Lq, 1)[0]
    q16 = f16_of(ix, q)
    ref = np.array([M.maxsim(q16, ix.doc(i)) for i in range(N)])
    with capped(ix, 1):
        got = ix.score(q)
        assert last_grid(ix) == 1
    err = np.abs(got.astype(np.float64) - ref)
    print("worst |score - float64 MaxSim| / score_tol under one workgroup: %.3f" % (err.max() / M.score_tol(Lq, w)))
    assert err.max() <= M.score_tol(Lq, w), (int(err.argmax()), err.max())


def test_capped_int8_scorer_against_numpy(stores):
    """The same for the int8 store, which test_gpu_maxsim_i8.py holds to the numpy restatement bit for bit."""
    w, Lq = 768, 64
    ix = stores("int8", w)
    q = make_queries(w, Lq, 1)[0]
    qp = R8.pack(q)
    ref = np.array([R8.score(qp, R8.pack(d)) for d in docs_of(w)], np.float32)
    with capped(ix, 1):
        got = ix.score(q)
        assert last_grid(ix) == 1
    assert same(got, ref), np.flatnonzero(got != ref)[:8]


# ---- 3. the full scan ----
# (Lq, B, k): 1 .. 4 tiles, 1 .. 4 queries per pass, a remainder pass, k of 1, 10, 64, 65, 128
SEARCH_COMBOS = [(1, 4, 128), (16, 5, 10), (17, 2, 65), (33, 1, 1), (64, 1, 128), (32, 3, 64)]


@pytest.mark.parametrize("w", (64, 192, 768))
@pytest.mark.parametrize("storage", STORAGES)
def test_full_scan_under_caps(stores, storage, w):
    ix = stores(storage, w)
    assert set_cap(ix, 0) == 0
    cases = [(make_queries(w, Lq, B), k) for Lq, B, k in SEARCH_COMBOS]
    wants = [SR.expected(ix, qs, k) for qs, k in cases]                     # the uncapped scorer
    for cap in CAPS + (0,):
        with capped(ix, cap) if cap else contextlib.nullcontext():
            for (qs, k), (want_s, want_i) in zip(cases, wants):
                got_s, got_i = ix.search(qs, k)
                assert ran_grid(ix, cap), (cap, last_grid(ix))
                assert np.array_equal(got_i, want_i), (cap, len(qs[0]), len(qs), k)
                assert same(got_s, want_s), (cap, len(qs[0]), len(qs), k)


# ---- 4. planted documents at the edges of a wave's run ----
@pytest.mark.parametrize("cap", (1, 2))
@pytest.mark.parametrize("w", (64, 768))
@pytest.mark.parametrize("storage", STORAGES)
def test_planted_documents_at_the_edges(model, storage, w, cap):
    """The first and the last document of every wave's range, one at a time, replaced by a
    one-token document that is the query's single row: it comes first, and the rest is the
    scorer's.  (Where the replaced document was longer the later documents move up; where the
    planted ids then lie is pinned by test_cpu_maxsim_search.py.)"""
    v = M.token_rows(np.random.default_rng(3), 1, w)
    edges = SR.edge_ids(LENS, SR.FULL_WAVES * cap)
    assert len(edges) == 8 * cap
    for wave, side, p in edges:
        docs = list(docs_of(w))
        docs[p] = v
        ix = store_of(model, docs, w, storage=storage)
        want_s, want_i = SR.expected(ix, [v], 128)
        assert want_i[0, 0] == p and want_s[0, 0] > want_s[0, 1]
        with capped(ix, cap):
            for k in (1, 128):
                got_s, got_i = ix.search([v], k)
                assert last_grid(ix) == cap
                assert got_i[0, 0] == p, (wave, side, p, k)
                assert np.array_equal(got_i, want_i[:, :k]) and same(got_s, want_s[:, :k]), (wave, side, p, k)


# ---- 5. ties on the two sides of a flush ----
@pytest.mark.parametrize("w", (64, 192))
@pytest.mark.parametrize("storage", STORAGES)
def test_ties_across_a_flush(model, storage, w):
    """Nine one-token copies of one document: in the second of a single workgroup's four waves
    three are offered before its first mid-stream flush, three before its second, one behind
    it (SR.tie_ids; pinned on the CPU), and one each lies in the first and the last wave."""
    ids = SR.tie_ids(LENS, SR.FULL_WAVES, w, storage)
    v = M.token_rows(np.random.default_rng(3), 1, w)
    docs = list(docs_of(w))
    for p in ids:
        docs[p] = v
    ix = store_of(model, docs, w, storage=storage)
    planted = sorted(ids)
    for Lq in (1, 17):
        qs = [np.repeat(v, Lq, axis=0), make_queries(w, Lq, 1)[0]]
        wants = {k: SR.expected(ix, qs, k) for k in (4, 9, 10, 128)}
        for cap in (1, 2):
            with capped(ix, cap):
                for k, (want_s, want_i) in wants.items():
                    s, i = ix.search(qs, k)
                    assert last_grid(ix) == cap
                    assert np.array_equal(i, want_i) and same(s, want_s), (Lq, cap, k)
                    m = min(k, len(planted))
                    assert i[0, :m].tolist() == planted[:m]                 # k cuts the run: the lower ids survive
                    assert len(set(s[0, :m].view(np.uint32).tolist())) == 1
                    if k > len(planted):
                        assert s[0, len(planted)] < s[0, 0]


# ---- 6. the centroid scan ----
# (Lq, B, n_cand)
CAND_COMBOS = [(1, 4, 128), (16, 9, 10), (17, 2, 1), (33, 1, 10), (64, 1, 128)]


def test_capped_centroid_scan_waves_take_every_path():
    """What caps 1 and 2 give a centroid-scan wave (the predicates of maxsim_search_refs.py)."""
    for cap in (1, 2):
        load = SR.wave_load(LENS, SR.CENTROID_WAVES * cap)
        assert all(SR.code_chunks(g) >= 3 for dA, dB, g in load)
        assert any(SR.closes_on_chunk_end(g) for dA, dB, g in load) and any(SR.spans_chunks(g) for dA, dB, g in load)
        # a flush at 64 pending: every wave of 64 documents or more, which at cap 2 is every wave but the first (62)
        flushing = [len(SR.centroid_scan_flushes(g)) >= 1 for dA, dB, g in load]
        assert flushing == [dB - dA >= 64 for dA, dB, g in load] and flushing.count(False) == cap - 1


@pytest.mark.parametrize("C", (16, 1040))
@pytest.mark.parametrize("w", (64, 192))
@pytest.mark.parametrize("storage", STORAGES)
def test_centroid_scan_under_caps(model, coded, storage, w, C):
    lib = model.lib
    ix, sub = coded(storage, w, C)
    assert set_cap(ix, 0) == 0 and set_cap(sub, 0) == 0
    cases = [(make_queries(w, Lq, B), n_cand) for Lq, B, n_cand in CAND_COMBOS]
    wants = [SR.expected(sub, qs, n_cand) for qs, n_cand in cases]          # the uncapped scorer over the substituted store
    forms = 0
    for cap in (1, 2, 33, 0):
        with capped(ix, cap) if cap else contextlib.nullcontext():
            for (qs, n_cand), (want_s, want_i) in zip(cases, wants):
                lib.bertx_test_approx_ran(1)
                got_s, got_i = ix.candidates(qs, n_cand)
                ran = lib.bertx_test_approx_ran(0)
                assert ran_grid(ix, cap), (cap, last_grid(ix))
                assert got_i.dtype == np.int32 and np.array_equal(got_i, want_i), (cap, len(qs[0]), len(qs), n_cand)
                assert same(got_s, want_s), (cap, len(qs[0]), len(qs), n_cand)
                Lq = len(qs[0])
                if C == 16:                                                 # the table beside the lists in LDS
                    assert ran == 1
                elif (Lq + 15) // 16 * min(len(qs), 4 // ((Lq + 15) // 16)) == 4:
                    assert ran & 2                                          # four tiles of 1,040 centroids never fit
                forms |= ran
    assert forms == (1 if C == 16 else 3)


# ---- 7. the pruned search, residual stores included ----
@pytest.mark.parametrize("w", (64, 192))
@pytest.mark.parametrize("storage", STORAGES + KINDS)
def test_pruned_search_under_caps(coded, residual, storage, w):
    if storage in KINDS:
        ix, cent = residual(storage, w)
        rng = np.random.default_rng(90 + w)
        queries = lambda Lq, B: [near_centroids(rng, cent, Lq) for _ in range(B)]   # noqa: E731
    else:
        ix = coded(storage, w, 16)[0]
        queries = lambda Lq, B: make_queries(w, Lq, B, seed=6)                     # noqa: E731
    for Lq, B, k, n_cand in ((17, 3, 10, 32), (64, 2, 128, 128)):
        qs = queries(Lq, B)
        assert set_cap(ix, 0) == 0
        want_s, want_i = ix.search_pruned(qs, k, n_cand)
        assert np.all(want_i >= 0)
        for cap in (1, 33):
            with capped(ix, cap):
                got_s, got_i = ix.search_pruned(qs, k, n_cand)
                assert last_grid(ix) == min(cap, n_cand // 4)              # its last scan: the scorer over n_cand ids
                cs, ci = ix.candidates(qs, n_cand)
                assert last_grid(ix) == cap
                exact = [ix.score(q, ci[b]) for b, q in enumerate(qs)]
            assert np.array_equal(got_i, want_i) and same(got_s, want_s), (Lq, cap)
            for b in range(B):                                             # and still its own candidates, scored and ordered
                comp_s, comp_i = PR.compose(exact[b], ci[b], k)
                assert np.array_equal(got_i[b], comp_i) and same(got_s[b], comp_s), (Lq, cap, b)
