"""Centroid codes and the pruned MaxSim search of the token store (bertx_mvindex_set_centroids,
_train_centroids, _candidates*, _search_pruned*; maxsim_codes.hip, maxsim_approx.hip).  Every
reference is built from entries that existed before: a row's code is what the full-scan
search over a store of the centroids returns for it, a candidate list is the full-scan search
over the store with every row replaced by its centroid, and the pruned search is candidates,
then the scorer, then the (score, id) order.  Every comparison is on bits."""
import ctypes
import os

import numpy as np
import pytest

import bertpy
import maxsim_pruned_refs as PR
import maxsim_refs as M
import maxsim_search_refs as SR
from conftest import GOLDEN
from test_gpu_maxsim_i8 import DeviceArrays, same, slots_of, store_of
from test_gpu_maxsim_search import COLBERT_TEXTS, colbert_model, corpus_texts, corpus_words, tool_lines  # noqa: F401

pytestmark = pytest.mark.gpu

TINY64 = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
STORAGES = ("f16", "int8")
DOC_LENS = (1, 15, 16, 17, 33, 100)
SHAPES = [(64, 5000), (64, 130), (192, 130), (768, 130)]


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


def make_centroids(w, C, seed=0):
    """C token rows; centroid 5 repeats centroid 2 (the lower index must win)."""
    cent = M.token_rows(np.random.default_rng(31 * w + C + seed), C, w)
    cent[5] = cent[2]
    return cent


def centroid_store(model, cent, storage):
    """S_c of the contract: a store whose documents are the centroids, one row each."""
    return store_of(model, [c[None, :] for c in cent], cent.shape[1], storage=storage)


def codes_by_search(ix, S_c):
    """Per document of ix the ids S_c.search returns for its rows, each row a query of its own."""
    rows = [ix.doc(i) for i in range(len(ix))]
    flat = np.concatenate(rows)
    ids = S_c.search([r[None, :] for r in flat], 1)[1][:, 0]
    return np.split(ids, np.cumsum([len(r) for r in rows])[:-1])


def assert_codes(ix, S_c):
    want = codes_by_search(ix, S_c)
    got = [ix.doc_codes(i) for i in range(len(ix))]
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g.dtype == np.uint16 and np.array_equal(g.astype(np.int64), w_.astype(np.int64)), (i, g, w_)
    return got


# ---- 1. codes ----
_small = {}


@pytest.fixture(scope="module")
def small_docs():
    """130 documents per width, one of them with a zero row."""
    def get(w):
        if w not in _small:
            docs = make_docs(w, 130, 7 * w + 130)
            docs[3] = docs[3].copy()
            docs[3][0] = 0.0
            _small[w] = docs
        return _small[w]
    yield get
    _small.clear()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("w", (64, 192, 768))
def test_codes_are_the_search_over_the_centroids(model, small_docs, storage, w):
    docs = [d.copy() for d in small_docs(w)]
    for C in (16, 48, 1040):
        cent = make_centroids(w, C)
        docs[4][0] = cent[2]                                               # a row that is the duplicated centroid
        ix = store_of(model, docs, w, storage=storage)
        assert ix.n_centroids == 0
        ix.set_centroids(cent)
        assert ix.n_centroids == C
        S_c = centroid_store(model, cent, storage)
        got = assert_codes(ix, S_c)
        flat = np.concatenate(got)
        assert flat.max() < C and not np.any(flat == 5)                    # the duplicate's lower index wins
        assert got[4][0] == 2 and got[3][0] == 0                           # the planted row; the zero row
        assert len(set(flat.tolist())) > 8
        for c in (0, 2, 5, C - 1):                                         # a centroid holds a one-token document's bits
            assert same(ix.centroid(c), S_c.doc(c)[0])


# ---- 2. codes follow the store ----
@pytest.mark.parametrize("storage", STORAGES)
def test_codes_follow_the_store(model, storage):
    w = 64
    docs = make_docs(w, 24, 3)
    ix = bertpy.BertTokenIndex(model, 64, 4 * slots_of(docs), width=w, storage=storage)
    cent_a, cent_b = make_centroids(w, 48), make_centroids(w, 16, seed=9)
    S_a, S_b = centroid_store(model, cent_a, storage), centroid_store(model, cent_b, storage)
    assert ix.add(docs[:8]) == 0
    with pytest.raises(RuntimeError):
        ix.doc_codes(0)                                                    # no centroids yet
    ix.set_centroids(cent_a)
    assert_codes(ix, S_a)
    assert ix.add(docs[8:16]) == 8                                         # one call of several documents
    assert_codes(ix, S_a)
    for j, d in enumerate(docs[16:24]):                                    # one call per document
        assert ix.add([d]) == 16 + j
    several = assert_codes(ix, S_a)
    ix.set_centroids(cent_b)                                               # other centroids: every code again
    assert ix.n_centroids == 16
    assert_codes(ix, S_b)
    ix.set_centroids(cent_a)
    again = assert_codes(ix, S_a)
    assert all(np.array_equal(a, b) for a, b in zip(several, again))
    ix.clear()
    assert len(ix) == 0 and ix.n_centroids == 48                           # clear keeps the centroids
    assert ix.add(docs[12:20]) == 0
    assert len(assert_codes(ix, S_a)) == 8


# ---- 3. candidates ----
# (Lq, B, n_cand): Lq of 1, 16, 17, 32, 33, 64 (1 .. 4 tiles), B of 1 .. 9, n_cand of 1, 10, 128
COMBOS = [(1, 9, 10), (16, 5, 128), (16, 1, 1), (17, 3, 10), (32, 2, 128), (33, 2, 10), (64, 2, 10), (64, 1, 128),
          (16, 9, 10), (32, 1, 1), (1, 4, 128), (17, 6, 1), (32, 7, 10), (64, 3, 1), (33, 8, 128)]

_coded = {}


@pytest.fixture(scope="module")
def coded(model):
    """(ix, cent, sub) by (storage, w, n, C): a coded store and its substituted store (every
    row replaced by the caller's f32 centroid row of its code); built once, never changed."""
    def get(storage, w, n, C):
        key = (storage, w, n, C)
        if key not in _coded:
            docs = make_docs(w, n, 7 * w + n)
            ix = store_of(model, docs, w, storage=storage)
            cent = make_centroids(w, C)
            ix.set_centroids(cent)
            codes = [ix.doc_codes(i) for i in range(n)]
            sub = store_of(model, PR.substitute(cent, codes), w, storage=storage)
            _coded[key] = (ix, cent, sub)
        return _coded[key]
    yield get
    _coded.clear()


def check_candidates(ix, sub, queries, n_cand):
    want_s, want_i = sub.search(queries, n_cand)
    got_s, got_i = ix.candidates(queries, n_cand)
    assert got_i.dtype == np.int32 and np.array_equal(got_i, want_i), (got_i, want_i)
    assert same(got_s, want_s)
    return got_s, got_i


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("w,n", SHAPES)
def test_candidates_equal_the_search_of_the_substituted_store(model, coded, storage, w, n):
    lib = model.lib
    forms, ties = 0, 0
    for C in (16, 1040):
        ix, cent, sub = coded(storage, w, n, C)
        for Lq, B, n_cand in (COMBOS if n == 5000 or w == 192 else COMBOS[::3]):
            lib.bertx_test_approx_ran(1)
            s, i = check_candidates(ix, sub, make_queries(w, Lq, B), n_cand)
            ran = lib.bertx_test_approx_ran(0)
            # 64 * tiles * C bytes beside the lists of 8 waves: C 16 always fits, C 1,040 with
            # four tiles (266 KB) never does
            if C == 16:
                assert ran == 1
            elif (Lq + 15) // 16 * min(B, 4 // ((Lq + 15) // 16)) == 4:
                assert ran & 2
            forms |= ran
            tied = (s[:, 1:] == s[:, :-1]) & (i[:, 1:] >= 0)
            ties += int(tied.sum())
            assert np.all(i[:, 1:][tied] > i[:, :-1][tied])                 # equal scores by ascending id
    assert forms == 3                                                       # both placements ran
    assert ties > 0                                                         # documents that share their code sets tie


@pytest.mark.parametrize("storage", STORAGES)
def test_a_candidate_list_is_independent_of_the_call(coded, storage):
    ix, cent, sub = coded(storage, 192, 130, 16)
    for Lq, B in ((16, 9), (64, 3)):
        qs = make_queries(192, Lq, B, seed=9)
        s, i = ix.candidates(qs, 128)
        for b in range(B):
            s1, i1 = ix.candidates([qs[b]], 128)
            assert same(s1[0], s[b]) and np.array_equal(i1[0], i[b])
            s2, i2 = ix.candidates([qs[b]], 10)                            # another n_cand: a prefix
            assert same(s2[0], s[b, :10]) and np.array_equal(i2[0], i[b, :10])


# ---- 4. the pruned search ----
def check_pruned(ix, queries, k, n_cand):
    got_s, got_i = ix.search_pruned(queries, k, n_cand)
    cs, ci = ix.candidates(queries, n_cand)
    for b, q in enumerate(queries):
        exact = ix.score(q, ci[b])
        assert np.all(np.isneginf(exact[ci[b] < 0]))
        want_s, want_i = PR.compose(exact, ci[b], k)
        assert np.array_equal(got_i[b], want_i), (got_i[b], want_i)
        assert same(got_s[b], want_s)
    return got_s, got_i


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("w,n", SHAPES)
def test_pruned_search_is_candidates_score_topk(coded, storage, w, n):
    for C in (16, 1040):
        ix, cent, sub = coded(storage, w, n, C)
        for Lq, B, k, n_cand in ((17, 3, 10, 32), (64, 2, 1, 1), (16, 9, 128, 128), (32, 5, 5, 128), (1, 4, 10, 11)):
            check_pruned(ix, make_queries(w, Lq, B, seed=6), k, n_cand)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("k", (10, 128))
def test_pruned_search_over_every_document_is_the_full_scan(model, storage, k):
    w = 192
    cent = make_centroids(w, 48)
    for n in (0, 1, k - 1, k, k + 1):
        if n > 128:
            continue                                                       # more documents than candidates: not this rule
        docs = make_docs(w, n, 31 * n + k)
        ix = bertpy.BertTokenIndex(model, max(n, 1), max(slots_of(docs), 16), width=w, storage=storage)
        ix.set_centroids(cent)
        if n:
            assert ix.add(docs) == 0
        qs = make_queries(w, 17, 3)
        n_cand = max(k, min(n + 3, 128))
        want_s, want_i = ix.search(qs, k)
        got_s, got_i = check_pruned(ix, qs, k, n_cand)
        assert np.array_equal(got_i, want_i) and same(got_s, want_s)
        assert np.all(got_i[:, min(n, k):] == -1) and np.all(np.isneginf(got_s[:, min(n, k):]))
        assert np.all(got_i[:, :min(n, k)] >= 0)


# ---- 5. the device forms ----
@pytest.mark.parametrize("storage", STORAGES)
def test_device_forms_captured_graph(model, coded, dev, storage):
    w, Lq, B, k, n_cand = 192, 33, 3, 10, 32
    ix, cent, sub = coded(storage, w, 130, 1040)
    q = np.stack(make_queries(w, Lq, B, seed=8))
    want_s, want_i = ix.search_pruned(list(q), k, n_cand)
    want_cs, want_ci = ix.candidates(list(q), n_cand)
    hip, vp, lib = dev.hip, ctypes.c_void_p, model.lib
    s = vp()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    dq = dev.up(q)
    ds, di = dev.alloc(B * k * 4), dev.alloc(B * k * 4)
    dcs, dci = dev.alloc(B * n_cand * 4), dev.alloc(B * n_cand * 4)

    def both():
        rc = lib.bertx_mvindex_candidates_device(ix.mv, dq, B, Lq, n_cand, dcs, dci, s)
        return rc or lib.bertx_mvindex_search_pruned_device(ix.mv, dq, B, Lq, k, n_cand, ds, di, s)

    def check():
        assert same(dev.down(ds, (B, k), np.float32), want_s) and np.array_equal(dev.down(di, (B, k), np.int32), want_i)
        assert same(dev.down(dcs, (B, n_cand), np.float32), want_cs)
        assert np.array_equal(dev.down(dci, (B, n_cand), np.int32), want_ci)

    assert both() == 0 and hip.hipStreamSynchronize(s) == 0
    check()
    graph, ex = vp(), vp()
    assert hip.hipStreamBeginCapture(s, 1) == 0   # thread-local mode
    rc = both()
    assert hip.hipStreamEndCapture(s, ctypes.byref(graph)) == 0 and rc == 0
    assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, 0) == 0
    for _ in range(2):
        for p, nbytes in ((ds, B * k * 4), (di, B * k * 4), (dcs, B * n_cand * 4), (dci, B * n_cand * 4)):
            zeros = np.zeros(nbytes, np.uint8)
            assert hip.hipMemcpy(p, zeros.ctypes.data, nbytes, 1) == 0
        assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
        check()
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    hip.hipStreamDestroy(s)


# ---- 6. refusals ----
@pytest.mark.parametrize("storage", STORAGES)
def test_refusals_leave_the_outputs_alone(model, storage):
    w = 64
    docs = make_docs(w, 20, 4)
    ix = store_of(model, docs, w, storage=storage)
    L = model.lib
    q = np.stack(make_queries(w, 64, 2) + make_queries(w, 64, 1, seed=7))[:, :, :]
    q65 = np.zeros((1, 65, w), np.float32)
    s = np.full((3, 128), 7.0, np.float32)
    i = np.full((3, 128), 7, np.int32)

    def cand(qa, B, Lq, n_cand):
        return L.bertx_mvindex_candidates(ix.mv, qa.ctypes.data, B, Lq, n_cand, s.ctypes.data, i.ctypes.data)

    def pruned(qa, B, Lq, k, n_cand):
        return L.bertx_mvindex_search_pruned(ix.mv, qa.ctypes.data, B, Lq, k, n_cand, s.ctypes.data, i.ctypes.data)

    assert cand(q, 3, 64, 10) == -1 and pruned(q, 3, 64, 5, 10) == -1       # no centroids
    assert L.bertx_mvindex_train_centroids(ix.mv, 24, 1, 0) == -1
    cent = make_centroids(w, 32)
    assert L.bertx_mvindex_set_centroids(ix.mv, cent.ctypes.data, 24) == -1 # C = 24
    assert L.bertx_mvindex_set_centroids(ix.mv, cent.ctypes.data, 0) == -1
    assert ix.n_centroids == 0
    ix.set_centroids(cent)
    assert pruned(q, 3, 64, 11, 10) == -1                                   # n_cand < k
    assert pruned(q, 3, 64, 10, 129) == -1 and cand(q, 3, 64, 129) == -1    # n_cand = 129
    assert cand(q, 3, 64, 0) == -1 and pruned(q, 3, 64, 0, 10) == -1
    assert cand(q65, 1, 65, 10) == -1 and pruned(q65, 1, 65, 5, 10) == -1   # Lq = 65
    assert cand(q, 0, 64, 10) == -1
    assert L.bertx_mvindex_train_centroids(ix.mv, 16, -1, 0) == -1
    big = sum(len(d) for d in docs) // 16 * 16 + 16
    assert L.bertx_mvindex_train_centroids(ix.mv, big, 1, 0) == -1          # more centroids than sample rows
    assert np.all(s == 7.0) and np.all(i == 7)
    assert ix.n_centroids == 32
    c = np.full(4, 9, np.uint16)
    assert L.bertx_mvindex_doc_codes(ix.mv, 99, c.ctypes.data) == -1 and np.all(c == 9)
    assert cand(q, 3, 64, 10) == 0 and pruned(q, 3, 64, 5, 10) == 0          # and the same calls in range succeed


# ---- 7. training ----
@pytest.mark.parametrize("storage", STORAGES)
def test_training_is_reproducible_and_follows_the_rule(model, storage):
    w, n, C, iters = 64, 300, 16, 3
    rng = np.random.default_rng(11)
    # Rows around 14 directions.  The rows that seed centroids 0 .. 13 come one from each
    # direction, and the two that seed centroids 14 and 15 are one and the same row x far from
    # all of them: the two x tie for centroid 14 in every assignment, its mean (x + x) / 2 is
    # x again, and centroid 15 never has a member.
    dirs = M.unit_rows(rng, 15, w)
    lens = rng.choice((1, 15, 16, 17, 33), n)
    T = int(lens.sum())
    flat = (dirs[rng.integers(0, 14, T)] + 0.01 * rng.standard_normal((T, w))).astype(np.float32)
    seeds = PR.initial_rows(T, C)
    for c in range(14):
        flat[seeds[c]] = (dirs[c] + 0.01 * rng.standard_normal(w)).astype(np.float32)
    flat[seeds[14]] = flat[seeds[15]] = dirs[14]
    docs = np.split(flat, np.cumsum(lens)[:-1])
    ix = store_of(model, docs, w, storage=storage)
    ix.train_centroids(C, iters=iters, seed=5)
    first = np.stack([ix.centroid(c) for c in range(C)])
    codes_first = [ix.doc_codes(i) for i in range(n)]
    other = store_of(model, docs, w, storage=storage)
    other.train_centroids(C, iters=iters, seed=5)
    assert same(np.stack([other.centroid(c) for c in range(C)]), first)
    assert all(np.array_equal(other.doc_codes(i), codes_first[i]) for i in range(n))

    # the rule, replayed through set_centroids / doc_codes / doc
    replay = store_of(model, docs, w, storage=storage)
    sample = np.concatenate([replay.doc(i) for i in range(n)])             # stride 1: every valid row
    assert PR.sample_rule(T, 5) == (1, 0, T)
    assert len(sample) == T
    cent = sample[PR.initial_rows(T, C)].copy()
    for _ in range(iters):
        replay.set_centroids(cent)
        codes = np.concatenate([replay.doc_codes(i) for i in range(n)])
        kept = cent[15].copy()
        cent, empty = PR.kmeans_update(sample, codes, cent)
        assert empty >= 1 and not np.any(codes == 15) and same(cent[15], kept)   # the empty centroid keeps its row
    replay.set_centroids(cent)
    assert not np.any(np.concatenate(codes_first) == 15)
    assert same(np.stack([replay.centroid(c) for c in range(C)]), first)
    assert all(np.array_equal(replay.doc_codes(i), codes_first[i]) for i in range(n))
    # iters = 0: the initial centroids, the store coded
    zero = store_of(model, docs, w, storage=storage)
    zero.train_centroids(C, iters=0)
    replay.set_centroids(sample[PR.initial_rows(T, C)])
    assert same(np.stack([zero.centroid(c) for c in range(C)]), np.stack([replay.centroid(c) for c in range(C)]))


# ---- 8. planted recall ----
@pytest.mark.parametrize("storage", STORAGES)
def test_planted_documents_come_first(model, storage):
    cent, docs, queries, targets, dirs = PR.planted_case()
    ix = store_of(model, docs, PR.PLANT_W, storage=storage)
    ix.set_centroids(cent)
    for i in (0, 7, len(docs) - 1):
        assert np.array_equal(ix.doc_codes(i), dirs[i])
    s, ids = ix.search_pruned(queries, 10, 32)
    assert ids[:, 0].tolist() == targets
    full_s, full_i = ix.search(queries, 10)
    assert full_i[:, 0].tolist() == targets and same(s[:, 0], full_s[:, 0])
    cs, ci = ix.candidates(queries, 32)
    assert ci[:, 0].tolist() == targets


# ---- 9. the text forms, the tool, the bench hook ----
def assert_sorted(s, i):
    for a in range(len(s) - 1):
        if i[a + 1] >= 0:
            assert SR.better(s[a], int(i[a]), s[a + 1], int(i[a + 1]))


@pytest.mark.parametrize("storage", STORAGES)
def test_search_texts_pruned(model, tok_golden, storage):
    words = corpus_words(tok_golden)
    texts = corpus_texts(words, 40)
    ix = bertpy.BertTokenIndex(model, 40, 40 * 48, storage=storage)
    assert ix.add_texts(texts) == 0
    queries = [texts[3], " ".join(words[200:204]), words[5], texts[22]]        # ragged: 3 .. 30 tokens
    with pytest.raises(RuntimeError):
        ix.search_texts(queries, 3, n_cand=8)                                  # no centroids
    ix.train_centroids(32, iters=2)
    full_s, full_i = ix.search_texts(queries, 5)
    s, i = ix.search_texts(queries, 5, n_cand=64)                              # every document is a candidate
    assert same(s, full_s) and np.array_equal(i, full_i)
    s, i = ix.search_texts(queries, 3, n_cand=8)
    for b, q in enumerate(queries):
        assert np.all(i[b] >= 0) and len(set(i[b].tolist())) == 3
        assert same(s[b], ix.score_text(q, i[b]))                              # the scorer's bits
        assert_sorted(s[b], i[b])
    assert i[0, 0] == 3 and i[3, 0] == 22                                      # every token finds itself
    long_q = " ".join(words[j] for j in range(70))
    nan_bits = np.uint32(0x7fc01234)
    so, io = np.full(3 * 5, nan_bits, np.uint32), np.full(3 * 5, nan_bits, np.uint32)
    rc = model.lib.bertx_mvindex_search_pruned_texts(ix.mv, model.ctx, 2, 3,
                                                     bertpy.BertIndex._texts([texts[0], long_q, texts[1]]), 5, 8, 0,
                                                     so.ctypes.data, io.ctypes.data)
    assert rc == -4 and np.all(so == nan_bits) and np.all(io == nan_bits)


def test_search_tool_pruned(model, colbert_model, tmp_path):
    """search -l -a -C 16 and search -L MODEL -a -C 16 print what the Python calls return;
    -C without -a, a C that is no multiple of 16 and a -c below k are usage errors."""
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(COLBERT_TEXTS) + "\n")
    queries = ["stone bridge", "one two", "marks, words"]
    k = 3
    base = ["-m", TINY64, "-f", str(corpus), "-k", str(k)]
    r, got = tool_lines(base + ["-l", "-a", "-C", "16", "-c", "5"], queries)
    assert r.returncode == 0, r.stderr
    ix = bertpy.BertTokenIndex(model, 10, 10 * 32)
    assert ix.add_texts(COLBERT_TEXTS) == 0
    ix.train_centroids(16, iters=8, seed=0)
    s, i = ix.search_texts(queries, k, n_cand=5)
    want = ["%d\t%d\t%.4f\t%s" % (j + 1, i[b, j], s[b, j], COLBERT_TEXTS[i[b, j]]) for b in range(3) for j in range(k)]
    assert got == want
    r, got = tool_lines(base + ["-L", colbert_model, "-a", "-C", "16", "-S", "int8"], queries)
    assert r.returncode == 0, r.stderr
    c = bertpy.BertModel(colbert_model)
    cx = bertpy.BertTokenIndex(c, 10, 10 * 192, width=c.proj_width, storage="int8")
    assert cx.add_texts(COLBERT_TEXTS, colbert=min(180, c.n_max_tokens)) == 0
    cx.train_centroids(16, iters=8, seed=0)
    s, i = cx.search_texts(queries, k, colbert=32, n_cand=12)                  # the tool's default: min(128, 4 k)
    want = ["%d\t%d\t%.4f\t%s" % (j + 1, i[b, j], s[b, j], COLBERT_TEXTS[i[b, j]]) for b in range(3) for j in range(k)]
    assert got == want
    for bad in (["-l", "-C", "16"], ["-l", "-a", "-C", "24"], ["-l", "-a", "-C", "16", "-c", "2"], ["-C", "16"]):
        r, _ = tool_lines(base + bad, [])
        assert r.returncode == 2 and "usage" in r.stderr, bad


@pytest.mark.parametrize("storage", (0, 1))
def test_bench_hook(model, storage):
    us = (ctypes.c_float * 3)(0, 0, 0)
    assert model.lib.bertx_bench_maxsim_pruned(64, 300, 0, 16, 32, 2, 10, 32, storage, 2, us) == 0
    assert min(us) > 0 and us[2] > us[0]
    assert model.lib.bertx_bench_maxsim_pruned(64, 300, 0, 16, 32, 2, 33, 32, storage, 2, us) < 0
