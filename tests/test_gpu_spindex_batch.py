"""GPU tests of the sparse index's batched sparse-query search (sparse_batch.hip, spindex.cpp):
ids and score bits against the numpy restatement of the contract on the densified queries
(spindex_refs.scores_ref, topk_ref), never a tolerance."""
import os

import numpy as np
import pytest

import bertpy
import sparse_refs as SR
import spindex_refs as PR
from row_kernel_refs import bits
from test_gpu_search import corpus_texts
from test_gpu_search_bin import dev, replay_twice, stream  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_TOP = {130: 65, 30522: 256, 65536: 256}
N_DOCS = {130: [1, 67, 2100], 30522: [1, 67, 2100], 65536: [67]}
SHAPES = [(130, 1, 1), (130, 16, 10), (30522, 32, 10), (30522, 128, 128), (65536, 16, 10)]


@pytest.fixture(autouse=True)
def _one_device(monkeypatch):
    monkeypatch.delenv("BERT_HOST_ONLY", raising=False)
    monkeypatch.setenv("BERT_DEVICES", "0")


@pytest.fixture(scope="module")
def model(lib):
    os.environ["BERT_DEVICES"] = "0"
    return bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))


def queries(V, q_top):
    """64 queries (terms int32 [64][q_top], -1 past a row's count; weights in (-0.5, 3)) drawn from a
    pool of 6 q_top terms, so queries share terms; slot 0 of rows 0 .. 4 planted: an empty query, term 0
    (the padding postings' term) with a negative weight, term V - 1, a weight that rounds to f16 zero,
    and term V - 2, which no document holds."""
    rng = np.random.default_rng(V + q_top)
    pool = rng.permutation(np.arange(1, V - 2))[:6 * q_top]
    t, w = np.full((64, q_top), -1, np.int32), np.zeros((64, q_top), F)
    for b in range(64):
        c = int(rng.integers(1, q_top + 1))
        t[b, :c], w[b, :c] = rng.permutation(pool)[:c], rng.uniform(-0.5, 3.0, c)
    t[0], w[0] = -1, 0
    t[1, 0], w[1, 0] = 0, -1.25
    t[2, 0] = V - 1
    w[3, 0] = 1e-9
    t[4], w[4] = -1, 0
    t[4, 0], w[4, 0] = V - 2, 2.0
    return t, w


def densify(t, w, V):
    q = np.zeros((t.shape[0], V), F)
    for b in range(t.shape[0]):
        q[b, t[b][t[b] >= 0]] = w[b][t[b] >= 0]
    return q


@pytest.fixture(scope="module")
def stores(model):
    """{(V, n_docs): (index, docs)}: make_docs over the terms below V - 2, every fifth document ending in V - 1."""
    out = {}
    for V, n_top in N_TOP.items():
        for n_docs in N_DOCS[V]:
            docs = PR.make_docs(V - 2, n_top, n_docs, seed=V + n_docs)
            for i in range(1, n_docs, 5):
                if len(docs[i][0]):
                    docs[i] = (np.append(docs[i][0][:-1], V - 1).astype(np.int32), docs[i][1])
            ix = bertpy.BertSparseIndex(model, n_docs, sum(-(-len(t) // 16) * 16 for t, _ in docs) + 16, n_top=n_top, n_vocab=V)
            assert ix.add_postings(docs) == 0 and len(ix) == n_docs
            out[V, n_docs] = (ix, docs)
    return out


@pytest.fixture(scope="module")
def refs(stores):
    """(V, q_top, n_docs) -> (terms, weights, dense queries, scores_ref of the 64 queries), computed once."""
    memo = {}

    def get(V, q_top, n_docs):
        if (V, q_top, n_docs) not in memo:
            t, w = queries(V, q_top)
            q = densify(t, w, V)
            memo[V, q_top, n_docs] = (t, w, q, PR.scores_ref(q, stores[V, n_docs][1])[0])
        return memo[V, q_top, n_docs]
    return get


@pytest.mark.parametrize("B_of", [lambda NQ: 1, lambda NQ: 5, lambda NQ: NQ, lambda NQ: NQ + 1, lambda NQ: 64],
                         ids=["1", "5", "NQ", "NQ+1", "64"])
@pytest.mark.parametrize("V,q_top,k", SHAPES)
def test_scan_batch(lib, stores, refs, V, q_top, k, B_of):
    """Ids and score bits equal the reference at every store size (2,100 documents on one workgroup,
    whose staging tile fills and drains many times, and on three that merge); the passes are
    ceil(B / NQ); up to five queries also equal the dense-query search, bit for bit."""
    for n_docs in N_DOCS[V]:
        ix, _ = stores[V, n_docs]
        NQ = lib.bertx_spindex_batch_queries(ix.sp, q_top, k)
        assert NQ in (4, 8, 16, 32)
        B = B_of(NQ)
        t, w, q, ref = refs(V, q_top, n_docs)
        want_s, want_i = PR.topk_ref(ref[:B], k)
        for cap in ((1, 3) if n_docs == 2100 else (0,)):
            assert lib.bertx_test_spindex_grid(ix.sp, cap) == 0
            got_s, got_i = ix.search_sparse(t[:B], w[:B], k)
            assert lib.bertx_test_spindex_last_passes(ix.sp) == -(-B // NQ)
            assert cap == 0 or lib.bertx_test_spindex_last_grid(ix.sp) == cap
            assert np.array_equal(got_i, want_i), (n_docs, cap)
            assert np.array_equal(bits(got_s), bits(want_s)), (n_docs, cap)
        lib.bertx_test_spindex_grid(ix.sp, 0)
        if B <= 5:
            dense_s, dense_i = ix.search(q[:B], k)
            assert np.array_equal(dense_i, want_i) and np.array_equal(bits(dense_s), bits(want_s))


def test_query_alone_pairs_and_refusals(stores, refs):
    """A query alone returns the bits it gets inside a batch of 64; pair lists pad to the same search;
    the host form refuses a term >= n_vocab, a term repeated within a query and a non-finite weight."""
    ix, _ = stores[30522, 67]
    t, w, _, _ = refs(30522, 32, 67)
    batch_s, batch_i = ix.search_sparse(t, w, 10)
    for b in (1, 40):
        one_s, one_i = ix.search_sparse(t[b], w[b], 10)
        assert np.array_equal(one_i[0], batch_i[b]) and np.array_equal(bits(one_s[0]), bits(batch_s[b]))
    pairs = [[(int(a), float(x)) for a, x in zip(t[b], w[b]) if a >= 0] for b in range(6)]
    pair_s, pair_i = ix.search_sparse(pairs, k=10)
    assert np.array_equal(pair_i, batch_i[:6]) and np.array_equal(bits(pair_s), bits(batch_s[:6]))
    for bad in ([(30522, 1.0)], [(7, 1.0), (9, 1.0), (7, 2.0)], [(7, np.inf)], [(7, np.nan)]):
        with pytest.raises(RuntimeError):
            ix.search_sparse([[(3, 1.0)], bad], k=10)


def test_texts_and_graph(lib, tok_golden, tmp_path, dev, stream):
    """search_texts with q_top = n_top is search_sparse of forward_sparse_top's output and, no query
    holding more positive weights than that, the dense text search; a captured search replays the eager bits."""
    m = bertpy.BertModel(SR.make_sparse_models(lib, GOLDEN, str(tmp_path))["f16"])
    texts, new, _ = corpus_texts(tok_golden)
    n_top = 24
    ix = bertpy.BertSparseIndex(m, len(texts), len(texts) * 32, n_top=n_top)
    assert ix.add_texts(texts) == 0
    queries_ = texts[3:40:8] + new
    ids = [np.asarray(m.tokenize(t)[0], np.int32) for t in queries_]
    terms, wts, counts = m.forward_sparse_top(ids, n_top)
    want_s, want_i = ix.search_sparse(terms, wts, 5)
    got_s, got_i = ix.search_texts(queries_, 5, q_top=n_top)
    assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), bits(want_s))
    wide = int((m.forward_sparse(ids) > 0).sum(axis=1).max())
    full_s, full_i = ix.search_texts(queries_, 5, q_top=wide)
    dense_s, dense_i = ix.search_texts(queries_, 5)
    assert np.array_equal(full_i, dense_i) and np.array_equal(bits(full_s), bits(dense_s))
    B, k = len(queries_), 5
    d_t, d_w, d_s, d_i = dev.up(terms), dev.up(wts), dev.alloc(B * k * 4), dev.alloc(B * k * 4)
    replay_twice(dev, stream, lambda: lib.bertx_spindex_search_sparse_device(ix.sp, d_t, d_w, B, n_top, k, d_s, d_i, stream),
                 [(d_s, (B, k), F), (d_i, (B, k), np.int32)], [want_s, want_i])
