"""GPU tests of the sparse index (sparse_select.hip, sparse_scan.hip, spindex.cpp): the device
top-n selection through bertx_test_sparse_select, the fused scan against the contract restated
in numpy, and the text forms end to end on the golden masked-LM model.  References: spindex_refs.py."""
import ctypes
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
N_TOP = {130: 65, 30522: 256}
N_DOCS = [1, 67, 2100]


@pytest.fixture(autouse=True)
def _one_device(monkeypatch):
    monkeypatch.delenv("BERT_HOST_ONLY", raising=False)
    monkeypatch.setenv("BERT_DEVICES", "0")


@pytest.fixture(scope="module")
def model(lib):
    os.environ["BERT_DEVICES"] = "0"
    return bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))


@pytest.mark.parametrize("group", [0, 1], ids=["-".join(g) for g in PR.PLANTED])
@pytest.mark.parametrize("n", [1, 16, 256, 1024])
@pytest.mark.parametrize("V", [1, 130, 1027, 30522])
def test_select(lib, V, n, group):
    """Terms, weight bits and counts equal the stable argsort cut at n; the guard rows stay untouched (rc 0)."""
    rng = np.random.default_rng(1000 * V + n)
    rows = np.stack([PR.planted_row(kind, V, n, rng) for kind in PR.PLANTED[group]])
    terms, wts, counts = np.zeros((3, n), np.int32), np.zeros((3, n), F), np.zeros(3, np.int32)
    assert lib.bertx_test_sparse_select(rows.ctypes.data, 3, V, n, terms.ctypes.data, wts.ctypes.data, counts.ctypes.data) == 0
    want_t, want_w, want_c = PR.select_ref(rows, n)
    assert np.array_equal(counts, want_c)
    assert np.array_equal(terms, want_t)
    assert np.array_equal(bits(wts), bits(want_w))


@pytest.fixture(scope="module")
def stores(model):
    """{(V, n_docs): (index, scores_ref of the five queries, exact, bound, queries)}, built once."""
    out = {}
    for V, n_top in N_TOP.items():
        rng = np.random.default_rng(V)
        q = np.where(rng.random((5, V)) < 0.3, rng.uniform(-0.5, 3.0, (5, V)), 0.0).astype(F)
        for n_docs in N_DOCS:
            docs = PR.make_docs(V, n_top, n_docs, seed=V + n_docs)
            ix = bertpy.BertSparseIndex(model, n_docs, sum(-(-len(t) // 16) * 16 for t, _ in docs) + 16, n_top=n_top, n_vocab=V)
            assert ix.add_postings(docs) == 0 and len(ix) == n_docs
            out[V, n_docs] = (ix, docs, q) + PR.scores_ref(q, docs)
    return out


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("V", [130, 30522])
def test_scan(lib, stores, V, B, k):
    """Ids and score bits equal the numpy restatement of the contract, at 1, 67 and 2,100 documents
    (the last on one workgroup, about 130 documents per wave, and on three that merge); the scores
    lie within count * 2^-24 * sum |qh w| of float64; the stored postings read back."""
    for n_docs in N_DOCS:
        ix, docs, q, ref, exact, bound = stores[V, n_docs]
        assert np.all(np.abs(ref.astype(np.float64) - exact) <= bound)
        want_s, want_i = PR.topk_ref(ref[:B], k)
        for cap in ((1, 3) if n_docs == 2100 else (0,)):
            assert lib.bertx_test_spindex_grid(ix.sp, cap) == 0
            got_s, got_i = ix.search(q[:B], k)
            assert cap == 0 or lib.bertx_test_spindex_last_grid(ix.sp) == cap
            assert np.array_equal(got_i, want_i), (n_docs, cap)
            assert np.array_equal(bits(got_s), bits(want_s)), (n_docs, cap)
        lib.bertx_test_spindex_grid(ix.sp, 0)
        for i in (0, n_docs // 2, n_docs - 1):
            t, w = ix.doc(i)
            assert np.array_equal(t, docs[i][0]) and np.array_equal(bits(w), bits(docs[i][1]))


def test_scan_query_alone_and_pairs(stores):
    """A query row alone returns the bits it gets inside a batch; (term, weight) pair lists densify to the same search."""
    ix, docs, q, ref, _, _ = stores[30522, 67]
    batch_s, batch_i = ix.search(q, 10)
    for b in (1, 4):
        one_s, one_i = ix.search(q[b], 10)
        assert np.array_equal(one_i[0], batch_i[b]) and np.array_equal(bits(one_s[0]), bits(batch_s[b]))
    pairs = [[(int(t), float(q[b, t])) for t in np.flatnonzero(q[b])] for b in range(2)]
    pair_s, pair_i = ix.search(pairs, 10)
    assert np.array_equal(pair_i, batch_i[:2]) and np.array_equal(bits(pair_s), bits(batch_s[:2]))


def test_add_postings_refusals(model):
    ix = bertpy.BertSparseIndex(model, 4, 256, n_top=4, n_vocab=100)
    for terms, wts in (([3, 2], [1, 1]), ([2, 2], [1, 1]), ([100], [1]), ([1], [-1.0]), ([1], [np.inf]), ([1, 2, 3, 4, 5], [1] * 5)):
        with pytest.raises(RuntimeError):
            ix.add_postings([(terms, wts)])
    assert len(ix) == 0 and ix.add_postings([([1, 99], [0.5, 2.0]), ([], [])]) == 0 and len(ix) == 2
    scores, ids = ix.search(np.ones((1, 100), F), 3)
    assert ids.tolist() == [[0, 1, -1]] and scores.tolist() == [[2.5, 0.0, -np.inf]]


def test_end_to_end(lib, tok_golden, tmp_path, dev, stream):
    """add_texts then doc(i) is numpy's select-and-round of that run's forward_sparse rows, from dense
    rows (add) as well; forward_sparse_top is the selection; search_texts is search on the same rows;
    a captured search_device replays the eager bits."""
    m = bertpy.BertModel(SR.make_sparse_models(lib, GOLDEN, str(tmp_path))["f16"])
    texts, new, _ = corpus_texts(tok_golden)
    ids = [np.asarray(m.tokenize(t)[0], np.int32) for t in texts]
    rows = m.forward_sparse(ids)
    V, n_top = m.sparse_width, 24
    want_t, want_w, want_c = PR.select_ref(rows, n_top)
    assert (want_c == n_top).any()
    top = m.forward_sparse_top(ids, n_top)
    assert np.array_equal(top[0], want_t) and np.array_equal(bits(top[1]), bits(want_w)) and np.array_equal(top[2], want_c)
    ix = bertpy.BertSparseIndex(m, 2 * len(texts), 2 * len(texts) * 32, n_top=n_top)
    assert ix.add_texts(texts) == 0 and ix.add(rows) == len(texts) and len(ix) == 2 * len(texts)
    assert ix.postings() == 2 * sum(-(-int(c) // 16) * 16 for c in want_c)
    for i in range(2 * len(texts)):
        t, w = ix.doc(i)
        c = want_c[i % len(texts)]
        assert np.array_equal(t, want_t[i % len(texts), :c])
        assert np.array_equal(bits(w), bits(want_w[i % len(texts), :c].astype(np.float16).astype(F)))
    queries = texts[3:40:8] + new
    qrows = m.forward_sparse([np.asarray(m.tokenize(t)[0], np.int32) for t in queries])
    got_s, got_i = ix.search_texts(queries, 5)
    want_s, want_i = ix.search(qrows, 5)
    assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), bits(want_s))
    docs = [ix.doc(i) for i in range(len(ix))]
    ref_s, ref_i = PR.topk_ref(PR.scores_ref(qrows, docs)[0], 5)
    assert np.array_equal(want_i, ref_i) and np.array_equal(bits(want_s), bits(ref_s))
    B, k = len(queries), 5
    d_q, d_s, d_i = dev.up(qrows), dev.alloc(B * k * 4), dev.alloc(B * k * 4)
    replay_twice(dev, stream, lambda: lib.bertx_spindex_search_device(ix.sp, d_q, B, k, d_s, d_i, stream),
                 [(d_s, (B, k), F), (d_i, (B, k), np.int32)], [want_s, want_i])
