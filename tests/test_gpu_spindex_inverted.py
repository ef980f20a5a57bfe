"""GPU tests of the sparse index's block-local inverted lists and term-major search
(sparse_invert.hip, spindex.cpp): ids and score bits against the numpy restatement of the
contract (bert_hip.h "Inverted lists"), never a tolerance."""
import os

import numpy as np
import pytest

import bertpy
import sparse_refs as SR
import spindex_refs as PR
from row_kernel_refs import bits
from test_gpu_search import corpus_texts
from test_gpu_search_bin import dev, replay_twice, stream  # noqa: F401
from test_gpu_spindex_batch import _one_device, model, queries  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_TOP = {130: 65, 30522: 256, 65536: 256}
N_DOCS = {130: [1, 63, 64, 65, 257, 2100], 30522: [1, 65, 2100], 65536: [64, 257]}
SHAPES = [(130, 1, 1), (130, 32, 10), (30522, 32, 10), (30522, 128, 128), (65536, 32, 10), (65536, 128, 128)]


def inverted_ref(t, w, docs):
    """Scores f32 [B][docs] of the contract: s = +0, then over the query's slots i in slot order whose
    term the document holds s = fmaf(f16(weight_i), w, s); the product of two f16 values is exact in
    f32, so the f32 multiply and add round once, as the fma does."""
    doc = np.concatenate([np.full(len(d[0]), i) for i, d in enumerate(docs)] + [np.zeros(0, int)])
    term = np.concatenate([d[0] for d in docs] + [np.zeros(0, np.int32)])
    wt = np.concatenate([d[1] for d in docs] + [np.zeros(0, F)])
    order = np.argsort(term, kind="stable")
    term, doc, wt = term[order], doc[order], wt[order]
    qh = w.astype(np.float16).astype(F)
    s = np.zeros((t.shape[0], len(docs)), F)
    for b, i in np.ndindex(t.shape):
        lo, hi = np.searchsorted(term, t[b, i]), np.searchsorted(term, t[b, i], "right")
        s[b, doc[lo:hi]] = qh[b, i] * wt[lo:hi] + s[b, doc[lo:hi]]
    return s


def make_docs(V, n_docs, n_top=None):
    """test_gpu_spindex_batch's documents: terms below V - 2, every fifth document ending in V - 1."""
    docs = PR.make_docs(V - 2, n_top or N_TOP[V], n_docs, seed=V + n_docs)
    for i in range(1, n_docs, 5):
        if len(docs[i][0]):
            docs[i] = (np.append(docs[i][0][:-1], V - 1).astype(np.int32), docs[i][1])
    return docs


def new_index(model, lib, V, docs, inv_block=None, room=0):
    ix = bertpy.BertSparseIndex(model, len(docs) + room, sum(-(-len(t) // 16) * 16 for t, _ in docs) + 16 + 16 * room,
                                n_top=max(len(t) for t, _ in docs) or 1, n_vocab=V)
    assert inv_block is None or lib.bertx_test_spindex_inv_block(ix.sp, inv_block) == 0
    return ix


@pytest.fixture(scope="module")
def refs():
    """(V, q_top, n_docs) -> (docs, terms, weights, inverted_ref of the 64 queries), computed once."""
    memo = {}

    def get(V, q_top, n_docs):
        if (V, q_top, n_docs) not in memo:
            if (V, n_docs) not in memo:
                memo[V, n_docs] = make_docs(V, n_docs)
            docs, (t, w) = memo[V, n_docs], queries(V, q_top)
            memo[V, q_top, n_docs] = (docs, t, w, inverted_ref(t, w, docs))
        return memo[V, q_top, n_docs]
    return get


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("V,q_top,k", SHAPES)
def test_bits(lib, model, refs, V, q_top, k, B):
    """Ids and score bits equal the restatement with blocks of 64 and of 256 documents at every store
    size: a partial block alone, exact block boundaries, many blocks on one workgroup and on three
    that merge; k above the number of documents gives the (-inf, -1) fill."""
    for n_docs in N_DOCS[V]:
        docs, t, w, ref = refs(V, q_top, n_docs)
        want_s, want_i = PR.topk_ref(ref[:B], k)
        for inv_block in (64, 256):
            ix = new_index(model, lib, V, docs, inv_block)
            assert ix.add_postings(docs) == 0 and ix.inverted_docs == 0
            ix.build_inverted()
            assert ix.inverted_docs == n_docs and lib.bertx_spindex_inv_block(ix.sp) == inv_block
            for cap in ((1, 3) if n_docs >= 257 else (0,)):
                assert lib.bertx_test_spindex_grid(ix.sp, cap) == 0
                got_s, got_i = ix.search_inverted(t[:B], w[:B], k)
                assert cap == 0 or lib.bertx_test_spindex_last_grid(ix.sp) == min(cap, -(-n_docs // inv_block))
                assert np.array_equal(got_i, want_i), (n_docs, inv_block, cap)
                assert np.array_equal(bits(got_s), bits(want_s)), (n_docs, inv_block, cap)


def test_default_block(lib, model):
    """One more document than the default block holds: a real block boundary with the full LDS request,
    and at V 130 the queries' lists of a block are several staging areas long."""
    V = 130
    probe = new_index(model, lib, V, [(np.zeros(1, np.int32), np.ones(1, F))])
    n_docs = lib.bertx_spindex_inv_block(probe.sp) + 1
    docs = make_docs(V, n_docs, n_top=8)
    t, w = queries(V, 32)
    t, w = t[[5, 1]], w[[5, 1]]
    ix = new_index(model, lib, V, docs)
    assert ix.add_postings(docs) == 0
    got_s, got_i = ix.search_inverted(t, w, 10)
    want_s, want_i = PR.topk_ref(inverted_ref(t, w, docs), 10)
    assert lib.bertx_spindex_inverted_bytes(ix.sp) > 0 and ix.inverted_docs == n_docs
    assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), bits(want_s))


def test_equals_sparse_search_where_sums_are_exact(lib, model):
    """Weights in eighths: every partial sum is exact in f32, the order of additions is immaterial and
    search_inverted equals search_sparse, ids and score bits."""
    V, rng = 30522, np.random.default_rng(8)
    docs = [(tt, (rng.integers(0, 17, len(tt)) / 8).astype(F)) for tt, _ in make_docs(V, 700)]
    t, w = queries(V, 32)
    w = (np.round(w * 8) / 8).astype(F)
    ix = new_index(model, lib, V, docs, 256)
    assert ix.add_postings(docs) == 0
    inv_s, inv_i = ix.search_inverted(t, w, 10)
    sp_s, sp_i = ix.search_sparse(t, w, 10)
    assert np.array_equal(inv_i, sp_i) and np.array_equal(bits(inv_s), bits(sp_s))


def test_incremental_build_and_staleness(lib, model, refs, dev, stream):
    """Add, build, add across a block boundary, build: the result of a store filled and built at once.
    A stale image refuses the device form and writes nothing; the host form builds by itself; clear()
    resets the image."""
    V, k, B = 130, 10, 5
    docs, t, w, ref = refs(V, 32, 257)
    want_s, want_i = PR.topk_ref(ref[:B], k)
    ix = new_index(model, lib, V, docs, 64)
    assert ix.add_postings(docs[:100]) == 0
    ix.build_inverted()
    assert ix.inverted_docs == 100 and ix.add_postings(docs[100:]) == 100 and ix.inverted_docs == 100
    d_t, d_w, d_s, d_i = dev.up(t[:B]), dev.up(w[:B]), dev.up(np.full((B, k), 3, F)), dev.up(np.full((B, k), 3, np.int32))
    assert lib.bertx_spindex_search_inverted_device(ix.sp, d_t, d_w, B, 32, k, d_s, d_i, stream) == -1
    assert np.all(dev.down(d_s, (B, k), F) == 3) and np.all(dev.down(d_i, (B, k), np.int32) == 3)
    assert lib.bertx_test_spindex_inv_block(ix.sp, 128) == -1          # something is inverted
    ix.build_inverted()
    assert ix.inverted_docs == 257
    assert lib.bertx_spindex_search_inverted_device(ix.sp, d_t, d_w, B, 32, k, d_s, d_i, stream) == 0
    assert dev.hip.hipStreamSynchronize(stream) == 0
    assert np.array_equal(dev.down(d_i, (B, k), np.int32), want_i)
    assert np.array_equal(bits(dev.down(d_s, (B, k), F)), bits(want_s))
    ix.clear()
    assert ix.inverted_docs == 0 and ix.add_postings(docs[:150]) == 0 and ix.add_postings(docs[150:]) == 150
    got_s, got_i = ix.search_inverted(t[:B], w[:B], k)                 # builds by itself
    assert ix.inverted_docs == 257 and np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), bits(want_s))


def test_texts_and_graph(lib, tok_golden, tmp_path, dev, stream):
    """search_texts(q_top = n, inverted = True) is search_inverted of forward_sparse_top's output; a
    captured device search replays the eager bits twice."""
    m = bertpy.BertModel(SR.make_sparse_models(lib, GOLDEN, str(tmp_path))["f16"])
    texts, new, _ = corpus_texts(tok_golden)
    n_top = 24
    ix = bertpy.BertSparseIndex(m, len(texts), len(texts) * 32, n_top=n_top)
    assert lib.bertx_test_spindex_inv_block(ix.sp, 64) == 0 and ix.add_texts(texts) == 0
    queries_ = texts[3:40:8] + new
    terms, wts, _ = m.forward_sparse_top([np.asarray(m.tokenize(t)[0], np.int32) for t in queries_], n_top)
    want_s, want_i = ix.search_inverted(terms, wts, 5)
    docs = [ix.doc(i) for i in range(len(ix))]
    ref_s, ref_i = PR.topk_ref(inverted_ref(terms, wts, docs), 5)
    assert np.array_equal(want_i, ref_i) and np.array_equal(bits(want_s), bits(ref_s))
    got_s, got_i = ix.search_texts(queries_, 5, q_top=n_top, inverted=True)
    assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), bits(want_s))
    B, k = len(queries_), 5
    d_t, d_w, d_s, d_i = dev.up(terms), dev.up(wts), dev.alloc(B * k * 4), dev.alloc(B * k * 4)
    replay_twice(dev, stream, lambda: lib.bertx_spindex_search_inverted_device(ix.sp, d_t, d_w, B, n_top, k, d_s, d_i, stream),
                 [(d_s, (B, k), F), (d_i, (B, k), np.int32)], [want_s, want_i])
