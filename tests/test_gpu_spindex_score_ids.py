"""GPU tests of the sparse index's scorer of listed documents (sparse_gather.hip; bert_hip.h "Sparse
index", "Listed documents"): score bits against the numpy restatement of the document-major contract
on the densified queries (spindex_refs.scores_ref) and against the search's own output, -inf exactly
for the ids the store does not hold or has deleted.  Never a tolerance."""
import numpy as np
import pytest

import bertpy
import spindex_refs as PR
from row_kernel_refs import bits
from test_gpu_search_bin import dev, stream  # noqa: F401
from test_gpu_spindex_batch import _one_device, densify, model  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
N_TOP = 130                                   # up to 9 units: two full load rounds of four and one more
SHAPES = [(1000, 1), (30522, 32), (65536, 1024)]
NS = [1, 5, 128]
GONE = np.array([0, 3, 31, 32, 100, 306], np.int32)


def make_store(V):
    """About 300 make_docs documents over the low terms (so that queries hit often), then planted ones
    of 0, 1, 15, 16, 17 and N_TOP postings, where the lane assignment and the load rounds change, and
    one that ends in term V - 1."""
    rng = np.random.default_rng(V)
    low = min(V - 1, 2048)
    docs = PR.make_docs(low, N_TOP, 300, seed=V)
    for L in (0, 1, 15, 16, 17, N_TOP):
        docs.append((np.sort(rng.permutation(low)[:L]).astype(np.int32), rng.uniform(0, 3, L).astype(np.float16).astype(F)))
    docs.append((np.append(docs[-1][0][:20], V - 1).astype(np.int32), docs[-1][1][:21]))
    return docs


def make_queries(V, q_top):
    """64 queries over the documents' terms, weights in (-0.5, 3); query 1 asks for term V - 1 in its
    first slot, query 2 is empty."""
    rng = np.random.default_rng(V + q_top)
    low = min(V - 1, 2048)
    t, w = np.full((64, q_top), -1, np.int32), np.zeros((64, q_top), F)
    for b in range(64):
        c = int(rng.integers(1, min(q_top, low) + 1))
        t[b, :c], w[b, :c] = rng.permutation(low)[:c], rng.uniform(-0.5, 3.0, c)
    t[1, 0] = V - 1
    t[2], w[2] = -1, 0
    return t, w


@pytest.fixture(scope="module")
def refs():
    """(V, q_top) -> (docs, terms, weights, scores_ref of the 64 queries), computed once."""
    memo = {}

    def get(V, q_top):
        if (V, q_top) not in memo:
            docs, (t, w) = make_store(V), make_queries(V, q_top)
            memo[V, q_top] = (docs, t, w, PR.scores_ref(densify(t, w, V), docs)[0])
        return memo[V, q_top]
    return get


def new_index(model, docs, V):
    ix = bertpy.BertSparseIndex(model, len(docs), sum(-(-len(t) // 16) * 16 for t, _ in docs) + 16, n_top=N_TOP, n_vocab=V)
    assert ix.add_postings(docs) == 0
    return ix


def id_lists(rng, B, n, N):
    """Random ids; a third of the entries replaced by -1, N, N + 5 and the ids of GONE; a repeated id."""
    ids = rng.integers(0, N, (B, n)).astype(np.int32)
    at = rng.permutation(B * n)[:B * n // 3]
    ids.ravel()[at] = rng.choice(np.concatenate([[-1, N, N + 5], GONE]), len(at))
    ids[:, n // 2] = ids[:, 0]
    return ids


def expected(ref, ids, dead):
    ok = (ids >= 0) & (ids < ref.shape[1])
    safe = np.where(ok, ids, 0)
    return np.where(ok & ~dead[safe], np.take_along_axis(ref[:len(ids)], safe, axis=1), F(-np.inf)).astype(F)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("V,q_top", SHAPES)
def test_bits(lib, model, refs, dev, stream, V, q_top, n):
    """The listed pairs' bits on a store with nothing removed (the instantiation without the tombstone
    test) and after a removal (the other one); the search's own ids give the search's own bits; the
    device form writes B n scores and nothing behind them."""
    B = [1, 5, 64][(SHAPES.index((V, q_top)) + NS.index(n)) % 3]
    docs, t, w, ref = refs(V, q_top)
    t, w, N = t[:B], w[:B], len(docs)
    ix = new_index(model, docs, V)
    rng = np.random.default_rng(n)
    dead = np.zeros(N, bool)
    for masked in (0, 1):
        if masked:
            ix.remove(GONE)
            dead[GONE] = True
        ids = id_lists(rng, B, n, N)
        assert np.array_equal(bits(ix.score_ids(t, w, ids)), bits(expected(ref, ids, dead)))
        assert lib.bertx_test_spindex_last_masked(ix.sp) == masked
        found_s, found_i = ix.search_sparse(t, w, n)
        assert np.array_equal(bits(ix.score_ids(t, w, found_i)), bits(found_s))
    d_s = dev.up(np.full(B * n + 64, 3, F))
    assert lib.bertx_spindex_score_ids_device(ix.sp, dev.up(t), dev.up(w), B, q_top, dev.up(ids), n, d_s, stream) == 0
    assert dev.hip.hipStreamSynchronize(stream) == 0
    got = dev.down(d_s, (B * n + 64,), F)
    assert np.array_equal(bits(got[:B * n]), bits(expected(ref, ids, dead)).ravel()) and np.all(got[B * n:] == 3)


def test_repeated_term_and_refusals(lib, model, refs, dev, stream):
    """Of a term repeated within a query the highest slot counts, within one stride of the image's build
    and across strides (the device form; the host form refuses the query).  Refusals write nothing."""
    V, q_top, n = 30522, 600, 7
    docs, _, _, _ = refs(V, 32)
    ix = new_index(model, docs, V)
    t, w = make_queries(V, q_top)
    t, w = t[:2].copy(), w[:2].copy()
    t[:, 0:8] = t[:, 590:598] = -1
    hot = docs[26][0][:2]                                      # terms of an N_TOP-posting document
    t[np.isin(t, hot)] = -1
    t[0, [3, 5, 515]], w[0, [3, 5, 515]] = hot[0], (1.0, 2.0, 0.75)
    t[1, [4, 597]], w[1, [4, 597]] = hot[1], (2.5, -1.5)
    kept_t, kept_w = t.copy(), w.copy()
    kept_t[0, [3, 5]] = kept_t[1, 4] = -1                      # what the repeats leave
    ids = np.array([[26, 0, 5, 305, 100, -1, 26], [26, 1, 2, 3, 4, 5, 6]], np.int32)
    want = expected(PR.scores_ref(densify(kept_t, kept_w, V), docs)[0], ids, np.zeros(len(docs), bool))
    d_t, d_w, d_i, d_s = dev.up(t), dev.up(w), dev.up(ids), dev.up(np.full((2, n), 3, F))
    assert lib.bertx_spindex_score_ids_device(ix.sp, d_t, d_w, 2, q_top, d_i, n, d_s, stream) == 0
    assert dev.hip.hipStreamSynchronize(stream) == 0
    assert np.array_equal(bits(dev.down(d_s, (2, n), F)), bits(want))
    assert np.array_equal(bits(ix.score_ids(kept_t, kept_w, ids)), bits(want))
    out = np.full((2, n), 3, F)
    assert lib.bertx_spindex_score_ids(ix.sp, t.ctypes.data, w.ctypes.data, 2, q_top, ids.ctypes.data, n, out.ctypes.data) == -1
    dev.fill(d_s, (2, n), F, 3)
    for args in ((d_t, d_w, 65, q_top, d_i, n, d_s), (d_t, d_w, 2, 1025, d_i, n, d_s), (d_t, d_w, 2, q_top, d_i, 129, d_s),
                 (d_t, d_w, 2, q_top, d_i, 0, d_s), (None, d_w, 2, q_top, d_i, n, d_s), (d_t, d_w, 2, q_top, None, n, d_s)):
        assert lib.bertx_spindex_score_ids_device(ix.sp, *args, stream) == -1
    assert dev.hip.hipStreamSynchronize(stream) == 0
    assert np.all(dev.down(d_s, (2, n), F) == 3) and np.all(out == 3)
