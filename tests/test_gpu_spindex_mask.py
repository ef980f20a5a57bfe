"""GPU tests of the sparse index's tombstones and filters (bert_hip.h "Sparse index", "Deleting
documents and filtered search"): the three searches over the admissible documents against the
numpy restatements of their scores and search_mask_refs.select.  Ids and score bits, never a
tolerance."""
import ctypes
import os

import numpy as np
import pytest

import bertpy
import search_mask_refs as SM
import sparse_refs as SR
import spindex_refs as PR
from test_gpu_search import corpus_texts
from test_gpu_search_bin import dev, stream  # noqa: F401
from test_gpu_spindex_batch import _one_device, densify, model, queries  # noqa: F401
from test_gpu_spindex_inverted import inverted_ref, make_docs, new_index

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ["dense", "sparse", "inverted"]
N_DOCS = [31, 32, 33, 64, 65, 2100]
SHAPES = [(130, 16, 1, 5), (130, 16, 10, 64), (30522, 32, 10, 1), (30522, 32, 128, 64)]   # V, q_top, k, B


def search(ix, kind, t, w, k, allow=None):
    if kind == "dense":
        return ix.search(densify(t, w, ix.n_vocab), k, allow)
    return (ix.search_sparse if kind == "sparse" else ix.search_inverted)(t, w, k, allow)


def scores_of(kind, t, w, V, docs):
    return inverted_ref(t, w, docs) if kind == "inverted" else PR.scores_ref(densify(t, w, V), docs)[0]


def device_search(lib, ix, kind, d_t, d_w, d_q, B, q_top, k, filt, d_s, d_i, stream):
    """The filtered device entry of `kind`; filt = (pointer, n_filters, words)."""
    if kind == "dense":
        return lib.bertx_spindex_search_filtered_device(ix.sp, d_q, B, k, *filt, d_s, d_i, stream)
    fn = lib.bertx_spindex_search_sparse_filtered_device if kind == "sparse" else lib.bertx_spindex_search_inverted_filtered_device
    return fn(ix.sp, d_t, d_w, B, q_top, k, *filt, d_s, d_i, stream)


def removals(N, block, best):
    """name -> ids: the removal patterns over N documents in blocks of `block`."""
    blocks = sorted({0, (N - 1) // block // 2, (N - 1) // block})
    pats = {"none": [], "edges": [i for i in (0, 31, 32, 63, 64, N - 1) if i < N], "every other": range(0, N, 2),
            "a word": range(32, min(64, N)), "all": range(N), "the best": best}
    pats.update({"block %d" % b: range(b * block, min((b + 1) * block, N)) for b in blocks})
    return {name: np.asarray(list(ids), np.int32) for name, ids in pats.items()}


def with_garbage(f, N):
    """The packed words of filter(s) f, one word more than needed, every bit at and above N set."""
    return SM.pack_bits(np.concatenate([f, np.ones(f.shape[:-1] + (32 * (SM.words_for(N) + 1) - N,), bool)], axis=-1))


@pytest.mark.parametrize("V,q_top,k,B", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_masked_bits(lib, model, kind, V, q_top, k, B):
    """Every removal pattern (word edges, whole words, whole blocks so that the inverted search skips,
    everything, every query's best document) under no filter, one shared filter and B filters with
    spare words and garbage bits above docs: the k best admissible documents of the reference."""
    rng = np.random.default_rng(V + k)
    t, w = (a[:B] for a in queries(V, q_top))
    few = many = False
    for N in N_DOCS:
        docs = make_docs(V, N)
        S = scores_of(kind, t, w, V, docs)
        shared = rng.random(N) < 0.5
        own = rng.random((B, N)) < np.linspace(0.02, 0.9, B)[:, None]
        own[0] = np.arange(N) % 11 == 3                       # few documents for query 0
        for block in ((64, 256) if kind == "inverted" else (64,)):
            ix = new_index(model, lib, V, docs, block)
            for name, gone in removals(N, block, S.argmax(axis=1)).items():
                ix.clear()
                assert ix.add_postings(docs) == 0
                if len(gone):
                    ix.remove(gone)
                dead = SM.tombstones(N, gone)
                assert ix.live() == N - dead.sum() and np.array_equal(ix.deleted(0, N), dead)
                for cap in ((1, 3) if N == 2100 else (0,)):
                    assert lib.bertx_test_spindex_grid(ix.sp, cap) == 0
                    for f, allow in ((None, None), (shared, shared), (own, with_garbage(own, N))):
                        adm = SM.admissible(N, B, dead, f)
                        few |= bool(((adm.sum(1) > 0) & (adm.sum(1) < k)).any())
                        many |= bool((adm.sum(1) >= k).any())
                        got = search(ix, kind, t, w, k, allow)
                        assert SM.same(got, SM.select(S, adm, k)), (N, block, name, cap, f is own)
                        assert lib.bertx_test_spindex_last_masked(ix.sp) == int(len(gone) > 0 or f is not None)
    assert many and (few or k == 1)


@pytest.mark.parametrize("kind", KINDS)
def test_remove_clear_and_refusals(lib, model, dev, stream, kind):
    """remove ignores ids outside the store and repeats; refusals change nothing and leave the outputs
    untouched; a removal needs no rebuild of the inverted image; clear() followed by adds starts
    clean, with the unmasked kernels again; (NULL, 0, 0) is the unfiltered entry."""
    V, q_top, k, B, N = 130, 16, 10, 5, 257
    docs = make_docs(V, N)
    t, w = (a[:B] for a in queries(V, q_top))
    S = scores_of(kind, t, w, V, docs)
    ix = new_index(model, lib, V, docs, 64, room=8)
    assert ix.add_postings(docs) == 0
    plain = search(ix, kind, t, w, k)
    assert lib.bertx_test_spindex_last_masked(ix.sp) == 0 and SM.same(plain, PR.topk_ref(S, k))
    d_t, d_w, d_q = dev.up(t), dev.up(w), dev.up(densify(t, w, V))
    d_s, d_i = dev.up(np.full((B, k), 3, F)), dev.up(np.full((B, k), 3, np.int32))
    out = lambda: (dev.down(d_s, (B, k), F), dev.down(d_i, (B, k), np.int32))
    assert device_search(lib, ix, kind, d_t, d_w, d_q, B, q_top, k, (None, 0, 0), d_s, d_i, stream) == 0
    assert dev.hip.hipStreamSynchronize(stream) == 0 and SM.same(out(), plain)
    assert lib.bertx_test_spindex_last_masked(ix.sp) == 0
    built = ix.inverted_docs
    # removal
    assert lib.bertx_spindex_remove(ix.sp, None, 3) < 0 and lib.bertx_spindex_remove(ix.sp, d_t, 0) < 0
    assert ix.live() == N and lib.bertx_test_spindex_last_masked(ix.sp) == 0
    gone = np.array([5, 64, 64, -1, N, N + 3, 256, 2 ** 30], np.int32)
    ix.remove(gone)
    dead = SM.tombstones(N, gone)
    assert ix.live() == N - 3 and len(ix) == N and ix.inverted_docs == built
    assert np.array_equal(ix.deleted(0, N), dead) and np.array_equal(ix.deleted(64, 1), [True])
    probe = np.full(4, 7, np.uint8)
    assert lib.bertx_spindex_deleted(ix.sp, N - 2, 3, probe.ctypes.data) == -1 and np.all(probe == 7)
    assert np.array_equal(ix.doc(64)[0], docs[64][0])
    assert SM.same(search(ix, kind, t, w, k), SM.select(S, ~dead, k)) and lib.bertx_test_spindex_last_masked(ix.sp) == 1
    # refusals of the filtered device entry: the outputs keep the sentinel
    for p, v in ((d_s, F), (d_i, np.int32)):
        dev.fill(p, (B, k), v, 3)
    words = SM.words_for(N)
    d_f = dev.up(SM.pack_bits(np.ones((B, N), bool)))
    for filt in ((d_f, 2, words), (d_f, B, words - 1), (d_f, 0, words), (None, 1, words), (d_f, -1, words)):
        assert device_search(lib, ix, kind, d_t, d_w, d_q, B, q_top, k, filt, d_s, d_i, stream) == -1
    assert device_search(lib, ix, kind, d_t, d_w, d_q, B, q_top, 129, (d_f, B, words), d_s, d_i, stream) == -1
    if kind == "inverted":                                    # a stale image refuses, filter or not
        assert ix.add_postings(docs[:1]) == N
        assert device_search(lib, ix, kind, d_t, d_w, d_q, B, q_top, k, (d_f, B, words), d_s, d_i, stream) == -1
    assert dev.hip.hipStreamSynchronize(stream) == 0
    assert all(np.all(a == 3) for a in out())
    # clear
    ix.clear()
    assert ix.add_postings(docs) == 0 and ix.live() == N and not ix.deleted(0, N).any()
    assert SM.same(search(ix, kind, t, w, k), plain) and lib.bertx_test_spindex_last_masked(ix.sp) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_captured_search_reads_the_filter_at_replay(lib, model, dev, stream, kind):
    """A captured filtered device search with B filters, replayed after the filter buffer was rewritten
    in place: each replay follows the bits the buffer holds then."""
    V, q_top, k, B, N = 130, 16, 10, 5, 300
    rng = np.random.default_rng(3)
    docs = make_docs(V, N)
    t, w = (a[:B] for a in queries(V, q_top))
    S = scores_of(kind, t, w, V, docs)
    ix = new_index(model, lib, V, docs, 64)
    assert ix.add_postings(docs) == 0
    ix.build_inverted()
    ix.remove([7, 200])
    dead = SM.tombstones(N, [7, 200])
    filters = [rng.random((B, N)) < 0.5, rng.random((B, N)) < 0.02]
    d_t, d_w, d_q, d_f = dev.up(t), dev.up(w), dev.up(densify(t, w, V)), dev.up(SM.pack_bits(filters[0]))
    d_s, d_i = dev.alloc(B * k * 4), dev.alloc(B * k * 4)
    hip, graph, ex = dev.hip, ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 1) == 0          # thread-local mode
    rc = device_search(lib, ix, kind, d_t, d_w, d_q, B, q_top, k, (d_f, B, SM.words_for(N)), d_s, d_i, stream)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0 and rc == 0
    assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, 0) == 0
    for f in filters + filters[:1]:
        packed = SM.pack_bits(f)
        assert hip.hipMemcpy(d_f, packed.ctypes.data, packed.nbytes, 1) == 0
        dev.fill(d_s, (B, k), F, 3)
        dev.fill(d_i, (B, k), np.int32, 3)
        assert hip.hipGraphLaunch(ex, stream) == 0 and hip.hipStreamSynchronize(stream) == 0
        got = (dev.down(d_s, (B, k), F), dev.down(d_i, (B, k), np.int32))
        assert SM.same(got, SM.select(S, SM.admissible(N, B, dead, f), k))
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)


def test_texts_after_removal(lib, tok_golden, tmp_path):
    """The text forms on a store with deletions: two documents the inverted text search returned are
    removed, and the next call returns the reference over the rest; allow= limits it further."""
    m = bertpy.BertModel(SR.make_sparse_models(lib, GOLDEN, str(tmp_path))["f16"])
    texts, new, _ = corpus_texts(tok_golden)
    n_top, k = 24, 5
    ix = bertpy.BertSparseIndex(m, len(texts), len(texts) * 32, n_top=n_top)
    assert lib.bertx_test_spindex_inv_block(ix.sp, 64) == 0 and ix.add_texts(texts) == 0
    queries_ = texts[3:40:8] + new
    _, before = ix.search_texts(queries_, k, q_top=n_top, inverted=True)
    gone = before[0, :2]
    ix.remove(gone)
    terms, wts, _ = m.forward_sparse_top([np.asarray(m.tokenize(q)[0], np.int32) for q in queries_], n_top)
    docs = [ix.doc(i) for i in range(len(ix))]
    dead = SM.tombstones(len(ix), gone)
    want = SM.select(inverted_ref(terms, wts, docs), ~dead, k)
    assert SM.same(ix.search_texts(queries_, k, q_top=n_top, inverted=True), want) and not np.isin(want[1], gone).any()
    assert SM.same(ix.search_texts(queries_, k, q_top=n_top), SM.select(PR.scores_ref(densify(terms, wts, ix.n_vocab), docs)[0], ~dead, k))
    allow = np.arange(len(ix)) % 3 != 0
    want = SM.select(inverted_ref(terms, wts, docs), SM.admissible(len(ix), len(queries_), dead, allow), k)
    assert SM.same(ix.search_texts(queries_, k, q_top=n_top, inverted=True, allow=allow), want)
