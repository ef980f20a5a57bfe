"""GPU tests of the hybrid dense + sparse search (hybrid.hip, spindex.cpp; bert_hip.h "Hybrid search"):
numpy applies the union and fusion rule to the library's own stage outputs (BertIndex.search,
search_sparse or search_inverted, both score_ids) in np.float32 arithmetic, one rounding per
operation; ids and score bits must be equal.  Never a tolerance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import sparse_refs as SR
import spindex_refs as PR
from test_gpu_search import corpus_texts
from test_gpu_search_bin import dev, replay_twice, same, stream  # noqa: F401
from test_gpu_spindex_batch import _one_device, model  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, V, N_TOP, Q_TOP = 300, 30522, 128, 32
MODES = [("linear", 1.0, 1.0), ("linear", 0.3, 2.5), ("rrf", 60.0, 1.0)]


@pytest.fixture(scope="module")
def world():
    """(rows f32 [N][64], documents, dense queries [64][64], sparse queries): query b's heavy terms
    100 + 2 b and 101 + 2 b are given to every other of its eight best dense rows, so the two
    candidate lists overlap partly; its other terms come from three documents."""
    rng = np.random.default_rng(11)
    rows, Q = (a / np.linalg.norm(a, axis=1, keepdims=True) for a in (rng.standard_normal((N, 64)), rng.standard_normal((64, 64))))
    docs = [dict(zip((t + 400).tolist(), w.tolist())) for t, w in PR.make_docs(V - 400, 40, N, seed=5)]
    t, w = np.full((64, Q_TOP), -1, np.int32), np.zeros((64, Q_TOP), F)
    for b in range(64):
        other = np.unique(np.concatenate([list(docs[r]) for r in rng.integers(0, N, 3)] + [np.zeros(0, int)]))
        other = rng.permutation(other[other >= 400])[:Q_TOP - 2]
        t[b, :2], w[b, :2] = (100 + 2 * b, 101 + 2 * b), (2.5, 1.5)
        t[b, 2:2 + len(other)], w[b, 2:2 + len(other)] = other, rng.uniform(0.1, 1.0, len(other))
        for r in np.argsort(-(Q[b] @ rows.T))[:8:2]:
            docs[r][100 + 2 * b] = docs[r][101 + 2 * b] = 2.0
    docs = [(np.array(sorted(d), np.int32), np.array([d[x] for x in sorted(d)], F)) for d in docs]
    return rows.astype(F), docs, Q.astype(F), t, w


def stores(model, world, n=N, storage="f16"):
    rows, docs = world[0][:n], world[1][:n]
    dense = bertpy.BertIndex(model, n + 8, storage=storage)
    sp = bertpy.BertSparseIndex(model, n + 8, sum(-(-len(t) // 16) * 16 for t, _ in docs) + 160, n_top=N_TOP, n_vocab=V)
    assert dense.add(rows) == 0 and sp.add_postings(docs) == 0
    sp.build_inverted()
    return dense, sp


@pytest.fixture(scope="module")
def full(model, world):
    return stores(model, world)


def compose(dense, sp, Q, t, w, k, n_cand, fusion, a, b, inverted):
    """The contract over the library's own stage outputs."""
    cd = dense.search(Q, n_cand)[1]
    cs = (sp.search_inverted if inverted else sp.search_sparse)(t, w, n_cand)[1]
    return fused(cd, cs, k, fusion, a, b, lambda U: (dense.score_ids(Q, U), sp.score_ids(t, w, U)))


def fused(cd, cs, k, fusion, a, b, scorers):
    """The stages' candidates -> their ascending union, both scorers (linear) or the positions (rrf),
    the fused score in single float32 operations, the k best."""
    n_cand = cd.shape[1]
    U = np.full((len(cd), 2 * n_cand), -1, np.int32)
    for i, both in enumerate(np.concatenate([cd, cs], axis=1)):
        u = np.unique(both[both >= 0])
        U[i, :len(u)] = u
    if fusion == "linear":
        sd, ss = scorers(U)
        ok = (U >= 0) & (sd != -np.inf) & (ss != -np.inf)
        with np.errstate(invalid="ignore"):
            f = F(a) * sd + F(b) * ss
    else:
        def rr(c):
            hit = (U[:, :, None] == c[:, None, :]) & (U[:, :, None] >= 0)
            return np.where(hit.any(2), F(1) / (F(a) + (hit.argmax(2) + 1).astype(F)), F(0))
        ok, f = U >= 0, rr(cd) + rr(cs)
    assert f.dtype == F
    f, ids = np.where(ok, f, F(-np.inf)), np.where(ok, U, -1)
    order = np.stack([np.lexsort((ids[i].astype(np.uint32), -f[i].astype(np.float64))) for i in range(len(U))])[:, :k]
    return np.take_along_axis(f, order, 1), np.take_along_axis(ids, order, 1)


@pytest.mark.parametrize("inverted", [False, True])
@pytest.mark.parametrize("fusion,a,b", MODES)
@pytest.mark.parametrize("n_cand,k", [(1, 1), (1, 2), (7, 10), (64, 128)])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_composition(full, world, B, n_cand, k, fusion, a, b, inverted):
    dense, sp = full
    Q, t, w = (x[:B] for x in world[2:])
    want = compose(dense, sp, Q, t, w, k, n_cand, fusion, a, b, inverted)
    assert same(sp.search_hybrid(dense, Q, t, w, k, n_cand, fusion, a, b, inverted), want)
    if (n_cand, fusion, inverted) == (7, "rrf", False):   # the lists overlap partly
        shared = sum(len(np.intersect1d(c, s)) for c, s in zip(dense.search(Q, 7)[1], sp.search_sparse(t, w, 7)[1]))
        assert 0 < shared < 7 * B


def test_int8_small_store_identities_and_deletion(model, world):
    """An int8 embedding index; stores of 40 ids under n_cand 64, so the fill appears and (a, b) = (0, 1)
    / (1, 0) are the single-store searches; a document deleted in one store only never comes back."""
    Q, t, w = (x[:5] for x in world[2:])
    dense, sp = stores(model, world, storage="int8")
    assert same(sp.search_hybrid(dense, Q, t, w, 10, 7), compose(dense, sp, Q, t, w, 10, 7, "linear", 1.0, 1.0, False))
    dense, sp = stores(model, world, 40)
    for fusion, a in (("linear", 1.0), ("rrf", None)):
        got = sp.search_hybrid(dense, Q, t, w, 100, 64, fusion, a)
        assert same(got, compose(dense, sp, Q, t, w, 100, 64, fusion, a or 60.0, 1.0, False))
        assert np.all(got[1][:, :40] >= 0) and np.all(got[1][:, 40:] == -1) and np.all(got[0][:, 40:] == -np.inf)
    assert same(sp.search_hybrid(dense, Q, t, w, 10, 64, "linear", 0.0, 1.0), sp.search_sparse(t, w, 10))
    assert same(sp.search_hybrid(dense, Q, t, w, 10, 64, "linear", 1.0, 0.0, inverted=True), dense.search(Q, 10))
    best = sp.search_hybrid(dense, Q, t, w, 3, 64)[1]
    dense.remove(best[:, 0])
    sp.remove(best[:, 1])
    got = sp.search_hybrid(dense, Q, t, w, 40, 64)
    assert same(got, compose(dense, sp, Q, t, w, 40, 64, "linear", 1.0, 1.0, False))
    assert not np.isin(got[1], best[:, :2]).any() and np.all((got[1] >= 0).sum(1) == 40 - len(np.unique(best[:, :2])))


def test_texts(lib, tok_golden, tmp_path):
    """The text form against the text forms of its stages (reciprocal ranks need no scores), and the
    linear form against the array form on the queries' own sparse weights."""
    m = bertpy.BertModel(SR.make_sparse_models(lib, GOLDEN, str(tmp_path))["f16"])
    texts, new, _ = corpus_texts(tok_golden)
    dense, sp = bertpy.BertIndex(m, len(texts)), bertpy.BertSparseIndex(m, len(texts), len(texts) * 32, n_top=24)
    assert dense.add_texts(texts) == 0 and sp.add_texts(texts) == 0
    ask = texts[3:40:8] + new
    cd, cs = dense.search_texts(ask, 7)[1], sp.search_texts(ask, 7, q_top=24)[1]
    assert same(sp.search_hybrid_texts(dense, m, ask, 10, 24, 7, "rrf"), fused(cd, cs, 10, "rrf", 60.0, 1.0, None))
    got = sp.search_hybrid_texts(dense, m, ask, 10, 24, 7, "linear", 0.0, 1.0)
    terms, wts, _ = m.forward_sparse_top([np.asarray(m.tokenize(q)[0], np.int32) for q in ask], 24)
    ss = lambda U: (np.zeros(U.shape, F), sp.score_ids(terms, wts, U))
    assert same(got, fused(cd, cs, 10, "linear", 0.0, 1.0, ss))


def test_the_tool(lib, tok_golden, tmp_path):
    """build/bin/search -H prints search_hybrid_texts' fused hits (the inverted first stage) over the
    same two stores, with the defaults and with every option; :del removes from both stores."""
    path = SR.make_sparse_models(lib, GOLDEN, str(tmp_path))["f16"]
    m, texts = bertpy.BertModel(path), corpus_texts(tok_golden)[0][:40]
    (tmp_path / "corpus.txt").write_text("\n".join(texts) + "\n")
    dense, sp = bertpy.BertIndex(m, 40), bertpy.BertSparseIndex(m, 40, 40 * 128, n_top=128)
    assert dense.add_texts(texts) == 0 and sp.add_texts(texts) == 0
    tool = [os.path.join(os.path.dirname(GOLDEN), "..", "build", "bin", "search"), "-m", path, "-f", str(tmp_path / "corpus.txt"),
            "-k", "3", "-H", path]
    for args, kw in (([], dict(q_top=32, n_cand=12)), (["-F", "rrf", "-q", "16", "-c", "5", "-w", "30,1"],
                                                       dict(q_top=16, n_cand=5, fusion="rrf", a=30.0))):
        def hits():
            s, i = sp.search_hybrid_texts(dense, m, [texts[3]], 3, inverted=True, **kw)
            return ["%d\t%d\t%.4f\t%s" % (j + 1, d, f, texts[d]) for j, (f, d) in enumerate(zip(s[0], i[0])) if d >= 0], i[0, :1]
        first, gone = hits()
        dense.remove(gone)
        sp.remove(gone)
        want = first + ["deleted 1"] + hits()[0]
        r = subprocess.run(tool + args, input="%s\n:del %d\n%s\nq\n" % (texts[3], gone[0], texts[3]), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = [ln for ln in r.stdout.splitlines() if "deleted" in ln or (len(ln.split("\t")) == 4 and ln.split("\t")[0].isdigit())]
        assert got == want and len(first) == 3 and str(gone[0]) not in [ln.split("\t")[1] for ln in want[4:]]
        dense.clear(), sp.clear()
        assert dense.add_texts(texts) == 0 and sp.add_texts(texts) == 0
    assert subprocess.run(tool + ["-l"], input="q\n", capture_output=True, text=True, timeout=120).returncode == 2


def test_refusals_and_capture(lib, model, world, dev, stream):
    """Refusals of the device form leave the outputs untouched; the first call allocates and is not
    capturable, the second one captured and replayed twice gives the eager bits."""
    B, k, n_cand = 5, 10, 7
    Q, t, w = (x[:B] for x in world[2:])
    dense, sp = stores(model, world)
    d_q, d_t, d_w = dev.up(Q), dev.up(t), dev.up(w)
    d_s, d_i = dev.up(np.full((B, k), 3, F)), dev.up(np.full((B, k), 3, np.int32))
    call = lambda *a: lib.bertx_hybrid_search_device(*a, d_s, d_i, stream)
    good = (dense.idx, sp.sp, d_q, d_t, d_w, B, Q_TOP, k, n_cand, 0, 1.0, 1.0)
    hip, graph = dev.hip, ctypes.c_void_p()
    for at, bad in ((7, 0), (7, 15), (8, 65), (8, 0), (5, 65), (9, 2), (9, 8), (0, None), (1, None), (2, None), (3, None),
                    (4, None)):
        assert call(*good[:at], bad, *good[at + 1:]) < 0
    assert sp.add_postings(world[1][:1]) == N                  # the inverted image is stale now
    assert call(*good[:9], 16, *good[10:]) == -1
    assert lib.bertx_hybrid_search_device(*good, None, d_i, stream) < 0 and hip.hipStreamSynchronize(stream) == 0
    assert np.all(dev.down(d_s, (B, k), F) == 3) and np.all(dev.down(d_i, (B, k), np.int32) == 3)
    assert dense.add(world[0][:1]) == N
    assert hip.hipStreamBeginCapture(stream, 1) == 0           # thread-local mode
    rc = call(*good)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0 and rc == -2
    hip.hipGraphDestroy(graph)
    for mode, fusion in ((0, "linear"), (1, "rrf")):
        args = good[:9] + (mode,) + good[10:]
        assert call(*args) == 0 and hip.hipStreamSynchronize(stream) == 0
        eager = (dev.down(d_s, (B, k), F), dev.down(d_i, (B, k), np.int32))
        assert same(eager, compose(dense, sp, Q, t, w, k, n_cand, fusion, 1.0, 1.0, False))
        replay_twice(dev, stream, lambda: call(*args), [(d_s, (B, k), F), (d_i, (B, k), np.int32)], eager)
