"""The numpy reference of the int8 token store (maxsim_i8_refs.py) checked against a
restatement of itself, the contract's accuracy bound and exactness claims checked on the
GPU tests' own inputs, and the ABI surface that needs no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import bertpy
import maxsim_i8_refs as R
import maxsim_refs as M
from conftest import GOLDEN, LIB_SO

NEW_SYMBOLS = ["bertx_mvindex_create_ex", "bertx_mvindex_storage", "bertx_mvindex_doc_i8", "bertx_bench_maxsim_ex"]


def ref_scores(q, docs):
    qp = R.pack(q)
    return np.array([R.score(qp, R.pack(d)) for d in docs], np.float32)


def test_reference_agrees_with_three_loops():
    rng = np.random.default_rng(1)
    for w, Lq, n in ((64, 1, 1), (64, 17, 5), (192, 33, 3), (64, 64, 2)):
        qp, dp = R.pack(M.token_rows(rng, Lq, w)), R.pack(M.token_rows(rng, n, w))
        a, b = R.score(qp, dp), R.score_loops(qp, dp)
        assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32), (w, Lq, n, a, b)
    # a zero row: zeros with u == 0; its similarities are 0, not NaN
    q, u = R.pack(np.zeros((2, 64), np.float32))
    assert not q.any() and not u.any()
    x = M.token_rows(rng, 3, 64)
    assert R.score(R.pack(x), (q, u)) == 0.0
    # the dequantized row has unit length to f32 rounding
    q, u = R.pack(M.token_rows(rng, 8, 192))
    assert np.abs(np.linalg.norm(q.astype(np.float64) * u[:, None].astype(np.float64), axis=1) - 1.0).max() < 2.0 ** -22


def every_input():
    for w in R.WIDTHS:
        yield from M.pack_case(w)
        docs, queries = M.parity_case(w)
        yield from docs
        yield from queries.values()
        for n in (17, 33):
            yield from M.planted_last(w, n)
        for Lq in (1, 17):
            yield from M.planted_negative(w, Lq)
    for case in M.RANKING_CASES:
        q, docs, _ = M.ranking_corpus(*case)
        yield q
        yield from docs


def test_norms_are_exact_integers_below_2_to_24():
    worst = 0
    for x in every_input():
        n2 = R.n2_of(R.pack(x)[0])
        worst = max(worst, int(n2.max()))
        assert np.array_equal(n2.astype(np.float32).astype(np.int64), n2)
    print("largest n2: %d (2^24 = %d)" % (worst, 2 ** 24))
    assert worst < 2 ** 24


@pytest.mark.parametrize("w", (64, 192, 768))
def test_accuracy_bound_holds_for_the_reference(w):
    """|sim - cos| <= 2 (e_x + e_y) + 2^-21 for every pair of parity_case(w)."""
    docs, queries = M.parity_case(w)
    worst, worst_abs = 0.0, 0.0
    for q in queries.values():
        qp = R.pack(q)
        for d in docs:
            dp = R.pack(d)
            sims = R.S.ref_scores_i8(qp[0], qp[1], dp[0], dp[1]).astype(np.float64)
            err = np.abs(sims - M.normalise(q) @ M.normalise(d).T)
            worst = max(worst, float((err / R.sim_bound(q, d)).max()))
            worst_abs = max(worst_abs, float(err.max()))
    print("w = %d: worst error / bound %.3f, worst absolute error %.2e" % (w, worst, worst_abs))
    assert worst <= 1.0


@pytest.mark.parametrize("w,Lq,N,seed", M.RANKING_CASES)
def test_reference_reproduces_the_planted_order(w, Lq, N, seed):
    q, docs, order = M.ranking_corpus(w, Lq, N, seed)
    scores = ref_scores(q, docs)
    exact = np.array([R.exact_maxsim(q, d) for d in docs])
    print("w = %d: min gap %.3f, max |int8 - exact| %.2e" % (w, M.min_gap(scores), np.abs(scores - exact).max()))
    assert np.array_equal(np.argsort(-scores, kind="stable"), order)


@pytest.mark.parametrize("w", R.WIDTHS)
def test_planted_rows(w):
    for n in (17, 33):
        q, doc = M.planted_last(w, n)
        with_last, without = ref_scores(q, [doc, doc[:-1]])
        assert abs(float(with_last) - 1.0) <= 2.0 ** -22, with_last      # the last row counts ...
        assert abs(float(without)) < 0.01, without                        # ... and without it the score is about 0
    for Lq in (1, 17):
        q, doc = M.planted_negative(w, Lq)
        assert abs(float(ref_scores(q, [doc])[0]) + Lq) <= Lq * 2.0 ** -22


def test_library_exports_the_new_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_SO], capture_output=True, text=True, check=True).stdout
    have = set(re.findall(r"\bT (bertx_\w+)", out))
    missing = [s for s in NEW_SYMBOLS if s not in have]
    assert not missing, missing
    lib = bertpy.load_lib()
    for s in NEW_SYMBOLS:
        assert getattr(lib, s).argtypes is not None


def test_unknown_storage_raises_before_the_library_is_called():
    for bad in ("int4", "i8", None, 1):
        with pytest.raises(ValueError):
            bertpy.BertTokenIndex(None, 8, 256, storage=bad)


def test_create_ex_on_a_tokenizer_only_context_returns_null(capfd):
    old = os.environ.get("BERT_HOST_ONLY")
    os.environ["BERT_HOST_ONLY"] = "1"
    try:
        m = bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))
        for kind in (0, 1, 2):
            assert not m.lib.bertx_mvindex_create_ex(m.ctx, 0, 64, 8, 256, kind)
        with pytest.raises(RuntimeError):
            bertpy.BertTokenIndex(m, 8, 256, storage="int8")
        assert m.lib.bertx_mvindex_storage(None) == -1
    finally:
        if old is None:
            os.environ.pop("BERT_HOST_ONLY", None)
        else:
            os.environ["BERT_HOST_ONLY"] = old
