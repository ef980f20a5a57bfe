"""The numpy reference of the token store (maxsim_refs.py) checked against itself, the
tolerances of the contract checked on the GPU tests' own inputs with an f32 emulation,
the ranking corpora's gaps, and the ABI surface that needs no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import bertpy
import maxsim_refs as M
from conftest import GOLDEN, LIB_SO

SYMBOLS = ["create", "free", "clear", "docs", "token_slots", "capacity_docs", "capacity_token_slots", "dim", "add",
           "add_device", "doc_len", "doc", "score", "score_device", "add_texts", "score_text"]


def test_reference_agrees_with_three_loops():
    rng = np.random.default_rng(1)
    for w, Lq, n in ((64, 1, 1), (64, 3, 17), (192, 5, 9)):
        q, c = M.f16_view(M.token_rows(rng, Lq, w)), M.f16_view(M.token_rows(rng, n, w))
        a, b = M.maxsim(q, c), M.maxsim_loops(q, c)
        assert abs(a - b) <= 1e-12 * max(1.0, abs(b))
    # negative similarities: the max of negatives is negative, not 0
    v = M.f16_view(M.unit_rows(rng, 1, 64))
    assert M.maxsim(v, -np.repeat(v, 3, axis=0)) < -0.99
    # a zero row normalises to zeros
    assert not M.normalise(np.zeros((2, 64))).any() and not M.f16_view(np.zeros((2, 64), np.float32)).any()


@pytest.mark.parametrize("w", M.WIDTHS + (1024,))
def test_emulated_pack_is_inside_the_element_tolerance(w):
    worst = 0.0
    for rows in M.pack_case(w) + M.parity_case(w)[0][:6]:
        got, want = M.f16_view(rows).astype(np.float64), M.normalise(rows)
        ratio = np.abs(got - want) / M.elem_tol(want, w)
        worst = max(worst, float(ratio.max()))
    print("worst element error / bound at w = %d: %.3f" % (w, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("w", M.WIDTHS)
def test_emulated_score_is_inside_the_score_tolerance(w):
    docs, queries = M.parity_case(w)
    d16 = [M.f16_view(d) for d in docs]
    for Lq, q in queries.items():
        q16 = M.f16_view(q)
        for c in d16:
            err = abs(M.maxsim_f32(q16, c) - M.maxsim(q16, c))
            assert err <= M.score_tol(Lq, w), (w, Lq, len(c), err)
    for n in (17, 33):
        q, doc = M.planted_last(w, n)
        q16, c16 = M.f16_view(q), M.f16_view(doc)
        assert abs(M.maxsim(q16, c16) - 1.0) < 2e-3          # the last row counts ...
        assert abs(M.maxsim(q16, c16[:-1])) < 1e-2            # ... and without it the score is about 0
        assert abs(M.maxsim_f32(q16, c16) - M.maxsim(q16, c16)) <= M.score_tol(1, w)
    for Lq in (1, 17):
        q, doc = M.planted_negative(w, Lq)
        q16, c16 = M.f16_view(q), M.f16_view(doc)
        assert abs(M.maxsim(q16, c16) + Lq) < 2e-3 * Lq
        assert abs(M.maxsim_f32(q16, c16) - M.maxsim(q16, c16)) <= M.score_tol(Lq, w)


@pytest.mark.parametrize("w,Lq,N,seed", M.RANKING_CASES)
def test_ranking_corpora_have_wide_gaps(w, Lq, N, seed):
    q, docs, order = M.ranking_corpus(w, Lq, N, seed)
    q16 = M.f16_view(q)
    scores = np.array([M.maxsim(q16, M.f16_view(d)) for d in docs])
    assert np.array_equal(np.argsort(-scores, kind="stable"), order)
    # a stored element may differ from the emulation's by one f16 step: the gap must also
    # cover what that moves a score by, Lq (2^-10 + 2^-10) at most for unit rows
    assert M.min_gap(scores) > 4 * M.score_tol(Lq, w) + Lq * 2.0 ** -8, M.min_gap(scores)


def test_library_exports_the_mvindex_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_SO], capture_output=True, text=True, check=True).stdout
    have = set(re.findall(r"\bT (bertx_\w+)", out))
    missing = [s for s in ["bertx_mvindex_" + n for n in SYMBOLS] + ["bertx_bench_maxsim"] if s not in have]
    assert not missing, missing
    lib = bertpy.load_lib()
    for n in SYMBOLS:
        assert getattr(lib, "bertx_mvindex_" + n).argtypes is not None


def test_create_on_a_tokenizer_only_context_returns_null(capfd):
    old = os.environ.get("BERT_HOST_ONLY")
    os.environ["BERT_HOST_ONLY"] = "1"
    try:
        m = bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))
        assert not m.lib.bertx_mvindex_create(m.ctx, 0, 64, 8, 256)
        with pytest.raises(RuntimeError):
            bertpy.BertTokenIndex(m, 8, 256)
        for fn in (m.lib.bertx_mvindex_docs, m.lib.bertx_mvindex_clear, m.lib.bertx_mvindex_dim):
            assert fn(None) == -1
        m.lib.bertx_mvindex_free(None)
    finally:
        if old is None:
            os.environ.pop("BERT_HOST_ONLY", None)
        else:
            os.environ["BERT_HOST_ONLY"] = old
