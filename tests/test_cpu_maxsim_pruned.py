"""The host-checkable rules of the centroid codes and the pruned MaxSim search
(maxsim_pruned_refs.py): the planted store of the recall test vetted in float64, the
(score, id) order of the composition, the substitution rule on the CPU references of both
storage kinds, the training sample and update (against the library's host code), and the
argument checks a tokenizer-only context can reach."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bertpy
import maxsim_i8_refs as R8
import maxsim_pruned_refs as PR
import maxsim_refs as M
import maxsim_search_refs as SR
from conftest import GOLDEN, LIB_SO

SYMBOLS = ["set_centroids", "train_centroids", "centroids", "centroid", "doc_codes", "candidates", "candidates_device",
           "search_pruned", "search_pruned_device", "search_pruned_texts"]
HOOKS = ["bertx_bench_maxsim_pruned", "bertx_test_approx_ran", "bertx_test_kmeans_update", "bertx_test_kmeans_sample"]


# ---- the planted store in float64 ----
@pytest.mark.parametrize("storage", ("f16", "int8"))
def test_planted_store_has_wide_margins(storage):
    """The recall test cannot pass or fail by rounding: the target leads the runner-up by at
    least 64 times the header's bound Lq (2 w + Lq) 2^-24 in the approximate and in the exact
    score.  The codes must be the planted directions too: a stored row re-packed as a query
    moves a similarity by at most 2^-10 (one f16 step of a unit row's elements; int8
    re-quantizes to the same bytes), so a lead of 0.1 over the second centroid decides them."""
    bound = 64 * M.score_tol(PR.PLANT_LEN, PR.PLANT_W)
    for approx_lead, exact_lead, code_lead in PR.planted_margins(storage):
        assert approx_lead >= bound and exact_lead >= bound, (approx_lead, exact_lead, bound)
        assert approx_lead > 0.5 and exact_lead > 0.5
        assert code_lead > 0.1


# ---- the order of the composition ----
@pytest.mark.parametrize("n,k", [(1, 1), (5, 3), (10, 10), (32, 10), (128, 128)])
def test_compose_is_the_better_order_with_fill(n, k):
    rng = np.random.default_rng(100 * n + k)
    pool = np.array([-np.inf, -1.5, -0.0, 0.0, 0.25, 0.25, 3.0], np.float32)
    ids = rng.permutation(4 * n)[:n].astype(np.int32)
    ids[rng.random(n) < 0.2] = -1                                      # fill slots among the candidates
    exact = pool[rng.integers(0, len(pool), n)]
    exact[ids < 0] = -np.inf
    s, i = PR.compose(exact, ids, k)
    live = np.flatnonzero(ids >= 0)
    # the same through the full-scan reference: scores by id, the rest of the id space absent
    order = sorted(live, key=lambda j: (-float(exact[j]), int(ids[j])))[:k]
    m = len(order)
    assert i[:m].tolist() == [int(ids[j]) for j in order]
    assert np.array_equal(s[:m].view(np.uint32), exact[order].view(np.uint32))
    assert np.all(i[m:] == -1) and np.all(np.isneginf(s[m:]))
    for a in range(m - 1):
        assert SR.better(s[a], int(i[a]), s[a + 1], int(i[a + 1]))


def test_nearest_prefers_the_lower_index():
    assert PR.nearest([0.0, 0.0, 0.0]) == 0
    assert PR.nearest([0.1, 0.5, 0.5, 0.2]) == 1
    assert PR.nearest(np.array([-0.0, 0.0], np.float32)) == 0
    assert PR.nearest([-1.0, -0.5]) == 1


# ---- the substitution rule on the CPU references ----
@pytest.mark.parametrize("storage", ("f16", "int8"))
def test_substitution_is_the_table_lookup(storage):
    """sum_i max_j T[i][code_j] with T = sim(query row, centroid) is the reference scorer's
    score of the substituted document, bit for bit: a centroid packs to the same values
    wherever it stands, and the max and the lane sum see the same numbers."""
    rng = np.random.default_rng(5)
    w, C, Lq = 64, 16, 17
    cent = M.token_rows(rng, C, w)
    q = M.token_rows(rng, Lq, w)
    codes = [rng.integers(0, C, n) for n in (1, 15, 16, 33)]
    docs = PR.substitute(cent, codes)
    if storage == "int8":
        qp, cp = R8.pack(q), R8.pack(cent)
        T = R8.S.ref_scores_i8(qp[0], qp[1], cp[0], cp[1])
        for c, d in zip(codes, docs):
            want = R8.score(qp, R8.pack(d))
            got = R8.lane_sum(T[:, c].max(axis=1))
            assert np.float32(want).tobytes() == np.float32(got).tobytes()
    else:
        q16, c16 = M.f16_view(q), M.f16_view(cent)
        T = np.array([[M.maxsim_f32(q16[i:i + 1], c16[c:c + 1]) for c in range(C)] for i in range(Lq)], np.float32)
        for c, d in zip(codes, docs):
            d16 = M.f16_view(d)
            assert np.array_equal(d16, c16[c])
            want = R8.lane_sum(np.array([M.maxsim_f32(q16[i:i + 1], d16) for i in range(Lq)], np.float32))
            got = R8.lane_sum(T[:, c].max(axis=1))
            assert np.float32(want).tobytes() == np.float32(got).tobytes()


# ---- training ----
def test_sample_rule_against_the_library(lib):
    for T, seed in [(1, 0), (100, 7), (1 << 18, 3), ((1 << 18) + 1, 0), ((1 << 18) + 1, 1), (1000003, 12345), (3 << 18, 2)]:
        out = np.zeros(3, np.int64)
        assert lib.bertx_test_kmeans_sample(T, seed, out.ctypes.data) == 0
        stride, start, n = PR.sample_rule(T, seed)
        assert out.tolist() == [stride, start, n]
        assert n == len(range(start, T, stride)) and n <= (1 << 18)


def test_update_rule_on_a_hand_made_example(lib):
    sample = np.array([[1, 0], [3, 0], [0, 2], [0, 4], [5, 5], [0.1, 0.2]], np.float32)
    codes = np.array([0, 0, 2, 2, 0, 2], np.uint16)
    cent = np.array([[9, 9], [7, 8], [9, 9], [-1, -2]], np.float32)
    want = np.array([[3, 5 / 3], [7, 8], [np.float64(np.float32(0.1)) / 3, (2 + 4 + np.float64(np.float32(0.2))) / 3], [-1, -2]])
    got, empty = PR.kmeans_update(sample, codes, cent)
    assert empty == 2
    assert np.array_equal(got, want.astype(np.float32))                # centroids 1 and 3 keep their rows
    mine = cent.copy()
    assert lib.bertx_test_kmeans_update(sample.ctypes.data, codes.ctypes.data, len(sample), 2, 4, mine.ctypes.data) == 2
    assert np.array_equal(mine.view(np.uint32), got.view(np.uint32))


def test_update_rule_is_order_sensitive_and_matches_the_library(lib):
    """Values whose float64 sum depends on the order: the library adds in ascending sample
    order, as the restatement does."""
    rng = np.random.default_rng(9)
    n, w, C = 400, 8, 16
    sample = (rng.standard_normal((n, w)) * np.float32(10.0) ** rng.integers(-6, 7, (n, 1))).astype(np.float32)
    codes = rng.integers(0, C - 1, n).astype(np.uint16)                # centroid C - 1 stays empty
    cent = rng.standard_normal((C, w)).astype(np.float32)
    got, empty = PR.kmeans_update(sample, codes, cent)
    mine = cent.copy()
    assert lib.bertx_test_kmeans_update(sample.ctypes.data, codes.ctypes.data, n, w, C, mine.ctypes.data) == empty == 1
    assert np.array_equal(mine.view(np.uint32), got.view(np.uint32))
    assert np.array_equal(mine[C - 1], cent[C - 1])


def test_initial_rows_spread_over_the_sample():
    assert PR.initial_rows(16, 16) == list(range(16))
    rows = PR.initial_rows(1000, 48)
    assert rows[0] == 0 and rows[-1] == 47 * 1000 // 48 and len(set(rows)) == 48


# ---- the library's surface without a GPU ----
def test_library_exports_the_pruned_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_SO], capture_output=True, text=True, check=True).stdout
    have = set(re.findall(r"\bT (bertx_\w+)", out))
    missing = [s for s in ["bertx_mvindex_" + n for n in SYMBOLS] + HOOKS if s not in have]
    assert not missing, missing
    lib = bertpy.load_lib()
    for n in SYMBOLS:
        assert getattr(lib, "bertx_mvindex_" + n).argtypes is not None
    for n in ("set_centroids", "train_centroids", "n_centroids", "centroid", "doc_codes", "candidates", "search_pruned"):
        assert hasattr(bertpy.BertTokenIndex, n)


def test_argument_checks_without_a_store():
    """What a tokenizer-only context can reach: every entry refuses a NULL store with -1 and
    leaves its outputs alone; the bench refuses bad arguments before it looks for a device."""
    old = os.environ.get("BERT_HOST_ONLY")
    os.environ["BERT_HOST_ONLY"] = "1"
    try:
        m = bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))
        L = m.lib
        q = np.ones((2, 3, 64), np.float32)
        s = np.full((2, 4), 7.0, np.float32)
        i = np.full((2, 4), 7, np.int32)
        c16 = np.full(8, 7, np.uint16)
        assert L.bertx_mvindex_set_centroids(None, q.ctypes.data, 16) == -1
        assert L.bertx_mvindex_train_centroids(None, 16, 1, 0) == -1
        assert L.bertx_mvindex_centroids(None) == -1
        assert L.bertx_mvindex_centroid(None, 0, s.ctypes.data) == -1
        assert L.bertx_mvindex_doc_codes(None, 0, c16.ctypes.data) == -1
        assert L.bertx_mvindex_candidates(None, q.ctypes.data, 2, 3, 4, s.ctypes.data, i.ctypes.data) == -1
        assert L.bertx_mvindex_candidates_device(None, None, 2, 3, 4, None, None, None) == -1
        assert L.bertx_mvindex_search_pruned(None, q.ctypes.data, 2, 3, 4, 4, s.ctypes.data, i.ctypes.data) == -1
        assert L.bertx_mvindex_search_pruned_device(None, None, 2, 3, 4, 4, None, None, None) == -1
        texts = (ctypes.c_char_p * 2)(b"a", b"b")
        assert L.bertx_mvindex_search_pruned_texts(None, m.ctx, 1, 2, texts, 4, 4, 0, s.ctypes.data, i.ctypes.data) == -1
        assert np.all(s == 7.0) and np.all(i == 7) and np.all(c16 == 7)
        us = np.full(3, 7.0, np.float32)
        for args in [(64, 100, 16, 24, 16, 1, 10, 32, 0, 2), (64, 100, 16, 16, 16, 0, 10, 32, 0, 2),
                     (64, 100, 16, 16, 16, 1, 33, 32, 0, 2), (64, 100, 16, 16, 16, 1, 10, 129, 0, 2)]:
            assert L.bertx_bench_maxsim_pruned(*args, bertpy._as_f32p(us)) == -1
        assert np.all(us == 7.0)
        assert L.bertx_test_approx_ran(0) in (0, 1, 2, 3)
    finally:
        if old is None:
            os.environ.pop("BERT_HOST_ONLY", None)
        else:
            os.environ["BERT_HOST_ONLY"] = old
