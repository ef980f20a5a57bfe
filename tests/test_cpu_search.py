"""CPU side of the embedding index (bertx_index_*): the ABI is declared and exported,
a tokenizer-only context refuses an index, the result checker of the GPU tests
rejects what it must, and the planted corpora keep their margins."""
import os
import re

import numpy as np
import pytest

import search_refs as R
from conftest import GOLDEN, ROOT

INDEX_ABI = ["bertx_index_create", "bertx_index_free", "bertx_index_clear", "bertx_index_size",
             "bertx_index_capacity", "bertx_index_dim", "bertx_index_add", "bertx_index_add_device",
             "bertx_index_rows", "bertx_index_search", "bertx_index_search_device", "bertx_index_add_texts",
             "bertx_index_search_texts", "bertx_bench_search"]


def test_index_abi_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    for name in INDEX_ABI:
        assert re.search(r"BERT_API[^;]*\b%s\(" % name, hdr), name
        assert hasattr(lib, name), name


def test_python_class_exists():
    import bertpy
    for attr in ("add", "add_texts", "search", "search_texts", "rows", "clear", "__len__"):
        assert hasattr(bertpy.BertIndex, attr), attr


def test_host_only_context_refuses_an_index(lib, monkeypatch):
    import bertpy
    monkeypatch.setenv("BERT_HOST_ONLY", "1")
    m = bertpy.BertModel(os.path.join(GOLDEN, "tiny32", "ggml-model-f32.bin"), lib=lib)
    assert not lib.bertx_index_create(m.ctx, 0, 16)
    with pytest.raises(RuntimeError):
        bertpy.BertIndex(m, 16)
    # NULL handles are refused, not dereferenced
    assert lib.bertx_index_size(None) < 0 and lib.bertx_index_clear(None) < 0
    assert lib.bertx_index_add(None, None, 1) < 0
    lib.bertx_index_free(None)


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(5)
    rows = R.unit_rows(rng, 200, 64).astype(np.float16).astype(np.float32)
    queries = R.unit_rows(rng, 4, 64)
    # an exact tie: rows 7 and 90 equal
    rows[90] = rows[7]
    queries[0] = rows[7]
    return rows, queries, R.ref_scores(queries, rows), R.tolerances(queries, rows)


def _check_all(ref, scores, ids, k, tol):
    for b in range(len(ref)):
        R.check_topk(ref[b], scores[b], ids[b], k, tol[b])


def test_checker_accepts_numpy_device(small):
    rows, queries, ref, tol = small
    for k in (1, 10, 128):
        scores, ids = R.numpy_device(queries, rows, k)
        _check_all(ref, scores, ids, k, tol)
    assert list(R.numpy_device(queries, rows, 2)[1][0]) == [7, 90]
    # fewer rows than k: the (-1, -inf) fill
    scores, ids = R.numpy_device(queries, rows[:7], 10)
    _check_all(R.ref_scores(queries, rows[:7]), scores, ids, 10, tol)
    assert np.all(ids[:, 7:] == -1)


def test_checker_rejections(small):
    rows, queries, ref, tol = small
    k = 10
    good_s, good_i = R.numpy_device(queries, rows, k)

    def rejected(mut, b=1, r=ref, kk=k, base=(good_s, good_i)):
        s, i = base[0][b].copy(), base[1][b].copy()
        mut(s, i)
        with pytest.raises(AssertionError):
            R.check_topk(r[b], s, i, kk, tol[b])

    worst = int(np.argmin(ref[1]))

    def wrong_id(s, i):
        i[4] = worst
    rejected(wrong_id)

    def duplicate(s, i):
        i[5], s[5] = i[4], s[4]
    rejected(duplicate)

    def unsorted(s, i):
        s[[2, 3]], i[[2, 3]] = s[[3, 2]], i[[3, 2]]
    rejected(unsorted)

    def tie_descending(s, i):
        assert s[0] == s[1] and list(i[:2]) == [7, 90]
        i[[0, 1]] = i[[1, 0]]
    rejected(tie_descending, b=0)

    def off_by_3tol(s, i):
        s[:] = s + np.float32(3 * tol[1])
    rejected(off_by_3tol)

    def dropped_best(s, i):   # the best row missing: everything shifted up by one
        full_s, full_i = R.numpy_device(queries, rows, k + 1)
        s[:], i[:] = full_s[1][1:], full_i[1][1:]
    rejected(dropped_best)

    short = rows[:7]
    fs, fi = R.numpy_device(queries, short, k)

    def missing_fill(s, i):
        i[8], s[8] = 0, 0.0
    rejected(missing_fill, r=R.ref_scores(queries, short), base=(fs, fi))


@pytest.mark.parametrize("d,N,B,k", R.PLANTED_SHAPES)
def test_planted_margins(d, N, B, k):
    rows, queries, ids = R.planted(d, N, B, k)
    assert set(R.edge_ids(N)) <= set(ids.ravel().tolist())
    stored = rows.astype(np.float16).astype(np.float32)
    ref = R.ref_scores(queries, stored)
    tol = R.tolerances(queries, stored)
    assert tol.max() <= 2.5e-4
    order = np.argsort(-ref, axis=1, kind="stable")
    assert np.array_equal(order[:, :k], ids)
    top = np.take_along_axis(ref, order[:, :k + 1], axis=1)
    gaps = top[:, :-1] - top[:, 1:]
    print("minimum gap", gaps.min())
    assert gaps.min() >= 0.005
