"""CPU side of the binary embedding index (BERTX_INDEX_BIN), the scorer of listed rows and
the two-stage search: the new ABI is declared and exported, refusals that need no device,
the properties of the numpy restatement (search_bin_refs.py) that the GPU tests rest on,
and the premise of the planted two-stage test."""
import ctypes
import os
import re

import numpy as np
import pytest

import search_bin_refs as BR
import search_refs as R
from conftest import GOLDEN, ROOT

NEW_ABI = ["bertx_index_rows_bits", "bertx_index_score_ids", "bertx_index_score_ids_device",
           "bertx_index_search_rescored", "bertx_index_search_rescored_device", "bertx_index_search_rescored_texts",
           "bertx_bench_search_rescored"]


def test_new_abi_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    for name in NEW_ABI:
        assert re.search(r"BERT_API[^;]*\b%s\(" % name, hdr), name
        assert hasattr(lib, name), name
    assert re.search(r"enum\s*\{\s*BERTX_INDEX_BIN\s*=\s*8\s*\}", hdr)
    # the first enum keeps its text, the new kind has one of its own
    assert re.search(r"enum\s*\{\s*BERTX_INDEX_F16\s*=\s*0\s*,\s*BERTX_INDEX_I8\s*=\s*1\s*\}", hdr)
    for phrase in ("bit_i = 1 iff x_i > 0", "d - 2 * popcount(bits_query xor bits_row)", "no cosine", "np.packbits"):
        assert phrase in hdr, phrase


def test_python_classes():
    import bertpy
    assert issubclass(bertpy.BertBinaryIndex, bertpy.BertIndex)
    assert bertpy.BertBinaryIndex.STORAGE == {"binary": 8}
    assert bertpy.BertIndex.STORAGE == {"f16": 0, "int8": 1}
    for name in ("score_ids", "search_rescored", "search_rescored_texts"):
        assert hasattr(bertpy.BertIndex, name), name
    assert hasattr(bertpy.BertBinaryIndex, "rows_bits") and not hasattr(bertpy.BertIndex, "rows_bits")
    assert bertpy.BertIndex._n_cand(10, None) == 40 and bertpy.BertIndex._n_cand(100, None) == 128
    assert bertpy.BertIndex._n_cand(10, 17) == 17


def test_refusals_without_a_device(lib, monkeypatch, capfd):
    import bertpy
    monkeypatch.setenv("BERT_HOST_ONLY", "1")
    m = bertpy.BertModel(os.path.join(GOLDEN, "tiny32", "ggml-model-f32.bin"), lib=lib)
    capfd.readouterr()
    assert not lib.bertx_index_create_ex(m.ctx, 0, 16, 8)
    assert "tokenizer-only" in capfd.readouterr().err
    for storage in (2, 3, 6, 7, 9, -1):
        assert not lib.bertx_index_create_ex(m.ctx, 0, 16, storage)
        assert "storage %d" % storage in capfd.readouterr().err
    # the token store does not take the kind
    assert not lib.bertx_mvindex_create_ex(m.ctx, 0, 64, 4, 64, 8)
    with pytest.raises(ValueError):
        bertpy.BertIndex(m, 16, storage="binary")
    with pytest.raises(ValueError):
        bertpy.BertBinaryIndex(m, 16, storage="f16")
    with pytest.raises(RuntimeError):
        bertpy.BertBinaryIndex(m, 16)
    # NULL handles are refused, not dereferenced, and the outputs stay as they were
    bits = np.full(8, 5, np.uint8)
    assert lib.bertx_index_rows_bits(None, 0, 1, bits.ctypes.data) < 0 and np.all(bits == 5)
    q = np.zeros((1, 64), np.float32)
    ids = np.zeros((1, 4), np.int32)
    sc = np.full((1, 4), 7.0, np.float32)
    out_i = np.full((1, 4), 7, np.int32)
    assert lib.bertx_index_score_ids(None, q.ctypes.data, 1, ids.ctypes.data, 4, sc.ctypes.data) < 0
    assert lib.bertx_index_score_ids_device(None, None, 1, None, 4, None, None) < 0
    assert lib.bertx_index_search_rescored(None, None, q.ctypes.data, 1, 2, 4, sc.ctypes.data, out_i.ctypes.data) < 0
    assert lib.bertx_index_search_rescored_device(None, None, None, 1, 2, 4, None, None, None) < 0
    texts = (ctypes.c_char_p * 1)(b"a")
    assert lib.bertx_index_search_rescored_texts(None, None, m.ctx, 1, 1, texts, 2, 4, sc.ctypes.data,
                                                 out_i.ctypes.data) < 0
    assert np.all(sc == 7.0) and np.all(out_i == 7)


# ---- the reference's own properties ----
def test_binarize_is_packbits_of_positive():
    rng = np.random.default_rng(1)
    for d in (64, 192, 768, 1024):
        x = BR.special_rows(rng, 7, d)
        with np.errstate(invalid="ignore"):
            want = np.packbits(x > 0, axis=1)
        assert np.array_equal(BR.binarize(x), want)
    edge = np.zeros((1, 64), np.float32)
    edge[0, :10] = [0.0, -0.0, np.nan, -np.nan, 1e-45, -1e-45, -1e-30, 1e-30, np.inf, -np.inf]
    got = np.unpackbits(BR.binarize(edge), axis=1)[0, :10]
    assert list(got) == [0, 0, 0, 0, 1, 0, 0, 1, 1, 0]
    assert np.float32(1e-45) > 0 and np.float32(1e-45) < np.finfo(np.float32).tiny    # a subnormal
    assert not BR.binarize(-np.abs(rng.standard_normal((3, 64)).astype(np.float32)) - 1).any()


@pytest.mark.parametrize("d", [64, 192, 768])
def test_score_is_the_dot_of_the_signs(d):
    rng = np.random.default_rng(d)
    rows, queries = BR.special_rows(rng, 50, d), BR.special_rows(rng, 6, d)
    rb, qb = BR.binarize(rows), BR.binarize(queries)
    ref = BR.ref_scores_bin(qb, rb, d)
    assert ref.dtype == np.float32 and ref.shape == (6, 50)
    assert np.array_equal(ref.astype(np.int64), BR.signs(qb, d) @ BR.signs(rb, d).T)
    assert np.abs(ref).max() <= d and np.all((ref.astype(np.int64) - d) % 2 == 0)
    assert np.all(np.diag(BR.ref_scores_bin(rb, rb, d)) == d)


def test_expected_topk_obeys_the_tie_rule():
    rng = np.random.default_rng(3)
    ref = rng.integers(0, 3, (4, 500)).astype(np.float32) * 2 - 2     # three distinct scores over 500 rows
    sc, ids = BR.expected_topk(ref, 128)
    for b in range(4):
        R.check_topk(ref[b], sc[b], ids[b], 128, 0.0)
        best = np.flatnonzero(ref[b] == 2)
        assert np.array_equal(ids[b, :min(128, len(best))], best[:128])
        assert BR.ranks(ref[b], ids[b]) == list(range(128))
    sc, ids = BR.expected_topk(ref[:, :5], 8)
    assert np.all(ids[:, 5:] == -1) and np.all(np.isneginf(sc[:, 5:]))


def test_select_orders_and_fills():
    s = np.array([[1.0, 3.0, 3.0, -np.inf, 2.0, 9.0]], np.float32)
    i = np.array([[7, 5, 2, -1, 4, 12]], np.int32)
    out_s, out_i = BR.select(s, i, 10, 5)                      # id 12 is not in a fine index of 10 rows
    assert list(out_i[0]) == [2, 5, 4, 7, -1]
    assert list(out_s[0, :4]) == [3.0, 3.0, 2.0, 1.0] and np.isneginf(out_s[0, 4])


# ---- the premise of the planted two-stage GPU test ----
@pytest.mark.parametrize("d,N,B,k", R.PLANTED_SHAPES)
def test_planted_ids_are_inside_the_binary_candidates(d, N, B, k):
    rows, queries, ids = R.planted(d, N, B, k)
    ref = BR.ref_scores_bin(BR.binarize(queries), BR.binarize(rows), d)
    worst = max(max(BR.ranks(ref[b], ids[b])) for b in range(B))
    print("worst binary rank of a planted id", worst, "k", k)
    assert worst < 4 * k
