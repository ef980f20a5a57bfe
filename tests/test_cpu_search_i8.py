"""CPU side of the int8 embedding index (bertx_index_create_ex, BERTX_INDEX_I8): the new
ABI is declared and exported, refusals that need no device, and the properties of the
numpy restatement (search_i8_refs.py) that the GPU tests rest on."""
import os
import re

import numpy as np
import pytest

import search_i8_refs as Q
import search_refs as R
from conftest import GOLDEN, ROOT

NEW_ABI = ["bertx_index_create_ex", "bertx_index_storage", "bertx_index_rows_i8", "bertx_bench_search_ex",
           "bertx_bench_search_add_rate_ex"]


def test_new_abi_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    for name in NEW_ABI:
        assert re.search(r"BERT_API[^;]*\b%s\(" % name, hdr), name
        assert hasattr(lib, name), name
    assert re.search(r"enum\s*\{\s*BERTX_INDEX_F16\s*=\s*0\s*,\s*BERTX_INDEX_I8\s*=\s*1\s*\}", hdr)
    # the old entries keep their declarations
    assert re.search(r"bertx_index_create\(struct bert_ctx \*ctx, int32_t slot, int32_t capacity_rows\);", hdr)
    assert re.search(r"bertx_bench_search\(int32_t d, int32_t N, int32_t B, int32_t k, int32_t iters, float \*avg_us\);",
                     hdr)


def test_python_class_accepts_storage():
    import inspect

    import bertpy
    sig = inspect.signature(bertpy.BertIndex.__init__)
    assert sig.parameters["storage"].default == "f16"
    assert list(sig.parameters)[:4] == ["self", "model", "capacity", "slot"]
    assert hasattr(bertpy.BertIndex, "rows_i8")
    assert bertpy.BertIndex.STORAGE == {"f16": 0, "int8": 1}


def test_host_only_context_and_unknown_storage_are_refused(lib, monkeypatch, capfd):
    import bertpy
    monkeypatch.setenv("BERT_HOST_ONLY", "1")
    m = bertpy.BertModel(os.path.join(GOLDEN, "tiny32", "ggml-model-f32.bin"), lib=lib)
    capfd.readouterr()
    for storage in (0, 1):
        assert not lib.bertx_index_create_ex(m.ctx, 0, 16, storage)
        assert "tokenizer-only" in capfd.readouterr().err
    for storage in (2, -1, 7):
        assert not lib.bertx_index_create_ex(m.ctx, 0, 16, storage)
        assert "storage %d" % storage in capfd.readouterr().err
    assert not lib.bertx_index_create_ex(None, 0, 16, 1)
    with pytest.raises(RuntimeError):
        bertpy.BertIndex(m, 16, storage="int8")
    with pytest.raises(ValueError):
        bertpy.BertIndex(m, 16, storage="int4")
    # NULL handles are refused, not dereferenced
    assert lib.bertx_index_storage(None) == -1
    q, s = np.full(64, 5, np.int8), np.full(1, 5.0, np.float32)
    assert lib.bertx_index_rows_i8(None, 0, 1, q.ctypes.data, s.ctypes.data) < 0
    assert np.all(q == 5) and s[0] == 5.0


# ---- the reference's own properties ----
@pytest.mark.parametrize("d", [64, 192, 768])
def test_quantizer_range_and_dequantization_error(d):
    rng = np.random.default_rng(d)
    x = R.unit_rows(rng, 300, d)
    x[7] *= np.float32(1e3)
    x[8] *= np.float32(1e-3)
    q, s = Q.quantize(x)
    assert q.dtype == np.int8 and s.dtype == np.float32 and q.shape == x.shape and s.shape == (300,)
    assert np.abs(q.astype(np.int32)).max() <= 127
    # the element that carries amax maps to +-127
    assert np.all(np.abs(q.astype(np.int32)).max(axis=1) == 127)
    deq = q.astype(np.float64) * s.astype(np.float64)[:, None]
    err = np.abs(deq - x.astype(np.float64))
    print("worst dequantization error / (scale / 2)", (err / (s.astype(np.float64)[:, None] / 2)).max())
    assert np.all(err <= s.astype(np.float64)[:, None] / 2)


def test_zero_row_and_nearest_even():
    x = np.zeros((3, 64), np.float32)
    x[1, 5] = 2.0
    x[2, :4] = [127.0, 0.5, 1.5, -2.5]       # inv = 1 exactly: ties go to the even neighbour
    q, s = Q.quantize(x)
    assert s[0] == 0.0 and not q[0].any()
    assert q[1, 5] == 127 and np.count_nonzero(q[1]) == 1 and s[1] == np.float32(2.0) / np.float32(127.0)
    assert list(q[2, :4]) == [127, 0, 2, -2] and s[2] == 1.0
    ref = Q.ref_scores_i8(q, s, q, s)
    assert np.all(ref[0] == 0.0) and np.all(ref[:, 0] == 0.0)
    assert ref[1, 1] == np.float32(127 * 127) * (s[1] * s[1])
    sc, ids = Q.expected_topk(ref[:1], 5)
    assert list(ids[0]) == [0, 1, 2, -1, -1] and np.all(sc[0, :3] == 0.0) and np.all(np.isneginf(sc[0, 3:]))


@pytest.mark.parametrize("d", [64, 192, 768])
def test_error_bound_holds_on_unit_rows(d):
    rng = np.random.default_rng(100 + d)
    rows, queries = R.unit_rows(rng, 400, d), R.unit_rows(rng, 8, d)
    rq, rs = Q.quantize(rows)
    qq, qs = Q.quantize(queries)
    ref = Q.ref_scores_i8(qq, qs, rq, rs).astype(np.float64)
    exact = queries.astype(np.float64) @ rows.astype(np.float64).T
    bound = np.array([[Q.error_bound(queries[b], rows[i], qs[b], rs[i]) for i in range(400)] for b in range(8)])
    err = np.abs(exact - ref)
    slack = 3 * 2.0 ** -24 * np.abs(ref)     # the two roundings of the final multiplies
    print("d", d, "rms error", np.sqrt((err ** 2).mean()), "worst error / bound", (err / bound).max())
    assert np.all(err <= bound + slack)


@pytest.mark.parametrize("d,N,B,k", R.PLANTED_SHAPES)
def test_planted_ids_survive_quantization(d, N, B, k):
    rows, queries, ids = R.planted(d, N, B, k)
    rq, rs = Q.quantize(rows)
    qq, qs = Q.quantize(queries)
    ref = Q.ref_scores_i8(qq, qs, rq, rs)
    sc, got = Q.expected_topk(ref, k + 1)
    assert np.array_equal(got[:, :k], ids)
    gaps = sc[:, :-1].astype(np.float64) - sc[:, 1:].astype(np.float64)
    print("minimum gap", gaps.min())
    assert gaps.min() >= 0.005
