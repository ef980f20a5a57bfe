"""CPU tests of the pooling feature: the float64 reference forward (ref_forward.py)
pinned to the oracle, and the pooling setters on a tokenizer-only context."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import ref_forward
from conftest import GOLDEN

F32_COS_TOL = 1e-6   # the project's bound between two float forwards of the same weights


def ragged_ids(n_vocab, lens, seed=3):
    rng = np.random.default_rng(seed)
    return [np.concatenate([[101], rng.integers(104, n_vocab, L - 2), [102]]).astype(np.int32) if L >= 2
            else np.array([101], np.int32) for L in lens]


@pytest.mark.parametrize("fmt", ["f32", "f16", "q4_0", "q4_1", "q8_0"])
@pytest.mark.parametrize("tiny", ["tiny32", "tiny64"])
def test_ref_forward_mean_matches_oracle(quant_models, tiny, fmt):
    """ref_forward's mean-pooled output against the oracle: f32 / f16 files as the
    oracle runs them, quantized files with the oracle's f32 activations (the same
    weights, float arithmetic).  The committed goldens show an independent float
    forward and the oracle 1.2e-7 apart on both tiny models."""
    path = quant_models[(tiny, fmt)]
    o = oracle_lib.Oracle(path)
    maxl = o.n_max_tokens
    ids = ragged_ids(o.n_vocab, [2, 3, 17, 64, 100, maxl - 1, maxl, 33])
    want = o.forward_batch(ids) if fmt in ("f32", "f16") else o.forward_batch(ids, activations="f32")
    got = ref_forward.mean_pool(ref_forward.RefModel(path).hidden_batch(ids))
    one_minus_cos = 1.0 - np.sum(got * want.astype(np.float64), axis=1)
    print(tiny, fmt, "1 - cos vs oracle:", one_minus_cos.max())
    assert np.all(np.abs(np.linalg.norm(got, axis=1) - 1.0) < 1e-12)
    assert one_minus_cos.max() <= F32_COS_TOL, one_minus_cos


@pytest.fixture
def host_model(lib, monkeypatch):
    import bertpy
    monkeypatch.setenv("BERT_HOST_ONLY", "1")
    monkeypatch.delenv("BERT_POOL", raising=False)
    m = bertpy.BertModel(os.path.join(GOLDEN, "tiny32", "ggml-model-f32.bin"), lib=lib)
    yield m
    del m


def test_pooling_setter_getter_host_only(host_model):
    m = host_model
    L = m.lib
    assert L.bertx_pooling(m.ctx) == 0 and m.pooling == "mean"
    assert L.bertx_set_pooling(m.ctx, 1) == 0
    assert L.bertx_pooling(m.ctx) == 1 and m.pooling == "cls"
    assert L.bertx_set_pooling(m.ctx, 7) == -1
    assert L.bertx_set_pooling(m.ctx, -1) == -1
    assert L.bertx_pooling(m.ctx) == 1          # a refused mode changes nothing
    m.set_pooling("mean")
    assert L.bertx_pooling(m.ctx) == 0
    with pytest.raises(ValueError):
        m.set_pooling("max")
    assert L.bertx_set_cls_pruning(m.ctx, 0) == 0
    assert L.bertx_set_cls_pruning(m.ctx, 1) == 0


def test_host_only_forwards_still_refuse(host_model):
    """A tokenizer-only context accepts the mode; its forwards print their error and write nothing."""
    m = host_model
    m.set_pooling("cls")
    ids = [np.array([101, 200, 102], np.int32)]
    out = m.forward_batch(ids, fill=7.0)
    assert np.all(out == 7.0)
    with pytest.raises(RuntimeError):
        m.forward_tokens(ids)


_ENV_CODE = """
import os, sys
sys.path.insert(0, sys.argv[1])
import bertpy
L = bertpy.load_lib()
ctx = L.bert_load_from_file(sys.argv[2].encode())
print("CTX", "null" if not ctx else L.bertx_pooling(ctx))
"""


@pytest.mark.parametrize("value,want", [("bogus", "null"), ("cls", "1"), ("mean", "0"), (None, "0")])
def test_bert_pool_environment(lib, value, want):
    """BERT_POOL is read at load: mean / cls / unset, anything else a NULL load."""
    import bertpy
    env = dict(os.environ, BERT_HOST_ONLY="1")
    env.pop("BERT_POOL", None)
    if value is not None:
        env["BERT_POOL"] = value
    r = subprocess.run([sys.executable, "-c", _ENV_CODE, os.path.join(os.path.dirname(bertpy.__file__), ".."),
                        os.path.join(GOLDEN, "tiny32", "ggml-model-f32.bin")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("CTX " + want) in r.stdout, r.stdout + r.stderr[-500:]
