"""GPU tests of [CLS] pooling, the pruned last layer and the per-token output."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bertpy
import ref_forward

pytestmark = pytest.mark.gpu

COS_TOL = 1e-3       # north star: float vectors within 1e-3 cosine of the reference path
PRUNE_TOL = 1e-4     # the pruned last layer may use a tenth of that budget
FORMATS = ["f32", "f16", "q4_0", "q4_1", "q8_0"]
QUANT = ["q4_0", "q4_1", "q8_0"]


@pytest.fixture(autouse=True, scope="module")
def _one_device():
    old = os.environ.get("BERT_DEVICES")
    os.environ["BERT_DEVICES"] = "0"
    os.environ.pop("BERT_POOL", None)
    yield
    if old is None:
        os.environ.pop("BERT_DEVICES", None)
    else:
        os.environ["BERT_DEVICES"] = old


def ragged_ids(n_vocab, lens, seed=3):
    rng = np.random.default_rng(seed)
    return [np.concatenate([[101], rng.integers(104, n_vocab, L - 2), [102]]).astype(np.int32) if L >= 2
            else np.array([101], np.int32) for L in lens]


def ref_lens(maxl):
    return [1, 2, 3, 17, 64, 65, 100, maxl - 1, maxl, 33]


def one_minus_cos(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return 1.0 - np.sum(a * b, axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


@pytest.fixture(scope="module")
def reference(quant_models):
    """(ids, float64 per-token hidden states) per (tiny, fmt), computed once and shared."""
    cache = {}

    def get(tiny, fmt):
        if (tiny, fmt) not in cache:
            r = ref_forward.RefModel(quant_models[(tiny, fmt)])
            ids = ragged_ids(r.hp["n_vocab"], ref_lens(r.hp["n_max_tokens"]))
            hid = r.hidden_batch(ids)
            for h in hid:
                h.setflags(write=False)
            cache[(tiny, fmt)] = (ids, hid)
        return cache[(tiny, fmt)]
    return get


def attention_ref(qkv, cu, n_head, d):
    """f64 softmax(Q K^T / sqrt(dh)) V per (sentence, head) on the f16 inputs (bert.cpp:1018-1036)."""
    dh = d // n_head
    q, k, v = (qkv[:, i * d:(i + 1) * d].astype(np.float64) for i in range(3))
    out = np.zeros((qkv.shape[0], d))
    for b in range(len(cu) - 1):
        s0, s1 = cu[b], cu[b + 1]
        for h in range(n_head):
            c = slice(h * dh, (h + 1) * dh)
            sc = q[s0:s1, c] @ k[s0:s1, c].T / np.sqrt(dh)
            p = np.exp(sc - sc.max(axis=1, keepdims=True))
            out[s0:s1, c] = (p / p.sum(axis=1, keepdims=True)) @ v[s0:s1, c]
    return out


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("dh", [64, 32])
def test_attention_cls_matches_numpy(lib, dh):
    """The single-query kernel on ragged sentences (1 .. 1000 tokens: chunk edges of
    256, lengths past the LDS form of the full kernel), one with sharp scores (Q x 4,
    keys growing along the sentence), against row cu[b] of the f64 attention."""
    n_head = 4
    d = n_head * dh
    lens = [1, 2, 5, 63, 64, 65, 200, 512, 130, 513, 1000]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T = int(cu[-1])
    rng = np.random.default_rng(dh + 3)
    qkv = rng.standard_normal((T, 3 * d)).astype(np.float32)
    s0, s1 = cu[8], cu[9]                 # sentence 8 (130 tokens): large Q, keys that grow along the sentence
    qkv[s0:s1, :d] *= 4.0
    qkv[s0:s1, d:2 * d] *= np.linspace(0.2, 3.0, s1 - s0)[:, None]
    qkv = qkv.astype(np.float16)
    out = np.zeros((len(lens), d), np.float16)
    rc = lib.bertx_test_attention_cls(qkv.ctypes.data, cu.ctypes.data, len(lens), n_head, d, out.ctypes.data)
    assert rc == 0, rc
    ref = attention_ref(qkv, cu, n_head, d)[cu[:-1]]
    got = out.astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max()
    print("attention_cls dh", dh, "max|err|", err, "max|ref|", np.abs(ref).max())
    assert err < 6e-3 * max(1.0, np.abs(ref).max()), err


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("tiny", ["tiny32", "tiny64"])
def test_cls_matches_reference(quant_models, reference, tiny, fmt):
    ids, hid = reference(tiny, fmt)
    m = bertpy.BertModel(quant_models[(tiny, fmt)])
    m.set_pooling("cls")
    got = m.forward_batch(ids)
    want = ref_forward.cls_pool(hid)
    omc = one_minus_cos(got, want)
    print(tiny, fmt, "CLS 1 - cos vs reference: max", omc.max())
    assert np.isfinite(got).all()
    assert np.all(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0) <= 1e-5)
    assert omc.max() <= COS_TOL, omc


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("tiny", ["tiny32", "tiny64"])
def test_tokens_match_reference(quant_models, reference, tiny, fmt):
    ids, hid = reference(tiny, fmt)
    m = bertpy.BertModel(quant_models[(tiny, fmt)])
    got = m.forward_tokens(ids)
    worst_cos, worst_norm = 0.0, 0.0
    for g, h in zip(got, hid):
        assert g.shape == h.shape and np.isfinite(g).all()
        worst_cos = max(worst_cos, one_minus_cos(g, h).max())
        gn, hn = np.linalg.norm(g.astype(np.float64), axis=1), np.linalg.norm(h, axis=1)
        worst_norm = max(worst_norm, np.abs(gn / hn - 1.0).max())
    print(tiny, fmt, "tokens: max 1 - cos", worst_cos, "max norm ratio error", worst_norm)
    assert worst_cos <= COS_TOL
    assert worst_norm <= 0.01


# 4 ---------------------------------------------------------------------------
CHAINS = [(fmt, None) for fmt in FORMATS] + [(fmt, "q8") for fmt in QUANT]


@pytest.mark.parametrize("fmt,act", CHAINS)
def test_cls_and_tokens_consistent_with_mean(quant_models, fmt, act):
    """Every chain, pruning off: CLS is the normalised first token row, and the
    normalised mean of the token rows is the mean-mode output (which the existing
    tests pin to the oracle)."""
    m = bertpy.BertModel(quant_models[("tiny64", fmt)], act=act)
    ids = ragged_ids(690, ref_lens(m.n_max_tokens))
    mean = m.forward_batch(ids)
    toks = m.forward_tokens(ids)
    m.set_cls_pruning(False)
    m.set_pooling("cls")
    cls = m.forward_batch(ids)
    row0 = np.stack([t[0] for t in toks]).astype(np.float64)
    row0 /= np.linalg.norm(row0, axis=1, keepdims=True)
    assert np.allclose(cls, row0, rtol=0, atol=1e-6), np.abs(cls - row0).max()
    pooled = np.stack([t.astype(np.float64).mean(axis=0) for t in toks])
    omc = one_minus_cos(pooled, mean)
    print(fmt, act, "mean of token rows vs mean mode: max 1 - cos", omc.max())
    assert omc.max() <= 1e-6, omc


# 5 ---------------------------------------------------------------------------
def _pruned_vs_unpruned(m, ids):
    m.set_pooling("cls")
    m.set_cls_pruning(True)
    pruned = m.forward_batch(ids)
    m.set_cls_pruning(False)
    full = m.forward_batch(ids)
    assert np.isfinite(pruned).all() and np.isfinite(full).all()
    return one_minus_cos(pruned, full)


@pytest.mark.parametrize("fmt", ["f16"] + QUANT)
def test_pruned_matches_unpruned_tiny(quant_models, fmt):
    m = bertpy.BertModel(quant_models[("tiny64", fmt)])
    rng = np.random.default_rng(11)
    batches = {"ragged": ragged_ids(690, ref_lens(m.n_max_tokens)),
               "single": ragged_ids(690, [37], seed=5),
               "65 short": ragged_ids(690, [int(x) for x in rng.integers(2, 10, 65)], seed=6)}
    for name, ids in batches.items():
        omc = _pruned_vs_unpruned(m, ids)
        print(fmt, name, "pruned vs unpruned: max 1 - cos", omc.max())
        assert omc.max() <= PRUNE_TOL, (name, omc)


def test_pruned_matches_unpruned_bge_base(tmp_path):
    hp = bertpy.ARCHS["bge-base-en-v1.5"]
    path = str(tmp_path / "bge-base-q4_0.bin")
    bertpy.synthetic_model(path, "bge-base-en-v1.5", "q4_0")
    m = bertpy.BertModel(path)
    ids = bertpy.synthetic_ids(4, [512, 300, 64, 7], hp["n_vocab"])
    omc = _pruned_vs_unpruned(m, ids)
    print("bge-base q4_0 pruned vs unpruned: max 1 - cos", omc.max())
    assert omc.max() <= PRUNE_TOL, omc


# 6 ---------------------------------------------------------------------------
def test_cls_pruned_invariances_bitwise(quant_models):
    """Under CLS with pruning a sentence has the same bits alone, in a ragged batch
    and in the reversed batch; eager, captured and replayed calls of one shape agree."""
    m = bertpy.BertModel(quant_models[("tiny64", "q4_0")])
    m.set_pooling("cls")
    ids = ragged_ids(690, [5, 300, 512, 40, 2, 129])
    full = m.forward_batch(ids)
    for i in (0, 2, 4, 5):
        alone = m.forward_batch([ids[i]])
        assert np.array_equal(alone[0], full[i]), i
    rev = m.forward_batch(ids[::-1])
    assert np.array_equal(rev[::-1], full)
    a, b, c = (m.forward_batch(ids) for _ in range(3))   # eager, captured, replayed
    assert np.array_equal(a, full) and np.array_equal(b, full) and np.array_equal(c, full)


# 7 ---------------------------------------------------------------------------
def test_mode_switching_keeps_bits(quant_models):
    path = quant_models[("tiny64", "q4_0")]
    ids = ragged_ids(690, [5, 300, 512, 40, 2, 129])
    m = bertpy.BertModel(path)
    outs = []
    for mode in ("mean", "cls", "mean", "cls"):
        m.set_pooling(mode)
        assert m.pooling == mode
        outs.append(m.forward_batch(ids))
    assert np.array_equal(outs[0], outs[2])
    assert np.array_equal(outs[1], outs[3])
    assert not np.array_equal(outs[0], outs[1])
    fresh = bertpy.BertModel(path)
    assert fresh.pooling == "mean"
    for _ in range(3):
        assert np.array_equal(fresh.forward_batch(ids), outs[0])


# 8 ---------------------------------------------------------------------------
def test_text_path_follows_the_mode(quant_models):
    m = bertpy.BertModel(quant_models[("tiny64", "f16")])
    texts = ["hello world", "the quick brown fox jumps over the lazy dog", "a"]
    ids = [np.asarray(m.tokenize(t)[0], np.int32) for t in texts]
    mean = m.encode(texts)
    m.set_pooling("cls")
    got = m.encode(texts)
    assert np.array_equal(got, m.forward_batch(ids))
    assert not np.array_equal(got, mean)
    assert np.array_equal(m.encode(texts[1]), m.forward(ids[1]))


def test_bert_pool_environment_on_device(quant_models):
    code = ("import sys\n"
            "sys.path.insert(0, sys.argv[1])\n"
            "import bertpy\n"
            "m = bertpy.BertModel(sys.argv[2])\n"
            "print('POOL', m.lib.bertx_pooling(m.ctx), m.lib.bertx_num_devices(m.ctx))\n")
    env = dict(os.environ, BERT_POOL="cls", BERT_DEVICES="0")
    r = subprocess.run([sys.executable, "-c", code, os.path.join(os.path.dirname(bertpy.__file__), ".."),
                        quant_models[("tiny64", "f16")]], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "POOL 1 1" in r.stdout, r.stdout
