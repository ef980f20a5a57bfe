"""CPU tests of cross-encoder reranking: pair tokenisation, the optional head of the model
file (loader, quantizer), the converter's head form, and the float64 reference's own
conditions.  Tokenizer-only contexts (BERT_HOST_ONLY=1): no GPU."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import bertpy
import ref_forward
import rerank_refs as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True, scope="module")
def _host_only():
    old = os.environ.get("BERT_HOST_ONLY")
    os.environ["BERT_HOST_ONLY"] = "1"
    yield
    if old is None:
        os.environ.pop("BERT_HOST_ONLY", None)
    else:
        os.environ["BERT_HOST_ONLY"] = old


@pytest.fixture(scope="module")
def head_models(lib, tmp_path_factory):
    return RR.make_head_models(lib, GOLDEN, str(tmp_path_factory.mktemp("head")))


@pytest.fixture(scope="module")
def tok(lib):
    return bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))


# 1 --------------------------------------------------------------------------- pair tokenisation

def pieces(m, text):
    """bert_tokenize of the text alone (no token limit), without its [CLS] / [SEP]."""
    ids, n = m.tokenize(text, n_max_tokens=4096)
    assert n == len(ids) and ids[0] == 101 and ids[-1] == 102
    return ids[1:-1]


def restated_pair(m, a, b, truncate, n_max):
    """(ids, types, full count): layout and HF's longest_first as its own *iterative* loop --
    one token at a time from the longer side, from the pair (B) on equal lengths."""
    pa, pb = pieces(m, a), pieces(m, b)
    full = len(pa) + len(pb) + 3
    if full > n_max:
        if not truncate:
            return None, None, full
        for _ in range(full - n_max):
            if len(pa) > len(pb):
                pa = pa[:-1]
            else:
                pb = pb[:-1]
    ids = [101] + pa + [102] + pb + [102]
    types = [0] * (len(pa) + 2) + [1] * (len(pb) + 1)
    return ids, types, full


def words(m, n, seed):
    """A text of n words whose piece count is not n in general (multi-piece and unknown words)."""
    rng = np.random.default_rng(seed)
    vocab = [m.id_to_token(i).decode() for i in range(104, 692)]
    pool = [w for w in vocab if w.isalnum() and w.isascii()] + ["zzzqqq", "naïve", "x,y", "42"]
    return " ".join(pool[int(i)] for i in rng.integers(0, len(pool), n))


def text_of_pieces(m, n, seed):
    """A text of exactly n pieces."""
    t = words(m, n, seed).split(" ")
    while len(pieces(m, " ".join(t))) > n:
        t.pop()
    k = len(pieces(m, " ".join(t)))
    one = next(w for w in (m.id_to_token(i).decode() for i in range(104, 692))
               if w.isalnum() and w.isascii() and len(pieces(m, w)) == 1)
    t += [one] * (n - k)
    assert len(pieces(m, " ".join(t))) == n
    return " ".join(t)


PAIR_CASES = [
    # (pieces of A, pieces of B, n_max): the budget is m = n_max - 3
    (0, 0, 16),        # both empty: [CLS][SEP][SEP]
    (5, 0, 16),        # B empty: its [SEP] stays, type 1
    (40, 3, 20),       # A alone over the budget
    (30, 40, 20),      # both over, m odd (17)
    (30, 40, 21),      # both over, m even (18)
    (40, 30, 20),      # ... the other side longer
    (25, 25, 20),      # equal lengths, m odd: B gives first
    (9, 30, 21),       # 2 s == m
    (30, 9, 21),
    (10, 30, 22),      # 2 s == m + 1, A shorter
    (30, 10, 22),      # 2 s == m + 1, B shorter
    (10, 7, 20),       # exactly n_max
    (10, 8, 20),       # n_max + 1
]


@pytest.mark.parametrize("la,lb,n_max", PAIR_CASES)
def test_tokenize_pair_matches_restatement(tok, la, lb, n_max):
    a, b = text_of_pieces(tok, la, 3 * la + 1), text_of_pieces(tok, lb, 5 * lb + 2)
    for truncate in (True, False):
        want_ids, want_types, full = restated_pair(tok, a, b, truncate, n_max)
        if want_ids is None:
            # refused, the full count reported, the buffers untouched
            ids, types = np.full(n_max, -7, np.int32), np.full(n_max, -7, np.int32)
            n = ctypes.c_int32(0)
            rc = tok.lib.bertx_tokenize_pair(tok.ctx, a.encode(), b.encode(), 0, ids.ctypes.data, types.ctypes.data,
                                             ctypes.byref(n), n_max)
            assert rc < 0 and n.value == full == la + lb + 3
            assert np.all(ids == -7) and np.all(types == -7)
            with pytest.raises(ValueError):
                tok.tokenize_pair(a, b, truncate=False, n_max=n_max)
            continue
        ids, types = tok.tokenize_pair(a, b, truncate=truncate, n_max=n_max)
        assert ids.tolist() == want_ids and types.tolist() == want_types
        assert len(ids) == min(full, n_max)
        if full == n_max + 1 and truncate:
            assert len(ids) == n_max


def test_tokenize_pair_layout_and_text_forms(tok):
    ids, types = tok.tokenize_pair("", "")
    assert ids.tolist() == [101, 102, 102] and types.tolist() == [0, 0, 1]
    ids, types = tok.tokenize_pair("Hello, World", "")
    assert ids.tolist() == [101] + pieces(tok, "Hello, World") + [102, 102]
    assert types.tolist() == [0] * (len(ids) - 1) + [1]
    # the same normalisation as bert_tokenize: case, accents, punctuation, unknown words
    a, b = "Café NAÏVE (x,y)", "zzzqqq  42\tfoo"
    ids, types = tok.tokenize_pair(a, b)
    assert ids.tolist() == [101] + pieces(tok, a) + [102] + pieces(tok, b) + [102]
    assert tok.lib.bertx_tokenize_pair(tok.ctx, b"a", b"b", 1, ids.ctypes.data, types.ctypes.data,
                                       ctypes.byref(ctypes.c_int32()), 2) == -1


# 2 --------------------------------------------------------------------------- model file

def test_head_file_loads_and_reports_labels(head_models):
    assert bertpy.BertModel(head_models[("tiny32", "f16")]).n_labels == 1
    assert bertpy.BertModel(head_models[("tiny64", "f32")]).n_labels == 3
    assert bertpy.BertModel(head_models[("tiny64", "q4_1")]).n_labels == 3
    # classifier.weight is 2-D also for one label
    recs = {r[0]: r for r in RR.records(head_models[("tiny32", "f16")])[1]}
    assert recs["classifier.weight"][1] == 2 and recs["classifier.weight"][3] == (64, 1)
    assert recs["classifier.weight"][2] == 0 and recs["pooler.dense.weight"][2] == 1


@pytest.mark.parametrize("name", RR.HEAD)
def test_partial_head_is_refused(head_models, tmp_path, name, capfd):
    p = RR.drop_record(head_models[("tiny64", "f16")], str(tmp_path / "partial.bin"), name)
    with pytest.raises(RuntimeError):
        bertpy.BertModel(p)
    assert "incomplete classification head" in capfd.readouterr().err


def test_bad_head_records_are_refused(head_models, tmp_path):
    src = head_models[("tiny64", "f16")]
    data = bytearray(open(src, "rb").read())
    recs = {r[0]: r for r in RR.records(src)[1]}
    # classifier.weight stored as f16: refused (f32 in every ftype)
    bad = bytearray(data)
    struct.pack_into("<i", bad, recs["classifier.weight"][6] + 8, 1)
    p = str(tmp_path / "cls_f16.bin")
    open(p, "wb").write(bytes(bad))
    with pytest.raises(RuntimeError):
        bertpy.BertModel(p)
    # 17 labels: refused
    p = str(tmp_path / "labels17.bin")
    bertpy.append_head(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"), p, RR.head_tensors(64, 17, 1))
    with pytest.raises(RuntimeError):
        bertpy.BertModel(p)


def test_headless_file_scores_minus_six(tok):
    assert tok.n_labels == 0
    L, n = tok.lib, 2
    ids, types = tok.tokenize_pair("a b", "c")
    lens = np.array([len(ids)] * n, np.int32)
    ip = np.array([ids.ctypes.data] * n, np.uintp)
    tp = np.array([types.ctypes.data] * n, np.uintp)
    out = np.full((n, 4), 7.0, np.float32)
    assert L.bertx_score_ids(tok.ctx, n, ip.ctypes.data, tp.ctypes.data, lens.ctypes.data, out.ctypes.data) == -6
    ta = (ctypes.c_char_p * n)(b"x", b"y")
    assert L.bertx_score_pairs(tok.ctx, 2, n, ta, ta, 1, out.ctypes.data) == -6
    assert L.bertx_rerank(tok.ctx, 2, b"q", n, ta, 1, out.ctypes.data) == -6
    assert np.all(out == 7.0)


@pytest.mark.parametrize("fmt", RR.QUANT)
def test_quantizer_keeps_the_classifier(head_models, fmt):
    src, dst = head_models[("tiny64", "f16")], head_models[("tiny64", fmt)]
    a, b = open(src, "rb").read(), open(dst, "rb").read()
    ra = {r[0]: r for r in RR.records(src)[1]}
    rb = {r[0]: r for r in RR.records(dst)[1]}
    assert [r[0] for r in RR.records(src)[1]] == [r[0] for r in RR.records(dst)[1]]
    ca, cb = ra["classifier.weight"], rb["classifier.weight"]
    assert cb[2] == 0 and a[ca[4]:ca[4] + ca[5]] == b[cb[4]:cb[4] + cb[5]]
    assert rb["pooler.dense.weight"][2] == bertpy.FTYPE[fmt]
    for n in ("pooler.dense.bias", "classifier.bias"):
        assert rb[n][2] == 0 and a[ra[n][4]:ra[n][4] + ra[n][5]] == b[rb[n][4]:rb[n][4] + rb[n][5]]


def test_headless_file_quantizes_as_before(lib, oracle, tmp_path):
    """A file without the head is written exactly as the oracle's quantizer writes it."""
    import oracle_lib
    src = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
    for it in (2, 3, 8):
        a, b = str(tmp_path / ("a%d.bin" % it)), str(tmp_path / ("b%d.bin" % it))
        assert lib.bertx_quantize_file(src.encode(), a.encode(), it) == 0
        assert oracle_lib.quantize_file(src, b, it) == 0
        assert open(a, "rb").read() == open(b, "rb").read()


# 3 --------------------------------------------------------------------------- converter

def _hf_dir(d, tensors, hp, vocab, shards, classifier=True, pooler=True):
    from safetensors.numpy import save_file
    os.makedirs(d, exist_ok=True)
    cfg = {"vocab_size": hp["n_vocab"], "max_position_embeddings": hp["n_max_tokens"], "hidden_size": hp["n_embd"],
           "intermediate_size": hp["n_intermediate"], "num_attention_heads": hp["n_head"],
           "num_hidden_layers": hp["n_layer"]}
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("".join(w + "\n" for w in vocab))
    t = {}
    for name, a in tensors.items():
        if name.startswith("classifier."):
            if classifier:
                t[name] = np.ascontiguousarray(a, np.float32)
        elif name.startswith("pooler."):
            if pooler:
                t["bert." + name] = np.ascontiguousarray(a, np.float32)
        else:
            t["bert." + name] = np.ascontiguousarray(a, np.float32)
    names = sorted(t)
    if shards == 1:
        save_file(t, os.path.join(d, "model.safetensors"))
        return d
    wm = {}
    for s in range(shards):
        fn = "model-%05d-of-%05d.safetensors" % (s + 1, shards)
        part = {n: t[n] for n in names[s::shards]}
        save_file(part, os.path.join(d, fn))
        wm.update({n: fn for n in part})
    json.dump({"weight_map": wm}, open(os.path.join(d, "model.safetensors.index.json"), "w"))
    return d


@pytest.fixture(scope="module")
def hf_case():
    hp = dict(n_vocab=140, n_max_tokens=32, n_embd=64, n_intermediate=128, n_head=2, n_layer=2)
    vocab = bertpy.synthetic_vocab(hp["n_vocab"])
    return hp, vocab


@pytest.mark.parametrize("n_labels,shards", [(1, 1), (3, 3)])
def test_convert_hf_head_bytes(lib, hf_case, tmp_path, n_labels, shards):
    hp, vocab = hf_case
    tensors = bertpy.synthetic_tensors(hp, seed=5)
    tensors.update(RR.head_tensors(hp["n_embd"], n_labels, 9))
    d = _hf_dir(str(tmp_path / "hf"), tensors, hp, vocab, shards)
    for ftype in (0, 1):
        want, want_plain = str(tmp_path / "want.bin"), str(tmp_path / "want_plain.bin")
        bertpy.write_model(want, hp, vocab, tensors, ftype, head=True)
        bertpy.write_model(want_plain, hp, vocab, tensors, ftype)
        got, got_plain = str(tmp_path / "got.bin"), str(tmp_path / "got_plain.bin")
        assert lib.bertx_convert_hf_head(d.encode(), got.encode(), ftype) == 0
        assert lib.bertx_convert_hf(d.encode(), got_plain.encode(), ftype) == 0
        assert open(got, "rb").read() == open(want, "rb").read()
        assert open(got_plain, "rb").read() == open(want_plain, "rb").read()
        assert bertpy.BertModel(got).n_labels == n_labels
        assert bertpy.BertModel(got_plain).n_labels == 0


@pytest.mark.parametrize("missing", ["classifier", "pooler"])
def test_convert_hf_head_refuses_a_headless_checkpoint(lib, hf_case, tmp_path, missing, capfd):
    hp, vocab = hf_case
    tensors = bertpy.synthetic_tensors(hp, seed=5)
    tensors.update(RR.head_tensors(hp["n_embd"], 1, 9))
    d = _hf_dir(str(tmp_path / "hf"), tensors, hp, vocab, 1, classifier=missing != "classifier",
                pooler=missing != "pooler")
    out = str(tmp_path / "out.bin")
    assert lib.bertx_convert_hf_head(d.encode(), out.encode(), 1) != 0
    assert "lacks tensor '%s." % missing in capfd.readouterr().err
    assert lib.bertx_convert_hf(d.encode(), out.encode(), 1) == 0


# the reference ------------------------------------------------------------------

def test_reference_with_types(head_models):
    """The extended reference: type-0 input is RefModel's own hidden state (the oracle pin of
    test_cpu_pooling_ref.py); all-one types on M are type-0 input on M with its type rows
    swapped; and the seeded heads leave the tanh unsaturated on the models' [CLS] rows."""
    for tiny in ("tiny32", "tiny64"):
        path = head_models[(tiny, "f32")]
        r = RR.RerankRef(path)
        ids, types = RR.pairs_of_lengths(r.hp["n_vocab"], [3, 20, 64, 65, r.hp["n_max_tokens"]], 4)
        base = ref_forward.RefModel(path)
        h0 = []
        for i, t in zip(ids, types):
            assert np.allclose(r.hidden(i, np.zeros_like(t)), base.hidden(i), rtol=0, atol=1e-12)
            assert np.abs(r.hidden(i, t) - base.hidden(i)).max() > 1e-3 or len(i) == 3
            h0.append(r.hidden(i, t)[0])
        a, p, lg = r.head_of(np.stack(h0))
        assert RR.unsaturated(a), np.mean(np.abs(a) < 2)
        assert lg.shape == (len(ids), r.head[2].shape[0]) and np.isfinite(lg).all()


def test_reference_swap(head_models, tmp_path):
    path = head_models[("tiny64", "q4_1")]
    swapped = RR.swap_type_rows(path, str(tmp_path / "swapped.bin"))
    r, rs = RR.RerankRef(path), RR.RerankRef(swapped)
    ids, types = RR.pairs_of_lengths(692, [40], 1)
    assert np.allclose(r.hidden(ids[0], np.ones_like(types[0])), rs.hidden(ids[0]), rtol=0, atol=1e-12)


def test_head_fixture_seeds_unsaturated():
    """The head-kernel test's operands (x ~ N(0, 1), Wp ~ N(0, 1/d)) meet the tanh condition."""
    for d in (64, 384, 1024):
        for nl in (1, 3):
            t = RR.head_tensors(d, nl, 100 + d + nl)
            x = np.random.default_rng(d + nl).standard_normal((65, d)).astype(np.float32)
            a = x.astype(np.float64) @ t["pooler.dense.weight"].astype(np.float64).T + t["pooler.dense.bias"]
            assert RR.unsaturated(a), (d, nl, np.mean(np.abs(a) < 2))
