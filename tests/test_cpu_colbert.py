"""CPU tests of the ColBERT model side: the optional projection record of the model file
(loader, quantizer), the converter's --colbert form, [Q] / [D] tokenisation, and the
conditions the GPU tests put on their float64 reference.  Tokenizer-only contexts
(BERT_HOST_ONLY=1): no GPU."""
import ctypes
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import bertpy
import colbert_refs as CR
import rerank_refs as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY64 = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")


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
def proj_models(lib, tmp_path_factory):
    return CR.make_proj_models(lib, GOLDEN, str(tmp_path_factory.mktemp("proj")))


@pytest.fixture(scope="module")
def tok(lib):
    return bertpy.BertModel(TINY64)


# 1 --------------------------------------------------------------------------- model file

def test_projection_file_loads_and_reports_dims(proj_models, tok):
    """The test that fails without the feature: the loader knew no linear.weight."""
    for fmt in ("f32", "f16"):
        m = bertpy.BertModel(proj_models[("tiny32", fmt)])
        assert (m.proj_dim, m.proj_width) == (32, 64)
        m = bertpy.BertModel(proj_models[("tiny64", fmt)])
        assert (m.proj_dim, m.proj_width) == (64, 64)
    assert (tok.proj_dim, tok.proj_width) == (0, 0)
    rec = {r[0]: r for r in RR.records(proj_models[("tiny32", "f16")])[1]}[CR.REC]
    assert rec[1] == 2 and rec[2] == 1 and rec[3] == (64, 32)
    rec = {r[0]: r for r in RR.records(proj_models[("tiny32", "f32")])[1]}[CR.REC]
    assert rec[2] == 0


def test_width_rule(tmp_path):
    for dim, width in ((32, 64), (64, 64), (96, 128), (128, 128), (160, 192), (256, 256)):
        p = bertpy.append_projection(TINY64, str(tmp_path / ("w%d.bin" % dim)), CR.proj_weight(64, dim, dim))
        m = bertpy.BertModel(p)
        assert (m.proj_dim, m.proj_width) == (dim, width) and width == CR.width_of(dim)


def test_projection_beside_a_head(lib, tmp_path_factory):
    both = CR.make_proj_models(lib, GOLDEN, str(tmp_path_factory.mktemp("both")), head=True)
    for fmt in ("f16", "q4_0"):
        m = bertpy.BertModel(both[("tiny64", fmt)])
        assert m.n_labels == 3 and m.proj_dim == 64


def _raw_record(name, n_dims, ftype, ne, payload):
    nb = name.encode()
    return struct.pack("<3i", n_dims, len(nb), ftype) + b"".join(struct.pack("<i", v) for v in ne) + nb + payload


@pytest.mark.parametrize("what", ["dim48", "dim288", "one_dim", "ne0"])
def test_bad_projection_records_are_refused(tmp_path, what, capfd):
    base = open(TINY64, "rb").read()
    p = str(tmp_path / "bad.bin")
    if what == "dim48":
        rec = _raw_record(CR.REC, 2, 1, (64, 48), np.zeros((48, 64), np.float16).tobytes())
    elif what == "dim288":
        rec = _raw_record(CR.REC, 2, 1, (64, 288), np.zeros((288, 64), np.float16).tobytes())
    elif what == "one_dim":
        rec = _raw_record(CR.REC, 1, 0, (64,), np.zeros(64, np.float32).tobytes())
    else:
        rec = _raw_record(CR.REC, 2, 1, (32, 64), np.zeros((64, 32), np.float16).tobytes())
    open(p, "wb").write(base + rec)
    with pytest.raises(RuntimeError):
        bertpy.BertModel(p)
    err = capfd.readouterr().err
    assert CR.REC in err and ("wrong shape" in err or "multiple of 32" in err), err


@pytest.mark.parametrize("fmt", RR.QUANT)
def test_quantizer_quantizes_the_projection(proj_models, fmt):
    """bertx_quantize_file's general rule covers the record: 2-D, the name ends in `weight`."""
    for tiny, dim in CR.DIMS.items():
        src, dst = proj_models[(tiny, "f16")], proj_models[(tiny, fmt)]
        assert [r[0] for r in RR.records(src)[1]] == [r[0] for r in RR.records(dst)[1]]
        rec = {r[0]: r for r in RR.records(dst)[1]}[CR.REC]
        assert rec[2] == bertpy.FTYPE[fmt] and rec[3] == (64, dim)
        m = bertpy.BertModel(dst)
        assert m.proj_dim == dim
        # the quantized rows stay near the f16 rows (the block formats' own step)
        a, b = CR.proj_f32(src), CR.proj_f32(dst)
        assert a.shape == b.shape == (dim, 64)
        assert np.abs(a - b).max() <= np.abs(a).max() / (7 if fmt != "q8_0" else 100)


# 2 --------------------------------------------------------------------------- converter

def _colbert_dir(d, tensors, hp, vocab, W=None, bias=None, meta=None):
    from safetensors.numpy import save_file
    os.makedirs(d, exist_ok=True)
    cfg = {"vocab_size": hp["n_vocab"], "max_position_embeddings": hp["n_max_tokens"], "hidden_size": hp["n_embd"],
           "intermediate_size": hp["n_intermediate"], "num_attention_heads": hp["n_head"],
           "num_hidden_layers": hp["n_layer"]}
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("".join(w + "\n" for w in vocab))
    t = {"bert." + n: np.ascontiguousarray(a, np.float32) for n, a in tensors.items()}
    if W is not None:
        t["linear.weight"] = np.ascontiguousarray(W, np.float32)
    if bias is not None:
        t["linear.bias"] = np.ascontiguousarray(bias, np.float32)
    save_file(t, os.path.join(d, "model.safetensors"))
    if meta is not None:
        json.dump(meta, open(os.path.join(d, "artifact.metadata"), "w"))
    return d


@pytest.fixture(scope="module")
def hf_case():
    hp = dict(n_vocab=140, n_max_tokens=32, n_embd=64, n_intermediate=128, n_head=2, n_layer=2)
    return hp, bertpy.synthetic_vocab(hp["n_vocab"]), bertpy.synthetic_tensors(hp, seed=5)


@pytest.mark.parametrize("dim", [32, 96])
def test_convert_colbert(lib, hf_case, tmp_path, dim, capfd):
    hp, vocab, tensors = hf_case
    W = CR.proj_weight(64, dim, 3)
    d = _colbert_dir(str(tmp_path / "hf"), tensors, hp, vocab, W, meta={"attend_to_mask_tokens": False, "dim": dim})
    for ftype in (0, 1):
        plain, want, got = (str(tmp_path / n) for n in ("plain.bin", "want.bin", "got.bin"))
        bertpy.write_model(plain, hp, vocab, tensors, ftype)
        bertpy.append_projection(plain, want, W)
        capfd.readouterr()
        assert lib.bertx_convert_hf_colbert(d.encode(), got.encode(), ftype) == 0
        assert "attend_to_mask_tokens" in capfd.readouterr().out
        assert open(got, "rb").read() == open(want, "rb").read()
        m = bertpy.BertModel(got)
        assert (m.proj_dim, m.proj_width) == (dim, CR.width_of(dim))
        # the record dequantizes to the values written: f32 as they are, f16 rounded once
        back = CR.proj_f32(got)
        assert np.array_equal(back, W if ftype == 0 else W.astype(np.float16).astype(np.float32))
        # the plain converter still reads the same directory and writes no record
        assert lib.bertx_convert_hf(d.encode(), got.encode(), ftype) == 0
        assert open(got, "rb").read() == open(plain, "rb").read()


def test_convert_tool_colbert(hf_case, tmp_path):
    hp, vocab, tensors = hf_case
    d = _colbert_dir(str(tmp_path / "hf"), tensors, hp, vocab, CR.proj_weight(64, 32, 3))
    r = subprocess.run([os.path.join(ROOT, "build", "bin", "convert"), d, "1", "--colbert"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "attend_to_mask_tokens" not in r.stdout          # no metadata file: no line
    assert bertpy.BertModel(os.path.join(d, "ggml-model-f16.bin")).proj_dim == 32


@pytest.mark.parametrize("what", ["missing", "bias", "dim48", "hidden"])
def test_convert_colbert_refuses(lib, hf_case, tmp_path, what, capfd):
    hp, vocab, tensors = hf_case
    W = {"missing": None, "bias": CR.proj_weight(64, 32, 3), "dim48": CR.proj_weight(64, 48, 3),
         "hidden": CR.proj_weight(32, 64, 3)}[what]
    d = _colbert_dir(str(tmp_path / "hf"), tensors, hp, vocab, W, bias=np.zeros(32) if what == "bias" else None)
    out = str(tmp_path / "out.bin")
    assert lib.bertx_convert_hf_colbert(d.encode(), out.encode(), 1) != 0
    err = capfd.readouterr().err
    assert "--colbert" in err and ("linear.bias" if what == "bias" else "linear.weight") in err
    assert not os.path.exists(out)
    assert lib.bertx_convert_hf(d.encode(), out.encode(), 1) == 0


# 3 --------------------------------------------------------------------------- tokenisation

TEXTS = ["", "Hello, World!", "...", "a.b,c;d", "Café NAÏVE (x,y) zzzqqq 42", "[CLS] ! ? # one two",
         " ".join(["stone", "river", "x,y", "42", "naïve"] * 9)]


@pytest.mark.parametrize("maxlen", [4, 8, 32])
def test_tokenize_colbert_matches_restatement(tok, maxlen):
    for text in TEXTS:
        for kind in (0, 1):
            want_ids, want_keep = CR.restated_colbert(tok, text, kind, maxlen)
            ids, keep = tok.tokenize_colbert(text, kind, maxlen)
            assert ids.tolist() == want_ids and keep.tolist() == want_keep, (text, kind)
            assert ids[0] == 101 and ids[1] == (1 if kind == 0 else 2)
            if kind == 0:
                # padded (or truncated) to exactly maxlen, [SEP] kept, [MASK] behind it
                assert len(ids) == maxlen and np.all(keep == 1)
                sep = ids.tolist().index(102)
                assert np.all(ids[sep + 1:] == 103) and sep <= maxlen - 1
            else:
                assert len(ids) == min(len(CR.pieces(tok, text)), maxlen - 3) + 3 and ids[-1] == 102


def test_tokenize_colbert_pieces_are_the_reference_goldens(tok, tok_golden):
    """The pieces between the marker and [SEP] are the reference tokenizer's own ids (the
    committed goldens), not only what this library's bert_tokenize says they are."""
    n = 0
    for c in tok_golden["cases"]:
        g = c["ids"]
        if c["n_max_tokens"] != 512 or len(g) > 200 or g[0] != 101 or g[-1] != 102:
            continue
        text = bytes.fromhex(c["text_hex"])
        if b"\0" in text:
            continue
        for kind, marker in ((0, 1), (1, 2)):
            ids, keep = tok.tokenize_colbert(text, kind, 24)
            want = [101, marker] + g[1:-1][:21] + [102]
            assert ids.tolist()[:len(want)] == want, text
        n += 1
    assert n >= 20, n
    ids, _ = tok.tokenize_colbert("hello world", "doc", 8)
    assert ids.tolist() == [101, 2, 620, 447, 102]


def test_tokenize_colbert_truncation_keeps_sep(tok):
    long = TEXTS[-1]
    assert len(CR.pieces(tok, long)) > 29
    for kind in (0, 1):
        ids, _ = tok.tokenize_colbert(long, kind, 32)
        assert len(ids) == 32 and ids[-1] == 102 and ids[2:31].tolist() == CR.pieces(tok, long)[:29]
    ids, keep = tok.tokenize_colbert("", "query", 8)
    assert ids.tolist() == [101, 1, 102] + [103] * 5 and keep.tolist() == [1] * 8
    ids, keep = tok.tokenize_colbert("", "doc", 8)
    assert ids.tolist() == [101, 2, 102] and keep.tolist() == [1] * 3


def test_skiplist_is_the_32_punctuation_ids(tok):
    """keep is 0 exactly on ids 104 .. 135 of the tiny vocab (the 32 characters of
    string.punctuation) and 1 on every other id, the special ones included."""
    n_vocab = tok.hparams()[0]
    punct = [i for i in range(n_vocab) if tok.id_to_token(i).decode("utf-8", "replace") in CR.PUNCT]
    assert punct == list(range(104, 136))
    text = " ".join(tok.id_to_token(i).decode() for i in range(104, 136)) + " stone 7"
    ids, keep = tok.tokenize_colbert(text, "doc", 64)
    assert ids[2:34].tolist() == list(range(104, 136))
    assert keep.tolist() == [1, 1] + [0] * 32 + [1] * (len(ids) - 34)
    qids, qkeep = tok.tokenize_colbert(text, "query", 64)
    assert np.all(qkeep == 1) and qids[2:34].tolist() == list(range(104, 136))


def test_tokenize_colbert_refusals(tok):
    L = tok.lib
    ids, keep, n = np.full(600, -7, np.int32), np.full(600, -7, np.int32), ctypes.c_int32(-7)
    for kind, maxlen in ((0, 3), (1, 3), (0, tok.n_max_tokens + 1), (1, tok.n_max_tokens + 1), (2, 16), (-1, 16)):
        assert L.bertx_tokenize_colbert(tok.ctx, b"a b", kind, maxlen, ids.ctypes.data, keep.ctypes.data,
                                        ctypes.byref(n)) == -1
    assert np.all(ids == -7) and np.all(keep == -7) and n.value == -7
    assert L.bertx_tokenize_colbert(tok.ctx, b"a b", 1, tok.n_max_tokens, ids.ctypes.data, keep.ctypes.data,
                                    ctypes.byref(n)) == 0


def test_forward_entries_refuse_without_device_or_record(tok, proj_models):
    """Tokenizer-only contexts: the host form refuses; a file without the record says -6 first."""
    ids = np.array([101, 2, 150, 102], np.int32)
    for m, want in ((tok, -6), (bertpy.BertModel(proj_models[("tiny64", "f16")]), -1)):
        with pytest.raises(RuntimeError, match=r"\(%d\)" % want):
            m.forward_project([ids])


# 4 --------------------------------------------------------------------------- the reference's conditions

KERNEL_SHAPES = [(64, 32), (64, 256), (384, 96), (768, 128), (1024, 256), (1024, 32)]


@pytest.mark.parametrize("d,dim", KERNEL_SHAPES)
def test_kernel_cases_are_well_scaled(d, dim):
    """The inputs of the GPU accuracy tests (same seeds): every reference ||p|| >= 0.1 sqrt(dim),
    in both modes, so the normalisation bound divides by nothing small."""
    case = CR.ProjCase(d, dim, 129, 1000 + d + dim)
    for x in (case.ln_f64().astype(np.float32), case.x32):
        p, out, E, bound = CR.project_ref(x, case.W)
        assert CR.well_scaled(p), np.linalg.norm(p, axis=1).min()
        assert np.allclose(np.linalg.norm(out, axis=1), 1.0, rtol=0, atol=1e-12)
        assert np.all(bound > 0) and bound.max() < 1e-2


def test_reference_bound_is_not_vacuous():
    """An f32 dot product in plain ascending order stays inside E, and a one-f16-ulp change of
    one operand leaves it: the bound separates a right kernel from a wrong operand."""
    case = CR.ProjCase(384, 96, 17, 5)
    p, out, E, bound = CR.project_ref(case.x32, case.W)
    a = case.x32.astype(np.float16).astype(np.float32)
    w = case.W.astype(np.float16).astype(np.float32)
    acc = np.zeros((17, 96), np.float32)
    for k in range(384):
        acc += a[:, k:k + 1] * w[None, :, k]
    assert np.all(np.abs(acc - p) <= E)
    a2 = a.copy()
    a2[:, 7] = np.nextafter(a2[:, 7].astype(np.float16), np.float16(np.inf)).astype(np.float32)
    assert np.any(np.abs(a2.astype(np.float64) @ w.astype(np.float64).T - p) > E)
