"""CPU tests of the SPLADE sparse head: the float64 reference against the published
formulation, and the masked-LM head records through the converter, the quantizer and the
loader (BERT_HOST_ONLY=1): no GPU."""
import os
import subprocess

import numpy as np
import pytest

import bertpy
import rerank_refs as RR
import sparse_refs as SR
from test_cpu_abi import _parse_model_file, _write_hf_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY = os.path.join(GOLDEN, "tiny64", "ggml-model-f32.bin")


@pytest.fixture(autouse=True)
def _host_only(monkeypatch):
    monkeypatch.setenv("BERT_HOST_ONLY", "1")


@pytest.mark.parametrize("lens", [[1], [15, 16, 17], [3, 200, 1, 60]])
def test_reference_is_splade_max(lens):
    """log1p(relu(.)) once after the max is the per-token form followed by the max; the planted
    cases hold what their docstring says."""
    case = SR.DecoderCase(64, 130, lens, 7)
    w, m, _ = SR.decoder_ref(case.h, case.E, case.b, case.cu)
    assert np.allclose(w, SR.decoder_naive(case.h, case.E, case.b, case.cu), rtol=1e-14, atol=0)
    l = case.h.astype(np.float64) @ case.E.astype(np.float64).T + case.b
    for s in range(len(lens)):
        seg = l[case.cu[s]:case.cu[s + 1]]
        assert np.all(seg[:, 0::4].argmax(axis=0) == 0) and np.all(seg[:, 1::4].argmax(axis=0) == len(seg) - 1)
        if s:
            assert np.all(l[case.cu[s] - 1, 0::4] > m[s, 0::4])
        if s + 1 < len(lens):
            assert np.all(l[case.cu[s + 1], 1::4] > m[s, 1::4])
    for s, v in case.neg:
        assert m[s, v] < -1 and w[s, v] == 0


def _mlm_dir(path, decoder=None, drop=(), bias_name="cls.predictions.bias"):
    """A BertForMaskedLM directory on the committed tiny64 weights: bert.* encoder, cls.* head."""
    hp, vocab, tens = _parse_model_file(TINY)
    head = SR.mlm_tensors(hp[2], hp[0], 90)
    t = [("bert." + n, a) for n, a in tens]
    t += [(bias_name if n == "cls.predictions.bias" else n, a) for n, a in head.items() if n not in drop]
    if decoder is not None:
        t.append(("cls.predictions.decoder.weight", decoder(dict(tens)[SR.WORD])))
    _write_hf_dir(path, hp, vocab, t)
    return path, head


@pytest.mark.parametrize("ftype", [0, 1])
def test_convert_mlm_round_trip(lib, tmp_path, ftype):
    """The test that fails without the feature.  --mlm on a tied checkpoint (decoder weight absent,
    or present and equal; either bias name) writes plain convert's bytes followed by the five
    records; the file loads, reports n_vocab, and quantizes its 2-D record only."""
    plain, want = str(tmp_path / "plain.bin"), None
    for k, kw in enumerate([dict(), dict(decoder=lambda w: w.copy(), bias_name="cls.predictions.decoder.bias")]):
        d, head = _mlm_dir(str(tmp_path / ("hf%d" % k)), **kw)
        out = str(tmp_path / ("mlm%d.bin" % k))
        assert lib.bertx_convert_hf_mlm(d.encode(), out.encode(), ftype) == 0
        assert lib.bertx_convert_hf(d.encode(), plain.encode(), ftype) == 0
        raw, base = open(out, "rb").read(), open(plain, "rb").read()
        assert base == open(TINY.replace("f32", "f32" if ftype == 0 else "f16"), "rb").read()
        assert raw[:len(base)] == base and len(raw) > len(base)
        assert want is None or raw == want
        want = raw
    recs = RR.records(out)[1][-5:]
    assert [r[0] for r in recs] == bertpy.MLM_NAMES and [r[2] for r in recs] == [ftype, 0, 0, 0, 0]
    for n in bertpy.MLM_NAMES[1:]:
        assert np.array_equal(RR.tensor_f32(out, n).reshape(-1), head[n])
    m = bertpy.BertModel(out)
    assert m.sparse_width == m.hparams()[0] and bertpy.BertModel(plain).sparse_width == 0
    q = str(tmp_path / "q.bin")
    assert lib.bertx_quantize_file(out.encode(), q.encode(), bertpy.FTYPE["q4_0"]) == 0
    assert [r[2] for r in RR.records(q)[1][-5:]] == [bertpy.FTYPE["q4_0"], 0, 0, 0, 0]
    assert bertpy.BertModel(q).sparse_width == m.hparams()[0]
    r = subprocess.run([os.path.join(ROOT, "build", "bin", "convert"), d, str(ftype), "--mlm"], capture_output=True)
    assert r.returncode == 0 and open(os.path.join(d, os.path.basename(TINY).replace("f32", ["f32", "f16"][ftype])),
                                      "rb").read() == want


@pytest.mark.parametrize("what", ["untied", "no_transform", "no_bias"])
def test_convert_mlm_refuses(lib, tmp_path, what, capfd):
    kw = {"untied": dict(decoder=lambda w: w + np.float32(2.0 ** -10) * (np.arange(w.size).reshape(w.shape) == 5)),
          "no_transform": dict(drop=(bertpy.MLM_NAMES[0],)), "no_bias": dict(drop=(bertpy.MLM_NAMES[4],))}[what]
    d, _ = _mlm_dir(str(tmp_path / "hf"), **kw)
    out = str(tmp_path / "x.bin")
    assert lib.bertx_convert_hf_mlm(d.encode(), out.encode(), 1) != 0
    assert not os.path.exists(out)
    assert "--mlm" in capfd.readouterr().err


@pytest.mark.parametrize("missing", range(5))
def test_partial_record_set_is_a_load_error(tmp_path, missing, capfd):
    names = [n for i, n in enumerate(bertpy.MLM_NAMES) if i != missing]
    p = bertpy.append_mlm_head(TINY, str(tmp_path / "part.bin"), SR.mlm_tensors(64, _parse_model_file(TINY)[0][0], 90), names)
    with pytest.raises(RuntimeError):
        bertpy.BertModel(p)
    assert "incomplete masked-LM head" in capfd.readouterr().err
