"""The activation-mode switch at the library's boundary, without a device (BERT_HOST_ONLY=1
contexts): BERT_ACT for the reference's own bert_load_from_file, the act_mode argument of
bertx_load_from_file, and the mode a context reports (bertx_activation_mode): 1 only for
q4_0 / q4_1 / q8_0 files, which are the ones the reference multiplies with q8 activations."""
import pytest


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setenv("BERT_HOST_ONLY", "1")
    monkeypatch.delenv("BERT_ACT", raising=False)
    return monkeypatch


def _load(lib, path, act_mode=None):
    ctx = lib.bert_load_from_file(path.encode()) if act_mode is None else lib.bertx_load_from_file(path.encode(),
                                                                                                   act_mode)
    if not ctx:
        return None
    mode = lib.bertx_activation_mode(ctx)
    lib.bert_free(ctx)
    return mode


def test_bert_act_bogus_is_refused(lib, quant_models, host_only):
    host_only.setenv("BERT_ACT", "bogus")
    for fmt in ("q4_0", "f16"):
        assert not lib.bert_load_from_file(quant_models[("tiny32", fmt)].encode())
    # the argument of bertx_load_from_file is its own: the environment is not consulted
    assert _load(lib, quant_models[("tiny32", "q4_0")], 1) == 1


def test_bert_act_env_selects_the_mode(lib, quant_models, host_only):
    q4, f16 = quant_models[("tiny32", "q4_0")], quant_models[("tiny32", "f16")]
    assert _load(lib, q4) == 0                       # unset: f16 activations
    host_only.setenv("BERT_ACT", "f16")
    assert _load(lib, q4) == 0
    host_only.setenv("BERT_ACT", "q8")                # read at each load, not cached
    assert _load(lib, q4) == 1
    assert _load(lib, f16) == 0                      # no q8 arithmetic for f16 files: loads, mode 0
    host_only.delenv("BERT_ACT")
    assert _load(lib, q4) == 0


@pytest.mark.parametrize("tiny", ["tiny32", "tiny64"])
def test_load_with_act_mode(lib, quant_models, host_only, tiny):
    for fmt, want in (("q4_0", 1), ("q4_1", 1), ("q8_0", 1), ("f16", 0), ("f32", 0)):
        p = quant_models[(tiny, fmt)]
        assert _load(lib, p, 1) == want, fmt
        assert _load(lib, p, 0) == 0, fmt
    for bad in (-1, 2, 8):
        assert not lib.bertx_load_from_file(quant_models[(tiny, "q4_0")].encode(), bad)


def test_bertpy_act_argument(lib, quant_models, host_only):
    import bertpy
    q4 = quant_models[("tiny32", "q4_0")]
    assert bertpy.BertModel(q4, lib=lib, act="q8").activation_mode == 1
    assert bertpy.BertModel(q4, lib=lib, act="f16").activation_mode == 0
    assert bertpy.BertModel(q4, lib=lib).activation_mode == 0
    host_only.setenv("BERT_ACT", "q8")
    assert bertpy.BertModel(q4, lib=lib).activation_mode == 1          # None: the plain ABI call
    assert bertpy.BertModel(q4, lib=lib, act="f16").activation_mode == 0
    with pytest.raises(ValueError):
        bertpy.BertModel(q4, lib=lib, act="int8")
