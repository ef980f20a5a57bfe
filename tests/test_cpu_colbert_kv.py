"""CPU tests of the key-count references (colbert_kv_refs.py) and of bertx_tokenize_colbert_ex
(a tokenizer-only context, BERT_HOST_ONLY=1): no GPU."""
import os

import numpy as np
import pytest

import bertpy
import colbert_kv_refs as KR
import colbert_refs as CR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
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
def tok(lib):
    return bertpy.BertModel(TINY64)


def test_cos_tol_is_the_pooling_tests():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_pooling.py")).read()
    assert "COS_TOL = 1e-3" in src and KR.COS_TOL == 1e-3


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("tiny", KR.TINIES)
def test_masked_reference(tiny, fmt):
    """Rows below the count are the forward of the truncated sentence (no row below the count
    reads anything of the rows behind it); with the count equal to the length the plain
    reference; and every row is at least 5 COS_TOL from the unmasked reference."""
    ref = KR.KVRefModel(os.path.join(GOLDEN, tiny, "ggml-model-%s.bin" % fmt))
    ids, keys = KR.queries()
    assert ref.hp["n_max_tokens"] >= max(len(i) for i in ids)
    worst, least = 0.0, np.inf
    for i, k in zip(ids, keys):
        masked, plain = ref.hidden(i, int(k)), ref.hidden(i)
        worst = max(worst, float(np.abs(masked[:k] - ref.hidden(i[:k])).max()))
        assert np.array_equal(ref.hidden(i, len(i)), plain)
        omc = KR.one_minus_cos(masked, plain)
        least = min(least, float(omc.min()))
        assert omc.min() >= 5 * KR.COS_TOL, (len(i), int(k), float(omc.min()))
    print("\n%s %s: rows below the count vs the truncated forward %.3g; least 1 - cos masked vs unmasked %.3g" %
          (tiny, fmt, worst, least))
    assert worst <= 1e-12


TEXTS = ["", "Hello, World!", "...", "a.b,c;d", "Café NAÏVE (x,y) zzzqqq 42", "[CLS] ! ? # one two",
         " ".join(["stone", "river", "x,y", "42", "naïve"] * 9)]


@pytest.mark.parametrize("maxlen", [4, 8, 32])
def test_tokenize_colbert_ex(tok, maxlen):
    """bertx_tokenize_colbert plus the count: a query's rows up to and including [SEP],
    3 + min(pieces, maxlen - 3); a document's, all of them."""
    for text in TEXTS:
        n_pieces = len(CR.pieces(tok, text))
        for kind in (0, 1):
            want_ids, want_keep = CR.restated_colbert(tok, text, kind, maxlen)
            ids, keep, nk = tok.tokenize_colbert(text, kind, maxlen, with_keys=True)
            assert ids.tolist() == want_ids and keep.tolist() == want_keep, (text, kind)
            ids2, keep2 = tok.tokenize_colbert(text, kind, maxlen)
            assert ids2.tolist() == want_ids and keep2.tolist() == want_keep
            if kind == 0:
                assert nk == 3 + min(n_pieces, maxlen - 3)
                assert ids[nk - 1] == 102 and np.all(ids[nk:] == 103) and not (ids[:nk] == 103).any()
            else:
                assert nk == len(ids)


def test_tokenize_colbert_ex_refusals(tok):
    ids, keep = np.zeros(8, np.int32), np.zeros(8, np.int32)
    import ctypes
    n, nk = ctypes.c_int32(0), ctypes.c_int32(0)
    L = tok.lib
    args = (ids.ctypes.data, keep.ctypes.data, ctypes.byref(n))
    assert L.bertx_tokenize_colbert_ex(tok.ctx, b"x", 0, 8, *args, ctypes.byref(nk)) == 0 and nk.value == 4
    assert L.bertx_tokenize_colbert_ex(tok.ctx, b"x", 0, 8, *args, None) == -1
    assert L.bertx_tokenize_colbert_ex(tok.ctx, b"x", 2, 8, *args, ctypes.byref(nk)) == -1
    assert L.bertx_tokenize_colbert_ex(tok.ctx, b"x", 0, 3, *args, ctypes.byref(nk)) == -1


def test_mask_keys_setting(tok):
    """The context's setting: default on, 0 / 1 accepted, anything else -1 and unchanged."""
    assert tok.mask_keys is True
    tok.set_mask_keys(False)
    assert tok.mask_keys is False
    assert tok.lib.bertx_set_mask_keys(tok.ctx, 2) == -1 and tok.mask_keys is False
    tok.set_mask_keys(True)
    assert tok.mask_keys is True
