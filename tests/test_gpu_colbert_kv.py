"""GPU tests of the forward with key counts (bert_hip.h "Key counts"): ColBERT queries whose
[MASK] rows are queries but not attention keys, under every chain; the host and device forms,
graphs, refusals, the store's setting and the search tool's -M.
References and the inputs' condition: colbert_kv_refs.py, test_cpu_colbert_kv.py.

Every accuracy test here fails on a forward that ignores the counts: without counts every row
is more than COS_TOL from the masked reference (asserted below on the same inputs)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bertpy
import colbert_kv_refs as KR
import colbert_refs as CR
import rerank_refs as RR
from row_kernel_refs import bits

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = [(fmt, None) for fmt in RR.FORMATS] + [(fmt, "q8") for fmt in RR.QUANT]
POOLED, TOKENS, LOGITS, PROJ = 0, 1, 2, 3
COS_TOL = KR.COS_TOL


@pytest.fixture(autouse=True, scope="module")
def _one_device():
    old = {k: os.environ.get(k) for k in ("BERT_DEVICES", "BERT_MASK_KEYS")}
    os.environ.pop("BERT_HOST_ONLY", None)
    os.environ.pop("BERT_POOL", None)
    os.environ.pop("BERT_MASK_KEYS", None)
    os.environ["BERT_DEVICES"] = "0"
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def proj_models(lib, tmp_path_factory):
    return CR.make_proj_models(lib, GOLDEN, str(tmp_path_factory.mktemp("projkv")))


@pytest.fixture(scope="module")
def hip():
    return RR.Hip()


_refs = {}


def masked_refs(path):
    """The float64 rows of colbert_kv_refs.queries() with their counts, once per model file."""
    if path not in _refs:
        ref = KR.KVRefModel(path)
        ids, keys = KR.queries()
        _refs[path] = [ref.hidden(i, int(k)) for i, k in zip(ids, keys)]
    return _refs[path]


class KVBatch(CR.ProjBatch):
    """ProjBatch with the key counts on the device: bertx_forward_device_kv."""

    def __init__(self, hip, m, ids, keys):
        super().__init__(hip, m, ids)
        self.d_keys = hip.upload(np.ascontiguousarray(keys, np.int32))

    def kv(self, kind, keys=True, rows=None):
        width = self.width if kind == PROJ else self.m.n_embd
        buf = self.d_proj if kind == PROJ else self.d_out
        self.hip.h.hipMemset(buf, 0xFF, self.T * max(width, 64) * 4)
        d_rows = None if rows is None else self.hip.upload(np.ascontiguousarray(rows, np.int32))
        rc = self.m.lib.bertx_forward_device_kv(self.m.ctx, 0, self.d_ids, None, self.d_cu, self.d_keys if keys else None,
                                                self.B, self.max_len, self.T, kind, d_rows, 0 if rows is None else len(rows),
                                                buf, self.s)
        assert rc == 0, rc
        assert self.hip.h.hipStreamSynchronize(self.s) == 0
        out = self.hip.download(buf, (self.T, width))
        if d_rows is not None:
            self.hip.h.hipFree(d_rows)
        return out

    def close(self):
        self.hip.h.hipFree(self.d_keys)
        super().close()


@pytest.mark.parametrize("tiny", KR.TINIES)
@pytest.mark.parametrize("fmt,act", CHAINS)
def test_forward_with_key_counts(lib, proj_models, hip, tiny, fmt, act):
    path = proj_models[(tiny, fmt)]
    m = bertpy.BertModel(path, act=act)
    dim = CR.DIMS[tiny]
    ids, keys = KR.queries()
    want = masked_refs(path)
    got = m.forward_tokens(ids, n_keys=keys)
    plain = m.forward_tokens(ids)
    trunc = m.forward_tokens([i[:k] for i, k in zip(ids, keys)])
    for g, p, t, w, k in zip(got, plain, trunc, want, keys):
        # a. every row, the [MASK] rows included, against the masked float64 reference
        omc = KR.one_minus_cos(g, w)
        assert omc.max() <= COS_TOL, (len(g), int(k), float(omc.max()))
        # b. rows below the count: the plain forward of the truncated sentence
        assert KR.one_minus_cos(g[:k], t).max() <= COS_TOL
        # c. the same call without counts is somewhere else, on every row
        assert KR.one_minus_cos(p, w).min() > COS_TOL, (len(g), int(k))
    # d. PROJ = the projector (mode 1) on the TOKENS rows of the same call, bit for bit
    W = CR.proj_f32(path)
    proj = m.forward_project(ids, n_keys=keys)
    rc, pw, _ = CR.run_project(lib, 1, np.concatenate(got), None, None, None, W)
    assert rc == 0
    assert np.array_equal(bits(np.concatenate(proj)), bits(pw))
    # e. no counts, and counts equal to the lengths: the existing call's bits
    full = np.array([len(i) for i in ids], np.int32)
    assert np.array_equal(bits(np.concatenate(m.forward_tokens(ids, n_keys=full))), bits(np.concatenate(plain)))
    assert np.array_equal(bits(np.concatenate(m.forward_project(ids, n_keys=full))),
                          bits(np.concatenate(m.forward_project(ids))))
    # f. the device form: the host form's bits with counts (a row map too); with d_keys NULL bertx_forward_device_ex's
    db = KVBatch(hip, m, ids, keys)
    assert np.array_equal(bits(db.kv(TOKENS)), bits(np.concatenate(got)))
    assert np.array_equal(bits(db.kv(PROJ)), bits(np.concatenate(proj)))
    rows = np.arange(db.T - 1, -1, -3).astype(np.int32)
    assert np.array_equal(bits(db.kv(PROJ, rows=rows)[:len(rows)]), bits(np.concatenate(proj)[rows]))
    assert np.array_equal(bits(db.kv(TOKENS, keys=False)), bits(db.ex(TOKENS, types=False)))
    assert np.array_equal(bits(db.kv(PROJ, keys=False)), bits(db.proj()))
    assert np.array_equal(bits(db.kv(PROJ, keys=False)[:, :dim]), bits(np.concatenate(m.forward_project(ids))[:, :dim]))
    db.close()


def test_batch_invariance_across_kernels(proj_models):
    """dh 64, the f16 chain: a 32-token query with 5 keys alone (attention_short), beside a
    100-token sentence (attention_pp), and with the order reversed: the same bits."""
    m = bertpy.BertModel(proj_models[("tiny64", "f16")])
    q, long = KR.query_ids(32, 5), KR.query_ids(100, 40)
    alone = m.forward_tokens([q], n_keys=[5])[0]
    a = m.forward_tokens([q, long], n_keys=[5, 40])
    b = m.forward_tokens([long, q], n_keys=[40, 5])
    assert np.array_equal(bits(alone), bits(a[0]))
    assert np.array_equal(bits(alone), bits(b[1]))
    assert np.array_equal(bits(a[1]), bits(b[0]))
    # (and the counts are not a no-op here)
    assert not np.array_equal(bits(alone), bits(m.forward_tokens([q])[0]))


@pytest.mark.parametrize("fmt,act", [("f16", None), ("f32", None), ("q8_0", "q8")])
def test_graphs_keep_counts_apart(proj_models, hip, fmt, act):
    """One set of pointers, with and without d_keys in turn on one stream (a shape is captured
    on its second use): every call gives the bits of its own first, eager call."""
    m = bertpy.BertModel(proj_models[("tiny64", fmt)], act=act)
    ids, keys = KR.queries()
    db = KVBatch(hip, m, ids, keys)
    with_keys, without = db.kv(TOKENS), db.kv(TOKENS, keys=False)
    assert not np.array_equal(bits(with_keys), bits(without))
    for _ in range(4):
        assert np.array_equal(bits(db.kv(TOKENS)), bits(with_keys))
        assert np.array_equal(bits(db.kv(TOKENS, keys=False)), bits(without))
    db.close()


def test_refusals(lib, proj_models, hip):
    m = bertpy.BertModel(proj_models[("tiny64", "f16")])
    ids, keys = KR.queries()
    db = KVBatch(hip, m, ids, keys)
    L = lib
    for kind in (POOLED, LOGITS, 4, -1):
        for dk in (db.d_keys, None):
            assert L.bertx_forward_device_kv(m.ctx, 0, db.d_ids, None, db.d_cu, dk, db.B, db.max_len, db.T, kind, None, 0,
                                             db.d_out, db.s) == -1
    assert L.bertx_forward_device_kv(m.ctx, 1, db.d_ids, None, db.d_cu, db.d_keys, db.B, db.max_len, db.T, TOKENS, None, 0,
                                     db.d_out, db.s) == -1
    plain = bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))
    assert L.bertx_forward_device_kv(plain.ctx, 0, db.d_ids, None, db.d_cu, db.d_keys, db.B, db.max_len, db.T, PROJ, None,
                                     0, db.d_proj, db.s) == -6
    db.close()
    # the host forms: a count of 0 or over the length, -1 with every output still NaN bits
    import ctypes
    lens = np.array([len(i) for i in ids], np.int32)
    flat = np.ascontiguousarray(np.concatenate(ids))
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uintp)
    tp = (flat.ctypes.data + 4 * offs).astype(np.uintp)
    for fn, width in ((L.bertx_forward_tokens_kv, m.n_embd), (L.bertx_forward_project_kv, m.proj_width)):
        for j, bad in ((0, 0), (3, int(lens[3]) + 1), (4, -1)):
            out = CR.nan_rows(int(lens.sum()), width)
            op = (out.ctypes.data + out.strides[0] * offs).astype(np.uintp)
            k = keys.copy()
            k[j] = bad
            rc = fn(m.ctx, len(ids), tp.ctypes.data_as(ctypes.POINTER(bertpy.c_i32p)), lens.ctypes.data_as(bertpy.c_i32p),
                    k.ctypes.data_as(bertpy.c_i32p), op.ctypes.data_as(ctypes.POINTER(bertpy.c_f32p)))
            assert rc == -1
            assert np.all(out.view(np.uint32) == CR.NAN_BITS)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        m.forward_tokens(ids, n_keys=np.zeros(len(ids), np.int32))


# ---------------------------------------------------------------- the store's setting and the tool

TEXTS = ["stone river, bridge. water!", "plain words without any marks", "one, two, three.",
         "a.b,c;d (e) [f] stone", "river water bridge stone river", "...", "! ? #"]
QUERIES = ["stone bridge", "", "a, b.", "one two three four five six seven eight nine ten " * 4]
QUERY_MAXLEN = 32


@pytest.mark.parametrize("storage", ["f16", "int8"])
def test_store_follows_the_setting(proj_models, storage):
    m = bertpy.BertModel(proj_models[("tiny32", "f16")])
    assert m.mask_keys is True
    mv = bertpy.BertTokenIndex(m, 16, 16 * 64, width=m.proj_width, storage=storage)
    assert mv.add_texts(TEXTS, colbert=48) == 0
    sel = np.array([3, -1, 0, 6, 99, 5], np.int32)
    k = 4
    toks = [m.tokenize_colbert(q, "query", QUERY_MAXLEN, with_keys=True) for q in QUERIES]
    assert [t[2] for t in toks][:3] == [3 + len(CR.pieces(m, q)) for q in QUERIES[:3]] and toks[3][2] == QUERY_MAXLEN
    masked = m.forward_project([t[0] for t in toks], n_keys=[t[2] for t in toks])
    plain = m.forward_project([t[0] for t in toks])
    for on, rows in ((True, plain), (False, masked), (True, plain)):
        m.set_mask_keys(on)
        assert m.mask_keys is on
        for q, r in zip(QUERIES, rows):
            for s in (sel, None):
                assert np.array_equal(bits(mv.score_text(q, s, colbert=QUERY_MAXLEN)), bits(mv.score(r, s))), (on, q)
        sc, ids = mv.search_texts(QUERIES, k, colbert=QUERY_MAXLEN)
        wsc, wids = mv.search(list(rows), k)
        assert np.array_equal(ids, wids) and np.array_equal(bits(sc), bits(wsc)), on
    # the setting matters on these queries, and the document form ignores it
    assert not np.array_equal(bits(mv.score(masked[0])), bits(mv.score(plain[0])))
    m.set_mask_keys(False)
    b = bertpy.BertTokenIndex(m, 16, 16 * 64, width=m.proj_width, storage=storage)
    assert b.add_texts(TEXTS, colbert=48) == 0
    for i in range(len(TEXTS)):
        assert np.array_equal(bits(b.doc(i)), bits(mv.doc(i)))


CHILD = """
import sys
sys.path.insert(0, %r)
import bertpy
try:
    m = bertpy.BertModel(%r)
    print("mask_keys", int(m.mask_keys))
except RuntimeError:
    print("load failed")
"""


@pytest.mark.parametrize("value,want", [("0", "mask_keys 0"), ("1", "mask_keys 1"), ("", "mask_keys 1"),
                                        ("no", "load failed"), ("2", "load failed")])
def test_env_sets_the_setting(proj_models, value, want):
    env = dict(os.environ, BERT_MASK_KEYS=value, BERT_HOST_ONLY="1")
    src = CHILD % (os.path.join(ROOT, "embeddings.cpp_amd"), proj_models[("tiny32", "f16")])
    r = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == want
    if want == "load failed":
        assert "BERT_MASK_KEYS" in r.stderr


def test_search_tool_mask_keys(proj_models, tmp_path):
    """search -L ... -M -a: the ranking of the Python route with the setting off; without -M
    the ranking of today's route; -M without -L is a usage error."""
    base = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
    cpath = proj_models[("tiny32", "f16")]
    c = bertpy.BertModel(cpath)
    texts = TEXTS[:5]
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(texts) + "\n")
    queries = ["stone bridge", "one two", "marks, words"]
    k = 2
    tool = [os.path.join(ROOT, "build", "bin", "search"), "-m", base, "-f", str(corpus), "-k", str(k), "-L", cpath, "-a"]
    mv = bertpy.BertTokenIndex(c, 8, 8 * 192, width=c.proj_width)
    assert mv.add_texts(texts, colbert=min(180, c.n_max_tokens)) == 0
    lines = {}
    for flag, on in (("-M", False), (None, True)):
        r = subprocess.run(tool + ([flag] if flag else []), input="\n".join(queries) + "\nq\n", capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = [ln for ln in r.stdout.splitlines() if "\t" in ln]
        c.set_mask_keys(on)
        sc, ids = mv.search_texts(queries, k, colbert=32)
        want = ["%d\t%d\t%.4f\t%s" % (j + 1, ids[q][j], sc[q][j], texts[ids[q][j]]) for q in range(len(queries))
                for j in range(k)]
        assert got == want, flag
        lines[flag] = got
    assert lines["-M"] != lines[None]
    r = subprocess.run(tool[:7] + ["-M"], input="q\n", capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "usage" in r.stderr
