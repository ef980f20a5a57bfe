"""GPU tests of the ColBERT path: the fused projector alone (bertx_test_project), the
projected output of the forward (BERTX_OUT_PROJ, the row map, the host form) under every
chain, and the text forms of the token store with the search tool on top.
References, fixtures and bounds: colbert_refs.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import colbert_refs as CR
import ref_forward
import rerank_refs as RR
from row_kernel_refs import bits, ptr
from test_cpu_colbert import KERNEL_SHAPES
from test_gpu_pooling import COS_TOL, one_minus_cos

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = [(fmt, None) for fmt in RR.FORMATS] + [(fmt, "q8") for fmt in RR.QUANT]
POOLED, TOKENS, LOGITS, PROJ = 0, 1, 2, 3
ROWS = [1, 15, 16, 17, 63, 64, 65, 129]


@pytest.fixture(autouse=True, scope="module")
def _one_device():
    old = os.environ.get("BERT_DEVICES")
    os.environ.pop("BERT_HOST_ONLY", None)
    os.environ["BERT_DEVICES"] = "0"
    os.environ.pop("BERT_POOL", None)
    yield
    if old is None:
        os.environ.pop("BERT_DEVICES", None)
    else:
        os.environ["BERT_DEVICES"] = old


@pytest.fixture(scope="module")
def proj_models(lib, tmp_path_factory):
    return CR.make_proj_models(lib, GOLDEN, str(tmp_path_factory.mktemp("proj")))


@pytest.fixture(scope="module")
def both_models(lib, tmp_path_factory):
    return CR.make_proj_models(lib, GOLDEN, str(tmp_path_factory.mktemp("both")), head=True)


@pytest.fixture(scope="module")
def hip():
    return RR.Hip()


_cases = {}


def kernel_case(d, dim):
    """One case per shape, shared by the tests and never changed (seeds: test_cpu_colbert)."""
    if (d, dim) not in _cases:
        _cases[(d, dim)] = CR.ProjCase(d, dim, 129, 1000 + d + dim)
    return _cases[(d, dim)]


def is_pos_zero(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint32) == 0))


# 1 --------------------------------------------------------------------------- the kernel

@pytest.mark.parametrize("d,dim", KERNEL_SHAPES)
def test_project_rows_and_accuracy(lib, d, dim):
    """Every row count in both modes gives the bits of the 129-row run on the same rows (a
    row's output depends on that row only), leaves the rows behind n_out and the guard rows
    alone, and writes +0 into the padded columns; the 129-row run is within the unit-row bound
    (the kernel stores no un-normalised p, so E_j is checked through that bound, which it
    dominates: the rounding terms of the normalisation are (dim + 8) U |out_j|)."""
    case = kernel_case(d, dim)
    x0 = CR.tokens_on_device(lib, case)
    for mode, x in ((0, x0), (1, case.x32)):
        full = CR.run_case(lib, case, mode)
        assert np.isfinite(full).all()
        assert is_pos_zero(full[:, dim:])
        for T in ROWS:
            got = CR.run_case(lib, case, mode, T=T)            # (run_case checks the rows behind)
            assert np.array_equal(bits(got), bits(full[:T])), (mode, T)
        p, out, E, bound = CR.project_ref(x, case.W)
        assert CR.well_scaled(p)
        err = np.abs(full[:, :dim].astype(np.float64) - out)
        ratio = float((err / bound).max())
        print("project d %d dim %d mode %d: worst |dout| / bound = %.4f (worst |dout| %.3g)" % (d, dim, mode, ratio,
                                                                                               err.max()))
        assert ratio <= 1.0, ratio
        assert np.allclose(np.linalg.norm(full.astype(np.float64), axis=1), 1.0, rtol=0, atol=(dim + 8) * CR.U * 2)


@pytest.mark.parametrize("d,dim", [(64, 32), (768, 128), (1024, 256)])
def test_project_planted_row(lib, d, dim):
    """One row planted at rows 0, 16, 64 and 128 of a batch, and alone, comes back as the
    same bits every time, in both modes."""
    base = kernel_case(d, dim)
    case = CR.ProjCase(d, dim, 129, 1000 + d + dim)            # a private copy to plant in
    for r in (0, 16, 64, 128):
        case.z[r], case.stats[r], case.x32[r] = base.z[40], base.stats[40], base.x32[40]
    for mode in (0, 1):
        full = CR.run_case(lib, case, mode)
        alone = CR.run_case(lib, case, mode, T=1)
        want = CR.run_case(lib, base, mode)[40]
        for r in (0, 16, 64, 128):
            assert np.array_equal(bits(full[r]), bits(want)), (mode, r)
        assert np.array_equal(bits(alone[0]), bits(want))
        assert not np.array_equal(bits(full[1]), bits(want))


@pytest.mark.parametrize("d,dim", [(64, 32), (384, 96), (1024, 256)])
def test_project_row_map(lib, d, dim):
    """A map that drops rows, repeats a row and reverses the order gives, row for row, the
    bits of the unmapped run; so does a map of one row; only n_out rows are stored."""
    case = kernel_case(d, dim)
    maps = [np.concatenate([np.arange(128, -1, -3), [5, 5, 5], [0, 128]]), np.array([77]), np.arange(0, 129, 2),
            np.array([128] * 17)]
    for mode in (0, 1):
        full = CR.run_case(lib, case, mode)
        for rows in maps:
            got = CR.run_case(lib, case, mode, rows=rows)
            assert got.shape[0] == len(rows)
            assert np.array_equal(bits(got), bits(full[rows])), (mode, len(rows))
    # a row outside [0, T) is refused by the hook before any launch
    rc, _, _ = CR.run_project(lib, 1, case.x32, None, None, None, case.W, rows=np.array([0, 129]))
    assert rc == -1


@pytest.mark.parametrize("d,dim", KERNEL_SHAPES)
def test_project_mode0_equals_mode1_on_the_token_values(lib, d, dim):
    """Mode 1 fed the BERTX_OUT_TOKENS-expression values of the same z, statistics, gamma and
    beta gives the bits of mode 0: one arithmetic for the three chains."""
    case = kernel_case(d, dim)
    x = CR.tokens_on_device(lib, case)
    rc, got, tail = CR.run_project(lib, 1, x, None, None, None, case.W)
    assert rc == 0
    assert np.array_equal(bits(got), bits(CR.run_case(lib, case, 0)))


def test_project_zero_row(lib):
    """An all-zero row with zero beta gives a +0 row, not NaN, in both modes; its neighbours are unchanged."""
    case = CR.ProjCase(384, 96, 129, 1000 + 384 + 96)
    case.b[:] = 0
    base0 = CR.ProjCase(384, 96, 129, 1000 + 384 + 96)
    base0.b[:] = 0
    for r in (0, 17, 128):
        case.z[r] = 0
        case.stats[r] = (0.0, 1.0)
        case.x32[r] = 0
    for mode in (0, 1):
        got, ref = CR.run_case(lib, case, mode), CR.run_case(lib, base0, mode)
        for r in (0, 17, 128):
            assert is_pos_zero(got[r]), (mode, r)
        keep = np.setdiff1d(np.arange(129), [0, 17, 128])
        assert np.array_equal(bits(got[keep]), bits(ref[keep]))


def test_project_refusals(lib):
    x = np.zeros((4, 96), F)
    rc, out, tail = CR.run_project(lib, 1, x, None, None, None, np.zeros((32, 96), F))            # d 96
    assert rc == -1 and np.all(out.view(np.uint32) == CR.NAN_BITS)
    x = np.zeros((4, 128), F)
    rc, out, tail = CR.run_project(lib, 1, x, None, None, None, np.zeros((48, 128), F))           # dim 48
    assert rc == -1 and np.all(out.view(np.uint32) == CR.NAN_BITS)
    rc, out, tail = CR.run_project(lib, 1, x, None, None, None, np.zeros((32, 128), F), out_rows=3)   # out_rows < n_out
    assert rc == -1
    rc, out, tail = CR.run_project(lib, 2, x, None, None, None, np.zeros((32, 128), F))           # no such mode
    assert rc == -1
    rc, out, tail = CR.run_project(lib, 1, x, None, None, None, np.zeros((32, 128), F), pad=0)    # exactly n_out rows
    assert rc == 0


# 2 --------------------------------------------------------------------------- the forward

def ragged(n_vocab, lens, seed):
    rng = np.random.default_rng(seed)
    return [np.concatenate([[101], rng.integers(104, n_vocab, max(L - 2, 0)), [102]])[:L].astype(np.int32) for L in lens]


LENS = [1, 2, 17, 64, 65, 3, 40]


@pytest.mark.parametrize("tiny", ["tiny32", "tiny64"])
@pytest.mark.parametrize("fmt,act", CHAINS)
def test_forward_project(lib, proj_models, hip, tiny, fmt, act):
    path = proj_models[(tiny, fmt)]
    dim, width = CR.DIMS[tiny], 64
    m = bertpy.BertModel(path, act=act)
    assert (m.proj_dim, m.proj_width) == (dim, width)
    ids = ragged(692, LENS, 11)
    W = CR.proj_f32(path)
    db = CR.ProjBatch(hip, m, ids)
    tokens, proj = db.ex(TOKENS, types=False), db.proj()
    # a. OUT_PROJ = the projector (mode 1) on the same call's OUT_TOKENS rows and the file's W
    rc, want, _ = CR.run_project(lib, 1, tokens, None, None, None, W)
    assert rc == 0
    assert np.isfinite(proj).all() and is_pos_zero(proj[:, dim:])
    assert np.array_equal(bits(proj), bits(want))
    # b. the row map: the mapped rows of OUT_PROJ, nothing stored behind them
    rows = np.concatenate([np.arange(db.T - 1, -1, -2), [0, 0, 64]]).astype(np.int32)
    got, tail = db.proj_rows(rows)
    assert np.array_equal(bits(got), bits(proj[rows]))
    assert np.all(tail.view(np.uint32) == CR.NAN_BITS)
    got, tail = db.proj_rows(np.array([db.T - 1]))
    assert np.array_equal(bits(got), bits(proj[-1:]))
    # c. the host form
    host = m.forward_project(ids)
    assert [h.shape for h in host] == [(L, width) for L in LENS]
    assert np.array_equal(bits(np.concatenate(host)), bits(proj))
    # d. against float64: hidden states of the reference times W, normalised
    ref = ref_forward.RefModel(path)
    W64 = W.astype(np.float64)
    for h, i in zip(host, ids):
        p = ref.hidden(i) @ W64.T
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        omc = one_minus_cos(h[:, :dim], p)
        assert omc.max() <= COS_TOL, (len(i), omc.max())
    # e. a sentence alone gives the bits it has inside the batch
    for j in (0, 3, 4):
        alone = CR.ProjBatch(hip, m, [ids[j]])
        assert np.array_equal(bits(alone.proj()), bits(proj[db.cu[j]:db.cu[j + 1]]))
        alone.close()
    # f. a graph replay (the third call of one shape) gives the eager call's bits
    for _ in range(3):
        assert np.array_equal(bits(db.proj()), bits(proj))
    for _ in range(3):
        assert np.array_equal(bits(db.proj_rows(rows)[0]), bits(proj[rows]))
    db.close()


def test_forward_project_refusals(lib, proj_models, hip):
    plain = bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))
    ids = ragged(692, [5, 9], 1)
    db = CR.ProjBatch(hip, plain, ids)
    L = lib
    # a file without the record: the entries of the projection say -6; bertx_forward_device_ex has
    # no kind 3 on such a file and keeps its -1 (test_gpu_rerank.test_device_ex_return_codes)
    assert L.bertx_forward_device_ex(plain.ctx, 0, db.d_ids, None, db.d_cu, db.B, db.max_len, db.T, PROJ, db.d_proj,
                                     db.s) == -1
    assert L.bertx_forward_project_device(plain.ctx, 0, db.d_ids, None, db.d_cu, db.B, db.max_len, db.T, None, 0,
                                          db.d_proj, db.s) == -6
    with pytest.raises(RuntimeError, match=r"\(-6\)"):
        plain.forward_project(ids)
    db.close()
    m = bertpy.BertModel(proj_models[("tiny64", "f16")])
    db = CR.ProjBatch(hip, m, ids)
    assert L.bertx_forward_device_ex(m.ctx, 0, db.d_ids, None, db.d_cu, db.B, db.max_len, db.T, 4, db.d_proj, db.s) == -1
    assert L.bertx_forward_device_ex(m.ctx, 0, db.d_ids, None, db.d_cu, db.B, db.max_len, db.T, -1, db.d_proj, db.s) == -1
    db.close()


@pytest.mark.parametrize("fmt,act", CHAINS)
def test_other_outputs_do_not_see_the_record(both_models, hip, tmp_path, fmt, act):
    """POOLED, TOKENS and LOGITS on a file with the record give the bits of the same file
    with the record dropped."""
    path = both_models[("tiny64", fmt)]
    m = bertpy.BertModel(path, act=act)
    m0 = bertpy.BertModel(RR.drop_record(path, str(tmp_path / "dropped.bin"), CR.REC), act=act)
    assert (m.proj_dim, m0.proj_dim, m.n_labels, m0.n_labels) == (64, 0, 3, 3)
    ids = ragged(692, LENS, 5)
    a, b = RR.DeviceBatch(hip, m, ids), RR.DeviceBatch(hip, m0, ids)
    for kind in (POOLED, TOKENS, LOGITS):
        assert np.array_equal(bits(a.ex(kind, types=False)), bits(b.ex(kind, types=False))), kind
    a.close()
    b.close()


# 3 --------------------------------------------------------------------------- the store

TEXTS = ["stone river, bridge. water!", "...", "", "a.b,c;d (e) [f]", "plain words without any marks",
         " ".join(["stone", "river,", "x.y", "42", "bridge!"] * 12), "! ? #", "one, two, three."]
DOC_MAXLEN, QUERY_MAXLEN = 32, 16


def manual_docs(m, texts, maxlen):
    """tokenize_colbert -> forward_project -> drop the keep == 0 rows."""
    toks = [m.tokenize_colbert(t, "doc", maxlen) for t in texts]
    rows = m.forward_project([i for i, _ in toks])
    return [r[k == 1] for r, (_, k) in zip(rows, toks)], toks


@pytest.mark.parametrize("fmt,act", [("f16", None), ("q4_0", None), ("f32", None), ("q8_0", "q8")])
def test_add_texts_colbert_equals_the_manual_route(proj_models, fmt, act):
    m = bertpy.BertModel(proj_models[("tiny32", fmt)], act=act)
    docs, toks = manual_docs(m, TEXTS, DOC_MAXLEN)
    assert len(toks[5][0]) == DOC_MAXLEN and toks[5][0][-1] == 102          # one text truncates
    assert [len(d) for d in docs][1:3] == [3, 3]                            # punctuation-only and empty: [CLS] [D] [SEP]
    assert any((k == 0).any() for _, k in toks)
    a = bertpy.BertTokenIndex(m, 16, 16 * 32, width=m.proj_width)
    b = bertpy.BertTokenIndex(m, 16, 16 * 32, width=m.proj_width)
    assert a.add_texts(TEXTS, colbert=DOC_MAXLEN) == 0
    assert b.add(docs) == 0
    assert len(a) == len(b) == len(TEXTS) and a.token_slots == b.token_slots
    for i in range(len(TEXTS)):
        assert a.doc_len(i) == b.doc_len(i) == len(docs[i]) >= 3
        assert np.array_equal(bits(a.doc(i)), bits(b.doc(i))), i
    # a second call appends behind the first
    assert a.add_texts(TEXTS[:2], colbert=DOC_MAXLEN) == len(TEXTS)
    assert np.array_equal(bits(a.doc(len(TEXTS))), bits(b.doc(0)))
    # the query: augmented to QUERY_MAXLEN rows, all of which score; ids with -1 and out of range
    ids = np.array([3, -1, 0, 7, 99, 5, 5], np.int32)
    for q in ("stone bridge", "", "a, b."):
        qi, qk = m.tokenize_colbert(q, "query", QUERY_MAXLEN)
        assert len(qi) == QUERY_MAXLEN and np.all(qk == 1)
        qrows = m.forward_project([qi])[0]
        for sel in (ids, None):
            got, want = a.score_text(q, sel, colbert=QUERY_MAXLEN), a.score(qrows, sel)
            assert np.array_equal(bits(got), bits(want))
        assert np.isneginf(a.score_text(q, ids, colbert=QUERY_MAXLEN)[[1, 4]]).all()


def test_add_texts_colbert_across_the_sentence_limit(proj_models):
    """4,097 texts in one call: the last one is a forward of its own.  Two texts of three drop
    punctuation rows, among them the last of the first forward and the only one of the second,
    so neither forward's row map is the identity."""
    m = bertpy.BertModel(proj_models[("tiny32", "f16")])
    vocab = ["stone", "river", "bridge", "water", "plain", "words", "marks", "one", "two", "three"]
    n = 4097

    def text(i):
        a, b, c = vocab[i % 10], vocab[i // 10 % 10], vocab[i // 100 % 10]
        return "%s, %s. %s!" % (a, b, c) if i % 3 != 2 else "%s %s %s %s" % (a, b, c, vocab[i // 1000])

    texts = [text(i) for i in range(n)]
    kept = []
    for t in texts:
        ids, keep = m.tokenize_colbert(t, "doc", DOC_MAXLEN)
        kept.append(int(keep.sum()))
        assert (keep == 0).any() == ("," in t)
    assert "," in texts[4095] and "," in texts[4096] and "," not in texts[4094]
    slots = sum((k + 15) // 16 * 16 for k in kept)
    a = bertpy.BertTokenIndex(m, n, slots, width=m.proj_width)
    assert a.add_texts(texts, colbert=DOC_MAXLEN) == 0
    assert len(a) == n and a.token_slots == slots
    assert [a.doc_len(i) for i in range(n)] == kept
    picks = [0, 1, 2, 4094, 4095, 4096]
    docs, _ = manual_docs(m, [texts[i] for i in picks], DOC_MAXLEN)
    b = bertpy.BertTokenIndex(m, len(picks), sum((len(d) + 15) // 16 * 16 for d in docs), width=m.proj_width)
    assert b.add(docs) == 0
    for j, i in enumerate(picks):
        assert a.doc_len(i) == b.doc_len(j) == len(docs[j]) >= 3
        assert np.array_equal(bits(a.doc(i)), bits(b.doc(j))), i


def test_store_colbert_refusals(lib, proj_models):
    m = bertpy.BertModel(proj_models[("tiny32", "f16")])
    plain = bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))
    texts = bertpy.BertIndex._texts(TEXTS)
    out = np.full(4, 7.0, F)
    ok = bertpy.BertTokenIndex(m, 16, 16 * 32, width=64)
    wide = bertpy.BertTokenIndex(m, 16, 16 * 32, width=128)
    L = lib
    # a store of another width: -1; a model without the record: -6
    assert L.bertx_mvindex_add_texts_colbert(wide.mv, m.ctx, 2, len(TEXTS), texts, DOC_MAXLEN) == -1
    assert L.bertx_mvindex_score_text_colbert(wide.mv, m.ctx, b"q", QUERY_MAXLEN, None, 1, out.ctypes.data) == -1
    assert L.bertx_mvindex_add_texts_colbert(ok.mv, plain.ctx, 2, len(TEXTS), texts, DOC_MAXLEN) == -6
    assert L.bertx_mvindex_score_text_colbert(ok.mv, plain.ctx, b"q", QUERY_MAXLEN, None, 1, out.ctypes.data) == -6
    # maxlen out of range
    assert L.bertx_mvindex_add_texts_colbert(ok.mv, m.ctx, 2, len(TEXTS), texts, 3) == -1
    assert L.bertx_mvindex_add_texts_colbert(ok.mv, m.ctx, 2, len(TEXTS), texts, m.n_max_tokens + 1) == -1
    assert len(ok) == 0 and len(wide) == 0
    assert ok.add_texts(TEXTS, colbert=DOC_MAXLEN) == 0
    assert L.bertx_mvindex_score_text_colbert(ok.mv, m.ctx, b"q", 65, None, 1, out.ctypes.data) == -1
    assert L.bertx_mvindex_score_text_colbert(ok.mv, m.ctx, b"q", 3, None, 1, out.ctypes.data) == -1
    assert np.all(out == 7.0)
    # over either capacity: -2 with nothing added
    docs, _ = manual_docs(m, TEXTS, DOC_MAXLEN)
    slots = sum((len(d) + 15) // 16 * 16 for d in docs)
    tight = bertpy.BertTokenIndex(m, len(TEXTS), slots, width=64)
    assert tight.add_texts(TEXTS, colbert=DOC_MAXLEN) == 0 and tight.token_slots == slots
    for cap_docs, cap_slots in ((len(TEXTS) - 1, slots), (len(TEXTS), slots - 16)):
        small = bertpy.BertTokenIndex(m, cap_docs, cap_slots, width=64)
        assert L.bertx_mvindex_add_texts_colbert(small.mv, m.ctx, 2, len(TEXTS), texts, DOC_MAXLEN) == -2
        assert len(small) == 0 and small.token_slots == 0


def test_search_tool_colbert(proj_models, tmp_path):
    """search -L on a five-line corpus: k lines per query, the ranks of the Python route."""
    base = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
    cpath = proj_models[("tiny32", "f16")]
    m, c = bertpy.BertModel(base), bertpy.BertModel(cpath)
    texts = ["stone river, bridge. water!", "plain words without any marks", "one, two, three.",
             "a.b,c;d (e) [f] stone", "river water bridge stone river"]
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(texts) + "\n")
    queries = ["stone bridge", "one two", "marks, words"]
    k, cand = 2, 5
    tool = [os.path.join(ROOT, "build", "bin", "search"), "-m", base, "-f", str(corpus), "-k", str(k), "-L", cpath, "-c",
            str(cand)]
    r = subprocess.run(tool, input="\n".join(queries) + "\nq\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [ln for ln in r.stdout.splitlines() if "\t" in ln]
    ix = bertpy.BertIndex(m, 8)
    assert ix.add_texts(texts) == 0
    doc_maxlen, query_maxlen = min(180, c.n_max_tokens), 32
    mv = bertpy.BertTokenIndex(c, 8, 8 * 192, width=c.proj_width)
    assert mv.add_texts(texts, colbert=doc_maxlen) == 0
    want = []
    for q in queries:
        cands = ix.search_texts([q], cand)[1][0]
        sc = mv.score_text(q, cands, colbert=query_maxlen)
        order = np.lexsort((cands, -sc.astype(np.float64)))[:k]
        want += ["%d\t%d\t%.4f\t%s" % (j + 1, cands[o], sc[o], texts[cands[o]]) for j, o in enumerate(order)]
    assert len(got) == k * len(queries)
    assert got == want
    # -L excludes -l and -r
    r = subprocess.run(tool + ["-l"], input="q\n", capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "usage" in r.stderr
