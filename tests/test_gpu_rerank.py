"""GPU tests of cross-encoder reranking: the head kernel alone, the embedding kernels with
token types, the whole forward through bertx_forward_device_ex (type-0 equivalence, the
type-row swap, logits against the head hook, accuracy against float64, pruned against
unpruned, composition invariance, graph replay), the host entries and the search tool.
References, fixtures and bounds: rerank_refs.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bertpy
import rerank_refs as RR
import row_kernel_refs as R
from row_kernel_refs import PAD, SENT, SENT16, bits, ptr
from test_gpu_pooling import COS_TOL, PRUNE_TOL, one_minus_cos

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = [(fmt, None) for fmt in RR.FORMATS] + [(fmt, "q8") for fmt in RR.QUANT]
POOLED, TOKENS, LOGITS = 0, 1, 2


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


@pytest.fixture(scope="module")
def head_models(lib, tmp_path_factory):
    return RR.make_head_models(lib, GOLDEN, str(tmp_path_factory.mktemp("head")))


@pytest.fixture(scope="module")
def hip():
    return RR.Hip()


def ragged_pairs(n_vocab, lens, seed=3):
    return RR.pairs_of_lengths(n_vocab, lens, seed)


# 4 --------------------------------------------------------------------------- the head kernel

@pytest.mark.parametrize("n_labels", [1, 3])
@pytest.mark.parametrize("d", [64, 384, 1024])
def test_head_kernel(lib, d, n_labels):
    """bertx_test_head against float64 on the same f32 operands: 1, 15, 16, 17 and 65 rows
    (one tile, the tile edge, a second tile, five tiles), every logit within rerank_refs.
    head_bound, the rows behind the n-th untouched, and one row's logits the same bits
    alone, as row 16 of 17 and as row 64 of 65."""
    t = RR.head_tensors(d, n_labels, 100 + d + n_labels)
    wp, bp, wc, bc = (np.ascontiguousarray(t[n]) for n in RR.HEAD)
    X = np.random.default_rng(d + n_labels).standard_normal((65, d)).astype(F)
    X[16] = X[0]
    X[64] = X[0]
    same, worst = [], 0.0
    for n in (1, 15, 16, 17, 65):
        x = X[:n]
        got, tail = RR.run_head(lib, x, wp, bp, wc, bc)
        assert np.all(tail.view(np.uint32) == RR.NAN_BITS), n
        a = x.astype(np.float64) @ wp.astype(np.float64).T + bp
        p = np.tanh(a)
        ref = p @ wc.astype(np.float64).T + bc
        assert RR.unsaturated(a)
        ratio = np.abs(got - ref) / RR.head_bound(x, wp, bp, wc, p)
        worst = max(worst, ratio.max())
        assert np.isfinite(got).all() and ratio.max() <= 1.0, (n, ratio.max())
        same += [got[r] for r in (0, 16, 64) if r < n]
    print("head d %d labels %d: worst error / bound %.3f" % (d, n_labels, worst))
    assert len(same) == 5 + 2 + 1
    for row in same[1:]:
        assert np.array_equal(bits(row), bits(same[0]))


def test_head_kernel_refusals(lib):
    t = RR.head_tensors(64, 1, 1)
    wp, bp, wc, bc = (np.ascontiguousarray(t[n]) for n in RR.HEAD)
    x, out = np.zeros((2, 64), F), np.zeros((2, 1), F)
    args = (wp.ctypes.data, bp.ctypes.data, wc.ctypes.data, bc.ctypes.data)
    assert lib.bertx_test_head(x.ctypes.data, 2, 64, *args, 17, out.ctypes.data, 2) == -1
    assert lib.bertx_test_head(x.ctypes.data, 2, 96, *args, 1, out.ctypes.data, 2) == -1
    assert lib.bertx_test_head(x.ctypes.data, 2, 64, *args, 1, out.ctypes.data, 1) == -1


# 5 --------------------------------------------------------------------------- embedding kernels

def run_embed_types(lib, case, mode, types, old=False):
    d, T = case.d, case.T
    out = np.full((T + PAD, d), SENT16, np.float16) if mode == 0 else np.full((T + PAD, d), SENT, F)
    stats = np.full((T + PAD, 2), SENT, F)
    head = (mode, case.fmts[0], case.fmts[1], case.fmts[2], R.WORD_ROWS, R.POS_ROWS, d, case.raw[0], case.raw[1],
            case.raw[2], ptr(case.g), ptr(case.b), ptr(case.ids))
    tail = (ptr(case.cu), len(case.lens), case.max_len, ptr(out), ptr(stats), T + PAD)
    if old:
        rc = lib.bertx_test_embed_ln(*head, *tail)
    else:
        rc = lib.bertx_test_embed_ln_types(*head, None if types is None else ptr(types), *tail)
    assert rc == 0, rc
    return bits(out), bits(stats)


@pytest.mark.parametrize("d", [64, 384])
@pytest.mark.parametrize("fmt", sorted(R.FMTS))
@pytest.mark.parametrize("mode", [0, 1])
def test_embed_ln_types(lib, oracle, mode, fmt, d):
    """Both embedding kernels, every table format: NULL and all-zero types give the bits of
    bertx_test_embed_ln; all-one types the bits of the same tables with the type rows
    swapped; mixed types, row by row, the all-zero or the all-one result."""
    case = R.EmbedCase((fmt, fmt, fmt), d, seed=fmt)
    swapped = R.EmbedCase.__new__(R.EmbedCase)
    swapped.__dict__.update(case.__dict__)
    h = len(case.raw[1]) // 2
    swapped.raw = [case.raw[0], case.raw[1][h:] + case.raw[1][:h], case.raw[2]]
    T = case.T
    zeros, ones = np.zeros(T, np.int32), np.ones(T, np.int32)
    mixed = (np.random.default_rng(fmt + d).random(T) < 0.5).astype(np.int32)
    assert 0 < mixed.sum() < T
    base = run_embed_types(lib, case, mode, None, old=True)
    for types in (None, zeros):
        got = run_embed_types(lib, case, mode, types)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
    one = run_embed_types(lib, case, mode, ones)
    want = run_embed_types(lib, swapped, mode, None, old=True)
    assert np.array_equal(one[0], want[0]) and np.array_equal(one[1], want[1])
    assert not np.array_equal(one[0][:T], base[0][:T])
    mix = run_embed_types(lib, case, mode, mixed)
    for k in (0, 1):
        sel = np.concatenate([mixed == 1, np.zeros(PAD, bool)])[:, None]
        assert np.array_equal(mix[k], np.where(sel, one[k], base[k]))
    bad = mixed.copy()
    bad[3] = 2
    out = np.zeros((T, d), F)
    assert lib.bertx_test_embed_ln_types(mode, fmt, fmt, fmt, R.WORD_ROWS, R.POS_ROWS, d, case.raw[0], case.raw[1],
                                         case.raw[2], ptr(case.g), ptr(case.b), ptr(case.ids), ptr(bad), ptr(case.cu),
                                         len(case.lens), case.max_len, ptr(out), ptr(out), T) == -1


# 6 --------------------------------------------------------------------------- the whole forward

LENS = [5, 300, 512, 40, 3, 129]


@pytest.mark.parametrize("fmt", ["f32", "f16", "q4_0"])
def test_type0_equivalence(head_models, hip, fmt):
    """a. bertx_forward_device_ex with a NULL types pointer: POOLED gives the bits of
    bertx_forward_device under mean, CLS and pruned-CLS pooling, TOKENS those of
    bertx_forward_tokens_device; an all-zero types array gives them too."""
    m = bertpy.BertModel(head_models[("tiny64", fmt)])
    ids, types = ragged_pairs(692, LENS)
    db = RR.DeviceBatch(hip, m, ids, [np.zeros_like(t) for t in types])
    for pool, prune in (("mean", True), ("cls", False), ("cls", True)):
        m.set_pooling(pool)
        m.set_cls_pruning(prune)
        want = db.old(POOLED)
        assert np.isfinite(want).all()
        assert np.array_equal(bits(db.ex(POOLED, types=False)), bits(want)), (pool, prune)
        assert np.array_equal(bits(db.ex(POOLED, types=True)), bits(want)), (pool, prune)
    want = db.old(TOKENS)
    assert np.array_equal(bits(db.ex(TOKENS, types=False)), bits(want))
    assert np.array_equal(bits(db.ex(TOKENS, types=True)), bits(want))
    db.close()


@pytest.mark.parametrize("fmt,act", CHAINS)
def test_type_row_swap(head_models, hip, tmp_path, fmt, act):
    """b. All-one types on M give the bits of type-0 input on M', M with the two rows of its
    type table exchanged in the file: POOLED and LOGITS, every format, both activation modes."""
    path = head_models[("tiny64", fmt)]
    m = bertpy.BertModel(path, act=act)
    ms = bertpy.BertModel(RR.swap_type_rows(path, str(tmp_path / "swapped.bin")), act=act)
    ids, types = ragged_pairs(692, LENS)
    one = RR.DeviceBatch(hip, m, ids, [np.ones_like(t) for t in types])
    zero = RR.DeviceBatch(hip, ms, ids, None)
    base = RR.DeviceBatch(hip, m, ids, None)
    for kind in (POOLED, LOGITS):
        got, want = one.ex(kind), zero.ex(kind, types=False)
        assert np.isfinite(got).all()
        assert np.array_equal(bits(got), bits(want)), kind
        assert not np.array_equal(bits(got), bits(base.ex(kind, types=False))), kind
    for b in (one, zero, base):
        b.close()


@pytest.mark.parametrize("fmt,act", CHAINS)
def test_logits_are_the_head_of_the_cls_rows(lib, head_models, hip, fmt, act):
    """c. With pruning off, LOGITS gives the bits of bertx_test_head on rows cu[b] of the
    TOKENS output of the same arguments, with the file's head as the library dequantizes it."""
    path = head_models[("tiny64", fmt)]
    m = bertpy.BertModel(path, act=act)
    m.set_cls_pruning(False)
    ids, types = ragged_pairs(692, LENS + [64, 65, 3] * 5)
    db = RR.DeviceBatch(hip, m, ids, types)
    logits, tokens = db.ex(LOGITS), db.ex(TOKENS)
    want, _ = RR.run_head(lib, db.cls_rows(tokens), *RR.head_f32(path))
    assert np.isfinite(logits).all()
    assert np.array_equal(bits(logits), bits(want))
    db.close()


def word_text(m, n, seed):
    rng = np.random.default_rng(seed)
    pool = [w for w in (m.id_to_token(i).decode() for i in range(104, 692)) if w.isalnum() and w.isascii()]
    return " ".join(pool[int(i)] for i in rng.integers(0, len(pool), n))


def accuracy_batches(m):
    """Mixed-type pairs: the n_max pair reached by truncation (text), 3 / 64 / 65 tokens, and
    fillers; as the batches of test d: each special length alone, 17 pairs of at most 64
    tokens (the short attention path), 65 pairs with every length."""
    n_max = m.n_max_tokens
    long_pair = m.tokenize_pair(word_text(m, 400, 1), word_text(m, 300, 2), truncate=True)
    assert len(long_pair[0]) == n_max
    rng = np.random.default_rng(17)
    short = [3, 64] + [int(x) for x in rng.integers(4, 64, 15)]
    i17, t17 = ragged_pairs(692, short, seed=21)
    rest = [65] + [int(x) for x in rng.integers(3, 70, 46)]
    ir, tr = ragged_pairs(692, rest, seed=22)
    ids, types = [long_pair[0]] + i17 + ir, [long_pair[1]] + t17 + tr
    assert len(ids) == 65
    alone = [0, 1, 2, 18]            # n_max, 3, 64, 65 tokens
    assert [len(ids[i]) for i in alone] == [n_max, 3, 64, 65]
    batches = [[i] for i in alone] + [list(range(1, 18)), list(range(65))]
    return ids, types, batches


@pytest.fixture(scope="module")
def accuracy_reference(head_models):
    """Per (tiny, fmt): the pairs, the batches and the float64 hidden states, computed once."""
    cache = {}

    def get(tiny, fmt):
        if (tiny, fmt) not in cache:
            path = head_models[(tiny, fmt)]
            m = bertpy.BertModel(path)
            ids, types, batches = accuracy_batches(m)
            r = RR.RerankRef(path)
            hid = [r.hidden(i, t) for i, t in zip(ids, types)]
            for h in hid:
                h.setflags(write=False)
            cache[(tiny, fmt)] = (m, r, ids, types, batches, hid)
        return cache[(tiny, fmt)]
    return get


@pytest.mark.parametrize("fmt", RR.FORMATS)
@pytest.mark.parametrize("tiny", ["tiny32", "tiny64"])
def test_accuracy_against_float64(accuracy_reference, hip, tiny, fmt):
    """d. Mixed-type pairs against the float64 reference.  TOKENS is held to COS_TOL; each
    logit to ||wc_c|| ||Wp||_2 ||h_gpu - h_ref|| (tanh is 1-Lipschitz) plus head_bound on
    h_gpu, the [CLS] row of the same run's TOKENS output.  Pruning is off, so the logits are
    the head of exactly those rows (test c); test e holds the pruned logits to the unpruned."""
    m, r, ids, types, batches, hid = accuracy_reference(tiny, fmt)
    m.set_cls_pruning(False)
    wp, bp, wc, bc = r.head
    lip = np.linalg.norm(wc, axis=1) * np.linalg.norm(wp, 2)          # [n_labels]
    worst, worst_cos = 0.0, 0.0
    for sel in batches:
        db = RR.DeviceBatch(hip, m, [ids[i] for i in sel], [types[i] for i in sel])
        tokens, logits = db.ex(TOKENS), db.ex(LOGITS)
        assert np.isfinite(tokens).all() and np.isfinite(logits).all()
        for k, i in enumerate(sel):
            worst_cos = max(worst_cos, one_minus_cos(tokens[db.cu[k]:db.cu[k + 1]], hid[i]).max())
        h_gpu = db.cls_rows(tokens)
        h_ref = np.stack([hid[i][0] for i in sel])
        a, p, ref = r.head_of(h_ref)
        assert RR.unsaturated(a), np.mean(np.abs(a) < 2)
        p_gpu = np.tanh(h_gpu.astype(np.float64) @ wp.T + bp)
        bound = np.linalg.norm(h_gpu - h_ref, axis=1)[:, None] * lip[None, :] + RR.head_bound(h_gpu, wp, bp, wc, p_gpu)
        worst = max(worst, (np.abs(logits - ref) / bound).max())
        db.close()
    print("%s %s: tokens max 1 - cos %.3g, logits worst error / bound %.3f" % (tiny, fmt, worst_cos, worst))
    assert worst_cos <= COS_TOL
    assert worst <= 1.0


def pruned_vs_unpruned(m, hip, ids, types, path):
    """e. (max 1 - cos of the pruned against the unpruned [CLS] rows, worst logit difference /
    bound).  The [CLS]-row difference: POOLED under CLS with pruning on and off, brought back
    to the rows' scale by the norm of the unpruned TOKENS row."""
    wp, bp, wc, bc = (a.astype(np.float64) for a in RR.head_f32(path))
    lip = np.linalg.norm(wc, axis=1) * np.linalg.norm(wp, 2)
    db = RR.DeviceBatch(hip, m, ids, types)
    m.set_pooling("cls")
    m.set_cls_pruning(True)
    pooled_p, logits_p = db.ex(POOLED), db.ex(LOGITS)
    m.set_cls_pruning(False)
    pooled_u, logits_u, tokens = db.ex(POOLED), db.ex(LOGITS), db.ex(TOKENS)
    m.set_pooling("mean")
    h_u = db.cls_rows(tokens).astype(np.float64)
    db.close()
    assert np.isfinite(logits_p).all() and np.isfinite(logits_u).all()
    diff = (pooled_p.astype(np.float64) - pooled_u) * np.linalg.norm(h_u, axis=1, keepdims=True)
    p_u = np.tanh(h_u @ wp.T + bp)
    assert RR.unsaturated(h_u @ wp.T + bp)
    bound = np.linalg.norm(diff, axis=1)[:, None] * lip[None, :] + RR.head_bound(h_u, wp, bp, wc, p_u)
    return one_minus_cos(pooled_p, pooled_u).max(), (np.abs(logits_p.astype(np.float64) - logits_u) / bound).max()


@pytest.mark.parametrize("fmt", ["f16"] + RR.QUANT)
def test_pruned_logits_match_unpruned_tiny(head_models, hip, fmt):
    path = head_models[("tiny64", fmt)]
    m = bertpy.BertModel(path)
    rng = np.random.default_rng(11)
    for name, lens in (("ragged", LENS + [17, 64, 65, 100, 511]), ("single", [37]),
                       ("65 short", [int(x) for x in rng.integers(3, 10, 65)])):
        ids, types = ragged_pairs(692, lens, seed=len(lens))
        omc, ratio = pruned_vs_unpruned(m, hip, ids, types, path)
        print("%s %s: pruned vs unpruned [CLS] 1 - cos %.3g, logits worst difference / bound %.3f" % (fmt, name, omc, ratio))
        assert omc <= PRUNE_TOL and ratio <= 1.0, (name, omc, ratio)


def test_pruned_logits_match_unpruned_bge_base(lib, hip, tmp_path):
    """The case of test_pruned_matches_unpruned_bge_base, with a head: bge-base dims, q4_0,
    pairs of 512 / 300 / 64 / 7 tokens."""
    hp = bertpy.ARCHS["bge-base-en-v1.5"]
    tensors = bertpy.synthetic_tensors(hp)
    tensors.update(RR.head_tensors(hp["n_embd"], 1, 77))
    f16, path = str(tmp_path / "bge-base-head-f16.bin"), str(tmp_path / "bge-base-head-q4_0.bin")
    bertpy.write_model(f16, hp, bertpy.synthetic_vocab(hp["n_vocab"]), tensors, 1, head=True)
    assert lib.bertx_quantize_file(f16.encode(), path.encode(), 2) == 0
    os.remove(f16)
    m = bertpy.BertModel(path)
    assert m.n_labels == 1
    ids = bertpy.synthetic_ids(4, [512, 300, 64, 7], hp["n_vocab"])
    types = [(np.arange(len(x)) >= (len(x) * 2) // 5).astype(np.int32) for x in ids]
    omc, ratio = pruned_vs_unpruned(m, hip, ids, types, path)
    print("bge-base q4_0: pruned vs unpruned [CLS] 1 - cos %.3g, logits worst difference / bound %.3f" % (omc, ratio))
    assert omc <= PRUNE_TOL and ratio <= 1.0, (omc, ratio)


@pytest.mark.parametrize("fmt", ["q4_0", "f32"])
def test_composition_invariance_bitwise(head_models, hip, fmt):
    """f. A pair's logits alone are its logits inside a ragged batch of 65, at any position,
    with the pruned last layer and without."""
    m = bertpy.BertModel(head_models[("tiny64", fmt)])
    rng = np.random.default_rng(5)
    lens = [512, 3, 64, 65, 129] + [int(x) for x in rng.integers(3, 200, 60)]
    ids, types = ragged_pairs(692, lens, seed=8)
    for prune in (True, False):
        m.set_cls_pruning(prune)
        db = RR.DeviceBatch(hip, m, ids, types)
        full = db.ex(LOGITS)
        db.close()
        rev = RR.DeviceBatch(hip, m, ids[::-1], types[::-1])
        assert np.array_equal(bits(rev.ex(LOGITS)[::-1]), bits(full)), prune
        rev.close()
        for i in (0, 1, 2, 3, 16, 63, 64):
            one = RR.DeviceBatch(hip, m, [ids[i]], [types[i]])
            assert np.array_equal(bits(one.ex(LOGITS)[0]), bits(full[i])), (prune, i)
            one.close()


@pytest.mark.parametrize("fmt", ["q4_0", "f32"])
def test_graph_replay_keeps_kind_and_types(head_models, hip, fmt):
    """g. On one set of pointers and one stream: the eager, captured and replayed calls of
    POOLED and LOGITS, alternating, each keep the bits of their own first result; so do the
    calls with and without the types pointer."""
    m = bertpy.BertModel(head_models[("tiny64", fmt)])
    ids, types = ragged_pairs(692, LENS)
    db = RR.DeviceBatch(hip, m, ids, types)
    first = {}
    for rnd in range(3):
        for key in ((POOLED, True), (LOGITS, True), (POOLED, False), (LOGITS, False)):
            got = db.ex(key[0], types=key[1])
            assert np.isfinite(got).all()
            if rnd == 0:
                first[key] = got
            assert np.array_equal(bits(got), bits(first[key])), (rnd, key)
    assert not np.array_equal(bits(first[(POOLED, True)]), bits(first[(POOLED, False)]))
    assert not np.array_equal(bits(first[(LOGITS, True)]), bits(first[(LOGITS, False)]))
    db.close()


def test_device_ex_return_codes(head_models, hip):
    m = bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))
    ids, types = ragged_pairs(692, [5, 9])
    db = RR.DeviceBatch(hip, m, ids, types)
    args = (db.d_cu, db.B, db.max_len, db.T)
    assert m.lib.bertx_forward_device_ex(m.ctx, 0, db.d_ids, db.d_types, *args, LOGITS, db.d_out, db.s) == -6
    assert m.lib.bertx_forward_device_ex(m.ctx, 0, db.d_ids, db.d_types, *args, 3, db.d_out, db.s) == -1
    assert m.lib.bertx_forward_device_ex(m.ctx, 1, db.d_ids, db.d_types, *args, POOLED, db.d_out, db.s) == -1
    assert m.lib.bertx_forward_device_ex(m.ctx, 0, db.d_ids, db.d_types, db.d_cu, db.B, 513, db.T, POOLED, db.d_out,
                                         db.s) == -4
    db.close()


# 7 --------------------------------------------------------------------------- host entries

def text_pairs(m, n, seed):
    rng = np.random.default_rng(seed)
    return [(word_text(m, int(rng.integers(0, 30)), 100 + 2 * i + seed),
             word_text(m, int(rng.integers(0, 90)), 101 + 2 * i + seed)) for i in range(n)]


def test_host_entries(head_models):
    m = bertpy.BertModel(head_models[("tiny64", "q4_0")])
    assert m.n_labels == 3
    pairs = text_pairs(m, 23, 1) + [(word_text(m, 400, 5), word_text(m, 300, 6)), ("", "")]
    tok = [m.tokenize_pair(a, b) for a, b in pairs]
    ids, types = [t[0] for t in tok], [t[1] for t in tok]
    assert sorted(len(x) for x in ids) != [len(x) for x in ids]        # an unsorted batch
    by_ids = m.score_ids(ids, types)
    assert np.isfinite(by_ids).all()
    assert np.array_equal(bits(m.score_pairs(pairs)), bits(by_ids))
    # outputs at the caller's indices
    for i in (0, 7, 23, 24):
        assert np.array_equal(bits(m.score_ids([ids[i]], [types[i]])[0]), bits(by_ids[i])), i
    # rerank = score_pairs with the query repeated
    q, docs = pairs[3][1], [b for _, b in pairs]
    rr = m.rerank_logits(q, docs)
    assert np.array_equal(bits(rr), bits(m.score_pairs([(q, dd) for dd in docs])))
    top = m.rerank(q, docs, top_k=5)
    assert [i for i, _ in top] == list(np.argsort(-rr[:, 0], kind="stable")[:5])
    assert all(np.float32(s) == rr[i, 0] for i, s in top)


def test_host_entry_refusals(head_models):
    m = bertpy.BertModel(head_models[("tiny64", "q4_0")])
    L, nl = m.lib, m.n_labels
    pairs = text_pairs(m, 4, 2) + [(word_text(m, 400, 5), word_text(m, 300, 6))]
    n = len(pairs)
    ta, tb = (ctypes.c_char_p * n)(), (ctypes.c_char_p * n)()
    for j, (a, b) in enumerate(pairs):
        ta[j], tb[j] = a.encode(), b.encode()
    out = np.full((n, nl), 7.0, F)
    # one pair over n_max without truncation: the whole call fails, outputs untouched
    assert L.bertx_score_pairs(m.ctx, 2, n, ta, tb, 0, out.ctypes.data) < 0
    assert np.all(out == 7.0)
    assert L.bertx_score_pairs(m.ctx, 2, n, ta, tb, 1, out.ctypes.data) == 0
    assert np.isfinite(out).all() and not np.any(out == 7.0)
    # types outside {0, 1}
    ids, types = m.tokenize_pair(*pairs[0])
    bad = types.copy()
    bad[-1] = 2
    lens = np.array([len(ids)], np.int32)
    ip, tp = np.array([ids.ctypes.data], np.uintp), np.array([bad.ctypes.data], np.uintp)
    out = np.full((1, nl), 7.0, F)
    assert L.bertx_score_ids(m.ctx, 1, ip.ctypes.data, tp.ctypes.data, lens.ctypes.data, out.ctypes.data) == -1
    # an input over n_max_tokens
    long_ids, long_types = np.full(513, 200, np.int32), np.zeros(513, np.int32)
    lens = np.array([513], np.int32)
    ip, tp = np.array([long_ids.ctypes.data], np.uintp), np.array([long_types.ctypes.data], np.uintp)
    assert L.bertx_score_ids(m.ctx, 1, ip.ctypes.data, tp.ctypes.data, lens.ctypes.data, out.ctypes.data) == -4
    assert np.all(out == 7.0)
    # a file without a head
    plain = bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))
    assert plain.n_labels == 0
    assert L.bertx_score_pairs(plain.ctx, 2, n, ta, tb, 1, out.ctypes.data) == -6
    assert L.bertx_rerank(plain.ctx, 2, b"q", n, tb, 1, out.ctypes.data) == -6
    lens = np.array([len(ids)], np.int32)
    ip, tp = np.array([ids.ctypes.data], np.uintp), np.array([types.ctypes.data], np.uintp)
    assert L.bertx_score_ids(plain.ctx, 1, ip.ctypes.data, tp.ctypes.data, lens.ctypes.data, out.ctypes.data) == -6
    assert np.all(out == 7.0)


def test_four_replicas_give_the_bits_of_one(head_models, monkeypatch):
    """256 pairs of about 160 tokens (enough for four shares) through bertx_score_ids."""
    path = head_models[("tiny64", "q4_0")]
    rng = np.random.default_rng(9)
    ids, types = ragged_pairs(692, [int(x) for x in rng.integers(130, 190, 256)], seed=10)
    monkeypatch.setenv("BERT_DEVICES", "0")
    one = bertpy.BertModel(path).score_ids(ids, types)
    monkeypatch.setenv("BERT_DEVICES", "0,0,0,0")
    m4 = bertpy.BertModel(path)
    assert m4.lib.bertx_num_devices(m4.ctx) == 4
    four = m4.score_ids(ids, types)
    used = sum(1 for ms, ns, nt in m4.device_last_call() if ns > 0)
    assert used == 4, m4.device_last_call()
    assert np.isfinite(one).all() and np.array_equal(bits(four), bits(one))


# 8 --------------------------------------------------------------------------- the tool

def test_search_tool_reranks(head_models, tmp_path):
    """build/bin/search: without -r, the lines of the index's own k best (its output before
    the option existed); with -r, ids out of the index's N best, in the order and with the
    logits bertpy's rerank gives for the same texts."""
    exe = os.path.join(ROOT, "build", "bin", "search")
    embed = os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin")
    rerank = head_models[("tiny64", "q4_0")]
    m = bertpy.BertModel(embed)
    texts = [word_text(m, 5 + i % 11, 300 + i) for i in range(40)]
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("".join(t + "\n" for t in texts))
    queries = [word_text(m, 6, 900), texts[7]]
    k, N = 3, 10

    def run(extra):
        r = subprocess.run([exe, "-m", embed, "-f", str(corpus), "-k", str(k)] + extra,
                           input="".join(q + "\n" for q in queries) + "q\n", capture_output=True, text=True,
                           timeout=120, env=dict(os.environ, BERT_DEVICES="0"))
        assert r.returncode == 0, r.stderr[-2000:]
        return [l.split("\t") for l in r.stdout.splitlines() if l[:1].isdigit() and "\t" in l]

    idx = bertpy.BertIndex(m, len(texts))
    idx.add_texts(texts)
    scores, ids = idx.search_texts(queries, N)
    plain = run([])
    want = [[str(j + 1), str(int(ids[q][j])), "%.4f" % scores[q][j], texts[int(ids[q][j])]]
            for q in range(len(queries)) for j in range(k)]
    assert plain == want
    rm = bertpy.BertModel(rerank)
    got = run(["-r", rerank, "-c", str(N)])
    assert len(got) == k * len(queries)
    for q, query in enumerate(queries):
        cand = [int(i) for i in ids[q]]
        ranked = rm.rerank(query, [texts[i] for i in cand], top_k=k)
        lines = got[q * k:(q + 1) * k]
        assert [int(l[1]) for l in lines] == [cand[i] for i, _ in ranked]
        assert set(int(l[1]) for l in lines) <= set(cand)
        assert [l[0] for l in lines] == [str(j + 1) for j in range(k)]
        assert [l[2] for l in lines] == ["%.4f" % s for _, s in ranked]
        assert [l[3] for l in lines] == [texts[cand[i]] for i, _ in ranked]
