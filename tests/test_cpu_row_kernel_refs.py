"""The references of test_gpu_row_kernels.py checked against each other on the CPU, on the
same inputs and seeds: every numpy-float32 restatement of a kernel sits inside the bound
the GPU test applies to that kernel (so a correct implementation can meet it), the
restated table decode is the oracle's bit for bit, and no f64 -> f32 rounding that a
bitwise assertion depends on lies near a tie.  Prints the worst error / bound per kernel."""
import numpy as np
import pytest

import row_kernel_refs as R
from row_kernel_refs import F, U, bits


def report(name, err, bound):
    w = R.worst(err, bound)
    print("%s: worst error / bound %.3f" % (name, w))
    return w


@pytest.mark.parametrize("fmt", sorted(R.FMTS))
def test_table_decode_is_the_oracles(oracle, fmt):
    for d in R.WIDTHS:
        raw, deq = R.make_table(fmt, R.WORD_ROWS, d, seed=fmt + d)
        assert np.array_equal(bits(R.decode_table_f32(fmt, raw, R.WORD_ROWS, d)), bits(deq))
        # every block has its own scale: neighbouring blocks never decode to the same values
        blocks = deq.reshape(R.WORD_ROWS, d // 32, 32)
        assert not np.any(np.all(blocks[:, 1:] == blocks[:, :-1], axis=2))


def embed_cases():
    for fmt in sorted(R.FMTS):
        for d in R.WIDTHS:
            yield R.EmbedCase((fmt, fmt, fmt), d, seed=fmt), "%s d %d" % (R.FMTS[fmt], d)
    for fmts in ((2, 0, 1), (8, 3, 0)):
        for d in (384, 1024):
            yield R.EmbedCase(fmts, d, seed=20 + fmts[0]), "mixed %s d %d" % (fmts, d)


def test_embed_references(oracle):
    worst = {"mean": 0.0, "rsig": 0.0, "ln": 0.0}
    for case, tag in embed_cases():
        # the restated decode of the case's own tables, and the sum from it
        for f, raw, tab in zip(case.fmts, case.raw, (case.word, case.type, case.pos)):
            assert np.array_equal(bits(R.decode_table_f32(f, raw, tab.shape[0], case.d)), bits(tab)), tag
        y = case.sum_f32()
        assert case.ids.min() == 0 and case.ids.max() == R.WORD_ROWS - 1
        assert case.pos_idx.max() == case.max_len - 1
        mean, r = R.ln_ref(y)
        bm, br = R.embed_stats_bound(y)
        st = R.embed_stats_f32(y)
        worst["mean"] = max(worst["mean"], R.worst(np.abs(st[:, 0] - mean), bm))
        worst["rsig"] = max(worst["rsig"], R.worst(np.abs(st[:, 1] - r), br))
        assert R.ln_tie_ok(y) > 1, tag
        ref, bound = R.ln_ref_bound(y, case.g, case.b)
        worst["ln"] = max(worst["ln"], R.worst(np.abs(R.ln_exact_f32(y, case.g, case.b) - ref), bound))
    for k, v in worst.items():
        print("embed %s: worst error / bound %.3f" % (k, v))
        assert v <= 1


def test_ln_stats_references():
    w = 0.0
    for G in R.STATS_G:
        for rows in R.STATS_ROWS:
            part = R.stats_parts(rows, G, seed=100 * G + rows % 97)
            ref, bound = R.stats_ref(part, rows)
            f32 = R.ln_row_stats_f32(np.ascontiguousarray(part[:, :rows]), 32 * G)
            w = max(w, R.worst(np.abs(f32 - ref), bound))
            # every row has its own mean
            assert len(np.unique(ref[:, 0])) == rows
    print("ln_stats: worst error / bound %.3f" % w)
    assert w <= 1


def test_pool_references():
    for d in R.WIDTHS:
        for lens, max_len in R.POOL_BATCHES:
            case = R.StreamCase(lens, d, seed=d + max_len, pad=max_len)
            ref, bound = R.pool_ref(case, max_len)
            assert report("pool_l2 d %d max_len %d" % (d, max_len), np.abs(R.pool_f32(case, max_len) - ref), bound) <= 1
        case = R.StreamCase(R.LENS, d, seed=d + 2, pad=0)
        v, mag = case.terms()
        assert report("tokens_f32 d %d" % d, np.abs(R.tokens_f32(case) - v), R.C_TOKEN * U * mag) <= 1
        ref, bound = R.cls_ref(case)
        assert report("cls_l2 d %d" % d, np.abs(R.cls_f32(case) - ref), bound) <= 1


def test_f32_ln_references():
    for d in R.WIDTHS:
        x, g, b = R.f32_ln_case(d)
        assert R.ln_tie_ok(x) > 1, d
        ref, bound = R.ln_ref_bound(x, g, b)
        assert report("f32_ln d %d" % d, np.abs(R.ln_exact_f32(x, g, b) - ref), bound) <= 1


def test_tie_check_sees_a_tie():
    """tie_distance is 0 at the midpoint of two f32 values and the offset beside it; a sum
    that is exact in every order is never reported, an inexact one at a midpoint is."""
    assert R.tie_distance(1 + 2.0 ** -24) == 0
    assert R.tie_distance(1 + 2.0 ** -24 + 2.0 ** -40) == 2.0 ** -40
    x = np.tile(np.array([1.0, np.nextafter(F(1), F(2))], F), 32)[None, :]      # mean 1 + 2^-24, exact
    assert R.sum_tie_ratio(x, 1, 64)[0][0] == np.inf
    y = np.array([[2.0 ** 30, 2.0 ** -24, -2.0 ** 30 + 64, 2.0 ** -24]], F)     # span of 54 bits
    assert R.sum_tie_ratio(y, 1, 1)[0][0] < np.inf


@pytest.mark.parametrize("dh", [32, 64])
def test_f32_attention_references(oracle, dh):
    for lens, seed in ((R.ATT_LENS, 0), ([600, 1000, 17], 1)):
        if seed and dh == 32:
            continue                          # (the long batch once: the restatement is the slow part)
        qkv, cu, n_head, d = R.attention_case(dh, lens=lens, seed=seed)
        ref, bound = R.attention_ref(qkv, cu, n_head, d)
        got = R.attention_era_f32(qkv, cu, n_head, d)
        assert report("f32_attention dh %d lens %s" % (dh, lens[:3]), np.abs(got - ref), bound) <= 1


def test_f32_pool_references():
    for d in R.WIDTHS:
        x, cu = R.f32_pool_case(d)
        ref, bound = R.f32_pool_ref(x, cu)
        got, tie = R.f32_pool_era_f32(x, cu)
        assert tie.min() > 1, d
        assert report("f32_pool d %d" % d, np.abs(got - ref), bound) <= 1
        ref, bound = R.f32_cls_ref(x, cu)
        assert report("f32_cls d %d" % d, np.abs(R.f32_cls_f32(x, cu) - ref), bound) <= 1
