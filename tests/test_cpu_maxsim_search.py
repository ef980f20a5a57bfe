"""The host-checkable rules of the full-scan MaxSim search (maxsim_search_refs.py): the
(score, id) order with its fill, the wave-range rule over a (first group, len) table, and
zero-row padding of a query on the CPU references of both storage kinds."""
import numpy as np
import pytest

import maxsim_i8_refs as R8
import maxsim_refs as M
import maxsim_search_refs as SR


# ---- the (score, id) order with fill ----
@pytest.mark.parametrize("n,k", [(0, 1), (0, 5), (1, 1), (3, 10), (9, 10), (10, 10), (11, 10), (40, 7), (200, 128)])
def test_order_against_brute_force(n, k):
    rng = np.random.default_rng(10 * n + k)
    # few distinct values: ties everywhere, and -inf and both zeros among them
    pool = np.array([-np.inf, -1.5, -0.0, 0.0, 0.25, 0.25, 3.0], np.float32)
    scores = pool[rng.integers(0, len(pool), n)]
    s, i = SR.topk(scores, k)
    bs, bi = SR.topk_brute(scores, k)
    assert np.array_equal(i, bi) and np.array_equal(s.view(np.uint32), bs.view(np.uint32))
    m = min(n, k)
    assert np.all(i[m:] == -1) and np.all(np.isneginf(s[m:]))
    for a in range(m - 1):
        assert SR.better(s[a], int(i[a]), s[a + 1], int(i[a + 1]))
    if m:
        assert SR.better(s[m - 1], int(i[m - 1]), SR.NEG_INF, -1)               # a document at -inf still beats the fill
    # the survivors of a tied run cut by k are the lower ids
    kept = set(i[:m].tolist())
    for j in range(n):
        if j not in kept:
            assert all(SR.better(scores[t], t, scores[j], j) for t in kept)


# ---- the wave-range rule ----
def ragged_lens(seed, n):
    rng = np.random.default_rng(seed)
    return rng.choice([1, 15, 16, 17, 33, 100, 512], n)


TABLES = [([], "no documents"), ([512], "a single 512-token document"), ([1, 1, 1], "fewer documents than waves"),
          (ragged_lens(1, 130), "130 ragged"), (ragged_lens(2, 5000), "5,000 ragged"), ([16] * 64, "uniform")]


@pytest.mark.parametrize("lens,name", TABLES, ids=[t[1] for t in TABLES])
@pytest.mark.parametrize("W", [1, 4, 64, 1024, 4096])
def test_wave_ranges_partition_the_documents(lens, name, W):
    table, G = SR.table_of(lens)
    n = len(table)
    ranges = SR.wave_ranges(table, G, W)
    assert len(ranges) == W
    # contiguous and ascending: every document in exactly one range
    at = 0
    for dA, dB in ranges:
        assert dA == at and dB >= dA
        at = dB
    assert at == n
    # a wave streams at most its share of the groups plus one document's
    biggest = max(((int(l) + 15) // 16 for l in lens), default=0)
    for v, r in enumerate(ranges):
        share = (v + 1) * G // W - v * G // W
        assert SR.range_groups(table, G, r) <= share + biggest
    assert sum(SR.range_groups(table, G, r) for r in ranges) == G
    if n == 0:
        assert all(r == (0, 0) for r in ranges)
    if n == 1 and W > 1:
        assert sum(1 for dA, dB in ranges if dB > dA) == 1                     # the 512-token document: one wave, whole


# ---- zero-row padding ----
@pytest.mark.parametrize("w", [64, 192])
def test_zero_row_padding_leaves_the_reference_bits(w):
    rng = np.random.default_rng(w)
    q = M.token_rows(rng, 5, w)
    docs = [M.token_rows(rng, n, w) for n in (1, 17, 33)]
    for Lq in (16, 17, 64):
        qp = SR.pad_rows(q, Lq)
        assert qp.shape == (Lq, w) and not qp[5:].any()
        for d in docs:
            a = SR.maxsim_f32_by_rows(M.f16_view(q), M.f16_view(d))
            b = SR.maxsim_f32_by_rows(M.f16_view(qp), M.f16_view(d))
            assert a.view(np.uint32) == b.view(np.uint32)
            pad = np.float32(M.maxsim_f32(M.f16_view(qp[5:6]), M.f16_view(d)))  # a zero row's maximum: +0, not -0
            assert pad.view(np.uint32) == 0
            a8 = np.float32(R8.score(R8.pack(q), R8.pack(d)))
            b8 = np.float32(R8.score(R8.pack(qp), R8.pack(d)))
            assert a8.view(np.uint32) == b8.view(np.uint32)
    # and the packed zero row: zero bytes and u = 0
    zq, zu = R8.pack(SR.pad_rows(q, 6))
    assert not zq[5].any() and zu[5] == 0 and not M.f16_view(SR.pad_rows(q, 6))[5].any()
