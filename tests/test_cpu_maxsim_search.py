"""The host-checkable rules of the full-scan MaxSim search (maxsim_search_refs.py): the
(score, id) order with its fill, the wave-range rule over a (first group, len) table,
zero-row padding of a query on the CPU references of both storage kinds, and what a wave of
the scans sees (documents, flushes, code chunks) at the suite's shapes and at the capped
grids of test_gpu_maxsim_grid.py."""
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


# ---- what a wave sees: the suite's shapes, and the capped grids of test_gpu_maxsim_grid.py ----
def loads(lens, W):
    ld = SR.wave_load(lens, W)
    docs = [dB - dA for dA, dB, g in ld]
    return ld, docs, [sum(g) for dA, dB, g in ld]


@pytest.mark.parametrize("w,n,waves,most_docs,most_groups",
                         [(64, 5000, (4096, 8192), (4, 2), (10, 8)), (64, 130, (304, 304), (1, 1), (7, 7)),
                          (192, 130, (304, 304), (1, 1), (7, 7)), (768, 130, (316, 320), (1, 1), (7, 7))])
def test_the_natural_grids_leave_a_wave_almost_nothing(w, n, waves, most_docs, most_groups):
    """The stores of test_gpu_maxsim_search.py / _pruned.py at 256 CUs: no wave makes a
    mid-stream flush, and no centroid-scan wave reads a second chunk of codes."""
    lens = SR.suite_lens(n, 7 * w + n)
    G = SR.table_of(lens)[1]
    for i, per in enumerate((SR.FULL_WAVES, SR.CENTROID_WAVES)):
        W = SR.natural_waves(G, per)
        ld, docs, groups = loads(lens, W)
        assert (W, max(docs), max(groups)) == (waves[i], most_docs[i], most_groups[i])
        for dA, dB, g in ld:
            if per == SR.FULL_WAVES:
                assert not any(SR.full_scan_flushes(g, w, kind) for kind in ("f16", "int8"))
            else:
                assert not SR.centroid_scan_flushes(g) and SR.code_chunks(g) <= 1


def test_the_capped_grids_give_a_wave_hundreds_of_documents():
    lens = SR.grid_lens()
    assert len(lens) == 1200 and lens[7] == 512 and lens[600] == 257 and SR.table_of(lens)[1] == 2957
    assert set(lens.tolist()) == set(SR.DOC_LENS) | {512, 257}
    want = {1: ((4, 288, 308, 741), (8, 132, 160, 374)), 2: ((8, 132, 160, 374), (16, 62, 86, 190)),
            5: ((20, 50, 71, 151), (40, 18, 44, 80)), 33: ((132, 0, 19, 46), (264, 0, 11, 34))}
    for cap, rows in want.items():
        for per, row in zip((SR.FULL_WAVES, SR.CENTROID_WAVES), rows):
            ld, docs, groups = loads(lens, per * cap)
            assert (per * cap, min(docs), max(docs), max(groups)) == row, (cap, per)
    # the natural grid of this store at 256 CUs lies above every cap used
    assert SR.natural_waves(2957, SR.FULL_WAVES) // SR.FULL_WAVES == 740
    assert SR.natural_waves(2957, SR.CENTROID_WAVES) // SR.CENTROID_WAVES == 370


@pytest.mark.parametrize("w", (64, 192, 768))
@pytest.mark.parametrize("kind", ("f16", "int8"))
def test_capped_full_scan_waves_flush_mid_stream(w, kind):
    lens = SR.grid_lens()
    NU = SR.RING_UNITS[kind]
    for cap, least in ((1, 4), (2, 2)):
        for dA, dB, g in SR.wave_load(lens, SR.FULL_WAVES * cap):
            f = SR.full_scan_flushes(g, w, kind)
            assert len(f) >= least
            # a flush offers 65 - NU .. 64 documents; with k < that a list takes more than k offers
            steps = np.diff([0] + f)
            assert np.all(steps > 64 - NU) and np.all(steps <= 64)
    # cap 5 still flushes in some wave; cap 33 in none (at most 19 documents)
    assert any(SR.full_scan_flushes(g, w, kind) for dA, dB, g in SR.wave_load(lens, SR.FULL_WAVES * 5))
    assert not any(SR.full_scan_flushes(g, w, kind) for dA, dB, g in SR.wave_load(lens, SR.FULL_WAVES * 33))


def test_full_scan_flushes_by_hand():
    # width 64, f16: a unit is a group, a pass four of them; 61 one-group documents are the least that flush
    assert SR.full_scan_flushes([1] * 60, 64, "f16") == []
    assert SR.full_scan_flushes([1] * 63, 64, "f16") == []                  # pass 15 ends at 60 pending; 3 units left over
    assert SR.full_scan_flushes([1] * 64, 64, "f16") == [64]
    assert SR.full_scan_flushes([1] * 130, 64, "f16") == [64, 128]
    assert SR.full_scan_flushes([1] * 130, 64, "int8") == [64, 128]         # passes of 8: 57 .. 64 pending
    assert SR.full_scan_flushes([2] * 130, 64, "f16") == [62, 124]          # two documents a pass: 62 > 60
    assert SR.full_scan_flushes([2] * 130, 64, "int8") == [60, 120]         # four a pass: 60 > 56
    assert SR.full_scan_flushes([1] * 130, 768, "f16") == [61, 122]         # a document takes three passes
    assert SR.full_scan_flushes([1] * 130, 768, "int8") == [57, 114]        # two in three passes: 57 by unit 688
    assert SR.full_scan_flushes([7, 1, 1], 64, "f16") == [] and SR.full_scan_flushes([], 64, "f16") == []
    assert SR.centroid_scan_flushes([1] * 63) == [] and SR.centroid_scan_flushes([3] * 64) == [64]
    assert SR.centroid_scan_flushes([1] * 130) == [64, 128]


def test_code_chunks_by_hand():
    assert [SR.code_chunks(g) for g in ([], [1], [8], [7, 2], [1] * 17)] == [0, 1, 1, 2, 3]
    assert SR.closes_on_chunk_end([3, 5]) and SR.closes_on_chunk_end([8]) and not SR.closes_on_chunk_end([3, 4, 2])
    assert SR.spans_chunks([7, 2]) and SR.spans_chunks([9]) and not SR.spans_chunks([7, 1, 8]) and not SR.spans_chunks([])


def test_capped_centroid_scan_waves_prefetch_and_flush():
    lens = SR.grid_lens()
    for cap in (1, 2):
        ld = SR.wave_load(lens, SR.CENTROID_WAVES * cap)
        for dA, dB, g in ld:
            assert SR.code_chunks(g) >= 3                                   # the hand-over c0 = c1 and the clamped load(ch + 2)
            assert SR.closes_on_chunk_end(g) and SR.spans_chunks(g)
        # 64 pending: every wave at cap 1; at cap 2 every wave but the first (62 documents)
        assert [len(SR.centroid_scan_flushes(g)) >= 1 for dA, dB, g in ld] == [cap == 1] + [True] * (len(ld) - 1)


def test_planted_edges_stay_at_the_edges():
    """test_planted_documents_at_the_edges replaces the first or last document of a range by a
    one-token document; where that document was longer the later documents move up.  Most of
    the planted ids are still the first or last of a range, the others lie within five
    documents of an edge."""
    lens = SR.grid_lens()
    for cap, exact in ((1, 7), (2, 10)):
        W = SR.FULL_WAVES * cap
        edges = SR.edge_ids(lens, W)
        assert len(edges) == 2 * W and len({p for v, side, p in edges}) == 2 * W
        dist = [min(SR.edge_distance(SR.one_token_at(lens, [p]), W, p, s) for s in (0, 1)) for v, side, p in edges]
        assert dist.count(0) >= exact and max(dist) <= 5, dist
        on_side = [SR.edge_distance(SR.one_token_at(lens, [p]), W, p, side) == 0 for v, side, p in edges]
        assert any(on_side[0::2]) and any(on_side[1::2])                    # first ones and last ones among the exact


@pytest.mark.parametrize("w", (64, 192))
@pytest.mark.parametrize("kind", ("f16", "int8"))
def test_tie_ids_lie_around_two_flushes(w, kind):
    lens = SR.grid_lens()
    ids = SR.tie_ids(lens, SR.FULL_WAVES, w, kind)
    assert len(ids) == 9 and len(set(ids)) == 9 and ids[:7] == sorted(ids[:7])
    sides = SR.tie_sides(SR.one_token_at(lens, ids), ids, SR.FULL_WAVES, w, kind)
    assert sides[:7] == [(1, n) for n in SR.TIE_PATTERN] and sides[7][0] == 0 and sides[8][0] == 3
    assert ids[3] - ids[2] <= 8 and ids[6] - ids[5] <= 8                    # neighbours across each flush


# ---- the grid cap's entry points without a GPU ----
def test_grid_hooks_are_exported_and_bound():
    import ctypes
    import re
    import subprocess

    import bertpy
    from conftest import LIB_SO
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_SO], capture_output=True, text=True, check=True).stdout
    have = set(re.findall(r"\bT (bertx_\w+)", out))
    assert {"bertx_test_mvindex_grid", "bertx_test_mvindex_last_grid"} <= have
    lib = bertpy.load_lib()
    assert lib.bertx_test_mvindex_grid.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert lib.bertx_test_mvindex_last_grid.argtypes == [ctypes.c_void_p]
    for cap in (-1, 0, 1):
        assert lib.bertx_test_mvindex_grid(None, cap) == -1                 # no store
    assert lib.bertx_test_mvindex_last_grid(None) == -1
