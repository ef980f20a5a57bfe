"""The references of the token store's document masks (maxsim_mask_refs.py) against brute
force, and the comparison the GPU tests make against stand-in devices that ignore a mask."""
import numpy as np
import pytest

import maxsim_mask_refs as MM
import maxsim_search_refs as SR
import search_mask_refs as M


def tied_scores(rng, B, N):
    """f32 [B][N] with many equal scores: a few distinct values, and -inf among them."""
    S = rng.choice(np.array([-np.inf, -1.5, 0.0, 0.25, 0.25, 3.0], np.float32), (B, N))
    return S.astype(np.float32)


@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 65, 300])
def test_expected_is_the_brute_force_selection(N):
    rng = np.random.default_rng(N)
    B = 3
    for S in (rng.standard_normal((B, N)).astype(np.float32), tied_scores(rng, B, N)):
        for name, ids in M.removal_patterns(N, rng).items():
            dead = M.tombstones(N, ids)
            for allow in (None, rng.random(N) < 0.5, MM.per_query_filters(B, N, rng)):
                for k in (1, min(N, 7), min(N + 2, 128)):
                    assert M.same(MM.expected(S, k, dead, allow), MM.brute(S, k, dead, allow)), (name, k)
    dead = M.tombstones(N, range(N))
    s, i = MM.expected(S, 4, dead)
    assert np.all(np.isneginf(s)) and np.all(i == -1)                      # every document deleted: all fill


def test_unmasked_expected_is_the_search_order():
    rng = np.random.default_rng(5)
    S = tied_scores(rng, 2, 90)
    for b in range(2):
        s, i = SR.topk(S[b], 12)
        e = MM.expected(S[b:b + 1], 12)
        assert M.same((s[None], i[None]), e)


@pytest.mark.parametrize("N", [33, 300])
def test_a_device_that_ignores_a_mask_is_rejected(N):
    rng = np.random.default_rng(7 * N)
    B, k = 5, 10
    S = rng.standard_normal((B, N)).astype(np.float32)
    dead = M.tombstones(N, np.flatnonzero(rng.random(N) < 0.3))
    for allow in (rng.random(N) < 0.5, MM.per_query_filters(B, N, rng)):
        words = M.words_for(N) + 2
        tw, fw = M.pack_bits(dead, words), M.pack_bits(allow, words)
        fw = fw.copy()
        fw[..., -1] = 0xFFFFFFFF                                           # garbage beyond docs is ignored
        want = MM.expected(S, k, dead, allow)
        assert M.same(MM.stand_in_device(S, N, k, tw, fw), want)
        assert not M.same(MM.stand_in_device(S, N, k, tw, fw, use_tomb=False), want)
        assert not M.same(MM.stand_in_device(S, N, k, tw, fw, use_filt=False), want)
        assert not M.same(MM.stand_in_device(S, N, k, tw, fw, use_tomb=False, use_filt=False), want)
    # a device that lists a masked document as (-inf, id) instead of leaving it out is rejected too
    dead = M.tombstones(N, range(1, N))
    want = MM.expected(S, 3, dead)
    leaky = (want[0].copy(), want[1].copy())
    leaky[1][:, 1] = 1
    assert np.all(want[1][:, 1:] == -1) and not M.same(leaky, want)


def test_scatter_scores_with_deleted_and_map_live():
    rng = np.random.default_rng(11)
    N, B = 40, 2
    S = rng.standard_normal((B, N)).astype(np.float32)
    full = MM.expected(S, N)
    assert M.same((MM.scatter(*full, N), np.zeros(1)), (S, np.zeros(1)))
    dead = M.tombstones(N, [0, 7, 39])
    ids = np.array([0, 1, 7, 8, -1, N, 39, 38], np.int32)
    got = MM.scores_with_deleted(S[0], ids, dead)
    assert np.isneginf(got[[0, 2, 4, 5, 6]]).all() and np.array_equal(got[[1, 3, 7]], S[0, [1, 8, 38]])
    # a fresh store of the live documents: ids through flatnonzero(live)
    live = np.flatnonzero(~dead)
    fresh = MM.expected(S[:, live], 38)
    assert M.same(MM.map_live(fresh, dead), MM.expected(S, 38, dead))
    assert fresh[1][0, -1] == -1 and MM.map_live(fresh, dead)[1][0, -1] == -1


def test_per_query_filters_cover_the_cases():
    rng = np.random.default_rng(3)
    for B in (2, 3, 5):
        f = MM.per_query_filters(B, 100, rng)
        n = f.sum(axis=0)
        assert (n == B).any() and (n == 0).any() and (n == 1).any()
        for p0 in range(0, B, 4):                                          # per pass of up to four queries
            m = f[p0:p0 + 4].sum(axis=0)
            assert (m == 0).any() and (m == len(f[p0:p0 + 4])).any()
