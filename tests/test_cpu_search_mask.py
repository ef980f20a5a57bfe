"""The references of the embedding index's row masks (search_mask_refs.py) against brute force,
and the comparison the GPU tests make against a stand-in device that ignores the masks."""
import numpy as np

import search_mask_refs as M
import search_refs as R


def brute_select(S, adm, k):
    """select() as a loop: repeatedly take the best remaining admissible row."""
    B, N = S.shape
    out_s = np.full((B, k), -np.inf, np.float32)
    out_i = np.full((B, k), -1, np.int32)
    for b in range(B):
        left = [i for i in range(N) if adm[b][i]]
        for j in range(k):
            if not left:
                break
            best = left[0]
            for i in left[1:]:
                if S[b, i] > S[b, best] or (S[b, i] == S[b, best] and i < best):
                    best = i
            out_s[b, j], out_i[b, j] = S[b, best], best
            left.remove(best)
    return out_s, out_i


def test_packers_follow_the_bit_definition():
    rng = np.random.default_rng(0)
    for N in (1, 31, 32, 33, 64, 150):
        x = rng.random(N) < 0.4
        w = M.pack_bits(x)
        assert w.dtype == np.uint32 and w.shape == (M.words_for(N),)
        for r in range(32 * len(w)):
            assert ((int(w[r // 32]) >> (r % 32)) & 1) == (int(x[r]) if r < N else 0)
        assert np.array_equal(M.unpack_bits(w, N), x)
        wide = M.pack_bits(x, words=len(w) + 3)
        assert np.array_equal(wide[:len(w)], w) and not wide[len(w):].any()
    x2 = rng.random((5, 70)) < 0.5
    w2 = M.pack_bits(x2)
    assert w2.shape == (5, 3)
    for b in range(5):
        assert np.array_equal(w2[b], M.pack_bits(x2[b]))
    assert np.array_equal(M.unpack_bits(w2, 70), x2)


def test_tombstones_ignore_ids_outside_the_index():
    dead = M.tombstones(150, [0, 15, 16, 31, 32, 63, 64, 149, 149, -1, 150, 2 ** 31 - 1])
    assert np.array_equal(np.flatnonzero(dead), [0, 15, 16, 31, 32, 63, 64, 149])
    assert 150 - dead.sum() == 142


def test_select_equals_brute_force():
    rng = np.random.default_rng(1)
    for B, N, k in ((3, 1, 4), (4, 40, 10), (2, 100, 128), (5, 70, 7)):
        S = rng.integers(-3, 4, (B, N)).astype(np.float32)          # many equal scores
        S[0, :N // 2] = -np.inf if N > 1 else S[0, :N // 2]          # -inf scores are scores, not fill
        for adm in (np.ones((B, N), bool), np.zeros((B, N), bool), rng.random((B, N)) < 0.5, rng.random(N) < 0.3):
            full = np.broadcast_to(adm, (B, N))
            assert M.same(M.select(S, adm, k), brute_select(S, full, k)), (B, N, k)
    # fewer admissible rows than k: the fill
    S = rng.standard_normal((2, 50)).astype(np.float32)
    adm = np.zeros(50, bool)
    adm[[3, 17, 40]] = True
    s, i = M.select(S, adm, 5)
    assert np.all(i[:, 3:] == -1) and np.all(np.isneginf(s[:, 3:])) and set(i[0, :3].tolist()) == {3, 17, 40}


def test_admissible_composes_tombstones_and_filters():
    dead = M.tombstones(10, [2, 5])
    allow = np.zeros((2, 10), bool)
    allow[0, [1, 2, 3]] = True
    allow[1, [5, 9]] = True
    adm = M.admissible(10, 2, dead, allow)
    assert np.array_equal(np.flatnonzero(adm[0]), [1, 3]) and np.array_equal(np.flatnonzero(adm[1]), [9])
    assert np.array_equal(M.admissible(10, 3, dead), np.tile(~dead, (3, 1)))


def test_a_device_that_ignores_the_mask_is_rejected():
    d, N, B, k = 64, 300, 5, 10
    rows, queries, planted = R.planted(d, N, B, k)
    S = (queries.astype(np.float16).astype(np.float32) @ rows.astype(np.float16).astype(np.float32).T)
    dead = M.tombstones(N, planted[:, 0])                  # every query's best row is deleted
    allow = np.ones((B, N), bool)
    allow[np.arange(B), planted[:, 1]] = False             # ... and its second best is filtered out
    tw, fw = M.pack_bits(dead, words=M.words_for(N) + 1), M.pack_bits(allow)
    want = M.select(S, M.admissible(N, B, dead, allow), k)
    good = M.masked_device(S, N, k, tw, fw)
    assert M.same(good, want)
    assert np.array_equal(want[1][:, :k - 2], planted[:, 2:])
    for bad in (M.masked_device(S, N, k, tw, fw, honour=False), M.masked_device(S, N, k, tw, None),
                M.masked_device(S, N, k, None, fw)):
        assert not M.same(bad, want)
    # the unmasked stand-in of the existing tests is the honour=False device
    sc, ids = R.numpy_device(queries, rows.astype(np.float16).astype(np.float32), k)
    assert np.array_equal(ids, M.masked_device(S, N, k, tw, fw, honour=False)[1])
    # a shared filter, and bits of rows >= size, which are ignored whatever they hold
    shared = np.zeros(N, bool)
    shared[::3] = True
    fw1 = M.pack_bits(shared, words=M.words_for(N) + 2)
    fw1[-2:] = 0xFFFFFFFF
    fw1[M.words_for(N) - 1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    got = M.masked_device(S, N, k, None, fw1)
    assert M.same(got, M.select(S, shared, k)) and got[1].max() < N
