"""References of the embedding index's row masks (bertx_index_remove, bertx_index_search_filtered;
bert_hip.h "Deleting rows and filtered search").

A mask packs 32 rows to a uint32 word: row r is bit r % 32 of word r / 32, which is
np.packbits(x, bitorder="little") viewed as uint32.  Tombstones: 1 = deleted.  Filters:
1 = the row may be returned.  A row is admissible for query b iff id < size, its tombstone
is 0 and (when a filter is given) its filter bit is 1.  The result of a masked search is
select(): the k best admissible rows by (score descending, id ascending) with the scorer's
bits and the (-inf, -1) fill.  Nothing here has a tolerance.
"""
import numpy as np


def words_for(n):
    return (int(n) + 31) // 32


def pack_bits(x, words=None):
    """uint32 [words] (x bool [N]) or [B][words] (x bool [B][N]): the packed mask, padded with
    zero bits to whole words; `words` >= ceil(N / 32) pads further."""
    x = np.asarray(x, bool)
    one = x.ndim == 1
    x = np.atleast_2d(x)
    w = words_for(x.shape[1]) if words is None else int(words)
    assert w >= words_for(x.shape[1])
    padded = np.zeros((x.shape[0], 32 * w), bool)
    padded[:, :x.shape[1]] = x
    out = np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint32).reshape(x.shape[0], w)
    return out[0] if one else out


def unpack_bits(words, n):
    """bool [n] / [B][n] out of packed words: bit r % 32 of word r / 32."""
    words = np.ascontiguousarray(np.asarray(words, np.uint32))
    one = words.ndim == 1
    words = np.atleast_2d(words)
    r = np.arange(n)
    out = ((words[:, r // 32] >> (r % 32).astype(np.uint32)) & np.uint32(1)).astype(bool)
    return out[0] if one else out


def tombstones(size, removed_ids):
    """bool [size]: what bertx_index_remove(ids) leaves set on an index of `size` rows with no
    earlier removal: ids outside [0, size) are ignored, repeats are harmless."""
    dead = np.zeros(size, bool)
    for i in np.asarray(removed_ids, np.int64).ravel().tolist():
        if 0 <= i < size:
            dead[i] = True
    return dead


def admissible(size, B, dead=None, allow=None):
    """bool [B][size]: tombstone 0 and, when `allow` (bool [size] or [B][size]) is given, filter 1."""
    ok = np.ones((B, size), bool)
    if dead is not None:
        ok &= ~np.asarray(dead, bool)[None, :size]
    if allow is not None:
        a = np.asarray(allow, bool)
        ok &= (a[None, :size] if a.ndim == 1 else a[:, :size])
    return ok


def select(S, adm, k):
    """(scores f32 [B][k], ids i32 [B][k]): per query the k best admissible rows of the score
    matrix S f32 [B][N] by (score descending, id ascending), S's own bits, (-inf, -1) fill.
    adm: bool [N] or [B][N]."""
    S = np.asarray(S, np.float32)
    B, N = S.shape
    adm = np.asarray(adm, bool)
    if adm.ndim == 1:
        adm = np.broadcast_to(adm, (B, N))
    out_s = np.full((B, k), -np.inf, np.float32)
    out_i = np.full((B, k), -1, np.int32)
    for b in range(B):
        i = np.flatnonzero(adm[b])
        s = S[b, i]
        o = np.lexsort((i, -s.astype(np.float64)))[:k]
        out_s[b, :len(o)] = s[o]
        out_i[b, :len(o)] = i[o]
    return out_s, out_i


def masked_device(S, size, k, tomb_words=None, filt_words=None, honour=True):
    """A stand-in device that works from the packed words as the kernels do: row r of query b is
    offered iff r < size, bit r of tomb_words is 0 and bit r of filter b (filt_words uint32
    [words] shared or [B][words]) is 1.  honour=False ignores both masks: the device a
    comparison must reject."""
    S = np.asarray(S, np.float32)
    B = S.shape[0]
    ok = np.ones((B, size), bool)
    if honour and tomb_words is not None:
        ok &= ~unpack_bits(tomb_words, size)[None, :]
    if honour and filt_words is not None:
        f = unpack_bits(filt_words, size)
        ok &= f[None, :] if f.ndim == 1 else f
    return select(S[:, :size], ok, k)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """(scores, ids) pairs equal bit for bit."""
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))


# the removal patterns of the grid: name -> ids to remove from an index of N rows
def removal_patterns(N, rng):
    edge = [i for i in (0, 15, 16, 31, 32, 63, 64, N - 1) if 0 <= i < N]
    pats = {
        "edges": edge,
        "every row": list(range(N)),
        "all but the last": list(range(N - 1)),
        "a 16-row group": list(range(16, min(32, N))),
        "a 32-row word": list(range(32, min(64, N))),
        "a 64-row step": list(range(64, min(128, N))),
        "a random half": np.flatnonzero(rng.random(N) < 0.5).tolist(),
    }
    return {name: ids for name, ids in pats.items() if len(ids)}
