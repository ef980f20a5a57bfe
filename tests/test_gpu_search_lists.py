"""Lists and the probed search of the embedding index on the GPU (bertx_index_set_lists,
bertx_index_search_probed, search_lists.hip).  The contract is a composition of entries the index
already has, so every comparison is exact equality of ids and of score bits against that
composition: the centroids in a second f16 index, the probed lists as an allow= mask of the flat
filtered search."""
import numpy as np
import pytest

import bertpy
from test_gpu_search import DeviceArrays, _one_device, dev, model_of_width   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

D = 128
BIG = 600   # rows of list 5: 38 groups, ten per wave, more blocks than the scan's ring holds
SIZES = {1: [BIG + 49], 16: [0, 1, 15, 16, 17, BIG] + [3] * 10, 40: [0, 1, 15, 16, 17, BIG] + [5] * 34}


def unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def planted(C, seed=0):
    """(orthonormal centroids [C][D], rows near them in shuffled order with SIZES[C] per list, 65 queries:
    the first 20 near the longest list's centroid, the others near every list in turn)."""
    rng = np.random.default_rng(100 * C + seed)
    cent = np.linalg.qr(rng.standard_normal((D, D)))[0][:C].astype(np.float32)
    owner = rng.permutation(np.repeat(np.arange(C), SIZES[C]))
    rows = unit(cent[owner] + 0.3 * unit(rng.standard_normal((len(owner), D))))
    near = np.r_[np.full(20, int(np.argmax(SIZES[C]))), np.arange(45) % C]
    return cent, rows, unit(cent[near] + 0.3 * unit(rng.standard_normal((65, D))))


_built = {}


@pytest.fixture
def listed(model_of_width):
    """(index with lists, centroid index, rows, queries) for (storage, C), built once and left unchanged."""
    def get(storage, C):
        if (storage, C) not in _built:
            cent, rows, queries = planted(C)
            model = model_of_width(D)
            ix, ci = bertpy.BertIndex(model, len(rows) + 64, storage=storage), bertpy.BertIndex(model, C)
            ix.add(rows), ci.add(cent), ix.set_lists(cent)
            _built[storage, C] = ix, ci, cent, queries
        return _built[storage, C]
    yield get


def composed(ix, ci, q, k, n_probe, allow=None):
    probes = ci.search(q, n_probe)[1]
    mask = (ix.row_lists()[None, :, None] == probes[:, None, :]).any(-1)
    return ix.search(q, k, allow=mask if allow is None else mask & allow)


def same(got, want):
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("storage", ["f16", "int8"])
@pytest.mark.parametrize("C", [1, 16, 40])
def test_assignment(listed, storage, C):
    ix, ci, cent, _ = listed(storage, C)
    stored = ix.rows(0, len(ix))
    assert ix.n_lists() == C and ix.listed_rows() == len(ix)
    assert np.array_equal(ix.row_lists(), ci.search(stored, 1)[1][:, 0])
    c16 = cent.astype(np.float16).astype(np.float64)
    assert np.array_equal(ix.list_centroid(C - 1), c16[C - 1].astype(np.float32))
    S = np.sort(stored.astype(np.float64) @ c16.T, axis=1)
    assert C == 1 or (S[:, -1] - S[:, -2]).min() > 1e-2
    assert np.array_equal(ix.row_lists(), np.argmax(stored.astype(np.float64) @ c16.T, axis=1))
    assert np.array_equal(np.bincount(ix.row_lists(), minlength=C), SIZES[C])


@pytest.mark.parametrize("storage", ["f16", "int8"])
@pytest.mark.parametrize("C", [1, 16, 40])
@pytest.mark.parametrize("n_probe,B,k", [(1, 65, 128), (3, 17, 10), (None, 1, 1), (None, 17, 10), (3, 65, 1)])
def test_probed_equals_composition(listed, storage, C, n_probe, B, k):
    ix, ci, _, queries = listed(storage, C)
    n_probe = C if n_probe is None else min(n_probe, C)
    got = ix.search(queries[:B], k, n_probe=n_probe)
    same(got, composed(ix, ci, queries[:B], k, n_probe))
    if n_probe == C:
        same(got, ix.search(queries[:B], k))
    if n_probe == 1 and k == 128 and C > 1:
        assert (got[1][20:] == -1).any() and (got[1][0] >= 0).all()   # short lists fill, the longest one does not


@pytest.mark.parametrize("storage", ["f16", "int8"])
def test_masks(model_of_width, storage):
    cent, rows, queries = planted(16, seed=1)
    model = model_of_width(D)
    ix, ci = bertpy.BertIndex(model, len(rows), storage=storage), bertpy.BertIndex(model, 16)
    ix.add(rows), ci.add(cent), ix.set_lists(cent)
    gone = np.arange(0, len(rows), 7)
    ix.remove(gone)
    rng = np.random.default_rng(5)
    for allow in (None, rng.random(len(rows)) < 0.5, rng.random((33, len(rows))) < 0.5):
        got = ix.search(queries[:33], 20, allow=allow, n_probe=3)
        assert not np.isin(got[1], gone).any()
        same(got, composed(ix, ci, queries[:33], 20, 3, allow))


def test_stale_and_refusals(model_of_width, dev):
    cent, rows, queries = planted(16, seed=2)
    model = model_of_width(D)
    ix, ci = bertpy.BertIndex(model, len(rows) + 40), bertpy.BertIndex(model, 16)
    with pytest.raises(RuntimeError):
        ix.search(queries[:2], 5, n_probe=1)            # no lists
    ix.add(rows[:-40]), ci.add(cent), ix.set_lists(cent)
    for bad in (17, 129):
        with pytest.raises(RuntimeError):
            ix.search(queries[:2], 5, n_probe=bad)
    ix.add(rows[-40:])
    assert ix.listed_rows() == len(rows) - 40
    dq, ds, di = dev.up(queries[:2]), dev.up(np.full((2, 5), 7.0, np.float32)), dev.up(np.full((2, 5), 7, np.int32))
    assert ix.lib.bertx_index_search_probed_device(ix.idx, dq, 2, 5, 2, None, 0, 0, ds, di, None) == -1
    assert (dev.down(ds, (2, 5), np.float32) == 7.0).all() and (dev.down(di, (2, 5), np.int32) == 7).all()
    got = ix.search(queries, 10, n_probe=2)             # the host form builds first
    assert ix.listed_rows() == len(rows)
    same(got, composed(ix, ci, queries, 10, 2))
    assert ix.lib.bertx_index_search_probed_device(ix.idx, dq, 2, 5, 2, None, 0, 0, ds, di, None) == 0
    want = ix.search(queries[:2], 5, n_probe=2)[1]      # (a host call on the index's stream: the device call is done)
    assert np.array_equal(dev.down(di, (2, 5), np.int32), want)
    ix.clear()
    assert ix.n_lists() == 0
    with pytest.raises(RuntimeError):
        bertpy.BertBinaryIndex(model, 16).set_lists(cent)


@pytest.mark.parametrize("storage", ["f16", "int8"])
def test_training(model_of_width, storage):
    _, rows, _ = planted(16, seed=3)
    model, C, n = model_of_width(D), 12, len(rows)
    a, b = bertpy.BertIndex(model, n, storage=storage), bertpy.BertIndex(model, n, storage=storage)
    a.add(rows), b.add(rows), a.train_lists(C, 3, 9), b.train_lists(C, 3, 9)
    assert np.array_equal(a.row_lists(), b.row_lists())
    assert all(np.array_equal(a.list_centroid(c), b.list_centroid(c)) for c in range(C))
    # one iteration restated: initial centroid c = stored row floor(c n / C), then the f64 mean in ascending row order
    stored = a.rows(0, n)
    b.set_lists(stored[np.arange(C) * n // C])
    first = b.row_lists()
    a.train_lists(C, 1, 0)
    for c in range(C):
        total = np.zeros(D, np.float64)
        for r in np.flatnonzero(first == c):
            total += stored[r].astype(np.float64)
        want = (total / (first == c).sum()).astype(np.float32).astype(np.float16).astype(np.float32)
        assert (first == c).any() and np.array_equal(a.list_centroid(c), want)
