"""The attention tests' own references, checked without a GPU (attention_refs.py): the numpy
restatements of the kernels meet every per-element bound on every input the GPU file uses
(so the bounds are reachable), planted mutations of the restatements break a bound in every
sentence they touch (so the bounds are tight enough to notice them), the offset-move path is
really taken where a batch claims it, and the planted builders' conditions hold.

Run with -s for the ratio tables."""
import numpy as np
import pytest

import attention_refs as R

# (batch, arithmetic) as test_gpu_attention_kernels.py runs them; ("lds", STREAM) is variant -1
BATTERY = [("short", R.WAVE64), ("lds", R.WAVE64), ("heads3", R.WAVE64), ("heads3_short", R.WAVE64),
           ("lds32", R.LDS32), ("stream64", R.STREAM), ("stream32", R.STREAM), ("lds", R.STREAM),
           ("heads3", R.STREAM), ("cls64", R.CLS), ("cls32", R.CLS)]
IDS = ["%s-%s" % b for b in BATTERY]


def kinds_of(name, arith):
    return R.ALL_KINDS if arith == R.WAVE64 and name in ("lds", "heads3") else R.KINDS


def sentence_ratios(cs, arith, out):
    """Per sentence: the worst |out - want| / bound over the general bound and, for a planted
    input, its own."""
    rows = cs.cu[:-1] if arith == R.CLS else slice(None)
    pairs = [(cs.ref[rows], cs.bound(arith))]
    if cs.kind in ("uniform", "onehot"):
        want, pb = cs.planted_bound(arith)
        pairs.append((want[rows], pb[rows]))
    res = []
    for b in range(len(cs.lens)):
        r = slice(b, b + 1) if arith == R.CLS else slice(int(cs.cu[b]), int(cs.cu[b + 1]))
        res.append(max(R.worst_ratio(out[r], want[r], bd[r]) for want, bd in pairs))
    return np.array(res)


@pytest.fixture(scope="module")
def faithful():
    """The unmutated restatement of every (batch, arithmetic, kind), computed once."""
    cache = {}

    def get(name, arith, kind):
        key = (name, arith, kind)
        if key not in cache:
            cache[key] = R.restate(R.case(name, kind), arith)
        return cache[key]
    return get


@pytest.mark.parametrize("name,arith", BATTERY, ids=IDS)
def test_restatements_meet_every_bound(faithful, name, arith):
    worst = {}
    for kind in kinds_of(name, arith):
        cs = R.case(name, kind)
        out, _ = faithful(name, arith, kind)
        worst[kind] = sentence_ratios(cs, arith, out).max()
    print("\nworst error / bound, restatement %-7s on %-12s: " % (arith, name) +
          "  ".join("%s %.3f" % kv for kv in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def touched(cs, arith, mut, moves):
    """The sentences a mutation changes (so a bound has to notice it there)."""
    L = np.array(cs.lens)
    if mut in ("drop_last", "drop_block_first"):
        return L >= 1
    if mut == "swap_v":
        return L >= 2
    if mut == "mask_gt":
        # a key past the end exists only inside a block; in the LDS images it is a copy of the
        # last key, and a copy of a sentence's only key changes nothing
        return (L % 64 != 0) & ((L > 1) | (arith == R.STREAM))
    if mut == "unrounded_offset":             # block 0 alone has no bias operand to disagree with
        return L > 64
    if mut == "skip_rescale":                 # some query of the sentence moved its offset
        nh = cs.n_head
        return np.array([any(moves[b * nh + h].any() for h in range(nh)) for b in range(len(L))])
    raise AssertionError(mut)


def applies(name, arith, mut):
    if mut in ("skip_rescale", "unrounded_offset"):
        # the f16 offset and its move exist in AttWave64 only, and only behind block 0
        return arith == R.WAVE64 and name in ("lds", "heads3")
    if mut == "mask_gt":
        return arith != R.CLS             # attention_cls has no key image past the sentence to unmask
    return True


# (variant -1 runs the streaming arithmetic on the LDS batches too; its own batches cover it here)
MUTATED = [(n, a, m) for n, a in BATTERY if not (a == R.STREAM and n in ("lds", "heads3"))
           for m in R.MUTATIONS if applies(n, a, m)]


@pytest.mark.parametrize("name,arith,mut", MUTATED, ids=["%s-%s-%s" % c for c in MUTATED])
def test_bounds_reject_planted_mutations(faithful, name, arith, mut):
    """Each mutation of the restatement must leave, in every sentence it touches, an element
    outside a bound for at least one input kind (swapping two V rows, say, cannot show under
    uniform probabilities).  skip_rescale must show on the very input whose offset moved."""
    caught = None
    need = None
    for kind in kinds_of(name, arith):
        cs = R.case(name, kind)
        t = touched(cs, arith, mut, faithful(name, arith, kind)[1])
        if kind in ("latemax", "onehot"):     # these batches run the reversed order
            t = t[::-1]
        out, _ = R.restate(cs, arith, mut)
        hit = sentence_ratios(cs, arith, out) > 1.0
        if kind in ("latemax", "onehot"):
            hit = hit[::-1]
        if mut == "skip_rescale":
            hit = hit & t
        caught = hit if caught is None else caught | hit
        need = t if need is None else need | t
    lens = np.array(R.case(name, "random").lens)
    print("\n%s on %s-%s: rejected in %d of the %d sentences it touches" %
          (mut, name, arith, int((caught & need).sum()), int(need.sum())))
    assert need.any()
    assert (caught | ~need).all(), ("not rejected at lengths", lens[need & ~caught])


@pytest.mark.parametrize("name", ["lds", "heads3"])
def test_offset_moves_are_exercised(faithful, name):
    """A batch that claims the offset-move path has queries that move (in several blocks too)
    and queries that do not, per the restatement.  Counted per (query, head): lds latemax 8556 of
    8704 move (6522 in more than one block, 148 never), lds onehot 6654 (2084, 2050 never); heads3
    latemax 1277 of 1485 (703, 208 never), heads3 onehot 906 (186, 579 never)."""
    for kind in ("latemax", "onehot"):
        _, moves = faithful(name, R.WAVE64, kind)
        per_query = np.concatenate([m.sum(axis=1) for m in moves])
        n, some, many = len(per_query), int((per_query > 0).sum()), int((per_query > 1).sum())
        print("\n%s %s: %d of %d queries move the offset, %d of them in more than one block, %d never" %
              (name, kind, some, n, many, n - some))
        assert some >= 1 and n - some >= 1
        if kind == "latemax":
            assert many >= 1
    for kind in ("random", "uniform"):
        _, moves = faithful(name, R.WAVE64, kind)
        assert not any(m.any() for m in moves)          # the fixed-offset path alone


@pytest.mark.parametrize("name,arith", BATTERY, ids=IDS)
def test_planted_conditions_hold(name, arith):
    assert R.case(name, "uniform").uniform_exact()
    margin = R.case(name, "onehot").onehot_margin()
    print("\n%s: 1 - (smallest target probability) = %.3g" % (name, 1.0 - margin))
    assert margin >= 1.0 - 2.0 ** -20


def test_uniform_sums_are_exact_in_f32():
    """The builder's claim itself: f32 partial sums of a uniform V in two different orders equal
    the float64 sum."""
    cs = R.case("stream64", "uniform")
    for _, _, _, _, V in cs.items():
        want = V.astype(np.float64).sum(axis=0)
        fwd = np.zeros(V.shape[1], np.float32)
        for row in V.astype(np.float32):
            fwd = fwd + row
        assert np.array_equal(fwd.astype(np.float64), want)
        assert np.array_equal(V[::-1].astype(np.float32).sum(axis=0, dtype=np.float32).astype(np.float64), want)
