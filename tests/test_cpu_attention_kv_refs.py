"""The key-count attention tests' own references, checked without a GPU (attention_kv_refs.py):
the restatements of the kernels, run on the counted keys, meet every bound on every batch and
kind the GPU file uses; the planted builders' conditions hold with counts; a kernel that ignored
the counts (the unmasked reference) would be far outside the bounds on every batch; and the
two planted mutations at the count's edge (the last counted key dropped, the first excluded key
let in) are rejected.

Run with -s for the ratio tables."""
import numpy as np
import pytest

import attention_kv_refs as KV
import attention_refs as R

# (batch, arithmetic) as test_gpu_attention_kv.py runs them; ("lds", STREAM) is variant -1
BATTERY = [("short", R.WAVE64), ("lds", R.WAVE64), ("heads3", R.WAVE64), ("heads3_short", R.WAVE64),
           ("lds32", R.LDS32), ("stream64", R.STREAM), ("stream32", R.STREAM), ("lds", R.STREAM),
           ("lds32", R.STREAM), ("heads3", R.STREAM)]
IDS = ["%s-%s" % b for b in BATTERY]
# the kinds on which excluded keys carry weight (onehot gives them P < 2^-20 by construction)
LEAK_KINDS = ("random", "latemax", "uniform")


def ratios(cs, arith, out):
    """Per sentence: the worst |out - want| / bound over the general bound and a planted one."""
    pairs = [(cs.ref, cs.bound(arith))]
    if cs.kind in ("uniform", "onehot"):
        pairs.append(cs.planted_bound(arith))
    return np.array([max(R.worst_ratio(out[r], want[r], bd[r]) for want, bd in pairs)
                     for r in (slice(int(cs.cu[b]), int(cs.cu[b + 1])) for b in range(len(cs.lens)))])


@pytest.fixture(scope="module")
def faithful():
    cache = {}

    def get(name, arith, kind):
        key = (name, arith, kind)
        if key not in cache:
            cache[key] = KV.restate(KV.case(name, kind), arith)[0]
        return cache[key]
    return get


@pytest.mark.parametrize("name,arith", BATTERY, ids=IDS)
def test_restatements_meet_every_bound(faithful, name, arith):
    worst = {kind: ratios(KV.case(name, kind), arith, faithful(name, arith, kind)).max() for kind in R.KINDS}
    print("\nworst error / bound with key counts, restatement %-7s on %-12s: " % (arith, name) +
          "  ".join("%s %.3f" % kv for kv in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("name", sorted(KV.BATCHES))
def test_planted_conditions_hold(name):
    assert KV.case(name, "uniform").uniform_exact()
    cs = KV.case(name, "onehot")
    # every target is a counted key of its own sentence
    for b in range(len(cs.lens)):
        t = cs.target[int(cs.cu[b]):int(cs.cu[b + 1])] - int(cs.cu[b])
        assert t.min() >= 0 and t.max() < cs.keys[b]
    margin = cs.onehot_margin()
    print("\n%s: 1 - (smallest target probability) = %.3g" % (name, 1.0 - margin))
    assert margin >= 1.0 - 2.0 ** -20


@pytest.mark.parametrize("name", sorted(KV.BATCHES))
def test_uniform_reference_is_the_mean_of_the_counted_rows(name):
    cs = KV.case(name, "uniform")
    v = cs.qkv[:, 2 * cs.d:].astype(np.float64)
    for b in range(len(cs.lens)):
        s, nk = int(cs.cu[b]), int(cs.keys[b])
        mean = v[s:s + nk].mean(axis=0)
        assert np.abs(cs.ref[s:int(cs.cu[b + 1])] - mean[None, :]).max() <= 2.0 ** -40


@pytest.mark.parametrize("name,arith", BATTERY, ids=IDS)
def test_unmasked_reference_is_far_outside_the_bound(name, arith):
    """What a kernel that ignored the counts would return lies more than 100 bounds from the
    reference on every batch, on each kind that weighs the excluded keys; under uniform, whose
    excluded V rows are 512, in every sentence that has an excluded key (one random key of 512,
    as in (512, 511), weighs about 1 / 512 and is 31 bounds away)."""
    for kind in LEAK_KINDS:
        cs = KV.case(name, kind)
        r = ratios(cs, arith, KV.unmasked_reference(cs))
        cut = cs.keys < np.array(cs.lens)
        print("\n%s-%s %s: unmasked reference / bound, per sentence with excluded keys: %s" %
              (name, arith, kind, " ".join("%.3g" % x for x in r[cut])))
        assert cut.any() and r[cut].max() > 100.0 and (r[cut] > 1.0).all(), (kind, r)
        assert kind != "uniform" or (r[cut] > 100.0).all(), (kind, r)


MUTATED = [(n, a, m) for n, a in BATTERY if not (a == R.STREAM and n in ("lds", "lds32", "heads3")) for m in KV.KV_MUTATIONS]


@pytest.mark.parametrize("name,arith,mut", MUTATED, ids=["%s-%s-%s" % c for c in MUTATED])
def test_bounds_reject_mutations_at_the_count(name, arith, mut):
    """drop_last masks the last counted key, mask_gt lets key `keys` in: each leaves, in every
    sentence it touches, an element outside a bound for at least one input kind."""
    caught = need = None
    for kind in R.KINDS:
        cs = KV.case(name, kind)
        L, K = np.array(cs.lens), cs.keys
        # mask_gt: a real row behind the count (keys < len); else attention_refs' own condition
        t = L >= 1 if mut == "drop_last" else (K < L) | ((K % 64 != 0) & ((K > 1) | (arith == R.STREAM)))
        hit = ratios(cs, arith, KV.restate(cs, arith, mut)[0]) > 1.0
        if kind in ("latemax", "onehot"):
            t, hit = t[::-1], hit[::-1]
        caught = hit if caught is None else caught | hit
        need = t if need is None else need | t
    pairs = KV.BATCHES[name][0]
    print("\n%s on %s-%s: rejected in %d of the %d sentences it touches" %
          (mut, name, arith, int((caught & need).sum()), int(need.sum())))
    assert need.any()
    assert (caught | ~need).all(), ("not rejected at", [p for p, n, c in zip(pairs, need, caught) if n and not c])


@pytest.mark.parametrize("name", ["short", "lds", "heads3", "heads3_short"])
def test_some_kind_moves_no_offset(name):
    """The GPU file compares the wave64 kernels with the truncated batch on the kinds where no
    offset moves in either run; there must be such kinds (uniform is one: every score is 0)."""
    still = [k for k in R.KINDS if not KV.wave64_moves(name, k)]
    print("\n%s: no offset move with counts or truncated on: %s" % (name, ", ".join(still)))
    assert "uniform" in still and len(still) >= 2
