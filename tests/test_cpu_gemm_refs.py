"""The GEMM tests' own references, checked without a GPU (gemm_refs.py): a numpy float32
restatement of the kernel's sum and epilogues meets every per-element bound in three internal
orders of the 32 products of a block (so the bounds are reachable), planted mutations of the
restatement are rejected by the bound or by the exact kinds (so they are tight enough to notice
them), the `integers` condition holds for every committed seed, and the numpy f16 restatement of
the GELU epilogue is measured against the era table over every finite f16 input.

The same mutations against the criterion of test_gpu_kernels.py (largest error <= 2e-3, GELU
3e-3, of the largest |reference| on inputs with its outlier channels; the residual statistics at
rtol 1e-4 / 2e-4), at that file's own shapes: it lets through `group_shift` (the row statistics
do not depend on which group a partial sits in) and `gelu_no_cubic` (an error of 0.035, under 3e-3
of a largest |reference| of 17.5 at N = K = 768; at its smallest shape the largest |reference| is
9.3 and it rejects it by 0.035 against 0.028) -- OLD_LETS_THROUGH, asserted below.  On the
negative side of the GELU (|gelu| <= 0.17) it sees no error below 16 % of the value.

The GELU restatement (correctly rounded exp2 and reciprocal) is at most GELU_STEPS_RESTATED = 15
f16 steps from the table where |T| >= 2^-13 (at x = -3.74; mean 0.5) and at most 6.2e-5 from it
below that: for -5.16 <= x <= -4.03 exp2 overflows f16 (z >= 16) and the result is -0 where the
table holds -6.2e-5 .. -2e-7.

Run with -s for the ratio tables."""
import numpy as np
import pytest

import gemm_refs as R

D, F, H = np.float64, np.float32, np.float16
SHAPE = dict(N=96, M=64)                       # one 64-row tile, a column tile and a half


LEGACY = dict(N=192, K=256, M=300)             # the smallest shape of test_gemm_matches_numpy


def inputs(form, fmt, K, kind, seed, legacy=False):
    """One small launch of an epilogue form: the operands as a dict.  legacy: the inputs of
    test_gpu_kernels.py (its outlier column, scaled row and channels) at its smallest shape."""
    rng = np.random.default_rng(seed)
    N, M = SHAPE["N"], SHAPE["M"]
    if legacy:
        N, K, M = LEGACY["N"], LEGACY["K"], LEGACY["M"]
    wkind = "legacy" if legacy else kind
    wt = R.random_weights(fmt, N, K, rng, wkind)
    bias = (rng.standard_normal(N) * 0.1).astype(F)
    c = dict(form=form, wt=wt, bias=bias)
    if form in ("plain0", "plain2", "gelu"):
        c["x"] = R.random_x(M, K, rng, wkind)
        c["res"] = rng.standard_normal((M, N)).astype(H) if form == "plain2" else None
    elif form == "inln":
        _, c["g"], c["be"], c["x"], c["stats"] = R.ln_stream(M, K, rng, legacy)
    else:
        c["x"] = R.random_x(M, K, rng, wkind)
        _, c["g"], c["be"], c["z"], c["stats"] = R.ln_stream(M, N, rng)
        c["gn"] = (1.0 + rng.standard_normal(N) * 0.3).astype(F)
        if legacy:
            c["bias"][11] += 60.0
            c["gn"][11] = 0.3
    return c


def reference(c):
    if c["form"] in ("plain0", "plain2"):
        return R.plain(c["wt"], c["x"], c["bias"], c["res"])
    if c["form"] == "inln":
        return R.input_ln(c["wt"], c["x"], c["stats"], c["g"], c["be"], c["bias"])
    return R.ResidualLn(c["wt"], c["x"], c["bias"], c["z"], c["stats"], c["g"], c["be"], c["gn"])


def restate(c, order="block", w=None, **mut):
    """The restated launch: out f16, and the partials for the residual form."""
    acc = R.chain_f32(c["wt"], c["x"], order, w)
    if c["form"] in ("plain0", "plain2"):
        return R.epi_plain(acc, mut.pop("bias", c["bias"]), c["res"])
    if c["form"] == "inln":
        return R.epi_input_ln(c["wt"], acc, c["stats"], c["g"], c["be"], c["bias"], **mut)
    return R.epi_residual_ln(acc, c["bias"], c["z"], c["stats"], c["g"], c["be"], c["gn"], **mut)


@pytest.mark.parametrize("fmt", sorted(R.FMTS))
@pytest.mark.parametrize("form", ["plain0", "plain2", "inln", "resln"])
def test_restatement_meets_every_bound(fmt, form):
    worst = {}
    for K in (64, 448):
        for order in R.ORDERS:
            for i, kind in enumerate(R.KINDS):
                c = inputs(form, fmt, K, kind, 100 * fmt + K + i)
                ref = reference(c)
                got = restate(c, order)
                if form == "resln":
                    out, part = got
                    ratio = R.worst_ratio(out, ref.ref, ref.bound)
                    ps = R.worst_ratio(part[:, :, 0], ref.s, ref.s_bound)
                    pq = R.worst_ratio(part[:, :, 1], ref.q, ref.q_bound)
                    st, sb = ref.stats()
                    pst = R.worst_ratio(R.ln_row_stats_f32(part, SHAPE["N"]), st, sb)
                    worst[("partials", K)] = max(worst.get(("partials", K), 0.0), ps, pq)
                    worst[("stats", K)] = max(worst.get(("stats", K), 0.0), pst)
                else:
                    ratio = R.worst_ratio(got, *ref)
                worst[(order, K)] = max(worst.get((order, K), 0.0), ratio)
    print("\nworst error / bound, restated %-5s %-6s: " % (R.FMTS[fmt], form) +
          "  ".join("%s/%d %.3f" % (k[0], k[1], v) for k, v in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst
    # reachable: if no order came near the bound at one K-step, n_epi would be to recount
    assert max(worst[(o, 64)] for o in R.ORDERS) >= 0.3, worst


# ---------------------------------------------------------------- planted mutations

def old_ok(got, ref, factor=2e-3):
    """test_gpu_kernels.py's criterion: the largest error against a share of the largest |ref|."""
    return np.abs(np.asarray(got, D) - ref).max() <= factor * np.abs(ref).max()


def old_stats_ok(part, y2):
    st = R.ln_row_stats_f32(part, y2.shape[1])
    m2, r2 = R.ln_stats64(y2)
    return bool(np.allclose(st[:, 0], m2, rtol=1e-4, atol=1e-5 * np.abs(y2).max()) and
                np.allclose(st[:, 1], r2, rtol=2e-4))


def mutate_weights(name, wt):
    """The weights a mutated kernel would multiply, [N][Ke]."""
    w = wt.w.copy()
    if name == "drop_k":
        w[:, 37] = 0.0
    elif name == "double_k":
        w[:, 37] *= 2.0
    elif name == "swap_features":               # two elements of a block, between features 20 and 21
        w[[20, 21], 37] = w[[21, 20], 37]
    elif name == "swap_blocks":                 # blocks 2 ks and 2 ks + 1 of the first K-step
        w[:, :64] = np.concatenate([w[:, 32:64], w[:, :32]], axis=1)
    elif name == "neighbour_scale":             # the block scale of feature n - 1
        wq, wd, wm = R.parse_blocks(wt.fmt, wt.wb, wt.N, wt.K)
        w = R.Weights(wt.fmt, R.build_blocks(wt.fmt, wq, np.roll(wd, 1, axis=0), wm), wt.N, wt.K).w
    return w


WEIGHT_MUTATIONS = ("drop_k", "double_k", "swap_features", "swap_blocks", "neighbour_scale")


def weight_mutation(name):
    """(rejected by the new criteria, passed by the old one), q4_0 at one K-step."""
    fmt, K = 2, 64
    c = inputs("plain0", fmt, K, "random", 7)
    new = R.worst_ratio(restate(c, w=mutate_weights(name, c["wt"])), *reference(c)) > 1.0
    # the exact kinds: integers (bit for bit) and one-hot decode
    wt, x, bias, _, want = R.integer_case(fmt, SHAPE["N"], K, SHAPE["M"], 11)
    ci = dict(form="plain0", wt=wt, x=x, bias=bias, res=None)
    assert np.array_equal(restate(ci).view(np.uint16), want.astype(H).view(np.uint16))
    exact = not np.array_equal(restate(ci, w=mutate_weights(name, wt)).view(np.uint16), want.astype(H).view(np.uint16))
    co = dict(form="plain0", wt=c["wt"], x=R.onehot_x(K), bias=np.zeros(SHAPE["N"], F), res=None)
    want1 = c["wt"].w[:, R.onehot_map(K)].T.astype(H)
    assert np.array_equal(restate(co).view(np.uint16), want1.view(np.uint16))
    onehot = not np.array_equal(restate(co, w=mutate_weights(name, c["wt"])).view(np.uint16), want1.view(np.uint16))
    lg = inputs("plain0", fmt, K, "random", 7, legacy=True)
    old = old_ok(restate(lg, w=mutate_weights(name, lg["wt"])), reference(lg)[0])
    return (new or exact or onehot), old, dict(bound=new, integers=exact, onehot=onehot)


def epilogue_mutation(name):
    K = 64
    if name == "bias_shift":                    # the bias of column n + 8
        c, lg = (inputs("plain0", 2, K, "random", 8, legacy=l) for l in (False, True))
        new = R.worst_ratio(restate(c, bias=np.roll(c["bias"], 8)), *reference(c)) > 1.0
        old = old_ok(restate(lg, bias=np.roll(lg["bias"], 8)), reference(lg)[0])
        return new, old, {}
    if name == "neighbour_stats":               # st0 c1 with the statistics of row m + 1
        rows = lambda c: np.roll(np.arange(len(c["x"])), -1)
        c, lg = (inputs("inln", 2, K, "random", 9, legacy=l) for l in (False, True))
        new = R.worst_ratio(restate(c, stats_rows=rows(c)), *reference(c)) > 1.0
        old = old_ok(restate(lg, stats_rows=rows(lg)), reference(lg)[0])
        return new, old, {}
    mut = {"no_beta": dict(beta=False), "gnext_before_partials": dict(gnext_first=True),
           "group_shift": dict(group_shift=1)}[name]
    c, lg = (inputs("resln", 2, K, "random", 10, legacy=l) for l in (False, True))
    ref = reference(c)
    out, part = restate(c, **mut)
    how = dict(out=R.worst_ratio(out, ref.ref, ref.bound) > 1.0,
               partials=max(R.worst_ratio(part[:, :, 0], ref.s, ref.s_bound),
                            R.worst_ratio(part[:, :, 1], ref.q, ref.q_bound)) > 1.0)
    lref = reference(lg)
    lout, lpart = restate(lg, **mut)
    old = old_ok(lout, lref.ref) and old_stats_ok(lpart, lref.y2)
    return any(how.values()), old, how


def gelu_mutation(name):
    mut = {"gelu_no_cubic": dict(cubic=False), "gelu_flush_negative": dict(flush_negative=True)}[name]
    steps, small = R.gelu_distance(R.gelu_restated(R.FINITE16, **mut), R.FINITE16)
    new = steps > R.GELU_STEPS_DEVICE or small > R.GELU_FLOOR
    # the old criterion, 3e-3 of the largest |tanh-form GELU| on its inputs with outliers: the
    # plain epilogue, and the input-LN form whose outlier channels raise the largest |reference|
    def tanh_form(v):
        x16 = v.astype(H).astype(D)
        return 0.5 * x16 * (1 + np.tanh(0.7978845608028654 * x16 * (1 + 0.044715 * x16 * x16)))
    old = {}
    lg = inputs("gelu", 2, 64, "random", 12, legacy=True)
    acc = R.chain_f32(lg["wt"], lg["x"], "block")
    ref = tanh_form(R.plain_f32(lg["wt"], lg["x"], lg["bias"])[0])
    assert old_ok(R.epi_plain(acc, lg["bias"], gelu=True), ref, 3e-3)
    old["plain"] = bool(old_ok(R.epi_plain(acc, lg["bias"], gelu=True, **mut), ref, 3e-3))
    # ... and at (N, K, M) = (768, 768, 512) of the same test, where the outlier column times the
    # scaled row gives a larger |reference| (the accumulator as the rounded float64 sum: its
    # error is far below this tolerance)
    rng = np.random.default_rng(14)
    wt, x = R.random_weights(2, 768, 768, rng, "legacy"), R.random_x(512, 768, rng, "legacy")
    bias = (rng.standard_normal(768) * 0.1).astype(F)
    ref = tanh_form(R.plain_f32(wt, x, bias)[0])
    acc = R.acc_terms(wt, x)[0].astype(F)
    assert old_ok(R.epi_plain(acc, bias, gelu=True), ref, 3e-3)
    old["plain_768"] = bool(old_ok(R.epi_plain(acc, bias, gelu=True, **mut), ref, 3e-3))
    return new, any(old.values()), dict(steps=steps, below_floor=small, old=old, largest_ref=float(np.abs(ref).max()))


MUTATIONS = WEIGHT_MUTATIONS + ("bias_shift", "neighbour_stats", "no_beta", "gnext_before_partials", "group_shift",
                                "gelu_no_cubic", "gelu_flush_negative")
OLD_LETS_THROUGH = {"group_shift", "gelu_no_cubic"}


@pytest.mark.parametrize("name", MUTATIONS)
def test_planted_mutation_is_rejected(name):
    fn = weight_mutation if name in WEIGHT_MUTATIONS else gelu_mutation if name.startswith("gelu") else epilogue_mutation
    new, old, how = fn(name)
    print("\n%-22s new criteria reject: %s %s; old criterion passes it: %s" % (name, new, how, old))
    assert new, (name, how)
    assert old == (name in OLD_LETS_THROUGH), (name, old)


# ---------------------------------------------------------------- the exact kinds' conditions

@pytest.mark.parametrize("fmt", sorted(R.FMTS))
def test_integer_condition_holds_for_every_seed(fmt):
    low = 1.0
    for cfg, rows, N, K, res, seed in R.integer_battery(fmt):
        share = R.integer_condition(*R.integer_case(fmt, N, K, rows, seed, res))
        low = min(low, share)
        assert share >= 0.99, (cfg, rows, K, res, share)
    print("\n%s: lowest share of |want| < 512 over the battery %.4f" % (R.FMTS[fmt], low))


def test_onehot_map_is_a_permutation():
    for K in (64, 256):
        assert np.array_equal(np.sort(R.onehot_map(K)), np.arange(K))


# ---------------------------------------------------------------- GELU

def test_gelu_restatement_against_the_era_table():
    steps, small = R.gelu_distance(R.gelu_restated(R.FINITE16), R.FINITE16)
    print("\ngelu restated over %d finite f16 inputs: worst %d steps where |T| >= 2^-13, worst |error| %.3g below"
          % (len(R.FINITE16), steps, small))
    assert steps == R.GELU_STEPS_RESTATED
    assert small <= R.GELU_FLOOR
    # the launch that feeds the epilogue every normal f16 value
    W, X, acc = R.gelu_input_launch()
    assert len(np.unique(acc[:60].view(np.uint16))) == 60 * 1024
