"""The numpy restatement of the residual codec (maxsim_res_refs.py) checked against itself:
what test_gpu_maxsim_res.py holds the device to must first be right on its own."""
from fractions import Fraction

import numpy as np
import pytest

import maxsim_refs as M
import maxsim_res_refs as RR


def case(w, nb, n=40, seed=0):
    """Twin rows v, their centroids c (both f16 values in f32) and a codec from the rule."""
    rng = np.random.default_rng(100 * w + nb + seed)
    cent = M.unit_rows(rng, 16, w).astype(np.float16).astype(np.float32)
    codes = rng.integers(0, 16, n)
    v = M.f16_view(cent[codes] + (0.4 / np.sqrt(w)) * rng.standard_normal((n, w)).astype(np.float32))
    v[3] = 0.0                                                             # a row stored as zeros
    c = cent[codes]
    cut, wts = RR.quantile_rule(v - c, nb)
    return v, c, cut, wts


@pytest.mark.parametrize("nb", (2, 4))
@pytest.mark.parametrize("w", (64, 192))
def test_loops_equal_the_vectorised_restatement(w, nb):
    v, c, cut, wts = case(w, nb)
    b, e, u = RR.encode(v, c, cut, wts)
    bl, el, ul = RR.encode_loops(v, c, cut, wts)
    assert np.array_equal(b, bl) and b.max() == (1 << nb) - 1 and b.min() == 0
    assert np.array_equal(e.view(np.uint16), el.view(np.uint16))
    assert np.array_equal(u.view(np.uint32), ul.view(np.uint32))
    assert np.all(np.abs(np.delete(u, 3) - 1.0) < 0.2)                    # a unit centroid plus a small residual
    # ties: a residual equal to a cutoff falls into the bucket below it
    r = (v - c).astype(np.float32)
    hit = r == cut[0]
    assert hit.any() and np.all(b[hit] == 0)
    # the canonical bytes round-trip, and element 1 sits above element 0 in byte 0
    bits = RR.pack_bits(b, nb)
    assert bits.shape == (len(v), w * nb // 8) and np.array_equal(RR.unpack_bits(bits, nb), b)
    assert np.all(bits[:, 0] & ((1 << nb) - 1) == b[:, 0]) and np.all((bits[:, 0] >> nb) & ((1 << nb) - 1) == b[:, 1])


def f16_round_exact(x):
    """A Fraction rounded once to f16, nearest even, subnormals kept (finite results only)."""
    if x == 0:
        return np.float16(0.0)
    sign, a = (-1 if x < 0 else 1), abs(x)
    ex = -14
    while a >= Fraction(2) ** (ex + 1):
        ex += 1
    step = Fraction(2) ** (ex - 10)                                        # subnormals: ex stays -14, step 2^-24
    q, rem = divmod(a, step)
    q = int(q)
    if rem * 2 > step or (rem * 2 == step and q % 2 == 1):
        q += 1
    return np.float16(sign * float(q * step))


def test_f16_addition_is_one_rounding():
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(3000) * np.exp2(rng.integers(-16, 3, 3000))).astype(np.float16)
    b = (rng.standard_normal(3000) * np.exp2(rng.integers(-16, 3, 3000))).astype(np.float16)
    edge = np.array([0x0001, 0x8001, 0x03ff, 0x0400, 0x0401, 0x3c00, 0x3c01, 0xbc01, 0x3bff, 0x13ff, 0x1400, 0x1001,
                     0x0000, 0x8000, 0x7bff, 0x2e66, 0xae66], np.uint16).view(np.float16)
    ea, eb = np.meshgrid(edge, edge)
    a, b = np.concatenate([a, ea.ravel()]), np.concatenate([b, eb.ravel()])
    with np.errstate(over="ignore"):
        got = a + b
    assert got.dtype == np.float16
    checked = 0
    for x, y, g in zip(a, b, got):
        exact = Fraction(float(x)) + Fraction(float(y))
        if abs(exact) >= 65520:
            continue                                                       # overflows: outside the contract
        want = f16_round_exact(exact)
        assert float(g) == float(want), (x, y, g, want)
        checked += 1
    assert checked > 3200


@pytest.mark.parametrize("w", (64, 768))
def test_sum_of_squares_is_exact_in_any_order(w):
    v, c, cut, wts = case(w, 4)
    _, e, u = RR.encode(v, c, cut, wts)
    e64 = e.astype(np.float64)
    for j in range(len(e)):
        fwd = rev = 0.0
        for x in e64[j]:
            fwd += x * x
        for x in e64[j][::-1]:
            rev += x * x
        exact = sum(Fraction(float(x)) ** 2 for x in e64[j])
        assert fwd == rev == float(exact) and Fraction(fwd) == exact and fwd < 32


def test_quantile_rule_on_a_hand_made_array():
    r = np.array([0.5, -0.25, 0.0, 0.75, -1.0, 0.25, 1.0, -0.5], np.float32)   # sorted: -1 -.5 -.25 0 .25 .5 .75 1
    cut, wts = RR.quantile_rule(r, 2)
    assert cut.tolist() == [-0.25, 0.25, 0.75]                             # sorted[2], [4], [6]
    assert wts.tolist() == [-0.5, 0.0, 0.5, 1.0]                           # sorted[1], [3], [5], [7]
    cut, wts = RR.quantile_rule(r, 4)
    assert cut.tolist() == [-1.0, -0.5, -0.5, -0.25, -0.25, 0.0, 0.0, 0.25, 0.25, 0.5, 0.5, 0.75, 0.75, 1.0, 1.0]
    assert wts.tolist() == [-1.0, -1.0, -0.5, -0.5, -0.25, -0.25, 0.0, 0.0, 0.25, 0.25, 0.5, 0.5, 0.75, 0.75, 1.0, 1.0]
    cut, wts = RR.quantile_rule(np.array([2.0], np.float32), 2)            # n = 1: every index clamps to n - 1
    assert cut.tolist() == [2.0] * 3 and wts.tolist() == [2.0] * 4
    assert RR.sample_stride(1) == 1 and RR.sample_stride(65536) == 1 and RR.sample_stride(65537) == 2
    rows = np.arange(12, dtype=np.float32).reshape(6, 2)
    cent = np.zeros((16, 2), np.float32)
    cut, wts = RR.train_buckets(rows, np.zeros(6, np.int64), cent, 2)      # stride 1: all 12 residuals
    assert cut.tolist() == [3.0, 6.0, 9.0] and wts.tolist() == [1.0, 4.0, 7.0, 10.0]


@pytest.mark.parametrize("sigma", (0.3, 0.6))
@pytest.mark.parametrize("w", (64, 128, 192))
def test_accuracy_ordering_of_the_reference(w, sigma):
    r4, r2, c0 = RR.accuracy_errors(w, sigma)
    assert 0 < r4 and 1.5 * r4 <= r2 and 1.5 * r2 <= c0, (r4, r2, c0)


def test_score_bound_is_the_f16_bound_plus_one_rounding():
    for Lq in M.QUERY_LENS:
        for w in M.WIDTHS:
            assert RR.score_tol(Lq, w) == M.score_tol(Lq, w) + Lq * 2.0 ** -24
    v, c, cut, wts = case(64, 2)
    _, e, u = RR.encode(v, c, cut, wts)
    q = v[:5]
    want = sum(max(float(np.dot(q[i].astype(np.float64), e[j].astype(np.float64))) * float(u[j]) for j in range(len(e)))
               for i in range(5))
    assert abs(RR.maxsim(q, e, u) - want) < 1e-12
