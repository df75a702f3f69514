"""tests/chunk_sum_ref.py against independent routes, on the CPU: the reference the GPU tests of the exact chunk sum
(tests/test_gpu_chunk_sum.py) compare with must itself be right, and the directed double-rounding set must hit the case."""
from fractions import Fraction
import math

import numpy as np

import chunk_sum_ref as R

F = np.float32


def nearest_float32(x):
    """The float32 nearest the Fraction x, ties to even, by comparing the neighbouring floats exactly: no shifts, no
    remainders (round_once's route), only Fraction distances."""
    guess = F(float(x))  # within an ulp of the answer; possibly the wrong neighbour
    cands = {float(guess), float(np.nextafter(guess, F(-np.inf))), float(np.nextafter(guess, F(np.inf)))}
    best = min(abs(Fraction(c) - x) for c in cands)
    winners = [c for c in cands if abs(Fraction(c) - x) == best]
    if len(winners) > 1:
        winners = [c for c in winners if (int(F(c).view(np.uint32)) & 1) == 0]
    assert len(winners) == 1
    return F(winners[0])


def test_round_once_matches_the_nearest_neighbour_search():
    rng = np.random.default_rng(20)
    for bits in list(range(1, 63)) * 40:
        q = int(rng.integers(1 << (bits - 1), 1 << bits, dtype=np.uint64)) * (1 if rng.random() < 0.5 else -1)
        got, want = R.round_once(q), nearest_float32(Fraction(q, R.UNITS))
        assert got.view(np.uint32) == want.view(np.uint32), q
    # exact ties at every width that has any: q = (2m + 1) * 2^(s-1), both parities of m
    for s in range(1, 38):
        for m in (1 << 23, (1 << 23) + 1, (1 << 24) - 2, (1 << 24) - 1):
            q = (2 * m + 1) << (s - 1)
            want = math.ldexp(m + (m & 1), s - 36)
            assert float(R.round_once(q)) == want and float(R.round_once(-q)) == -want
            assert float(nearest_float32(Fraction(q, R.UNITS))) == want
    zero = R.round_once(0)
    assert zero == 0.0 and not np.signbit(zero)


def test_reference_matches_a_fraction_sum_on_random_slots():
    """Seeded random slots, mixed signs and magnitudes: the reference equals the Fraction sum of the truncated values
    rounded by the neighbour search.  The truncation itself is restated with floor division on the float's own
    numerator and denominator."""
    rng = np.random.default_rng(21)
    for chunks in (2, 3, 7, 64):
        lim = R.limit(chunks)
        mag = np.exp2(rng.uniform(-40.0, math.log2(lim), (300, chunks)))
        rows = (mag * rng.choice([-1.0, 1.0], mag.shape)).astype(F)
        rows = np.where(np.abs(rows) < F(lim), rows, np.nextafter(F(lim), F(0.0)))
        got = R.rows_sum(rows, chunks)
        for r, g in zip(rows, got):
            total = Fraction(0)
            for v in r:
                num, den = abs(Fraction(float(v))).as_integer_ratio()
                total += Fraction((num * R.UNITS) // den, R.UNITS) * (-1 if v < 0 else 1)
            want = nearest_float32(total) if total else F(0.0)
            assert g.view(np.uint32) == want.view(np.uint32), (chunks, r)


def test_flags_and_the_limit():
    lim = R.limit(3)
    assert lim == 2.0 ** 24 and R.limit(1) == 2.0 ** 26 and R.limit(64) == 2.0 ** 20 and R.limit(65) == 2.0 ** 19 and R.limit(640) == 2.0 ** 16
    below = float(np.nextafter(F(lim), F(0)))
    assert R.to_fixed(below, lim) == int(below) << 36
    assert R.to_fixed(lim, lim) == R.PINF and R.to_fixed(-lim, lim) == R.NINF
    assert R.to_fixed(np.nan, lim) == R.NAN and R.to_fixed(np.inf, lim) == R.PINF and R.to_fixed(-np.inf, lim) == R.NINF
    assert R.to_fixed(2.0 ** -36, lim) == 1 and R.to_fixed(-(2.0 ** -36), lim) == -1
    assert R.to_fixed(1.5 * 2.0 ** -36, lim) == 1 and R.to_fixed(2.0 ** -37, lim) == 0 and R.to_fixed(-0.0, lim) == 0
    assert np.isnan(R.channel_sum([lim, -lim, 1.0], lim)) and np.isnan(R.channel_sum([np.nan, 1.0, 1.0], lim))
    assert R.channel_sum([lim, 1.0, 1.0], lim) == np.inf and R.channel_sum([1.0, -3e38, 1.0], lim) == -np.inf
    z = R.channel_sum([-0.0, -0.0, -0.0], lim)
    assert z == 0.0 and not np.signbit(z)


def test_directed_rows_hit_the_double_rounding():
    """Every row of the directed set is one the conversion through double gets wrong, and the reference gets right (the
    wanted values come from the rows' construction).  The ties beside them are no such case: both routes agree there."""
    rows, want = R.double_rounding_rows()
    assert len(rows) == 8 * 2 * 2 * 6
    got, naive = R.rows_sum(rows, 3), R.naive_sum(rows, 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (naive.view(np.uint32) != want.view(np.uint32)).all()
    assert (np.abs(naive.view(np.uint32).astype(np.int64) - want.view(np.uint32).astype(np.int64)) == 1).all()  # by one ulp
    rows, want = R.tie_rows()
    assert np.array_equal(R.rows_sum(rows, 3).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(R.naive_sum(rows, 3).view(np.uint32), want.view(np.uint32))


def test_rounding_once_changes_no_sum_below_2_17():
    """fromFixed36's fix cannot move an image: below 2^17 (|q| < 2^53) the integer sum is exact in double, so the old
    expression rounded once as well.  Random and boundary integers: old expression == reference, bit for bit."""
    rng = np.random.default_rng(22)
    qs = [int(x) for x in rng.integers(-(1 << 53) + 1, 1 << 53, 20000)]
    qs += [int(x) for x in rng.integers(-(1 << 30), 1 << 30, 5000)]
    qs += [(1 << 53) - 1, -(1 << 53) + 1, 0, 1, -1, (1 << 24) + 1, (3 << 28) + 1]
    for q in qs:
        old = np.float32(np.float64(q) * 2.0 ** -36)
        assert old.view(np.uint32) == R.round_once(q).view(np.uint32), q
