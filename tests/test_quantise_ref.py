"""tests/quantise_ref.py on the CPU: the exact statement of the 8-bit quantisation against independent routes, the three
host-side copies of color.h:25-41 (the oracle's writeColorTarget, adaptive_ref.resolve, progressive.image_rgba8) against it
byte for byte on the inputs the GPU test uses (tests/test_gpu_quantise.py), and what those inputs reach."""
from fractions import Fraction
import importlib

import numpy as np
import pytest

import adaptive_ref
import quantise_ref as Q

F = np.float32
W, H, case = Q.W, Q.H, Q.case


def test_sqrt_rn_is_the_nearest_float32():
    """isqrt route against exact Fraction comparisons of the squared neighbours: g is nearest iff m lies between the squares
    of the midpoints to g's neighbours."""
    rng = np.random.default_rng(5)
    ms = np.concatenate([np.exp2(rng.uniform(-149, 128, 3000)).astype(F), rng.uniform(0, 1.1, 3000).astype(F),
                         np.array([Q.step(Q.boundary(L), d) for L in range(1, 256) for d in (-2, -1, 0, 1, 2)], F)])
    ms = ms[np.isfinite(ms) & (ms > 0)]
    for m in ms:
        g = F(Q.sqrt_rn(m))
        assert float(g) == Q.sqrt_rn(m)
        lo, hi = np.nextafter(g, F(0)), np.nextafter(g, F(np.inf))
        mid_lo, mid_hi = (Fraction(float(lo)) + Fraction(float(g))) / 2, (Fraction(float(g)) + Fraction(float(hi))) / 2
        assert mid_lo ** 2 < Fraction(float(m)) < mid_hi ** 2, m
    with np.errstate(all="ignore"):
        assert np.array_equal(np.sqrt(ms), np.array([Q.sqrt_rn(m) for m in ms], F))  # and numpy's float32 root is that root


def test_levels_at_the_boundaries():
    """The mean (L/256)^2 is the first of level L by its exact root.  For the 127 levels whose L/256 has a mantissa in
    (1, sqrt 2) the float one ulp BELOW it still resolves to L: its root lies within half an ulp of L/256 and the
    correctly rounded sqrtf returns L/256 (quantise_ref.one_below_holds); that is what an approximate square root gets
    wrong.  For the other levels one ulp below is L - 1, and two ulps below is L - 1 for all."""
    for L in range(1, 256):
        b = Q.boundary(L)
        assert float(b) * 65536.0 == L * L
        assert Q.level_of_mean(b) == L and Q.level_of_mean(Q.step(b, 1)) == L and Q.level_of_mean(Q.step(b, 2)) == L
        below = Q.step(b, -1)
        assert Fraction(float(below)) < Fraction(L, 256) ** 2
        if Q.one_below_holds(L):
            assert Q.level_of_mean(below) == L and Fraction(Q.sqrt_rn(below)) == Fraction(L, 256), L
        else:
            assert Q.level_of_mean(below) == L - 1 and Fraction(Q.sqrt_rn(below)) < Fraction(L, 256), L
        assert Q.level_of_mean(Q.step(b, -2)) == L - 1, L
    top = F(0.999) * F(0.999)
    for m, want in ((top, 255), (F(1.0), 255), (np.finfo(F).max, 255), (F(np.inf), 255), (F(-np.inf), 0), (F(np.nan), 0), (F(-0.0), 0),
                    (F(0.0), 0), (F(-1e-30), 0), (np.nextafter(F(0), F(1)), 0), (F(255.0 / 256.0) ** 2, 255), (Q.step(F(255.0 / 256.0) ** 2, -2), 254)):
        assert Q.level_of_mean(m) == want, m


# Sums near the level boundaries where dividing by spp lands on another level than multiplying by fl32(1 / spp)
# (quantise_ref.divide_differs: 25 neighbouring sums per boundary).  Powers of two have none: both are exact.
DIVIDE_DIFFERS = {3: 57, 5: 102, 7: 83, 1000: 167, 5000: 37}


@pytest.mark.parametrize("spp", Q.SPPS)
def test_inputs_reach_what_they_are_for(spp):
    acc, want, info = case(spp)
    hits = info["hits"]
    # most boundary means are reached by some sum exactly, at every offset; one ulp below a boundary still gives L
    for d in (-2, -1, 0, 1, 2):
        assert sum((L, d) in hits for L in range(1, 256)) >= 100, (spp, d)
    assert sum((L, -1) in hits and Q.one_below_holds(L) for L in range(1, 256)) >= 50, spp
    for (L, d), c in hits.items():
        assert Q.levels(np.array([c], F), spp)[0] == (L if d >= 0 or (d == -1 and Q.one_below_holds(L)) else L - 1), (spp, L, d)
    if spp & (spp - 1):
        assert info["divide_differs"] == DIVIDE_DIFFERS[spp] and info["divide_differs"] >= 1
    lv = want[..., :3]
    assert set(np.unique(lv)) == set(range(256))  # every level appears
    nan = np.isnan(acc[..., :3])
    assert (nan.sum(axis=-1) == 1).sum() >= 6 and (nan.sum(axis=-1) <= 1).all()  # a NaN channel beside two good ones
    assert (lv[nan] == 0).all()


@pytest.mark.parametrize("spp", Q.SPPS)
def test_host_copies_give_the_exact_bytes(spp, oracle, srt):
    """oracle.resolve (writeColorTarget restated in C++), adaptive_ref.resolve (the count in w) and
    progressive.image_rgba8, on the GPU test's inputs: the exact reference's bytes."""
    acc, want, _ = case(spp)
    assert np.array_equal(oracle.resolve(np.array(acc), spp), want)
    assert np.array_equal(adaptive_ref.resolve(np.array(acc)), want)
    pr = importlib.import_module(srt.__name__ + ".progressive").ProgressiveRender(None, None, W, H, 1)
    pr.accum, pr.next_sample = np.array(acc), spp
    with np.errstate(all="ignore"):
        assert np.array_equal(pr.image_rgba8(), want)
