"""The denoiser's references held to one another (no GPU), on the inputs tests/denoise_cases.py makes for
tests/test_gpu_denoise_edges.py:

  * tests/denoise_ref.py (fp32, the kernel's order of operations) against tests/denoise_f64.py (the header's formulas in
    float64, written from include/srt_hip.h alone) on every parity case, the output and every level's record;
  * denoise_moments_ref.sample_variance against an evaluation in Python fractions with every IEEE rounding written out;
  * the region-isolation expectations (class colours where a boolean emulation reaches) against denoise_ref.py's bits;
  * the underflow rule (an exponential below 2^-126 counts as 0) in both references."""
from fractions import Fraction

import numpy as np
import pytest

import denoise_cases as K
import denoise_f64 as R64
import denoise_moments_ref as RM
import denoise_ref as R

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- fp32 reference against the float64 statement


@pytest.mark.parametrize("cid", K.parity_ids(), ids=lambda c: "%dx%d-sig%d-lv%d-mom%d" % c)
def test_fp32_reference_follows_float64_statement(cid):
    """D_ref, the fp32 reference's deviation from the statement, over the output (which bounds the kernel's output) and
    over every level's {e, v} (which bounds the kernel's records), is at most 5e-5 on every case: the condition under which
    four times D_ref bounds the kernel.  Measured maxima: 2.1e-5 on the output, 3.0e-5 on the records (both at sigmaNormal
    128).  The valid pixels of every level are the same in both references."""
    r = K.parity_refs(*cid)
    print("%s: D_ref output %.3g, records %.3g" % (cid, r["d_out"], r["d_rec"]))
    assert np.array_equal(r["out32"][..., 3], r["out64"][..., 3])
    assert np.array_equal(r["i32"]["hit"], r["i64"]["hit"])
    assert r["d_out"] <= K.D_REF_MAX and r["d_rec"] <= K.D_REF_MAX


@pytest.mark.parametrize("size", K.SIZES_B, ids=lambda s: "%dx%d" % s)
def test_fp32_guides_follow_float64_statement(size):
    """The prepare pass's records on the edge list: hits, normals, depths and the one-sided gradient with its tie rule
    read the same way by both references (the quantised depths are exact in float32, so a tie is a tie in both)."""
    c = K.prepare_case(*size)
    i32, i64 = {}, {}
    R.denoise(c["beauty"], c["normal"], c["depth"], iterations=1, intermediates=i32)
    R64.denoise(c["beauty"], c["normal"], c["depth"], iterations=1, intermediates=i64)
    assert np.array_equal(i32["hit"], i64["hit"]) and np.array_equal(i32["levels"][0][0], i64["levels"][0][0])
    assert np.abs(i32["n"] - i64["n"]).max() <= 2e-7
    assert np.abs(i32["z"] - i64["z"]).max() <= np.spacing(F(5))
    assert np.abs(i32["grad"] - i64["grad"]).max() <= 2 * np.spacing(F(5))
    z, hit = i64["z"], i64["hit"]
    if size[0] > 2:  # the tie is there, and taking the forward difference would show
        back, fwd = z[:, 1:-1] - z[:, :-2], z[:, 2:] - z[:, 1:-1]
        tie = hit[:, 1:-1] & hit[:, :-2] & hit[:, 2:] & (np.abs(back) == np.abs(fwd)) & (back != fwd)
        assert tie.sum() >= 2
        assert np.array_equal(i32["grad"][:, 1:-1, 0][tie], back[tie].astype(F))


# ---- the sample variance against fractions


def _rn(x, p, emin):
    """Fraction -> the nearest binary float of p significand bits and least exponent emin (ties to even), as a Fraction"""
    if x == 0:
        return Fraction(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = Fraction(2) ** max(e - p + 1, emin)
    k = a / q
    lo = k.numerator // k.denominator
    rem = k - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo & 1):
        lo += 1
    return (lo * q) if x > 0 else -(lo * q)


def _r64(x):
    return _rn(x, 53, -1074)


def _r32(x):
    return _rn(x, 24, -149)


def _exact_sample_variance(m, alb, demodulate):
    """one record by the header: NaN unless n >= 2 and S1, S2 finite; every operation rounded as the type it is done in"""
    s1, s2, n = float(m[0]), float(m[1]), float(m[3])
    if not (n >= 2 and np.isfinite(s1) and np.isfinite(s2)):
        return None
    s1, s2, n = Fraction(s1), Fraction(s2), Fraction(n)
    d = _r64(s2 - _r64(_r64(s1 * s1) / n))
    d = max(d, Fraction(0))
    v = _r32(_r64(d / _r64(n * _r64(n - 1))))
    if demodulate:
        div = []
        for k in range(3):
            mean = _r32(Fraction(float(alb[k])) / Fraction(float(alb[3]))) if alb[3] != 0 else Fraction(0)
            div.append(max(mean, Fraction(float(F(1e-3)))))
        co = [Fraction(float(F(c))) for c in (0.2126, 0.7152, 0.0722)]
        la = _r32(_r32(_r32(co[0] * div[0]) + _r32(co[1] * div[1])) + _r32(co[2] * div[2]))
        v = _r32(v / _r32(la * la))
    return v


@pytest.mark.parametrize("demodulate", [False, True])
def test_sample_variance_matches_fractions(demodulate):
    """Every record of the prepare cases (the edge list: n in {0, 1, 2, 3, 2^24}, S2 under, at and over S1^2 / n, NaN and inf
    sums; albedo at, under and over the clamp), to the last float."""
    seen = {"zero": 0, "unused": 0, "positive": 0}
    for size in K.SIZES_B:
        c = K.prepare_case(*size)
        got = RM.sample_variance(c["moments"], c["albedo"], demodulate)
        H, W = got.shape
        for y in range(H):
            for x in range(W):
                want = _exact_sample_variance(c["moments"][y, x], c["albedo"][y, x], demodulate)
                if want is None:
                    assert np.isnan(got[y, x]), (size, y, x)
                    seen["unused"] += 1
                else:
                    assert Fraction(float(got[y, x])) == want, (size, y, x, got[y, x], float(want))
                    seen["zero" if want == 0 else "positive"] += 1
    assert min(seen.values()) >= 8, seen


# ---- A's expectations are the fp32 reference's bits


@pytest.mark.parametrize("size", K.SIZES_A, ids=lambda s: "%dx%d" % s)
def test_region_expectations_are_reference_bits(size):
    W, H = size
    specials = [None] + (["all_miss", "all_invalid", "single_valid"] if size in ((17, 17), (50, 37), (1, 40)) else [])
    for special in specials:
        c = K.region_case(W, H, special)
        for levels in K.LEVELS_A:
            for demod in K.DEMOD_A:
                want, want_rgba, _ = K.region_expected(W, H, special, levels, demod)
                for mom in (False, True):
                    inter = {}
                    out, rgba = RM.denoise(c["beauty"], c["normal"], c["depth"], K.region_albedo(c, demod), iterations=levels,
                                           demodulate=demod != "off", moments=c["moments"] if mom else None, intermediates=inter)
                    label = (size, special, levels, demod, mom)
                    assert np.array_equal(_bits(out), _bits(want)), label
                    assert np.array_equal(rgba, want_rgba), label
                    if not mom:  # the spatial variance of a valid pixel among its own class is exactly 0
                        assert (inter["levels"][0][2][c["valid"]] == 0).all(), label


def test_region_cases_cover_what_they_claim():
    c = K.region_case(50, 37)
    lab = c["lab"]
    for e in K.EDGES_A:  # a class edge on each side of every listed row and column
        assert (lab[:, e] != lab[:, e - 1]).any() and (lab[e] != lab[e - 1]).any()
    assert set(np.unique(lab)) == {0, 1, 2, 3}
    frac = 1 - c["valid"].mean()
    assert 0.08 <= frac <= 0.2
    reached1, reached3 = (K.region_expected(50, 37, None, lv, "off")[2] for lv in (1, 3))
    assert (~reached1).sum() >= 1 and reached3.all()  # both outcomes of the emulation occur
    out, _, reached = K.region_expected(50, 37, "single_valid", 3, "off")
    assert 0 < reached.sum() < reached.size
    clamped = K.region_expected(50, 37, None, 1, "clamped")[0]
    assert (_bits(clamped[..., :3]) != _bits(K.region_expected(50, 37, None, 1, "dyadic")[0][..., :3])).any()


# ---- D: the underflow rule


@pytest.mark.parametrize("k", K.EXPONENTS_D)
def test_underflow_rule_in_both_references(k):
    """An exponential below 2^-126 counts as 0: the invalid centre is filled at 2^-66, 2^-120 and 2^-124 (there through
    denormal products with h) and stays invalid, output 0, at 2^-132 and 2^-152.  A valid centre comes back untouched."""
    sig = K.sigma_for_exponent(k)
    assert abs(sig * np.log2(K.DOT_D) - k) < 0.01
    for iterations in (1, 2):
        r = K.underflow_refs(False, k, iterations)
        for out, lv in ((r["out32"], r["i32"]["levels"]), (r["out64"], r["i64"]["levels"])):
            if k > -126:
                assert lv[1][0][4, 4]
                assert K.rel_rgb(out[4, 4, :3], K.CLASS_COLOUR[0].astype(np.float64)).max() <= K.FLOOR_C
            else:
                assert not lv[1][0][4, 4] and (out[4, 4, :3] == 0).all()
            others = np.ones((9, 9), bool)
            others[4, 4] = False
            assert np.array_equal(_bits(out[others][:, :3]), _bits(np.tile(K.CLASS_COLOUR[0], (80, 1))))
        r = K.underflow_refs(True, k, iterations)
        want = K.underflow_case(True)["beauty"][..., :3] / F(K.SPP)
        assert np.array_equal(_bits(r["out32"][..., :3]), _bits(want))
        assert np.array_equal(r["out64"][..., :3], want.astype(np.float64))
