"""The denoiser (csrc/srt_denoise.hip) pass by pass on caller-made planes (tests/denoise_cases.py), its scratch read back
through srtTestDenoiseScratch (include/srt_hip_test.h):

  A  region isolation, no tolerance: every pixel comes back as its class colour on bits, an invalid pixel too where a
     boolean emulation of the taps reaches it; sizes under, at and over a tile, class edges on the tile boundaries
  B  the prepare pass on bits against the fp32 reference: guide, gradient (ties, borders, one-pixel-wide images), the first
     colour record, the sample variance
  C  parity with the float64 statement of the header (tests/denoise_f64.py): the output and the per-level {e, v} records
     within max(4 D_ref, 7.2e-6), D_ref the fp32 reference's own deviation in the same quantity (tests/test_denoise_ref.py)
  D  the underflow rule: an exponential below 2^-126 counts as 0

Every run is made twice, with the levels read through the caches (denoise_lds_step 0) and staged in LDS (8); output, bytes
and scratch records of the two must be equal on bits."""

import numpy as np
import pytest

import denoise_cases as K
import denoise_moments_ref as RM

pytestmark = pytest.mark.gpu

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    """equal on bits, NaNs equal by position"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (_bits(a) == _bits(b))))


def _once(ctx, d, dev_planes, moments, W, H):
    import torch
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.denoise(d, W, H, dev_planes[0].data_ptr(), [t.data_ptr() if t is not None else None for t in dev_planes[1:]],
                out.data_ptr(), rgba.data_ptr(), None, d_moments_ptr=moments.data_ptr() if moments is not None else None)
    torch.cuda.synchronize()
    guide, col0, col1, grad = ctx.denoise_scratch(W, H)
    return dict(out=out.cpu().numpy(), rgba=rgba.cpu().numpy(), guide=guide, grad=grad, col=(col0, col1))


def _denoise(ctx, abi, planes, iterations, albedo=None, moments=None, sigmas=(0.0, 0.0, 0.0)):
    """One denoise of NumPy planes in both forms of the level kernel; returns the (identical) results of one.  The colour
    buffer the run did not write (the other one after a single level) is left out of the comparison."""
    import torch
    up = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda() if a is not None else None  # noqa: E731  (a copy: the cases are read-only)
    H, W = planes["beauty"].shape[:2]
    dev_planes = [up(planes["beauty"]), up(albedo), up(planes["normal"]), None, up(planes["depth"])]
    d = abi.default_denoise_params(iterations, 1 if albedo is not None else 0, *sigmas)
    saved = ctx.get_tunable("denoise_lds_step")
    try:
        runs = []
        for step in (0, 8):
            ctx.set_tunable("denoise_lds_step", step)
            runs.append(_once(ctx, d, dev_planes, up(moments), W, H))
    finally:
        ctx.set_tunable("denoise_lds_step", saved)
    a, b = runs
    k = iterations - 1
    assert np.array_equal(_bits(a["out"]), _bits(b["out"])) and np.array_equal(a["rgba"], b["rgba"])
    assert np.array_equal(_bits(a["guide"]), _bits(b["guide"])) and np.array_equal(_bits(a["grad"]), _bits(b["grad"]))
    assert np.array_equal(_bits(a["col"][k & 1]), _bits(b["col"][k & 1]))
    if k >= 1:
        assert np.array_equal(_bits(a["col"][(k - 1) & 1]), _bits(b["col"][(k - 1) & 1]))
    a["iterations"] = iterations
    return a


def _record(col):
    """a colour record as the references keep it: (valid, e with 0 where not valid, v)"""
    valid = ~np.isnan(col[..., 0])
    return valid, np.where(valid[..., None], col[..., :3], F(0)), col[..., 3]


def _levels(res):
    """levels[k] = the record after k levels where the scratch still holds it (k = iterations - 1 and the one before), else
    None"""
    k = res["iterations"] - 1
    out = [None] * (k + 1)
    out[k] = _record(res["col"][k & 1])
    if k >= 1:
        out[k - 1] = _record(res["col"][(k - 1) & 1])
    return out


# ------------------------------------------------------------------ A


def _specials(size):
    return [None] + (["all_miss", "all_invalid", "single_valid"] if size in ((17, 17), (50, 37), (1, 40)) else [])


@pytest.mark.parametrize("size", K.SIZES_A, ids=lambda s: "%dx%d" % s)
def test_regions_come_back_on_bits(ctx, abi, size):
    """1, 3, 5 and 8 levels (steps 64 and 128 reach past every image), demodulation off, by dyadic albedos and with one
    class's albedo under the clamp, with and without a moments plane; then an all-miss image, an all-invalid one (output 0)
    and a single valid pixel in an invalid field.  A mis-indexed tap, halo cell or ping-pong buffer leaks a foreign colour."""
    W, H = size
    for special in _specials(size):
        c = K.region_case(W, H, special)
        for levels in K.LEVELS_A:
            for demod in K.DEMOD_A:
                want, want_rgba, reached = K.region_expected(W, H, special, levels, demod)
                for mom in (False, True):
                    label = (size, special, levels, demod, mom)
                    res = _denoise(ctx, abi, c, levels, K.region_albedo(c, demod), c["moments"] if mom else None)
                    bad = np.argwhere((_bits(res["out"]) != _bits(want)).any(-1))
                    assert len(bad) == 0, (label, len(bad), bad[:4].tolist(), res["out"][tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
                    assert np.array_equal(res["rgba"], want_rgba), label
                    rec = _levels(res)[levels - 1]
                    if levels == 1:
                        assert np.array_equal(rec[0], c["valid"]), label
                        if not mom:  # the spatial variance of a valid pixel among its own class is exactly 0
                            assert (rec[2][c["valid"]] == 0).all(), label
                    else:
                        assert np.array_equal(rec[0], K.region_expected(W, H, special, levels - 1, demod)[2]), label
        if special == "all_invalid":
            assert not reached.any() and (want[..., :3] == 0).all()


# ------------------------------------------------------------------ B


@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulated"])
@pytest.mark.parametrize("size", K.SIZES_B, ids=lambda s: "%dx%d" % s)
def test_prepare_pass_on_bits(ctx, abi, size, demodulate):
    """Everything the prepare pass writes that is +, *, / and sqrt: the guide {n, z}, the gradient, e of col[0] and the
    sample variance, against the fp32 reference with NaN by position.  (The spatial variance goes through exp2: test C.)"""
    W, H = size
    c = K.prepare_case(W, H)
    alb = c["albedo"] if demodulate else None
    res = _denoise(ctx, abi, c, 1, alb, c["moments"])
    ref = {}
    RM.denoise(c["beauty"], c["normal"], c["depth"], alb, iterations=1, demodulate=demodulate, moments=c["moments"], intermediates=ref)
    hit = ~np.isnan(res["guide"][..., 3])
    assert np.array_equal(hit, ref["hit"])
    assert np.array_equal(_bits(res["guide"][..., :3]), _bits(ref["n"]))
    assert np.array_equal(_bits(res["guide"][..., 3][hit]), _bits(ref["z"][hit]))
    bad = np.argwhere((_bits(res["grad"]) != _bits(ref["grad"])).any(-1))
    assert len(bad) == 0, (len(bad), bad[:4].tolist())
    valid, e, v = _record(res["col"][0])
    rvalid, re, rv = ref["levels"][0]
    assert np.array_equal(valid, rvalid)
    assert np.isnan(res["col"][0][..., :3][~valid]).all()
    assert np.array_equal(_bits(e[valid]), _bits(re[valid]))
    sv = RM.sample_variance(c["moments"], alb, demodulate)
    use = ~np.isnan(sv)
    assert use.sum() >= 30 and (~use).sum() >= 8
    assert _same(v[use], sv[use]) and _same(v[use], rv[use])
    assert (v[~use] >= 0).all()
    # the run with no moments plane: the same records but for v
    res0 = _denoise(ctx, abi, c, 1, alb, None)
    assert np.array_equal(_bits(res0["guide"]), _bits(res["guide"])) and np.array_equal(_bits(res0["grad"]), _bits(res["grad"]))
    assert np.array_equal(_bits(res0["col"][0][..., :3]), _bits(res["col"][0][..., :3]))
    assert np.array_equal(_bits(res0["col"][0][..., 3][~use]), _bits(v[~use]))


# ------------------------------------------------------------------ C


@pytest.mark.parametrize("cid", K.parity_ids(), ids=lambda c: "%dx%d-sig%d-lv%d-mom%d" % c)
def test_parity_with_float64_statement(ctx, abi, cid):
    """Output rgb and the {e, v} records the scratch still holds (after iterations - 1 levels and the level before) against
    the float64 statement, each within max(4 D_ref, 7.2e-6) with the fp32 reference's D_ref of the same quantity.  Measured
    on an MI355X: output 2.1e-5 at most (4.8e-6 with the default sigmas), records 3.0e-5 (1.1e-5), always
    within 1.3 D_ref."""
    W, H, s, lv, mom = cid
    it, dm = K.LEVELS_C[lv]
    c = K.parity_case(W, H)
    r = K.parity_refs(*cid)
    res = _denoise(ctx, abi, c, it, c["albedo"] if dm else None, c["moments"] if mom else None, K.SIGMAS_C[s])
    bound, rec_bound = K.kernel_bound(r["d_out"]), K.kernel_bound(r["d_rec"])
    assert bound <= 2e-4 and rec_bound <= 2e-4
    rel = K.rel_rgb(res["out"][..., :3], r["out64"][..., :3])
    rec = K.record_deviation(_levels(res), r["i64"]["levels"], cid)
    print("parity %s: output %.3g (D_ref %.3g, bound %.3g), records %.3g (D_ref %.3g, bound %.3g)" % (
        cid, rel.max(), r["d_out"], bound, rec, r["d_rec"], rec_bound))
    assert np.isfinite(res["out"]).all()
    assert np.array_equal(res["out"][..., 3], r["out64"][..., 3].astype(F))
    assert rel.max() <= bound, (cid, rel.max(), bound, np.unravel_index(rel.argmax(), rel.shape))
    assert rec <= rec_bound, (cid, rec, rec_bound)
    assert np.abs(res["rgba"].astype(int) - r["rgba32"].astype(int)).max() <= 1


# ------------------------------------------------------------------ D


@pytest.mark.parametrize("k", K.EXPONENTS_D)
def test_underflowed_weights(ctx, abi, k):
    """The invalid centre of the 9x9 plane sees its neighbours through 2^k.  Above 2^-126 it is filled (at 2^-124 through
    nothing but denormal products with h); below, the exponential counts as 0: the pixel is exactly 0 and stays invalid.  A valid
    centre comes back untouched either way."""
    sig = (0.0, K.sigma_for_exponent(k), 0.0)
    others = np.ones((9, 9), bool)
    others[4, 4] = False
    for iterations in (1, 2):
        c, r = K.underflow_case(False), K.underflow_refs(False, k, iterations)
        res = _denoise(ctx, abi, c, iterations, sigmas=sig)
        centre = res["out"][4, 4, :3]
        print("underflow 2^%d, %d levels: centre %s" % (k, iterations, centre.tolist()))
        if k > -126:
            assert K.rel_rgb(centre, r["out64"][4, 4, :3]).max() <= K.kernel_bound(r["d_out"])
        else:
            assert (_bits(centre) == 0).all() and (res["rgba"][4, 4, :3] == 0).all()
        if iterations == 2:  # col[1]: after the first level
            assert _record(res["col"][1])[0][4, 4] == (k > -126)
        assert np.array_equal(_bits(res["out"][others][:, :3]), _bits(np.tile(K.CLASS_COLOUR[0], (80, 1))))
        c = K.underflow_case(True)
        res = _denoise(ctx, abi, c, iterations, sigmas=sig)
        assert np.array_equal(_bits(res["out"][..., :3]), _bits(c["beauty"][..., :3] / F(K.SPP)))


# ------------------------------------------------------------------ the hook itself


def test_scratch_hook_reads_and_refuses(ctx, dev, abi):
    c = K.region_case(17, 17)
    res = _denoise(ctx, abi, c, 3)
    again = ctx.denoise_scratch(17, 17)  # nothing launched, nothing changed
    assert np.array_equal(_bits(again[0]), _bits(res["guide"])) and np.array_equal(_bits(again[3]), _bits(res["grad"]))
    assert np.array_equal(_bits(again[1]), _bits(res["col"][0])) and np.array_equal(_bits(again[2]), _bits(res["col"][1]))
    assert dev.lib.srtTestDenoiseScratch(ctx.h, 17, 17, None, None, None, None) == 0  # every buffer may be NULL
    with pytest.raises(dev.SrtError, match="size"):
        ctx.denoise_scratch(0, 17)
    fresh = dev.Context(0)
    try:
        with pytest.raises(dev.SrtError, match="scratch holds 0 bytes"):
            fresh.denoise_scratch(4, 4)
    finally:
        fresh.close()
