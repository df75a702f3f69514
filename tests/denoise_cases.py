"""Caller-made inputs of the denoiser's edge tests, shared by tests/test_denoise_ref.py (CPU: the references against one
another) and tests/test_gpu_denoise_edges.py (the kernel).  Every builder is cached and returns read-only arrays.

    region_case    A: four classes (three hit classes with normals +x, +y, +z, one miss class), constant depth, dyadic
                   class colours and albedos: every tap's exponent is exactly 0 or -inf, so a pixel comes back as its
                   class colour on bits, and so does an invalid pixel some chain of taps reaches
    prepare_case   B: random planes with the edge list of the prepare pass
    parity_case    C: noisy planes for the comparison with the float64 statement
    underflow_case D: the 9x9 plane whose centre sees its neighbours through a weight of 2^-66 .. 2^-152"""
import functools

import numpy as np

import denoise_f64 as R64
import denoise_moments_ref as RM
import denoise_ref as R
import quantise_ref as Q

F = np.float32
SPP = 4


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _sums(mean, count):
    """(H, W, 3) means and an (H, W) count -> the (H, W, 4) float32 plane of sums with counts"""
    out = np.zeros(mean.shape[:2] + (4,), F)
    out[..., :3] = np.asarray(mean, F) * np.asarray(count, F)[..., None]
    out[..., 3] = count
    return out


# ------------------------------------------------------------------ A. region isolation

SIZES_A = [(1, 1), (1, 40), (40, 1), (15, 15), (16, 16), (17, 17), (33, 18), (50, 37)]  # width, height
LEVELS_A = (1, 3, 5, 8)
DEMOD_A = ("off", "dyadic", "clamped")
EDGES_A = (15, 16, 17, 31, 32, 33)  # class edges on, before and after the 16-pixel tile boundaries
MISS = 3
CLASS_NORMAL = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], F)
# (class 1's channels are dyadic numbers c with fl(fl(c / 1e-3f) * 1e-3f) != c: the clamped albedo shows in the output)
CLASS_COLOUR = np.array([[0.5, 1.5, 2.0], [2.625, 0.65625, 1.3125], [0.75, 1.0, 0.0625], [0.25, 0.5, 1.75]], F)
CLASS_ALBEDO = np.array([[0.5, 0.25, 1.0], [0.25, 0.5, 0.125], [1.0, 0.5, 0.25], [0.5, 0.5, 0.5]], F)  # colour / albedo is exact
CLAMPED_CLASS, CLAMPED_ALBEDO = 1, np.array([2.0 ** -11, 2.0 ** -11, 2.0 ** -10], F)  # every channel under 1e-3


def _labels(W, H, rng):
    """random blocks of 1-5 pixels, then one-pixel stripes on the rows and columns of EDGES_A"""
    lab = np.zeros((H, W), np.int64)
    y = 0
    while y < H:
        h, x = int(rng.integers(1, 6)), 0
        while x < W:
            w = int(rng.integers(1, 6))
            lab[y:y + h, x:x + w] = rng.integers(0, 4)
            x += w
        y += h
    base = lab.copy()
    for c in EDGES_A:
        if c < W:
            lab[:, c] = (base[:, 0] + c) % 4  # neighbouring stripes differ by one class
    for r in EDGES_A:
        if r < H:
            half = (np.arange(W) // 4) % 2 == 0
            lab[r, half] = ((base[0, :] + r) % 4)[half]
    return lab


def _region_planes(lab, invalid_kind, moments_seed):
    """planes of a label map.  invalid_kind: (H, W) ints, 0 valid, 1 a NaN channel, 2 an inf channel, 3 count 0."""
    H, W = lab.shape
    hit = lab != MISS
    cnt = np.full((H, W), SPP, F)
    beauty = _sums(CLASS_COLOUR[lab], cnt)
    ys, xs = np.nonzero(invalid_kind == 1)
    beauty[ys, xs, (ys + xs) % 3] = np.nan
    ys, xs = np.nonzero(invalid_kind == 2)
    beauty[ys, xs, (ys + 2 * xs) % 3] = np.where((ys + xs) % 2 == 0, np.inf, -np.inf)
    beauty[invalid_kind == 3, 3] = 0
    normal = _sums(CLASS_NORMAL[lab], np.where(hit, SPP, 0))
    depth = np.zeros((H, W, 4), F)
    depth[..., 0] = np.where(hit, 2.0 * SPP, 0)
    depth[..., 3] = np.where(hit, SPP, 0)
    rng = np.random.default_rng(moments_seed)
    n = F(8)
    s1 = rng.uniform(1.0, 4.0, (H, W)).astype(F) * n
    s2 = (s1 * s1 / n * rng.uniform(1.1, 2.0, (H, W)).astype(F)).astype(F)
    moments = np.stack([s1, s2, np.zeros_like(s1), np.full_like(s1, n)], -1)
    return dict(beauty=beauty, normal=normal, depth=depth, moments=moments)


def _reach(valid, lab, levels):
    """the boolean emulation: a pixel is valid after a level if a valid tap of its own class lies on the level's grid"""
    H, W = lab.shape
    for i in range(levels):
        s, new = 1 << i, np.zeros_like(valid)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                if y0 < y1 and x0 < x1:
                    q = valid[y0 + oy:y1 + oy, x0 + ox:x1 + ox] & (lab[y0 + oy:y1 + oy, x0 + ox:x1 + ox] == lab[y0:y1, x0:x1])
                    new[y0:y1, x0:x1] |= q
        valid = new
    return valid


@functools.lru_cache(maxsize=None)
def region_case(W, H, special=None):
    """special: None (the random label map with 15 % invalid pixels), "all_miss", "all_invalid", "single_valid".
    Returns dict(lab, valid, beauty, normal, depth, moments, albedo_dyadic, albedo_clamped)."""
    rng = np.random.default_rng(1000 * W + H)
    if special is None:
        lab = _labels(W, H, rng)
        kind = np.where(rng.random((H, W)) < 0.15, rng.integers(1, 4, (H, W)), 0)
        # the class whose albedo the clamp replaces keeps its pixels valid in every mode: its e = c / 1e-3f is no dyadic
        # number, so a FILLED pixel of it (sum w e / sum w) would come back within an ulp or two, not on bits
        kind[lab == CLAMPED_CLASS] = 0
    elif special == "all_miss":
        lab = np.full((H, W), MISS)
        kind = np.where(rng.random((H, W)) < 0.15, rng.integers(1, 4, (H, W)), 0)
    elif special == "all_invalid":
        lab = _labels(W, H, rng)
        kind = rng.integers(1, 4, (H, W))
    elif special == "single_valid":
        lab = np.zeros((H, W), np.int64)
        kind = rng.integers(1, 4, (H, W))
        kind[H // 2 + 1, W // 3] = 0
    else:
        raise ValueError(special)
    d = _region_planes(lab, kind, W + 7 * H)
    cnt = np.full((H, W), SPP, F)
    d.update(lab=lab, valid=kind == 0, albedo_dyadic=_sums(CLASS_ALBEDO[lab], cnt))
    alb = CLASS_ALBEDO.copy()
    alb[CLAMPED_CLASS] = CLAMPED_ALBEDO
    d["albedo_clamped"] = _sums(alb[lab], cnt)
    return _freeze(d)


def region_albedo(case, demod):
    return {"off": None, "dyadic": case["albedo_dyadic"], "clamped": case["albedo_clamped"]}[demod]


@functools.lru_cache(maxsize=None)
def region_expected(W, H, special, levels, demod):
    """(out (H, W, 4) float32, rgba (H, W, 4) uint8): the class colour where the emulation reaches, 0 elsewhere; w = the
    beauty count; the bytes by tests/quantise_ref.py.  Neither a moments plane nor the sigmas change it."""
    c = region_case(W, H, special)
    colour = CLASS_COLOUR.copy()
    if demod == "clamped":
        colour[CLAMPED_CLASS] = (colour[CLAMPED_CLASS] / R.ALBEDO_MIN).astype(F) * R.ALBEDO_MIN
    reached = _reach(c["valid"], c["lab"], levels)
    out = np.zeros((H, W, 4), F)
    out[..., :3] = np.where(reached[..., None], colour[c["lab"]], F(0))
    out[..., 3] = c["beauty"][..., 3]
    rgba = np.full((H, W, 4), 255, np.uint8)
    rgba[..., :3] = Q.levels(out[..., :3], 1)
    out.setflags(write=False)
    rgba.setflags(write=False)
    return out, rgba, reached


# ------------------------------------------------------------------ B. the prepare pass

SIZES_B = [(33, 18), (17, 17), (1, 40), (40, 1)]  # width, height
_NAN, _INF = F(np.nan), F(np.inf)


def _moment_edges():
    """{S1, S2, 0, n} records: n in {0, 1, 2, 3, 2^24}, S2 under, at and over S1^2 / n, NaN and inf sums"""
    out = []
    for n, s1 in ((2, 3.0), (3, 6.0), (2.0 ** 24, 2.0 ** 23), (3, 1.7), (2, 0.3), (2.0 ** 24, 1.0e7)):
        at = F(np.float64(F(s1)) ** 2 / n)
        for s2 in (np.nextafter(at, F(0)), at, np.nextafter(at, _INF), F(at * F(1.5)), F(at * F(0.5))):
            out.append((s1, s2, 0, n))
    for n in (0, 1, 1.5, -2, _NAN):
        out.append((5.0, 30.0, 0, n))
    for s1, s2 in ((_NAN, 4.0), (2.0, _NAN), (_INF, 4.0), (2.0, _INF), (-_INF, _INF)):
        out.append((s1, s2, 0, 4))
    return np.array(out, F)


@functools.lru_cache(maxsize=None)
def prepare_case(W, H):
    """Random planes with the edge list spread over them by a permutation of the pixels.  Depths are multiples of 0.25 in
    the upper half of the rows (or the left half of a one-row image), so equal backward and forward differences of
    opposite sign (the tie) are common."""
    rng = np.random.default_rng(77 * W + H)
    n = W * H
    cnt = rng.choice(np.array([1, 2, 4, 7], F), (H, W))
    beauty = _sums(rng.uniform(0.05, 3.0, (H, W, 3)), cnt)
    normal = _sums(rng.normal(0, 1, (H, W, 3)), cnt)
    z = rng.uniform(1.0, 5.0, (H, W))
    quant = np.zeros((H, W), bool)
    quant[:max(1, H // 2), :max(1, W // 2) if H == 1 else W] = True
    z = np.where(quant, 2.0 + 0.25 * rng.integers(0, 4, (H, W)), z)
    depth = _sums(np.repeat(z[..., None], 3, -1), cnt)
    depth[..., 1:3] = 0
    albedo = _sums(10.0 ** rng.uniform(-4, 0, (H, W, 3)), cnt)
    s1 = rng.uniform(0.5, 3.0, (H, W)).astype(F) * F(16)
    moments = np.stack([s1, (s1 * s1 / F(16) * rng.uniform(0.9, 1.5, (H, W))).astype(F), np.zeros_like(s1), np.full_like(s1, 16)], -1)
    order = iter(np.tile(rng.permutation(n), 8))
    at = lambda: divmod(int(next(order)), W)  # noqa: E731
    flat_hit = np.ones(n, bool)
    for k in range(max(3, n // 8)):  # misses: count 0, the sums left as they are; the depth plane likewise
        y, x = at()
        normal[y, x, 3] = 0
        depth[y, x, 3] = 0
        flat_hit[y * W + x] = False
    for k in range(4):  # a mean normal of length 0 (a hit all the same)
        y, x = at()
        normal[y, x, :3] = 0
    for edit in ((0, _NAN), (1, _INF), (2, -_INF), (3, F(0)), (0, _INF), (1, _NAN)) * 2:  # colour: channel / count
        y, x = at()
        beauty[y, x, edit[0]] = edit[1]
    one = F(1e-3)
    for ch, a in ((0, one), (1, np.nextafter(one, F(0))), (2, np.nextafter(one, F(1))), (0, F(0)), (1, F(-0.5))) * 2:
        y, x = at()
        c = F(4)
        albedo[y, x] = (0.5 * c, 0.25 * c, 0.75 * c, c)
        albedo[y, x, ch] = a * c  # exact: c is a power of two
    for k in range(3):  # albedo count 0: the mean is 0, the divisor the clamp
        y, x = at()
        albedo[y, x, 3] = 0
    for rec in _moment_edges():
        y, x = at()
        moments[y, x] = rec
    return _freeze(dict(beauty=beauty, normal=normal, depth=depth, albedo=albedo, moments=moments))


# ------------------------------------------------------------------ C. parity with the float64 statement

SIZES_C = [(17, 33), (40, 40)]  # width, height
SIGMAS_C = [(0.0, 0.0, 0.0), (0.3, 128.0, 1.0), (1e29, 0.01, 50.0)]  # luminance, normal, depth; 0 = default
LEVELS_C = [(1, False), (5, True), (8, True)]  # iterations, demodulate
D_REF_MAX = 5e-5   # the condition under which the fp32 reference may stand for the statement
FLOOR_C = 7.2e-6   # twice the 3.6e-6 measured on rendered frames
V_FLOOR = 1e-12


@functools.lru_cache(maxsize=None)
def parity_case(W, H):
    rng = np.random.default_rng(5 * W + H)
    yy, xx = np.mgrid[0:H, 0:W]
    cnt = np.full((H, W), 8, F)
    base = np.array([0.8, 0.5, 0.3]) * (1.0 + 0.5 * np.sin(xx / 5.0) * np.cos(yy / 7.0))[..., None]
    beauty = _sums(base * rng.uniform(0.5, 1.5, (H, W, 3)), cnt)
    nrm = np.array([0.0, 0.0, 1.0]) + rng.normal(0, 0.3, (H, W, 3))
    z = 2.0 + 0.05 * xx + 0.03 * yy + np.where(xx > W // 2, 1.5, 0.0)
    hit = rng.random((H, W)) >= 0.10
    normal = _sums(nrm, np.where(hit, 8, 0))
    depth = _sums(np.repeat(z[..., None], 3, -1), np.where(hit, 8, 0))
    depth[..., 1:3] = 0
    albedo = _sums(10.0 ** rng.uniform(-4, 0, (H, W, 3)), cnt)
    bad = rng.random((H, W)) < 0.05
    ys, xs = np.nonzero(bad)
    beauty[ys, xs, (ys + xs) % 3] = np.where((ys * 3 + xs) % 2 == 0, np.nan, np.inf)
    l = R.lum(beauty[..., :3] / F(8))
    s1 = np.where(np.isfinite(l), l, F(1)) * F(8)
    s2 = (s1 * s1 / F(8) * rng.uniform(1.01, 1.6, (H, W))).astype(F)
    moments = np.stack([s1.astype(F), s2, np.zeros((H, W), F), cnt], -1)
    moments[rng.random((H, W)) < 0.05, 3] = 1  # too few samples: the spatial estimate
    return _freeze(dict(beauty=beauty, normal=normal, depth=depth, albedo=albedo, moments=moments))


def parity_ids():
    return [(W, H, s, lv, m) for (W, H) in SIZES_C for s in range(len(SIGMAS_C)) for lv in range(len(LEVELS_C)) for m in (False, True)]


def rel_rgb(got, want):
    """test_gpu_denoise.py::_compare's metric: |got - want| / max(|want|, 1e-6) per channel"""
    return np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), 1e-6)


def rel_v(got, want):
    return np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), V_FLOOR)


def record_deviation(got_levels, want_levels, label=""):
    """The largest deviation of {e, v} records from the float64 statement's, over the levels given (None: not there) and
    the valid pixels; the valid masks must be equal.  e by rel_rgb, v by rel_v."""
    worst = 0.0
    for k, (got, want) in enumerate(zip(got_levels, want_levels)):
        if got is None:
            continue
        assert np.array_equal(got[0], want[0]), (label, "valid pixels differ after %d levels" % k)
        m = want[0]
        if m.any():
            worst = max(worst, float(rel_rgb(got[1], want[1])[m].max()), float(rel_v(got[2], want[2])[m].max()))
    return worst


def _both(planes, iterations, demodulate, sigmas, use_moments):
    kw = dict(iterations=iterations, demodulate=demodulate, sigma_l=sigmas[0], sigma_n=sigmas[1], sigma_z=sigmas[2])
    alb = planes.get("albedo") if demodulate else None
    i32, i64 = {}, {}
    out32, rgba32 = RM.denoise(planes["beauty"], planes["normal"], planes["depth"], alb,
                               moments=planes["moments"] if use_moments else None, intermediates=i32, **kw)
    out64 = R64.denoise(planes["beauty"], planes["normal"], planes["depth"], alb,
                        moments=planes["moments"] if use_moments else None, intermediates=i64, **kw)
    d_out = float(rel_rgb(out32[..., :3], out64[..., :3]).max())
    d_rec = record_deviation(i32["levels"], i64["levels"])
    return dict(out32=out32, rgba32=rgba32, i32=i32, out64=out64, i64=i64, d_out=d_out, d_rec=d_rec)


@functools.lru_cache(maxsize=None)
def parity_refs(W, H, s, lv, use_moments):
    """Both references on one case of C, with their intermediates, and the fp32 reference's deviation from the float64
    statement: d_out over the output's rgb (the D_ref the kernel's output is bounded by) and d_rec over every level's
    {e, v} record (the D_ref the kernel's records are bounded by: v = sum w^2 v / (sum w)^2 carries the weights' rounding
    twice and the level-0 variance is a difference of moments, so the records deviate more than the output does, 3.0e-5
    against 2.1e-5 at most)."""
    it, dm = LEVELS_C[lv]
    return _both(parity_case(W, H), it, dm, SIGMAS_C[s], use_moments)


def kernel_bound(d_ref):
    """The kernel against the float64 statement: four times the fp32 reference's own deviation (the kernel's exp, log
    and reciprocal are 1-ulp hardware operations where libm's are correctly rounded, and the reciprocal adds a rounding),
    and never under the floor."""
    return max(4.0 * d_ref, FLOOR_C)


# ------------------------------------------------------------------ D. underflowed weights

DOT_D = 0.6329
# log2 of the centre's normal weight.  The rule zeroes the last two; at -124 every product with h is a denormal (the
# largest, 36/256 2^-124, is 2^-126.8), so the fill there shows that the products keep them
EXPONENTS_D = (-66, -120, -124, -132, -152)


def sigma_for_exponent(k):
    return float(F(k / np.log2(DOT_D)))


@functools.lru_cache(maxsize=None)
def underflow_case(valid_centre):
    H = W = 9
    cnt = np.full((H, W), SPP, F)
    colour = np.tile(CLASS_COLOUR[0], (H, W, 1))
    nrm = np.tile(np.array([0.0, 1.0, 0.0]), (H, W, 1))
    nrm[4, 4] = (np.sqrt(1.0 - DOT_D ** 2), DOT_D, 0.0)
    if valid_centre:
        colour[4, 4] = (0.25, 0.75, 1.0)
    beauty = _sums(colour, cnt)
    if not valid_centre:
        beauty[4, 4, 1] = np.nan
    depth = np.zeros((H, W, 4), F)
    depth[..., 0] = 2.0 * SPP
    depth[..., 3] = SPP
    return _freeze(dict(beauty=beauty, normal=_sums(nrm, cnt), depth=depth))


@functools.lru_cache(maxsize=None)
def underflow_refs(valid_centre, k, iterations):
    return _both(underflow_case(valid_centre), iterations, False, (0.0, sigma_for_exponent(k), 0.0), False)
