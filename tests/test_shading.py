"""The shading step, call by call, at its edges: shade(), texValue / texLeaf, checkerOdd and the slot decoding of the
shading record (csrc/srt_path.h), through srtScatterRaysForm in all four instances the render kernels run (WIDE x COUNT),
on caller-made hit records.

One "shading bench" scene holds every material; only the materials matter, the hit records are written here.  Four groups:
(a) the checker's choice at points on and around its boundaries, (b) imagePNG::value's texel index at every rounding edge
of u * width, with the 1- and 2-byte images' read past their last texel, (c) dielectric and metal at normal, critical and
grazing incidence, (d) pbr with normal maps and metalness / roughness textures.  Every group goes through all four forms,
whose outputs must be bit-identical, and is compared with the oracle under the same keys; (a) and (b) are also compared
with tests/shade_ref.py (mpmath, NumPy), to which the tests not marked gpu hold the oracle."""
import numpy as np
import pytest

import shade_ref as R

gpu = pytest.mark.gpu
f32 = np.float32
FORMS = (0, 1, 2, 3)  # bit 0 WIDE, bit 1 COUNT
SEED = 20240611
ATT_TOL = dict(rtol=2e-6, atol=1e-9)  # test_scatter_known_answers' tolerance of an attenuation (exp2 is its only libm call)
EVEN, ODD = (0.9, 0.5, 0.25), (0.1, 0.5, 0.75)  # red above green in the even colour, below it in the odd one


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_same_floats(got, want, what):
    """Equal bit for bit, NaNs in the same places (a NaN's own bits are the platform's)."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(-1) & ~nan.reshape(-1))
    assert len(bad) == 0, (what, len(bad), bad[:4], got.reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]])


# ---------------------------------------------------------------- the scene
SMALL_IMAGES = (("rgb6x4", 6, 4, 3), ("rgba9x5", 9, 5, 4), ("one1x1", 1, 1, 3))
# 1- and 2-byte images followed by a 3-byte image whose first bytes are not zero; byte counts 35 and 30 (the device's dword
# alignment puts zeros behind them) and 32 and 24 (it does not)
FOLLOWED_IMAGES = (("g7x5_mid", 7, 5, 1), ("ga5x3_mid", 5, 3, 2), ("g8x4_mid", 8, 4, 1), ("ga4x3_mid", 4, 3, 2))
WIDE_IMAGES = (("wide32767", 32767, 1, 4),   # the widest packed slot
               ("wide40000", 40000, 1, 3))   # too wide to pack: the generic path
LAST_IMAGES = {1: ("g7x5_last", 7, 5, 1), 2: ("ga5x3_last", 5, 3, 2)}
NORMAL_TEXELS = {"n_zero": (128, 128, 128), "n_000": (0, 0, 0), "n_255": (255, 255, 255), "n_up": (128, 128, 255)}


class Bench:
    """The scene (abi.SceneBuilder), its images by name (pixels as loaded, None = a failed load) and materials by name."""

    def __init__(self, abi, last_bpp):
        self.sb = sb = abi.SceneBuilder()
        self.pixels, self.tex, self.mat = {}, {}, {}
        rng = np.random.default_rng(5)

        def image(name, w, h, bpp, pixels=None):
            if pixels is None:
                pixels = rng.integers(1, 256, (h, w, bpp), dtype=np.uint8)  # no zero byte anywhere: an overrun shows
            self.pixels[name] = pixels
            self.tex[name] = sb.image(pixels, bpp)

        for spec in SMALL_IMAGES:
            image(*spec)
        for k, spec in enumerate(FOLLOWED_IMAGES):
            image(*spec)
            image("follow%d" % k, 2, 2, 3)
        for spec in WIDE_IMAGES:
            image(*spec)
        self.pixels["failed"] = None
        self.tex["failed"] = sb.image(None, 3)
        for name, texel in NORMAL_TEXELS.items():
            image(name, 1, 1, 3, np.array(texel, np.uint8).reshape(1, 1, 3))
        image("t0", 1, 1, 3, np.zeros((1, 1, 3), np.uint8))
        image("t255", 1, 1, 3, np.full((1, 1, 3), 255, np.uint8))
        image("warm2x2", 2, 2, 3, np.array([[[230, 128, 7], [200, 100, 9]], [[255, 150, 1], [210, 140, 3]]], np.uint8))
        image(*LAST_IMAGES[last_bpp])  # the last texture of the texel buffer
        self.texel_images = [s[0] for s in SMALL_IMAGES + FOLLOWED_IMAGES + WIDE_IMAGES] + ["failed", LAST_IMAGES[last_bpp][0]]
        self.overrun_images = [s[0] for s in FOLLOWED_IMAGES] + [LAST_IMAGES[last_bpp][0]]

        m = self.mat
        # (a) the three ways a checker reaches shade()
        solids = sb.checker(EVEN, ODD)
        m["checker_light"] = sb.light(emit_tex=solids)              # texValue
        m["checker_solids"] = sb.pbr(albedo_tex=solids, roughness=0.5)  # SRT_SLOT_CHECKER2: colours in the record
        odd = sb.solid(*ODD)
        sb.textures.append(abi.SrtTextureIn(kind=abi.SRT_TEX_CHECKER, even=self.tex["warm2x2"], odd=odd))
        m["checker_image"] = sb.pbr(albedo_tex=len(sb.textures) - 1, roughness=0.5)  # slotValue -> texValue
        # (b) every image as a light's emit texture and in each pbr slot
        for name in self.texel_images:
            t = self.tex[name]
            m["light:" + name] = sb.light(emit_tex=t)
            for slot in ("albedo", "normal", "metallic", "roughness"):
                m[slot + ":" + name] = sb.pbr(albedo=(0.8, 0.7, 0.6, 1.0), metalness=0.3, roughness=0.6, **{slot + "_tex": t})
        # (c)
        for ir in (1.5, 2.4, 1.0, 0.5):
            m["glass%g" % ir] = sb.dielectric(ir)
        for fuzz in (0.0, 0.2, 1.0):
            m["metal%g" % fuzz] = sb.metal((0.8, 0.6, 0.4), fuzz)
        # (d)
        for n in NORMAL_TEXELS:
            for mt in ("t0", "t255"):
                for rg in ("t0", "t255"):
                    m["pbr:%s:%s:%s" % (n, mt, rg)] = sb.pbr(albedo_tex=self.tex["rgb6x4"], normal_tex=self.tex[n],
                                                            metallic_tex=self.tex[mt], roughness_tex=self.tex[rg],
                                                            albedo=(0.9, 0.8, 0.7, 1.0))
        m["smooth"] = sb.pbr(albedo=(0.9, 0.8, 0.7, 1.0), metalness=0.5, roughness=0.0)
        m["smooth_tex"] = sb.pbr(albedo=(0.9, 0.8, 0.7, 1.0), metalness=0.5, roughness=0.7, roughness_tex=self.tex["t0"])
        for i in range(len(sb.materials)):
            sb.add_sphere((3.0 * i, 0.0, 0.0), 1.0, i)
        sb.world_bvh()
        self.abi = abi

    def hits(self, material, n, p=(0.05, 0.4, 0.05), uv=(0.5, 0.5), normal=(0, 1, 0), tangent=(1, 0, 0), bitangent=(0, 0, 1),
             front=1, d=(0.3, -1.0, 0.2)):
        """n caller-made (ray, hit record) pairs; every argument is one value or one per entry."""
        rays, hits = np.zeros(n, self.abi.RAY_DTYPE), np.zeros(n, self.abi.HIT_DTYPE)
        rays["o"], rays["d"], rays["tMin"], rays["tMax"] = (0.0, 5.0, 0.0), d, 0.001, np.inf
        hits["t"], hits["p"], hits["uv"], hits["frontFace"] = 1.0, p, uv, front
        hits["normal"], hits["tangent"], hits["bitangent"] = normal, tangent, bitangent
        hits["material"] = self.mat[material] if isinstance(material, str) else material
        return rays, hits


def cat(parts):
    return np.concatenate([r for r, _ in parts]), np.concatenate([h for _, h in parts])


def count(parts):
    return sum(len(r) for r, _ in parts)


_benches = {}


def bench_for(abi, oracle, last_bpp=1):
    """One bench and its oracle scene per variant (the image that ends the texel buffer), built once."""
    if last_bpp not in _benches:
        b = Bench(abi, last_bpp)
        _benches[last_bpp] = (b, oracle.OracleScene(b.sb))
    return _benches[last_bpp]


def run_forms(ctx, rays, hits, what):
    """The four forms on the uploaded scene: bit-identical outputs; the COUNT forms agree on the fetch counter and the
    others leave it 0.  Returns (form 0's out13, the counter)."""
    outs = [ctx.scatter_test_form(rays, hits, SEED, form) for form in FORMS]
    for form in FORMS[1:]:
        assert_same_floats(outs[form][0], outs[0][0], (what, "form", form))
    assert not outs[0][1].any() and not outs[1][1].any(), what
    assert np.array_equal(outs[2][1], outs[3][1]), what
    assert_same_floats(ctx.scatter_test(rays, hits, SEED), outs[0][0], (what, "srtScatterRays"))
    return outs[0][0], outs[2][1]


def assert_matches_oracle(bench, hits, got, want, what, att_bits=False):
    """out13 against the oracle's: scatter's bool and the emitted colour on bits; direction, origin and attenuation of
    every material that makes a scattered ray (diffuseLight::scatter returns false without touching its outputs, which
    the reference leaves uninitialised): direction and origin on bits, the attenuation on bits too where no libm call is
    involved, else within ATT_TOL (NaNs in the same places)."""
    assert np.array_equal(got[:, 9], want[:, 9]), what
    assert_same_floats(got[:, 10:13], want[:, 10:13], (what, "emitted"))
    light = np.array([m.type == bench.abi.SRT_MAT_LIGHT for m in bench.sb.materials])[hits["material"]]
    assert not want[light, 9].any(), what
    got, want = got[~light], want[~light]
    assert_same_floats(got[:, 3:6], want[:, 3:6], (what, "direction"))
    assert_same_floats(got[:, 6:9], want[:, 6:9], (what, "origin"))
    if att_bits:
        assert_same_floats(got[:, 0:3], want[:, 0:3], (what, "attenuation"))
    else:
        np.testing.assert_allclose(got[:, 0:3], want[:, 0:3], err_msg=str(what), **ATT_TOL)


class Case:
    """A group's hit records with the oracle's answer, computed once and shared by the tests of the group."""

    def __init__(self, bench, osc, parts):
        self.bench, self.osc = bench, osc
        self.rays, self.hits = cat(parts)
        self.want, self.want_fetches = osc.scatter_many(self.rays, self.hits, SEED)

    def of(self, material):
        return self.hits["material"] == self.bench.mat[material]


# ---------------------------------------------------------------- (a) checker parity
CHECKER_MATERIALS = ("checker_light", "checker_solids", "checker_image")


@pytest.fixture(scope="module")
def checker_case(abi, oracle):
    bench, osc = bench_for(abi, oracle)
    points = np.concatenate([R.checker_points(R.checker_coordinates()), R.underflow_points()])
    case = Case(bench, osc, [bench.hits(m, len(points), p=points) for m in CHECKER_MATERIALS])
    case.points, case.odd = points, R.checker_truth(points)
    assert 0.3 < case.odd.mean() < 0.7  # both parities are reached
    return case


def check_checker_choice(case, out, fetches, who):
    """The child every one of the three materials picked, read off `out` without libm or RNG, against mpmath's sign."""
    odd = case.odd
    colour = (np.where(odd[:, None], np.array(ODD, f32), np.array(EVEN, f32)) * f32(255.0)).astype(f32)
    assert_same_floats(out[case.of("checker_light")][:, 10:13], colour, (who, "checker_light"))
    for name in ("checker_solids", "checker_image"):
        att = out[case.of(name)][:, 0:3]
        lit = att[:, 1] > 0  # (a scatter direction perpendicular to the normal leaves nothing to compare)
        assert lit.mean() > 0.99, (who, name)
        # F0 is grey (metalness 0): the specular term is the same in every channel, and the diffuse one follows the albedo
        picked_odd = att[:, 0] < att[:, 1]
        bad = np.flatnonzero((picked_odd != odd) & lit)
        assert len(bad) == 0, (who, name, len(bad), case.points[bad[:4]])
    if fetches is not None:  # checker(image, solid): the even child is the one image lookup
        assert np.array_equal(fetches[case.of("checker_image")], (~odd).astype(np.uint32)), who
        assert not fetches[~case.of("checker_image")].any(), who


def test_pi_periods_replay_vs_mpmath():
    """The float32 replay of piPeriods (shade_ref.pi_periods) on +-40 ulps around k * pi for k up to and past 2^22, and on
    uniform arguments: no accepted argument has the wrong parity, and the smallest |sin| among the accepted ones stays above
    the 3e-6 checkerOdd's comment claims (3.15e-6 over 1.6e8 arguments when the test was written)."""
    import mpmath
    rng = np.random.default_rng(3)
    ks = np.unique(np.concatenate([np.arange(0, 151), R.CHECKER_K, rng.integers(151, 1 << 22, 150),
                                   (1 << 22) + np.arange(-2, 3)]))
    with mpmath.workprec(128):
        centres = [f32(float(mpmath.pi * int(k))) for k in ks]
    a = np.concatenate([R.ulp_neighbours(s * c, R.ULP_SPAN) for c in centres for s in (f32(1), f32(-1))]
                       + [rng.uniform(-1.3e7, 1.3e7, 20000).astype(f32)])
    ok, periods, _ = R.pi_periods(a)
    sin = R.sines(a)
    assert 0.5 < ok.mean() < 1.0 and (~ok[np.abs(a) > 1.32e7]).all() and not ok[a == 0].any()
    wrong = np.flatnonzero(ok & ((periods & 1).astype(bool) != (sin < 0)))
    assert len(wrong) == 0, (len(wrong), a[wrong[:4]])
    assert np.abs(sin[ok]).min() >= 3e-6, np.abs(sin[ok]).min()


def test_checker_oracle_vs_mpmath(checker_case):
    """Group (a) on the CPU: the oracle's sinf product picks the child mpmath's sign names at every point, and the replay
    of the kernel's fast path agrees wherever it decides."""
    check_checker_choice(checker_case, checker_case.want, checker_case.want_fetches, "oracle")
    odd, decided = R.checker_replay(checker_case.points)
    assert decided.mean() > 0.9 and not decided.all()  # the fallback is exercised too
    assert np.array_equal(odd[decided], checker_case.odd[decided])


@gpu
def test_checker_choice(ctx, checker_case):
    """Group (a): every point of shade_ref.checker_points, and those of underflow_points, through the three materials.
    (What no output shows: a change that only turns arguments piPeriods accepts into fallbacks -- its `below` and `above`
    swapped, say -- since sinf then gives the same answer; 10 500 of these points are accepted through `below`.)"""
    ctx.upload_scene(checker_case.bench.sb)
    out, fetches = run_forms(ctx, checker_case.rays, checker_case.hits, "checker")
    check_checker_choice(checker_case, out, fetches, "device")
    assert_matches_oracle(checker_case.bench, checker_case.hits, out, checker_case.want, "checker")
    assert np.array_equal(fetches, checker_case.want_fetches)


# ---------------------------------------------------------------- (b) texel indexing
SLOTS = ("light", "albedo", "normal", "metallic", "roughness")


def texel_parts(bench, name, us, vs):
    uv = np.stack([np.asarray(us, f32), np.asarray(vs, f32)], axis=-1)
    return [bench.hits("%s:%s" % (slot, name), len(uv), uv=uv) for slot in SLOTS]


def grid(us, vs):
    uu, vv = np.meshgrid(us, vs, indexing="ij")
    return uu.reshape(-1), vv.reshape(-1)


def texel_case(bench, osc, names, wide):
    parts = []
    for name in names:
        px = bench.pixels[name]
        h, w = (4, 6) if px is None else px.shape[:2]  # a failed load: any coordinates
        if wide:  # every i / width at one v, and the coordinates that depend on no size against every v
            us, vs = R.uv_coordinates(w), np.full(len(R.uv_coordinates(w)), 0.25, f32)
            parts += texel_parts(bench, name, us, vs)
            us, vs = grid(R.uv_coordinates(1), R.uv_coordinates(h))
        else:
            us, vs = grid(R.uv_coordinates(w), R.uv_coordinates(h))
        parts += texel_parts(bench, name, us, vs)
    return Case(bench, osc, parts)


def check_texels(case, names, out, fetches, who):
    """Lights: the emitted colour is the texel shade_ref names, on bits.  The fetch counter is the number of loaded images
    the material looks up: one per hit, none for a failed load."""
    for name in names:
        px = case.bench.pixels[name]
        m = case.of("light:" + name)
        want = R.texel_lookup(px, case.hits["uv"][m, 0], case.hits["uv"][m, 1])
        assert_same_floats(out[m][:, 10:13], want, (who, name))
        if fetches is not None:
            for slot in SLOTS:
                got = fetches[case.of("%s:%s" % (slot, name))]
                assert len(got) and (got == (0 if px is None else 1)).all(), (who, slot, name)


@pytest.fixture(scope="module")
def small_texel_case(abi, oracle):
    bench, osc = bench_for(abi, oracle)
    names = [n for n in bench.texel_images if not n.startswith("wide")]
    return names, texel_case(bench, osc, names, wide=False)


@pytest.fixture(scope="module")
def wide_texel_case(abi, oracle):
    bench, osc = bench_for(abi, oracle)
    names = [s[0] for s in WIDE_IMAGES]
    return names, texel_case(bench, osc, names, wide=True)


@pytest.fixture(scope="module")
def last_2bpp_case(abi, oracle):
    bench, osc = bench_for(abi, oracle, last_bpp=2)  # the variant whose texel buffer ends with the 2-byte image
    return bench.overrun_images, texel_case(bench, osc, bench.overrun_images, wide=False)


def test_texel_oracle_vs_numpy(small_texel_case, wide_texel_case, last_2bpp_case):
    """Group (b) on the CPU: the oracle's imagePNG::value against shade_ref.texel_lookup.  The overrun cases are the ones
    that failed before the 1-bpp overrun was defined as 0 past the end of the IMAGE: with "the end" the end of the caller's
    texel buffer, light:g7x5_mid at u = 1, v = 0 (its last texel) emitted (57, 6, 1) -- its byte and the two that start the
    next image -- where (57, 0, 0) is defined, and so did 90 to 143 hits of each of the four followed images."""
    for names, case in (small_texel_case, wide_texel_case, last_2bpp_case):
        check_texels(case, names, case.want, case.want_fetches, "oracle")


@gpu
@pytest.mark.parametrize("which", ["small", "wide", "last_2bpp"])
def test_texel_indexing(ctx, which, small_texel_case, wide_texel_case, last_2bpp_case):
    """Group (b): every image as a light's emit texture and in each pbr slot, u and v at the edges of [0, 1], at every
    i / size +- 1 ulp and outside; `last_2bpp` repeats the overrun images on the scene whose last texture is the 2-byte one."""
    names, case = {"small": small_texel_case, "wide": wide_texel_case, "last_2bpp": last_2bpp_case}[which]
    ctx.upload_scene(case.bench.sb)
    out, fetches = run_forms(ctx, case.rays, case.hits, which)
    check_texels(case, names, out, fetches, "device")
    assert_matches_oracle(case.bench, case.hits, out, case.want, which)
    assert np.array_equal(fetches, case.want_fetches)


# ---------------------------------------------------------------- (c) dielectric and metal
LENGTHS = (1e-3, 1.0, 1e3)


def directions(cos, azimuth=(1.0, 0.0)):
    """Incoming directions at angle acos(cos) to the normal (0, 1, 0), of every length of LENGTHS: (3 * len(cos), 3)."""
    cos = np.asarray(cos, np.float64)
    sin = np.sqrt(np.maximum(0.0, 1.0 - cos * cos))
    d = np.stack([sin * azimuth[0], -cos, sin * azimuth[1]], axis=-1)
    return np.concatenate([(d * s).astype(f32) for s in LENGTHS])


def unit_dot_replay(n, d):
    """dot(n, -unitVector(d)) in float32, as vec3.h evaluates it: to know that the inputs reach what they are meant to."""
    n, d = np.asarray(n, f32), np.asarray(d, f32)
    length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    u = -(d / length[:, None])
    return n[:, 0] * u[:, 0] + (n[:, 1] * u[:, 1] + n[:, 2] * u[:, 2])


@gpu
def test_dielectric_and_metal(ctx, abi, oracle):
    """Group (c): no libm call, so every output is compared on bits."""
    bench, osc = bench_for(abi, oracle)
    rng = np.random.default_rng(9)
    generic = np.concatenate([[1.0, 0.0, -0.0, 1e-40], [s * c for c in (1e-7, 1e-4, 1e-2) for s in (1, -1)], np.linspace(0.02, 0.98, 25)])
    normals = rng.normal(size=(500, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(f32)
    head_on = np.concatenate([(-normals * f32(s)).astype(f32) for s in LENGTHS])
    assert (unit_dot_replay(np.tile(normals, (3, 1)), head_on) > 1).any()  # the fmin(.., 1) is reached
    parts, bands = [], {}
    for ir in (1.5, 2.4, 1.0, 0.5):
        for front in (1, 0):
            name = "glass%g" % ir
            ratio = f32(1) / f32(ir) if front else f32(ir)
            cos = generic
            if ratio > 1:  # +-64 ulps of cos(theta) around the critical angle ratio * sin(theta) = 1
                cos = np.concatenate([cos, R.ulp_neighbours(np.sqrt(1.0 - 1.0 / float(ratio) ** 2), 64)])
            for az in ((1.0, 0.0), (0.6, 0.8)):
                d = directions(cos, az)
                if ratio > 1:
                    bands[(ir, front, az)] = (count(parts), len(d), len(generic))
                parts.append(bench.hits(name, len(d), d=d, front=front))
            parts.append(bench.hits(name, len(head_on), d=head_on, normal=np.tile(normals, (3, 1)), front=front))
    schlick = count(parts)
    d = directions(rng.uniform(0.01, 1.0, 2000))[2000:4000]  # 2 000 keyed draws decide reflect or refract (unit length)
    parts.append(bench.hits("glass1.5", len(d), d=d))
    metal_at = {}
    for fuzz in (0.0, 0.2, 1.0):
        cos = np.repeat([0.0, -0.0, 1e-7, -1e-7, 1e-4, -1e-4, 1e-2, -1e-2, 0.1, -0.1, 0.5], 60)
        d = directions(cos)
        metal_at[fuzz] = (count(parts), len(d))
        parts.append(bench.hits("metal%g" % fuzz, len(d), d=d))
    rays, hits = cat(parts)
    want, _ = osc.scatter_many(rays, hits, SEED)
    # the inputs reach both sides of every decision
    for (ir, front, az), (at, n, skip) in bands.items():
        y = want[at:at + n, 4].reshape(3, -1)[:, skip:]  # the band, at each length: reflected rays leave upwards
        assert (y > 0).any() and (y < 0).any(), (ir, front, az)
    y = want[schlick:schlick + 2000, 4]
    assert 100 < (y > 0).sum() < 1900
    for fuzz, (at, n) in metal_at.items():
        assert 0 < want[at:at + n, 9].sum() < n, fuzz
    ctx.upload_scene(bench.sb)
    out, fetches = run_forms(ctx, rays, hits, "dielectric and metal")
    assert_matches_oracle(bench, hits, out, want, "dielectric and metal", att_bits=True)
    assert not fetches.any()


# ---------------------------------------------------------------- (d) pbr with normal maps
@gpu
def test_pbr_normal_maps(ctx, abi, oracle):
    """Group (d): normal-map texels that give the zero vector, the corners and straight up; metalness and roughness
    textures reading 0 and 255; views perpendicular to the normal and behind it; roughness exactly 0 with NdotH = 1 (the
    view mirrored from the scatter direction the key draws: D = 0 / 0).  Direction and origin on bits, NaNs in the same
    places, attenuation within test_scatter_known_answers' tolerance.
    Measured share of bit-identical attenuations on an MI355X: 1.0000 (all 12 720 values); asserted >= 0.97, the bound
    test_scatter_known_answers sets."""
    bench, osc = bench_for(abi, oracle)
    views = [(0.3, -1.0, 0.2), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1e-3, 0.0), (0.0, -1e3, 0.0), (0.5, 0.25, -0.5)]
    tilt = dict(normal=(0.6, 0.8, 0.0), tangent=(0.8, -0.6, 0.0), bitangent=(0.0, 0.1, 1.0))  # not orthonormal: nothing asks for it
    parts = []
    for name in bench.mat:
        if name.startswith("pbr:"):
            for view in views:
                parts.append(bench.hits(name, 20, d=view, uv=(0.3, 0.6)))
                parts.append(bench.hits(name, 20, d=view, uv=(0.9, 0.1), **tilt))
    for name in ("smooth", "smooth_tex"):
        parts.append(bench.hits(name, 200))
    rays, hits = cat(parts)
    # roughness 0 and NdotH = 1: the scatter direction depends on the key and the normal alone, so a first pass tells it
    smooth = (hits["material"] == bench.mat["smooth"]) | (hits["material"] == bench.mat["smooth_tex"])
    sd = osc.scatter_many(rays, hits, SEED)[0][smooth, 3:6]  # unit vectors about the normal (0, 1, 0)
    rays["d"][smooth] = np.stack([sd[:, 0], -sd[:, 1], sd[:, 2]], axis=-1)  # view = (-sd.x, sd.y, -sd.z): sd + view = (0, 2 sd.y, 0)
    want, want_fetches = osc.scatter_many(rays, hits, SEED)
    assert np.isnan(want[smooth, 0:3]).any(axis=1).mean() > 0.5  # D = 0 / 0 is reached
    ctx.upload_scene(bench.sb)
    out, fetches = run_forms(ctx, rays, hits, "pbr")
    assert_matches_oracle(bench, hits, out, want, "pbr")
    assert np.array_equal(fetches, want_fetches)
    assert (fetches[hits["material"] == bench.mat["pbr:n_up:t0:t255"]] == 4).all()
    same = (_bits(out[:, 0:3]) == _bits(want[:, 0:3])) | np.isnan(want[:, 0:3])
    assert same.mean() >= 0.97, same.mean()
    print("pbr attenuations bit-identical: %.4f of %d" % (same.mean(), same.size))


# ---------------------------------------------------------------- the entry's argument checks
@gpu
def test_scatter_refuses_unknown_material(ctx, dev, abi, oracle):
    bench, _ = bench_for(abi, oracle)
    ctx.upload_scene(bench.sb)
    rays, hits = bench.hits(len(bench.sb.materials), 3)  # one past the last material
    hits["material"][:2] = 0
    for call in (lambda: ctx.scatter_test(rays, hits, SEED), lambda: ctx.scatter_test_form(rays, hits, SEED, 3)):
        with pytest.raises(dev.SrtError, match="hit 2 names material %d of %d" % (len(bench.sb.materials), len(bench.sb.materials))):
            call()
    hits["material"] = 0
    with pytest.raises(dev.SrtError, match="form 4"):
        ctx.scatter_test_form(rays, hits, SEED, 4)
