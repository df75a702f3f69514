"""The scenes of tests/exact_scenes.py and the helpers of tests/test_gpu_exact_frames.py, on the CPU: every scene passes
the structural check, the oracle renders each to the same bytes on one thread and on four (its counter-keyed generator makes a
sample independent of the thread that draws it -- what lets the GPU tests share one cached frame), the vectorised chunk sum
equals tests/chunk_sum_ref.py's integer statement, and OracleScene.sample_path retraces render()'s samples bit for bit."""
import numpy as np
import pytest

import chunk_sum_ref
import exact_scenes as X
import test_gpu_exact_frames as G

SCENE_KEYS = ([("random", seed, tier) for tier in X.TIERS for seed in range(6)] + [("room", tier) for tier in X.TIERS] +
              [("mesh", tier) for tier in X.TIERS])
SHAPES = {"random": (48, 27, 5, 6, 3), "room": (96, 54, 4, 16, 0), "mesh": (160, 90, 8, 4, 0)}  # test_gpu_exact_frames.FRAME_CASES

_scenes = {}


def scene(srt, abi, key):
    if key not in _scenes:
        _scenes[key] = G.build_scene(srt, abi, key)
    return _scenes[key]


@pytest.mark.parametrize("key", SCENE_KEYS, ids=str)
def test_scene_is_libm_free(srt, abi, key):
    sb = scene(srt, abi, key)
    tier = key[-1]
    X.assert_libm_free(sb, tier)
    kinds = X.material_kinds(sb)
    used = kinds["sphere"] | kinds["triangle"]
    assert all(t != abi.SRT_MAT_PBR for t, _ in used) == (tier == "A")
    if key[0] == "mesh":
        assert len(sb.triangles) and sum(len(t) for t in sb.triangles) == 3042 and G.tree_nodes(sb, abi) == 4043
        assert not any(sb.textures[m.albedoTex].kind != abi.SRT_TEX_SOLID for m in sb.materials if m.albedoTex >= 0)
        if tier == "B":  # pbr with a solid texture on triangles, pbr factors on spheres
            assert (abi.SRT_MAT_PBR, True) in kinds["triangle"] and (abi.SRT_MAT_PBR, False) in kinds["sphere"]


def test_structural_check_rejects_what_it_must(srt, abi):
    """assert_libm_free is what keeps single-precision libm out: it must refuse a checker, an image, a normal map, and pbr
    in tier A."""
    def with_material(make):
        sb = abi.SceneBuilder()
        sb.add_sphere((0.0, 0.0, 0.0), 1.0, make(sb))
        return sb
    X.assert_libm_free(with_material(lambda sb: sb.pbr(albedo_tex=sb.solid(1.0, 2.0, 3.0))), "B")
    for tier, make in (("A", lambda sb: sb.pbr(albedo=(0.5, 0.5, 0.5, 1.0))),
                       ("B", lambda sb: sb.pbr(albedo_tex=sb.checker((0.1, 0.2, 0.3), (0.9, 0.9, 0.9)))),
                       ("B", lambda sb: sb.pbr(albedo_tex=sb.image(np.zeros((2, 2, 3), np.uint8), 3))),
                       ("B", lambda sb: sb.pbr(normal_tex=sb.solid(128.0, 128.0, 255.0))),
                       ("A", lambda sb: sb.light(emit_tex=sb.checker((0.1, 0.2, 0.3), (0.9, 0.9, 0.9)))),
                       ("A", lambda sb: sb.light(emit_tex=sb.image(None, 3)))):
        with pytest.raises(AssertionError):
            X.assert_libm_free(with_material(make), tier)
    with pytest.raises(AssertionError):
        X.assert_libm_free(srt.scenes.scene_masterchief(), "B")


def test_random_scenes_cover_layouts_and_materials(abi):
    """Seeds 0-5 of each tier: the three world layouts twice; over the tier's seeds every material kind of the tier occurs,
    in tier B pbr with and without a solid texture on spheres and with one on triangles."""
    for tier in X.TIERS:
        scenes = [X.random(abi, seed, tier) for seed in range(6)]
        assert [sb.layout for sb in scenes] == [0, 1, 2, 0, 1, 2]
        assert [len(sb.world) > 1 for sb in scenes] == [False, True, True] * 2
        sph = set().union(*(X.material_kinds(sb)["sphere"] for sb in scenes))
        tri = set().union(*(X.material_kinds(sb)["triangle"] for sb in scenes))
        assert {(abi.SRT_MAT_METAL, False), (abi.SRT_MAT_DIELECTRIC, False), (abi.SRT_MAT_LIGHT, True)} <= sph
        if tier == "B":
            assert {(abi.SRT_MAT_PBR, False), (abi.SRT_MAT_PBR, True)} <= sph and (abi.SRT_MAT_PBR, True) in tri
        a, b = X.random(abi, 4, tier), X.random(abi, 4, tier)
        assert bytes(a.desc().spheres[0]) == bytes(b.desc().spheres[0]) and a.num_prims == b.num_prims  # seeded
    seed, sb = X.random_with_tree(abi, "B")
    assert sb.layout == 0 and 24 < G.tree_nodes(sb, abi) < 200


@pytest.mark.parametrize("key", SCENE_KEYS, ids=str)
def test_oracle_frame_is_thread_independent(srt, abi, oracle, key):
    """OracleScene.render(RNG_COUNTER): the same bytes, rgba and stats on one thread and on four; no texel is fetched."""
    sb = scene(srt, abi, key)
    W, H, spp, bounces, first = SHAPES[key[0]]
    if key[0] == "room":
        W, H = 48, 27  # a quarter of the GPU test's frame: the single-thread render is what takes the time here
    if key[0] == "mesh":
        W, H, spp = 80, 45, 4
    p = abi.default_render_params(W, H, spp, bounces, seed=5, sample_first=first, count_stats=1)
    cam = oracle.make_camera(abi.default_camera_params())
    osc = oracle.OracleScene(sb)
    a1, r1, s1 = osc.render(cam, p, oracle.RNG_COUNTER, threads=1)
    a4, r4, s4 = osc.render(cam, p, oracle.RNG_COUNTER, threads=4)
    assert a1.tobytes() == a4.tobytes() and r1.tobytes() == r4.tobytes() and s1 == s4
    assert s1["texelFetches"] == 0 and s1["samples"] == W * H * spp
    if key[-1] == "A":
        assert not np.isnan(a1).any()


def test_sample_path_retraces_render(srt, abi, oracle):
    """sample_path's colour is the sample render() adds (spp = 1 at sample_first = s, bit for bit), its steps are the rays
    render() counts, each step's hit is what trace() makes of its ray, and the colour is the steps' emitted and attenuation
    folded from the last bounce up (main.cpp:48-51)."""
    key = ("room", "B")
    sb = scene(srt, abi, key)
    cam = oracle.make_camera(abi.default_camera_params())
    osc = oracle.OracleScene(sb)
    W, H, bounces = 24, 13, 12
    bg = np.array([0.53, 0.81, 0.92], np.float32)
    rays = 0
    for s in (0, 5):
        p = abi.default_render_params(W, H, 1, bounces, seed=9, sample_first=s, count_stats=1)
        acc, _, st = osc.render(cam, p, oracle.RNG_COUNTER, threads=4)
        for y in range(H):
            for x in range(W):
                steps, colour = osc.sample_path(cam, p, x, y, s)
                assert G._same(colour, acc[y, x, :3]), (x, y, s)
                rays += len(steps)
                value = bg if len(steps) and steps[-1]["prim"] < 0 else np.zeros(3, np.float32)
                for st_ in steps[::-1]:
                    if st_["prim"] >= 0:
                        value = (st_["emitted"] + value * st_["attenuation"]).astype(np.float32) if st_["scattered"] else st_["emitted"]
                assert G._same(value, colour), (x, y, s)
        assert rays == st["rays"]
        rays = 0
    p = abi.default_render_params(W, H, 1, bounces, seed=9)
    steps, _ = osc.sample_path(cam, p, 11, 6, 0)
    r = np.zeros(len(steps), abi.RAY_DTYPE)
    r["o"], r["d"], r["time"], r["tMin"], r["tMax"] = steps["o"], steps["d"], steps["time"], 0.001, np.inf
    hits = osc.trace(r)
    assert np.array_equal(hits["prim"], steps["prim"]) and G._same(hits["t"], steps["t"]) and np.array_equal(hits["material"], steps["material"])
    assert len(steps) > 4


def test_fixed_chunk_sum_is_the_integer_statement():
    """fixed_chunk_sum against chunk_sum_ref.rows_sum (Python integers) on its directed rows (double rounding, ties) and on
    seeded rows with tiny, negative, NaN, infinite and beyond-the-limit entries; and where every partial sum is at least
    2^-13 it is the float64 sum rounded once, which is what tests/test_gpu_parity.py's chunked oracle computes."""
    for rows, want in (chunk_sum_ref.double_rounding_rows(), chunk_sum_ref.tie_rows()):
        parts = np.repeat(rows.T[:, :, None], 3, axis=2)
        assert G._same(G.fixed_chunk_sum(parts)[:, 0], want)
    rng = np.random.default_rng(8)
    for chunks in (2, 3, 7, 8, 32):
        rows = (rng.uniform(0, 4, (400, chunks)) * 2.0 ** rng.integers(-30, 8, (400, chunks))).astype(np.float32)
        rows[::7] *= -1
        plain = rows[:200].copy()
        plain[plain < 2.0 ** -13] = 0.5
        plain = np.abs(plain)
        rows[5, 0], rows[6, 1], rows[7, 0], rows[8, 0], rows[8, 1] = np.nan, np.inf, -np.inf, np.inf, -np.inf
        rows[9, 0] = chunk_sum_ref.limit(chunks)
        rows[10, :] = -0.0
        for r in (rows, plain):
            parts = np.repeat(r.T[:, :, None], 3, axis=2)
            got = G.fixed_chunk_sum(parts)
            assert G._same(got[:, 0], chunk_sum_ref.rows_sum(r, chunks)) and G._same(got[:, 0], got[:, 2])
        with np.errstate(over="ignore"):
            assert G._same(G.fixed_chunk_sum(np.repeat(plain.T[:, :, None], 3, axis=2))[:, 0], plain.astype(np.float64).sum(axis=1).astype(np.float32))


class OracleAsKernel:
    """The part of a device context explain_pixel uses, served by an OracleScene: a stand-in kernel whose difference from
    the oracle under comparison is known, because the test made it."""

    def __init__(self, oracle, abi, osc, cam):
        self.oracle, self.abi, self.osc, self.cam = oracle, abi, osc, cam

    def render_image(self, p, want_accum=True, want_rgba=True):
        acc, rgba, _ = self.osc.render(self.cam, p, self.oracle.RNG_COUNTER, threads=4, want_stats=False)
        return acc, rgba

    def render_aov(self, p, depth):
        ctx = self

        class Lazy:
            def __getitem__(self, yx):
                steps, _ = ctx.osc.sample_path(ctx.cam, p, yx[1], yx[0], p.sampleFirst)
                rec = np.zeros((), ctx.abi.AOV_DTYPE)
                if depth < len(steps):
                    for f in ("o", "d", "time", "prim", "t"):
                        rec[f] = steps[depth][f]
                    rec["valid"] = 1
                return rec
        return Lazy()

    def scatter_test(self, rays, hits, seed):
        return self.osc.scatter_many(rays, hits, seed)[0]


def test_explain_pixel_names_sample_bounce_and_material(abi, oracle):
    """explain_pixel on a stand-in kernel that is the oracle of a scene altered in one known place: a metal's albedo moved
    by one ulp (rays and hits all agree: the attenuation at the first hit of that metal is named), a sphere moved (a hit
    differs), a pbr factor moved by an ulp (no draw-free shading to ask: the truncated paths name the bounce).  The pixel
    is the first that differs, as assert_frame_identical picks it."""
    cam = oracle.make_camera(abi.default_camera_params())
    p = abi.default_render_params(32, 18, 3, 8, seed=12, sample_first=2)

    def first_difference(tier, alter):
        a, b = X.room(abi, tier), X.room(abi, tier)
        alter(b)
        oa, ob = oracle.OracleScene(a), oracle.OracleScene(b)
        want = oa.render(cam, p, oracle.RNG_COUNTER, threads=4)
        got = ob.render(cam, p, oracle.RNG_COUNTER, threads=4)
        seen = {}
        with pytest.raises(pytest.fail.Exception):
            G.assert_frame_identical(got[0], got[1], got[2], *want, what="altered",
                                     explain=lambda x, y: seen.update(G.explain_pixel(OracleAsKernel(oracle, abi, ob, cam), oa, cam, p, x, y)))
        steps, _ = oa.sample_path(cam, abi.default_render_params(32, 18, 1, 8, seed=12, sample_first=seen["sample"]),
                                  seen["pixel"][0], seen["pixel"][1], seen["sample"])
        return seen, steps

    def albedo_ulp(k):
        def alter(sb):
            sb.materials[k].albedo[1] = float(np.nextafter(np.float32(sb.materials[k].albedo[1]), np.float32(2)))
        return alter

    wall = 0  # room(): material 0 is the enclosing fuzzy metal
    seen, steps = first_difference("A", albedo_ulp(wall))
    assert 2 <= seen["sample"] < 5 and seen["what"].startswith("attenuation"), seen
    d = seen["depth"]
    assert steps[d]["material"] == wall and all(st["material"] != wall for st in steps[:d]), (seen, steps["material"])
    assert seen["material_before"] == (int(steps[d - 1]["material"]) if d else None)

    def move(sb):
        sb.spheres[3].center0[0] += 0.25  # the small mirror sphere
        sb.spheres[3].center1[0] += 0.25
    seen, steps = first_difference("A", move)
    assert seen["what"].startswith("hit") or seen["what"] == "ray" or "trace" in seen["what"], seen
    assert seen["depth"] is not None and seen["depth"] < len(steps) + 1

    pbr = 1  # tier B: the pbr sphere in the middle
    seen, steps = first_difference("B", albedo_ulp(pbr))
    assert seen["what"].startswith("the sample's value"), seen
    # its attenuation at bounce d shows once the path goes on to bounce d + 1 and brings light back: depth is past a pbr hit
    assert any(st["material"] == pbr for st in steps[:seen["depth"] + 1]), (seen, steps["material"])


def test_residual_list_is_within_its_cap():
    """tests/golden/exact_residual.json: at most two entries, each with its proven cause written down."""
    entries = G.residual()
    assert len(entries) <= 2
    for e in entries:
        assert e["scene"] in ("random", "room", "mesh") and len(e["pixel"]) == 2 and e["cause"]


def test_assert_frame_identical_reports_the_pixel():
    """The comparison itself: identical frames pass, NaNs match by position only, one moved bit, one count, one byte of a
    defined pixel and one counter each fail, naming the pixel; a listed pixel is left out."""
    rng = np.random.default_rng(2)
    acc = rng.uniform(0, 3, (5, 7, 4)).astype(np.float32)
    acc[..., 3] = 4.0
    acc[2, 3, 1] = np.nan
    rgba = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    st = dict.fromkeys(G.COUNTERS, 5)
    st["texelFetches"] = 0
    G.assert_frame_identical(acc.copy(), rgba.copy(), dict(st), acc, rgba, st, "same")
    other_nan = rgba.copy()
    other_nan[2, 3, 0] ^= 1  # the bytes of a NaN pixel are not compared
    G.assert_frame_identical(acc.copy(), other_nan, dict(st), acc, rgba, st, "NaN pixel's bytes")

    def moved(f):
        a, r, s = acc.copy(), rgba.copy(), dict(st)
        f(a, r, s)
        return a, r, s

    def bit(a, r, s):
        a[1, 2, 0] = np.nextafter(a[1, 2, 0], np.float32(9))

    def count(a, r, s):
        a[1, 2, 3] = 3.0

    def byte(a, r, s):
        r[1, 2, 2] ^= 1

    def nan_gone(a, r, s):
        a[2, 3, 1] = 0.0

    def nan_new(a, r, s):
        a[1, 2, 1] = np.nan

    for f in (bit, count, byte, nan_gone, nan_new):
        with pytest.raises(pytest.fail.Exception, match=r"first \(x [23], y [12]\)"):
            G.assert_frame_identical(*moved(f), acc, rgba, st, f.__name__, explain=lambda x, y: "explained")
    G.assert_frame_identical(*moved(bit), acc, rgba, st, "listed", skip=[(2, 1)])
    with pytest.raises(AssertionError):
        G.assert_frame_identical(*moved(lambda a, r, s: s.update(rays=6)), acc, rgba, st, "counter")
