"""The CPU oracle (oracle/oracle.cpp) against the reference's own headers as g++ compiles them (oracle/ref_harness.cpp,
run by tests/ref_harness.py), function by function and frame by frame.

Every comparison is on bits: both sides are IEEE binary32 code from the same compiler without FMA, calling the same libm
on the same machine.  There is no tolerance anywhere in this file.  NaNs are compared by position.  A field that differs
means the oracle restates the reference wrongly -- and so does the kernel that was matched to it.

The tests that run the harness live need oracle/_ref/ref_harness; where neither it nor the reference's sources exist they
skip.  The tests over tests/golden/ref_*.npz (the harness's recorded results, written by tests/make_golden.py) always run.

Inputs left out because the REFERENCE's behaviour on them is undefined (left out by what the input is, never by what
comes out):"""
import os

import numpy as np
import pytest

import exact_scenes
import ref_cases
import ref_harness as H
import shade_ref
from conftest import GOLD

f32 = np.float32

EXCLUDED = {
    "texture coordinates that are NaN": "texture.h:136-137 casts NaN * width to int",
    "a 1- or 2-byte image's texels whose pixel[1] or pixel[2] lies past the image": "texture.h:147 reads past the block "
    "stbi_load returned; in whole frames (the `textures` variant, the iron maps) the read is not left out: it lands in "
    "the two zero bytes the harness's own stbi_load appends, which is also what the oracle defines",
    "pbrMetallicRoughness built by the constructors of material.h:25-40": "metalness, roughness and anisotropy stay "
    "uninitialised (material.h:82-84); the harness only uses material.h:67-70 and gltfLoad's material.h:60-66",
    "a pixel sum that is NaN, in RGBA8": "color.h:37-39 casts NaN to uint8_t; such a pixel's bytes are not compared, its "
    "float sum is (NaN by position)",
}
__doc__ += "".join("\n  * %s -- %s" % kv for kv in EXCLUDED.items())

SCENES = ("spheres", "iron", "masterchief")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_same_floats(got, want, what):
    """Equal bit for bit, NaNs in the same places."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(-1) & ~nan.reshape(-1))
    assert len(bad) == 0, (what, len(bad), bad[:4], got.reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]])


def assert_hits_identical(got, want, names=None):
    """Every field of HIT_DTYPE, the four counters included."""
    def where(bad):
        i = int(np.flatnonzero(bad)[0])
        return i, names[i] if names is not None and i < len(names) else None

    for f in got.dtype.names:
        a, b = got[f], want[f]
        if a.dtype == f32:
            nan = np.isnan(b)
            bad = (np.isnan(a) != nan) | ((_bits(a) != _bits(b)) & ~nan)
        else:
            bad = a != b
        bad = bad.reshape(len(got), -1).any(axis=1)
        assert not bad.any(), (f, int(bad.sum()), where(bad), a[bad][:2], b[bad][:2])


def assert_trees_identical(got, want, what):
    """Per node in pre-order: the child kinds and primitive ids (left / right) and the box bits."""
    assert len(got) == len(want), (what, "node count")
    for f in ("left", "right"):
        assert np.array_equal(got[f], want[f]), (what, f)
    for f in ("bmin", "bmax"):
        assert np.array_equal(_bits(got[f]), _bits(want[f])), (what, f)


# ---------------------------------------------------------------------------------------------------- scenes
def _variants(abi):
    from test_gpu_properties import _world_variants
    return _world_variants(abi)


def dielectric_scene(abi):
    """Three glass spheres on the checker ground: front and back faces, total internal reflection and the reflectance
    draw in every path (material.h:104-137)."""
    sb = abi.SceneBuilder()
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.pbr(albedo_tex=sb.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))))
    sb.add_sphere((-2.2, 1.5, 0.0), 1.0, sb.dielectric(1.5))
    sb.add_sphere((0.0, 2.0, 0.5), 1.5, sb.dielectric(2.4))
    sb.add_sphere((2.4, 1.2, 1.0), 1.0, sb.dielectric(1.0 / 1.5))
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


_scene_cache = {}


def scene(srt, abi, name):
    """(scene, whether its triangles go through gltfLoad in the harness), built once."""
    if name not in _scene_cache:
        if name in srt.scenes.SCENES:
            sb = srt.scenes.SCENES[name]()
        elif name == "edges":
            sb = ref_cases.edge_scene(abi)
        elif name == "dielectric":
            sb = dielectric_scene(abi)
        elif name.startswith("exact_"):  # "exact_room_A", "exact_random_B": tests/exact_scenes.py
            _, kind, tier = name.split("_")
            sb = exact_scenes.room(abi, tier) if kind == "room" else exact_scenes.random(abi, EXACT_RANDOM_SEED, tier)
        else:
            sb = _variants(abi)[name]
        _scene_cache[name] = sb
    return _scene_cache[name], name == "masterchief"


# ---------------------------------------------------------------------------------------------------- (a) generator
def test_generator(oracle):
    H.require()
    n = 200000
    assert np.array_equal(_bits(H.rng(n)), _bits(oracle.rng_kat(n)))
    want = np.zeros(3, f32)
    oracle.lib().orc_random_vec3_kat(want.ctypes.data)
    got = H.random_vec3()
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    assert np.allclose(got, (0.811584, -0.729046, 0.629447), atol=1e-6)  # SURVEY.md A.5, g++'s order


# ---------------------------------------------------------------------------------------------------- (b) tree build
TREE_SCENES = SCENES + ("sphere_field", "list", "two_bvh", "moving", "edges")


@pytest.mark.parametrize("name", TREE_SCENES)
def test_tree_build(srt, abi, oracle, name):
    """boxCompare, std::sort with it, surroundingBox, triangle::boundingBox's padding, the moving sphere's two-time box,
    and the draws: one per node, after the scene's own (sphere_field draws its placements first)."""
    H.require()
    sb, gltf = scene(srt, abi, name)
    items, position = H.tree(sb, gltf)
    osc = oracle.OracleScene(sb)
    d = sb.desc()
    roots = [i for i in range(d.numWorld) if d.world[i].kind == abi.SRT_WORLD_BVH]
    assert len(items) == len(roots)
    for (nodes, depth), item in zip(items, roots):
        want, want_depth = osc.bvh(item)
        assert_trees_identical(nodes, want, (name, item))
        assert depth == want_depth
    assert position == int(getattr(sb, "global_rng_draws", 0)) + osc.build_draws()
    assert osc.build_draws() == sum(len(nodes) for nodes, _ in items)
    if name == "sphere_field":
        assert sb.global_rng_draws > 0


# ---------------------------------------------------------------------------------------------------- (c) hit records
@pytest.mark.parametrize("name", SCENES + ("edges", "moving"))
def test_hit_records(srt, abi, oracle, name):
    """world.hit on the golden fixed rays and on the edge set (tests/ref_cases.py names every ray): every field of
    HIT_DTYPE and the four counters."""
    H.require()
    sb, gltf = scene(srt, abi, name)
    rays, names = ref_cases.edge_rays(abi, sb)
    assert 100 <= len(rays) and len(set(names)) == len(names)
    if name in SCENES:
        fixed = np.load(os.path.join(GOLD, "trace_%s.npz" % name))["rays"]
        rays, names = np.concatenate([rays, fixed]), names + ["fixed ray %d" % i for i in range(len(fixed))]
    got = oracle.OracleScene(sb).trace(rays)
    want = H.trace(sb, rays, gltf)
    assert_hits_identical(got, want, names)
    assert (want["prim"] >= 0).sum() > len(rays) // 8


def test_edge_set_reaches_its_cases(srt, abi):
    """The edge scene's rays reach the branches they are named for (read off the recorded reference results)."""
    g = np.load(os.path.join(GOLD, "ref_edges.npz"))
    names, hits = [str(n) for n in g["names"]], g["hits"][:len(g["names"])]
    by = dict(zip(names, hits))
    assert by["triangle 0 front"]["prim"] >= 0 and by["triangle 0 back-facing"]["prim"] != 0
    assert by["triangle 0 tMax below t"]["prim"] < 0  # the boxes cull it
    assert by["triangle 0 tMax just below t"]["prim"] == 0 and by["triangle 0 tMax just below t"]["t"] == 1.0  # F4: t > tMax
    assert by["triangle 0 through vertex 2"]["prim"] == 1 and np.isnan(by["triangle 0 through vertex 2"]["uv"]).all()  # d_i = 0: inf / inf
    assert by["triangle 2 front"]["prim"] != 2  # zero area
    assert by["triangle 3 front"]["prim"] == 3 and (by["triangle 3 front"]["tangent"] == 0).all()  # uv determinant 0
    assert by["sphere 1@0 tangent ray, discriminant 0"]["prim"] == 7 and by["sphere 1@0 tangent ray, discriminant 0"]["t"] == 1.0
    assert by["sphere 1@0 tangent ray, one ulp inside (discriminant 0 on)"]["prim"] == 7
    assert by["sphere 1@0 tangent ray, one ulp outside (discriminant 0 on)"]["prim"] < 0
    assert by["sphere 1@0 normal near +1Y, dx/R 0"]["tangent"][0] != by["sphere 1@0 normal near +1Y, dx/R 0.001"]["tangent"][0]
    t_near, t_far = by["sphere 1@0 tMin at the near root"]["t"], by["sphere 1@0 tMin above the near root"]["t"]
    assert t_near == 2.0 and t_far == 4.0
    moving = [by["sphere 0@%g axis-parallel +1z" % t]["p"] for t in (0, 1, -0.5, 1.5)]
    assert len({tuple(p) for p in moving}) == 4


# ---------------------------------------------------------------------------------------------------- (d) textures
def test_textures_and_emitted(abi, oracle):
    """checker::value, imagePNG::value and solidColor, all through diffuseLight::emitted, at shade_ref.checker_points and
    the texel edges of test_shading.py (shade_ref.uv_coordinates)."""
    H.require()
    rng = np.random.default_rng(9)
    sb = abi.SceneBuilder()
    images = {"rgb6x4": (6, 4, 3), "rgba9x5": (9, 5, 4), "one1x1": (1, 1, 3), "g7x5": (7, 5, 1), "ga5x3": (5, 3, 2)}
    lights = {"solid": sb.light((250.2, 220.9, 110.2)), "checker": sb.light(emit_tex=sb.checker((0.9, 0.5, 0.25), (0.1, 0.5, 0.75))),
              "failed": sb.light(emit_tex=sb.image(None, 3))}
    for name, (w, h, bpp) in images.items():
        lights[name] = sb.light(emit_tex=sb.image(rng.integers(1, 256, (h, w, bpp), dtype=np.uint8), bpp))
    parts = []

    def add(light, u, v, p):
        q = np.zeros(len(p), H.VALUE_DTYPE)
        q["kind"], q["id"], q["u"], q["v"], q["p"] = H.VALUE_EMITTED, lights[light], u, v, p
        parts.append(q)

    points = np.concatenate([shade_ref.checker_points(shade_ref.checker_coordinates(n_uniform=2000)), shade_ref.underflow_points()])
    add("checker", 0.5, 0.5, points)
    add("solid", 0.5, 0.5, points[:16])
    for name, (w, h, bpp) in list(images.items()) + [("failed", (1, 1, 3))]:
        us, vs = np.meshgrid(shade_ref.uv_coordinates(w), shade_ref.uv_coordinates(h), indexing="ij")
        us, vs = us.reshape(-1), vs.reshape(-1)
        keep = ~(np.isnan(us) | np.isnan(vs))  # EXCLUDED: NaN coordinates
        if bpp < 3:  # EXCLUDED: pixel[2] past the image (from the texel index, shade_ref.texel_index)
            i, j = shade_ref.texel_index(w, h, us, vs)
            keep &= (j * w + i) * bpp + 2 < w * h * bpp
        assert keep.sum() > 0.5 * len(keep)
        add(name, us[keep], vs[keep], np.broadcast_to(np.array([0.05, 0.4, 0.05], f32), (int(keep.sum()), 3)))
    q = np.concatenate(parts)
    got_harness = H.values(sb, q)
    rays, hits = np.zeros(len(q), abi.RAY_DTYPE), np.zeros(len(q), abi.HIT_DTYPE)
    rays["d"] = (0.0, -1.0, 0.0)
    hits["p"], hits["uv"][:, 0], hits["uv"][:, 1], hits["material"], hits["normal"] = q["p"], q["u"], q["v"], q["id"], (0, 1, 0)
    out, _, _ = oracle.OracleScene(sb).scatter_many_mt(rays, hits)
    assert (out[:, 9] == 0).all()  # diffuseLight::scatter is false
    assert_same_floats(out[:, 10:13], got_harness, "emitted")
    assert len(np.unique(got_harness[:len(points)], axis=0)) == 2  # both checker colours were reached


# ---------------------------------------------------------------------------------------------------- (e) scatter
@pytest.mark.parametrize("pre_draws", [0, 7])
def test_scatter(abi, oracle, pre_draws):
    """Every material's scatter() and emitted() on a fixed list of records, all in one process so the stream is
    continuous: bool, attenuation, scattered origin, direction and time, emitted, and the draw after the last record
    (both sides consumed the same number).  One record that differs desynchronises the rest: the first is reported."""
    H.require()
    sb, materials = ref_cases.scatter_scene(abi)
    sb.global_rng_draws = pre_draws
    rays, hits, names = ref_cases.scatter_records(abi, materials)
    want, want_time, want_next = H.scatter(sb, rays, hits)
    got, got_time, got_next = oracle.OracleScene(sb).scatter_many_mt(rays, hits, pre_draws)
    nan = np.isnan(want)
    bad = ((np.isnan(got) != nan) | ((_bits(got) != _bits(want)) & ~nan)).any(axis=1) | (_bits(got_time) != _bits(want_time))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail("first differing record %d: %s\n oracle  %r time %r\n harness %r time %r" % (i, names[i], got[i], got_time[i], want[i], want_time[i]))
    assert _bits(got_next) == _bits(want_next), "the two sides consumed different numbers of draws"
    # the list reaches the branches it is there for
    by = {n: k for k, n in enumerate(names)}
    ok = want[:, 9]
    assert (ok[[k for n, k in by.items() if n.startswith("light")]] == 0).all()
    metal = [k for n, k in by.items() if n.startswith("metal fuzz 1.7")]
    assert 0 < ok[metal].sum() < len(metal)  # fuzz can turn the ray under the surface (material.h:96)
    glass = np.array([k for n, k in by.items() if n.startswith("dielectric 1.5")])
    refl = (want[glass, 3:6] * hits["normal"][glass]).sum(1) > 0
    assert refl.any() and (~refl).any()  # reflected (total internal reflection or the draw) and refracted


# ---------------------------------------------------------------------------------------------------- (f) whole frames
FRAMES = {  # scene: width, height, samples, bounces
    "spheres": (64, 36, 4, 8), "iron": (64, 36, 4, 4), "masterchief": (64, 36, 4, 4),  # those of render_<scene>.npz
    "sphere_field": (64, 36, 4, 4), "moving": (32, 18, 2, 6), "textures": (32, 18, 2, 6), "dielectric": (48, 27, 4, 8),
    # the scenes the GPU's zero-tolerance frames use (tests/exact_scenes.py), so that the reference's own headers pin the
    # oracle on exactly these: the closed room with deep paths, and one random scene (a single tree) per tier
    "exact_room_A": (48, 27, 2, 12), "exact_room_B": (48, 27, 2, 12), "exact_random_A": (48, 27, 3, 6), "exact_random_B": (48, 27, 3, 6),
}
EXACT_RANDOM_SEED = 3


@pytest.mark.parametrize("name", list(FRAMES))
def test_whole_frames(srt, abi, oracle, name):
    """The harness's pixel loop against OracleScene.render(RNG_MT, threads=1): float sums per pixel and RGBA8, and the
    generator's position after the frame.  Covers the camera's construction and getRay with an aperture, a sample's draw
    order, rayColor's recursion and bounce limit, writeColorTarget."""
    H.require()
    sb, gltf = scene(srt, abi, name)
    W, Hh, spp, bounces = FRAMES[name]
    p = abi.default_render_params(W, Hh, spp, bounces, seed=7)
    cp = abi.default_camera_params()
    want, want_rgba, position = H.render(sb, cp, p, gltf)
    osc = oracle.OracleScene(sb)  # a fresh generator: the tree build, then the frame, like a new process
    got, got_rgba, st = osc.render(oracle.make_camera(cp), p, oracle.RNG_MT, threads=1)
    assert_same_floats(got, want, name)
    defined = ~np.isnan(want[..., :3]).any(axis=-1)  # EXCLUDED: the bytes of a NaN pixel
    assert np.array_equal(got_rgba[defined], want_rgba[defined])
    assert position == int(getattr(sb, "global_rng_draws", 0)) + osc.build_draws() + st["rngDraws"]
    if name in SCENES:
        g = np.load(os.path.join(GOLD, "render_%s.npz" % name))
        assert (int(g["width"]), int(g["height"]), int(g["spp"]), int(g["max_bounce"])) == FRAMES[name]
        assert_same_floats(want, g["accum_mt"], name + " committed accum_mt")
        assert np.array_equal(want_rgba[defined], g["rgba_mt"][defined])


CAMERAS = ref_cases.CAMERAS


@pytest.mark.parametrize("k", range(len(CAMERAS)))
def test_cameras(srt, abi, oracle, k):
    """The camera's constructor (camera.h:10-38: the double tan and the double viewport sizes cast into the vectors) and
    getRay at other settings than main.cpp's, through a 9 x 5 frame of the spheres scene at one sample."""
    H.require()
    sb, _ = scene(srt, abi, "spheres")
    cp = abi.SrtCameraParams()
    cp.eye[:], cp.lookAt[:], cp.up[:] = CAMERAS[k][:3]
    cp.vfovDegrees, cp.aspect, cp.aperture, cp.focusDist, cp.time0, cp.time1 = CAMERAS[k][3:]
    p = abi.default_render_params(9, 5, 1, 3, seed=7)
    want, _, position = H.render(sb, cp, p)
    osc = oracle.OracleScene(sb)
    got, _, st = osc.render(oracle.make_camera(cp), p, oracle.RNG_MT, threads=1)
    assert_same_floats(got, want, CAMERAS[k])
    assert position == osc.build_draws() + st["rngDraws"]


# ---------------------------------------------------------------------------------------------------- recorded results
REF_FIXTURES = SCENES + ("edges",)


def expected_fixture_rays(abi, sb, name):
    """The rays a ref_<scene>.npz holds: the whole edge set, then every second ray of trace_<scene>.npz."""
    rays, names = ref_cases.edge_rays(abi, sb)
    if name in SCENES:
        rays = np.concatenate([rays, np.load(os.path.join(GOLD, "trace_%s.npz" % name))["rays"][::2]])
    return rays, names


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_oracle_reproduces_recorded_reference(srt, abi, oracle, name):
    """Always runs: tests/golden/ref_<scene>.npz holds what the harness gave (hits, counters, the pre-order tree)."""
    g = np.load(os.path.join(GOLD, "ref_%s.npz" % name))
    sb, _ = scene(srt, abi, name)
    rays, names = expected_fixture_rays(abi, sb, name)
    assert g["rays"].tobytes() == rays.tobytes() and [str(n) for n in g["names"]] == names  # the whole edge set is in it
    osc = oracle.OracleScene(sb)
    assert_hits_identical(osc.trace(g["rays"]), g["hits"], names)
    near = osc.trace(g["rays"], abi.SRT_TRAVERSE_CLOSEST)
    assert np.array_equal(near["prim"], g["brute_prim"])  # the oracle's closest mode is the brute force
    assert_same_floats(near["t"], g["brute_t"], "closest t")
    nodes, depth = osc.bvh(0)
    assert_trees_identical(nodes, g["nodes"], name)
    assert depth == int(g["depth"]) and osc.build_draws() == int(g["build_draws"])
    assert os.path.getsize(os.path.join(GOLD, "ref_%s.npz" % name)) <= 370 * 1024


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_harness_reproduces_recorded_reference(srt, abi, name):
    H.require()
    g = np.load(os.path.join(GOLD, "ref_%s.npz" % name))
    sb, gltf = scene(srt, abi, name)
    assert_hits_identical(H.trace(sb, g["rays"], gltf), g["hits"])
    near = H.closest(sb, g["rays"], gltf)
    for f, key in (("prim", "closest_prim"), ("ties", "closest_ties"), ("brute_prim", "brute_prim")):
        assert np.array_equal(near[f], g[key]), key
    assert_same_floats(near["t"], g["closest_t"], "closest t")
    assert_same_floats(near["brute_t"], g["brute_t"], "brute t")
    items, position = H.tree(sb, gltf)
    assert_trees_identical(items[0][0], g["nodes"], name)
    assert items[0][1] == int(g["depth"]) and position == int(g["build_draws"])
