"""The sign form of the certified slab test (csrc/srt_slab.h: a box's near and far planes picked by the sign of the ray's
reciprocal, twelve FMAs and no min/max pairs) in the path-pool kernel over a whole LDS-resident tree, against the 256-thread
step-scheduler kernel, which keeps the min/max form, and against the CPU oracle.  No tolerances: accumulators equal in
bits (tests/test_gpu_exact_frames.assert_frame_identical), all eight counters -- node visits and box passes among them --
equal to the oracle's.  Frames are 33 x 17 at 4 samples and 6 bounces on tier-A scenes of tests/exact_scenes.py (no libm
call in the shading).

  * a random-tree scene seen from inside its cloud of geometry: rays with a hit in all eight direction octants (asserted
    on the kernel's own ray records), so both signs of every axis pick the near plane;
  * planes at coordinate 0 and flat boxes: axis-aligned triangles in the three coordinate planes, spheres of radius 0;
  * a frame after srtUpdateTriangles + srtRefitScene, whose device pass computes the ordered-box word again;
  * an INVERTED node box.  validateScene admits a sphere of negative radius, and its box is (c - r, c + r) with min > max on
    every axis; as a tree of its own its node box is that box.  The reference orders the two quotients per visit, so it
    treats the box as the ordered one; the sign form must not decide such a scene: the ordered-box word is 0, every ray
    of the path-pool kernel is uncertified and takes the exact test on every visit -- same bits, same counters.  A refit
    after the radius has been made positive raises the word again."""
import copy

import numpy as np
import pytest

import exact_scenes
import refit_ref as RF
from test_gpu_exact_frames import COUNTERS, assert_frame_identical, counted, oracle_frame

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, BOUNCES = 33, 17, 4, 6
FORMS = {"wavefront": (3,), "l1_nodes": (0,)}  # launch_info()["lds_tree_mode"] of the path-pool kernel / the 256-thread kernel


@pytest.fixture()
def forms(ctx):
    """render(sb, cams, p, after_upload=None) -> {form: (acc, rgba, stats)} of the two kernels, tunables restored afterwards."""
    saved = {k: ctx.get_tunable(k) for k in ("lds_tree", "wavefront", "wf_resident_max")}

    def render(sb, cam, p, after_upload=None):
        out = {}
        for form, modes in FORMS.items():
            ctx.set_tunable("lds_tree", 0 if form == "l1_nodes" else 1)
            ctx.set_tunable("wavefront", 1 if form == "wavefront" else 0)
            ctx.set_tunable("wf_resident_max", 0)
            ctx.upload_scene(sb)
            ctx.set_camera(cam)
            if after_upload is not None:
                after_upload()
            out[form] = counted(ctx, copy.copy(p), form)
            assert ctx.launch_info()["lds_tree_mode"] in modes, (form, ctx.launch_info())
        return out

    yield render
    for k, v in saved.items():
        ctx.set_tunable(k, v)


def _cameras(dev, oracle, abi, eye=None, look_at=None, vfov=None):
    cp = abi.default_camera_params()
    if eye is not None:
        cp.eye[:], cp.lookAt[:], cp.vfovDegrees = eye, look_at, vfov
    cams = dev.make_camera(cp), oracle.make_camera(cp)
    assert bytes(cams[0]) == bytes(cams[1])
    return cams


def _check(got, oracle, abi, dev, sb, ocam, p, what):
    """Both kernels against the oracle on `sb` (bits and counters), and so against each other."""
    chunks = dev.plan_spp_chunks(p.imageWidth, p.imageHeight, p.spp, p.sppChunks)
    want = oracle_frame(oracle, oracle.OracleScene(sb), abi, ocam, p, chunks, 8)
    for form in FORMS:
        assert_frame_identical(*got[form], *want, what=(what, form))
    a, b = got["wavefront"], got["l1_nodes"]
    nan = np.isnan(b[0])
    assert np.array_equal(np.isnan(a[0]), nan) and np.array_equal(a[0].view(np.uint32)[~nan], b[0].view(np.uint32)[~nan]), what
    assert [a[2][k] for k in COUNTERS] == [b[2][k] for k in COUNTERS], (what, a[2], b[2])


def _octants(ctx, p, depths=(0, 1, 2)):
    """The direction octants (sign bits of d) of the kernel's own rays that hit something, over the first sample's bounces."""
    seen = set()
    for d in depths:
        rec = ctx.render_aov(p, d)
        hit = (rec["valid"] != 0) & (rec["prim"] >= 0)
        s = (rec["d"][hit] < 0).astype(int)
        seen |= set((s[:, 0] | (s[:, 1] << 1) | (s[:, 2] << 2)).tolist())
    return seen


def test_all_eight_octants(ctx, forms, dev, oracle, abi):
    seed, sb = exact_scenes.random_with_tree(abi, "A")
    # from the middle of the cloud (triangles and spheres within 3 of (0, 3, -1)), wide open: geometry on every side
    cams = _cameras(dev, oracle, abi, eye=(0.1, 3.2, -0.9), look_at=(0.3, 2.5, -3.0), vfov=150.0)
    p = abi.default_render_params(W, H, SPP, BOUNCES, seed=811)
    octants = []
    got = forms(sb, cams[0], p, after_upload=lambda: octants.append(_octants(ctx, p)))
    assert ctx.slab_scene() == (1, 1)
    assert octants[0] == set(range(8)), (seed, sorted(octants[0]))
    _check(got, oracle, abi, dev, sb, cams[1], p, ("octants", seed))


def _flat_scene(abi):
    """Axis-aligned triangles in the planes x = 0, y = 0 and z = 0 (and one at y = 1.25), spheres of radius 0 at the origin
    and on an axis, a few solid ones and the ground: one tree."""
    rng = np.random.default_rng(5)
    sb = abi.SceneBuilder()
    mats = exact_scenes.palette(sb, rng, "A")
    pos = []
    for axis, value in ((0, 0.0), (1, 0.0), (2, 0.0), (1, 1.25), (0, -0.0), (2, 0.0)):
        for _ in range(3):
            tri = rng.uniform(-2.5, 2.5, (3, 3))
            tri[:, axis] = value
            pos.append(tri)
    pos = np.concatenate(pos).astype(F)
    uv = np.zeros((len(pos), 2), F)
    idx = np.arange(len(pos)).reshape(-1, 3)
    sb.add_triangles(pos, uv, idx[:9], mats[1])
    sb.add_triangles(pos, uv, idx[9:], mats[3])
    for c in ((0.0, 0.0, 0.0), (0.0, 2.0, 0.0), (-1.5, 0.0, 0.0)):
        sb.add_sphere(c, 0.0, mats[0])
    sb.add_sphere((1.0, 1.0, -1.0), 0.7, mats[4])
    sb.add_sphere((-1.0, 0.5, 1.0), 0.5, mats[6])
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, mats[2])  # (its top is the plane y = 0 too)
    sb.world_bvh(0, None, 0.0, 1.0)
    return exact_scenes.assert_libm_free(sb, "A")


def test_planes_at_zero_and_flat_boxes(ctx, forms, dev, oracle, abi):
    sb = _flat_scene(abi)
    cams = _cameras(dev, oracle, abi, eye=(3.0, 2.0, 4.0), look_at=(0.0, 0.5, 0.0), vfov=60.0)
    p = abi.default_render_params(W, H, SPP, BOUNCES, seed=812)
    got = forms(sb, cams[0], p)
    assert ctx.slab_scene() == (1, 1)
    nodes = ctx.bvh(0)
    assert (nodes["bmin"] == 0).any() and (nodes["bmax"] == 0).any()        # planes at coordinate 0
    assert (nodes["bmin"] <= nodes["bmax"]).all()
    _check(got, oracle, abi, dev, sb, cams[1], p, "flat")


def test_frame_after_update_and_refit(ctx, forms, dev, oracle, abi):
    """The scene scaled by exactly 2 through srtUpdateTriangles / srtUpdateSpheres + srtRefitScene, camera unchanged: the
    oracle's own build of the scaled scene has the same topology (every comparison of the builder scales along; the
    reference's triangle test depends on the order of the walk), so the frame must be the oracle's."""
    seed, sb = exact_scenes.random_with_tree(abi, "A")
    tri = RF.scene_triangles(sb)
    tri["p"] *= F(2)
    sph = np.zeros(len(sb.spheres), abi.SPHERE_DTYPE)
    moved_spheres = []
    for i, s in enumerate(sb.spheres):
        m = abi.SrtSphereIn(time0=s.time0, time1=s.time1, radius=2.0 * s.radius, material=s.material)
        m.center0[:] = [2.0 * v for v in s.center0]
        m.center1[:] = [2.0 * v for v in s.center1]
        moved_spheres.append(m)
        sph[i] = (tuple(m.center0), tuple(m.center1), m.time0, m.time1, m.radius, m.material)
    cams = _cameras(dev, oracle, abi)
    p = abi.default_render_params(W, H, SPP, BOUNCES, seed=813)
    words = []

    def move():
        ctx.update_triangles(0, tri)
        ctx.update_spheres(0, sph)
        ctx.refit()
        words.append(ctx.slab_scene())

    got = forms(sb, cams[0], p, after_upload=move)
    assert words == [(1, 1), (1, 1)]
    _check(got, oracle, abi, dev, RF.moved_scene(sb, tri, moved_spheres), cams[1], p, ("refit", seed))


def _inverted_scene(abi):
    """A tier-A random scene's geometry as one tree, and a sphere of negative radius as a tree of its own: one node, box
    (c - r, c + r) inverted on every axis."""
    rng = np.random.default_rng(6)
    sb = abi.SceneBuilder()
    mats = exact_scenes.palette(sb, rng, "A")
    n = 12
    pos = (rng.uniform(-3, 3, (n * 3, 3)) + np.array([0, 3, -1])).astype(F)
    sb.add_triangles(pos, np.zeros((n * 3, 2), F), np.arange(n * 3).reshape(-1, 3), mats[1])
    sb.add_sphere((1.0, 1.0, -1.0), 0.8, mats[4])
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, mats[2])
    first = sb.num_prims
    sb.add_sphere((-1.0, 1.5, 0.5), -1.0, mats[0])
    sb.world_bvh(0, first, 0.0, 1.0)
    sb.world_bvh(first, 1, 0.0, 1.0)
    return exact_scenes.assert_libm_free(sb, "A")


def test_inverted_box_leaves_every_ray_to_the_exact_test(ctx, forms, dev, oracle, abi):
    sb = _inverted_scene(abi)
    cams = _cameras(dev, oracle, abi)
    p = abi.default_render_params(W, H, SPP, BOUNCES, seed=814)
    words = []
    got = forms(sb, cams[0], p, after_upload=lambda: words.append(ctx.slab_scene()))
    assert words == [(1, 0), (1, 0)]  # the ranges hold; the order does not
    box = ctx.bvh(1)
    assert len(box) == 1 and (box["bmin"] > box["bmax"]).all()
    _check(got, oracle, abi, dev, sb, cams[1], p, "inverted")
    assert got["wavefront"][2]["sphereTests"] > 0
    # the radius made positive and a refit: the device pass finds every box ordered again
    sph = np.zeros(1, abi.SPHERE_DTYPE)
    s = sb.spheres[-1]
    sph[0] = (tuple(s.center0), tuple(s.center1), s.time0, s.time1, 1.0, s.material)
    ctx.update_spheres(len(sb.spheres) - 1, sph)
    ctx.refit()
    assert ctx.slab_scene() == (1, 1)
