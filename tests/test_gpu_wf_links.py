"""The path-pool kernel's whole-tree form over its LDS link words (csrc/srt_wf_links.h: node = LDS byte offset, leaf = one
word holding both objects, link = the successor alone), on the GPU.  For each scene, with tunable wavefront = 1:
  * the accumulators are equal as uint32 to the same context's render with wavefront = 0 (the step-scheduler kernel over
    the same tree, which walks DevScene::nodeThread's 16-bit links);
  * the srtRenderAov records of the counting instance (primitive, the bits of t, node visits, box passes, triangle and
    sphere tests) are equal to the oracle's world.hit() on the same rays, ray by ray.
Scenes: the three-sphere scene (a tree of a few nodes); a seeded triangle soup with the ground whose tree has node indices
beyond 2048 (record byte offsets beyond 16 bits) and still fits a CU's LDS; the headline mesh; a world of two trees and a
bare primitive with a triangle + sphere leaf and a sphere + triangle leaf.  One case through srtRenderTilesMoments."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 64, 48, 4, 4
# the reference builder (bvh.h:55-95) halves a span down to one or two objects: 1025..2048 primitives make 2047 nodes, and
# 2048 + k make 2047 + 2 k.  2101 primitives (2100 triangles and the ground): 2153 nodes, indices up to 2152.
SOUP_TRIANGLES = 2100


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def two_root_world(abi):
    """Two trees and a bare primitive.  The second tree is one leaf of a triangle and a sphere; the first has the ground, two
    spheres, four triangles and ends (bvh.h's sort along a random axis decides the order inside a leaf) in leaves of
    two triangles or of a sphere and a triangle."""
    sb = abi.SceneBuilder()
    grey = sb.pbr(albedo_tex=sb.solid(150, 140, 120), metalness=0.0, roughness=0.4)
    red = sb.pbr(albedo_tex=sb.solid(200, 60, 50), metalness=0.2, roughness=0.6)
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.pbr(albedo_tex=sb.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))))
    sb.add_sphere((-2.0, 1.0, 0.5), 1.0, sb.metal((0.7, 0.6, 0.5), 0.1))
    sb.add_sphere((4.0, 0.7, 1.5), 0.7, sb.dielectric(1.5))
    pos = np.array([[-1, 0, -2], [1, 0, -2], [0, 2.5, -2], [1, 0, -2], [3, 0, -2.5], [2, 2, -2], [0.5, 0, 2.5], [2, 0, 2], [1.2, 1.5, 2.2],
                    [5, 0, -1], [6, 0, 0], [5.5, 2, -0.5]], np.float32)
    uv = np.tile(np.array([[0, 0], [1, 0], [0.5, 1]], np.float32), (4, 1))
    sb.add_triangles(pos, uv, np.arange(12).reshape(-1, 3), grey)
    first_tree = sb.num_prims
    sb.add_triangles(np.array([[1.5, 0, 0.5], [3.0, 0, 0.2], [2.2, 2.2, 0.4]], np.float32), uv[:3], np.arange(3).reshape(-1, 3), red)
    sb.add_sphere((2.2, 0.8, 1.2), 0.8, red)
    sb.add_sphere((7.0, 4.0, 5.0), 1.0, sb.light((20.0, 18.0, 12.0)))
    sb.world_bvh(0, first_tree, 0.0, 1.0)
    sb.world_bvh(first_tree, 2, 0.0, 1.0)
    sb.world_prim(sb.num_prims - 1)
    return sb


def _scene(srt, abi, name):
    if name == "spheres":
        return srt.scenes.scene_spheres(), (W, H)
    if name == "soup":
        return srt.scenes.scene_soup(SOUP_TRIANGLES, seed=21, extent=5.0, size=0.5), (W, H)
    if name == "masterchief":
        return srt.scenes.scene_masterchief(), (64, 36)
    return two_root_world(abi), (W, H)


@pytest.fixture
def whole_tree_form(ctx):
    """wavefront = 1, lds_tree = 1: the path-pool kernel for every tree that fits, however small.  Restored afterwards."""
    saved = {k: ctx.get_tunable(k) for k in ("lds_tree", "wavefront", "wf_resident_max")}
    ctx.set_tunable("lds_tree", 1)
    ctx.set_tunable("wavefront", 1)
    ctx.set_tunable("wf_resident_max", 0)
    yield ctx
    for k, v in saved.items():
        ctx.set_tunable(k, v)


def _check_shape(ctx, sb, name):
    """The scene is the case its name says."""
    if name == "two_roots":
        trees = [ctx.bvh(0), ctx.bvh(1)]
        assert len(trees[1]) == 1
        kind = np.concatenate(sb._prim_chunks)[:, 0]  # per entry of the prims list: SRT_PRIM_TRIANGLE / SRT_PRIM_SPHERE
        for n in trees:  # every tree has a leaf of a triangle with a sphere
            leaves = n[n["left"] < 0]
            assert any(kind[~int(l)] != kind[~int(r)] for l, r in zip(leaves["left"], leaves["right"]))
        return
    nodes = ctx.bvh(0)
    if name == "soup":
        assert 2048 < len(nodes) <= (160 * 1024 - 256 - 18 * 1024) // 32, len(nodes)
    elif name == "spheres":
        assert len(nodes) <= 8
    else:
        assert len(nodes) > 4000


@pytest.mark.parametrize("name", ["spheres", "soup", "masterchief", "two_roots"])
def test_link_words_render_and_walk(whole_tree_form, oracle, abi, srt, camera, name):
    ctx = whole_tree_form
    sb, (w, h) = _scene(srt, abi, name)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    _check_shape(ctx, sb, name)
    p = abi.default_render_params(w, h, SPP, BOUNCES, seed=9)
    acc, _ = ctx.render_image(p)
    info = ctx.launch_info()
    assert info["lds_tree_mode"] == 3, info  # the whole-tree form of the path-pool kernel
    ctx.set_tunable("wavefront", 0)
    want, _ = ctx.render_image(p)
    assert ctx.launch_info()["lds_tree_mode"] in (1, 2), ctx.launch_info()
    ctx.set_tunable("wavefront", 1)
    assert np.array_equal(_bits(acc), _bits(want)), np.argwhere((_bits(acc) != _bits(want)).any(axis=-1))[:4].tolist()
    # the counting instance's walks, ray by ray (as test_render_kernel_traversal_per_ray_vs_oracle compares them)
    osc = oracle.OracleScene(sb)
    p1 = abi.default_render_params(w, h, 1, BOUNCES, seed=9)
    seen = 0
    for depth in range(3):
        rec = ctx.render_aov(p1, depth).reshape(-1)
        assert ctx.launch_info()["lds_tree_mode"] == 3
        rec = rec[rec["valid"] == 1]
        assert len(rec) >= (w * h if depth == 0 else 20), (name, depth, len(rec))
        rays = np.zeros(len(rec), abi.RAY_DTYPE)
        rays["o"], rays["d"], rays["time"] = rec["o"], rec["d"], rec["time"]
        rays["tMin"], rays["tMax"] = 0.001, np.inf
        hit = osc.trace(rays)
        assert np.array_equal(rec["prim"], hit["prim"]), (name, depth)
        m = hit["prim"] >= 0
        assert np.array_equal(_bits(rec["t"][m]), _bits(hit["t"][m])), (name, depth)
        for f in ("nodeVisits", "boxPasses", "triTests", "sphereTests"):
            bad = np.flatnonzero(rec[f] != hit[f])
            assert len(bad) == 0, (name, depth, f, len(bad), rec[f][bad[:4]], hit[f][bad[:4]])
        seen += len(rec)
    assert seen > 1.2 * w * h
    if name == "two_roots":  # the walks reached both kinds of object of the mixed leaf
        assert rec["sphereTests"].max() >= 2 and rec["triTests"].max() >= 2


def test_link_words_through_the_moments_instance(whole_tree_form, abi, srt, camera):
    """srtRenderImageMoments (srtRenderTilesMoments underneath) runs the MOMENTS instance of the same form: sums and moments
    equal as uint32 to the step-scheduler kernel's."""
    ctx = whole_tree_form
    sb, (w, h) = _scene(srt, abi, "two_roots")
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(w, h, SPP, BOUNCES, seed=4)
    acc, mom, _ = ctx.render_image_moments(p)
    assert ctx.launch_info()["lds_tree_mode"] == 3, ctx.launch_info()
    plain, _ = ctx.render_image(p)
    ctx.set_tunable("wavefront", 0)
    want_acc, want_mom, _ = ctx.render_image_moments(p)
    assert ctx.launch_info()["lds_tree_mode"] in (1, 2)
    ctx.set_tunable("wavefront", 1)
    assert np.array_equal(_bits(acc), _bits(want_acc)) and np.array_equal(_bits(acc), _bits(plain))
    assert np.array_equal(_bits(mom), _bits(want_mom))
    assert (mom[..., 3] == SPP).all()
