"""The regrouped tree on the device (csrc/srt_regroup.h, csrc/srt_wavefront.hip; tunable "wf_regroup"): the whole-tree form
of the path-pool kernel walks other inner nodes over the reference's leaves, and nothing a frame holds may move by a bit.

  * frames: the masterchief scene at 64 x 48, 4 spp, 4 bounces; a ground sphere and a mesh of 256-600 nodes at 96 x 64, 8 spp;
    a world of two trees and a bare primitive; a room of axis-aligned quads.  wf_regroup 1 against 0 against the step
    scheduler over the LDS-resident tree: accumulators bit-identical, through the production, the moments and the
    profiling instance;
  * the LDS copy IS the regrouped tree: the profiling instance's node visits fall to well under three quarters;
  * counters: a counting launch's eight counters with wf_regroup 1 are those with 0 (the counting instances walk the
    reference tree) and, on the libm-free version of the mesh scene, the oracle's;
  * refit: after srtUpdateTriangles + srtUpdateSpheres + srtRefitScene the regrouped array holds the reference leaves' new
    boxes under unions of them, and the frame is the wf_regroup 0 frame.

No ray of these frames has a direction component of exactly +-0 (the quad room's quads are axis-aligned, its rays are not), so
none reaches the gate form of the exact test: tests/test_gpu_planar_frames.py renders frames made of such rays alone and
pins the regrouped walk's node visits to a replay of the closed gate."""
import numpy as np
import pytest

import exact_scenes as X

pytestmark = pytest.mark.gpu

F = np.float32
TUNABLES = ("lds_tree", "wavefront", "wf_resident_max", "wf_regroup", "wf_profile")
COUNTERS = ("samples", "rays", "nodeVisits", "boxPasses", "triTests", "sphereTests", "shadedTriHits", "texelFetches")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture
def forms(ctx):
    """The tunables the parity tests use to force the forms: every tree that fits goes to LDS and, with wavefront = 1, to the
    path-pool kernel's whole-tree form.  Read at upload (wf_resident_max) and at launch (the others)."""
    saved = {k: ctx.get_tunable(k) for k in TUNABLES}
    for k, v in zip(TUNABLES, (1, 1, 0, 1, 0)):
        ctx.set_tunable(k, v)
    yield ctx
    for k, v in saved.items():
        ctx.set_tunable(k, v)


def _soup_mesh(srt):
    """400 visible triangles and the ground sphere of radius 1000 in one tree."""
    return srt.scenes.scene_soup(400, seed=11, extent=3.0, size=0.5)


def _two_trees(srt):
    sb = srt.scenes.scene_soup(300, seed=12, extent=3.0, size=0.5)
    sb.world = []
    sb.world_bvh(0, 150, 0.0, 1.0)
    sb.world_prim(150)
    sb.world_bvh(151, sb.num_prims - 151, 0.0, 1.0)
    return sb


def _quad_room(abi):
    """Axis-aligned quads (two triangles each: every leaf box is flat on one axis before its padding) around three spheres."""
    sb = abi.SceneBuilder()
    rng = np.random.default_rng(4)
    wall = sb.metal((0.8, 0.7, 0.6), 0.3)
    pos, idx = [], []
    for k in range(60):
        axis = k % 3
        u, v = (axis + 1) % 3, (axis + 2) % 3
        c = rng.uniform(-3, 3, 3) + np.array([0.0, 3.0, -2.0])
        c[axis] = float(np.round(c[axis] * 2) / 2)  # planes on a half-integer grid: shared by many quads
        h = rng.uniform(0.3, 1.2, 2)
        q = np.repeat(c[None, :], 4, axis=0)
        q[:, u] += np.array([-h[0], h[0], h[0], -h[0]])
        q[:, v] += np.array([-h[1], -h[1], h[1], h[1]])
        base = len(pos)
        pos += list(q)
        idx += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
    pos = np.array(pos, F)
    sb.add_triangles(pos, np.zeros((len(pos), 2), F), np.array(idx), wall)
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.metal((0.5, 0.5, 0.5), 0.6))
    sb.add_sphere((0.0, 1.0, 0.0), 1.0, sb.dielectric(1.5))
    sb.add_sphere((-7.0, 4.0, 6.0), 1.0, sb.light((25.0, 22.0, 11.0)))
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


SCENES = {
    "masterchief": (lambda srt, abi: srt.scenes.scene_masterchief(), (64, 48, 4, 4)),
    "soup_mesh": (lambda srt, abi: _soup_mesh(srt), (96, 64, 8, 4)),
    "two_trees": (lambda srt, abi: _two_trees(srt), (64, 48, 4, 4)),
    "quad_room": (lambda srt, abi: _quad_room(abi), (64, 48, 4, 4)),
}


def _render(ctx, p, regroup, moments=False, profile=False, form=3):
    ctx.set_tunable("wf_regroup", regroup)
    ctx.set_tunable("wf_profile", 1 if profile else 0)
    out = ctx.render_image_moments(p) if moments else ctx.render_image(p)
    ctx.last_kernel_ms()  # (waits, and raises if a workgroup gave up)
    assert ctx.launch_info()["lds_tree_mode"] == form, ctx.launch_info()
    ctx.set_tunable("wf_profile", 0)
    return out


def _node_visits(ctx):
    return ctx.wf_profile()["node"]["lanes"]


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_frames_are_bit_identical(forms, srt, abi, camera, scene):
    ctx = forms
    make, (w, h, spp, bounces) = SCENES[scene]
    ctx.upload_scene(make(srt, abi))
    ctx.set_camera(camera)
    rg = ctx.regroup()
    assert rg is not None, "the upload built no regrouped tree"
    if scene == "soup_mesh":
        assert 256 <= len(rg[0]) <= 600, len(rg[0])
    p = abi.default_render_params(w, h, spp, bounces, seed=9)
    on = _render(ctx, p, 1)
    off = _render(ctx, p, 0)
    ctx.set_tunable("wavefront", 0)
    step = ctx.render_image(p)
    assert ctx.launch_info()["lds_tree_mode"] in (1, 2), ctx.launch_info()
    step_m = ctx.render_image_moments(p)
    ctx.set_tunable("wavefront", 1)
    assert np.isfinite(np.asarray(step[0])[..., :3]).any() and np.asarray(step[0])[..., :3].max() > 0
    for a, b, c in zip(on, off, step):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    # the moments instance, and the profiling instance (whose LDS copy must be the regrouped tree as well)
    for got in (_render(ctx, p, 1, moments=True), _render(ctx, p, 0, moments=True)):
        for a, c in zip(got, step_m):
            assert a.tobytes() == c.tobytes()
    prof_on = _render(ctx, p, 1, profile=True)
    visits_on = _node_visits(ctx)
    prof_off = _render(ctx, p, 0, profile=True)
    visits_off = _node_visits(ctx)
    assert prof_on[0].tobytes() == prof_off[0].tobytes() == step[0].tobytes()
    print("%s: node visits of the frame, reference tree %d, regrouped %d (ratio %.2f)" % (scene, visits_off, visits_on, visits_on / visits_off))
    assert 0 < visits_on < visits_off
    if scene == "masterchief":
        assert visits_on < 0.75 * visits_off  # (the host replay of these rays: 0.50-0.58)


def test_counters_are_the_reference_walks(forms, srt, abi, oracle, camera):
    ctx = forms
    sb = X.mesh(srt, abi, "A")
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    assert ctx.regroup() is not None
    p = abi.default_render_params(64, 48, 4, 4, seed=9)
    plain = _render(ctx, p, 1)[0]
    p.countStats = 1
    stats = {}
    for regroup in (1, 0):
        acc = _render(ctx, p, regroup)[0]
        assert acc.tobytes() == plain.tobytes()
        stats[regroup] = ctx.stats()
    want_acc, _, want = oracle.OracleScene(sb).render(camera, p, oracle.RNG_COUNTER, threads=8, want_rgba=False)
    assert _bits(plain).tobytes() == _bits(want_acc).tobytes()
    for k in COUNTERS:
        assert stats[1][k] == stats[0][k] == want[k], (k, stats[1][k], stats[0][k], want[k])
    assert want["nodeVisits"] > 40 * want["rays"]  # the reference walk's count, not the regrouped tree's


def _leaves(nodes8):
    """Leaf records of a flattened array in pre-order (two primitive children)."""
    refs = nodes8.view(np.int32)
    return nodes8[(refs[:, 3] < 0) & (refs[:, 7] < 0)]


def test_refit_keeps_the_regrouped_tree_valid(forms, srt, abi, camera):
    ctx = forms
    sb = _soup_mesh(srt)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    before, links = ctx.regroup()
    rng = np.random.default_rng(3)
    tri = np.concatenate(sb.triangles).copy()
    tri["p"] += rng.normal(0, 0.25, tri["p"].shape).astype(F)
    ctx.update_triangles(0, tri)
    ctx.refit()
    after, links_after = ctx.regroup()
    refs = after.view(np.int32)
    assert np.array_equal(links, links_after) and np.array_equal(before.view(np.int32)[:, [3, 7]], refs[:, [3, 7]])  # topology stays
    assert not np.array_equal(_bits(before), _bits(after))
    # leaf boxes: the reference tree's leaves after its own refit, in order (pre-order leaves of both arrays)
    ref_nodes = ctx.bvh(0)
    ref_leaf = (ref_nodes["left"] < 0) & (ref_nodes["right"] < 0)
    lv = _leaves(after)
    assert np.array_equal(_bits(lv[:, 0:3]), _bits(ref_nodes["bmin"][ref_leaf])) and np.array_equal(_bits(lv[:, 4:7]), _bits(ref_nodes["bmax"][ref_leaf]))
    # inner boxes: the union of the two children's
    inner = np.flatnonzero(refs[:, 3] >= 0)
    l, r = refs[inner, 3] >> 5, refs[inner, 7] >> 5
    assert np.array_equal(_bits(after[inner, 0:3]), _bits(np.minimum(after[l, 0:3], after[r, 0:3])))
    assert np.array_equal(_bits(after[inner, 4:7]), _bits(np.maximum(after[l, 4:7], after[r, 4:7])))
    p = abi.default_render_params(96, 64, 8, 4, seed=9)
    on = _render(ctx, p, 1, profile=True)
    visits_on = _node_visits(ctx)
    off = _render(ctx, p, 0, profile=True)
    assert 0 < visits_on < _node_visits(ctx)  # (still the regrouped tree that is walked)
    assert on[0].tobytes() == off[0].tobytes()
    ctx.set_tunable("wavefront", 0)
    step = ctx.render_image(p)
    ctx.set_tunable("wavefront", 1)
    assert on[0].tobytes() == step[0].tobytes()
