"""Geometry updates in place and the device refit (include/srt_hip.h srtUpdateTriangles / srtUpdateSpheres /
srtRefitScene; csrc/srt_refit.hip) on bits: the refit boxes and pair records against the NumPy replay tests/refit_ref.py,
the rewritten primitive records against the oracle built on the MOVED scene, FAITHFUL renders against the oracle and
against a fresh upload of the moved scene with caller-supplied nodes (code from before the refit existed), on every form
of the render kernel.  No tolerances.  Images are 64 x 40 at 4 samples and 4 bounces."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import records_cases as RC
import refit_ref as RF
import tree_build_ref as R
import tree_build_scenes as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, BOUNCES = 64, 40, 4, 4


def _params(abi, traversal=None, seed=5):
    return abi.default_render_params(W, H, SPP, BOUNCES, seed=seed, traversal=abi.SRT_TRAVERSE_FAITHFUL if traversal is None else traversal)


def _sphere_array(abi, sb):
    a = np.zeros(len(sb.spheres), abi.SPHERE_DTYPE)
    for i, s in enumerate(sb.spheres):
        a[i] = (tuple(s.center0), tuple(s.center1), s.time0, s.time1, s.radius, s.material)
    return a


def _sphere_list(abi, a):
    out = []
    for r in a:
        s = abi.SrtSphereIn(time0=r["time0"], time1=r["time1"], radius=r["radius"], material=int(r["material"]))
        s.center0[:] = r["center0"].tolist()
        s.center1[:] = r["center1"].tolist()
        out.append(s)
    return out


def _geometry(abi, sb):
    return RF.scene_triangles(sb) if sb.triangles else np.zeros(0, abi.TRIANGLE_DTYPE), _sphere_array(abi, sb)


def _moved(abi, sb, tri, sph):
    return RF.moved_scene(sb, tri if len(tri) else None, _sphere_list(abi, sph))


def _displaced(abi, sb, amount, seed=3):
    """Every vertex and every sphere centre moved by a random vector of about `amount`; a moving sphere stays moving, a
    static one static; radii change a little.  The materials written into the records are WRONG on purpose: ignored."""
    rng = np.random.default_rng(seed)
    tri, sph = _geometry(abi, sb)
    tri["p"] += rng.normal(0, amount, tri["p"].shape).astype(F)
    d = rng.normal(0, amount, (len(sph), 3)).astype(F)
    moving = (sph["center0"] != sph["center1"]).any(axis=1)
    sph["center0"] += d
    sph["center1"] += np.where(moving[:, None], rng.normal(0, amount, (len(sph), 3)).astype(F), d)
    sph["radius"] *= np.where(sph["radius"] < 10, F(1.0) + F(0.1) * rng.random(len(sph), dtype=F), F(1.0))  # (not the ground)
    sent_tri, sent_sph = tri.copy(), sph.copy()
    sent_tri["material"] = 12345
    sent_sph["material"] = -7
    return tri, sph, sent_tri, sent_sph


def _update_all(ctx, tri, sph):
    if len(tri):
        ctx.update_triangles(0, tri)
    if len(sph):
        ctx.update_spheres(0, sph)
    ctx.refit()


def _trees(ctx, sb):
    return [ctx.bvh(w) if it.kind == R.WORLD_BVH else None for w, it in enumerate(sb.world)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_trees(ctx, want_nodes, want_pairs, axis_before=None):
    for w, want in enumerate(want_nodes):
        if want is None:
            continue
        got = ctx.bvh(w)
        assert np.array_equal(got["left"], want["left"]) and np.array_equal(got["right"], want["right"]), w
        assert np.array_equal(_bits(got["bmin"]), _bits(want["bmin"])) and np.array_equal(_bits(got["bmax"]), _bits(want["bmax"])), w
        axis, pairs = ctx.tree_aux(w)
        assert np.array_equal(_bits(pairs), _bits(want_pairs[w])), w
        if axis_before is not None:
            assert np.array_equal(axis, axis_before[w]), w


def _spheres_one_moving(srt):
    sb = srt.scenes.scene_spheres()
    sb.spheres[2].center1[:] = (0.5, 1.25, -0.5)
    return sb


def _soup(srt, builder=0):
    """300 triangles large enough to be seen, and the ground sphere: 300 nodes, past the forced-hybrid limit of 24; the
    upload reorders the triangles of a host-built tree."""
    return srt.scenes.scene_soup(300, seed=11, extent=3.0, size=0.5, builder=builder)


# ------------------------------------------------------------------------------------------------ identity
@pytest.mark.parametrize("scene", ["spheres", "soup"])
def test_identity_update_changes_nothing(ctx, srt, abi, camera, node_path, scene):
    sb = _spheres_one_moving(srt) if scene == "spheres" else _soup(srt)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = _params(abi)
    before = ctx.render_image(p)[0]
    form = ctx.launch_info()["lds_tree_mode"]
    if scene == "soup":
        assert (form == 4) == (node_path == "hybrid")  # past the forced-hybrid limit of 24 nodes
    nodes, depth, aux = _trees(ctx, sb), ctx.bvh_depth(), ctx.tree_aux(0)
    tri, sph = _geometry(abi, sb)
    _update_all(ctx, tri, sph)
    assert ctx.bvh(0).tobytes() == nodes[0].tobytes() and ctx.bvh_depth() == depth
    axis, pairs = ctx.tree_aux(0)
    assert axis.tobytes() == aux[0].tobytes() and pairs.tobytes() == aux[1].tobytes()
    after = ctx.render_image(p)[0]
    assert ctx.launch_info()["lds_tree_mode"] == form
    assert after.tobytes() == before.tobytes()


# ------------------------------------------------------------------------------------------------ boxes
def _world_scene(abi, kind):
    if kind == "four_items":
        return S.four_items(abi)
    return S.soup(abi, 300, {"host": abi.SRT_BUILDER_REFERENCE, "lbvh": abi.SRT_BUILDER_LBVH, "ploc": abi.SRT_BUILDER_PLOC}[kind])


@pytest.mark.parametrize("kind", ["host", "lbvh", "ploc", "four_items"])
def test_refit_boxes_and_pair_records_match_replay(ctx, abi, kind):
    """Triangles, static and moving spheres under a random displacement: host-built, linear-BVH and PLOC trees, and a
    world of one of each (own bases, own times, renumbered triangles) with a lone primitive."""
    sb = _world_scene(abi, kind)
    ctx.upload_scene(sb)
    nodes = _trees(ctx, sb)
    axis = [None if n is None else ctx.tree_aux(w)[0] for w, n in enumerate(nodes)]
    depth = ctx.bvh_depth()
    tri, sph, sent_tri, sent_sph = _displaced(abi, sb, 0.4)
    _update_all(ctx, sent_tri, sent_sph)
    moved = _moved(abi, sb, tri, sph)
    want = RF.refit_world(moved, nodes)
    assert any(w is not None and w.tobytes() != n.tobytes() for w, n in zip(want, nodes))
    _assert_trees(ctx, want, RF.pair_records_world(moved, want), axis)
    assert ctx.bvh_depth() == depth


# ------------------------------------------------------------------------------------------------ records
HIT_FIELDS = ("prim", "t", "p", "normal", "tangent", "bitangent", "frontFace")


@pytest.mark.parametrize("builder", ["host", "lbvh", "ploc"])
def test_updated_records_trace_like_the_oracle_on_the_moved_scene(ctx, oracle, srt, abi, builder):
    """Independent of the tree: the closest hit of a fixed ray set, every field of the hit record on bits, against the
    oracle's brute force over the moved scene (random uvs: the tangent basis; triangles reordered at upload).  uv on bits
    where it is arithmetic on the records (triangles); a sphere's uv goes through acosf / atan2f in the trace kernel, where
    device libm and glibc differ by an ulp whatever the records hold: tests/test_gpu_parity.py's bar for it, 1e-6."""
    sb = _soup(srt, {"host": 0, "lbvh": abi.SRT_BUILDER_LBVH, "ploc": abi.SRT_BUILDER_PLOC}[builder])
    ctx.upload_scene(sb)
    tri, sph, sent_tri, sent_sph = _displaced(abi, sb, 0.3)
    _update_all(ctx, sent_tri, sent_sph)
    rays = S.random_rays(abi, with_time=False)
    got = ctx.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    want = oracle.OracleScene(_moved(abi, sb, tri, sph)).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    hit = want["prim"] >= 0
    assert hit.mean() > 0.2 and (want["prim"][hit] < 300).mean() > 0.05  # triangles among them
    for f in HIT_FIELDS:
        assert np.array_equal(_bits(got[f][hit]), _bits(want[f][hit])), f
    assert np.array_equal(got["prim"], want["prim"])
    on_tri, on_sph = hit & (want["prim"] < 300), want["prim"] == 300
    print("uv words that differ: %d on triangles, %d on the sphere" % (
        (_bits(got["uv"][on_tri]) != _bits(want["uv"][on_tri])).sum(), (_bits(got["uv"][on_sph]) != _bits(want["uv"][on_sph])).sum()))
    assert np.array_equal(_bits(got["uv"][on_tri]), _bits(want["uv"][on_tri]))
    assert np.abs(got["uv"][on_sph].astype(np.float64) - want["uv"][on_sph]).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ edge cases
EDGE_HIT_FIELDS = HIT_FIELDS + ("uv", "material")


@pytest.mark.parametrize("builder", ["host", "lbvh", "ploc"])
def test_edge_case_records_and_boxes_are_an_uploads(ctx, dev, abi, builder):
    """tests/records_cases.py as one world item: uploaded scaled by exactly 2 with every zero made +0 (same topology: every
    box minimum and centroid doubles, but no record, box or zero sign is the one wanted), updated to the edge cases and
    refitted, against a fresh context that uploads the edge cases.  Trees, pair records (they hold the primitives' own
    boxes) and the closest hits of one ray per primitive on bits, the signs of zeros included."""
    tri, sph = RC.geometry(abi)
    which = {"host": abi.SRT_BUILDER_REFERENCE, "lbvh": abi.SRT_BUILDER_LBVH, "ploc": abi.SRT_BUILDER_PLOC}[builder]
    far_tri, far_sph = tri.copy(), sph.copy()
    far_tri["p"] = far_tri["p"] * F(2) + F(0)
    for f in ("center0", "center1", "radius"):
        far_sph[f] = far_sph[f] * F(2) + F(0)
    neg_zero = lambda v: ((v == 0) & np.signbit(v)).any()
    assert not neg_zero(far_tri["p"]) and neg_zero(tri["p"])
    edge = RC.scene(abi, tri, sph, which)
    ctx.upload_scene(RC.scene(abi, far_tri, far_sph, which))
    stale = ctx.bvh(0)
    sent_tri, sent_sph = tri.copy(), sph.copy()
    sent_tri["material"], sent_sph["material"] = 12345, -7  # ignored
    _update_all(ctx, sent_tri, sent_sph)
    rays = RC.rays(abi, tri, sph)
    got_nodes, (got_axis, got_pairs), got = ctx.bvh(0), ctx.tree_aux(0), ctx.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    fresh = dev.Context(0)
    try:
        fresh.upload_scene(edge)
        want_nodes, (want_axis, want_pairs), want = fresh.bvh(0), fresh.tree_aux(0), fresh.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    finally:
        fresh.close()
    assert stale.tobytes() != want_nodes.tobytes()
    assert got_nodes.tobytes() == want_nodes.tobytes()
    assert got_axis.tobytes() == want_axis.tobytes() and got_pairs.tobytes() == want_pairs.tobytes()
    # every primitive with an area is met by its own ray (list order: the triangles, then the spheres)
    no_area = [4, 5]
    assert [int(p) for p in want["prim"]] == [-1 if i in no_area else i for i in range(len(rays))]
    for f in EDGE_HIT_FIELDS:
        assert np.array_equal(_bits(got[f]), _bits(want[f])), f
    # the zero rule reached the device: the root's minimum is +0 on x (triangle 2 alone) and -0 on y (triangle 3 alone)
    assert _bits(got_nodes["bmin"][0, :2]).tolist() == [0x00000000, 0x80000000]
    if builder == "host":
        built = dev.build_bvh_host(edge)[0]
        assert got_nodes.tobytes() == built.tobytes()


# ------------------------------------------------------------------------------------------------ FAITHFUL renders
def test_scaled_scene_renders_like_the_oracle(ctx, oracle, srt, abi, camera, node_path):
    """The soup scaled by exactly 2 through update + refit, camera unchanged: the oracle's own build of the scaled scene
    has the same topology (tests/test_refit_ref.py), so the FAITHFUL render must be the oracle's, and a fresh upload's."""
    sb = _soup(srt)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    tri, sph = _geometry(abi, sb)
    tri["p"] *= F(2)
    for f in ("center0", "center1", "radius"):
        sph[f] *= F(2)
    _update_all(ctx, tri, sph)
    p = _params(abi)
    got = ctx.render_image(p)[0]
    moved = _moved(abi, sb, tri, sph)
    want = oracle.OracleScene(moved).render(camera, p, oracle.RNG_COUNTER, threads=8, want_rgba=False, want_stats=False)[0]
    same = (_bits(got) == _bits(want)).all(axis=-1)
    print("pixels equal to the oracle's on bits: %d of %d" % (same.sum(), same.size))
    ctx.upload_scene(moved)
    fresh = ctx.render_image(p)[0]
    assert got.tobytes() == fresh.tobytes()
    assert same.all()


def _prebuilt(abi, sb, nodes):
    """`sb` with its one world item's tree supplied by the caller."""
    out = RF.moved_scene(sb)
    it = sb.world[0]
    out.world = []
    out.world_prebuilt(nodes, it.first, it.count, it.time0, it.time1)
    return out


@pytest.mark.parametrize("scene", ["spheres", "soup"])
def test_general_motion_renders_like_a_fresh_upload_with_the_refit_tree(ctx, srt, abi, camera, node_path, scene):
    sb = _spheres_one_moving(srt) if scene == "spheres" else _soup(srt)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    nodes = ctx.bvh(0)
    tri, sph, sent_tri, sent_sph = _displaced(abi, sb, 0.25)
    _update_all(ctx, sent_tri, sent_sph)
    p = _params(abi)
    got = ctx.render_image(p)[0]
    form = ctx.launch_info()["lds_tree_mode"]
    moved = _moved(abi, sb, tri, sph)
    it = sb.world[0]
    ctx.upload_scene(_prebuilt(abi, moved, RF.refit(moved, nodes, it.time0, it.time1)))
    want = ctx.render_image(p)[0]
    assert ctx.launch_info()["lds_tree_mode"] == form
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ partial updates
def test_two_ranges_and_a_device_tensor(ctx, srt, abi):
    import torch
    sb = _soup(srt)
    ctx.upload_scene(sb)
    nodes = _trees(ctx, sb)
    tri, sph, sent_tri, _ = _displaced(abi, sb, 0.3)
    orig = RF.scene_triangles(sb)
    ctx.update_triangles(10, sent_tri[10:57])             # host records
    dev = torch.from_numpy(sent_tri[120:300].copy().view(np.uint8).reshape(-1, 64)).cuda()
    ctx.update_triangles(120, dev)                        # device records, asynchronous on the null stream
    ctx.update_triangles(0, sent_tri[:0])                 # count == 0: a no-op
    ctx.refit()
    tri[:10], tri[57:120] = orig[:10], orig[57:120]
    moved = RF.moved_scene(sb, tri)
    want = RF.refit_world(moved, nodes)
    _assert_trees(ctx, want, RF.pair_records_world(moved, want))


def test_caller_built_tree_with_a_mixed_node(ctx, oracle, abi):
    """Node 0 = (node 1, sphere 3): one node child and one primitive child; node 1 = (node 2, node 3); node 2 = (triangle 0,
    triangle 1); node 3 = a single-object leaf over triangle 2.  A shape no median split builds."""
    sb = abi.SceneBuilder()
    m = sb.metal((0.7, 0.6, 0.5), 0.0)
    rng = np.random.default_rng(8)
    v = (rng.random((3, 3, 3), dtype=F) - F(0.5)) * F(3) + np.array([0, 2.5, -2], F)
    sb.add_triangles(v.reshape(-1, 3), rng.random((9, 2), dtype=F), np.arange(9).reshape(-1, 3), m)
    sb.add_sphere((1.0, 2.0, -3.0), 0.7, m, center1=(1.5, 2.0, -3.0))
    nodes = np.zeros(4, abi.NODE_DTYPE)
    nodes["left"] = [1, 2, ~0, ~2]
    nodes["right"] = [~3, 3, ~1, ~2]
    sb.world_bvh(0, 4, 0.0, 1.0)                          # (only its times are read by the replay)
    boxed = RF.refit(sb, nodes, 0.0, 1.0)                 # a consistent tree to upload
    sb.world = []
    sb.world_prebuilt(boxed, 0, 4, 0.0, 1.0)
    ctx.upload_scene(sb)
    tri, sph, sent_tri, sent_sph = _displaced(abi, sb, 0.5)
    _update_all(ctx, sent_tri, sent_sph)
    moved = _moved(abi, sb, tri, sph)
    want = [RF.refit(moved, boxed, 0.0, 1.0)]
    _assert_trees(ctx, want, RF.pair_records_world(moved, want))
    rays = S.random_rays(abi, count=2000, with_time=True)
    got = ctx.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    ref = oracle.OracleScene(moved).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    assert np.array_equal(got["prim"], ref["prim"]) and (ref["prim"] >= 0).mean() > 0.02
    assert np.array_equal(_bits(got["t"]), _bits(ref["t"]))


# ------------------------------------------------------------------------------------------------ certificate
def test_certificate_follows_the_moved_boxes(ctx, srt, abi, camera, node_path):
    """A vertex coordinate at 2^-80 is outside the fast division's operand range: the refit must withdraw the certificate as
    an upload of that scene does, or the two renders part."""
    sb = _soup(srt)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    nodes = ctx.bvh(0)
    tri, sph = _geometry(abi, sb)
    # the lowest corner on x of the whole soup goes to 2^-80: a box minimum from that leaf up to wherever it stays one
    tri["p"][..., 0] += F(7.0)
    k = np.unravel_index(np.argmin(tri["p"][..., 0]), tri["p"].shape[:2])
    tri["p"][k][0] = F(2.0 ** -80)
    sph["center0"][:, 0] += F(1008.0)                     # the ground's box off 0 as well
    sph["center1"][:, 0] += F(1008.0)
    _update_all(ctx, tri, sph)
    moved = _moved(abi, sb, tri, sph)
    it = sb.world[0]
    want_nodes = RF.refit(moved, nodes, it.time0, it.time1)
    assert not RF.fast_div_certified([want_nodes]) and RF.fast_div_certified([nodes])
    p = _params(abi)
    got = ctx.render_image(p)[0]
    ctx.upload_scene(_prebuilt(abi, moved, want_nodes))
    want = ctx.render_image(p)[0]
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ contract
def test_contract(ctx, dev, srt, abi, camera):
    sb = _soup(srt)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    tri, sph = _geometry(abi, sb)
    p = _params(abi)
    first = ctx.render_image(p)[0]
    tunables = {k: ctx.get_tunable(k) for k in ("fast_div", "wavefront", "lds_tree", "wf_resident_max", "ploc_radius")}
    dev.host_random_reset()
    draws = [dev.host_random_float() for _ in range(3)]
    dev.host_random_reset()
    dev.host_random_float()
    # errors: nothing is launched, nothing becomes dirty
    for first_i, arr in ((-1, tri[:4]), (298, tri[:4]), (2 ** 31 - 2, tri[:4])):
        with pytest.raises(dev.SrtError, match="outside"):
            ctx.update_triangles(first_i, arr)
    with pytest.raises(dev.SrtError, match="outside"):
        ctx.update_spheres(1, sph[:1])
    assert dev.lib.srtUpdateTriangles(ctx.h, 0, 4, None) != 0 and b"null" in dev.lib.srtLastError(ctx.h)
    assert dev.lib.srtUpdateSpheresDevice(ctx.h, 0, 1, None, None) != 0
    assert dev.lib.srtUpdateTriangles(ctx.h, 300, 0, None) == 0  # count == 0
    assert ctx.render_image(p)[0].tobytes() == first.tobytes()
    fresh = dev.Context(0)
    try:
        with pytest.raises(dev.SrtError, match="no scene"):
            fresh.update_triangles(0, tri[:1])
        with pytest.raises(dev.SrtError, match="no scene"):
            fresh.refit()
    finally:
        fresh.close()
    # between update and refit nothing traverses the scene; the last render stays the one that is described
    info, ms = ctx.launch_info(), ctx.last_kernel_ms()
    ctx.update_triangles(0, tri)
    rays = S.random_rays(abi, count=16)
    for call in (lambda: ctx.render_image(p), lambda: ctx.render_features(p), lambda: ctx.trace(rays),
                 lambda: ctx.render_temporal_frame(p), lambda: ctx.scatter_test(rays[:1], np.zeros(1, abi.HIT_DTYPE), 1)):
        with pytest.raises(dev.SrtError, match="srtRefitScene"):
            call()
    assert ctx.launch_info() == info and ctx.last_kernel_ms() == ms
    ctx.refit()
    assert ctx.launch_info() == info and ctx.last_kernel_ms() == ms
    assert [dev.host_random_float() for _ in range(2)] == draws[1:]  # the host generator went on undisturbed
    assert {k: ctx.get_tunable(k) for k in tunables} == tunables
    assert ctx.render_image(p)[0].tobytes() == first.tobytes()
    # the temporal history is dropped: the frame after a refit is a first frame
    ctx.temporal_reset()
    a0 = ctx.render_temporal_frame(p)
    a1 = ctx.render_temporal_frame(p)
    assert a1[3]["historyPixels"] > 0
    ctx.update_spheres(0, sph)
    ctx.refit()
    a2 = ctx.render_temporal_frame(p)
    assert a2[3] == a0[3] and all(x.tobytes() == y.tobytes() for x, y in zip(a0[:3], a2[:3]))


# ------------------------------------------------------------------------------------------------ a scene after another
def _upload_and_record(c, dev, abi, camera, sb):
    """What a scene could inherit from the one before it: the tree as srtGetBvh reads it back, its depth, the axis and pair
    records, the render kernel's form and the image -- and all of them again after an identity update and a refit, which
    make the refit's per-scene tables; the render between the two is refused."""
    c.upload_scene(sb)
    c.set_camera(camera)
    p = _params(abi)

    def record():
        tree, depth, (axis, pairs) = c.bvh(0), c.bvh_depth(), c.tree_aux(0)
        image = c.render_image(p)[0]
        return tree.tobytes(), depth, axis.tobytes(), pairs.tobytes(), c.launch_info()["lds_tree_mode"], image.tobytes()

    before = record()
    c.update_spheres(0, _sphere_array(abi, sb))
    with pytest.raises(dev.SrtError, match="geometry was updated"):
        c.render_image(p)
    c.refit()
    return before, record()


@pytest.mark.parametrize("order", ["soup_then_spheres", "spheres_then_soup"])
@pytest.mark.parametrize("builder", [0, 2])
def test_scene_after_another_behaves_as_on_a_fresh_context(ctx, dev, srt, abi, camera, builder, order):
    """The first scene is rendered, displaced and refitted on the hybrid form, so that its triangle table, hybrid
    renumbering, parent links and stale-box flags all exist; the scene uploaded after it must be served by none of them.
    The render kernels are deterministic from run to run: byte equality, no tolerance."""
    tunables = {"wavefront": 1, "lds_tree": 1, "wf_resident_max": 24}
    saved = {k: ctx.get_tunable(k) for k in tunables}
    scenes = [_soup(srt, builder), _spheres_one_moving(srt)]
    first, second = scenes if order == "soup_then_spheres" else scenes[::-1]
    fresh = dev.Context(0)
    try:
        for k, v in tunables.items():
            ctx.set_tunable(k, v)
            fresh.set_tunable(k, v)
        ctx.upload_scene(first)
        ctx.set_camera(camera)
        ctx.render_image(_params(abi))
        _update_all(ctx, *_displaced(abi, first, 0.05)[2:])
        got = _upload_and_record(ctx, dev, abi, camera, second)
        want = _upload_and_record(fresh, dev, abi, camera, second)
        assert got[0] == want[0]
        assert got[1] == want[1]
    finally:
        fresh.close()
        for k, v in saved.items():
            ctx.set_tunable(k, v)


# ------------------------------------------------------------------------------------------------ example
def _example_data(tmp_path, srt):
    from PIL import Image
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sexy-raytracer_amd", "host")])
    data = tmp_path / "data"
    data.mkdir()
    for f in ("masterchief2-separate-xf.gltf", "masterchief2-separate-xf.bin", "Image_0.png", "Image_1.png"):
        shutil.copy(os.path.join(ROOT, "assets", f), data / f)
    a, n, m, r = srt.scenes.iron_textures()
    Image.fromarray(a).save(data / "rustediron2_basecolor-2x1.png")
    Image.fromarray(n).save(data / "rustediron2_normal-2x1.png")
    Image.fromarray(m[..., 0]).save(data / "rustediron2_metallic-2x1.png")
    Image.fromarray(r[..., 0]).save(data / "rustediron2_roughness-2x1.png")
    return data


def _run_example(tmp_path, data, *args):
    out = tmp_path / "spin.png"
    cmd = [os.path.join(ROOT, "examples", "srt_main"), "--gltf", str(data / "masterchief2-separate-xf.gltf"), "--height", "72",
           "--spp", "4", "--bounces", "4", "--chunks", "1", "--out", str(out)] + list(args)
    return subprocess.run(cmd, env=dict(os.environ, SRT_DATA_DIR=str(data)), capture_output=True)


def test_example_spin(tmp_path, ctx, srt, abi, camera):
    from PIL import Image
    data = _example_data(tmp_path, srt)
    frame = lambda k: np.asarray(Image.open(tmp_path / ("spin_%03d.png" % k)).convert("RGBA"))
    assert _run_example(tmp_path, data, "--frames", "2", "--spin", "0").returncode == 0
    assert np.array_equal(frame(0), frame(1))
    still = frame(0)
    assert _run_example(tmp_path, data, "--frames", "2", "--spin", "20").returncode == 0
    assert np.array_equal(frame(0), still) and not np.array_equal(frame(1), still)
    sb = srt.scenes.scene_masterchief()
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    tri = RF.scene_triangles(sb)
    angle = float(F(20.0)) * 1 * (3.14159265358979323846 / 180.0)
    c, s = F(np.cos(angle)), F(np.sin(angle))
    x, z = tri["p"][..., 0].copy(), tri["p"][..., 2].copy()
    tri["p"][..., 0] = c * x + s * z
    tri["p"][..., 2] = c * z - s * x
    ctx.update_triangles(0, tri)
    ctx.refit()
    want = ctx.render_image(abi.default_render_params(128, 72, 4, 4, seed=1, spp_chunks=1))[1]
    assert np.array_equal(frame(1), want)
    bad = _run_example(tmp_path, data, "--frames", "2", "--spin", "20", "--temporal")
    assert bad.returncode != 0 and b"--temporal" in bad.stderr
