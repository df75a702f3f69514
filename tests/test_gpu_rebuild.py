"""srtRebuildScene and srtGetTreeCost on the GPU (include/srt_hip.h "Rebuilding"; csrc/srt_refit_host.cpp, csrc/srt_refit.hip,
csrc/srt_api.cpp buildDeviceTrees), on bits: the rebuilt trees against the NumPy replay of the builders on the MOVED scene
(tests/tree_build_ref.py) and against a fresh upload of it, the host-built trees against the refit replay
(tests/refit_ref.py), the depth the kernels size their stacks by, idempotence, the scenes without a device-built item, the
cost against tests/tree_cost_ref.py, the temporal history across a rebuild, the contract and the example.  No tolerances.
Images are 44 x 28 at 2 samples and 4 bounces."""
import numpy as np
import pytest

import refit_ref as RF
import tree_build_ref as R
import tree_build_scenes as S
import tree_cost_ref as C

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, BOUNCES = 44, 28, 2, 4
BUILDERS = ["LBVH", "PLOC-1", "PLOC-16"]


# ------------------------------------------------------------------------------------------------ helpers
def _params(abi, traversal, seed=5):
    return abi.default_render_params(W, H, SPP, BOUNCES, seed=seed, traversal=traversal)


def _builder(abi, name):
    """'LBVH' or 'PLOC-<radius>' -> (SRT_BUILDER_*, radius or None)."""
    kind, _, radius = name.partition("-")
    return getattr(abi, "SRT_BUILDER_" + kind), int(radius) if radius else None


def _upload(c, sb, radius=None):
    """The ploc_radius tunable is read at the upload and put back BEFORE anything else happens: a rebuild must use the
    upload's."""
    saved = c.get_tunable("ploc_radius")
    try:
        if radius is not None:
            c.set_tunable("ploc_radius", radius)
        c.upload_scene(sb)
    finally:
        c.set_tunable("ploc_radius", saved)
    return saved if radius is None else radius


def _geometry(abi, sb):
    sph = np.zeros(len(sb.spheres), abi.SPHERE_DTYPE)
    for i, s in enumerate(sb.spheres):
        sph[i] = (tuple(s.center0), tuple(s.center1), s.time0, s.time1, s.radius, s.material)
    return (RF.scene_triangles(sb) if sb.triangles else np.zeros(0, abi.TRIANGLE_DTYPE)), sph


def _moved(abi, sb, tri, sph):
    spheres = []
    for r in sph:
        s = abi.SrtSphereIn(time0=r["time0"], time1=r["time1"], radius=r["radius"], material=int(r["material"]))
        s.center0[:] = r["center0"].tolist()
        s.center1[:] = r["center1"].tolist()
        spheres.append(s)
    return RF.moved_scene(sb, tri if len(tri) else None, spheres)


def _displaced(abi, sb, amount, seed=3, rigid=False):
    """(tri, sph): every vertex and every sphere centre moved by a random vector of about `amount` (a moving sphere's two
    centres each by its own); rigid: one vector per triangle, so that the primitives keep their size and only drift apart."""
    rng = np.random.default_rng(seed)
    tri, sph = _geometry(abi, sb)
    tri["p"] += rng.normal(0, amount, (len(tri), 1, 3) if rigid else tri["p"].shape).astype(F)
    d = rng.normal(0, amount, (len(sph), 3)).astype(F)
    moving = (sph["center0"] != sph["center1"]).any(axis=1)
    sph["center0"] += d
    sph["center1"] += np.where(moving[:, None] & (not rigid), rng.normal(0, amount, (len(sph), 3)).astype(F), d)
    return tri, sph


def _send(c, tri, sph, then="rebuild", stream=None):
    if len(tri):
        c.update_triangles(0, tri)
    if len(sph):
        c.update_spheres(0, sph)
    if then:
        getattr(c, then)(stream)


def _replay(scene, item, radius):
    """(nodes, axis, depth) of the device-built world item `item` of `scene`, by the builders' replay."""
    it = scene.world[item]
    refs = np.arange(it.first, it.first + it.count)
    if it.builder == R.BUILDER_LBVH:
        return R.build_lbvh(scene, refs, it.time0, it.time1)
    return R.build_ploc(scene, refs, it.time0, it.time1, radius)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _assert_item(c, item, nodes, axis, layout):
    """World item `item` is this tree: boxes as uint32, children, axis, all sixteen words of the pair records."""
    got = c.bvh(item)
    assert len(got) == len(nodes)
    for f in ("bmin", "bmax"):
        assert np.array_equal(_bits(got[f]), _bits(nodes[f])), "boxes of item %d" % item
    for f in ("left", "right"):
        assert np.array_equal(got[f], nodes[f]), "children of item %d" % item
    got_axis, got_pairs = c.tree_aux(item)
    if axis is not None:
        assert np.array_equal(got_axis, axis), "axis of item %d" % item
    want = R.pair_records(nodes, layout.base[item], layout)
    assert np.array_equal(_bits(got_pairs), _bits(want)), "pair records of item %d" % item


def _assert_cost(c, item=0):
    """srtGetTreeCost against the NumPy statement over the tree read back, as uint64."""
    got, want = c.tree_cost(item), C.tree_cost(c.bvh(item))
    assert C.bits(got) == C.bits(want), (item, got, float(want))
    return got


def _state(c, items=(0,)):
    """Every byte the tests can read of the trees: nodes, axis, pair records, depth."""
    out = [c.bvh_depth()]
    for w in items:
        axis, pairs = c.tree_aux(w)
        out += [c.bvh(w).tobytes(), axis.tobytes(), pairs.tobytes()]
    return out


def _children_differ(a, b):
    return not (np.array_equal(a["left"], b["left"]) and np.array_equal(a["right"], b["right"]))


def _view_soup(srt, builder):
    """300 triangles large enough to be seen, and the ground sphere (tests/test_gpu_refit.py's soup)."""
    return srt.scenes.scene_soup(300, seed=11, extent=3.0, size=0.5, builder=builder)


@pytest.fixture
def fresh(dev):
    c = dev.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ 1. the replay's tree
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n", [2, 3, 257, 513])
def test_rebuilt_tree_is_the_replays_tree_of_the_moved_scene(ctx, abi, builder, n):
    """Below, over and across PLOC blocks of 256; the radius is the upload's although the tunable has been put back."""
    which, radius = _builder(abi, builder)
    sb = S.soup(abi, n, which)
    used = _upload(ctx, sb, radius)
    assert radius is None or ctx.get_tunable("ploc_radius") != radius
    uploaded = ctx.bvh(0)
    tri, sph = _displaced(abi, sb, 0.4)
    moved = _moved(abi, sb, tri, sph)
    nodes, axis, depth = _replay(moved, 0, used)
    if n >= 257:  # or the case could not tell a rebuild from a refit
        assert _children_differ(nodes, uploaded)
    _send(ctx, tri, sph)
    _assert_item(ctx, 0, nodes, axis, R.Layout(moved, [nodes]))
    assert ctx.bvh_depth() == depth
    _assert_cost(ctx)


# ------------------------------------------------------------------------------------------------ 2. a fresh upload
def _observe(c, abi, camera, rays, traversals):
    c.set_camera(camera)
    out = _state(c)
    for t in traversals:
        out.append(c.render_image(_params(abi, t))[0].tobytes())
    hits = c.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    return out + [hits.tobytes()]


@pytest.mark.parametrize("builder", ["LBVH", "PLOC-16"])
def test_rebuild_equals_a_fresh_upload(ctx, fresh, srt, abi, camera, builder):
    which, radius = _builder(abi, builder)
    sb = _view_soup(srt, which)
    _upload(ctx, sb, radius)
    uploaded = ctx.bvh(0)
    tri, sph = _displaced(abi, sb, 0.4)
    _send(ctx, tri, sph)
    rays = S.random_rays(abi, with_time=False)
    got = _observe(ctx, abi, camera, rays, [abi.SRT_TRAVERSE_CLOSEST])
    _upload(fresh, _moved(abi, sb, tri, sph), radius)
    assert _children_differ(fresh.bvh(0), uploaded)
    want = _observe(fresh, abi, camera, rays, [abi.SRT_TRAVERSE_CLOSEST])
    assert got == want
    assert C.bits(ctx.tree_cost(0)) == C.bits(fresh.tree_cost(0))


@pytest.mark.parametrize("builder", ["LBVH", "PLOC-16"])
def test_rebuild_withdraws_the_certificate_like_an_upload(ctx, fresh, srt, abi, camera, builder):
    """tests/test_gpu_refit.py's certificate case: a vertex coordinate at 2^-80 is outside the fast division's operand
    range.  The rebuild must withdraw the certificate as the upload of that scene does, or the renders under fast_div part."""
    which, radius = _builder(abi, builder)
    sb = _view_soup(srt, which)
    assert ctx.get_tunable("fast_div") == 1
    used = _upload(ctx, sb, radius)
    tri, sph = _geometry(abi, sb)
    tri["p"][..., 0] += F(7.0)
    k = np.unravel_index(np.argmin(tri["p"][..., 0]), tri["p"].shape[:2])
    tri["p"][k][0] = F(2.0 ** -80)
    sph["center0"][:, 0] += F(1008.0)
    sph["center1"][:, 0] += F(1008.0)
    moved = _moved(abi, sb, tri, sph)
    assert RF.fast_div_certified([ctx.bvh(0)]) and not RF.fast_div_certified([_replay(moved, 0, used)[0]])
    _send(ctx, tri, sph)
    rays = S.random_rays(abi, with_time=False)
    both = [abi.SRT_TRAVERSE_FAITHFUL, abi.SRT_TRAVERSE_CLOSEST]
    got = _observe(ctx, abi, camera, rays, both)
    _upload(fresh, moved, radius)
    assert got == _observe(fresh, abi, camera, rays, both)


# ------------------------------------------------------------------------------------------------ 3. one of each
def test_a_world_of_one_of_each(ctx, oracle, abi):
    """S.four_items: the host-built item is refitted, the LBVH and PLOC items are rebuilt at their bases over the
    renumbered triangles, each with its own times, and the lone primitive stays a primitive."""
    sb = S.four_items(abi)
    radius = _upload(ctx, sb, 16)
    before = [ctx.bvh(w) for w in range(3)]
    host_axis = ctx.tree_aux(0)[0]
    for w in range(3):
        _assert_cost(ctx, w)
    tri, sph = _displaced(abi, sb, 0.4)
    moved = _moved(abi, sb, tri, sph)
    _send(ctx, tri, sph)
    host = RF.refit_world(moved, [before[0], None, None, None])[0]
    lb, pl = _replay(moved, 1, radius), _replay(moved, 2, radius)
    assert _children_differ(lb[0], before[1]) and _children_differ(pl[0], before[2])
    layout = R.Layout(moved, [host, lb[0], pl[0], None])
    assert layout.base == [0, len(host), len(host) + 300, None]
    _assert_item(ctx, 0, host, host_axis, layout)  # (children and axis as uploaded: refit never writes them)
    assert host.tobytes() != before[0].tobytes()
    _assert_item(ctx, 1, lb[0], lb[1], layout)
    _assert_item(ctx, 2, pl[0], pl[1], layout)
    for w in range(3):
        _assert_cost(ctx, w)
    with pytest.raises(Exception):
        ctx.tree_aux(3)
    # the lone primitive among them: brute-force closest hits over the moved scene, inside every item's time range
    rays = S.random_rays(abi, with_time=False)
    rays["time"] = 0.5
    got = ctx.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    want = oracle.OracleScene(moved).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    assert (want["prim"] == 900).any() and (want["prim"] >= 0).mean() > 0.2
    assert np.array_equal(got["prim"], want["prim"]) and np.array_equal(_bits(got["t"]), _bits(want["t"]))


# ------------------------------------------------------------------------------------------------ 4. a deeper tree
def _sphere_cloud(abi, builder, n=40):
    sb = abi.SceneBuilder()
    m = sb.metal((0.7, 0.6, 0.5), 0.1)
    rng = np.random.default_rng(17)
    for _ in range(n):
        c = (rng.random(3, dtype=F) - F(0.5)) * F(6) + np.array([0, 3, -1], F)
        sb.add_sphere(tuple(c.tolist()), float(F(0.1) + rng.random(dtype=F) * F(0.3)), m)
    sb.world_bvh(0, None, 0.0, 1.0, builder=builder)
    return sb


def test_rebuild_into_a_deeper_tree(ctx, fresh, oracle, abi, camera):
    """Forty spheres of a cloud moved onto the positions of S.chain, which PLOC merges into a chain forty deep: the depth the
    traversal stacks are sized by has to grow with the tree, or pushes are dropped silently."""
    sb = _sphere_cloud(abi, abi.SRT_BUILDER_PLOC)
    radius = _upload(ctx, sb)
    shallow = ctx.bvh_depth()
    tri, sph = _geometry(abi, sb)
    x = 1.5 ** np.arange(40)
    sph["center0"] = sph["center1"] = np.stack([x, 0 * x, 0 * x], axis=1).astype(F)
    sph["radius"] = (0.1 * x).astype(F)
    moved = _moved(abi, sb, tri, sph)
    nodes, axis, depth = _replay(moved, 0, radius)
    assert depth == 40 and depth > shallow
    _send(ctx, tri, sph)
    assert ctx.bvh_depth() == depth
    _assert_item(ctx, 0, nodes, axis, R.Layout(moved, [nodes]))
    rays = S.chain_rays(abi)
    got = ctx.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    want = oracle.OracleScene(moved).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    assert (want["prim"] >= 0).mean() > 0.2
    assert np.array_equal(got["prim"], want["prim"]) and np.array_equal(_bits(got["t"]), _bits(want["t"]))
    ctx.set_camera(camera)
    p = _params(abi, abi.SRT_TRAVERSE_CLOSEST)
    image = ctx.render_image(p)[0]
    _upload(fresh, moved)
    fresh.set_camera(camera)
    assert fresh.bvh_depth() == depth
    assert image.tobytes() == fresh.render_image(p)[0].tobytes()
    # ... and back: the depth shrinks again with the tree
    _send(ctx, *_geometry(abi, sb))
    assert ctx.bvh_depth() == shallow


# ------------------------------------------------------------------------------------------------ 5. idempotence
@pytest.mark.parametrize("builder", ["LBVH", "PLOC-16"])
def test_idempotence_and_history_independence(ctx, abi, builder):
    which, radius = _builder(abi, builder)
    sb = S.soup(abi, 300, which)
    used = _upload(ctx, sb, radius)
    uploaded = _state(ctx)
    ctx.rebuild()
    assert _state(ctx) == uploaded
    ctx.rebuild()
    assert _state(ctx) == uploaded
    a, b = _displaced(abi, sb, 0.5, seed=4), _displaced(abi, sb, 0.4, seed=5)
    _send(ctx, *a, then="refit")
    _send(ctx, *b)
    moved = _moved(abi, sb, *b)
    nodes, axis, depth = _replay(moved, 0, used)
    _assert_item(ctx, 0, nodes, axis, R.Layout(moved, [nodes]))
    assert ctx.bvh_depth() == depth
    once = _state(ctx)
    ctx.rebuild()
    assert _state(ctx) == once


# ------------------------------------------------------------------------------------------------ 6. nothing to rebuild
@pytest.mark.parametrize("scene", ["spheres", "soup"])
def test_without_a_device_built_item_rebuild_is_refit(ctx, srt, abi, camera, node_path, scene):
    if scene == "spheres":
        sb = srt.scenes.scene_spheres()
        sb.spheres[2].center1[:] = (0.5, 1.25, -0.5)
    else:
        sb = _view_soup(srt, 0)
    tri, sph = _displaced(abi, sb, 0.25)
    p = _params(abi, abi.SRT_TRAVERSE_FAITHFUL)
    seen = {}
    for then in ("refit", "rebuild"):
        ctx.upload_scene(sb)
        ctx.set_camera(camera)
        _send(ctx, tri, sph, then=then)
        image = ctx.render_image(p)[0]
        seen[then] = _state(ctx) + [ctx.launch_info()["lds_tree_mode"], image.tobytes(), C.bits(ctx.tree_cost(0))]
    assert seen["rebuild"] == seen["refit"]
    if scene == "soup":
        assert (seen["refit"][4] == 4) == (node_path == "hybrid")


# ------------------------------------------------------------------------------------------------ 7. tree cost
def _one_sphere(abi, builder):
    sb = abi.SceneBuilder()
    sb.add_sphere((0.5, 3.0, -1.0), 0.75, sb.metal((0.7, 0.6, 0.5), 0.1))
    sb.world_bvh(0, None, 0.0, 1.0, builder=builder)
    return sb


@pytest.mark.parametrize("nodes", [63, 64, 65, 255, 256, 257])
def test_tree_cost_around_a_wave_and_a_block(ctx, abi, nodes):
    ctx.upload_scene(S.soup(abi, nodes + 1, abi.SRT_BUILDER_LBVH))
    assert len(ctx.bvh(0)) == nodes
    assert _assert_cost(ctx) > 1.0


def test_tree_cost_small_and_host_built(ctx, srt, abi):
    for which in (abi.SRT_BUILDER_LBVH, abi.SRT_BUILDER_PLOC):
        ctx.upload_scene(_one_sphere(abi, which))   # one primitive: a single-object leaf
        assert len(ctx.bvh(0)) == 1 and C.bits(_assert_cost(ctx)) == C.bits(1.0)
        ctx.upload_scene(S.soup(abi, 2, which))     # two primitives: one node
        assert len(ctx.bvh(0)) == 1 and C.bits(_assert_cost(ctx)) == C.bits(1.0)
    ctx.upload_scene(_view_soup(srt, 0))            # host-built
    assert _assert_cost(ctx) > 1.0


def test_tree_cost_through_every_level(ctx, srt, abi):
    """65 537 nodes (65 537 triangles and the ground sphere under the linear BVH).  The reduction sums 256 values per
    workgroup and level and hands at most 256 partials to the host: 256^2 + 1 nodes are the fewest that leave more than 256
    partials (257) after the node level, so the partials level runs (257 -> 2, its second workgroup all padding but one
    value) and the host finishes (2 -> 1)."""
    ctx.upload_scene(srt.scenes.scene_soup(65537, seed=3, builder=abi.SRT_BUILDER_LBVH))
    assert len(ctx.bvh(0)) == 256 * 256 + 1
    _assert_cost(ctx)


def test_tree_cost_follows_refit_and_rebuild(ctx, fresh, abi):
    """A PLOC soup of 513 whose primitives drift apart by about the scene's extent: the refit tree costs more than the
    rebuilt one (on the CPU, with the replays: by a factor of 5.1 for this seed)."""
    sb = S.soup(abi, 513, abi.SRT_BUILDER_PLOC)
    radius = _upload(ctx, sb)
    uploaded = ctx.bvh(0)
    tri, sph = _displaced(abi, sb, 3.0, rigid=True)
    moved = _moved(abi, sb, tri, sph)
    refit = RF.refit_world(moved, [uploaded])[0]
    rebuilt = _replay(moved, 0, radius)[0]
    assert R.sah_cost(refit) >= 2 * R.sah_cost(rebuilt)
    _send(ctx, tri, sph, then="refit")
    after_refit = ctx.tree_cost(0)
    assert C.bits(after_refit) == C.bits(C.tree_cost(refit)) == C.bits(C.tree_cost(ctx.bvh(0)))
    ctx.rebuild()
    after_rebuild = _assert_cost(ctx)
    _upload(fresh, moved)
    assert C.bits(after_rebuild) == C.bits(fresh.tree_cost(0))
    print("tree cost: %.3f after refit, %.3f after rebuild" % (after_refit, after_rebuild))
    assert after_refit > after_rebuild


# ------------------------------------------------------------------------------------------------ 8. temporal history
def test_temporal_history_across_a_rebuild(fresh, srt, abi, camera):
    """The feature scene under PLOC, CLOSEST traversal (its results do not depend on the tree), tracking on: frame, update,
    REBUILD, frame is frame, update, refit, frame in every bit, history included."""
    from test_gpu_motion import _feature_scene
    c = fresh
    sb = _feature_scene(srt, abi)
    it = sb.world[0]
    sb.world = []
    sb.world_bvh(it.first, it.count, it.time0, it.time1, builder=abi.SRT_BUILDER_PLOC)
    tri, sph = _displaced(abi, sb, 0.08, seed=8)
    d, t = abi.default_denoise_params(), abi.default_temporal_params()
    pk = [abi.default_render_params(W, H, 3, 4, seed=9, spp_chunks=0, sample_first=3 * k, traversal=abi.SRT_TRAVERSE_CLOSEST)
          for k in range(2)]

    def start(tracking):
        c.upload_scene(sb)
        c.set_motion_tracking(tracking)
        c.temporal_reset()
        c.set_camera(camera)

    seen = {}
    for then in ("refit", "rebuild"):
        start(True)
        assert c.render_temporal_frame(pk[0], d, t)[3]["historyPixels"] == 0
        _send(c, tri, sph, then=then)
        frame = c.render_temporal_frame(pk[1], d, t)
        seen[then] = [x.tobytes() for x in frame[:3]] + [frame[3], c.render_motion(pk[1]).tobytes()]
    assert seen["rebuild"][3]["historyPixels"] > 0.2 * W * H
    assert seen["rebuild"] == seen["refit"]
    # two rebuilds between frames: the snapshot spans only the last epoch, a first frame
    start(True)
    first = c.render_temporal_frame(pk[0], d, t)
    _send(c, tri, sph)
    c.rebuild()
    assert c.render_temporal_frame(pk[1], d, t)[3]["historyPixels"] == 0
    # tracking off: a rebuild drops the history
    start(False)
    again = c.render_temporal_frame(pk[0], d, t)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first[:3], again[:3]))
    _send(c, tri, sph)
    assert c.render_temporal_frame(pk[1], d, t)[3]["historyPixels"] == 0


# ------------------------------------------------------------------------------------------------ 9. contract
def test_contract(ctx, fresh, dev, srt, abi, camera):
    import ctypes
    import torch
    cost = ctypes.c_double(7.5)
    with pytest.raises(dev.SrtError, match="no scene"):
        fresh.rebuild()
    assert dev.lib.srtGetTreeCost(fresh.h, 0, ctypes.byref(cost)) != 0 and b"no scene" in dev.lib.srtLastError(fresh.h)
    sb = S.four_items(abi)
    _upload(ctx, sb, 16)
    ctx.set_camera(camera)
    for item, text in ((3, b"not a bvh"), (4, b"out of range"), (-1, b"out of range")):
        assert dev.lib.srtGetTreeCost(ctx.h, item, ctypes.byref(cost)) != 0 and text in dev.lib.srtLastError(ctx.h)
    assert dev.lib.srtGetTreeCost(ctx.h, 1, None) != 0 and b"null" in dev.lib.srtLastError(ctx.h)
    # no side effects: tunables, the host generator, the statistics, the last render's description
    p = _params(abi, abi.SRT_TRAVERSE_CLOSEST)
    first = ctx.render_image(p)[0]
    tunables = {k: ctx.get_tunable(k) for k in ("ploc_radius", "fast_div", "wavefront", "lds_tree", "wf_resident_max")}
    dev.host_random_reset()
    draws = [dev.host_random_float() for _ in range(3)]
    dev.host_random_reset()
    dev.host_random_float()
    stats, info, ms = ctx.stats(), ctx.launch_info(), ctx.last_kernel_ms()
    tri, sph = _geometry(abi, sb)
    ctx.update_triangles(0, tri)
    # dirty: nothing traverses the scene, and the cost is refused in checkSceneReady's words
    rays = S.random_rays(abi, count=16)
    for call in (lambda: ctx.render_image(p), lambda: ctx.trace(rays), lambda: ctx.render_features(p), lambda: ctx.tree_cost(1)):
        with pytest.raises(dev.SrtError, match="geometry was updated"):
            call()
    assert dev.lib.srtGetTreeCost(ctx.h, 1, ctypes.byref(cost)) != 0 and cost.value == 7.5
    ctx.rebuild()
    ctx.tree_cost(1)
    assert (ctx.stats(), ctx.launch_info(), ctx.last_kernel_ms()) == (stats, info, ms)
    assert [dev.host_random_float() for _ in range(2)] == draws[1:]
    assert {k: ctx.get_tunable(k) for k in tunables} == tunables
    assert ctx.render_image(p)[0].tobytes() == first.tobytes()  # an identity update and a rebuild: the upload's trees
    assert len(ctx.trace(rays)) == 16 and ctx.render_features(p) is not None
    # records in device memory, updated on a side stream, rebuilt behind it: the null-stream result
    moved_tri, moved_sph = _displaced(abi, sb, 0.4)
    _send(ctx, moved_tri, moved_sph)
    want = _state(ctx, (0, 1, 2))
    _send(ctx, tri, sph)
    side = torch.cuda.Stream()
    d_tri = torch.from_numpy(moved_tri.copy().view(np.uint8).reshape(-1, 64)).cuda()
    d_sph = torch.from_numpy(moved_sph.copy().view(np.uint8).reshape(-1, 40)).cuda()
    side.wait_stream(torch.cuda.current_stream())
    ctx.update_triangles(0, d_tri, stream=side.cuda_stream)
    ctx.update_spheres(0, d_sph, stream=side.cuda_stream)
    ctx.rebuild(side.cuda_stream)
    assert _state(ctx, (0, 1, 2)) == want


# ------------------------------------------------------------------------------------------------ 10. example
def test_example_reports_the_tree_cost(tmp_path, srt):
    import re
    from PIL import Image
    from test_gpu_refit import _example_data, _run_example
    data = _example_data(tmp_path, srt)
    frame = lambda k: np.asarray(Image.open(tmp_path / ("spin_%03d.png" % k)).convert("RGBA"))
    assert _run_example(tmp_path, data, "--frames", "2", "--spin", "5").returncode == 0
    plain = [frame(0), frame(1)]
    run = _run_example(tmp_path, data, "--frames", "2", "--spin", "5", "--tree-cost")
    assert run.returncode == 0
    lines = re.findall(r"^frame (\d+) tree cost (\S+)$", run.stderr.decode(), flags=re.M)
    assert [int(k) for k, _ in lines] == [0, 1]
    assert all(np.isfinite(float(x)) and float(x) > 0 for _, x in lines)
    assert np.array_equal(frame(0), plain[0]) and np.array_equal(frame(1), plain[1])
    bad = _run_example(tmp_path, data, "--tree-cost")
    assert bad.returncode != 0 and b"--tree-cost" in bad.stderr
