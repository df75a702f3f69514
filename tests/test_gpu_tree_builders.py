"""The device tree builders (csrc/srt_lbvh.hip: linear BVH, PLOC, the paired child-box records) against the NumPy replay
tests/tree_build_ref.py, on bits: node boxes as uint32, child references, split axes, the reported depth and the sixteen
words of every 64-byte record.  No tolerances.  The scenes (tests/tree_build_scenes.py) are the smallest that reach the
kernels' edges: sizes around the 256-wide PLOC block, fewer clusters than the search radius, the radius at the LDS halo's
limit (128), equal keys, equal merge costs, a flat axis, one centroid, a chain-deep tree, and trees at a base other than 0.

A mismatch names the first stage that differs, in build order: boxes, children, axis, depth, pair records."""
import functools
import importlib
import math

import numpy as np
import pytest

import tree_build_ref as R
import tree_build_scenes as S

pytestmark = pytest.mark.gpu

RADII = (1, 2, 16, 64, 128)
BUILDERS = ["LBVH"] + ["PLOC-%d" % r for r in RADII]
SIZES = (2, 3, 4, 255, 256, 257, 513, 3000)


def _abi():
    return importlib.import_module("sexy-raytracer_amd").abi


def _builder(abi, name):
    """'LBVH' or 'PLOC-<radius>' -> (SRT_BUILDER_*, radius or None)."""
    kind, _, radius = name.partition("-")
    return getattr(abi, "SRT_BUILDER_" + kind), int(radius) if radius else None


def _upload(ctx, sb, radius=None):
    """The ploc_radius tunable is read at upload; it is put back whatever happens."""
    saved = ctx.get_tunable("ploc_radius")
    try:
        if radius is not None:
            ctx.set_tunable("ploc_radius", radius)
        ctx.upload_scene(sb)
    finally:
        ctx.set_tunable("ploc_radius", saved)


@functools.lru_cache(maxsize=None)
def _replay(scene, name):
    """(scene builder, replayed nodes, axis, depth) of a one-item scene; computed once per scene and builder."""
    abi = _abi()
    builder, radius = _builder(abi, name)
    if scene.startswith("soup"):
        sb = S.soup(abi, int(scene[4:]), builder)
    else:
        sb = getattr(S, scene)(abi, builder)
    it = sb.world[0]
    refs = np.arange(it.first, it.first + it.count)
    if radius is None:
        return (sb,) + R.build_lbvh(sb, refs, it.time0, it.time1)
    return (sb,) + R.build_ploc(sb, refs, it.time0, it.time1, radius)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _first_diff(got, want):
    bad = np.nonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))[0]
    return "%d of %d differ, first at %d: got %s, want %s" % (len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


def _compare_tree(ctx, item, nodes, axis):
    got = ctx.bvh(item)
    assert len(got) == len(nodes)
    for f in ("bmin", "bmax"):
        assert np.array_equal(_bits(got[f]), _bits(nodes[f])), "boxes (%s): %s" % (f, _first_diff(_bits(got[f]), _bits(nodes[f])))
    for f in ("left", "right"):
        assert np.array_equal(got[f], nodes[f]), "children (%s): %s" % (f, _first_diff(got[f], nodes[f]))
    got_axis, _ = ctx.tree_aux(item)
    assert got_axis.dtype == np.uint8 and np.array_equal(got_axis, axis), "axis: " + _first_diff(got_axis, axis)


def _compare_pairs(ctx, item, nodes, layout):
    _, got = ctx.tree_aux(item)
    want = R.pair_records(nodes, layout.base[item], layout)
    assert got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want)), "pair records: " + _first_diff(_bits(got), _bits(want))


def _check_one_item_scene(ctx, scene, name):
    sb, nodes, axis, depth = _replay(scene, name)
    _upload(ctx, sb, _builder(_abi(), name)[1])
    _compare_tree(ctx, 0, nodes, axis)
    assert ctx.bvh_depth() == depth, "depth"
    _compare_pairs(ctx, 0, nodes, R.Layout(sb, [nodes]))
    return sb, nodes, depth


def _assert_closest_hits(ctx, oracle, abi, sb, rays):
    got = ctx.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    want = oracle.OracleScene(sb).trace(rays, abi.SRT_TRAVERSE_CLOSEST)  # brute force over all primitives
    assert (want["prim"] >= 0).mean() > 0.2
    assert np.array_equal(got["prim"], want["prim"])
    assert np.array_equal(got["t"].view(np.uint32), want["t"].view(np.uint32))


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n", SIZES)
def test_soup_tree_matches_replay(ctx, builder, n):
    """A. Mixed soup (triangles, static and moving spheres): below, at and over one PLOC block, the halo crossing a block
    edge, fewer clusters than the radius."""
    _check_one_item_scene(ctx, "soup%d" % n, builder)


@pytest.mark.parametrize("builder", BUILDERS)
def test_duplicates_tree_matches_replay(ctx, builder):
    """B. Two stacks of identical triangles: the linear BVH splits on the index word (axis 3), every PLOC area ties and the
    pair-partner rule halves the stacks: the depth stays logarithmic."""
    _, nodes, depth = _check_one_item_scene(ctx, "duplicates", builder)
    n = len(nodes) + 1
    assert ctx.bvh_depth() <= 2 * math.ceil(math.log2(n)) + 2
    if builder == "LBVH":  # one split between the stacks, every other one on the index word
        assert (ctx.tree_aux(0)[0] == 3).sum() == n - 2


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("scene", ["flat", "concentric"])
def test_degenerate_extent_tree_matches_replay(ctx, scene, builder):
    """C. Triangles in one axis-aligned plane (padded boxes, no extent of the centroids on z).  D. Concentric spheres: one
    Morton code, the linear BVH is over the index alone, PLOC pairs by area."""
    _check_one_item_scene(ctx, scene, builder)


@pytest.mark.parametrize("builder", BUILDERS)
def test_chain_tree_depth_and_hits(ctx, oracle, abi, builder):
    """E. PLOC merges the geometric line of spheres into a chain as deep as it has primitives.  The reported depth sizes the
    traversal stack, and a push beyond it is dropped silently: the closest hits must still be the brute-force ones."""
    sb, nodes, depth = _check_one_item_scene(ctx, "chain", builder)
    if builder != "LBVH":
        assert depth == len(nodes) + 1
    _assert_closest_hits(ctx, oracle, abi, sb, S.chain_rays(abi))


def _chain_depth(nodes):
    """Nodes on the longest root-to-node chain (what the host-built trees report)."""
    level = np.zeros(len(nodes), np.int64)
    level[0] = 1
    for i in range(len(nodes)):  # pre-order: parents precede children
        for c in (nodes["left"][i], nodes["right"][i]):
            if c >= 0:
                level[c] = level[i] + 1
    return int(level.max())


@pytest.mark.parametrize("radius", [2, 64])
def test_trees_at_a_base_other_than_zero(ctx, oracle, abi, radius):
    """F. A host-built item, a linear-BVH item, a PLOC item and a lone primitive in one world: each device-built tree at its
    own base of the node array, with its own time range, over triangles the flattening renumbered; the records of the whole
    node array, the host-built item's included, over the scene-wide time range."""
    sb = S.four_items(abi)
    _upload(ctx, sb, radius)
    host = ctx.bvh(0)
    lb = R.build_lbvh(sb, np.arange(0, 301), 0.25, 0.5)
    pl = R.build_ploc(sb, np.arange(601, 900), 0.5, 2.0, radius)
    _compare_tree(ctx, 1, lb[0], lb[1])
    _compare_tree(ctx, 2, pl[0], pl[1])
    assert ctx.bvh_depth() == max(_chain_depth(host), lb[2], pl[2]) and max(lb[2], pl[2]) > _chain_depth(host)
    layout = R.Layout(sb, [host, lb[0], pl[0], None])
    assert layout.base == [0, len(host), len(host) + 300, None] and not np.array_equal(layout.tri_dev, np.arange(len(layout.tri_dev)))
    for item, nodes in ((0, host), (1, lb[0]), (2, pl[0])):
        _compare_pairs(ctx, item, nodes, layout)
    with pytest.raises(Exception):
        ctx.tree_aux(3)  # the lone primitive is not a tree
    rays = S.random_rays(abi, with_time=False)
    rays["time"] = 0.5  # inside every item's range: the trees' boxes hold the moving spheres there
    _assert_closest_hits(ctx, oracle, abi, sb, rays)


@pytest.mark.parametrize("scene", ["spheres", "masterchief"])
def test_host_built_tree_pair_records(ctx, srt, scene):
    """pairNodes runs on the host-built trees as well: their records against pair_records over the trees read back."""
    sb = srt.scenes.SCENES[scene]()
    ctx.upload_scene(sb)
    arr = R.arrays(sb)
    item_nodes = [ctx.bvh(w) if it["kind"] == R.WORLD_BVH else None for w, it in enumerate(arr.world)]
    layout = R.Layout(arr, item_nodes)
    for w, nodes in enumerate(item_nodes):
        if nodes is not None:
            _compare_pairs(ctx, w, nodes, layout)
