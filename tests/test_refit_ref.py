"""The refit replay (tests/refit_ref.py) held to the host tree builder, srtBuildBvh, and to cases worked by hand.  No GPU.

srtBuildBvh (bvh.h:55-95) draws one axis per node and sorts on the primitives' box minima.  A scene scaled by exactly 2
about the origin has every coordinate, every box and every sort key doubled exactly, so the builder draws the same axes,
sorts the same order and builds the same topology: the replay of (the original's topology, the primitives x 2) must be
srtBuildBvh of the scaled scene, bit for bit.  The scene has no axis-flat triangle -- the 0.0001 pad of a flat axis does
not scale."""
import numpy as np

import refit_ref as RF
import tree_build_ref as R

F = np.float32


def _scaled(abi, sb, k):
    tri = RF.scene_triangles(sb)
    tri["p"] *= F(k)
    sph = []
    for s in sb.spheres:
        t = abi.SrtSphereIn(time0=s.time0, time1=s.time1, radius=F(s.radius) * F(k), material=s.material)
        t.center0[:] = [F(x) * F(k) for x in s.center0]
        t.center1[:] = [F(x) * F(k) for x in s.center1]
        sph.append(t)
    return RF.moved_scene(sb, tri, sph)


def _same_bits(a, b):
    return a.tobytes() == b.tobytes()


def test_scaled_scene_equals_host_build(srt, dev):
    sb = srt.scenes.scene_soup(300, seed=11)
    tri = RF.scene_triangles(sb)["p"]
    assert (tri.min(axis=1) != tri.max(axis=1)).all(), "an axis-flat triangle: its pad does not scale"
    nodes, depth = dev.build_bvh_host(sb)
    sb2 = _scaled(srt.abi, sb, 2.0)
    want, depth2 = dev.build_bvh_host(sb2)
    assert depth2 == depth
    assert np.array_equal(want["left"], nodes["left"]) and np.array_equal(want["right"], nodes["right"])
    it = sb.world[0]
    got = RF.refit(sb2, nodes, it.time0, it.time1)
    assert _same_bits(got, want)
    # and the replay of the unmoved scene is the build itself
    assert _same_bits(RF.refit(sb, nodes, it.time0, it.time1), nodes)


def test_random_displacement_unions(srt, dev):
    sb = srt.scenes.scene_soup(300, seed=12)
    nodes, _ = dev.build_bvh_host(sb)
    rng = np.random.default_rng(5)
    tri = RF.scene_triangles(sb)
    tri["p"] += rng.normal(0, 0.3, tri["p"].shape).astype(F)
    sb2 = RF.moved_scene(sb, tri)
    it = sb.world[0]
    got = RF.refit(sb2, nodes, it.time0, it.time1)
    assert not _same_bits(got, nodes)
    pmn, pmx = R.prim_boxes(sb2, np.arange(it.first, it.first + it.count), it.time0, it.time1)
    assert np.array_equal(got["bmin"][0], pmn.min(axis=0)) and np.array_equal(got["bmax"][0], pmx.max(axis=0))
    for i in range(len(got)):
        mn, mx = [], []
        for c in (int(got["left"][i]), int(got["right"][i])):
            if c >= 0:
                mn.append(got["bmin"][c]); mx.append(got["bmax"][c])
            else:
                mn.append(pmn[~c - it.first]); mx.append(pmx[~c - it.first])
        assert np.array_equal(got["bmin"][i], np.minimum(*mn)) and np.array_equal(got["bmax"][i], np.maximum(*mx)), i


def _tri(abi, sb, verts, mat):
    return sb.add_triangles(np.array(verts, F), np.zeros((3, 2), F), [[0, 1, 2]], mat)


def _node(left, right):
    n = np.zeros(1, R.NODE_DTYPE)
    n["left"], n["right"] = left, right
    return n


def test_hand_single_object_leaf(srt):
    abi = srt.abi
    sb = abi.SceneBuilder()
    _tri(abi, sb, [[0, 0, 0], [1, 2, 0], [0.5, 1, 3]], sb.metal((1, 1, 1), 0))
    sb.world_bvh(0, 1)
    got = RF.refit(sb, _node(~0, ~0), 0, 1)
    assert got["bmin"][0].tolist() == [0, 0, 0] and got["bmax"][0].tolist() == [1, 2, 3]


def test_hand_flat_axis_is_padded(srt):
    abi = srt.abi
    sb = abi.SceneBuilder()
    _tri(abi, sb, [[0, 5, 0], [1, 5, 0], [0, 5, 1]], sb.metal((1, 1, 1), 0))
    sb.world_bvh(0, 1)
    got = RF.refit(sb, _node(~0, ~0), 0, 1)
    assert got["bmin"][0, 1] == F(5) - F(0.0001) and got["bmax"][0, 1] == F(5) + F(0.0001)


def test_hand_mixed_node(srt):
    """Node 0 = (node 1, triangle 2), node 1 = (triangle 0, triangle 1): a caller-built shape."""
    abi = srt.abi
    sb = abi.SceneBuilder()
    m = sb.metal((1, 1, 1), 0)
    _tri(abi, sb, [[0, 0, 0], [1, 1, 1], [0.5, 0.25, 0.75]], m)
    _tri(abi, sb, [[2, 2, 2], [3, 3, 3], [2.5, 2.25, 2.75]], m)
    _tri(abi, sb, [[-4, 7, 1], [-3, 8, 2], [-3.5, 7.5, 1.5]], m)
    nodes = np.concatenate([_node(1, ~2), _node(~0, ~1)])
    got = RF.refit(sb, nodes, 0, 1)
    assert got["bmin"][1].tolist() == [0, 0, 0] and got["bmax"][1].tolist() == [3, 3, 3]
    assert got["bmin"][0].tolist() == [-4, 0, 0] and got["bmax"][0].tolist() == [3, 8, 3]
    assert got["left"].tolist() == [1, ~0] and got["right"].tolist() == [~2, ~1]


def test_hand_moving_sphere(srt):
    """sphere.h:47-52: centre(t) = c0 + ((t - t0) / (t1 - t0)) * (c1 - c0); the box is the union over both item times."""
    abi = srt.abi
    sb = abi.SceneBuilder()
    sb.add_sphere((0, 0, 0), 1.0, sb.metal((1, 1, 1), 0), center1=(4, 0, -2), time0=0.0, time1=2.0)
    sb.world_bvh(0, 1, 0.0, 1.0)
    got = RF.refit(sb, _node(~0, ~0), 0.0, 1.0)  # the centre moves from (0, 0, 0) to (2, 0, -1) over the item's times
    assert got["bmin"][0].tolist() == [-1, -1, -2] and got["bmax"][0].tolist() == [3, 1, 1]
    still = RF.refit(sb, _node(~0, ~0), 0.0, 0.0)
    assert still["bmin"][0].tolist() == [-1, -1, -1] and still["bmax"][0].tolist() == [1, 1, 1]


def test_hand_two_item_world(srt):
    """Two trees with their own times: the same moving sphere under item times (0, 0) and (0, 1)."""
    abi = srt.abi
    sb = abi.SceneBuilder()
    m = sb.metal((1, 1, 1), 0)
    sb.add_sphere((0, 0, 0), 1.0, m, center1=(2, 0, 0), time0=0.0, time1=1.0)
    sb.add_sphere((0, 0, 0), 1.0, m, center1=(2, 0, 0), time0=0.0, time1=1.0)
    sb.world_bvh(0, 1, 0.0, 0.0)
    sb.world_bvh(1, 1, 0.0, 1.0)
    a, b = RF.refit_world(sb, [_node(~0, ~0), _node(~1, ~1)])
    assert a["bmax"][0].tolist() == [1, 1, 1] and b["bmax"][0].tolist() == [3, 1, 1]
    pairs = RF.pair_records_world(sb, [a, b])
    # the pair records use the widest times of the world for every item (srt_lbvh.hip pairNodes)
    assert pairs[0][0, 4:7].tolist() == [3, 1, 1] and pairs[1][0, 4:7].tolist() == [3, 1, 1]
    assert RF.fast_div_certified([a, b])
    a["bmin"][0, 0] = F(2.0 ** -80)
    assert not RF.fast_div_certified([a, b])
