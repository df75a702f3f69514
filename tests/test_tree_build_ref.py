"""CPU-side checks of tests/tree_build_ref.py (no GPU): the replay is the oracle of tests/test_gpu_tree_builders.py, so it
is held here to independent restatements -- a recursive top-down radix tree, a loop-per-cluster PLOC, hand-worked merges --
and to the structural invariants of both builders."""
import math
import sys

import numpy as np
import pytest

import tree_build_ref as R
import tree_build_scenes as S

F = np.float32
SIZES = (2, 3, 4, 255, 256, 257, 513, 3000)


def _scenes(abi, builder=0):
    out = [("soup%d" % n, S.soup(abi, n, builder)) for n in (2, 3, 4, 37, 257)]
    return out + [("duplicates", S.duplicates(abi, builder, 200)), ("flat", S.flat(abi, builder)),
                  ("concentric", S.concentric(abi, builder)), ("chain", S.chain(abi, builder))]


def _keys(sb):
    it = sb.world[0]
    refs = np.arange(it.first, it.first + it.count)
    boxes = R.prim_boxes(sb, refs, it.time0, it.time1)
    keys, order = R.sort_keys(R.morton_keys(boxes))
    return refs, boxes, keys, order


# ------------------------------------------------------------------ independent restatements
def _topdown(keys):
    """The radix tree by recursion: split the sorted range at the highest differing key bit."""
    k = [int(x) for x in keys]
    left, right = {}, {}

    def build(node, lo, hi):
        bit = (k[lo] ^ k[hi]).bit_length() - 1
        g = lo
        while (k[g + 1] >> bit) & 1 == 0:
            g += 1
        left[node] = ~lo if lo == g else g
        right[node] = ~hi if g + 1 == hi else g + 1
        if lo < g:
            build(g, lo, g)
        if g + 1 < hi:
            build(g + 1, g + 1, hi)

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(10000)
    try:
        build(0, 0, len(k) - 1)
    finally:
        sys.setrecursionlimit(old)
    n = len(k) - 1
    return np.array([left[i] for i in range(n)]), np.array([right[i] for i in range(n)])


def _area(amn, amx, bmn, bmx):
    d = [F(max(amx[k], bmx[k])) - F(min(amn[k], bmn[k])) for k in range(3)]
    return F(F(F(d[0] * d[1]) + F(d[1] * d[2])) + F(d[2] * d[0]))


def _ploc_slow(bmn, bmx, order, radius):
    """One Python loop per cluster and candidate: (left, right, axis, boxes, depth, rounds)."""
    n = len(order)
    cl = [dict(mn=bmn[p], mx=bmx[p], ref=~int(p), depth=1) for p in order]
    left, right, axis = [None] * (n - 1), [None] * (n - 1), [None] * (n - 1)
    box = [None] * (n - 1)
    made = rounds = 0
    while len(cl) > 1:
        m = len(cl)
        nn = []
        for i in range(m):
            best, bj = None, -1
            for j in range(max(0, i - radius), min(m - 1, i + radius) + 1):
                if j == i:
                    continue
                a = _area(cl[i]["mn"], cl[i]["mx"], cl[j]["mn"], cl[j]["mx"])
                if best is None or a < best or (a == best and j == (i ^ 1)):
                    best, bj = a, j
            nn.append(bj)
        nxt = []
        for i in range(m):
            j = nn[i]
            if nn[j] != i:
                nxt.append(cl[i])
            elif i < j:
                me, ot = cl[i], cl[j]
                node = (n - 2) - made
                made += 1
                d = [F(F(ot["mn"][k] + ot["mx"][k]) - F(me["mn"][k] + me["mx"][k])) for k in range(3)]
                big = max(abs(x) for x in d)
                ax = [abs(x) for x in d].index(big)  # the first axis attaining the largest difference
                first = (me, ot) if d[ax] >= 0 else (ot, me)
                left[node], right[node] = first[0]["ref"], first[1]["ref"]
                axis[node] = 3 if d[ax] == 0 else ax
                mn, mx = np.minimum(me["mn"], ot["mn"]), np.maximum(me["mx"], ot["mx"])
                box[node] = (mn, mx)
                nxt.append(dict(mn=mn, mx=mx, ref=node, depth=max(me["depth"], ot["depth"]) + 1))
        assert len(nxt) < m
        cl = nxt
        rounds += 1
    return np.array(left), np.array(right), np.array(axis), box, cl[0]["depth"], rounds


def _recursive_depth(left, right):
    # parents are not ordered in the radix tree's numbering: plain memoised recursion on an explicit stack
    seen = {}
    stack = [0]
    while stack:
        i = stack[-1]
        kids = [int(c) for c in (left[i], right[i]) if c >= 0]
        todo = [c for c in kids if c not in seen]
        if todo:
            stack.extend(todo)
            continue
        stack.pop()
        seen[i] = 1 + max([seen[c] for c in kids] + [1])
    return seen[0]


def _inorder_leaves(left, right):
    out, stack = [], [0]
    while stack:
        c = stack.pop()
        if c < 0:
            out.append(~c)
        else:
            stack.append(int(right[c]))
            stack.append(int(left[c]))
    return out


def _check_tree(left, right, leaves):
    n = len(left)
    refs = np.concatenate([left, right])
    assert sorted((~refs[refs < 0]).tolist()) == sorted(leaves)
    assert sorted(refs[refs >= 0].tolist()) == list(range(1, n))


# ------------------------------------------------------------------ the radix tree
def test_lbvh_equals_recursive_topdown_form(abi):
    for name, sb in _scenes(abi):
        _, _, keys, _ = _keys(sb)
        assert len(np.unique(keys)) == len(keys)
        left, right, axis, depth = R.lbvh(keys)
        wl, wr = _topdown(keys)
        assert np.array_equal(left, wl) and np.array_equal(right, wr), name
        _check_tree(left, right, list(range(len(keys))))
        assert _inorder_leaves(left, right) == list(range(len(keys))), name  # key order
        assert depth == _recursive_depth(left, right), name


def test_lbvh_axis_names_the_splitting_coordinate(abi):
    """Decode each node's split from the boxes' quantised centroids: the children's keys differ first in a bit of the named
    coordinate, the left side holding 0; axis 3 exactly when the Morton codes of the node's range are all equal."""
    for name, sb in _scenes(abi):
        _, boxes, keys, order = _keys(sb)
        left, right, axis, _ = R.lbvh(keys)
        codes = (keys >> np.uint64(32)).astype(np.int64)
        for i in range(len(left)):
            span = _span(left, right, i)
            lo, hi = min(span), max(span)
            if codes[lo] == codes[hi]:
                assert axis[i] == 3, name
                continue
            bit = int(codes[lo] ^ codes[hi]).bit_length() - 1
            assert axis[i] == 2 - bit % 3, name
            first_right = min(_span(left, right, int(right[i])) if right[i] >= 0 else [~int(right[i])])
            assert (codes[first_right] >> bit) & 1 == 1 and (codes[first_right - 1] >> bit) & 1 == 0


def _span(left, right, i):
    out, stack = [], [i]
    while stack:
        c = stack.pop()
        if c < 0:
            out.append(~c)
        else:
            stack += [int(left[c]), int(right[c])]
    return out


def test_morton_keys_by_hand():
    """Four centroids at the corners and the middle of a 2 x 4 x 8 block: quantised coordinates 0, 512 and 1023, x in the
    highest bit of each triple and z in the lowest; the index in the low word."""
    c = np.array([[0, 0, 0], [2, 4, 8], [1, 2, 4], [2, 0, 0], [0, 4, 0], [0, 0, 8]], F)
    keys = R.morton_keys((c - F(0.25), c + F(0.25)))
    codes = (keys >> np.uint64(32)).astype(np.int64)

    def spread(v):
        return sum(((v >> b) & 1) << (3 * b) for b in range(10))

    assert codes[0] == 0 and codes[1] == (1 << 30) - 1
    assert codes[2] == spread(512) << 2 | spread(512) << 1 | spread(512)
    assert codes[3] == spread(1023) << 2 and codes[4] == spread(1023) << 1 and codes[5] == spread(1023)
    assert ((keys & np.uint64(0xffffffff)) == np.arange(6, dtype=np.uint64)).all()
    # no extent on an axis: u = 0 there
    flat = c.copy()
    flat[:, 1] = 7.0
    codes = (R.morton_keys((flat, flat)) >> np.uint64(32)).astype(np.int64)
    assert all((int(x) & spread(1023) << 1) == 0 for x in codes)


# ------------------------------------------------------------------ primitive boxes
def test_prim_boxes_by_hand(abi):
    sb = abi.SceneBuilder()
    mat = sb.metal((0.5, 0.5, 0.5), 0.0)
    sb.add_triangles(np.array([[1, 2, 3], [4, 2, -1], [0, 2, 5]], F), np.zeros((3, 2), F), [[0, 1, 2]], mat)
    sb.add_sphere((1.0, 2.0, 3.0), 0.5, mat)
    sb.add_sphere((1.0, 2.0, 3.0), 0.5, mat, center1=(3.0, 2.0, 3.0), time0=1.0, time1=2.0)
    mn, mx = R.prim_boxes(sb, [0, 1, 2], 0.0, 1.5)
    pad = F(0.0001)
    assert mn[0].tolist() == [0, F(2) - pad, -1] and mx[0].tolist() == [4, F(2) + pad, 5]
    assert mn[1].tolist() == [0.5, 1.5, 2.5] and mx[1].tolist() == [1.5, 2.5, 3.5]
    # the moving sphere at t = 0 is at x = 1 + (-1) * 2 = -1, at t = 1.5 at x = 2
    assert mn[2].tolist() == [-1.5, 1.5, 2.5] and mx[2].tolist() == [2.5, 2.5, 3.5]
    assert mn.dtype == mx.dtype == np.float32


# ------------------------------------------------------------------ PLOC
def _cubes(xs):
    xs = np.asarray(xs, F)
    mn = np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], axis=1)
    return mn, (mn + F(1)).astype(F)


def test_ploc_hand_worked_merges():
    """Unit cubes at x = 0, 1, 3, 4, 10 (union area 2 dx + 3, so nearest = closest): round 1 merges (0, 1) -> node 3 and
    (2, 3) -> node 2, round 2 merges those -> node 1, round 3 adds the far cube -> node 0."""
    boxes = _cubes([0, 1, 3, 4, 10])
    nodes, axis, depth, rounds = R.ploc(boxes, np.arange(5), 2)
    assert nodes["left"].tolist() == [1, 3, ~2, ~0] and nodes["right"].tolist() == [~4, 2, ~3, ~1]
    assert axis.tolist() == [0, 0, 0, 0] and depth == 4 and rounds == 3
    assert nodes["bmin"][:, 0].tolist() == [0, 0, 3, 0] and nodes["bmax"][:, 0].tolist() == [11, 5, 5, 2]
    # the lower centroid goes left whatever the positions in the array are
    nodes, axis, _, _ = R.ploc(_cubes([1, 0, 4, 3, 10]), np.arange(5), 2)
    assert nodes["left"].tolist() == [1, 3, ~3, ~1] and nodes["right"].tolist() == [~4, 2, ~2, ~0]


def test_ploc_pair_partner_wins_ties():
    """Equally spaced cubes: every inner cube's two neighbours tie.  The pair partner i ^ 1 wins, so (0, 1) and (2, 3) merge
    in one round; the lower position alone would chain 2 -> 1 -> 0 and merge one pair."""
    boxes = _cubes([0, 2, 4, 6])
    assert R.ploc_nearest(boxes[0], boxes[1], 1).tolist() == [1, 0, 3, 2]
    nodes, axis, depth, rounds = R.ploc(boxes, np.arange(4), 3)
    assert rounds == 2 and depth == 3
    assert nodes["left"].tolist() == [2, ~2, ~0] and nodes["right"].tolist() == [1, ~3, ~1]
    # identical boxes: all areas tie, the array halves every round, axis 3 and the leader on the left
    same = _cubes([5] * 16)
    nodes, axis, depth, rounds = R.ploc(same, np.arange(16), 128)
    assert rounds == 4 and depth == 5 and (axis == 3).all()
    assert nodes["left"][14] == ~0 and nodes["right"][14] == ~1
    # a tie that the partner does not take part in goes to the lower position
    boxes = _cubes([0, 2, 4, 6, 8])
    assert R.ploc_nearest(boxes[0], boxes[1], 4)[4] == 3 and R.ploc_nearest(boxes[0], boxes[1], 4)[1] == 0
    # the window: with radius 1 cube 2 cannot see cube 0, although it is the closest
    far = _cubes([0, 50, 1, 60])
    assert R.ploc_nearest(far[0], far[1], 1).tolist() == [1, 2, 1, 2]
    assert R.ploc_nearest(far[0], far[1], 2).tolist() == [2, 3, 0, 1]


@pytest.mark.parametrize("radius", [1, 2, 16, 128])
def test_ploc_rounds_equal_loop_per_cluster(abi, radius):
    for name, sb in _scenes(abi):
        _, boxes, _, order = _keys(sb)
        if len(order) > 100:
            order = order[:97]  # the slow form is quadratic in Python
        nodes, axis, depth, rounds = R.ploc(boxes, order, radius)
        left, right, waxis, box, wdepth, wrounds = _ploc_slow(boxes[0], boxes[1], order, radius)
        assert np.array_equal(nodes["left"], left) and np.array_equal(nodes["right"], right), name
        assert np.array_equal(axis, waxis) and depth == wdepth and rounds == wrounds, name
        assert np.array_equal(nodes["bmin"].view(np.uint32), np.array([b[0] for b in box]).view(np.uint32))
        assert np.array_equal(nodes["bmax"].view(np.uint32), np.array([b[1] for b in box]).view(np.uint32))


def test_ploc_invariants(abi):
    for name, sb in _scenes(abi):
        _, boxes, _, order = _keys(sb)
        for radius in (1, 16, 128):
            nodes, axis, depth, rounds = R.ploc(boxes, order, radius)
            left, right = nodes["left"], nodes["right"]
            _check_tree(left, right, order.tolist())
            for c in (left, right):  # children are numbered after their parents
                assert (c[c >= 0] > np.nonzero(c >= 0)[0]).all(), name
            assert depth == _recursive_depth(left, right), name
            for i in range(len(nodes)):  # boxes are the unions of the children's
                kids = [(nodes["bmin"][c], nodes["bmax"][c]) if c >= 0 else (boxes[0][~c], boxes[1][~c]) for c in (left[i], right[i])]
                assert np.array_equal(nodes["bmin"][i], np.minimum(kids[0][0], kids[1][0]))
                assert np.array_equal(nodes["bmax"][i], np.maximum(kids[0][1], kids[1][1]))


def test_duplicates_halve_and_chain_chains(abi):
    """Identical boxes must not merge one pair per round (the i ^ 1 rule), so the depth stays logarithmic; the chain scene
    is the opposite: one merge per round by construction, a tree as deep as it has primitives."""
    n = 600
    _, boxes, _, order = _keys(S.duplicates(abi, 0, n))
    for radius in (1, 2, 16, 64, 128):
        _, _, depth, rounds = R.ploc(boxes, order, radius)
        assert depth <= 2 * math.ceil(math.log2(n)) + 2 and rounds <= 2 * math.ceil(math.log2(n)) + 2, (radius, depth, rounds)
    _, boxes, _, order = _keys(S.chain(abi, 0))
    _, _, depth, _ = R.ploc(boxes, order, 16)
    assert depth == 40


# ------------------------------------------------------------------ pair records, quality
def test_pair_records_by_hand(abi):
    sb = abi.SceneBuilder()
    mat = sb.metal((0.5, 0.5, 0.5), 0.0)
    sb.add_sphere((0.0, 0.0, 0.0), 1.0, mat)
    sb.add_sphere((4.0, 0.0, 0.0), 1.0, mat, center1=(6.0, 0.0, 0.0), time0=0.0, time1=1.0)
    sb.add_triangles(np.array([[1, 2, 3], [4, 2, -1], [0, 2, 5]], F), np.zeros((3, 2), F), [[0, 1, 2]], mat)
    sb.world_bvh(0, 3, 0.0, 0.5, builder=abi.SRT_BUILDER_LBVH)
    sb.world_prim(0)  # times 0, 0
    sb.world_bvh(0, 2, 0.25, 2.0, builder=abi.SRT_BUILDER_PLOC)
    nodes = np.zeros(2, R.NODE_DTYPE)
    nodes["bmin"], nodes["bmax"] = [[0, 1, 2], [3, 4, 5]], [[6, 7, 8], [9, 10, 11]]
    nodes["left"], nodes["right"] = [1, ~1], [~2, R.REF_DONE]
    one = np.zeros(1, R.NODE_DTYPE)
    lay = R.Layout(sb, [nodes, None, one])
    assert lay.base == [0, None, 2] and lay.num_nodes == 3 and (lay.time0, lay.time1) == (0.0, 2.0)
    rec = R.pair_records(nodes, 5, lay)
    w = rec.view(np.int32)
    assert rec[0, 0:3].tolist() == [3, 4, 5] and rec[0, 4:7].tolist() == [9, 10, 11] and w[0, 3] == 6 << 6
    pad = F(0.0001)
    assert rec[0, 8:11].tolist() == [0, F(2) - pad, -1] and rec[0, 12:15].tolist() == [4, F(2) + pad, 5] and w[0, 7] == ~0
    # the moving sphere over the widest range [0, 2]: x from 4 - 1 to 8 + 1
    assert rec[1, 0:3].tolist() == [3, -1, -1] and rec[1, 4:7].tolist() == [9, 1, 1] and w[1, 3] == ~(1 << 1 | 1)
    assert rec[1, 8:11].tolist() == [1, 1, 1] and rec[1, 12:15].tolist() == [-1, -1, -1] and w[1, 7] == R.REF_DONE
    assert (w[:, [11, 15]] == 0).all()


def test_layout_renumbers_triangles_by_host_tree_order(abi):
    """Triangles are renumbered by first appearance in the host-built node arrays; the others follow in their own order."""
    sb = abi.SceneBuilder()
    mat = sb.metal((0.5, 0.5, 0.5), 0.0)
    sb.add_triangles(np.zeros((15, 3), F), np.zeros((15, 2), F), np.arange(15).reshape(5, 3), mat)
    nodes = np.zeros(2, R.NODE_DTYPE)
    nodes["left"], nodes["right"] = [~3, ~1], [1, ~4]
    sb.world_prebuilt(nodes, 1, 4)
    sb.world_bvh(0, 5, builder=abi.SRT_BUILDER_PLOC)
    lay = R.Layout(sb, [nodes, np.zeros(4, R.NODE_DTYPE)])
    assert lay.tri_dev.tolist() == [3, 1, 4, 0, 2] and lay.base == [0, 2]
    assert lay.device_ref(3) == ~0 and lay.device_ref(0) == ~(3 << 1)


def test_ploc_trees_are_tighter_than_the_linear_bvh(abi):
    """The header's claim on the soup of the device tests: the surface-area cost (sum of node areas over the root's) of the
    PLOC tree at the default radius is below the linear BVH's.  (DESIGN.md N2 records the figures.)"""
    sb = S.soup(abi, 3000, 0)
    refs = np.arange(3000)
    lb, _, _ = R.build_lbvh(sb, refs, 0.0, 1.0)
    costs = {r: R.sah_cost(R.build_ploc(sb, refs, 0.0, 1.0, r)[0]) for r in (1, 16, 64)}
    print("sah cost: lbvh %.3f ploc %s" % (R.sah_cost(lb), costs))
    assert costs[64] < R.sah_cost(lb) and costs[16] < R.sah_cost(lb)


@pytest.mark.parametrize("n", SIZES)
def test_builders_on_every_soup_size(abi, n):
    """Both replays end to end at the sizes of the device tests: a tree over the item's primitives, leaves as list indices."""
    sb = S.soup(abi, n, 0)
    refs = np.arange(n)
    for nodes, axis, depth in (R.build_lbvh(sb, refs, 0.0, 1.0), R.build_ploc(sb, refs, 0.0, 1.0, 128)):
        assert len(nodes) == len(axis) == n - 1
        _check_tree(nodes["left"], nodes["right"], list(range(n)))
        assert depth == _recursive_depth(nodes["left"], nodes["right"])
    one = R.build_ploc(S.soup(abi, 2, 0), [1], 0.0, 1.0, 4)
    assert one[0]["left"][0] == one[0]["right"][0] == ~1 and one[1].tolist() == [3] and one[2] == 1
