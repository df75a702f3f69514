"""NumPy replay of the device tree builders (csrc/srt_lbvh.hip), one function per kernel, in the kernels' operation order.

Everything that is a float in the kernels is a float32 here and is combined in the order the file's comments state (the
library is built without multiply-add contraction and with IEEE division), so the results are meant to be compared with
the device's on bits.  No GPU and no library: a scene is an abi.SceneBuilder (or anything with its `triangles`,
`spheres`, `_prim_chunks` and `world` attributes).

Two facts come from the host code around the kernels and are relied on here.

The order of `refs` (srt_scene.cpp flattenScene, DeviceBuild::refs).  A device-built world item {first, count} hands the
builder its primitives in list order: refs[i] is the device reference of prims[first + i], i = 0 .. count - 1.  The low
word of a Morton key is that i, so equal Morton codes sort by list position, and PLOC's first round sees the primitives
in (code, i) order.  A device reference is ~(index << 1 | 1) for sphere `index` and ~(devIndex << 1) for a triangle, where
devIndex is the triangle's own index unless the world has host-built trees: then the triangles are renumbered by their
first appearance in the host-built node arrays (world order, node order, left before right) and the triangles no
host-built tree references follow in their own order (`Layout.tri_dev`).

The mapping of srtGetBvh (srt_api.cpp).  What Context.bvh(item) returns is the item's slice of the device node array
with node references made item-local (scene-wide node index minus the item's base) and primitive references turned back
into ~(index into prims[]).  The functions here speak that convention: a child >= 0 is a node of the same item, a child
< 0 is ~listPrim; `refs` arguments are list primitive indices.  Only pair_records, whose records hold what the traversal
reads, produces scene-wide record offsets (index << 6) and device primitive references.
"""
import numpy as np

F = np.float32
NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("left", "<i4"), ("bmax", "<f4", 3), ("right", "<i4")])
PRIM_TRIANGLE, PRIM_SPHERE = 0, 1
WORLD_PRIM, WORLD_BVH = 0, 1
BUILDER_REFERENCE, BUILDER_LBVH, BUILDER_PLOC = 0, 1, 2
REF_DONE = -2 ** 31  # an unused child slot (pair_records: the empty box)
PLOC_MAX_RADIUS = 128
PAD = F(0.0001)


# ------------------------------------------------------------------ the scene as arrays
class SceneArrays:
    """The arrays of a SceneBuilder the builders read."""

    def __init__(self, sb):
        tri = np.concatenate(sb.triangles) if sb.triangles else None
        self.tri = np.ascontiguousarray(tri["p"], F) if tri is not None else np.zeros((0, 3, 3), F)
        s = sb.spheres
        self.c0 = np.array([list(x.center0) for x in s], F).reshape(-1, 3)
        self.c1 = np.array([list(x.center1) for x in s], F).reshape(-1, 3)
        self.st0 = np.array([x.time0 for x in s], F)
        self.st1 = np.array([x.time1 for x in s], F)
        self.radius = np.array([x.radius for x in s], F)
        self.prims = np.concatenate(sb._prim_chunks) if sb._prim_chunks else np.zeros((0, 2), np.int32)
        self.world = [dict(kind=w.kind, first=w.first, count=w.count, time0=F(w.time0), time1=F(w.time1), builder=w.builder,
                           prebuilt=w.numNodes > 0) for w in sb.world]


def arrays(scene):
    return scene if isinstance(scene, SceneArrays) else SceneArrays(scene)


# ------------------------------------------------------------------ primBox / lbvhPrimBoxes
def prim_boxes(scene, refs, time0, time1):
    """(mn, mx), (n, 3) float32 each: the boxes of the list primitives `refs` over [time0, time1].  A triangle: min / max
    of its vertices, an axis on which they are equal padded by 0.0001 on either side.  A sphere: centre -+ radius at both
    times, the centre of a moving one (center0 != center1) being c0 + ((t - t0) / (t1 - t0)) * (c1 - c0)."""
    sc = arrays(scene)
    refs = np.asarray(refs, np.int64).reshape(-1)
    time0, time1 = F(time0), F(time1)
    mn, mx = np.zeros((len(refs), 3), F), np.zeros((len(refs), 3), F)
    kind, index = sc.prims[refs, 0], sc.prims[refs, 1]
    t = kind == PRIM_TRIANGLE
    if t.any():
        v = sc.tri[index[t]]
        # model.h:191-197: std::min / std::max folded over the vertices in order from +-infinity, so of two zeros of
        # opposite sign the first one seen stays (NumPy's min / max leave that open)
        lo, hi = np.full(v[:, 0].shape, np.inf, F), np.full(v[:, 0].shape, -np.inf, F)
        for k in range(3):
            lo = np.where(v[:, k] < lo, v[:, k], lo)
            hi = np.where(hi < v[:, k], v[:, k], hi)
        flat = lo == hi
        mn[t] = np.where(flat, lo - PAD, lo)
        mx[t] = np.where(flat, hi + PAD, hi)
    s = ~t
    if s.any():
        k = index[s]
        c0, c1, r = sc.c0[k], sc.c1[k], sc.radius[k][:, None]
        moving = (c0 != c1).any(axis=1)[:, None]
        span = (sc.st1[k] - sc.st0[k])[:, None]
        with np.errstate(all="ignore"):
            a = c0 + ((time0 - sc.st0[k])[:, None] / span) * (c1 - c0)
            b = c0 + ((time1 - sc.st0[k])[:, None] / span) * (c1 - c0)
        a, b = np.where(moving, a, c0).astype(F), np.where(moving, b, c0).astype(F)
        mn[s] = np.minimum(a - r, b - r)
        mx[s] = np.maximum(a + r, b + r)
    return mn, mx


# ------------------------------------------------------------------ lbvhMorton
def _expand_bits(v):
    """10 bits -> every third bit."""
    v = v.astype(np.uint64)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton_keys(boxes):
    """uint64 keys: the 30-bit Morton code of each centroid (x, y, z interleaved, z lowest) in the high word, the position
    in `boxes` in the low word.  Centroids 0.5 * (mn + mx) are scaled to the bounds of all centroids, u = 0 on an axis
    without extent, and quantised by truncating min(max(u * 1024, 0), 1023)."""
    mn, mx = boxes
    c = (F(0.5) * (mn + mx)).astype(F)
    lo, hi = c.min(axis=0), c.max(axis=0)
    ext = (hi - lo).astype(F)
    with np.errstate(all="ignore"):
        u = np.where(ext > 0, (c - lo) / np.where(ext > 0, ext, F(1)), F(0)).astype(F)
    q = np.minimum(np.maximum(u * F(1024), F(0)), F(1023)).astype(F).astype(np.uint32)
    m = (_expand_bits(q[:, 0]) << np.uint64(2)) | (_expand_bits(q[:, 1]) << np.uint64(1)) | _expand_bits(q[:, 2])
    return (m << np.uint64(32)) | np.arange(len(c), dtype=np.uint64)


def sort_keys(keys):
    """(sorted keys, order): order[s] = the position in refs of the primitive at sorted position s."""
    order = np.argsort(keys, kind="stable")
    return keys[order], order.astype(np.int64)


def _leaf(refs, order, s):
    return ~int(refs[order[s]])


def _single(scene, refs, time0, time1):
    mn, mx = prim_boxes(scene, refs, time0, time1)
    nodes = np.zeros(1, NODE_DTYPE)
    nodes["bmin"], nodes["bmax"] = mn, mx
    nodes["left"] = nodes["right"] = ~int(refs[0])
    return nodes, np.full(1, 3, np.uint8), 1


# ------------------------------------------------------------------ lbvhHierarchy + lbvhFit
def lbvh(keys):
    """The binary radix tree over the sorted unique keys with Karras' numbering.  Returns (left, right, axis, depth):
    children >= 0 are nodes, < 0 are ~sortedPosition.

    delta(i, j) is the length of the common prefix of keys i and j (-1 outside the array).  Node i sits at one end of its
    range; the range grows towards the neighbour with the longer common prefix, as far as the prefix stays longer than
    the one shared with the other neighbour.  The split gamma is the last position that shares more than the range's own
    prefix with node i's end; the children are gamma (left) and gamma + 1 (right), leaves where a child's range is one
    key.  The first differing bit names the axis: Morton bits 61..32 cycle x, y, z (z lowest), an index bit gives 3."""
    k = [int(x) for x in keys]
    n = len(k)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        return 64 - (k[i] ^ k[j]).bit_length()

    left, right, axis = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32), np.zeros(n - 1, np.uint8)
    parent = {}
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) >= delta(i, i - 1) else -1
        dmin = delta(i, i - d)
        length = 0  # the other end: the farthest j = i + length * d with delta(i, j) > dmin (monotone in length)
        step = 1
        while delta(i, i + (length + step) * d) > dmin:  # gallop, then bisect
            length += step
            step *= 2
        while step >= 1:
            if delta(i, i + (length + step) * d) > dmin:
                length += step
            step //= 2
        j = i + length * d
        lo, hi = min(i, j), max(i, j)
        own = delta(lo, hi)
        g = lo  # the last position of [lo, hi) sharing more than `own` bits with lo
        step = 1
        while step * 2 <= hi - lo:
            step *= 2
        while step >= 1:
            if g + step < hi and delta(lo, g + step) > own:
                g += step
            step //= 2
        left[i] = ~g if g == lo else g
        right[i] = ~(g + 1) if g + 1 == hi else g + 1
        for c in (left[i], right[i]):
            if c >= 0:
                parent[int(c)] = i
        bit = 63 - own
        axis[i] = 2 - (bit - 32) % 3 if bit >= 32 else 3
    # depth: node records on the longest root-to-primitive chain, plus one
    level = np.zeros(n - 1, np.int64)
    level[0] = 1
    todo = [0]
    while todo:
        i = todo.pop()
        for c in (int(left[i]), int(right[i])):
            if c >= 0:
                level[c] = level[i] + 1
                todo.append(c)
    return left, right, axis, int(level.max()) + 1


def _fit(left, right, leaf_mn, leaf_mx):
    """Node boxes = min / max unions of the children's (children as in lbvh: < 0 is ~index into leaf_mn / leaf_mx)."""
    n = len(left)
    mn, mx = np.zeros((n, 3), F), np.zeros((n, 3), F)
    done = np.zeros(n, bool)
    stack = [0]
    while stack:
        i = stack[-1]
        kids = [int(left[i]), int(right[i])]
        wait = [c for c in kids if c >= 0 and not done[c]]
        if wait:
            stack.extend(wait)
            continue
        stack.pop()
        a = [(mn[c], mx[c]) if c >= 0 else (leaf_mn[~c], leaf_mx[~c]) for c in kids]
        mn[i] = np.minimum(a[0][0], a[1][0])
        mx[i] = np.maximum(a[0][1], a[1][1])
        done[i] = True
    return mn, mx


def build_lbvh(scene, refs, time0, time1):
    """srt_lbvh_build of the list primitives `refs`: (nodes as Context.bvh returns them, axis, depth)."""
    refs = np.asarray(refs, np.int64)
    if len(refs) == 1:
        return _single(scene, refs, time0, time1)
    boxes = prim_boxes(scene, refs, time0, time1)
    keys, order = sort_keys(morton_keys(boxes))
    left, right, axis, depth = lbvh(keys)
    mn, mx = _fit(left, right, boxes[0][order], boxes[1][order])
    nodes = np.zeros(len(refs) - 1, NODE_DTYPE)
    nodes["bmin"], nodes["bmax"] = mn, mx
    nodes["left"] = [c if c >= 0 else _leaf(refs, order, ~c) for c in left.tolist()]
    nodes["right"] = [c if c >= 0 else _leaf(refs, order, ~c) for c in right.tolist()]
    return nodes, axis, depth


# ------------------------------------------------------------------ plocInit .. plocMerge
def _union_area(amn, amx, bmn, bmx):
    d = (np.maximum(amx, bmx) - np.minimum(amn, bmn)).astype(F)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):
        return ((dx * dy + dy * dz) + dz * dx).astype(F)


def ploc_nearest(mn, mx, radius):
    """nn[i]: the position within `radius` places of i whose union with cluster i has the smallest area; among equal
    areas the pair partner i ^ 1, then the lowest position."""
    m = len(mn)
    i = np.arange(m)
    offs = np.array([d for d in range(-radius, radius + 1) if d != 0 and abs(d) < m], np.int64)  # ascending j
    j = i[:, None] + offs[None, :]
    ok = (j >= 0) & (j < m)
    jc = np.clip(j, 0, m - 1)
    area = _union_area(mn[:, None, :], mx[:, None, :], mn[jc], mx[jc])
    area = np.where(ok & (area < F(3.0e38)), area, np.inf)  # the kernel's search starts from 3.0e38
    col = np.argmin(area, axis=1)  # the first of equal minima = the lowest position
    best = area[i, col]
    nn = np.where(np.isfinite(best), j[i, col], -1)
    partner = i ^ 1
    inwin = (partner < m) & (np.abs(partner - i) <= radius)
    pa = _union_area(mn, mx, mn[np.minimum(partner, m - 1)], mx[np.minimum(partner, m - 1)])
    # (an area of exactly 3.0e38 at the partner also wins in the kernel; no finite scene of the tests comes near it)
    nn = np.where(inwin & np.isfinite(best) & (pa == best), partner, nn)
    return nn.astype(np.int64)


def ploc(boxes, order, radius, refs=None):
    """The PLOC rounds over the primitive boxes (`boxes` in refs order, `order` from sort_keys).  Returns (nodes, axis,
    depth, rounds): nodes in NODE_DTYPE with leaves ~order[s] (or ~refs[order[s]]), node indices (n - 2) - creation order.

    Per round: nearest neighbours (ploc_nearest); mutual pairs merge, the lower position leads and keeps its place, the
    other one leaves the array; nodes are created in position order.  A node's axis is the one on which the two centroid
    sums (mn + mx) differ most, x before y before z on equal differences, its left child the leader when the other's
    sum is not below the leader's there; axis 3 when they do not differ.  depth = max of the children's + 1, leaves 1."""
    bmn, bmx = boxes
    n = len(order)
    radius = min(max(int(radius), 1), PLOC_MAX_RADIUS)
    mn, mx = bmn[order].astype(F), bmx[order].astype(F)
    src = order if refs is None else np.asarray(refs, np.int64)[order]
    ref = (~src).astype(np.int64)  # < 0 leaf, >= 0 node
    depth = np.ones(n, np.int64)
    nodes = np.zeros(n - 1, NODE_DTYPE)
    axis_out = np.full(n - 1, 3, np.uint8)
    made = rounds = 0
    while len(mn) > 1:
        m = len(mn)
        nn = ploc_nearest(mn, mx, radius)
        i = np.arange(m)
        mutual = (nn >= 0) & (nn[np.maximum(nn, 0)] == i)
        lead = mutual & (i < nn)
        gone = mutual & (i > nn)
        L = np.nonzero(lead)[0]
        assert len(L) >= 1, "no mutual pair"
        O = nn[L]
        node = (n - 2) - (made + np.arange(len(L)))
        diff = ((mn[O] + mx[O]).astype(F) - (mn[L] + mx[L]).astype(F)).astype(F)
        ad = np.abs(diff)
        ax = np.where(ad[:, 0] >= ad[:, 1], np.where(ad[:, 0] >= ad[:, 2], 0, 2), np.where(ad[:, 1] >= ad[:, 2], 1, 2))
        dsel = diff[np.arange(len(L)), ax]
        me_first = dsel >= 0
        umn, umx = np.minimum(mn[L], mn[O]), np.maximum(mx[L], mx[O])
        nodes["bmin"][node], nodes["bmax"][node] = umn, umx
        nodes["left"][node] = np.where(me_first, ref[L], ref[O])
        nodes["right"][node] = np.where(me_first, ref[O], ref[L])
        axis_out[node] = np.where(dsel == 0, 3, ax)
        mn, mx, ref, depth = mn.copy(), mx.copy(), ref.copy(), depth.copy()
        mn[L], mx[L], ref[L] = umn, umx, node
        depth[L] = np.maximum(depth[L], depth[O]) + 1
        keep = ~gone
        mn, mx, ref, depth = mn[keep], mx[keep], ref[keep], depth[keep]
        made += len(L)
        rounds += 1
    assert made == n - 1
    return nodes, axis_out, int(depth[0]), rounds


def build_ploc(scene, refs, time0, time1, radius):
    """srt_ploc_build of the list primitives `refs`: (nodes as Context.bvh returns them, axis, depth)."""
    refs = np.asarray(refs, np.int64)
    if len(refs) == 1:
        return _single(scene, refs, time0, time1)
    boxes = prim_boxes(scene, refs, time0, time1)
    _, order = sort_keys(morton_keys(boxes))
    nodes, axis, depth, _ = ploc(boxes, order, radius, refs)
    return nodes, axis, depth


# ------------------------------------------------------------------ the node array of a world, pairNodes
class Layout:
    """Where the trees of a world lie in the scene-wide node array, and the device numbering of its triangles.
    item_nodes[w]: the item's nodes as Context.bvh(w) returns them (None for a lone primitive)."""

    def __init__(self, scene, item_nodes):
        sc = self.scene = arrays(scene)
        self.item_nodes = item_nodes
        self.base, at = [], 0
        for w, it in enumerate(sc.world):
            self.base.append(at if it["kind"] == WORLD_BVH else None)
            if it["kind"] == WORLD_BVH:
                assert not self.device_built(w) or len(item_nodes[w]) == max(it["count"] - 1, 1)
                at += len(item_nodes[w])
        self.num_nodes = at
        self.time0 = min(it["time0"] for it in sc.world)
        self.time1 = max(it["time1"] for it in sc.world)
        nt = len(sc.tri)
        self.tri_dev = np.arange(nt, dtype=np.int64)
        seen = []
        for w, it in enumerate(sc.world):
            if it["kind"] == WORLD_BVH and not self.device_built(w):
                lr = np.stack([item_nodes[w]["left"], item_nodes[w]["right"]], axis=1).reshape(-1)
                p = ~lr[lr < 0].astype(np.int64)
                seen.append(sc.prims[p, 1][sc.prims[p, 0] == PRIM_TRIANGLE])
        if nt > 1 and seen and sum(len(s) for s in seen):
            first = np.concatenate(seen)
            _, idx = np.unique(first, return_index=True)
            ordered = first[np.sort(idx)]
            rest = np.setdiff1d(np.arange(nt), ordered)
            self.tri_dev[np.concatenate([ordered, rest])] = np.arange(nt)

    def device_built(self, w):
        it = self.scene.world[w]
        return it["kind"] == WORLD_BVH and not it["prebuilt"] and it["builder"] in (BUILDER_LBVH, BUILDER_PLOC)

    def device_ref(self, prim):
        kind, index = self.scene.prims[prim]
        return ~((int(index) << 1) | 1) if kind == PRIM_SPHERE else ~(int(self.tri_dev[index]) << 1)


def pair_records(nodes, base, layout):
    """pairNodes over one item's nodes (Context.bvh convention) lying at `base` of the scene-wide array: (n, 16) float32,
    {left min, left ref, left max, right ref, right min, 0, right max, 0}.  A node child: that node's own box and its
    record's byte offset (scene-wide index << 6).  A primitive child: its box over the scene-wide [min time0, max time1]
    and its device reference.  An unused slot (REF_DONE): the empty box (1, 1, 1) / (-1, -1, -1), the reference kept."""
    n = len(nodes)
    out = np.zeros((n, 16), F)
    words = out.view(np.int32)
    for c, (name, at, refat) in enumerate((("left", 0, 3), ("right", 8, 7))):
        ch = nodes[name].astype(np.int64)
        isnode = ch >= 0
        unused = ch == REF_DONE
        prim = ~isnode & ~unused
        mn, mx = np.zeros((n, 3), F), np.zeros((n, 3), F)
        ref = np.zeros(n, np.int64)
        mn[isnode], mx[isnode] = nodes["bmin"][ch[isnode]], nodes["bmax"][ch[isnode]]
        ref[isnode] = (ch[isnode] + base) << 6
        mn[unused], mx[unused], ref[unused] = F(1), F(-1), REF_DONE
        if prim.any():
            p = ~ch[prim]
            mn[prim], mx[prim] = prim_boxes(layout.scene, p, layout.time0, layout.time1)
            ref[prim] = [layout.device_ref(int(x)) for x in p]
        out[:, at:at + 3], out[:, at + 4:at + 7] = mn, mx
        words[:, refat] = ref.astype(np.int32)
    return out


# ------------------------------------------------------------------ tree quality
def sah_cost(nodes):
    """Sum of the node boxes' surface areas over the root's (node 0), in float64."""
    d = nodes["bmax"].astype(np.float64) - nodes["bmin"].astype(np.float64)
    area = d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]
    return float(area.sum() / area[0])
