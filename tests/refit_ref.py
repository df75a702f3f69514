"""NumPy float32 replay of srtRefitScene (csrc/srt_refit.hip): primitive boxes by the reference's rules
(tree_build_ref.prim_boxes: model.h:183-212, sphere.h:85-94), then min / max unions over a GIVEN topology.  No GPU and no
library.  Trees are in Context.bvh's convention (tree_build_ref's docstring): a child >= 0 is a node of the same item, a
child < 0 is ~(index into prims[]), left == right is a single-object leaf; node 0 is the root.  Nothing is assumed about
the numbering beyond that (a linear BVH's children may have smaller indices than their parents)."""
import copy

import numpy as np

import tree_build_ref as R

F = np.float32


def moved_scene(sb, triangles=None, spheres=None):
    """A copy of the scene builder `sb` with other geometry: triangles = an abi.TRIANGLE_DTYPE array over all of the scene's
    triangles (its own order), spheres = a list of SrtSphereIn.  Materials, the primitive list and the world are shared."""
    out = copy.copy(sb)
    out._keep = None
    if triangles is not None:
        assert len(triangles) == sb._tri_count
        out.triangles = [np.ascontiguousarray(triangles)]
    if spheres is not None:
        assert len(spheres) == len(sb.spheres)
        out.spheres = list(spheres)
    return out


def scene_triangles(sb):
    """All triangles of a scene builder as one array, in the scene's order."""
    return np.concatenate(sb.triangles).copy()


def post_order(nodes):
    """Node indices, children before parents, of the tree under node 0."""
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        l, r = int(nodes["left"][i]), int(nodes["right"][i])
        if l >= 0:
            stack.append(l)
        if r >= 0 and r != l:
            stack.append(r)
    return order[::-1]


def refit(scene, nodes, time0, time1):
    """The item's nodes with every box recomputed from `scene`'s primitives over [time0, time1]: a primitive child's box
    from prim_boxes, a node child's box that node's new box, the node's box their union (aabb.h:33-43: min of the
    minima, max of the maxima).  The child words are returned as they came."""
    out = nodes.copy()
    n = len(nodes)
    ch = np.stack([nodes["left"], nodes["right"]], axis=1).astype(np.int64)
    mn = np.full((n, 2, 3), np.inf, F)
    mx = np.full((n, 2, 3), -np.inf, F)
    prim = ch < 0
    if prim.any():
        pmn, pmx = R.prim_boxes(scene, ~ch[prim], time0, time1)
        mn[prim], mx[prim] = pmn, pmx
    for i in post_order(nodes):
        for c in range(2):
            j = ch[i, c]
            if j >= 0:
                mn[i, c], mx[i, c] = out["bmin"][j], out["bmax"][j]
        out["bmin"][i] = np.minimum(mn[i, 0], mn[i, 1])
        out["bmax"][i] = np.maximum(mx[i, 0], mx[i, 1])
    return out


def refit_world(scene, item_nodes):
    """refit over every tree of a world: item_nodes[w] as Context.bvh(w) gives it (None for a lone primitive), each with its
    own item's (time0, time1)."""
    sc = R.arrays(scene)
    return [None if nodes is None else refit(sc, nodes, sc.world[w]["time0"], sc.world[w]["time1"])
            for w, nodes in enumerate(item_nodes)]


def pair_records_world(scene, item_nodes):
    """The closest-hit pair records of every tree (tree_build_ref.pair_records), [w] -> (n, 16) float32 or None."""
    layout = R.Layout(scene, item_nodes)
    return [None if nodes is None else R.pair_records(nodes, layout.base[w], layout) for w, nodes in enumerate(item_nodes)]


def fast_div_certified(item_nodes):
    """srt_scene.cpp's certificate over the node boxes: every coordinate 0 or 2^-77 <= |c| <= 2^30."""
    ok = True
    for nodes in item_nodes:
        if nodes is None:
            continue
        c = np.abs(np.concatenate([nodes["bmin"].reshape(-1), nodes["bmax"].reshape(-1)]))
        ok = ok and bool(((c == 0) | ((c >= F(2.0 ** -77)) & (c <= F(2.0 ** 30)))).all())
    return ok
