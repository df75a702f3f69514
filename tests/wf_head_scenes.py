"""Scenes of the head-of-walk tests (csrc/srt_regroup.h SrtRegroupWalk::head; tests/test_wf_head_host.py on the CPU,
tests/test_gpu_wf_head.py on the device) and the hook srtTestWfHead.  No test lives here.

The reference builder (bvh.h:55-95) sorts a range by box minimum on a random axis and halves it, the left half taking
floor(n / 2): the ground sphere (radius 1000) has the lowest minimum on every axis and ends up in the tree's first leaf
whatever the axes drawn, next to whatever sorts second, or alone where the leftmost range halves down to three.  So the
primitive COUNT and one object that is second-lowest on every axis decide what the head leaf holds:
    48 = 3 * 2^4 primitives                         -> the ground alone
    42 -> 21 -> 10 -> 5 -> 2, a low sphere in it    -> the ground and that sphere
    41 -> 20 -> 10 -> 5 -> 2, triangles alone       -> the ground and a triangle: no head"""
import numpy as np

F = np.float32


def _soup(sb, rng, count, material):
    """`count` triangles with corners inside [-3, 3] x [0.5, 6.5] x [-3, 3]"""
    c = rng.uniform(-2.5, 2.5, (count, 1, 3)) + np.array([0.0, 3.5, 0.0])
    v = (c + rng.uniform(-0.5, 0.5, (count, 3, 3))).astype(F)
    sb.add_triangles(v.reshape(-1, 3), rng.random((3 * count, 2)).astype(F), np.arange(3 * count).reshape(-1, 3), material)


def _materials(sb):
    return sb.metal((0.7, 0.6, 0.5), 0.1), sb.metal((0.5, 0.5, 0.5), 0.4), sb.light((6.0, 5.0, 4.0))


def ground_alone(abi):
    """The ground, a 40-triangle soup and seven small spheres above it: 48 primitives, the head leaf holds the ground alone
    (sphere 0 of the scene)."""
    rng = np.random.default_rng(31)
    sb = abi.SceneBuilder()
    tri, ground, lamp = _materials(sb)
    _soup(sb, rng, 40, tri)
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, ground)
    for k in range(7):
        p = rng.uniform(-2.5, 2.5, 3) + np.array([0.0, 3.5, 0.0])
        sb.add_sphere(tuple(float(x) for x in p), float(rng.uniform(0.2, 0.5)), lamp if k == 0 else tri)
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


def ground_and_moving(abi):
    """The ground, a 40-triangle soup and one MOVING sphere whose box is the second-lowest on every axis: 42 primitives, the
    head leaf holds the ground and, as its second object, the moving sphere."""
    rng = np.random.default_rng(32)
    sb = abi.SceneBuilder()
    tri, ground, _ = _materials(sb)
    _soup(sb, rng, 40, tri)
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, ground)
    sb.add_sphere((-4.5, 1.2, -4.5), 1.1, tri, center1=(-4.5, 2.4, -4.5), time0=0.0, time1=1.0)
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


def ground_and_triangle(abi):
    """The ground and a 40-triangle soup: 41 primitives, the first leaf holds the ground and a triangle -- no head."""
    rng = np.random.default_rng(33)
    sb = abi.SceneBuilder()
    tri, ground, _ = _materials(sb)
    _soup(sb, rng, 40, tri)
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, ground)
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


def two_spheres(abi):
    """A world that is one leaf of two spheres: the tree is its root, the head's miss word is DONE."""
    sb = abi.SceneBuilder()
    tri, ground, _ = _materials(sb)
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, ground)
    sb.add_sphere((0.0, 1.5, 0.0), 1.5, tri)
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


def two_items(abi):
    """ground_alone's primitives as a world of two items, the ground a bare primitive in front of the tree -- no head."""
    sb = ground_alone(abi)
    sb.world = []
    sb.world_prim(40)
    sb.world_bvh(0, 40, 0.0, 1.0)
    return sb


def kinds_of(abi, sb):
    """kinds[prim] of a scene: 1 = a sphere (srtTestWfHead's list)."""
    prims = np.concatenate(sb._prim_chunks)
    return (prims[:, 0] == abi.SRT_PRIM_SPHERE).astype(np.uint8)


def head_host(dev, arr, world, kinds):
    """srtTestWfHead -> (rc, head word)."""
    import ctypes as C
    arr = np.ascontiguousarray(arr, F)
    world = np.ascontiguousarray(world, np.int32)
    kinds = np.ascontiguousarray(kinds, np.uint8)
    head = C.c_int32(-1)
    rc = dev.lib.srtTestWfHead(arr.ctypes.data, len(arr), world.ctypes.data, len(world), kinds.ctypes.data, len(kinds), C.byref(head))
    return rc, head.value


def device_ref(prim, sphere):
    """The device's reference of primitive `prim` of a kinds list: ~(index << 1 | sphere)."""
    return ~(prim << 1 | (1 if sphere else 0))
