"""The small scenes the tree-builder tests share (tests/test_tree_build_ref.py on the CPU, tests/test_gpu_tree_builders.py on
the device): each reaches one edge of csrc/srt_lbvh.hip at the smallest size that does.  `abi` is the package's abi module."""
import numpy as np

F = np.float32


def _materials(sb):
    return sb.pbr(albedo_tex=sb.solid(200, 150, 100), metalness=0.0, roughness=0.5), sb.metal((0.7, 0.6, 0.5), 0.1)


def _add_soup(sb, rng, n, mats, centre=(0.0, 3.0, -1.0), extent=3.0):
    """n primitives in list order: half of the triangles, the spheres (static ones, then moving ones; a moving sphere's own
    times are [0.25, 0.75], so the item's [time0, time1] extrapolates its path), the other triangles."""
    n_mov = max(1, n // 5)
    n_stat = max(1, n // 5) if n >= 3 else 0
    n_tri = n - n_mov - n_stat
    assert n_tri >= 1
    c = (rng.random((n_tri, 1, 3), dtype=F) - F(0.5)) * F(2 * extent) + np.array(centre, F)
    v = (c + (rng.random((n_tri, 3, 3), dtype=F) - F(0.5)) * F(0.6)).astype(F)

    def tris(a):
        if len(a):
            sb.add_triangles(a.reshape(-1, 3), np.zeros((3 * len(a), 2), F), np.arange(3 * len(a), dtype=np.int32).reshape(-1, 3), mats[0])

    tris(v[:n_tri // 2])
    for k in range(n_stat + n_mov):
        c0 = (rng.random(3, dtype=F) - F(0.5)) * F(2 * extent) + np.array(centre, F)
        r = float(F(0.05) + rng.random(dtype=F) * F(0.35))
        if k >= n_stat:
            c1 = c0 + (rng.random(3, dtype=F) - F(0.5)) * F(0.8)
            sb.add_sphere(tuple(c0.tolist()), r, mats[1], center1=tuple(c1.tolist()), time0=0.25, time1=0.75)
        else:
            sb.add_sphere(tuple(c0.tolist()), r, mats[1])
    tris(v[n_tri // 2:])


def soup(abi, n, builder, seed=11):
    """A. Mixed soup: random triangles, static and moving spheres; one item over [0, 1]."""
    sb = abi.SceneBuilder()
    _add_soup(sb, np.random.default_rng(seed + n), n, _materials(sb))
    assert sb.num_prims == n
    sb.world_bvh(0, None, 0.0, 1.0, builder=builder)
    return sb


def duplicates(abi, builder, n=600):
    """B. Two stacks of identical triangles: keys equal up to the index word, every PLOC area of a stack ties."""
    sb = abi.SceneBuilder()
    tri = np.array([[-1.0, 2.0, -1.0], [1.0, 2.0, -1.0], [0.0, 4.0, -1.0]], F)
    pos = np.tile(tri, (n, 1))
    pos[3 * (n // 2):] += F(2.5)
    sb.add_triangles(pos, np.zeros((3 * n, 2), F), np.arange(3 * n, dtype=np.int32).reshape(-1, 3), _materials(sb)[0])
    sb.world_bvh(0, None, 0.0, 1.0, builder=builder)
    return sb


def flat(abi, builder, nx=15, ny=10):
    """C. Axis-aligned right triangles tiling a rectangle of the plane z = -1.5, two per cell (2 nx ny = 300): every box is
    padded on z, the centroids have no extent on z, and the two triangles of a cell share one box."""
    sb = abi.SceneBuilder()
    pos = []
    for j in range(ny):
        for i in range(nx):
            x0, y0, x1, y1, z = 0.5 * i - 3.0, 0.5 * j + 1.0, 0.5 * i - 2.5, 0.5 * j + 1.5, -1.5
            pos += [[x0, y0, z], [x1, y0, z], [x0, y1, z], [x1, y1, z], [x0, y1, z], [x1, y0, z]]
    pos = np.array(pos, F)
    sb.add_triangles(pos, np.zeros((len(pos), 2), F), np.arange(len(pos), dtype=np.int32).reshape(-1, 3), _materials(sb)[0])
    sb.world_bvh(0, None, 0.0, 1.0, builder=builder)
    return sb


def concentric(abi, builder, n=64):
    """D. Concentric spheres (centre and radii dyadic, so every centroid is the centre exactly): one Morton code."""
    sb = abi.SceneBuilder()
    m = _materials(sb)[1]
    for i in range(n):
        sb.add_sphere((0.5, 3.0, -1.0), (i + 1) / 32.0, m)
    sb.world_bvh(0, None, 0.0, 1.0, builder=builder)
    return sb


def chain(abi, builder, n=40, ratio=1.5):
    """E. Spheres on a line, spacing and radius growing geometrically: every sphere's cheapest partner is the cluster below
    it, so PLOC merges one pair per round into a chain.  (The line is the x axis: the centroids are exactly 0 on y and z,
    so the Morton order is the order along the line.)"""
    sb = abi.SceneBuilder()
    m = _materials(sb)[1]
    for i in range(n):
        x = ratio ** i
        sb.add_sphere((x, 0.0, 0.0), 0.1 * x, m)
    sb.world_bvh(0, None, 0.0, 1.0, builder=builder)
    return sb


def chain_rays(abi, count=5000, n=40, ratio=1.5, seed=4):
    """Rays at the chain's spheres: half from one point near the small end (they run along the line and stop at the first
    sphere in the way), half from beside the sphere they aim at, at a distance in proportion to it."""
    rng = np.random.default_rng(seed)
    rays = np.zeros(count, abi.RAY_DTYPE)
    x = ratio ** rng.integers(0, n, count)
    target = np.stack([x * (1.0 + 0.12 * rng.normal(size=count)), 0.1 * x * rng.normal(size=count), np.zeros(count)], axis=1)
    origin = np.where((np.arange(count) % 2 == 0)[:, None], np.array([0.0, 0.2, 1.5]), np.stack([0.7 * x, 0.2 * x, 1.5 * x], axis=1))
    rays["o"] = origin.astype(F)
    rays["d"] = (target - origin).astype(F)
    rays["tMin"], rays["tMax"] = 0.001, np.inf
    return rays


def four_items(abi):
    """F. A world of a host-built item, a linear-BVH item, a PLOC item and a lone primitive, about 300 primitives and
    another time range each.  The host-built item's primitives are NOT the first of the list, so the flattening renumbers
    the triangles of all three, and the device-built trees lie at a base other than 0."""
    sb = abi.SceneBuilder()
    mats = _materials(sb)
    rng = np.random.default_rng(23)
    _add_soup(sb, rng, 301, mats, centre=(-3.0, 3.0, -1.0), extent=1.5)   # prims [0, 301): the linear BVH's
    _add_soup(sb, rng, 300, mats, centre=(0.0, 3.0, -1.0), extent=1.5)    # [301, 601): the host-built tree's
    _add_soup(sb, rng, 299, mats, centre=(3.0, 3.0, -1.0), extent=1.5)    # [601, 900): PLOC's
    lone = sb.add_sphere((0.0, 6.0, -1.0), 0.5, mats[1])
    sb.world_bvh(301, 300, 0.0, 1.0)
    sb.world_bvh(0, 301, 0.25, 0.5, builder=abi.SRT_BUILDER_LBVH)
    sb.world_bvh(601, 299, 0.5, 2.0, builder=abi.SRT_BUILDER_PLOC)
    sb.world_prim(lone)
    return sb


def random_rays(abi, count=5000, seed=9, with_time=True):
    rng = np.random.default_rng(seed)
    rays = np.zeros(count, abi.RAY_DTYPE)
    rays["o"] = (0.0, 3.0, 5.0)
    rays["d"] = rng.normal(size=(count, 3)).astype(F) * F(0.5) + np.array([0.0, 0.0, -1.0], F)
    if with_time:
        rays["time"] = rng.random(count).astype(F)
    rays["tMin"], rays["tMax"] = 0.001, np.inf
    return rays
