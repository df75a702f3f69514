"""Scenes and ray classes of the certified triangle test's tests (tests/test_tri_cert_host.py, tests/test_gpu_tri_cert.py):
rays built around a scene's own triangles -- random ones in and around a triangle, rays aimed at float points on its edges
and at its vertices, origins on its plane, grazing directions (|n . d| around FLT_EPSILON), directions with zero
components and origins at 1e30 -- and the scenes: a bumpy sheet of 312 triangles (one tree of more than 256 nodes, tier-A
materials of tests/exact_scenes.py), a one-triangle world, and a scene with a triangle the record cannot certify."""
import numpy as np

import exact_scenes as ES

F = np.float32
EDGE_AIMED = ("edge", "vertex")
CLASSES = ("random",) + EDGE_AIMED + ("plane_origin", "grazing", "axis_directions", "far_origin")


def sheet(abi, seed=5):
    """A 12 x 13 grid of quads over [-3, 3]^2, heights drawn in [0, 1.2], two triangles per quad, some with the other
    winding; a fuzzy-metal ground, a light, one tree."""
    rng = np.random.default_rng(seed)
    sb = abi.SceneBuilder()
    mats = ES.palette(sb, rng, "A")
    nx, ny = 13, 14
    gx, gy = np.meshgrid(np.linspace(-3, 3, nx), np.linspace(-3, 3, ny), indexing="ij")
    pos = np.stack([gx, rng.uniform(0.0, 1.2, gx.shape) + 1.0, gy - 1.0], axis=-1).reshape(-1, 3).astype(F)
    idx = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            a, b, c, d = i * ny + j, (i + 1) * ny + j, (i + 1) * ny + j + 1, i * ny + j + 1
            idx += [(a, c, b), (a, d, c)] if (i + j) % 5 else [(a, b, c), (a, c, d)]
    idx = np.array(idx)
    uv = rng.uniform(0, 1, (len(pos), 2)).astype(F)
    sb.add_triangles(pos, uv, idx[:200], mats[2])
    sb.add_triangles(pos, uv, idx[200:], mats[5])
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, mats[2])
    sb.add_sphere((0.0, 9.0, -1.0), 2.0, mats[6])
    sb.world_bvh(0, None, 0.0, 1.0)
    assert len(idx) == 312 and ES.bvh_nodes(sb.num_prims) >= 256
    return ES.assert_libm_free(sb, "A")


def one_triangle(abi, p=((-1.0, 0.5, -2.0), (1.5, 0.25, -1.0), (0.25, 2.0, -1.5))):
    """A world that is one bare triangle."""
    sb = abi.SceneBuilder()
    m = sb.metal((0.8, 0.8, 0.8), 0.4)
    sb.add_triangles(np.array(p, F), np.zeros((3, 2), F), np.array([[0, 1, 2]]), m)
    sb.world_prim(0)
    return sb


UNCERTIFIED = ((0.0, 1.0, -1.0), (2.0 ** -40, 1.0, -1.0), (0.0, 1.0 + 2.0 ** -20, -1.0 + 2.0 ** -21))  # an edge component below 2^-36


def with_uncertified(abi):
    """A few ordinary triangles and two the record cannot certify (kappa = +inf): a sliver with an edge component of 2^-40,
    and a triangle with an edge of 2^31."""
    sb = abi.SceneBuilder()
    m = sb.metal((0.8, 0.8, 0.8), 0.4)
    pos = np.array([(-1, 0.5, -2), (1.5, 0.25, -1), (0.25, 2, -1.5), (-2, 0.1, -3), (2, 0.2, -3), (0, 3, -3.5)] + list(UNCERTIFIED)
                   + [(-2.0 ** 30, -5.0, -6.0), (2.0 ** 30, -5.0, -6.0), (0.0, 2.0 ** 20, -6.0)], F)
    sb.add_triangles(pos, np.zeros((len(pos), 2), F), np.arange(len(pos)).reshape(-1, 3), m)
    sb.add_sphere((0.0, -1000.0, 0.0), 999.0, m)
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


def triangles_of(sb):
    """(n, 3, 3) float32: the scene's triangles in its own order."""
    return np.concatenate([np.asarray(t["p"], F).reshape(-1, 3, 3) for t in sb.triangles])


def _through(o, q, rng):
    d = q - o
    length = np.linalg.norm(d, axis=1, keepdims=True)
    length[length == 0] = 1.0
    return d * (rng.uniform(0.25, 4.0, (len(d), 1)) / length)


def rays(abi, tris, rng, per_class, t_min=1e-3):
    """{class: abi.RAY_DTYPE array of per_class rays} around triangles drawn from `tris`; float64 construction, rounded
    once.  Origins lie on the side the normal points to unless the class says otherwise; tMax = +inf."""
    tris = np.asarray(tris, np.float64)
    out = {}
    for name in CLASSES:
        t = tris[rng.integers(0, len(tris), per_class)]
        v0, v1, v2 = t[:, 0], t[:, 1], t[:, 2]
        n = np.cross(v1 - v0, v2 - v0)
        nl = np.linalg.norm(n, axis=1, keepdims=True)
        nu = np.divide(n, nl, out=np.zeros_like(n), where=nl > 0)
        size = np.abs(t - t.mean(axis=1, keepdims=True)).max(axis=(1, 2))[:, None] + 1e-30
        centre = t.mean(axis=1)
        front = centre + nu * size * rng.uniform(0.5, 4.0, (per_class, 1)) + rng.uniform(-1, 1, (per_class, 3)) * size
        a, b = rng.uniform(-0.5, 1.5, (2, per_class, 1))
        inside = v0 * (1 - a - b) + v1 * a + v2 * b
        tmin = np.full(per_class, t_min, F)
        if name == "random":
            o = centre + rng.uniform(-6, 6, (per_class, 3))
            d = _through(o, inside, rng)
        elif name == "edge":
            e = rng.integers(0, 3, per_class)
            s = rng.uniform(0, 1, (per_class, 1))
            k = np.arange(per_class)
            q = (t[k, e] * (1 - s) + t[k, (e + 1) % 3] * s).astype(F).astype(np.float64)  # a float point on the edge
            o, d = front, _through(front, q, rng)
        elif name == "vertex":
            q = t[np.arange(per_class), rng.integers(0, 3, per_class)]
            o, d = front, _through(front, q, rng)
        elif name == "plane_origin":
            o = inside
            d = _through(o, centre + rng.uniform(-2, 2, (per_class, 3)) * size, rng)
            tmin[::2] = 0.0
            tmin[1::4] = -1.0
        elif name == "grazing":
            o = front
            want = -1.1920928955078125e-07 * rng.uniform(0.25, 3.25, (per_class, 1)) * np.where(rng.uniform(size=(per_class, 1)) < 0.85, 1, -1)
            nn = np.maximum((n * n).sum(axis=1, keepdims=True), 1e-300)
            d = (v1 - v0) * rng.uniform(-4, 4, (per_class, 1)) + (v2 - v0) * rng.uniform(-4, 4, (per_class, 1)) + n * want / nn
        elif name == "axis_directions":
            o = front.copy()
            q = inside.astype(F).astype(np.float64)
            keep = rng.integers(0, 3, per_class)
            both = rng.uniform(size=per_class) < 0.5
            for c in range(3):
                zero = (keep != c) & (both | ((keep + 1) % 3 == c))
                o[zero, c] = q[zero, c]  # this component of d is exactly 0
            d = _through(o, q, rng)
        else:  # far_origin
            o = np.where(n >= 0, 1e30, -1e30) * rng.uniform(0.1, 1.0, (per_class, 3))
            d = _through(o, inside, rng)
            d[::2] *= 1e30
        r = np.zeros(per_class, abi.RAY_DTYPE)
        r["o"], r["d"], r["time"], r["tMin"], r["tMax"] = o.astype(F), d.astype(F), 0.5, tmin, np.inf
        out[name] = r
    return out
