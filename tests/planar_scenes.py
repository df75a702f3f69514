"""Frames whose EVERY ray, camera ray and bounce alike, has a direction component of exactly +-0 (tests/test_planar_scenes.py,
tests/test_gpu_planar_frames.py).  Such a ray is never certified by the slab test (csrc/srt_slab.h srtSlabOperandOk), so each of
its node visits takes the IEEE block, and on the regrouped tree the gate form; camera rays and fuzzy
reflections never have an exact zero, so no other frame reaches that code.

The construction: a hand-filled SrtCamera whose origin, lleft, horizontal and vertical all have component `axis` equal to
zero, with no lens (lensRadius 0, hor = vert = w = 0), in a scene that is mirror-symmetric in the plane x_axis = 0 -- sphere
centres in the plane, moving spheres moving within it, quads perpendicular to one of the other two axes, metals of fuzz 0,
dielectrics, solid lights, the background (tier A of tests/exact_scenes.py: no libm call).  Every normal then has a zero
component on the axis, reflect and refract keep the zero, and o + t d keeps the origin's 0.

Everything is built in x-planar coordinates (the plane is x = 0) and rolled: component k goes to (k + axis) % 3.  The
builders are seeded plain functions of `abi`; every scene has passed exact_scenes.assert_libm_free(sb, "A")."""
import numpy as np

import exact_scenes

F = np.float32
CONFIGS = [(axis, negative_zero) for axis in range(3) for negative_zero in (0, 1)]
MISS_PLANES = (0.0, 1e-4, -1e-4, 0.5, -0.5, 5e-5)


def _roll(v, axis):
    return np.roll(np.asarray(v, F), axis, axis=-1)


def camera(abi, axis, negative_zero):
    """Origin (0, 3, 9), lower left (0, -1, -3), horizontal (0, 0, 6), vertical (0, 8, 0), rolled by `axis`.  negative_zero:
    -0.0 in component `axis` of lleft, horizontal and vertical (the origin keeps +0.0), which makes the camera rays' -0.0."""
    z = -0.0 if negative_zero else 0.0
    cam = abi.SrtCamera()
    for field, v in (("origin", (0.0, 3.0, 9.0)), ("lleft", (z, -1.0, -3.0)), ("horizontal", (z, 0.0, 6.0)), ("vertical", (z, 8.0, 0.0))):
        getattr(cam, field)[:] = [float(c) for c in _roll(v, axis)]
    for field in ("w", "hor", "vert"):
        getattr(cam, field)[:] = (0.0, 0.0, 0.0)
    cam.lensRadius, cam.time0, cam.time1 = 0.0, 0.0, 1.0
    return cam


def _quads(rng, count, normals, axis, place):
    """`count` quads of two triangles each in x-planar coordinates, quad k perpendicular to normals[k % len(normals)], its plane
    on a half-integer grid, half-extents 0.3-1.2, centre uniform in +-3 around (0, 3, -2); place(k, q) may move the float32
    corners q (4, 3) of quad k.  Returns (positions rolled by `axis`, indices)."""
    pos, idx = [], []
    for k in range(count):
        n = normals[k % len(normals)]
        u, v = (n + 1) % 3, (n + 2) % 3
        c = rng.uniform(-3, 3, 3) + np.array([0.0, 3.0, -2.0])
        c[n] = float(np.round(c[n] * 2) / 2)
        h = rng.uniform(0.3, 1.2, 2)
        q = np.repeat(c[None, :], 4, axis=0)
        q[:, u] += np.array([-h[0], h[0], h[0], -h[0]])
        q[:, v] += np.array([-h[1], -h[1], h[1], h[1]])
        q = place(k, q.astype(F))
        base = len(pos)
        pos += list(q)
        idx += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
    return _roll(np.array(pos, F), axis), np.array(idx)


def mirror_scene(abi, axis, touch):
    """60 mirror quads, alternately perpendicular to y and z (x-planar), the ground sphere as a mirror, a glass sphere, a
    moving mirror sphere and a light sphere with their centres in the plane, one tree.  touch: every third quad is shifted
    along the axis so that its minimum there is exactly 0 -- the rays' origin coordinate -- and every third so that its
    maximum is: the reference's quotients on such a box are NaN and +-inf, and it culls it."""
    rng = np.random.default_rng(4)
    sb = abi.SceneBuilder()
    mirror = sb.metal((0.8, 0.7, 0.6), 0.0)

    def place(k, q):
        if touch and k % 3 == 0:
            q[:, 0] -= q[:, 0].min()  # float32: x - x = 0 exactly
        elif touch and k % 3 == 1:
            q[:, 0] -= q[:, 0].max()
        return q

    pos, idx = _quads(rng, 60, (1, 2), axis, place)
    sb.add_triangles(pos, np.zeros((len(pos), 2), F), idx, mirror)

    def at(*c):
        return tuple(float(x) for x in _roll(c, axis))

    sb.add_sphere(at(0.0, -1000.0, 0.0), 1000.0, sb.metal((0.5, 0.5, 0.5), 0.0))
    sb.add_sphere(at(0.0, 1.0, 0.0), 1.0, sb.dielectric(1.5))
    sb.add_sphere(at(0.0, 2.0, 3.0), 0.75, sb.metal((0.9, 0.9, 0.9), 0.0), center1=at(0.0, 2.5, 4.0), time0=0.0, time1=1.0)
    sb.add_sphere(at(0.0, 6.0, 4.0), 1.5, sb.light((25.0, 22.0, 11.0)))
    sb.world_bvh(0, None, 0.0, 1.0)
    return exact_scenes.assert_libm_free(sb, "A")


def miss_scene(abi, axis):
    """96 quads lying in planes perpendicular to the axis, at MISS_PLANES in turn; no spheres, one tree.  Every planar ray is
    parallel to every triangle: the whole frame is background, one ray per sample, and `closest` stays +inf, so the node
    visits of a frame are a function of the box tests alone.  The flat axis of a triangle's box is padded by 1e-4
    (model.h:199-203): boxes that straddle 0, boxes whose padded minimum is fl(1e-4f - 1e-4f) == 0 == o, and inner nodes with
    a plane at 0."""
    rng = np.random.default_rng(6)
    sb = abi.SceneBuilder()

    def place(k, q):
        q[:, 0] = F(MISS_PLANES[k % len(MISS_PLANES)])
        return q

    pos, idx = _quads(rng, 96, (0,), axis, place)
    sb.add_triangles(pos, np.zeros((len(pos), 2), F), idx, sb.metal((0.8, 0.7, 0.6), 0.0))
    sb.world_bvh(0, None, 0.0, 1.0)
    return exact_scenes.assert_libm_free(sb, "A")


def camera_rays(oracle, abi, osc, cam, p):
    """The camera ray of every (pixel, sample) of a frame with parameters p, in row-major pixel order, through
    OracleScene.sample_path -- and with it the number of rays each sample traced."""
    steps = [osc.sample_path(cam, p, x, y, p.sampleFirst + s)[0] for y in range(p.imageHeight) for x in range(p.imageWidth) for s in range(p.spp)]
    first = np.array([s[0] for s in steps])
    rays = np.zeros(len(first), abi.RAY_DTYPE)
    rays["o"], rays["d"], rays["time"] = first["o"], first["d"], first["time"]
    rays["tMin"], rays["tMax"] = p.tMin, np.inf
    return rays, np.array([len(s) for s in steps])


GATE_FORMS = ("closed", "reference", "open")


def gate_replay(arr, rays):
    """Node visits of `rays` (none of which hits anything: closest = +inf throughout) over the flattened array `arr` under the
    three forms an inner node's test can take on an axis with d == +-0 -- "closed": the kernel's gate, min <= o <= max and no
    bound on t; "reference": aabb.h:11-27 as it stands; "open": no test at all there -- leaves always taking the reference's.
    Returns {form: (visits per ray, entered leaves (rays x leaves))}, from test_regroup_host's float32 replay."""
    from test_regroup_host import _entered, _intervals
    a0, b0, _ = _intervals(arr, rays, gates=False)
    a1, b1, inside = _intervals(arr, rays, gates=True)
    return {"closed": _entered(arr, 0, inside & ~(b1 <= a1)),
            "reference": _entered(arr, 0, ~(b0 <= a0)),
            "open": _entered(arr, 0, ~(b1 <= a1))}
