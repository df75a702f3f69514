"""Inputs of the reference pin (tests/test_reference_pin.py, tests/make_golden.py, tests/test_gpu_reference_pin.py): the
edge rays, the edge scene, the cameras and the scatter records.  Everything here is made from the scene's own numbers in float32 and
from seeded generators: nothing calls the oracle, the harness or the device library."""
import numpy as np

f32 = np.float32
EPS = np.finfo(f32).eps  # globals.h:14


def _unit(v):
    v = np.asarray(v, np.float64)
    n = np.linalg.norm(v)
    return v / n if n > 0 else v


class _Rays:
    def __init__(self, abi):
        self.abi, self.rows, self.names = abi, [], []

    def add(self, name, o, d, time=0.0, tMin=0.001, tMax=np.inf):
        r = np.zeros(1, self.abi.RAY_DTYPE)
        r["o"], r["d"], r["time"], r["tMin"], r["tMax"] = np.asarray(o, f32), np.asarray(d, f32), time, tMin, tMax
        self.rows.append(r)
        self.names.append(name)

    def done(self):
        return np.concatenate(self.rows), list(self.names)


def _sphere_rays(R, tag, s):
    """The cases of sphere::hit (sphere.h:54-83) and sphere::calcTangentBasis (:96-106) on one sphere."""
    t0, t1 = float(s.time0), float(s.time1)
    c0, c1, rad = np.array(s.center0[:], f32), np.array(s.center1[:], f32), f32(s.radius)
    moving = bool((c0 != c1).any())
    times = (0.0, 1.0, 0.5, -0.5, 1.5) if moving else (0.0,)
    for time in times:
        # sphere.h:47-52 in float32, so that the rays below are built on the centre the reference computes
        c = (c0 + f32((f32(time) - f32(t0)) / (f32(t1) - f32(t0))) * (c1 - c0)).astype(f32) if moving else c0
        at = "%s@%g" % (tag, time)
        for axis in range(3):
            for sign in (1.0, -1.0):
                d = np.zeros(3, f32)
                d[axis] = -sign
                o = c.copy()
                o[axis] += f32(sign) * f32(3) * rad
                R.add("%s axis-parallel %+d%s" % (at, int(sign), "xyz"[axis]), o, d, time)
        far = (c + np.array([0, 0, 3], f32) * rad).astype(f32)
        R.add(at + " zero direction outside", far, (0, 0, 0), time)
        R.add(at + " zero direction inside", c, (0, 0, 0), time)
        R.add(at + " -0.0 components a", far, (-0.0, -0.0, -1.0), time)
        R.add(at + " -0.0 components b", (c + np.array([0, -3, 0], f32) * rad).astype(f32), (-0.0, 1.0, -0.0), time)
        R.add(at + " -0.0 component and tMin -0.0", far, (0.0, -0.0, -1.0), time, tMin=-0.0)
        for axis in range(3):
            o = far.copy()
            o[axis] = np.nan
            R.add("%s NaN origin %s" % (at, "xyz"[axis]), o, (0, 0, -1), time)
        t_near = f32(2) * rad  # o = c + 3R z, d = -z: the roots are 2R and 4R
        for name, v in (("below", np.nextafter(t_near, f32(0))), ("at", t_near), ("above", np.nextafter(t_near, f32(np.inf)))):
            R.add("%s tMax %s the near root" % (at, name), far, (0, 0, -1), time, tMax=v)
            R.add("%s tMin %s the near root" % (at, name), far, (0, 0, -1), time, tMin=v)  # above: the far root is taken
        for scale in (0.5, 2.0, 3.0):  # a direction that is not normalised: a = |d|^2 divides the roots (sphere.h:56,67)
            t_scaled = (f32(2) * rad / f32(scale)).astype(f32)
            for name, v in (("below", np.nextafter(t_scaled, f32(0))), ("at", t_scaled), ("above", np.nextafter(t_scaled, f32(np.inf)))):
                R.add("%s |d| %g, tMax %s the near root" % (at, scale, name), far, (0, 0, -scale), time, tMax=v)
                R.add("%s |d| %g, tMin %s the near root" % (at, scale, name), far, (0, 0, -scale), time, tMin=v)
        R.add(at + " tMax between the roots, tMin above the near one", far, (0, 0, -1), time, tMin=f32(2.5) * rad, tMax=f32(3.5) * rad)
        R.add(at + " tMax finite beyond both roots", far, (0, 0, -1), time, tMax=f32(10) * rad)
        # o = c + (R, 0, R), d = -z: |oc|^2 - R^2 = R^2 = halfB^2, discriminant 0 (exactly, for the unit spheres at whole
        # coordinates); one ulp of o.x to either side of it
        touch = (c + np.array([1, 0, 1], f32) * rad).astype(f32)
        toward, away = (f32(-np.inf), f32(np.inf)) if touch[0] >= c[0] else (f32(np.inf), f32(-np.inf))
        for name, x in (("inside", np.nextafter(touch[0], toward)), ("on", touch[0]), ("outside", np.nextafter(touch[0], away))):
            R.add("%s tangent ray, one ulp %s (discriminant 0 on)" % (at, name) if name != "on" else "%s tangent ray, discriminant 0" % at,
                  (x, touch[1], touch[2]), (0, 0, -1), time)
        on = (c + np.array([0, 0, 1], f32) * rad).astype(f32)
        R.add(at + " from the surface outwards", on, (0, 0, 1), time)
        R.add(at + " from the surface inwards", on, (0, 0, -1), time)
        R.add(at + " from the surface inwards, tMin 0", on, (0, 0, -1), time, tMin=0.0)
        R.add(at + " from the centre (near root negative)", c, (0.3, 0.2, 1.0), time)
        for pole in (1.0, -1.0):  # 1 - |n.y| < epsilon for dx / R below about 4.9e-4 (the -UnitZ branch)
            for dx in (0.0, 2e-4, 4e-4, 4.8e-4, 4.9e-4, 5e-4, 6e-4, 1e-3):
                o = (c + np.array([dx, 3 * pole, 0], f32) * rad).astype(f32)
                R.add("%s normal near %+dY, dx/R %g" % (at, int(pole), dx), o, (0, -pole, 0), time)


def _triangle_rays(R, tag, P):
    """The cases of triangle::hit (model.h:104-181) on one triangle P (3, 3)."""
    P = np.asarray(P, f32)
    N = np.cross((P[1] - P[0]).astype(np.float64), (P[2] - P[0]).astype(np.float64))
    area = np.linalg.norm(N)
    n = _unit(N) if area > 0 else np.array([0.0, 0.0, 1.0])
    G = P.astype(np.float64).mean(0)
    front_o, front_d = (G + n).astype(f32), (-n).astype(f32)
    R.add(tag + " front", front_o, front_d)
    R.add(tag + " back-facing", (G - n).astype(f32), n.astype(f32))
    R.add(tag + " tMax below t", front_o, front_d, tMax=0.5)
    # inside the 1e-4 padding of a flat triangle's box (model.h:199-204): the box passes, triangle::hit never tests tMax (F4)
    R.add(tag + " tMax just below t", front_o, front_d, tMax=0.99995)
    for name, v in (("below", np.nextafter(f32(1), f32(0))), ("at", f32(1)), ("above", np.nextafter(f32(1), f32(2)))):
        R.add("%s tMin %s 1 (t is about 1)" % (tag, name), front_o, front_d, tMin=v)
    for k in range(3):
        mid = (P[k].astype(np.float64) + P[(k + 1) % 3]) / 2
        R.add("%s through edge %d" % (tag, k), (mid + n).astype(f32), front_d)
        R.add("%s through vertex %d" % (tag, k), (P[k].astype(np.float64) + n).astype(f32), front_d)
    R.add(tag + " zero direction", front_o, (0, 0, 0))
    R.add(tag + " NaN origin x", (np.nan, front_o[1], front_o[2]), front_d)
    e = _unit(P[1].astype(np.float64) - P[0]) if area > 0 else np.array([1.0, 0.0, 0.0])
    for sign in (-1.0, 1.0):  # |N.d| against epsilon (model.h:119): d = e + s n gives N.d = s |N|
        for k in (0.0, 0.5, 0.99, 1.01, 2.0, 64.0):
            s = sign * k * float(EPS) / area if area > 0 else 0.0
            d = (e + s * n)
            R.add("%s N.d about %+g epsilon" % (tag, sign * k), (G - d).astype(f32), d.astype(f32))
    R.add(tag + " along the plane", (G - e).astype(f32), e.astype(f32))
    R.add(tag + " axis-parallel -z", (G + np.array([0, 0, 2.0])).astype(f32), (0, 0, -1))
    R.add(tag + " axis-parallel -y", (G + np.array([0, 2.0, 0])).astype(f32), (0, -1, 0))
    R.add(tag + " axis-parallel +x", (G - np.array([2.0, 0, 0])).astype(f32), (1, 0, 0))


def pick_triangles(tris, limit=4):
    """Indices of the triangles the edge set visits in a scene: the first, second, middle and last, and the first one
    with zero area and with a zero uv determinant (model.h:220-222), where the scene has one."""
    n = len(tris)
    if n == 0:
        return []
    if n <= 12:
        return list(range(n))
    pick = [0, 1, n // 2, n - 1][:limit]
    P, UV = tris["p"], tris["uv"]
    cross = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    zero_area = np.flatnonzero((cross == 0).all(axis=1))
    d0, d1 = UV[:, 1] - UV[:, 0], UV[:, 2] - UV[:, 0]
    det0 = np.flatnonzero((d0[:, 0] * d1[:, 1] - d1[:, 0] * d0[:, 1]).astype(f32) == 0)
    for extra in (zero_area, det0):
        if len(extra) and int(extra[0]) not in pick:
            pick.append(int(extra[0]))
    return pick


def edge_rays(abi, sb, max_spheres=6):
    """(rays, names): the edge set of one scene -- every case on each of its first spheres and on pick_triangles."""
    R = _Rays(abi)
    for i, s in enumerate(sb.spheres[:max_spheres]):
        _sphere_rays(R, "sphere %d" % i, s)
    tris = np.concatenate(sb.triangles) if sb.triangles else np.zeros(0, abi.TRIANGLE_DTYPE)
    for i in pick_triangles(tris):
        _triangle_rays(R, "triangle %d" % i, tris["p"][i])
    return R.done()


def edge_scene(abi):
    """The geometry the config scenes lack: two triangles sharing an edge in the plane z = 0 (a box with a zero-extent
    axis, model.h:199-204), a zero-area triangle, triangles whose uv determinant is 0 (the f += epsilon branch of
    calcTangentBasis, model.h:220-222), a tilted triangle, a moving sphere (sphere.h:47-52) and a static one."""
    sb = abi.SceneBuilder()
    mat = sb.pbr(albedo_tex=sb.solid(120.0, 130.0, 140.0), metalness=0.0, roughness=0.5)
    pos = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0],            # 0-3: a square of two triangles
                    [4, 0, 1], [5, 0, 1], [6, 0, 1],                      # 4-6: collinear, zero area
                    [-3, 0, 0], [-1, 0, 0.5], [-2, 2, 1],                 # 7-9: all three uv equal
                    [-3, 3, 0], [-1, 3, 0.5], [-2, 5, 1],                 # 10-12: collinear uv
                    [3, 3, -1], [5, 3.5, -2], [4, 5, 0.25]], np.float32)  # 13-15: tilted
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [0, 0], [0.5, 0], [1, 0], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5],
                   [0.1, 0.1], [0.2, 0.2], [0.4, 0.4], [0.2, 0.1], [0.9, 0.3], [0.4, 0.8]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15]])
    sb.add_triangles(pos, uv, idx, mat)
    sb.add_sphere((0.5, 4.0, -1.0), 0.75, mat, center1=(1.25, 4.5, -0.5), time0=0.0, time1=1.0)
    sb.add_sphere((-4.0, 1.0, 2.0), 1.0, mat)
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


# ---------------------------------------------------------------------------------------------------- cameras
# camera.h:10-38 at other settings than main.cpp's: aperture 0, time0 == time1, vfov 20 to 151 degrees, another eye, a tilted up
# vector (tests/test_reference_pin.py test_cameras on the CPU, tests/test_gpu_exact_frames.py on the GPU)
CAMERAS = [  # eye, lookAt, up, vfov, aspect, aperture, focus distance, time0, time1
    ((0, 3, 5), (0, 2.5, 0), (0, 1, 0), vfov, aspect, aperture, focus, t0, t1)
    for vfov, aspect, aperture, focus, t0, t1 in (
        (20.0, 16 / 9, 0.1, 10.0, 0.0, 1.0), (33.3, 1.5, 0.0, 1.0, 0.0, 0.0), (45.0, 1.0, 2.0, 5.5, 0.25, 0.75),
        (59.9, 2.35, 0.3, 7.3, 0.0, 1.0), (89.0, 4 / 3, 0.05, 3.1, 0.0, 2.0), (101.7, 16 / 9, 0.7, 12.9, 1.0, 3.0),
        (120.0, 0.75, 1.1, 0.37, 0.0, 1.0), (151.3, 2.0, 0.01, 25.0, 0.0, 1.0))
] + [((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 1.5, 0.1, 10.0, 0.0, 1.0), ((-2, 7, 1), (1, 0.5, -3), (0.2, 1, -0.1), 64.2, 1.25, 0.4, 6.6, 0.0, 1.0)]


def camera_params(abi, k):
    """CAMERAS[k] as an SrtCameraParams."""
    cp = abi.SrtCameraParams()
    cp.eye[:], cp.lookAt[:], cp.up[:] = CAMERAS[k][:3]
    cp.vfovDegrees, cp.aspect, cp.aperture, cp.focusDist, cp.time0, cp.time1 = CAMERAS[k][3:]
    return cp


# ---------------------------------------------------------------------------------------------------- scatter records
def scatter_scene(abi):
    """(scene, {name: material}): every material type the reference has, at the settings where scatter takes another
    path.  The scene has no world: only its materials and textures are used."""
    sb = abi.SceneBuilder()
    rng = np.random.default_rng(21)
    m = {}
    for fuzz in (0.0, 0.3, 1.7):  # above 1: material.h:89 clamps it
        m["metal fuzz %g" % fuzz] = sb.metal((0.8, 0.6, 0.4), 0.0)
        sb.materials[-1].fuzz = fuzz  # SceneBuilder.metal clamps too; the reference's constructor is what is under test
    for ir in (1.5, 2.4):
        m["dielectric %g" % ir] = sb.dielectric(ir)
    rgb = sb.image(rng.integers(0, 256, (4, 6, 3), dtype=np.uint8), 3)
    nrm = sb.image(rng.integers(0, 256, (5, 5, 3), dtype=np.uint8), 3)
    chk = sb.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))
    grey = {v: sb.image(np.full((2, 2, 3), v, np.uint8), 3) for v in (0, 128, 255)}  # 3 bytes: roughness reads byte 1 defined
    for mv in (0.0, 0.5, 1.0):
        for rv in (0.0, 0.5, 1.0):
            m["pbr factors m %g r %g" % (mv, rv)] = sb.pbr(albedo=(0.9, 0.8, 0.7, 1.0), metalness=mv, roughness=rv)
    for mv in (0, 128, 255):
        for rv in (0, 128, 255):
            m["pbr maps m %d r %d" % (mv, rv)] = sb.pbr(albedo_tex=rgb, normal_tex=nrm, metallic_tex=grey[mv], roughness_tex=grey[rv],
                                                        albedo=(0.9, 0.8, 0.7, 1.0), metalness=0.2, roughness=0.9)
    m["pbr albedo map only"] = sb.pbr(albedo_tex=rgb, metalness=0.3, roughness=0.6)
    m["pbr normal map only"] = sb.pbr(normal_tex=nrm, albedo=(0.5, 0.6, 0.7, 1.0), metalness=0.3, roughness=0.6)
    m["pbr checker"] = sb.pbr(albedo_tex=chk, metalness=0.0, roughness=0.0)
    m["light colour"] = sb.light((250.2, 220.9, 110.2))
    m["light image"] = sb.light(emit_tex=rgb)
    m["light checker"] = sb.light(emit_tex=chk)
    return sb, m


def scatter_records(abi, materials, per_material=24, seed=33):
    """(rays, hits, names): per material, records with seeded unit normals, an orthonormal tangent frame, incidence from
    head-on to grazing, both faces.  For the dielectrics the back-face records past the critical angle are total internal
    reflection (no draw, material.h:119), the others take the reflectance draw."""
    rng = np.random.default_rng(seed)
    rays, hits, names = [], [], []
    for name, mat in materials.items():
        for k in range(per_material):
            n = _unit(rng.normal(size=3))
            t = _unit(np.cross(n, _unit(rng.normal(size=3))))
            b = np.cross(n, t)
            cos = (1.0, 0.95, 0.7, 0.4, 0.1, 0.01)[k % 6]  # cos of the angle between -d and the shading normal
            phi = rng.uniform(0, 2 * np.pi)
            sin = np.sqrt(1 - cos * cos)
            d = -(cos * n + sin * (np.cos(phi) * t + np.sin(phi) * b)) * rng.uniform(0.5, 3.0)  # not normalised (camera.h:45)
            r, h = np.zeros(1, abi.RAY_DTYPE), np.zeros(1, abi.HIT_DTYPE)
            p = rng.uniform(-5, 5, 3)
            r["o"], r["d"], r["time"], r["tMin"], r["tMax"] = (p - d).astype(f32), d.astype(f32), rng.uniform(0, 1), 0.001, np.inf
            h["t"], h["p"], h["uv"] = 1.0, p.astype(f32), rng.uniform(0, 1, 2).astype(f32)
            h["normal"], h["tangent"], h["bitangent"] = n.astype(f32), t.astype(f32), b.astype(f32)
            h["frontFace"], h["material"] = (k // 6) % 2 == 0, mat
            rays.append(r)
            hits.append(h)
            names.append("%s #%d (cos %g, %s face)" % (name, k, cos, "front" if h["frontFace"][0] else "back"))
    return np.concatenate(rays), np.concatenate(hits), names
