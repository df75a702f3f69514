"""The edge cases of the record and box arithmetic (csrc/srt_records.h) as one fixed list of 12 triangles and 4 spheres,
shared by tests/test_records_host.py (CPU) and tests/test_gpu_refit.py (as a real scene).  `abi` is the package's abi module.

The primitives lie apart on a grid in x and y and every triangle with an area turns its front (model.h:122 drops a hit
from behind) to +z, so a ray from +z at a primitive's centroid meets that primitive first.  Only
triangle 2 has a zero on x and only triangle 3 one on y, and no z extreme of the whole list is a zero: a union of boxes
(fminf / fmaxf, which do not order zeros) never meets two zeros of opposite sign, so every node box is defined too."""
import numpy as np

F = np.float32
UV = [(0.125, 0.25), (0.875, 0.375), (0.375, 0.75)]  # a general mapping, f > 0

# (what it exercises, three vertices, three uvs)
TRIANGLES = [
    ("general, tilted", [(3, 3, 0.5), (4.25, 3.5, -0.75), (3.5, 4.5, 1.25)], UV),
    ("axis-flat on z: the pad", [(6, 3, 0.5), (7, 3, 0.5), (6, 4, 0.5)], UV),
    ("x = {+0, -0, 1}: box minimum +0", [(0.0, 13, 0.25), (-0.0, 12, 0.5), (1, 12.5, -0.25)], UV),
    ("y = {-0, +0, 1}: box minimum -0", [(15, -0.0, 0.25), (16, 0.0, 0.5), (15.5, 1, -0.25)], UV),
    ("zero area, collinear: unit of the zero normal", [(9, 3, 0.5), (10, 4, 1.5), (11, 5, 2.5)], UV),
    ("a point: every vector zero, every axis padded", [(12, 3, 0.5), (12, 3, 0.5), (12, 3, 0.5)], UV),
    ("collinear uvs: f == 0, the epsilon, a tangent that is not zero", [(12, 6, 0.5), (13, 6.25, -0.25), (12.25, 7, 0.75)],
     [(0, 0), (1, 1), (2, 2)]),
    ("equal uvs: f == 0, zero tangent and bitangent", [(15, 6, 0.5), (16, 6.5, 0.125), (15.5, 7, 1)], [(0.5, 0.5)] * 3),
    ("negative f", [(15, 3, 0.25), (16, 3, 0.75), (15, 4, -0.5)], [(0, 0), (0, 1), (1, 0)]),
    ("z = {-1, -0, +0}: box maximum -0", [(3, 6, -1), (4, 6, -0.0), (3.5, 7, 0.0)], UV),
    ("z = {+0, -0, +0}: min == max across the signs, padded", [(6, 6, 0.0), (7, 6, -0.0), (6, 7, 0.0)], UV),
    ("general, uvs outside [0, 1]", [(9, 6, -2.5), (10.5, 6.25, 0.75), (9.25, 7.75, 1.5)], [(-1.5, 2.25), (3.0, -0.5), (0.25, 0.125)]),
]

# (what it exercises, center0, center1, time0, time1, radius)
SPHERES = [
    ("static", (3, 9.5, 0.25), (3, 9.5, 0.25), 0.0, 1.0, 0.75),
    ("moving, own times inside the item's: the path is extrapolated", (6, 9.5, 0.25), (7, 10, -0.5), 0.25, 0.75, 0.5),
    ("moving", (9.5, 9.5, 0.5), (10, 9.75, 0.25), 0.0, 1.0, 0.625),
    ("centres that differ in the sign of a zero: equal, not moving", (12.5, 9.5, 0.0), (12.5, 9.5, -0.0), 0.0, 1.0, 0.375),
]


def geometry(abi, tri_material=0, sphere_material=0):
    """(triangles, spheres) as abi.TRIANGLE_DTYPE / abi.SPHERE_DTYPE arrays."""
    tri = np.zeros(len(TRIANGLES), abi.TRIANGLE_DTYPE)
    for i, (_, p, uv) in enumerate(TRIANGLES):
        tri[i] = (p, uv, tri_material)
    sph = np.zeros(len(SPHERES), abi.SPHERE_DTYPE)
    for i, (_, c0, c1, t0, t1, r) in enumerate(SPHERES):
        sph[i] = (c0, c1, t0, t1, r, sphere_material)
    return tri, sph


def scene(abi, tri, sph, builder=0, one_item=True):
    """The geometry as a scene: 12 triangles then 4 spheres.  one_item: one world item over [0, 1] built by `builder`;
    otherwise one single-primitive host-built item per primitive over [0, 1], then one per primitive over [0, 0]."""
    sb = abi.SceneBuilder()
    mats = sb.pbr(albedo_tex=sb.solid(200, 150, 100), metalness=0.0, roughness=0.5), sb.metal((0.7, 0.6, 0.5), 0.1)
    n = len(tri)
    sb.add_triangles(tri["p"].reshape(-1, 3), tri["uv"].reshape(-1, 2), np.arange(3 * n, dtype=np.int32).reshape(-1, 3), mats[0])
    for s in sph:
        sb.add_sphere(tuple(s["center0"].tolist()), float(s["radius"]), mats[1], center1=tuple(s["center1"].tolist()),
                      time0=float(s["time0"]), time1=float(s["time1"]))
    if one_item:
        sb.world_bvh(0, None, 0.0, 1.0, builder=builder)
    else:
        for t1 in (1.0, 0.0):
            for i in range(sb.num_prims):
                sb.world_bvh(i, 1, 0.0, t1)
    return sb


def rays(abi, tri, sph):
    """One ray per primitive, from outside (+z, a little aslant) at its centroid or its centre at the sphere's own time0."""
    target = np.concatenate([tri["p"].astype(np.float64).mean(axis=1), sph["center0"].astype(np.float64)])
    r = np.zeros(len(target), abi.RAY_DTYPE)
    origin = target + np.array([0.3, 0.2, 10.0])
    r["o"], r["d"] = origin.astype(F), (target - origin).astype(F)
    r["time"][len(tri):] = sph["time0"]
    r["tMin"], r["tMax"] = 0.001, np.inf
    return r
