"""NumPy float32 statement of the rules that turn caller geometry into device records and primitive boxes, written from the
reference (model.h:172, 183-235, 276-283 for triangles; sphere.h:47-52, 85-94 for spheres; vec3.h:29-31, 54-60;
aabb.h:33-43), not from csrc/srt_records.h, which it checks on bits.  Every operation is one float32 operation, in the
reference's order (the library is built without multiply-add contraction and with IEEE division and square root).

Inputs are arrays of abi.TRIANGLE_DTYPE / abi.SPHERE_DTYPE.  No GPU and no library."""
import numpy as np

F = np.float32
EPSILON = F(1.1920928955078125e-7)  # std::numeric_limits<float>::epsilon(), globals.h
PAD = F(0.0001)
MOVING = 1 << 30


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(F)


def _unit(v):
    """unitVector, vec3.h:54-60: v / sqrtf(lengthSquared(v)), v itself when the length is 0."""
    length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(F)).astype(F)
    with np.errstate(all="ignore"):
        u = (v / length[:, None]).astype(F)
    return np.where((length != 0)[:, None], u, v).astype(F)


def triangle_records(tri):
    """(test (n, 3, 4), shade (n, 4, 4)) float32.  test: the vertices, the w words the geometric normal (getNormal).  shade:
    unit normal | uv0.u, tangent | uv0.v, bitangent | uv1.u, (uv1.v, uv2.u, uv2.v, the material word as given)."""
    p, uv = np.ascontiguousarray(tri["p"], F), np.ascontiguousarray(tri["uv"], F)
    n = len(p)
    e0, e1 = (p[:, 1] - p[:, 0]).astype(F), (p[:, 2] - p[:, 0]).astype(F)
    normal = _cross(e0, e1)
    test = np.zeros((n, 3, 4), F)
    test[:, :, :3] = p
    test[:, :, 3] = normal
    d0, d1 = (uv[:, 1] - uv[:, 0]).astype(F), (uv[:, 2] - uv[:, 0]).astype(F)  # deltaUV0, deltaUV1
    f = (d0[:, 0] * d1[:, 1] - d1[:, 0] * d0[:, 1]).astype(F)
    f = np.where(f == 0, f + EPSILON, f).astype(F)
    with np.errstate(all="ignore"):
        f = (F(1.0) / f).astype(F)[:, None]
        tangent = _unit((f * (d1[:, 1:2] * e0 - d0[:, 1:2] * e1)).astype(F))
        bitangent = _unit((f * (-d1[:, 0:1] * e0 + d0[:, 0:1] * e1)).astype(F))
    shade = np.zeros((n, 4, 4), F)
    shade[:, 0, :3], shade[:, 1, :3], shade[:, 2, :3] = _unit(normal), tangent, bitangent
    shade[:, 0, 3], shade[:, 1, 3], shade[:, 2, 3] = uv[:, 0, 0], uv[:, 0, 1], uv[:, 1, 0]
    shade[:, 3, 0], shade[:, 3, 1], shade[:, 3, 2] = uv[:, 1, 1], uv[:, 2, 0], uv[:, 2, 1]
    shade[:, 3, 3] = np.ascontiguousarray(tri["material"], np.int32).view(F)
    return test, shade


def fold_min_max(v):
    """model.h:191-197 over v (n, 3 vertices, 3 axes): from +-infinity, min = std::min(min, vertex) = vertex < min ? vertex
    : min and max = std::max(max, vertex) = max < vertex ? vertex : max over the vertices in order.  Of two zeros of
    opposite sign the first one seen stays."""
    v = np.ascontiguousarray(v, F)
    mn = np.full((len(v), 3), np.inf, F)
    mx = np.full((len(v), 3), -np.inf, F)
    for k in range(v.shape[1]):
        mn = np.where(v[:, k] < mn, v[:, k], mn)
        mx = np.where(mx < v[:, k], v[:, k], mx)
    return mn, mx


def triangle_boxes(tri):
    """(mn, mx), (n, 3) each: triangle::boundingBox, model.h:183-212 (an axis without extent padded by 0.0001)."""
    mn, mx = fold_min_max(tri["p"])
    flat = mn == mx
    return np.where(flat, mn - PAD, mn).astype(F), np.where(flat, mx + PAD, mx).astype(F)


def sphere_records(sph):
    """(n, 3, 4) float32: (center0, radius), (center1, material word with bit 30 = center0 != center1), (time0, time1, 0, 0)."""
    rec = np.zeros((len(sph), 3, 4), F)
    rec[:, 0, :3], rec[:, 0, 3] = sph["center0"], sph["radius"]
    moving = (sph["center0"] != sph["center1"]).any(axis=1)
    bits = (sph["material"].astype(np.int32) & ~MOVING) | np.where(moving, MOVING, 0).astype(np.int32)
    rec[:, 1, :3], rec[:, 1, 3] = sph["center1"], bits.view(F)
    rec[:, 2, 0], rec[:, 2, 1] = sph["time0"], sph["time1"]
    return rec


def sphere_boxes(sph, time0, time1):
    """(mn, mx): sphere::boundingBox, sphere.h:85-94, with sphere::center, sphere.h:47-52."""
    c0, c1 = np.ascontiguousarray(sph["center0"], F), np.ascontiguousarray(sph["center1"], F)
    moving = (c0 != c1).any(axis=1)[:, None]
    r = sph["radius"].astype(F)[:, None]

    def center(time):
        with np.errstate(all="ignore"):
            s = ((F(time) - sph["time0"]) / (sph["time1"] - sph["time0"])).astype(F)[:, None]
            return np.where(moving, c0 + s * (c1 - c0), c0).astype(F)

    a, b = center(time0), center(time1)
    return np.minimum(a - r, b - r).astype(F), np.maximum(a + r, b + r).astype(F)
