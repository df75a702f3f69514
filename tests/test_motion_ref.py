"""CPU-side checks of the motion replay tests/motion_ref.py (no GPU): it is tests/temporal_ref.py where there is no
motion, a translated triangle moves back by the translation, a quad shifted by whole pixels reprojects onto the pixel
that many to the side, and the mean of affine displacements is the displacement at the mean."""
import numpy as np
import pytest

import motion_ref as M
import temporal_ref as R

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _camera(dev, abi, eye, look, vfov=40.0, aspect=1.5, focus=10.0):
    c = abi.default_camera_params(aspect)
    c.eye[:], c.lookAt[:] = eye, look
    c.vfovDegrees, c.aperture, c.focusDist = vfov, 0.0, focus
    return dev.make_camera(c)


def quad_planes(cam, W, H, n, lo, hi, z, rng):
    """Analytic planes (sums with counts over n samples) of the quad [lo.x, hi.x] x [lo.y, hi.y] at height z, facing +z, in
    front of sky, for a camera that looks down -z: (beauty, moments, normal, position, depth, albedo, hit)."""
    d, _ = R.pixel_ray(cam, W, H, np.float64)
    o = np.array(list(cam.origin), np.float64)
    D = np.stack(d, -1)
    with np.errstate(all="ignore"):
        t = (z - o[2]) / D[..., 2]
    P = o + t[..., None] * D
    hit = (t > 0) & (P[..., 0] >= lo[0]) & (P[..., 0] <= hi[0]) & (P[..., 1] >= lo[1]) & (P[..., 1] <= hi[1])
    cnt = np.where(hit, n, 0).astype(F)

    def plane(v):
        out = np.zeros((H, W, 4), F)
        out[..., :3] = np.where(hit[..., None], v, 0.0).astype(F) * F(n)
        out[..., 3] = cnt
        return out

    depth = np.zeros((H, W, 4), F)
    depth[..., 0] = np.where(hit, t, 0.0).astype(F) * F(n)
    depth[..., 3] = cnt
    beauty = np.zeros((H, W, 4), F)
    beauty[..., :3] = rng.uniform(0.1, 2.0, (H, W, 3)).astype(F) * F(n)
    beauty[..., 3] = n
    lum = beauty[..., :3] @ F([0.2126, 0.7152, 0.0722]) / F(n)
    moments = np.zeros((H, W, 4), F)
    moments[..., 0], moments[..., 1], moments[..., 3] = lum * F(n), lum * lum * F(n), n
    albedo = np.zeros((H, W, 4), F)
    albedo[..., :3] = rng.uniform(0.2, 0.9, (H, W, 3)).astype(F) * F(n)
    albedo[..., 3] = n
    normal = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (H, W, 3))
    return beauty, moments, plane(normal), plane(P), depth, albedo, hit


def _random_history(rng, W, H):
    """A history of random sums: counts of 0, inf and NaN among them, misses (nx = NaN), normals and positions near a
    surface so that some taps pass and some fail."""
    hist = rng.normal(0, 1, (3, H, W, 4)).astype(F)
    hist[0][..., 3] = rng.choice(F([0, 1, 4, 9, 70, np.inf, np.nan]), (H, W))
    hist[1][..., :3] = F([0, 0, 1]) + rng.normal(0, 0.6, (H, W, 3)).astype(F)
    hist[1][..., 0] = np.where(rng.random((H, W)) < 0.15, F(np.nan), hist[1][..., 0])
    hist[2][..., :3] = rng.normal(0, 0.5, (H, W, 3)).astype(F) + F([0, 0, -6])
    return hist


@pytest.mark.parametrize("demodulate", [False, True])
def test_without_motion_the_replay_is_temporal_ref(dev, abi, demodulate):
    W, H, n = 44, 28, 3
    rng = np.random.default_rng(5)
    prev = _camera(dev, abi, (0.0, 0.0, 4.0), (0.0, 0.0, 0.0))
    moved = _camera(dev, abi, (0.3, 0.1, 4.0), (0.1, 0.0, 0.0))
    lo, hi = (-1.4, -0.9), (1.2, 1.0)
    hist = _random_history(rng, W, H)
    hist[2][..., 2] = F(-6.0) + rng.normal(0, 0.05, (H, W)).astype(F)
    some = 0
    for cam in (prev, moved):
        b, m, nm, ps, dp, al, hit = quad_planes(cam, W, H, n, lo, hi, -6.0, rng)
        b[3, 4, 0], b[5, 6, 3] = np.nan, 0.0  # pixels that are not usable
        want = R.accumulate(b, m, nm, ps, dp, al, cam, prev, hist, demodulate=demodulate, info=(wi := {}))
        forms = [None] if cam is prev else [None, np.zeros((H, W, 4), F)]  # a zero plane only with two different cameras
        zero = np.zeros((H, W, 4), F)
        zero[..., 3] = nm[..., 3]
        forms += [] if cam is prev else [zero]
        for motion in forms:
            got = M.accumulate(b, m, nm, ps, dp, al, cam, prev, hist, motion=motion, demodulate=demodulate, info=(gi := {}))
            for g, w in zip(got, want):
                assert np.array_equal(_bits(g), _bits(w))
            assert np.array_equal(gi["has"], wi["has"])
        some += int(wi["has"].sum())
        assert np.array_equal(_bits(M.accumulate(b, None, nm, ps, dp, al, cam, prev, None, demodulate=demodulate)[2]),
                              _bits(R.accumulate(b, None, nm, ps, dp, al, cam, prev, None, demodulate=demodulate)[2]))
    assert some > 100  # taps were accepted: the comparison exercised the blend


def _scalar_triangle(p, cur, prev):
    """The header's triangle text, operation by operation on np.float32 scalars."""
    def sub(a, b):
        return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def dot(a, b):
        return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])

    v0, v1, v2 = cur
    n = cross(sub(v1, v0), sub(v2, v0))
    d0, d1, d2 = sub(prev[0], v0), sub(prev[1], v1), sub(prev[2], v2)
    e0, e1, e2 = dot(n, cross(sub(v1, v0), sub(p, v0))), dot(n, cross(sub(v2, v1), sub(p, v1))), dot(n, cross(sub(v0, v2), sub(p, v2)))
    s = (e0 + e1) + e2
    b0, b1, b2 = e1 / s, e2 / s, e0 / s
    assert all(isinstance(x, np.float32) for x in (s, b0, b1, b2))
    return F([(b0 * d0[k] + b1 * d1[k]) + b2 * d2[k] for k in range(3)]) if s > 0 else F(d0)


def test_translated_triangle_moves_back_by_the_translation():
    rng = np.random.default_rng(2)
    prev = rng.normal(0, 2, (50, 3, 3)).astype(F)
    a = rng.normal(0, 0.3, (50, 1, 3)).astype(F)
    cur = (prev + a).astype(F)
    d = (prev - cur).astype(F)  # per vertex, -a up to the rounding of prev + a
    centroid = ((cur[:, 0] + cur[:, 1]) + cur[:, 2]) / F(3)
    for p, corner in ((cur[:, 0], 0), (cur[:, 1], 1), (cur[:, 2], 2), (centroid, None)):
        m = M.displacement_triangle(p, cur, prev)
        # the bits of the stated formula, evaluated here on float32 scalars without the helper's vectorisation
        for i in (0, 17, 49):
            assert np.array_equal(_bits(m[i]), _bits(_scalar_triangle(p[i], cur[i], prev[i])))
        # and what the formula means: m = -a.  At a corner the weights are (1, 0, 0) up to the rounding of the edge
        # values, at the centroid a third each; the three d_i differ from -a by at most one rounding of |prev + a| <= 16
        tol = 8 * 2.0 ** -24 * 16
        assert np.abs(m.astype(np.float64) + a[:, 0]).max() <= tol
        if corner is not None:
            assert np.abs(m.astype(np.float64) - d[:, corner]).max() <= tol
    # nothing moved: exactly zero
    assert not M.displacement_triangle(centroid, cur, cur).any()
    # a degenerate current triangle moves as its first vertex
    flat = cur.copy()
    flat[:, 2] = flat[:, 1]
    assert np.array_equal(_bits(M.displacement_triangle(centroid, flat, prev)), _bits(prev[:, 0] - flat[:, 0]))


def test_sphere_displacement():
    rng = np.random.default_rng(4)
    dt = np.dtype([("center0", "<f4", 3), ("center1", "<f4", 3), ("time0", "<f4"), ("time1", "<f4"), ("radius", "<f4")])
    cur = np.zeros(20, dt)
    cur["center0"] = rng.normal(0, 2, (20, 3))
    cur["center1"] = cur["center0"]
    cur["center1"][::2] += rng.normal(0, 0.5, (10, 3)).astype(F)  # every other one moves
    cur["time1"], cur["radius"] = 1.0, rng.uniform(0.5, 2, 20)
    time = rng.random(20).astype(F)
    c = M.sphere_center(cur, time)
    dirs = rng.normal(0, 1, (20, 3))
    p = (c + cur["radius"][:, None] * (dirs / np.linalg.norm(dirs, axis=1, keepdims=True))).astype(F)
    assert not M.displacement_sphere(p, time, cur, cur).any()  # unmoved: exact zeros
    prev = cur.copy()
    shift = rng.normal(0, 0.4, (20, 3)).astype(F)
    prev["center0"] += shift
    prev["center1"] += shift
    prev["radius"] *= F(1.25)
    m = M.displacement_sphere(p, time, cur, prev).astype(np.float64)
    # the point keeps its direction from the centre: p + m = c' + 1.25 (p - c)
    want = (M.sphere_center(prev, time).astype(np.float64) + 1.25 * (p.astype(np.float64) - c)) - p
    assert np.abs(m - want).max() <= 1e-5


def test_quad_shifted_by_whole_pixels_reprojects_sideways(dev, abi):
    """A quad in the focus plane, parallel to the image plane: one pixel is |horizontal| / (W - 1) wide there."""
    W, H, n, k = 44, 28, 2, 3
    cam = _camera(dev, abi, (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), focus=10.0)
    pitch = np.linalg.norm(np.float64(list(cam.horizontal))) / (W - 1)
    rng = np.random.default_rng(7)
    lo0, hi0 = np.array([-4.0, -2.5]), np.array([2.5, 2.6])
    shift = np.array([k * pitch, 0.0])
    b0, m0, nm0, ps0, dp0, al0, hit0 = quad_planes(cam, W, H, n, lo0, hi0, -6.0, rng)
    b1, m1, nm1, ps1, dp1, al1, hit1 = quad_planes(cam, W, H, n, lo0 + shift, hi0 + shift, -6.0, rng)
    _, _, h0 = R.accumulate(b0, m0, nm0, ps0, dp0, None, cam, cam, None)
    motion = np.zeros((H, W, 4), F)
    motion[..., 0] = np.where(hit1, F(-k * pitch) * F(n), F(0))
    motion[..., 3] = nm1[..., 3]
    info = {}
    out_b, _, _ = M.accumulate(b1, m1, nm1, ps1, dp1, None, cam, cam, h0, motion=motion, info=info)
    x = np.broadcast_to(np.arange(W)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H)[:, None], (H, W))
    interior = hit1 & np.roll(hit0, k, axis=1) & (x >= k)
    assert interior.sum() > 150
    assert np.abs(info["xf"] - (x - k))[interior].max() <= R.SNAP and np.abs(info["yf"] - y)[interior].max() <= R.SNAP
    assert info["has"][interior].all()
    # one tap of weight 1: the accumulated sum is this pixel plus the pixel k to the left of the previous frame
    want = b1[..., :3] + np.roll(b0, k, axis=1)[..., :3]
    assert np.array_equal(_bits(out_b[..., :3][interior]), _bits(want[interior]))
    # without the plane the cameras agree and every pixel is its own history: the strip the quad left keeps the quad's
    static = R.accumulate(b1, m1, nm1, ps1, dp1, None, cam, cam, h0)[0]
    left = hit0 & ~hit1
    assert left.any() and (static[..., 3][left] == 2 * n).all() and (out_b[..., 3][left] == n).all()


def test_mean_of_affine_displacements_is_the_displacement_at_the_mean():
    """The motion pass sums per-sample m; the reprojection uses the sum divided by the count.  For points on one triangle
    under an affine map the barycentric mix is affine in p, so the mean of m equals m at the mean point.  Bound: each m is
    a 3-term sum of products whose terms are at most B = max |d_i|; every operation rounds by 2^-24 relative, about 10
    operations deep (edge values, their sum, the quotient, the mix), and the float32 mean of K values adds K roundings:
    (10 + K) 2^-24 B, against which 1e-5 B leaves a factor of ten for K = 3."""
    rng = np.random.default_rng(9)
    K, N = 3, 400
    prev = rng.normal(0, 1, (N, 3, 3))
    ang = rng.uniform(0.05, 0.5, N)
    rot = np.zeros((N, 3, 3))
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang), 1
    scale = rng.uniform(0.8, 1.3, (N, 1, 1))
    cur = (scale * np.einsum("nij,nvj->nvi", rot, prev) + rng.normal(0, 0.2, (N, 1, 3))).astype(F)
    prev = prev.astype(F)
    w = rng.dirichlet((1, 1, 1), (K, N))  # interior points
    pts = np.einsum("knv,nvi->kni", w, cur.astype(np.float64)).astype(F)
    ms = [M.displacement_triangle(p, cur, prev) for p in pts]
    total = np.zeros((N, 3), F)
    for m in ms:  # the kernel's running sum, then the reprojection's mean
        total = total + m
    mean_m = total / F(K)
    mean_p = (((pts[0] + pts[1]) + pts[2]) / F(K)).astype(F)
    at_mean = M.displacement_triangle(mean_p, cur, prev)
    B = np.abs(prev - cur).max(axis=(1, 2))
    assert (10 + K) * 2.0 ** -24 < 1e-5
    # the mean point is itself rounded (3 adds and a division of coordinates up to C): it moves m by the map's linear
    # part (at most 2 in norm here) times that, inside the same budget for |C| <= 4 B
    assert (np.abs(mean_m.astype(np.float64) - at_mean).max(axis=1) <= 1e-5 * np.maximum(B, np.abs(cur).max(axis=(1, 2)))).all()
