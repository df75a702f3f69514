"""NumPy float32 replay of include/srt_hip.h "Motion": the per-sample displacement of the motion pass
(csrc/srt_motion.hip) and srtTemporalAccumulateMotion / srtTemporalReprojectMotion (csrc/srt_reproject.h with MOTION).

The library is built without multiply-add contraction and with IEEE division, and the header restricts the math to
+ - * / in a stated order, so both halves agree with the kernels bit for bit.  Points and records are arrays whose last
axis is xyz; everything is evaluated in `dtype` (float32 unless a test asks for the float64 yardstick).

displacement_triangle / displacement_sphere take the CURRENT and the PREVIOUS geometry of the primitive each hit belongs
to, as the host sent it (abi.TRIANGLE_DTYPE's "p", abi.SPHERE_DTYPE records); accumulate / reproject take the planes of
tests/temporal_ref.py plus the resolved motion plane (sums with counts)."""
import numpy as np

import temporal_ref as T

F = np.float32


def dot3(a, b):
    """srt_path.h dot3: x x' + (y y' + z z')."""
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def triangle_normal(v, dtype=F):
    """The record's n = (v1 - v0) x (v2 - v0), as the upload and srtUpdateTriangles compute it.  v: (..., 3, 3)."""
    v = np.asarray(v, dtype)
    return cross3(v[..., 1, :] - v[..., 0, :], v[..., 2, :] - v[..., 0, :])


def displacement_triangle(p, cur, prev, dtype=F):
    """m of hits at p (n, 3) on triangles with current vertices cur (n, 3, 3) and previous vertices prev (n, 3, 3)."""
    p, cur, prev = (np.asarray(a, dtype) for a in (p, cur, prev))
    v0, v1, v2 = cur[..., 0, :], cur[..., 1, :], cur[..., 2, :]
    n = triangle_normal(cur, dtype)
    d0, d1, d2 = prev[..., 0, :] - v0, prev[..., 1, :] - v1, prev[..., 2, :] - v2
    with np.errstate(all="ignore"):
        e0 = dot3(n, cross3(v1 - v0, p - v0))
        e1 = dot3(n, cross3(v2 - v1, p - v1))
        e2 = dot3(n, cross3(v0 - v2, p - v2))
        s = (e0 + e1) + e2
        b0, b1, b2 = (e1 / s)[..., None], (e2 / s)[..., None], (e0 / s)[..., None]
        m = (b0 * d0 + b1 * d1) + b2 * d2
    return np.where((s > 0)[..., None], m, d0).astype(dtype)


def sphere_center(s, time, dtype=F):
    """sphere.h:47-52 on abi.SPHERE_DTYPE records: center0 unless the sphere moves (center0 != center1 in any bit-compared
    component, the device's "moving" bit), else c0 + ((time - t0) / (t1 - t0)) (c1 - c0)."""
    c0, c1 = s["center0"].astype(dtype), s["center1"].astype(dtype)
    moving = (s["center0"] != s["center1"]).any(axis=-1)
    t0, t1 = s["time0"].astype(dtype), s["time1"].astype(dtype)
    with np.errstate(all="ignore"):
        k = ((np.asarray(time, dtype) - t0) / (t1 - t0))[..., None]
        return np.where(moving[..., None], c0 + k * (c1 - c0), c0).astype(dtype)


def displacement_sphere(p, time, cur, prev, dtype=F):
    """m of hits at p (n, 3), ray times (n,), on spheres with current records cur (n,) and previous records prev (n,)."""
    p = np.asarray(p, dtype)
    c, cp = sphere_center(cur, time, dtype), sphere_center(prev, time, dtype)
    with np.errstate(all="ignore"):
        k = (prev["radius"].astype(dtype) / cur["radius"].astype(dtype)) - dtype(1)
        return ((cp - c) + k[..., None] * (p - c)).astype(dtype)


def displacement(prims, prim, p, time, tri_cur, tri_prev, sph_cur, sph_prev, dtype=F):
    """Per-ray m (n, 3) and the hit mask.  prims: the scene's (numPrims, 2) list of (type, index); prim: per-ray index into
    it (< 0: a miss, m = 0); the geometry arrays are in the scene's own order (abi.TRIANGLE_DTYPE / SPHERE_DTYPE)."""
    prim = np.asarray(prim)
    hit = prim >= 0
    m = np.zeros((len(prim), 3), dtype)
    kind = np.where(hit, prims[np.maximum(prim, 0), 0], -1)
    index = prims[np.maximum(prim, 0), 1]
    tri, sph = kind == 0, kind == 1
    if tri.any():
        m[tri] = displacement_triangle(p[tri], tri_cur["p"][index[tri]], tri_prev["p"][index[tri]], dtype)
    if sph.any():
        m[sph] = displacement_sphere(p[sph], np.asarray(time)[sph], sph_cur[index[sph]], sph_prev[index[sph]], dtype)
    return m, hit


def _reprojected(normal, depth, cam, prev, hist, motion, normal_cos, plane_dist, max_history, dtype):
    """h = [r, g, b, count, S1, S2], has, and (hit, n_p, Q-independent) surface terms, by the header's text with the three
    Motion changes where `motion` is given."""
    D = dtype
    H, W = normal.shape[:2]
    normal_cos = D(F(normal_cos or T.DEFAULT_NORMAL_COS))
    plane_dist = D(F(plane_dist or T.DEFAULT_PLANE_DIST))
    max_history = D(F(max_history or T.DEFAULT_MAX_HISTORY))
    nm, dp = normal.astype(D), depth.astype(D)
    dot = T._dot
    with np.errstate(all="ignore"):
        hit = nm[..., 3] > 0
        nv = [T._mean(nm[..., k], nm[..., 3], D) for k in range(3)]
        ln = np.sqrt(dot(nv, nv)).astype(D)
        good = (ln > 0) & (ln < np.inf)
        n_p = [np.where(good, nv[k] / np.where(good, ln, D(1)), D(0)).astype(D) for k in range(3)]
        tbar = T._mean(dp[..., 0], dp[..., 3], D)
    h = [np.zeros((H, W), D) for _ in range(6)]
    has = np.zeros((H, W), bool)
    info = {"xf": None, "yf": None}
    if hist is not None:
        hs = hist.astype(D)
        static = motion is None and T.same_camera(cam, prev)  # change 3: no camera-not-moved rule with a motion plane
        if static:
            ok = np.ones((H, W), bool)
            tx = [np.broadcast_to(np.arange(W)[None, :], (H, W))] * 4
            ty = [np.broadcast_to(np.arange(H)[:, None], (H, W))] * 4
            wt = [np.ones((H, W), D)] + [np.zeros((H, W), D)] * 3
        else:
            d, dlen = T.pixel_ray(cam, W, H, D)
            o, po = T._vec(cam, "origin", D), T._vec(prev, "origin", D)
            P = [(o[k] + tbar * d[k]).astype(D) for k in range(3)]
            if motion is not None:  # changes 1 and 2: P' = P + mbar, used by the projection and by the plane test
                mo = motion.astype(D)
                P = [(P[k] + T._mean(mo[..., k], mo[..., 3], D)).astype(D) for k in range(3)]
            v = [np.where(hit, P[k] - po[k], d[k]).astype(D) for k in range(3)]
            xf, yf, z = T.project(prev, v, W, H, D)
            with np.errstate(invalid="ignore"):
                ok = (z > 0) & (xf > -1) & (xf < W) & (yf > -1) & (yf < H)
            info.update(xf=xf, yf=yf)
            xs, ys = np.where(ok, xf, D(0)).astype(D), np.where(ok, yf, D(0)).astype(D)
            xr, yr = np.rint(xs), np.rint(ys)
            snap = (np.abs(xs - xr) <= D(T.SNAP)) & (np.abs(ys - yr) <= D(T.SNAP))
            x0, y0 = np.floor(xs), np.floor(ys)
            fx, fy = (xs - x0).astype(D), (ys - y0).astype(D)
            gx, gy = (D(1) - fx).astype(D), (D(1) - fy).astype(D)
            bx = np.where(snap, xr, x0).astype(np.int64)
            by = np.where(snap, yr, y0).astype(np.int64)
            one, zero = np.ones((H, W), D), np.zeros((H, W), D)
            wt = [np.where(snap, one, gx * gy), np.where(snap, zero, fx * gy), np.where(snap, zero, gx * fy),
                  np.where(snap, zero, fx * fy)]
            tx = [bx, bx + 1, bx, bx + 1]
            ty = [by, by, by + 1, by + 1]
        acc, taps = [], []
        with np.errstate(all="ignore"):
            for k in range(4):
                inside = ok & (wt[k] > 0) & (tx[k] >= 0) & (tx[k] < W) & (ty[k] >= 0) & (ty[k] < H)
                cx, cy = np.clip(tx[k], 0, W - 1), np.clip(ty[k], 0, H - 1)
                r0, r1, r2 = hs[0][cy, cx], hs[1][cy, cx], hs[2][cy, cx]
                c = r0[..., 3]
                a = inside & (c > 0) & (c < np.inf)
                if not static:
                    a &= ~np.isnan(r1[..., 0]) == hit
                    nq = [r1[..., j] for j in range(3)]
                    dq = [(r2[..., j] - P[j]).astype(D) for j in range(3)]
                    geo = (dot(n_p, nq) >= normal_cos) & (np.abs(dot(dq, n_p)) <= (plane_dist * tbar) * dlen)
                    a &= geo | ~hit
                acc.append(a)
                taps.append((r0, r1, r2))
            wsum = np.zeros((H, W), D)
            for k in range(4):
                wsum = np.where(acc[k], wsum + wt[k], wsum).astype(D)
            for k in range(4):
                r0, r1, r2 = taps[k]
                wn = (wt[k] / np.where(acc[k], wsum, D(1))).astype(D)
                vals = [r0[..., 0], r0[..., 1], r0[..., 2], r0[..., 3], r1[..., 3], r2[..., 3]]
                for j in range(6):
                    h[j] = np.where(acc[k], h[j] + wn * vals[j], h[j]).astype(D)
                has |= acc[k]
            over = has & (h[3] > max_history)
            scale = (max_history / np.where(over, h[3], D(1))).astype(D)
            for j in (0, 1, 2, 4, 5):
                h[j] = np.where(over, h[j] * scale, h[j]).astype(D)
            h[3] = np.where(over, max_history, h[3]).astype(D)
    info.update(has=has, hcount=h[3])
    return h, has, hit, n_p, info


def reproject(normal, depth, cam, prev, hist, motion=None, normal_cos=0.0, plane_dist=0.0, max_history=0.0, dtype=F, info=None):
    """srtTemporalReprojectMotion's two planes, (2, H, W, 4): {h.r, h.g, h.b, h.count} and {h.S1, h.S2, 0, has}."""
    h, has, _, _, inf = _reprojected(normal, depth, cam, prev, hist, motion, normal_cos, plane_dist, max_history, dtype)
    if info is not None:
        info.update(inf)
    out = np.zeros((2,) + normal.shape[:2] + (4,), dtype)
    for k in range(4):
        out[0][..., k] = h[k]
    out[1][..., 0], out[1][..., 1], out[1][..., 3] = h[4], h[5], has.astype(dtype)
    return out


def accumulate(beauty, moments, normal, position, depth, albedo, cam, prev, hist, motion=None, normal_cos=0.0, plane_dist=0.0,
               max_history=0.0, demodulate=False, dtype=F, info=None):
    """srtTemporalAccumulateMotion: (beauty_out, moments_out, history_out) as temporal_ref.accumulate returns them.  motion:
    the resolved motion plane (H, W, 4), sums with counts, or None for srtTemporalAccumulate itself."""
    D = dtype
    H, W = beauty.shape[:2]
    h, has, hit, n_p, inf = _reprojected(normal, depth, cam, prev, hist, motion, normal_cos, plane_dist, max_history, D)
    if info is not None:
        info.update(inf)
    b = beauty.astype(D)
    m = moments.astype(D) if moments is not None else None
    ps = position.astype(D)
    with np.errstate(all="ignore"):
        Q = [T._mean(ps[..., k], ps[..., 3], D) for k in range(3)]
        if demodulate:
            al = albedo.astype(D)
            at = [np.maximum(T._mean(al[..., k], al[..., 3], D), D(F(T.ALBEDO_MIN))) for k in range(3)]
            la = (D(F(0.2126)) * at[0] + D(F(0.7152)) * at[1] + D(F(0.0722)) * at[2]).astype(D)
            la2 = (la * la).astype(D)
        S1 = m[..., 0] if m is not None else np.zeros((H, W), D)
        S2 = m[..., 1] if m is not None else np.zeros((H, W), D)
        n = b[..., 3]
        usable = (n > 0) & np.isfinite(n) & np.isfinite(b[..., 0]) & np.isfinite(b[..., 1]) & np.isfinite(b[..., 2])
        if m is not None:
            usable &= np.isfinite(S1) & np.isfinite(S2)
        add = has & usable
        out_b = b.copy()
        out_m = np.zeros((H, W, 4), D)
        for k in range(3):
            out_b[..., k] = np.where(add, b[..., k] + (at[k] * h[k] if demodulate else h[k]), b[..., k])
        cnt = np.where(add, n + h[3], n).astype(D)
        out_b[..., 3] = cnt
        out_m[..., 0] = np.where(add, S1 + (la * h[4] if demodulate else h[4]), S1)
        out_m[..., 1] = np.where(add, S2 + (la2 * h[5] if demodulate else h[5]), S2)
        out_m[..., 3] = cnt
        new = np.zeros((3, H, W, 4), D)
        cur = [b[..., k] / at[k] if demodulate else b[..., k] for k in range(3)] + [n, S1 / la if demodulate else S1,
                                                                                   S2 / la2 if demodulate else S2]
        res = [np.where(usable, np.where(has, h[j] + cur[j], cur[j]), np.where(has, h[j], D(0))).astype(D) for j in range(6)]
        for k in range(4):
            new[0][..., k] = res[k]
        new[1][..., 3], new[2][..., 3] = res[4], res[5]
        new[1][..., 0] = np.where(hit, n_p[0], D(np.nan))
        for k in (1, 2):
            new[1][..., k] = np.where(hit, n_p[k], D(0))
        for k in range(3):
            new[2][..., k] = np.where(hit, Q[k], D(0))
    return out_b, out_m, new
