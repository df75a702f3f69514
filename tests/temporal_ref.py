"""NumPy reference of srtTemporalAccumulate (include/srt_hip.h "Temporal accumulation"), in the header's operation order.

Everything is evaluated in `dtype` (float32: what the kernel computes, bit for bit -- the library is built without
multiply-add contraction and with IEEE division and sqrt; float64: the yardstick for how far float32 rounding moves the
result).  Buffers are (H, W, 4) arrays of sums with counts, a history is (3, H, W, 4); cameras are abi.SrtCamera or
anything with origin / lleft / horizontal / vertical / w attributes."""
import numpy as np

SNAP = 2.0 ** -6
DEFAULT_NORMAL_COS, DEFAULT_PLANE_DIST, DEFAULT_MAX_HISTORY = 0.5, 0.02, 64.0
ALBEDO_MIN = 1e-3
CAMERA_FIELDS = ("origin", "lleft", "horizontal", "vertical", "w")


def _vec(cam, name, T):
    return [T(np.float32(c)) for c in getattr(cam, name)]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def same_camera(cam, prev):
    """The static-camera rule compares the fields the projection reads, bit for bit."""
    return all(np.array_equal(np.float32(list(getattr(cam, f))).view(np.uint32), np.float32(list(getattr(prev, f))).view(np.uint32))
               for f in CAMERA_FIELDS)


def _mean(s, c, T):
    with np.errstate(all="ignore"):
        return np.where(c != 0, s / np.where(c != 0, c, T(1)), T(0)).astype(T)


def pixel_ray(cam, W, H, T=np.float32):
    """d of every pixel centre and its length: ((lleft + s_c horizontal) + t_c vertical) - origin."""
    x = np.arange(W, dtype=T)[None, :]
    y = np.arange(H, dtype=T)[:, None]
    sc = (x + T(0.5)) / T(W - 1)
    tc = ((T(H) - y) + T(0.5)) / T(H - 1)
    o, ll, hz, vt = (_vec(cam, f, T) for f in ("origin", "lleft", "horizontal", "vertical"))
    d = [np.broadcast_to(((ll[k] + sc * hz[k]) + tc * vt[k]) - o[k], (H, W)).astype(T) for k in range(3)]
    return d, np.sqrt(_dot(d, d)).astype(T)


def project(prev, v, W, H, T=np.float32):
    """(xf, yf, z) of the points prev.origin + v through prev's lens centre onto its focus plane."""
    o, ll, hz, vt, w = (_vec(prev, f, T) for f in CAMERA_FIELDS)
    e = [o[k] - ll[k] for k in range(3)]
    f = _dot(e, w)
    with np.errstate(all="ignore"):
        z = -_dot(v, w)
        k = f / z
        g = [e[c] + k * v[c] for c in range(3)]
        s = _dot(g, hz) / _dot(hz, hz)
        t = _dot(g, vt) / _dot(vt, vt)
        xf = s * T(W - 1) - T(0.5)
        yf = (T(H) + T(0.5)) - t * T(H - 1)
    return xf.astype(T), yf.astype(T), z.astype(T)


def reproject(cam, prev, tbar, hit, W, H, T=np.float32):
    """Previous-frame pixel coordinates of every pixel: (xf, yf, ok, P, d, dlen)."""
    d, dlen = pixel_ray(cam, W, H, T)
    o = _vec(cam, "origin", T)
    po = _vec(prev, "origin", T)
    P = [(o[k] + tbar * d[k]).astype(T) for k in range(3)]
    v = [np.where(hit, P[k] - po[k], d[k]).astype(T) for k in range(3)]
    xf, yf, z = project(prev, v, W, H, T)
    with np.errstate(invalid="ignore"):
        ok = (z > 0) & (xf > -1) & (xf < W) & (yf > -1) & (yf < H)
    return xf, yf, ok, P, d, dlen


def round_trip_error(cam, W, H, depth, T=np.float32):
    """The snap measurement: max |xf - x|, |yf - y| of pixel -> P at `depth` -> the same camera."""
    tbar = np.full((H, W), depth, T)
    xf, yf, ok, _, _, _ = reproject(cam, cam, tbar, np.ones((H, W), bool), W, H, T)
    assert ok.all()
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    return float(np.abs(xf.astype(np.float64) - x).max()), float(np.abs(yf.astype(np.float64) - y).max())


def accumulate(beauty, moments, normal, position, depth, albedo, cam, prev, hist, normal_cos=0.0, plane_dist=0.0,
               max_history=0.0, demodulate=False, dtype=np.float32, info=None):
    """Returns (beauty_out, moments_out, history_out).  moments / albedo / hist may be None.  info: a dict that receives
    xf, yf, the per-pixel accepted mask `has` and the reprojected count `hcount`."""
    T = dtype
    H, W = beauty.shape[:2]
    normal_cos = T(np.float32(normal_cos or DEFAULT_NORMAL_COS))
    plane_dist = T(np.float32(plane_dist or DEFAULT_PLANE_DIST))
    max_history = T(np.float32(max_history or DEFAULT_MAX_HISTORY))
    b = beauty.astype(T)
    m = moments.astype(T) if moments is not None else None
    nm, ps, dp = normal.astype(T), position.astype(T), depth.astype(T)

    with np.errstate(all="ignore"):
        hit = nm[..., 3] > 0
        nv = [_mean(nm[..., k], nm[..., 3], T) for k in range(3)]
        ln = np.sqrt(_dot(nv, nv)).astype(T)
        good = (ln > 0) & (ln < np.inf)
        n_p = [np.where(good, nv[k] / np.where(good, ln, T(1)), T(0)).astype(T) for k in range(3)]
        tbar = _mean(dp[..., 0], dp[..., 3], T)
        Q = [_mean(ps[..., k], ps[..., 3], T) for k in range(3)]
        if demodulate:
            al = albedo.astype(T)
            at = [np.maximum(_mean(al[..., k], al[..., 3], T), T(np.float32(ALBEDO_MIN))) for k in range(3)]
            la = (T(np.float32(0.2126)) * at[0] + T(np.float32(0.7152)) * at[1] + T(np.float32(0.0722)) * at[2]).astype(T)
            la2 = (la * la).astype(T)
        S1 = m[..., 0] if m is not None else np.zeros((H, W), T)
        S2 = m[..., 1] if m is not None else np.zeros((H, W), T)
        n = b[..., 3]
        usable = (n > 0) & np.isfinite(n) & np.isfinite(b[..., 0]) & np.isfinite(b[..., 1]) & np.isfinite(b[..., 2])
        if m is not None:
            usable &= np.isfinite(S1) & np.isfinite(S2)

    # ---- the reprojected history h = {r, g, b, count, S1, S2}
    h = [np.zeros((H, W), T) for _ in range(6)]
    has = np.zeros((H, W), bool)
    xf = yf = None
    if hist is not None:
        hs = hist.astype(T)
        static = same_camera(cam, prev)
        if static:  # the pixel itself, no geometry tests
            ok = np.ones((H, W), bool)
            tx = [np.broadcast_to(np.arange(W)[None, :], (H, W))] * 4
            ty = [np.broadcast_to(np.arange(H)[:, None], (H, W))] * 4
            wt = [np.ones((H, W), T)] + [np.zeros((H, W), T)] * 3
        else:
            xf, yf, ok, P, d, dlen = reproject(cam, prev, tbar, hit, W, H, T)
            xs, ys = np.where(ok, xf, T(0)).astype(T), np.where(ok, yf, T(0)).astype(T)
            xr, yr = np.rint(xs), np.rint(ys)
            snap = (np.abs(xs - xr) <= T(SNAP)) & (np.abs(ys - yr) <= T(SNAP))
            x0, y0 = np.floor(xs), np.floor(ys)
            fx, fy = (xs - x0).astype(T), (ys - y0).astype(T)
            gx, gy = (T(1) - fx).astype(T), (T(1) - fy).astype(T)
            bx = np.where(snap, xr, x0).astype(np.int64)
            by = np.where(snap, yr, y0).astype(np.int64)
            one, zero = np.ones((H, W), T), np.zeros((H, W), T)
            wt = [np.where(snap, one, gx * gy), np.where(snap, zero, fx * gy), np.where(snap, zero, gx * fy),
                  np.where(snap, zero, fx * fy)]
            tx = [bx, bx + 1, bx, bx + 1]
            ty = [by, by, by + 1, by + 1]
        acc = []
        taps = []
        with np.errstate(all="ignore"):
            for k in range(4):
                inside = ok & (wt[k] > 0) & (tx[k] >= 0) & (tx[k] < W) & (ty[k] >= 0) & (ty[k] < H)
                cx, cy = np.clip(tx[k], 0, W - 1), np.clip(ty[k], 0, H - 1)
                r0, r1, r2 = hs[0][cy, cx], hs[1][cy, cx], hs[2][cy, cx]
                c = r0[..., 3]
                a = inside & (c > 0) & (c < np.inf)
                if not static:
                    hit_q = ~np.isnan(r1[..., 0])
                    a &= hit_q == hit
                    nq = [r1[..., j] for j in range(3)]
                    dq = [(r2[..., j] - P[j]).astype(T) for j in range(3)]
                    geo = (_dot(n_p, nq) >= normal_cos) & (np.abs(_dot(dq, n_p)) <= (plane_dist * tbar) * dlen)
                    a &= geo | ~hit
                acc.append(a)
                taps.append((r0, r1, r2))
            wsum = np.zeros((H, W), T)
            for k in range(4):
                wsum = np.where(acc[k], wsum + wt[k], wsum).astype(T)
            for k in range(4):
                r0, r1, r2 = taps[k]
                wn = (wt[k] / np.where(acc[k], wsum, T(1))).astype(T)
                vals = [r0[..., 0], r0[..., 1], r0[..., 2], r0[..., 3], r1[..., 3], r2[..., 3]]
                for j in range(6):
                    h[j] = np.where(acc[k], h[j] + wn * vals[j], h[j]).astype(T)
                has |= acc[k]
            over = has & (h[3] > max_history)
            scale = (max_history / np.where(over, h[3], T(1))).astype(T)
            for j in (0, 1, 2, 4, 5):
                h[j] = np.where(over, h[j] * scale, h[j]).astype(T)
            h[3] = np.where(over, max_history, h[3]).astype(T)
    if info is not None:
        info.update(xf=xf, yf=yf, has=has, hcount=h[3])

    # ---- outputs
    with np.errstate(all="ignore"):
        add = has & usable
        out_b = b.copy()
        out_m = np.zeros((H, W, 4), T)
        out_m[..., 0], out_m[..., 1], out_m[..., 3] = S1, S2, n
        for k in range(3):
            hk = at[k] * h[k] if demodulate else h[k]
            out_b[..., k] = np.where(add, b[..., k] + hk, b[..., k])
        cnt = np.where(add, n + h[3], n).astype(T)
        out_b[..., 3] = cnt
        out_m[..., 0] = np.where(add, S1 + (la * h[4] if demodulate else h[4]), S1)
        out_m[..., 1] = np.where(add, S2 + (la2 * h[5] if demodulate else h[5]), S2)
        out_m[..., 3] = cnt

        new = np.zeros((3, H, W, 4), T)
        cur = [b[..., k] / at[k] if demodulate else b[..., k] for k in range(3)] + [n, S1 / la if demodulate else S1,
                                                                                   S2 / la2 if demodulate else S2]
        res = []
        for j in range(6):
            both = h[j] + cur[j]
            res.append(np.where(usable, np.where(has, both, cur[j]), np.where(has, h[j], T(0))).astype(T))
        for k in range(4):
            new[0][..., k] = res[k]
        new[1][..., 3], new[2][..., 3] = res[4], res[5]
        new[1][..., 0] = np.where(hit, n_p[0], T(np.nan))
        for k in (1, 2):
            new[1][..., k] = np.where(hit, n_p[k], T(0))
        for k in range(3):
            new[2][..., k] = np.where(hit, Q[k], T(0))
    return out_b, out_m, new
