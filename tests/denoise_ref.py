"""NumPy reference of the denoiser (include/srt_hip.h "Denoiser", csrc/srt_denoise.hip), fp32 throughout.

It follows the header's math operation by operation and sums the taps in the kernel's order (rows outer, columns inner);
the kernel differs only where it evaluates exp and the normal power with the hardware's v_exp_f32 / v_log_f32 and
divides by a reciprocal.  The header's underflow rule is `_exp`: an exponential below 2^-126 counts as 0.

tests/denoise_f64.py states the same formulas in float64, written from the header alone; tests/test_denoise_ref.py holds
this file to it.  `denoise(..., intermediates={})` fills the dict with what the kernel keeps between its passes (the scratch
srtTestDenoiseScratch reads back): hit, n, z, grad and levels[k] = (valid, e, v) after k levels, k = 0 .. iterations."""
import numpy as np

F = np.float32
H5 = np.array([1, 4, 6, 4, 1], F) / F(16)
K3 = np.array([0.25, 0.5, 0.25], F)
ALBEDO_MIN, DEPTH_EPS, LUM_EPS = F(1e-3), F(1e-3), F(1e-10)
DEFAULTS = dict(iterations=5, sigma_l=4.0, sigma_n=16.0, sigma_z=1.0)


TINY = np.finfo(F).tiny  # 2^-126


def _exp(t):
    """exp(t) in float32, 0 where the result is below the normal range (the hardware exponential returns no denormals)."""
    x = np.exp(t)
    return np.where(x < TINY, F(0), x).astype(F)


def mean(plane):
    """sum / count per channel, 0 where the count is 0 (srtRenderFeatureImage's float division)."""
    s, n = plane[..., :3], plane[..., 3:4]
    return np.where(n != 0, s / np.where(n != 0, n, F(1)), F(0)).astype(F)


def lum(e):
    return F(0.2126) * e[..., 0] + F(0.7152) * e[..., 1] + F(0.0722) * e[..., 2]


def _shift(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx] where that is inside the image, else `fill`; and the inside mask."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    inside = np.zeros((H, W), bool)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return out, inside


class _Guide:
    def __init__(self, normal, depth):
        self.hit = normal[..., 3] > 0
        nm = mean(normal)
        ln = np.sqrt(nm[..., 0] * nm[..., 0] + nm[..., 1] * nm[..., 1] + nm[..., 2] * nm[..., 2])
        n = np.where((ln > 0)[..., None], nm / np.where(ln > 0, ln, F(1))[..., None], F(0)).astype(F)
        self.n = np.where(self.hit[..., None], n, F(0))
        self.z = np.where(self.hit, mean(depth)[..., 0], F(0))
        self.grad = [self._one_sided(1, 0), self._one_sided(0, 1)]

    def _one_sided(self, ax, ay):
        zl, _ = _shift(self.z, -ax, -ay, F(0))
        zh, _ = _shift(self.z, ax, ay, F(0))
        hl, _ = _shift(self.hit, -ax, -ay, False)
        hh, _ = _shift(self.hit, ax, ay, False)
        dl, dh = self.z - zl, zh - self.z
        g = np.where(hl & hh, np.where(np.abs(dh) < np.abs(dl), dh, dl), np.where(hl, dl, np.where(hh, dh, F(0))))
        return np.where(self.hit, g, F(0)).astype(F)

    def log_weight(self, dx, dy, sigma_n, sigma_z):
        """(tap allowed, sigmaN ln(max(0, n_p.n_q)) - a_z) for the neighbour at offset (dx, dy); 0 between two misses."""
        nq, _ = _shift(self.n, dx, dy, F(0))
        zq, _ = _shift(self.z, dx, dy, F(0))
        hq, _ = _shift(self.hit, dx, dy, False)
        both = self.hit & hq
        ok = both | (~self.hit & ~hq)
        d = np.maximum(self.n[..., 0] * nq[..., 0] + self.n[..., 1] * nq[..., 1] + self.n[..., 2] * nq[..., 2], F(0))
        den = sigma_z * np.abs(self.grad[0] * F(dx) + self.grad[1] * F(dy)) + DEPTH_EPS * self.z
        az = np.abs(self.z - zq) / den
        t = np.where(both, sigma_n * np.log(d) - az, F(0))
        return ok, t.astype(F)


def denoise(beauty, normal, depth, albedo=None, iterations=0, demodulate=False, sigma_l=0.0, sigma_n=0.0, sigma_z=0.0,
            v0=None, intermediates=None):
    """beauty, normal, depth, albedo: (H, W, 4) float32 image-order sums with counts.  A parameter of 0 takes its default.
    v0: a per-pixel override of the level-0 variance, NaN where the spatial estimate stays (denoise_moments_ref).
    intermediates: a dict to fill (see above).
    Returns (out, rgba): (H, W, 4) float32, rgb = the denoised mean, w = the beauty count; (H, W, 4) uint8."""
    iterations = iterations or DEFAULTS["iterations"]
    sigma_l, sigma_n, sigma_z = (F(s or DEFAULTS[k]) for s, k in ((sigma_l, "sigma_l"), (sigma_n, "sigma_n"), (sigma_z, "sigma_z")))
    beauty = np.asarray(beauty, F)
    with np.errstate(all="ignore"):
        g = _Guide(np.asarray(normal, F), np.asarray(depth, F))
        cnt = beauty[..., 3]
        c = (beauty[..., :3] / np.where(cnt > 0, cnt, F(1))[..., None]).astype(F)
        valid = (cnt > 0) & np.isfinite(c).all(axis=-1)
        at = np.maximum(mean(np.asarray(albedo, F)), ALBEDO_MIN) if demodulate else np.ones_like(c)
        e = np.where(valid[..., None], c / at, F(0)).astype(F)
        el = lum(e)
        # level-0 variance over the 7x7 window
        sw = np.zeros(cnt.shape, F)
        s1, s2 = np.zeros_like(sw), np.zeros_like(sw)
        l0 = np.where(valid, el, F(0))  # moments about l_p (0 for a centre that is not valid)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                ok, t = g.log_weight(dx, dy, sigma_n, sigma_z)
                lq, _ = _shift(el, dx, dy, F(0))
                vq, _ = _shift(valid, dx, dy, False)
                w = np.where(ok & vq, _exp(t), F(0))
                dl = lq - l0
                sw, s1, s2 = sw + w, s1 + w * dl, s2 + w * (dl * dl)
        m1, m2 = s1 / np.where(sw > 0, sw, F(1)), s2 / np.where(sw > 0, sw, F(1))
        v = np.where(sw > 0, m2 - m1 * m1, F(0))
        v = np.where(v > 0, v, F(0)).astype(F)
        if v0 is not None:
            v0 = np.asarray(v0, F)
            v = np.where(np.isnan(v0), v, v0).astype(F)
        if intermediates is not None:
            intermediates.update(hit=g.hit, n=g.n, z=g.z, grad=np.stack(g.grad, -1), levels=[(valid, e, v)])
        for lv in range(iterations):
            s = 1 << lv
            gs, ks = np.zeros_like(v), np.zeros_like(v)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    vq, inside = _shift(v, dx, dy, F(0))
                    k = K3[dx + 1] * K3[dy + 1]
                    gs, ks = gs + np.where(inside, k * vq, F(0)), ks + np.where(inside, k, F(0))
            gvar = gs / ks
            lp = np.where(valid, lum(e), F(0))
            ep = np.where(valid[..., None], e, F(0))  # colour sums about e_p (0 for a centre that is not valid)
            den = sigma_l * np.sqrt(gvar) + LUM_EPS
            sw = np.zeros_like(v)
            se, sv = np.zeros_like(e), np.zeros_like(v)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ok, t = g.log_weight(dx * s, dy * s, sigma_n, sigma_z)
                    eq, _ = _shift(e, dx * s, dy * s, F(0))
                    vq, _ = _shift(v, dx * s, dy * s, F(0))
                    qv, _ = _shift(valid, dx * s, dy * s, False)
                    al = np.where(valid, np.abs(lp - lum(eq)) / den, F(0))
                    w = np.where(ok & qv, (H5[dx + 2] * H5[dy + 2]) * _exp(t - al), F(0)).astype(F)
                    sw, se, sv = sw + w, se + w[..., None] * (eq - ep), sv + (w * w) * vq
            valid = sw > 0
            d = np.where(valid, sw, F(1))
            e = np.where(valid[..., None], ep + se / d[..., None], F(0)).astype(F)
            v = np.where(valid, sv / d / d, F(0)).astype(F)
            if intermediates is not None:
                intermediates["levels"].append((valid, e, v))
        rgb = np.where(valid[..., None], e * at, F(0)).astype(F)
        out = np.concatenate([rgb, cnt[..., None]], axis=-1).astype(F)
        q = F(256) * np.clip(np.sqrt(rgb), F(0), F(0.999))
        rgba = np.concatenate([np.where(np.isnan(q), 0, q).astype(np.uint8), np.full(cnt.shape + (1,), 255, np.uint8)], -1)
    return out, rgba
