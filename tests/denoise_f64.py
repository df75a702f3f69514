"""The denoiser as include/srt_hip.h states it ("Denoiser", "Sample variance"), in float64.

Written from the header's formulas, not from csrc/srt_denoise.hip or tests/denoise_ref.py: the inputs are the float32 planes,
every operation after them is float64, the constants are the float32 values the header's literals denote (1e-3f, 1e-10f,
the luminance coefficients, the sigmas as the float32 parameters hold them).  Taps are summed in no particular order.  The
header's underflow rule is applied: a tap whose exponential is below 2^-126 has weight 0.

tests/test_denoise_ref.py holds the fp32 reference to this file; tests/test_gpu_denoise_edges.py holds the kernel to it."""
import numpy as np

D = np.float64
_f = lambda x: D(np.float32(x))  # noqa: E731  the float32 literal's value
ALBEDO_MIN, DEPTH_EPS, LUM_EPS = _f(1e-3), _f(1e-3), _f(1e-10)
LUM = (_f(0.2126), _f(0.7152), _f(0.0722))
H5 = np.array([1, 4, 6, 4, 1], D) / 16
K3 = np.array([1, 2, 1], D) / 4
EXP_MIN = D(2.0) ** -126
DEFAULT_ITERATIONS, DEFAULT_SIGMA_L, DEFAULT_SIGMA_N, DEFAULT_SIGMA_Z = 5, 4.0, 16.0, 1.0


def lum(e):
    return LUM[0] * e[..., 0] + LUM[1] * e[..., 1] + LUM[2] * e[..., 2]


def _mean(plane):
    """sum / count, 0 where count == 0: (H, W, 3)"""
    p = np.asarray(plane, np.float32).astype(D)
    n = p[..., 3:4]
    return np.where(n != 0, p[..., :3] / np.where(n != 0, n, 1), 0.0)


def _at(a, dx, dy, fill):
    """a at pixel offset (dx, dy): q = p + (dx, dy); `fill` outside the image."""
    H, W = a.shape[:2]
    out = np.full(a.shape, fill, a.dtype)
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    yi, xi = np.nonzero((ys >= 0) & (ys < H))[0], np.nonzero((xs >= 0) & (xs < W))[0]
    if len(yi) and len(xi):
        out[np.ix_(yi, xi)] = a[np.ix_(ys[yi], xs[xi])]
    return out


def _exp(t):
    """exp(t); 0 where it is below 2^-126 (the header's underflow rule)"""
    x = np.exp(t)
    return np.where(x < EXP_MIN, 0.0, x)


class _Edges:
    """hit, n, z, the depth gradient, and the geometric exponent of a tap"""

    def __init__(self, normal, depth, sigma_n, sigma_z):
        self.sn, self.sz = sigma_n, sigma_z
        self.hit = np.asarray(normal, np.float32)[..., 3] > 0
        m = _mean(normal)
        ln = np.sqrt((m * m).sum(-1))
        self.n = np.where((self.hit & (ln > 0))[..., None], m / np.where(ln > 0, ln, 1)[..., None], 0.0)
        self.z = np.where(self.hit, _mean(depth)[..., 0], 0.0)
        self.grad = np.stack([self._one_sided(1, 0), self._one_sided(0, 1)], -1)

    def _one_sided(self, ax, ay):
        back = self.z - _at(self.z, -ax, -ay, 0.0)
        fwd = _at(self.z, ax, ay, 0.0) - self.z
        hb, hf = _at(self.hit, -ax, -ay, False), _at(self.hit, ax, ay, False)
        # the smaller magnitude, a tie the backward one; one hit neighbour: that one; none: 0
        both = np.where(np.abs(fwd) < np.abs(back), fwd, back)
        g = np.where(hb & hf, both, np.where(hb, back, np.where(hf, fwd, 0.0)))
        return np.where(self.hit, g, 0.0)

    def exponent(self, dx, dy):
        """(allowed, sigmaN ln(max(0, n_p.n_q)) - a_z) towards q = p + (dx, dy): -inf where w_n = 0, 0 between misses;
        not allowed between a hit and a miss and outside the image"""
        inside = _at(np.ones(self.hit.shape, bool), dx, dy, False)
        hq = _at(self.hit, dx, dy, False)
        both = self.hit & hq & inside
        allowed = inside & (self.hit == hq)
        d = np.maximum((self.n * _at(self.n, dx, dy, 0.0)).sum(-1), 0.0)
        den = self.sz * np.abs(self.grad[..., 0] * dx + self.grad[..., 1] * dy) + DEPTH_EPS * self.z
        az = np.abs(self.z - _at(self.z, dx, dy, 0.0)) / den
        return allowed, np.where(both, self.sn * np.log(d) - az, 0.0)


def sample_variance(moments, albedo_div=None):
    """max(0, S2 - S1^2 / n) / (n (n - 1)) where n >= 2 and S1, S2 are finite, NaN elsewhere; / lum(a~)^2 with a divisor"""
    m = np.asarray(moments, np.float32)
    use = (m[..., 3] >= 2) & np.isfinite(m[..., 0]) & np.isfinite(m[..., 1])
    s1, s2, n = (m[..., k].astype(D) for k in (0, 1, 3))
    n = np.where(use, n, 2.0)
    v = np.maximum(s2 - s1 * s1 / n, 0.0) / (n * (n - 1))
    if albedo_div is not None:
        v = v / lum(albedo_div) ** 2
    return np.where(use, v, np.nan)


def denoise(beauty, normal, depth, albedo=None, moments=None, iterations=0, demodulate=False, sigma_l=0.0, sigma_n=0.0,
            sigma_z=0.0, intermediates=None):
    """Planes (H, W, 4) float32 sums with counts; a parameter of 0 takes its default.  Returns the (H, W, 4) float64 output
    (rgb = the denoised mean, w = the beauty count).  intermediates: a dict that receives hit, n, z, grad and
    levels[k] = (valid, e, v) after k levels, k = 0 .. iterations."""
    iterations = iterations or DEFAULT_ITERATIONS
    sl, sn, sz = (_f(s) if s else D(d) for s, d in ((sigma_l, DEFAULT_SIGMA_L), (sigma_n, DEFAULT_SIGMA_N), (sigma_z, DEFAULT_SIGMA_Z)))
    b = np.asarray(beauty, np.float32).astype(D)
    with np.errstate(all="ignore"):
        cnt = b[..., 3]
        c = b[..., :3] / np.where(cnt > 0, cnt, 1)[..., None]
        valid = (cnt > 0) & np.isfinite(c).all(-1)
        adiv = np.maximum(_mean(albedo), ALBEDO_MIN) if demodulate else np.ones_like(c)
        e = np.where(valid[..., None], c / adiv, 0.0)
        g = _Edges(normal, depth, sn, sz)
        # level-0 variance: the weighted moments of l over the valid pixels of the 7x7 window, about l_p
        l = np.where(valid, lum(e), 0.0)
        sw, s1, s2 = (np.zeros(cnt.shape, D) for _ in range(3))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                allowed, t = g.exponent(dx, dy)
                w = np.where(allowed & _at(valid, dx, dy, False), _exp(t), 0.0)
                dl = _at(l, dx, dy, 0.0) - l
                sw, s1, s2 = sw + w, s1 + w * dl, s2 + w * dl * dl
        den = np.where(sw > 0, sw, 1.0)
        v = np.where(sw > 0, np.maximum(s2 / den - (s1 / den) ** 2, 0.0), 0.0)
        if moments is not None:
            sv = sample_variance(moments, adiv if demodulate else None)
            v = np.where(np.isnan(sv), v, sv)
        levels = [(valid, e, v)]
        for i in range(iterations):
            s = 1 << i
            gs, ks = np.zeros_like(v), np.zeros_like(v)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    inside = _at(np.ones(v.shape, bool), dx, dy, False)
                    k = K3[dx + 1] * K3[dy + 1]
                    gs, ks = gs + np.where(inside, k * _at(v, dx, dy, 0.0), 0.0), ks + np.where(inside, k, 0.0)
            lden = sl * np.sqrt(gs / ks) + LUM_EPS
            lp = np.where(valid, lum(e), 0.0)
            ep = np.where(valid[..., None], e, 0.0)
            sw, sv = np.zeros_like(v), np.zeros_like(v)
            se = np.zeros_like(e)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    allowed, t = g.exponent(dx * s, dy * s)
                    eq = _at(e, dx * s, dy * s, 0.0)
                    al = np.where(valid, np.abs(lp - lum(eq)) / lden, 0.0)
                    w = np.where(allowed & _at(valid, dx * s, dy * s, False), H5[dx + 2] * H5[dy + 2] * _exp(t - al), 0.0)
                    sw, se, sv = sw + w, se + w[..., None] * (eq - ep), sv + w * w * _at(v, dx * s, dy * s, 0.0)
            valid = sw > 0
            den = np.where(valid, sw, 1.0)
            e = np.where(valid[..., None], ep + se / den[..., None], 0.0)
            v = np.where(valid, sv / den ** 2, 0.0)
            levels.append((valid, e, v))
        out = np.concatenate([np.where(valid[..., None], e * adiv, 0.0), cnt[..., None]], -1)
    if intermediates is not None:
        intermediates.update(hit=g.hit, n=g.n, z=g.z, grad=g.grad, levels=levels)
    return out
