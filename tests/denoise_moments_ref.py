"""NumPy reference of the denoiser with the sample variance (include/srt_hip.h "Sample variance", srtDenoiseMoments).

The filter is tests/denoise_ref.py's, operation by operation; only the level-0 variance differs: `denoise` takes an
override `v0` (a per-pixel array, NaN where the spatial estimate stays), and `sample_variance` computes the override from
a resolved moments plane as the kernel does (the subtraction in double, the division by lum(a~)^2 in float)."""
import numpy as np

from denoise_ref import ALBEDO_MIN, DEFAULTS, DEPTH_EPS, F, H5, K3, LUM_EPS, _Guide, _shift, lum, mean

MOMENTS_DEFAULT_SIGMA_L = 4.0  # SRT_DENOISE_MOMENTS_DEFAULT_SIGMA_LUMINANCE


def sample_variance(moments, albedo=None, demodulate=False):
    """v_p = max(0, S2 - S1^2 / n) / (n (n - 1)) for pixels with n >= 2 and finite S1, S2 (NaN elsewhere: keep the spatial
    estimate); divided by lum(a~_p)^2 when demodulating."""
    m = np.asarray(moments, F)
    s1, s2, n = m[..., 0].astype(np.float64), m[..., 1].astype(np.float64), m[..., 3].astype(np.float64)
    use = (m[..., 3] >= F(2)) & np.isfinite(m[..., 0]) & np.isfinite(m[..., 1])
    with np.errstate(all="ignore"):
        nn = np.where(use, n, 2.0)
        d = np.maximum(s2 - s1 * s1 / nn, 0.0)
        v = (d / (nn * (nn - 1.0))).astype(F)
        if demodulate:
            at = np.maximum(mean(np.asarray(albedo, F)), ALBEDO_MIN)
            la = lum(at).astype(F)
            v = (v / (la * la)).astype(F)
    return np.where(use, v, F(np.nan)).astype(F)


def denoise(beauty, normal, depth, albedo=None, iterations=0, demodulate=False, sigma_l=0.0, sigma_n=0.0, sigma_z=0.0,
            v0=None, moments=None):
    """denoise_ref.denoise with the level-0 variance replaced where `v0` is not NaN.  moments (resolved plane) computes v0
    by sample_variance and takes the moments' sigma_l default; neither given: denoise_ref.denoise exactly."""
    if moments is not None:
        v0 = sample_variance(moments, albedo, demodulate)
        sigma_l = sigma_l or MOMENTS_DEFAULT_SIGMA_L
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
        # level-0 variance over the 7x7 window (denoise_ref), then the override
        sw = np.zeros(cnt.shape, F)
        s1, s2 = np.zeros_like(sw), np.zeros_like(sw)
        l0 = np.where(valid, el, F(0))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                ok, t = g.log_weight(dx, dy, sigma_n, sigma_z)
                lq, _ = _shift(el, dx, dy, F(0))
                vq, _ = _shift(valid, dx, dy, False)
                w = np.where(ok & vq, np.exp(t), F(0))
                dl = lq - l0
                sw, s1, s2 = sw + w, s1 + w * dl, s2 + w * (dl * dl)
        m1, m2 = s1 / np.where(sw > 0, sw, F(1)), s2 / np.where(sw > 0, sw, F(1))
        v = np.where(sw > 0, m2 - m1 * m1, F(0))
        v = np.where(v > 0, v, F(0)).astype(F)
        if v0 is not None:
            v0 = np.asarray(v0, F)
            v = np.where(np.isnan(v0), v, v0).astype(F)
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
            ep = np.where(valid[..., None], e, F(0))
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
                    w = np.where(ok & qv, (H5[dx + 2] * H5[dy + 2]) * np.exp(t - al), F(0)).astype(F)
                    sw, se, sv = sw + w, se + w[..., None] * (eq - ep), sv + (w * w) * vq
            valid = sw > 0
            d = np.where(valid, sw, F(1))
            e = np.where(valid[..., None], ep + se / d[..., None], F(0)).astype(F)
            v = np.where(valid, sv / d / d, F(0)).astype(F)
        rgb = np.where(valid[..., None], e * at, F(0)).astype(F)
        out = np.concatenate([rgb, cnt[..., None]], axis=-1).astype(F)
        q = F(256) * np.clip(np.sqrt(rgb), F(0), F(0.999))
        rgba = np.concatenate([np.where(np.isnan(q), 0, q).astype(np.uint8), np.full(cnt.shape + (1,), 255, np.uint8)], -1)
    return out, rgba
