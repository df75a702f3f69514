"""NumPy reference of the denoiser with the sample variance (include/srt_hip.h "Sample variance", srtDenoiseMoments).

The filter is tests/denoise_ref.py's own; only the level-0 variance differs: `denoise` passes it an override `v0` (a
per-pixel array, NaN where the spatial estimate stays), and `sample_variance` computes the override from a resolved
moments plane as the kernel does (the subtraction in double, the division by lum(a~)^2 in float)."""
import numpy as np

import denoise_ref as R
from denoise_ref import ALBEDO_MIN, F, lum, mean

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
            v0=None, moments=None, intermediates=None):
    """denoise_ref.denoise with the level-0 variance replaced where `v0` is not NaN.  moments (resolved plane) computes v0
    by sample_variance and takes the moments' sigma_l default; neither given: denoise_ref.denoise exactly."""
    if moments is not None:
        v0 = sample_variance(moments, albedo, demodulate)
        sigma_l = sigma_l or MOMENTS_DEFAULT_SIGMA_L
    return R.denoise(beauty, normal, depth, albedo, iterations=iterations, demodulate=demodulate, sigma_l=sigma_l,
                     sigma_n=sigma_n, sigma_z=sigma_z, v0=v0, intermediates=intermediates)
