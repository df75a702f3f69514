"""NumPy restatement of tile-adaptive sampling (include/srt_hip.h "Adaptive sampling"): the schedule, the convergence rule
(float64, in the header's operation order), the active-set rule, the per-pixel-count resolve, and a whole adaptive render
emulated from full-frame range renders.  The emulation works because a listed tile is bit-identical to the same tile of a
full-frame render of the same sample range: each round takes render_image_moments of [n_{r-1}, n_r), masks it by the
active tiles and adds it in float32."""
import copy

import numpy as np

F = np.float32
TILE = 8


def schedule(n0, spp_max):
    """Samples per launch: b_0 = n_0, then b_r = min(n_{r-1}, sppMax - n_{r-1}) until n = sppMax."""
    out, n = [n0], n0
    while n < spp_max:
        b = min(n, spp_max - n)
        out.append(b)
        n += b
    return out


def converged(moments, thr):
    """(H, W) bool: the convergence test of each pixel's accumulated float moments {S1, S2, 0, n}."""
    s1 = moments[..., 0].astype(np.float64)
    s2 = moments[..., 1].astype(np.float64)
    n = moments[..., 3].astype(np.float64)
    with np.errstate(all="ignore"):
        mu = s1 / n
        d = s2 - (s1 * s1) / n
        v = np.maximum(d, 0.0) / (n * (n - 1.0))
        limit = 4.0 * (np.float64(F(thr)) * np.float64(F(thr)))
        ok = v < limit * np.maximum(mu, 2.0 ** -16)
    return ~(np.isfinite(s1) & np.isfinite(s2)) | ok


def tile_open(conv):
    """(tilesY, tilesX) bool: tiles with at least one in-image pixel that has not converged (padding counts as converged)."""
    H, W = conv.shape
    ty, tx = -(-H // TILE), -(-W // TILE)
    pad = np.ones((ty * TILE, tx * TILE), bool)
    pad[:H, :W] = conv
    return ~pad.reshape(ty, TILE, tx, TILE).all(axis=(1, 3))


def pixel_mask(tiles, H, W):
    return np.repeat(np.repeat(tiles, TILE, 0), TILE, 1)[:H, :W]


def resolve(accum):
    """srtResolveTiles's quantisation with the pixel's own count: sqrtf(c * (1.0f / w)), clamp to 0.999, x256, NaN -> 0."""
    with np.errstate(all="ignore"):
        scale = F(1.0) / accum[..., 3:4]
        g = np.sqrt((accum[..., :3] * scale).astype(F))
        q = F(256.0) * np.clip(g, F(0.0), F(0.999))
    out = np.zeros(accum.shape[:2] + (4,), np.uint8)
    out[..., :3] = np.where(np.isnan(q), 0, q).astype(np.uint8)
    out[..., 3] = 255
    return out


def display_error(moments):
    """(H, W) float64: the threshold a pixel needs to count as converged, sqrt(v / (4 max(mu, 2^-16)))."""
    s1, s2, n = (moments[..., k].astype(np.float64) for k in (0, 1, 3))
    with np.errstate(all="ignore"):
        v = np.maximum(s2 - (s1 * s1) / n, 0.0) / (n * (n - 1.0))
        return np.sqrt(v / (4.0 * np.maximum(s1 / n, 2.0 ** -16)))


def emulate(ctx, p, spp_max, thr):
    """A whole adaptive render from full-frame range renders.  Returns (accum, moments, rgba, active tile counts per
    launch, pixelSamples)."""
    H, W = p.imageHeight, p.imageWidth
    sched = schedule(p.spp, spp_max)
    accum, moments, _ = ctx.render_image_moments(p, want_rgba=False)
    n = p.spp
    active = np.ones((-(-H // TILE), -(-W // TILE)), bool)
    counts = [int(active.sum())]
    pixel_samples = H * W * p.spp
    for b in sched[1:]:
        active &= tile_open(converged(moments, thr))
        if not active.any():
            break
        q = copy.copy(p)
        q.spp, q.sampleFirst = b, p.sampleFirst + n
        q.sppChunks = min(p.sppChunks, b) if p.sppChunks > 0 else 0
        a2, m2, _ = ctx.render_image_moments(q, want_rgba=False)
        mask = pixel_mask(active, H, W)
        accum[mask] = accum[mask] + a2[mask]
        moments[mask] = moments[mask] + m2[mask]
        n += b
        counts.append(int(active.sum()))
        pixel_samples += int(mask.sum()) * b
    return accum, moments, resolve(accum), counts, pixel_samples
