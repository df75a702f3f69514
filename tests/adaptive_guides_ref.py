"""NumPy restatement of the guide planes of a guided adaptive render (include/srt_hip.h srtRenderAdaptiveGuided,
srtRenderTemporalAdaptiveGuided): image-order feature sums that follow the rounds.

It needs no knowledge of the decisions.  The schedule is deterministic, so a tile's final count c says it was active in
launch r exactly when n_r <= c.  The expected planes are the resolved whole-frame feature sums of [0, n_0), plus, for each
r >= 1, the resolved whole-frame feature sums of [n_{r-1}, n_r) masked to the tiles with c >= n_r, added in float32 -- which
rests on srtRenderFeatureTiles alone (a listed tile's sums are the same tile's of a full-frame pass over that range)."""
import copy

import numpy as np

import adaptive_ref as A

F = np.float32
TILE = A.TILE


def tile_counts(count):
    """(tilesY, tilesX) float32 from an (H, W) plane of per-pixel counts; every in-image pixel of a tile has the same."""
    h, w = count.shape
    ty, tx = -(-h // TILE), -(-w // TILE)
    pad = np.full((ty * TILE, tx * TILE), np.nan, F)
    pad[:h, :w] = count
    t = pad.reshape(ty, TILE, tx, TILE)
    lo, hi = np.nanmin(t, axis=(1, 3)), np.nanmax(t, axis=(1, 3))
    assert (lo == hi).all(), "a tile's pixels differ in their counts"
    return hi


def emulate_planes(feature_sums, p, spp_max, count, first=None):
    """feature_sums(q) -> the resolved whole-frame feature sums of q's sample range, a list of (H, W, 4) float32 (None for a
    plane that is not followed); count = the finished render's (H, W) per-pixel sample counts (accum[..., 3]); first = the
    planes of [sampleFirst, sampleFirst + spp) when the caller has them already.  Returns the expected planes."""
    H, W = p.imageHeight, p.imageWidth
    c = tile_counts(np.asarray(count, F))
    planes = [None if x is None else np.array(x, F) for x in (feature_sums(p) if first is None else first)]
    n = p.spp
    for b in A.schedule(p.spp, spp_max)[1:]:
        active = c >= n + b
        if not active.any():
            break
        q = copy.copy(p)
        q.spp, q.sampleFirst = b, p.sampleFirst + n
        q.sppChunks = min(p.sppChunks, b) if p.sppChunks > 0 else 0
        add = feature_sums(q)
        mask = A.pixel_mask(active, H, W)
        for k, plane in enumerate(planes):
            if plane is not None:
                plane[mask] = plane[mask] + np.asarray(add[k], F)[mask]
        n += b
    return planes


def tile_list(tiles_xy):
    """uint32 list entries tx | ty << 16 from (tx, ty) pairs."""
    return np.array([tx | ty << 16 for tx, ty in tiles_xy], np.uint32)
