"""NumPy restatement of the temporal-adaptive frame (include/srt_hip.h "Temporal-adaptive frames"), built from
tests/temporal_ref.py and tests/adaptive_ref.py as they are: the reprojected history through temporal_ref.accumulate, the
pooled moments as its moments output, the decisions through adaptive_ref.converged and tile_open."""
import copy

import numpy as np

import adaptive_ref as A
import temporal_ref as R

F = np.float32


def reproject_history(normal, position, depth, cam, prev, hist, normal_cos=0.0, plane_dist=0.0, max_history=0.0):
    """The two planes srtTemporalReproject writes, (2, H, W, 4): {h.r, h.g, h.b, h.count} and {h.S1, h.S2, 0, has}.
    temporal_ref.accumulate is run on an all-zero current frame of one sample without demodulation: the new history of a
    pixel with an accepted tap is then h + 0 in every channel, which is h bit for bit (h is a sum that starts from +0, so
    it is never -0), and `info` carries has and h.count."""
    H, W = normal.shape[:2]
    out = np.zeros((2, H, W, 4), F)
    if hist is None:
        return out
    zero = np.zeros((H, W, 4), F)
    zero[..., 3] = 1
    info = {}
    _, _, new = R.accumulate(zero, zero, normal, position, depth, None, cam, prev, hist, normal_cos, plane_dist, max_history,
                             False, info=info)
    has = info["has"]
    out[0][..., :3] = np.where(has[..., None], new[0][..., :3], F(0))
    out[0][..., 3] = np.where(has, info["hcount"], F(0))
    out[1][..., 0] = np.where(has, new[1][..., 3], F(0))
    out[1][..., 1] = np.where(has, new[2][..., 3], F(0))
    out[1][..., 3] = has
    return out


def pooled_moments(accum, moments, planes, cam, prev, hist, tp):
    """M~: dMomentsOut of srtTemporalAccumulate applied to the sums so far.  planes = [albedo, normal, position, depth];
    tp = dict(normal_cos, plane_dist, max_history, demodulate)."""
    return R.accumulate(accum, moments, planes[1], planes[2], planes[3], planes[0] if tp["demodulate"] else None, cam, prev, hist,
                        tp["normal_cos"], tp["plane_dist"], tp["max_history"], bool(tp["demodulate"]))[1]


def emulate_frame(ctx, p, spp_max, thr, planes, cam, prev, hist, tp):
    """A whole temporal-adaptive frame from full-frame range renders, as adaptive_ref.emulate builds an adaptive one; the
    context's camera must be `cam`.  Returns a dict: accum, moments (this frame's sums), beauty_out, moments_out,
    history_out (srtTemporalAccumulate of them), counts (tiles per launch), pixel_samples, has (the accepted mask) and
    open0 (the tiles open after round 0)."""
    H, W = p.imageHeight, p.imageWidth
    sched = A.schedule(p.spp, spp_max)
    accum, moments, _ = ctx.render_image_moments(p, want_rgba=False)
    n = p.spp
    active = np.ones((-(-H // A.TILE), -(-W // A.TILE)), bool)
    counts = [int(active.sum())]
    pixel_samples = H * W * p.spp
    open0 = None
    for b in sched[1:]:
        active &= A.tile_open(A.converged(pooled_moments(accum, moments, planes, cam, prev, hist, tp), thr))
        if open0 is None:
            open0 = active.copy()
        if not active.any():
            break
        q = copy.copy(p)
        q.spp, q.sampleFirst = b, p.sampleFirst + n
        q.sppChunks = min(p.sppChunks, b) if p.sppChunks > 0 else 0
        a2, m2, _ = ctx.render_image_moments(q, want_rgba=False)
        mask = A.pixel_mask(active, H, W)
        accum[mask] = accum[mask] + a2[mask]
        moments[mask] = moments[mask] + m2[mask]
        n += b
        counts.append(int(active.sum()))
        pixel_samples += int(mask.sum()) * b
    info = {}
    out_b, out_m, new = R.accumulate(accum, moments, planes[1], planes[2], planes[3], planes[0] if tp["demodulate"] else None, cam,
                                     prev, hist, tp["normal_cos"], tp["plane_dist"], tp["max_history"], bool(tp["demodulate"]),
                                     info=info)
    return dict(accum=accum, moments=moments, beauty_out=out_b, moments_out=out_m, history_out=new, counts=counts,
                pixel_samples=pixel_samples, has=info["has"], open0=open0)
