"""Temporal history across a refit, measured in one process.  Prints one JSON line.

The masterchief model turns by --degrees per frame about the vertical axis (examples/main.cpp --spin: every triangle as
loaded, turned by k * degrees on the host, srtUpdateTriangles + srtRefitScene), the camera stands still, 1280 x 720, frame k
draws samples [k * spp, (k + 1) * spp).  For 4, 8 and 16 spp, three forms of the same --frames frames:
  single    every frame rendered and denoised on its own (srtRenderDenoisedImageMoments): what a refit forces without
            motion tracking, and what the commit before motion tracking does
  tracked   srtSetMotionTracking on, srtRenderTemporalFrame after every update + refit: the history follows the model
  static    the bound: srtRenderTemporalFrame of the model standing still (no update, no refit), same samples
Against a --truth-spp render of each frame's geometry, in display space (sqrt of the clamped mean):
  mse       of the last frame
  flicker   mean |e_k - e_(k-1)| over the last half of the frames, e_k = the frame's display-space error image: how much of
            the frame-to-frame change is not the truth's own
and the share of pixels that accepted history in the last frame.
  timing    the motion pass (srtRenderMotionTiles) next to the feature pass (srtRenderFeatureTiles, four planes) and the
            render (srtRenderTilesMoments) of the same frame, events over --steps launches after a warm-up; and
            srtTemporalAccumulateMotion next to srtTemporalAccumulate on the same buffers

usage: python tools/motion_bench.py [--frames 8] [--degrees 3] [--truth-spp 512] [--steps 20] [--warmup 3] [--height 720]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

srt = importlib.import_module("sexy-raytracer_amd")
abi, dev = srt.abi, srt.device()
F = np.float32


def turned(tri, degrees):
    a = np.deg2rad(np.float64(degrees))
    c, s = F(np.cos(a)), F(np.sin(a))
    out = tri.copy()
    x, z = tri["p"][..., 0], tri["p"][..., 2]
    out["p"][..., 0] = c * x + s * z
    out["p"][..., 2] = c * z - s * x
    return out


def display(mean):
    return np.sqrt(np.clip(np.nan_to_num(mean[..., :3], nan=0.0, posinf=1.0), 0.0, 1.0))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def truths(ctx, tri, W, H, frames, degrees, spp):
    out = []
    for k in range(frames):
        ctx.update_triangles(0, turned(tri, k * degrees))
        ctx.refit()
        ref, _ = ctx.render_image(abi.default_render_params(W, H, spp, 4, seed=99, spp_chunks=0), want_rgba=False)
        out.append(display(ref[..., :3] / ref[..., 3:4]))
    return out


def sequence(ctx, tri, W, H, frames, degrees, spp, form):
    """The denoised display images of the frames, and the last frame's stats (None for `single`)."""
    d, t = abi.default_denoise_params(), abi.default_temporal_params()
    ctx.update_triangles(0, tri)
    ctx.refit()
    ctx.temporal_reset()
    outs, st = [], None
    for k in range(frames):
        if form != "static" and k:
            ctx.update_triangles(0, turned(tri, k * degrees))
            ctx.refit()
        p = abi.default_render_params(W, H, spp, 4, seed=11, spp_chunks=0, sample_first=k * spp)
        if form == "single":
            den = ctx.render_denoised_moments(p, d)[2]
        else:
            _, den, _, st = ctx.render_temporal_frame(p, d, t)
        outs.append(display(den))
    return outs, st


def quality(ctx, sb, W, H, frames, degrees, truth_spp):
    tri = np.concatenate(sb.triangles)
    truth = truths(ctx, tri, W, H, frames, degrees, truth_spp)
    rows = []
    for spp in (4, 8, 16):
        row = {"spp": spp}
        for form in ("single", "tracked", "static"):
            ctx.set_motion_tracking(form == "tracked")
            outs, st = sequence(ctx, tri, W, H, frames, degrees, spp, form)
            ref = [truth[0]] * frames if form == "static" else truth
            err = [o - r for o, r in zip(outs, ref)]
            half = max(1, frames // 2)
            row["mse_" + form] = float((err[-1] ** 2).mean())
            row["flicker_" + form] = float(np.mean([np.abs(a - b).mean() for a, b in zip(err[half:], err[half - 1:-1])]))
            if st is not None:
                row["history_share_" + form] = st["historyPixels"] / (W * H)
                row["mean_history_" + form] = st["meanHistoryCount"]
        rows.append(row)
    ctx.set_motion_tracking(False)
    return rows


def timing(ctx, sb, W, H, degrees, steps, warmup):
    tri = np.concatenate(sb.triangles)
    ctx.set_motion_tracking(True)
    ctx.update_triangles(0, tri)
    ctx.refit()
    nloc = dev.num_local_tiles(W, H, 1)
    tiles = [torch.zeros((nloc, 64, 4), dtype=torch.float32, device="cuda") for _ in range(7)]
    img = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(9)]
    hist = [torch.zeros((3, H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    cam = dev.make_camera(abi.default_camera_params())
    t = abi.default_temporal_params()
    rows = []
    for spp in (4, 8, 16):
        p0 = abi.default_render_params(W, H, spp, 4, seed=1, spp_chunks=0)
        ctx.update_triangles(0, tri)
        ctx.refit()
        ctx.render_tiles_moments(p0, tiles[0].data_ptr(), tiles[1].data_ptr(), None)
        ctx.render_feature_tiles(p0, abi.SRT_FEATURE_ALL, [q.data_ptr() for q in tiles[2:6]], None)
        for k in range(6):
            ctx.resolve_tiles(p0, tiles[k].data_ptr(), None, img[k].data_ptr(), None)
        planes = [None] + [q.data_ptr() for q in img[3:6]]
        ctx.temporal_accumulate(t, W, H, img[0].data_ptr(), img[1].data_ptr(), planes, cam, None, None, img[7].data_ptr(),
                                img[8].data_ptr(), hist[0].data_ptr(), None)
        ctx.update_triangles(0, turned(tri, degrees))
        ctx.refit()
        p = abi.default_render_params(W, H, spp, 4, seed=1, spp_chunks=0, sample_first=spp)
        row = {"spp": spp,
               "render_ms": timed(lambda: ctx.render_tiles_moments(p, tiles[0].data_ptr(), tiles[1].data_ptr(), None), steps, warmup),
               "features_ms": timed(lambda: ctx.render_feature_tiles(p, abi.SRT_FEATURE_ALL, [q.data_ptr() for q in tiles[2:6]], None),
                                    steps, warmup),
               "motion_ms": timed(lambda: ctx.render_motion_tiles(p, tiles[6].data_ptr(), None), steps, warmup)}
        for k in range(7):
            ctx.resolve_tiles(p, tiles[k].data_ptr(), None, img[k].data_ptr(), None)
        for name, motion in (("accumulate_ms", None), ("accumulate_motion_ms", img[6].data_ptr())):
            row[name] = timed(lambda: ctx.temporal_accumulate(t, W, H, img[0].data_ptr(), img[1].data_ptr(), planes, cam, cam,
                                                              hist[0].data_ptr(), img[7].data_ptr(), img[8].data_ptr(),
                                                              hist[1].data_ptr(), None, motion_ptr=motion), steps, warmup)
        rows.append(row)
    ctx.set_motion_tracking(False)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--degrees", type=float, default=3.0)
    ap.add_argument("--truth-spp", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=720)
    a = ap.parse_args()
    W, H = int(a.height * 16 / 9), a.height
    ctx = dev.Context(0)
    sb = srt.scenes.scene_masterchief()
    ctx.upload_scene(sb)
    ctx.set_camera(dev.make_camera(abi.default_camera_params()))
    out = {"device": ctx.device_info(), "width": W, "height": H, "frames": a.frames, "degrees": a.degrees, "truth_spp": a.truth_spp,
           "steps": a.steps, "timing": timing(ctx, sb, W, H, a.degrees, a.steps, a.warmup),
           "quality": quality(ctx, sb, W, H, a.frames, a.degrees, a.truth_spp)}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
