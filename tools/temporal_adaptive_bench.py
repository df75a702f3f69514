"""Temporal-adaptive frames (srtRenderTemporalAdaptiveFrame), measured in one process.  Prints one JSON line.
  timing   at 720p and 1080p (masterchief, a 1.5 degree orbit step): srtTemporalReproject next to srtTemporalAccumulate and
           srtDenoiseMoments with events over --steps launches after a warm-up, and the wall time of a whole
           temporal-adaptive frame (spp 4, sppMax 32) against the uniform temporal frame of ceil(its mean samples) samples,
           the median of 5 frames of a running orbit
  quality  DESIGN.md 5.9's protocol: an 8-frame orbit at 1.5 degrees per frame, 426x240, final-frame display-space MSE and
           band MSE (pixels within 2 px of a hit/miss or depth edge) against a 1024-spp render of the last camera; the
           adaptive run at spp 4 over sppMax x threshold against the uniform srtRenderTemporalFrame run with
           spp = ceil(the adaptive run's mean samples per pixel per frame), masterchief, spheres and iron
  --frames-only HEIGHT  nothing but 30 temporal-adaptive frames at that height, for a kernel trace
           (rocprofv3 --kernel-trace --stats -- python tools/temporal_adaptive_bench.py --frames-only 720): the per-round
           srt_temporal_adaptive_update_kernel is launched by the frame only
usage: python tools/temporal_adaptive_bench.py [--steps 30] [--warmup 3] [--no-timing] [--no-quality]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from temporal_bench import SCENES, abi, dev, device_frame, display, edge_band, orbit_camera, timed, torch  # noqa: E402

STEP = 1.5


def adaptive_orbit(ctx, W, H, spp, spp_max, thr, frames, seed=11):
    d, t = abi.default_denoise_params(), abi.default_temporal_params()
    ap = abi.default_adaptive_params(spp_max, thr)
    ctx.temporal_reset()
    samples, per_frame = 0, []
    for k in range(frames):
        ctx.set_camera(orbit_camera(k * STEP))
        p = abi.default_render_params(W, H, spp, 4, seed=seed, spp_chunks=0, sample_first=k * spp_max)
        _, den, _, st = ctx.render_temporal_adaptive_frame(p, ap, d, t)
        samples += st["pixelSamples"]
        per_frame.append(st["pixelSamples"] / (W * H))
    return den, samples / (frames * W * H), per_frame, st


def uniform_orbit(ctx, W, H, spp, frames, seed=11):
    d, t = abi.default_denoise_params(), abi.default_temporal_params()
    ctx.temporal_reset()
    for k in range(frames):
        ctx.set_camera(orbit_camera(k * STEP))
        p = abi.default_render_params(W, H, spp, 4, seed=seed, spp_chunks=0, sample_first=k * spp)
        _, den, _, _ = ctx.render_temporal_frame(p, d, t)
    return den


def quality(ctx):
    W, H, spp, frames = 426, 240, 4, 8
    rows = []
    for name in ("masterchief", "spheres", "iron"):
        ctx.upload_scene(SCENES[name]())
        ctx.set_camera(orbit_camera((frames - 1) * STEP))
        ref, _ = ctx.render_image(abi.default_render_params(W, H, 1024, 4, seed=99, spp_chunks=0), want_rgba=False)
        truth = display(ref[..., :3] / ref[..., 3:4])
        band = edge_band(ctx, W, H)
        uniform = {}
        for spp_max in (16, 32, 64):
            for thr in (0.01, 0.02, 0.03, 0.05, 0.08):
                den, mean_spp, per_frame, st = adaptive_orbit(ctx, W, H, spp, spp_max, thr, frames)
                u = math.ceil(mean_spp)
                if u not in uniform:
                    e = (display(uniform_orbit(ctx, W, H, u, frames)) - truth) ** 2
                    uniform[u] = (float(e.mean()), float(e[band].mean()))
                e = (display(den) - truth) ** 2
                rows.append({"scene": name, "sppMax": spp_max, "threshold": thr, "mean_spp": mean_spp, "spp_per_frame": per_frame,
                             "last_frame_tiles": st["roundTiles"], "mse": float(e.mean()), "mse_band": float(e[band].mean()),
                             "uniform_spp": u, "mse_uniform": uniform[u][0], "mse_band_uniform": uniform[u][1],
                             "band_share": float(band.mean())})
    ctx.temporal_reset()
    return rows


def timing(ctx, height, steps, warmup):
    W, H = int(height * 16 / 9), height
    ctx.upload_scene(SCENES["masterchief"]())
    cams = [orbit_camera(0.0), orbit_camera(STEP)]
    frames = []
    for k, cam in enumerate(cams):
        ctx.set_camera(cam)
        frames.append(device_frame(ctx, abi.default_render_params(W, H, 4, 4, seed=1, spp_chunks=0, sample_first=4 * k)))
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
    hist = [torch.zeros((3, H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    rp = torch.zeros((2, H, W, 4), dtype=torch.float32, device="cuda")
    t = abi.default_temporal_params()
    b, m, pl = frames[0]
    ptrs = [None] + [q.data_ptr() for q in pl[1:]]
    ctx.temporal_accumulate(t, W, H, b.data_ptr(), m.data_ptr(), ptrs, cams[0], None, None, bufs[0].data_ptr(), bufs[1].data_ptr(),
                            hist[0].data_ptr(), None)
    b, m, pl = frames[1]
    ptrs = [None] + [q.data_ptr() for q in pl[1:]]
    out = {"width": W, "height": H}
    out["reproject_ms"] = timed(lambda: ctx.temporal_reproject(t, W, H, ptrs, cams[1], cams[0], hist[0].data_ptr(), rp.data_ptr(), None),
                                steps, warmup)
    out["reproject_same_camera_ms"] = timed(
        lambda: ctx.temporal_reproject(t, W, H, ptrs, cams[1], cams[1], hist[0].data_ptr(), rp.data_ptr(), None), steps, warmup)
    out["temporal_ms"] = timed(lambda: ctx.temporal_accumulate(t, W, H, b.data_ptr(), m.data_ptr(), ptrs, cams[1], cams[0],
                                                               hist[0].data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(),
                                                               hist[1].data_ptr(), None), steps, warmup)
    d = abi.default_denoise_params()
    planes = [None, pl[1].data_ptr(), None, pl[3].data_ptr()]
    out["denoise_moments_ms"] = timed(lambda: ctx.denoise(d, W, H, bufs[0].data_ptr(), planes, bufs[2].data_ptr(), None, None,
                                                          d_moments_ptr=bufs[1].data_ptr()), steps, warmup)
    # whole frames, host to host: a running orbit, the median of the frames after the first three
    spp, spp_max, thr, n = 4, 32, 0.03, 8
    ap = abi.default_adaptive_params(spp_max, thr)
    ctx.temporal_reset()
    wall, samples, rounds = [], [], []
    for k in range(n):
        ctx.set_camera(orbit_camera(k * STEP))
        p = abi.default_render_params(W, H, spp, 4, seed=11, spp_chunks=0, sample_first=k * spp_max)
        t0 = time.perf_counter()
        st = ctx.render_temporal_adaptive_frame(p, ap, d, t)[3]
        wall.append(1e3 * (time.perf_counter() - t0))
        samples.append(st["pixelSamples"] / (W * H))
        rounds.append({"tiles": st["roundTiles"], "render_ms": st["roundMs"]})
    u = math.ceil(float(np.mean(samples[3:])))
    ctx.temporal_reset()
    wall_u = []
    for k in range(n):
        ctx.set_camera(orbit_camera(k * STEP))
        p = abi.default_render_params(W, H, u, 4, seed=11, spp_chunks=0, sample_first=k * u)
        t0 = time.perf_counter()
        ctx.render_temporal_frame(p, d, t)
        wall_u.append(1e3 * (time.perf_counter() - t0))
    ctx.temporal_reset()
    out.update(frame_spp=spp, frame_spp_max=spp_max, frame_threshold=thr, adaptive_frame_wall_ms=float(np.median(wall[3:])),
               adaptive_mean_spp=float(np.mean(samples[3:])), uniform_spp=u, uniform_frame_wall_ms=float(np.median(wall_u[3:])),
               last_frame_rounds=rounds[-1])
    return out


def frames_only(ctx, height):
    W, H = int(height * 16 / 9), height
    ctx.upload_scene(SCENES["masterchief"]())
    ap = abi.default_adaptive_params(32, 0.03)
    for k in range(30):
        ctx.set_camera(orbit_camera(k * STEP))
        ctx.render_temporal_adaptive_frame(abi.default_render_params(W, H, 4, 4, seed=11, spp_chunks=0, sample_first=k * 32), ap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--frames-only", type=int, default=0)
    a = ap.parse_args()
    ctx = dev.Context(0)
    if a.frames_only:
        frames_only(ctx, a.frames_only)
        ctx.close()
        return
    out = {"device": ctx.device_info(), "steps": a.steps}
    if not a.no_timing:
        out["timing"] = [timing(ctx, h, a.steps, a.warmup) for h in (720, 1080)]
    if not a.no_quality:
        out["quality"] = quality(ctx)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
