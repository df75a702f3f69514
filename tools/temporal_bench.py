"""Temporal accumulation, measured in one process.  Prints one JSON line.
  timing   srtTemporalAccumulate (masterchief, a 1.5 degree orbit step, default parameters, with and without demodulation)
           at 720p and 1080p with events over --steps launches after a warm-up, next to srtDenoiseMoments and srtDenoise on the
           same frame in the same run
  sweep    the three defaults: final-frame display MSE of an 8-frame 426x240 4-spp orbit (temporal + denoise) against a
           1024-spp render of the last camera, over normalCos x planeDist x maxHistory, masterchief and spheres, and the MSE
           restricted to the silhouette band (pixels within 2 px of a hit/miss or depth edge), where ghosting shows
  quality  final-frame display MSE and consecutive-frame difference (static camera), single-frame vs temporal, 4 / 8 / 16
           spp, masterchief, spheres and iron
usage: python tools/temporal_bench.py [--steps 20] [--warmup 3] [--no-sweep] [--no-quality]"""
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
SCENES = {"masterchief": srt.scenes.scene_masterchief, "spheres": srt.scenes.scene_spheres, "iron": srt.scenes.scene_iron}


def orbit_camera(degrees):
    c = abi.default_camera_params()
    a = np.deg2rad(np.float64(degrees))
    dx, dz = np.float32(c.eye[0] - c.lookAt[0]), np.float32(c.eye[2] - c.lookAt[2])
    co, si = np.float32(np.cos(a)), np.float32(np.sin(a))
    c.eye[0] = np.float32(c.lookAt[0]) + (co * dx + si * dz)
    c.eye[2] = np.float32(c.lookAt[2]) + (co * dz - si * dx)
    return dev.make_camera(c)


def device_frame(ctx, p):
    W, H = p.imageWidth, p.imageHeight
    nloc = dev.num_local_tiles(W, H, 1)
    tiles = [torch.zeros((nloc, 64, 4), dtype=torch.float32, device="cuda") for _ in range(6)]
    ctx.render_tiles_moments(p, tiles[0].data_ptr(), tiles[1].data_ptr(), None)
    ctx.render_feature_tiles(p, abi.SRT_FEATURE_ALL, [t.data_ptr() for t in tiles[2:]], None)
    img = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(6)]
    for k in range(6):
        ctx.resolve_tiles(p, tiles[k].data_ptr(), None, img[k].data_ptr(), None)
    torch.cuda.synchronize()
    return img[0], img[1], img[2:]


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


def timing(ctx, height, steps, warmup):
    W, H = int(height * 16 / 9), height
    ctx.upload_scene(SCENES["masterchief"]())
    cams = [orbit_camera(0.0), orbit_camera(1.5)]
    frames = []
    for k, cam in enumerate(cams):
        ctx.set_camera(cam)
        frames.append(device_frame(ctx, abi.default_render_params(W, H, 4, 4, seed=1, spp_chunks=0, sample_first=4 * k)))
    out = {"width": W, "height": H}
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
    hist = [torch.zeros((3, H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    for dm in (0, 1):
        t = abi.default_temporal_params(demodulate=dm)
        for k, (b, m, pl) in enumerate(frames):
            ptrs = [q.data_ptr() for q in pl] if dm else [None] + [q.data_ptr() for q in pl[1:]]
            args = (t, W, H, b.data_ptr(), m.data_ptr(), ptrs, cams[k], cams[0] if k else None, hist[0].data_ptr() if k else None,
                    bufs[0].data_ptr(), bufs[1].data_ptr(), hist[k].data_ptr(), None)
            ctx.temporal_accumulate(*args)
        out["temporal_ms_dm%d" % dm] = timed(lambda: ctx.temporal_accumulate(*args), steps, warmup)
        out["temporal_same_camera_ms_dm%d" % dm] = timed(
            lambda: ctx.temporal_accumulate(t, W, H, b.data_ptr(), m.data_ptr(), ptrs, cams[1], cams[1], hist[0].data_ptr(),
                                            bufs[0].data_ptr(), bufs[1].data_ptr(), hist[1].data_ptr(), None), steps, warmup)
    b, m, pl = frames[1]
    planes = [pl[0].data_ptr(), pl[1].data_ptr(), None, pl[3].data_ptr()]
    d = abi.default_denoise_params(demodulate=1)
    out["denoise_ms"] = timed(lambda: ctx.denoise(d, W, H, b.data_ptr(), planes, bufs[2].data_ptr(), None, None), steps, warmup)
    out["denoise_moments_ms"] = timed(lambda: ctx.denoise(d, W, H, bufs[0].data_ptr(), planes, bufs[2].data_ptr(), None, None,
                                                          d_moments_ptr=bufs[1].data_ptr()), steps, warmup)
    pix = W * H
    # bytes the kernel must move per pixel: beauty, moments, three planes (+ albedo), one history record in, two outputs and
    # the history out; bilinear taps re-read neighbours' records out of the caches
    out["min_bytes_per_pixel"] = 16 * (2 + 3) + 48 + 16 * 2 + 48
    out["temporal_gbs_dm0"] = out["min_bytes_per_pixel"] * pix / out["temporal_ms_dm0"] / 1e6
    return out


def display(mean):
    return np.sqrt(np.clip(np.nan_to_num(mean[..., :3], nan=0.0, posinf=1.0), 0.0, 1.0))


def orbit_run(ctx, W, H, spp, frames, step, t, seed=11):
    d = abi.default_denoise_params()
    ctx.temporal_reset()
    for k in range(frames):
        ctx.set_camera(orbit_camera(k * step))
        p = abi.default_render_params(W, H, spp, 4, seed=seed, spp_chunks=0, sample_first=k * spp)
        _, den, _, st = ctx.render_temporal_frame(p, d, t)
    single = ctx.render_denoised_moments(p, d)[2]
    return den, single, st


def edge_band(ctx, W, H):
    """Pixels within 2 px of a hit/miss boundary or a relative depth step of more than 10 %, for the camera currently set."""
    f = ctx.render_features(abi.default_render_params(W, H, 16, 4, seed=5), abi.SRT_FEATURE_DEPTH)["depth"]
    z = np.where(f[..., 3] > 0, f[..., 0], np.inf)
    e = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        for ax in (0, 1):
            a, b = np.moveaxis(z, ax, 0)[:-1], np.moveaxis(z, ax, 0)[1:]
            step = (np.isinf(a) != np.isinf(b)) | (np.abs(a - b) > 0.1 * np.minimum(a, b))
            m = np.zeros_like(np.moveaxis(e, ax, 0))
            m[:-1] |= step
            m[1:] |= step
            e |= np.moveaxis(m, 0, ax)
    for _ in range(2):
        g = e.copy()
        g[1:] |= e[:-1]; g[:-1] |= e[1:]; g[:, 1:] |= e[:, :-1]; g[:, :-1] |= e[:, 1:]
        e = g
    return e


def sweep(ctx):
    W, H, spp, frames, step = 426, 240, 4, 8, 1.5
    rows = []
    for name in ("masterchief", "spheres"):
        ctx.upload_scene(SCENES[name]())
        ctx.set_camera(orbit_camera((frames - 1) * step))
        ref, _ = ctx.render_image(abi.default_render_params(W, H, 1024, 4, seed=99, spp_chunks=0), want_rgba=False)
        truth = display(ref[..., :3] / ref[..., 3:4])
        band = edge_band(ctx, W, H)
        grid = [(nc, pd, 64.0) for nc in (0.5, 0.8, 0.9, 0.97) for pd in (0.005, 0.02, 0.08)]
        grid += [(0.9, 0.02, mh) for mh in (8.0, 16.0, 32.0, 128.0, float("inf"))]
        for nc, pd, mh in grid:
            den, single, st = orbit_run(ctx, W, H, spp, frames, step, abi.default_temporal_params(nc, pd, mh))
            err, err1 = (display(den) - truth) ** 2, (display(single) - truth) ** 2
            rows.append({"scene": name, "normalCos": nc, "planeDist": pd, "maxHistory": mh, "mse": float(err.mean()),
                         "mse_single": float(err1.mean()), "mse_band": float(err[band].mean()),
                         "mse_band_single": float(err1[band].mean()), "band_share": float(band.mean()),
                         "history_share": st["historyPixels"] / (W * H), "mean_history": st["meanHistoryCount"]})
    ctx.temporal_reset()
    return rows


def quality(ctx):
    W, H, frames, step = 426, 240, 8, 1.5
    rows = []
    for name in ("masterchief", "spheres", "iron"):
        ctx.upload_scene(SCENES[name]())
        ctx.set_camera(orbit_camera((frames - 1) * step))
        ref, _ = ctx.render_image(abi.default_render_params(W, H, 1024, 4, seed=99, spp_chunks=0), want_rgba=False)
        truth = display(ref[..., :3] / ref[..., 3:4])
        for spp in (4, 8, 16):
            t, d = abi.default_temporal_params(), abi.default_denoise_params()
            den, single, st = orbit_run(ctx, W, H, spp, frames, step, t)
            ctx.temporal_reset()
            outs_t, outs_s = [], []
            for k in range(6):
                p = abi.default_render_params(W, H, spp, 4, seed=12, spp_chunks=0, sample_first=k * spp)
                outs_t.append(display(ctx.render_temporal_frame(p, d, t)[1]))
                outs_s.append(display(ctx.render_denoised_moments(p, d)[2]))
            rows.append({"scene": name, "spp": spp, "mse_temporal": float(((display(den) - truth) ** 2).mean()),
                         "mse_single": float(((display(single) - truth) ** 2).mean()),
                         "flicker_temporal": float(np.mean([np.abs(a - b).mean() for a, b in zip(outs_t[1:], outs_t[2:])])),
                         "flicker_single": float(np.mean([np.abs(a - b).mean() for a, b in zip(outs_s[1:], outs_s[2:])])),
                         "history_share": st["historyPixels"] / (W * H)})
    ctx.temporal_reset()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    a = ap.parse_args()
    ctx = dev.Context(0)
    out = {"device": ctx.device_info(), "steps": a.steps,
           "timing": [timing(ctx, h, a.steps, a.warmup) for h in (720, 1080)]}
    if not a.no_sweep:
        out["sweep"] = sweep(ctx)
    if not a.no_quality:
        out["quality"] = quality(ctx)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
