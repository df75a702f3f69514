"""Guide planes from every adaptive sample (srtRenderFeatureTileList and the guided entries), measured in one process.
Prints one JSON line.
  timing   at 720p and 1080p on masterchief (spp 4, sppMax 32, thr 0.03): per round of a guided adaptive render, the list
           pass over that round's tiles and sample range (events over --steps launches after a warm-up; the list is rebuilt
           from the final counts in row-major order) beside the round's render launch (SrtAdaptiveStats.roundMs); the wall
           time of the guided against the unguided adaptive render, and of guided against unguided temporal-adaptive frames
           (the median of the frames after the first three of a running orbit), alternating in the same run
  quality  DESIGN.md 5.10's protocol unchanged: an 8-frame orbit at 1.5 degrees per frame, 426x240, spp 4, final-frame
           display-space MSE and band MSE against a 1024-spp render of the last camera, sppMax x threshold, masterchief,
           spheres and iron; guided against unguided against the uniform temporal frame of ceil(mean samples) samples
  single   one frame, 426x240: srtRenderAdaptiveDenoisedImage (spp 4, sppMax x threshold) against
           srtRenderDenoisedImageMoments at ceil(its mean samples per pixel) samples, same error measures
usage: python tools/adaptive_guides_bench.py [--steps 20] [--warmup 3] [--no-timing] [--no-quality] [--no-single]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from temporal_bench import SCENES, abi, dev, display, edge_band, orbit_camera, timed, torch  # noqa: E402
from temporal_adaptive_bench import STEP, uniform_orbit  # noqa: E402

GRID = [(spp_max, thr) for spp_max in (16, 32, 64) for thr in (0.01, 0.02, 0.03, 0.05, 0.08)]


def adaptive_orbit(ctx, W, H, spp, spp_max, thr, frames, guided, seed=11):
    d, t = abi.default_denoise_params(), abi.default_temporal_params()
    ap = abi.default_adaptive_params(spp_max, thr)
    ctx.temporal_reset()
    samples, wall = 0, []
    for k in range(frames):
        ctx.set_camera(orbit_camera(k * STEP))
        p = abi.default_render_params(W, H, spp, 4, seed=seed, spp_chunks=0, sample_first=k * spp_max)
        t0 = time.perf_counter()
        _, den, _, st = ctx.render_temporal_adaptive_frame(p, ap, d, t, guided=guided)
        wall.append(1e3 * (time.perf_counter() - t0))
        samples += st["pixelSamples"]
    return den, samples / (frames * W * H), wall, st


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
        for spp_max, thr in GRID:
            row = {"scene": name, "sppMax": spp_max, "threshold": thr, "band_share": float(band.mean())}
            for guided in (False, True):
                den, mean_spp, _, st = adaptive_orbit(ctx, W, H, spp, spp_max, thr, frames, guided)
                e = (display(den) - truth) ** 2
                tag = "guided" if guided else "unguided"
                row.update({"mean_spp_" + tag: mean_spp, "mse_" + tag: float(e.mean()), "mse_band_" + tag: float(e[band].mean()),
                            "last_frame_tiles_" + tag: st["roundTiles"]})
            u = math.ceil(max(row["mean_spp_guided"], row["mean_spp_unguided"]))
            if u not in uniform:
                e = (display(uniform_orbit(ctx, W, H, u, frames)) - truth) ** 2
                uniform[u] = (float(e.mean()), float(e[band].mean()))
            row.update(uniform_spp=u, mse_uniform=uniform[u][0], mse_band_uniform=uniform[u][1])
            rows.append(row)
    ctx.temporal_reset()
    return rows


def single(ctx):
    W, H, spp = 426, 240, 4
    rows = []
    d = abi.default_denoise_params()
    for name in ("masterchief", "spheres", "iron"):
        ctx.upload_scene(SCENES[name]())
        ctx.set_camera(orbit_camera(0.0))
        ref, _ = ctx.render_image(abi.default_render_params(W, H, 1024, 4, seed=99, spp_chunks=0), want_rgba=False)
        truth = display(ref[..., :3] / ref[..., 3:4])
        band = edge_band(ctx, W, H)
        uniform = {}
        for spp_max, thr in GRID:
            p = abi.default_render_params(W, H, spp, 4, seed=11, spp_chunks=0)
            _, _, den, _, st = ctx.render_adaptive_denoised(p, abi.default_adaptive_params(spp_max, thr), d)
            mean_spp = st["pixelSamples"] / (W * H)
            u = math.ceil(mean_spp)
            if u not in uniform:
                den_u = ctx.render_denoised_moments(abi.default_render_params(W, H, u, 4, seed=11, spp_chunks=0), d)[2]
                e = (display(den_u) - truth) ** 2
                uniform[u] = (float(e.mean()), float(e[band].mean()))
            e = (display(den) - truth) ** 2
            rows.append({"scene": name, "sppMax": spp_max, "threshold": thr, "mean_spp": mean_spp, "tiles": st["roundTiles"],
                         "mse": float(e.mean()), "mse_band": float(e[band].mean()), "uniform_spp": u, "mse_uniform": uniform[u][0],
                         "mse_band_uniform": uniform[u][1]})
    return rows


def timing(ctx, height, steps, warmup):
    W, H = int(height * 16 / 9), height
    spp, spp_max, thr = 4, 32, 0.03
    ctx.upload_scene(SCENES["masterchief"]())
    ctx.set_camera(orbit_camera(0.0))
    p = abi.default_render_params(W, H, spp, 4, seed=11, spp_chunks=0)
    ap = abi.default_adaptive_params(spp_max, thr)
    acc, mom = (torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    planes = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    ptrs = [q.data_ptr() for q in planes]
    out = {"width": W, "height": H, "spp": spp, "sppMax": spp_max, "threshold": thr}
    wall = {"guided": [], "unguided": []}
    for _ in range(2 + 5):  # alternating; the first two of each are warm-up
        t0 = time.perf_counter()
        st = ctx.render_adaptive_guided_device(p, ap, abi.SRT_FEATURE_ALL, ptrs, acc.data_ptr(), mom.data_ptr(), None, None)
        wall["guided"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        ctx.render_adaptive_device(p, ap, acc.data_ptr(), mom.data_ptr(), None, None)
        wall["unguided"].append(1e3 * (time.perf_counter() - t0))
    out.update(adaptive_guided_wall_ms=float(np.median(wall["guided"][2:])), adaptive_unguided_wall_ms=float(np.median(wall["unguided"][2:])))
    # the list pass of each round, over the tiles that round rendered
    count = acc.cpu().numpy()[..., 3]
    ty, tx = -(-H // 8), -(-W // 8)
    pad = np.zeros((ty * 8, tx * 8), np.float32)
    pad[:H, :W] = count
    tiles = pad.reshape(ty, 8, tx, 8).max(axis=(1, 3))
    rounds, n = [], 0
    for r, b in enumerate(st["roundSpp"]):
        ys, xs = np.nonzero(tiles >= n + b)
        lst = torch.from_numpy((xs.astype(np.uint32) | ys.astype(np.uint32) << 16).view(np.int32)).cuda()
        assert len(xs) == st["roundTiles"][r]
        q = abi.default_render_params(W, H, b, 4, seed=11, spp_chunks=0, sample_first=n)
        ms = timed(lambda: ctx.render_feature_tile_list(q, abi.SRT_FEATURE_ALL, lst.data_ptr(), len(xs), ptrs, r > 0, None), steps, warmup)
        rounds.append({"round": r, "tiles": len(xs), "spp": b, "list_pass_ms": ms, "render_ms": st["roundMs"][r]})
        n += b
    out["rounds"] = rounds
    # whole temporal-adaptive frames, guided and unguided orbits one after the other, twice
    frames = {"guided": [], "unguided": []}
    for _ in range(2):
        for guided in (True, False):
            _, mean_spp, w, _ = adaptive_orbit(ctx, W, H, spp, spp_max, thr, 8, guided)
            frames["guided" if guided else "unguided"].append((float(np.median(w[3:])), mean_spp))
    ctx.temporal_reset()
    out["temporal_frame_wall_ms"] = {k: [v[0] for v in vs] for k, vs in frames.items()}
    out["temporal_frame_mean_spp"] = {k: [v[1] for v in vs] for k, vs in frames.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--no-single", action="store_true")
    a = ap.parse_args()
    ctx = dev.Context(0)
    out = {"device": ctx.device_info(), "steps": a.steps}
    if not a.no_timing:
        out["timing"] = [timing(ctx, h, a.steps, a.warmup) for h in (720, 1080)]
    if not a.no_single:
        out["single_frame"] = single(ctx)
    if not a.no_quality:
        out["quality"] = quality(ctx)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
