"""What tile-adaptive sampling (srtRenderAdaptive) buys, one process, 720p: for each scene and a few thresholds the pixel
samples, the render kernel time of every round, the wall time of the whole call, the time between the rounds' render
kernels (the accumulate / decide / compact / resolve kernels, the count read-back and the launch gaps), and the display-space
RMSE against a 4096-spp uniform frame; next to it a uniform sweep (kernel time and RMSE per spp) and, interpolated in it
(RMSE ~ spp^-1/2 between neighbours, time linear), the uniform render of equal RMSE and its time.  Device events, one
warm-up, the median of --reps runs.  Prints one JSON line.

usage: python tools/adaptive_bench.py [--scenes masterchief,spheres,iron] [--spp0 16] [--max-spp 1024] [--reps 3] [--out FILE]"""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

srt = importlib.import_module("sexy-raytracer_amd")
abi, dev = srt.abi, srt.device()

SCENES = {"masterchief": srt.scenes.scene_masterchief, "spheres": srt.scenes.scene_spheres, "iron": srt.scenes.scene_iron}
THRESHOLDS = (2.0 / 256, 1.0 / 256, 0.5 / 256)  # display-space standard error: 2, 1 and 1/2 display steps


def rmse(accum, ref):
    img = accum[..., :3] / accum[..., 3:4]
    m = np.isfinite(img).all(-1) & np.isfinite(ref).all(-1)
    return float(np.sqrt(np.mean((np.sqrt(np.maximum(img[m], 0)) - np.sqrt(np.maximum(ref[m], 0))) ** 2)))


def uniform_point(ctx, W, H, spp, ref, reps):
    p = abi.default_render_params(W, H, spp, 4, seed=1, spp_chunks=0)
    acc, _ = ctx.render_image(p)  # warm-up, and the image
    ms = []
    for _ in range(reps):
        ctx.render_image(p, want_accum=False, want_rgba=False)
        ms.append(ctx.last_kernel_ms())
    return {"spp": spp, "kernel_ms": round(float(np.median(ms)), 3), "rmse": round(rmse(acc, ref), 6)}


def adaptive_point(ctx, W, H, spp0, spp_max, thr, ref, reps):
    p = abi.default_render_params(W, H, spp0, 4, seed=1, spp_chunks=0)
    ap = abi.default_adaptive_params(spp_max, thr)
    acc, mom, rgba = (torch.zeros((H, W, 4), dtype=d, device="cuda") for d in (torch.float32, torch.float32, torch.uint8))
    run = lambda: ctx.render_adaptive_device(p, ap, acc.data_ptr(), mom.data_ptr(), rgba.data_ptr(), None)  # noqa: E731
    run()  # warm-up
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    walls, stats = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        a.record()
        st = run()
        b.record()
        torch.cuda.synchronize()
        walls.append(a.elapsed_time(b))
        stats.append(st)
    k = int(np.argsort(walls)[len(walls) // 2])
    st, wall = stats[k], walls[k]
    render = float(sum(st["roundMs"]))
    return {"threshold": thr, "threshold_steps": thr * 256, "rounds": st["rounds"], "round_spp": st["roundSpp"],
            "round_tiles": st["roundTiles"], "round_ms": [round(x, 3) for x in st["roundMs"]],
            "pixel_samples": st["pixelSamples"], "mean_spp": round(st["pixelSamples"] / (W * H), 2),
            "wall_ms": round(wall, 3), "render_ms": round(render, 3),
            "between_rounds_ms_per_round": round((wall - render) / st["rounds"], 4),
            "rmse": round(rmse(acc.cpu().numpy(), ref), 6)}


def equal_rmse_uniform(sweep, target):
    """spp and kernel time of the uniform render whose RMSE equals `target`, interpolated between the sweep's neighbours
    (log RMSE linear in log spp; time linear in spp); None outside the sweep."""
    for lo, hi in zip(sweep, sweep[1:]):
        if hi["rmse"] <= target <= lo["rmse"]:
            t = math.log(lo["rmse"] / target) / math.log(lo["rmse"] / hi["rmse"]) if lo["rmse"] != hi["rmse"] else 0.0
            spp = math.exp(math.log(lo["spp"]) + t * (math.log(hi["spp"]) - math.log(lo["spp"])))
            ms = lo["kernel_ms"] + (spp - lo["spp"]) / (hi["spp"] - lo["spp"]) * (hi["kernel_ms"] - lo["kernel_ms"])
            return {"spp": round(spp, 1), "kernel_ms": round(ms, 3)}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="masterchief,spheres,iron")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp0", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    W, H = args.width, args.height
    ctx = dev.Context(0)
    rec = {"tool": "adaptive_bench", "width": W, "height": H, "spp0": args.spp0, "max_spp": args.max_spp, "ref_spp": args.ref_spp,
           "device": ctx.device_info()["name"], "scenes": {}}
    for name in args.scenes.split(","):
        ctx.upload_scene(SCENES[name]())
        ctx.set_camera(dev.make_camera(abi.default_camera_params()))
        ref, _ = ctx.render_image(abi.default_render_params(W, H, args.ref_spp, 4, seed=99, spp_chunks=0), want_rgba=False)
        ref = ref[..., :3] / ref[..., 3:4]
        sweep = []
        spp = args.spp0
        while spp <= args.max_spp:
            sweep.append(uniform_point(ctx, W, H, spp, ref, args.reps))
            print(name, sweep[-1], file=sys.stderr, flush=True)
            spp *= 2
        points = []
        for thr in THRESHOLDS:
            pt = adaptive_point(ctx, W, H, args.spp0, args.max_spp, thr, ref, args.reps)
            pt["uniform_equal_rmse"] = equal_rmse_uniform(sweep, pt["rmse"])
            if pt["uniform_equal_rmse"]:
                pt["speedup_vs_equal_rmse_uniform"] = round(pt["uniform_equal_rmse"]["kernel_ms"] / pt["wall_ms"], 3)
            points.append(pt)
            print(name, pt, file=sys.stderr, flush=True)
        rec["scenes"][name] = {"uniform": sweep, "adaptive": points}
    ctx.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
