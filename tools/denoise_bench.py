"""The denoiser against the frame it cleans, one process: masterchief at 720p, 64 spp.  Times srtDenoise (default parameters,
albedo demodulation on) with events after a warm-up and a synchronise over --steps launches, for every value of the
denoise_lds_step tunable (levels of step <= it staged in LDS: the crossover), plus the 4-bounce beauty render
(srtRenderTiles) and the feature pass (srtRenderFeatureTiles, albedo + normal + depth) of the same frame.  Adds the
kernels' VGPRs / LDS / scratch (compiler resource remarks of csrc/srt_denoise.hip) and the quality figures: denoised over
noisy MSE in display (sqrt) space against a 1024-spp render, 320x180 at 16 spp, for masterchief, spheres and iron.
Prints one JSON line.

usage: python tools/denoise_bench.py [--steps 20] [--warmup 3] [--spp 64] [--height 720] [--no-quality]"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

srt = importlib.import_module("sexy-raytracer_amd")
abi, dev = srt.abi, srt.device()
CSRC = os.path.join(ROOT, "sexy-raytracer_amd", "csrc")


def kernel_resources():
    """VGPRs, scratch and static LDS of the denoiser's kernels, from the compiler's resource remarks (the Makefile's flags)."""
    flags = subprocess.check_output(["make", "-s", "-C", CSRC, "--eval=print-flags:\n\t@echo $(FLAGS) $(KFLAGS)", "print-flags", "ARCH=gfx950"],
                                    text=True).split()
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(CSRC, "srt_denoise.hip")], capture_output=True, text=True).stderr
    names = {"prepare": "prepare", "levelILb1E": "level_lds", "levelILb0E": "level_cache"}
    res, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: _Z\w*srt_denoise_(prepare|levelILb[01]E)", line)
        if m:
            cur = names[m.group(1)]
            res[cur] = {}
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            res[cur][m.group(1).split()[0]] = int(m.group(2))
    return res


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


def frame(ctx, p):
    W, H = p.imageWidth, p.imageHeight
    nloc = dev.num_local_tiles(W, H, 1)
    tiles = [torch.zeros((nloc, 64, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    img = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    planes = abi.SRT_FEATURE_ALBEDO | abi.SRT_FEATURE_NORMAL | abi.SRT_FEATURE_DEPTH
    feat_ptrs = [tiles[1].data_ptr(), tiles[2].data_ptr(), None, tiles[3].data_ptr()]
    render = lambda: ctx.render_tiles(p, tiles[0].data_ptr(), None)  # noqa: E731
    features = lambda: ctx.render_feature_tiles(p, planes, feat_ptrs, None)  # noqa: E731
    render()
    features()
    for k in range(4):
        ctx.resolve_tiles(p, tiles[k].data_ptr(), None, img[k].data_ptr(), None)
    torch.cuda.synchronize()
    return render, features, img[0], [img[1], img[2], None, img[3]]


def quality(ctx, scene, demodulate, W=320, H=180, spp=16, ref_spp=1024):
    ctx.upload_scene(scene)
    ctx.set_camera(dev.make_camera(abi.default_camera_params()))
    accum, den, _ = ctx.render_denoised(abi.default_render_params(W, H, spp, 4, seed=1, spp_chunks=0),
                                        abi.default_denoise_params(demodulate=demodulate))
    ref, _ = ctx.render_image(abi.default_render_params(W, H, ref_spp, 4, seed=99, spp_chunks=0))
    noisy, ref = accum[..., :3] / accum[..., 3:4], ref[..., :3] / ref[..., 3:4]
    m = np.isfinite(noisy).all(-1) & np.isfinite(ref).all(-1)
    mse = lambda x: float(np.mean((np.sqrt(np.maximum(x[m], 0)) - np.sqrt(np.maximum(ref[m], 0))) ** 2))  # noqa: E731
    return {"noisy_mse": mse(noisy), "denoised_mse": mse(den[..., :3]), "ratio": mse(den[..., :3]) / mse(noisy)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    H = args.height
    W = H * 16 // 9
    ctx = dev.Context(0)
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(dev.make_camera(abi.default_camera_params()))
    p = abi.default_render_params(W, H, args.spp, 4, seed=1, spp_chunks=0)
    render, features, beauty, planes = frame(ctx, p)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    ptrs = [t.data_ptr() if t is not None else None for t in planes]
    d = abi.default_denoise_params(demodulate=1)
    den = lambda: ctx.denoise(d, W, H, beauty.data_ptr(), ptrs, out.data_ptr(), rgba.data_ptr(), None)  # noqa: E731
    default_step = ctx.get_tunable("denoise_lds_step")
    by_step = {}
    for s in (0, 1, 2, 4, 8):
        ctx.set_tunable("denoise_lds_step", s)
        by_step[s] = round(timed(den, args.steps, args.warmup), 4)
    ctx.set_tunable("denoise_lds_step", default_step)
    denoise_ms = timed(den, args.steps, args.warmup)
    beauty_ms = timed(render, max(3, args.steps // 10), 1)
    feature_ms = timed(features, max(3, args.steps // 4), 1)
    rec = {"tool": "denoise_bench", "scene": "masterchief", "width": W, "height": H, "spp": args.spp, "iterations": 5,
           "demodulate": 1, "device": ctx.device_info()["name"], "launches": args.steps,
           "denoise_ms": round(denoise_ms, 4), "denoise_lds_step": default_step, "denoise_ms_by_lds_step": by_step,
           "beauty_render_ms": round(beauty_ms, 3), "feature_pass_ms": round(feature_ms, 3),
           "denoise_share_of_frame": round(denoise_ms / (beauty_ms + feature_ms + denoise_ms), 4),
           "kernels": kernel_resources()}
    if not args.no_quality:
        rec["quality_320x180_16spp_vs_1024spp"] = {
            "demodulate%d" % dm: {name: quality(ctx, fn(), dm) for name, fn in
                                  (("masterchief", srt.scenes.scene_masterchief), ("spheres", srt.scenes.scene_spheres),
                                   ("iron", srt.scenes.scene_iron))} for dm in (1, 0)}
    ctx.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
