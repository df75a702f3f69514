"""What the sample moments cost, one process: the plain render (srtRenderTiles) against the moments render
(srtRenderTilesMoments) by srtLastKernelMs, on masterchief 720p at 64 spp and on the 5000-spp headline frame, and
srtDenoiseMoments against srtDenoise (720p, 64 spp, demodulation on) with events over --steps launches.  With --quality
also the denoised / noisy display MSE of both variances (320x180, 16 spp against 1024 spp) for a few sigmaL values.
Prints one JSON line.

usage: python tools/moments_bench.py [--steps 20] [--warmup 3] [--headline-spp 5000] [--quality] [--out FILE]"""
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


def render_ms(ctx, p, moments, reps):
    """median srtLastKernelMs of `reps` launches after one warm-up, alternating nothing: one variant per call"""
    nloc = dev.num_local_tiles(p.imageWidth, p.imageHeight, 1)
    acc = torch.zeros((nloc, 64, 4), dtype=torch.float32, device="cuda")
    mom = torch.zeros_like(acc)
    go = (lambda: ctx.render_tiles_moments(p, acc.data_ptr(), mom.data_ptr(), None)) if moments else \
        (lambda: ctx.render_tiles(p, acc.data_ptr(), None))
    go()
    ms = []
    for _ in range(reps):
        go()
        ms.append(ctx.last_kernel_ms())
    return float(np.median(ms)), ctx.launch_info()


def quality(ctx, scene, sigmas, W=320, H=180, spp=16, ref_spp=1024):
    ctx.upload_scene(scene)
    ctx.set_camera(dev.make_camera(abi.default_camera_params()))
    ref, _ = ctx.render_image(abi.default_render_params(W, H, ref_spp, 4, seed=99, spp_chunks=0))
    ref = ref[..., :3] / ref[..., 3:4]
    p = abi.default_render_params(W, H, spp, 4, seed=1, spp_chunks=0)
    out = {}
    for dm in (0, 1):
        for s in sigmas:
            d = abi.default_denoise_params(demodulate=dm, sigma_luminance=s)
            accum, spatial, _ = ctx.render_denoised(p, d)
            _, _, sample, _ = ctx.render_denoised_moments(p, d)
            noisy = accum[..., :3] / accum[..., 3:4]
            m = np.isfinite(noisy).all(-1) & np.isfinite(ref).all(-1)
            mse = lambda x: float(np.mean((np.sqrt(np.maximum(x[m], 0)) - np.sqrt(np.maximum(ref[m], 0))) ** 2))  # noqa: E731
            out["dm%d_sigmaL%g" % (dm, s)] = {"spatial": round(mse(spatial[..., :3]) / mse(noisy), 4),
                                              "sample_variance": round(mse(sample[..., :3]) / mse(noisy), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--headline-spp", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    ctx = dev.Context(0)
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(dev.make_camera(abi.default_camera_params()))
    W, H = 1280, 720
    rec = {"tool": "moments_bench", "scene": "masterchief", "width": W, "height": H, "device": ctx.device_info()["name"]}
    for spp, reps in ((64, args.reps), (args.headline_spp, max(2, args.reps // 2))):
        p = abi.default_render_params(W, H, spp, 4, seed=1, spp_chunks=0)
        plain, info = render_ms(ctx, p, False, reps)
        mom, info_m = render_ms(ctx, p, True, reps)
        plain2, _ = render_ms(ctx, p, False, reps)  # plain again: drift between the two variants shows here
        rec["render_%dspp" % spp] = {"plain_ms": round(plain, 3), "moments_ms": round(mom, 3), "plain_again_ms": round(plain2, 3),
                                     "cost": round(mom / min(plain, plain2) - 1.0, 4), "form": info["lds_tree_mode"],
                                     "same_launch": info == info_m}
    # the denoiser on the 64-spp frame
    p = abi.default_render_params(W, H, 64, 4, seed=1, spp_chunks=0)
    nloc = dev.num_local_tiles(W, H, 1)
    tiles = [torch.zeros((nloc, 64, 4), dtype=torch.float32, device="cuda") for _ in range(5)]
    img = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(5)]
    ctx.render_tiles_moments(p, tiles[0].data_ptr(), tiles[4].data_ptr(), None)
    ctx.render_feature_tiles(p, abi.SRT_FEATURE_ALBEDO | abi.SRT_FEATURE_NORMAL | abi.SRT_FEATURE_DEPTH,
                             [tiles[1].data_ptr(), tiles[2].data_ptr(), None, tiles[3].data_ptr()], None)
    for k in range(5):
        ctx.resolve_tiles(p, tiles[k].data_ptr(), None, img[k].data_ptr(), None)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    ptrs = [img[1].data_ptr(), img[2].data_ptr(), None, img[3].data_ptr()]
    d = abi.default_denoise_params(demodulate=1)
    plain = timed(lambda: ctx.denoise(d, W, H, img[0].data_ptr(), ptrs, out.data_ptr(), None, None), args.steps, args.warmup)
    mom = timed(lambda: ctx.denoise(d, W, H, img[0].data_ptr(), ptrs, out.data_ptr(), None, None, d_moments_ptr=img[4].data_ptr()),
                args.steps, args.warmup)
    rec["denoise_ms"] = round(plain, 4)
    rec["denoise_moments_ms"] = round(mom, 4)
    if args.quality:
        rec["quality_320x180_16spp_vs_1024spp"] = {
            name: quality(ctx, fn(), (2.0, 4.0, 8.0)) for name, fn in
            (("spheres", srt.scenes.scene_spheres), ("iron", srt.scenes.scene_iron), ("masterchief", srt.scenes.scene_masterchief))}
    ctx.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
