"""Device ray queries (srtTraceRaysDevice, srtOccludedDevice): Mrays/s on ray sets that never leave the GPU.

Ray sets, per scene:
  primary  the 720p lens-centre primary rays of the default camera, one per pixel, tMax = inf
  ao       ambient-occlusion rays built with torch ops on the device from the feature pass's planes: from the POSITION
           mean of every pixel that hit something, pushed off the surface along the NORMAL mean, --ao-rays cosine-
           distributed directions about that normal, tMax = --ao-radius times the scene's extent
Scenes: masterchief (the reference's tree) and bench.py's soups of 200 k and 1 M triangles with PLOC trees.
Per scene and ray set: FAITHFUL (reference tree only), CLOSEST and ANY (occlusion), timed with events on a stream around
the calls (mean of --steps back-to-back calls after --warmup), and beside them `host_trace_ms`: srtTraceRays on the same rays copied to the
host, wall clock.  NOTE that the latter includes what the host entry does on every call -- two device allocations, 36 B
per ray in, 88 B per ray out, a device synchronisation -- and its kernel keeps traversal counters: it is the cost of asking
through the only entry there was, not a kernel comparison.
--ao-png FILE writes the AO image 1 - mean(occluded) of the first scene.  Prints one JSON line.

--path-loop measures the device path steps instead (path_loop below): pathloop.render fused and unfused against
srtRenderTiles on masterchief (reference tree FAITHFUL, PLOC tree CLOSEST) and soup_200k (PLOC, CLOSEST), 4 and 16 spp,
4 bounces, with the active share of the entries per bounce; the same two loops with the live set compacted between bounces
(compact=True) alternate with them, and `compact_call` is one srtCompactPathsDevice call behind the first bounce of the
whole batch (rays, states and slots moved), timed with events like the queries above.  `whole` is the same frame through
srtTracePathsDevice (whole=True: one kernel per batch) as the library ships it -- a wave claims entries once a quarter of it
is idle (tunable paths_refill_min 16) -- and `whole_refill1` with a refill on every trip; `peak_mb` is torch's peak
allocation over one frame of `whole` and of the compacted fused loop.  --sort-bits 3,5,7,9 adds the fused loop with
srtSortPathsDevice in the place of the compaction (pathloop.render(sort=b)) at each of those cell sizes, as variants that
alternate with the others; --variants NAMES keeps the listed variants only (the yardstick of a sorted loop is
fused_compact measured in the same session).

--sort-ao measures the AO set again with srtSortPathsDevice in front of srtOccludedDevice: `any` on the rays as they are,
on rays sorted once outside the clock (`sorted_b`), and the sort together with the query (`sort_and_any_b`, the box from
the origins included), per cell size of --sort-bits; the variants alternate, --warmup-loops + --loop-reps rounds of
--steps back-to-back calls, median and spread of the rounds.
--sort-call SPP times --steps srtSortPathsDevice calls behind the first bounce of all W * H * SPP camera rays at the
first cell size of --sort-bits (run it under a kernel trace for the split into key, sort and gather).

--direct measures direct light sampling (direct_bench below): plain and direct whole paths at 4 to 256 spp against a
5000-spp srtRenderImage, RMSE and frame time, and the equal-error time ratio.

usage: python tools/query_bench.py --direct [--cases masterchief,iron,spheres] [--loop-reps 3] [--ref-spp 5000] [--clamp X]
       python tools/query_bench.py [--steps 200] [--warmup 5] [--host-steps 3] [--cases masterchief,soup_200k,soup_1m] [--ao-rays 4]
                                   [--ao-radius 0.1] [--ao-png FILE] [--width 1280] [--height 720]
       python tools/query_bench.py --path-loop [--loop-reps 5] [--warmup-loops 1] [--cases masterchief,soup_200k,soup_1m]
                                   [--sort-bits 3,5,7,9] [--variants fused_compact,fused_sort_3,...]
       python tools/query_bench.py --sort-ao [--sort-bits 3,5,7,9] [--steps 20] [--loop-reps 5] [--cases ...]
       python tools/query_bench.py --sort-call 16 [--sort-bits 5] [--steps 5] [--cases soup_200k]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

srt = importlib.import_module("sexy-raytracer_amd")
abi, dev = srt.abi, srt.device()
F = np.float32


def scene(case):
    if case.startswith("soup_"):
        n = {"200k": 200000, "1m": 1000000, "4m": 4000000}[case[5:]]
        # bench.py's soups
        return srt.scenes.scene_soup(n, seed=7, extent=6.0, size=max(0.01, 0.08 * (100000.0 / n) ** (1.0 / 3.0)), builder=abi.SRT_BUILDER_PLOC)
    return srt.scenes.SCENES[case]()


def primary_rays(cam, W, H):
    """(W*H, 9) float32 on the GPU: camera.h:40-46 with a zero lens offset, pixel centres, time 0.5 of the shutter."""
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    u = ((xs + 0.5) / (W - 1)).reshape(-1, 1)
    v = ((H - ys - 0.5) / (H - 1)).reshape(-1, 1)
    o, ll, hz, vt = (torch.tensor(list(a), device="cuda", dtype=torch.float32) for a in (cam.origin, cam.lleft, cam.horizontal, cam.vertical))
    rays = torch.empty((W * H, 9), device="cuda", dtype=torch.float32)
    rays[:, 0:3] = o
    rays[:, 3:6] = ll + u * hz + v * vt - o
    rays[:, 6] = 0.5 * (cam.time0 + cam.time1)
    rays[:, 7] = 0.001
    rays[:, 8] = float("inf")
    return rays


def ao_rays(planes, count, radius, time, seed=1):
    """Cosine-distributed directions about the NORMAL mean from the POSITION mean of every pixel with a hit, torch ops on the
    device.  Returns (rays (pixels * count, 9), pixel index of every ray's pixel)."""
    pos = torch.from_numpy(planes["position"].reshape(-1, 4)).cuda()
    nrm = torch.from_numpy(planes["normal"].reshape(-1, 4)).cuda()
    pix = torch.nonzero(nrm[:, 3] > 0).reshape(-1)
    n = torch.nn.functional.normalize(nrm[pix, :3], dim=1)
    p = pos[pix, :3]
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    # a unit vector uniform on the sphere added to the unit normal: cosine-distributed about it
    s = torch.nn.functional.normalize(torch.randn((len(pix), count, 3), device="cuda", generator=g), dim=2)
    d = torch.nn.functional.normalize(n[:, None, :] + 0.999 * s, dim=2)
    rays = torch.empty((len(pix), count, 9), device="cuda", dtype=torch.float32)
    rays[:, :, 0:3] = (p + 5e-3 * radius * n)[:, None, :]
    rays[:, :, 3:6] = d
    rays[:, :, 6] = time
    rays[:, :, 7] = 5e-3 * radius
    rays[:, :, 8] = radius
    return rays.reshape(-1, 9).contiguous(), pix


def event_ms(stream, fn, steps, warmup):
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        for _ in range(steps):
            fn()
        stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def measure(ctx, rays, faithful, steps, warmup, host_steps):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    n = rays.shape[0]
    out = {"rays": n}
    modes = [("closest", lambda: ctx.trace_device(rays, abi.SRT_TRAVERSE_CLOSEST, stream=stream)),
             ("any", lambda: ctx.occluded_device(rays, stream=stream))]
    if faithful:
        modes.insert(0, ("faithful", lambda: ctx.trace_device(rays, abi.SRT_TRAVERSE_FAITHFUL, stream=stream)))
    for name, fn in modes:
        ms = event_ms(stream, fn, steps, warmup)
        out[name + "_ms"] = ms
        out[name + "_mrays_s"] = n / ms * 1e-3
    with torch.cuda.stream(stream):
        hits = ctx.trace_device(rays, abi.SRT_TRAVERSE_CLOSEST, stream=stream)
        occ = ctx.occluded_device(rays, stream=stream)
    stream.synchronize()
    out["hit_share"] = float((hits[:, 0] >= 0).float().mean())
    assert bool(((hits[:, 0] >= 0) == (occ != 0)).all()), "occlusion disagrees with the closest hit"
    # the host entry on the same rays: allocation, both transfers and a device synchronisation are inside the clock
    host = rays.cpu().numpy().view(abi.RAY_DTYPE).reshape(-1)
    ctx.trace(host[:1024], abi.SRT_TRAVERSE_CLOSEST)
    t = time.perf_counter()
    for _ in range(host_steps):
        ctx.trace(host, abi.SRT_TRAVERSE_CLOSEST)
    out["host_trace_ms"] = (time.perf_counter() - t) * 1e3 / host_steps
    out["host_trace_mrays_s"] = n / out["host_trace_ms"] * 1e-3
    return out, occ


def compact_call(ctx, p, traversal, steps, warmup):
    """One srtCompactPathsDevice call at the batch size of the frame: behind the first bounce of all W * H * spp camera
    rays, moving rays, states and slots into buffers allocated once."""
    rays, rng = ctx.camera_rays_device(p)
    out, _ = ctx.path_step_device(rays, rng, traversal, rays_out=rays)
    n = rays.shape[0]
    rays_out, rng_out = torch.empty_like(rays), torch.empty_like(rng)
    slot_out = torch.empty((n,), dtype=torch.int32, device="cuda")
    count = torch.empty((1,), dtype=torch.int64, device="cuda")
    scratch = torch.empty((ctx.compact_scratch_bytes(n),), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    ms = event_ms(stream, lambda: ctx.compact_paths_device(out=out, rays=rays, rng=rng, rays_out=rays_out, rng_out=rng_out, slot_out=slot_out,
                                                           count=count, scratch=scratch, stream=stream), steps, warmup)
    return {"n": n, "kept_share": int(count) / float(n), "ms": ms, "steps": steps}


def median_and_spread(v):
    return {"ms": float(np.median(v)), "spread_ms": [min(v), max(v)]}


def sort_bits(a):
    return [int(b) for b in a.sort_bits.split(",") if b]


def sort_ao(a):
    """--sort-ao: srtOccludedDevice on the AO set of every case as it is, on the set sorted once outside the clock, and with
    the sort (and the box from the origins) inside it."""
    ctx = dev.Context(0)
    cam = dev.make_camera(abi.default_camera_params())
    W, H = a.width, a.height
    result = {"device": ctx.device_info()["name"], "width": W, "height": H, "ao_rays_per_pixel": a.ao_rays, "steps": a.steps,
              "reps": a.loop_reps, "note": "ms per call: median and (min, max) over the alternating rounds of `steps` calls", "cases": {}}
    stream = torch.cuda.Stream()
    for case in a.cases.split(","):
        sb = scene(case)
        ctx.upload_scene(sb)
        ctx.set_camera(cam)
        faithful = all(it.builder == abi.SRT_BUILDER_REFERENCE for it in sb.world)
        p = abi.default_render_params(W, H, 1, 1, seed=1, traversal=abi.SRT_TRAVERSE_FAITHFUL if faithful else abi.SRT_TRAVERSE_CLOSEST)
        planes = ctx.render_features(p, abi.SRT_FEATURE_NORMAL | abi.SRT_FEATURE_POSITION)
        rays, _ = ao_rays(planes, a.ao_rays, a.ao_radius * 6.0, 0.5 * (cam.time0 + cam.time1))
        n = rays.shape[0]
        scratch = torch.empty((ctx.sort_scratch_bytes(n),), dtype=torch.uint8, device="cuda")
        rays_out, slot_out = torch.empty_like(rays), torch.empty((n,), dtype=torch.int32, device="cuda")
        count = torch.empty((1,), dtype=torch.int64, device="cuda")
        want = ctx.occluded_device(rays)
        variants = {"any": lambda: ctx.occluded_device(rays, stream=stream)}
        torch.cuda.synchronize()
        for b in sort_bits(a):
            ordered, _, slot, _, _ = ctx.sort_paths_device(b, rays=rays, scratch=scratch)
            back = torch.empty_like(want)
            back.index_copy_(0, slot.to(torch.int64), ctx.occluded_device(ordered))
            assert torch.equal(back, want), "occlusion of the sorted rays, scattered back, differs"
            variants["sorted_%d" % b] = lambda ordered=ordered: ctx.occluded_device(ordered, stream=stream)

            def both(b=b):
                ctx.sort_paths_device(b, rays=rays, rays_out=rays_out, slot_out=slot_out, count=count, scratch=scratch, stream=stream)
                ctx.occluded_device(rays_out, stream=stream)
            variants["sort_and_any_%d" % b] = both
        torch.cuda.synchronize()
        stream.wait_stream(torch.cuda.current_stream())
        ms = {k: [] for k in variants}
        for round_ in range(a.warmup_loops + a.loop_reps):
            for name, fn in variants.items():
                t = event_ms(stream, fn, a.steps, 1)
                if round_ >= a.warmup_loops:
                    ms[name].append(t)
        out = {"rays": n, "bvh_depth": ctx.bvh_depth(), "occluded_share": float((want != 0).float().mean())}
        for name, v in ms.items():
            out[name] = dict(median_and_spread(v), mrays_s=n / float(np.median(v)) * 1e-3)
        result["cases"][case] = out
    ctx.close()
    print(json.dumps(result))


def sort_call(a):
    """--sort-call SPP: srtSortPathsDevice behind the first bounce of all W * H * SPP camera rays of the first case, --steps
    times at the first cell size, rays, states and slots moved into buffers allocated once, the box made once."""
    ctx = dev.Context(0)
    ctx.upload_scene(scene(a.cases.split(",")[0]))
    ctx.set_camera(dev.make_camera(abi.default_camera_params()))
    bits = sort_bits(a)[0]
    p = abi.default_render_params(a.width, a.height, a.sort_call, 4, seed=1, traversal=abi.SRT_TRAVERSE_CLOSEST)
    rays, rng = ctx.camera_rays_device(p)
    out, _ = ctx.path_step_device(rays, rng, abi.SRT_TRAVERSE_CLOSEST, rays_out=rays)
    n = rays.shape[0]
    box = ctx.origin_box(rays, out)
    rays_out, rng_out = torch.empty_like(rays), torch.empty_like(rng)
    slot_out = torch.empty((n,), dtype=torch.int32, device="cuda")
    count = torch.empty((1,), dtype=torch.int64, device="cuda")
    scratch = torch.empty((ctx.sort_scratch_bytes(n),), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    ms = event_ms(stream, lambda: ctx.sort_paths_device(bits, rays=rays, out=out, box=box, rng=rng, rays_out=rays_out, rng_out=rng_out,
                                                        slot_out=slot_out, count=count, scratch=scratch, stream=stream), a.steps, 1)
    compact_scratch = torch.empty((ctx.compact_scratch_bytes(n),), dtype=torch.uint8, device="cuda")
    compact_ms = event_ms(stream, lambda: ctx.compact_paths_device(out=out, rays=rays, rng=rng, rays_out=rays_out, rng_out=rng_out,
                                                                   slot_out=slot_out, count=count, scratch=compact_scratch, stream=stream),
                          a.steps, 1)
    print(json.dumps({"device": ctx.device_info()["name"], "case": a.cases.split(",")[0], "n": n, "cell_bits": bits,
                      "kept_share": int(count) / float(n), "steps": a.steps, "sort_ms": ms, "compact_ms": compact_ms,
                      "scratch_mb": ctx.sort_scratch_bytes(n) / 2.0 ** 20}))
    ctx.close()


def path_loop(a):
    """--path-loop: the user-land path tracer (pathloop.render over srtCameraRaysDevice + srtPathStepDevice, fused, and
    over srtTraceRaysDevice(records) + srtScatterRaysDevice, unfused) against srtRenderTiles of the same samples.
    Events around whole loops after a warm-up; these three and the two loops with compaction between bounces alternate
    within one session, --loop-reps times, and every figure is the median with the spread (min, max) beside it."""
    pathloop = importlib.import_module("sexy-raytracer_amd.pathloop")
    ctx = dev.Context(0)
    cam = dev.make_camera(abi.default_camera_params())
    W, H, bounces = a.width, a.height, 4
    result = {"device": ctx.device_info()["name"], "width": W, "height": H, "max_bounce": bounces, "reps": a.loop_reps,
              "note": "msamples_s = W * H * spp / median ms; spread = (min ms, max ms) over the alternating repetitions", "cases": {}}
    cases = [("masterchief_reference_faithful", "masterchief", None, abi.SRT_TRAVERSE_FAITHFUL),
             ("masterchief_ploc_closest", "masterchief", abi.SRT_BUILDER_PLOC, abi.SRT_TRAVERSE_CLOSEST),
             ("soup_200k_ploc_closest", "soup_200k", None, abi.SRT_TRAVERSE_CLOSEST),
             ("soup_1m_ploc_closest", "soup_1m", None, abi.SRT_TRAVERSE_CLOSEST)]
    stream = torch.cuda.current_stream()
    refill_default = ctx.get_tunable("paths_refill_min")
    for label, case, builder, traversal in cases:
        if case not in a.cases.split(","):
            continue
        if (case == "soup_1m" and not sort_bits(a)) or (label == "masterchief_reference_faithful" and sort_bits(a)):
            continue  # the sorted loops: masterchief's PLOC tree with CLOSEST steps, and soup_1m as well
        sb = scene(case)
        if builder is not None:
            for it in sb.world:
                if it.kind == abi.SRT_WORLD_BVH:
                    it.builder = builder
        ctx.upload_scene(sb)
        ctx.set_camera(cam)
        tiles = torch.empty((dev.lib.srtNumLocalTiles(W, H, 1) * 64, 4), dtype=torch.float32, device="cuda")
        out = {"bvh_depth": ctx.bvh_depth()}
        for spp in (4, 16):
            p = abi.default_render_params(W, H, spp, bounces, seed=1, traversal=traversal)

            def whole(refill_min):
                ctx.set_tunable("paths_refill_min", refill_min)
                return pathloop.render(ctx, p, traversal=traversal, whole=True)

            variants = {"fused": lambda: pathloop.render(ctx, p, fused=True, traversal=traversal),
                        "unfused": lambda: pathloop.render(ctx, p, fused=False, traversal=traversal),
                        "fused_compact": lambda: pathloop.render(ctx, p, fused=True, traversal=traversal, compact=True),
                        "unfused_compact": lambda: pathloop.render(ctx, p, fused=False, traversal=traversal, compact=True),
                        "whole": lambda: whole(refill_default),
                        "whole_refill1": lambda: whole(1),
                        "render_tiles": lambda: ctx.render_tiles(p, tiles.data_ptr(), stream.cuda_stream)}
            for b in sort_bits(a):
                variants["fused_sort_%d" % b] = lambda b=b: pathloop.render(ctx, p, fused=True, traversal=traversal, sort=b)
            if a.variants:
                variants = {k: v for k, v in variants.items() if k in a.variants.split(",")}
            ms = {k: [] for k in variants}
            for rep in range(a.warmup_loops + a.loop_reps):
                for name, fn in variants.items():
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record(stream)
                    fn()
                    stop.record(stream)
                    stop.synchronize()
                    if rep >= a.warmup_loops:
                        ms[name].append(start.elapsed_time(stop))
            counts = []
            pathloop.render(ctx, p, fused=True, traversal=traversal, active_counts=counts)
            torch.cuda.synchronize()
            entry = {"active_share_per_bounce": [int(c) / float(W * H * spp) for c in counts]}
            for name, v in ms.items():
                med = float(np.median(v))
                entry[name] = {"ms": med, "spread_ms": [min(v), max(v)], "msamples_s": W * H * spp / med * 1e-3}
            entry["compact_call"] = compact_call(ctx, p, traversal, a.steps, a.warmup)
            entry["peak_mb"] = {}
            for name in [k for k in ("whole", "fused_compact", "fused_sort_5") if k in variants]:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                variants[name]()
                torch.cuda.synchronize()
                entry["peak_mb"][name] = (torch.cuda.max_memory_allocated() - before) / 2.0 ** 20
            out["spp_%d" % spp] = entry
        result["cases"][label] = out
    ctx.set_tunable("paths_refill_min", refill_default)
    ctx.close()
    print(json.dumps(result))


def direct_bench(a):
    """--direct: what direct light sampling buys in samples and costs in time.  Per case (--cases, default
    masterchief,iron,spheres) at --width x --height, 4 bounces, FAITHFUL: the reference is srtRenderImage at --ref-spp (5000);
    plain whole paths (pathloop.render(whole=True)) and direct ones (direct=True) at 4, 16, 64 and 256 spp, each --loop-reps
    times alternating, events around the whole frame, --direct-batch sample indices per batch for both; RMSE of the mean
    radiance against the reference over the pixels finite in all three (--clamp X clamps the radiance first; default: no
    clamp).  equal_error: for each direct point, the plain frame time that
    reaches the same RMSE -- interpolated, or extrapolated along the last segment, on plain's (log time, log RMSE) points --
    over the direct frame time: above 1 direct sampling pays.  The reference's own noise is a floor under both."""
    pathloop = importlib.import_module("sexy-raytracer_amd.pathloop")
    ctx = dev.Context(0)
    cam = dev.make_camera(abi.default_camera_params())
    W, H, bounces = a.width, a.height, 4
    stream = torch.cuda.current_stream()
    result = {"device": ctx.device_info()["name"], "width": W, "height": H, "max_bounce": bounces, "ref_spp": a.ref_spp, "clamp": a.clamp if np.isfinite(a.clamp) else None,
              "reps": a.loop_reps, "batch": a.direct_batch, "cases": {}}
    for case in a.cases.split(","):
        ctx.upload_scene(scene(case))
        ctx.set_camera(cam)
        ref_acc, _ = ctx.render_image(abi.default_render_params(W, H, a.ref_spp, bounces, seed=99), want_rgba=False)
        ref = np.minimum(ref_acc[..., :3] / ref_acc[..., 3:4], F(a.clamp)).astype(np.float64)
        out = {"sampled_lights": int(len(ctx.sampled_lights())), "points": {}}
        for spp in (4, 16, 64, 256):
            p = abi.default_render_params(W, H, spp, bounces, seed=1)
            ms, image = {"plain": [], "direct": []}, {}
            for rep in range(1 + a.loop_reps):
                for name in ("plain", "direct"):
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record(stream)
                    img = pathloop.render(ctx, p, whole=True, direct=(name == "direct"), samples_per_batch=a.direct_batch)
                    stop.record(stream)
                    stop.synchronize()
                    if rep:
                        ms[name].append(start.elapsed_time(stop))
                    image[name] = img
            means = {k: np.minimum((v[..., :3] / v[..., 3:4]).cpu().numpy(), F(a.clamp)).astype(np.float64) for k, v in image.items()}
            ok = np.isfinite(ref).all(axis=-1) & np.isfinite(means["plain"]).all(axis=-1) & np.isfinite(means["direct"]).all(axis=-1)
            point = {"finite_share": float(ok.mean())}
            for name in ("plain", "direct"):
                point[name] = {"ms": float(np.median(ms[name])), "spread_ms": [min(ms[name]), max(ms[name])],
                               "rmse": float(np.sqrt(((means[name][ok] - ref[ok]) ** 2).mean()))}
            out["points"]["spp_%d" % spp] = point
        pts = [out["points"]["spp_%d" % s] for s in (4, 16, 64, 256)]
        lt = np.log([q["plain"]["ms"] for q in pts])
        le = np.log([q["plain"]["rmse"] for q in pts])
        out["equal_error"] = {}
        for s, q in zip((4, 16, 64, 256), pts):
            e = np.log(q["direct"]["rmse"])
            k = int(np.clip(np.searchsorted(-le, -e) - 1, 0, len(le) - 2))  # le falls with time
            t = lt[k] + (e - le[k]) * (lt[k + 1] - lt[k]) / (le[k + 1] - le[k])
            out["equal_error"]["spp_%d" % s] = {"plain_ms_for_direct_rmse": float(np.exp(t)), "time_ratio": float(np.exp(t) / q["direct"]["ms"]),
                                                "extrapolated": bool(e < le[-1] or e > le[0])}
        result["cases"][case] = out
    ctx.close()
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path-loop", action="store_true", help="measure pathloop.render (fused / unfused) against srtRenderTiles instead")
    ap.add_argument("--direct", action="store_true", help="direct light sampling against plain whole paths: RMSE and frame time (direct_bench)")
    ap.add_argument("--ref-spp", type=int, default=5000, help="--direct: samples of the srtRenderImage reference")
    ap.add_argument("--clamp", type=float, default=float("inf"), help="--direct: radiance is clamped to this before the RMSE (default: not at all)")
    ap.add_argument("--direct-batch", type=int, default=4, help="--direct: sample indices per batch of both estimators")
    ap.add_argument("--loop-reps", type=int, default=5, help="--path-loop: timed repetitions of every variant, alternating")
    ap.add_argument("--warmup-loops", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed device calls per figure (a call is 0.2 - 3 ms)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3, help="timed srtTraceRays calls (10 - 70 ms each)")
    ap.add_argument("--sort-bits", default="", help="cell bits per axis of the sorted variants, e.g. 3,5,7,9")
    ap.add_argument("--variants", default="", help="--path-loop: only these variants")
    ap.add_argument("--sort-ao", action="store_true", help="srtOccludedDevice on the AO set, sorted and unsorted")
    ap.add_argument("--sort-call", type=int, default=0, metavar="SPP", help="srtSortPathsDevice calls behind the first bounce of W * H * SPP rays")
    ap.add_argument("--cases", default="masterchief,soup_200k,soup_1m")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--ao-rays", type=int, default=4)
    ap.add_argument("--ao-radius", type=float, default=0.1, help="AO tMax as a share of the scene's extent (6 units)")
    ap.add_argument("--ao-png", default=None)
    a = ap.parse_args()
    if a.direct:
        if a.cases == ap.get_default("cases"):
            a.cases = "masterchief,iron,spheres"
        return direct_bench(a)
    if a.path_loop:
        return path_loop(a)
    if a.sort_ao:
        return sort_ao(a)
    if a.sort_call:
        return sort_call(a)
    ctx = dev.Context(0)
    cam = dev.make_camera(abi.default_camera_params())
    W, H = a.width, a.height
    result = {"device": ctx.device_info()["name"], "steps": a.steps, "host_steps": a.host_steps, "width": W, "height": H, "ao_rays_per_pixel": a.ao_rays,
              "note": "host_trace_* is srtTraceRays end to end on the same rays: it includes allocation and transfers", "cases": {}}
    for k, case in enumerate(a.cases.split(",")):
        sb = scene(case)
        ctx.upload_scene(sb)
        ctx.set_camera(cam)
        faithful = all(it.builder == abi.SRT_BUILDER_REFERENCE for it in sb.world)
        out = {"tree": "reference" if faithful else "ploc", "bvh_depth": ctx.bvh_depth()}
        out["primary"], _ = measure(ctx, primary_rays(cam, W, H), faithful, a.steps, a.warmup, a.host_steps)
        p = abi.default_render_params(W, H, 1, 1, seed=1, traversal=abi.SRT_TRAVERSE_FAITHFUL if faithful else abi.SRT_TRAVERSE_CLOSEST)
        planes = ctx.render_features(p, abi.SRT_FEATURE_NORMAL | abi.SRT_FEATURE_POSITION)
        rays, pix = ao_rays(planes, a.ao_rays, a.ao_radius * 6.0, 0.5 * (cam.time0 + cam.time1))
        out["ao"], occ = measure(ctx, rays, faithful, a.steps, a.warmup, a.host_steps)
        out["ao"]["occluded_share"] = float((occ != 0).float().mean())
        if a.ao_png and k == 0:
            from PIL import Image
            img = torch.ones(W * H, device="cuda")
            img[pix] = 1.0 - (occ != 0).float().reshape(-1, a.ao_rays).mean(dim=1)
            Image.fromarray((img.reshape(H, W).clamp(0, 1) * 255).byte().cpu().numpy(), "L").save(a.ao_png)
        result["cases"][case] = out
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
