"""Moving geometry: update + refit against the only other way to move a vertex, srtUploadScene of the moved scene, in one
process.  On soup_200k, soup_1m and soup_4m with PLOC trees and on masterchief with the reference tree, all triangles
turn by a small angle about the vertical axis; timed are
  update_refit_ms       srtUpdateTrianglesDevice (records already on the device) + srtRefitScene, host clock around calls
                        that end synchronised (srtRefitScene returns when its work has finished), mean over --steps
  update_host_refit_ms  the same through srtUpdateTriangles (64 B per triangle cross the bus first)
  upload_ms             srtUploadScene of the moved scene: validation, flattening, host or device tree build, texture and
                        record upload; mean over --upload-steps
and reported beside them the bytes the device path must move (bytes_moved: what its kernels read and write once, from the
scene's counts, below) over update_refit_ms as a share of the 8 TB/s HBM peak.
Tree quality after a refit: on soup_1m every triangle is moved rigidly by a random vector of up to a tenth of the soup's
extent; CLOSEST Msamples/s (720p, 16 spp, srtRenderTiles kernel time) on the refit PLOC tree against a fresh PLOC build of
the moved scene.
Rebuilding (--rebuild-cases, PLOC soups): every triangle is moved rigidly by a random vector, uniform in a ball whose
radius sweeps from a hundredth of the soup's extent to the whole extent (--displacements); per amount, on the same moved scene,
  update_refit_ms / update_rebuild_ms / upload_ms   device records + srtRefitScene, the same + srtRebuildScene, and
                        srtUploadScene of the moved scene, clocked as above
  cost_*                srtGetTreeCost at the upload of the unmoved scene, after the refit, after the rebuild and after the
                        fresh upload (the last two are equal bit for bit)
  msamples_* / frame_ms_*   CLOSEST 720p 16 spp (srtRenderTiles kernel time) on the refitted, the rebuilt and the freshly
                        uploaded tree
and `rebuild_pays_from_cost_ratio`: the smallest cost_refit / cost_at_build of the sweep at which update + rebuild + one
frame takes less than update + refit + one frame (null if at none).  A refitted tree whose frame takes longer than
--frame-budget-ms is rendered once, and not at all for the larger displacements (null; the rebuild pays there a fortiori).
Prints one JSON line.

usage: python tools/refit_bench.py [--steps 10] [--warmup 2] [--upload-steps 2] [--cases soup_200k,soup_1m,soup_4m,masterchief]
                                   [--no-quality] [--rebuild-cases soup_200k,soup_1m,soup_4m]
                                   [--displacements 0.01,0.03,0.1,0.3,1.0] [--rebuild-steps 3]
                                   [--frame-budget-ms 2000]"""
import argparse
import copy
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
HBM_PEAK = 8.0e12
F = np.float32


def scene(case):
    if case.startswith("soup_"):
        n = {"200k": 200000, "1m": 1000000, "4m": 4000000}[case[5:]]
        # bench.py's soups
        return srt.scenes.scene_soup(n, seed=7, extent=6.0, size=max(0.01, 0.08 * (100000.0 / n) ** (1.0 / 3.0)), builder=abi.SRT_BUILDER_PLOC)
    return srt.scenes.SCENES[case]()


def with_triangles(sb, tri):
    out = copy.copy(sb)
    out._keep = None
    out.triangles = [tri]
    return out


def turned(tri, degrees):
    a = np.deg2rad(degrees)
    c, s = F(np.cos(a)), F(np.sin(a))
    out = tri.copy()
    x, z = tri["p"][..., 0], tri["p"][..., 2]
    out["p"][..., 0] = c * x + s * z
    out["p"][..., 2] = c * z - s * x
    return out


def wall(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def bytes_moved(ctx, sb, num_tris):
    """What the update and refit kernels read and write once: per triangle 64 B of input and 112 B of records, then 48 B read
    for its box by the refit and again by the pair records; per node 32 B read + 32 B written by the refit, 4 + 4 B of link and
    counter, 32 B read by the certificate pass (+ 64 B where hybrid records are rewritten), 32 B read + 64 B written by the
    pair records."""
    nodes = sum(len(ctx.bvh(w)) for w, it in enumerate(sb.world) if it.kind == abi.SRT_WORLD_BVH)
    hybrid = ctx.get_tunable("wf_hybrid") > 0 and all(it.builder == abi.SRT_BUILDER_REFERENCE for it in sb.world) and nodes > 4400
    return num_tris * (64 + 112 + 2 * 48) + nodes * (64 + 8 + 32 + (64 if hybrid else 0) + 96), nodes


def case_times(ctx, case, steps, warmup, upload_steps):
    sb = scene(case)
    tri = np.concatenate(sb.triangles)
    moved = turned(tri, 3.0)
    sb_moved = with_triangles(sb, moved)
    ctx.upload_scene(sb)
    d_moved = torch.from_numpy(moved.view(np.uint8).reshape(-1, 64)).cuda()
    d_orig = torch.from_numpy(tri.view(np.uint8).reshape(-1, 64)).cuda()
    flip = [0]

    def device_path():
        flip[0] ^= 1
        ctx.update_triangles(0, d_moved if flip[0] else d_orig)
        ctx.refit()

    def host_path():
        flip[0] ^= 1
        ctx.update_triangles(0, moved if flip[0] else tri)
        ctx.refit()

    out = {"triangles": len(tri)}
    out["update_refit_ms"] = wall(device_path, steps, warmup)
    out["update_host_refit_ms"] = wall(host_path, max(2, steps // 2), 1)
    out["bytes_moved"], out["nodes"] = bytes_moved(ctx, sb, len(tri))
    out["hbm_fraction"] = out["bytes_moved"] / (out["update_refit_ms"] * 1e-3) / HBM_PEAK
    out["upload_ms"] = wall(lambda: ctx.upload_scene(sb_moved), upload_steps, 0)
    out["upload_over_update_refit"] = out["upload_ms"] / out["update_refit_ms"]
    return out


def quality(ctx, W=1280, H=720, spp=16):
    sb = scene("soup_1m")
    tri = np.concatenate(sb.triangles)
    rng = np.random.default_rng(1)
    v = rng.normal(size=(len(tri), 1, 3))
    v *= (rng.random((len(tri), 1, 1)) ** (1 / 3)) * 0.1 * 12.0 / np.linalg.norm(v, axis=-1, keepdims=True)
    moved = tri.copy()
    moved["p"] += v.astype(F)
    cam = dev.make_camera(abi.default_camera_params())
    p = abi.default_render_params(W, H, spp, 4, seed=3, traversal=abi.SRT_TRAVERSE_CLOSEST, spp_chunks=0)
    tiles = torch.zeros((dev.num_local_tiles(W, H, 1), 64, 4), dtype=torch.float32, device="cuda")

    def rate():
        ctx.set_camera(cam)
        ms = []
        for _ in range(4):
            ctx.render_tiles(p, tiles.data_ptr(), None)
            torch.cuda.synchronize()
            ms.append(ctx.last_kernel_ms())
        return W * H * spp / (min(ms[1:]) * 1e3), tiles.clone()

    ctx.upload_scene(sb)
    before, _ = rate()
    ctx.update_triangles(0, moved)
    ctx.refit()
    refit, img_refit = rate()
    ctx.upload_scene(with_triangles(sb, moved))
    fresh, img_fresh = rate()
    return {"displacement": "rigid per triangle, uniform in a ball of radius 1.2 (a tenth of the soup's 12-unit extent)",
            "msamples_unmoved_tree": before, "msamples_refit_tree": refit, "msamples_fresh_ploc": fresh,
            "refit_over_fresh": refit / fresh,
            "images_equal_bits": bool(torch.equal(img_refit.view(torch.int32), img_fresh.view(torch.int32)))}


SOUP_EXTENT = 12.0  # scene(): centres over 2 * extent on x and z


def displaced(tri, fraction, seed=1):
    """Every triangle moved rigidly by a random vector, uniform in a ball of radius fraction * SOUP_EXTENT."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(len(tri), 1, 3))
    v *= (rng.random((len(tri), 1, 1)) ** (1 / 3)) * fraction * SOUP_EXTENT / np.linalg.norm(v, axis=-1, keepdims=True)
    moved = tri.copy()
    moved["p"] += v.astype(F)
    return moved


def rebuild_sweep(ctx, case, fractions, steps, upload_steps, budget_ms, W=1280, H=720, spp=16):
    sb = scene(case)
    tri = np.concatenate(sb.triangles)
    cam = dev.make_camera(abi.default_camera_params())
    p = abi.default_render_params(W, H, spp, 4, seed=3, traversal=abi.SRT_TRAVERSE_CLOSEST, spp_chunks=0)
    tiles = torch.zeros((dev.num_local_tiles(W, H, 1), 64, 4), dtype=torch.float32, device="cuda")

    def frame():
        """(Msamples/s, kernel ms, the tree's cost): the best of three frames after a warm-up -- or the first frame alone
        when it took longer than --frame-budget-ms (a tree a refit has ruined renders for seconds)"""
        ctx.set_camera(cam)
        ms = []
        for _ in range(4):
            ctx.render_tiles(p, tiles.data_ptr(), None)
            torch.cuda.synchronize()
            ms.append(ctx.last_kernel_ms())
            if ms[0] > budget_ms:
                break
        best = min(ms[1:]) if len(ms) > 1 else ms[0]
        return W * H * spp / (best * 1e3), best, ctx.tree_cost(0)

    def moving(d_records, then):
        def fn():
            ctx.update_triangles(0, d_records)
            then()
        return fn

    out = {"triangles": len(tri), "sweep": []}
    over_budget = False
    for f in sorted(fractions):
        moved = displaced(tri, f)
        d_moved = torch.from_numpy(moved.view(np.uint8).reshape(-1, 64)).cuda()
        ctx.upload_scene(sb)  # the unmoved scene's tree: what the refit keeps
        row = {"displacement_over_extent": f, "cost_at_build": ctx.tree_cost(0)}
        for name, then in (("refit", ctx.refit), ("rebuild", ctx.rebuild)):
            row["update_%s_ms" % name] = wall(moving(d_moved, then), steps, 1)
            if name == "refit" and over_budget:  # a smaller displacement's refit tree was over the budget already
                row["msamples_refit"], row["frame_ms_refit"], row["cost_refit"] = None, None, ctx.tree_cost(0)
                continue
            row["msamples_" + name], row["frame_ms_" + name], row["cost_" + name] = frame()
        row["upload_ms"] = wall(lambda: ctx.upload_scene(with_triangles(sb, moved)), upload_steps, 0)
        row["msamples_upload"], row["frame_ms_upload"], row["cost_upload"] = frame()
        row["cost_ratio"] = row["cost_refit"] / row["cost_at_build"]
        row["rebuild_pays"] = over_budget or row["update_rebuild_ms"] + row["frame_ms_rebuild"] < row["update_refit_ms"] + row["frame_ms_refit"]
        over_budget = over_budget or row["frame_ms_refit"] > budget_ms
        out["sweep"].append(row)
        del d_moved
    pays = [r["cost_ratio"] for r in out["sweep"] if r["rebuild_pays"]]
    out["rebuild_pays_from_cost_ratio"] = min(pays) if pays else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--upload-steps", type=int, default=2)
    ap.add_argument("--cases", default="soup_200k,soup_1m,soup_4m,masterchief")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--rebuild-cases", default="soup_200k,soup_1m,soup_4m")
    ap.add_argument("--displacements", default="0.01,0.03,0.1,0.3,1.0")
    ap.add_argument("--rebuild-steps", type=int, default=3)
    ap.add_argument("--frame-budget-ms", type=float, default=2000.0)
    a = ap.parse_args()
    ctx = dev.Context(0)
    res = {"device": ctx.device_info()["name"], "cases": {}}
    for case in [c for c in a.cases.split(",") if c]:
        res["cases"][case] = case_times(ctx, case, a.steps, a.warmup, a.upload_steps)
    if not a.no_quality:
        res["quality_soup_1m"] = quality(ctx)
    fractions = [float(x) for x in a.displacements.split(",") if x]
    res["rebuild"] = {case: rebuild_sweep(ctx, case, fractions, a.rebuild_steps, a.upload_steps, a.frame_budget_ms)
                      for case in a.rebuild_cases.split(",") if case}
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
