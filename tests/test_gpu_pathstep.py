"""Path steps on device buffers (srtCameraRaysDevice, srtScatterRaysDevice, srtPathStepDevice; include/srt_hip.h "Path
steps on device buffers") and the user-land loop over them (sexy-raytracer_amd/pathloop.py).

Every comparison is ZERO tolerance, on bytes or on uint32 views (NaN by position where a colour may be one): the camera
rays against the oracle's first path step and the NumPy mirror of the generator, the device scatter against the host
parity entry, the fused step against trace + scatter, and the loop against srtRenderImage.

Every raw call goes through buffers that are 64 elements longer than n and filled with a sentinel, and the sentinel must
survive."""
import copy
import importlib

import numpy as np
import pytest
import torch

import exact_scenes
import pathstep_ref as PR
import refit_ref as RF
import tree_build_scenes as S
from test_gpu_parity import scenes  # noqa: F401  (the module fixture of the BASELINE scenes)

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 64
SENTINEL = 0x5A
ROW = {"out": 32, "rng": 8, "rays_out": 36, "hits": 16, "recs": 88}
BUILDERS = ("REFERENCE", "LBVH", "PLOC")


@pytest.fixture(scope="module")
def pathloop(srt):
    return importlib.import_module("sexy-raytracer_amd.pathloop")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _padded(rows, n, row_bytes):
    """A device byte buffer of n + PAD rows: `rows` (or the sentinel where None) in the first n, the sentinel behind."""
    buf = np.full((n + PAD) * row_bytes, SENTINEL, np.uint8)
    if rows is not None and n:
        buf[:n * row_bytes] = np.ascontiguousarray(rows).view(np.uint8).ravel()
    return torch.from_numpy(buf).cuda()


def _rows(t, n, row_bytes):
    a = t.cpu().numpy()
    assert (a[n * row_bytes:] == SENTINEL).all(), "written beyond element n"
    return a[:n * row_bytes].reshape(n, row_bytes).copy()


def _ok(dev, c, rc):
    assert rc == 0, dev.lib.srtLastError(c.h)


def _step(dev, c, traversal, rays, rng0, fused, active=None, in_place=False, stream=None):
    """One bounce of rays (n, 9) float32 with the states rng0 (n,) int64 through the raw entries, fused or as trace +
    scatter: {name: (n, row bytes) uint8} of out, rng, rays_out and hits."""
    n = len(rays)
    handle = stream.cuda_stream if stream is not None else None
    with torch.cuda.stream(stream):
        d_rays = _padded(rays, n, 36)
        d = {"out": _padded(None, n, 32), "rng": _padded(rng0, n, 8), "hits": _padded(None, n, 16),
             "rays_out": d_rays if in_place else _padded(None, n, 36)}
        d_active = None if active is None else torch.from_numpy(np.ascontiguousarray(active, np.uint8)).cuda()
        if fused:
            _ok(dev, c, dev.lib.srtPathStepDevice(c.h, traversal, d_rays.data_ptr(), n, d_active.data_ptr() if active is not None else None,
                                                  d["rng"].data_ptr(), d["out"].data_ptr(), d["rays_out"].data_ptr(), d["hits"].data_ptr(), handle))
        else:
            assert active is None
            d_recs = _padded(None, n, 88)
            _ok(dev, c, dev.lib.srtTraceRaysDevice(c.h, d_rays.data_ptr(), n, traversal, d["hits"].data_ptr(), d_recs.data_ptr(), handle))
            _ok(dev, c, dev.lib.srtScatterRaysDevice(c.h, d_rays.data_ptr(), d_recs.data_ptr(), n, d["rng"].data_ptr(), d["out"].data_ptr(),
                                                     d["rays_out"].data_ptr(), handle))
    (stream or torch.cuda).synchronize()
    return {k: _rows(v, n, ROW[k]) for k, v in d.items()}


def _states(n, seed=1):
    return np.random.default_rng(seed).integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64)  # any 64 bits are a state


def _ray_rows(rays):
    return np.ascontiguousarray(rays).view(F).reshape(-1, 9)


def _same_floats(a, b, what=None):
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b)), what
    assert np.array_equal(_bits(a)[~nan], _bits(b)[~nan]), what


# ------------------------------------------------------------------------------------------------ 1. camera rays
@pytest.mark.parametrize("lens", ["pinhole", "aperture"])
def test_camera_rays_are_the_oracles_first_step(ctx, dev, abi, oracle, lens):
    cp = abi.default_camera_params(16.0 / 12.0)
    if lens == "pinhole":
        cp.aperture, cp.time0, cp.time1 = 0.0, 0.0, 0.0
    else:
        cp.aperture, cp.time0, cp.time1 = 0.5, 0.25, 0.75
    cam, ocam = dev.make_camera(cp), oracle.make_camera(cp)
    assert bytes(cam) == bytes(ocam)
    sb = abi.SceneBuilder()
    sb.add_sphere((0.0, 3.0, -1.0), 1.0, sb.metal((0.7, 0.6, 0.5), 0.1))
    sb.world_bvh()
    osc = oracle.OracleScene(sb)
    ctx.upload_scene(sb)
    ctx.set_camera(cam)
    W, H, seed = 16, 12, 77
    for first, spp in ((0, 3), (5, 2)):
        p = abi.default_render_params(W, H, spp, 1, seed=seed, sample_first=first)
        p.tMin = 0.125
        n = W * H * spp
        rays, rng = ctx.camera_rays_device(p)
        torch.cuda.synchronize()
        assert tuple(rays.shape) == (n, 9) and rays.dtype == torch.float32 and tuple(rng.shape) == (n,) and rng.dtype == torch.int64
        r, st = rays.cpu().numpy(), rng.cpu().numpy()
        pixel, sample = np.arange(n) // spp, first + np.arange(n) % spp
        assert (r[:, 7] == F(0.125)).all() and np.isposinf(r[:, 8]).all()
        trips = 0
        for i in range(n):
            q = abi.default_render_params(W, H, 1, 1, seed=seed, sample_first=int(sample[i]))
            steps, _ = osc.sample_path(ocam, q, int(pixel[i] % W), int(pixel[i] // W), int(sample[i]))
            want = np.concatenate([steps[0]["o"], steps[0]["d"], [steps[0]["time"]]]).astype(F)
            assert _bits(r[i, :7]).tolist() == _bits(want).tolist(), (i, r[i], want)
            assert PR.from_int64(st[i]) == PR.after_camera_ray(seed, int(pixel[i]), int(sample[i])), i
            trips += PR.from_int64(st[i]) != _advance(PR.rng_key(seed, int(pixel[i]), int(sample[i])), 5)
        assert trips > 0, "no entry's lens disk rejected a point: the rejection loop went untested"
        if lens == "aperture":
            assert len(np.unique(r[:, 6])) > n // 2 and (r[:, 6] >= 0.25).all() and (r[:, 6] <= 0.75).all()
            assert len(np.unique(r[:, 0])) > n // 2  # the lens offset moves the origin
        else:
            assert (r[:, 6] == 0).all() and (_bits(r[:, 0:3]) == _bits(r[0, 0:3])).all()
        # the explicit list, on sentinel-padded buffers, with two entries outside the image in it
        ps = np.stack([pixel, sample], axis=1).astype(np.int32)
        ps = np.concatenate([ps, [[W * H, 0], [-1, 1]]]).astype(np.int32)
        m = len(ps)
        d_rays, d_rng = _padded(None, m, 36), _padded(None, m, 8)
        d_ps = torch.from_numpy(ps).cuda()
        _ok(dev, ctx, dev.lib.srtCameraRaysDevice(ctx.h, p, d_ps.data_ptr(), m, d_rays.data_ptr(), d_rng.data_ptr(), None))
        torch.cuda.synchronize()
        lr, ls = _rows(d_rays, m, 36), _rows(d_rng, m, 8)
        assert lr[:n].tobytes() == r.tobytes() and ls[:n].tobytes() == st.tobytes()
        assert (lr[n:] == SENTINEL).all() and (ls[n:] == SENTINEL).all()
        lr2, ls2 = ctx.camera_rays_device(p, torch.from_numpy(ps[:n]).cuda())
        assert lr2.cpu().numpy().tobytes() == r.tobytes() and ls2.cpu().numpy().tobytes() == st.tobytes()


def _advance(state, draws):
    g = PR.Pcg(state)
    for _ in range(draws):
        g.bits()
    return g.state


# ------------------------------------------------------------------------------------------------ 2. scatter
@pytest.mark.parametrize("name", ["spheres", "iron", "masterchief"])
def test_scatter_device_is_the_parity_entry(ctx, dev, abi, camera, scenes, name):  # noqa: F811
    sb = scenes[name]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(64, 36, 1, 1, seed=3)
    rays, _ = ctx.camera_rays_device(p)
    _, recs = ctx.trace_device(rays, abi.SRT_TRAVERSE_FAITHFUL, records=True)
    torch.cuda.synchronize()
    rays_np = rays.cpu().numpy().view(abi.RAY_DTYPE).reshape(-1)
    recs_np = recs.cpu().numpy().view(abi.HIT_DTYPE).reshape(-1)
    hit = recs_np["prim"] >= 0
    assert 0.1 <= hit.mean()
    mats = {int(m) for m in np.unique(recs_np["material"][hit])}
    kinds = set()
    for m in mats:
        mat = sb.materials[m]
        if mat.albedoTex >= 0:
            kinds.add(("albedo", sb.textures[mat.albedoTex].kind))
        if mat.type == abi.SRT_MAT_PBR and mat.normalTex >= 0:
            kinds.add("normal map")
    want_kind = {"spheres": ("albedo", abi.SRT_TEX_CHECKER), "iron": "normal map", "masterchief": ("albedo", abi.SRT_TEX_IMAGE)}[name]
    assert want_kind in kinds, kinds
    # the hits, compacted, against srtScatterRays keyed (seed, i, 0); the misses and two bad materials behind them
    seed = 41
    h_rays, h_recs = rays_np[hit], recs_np[hit]
    k = len(h_rays)
    want = ctx.scatter_test(h_rays, h_recs, seed)
    miss = recs_np[~hit][:5]
    bad = h_recs[:2].copy()
    bad["material"] = (-1, len(sb.materials))
    all_recs = np.concatenate([h_recs, miss, bad])
    all_rays = np.concatenate([h_rays, rays_np[~hit][:5], h_rays[:2]])
    n = len(all_recs)
    rng0 = np.array([PR.as_int64(PR.rng_key(seed, i, 0)) for i in range(n)], np.int64)
    assert dev.rng_key(seed, 3, 0) == PR.rng_key(seed, 3, 0)
    got = {}
    for in_place in (False, True):
        d_rays = _padded(all_rays, n, 36)
        d = {"out": _padded(None, n, 32), "rng": _padded(rng0, n, 8), "rays_out": d_rays if in_place else _padded(None, n, 36)}
        d_recs = _padded(all_recs, n, 88)
        _ok(dev, ctx, dev.lib.srtScatterRaysDevice(ctx.h, d_rays.data_ptr(), d_recs.data_ptr(), n, d["rng"].data_ptr(),
                                                   d["out"].data_ptr(), d["rays_out"].data_ptr(), None))
        torch.cuda.synchronize()
        got[in_place] = {key: _rows(v, n, ROW[key]) for key, v in d.items()}
    out = got[False]["out"].view(abi.PATH_OUT_DTYPE).reshape(-1)
    ro = got[False]["rays_out"].view(F).reshape(n, 9)
    scattered = want[:, 9] != 0
    assert scattered.any()
    assert np.array_equal(out["status"][:k], np.where(scattered, abi.SRT_PATH_SCATTERED, abi.SRT_PATH_ENDED))
    _same_floats(out["attenuation"][:k][scattered], want[scattered, 0:3], "attenuation")
    assert (_bits(out["attenuation"][:k][~scattered]) == 0).all()
    _same_floats(out["emitted"][:k], want[:, 10:13], "emitted")
    assert np.array_equal(out["prim"][:k], h_recs["prim"])
    _same_floats(ro[:k][scattered][:, 3:6], want[scattered, 3:6], "scattered direction")
    _same_floats(ro[:k][scattered][:, 0:3], want[scattered, 6:9], "scattered origin")
    assert ro[:k][scattered][:, 6:9].tobytes() == _ray_rows(h_rays)[scattered][:, 6:9].tobytes()  # time, tMin, tMax
    assert (got[False]["rays_out"][:k][~scattered] == SENTINEL).all()
    # misses: MISS, zeros, the state and the ray untouched
    ms = slice(k, k + len(miss))
    assert (out["status"][ms] == abi.SRT_PATH_MISS).all() and (out["prim"][ms] == abi.SRT_NO_HIT).all()
    assert (_bits(out["attenuation"][ms]) == 0).all() and (_bits(out["emitted"][ms]) == 0).all()
    assert got[False]["rng"][ms].tobytes() == rng0[ms].tobytes() and (got[False]["rays_out"][ms] == SENTINEL).all()
    # a material outside the scene's: INVALID, and neither the state nor the ray is touched
    bs = slice(k + len(miss), n)
    assert (out["status"][bs] == abi.SRT_PATH_INVALID).all()
    assert got[False]["rng"][bs].tobytes() == rng0[bs].tobytes() and (got[False]["rays_out"][bs] == SENTINEL).all()
    # in place: the same outputs, and the rays that did not scatter are the incoming ones
    assert got[True]["out"].tobytes() == got[False]["out"].tobytes() and got[True]["rng"].tobytes() == got[False]["rng"].tobytes()
    moved = np.zeros(n, bool)
    moved[:k] = scattered
    assert got[True]["rays_out"][moved].tobytes() == got[False]["rays_out"][moved].tobytes()
    assert got[True]["rays_out"][~moved].tobytes() == _ray_rows(all_rays)[~moved].tobytes()
    # the wrapper: the same bytes
    w_rng = torch.from_numpy(rng0.copy()).cuda()
    w_out, w_rays = ctx.scatter_device(torch.from_numpy(_ray_rows(all_rays).copy()).cuda(),
                                       torch.from_numpy(all_recs.view(np.int32).reshape(n, 22).copy()).cuda(), w_rng)
    torch.cuda.synchronize()
    assert w_out.cpu().numpy().tobytes() == got[False]["out"].tobytes() and w_rng.cpu().numpy().tobytes() == got[False]["rng"].tobytes()
    assert w_rays.cpu().numpy()[moved].tobytes() == got[False]["rays_out"][moved].tobytes()


# ------------------------------------------------------------------------------------------------ 3. fused = unfused
@pytest.fixture(scope="module")
def step_scenes(abi):
    out = {"tierB": exact_scenes.random(abi, 4, "B")}
    for b in BUILDERS:
        out[b] = S.soup(abi, 3000, getattr(abi, "SRT_BUILDER_" + b))
    return out


@pytest.mark.parametrize("which", ["tierB"] + list(BUILDERS))
def test_fused_step_is_trace_then_scatter(ctx, dev, abi, step_scenes, which):
    ctx.upload_scene(step_scenes[which])
    capacity = ctx.device_info()["cus"] * 8 * 256  # the grid cap: one size beyond it, so that lanes take a second entry
    sizes = [0, 1, 63, 64, 65, 255, 256, 257] + ([capacity + 12_345] if which == "PLOC" else [])
    rays = _ray_rows(S.random_rays(abi, max(sizes + [4096])))
    rng0 = _states(len(rays))
    for traversal in (abi.SRT_TRAVERSE_FAITHFUL, abi.SRT_TRAVERSE_CLOSEST):
        for n in sizes + [4096]:
            fused = _step(dev, ctx, traversal, rays[:n], rng0[:n], True)
            unfused = _step(dev, ctx, traversal, rays[:n], rng0[:n], False)
            for key in ("out", "rng", "rays_out", "hits"):
                assert fused[key].tobytes() == unfused[key].tobytes(), (which, traversal, n, key)
            if n < 4096:
                continue
            status = fused["out"].view(abi.PATH_OUT_DTYPE).reshape(-1)["status"]
            assert {abi.SRT_PATH_MISS, abi.SRT_PATH_SCATTERED} <= set(status.tolist()) and abi.SRT_PATH_INVALID not in status
            # the wrapper with hits: the same bytes where something is written
            w_rng = torch.from_numpy(rng0[:n].copy()).cuda()
            w_out, w_rays, w_hits = ctx.path_step_device(torch.from_numpy(rays[:n].copy()).cuda(), w_rng, traversal, hits=True)
            torch.cuda.synchronize()
            assert w_out.cpu().numpy().tobytes() == fused["out"].tobytes() and w_hits.cpu().numpy().tobytes() == fused["hits"].tobytes()
            assert w_rng.cpu().numpy().tobytes() == fused["rng"].tobytes()
            # a random mask: masked-out entries keep their sentinels (and their state), the rest equal the unmasked call
            active = (np.random.default_rng(n).random(n) < 0.6).astype(np.uint8)
            active[:3] = (0, 1, 2)  # any non-zero byte is active
            masked = _step(dev, ctx, traversal, rays[:n], rng0[:n], True, active=active)
            on = active != 0
            for key in ("out", "rng", "rays_out", "hits"):
                assert masked[key][on].tobytes() == fused[key][on].tobytes(), (which, traversal, key)
                if key == "rng":
                    assert masked[key][~on].tobytes() == rng0[:n][~on].tobytes()
                else:
                    assert (masked[key][~on] == SENTINEL).all(), (which, traversal, key)
            in_place = _step(dev, ctx, traversal, rays[:n], rng0[:n], True, in_place=True)
            moved = status == abi.SRT_PATH_SCATTERED
            assert in_place["out"].tobytes() == fused["out"].tobytes()
            assert in_place["rays_out"][moved].tobytes() == fused["rays_out"][moved].tobytes()
            assert in_place["rays_out"][~moved].tobytes() == rays[:n][~moved].tobytes()
    assert dev.lib.srtPathStepDevice(ctx.h, abi.SRT_TRAVERSE_CLOSEST, None, 0, None, None, None, None, None, None) == 0
    assert dev.lib.srtScatterRaysDevice(ctx.h, None, None, 0, None, None, None, None) == 0
    empty = torch.zeros((0, 9), dtype=torch.float32, device="cuda")
    out, _ = ctx.path_step_device(empty, torch.zeros((0,), dtype=torch.int64, device="cuda"))
    assert tuple(out.shape) == (0, 8)


# ------------------------------------------------------------------------------------------------ 4. the loop is the render
def _assert_loop_is_render(ctx, pathloop, p, what):
    want = ctx.render_image(p, want_rgba=False)[0]
    for fused in (True, False):
        got = pathloop.render(ctx, p, fused=fused)
        torch.cuda.synchronize()
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32
        got = got.cpu().numpy()
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, fused)
        differ = ((_bits(got) != _bits(want)) & ~nan).any(axis=-1)
        assert not differ.any(), (what, "fused" if fused else "unfused", int(differ.sum()), np.argwhere(differ)[:4].tolist(),
                                  got[differ][:2].tolist(), want[differ][:2].tolist())
    return want


@pytest.mark.parametrize("tier", exact_scenes.TIERS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_loop_is_the_render_on_exact_scenes(ctx, dev, abi, camera, pathloop, tier, seed):
    sb = exact_scenes.random(abi, seed, tier)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    for bounces, first in ((1, 0), (4, 0), (16, 0), (4, 7)):
        p = abi.default_render_params(32, 24, 4, bounces, seed=11 + seed, sample_first=first)
        want = _assert_loop_is_render(ctx, pathloop, p, (tier, seed, bounces, first))
        assert (want[..., 3] == 4).all()  # (a frame may well be black: tier B, seed 0 puts the camera inside a sphere)
    # batches of sample indices: the same running sum
    p = abi.default_render_params(32, 24, 4, 4, seed=11 + seed)
    whole, parts = pathloop.render(ctx, p), pathloop.render(ctx, p, samples_per_batch=3)
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))


@pytest.mark.parametrize("name", ["spheres", "iron", "masterchief"])
def test_loop_is_the_render_on_the_baseline_scenes(ctx, abi, camera, pathloop, scenes, name):  # noqa: F811
    ctx.upload_scene(scenes[name])
    ctx.set_camera(camera)
    want = _assert_loop_is_render(ctx, pathloop, abi.default_render_params(64, 36, 2, 8, seed=5), name)
    assert len(np.unique(want[..., :3])) > 500  # a real frame


def test_loop_steps_are_the_oracles_path(ctx, dev, abi, oracle, pathloop):
    """prim, attenuation and emitted of every bounce of a handful of samples against OracleScene.sample_path (tier A: no
    libm call anywhere in the shading)."""
    sb = exact_scenes.random(abi, 0, "A")
    cp = abi.default_camera_params()
    cam, ocam = dev.make_camera(cp), oracle.make_camera(cp)
    ctx.upload_scene(sb)
    ctx.set_camera(cam)
    osc = oracle.OracleScene(sb)
    W, H, bounces, seed = 32, 24, 8, 19
    picks = [(3, 2, 0), (16, 12, 1), (31, 23, 2), (10, 20, 0), (20, 5, 3), (8, 8, 1), (25, 14, 2), (14, 17, 0)]
    p = abi.default_render_params(W, H, 1, bounces, seed=seed)
    ps = torch.tensor([[y * W + x, s] for x, y, s in picks], dtype=torch.int32, device="cuda")
    rays, rng = ctx.camera_rays_device(p, ps)
    active = torch.ones(len(picks), dtype=torch.uint8, device="cuda")
    depth = np.zeros(len(picks), int)
    paths = [osc.sample_path(ocam, abi.default_render_params(W, H, 1, bounces, seed=seed, sample_first=s), x, y, s)[0] for x, y, s in picks]
    assert max(len(s) for s in paths) >= 3
    for j in range(bounces):
        out, rays, hits = ctx.path_step_device(rays, rng, abi.SRT_TRAVERSE_FAITHFUL, active=active, rays_out=rays, hits=True)
        torch.cuda.synchronize()
        o = out.cpu().numpy().view(abi.PATH_OUT_DTYPE).reshape(-1)
        on = active.cpu().numpy() != 0
        for i in np.flatnonzero(on):
            step = paths[i][j]
            assert o["prim"][i] == step["prim"] == hits.cpu().numpy()[i, 0], (i, j)
            if step["prim"] < 0:
                assert o["status"][i] == abi.SRT_PATH_MISS
                continue
            assert (o["status"][i] == abi.SRT_PATH_SCATTERED) == bool(step["scattered"]), (i, j)
            _same_floats(o["emitted"][i], step["emitted"], (i, j))
            if step["scattered"]:
                _same_floats(o["attenuation"][i], step["attenuation"], (i, j))
            depth[i] = j + 1
        active = torch.from_numpy(((o["status"] == abi.SRT_PATH_SCATTERED) & on).astype(np.uint8)).cuda()
        for i in range(len(picks)):  # a path is as long as the oracle's
            assert bool(active[i]) == (j + 1 < len(paths[i]) or (j + 1 == len(paths[i]) == bounces and bool(paths[i][j]["scattered"]))), (i, j)


# ------------------------------------------------------------------------------------------------ 5. ordering, state, errors
def test_step_runs_behind_the_op_that_made_the_rays(ctx, dev, abi, step_scenes):
    ctx.upload_scene(step_scenes["PLOC"])
    rays = _ray_rows(S.random_rays(abi, 8192)).copy()
    rng0 = _states(len(rays))
    moved = rays.copy()
    moved[:, 0] += F(0.75)  # another origin: other primitives, other colours
    want = _step(dev, ctx, abi.SRT_TRAVERSE_CLOSEST, moved, rng0, True)
    assert want["out"].tobytes() != _step(dev, ctx, abi.SRT_TRAVERSE_CLOSEST, rays, rng0, True)["out"].tobytes()
    side = torch.cuda.Stream()
    d = torch.from_numpy(rays).cuda()
    d_rng = torch.from_numpy(rng0.copy()).cuda()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d[:, 0] += 0.75
        out, rays_out, hits = ctx.path_step_device(d, d_rng, abi.SRT_TRAVERSE_CLOSEST, hits=True, stream=side)
    side.synchronize()
    assert out.cpu().numpy().tobytes() == want["out"].tobytes() and hits.cpu().numpy().tobytes() == want["hits"].tobytes()
    assert d_rng.cpu().numpy().tobytes() == want["rng"].tobytes()
    torch.cuda.synchronize()


@pytest.mark.parametrize("builder", ["LBVH", "PLOC"])
def test_loop_is_the_render_after_refit_and_rebuild(ctx, abi, camera, pathloop, step_scenes, builder):
    sb = step_scenes[builder]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(32, 24, 2, 4, seed=9)
    before = _assert_loop_is_render(ctx, pathloop, p, "uploaded")
    tri = RF.scene_triangles(sb)
    first, count = 200, 700
    tri["p"][first:first + count] += np.random.default_rng(2).normal(0, 0.5, (count, 1, 3)).astype(F)
    ctx.update_triangles(first, tri[first:first + count])
    ctx.refit()
    refit = _assert_loop_is_render(ctx, pathloop, p, "refitted")
    assert refit.tobytes() != before.tobytes()
    ctx.rebuild()
    _assert_loop_is_render(ctx, pathloop, p, "rebuilt")


def test_side_effects_and_errors(ctx, dev, abi, camera, step_scenes):
    sb = step_scenes["PLOC"]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(64, 36, 2, 4, seed=5)
    first = ctx.render_image(p)[0]
    info, ms, stats = ctx.launch_info(), ctx.last_kernel_ms(), ctx.stats()
    tunables = {k: ctx.get_tunable(k) for k in ("ploc_radius", "fast_div", "wavefront", "lds_tree", "wf_resident_max")}
    dev.host_random_reset()
    draws = [dev.host_random_float() for _ in range(3)]
    dev.host_random_reset()
    dev.host_random_float()
    rays = _ray_rows(S.random_rays(abi, 4096))
    rng0 = _states(len(rays))
    for fused in (True, False):
        _step(dev, ctx, abi.SRT_TRAVERSE_CLOSEST, rays, rng0, fused)
        _step(dev, ctx, abi.SRT_TRAVERSE_FAITHFUL, rays, rng0, fused)
    ctx.camera_rays_device(p)
    torch.cuda.synchronize()
    assert (ctx.launch_info(), ctx.last_kernel_ms(), ctx.stats()) == (info, ms, stats)
    assert [dev.host_random_float() for _ in range(2)] == draws[1:]
    assert {k: ctx.get_tunable(k) for k in tunables} == tunables
    assert ctx.render_image(p)[0].tobytes() == first.tobytes()
    assert ctx.launch_info() == info

    # errors: refused on the host, nothing launched, the outputs keep their sentinel.  Every address below is either NULL
    # or inside a live buffer: a misaligned pointer is a live buffer's address plus a few bytes.
    n = len(rays)
    d_rays = _padded(rays, n, 36)
    d_recs = torch.zeros(((n + PAD) * 88,), dtype=torch.uint8, device="cuda")
    outs = {k: _padded(None, n, ROW[k]) for k in ("out", "rng", "rays_out", "hits")}
    R, RC, O, G, RO, H = (t.data_ptr() for t in (d_rays, d_recs, outs["out"], outs["rng"], outs["rays_out"], outs["hits"]))
    assert all(a % 16 == 0 for a in (R, RC, O, G, RO, H))
    CL = abi.SRT_TRAVERSE_CLOSEST
    step, scatter, camera_rays = dev.lib.srtPathStepDevice, dev.lib.srtScatterRaysDevice, dev.lib.srtCameraRaysDevice

    def refused(rc, text, c=ctx):
        assert rc != 0 and text in dev.lib.srtLastError(c.h), (rc, dev.lib.srtLastError(c.h))
        torch.cuda.synchronize()
        for buf in outs.values():
            assert bool((buf == SENTINEL).all())

    refused(step(ctx.h, CL, R, -1, None, G, O, RO, H, None), b"negative")
    refused(scatter(ctx.h, R, RC, -1, G, O, RO, None), b"negative")
    refused(camera_rays(ctx.h, p, R, -1, RO, G, None), b"negative")
    refused(step(ctx.h, CL, None, n, None, G, O, RO, H, None), b"null rays")
    refused(step(ctx.h, CL, R, n, None, None, O, RO, H, None), b"null rng")
    refused(step(ctx.h, CL, R, n, None, G, None, RO, H, None), b"null outputs")
    refused(step(ctx.h, CL, R, n, None, G, O, None, H, None), b"null scattered")
    refused(scatter(ctx.h, None, RC, n, G, O, RO, None), b"null rays")
    refused(scatter(ctx.h, R, None, n, G, O, RO, None), b"null records")
    refused(scatter(ctx.h, R, RC, n, None, O, RO, None), b"null rng")
    refused(scatter(ctx.h, R, RC, n, G, None, RO, None), b"null outputs")
    refused(scatter(ctx.h, R, RC, n, G, O, None, None), b"null scattered")
    refused(step(ctx.h, CL, R + 2, n, None, G, O, RO, H, None), b"rays are not aligned")
    refused(step(ctx.h, CL, R, n, None, G + 4, O, RO, H, None), b"rng states are not aligned")
    refused(step(ctx.h, CL, R, n, None, G, O + 8, RO, H, None), b"outputs are not aligned")
    refused(step(ctx.h, CL, R, n, None, G, O, RO + 2, H, None), b"scattered rays are not aligned")
    refused(step(ctx.h, CL, R, n, None, G, O, RO, H + 8, None), b"hits are not aligned")
    refused(scatter(ctx.h, R, RC + 2, n, G, O, RO, None), b"records are not aligned")
    refused(scatter(ctx.h, R, RC, n, G + 4, O, RO, None), b"rng states are not aligned")
    refused(scatter(ctx.h, R, RC, n, G, O + 8, RO, None), b"outputs are not aligned")
    for bad in (2, -1, 7):
        refused(step(ctx.h, bad, R, n, None, G, O, RO, H, None), b"neither")
    assert step(None, CL, R, n, None, G, O, RO, H, None) != 0 and scatter(None, R, RC, n, G, O, RO, None) != 0
    assert camera_rays(None, p, None, n, RO, G, None) != 0
    # the camera entry: the frame's own count without a list, an image of at least 2 x 2, its pointers
    p = abi.default_render_params(64, 36, 1, 4, seed=5)
    frame = p.imageWidth * p.imageHeight * p.spp
    assert frame <= n
    refused(camera_rays(ctx.h, p, None, frame - 1, RO, G, None), b"without a list")
    refused(camera_rays(ctx.h, None, None, frame, RO, G, None), b"null parameters")
    refused(camera_rays(ctx.h, p, None, frame, None, G, None), b"null rays")
    refused(camera_rays(ctx.h, p, None, frame, RO, None, None), b"null rng")
    refused(camera_rays(ctx.h, p, None, frame, RO + 2, G, None), b"rays are not aligned")
    refused(camera_rays(ctx.h, p, None, frame, RO, G + 4, None), b"rng states are not aligned")
    refused(camera_rays(ctx.h, p, R + 2, 16, RO, G, None), b"list is not aligned")
    for w, h in ((1, 36), (64, 1)):
        small = copy.copy(p)
        small.imageWidth, small.imageHeight = w, h
        refused(camera_rays(ctx.h, small, R, 16, RO, G, None), b"at least 2x2")
    fresh = dev.Context(0)
    try:
        refused(step(fresh.h, CL, R, n, None, G, O, RO, H, None), b"no scene", fresh)
        refused(scatter(fresh.h, R, RC, n, G, O, RO, None), b"no scene", fresh)
        refused(camera_rays(fresh.h, p, None, frame, RO, G, None), b"no camera", fresh)
    finally:
        fresh.close()
    with pytest.raises(dev.SrtError, match="neither"):
        ctx.path_step_device(torch.zeros((4, 9), dtype=torch.float32, device="cuda"), torch.zeros((4,), dtype=torch.int64, device="cuda"), traversal=5)
    # updated and not refitted: refused in checkSceneReady's words; then refitted, so that the shared context works again
    tri = RF.scene_triangles(sb)
    ctx.update_triangles(0, tri[:16])
    try:
        refused(step(ctx.h, CL, R, n, None, G, O, RO, H, None), b"geometry was updated")
        refused(scatter(ctx.h, R, RC, n, G, O, RO, None), b"geometry was updated")
    finally:
        ctx.refit()
    assert _step(dev, ctx, CL, rays, rng0, True)["out"].tobytes() == _step(dev, ctx, CL, rays, rng0, False)["out"].tobytes()
