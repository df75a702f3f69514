"""srtTracePathsDevice (include/srt_hip.h "Path steps on device buffers"): whole paths for device rays in one kernel.

The checker is tests/paths_ref.py: the masked srtPathStepDevice loop that was there before this entry, a launch per bounce.
The kernel is compared to that, to pathloop's loops and to srtRenderImage, never to itself, and with ZERO tolerance: the
bytes of steps, status and the final generator state; the radiance on uint32 views, NaN by position.

Every raw call goes through buffers that are 64 elements longer than n and filled with a sentinel, the scratch included, and
the sentinel must survive; the rays must keep their bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_scenes
import paths_ref
import refit_ref as RF
import tree_build_scenes as S
from test_gpu_parity import scenes  # noqa: F401  (the module fixture of the BASELINE scenes)
from test_gpu_pathstep import (BUILDERS, PAD, SENTINEL, _bits, _padded, _ray_rows, _rows, _same_floats, _states,  # noqa: F401
                               pathloop, step_scenes)

pytestmark = pytest.mark.gpu

F = np.float32
BG = (0.53, 0.81, 0.92)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4096)
BOUNCES = (0, 1, 4, 16)
DEEP_NODES = 120  # the chain tree below: a walk stack of 120 slots


def _traversals(abi):
    return (abi.SRT_TRAVERSE_FAITHFUL, abi.SRT_TRAVERSE_CLOSEST)


def _call(dev, c, traversal, max_bounce, d_rays, n, d_rng, d_result, d_scratch, stream=None, background=BG):
    bg = (C.c_float * 3)(*background)
    return dev.lib.srtTracePathsDevice(c.h, traversal, max_bounce, bg, d_rays.data_ptr(), n, d_rng.data_ptr(), d_result.data_ptr(),
                                       d_scratch.data_ptr(), stream.cuda_stream if stream is not None else None)


def _trace(dev, abi, c, traversal, max_bounce, rays, rng0, stream=None, background=BG):
    """One raw call on sentinel-padded buffers: {"radiance", "steps", "status", "rng"} as paths_ref.loop returns them."""
    n = len(rays)
    with torch.cuda.stream(stream):
        d_rays, d_rng, d_result = _padded(rays, n, 36), _padded(rng0, n, 8), _padded(None, n, 16)
        d_scratch = _padded(None, 1, abi.SRT_PATHS_SCRATCH_BYTES)
        rc = _call(dev, c, traversal, max_bounce, d_rays, n, d_rng, d_result, d_scratch, stream, background)
        assert rc == 0, dev.lib.srtLastError(c.h)
    (stream or torch.cuda).synchronize()
    assert _rows(d_rays, n, 36).tobytes() == np.ascontiguousarray(rays).tobytes(), "the rays were written"
    scratch = _rows(d_scratch, 1, abi.SRT_PATHS_SCRATCH_BYTES)  # (its tail keeps the sentinel)
    assert n > 0 or (scratch == SENTINEL).all(), "n == 0 launches nothing, the memset included"
    return _split(abi, _rows(d_result, n, 16), _rows(d_rng, n, 8))


def _split(abi, result_rows, rng_rows):
    res = np.ascontiguousarray(result_rows).view(abi.PATH_RADIANCE_DTYPE).reshape(-1)
    return {"radiance": res["radiance"].copy(), "steps": res["steps"].copy(), "status": res["status"].copy(),
            "rng": np.ascontiguousarray(rng_rows).view(np.int64).reshape(-1).copy()}


def _assert_same(got, want, what):
    for key in ("steps", "status", "rng"):
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (what, key, np.flatnonzero(got[key] != want[key])[:8])
    _same_floats(got["radiance"], want["radiance"], what)


def _chain_tree(abi, nodes=DEEP_NODES):
    """nodes + 1 spheres in a row under a caller-built tree that is one long chain: node i holds sphere i and node i + 1, so a
    walk may have `nodes` references pending.  Every box is the whole row's (a valid, if useless, tree)."""
    sb = abi.SceneBuilder()
    mats = [sb.metal((0.8, 0.7, 0.6), 0.3), sb.light((4.0, 3.0, 2.0)), sb.dielectric(1.5)]
    for i in range(nodes + 1):
        sb.add_sphere((0.06 * (i - nodes / 2), 3.0 + 0.3 * np.sin(i), -1.0 - 0.02 * i), 0.2, mats[i % 3])
    tree = np.zeros(nodes, abi.NODE_DTYPE)
    tree["bmin"], tree["bmax"] = (-10.0, -10.0, -10.0), (10.0, 10.0, 10.0)
    tree["left"] = np.arange(1, nodes + 1)
    tree["right"] = ~np.arange(nodes)
    tree["left"][-1] = ~(nodes - 1)
    tree["right"][-1] = ~nodes
    sb.world_prebuilt(tree)
    return sb


@pytest.fixture(scope="module")
def path_scenes(abi, step_scenes):  # noqa: F811
    out = dict(step_scenes)
    out["room"] = exact_scenes.room(abi, "B")
    out["chain"] = _chain_tree(abi)
    return out


# ------------------------------------------------------------------------------------------------ 1. whole path = the loop
@pytest.mark.parametrize("which", ["tierB"] + list(BUILDERS) + ["room", "chain"])
def test_whole_path_is_the_loop_entry_by_entry(ctx, dev, abi, path_scenes, which):
    ctx.upload_scene(path_scenes[which])
    rays = _ray_rows(S.random_rays(abi, max(SIZES)))
    rng0 = _states(len(rays))
    # the chain's walk stack is 122 KB: 16 bounces of attenuations beside it do not fit (refused: test_side_effects_and_errors)
    bounces = [b for b in BOUNCES if which != "chain" or b <= 4]
    if which == "chain":
        assert ctx.bvh_depth() >= DEEP_NODES
    for traversal in _traversals(abi):
        for max_bounce in bounces:
            want = paths_ref.loop(ctx, abi, rays, rng0, max_bounce, BG, traversal)
            assert want["steps"].max() <= max_bounce and (want["steps"] >= min(1, max_bounce)).all()
            if max_bounce == 4 and which != "chain":  # on the REFERENCE loop's output alone: the cases are there
                st = set(want["status"].tolist())
                assert len(set(want["steps"].tolist())) >= 3, (which, set(want["steps"].tolist()))
                assert abi.SRT_PATH_SCATTERED in st and abi.SRT_PATH_INVALID not in st, (which, st)  # SCATTERED: at the limit
                assert (abi.SRT_PATH_ENDED if which == "room" else abi.SRT_PATH_MISS) in st, (which, st)  # (the room is closed)
                assert (want["steps"][want["status"] == abi.SRT_PATH_SCATTERED] == 4).all()
            if max_bounce == 4 and which == "chain":
                assert (want["steps"] > 1).any()
            for n in SIZES:
                got = _trace(dev, abi, ctx, traversal, max_bounce, rays[:n], rng0[:n])
                _assert_same(got, paths_ref.prefix(want, n), (which, traversal, max_bounce, n))
    # the wrapper: the same bytes, the states advanced in place
    w_rng = torch.from_numpy(rng0.copy()).cuda()
    w = ctx.trace_paths_device(torch.from_numpy(rays.copy()).cuda(), w_rng, 4, BG, abi.SRT_TRAVERSE_CLOSEST)
    torch.cuda.synchronize()
    assert tuple(w.shape) == (len(rays), 4) and w.dtype == torch.int32
    _assert_same(_split(abi, w.cpu().numpy().view(np.uint8), w_rng.cpu().numpy().view(np.uint8)),
                 paths_ref.loop(ctx, abi, rays, rng0, 4, BG, abi.SRT_TRAVERSE_CLOSEST), (which, "wrapper"))
    empty = ctx.trace_paths_device(torch.zeros((0, 9), dtype=torch.float32, device="cuda"), torch.zeros((0,), dtype=torch.int64, device="cuda"), 4, BG)
    assert tuple(empty.shape) == (0, 4)


def test_lanes_refill_beyond_the_resident_lanes(ctx, dev, abi, path_scenes):
    """More entries than lanes can be resident at once (8 workgroups of 256 on every CU is the hardware's limit), so lanes
    take second entries from the counter; with either refill threshold."""
    ctx.upload_scene(path_scenes["PLOC"])
    n = ctx.device_info()["cus"] * 8 * 256 + 12_345
    rays = _ray_rows(S.random_rays(abi, n))
    rng0 = _states(n)
    saved = ctx.get_tunable("paths_refill_min")
    try:
        for traversal, refill in zip(_traversals(abi), (16, 1)):
            ctx.set_tunable("paths_refill_min", refill)
            want = paths_ref.loop(ctx, abi, rays, rng0, 4, BG, traversal)
            assert len(set(want["steps"].tolist())) >= 3
            _assert_same(_trace(dev, abi, ctx, traversal, 4, rays, rng0), want, (traversal, refill))
    finally:
        ctx.set_tunable("paths_refill_min", saved)


# ------------------------------------------------------------------------------------------------ 2. uneven waves
@pytest.mark.parametrize("refill", [1, 16, 64])
def test_uneven_waves(ctx, dev, abi, path_scenes, refill):
    """Every 64th entry starts inside the closed room and runs long; all the others start outside it and fly away: one step.
    The counter runs out in the middle of a wave."""
    ctx.upload_scene(path_scenes["room"])
    n = 64 * 37 + 5
    rays = _ray_rows(S.random_rays(abi, n)).copy()
    away = np.arange(n) % 64 != 0
    rays[away, 0:3] = (0.0, 100.0, 0.0)   # outside the room's sphere of radius 30 about the origin ...
    rays[away, 3:6] = np.abs(rays[away, 3:6]) + F(0.25) * np.array([0.0, 1.0, 0.0], F)  # ... and upward, away from it
    rng0 = _states(n)
    saved = ctx.get_tunable("paths_refill_min")
    ctx.set_tunable("paths_refill_min", refill)
    try:
        for traversal in _traversals(abi):
            want = paths_ref.loop(ctx, abi, rays, rng0, 16, BG, traversal)
            assert (want["steps"][away] == 1).all() and (want["status"][away] == abi.SRT_PATH_MISS).all()
            assert np.median(want["steps"][~away]) >= 4 and want["steps"].max() == 16
            _assert_same(_trace(dev, abi, ctx, traversal, 16, rays, rng0), want, (traversal, "forward"))
            back = np.arange(n)[::-1]
            _assert_same(_trace(dev, abi, ctx, traversal, 16, rays[back], rng0[back]), paths_ref.take(want, back), (traversal, "reversed"))
    finally:
        ctx.set_tunable("paths_refill_min", saved)


# ------------------------------------------------------------------------------------------------ 3. the frame is the render
def _assert_whole_is_render(ctx, pathloop, p, what, **kwargs):  # noqa: F811
    want = ctx.render_image(p, want_rgba=False)[0]
    got = pathloop.render(ctx, p, whole=True, **kwargs)
    torch.cuda.synchronize()
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    differ = ((_bits(got) != _bits(want)) & ~nan).any(axis=-1)
    assert not differ.any(), (what, int(differ.sum()), np.argwhere(differ)[:4].tolist(), got[differ][:2].tolist(), want[differ][:2].tolist())
    return want


@pytest.mark.parametrize("tier", exact_scenes.TIERS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_frame_is_the_render_on_exact_scenes(ctx, abi, camera, pathloop, tier, seed):  # noqa: F811
    ctx.upload_scene(exact_scenes.random(abi, seed, tier))
    ctx.set_camera(camera)
    for bounces, first in ((1, 0), (4, 0), (16, 0), (4, 7)):
        p = abi.default_render_params(32, 24, 4, bounces, seed=11 + seed, sample_first=first)
        want = _assert_whole_is_render(ctx, pathloop, p, (tier, seed, bounces, first))
        assert (want[..., 3] == 4).all()
    p = abi.default_render_params(32, 24, 4, 4, seed=11 + seed)
    _assert_whole_is_render(ctx, pathloop, p, (tier, seed, "batches of 3"), samples_per_batch=3)


@pytest.mark.parametrize("name", ["spheres", "iron", "masterchief"])
def test_frame_is_the_render_on_the_baseline_scenes(ctx, abi, camera, pathloop, scenes, name):  # noqa: F811
    ctx.upload_scene(scenes[name])
    ctx.set_camera(camera)
    want = _assert_whole_is_render(ctx, pathloop, abi.default_render_params(64, 36, 2, 8, seed=5), name)
    assert len(np.unique(want[..., :3])) > 500  # a real frame


# ------------------------------------------------------------------------------------------------ 4. builders
@pytest.mark.parametrize("builder", ["LBVH", "PLOC"])
def test_frame_is_the_render_after_refit_and_rebuild(ctx, abi, camera, pathloop, step_scenes, builder):  # noqa: F811
    sb = step_scenes[builder]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(32, 24, 2, 4, seed=9)
    before = _assert_whole_is_render(ctx, pathloop, p, "uploaded")
    tri = RF.scene_triangles(sb)
    first, count = 200, 700
    tri["p"][first:first + count] += np.random.default_rng(2).normal(0, 0.5, (count, 1, 3)).astype(F)
    ctx.update_triangles(first, tri[first:first + count])
    ctx.refit()
    refit = _assert_whole_is_render(ctx, pathloop, p, "refitted")
    assert refit.tobytes() != before.tobytes()
    ctx.rebuild()
    _assert_whole_is_render(ctx, pathloop, p, "rebuilt")


# ------------------------------------------------------------------------------------------------ 5. nothing else is written
def test_nothing_else_is_written(ctx, dev, abi, path_scenes):
    """_trace checks every call of this file; here once in the open, with a scratch whose bytes in front are looked at too."""
    ctx.upload_scene(path_scenes["tierB"])
    n = 1000
    rays, rng0 = _ray_rows(S.random_rays(abi, n)), _states(n)
    d_rays, d_rng, d_result = _padded(rays, n, 36), _padded(rng0, n, 8), _padded(None, n, 16)
    d_scratch = torch.full((PAD + abi.SRT_PATHS_SCRATCH_BYTES + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    bg = (C.c_float * 3)(*BG)
    rc = dev.lib.srtTracePathsDevice(ctx.h, abi.SRT_TRAVERSE_CLOSEST, 4, bg, d_rays.data_ptr(), n, d_rng.data_ptr(), d_result.data_ptr(),
                                     d_scratch.data_ptr() + PAD, None)
    assert rc == 0, dev.lib.srtLastError(ctx.h)
    torch.cuda.synchronize()
    assert d_rays.cpu().numpy()[:n * 36].tobytes() == rays.tobytes() and (d_rays.cpu().numpy()[n * 36:] == SENTINEL).all()
    assert (d_result.cpu().numpy()[n * 16:] == SENTINEL).all() and (d_rng.cpu().numpy()[n * 8:] == SENTINEL).all()
    s = d_scratch.cpu().numpy()
    assert (s[:PAD] == SENTINEL).all() and (s[PAD + abi.SRT_PATHS_SCRATCH_BYTES:] == SENTINEL).all()
    assert (s[PAD:PAD + abi.SRT_PATHS_SCRATCH_BYTES] != SENTINEL).any()  # (the call did clear its 64 bytes)
    _assert_same(_split(abi, _rows(d_result, n, 16), _rows(d_rng, n, 8)), paths_ref.loop(ctx, abi, rays, rng0, 4, BG, abi.SRT_TRAVERSE_CLOSEST), "open")


# ------------------------------------------------------------------------------------------------ 6. ordering
def test_call_runs_behind_the_op_that_made_the_rays(ctx, dev, abi, path_scenes):
    ctx.upload_scene(path_scenes["PLOC"])
    rays = _ray_rows(S.random_rays(abi, 8192)).copy()
    rng0 = _states(len(rays))
    moved = rays.copy()
    moved[:, 0] += F(0.75)  # another origin: other primitives, other colours
    want = paths_ref.loop(ctx, abi, moved, rng0, 4, BG, abi.SRT_TRAVERSE_CLOSEST)
    assert want["radiance"].tobytes() != paths_ref.loop(ctx, abi, rays, rng0, 4, BG, abi.SRT_TRAVERSE_CLOSEST)["radiance"].tobytes()
    side = torch.cuda.Stream()
    d = torch.from_numpy(rays).cuda()
    d_rng = torch.from_numpy(rng0.copy()).cuda()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d[:, 0] += 0.75
        result = ctx.trace_paths_device(d, d_rng, 4, BG, abi.SRT_TRAVERSE_CLOSEST, stream=side)
    side.synchronize()
    _assert_same(_split(abi, result.cpu().numpy().view(np.uint8), d_rng.cpu().numpy().view(np.uint8)), want, "side stream")
    torch.cuda.synchronize()


def test_two_calls_on_one_stream_may_share_the_scratch(ctx, dev, abi, path_scenes):
    ctx.upload_scene(path_scenes["LBVH"])
    n = 20_000
    rays = torch.from_numpy(_ray_rows(S.random_rays(abi, n)).copy()).cuda()
    other = rays.clone()
    other[:, 0] += 0.5
    rng0 = _states(n)
    got = {}
    for shared in (True, False):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            scratch = [torch.empty((abi.SRT_PATHS_SCRATCH_BYTES,), dtype=torch.uint8, device="cuda") for _ in range(2)]
            rng_a, rng_b = torch.from_numpy(rng0.copy()).cuda(), torch.from_numpy(rng0.copy()).cuda()
            a = ctx.trace_paths_device(rays, rng_a, 4, BG, abi.SRT_TRAVERSE_CLOSEST, scratch=scratch[0], stream=stream)
            b = ctx.trace_paths_device(other, rng_b, 16, BG, abi.SRT_TRAVERSE_FAITHFUL, scratch=scratch[0 if shared else 1], stream=stream)
        stream.synchronize()
        got[shared] = [t.cpu().numpy().tobytes() for t in (a, b, rng_a, rng_b)]
    assert got[True] == got[False]
    assert got[True][0] != got[True][1]
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. side effects, errors
def test_side_effects_and_errors(ctx, dev, abi, camera, path_scenes):
    sb = path_scenes["PLOC"]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(64, 36, 2, 4, seed=5)
    first = ctx.render_image(p)[0]
    info, ms, stats = ctx.launch_info(), ctx.last_kernel_ms(), ctx.stats()
    tunables = {k: ctx.get_tunable(k) for k in ("ploc_radius", "fast_div", "wavefront", "lds_tree", "wf_resident_max", "paths_refill_min")}
    dev.host_random_reset()
    draws = [dev.host_random_float() for _ in range(3)]
    dev.host_random_reset()
    dev.host_random_float()
    rays = _ray_rows(S.random_rays(abi, 4096))
    rng0 = _states(len(rays))
    for traversal in _traversals(abi):
        _trace(dev, abi, ctx, traversal, 4, rays, rng0)
    torch.cuda.synchronize()
    assert (ctx.launch_info(), ctx.last_kernel_ms(), ctx.stats()) == (info, ms, stats)
    assert [dev.host_random_float() for _ in range(2)] == draws[1:]
    assert {k: ctx.get_tunable(k) for k in tunables} == tunables
    assert ctx.render_image(p)[0].tobytes() == first.tobytes()
    assert ctx.launch_info() == info

    # errors: refused on the host, nothing launched, the outputs keep their sentinel.  Every address below is either NULL
    # or inside a live buffer: a misaligned or overlapping pointer is a live buffer's address plus a few bytes.
    n = len(rays)
    d_rays = _padded(rays, n, 36)
    outs = {"result": _padded(None, n, 16), "rng": _padded(None, n, 8), "scratch": _padded(None, 1, abi.SRT_PATHS_SCRATCH_BYTES)}
    R, O, G, X = (t.data_ptr() for t in (d_rays, outs["result"], outs["rng"], outs["scratch"]))
    assert all(a % 16 == 0 for a in (R, O, G, X))
    CL, bg = abi.SRT_TRAVERSE_CLOSEST, (C.c_float * 3)(*BG)
    call = dev.lib.srtTracePathsDevice

    def refused(rc, text, c=ctx):
        assert rc != 0 and text in dev.lib.srtLastError(c.h), (rc, text, dev.lib.srtLastError(c.h))
        torch.cuda.synchronize()
        for buf in outs.values():
            assert bool((buf == SENTINEL).all())
        assert d_rays.cpu().numpy()[:n * 36].tobytes() == rays.tobytes()

    refused(call(ctx.h, CL, 4, bg, R, -1, G, O, X, None), b"negative")
    for bad in (2, -1, 7):
        refused(call(ctx.h, bad, 4, bg, R, n, G, O, X, None), b"neither")
    for bad in (17, -1):
        refused(call(ctx.h, CL, bad, bg, R, n, G, O, X, None), b"maxBounce")
    refused(call(ctx.h, CL, 4, None, R, n, G, O, X, None), b"null background")
    refused(call(ctx.h, CL, 4, None, None, 0, None, None, None, None), b"null background")  # also with nothing to do
    refused(call(ctx.h, CL, 4, bg, None, n, G, O, X, None), b"null rays")
    refused(call(ctx.h, CL, 4, bg, R, n, None, O, X, None), b"null rng")
    refused(call(ctx.h, CL, 4, bg, R, n, G, None, X, None), b"null results")
    refused(call(ctx.h, CL, 4, bg, R, n, G, O, None, None), b"null scratch")
    refused(call(ctx.h, CL, 4, bg, R + 2, n, G, O, X, None), b"rays are not aligned")
    refused(call(ctx.h, CL, 4, bg, R, n, G + 4, O, X, None), b"rng states are not aligned")
    refused(call(ctx.h, CL, 4, bg, R, n, G, O + 8, X, None), b"results are not aligned")
    refused(call(ctx.h, CL, 4, bg, R, n, G, O, X + 4, None), b"scratch are not aligned")
    # overlaps, by range: the very buffer, and one that begins in another's last element
    last = lambda base, row: base + (n * row - 1) // 16 * 16  # noqa: E731  (16-byte aligned, inside the last element)
    for dr, dg, do, dx, text in ((R, R, O, X, b"rng states overlap the rays"), (R, last(R, 36), O, X, b"rng states overlap the rays"),
                                 (R, G, R, X, b"results overlap the rays"), (R, G, last(R, 36), X, b"results overlap the rays"),
                                 (R, G, G, X, b"results overlap the rng states"), (R, G, last(G, 8), X, b"results overlap the rng states"),
                                 (R, G, O, R, b"scratch overlap the rays"), (R, G, O, last(R, 36), b"scratch overlap the rays"),
                                 (R, G, O, G, b"scratch overlap the rng states"), (R, G, O, last(G, 8), b"scratch overlap the rng states"),
                                 (R, G, O, O, b"scratch overlap the results"), (R, G, O, last(O, 16), b"scratch overlap the results")):
        refused(call(ctx.h, CL, 4, bg, dr, n, dg, do, dx, None), text)
    assert call(None, CL, 4, bg, R, n, G, O, X, None) != 0
    assert call(ctx.h, CL, 4, bg, None, 0, None, None, None, None) == 0  # n == 0: nothing to check, nothing launched
    fresh = dev.Context(0)
    try:
        refused(call(fresh.h, CL, 4, bg, R, n, G, O, X, None), b"no scene", fresh)
    finally:
        fresh.close()
    with pytest.raises(dev.SrtError, match="neither"):
        ctx.trace_paths_device(torch.zeros((4, 9), dtype=torch.float32, device="cuda"), torch.zeros((4,), dtype=torch.int64, device="cuda"), 4, BG, traversal=5)
    with pytest.raises(ValueError, match="scratch must hold"):
        ctx.trace_paths_device(torch.zeros((4, 9), dtype=torch.float32, device="cuda"), torch.zeros((4,), dtype=torch.int64, device="cuda"), 4, BG,
                               scratch=torch.zeros((63,), dtype=torch.uint8, device="cuda"))
    # updated and not refitted: refused in checkSceneReady's words; then refitted, so that the shared context works again
    tri = RF.scene_triangles(sb)
    ctx.update_triangles(0, tri[:16])
    try:
        refused(call(ctx.h, CL, 4, bg, R, n, G, O, X, None), b"geometry was updated")
    finally:
        ctx.refit()
    # a tree too deep for the LDS of 16 bounces: 120 walk slots + 2 + 3 * 16 KB > 160 KB; 4 bounces fit (test 1 runs them)
    ctx.upload_scene(path_scenes["chain"])
    refused(call(ctx.h, CL, 16, bg, R, n, G, O, X, None), b"of LDS")
    refused(call(ctx.h, abi.SRT_TRAVERSE_FAITHFUL, 13, bg, R, n, G, O, X, None), b"of LDS")
    _assert_same(_trace(dev, abi, ctx, CL, 12, rays, rng0), paths_ref.loop(ctx, abi, rays, rng0, 12, BG, CL), "the deepest that fits")
