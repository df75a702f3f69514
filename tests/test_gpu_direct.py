"""Direct light sampling on device buffers (include/srt_hip.h "Direct light sampling"): srtGetSampledLights,
srtDirectLightDevice, srtTracePathsDirectDevice and the hook srtTestEvalScatterDevice.

Every comparison is ZERO tolerance, on bytes or on uint32 views (NaN by position where a colour may be one).  The checkers:
the hook against srtScatterRaysDevice's own attenuation; the per-hit piece against the NumPy replay of its draws and cone
(tests/direct_ref.py), the hook and srtTraceRaysDevice on its shadow rays; the one-kernel entry against the loop over the
per-hit entries (tests/paths_direct_ref.py) and against srtTracePathsDevice -- never against itself.

Every raw call goes through buffers that are 64 elements longer than n and filled with a sentinel, and the sentinel must
survive; inputs must keep their bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import direct_ref as DR
import direct_scenes as DS
import exact_scenes
import paths_direct_ref
import pathstep_ref as PR
import tree_build_scenes as S
from test_gpu_parity import scenes  # noqa: F401  (the module fixture of the BASELINE scenes)
from test_gpu_pathstep import BUILDERS, PAD, SENTINEL, _bits, _padded, _ray_rows, _rows, _same_floats, _states, step_scenes  # noqa: F401
from test_gpu_paths import BG, _assert_same, _chain_tree, _split
from test_gpu_paths import _trace as _trace_plain

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = (0, 1, 63, 64, 65, 257, 4096)
BOUNCES = (0, 1, 4, 16)


def _traversals(abi):
    return (abi.SRT_TRAVERSE_FAITHFUL, abi.SRT_TRAVERSE_CLOSEST)


@pytest.fixture(scope="module")
def direct_scenes(abi, step_scenes):  # noqa: F811
    out = dict(step_scenes)
    out["room"] = exact_scenes.room(abi, "B")
    out["lights"] = DS.lights(abi)
    for k in (0, 1, 3):
        out["lit%d" % k] = DS.lit(abi, k)
    return out


def _rays_for(abi, which, n):
    if which.startswith("lit") or which == "lights":
        return DS.rays_at(n)
    return _ray_rows(S.random_rays(abi, n))


# ------------------------------------------------------------------------------------------------ raw calls
def _trace_direct(dev, abi, c, traversal, max_bounce, rays, rng0, background=BG):
    """srtTracePathsDirectDevice on sentinel-padded buffers: paths_ref.loop's dict."""
    n = len(rays)
    d_rays, d_rng, d_result = _padded(rays, n, 36), _padded(rng0, n, 8), _padded(None, n, 16)
    d_scratch = _padded(None, 1, abi.SRT_PATHS_SCRATCH_BYTES)
    bg = (C.c_float * 3)(*background)
    rc = dev.lib.srtTracePathsDirectDevice(c.h, traversal, max_bounce, bg, d_rays.data_ptr(), n, d_rng.data_ptr(), d_result.data_ptr(),
                                           d_scratch.data_ptr(), None)
    assert rc == 0, dev.lib.srtLastError(c.h)
    torch.cuda.synchronize()
    assert _rows(d_rays, n, 36).tobytes() == np.ascontiguousarray(rays).tobytes(), "the rays were written"
    scratch = _rows(d_scratch, 1, abi.SRT_PATHS_SCRATCH_BYTES)
    assert n > 0 or (scratch == SENTINEL).all(), "n == 0 launches nothing, the memset included"
    return _split(abi, _rows(d_result, n, 16), _rows(d_rng, n, 8))


def _first_hits(ctx, abi, rays, traversal, bounces=2):
    """Rays and their hit records over the first `bounces` steps of the paths of `rays`, with the states before each step's
    scatter draws: (rays (m, 9), records (m, 22) int32, rng (m,) int64) on the host, and every step's SrtPathOut and
    scattered rays."""
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    d_rng = torch.from_numpy(_states(len(rays), seed=9)).cuda()
    got = {"rays": [], "records": [], "rng": [], "out": [], "rays_out": []}
    for _ in range(bounces):
        _, recs = ctx.trace_device(d_rays, traversal, records=True)
        got["rays"].append(d_rays.cpu().numpy().copy())
        got["rng"].append(d_rng.cpu().numpy().copy())
        out, rays_out = ctx.scatter_device(d_rays, recs, d_rng)
        torch.cuda.synchronize()
        got["records"].append(recs.cpu().numpy().copy())
        got["out"].append(out.cpu().numpy().copy())
        got["rays_out"].append(rays_out.cpu().numpy().copy())
        status = out[:, 3]
        # the next step: the scattered rays; everything else gets an empty interval and misses
        rays_out[:, 8].masked_fill_(status != abi.SRT_PATH_SCATTERED, 0.0)
        rays_out[:, 0:7].masked_fill_((status != abi.SRT_PATH_SCATTERED)[:, None], 1.0)
        d_rays = rays_out.contiguous()
    return {k: np.concatenate(v) for k, v in got.items()}


def _hook(dev, c, rays, records, dirs):
    n = len(rays)
    d_rays, d_recs, d_dirs, d_att = _padded(rays, n, 36), _padded(records, n, 88), _padded(dirs, n, 12), _padded(None, n, 12)
    rc = dev.lib.srtTestEvalScatterDevice(c.h, d_rays.data_ptr(), d_recs.data_ptr(), d_dirs.data_ptr(), n, d_att.data_ptr())
    assert rc == 0, dev.lib.srtLastError(c.h)
    torch.cuda.synchronize()
    for t, rows, size in ((d_rays, rays, 36), (d_recs, records, 88), (d_dirs, dirs, 12)):
        assert _rows(t, n, size).tobytes() == np.ascontiguousarray(rows).tobytes()
    return _rows(d_att, n, 12).view(F).reshape(n, 3)


def _direct(dev, c, traversal, rays, records, rng):
    n = len(rays)
    d_rays, d_recs, d_rng, d_out = _padded(rays, n, 36), _padded(records, n, 88), _padded(rng, n, 8), _padded(None, n, 32)
    rc = dev.lib.srtDirectLightDevice(c.h, traversal, d_rays.data_ptr(), d_recs.data_ptr(), n, d_rng.data_ptr(), d_out.data_ptr(), None)
    assert rc == 0, dev.lib.srtLastError(c.h)
    torch.cuda.synchronize()
    for t, rows, size in ((d_rays, rays, 36), (d_recs, records, 88), (d_rng, rng, 8)):
        assert _rows(t, n, size).tobytes() == np.ascontiguousarray(rows).tobytes(), "an input was written"
    return _rows(d_out, n, 32)


# ------------------------------------------------------------------------------------------------ 1. hook = scatter
def _assert_hook_is_scatter(ctx, dev, abi, sb, rays, what, want_normal_map=False):
    h = _first_hits(ctx, abi, rays, abi.SRT_TRAVERSE_FAITHFUL)
    out = h["out"].view(abi.PATH_OUT_DTYPE).reshape(-1)
    rec = h["records"].view(abi.HIT_DTYPE).reshape(-1)
    pbr = np.zeros(len(sb.materials) + 1, bool)
    pbr[DS.pbr_materials(sb)] = True
    is_pbr = (rec["prim"] >= 0) & pbr[np.clip(rec["material"], 0, len(sb.materials))]
    assert is_pbr.sum() >= 100 and not is_pbr.all(), what  # (misses, and on most scenes hits on other materials: they get 0)
    assert (out["status"][is_pbr] == abi.SRT_PATH_SCATTERED).all()
    if want_normal_map:
        mapped = np.zeros(len(sb.materials) + 1, bool)
        mapped[DS.pbr_materials(sb, normal_mapped=True)] = True
        assert (is_pbr & mapped[np.clip(rec["material"], 0, len(sb.materials))]).sum() >= 50, what
    dirs = np.ascontiguousarray(h["rays_out"][:, 3:6])
    dirs[~is_pbr] = (0.0, 1.0, 0.0)  # (what torch.empty left is no direction)
    for n in sorted(set(SIZES) | {len(rays)}):
        att = _hook(dev, ctx, h["rays"][:n], h["records"][:n], dirs[:n])
        sel = is_pbr[:n]
        _same_floats(att[sel], out["attenuation"][:n][sel], (what, n))
        assert not _bits(att[~sel]).any(), (what, n, "not pbr: 0")
    w = ctx.eval_scatter_test(torch.from_numpy(h["rays"]).cuda(), torch.from_numpy(h["records"]).cuda(), torch.from_numpy(dirs).cuda())
    torch.cuda.synchronize()
    _same_floats(w.cpu().numpy()[is_pbr], out["attenuation"][is_pbr], (what, "wrapper"))


@pytest.mark.parametrize("seed", [0, 1, 2, 4])
def test_hook_is_scatters_attenuation_on_exact_scenes(ctx, dev, abi, seed):
    sb = exact_scenes.random(abi, seed, "B")
    ctx.upload_scene(sb)
    _assert_hook_is_scatter(ctx, dev, abi, sb, _ray_rows(S.random_rays(abi, 4096)), ("tierB", seed))


@pytest.mark.parametrize("name", ["iron", "masterchief"])
def test_hook_is_scatters_attenuation_on_textured_scenes(ctx, dev, abi, camera, scenes, name):  # noqa: F811
    sb = scenes[name]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    rays, _ = ctx.camera_rays_device(abi.default_render_params(80, 52, 1, 1, seed=3))
    torch.cuda.synchronize()
    _assert_hook_is_scatter(ctx, dev, abi, sb, rays.cpu().numpy()[:4096], name, want_normal_map=(name == "iron"))
    kinds = {sb.textures[sb.materials[m].albedoTex].kind for m in DS.pbr_materials(sb) if sb.materials[m].albedoTex >= 0}
    assert (abi.SRT_TEX_IMAGE in kinds) if name == "masterchief" else True


# ------------------------------------------------------------------------------------------------ 2. direct piece = replay
@pytest.mark.parametrize("which", ["lit0", "lit1", "lit3", "lights"])
def test_direct_piece_is_the_replay(ctx, dev, abi, direct_scenes, which):
    sb = direct_scenes[which]
    ctx.upload_scene(sb)
    table = DS.light_table(sb)
    K = len(table)
    assert K == {"lit0": 0, "lit1": 1, "lit3": 3, "lights": 5}[which]
    assert ctx.sampled_lights().tolist() == [t[0] for t in table]
    h = _first_hits(ctx, abi, DS.rays_at(2048), abi.SRT_TRAVERSE_CLOSEST)
    rec = h["records"].view(abi.HIT_DTYPE).reshape(-1)
    pbr = np.zeros(len(sb.materials) + 1, bool)
    pbr[DS.pbr_materials(sb, normal_mapped=False)] = True
    is_pbr = (rec["prim"] >= 0) & pbr[np.clip(rec["material"], 0, len(sb.materials))]
    assert is_pbr.sum() >= 500 and (rec["prim"] < 0).any() and (~is_pbr & (rec["prim"] >= 0)).any()
    m = len(rec)
    assert m == 4096
    lights = [(c, r, moving) for _, c, r, moving in table]
    want = np.zeros(m, abi.DIRECT_OUT_DTYPE)
    want["light"] = -1
    if K:
        for i in np.flatnonzero(is_pbr):
            s = DR.sample(PR.from_int64(h["rng"][i]), rec["p"][i], rec["normal"][i], lights)
            want["light"][i] = table[s["light"]][0] if s["light"] >= 0 else -1
            want["dir"][i], want["weight"][i] = s["dir"], s["weight"]
    for traversal in _traversals(abi):
        got = _direct(dev, ctx, traversal, h["rays"], h["records"], h["rng"]).view(abi.DIRECT_OUT_DTYPE).reshape(-1)
        assert got["light"].tolist() == want["light"].tolist(), (which, traversal)
        _same_floats(got["dir"], want["dir"], (which, traversal, "dir"))
        _same_floats(got["weight"], want["weight"], (which, traversal, "weight"))
        # the radiance: the hook at the sampled direction, times the light's colour, times the weight -- where the shadow
        # ray's own query returns the light; an exact 0 elsewhere
        chosen = got["light"] >= 0
        shadow = h["rays"].copy()
        shadow[:, 0:3], shadow[:, 3:6] = rec["p"], got["dir"]
        shadow[~chosen, 8] = 0.0
        hits = ctx.trace_device(torch.from_numpy(shadow).cuda(), traversal).cpu().numpy()
        visible = chosen & (hits[:, 0] == got["light"])
        att = _hook(dev, ctx, h["rays"], h["records"], np.ascontiguousarray(got["dir"]))
        colour = np.zeros((m, 3), F)
        for i in np.flatnonzero(visible):
            colour[i] = DS.light_colour(sb, int(got["light"][i]))
        with np.errstate(all="ignore"):
            radiance = np.where(visible[:, None], (att * colour) * got["weight"][:, None], F(0.0)).astype(F)
        _same_floats(got["radiance"], radiance, (which, traversal, "radiance"))
        assert not _bits(got["radiance"][~visible]).any()
        if K == 0:
            assert not got.view(np.int32).reshape(m, 8)[:, [0, 1, 2, 4, 5, 6, 7]].any() and (got["light"] == -1).all()
            continue
        # the cases are there: lit and shadowed terms, lights below the horizon, and in `lights` the unsampled choices
        assert (visible & (got["radiance"] > 0).any(axis=1)).sum() >= 50, which
        assert (chosen & ~visible).sum() >= 20 and (chosen & (got["weight"] == 0)).any(), which
        # every static light is chosen somewhere, the moving one never; the enclosing one only from the ground beyond it
        static = {t[0] for t in table if not t[3] and t[0] != getattr(sb, "enclosing", -2)}
        assert static <= set(got["light"][chosen].tolist()) <= static | {getattr(sb, "enclosing", -2)}
        far = got["light"] == getattr(sb, "enclosing", -2)
        assert (np.linalg.norm(rec["p"][far].astype(np.float64), axis=1) > 30.0).all()
        if which == "lights":
            assert (is_pbr & ~chosen).sum() >= 100  # the moving and the enclosing light were chosen: nothing sampled
        # every prefix: an entry depends on its own ray, record and state alone
        for n in SIZES:
            part = _direct(dev, ctx, traversal, h["rays"][:n], h["records"][:n], h["rng"][:n])
            assert part.tobytes() == got[:n].tobytes(), (which, traversal, n)
    w = ctx.direct_light_device(torch.from_numpy(h["rays"]).cuda(), torch.from_numpy(h["records"]).cuda(), torch.from_numpy(h["rng"]).cuda(),
                                abi.SRT_TRAVERSE_CLOSEST)
    torch.cuda.synchronize()
    assert tuple(w.shape) == (m, 8) and w.dtype == torch.int32 and w.cpu().numpy().tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------ 3. whole = loop
@pytest.mark.parametrize("which", ["tierB"] + list(BUILDERS) + ["room", "lights", "lit3"])
def test_whole_path_is_the_loop_over_the_pieces(ctx, dev, abi, direct_scenes, which):
    sb = direct_scenes[which]
    ctx.upload_scene(sb)
    K = len(ctx.sampled_lights())
    rays = _rays_for(abi, which, max(SIZES))
    rng0 = _states(len(rays))
    for traversal in _traversals(abi):
        for max_bounce in BOUNCES:
            cases = {}
            want = paths_direct_ref.loop(ctx, abi, sb, rays, rng0, max_bounce, BG, traversal, cases=cases)
            if which == "lights" and max_bounce >= 4:  # on the REFERENCE loop alone: each case occurs
                assert K == 5
                for case in ("dropped", "kept: camera ray or not after pbr", "kept: moving", "kept: inside", "kept: not in S", "term > 0",
                             "term 0: shadowed or below the horizon", "nothing sampled"):
                    assert cases[case] > 0, (case, cases)
            if which == "lit3" and max_bounce >= 4:
                assert cases["dropped"] > 0 and cases["term > 0"] > 100, cases
            for n in SIZES:
                got = _trace_direct(dev, abi, ctx, traversal, max_bounce, rays[:n], rng0[:n])
                _assert_same(got, {k: v[:n] for k, v in want.items()}, (which, traversal, max_bounce, n))
    w_rng = torch.from_numpy(rng0.copy()).cuda()
    w = ctx.trace_paths_device(torch.from_numpy(rays.copy()).cuda(), w_rng, 4, BG, abi.SRT_TRAVERSE_CLOSEST, direct=True)
    torch.cuda.synchronize()
    _assert_same(_split(abi, w.cpu().numpy().view(np.uint8), w_rng.cpu().numpy().view(np.uint8)),
                 paths_direct_ref.loop(ctx, abi, sb, rays, rng0, 4, BG, abi.SRT_TRAVERSE_CLOSEST), (which, "wrapper"))


# ------------------------------------------------------------------------------------------------ 4. properties
@pytest.mark.parametrize("which", ["tierB"] + list(BUILDERS) + ["room", "lights", "lit0", "lit1", "lit3"])
def test_paths_are_the_plain_entrys(ctx, dev, abi, direct_scenes, which):
    """steps, status and the final generator state are srtTracePathsDevice's; with K = 0 so is every byte of the radiance."""
    ctx.upload_scene(direct_scenes[which])
    K = len(ctx.sampled_lights())
    rays = _rays_for(abi, which, 4096)
    rng0 = _states(len(rays))
    differs = False
    for traversal in _traversals(abi):
        for max_bounce in BOUNCES:
            plain = _trace_plain(dev, abi, ctx, traversal, max_bounce, rays, rng0)
            got = _trace_direct(dev, abi, ctx, traversal, max_bounce, rays, rng0)
            for key in ("steps", "status", "rng"):
                assert got[key].tobytes() == plain[key].tobytes(), (which, traversal, max_bounce, key)
            if K == 0:
                _same_floats(got["radiance"], plain["radiance"], (which, traversal, max_bounce))
            else:
                differs = differs or got["radiance"].tobytes() != plain["radiance"].tobytes()
    assert K > 0 or not differs
    if which in ("room", "lights", "lit1", "lit3"):  # lights over pbr surfaces: the term is there
        assert K > 0 and differs, (which, K)


def test_a_moved_light_is_followed(ctx, dev, abi, direct_scenes):
    sb = direct_scenes["lit3"]
    ctx.upload_scene(sb)
    rays, rng0 = DS.rays_at(4096), _states(4096)
    CL = abi.SRT_TRAVERSE_CLOSEST
    before = _trace_direct(dev, abi, ctx, CL, 4, rays, rng0)
    spheres = DS.sphere_records(sb)
    first = DS.sphere_of_prim(sb)[ctx.sampled_lights()[0]]
    spheres["center0"][first] += F(1.5)
    spheres["center1"][first] = spheres["center0"][first]
    spheres["radius"][first] = 1.4
    try:
        ctx.update_spheres(first, spheres[first:first + 1])
        ctx.refit()
        refit = _trace_direct(dev, abi, ctx, CL, 4, rays, rng0)
        assert refit["radiance"].tobytes() != before["radiance"].tobytes()
        _assert_same(refit, paths_direct_ref.loop(ctx, abi, sb, rays, rng0, 4, BG, CL, spheres=spheres), "refit = the loop with the moved table")
        ctx.rebuild()
        rebuilt = _trace_direct(dev, abi, ctx, CL, 4, rays, rng0)
        # a fresh upload of the moved scene
        moved = DS.lit(abi, 3)
        s = moved.spheres[first]
        s.center0[:] = tuple(spheres["center0"][first])
        s.center1[:] = tuple(spheres["center1"][first])
        s.radius = float(spheres["radius"][first])
        ctx.upload_scene(moved)
        fresh = _trace_direct(dev, abi, ctx, CL, 4, rays, rng0)
        _assert_same(refit, fresh, "refit = fresh upload")
        _assert_same(rebuilt, fresh, "rebuild = fresh upload")
    finally:
        ctx.upload_scene(sb)


def test_refusals_launch_nothing(ctx, dev, abi, direct_scenes):
    ctx.upload_scene(direct_scenes["lit3"])
    n = 512
    rays, rng0 = DS.rays_at(n), _states(n)
    h = _first_hits(ctx, abi, rays, abi.SRT_TRAVERSE_CLOSEST, bounces=1)
    d_rays, d_recs, d_rng = _padded(rays, n, 36), _padded(h["records"], n, 88), _padded(rng0, n, 8)
    outs = {"result": _padded(None, n, 16), "direct": _padded(None, n, 32), "scratch": _padded(None, 1, abi.SRT_PATHS_SCRATCH_BYTES)}
    R, H, G, O, D, X = (t.data_ptr() for t in (d_rays, d_recs, d_rng, outs["result"], outs["direct"], outs["scratch"]))
    CL, bg = abi.SRT_TRAVERSE_CLOSEST, (C.c_float * 3)(*BG)
    paths, direct = dev.lib.srtTracePathsDirectDevice, dev.lib.srtDirectLightDevice

    def refused(rc, text, c=ctx):
        assert rc != 0 and text in dev.lib.srtLastError(c.h), (rc, text, dev.lib.srtLastError(c.h))
        torch.cuda.synchronize()
        for buf in outs.values():
            assert bool((buf == SENTINEL).all())
        assert d_rng.cpu().numpy()[:n * 8].tobytes() == rng0.tobytes()

    refused(paths(ctx.h, CL, 4, bg, R, -1, G, O, X, None), b"srtTracePathsDirectDevice: n = -1 is negative")
    refused(paths(ctx.h, 5, 4, bg, R, n, G, O, X, None), b"neither")
    refused(paths(ctx.h, CL, 17, bg, R, n, G, O, X, None), b"maxBounce")
    refused(paths(ctx.h, CL, 4, None, R, n, G, O, X, None), b"null background")
    refused(paths(ctx.h, CL, 4, bg, None, n, G, O, X, None), b"null rays")
    refused(paths(ctx.h, CL, 4, bg, R, n, None, O, X, None), b"null rng")
    refused(paths(ctx.h, CL, 4, bg, R, n, G, None, X, None), b"null results")
    refused(paths(ctx.h, CL, 4, bg, R, n, G, O, None, None), b"null scratch")
    refused(paths(ctx.h, CL, 4, bg, R, n, G, O + 8, X, None), b"results are not aligned")
    refused(paths(ctx.h, CL, 4, bg, R, n, G, R, X, None), b"results overlap the rays")
    refused(paths(ctx.h, CL, 4, bg, R, n, G, G, X, None), b"results overlap the rng states")
    refused(paths(ctx.h, CL, 4, bg, R, n, G, O, G, None), b"scratch overlap the rng states")
    refused(direct(ctx.h, CL, R, H, -1, G, D, None), b"srtDirectLightDevice: n = -1 is negative")
    refused(direct(ctx.h, 7, R, H, n, G, D, None), b"neither")
    refused(direct(ctx.h, CL, None, H, n, G, D, None), b"null rays")
    refused(direct(ctx.h, CL, R, None, n, G, D, None), b"null records")
    refused(direct(ctx.h, CL, R, H, n, None, D, None), b"null rng")
    refused(direct(ctx.h, CL, R, H, n, G, None, None), b"null direct")
    refused(direct(ctx.h, CL, R + 2, H, n, G, D, None), b"rays are not aligned")
    refused(direct(ctx.h, CL, R, H, n, G + 4, D, None), b"rng states are not aligned")
    refused(direct(ctx.h, CL, R, H, n, G, D + 8, None), b"direct terms are not aligned")
    refused(direct(ctx.h, CL, R, H, n, G, R, None), b"direct terms overlap the rays")
    refused(direct(ctx.h, CL, R, H, n, G, H, None), b"direct terms overlap the records")
    refused(direct(ctx.h, CL, R, H, n, G, G, None), b"direct terms overlap the rng states")
    assert paths(ctx.h, CL, 4, bg, None, 0, None, None, None, None) == 0 and direct(ctx.h, CL, None, None, 0, None, None, None) == 0
    assert paths(None, CL, 4, bg, R, n, G, O, X, None) != 0 and direct(None, CL, R, H, n, G, D, None) != 0
    count = C.c_int32(-7)
    assert dev.lib.srtGetSampledLights(ctx.h, None, 0, C.byref(count)) == 0 and count.value == 3
    small = (C.c_int32 * 2)(-1, -1)
    assert dev.lib.srtGetSampledLights(ctx.h, small, 2, C.byref(count)) != 0 and b"capacity" in dev.lib.srtLastError(ctx.h)
    assert list(small) == [-1, -1]
    assert dev.lib.srtGetSampledLights(ctx.h, None, 0, None) != 0 and b"null count" in dev.lib.srtLastError(ctx.h)
    fresh = dev.Context(0)
    try:
        refused(paths(fresh.h, CL, 4, bg, R, n, G, O, X, None), b"no scene", fresh)
        refused(direct(fresh.h, CL, R, H, n, G, D, None), b"no scene", fresh)
        assert dev.lib.srtGetSampledLights(fresh.h, None, 0, C.byref(count)) != 0 and b"no scene" in dev.lib.srtLastError(fresh.h)
    finally:
        fresh.close()
    # the LDS limit: the chain's walk stack is 122 KB; 6 KB per bounce beside it: 6 bounces fit, 7 do not (the plain entry takes 12)
    ctx.upload_scene(_chain_tree(abi))
    refused(paths(ctx.h, CL, 7, bg, R, n, G, O, X, None), b"of LDS")
    refused(paths(ctx.h, abi.SRT_TRAVERSE_FAITHFUL, 12, bg, R, n, G, O, X, None), b"of LDS")
    chain_rays = _ray_rows(S.random_rays(abi, n))
    got = _trace_direct(dev, abi, ctx, CL, 6, chain_rays, rng0)
    plain = _trace_plain(dev, abi, ctx, CL, 6, chain_rays, rng0)
    for key in ("steps", "status", "rng"):
        assert got[key].tobytes() == plain[key].tobytes(), key
