"""The temporal-adaptive frame on the GPU (include/srt_hip.h srtTemporalReproject / srtRenderTemporalAdaptive /
srtRenderTemporalAdaptiveFrame, csrc/srt_temporal_adaptive.hip): the reprojected history and whole frames bit for bit
against tests/temporal_adaptive_ref.py over 3-frame orbits, the outputs against srtTemporalAccumulate, the degenerate
thresholds against the existing entries, where the samples go, interleaving with uniform temporal frames, errors and side
effects, the C++ example, and the band error against a uniform temporal frame of at least as many samples.

Nothing is compared with a tolerance: every value is float32 + - * / sqrt, rint, floor and comparisons, and the decisions
are the double test of adaptive_ref.converged."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import adaptive_ref as A
import temporal_adaptive_ref as TA
import temporal_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
INF = float("inf")
W, H, SPP, SPP_MAX = 97, 61, 4, 32  # edge tiles on both axes: 13 x 8 tiles
ORBIT = (0.0, 2.0, 4.5)
TUNABLES = ("tile_block", "unit_tiles", "queues", "lds_tree", "wavefront", "wf_pool", "chunk_scratch_mb", "wf_resident_max")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    """bit-identical, NaNs of any payload counted equal"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint32) == b.view(np.uint32))))


def _h(t):
    return t.cpu().numpy()


def _orbit_camera(dev, abi, degrees):
    """examples/main.cpp --orbit: the default eye turned about the vertical axis through the lookAt point."""
    c = abi.default_camera_params()
    a = np.deg2rad(np.float64(degrees))
    dx, dz = F(c.eye[0] - c.lookAt[0]), F(c.eye[2] - c.lookAt[2])
    co, si = F(np.cos(a)), F(np.sin(a))
    c.eye[0] = F(c.lookAt[0]) + (co * dx + si * dz)
    c.eye[2] = F(c.lookAt[2]) + (co * dz - si * dx)
    return dev.make_camera(c)


def _scene(srt, name):
    return {"spheres": srt.scenes.scene_spheres, "masterchief": srt.scenes.scene_masterchief}[name]()


def _params(abi, k, w=W, h=H, seed=7):
    return abi.default_render_params(w, h, SPP, 4, seed=seed, spp_chunks=0, sample_first=k * SPP_MAX)


def _feature_planes(ctx, dev, abi, p):
    """The resolved feature planes of p's samples, [albedo, normal, position, depth] as (H, W, 4) cuda tensors."""
    import torch
    w, h = p.imageWidth, p.imageHeight
    tiles = [torch.zeros((dev.num_local_tiles(w, h, 1), 64, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    ctx.render_feature_tiles(p, abi.SRT_FEATURE_ALL, [t.data_ptr() for t in tiles], None)
    img = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    for k in range(4):
        ctx.resolve_tiles(p, tiles[k].data_ptr(), None, img[k].data_ptr(), None)
    torch.cuda.synchronize()
    return img


def _tp(abi, dm, cap, ncos=0.0, pdist=0.0):
    return abi.default_temporal_params(ncos, pdist, cap, dm), dict(normal_cos=ncos, plane_dist=pdist, max_history=cap, demodulate=dm)


def _device_frame(ctx, p, ap, t, planes, prev, hist, fill=float("nan")):
    """srtRenderTemporalAdaptive into fresh device buffers.  Returns a dict of cuda tensors and the stats."""
    import torch
    h, w = p.imageHeight, p.imageWidth
    out = {k: torch.full((h, w, 4), fill, dtype=torch.float32, device="cuda") for k in ("accum", "moments", "beauty_out", "moments_out")}
    out["history_out"] = torch.full((3, h, w, 4), fill, dtype=torch.float32, device="cuda")
    ptrs = [q.data_ptr() if (k or t.demodulate) else None for k, q in enumerate(planes)]
    out["stats"] = ctx.render_temporal_adaptive_device(p, ap, t, ptrs, prev, hist.data_ptr() if hist is not None else None,
                                                       out["accum"].data_ptr(), out["moments"].data_ptr(), out["beauty_out"].data_ptr(),
                                                       out["moments_out"].data_ptr(), out["history_out"].data_ptr(), None)
    return out


def _tile_counts(accum):
    """(tilesY, tilesX): a tile's current count (every pixel of a tile has the same)."""
    n = accum[..., 3]
    h, w = n.shape
    ty, tx = -(-h // 8), -(-w // 8)
    pad = np.full((ty * 8, tx * 8), np.nan, F)
    pad[:h, :w] = n
    t = pad.reshape(ty, 8, tx, 8)
    assert (np.nanmin(t, axis=(1, 3)) == np.nanmax(t, axis=(1, 3))).all()
    return np.nanmax(t, axis=(1, 3))


def _tiles_with(mask):
    """(tilesY, tilesX) bool: tiles with at least one in-image pixel of `mask`."""
    return A.tile_open(~mask)


# thresholds (display units) between the pooled errors of settled tiles and the own errors of fresh ones: chosen on the
# emulation so that the frames after the first stop some tiles at SPP, take some to SPP_MAX and launch part of the frame
# in launch 1 -- which test_frames_match_the_emulation asserts
CASES = [  # scene, demodulate, maxHistory, threshold
    ("spheres", 0, 64.0, 0.02),
    ("masterchief", 1, INF, 0.04),
]
IDS = ["%s-dm%d-cap%s" % c[:3] for c in CASES]


@pytest.fixture(scope="module")
def orbits(ctx, dev, abi, srt):
    """Each case's 3-frame orbit through srtRenderTemporalAdaptive, the emulation alongside on its own chain, computed once
    and left unchanged: per frame the device outputs (host copies), the emulation, the planes, the cameras and the history
    that went in."""
    out = {}
    for name, dm, cap, thr in CASES:
        ctx.upload_scene(_scene(srt, name))
        t, tp = _tp(abi, dm, cap)
        ap = abi.default_adaptive_params(SPP_MAX, thr)
        hist_gpu = hist_ref = prev = None
        frames = []
        for k, deg in enumerate(ORBIT):
            cam = _orbit_camera(dev, abi, deg)
            ctx.set_camera(cam)
            p = _params(abi, k)
            planes = _feature_planes(ctx, dev, abi, p)
            got = _device_frame(ctx, p, ap, t, planes, prev, hist_gpu)
            hplanes = [_h(q) for q in planes]
            want = TA.emulate_frame(ctx, p, SPP_MAX, thr, hplanes, cam, prev, hist_ref, tp)
            frames.append(dict(p=p, cam=cam, prev=prev, planes=planes, hplanes=hplanes, hist_in=hist_gpu, hist_in_ref=hist_ref,
                               got={k2: (_h(v) if k2 != "stats" else v) for k2, v in got.items()}, want=want, t=t, tp=tp, ap=ap))
            hist_gpu, hist_ref, prev = got["history_out"], want["history_out"], cam
        out[(name, dm, cap)] = frames
    return out


# ------------------------------------------------------------------ 1. the reprojected history


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reprojection_matches_reference(ctx, dev, abi, orbits, case):
    import torch
    frames = orbits[case[:3]]
    for k, f in enumerate(frames):
        rp = torch.full((2, H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        ptrs = [q.data_ptr() if (j or f["t"].demodulate) else None for j, q in enumerate(f["planes"])]
        ctx.temporal_reproject(f["t"], W, H, ptrs, f["cam"], f["prev"], f["hist_in"].data_ptr() if k else None, rp.data_ptr(), None)
        torch.cuda.synchronize()
        hist = _h(f["hist_in"]) if k else None
        want = TA.reproject_history(f["hplanes"][1], f["hplanes"][2], f["hplanes"][3], f["cam"], f["prev"], hist,
                                    f["tp"]["normal_cos"], f["tp"]["plane_dist"], f["tp"]["max_history"])
        diff = _bits(_h(rp)) != _bits(want)
        assert not diff.any(), (case[:3], k, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        has = want[1][..., 3] != 0
        if k:
            assert has.any() and (~has).any(), (k, has.mean())  # a moved camera: reuse and disocclusion
            assert (want[0][..., 3][has] > 0).all() and (want[:, ~has] == 0).all()
        else:
            assert (want == 0).all()  # no history: zeros
    # an unmoved camera: every pixel's own record, whatever the geometry tests would say
    f = frames[2]
    hist = _h(f["hist_in"])
    rp = torch.full((2, H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    ptrs = [q.data_ptr() if (j or f["t"].demodulate) else None for j, q in enumerate(f["planes"])]
    ctx.temporal_reproject(abi.default_temporal_params(max_history=INF, demodulate=f["t"].demodulate), W, H, ptrs, f["cam"], f["cam"],
                           f["hist_in"].data_ptr(), rp.data_ptr(), None)
    torch.cuda.synchronize()
    got = _h(rp)
    own = np.isfinite(hist[0][..., 3]) & (hist[0][..., 3] > 0)
    assert own.mean() > 0.99 and np.array_equal(got[1][..., 3] != 0, own)
    assert np.array_equal(_bits(got[0][own]), _bits(hist[0][own]))
    assert np.array_equal(_bits(got[1][..., 0][own]), _bits(hist[1][..., 3][own]))
    assert np.array_equal(_bits(got[1][..., 1][own]), _bits(hist[2][..., 3][own]))


# ------------------------------------------------------------------ 2. whole frames against the emulation


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_frames_match_the_emulation(dev, abi, orbits, case):
    tiles = dev.num_tiles(W, H)
    for k, f in enumerate(orbits[case[:3]]):
        got, want, st = f["got"], f["want"], f["got"]["stats"]
        label = (case[:3], k)
        print("%s frame %d: tiles per launch %s, %.2f samples per pixel, history on %.0f%% of the pixels" % (
            case[0], k, st["roundTiles"], st["pixelSamples"] / (W * H), 100.0 * want["has"].mean()))
        assert st["roundTiles"] == want["counts"], (label, st["roundTiles"], want["counts"])
        assert st["roundSpp"] == A.schedule(SPP, SPP_MAX)[:len(want["counts"])]
        assert st["pixelSamples"] == want["pixel_samples"] == int(got["accum"][..., 3].astype(np.int64).sum())
        for what in ("accum", "moments", "beauty_out", "moments_out", "history_out"):
            assert _same(got[what], want[what]), (label, what)
        assert st["historyPixels"] == int((want["beauty_out"][..., 3] > want["accum"][..., 3]).sum())
        assert st["meanHistoryCount"] == pytest.approx(float(want["history_out"][0][..., 3].astype(np.float64).mean()), rel=1e-12)
        if k:  # the schedule is not a trivial one
            counts = _tile_counts(want["accum"])
            assert 0 < want["counts"][1] < tiles, (label, want["counts"])
            assert (counts == SPP).any() and (counts == SPP_MAX).any(), (label, np.unique(counts))


# ------------------------------------------------------------------ 3. the outputs are srtTemporalAccumulate of the sums


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_outputs_are_the_accumulation_of_the_returned_sums(ctx, orbits, case):
    import torch
    for k, f in enumerate(orbits[case[:3]]):
        acc, mom = (torch.from_numpy(f["got"][w]).cuda() for w in ("accum", "moments"))
        out_b, out_m = (torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
        new = torch.full((3, H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        ptrs = [q.data_ptr() if (j or f["t"].demodulate) else None for j, q in enumerate(f["planes"])]
        ctx.temporal_accumulate(f["t"], W, H, acc.data_ptr(), mom.data_ptr(), ptrs, f["cam"], f["prev"],
                                f["hist_in"].data_ptr() if k else None, out_b.data_ptr(), out_m.data_ptr(), new.data_ptr(), None)
        torch.cuda.synchronize()
        assert _same(f["got"]["beauty_out"], _h(out_b)) and _same(f["got"]["moments_out"], _h(out_m))
        assert _same(f["got"]["history_out"], _h(new))


# ------------------------------------------------------------------ 4. the degenerate thresholds


def test_infinite_threshold_is_the_uniform_temporal_frame(ctx, dev, abi, srt):
    ctx.upload_scene(_scene(srt, "masterchief"))
    d, t = abi.default_denoise_params(), abi.default_temporal_params()
    ap = abi.default_adaptive_params(SPP_MAX, INF)
    runs = []
    for adaptive in (True, False):
        ctx.temporal_reset()
        frames = []
        for k, deg in enumerate(ORBIT):
            ctx.set_camera(_orbit_camera(dev, abi, deg))
            p = _params(abi, k)
            frames.append(ctx.render_temporal_adaptive_frame(p, ap, d, t) if adaptive else ctx.render_temporal_frame(p, d, t))
        runs.append(frames)
    for k, (a, u) in enumerate(zip(*runs)):
        assert _same(a[0], u[0]) and _same(a[1], u[1]) and np.array_equal(a[2], u[2]), k
        assert a[3]["rounds"] == 1 and a[3]["roundTiles"] == [dev.num_tiles(W, H)] and a[3]["pixelSamples"] == W * H * SPP
        assert (a[3]["historyPixels"], a[3]["meanHistoryCount"]) == (u[3]["historyPixels"], u[3]["meanHistoryCount"])
    # sppMax == spp is the same frame whatever the threshold
    ctx.temporal_reset()
    ctx.set_camera(_orbit_camera(dev, abi, ORBIT[0]))
    a = ctx.render_temporal_adaptive_frame(_params(abi, 0), abi.default_adaptive_params(SPP, 0.0), d, t)
    assert _same(a[0], runs[1][0][0]) and _same(a[1], runs[1][0][1]) and a[3]["rounds"] == 1
    ctx.temporal_reset()


def test_first_frame_after_a_reset_is_the_adaptive_render_denoised(ctx, dev, abi, srt, camera):
    import torch
    ctx.upload_scene(_scene(srt, "masterchief"))
    ctx.set_camera(camera)
    p = _params(abi, 0)
    ap = abi.default_adaptive_params(SPP_MAX, 0.04)
    d = abi.default_denoise_params()
    ctx.temporal_reset()
    acc, den, rgba, st = ctx.render_temporal_adaptive_frame(p, ap, d)
    beauty, moments = (torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    st2 = ctx.render_adaptive_device(p, ap, beauty.data_ptr(), moments.data_ptr(), None, None)
    assert _same(acc, _h(beauty)) and st["roundTiles"] == st2["roundTiles"] and st["pixelSamples"] == st2["pixelSamples"]
    assert st["rounds"] > 1 and st["historyPixels"] == 0
    planes = _feature_planes(ctx, dev, abi, p)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.denoise(d, W, H, beauty.data_ptr(), [None, planes[1].data_ptr(), None, planes[3].data_ptr()], out.data_ptr(), out8.data_ptr(),
                None, d_moments_ptr=moments.data_ptr())
    torch.cuda.synchronize()
    assert _same(den, _h(out)) and np.array_equal(rgba, _h(out8))
    ctx.temporal_reset()


def test_null_history_is_the_adaptive_render(ctx, dev, abi, srt, orbits):
    """Frame 0 of every orbit had no history: srtRenderAdaptive's sums and tile counts, bit for bit."""
    import torch
    for key, frames in orbits.items():
        f = frames[0]
        ctx.upload_scene(_scene(srt, key[0]))
        ctx.set_camera(f["cam"])
        beauty, moments = (torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        st = ctx.render_adaptive_device(f["p"], f["ap"], beauty.data_ptr(), moments.data_ptr(), None, None)
        assert _same(f["got"]["accum"], _h(beauty)) and _same(f["got"]["moments"], _h(moments))
        assert f["got"]["stats"]["roundTiles"] == st["roundTiles"] and st["rounds"] > 1
        assert _same(f["got"]["beauty_out"], _h(beauty)) and _same(f["got"]["moments_out"], _h(moments))


# ------------------------------------------------------------------ 5. where the samples go


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_disoccluded_tiles_get_the_samples(ctx, abi, srt, orbits, case):
    thr = case[3]
    second_step = sum(A.schedule(SPP, SPP_MAX)[:2])
    for k, f in enumerate(orbits[case[:3]]):
        if not k:
            continue
        want, got = f["want"], f["got"]
        fresh = _tiles_with(~want["has"])  # tiles with an in-image pixel that has no history
        assert fresh.any() and (~fresh).any(), (case[:3], k)  # the orbit and threshold produce both kinds (in the emulation)
        counts = _tile_counts(got["accum"])
        # a fresh tile was launched again unless every pixel of it had converged after round 0; for its pixels without
        # history that is a statement about their own round-0 moments
        ctx.upload_scene(_scene(srt, case[0]))
        ctx.set_camera(f["cam"])
        _, m0, _ = ctx.render_image_moments(f["p"], want_rgba=False)
        own_open = _tiles_with(~want["has"] & ~A.converged(m0, thr))
        assert (counts[own_open] >= second_step).all(), (case[:3], k)
        assert own_open.any()
        mean_fresh, mean_rest = float(counts[fresh].mean()), float(counts[~fresh].mean())
        print("%s frame %d: %d fresh tiles at %.2f samples, %d others at %.2f" % (case[0], k, fresh.sum(), mean_fresh, (~fresh).sum(),
                                                                                   mean_rest))
        assert mean_fresh > mean_rest


# ------------------------------------------------------------------ 6. interleaving, state, errors, the example


def test_uniform_and_adaptive_frames_share_the_history(ctx, dev, abi, srt):
    ctx.upload_scene(_scene(srt, "spheres"))
    d, t = abi.default_denoise_params(), abi.default_temporal_params()
    tp = dict(normal_cos=0.0, plane_dist=0.0, max_history=0.0, demodulate=0)
    thr = 0.02
    ap = abi.default_adaptive_params(SPP_MAX, thr)
    cams = [_orbit_camera(dev, abi, deg) for deg in ORBIT]
    ctx.temporal_reset()
    ctx.set_camera(cams[0])
    p0 = _params(abi, 0)
    acc0, _, _, _ = ctx.render_temporal_frame(p0, d, t)  # a uniform frame leaves the history ...
    _, m0, _ = ctx.render_image_moments(p0, want_rgba=False)
    pl0 = [_h(q) for q in _feature_planes(ctx, dev, abi, p0)]
    _, _, hist0 = R.accumulate(acc0, m0, pl0[1], pl0[2], pl0[3], None, cams[0], None, None)
    ctx.set_camera(cams[1])
    p1 = _params(abi, 1)
    acc1, den1, _, st1 = ctx.render_temporal_adaptive_frame(p1, ap, d, t)  # ... an adaptive frame uses and replaces it ...
    pl1 = [_h(q) for q in _feature_planes(ctx, dev, abi, p1)]
    want = TA.emulate_frame(ctx, p1, SPP_MAX, thr, pl1, cams[1], cams[0], hist0, tp)
    assert _same(acc1, want["accum"]) and st1["roundTiles"] == want["counts"] and st1["historyPixels"] > 0.5 * W * H
    assert np.array_equal(den1[..., 3], want["beauty_out"][..., 3])  # the denoised frame's w is the accumulated count
    assert 1 < st1["rounds"] and st1["roundTiles"][1] < dev.num_tiles(W, H)
    ctx.set_camera(cams[2])
    p2 = _params(abi, 2)
    acc2, den2, _, st2 = ctx.render_temporal_frame(p2, d, t)  # ... and the next uniform frame uses the adaptive one's
    _, m2, _ = ctx.render_image_moments(p2, want_rgba=False)
    pl2 = [_h(q) for q in _feature_planes(ctx, dev, abi, p2)]
    want_b, _, _ = R.accumulate(acc2, m2, pl2[1], pl2[2], pl2[3], None, cams[2], cams[1], want["history_out"])
    assert np.array_equal(den2[..., 3], want_b[..., 3]) and st2["historyPixels"] == int((want_b[..., 3] > SPP).sum())
    assert want_b[..., 3].max() > SPP_MAX  # samples of the adaptive frame's refined tiles came along
    ctx.temporal_reset()


def test_errors_launch_nothing_and_leave_no_trace(ctx, dev, abi, srt, camera):
    import torch
    ctx.upload_scene(_scene(srt, "masterchief"))
    ctx.set_camera(camera)
    p = _params(abi, 0)
    before, _ = ctx.render_image(p)
    info, ms = ctx.launch_info(), ctx.last_kernel_ms()
    tun = {k: ctx.get_tunable(k) for k in TUNABLES}
    planes = _feature_planes(ctx, dev, abi, p)
    ptrs = [q.data_ptr() for q in planes]
    bufs = [torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda") for _ in range(4)]
    hist = [torch.full((3, H, W, 4), 7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    rp = torch.full((2, H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    t = abi.default_temporal_params()

    def bad(spp_max=SPP_MAX, thr=0.01, tp=t, pl=None, use=(0, 1, 2, 3), hin=0, hout=1, prev=camera, **fields):
        q = _params(abi, 0)
        for k, v in fields.items():
            setattr(q, k, v)
        b = [bufs[i].data_ptr() if i in use else None for i in range(4)]
        with pytest.raises(dev.SrtError):
            ctx.render_temporal_adaptive_device(q, abi.default_adaptive_params(spp_max, thr), tp, ptrs if pl is None else pl, prev,
                                                hist[hin].data_ptr() if hin is not None else None, b[0], b[1], b[2], b[3],
                                                hist[hout].data_ptr() if hout is not None else None, None)
        msg = dev.lib.srtLastError(ctx.h).decode()
        assert any(w in msg for w in ("adaptive", "temporal", "render")), msg

    # srtRenderAdaptive's
    bad(spp=1, spp_max=8)
    bad(spp_max=3)
    bad(spp_max=(1 << 24) + 1)
    bad(sampleFirst=(1 << 31) - 40, spp_max=64)
    bad(thr=-0.5)
    bad(thr=float("nan"))
    bad(countStats=1)
    bad(tileFirst=1, tileStride=2)
    bad(use=(1, 2, 3))
    bad(use=(0, 2, 3))
    bad(sppChunks=5)
    # srtTemporalAccumulate's
    bad(pl=[ptrs[0], None, ptrs[2], ptrs[3]])
    bad(pl=[ptrs[0], ptrs[1], None, ptrs[3]])
    bad(pl=[ptrs[0], ptrs[1], ptrs[2], None])
    bad(tp=abi.default_temporal_params(demodulate=1), pl=[None] + ptrs[1:])
    bad(hout=0)
    bad(hout=None)
    bad(use=(0, 1))
    bad(prev=None)
    bad(tp=abi.default_temporal_params(normal_cos=1.5))
    bad(tp=abi.default_temporal_params(plane_dist=-1.0))
    bad(tp=abi.default_temporal_params(max_history=float("nan")))
    for kw in (dict(pl=[ptrs[0], None, ptrs[2], ptrs[3]]), dict(out=None), dict(out=hist[0].data_ptr()), dict(w=1),
               dict(tp=abi.default_temporal_params(plane_dist=-1.0)), dict(tp=abi.default_temporal_params(demodulate=1), pl=[None] + ptrs[1:])):
        with pytest.raises(dev.SrtError):
            ctx.temporal_reproject(kw.get("tp", t), kw.get("w", W), H, kw.get("pl", ptrs), camera, camera, hist[0].data_ptr(),
                                   kw.get("out", rp.data_ptr()), None)
        assert "temporal" in dev.lib.srtLastError(ctx.h).decode()
    with pytest.raises(dev.SrtError):
        ctx.render_temporal_adaptive_frame(p, abi.default_adaptive_params(3, 0.01))
    with pytest.raises(dev.SrtError):
        ctx.render_temporal_adaptive_frame(p, abi.default_adaptive_params(SPP_MAX, 0.01), abi.default_denoise_params(iterations=99))
    with pytest.raises(dev.SrtError):
        ctx.render_temporal_adaptive_frame(p, abi.default_adaptive_params(SPP_MAX, 0.01), None, abi.default_temporal_params(plane_dist=-1.0))
    torch.cuda.synchronize()
    assert all((b == 7.0).all() for b in bufs + hist + [rp])
    assert ctx.launch_info() == info and ctx.last_kernel_ms() == ms  # nothing launched
    # a good frame changes nothing a later render reads; the launch diagnostics describe its last render launch
    dev.host_random_reset()
    want_draw = dev.host_random_float()
    dev.host_random_reset()
    ctx.temporal_reset()
    _, _, _, st = ctx.render_temporal_adaptive_frame(p, abi.default_adaptive_params(SPP_MAX, 0.04))
    assert st["rounds"] > 1 and ctx.last_kernel_ms() == pytest.approx(st["roundMs"][-1])
    assert dev.host_random_float() == want_draw
    assert {k: ctx.get_tunable(k) for k in TUNABLES} == tun
    after, _ = ctx.render_image(p)
    assert _same(after, before)
    ctx.temporal_reset()


def test_cpp_example_sequence_matches_python_path(tmp_path, ctx, dev, abi, srt):
    """examples/main.cpp --frames 3 --orbit 4 --temporal --adaptive 0.04 --max-spp 32 writes the frames the Python path
    computes, byte for byte."""
    from PIL import Image
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sexy-raytracer_amd", "host")])
    data = tmp_path / "data"
    data.mkdir()
    for f in ("masterchief2-separate-xf.gltf", "masterchief2-separate-xf.bin", "Image_0.png", "Image_1.png"):
        shutil.copy(os.path.join(ROOT, "assets", f), data / f)
    a, n, m, r = srt.scenes.iron_textures()
    Image.fromarray(a).save(data / "rustediron2_basecolor-2x1.png")
    Image.fromarray(n).save(data / "rustediron2_normal-2x1.png")
    Image.fromarray(m[..., 0]).save(data / "rustediron2_metallic-2x1.png")
    Image.fromarray(r[..., 0]).save(data / "rustediron2_roughness-2x1.png")
    env = dict(os.environ, SRT_DATA_DIR=str(data))
    frames, orbit = 3, 4.0
    subprocess.check_call([os.path.join(ROOT, "examples", "srt_main"), "--gltf", str(data / "masterchief2-separate-xf.gltf"),
                           "--height", "72", "--spp", str(SPP), "--bounces", "4", "--frames", str(frames), "--orbit", str(orbit),
                           "--out", str(tmp_path / "seq.png"), "--temporal", "--adaptive", "0.04", "--max-spp", str(SPP_MAX)], env=env)
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.temporal_reset()
    ap = abi.default_adaptive_params(SPP_MAX, 0.04)
    rounds = []
    for k in range(frames):
        ctx.set_camera(_orbit_camera(dev, abi, orbit * k / (frames - 1)))
        p = abi.default_render_params(128, 72, SPP, 4, seed=1, spp_chunks=0, sample_first=k * SPP_MAX)
        _, _, want, st = ctx.render_temporal_adaptive_frame(p, ap)
        rounds.append(st["rounds"])
        got = np.asarray(Image.open(tmp_path / ("seq_%03d.png" % k)).convert("RGBA"))
        assert np.array_equal(got, want), k
    assert max(rounds) > 1
    ctx.temporal_reset()


# ------------------------------------------------------------------ 7. quality: the band


def _display(mean):
    return np.sqrt(np.clip(np.nan_to_num(mean[..., :3], nan=0.0, posinf=1.0), 0.0, 1.0))


def _edge_band(ctx, abi, w, h):
    """DESIGN.md 5.9's band: pixels within 2 px of a hit/miss boundary or a relative depth step of more than 10 %."""
    f = ctx.render_features(abi.default_render_params(w, h, 16, 4, seed=5), abi.SRT_FEATURE_DEPTH)["depth"]
    z = np.where(f[..., 3] > 0, f[..., 0], np.inf)
    e = np.zeros((h, w), bool)
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
        g[1:] |= e[:-1]
        g[:-1] |= e[1:]
        g[:, 1:] |= e[:, :-1]
        g[:, :-1] |= e[:, 1:]
        e = g
    return e


# threshold and sppMax of the assertion, from tools/temporal_adaptive_bench.py's sweep (DESIGN.md 5.10,
# profiles/r09/temporal_adaptive_bench.json; 8 frames, band MSE adaptive / uniform of at least as many samples):
#   spheres      0.00179 / 0.00277  (9.57 samples per pixel per frame against 10)
#   iron         0.00165 / 0.00290  (8.53 against 9)
#   masterchief  0.00481 / 0.00475  (18.99 against 19): NOT ahead, so it stays out of the assertion.  Its lit model never
#                gets below the threshold, two thirds of its tiles go to sppMax with or without history, and the uniform frame's
#                feature means come from 19 samples where the adaptive frame's come from its first 4 ("where
#                it does not pay")
QUALITY_THR, QUALITY_SPP_MAX = 0.02, 32


@pytest.mark.parametrize("name", ["spheres", "iron"])
def test_band_error_is_below_the_uniform_temporal_frame(ctx, dev, abi, srt, name):
    """DESIGN.md 5.9's orbit (1.5 degrees a frame, 426 x 240, 4 spp) shortened to 5 frames: the last frame's display-space
    MSE over the edge band against a 1024-spp render of that camera is below the uniform temporal frame's, which gets
    ceil(the adaptive run's mean samples per pixel per frame) samples, never fewer.  A direction only; the seeds are fixed."""
    w, h, frames, step = 426, 240, 5, 1.5
    ctx.upload_scene({"spheres": srt.scenes.scene_spheres, "iron": srt.scenes.scene_iron}[name]())
    d, t = abi.default_denoise_params(), abi.default_temporal_params()
    ap = abi.default_adaptive_params(QUALITY_SPP_MAX, QUALITY_THR)
    ctx.temporal_reset()
    samples = 0
    for k in range(frames):
        ctx.set_camera(_orbit_camera(dev, abi, k * step))
        p = abi.default_render_params(w, h, SPP, 4, seed=11, spp_chunks=0, sample_first=k * QUALITY_SPP_MAX)
        _, den_a, _, st = ctx.render_temporal_adaptive_frame(p, ap, d, t)
        samples += st["pixelSamples"]
    spp_uniform = math.ceil(samples / (frames * w * h))
    assert spp_uniform * frames * w * h >= samples
    ctx.temporal_reset()
    for k in range(frames):
        ctx.set_camera(_orbit_camera(dev, abi, k * step))
        p = abi.default_render_params(w, h, spp_uniform, 4, seed=11, spp_chunks=0, sample_first=k * spp_uniform)
        _, den_u, _, _ = ctx.render_temporal_frame(p, d, t)
    ctx.temporal_reset()
    ref, _ = ctx.render_image(abi.default_render_params(w, h, 1024, 4, seed=99, spp_chunks=0), want_rgba=False)
    truth = _display(ref[..., :3] / ref[..., 3:4])
    band = _edge_band(ctx, abi, w, h)
    err_a, err_u = (_display(den_a) - truth) ** 2, (_display(den_u) - truth) ** 2
    print("%s: %.2f samples per pixel per frame adaptive, %d uniform; band MSE %.5f / %.5f, frame MSE %.5f / %.5f" % (
        name, samples / (frames * w * h), spp_uniform, err_a[band].mean(), err_u[band].mean(), err_a.mean(), err_u.mean()))
    assert err_a[band].mean() < err_u[band].mean()
