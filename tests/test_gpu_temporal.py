"""Temporal accumulation on the GPU (include/srt_hip.h srtTemporalAccumulate / srtRenderTemporalFrame,
csrc/srt_temporal.hip): bit parity with the NumPy reference tests/temporal_ref.py on the renderer's own device buffers over
orbit sequences, the static-camera running sum in every render kernel form, the frame entry and what resets it, image
quality and stability against the single-frame pipeline, errors, side effects and the C++ example.

Every operation of the kernel (+ - * / sqrt rint floor, comparisons) is reproducible in NumPy float32, so nothing here is
compared with a tolerance: beauty, moments and the whole history are bit-identical on every pixel."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import temporal_ref as R

pytestmark = pytest.mark.gpu
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _orbit_camera(dev, abi, degrees):
    """examples/main.cpp --orbit: the default eye turned about the vertical axis through the lookAt point."""
    c = abi.default_camera_params()
    a = np.deg2rad(np.float64(degrees))
    dx, dz = np.float32(c.eye[0] - c.lookAt[0]), np.float32(c.eye[2] - c.lookAt[2])
    co, si = np.float32(np.cos(a)), np.float32(np.sin(a))
    c.eye[0] = np.float32(c.lookAt[0]) + (co * dx + si * dz)
    c.eye[2] = np.float32(c.lookAt[2]) + (co * dz - si * dx)
    return dev.make_camera(c)


def _device_frame(ctx, dev, abi, p):
    """The all-device pipeline of one frame: beauty and moments tiles, the four feature planes, each resolved to image
    order.  Returns (beauty, moments, [albedo, normal, position, depth]) as (H, W, 4) cuda tensors."""
    import torch
    W, H = p.imageWidth, p.imageHeight
    nloc = dev.num_local_tiles(W, H, 1)
    tiles = [torch.zeros((nloc, 64, 4), dtype=torch.float32, device="cuda") for _ in range(6)]
    ctx.render_tiles_moments(p, tiles[0].data_ptr(), tiles[1].data_ptr(), None)
    ctx.render_feature_tiles(p, abi.SRT_FEATURE_ALL, [t.data_ptr() for t in tiles[2:]], None)
    img = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(6)]
    for k in range(6):
        ctx.resolve_tiles(p, tiles[k].data_ptr(), None, img[k].data_ptr(), None)
    torch.cuda.synchronize()
    return img[0], img[1], img[2:]


def _accumulate(ctx, t, beauty, moments, planes, cam, prev, hist, want_moments=True):
    import torch
    H, W = beauty.shape[:2]
    out_b = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    out_m = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    new = torch.full((3, H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    ctx.temporal_accumulate(t, W, H, beauty.data_ptr(), moments.data_ptr() if moments is not None else None,
                            [q.data_ptr() if q is not None else None for q in planes], cam, prev,
                            hist.data_ptr() if hist is not None else None, out_b.data_ptr(),
                            out_m.data_ptr() if want_moments else None, new.data_ptr(), None)
    torch.cuda.synchronize()
    return out_b, out_m, new


def _scene(srt, name):
    return {"spheres": srt.scenes.scene_spheres, "masterchief": srt.scenes.scene_masterchief}[name]()


def _h(t):
    return t.cpu().numpy()


CASES = [  # scene, width, height, spp, demodulate, maxHistory, (normalCos, planeDist); 0 = default
    ("spheres", 426, 240, 4, 0, 0, (0, 0)),
    ("spheres", 97, 61, 4, 1, INF, (0.8, 0.05)),
    ("masterchief", 426, 240, 4, 1, 6.0, (0, 0)),
    ("masterchief", 97, 61, 8, 0, INF, (0.95, 0.01)),
    ("masterchief", 426, 240, 8, 0, 0, (0, 0)),
    ("spheres", 426, 240, 4, 1, 5.0, (0.5, 0.1)),
]


@pytest.mark.parametrize("case", CASES, ids=["%s-%dx%d-dm%d-cap%s" % (c[0], c[1], c[2], c[4], c[5]) for c in CASES])
def test_temporal_matches_reference(ctx, dev, abi, srt, case):
    """Three frames of an orbit: kernel and reference each run their own chain, and every output of every frame agrees
    bit for bit.  Where the reference rejects the history, the output is exactly the current frame (no ghosting)."""
    name, W, H, spp, dm, cap, (ncos, pdist) = case
    ctx.upload_scene(_scene(srt, name))
    t = abi.default_temporal_params(ncos, pdist, cap, dm)
    hist_gpu = hist_ref = prev = None
    accepted = 0
    for k, deg in enumerate((0.0, 2.0, 4.5)):
        cam = _orbit_camera(dev, abi, deg)
        ctx.set_camera(cam)
        p = abi.default_render_params(W, H, spp, 4, seed=7, spp_chunks=0, sample_first=k * spp)
        beauty, moments, planes = _device_frame(ctx, dev, abi, p)
        use = planes if dm else [None] + planes[1:]
        got_b, got_m, hist_gpu = _accumulate(ctx, t, beauty, moments, use, cam, prev, hist_gpu)
        info = {}
        want_b, want_m, hist_ref = R.accumulate(_h(beauty), _h(moments), _h(planes[1]), _h(planes[2]), _h(planes[3]),
                                                _h(planes[0]) if dm else None, cam, prev, hist_ref, ncos, pdist, cap, bool(dm),
                                                info=info)
        label = "%s frame %d" % (case[:3], k)
        for g, w, what in ((got_b, want_b, "beauty"), (got_m, want_m, "moments"), (hist_gpu, hist_ref, "history")):
            g = _h(g)
            diff = _bits(g) != _bits(w)
            assert not diff.any(), (label, what, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        rejected = ~info["has"]
        assert np.array_equal(_bits(_h(got_b)[rejected]), _bits(_h(beauty)[rejected])), label
        if k:
            accepted += int(info["has"].sum())
            assert 0.2 < info["has"].mean() < 1.0, (label, info["has"].mean())  # pixels reuse, some are disoccluded
        prev = cam
    assert accepted > 0


def test_static_camera_is_the_sum_of_the_passes(ctx, dev, abi, srt, camera, node_path):
    """K frames from one camera with fresh samples, no cap, no demodulation: the image-order sum of the K
    srtRenderImageMoments passes, ((f0 + f1) + f2) + ..., bit for bit, beauty and moments, in every render kernel form."""
    W, H, n, K = 97, 61, 4, 4
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    t = abi.default_temporal_params(max_history=INF)
    hist, sum_b, sum_m = None, None, None
    clean = np.ones((H, W), bool)
    for k in range(K):
        p = abi.default_render_params(W, H, n, 4, seed=3, spp_chunks=0, sample_first=k * n)
        beauty, moments, planes = _device_frame(ctx, dev, abi, p)
        got_b, got_m, hist = _accumulate(ctx, t, beauty, moments, [None] + planes[1:], camera, camera, hist)
        acc, mom, _ = ctx.render_image_moments(p, want_rgba=False)
        assert np.array_equal(_bits(acc), _bits(_h(beauty)))
        # a pass's NaN / inf pixel (the r = 0 ground) stays out of the history by contract, where a plain sum would keep
        # it for ever: the sum is claimed for the pixels every pass so far rendered finite
        clean &= np.isfinite(acc).all(-1) & np.isfinite(mom).all(-1)
        sum_b = acc if sum_b is None else sum_b + acc
        sum_m = mom if sum_m is None else sum_m + mom
        assert np.array_equal(_bits(_h(got_b))[clean], _bits(sum_b)[clean]), (node_path, k)
        assert np.array_equal(_bits(_h(got_m))[clean], _bits(sum_m)[clean]), (node_path, k)
    assert clean.mean() > 0.99
    assert (sum_b[..., 3][clean] == K * n).all()


def test_null_moments_accumulates_beauty_only(ctx, dev, abi, srt, camera):
    ctx.upload_scene(srt.scenes.scene_spheres())
    ctx.set_camera(camera)
    t = abi.default_temporal_params(max_history=INF)
    p = abi.default_render_params(97, 61, 4, 4, seed=5, spp_chunks=0)
    beauty, moments, planes = _device_frame(ctx, dev, abi, p)
    _, _, hist = _accumulate(ctx, t, beauty, None, [None] + planes[1:], camera, None, None)
    got_b, got_m, _ = _accumulate(ctx, t, beauty, None, [None] + planes[1:], camera, camera, hist)
    want_b, want_m, _ = R.accumulate(_h(beauty), None, _h(planes[1]), _h(planes[2]), _h(planes[3]), None, camera, camera, _h(hist),
                                     max_history=INF)
    assert np.array_equal(_bits(_h(got_b)), _bits(want_b)) and np.array_equal(_bits(_h(got_m)), _bits(want_m))
    assert (_h(got_m)[..., :3] == 0).all() and np.array_equal(_h(got_m)[..., 3], _h(got_b)[..., 3])


def test_frame_entry_matches_the_device_path_and_starts_over(ctx, dev, abi, srt, camera):
    W, H, n = 97, 61, 4
    ctx.upload_scene(srt.scenes.scene_masterchief())
    d = abi.default_denoise_params()
    t = abi.default_temporal_params()
    cams = [camera, _orbit_camera(dev, abi, 3.0)]

    def first_frame_is_single_frame(width, height):
        ctx.set_camera(cams[0])
        p = abi.default_render_params(width, height, n, 4, seed=9, spp_chunks=0)
        acc, den, rgba, st = ctx.render_temporal_frame(p, d, t)
        acc1, _, den1, rgba1 = ctx.render_denoised_moments(p, d)
        assert np.array_equal(_bits(acc), _bits(acc1)) and np.array_equal(_bits(den), _bits(den1)) and np.array_equal(rgba, rgba1)
        assert np.array_equal(_bits(acc), _bits(ctx.render_image(p, want_rgba=False)[0]))
        assert st["historyPixels"] == 0
        return p

    ctx.temporal_reset()
    first_frame_is_single_frame(W, H)
    # frame 1 through the entry against the same two frames through the device path
    ctx.set_camera(cams[1])
    p1 = abi.default_render_params(W, H, n, 4, seed=9, spp_chunks=0, sample_first=n)
    acc, den, rgba, st = ctx.render_temporal_frame(p1, d, t)
    assert np.array_equal(_bits(acc), _bits(ctx.render_image(p1, want_rgba=False)[0]))
    assert 0.5 * W * H < st["historyPixels"] < W * H and n < st["meanHistoryCount"] < 2 * n
    import torch
    hist = prev = None
    for k, cam in enumerate(cams):
        ctx.set_camera(cam)
        p = abi.default_render_params(W, H, n, 4, seed=9, spp_chunks=0, sample_first=k * n)
        beauty, moments, planes = _device_frame(ctx, dev, abi, p)
        out_b, out_m, hist = _accumulate(ctx, t, beauty, moments, [None] + planes[1:], cam, prev, hist)
        prev = cam
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.denoise(d, W, H, out_b.data_ptr(), [None, planes[1].data_ptr(), None, planes[3].data_ptr()], out.data_ptr(), out8.data_ptr(),
                None, d_moments_ptr=out_m.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(den), _bits(_h(out))) and np.array_equal(rgba, _h(out8))
    assert np.array_equal(den[..., 3], _h(out_b)[..., 3])  # w = the accumulated count
    # reset, another size, a re-upload and a flip of demodulate each start over
    ctx.temporal_reset()
    first_frame_is_single_frame(W, H)
    first_frame_is_single_frame(80, 48)
    ctx.upload_scene(srt.scenes.scene_masterchief())
    first_frame_is_single_frame(80, 48)
    t.demodulate = 1
    first_frame_is_single_frame(80, 48)
    ctx.temporal_reset()


def _display(mean):
    return np.sqrt(np.clip(np.nan_to_num(mean[..., :3], nan=0.0, posinf=1.0), 0.0, 1.0))


@pytest.mark.parametrize("name", ["masterchief", "spheres"])
def test_temporal_beats_the_single_frame_pipeline(ctx, dev, abi, srt, name):
    """An 8-frame orbit at 4 spp: the last frame's display-space MSE against a 1024-spp render of that camera is below the
    single-frame denoiser's at the same 4 spp; and with a static camera consecutive outputs differ less."""
    W, H, n, K, step = 426, 240, 4, 8, 1.5
    ctx.upload_scene(_scene(srt, name))
    d, t = abi.default_denoise_params(), abi.default_temporal_params()
    ctx.temporal_reset()
    for k in range(K):
        cam = _orbit_camera(dev, abi, k * step)
        ctx.set_camera(cam)
        p = abi.default_render_params(W, H, n, 4, seed=11, spp_chunks=0, sample_first=k * n)
        _, den, _, st = ctx.render_temporal_frame(p, d, t)
    _, _, single, _ = ctx.render_denoised_moments(p, d)
    ref, _ = ctx.render_image(abi.default_render_params(W, H, 1024, 4, seed=99, spp_chunks=0), want_rgba=False)
    truth = _display(ref[..., :3] / ref[..., 3:4])
    mse_t = float(((_display(den) - truth) ** 2).mean())
    mse_s = float(((_display(single) - truth) ** 2).mean())
    print("%s orbit: display MSE temporal %.4g, single frame %.4g, ratio %.3f; history %.0f%% of the pixels, %.1f samples"
          % (name, mse_t, mse_s, mse_t / mse_s, 100.0 * st["historyPixels"] / (W * H), st["meanHistoryCount"]))
    assert mse_t / mse_s < 1
    # static camera: frame-to-frame flicker
    ctx.temporal_reset()
    ctx.set_camera(cam)
    outs_t, outs_s = [], []
    for k in range(6):
        p = abi.default_render_params(W, H, n, 4, seed=12, spp_chunks=0, sample_first=k * n)
        outs_t.append(_display(ctx.render_temporal_frame(p, d, t)[1]))
        outs_s.append(_display(ctx.render_denoised_moments(p, d)[2]))
    flick_t = float(np.mean([np.abs(a - b).mean() for a, b in zip(outs_t[1:], outs_t[2:])]))
    flick_s = float(np.mean([np.abs(a - b).mean() for a, b in zip(outs_s[1:], outs_s[2:])]))
    print("%s static: mean |frame - previous| temporal %.4g, single frame %.4g" % (name, flick_t, flick_s))
    assert flick_t < flick_s
    ctx.temporal_reset()


def test_temporal_errors_and_side_effects(ctx, dev, abi, srt, camera):
    import torch
    W, H = 97, 61
    ctx.upload_scene(srt.scenes.scene_spheres())
    ctx.set_camera(camera)
    p = abi.default_render_params(W, H, 4, 4, seed=2, spp_chunks=0)
    beauty, moments, planes = _device_frame(ctx, dev, abi, p)
    ctx.render_image(p)  # the launch the diagnostics describe
    before = (ctx.launch_info(), ctx.last_kernel_ms(), {k: ctx.get_tunable(k) for k in ("lds_tree", "wavefront", "denoise_lds_step")})
    dev.host_random_reset()
    rnd = [dev.host_random_float() for _ in range(3)]
    dev.host_random_reset()
    t = abi.default_temporal_params()
    _, _, hist = _accumulate(ctx, t, beauty, moments, [None] + planes[1:], camera, None, None)
    assert [dev.host_random_float() for _ in range(3)] == rnd
    assert (ctx.launch_info(), ctx.last_kernel_ms(), {k: ctx.get_tunable(k) for k in before[2]}) == before
    out_b = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    out_m = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    new = torch.full((3, H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    ptrs = [q.data_ptr() for q in planes]

    def call(tp=t, w=W, h=H, pl=None, hin=hist.data_ptr(), ob=out_b.data_ptr(), om=out_m.data_ptr(), hout=new.data_ptr()):
        ctx.temporal_accumulate(tp, w, h, beauty.data_ptr(), moments.data_ptr(), ptrs if pl is None else pl, camera, camera, hin, ob,
                                om, hout, None)

    bad = [dict(pl=[ptrs[0], None, ptrs[2], ptrs[3]]), dict(pl=[ptrs[0], ptrs[1], None, ptrs[3]]),
           dict(pl=[ptrs[0], ptrs[1], ptrs[2], None]), dict(tp=abi.default_temporal_params(demodulate=1), pl=[None] + ptrs[1:]),
           dict(w=0), dict(h=-3), dict(hout=hist.data_ptr()), dict(hout=None), dict(ob=None, om=None),
           dict(tp=abi.default_temporal_params(normal_cos=-0.5)), dict(tp=abi.default_temporal_params(normal_cos=1.5)),
           dict(tp=abi.default_temporal_params(plane_dist=-1.0)), dict(tp=abi.default_temporal_params(max_history=-2.0)),
           dict(tp=abi.default_temporal_params(plane_dist=float("nan"))), dict(tp=abi.default_temporal_params(max_history=float("nan")))]
    for kw in bad:
        with pytest.raises(dev.SrtError):
            call(**kw)
    torch.cuda.synchronize()
    assert (out_b == 7.0).all() and (out_m == 7.0).all() and (new == 7.0).all()
    call()  # and the good call writes everything
    torch.cuda.synchronize()
    assert not (out_b == 7.0).all(-1).any() and not (new[0] == 7.0).all(-1).any()
    with pytest.raises(dev.SrtError):
        ctx.render_temporal_frame(p, abi.default_denoise_params(iterations=99), t)
    with pytest.raises(dev.SrtError):
        ctx.render_temporal_frame(p, None, abi.default_temporal_params(plane_dist=-1.0))
    ctx.temporal_reset()


def test_cpp_example_sequence_matches_python_path(tmp_path, ctx, dev, abi, srt):
    """examples/main.cpp --frames 3 --orbit 4 --temporal writes the frames the Python path computes, byte for byte; without
    --temporal the same cameras denoised frame by frame."""
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
    frames, orbit, spp = 3, 4.0, 4
    base = [os.path.join(ROOT, "examples", "srt_main"), "--gltf", str(data / "masterchief2-separate-xf.gltf"), "--height", "120",
            "--spp", str(spp), "--bounces", "4", "--frames", str(frames), "--orbit", str(orbit)]
    subprocess.check_call(base + ["--out", str(tmp_path / "seq.png"), "--temporal"], env=env)
    subprocess.check_call(base + ["--out", str(tmp_path / "single.png")], env=env)
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.temporal_reset()
    for k in range(frames):
        ctx.set_camera(_orbit_camera(dev, abi, orbit * k / (frames - 1)))
        p = abi.default_render_params(213, 120, spp, 4, seed=1, spp_chunks=0, sample_first=k * spp)
        want = ctx.render_temporal_frame(p)[2]
        got = np.asarray(Image.open(tmp_path / ("seq_%03d.png" % k)).convert("RGBA"))
        assert np.array_equal(got, want), k
        want = ctx.render_denoised_moments(p)[3]
        got = np.asarray(Image.open(tmp_path / ("single_%03d.png" % k)).convert("RGBA"))
        assert np.array_equal(got, want), k
    ctx.temporal_reset()
