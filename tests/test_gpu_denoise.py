"""The denoiser (include/srt_hip.h srtDenoise / srtRenderDenoisedImage, csrc/srt_denoise.hip): parity with the NumPy
reference tests/denoise_ref.py on the renderer's own device buffers, synthetic inputs, the device and the blocking paths,
the tile split, image quality against a high-spp render, side effects, errors and the C++ example."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import denoise_ref as R

pytestmark = pytest.mark.gpu

# the kernel's v_exp_f32 / v_log_f32 against libm: per channel relative, and the mean absolute difference
REL_TOL, MEAN_ABS_TOL = 2e-4, 1e-6


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device_frame(ctx, dev, abi, p, ranks=1):
    """The all-device pipeline: beauty and feature tiles of `ranks` tile-split renders concatenated as the gather lays them
    out, each resolved to image order.  Returns (beauty, [albedo, normal, None, depth]) as (H, W, 4) cuda tensors."""
    import torch
    W, H = p.imageWidth, p.imageHeight
    nloc = dev.num_local_tiles(W, H, ranks)
    tiles = [torch.zeros((ranks, nloc, 64, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    planes = abi.SRT_FEATURE_ALBEDO | abi.SRT_FEATURE_NORMAL | abi.SRT_FEATURE_DEPTH
    for r in range(ranks):
        p.tileFirst, p.tileStride = r, ranks
        ctx.render_tiles(p, tiles[0][r].data_ptr(), None)
        ctx.render_feature_tiles(p, planes, [tiles[1][r].data_ptr(), tiles[2][r].data_ptr(), None, tiles[3][r].data_ptr()], None)
    img = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    for k in range(4):
        ctx.resolve_tiles(p, tiles[k].data_ptr(), None, img[k].data_ptr(), None)
    torch.cuda.synchronize()
    p.tileFirst, p.tileStride = 0, 1
    return img[0], [img[1], img[2], None, img[3]]


def _run(ctx, d, beauty, planes):
    import torch
    H, W = beauty.shape[:2]
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.denoise(d, W, H, beauty.data_ptr(), [t.data_ptr() if t is not None else None for t in planes], out.data_ptr(),
                rgba.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), rgba.cpu().numpy()


def _reference(d, beauty, planes):
    h = lambda t: t.cpu().numpy()  # noqa: E731
    return R.denoise(h(beauty), h(planes[1]), h(planes[3]), h(planes[0]) if planes[0] is not None else None,
                     iterations=d.iterations, demodulate=bool(d.demodulate), sigma_l=d.sigmaLuminance,
                     sigma_n=d.sigmaNormal, sigma_z=d.sigmaDepth)


def _compare(got, want, got_rgba, want_rgba, label):
    """The kernel against the reference: rgb within REL_TOL per channel and MEAN_ABS_TOL on average, w equal, rgba within
    one step.  Returns (max relative, mean absolute) difference."""
    assert np.isfinite(got).all(), label
    assert np.array_equal(got[..., 3], want[..., 3]), label
    diff = np.abs(got[..., :3].astype(np.float64) - want[..., :3])
    rel = diff / np.maximum(np.abs(want[..., :3]), 1e-6)
    print("%s: max relative %.3g, mean absolute %.3g" % (label, rel.max(), diff.mean()))
    assert rel.max() <= REL_TOL, (label, rel.max(), np.unravel_index(rel.argmax(), rel.shape))
    assert diff.mean() <= MEAN_ABS_TOL, (label, diff.mean())
    assert np.abs(got_rgba.astype(int) - want_rgba.astype(int)).max() <= 1, label
    return rel.max(), diff.mean()


def _scene(srt, name):
    return {"spheres": srt.scenes.scene_spheres, "masterchief": srt.scenes.scene_masterchief}[name]()


CASES = [  # scene, width, height, spp, iterations, demodulate, (sigmaL, sigmaN, sigmaZ); 0 = default
    ("spheres", 426, 240, 8, 5, 0, (0, 0, 0)),
    ("spheres", 97, 61, 4, 8, 1, (2.0, 64.0, 0.5)),
    ("masterchief", 426, 240, 8, 3, 1, (0, 0, 0)),
    ("masterchief", 97, 61, 16, 1, 0, (8.0, 32.0, 2.0)),
    ("masterchief", 426, 240, 4, 8, 0, (6.0, 200.0, 0.25)),
    ("masterchief", 97, 61, 8, 5, 1, (0, 0, 0)),
]


@pytest.mark.parametrize("case", CASES, ids=["%s-%dx%d-it%d-dm%d" % (c[0], c[1], c[2], c[4], c[5]) for c in CASES])
def test_denoise_matches_reference(ctx, dev, abi, srt, camera, case):
    name, W, H, spp, it, dm, sig = case
    ctx.upload_scene(_scene(srt, name))
    ctx.set_camera(camera)
    beauty, planes = _device_frame(ctx, dev, abi, abi.default_render_params(W, H, spp, 4, seed=7, spp_chunks=0))
    d = abi.default_denoise_params(it, dm, *sig)
    got, got_rgba = _run(ctx, d, beauty, planes)
    want, want_rgba = _reference(d, beauty, planes)
    _compare(got, want, got_rgba, want_rgba, "%s %dx%d it=%d dm=%d" % (case[:3] + case[4:6]))


def test_denoise_lds_and_cache_forms_agree(ctx, dev, abi, srt, camera):
    """Levels staged in LDS and levels read through the caches: the same bits."""
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    beauty, planes = _device_frame(ctx, dev, abi, abi.default_render_params(426, 240, 4, 4, seed=2, spp_chunks=0))
    d = abi.default_denoise_params(5, 1)
    saved = ctx.get_tunable("denoise_lds_step")
    try:
        runs = []
        for v in (0, 1, 4, 8):
            ctx.set_tunable("denoise_lds_step", v)
            runs.append(_run(ctx, d, beauty, planes))
    finally:
        ctx.set_tunable("denoise_lds_step", saved)
    for out, rgba in runs[1:]:
        assert np.array_equal(_bits(out), _bits(runs[0][0])) and np.array_equal(rgba, runs[0][1])


def _synthetic(H, W, spp=4, seed=0):
    import torch
    rng = np.random.default_rng(seed)
    beauty = np.zeros((H, W, 4), np.float32)
    beauty[..., :3] = rng.uniform(0.05, 3.0, (H, W, 3)).astype(np.float32) * spp
    beauty[..., 3] = spp
    normal = np.zeros((H, W, 4), np.float32)
    normal[..., :3] = rng.normal(0, 0.1, (H, W, 3)).astype(np.float32) * spp
    normal[..., 1] += spp
    normal[..., 3] = spp
    depth = np.zeros((H, W, 4), np.float32)
    depth[..., 0] = (2.0 + 0.01 * np.arange(W, dtype=np.float32))[None, :] * spp
    depth[..., 3] = spp
    albedo = np.zeros((H, W, 4), np.float32)
    albedo[..., :3] = rng.uniform(0.1, 0.9, (H, W, 3)).astype(np.float32) * spp
    albedo[..., 3] = spp
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    return t(beauty), [t(albedo), t(normal), None, t(depth)]


@pytest.mark.parametrize("demodulate", [0, 1])
def test_constant_image_is_unchanged(ctx, abi, demodulate):
    beauty, planes = _synthetic(61, 97)
    col = np.float32([0.7, 0.3, 1.9])
    beauty[..., :3] = beauty.new_tensor(col * np.float32(4))
    planes[0][..., :3] = planes[0].new_tensor(np.float32([0.5, 0.25, 0.75]) * np.float32(4))  # demodulation by a constant
    out, rgba = _run(ctx, abi.default_denoise_params(8, demodulate), beauty, planes)
    assert (np.abs(out[..., :3] - col) <= 2 * np.spacing(col)).all()
    assert (out[..., 3] == 4).all() and (rgba[..., 3] == 255).all()


def test_sky_stays_background_next_to_geometry(ctx, dev, abi, srt, camera):
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    p = abi.default_render_params(426, 240, 16, 4, seed=3, spp_chunks=0)
    beauty, planes = _device_frame(ctx, dev, abi, p)
    out, _ = _run(ctx, abi.default_denoise_params(5, 1), beauty, planes)
    nrm = planes[1].cpu().numpy()
    sky = nrm[..., 3] == 0
    # sky pixels with hit pixels within the filter's reach on both sides of the horizon
    near = np.zeros_like(sky)
    near[:, 1:] |= ~sky[:, :-1]
    near[:, :-1] |= ~sky[:, 1:]
    near[1:] |= ~sky[:-1]
    near[:-1] |= ~sky[1:]
    assert (sky & near).sum() > 50 and sky.sum() > 1000
    bg = np.float32(p.background[:])
    rel = np.abs(out[sky, :3] - bg) / bg
    assert rel.max() <= 1e-6, rel.max()


def test_nan_and_inf_pixels_are_filled(ctx, dev, abi, srt, camera):
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    beauty, planes = _device_frame(ctx, dev, abi, abi.default_render_params(97, 61, 8, 4, seed=5, spp_chunks=0))
    bad = [(10, 20, float("nan")), (30, 40, float("inf")), (31, 40, float("inf")), (50, 90, float("-inf")), (0, 0, float("nan"))]
    for y, x, v in bad:
        beauty[y, x, 1] = v
    beauty[20, 60, :3] = float("inf")  # a white overflowed chunk sum
    for dm in (0, 1):
        d = abi.default_denoise_params(3, dm)
        got, got_rgba = _run(ctx, d, beauty, planes)
        want, want_rgba = _reference(d, beauty, planes)
        assert np.isfinite(got).all()
        for y, x, _ in bad:
            assert np.isfinite(got[y, x, :3]).all()
        _compare(got, want, got_rgba, want_rgba, "nan/inf dm=%d" % dm)


def test_device_path_and_blocking_entry_agree(ctx, dev, abi, srt, camera):
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    p = abi.default_render_params(426, 240, 8, 4, seed=11, spp_chunks=0)
    d = abi.default_denoise_params(5, 1, 3.0)
    accum, denoised, rgba = ctx.render_denoised(p, d)
    acc_img, _ = ctx.render_image(p)
    assert np.array_equal(_bits(accum), _bits(acc_img))
    for ranks in (1, 3):
        beauty, planes = _device_frame(ctx, dev, abi, p, ranks)
        assert np.array_equal(_bits(beauty.cpu().numpy()), _bits(accum)), ranks
        out, out_rgba = _run(ctx, d, beauty, planes)
        assert np.array_equal(_bits(out), _bits(denoised)), ranks
        assert np.array_equal(out_rgba, rgba), ranks


def _display_mse(img, ref, mask):
    return float(np.mean((np.sqrt(np.maximum(img[mask], 0)) - np.sqrt(np.maximum(ref[mask], 0))) ** 2))


def test_denoised_quality_beats_noise(ctx, abi, srt, camera):
    """masterchief, 320x180, 16 spp against 1024 spp of the same frame, in display (sqrt) space; default sigmas, albedo
    demodulation on (0.41 measured)."""
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    p = abi.default_render_params(320, 180, 16, 4, seed=1, spp_chunks=0)
    accum, denoised, _ = ctx.render_denoised(p, abi.default_denoise_params(demodulate=1))
    ref, _ = ctx.render_image(abi.default_render_params(320, 180, 1024, 4, seed=99, spp_chunks=0))
    noisy = accum[..., :3] / accum[..., 3:4]
    ref = ref[..., :3] / ref[..., 3:4]
    mask = np.isfinite(noisy).all(-1) & np.isfinite(ref).all(-1)
    ratio = _display_mse(denoised[..., :3], ref, mask) / _display_mse(noisy, ref, mask)
    print("masterchief 320x180 16 spp: denoised / noisy MSE %.3f" % ratio)
    assert ratio <= 0.5, ratio


def test_denoise_has_no_side_effects(ctx, dev, abi, srt, camera):
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    p = abi.default_render_params(128, 72, 16, 4, seed=2, spp_chunks=0)
    tun = {k: ctx.get_tunable(k) for k in ("tile_block", "queues", "lds_tree", "wavefront", "chunk_scratch_mb", "denoise_lds_step")}
    before, _ = ctx.render_image(p)
    info, ms = ctx.launch_info(), ctx.last_kernel_ms()
    beauty, planes = _device_frame(ctx, dev, abi, abi.default_render_params(128, 72, 4, 4, seed=2))
    info, ms = ctx.launch_info(), ctx.last_kernel_ms()
    for it in (1, 8):
        _run(ctx, abi.default_denoise_params(it, 1), beauty, planes)
    assert ctx.launch_info() == info and ctx.last_kernel_ms() == ms
    assert {k: ctx.get_tunable(k) for k in tun} == tun
    after, _ = ctx.render_image(p)
    assert np.array_equal(_bits(before), _bits(after))


def test_denoise_argument_errors(ctx, dev, abi, srt, camera):
    import torch
    lib = dev.lib
    ctx.upload_scene(srt.scenes.scene_spheres())
    ctx.set_camera(camera)
    beauty, planes = _synthetic(16, 24)
    out = torch.zeros((16, 24, 4), dtype=torch.float32, device="cuda")
    ok = abi.default_denoise_params()
    ptr = lambda ps: [t.data_ptr() if t is not None else None for t in ps]  # noqa: E731
    cases = [
        (ok, 24, 16, [planes[0], None, None, planes[3]], "NORMAL"),
        (ok, 24, 16, [planes[0], planes[1], None, None], "DEPTH"),
        (abi.default_denoise_params(demodulate=1), 24, 16, [None, planes[1], None, planes[3]], "ALBEDO"),
        (ok, 0, 16, planes, "size"),
        (ok, 24, -1, planes, "size"),
        (abi.default_denoise_params(9), 24, 16, planes, "iterations"),
        (abi.default_denoise_params(-1), 24, 16, planes, "iterations"),
        (abi.default_denoise_params(sigma_normal=-1.0), 24, 16, planes, "sigma"),
    ]
    for d, W, H, ps, msg in cases:
        out.fill_(7.0)
        torch.cuda.synchronize()
        with pytest.raises(dev.SrtError, match=msg):
            ctx.denoise(d, W, H, beauty.data_ptr(), ptr(ps), out.data_ptr(), None, None)
        torch.cuda.synchronize()
        assert (out == 7.0).all(), msg  # nothing launched
    assert lib.srtDenoise(ctx.h, None, 24, 16, beauty.data_ptr(), None, out.data_ptr(), None, None) != 0
    assert lib.srtRenderDenoisedImage(ctx.h, None, C.byref(ok), None, None, None) != 0
    with pytest.raises(dev.SrtError, match="iterations"):
        ctx.render_denoised(abi.default_render_params(64, 48, 2, 4), abi.default_denoise_params(9))
    acc, _ = ctx.render_image(abi.default_render_params(64, 48, 2, 4))  # the context still renders
    assert np.isfinite(acc).any()
    a2, dn, rgba = ctx.render_denoised(abi.default_render_params(64, 48, 2, 4))
    assert np.isfinite(dn).all() and (rgba[..., 3] == 255).all()


def test_cpp_example_writes_denoised_png(tmp_path, ctx, abi, srt, camera):
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
    out = tmp_path / "denoised.png"
    subprocess.check_call([os.path.join(ROOT, "examples", "srt_main"), "--gltf", str(data / "masterchief2-separate-xf.gltf"),
                           "--height", "240", "--spp", "4", "--bounces", "4", "--out", str(tmp_path / "beauty.png"),
                           "--denoise", str(out)], env=env)
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    p = abi.default_render_params(426, 240, 4, 4, seed=1, spp_chunks=0)
    _, _, rgba = ctx.render_denoised(p)
    _, beauty_rgba = ctx.render_image(p)
    assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")), rgba)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "beauty.png").convert("RGBA")), beauty_rgba)
