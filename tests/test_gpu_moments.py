"""Per-pixel sample moments (include/srt_hip.h srtRenderTilesMoments / srtRenderImageMoments) and the denoiser's sample
variance (srtDenoiseMoments / srtRenderDenoisedImageMoments): the beauty stays bit for bit what srtRenderTiles renders,
the moments are the exact sums of the samples' luminance and its square (restated here from one-sample renders), they do
not depend on the kernel form, the chunk path, the tile split or the run, and the denoiser follows
tests/denoise_moments_ref.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import denoise_moments_ref as RM

pytestmark = pytest.mark.gpu

F = np.float32
REL_TOL, MEAN_ABS_TOL = 2e-4, 1e-6  # the denoiser's tolerances (test_gpu_denoise.py)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    """bit-identical, NaNs of any payload counted equal"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(both_nan | (_bits(a) == _bits(b))))


def _scene(srt, name):
    return {"spheres": srt.scenes.scene_spheres, "iron": srt.scenes.scene_iron, "masterchief": srt.scenes.scene_masterchief}[name]()


def _setup(ctx, srt, camera, name):
    ctx.upload_scene(_scene(srt, name))
    ctx.set_camera(camera)


def _tiles(ctx, dev, abi, p, ranks=1, moments=True):
    """The device path: `ranks` tile-split renders laid out as the gather does, resolved.  Returns (beauty, moments) as
    (H, W, 4) numpy arrays (moments None for the plain render)."""
    import torch
    W, H = p.imageWidth, p.imageHeight
    nloc = dev.num_local_tiles(W, H, ranks)
    t = [torch.full((ranks, nloc, 64, 4), 7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    for r in range(ranks):
        p.tileFirst, p.tileStride = r, ranks
        if moments:
            ctx.render_tiles_moments(p, t[0][r].data_ptr(), t[1][r].data_ptr(), None)
        else:
            ctx.render_tiles(p, t[0][r].data_ptr(), None)
    p.tileFirst, p.tileStride = 0, 1
    img = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    q = abi.default_render_params(W, H, p.spp, p.maxBounce)
    q.tileStride = ranks
    for k in range(2 if moments else 1):
        ctx.resolve_tiles(q, t[k].data_ptr(), None, img[k].data_ptr(), None)
    torch.cuda.synchronize()
    return img[0].cpu().numpy(), (img[1].cpu().numpy() if moments else None)


def _lum(L):
    return (F(0.2126) * L[..., 0] + F(0.7152) * L[..., 1]) + F(0.0722) * L[..., 2]


def _samples(ctx, abi, p, n):
    """Each sample's colour, from n one-sample renders (sampleFirst = s): a one-sample float sum is the sample itself."""
    out = []
    for s in range(n):
        q = abi.default_render_params(p.imageWidth, p.imageHeight, 1, p.maxBounce, seed=p.seed, traversal=p.traversal,
                                      spp_chunks=1, sample_first=p.sampleFirst + s)
        acc, _ = ctx.render_image(q, want_rgba=False)
        out.append(acc[..., :3].copy())
    return out


def _fixed_sum(partials, limit):
    """The exact chunk sum of srt_path.h (toFixed36 / fromFixed36) over float32 partial sums, restated."""
    q = np.zeros(partials[0].shape, np.int64)
    nan, pinf, ninf = (np.zeros(partials[0].shape, bool) for _ in range(3))
    for v in partials:
        av = np.abs(v)
        ok = av < limit  # false for NaN, inf and at or beyond the limit
        m = np.floor(np.where(ok, av, 0).astype(np.float64) * 2.0 ** 36).astype(np.int64)
        q += np.where(v < 0, -m, m)
        nan |= np.isnan(v)
        pinf |= ~ok & ~np.isnan(v) & (v > 0)
        ninf |= ~ok & ~np.isnan(v) & ~(v > 0)
    out = (q.astype(np.float64) * 2.0 ** -36).astype(F)
    out = np.where(pinf, F(np.inf), out)
    out = np.where(ninf, F(-np.inf), out)
    return np.where(nan | (pinf & ninf), F(np.nan), out).astype(F)


def _expected_moments(samples, chunks):
    """{sum l, sum l^2, 0, n} as the kernels sum them: float running sums in sample order per chunk, exact chunk sums."""
    n = len(samples)
    ls = [_lum(L) for L in samples]
    base, rem = divmod(n, chunks)
    parts1, parts2, s = [], [], 0
    for c in range(chunks):
        k = base + (1 if c < rem else 0)
        a1 = np.zeros(ls[0].shape, F)
        a2 = np.zeros(ls[0].shape, F)
        for l in ls[s:s + k]:
            a1 = (a1 + l).astype(F)
            a2 = (a2 + (l * l).astype(F)).astype(F)
        parts1.append(a1)
        parts2.append(a2)
        s += k
    if chunks == 1:
        m1, m2 = parts1[0], parts2[0]
    else:
        pow2 = 1
        while pow2 < chunks:
            pow2 *= 2
        limit = F(2.0 ** 26 / pow2)
        m1, m2 = _fixed_sum(parts1, limit), _fixed_sum(parts2, limit)
    return np.stack([m1, m2, np.zeros_like(m1), np.full(m1.shape, F(n))], -1)


# ------------------------------------------------------------------ 1. the beauty is untouched


@pytest.mark.parametrize("case", ["chunks1", "chunks3", "default", "atomic", "split3"])
def test_beauty_is_bit_identical(ctx, dev, abi, srt, camera, node_path, case):
    _setup(ctx, srt, camera, "masterchief")
    chunks = {"chunks1": 1, "chunks3": 3, "default": 0, "atomic": 4, "split3": 0}[case]
    p = abi.default_render_params(80, 48, 24, 4, seed=5, spp_chunks=chunks)
    ranks = 3 if case == "split3" else 1
    saved = ctx.get_tunable("chunk_scratch_mb")
    try:
        if case == "atomic":
            ctx.set_tunable("chunk_scratch_mb", 0)
        plain, _ = _tiles(ctx, dev, abi, p, ranks, moments=False)
        info = ctx.launch_info()
        beauty, mom = _tiles(ctx, dev, abi, p, ranks)
        assert ctx.launch_info() == info
        assert _same(beauty, plain), case
        assert (mom[..., 3] == beauty[..., 3]).all() and (mom[..., 2] == 0).all()
        acc, rgba = ctx.render_image(p)
        acc2, mom2, rgba2 = ctx.render_image_moments(p)
        assert _same(acc2, acc) and np.array_equal(rgba2, rgba)
        assert _same(mom2, mom)
    finally:
        ctx.set_tunable("chunk_scratch_mb", saved)


def test_beauty_is_bit_identical_closest(ctx, dev, abi, srt, camera):
    _setup(ctx, srt, camera, "masterchief")
    for chunks in (1, 3):
        p = abi.default_render_params(80, 48, 12, 4, seed=6, spp_chunks=chunks, traversal=abi.SRT_TRAVERSE_CLOSEST)
        plain, _ = _tiles(ctx, dev, abi, p, moments=False)
        assert ctx.launch_info()["lds_tree_mode"] == 0
        beauty, mom = _tiles(ctx, dev, abi, p)
        assert _same(beauty, plain)
        samples = _samples(ctx, abi, p, p.spp)
        assert _same(mom, _expected_moments(samples, chunks)), chunks


# ------------------------------------------------------------------ 2. the moments, bit for bit


@pytest.mark.parametrize("scene", ["spheres", "iron", "masterchief"])
def test_moments_match_the_samples(ctx, dev, abi, srt, camera, node_path, scene):
    _setup(ctx, srt, camera, scene)
    n = 12
    p = abi.default_render_params(64, 36, n, 4, seed=3, spp_chunks=1)
    samples = _samples(ctx, abi, p, n)
    for chunks in (1, 4, 5):
        p.sppChunks = chunks
        _, mom, _ = ctx.render_image_moments(p, want_accum=False, want_rgba=False)
        want = _expected_moments(samples, chunks)
        bad = ~((np.isnan(mom) & np.isnan(want)) | (_bits(mom) == _bits(want)))
        assert not bad.any(), (scene, chunks, int(bad.sum()), np.argwhere(bad)[:3])
        # NaN / inf samples poison the moments as they poison rgb
        lum_bad = ~np.isfinite(np.stack([_lum(L) for L in samples])).all(0)
        assert (~np.isfinite(mom[..., 0]) == lum_bad).all() or chunks > 1


def test_moments_of_split_sample_ranges_add_up(ctx, dev, abi, srt, camera):
    _setup(ctx, srt, camera, "masterchief")
    p = abi.default_render_params(64, 36, 16, 4, seed=8, spp_chunks=0)
    _, whole, _ = ctx.render_image_moments(p)
    a = abi.default_render_params(64, 36, 6, 4, seed=8, spp_chunks=0)
    b = abi.default_render_params(64, 36, 10, 4, seed=8, spp_chunks=0, sample_first=6)
    _, ma, _ = ctx.render_image_moments(a)
    _, mb, _ = ctx.render_image_moments(b)
    fin = np.isfinite(whole[..., :2]).all(-1)
    sum_ = ma + mb
    assert (sum_[..., 3] == whole[..., 3]).all()
    assert np.allclose(sum_[fin][:, :2], whole[fin][:, :2], rtol=2e-5, atol=1e-6)


# ------------------------------------------------------------------ 3. order independence


def test_moments_do_not_depend_on_form_path_split_or_run(ctx, dev, abi, srt, camera):
    saved = {k: ctx.get_tunable(k) for k in ("lds_tree", "wavefront", "wf_resident_max", "chunk_scratch_mb")}
    p = abi.default_render_params(96, 56, 20, 4, seed=4, spp_chunks=5)
    runs = {}
    try:
        for form, (lds, wf, res) in {"wavefront": (1, 1, 0), "hybrid": (1, 1, 24), "lds_tree": (1, 0, 0), "l1_nodes": (0, 0, 0)}.items():
            ctx.set_tunable("lds_tree", lds)
            ctx.set_tunable("wavefront", wf)
            ctx.set_tunable("wf_resident_max", res)
            _setup(ctx, srt, camera, "masterchief")
            for mb in (12288, 0):
                ctx.set_tunable("chunk_scratch_mb", mb)
                for ranks in (1, 3):
                    runs[(form, mb, ranks)] = _tiles(ctx, dev, abi, p, ranks)[1]
            runs[(form, "again")] = _tiles(ctx, dev, abi, p, 1)[1]
    finally:
        for k, v in saved.items():
            ctx.set_tunable(k, v)
    first = next(iter(runs.values()))
    for k, m in runs.items():
        assert _same(m, first), k


# ------------------------------------------------------------------ 4. launch and errors


def test_launch_info_and_errors(ctx, dev, abi, srt, camera):
    import torch
    _setup(ctx, srt, camera, "masterchief")
    W, H = 64, 36
    nloc = dev.num_local_tiles(W, H, 1)
    acc = torch.full((nloc, 64, 4), 7.0, dtype=torch.float32, device="cuda")
    mom = torch.full((nloc, 64, 4), 7.0, dtype=torch.float32, device="cuda")
    tun = {k: ctx.get_tunable(k) for k in ("tile_block", "queues", "lds_tree", "wavefront", "chunk_scratch_mb", "wf_profile")}
    p = abi.default_render_params(W, H, 8, 4, seed=2, spp_chunks=0)
    ctx.render_tiles(p, acc.data_ptr(), None)
    info = ctx.launch_info()
    ctx.render_tiles_moments(p, acc.data_ptr(), mom.data_ptr(), None)
    assert ctx.launch_info() == info
    ms = ctx.last_kernel_ms()
    bad = [
        (abi.default_render_params(W, H, 8, 4, count_stats=1), True, "countStats"),
        (abi.default_render_params(W, H, 8, 4), False, "moments buffer"),
        (abi.default_render_params(W, H, 0, 4), True, "spp"),
        (abi.default_render_params(W, H, 8, 4, spp_chunks=9), True, "sppChunks"),
        (abi.default_render_params(W, H, 8, 4, tile_first=2, tile_stride=2), True, "tile split"),
        (abi.default_render_params(1, H, 8, 4), True, "2x2"),
    ]
    for q, with_moments, msg in bad:
        acc.fill_(7.0)
        mom.fill_(7.0)
        torch.cuda.synchronize()
        with pytest.raises(dev.SrtError, match=msg):
            ctx.render_tiles_moments(q, acc.data_ptr(), mom.data_ptr() if with_moments else None, None)
        torch.cuda.synchronize()
        assert (acc == 7.0).all() and (mom == 7.0).all(), msg  # nothing launched
        assert ctx.launch_info() == info and ctx.last_kernel_ms() == ms, msg
    with pytest.raises(dev.SrtError, match="countStats"):
        ctx.render_image_moments(abi.default_render_params(W, H, 8, 4, count_stats=1))
    with pytest.raises(dev.SrtError, match="countStats"):
        ctx.render_denoised_moments(abi.default_render_params(97, 61, 8, 4, count_stats=1))
    with pytest.raises(dev.SrtError, match="maxBounce"):
        ctx.render_aov(abi.default_render_params(97, 61, 8, 99))
    assert ctx.launch_info() == info and ctx.last_kernel_ms() == ms  # the blocking entries launched nothing either
    assert {k: ctx.get_tunable(k) for k in tun} == tun
    # wf_profile is ignored by a moments launch: the same bits and launch as without it
    want = _tiles(ctx, dev, abi, p)[1]
    ctx.set_tunable("wf_profile", 1)
    try:
        assert _same(_tiles(ctx, dev, abi, p)[1], want)
        assert ctx.launch_info()["lds_tree_mode"] == info["lds_tree_mode"]
    finally:
        ctx.set_tunable("wf_profile", tun["wf_profile"])


# ------------------------------------------------------------------ 5. the denoiser


def _device_frame(ctx, dev, abi, p):
    """Beauty, moments and the feature planes of one frame, resolved on the device: cuda tensors (H, W, 4)."""
    import torch
    W, H = p.imageWidth, p.imageHeight
    nloc = dev.num_local_tiles(W, H, 1)
    tiles = [torch.zeros((nloc, 64, 4), dtype=torch.float32, device="cuda") for _ in range(5)]
    ctx.render_tiles_moments(p, tiles[0].data_ptr(), tiles[4].data_ptr(), None)
    planes = abi.SRT_FEATURE_ALBEDO | abi.SRT_FEATURE_NORMAL | abi.SRT_FEATURE_DEPTH
    ctx.render_feature_tiles(p, planes, [tiles[1].data_ptr(), tiles[2].data_ptr(), None, tiles[3].data_ptr()], None)
    img = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(5)]
    for k in range(5):
        ctx.resolve_tiles(p, tiles[k].data_ptr(), None, img[k].data_ptr(), None)
    torch.cuda.synchronize()
    return img[0], [img[1], img[2], None, img[3]], img[4]


def _run(ctx, d, beauty, planes, moments):
    import torch
    H, W = beauty.shape[:2]
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.denoise(d, W, H, beauty.data_ptr(), [t.data_ptr() if t is not None else None for t in planes], out.data_ptr(),
                rgba.data_ptr(), None, d_moments_ptr=moments.data_ptr() if moments is not None else None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), rgba.cpu().numpy()


def _run_plain(ctx, dev, d, beauty, planes):
    """srtDenoiseMoments with dMoments = NULL, straight through ctypes (the binding routes None to srtDenoise)."""
    import torch
    H, W = beauty.shape[:2]
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    arr = (C.c_void_p * 4)(*[t.data_ptr() if t is not None else None for t in planes])
    assert dev.lib.srtDenoiseMoments(ctx.h, C.byref(d), W, H, beauty.data_ptr(), arr, None, out.data_ptr(), rgba.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), rgba.cpu().numpy()


def _compare(got, want, got_rgba, want_rgba, label):
    assert np.isfinite(got).all(), label
    assert np.array_equal(got[..., 3], want[..., 3]), label
    diff = np.abs(got[..., :3].astype(np.float64) - want[..., :3])
    rel = diff / np.maximum(np.abs(want[..., :3]), 1e-6)
    print("%s: max relative %.3g, mean absolute %.3g" % (label, rel.max(), diff.mean()))
    assert rel.max() <= REL_TOL, (label, rel.max(), np.unravel_index(rel.argmax(), rel.shape))
    assert diff.mean() <= MEAN_ABS_TOL, (label, diff.mean())
    assert np.abs(got_rgba.astype(int) - want_rgba.astype(int)).max() <= 1, label


CASES = [  # scene, width, height, spp, iterations, demodulate, sigmaL (0 = default)
    ("spheres", 160, 90, 8, 5, 0, 0),
    ("iron", 97, 61, 16, 1, 1, 0),
    ("masterchief", 160, 90, 8, 8, 1, 0),
    ("masterchief", 97, 61, 4, 3, 0, 6.0),
]


@pytest.mark.parametrize("case", CASES, ids=["%s-%dx%d-it%d-dm%d" % (c[0], c[1], c[2], c[4], c[5]) for c in CASES])
def test_denoise_moments_matches_reference(ctx, dev, abi, srt, camera, case):
    name, W, H, spp, it, dm, sl = case
    _setup(ctx, srt, camera, name)
    beauty, planes, moments = _device_frame(ctx, dev, abi, abi.default_render_params(W, H, spp, 4, seed=7, spp_chunks=0))
    d = abi.default_denoise_params(it, dm, sl)
    # NULL moments: srtDenoise bit for bit
    plain, plain_rgba = _run(ctx, d, beauty, planes, None)
    nul, nul_rgba = _run_plain(ctx, dev, d, beauty, planes)
    assert _same(nul, plain) and np.array_equal(nul_rgba, plain_rgba)
    got, got_rgba = _run(ctx, d, beauty, planes, moments)
    h = lambda t: t.cpu().numpy()  # noqa: E731
    want, want_rgba = RM.denoise(h(beauty), h(planes[1]), h(planes[3]), h(planes[0]), iterations=it, demodulate=bool(dm),
                                 sigma_l=sl, moments=h(moments))
    _compare(got, want, got_rgba, want_rgba, "%s %dx%d it=%d dm=%d" % (name, W, H, it, dm))
    assert not _same(got, plain)  # the sample variance changes the result
    # every count below 2: the spatial estimate everywhere, srtDenoise exactly
    low = moments.clone()
    low[..., 3] = 1.0
    one, one_rgba = _run(ctx, abi.default_denoise_params(it, dm, sl or abi.SRT_DENOISE_DEFAULT_SIGMA_LUMINANCE), beauty, planes, low)
    assert _same(one, plain) and np.array_equal(one_rgba, plain_rgba)


def test_blocking_entry_agrees_with_the_device_path(ctx, dev, abi, srt, camera):
    _setup(ctx, srt, camera, "masterchief")
    p = abi.default_render_params(160, 90, 8, 4, seed=11, spp_chunks=0)
    d = abi.default_denoise_params(5, 1)
    accum, moments, denoised, rgba = ctx.render_denoised_moments(p, d)
    acc_img, _ = ctx.render_image(p)
    assert _same(accum, acc_img)
    beauty, planes, mom = _device_frame(ctx, dev, abi, p)
    assert _same(moments, mom.cpu().numpy())
    out, out_rgba = _run(ctx, d, beauty, planes, mom)
    assert _same(out, denoised) and np.array_equal(out_rgba, rgba)


# ------------------------------------------------------------------ 6. quality: why this exists


def _display_mse(img, ref, mask):
    return float(np.mean((np.sqrt(np.maximum(img[mask], 0)) - np.sqrt(np.maximum(ref[mask], 0))) ** 2))


# denoised / noisy display MSE with the sample variance, measured: spheres 0.825 / 0.627, iron 0.672 / 0.465,
# masterchief 0.375 / 0.323 (without / with demodulation); the bounds keep margin
QUALITY = {"spheres": 1.0, "iron": 0.85, "masterchief": 0.5}


@pytest.mark.parametrize("scene", ["spheres", "iron", "masterchief"])
def test_sample_variance_improves_quality(ctx, abi, srt, camera, scene):
    """320x180, 16 spp against 1024 spp of the same frame, in display (sqrt) space, default sigmas: the sample variance
    beats the spatial estimate with and without demodulation."""
    _setup(ctx, srt, camera, scene)
    p = abi.default_render_params(320, 180, 16, 4, seed=1, spp_chunks=0)
    ref, _ = ctx.render_image(abi.default_render_params(320, 180, 1024, 4, seed=99, spp_chunks=0))
    ref = ref[..., :3] / ref[..., 3:4]
    for dm in (0, 1):
        d = abi.default_denoise_params(demodulate=dm)
        accum, spatial, _ = ctx.render_denoised(p, d)
        accum2, _, sample, _ = ctx.render_denoised_moments(p, d)
        assert _same(accum2, accum)
        noisy = accum[..., :3] / accum[..., 3:4]
        mask = np.isfinite(noisy).all(-1) & np.isfinite(ref).all(-1)
        base = _display_mse(noisy, ref, mask)
        r_spatial = _display_mse(spatial[..., :3], ref, mask) / base
        r_sample = _display_mse(sample[..., :3], ref, mask) / base
        print("%s dm=%d: denoised / noisy MSE spatial %.3f, sample variance %.3f" % (scene, dm, r_spatial, r_sample))
        assert r_sample < r_spatial, (scene, dm, r_sample, r_spatial)
        assert r_sample <= QUALITY[scene], (scene, dm, r_sample)


def test_cpp_example_writes_sample_variance_png(tmp_path, ctx, abi, srt, camera):
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
                           "--denoise", str(out), "--sample-variance"], env=env)
    _setup(ctx, srt, camera, "masterchief")
    p = abi.default_render_params(426, 240, 4, 4, seed=1, spp_chunks=0)
    _, _, _, rgba = ctx.render_denoised_moments(p)
    _, beauty_rgba = ctx.render_image(p)
    assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")), rgba)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "beauty.png").convert("RGBA")), beauty_rgba)
