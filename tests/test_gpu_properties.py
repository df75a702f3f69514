"""GPU tests through the C-ABI at BASELINE sizes via size-independent properties, plus the edge
cases of the domain (ragged tiles, no-BVH worlds, single-object leaves, moving spheres, missing
textures, the 1-bpp texel quirk, bounce limits) and the boundary's error behaviour."""
import ctypes as C
import zlib

import os

import numpy as np
import pytest

from conftest import render_counted

pytestmark = pytest.mark.gpu


def assert_counter(got, want, name):
    """Traversal counters equal the oracle's; a sample whose checker sign / texel / scatter test
    flips on a libm ulp (see test_gpu_parity's header) may change its path, so totals may move by a
    few parts per million."""
    assert abs(got - want) <= max(2, 2e-5 * want), (name, got, want)


def _render_tiles_all_ranks(ctx, dev, abi, p, nranks):
    """Renders every rank's tile share one after another on the one GPU and gathers them the
    way dist.gather would (rank-major), then resolves on the device."""
    import torch
    W, H = p.imageWidth, p.imageHeight
    nloc = dev.num_local_tiles(W, H, nranks)
    gathered = torch.zeros((nranks, nloc, 64, 4), dtype=torch.float32, device="cuda")
    for r in range(nranks):
        p.tileFirst, p.tileStride = r, nranks
        ctx.render_tiles(p, gathered[r].data_ptr(), None)
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    p.tileStride = nranks
    ctx.resolve_tiles(p, gathered.data_ptr(), rgba.data_ptr(), accum.data_ptr(), None)
    torch.cuda.synchronize()
    return accum.cpu().numpy(), rgba.cpu().numpy()


def test_720p_tile_split_invariance_and_determinism(ctx, dev, abi, srt, camera):
    """BASELINE 720p (configs 2-4 geometry) on the main.cpp scene: the image is bit-identical for
    1/2/3/8-way interleaved tile splits (SURVEY 8e invariant) and across repeated runs."""
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    p = abi.default_render_params(1280, 720, 4, 4, seed=31)
    ref_acc, ref_rgba = ctx.render_image(p)
    crc = zlib.crc32(ref_acc.tobytes())
    for n in (1, 2, 3, 8):
        acc, rgba = _render_tiles_all_ranks(ctx, dev, abi, abi.default_render_params(1280, 720, 4, 4, seed=31), n)
        assert zlib.crc32(acc.tobytes()) == crc, n
        assert np.array_equal(rgba, ref_rgba)
    # sky rows are pure background: sqrt-gamma of (0.53,0.81,0.92) -> 186,230,245, alpha 255
    assert (ref_rgba[:40, :, :] == np.array([186, 230, 245, 255])).all()
    assert (ref_acc[..., 3] == 4).all()


def test_sample_sum_linearity(ctx, abi, srt, camera):
    """Samples are keyed by (pixel, sample index): a chunked render equals the sequential one up to
    the re-association of the per-pixel sum, and chunks=spp still visits every sample once."""
    ctx.upload_scene(srt.scenes.scene_spheres())
    ctx.set_camera(camera)
    p = abi.default_render_params(426, 240, 32, 8, seed=8)
    seq, _ = ctx.render_image(p)
    for chunks in (2, 5, 32):
        p.sppChunks = chunks
        ch, _ = ctx.render_image(p)
        assert (ch[..., 3] == 32).all()
        np.testing.assert_allclose(ch[..., :3], seq[..., :3], rtol=2e-5, atol=1e-6)
    # the library's own plan (0 = srtDefaultSppChunks(spp) equal chunks): every sample exactly once, and the
    # same per-pixel summation order for any tile split
    for spp in (64, 100, 333):
        p = abi.default_render_params(426, 240, spp, 8, seed=8)
        seq, _ = ctx.render_image(p)
        p.sppChunks = 0
        auto, _ = ctx.render_image(p)
        assert (auto[..., 3] == spp).all()
        np.testing.assert_allclose(auto[..., :3], seq[..., :3], rtol=2e-5, atol=1e-6)
    import torch
    from importlib import import_module
    tiles = import_module("sexy-raytracer_amd.tiles")
    dev = srt.device()
    nloc = dev.num_local_tiles(426, 240, 3)
    parts = []
    for r in range(3):
        buf = torch.zeros((nloc, 64, 4), dtype=torch.float32, device="cuda")
        ctx.render_tiles(abi.default_render_params(426, 240, 333, 8, seed=8, tile_first=r, tile_stride=3, spp_chunks=0),
                         buf.data_ptr())
        torch.cuda.synchronize()
        parts.append(buf.cpu().numpy())
    joined = np.ascontiguousarray(tiles.untile(np.stack(parts), 426, 240, 3), dtype=np.float32)
    assert np.array_equal(joined.view(np.uint32), np.ascontiguousarray(auto).view(np.uint32))  # bit patterns: NaN-safe
    p = abi.default_render_params(426, 240, 32, 8, seed=8)
    seq, _ = ctx.render_image(p)
    # different seed -> different image, same statistics
    p.seed = 9
    other, _ = ctx.render_image(p)
    assert not np.array_equal(other, seq)
    assert abs(other[..., :3].mean() - seq[..., :3].mean()) < 0.01 * seq[..., :3].mean()


def test_hybrid_form_on_odd_shapes(ctx, dev, abi, srt, camera):
    """The path-pool kernel's hybrid form (what a tree beyond LDS gets by default) against the 256-thread kernel where its
    bookkeeping is least comfortable: more bounces than a context line holds attenuations for, frames smaller than a
    workgroup's pool of contexts, a rank's share of the tiles, a sample range that starts late (progressive pass), one
    chunk and many.  Same accumulators, bit for bit."""
    import torch
    sb = srt.scenes.scene_soup(30000, seed=9, extent=5.0, size=0.12)
    cases = [  # width, height, spp, bounces, chunks, tile_first, tile_stride, sample_first
        (33, 17, 3, 12, 1, 0, 1, 0), (200, 120, 24, 9, 0, 0, 1, 0), (320, 180, 16, 6, 5, 2, 3, 0), (160, 90, 8, 4, 0, 0, 1, 40)]
    out = {}
    for hybrid in (1, 0):
        ctx.set_tunable("wf_hybrid", hybrid)
        try:
            ctx.upload_scene(sb)
        finally:
            ctx.set_tunable("wf_hybrid", 1)
        ctx.set_camera(camera)
        for case in cases:
            w, h, spp, mb, chunks, first, stride, s0 = case
            p = abi.default_render_params(w, h, spp, mb, seed=21, spp_chunks=chunks, tile_first=first, tile_stride=stride, sample_first=s0)
            local = torch.zeros((dev.num_local_tiles(w, h, stride), 64, 4), dtype=torch.float32, device="cuda")
            ctx.render_tiles(p, local.data_ptr(), None)
            torch.cuda.synchronize()
            ctx.last_kernel_ms()  # raises if a path-pool workgroup gave up
            assert ctx.launch_info()["lds_tree_mode"] == (4 if hybrid else 0), (case, ctx.launch_info())
            out[(hybrid, case)] = local.cpu().numpy()
    for case in cases:
        a, b = out[(1, case)], out[(0, case)]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), case
        assert (a[..., 3] > 0).any()


def test_image_independent_of_work_distribution(ctx, abi, srt, camera):
    """The tile order, the number of work queues and the unit size decide only WHO renders WHAT WHEN
    (csrc/srt_kernels.hip "work queues"): the image must not change, also when every queue has to be
    stolen from (more queues than units) and for frames that are not a whole number of tiles/blocks."""
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    for (w, h, spp) in ((203, 117, 48), (64, 8, 70)):
        p = abi.default_render_params(w, h, spp, 4, seed=11, spp_chunks=0)
        defaults = {k: ctx.get_tunable(k) for k in ("queues", "unit_tiles", "tile_block")}
        want, want_rgba = ctx.render_image(p)
        assert (want[..., 3] == spp).all()
        for queues, unit, block in ((1, 8, 8), (64, 1, 8), (64, 16, 8), (7, 3, 5), (8, 8, 1), (64, 1024, 16)):
            ctx.set_tunable("queues", queues)
            ctx.set_tunable("unit_tiles", unit)
            ctx.set_tunable("tile_block", block)
            got, got_rgba = ctx.render_image(p)
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (queues, unit, block)
            assert np.array_equal(got_rgba, want_rgba)
        for k, v in defaults.items():
            ctx.set_tunable(k, v)


def test_exact_chunk_sum_paths_agree(ctx, dev, abi, srt, camera):
    """The chunk sums of a pixel are added exactly (64-bit fixed point), by chunk slots + a summing kernel
    while the frame's slots fit the memory budget and by integer atomics beyond it (32 B per pixel for any
    chunk count): the two must give the same bits, for whole frames and for a rank's share of the tiles, NaN
    pixels included (the r = 0 ground BRDF of the main.cpp scene produces them)."""
    import torch
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    budget = ctx.get_tunable("chunk_scratch_mb")
    try:
        for (w, h, spp, chunks, first, stride) in ((203, 117, 48, 0, 0, 1), (426, 240, 96, 7, 0, 1), (426, 240, 96, 7, 1, 3)):
            p = abi.default_render_params(w, h, spp, 4, seed=17, spp_chunks=chunks, tile_first=first, tile_stride=stride)
            out = {}
            for mb in (budget, 0):
                ctx.set_tunable("chunk_scratch_mb", mb)
                if stride == 1:
                    out[mb] = ctx.render_image(p)[0]
                else:
                    local = torch.zeros((dev.num_local_tiles(w, h, stride), 64, 4), dtype=torch.float32, device="cuda")
                    ctx.render_tiles(p, local.data_ptr(), None)
                    torch.cuda.synchronize()
                    out[mb] = local.cpu().numpy()
            a, b = (np.ascontiguousarray(out[k]).view(np.uint32) for k in (budget, 0))
            assert np.array_equal(a, b), (w, h, spp, chunks, first, stride)
            if stride == 1:
                assert (out[0][..., 3] == spp).all()
    finally:
        ctx.set_tunable("chunk_scratch_mb", budget)


def test_chunk_sums_cannot_wrap_on_fireflies(ctx, abi, camera):
    """a few chunk sums near 2^26 used to wrap the 64-bit fixed-point pixel sum negative (a black pixel where
    the reference's float sum gives white).  A partial sum of 2^26 / (chunk count rounded up to a power of two) or more
    now counts as infinite.  A light of radiance 3e7 seen directly: with 64 chunks (limit 2^20) and with 4 chunks (limit
    2^24) every chunk sum over the light is beyond the limit: the scratch path, the atomic path
    and the single float sum must all resolve to the same white pixels, the two exact paths bit-identical, and nothing
    anywhere may come out negative or NaN."""
    sb = abi.SceneBuilder()
    sb.add_sphere((0.0, 2.5, 0.0), 1.5, sb.light((3.0e7, 2.0e7, 4.0e7)))
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.pbr(albedo=(0.8, 0.8, 0.8, 1.0), roughness=0.5))
    sb.world_bvh(0, None, 0.0, 1.0)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    budget = ctx.get_tunable("chunk_scratch_mb")
    try:
        single_acc, single = ctx.render_image(abi.default_render_params(160, 90, 64, 4, seed=23, spp_chunks=1))
        assert (single[..., :3] == 255).all(axis=-1).mean() > 0.02  # the light is in the picture
        for chunks in (64, 4):
            out = {}
            for mb in (budget, 0):
                ctx.set_tunable("chunk_scratch_mb", mb)
                out[mb] = ctx.render_image(abi.default_render_params(160, 90, 64, 4, seed=23, spp_chunks=chunks))
            (acc_s, rgba_s), (acc_a, rgba_a) = out[budget], out[0]
            assert np.array_equal(acc_s.view(np.uint32), acc_a.view(np.uint32)), chunks
            assert np.array_equal(rgba_s, rgba_a) and np.array_equal(rgba_s, single), chunks
            assert not np.isnan(acc_s).any() and (acc_s[..., :3] >= 0).all(), chunks
            lit = (single[..., :3] == 255).all(axis=-1)
            assert np.isinf(acc_s[lit][:, :3]).any(), chunks  # beyond the limit: counted as infinite, not wrapped
            finite = np.isfinite(acc_s[..., :3]).all(axis=-1)
            assert np.allclose(acc_s[finite][:, :3], single_acc[finite][:, :3], rtol=2e-5, atol=1e-6)
    finally:
        ctx.set_tunable("chunk_scratch_mb", budget)


def test_ragged_and_tiny_images(ctx, oracle, abi, srt, camera):
    sb = srt.scenes.scene_spheres()
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    osc = oracle.OracleScene(sb)
    for (w, h) in ((9, 9), (2, 2), (17, 5), (426, 3)):
        p = abi.default_render_params(w, h, 3, 8, seed=4)
        acc, rgba = ctx.render_image(p)
        want, want_rgba, _ = osc.render(camera, p, oracle.RNG_COUNTER, threads=2)
        bit = (acc.view(np.uint32) == want.view(np.uint32)).all(axis=-1)
        assert bit.mean() >= 0.97 and np.allclose(acc, want, rtol=1e-3, atol=1e-6)
        assert np.abs(rgba.astype(int) - want_rgba.astype(int)).max() <= 1


def test_bounce_limits(ctx, abi, srt, camera, node_path):
    ctx.upload_scene(srt.scenes.scene_spheres())
    ctx.set_camera(camera)
    p = abi.default_render_params(64, 36, 2, 0, seed=1)
    acc, rgba = ctx.render_image(p)  # main.cpp:36-37: no bounces -> black, nothing traced
    assert (acc[..., :3] == 0).all() and (rgba[..., :3] == 0).all() and (rgba[..., 3] == 255).all()
    p.maxBounce = 1  # only misses (background) and lights contribute
    acc, _ = ctx.render_image(p)
    bg = np.array([0.53, 0.81, 0.92], np.float32)
    px = acc[..., :3] / 2
    is_bg = np.isclose(px, bg).all(axis=-1)
    is_black = (px == 0).all(axis=-1)
    assert (is_bg | is_black | np.isclose(px, bg / 2).all(axis=-1)).all() and is_bg.any() and is_black.any()


def _world_variants(abi):
    def three(sb):
        m1, m2 = sb.metal((0.8, 0.7, 0.6), 0.2), sb.dielectric(1.5)
        sb.add_sphere((0.0, 2.0, 0.0), 1.0, m1)
        sb.add_sphere((-2.2, 2.0, 0.0), 1.0, m2)
        sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.pbr(albedo_tex=sb.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))))
    out = {}
    sb = abi.SceneBuilder(); three(sb)
    for i in range(3):
        sb.world_prim(i)            # plain hittableList, no BVH (main.cpp:153 `return objects`)
    out["list"] = sb
    sb = abi.SceneBuilder(); three(sb)
    sb.world_bvh(0, 1); sb.world_bvh(1, 2)   # span-1 leaf (left == right) + span-2 node, two roots
    out["two_bvh"] = sb
    sb = abi.SceneBuilder()
    m = sb.metal((0.7, 0.6, 0.5), 0.0)
    rng = np.random.default_rng(12)
    for _ in range(23):             # moving spheres, sphere.h:47-52
        c = rng.uniform(-3, 3, 3) + np.array([0, 3, -1])
        sb.add_sphere(tuple(c), 0.4, m, center1=tuple(c + rng.uniform(-0.4, 0.4, 3)), time0=0.0, time1=1.0)
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.pbr(albedo_tex=sb.solid(120.0, 130.0, 140.0), roughness=0.4))
    sb.world_bvh(0, None, 0.0, 1.0)
    out["moving"] = sb
    sb = abi.SceneBuilder()
    tex = np.arange(7 * 5, dtype=np.uint8).reshape(5, 7, 1) * 7
    missing = sb.image(None, 3)     # failed load -> (1,0,1), texture.h:130-131
    onebpp = sb.image(tex, 1)       # roughness reads pixel[1] = next texel, overrun at the end (texture.h:147)
    rgb = sb.image((np.arange(6 * 4 * 3, dtype=np.uint8).reshape(4, 6, 3) * 3), 3)
    sb.add_sphere((0.0, 2.0, 0.0), 1.5, sb.pbr(albedo_tex=missing, metallic_tex=onebpp, roughness_tex=onebpp))
    sb.add_sphere((3.0, 2.0, 0.0), 1.0, sb.pbr(albedo_tex=rgb, normal_tex=rgb, albedo=(0.9, 0.8, 0.7, 1.0), metalness=0.3, roughness=0.6))
    sb.add_sphere((-3.5, 3.0, 1.0), 0.7, sb.light((4.0, 3.0, 2.0)))
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.pbr(albedo_tex=sb.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))))
    sb.world_bvh(0, None, 0.0, 1.0)
    out["textures"] = sb
    # the ways a shading record's slots can be filled (srt_kernels.hip "materials") beyond the variants above: lights
    # emitting an image and a checker, a 4-byte image in all four pbr slots, an image wider than a packed slot takes
    sb = abi.SceneBuilder()
    rgba = sb.image((np.arange(9 * 5 * 4, dtype=np.uint8).reshape(5, 9, 4) * 5 + 11), 4)
    rgb = sb.image((np.arange(6 * 4 * 3, dtype=np.uint8).reshape(4, 6, 3) * 3 + 40), 3)
    wide = sb.image(np.tile(np.arange(40000, dtype=np.uint32)[None, :, None] % 251, (1, 1, 3)).astype(np.uint8), 3)  # 40000 x 1
    sb.add_sphere((-3.0, 2.5, 0.5), 0.8, sb.light(emit_tex=rgba))
    sb.add_sphere((3.2, 3.0, -0.5), 0.6, sb.light(emit_tex=sb.checker((3.0, 0.5, 0.5), (0.5, 0.5, 3.0))))
    sb.add_sphere((0.0, 1.5, 0.0), 1.5, sb.pbr(albedo_tex=rgba, normal_tex=rgba, metallic_tex=rgba, roughness_tex=rgba))
    sb.add_sphere((2.5, 1.0, 1.5), 1.0, sb.pbr(albedo_tex=wide, roughness_tex=rgb, metalness=0.2))
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.pbr(albedo_tex=rgb, roughness=0.7))
    sb.world_bvh(0, None, 0.0, 1.0)
    out["slots"] = sb
    return out


@pytest.mark.parametrize("variant", ["list", "two_bvh", "moving", "textures", "slots"])
def test_world_and_material_variants_vs_oracle(ctx, oracle, abi, camera, variant, node_path):
    sb = _world_variants(abi)[variant]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    osc = oracle.OracleScene(sb)
    p = abi.default_render_params(160, 90, 8, 6, seed=77, count_stats=1)
    acc, rgba = render_counted(ctx, p, node_path)
    st = ctx.stats()
    want, want_rgba, want_st = osc.render(camera, p, oracle.RNG_COUNTER, threads=4)
    assert np.array_equal(np.isnan(acc), np.isnan(want))
    bit = (acc.view(np.uint32) == want.view(np.uint32)).all(axis=-1)
    assert bit.mean() >= 0.995, bit.mean()
    ok = np.isnan(want) | (np.abs(acc - want) <= 0.05 * np.maximum(np.abs(want), 1e-3) + 0.05)
    assert ok.all()
    assert np.abs(rgba.astype(int) - want_rgba.astype(int)).max() <= 3
    for k in ("samples", "rays", "nodeVisits", "boxPasses", "triTests", "sphereTests", "texelFetches"):
        assert_counter(st[k], want_st[k], k)


def test_soup_scene_trace_and_render(ctx, oracle, abi, srt, camera):
    """Synthetic 20k-triangle soup (deeper tree, degenerate slivers): bit-exact trace, close render."""
    sb = srt.scenes.scene_soup(20000, seed=3)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    osc = oracle.OracleScene(sb)
    assert ctx.bvh(0).tobytes() == osc.bvh(0)[0].tobytes()
    rng = np.random.default_rng(2)
    rays = np.zeros(20000, abi.RAY_DTYPE)
    rays["o"] = (0.0, 3.0, 5.0)
    rays["d"] = rng.normal(size=(len(rays), 3)).astype(np.float32)
    rays["tMin"], rays["tMax"] = 0.001, np.inf
    want, got = osc.trace(rays), ctx.trace(rays)
    assert np.array_equal(got["prim"], want["prim"])
    m = want["prim"] >= 0
    assert np.array_equal(got["t"][m].view(np.uint32), want["t"][m].view(np.uint32))
    for f in ("nodeVisits", "boxPasses", "triTests", "sphereTests"):
        assert np.array_equal(got[f], want[f])
    p = abi.default_render_params(160, 90, 4, 4, seed=6)
    acc, _ = ctx.render_image(p)
    # 40 k nodes: beyond LDS and beyond 16-bit references -- the path-pool kernel's hybrid form with its 32-bit links
    assert ctx.launch_info()["lds_tree_mode"] == 4, ctx.launch_info()
    wacc, _, _ = osc.render(camera, p, oracle.RNG_COUNTER, threads=8, want_stats=False)
    bit = (acc.view(np.uint32) == wacc.view(np.uint32)).all(axis=-1)
    assert bit.mean() >= 0.995


def test_error_behaviour(dev, abi, srt, camera):
    """int return codes + text from srtLastError, never an exception or a silent fallback."""
    c = dev.Context(0)
    p = abi.default_render_params(64, 36, 1, 4)
    with pytest.raises(dev.SrtError, match="no scene"):
        c.render_image(p)
    sb = srt.scenes.scene_spheres()
    c.upload_scene(sb)
    with pytest.raises(dev.SrtError, match="no camera"):
        c.render_image(p)
    c.set_camera(camera)
    for field, bad in (("spp", 0), ("maxBounce", 99), ("imageWidth", 1), ("sppChunks", -1), ("sppChunks", 2)):
        q = abi.default_render_params(64, 36, 1, 4)
        setattr(q, field, bad)
        with pytest.raises(dev.SrtError):
            c.render_image(q)
    d = srt.scenes.scene_spheres().desc()
    d.materials[0].albedoTex = 1234
    assert dev.lib.srtUploadScene(c.h, C.byref(d)) != 0
    assert b"texture id" in dev.lib.srtLastError(c.h)
    h = C.c_void_p()
    assert dev.lib.srtCreate(4096, C.byref(h)) != 0
    c.close()


def test_progressive_passes_checkpoint_and_resume(tmp_path, ctx, oracle, abi, srt, camera):
    """Two passes of 8 samples (with a checkpoint written and resumed in between) add up bit for bit
    to one 16-sample render whose per-pixel sum is taken as two 8-sample chunks -- and each pass is the
    ORACLE's render of that sample range (SrtRenderParams.sampleFirst, absolute sample indices in the RNG
    keys), so the passes are pinned to the CPU restatement, not only to each other.  A checkpoint is
    refused on a context that holds another scene."""
    import importlib
    from test_gpu_parity import assert_accum_close
    prog = importlib.import_module("sexy-raytracer_amd.progressive")
    sb = srt.scenes.scene_masterchief()
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    osc = oracle.OracleScene(sb)
    pr = prog.ProgressiveRender(ctx, abi, 160, 90, 4, seed=21)
    pr.render_pass(8)
    want0, _, _ = osc.render(camera, abi.default_render_params(160, 90, 8, 4, seed=21, sample_first=0), oracle.RNG_COUNTER, want_rgba=False)
    assert_accum_close(pr.accum, want0)
    ck = str(tmp_path / "ck.npz")
    pr.save(ck)
    pr2 = prog.ProgressiveRender.resume(ctx, abi, ck)
    assert pr2.next_sample == 8
    pr2.render_pass(8)
    want1, _, _ = osc.render(camera, abi.default_render_params(160, 90, 8, 4, seed=21, sample_first=8), oracle.RNG_COUNTER, want_rgba=False)
    sum01 = want0.copy()
    sum01 += want1
    assert_accum_close(pr2.accum, sum01)
    assert not np.array_equal(want0, want1)  # the second pass drew other samples
    want, want_rgba = ctx.render_image(abi.default_render_params(160, 90, 16, 4, seed=21, spp_chunks=2))
    assert pr2.accum.tobytes() == want.tobytes()
    assert np.array_equal(pr2.image_rgba8(), want_rgba)
    ctx.upload_scene(srt.scenes.scene_spheres())
    with pytest.raises(ValueError):
        prog.ProgressiveRender.resume(ctx, abi, ck)


def _tree_checks(nodes, num_prims):
    """A valid binary tree over num_prims leaves: every primitive referenced once, every internal
    node except the root referenced once, every box the union of its children's boxes."""
    n = len(nodes)
    assert n == max(num_prims - 1, 1)
    refs = np.concatenate([nodes["left"], nodes["right"]]) if num_prims > 1 else nodes["left"]
    prims = ~refs[refs < 0]
    assert sorted(prims.tolist()) == list(range(num_prims))
    inner = refs[refs >= 0]
    assert sorted(inner.tolist()) == list(range(1, n))
    return True


@pytest.mark.parametrize("builder", ["LBVH", "PLOC"])
def test_device_lbvh_build_and_closest_hit(ctx, oracle, abi, srt, camera, builder):
    """the device-built trees (linear BVH; PLOC).  The closest hit does not depend on the
    tree, so CLOSEST traversal of the device tree must reproduce the oracle's brute-force closest hit bit
    for bit, and CLOSEST renders through the device tree and through the reference tree must agree."""
    n = 30000
    builder = getattr(abi, "SRT_BUILDER_" + builder)
    sb = srt.scenes.scene_soup(n, seed=5, builder=builder)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    nodes = ctx.bvh(0)
    assert _tree_checks(nodes, n + 1)
    # boxes: every parent's box is exactly the union of its children's -- the bitwise min / max of the two boxes, a leaf's
    # being its primitive's box (tests/tree_build_ref.py prim_boxes) over the item's time range
    import tree_build_ref
    leaf_mn, leaf_mx = tree_build_ref.prim_boxes(sb, np.arange(n + 1), 0.0, 1.0)
    kids = []
    for child in ("left", "right"):
        c = nodes[child]
        inner, node, prim = (c >= 0)[:, None], np.maximum(c, 0), np.maximum(~c, 0)
        kids.append((np.where(inner, nodes["bmin"][node], leaf_mn[prim]), np.where(inner, nodes["bmax"][node], leaf_mx[prim])))
    assert np.array_equal(nodes["bmin"].view(np.uint32), np.minimum(kids[0][0], kids[1][0]).view(np.uint32))
    assert np.array_equal(nodes["bmax"].view(np.uint32), np.maximum(kids[0][1], kids[1][1]).view(np.uint32))
    assert 15 <= ctx.bvh_depth() <= 64
    if builder == abi.SRT_BUILDER_PLOC:
        # children are numbered after their parents (creation order reversed)
        for child in ("left", "right"):
            c = nodes[child]
            assert (c[c >= 0] > np.nonzero(c >= 0)[0]).all()
    rng = np.random.default_rng(9)
    rays = np.zeros(40000, abi.RAY_DTYPE)
    rays["o"] = (0.0, 3.0, 5.0)
    rays["d"] = rng.normal(size=(len(rays), 3)).astype(np.float32)
    rays["tMin"], rays["tMax"] = 0.001, np.inf
    got = ctx.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    want = oracle.OracleScene(sb).trace(rays, abi.SRT_TRAVERSE_CLOSEST)  # brute force over all primitives
    assert np.array_equal(got["prim"] >= 0, want["prim"] >= 0)
    m = want["prim"] >= 0
    assert np.array_equal(got["t"][m].view(np.uint32), want["t"][m].view(np.uint32))
    assert (got["prim"][m] != want["prim"][m]).mean() < 1e-3  # exact ties only
    p = abi.default_render_params(160, 90, 4, 4, seed=3, traversal=abi.SRT_TRAVERSE_CLOSEST)
    acc_dev, _ = ctx.render_image(p)
    ctx.upload_scene(srt.scenes.scene_soup(n, seed=5))  # same scene, the reference's tree
    acc_ref, _ = ctx.render_image(p)
    same = (acc_dev.view(np.uint32) == acc_ref.view(np.uint32)).all(axis=-1)
    assert same.mean() > 0.999


@pytest.mark.parametrize("builder", ["LBVH", "PLOC"])
def test_device_builders_on_duplicated_geometry(ctx, oracle, abi, srt, builder):
    """Many identical primitives (equal boxes, equal Morton keys, equal merge costs): the builders must
    neither fail nor degenerate into one merge per round (the call would not return in test time)."""
    n = 20000
    sb = abi.SceneBuilder()
    mat = sb.pbr(albedo_tex=sb.solid(200, 150, 100), metalness=0.0, roughness=0.5)
    tri = np.array([[-1.0, 2.0, -1.0], [1.0, 2.0, -1.0], [0.0, 4.0, -1.0]], np.float32)
    pos = np.tile(tri, (n, 1))
    pos[3 * (n // 2):] += np.float32(2.5)  # two stacks of identical triangles
    sb.add_triangles(pos, np.zeros((3 * n, 2), np.float32), np.arange(3 * n, dtype=np.int32).reshape(-1, 3), mat)
    sb.world_bvh(0, None, 0.0, 1.0, builder=getattr(abi, "SRT_BUILDER_" + builder))
    ctx.upload_scene(sb)
    assert _tree_checks(ctx.bvh(0), n)
    rng = np.random.default_rng(2)
    rays = np.zeros(2000, abi.RAY_DTYPE)
    rays["o"] = (0.5, 3.0, 5.0)
    rays["d"] = rng.normal(size=(len(rays), 3)).astype(np.float32) * np.float32(0.3) + np.array([0.1, 0.0, -1.0], np.float32)
    rays["tMin"], rays["tMax"] = 0.001, np.inf
    got = ctx.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    want = oracle.OracleScene(sb).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    assert np.array_equal(got["prim"] >= 0, want["prim"] >= 0) and (want["prim"] >= 0).any()
    m = want["prim"] >= 0
    assert np.array_equal(got["t"][m].view(np.uint32), want["t"][m].view(np.uint32))


@pytest.mark.parametrize("builder", ["LBVH", "PLOC"])
def test_device_lbvh_small_and_moving(ctx, oracle, abi, camera, builder):
    for count in (1, 2, 3, 37):
        sb = abi.SceneBuilder()
        m = sb.metal((0.7, 0.6, 0.5), 0.1)
        rng = np.random.default_rng(count)
        for _ in range(count):
            c = rng.uniform(-3, 3, 3) + np.array([0, 3, -1])
            sb.add_sphere(tuple(c), 0.5, m, center1=tuple(c + rng.uniform(-0.4, 0.4, 3)), time0=0.0, time1=1.0)
        sb.world_bvh(0, None, 0.0, 1.0, builder=getattr(abi, "SRT_BUILDER_" + builder))
        ctx.upload_scene(sb)
        ctx.set_camera(camera)
        assert _tree_checks(ctx.bvh(0), count)
        rng = np.random.default_rng(1)
        rays = np.zeros(5000, abi.RAY_DTYPE)
        rays["o"] = (0.0, 3.0, 5.0)
        rays["d"] = rng.normal(size=(len(rays), 3)).astype(np.float32)
        rays["time"] = rng.random(len(rays)).astype(np.float32)
        rays["tMin"], rays["tMax"] = 0.001, np.inf
        got = ctx.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
        want = oracle.OracleScene(sb).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
        assert np.array_equal(got["prim"], want["prim"])
        mm = want["prim"] >= 0
        assert np.array_equal(got["t"][mm].view(np.uint32), want["t"][mm].view(np.uint32))


def test_headline_frame_against_published_render(ctx, abi, srt, camera):
    """The headline config itself (1280x720, 5000 spp, 4 bounces: 4.6 G samples, ~2 s) against the
    reference's published render images/test-5kx720p.png (tests/golden/published_regions.json): region
    means within a few 8-bit levels (sky exact).  Statistical: different RNG streams, and the iron
    sphere (missing texture blobs, procedural stand-ins) is excluded.  The published image has 146
    pure-black pixels (NaN samples of the r = 0 ground BRDF); the NaN rate here must be of
    the same order."""
    import json
    import os
    from conftest import GOLD
    pub = json.load(open(os.path.join(GOLD, "published_regions.json")))["test-5kx720p.png"]
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    _, rgba = ctx.render_image(abi.default_render_params(1280, 720, 5000, 4, seed=1, spp_chunks=0), want_accum=False)
    img = rgba[..., :3].astype(np.float64)
    tol = {"sky": 0.01, "far_ground": 2.5, "metal_sphere": 2.5, "ground": 3.0, "chief": 4.0}
    for name, t in tol.items():
        y0, y1, x0, x1 = pub["regions"][name]["rows_cols"]
        mean = img[y0:y1, x0:x1].mean((0, 1))
        assert np.abs(mean - pub["regions"][name]["mean_rgb"]).max() <= t, (name, mean, pub["regions"][name]["mean_rgb"])
    black = int((rgba[..., :3].sum(-1) == 0).sum())
    assert black < 20 * max(1, pub["black_pixels"]), black


def test_headline_frame_pooled_residuals_vs_published(ctx, abi, srt, camera):
    """The strong statistical pin: the headline frame (1280x720, 5000 spp) against the
    reference's published render of the same config block by block (tests/published.py, fixture made by
    tests/make_golden.py from images/test-5kx720p.png: 57 600 block means instead of five region means).
      * signed bias over all blocks lying wholly on the mesh / ground / metal sphere / sky: a wrong uv
        formula, v flip, normal-map axis or Fresnel constant shows here;
      * the mean absolute block difference halves each time the pool side doubles (4 -> 8 -> 16 -> 32 px):
        what is left is the Monte-Carlo noise of two independent 5000-spp renders, nothing systematic;
      * pure-black pixels (NaN samples of the r = 0 ground BRDF): same count within a factor of
        two of the published image's 146, and where theirs are: four fifths on the ground, the rest on
        surfaces that see the ground in a bounce (a NaN radiance poisons the whole path).
    The iron sphere is masked out (its texture blobs are missing from the reference; stand-ins here)."""
    import published
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    _, rgba = ctx.render_image(abi.default_render_params(1280, 720, 5000, 4, seed=1, spp_chunks=0), want_accum=False)
    r = published.compare(rgba[..., :3].astype(np.float64), "720p")
    print("published-image residuals:", r)
    assert abs(r["bias"]["sky"]) <= 0.02, r
    assert abs(r["bias"]["ground"]) <= 0.3, r
    assert abs(r["bias"]["mesh"]) <= 0.3, r
    assert abs(r["bias"]["metal"]) <= 0.5, r
    mad = r["mad"]
    assert mad[4] <= 0.8 and mad[16] <= 0.25, mad  # measured 0.44 / 0.12 (two independent 5000-spp renders)
    for a, b in ((4, 8), (8, 16), (16, 32)):
        assert 0.40 <= mad[b] / mad[a] <= 0.64, (a, b, mad)
    black = np.argwhere(rgba[..., :3].sum(-1) == 0)
    pub_black = published.published_black("720p")
    assert 0.5 * len(pub_black) <= len(black) <= 2.0 * len(pub_black), (len(black), len(pub_black))
    cls = np.load(os.path.join(published.GOLD, "published_blocks.npz"))["720p_class"]
    mine_ground = (cls[black[:, 0], black[:, 1]] == published.CLASSES["ground"]).mean()
    pub_ground = (cls[pub_black[:, 0], pub_black[:, 1]] == published.CLASSES["ground"]).mean()  # 116 of 146
    assert abs(mine_ground - pub_ground) <= 0.2


def test_240p_frame_against_published_render(ctx, abi, srt, camera):
    """The other published render, images/test-1kx240p.png (426x240, ~1000 spp)."""
    import json
    import os
    from conftest import GOLD
    pub = json.load(open(os.path.join(GOLD, "published_regions.json")))["test-1kx240p.png"]
    ctx.upload_scene(srt.scenes.scene_masterchief())
    ctx.set_camera(camera)
    _, rgba = ctx.render_image(abi.default_render_params(426, 240, 1000, 4, seed=1, spp_chunks=0), want_accum=False)
    img = rgba[..., :3].astype(np.float64)
    tol = {"sky": 0.01, "far_ground": 2.5, "metal_sphere": 2.5, "ground": 3.0, "chief": 4.0}
    for name, t in tol.items():
        y0, y1, x0, x1 = pub["regions"][name]["rows_cols"]
        mean = img[y0:y1, x0:x1].mean((0, 1))
        assert np.abs(mean - pub["regions"][name]["mean_rgb"]).max() <= t, (name, mean, pub["regions"][name]["mean_rgb"])


def test_native_gather_one_rank_and_argument_errors(dev, abi, srt, camera):
    """srt_comm.cpp through the C-ABI on the one GPU a test box has: a one-rank RCCL communicator
    (ncclCommInitRank with nranks = 1), srtGatherTiles degenerating to a device copy, the collective
    blocking render equal to srtRenderImage, and the error paths (the N > 1 exchange itself needs N GPUs:
    its tile permutation is covered by tests/test_distributed_cpu.py, its bytes by the driver's multi-GPU run)."""
    import torch
    c = dev.Context(0)
    try:
        c.upload_scene(srt.scenes.scene_spheres())
        c.set_camera(camera)
        p = abi.default_render_params(200, 120, 8, 8, seed=4)
        want, want_rgba = c.render_image(p)
        with pytest.raises(dev.SrtError):
            c.comm_init(dev.comm_unique_id(), 2, 2)          # rank out of range
        c.comm_init(dev.comm_unique_id(), 1, 0)
        with pytest.raises(dev.SrtError):
            c.comm_init(dev.comm_unique_id(), 1, 0)          # already has a communicator
        nloc = dev.num_local_tiles(200, 120, 1)
        local = torch.zeros((nloc, 64, 4), dtype=torch.float32, device="cuda")
        gathered = torch.zeros_like(local)
        stream = torch.cuda.current_stream().cuda_stream
        c.render_tiles(p, local.data_ptr(), stream)
        c.gather_tiles(p, local.data_ptr(), gathered.data_ptr(), stream)
        torch.cuda.synchronize()
        assert torch.equal(local, gathered)
        bad = abi.default_render_params(200, 120, 8, 8, seed=4, tile_first=1, tile_stride=2)
        with pytest.raises(dev.SrtError):
            c.gather_tiles(bad, local.data_ptr(), gathered.data_ptr(), stream)   # not this communicator's split
        got, got_rgba = c.render_image_ranks(p)
        assert got.tobytes() == want.tobytes() and got_rgba.tobytes() == want_rgba.tobytes()
        c.comm_destroy()
        c.comm_init(dev.comm_unique_id(), 1, 0)              # can be set up again after destroy
    finally:
        c.close()


def test_lds_resident_tree_is_used_and_changes_nothing(ctx, dev, abi, srt, camera):
    """Scenes whose node array fits a CU's LDS render through the path-pool kernel (srt_wavefront.hip) or, with
    wavefront = 0, through the step-scheduler kernel over the same LDS-resident threaded tree (one workgroup of 1024
    threads per CU each); larger ones and lds_tree = 0 through the 256-thread kernel.  Same records, same arithmetic,
    same samples per work item: identical accumulators, bit for bit -- single running sums and exact chunk sums."""
    import torch
    W, H = 320, 180
    saved = {k: ctx.get_tunable(k) for k in ("lds_tree", "wavefront")}
    assert saved["lds_tree"] >= 1 and saved["wavefront"] >= 1  # the defaults: node-count thresholds
    for name, spp, mb in (("masterchief", 8, 4), ("spheres", 8, 8), ("iron", 4, 4)):
        ctx.upload_scene(srt.scenes.SCENES[name]())
        ctx.set_camera(camera)
        for chunks in (0, 1):
            images = {}
            for path, tree, wf in (("wavefront", 1, 1), ("lds_tree", 1, 0), ("l1_nodes", 0, 0)):
                ctx.set_tunable("lds_tree", tree)
                ctx.set_tunable("wavefront", wf)
                try:
                    local = torch.zeros((dev.num_local_tiles(W, H, 1), 64, 4), dtype=torch.float32, device="cuda")
                    p = abi.default_render_params(W, H, spp, mb, seed=3, spp_chunks=chunks)
                    ctx.render_tiles(p, local.data_ptr(), None)
                    torch.cuda.synchronize()
                    ctx.last_kernel_ms()  # raises if a path-pool workgroup gave up
                    info = ctx.launch_info()
                    assert info["lds_tree"] == bool(tree) and info["wavefront"] == bool(wf), (name, path, info)
                    # the headline mesh's tree leaves no room for the attenuation stacks (mode 1), the small trees do (mode 2)
                    assert info["lds_tree_mode"] == (3 if wf else 0 if not tree else 1 if name == "masterchief" else 2), (name, info)
                    assert info["threads"] == (1024 if tree else 256)
                    assert info["lds_bytes"] <= 160 * 1024
                    images[path] = local.cpu().numpy()
                finally:
                    for k, v in saved.items():
                        ctx.set_tunable(k, v)
            for path in ("wavefront", "lds_tree"):
                assert np.array_equal(images[path].view(np.uint32), images["l1_nodes"].view(np.uint32)), (name, chunks, path)
    # a tree that does not fit: 40 000 triangles -> ~40 000 nodes, 1.3 MB.  The path-pool kernel's hybrid form keeps its top
    # in LDS and reads the rest from global memory (32-bit references); with wf_hybrid = 0 (read at upload) the 256-thread
    # kernel renders it.  Same bits.
    big = {}
    for hybrid in (1, 0):
        ctx.set_tunable("wf_hybrid", hybrid)
        try:
            ctx.upload_scene(srt.scenes.scene_soup(40000, seed=5, extent=6.0, size=0.1))
        finally:
            ctx.set_tunable("wf_hybrid", 1)
        ctx.set_camera(camera)
        local = torch.zeros((dev.num_local_tiles(W, H, 1), 64, 4), dtype=torch.float32, device="cuda")
        ctx.render_tiles(abi.default_render_params(W, H, 2, 4, seed=3), local.data_ptr(), None)
        torch.cuda.synchronize()
        ctx.last_kernel_ms()
        info = ctx.launch_info()
        assert info["lds_tree_mode"] == (4 if hybrid else 0) and info["threads"] == (1024 if hybrid else 256), info
        big[hybrid] = local.cpu().numpy()
    assert np.array_equal(big[1].view(np.uint32), big[0].view(np.uint32))
