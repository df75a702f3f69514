"""GPU parity tests: the HIP path, called through the C-ABI (include/srt_hip.h), against the CPU
oracle and the committed golden fixtures on identical inputs and RNG keys.

Bars:
  * BVH: flattened tree bit-identical to the oracle's.
  * fixed ray set (srtTraceRays): primitive index, t, p, normal, tangent, bitangent, frontFace,
    material and the traversal counters are BIT-EXACT.  uv goes through acosf/atan2f on spheres
    (device libm vs glibc): |duv| <= 1e-6.
  * render (float accumulators, same counter-RNG keys): >= 99.9 % of pixels bit-identical,
    >= 99.99 % within 1e-3 relative, every pixel within 5 % + 0.05; RGBA8 within 3 levels on
    < 0.1 % of bytes.  The residual comes from sinf/acosf/atan2f/exp2 differing by an ulp between
    device libm and glibc (an ulp of uv can select the neighbouring texel of a nearest-neighbour
    lookup); all other arithmetic keeps the reference's operation order without FMA contraction.
  * traversal/shading counters (rays, node visits, box passes, primitive tests, texel fetches)
    equal the oracle's exactly.

The render bars above accept their residual whatever its cause: one wrong sample in a few thousand passes them.  The
EXACT tier (tests/test_gpu_exact_frames.py on the scenes of tests/exact_scenes.py) closes that: on scenes whose shading
calls no single-precision libm (metal, dielectric, solid-colour lights, the background; pbr with constant factors or
solid-colour textures, whose one libm call is a double exp2) whole frames are compared with NO tolerance -- every kernel
form, chunk plan, camera, ring capacity of the path pool and scheduling tunable.  It proves that the sample keys, the
bounce bookkeeping, the attenuation levels, the chunk sums and the work distribution are the oracle's, bit for bit.  It
cannot see what needs sinf / acosf / atan2f or a texel: checker and image textures, normal and metallic / roughness
maps stay with the residual bars of this file.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLD, render_counted

pytestmark = pytest.mark.gpu

SCENES = ("spheres", "iron", "masterchief")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_hits_equal(got, want, uv_atol=1e-6):
    assert np.array_equal(got["prim"], want["prim"])
    m = want["prim"] >= 0
    for f in ("t", "p", "normal", "tangent", "bitangent"):
        assert np.array_equal(_bits(got[f][m]), _bits(want[f][m])), f
    for f in ("frontFace", "material"):
        assert np.array_equal(got[f], want[f]), f
    assert np.nanmax(np.abs(got["uv"][m].astype(np.float64) - want["uv"][m])) <= uv_atol
    assert np.array_equal(np.isnan(got["uv"][m]), np.isnan(want["uv"][m]))


def assert_counter(got, want, name):
    """Render-wide counters equal the oracle's; a sample whose checker sign / texel / scatter test
    flips on a libm ulp (header above) may change its path, so totals may move by parts per million."""
    assert abs(got - want) <= max(2, 2e-5 * want), (name, got, want)


def assert_counters_equal(got, want):
    for f in ("nodeVisits", "boxPasses", "triTests", "sphereTests"):
        assert np.array_equal(got[f], want[f]), f


def assert_accum_close(gpu, ref, min_bitexact=0.999):
    """>= 99.9 % of pixels bit-identical; >= 99.99 % within 1e-3 relative; the rest are samples
    whose nearest-neighbour texel lookup (texture.h:136-137) or checker sign flipped because the
    device's acosf/atan2f/sinf differ from glibc's by an ulp: bounded by 5 % + 0.05 of the sum."""
    a, b = gpu[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    nan = np.isnan(b)
    err = np.where(nan, 0.0, np.abs(a - b))
    scale = np.where(nan, 1.0, np.maximum(np.abs(b), 1e-3))
    bit = (_bits(gpu[..., :3]) == _bits(ref[..., :3])).all(axis=-1)
    assert bit.mean() >= min_bitexact, bit.mean()
    assert (err <= 1e-3 * scale).all(axis=-1).mean() >= 0.9999
    assert (err <= 0.05 * scale + 0.05).all(), "max rel err %g" % (err / scale).max()
    assert np.array_equal(gpu[..., 3], ref[..., 3])


def assert_rgba_close(gpu, ref):
    d = np.abs(gpu.astype(int) - ref.astype(int))
    assert d.max() <= 3 and (d > 0).mean() < 1e-3, (d.max(), (d > 0).mean())


@pytest.fixture(scope="module")
def scenes(srt):
    return {n: srt.scenes.SCENES[n]() for n in SCENES}


@pytest.mark.parametrize("name", SCENES)
def test_bvh_upload_matches_oracle(ctx, oracle, scenes, name):
    ctx.upload_scene(scenes[name])
    onodes, depth = oracle.OracleScene(scenes[name]).bvh(0)
    assert ctx.bvh(0).tobytes() == onodes.tobytes()
    assert ctx.bvh_depth() == depth


@pytest.mark.parametrize("name", SCENES)
def test_trace_fixed_ray_set_bit_exact(ctx, abi, scenes, name):
    """Golden fixed ray set (grid primaries + seeded secondaries): reference traversal order."""
    g = np.load(os.path.join(GOLD, "trace_%s.npz" % name))
    ctx.upload_scene(scenes[name])
    got = ctx.trace(g["rays"])
    assert_hits_equal(got, g["hits"])
    assert_counters_equal(got, g["hits"])
    closest = ctx.trace(g["rays"], abi.SRT_TRAVERSE_CLOSEST)
    assert np.array_equal(closest["prim"], g["closest_prim"])
    m = g["closest_prim"] >= 0
    assert np.array_equal(_bits(closest["t"][m]), _bits(g["closest_t"][m]))


def test_trace_240p_primaries_vs_live_oracle(ctx, oracle, abi, scenes, camera):
    """102 240 lens-centre primaries + their secondaries on the main.cpp scene; also the F4 census."""
    sb = scenes["masterchief"]
    ctx.upload_scene(sb)
    osc = oracle.OracleScene(sb)
    W, H = 426, 240
    rng = np.random.default_rng(3)
    ys, xs = np.mgrid[0:H, 0:W]
    u = ((xs + rng.random((H, W))) / (W - 1)).astype(np.float32).ravel()
    v = (((H - ys) + rng.random((H, W))) / (H - 1)).astype(np.float32).ravel()
    o = np.array(camera.origin[:], np.float32)
    ll, hz, vt = (np.array(a[:], np.float32) for a in (camera.lleft, camera.horizontal, camera.vertical))
    rays = np.zeros(W * H, abi.RAY_DTYPE)
    rays["o"] = o
    rays["d"] = (ll[None] + u[:, None] * hz[None] + v[:, None] * vt[None] - o[None]).astype(np.float32)
    rays["time"] = rng.random(W * H).astype(np.float32)
    rays["tMin"], rays["tMax"] = 0.001, np.inf
    want = osc.trace(rays)
    got = ctx.trace(rays)
    assert_hits_equal(got, want)
    assert_counters_equal(got, want)
    m = want["prim"] >= 0
    sec = np.zeros(int(m.sum()), abi.RAY_DTYPE)
    sec["o"] = want["p"][m]
    sec["d"] = rng.normal(size=(len(sec), 3)).astype(np.float32)
    sec["time"] = rays["time"][m]
    sec["tMin"], sec["tMax"] = 0.001, np.inf
    want2, got2 = osc.trace(sec), ctx.trace(sec)
    assert_hits_equal(got2, want2)
    assert_counters_equal(got2, want2)
    # F4: faithful vs closest differ on a handful of rays, always farther, never hit/miss
    closest = ctx.trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    assert np.array_equal(closest["prim"] >= 0, got["prim"] >= 0)
    diff = (closest["prim"] != got["prim"]) | (m & (closest["t"] != got["t"]))
    assert diff.sum() < 0.002 * len(rays)
    assert (got["t"][diff] >= closest["t"][diff]).all()


def test_trace_ray_edge_cases(ctx, oracle, abi, scenes):
    """axis-parallel directions (division by zero in the slab test), zero direction, tMax cut-offs."""
    sb = scenes["masterchief"]
    ctx.upload_scene(sb)
    osc = oracle.OracleScene(sb)
    dirs = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, -1, 1e-30), (0, 0, 0),
            (1, 1, 0), (0, -0.0, -1)]
    rays = np.zeros(len(dirs) * 4, abi.RAY_DTYPE)
    k = 0
    for o, tmax in (((0.0, 3.0, 5.0), np.inf), ((0.0, 2.5, 5.0), 4.0), ((0.1, 50.0, 0.2), np.inf), ((0.0, 1.0, 0.0), 0.5)):
        for d in dirs:
            rays[k]["o"], rays[k]["d"], rays[k]["tMin"], rays[k]["tMax"] = o, d, 0.001, tmax
            k += 1
    want, got = osc.trace(rays), ctx.trace(rays)
    assert np.array_equal(got["prim"], want["prim"])
    m = want["prim"] >= 0
    assert np.array_equal(_bits(got["t"][m]), _bits(want["t"][m]))
    assert_counters_equal(got, want)


@pytest.mark.parametrize("name", SCENES)
def test_render_matches_golden_fixture(ctx, abi, scenes, camera, name, node_path):
    g = np.load(os.path.join(GOLD, "render_%s.npz" % name))
    ctx.upload_scene(scenes[name])
    ctx.set_camera(camera)
    p = abi.default_render_params(int(g["width"]), int(g["height"]), int(g["spp"]), int(g["max_bounce"]),
                                  seed=int(g["seed"]), count_stats=1)
    acc, rgba = render_counted(ctx, p, node_path)
    assert_accum_close(acc, g["accum_counter"])
    assert_rgba_close(rgba, g["rgba_counter"])
    st, want = ctx.stats(), json.loads(str(g["stats_counter"]))
    for k in ("samples", "rays", "nodeVisits", "boxPasses", "triTests", "sphereTests", "shadedTriHits", "texelFetches"):
        assert st[k] == want[k], k


def test_render_config1_vs_oracle(ctx, oracle, abi, scenes, camera, node_path):
    """BASELINE config 1 exactly: 3 spheres + ground, 426x240 (240p), 64 spp, 8 bounces."""
    sb = scenes["spheres"]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(426, 240, 64, 8, seed=2024, count_stats=1)
    acc, rgba = render_counted(ctx, p, node_path)
    st = ctx.stats()
    want_acc, want_rgba, want_st = oracle.OracleScene(sb).render(camera, p, oracle.RNG_COUNTER, threads=min(16, os.cpu_count() or 8))
    assert_accum_close(acc, want_acc)
    assert_rgba_close(rgba, want_rgba)
    for k in ("samples", "rays", "nodeVisits", "boxPasses", "triTests", "sphereTests", "shadedTriHits", "texelFetches"):
        assert_counter(st[k], want_st[k], k)
    # non-counting variant produces the same image
    p.countStats = 0
    acc2, _ = ctx.render_image(p)
    assert acc2.tobytes() == acc.tobytes()


@pytest.mark.parametrize("name,spp,mb", [("iron", 16, 4), ("masterchief", 16, 4)])
def test_render_240p_vs_oracle(ctx, oracle, abi, scenes, camera, name, spp, mb, node_path):
    sb = scenes[name]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(426, 240, spp, mb, seed=99, count_stats=1)
    acc, rgba = render_counted(ctx, p, node_path)
    st = ctx.stats()
    want_acc, want_rgba, want_st = oracle.OracleScene(sb).render(camera, p, oracle.RNG_COUNTER, threads=min(16, os.cpu_count() or 8))
    assert_accum_close(acc, want_acc)
    assert_rgba_close(rgba, want_rgba)
    for k in ("samples", "rays", "nodeVisits", "boxPasses", "triTests", "sphereTests", "shadedTriHits", "texelFetches"):
        assert_counter(st[k], want_st[k], k)


def test_render_720p_headline_frame_vs_oracle(ctx, oracle, abi, scenes, camera, node_path):
    """The headline frame at its BASELINE size (1280x720, 4 bounces) through the PRODUCTION (non-counting) render
    kernel, 8 of its samples per pixel, against the oracle with identical counter-RNG keys: the chunked default
    (exact chunk sums) and the reference's single running sum."""
    sb = scenes["masterchief"]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    osc = oracle.OracleScene(sb)
    for chunks in (1, 0):
        p = abi.default_render_params(1280, 720, 8, 4, seed=7, spp_chunks=chunks)
        acc, rgba = ctx.render_image(p)
        if chunks == 1:
            want_acc, want_rgba, _ = osc.render(camera, p, oracle.RNG_COUNTER, threads=min(16, os.cpu_count() or 8), want_stats=False)
        # one running sum: bit-identical; exact chunk sums: the same samples added in another association (<= 2e-5 relative)
        assert_accum_close(acc, want_acc, min_bitexact=0.999 if chunks == 1 else 0.0)
        assert_rgba_close(rgba, want_rgba)
    info = ctx.launch_info()
    assert info["lds_tree_mode"] == {"wavefront": 3, "hybrid": 4, "lds_tree": 1, "l1_nodes": 0}[node_path], info


FULL_SIZE_CONFIGS = {  # BASELINE.json configs[1..4] at their own size; two adjacent pixel rows each
    "C2_spheres_720p_1024spp": ("spheres", 1280, 720, 1024, 8, 420),
    "C3_iron_720p_5000spp": ("iron", 1280, 720, 5000, 4, 470),
    "C4_masterchief_720p_5000spp": ("masterchief", 1280, 720, 5000, 4, 400),
    "C5_masterchief_1080p_8192spp": ("masterchief", 1920, 1080, 8192, 4, 640),
}


def _oracle_rows_in_chunks(oracle, osc, abi, camera, W, H, spp, mb, seed, chunks, y0, y1, threads):
    """The oracle's render of rows [y0, y1) with the kernel's chunk plan: chunk c holds samples
    [c * base + min(c, rem), ...) (base = spp // chunks, rem = spp % chunks: srt_render.cpp), each chunk a float running sum
    in sample order (main.cpp:217), the chunk sums added exactly (float64 holds the sum of a few hundred float32 chunk
    sums of this size without rounding) and rounded to float32 once -- what the exact chunk sums of the kernel compute."""
    base, rem = spp // chunks, spp % chunks
    total = np.zeros((y1 - y0, W, 3), np.float64)
    count = np.zeros((y1 - y0, W), np.float64)
    for c in range(chunks):
        s0 = c * base + min(c, rem)
        n = base + (1 if c < rem else 0)
        p = abi.default_render_params(W, H, n, mb, seed=seed, sample_first=s0)
        part, _, _ = osc.render(camera, p, oracle.RNG_COUNTER, threads=threads, rows=(y0, y1), want_rgba=False, want_stats=False)
        total += part[y0:y1, :, :3].astype(np.float64)
        count += part[y0:y1, :, 3]
    with np.errstate(over="ignore", invalid="ignore"):
        return total.astype(np.float32), count


@pytest.mark.parametrize("config", sorted(FULL_SIZE_CONFIGS))
def test_full_sample_count_rows_vs_oracle(ctx, dev, oracle, abi, scenes, camera, config):
    """Every BASELINE frame at ITS OWN size and sample count through the production kernel with the library's default
    chunk plan (the launch bench.py times), two pixel rows of it against the oracle rendered at the same sample count
    with the same counter-RNG keys and the same chunk plan (main.cpp:200-227 at the sizes of main.cpp:175-180): the
    pixel sums must be the same BITS, except where one of a pixel's thousands of samples took another texel or checker
    square (device libm vs glibc, one ulp: the residual every render test carries).  C5 also runs the atomic form of the
    exact chunk sum (its 21 GB of chunk slots exceed the scratch budget) and must be bit-identical for the 8-way tile
    split.  (Against the reference's SINGLE running float sum the same rows differ by up to 1e-4 relative at 5000 spp:
    that is the running sum's own rounding drift -- adding 0.53 five thousand times -- not the kernel's.)"""
    import torch
    name, W, H, spp, mb, y = FULL_SIZE_CONFIGS[config]
    sb = scenes[name]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(W, H, spp, mb, seed=11, spp_chunks=0)
    acc, rgba = ctx.render_image(p)
    info = ctx.launch_info()
    assert info["lds_tree"] and info["wavefront"] == (name == "masterchief"), info  # the default kernels for these scenes (trees of >= 256 nodes: path pool)
    chunks = dev.plan_spp_chunks(W, H, spp, 0)
    assert chunks == dev.default_spp_chunks(spp)
    osc = oracle.OracleScene(sb)
    want, count = _oracle_rows_in_chunks(oracle, osc, abi, camera, W, H, spp, mb, 11, chunks, y, y + 2, min(16, os.cpu_count() or 8))
    got = acc[y:y + 2, :, :3]
    assert np.array_equal(np.isnan(got), np.isnan(want)), config
    bit = (_bits(got) == _bits(want)).all(axis=-1)
    assert bit.mean() >= 0.98, (config, bit.mean())
    nan = np.isnan(want)
    err = np.where(nan, 0.0, np.abs(got.astype(np.float64) - want.astype(np.float64)))
    scale = np.where(nan, 1.0, np.maximum(np.abs(want.astype(np.float64)), 1e-3))
    assert (err <= 2e-3 * scale).all(), (config, (err / scale).max())
    assert np.array_equal(acc[y:y + 2, :, 3], count)  # every sample counted
    want_rgba = oracle.resolve(np.concatenate([want, count[..., None].astype(np.float32)], axis=-1), spp)
    d = np.abs(rgba[y:y + 2].astype(int) - want_rgba.astype(int))
    assert d.max() <= 1, (config, d.max())
    if config.startswith("C5"):
        # the 8-way interleaved tile split (one rank's share after the other on this GPU) against the 1-way frame
        one = torch.zeros((dev.num_local_tiles(W, H, 1), 64, 4), dtype=torch.float32, device="cuda")
        ctx.render_tiles(p, one.data_ptr(), None)
        torch.cuda.synchronize()
        parts = []
        for r in range(8):
            local = torch.zeros((dev.num_local_tiles(W, H, 8), 64, 4), dtype=torch.float32, device="cuda")
            pr = abi.default_render_params(W, H, spp, mb, seed=11, spp_chunks=0, tile_first=r, tile_stride=8)
            ctx.render_tiles(pr, local.data_ptr(), None)
            parts.append(local)
        torch.cuda.synchronize()
        ctx.last_kernel_ms()
        split = torch.stack(parts, 1).reshape(-1, 64, 4)[: one.shape[0]]  # local tile l of rank r is tile position l * 8 + r
        assert torch.equal(split.view(torch.int32), one.view(torch.int32))


def test_sphere_field_vs_oracle(ctx, oracle, abi, srt, camera, node_path):
    """the 22x22 sphere field main.cpp:92-122 keeps commented out -- 480-odd small spheres,
    most of them moving (sphere.h:47-52), fuzzy metals and glass, in one bvhNode: same tree as the oracle,
    render and counters against the oracle with identical counter-RNG keys."""
    sb = srt.scenes.scene_sphere_field()
    assert 400 < len(sb.spheres) < 490
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    osc = oracle.OracleScene(sb)
    onodes, depth = osc.bvh(0)
    assert np.array_equal(ctx.bvh(0), onodes) and ctx.bvh_depth() == depth
    p = abi.default_render_params(426, 240, 8, 8, seed=31, count_stats=1)
    acc, rgba = render_counted(ctx, p, node_path)
    st = ctx.stats()
    want_acc, want_rgba, want_st = osc.render(camera, p, oracle.RNG_COUNTER, threads=min(16, os.cpu_count() or 8))
    assert_accum_close(acc, want_acc)
    assert_rgba_close(rgba, want_rgba)
    for k in ("samples", "rays", "nodeVisits", "boxPasses", "triTests", "sphereTests", "shadedTriHits", "texelFetches"):
        assert_counter(st[k], want_st[k], k)
    assert st["sphereTests"] > 5 * st["samples"]


def test_render_closest_mode_vs_statistics(ctx, abi, scenes, camera):
    """CLOSEST traversal only differs on the F4 rays: images agree except on a few pixels."""
    ctx.upload_scene(scenes["masterchief"])
    ctx.set_camera(camera)
    p = abi.default_render_params(426, 240, 4, 4, seed=5)
    a, _ = ctx.render_image(p)
    p.traversal = abi.SRT_TRAVERSE_CLOSEST
    b, _ = ctx.render_image(p)
    same = (_bits(a) == _bits(b)).all(axis=-1)
    assert 0.98 < same.mean() < 1.0


def test_scatter_known_answers(ctx, oracle, abi, scenes):
    """material::scatter / emitted per material through the kernel's own shading function."""
    for name in SCENES:
        sb = scenes[name]
        ctx.upload_scene(sb)
        osc = oracle.OracleScene(sb)
        g = np.load(os.path.join(GOLD, "trace_%s.npz" % name))
        m = g["hits"]["prim"] >= 0
        rays, hits = g["rays"][m][:600], g["hits"][m][:600]
        got = ctx.scatter_test(rays, hits, seed=123)
        want = np.stack([osc.scatter(rays[i:i + 1], hits[i:i + 1], 123, i, 0) for i in range(len(rays))])
        assert np.array_equal(got[:, 9], want[:, 9])               # scatter's bool
        assert np.array_equal(_bits(got[:, 6:9]), _bits(want[:, 6:9]))  # scattered origin = rec.p
        np.testing.assert_allclose(got[:, 3:6], want[:, 3:6], rtol=0, atol=0)  # direction: no libm involved
        np.testing.assert_allclose(got[:, 0:3], want[:, 0:3], rtol=2e-6, atol=1e-9)  # attenuation (exp2, sinf)
        np.testing.assert_allclose(got[:, 10:13], want[:, 10:13], rtol=0, atol=0)  # emitted
        frac = (_bits(got[:, 0:3]) == _bits(want[:, 0:3])).mean()
        assert frac > 0.97, frac


@pytest.mark.parametrize("name,bounces", [("masterchief", 4), ("spheres", 8), ("iron", 4)])
def test_render_kernel_traversal_per_ray_vs_oracle(ctx, oracle, abi, scenes, camera, name, bounces, node_path):
    """srtTraceRays runs its own kernel; this pins the RENDER kernel's node / primitive steps ray by ray
    (VERDICT r1 item 4): srtRenderAov records, per pixel, the ray the render kernel traced at bounce `depth` of the first
    sample and the hit, t and counters its traversal produced -- the counting instance of whichever kernel the same launch
    without counting runs: the step scheduler's walk (one-FMA slab certificate, stack or thread links, node bursts) for
    lds_tree / l1_nodes, the path-pool kernel's for wavefront / hybrid (lanes as traversal engines, hybrid form: resident /
    far records, 32-bit links).  The oracle's world.hit() (bvh.h:97-105 recursion, IEEE divisions) on the same rays must
    agree bit for bit, counters included."""
    sb = scenes[name]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    osc = oracle.OracleScene(sb)
    W, H = 426, 240
    p = abi.default_render_params(W, H, 1, bounces, seed=5)
    seen = 0
    for depth in range(3):
        aov = ctx.render_aov(p, depth).reshape(-1)
        mode = ctx.launch_info()["lds_tree_mode"]
        if node_path == "wavefront":
            assert mode == 3, (name, mode)
        elif node_path == "hybrid":  # (wf_resident_max = 24: a tree of no more than 24 nodes is not split)
            assert mode == (4 if len(ctx.bvh(0)) > 24 else 3), (name, mode)
        else:
            assert mode in ((1, 2) if node_path == "lds_tree" else (0,)), (name, mode)
        seen += assert_aov_matches_oracle(aov, osc, abi, (name, depth), min_rays=W * H if depth == 0 else 1001)
    assert seen > 1.5 * W * H


def assert_aov_matches_oracle(aov, osc, abi, what, min_rays=1):
    """srtRenderAov's records (valid ones) against the oracle's world.hit() on the same rays: primitive, the bits of t and
    the four traversal counters exactly.  Returns the number of records."""
    rec = aov.reshape(-1)
    rec = rec[rec["valid"] == 1]
    assert len(rec) >= min_rays, (what, len(rec))
    rays = np.zeros(len(rec), abi.RAY_DTYPE)
    rays["o"], rays["d"], rays["time"] = rec["o"], rec["d"], rec["time"]
    rays["tMin"], rays["tMax"] = 0.001, np.inf
    want = osc.trace(rays)
    assert np.array_equal(rec["prim"], want["prim"]), what
    m = want["prim"] >= 0
    assert np.array_equal(_bits(rec["t"][m]), _bits(want["t"][m])), what
    for f in ("nodeVisits", "boxPasses", "triTests", "sphereTests"):
        bad = np.flatnonzero(rec[f] != want[f])
        assert len(bad) == 0, (what, f, len(bad), rec[f][bad[:4]], want[f][bad[:4]])
    return len(rec)


class path_pool_form:
    """Tunables for one form of the path-pool kernel for the scenes uploaded inside the block: "wavefront" (the whole tree
    in LDS) or "hybrid" (only `resident` nodes in LDS, the rest read from global memory; read at upload), or "natural"
    (the library's defaults: a tree beyond LDS gets the hybrid form by itself).  Restores the tunables afterwards."""

    def __init__(self, ctx, form, resident=24):
        self.ctx, self.form, self.resident = ctx, form, resident

    def __enter__(self):
        self.saved = {k: self.ctx.get_tunable(k) for k in ("lds_tree", "wavefront", "wf_resident_max", "wf_hybrid")}
        if self.form != "natural":
            self.ctx.set_tunable("lds_tree", 1)
            self.ctx.set_tunable("wavefront", 1)  # every tree that fits, however small
            self.ctx.set_tunable("wf_hybrid", 1)
            self.ctx.set_tunable("wf_resident_max", self.resident if self.form == "hybrid" else 0)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.ctx.set_tunable(k, v)

    def mode(self):
        return {"wavefront": 3, "hybrid": 4, "natural": 4}[self.form]


def aov_per_ray_vs_oracle_and_step_scheduler(ctx, osc, abi, p, depths, mode, what, min_rays=1):
    """For each bounce depth: the path-pool kernel's AOV launch runs `mode` (3 whole tree in LDS, 4 hybrid form), its
    records match the oracle's world.hit() per ray, and they are byte-identical to the step-scheduler kernel's records
    (tunable wavefront = 0) -- the same rays at the same bounces, so the path pool's depth bookkeeping is pinned too.
    Returns the number of records per depth."""
    counts = []
    wf = ctx.get_tunable("wavefront")
    for depth in depths:
        aov = ctx.render_aov(p, depth)
        assert ctx.launch_info()["lds_tree_mode"] == mode, (what, depth, ctx.launch_info())
        counts.append(assert_aov_matches_oracle(aov, osc, abi, (what, depth), min_rays))
        ctx.set_tunable("wavefront", 0)
        try:
            step = ctx.render_aov(p, depth)
            assert not ctx.launch_info()["wavefront"], ctx.launch_info()
        finally:
            ctx.set_tunable("wavefront", wf)
        assert aov.tobytes() == step.tobytes(), (what, depth, int((aov != step).sum()))
    return counts


def test_path_pool_per_ray_on_a_tree_beyond_lds(ctx, oracle, abi, srt, camera):
    """The 20k-triangle soup: some 24 k nodes (750 KB), far beyond LDS, and primitive references beyond 16 bits -- the
    hybrid form the library picks by itself (the LDS keeps the top of the tree, the walk reads the rest from global memory, 32-bit thread
    links, primSecond for leaves whose two objects are not neighbours).  Per ray at bounces 0, 1, 2 against the oracle and
    the step scheduler, then a small frame's counters EXACTLY equal to the oracle's."""
    sb = srt.scenes.scene_soup(20000, seed=3)
    with path_pool_form(ctx, "natural"):
        ctx.upload_scene(sb)
        ctx.set_camera(camera)
        assert len(ctx.bvh(0)) * 32 > 160 * 1024 and 2 * 20000 > 0x7fff  # beyond LDS; 32-bit links (~(index << 1 | sphere))
        osc = oracle.OracleScene(sb)
        W, H = 320, 180
        p = abi.default_render_params(W, H, 1, 4, seed=13)
        n = aov_per_ray_vs_oracle_and_step_scheduler(ctx, osc, abi, p, (0, 1, 2), 4, "soup20k", min_rays=1000)
        assert n[0] == W * H
        p = abi.default_render_params(96, 54, 2, 4, seed=14, count_stats=1)
        acc, _ = ctx.render_image(p)
        assert ctx.launch_info()["lds_tree_mode"] == 4
        st = ctx.stats()
        want_acc, _, want_st = osc.render(camera, p, oracle.RNG_COUNTER, threads=min(16, os.cpu_count() or 8))
        for k in ("samples", "rays", "nodeVisits", "boxPasses", "triTests", "sphereTests", "shadedTriHits", "texelFetches"):
            assert st[k] == want_st[k], (k, st[k], want_st[k])
        assert (_bits(acc) == _bits(want_acc)).all(axis=-1).mean() >= 0.995


def _multi_root_worlds(abi):
    """Worlds of more than one root (hittableList over several items, main.cpp:153): "two_bvh" of
    test_world_and_material_variants_vs_oracle (a single-object leaf and a two-sphere node as two trees), and a list of
    plain spheres around a tree (primitive roots before and after it)."""
    def spheres(sb, n):
        mats = (sb.metal((0.8, 0.7, 0.6), 0.2), sb.dielectric(1.5), sb.pbr(albedo_tex=sb.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))))
        rng = np.random.default_rng(n)
        for i in range(n):
            sb.add_sphere(tuple(rng.uniform(-3, 3, 3) + np.array([0.0, 2.0, -1.0])), float(rng.uniform(0.3, 0.9)), mats[i % 3])
        sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, mats[2])
    out = {}
    sb = abi.SceneBuilder()
    m1, m2 = sb.metal((0.8, 0.7, 0.6), 0.2), sb.dielectric(1.5)
    sb.add_sphere((0.0, 2.0, 0.0), 1.0, m1)
    sb.add_sphere((-2.2, 2.0, 0.0), 1.0, m2)
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.pbr(albedo_tex=sb.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))))
    sb.world_bvh(0, 1)
    sb.world_bvh(1, 2)
    out["two_bvh"] = sb
    sb = abi.SceneBuilder()
    spheres(sb, 9)
    sb.world_prim(0)
    sb.world_bvh(1, 8)
    sb.world_prim(9)  # the ground
    out["list_around_bvh"] = sb
    return out


@pytest.mark.parametrize("form", ["wavefront", "hybrid"])
@pytest.mark.parametrize("variant", ["two_bvh", "list_around_bvh"])
def test_path_pool_per_ray_multi_root_worlds(ctx, oracle, abi, camera, variant, form):
    """Several roots: the path-pool kernel's SINGLE = false instance, which walks on to the next root of the world list
    (worldRef: DevScene::world in the whole-tree form, worldWf in the hybrid form) when a walk is done.  The hybrid form is
    forced with one resident node, so that roots lie outside LDS.  Per ray at bounces 0, 1, 2."""
    sb = _multi_root_worlds(abi)[variant]
    with path_pool_form(ctx, form, resident=1):
        ctx.upload_scene(sb)
        ctx.set_camera(camera)
        osc = oracle.OracleScene(sb)
        p = abi.default_render_params(160, 90, 1, 6, seed=78)
        n = aov_per_ray_vs_oracle_and_step_scheduler(ctx, osc, abi, p, (0, 1, 2), path_pool_form(ctx, form).mode(), variant, min_rays=500)
        assert n[0] == 160 * 90


def _mirror_room(abi):
    """A closed room: the camera and a few spheres inside a fuzzy-metal sphere, lit by a small light.  Nearly every path
    goes on bouncing until maxBounce (only the light ends one early), so deep bounces are the rule."""
    sb = abi.SceneBuilder()
    sb.add_sphere((0.0, 0.0, 0.0), 30.0, sb.metal((0.9, 0.85, 0.8), 0.3))
    sb.add_sphere((0.0, 1.0, 0.0), 1.0, sb.pbr(albedo=(0.7, 0.5, 0.3, 1.0), roughness=0.6))
    sb.add_sphere((-2.5, 1.5, -1.0), 1.2, sb.dielectric(1.5))
    sb.add_sphere((2.5, 1.2, -0.5), 0.9, sb.metal((0.6, 0.7, 0.8), 0.05))
    sb.add_sphere((0.0, 8.0, -3.0), 4.0, sb.light((6.0, 5.0, 4.0)))
    sb.add_sphere((1.0, -0.5, 2.0), 0.4, sb.pbr(albedo_tex=sb.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))))
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


@pytest.mark.parametrize("form", ["wavefront", "hybrid"])
def test_path_pool_per_ray_deep_bounces(ctx, oracle, abi, camera, form):
    """Bounces past the four a context line holds attenuations for (wfAttHi) and the depth bookkeeping of the hit step:
    maxBounce 10, per ray at bounces 5 and 8; the frame's accumulators bit-identical to the step-scheduler kernel's and
    close to the oracle's (deep paths through pbr surfaces carry more libm-ulp differences than the other frames)."""
    sb = _mirror_room(abi)
    with path_pool_form(ctx, form, resident=2):
        ctx.upload_scene(sb)
        ctx.set_camera(camera)
        osc = oracle.OracleScene(sb)
        W, H = 160, 90
        p = abi.default_render_params(W, H, 1, 10, seed=41)
        n = aov_per_ray_vs_oracle_and_step_scheduler(ctx, osc, abi, p, (5, 8), path_pool_form(ctx, form).mode(), "mirror room",
                                                     min_rays=W * H // 4)
        assert n[0] >= n[1] > 0
        p = abi.default_render_params(W, H, 4, 10, seed=42)
        acc, _ = ctx.render_image(p)
        assert ctx.launch_info()["lds_tree_mode"] == path_pool_form(ctx, form).mode()
        ctx.set_tunable("wavefront", 0)
        step, _ = ctx.render_image(p)
        assert not ctx.launch_info()["wavefront"]
    assert _bits(acc).tobytes() == _bits(step).tobytes()
    want, _, _ = osc.render(camera, p, oracle.RNG_COUNTER, threads=min(16, os.cpu_count() or 8), want_rgba=False, want_stats=False)
    assert np.array_equal(np.isnan(acc), np.isnan(want)) and np.array_equal(acc[..., 3], want[..., 3])
    assert (_bits(acc[..., :3]) == _bits(want[..., :3])).all(axis=-1).mean() >= 0.9
    fin = np.isfinite(want[..., :3])
    rel = np.abs(acc[..., :3][fin].astype(np.float64) - want[..., :3][fin]) / np.maximum(np.abs(want[..., :3][fin]), 1e-3)
    assert rel.mean() < 1e-3, rel.mean()


@pytest.mark.parametrize("form", ["wavefront", "hybrid"])
def test_path_pool_per_ray_frame_smaller_than_a_pool(ctx, oracle, abi, scenes, camera, form):
    """A 33 x 17 frame: fewer work items than a workgroup has contexts (partial tiles, most contexts never get an item).
    Per ray at bounces 0, 1, 2 on the main.cpp scene, and its counters exactly equal to the oracle's."""
    sb = scenes["masterchief"]
    with path_pool_form(ctx, form, resident=300):
        ctx.upload_scene(sb)
        ctx.set_camera(camera)
        osc = oracle.OracleScene(sb)
        p = abi.default_render_params(33, 17, 1, 4, seed=6)
        n = aov_per_ray_vs_oracle_and_step_scheduler(ctx, osc, abi, p, (0, 1, 2), path_pool_form(ctx, form).mode(), "33x17")
        assert n[0] == 33 * 17
        p = abi.default_render_params(33, 17, 3, 4, seed=6, count_stats=1)
        acc, _ = ctx.render_image(p)
        assert ctx.launch_info()["lds_tree_mode"] == path_pool_form(ctx, form).mode()
        st = ctx.stats()
        _, _, want_st = osc.render(camera, p, oracle.RNG_COUNTER, threads=4, want_rgba=False)
        for k in ("samples", "rays", "nodeVisits", "boxPasses", "triTests", "sphereTests"):
            assert st[k] == want_st[k], (k, st[k], want_st[k])


@pytest.mark.parametrize("form", ["wavefront", "hybrid"])
@pytest.mark.parametrize("case", ["config1", "masterchief_240p", "sphere_field"])
def test_path_pool_counting_instance_does_not_perturb_the_path(ctx, abi, srt, scenes, camera, case, form):
    """A counting launch runs the counting instance of the kernel the production launch runs (same form, same launch
    mode); its counters must come from the very paths the production kernel traces: the accumulators are the same bits."""
    name, W, H, spp, mb, seed, resident = {"config1": ("spheres", 426, 240, 64, 8, 2024, 1),
                                           "masterchief_240p": ("masterchief", 426, 240, 16, 4, 99, 300),
                                           "sphere_field": ("sphere_field", 426, 240, 8, 8, 31, 100)}[case]
    sb = srt.scenes.scene_sphere_field() if name == "sphere_field" else scenes[name]
    with path_pool_form(ctx, form, resident=resident):
        ctx.upload_scene(sb)
        ctx.set_camera(camera)
        p = abi.default_render_params(W, H, spp, mb, seed=seed)
        acc, rgba = ctx.render_image(p)
        mode = ctx.launch_info()["lds_tree_mode"]
        assert mode == path_pool_form(ctx, form).mode(), (case, mode)
        p.countStats = 1
        acc_c, rgba_c = ctx.render_image(p)
        assert ctx.launch_info()["lds_tree_mode"] == mode
        st = ctx.stats()
    assert _bits(acc_c).tobytes() == _bits(acc).tobytes(), (case, form)
    assert np.array_equal(rgba_c, rgba)
    assert st["samples"] == W * H * spp and st["rays"] >= st["samples"] and st["nodeVisits"] > st["rays"], st
