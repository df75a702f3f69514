"""Whole frames of the render kernels against the CPU oracle with NO tolerance, on the scenes of tests/exact_scenes.py whose
shading makes no single-precision libm call.  Every comparison goes through assert_frame_identical: NaNs by position,
every other accumulator word equal in bits (the count channel included), RGBA8 byte for byte where the pixel is defined,
all eight counters exactly equal.  No comparison of a rendered value in this file has a tolerance or accepts a fraction
of pixels.

What this adds to tests/test_gpu_parity.py, whose frames carry a residual (device libm against glibc) that also hides one
wrong sample in a few thousand:
  (a) frames x the four kernel forms, deep bounces (the path pool keeps attenuation levels >= 4 in wfAttHi) included;
  (b) chunk plans 1, 3, default and 7, the atomic path of the exact chunk sum, and a 3-way tile split;
  (c) the cameras of tests/ref_cases.py, which no GPU test rendered with;
  (d) every ring capacity of the path-pool kernel (1024, 1536, 2048, 3072, 4096; the 3 * 2^j ones take a multiply-shift
      modulo in ringPos), whole-tree and hybrid form, on a frame large enough that the rings' counters pass their
      capacity several times.  Ring counters wrapping at 2^32 needs some 10^9 enqueues per workgroup and is out of scope;
  (e) the scheduling tunables wf_far_rounds 1-4 (1 is what trees beyond 2^20 nodes get), wf_swap_min, wf_swap_big.
Tunables only reschedule work: the image must not move by a bit.

On a mismatch explain_pixel names the first differing sample of the first differing pixel, the first bounce whose ray,
hit or shading differs, and the material of the hit before it; it runs only on failure.

tests/golden/exact_residual.json lists the pixels left out: at most 2, each a tier-B pbr or dielectric hit where
ctx.scatter_test and OracleScene.scatter on IDENTICAL inputs give attenuations one float ulp apart (the two libms' double
exp2 / pow straddling a float rounding boundary).  Anything else that differs is a bug."""
import copy
import json
import os

import numpy as np
import pytest

import chunk_sum_ref
import exact_scenes
import ref_cases
from conftest import GOLD, render_counted
from test_gpu_parity import path_pool_form

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "rays", "nodeVisits", "boxPasses", "triTests", "sphereTests", "shadedTriHits", "texelFetches")
RING_CAPACITIES = (1024, 1536, 2048, 3072, 4096)
MAX_BOUNCE = 16  # SRT_MAX_BOUNCE of include/srt_hip.h: the deepest path a render accepts
RESIDUAL_PATH = os.path.join(GOLD, "exact_residual.json")
RESIDUAL_CAP = 2


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def residual():
    """The listed pixels: [{"scene", "seed", "pixel": [x, y], "sample", "depth", "cause"}], at most RESIDUAL_CAP."""
    entries = json.load(open(RESIDUAL_PATH))
    assert isinstance(entries, list) and len(entries) <= RESIDUAL_CAP, "exact_residual.json holds more than %d entries" % RESIDUAL_CAP
    for e in entries:
        assert set(e) == {"scene", "seed", "pixel", "sample", "depth", "cause"}, e
    return entries


# ---------------------------------------------------------------------------------------------------- the chunk sum
def fixed_chunk_sum(parts):
    """parts (chunks, ..., 3) float32 partial sums -> (..., 3) float32: the exact chunk sum as the kernels define it and
    tests/chunk_sum_ref.py states it in Python integers (vectorised here, held to it by tests/test_exact_scenes.py): each
    partial sum truncated to units of 2^-36 (exact for |v| >= 2^-13), the integers added, the sum rounded to float32 ONCE;
    NaN / infinite / beyond-the-limit partial sums poison the channel."""
    parts = np.asarray(parts, np.float32)
    lim = chunk_sum_ref.limit(parts.shape[0])
    v = parts.astype(np.float64)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        big = ~nan & ~(np.abs(v) < lim)
    ok = ~nan & ~big
    q = np.where(ok, np.trunc(np.where(ok, v, 0.0) * float(chunk_sum_ref.UNITS)), 0.0).astype(np.int64)  # exact: |v| * 2^36 < 2^62
    total = q.sum(axis=0)
    out = total.astype(np.float32) * np.float32(2.0 ** -36)  # int64 -> float32 rounds once, to nearest even; the scaling is exact
    pinf, ninf = (big & (v > 0)).any(axis=0), (big & ~(v > 0)).any(axis=0)
    out = np.where(pinf, np.float32(np.inf), out)
    out = np.where(ninf, np.float32(-np.inf), out)
    return np.where(nan.any(axis=0) | (pinf & ninf), np.float32(np.nan), out).astype(np.float32)


def oracle_frame(oracle, osc, abi, cam, p, chunks, threads):
    """(accum, rgba, stats) of the oracle for render parameters p rendered in `chunks` chunks with the kernel's chunk plan:
    chunk c holds samples [c * base + min(c, rem), ...) from p.sampleFirst on (base = spp // chunks, rem = spp % chunks:
    srt_render.cpp), each chunk a float running sum in sample order (main.cpp:217), the chunk sums added exactly and rounded
    once (fixed_chunk_sum).  One chunk: the reference's single running sum."""
    W, H, spp = p.imageWidth, p.imageHeight, p.spp
    if chunks == 1:
        q = copy.copy(p)
        q.sppChunks, q.countStats = 1, 1
        return osc.render(cam, q, oracle.RNG_COUNTER, threads=threads)
    base, rem = spp // chunks, spp % chunks
    parts, total = [], dict.fromkeys(COUNTERS, 0)
    for c in range(chunks):
        n = base + (1 if c < rem else 0)
        q = abi.default_render_params(W, H, n, p.maxBounce, seed=p.seed, sample_first=p.sampleFirst + c * base + min(c, rem))
        q.background[:] = p.background[:]
        part, _, st = osc.render(cam, q, oracle.RNG_COUNTER, threads=threads, want_rgba=False)
        parts.append(part[..., :3])
        for k in COUNTERS:
            total[k] += st[k]
    acc = np.concatenate([fixed_chunk_sum(np.stack(parts)), np.full((H, W, 1), spp, np.float32)], axis=-1)
    return acc, oracle.resolve(acc, spp), total


# ---------------------------------------------------------------------------------------------------- the scenes and the cache
def build_scene(srt, abi, key):
    """key: ("random", seed, tier) | ("room", tier) | ("mesh", tier)."""
    if key[0] == "random":
        return exact_scenes.random(abi, key[1], key[2])
    return exact_scenes.room(abi, key[1]) if key[0] == "room" else exact_scenes.mesh(srt, abi, key[1])


class Frames:
    """Scenes, their oracle instances and the oracle's frames, each made once per module and shared by every form and
    tunable setting compared against it; nothing hands out a frame for writing."""

    def __init__(self, srt, abi, oracle, dev):
        self.srt, self.abi, self.oracle, self.dev = srt, abi, oracle, dev
        self.scenes, self.frames = {}, {}
        self.threads = min(16, os.cpu_count() or 8)

    def scene(self, key):
        if key not in self.scenes:
            sb = build_scene(self.srt, self.abi, key)
            self.scenes[key] = (sb, self.oracle.OracleScene(sb))
        return self.scenes[key]

    def want(self, key, p, cam_key=None, cam=None):
        """The oracle's (accum, rgba, stats) of scene `key` for p in the chunk plan the library uses for p."""
        chunks = self.dev.plan_spp_chunks(p.imageWidth, p.imageHeight, p.spp, p.sppChunks)
        assert chunks >= 1
        fk = (key, p.imageWidth, p.imageHeight, p.spp, p.maxBounce, int(p.seed), p.sampleFirst, chunks, cam_key)
        if fk not in self.frames:
            cam = cam if cam is not None else self.oracle.make_camera(self.abi.default_camera_params())
            acc, rgba, st = oracle_frame(self.oracle, self.scene(key)[1], self.abi, cam, p, chunks, self.threads)
            acc.setflags(write=False)
            rgba.setflags(write=False)
            self.frames[fk] = (acc, rgba, st)
        return self.frames[fk]


@pytest.fixture(scope="module")
def frames(srt, abi, oracle, dev):
    return Frames(srt, abi, oracle, dev)


def tree_nodes(sb, abi):
    """Nodes over all trees of the world."""
    return sum(exact_scenes.bvh_nodes(w.count) for w in sb.world if w.kind == abi.SRT_WORLD_BVH)


def expected_mode(node_path, nodes):
    """launch_info()["lds_tree_mode"] of the node_path fixture's forms on a world with `nodes` tree nodes: a world without a
    tree has no LDS-resident form; the forced hybrid form splits trees of more than its 24 resident nodes."""
    if nodes == 0 or node_path == "l1_nodes":
        return (0,)
    if node_path == "lds_tree":
        return (1, 2)
    return (4,) if node_path == "hybrid" and nodes > 24 else (3,)


# ---------------------------------------------------------------------------------------------------- explain_pixel
def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def explain_pixel(ctx, osc, cam, p, x, y):
    """Where pixel (x, y) of a render with parameters p (scene uploaded, camera `cam` set) parts from the oracle:
    {"sample": the first sample index whose single-sample value differs (None: every sample agrees, so the samples are
    summed differently), "depth": the first bounce whose ray, hit or shading differs, "what": which of them,
    "material_before": the material of the hit before that bounce}.  Single samples are renders with spp = 1 at
    sample_first = s on both sides; the bounces come from srtRenderAov's record of the kernel's ray against
    OracleScene.sample_path; where all rays and hits agree, shade() is asked directly (ctx.scatter_test on the oracle's ray
    and hit, for the materials whose attenuation takes no draw), and last the sample is rendered with maxBounce cut short."""
    import oracle.oracle_py as O
    abi = O.abi
    out = {"pixel": (x, y), "sample": None, "depth": None, "what": "every single sample agrees: the samples are summed differently",
           "material_before": None}

    def one(s, bounces):
        q = abi.default_render_params(p.imageWidth, p.imageHeight, 1, bounces, seed=p.seed, sample_first=s)
        q.background[:] = p.background[:]
        return q

    for s in range(p.sampleFirst, p.sampleFirst + p.spp):
        q = one(s, p.maxBounce)
        got = ctx.render_image(q, want_rgba=False)[0][y, x, :3]
        steps, want = osc.sample_path(cam, q, x, y, s)
        if not _same(got, want):
            out.update(sample=s, got=got.tolist(), want=want.tolist())
            break
    else:
        return out
    for d in range(p.maxBounce):
        rec = ctx.render_aov(q, d)[y, x]
        there = d < len(steps)
        before = int(steps[d - 1]["material"]) if 0 < d <= len(steps) else None
        if bool(rec["valid"]) != there:
            return dict(out, depth=d, what="the kernel %s a ray here, the oracle %s" % (("traces", "does not") if rec["valid"] else ("does not trace", "does")),
                        material_before=before)
        if not there:
            break
        st = steps[d]
        if not (_same(rec["o"], st["o"]) and _same(rec["d"], st["d"]) and _same(rec["time"], st["time"])):
            return dict(out, depth=d, what="ray", material_before=before)
        if rec["prim"] != st["prim"] or (st["prim"] >= 0 and not _same(rec["t"], st["t"])):
            return dict(out, depth=d, what="hit (primitive %d t %r, oracle %d t %r)" % (rec["prim"], float(rec["t"]), st["prim"], float(st["t"])),
                        material_before=before)
    sb = osc.sb
    for d, st in enumerate(steps):  # every ray and hit agrees: the shading of a hit, where it takes no draw
        if st["prim"] < 0 or sb.materials[st["material"]].type == abi.SRT_MAT_PBR:
            continue
        ray = np.zeros(1, abi.RAY_DTYPE)
        ray["o"], ray["d"], ray["time"], ray["tMin"], ray["tMax"] = st["o"], st["d"], st["time"], p.tMin, np.inf
        shade = ctx.scatter_test(ray, osc.trace(ray), seed=int(p.seed))[0]
        for what, got, want in (("attenuation", shade[0:3], st["attenuation"]), ("emitted", shade[10:13], st["emitted"])):
            if (what == "emitted" or st["scattered"]) and not _same(got, want):
                return dict(out, depth=d, what="%s %r, oracle %r" % (what, got.tolist(), want.tolist()),
                            material_before=int(steps[d - 1]["material"]) if d else None)
    for k in range(1, p.maxBounce + 1):  # pbr hits draw before they shade: cut the path short instead
        q = one(out["sample"], k)
        if not _same(ctx.render_image(q, want_rgba=False)[0][y, x, :3], osc.sample_path(cam, q, x, y, out["sample"])[1]):
            return dict(out, depth=k - 1, what="the sample's value, from maxBounce %d on" % k,
                        material_before=int(steps[k - 2]["material"]) if k >= 2 and k - 2 < len(steps) else None)
    return dict(out, what="the sample differs, yet no ray, hit or truncated path does")


def assert_frame_identical(acc, rgba, stats, want_acc, want_rgba, want_stats, what, explain=None, skip=()):
    """acc / want_acc (H, W, 4) float32, rgba (H, W, 4) uint8, stats dicts (None: a launch that has no counters).
    skip: [(x, y)] pixels listed in exact_residual.json for this frame.  explain: (x, y) -> explain_pixel's result."""
    assert acc.shape == want_acc.shape and acc.dtype == want_acc.dtype == np.float32, what
    nan = np.isnan(want_acc)
    bad = (np.isnan(acc) != nan) | ((_bits(acc) != _bits(want_acc)) & ~nan)
    defined = ~nan[..., :3].any(axis=-1)
    if rgba is not None:
        bad[..., 3] |= (rgba != want_rgba).any(axis=-1) & defined
    bad = bad.any(axis=-1)
    for x, y in skip:
        bad[y, x] = False
    if bad.any():
        y, x = (int(v) for v in np.argwhere(bad)[0])
        where = explain(x, y) if explain is not None else None
        pytest.fail("%s: %d of %d pixels differ; first (x %d, y %d): kernel %r %r, oracle %r %r\n  %r" % (
            what, int(bad.sum()), bad.size, x, y, acc[y, x].tolist(), None if rgba is None else rgba[y, x].tolist(),
            want_acc[y, x].tolist(), want_rgba[y, x].tolist(), where))
    if stats is not None:
        assert want_stats["texelFetches"] == 0, what
        for k in COUNTERS:
            assert stats[k] == want_stats[k], (what, k, stats[k], want_stats[k])


def check(ctx, frames, key, p, got, what, cam_key=None, cams=None):
    """got = (acc, rgba, stats or None) of a render of scene `key` with p, against the cached oracle frame."""
    osc = frames.scene(key)[1]
    ocam = cams[1] if cams else frames.oracle.make_camera(frames.abi.default_camera_params())
    want = frames.want(key, p, cam_key, ocam)
    seed = key[1] if key[0] == "random" else None
    skip = [tuple(e["pixel"]) for e in residual() if e["scene"] == key[0] and e["seed"] == seed]
    q = copy.copy(p)
    assert_frame_identical(got[0], got[1], got[2], *want, what=(key, what), skip=skip,
                           explain=lambda x, y: explain_pixel(ctx, osc, ocam, q, x, y))


def counted(ctx, p, node_path):
    """render_counted with its counters: (acc, rgba, stats)."""
    p = copy.copy(p)
    p.countStats = 1
    acc, rgba = render_counted(ctx, p, node_path)
    return acc, rgba, ctx.stats()


# ---------------------------------------------------------------------------------------------------- (a) frames x forms
FRAME_CASES = ([(("random", seed, tier), (48, 27, 5, 6, 3)) for tier in exact_scenes.TIERS for seed in range(6)] +
               [(("room", tier), (96, 54, 4, bounces, 0)) for tier in exact_scenes.TIERS for bounces in (10, MAX_BOUNCE)] +
               [(("mesh", tier), (160, 90, 8, 4, 0)) for tier in exact_scenes.TIERS])


@pytest.mark.parametrize("key,shape", FRAME_CASES, ids=["-".join(str(v) for v in k) + "-b%d" % s[3] for k, s in FRAME_CASES])
def test_frames_by_form(ctx, frames, abi, camera, node_path, key, shape):
    """Every scene through the four forms of the render kernel (conftest.node_path); the form is asserted.  The closed room
    runs at 10 bounces and at the deepest the C ABI accepts, 16 (SRT_MAX_BOUNCE; test_deeper_paths_are_refused): the path
    pool keeps a context's attenuation levels 0-3 in its line and levels 4-15 in wfAttHi, and nearly every path of the room
    fills them all."""
    sb, _ = frames.scene(key)
    W, H, spp, bounces, first = shape
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(W, H, spp, bounces, seed=1000 + 7 * bounces, sample_first=first)
    got = counted(ctx, p, node_path)
    assert ctx.launch_info()["lds_tree_mode"] in expected_mode(node_path, tree_nodes(sb, abi)), (key, node_path, ctx.launch_info())
    check(ctx, frames, key, p, got, node_path)


def test_deeper_paths_are_refused(ctx, dev, frames, abi, camera):
    """Why the room's deep frame stops at 16 bounces: one more is an error of the render entry, not a frame."""
    ctx.upload_scene(frames.scene(("room", "A"))[0])
    ctx.set_camera(camera)
    with pytest.raises(dev.SrtError, match="maxBounce"):
        ctx.render_image(abi.default_render_params(16, 9, 1, MAX_BOUNCE + 1))


# ---------------------------------------------------------------------------------------------------- (b) chunk plans
def _gathered(ctx, dev, p, nranks):
    """Every rank's share of an nranks-way interleaved tile split, rendered one after the other, gathered rank-major as
    dist.gather would and resolved on the device: (acc, rgba, None)."""
    import torch
    W, H = p.imageWidth, p.imageHeight
    gathered = torch.zeros((nranks, dev.num_local_tiles(W, H, nranks), 64, 4), dtype=torch.float32, device="cuda")
    p = copy.copy(p)
    p.tileStride = nranks
    for r in range(nranks):
        p.tileFirst = r
        ctx.render_tiles(p, gathered[r].data_ptr(), None)
        torch.cuda.synchronize()
        ctx.last_kernel_ms()  # raises if a path-pool workgroup gave up
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    ctx.resolve_tiles(p, gathered.data_ptr(), rgba.data_ptr(), accum.data_ptr(), None)
    torch.cuda.synchronize()
    return accum.cpu().numpy(), rgba.cpu().numpy(), None


CHUNK_CASES = {"mesh": (("mesh", "B"), (160, 90, 8, 4)),
               # 8 samples, not the 5 of (a): a plan of 7 chunks needs at least 7, and the default plan of 8 samples is 8 chunks
               "random": (("random", 3, "A"), (48, 27, 8, 6))}


@pytest.mark.parametrize("form", ["wavefront", "lds_tree"])
@pytest.mark.parametrize("case", sorted(CHUNK_CASES))
def test_chunk_plans(ctx, dev, frames, abi, camera, case, form):
    """spp_chunks 1, 3, 0 (the default plan) and 7 on the chunk-slot path, the default plan once more on the atomic path
    (chunk_scratch_mb 0), and the default plan as the three shares of a 3-way tile split (tile_first 0, 1, 2 of stride 3)
    gathered: each against the oracle summed in the same plan (oracle_frame)."""
    key, (W, H, spp, bounces) = CHUNK_CASES[case]
    sb, _ = frames.scene(key)
    saved = {k: ctx.get_tunable(k) for k in ("lds_tree", "wavefront", "wf_resident_max", "chunk_scratch_mb")}
    try:
        ctx.set_tunable("lds_tree", 1)
        ctx.set_tunable("wavefront", 1 if form == "wavefront" else 0)
        ctx.set_tunable("wf_resident_max", 0)
        ctx.upload_scene(sb)
        ctx.set_camera(camera)
        mode = (3,) if form == "wavefront" else (1, 2)
        for chunks in (1, 3, 0, 7):
            p = abi.default_render_params(W, H, spp, bounces, seed=77, spp_chunks=chunks)
            got = counted(ctx, p, form)
            assert ctx.launch_info()["lds_tree_mode"] in mode, ctx.launch_info()
            check(ctx, frames, key, p, got, (form, "chunks", chunks))
        p = abi.default_render_params(W, H, spp, bounces, seed=77, spp_chunks=0)
        assert dev.plan_spp_chunks(W, H, spp, 0) == 8
        ctx.set_tunable("chunk_scratch_mb", 0)
        check(ctx, frames, key, p, counted(ctx, p, form), (form, "atomic path"))
        ctx.set_tunable("chunk_scratch_mb", saved["chunk_scratch_mb"])
        check(ctx, frames, key, p, _gathered(ctx, dev, p, 3), (form, "3-way tile split"))
        assert ctx.launch_info()["lds_tree_mode"] in mode, ctx.launch_info()
    finally:
        for k, v in saved.items():
            ctx.set_tunable(k, v)


# ---------------------------------------------------------------------------------------------------- (c) cameras
@pytest.mark.parametrize("form", ["wavefront", "lds_tree"])
@pytest.mark.parametrize("k", range(len(ref_cases.CAMERAS)))
def test_cameras(ctx, dev, frames, abi, oracle, k, form):
    """ref_cases.CAMERAS (aperture 0, time0 == time1, vfov 20 to 151 degrees, another eye, a tilted up vector), each built by
    dev.make_camera and by oracle.make_camera from the same parameters -- the two must be the same bytes -- on a tier-A
    random scene with one tree."""
    key = ("random", 0, "A")
    sb, _ = frames.scene(key)
    cp = ref_cases.camera_params(abi, k)
    cams = dev.make_camera(cp), oracle.make_camera(cp)
    assert bytes(cams[0]) == bytes(cams[1]), ref_cases.CAMERAS[k]
    saved = {t: ctx.get_tunable(t) for t in ("lds_tree", "wavefront", "wf_resident_max")}
    try:
        ctx.set_tunable("lds_tree", 1)
        ctx.set_tunable("wavefront", 1 if form == "wavefront" else 0)
        ctx.set_tunable("wf_resident_max", 0)
        ctx.upload_scene(sb)
        ctx.set_camera(cams[0])
        p = abi.default_render_params(33, 17, 4, 6, seed=500 + k)
        got = counted(ctx, p, form)
        assert ctx.launch_info()["lds_tree_mode"] in ((3,) if form == "wavefront" else (1, 2)), ctx.launch_info()
        check(ctx, frames, key, p, got, (form, "camera", k), cam_key=k, cams=cams)
    finally:
        for t, v in saved.items():
            ctx.set_tunable(t, v)


# ---------------------------------------------------------------------------------------------------- (d) ring capacities
def ring_capacity(info, nodes, hybrid):
    """The ring capacity of a path-pool launch from its LDS size: lds = 32 * resident + 256 + (18 | 20) * capacity
    (srt_plan.cpp planRender), resident = the whole tree, or 1 to 24 nodes in the forced hybrid form."""
    fits = [c for c in RING_CAPACITIES
            if (info["lds_bytes"] - 256 - (20 if hybrid else 18) * c) in ([32 * r for r in range(1, 25)] if hybrid else [32 * nodes])]
    assert len(fits) == 1, (info, nodes, hybrid, fits)
    return fits[0]


def _ring_scene(frames, abi):
    seed, _ = exact_scenes.random_with_tree(abi, "B")
    key = ("random", seed, "B")
    sb, _ = frames.scene(key)
    nodes = tree_nodes(sb, abi)
    assert 24 < nodes and 32 * nodes + 256 + 18 * 4096 <= 160 * 1024  # splits at 24 resident nodes; 4096 contexts fit beside it
    return key, sb, nodes


@pytest.mark.parametrize("form", ["wavefront", "hybrid"])
def test_every_ring_capacity(ctx, frames, abi, camera, form):
    """wf_pool 1024, 1536, 2048, 3072, 4096 on a frame that exercises the rings.  The pool equals the capacity only when a
    workgroup has at least that many work items (wfPoolSize = min(capacity, items / grid + 63)), and a ring is exercised
    only when its counters pass its capacity several times; so, with the launch's workgroups:
        pixels * chunks >= 4096 * workgroups           (asserted)
        the oracle's rays >= 4 * 4096 * workgroups     (asserted)
    The frame is sized from the device's CU count (one workgroup per CU): 16:9, 64 samples in 32 chunks, 6 bounces --
    256 x 144 on 256 CUs.  Ring counters wrapping at 2^32 (some 10^9 enqueues per workgroup) is out of scope."""
    key, sb, nodes = _ring_scene(frames, abi)
    cus = ctx.device_info()["cus"]
    W = 16
    while W * (W * 9 // 16) * 32 < 4096 * cus:
        W += 16
    H = W * 9 // 16
    p = abi.default_render_params(W, H, 64, 6, seed=4096, spp_chunks=32)
    saved = ctx.get_tunable("wf_pool")
    try:
        with path_pool_form(ctx, form, resident=24) as pf:
            ctx.upload_scene(sb)
            ctx.set_camera(camera)
            for cap in RING_CAPACITIES:
                ctx.set_tunable("wf_pool", cap)
                got = counted(ctx, p, form)
                info = ctx.launch_info()
                assert info["lds_tree_mode"] == pf.mode(), (cap, info)
                assert ring_capacity(info, nodes, form == "hybrid") == cap, (cap, info)
                assert W * H * 32 >= 4096 * info["workgroups"], (W, H, info)
                assert frames.want(key, p)[2]["rays"] >= 4 * 4096 * info["workgroups"], (frames.want(key, p)[2]["rays"], info)
                check(ctx, frames, key, p, got, (form, "ring capacity", cap))
    finally:
        ctx.set_tunable("wf_pool", saved)


@pytest.mark.parametrize("form", ["wavefront", "hybrid"])
def test_every_ring_capacity_pool_smaller_than_ring(ctx, frames, abi, camera, form):
    """33 x 17 at 1 spp: 561 work items over a handful of workgroups, so every pool is far smaller than any capacity."""
    key, sb, nodes = _ring_scene(frames, abi)
    p = abi.default_render_params(33, 17, 1, 6, seed=33)
    saved = ctx.get_tunable("wf_pool")
    try:
        with path_pool_form(ctx, form, resident=24) as pf:
            ctx.upload_scene(sb)
            ctx.set_camera(camera)
            for cap in RING_CAPACITIES:
                ctx.set_tunable("wf_pool", cap)
                got = counted(ctx, p, form)
                info = ctx.launch_info()
                assert info["lds_tree_mode"] == pf.mode() and ring_capacity(info, nodes, form == "hybrid") == cap, (cap, info)
                check(ctx, frames, key, p, got, (form, "small frame, ring capacity", cap))
    finally:
        ctx.set_tunable("wf_pool", saved)


# ---------------------------------------------------------------------------------------------------- (e) scheduling tunables
SCHEDULE_CASES = [(("mesh", tier), resident, 4) for tier in exact_scenes.TIERS for resident in (24, 300)] + \
                 [(("room", tier), 2, 10) for tier in exact_scenes.TIERS]


@pytest.mark.parametrize("key,resident,bounces", SCHEDULE_CASES, ids=["%s-%s-resident%d" % (k[0], k[1], r) for k, r, _ in SCHEDULE_CASES])
def test_scheduling_tunables(ctx, frames, abi, camera, key, resident, bounces):
    """The hybrid form's node visits per round (wf_far_rounds 1 to 4; production picks 1 for trees beyond 2^20 nodes, which
    no test can afford) and the swap thresholds (wf_swap_min 1, 16, 64; wf_swap_big at its minimum -- it is raised to
    wf_swap_min -- and 64): 160 x 90 at 4 spp, every setting against the one cached oracle frame."""
    sb, _ = frames.scene(key)
    names = ("wf_far_rounds", "wf_swap_min", "wf_swap_big")
    saved = {k: ctx.get_tunable(k) for k in names}
    p = abi.default_render_params(160, 90, 4, bounces, seed=160)
    try:
        with path_pool_form(ctx, "hybrid", resident=resident):
            ctx.upload_scene(sb)
            ctx.set_camera(camera)
            for name, values in (("wf_far_rounds", (1, 2, 3, 4)), ("wf_swap_min", (1, 16, 64)), ("wf_swap_big", (1, 64))):
                for v in values:
                    ctx.set_tunable(name, v)
                    got = counted(ctx, p, "hybrid")
                    assert ctx.launch_info()["lds_tree_mode"] == 4, ctx.launch_info()
                    check(ctx, frames, key, p, got, ("resident", resident, name, v))
                ctx.set_tunable(name, saved[name])
    finally:
        for k, v in saved.items():
            ctx.set_tunable(k, v)
