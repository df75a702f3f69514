"""Device ray queries (srtTraceRaysDevice, srtOccludedDevice; include/srt_hip.h "Ray queries") against the CPU oracle.

Every comparison is ZERO tolerance on prim, t (as uint32), material, frontFace and the occlusion byte against the oracle's
brute force over prims[] (oracle.OracleScene(sb).trace(rays, SRT_TRAVERSE_CLOSEST)), unless a test says otherwise: the
CLOSEST query is defined as min t, then max prims[] index, over all primitives, which is what that loop returns.

Every query of this file goes through buffers that are 64 elements longer than n and filled with a sentinel, and the
sentinel must survive (_query)."""
import os

import numpy as np
import pytest
import torch

import refit_ref as RF
import tree_build_scenes as S
from conftest import GOLD
from test_gpu_parity import assert_hits_equal, scenes  # noqa: F401  (scenes: the module fixture of the parity scenes)

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 64
SENTINEL = 0x5A
REC = 88  # sizeof(SrtHit): 22 words
KEY = ("prim", "t", "material", "frontFace")
BUILDERS = ("REFERENCE", "LBVH", "PLOC")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device_rays(rays):
    return torch.from_numpy(np.ascontiguousarray(rays).view(F).reshape(-1, 9).copy()).cuda()


def _query(dev, abi, c, rays, traversal=None, records=False, hits=True, stream=None, d_rays=None):
    """One call of each entry on sentinel-padded buffers: (hits RAY_HIT_DTYPE or None, records HIT_DTYPE or None) for a
    traversal, the occlusion bytes for traversal None.  Synchronises `stream` (a torch stream) or the device."""
    d_rays = _device_rays(rays) if d_rays is None else d_rays
    n = d_rays.shape[0]
    handle = stream.cuda_stream if stream is not None else None
    with torch.cuda.stream(stream):
        d_hits = torch.full(((n + PAD) * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_recs = torch.full(((n + PAD) * REC,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_occ = torch.full((n + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    if traversal is None:
        rc = dev.lib.srtOccludedDevice(c.h, d_rays.data_ptr(), n, d_occ.data_ptr(), handle)
    else:
        rc = dev.lib.srtTraceRaysDevice(c.h, d_rays.data_ptr(), n, traversal, d_hits.data_ptr() if hits else None,
                                        d_recs.data_ptr() if records else None, handle)
    assert rc == 0, dev.lib.srtLastError(c.h)
    (stream or torch.cuda).synchronize()
    h, r, o = d_hits.cpu().numpy(), d_recs.cpu().numpy(), d_occ.cpu().numpy()
    written = {"hits": traversal is not None and hits, "recs": traversal is not None and records, "occ": traversal is None}
    for name, a, size in (("hits", h, 16), ("recs", r, REC), ("occ", o, 1)):
        assert (a[(n * size if written[name] else 0):] == SENTINEL).all(), "%s: written beyond element n, or unasked" % name
    if traversal is None:
        assert np.isin(o[:n], (0, 1)).all()
        return o[:n].copy()
    return (h[:n * 16].view(abi.RAY_HIT_DTYPE).copy() if hits else None,
            r[:n * REC].view(abi.HIT_DTYPE).copy() if records else None)


def _assert_key(got, want):
    """prim, t's bits, material and frontFace of a query's hits (or records) against the oracle's records."""
    assert np.array_equal(got["prim"], want["prim"])
    assert np.array_equal(_bits(got["t"]), _bits(want["t"]))
    assert np.array_equal(got["material"], want["material"])
    assert np.array_equal(got["frontFace"], want["frontFace"])


def _check(dev, abi, oracle, c, sb, rays, want=None):
    """CLOSEST and occlusion of `rays` on the uploaded scene `sb` against the brute force; returns (hits, want)."""
    want = oracle.OracleScene(sb).trace(rays, abi.SRT_TRAVERSE_CLOSEST) if want is None else want
    got = _query(dev, abi, c, rays, abi.SRT_TRAVERSE_CLOSEST)[0]
    _assert_key(got, want)
    assert np.array_equal(_query(dev, abi, c, rays), (want["prim"] >= 0).astype(np.uint8))
    return got, want


def _builder(abi, name):
    return getattr(abi, "SRT_BUILDER_" + name)


@pytest.fixture(scope="module")
def soup3000(abi, oracle):
    """The 3000 soup per builder (one geometry, three trees), its 20 000 rays and the brute force over them, computed once."""
    sbs = {b: S.soup(abi, 3000, _builder(abi, b)) for b in BUILDERS}
    rays = S.random_rays(abi, 20_000)
    want = oracle.OracleScene(sbs["REFERENCE"]).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    want.setflags(write=False)
    rays.setflags(write=False)
    return sbs, rays, want


# ------------------------------------------------------------------------------------------------ 1. three builders
def test_closest_hit_is_the_brute_force_for_every_builder(ctx, dev, abi, soup3000):
    sbs, rays, want = soup3000
    share = (want["prim"] >= 0).mean()
    assert 0.1 <= share <= 0.9, share
    out = {}
    for b in BUILDERS:
        ctx.upload_scene(sbs[b])
        got = _query(dev, abi, ctx, rays, abi.SRT_TRAVERSE_CLOSEST)[0]
        _assert_key(got, want)
        miss = want["prim"] < 0
        assert (got["t"][miss] == 0).all() and (got["material"][miss] == -1).all() and (got["frontFace"][miss] == 0).all()
        # the Python wrappers: the same bytes, as torch tensors on the rays' device
        d = _device_rays(rays)
        t = ctx.trace_device(d)
        occ = ctx.occluded_device(d)
        torch.cuda.synchronize()
        assert t.dtype == torch.int32 and tuple(t.shape) == (len(rays), 4) and t.device == d.device
        assert occ.dtype == torch.uint8 and tuple(occ.shape) == (len(rays),)
        assert t.cpu().numpy().tobytes() == got.tobytes()
        assert np.array_equal(occ.cpu().numpy(), (want["prim"] >= 0).astype(np.uint8))
        out[b] = got.tobytes()
    assert out["REFERENCE"] == out["LBVH"] == out["PLOC"]


# ------------------------------------------------------------------------------------------------ 2. tMax
def test_tmax_cuts_and_keeps(ctx, dev, abi, oracle, soup3000):
    """tMax from the oracle's own t: half of it on even rays (a miss unless something nearer exists), exactly t on odd rays
    (a hit with t == tMax is a hit), 3 on the oracle's misses."""
    sbs, rays, want = soup3000
    cut = rays.copy()
    hit = want["prim"] >= 0
    even = (np.arange(len(rays)) % 2 == 0)
    cut["tMax"] = np.where(hit, np.where(even, F(0.5) * want["t"], want["t"]), F(3.0)).astype(F)
    osc = oracle.OracleScene(sbs["PLOC"])
    want_cut = osc.trace(cut, abi.SRT_TRAVERSE_CLOSEST)
    assert (want_cut["prim"][hit & ~even] >= 0).all()  # t == tMax stays a hit in the oracle
    assert (want_cut["prim"] >= 0).sum() < hit.sum()
    for b in ("REFERENCE", "PLOC"):
        ctx.upload_scene(sbs[b])
        _check(dev, abi, oracle, ctx, sbs[b], cut, want_cut)
        assert np.array_equal(_query(dev, abi, ctx, rays), hit.astype(np.uint8))


# ------------------------------------------------------------------------------------------------ 3. ties
@pytest.mark.parametrize("builder", BUILDERS)
def test_ties_go_to_the_largest_list_index(ctx, dev, abi, oracle, builder):
    sb = S.duplicates(abi, _builder(abi, builder))
    ctx.upload_scene(sb)
    rays = S.random_rays(abi, 5000, with_time=False)
    got, want = _check(dev, abi, oracle, ctx, sb, rays)
    hit = got["prim"][got["prim"] >= 0]
    assert np.isin(hit, (299, 599)).all()
    assert (hit == 299).sum() >= 50 and (hit == 599).sum() >= 50

    sb = abi.SceneBuilder()
    m = sb.metal((0.7, 0.6, 0.5), 0.1)
    for _ in range(3):
        sb.add_sphere((0.0, 3.0, -1.0), 1.0, m)
    sb.world_bvh(0, None, 0.0, 1.0, builder=_builder(abi, builder))
    ctx.upload_scene(sb)
    got, want = _check(dev, abi, oracle, ctx, sb, rays)
    assert (got["prim"] >= 0).sum() >= 50 and (got["prim"][got["prim"] >= 0] == 2).all()

    sb = S.concentric(abi, _builder(abi, builder))
    ctx.upload_scene(sb)
    got, want = _check(dev, abi, oracle, ctx, sb, rays)
    assert (want["prim"] >= 0).sum() >= 50


# ------------------------------------------------------------------------------------------------ 4. deep stack
def test_chain_tree(ctx, dev, abi, oracle):
    sb = S.chain(abi, abi.SRT_BUILDER_PLOC)
    ctx.upload_scene(sb)
    assert ctx.bvh_depth() >= 30
    got, want = _check(dev, abi, oracle, ctx, sb, S.chain_rays(abi))
    assert 0.1 <= (want["prim"] >= 0).mean()


# ------------------------------------------------------------------------------------------------ 5. worlds
def test_worlds_of_several_items_and_of_one_primitive(ctx, dev, abi, oracle):
    rays = S.random_rays(abi, 5000, with_time=False)
    rays["time"] = 0.5  # the one instant inside all four items' ranges
    sb = S.four_items(abi)
    ctx.upload_scene(sb)
    got, want = _check(dev, abi, oracle, ctx, sb, rays)
    for lo, hi in ((0, 301), (301, 601), (601, 900), (900, 901)):  # every item answers some ray
        assert ((want["prim"] >= lo) & (want["prim"] < hi)).any(), (lo, hi)

    for bare in (True, False):
        sb = abi.SceneBuilder()
        s = sb.add_sphere((0.0, 3.0, -1.0), 1.5, sb.metal((0.7, 0.6, 0.5), 0.1))
        if bare:
            sb.world_prim(s)
        else:
            sb.world_bvh(0, None, 0.0, 1.0, builder=abi.SRT_BUILDER_LBVH)  # a tree of one node whose children are one object
        ctx.upload_scene(sb)
        got, want = _check(dev, abi, oracle, ctx, sb, rays)
        assert 50 <= (want["prim"] >= 0).sum() < len(rays)


# ------------------------------------------------------------------------------------------------ 6. degenerate directions
def test_axis_parallel_inside_and_tmin_zero(ctx, dev, abi, oracle, soup3000):
    sbs, _, _ = soup3000
    rng = np.random.default_rng(17)
    n = 6000
    rays = np.zeros(n, abi.RAY_DTYPE)
    rays["time"] = rng.random(n).astype(F)
    rays["tMin"], rays["tMax"] = 0.001, np.inf
    # [0, 2000): one zero component, [2000, 4000): two, from outside the soup towards it; [4000, 5000): from inside its
    # extent (centre (0, 3, -1), half side 3), any direction; [5000, 6000): from outside with tMin = 0
    d = rng.normal(size=(n, 3)).astype(F)
    k = np.arange(n)
    axis = rng.integers(0, 3, n)
    d[k[:2000], axis[:2000]] = 0.0
    two = k[2000:4000]
    keep = axis[2000:4000]
    sign = np.where(rng.random(2000) < 0.5, F(-1.0), F(1.0))
    d[two] = 0.0
    d[two, keep] = sign
    o = np.tile(np.array([0.0, 3.0, -1.0], F), (n, 1))
    o[:4000] += (rng.random((4000, 3)).astype(F) - F(0.5)) * F(10.0)      # a point in and around the soup's extent ...
    o[:4000] -= d[:4000] * (F(8.0) / np.maximum(np.abs(d[:4000]).max(axis=1, keepdims=True), F(1e-3)))  # ... seen from outside
    o[4000:5000] += (rng.random((1000, 3)).astype(F) - F(0.5)) * F(5.0)
    o[5000:] = (0.0, 3.0, 5.0)
    d[5000:] = d[5000:] * F(0.5) + np.array([0.0, 0.0, -1.0], F)
    rays["o"], rays["d"] = o, d
    rays["tMin"][5000:] = 0.0
    assert ((d[:2000] == 0).sum(axis=1) == 1).all() and ((d[2000:4000] == 0).sum(axis=1) == 2).all()
    want = oracle.OracleScene(sbs["PLOC"]).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    for lo, hi in ((0, 2000), (2000, 4000), (4000, 5000), (5000, 6000)):
        share = (want["prim"][lo:hi] >= 0).mean()
        assert 0.05 <= share <= 0.98, (lo, share)
    for b in ("REFERENCE", "PLOC"):
        ctx.upload_scene(sbs[b])
        _check(dev, abi, oracle, ctx, sbs[b], rays, want)


# ------------------------------------------------------------------------------------------------ 7. FAITHFUL
@pytest.mark.parametrize("name", ["spheres", "iron"])
def test_faithful_is_the_parity_entry_without_counters(ctx, dev, abi, scenes, name):  # noqa: F811
    g = np.load(os.path.join(GOLD, "trace_%s.npz" % name))
    ctx.upload_scene(scenes[name])
    want = ctx.trace(g["rays"], abi.SRT_TRAVERSE_FAITHFUL)
    assert 0.1 <= (want["prim"] >= 0).mean()
    hits, recs = _query(dev, abi, ctx, g["rays"], abi.SRT_TRAVERSE_FAITHFUL, records=True)
    for f in ("nodeVisits", "boxPasses", "triTests", "sphereTests"):
        assert (recs[f] == 0).all()
        want[f] = 0
    assert recs.tobytes() == want.tobytes()
    for f in KEY:
        assert hits[f].tobytes() == want[f].tobytes(), f
    # each output alone: the same bytes
    assert _query(dev, abi, ctx, g["rays"], abi.SRT_TRAVERSE_FAITHFUL)[0].tobytes() == hits.tobytes()
    assert _query(dev, abi, ctx, g["rays"], abi.SRT_TRAVERSE_FAITHFUL, records=True, hits=False)[1].tobytes() == recs.tobytes()


# ------------------------------------------------------------------------------------------------ 8. records in CLOSEST
def test_closest_records(ctx, dev, abi, oracle, soup3000):
    sbs, rays, _ = soup3000
    rays = rays[:5000]
    sb = sbs["LBVH"]
    ctx.upload_scene(sb)
    want = oracle.OracleScene(sb).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    hits, recs = _query(dev, abi, ctx, rays, abi.SRT_TRAVERSE_CLOSEST, records=True)
    for f in KEY:
        assert recs[f].tobytes() == hits[f].tobytes(), f
    assert_hits_equal(recs, want)
    for f in ("nodeVisits", "boxPasses", "triTests", "sphereTests"):
        assert (recs[f] == 0).all()
    t, r = ctx.trace_device(_device_rays(rays), records=True)
    torch.cuda.synchronize()
    assert tuple(r.shape) == (len(rays), 22) and r.dtype == torch.int32
    assert t.cpu().numpy().tobytes() == hits.tobytes() and r.cpu().numpy().tobytes() == recs.tobytes()


# ------------------------------------------------------------------------------------------------ 9. sizes
def _spheres37(abi):
    sb = abi.SceneBuilder()
    m = sb.metal((0.7, 0.6, 0.5), 0.1)
    rng = np.random.default_rng(5)
    for _ in range(37):
        c = (rng.random(3) - 0.5) * 6.0 + np.array([0.0, 3.0, -1.0])
        sb.add_sphere(tuple(float(x) for x in c), float(0.2 + 0.5 * rng.random()), m)
    sb.world_bvh(0, None, 0.0, 1.0, builder=abi.SRT_BUILDER_PLOC)
    return sb


def test_sizes_around_a_wave_a_block_and_the_grid(ctx, dev, abi, oracle):
    sb = _spheres37(abi)
    ctx.upload_scene(sb)
    # the grid is capped at 8 workgroups of 256 lanes per CU: one size beyond it, so that lanes take a second ray
    capacity = ctx.device_info()["cus"] * 8 * 256
    big = capacity + 12_345
    assert big <= 700_000, "the oracle's brute force over %d rays is no longer a second or two" % big
    rays = S.random_rays(abi, big, with_time=False)
    want = oracle.OracleScene(sb).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    assert 0.1 <= (want["prim"] >= 0).mean() <= 0.9
    for n in (0, 1, 63, 64, 65, 255, 256, 257, big):
        if n == 0:  # launches nothing, takes NULL buffers, and the wrappers return empty tensors
            assert dev.lib.srtTraceRaysDevice(ctx.h, None, 0, abi.SRT_TRAVERSE_CLOSEST, None, None, None) == 0
            assert dev.lib.srtOccludedDevice(ctx.h, None, 0, None, None) == 0
            empty = torch.zeros((0, 9), dtype=torch.float32, device="cuda")
            assert tuple(ctx.trace_device(empty).shape) == (0, 4) and tuple(ctx.occluded_device(empty).shape) == (0,)
        _check(dev, abi, oracle, ctx, sb, rays[:n], want[:n])


# ------------------------------------------------------------------------------------------------ 10. stream order
def test_query_runs_behind_the_op_that_made_the_rays(ctx, dev, abi, oracle, soup3000):
    sbs, rays, _ = soup3000
    rays = rays[:8192].copy()
    rays["tMax"] = 40.0
    sb = sbs["PLOC"]
    ctx.upload_scene(sb)
    scaled = rays.copy()
    scaled["d"] *= F(2.0)
    scaled["tMax"] *= F(0.5)
    want = oracle.OracleScene(sb).trace(scaled, abi.SRT_TRAVERSE_CLOSEST)
    assert not np.array_equal(want["t"], oracle.OracleScene(sb).trace(rays, abi.SRT_TRAVERSE_CLOSEST)["t"])
    side = torch.cuda.Stream()
    d = _device_rays(rays)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d[:, 3:6] *= 2.0
        d[:, 8] *= 0.5
    got = _query(dev, abi, ctx, None, abi.SRT_TRAVERSE_CLOSEST, stream=side, d_rays=d)[0]  # synchronises `side` only
    _assert_key(got, want)
    occ = _query(dev, abi, ctx, None, stream=side, d_rays=d)
    assert np.array_equal(occ, (want["prim"] >= 0).astype(np.uint8))
    with torch.cuda.stream(side):
        t = ctx.trace_device(d, stream=side)
    side.synchronize()
    assert t.cpu().numpy().tobytes() == got.tobytes()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 11. after an update
@pytest.mark.parametrize("builder", ["LBVH", "PLOC"])
def test_after_refit_and_rebuild(ctx, dev, abi, oracle, soup3000, builder):
    sbs, rays, before = soup3000
    rays = rays[:8000]
    sb = sbs[builder]
    ctx.upload_scene(sb)
    tri = RF.scene_triangles(sb)
    first, count = 200, 700
    rng = np.random.default_rng(2)
    tri["p"][first:first + count] += rng.normal(0, 0.5, (count, 1, 3)).astype(F)
    ctx.update_triangles(first, tri[first:first + count])
    ctx.refit()
    moved = RF.moved_scene(sb, tri)
    want = oracle.OracleScene(moved).trace(rays, abi.SRT_TRAVERSE_CLOSEST)
    assert not np.array_equal(want["prim"], before["prim"][:8000])
    refit, _ = _check(dev, abi, oracle, ctx, moved, rays, want)
    nodes = ctx.bvh(0)
    ctx.rebuild()
    assert ctx.bvh(0).tobytes() != nodes.tobytes()  # the tree changed ...
    rebuilt, _ = _check(dev, abi, oracle, ctx, moved, rays, want)
    assert rebuilt.tobytes() == refit.tobytes()     # ... and the answer did not


# ------------------------------------------------------------------------------------------------ 12. side effects, errors
def test_side_effects_and_errors(ctx, dev, abi, camera, soup3000):
    sbs, rays, want = soup3000
    rays = rays[:4096]
    sb = sbs["PLOC"]
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(64, 36, 2, 4, seed=5, traversal=abi.SRT_TRAVERSE_CLOSEST)
    first = ctx.render_image(p)[0]
    info, ms, stats = ctx.launch_info(), ctx.last_kernel_ms(), ctx.stats()
    tunables = {k: ctx.get_tunable(k) for k in ("ploc_radius", "fast_div", "wavefront", "lds_tree", "wf_resident_max")}
    dev.host_random_reset()
    draws = [dev.host_random_float() for _ in range(3)]
    dev.host_random_reset()
    dev.host_random_float()
    for traversal in (abi.SRT_TRAVERSE_CLOSEST, abi.SRT_TRAVERSE_FAITHFUL, None):
        _query(dev, abi, ctx, rays, traversal, records=traversal is not None)
    assert (ctx.launch_info(), ctx.last_kernel_ms(), ctx.stats()) == (info, ms, stats)
    assert [dev.host_random_float() for _ in range(2)] == draws[1:]
    assert {k: ctx.get_tunable(k) for k in tunables} == tunables
    assert ctx.render_image(p)[0].tobytes() == first.tobytes()
    assert ctx.launch_info() == info

    # errors: refused on the host, nothing launched, the outputs keep their sentinel.  Every address below is either NULL
    # or inside a live buffer: a misaligned pointer is a live buffer's address plus a few bytes.
    n = len(rays)
    d_rays = torch.cat([_device_rays(rays), torch.zeros((1, 9), dtype=torch.float32, device="cuda")])
    d_hits = torch.full(((n + PAD) * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_recs = torch.full(((n + PAD) * REC,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_occ = torch.full((n + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    R, H, RC, O = d_rays.data_ptr(), d_hits.data_ptr(), d_recs.data_ptr(), d_occ.data_ptr()
    assert R % 16 == 0 and H % 16 == 0 and RC % 16 == 0
    CL = abi.SRT_TRAVERSE_CLOSEST
    trace, occluded = dev.lib.srtTraceRaysDevice, dev.lib.srtOccludedDevice

    def refused(rc, text, c=ctx):
        assert rc != 0 and text in dev.lib.srtLastError(c.h), (rc, dev.lib.srtLastError(c.h))
        torch.cuda.synchronize()
        for buf in (d_hits, d_recs, d_occ):
            assert bool((buf == SENTINEL).all())

    refused(trace(ctx.h, R, -1, CL, H, RC, None), b"negative")
    refused(occluded(ctx.h, R, -1, O, None), b"negative")
    refused(trace(ctx.h, None, n, CL, H, RC, None), b"null rays")
    refused(occluded(ctx.h, None, n, O, None), b"null rays")
    refused(trace(ctx.h, R, n, CL, None, None, None), b"no output")
    refused(occluded(ctx.h, R, n, None, None), b"no output")
    refused(trace(ctx.h, R + 2, n, CL, H, RC, None), b"rays are not aligned")
    refused(occluded(ctx.h, R + 1, n, O, None), b"rays are not aligned")
    refused(trace(ctx.h, R, n, CL, H + 8, RC, None), b"hits are not aligned")
    refused(trace(ctx.h, R, n, CL, H, RC + 2, None), b"records are not aligned")
    for bad in (2, -1, 7):
        refused(trace(ctx.h, R, n, bad, H, RC, None), b"neither")
    assert trace(None, R, n, CL, H, RC, None) != 0 and occluded(None, R, n, O, None) != 0
    fresh = dev.Context(0)
    try:
        refused(trace(fresh.h, R, n, CL, H, RC, None), b"no scene", fresh)
        refused(occluded(fresh.h, R, n, O, None), b"no scene", fresh)
    finally:
        fresh.close()
    with pytest.raises(dev.SrtError, match="neither"):
        ctx.trace_device(d_rays, traversal=5)
    # updated and not refitted: refused in checkSceneReady's words; then refitted, so that the shared context works again
    tri = RF.scene_triangles(sb)
    ctx.update_triangles(0, tri[:16])
    try:
        refused(trace(ctx.h, R, n, CL, H, RC, None), b"geometry was updated")
        refused(occluded(ctx.h, R, n, O, None), b"geometry was updated")
    finally:
        ctx.refit()
    got = _query(dev, abi, ctx, rays, CL)[0]
    _assert_key(got, want[:n])
