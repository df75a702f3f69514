"""Every form of the render kernel on frames made of rays with a direction component of exactly +-0 (tests/planar_scenes.py;
the conditions that make these frames what they claim to be are asserted on the CPU in tests/test_planar_scenes.py).  Such
a ray is never certified: every node visit takes the IEEE block, and in the path-pool kernel's whole-tree form the inner
nodes of the regrouped tree take the gate form there (boxHitOrGate) -- code that camera rays and fuzzy
reflections never reach.  Every comparison is bit for bit; nothing here has a tolerance.

  * frames: axis x sign of the zero x `touch` (boxes with a plane at exactly the rays' origin coordinate) through the four
    forms of conftest.node_path at 48 x 32, 4 spp, 6 bounces: the accumulator is the oracle's, byte for byte, and a counting
    launch's eight counters are the oracle's.  The whole-tree form also with wf_regroup 1 and 0, through the moments and the
    profiling instance;
  * per ray: srtRenderAov at bounces 0, 1, 2 on the `touch` scenes against the oracle's world.hit (primitive, bits of t, four
    counters), as many records as the oracle's own paths have, each with d[axis] == 0;
  * the device path loop (pathloop.render fused, unfused, compacted) is the render;
  * the gate, in the walk: on the miss scene -- all background, closest = +inf throughout -- the profiling instance's node
    visits are the oracle's nodeVisits with wf_regroup 0 and, with wf_regroup 1, the float32 replay of the CLOSED gate over
    the context's own regrouped array, which differs from the totals a gate in the reference's form or an open gate gives."""
import copy
import os

import numpy as np
import pytest

import planar_scenes as P
from conftest import render_counted
from test_gpu_parity import assert_aov_matches_oracle
from test_gpu_regroup import COUNTERS, _node_visits, _render, forms  # noqa: F401  (forms: the fixture that forces the whole-tree form)

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 48, 32, 4, 6
CASES = [(axis, nz, touch) for axis, nz in P.CONFIGS for touch in (0, 1)]


def _id(case):
    return "axis%d-%s%s" % (case[0], "negzero" if case[1] else "poszero", "-touch" if len(case) > 2 and case[2] else "")


class Planar:
    """Scenes, oracle instances, cameras and the oracle's frames, each made once per module and handed out read-only."""

    def __init__(self, abi, oracle):
        self.abi, self.oracle = abi, oracle
        self.scenes, self.frames = {}, {}
        self.threads = min(16, os.cpu_count() or 8)

    def scene(self, axis, touch):
        """touch None: the miss scene."""
        key = (axis, touch)
        if key not in self.scenes:
            sb = P.miss_scene(self.abi, axis) if touch is None else P.mirror_scene(self.abi, axis, touch)
            self.scenes[key] = (sb, self.oracle.OracleScene(sb))
        return self.scenes[key]

    def params(self, spp=SPP):
        return self.abi.default_render_params(W, H, spp, BOUNCES, seed=9)

    def want(self, axis, nz, touch, spp=SPP):
        """(accum, counters) of the oracle: its single running sum per pixel (one chunk)."""
        key = (axis, nz, touch, spp)
        if key not in self.frames:
            acc, _, st = self.scene(axis, touch)[1].render(P.camera(self.abi, axis, nz), self.params(spp), self.oracle.RNG_COUNTER,
                                                           threads=self.threads, want_rgba=False)
            acc.setflags(write=False)
            self.frames[key] = (acc, st)
        return self.frames[key]


@pytest.fixture(scope="module")
def planar(abi, oracle):
    return Planar(abi, oracle)


def _expected_mode(node_path, nodes):
    if node_path == "l1_nodes":
        return (0,)
    if node_path == "lds_tree":
        return (1, 2)
    return (4,) if node_path == "hybrid" and nodes > 24 else (3,)


def _assert_frame(acc, want, what):
    assert acc.dtype == want.dtype == np.float32 and acc.shape == want.shape
    if acc.tobytes() != want.tobytes():
        bad = (acc.view(np.uint32) != want.view(np.uint32)).any(axis=-1)
        y, x = (int(v) for v in np.argwhere(bad)[0])
        pytest.fail("%r: %d of %d pixels differ; first (x %d, y %d): kernel %r, oracle %r" % (what, int(bad.sum()), bad.size, x, y, acc[y, x].tolist(), want[y, x].tolist()))


# ---------------------------------------------------------------------------------------------------- frames by form
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_frames_by_form(ctx, dev, abi, planar, node_path, case):
    axis, nz, touch = case
    sb, _ = planar.scene(axis, touch)
    want_acc, want_st = planar.want(axis, nz, touch)
    saved = {k: ctx.get_tunable(k) for k in ("wf_regroup", "wf_profile")}
    try:
        ctx.upload_scene(sb)
        ctx.set_camera(P.camera(abi, axis, nz))
        nodes = len(ctx.bvh(0))
        p = planar.params()
        assert dev.plan_spp_chunks(W, H, SPP, p.sppChunks) == 1
        q = copy.copy(p)
        q.countStats = 1
        acc, _ = render_counted(ctx, q, node_path)
        stats = ctx.stats()
        assert ctx.launch_info()["lds_tree_mode"] in _expected_mode(node_path, nodes), (case, node_path, ctx.launch_info())
        _assert_frame(acc, want_acc, (case, node_path))
        assert want_st["texelFetches"] == 0
        for k in COUNTERS:
            assert stats[k] == want_st[k], (case, node_path, k, stats[k], want_st[k])
        if node_path != "wavefront":
            return
        # the whole-tree form: the regrouped tree and the reference tree, through the production, the moments and the profiling instance
        assert ctx.regroup() is not None, "the upload built no regrouped tree"
        for regroup in (1, 0):
            _assert_frame(_render(ctx, p, regroup)[0], want_acc, (case, "wf_regroup", regroup))
            _assert_frame(_render(ctx, p, regroup, moments=True)[0], want_acc, (case, "moments, wf_regroup", regroup))
            _assert_frame(_render(ctx, p, regroup, profile=True)[0], want_acc, (case, "profiling, wf_regroup", regroup))
            assert _node_visits(ctx) > 0
    finally:
        for k, v in saved.items():
            ctx.set_tunable(k, v)


# ---------------------------------------------------------------------------------------------------- per ray
@pytest.mark.parametrize("case", P.CONFIGS, ids=[_id(c) for c in P.CONFIGS])
def test_per_ray_on_the_touch_scenes(ctx, abi, planar, node_path, case):
    """The counting instance of each form, ray by ray.  min_rays is the census itself: the number of first samples whose
    oracle path has a ray at that bounce."""
    axis, nz = case
    sb, osc = planar.scene(axis, 1)
    cam = P.camera(abi, axis, nz)
    ctx.upload_scene(sb)
    ctx.set_camera(cam)
    nodes = len(ctx.bvh(0))
    p = planar.params(1)
    lengths = np.array([len(osc.sample_path(cam, p, x, y, 0)[0]) for y in range(H) for x in range(W)])
    assert (lengths >= 1).all() and (lengths > 2).sum() > 100
    for depth in range(3):
        aov = ctx.render_aov(p, depth)
        assert ctx.launch_info()["lds_tree_mode"] in _expected_mode(node_path, nodes), (case, node_path, ctx.launch_info())
        census = int((lengths > depth).sum())
        assert assert_aov_matches_oracle(aov, osc, abi, (case, node_path, depth), min_rays=census) == census
        rec = aov.reshape(-1)
        rec = rec[rec["valid"] == 1]
        assert (rec["d"][:, axis] == 0).all() and (rec["o"][:, axis] == 0).all(), (case, node_path, depth)
        if depth == 0:
            assert np.signbit(rec["d"][:, axis]).any() == bool(nz)


# ---------------------------------------------------------------------------------------------------- the device path loop
@pytest.mark.parametrize("case", [(0, 1, 1), (1, 0, 1), (2, 1, 0)], ids=_id)
def test_loop_is_the_render(ctx, srt, abi, planar, case):
    import importlib

    import torch
    pathloop = importlib.import_module("sexy-raytracer_amd.pathloop")
    axis, nz, touch = case
    ctx.upload_scene(planar.scene(axis, touch)[0])
    ctx.set_camera(P.camera(abi, axis, nz))
    p = planar.params()
    want = ctx.render_image(p, want_rgba=False)[0]
    _assert_frame(want, planar.want(axis, nz, touch)[0], (case, "render_image"))
    for kw in ({"fused": True}, {"fused": False}, {"fused": True, "compact": True}, {"fused": False, "compact": True}):
        got = pathloop.render(ctx, p, **kw)
        torch.cuda.synchronize()
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32
        _assert_frame(got.cpu().numpy(), want, (case, kw))


# ---------------------------------------------------------------------------------------------------- the gate, in the walk
@pytest.mark.parametrize("case", P.CONFIGS, ids=[_id(c) for c in P.CONFIGS])
def test_gate_form_in_the_walk(forms, abi, oracle, planar, case):
    """The whole-tree form's profiling instance counts, per node visit, the lanes that perform it (srt_wavefront.hip: pLanes[0] +=
    popcount(ballot(here)) -- "node"/"lanes" of wf_profile).  On the miss scene no ray ever hits, so the count is a function
    of the box verdicts alone.  The regrouped walk visits MORE nodes than the reference walk here."""
    ctx = forms
    axis, nz = case
    sb, osc = planar.scene(axis, None)
    cam = P.camera(abi, axis, nz)
    p = planar.params(2)
    want_acc, want_st = planar.want(axis, nz, None, 2)
    assert want_st["rays"] == want_st["samples"] == W * H * 2
    ctx.upload_scene(sb)
    ctx.set_camera(cam)
    rg = ctx.regroup()
    assert rg is not None, "the upload built no regrouped tree"
    rays, _ = P.camera_rays(oracle, abi, osc, cam, p)
    totals = {k: int(v.sum()) for k, (v, _) in P.gate_replay(rg[0], rays).items()}
    assert len(set(totals.values())) == 3, totals
    _assert_frame(_render(ctx, p, 1)[0], want_acc, (case, "wf_regroup 1"))
    _assert_frame(_render(ctx, p, 1, profile=True)[0], want_acc, (case, "profiling, wf_regroup 1"))
    visits_on = _node_visits(ctx)
    _assert_frame(_render(ctx, p, 0, profile=True)[0], want_acc, (case, "profiling, wf_regroup 0"))
    visits_off = _node_visits(ctx)
    print("%s: node visits, reference tree %d (oracle %d), regrouped %d (replay: %s)" % (_id(case), visits_off, want_st["nodeVisits"], visits_on, totals))
    assert visits_off == want_st["nodeVisits"], (visits_off, want_st["nodeVisits"])
    assert visits_on == totals["closed"], (visits_on, totals)
    assert visits_on != totals["reference"] and visits_on != totals["open"], (visits_on, totals)
