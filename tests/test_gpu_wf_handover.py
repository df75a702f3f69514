"""The path-pool kernel's hand-over machinery (csrc/srt_wf_rings.h: enqueue specialised per call site, claim; the swap, hit,
restart and item-pull steps of csrc/srt_wavefront.hip) through the PRODUCTION instances -- the ring-capacity tests of
tests/test_gpu_exact_frames.py render through the counting ones -- and the moments instances.

Every frame: accumulators and RGBA8 equal bit for bit (NaNs by position) to the step-scheduler kernel's on the same context
(tunable wavefront = 0: one path per lane, no rings), and ctx.last_kernel_ms() -- which reports a workgroup that gave up
waiting on a ring -- raises nothing.  The scene is the first single-tree tier-B random scene of tests/exact_scenes.py whose
hits fall in all three material classes of the pool and whose rays also miss (found, and asserted, on the AOV records of
the first three bounces).  Forms: the whole tree in LDS (the ring operations specialised per call site), and the hybrid
form with 24 resident nodes (the generic ones).

  (a) 33 x 17 at 1 spp, 6 bounces: the pool is smaller than every ring, partial batches only, and the tiles hold pixels
      outside the image, so the item pull's "again" path runs;
  (b) test_every_ring_capacity's frame (16:9, sized from the CU count, 64 spp in 32 chunks, 6 bounces: levels >= 4 go
      through wfAttHi) at wf_pool 1024, 1536, 2048 x wf_swap_min 1, 32, 64;
  (c) maxBounce 0 and 1 on 33 x 17: items with nothing to trace, and every hit terminal;
  moments: (a) and wf_pool 1536 of (b) through srtRenderTilesMoments against the step scheduler's moments."""
import numpy as np
import pytest

import exact_scenes
from test_gpu_parity import path_pool_form

pytestmark = pytest.mark.gpu

FORMS = ("wavefront", "hybrid")
POOLS = (1024, 1536, 2048)
SWAP_MINS = (1, 32, 64)


def _same(got, want, what):
    """Bit for bit; a NaN must meet a NaN (whatever its payload)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.float32:
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), (what, "NaN positions", np.argwhere(gn != wn)[:4].tolist())
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~wn
    else:
        bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _big_frame(ctx, abi):
    """test_every_ring_capacity's frame: every workgroup gets at least 4096 work items."""
    cus = ctx.device_info()["cus"]
    W = 16
    while W * (W * 9 // 16) * 32 < 4096 * cus:
        W += 16
    return abi.default_render_params(W, W * 9 // 16, 64, 6, seed=4096, spp_chunks=32)


class Pinned:
    """The scene, and the step-scheduler kernel's frames of it: each rendered once, shared, read-only."""

    def __init__(self, ctx, abi, camera):
        self.ctx, self.abi, self.camera = ctx, abi, camera
        self.frames = {}
        # the first single-tree tier-B scene whose walks end in all three classes and in misses (a random scene may lie
        # inside one of its huge spheres: then no ray ever leaves it)
        first = 0
        for _ in range(16):
            self.seed, self.sb = exact_scenes.random_with_tree(abi, "B", first_seed=first)
            self.classes, self.misses = self._walk_ends()
            if self.classes == {0, 1, 2} and self.misses > 0:
                break
            first = self.seed + 1

    def _walk_ends(self):
        """({material class of the hits}, number of misses) over the AOV records of bounces 0 to 2 of a 64 x 36 frame."""
        sb, abi = self.sb, self.abi
        prims = np.concatenate(sb._prim_chunks)
        tri_mat = np.concatenate([t["material"] for t in sb.triangles])
        with path_pool_form(self.ctx, "wavefront"):
            self.upload()
            p = abi.default_render_params(64, 36, 1, 6, seed=3)
            rec = np.concatenate([self.ctx.render_aov(p, depth).reshape(-1) for depth in (0, 1, 2)])
        rec = rec[rec["valid"] == 1]
        classes = set()
        for pr in np.unique(rec["prim"][rec["prim"] >= 0]):
            kind, k = (int(x) for x in prims[pr])
            mat = int(tri_mat[k]) if kind == abi.SRT_PRIM_TRIANGLE else int(sb.spheres[k].material)
            pbr = sb.materials[mat].type == abi.SRT_MAT_PBR
            classes.add(0 if pbr and kind == abi.SRT_PRIM_TRIANGLE else 1 if pbr else 2)
        return classes, int((rec["prim"] == abi.SRT_NO_HIT).sum())

    def upload(self):
        self.ctx.upload_scene(self.sb)
        self.ctx.set_camera(self.camera)

    def want(self, key, p, moments=False):
        """The step scheduler's (accum, rgba) or (accum, moments, rgba) for p; the scene is uploaded.  Leaves wavefront = 1."""
        key = (key, moments)
        if key not in self.frames:
            self.ctx.set_tunable("wavefront", 0)
            out = self.ctx.render_image_moments(p) if moments else self.ctx.render_image(p)
            assert self.ctx.launch_info()["lds_tree_mode"] in (1, 2), self.ctx.launch_info()
            self.ctx.last_kernel_ms()
            for a in out:
                a.setflags(write=False)
            self.frames[key] = out
        self.ctx.set_tunable("wavefront", 1)
        return self.frames[key]


@pytest.fixture(scope="module")
def pinned(ctx, abi, camera):
    return Pinned(ctx, abi, camera)


def _render_and_compare(ctx, pf, p, want, what, moments=False):
    got = ctx.render_image_moments(p) if moments else ctx.render_image(p)
    info = ctx.launch_info()
    assert info["lds_tree_mode"] == pf.mode(), (what, info)
    ctx.last_kernel_ms()  # raises when a workgroup of the launch gave up waiting on a ring
    for g, w, name in zip(got, want, ("accum", "moments", "rgba") if moments else ("accum", "rgba")):
        _same(g, w, (what, name))
    return info


def test_scene_hits_every_class_and_misses(abi, pinned):
    """Hits (AOV records of bounces 0 to 2) on a triangle with a pbr material, on a sphere with a pbr material and on
    something else; rays that leave the scene; one tree that the forced hybrid form splits and that leaves room for every
    ring capacity the frames ask for."""
    assert pinned.classes == {0, 1, 2} and pinned.misses > 0, (pinned.seed, pinned.classes, pinned.misses)
    nodes = sum(exact_scenes.bvh_nodes(w.count) for w in pinned.sb.world if w.kind == abi.SRT_WORLD_BVH)
    assert pinned.sb.layout == 0 and 24 < nodes and 32 * nodes + 256 + 20 * max(POOLS) <= 160 * 1024


@pytest.mark.parametrize("form", FORMS)
def test_small_frame(ctx, abi, pinned, form):
    """(a), then (c)."""
    saved = ctx.get_tunable("wf_pool")
    try:
        with path_pool_form(ctx, form, resident=24) as pf:
            pinned.upload()
            for bounces in (6, 0, 1):
                p = abi.default_render_params(33, 17, 1, bounces, seed=33)
                want = pinned.want(("small", bounces), p)
                for pool in POOLS:
                    ctx.set_tunable("wf_pool", pool)
                    _render_and_compare(ctx, pf, p, want, (form, "33x17", bounces, pool))
            assert np.asarray(pinned.want(("small", 0), p)[0])[..., :3].max() == 0.0  # no bounces: black (main.cpp:36-37)
    finally:
        ctx.set_tunable("wf_pool", saved)


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("form", FORMS)
def test_every_ring_capacity_and_swap_threshold(ctx, abi, pinned, form, pool):
    """(b)."""
    saved = {k: ctx.get_tunable(k) for k in ("wf_pool", "wf_swap_min")}
    try:
        with path_pool_form(ctx, form, resident=24) as pf:
            pinned.upload()
            p = _big_frame(ctx, abi)
            want = pinned.want("big", p)
            ctx.set_tunable("wf_pool", pool)
            for swap_min in SWAP_MINS:
                ctx.set_tunable("wf_swap_min", swap_min)
                info = _render_and_compare(ctx, pf, p, want, (form, "ring frame", pool, swap_min))
                assert p.imageWidth * p.imageHeight * 32 >= 4096 * info["workgroups"], info
    finally:
        for k, v in saved.items():
            ctx.set_tunable(k, v)


@pytest.mark.parametrize("form", FORMS)
def test_moments_instances(ctx, abi, pinned, form):
    saved = ctx.get_tunable("wf_pool")
    try:
        with path_pool_form(ctx, form, resident=24) as pf:
            pinned.upload()
            ctx.set_tunable("wf_pool", 1536)
            for key, p in (("small-moments", abi.default_render_params(33, 17, 1, 6, seed=33)), ("big-moments", _big_frame(ctx, abi))):
                want = pinned.want(key, p, moments=True)
                _render_and_compare(ctx, pf, p, want, (form, key), moments=True)
                assert (np.asarray(want[1])[..., 3] == p.spp).all()
    finally:
        ctx.set_tunable("wf_pool", saved)
