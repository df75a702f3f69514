"""The regrouped tree's walk sequence on the device (csrc/srt_regroup.h srtRegroupWalk, csrc/srt_wavefront.hip's set-up copy;
tunable "wf_regroup" 2, the default): the whole-tree form of the path-pool kernel walks the regrouped tree without the gates
that rarely cull a ray, and nothing a frame holds may move by a bit.

  * frames: the four scenes of test_gpu_regroup at its sizes; wf_regroup 2 against 1 against 0 against the step scheduler,
    accumulators byte-identical through the production, the moments and the profiling instance;
  * the LDS copy IS the sequence: the profiling instance's node lanes under 2 lie below those under 1 on every scene, below
    0.9 x on masterchief; on the miss scenes of tests/planar_scenes.py -- no ray hits, the count is a function of the box
    verdicts alone -- the count under 2 EQUALS the float32 replay of the closed gate over Context.regroup_walk(), and the
    count under 1 still equals the replay over Context.regroup();
  * planar frames: the touch and miss frames of planar_scenes under 2 are the oracle's accumulators, bit for bit (every ray
    there has a +-0 component, so kept gates take boxHitOrGate);
  * counters: a counting launch with the tunable at 2 returns the oracle's eight counters (it walks the reference tree);
  * refit: after srtUpdateTriangles + srtUpdateSpheres + srtRefitScene the sequence is what it was (mask, sources, links,
    entries), the frame under 2 is the frame under 0, and the count under 2 still lies below that under 1;
  * gate off: a scene that loses boxOrderedScene in a refit (a sphere of negative radius) walks the reference tree under 2
    as it does under 1."""
import numpy as np
import pytest

import exact_scenes as X
import planar_scenes as P
import regroup_elide as E
from test_gpu_planar_frames import H, W, Planar, _assert_frame, _id
from test_gpu_regroup import COUNTERS, SCENES, _bits, _node_visits, _render, _soup_mesh, forms  # noqa: F401  (forms: forces the whole-tree form)
from test_regroup_host import _intervals

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def planar(abi, oracle):
    return Planar(abi, oracle)


def _same_walk(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_frames_are_bit_identical(forms, srt, abi, camera, scene):
    ctx = forms
    make, (w, h, spp, bounces) = SCENES[scene]
    ctx.upload_scene(make(srt, abi))
    ctx.set_camera(camera)
    rg, walk = ctx.regroup(), ctx.regroup_walk()
    assert rg is not None and walk is not None, "the upload built no walk sequence"
    keep, src, links, entry = walk
    E.check_sequence(rg[0], np.array([int(r) for r in _world_refs(rg[0], entry)], np.int32), keep, src, links, entry)
    p = abi.default_render_params(w, h, spp, bounces, seed=9)
    frames = {m: _render(ctx, p, m) for m in (2, 1, 0)}
    ctx.set_tunable("wavefront", 0)
    step = ctx.render_image(p)
    assert ctx.launch_info()["lds_tree_mode"] in (1, 2), ctx.launch_info()
    step_m = ctx.render_image_moments(p)
    ctx.set_tunable("wavefront", 1)
    assert np.isfinite(np.asarray(step[0])[..., :3]).any() and np.asarray(step[0])[..., :3].max() > 0
    for m in (2, 1, 0):
        for a, c in zip(frames[m], step):
            assert a.tobytes() == c.tobytes(), (scene, m)
        for a, c in zip(_render(ctx, p, m, moments=True), step_m):
            assert a.tobytes() == c.tobytes(), (scene, "moments", m)
    visits = {}
    for m in (2, 1, 0):
        assert _render(ctx, p, m, profile=True)[0].tobytes() == step[0].tobytes(), (scene, "profiling", m)
        visits[m] = _node_visits(ctx)
    print("%s: node lanes of the frame, reference tree %d, regrouped %d, sequence %d (x %.3f of the regrouped tree's); records %d of %d"
          % (scene, visits[0], visits[1], visits[2], visits[2] / visits[1], len(src), len(rg[0])))
    assert 0 < visits[2] < visits[1] < visits[0]
    if scene == "masterchief":
        assert visits[2] < 0.9 * visits[1]


def _world_refs(rg, entry):
    """The world list of the uploaded scene in the flattened array's terms, from the scene description: a tree's root is the
    first record of its node range (ranges follow one another in world order), a primitive is told by its entry word."""
    refs = rg.view(np.int32)
    out, at = [], 0
    for e in entry:
        e = int(e)
        if e < 0:  # a bare primitive's root word: its 16-bit reference, sign-extended
            out.append(((e & 0xffff) ^ 0x8000) - 0x8000)
            continue
        out.append(at * 32)
        # behind this tree: a tree of k leaves has 2 k - 1 records in pre-order
        todo, n = [at], 0
        while todo:
            i = todo.pop()
            n += 1
            if refs[i, 3] >= 0:
                todo += [int(refs[i, 7]) >> 5, int(refs[i, 3]) >> 5]
        at += n
    return out


# ---------------------------------------------------------------------------------------------------- the LDS copy is the sequence
@pytest.mark.parametrize("case", P.CONFIGS, ids=[_id(c) for c in P.CONFIGS])
def test_node_lanes_are_the_replay_of_the_sequence(forms, abi, oracle, planar, case):
    ctx = forms
    axis, nz = case
    sb, osc = planar.scene(axis, None)
    cam = P.camera(abi, axis, nz)
    p = planar.params(2)
    want_acc, want_st = planar.want(axis, nz, None, 2)
    assert want_st["rays"] == want_st["samples"] == W * H * 2
    ctx.upload_scene(sb)
    ctx.set_camera(cam)
    rg, walk = ctx.regroup(), ctx.regroup_walk()
    assert rg is not None and walk is not None
    keep, src, links, entry = walk
    assert len(entry) == 1 and 0 < len(src) < len(rg[0])
    rays, _ = P.camera_rays(oracle, abi, osc, cam, p)
    binary = int(P.gate_replay(rg[0], rays)["closed"][0].sum())
    a1, b1, inside = _intervals(rg[0], rays, gates=True)
    sequence = int(E.sequence_walk(rg[0], src, links, int(entry[0]), inside & ~(b1 <= a1))[0].sum())
    _assert_frame(_render(ctx, p, 2)[0], want_acc, (case, "wf_regroup 2"))
    _assert_frame(_render(ctx, p, 2, profile=True)[0], want_acc, (case, "profiling, wf_regroup 2"))
    lanes2 = _node_visits(ctx)
    _assert_frame(_render(ctx, p, 1, profile=True)[0], want_acc, (case, "profiling, wf_regroup 1"))
    lanes1 = _node_visits(ctx)
    print("%s: node lanes, regrouped %d (replay %d), sequence %d (replay %d)" % (_id(case), lanes1, binary, lanes2, sequence))
    assert lanes2 == sequence, (lanes2, sequence)
    assert lanes1 == binary, (lanes1, binary)
    assert sequence != binary


# ---------------------------------------------------------------------------------------------------- planar frames
PLANAR = [(axis, nz, touch) for axis, nz in P.CONFIGS for touch in (0, 1, None)]


@pytest.mark.parametrize("case", PLANAR, ids=[_id(c[:2]) + {0: "", 1: "-touch", None: "-miss"}[c[2]] for c in PLANAR])
def test_planar_frames(forms, abi, planar, case):
    ctx = forms
    axis, nz, touch = case
    sb, _ = planar.scene(axis, touch)
    want_acc, _ = planar.want(axis, nz, touch)
    ctx.upload_scene(sb)
    ctx.set_camera(P.camera(abi, axis, nz))
    assert ctx.regroup_walk() is not None, "the upload built no walk sequence"
    p = planar.params()
    _assert_frame(_render(ctx, p, 2)[0], want_acc, (case, "wf_regroup 2"))
    _assert_frame(_render(ctx, p, 2, moments=True)[0], want_acc, (case, "moments, wf_regroup 2"))
    _assert_frame(_render(ctx, p, 2, profile=True)[0], want_acc, (case, "profiling, wf_regroup 2"))
    assert _node_visits(ctx) > 0


# ---------------------------------------------------------------------------------------------------- counters
def test_counters_are_the_reference_walks(forms, srt, abi, oracle, camera):
    ctx = forms
    sb = X.mesh(srt, abi, "A")
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    assert ctx.regroup_walk() is not None
    p = abi.default_render_params(64, 48, 4, 4, seed=9)
    plain = _render(ctx, p, 2)[0]
    p.countStats = 1
    acc = _render(ctx, p, 2)[0]
    stats = ctx.stats()
    assert acc.tobytes() == plain.tobytes()
    want_acc, _, want = oracle.OracleScene(sb).render(camera, p, oracle.RNG_COUNTER, threads=8, want_rgba=False)
    assert _bits(plain).tobytes() == _bits(want_acc).tobytes()
    for k in COUNTERS:
        assert stats[k] == want[k], (k, stats[k], want[k])
    assert want["nodeVisits"] > 40 * want["rays"]  # the reference walk's count


# ---------------------------------------------------------------------------------------------------- refit, and the gate off
def _spheres(abi, sb, radius=None):
    sph = np.zeros(len(sb.spheres), abi.SPHERE_DTYPE)
    for i, s in enumerate(sb.spheres):
        sph[i] = (tuple(s.center0), tuple(s.center1), s.time0, s.time1, s.radius if radius is None else radius(s.radius), s.material)
    return sph


def test_refit_keeps_the_sequence(forms, srt, abi, camera):
    ctx = forms
    sb = _soup_mesh(srt)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    before, walk = ctx.regroup()[0], ctx.regroup_walk()
    rng = np.random.default_rng(3)
    tri = np.concatenate(sb.triangles).copy()
    tri["p"] += rng.normal(0, 0.25, tri["p"].shape).astype(F)
    ctx.update_triangles(0, tri)
    ctx.update_spheres(0, _spheres(abi, sb, lambda r: r * 0.999))
    ctx.refit()
    assert ctx.slab_scene()[1] == 1
    assert not np.array_equal(_bits(before), _bits(ctx.regroup()[0]))
    assert _same_walk(walk, ctx.regroup_walk())
    p = abi.default_render_params(96, 64, 8, 4, seed=9)
    on = _render(ctx, p, 2, profile=True)
    lanes2 = _node_visits(ctx)
    _render(ctx, p, 1, profile=True)
    lanes1 = _node_visits(ctx)
    off = _render(ctx, p, 0)
    assert 0 < lanes2 < lanes1
    assert on[0].tobytes() == off[0].tobytes() == _render(ctx, p, 2)[0].tobytes()
    ctx.set_tunable("wavefront", 0)
    step = ctx.render_image(p)
    ctx.set_tunable("wavefront", 1)
    assert on[0].tobytes() == step[0].tobytes()


def test_gate_off_without_ordered_boxes(forms, srt, abi, camera):
    ctx = forms
    sb = _soup_mesh(srt)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    walk = ctx.regroup_walk()
    assert walk is not None and ctx.slab_scene()[1] == 1
    p = abi.default_render_params(96, 64, 8, 4, seed=9)
    ctx.update_spheres(0, _spheres(abi, sb, lambda r: -r))
    ctx.refit()
    assert ctx.slab_scene()[1] == 0  # a box with min > max: the regrouped tree's lemma no longer holds
    assert _same_walk(walk, ctx.regroup_walk())  # (the sequence stays where it is; the launch does not take it)
    frames, lanes = {}, {}
    for m in (2, 1, 0):
        frames[m] = _render(ctx, p, m, profile=True)[0]
        lanes[m] = _node_visits(ctx)
    assert lanes[2] == lanes[1] == lanes[0] > 0, lanes
    assert frames[2].tobytes() == frames[1].tobytes() == frames[0].tobytes() == _render(ctx, p, 2)[0].tobytes()
    ctx.set_tunable("wavefront", 0)
    step = ctx.render_image(p)
    ctx.set_tunable("wavefront", 1)
    assert frames[2].tobytes() == step[0].tobytes()
