"""The head leaf's sphere records in LDS (csrc/srt_wavefront.hip: the set-up of every launch copies the two records of the
walks' head leaf from DevScene::spheres into control words 32..55 behind the LDS tree, and the swap step reads them there
instead of through the vector memory path; tunable "wf_head", default 1).  With wf_head 0 none of that code runs, so
every case compares wf_head 1 with wf_head 0 on uint32 views, zero tolerance, and with the CPU oracle's frame where a
freshly built scene has the oracle's tree.  64 x 48, 4 spp, 4 bounces, seed 1, as tests/test_gpu_wf_head.py.

What a staged copy can get wrong and the loads it replaced could not:
  * the third quad of each of the two slots and the flag that asks for it: the first object moves, both move (the second
    alone: test_gpu_wf_head.py's ground_and_moving), a head of one moving sphere -- production, profiling and moments;
  * records rewritten between launches (srtUpdateSpheres + srtRefitScene): a stale copy would render the old sphere;
  * another scene without a head between two launches of one with a head, on one context;
  * a frame smaller than the pool: most workgroups claim no context, most swap steps start no ray;
  * a head of one sphere: the second slot holds zeros and is not tested."""
import numpy as np
import pytest

import wf_head_records_scenes as R
import wf_head_scenes as S
from test_gpu_planar_frames import _assert_frame
from test_gpu_regroup import _render, forms  # noqa: F401  (forms: forces the whole-tree form)
from test_gpu_wf_head import H, SPP, W, _check, _params, head, wanted  # noqa: F401  (head, wanted: fixtures)

pytestmark = pytest.mark.gpu


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint32).tobytes()


def _moments_agree(ctx, abi, production):
    """The moments instance with wf_head 0 and 1: every plane the same, the accumulators the production instance's."""
    got = {}
    for on in (0, 1):
        ctx.set_tunable("wf_head", on)
        got[on] = _render(ctx, _params(abi), 2, moments=True)
    for a, b in zip(got[0], got[1]):
        assert _bytes(a) == _bytes(b)
    assert _bytes(got[1][0]) == _bytes(production)


def _head_ran(prof):
    """The profile of a launch whose swap steps ran the head for every ray they started; returns the rays started."""
    started = prof["swap"]["lanes"] // 2
    assert prof["swap"]["lanes"] % 2 == 0 and started > 0
    assert prof["far_node"]["lanes"] == started and 0 < prof["far_node"]["runs"] <= prof["swap"]["runs"]
    return started


@pytest.mark.parametrize("scene", ["moving_ground_and_still", "both_moving", "moving_ground_alone"])
def test_moving_objects_in_the_head_leaf(head, abi, camera, wanted, scene):
    ctx = head
    sb = getattr(R, scene)(abi)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    assert ctx.regroup_walk() is not None, "the upload built no walk sequence"
    fr = _check(ctx, abi, wanted(scene, sb, camera), True, what=scene)
    assert fr[1][2]["prim"]["lanes"] < fr[0][2]["prim"]["lanes"]
    _moments_agree(ctx, abi, fr[0][0])


def test_second_object_moves_through_the_moments_instance(head, abi, camera, wanted):
    ctx = head
    sb = S.ground_and_moving(abi)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    fr = _check(ctx, abi, wanted("ground_and_moving", sb, camera), True, what="ground_and_moving")
    _moments_agree(ctx, abi, fr[0][0])


def test_records_rewritten_between_launches(head, abi, camera):
    ctx = head
    sb = S.ground_and_moving(abi)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    assert ctx.regroup_walk() is not None
    ctx.set_tunable("wf_head", 1)
    before = _render(ctx, _params(abi), 2)[0].copy()
    # the head's second sphere: another (positive) radius and another end of its motion; the tree keeps its topology
    ctx.update_spheres(0, R.sphere_records(abi, sb, {1: {"radius": 1.6, "center1": (-4.0, 3.1, -4.2)}}))
    ctx.refit()
    assert ctx.slab_scene()[1] == 1
    fr = _check(ctx, abi, None, True, what="after the update")  # wf_head 0 and 1, production and profiling; the head runs
    _head_ran(fr[1][2])
    ctx.set_tunable("wavefront", 0)
    step = ctx.render_image(_params(abi))[0]
    ctx.set_tunable("wavefront", 1)
    assert _bytes(step) == _bytes(fr[1][0]) == _bytes(fr[0][0])
    assert _bytes(fr[1][0]) != _bytes(before), "the update changed nothing: the case shows nothing"
    _moments_agree(ctx, abi, fr[0][0])
    # ... and back: the first launch's records again, the first launch's frame
    ctx.update_spheres(0, R.sphere_records(abi, sb, {}))
    ctx.refit()
    ctx.set_tunable("wf_head", 1)
    assert _bytes(_render(ctx, _params(abi), 2)[0]) == _bytes(before)


def test_launch_sequence_on_one_context(head, abi, camera, wanted):
    ctx = head
    with_head, without = R.both_moving(abi), S.ground_and_triangle(abi)
    ctx.set_tunable("wf_head", 1)
    ctx.upload_scene(with_head)
    ctx.set_camera(camera)
    first = _render(ctx, _params(abi), 2)[0].copy()
    _assert_frame(first, wanted("both_moving", with_head, camera), "the first launch against the oracle")
    ctx.upload_scene(without)
    ctx.set_camera(camera)
    fr = _check(ctx, abi, wanted("ground_and_triangle", without, camera), False, what="no head in between")
    assert fr[1][2]["far_node"]["runs"] == 0 and fr[1][2]["far_node"]["lanes"] == 0
    ctx.set_tunable("wf_head", 1)
    ctx.upload_scene(with_head)
    ctx.set_camera(camera)
    third = _render(ctx, _params(abi), 2)[0]
    assert _bytes(third) == _bytes(first)
    _render(ctx, _params(abi), 2, profile=True)
    _head_ran(ctx.wf_profile())


def test_frame_smaller_than_the_pool(head, abi, camera, oracle):
    ctx = head
    sb = R.both_moving(abi)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    p = abi.default_render_params(8, 8, 1, 4, seed=1)
    want = oracle.OracleScene(sb).render(camera, p, oracle.RNG_COUNTER, threads=4, want_rgba=False)[0]
    got = {}
    for on in (0, 1):
        ctx.set_tunable("wf_head", on)
        got[on] = (_render(ctx, p, 2)[0].copy(), _render(ctx, p, 2, profile=True)[0].copy(), ctx.wf_profile())
        for k, name in enumerate(("production", "profiling")):
            _assert_frame(got[on][k], want, ("8 x 8 at 1 spp", name, "wf_head", on))
    assert got[0][2]["far_node"]["runs"] == 0
    assert _head_ran(got[1][2]) >= 64 and got[1][2]["swap"]["lanes"] == got[0][2]["swap"]["lanes"]


def test_head_of_one_sphere(head, abi, camera, wanted):
    """wf_head_scenes.ground_alone: the second slot of the staged records is zeros and no lane tests it."""
    ctx = head
    sb = S.ground_alone(abi)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    fr = _check(ctx, abi, wanted("ground_alone", sb, camera), True, what="ground_alone")
    off, on = fr[0][2], fr[1][2]
    started = _head_ran(on)
    assert started >= W * H * SPP
    assert on["node"]["lanes"] == off["node"]["lanes"] - started  # the head leaf's visit, one per ray, left the node step
    # ... and the ground's test left the primitive step for every ray whose head box passed: at most one test per ray
    assert 0 < off["prim"]["lanes"] - on["prim"]["lanes"] <= started
    _moments_agree(ctx, abi, fr[0][0])
