"""The head of the walks on the device (csrc/srt_wavefront.hip swapStep, csrc/srt_regroup.h SrtRegroupWalk::head; tunable
"wf_head", default 1): where every walk of the sequence begins at a leaf of spheres alone, the path-pool kernel's whole-tree
form tests that leaf where its swap step sets a new ray up and starts the walk at the leaf's miss word.  Nothing a frame
holds may move by a bit: every case compares the accumulators of wf_head 0 and 1 as uint32, zero tolerance, through the
production and the profiling instance, and against the CPU oracle's frame.  64 x 48, 4 spp, 4 bounces, seed 1.

The profiling instance counts the swap steps that ran the head and the lanes they ran it for (wf_profile()["far_node"]: the
slot of the hybrid form's visits outside LDS, free in this form).  A ray is started once and handed over once, and the swap
step's lanes count both, so with the head on its lanes are half the swap step's; with it off, for whatever reason, zero.

  * masterchief: a head of two spheres; also through the moments instance, and the primitive-step lanes fall;
  * the ground alone in the head leaf; the ground and a MOVING sphere; a world that is one leaf of two spheres (miss word
    DONE: the walk is over when the swap step ends);
  * no head: a first leaf of a sphere and a triangle, a world of two items, wf_regroup 1 and 0 (whose frames are mode 2's);
  * a sphere of negative radius in the head leaf (srtUpdateSpheres + srtRefitScene): its box is no longer ordered, so the
    launch takes neither the sequence nor its head and walks the reference tree, where every visit is the exact test --
    the frames agree with each other and with the step scheduler's;
  * rays with a zero direction component (the cameras of tests/planar_scenes.py): no such ray is certified, so every lane
    of the head takes the exact box test."""
import numpy as np
import pytest

import planar_scenes as P
import wf_head_scenes as S
from test_gpu_planar_frames import _assert_frame
from test_gpu_regroup import _render, forms  # noqa: F401  (forms: forces the whole-tree form)

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES, SEED = 64, 48, 4, 4, 1


@pytest.fixture
def head(forms):
    saved = forms.get_tunable("wf_head")
    yield forms
    forms.set_tunable("wf_head", saved)


@pytest.fixture(scope="module")
def wanted(abi, oracle):
    """The oracle's accumulators per (scene, camera), made once and handed out read-only."""
    made = {}

    def want(key, sb, cam):
        if key not in made:
            acc = oracle.OracleScene(sb).render(cam, _params(abi), oracle.RNG_COUNTER, threads=8, want_rgba=False)[0]
            acc.setflags(write=False)
            made[key] = acc
        return made[key]
    return want


def _params(abi):
    return abi.default_render_params(W, H, SPP, BOUNCES, seed=SEED)


def _frames(ctx, p, regroup=2):
    """{wf_head: (accumulators of the production instance, of the profiling instance, its profile)}"""
    out = {}
    for on in (0, 1):
        ctx.set_tunable("wf_head", on)
        plain = _render(ctx, p, regroup)[0]
        prof = _render(ctx, p, regroup, profile=True)[0]
        out[on] = (plain, prof, ctx.wf_profile())
    return out


def _check(ctx, abi, want, expect_head, regroup=2, what=""):
    p = _params(abi)
    fr = _frames(ctx, p, regroup)
    for on in (0, 1):
        for k, name in enumerate(("production", "profiling")):
            if want is not None:
                _assert_frame(fr[on][k], want, (what, name, "wf_head", on, "against the oracle"))
            assert fr[on][k].view(np.uint32).tobytes() == fr[0][0].view(np.uint32).tobytes(), (what, name, "wf_head", on)
    off, on = fr[0][2], fr[1][2]
    assert off["far_node"]["runs"] == 0 and off["far_node"]["lanes"] == 0
    started = on["swap"]["lanes"] // 2
    print("%s: rays %d, head executions %d, head lanes %d; primitive-step lanes %d -> %d, node lanes %d -> %d" % (
        what, started, on["far_node"]["runs"], on["far_node"]["lanes"], off["prim"]["lanes"], on["prim"]["lanes"], off["node"]["lanes"], on["node"]["lanes"]))
    assert on["swap"]["lanes"] == off["swap"]["lanes"] and on["swap"]["lanes"] % 2 == 0 and started >= W * H * SPP
    if expect_head:
        assert on["far_node"]["lanes"] == started and 0 < on["far_node"]["runs"] <= on["swap"]["runs"]
        assert on["node"]["lanes"] == off["node"]["lanes"] - started  # the head leaf's visit, one per ray, left the node step
    else:
        assert on["far_node"]["runs"] == 0 and on["far_node"]["lanes"] == 0
        assert on["node"]["lanes"] == off["node"]["lanes"] and on["prim"]["lanes"] == off["prim"]["lanes"]
    return fr


def test_masterchief(head, srt, abi, camera, wanted):
    ctx = head
    sb = srt.scenes.scene_masterchief()
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    fr = _check(ctx, abi, wanted("masterchief", sb, camera), True, what="masterchief")
    # its primitive-step lanes fall: every ray's tests of the head leaf's two spheres have left that step
    assert fr[1][2]["prim"]["lanes"] < fr[0][2]["prim"]["lanes"]
    # the moments instance
    p = _params(abi)
    got = {}
    for on in (0, 1):
        ctx.set_tunable("wf_head", on)
        got[on] = _render(ctx, p, 2, moments=True)
    for a, b in zip(got[0], got[1]):
        assert a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes()
    assert got[1][0].view(np.uint32).tobytes() == fr[0][0].view(np.uint32).tobytes()


@pytest.mark.parametrize("scene", ["ground_alone", "ground_and_moving", "two_spheres"])
def test_scenes_with_a_head(head, abi, camera, wanted, scene):
    ctx = head
    sb = getattr(S, scene)(abi)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    assert ctx.regroup_walk() is not None, "the upload built no walk sequence"
    fr = _check(ctx, abi, wanted(scene, sb, camera), True, what=scene)
    assert fr[1][2]["prim"]["lanes"] < fr[0][2]["prim"]["lanes"]
    if scene == "two_spheres":  # the tree is the head leaf: nothing is left for the traversal steps
        assert fr[1][2]["node"]["lanes"] == 0 and fr[1][2]["prim"]["lanes"] == 0


@pytest.mark.parametrize("scene", ["ground_and_triangle", "two_items"])
def test_scenes_without_a_head(head, abi, camera, wanted, scene):
    ctx = head
    sb = getattr(S, scene)(abi)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    assert ctx.regroup_walk() is not None, "the upload built no walk sequence"
    _check(ctx, abi, wanted(scene, sb, camera), False, what=scene)


@pytest.mark.parametrize("regroup", [1, 0])
def test_other_walks_have_no_head(head, abi, camera, wanted, regroup):
    ctx = head
    sb = S.ground_and_moving(abi)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    fr = _check(ctx, abi, wanted("ground_and_moving", sb, camera), False, regroup=regroup, what="wf_regroup %d" % regroup)
    ctx.set_tunable("wf_head", 1)
    assert _render(ctx, _params(abi), 2)[0].view(np.uint32).tobytes() == fr[1][0].view(np.uint32).tobytes()


def test_negative_radius_in_the_head_leaf(head, abi, camera):
    ctx = head
    sb = S.ground_alone(abi)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    walk = ctx.regroup_walk()
    assert walk is not None and ctx.slab_scene()[1] == 1
    sph = np.zeros(len(sb.spheres), abi.SPHERE_DTYPE)
    for i, s in enumerate(sb.spheres):
        sph[i] = (tuple(s.center0), tuple(s.center1), s.time0, s.time1, -s.radius if i == 0 else s.radius, s.material)
    ctx.update_spheres(0, sph)
    ctx.refit()
    assert ctx.slab_scene()[1] == 0  # the ground's box has min > max: the launch walks the reference tree, without a head
    assert all(np.array_equal(x, y) for x, y in zip(walk, ctx.regroup_walk()))
    fr = _check(ctx, abi, None, False, what="negative radius")
    ctx.set_tunable("wavefront", 0)
    step = ctx.render_image(_params(abi))
    ctx.set_tunable("wavefront", 1)
    assert fr[1][0].view(np.uint32).tobytes() == step[0].view(np.uint32).tobytes()


@pytest.mark.parametrize("case", P.CONFIGS[:2] + P.CONFIGS[4:], ids=["x-poszero", "x-negzero", "z-poszero", "z-negzero"])
def test_rays_with_a_zero_component(head, abi, wanted, case):
    ctx = head
    axis, nz = case
    sb = S.ground_and_moving(abi)
    cam = P.camera(abi, axis, nz)
    ctx.upload_scene(sb)
    ctx.set_camera(cam)
    _check(ctx, abi, wanted(("planar",) + tuple(case), sb, cam), True, what="planar axis %d, %s zero" % (axis, "-" if nz else "+"))
