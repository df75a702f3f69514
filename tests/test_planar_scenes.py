"""tests/planar_scenes.py on the CPU oracle, no GPU: the conditions that keep tests/test_gpu_planar_frames.py from being
vacuous.  For each of the three axes and both signs of the zero:

  * every ray of every bounce of the mirror scene has d[axis] == +-0 and o[axis] == 0; with the negative-zero camera at least a
    quarter of them carry -0.0, without it none does; paths bounce (mean length >= 1.8), the frame is lit, nothing is a NaN,
    triangles are shaded and spheres tested; the `touch` variant changes the oracle's node visits and has inner and leaf
    boxes with a plane at exactly 0 == o on the axis;
  * the miss scene is all background, one ray per sample; the float32 replay of aabb.h (tests/test_regroup_host.py
    _intervals / _entered) over the reference tree gives the oracle's nodeVisits, and over the regrouped array
    (srtTestRegroup) three pairwise different totals for the three forms a gate could take on a zero axis -- closed (the
    kernel's), the reference's own, open -- all of which enter the reference walk's leaves.  So a frame's node-visit count
    tells the three apart."""
import numpy as np
import pytest

import planar_scenes as P
from test_regroup_host import _flat, _regroup, _walk

W, H, SPP, BOUNCES = 48, 32, 4, 6
IDS = ["axis%d-%s" % (a, "negzero" if z else "poszero") for a, z in P.CONFIGS]


def _census(osc, cam, p, axis):
    """sample_path over every second pixel (a checkerboard), first sample: (rays, rays off the plane, rays with -0.0, lengths)."""
    rays = off = neg = 0
    lengths = []
    for y in range(p.imageHeight):
        for x in range(y % 2, p.imageWidth, 2):
            steps, colour = osc.sample_path(cam, p, x, y, 0)
            assert not np.isnan(colour).any() and not np.isnan(steps["o"]).any() and not np.isnan(steps["d"]).any()
            rays += len(steps)
            off += int(((steps["d"][:, axis] != 0) | (steps["o"][:, axis] != 0)).sum())
            neg += int(np.signbit(steps["d"][:, axis]).sum())
            lengths.append(len(steps))
    return rays, off, neg, np.array(lengths)


@pytest.mark.parametrize("axis,negative_zero", P.CONFIGS, ids=IDS)
def test_mirror_scene_rays_stay_in_the_plane(oracle, abi, axis, negative_zero):
    cam = P.camera(abi, axis, negative_zero)
    assert np.signbit(cam.lleft[axis]) == bool(negative_zero) and not np.signbit(cam.origin[axis])
    assert cam.origin[axis] == cam.lleft[axis] == cam.horizontal[axis] == cam.vertical[axis] == 0.0 and cam.lensRadius == 0.0
    p = abi.default_render_params(W, H, SPP, BOUNCES, seed=9)
    visits = {}
    for touch in (0, 1):
        sb = P.mirror_scene(abi, axis, touch)
        osc = oracle.OracleScene(sb)
        rays, off, neg, lengths = _census(osc, cam, p, axis)
        print("axis %d, negative zero %d, touch %d: %d rays, %d with -0.0, mean path length %.2f" % (axis, negative_zero, touch, rays, neg, lengths.mean()))
        assert rays > 700 and off == 0
        assert neg >= 0.25 * rays if negative_zero else neg == 0
        assert lengths.mean() >= 1.8
        acc, _, st = osc.render(cam, p, oracle.RNG_COUNTER, threads=8, want_rgba=False)
        assert not np.isnan(acc).any()
        assert (acc[..., :3] > 0).any(axis=-1).mean() >= 0.9
        assert st["shadedTriHits"] > 0 and st["sphereTests"] > 0 and st["texelFetches"] == 0
        visits[touch] = st["nodeVisits"]
        nodes = osc.bvh(0)[0]
        leaf = nodes["left"] < 0
        at_zero = (nodes["bmin"][:, axis] == 0) | (nodes["bmax"][:, axis] == 0)
        if touch:
            assert (at_zero & leaf).any() and (at_zero & ~leaf).any()
        else:
            assert not at_zero.any()
    assert visits[0] != visits[1]


@pytest.mark.parametrize("axis,negative_zero", P.CONFIGS, ids=IDS)
def test_miss_scene_counts_tell_the_gate_forms_apart(oracle, abi, dev, axis, negative_zero):
    sb = P.miss_scene(abi, axis)
    osc = oracle.OracleScene(sb)
    cam = P.camera(abi, axis, negative_zero)
    p = abi.default_render_params(W, H, 2, BOUNCES, seed=9)
    acc, _, st = osc.render(cam, p, oracle.RNG_COUNTER, threads=8, want_rgba=False)
    assert st["rays"] == st["samples"] == W * H * 2 and st["shadedTriHits"] == 0 and st["triTests"] > 0
    assert not np.isnan(acc).any() and (acc[..., :3] > 0).all()
    rays, lengths = P.camera_rays(oracle, abi, osc, cam, p)
    assert (lengths == 1).all() and (rays["d"][:, axis] == 0).all() and (rays["o"][:, axis] == 0).all()
    assert np.signbit(rays["d"][:, axis]).any() == bool(negative_zero)
    ref = _flat(osc.bvh(0)[0])
    rc, rg = _regroup(dev, ref, [0])
    assert rc == 1
    # the boxes the scene is for: leaves that straddle 0, leaves whose padded minimum is fl(1e-4f - 1e-4f) == 0, gates with a plane at 0
    leaves = _walk(rg, 0)[1]
    lo, hi = rg[leaves][:, axis], rg[leaves][:, 4 + axis]
    assert ((lo < 0) & (hi > 0)).any() and (lo == 0).any()
    inner = rg.view(np.int32)[:, 3] >= 0
    assert ((rg[inner][:, axis] == 0) | (rg[inner][:, 4 + axis] == 0)).any()
    # the replay is the oracle's walk ...
    v_ref, e_ref = P.gate_replay(ref, rays)["reference"]
    assert int(v_ref.sum()) == st["nodeVisits"]
    # ... and on the regrouped array the three gate forms give three totals and the reference walk's leaves
    forms = P.gate_replay(rg, rays)
    totals = {k: int(v.sum()) for k, (v, _) in forms.items()}
    print("axis %d, negative zero %d: node visits, reference tree %d; regrouped: %s" % (axis, negative_zero, st["nodeVisits"], totals))
    assert len(set(totals.values())) == 3, totals
    for k, (_, entered) in forms.items():
        assert np.array_equal(entered, e_ref), k
    assert e_ref.any()
