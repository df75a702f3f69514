"""Scenes of the head-leaf record tests (csrc/srt_wavefront.hip: the set-up copies the head leaf's sphere records into LDS
control words, the swap step reads them there; tests/test_wf_head_records_host.py on the CPU,
tests/test_gpu_wf_head_records.py on the device).  No test lives here.

The primitive-count recipe is wf_head_scenes.py's: 42 primitives -- a 40-triangle soup, the ground and one low sphere
whose box is the second-lowest on every axis -- put the ground (primitive 40, sphere 0) and that sphere (primitive 41,
sphere 1) into the tree's first leaf, the head.  A MOVING ground (center1 != center0; its box is the union of the boxes at
both times, still the lowest on every axis) exercises the first record's third quad and its flag, a moving low sphere the
second record's; wf_head_scenes.ground_and_moving is the remaining combination."""
import numpy as np

from wf_head_scenes import _materials, _soup

GROUND0, GROUND1 = (0.0, -1000.0, 0.0), (0.3, -1000.4, -0.2)
LOW0, LOW1 = (-4.5, 1.2, -4.5), (-4.5, 2.4, -4.5)


def _scene(abi, seed, ground_moves, low_moves):
    rng = np.random.default_rng(seed)
    sb = abi.SceneBuilder()
    tri, ground, _ = _materials(sb)
    _soup(sb, rng, 40, tri)
    if ground_moves:
        sb.add_sphere(GROUND0, 1000.0, ground, center1=GROUND1, time0=0.0, time1=1.0)
    else:
        sb.add_sphere(GROUND0, 1000.0, ground)
    if low_moves:
        sb.add_sphere(LOW0, 1.1, tri, center1=LOW1, time0=0.0, time1=1.0)
    else:
        sb.add_sphere(LOW0, 1.1, tri)
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


def moving_ground_and_still(abi):
    """The first object of the head leaf moves, the second does not."""
    return _scene(abi, 34, True, False)


def both_moving(abi):
    """Both objects of the head leaf move."""
    return _scene(abi, 35, True, True)


def moving_ground_alone(abi):
    """wf_head_scenes.ground_alone's 48 primitives with a moving ground: a head of one sphere, and that one moves."""
    rng = np.random.default_rng(36)
    sb = abi.SceneBuilder()
    tri, ground, lamp = _materials(sb)
    _soup(sb, rng, 40, tri)
    sb.add_sphere(GROUND0, 1000.0, ground, center1=GROUND1, time0=0.0, time1=1.0)
    for k in range(7):
        p = rng.uniform(-2.5, 2.5, 3) + np.array([0.0, 3.5, 0.0])
        sb.add_sphere(tuple(float(x) for x in p), float(rng.uniform(0.2, 0.5)), lamp if k == 0 else tri)
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


def sphere_records(abi, sb, changes):
    """The scene's spheres as abi.SPHERE_DTYPE records (Context.update_spheres), with `changes` = {index: {field: value}}
    applied over center0, center1, time0, time1, radius."""
    out = np.zeros(len(sb.spheres), abi.SPHERE_DTYPE)
    for i, s in enumerate(sb.spheres):
        v = dict(center0=tuple(s.center0), center1=tuple(s.center1), time0=s.time0, time1=s.time1, radius=s.radius)
        v.update(changes.get(i, {}))
        out[i] = (v["center0"], v["center1"], v["time0"], v["time1"], v["radius"], s.material)
    return out
