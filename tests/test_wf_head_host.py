"""The head of the walk sequence on the host, no GPU (csrc/srt_regroup.h SrtRegroupWalk::head, tunable "wf_head"): the hook
srtTestWfHead over the CPU oracle's trees and hand-made arrays, and the stand-alone program examples/regroup_probe.cpp in
its mode `head`, under the address and undefined-behaviour sanitizers as the second stand-alone binary.

The head word is the leaf word of the sequence's record 0 where the world is ONE tree, that record is a leaf and every
object of it is a sphere; 0 otherwise.  The hook takes the oracle's references (~primitive) and a list of kinds and words
the result over the device's references ~(primitive << 1 | sphere)."""
import os

import numpy as np

import regroup_elide as E
import wf_head_scenes as S
from test_regroup_elide_host import _chain, _tree_over
from test_regroup_host import F, _build, _flat, _regroup, _run


def _oracle_tree(oracle, dev, sb):
    ref = _flat(oracle.OracleScene(sb).bvh(0)[0])
    rc, rg = _regroup(dev, ref, [0])
    assert rc == 1
    return rg


def _first_kept(dev, rg, world=(0,)):
    rc, _, src, links, _ = E.walk_host(dev, rg, world)
    assert rc == 1
    return int(src[0]), int(links[0, 0]), int(links[0, 1])


def test_masterchief(oracle, srt, abi, dev):
    """Primitives 3042 and 3044 of 3 042 triangles and 4 spheres: the ground and one more sphere in the reference's leaf 0,
    box [-1000, -2000, -1000] .. [1000, 2, 1000]; no gate is kept in front of it."""
    sb = srt.scenes.scene_masterchief()
    kinds = S.kinds_of(abi, sb)
    assert len(kinds) == 3046 and kinds[3042:].all() and not kinds[:3042].any()
    rg = _oracle_tree(oracle, dev, sb)
    first, hit, _ = _first_kept(dev, rg)
    refs = rg.view(np.int32)
    assert (int(refs[first, 3]), int(refs[first, 7])) == (~3042, ~3044)
    assert rg[first, 0:3].tolist() == [-1000.0, -2000.0, -1000.0] and rg[first, 4:7].tolist() == [1000.0, 2.0, 1000.0]
    assert hit == E.leaf_word(~3042, ~3044)  # (the sequence itself words the references it is given)
    want = E.leaf_word(S.device_ref(3042, 1), S.device_ref(3044, 1))
    assert S.head_host(dev, rg, [0], kinds) == (1, want) and want != 0
    # both objects: the first reference and the second, as the kernel decodes them (srt_wf_links.h)
    assert ((want & 0xffff) ^ 0x8000) - 0x8000 == S.device_ref(3042, 1)
    assert ((want >> 16) & 0xffff) + 1 - 0x10000 == S.device_ref(3044, 1)


def test_scenes_of_the_device_tests(oracle, abi, dev):
    """What tests/test_gpu_wf_head.py takes for granted of its scenes."""
    for make, want in ((S.ground_alone, lambda: E.leaf_word(S.device_ref(40, 1), S.device_ref(40, 1))),
                       (S.ground_and_moving, lambda: E.leaf_word(S.device_ref(40, 1), S.device_ref(41, 1))),
                       (S.two_spheres, lambda: E.leaf_word(S.device_ref(0, 1), S.device_ref(1, 1))),
                       (S.ground_and_triangle, lambda: 0)):
        sb = make(abi)
        rg = _oracle_tree(oracle, dev, sb)
        rc, head = S.head_host(dev, rg, [0], S.kinds_of(abi, sb))
        assert (rc, head) == (1, want()), (make.__name__, rc, head)
    first, _, miss = _first_kept(dev, _oracle_tree(oracle, dev, S.two_spheres(abi)))
    assert first == 0 and miss == E.DONE
    # the sphere-and-triangle scene: the first kept record IS a leaf, with the ground in it -- only the kinds switch the head off
    sb = S.ground_and_triangle(abi)
    rg = _oracle_tree(oracle, dev, sb)
    first, hit, _ = _first_kept(dev, rg)
    refs = rg.view(np.int32)[first]
    assert hit < 0 and 40 in (~int(refs[3]), ~int(refs[7])) and refs[3] != refs[7]


def test_first_kept_record_is_a_gate(dev):
    """Five unit boxes far apart on x and all spheres: the gates over them cull, so one is kept in front of the first leaf."""
    arr = _regroup(dev, _chain(5), [0])[1]
    _, hit, _ = _first_kept(dev, arr)
    assert hit >= 0
    assert S.head_host(dev, arr, [0], np.ones(16, np.uint8)) == (1, 0)


def _leaf_pair(first, second):
    """Two leaves under a root; the first holds primitives (first, second), the other primitive 5."""
    two = _tree_over(np.array([[0, 0, 0], [5, 0, 0]], F), np.array([[1, 1, 1], [6, 1, 1]], F))
    refs = two.view(np.int32)
    refs[1, 3], refs[1, 7] = ~first, ~second
    refs[2, 3] = refs[2, 7] = ~5
    return two


def test_sphere_and_triangle_in_either_order(dev):
    kinds = np.array([0, 1, 1, 0, 0, 0], np.uint8)
    assert S.head_host(dev, _leaf_pair(1, 3), [0], kinds) == (1, 0)
    assert S.head_host(dev, _leaf_pair(3, 1), [0], kinds) == (1, 0)
    assert S.head_host(dev, _leaf_pair(3, 4), [0], kinds) == (1, 0)
    assert S.head_host(dev, _leaf_pair(1, 2), [0], kinds) == (1, E.leaf_word(S.device_ref(1, 1), S.device_ref(2, 1)))
    assert S.head_host(dev, _leaf_pair(2, 1), [0], kinds) == (1, E.leaf_word(S.device_ref(2, 1), S.device_ref(1, 1)))


def test_one_sphere(dev):
    kinds = np.array([0, 1, 1, 0, 0, 0], np.uint8)
    want = E.leaf_word(S.device_ref(2, 1), S.device_ref(2, 1))
    assert want & 0xffff0000 == 0x80000000  # the single-object word: nothing follows
    assert S.head_host(dev, _leaf_pair(2, 2), [0], kinds) == (1, want)
    assert S.head_host(dev, _leaf_pair(3, 3), [0], kinds) == (1, 0)
    # a tree that is one leaf
    one = _tree_over(np.zeros((1, 3), F), np.ones((1, 3), F))
    one.view(np.int32)[0, 3] = one.view(np.int32)[0, 7] = ~1
    assert S.head_host(dev, one, [0], kinds) == (1, E.leaf_word(S.device_ref(1, 1), S.device_ref(1, 1)))


def test_worlds_without_a_head(dev):
    kinds = np.array([0, 1, 1, 0, 0, 0], np.uint8)
    arr = _leaf_pair(1, 2)
    assert S.head_host(dev, arr, [0], kinds)[1] != 0
    assert S.head_host(dev, arr, [0, ~2], kinds) == (1, 0)  # two items
    assert S.head_host(dev, arr, [~2, 0], kinds) == (1, 0)
    assert S.head_host(dev, arr, [~1], kinds) == (1, 0)     # a bare primitive, a sphere at that
    assert S.head_host(dev, arr, np.zeros(0, np.int32), kinds) == (1, 0)  # an empty world
    # what the walk refuses, and a primitive the kinds do not list
    bad = arr.copy()
    bad.view(np.int32)[0, 7] = ~0
    assert S.head_host(dev, bad, [0], kinds) == (0, 0)
    assert S.head_host(dev, arr, [0], kinds[:5]) == (0, 0)


# ------------------------------------------------------------------------------------------------ the probe, and under sanitizers
def _probe_head(exe, arr, world, kinds, d, env=None):
    world, kinds = np.asarray(world, np.int32), np.asarray(kinds, np.uint8)
    blob = np.array([len(arr), len(world), len(kinds)], np.int32).tobytes() + np.ascontiguousarray(arr, F).tobytes() + world.tobytes() + kinds.tobytes()
    blob += b"\0" * (-len(blob) % 4)
    out = _run(exe, "head", blob, d, env)
    assert len(out) == 2
    return int(out[0]), int(out[1])


def test_probe_is_the_hook(dev, tmp_path):
    exe = _build("srt_regroup_probe")
    kinds = np.array([0, 1, 1, 0, 0, 0], np.uint8)
    for arr, world in ((_leaf_pair(1, 2), [0]), (_leaf_pair(1, 3), [0]), (_leaf_pair(2, 2), [0]), (_leaf_pair(1, 2), [0, ~2])):
        assert _probe_head(exe, arr, world, kinds, tmp_path) == S.head_host(dev, arr, world, kinds)


def test_probe_under_sanitizers(oracle, srt, abi, dev, tmp_path):
    exe = _build("srt_regroup_probe_san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    sb = srt.scenes.scene_masterchief()
    kinds = S.kinds_of(abi, sb)
    rg = _oracle_tree(oracle, dev, sb)
    assert _probe_head(exe, rg, [0], kinds, tmp_path, env) == (1, E.leaf_word(S.device_ref(3042, 1), S.device_ref(3044, 1)))
    # the refused inputs of test_regroup_elide_host.test_probe_under_sanitizers: a reference that points outside the array
    bad = _chain()
    bad.view(np.int32)[0, 7] = 1 << 20
    assert _probe_head(exe, bad, [0], np.ones(80, np.uint8), tmp_path, env) == (0, 0)
    # ... and primitives beyond the kinds, in a leaf and in the world list: no read beyond the list
    assert _probe_head(exe, _chain(), [0], np.ones(3, np.uint8), tmp_path, env) == (0, 0)
    assert _probe_head(exe, _chain(), [~(1 << 20)], np.ones(3, np.uint8), tmp_path, env) == (0, 0)
