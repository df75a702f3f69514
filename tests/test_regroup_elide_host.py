"""The regrouped tree's walk sequence on the host, no GPU (csrc/srt_regroup.h srtRegroupWalk, the link words of
csrc/srt_wf_links.h; tunable "wf_regroup" 2): the hook srtTestRegroupWalk, the CPU oracle, and the stand-alone program
examples/regroup_probe.cpp in its mode `walk`.

  * structure, on the masterchief tree, the 301-triangle soup with 41 spheres, a multi-root array with a bare primitive and a
    40-leaf chain: every leaf kept in order, every inner root elided, every other gate kept or elided as the rule says when it
    is recomputed in float64 from the binary array, sources, and links that enumerate each tree's kept records in pre-order
    and skip exactly a gate's leaf range;
  * degenerate inputs: flat boxes (area 0 on both sides of the strict comparison: only roots go), a NaN plane (never elided),
    a single leaf, two leaves;
  * the walk: recorded rays of the masterchief frame, random rays on the soup and the multi-root world, replayed in float32
    with the closed gate form on kept gates -- the leaves entered through the sequence are the reference tree's, at closest =
    +inf and at the oracle's final t, zero tolerance; on masterchief the visits fall below 0.88 x the binary regrouped
    tree's at both (a condition of the change, not a measurement: the replay it was proposed with gave 0.81 and 0.82);
  * the probe's mode under the address and undefined-behaviour sanitizers, as the second stand-alone binary."""
import os

import numpy as np

import regroup_elide as E
from test_regroup_host import (F, _build, _check_structure, _entered, _flat, _intervals, _multi_root, _random_rays, _recorded_rays, _regroup, _run,
                               _soup_scene)


def _chain(m=40):
    """Leaf k a unit box at x = 4^k under a right-leaning chain (test_regroup_host's sanitizer input)."""
    chain = np.zeros((2 * m - 1, 8), F)
    cr = chain.view(np.int32)
    for k in range(m):
        inner, leaf = 2 * k, 2 * k + 1 if k < m - 1 else 2 * k
        chain[leaf, 0:3], chain[leaf, 4:7] = (4.0 ** k, 0, 0), (4.0 ** k + 1, 1, 1)
        cr[leaf, 3] = cr[leaf, 7] = ~(2 * k)
        if k < m - 1:
            cr[inner, 3], cr[inner, 7] = leaf * 32, (inner + 2) * 32
    for i in range(2 * m - 4, -1, -2):
        l, r = cr[i, 3] >> 5, cr[i, 7] >> 5
        chain[i, 0:3], chain[i, 4:7] = np.minimum(chain[l, 0:3], chain[r, 0:3]), np.maximum(chain[l, 4:7], chain[r, 4:7])
    return chain


def _tree_over(lo, hi):
    """A right-leaning chain over the given leaf boxes, inner boxes the unions (single-object leaves, primitive k)."""
    m = len(lo)
    arr = np.zeros((2 * m - 1, 8), F)
    refs = arr.view(np.int32)
    for k in range(m):
        leaf = 2 * k + 1 if k < m - 1 else 2 * k
        arr[leaf, 0:3], arr[leaf, 4:7] = lo[k], hi[k]
        refs[leaf, 3] = refs[leaf, 7] = ~(2 * k)
        if k < m - 1:
            refs[2 * k, 3], refs[2 * k, 7] = leaf * 32, (2 * k + 2) * 32
    for i in range(2 * m - 4, -1, -2):
        l, r = refs[i, 3] >> 5, refs[i, 7] >> 5
        arr[i, 0:3], arr[i, 4:7] = np.minimum(arr[l, 0:3], arr[r, 0:3]), np.maximum(arr[l, 4:7], arr[r, 4:7])
    return arr


def _sequence(dev, rg, world):
    rc, keep, src, links, entry = E.walk_host(dev, rg, world)
    assert rc == 1
    E.check_sequence(rg, world, keep, src, links, entry)
    return keep, src, links, entry


# ------------------------------------------------------------------------------------------------ structure
def test_structure_masterchief(oracle, srt, dev):
    ref = _flat(oracle.OracleScene(srt.scenes.scene_masterchief()).bvh(0)[0])
    rc, rg = _regroup(dev, ref, [0])
    assert rc == 1
    keep, src, _, _ = _sequence(dev, rg, [0])
    gates = rg.view(np.int32)[:, 3] >= 0
    print("masterchief: %d records, %d in the sequence; gates kept %d of %d" % (len(rg), len(src), int(keep[gates].sum()), int(gates.sum())))
    assert 0 < keep[gates].sum() < gates.sum() - 1  # the rule keeps some gates and drops more than the root


def test_structure_soup_and_chain(oracle, srt, abi, dev):
    sb = _soup_scene(srt, abi)
    sb.world_bvh(0, None, 0.0, 1.0)
    ref = _flat(oracle.OracleScene(sb).bvh(0)[0])
    assert int((ref.view(np.int32)[:, 3] < 0).sum()) >= 171  # 301 triangles and 41 spheres in leaves of one or two
    for arr in (ref, _chain()):
        rc, rg = _regroup(dev, arr, [0])
        assert rc == 1
        _check_structure(arr, rg, 0)
        _sequence(dev, rg, [0])
        _sequence(dev, arr, [0])  # (the rule asks nothing of the grouping: the reference's own tree has a sequence too)


def test_structure_multi_root_array(oracle, srt, abi, dev):
    """Two trees in one node array, records no tree reaches between them, and a bare primitive in the world list."""
    sb = _multi_root(srt, abi, lambda s, first=0, count=None: s.world_bvh(first, count, 0.0, 1.0))
    sc = oracle.OracleScene(sb)
    a, b = sc.bvh(0)[0], sc.bvh(2)[0]
    pad = np.full((3, 8), 7.0, F)
    arr = np.concatenate([_flat(a), pad, _flat(b, base=len(a) + 3)])
    world = np.array([0, ~5, (len(a) + 3) * 32], np.int32)
    rc, rg = _regroup(dev, arr, world)
    assert rc == 1
    keep, src, links, entry = _sequence(dev, rg, world)
    assert not keep[len(a):len(a) + 3].any()
    assert entry[1] == E.leaf_word(~5, ~5) and 0 <= entry[0] < entry[2]
    # the first tree's last record ends its walk: no link leads from one tree into the next
    second = int(entry[2]) >> 5
    assert (links[:second][links[:second] >= 0] >> 5 < second).all() and links[second - 1, 1] == E.DONE and links[-1, 1] == E.DONE
    # a node with one node child and one primitive child has no sequence
    bad = rg.copy()
    inner = int(np.flatnonzero(bad.view(np.int32)[:, 3] >= 0)[-1])
    bad.view(np.int32)[inner, 7] = ~0
    assert E.walk_host(dev, bad, world)[0] == 0
    # ... nor has a tree that is not in pre-order (the two children of the root swapped)
    swapped = rg.copy()
    sw = swapped.view(np.int32)
    sw[0, 3], sw[0, 7] = sw[0, 7], sw[0, 3]
    assert E.walk_host(dev, swapped, world)[0] == 0


# ------------------------------------------------------------------------------------------------ degenerate inputs
def test_flat_boxes_elide_roots_only(dev):
    """Every box flat in y and z: area 0 for every gate and every parent, 0 * m > 0 * (m - 1) is false."""
    rng = np.random.default_rng(2)
    m = 9
    lo = np.zeros((m, 3), F)
    lo[:, 0] = rng.random(m).astype(F) * F(10)
    hi = lo.copy()
    hi[:, 0] += F(1)
    arr = _tree_over(lo, hi)
    for rg in (arr, _regroup(dev, arr, [0])[1]):
        keep, src, _, _ = _sequence(dev, rg, [0])
        assert not keep[0] and keep[1:].all() and len(src) == len(rg) - 1


def test_nan_plane_is_never_elided(dev):
    """Four equal leaf boxes: every gate's box is its parent's, so every gate goes.  With a NaN plane in one gate its own
    comparison is false, and so is that of the gate below it (whose parent's area is the NaN): both stay."""
    m = 4
    lo, hi = np.zeros((m, 3), F), np.ones((m, 3), F)
    arr = _tree_over(lo, hi)
    keep, _, _, _ = _sequence(dev, arr, [0])
    gates = arr.view(np.int32)[:, 3] >= 0
    assert not keep[gates].any()
    nan = arr.copy()
    nan[2, 4] = np.nan  # the gate over leaves 1..3
    keep, _, _, _ = _sequence(dev, nan, [0])
    assert keep.tolist() == [0, 1, 1, 1, 1, 1, 1]
    root = arr.copy()
    root[0, 0] = np.nan  # an inner root goes whatever its box
    assert not _sequence(dev, root, [0])[0][0]


def test_single_leaf_and_two_leaves(dev):
    one = _tree_over(np.zeros((1, 3), F), np.ones((1, 3), F))
    keep, src, links, entry = _sequence(dev, one, [0])
    assert keep.tolist() == [1] and src.tolist() == [0] and entry.tolist() == [0]
    assert links.tolist() == [[E.leaf_word(~0, ~0), E.DONE]]
    two = _tree_over(np.array([[0, 0, 0], [5, 0, 0]], F), np.array([[1, 1, 1], [6, 1, 1]], F))
    two.view(np.int32)[2, 7] = ~7  # a leaf of two objects
    keep, src, links, entry = _sequence(dev, two, [0])
    assert keep.tolist() == [0, 1, 1] and src.tolist() == [1, 2] and entry.tolist() == [0]
    assert links.tolist() == [[E.leaf_word(~0, ~0), 32], [E.leaf_word(~2, ~7), E.DONE]]
    # an empty world list, and a world of bare primitives alone
    assert E.walk_host(dev, two, np.zeros(0, np.int32))[0] == 1
    rc, keep, src, _, entry = E.walk_host(dev, two, [~3, ~4])
    assert rc == 1 and not keep.any() and len(src) == 0 and entry.tolist() == [E.leaf_word(~3, ~3), E.leaf_word(~4, ~4)]


# ------------------------------------------------------------------------------------------------ the walk
def _replay(oracle, abi, dev, sb, rays, chunk=500):
    """Mean node visits per ray of (binary regrouped tree, sequence) at closest = +inf and at the oracle's final t."""
    sc = oracle.OracleScene(sb)
    hits = sc.trace(rays)
    t_final = np.where(hits["prim"] >= 0, hits["t"], F(np.inf)).astype(F)
    assert 0.02 < (hits["prim"] >= 0).mean() < 0.999
    visits = np.zeros((2, 2))
    for w, it in enumerate(sb.world):
        if it.kind != abi.SRT_WORLD_BVH:
            continue
        ref = _flat(sc.bvh(w)[0])
        rc, rg = _regroup(dev, ref, [0])
        assert rc == 1
        _, src, links, entry = _sequence(dev, rg, [0])
        for s in range(0, len(rays), chunk):
            r, tf = rays[s:s + chunk], t_final[s:s + chunk]
            a0, b0, _ = _intervals(ref, r, gates=False)
            a1, b1, in1 = _intervals(rg, r, gates=True)
            for k, c in enumerate((np.full(len(r), np.inf, F), tf)):
                _, e0 = _entered(ref, 0, ~(np.fmin(b0, c[:, None]) <= a0))
                passes = in1 & ~(np.fmin(b1, c[:, None]) <= a1)
                v1, e1 = _entered(rg, 0, passes)
                v2, e2, _ = E.sequence_walk(rg, src, links, int(entry[0]), passes)
                assert np.array_equal(e0, e1) and np.array_equal(e0, e2), (w, s, k)
                visits[k] += (v1.sum(), v2.sum())
    visits /= len(rays)
    for k, name in enumerate(("closest = +inf", "the oracle's final t")):
        print("rays %d, node visits per ray at %s: binary regrouped tree %.2f, sequence %.2f (ratio %.3f)"
              % (len(rays), name, visits[k, 0], visits[k, 1], visits[k, 1] / visits[k, 0]))
    return visits


def test_masterchief_recorded_rays(oracle, srt, abi, dev):
    sb = srt.scenes.scene_masterchief()
    sc = oracle.OracleScene(sb)
    visits = _replay(oracle, abi, dev, sb, _recorded_rays(oracle, abi, sc, 2000, 5))
    assert visits[0, 1] < 0.88 * visits[0, 0]
    assert visits[1, 1] < 0.88 * visits[1, 0]


def test_soup_random_rays(oracle, srt, abi, dev):
    sb = _soup_scene(srt, abi)
    sb.world_bvh(0, None, 0.0, 1.0)
    _replay(oracle, abi, dev, sb, _random_rays(abi, 4000, 3))


def test_multi_root_world(oracle, srt, abi, dev):
    sb = _multi_root(srt, abi, lambda s, first=0, count=None: s.world_bvh(first, count, 0.0, 1.0))
    _replay(oracle, abi, dev, sb, _random_rays(abi, 4000, 4))


# ------------------------------------------------------------------------------------------------ the probe, and under sanitizers
def _probe_walk(exe, arr, world, d, env=None):
    world = np.asarray(world, np.int32)
    out = _run(exe, "walk", np.array([len(arr), len(world)], np.int32).tobytes() + np.ascontiguousarray(arr, F).tobytes() + world.tobytes(), d, env)
    assert out[0] == 1
    count, n = int(out[1]), len(arr)
    keep = out[2:2 + n].astype(np.uint8)
    src = out[2 + n:2 + n + count]
    links = out[2 + n + count:2 + n + 3 * count].reshape(-1, 2)
    entry = out[2 + n + 3 * count:]
    assert len(entry) == len(world)
    return keep, src, links, entry


def test_probe_is_the_hook(oracle, srt, abi, dev, tmp_path):
    """The stand-alone program follows the links with srt_wf_links.h's own predicates before it writes; what it writes is
    what the library's hook returns."""
    exe = _build("srt_regroup_probe")
    for arr in (_regroup(dev, _chain(), [0])[1], _tree_over(np.zeros((1, 3), F), np.ones((1, 3), F))):
        got = _probe_walk(exe, arr, [0, ~9], tmp_path)
        want = E.walk_host(dev, arr, [0, ~9])
        for g, w in zip(got, want[1:]):
            assert np.array_equal(g, w)


def test_probe_under_sanitizers(oracle, srt, abi, dev, tmp_path):
    exe = _build("srt_regroup_probe_san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    sb = _soup_scene(srt, abi)
    sb.world_bvh(0, None, 0.0, 1.0)
    ref = _flat(oracle.OracleScene(sb).bvh(0)[0])
    for arr in (ref, _chain()):
        out = _run(exe, "regroup", np.array([len(arr), 1], np.int32).tobytes() + arr.tobytes() + np.int32(0).tobytes(), tmp_path, env)
        assert out[0] == 1
        rg = out[1:].view(F).reshape(-1, 8)
        keep, src, links, entry = _probe_walk(exe, rg, [0], tmp_path, env)
        E.check_sequence(rg, np.array([0], np.int32), keep, src, links, entry)
    # an array the function must refuse, and one whose references point outside it: no read beyond the array
    bad = _chain()
    bad.view(np.int32)[0, 7] = 1 << 20
    out = _run(exe, "walk", np.array([len(bad), 1], np.int32).tobytes() + bad.tobytes() + np.int32(0).tobytes(), tmp_path, env)
    assert out.tolist() == [0]
