"""Helpers of the walk-sequence tests (csrc/srt_regroup.h srtRegroupWalk; tests/test_regroup_elide_host.py on the CPU,
tests/test_gpu_regroup_elide.py on the device): the hook, the link words restated in Python, the elision rule recomputed in
float64 from the binary array, and the float32 replay of a walk through the sequence.  No test lives here."""
import numpy as np

from test_regroup_host import _half_area, _walk

F = np.float32
DONE = -(1 << 31)


def walk_host(dev, rg, world):
    """srtTestRegroupWalk -> (rc, keep (nodes,) uint8, src (records,), links (records, 2), entry (world,))."""
    rg = np.ascontiguousarray(rg, F)
    world = np.ascontiguousarray(world, np.int32)
    import ctypes as C
    n = len(rg)
    keep, src, links, entry = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros((n, 2), np.int32), np.zeros(len(world), np.int32)
    count = C.c_int32(-1)
    rc = dev.lib.srtTestRegroupWalk(rg.ctypes.data, n, world.ctypes.data, len(world), keep.ctypes.data, src.ctypes.data, links.ctypes.data,
                                    entry.ctypes.data, C.byref(count))
    return rc, keep, src[:max(count.value, 0)].copy(), links[:max(count.value, 0)].copy(), entry


def leaf_word(first, second):
    """srt_wf_links.h srtWfLeafWord, restated."""
    hi = ((second & 0xffff) - 1) & 0xffffffff if second != first else 0x8000
    v = ((hi << 16) | (first & 0xffff)) & 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


def expected_keep(rg, root):
    """The rule of the issue, from the binary array alone, in float64: gate g under its binary parent p with m effective
    children (per binary child one, or that child's own count where the child is an elided gate) is elided when
    area(g) * m > area(p) * (m - 1); bottom-up; the inner root always; leaves never.  Returns {node: keep}, {node: end of
    its subtree}."""
    refs = rg.view(np.int32)
    order, _ = _walk(rg, root)
    parent = {}
    for i in order:
        if refs[i, 3] >= 0:
            parent[int(refs[i, 3]) >> 5] = parent[int(refs[i, 7]) >> 5] = i
    area = _half_area(rg[:, 0:3], rg[:, 4:7])
    assert area.dtype == np.float64
    keep, children, end = {}, {}, {}
    with np.errstate(all="ignore"):
        for i in reversed(order):
            if refs[i, 3] < 0:
                keep[i], children[i], end[i] = True, 1, i + 1
                continue
            l, r = int(refs[i, 3]) >> 5, int(refs[i, 7]) >> 5
            m = children[l] + children[r]
            elide = i == root or bool(area[i] * np.float64(m) > area[parent[i]] * np.float64(m - 1))
            keep[i], children[i], end[i] = not elide, (m if elide else 1), end[r]
    return keep, end


def check_sequence(rg, world, keep, src, links, entry):
    """Everything the issue lists under "Structure", for every tree of `world` over the binary array `rg`."""
    refs = rg.view(np.int32)
    assert keep.dtype == np.uint8 and set(np.unique(keep)) <= {0, 1}
    assert np.array_equal(src, np.flatnonzero(keep)), "the sequence is not the kept records in array order"
    number = {int(s): j for j, s in enumerate(src)}
    assert links.shape == (len(src), 2) and len(entry) == len(world)
    covered = 0
    for k, wr in enumerate(world):
        wr = int(wr)
        if wr < 0:  # a bare primitive: its root word, as today
            assert int(entry[k]) == leaf_word(wr, wr)
            continue
        root = wr >> 5
        order, leaves = _walk(rg, root)
        assert order == list(range(root, root + len(order)))
        want, end = expected_keep(rg, root)
        for i in order:
            assert bool(keep[i]) == want[i], (i, "leaf" if refs[i, 3] < 0 else "gate", bool(keep[i]))
        assert all(keep[i] for i in leaves), "a leaf was elided"
        assert len(order) == 1 or not keep[root], "an inner root was kept"
        kept = [i for i in order if keep[i]]
        assert [i for i in kept if refs[i, 3] < 0] == leaves, "the leaves, in order"
        assert int(entry[k]) == number[kept[0]] * 32
        # from the entry with every box passing: each kept record of the tree once, in pre-order, then DONE
        cur, met = int(entry[k]), []
        while cur != DONE:
            assert cur >= 0 and cur % 32 == 0 and cur >> 5 < len(src)
            j = cur >> 5
            met.append(int(src[j]))
            hit, miss = int(links[j, 0]), int(links[j, 1])
            cur = hit if hit >= 0 else miss
        assert met == kept
        stop = root + len(order)
        for i in kept:
            j = number[i]
            hit, miss = int(links[j, 0]), int(links[j, 1])
            # the miss link: the first kept record behind the subtree -- it skips exactly the subtree's kept records, that is
            # exactly the gate's leaf range and the kept gates among them -- or DONE behind the tree's last leaf
            behind = [x for x in kept if x >= end[i]]
            assert miss == (number[behind[0]] * 32 if behind else DONE), (i, miss)
            inside = [x for x in kept if i < x < end[i]]
            assert (miss >> 5 if miss != DONE else number[kept[-1]] + 1) == j + 1 + len(inside)
            if refs[i, 3] >= 0:
                assert hit == (j + 1) * 32 and inside and [x for x in inside if refs[x, 3] < 0] == [x for x in leaves if i < x < end[i]]
            else:
                assert hit == leaf_word(int(refs[i, 3]), int(refs[i, 7])) and not inside
        assert end[root] == stop
        covered += len(kept)
    assert covered == len(src), "a record of the sequence belongs to no tree of the world list"


def sequence_walk(rg, src, links, entry_word, passes):
    """The kernel's walk through the sequence for box verdicts `passes` (rays x records of the BINARY array; record j of the
    sequence takes the verdict of its source): node visits per ray, and which leaves a ray enters (rays x kept leaves in
    order).  A gate that passes goes on to the next record, anything else to its miss link."""
    refs = rg.view(np.int32)
    rays = passes.shape[0]
    reach = np.zeros((rays, len(src) + 1), bool)  # (the last column: DONE)
    if entry_word >= 0:
        reach[:, entry_word >> 5] = True
    first = (entry_word >> 5) if entry_word >= 0 else len(src)
    leaf_cols, entered = [], []
    j = first
    last = first
    # the records of this tree: from the entry to the last record a link of it leads to
    while j < len(src) and j <= last:
        s = int(src[j])
        hit, miss = int(links[j, 0]), int(links[j, 1])
        mt = miss >> 5 if miss != DONE else len(src)
        r = reach[:, j]
        ok = r & passes[:, s]
        if refs[s, 3] >= 0:
            assert hit == (j + 1) * 32
            reach[:, j + 1] |= ok
            reach[:, mt] |= r & ~ok
            last = max(last, j + 1)
        else:
            leaf_cols.append(s)
            entered.append(ok)
            reach[:, mt] |= r
        if mt < len(src):
            assert mt > j
            last = max(last, mt)
        j += 1
    visits = reach[:, first:j].sum(axis=1) if j > first else np.zeros(rays, np.int64)
    return visits, (np.stack(entered, axis=1) if entered else np.zeros((rays, 0), bool)), leaf_cols
