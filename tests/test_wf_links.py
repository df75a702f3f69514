"""The link words of the path-pool kernel's LDS tree (csrc/srt_wf_links.h, whole-tree form) on the host, no GPU: the
stand-alone program examples/wf_links_probe.cpp builds the thread links as srtUploadScene does, encodes every record as the
kernel's prologue does and decodes it as its walk does.  For every node of the trees below the decoded record must give the
hit target, the miss successor and the leaf's first and second object exactly as the node array (and nodeThread) give
them, and DONE, the leaf words and the primitive references must be pairwise distinct values.

The trees: a random forest; a node index >= 2048 (a byte offset beyond 16 bits); the largest node count the launcher lets
into this form, as one tree and as a two-root world; every leaf shape (one object, two neighbouring triangles, a triangle
with a sphere, in both orders); the last node (successor DONE); the largest primitive references of both arrays and
triangle 0 in both places of a leaf; bare primitives in the world list."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "sexy-raytracer_amd", "csrc")
DONE = -(1 << 31)
# the whole-tree form's admission (srt_scene.cpp flattenScene / srt_plan.cpp planRender): the tree, 64 control words and the
# smallest pool (1024 contexts of 18 bytes) within a CU's 160 KB of LDS
MAX_NODES = (160 * 1024 - 64 * 4 - 18 * 1024) // 32
# srtThreadLinks16 admits 2 * numTriangles < 32766 and 2 * numSpheres + 1 < 32766
MAX_TRIS = MAX_SPHERES = 16382


def tri(i):
    return ~(i << 1)


def sph(i):
    return ~(i << 1 | 1)


def _tree(nodes, n_leaves, leaf_of, rng):
    """Appends a random binary tree of n_leaves leaves in pre-order; leaf_of(k) gives leaf k's (left, right) references."""
    me = len(nodes)
    nodes.append(None)
    if n_leaves == 1:
        nodes[me] = leaf_of()
        return me
    k = int(rng.integers(1, n_leaves))
    left = _tree(nodes, k, leaf_of, rng)
    right = _tree(nodes, n_leaves - k, leaf_of, rng)
    nodes[me] = (left * 32, right * 32)
    return me


def _leaves(shapes):
    """leaf_of() that walks a list of (left, right) pairs, then goes on with single fresh triangles."""
    state = {"k": 0, "next": 100}  # (the listed shapes use triangles below 31 and the last two)

    def leaf_of():
        k = state["k"]
        state["k"] += 1
        if k < len(shapes):
            return shapes[k]
        i = state["next"]
        state["next"] += 1
        return (tri(i), tri(i))
    return leaf_of


EDGE_LEAVES = [
    (tri(5), tri(5)),                                   # a single object
    (sph(7), sph(7)),
    (tri(8), tri(9)),                                   # two neighbouring triangles
    (tri(20), sph(3)), (sph(4), tri(21)),               # a triangle paired with a sphere
    (tri(0), tri(1)), (tri(30), tri(0)), (sph(0), tri(0)),  # triangle 0 (reference -1) first and second
    (tri(MAX_TRIS - 1), sph(MAX_SPHERES - 1)), (sph(MAX_SPHERES - 1), tri(MAX_TRIS - 1)),  # the largest references
    (tri(MAX_TRIS - 2), tri(MAX_TRIS - 1)), (sph(MAX_SPHERES - 1), sph(MAX_SPHERES - 1)),
    (sph(10), sph(11)),
]


def _cases():
    rng = np.random.default_rng(11)
    out = {}

    def case(name, tree_leaves, shapes, world_prims=(), ntri=MAX_TRIS, nsph=MAX_SPHERES):
        nodes, world = [], []
        leaf_of = _leaves(shapes)
        for n in tree_leaves:
            world.append(_tree(nodes, n, leaf_of, rng) * 32)
        world.extend(world_prims)
        out[name] = (np.asarray(nodes, np.int32), np.asarray(world, np.int32), ntri, nsph)

    case("one_leaf", [1], [(tri(0), tri(0))])
    case("small", [len(EDGE_LEAVES) + 3], EDGE_LEAVES)
    case("beyond_16_bit_offsets", [1100], EDGE_LEAVES)                       # 2199 nodes: indices >= 2048
    case("largest_one_tree", [MAX_NODES // 2], EDGE_LEAVES)                  # 2 L - 1 = 4535 nodes
    case("largest_two_roots", [MAX_NODES // 2 - 1, 2], EDGE_LEAVES)          # 4533 + 3 = 4536 nodes
    case("two_roots_and_primitives", [4, 3], EDGE_LEAVES[:6], world_prims=(sph(2), tri(0), tri(MAX_TRIS - 1), sph(MAX_SPHERES - 1)))
    assert len(out["beyond_16_bit_offsets"][0]) > 2048 and len(out["largest_two_roots"][0]) == MAX_NODES
    assert len(out["largest_one_tree"][0]) == MAX_NODES - 1
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """{case: (per-node records, per-root records)} from the program."""
    subprocess.check_call(["make", "-C", CSRC, "../../examples/srt_wf_links_probe"])
    d = tmp_path_factory.mktemp("wf_links")
    out = {}
    for name, (refs, world, ntri, nsph) in CASES.items():
        arr = np.zeros((len(refs), 8), np.float32)
        arr[:, 0:3], arr[:, 4:7] = 0.0, 1.0
        arr.view(np.int32)[:, 3], arr.view(np.int32)[:, 7] = refs[:, 0], refs[:, 1]
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([len(refs), len(world), ntri, nsph], np.int32).tobytes() + arr.tobytes() + world.tobytes())
        subprocess.check_call([os.path.join(ROOT, "examples", "srt_wf_links_probe"), str(d / "in.bin"), str(d / "out.bin")])
        raw = np.fromfile(d / "out.bin", np.int32)
        assert raw[0] == 1 and len(raw) == 1 + 8 * len(refs) + 4 * len(world), name
        out[name] = (raw[1:1 + 8 * len(refs)].reshape(-1, 8), raw[1 + 8 * len(refs):].reshape(-1, 4))
    return out


def _successors(refs, world):
    """Node index -> where the walk goes when the node's subtree is done (a node index, or None), from the node array alone."""
    succ = {}
    todo = [(int(w) >> 5, None) for w in world if w >= 0]
    while todo:
        i, after = todo.pop()
        assert i not in succ
        succ[i] = after
        l, r = int(refs[i, 0]), int(refs[i, 1])
        if l >= 0:
            todo.append((r >> 5, after))
            todo.append((l >> 5, r >> 5))
    return succ


@pytest.mark.parametrize("name", sorted(CASES))
def test_decoding_gives_back_the_tree(probe, name):
    refs, world, _, _ = CASES[name]
    rec, roots = probe[name]
    succ = _successors(refs, world)
    assert sorted(succ) == list(range(len(refs)))
    shapes = set()
    for i in range(len(refs)):
        thread, hit, miss, first, has2, second, has3, _ = (int(x) for x in rec[i])
        l, r = int(refs[i, 0]), int(refs[i, 1])
        # the miss successor: the node array's, and nodeThread's high half
        want = succ[i] * 32 if succ[i] is not None else DONE
        assert miss == want, (i, miss, want)
        t_after = thread >> 16
        assert miss == (t_after * 32 if t_after >= 0 else DONE) and (t_after >= 0 or t_after == -32768)
        if l >= 0:
            assert hit == l and l == (l >> 5) * 32 and (first, has2, second, has3) == (0, 0, 0, 0)
            continue
        # a leaf: negative, neither DONE nor a node, and the objects as the node array and nodeThread's low half give them
        assert hit < 0 and hit != DONE and (hit & 0xffffffff) > 0x80000000
        assert first == l and has3 == 0
        t_follows = thread & 0xffff
        if r != l:
            assert has2 == 1 and second == r and t_follows == (r & 0xffff)
        else:
            assert has2 == 0 and t_follows == (thread >> 16) & 0xffff
        shapes.add(("one" if r == l else "two") + ":" + "".join("s" if ~x & 1 else "t" for x in ((l,) if r == l else (l, r))))
    last = len(refs) - 1
    assert int(rec[last, 2]) == DONE  # pre-order: the last node ends its world entry's walk
    if len(refs) > 2048:
        assert (rec[2048:, 2] >= 2048 * 32).any() and rec[:, 2].max() >= 1 << 16
    if name != "one_leaf":
        assert {"one:t", "one:s", "two:tt", "two:ts", "two:st"} <= shapes, shapes
    for k, w in enumerate(world):
        word, first, has2, _ = (int(x) for x in roots[k])
        if w >= 0:
            assert word == int(w)
        else:
            assert word < 0 and word != DONE and first == int(w) and has2 == 0


def test_kinds_are_pairwise_distinct(probe):
    """Over every tree above: node offsets are non-negative; DONE, the leaf words (as stored, and as the walk holds them after
    the first object) and the primitive references share no value."""
    leaf_words, prim_refs = set(), set()
    for name, (refs, world, _, _) in CASES.items():
        rec, roots = probe[name]
        for i in range(len(refs)):
            hit, first, has2, second = int(rec[i, 1]), int(rec[i, 3]), int(rec[i, 4]), int(rec[i, 5])
            if refs[i, 0] >= 0:
                assert hit >= 0 and hit < MAX_NODES * 32
                continue
            leaf_words.add(hit)
            prim_refs.add(first)
            if has2:
                prim_refs.add(second)
        for k, w in enumerate(world):
            if w < 0:
                leaf_words.add(int(roots[k, 0]))
                prim_refs.add(int(w))
    # what the walk holds after a two-object leaf's first object: the second object's single-object word.  The probe decodes
    # through it; here it is restated from the layout (high half 0x8000, low half the reference's 16 bits)
    rest = {((0x80000000 | (p & 0xffff)) ^ (1 << 31)) - (1 << 31) for p in prim_refs}
    leaf_words |= rest
    assert tri(0) in prim_refs and tri(MAX_TRIS - 1) in prim_refs and sph(MAX_SPHERES - 1) in prim_refs
    assert all(-32766 <= p <= -1 for p in prim_refs)
    assert all(x < 0 for x in leaf_words)
    assert DONE not in leaf_words and DONE not in prim_refs
    assert not (leaf_words & prim_refs), sorted(leaf_words & prim_refs)[:4]
    # and by the layout, for every admissible pair: a leaf word's high half is 0x8000..0xfffe, a reference's 0xffff
    assert max(x & 0xffffffff for x in leaf_words) >> 16 <= 0xfffe and min(p & 0xffffffff for p in prim_refs) >> 16 == 0xffff


def test_cross_compile_keeps_registers_and_lds_base():
    """srt_wavefront.hip for gfx950 (`make resource-usage`'s line for it): no instance spills vector registers except the
    two profiling ones, which did before; the headline instance stays within 128; and no instance has static LDS -- the
    tree copy starts at LDS offset 0, which is what lets a node's byte offset be its address."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS = (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    kflags = re.search(r"^KFLAGS = (.*)$", mk, re.M).group(1).split()
    r = subprocess.run([hipcc] + flags + kflags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "srt_wavefront.hip"],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    usage, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if m and m.group(1) == "Function Name":
            name = m.group(2)
            usage[name] = {}
        elif m:
            usage[name][m.group(1)] = int(m.group(2))
    wf = {k: v for k, v in usage.items() if "srt_render_wf_kernel" in k}
    assert len(wf) == 14, sorted(wf)
    for k, v in wf.items():
        profiling = re.search(r"ILb[01]ELb1E", k) is not None  # <SINGLE, PROFILE = true, ...>
        assert v["LDS Size [bytes/block]"] == 0, k
        assert v["VGPRs"] <= 128, (k, v)
        if not profiling:
            assert v["VGPRs Spill"] == 0, (k, v)
    head = wf["_Z20srt_render_wf_kernelILb1ELb0ELb0ELb0ELb0EEv10RenderArgs"]
    assert head["VGPRs Spill"] == 0 and head["VGPRs"] <= 128
