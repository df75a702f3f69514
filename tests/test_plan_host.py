"""The planner of the render launches (csrc/srt_plan.cpp over csrc/srt_lds_layout.h) on the host, no GPU: the stand-alone
program examples/plan_probe.cpp runs the library's own functions over rows of plain inputs.

  * AGAINST THE PARENT.  tests/golden/plan_table.json holds what the commit before the planner existed decided for the rows
    of BLOCKS below: form, block, LDS bytes, ring capacity / shift / mul3, single, profile, unit tiles, queue count, chunk
    count, and the pool size and grid of the path-pool forms ("plans": the distinct decisions; a block's rows name theirs by
    index).  It was recorded AT THAT COMMIT by a throwaway host program (not kept): a translation unit that included that
    commit's srt_render.cpp whole, built without a device pass and linked with unresolved symbols ignored, filled an
    SrtContext's scene, tunables and CU count from each row and called its static renderPlan; the work split, the pool and
    the grid were lines 166-200 and 282-290 of its srtRenderTilesImpl copied verbatim (occupancy 1 for the path-pool kernel,
    as there).  The rows were expanded by _rows() of this file.  The planner must reproduce every row exactly.
  * INVARIANTS, derived here and not recorded: the layout's end offset is the planned LDS size; a plan fits SRT_LDS_BYTES
    or is reported as not launchable; the pool never exceeds the rings and its layout never the plan; and the upload's
    limits are the planner's -- the largest tree for which the planner picks the whole-tree path-pool form is the count
    flattenScene builds hybrid records beyond (and regroups up to), the largest resident top the hybrid form takes beside
    2048 contexts is flattenScene's resident cap.
  * the same program under the address and undefined-behaviour sanitizers, as a second stand-alone binary, over the same
    rows."""
import itertools
import json
import os
import subprocess

import pytest

from conftest import GOLD, ROOT

CSRC = os.path.join(ROOT, "sexy-raytracer_amd", "csrc")
TABLE = os.path.join(GOLD, "plan_table.json")

# the probe's input row (examples/plan_probe.cpp) and the part of its output the parent's table holds
FIELDS = ("nodes", "resident", "worlds", "stack_depth", "thread", "hybrid", "cls", "lds_tree", "wavefront", "wf_pool", "wf_profile",
          "unit_tiles", "queues", "cus", "width", "height", "spp", "chunks", "max_bounce", "traversal", "count", "stride", "moments", "list")
RECORDED = ("form", "block", "lds", "ring_cap", "ring_shift", "ring_mul3", "single", "profile", "unit_tiles", "queues", "chunks",
            "pool", "grid")
DERIVED = ("fits_lds", "layout_end", "pool_layout_end")
FAITHFUL, CLOSEST = 0, 1
LDS_BYTES = 160 * 1024
WHOLE_TREE_MAX, HYBRID_RESIDENT_MAX = 4536, 3832  # the limits the issue names; test_limits holds the header to them

DEFAULTS = dict(worlds=1, stack_depth=20, cls=1, lds_tree=1, wavefront=256, wf_pool=2048, wf_profile=0, unit_tiles=-1, queues=-1, cus=256,
                width=1280, height=720, spp=16, chunks=0, max_bounce=8, traversal=FAITHFUL, count=0, stride=1, moments=0, list=-1, rmax=0)


def _around(*thresholds):
    return sorted({t + d for t in thresholds for d in (-1, 0, 1) if t + d >= 1})


def _nodes_beside(per_context):
    """The largest node count that fits beside each ring capacity: 160 KB less the control words and the contexts."""
    return [(LDS_BYTES - 256 - per_context * cap) // 32 for cap in (4096, 3072, 2048, 1536, 1024)]


def _lds_tree_max(max_bounce=None):
    """... of the LDS-resident-tree forms: the tree and 16 queue words, with the attenuation stacks of 1024 lanes or without."""
    att = 0 if max_bounce is None else (3 * max_bounce + 3) * 1024 * 4
    return (LDS_BYTES - 64 - att) // 32


WHOLE_RING_NODES = _around(*_nodes_beside(18))     # 2808, 3384, 3960, 4248, 4536 = the whole-tree limit
HYBRID_RING_NODES = _around(*_nodes_beside(20))    # 2552, 3192, 3832 = the hybrid resident limit, 4152, 4472
# every threshold of the layout arithmetic with a node count on either side; the wavefront tunable's default and the hybrid
# form's single-root limit as well.  (Attenuation stacks of 50 bounces never fit: no threshold.)
NODES = sorted(set(WHOLE_RING_NODES + _around(HYBRID_RESIDENT_MAX, _lds_tree_max(), _lds_tree_max(1), _lds_tree_max(8), 256, 1 << 20)
                   + [1, 2, 6000, 32767, 32768]))
NODES_FEW = [1, 24, 25, 256, 4000, 4536, 4537, 6000, 1 << 20, (1 << 20) + 1]
MODES = ("plain", "count", "moments", "profile")
SIZES = ((16, 16), (17, 33), (64, 64), (250, 130), (640, 360), (1280, 720), (1920, 1080), (4096, 4096))

# name, fixed fields, axes: the rows are the product of the axes, the last one fastest
BLOCKS = (
    ("forms", {}, (("nodes", NODES), ("worlds", (1, 2)), ("mode", MODES), ("wf_pool", (1024, 2048, 4096)), ("max_bounce", (1, 8, 50)))),
    ("forms_resident_max", {"rmax": 24},
     (("nodes", NODES_FEW), ("worlds", (1, 2)), ("mode", MODES), ("wf_pool", (1024, 2048, 4096)), ("max_bounce", (1, 8)))),
    ("tunables", {}, (("nodes", NODES), ("traversal", (FAITHFUL, CLOSEST)), ("lds_tree", (0, 1)), ("wavefront", (0, 1, 4000)),
                      ("mode", ("plain", "count")))),
    ("tunables_resident_max", {"rmax": 24}, (("nodes", NODES_FEW), ("traversal", (FAITHFUL, CLOSEST)), ("lds_tree", (0, 1)),
                                             ("wavefront", (0, 1, 4000)), ("mode", ("plain", "count")))),
    # hybrid records whose resident top stands at each ring's limit (a pure function takes what no upload makes)
    ("hybrid_resident", {"nodes": 10000, "hybrid": 1},
     (("resident", HYBRID_RING_NODES), ("wf_pool", (1024, 2048, 4096)), ("mode", MODES))),
    ("scene_facts", {}, (("nodes", (100, 4000, 6000)), ("thread", (0, 1)), ("cls", (0, 1)), ("rmax", (0, 24)), ("traversal", (FAITHFUL, CLOSEST)))),
    # 3 * 2^j rings only below 2 * 10^9 enqueues per workgroup: 1920 x 1080 at 100 000 spp passes it on 256 CUs, every size on 8
    ("enqueue_bound", {"width": 1920, "height": 1080, "wf_pool": 4096},
     (("nodes", WHOLE_RING_NODES), ("spp", (5000, 100000)), ("cus", (8, 256)), ("list", (-1, 1000)))),
    ("stack_form", {"nodes": 6000, "wavefront": 0},
     (("stack_depth", (1, 3, 4, 5, 30, 60)), ("max_bounce", (1, 8, 16, 50)), ("traversal", (FAITHFUL, CLOSEST)))),
    ("split", {}, (("size", SIZES), ("spp", (1, 16, 5000)), ("chunks", (0, 1, "spp")), ("stride", (1, 8)), ("list", (-1, 1, "half")),
                   ("nodes", (100, 4000, 6000)))),
    ("split_tunables", {"nodes": 4000},
     (("size", SIZES), ("spp", (1, 16, 5000)), ("split", ((-1, -1), (16, -1), (-1, 4))), ("cus", (64, 256, 304)), ("traversal", (FAITHFUL, CLOSEST)))),
)


def _row(case):
    """One probe row from a case: DEFAULTS, the block's fixed fields and its axes' values; the pseudo-fields resolved."""
    d = dict(DEFAULTS, **case)
    if "size" in d:
        d["width"], d["height"] = d.pop("size")
    if "split" in d:
        d["unit_tiles"], d["queues"] = d.pop("split")
    mode = d.pop("mode", "plain")
    d["count"], d["moments"], d["wf_profile"] = int(mode == "count"), int(mode == "moments"), int(mode == "profile")
    tiles = ((d["width"] + 7) // 8) * ((d["height"] + 7) // 8)
    if d["chunks"] == "spp":
        d["chunks"] = d["spp"]
    if d["list"] == "half":
        d["list"] = max(1, tiles // 2)
    d["list"] = min(d["list"], tiles)
    # the scene as srt_scene.cpp flattenScene makes it for this node count and the tunable wf_resident_max: thread links
    # while the references fit 15 bits, hybrid records beyond the whole-tree limit or the tunable's cap
    rmax = d.pop("rmax")
    d.setdefault("thread", int(d["nodes"] < (1 << 15)))
    if "hybrid" not in d:
        cap = min(HYBRID_RESIDENT_MAX, rmax) if rmax > 0 else HYBRID_RESIDENT_MAX
        d["hybrid"] = int(d["nodes"] > (cap if rmax > 0 else WHOLE_TREE_MAX))
        d["resident"] = min(cap, d["nodes"]) if d["hybrid"] else 0
    d.setdefault("resident", 0)
    assert set(d) == set(FIELDS), set(d) ^ set(FIELDS)
    return [int(d[f]) for f in FIELDS]


def _rows(block):
    name, fixed, axes = block
    return [_row(dict(fixed, **dict(zip([a for a, _ in axes], values)))) for values in itertools.product(*[v for _, v in axes])]


def _build(target):
    subprocess.check_call(["make", "-C", CSRC, "../../examples/" + target])
    return os.path.join(ROOT, "examples", target)


def _plan(exe, rows, d, env=None):
    with open(d / "in.txt", "w") as f:
        f.write("".join(" ".join(map(str, r)) + "\n" for r in rows))
    r = subprocess.run([exe, "plan", str(d / "in.txt"), str(d / "out.txt")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-2000:]
    out = [[int(x) for x in line.split()] for line in open(d / "out.txt")]
    assert len(out) == len(rows) and all(len(o) == len(RECORDED) + len(DERIVED) for o in out)
    return out


@pytest.fixture(scope="module")
def probe():
    return _build("srt_plan_probe")


@pytest.fixture(scope="module")
def limits(probe):
    out = {"ring": []}
    for line in subprocess.check_output([probe, "limits"], text=True).splitlines():
        key, *values = line.split()
        if key == "ring":
            out["ring"].append(tuple(map(int, values)))
        else:
            out[key] = int(values[0])
    return out


@pytest.fixture(scope="module")
def planned(probe, tmp_path_factory):
    """{block name: (rows, the probe's output)}: computed once for the tests below."""
    d = tmp_path_factory.mktemp("plan")
    return {b[0]: (rows, _plan(probe, rows, d)) for b in BLOCKS for rows in [_rows(b)]}


def test_limits(limits):
    """The header's constants, as this file's grid and tests/test_wf_rings.py assume them."""
    assert limits["lds_bytes"] == LDS_BYTES
    assert (limits["context_bytes"], limits["context_bytes_hybrid"], limits["ctl_bytes"]) == (18, 20, 256)
    assert (limits["whole_tree_max_nodes"], limits["hybrid_resident_max"]) == (WHOLE_TREE_MAX, HYBRID_RESIDENT_MAX)
    assert [c for c, _, _ in limits["ring"]] == [4096, 3072, 2048, 1536, 1024]
    assert all(cap == (3 if mul3 else 1) << shift for cap, shift, mul3 in limits["ring"])


@pytest.mark.parametrize("block", [b[0] for b in BLOCKS])
def test_plans_are_the_parents(planned, block):
    table = json.load(open(TABLE))
    assert table["fields"] == list(FIELDS) and table["recorded"] == list(RECORDED)
    rows, out = planned[block]
    want = [table["plans"][i] for line in table["blocks"][block] for i in line]  # a line per value of the block's first axis
    assert len(want) == len(rows) > 0
    bad = [(dict(zip(FIELDS, r)), dict(zip(RECORDED, w)), dict(zip(RECORDED, o))) for r, w, o in zip(rows, want, out) if o[:len(RECORDED)] != w]
    assert not bad, (len(bad), bad[:3])


def test_grid_reaches_every_decision(planned):
    """The recorded rows are worth their name: every form, every ring, both sides of fits-LDS, an explicit chunk count that
    does not fit, a clamped default, and a 3 * 2^j ring refused for its enqueue count."""
    out = [dict(zip(RECORDED + DERIVED, o), **dict(zip(("in_" + f for f in FIELDS), r))) for rows, outs in planned.values() for r, o in zip(rows, outs)]
    assert {o["form"] for o in out} == {0, 1, 2, 3, 4}
    for form in (3, 4):
        assert {o["ring_cap"] for o in out if o["form"] == form} == {1024, 1536, 2048, 3072, 4096}
    assert {o["fits_lds"] for o in out} == {0, 1}
    assert any(o["chunks"] == -1 for o in out) and any(o["chunks"] == 127 and o["in_spp"] == 5000 for o in out)
    bound = [o for o in out if o["in_spp"] == 100000 and o["in_cus"] == 8 and o["form"] == 3]
    assert bound and all(o["ring_mul3"] == 0 for o in bound)
    assert any(o["ring_mul3"] == 1 for o in out if o["in_spp"] == 5000 and o["in_cus"] == 256 and o["in_width"] == 1920)
    assert len({(o["unit_tiles"], o["queues"]) for o in out}) > 12


def test_layout_invariants(planned):
    for rows, outs in planned.values():
        for r, o in zip(rows, outs):
            o, i = dict(zip(RECORDED + DERIVED, o)), dict(zip(FIELDS, r))
            assert o["layout_end"] == o["lds"], (i, o)
            assert o["fits_lds"] == int(o["lds"] <= LDS_BYTES), (i, o)
            # only the stack form can fail to fit: every other form is chosen because it does
            assert o["fits_lds"] or o["form"] == 0, (i, o)
            if o["form"] >= 3 and o["chunks"] > 0:
                assert 64 <= o["pool"] <= o["ring_cap"] <= max(1024, i["wf_pool"]), (i, o)
                assert o["pool_layout_end"] <= o["lds"] and 1 <= o["grid"] <= i["cus"], (i, o)
            else:
                assert (o["pool"], o["grid"]) == (0, 0) and (o["form"] >= 3 or o["ring_cap"] == 0), (i, o)


def test_upload_limits_are_the_planners(probe, limits, tmp_path):
    """What flattenScene decides by (srtWfMaxWholeTreeNodes, srtWfMaxResidentNodes beside SRT_WF_HYBRID_POOL contexts) against
    the planner itself, asked node count by node count with every other condition of the form granted."""
    counts = list(range(1, 6001))
    whole = _plan(probe, [_row(dict(nodes=n, hybrid=0, wavefront=1, wf_pool=4096)) for n in counts], tmp_path)
    assert max(n for n, o in zip(counts, whole) if o[0] == 3) == limits["whole_tree_max_nodes"]
    assert all((o[0] == 3) == (n <= limits["whole_tree_max_nodes"]) for n, o in zip(counts, whole))
    hybrid = _plan(probe, [_row(dict(nodes=10000, hybrid=1, resident=n, wf_pool=4096)) for n in counts], tmp_path)
    assert all(o[0] == 4 or n > _nodes_beside(20)[-1] for n, o in zip(counts, hybrid))
    assert max(n for n, o in zip(counts, hybrid) if o[0] == 4 and o[3] >= 2048) == limits["hybrid_resident_max"]


def test_probe_under_sanitizers(tmp_path):
    """The planner and the layout header under -fsanitize=address,undefined: a second stand-alone binary over every row of
    the table, with the plain binary's output."""
    exe = _build("srt_plan_probe_san")
    plain = _build("srt_plan_probe")
    # (a stand-alone binary with the sanitizers' runtime linked in: the environment is inherited, plus their options)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    rows = [r for b in BLOCKS for r in _rows(b)]
    assert _plan(exe, rows, tmp_path, env) == _plan(plain, rows, tmp_path)
