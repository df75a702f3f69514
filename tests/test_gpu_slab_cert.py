"""The certified slab test (csrc/srt_slab.h) as the device compiles it, pinned to the reference's divisions.

  * refinedRcp (csrc/srt_path.h: v_rcp_f32 and one Newton step) on EVERY float with |d| in [2^-20, 2^20], both signs, through
    srtTestRefinedRcp: |r d - 1| <= 3 * 2^-24, the hypothesis of the header's proof (tests/test_slab_host.py shows on the
    host that the certificate is sound for any reciprocal inside that band).  Measured: just under 1 * 2^-24, first at |d| = 0x1.fffffep-20.
  * pair by pair through srtTestSlabVisit, 2 * 10^4 cases per class of tests/slab_cases.py at tMin = 0.001, 0 and 64: boxHit is
    a NumPy float32 statement of aabb.h:14-22 on every case; a decided verdict of any certified form is that verdict; the
    conservative forms enter wherever the reference's interval is not strictly empty; the three certified forms agree; and
    every device result equals the HOST compile's (the probe's replay mode) on the device's own reciprocals.  Values are
    compared as values: a zero may carry either sign.
  * walks on rays aimed at the tree's own boxes -- corners, edge midpoints, rays lying in face planes -- in a small scene of
    spheres and axis-aligned triangles: srtTraceRays FAITHFUL equals the oracle's walk in hit and in all four counters,
    and the device queries equal the oracle as in tests/test_gpu_query.py (CLOSEST and occlusion: the brute force), over the
    reference tree and a device-built one.
  * the GATE form of the exact test (bit 10: boxHitOrGate with gate = true, what the path-pool kernel calls on an inner node of
    its regrouped tree) on the classes above and on the nested pairs of tests/test_regroup_host.py -- d of +-0,
    +-2^-20, +-inf and NaN, origins on planes, off planes and NaN: it is a NumPy float32 statement of the gate written from
    the design text, it is the host compile's, and boxHit passing on the inner box of a pair implies the gate passing on the
    outer one."""
import os
import subprocess

import numpy as np
import pytest

import slab_cases
from conftest import ROOT
from test_gpu_parity import assert_counters_equal, assert_hits_equal
from test_gpu_query import _assert_key, _query
from test_slab_host import replay_cases

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
N = 20_000
LO, HI = 0x35800000, 0x49800000  # 2^-20, 2^20
SIGN = 0x80000000


@pytest.fixture(scope="module")
def probe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sexy-raytracer_amd", "csrc"), "../../examples/srt_slab_probe"])
    return os.path.join(ROOT, "examples", "srt_slab_probe")


# ------------------------------------------------------------------------------------------------ 1. the reciprocal
def test_refined_rcp_is_inside_the_band_on_every_certified_direction(ctx):
    assert np.array([LO, HI], np.uint32).view(F).tolist() == [2.0 ** -20, 2.0 ** 20]
    count = HI - LO + 1
    assert count == 40 * 2 ** 23 + 1
    worst = []
    for first in (LO, SIGN | LO):
        half = count // 2
        for a, n in ((first, half), (first + half, count - half)):
            e, d = ctx.refined_rcp_test(a, n)
            print("patterns %#x + %d: max |r d - 1| = %.6f * 2^-24 at d = %s" % (a, n, e / U, float(d).hex()))
            assert 2.0 ** -20 <= abs(d) <= 2.0 ** 20
            worst.append(e)
    assert 0.0 < max(worst) <= 3.0 * U, [w / U for w in worst]
    # ... and what ONE Newton step gives.  With eps = 1 - d r0 (|eps| <= 2^-23: v_rcp_f32 is within one ulp), e0 = fl(eps) =
    # eps (1 + d1) and r = fl(r0 + e0 r0) = r0 (1 + eps + eps d1) (1 + d2), |d1|, |d2| <= u:
    #   d r - 1 = d2 + (eps d1 - eps^2) (1 + d2),   so   |d r - 1| <= u + (2^-47 + 2^-46) (1 + u) < (1 + 2^-21) u.
    # The seed alone reaches 1.53 u (measured with the step taken out of a scratch build), which the band above admits.
    assert max(worst) <= (1.0 + 2.0 ** -21) * U, [w / U for w in worst]


def test_refined_rcp_hook_edges_and_uncertified_directions(ctx, dev):
    """The range ends and one pattern either side; a range that reaches an infinity or a NaN, or both signs, is refused.  For
    0, denormals, infinities and NaN the only claim is the certificate's own: such a ray is not certified."""
    for bits in (LO, LO + 1, HI - 1, HI, SIGN | LO, SIGN | HI):
        e, d = ctx.refined_rcp_test(bits, 1)
        assert d.view(np.uint32) == bits and e <= 3.0 * U, (hex(bits), e / U)
    for bits in (LO - 1, HI + 1, 0x00000001, 0x007fffff, 0x7f7fffff):  # outside the certified range: any finite answer
        e, d = ctx.refined_rcp_test(bits, 1)
        assert d.view(np.uint32) == bits and e >= 0.0
    assert ctx.refined_rcp_test(0, 1)[0] == np.inf  # 0 * inf in the Newton step: a NaN, reported as an unbounded error
    import ctypes as C
    out = (C.c_uint64 * 2)()
    for first, n in ((0x7f800000, 1), (0x7fc00000, 1), (0xff800000, 1), (0x7f7fffff, 2), (0x7fffffff, 2), (HI, SIGN), (-1, 2),
                     (0, 0), (2 ** 32, 1)):
        assert dev.lib.srtTestRefinedRcp(ctx.h, first, n, out) != 0, (hex(first), n)
    assert dev.lib.srtTestRefinedRcp(ctx.h, LO, 1, None) != 0 and dev.lib.srtTestRefinedRcp(None, LO, 1, out) != 0
    bad = np.array([0.0, -0.0, 2.0 ** -149, 2.0 ** -127, np.inf, -np.inf, np.nan, 2.0 ** -21, 2.0 ** 21], F)
    ok = np.array([2.0 ** -20, -2.0 ** -20, 2.0 ** 20, -2.0 ** 20], F)
    cases = np.zeros((3 * (len(bad) + len(ok)), 13), F)
    cases[:, 0:3], cases[:, 3:6], cases[:, 6:9], cases[:, 9:12], cases[:, 12] = -1.0, 1.0, (0.25, 0.5, -4.0), 1.0, np.inf
    for k, v in enumerate(np.concatenate([bad, ok])):
        for axis in range(3):
            cases[3 * k + axis, 9 + axis] = v
    flags = ctx.slab_visit_test(cases, 0.001)[:, 5].view(np.int32)
    assert not (flags[:3 * len(bad)] & 1).any() and (flags[:3 * len(bad)] >> 2 & 1).all()
    assert (flags[3 * len(bad):] & 1).all()


# ------------------------------------------------------------------------------------------------ 2. pair by pair
def _same_values(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", slab_cases.CLASSES)
def test_device_compile_pair_by_pair(ctx, probe, tmp_path, name):
    for t_min in slab_cases.T_MINS:
        what = (name, t_min)
        cases = slab_cases.cases(name, N, t_min)
        out = ctx.slab_visit_test(cases, t_min)
        flags = out[:, 5].view(np.int32)
        bit = lambda k: (flags >> k & 1).astype(bool)  # noqa: E731
        entered, t0, t1 = slab_cases.reference(cases, t_min)
        certified = slab_cases.certified(cases)
        # the reference's divisions on the device, on every case
        assert np.array_equal(bit(8), entered), what
        assert np.array_equal(bit(10), slab_cases.gate(cases, t_min)), what  # ... and the gate form's closed interval
        assert np.array_equal(bit(0), certified), what
        assert certified.all() if name != "uncertified" else not certified.any()
        # a decided verdict is the reference's; the three certified forms agree
        for v, u in ((1, 2), (3, 4), (5, 6)):
            decided = ~bit(u)
            assert np.array_equal(bit(v)[decided], entered[decided]), (what, v)
            assert bit(u)[~certified].all() and not bit(v)[~certified].any(), (what, v)
        assert np.array_equal(bit(1), bit(3)) and np.array_equal(bit(1), bit(5)), what
        assert np.array_equal(bit(2), bit(4)) and np.array_equal(bit(2), bit(6)), what
        # the conservative forms lose nothing, ties included
        with np.errstate(invalid="ignore"):
            reachable = ~(t1 < t0)
        assert bit(7)[reachable].all(), what
        assert bit(9)[reachable & ~certified].all(), what
        assert bit(7)[~certified].all(), what
        # the reciprocals are inside the band where the certificate is used
        if name != "uncertified":
            e = np.abs(out[:, 0:3].astype(np.float64) * cases[:, 9:12].astype(np.float64) - 1.0)
            assert e.max() <= 3.0 * U, (what, e.max() / U)
        # the host compile of the same header on the same cases and the device's reciprocals
        host = replay_cases(probe, tmp_path, cases, out[:, 0:3], t_min)
        assert np.array_equal(host[:, 5].view(np.int32) & 0x1ff, flags & 0x1ff), what
        assert np.array_equal(host[:, 5].view(np.int32) >> 10 & 1, flags >> 10 & 1), what
        assert _same_values(host[:, 3], out[:, 3]) and _same_values(host[:, 4], out[:, 4]) and _same_values(out[:, 3], out[:, 4]), what
        assert _same_values(host[certified, 6], out[certified, 6]), what  # (a NaN end, uncertified rays only: v_max keeps the number)
        assert np.isinf(out[~certified, 3]).all(), what
        # a scene without the fast-division word: nothing is decided
        off = ctx.slab_visit_test(cases, t_min, certified_scene=0)
        foff = off[:, 5].view(np.int32)
        assert not (foff & 1).any() and (foff >> 2 & 1).all() and (foff >> 4 & 1).all() and (foff >> 6 & 1).all(), what
        assert not (foff & 0b101010).any() and (foff >> 7 & 1).all() and np.isinf(off[:, 3]).all(), what
        assert np.array_equal(foff >> 8 & 3, flags >> 8 & 3) and _same_values(off[:, 0:3], out[:, 0:3]), what
        assert np.array_equal(foff >> 10, flags >> 10), what
        undecided = bit(2).mean()
        print(name, t_min, "entered %.3f undecided %.3f" % (entered.mean(), undecided))
        if name in ("aimed", "touch"):
            assert undecided > 0.1, what  # the exact path is reached
        if name == "random":
            assert undecided <= 0.01, what
        if name not in ("flat", "uncertified"):
            assert 0.1 <= entered.mean() <= 0.9, what


def test_gate_form_on_the_nested_grid(ctx, probe, tmp_path):
    """slab_cases.gate_grid(): some 2.3 * 10^5 nested pairs of boxes, each box one case of srtTestSlabVisit.  tests/test_slab_host.py
    makes the same comparisons on the host compile alone and shows that the grid reaches both verdicts on the zero axes."""
    inner, outer = slab_cases.gate_grid()
    t = slab_cases.GATE_T_MIN
    got = {}
    for name, cases in (("inner", inner), ("outer", outer)):
        out = ctx.slab_visit_test(cases, t)
        flags = out[:, 5].view(np.int32)
        assert not (flags >> 11).any(), name
        exact, gate = (flags >> 8 & 1).astype(bool), (flags >> 10 & 1).astype(bool)
        assert np.array_equal(exact, slab_cases.reference(cases, t)[0]), name
        assert np.array_equal(gate, slab_cases.gate(cases, t)), name
        host = replay_cases(probe, tmp_path, cases, out[:, 0:3], t)[:, 5].view(np.int32)
        assert np.array_equal(host >> 10 & 1, flags >> 10 & 1) and np.array_equal(host & 0x1ff, flags & 0x1ff), name
        assert not (exact & ~gate).any(), name  # the gate never passes less than the reference's test on the same box
        assert not (flags & 1)[(cases[:, 9:12] == 0).any(axis=1)].any(), name  # a ray with a zero component is never certified
        got[name] = (exact, gate)
    bad = np.flatnonzero(got["inner"][0] & ~got["outer"][1])
    assert len(bad) == 0, (inner[bad[:3]], outer[bad[:3]])
    assert got["inner"][0].sum() > 10000 and (~got["outer"][1]).sum() > 10000
    assert (got["inner"][0] & ~got["outer"][0]).any()  # boxHit itself on the outer box does NOT have the property


def test_slab_visit_hook_refuses(ctx, dev):
    import ctypes as C
    fp = C.POINTER(C.c_float)
    buf = np.zeros((4, 13), F)
    out = np.zeros((4, 8), F)
    a, b = buf.ctypes.data_as(fp), out.ctypes.data_as(fp)
    assert dev.lib.srtTestSlabVisit(ctx.h, a, 0, 0.0, 1, b) != 0
    assert dev.lib.srtTestSlabVisit(ctx.h, a, (1 << 20) + 1, 0.0, 1, b) != 0
    assert dev.lib.srtTestSlabVisit(ctx.h, None, 4, 0.0, 1, b) != 0 and dev.lib.srtTestSlabVisit(ctx.h, a, 4, 0.0, 1, None) != 0
    assert dev.lib.srtTestSlabVisit(None, a, 4, 0.0, 1, b) != 0
    assert not out.any()
    # sizes around a wave and a workgroup: every case answered, nothing beyond
    cases = slab_cases.cases("random", 513, 0.001)
    want = ctx.slab_visit_test(cases, 0.001)
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        pad = np.full((n + 8, 8), 7.0, F)
        assert dev.lib.srtTestSlabVisit(ctx.h, np.ascontiguousarray(cases[:n]).ctypes.data_as(fp), n, 0.001, 1, pad.ctypes.data_as(fp)) == 0
        assert pad[:n].tobytes() == want[:n].tobytes() and (pad[n:] == 7.0).all(), n


# ------------------------------------------------------------------------------------------------ 3. walks on aimed rays
def _scene(abi, builder):
    """96 axis-aligned triangles tiling a rectangle of the plane z = -1.5, 24 in the plane x = 0, 80 spheres around them: one
    tree of 200 primitives; the triangles' boxes have the builder's padding as their only extent on one axis.  (No sphere of
    radius 0: its box is a point, and the brute force's quadratic can accept, by rounding, a ray aimed at that point which
    misses the box by an ulp -- an answer no walk over boxes gives, and no matter of the slab test.)"""
    rng = np.random.default_rng(41)
    sb = abi.SceneBuilder()
    mat = sb.metal((0.7, 0.6, 0.5), 0.1)
    pos = []
    for j in range(6):
        for i in range(8):
            x0, y0, x1, y1, z = 0.5 * i - 2.0, 0.5 * j + 1.0, 0.5 * i - 1.5, 0.5 * j + 1.5, -1.5
            pos += [[x0, y0, z], [x1, y0, z], [x0, y1, z], [x1, y1, z], [x0, y1, z], [x1, y0, z]]
    for j in range(3):
        for i in range(4):
            z0, y0, z1, y1 = 0.5 * i - 1.0, 0.5 * j + 2.0, 0.5 * i - 0.5, 0.5 * j + 2.5
            pos += [[0.0, y0, z0], [0.0, y0, z1], [0.0, y1, z0], [0.0, y1, z1], [0.0, y1, z0], [0.0, y0, z1]]
    pos = np.array(pos, F)
    sb.add_triangles(pos, np.zeros((len(pos), 2), F), np.arange(len(pos), dtype=np.int32).reshape(-1, 3), mat)
    for k in range(80):
        c = (rng.random(3) - 0.5) * 5.0 + np.array([0.0, 2.5, -0.5])
        sb.add_sphere(tuple(float(F(x)) for x in c), float(F(0.1 + 0.3 * rng.random())), mat)
    assert sb.num_prims == 200
    sb.world_bvh(0, None, 0.0, 1.0, builder=builder)
    return sb


def _aimed_rays(abi, nodes, count_cap=24_000):
    """Per node box: rays through its 8 corners and 12 edge midpoints from origins on a shell around the scene, each origin
    component moved by -2 .. 2 ulps; and axis-parallel rays lying in the box's six face planes (two zero direction components:
    uncertified rays, whose visits take the divisions and, in the CLOSEST walk, boxHitLoose).  A ray in a face plane has a
    0 / 0 quotient there; the tiles' edges lie in such planes, and the brute force hits them: boxHitLoose must leave the
    axis open (it used to keep the other plane's infinite quotient for both ends and lost every such hit at an upper face)."""
    rng = np.random.default_rng(43)
    lo, hi = nodes["bmin"].astype(F), nodes["bmax"].astype(F)
    pick = np.array([[(i >> k) & 1 for k in range(3)] for i in range(8)], bool)
    corners = np.where(pick[None], hi[:, None, :], lo[:, None, :])                      # (nodes, 8, 3)
    pairs = [(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count("1") == 1]
    mids = np.stack([(corners[:, a].astype(np.float64) + corners[:, b]) * 0.5 for a, b in pairs], axis=1).astype(F)
    targets = np.concatenate([corners, mids], axis=1).reshape(-1, 3).repeat(3, axis=0)  # 20 per node, three origins each
    centre, radius = np.array([0.0, 2.5, -0.5]), 9.0
    v = rng.normal(size=targets.shape)
    origin = ulps3(centre + radius * v / np.linalg.norm(v, axis=1, keepdims=True), rng)
    d = (targets.astype(np.float64) - origin).astype(F)
    # in the face planes: origin in the plane of one face, direction along one of the other two axes
    n = len(lo)
    face_axis, side, along = rng.integers(0, 3, (n, 6)), rng.integers(0, 2, (n, 6)).astype(bool), rng.integers(1, 3, (n, 6))
    fo = (lo[:, None, :] + (hi - lo)[:, None, :] * rng.random((n, 6, 3)).astype(F)).astype(F)
    rows = np.arange(n)[:, None].repeat(6, 1)
    cols = np.arange(6)[None, :].repeat(n, 0)
    fo[rows, cols, face_axis] = np.where(side, hi[rows, face_axis], lo[rows, face_axis])
    run = (face_axis + along) % 3
    fd = np.zeros((n, 6, 3), F)
    sign = np.where(rng.random((n, 6)) < 0.5, F(-1), F(1))
    fd[rows, cols, run] = sign
    fo[rows, cols, run] = fo[rows, cols, run] - sign * F(12.0)
    o = np.concatenate([origin.astype(F), fo.reshape(-1, 3)])
    d = np.concatenate([d, fd.reshape(-1, 3)])
    keep = rng.permutation(len(o))[:count_cap]
    rays = np.zeros(len(keep), abi.RAY_DTYPE)
    rays["o"], rays["d"] = o[keep], d[keep]
    rays["time"], rays["tMin"], rays["tMax"] = 0.5, 0.001, np.inf
    return rays


def ulps3(p, rng):
    return slab_cases.ulps(p.astype(F), rng.integers(-2, 3, p.shape))


@pytest.fixture(scope="module")
def aimed(ctx, abi, oracle):
    """The scene over the reference tree and over a device-built one, the rays aimed at the reference tree's boxes and at the
    device-built tree's, and the oracle's answers, computed once."""
    out = {}
    for builder in ("REFERENCE", "PLOC"):
        sb = _scene(abi, getattr(abi, "SRT_BUILDER_" + builder))
        ctx.upload_scene(sb)
        assert ctx.slab_scene() == (1, 1)
        nodes = ctx.bvh(0)
        rays = _aimed_rays(abi, nodes)
        assert 12_000 <= len(rays) <= 24_000  # 66 per node; the two trees have 255 and 199 nodes
        osc = oracle.OracleScene(sb)
        out[builder] = (sb, rays, osc.trace(rays, abi.SRT_TRAVERSE_FAITHFUL), osc.trace(rays, abi.SRT_TRAVERSE_CLOSEST))
    return out


def test_faithful_walk_on_aimed_rays_equals_the_oracle_in_hits_and_counters(ctx, abi, aimed):
    """Over the reference tree, which is the oracle's own: world.hit's answer belongs to the order of the walk (rays through
    box corners meet the tiles' shared vertices and edges, where equal t ties), so a device-built tree has no FAITHFUL
    oracle; its CLOSEST answer is no property of the tree and is checked below."""
    sb, rays, want, _ = aimed["REFERENCE"]
    ctx.upload_scene(sb)
    got = ctx.trace(rays, abi.SRT_TRAVERSE_FAITHFUL)
    assert 0.1 <= (want["prim"] >= 0).mean() <= 0.95
    assert want["nodeVisits"].max() > 8 and (want["boxPasses"] > 0).mean() > 0.5
    assert_hits_equal(got, want)
    assert_counters_equal(got, want)  # a wrong decided verdict at an aimed visit changes a counter even when the hit survives


@pytest.mark.parametrize("builder", ["REFERENCE", "PLOC"])
def test_device_queries_on_aimed_rays_equal_the_oracle(ctx, dev, abi, aimed, builder):
    sb, rays, faithful, closest = aimed[builder]
    ctx.upload_scene(sb)
    if builder == "REFERENCE":
        _assert_key(_query(dev, abi, ctx, rays, abi.SRT_TRAVERSE_FAITHFUL)[0], faithful)
    _assert_key(_query(dev, abi, ctx, rays, abi.SRT_TRAVERSE_CLOSEST)[0], closest)  # the brute force over prims[]
    assert np.array_equal(_query(dev, abi, ctx, rays), (closest["prim"] >= 0).astype(np.uint8))
