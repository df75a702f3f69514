"""The certified triangle test on the device (csrc/srt_tri_hit.h, tunable "tri_cert"): srtTraceRays against the CPU oracle
ray by ray on rays aimed at edges, vertices and the other hard classes of tests/tri_cert_cases.py, with the certificate on
and off; whole frames of every FAITHFUL kernel form with it on against off, bit for bit; and the triFast table after
srtUpdateTriangles + srtRefitScene against the host's records and a fresh upload."""
import numpy as np
import pytest

import refit_ref as RF
import tri_cert_cases as TC
from conftest import render_counted
from test_gpu_refit import _prebuilt

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "rays", "nodeVisits", "boxPasses", "triTests", "sphereTests", "shadedTriHits", "texelFetches")
PER_CLASS = 300  # x 7 classes: about 2 000 rays per scene
SCENES = {"sheet": TC.sheet, "one_triangle": TC.one_triangle, "uncertified": TC.with_uncertified}


@pytest.fixture
def tri_cert(ctx):
    """Sets the tunable for the test body; the default comes back afterwards."""
    saved = ctx.get_tunable("tri_cert")
    yield lambda v: ctx.set_tunable("tri_cert", v)
    ctx.set_tunable("tri_cert", saved)


@pytest.fixture(scope="module")
def cases(abi, oracle):
    """{scene: (builder, {class: rays}, {class: the oracle's hits})}, made once."""
    out = {}
    for k, (name, make) in enumerate(SCENES.items()):
        sb = make(abi)
        by_class = TC.rays(abi, TC.triangles_of(sb), np.random.default_rng(100 + k), PER_CLASS)
        osc = oracle.OracleScene(sb)
        out[name] = (sb, by_class, {c: osc.trace(r) for c, r in by_class.items()})
    return out


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("on", [1, 0])
def test_trace_is_the_oracles(ctx, cases, tri_cert, scene, on):
    sb, by_class, want = cases[scene]
    tri_cert(on)
    ctx.upload_scene(sb)
    undecided, tests, hits, hits_of = {}, {}, 0, {}
    n_tri = len(TC.triangles_of(sb))
    for c in TC.CLASSES:
        got = ctx.trace(by_class[c])
        undecided[c], tests[c] = ctx.tri_undecided(), int(got["triTests"].sum())
        w = want[c]
        assert np.array_equal(got["prim"], w["prim"]), (scene, c, np.flatnonzero(got["prim"] != w["prim"])[:8].tolist())
        hit = w["prim"] >= 0
        assert np.array_equal(got["t"][hit].view(np.uint32), w["t"][hit].view(np.uint32)), (scene, c)
        assert np.array_equal(got["triTests"], w["triTests"]), (scene, c)
        hits += int(hit.sum())
        hits_of[c] = int((hit & (w["prim"] < n_tri)).sum())  # triangle hits (the scenes list their triangles first)
    assert hits > PER_CLASS  # the rays do meet the geometry
    print(scene, "tri_cert", on, {c: (undecided[c], tests[c]) for c in TC.CLASSES})
    if not on:
        # every test that passes the plane conditions takes the exact code: at least the one behind every triangle hit
        assert all(undecided[c] >= hits_of[c] for c in TC.CLASSES) and sum(hits_of.values()) > 0, (undecided, hits_of)
        return
    for c in TC.EDGE_AIMED:
        assert undecided[c] > 0, (scene, c, undecided)
    if scene == "uncertified":
        # every test of a triangle the record cannot certify that passes the plane conditions is undecided: the random rays
        # aimed at those two triangles reach the exact test (the 10^-3 bound is the certified triangles')
        assert undecided["random"] > 0
    else:
        assert undecided["random"] < 1e-3 * tests["random"], (undecided["random"], tests["random"])


def test_the_uncertified_scene_holds_what_it_says(ctx, abi, dev):
    sb = TC.with_uncertified(abi)
    ctx.upload_scene(sb)
    kappa = ctx.tri_fast_records()[:, 11]
    assert np.isposinf(kappa).tolist() == [False, False, True, True]


def test_frames_with_and_without_the_certificate(ctx, abi, camera, node_path, tri_cert):
    """64 x 64, 4 spp of the sheet in the four kernel forms: accumulator bits, NaN positions and the eight counters.  (The
    instances over the LDS-resident tree run the certified test; the hybrid and the 256-thread instances keep the exact test
    whatever the tunable says, DESIGN 5.0 -- for them this pins that the tunable changes nothing.)"""
    sb = TC.sheet(abi)
    frames = {}
    for on in (1, 0):
        tri_cert(on)
        ctx.upload_scene(sb)
        ctx.set_camera(camera)
        p = abi.default_render_params(64, 64, 4, 6, seed=11)
        p.countStats = 1
        acc, _ = render_counted(ctx, p, node_path)
        info = ctx.launch_info()
        frames[on] = (acc, {k: ctx.stats()[k] for k in COUNTERS}, info["lds_tree_mode"])
    (a1, s1, f1), (a0, s0, f0) = frames[1], frames[0]
    assert f1 == f0
    assert s1["triTests"] > 10_000 and s1 == s0, (s1, s0)
    assert np.array_equal(np.isnan(a1), np.isnan(a0))
    assert np.array_equal(a1.view(np.uint32), a0.view(np.uint32))


def test_refit_rewrites_the_records(ctx, abi, dev, tri_cert):
    """srtUpdateTriangles + srtRefitScene: the triFast table read back is the host's record of every triangle, and a trace
    equals the one of a fresh upload of the moved scene with the refitted tree."""
    tri_cert(1)
    sb = TC.sheet(abi)
    ctx.upload_scene(sb)
    nodes = ctx.bvh(0)
    tri = RF.scene_triangles(sb)
    rng = np.random.default_rng(9)
    moved_ids = [3, 4, 5, 150, 151, 311]
    for i in moved_ids:
        tri["p"][i] += rng.normal(0, 0.2, (3, 3)).astype(np.float32)
    ctx.update_triangles(3, tri[3:6])
    ctx.update_triangles(150, tri[150:152])
    ctx.update_triangles(311, tri[311:])
    ctx.refit()
    got_records = ctx.tri_fast_records()
    host = np.array([dev.tri_fast_record(t.reshape(9)) for t in tri["p"]])
    assert np.array_equal(got_records.view(np.uint32), host.view(np.uint32))
    moved = RF.moved_scene(sb, tri)
    by_class = TC.rays(abi, tri["p"][moved_ids + [0, 100, 200]], np.random.default_rng(10), 150)
    rays = np.concatenate([by_class[c] for c in TC.CLASSES])
    got = ctx.trace(rays)
    it = sb.world[0]
    ctx.upload_scene(_prebuilt(abi, moved, RF.refit(moved, nodes, it.time0, it.time1)))
    assert np.array_equal(ctx.tri_fast_records().view(np.uint32), host.view(np.uint32))
    want = ctx.trace(rays)
    assert (want["prim"] >= 0).sum() > 100
    assert got.tobytes() == want.tobytes()
