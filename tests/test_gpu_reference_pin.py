"""GPU tests against the REFERENCE's recorded results: tests/golden/ref_<scene>.npz holds what the reference's own headers
gave (oracle/ref_harness.cpp, written by tests/make_golden.py) for the edge set of tests/ref_cases.py and every second ray
of trace_<scene>.npz -- hit records, the four counters, the brute-force closest hit -- and its tree in pre-order.  The
fixture takes the live oracle's place; the field rule is test_gpu_parity.py's assert_hits_equal / assert_counters_equal,
unchanged.  Nothing here reads anything but tests/golden/, and nothing renders a frame.

The edge set holds rays whose reference record carries NaNs (a NaN origin component or a zero direction makes every
comparison of sphere::hit false, so it "hits" with t = NaN).  A NaN's own bits are the platform's, so on those records
the float fields are compared by NaN position and bit for bit wherever the reference's value is a number; the integer
fields and the counters are compared exactly as on every other record."""
import os

import numpy as np
import pytest

import ref_cases
from conftest import GOLD
from test_gpu_parity import _bits, assert_counters_equal, assert_hits_equal

pytestmark = pytest.mark.gpu

FIXTURES = ("spheres", "iron", "masterchief", "edges")
FLOAT_FIELDS = ("t", "p", "normal", "tangent", "bitangent")


def _scene(srt, abi, name):
    return ref_cases.edge_scene(abi) if name == "edges" else srt.scenes.SCENES[name]()


@pytest.fixture(scope="module")
def fixtures():
    return {n: np.load(os.path.join(GOLD, "ref_%s.npz" % n)) for n in FIXTURES}


def _nan_records(want):
    """Records that hit and hold a NaN in a field assert_hits_equal compares on bits."""
    return (want["prim"] >= 0) & np.any([np.isnan(want[f]).reshape(len(want), -1).any(axis=1) for f in FLOAT_FIELDS], axis=0)


def assert_matches_reference(got, want, names):
    nan = _nan_records(want)
    assert_hits_equal(got[~nan], want[~nan])
    assert_counters_equal(got, want)
    for f in ("prim", "frontFace", "material"):
        assert np.array_equal(got[f][nan], want[f][nan]), f
    for f in FLOAT_FIELDS + ("uv",):
        a, b = got[f][nan], want[f][nan]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (f, "NaN pattern")
        if f != "uv":  # uv of the records without NaN went through assert_hits_equal's tolerance; here only its pattern
            number = ~np.isnan(b)
            assert np.array_equal(_bits(a)[number], _bits(b)[number]), f
    assert len(names) and nan.sum() < len(names)  # the records with NaNs all come from the edge set


@pytest.mark.parametrize("name", FIXTURES)
def test_trace_against_recorded_reference(ctx, srt, abi, fixtures, name, node_path):
    """srtTraceRays in the reference's traversal order over the fixture's rays (the fixed set and the whole edge set),
    with the scene uploaded under each of the four node_path forms."""
    g = fixtures[name]
    ctx.upload_scene(_scene(srt, abi, name))
    got = ctx.trace(g["rays"])
    assert_matches_reference(got, g["hits"], [str(n) for n in g["names"]])


def closest_mode_defined(g):
    """The rays of a fixture on which the closest-hit mode has one answer, told from the rays and the recorded results of
    the reference alone:
      * origin and direction are numbers and the direction is not zero (otherwise sphere::hit and triangle::hit "hit" at
        t = NaN, which the acceptance `t <= closest` drops and a traversal may keep);
      * one nearest primitive (where two hit at exactly the same t -- a shared edge or vertex -- the winner is the
        traversal order's)."""
    o, d = g["rays"]["o"], g["rays"]["d"]
    return np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1) & (g["closest_ties"] <= 1)


@pytest.mark.parametrize("name", FIXTURES)
def test_closest_mode_against_recorded_reference(ctx, srt, abi, fixtures, name):
    """The closest-hit traversal mode against the closest hit over the reference's tree: its own leaf hits, a node's
    children visited only where its own box test passes (oracle/ref_harness.cpp jobClosest; the reference itself never
    computes a closest hit).  Any traversal order gives that answer, a tie apart.  The brute force over the
    list differs from it where a box does not hold the hit -- exactly at tMax on a box face, a grazing ray with a zero
    direction component, a moving sphere outside its time range: the edge set has all three, and they are counted."""
    g = fixtures[name]
    names = [str(n) for n in g["names"]]
    names += ["fixed ray %d" % i for i in range(len(g["rays"]) - len(names))]
    ctx.upload_scene(_scene(srt, abi, name))
    got = ctx.trace(g["rays"], abi.SRT_TRAVERSE_CLOSEST)
    defined = closest_mode_defined(g)
    assert defined.sum() > 0.9 * len(defined)
    hit = g["closest_prim"] >= 0
    bad = defined & ((got["prim"] != g["closest_prim"]) | (hit & (_bits(got["t"]) != _bits(g["closest_t"]))))
    report = [(names[i], int(got["prim"][i]), float(got["t"][i]), int(g["closest_prim"][i]), float(g["closest_t"][i]))
              for i in np.flatnonzero(bad)]
    print("closest mode, %s: %d of %d rays defined, %d differ; tree and brute force differ on %d" % (
        name, defined.sum(), len(defined), len(report), int((g["closest_prim"] != g["brute_prim"]).sum())))
    assert not report, report[:20]
    assert (g["closest_prim"] != g["brute_prim"]).any()


@pytest.mark.parametrize("name", FIXTURES)
def test_bvh_upload_matches_recorded_reference(ctx, srt, abi, fixtures, name):
    """The uploaded tree is the reference's own, node for node (as test_bvh_upload_matches_oracle holds it against the
    oracle's)."""
    g = fixtures[name]
    ctx.upload_scene(_scene(srt, abi, name))
    assert ctx.bvh(0).tobytes() == g["nodes"].tobytes()
    assert ctx.bvh_depth() == int(g["depth"])
