"""csrc/srt_records.h on the host, bit for bit: the records and boxes the stand-alone program examples/records_probe.cpp
makes of the edge-case list (tests/records_cases.py) against the NumPy statement of the reference's rules
(tests/records_ref.py), and the boxes also against the leaves srtBuildBvh gives single-primitive world items.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import records_cases as RC
import records_ref as RR
from conftest import ROOT

F = np.float32
OUT_TRI = np.dtype([("test", "<f4", (3, 4)), ("shade", "<f4", (4, 4)), ("mn", "<f4", 3), ("mx", "<f4", 3)])
OUT_SPH = np.dtype([("rec", "<f4", (3, 4)), ("mn", "<f4", 3), ("mx", "<f4", 3)])
TIMES = [(0.0, 1.0), (0.0, 0.0)]  # the item's range; boxCompare's boundingBox(0, 0) (bvh.h:37)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want)).tolist())


@pytest.fixture(scope="module")
def geometry(abi):
    return RC.geometry(abi, tri_material=5, sphere_material=3 | 1 << 30)  # a stale moving bit on every sphere's word


@pytest.fixture(scope="module")
def probe(tmp_path_factory, geometry):
    """{(time0, time1): (triangle outputs, sphere outputs)} from the program."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sexy-raytracer_amd", "csrc"), "../../examples/srt_records_probe"])
    tri, sph = geometry
    d = tmp_path_factory.mktemp("records")
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([len(tri), len(sph)], np.int32).tobytes() + tri.tobytes() + sph.tobytes())
    out = {}
    for k, (t0, t1) in enumerate(TIMES):
        path = str(d / ("out%d.bin" % k))
        subprocess.check_call([os.path.join(ROOT, "examples", "srt_records_probe"), str(d / "in.bin"), path, repr(t0), repr(t1)])
        raw = open(path, "rb").read()
        assert len(raw) == len(tri) * OUT_TRI.itemsize + len(sph) * OUT_SPH.itemsize
        out[(t0, t1)] = (np.frombuffer(raw, OUT_TRI, len(tri)), np.frombuffer(raw, OUT_SPH, len(sph), len(tri) * OUT_TRI.itemsize))
    return out


def test_the_list_holds_its_cases(geometry):
    """The inputs are what their labels say (so that a case cannot quietly stop being one)."""
    tri, sph = geometry
    assert len(tri) == 12 and len(sph) == 4
    sign = lambda x: bool(np.signbit(x))
    assert [sign(v) for v in tri["p"][2, :, 0]] == [False, True, False] and tri["p"][2, :2, 0].tolist() == [0, 0]
    assert [sign(v) for v in tri["p"][3, :, 1]] == [True, False, False] and tri["p"][3, :2, 1].tolist() == [0, 0]
    test, shade = RR.triangle_records(tri)
    assert not test[4, :, 3].any() and not test[5, :, 3].any() and test[0, :, 3].all()         # zero normals
    d0, d1 = tri["uv"][:, 1] - tri["uv"][:, 0], tri["uv"][:, 2] - tri["uv"][:, 0]
    f = d0[:, 0] * d1[:, 1] - d1[:, 0] * d0[:, 1]
    assert f[6] == 0 and f[7] == 0 and f[8] < 0 and f[0] > 0
    assert shade[6, 1, :3].any() and not shade[7, 1, :3].any() and not shade[7, 2, :3].any()
    moving = (sph["center0"] != sph["center1"]).any(axis=1)
    assert moving.tolist() == [False, True, True, False]
    assert _bits(sph["center0"][3]).tolist() != _bits(sph["center1"][3]).tolist()


def test_triangle_records(probe, geometry):
    got = probe[TIMES[0]][0]
    test, shade = RR.triangle_records(geometry[0])
    _same(got["test"], test, "triTest")
    _same(got["shade"], shade, "triShade")
    assert (_bits(got["shade"][:, 3, 3]) == 5).all()  # the caller's material word


def test_triangle_boxes_and_the_zero_rule(probe, geometry):
    got = probe[TIMES[0]][0]
    mn, mx = RR.triangle_boxes(geometry[0])
    _same(got["mn"], mn, "min")
    _same(got["mx"], mx, "max")
    # the first zero seen stays: +0 for {+0, -0, 1}, -0 for {-0, +0, 1}; the maximum of {-1, -0, +0} is -0
    assert _bits(got["mn"][2, 0]) == 0x00000000 and _bits(got["mn"][3, 1]) == 0x80000000
    assert _bits(got["mx"][9, 2]) == 0x80000000
    pad = F(0.0001)
    assert got["mn"][1, 2] == F(0.5) - pad and got["mx"][1, 2] == F(0.5) + pad
    assert got["mn"][10, 2] == -pad and got["mx"][10, 2] == pad                       # +0 == -0: flat
    assert (got["mn"][5] == geometry[0]["p"][5, 0] - pad).all() and (got["mx"][5] == geometry[0]["p"][5, 0] + pad).all()


@pytest.mark.parametrize("times", TIMES)
def test_sphere_records_and_boxes(probe, geometry, times):
    got = probe[times][1]
    sph = geometry[1]
    _same(got["rec"], RR.sphere_records(sph), "records")
    assert ((_bits(got["rec"][:, 1, 3]) >> 30) & 1).tolist() == [0, 1, 1, 0]
    assert (_bits(got["rec"][:, 1, 3]) & ~np.uint32(1 << 30) == 3).all()
    mn, mx = RR.sphere_boxes(sph, *times)
    _same(got["mn"], mn, "min")
    _same(got["mx"], mx, "max")
    if times == (0.0, 0.0):  # one instant: centre -+ radius there; the extrapolated one is off center0
        assert (got["mx"][2] - got["mn"][2] == 2 * sph["radius"][2]).all() and not (got["mn"][1] == sph["center0"][1] - sph["radius"][1]).all()


def test_boxes_are_the_host_builders_leaves(probe, geometry, abi, dev):
    """srtBuildBvh over a single-primitive item: one node, left == right, its box the primitive's over the item's times."""
    tri, sph = geometry
    sb = RC.scene(abi, tri, sph, one_item=False)
    n = len(tri) + len(sph)
    for k, times in enumerate(TIMES):
        got_tri, got_sph = probe[times]
        mn, mx = np.concatenate([got_tri["mn"], got_sph["mn"]]), np.concatenate([got_tri["mx"], got_sph["mx"]])
        for i in range(n):
            nodes, _ = dev.build_bvh_host(sb, item=k * n + i)
            assert len(nodes) == 1 and nodes["left"][0] == nodes["right"][0] == ~i
            _same(nodes["bmin"][0], mn[i], ("min", times, i))
            _same(nodes["bmax"][0], mx[i], ("max", times, i))
