"""srtSortPathsDevice (include/srt_hip.h "Path steps on device buffers"), what a machine without a GPU can check: the two
prototypes against the header, SRT_SORT_MAX_CELL_BITS, the scratch function's promises, the Python wrapper's refusals
that need no device tensor (the others are in tests/test_gpu_sort.py), pathloop's sort= with whole=True, and the tests'
NumPy statement (tests/sort_ref.py) against cases worked by hand."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

import torch

import abi_header
from bad_tensors import bad_tensors
import sort_ref as SR


def test_prototypes_match_the_header(dev, abi):
    decls = abi_header.declarations("srt_hip.h")
    assert decls["srtSortPathsScratchBytes"] == ("int64_t", ["int64_t"])
    assert decls["srtSortPathsDevice"] == ("int", ["SrtContext*", "int64_t", "int32_t"] + ["const void*"] * 6 + ["void*"] * 6 +
                                           ["int64_t", "void*"])
    assert len(abi_header.assert_prototype(dev, abi, "srtSortPathsScratchBytes")) == 1
    assert len(abi_header.assert_prototype(dev, abi, "srtSortPathsDevice")) == 17
    assert dev.lib.srtSortPathsScratchBytes.restype is C.c_int64
    assert dev.lib.srtSortPathsDevice.restype is C.c_int


def test_entries_belong_to_the_drop_in_boundary(dev):
    for name in ("srtSortPathsScratchBytes", "srtSortPathsDevice"):
        assert name in dev.EXPORTS and name not in dev.TEST_EXPORTS
        assert hasattr(dev.lib, name)
        assert name not in abi_header.declarations("srt_hip_test.h")
    assert callable(getattr(dev.Context, "sort_paths_device", None))
    assert callable(getattr(dev.Context, "sort_scratch_bytes", None))


def test_max_cell_bits_constant(abi):
    found = re.findall(r"enum\s*\{\s*SRT_SORT_MAX_CELL_BITS\s*=\s*(\d+)\s*\}\s*;", abi_header.header())
    assert len(found) == 1
    assert int(found[0]) == abi.SRT_SORT_MAX_CELL_BITS == SR.MAX_CELL_BITS == 9
    assert 3 * SR.MAX_CELL_BITS + 4 <= 32  # the key and the dropped entries' bit fit a 32-bit word


def test_scratch_bytes_is_zero_for_nothing_and_never_decreases(dev):
    f = dev.lib.srtSortPathsScratchBytes
    for n in (0, -1, -1024, -2 ** 40):
        assert f(n) == 0
    sizes = [1, 63, 64, 65, 1023, 1024, 1025, 2 ** 20, 2 ** 31 - 1]
    values = [f(n) for n in sizes]
    assert values == sorted(values) and values[0] > 0
    # key and index of every entry, twice
    assert all(v >= 16 * n for v, n in zip(values, sizes))
    dense = [f(n) for n in range(0, 5000, 7)]
    assert dense == sorted(dense)
    assert dev.Context.sort_scratch_bytes(1025) == f(1025) and dev.Context.sort_scratch_bytes(0) == 0


def test_wrapper_refuses_before_the_c_call(dev, abi):
    """A context that was never created has no handle: reaching the C call would fail otherwise than by ValueError."""
    c = object.__new__(dev.Context)
    rays = torch.zeros((8, 9), dtype=torch.float32)
    for bits in (0, -1, abi.SRT_SORT_MAX_CELL_BITS + 1, 32):
        with pytest.raises(ValueError, match="cell_bits"):
            c.sort_paths_device(bits, rays=rays)
    with pytest.raises(ValueError, match="rays must not be None"):
        c.sort_paths_device(5, active=torch.ones((8,), dtype=torch.uint8))
    with pytest.raises(ValueError, match="rng_out without rng"):
        c.sort_paths_device(5, rays=rays, rng_out=torch.zeros((8,), dtype=torch.int64))
    with pytest.raises(ValueError, match="torch stream or a box"):
        c.sort_paths_device(5, rays=rays, stream=12345)
    for what, bad in bad_tensors(rays, 9).items():  # each refusal names its own reason
        with pytest.raises(ValueError, match="rays.*" + what.strip()):
            c.sort_paths_device(5, rays=bad)


def test_pathloop_refuses_sort_with_whole(srt):
    pathloop = importlib.import_module("sexy-raytracer_amd.pathloop")
    with pytest.raises(ValueError, match="sort does not apply"):
        pathloop.sample_radiance(None, None, None, 4, (0, 0, 0), whole=True, sort=5)
    with pytest.raises(ValueError, match="sort does not apply"):
        pathloop.render(None, None, whole=True, sort=5)


# ------------------------------------------------------------------------------------------------ the reference by hand
UNIT = np.array([0, 0, 0, 1, 1, 1], np.float32)


def _rays(origins, directions=None):
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    r = np.zeros((len(o), 9), np.float32)
    r[:, 0:3] = o
    r[:, 3:6] = 1.0 if directions is None else np.asarray(directions, np.float32).reshape(-1, 3)
    return r


def _cell(origin, box=UNIT, bits=1):
    return int(SR.keys(_rays(origin), box, bits)[0]) >> 3


def test_unit_cells_and_the_far_corner():
    assert [_cell(o) for o in ((0.75, 0.25, 0.25), (0.25, 0.75, 0.25), (0.25, 0.25, 0.75))] == [1, 2, 4]
    assert _cell((0.25, 0.25, 0.25)) == 0 and _cell((0.75, 0.75, 0.75)) == 7
    # x, y, z interleave from bit 0 upwards: cell (1, 0, 0) at two bits is 1, cell (2, 0, 0) is 8, (0, 2, 0) is 16
    assert _cell((0.3, 0.1, 0.1), bits=2) == 1 and _cell((0.6, 0.1, 0.1), bits=2) == 8 and _cell((0.1, 0.6, 0.1), bits=2) == 16
    assert _cell((0.999, 0.999, 0.999), bits=9) == 2 ** 27 - 1
    assert _cell((0.999, 0.0, 0.0), bits=9) == int("001" * 9, 2)
    assert SR.spread3(np.array([0b101, 511], np.uint32)).tolist() == [0b1000001, int("001" * 9, 2)]
    q = np.arange(1024, dtype=np.uint32)
    assert SR.spread3(q).tolist() == [sum(((int(v) >> k) & 1) << 3 * k for k in range(10)) for v in q]


def test_octant_is_the_sign_bit():
    d = [(1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, -1), (-0.0, 0.0, 0.0), (0.0, -0.0, 0.0), (0.0, 0.0, -0.0),
         (-np.inf, np.inf, 0.0)]
    key = SR.keys(_rays([(0.05, 0.05, 0.05)] * len(d), d), UNIT, 3)
    assert key.tolist() == [0, 1, 2, 4, 7, 1, 2, 4, 1]
    nan = _rays([(0.05, 0.05, 0.05)] * 2).view(np.uint32)
    nan[0, 3], nan[1, 3] = 0x7fc00000, 0xffc00000  # a NaN has the sign its bit says
    assert SR.keys(nan, UNIT, 3).tolist() == [0, 1]


def test_edges_of_the_box():
    box = np.array([1, 1, 1, 3, 3, 3], np.float32)
    last = 2 ** 5 - 1
    q = lambda x: int(SR.cells(np.array([x], np.float32), 1, 3, 5)[0])  # noqa: E731
    assert q(1.0) == 0 and q(3.0) == last and q(0.5) == 0 and q(-7.0) == 0 and q(3.5) == last and q(1e30) == last
    assert q(np.nextafter(np.float32(3), np.float32(0))) == last and q(2.0) == 16 and q(1.0625) == 1
    assert q(np.nan) == 0 and q(np.inf) == last and q(-np.inf) == 0
    assert _cell((3, 3, 3), box, 5) == 2 ** 15 - 1 and _cell((1, 1, 1), box, 5) == 0
    # hi == lo on an axis: s is infinite; c is NaN on lo, +inf above, -inf below
    flat = lambda x: int(SR.cells(np.array([x], np.float32), 2, 2, 4)[0])  # noqa: E731
    assert flat(2.0) == 0 and flat(2.5) == 15 and flat(1.5) == 0 and flat(np.nan) == 0
    # an inverted box: s is negative, so what lies "inside" counts from hi down and what lies above lo is cell 0
    inv = lambda x: int(SR.cells(np.array([x], np.float32), 3, 1, 4)[0])  # noqa: E731
    assert inv(3.0) == 0 and inv(2.0) == 8 and inv(1.0) == 15 and inv(0.0) == 15 and inv(4.0) == 0
    # a box that is not finite
    assert int(SR.cells(np.array([5.0], np.float32), -np.inf, np.inf, 4)[0]) == 0  # s = 0, c = inf * 0 = NaN
    assert int(SR.cells(np.array([5.0], np.float32), np.nan, 1.0, 4)[0]) == 0
    empty = SR.origin_box(_rays([(1, 2, 3)]), np.array([False]))
    assert empty.tolist() == [np.inf] * 3 + [-np.inf] * 3 and _cell((1, 2, 3), empty, 9) == 0


def test_dead_key_lies_above_every_live_key():
    corner = _rays([(2, 2, 2)], [(-1, -1, -1)])
    for bits in range(1, SR.MAX_CELL_BITS + 1):
        live = int(SR.keys(corner, UNIT, bits)[0])
        assert live == 2 ** (3 * bits + 3) - 1  # the last cell, the last octant: the largest live key
        assert SR.dead_key(bits) == live + 1 and SR.dead_key(bits) < 2 ** (3 * bits + 4) <= 2 ** 31
        assert int(SR.keys(corner, UNIT, bits, np.array([False]))[0]) == SR.dead_key(bits)
    with pytest.raises(AssertionError):
        SR.keys(corner, UNIT, 0)
    with pytest.raises(AssertionError):
        SR.keys(corner, UNIT, 10)


def test_sort_on_a_hand_worked_case():
    S, M = 2, 0
    #          cell 7 oct 0   cell 0 oct 1     cell 7 oct 0   cell 0 oct 0    dropped       cell 0 oct 1
    origins = [(.9, .9, .9), (.1, .1, .1), (.8, .8, .8), (.2, .2, .2), (.1, .1, .1), (.3, .3, .3)]
    dirs = [(1, 1, 1), (-1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 1, 1), (-1, 1, 1)]
    rays = _rays(origins, dirs)
    status = np.array([S, S, S, S, M, S], np.int32)
    rng = np.arange(100, 106, dtype=np.int64)
    r = SR.sort(6, 1, UNIT, rays, status=status, rng=rng)
    assert r["key"].tolist() == [56, 1, 56, 0, 64, 1]
    assert r["count"] == 5 and r["index"].tolist() == [3, 1, 5, 0, 2] == r["slot"].tolist()
    assert r["rng"].tolist() == [103, 101, 105, 100, 102] and r["rays"][:, 0].tolist() == [np.float32(x) for x in (.2, .1, .3, .9, .8)]
    assert r["active_out"].tolist() == [1, 1, 1, 1, 1, 0]
    # neither a status nor a mask: everything is kept
    r = SR.sort(6, 1, UNIT, rays, slot=np.arange(50, 56))
    assert r["count"] == 6 and r["slot"].tolist() == [53, 54, 51, 55, 50, 52] and r["slot"].dtype == np.int32
    # one key for all: the identity on the kept entries, which is compaction
    same = _rays([(.1, .1, .1)] * 6)
    import compact_ref as CR
    r, c = SR.sort(6, 9, UNIT, same, status=status, rng=rng), CR.compact(6, status=status, rays=same, rng=rng)
    assert r["index"].tolist() == c["index"].tolist() == [0, 1, 2, 3, 5] and r["rng"].tolist() == c["rng"].tolist()
    # two sorts compose through the slots
    first = SR.sort(6, 1, UNIT, rays, status=status)
    second = SR.sort(5, 1, UNIT, first["rays"], active=np.array([1, 0, 1, 1, 0], np.uint8), slot=first["slot"])
    assert second["slot"].tolist() == [3, 5, 0]
    assert SR.sort(0, 1, UNIT, np.zeros((0, 9), np.float32))["count"] == 0
