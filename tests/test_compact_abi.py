"""srtCompactPathsDevice (include/srt_hip.h "Path steps on device buffers"), what a machine without a GPU can check: the
two prototypes against the header, SRT_COMPACT_TILE, the scratch formula, the Python wrapper's refusal of a tensor the C
entry must never see, and the tests' NumPy statement (tests/compact_ref.py) against cases worked by hand."""
import ctypes as C
import re

import numpy as np
import pytest

import torch

import abi_header
from bad_tensors import bad_tensors
import compact_ref as CR


def test_prototypes_match_the_header(dev, abi):
    decls = abi_header.declarations("srt_hip.h")
    assert decls["srtCompactPathsScratchBytes"] == ("int64_t", ["int64_t"])
    assert decls["srtCompactPathsDevice"] == ("int", ["SrtContext*", "int64_t"] + ["const void*"] * 5 + ["void*"] * 7)
    assert len(abi_header.assert_prototype(dev, abi, "srtCompactPathsScratchBytes")) == 1
    assert len(abi_header.assert_prototype(dev, abi, "srtCompactPathsDevice")) == 14
    assert dev.lib.srtCompactPathsScratchBytes.restype is C.c_int64
    assert dev.lib.srtCompactPathsDevice.restype is C.c_int


def test_entries_belong_to_the_drop_in_boundary(dev):
    for name in ("srtCompactPathsScratchBytes", "srtCompactPathsDevice"):
        assert name in dev.EXPORTS and name not in dev.TEST_EXPORTS
        assert hasattr(dev.lib, name)
        assert name not in abi_header.declarations("srt_hip_test.h")
    assert callable(getattr(dev.Context, "compact_paths_device", None))
    assert callable(getattr(dev.Context, "compact_scratch_bytes", None))


def _tile():
    found = re.findall(r"enum\s*\{\s*SRT_COMPACT_TILE\s*=\s*(\d+)\s*\}\s*;", abi_header.header())
    assert len(found) == 1
    return int(found[0])


def test_tile_constant(abi):
    tile = _tile()
    assert tile == abi.SRT_COMPACT_TILE == CR.TILE
    assert tile >= 64 and tile & (tile - 1) == 0  # a power of two, whole waves


def test_scratch_bytes_is_the_documented_formula(dev):
    f = dev.lib.srtCompactPathsScratchBytes
    tile = _tile()
    assert "8 * ceil(n / SRT_COMPACT_TILE)" in abi_header.header()  # the formula the header documents
    for n in (0, -1, -tile, -2 ** 40):
        assert f(n) == 0
    for n in (1, tile - 1, tile, tile + 1, 2 ** 31):
        assert f(n) == CR.scratch_bytes(n, tile) == 8 * ((n + tile - 1) // tile), n
    assert f(1) == f(tile - 1) == f(tile) == 8 and f(tile + 1) == f(2 * tile) == 16  # the tile count alone
    assert f(2 ** 31) == 8 * 2 ** 31 // tile
    values = [f(n) for n in list(range(0, 4 * tile + 2, 37)) + [2 ** 20, 2 ** 31, 2 ** 40]]
    assert values == sorted(values)
    assert dev.Context.compact_scratch_bytes(tile + 1) == 16


def test_wrapper_refuses_a_bad_tensor_before_the_c_call(dev):
    """A context that was never created has no handle: reaching the C call would fail otherwise than by ValueError."""
    c = object.__new__(dev.Context)
    for what, bad in bad_tensors(torch.zeros((8, 9), dtype=torch.float32), 9).items():  # each refusal names its own reason
        with pytest.raises(ValueError, match="rays.*" + what.strip()):
            c.compact_paths_device(rays=bad, active=torch.ones((8,), dtype=torch.uint8))
    for what, bad in bad_tensors(torch.zeros((8, 8), dtype=torch.int32), 8).items():
        with pytest.raises(ValueError, match="out.*" + what.strip()):
            c.compact_paths_device(out=bad)
    with pytest.raises(ValueError, match="active.*on the GPU"):
        c.compact_paths_device(active=torch.ones((8,), dtype=torch.uint8))
    with pytest.raises(ValueError, match="active.*must be"):
        c.compact_paths_device(active=torch.ones((8,), dtype=torch.bool))
    with pytest.raises(ValueError, match="active.*shape"):
        c.compact_paths_device(active=torch.ones((8, 1), dtype=torch.uint8))
    with pytest.raises(ValueError, match="predicate"):
        c.compact_paths_device(rng=torch.zeros((8,), dtype=torch.int64))


def test_reference_on_hand_worked_cases():
    S, M, E, I = CR.SCATTERED, 0, 1, -1
    status = np.array([S, M, S, S, E, I, S, M], np.int32)
    rays = np.arange(8 * 9, dtype=np.uint32).reshape(8, 9)
    rng = np.arange(100, 108, dtype=np.int64)
    r = CR.compact(8, status=status, rays=rays, rng=rng)
    assert r["count"] == 4 and r["index"].tolist() == [0, 2, 3, 6] == r["slot"].tolist()
    assert r["rays"][:, 0].tolist() == [0, 18, 27, 54] and r["rng"].tolist() == [100, 102, 103, 106]
    assert r["active_out"].tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
    # the mask takes part: a stale SCATTERED behind a 0 does not survive; any non-zero byte is active
    active = np.array([0, 1, 7, 0, 1, 1, 255, 1], np.uint8)
    r = CR.compact(8, status=status, active=active, slot=np.arange(50, 58))
    assert r["index"].tolist() == [2, 6] and r["slot"].tolist() == [52, 56] and r["slot"].dtype == np.int32
    assert r["rays"] is None and r["rng"] is None and r["active_out"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    # the mask alone
    r = CR.compact(8, active=active)
    assert r["index"].tolist() == [1, 2, 4, 5, 6, 7] and r["count"] == 6
    # nothing and everything
    assert CR.compact(3, status=np.array([M, E, I]))["count"] == 0
    assert CR.compact(0, active=np.zeros(0, np.uint8))["active_out"].tolist() == []
    r = CR.compact(3, status=np.full(3, S))
    assert r["slot"].tolist() == [0, 1, 2] and r["active_out"].tolist() == [1, 1, 1]
    # two compactions compose: the second one's slots name the entries of the first buffer
    first = CR.compact(8, status=status)
    second = CR.compact(first["count"], active=np.array([1, 0, 0, 1], np.uint8), slot=first["slot"])
    assert second["slot"].tolist() == [0, 6]
    with pytest.raises(AssertionError):
        CR.keep(4)
