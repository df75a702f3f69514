"""Device ray queries (include/srt_hip.h "Ray queries"), what a machine without a GPU can check: the ctypes prototypes of
srtTraceRaysDevice and srtOccludedDevice against the header, SrtRayHit's layout, and the Python wrappers' refusal of a
tensor the C entry must never see."""
import ctypes as C

import numpy as np
import pytest

import torch

import abi_header

ENTRIES = ("srtTraceRaysDevice", "srtOccludedDevice")


def test_prototypes_match_the_header(dev, abi):
    decls = abi_header.declarations("srt_hip.h")
    for name in ENTRIES:
        assert name in decls
        assert decls[name][0] == "int"
    assert decls["srtTraceRaysDevice"][1] == ["SrtContext*", "const void*", "int64_t", "int32_t", "void*", "void*", "void*"]
    assert decls["srtOccludedDevice"][1] == ["SrtContext*", "const void*", "int64_t", "void*", "void*"]
    assert len(abi_header.assert_prototype(dev, abi, "srtTraceRaysDevice")) == 7
    assert len(abi_header.assert_prototype(dev, abi, "srtOccludedDevice")) == 5
    for name in ENTRIES:
        assert getattr(dev.lib, name).restype is C.c_int


def test_entries_belong_to_the_drop_in_boundary(dev):
    for name in ENTRIES:
        assert name in dev.EXPORTS and name not in dev.TEST_EXPORTS
        assert hasattr(dev.lib, name)
        assert name not in abi_header.declarations("srt_hip_test.h")


def test_ray_hit_layout(abi):
    assert C.sizeof(abi.SrtRayHit) == 16 == abi.RAY_HIT_DTYPE.itemsize
    want = {"prim": (0, C.c_int32), "t": (4, C.c_float), "material": (8, C.c_int32), "frontFace": (12, C.c_int32)}
    assert [f for f, _ in abi.SrtRayHit._fields_] == list(want)
    for (name, ctype) in abi.SrtRayHit._fields_:
        assert getattr(abi.SrtRayHit, name).offset == want[name][0] and ctype is want[name][1]
        assert abi.RAY_HIT_DTYPE.fields[name][1] == want[name][0]
    # the header's struct, field by field in the same order
    text = abi_header.header()
    body = text[text.index("typedef struct SrtRayHit"):text.index("} SrtRayHit;")]
    assert [body.index(f) for f in ("int32_t prim;", "float t;", "int32_t material;", "int32_t frontFace;")] == sorted(
        body.index(f) for f in ("int32_t prim;", "float t;", "int32_t material;", "int32_t frontFace;"))
    # the first four SrtHit fields a ray hit repeats keep their meaning
    assert abi.SRT_NO_HIT == -1 and C.sizeof(abi.SrtRay) == 36 == 9 * 4


@pytest.mark.parametrize("method", ["trace_device", "occluded_device"])
def test_wrappers_refuse_a_bad_tensor_before_the_c_call(dev, method):
    """A context that was never created has no handle: reaching the C call would fail otherwise than by ValueError."""
    c = object.__new__(dev.Context)
    call = getattr(c, method)
    good = torch.zeros((8, 9), dtype=torch.float32)
    bad = {"on the GPU": good,  # a CPU tensor, right in everything else
           "float32": good.double(),
           "shape": torch.zeros((8, 8), dtype=torch.float32),
           "shape ": torch.zeros(72, dtype=torch.float32),
           "contiguous": torch.zeros((9, 8), dtype=torch.float32).t(),
           "torch tensor": np.zeros((8, 9), np.float32)}
    assert not bad["contiguous"].is_contiguous() and bad["contiguous"].shape == (8, 9)
    for what, rays in bad.items():  # each refusal names its own reason
        with pytest.raises(ValueError, match=what.strip()):
            call(rays)
