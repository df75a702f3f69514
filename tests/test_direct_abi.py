"""Direct light sampling (include/srt_hip.h "Direct light sampling"), what a machine without a GPU can check: the
prototypes against the headers, the 32-byte SrtDirectOut, where the entries belong, the LDS the whole-path form asks for as
the header states it, and the Python wrappers' refusals that need no device tensor."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import abi_header
from bad_tensors import bad_tensors

PATHS = ["SrtContext*", "int32_t", "int32_t", "const float[3]", "const void*", "int64_t", "void*", "void*", "void*", "void*"]


def test_prototypes_match_the_headers(dev, abi):
    decls = abi_header.declarations("srt_hip.h")
    assert decls["srtGetSampledLights"] == ("int", ["SrtContext*", "int32_t*", "int32_t", "int32_t*"])
    assert decls["srtDirectLightDevice"] == ("int", ["SrtContext*", "int32_t", "const void*", "const void*", "int64_t", "const void*", "void*", "void*"])
    assert decls["srtTracePathsDirectDevice"] == ("int", PATHS) == decls["srtTracePathsDevice"]
    assert decls["srtRenderDirectImage"] == ("int", ["SrtContext*", "const SrtRenderParams*", "int32_t", "float*", "uint8_t*"])
    assert len(abi_header.assert_prototype(dev, abi, "srtRenderDirectImage")) == 5
    hook = abi_header.declarations("srt_hip_test.h")["srtTestEvalScatterDevice"]
    assert hook == ("int", ["SrtContext*", "const void*", "const void*", "const void*", "int64_t", "void*"])
    for name, count in (("srtGetSampledLights", 4), ("srtDirectLightDevice", 8), ("srtTracePathsDirectDevice", 10), ("srtTestEvalScatterDevice", 6)):
        assert len(abi_header.assert_prototype(dev, abi, name)) == count
        assert getattr(dev.lib, name).restype is C.c_int


def test_entries_are_where_they_belong(dev):
    for name in ("srtGetSampledLights", "srtDirectLightDevice", "srtTracePathsDirectDevice", "srtRenderDirectImage"):
        assert name in dev.EXPORTS and name not in dev.TEST_EXPORTS and hasattr(dev.lib, name)
        assert name not in abi_header.declarations("srt_hip_test.h")
    assert "srtTestEvalScatterDevice" in dev.TEST_EXPORTS and "srtTestEvalScatterDevice" not in dev.EXPORTS
    assert "srtTestEvalScatterDevice" not in abi_header.declarations("srt_hip.h")
    for method in ("sampled_lights", "direct_light_device", "eval_scatter_test", "trace_paths_device", "render_direct_image"):
        assert callable(getattr(dev.Context, method, None))


def test_direct_out_is_32_bytes_as_the_header_lays_it_out(abi):
    text = re.sub(r"/\*.*?\*/", "", abi_header.header(), flags=re.S)
    body = re.search(r"typedef struct SrtDirectOut\s*\{(.*?)\}\s*SrtDirectOut;", text, flags=re.S).group(1)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["float radiance[3]", "int32_t light", "float dir[3]", "float weight"]
    assert C.sizeof(abi.SrtDirectOut) == abi.DIRECT_OUT_DTYPE.itemsize == 32
    assert [(n, abi.DIRECT_OUT_DTYPE.fields[n][1]) for n in abi.DIRECT_OUT_DTYPE.names] == [("radiance", 0), ("light", 12), ("dir", 16), ("weight", 28)]
    assert [(n, getattr(abi.SrtDirectOut, n).offset) for n, _ in abi.SrtDirectOut._fields_] == [("radiance", 0), ("light", 12), ("dir", 16), ("weight", 28)]
    row = np.zeros(1, abi.DIRECT_OUT_DTYPE)
    row["light"], row["weight"] = -1, 2.5
    assert row.view(np.int32).tolist() == [0, 0, 0, -1, 0, 0, 0, int(np.float32(2.5).view(np.int32))]


def test_wrappers_refuse_before_the_c_call(dev):
    """A context that was never created has no handle: reaching the C call would fail otherwise than by ValueError."""
    c = object.__new__(dev.Context)
    rays = torch.zeros((8, 9), dtype=torch.float32)
    for what, bad in bad_tensors(rays, 9).items():
        with pytest.raises(ValueError, match="rays.*" + what.strip()):
            c.direct_light_device(bad, None, None)
        with pytest.raises(ValueError, match="rays.*" + what.strip()):
            c.eval_scatter_test(bad, None, None)
        with pytest.raises(ValueError, match="rays.*" + what.strip()):
            c.trace_paths_device(bad, None, 4, (0, 0, 0), direct=True)
