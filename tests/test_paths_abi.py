"""srtTracePathsDevice (include/srt_hip.h "Path steps on device buffers"), what a machine without a GPU can check: the
prototype and SrtPathRadiance against the header, the scratch constant, the Python wrapper's refusal of a tensor the C entry
must never see, and the arguments pathloop's whole=True does not go with."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

import torch

import abi_header
from bad_tensors import bad_tensors


def test_prototype_matches_the_header(dev, abi):
    decls = abi_header.declarations("srt_hip.h")
    assert decls["srtTracePathsDevice"] == ("int", ["SrtContext*", "int32_t", "int32_t", "const float[3]", "const void*", "int64_t",
                                                    "void*", "void*", "void*", "void*"])
    assert len(abi_header.assert_prototype(dev, abi, "srtTracePathsDevice")) == 10
    assert dev.lib.srtTracePathsDevice.restype is C.c_int


def test_entry_belongs_to_the_drop_in_boundary(dev):
    name = "srtTracePathsDevice"
    assert name in dev.EXPORTS and name not in dev.TEST_EXPORTS
    assert hasattr(dev.lib, name)
    assert name not in abi_header.declarations("srt_hip_test.h")
    assert name not in abi_header.header("srt_hip_test.h")
    assert callable(getattr(dev.Context, "trace_paths_device", None))


def test_path_radiance_layout(abi):
    assert C.sizeof(abi.SrtPathRadiance) == 16 == abi.PATH_RADIANCE_DTYPE.itemsize
    want = {"radiance": (0, C.c_float * 3), "steps": (12, C.c_int16), "status": (14, C.c_int16)}
    assert [f for f, _ in abi.SrtPathRadiance._fields_] == list(want)
    for (name, ctype) in abi.SrtPathRadiance._fields_:
        assert getattr(abi.SrtPathRadiance, name).offset == want[name][0] and ctype is want[name][1]
        assert abi.PATH_RADIANCE_DTYPE.fields[name][1] == want[name][0]
    text = abi_header.header()
    body = text[text.index("typedef struct SrtPathRadiance"):text.index("} SrtPathRadiance;")]
    at = [body.index(f) for f in ("float radiance[3];", "int16_t steps;", "int16_t status;")]
    assert at == sorted(at)
    # a status fits its 16 bits, and the row is the wrapper's (n, 4) int32: steps in the low half of column 3
    row = np.zeros(1, abi.PATH_RADIANCE_DTYPE)
    row["steps"], row["status"] = 5, abi.SRT_PATH_INVALID
    assert int(row.view(np.int32)[3]) == np.int32(np.uint32(0xffff0005).view(np.int32))


def test_scratch_constant(abi):
    found = re.findall(r"enum\s*\{\s*SRT_PATHS_SCRATCH_BYTES\s*=\s*(\d+)\s*\}\s*;", abi_header.header())
    assert found == ["64"] and abi.SRT_PATHS_SCRATCH_BYTES == 64
    found = re.findall(r"#define\s+SRT_MAX_BOUNCE\s+(\d+)", abi_header.header())
    assert found == [str(abi.SRT_MAX_BOUNCE)]


def test_wrapper_refuses_a_bad_tensor_before_the_c_call(dev):
    """A context that was never created has no handle: reaching the C call would fail otherwise than by ValueError."""
    c = object.__new__(dev.Context)
    rng = torch.zeros((8,), dtype=torch.int64)
    for what, bad in bad_tensors(torch.zeros((8, 9), dtype=torch.float32), 9).items():  # each refusal names its own reason
        with pytest.raises(ValueError, match="rays.*" + what.strip()):
            c.trace_paths_device(bad, rng, 4, (0.0, 0.0, 0.0))
    # rng is checked behind rays: rays that answer the wrapper's questions as an (8, 9) float32 tensor on a GPU would
    for what, bad in {"on the GPU": rng, "must be": rng.to(torch.int32), "shape": torch.zeros((8, 1), dtype=torch.int64),
                      "shape ": torch.zeros((7,), dtype=torch.int64), "contiguous": torch.zeros((16,), dtype=torch.int64)[::2],
                      "torch tensor": np.zeros(8, np.int64)}.items():
        with pytest.raises(ValueError, match="rng.*" + what.strip()):
            c.trace_paths_device(_RaysOnAGpu(), bad, 4, (0.0, 0.0, 0.0))


class _RaysOnAGpu:
    dtype, shape, is_cuda, device = torch.float32, (8, 9), True, torch.device("cuda", 0)

    def dim(self):
        return 2

    def is_contiguous(self):
        return True

    def data_ptr(self):
        raise AssertionError("the wrapper went on to the C call")


def test_whole_goes_with_neither_counts_nor_compaction_nor_the_unfused_steps(srt):
    pathloop = importlib.import_module("sexy-raytracer_amd.pathloop")
    p = srt.abi.default_render_params(16, 12, 1, 4)
    for kwargs in ({"active_counts": []}, {"compact": True}, {"fused": False}):
        with pytest.raises(ValueError, match="whole"):
            pathloop.render(None, p, whole=True, **kwargs)
        with pytest.raises(ValueError, match="whole"):
            pathloop.sample_radiance(None, None, None, 4, (0.0, 0.0, 0.0), whole=True, **kwargs)
    import inspect
    assert inspect.signature(pathloop.render).parameters["whole"].default is False
    assert inspect.signature(pathloop.sample_radiance).parameters["whole"].default is False
