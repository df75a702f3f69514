"""Path steps on device buffers (include/srt_hip.h), what a machine without a GPU can check: the ctypes prototypes of
srtRngKey, srtCameraRaysDevice, srtScatterRaysDevice and srtPathStepDevice against the header, SrtPathOut's layout, the
Python wrappers' refusal of a tensor the C entry must never see, and srtRngKey and the tests' NumPy mirror of the counter
RNG (tests/pathstep_ref.py) against the oracle's generator."""
import ctypes as C

import numpy as np
import pytest

import torch

import abi_header
from bad_tensors import bad_tensors
import pathstep_ref as PR

DEVICE_ENTRIES = ("srtCameraRaysDevice", "srtScatterRaysDevice", "srtPathStepDevice")
# seed, pixel, sample: zeros, values near 2^31 and 2^32, a seed with its top bit set
KEYS = [(0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0), (7, 12345, 3), (2 ** 63 + 5, 2 ** 31 - 1, 2 ** 31 - 1),
        (99, 2 ** 31, 0), (99, 0, 2 ** 31), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (5, 1280 * 720 - 1, 4999),
        (0xDEADBEEF, 2 ** 31 + 1, 2 ** 31 - 2), (42, 191, 2)]


def test_prototypes_match_the_header(dev, abi):
    decls = abi_header.declarations("srt_hip.h")
    assert decls["srtRngKey"] == ("uint64_t", ["uint64_t", "uint64_t", "uint64_t"])  # pixel, sample: their low 32 bits
    assert decls["srtCameraRaysDevice"] == ("int", ["SrtContext*", "const SrtRenderParams*", "const void*", "int64_t", "void*",
                                                    "void*", "void*"])
    assert decls["srtScatterRaysDevice"] == ("int", ["SrtContext*", "const void*", "const void*", "int64_t", "void*", "void*",
                                                     "void*", "void*"])
    assert decls["srtPathStepDevice"] == ("int", ["SrtContext*", "int32_t", "const void*", "int64_t", "const void*", "void*",
                                                  "void*", "void*", "void*", "void*"])
    for name, count in zip(("srtRngKey",) + DEVICE_ENTRIES, (3, 7, 8, 10)):
        assert len(abi_header.assert_prototype(dev, abi, name)) == count
    assert dev.lib.srtRngKey.restype is C.c_uint64
    for name in DEVICE_ENTRIES:
        assert getattr(dev.lib, name).restype is C.c_int


def test_entries_belong_to_the_drop_in_boundary(dev):
    for name in ("srtRngKey",) + DEVICE_ENTRIES:
        assert name in dev.EXPORTS and name not in dev.TEST_EXPORTS
        assert hasattr(dev.lib, name)
        assert name not in abi_header.declarations("srt_hip_test.h")
    for method in ("camera_rays_device", "scatter_device", "path_step_device"):
        assert callable(getattr(dev.Context, method, None)), method


def test_path_out_layout_and_status_values(abi):
    assert C.sizeof(abi.SrtPathOut) == 32 == abi.PATH_OUT_DTYPE.itemsize
    want = {"attenuation": (0, C.c_float * 3), "status": (12, C.c_int32), "emitted": (16, C.c_float * 3), "prim": (28, C.c_int32)}
    assert [f for f, _ in abi.SrtPathOut._fields_] == list(want)
    for (name, ctype) in abi.SrtPathOut._fields_:
        assert getattr(abi.SrtPathOut, name).offset == want[name][0] and ctype is want[name][1]
        assert abi.PATH_OUT_DTYPE.fields[name][1] == want[name][0]
    text = abi_header.header()
    body = text[text.index("typedef struct SrtPathOut"):text.index("} SrtPathOut;")]
    at = [body.index(f) for f in ("float attenuation[3];", "int32_t status;", "float emitted[3];", "int32_t prim;")]
    assert at == sorted(at)
    assert "enum { SRT_PATH_INVALID = -1, SRT_PATH_MISS = 0, SRT_PATH_ENDED = 1, SRT_PATH_SCATTERED = 2 };" in text
    assert (abi.SRT_PATH_INVALID, abi.SRT_PATH_MISS, abi.SRT_PATH_ENDED, abi.SRT_PATH_SCATTERED) == (-1, 0, 1, 2)


def test_wrappers_refuse_a_bad_tensor_before_the_c_call(dev, abi):
    """A context that was never created has no handle: reaching the C call would fail otherwise than by ValueError."""
    c = object.__new__(dev.Context)
    rays = torch.zeros((8, 9), dtype=torch.float32)
    rng = torch.zeros((8,), dtype=torch.int64)
    for what, bad in bad_tensors(rays, 9).items():  # each refusal names its own reason
        with pytest.raises(ValueError, match=what.strip()):
            c.path_step_device(bad, rng)
        with pytest.raises(ValueError, match=what.strip()):
            c.scatter_device(bad, torch.zeros((8, 22), dtype=torch.int32), rng)
    p = abi.default_render_params(16, 12, 1, 4)
    for what, bad in bad_tensors(torch.zeros((8, 2), dtype=torch.int32), 2).items():
        with pytest.raises(ValueError, match="pixel_sample.*" + what.strip()):
            c.camera_rays_device(p, bad)


def test_rng_key_and_the_mirror_are_the_oracle_generator(dev, oracle):
    for seed, pixel, sample in KEYS:
        state = dev.rng_key(seed, pixel, sample)
        assert state == PR.rng_key(seed, pixel, sample) == int(dev.lib.srtRngKey(seed, pixel, sample))
        g = PR.Pcg(state)
        got = np.array([g.uniform() for _ in range(64)], np.float32)
        want = oracle.rng_counter(seed, pixel, sample, 64)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (seed, pixel, sample)
        assert PR.from_int64(PR.as_int64(state)) == state
    assert len({PR.rng_key(*k) for k in KEYS}) == len(KEYS)
    # the C entry takes pixel and sample as uint64_t and uses their low 32 bits
    assert int(dev.lib.srtRngKey(9, 2 ** 32 + 5, 2 ** 40 + 7)) == PR.rng_key(9, 5, 7)
    # the rejection loops consume whole trips and return a point inside
    g = PR.Pcg(PR.rng_key(3, 4, 5))
    for _ in range(50):
        x, y = g.in_unit_disk()
        assert x * x + y * y < 1
        x, y, z = g.in_unit_sphere()
        assert x * x + y * y + z * z < 1
