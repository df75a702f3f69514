"""CPU-side checks of the denoiser (no GPU): SrtDenoiseParams and the two entries' ctypes prototypes against
include/srt_hip.h, the C++ host layer (srt/device.h hipDevice::rtFrameDenoised, examples/main.cpp --denoise) compiling
against them, and self-checks of the NumPy reference tests/denoise_ref.py that the GPU parity tests rely on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import abi_header
import denoise_ref as R

HEADER = os.path.join(ROOT, "include", "srt_hip.h")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"


def _header():
    return open(HEADER).read()


def _syntax_check(tmp_path, name, text):
    src = tmp_path / name
    src.write_text(text)
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call([HIPCC, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           "-x", "c++", str(src)])


def test_denoise_params_layout_matches_header(tmp_path, abi):
    body = re.search(r"typedef struct SrtDenoiseParams \{(.*?)\} SrtDenoiseParams;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f for _, f, _ in re.findall(r"(int32_t|float)\s+(\w+)(\[\d+\])?;", body)]
    assert fields == [f for f, _ in abi.SrtDenoiseParams._fields_]
    assert C.sizeof(abi.SrtDenoiseParams) == 32
    checks = ["static_assert(sizeof(SrtDenoiseParams) == %d, \"size\");" % C.sizeof(abi.SrtDenoiseParams)]
    for f, _ in abi.SrtDenoiseParams._fields_:
        checks.append("static_assert(offsetof(SrtDenoiseParams, %s) == %d, \"%s\");" % (f, getattr(abi.SrtDenoiseParams, f).offset, f))
    for k in ("MAX_ITERATIONS", "DEFAULT_ITERATIONS", "SCRATCH_BYTES_PER_PIXEL"):
        checks.append("static_assert(SRT_DENOISE_%s == %d, \"%s\");" % (k, getattr(abi, "SRT_DENOISE_" + k), k))
    for k in ("LUMINANCE", "NORMAL", "DEPTH"):
        checks.append("static_assert(SRT_DENOISE_DEFAULT_SIGMA_%s == %rf, \"%s\");" % (k, getattr(abi, "SRT_DENOISE_DEFAULT_SIGMA_" + k), k))
    _syntax_check(tmp_path, "layout.cpp", "#include <cstddef>\n#include \"srt_hip.h\"\n" + "\n".join(checks) + "\n")
    d = abi.default_denoise_params()
    assert (d.iterations, d.demodulate, d.sigmaLuminance, d.sigmaNormal, d.sigmaDepth) == (0, 0, 0.0, 0.0, 0.0)


def test_denoise_ctypes_prototypes_match_header(dev, abi):
    for name in ("srtDenoise", "srtRenderDenoisedImage"):
        abi_header.assert_prototype(dev, abi, name)
        assert name in dev.EXPORTS


def test_denoise_scratch_hook_is_a_test_entry(dev, abi):
    """srtTestDenoiseScratch (include/srt_hip_test.h): the ctypes prototype against the declaration; not an export of the
    drop-in boundary; without a context it fails instead of reading anything."""
    assert "srtTestDenoiseScratch" in abi_header.declarations("srt_hip_test.h")
    assert len(abi_header.assert_prototype(dev, abi, "srtTestDenoiseScratch")) == 7
    assert "srtTestDenoiseScratch" in dev.TEST_EXPORTS and "srtTestDenoiseScratch" not in dev.EXPORTS
    buf = np.full(16, 7.0, np.float32)
    assert dev.lib.srtTestDenoiseScratch(None, 2, 2, buf.ctypes.data_as(C.POINTER(C.c_float)), None, None, None) != 0
    assert (buf == 7.0).all()
    assert callable(getattr(dev.Context, "denoise_scratch", None))


def test_host_layer_compiles_with_denoise_call(tmp_path, dev):
    """srt/device.h's rtFrameDenoised and the example's --denoise path build against the header and the library."""
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    main = open(os.path.join(ROOT, "examples", "main.cpp")).read()
    assert '"--denoise"' in main and "rtFrameDenoised" in main
    _syntax_check(tmp_path, "denoise_call.cpp", """
#include "srt/device.h"
#include <type_traits>
static_assert(std::is_same<decltype(&srtDenoise), int (*)(SrtContext*, const SrtDenoiseParams*, int32_t, int32_t, const void*,
                                                          const void* const*, void*, void*, void*)>::value, "device entry");
static_assert(std::is_same<decltype(&srtRenderDenoisedImage), int (*)(SrtContext*, const SrtRenderParams*, const SrtDenoiseParams*,
                                                                      float*, float*, uint8_t*)>::value, "image entry");
bool frames(hipDevice& d, const camera& cam, std::vector<uint8_t>& noisy, std::vector<uint8_t>& clean) {
  SrtDenoiseParams p{};
  p.iterations = 3;
  p.demodulate = 1;
  std::vector<float> accum(16), out(16);
  return d.rtFrameDenoised(noisy.data(), clean.data(), 2, 2, cam, color3f(0.53f, 0.81f, 0.92f), 4, 4) &&
         d.rtFrameDenoised(nullptr, clean.data(), 2, 2, cam, color3f(0, 0, 0), 4, 4, 7, &p, accum.data(), out.data());
}
""")


# ---- the NumPy reference's own properties


def _planes(H, W, rng, hit=None, spp=4):
    """Synthetic resolved planes: beauty, normal, depth and albedo sums with counts."""
    hit = np.ones((H, W), bool) if hit is None else hit
    beauty = np.zeros((H, W, 4), np.float32)
    beauty[..., :3] = rng.uniform(0.1, 2.0, (H, W, 3)).astype(np.float32) * spp
    beauty[..., 3] = spp
    n = np.zeros((H, W, 4), np.float32)
    n[..., 2] = spp
    n[..., 0] = rng.normal(0, 0.05, (H, W)).astype(np.float32) * spp
    n[..., 3] = np.where(hit, spp, 0)
    n[~hit, :3] = 0
    depth = np.zeros((H, W, 4), np.float32)
    depth[..., 0] = np.where(hit, np.float32(3.0 * spp), 0)
    depth[..., 3] = np.where(hit, spp, 0)
    albedo = np.zeros((H, W, 4), np.float32)
    albedo[..., :3] = rng.uniform(0.2, 0.9, (H, W, 3)).astype(np.float32) * spp
    albedo[..., 3] = spp
    return beauty, n, depth, albedo


@pytest.mark.parametrize("demodulate", [False, True])
def test_reference_keeps_a_constant_image(demodulate):
    rng = np.random.default_rng(1)
    H, W = 23, 37
    beauty, n, depth, albedo = _planes(H, W, rng)
    col = np.float32([0.7, 0.3, 1.9])
    beauty[..., :3] = col * np.float32(4)
    if demodulate:
        albedo[..., :3] = np.float32([0.5, 0.25, 0.75]) * np.float32(4)
    out, rgba = R.denoise(beauty, n, depth, albedo, iterations=5, demodulate=demodulate)
    ulp = np.spacing(col)
    assert (np.abs(out[..., :3] - col) <= 2 * ulp).all()
    assert (out[..., 3] == 4).all() and (rgba[..., 3] == 255).all()


def test_reference_never_mixes_hits_and_misses():
    rng = np.random.default_rng(2)
    H, W = 32, 40
    hit = np.zeros((H, W), bool)
    hit[8:24, 10:30] = True
    beauty, n, depth, _ = _planes(H, W, rng, hit)
    beauty[hit, :3] = 400.0  # bright geometry
    beauty[~hit, :3] = rng.uniform(0.01, 0.02, ((~hit).sum(), 3)).astype(np.float32) * 4
    out, _ = R.denoise(beauty, n, depth, iterations=8)
    assert out[~hit, :3].max() < 0.02 and out[hit, :3].min() > 90


def test_reference_fills_nan_pixels_and_zeroes_unreachable_ones():
    rng = np.random.default_rng(3)
    H, W = 20, 20
    beauty, n, depth, _ = _planes(H, W, rng)
    beauty[7, 9, 0] = np.nan
    beauty[12, 3, :3] = np.inf
    beauty[15, 15, 3] = 0
    out, _ = R.denoise(beauty, n, depth, iterations=1)
    assert np.isfinite(out[..., :3]).all()
    assert (out[7, 9, :3] > 0).all() and (out[12, 3, :3] > 0).all()
    # no valid pixel within reach: a single miss surrounded by hits, its own beauty empty
    hit = np.ones((H, W), bool)
    hit[10, 10] = False
    beauty, n, depth, _ = _planes(H, W, rng, hit)
    beauty[10, 10] = 0
    out, rgba = R.denoise(beauty, n, depth, iterations=3)
    assert (out[10, 10, :3] == 0).all() and (rgba[10, 10, :3] == 0).all()
    assert (out[hit, :3] > 0).all()
