"""CPU-side checks of tile-adaptive sampling (no GPU): the two entries' ctypes prototypes, the structs' layouts and EXPORTS
against include/srt_hip.h, the C++ host layer (hipDevice::rtFrameAdaptive, examples/main.cpp --adaptive) compiling
against them, and self-checks of the NumPy reference tests/adaptive_ref.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
import abi_header
import adaptive_ref as A

HEADER = os.path.join(ROOT, "include", "srt_hip.h")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"


def _header():
    return open(HEADER).read()


def _define(name):
    m = re.search(r"#define %s \(?([^)\n]+)\)?" % name, _header())
    assert m, name
    return eval(m.group(1).replace("f", ""))


def test_adaptive_ctypes_prototypes_match_header(dev, abi):
    for name in ("srtRenderAdaptive", "srtRenderAdaptiveImage"):
        abi_header.assert_prototype(dev, abi, name)
        assert name in dev.EXPORTS and hasattr(dev.lib, name)


def _struct_fields(name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        t, rest = decl.split(" ", 1)
        for var in rest.split(","):
            var = var.strip()
            arr = re.match(r"(\w+)\[(\w+)\]", var)
            out.append((t, arr.group(1), arr.group(2)) if arr else (t, var, None))
    return out


def test_adaptive_struct_layouts(abi):
    sizes = {"int32_t": 4, "int64_t": 8, "float": 4}
    for name in ("SrtAdaptiveParams", "SrtAdaptiveStats"):
        cls = getattr(abi, name)
        fields = _struct_fields(name)
        assert [f[1] for f in fields] == [f[0] for f in cls._fields_], name
        for (t, fname, n), (pyname, ctyp) in zip(fields, cls._fields_):
            count = 1 if n is None else (_define(n) if not n.isdigit() else int(n))
            assert C.sizeof(ctyp) == sizes[t] * count, (name, fname)
            assert getattr(cls, pyname).offset % sizes[t] == 0
    assert C.sizeof(abi.SrtAdaptiveParams) == 16
    assert C.sizeof(abi.SrtAdaptiveStats) == 16 + 3 * 4 * 32
    assert _define("SRT_ADAPTIVE_MAX_ROUNDS") == abi.SRT_ADAPTIVE_MAX_ROUNDS == 32
    assert _define("SRT_ADAPTIVE_MAX_SPP") == abi.SRT_ADAPTIVE_MAX_SPP == 1 << 24
    assert _define("SRT_ADAPTIVE_SCRATCH_BYTES_PER_PIXEL") == abi.SRT_ADAPTIVE_SCRATCH_BYTES_PER_PIXEL
    p = abi.default_adaptive_params(100, 0.25)
    assert p.sppMax == 100 and p.threshold == 0.25


def test_context_has_the_adaptive_methods(dev):
    for name in ("render_adaptive", "render_adaptive_device"):
        assert callable(getattr(dev.Context, name, None)), name


def test_host_layer_and_example_compile(tmp_path, dev):
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    main = open(os.path.join(ROOT, "examples", "main.cpp")).read()
    assert '"--adaptive"' in main and '"--max-spp"' in main
    src = tmp_path / "adaptive_call.cpp"
    src.write_text("""
#include "srt/device.h"
#include <type_traits>
static_assert(std::is_same<decltype(&srtRenderAdaptive), int (*)(SrtContext*, const SrtRenderParams*, const SrtAdaptiveParams*,
                                                                 void*, void*, void*, SrtAdaptiveStats*, void*)>::value, "device");
static_assert(std::is_same<decltype(&srtRenderAdaptiveImage), int (*)(SrtContext*, const SrtRenderParams*, const SrtAdaptiveParams*,
                                                                      float*, float*, uint8_t*, SrtAdaptiveStats*)>::value, "image");
static_assert(sizeof(SrtAdaptiveParams) == 16 && sizeof(SrtAdaptiveStats) == 400, "layout");
bool frame(hipDevice& d, const camera& cam, std::vector<uint8_t>& px) {
  SrtAdaptiveStats st{};
  std::vector<float> accum(16);
  return d.rtFrameAdaptive(px.data(), 2, 2, cam, color3f(0.53f, 0.81f, 0.92f), 4, 4, 64, 0.01f) &&
         d.rtFrameAdaptive(nullptr, 2, 2, cam, color3f(0, 0, 0), 4, 4, 64, 0.0f, 7, accum.data(), &st);
}
""")
    subprocess.check_call([HIPCC, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           "-x", "c++", str(src)])


# ---- the NumPy reference's own properties


def test_schedule():
    assert A.schedule(16, 1000) == [16, 16, 32, 64, 128, 256, 488]
    assert A.schedule(3, 20) == [3, 3, 6, 8]
    assert A.schedule(8, 8) == [8]
    assert len(A.schedule(2, 1 << 24)) <= 32  # SRT_ADAPTIVE_MAX_ROUNDS holds every schedule


def _moments(s1, s2, n):
    m = np.zeros(np.shape(s1) + (4,), np.float32)
    m[..., 0], m[..., 1], m[..., 3] = s1, s2, n
    return m


def test_zero_variance_converges():
    # every sample the same luminance (the sky): v = 0 < any positive limit
    m = _moments(np.full((8, 8), 0.5 * 16, np.float32), np.full((8, 8), 0.25 * 16, np.float32), 16)
    assert A.converged(m, 1e-6).all()
    assert not A.tile_open(A.converged(m, 1e-6)).any()


def test_nan_and_inf_moments_converge():
    m = _moments(np.array([np.nan, np.inf, 1.0]), np.array([1.0, 1.0, np.inf]), 4)
    assert A.converged(m, 0.0).all()


def test_zero_threshold_keeps_everything_and_inf_nothing():
    rng = np.random.default_rng(1)
    x = rng.uniform(0, 2, (16, 20, 32)).astype(np.float32)
    m = _moments(x.sum(-1), (x * x).sum(-1), 32)
    m[:8, :8, 1] = m[:8, :8, 0] ** 2 / 32  # a zero-variance tile: still kept at thr = 0
    assert not A.converged(m, 0.0).any()
    assert A.tile_open(A.converged(m, 0.0)).all()
    assert A.converged(m, float("inf")).all()


def test_convergence_rule_in_display_units():
    # mean 0.25 (display 0.5), variance of the mean 1e-4: display standard error sqrt(1e-4) / (2 * 0.5) = 0.01
    n = 100
    s1 = 0.25 * n
    v_mean = 1e-4
    s2 = (v_mean * n * (n - 1)) + s1 * s1 / n
    m = _moments(np.float32(s1), np.float32(s2), n)[None, None]
    assert A.converged(m, 0.0101).all() and not A.converged(m, 0.0099).any()
    assert np.isclose(A.display_error(m)[0, 0], 0.01, rtol=1e-4)


def test_edge_tiles_ignore_padding():
    conv = np.ones((10, 12), bool)
    assert A.tile_open(conv).shape == (2, 2) and not A.tile_open(conv).any()
    conv[9, 11] = False
    assert A.tile_open(conv).tolist() == [[False, False], [False, True]]
    assert A.pixel_mask(A.tile_open(conv), 10, 12).sum() == 2 * 4


def test_resolve_with_per_pixel_counts():
    acc = np.zeros((1, 3, 4), np.float32)
    acc[0, :, :3] = [[0.5, 4.0, np.nan], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]
    acc[0, :, 3] = [2, 4, 8]
    out = A.resolve(acc)
    g = np.sqrt(np.float32(0.5) * (np.float32(1) / np.float32(2)))
    assert out[0, 0, 0] == int(np.float32(256) * g) and out[0, 0, 1] == 255 and out[0, 0, 2] == 0
    assert out[0, 1, 0] == int(np.float32(256) * np.float32(0.5)) and (out[..., 3] == 255).all()
