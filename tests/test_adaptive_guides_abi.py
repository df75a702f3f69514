"""CPU-side checks of the feature pass over tile lists and the guided adaptive entries (no GPU): the five entries' ctypes
prototypes against include/srt_hip.h, what they answer without a context, the Context methods, the C++ host layer
(hipDevice::rtFrameAdaptiveDenoised, the guided switch of rtFrameTemporalAdaptive, examples/main.cpp) compiling against
them, and the NumPy emulation tests/adaptive_guides_ref.py on synthetic count maps.  The entries' behaviour on a context is
in tests/test_gpu_adaptive_guides.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import abi_header
import adaptive_guides_ref as G
import adaptive_ref as A

HEADER = os.path.join(ROOT, "include", "srt_hip.h")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
F = np.float32
ENTRIES = ("srtRenderFeatureTileList", "srtRenderAdaptiveGuided", "srtRenderAdaptiveDenoisedImage",
           "srtRenderTemporalAdaptiveGuided", "srtRenderTemporalAdaptiveGuidedFrame")
METHODS = ("render_feature_tile_list", "render_adaptive_guided_device", "render_adaptive_denoised",
           "render_temporal_adaptive_guided_device", "render_temporal_adaptive_frame")


def _header():
    return open(HEADER).read()


def _syntax_check(tmp_path, name, text):
    src = tmp_path / name
    src.write_text(text)
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call([HIPCC, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           "-x", "c++", str(src)])


def test_ctypes_prototypes_match_header(dev, abi):
    for name in ENTRIES:
        abi_header.assert_prototype(dev, abi, name)
        assert name in dev.EXPORTS
    for method in METHODS:
        assert callable(getattr(dev.Context, method))
    import inspect
    assert "guided" in inspect.signature(dev.Context.render_temporal_adaptive_frame).parameters


def test_entries_without_a_context_fail(dev, abi):
    p, ap, t, d = abi.default_render_params(16, 16, 4, 4), abi.default_adaptive_params(8, 0.01), abi.default_temporal_params(), \
        abi.default_denoise_params()
    planes = (C.c_void_p * 4)()
    lib = dev.lib
    assert lib.srtRenderFeatureTileList(None, C.byref(p), 15, None, 0, planes, 0, None) != 0
    assert lib.srtRenderAdaptiveGuided(None, C.byref(p), C.byref(ap), 15, planes, None, None, None, None, None) != 0
    assert lib.srtRenderAdaptiveDenoisedImage(None, C.byref(p), C.byref(ap), C.byref(d), None, None, None, None, None) != 0
    assert lib.srtRenderTemporalAdaptiveGuided(None, C.byref(p), C.byref(ap), C.byref(t), planes, None, None, None, None, None, None,
                                               None, None, None) != 0
    assert lib.srtRenderTemporalAdaptiveGuidedFrame(None, C.byref(p), C.byref(ap), C.byref(d), C.byref(t), None, None, None, None) != 0
    assert lib.srtLastError(None) == b"no context"


def test_host_layer_and_example_compile(tmp_path, dev):
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    main = open(os.path.join(ROOT, "examples", "main.cpp")).read()
    assert "rtFrameAdaptiveDenoised" in main and "--guide-all-samples" in main
    _syntax_check(tmp_path, "adaptive_guides_call.cpp", """
#include "srt/device.h"
#include <type_traits>
static_assert(std::is_same<decltype(&srtRenderFeatureTileList),
                           int (*)(SrtContext*, const SrtRenderParams*, int32_t, const void*, int32_t, void* const*, int32_t,
                                   void*)>::value, "list");
static_assert(std::is_same<decltype(&srtRenderAdaptiveGuided),
                           int (*)(SrtContext*, const SrtRenderParams*, const SrtAdaptiveParams*, int32_t, void* const*, void*, void*,
                                   void*, SrtAdaptiveStats*, void*)>::value, "guided");
static_assert(std::is_same<decltype(&srtRenderAdaptiveDenoisedImage),
                           int (*)(SrtContext*, const SrtRenderParams*, const SrtAdaptiveParams*, const SrtDenoiseParams*, float*,
                                   float*, float*, uint8_t*, SrtAdaptiveStats*)>::value, "image");
static_assert(std::is_same<decltype(&srtRenderTemporalAdaptiveGuided),
                           int (*)(SrtContext*, const SrtRenderParams*, const SrtAdaptiveParams*, const SrtTemporalParams*,
                                   void* const*, const SrtCamera*, const void*, void*, void*, void*, void*, void*,
                                   SrtTemporalAdaptiveStats*, void*)>::value, "device entry");
static_assert(std::is_same<decltype(&srtRenderTemporalAdaptiveGuidedFrame), decltype(&srtRenderTemporalAdaptiveFrame)>::value, "frame");
bool frames(hipDevice& d, const camera& a, std::vector<uint8_t>& out) {
  SrtAdaptiveStats st{};
  SrtTemporalAdaptiveStats ts{};
  std::vector<float> accum(16), den(16);
  return d.rtFrameAdaptiveDenoised(out.data(), out.data(), 2, 2, a, color3f(0.53f, 0.81f, 0.92f), 4, 4, 32, 0.01f) &&
         d.rtFrameAdaptiveDenoised(nullptr, out.data(), 2, 2, a, color3f(0, 0, 0), 4, 4, 32, 0.01f, 7, nullptr, accum.data(),
                                   den.data(), &st) &&
         d.rtFrameTemporalAdaptive(out.data(), 2, 2, a, color3f(0, 0, 0), 4, 4, 32, 0.01f, 36, 7, nullptr, nullptr, accum.data(),
                                   den.data(), &ts, true);
}
""")


# ---- the emulation on synthetic count maps


class _Params:
    def __init__(self, w, h, spp, first):
        self.imageWidth, self.imageHeight, self.spp, self.sampleFirst, self.sppChunks = w, h, spp, first, 0


def _sample(s, H, W, k):
    """the synthetic feature value of sample s of every pixel, plane k"""
    y, x = np.mgrid[0:H, 0:W]
    return (np.sin(0.37 * s + 0.11 * x + 0.07 * y + k) + F(1.5)).astype(F)


def _range_sums(calls, H, W):
    def f(q):
        calls.append((q.sampleFirst, q.spp))
        out = []
        for k in range(4):
            acc = np.zeros((H, W, 4), F)
            for s in range(q.sampleFirst, q.sampleFirst + q.spp):  # the running float sum, in sample-index order from 0
                v = _sample(s, H, W, k)
                acc[..., 0] = acc[..., 0] + v
                acc[..., 1] = acc[..., 1] + v * F(0.5)
                acc[..., 3] = acc[..., 3] + F(1)
            out.append(acc)
        return out
    return f


def test_emulation_on_synthetic_count_maps():
    W, H, n0, spp_max, first = 21, 19, 4, 32, 5  # 3 x 3 tiles, edge tiles on both axes
    counts = np.array([[4, 8, 32], [16, 4, 32], [8, 32, 16]], F)  # stopped after round 0, in middle rounds, at sppMax
    pix = A.pixel_mask(counts, H, W)
    assert np.array_equal(G.tile_counts(pix), counts)
    calls = []
    got = G.emulate_planes(_range_sums(calls, H, W), _Params(W, H, n0, first), spp_max, pix)
    assert calls == [(5, 4), (9, 4), (13, 8), (21, 16)]
    # independently, tile by tile: ((pass0 + pass1) + pass2) + ... up to the tile's own count
    bounds = np.cumsum([0] + A.schedule(n0, spp_max))
    ranges = _range_sums([], H, W)
    for ty in range(3):
        for tx in range(3):
            sl = (slice(8 * ty, min(8 * ty + 8, H)), slice(8 * tx, min(8 * tx + 8, W)))
            for k in range(4):
                want = None
                for r in range(len(bounds) - 1):
                    if bounds[r + 1] > counts[ty, tx]:
                        break
                    part = ranges(_Params(W, H, int(bounds[r + 1] - bounds[r]), first + int(bounds[r])))[k][sl]
                    want = part if want is None else want + part
                assert np.array_equal(got[k][sl].view(np.uint32), want.view(np.uint32)), (ty, tx, k)
                assert (got[k][sl][..., 3] == counts[ty, tx]).all()
    # the caller's own first planes, planes that are not followed, and a frame that stopped after round 0
    calls = []
    base = _range_sums([], H, W)(_Params(W, H, n0, first))
    again = G.emulate_planes(_range_sums(calls, H, W), _Params(W, H, n0, first), spp_max, pix, first=[None] + base[1:])
    assert calls == [(9, 4), (13, 8), (21, 16)] and again[0] is None
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again[1:], got[1:]))
    calls = []
    flat = G.emulate_planes(_range_sums(calls, H, W), _Params(W, H, n0, first), spp_max, np.full((H, W), n0, F))
    assert calls == [(5, 4)] and all(np.array_equal(a, b) for a, b in zip(flat, base))
    with pytest.raises(AssertionError):
        bad = pix.copy()
        bad[0, 0] = 8
        G.tile_counts(bad)
    assert G.tile_list([(12, 3), (0, 7)]).tolist() == [12 | 3 << 16, 7 << 16]
