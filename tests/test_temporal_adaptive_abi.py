"""CPU-side checks of the temporal-adaptive frame (no GPU): SrtTemporalAdaptiveStats, the constant and the three entries'
ctypes prototypes against include/srt_hip.h, the C++ host layer (hipDevice::rtFrameTemporalAdaptive, examples/main.cpp)
compiling against them, what the entries answer without a context, and the NumPy reference
tests/temporal_adaptive_ref.py on synthetic buffers.  A context needs a GPU, so the entries' error paths proper (a message,
nothing launched, outputs untouched) are in tests/test_gpu_temporal_adaptive.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
import abi_header
import adaptive_ref as A
import temporal_adaptive_ref as TA
import temporal_ref as R
from test_temporal_abi import _camera, _planes

HEADER = os.path.join(ROOT, "include", "srt_hip.h")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
F = np.float32
ENTRIES = ("srtTemporalReproject", "srtRenderTemporalAdaptive", "srtRenderTemporalAdaptiveFrame")


def _header():
    return open(HEADER).read()


def _syntax_check(tmp_path, name, text):
    src = tmp_path / name
    src.write_text(text)
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call([HIPCC, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           "-x", "c++", str(src)])


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_stats_struct_and_constant_match_header(tmp_path, abi):
    body = re.search(r"typedef struct SrtTemporalAdaptiveStats \{(.*?)\} SrtTemporalAdaptiveStats;", _header(), re.S).group(1)
    fields = re.findall(r"(SrtAdaptiveStats|SrtTemporalStats)\s+(\w+);", body)
    cls = abi.SrtTemporalAdaptiveStats
    assert [(t, f) for t, f in fields] == [(t.__name__, f) for f, t in cls._fields_]
    assert C.sizeof(cls) == C.sizeof(abi.SrtAdaptiveStats) + C.sizeof(abi.SrtTemporalStats) == 416
    assert (cls.adaptive.offset, cls.temporal.offset) == (0, 400)
    _syntax_check(tmp_path, "stats.cpp", """#include <cstddef>
#include "srt_hip.h"
static_assert(sizeof(SrtTemporalAdaptiveStats) == %d, "size");
static_assert(offsetof(SrtTemporalAdaptiveStats, adaptive) == %d, "adaptive");
static_assert(offsetof(SrtTemporalAdaptiveStats, temporal) == %d, "temporal");
static_assert(SRT_TEMPORAL_REPROJECTED_BYTES_PER_PIXEL == %d, "reprojected");
""" % (C.sizeof(cls), cls.adaptive.offset, cls.temporal.offset, abi.SRT_TEMPORAL_REPROJECTED_BYTES_PER_PIXEL))
    assert abi.SRT_TEMPORAL_REPROJECTED_BYTES_PER_PIXEL == 32  # two float4 planes


def test_ctypes_prototypes_match_header(dev, abi):
    for name in ENTRIES:
        abi_header.assert_prototype(dev, abi, name)
        assert name in dev.EXPORTS
    for method in ("temporal_reproject", "render_temporal_adaptive_device", "render_temporal_adaptive_frame"):
        assert callable(getattr(dev.Context, method))


def test_entries_without_a_context_fail(dev, abi):
    """No context: non-zero, before any argument is looked at (srtLastError then has nothing to attach a message to)."""
    p, ap, t, d = abi.default_render_params(16, 16, 4, 4), abi.default_adaptive_params(8, 0.01), abi.default_temporal_params(), \
        abi.default_denoise_params()
    planes = (C.c_void_p * 4)()
    cam = dev.make_camera(abi.default_camera_params())
    assert dev.lib.srtTemporalReproject(None, C.byref(t), 16, 16, planes, C.byref(cam), None, None, None, None) != 0
    assert dev.lib.srtRenderTemporalAdaptive(None, C.byref(p), C.byref(ap), C.byref(t), planes, None, None, None, None, None, None,
                                             None, None, None) != 0
    assert dev.lib.srtRenderTemporalAdaptiveFrame(None, C.byref(p), C.byref(ap), C.byref(d), C.byref(t), None, None, None, None) != 0
    assert dev.lib.srtLastError(None) == b"no context"


def test_host_layer_and_example_compile(tmp_path, dev):
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    main = open(os.path.join(ROOT, "examples", "main.cpp")).read()
    assert "rtFrameTemporalAdaptive" in main and "rtFrameTemporal(" in main
    _syntax_check(tmp_path, "temporal_adaptive_call.cpp", """
#include "srt/device.h"
#include <type_traits>
static_assert(std::is_same<decltype(&srtTemporalReproject),
                           int (*)(SrtContext*, const SrtTemporalParams*, int32_t, int32_t, const void* const*, const SrtCamera*,
                                   const SrtCamera*, const void*, void*, void*)>::value, "reproject");
static_assert(std::is_same<decltype(&srtRenderTemporalAdaptive),
                           int (*)(SrtContext*, const SrtRenderParams*, const SrtAdaptiveParams*, const SrtTemporalParams*,
                                   const void* const*, const SrtCamera*, const void*, void*, void*, void*, void*, void*,
                                   SrtTemporalAdaptiveStats*, void*)>::value, "device entry");
static_assert(std::is_same<decltype(&srtRenderTemporalAdaptiveFrame),
                           int (*)(SrtContext*, const SrtRenderParams*, const SrtAdaptiveParams*, const SrtDenoiseParams*,
                                   const SrtTemporalParams*, float*, float*, uint8_t*, SrtTemporalAdaptiveStats*)>::value, "frame");
bool frames(hipDevice& d, const camera& a, const camera& b, std::vector<uint8_t>& out) {
  SrtTemporalParams t{};
  t.demodulate = 1;
  SrtTemporalAdaptiveStats st{};
  std::vector<float> accum(16), den(16);
  return d.rtFrameTemporalAdaptive(out.data(), 2, 2, a, color3f(0.53f, 0.81f, 0.92f), 4, 4, 32, 0.01f, 0) &&
         d.rtFrameTemporal(out.data(), 2, 2, b, color3f(0, 0, 0), 4, 4, 32) &&
         d.rtFrameTemporalAdaptive(out.data(), 2, 2, b, color3f(0, 0, 0), 4, 4, 32, 0.01f, 36, 7, nullptr, &t, accum.data(),
                                   den.data(), &st) &&
         d.temporalReset();
}
""")


# ---- the reference's own invariants, on the synthetic ground-and-box planes of test_temporal_abi.py

TP = dict(normal_cos=0.0, plane_dist=0.0, max_history=0.0, demodulate=False)


def _noisy(cam, W, H, n, rng):
    """_planes with per-pixel noise in the moments: S2 above S1^2 / n by a random relative amount."""
    b, m, nm, ps, dp, al, lab = _planes(cam, W, H, n, rng)
    m[..., 1] = (m[..., 1] * rng.uniform(1.0, 1.5, (H, W))).astype(F)
    return b, m, nm, ps, dp, al, lab


def test_reprojected_planes_reproduce_the_accumulation(dev, abi):
    """Pooling the two planes by the header's formula is temporal_ref.accumulate's moments output bit for bit, on a moved
    camera with accepted and rejected pixels, with and without demodulation and a cap."""
    W, H, n = 96, 64, 4
    prev = _camera(dev, abi, (0.0, 2.0, 4.0), (0.0, 0.5, 0.0))
    cam = _camera(dev, abi, (0.4, 2.0, 4.0), (0.4, 0.5, 0.0))
    rng = np.random.default_rng(11)
    b0, m0, nm0, ps0, dp0, al0, _ = _noisy(prev, W, H, n, rng)
    b1, m1, nm1, ps1, dp1, al1, _ = _noisy(cam, W, H, n, rng)
    m1[3, 5, 0] = np.nan  # not USABLE: stays what it is
    for dm, cap in ((False, 0.0), (True, 3.0), (False, np.inf)):
        _, _, h0 = R.accumulate(b0, m0, nm0, ps0, dp0, al0 if dm else None, prev, prev, None, max_history=cap, demodulate=dm)
        info = {}
        want_b, want_m, _ = R.accumulate(b1, m1, nm1, ps1, dp1, al1 if dm else None, cam, prev, h0, max_history=cap, demodulate=dm,
                                         info=info)
        rp = TA.reproject_history(nm1, ps1, dp1, cam, prev, h0, max_history=cap)
        has = rp[1][..., 3] != 0
        assert np.array_equal(has, info["has"]) and has.any() and (~has).any()
        assert (rp[:, ~has] == 0).all() and np.array_equal(_bits(rp[0][..., 3]), _bits(info["hcount"]))
        if cap == 3.0:
            assert rp[0][..., 3].max() == 3.0
        with np.errstate(all="ignore"):
            usable = np.isfinite(b1).all(-1) & np.isfinite(m1[..., :2]).all(-1) & (b1[..., 3] > 0)
            add = has & usable
            la = F(1)
            at = [F(1)] * 3
            if dm:
                at = [np.maximum(al1[..., k] / al1[..., 3], F(1e-3)) for k in range(3)]
                la = (F(0.2126) * at[0] + F(0.7152) * at[1] + F(0.0722) * at[2]).astype(F)
            pooled = m1.copy()
            pooled[..., 0] = np.where(add, m1[..., 0] + (la * rp[1][..., 0] if dm else rp[1][..., 0]), m1[..., 0])
            pooled[..., 1] = np.where(add, m1[..., 1] + ((la * la) * rp[1][..., 1] if dm else rp[1][..., 1]), m1[..., 1])
            pooled[..., 3] = np.where(add, m1[..., 3] + rp[0][..., 3], m1[..., 3])
            beauty = b1.copy()
            for k in range(3):
                beauty[..., k] = np.where(add, b1[..., k] + (at[k] * rp[0][..., k] if dm else rp[0][..., k]), b1[..., k])
        same = (_bits(pooled) == _bits(want_m)) | (np.isnan(pooled) & np.isnan(want_m))
        assert same.all(), (dm, cap, np.argwhere(~same)[:4].tolist())
        assert np.array_equal(_bits(beauty[..., :3]), _bits(want_b[..., :3]))
        assert np.isnan(pooled[3, 5, 0]) and pooled[3, 5, 3] == n


def test_zero_history_pools_to_the_frames_own_moments(dev, abi):
    W, H, n = 60, 40, 4
    cam = _camera(dev, abi, (0.0, 2.0, 4.0), (0.0, 0.5, 0.0))
    b, m, nm, ps, dp, al, _ = _noisy(cam, W, H, n, np.random.default_rng(12))
    planes = [al, nm, ps, dp]
    assert (TA.reproject_history(nm, ps, dp, cam, None, None) == 0).all()
    assert np.array_equal(_bits(TA.pooled_moments(b, m, planes, cam, None, None, TP)), _bits(m))
    empty = np.zeros((3, H, W, 4), F)  # a history whose every count is 0 is no history either
    assert (TA.reproject_history(nm, ps, dp, cam, cam, empty) == 0).all()
    assert np.array_equal(_bits(TA.pooled_moments(b, m, planes, cam, cam, empty, TP)), _bits(m))


class _Frames:
    """Stands in for a context: render_image_moments of a sample range = deterministic synthetic sums of that many samples."""

    def __init__(self, W, H):
        self.W, self.H, self.calls = W, H, []

    def render_image_moments(self, p, want_rgba=False):
        self.calls.append((p.sampleFirst, p.spp))
        rng = np.random.default_rng(100 + p.sampleFirst)
        x = rng.uniform(0.0, 2.0, (self.H, self.W, p.spp)).astype(F)
        x[:, : self.W // 2] = F(0.5)  # the left half has no noise at all
        acc = np.zeros((self.H, self.W, 4), F)
        acc[..., :3] = x.sum(-1, dtype=F)[..., None]
        acc[..., 3] = p.spp
        mom = np.zeros((self.H, self.W, 4), F)
        mom[..., 0], mom[..., 1], mom[..., 3] = x.sum(-1, dtype=F), (x * x).sum(-1, dtype=F), p.spp
        return acc, mom, None


def test_emulated_frame_schedule_and_thresholds(dev, abi):
    W, H, n, spp_max = 40, 24, 4, 32
    cam = _camera(dev, abi, (0.0, 2.0, 4.0), (0.0, 0.5, 0.0))
    _, _, nm, ps, dp, al, _ = _planes(cam, W, H, n, np.random.default_rng(13))
    planes = [al, nm, ps, dp]
    p = abi.default_render_params(W, H, n, 4, seed=1, spp_chunks=0, sample_first=7)
    tiles = (-(-H // 8)) * (-(-W // 8))
    # threshold = inf closes every tile after round 0: the frame is one moments render and one accumulation
    ctx = _Frames(W, H)
    e = TA.emulate_frame(ctx, p, spp_max, float("inf"), planes, cam, None, None, TP)
    assert ctx.calls == [(7, 4)] and e["counts"] == [tiles] and e["pixel_samples"] == W * H * n and not e["open0"].any()
    assert np.array_equal(_bits(e["beauty_out"]), _bits(e["accum"])) and np.array_equal(_bits(e["moments_out"]), _bits(e["moments"]))
    # threshold 0 without history: every tile to sppMax, the adaptive schedule
    ctx = _Frames(W, H)
    e0 = TA.emulate_frame(ctx, p, spp_max, 0.0, planes, cam, None, None, TP)
    assert ctx.calls == [(7, 4), (11, 4), (15, 8), (23, 16)] and e0["counts"] == [tiles] * 4
    assert (e0["accum"][..., 3] == spp_max).all() and not e0["has"].any()
    # a middle threshold without history is adaptive_ref.emulate itself
    thr = 0.05
    want = A.emulate(_Frames(W, H), p, spp_max, thr)
    e1 = TA.emulate_frame(_Frames(W, H), p, spp_max, thr, planes, cam, None, None, TP)
    assert e1["counts"] == want[3] and 0 < e1["counts"][1] < tiles and e1["pixel_samples"] == want[4]
    assert np.array_equal(_bits(e1["accum"]), _bits(want[0])) and np.array_equal(_bits(e1["moments"]), _bits(want[1]))
    # with that frame's history behind an unmoved camera the next frame needs fewer tiles, and its outputs are the
    # accumulation of its own sums
    q = abi.default_render_params(W, H, n, 4, seed=1, spp_chunks=0, sample_first=7 + spp_max)
    e2 = TA.emulate_frame(_Frames(W, H), q, spp_max, thr, planes, cam, cam, e1["history_out"], TP)
    assert e2["has"].all() and sum(e2["counts"]) < sum(e1["counts"])
    want_b, want_m, want_h = R.accumulate(e2["accum"], e2["moments"], nm, ps, dp, None, cam, cam, e1["history_out"])
    assert np.array_equal(_bits(e2["beauty_out"]), _bits(want_b)) and np.array_equal(_bits(e2["history_out"]), _bits(want_h))
    assert (e2["beauty_out"][..., 3] == e2["accum"][..., 3] + e1["history_out"][0][..., 3]).all()
