"""CPU-side checks of the temporal accumulation (no GPU): SrtTemporalParams, the constants and the entries' ctypes prototypes
against include/srt_hip.h, the C++ host layer (srt/device.h hipDevice::rtFrameTemporal, examples/main.cpp --temporal)
compiling against them, and the NumPy reference tests/temporal_ref.py on synthetic planes built analytically (a ground
plane and a box in front of it), including the measurement behind SRT_TEMPORAL_SNAP."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import abi_header
import temporal_ref as R

HEADER = os.path.join(ROOT, "include", "srt_hip.h")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
F = np.float32


def _header():
    return open(HEADER).read()


def _syntax_check(tmp_path, name, text):
    src = tmp_path / name
    src.write_text(text)
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call([HIPCC, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           "-x", "c++", str(src)])


def test_temporal_structs_and_constants_match_header(tmp_path, abi):
    for struct, size in (("SrtTemporalParams", 32), ("SrtTemporalStats", 16)):
        cls = getattr(abi, struct)
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f for _, f, _ in re.findall(r"(int32_t|int64_t|float|double)\s+(\w+)(\[\d+\])?;", body)]
        assert fields == [f for f, _ in cls._fields_]
        assert C.sizeof(cls) == size
        checks = ["static_assert(sizeof(%s) == %d, \"size\");" % (struct, size)]
        for f, _ in cls._fields_:
            checks.append("static_assert(offsetof(%s, %s) == %d, \"%s\");" % (struct, f, getattr(cls, f).offset, f))
        _syntax_check(tmp_path, struct + ".cpp", "#include <cstddef>\n#include \"srt_hip.h\"\n" + "\n".join(checks) + "\n")
    checks = ["static_assert(SRT_TEMPORAL_HISTORY_BYTES_PER_PIXEL == %d, \"history\");" % abi.SRT_TEMPORAL_HISTORY_BYTES_PER_PIXEL]
    for k in ("SNAP", "DEFAULT_NORMAL_COS", "DEFAULT_PLANE_DIST", "DEFAULT_MAX_HISTORY"):
        checks.append("static_assert(SRT_TEMPORAL_%s == (float)%r, \"%s\");" % (k, getattr(abi, "SRT_TEMPORAL_" + k), k))
    _syntax_check(tmp_path, "constants.cpp", "#include \"srt_hip.h\"\n" + "\n".join(checks) + "\n")
    assert abi.SRT_TEMPORAL_HISTORY_BYTES_PER_PIXEL == 48
    assert (R.SNAP, R.DEFAULT_NORMAL_COS, R.DEFAULT_PLANE_DIST, R.DEFAULT_MAX_HISTORY) == (
        abi.SRT_TEMPORAL_SNAP, abi.SRT_TEMPORAL_DEFAULT_NORMAL_COS, abi.SRT_TEMPORAL_DEFAULT_PLANE_DIST,
        abi.SRT_TEMPORAL_DEFAULT_MAX_HISTORY)
    t = abi.default_temporal_params()
    assert (t.normalCos, t.planeDist, t.maxHistory, t.demodulate) == (0.0, 0.0, 0.0, 0)


def test_temporal_ctypes_prototypes_match_header(dev, abi):
    for name in ("srtTemporalAccumulate", "srtRenderTemporalFrame", "srtTemporalReset"):
        abi_header.assert_prototype(dev, abi, name)
        assert name in dev.EXPORTS
    for method in ("temporal_accumulate", "render_temporal_frame", "temporal_reset"):
        assert callable(getattr(dev.Context, method))


def test_host_layer_compiles_with_temporal_call(tmp_path, dev):
    """srt/device.h's rtFrameTemporal and the example's --frames / --orbit / --temporal path build against the header."""
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    main = open(os.path.join(ROOT, "examples", "main.cpp")).read()
    assert all(s in main for s in ('"--temporal"', '"--frames"', '"--orbit"', "rtFrameTemporal"))
    _syntax_check(tmp_path, "temporal_call.cpp", """
#include "srt/device.h"
#include <type_traits>
static_assert(std::is_same<decltype(&srtTemporalAccumulate),
                           int (*)(SrtContext*, const SrtTemporalParams*, int32_t, int32_t, const void*, const void*, const void* const*,
                                   const SrtCamera*, const SrtCamera*, const void*, void*, void*, void*, void*)>::value, "device entry");
static_assert(std::is_same<decltype(&srtRenderTemporalFrame),
                           int (*)(SrtContext*, const SrtRenderParams*, const SrtDenoiseParams*, const SrtTemporalParams*, float*, float*,
                                   uint8_t*, SrtTemporalStats*)>::value, "frame entry");
bool frames(hipDevice& d, const camera& a, const camera& b, std::vector<uint8_t>& out) {
  SrtTemporalParams t{};
  t.maxHistory = 32.0f;
  t.demodulate = 1;
  SrtTemporalStats st{};
  std::vector<float> accum(16), den(16);
  return d.rtFrameTemporal(out.data(), 2, 2, a, color3f(0.53f, 0.81f, 0.92f), 4, 4, 0) &&
         d.rtFrameTemporal(out.data(), 2, 2, b, color3f(0, 0, 0), 4, 4, 4, 7, nullptr, &t, accum.data(), den.data(), &st) &&
         d.temporalReset();
}
""")


# ---- synthetic planes: a ground plane y = 0 and an axis-aligned box standing on it, seen through make_camera's pinhole


def _camera(dev, abi, eye, look, vfov=40.0, aspect=1.5):
    c = abi.default_camera_params(aspect)
    c.eye[:], c.lookAt[:] = eye, look
    c.vfovDegrees, c.aperture = vfov, 0.0
    return dev.make_camera(c)


BOX = (np.array([-0.5, 0.0, -0.5]), np.array([0.5, 1.0, 0.5]))


def _planes(cam, W, H, n, rng, box=True, colour=None):
    """Analytic feature planes (sums with counts, n samples) of the ground and the box for `cam`, and a beauty / moments pair.
    Returns (beauty, moments, normal, position, depth, albedo, label): label 0 = sky, 1 = ground, 2 = box."""
    d, _ = R.pixel_ray(cam, W, H, np.float64)
    o = np.array(list(cam.origin), np.float64)
    D = np.stack(d, -1)
    with np.errstate(all="ignore"):
        t = np.where(D[..., 1] < 0, -o[1] / D[..., 1], np.inf)
        normal = np.zeros((H, W, 3))
        normal[..., 1] = 1
        label = np.where(np.isfinite(t), 1, 0)
        if box:
            t0 = (BOX[0] - o) / D
            t1 = (BOX[1] - o) / D
            near, far = np.minimum(t0, t1), np.maximum(t0, t1)
            tn, tf = near.max(-1), far.min(-1)
            hitb = (tn <= tf) & (tn > 0) & (tn < t)
            axis = near.argmax(-1)
            nb = np.zeros((H, W, 3))
            np.put_along_axis(nb, axis[..., None], -np.sign(np.take_along_axis(D, axis[..., None], -1)), -1)
            t = np.where(hitb, tn, t)
            normal = np.where(hitb[..., None], nb, normal)
            label = np.where(hitb, 2, label)
    hit = label > 0
    ts = np.where(hit, t, 0.0)
    P = o + ts[..., None] * D
    cnt = np.where(hit, n, 0).astype(F)

    def plane(v):
        out = np.zeros((H, W, 4), F)
        out[..., :3] = np.where(hit[..., None], v, 0.0).astype(F) * F(n)
        out[..., 3] = cnt
        return out

    depth = np.zeros((H, W, 4), F)
    depth[..., 0] = ts.astype(F) * F(n)
    depth[..., 3] = cnt
    beauty = np.zeros((H, W, 4), F)
    beauty[..., :3] = (rng.uniform(0.1, 2.0, (H, W, 3)) if colour is None else colour).astype(F) * F(n)
    beauty[..., 3] = n
    lum = beauty[..., :3] @ np.float32([0.2126, 0.7152, 0.0722]) / F(n)
    moments = np.zeros((H, W, 4), F)
    moments[..., 0], moments[..., 1], moments[..., 3] = lum * F(n), lum * lum * F(n), n
    albedo = np.zeros((H, W, 4), F)
    albedo[..., :3] = rng.uniform(0.2, 0.9, (H, W, 3)).astype(F) * F(n)
    albedo[..., 3] = n
    return beauty, moments, plane(normal), plane(P), depth, albedo, label


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_same_camera_is_the_running_sum(dev, abi):
    W, H, n, K = 60, 40, 4, 5
    cam = _camera(dev, abi, (0.0, 2.0, 4.0), (0.0, 0.5, 0.0))
    rng = np.random.default_rng(1)
    hist, sum_b, sum_m = None, None, None
    for k in range(K):
        b, m, nm, ps, dp, al, _ = _planes(cam, W, H, n, rng)
        out_b, out_m, hist = R.accumulate(b, m, nm, ps, dp, None, cam, cam, hist, max_history=np.inf)
        sum_b = b if sum_b is None else sum_b + b
        sum_m = m if sum_m is None else sum_m + m
        assert np.array_equal(_bits(out_b), _bits(sum_b)) and np.array_equal(_bits(out_m), _bits(sum_m))
        assert (out_b[..., 3] == (k + 1) * n).all() and np.array_equal(_bits(hist[0]), _bits(sum_b))


def test_sideways_translation_over_the_ground(dev, abi):
    W, H, n, shift = 96, 64, 4, 0.3
    prev = _camera(dev, abi, (0.0, 4.0, 3.0), (0.0, 0.0, 0.0))
    cam = _camera(dev, abi, (shift, 4.0, 3.0), (shift, 0.0, 0.0))
    rng = np.random.default_rng(2)
    b0, m0, nm0, ps0, dp0, _, lab0 = _planes(prev, W, H, n, rng, box=False)
    assert (lab0 == 1).all()  # the ground fills the frame
    _, _, h0 = R.accumulate(b0, m0, nm0, ps0, dp0, None, prev, prev, None)
    b1, m1, nm1, ps1, dp1, _, _ = _planes(cam, W, H, n, rng, box=False)
    info = {}
    out_b, _, _ = R.accumulate(b1, m1, nm1, ps1, dp1, None, cam, prev, h0, info=info)
    # the camera moved along its own horizontal axis: a point at depth tbar (units of d) shifts by
    # shift (W - 1) / (tbar |horizontal|) pixels in x and not at all in y
    tbar = (dp1[..., 0] / dp1[..., 3]).astype(np.float64)
    hlen = np.linalg.norm(np.float64(list(cam.horizontal)))
    want_x = np.arange(W)[None, :] + shift * (W - 1) / (tbar * hlen)
    want_y = np.broadcast_to(np.arange(H)[:, None], (H, W))
    err = R.SNAP / 4  # the snap measurement's bound on the float32 projection error
    assert np.abs(info["xf"] - want_x).max() <= err and np.abs(info["yf"] - want_y).max() <= err
    inside = (info["xf"] >= 0) & (info["xf"] <= W - 1)
    assert inside.any() and (~inside).any()
    assert info["has"][inside].all()
    assert (out_b[..., 3][inside] > n).all() and (out_b[..., 3][inside] <= 2 * n).all()
    gone = info["xf"] >= W
    assert gone.any() and (out_b[..., 3][gone] == n).all()


def test_box_disocclusion_starts_over(dev, abi):
    W, H, n, shift = 120, 80, 4, 0.4
    prev = _camera(dev, abi, (0.0, 2.0, 4.0), (0.0, 0.5, 0.0))
    cam = _camera(dev, abi, (shift, 2.0, 4.0), (shift, 0.5, 0.0))
    rng = np.random.default_rng(3)
    b0, m0, nm0, ps0, dp0, _, lab0 = _planes(prev, W, H, n, rng)
    _, _, h0 = R.accumulate(b0, m0, nm0, ps0, dp0, None, prev, prev, None)
    b1, m1, nm1, ps1, dp1, _, lab1 = _planes(cam, W, H, n, rng)
    info = {}
    out_b, out_m, h1 = R.accumulate(b1, m1, nm1, ps1, dp1, None, cam, prev, h0, info=info)
    # labels of the four taps in the previous frame
    x0, y0 = np.floor(info["xf"]).astype(int), np.floor(info["yf"]).astype(int)
    tap_inside, tap_lab = [], []
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = x0 + dx, y0 + dy
            ins = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            tap_inside.append(ins)
            tap_lab.append(np.where(ins, lab0[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)], -1))
    tap_inside, tap_lab = np.stack(tap_inside), np.stack(tap_lab)
    uncovered = (lab1 == 1) & (tap_lab == 2).all(0)  # ground now, the box's front then
    kept = (lab1 == 2) & tap_inside.all(0) & (tap_lab == 2).all(0)
    assert uncovered.sum() > 20 and kept.sum() > 100
    assert (out_b[..., 3][uncovered] == n).all()
    assert np.array_equal(_bits(out_b[uncovered]), _bits(b1[uncovered]))  # exactly the current frame
    assert np.array_equal(_bits(h1[0][uncovered]), _bits(b1[uncovered]))
    # the box's own pixels keep their history unless the tap sits on another face (the side the move reveals)
    same_face = kept & (np.abs(nm1[..., :3] / n - h0[1][np.clip(y0, 0, H - 1), np.clip(x0, 0, W - 1), :3]).max(-1) == 0)
    assert same_face.sum() > 100 and info["has"][same_face].all()
    # sky never takes geometry and geometry never takes sky
    sky_from_hits = (lab1 == 0) & (tap_lab > 0).all(0)
    assert (out_b[..., 3][sky_from_hits] == n).all()


def test_max_history_caps_the_count_and_keeps_a_constant(dev, abi):
    W, H, n, cap = 40, 30, 4, 10.0
    cam = _camera(dev, abi, (0.0, 2.0, 4.0), (0.0, 0.5, 0.0))
    rng = np.random.default_rng(4)
    col = np.float32([0.7, 0.3, 1.9])
    hist = None
    for k in range(8):
        b, m, nm, ps, dp, al, _ = _planes(cam, W, H, n, rng, colour=np.broadcast_to(col, (H, W, 3)))
        out_b, out_m, hist = R.accumulate(b, m, nm, ps, dp, None, cam, cam, hist, max_history=cap)
        assert out_b[..., 3].max() <= n + cap and hist[0][..., 3].max() <= n + cap
        assert out_b[..., 3].min() == min((k + 1) * n, n + cap)
        mean = out_b[..., :3] / out_b[..., 3:4]
        assert np.abs(mean / col - 1).max() <= 4 * np.finfo(F).eps
        lum = out_m[..., 0] / out_m[..., 3]
        assert np.abs(lum / (col @ np.float32([0.2126, 0.7152, 0.0722])) - 1).max() <= 8 * np.finfo(F).eps


def test_demodulated_history_multiplies_back(dev, abi):
    """A static camera with constant radiance and a textured albedo: the accumulated mean stays the radiance, and a pixel
    without history is the current frame bit for bit."""
    W, H, n = 40, 30, 4
    cam = _camera(dev, abi, (0.0, 2.0, 4.0), (0.0, 0.5, 0.0))
    rng = np.random.default_rng(5)
    hist = None
    for k in range(4):
        b, m, nm, ps, dp, al, _ = _planes(cam, W, H, n, np.random.default_rng(5))  # the same frame (and albedo) every time
        out_b, out_m, hist = R.accumulate(b, m, nm, ps, dp, al, cam, cam, hist, max_history=np.inf, demodulate=True)
        if k == 0:
            assert np.array_equal(_bits(out_b), _bits(b)) and np.array_equal(_bits(out_m), _bits(m))
        assert (out_b[..., 3] == (k + 1) * n).all()
        assert np.abs(out_b[..., :3] / ((k + 1) * b[..., :3]) - 1).max() <= 16 * np.finfo(F).eps
    assert rng is not None


def test_non_finite_values_never_reach_another_pixels_history(dev, abi):
    W, H, n = 48, 32, 4
    prev = _camera(dev, abi, (0.0, 2.0, 4.0), (0.0, 0.5, 0.0))
    cam = _camera(dev, abi, (0.13, 2.0, 4.0), (0.13, 0.5, 0.0))
    rng = np.random.default_rng(6)
    b0, m0, nm0, ps0, dp0, _, lab0 = _planes(prev, W, H, n, rng)
    # current-frame NaN / inf: the pixel keeps them, its history stays clean
    b0[5, 7, 0] = np.nan
    b0[9, 11, :3] = np.inf
    m0[12, 3, 1] = np.inf
    out_b, out_m, h0 = R.accumulate(b0, m0, nm0, ps0, dp0, None, prev, prev, None)
    assert np.isnan(out_b[5, 7, 0]) and np.isinf(out_b[9, 11, 0]) and np.isinf(out_m[12, 3, 1])
    for y, x in ((5, 7), (9, 11), (12, 3)):
        assert (h0[0][y, x] == 0).all() and h0[1][y, x, 3] == 0 and h0[2][y, x, 3] == 0
    assert np.isfinite(h0[0]).all() and np.isfinite(h0[1][..., 3]).all() and np.isfinite(h0[2][..., 3]).all()
    # a history record that will be rejected (a non-finite count; a sky record poisoned with NaN where geometry looks)
    h0 = h0.copy()
    h0[0][20, 20] = (np.nan, np.nan, np.nan, np.inf)
    h0[1][20, 20, 3] = h0[2][20, 20, 3] = np.nan
    sky = np.argwhere(lab0 == 0)
    assert len(sky)
    b1, m1, nm1, ps1, dp1, _, lab1 = _planes(cam, W, H, n, rng)
    poisoned = h0.copy()
    ground = np.argwhere(lab0 == 1)[::7]
    for y, x in ground:  # ground records turned into NaN-filled sky records: geometry must not take them
        poisoned[0][y, x, :3] = np.nan
        poisoned[1][y, x] = (np.nan, 0, 0, np.nan)
        poisoned[2][y, x] = (0, 0, 0, np.nan)
    out_b, out_m, h1 = R.accumulate(b1, m1, nm1, ps1, dp1, None, cam, prev, poisoned)
    geometry = lab1 > 0
    assert np.isfinite(out_b[geometry]).all() and np.isfinite(out_m[geometry]).all()
    assert np.isfinite(h1[0][geometry]).all() and np.isfinite(h1[1][..., 3][geometry]).all()
    assert (out_b[..., 3] >= n).all() and np.isfinite(out_b[..., 3]).all()


def _orbit_camera(dev, abi, degrees):
    c = abi.default_camera_params()
    a = np.deg2rad(degrees)
    dx, dz = c.eye[0] - c.lookAt[0], c.eye[2] - c.lookAt[2]
    c.eye[0] = c.lookAt[0] + np.float32(np.cos(a)) * dx + np.float32(np.sin(a)) * dz
    c.eye[2] = c.lookAt[2] + np.float32(np.cos(a)) * dz - np.float32(np.sin(a)) * dx
    return dev.make_camera(c)


def test_snap_constant_covers_the_measured_round_trip(dev, abi):
    """The derivation of SRT_TEMPORAL_SNAP: the float32 round trip pixel -> P -> the same camera over every pixel of
    1920 x 1080, the test cameras (the default one and three positions of its orbit), depths 1e-2 .. 1e4."""
    W, H = 1920, 1080
    worst, by_depth = 0.0, {}
    for deg in (0.0, 7.0, 20.0, 45.0):
        cam = _orbit_camera(dev, abi, deg)
        for depth in (1e-2, 1e-1, 1.0, 10.0, 1e2, 1e3, 1e4):
            ex, ey = R.round_trip_error(cam, W, H, F(depth))
            by_depth[depth] = max(by_depth.get(depth, 0.0), ex, ey)
            worst = max(worst, ex, ey)
    print("round trip error by depth:", {k: "%.3g" % v for k, v in by_depth.items()}, "worst %.4g px" % worst)
    assert abi.SRT_TEMPORAL_SNAP >= 4 * worst
    assert abi.SRT_TEMPORAL_SNAP <= 8 * worst or abi.SRT_TEMPORAL_SNAP <= 2.0 ** -6  # a power of two just above, not a guess
    assert np.log2(abi.SRT_TEMPORAL_SNAP) == np.round(np.log2(abi.SRT_TEMPORAL_SNAP))
    # in float64 the same arithmetic closes the loop up to the float32 camera's own inconsistency (horizontal, vertical and
    # w are orthogonal to 1e-7 only): the error above is rounding, not the formulas
    ex, ey = R.round_trip_error(_orbit_camera(dev, abi, 7.0), W, H, 3.0, np.float64)
    print("float64 round trip: %.3g px" % max(ex, ey))
    assert max(ex, ey) < abi.SRT_TEMPORAL_SNAP / 256
