"""CPU-side checks of the motion entries (no GPU): the ctypes prototypes of hipdev.py against include/srt_hip.h, the
export table, the binding's methods, the host layer and the example compiling against the declarations, and the entries'
behaviour without a context."""
import ctypes as C
import inspect
import os
import subprocess

from conftest import ROOT
import abi_header

ENTRIES = ("srtSetMotionTracking", "srtRenderMotionTiles", "srtRenderMotionImage", "srtTemporalAccumulateMotion",
           "srtTemporalReprojectMotion")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"


def test_motion_ctypes_prototypes_match_header(dev, abi):
    decls = abi_header.declarations("srt_hip.h")
    for name in ENTRIES:
        assert name in decls and name in dev.EXPORTS and name not in dev.TEST_EXPORTS
        abi_header.assert_prototype(dev, abi, name)
        assert getattr(dev.lib, name).restype is C.c_int and decls[name][0] == "int"
        assert hasattr(dev.lib, name)
    assert decls["srtSetMotionTracking"][1] == ["SrtContext*", "int32_t"]
    assert decls["srtRenderMotionTiles"][1] == ["SrtContext*", "const SrtRenderParams*", "void*", "void*"]
    assert decls["srtRenderMotionImage"][1] == ["SrtContext*", "const SrtRenderParams*", "float*"]


def test_motion_entries_are_the_plain_entries_plus_the_plane():
    """Each Motion entry's parameter list is the plain entry's with `const void*` dMotion after the planes."""
    decls = abi_header.declarations("srt_hip.h")
    for plain in ("srtTemporalAccumulate", "srtTemporalReproject"):
        base, motion = decls[plain][1], decls[plain + "Motion"][1]
        at = base.index("const void* const[4]") + 1
        assert motion == base[:at] + ["const void*"] + base[at:]


def test_binding_methods(dev):
    for method in ("set_motion_tracking", "render_motion", "render_motion_tiles"):
        assert callable(getattr(dev.Context, method))
    for method in ("temporal_accumulate", "temporal_reproject"):
        par = inspect.signature(getattr(dev.Context, method)).parameters
        assert par["motion_ptr"].default is None


def test_entries_fail_without_a_context(dev, abi):
    p = abi.default_render_params(44, 28, 1, 1)
    out = (C.c_float * 4)(7, 7, 7, 7)
    assert dev.lib.srtSetMotionTracking(None, 1) != 0
    assert dev.lib.srtRenderMotionTiles(None, C.byref(p), C.cast(out, C.c_void_p), None) != 0
    assert dev.lib.srtRenderMotionImage(None, C.byref(p), out) != 0
    assert list(out) == [7, 7, 7, 7]


def test_host_layer_and_example_compile_with_the_motion_calls(tmp_path, dev):
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    main = open(os.path.join(ROOT, "examples", "main.cpp")).read()
    assert all(s in main for s in ('"--motion"', "setMotionTracking", "rtMotion"))
    src = tmp_path / "motion_call.cpp"
    src.write_text("""
#include "srt/device.h"
#include <type_traits>
static_assert(std::is_same<decltype(&srtSetMotionTracking), int (*)(SrtContext*, int32_t)>::value, "flag");
static_assert(std::is_same<decltype(&srtRenderMotionTiles), int (*)(SrtContext*, const SrtRenderParams*, void*, void*)>::value, "tiles");
static_assert(std::is_same<decltype(&srtRenderMotionImage), int (*)(SrtContext*, const SrtRenderParams*, float*)>::value, "image");
static_assert(std::is_same<decltype(&srtTemporalAccumulateMotion),
                           int (*)(SrtContext*, const SrtTemporalParams*, int32_t, int32_t, const void*, const void*, const void* const*,
                                   const void*, const SrtCamera*, const SrtCamera*, const void*, void*, void*, void*, void*)>::value, "accumulate");
static_assert(std::is_same<decltype(&srtTemporalReprojectMotion),
                           int (*)(SrtContext*, const SrtTemporalParams*, int32_t, int32_t, const void* const*, const void*,
                                   const SrtCamera*, const SrtCamera*, const void*, void*, void*)>::value, "reproject");
bool frames(hipDevice& d, const camera& c, std::vector<uint8_t>& out, std::vector<float>& plane) {
  SrtTemporalStats st{};
  return d.setMotionTracking(true) && d.updateTriangles(0, d.triangles) && d.refit() &&
         d.rtFrameTemporal(out.data(), 2, 2, c, color3f(0, 0, 0), 4, 4, 4, 1, nullptr, nullptr, nullptr, nullptr, &st) &&
         d.rtMotion(c, color3f(0, 0, 0), 4, 1, 4, plane) && d.setMotionTracking(false);
}
""")
    subprocess.check_call([HIPCC, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           "-x", "c++", str(src)])
