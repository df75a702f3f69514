"""ctypes binding of csrc/libsrt_hip.so, the C-ABI library declared in include/srt_hip.h.

Importing this module loads the HIP extension and raises if it is not built: there is
no CPU fallback for the hot path."""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsrt_hip.so")
if os.environ.get("SRT_HIP_LIB"):  # measurement tools only: an experimental build of the same library
    LIB_PATH = os.path.abspath(os.environ["SRT_HIP_LIB"])

if not os.path.exists(LIB_PATH):
    raise ImportError("HIP extension not built: %s is missing (run __graft_entry__.build() or "
                      "`make -C sexy-raytracer_amd/csrc`)" % LIB_PATH)

# PyTorch-ROCm wheels carry their own libamdhip64 / libhsa-runtime64 (same sonames as /opt/rocm's, which this library is
# linked against).  One process gets ONE of them -- whichever is loaded first -- and torch does not find the GPU through
# /opt/rocm's copy ("No HIP GPUs are available").  The tests and bench.py take their device buffers from torch, so torch
# goes first when it is there; the library runs on either copy.  (C / C++ callers never meet this.)
try:
    import torch  # noqa: F401
except ImportError:
    pass

lib = C.CDLL(LIB_PATH)

EXPORTS = ["srtCreate", "srtDestroy", "srtLastError", "srtMakeCamera", "srtHostRandomFloat", "srtHostRandomReset",
           "srtUploadScene", "srtSetCamera", "srtBuildBvh", "srtGetBvh", "srtGetBvhDepth", "srtNumTiles", "srtNumLocalTiles", "srtDefaultSppChunks", "srtPlanSppChunks",
           "srtRenderTiles", "srtResolveTiles", "srtRenderImage", "srtRenderFeatureTiles", "srtRenderFeatureImage",
           "srtDenoise", "srtRenderDenoisedImage", "srtTraceRays", "srtTraceRaysDevice", "srtOccludedDevice", "srtScatterRays",
           "srtRngKey", "srtCameraRaysDevice", "srtScatterRaysDevice", "srtPathStepDevice",
           "srtCompactPathsScratchBytes", "srtCompactPathsDevice", "srtSortPathsScratchBytes", "srtSortPathsDevice", "srtTracePathsDevice",
           "srtGetSampledLights", "srtDirectLightDevice", "srtTracePathsDirectDevice", "srtRenderDirectImage",
           "srtRenderTilesMoments", "srtRenderImageMoments", "srtDenoiseMoments", "srtRenderDenoisedImageMoments",
           "srtRenderAdaptive", "srtRenderAdaptiveImage",
           "srtTemporalAccumulate", "srtRenderTemporalFrame", "srtTemporalReset",
           "srtTemporalReproject", "srtRenderTemporalAdaptive", "srtRenderTemporalAdaptiveFrame",
           "srtRenderFeatureTileList", "srtRenderAdaptiveGuided", "srtRenderAdaptiveDenoisedImage",
           "srtRenderTemporalAdaptiveGuided", "srtRenderTemporalAdaptiveGuidedFrame",
           "srtUpdateTriangles", "srtUpdateSpheres", "srtUpdateTrianglesDevice", "srtUpdateSpheresDevice", "srtRefitScene",
           "srtRebuildScene", "srtGetTreeCost",
           "srtSetMotionTracking", "srtRenderMotionTiles", "srtRenderMotionImage", "srtTemporalAccumulateMotion",
           "srtTemporalReprojectMotion",
           "srtCommGetUniqueId", "srtCommInit", "srtGatherTiles", "srtRenderImageRanks", "srtCommDestroy",
           "srtLastKernelMs", "srtGetStats", "srtDeviceInfo"]
# include/srt_hip_test.h: test hooks and diagnostics, not part of the drop-in boundary
TEST_EXPORTS = ["srtSetTunable", "srtGetTunable", "srtGetShadeProfile", "srtGetWfProfile", "srtGetLaunchInfo", "srtRenderAov",
                "srtScatterRaysForm", "srtTestThreadLinks16", "srtTestHybridRecords", "srtTestGetTreeAux", "srtTestChunkSum",
                "srtTestDenoiseScratch", "srtTestGetTriUndecided", "srtTestGetTriFast", "srtTestTriFastRecord", "srtTestGetSlabScene",
                "srtTestRefinedRcp", "srtTestSlabVisit", "srtTestRegroup", "srtTestGetRegroup",
                "srtTestRegroupWalk", "srtTestGetRegroupWalk", "srtTestWfHead", "srtTestEvalScatterDevice"]

_vp = C.c_void_p
lib.srtCreate.argtypes = [C.c_int, C.POINTER(_vp)]
lib.srtDestroy.argtypes = [_vp]
lib.srtLastError.argtypes = [_vp]
lib.srtLastError.restype = C.c_char_p
lib.srtMakeCamera.argtypes = [C.POINTER(abi.SrtCameraParams), C.POINTER(abi.SrtCamera)]
lib.srtHostRandomFloat.restype = C.c_float
lib.srtHostRandomReset.restype = None
lib.srtUploadScene.argtypes = [_vp, C.POINTER(abi.SrtSceneDesc)]
lib.srtSetCamera.argtypes = [_vp, C.POINTER(abi.SrtCamera)]
lib.srtBuildBvh.argtypes = [C.POINTER(abi.SrtSceneDesc), C.c_int32, _vp, C.c_int32, C.POINTER(C.c_int32),
                            C.POINTER(C.c_int32)]
lib.srtGetBvh.argtypes = [_vp, C.c_int32, _vp, C.c_int32, C.POINTER(C.c_int32)]
lib.srtGetBvhDepth.argtypes = [_vp, C.POINTER(C.c_int32)]
lib.srtNumTiles.argtypes = [C.c_int32, C.c_int32]
lib.srtNumTiles.restype = C.c_int32
lib.srtNumLocalTiles.argtypes = [C.c_int32, C.c_int32, C.c_int32]
lib.srtNumLocalTiles.restype = C.c_int32
lib.srtDefaultSppChunks.argtypes = [C.c_int32]
lib.srtDefaultSppChunks.restype = C.c_int32
lib.srtPlanSppChunks.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
lib.srtPlanSppChunks.restype = C.c_int32
lib.srtRenderTiles.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), _vp, _vp]
lib.srtResolveTiles.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), _vp, _vp, _vp, _vp]
lib.srtRenderImage.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), _vp, _vp]
lib.srtRenderFeatureTiles.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.c_int32, C.POINTER(_vp), _vp]
lib.srtRenderFeatureImage.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.c_int32, C.POINTER(C.POINTER(C.c_float))]
lib.srtDenoise.argtypes = [_vp, C.POINTER(abi.SrtDenoiseParams), C.c_int32, C.c_int32, _vp, C.POINTER(_vp), _vp, _vp, _vp]
lib.srtRenderDenoisedImage.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.POINTER(abi.SrtDenoiseParams),
                                       C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
lib.srtRenderTilesMoments.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), _vp, _vp, _vp]
lib.srtRenderImageMoments.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), _vp, _vp, _vp]
lib.srtDenoiseMoments.argtypes = [_vp, C.POINTER(abi.SrtDenoiseParams), C.c_int32, C.c_int32, _vp, C.POINTER(_vp), _vp, _vp,
                                  _vp, _vp]
lib.srtRenderDenoisedImageMoments.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.POINTER(abi.SrtDenoiseParams),
                                              C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                              C.POINTER(C.c_uint8)]
lib.srtRenderAdaptive.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.POINTER(abi.SrtAdaptiveParams), _vp, _vp, _vp,
                                  C.POINTER(abi.SrtAdaptiveStats), _vp]
lib.srtRenderAdaptiveImage.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.POINTER(abi.SrtAdaptiveParams),
                                       C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8),
                                       C.POINTER(abi.SrtAdaptiveStats)]
lib.srtTemporalAccumulate.argtypes = [_vp, C.POINTER(abi.SrtTemporalParams), C.c_int32, C.c_int32, _vp, _vp, C.POINTER(_vp),
                                      C.POINTER(abi.SrtCamera), C.POINTER(abi.SrtCamera), _vp, _vp, _vp, _vp, _vp]
lib.srtRenderTemporalFrame.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.POINTER(abi.SrtDenoiseParams),
                                       C.POINTER(abi.SrtTemporalParams), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       C.POINTER(C.c_uint8), C.POINTER(abi.SrtTemporalStats)]
lib.srtTemporalReset.argtypes = [_vp]
lib.srtTemporalReproject.argtypes = [_vp, C.POINTER(abi.SrtTemporalParams), C.c_int32, C.c_int32, C.POINTER(_vp),
                                     C.POINTER(abi.SrtCamera), C.POINTER(abi.SrtCamera), _vp, _vp, _vp]
lib.srtRenderTemporalAdaptive.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.POINTER(abi.SrtAdaptiveParams),
                                          C.POINTER(abi.SrtTemporalParams), C.POINTER(_vp), C.POINTER(abi.SrtCamera), _vp, _vp,
                                          _vp, _vp, _vp, _vp, C.POINTER(abi.SrtTemporalAdaptiveStats), _vp]
lib.srtRenderTemporalAdaptiveFrame.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.POINTER(abi.SrtAdaptiveParams),
                                               C.POINTER(abi.SrtDenoiseParams), C.POINTER(abi.SrtTemporalParams),
                                               C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8),
                                               C.POINTER(abi.SrtTemporalAdaptiveStats)]
lib.srtRenderFeatureTileList.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.c_int32, _vp, C.c_int32, C.POINTER(_vp), C.c_int32,
                                         _vp]
lib.srtRenderAdaptiveGuided.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.POINTER(abi.SrtAdaptiveParams), C.c_int32,
                                        C.POINTER(_vp), _vp, _vp, _vp, C.POINTER(abi.SrtAdaptiveStats), _vp]
lib.srtRenderAdaptiveDenoisedImage.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.POINTER(abi.SrtAdaptiveParams),
                                               C.POINTER(abi.SrtDenoiseParams), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                               C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(abi.SrtAdaptiveStats)]
lib.srtRenderTemporalAdaptiveGuided.argtypes = lib.srtRenderTemporalAdaptive.argtypes
lib.srtRenderTemporalAdaptiveGuidedFrame.argtypes = lib.srtRenderTemporalAdaptiveFrame.argtypes
lib.srtUpdateTriangles.argtypes = lib.srtUpdateSpheres.argtypes = [_vp, C.c_int32, C.c_int32, _vp]
lib.srtUpdateTrianglesDevice.argtypes = lib.srtUpdateSpheresDevice.argtypes = [_vp, C.c_int32, C.c_int32, _vp, _vp]
lib.srtRefitScene.argtypes = [_vp, _vp]
lib.srtRebuildScene.argtypes = [_vp, _vp]
lib.srtGetTreeCost.argtypes = [_vp, C.c_int32, _vp]  # double* cost (an address, like the other untyped outputs)
lib.srtSetMotionTracking.argtypes = [_vp, C.c_int32]
lib.srtRenderMotionTiles.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), _vp, _vp]
lib.srtRenderMotionImage.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.POINTER(C.c_float)]
lib.srtTemporalAccumulateMotion.argtypes = [_vp, C.POINTER(abi.SrtTemporalParams), C.c_int32, C.c_int32, _vp, _vp, C.POINTER(_vp),
                                            _vp, C.POINTER(abi.SrtCamera), C.POINTER(abi.SrtCamera), _vp, _vp, _vp, _vp, _vp]
lib.srtTemporalReprojectMotion.argtypes = [_vp, C.POINTER(abi.SrtTemporalParams), C.c_int32, C.c_int32, C.POINTER(_vp), _vp,
                                           C.POINTER(abi.SrtCamera), C.POINTER(abi.SrtCamera), _vp, _vp, _vp]
lib.srtTraceRays.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int32]
lib.srtTraceRaysDevice.argtypes = [_vp, _vp, C.c_int64, C.c_int32, _vp, _vp, _vp]
lib.srtOccludedDevice.argtypes = [_vp, _vp, C.c_int64, _vp, _vp]
lib.srtRngKey.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
lib.srtRngKey.restype = C.c_uint64
lib.srtCameraRaysDevice.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), _vp, C.c_int64, _vp, _vp, _vp]
lib.srtScatterRaysDevice.argtypes = [_vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp]
lib.srtPathStepDevice.argtypes = [_vp, C.c_int32, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]
lib.srtCompactPathsScratchBytes.argtypes = [C.c_int64]
lib.srtCompactPathsScratchBytes.restype = C.c_int64
lib.srtCompactPathsDevice.argtypes = [_vp, C.c_int64] + [_vp] * 12
lib.srtSortPathsScratchBytes.argtypes = [C.c_int64]
lib.srtSortPathsScratchBytes.restype = C.c_int64
lib.srtSortPathsDevice.argtypes = [_vp, C.c_int64, C.c_int32] + [_vp] * 12 + [C.c_int64, _vp]
lib.srtTracePathsDevice.argtypes = [_vp, C.c_int32, C.c_int32, C.POINTER(C.c_float), _vp, C.c_int64, _vp, _vp, _vp, _vp]
lib.srtTracePathsDirectDevice.argtypes = lib.srtTracePathsDevice.argtypes
lib.srtGetSampledLights.argtypes = [_vp, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]
lib.srtDirectLightDevice.argtypes = [_vp, C.c_int32, _vp, _vp, C.c_int64, _vp, _vp, _vp]
lib.srtRenderDirectImage.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
lib.srtTestEvalScatterDevice.argtypes = [_vp, _vp, _vp, _vp, C.c_int64, _vp]
lib.srtCommGetUniqueId.argtypes = [_vp]
lib.srtCommInit.argtypes = [_vp, _vp, C.c_int32, C.c_int32]
lib.srtGatherTiles.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), _vp, _vp, _vp]
lib.srtRenderImageRanks.argtypes = [_vp, C.POINTER(abi.SrtRenderParams), _vp, _vp]
lib.srtCommDestroy.argtypes = [_vp]
lib.srtScatterRays.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_uint64, _vp]
lib.srtScatterRaysForm.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_uint64, C.c_int32, _vp, _vp]
lib.srtTestChunkSum.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp]
lib.srtTestDenoiseScratch.argtypes = [_vp, C.c_int32, C.c_int32] + [C.POINTER(C.c_float)] * 4
lib.srtSetTunable.argtypes = [_vp, C.c_char_p, C.c_int32]
lib.srtGetTunable.argtypes = [_vp, C.c_char_p, C.POINTER(C.c_int32)]
lib.srtGetShadeProfile.argtypes = [_vp, _vp]
lib.srtGetWfProfile.argtypes = [_vp, _vp]
lib.srtGetLaunchInfo.argtypes = [_vp, _vp]
lib.srtTestThreadLinks16.argtypes = [_vp, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, _vp]
lib.srtTestHybridRecords.argtypes = [_vp, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]
lib.srtTestThreadLinks16.restype = lib.srtTestHybridRecords.restype = C.c_int32
lib.srtTestGetTreeAux.argtypes = [_vp, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32)]
if hasattr(lib, "srtTestGetTriUndecided"):  # (an SRT_HIP_LIB build from before the certified triangle test lacks the three)
    lib.srtTestGetTriUndecided.argtypes = [_vp, C.POINTER(C.c_uint64)]
    lib.srtTestGetTriFast.argtypes = [_vp, _vp, C.c_int32, C.POINTER(C.c_int32)]
    lib.srtTestTriFastRecord.argtypes = [_vp, _vp]
if hasattr(lib, "srtTestGetSlabScene"):  # (likewise: an SRT_HIP_LIB build from before the ordered-box condition)
    lib.srtTestGetSlabScene.argtypes = [_vp, C.POINTER(C.c_int32)]
if hasattr(lib, "srtTestRefinedRcp"):  # (likewise: an SRT_HIP_LIB build from before the slab-test hooks)
    lib.srtTestRefinedRcp.argtypes = [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_uint64)]
    lib.srtTestSlabVisit.argtypes = [_vp, C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_int32, C.POINTER(C.c_float)]
if hasattr(lib, "srtTestRegroup"):  # (likewise: an SRT_HIP_LIB build from before the regrouped tree)
    lib.srtTestRegroup.argtypes = [_vp, C.c_int32, _vp, C.c_int32, _vp]
    lib.srtTestRegroup.restype = C.c_int32
    lib.srtTestGetRegroup.argtypes = [_vp, _vp, _vp, C.c_int32, C.POINTER(C.c_int32)]
if hasattr(lib, "srtTestRegroupWalk"):  # (likewise: an SRT_HIP_LIB build from before the walk sequence)
    lib.srtTestRegroupWalk.argtypes = [_vp, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32)]
    lib.srtTestRegroupWalk.restype = C.c_int32
    lib.srtTestGetRegroupWalk.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.POINTER(C.c_int32)]
if hasattr(lib, "srtTestWfHead"):  # (likewise: an SRT_HIP_LIB build from before the head of the walks)
    lib.srtTestWfHead.argtypes = [_vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, C.POINTER(C.c_int32)]
    lib.srtTestWfHead.restype = C.c_int32
lib.srtRenderAov.argtypes =[_vp, C.POINTER(abi.SrtRenderParams), C.c_int32, _vp]
lib.srtLastKernelMs.argtypes = [_vp, C.POINTER(C.c_float)]
lib.srtGetStats.argtypes = [_vp, C.POINTER(abi.SrtStats)]
lib.srtDeviceInfo.argtypes = [_vp, C.c_char_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]


class SrtError(RuntimeError):
    pass


def make_camera(params):
    """camera ctor arithmetic (camera.h:10-38) on the host; needs no GPU."""
    cam = abi.SrtCamera()
    if lib.srtMakeCamera(C.byref(params), C.byref(cam)):
        raise SrtError("srtMakeCamera failed")
    return cam


def rng_key(seed, pixel, sample):
    """srtRngKey: the generator state a render gives (pixel, sample) before its first draw, as a Python int in [0, 2^64).
    (A torch int64 tensor of states holds the same bits: subtract 2^64 from a value of 2^63 or more.)"""
    return int(lib.srtRngKey(int(seed) & (2 ** 64 - 1), int(pixel) & 0xffffffff, int(sample) & 0xffffffff))


def host_random_reset():
    lib.srtHostRandomReset()


def host_random_float():
    return float(lib.srtHostRandomFloat())


def num_tiles(w, h):
    return int(lib.srtNumTiles(w, h))


def num_local_tiles(w, h, stride):
    return int(lib.srtNumLocalTiles(w, h, stride))


def default_spp_chunks(spp):
    return int(lib.srtDefaultSppChunks(spp))


def plan_spp_chunks(width, height, spp, spp_chunks=0):
    """The chunk count a render of this size uses (-1: an explicit count that does not fit); include/srt_hip.h."""
    return int(lib.srtPlanSppChunks(width, height, spp, spp_chunks))


def _reset_generator_for(scene_builder):
    """The process-global generator as the reference's process would have it when the world's bvhNode is
    constructed: fresh (globals.h:31-32), minus the draws the scene's own construction code took
    (scenes.scene_sphere_field records them)."""
    host_random_reset()
    for _ in range(int(getattr(scene_builder, "global_rng_draws", 0))):
        lib.srtHostRandomFloat()


def build_bvh_host(scene_builder, item=0, reset_rng=True):
    """bvh.h:55-95 on the host, no GPU: returns (nodes, traversal stack depth)."""
    desc = scene_builder.desc()
    n, sd = C.c_int32(0), C.c_int32(0)
    if reset_rng:
        _reset_generator_for(scene_builder)
    if lib.srtBuildBvh(C.byref(desc), item, None, 0, C.byref(n), C.byref(sd)):
        raise SrtError("srtBuildBvh failed")
    if reset_rng:  # the sizing call consumed generator draws: rebuild from the same state
        _reset_generator_for(scene_builder)
    nodes = np.zeros(n.value, abi.NODE_DTYPE)
    if lib.srtBuildBvh(C.byref(desc), item, nodes.ctypes.data, n.value, C.byref(n), C.byref(sd)):
        raise SrtError("srtBuildBvh failed")
    return nodes, sd.value


def comm_unique_id():
    """128 opaque bytes from RCCL (rank 0 calls this and hands them to the other ranks)."""
    buf = C.create_string_buffer(128)
    if lib.srtCommGetUniqueId(buf):
        raise SrtError("srtCommGetUniqueId failed")
    return buf.raw


class Context:
    """One per GPU (glDevice's role, gl.h:16-40)."""

    def __init__(self, device=0):
        h = _vp()
        if lib.srtCreate(device, C.byref(h)):
            raise SrtError("srtCreate(%d) failed: no usable HIP device" % device)
        self.h = h
        self._scene_keep = None

    def close(self):
        # `lib` is already gone when a context is collected at interpreter shutdown
        if getattr(self, "h", None) and lib is not None:
            lib.srtDestroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc):
        if rc:
            raise SrtError(lib.srtLastError(self.h).decode())

    def upload_scene(self, scene_builder, reset_rng=True):
        """reset_rng: start from the process-global generator of a new process of the reference
        (globals.h:31-32), advanced past the draws the scene's construction took."""
        if reset_rng:
            _reset_generator_for(scene_builder)
        desc = scene_builder.desc()
        self._scene_keep = (scene_builder, desc)
        self._check(lib.srtUploadScene(self.h, C.byref(desc)))

    def set_camera(self, cam):
        self._check(lib.srtSetCamera(self.h, C.byref(cam)))
        self._camera_bytes = bytes(cam)

    def fingerprint(self):
        """sha1 over the uploaded scene description and the camera: what a checkpoint of accumulated samples
        belongs to (progressive.py)."""
        import hashlib
        h = hashlib.sha1()
        if self._scene_keep is not None:
            for a in self._scene_keep[0]._keep:
                h.update(bytes(memoryview(a)) if not hasattr(a, "tobytes") else a.tobytes())
        h.update(getattr(self, "_camera_bytes", b""))
        return h.hexdigest()

    def bvh(self, item=0):
        n = C.c_int32(0)
        self._check(lib.srtGetBvh(self.h, item, None, 0, C.byref(n)))
        nodes = np.zeros(n.value, abi.NODE_DTYPE)
        self._check(lib.srtGetBvh(self.h, item, nodes.ctypes.data, n.value, C.byref(n)))
        return nodes

    def bvh_depth(self):
        d = C.c_int32(0)
        self._check(lib.srtGetBvhDepth(self.h, C.byref(d)))
        return d.value

    def tree_aux(self, item=0):
        """What the near-child-first traversal reads beside the node array (include/srt_hip_test.h srtTestGetTreeAux):
        returns (axis, pairs) of world item `item`, uint8 (n,) and float32 (n, 16), n = the item's node count."""
        n = C.c_int32(0)
        self._check(lib.srtTestGetTreeAux(self.h, item, None, None, 0, C.byref(n)))
        axis = np.zeros(n.value, np.uint8)
        pairs = np.zeros((n.value, 16), np.float32)
        self._check(lib.srtTestGetTreeAux(self.h, item, axis.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          pairs.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)))
        return axis, pairs

    def render_image(self, params, want_accum=True, want_rgba=True):
        W, H = params.imageWidth, params.imageHeight
        accum = np.zeros((H, W, 4), np.float32) if want_accum else None
        rgba = np.zeros((H, W, 4), np.uint8) if want_rgba else None
        self._check(lib.srtRenderImage(self.h, C.byref(params), accum.ctypes.data if want_accum else None,
                                       rgba.ctypes.data if want_rgba else None))
        return accum, rgba

    def render_direct_image(self, params, samples_per_batch=0, want_accum=True, want_rgba=True):
        """srtRenderDirectImage: the frame through camera_rays_device and trace_paths_device(direct=True), samples_per_batch
        sample indices at a time (0: a default that bounds memory), summed per pixel in sample-index order.  Returns
        (accum, rgba) as render_image does: another estimator of the same image -- with no sampled light in the scene and
        FAITHFUL steps, render_image's bytes."""
        W, H = params.imageWidth, params.imageHeight
        accum = np.zeros((H, W, 4), np.float32) if want_accum else None
        rgba = np.zeros((H, W, 4), np.uint8) if want_rgba else None
        self._check(lib.srtRenderDirectImage(self.h, C.byref(params), int(samples_per_batch),
                                             accum.ctypes.data_as(C.POINTER(C.c_float)) if want_accum else None,
                                             rgba.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgba else None))
        return accum, rgba

    def render_image_moments(self, params, want_accum=True, want_rgba=True):
        """render_image with the luminance moments of the samples (srtRenderImageMoments).  Returns (accum, moments, rgba):
        accum and rgba bit-identical to render_image's; moments (H, W, 4) float32 {sum l, sum l^2, 0, count}."""
        W, H = params.imageWidth, params.imageHeight
        accum = np.zeros((H, W, 4), np.float32) if want_accum else None
        moments = np.zeros((H, W, 4), np.float32)
        rgba = np.zeros((H, W, 4), np.uint8) if want_rgba else None
        self._check(lib.srtRenderImageMoments(self.h, C.byref(params), accum.ctypes.data if want_accum else None,
                                              moments.ctypes.data, rgba.ctypes.data if want_rgba else None))
        return accum, moments, rgba

    @staticmethod
    def _adaptive_stats(st):
        r = st.rounds
        return {"rounds": r, "pixelSamples": st.pixelSamples, "roundSpp": list(st.roundSpp[:r]),
                "roundTiles": list(st.roundTiles[:r]), "roundMs": list(st.roundMs[:r])}

    def render_adaptive(self, params, aparams, want_accum=True, want_moments=True, want_rgba=True):
        """Tile-adaptive sampling (srtRenderAdaptiveImage): round 0 renders params.spp samples everywhere, later rounds double
        the samples of the tiles whose pixels have not converged (include/srt_hip.h "Adaptive sampling").  Returns (accum,
        moments, rgba, stats): (H, W, 4) float32 sums with per-pixel counts w, the moments {sum l, sum l^2, 0, w}, uint8 RGBA
        (each None when not wanted), and a dict of SrtAdaptiveStats with the per-round lists cut to `rounds`."""
        W, H = params.imageWidth, params.imageHeight
        accum = np.zeros((H, W, 4), np.float32) if want_accum else None
        moments = np.zeros((H, W, 4), np.float32) if want_moments else None
        rgba = np.zeros((H, W, 4), np.uint8) if want_rgba else None
        st = abi.SrtAdaptiveStats()
        fp = C.POINTER(C.c_float)
        self._check(lib.srtRenderAdaptiveImage(self.h, C.byref(params), C.byref(aparams),
                                               accum.ctypes.data_as(fp) if want_accum else None,
                                               moments.ctypes.data_as(fp) if want_moments else None,
                                               rgba.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgba else None, C.byref(st)))
        return accum, moments, rgba, self._adaptive_stats(st)

    def render_adaptive_device(self, params, aparams, d_accum_ptr, d_moments_ptr, d_rgba_ptr=None, stream=None):
        """srtRenderAdaptive into DEVICE image-order buffers (float4[W*H] beauty and moments, both required; uint8[W*H*4]
        RGBA or None).  Returns the stats dict; the work has finished when it returns."""
        st = abi.SrtAdaptiveStats()
        self._check(lib.srtRenderAdaptive(self.h, C.byref(params), C.byref(aparams), d_accum_ptr, d_moments_ptr, d_rgba_ptr,
                                          C.byref(st), stream))
        return self._adaptive_stats(st)

    def render_adaptive_guided_device(self, params, aparams, planes, plane_ptrs, d_accum_ptr, d_moments_ptr, d_rgba_ptr=None,
                                      stream=None):
        """srtRenderAdaptiveGuided: render_adaptive_device whose guide planes follow the rounds.  plane_ptrs[k] = DEVICE
        image-order float4[W*H] for every selected bit 1 << k (None otherwise): sums over all of a pixel's samples with
        per-pixel counts.  Returns the stats dict; the work has finished when it returns."""
        arr = (_vp * 4)(*[(p if p else None) for p in list(plane_ptrs) + [None] * (4 - len(plane_ptrs))])
        st = abi.SrtAdaptiveStats()
        self._check(lib.srtRenderAdaptiveGuided(self.h, C.byref(params), C.byref(aparams), int(planes), arr, d_accum_ptr,
                                                d_moments_ptr, d_rgba_ptr, C.byref(st), stream))
        return self._adaptive_stats(st)

    def render_adaptive_denoised(self, params, aparams, dparams=None):
        """Adaptive render, guide planes from every sample and the moments-driven denoiser on one frame
        (srtRenderAdaptiveDenoisedImage).  Returns (accum, moments, denoised, rgba, stats): accum, moments and stats as
        render_adaptive's, denoised and rgba as render_denoised_moments's."""
        if dparams is None:
            dparams = abi.default_denoise_params()
        W, H = params.imageWidth, params.imageHeight
        accum, moments, denoised = (np.zeros((H, W, 4), np.float32) for _ in range(3))
        rgba = np.zeros((H, W, 4), np.uint8)
        st = abi.SrtAdaptiveStats()
        fp = C.POINTER(C.c_float)
        self._check(lib.srtRenderAdaptiveDenoisedImage(self.h, C.byref(params), C.byref(aparams), C.byref(dparams),
                                                       accum.ctypes.data_as(fp), moments.ctypes.data_as(fp),
                                                       denoised.ctypes.data_as(fp), rgba.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                       C.byref(st)))
        return accum, moments, denoised, rgba, self._adaptive_stats(st)

    def render_features(self, params, planes=abi.SRT_FEATURE_ALL):
        """Feature pass (include/srt_hip.h srtRenderFeatureImage): the first hit of the beauty render's camera rays.
        Returns {plane name: (H, W, 4) float32}, xyz = the mean over the samples that counted (0 where none did), w = their
        count, for every plane selected in `planes` (SRT_FEATURE_* bits; names in abi.FEATURE_PLANES)."""
        W, H = params.imageWidth, params.imageHeight
        out = {}
        ptrs = (C.POINTER(C.c_float) * 4)()
        for k, name in enumerate(abi.FEATURE_PLANES):
            if planes >> k & 1:
                out[name] = np.zeros((H, W, 4), np.float32)
                ptrs[k] = out[name].ctypes.data_as(C.POINTER(C.c_float))
        self._check(lib.srtRenderFeatureImage(self.h, C.byref(params), int(planes), ptrs))
        return out

    def render_feature_tiles(self, params, planes, ptrs, stream=None):
        """Asynchronous feature pass into DEVICE tile buffers: ptrs[k] = float4[numLocalTiles*64] for every selected bit
        1 << k (None otherwise)."""
        arr = (_vp * 4)(*[(p if p else None) for p in list(ptrs) + [None] * (4 - len(ptrs))])
        self._check(lib.srtRenderFeatureTiles(self.h, C.byref(params), int(planes), arr, stream))

    def render_feature_tile_list(self, params, planes, d_list_ptr, num_listed, plane_ptrs, accumulate=False, stream=None):
        """Asynchronous feature pass over a DEVICE tile list (srtRenderFeatureTileList): d_list_ptr = uint32[num_listed],
        tx | ty << 16 per tile; plane_ptrs[k] = DEVICE image-order float4[W*H] for every selected bit 1 << k (None
        otherwise), stored, or added to when `accumulate` is set."""
        arr = (_vp * 4)(*[(p if p else None) for p in list(plane_ptrs) + [None] * (4 - len(plane_ptrs))])
        self._check(lib.srtRenderFeatureTileList(self.h, C.byref(params), int(planes), d_list_ptr, int(num_listed), arr,
                                                 1 if accumulate else 0, stream))

    def denoise(self, dparams, width, height, d_beauty_ptr, plane_ptrs, d_out_ptr=None, d_rgba_ptr=None, stream=None,
                d_moments_ptr=None):
        """Asynchronous denoiser over DEVICE image-order buffers (include/srt_hip.h srtDenoise): d_beauty_ptr = float4[W*H]
        sums with counts, plane_ptrs[k] = the resolved feature plane of bit 1 << k (None where not given).
        d_moments_ptr: the resolved moments plane of srtRenderTilesMoments -> srtDenoiseMoments (the sample variance)."""
        arr = (_vp * 4)(*[(p if p else None) for p in list(plane_ptrs) + [None] * (4 - len(plane_ptrs))])
        if d_moments_ptr is None:
            self._check(lib.srtDenoise(self.h, C.byref(dparams), int(width), int(height), d_beauty_ptr, arr, d_out_ptr,
                                       d_rgba_ptr, stream))
        else:
            self._check(lib.srtDenoiseMoments(self.h, C.byref(dparams), int(width), int(height), d_beauty_ptr, arr,
                                              d_moments_ptr, d_out_ptr, d_rgba_ptr, stream))

    def denoise_scratch(self, width, height):
        """srtTestDenoiseScratch (include/srt_hip_test.h): what the last denoise of a width x height image left in the
        context's scratch.  Returns (guide, col0, col1, grad): (H, W, 4) {n.xyz, z}, two (H, W, 4) {e.rgb, v}, (H, W, 2)
        float32; after k + 1 levels col[k & 1] holds {e, v} after k levels."""
        guide, col0, col1 = (np.zeros((height, width, 4), np.float32) for _ in range(3))
        grad = np.zeros((height, width, 2), np.float32)
        fp = C.POINTER(C.c_float)
        self._check(lib.srtTestDenoiseScratch(self.h, int(width), int(height), guide.ctypes.data_as(fp), col0.ctypes.data_as(fp),
                                              col1.ctypes.data_as(fp), grad.ctypes.data_as(fp)))
        return guide, col0, col1, grad

    def render_denoised(self, params, dparams=None):
        """Beauty render, feature pass and denoiser of one frame (srtRenderDenoisedImage).  Returns (accum, denoised, rgba):
        (H, W, 4) float32 sums with counts, bit-identical to render_image's; (H, W, 4) float32, rgb = the denoised mean,
        w = the count; (H, W, 4) uint8 of the denoised mean."""
        if dparams is None:
            dparams = abi.default_denoise_params()
        W, H = params.imageWidth, params.imageHeight
        accum = np.zeros((H, W, 4), np.float32)
        denoised = np.zeros((H, W, 4), np.float32)
        rgba = np.zeros((H, W, 4), np.uint8)
        fp = C.POINTER(C.c_float)
        self._check(lib.srtRenderDenoisedImage(self.h, C.byref(params), C.byref(dparams), accum.ctypes.data_as(fp),
                                               denoised.ctypes.data_as(fp), rgba.ctypes.data_as(C.POINTER(C.c_uint8))))
        return accum, denoised, rgba

    def render_denoised_moments(self, params, dparams=None):
        """render_denoised with the sample variance (srtRenderDenoisedImageMoments).  Returns (accum, moments, denoised,
        rgba): accum bit-identical to render_image's, moments as render_image_moments's."""
        if dparams is None:
            dparams = abi.default_denoise_params()
        W, H = params.imageWidth, params.imageHeight
        accum, moments, denoised = (np.zeros((H, W, 4), np.float32) for _ in range(3))
        rgba = np.zeros((H, W, 4), np.uint8)
        fp = C.POINTER(C.c_float)
        self._check(lib.srtRenderDenoisedImageMoments(self.h, C.byref(params), C.byref(dparams), accum.ctypes.data_as(fp),
                                                      moments.ctypes.data_as(fp), denoised.ctypes.data_as(fp),
                                                      rgba.ctypes.data_as(C.POINTER(C.c_uint8))))
        return accum, moments, denoised, rgba

    def temporal_accumulate(self, tparams, width, height, d_beauty_ptr, d_moments_ptr, plane_ptrs, cam, prev_cam, d_history_in_ptr,
                            d_beauty_out_ptr, d_moments_out_ptr, d_history_out_ptr, stream=None, motion_ptr=None):
        """Asynchronous temporal accumulation over DEVICE image-order buffers (include/srt_hip.h srtTemporalAccumulate):
        reprojects the history written with prev_cam (None / NULL history: the first frame) onto cam and adds the current
        frame.  plane_ptrs[k] = the resolved feature plane of bit 1 << k; a history is
        abi.SRT_TEMPORAL_HISTORY_BYTES_PER_PIXEL bytes per pixel.  motion_ptr: the resolved motion plane of
        render_motion_tiles (DEVICE float4[W*H]) -> srtTemporalAccumulateMotion, the motion-aware reprojection."""
        arr = (_vp * 4)(*[(p if p else None) for p in list(plane_ptrs) + [None] * (4 - len(plane_ptrs))])
        prev = C.byref(prev_cam) if prev_cam is not None else None
        if motion_ptr is None:
            self._check(lib.srtTemporalAccumulate(self.h, C.byref(tparams), int(width), int(height), d_beauty_ptr, d_moments_ptr,
                                                  arr, C.byref(cam), prev, d_history_in_ptr, d_beauty_out_ptr,
                                                  d_moments_out_ptr, d_history_out_ptr, stream))
        else:
            self._check(lib.srtTemporalAccumulateMotion(self.h, C.byref(tparams), int(width), int(height), d_beauty_ptr,
                                                        d_moments_ptr, arr, motion_ptr, C.byref(cam), prev, d_history_in_ptr,
                                                        d_beauty_out_ptr, d_moments_out_ptr, d_history_out_ptr, stream))

    def render_temporal_frame(self, params, dparams=None, tparams=None, want_stats=True):
        """One frame of a sequence (srtRenderTemporalFrame): render with the camera currently set, accumulate onto the history
        the context kept from the previous call, denoise.  Returns (accum, denoised, rgba, stats): accum = this frame's own
        sums, bit-identical to render_image's; stats = {"historyPixels", "meanHistoryCount"} or None."""
        dparams = abi.default_denoise_params() if dparams is None else dparams
        tparams = abi.default_temporal_params() if tparams is None else tparams
        W, H = params.imageWidth, params.imageHeight
        accum, denoised = (np.zeros((H, W, 4), np.float32) for _ in range(2))
        rgba = np.zeros((H, W, 4), np.uint8)
        st = abi.SrtTemporalStats()
        fp = C.POINTER(C.c_float)
        self._check(lib.srtRenderTemporalFrame(self.h, C.byref(params), C.byref(dparams), C.byref(tparams), accum.ctypes.data_as(fp),
                                               denoised.ctypes.data_as(fp), rgba.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               C.byref(st) if want_stats else None))
        stats = {"historyPixels": int(st.historyPixels), "meanHistoryCount": float(st.meanHistoryCount)} if want_stats else None
        return accum, denoised, rgba, stats

    def temporal_reset(self):
        """Drops the history srtRenderTemporalFrame keeps: the next frame starts over."""
        self._check(lib.srtTemporalReset(self.h))

    def temporal_reproject(self, tparams, width, height, plane_ptrs, cam, prev_cam, d_history_in_ptr, d_reprojected_ptr,
                           stream=None, motion_ptr=None):
        """srtTemporalReproject: the reprojected history h of temporal_accumulate, written once into DEVICE float4[2][W*H]
        ({h.r, h.g, h.b, h.count} and {h.S1, h.S2, 0, has}); None / NULL history gives zeros.  motion_ptr as
        temporal_accumulate's -> srtTemporalReprojectMotion."""
        arr = (_vp * 4)(*[(p if p else None) for p in list(plane_ptrs) + [None] * (4 - len(plane_ptrs))])
        prev = C.byref(prev_cam) if prev_cam is not None else None
        if motion_ptr is None:
            self._check(lib.srtTemporalReproject(self.h, C.byref(tparams), int(width), int(height), arr, C.byref(cam), prev,
                                                 d_history_in_ptr, d_reprojected_ptr, stream))
        else:
            self._check(lib.srtTemporalReprojectMotion(self.h, C.byref(tparams), int(width), int(height), arr, motion_ptr,
                                                       C.byref(cam), prev, d_history_in_ptr, d_reprojected_ptr, stream))

    @classmethod
    def _temporal_adaptive_stats(cls, st):
        out = cls._adaptive_stats(st.adaptive)
        out.update(historyPixels=int(st.temporal.historyPixels), meanHistoryCount=float(st.temporal.meanHistoryCount))
        return out

    def render_temporal_adaptive_device(self, params, aparams, tparams, plane_ptrs, prev_cam, d_history_in_ptr, d_accum_ptr,
                                        d_moments_ptr, d_beauty_out_ptr, d_moments_out_ptr, d_history_out_ptr, stream=None,
                                        entry=None):
        """srtRenderTemporalAdaptive over DEVICE image-order buffers with the camera currently set: adaptive rounds that
        decide on the frame's moments pooled with the reprojected history, then temporal_accumulate of the final sums.
        Returns render_adaptive's stats dict plus "historyPixels" and "meanHistoryCount"; the work has finished."""
        arr = (_vp * 4)(*[(p if p else None) for p in list(plane_ptrs) + [None] * (4 - len(plane_ptrs))])
        st = abi.SrtTemporalAdaptiveStats()
        entry = lib.srtRenderTemporalAdaptive if entry is None else entry
        self._check(entry(self.h, C.byref(params), C.byref(aparams), C.byref(tparams), arr,
                          C.byref(prev_cam) if prev_cam is not None else None, d_history_in_ptr, d_accum_ptr, d_moments_ptr,
                          d_beauty_out_ptr, d_moments_out_ptr, d_history_out_ptr, C.byref(st), stream))
        return self._temporal_adaptive_stats(st)

    def render_temporal_adaptive_guided_device(self, params, aparams, tparams, plane_ptrs, prev_cam, d_history_in_ptr, d_accum_ptr,
                                               d_moments_ptr, d_beauty_out_ptr, d_moments_out_ptr, d_history_out_ptr, stream=None):
        """srtRenderTemporalAdaptiveGuided: render_temporal_adaptive_device whose rounds extend the planes in plane_ptrs (in:
        the first params.spp samples; out: all of a pixel's samples); the closing accumulation reads the extended planes."""
        return self.render_temporal_adaptive_device(params, aparams, tparams, plane_ptrs, prev_cam, d_history_in_ptr, d_accum_ptr,
                                                    d_moments_ptr, d_beauty_out_ptr, d_moments_out_ptr, d_history_out_ptr, stream,
                                                    entry=lib.srtRenderTemporalAdaptiveGuided)

    def render_temporal_adaptive_frame(self, params, aparams, dparams=None, tparams=None, guided=False):
        """One frame of a sequence with history-steered sampling (srtRenderTemporalAdaptiveFrame); interleaves with
        render_temporal_frame on one context.  Returns (accum, denoised, rgba, stats): accum = this frame's own sums with
        per-pixel counts; stats as render_temporal_adaptive_device's.  Advance params.sampleFirst by aparams.sppMax.
        guided: srtRenderTemporalAdaptiveGuidedFrame, the guide planes follow the rounds."""
        dparams = abi.default_denoise_params() if dparams is None else dparams
        tparams = abi.default_temporal_params() if tparams is None else tparams
        W, H = params.imageWidth, params.imageHeight
        accum, denoised = (np.zeros((H, W, 4), np.float32) for _ in range(2))
        rgba = np.zeros((H, W, 4), np.uint8)
        st = abi.SrtTemporalAdaptiveStats()
        fp = C.POINTER(C.c_float)
        entry = lib.srtRenderTemporalAdaptiveGuidedFrame if guided else lib.srtRenderTemporalAdaptiveFrame
        self._check(entry(self.h, C.byref(params), C.byref(aparams), C.byref(dparams), C.byref(tparams), accum.ctypes.data_as(fp),
                          denoised.ctypes.data_as(fp), rgba.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st)))
        return accum, denoised, rgba, self._temporal_adaptive_stats(st)

    def render_tiles(self, params, d_accum_ptr, stream=None):
        self._check(lib.srtRenderTiles(self.h, C.byref(params), d_accum_ptr, stream))

    def render_tiles_moments(self, params, d_accum_ptr, d_moments_ptr, stream=None):
        """srtRenderTilesMoments: render_tiles (bit-identical accumulators) plus the moments plane, DEVICE
        float4[numLocalTiles*64] {sum l, sum l^2, 0, count} in the tiles' layout."""
        self._check(lib.srtRenderTilesMoments(self.h, C.byref(params), d_accum_ptr, d_moments_ptr, stream))

    def resolve_tiles(self, params, d_gathered_ptr, d_rgba_ptr=None, d_accum_image_ptr=None, stream=None):
        self._check(lib.srtResolveTiles(self.h, C.byref(params), d_gathered_ptr, d_rgba_ptr, d_accum_image_ptr, stream))

    def comm_init(self, unique_id, num_ranks, rank):
        self._check(lib.srtCommInit(self.h, C.c_char_p(unique_id), num_ranks, rank))

    def gather_tiles(self, params, d_local_ptr, d_gathered_ptr=None, stream=None):
        """The path's one collective: ncclGather of the ranks' tile buffers to rank 0 (srt_comm.cpp)."""
        self._check(lib.srtGatherTiles(self.h, C.byref(params), d_local_ptr, d_gathered_ptr, stream))

    def render_image_ranks(self, params, want_accum=True, want_rgba=True):
        """Collective blocking render across the communicator's ranks; rank 0 gets the image."""
        W, H = params.imageWidth, params.imageHeight
        accum = np.zeros((H, W, 4), np.float32) if want_accum else None
        rgba = np.zeros((H, W, 4), np.uint8) if want_rgba else None
        self._check(lib.srtRenderImageRanks(self.h, C.byref(params), accum.ctypes.data if want_accum else None,
                                            rgba.ctypes.data if want_rgba else None))
        return accum, rgba

    def comm_destroy(self):
        self._check(lib.srtCommDestroy(self.h))

    def _update(self, host_entry, device_entry, dtype, first, records, stream):
        size = dtype.itemsize
        if hasattr(records, "data_ptr"):  # a torch tensor: DEVICE memory, handed over as it is
            if not records.is_cuda or not records.is_contiguous():
                raise ValueError("a tensor of records must be contiguous and live on the GPU")
            nbytes = records.numel() * records.element_size()
            if nbytes % size:
                raise ValueError("the tensor holds %d bytes, not a whole number of %d-byte records" % (nbytes, size))
            self._check(device_entry(self.h, int(first), nbytes // size, records.data_ptr() if nbytes else None, stream))
            return
        a = np.ascontiguousarray(records)
        if a.dtype != dtype:
            if a.nbytes % size:
                raise ValueError("the array holds %d bytes, not a whole number of %d-byte records" % (a.nbytes, size))
            a = a.reshape(-1).view(np.uint8).view(dtype)
        self._check(host_entry(self.h, int(first), a.size, a.ctypes.data if a.size else None))

    def update_triangles(self, first, triangles, stream=None):
        """srtUpdateTriangles / srtUpdateTrianglesDevice: new positions and uvs for triangles [first, first + n) of the
        uploaded scene (its own triangle order; `material` is ignored).  triangles: a NumPy array of abi.TRIANGLE_DTYPE
        (or any array of n * 64 bytes laid out like SrtTriangleIn), or a contiguous torch tensor on the GPU with the same
        bytes, which is read asynchronously on `stream`.  Nothing renders until refit() has run."""
        self._update(lib.srtUpdateTriangles, lib.srtUpdateTrianglesDevice, abi.TRIANGLE_DTYPE, first, triangles, stream)

    def update_spheres(self, first, spheres, stream=None):
        """srtUpdateSpheres / srtUpdateSpheresDevice: new centres, times and radius for spheres [first, first + n); records
        of abi.SPHERE_DTYPE (40 bytes, SrtSphereIn), NumPy or a torch tensor on the GPU as in update_triangles."""
        self._update(lib.srtUpdateSpheres, lib.srtUpdateSpheresDevice, abi.SPHERE_DTYPE, first, spheres, stream)

    def refit(self, stream=None):
        """srtRefitScene: every node box from the current primitive records, and what is derived from boxes; the topology
        stays.  Blocking.  Drops the temporal history unless motion tracking is on."""
        self._check(lib.srtRefitScene(self.h, stream))

    def rebuild(self, stream=None):
        """srtRebuildScene: refit(), except that every tree the upload built on the device (LBVH, PLOC) is built anew from
        the current primitive records, as an upload of the moved scene would build it; PLOC's radius is the upload's.
        Blocking; ordered behind `stream`.  Counts as a refit for the temporal history."""
        self._check(lib.srtRebuildScene(self.h, stream))

    def tree_cost(self, item=0):
        """srtGetTreeCost: the sum of world item `item`'s node box areas over its root's, a float64 defined bit for bit
        (include/srt_hip.h).  Compare the value after a refit with the value at the build to decide on a rebuild()."""
        cost = C.c_double(0.0)
        self._check(lib.srtGetTreeCost(self.h, int(item), C.byref(cost)))
        return cost.value

    def set_motion_tracking(self, enable=True):
        """srtSetMotionTracking: keep the geometry of the previous refit (48 B per triangle and per sphere) so that
        render_motion has a displacement to report and render_temporal_frame keeps its history across one update + refit.
        Call order: enable, upload, then per frame update_*, refit, render_temporal_frame."""
        self._check(lib.srtSetMotionTracking(self.h, 1 if enable else 0))

    def render_motion(self, params):
        """Motion pass (srtRenderMotionImage): (H, W, 4) float32, xyz = the mean displacement from the first hit of the
        pixel's camera rays to where that surface point was at the previous refit (0 where nothing was hit), w = the
        hit count."""
        out = np.zeros((params.imageHeight, params.imageWidth, 4), np.float32)
        self._check(lib.srtRenderMotionImage(self.h, C.byref(params), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def render_motion_tiles(self, params, d_motion_ptr, stream=None):
        """Asynchronous motion pass into a DEVICE tile buffer float4[numLocalTiles*64] (sums with counts), laid out as
        render_feature_tiles's planes: resolve_tiles / gather_tiles take it unchanged."""
        self._check(lib.srtRenderMotionTiles(self.h, C.byref(params), d_motion_ptr, stream))

    def trace(self, rays, traversal=abi.SRT_TRAVERSE_FAITHFUL):
        rays = np.ascontiguousarray(rays, abi.RAY_DTYPE)
        hits = np.zeros(len(rays), abi.HIT_DTYPE)
        self._check(lib.srtTraceRays(self.h, rays.ctypes.data, len(rays), hits.ctypes.data, traversal))
        return hits

    @staticmethod
    def _device_rays(rays):
        """The rays of a device query: a contiguous float32 torch tensor (n, 9) on the GPU, laid out as SrtRay."""
        if not hasattr(rays, "data_ptr") or not hasattr(rays, "is_cuda"):
            raise ValueError("rays must be a torch tensor on the GPU (for host arrays there is trace())")
        if str(rays.dtype) != "torch.float32":
            raise ValueError("rays must be float32, not %s" % rays.dtype)
        if rays.dim() != 2 or rays.shape[1] != 9:
            raise ValueError("rays must have shape (n, 9) (o, d, time, tMin, tMax), not %s" % (tuple(rays.shape),))
        if not rays.is_contiguous():
            raise ValueError("rays must be contiguous")
        if not rays.is_cuda:
            raise ValueError("rays must live on the GPU, not on %s" % rays.device)
        return rays

    @staticmethod
    def _stream_handle(stream):
        """None (the NULL stream), a raw hipStream_t as an integer, or a torch stream."""
        return getattr(stream, "cuda_stream", stream)

    @staticmethod
    def _ptr(t, n=1):
        """The device address of a tensor for a C call: None (NULL) for no tensor, and for any tensor of a call on n = 0 entries."""
        return t.data_ptr() if t is not None and n else None

    def trace_device(self, rays, traversal=abi.SRT_TRAVERSE_CLOSEST, records=False, stream=None):
        """srtTraceRaysDevice: the hit of every ray of a DEVICE tensor, asynchronous on `stream`.  rays: contiguous float32
        (n, 9) on the GPU, one SrtRay per row.  Returns an int32 tensor (n, 4) laid out as SrtRayHit {prim, t's bits,
        material, frontFace} (column 1 viewed as float32 is t); with records=True also an int32 tensor (n, 22) laid out as
        SrtHit, its counters 0.  The outputs are allocated with torch on the rays' device: call this inside
        `with torch.cuda.stream(s)` when `stream` is s, so that the allocator knows the stream that uses them.
        CLOSEST is the tree-independent closest hit, ties to the largest prims[] index; triangles are one-sided; a ray's
        time must lie inside every world item's range (include/srt_hip.h "Ray queries")."""
        import torch
        rays = self._device_rays(rays)
        n = rays.shape[0]
        hits = torch.empty((n, 4), dtype=torch.int32, device=rays.device)
        recs = torch.empty((n, C.sizeof(abi.SrtHit) // 4), dtype=torch.int32, device=rays.device) if records else None
        self._check(lib.srtTraceRaysDevice(self.h, rays.data_ptr() if n else None, n, int(traversal),
                                           hits.data_ptr() if n else None, recs.data_ptr() if records and n else None,
                                           self._stream_handle(stream)))
        return (hits, recs) if records else hits

    def occluded_device(self, rays, stream=None):
        """srtOccludedDevice: a torch.uint8 tensor (n,), 1 where anything lies in a ray's (tMin, tMax); rays and stream as
        trace_device's.  The any-hit walk leaves at the first primitive in the way."""
        import torch
        rays = self._device_rays(rays)
        n = rays.shape[0]
        out = torch.empty((n,), dtype=torch.uint8, device=rays.device)
        self._check(lib.srtOccludedDevice(self.h, rays.data_ptr() if n else None, n, out.data_ptr() if n else None,
                                          self._stream_handle(stream)))
        return out

    @staticmethod
    def _device_tensor(t, what, dtype, shape, like=None):
        """A buffer of a path step: a contiguous torch tensor on the GPU of this dtype and shape (-1: any); `like`: on the same
        device as that tensor."""
        if not hasattr(t, "data_ptr") or not hasattr(t, "is_cuda"):
            raise ValueError("%s must be a torch tensor on the GPU" % what)
        if str(t.dtype) != "torch." + dtype:
            raise ValueError("%s must be %s, not %s" % (what, dtype, t.dtype))
        if t.dim() != len(shape) or any(want >= 0 and got != want for got, want in zip(t.shape, shape)):
            raise ValueError("%s must have shape %s, not %s" % (what, tuple("n" if s < 0 else s for s in shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % what)
        if not t.is_cuda:
            raise ValueError("%s must live on the GPU, not on %s" % (what, t.device))
        if like is not None and t.device != like.device:
            raise ValueError("%s must live on the GPU of the rays (%s), not on %s" % (what, like.device, t.device))
        return t

    def camera_rays_device(self, params, pixel_sample=None, device=None, stream=None):
        """srtCameraRaysDevice: the camera ray the renders trace for every (pixel, sample) entry, and the generator state
        after its draws, asynchronous on `stream`.  pixel_sample: a contiguous int32 tensor (n, 2) on the GPU holding
        {pixel index y * W + x, absolute sample index}, or None for every sample of the frame (entry i = pixel i // spp,
        sample sampleFirst + i % spp; `device` then names the GPU, default the current one).  Returns (rays, rng): float32
        (n, 9) laid out as SrtRay with tMin = params.tMin and tMax = +inf, and int64 (n,) holding the 64-bit states.  An
        entry whose pixel lies outside the image is left as torch.empty made it."""
        import torch
        if pixel_sample is None:
            n = params.imageWidth * params.imageHeight * params.spp
            device = torch.device("cuda" if device is None else device)
        else:
            pixel_sample = self._device_tensor(pixel_sample, "pixel_sample", "int32", (-1, 2))
            n, device = pixel_sample.shape[0], pixel_sample.device
        rays = torch.empty((n, 9), dtype=torch.float32, device=device)
        rng = torch.empty((n,), dtype=torch.int64, device=device)
        self._check(lib.srtCameraRaysDevice(self.h, C.byref(params), pixel_sample.data_ptr() if pixel_sample is not None and n else None,
                                            n, rays.data_ptr() if n else None, rng.data_ptr() if n else None,
                                            self._stream_handle(stream)))
        return rays, rng

    def scatter_device(self, rays, records, rng, rays_out=None, stream=None):
        """srtScatterRaysDevice: material::scatter and material::emitted on every (ray, hit record) pair, asynchronous on
        `stream`.  rays: float32 (n, 9); records: int32 (n, 22) as trace_device(records=True) returns them; rng: int64 (n,),
        the generator states, advanced IN PLACE by the draws made; rays_out: float32 (n, 9) that receives the scattered
        rays (may be `rays` itself; allocated when None -- rows that did not scatter then hold whatever torch.empty left).
        Returns (out, rays_out): out int32 (n, 8) laid out as SrtPathOut {attenuation's bits[3], status, emitted's
        bits[3], prim} (out.view(torch.float32) for the colours; status is one of abi.SRT_PATH_*)."""
        import torch
        rays = self._device_rays(rays)
        n = rays.shape[0]
        records = self._device_tensor(records, "records", "int32", (n, C.sizeof(abi.SrtHit) // 4), rays)
        rng = self._device_tensor(rng, "rng", "int64", (n,), rays)
        rays_out = torch.empty_like(rays) if rays_out is None else self._device_tensor(rays_out, "rays_out", "float32", (n, 9), rays)
        out = torch.empty((n, 8), dtype=torch.int32, device=rays.device)
        ptr = self._ptr
        self._check(lib.srtScatterRaysDevice(self.h, ptr(rays, n), ptr(records, n), n, ptr(rng, n), ptr(out, n), ptr(rays_out, n),
                                             self._stream_handle(stream)))
        return out, rays_out

    def path_step_device(self, rays, rng, traversal=abi.SRT_TRAVERSE_CLOSEST, active=None, rays_out=None, hits=False, stream=None):
        """srtPathStepDevice: one bounce in one kernel -- trace_device followed by scatter_device on its records, byte for
        byte, without the records' round trip through memory.  rays, rng, rays_out and the returned out as scatter_device's;
        active: uint8 (n,), entries with a 0 are neither read nor written (None: all).  Returns (out, rays_out), with
        hits=True (out, rays_out, hits), hits as trace_device returns them.  Rows of inactive entries in a tensor allocated
        here hold whatever torch.empty left."""
        import torch
        rays = self._device_rays(rays)
        n = rays.shape[0]
        rng = self._device_tensor(rng, "rng", "int64", (n,), rays)
        if active is not None:
            active = self._device_tensor(active, "active", "uint8", (n,), rays)
        rays_out = torch.empty_like(rays) if rays_out is None else self._device_tensor(rays_out, "rays_out", "float32", (n, 9), rays)
        out = torch.empty((n, 8), dtype=torch.int32, device=rays.device)
        d_hits = torch.empty((n, 4), dtype=torch.int32, device=rays.device) if hits else None
        ptr = self._ptr
        self._check(lib.srtPathStepDevice(self.h, int(traversal), ptr(rays, n), n, ptr(active, n), ptr(rng, n), ptr(out, n),
                                          ptr(rays_out, n), ptr(d_hits, n), self._stream_handle(stream)))
        return (out, rays_out, d_hits) if hits else (out, rays_out)

    def _path_payloads(self, n, first, rays, rng, slot, rays_out, rng_out, slot_out, active_out, slots, count, scratch, need):
        """What compact_paths_device and sort_paths_device share behind their predicates: rng and slot validated against n
        rows on the device of `first`; rays_out and rng_out allocated beside a given input or validated (an output without
        its input is refused); slot_out allocated when `slots` or a slot came in; active_out a tensor, True to allocate, or
        None; the scratch allocated or checked against `need` bytes; count allocated or validated, and zeroed for n == 0
        (the entry does not write the count of nothing).  Returns (rng, slot, (rays_out, rng_out, slot_out, active_out),
        count, scratch): the four outputs in the order of the C arguments and of the tuple both methods return."""
        import torch
        if rng is not None:
            rng = self._device_tensor(rng, "rng", "int64", (n,), first)
        if slot is not None:
            slot = self._device_tensor(slot, "slot", "int32", (n,), first)
        for name, given, source in (("rays_out", rays_out, rays), ("rng_out", rng_out, rng)):
            if given is not None and source is None:
                raise ValueError("%s without %s" % (name, name[:-4]))
        if rays is not None:
            rays_out = torch.empty_like(rays) if rays_out is None else self._device_tensor(rays_out, "rays_out", "float32", (n, 9), first)
        if rng is not None:
            rng_out = torch.empty_like(rng) if rng_out is None else self._device_tensor(rng_out, "rng_out", "int64", (n,), first)
        if slot_out is not None:
            slot_out = self._device_tensor(slot_out, "slot_out", "int32", (n,), first)
        elif slots or slot is not None:
            slot_out = torch.empty((n,), dtype=torch.int32, device=first.device)
        if active_out is True:
            active_out = torch.empty((n,), dtype=torch.uint8, device=first.device)
        elif active_out is not None and active_out is not False:
            active_out = self._device_tensor(active_out, "active_out", "uint8", (n,), first)
        else:
            active_out = None
        if scratch is None:
            scratch = torch.empty((max(need, 8),), dtype=torch.uint8, device=first.device)
        else:
            scratch = self._device_tensor(scratch, "scratch", "uint8", (-1,), first)
            if scratch.shape[0] < need:
                raise ValueError("scratch must hold %d bytes, not %d" % (need, scratch.shape[0]))
        if count is None:
            count = torch.empty((1,), dtype=torch.int64, device=first.device)
        else:
            count = self._device_tensor(count, "count", "int64", (1,), first)
        if n == 0:
            count.zero_()
        return rng, slot, (rays_out, rng_out, slot_out, active_out), count, scratch

    def compact_paths_device(self, out=None, active=None, rays=None, rng=None, slot=None, rays_out=None, rng_out=None, slot_out=None,
                             active_out=None, slots=True, count=None, scratch=None, stream=None):
        """srtCompactPathsDevice: the entries that go on, moved in their order to the front of fresh buffers, asynchronous on
        `stream`.  Kept are the entries whose `out` row (int32 (n, 8), as a step returns it) says SCATTERED and whose `active`
        byte (uint8 (n,)) is not 0; either may be None, not both -- pass the mask of the step that wrote `out`, because an
        inactive entry's row is stale.  rays float32 (n, 9), rng int64 (n,), slot int32 (n,): the payloads, each optional;
        *_out: where the kept rows go (allocated at n rows when None and the input is given; none may be an input).
        slots: also return the index every kept entry had (`slot` carried through, the identity without one).  active_out:
        a uint8 (n,) tensor that receives i < count (it may be `active` itself), or True to allocate one.  count: an int64
        tensor of one element to receive the number kept; scratch: uint8, at least compact_scratch_bytes(n).
        Returns (rays_out, rng_out, slot_out, active_out, count): None where nothing was asked for, rows behind count as
        they were, count a 0-dim int64 tensor on the GPU (reading it synchronises)."""
        first = None
        if rays is not None:
            first = rays = self._device_rays(rays)
        if out is not None:
            out = self._device_tensor(out, "out", "int32", (-1, 8), first)
            first = out if first is None else first
        if active is not None:
            active = self._device_tensor(active, "active", "uint8", (-1,), first)
            first = active if first is None else first
        if out is None and active is None:
            raise ValueError("out and active must not both be None: one of them is the predicate")
        n = (out if out is not None else active).shape[0]
        for name, t in (("rays", rays), ("out", out), ("active", active)):
            if t is not None and t.shape[0] != n:
                raise ValueError("%s must have %d rows like the predicate, not %d" % (name, n, t.shape[0]))
        rng, slot, outs, count, scratch = self._path_payloads(n, first, rays, rng, slot, rays_out, rng_out, slot_out, active_out, slots,
                                                              count, scratch, self.compact_scratch_bytes(n))
        if n:
            ptr = self._ptr
            self._check(lib.srtCompactPathsDevice(self.h, n, ptr(out), ptr(active), ptr(rays), ptr(rng), ptr(slot), *map(ptr, outs),
                                                  ptr(count), ptr(scratch), self._stream_handle(stream)))
        return outs + (count.reshape(()),)

    @staticmethod
    def compact_scratch_bytes(n):
        """srtCompactPathsScratchBytes: 8 bytes per tile of abi.SRT_COMPACT_TILE entries, 0 for n <= 0."""
        return int(lib.srtCompactPathsScratchBytes(int(n)))

    def sort_paths_device(self, cell_bits, rays=None, out=None, active=None, box=None, rng=None, slot=None, rays_out=None, rng_out=None,
                          slot_out=None, active_out=None, slots=True, count=None, scratch=None, stream=None):
        """srtSortPathsDevice: compact_paths_device with an order -- the entries that go on, moved to the front of fresh
        buffers and stably sorted by (Morton cell of the origin in `box` at cell_bits bits per axis, octant of the
        direction), asynchronous on `stream`.  rays is required (the key reads it); out and active are compact_paths_device's
        predicate, and here both may be None: every entry is then kept.  box: a float32 tensor (6,) on the GPU holding
        lo.xyz, hi.xyz; None computes it from the kept rays' origins with torch ops on `stream` (a torch stream or None,
        torch's current one) and reads nothing back.  Everything else, and the returned tuple (rays_out, rng_out, slot_out,
        active_out, count), is compact_paths_device's; scratch: uint8, at least sort_scratch_bytes(n)."""
        import torch
        cell_bits = int(cell_bits)
        if not 1 <= cell_bits <= abi.SRT_SORT_MAX_CELL_BITS:
            raise ValueError("cell_bits must lie in [1, %d], not %d" % (abi.SRT_SORT_MAX_CELL_BITS, cell_bits))
        if rays is None:
            raise ValueError("rays must not be None: the key is made of them")
        if rng_out is not None and rng is None:
            raise ValueError("rng_out without rng")
        if box is None and stream is not None and not hasattr(stream, "cuda_stream"):
            raise ValueError("box=None runs torch ops on the stream: pass a torch stream or a box")
        first = rays = self._device_rays(rays)
        n = rays.shape[0]
        if n > 2 ** 31 - 1:
            raise ValueError("n = %d does not fit a 32-bit index" % n)
        if out is not None:
            out = self._device_tensor(out, "out", "int32", (-1, 8), first)
        if active is not None:
            active = self._device_tensor(active, "active", "uint8", (-1,), first)
        for name, t in (("out", out), ("active", active)):
            if t is not None and t.shape[0] != n:
                raise ValueError("%s must have %d rows like the rays, not %d" % (name, n, t.shape[0]))
        if box is not None:
            box = self._device_tensor(box, "box", "float32", (6,), first)
        rng, slot, outs, count, scratch = self._path_payloads(n, first, rays, rng, slot, rays_out, rng_out, slot_out, active_out, slots,
                                                              count, scratch, self.sort_scratch_bytes(n))
        if n:
            if box is None:
                with torch.cuda.stream(stream):
                    box = self.origin_box(rays, out, active)
            ptr = self._ptr
            self._check(lib.srtSortPathsDevice(self.h, n, cell_bits, ptr(box), ptr(out), ptr(active), ptr(rays), ptr(rng), ptr(slot),
                                               *map(ptr, outs), ptr(count), ptr(scratch), scratch.shape[0], self._stream_handle(stream)))
        return outs + (count.reshape(()),)

    @staticmethod
    def origin_box(rays, out=None, active=None):
        """The box sort_paths_device makes with box=None: lo.xyz, hi.xyz over the origins of the kept rows of `rays`, a
        float32 tensor (6,) made with torch ops on torch's current stream, nothing read back.  No kept row: lo = +inf,
        hi = -inf, which the key's rule takes like any other box."""
        import torch
        origins = rays[:, 0:3]
        low = high = origins
        if out is not None or active is not None:
            keep = torch.ones((rays.shape[0],), dtype=torch.bool, device=rays.device)
            if active is not None:
                keep &= active != 0
            if out is not None:
                keep &= out[:, 3] == abi.SRT_PATH_SCATTERED
            low = torch.where(keep[:, None], origins, float("inf"))
            high = torch.where(keep[:, None], origins, float("-inf"))
        return torch.cat((low.amin(0), high.amax(0))).contiguous()

    @staticmethod
    def sort_scratch_bytes(n):
        """srtSortPathsScratchBytes: 0 for n <= 0, never smaller for a larger n."""
        return int(lib.srtSortPathsScratchBytes(int(n)))

    def sampled_lights(self):
        """srtGetSampledLights: the prims[] indices of the spheres direct light sampling chooses from (light materials with
        a solid-colour emit texture), an int32 array in prims[] order."""
        count = C.c_int32(0)
        self._check(lib.srtGetSampledLights(self.h, None, 0, C.byref(count)))
        prims = np.zeros(count.value, np.int32)
        self._check(lib.srtGetSampledLights(self.h, prims.ctypes.data_as(C.POINTER(C.c_int32)), count.value, C.byref(count)))
        return prims

    def direct_light_device(self, rays, records, rng, traversal=abi.SRT_TRAVERSE_CLOSEST, stream=None):
        """srtDirectLightDevice: the direct-light term of every (ray, hit record) pair, asynchronous on `stream`: one sampled
        light is chosen per pbr hit, a direction inside its cone drawn, the shadow ray walked with `traversal`.  rays,
        records and rng as scatter_device's; rng is only READ (the states before the hits' scatter draws: call this ahead
        of scatter_device).  Returns an int32 tensor (n, 8) laid out as SrtDirectOut {radiance's bits[3], light, dir's
        bits[3], weight's bits} (abi.DIRECT_OUT_DTYPE on the host); light is a prims[] index, -1 where nothing was sampled."""
        import torch
        rays = self._device_rays(rays)
        n = rays.shape[0]
        records = self._device_tensor(records, "records", "int32", (n, C.sizeof(abi.SrtHit) // 4), rays)
        rng = self._device_tensor(rng, "rng", "int64", (n,), rays)
        direct = torch.empty((n, 8), dtype=torch.int32, device=rays.device)
        ptr = self._ptr
        self._check(lib.srtDirectLightDevice(self.h, int(traversal), ptr(rays, n), ptr(records, n), n, ptr(rng, n), ptr(direct, n),
                                             self._stream_handle(stream)))
        return direct

    def eval_scatter_test(self, rays, records, dirs):
        """srtTestEvalScatterDevice: pbr's attenuation for the directions dirs (n, 3) float32 on the GPU, on the NULL stream:
        float32 (n, 3), 0 for entries that are not pbr hits."""
        import torch
        rays = self._device_rays(rays)
        n = rays.shape[0]
        records = self._device_tensor(records, "records", "int32", (n, C.sizeof(abi.SrtHit) // 4), rays)
        dirs = self._device_tensor(dirs, "dirs", "float32", (n, 3), rays)
        att = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
        ptr = self._ptr
        self._check(lib.srtTestEvalScatterDevice(self.h, ptr(rays, n), ptr(records, n), ptr(dirs, n), n, ptr(att, n)))
        return att

    def trace_paths_device(self, rays, rng, max_bounce, background, traversal=abi.SRT_TRAVERSE_CLOSEST, scratch=None, stream=None,
                           direct=False):
        """srtTracePathsDevice: the path-traced radiance of every ray of a DEVICE tensor in one kernel, asynchronous on
        `stream` -- at most max_bounce steps of path_step_device per ray, each on the scattered ray of the step before,
        then the unwinding; no tensor per bounce and no count read back.  rays: float32 (n, 9), only read; rng: int64 (n,),
        the generator states, advanced IN PLACE to the state after each path's last draw; background: three floats, the
        radiance of a ray that leaves the scene; scratch: a uint8 tensor of at least abi.SRT_PATHS_SCRATCH_BYTES bytes
        (allocated when None; calls on one stream may share one).  Returns an int32 tensor (n, 4) laid out as
        SrtPathRadiance: columns 0..2 viewed as float32 are the radiance, column 3 holds the number of steps that ran in
        its low 16 bits and the last step's abi.SRT_PATH_* status in its high 16 (result.view(torch.int16)[:, 6] and
        [:, 7]; SCATTERED: the bounce limit ended the path).  direct=True: srtTracePathsDirectDevice -- the same paths with
        the direct-light term of direct_light_device added at every pbr hit; steps, status and rng are the same."""
        import torch
        rays = self._device_rays(rays)
        n = rays.shape[0]
        rng = self._device_tensor(rng, "rng", "int64", (n,), rays)
        if scratch is None:
            scratch = torch.empty((abi.SRT_PATHS_SCRATCH_BYTES,), dtype=torch.uint8, device=rays.device)
        else:
            scratch = self._device_tensor(scratch, "scratch", "uint8", (-1,), rays)
            if scratch.shape[0] < abi.SRT_PATHS_SCRATCH_BYTES:
                raise ValueError("scratch must hold %d bytes, not %d" % (abi.SRT_PATHS_SCRATCH_BYTES, scratch.shape[0]))
        bg = (C.c_float * 3)(*[float(c) for c in background])
        result = torch.empty((n, 4), dtype=torch.int32, device=rays.device)
        ptr = self._ptr
        entry = lib.srtTracePathsDirectDevice if direct else lib.srtTracePathsDevice
        self._check(entry(self.h, int(traversal), int(max_bounce), bg, ptr(rays, n), n, ptr(rng, n), ptr(result, n), ptr(scratch, n),
                          self._stream_handle(stream)))
        return result

    def scatter_test(self, rays, hits, seed):
        rays = np.ascontiguousarray(rays, abi.RAY_DTYPE)
        hits = np.ascontiguousarray(hits, abi.HIT_DTYPE)
        out = np.zeros((len(rays), 13), np.float32)
        self._check(lib.srtScatterRays(self.h, rays.ctypes.data, hits.ctypes.data, len(rays), seed, out.ctypes.data))
        return out

    def scatter_test_form(self, rays, hits, seed, form):
        """scatter_test through the instance of the shading function `form` selects (bit 0 WIDE, bit 1 COUNT;
        include/srt_hip_test.h): (out13, fetches), fetches = the texel-fetch counter per entry."""
        rays = np.ascontiguousarray(rays, abi.RAY_DTYPE)
        hits = np.ascontiguousarray(hits, abi.HIT_DTYPE)
        out = np.zeros((len(rays), 13), np.float32)
        fetches = np.zeros(len(rays), np.uint32)
        self._check(lib.srtScatterRaysForm(self.h, rays.ctypes.data, hits.ctypes.data, len(rays), seed, form, out.ctypes.data,
                                           fetches.ctypes.data))
        return out, fetches

    def chunk_sum_test(self, slots, path, samples=0):
        """srtTestChunkSum (include/srt_hip_test.h): the exact chunk sum of caller-made partial sums.  slots: (chunks, n, 4)
        float32, rgb partial sums and the slot's sample count; path 0 the chunk-slot kernel, 1 the atomic path with one
        commit per slot.  Returns (n, 4) float32."""
        slots = np.ascontiguousarray(slots, np.float32)
        if slots.ndim != 3 or slots.shape[2] != 4:
            raise ValueError("slots must be (chunks, n, 4)")
        out = np.zeros((slots.shape[1], 4), np.float32)
        self._check(lib.srtTestChunkSum(self.h, slots.ctypes.data, slots.shape[1], slots.shape[0], path, samples, out.ctypes.data))
        return out

    def tri_undecided(self):
        """Triangle tests of the last trace() call that the certified test left to the exact one (include/srt_hip_test.h)."""
        out = C.c_uint64(0)
        self._check(lib.srtTestGetTriUndecided(self.h, C.byref(out)))
        return int(out.value)

    def tri_fast_records(self):
        """The uploaded scene's triFast records as they lie in device memory, (numTriangles, 16) float32 in the scene's
        triangle order (include/srt_hip_test.h)."""
        n = C.c_int32(0)
        self._check(lib.srtTestGetTriFast(self.h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 16), np.float32)
        if n.value:
            self._check(lib.srtTestGetTriFast(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def slab_scene(self):
        """(fast-division word, ordered-box word) of the uploaded scene as the kernels read them now (include/srt_hip_test.h)."""
        out = (C.c_int32 * 2)()
        self._check(lib.srtTestGetSlabScene(self.h, out))
        return int(out[0]), int(out[1])

    def regroup(self):
        """srtTestGetRegroup (include/srt_hip_test.h): the uploaded scene's regrouped node array (n, 8) float32 and its thread
        links (n,) int32 as they lie in device memory now, or None when the upload built none."""
        n = C.c_int32(0)
        self._check(lib.srtTestGetRegroup(self.h, None, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        nodes, links = np.zeros((n.value, 8), np.float32), np.zeros(n.value, np.int32)
        self._check(lib.srtTestGetRegroup(self.h, nodes.ctypes.data, links.ctypes.data, n.value, C.byref(n)))
        return nodes, links

    def regroup_walk(self):
        """srtTestGetRegroupWalk (include/srt_hip_test.h): the uploaded scene's walk sequence as it lies in device memory now
        -- (keep (nodes,) uint8, src (records,) int32, links (records, 2) int32: hit and miss word, entry (world items,)
        int32) -- or None when the upload built none."""
        n = C.c_int32(0)
        self._check(lib.srtTestGetRegroupWalk(self.h, None, None, None, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        nodes = len(self.regroup()[0])
        keep, src, links = np.zeros(nodes, np.uint8), np.zeros(nodes, np.int32), np.zeros((nodes, 2), np.int32)
        entry = np.zeros(int(self._scene_keep[1].numWorld), np.int32)
        self._check(lib.srtTestGetRegroupWalk(self.h, keep.ctypes.data, src.ctypes.data, links.ctypes.data, entry.ctypes.data, nodes, C.byref(n)))
        return keep, src[:n.value].copy(), links[:n.value].copy(), entry

    def refined_rcp_test(self, first_bits, count):
        """srtTestRefinedRcp (include/srt_hip_test.h): the largest |refinedRcp(d) d - 1| (in double) over the float bit patterns
        first_bits .. first_bits + count - 1, and the d that gives it.  Returns (error, d as np.float32)."""
        out = (C.c_uint64 * 2)()
        self._check(lib.srtTestRefinedRcp(self.h, int(first_bits), int(count), out))
        return float(np.array([out[0]], np.uint64).view(np.float64)[0]), np.array([out[1]], np.uint32).view(np.float32)[0]

    def slab_visit_test(self, cases, t_min, certified_scene=1):
        """srtTestSlabVisit (include/srt_hip_test.h): cases (n, 13) float32 -- box min, box max, origin, direction, tMax --
        through the device compile of the certified slab test at one tMin.  Returns (n, 8) float32; column 5 holds the flag
        bits (view it as int32)."""
        cases = np.ascontiguousarray(cases, np.float32)
        if cases.ndim != 2 or cases.shape[1] != 13:
            raise ValueError("cases must be (n, 13)")
        out = np.zeros((len(cases), 8), np.float32)
        fp = C.POINTER(C.c_float)
        self._check(lib.srtTestSlabVisit(self.h, cases.ctypes.data_as(fp), len(cases), float(t_min), int(certified_scene), out.ctypes.data_as(fp)))
        return out

    def set_tunable(self, name, value):
        """Diagnostic knobs of the work distribution / wave scheduler (include/srt_hip_test.h)."""
        self._check(lib.srtSetTunable(self.h, name.encode(), int(value)))

    def get_tunable(self, name):
        v = C.c_int32(0)
        self._check(lib.srtGetTunable(self.h, name.encode(), C.byref(v)))
        return v.value

    def render_aov(self, params, depth=0):
        """The render kernel's own traversal of the ray at bounce `depth` of every pixel's first sample
        (include/srt_hip_test.h): returns an AOV_DTYPE array (H, W)."""
        out = np.zeros((params.imageHeight, params.imageWidth), abi.AOV_DTYPE)
        self._check(lib.srtRenderAov(self.h, C.byref(params), depth, out.ctypes.data))
        return out

    def shade_profile(self):
        out = np.zeros(10, np.uint64)
        self._check(lib.srtGetShadeProfile(self.h, out.ctypes.data))
        return [int(x) for x in out]

    def wf_profile(self):
        """Step profile of the last path-pool launch with tunable wf_profile = 1 (include/srt_hip_test.h)."""
        out = np.zeros(46, np.uint64)
        self._check(lib.srtGetWfProfile(self.h, out.ctypes.data))
        kinds = ["node", "prim", "swap", "hit0", "hit1", "hit2", "restart", "idle", "lost_claim", "new_item", "far_node", "unused"]  # "unused": clocks = primitive steps that ran the exact triangle test, runs = undecided lanes; "far_node" in the whole-tree form: runs = swap steps that ran the head of the walks, lanes = the rays they ran it for
        K = len(kinds)
        prof = {k: {"clocks": int(out[i]), "runs": int(out[K + i]), "lanes": int(out[2 * K + i])} for i, k in enumerate(kinds)}
        prof["sched_clocks"], prof["total_clocks"] = int(out[3 * K]), int(out[3 * K + 1])
        n = max(1, int(out[3 * K + 2]))
        prof["decisions"] = int(out[3 * K + 2])
        prof["mean_seen"] = {k: float(out[3 * K + 3 + i]) / n for i, k in enumerate(["at_node", "at_prim", "finished", "idle", "ready_fill", "fullest_ring", "restart_fill"])}
        return prof

    def launch_info(self):
        """The most recent render launch (include/srt_hip_test.h).  lds_tree_mode: 0 node records through the L1,
        1 / 2 LDS-resident tree with the attenuation stacks in global memory / LDS, 3 the path-pool kernel, 4 its hybrid form
        (the tree's top in LDS, the rest read from global memory)."""
        out = np.zeros(4, np.int32)
        self._check(lib.srtGetLaunchInfo(self.h, out.ctypes.data))
        return {"lds_tree": bool(out[0]), "lds_tree_mode": int(out[0]), "wavefront": int(out[0]) in (3, 4), "hybrid": int(out[0]) == 4, "workgroups": int(out[1]),
                "threads": int(out[2]), "lds_bytes": int(out[3])}

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._check(lib.srtLastKernelMs(self.h, C.byref(ms)))
        return ms.value

    def stats(self):
        s = abi.SrtStats()
        self._check(lib.srtGetStats(self.h, C.byref(s)))
        return {n: int(getattr(s, n)) for n, _ in s._fields_}

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, mhz = C.c_int32(0), C.c_int32(0)
        self._check(lib.srtDeviceInfo(self.h, name, 256, C.byref(cus), C.byref(mhz)))
        return {"name": name.value.decode(), "cus": cus.value, "clock_mhz": mhz.value}


def tri_fast_record(p9):
    """Host only: the triFast record srtUploadScene makes of one triangle (nine floats), 16 float32 (include/srt_hip_test.h)."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(9)
    out = np.zeros(16, np.float32)
    if lib.srtTestTriFastRecord(p9.ctypes.data, out.ctypes.data):
        raise RuntimeError("srtTestTriFastRecord failed")
    return out
