// srt_passes.cpp -- the passes of the C ABI (include/srt_hip.h) over a rendered frame or beside it: the feature passes
// (over the rank's tiles, over a tile list), the denoiser, temporal accumulation and reprojection, and the
// temporal-adaptive frame, which runs srt_render.cpp's adaptive rounds between the two temporal kernels.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "srt_context.h"
#include "srt_launch.h"
#include "srt_lds_layout.h"

/* Feature pass (srt_features.hip).  Reads the scene, the camera and the tile_block tunable; writes only the caller's planes
 * and its own tile counter, so a later render sees the context as it was. */
int checkFeatureArgs(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, const void* const* buffers) {
  if (!ctx) return 1;
  if (!p) return fail(ctx, "features: null parameters");
  if (planes <= 0 || (planes & ~SRT_FEATURE_ALL) != 0) return fail(ctx, "features: bad plane mask 0x%x", (unsigned)planes);
  SrtRenderParams q = *p;  // maxBounce, sppChunks and countStats do not apply
  q.maxBounce = 1;
  q.sppChunks = 0;
  q.countStats = 0;
  if (checkParams(ctx, &q)) return 1;
  if (!buffers) return fail(ctx, "features: null plane array");
  for (int k = 0; k < 4; ++k)
    if ((planes >> k & 1) && !buffers[k]) return fail(ctx, "features: null buffer for selected plane %d", 1 << k);
  return 0;
}

/* What the two feature passes do alike once their arguments are set: the traversal form and its LDS, the kernel's plan, a
 * grid of at most `work` waves, the tile counter reset, the launch.  plan and launch are the pass's own kernel's. */
template <typename Plan, typename Launch>
static int launchFeaturePass(SrtContext* ctx, const SrtRenderParams* p, FeatureArgs& a, int work, hipStream_t stream, Plan plan,
                             Launch launch) {
  const DevScene& sc = ctx->upload.scene;
  // FAITHFUL over a threaded tree that fits a CU's LDS: the stackless walk out of LDS; otherwise the stack walk over
  // scene.nodes (stacks in LDS), which CLOSEST always takes
  const bool closest = p->traversal == SRT_TRAVERSE_CLOSEST;
  const size_t treeBytes = srtFeatureTreeBytes(sc.numNodes);
  const bool ldsTree = !closest && sc.nodeThread != nullptr && treeBytes <= SRT_LDS_BYTES;
  const size_t lds = ldsTree ? treeBytes : srtTraverseStackBytes(sc.stackDepth);
  if (lds > SRT_LDS_BYTES) return fail(ctx, "features: BVH depth %d needs %zu B of LDS per workgroup", sc.stackDepth, lds);
  int block = 0, perCU = 1;
  int rc = plan(closest, ldsTree, lds, &block, &perCU);
  if (rc) return fail(ctx, "features: kernel setup failed: %s", hipGetErrorString((hipError_t)rc));
  const int wavesPerGroup = block / 64;
  const int grid = std::max(1, std::min(ctx->prop.multiProcessorCount * perCU, (work + wavesPerGroup - 1) / wavesPerGroup));
  HIP_OK(ctx, ctx->dFeatureCounter.reserve(16 * sizeof(int32_t)));
  a.counter = ctx->dFeatureCounter.get<int32_t>();
  HIP_OK(ctx, hipMemsetAsync(a.counter, 0, sizeof(int32_t), stream));
  rc = launch(closest, ldsTree, grid, lds);
  if (rc) return fail(ctx, "features launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

int srtRenderFeatureTilesImpl(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, void* const dPlanes[4], void* streamPtr) {
  if (!ctx) return 1;
  if (checkFeatureArgs(ctx, p, planes, dPlanes)) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  FeatureArgs a;
  setImageArgs(a, ctx, p);
  a.planes = planes;
  for (int k = 0; k < 4; ++k) a.out[k] = (planes >> k & 1) ? static_cast<float4*>(dPlanes[k]) : nullptr;
  return launchFeaturePass(ctx, p, a, a.numLocalTiles, stream, [&](bool closest, bool ldsTree, size_t lds, int* block, int* perCU) {
    return srt_features_plan(closest, ldsTree, lds, block, perCU);
  }, [&](bool closest, bool ldsTree, int grid, size_t lds) { return srt_launch_features(&a, closest, ldsTree, grid, lds, stream); });
}

/* Motion pass (srt_motion.hip): the feature pass's checks, launch shape and side effects.  "Previous" is the snapshot
 * srt_refit_host.cpp keeps while tracking is on, or the current tables before there is one (exact zeros). */
int srtRenderMotionTilesImpl(SrtContext* ctx, const SrtRenderParams* p, void* dMotionTiles, void* streamPtr) {
  if (!ctx) return 1;
  if (!ctx->motionTracking) return fail(ctx, "motion: motion tracking is off (srtSetMotionTracking)");
  void* const planes[4] = {dMotionTiles, nullptr, nullptr, nullptr};
  if (checkFeatureArgs(ctx, p, 1, planes)) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  MotionArgs a;
  setImageArgs(a.f, ctx, p);
  a.f.out[0] = static_cast<float4*>(dMotionTiles);
  const Upload& up = ctx->upload;
  a.prevTriTest = up.haveSnapshot ? up.prevTriTest.get<const float4>() : up.scene.triTest;
  a.prevSpheres = up.haveSnapshot ? up.prevSpheres.get<const float4>() : up.scene.spheres;
  return launchFeaturePass(ctx, p, a.f, a.f.numLocalTiles, stream, [&](bool closest, bool ldsTree, size_t lds, int* block, int* perCU) {
    return srt_motion_plan(closest, ldsTree, lds, block, perCU);
  }, [&](bool closest, bool ldsTree, int grid, size_t lds) { return srt_launch_motion(&a, closest, ldsTree, grid, lds, stream); });
}

/* Feature pass over a tile list (srt_features_list.hip), into image-order planes.  The feature pass's side effects: its own
 * counter and the caller's planes. */
int srtRenderFeatureTileListImpl(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, const void* dTileList,
                                        int32_t numListed, void* const dPlaneImages[4], int32_t accumulate, void* streamPtr) {
  if (!ctx) return 1;
  if (checkFeatureArgs(ctx, p, planes, dPlaneImages)) return 1;
  if (p->tileFirst != 0 || p->tileStride != 1) return fail(ctx, "features: a tile list covers the whole image (tileFirst 0, tileStride 1)");
  if (numListed < 0 || numListed > srtNumTiles(p->imageWidth, p->imageHeight))
    return fail(ctx, "features: bad tile list of %d tiles", numListed);
  if (numListed > 0 && !dTileList) return fail(ctx, "features: null tile list");
  if (numListed == 0) return 0;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  FeatureListArgs a;
  setImageArgs(a.f, ctx, p);
  a.f.planes = planes;
  for (int k = 0; k < 4; ++k) a.f.out[k] = (planes >> k & 1) ? static_cast<float4*>(dPlaneImages[k]) : nullptr;
  a.list = static_cast<const uint32_t*>(dTileList);
  a.numListed = numListed;
  return launchFeaturePass(ctx, p, a.f, numListed, stream, [&](bool closest, bool ldsTree, size_t lds, int* block, int* perCU) {
    return srt_features_list_plan(closest, ldsTree, accumulate != 0, lds, block, perCU);
  }, [&](bool closest, bool ldsTree, int grid, size_t lds) {
    return srt_launch_features_list(&a, closest, ldsTree, accumulate != 0, grid, lds, stream);
  });
}

/* Denoiser (srt_denoise.hip).  Reads the tunable denoise_lds_step; writes only the caller's outputs and its own scratch. */
int checkDenoiseParams(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, DenoiseArgs& a,
                                    int& iterations, bool moments) {
  if (!d) return fail(ctx, "denoise: null parameters");
  if (width <= 0 || height <= 0) return fail(ctx, "denoise: image size %dx%d must be positive", width, height);
  if ((int64_t)width * height > 0x7fffffff) return fail(ctx, "denoise: image of %dx%d pixels is too large", width, height);
  iterations = d->iterations == 0 ? SRT_DENOISE_DEFAULT_ITERATIONS : d->iterations;
  if (iterations < 1 || iterations > SRT_DENOISE_MAX_ITERATIONS)
    return fail(ctx, "denoise: iterations %d not in [1, %d] (0 = %d)", d->iterations, SRT_DENOISE_MAX_ITERATIONS,
                SRT_DENOISE_DEFAULT_ITERATIONS);
  const float sig[3] = {d->sigmaLuminance, d->sigmaNormal, d->sigmaDepth};
  const float dflt[3] = {moments ? SRT_DENOISE_MOMENTS_DEFAULT_SIGMA_LUMINANCE : SRT_DENOISE_DEFAULT_SIGMA_LUMINANCE,
                         SRT_DENOISE_DEFAULT_SIGMA_NORMAL, SRT_DENOISE_DEFAULT_SIGMA_DEPTH};
  float use[3];
  for (int k = 0; k < 3; ++k) {
    if (!(sig[k] >= 0.0f && sig[k] < 1e30f)) return fail(ctx, "denoise: sigma %g must be finite and >= 0 (0 = default)", sig[k]);
    use[k] = sig[k] == 0.0f ? dflt[k] : sig[k];
  }
  memset(&a, 0, sizeof a);
  a.width = width;
  a.height = height;
  a.sigmaL = use[0];
  a.sigmaN = use[1];
  a.sigmaZ = use[2];
  return 0;
}

// srtDenoiseMoments (moments = true): dMoments may be null, and then this is srtDenoise bit for bit
int srtDenoiseImpl(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, const void* dBeauty,
                                const void* const dPlanes[4], void* dOut, void* dRgba, void* streamPtr, bool moments,
                                const void* dMoments) {
  if (!ctx) return 1;
  DenoiseArgs a;
  int iterations = 0;
  if (checkDenoiseParams(ctx, d, width, height, a, iterations, moments && dMoments)) return 1;
  if (!dBeauty) return fail(ctx, "denoise: null beauty buffer");
  if (!dPlanes) return fail(ctx, "denoise: null plane array");
  if (!dPlanes[1]) return fail(ctx, "denoise: the NORMAL plane is required");
  if (!dPlanes[3]) return fail(ctx, "denoise: the DEPTH plane is required");
  if (d->demodulate && !dPlanes[0]) return fail(ctx, "denoise: demodulate needs the ALBEDO plane");
  if (!dOut && !dRgba) return fail(ctx, "denoise: no output buffer");
  HIP_OK(ctx, hipSetDevice(ctx->device));
  const size_t nPix = (size_t)width * height;
  HIP_OK(ctx, ctx->denoiseScratch.reserve(nPix * SRT_DENOISE_SCRATCH_BYTES_PER_PIXEL));
  char* s = ctx->denoiseScratch.get<char>();
  a.beauty = static_cast<const float4*>(dBeauty);
  a.normal = static_cast<const float4*>(dPlanes[1]);
  a.depth = static_cast<const float4*>(dPlanes[3]);
  a.albedo = d->demodulate ? static_cast<const float4*>(dPlanes[0]) : nullptr;
  a.guide = reinterpret_cast<float4*>(s);
  a.col[0] = reinterpret_cast<float4*>(s + 16 * nPix);
  a.col[1] = reinterpret_cast<float4*>(s + 32 * nPix);
  a.grad = reinterpret_cast<float2*>(s + 48 * nPix);
  a.out = static_cast<float4*>(dOut);
  a.rgba = static_cast<uint8_t*>(dRgba);
  a.moments = moments ? static_cast<const float4*>(dMoments) : nullptr;
  const int rc = srt_launch_denoise(&a, iterations, std::max(0, ctx->tun.denoiseLdsStep), static_cast<hipStream_t>(streamPtr));
  if (rc) return fail(ctx, "denoise launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// test entry (include/srt_hip_test.h): the four regions of the denoise scratch as srtDenoiseImpl lays them out for a
// width x height image, copied to the host.  Launches nothing, changes nothing.
static int srtTestDenoiseScratchImpl(SrtContext* ctx, int32_t width, int32_t height, float* hGuide4, float* hCol0_4,
                                     float* hCol1_4, float* hGrad2) {
  if (!ctx) return 1;
  if (width <= 0 || height <= 0) return fail(ctx, "denoise scratch: image size %dx%d must be positive", width, height);
  if ((int64_t)width * height > 0x7fffffff) return fail(ctx, "denoise scratch: image of %dx%d pixels is too large", width, height);
  const size_t nPix = (size_t)width * height;
  if (ctx->denoiseScratch.bytes() < nPix * SRT_DENOISE_SCRATCH_BYTES_PER_PIXEL)
    return fail(ctx, "denoise scratch: the scratch holds %zu bytes, a %dx%d image needs %zu (no srtDenoise of that size yet)",
                ctx->denoiseScratch.bytes(), width, height, nPix * SRT_DENOISE_SCRATCH_BYTES_PER_PIXEL);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, hipDeviceSynchronize());
  const char* s = ctx->denoiseScratch.get<char>();
  float* const dst[4] = {hGuide4, hCol0_4, hCol1_4, hGrad2};
  const size_t off[4] = {0, 16 * nPix, 32 * nPix, 48 * nPix}, len[4] = {16 * nPix, 16 * nPix, 16 * nPix, 8 * nPix};
  for (int k = 0; k < 4; ++k)
    if (dst[k]) HIP_OK(ctx, hipMemcpy(dst[k], s + off[k], len[k], hipMemcpyDeviceToHost));
  return 0;
}

/* Temporal accumulation (srt_temporal.hip).  Reads nothing of the context but the device ordinal; the frame entry keeps
 * the histories and the previous camera in the context.  dMotion (the Motion entries) selects the motion-aware kernels;
 * null is the plain entry in every byte. */
static bool sameProjection(const SrtCamera& a, const SrtCamera& b) {
  return !memcmp(a.origin, b.origin, 12) && !memcmp(a.lleft, b.lleft, 12) && !memcmp(a.horizontal, b.horizontal, 12) &&
         !memcmp(a.vertical, b.vertical, 12) && !memcmp(a.w, b.w, 12);
}

int checkTemporalParams(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, TemporalArgs& a) {
  if (!t) return fail(ctx, "temporal: null parameters");
  if (width < 2 || height < 2) return fail(ctx, "temporal: image size %dx%d must be at least 2x2", width, height);
  if ((int64_t)width * height > 0x7fffffff / 3) return fail(ctx, "temporal: image of %dx%d pixels is too large", width, height);
  if (!(t->normalCos >= 0.0f && t->normalCos <= 1.0f)) return fail(ctx, "temporal: normalCos %g must be in [0, 1] (0 = default)", t->normalCos);
  if (!(t->planeDist >= 0.0f)) return fail(ctx, "temporal: planeDist %g must be >= 0 (0 = default)", t->planeDist);
  if (!(t->maxHistory >= 0.0f)) return fail(ctx, "temporal: maxHistory %g must be >= 0 (0 = default, +inf = no cap)", t->maxHistory);
  memset(&a, 0, sizeof a);
  a.width = width;
  a.height = height;
  a.normalCos = t->normalCos == 0.0f ? SRT_TEMPORAL_DEFAULT_NORMAL_COS : t->normalCos;
  a.planeDist = t->planeDist == 0.0f ? SRT_TEMPORAL_DEFAULT_PLANE_DIST : t->planeDist;
  a.maxHistory = t->maxHistory == 0.0f ? SRT_TEMPORAL_DEFAULT_MAX_HISTORY : t->maxHistory;
  return 0;
}

// Everything srtTemporalAccumulate checks, and the kernel's arguments: nothing is launched
static int temporalArgs(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* dBeauty,
                        const void* dMoments, const void* const dPlanes[4], const void* dMotion, const SrtCamera* cam,
                        const SrtCamera* prevCam, const void* dHistoryIn, void* dBeautyOut, void* dMomentsOut, void* dHistoryOut,
                        TemporalArgs& a) {
  if (!ctx) return 1;
  if (checkTemporalParams(ctx, t, width, height, a)) return 1;
  if (!dBeauty) return fail(ctx, "temporal: null beauty buffer");
  if (!dPlanes) return fail(ctx, "temporal: null plane array");
  if (!dPlanes[1]) return fail(ctx, "temporal: the NORMAL plane is required");
  if (!dPlanes[2]) return fail(ctx, "temporal: the POSITION plane is required");
  if (!dPlanes[3]) return fail(ctx, "temporal: the DEPTH plane is required");
  if (t->demodulate && !dPlanes[0]) return fail(ctx, "temporal: demodulate needs the ALBEDO plane");
  if (!dBeautyOut && !dMomentsOut) return fail(ctx, "temporal: no output buffer");
  if (!dHistoryOut) return fail(ctx, "temporal: null history output");
  if (dHistoryOut == dHistoryIn) return fail(ctx, "temporal: the history is not updated in place (dHistoryOut == dHistoryIn)");
  if (!cam || (dHistoryIn && !prevCam)) return fail(ctx, "temporal: null camera");
  HIP_OK(ctx, hipSetDevice(ctx->device));
  a.beauty = static_cast<const float4*>(dBeauty);
  a.moments = static_cast<const float4*>(dMoments);
  a.albedo = t->demodulate ? static_cast<const float4*>(dPlanes[0]) : nullptr;
  a.normal = static_cast<const float4*>(dPlanes[1]);
  a.position = static_cast<const float4*>(dPlanes[2]);
  a.depth = static_cast<const float4*>(dPlanes[3]);
  a.historyIn = static_cast<const float4*>(dHistoryIn);
  a.beautyOut = static_cast<float4*>(dBeautyOut);
  a.momentsOut = static_cast<float4*>(dMomentsOut);
  a.historyOut = static_cast<float4*>(dHistoryOut);
  a.cam = *cam;
  a.prev = dHistoryIn ? *prevCam : *cam;
  a.sameCamera = sameProjection(a.cam, a.prev) ? 1 : 0;
  a.motion = static_cast<const float4*>(dMotion);  // set: the Motion forms, which do not read sameCamera
  return 0;
}

int srtTemporalAccumulateImpl(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height,
                                           const void* dBeauty, const void* dMoments, const void* const dPlanes[4], const void* dMotion,
                                           const SrtCamera* cam, const SrtCamera* prevCam, const void* dHistoryIn, void* dBeautyOut,
                                           void* dMomentsOut, void* dHistoryOut, void* streamPtr) {
  TemporalArgs a;
  if (temporalArgs(ctx, t, width, height, dBeauty, dMoments, dPlanes, dMotion, cam, prevCam, dHistoryIn, dBeautyOut, dMomentsOut, dHistoryOut, a))
    return 1;
  const int rc = srt_launch_temporal(&a, static_cast<hipStream_t>(streamPtr));
  if (rc) return fail(ctx, "temporal launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// SrtTemporalStats from the finished frame's DEVICE buffers: this frame's sums, an accumulated plane (its w is the
// output count) and the new history
int temporalStats(SrtContext* ctx, size_t nPix, const void* dCurrent, const void* dAccumulated, const void* dHistory,
                               SrtTemporalStats* stats) {
  std::vector<float> cur(nPix * 4), acc(nPix * 4), hist(nPix * 4);
  if (hipMemcpy(cur.data(), dCurrent, nPix * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(acc.data(), dAccumulated, nPix * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(hist.data(), dHistory, nPix * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(ctx, "temporal: copy stats");
  stats->historyPixels = 0;
  double sum = 0.0;
  for (size_t i = 0; i < nPix; ++i) {
    if (acc[4 * i + 3] > cur[4 * i + 3]) stats->historyPixels++;
    sum += (double)hist[4 * i + 3];
  }
  stats->meanHistoryCount = sum / (double)nPix;
  return 0;
}

/* Temporal-adaptive frames (srt_temporal_adaptive.hip): the reprojected history once per frame, srtRenderAdaptive's rounds
 * deciding on the pooled moments, srtTemporalAccumulate of the final sums. */
static int srtTemporalReprojectImpl(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height,
                                    const void* const dPlanes[4], const void* dMotion, const SrtCamera* cam,
                                    const SrtCamera* prevCam, const void* dHistoryIn, void* dReprojected, void* streamPtr) {
  if (!ctx) return 1;
  if (!dReprojected) return fail(ctx, "temporal: null reprojected buffer");
  TemporalArgs a;
  // srtTemporalAccumulate's checks; the beauty and its outputs are not part of this entry (any non-null pointer passes)
  if (temporalArgs(ctx, t, width, height, dReprojected, nullptr, dPlanes, dMotion, cam, prevCam, dHistoryIn, dReprojected, nullptr, dReprojected, a))
    return 1;
  a.beauty = nullptr;
  a.beautyOut = nullptr;
  const int rc = srt_launch_temporal_reproject(&a, static_cast<hipStream_t>(streamPtr));
  if (rc) return fail(ctx, "temporal reprojection launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

int srtRenderTemporalAdaptiveImpl(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap,
                                               const SrtTemporalParams* t, const void* const dPlanes[4], const SrtCamera* prevCam,
                                               const void* dHistoryIn, void* dAccumImage, void* dMomentsImage, void* dBeautyOut,
                                               void* dMomentsOut, void* dHistoryOut, SrtTemporalAdaptiveStats* stats, void* streamPtr,
                                               bool guided) {
  // every check of both halves before the first launch
  if (!ctx) return 1;
  if (checkAdaptive(ctx, p, ap, true, dAccumImage, dMomentsImage)) return 1;
  const int W = p->imageWidth, H = p->imageHeight;
  const size_t nPix = (size_t)W * H;
  TemporalArgs a;
  if (temporalArgs(ctx, t, W, H, dAccumImage, dMomentsImage, dPlanes, nullptr, &ctx->camFull, prevCam, dHistoryIn, dBeautyOut, dMomentsOut,
                   dHistoryOut, a))
    return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, ctx->temporalReprojected.reserve(nPix * SRT_TEMPORAL_REPROJECTED_BYTES_PER_PIXEL));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  TemporalArgs ra = a;
  ra.historyOut = ctx->temporalReprojected.get<float4>();
  int rc = srt_launch_temporal_reproject(&ra, stream);
  if (rc) return fail(ctx, "temporal reprojection launch failed: %s", hipGetErrorString((hipError_t)rc));
  AdaptivePool pool{ctx->temporalReprojected.get<const float4>(), a.albedo};
  SrtTemporalAdaptiveStats st;
  memset(&st, 0, sizeof st);
  // guided: the rounds from 1 on extend the caller's planes (they hold round 0).  The pooled decisions keep reading the
  // ALBEDO means of the first p->spp samples -- h was formed beside them -- from a copy that lives as long as this call
  AdaptiveGuides guides{0, const_cast<void* const*>(dPlanes), false};
  DeviceBuffer albedoFirst;
  if (guided) {
    for (int k = 0; k < 4; ++k)
      if (dPlanes[k]) guides.planes |= 1 << k;
    if (a.albedo) {
      if (albedoFirst.reserve(nPix * sizeof(float4)) != hipSuccess) return fail(ctx, "temporal: hipMalloc");
      HIP_OK(ctx, hipMemcpyAsync(albedoFirst.get(), a.albedo, nPix * sizeof(float4), hipMemcpyDeviceToDevice, stream));
      pool.albedo = albedoFirst.get<const float4>();
    }
  }
  if (srtRenderAdaptiveImpl(ctx, p, ap, dAccumImage, dMomentsImage, nullptr, &st.adaptive, streamPtr, &pool, guided ? &guides : nullptr))
    return 1;
  rc = srt_launch_temporal(&a, stream);
  if (rc) return fail(ctx, "temporal launch failed: %s", hipGetErrorString((hipError_t)rc));
  if (hipStreamSynchronize(stream) != hipSuccess) return fail(ctx, "temporal: kernel failed: %s", hipGetErrorString(hipGetLastError()));
  if (stats) {
    if (temporalStats(ctx, nPix, dAccumImage, dBeautyOut ? dBeautyOut : dMomentsOut, dHistoryOut, &st.temporal)) return 1;
    *stats = st;
  }
  return 0;
}

extern "C" {

int srtRenderFeatureTiles(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, void* const dPlanes[4], void* stream) {
  SRT_GUARDED(ctx, srtRenderFeatureTilesImpl(ctx, p, planes, dPlanes, stream));
}
int srtRenderFeatureTileList(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, const void* dTileList, int32_t numListed,
                             void* const dPlaneImages[4], int32_t accumulate, void* stream) {
  SRT_GUARDED(ctx, srtRenderFeatureTileListImpl(ctx, p, planes, dTileList, numListed, dPlaneImages, accumulate, stream));
}
int srtDenoise(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, const void* dBeauty,
               const void* const dPlanes[4], void* dOut, void* dRgba, void* stream) {
  SRT_GUARDED(ctx, srtDenoiseImpl(ctx, d, width, height, dBeauty, dPlanes, dOut, dRgba, stream));
}
int srtDenoiseMoments(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, const void* dBeauty,
                      const void* const dPlanes[4], const void* dMoments, void* dOut, void* dRgba, void* stream) {
  SRT_GUARDED(ctx, srtDenoiseImpl(ctx, d, width, height, dBeauty, dPlanes, dOut, dRgba, stream, true, dMoments));
}
int srtTestDenoiseScratch(SrtContext* ctx, int32_t width, int32_t height, float* hGuide4, float* hCol0_4, float* hCol1_4,
                          float* hGrad2) {
  SRT_GUARDED(ctx, srtTestDenoiseScratchImpl(ctx, width, height, hGuide4, hCol0_4, hCol1_4, hGrad2));
}
int srtTemporalAccumulate(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* dBeauty,
                          const void* dMoments, const void* const dPlanes[4], const SrtCamera* cam, const SrtCamera* prevCam,
                          const void* dHistoryIn, void* dBeautyOut, void* dMomentsOut, void* dHistoryOut, void* stream) {
  return srtTemporalAccumulateMotion(ctx, t, width, height, dBeauty, dMoments, dPlanes, nullptr, cam, prevCam, dHistoryIn, dBeautyOut,
                                     dMomentsOut, dHistoryOut, stream);
}
int srtTemporalAccumulateMotion(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* dBeauty,
                                const void* dMoments, const void* const dPlanes[4], const void* dMotion, const SrtCamera* cam,
                                const SrtCamera* prevCam, const void* dHistoryIn, void* dBeautyOut, void* dMomentsOut,
                                void* dHistoryOut, void* stream) {
  SRT_GUARDED(ctx, srtTemporalAccumulateImpl(ctx, t, width, height, dBeauty, dMoments, dPlanes, dMotion, cam, prevCam, dHistoryIn,
                                             dBeautyOut, dMomentsOut, dHistoryOut, stream));
}
int srtRenderMotionTiles(SrtContext* ctx, const SrtRenderParams* p, void* dMotionTiles, void* stream) {
  SRT_GUARDED(ctx, srtRenderMotionTilesImpl(ctx, p, dMotionTiles, stream));
}
int srtTemporalReproject(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* const dPlanes[4],
                         const SrtCamera* cam, const SrtCamera* prevCam, const void* dHistoryIn, void* dReprojected, void* stream) {
  return srtTemporalReprojectMotion(ctx, t, width, height, dPlanes, nullptr, cam, prevCam, dHistoryIn, dReprojected, stream);
}
int srtTemporalReprojectMotion(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height,
                               const void* const dPlanes[4], const void* dMotion, const SrtCamera* cam, const SrtCamera* prevCam,
                               const void* dHistoryIn, void* dReprojected, void* stream) {
  SRT_GUARDED(ctx, srtTemporalReprojectImpl(ctx, t, width, height, dPlanes, dMotion, cam, prevCam, dHistoryIn, dReprojected, stream));
}
int srtRenderTemporalAdaptive(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, const SrtTemporalParams* t,
                              const void* const dPlanes[4], const SrtCamera* prevCam, const void* dHistoryIn, void* dAccumImage,
                              void* dMomentsImage, void* dBeautyOut, void* dMomentsOut, void* dHistoryOut,
                              SrtTemporalAdaptiveStats* stats, void* stream) {
  SRT_GUARDED(ctx, srtRenderTemporalAdaptiveImpl(ctx, p, ap, t, dPlanes, prevCam, dHistoryIn, dAccumImage, dMomentsImage, dBeautyOut,
                                                 dMomentsOut, dHistoryOut, stats, stream));
}
int srtRenderTemporalAdaptiveGuided(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap,
                                    const SrtTemporalParams* t, void* const dPlanes[4], const SrtCamera* prevCam,
                                    const void* dHistoryIn, void* dAccumImage, void* dMomentsImage, void* dBeautyOut,
                                    void* dMomentsOut, void* dHistoryOut, SrtTemporalAdaptiveStats* stats, void* stream) {
  SRT_GUARDED(ctx, srtRenderTemporalAdaptiveImpl(ctx, p, ap, t, dPlanes, prevCam, dHistoryIn, dAccumImage, dMomentsImage, dBeautyOut,
                                                 dMomentsOut, dHistoryOut, stats, stream, true));
}
int srtTemporalReset(SrtContext* ctx) {
  if (!ctx) return 1;
  (void)hipSetDevice(ctx->device);
  ctx->temporalValid = false;
  ctx->temporalRefits = 0;
  for (auto& h : ctx->temporalHistory) h = DeviceBuffer();
  return 0;
}

}  // extern "C"
