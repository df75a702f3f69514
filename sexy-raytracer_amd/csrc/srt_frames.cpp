// srt_frames.cpp -- the blocking entries of the C ABI that render a whole frame into HOST buffers (include/srt_hip.h,
// srtRenderAov: include/srt_hip_test.h).  Each is a composition of the device-level entries (srt_render.cpp and
// srt_passes.cpp, declared in srt_context.h; of srt_rays.cpp's only srtRenderDirectImage's two, through the C ABI) on the
// null stream, over staging buffers that live for the call.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "srt_context.h"
#include "srt_launch.h"

namespace {

// One call's staging: the parameters, the sizes, the device buffers an entry reserves before its first launch, and the
// steps the entries share.  Every step returns 0 or fail()'s 1.
struct FrameStage {
  SrtContext* const ctx;
  const char* const prefix;  // of this entry's failure messages
  SrtRenderParams p;
  size_t nPix = 0, imageBytes = 0, tileBytes = 0;  // pixels, a float4 image, a float4 tile buffer of the whole image
  DeviceBuffer tiles, mtiles, featTiles[4];        // tile order: beauty, moments, feature planes
  DeviceBuffer accum, mom, rgba, featImage[4];     // image order: what render() and features() resolve into
  DeviceBuffer motionTiles, motionImage;           // the motion plane (a fifth one: the frame after a tracked refit)
  DeviceBuffer accOut, momOut, out, outRgba;       // image order: the temporal step's and the denoiser's outputs
  void* dTiles[4] = {nullptr, nullptr, nullptr, nullptr};
  void* dPlanes[4] = {nullptr, nullptr, nullptr, nullptr};  // featImage as the denoiser and the temporal step take it

  // wholeImage: the entry renders every tile itself, whatever split the caller's parameters name
  FrameStage(SrtContext* c, const char* pre, const SrtRenderParams* pIn, bool wholeImage = true) : ctx(c), prefix(pre), p(*pIn) {
    if (wholeImage) {
      p.tileFirst = 0;
      p.tileStride = 1;
    }
  }
  // after the entry's argument checks
  int begin() {
    HIP_OK(ctx, hipSetDevice(ctx->device));
    nPix = (size_t)p.imageWidth * p.imageHeight;
    imageBytes = nPix * sizeof(float4);
    tileBytes = (size_t)srtNumTiles(p.imageWidth, p.imageHeight) * SRT_TILE_PIXELS * sizeof(float4);
    return 0;
  }
  int reserve(DeviceBuffer& b, size_t bytes) { return b.reserve(bytes) == hipSuccess ? 0 : fail(ctx, "%s: hipMalloc", prefix); }
  // the outputs the caller asked for: the denoised image and its 8-bit form
  int reserveDenoised(const void* hDenoised, const void* hRgba) {
    return (hDenoised && reserve(out, imageBytes)) || (hRgba && reserve(outRgba, nPix * 4));
  }
  int reserveFeatures(int32_t planes, bool withTiles = true) {
    for (int k = 0; k < 4; ++k) {
      if (!(planes >> k & 1)) continue;
      if ((withTiles && reserve(featTiles[k], tileBytes)) || reserve(featImage[k], imageBytes)) return 1;
      dTiles[k] = featTiles[k].get();
      dPlanes[k] = featImage[k].get();
    }
    return 0;
  }
  // The beauty, with the moments plane when mtiles is reserved, resolved into those of rgba, accum and mom that are
  int render() {
    if (srtRenderTilesImpl(ctx, &p, tiles.get(), nullptr, nullptr, 0, mtiles.get())) return 1;
    if (srtResolveTiles(ctx, &p, tiles.get(), rgba.get(), accum.get(), nullptr)) return 1;
    return mom.get() && srtResolveTiles(ctx, &p, mtiles.get(), nullptr, mom.get(), nullptr);
  }
  // The feature pass of the same parameters, resolved into featImage
  int features(int32_t planes) {
    if (srtRenderFeatureTilesImpl(ctx, &p, planes, dTiles, nullptr)) return 1;
    for (int k = 0; k < 4; ++k)
      if (dTiles[k] && srtResolveTiles(ctx, &p, dTiles[k], nullptr, dPlanes[k], nullptr)) return 1;
    return 0;
  }
  // The motion pass of the same parameters, resolved into motionImage
  int motion() {
    if (srtRenderMotionTilesImpl(ctx, &p, motionTiles.get(), nullptr)) return 1;
    return srtResolveTiles(ctx, &p, motionTiles.get(), nullptr, motionImage.get(), nullptr);
  }
  // The denoiser (moments: srtDenoiseMoments with that plane) into the outputs reserveDenoised reserved, if any
  int denoise(const SrtDenoiseParams* d, const DeviceBuffer& beauty, bool moments, const DeviceBuffer& dMoments) {
    if (!out.get() && !outRgba.get()) return 0;
    return srtDenoiseImpl(ctx, d, p.imageWidth, p.imageHeight, beauty.get(), dPlanes, out.get(), outRgba.get(), nullptr, moments, dMoments.get());
  }
  int finish() {
    if (hipDeviceSynchronize() != hipSuccess) return fail(ctx, "%s: kernel failed: %s", prefix, hipGetErrorString(hipGetLastError()));
    return wfCheck(ctx);
  }
  int copyOut(void* h, const DeviceBuffer& d, size_t bytes, const char* name) {
    if (h && hipMemcpy(h, d.get(), bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, "%s: copy %s", prefix, name);
    return 0;
  }
};

// The history ping-pong of the temporal frame entries (SrtContext::temporalHistory).  begin, before the frame's first
// launch: a history of another size or demodulation is forgotten (first: the reservation may reallocate), both histories
// are reserved, the frame reads the one the last frame wrote (null: none) and writes the other, and no history is valid
// until commit, after the frame is complete.  Refits with motion tracking on leave the history valid and are counted: a
// motionAware frame (srtRenderTemporalFrame) keeps it across exactly one -- the snapshot spans one epoch -- and *useMotion
// tells it to reproject with the motion plane; any other frame, or more refits, drop it as a refit without tracking does.
int beginTemporalFrame(SrtContext* ctx, int32_t W, int32_t H, bool demodulate, bool motionAware, const void** histIn, void** histOut,
                       bool* useMotion = nullptr) {
  const int32_t key[3] = {W, H, demodulate ? 1 : 0};
  if (memcmp(key, ctx->temporalKey, sizeof key) != 0) ctx->temporalValid = false;
  const bool across = motionAware && ctx->motionTracking && ctx->temporalRefits == 1;
  if (ctx->temporalRefits > 0 && !across) ctx->temporalValid = false;
  if (useMotion) *useMotion = across && ctx->temporalValid;
  for (auto& h : ctx->temporalHistory)
    if (h.reserve((size_t)W * H * SRT_TEMPORAL_HISTORY_BYTES_PER_PIXEL) != hipSuccess) return fail(ctx, "temporal: hipMalloc history");
  *histIn = ctx->temporalValid ? ctx->temporalHistory[ctx->temporalCurrent].get() : nullptr;
  *histOut = ctx->temporalHistory[ctx->temporalCurrent ^ 1].get();
  ctx->temporalValid = false;
  return 0;
}

void commitTemporalFrame(SrtContext* ctx, int32_t W, int32_t H, bool demodulate) {
  const int32_t key[3] = {W, H, demodulate ? 1 : 0};
  ctx->temporalCurrent ^= 1;
  ctx->temporalCam = ctx->camFull;
  memcpy(ctx->temporalKey, key, sizeof key);
  ctx->temporalValid = true;
  ctx->temporalRefits = 0;
}

// srtRenderImage, and srtRenderImageMoments (moments): the same render through srtRenderTilesMoments, both planes resolved
int renderImage(SrtContext* ctx, const SrtRenderParams* pIn, float* hAccum, float* hMoments, uint8_t* hRgba, bool moments) {
  FrameStage f(ctx, "render", pIn);
  if (checkParams(ctx, &f.p) || f.begin()) return 1;
  if (f.reserve(f.tiles, f.tileBytes) || (moments && f.reserve(f.mtiles, f.tileBytes))) return 1;
  if ((hRgba && f.reserve(f.rgba, f.nPix * 4)) || (hAccum && f.reserve(f.accum, f.imageBytes)) || (hMoments && f.reserve(f.mom, f.imageBytes))) return 1;
  if (f.render() || f.finish()) return 1;
  return f.copyOut(hRgba, f.rgba, f.nPix * 4, "rgba") || f.copyOut(hAccum, f.accum, f.imageBytes, "accum") ||
         f.copyOut(hMoments, f.mom, f.imageBytes, "moments");
}

int srtRenderImageMomentsImpl(SrtContext* ctx, const SrtRenderParams* pIn, float* hAccum, float* hMoments, uint8_t* hRgba) {
  if (!ctx) return 1;
  if (!pIn) return fail(ctx, "render: null parameters");
  if (pIn->countStats) return fail(ctx, "render: the moments entries have no counting variant (countStats must be 0)");
  return renderImage(ctx, pIn, hAccum, hMoments, hRgba, true);
}

// The adaptive loop synchronises its stream after every round and after its own RGBA resolve: nothing is left to wait for
int srtRenderAdaptiveImageImpl(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, float* hAccum,
                               float* hMoments, uint8_t* hRgba, SrtAdaptiveStats* stats) {
  if (checkAdaptive(ctx, p, ap, false, nullptr, nullptr)) return 1;
  FrameStage f(ctx, "adaptive", p, false);
  if (f.begin() || f.reserve(f.accum, f.imageBytes) || f.reserve(f.mom, f.imageBytes) || (hRgba && f.reserve(f.rgba, f.nPix * 4))) return 1;
  if (srtRenderAdaptiveImpl(ctx, p, ap, f.accum.get(), f.mom.get(), f.rgba.get(), stats, nullptr)) return 1;
  return f.copyOut(hRgba, f.rgba, f.nPix * 4, "rgba") || f.copyOut(hAccum, f.accum, f.imageBytes, "accum") ||
         f.copyOut(hMoments, f.mom, f.imageBytes, "moments");
}

// One image buffer serves the planes in turn; the division by the count is the host's
int srtRenderFeatureImageImpl(SrtContext* ctx, const SrtRenderParams* pIn, int32_t planes, float* const hPlanes[4]) {
  if (!ctx) return 1;
  if (checkFeatureArgs(ctx, pIn, planes, reinterpret_cast<const void* const*>(hPlanes))) return 1;
  FrameStage f(ctx, "features", pIn);
  if (f.begin()) return 1;
  for (int k = 0; k < 4; ++k) {
    if (!(planes >> k & 1)) continue;
    if (f.reserve(f.featTiles[k], f.tileBytes)) return 1;
    f.dTiles[k] = f.featTiles[k].get();
  }
  if (f.reserve(f.accum, f.imageBytes)) return 1;
  if (srtRenderFeatureTilesImpl(ctx, &f.p, planes, f.dTiles, nullptr)) return 1;
  for (int k = 0; k < 4; ++k) {
    if (!(planes >> k & 1)) continue;
    if (srtResolveTiles(ctx, &f.p, f.dTiles[k], nullptr, f.accum.get(), nullptr) || f.finish()) return 1;
    float* h = hPlanes[k];
    if (f.copyOut(h, f.accum, f.imageBytes, "out")) return 1;
    // the mean over the samples that counted (a float division, as the caller would do it), w stays the count
    for (size_t i = 0; i < f.nPix; ++i) {
      float* v = h + 4 * i;
      const float w = v[3];
      for (int c = 0; c < 3; ++c) v[c] = w != 0.0f ? v[c] / w : 0.0f;
    }
  }
  return 0;
}

// srtRenderMotionImage: the motion pass resolved, the division by the count the host's as above
int srtRenderMotionImageImpl(SrtContext* ctx, const SrtRenderParams* pIn, float* hMotion) {
  if (!ctx) return 1;
  if (!ctx->motionTracking) return fail(ctx, "motion: motion tracking is off (srtSetMotionTracking)");
  const void* const outs[4] = {hMotion, nullptr, nullptr, nullptr};
  if (checkFeatureArgs(ctx, pIn, 1, outs)) return 1;
  FrameStage f(ctx, "motion", pIn);
  if (f.begin() || f.reserve(f.motionTiles, f.tileBytes) || f.reserve(f.motionImage, f.imageBytes)) return 1;
  if (f.motion() || f.finish() || f.copyOut(hMotion, f.motionImage, f.imageBytes, "out")) return 1;
  for (size_t i = 0; i < f.nPix; ++i) {
    float* v = hMotion + 4 * i;
    const float w = v[3];
    for (int c = 0; c < 3; ++c) v[c] = w != 0.0f ? v[c] / w : 0.0f;
  }
  return 0;
}

// srtRenderDenoisedImage: the beauty render and its resolve exactly as srtRenderImage does them, the feature pass of the
// same parameters, the denoiser.  moments: srtRenderDenoisedImageMoments -- the moments render, its plane resolved (into
// hMoments as well) and handed to the denoiser
int srtRenderDenoisedImageImpl(SrtContext* ctx, const SrtRenderParams* pIn, const SrtDenoiseParams* d, float* hAccum,
                               float* hDenoised, uint8_t* hRgba, bool moments = false, float* hMoments = nullptr) {
  if (!ctx) return 1;
  if (!pIn) return fail(ctx, "denoise: null render parameters");
  DenoiseArgs check;
  int iterations = 0;
  if (checkDenoiseParams(ctx, d, pIn->imageWidth, pIn->imageHeight, check, iterations, moments)) return 1;
  if (moments && pIn->countStats) return fail(ctx, "render: the moments entries have no counting variant (countStats must be 0)");
  FrameStage f(ctx, "denoise", pIn);
  if (checkParams(ctx, &f.p) || f.begin()) return 1;
  const int32_t planes = SRT_FEATURE_NORMAL | SRT_FEATURE_DEPTH | (d->demodulate ? SRT_FEATURE_ALBEDO : 0);
  if (f.reserve(f.tiles, f.tileBytes) || f.reserve(f.accum, f.imageBytes)) return 1;
  if (moments && (f.reserve(f.mtiles, f.tileBytes) || f.reserve(f.mom, f.imageBytes))) return 1;
  if (f.reserveDenoised(hDenoised, hRgba) || f.reserveFeatures(planes)) return 1;
  if (f.render() || f.features(planes) || f.denoise(d, f.accum, moments, f.mom) || f.finish()) return 1;
  return f.copyOut(hAccum, f.accum, f.imageBytes, "accum") || f.copyOut(hDenoised, f.out, f.imageBytes, "denoised") ||
         f.copyOut(hRgba, f.outRgba, f.nPix * 4, "rgba") || f.copyOut(hMoments, f.mom, f.imageBytes, "moments");
}

// srtRenderAdaptiveDenoisedImage: the guided adaptive render with all four planes, srtDenoiseMoments on its sums
int srtRenderAdaptiveDenoisedImageImpl(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap,
                                       const SrtDenoiseParams* d, float* hAccum, float* hMoments, float* hDenoised,
                                       uint8_t* hRgba, SrtAdaptiveStats* stats) {
  if (!ctx) return 1;
  if (checkAdaptive(ctx, p, ap, false, nullptr, nullptr)) return 1;
  DenoiseArgs check;
  int iterations = 0;
  if (checkDenoiseParams(ctx, d, p->imageWidth, p->imageHeight, check, iterations, true)) return 1;
  FrameStage f(ctx, "denoise", p, false);
  if (f.begin() || f.reserve(f.accum, f.imageBytes) || f.reserve(f.mom, f.imageBytes)) return 1;
  if (f.reserveDenoised(hDenoised, hRgba) || f.reserveFeatures(SRT_FEATURE_ALL, false)) return 1;
  const AdaptiveGuides guides{SRT_FEATURE_ALL, f.dPlanes, true};
  if (srtRenderAdaptiveImpl(ctx, p, ap, f.accum.get(), f.mom.get(), nullptr, stats, nullptr, nullptr, &guides)) return 1;
  if (f.denoise(d, f.accum, true, f.mom) || f.finish()) return 1;
  return f.copyOut(hAccum, f.accum, f.imageBytes, "accum") || f.copyOut(hMoments, f.mom, f.imageBytes, "moments") ||
         f.copyOut(hDenoised, f.out, f.imageBytes, "denoised") || f.copyOut(hRgba, f.outRgba, f.nPix * 4, "rgba");
}

// srtRenderTemporalFrame: the frame exactly as srtRenderDenoisedImageMoments renders it, with all four planes, accumulated
// onto the context's history, the denoiser on the accumulated sums.  The one frame after a refit with motion tracking on
// also runs the motion pass and accumulates with srtTemporalAccumulateMotion (include/srt_hip.h "Motion")
int srtRenderTemporalFrameImpl(SrtContext* ctx, const SrtRenderParams* pIn, const SrtDenoiseParams* d, const SrtTemporalParams* t,
                               float* hAccum, float* hDenoised, uint8_t* hRgba, SrtTemporalStats* stats) {
  if (!ctx) return 1;
  if (!pIn) return fail(ctx, "temporal: null render parameters");
  DenoiseArgs dcheck;
  TemporalArgs tcheck;
  int iterations = 0;
  if (checkDenoiseParams(ctx, d, pIn->imageWidth, pIn->imageHeight, dcheck, iterations, true)) return 1;
  if (checkTemporalParams(ctx, t, pIn->imageWidth, pIn->imageHeight, tcheck)) return 1;
  if (pIn->countStats) return fail(ctx, "render: the moments entries have no counting variant (countStats must be 0)");
  FrameStage f(ctx, "temporal", pIn);
  if (checkParams(ctx, &f.p) || f.begin()) return 1;
  const int W = f.p.imageWidth, H = f.p.imageHeight;
  if (f.reserve(f.tiles, f.tileBytes) || f.reserve(f.mtiles, f.tileBytes) || f.reserve(f.accum, f.imageBytes) || f.reserve(f.mom, f.imageBytes) ||
      f.reserve(f.accOut, f.imageBytes) || f.reserve(f.momOut, f.imageBytes))
    return 1;
  if (f.reserveDenoised(hDenoised, hRgba) || f.reserveFeatures(SRT_FEATURE_ALL)) return 1;
  const void* histIn;
  void* histOut;
  bool useMotion;
  if (beginTemporalFrame(ctx, W, H, t->demodulate != 0, true, &histIn, &histOut, &useMotion)) return 1;
  if (useMotion && (f.reserve(f.motionTiles, f.tileBytes) || f.reserve(f.motionImage, f.imageBytes))) return 1;
  if (f.render() || f.features(SRT_FEATURE_ALL) || (useMotion && f.motion())) return 1;
  if (srtTemporalAccumulateImpl(ctx, t, W, H, f.accum.get(), f.mom.get(), f.dPlanes, f.motionImage.get(), &ctx->camFull, &ctx->temporalCam, histIn,
                                f.accOut.get(), f.momOut.get(), histOut, nullptr))
    return 1;
  if (f.denoise(d, f.accOut, true, f.momOut) || f.finish()) return 1;
  commitTemporalFrame(ctx, W, H, t->demodulate != 0);
  if (f.copyOut(hAccum, f.accum, f.imageBytes, "accum") || f.copyOut(hDenoised, f.out, f.imageBytes, "denoised") ||
      f.copyOut(hRgba, f.outRgba, f.nPix * 4, "rgba"))
    return 1;
  return stats && temporalStats(ctx, f.nPix, f.accum.get(), f.accOut.get(), histOut, stats);
}

// srtRenderTemporalAdaptiveFrame (guided: srtRenderTemporalAdaptiveGuidedFrame): the feature planes of the first p.spp
// samples -- the rounds' reprojection needs them before the first decision --, srtRenderTemporalAdaptive on the context's
// history, the denoiser on the accumulated sums
int srtRenderTemporalAdaptiveFrameImpl(SrtContext* ctx, const SrtRenderParams* pIn, const SrtAdaptiveParams* ap,
                                       const SrtDenoiseParams* d, const SrtTemporalParams* t, float* hAccum, float* hDenoised,
                                       uint8_t* hRgba, SrtTemporalAdaptiveStats* stats, bool guided = false) {
  if (!ctx) return 1;
  if (checkAdaptive(ctx, pIn, ap, false, nullptr, nullptr)) return 1;
  DenoiseArgs dcheck;
  TemporalArgs tcheck;
  int iterations = 0;
  if (checkDenoiseParams(ctx, d, pIn->imageWidth, pIn->imageHeight, dcheck, iterations, true)) return 1;
  if (checkTemporalParams(ctx, t, pIn->imageWidth, pIn->imageHeight, tcheck)) return 1;
  FrameStage f(ctx, "temporal", pIn, false);
  if (f.begin()) return 1;
  const int W = f.p.imageWidth, H = f.p.imageHeight;
  if (f.reserve(f.accum, f.imageBytes) || f.reserve(f.mom, f.imageBytes) || f.reserve(f.accOut, f.imageBytes) || f.reserve(f.momOut, f.imageBytes))
    return 1;
  if (f.reserveDenoised(hDenoised, hRgba) || f.reserveFeatures(SRT_FEATURE_ALL)) return 1;
  const void* histIn;
  void* histOut;
  if (beginTemporalFrame(ctx, W, H, t->demodulate != 0, false, &histIn, &histOut)) return 1;
  if (f.features(SRT_FEATURE_ALL)) return 1;
  if (srtRenderTemporalAdaptiveImpl(ctx, &f.p, ap, t, f.dPlanes, &ctx->temporalCam, histIn, f.accum.get(), f.mom.get(), f.accOut.get(),
                                    f.momOut.get(), histOut, stats, nullptr, guided))
    return 1;
  if (f.denoise(d, f.accOut, true, f.momOut) || f.finish()) return 1;
  commitTemporalFrame(ctx, W, H, t->demodulate != 0);
  return f.copyOut(hAccum, f.accum, f.imageBytes, "accum") || f.copyOut(hDenoised, f.out, f.imageBytes, "denoised") ||
         f.copyOut(hRgba, f.outRgba, f.nPix * 4, "rgba");
}

// srtRenderDirectImage: the frame through the device-path entries with direct light sampling.  Per batch of sample indices:
// srtCameraRaysDevice without a list (entries pixel-major), srtTracePathsDirectDevice, and the running sum of every pixel's
// samples in sample-index order (srt_direct.hip); then the adaptive entries' image-order quantisation.  The three buffers of
// a batch hold 60 bytes per entry; samplesPerBatch = 0 keeps a batch at 2^22 entries (240 MB) at most.
int srtRenderDirectImageImpl(SrtContext* ctx, const SrtRenderParams* pIn, int32_t samplesPerBatch, float* hAccum, uint8_t* hRgba) {
  if (!ctx) return 1;
  if (!pIn) return fail(ctx, "direct: null parameters");
  if (samplesPerBatch < 0) return fail(ctx, "direct: samplesPerBatch = %d is negative", samplesPerBatch);
  FrameStage f(ctx, "direct", pIn);
  if (checkParams(ctx, &f.p) || f.begin()) return 1;
  const int64_t nPix = (int64_t)f.nPix;
  int64_t batch = samplesPerBatch > 0 ? samplesPerBatch : std::max<int64_t>(1, ((int64_t)1 << 22) / nPix);
  batch = std::min<int64_t>(batch, f.p.spp);
  if (nPix * batch > 0x7fffffffll) return fail(ctx, "direct: %lld entries per batch do not fit: lower samplesPerBatch", (long long)(nPix * batch));
  DeviceBuffer rays, rng, result, scratch;
  const size_t entries = (size_t)(nPix * batch);
  if (f.reserve(rays, entries * 36) || f.reserve(rng, entries * 8) || f.reserve(result, entries * 16) || f.reserve(scratch, SRT_PATHS_SCRATCH_BYTES) ||
      f.reserve(f.accum, f.imageBytes) || (hRgba && f.reserve(f.rgba, f.nPix * 4)))
    return 1;
  if (hipMemsetAsync(f.accum.get(), 0, f.imageBytes, nullptr) != hipSuccess) return fail(ctx, "direct: memset");
  const int grid = planEntryGrid(ctx->prop.multiProcessorCount, nPix);
  for (int32_t first = 0; first < f.p.spp; first += (int32_t)batch) {
    SrtRenderParams q = f.p;
    q.spp = (int32_t)std::min<int64_t>(batch, f.p.spp - first);
    q.sampleFirst = f.p.sampleFirst + first;
    const int64_t n = nPix * q.spp;
    if (srtCameraRaysDevice(ctx, &q, nullptr, n, rays.get(), rng.get(), nullptr)) return 1;
    if (srtTracePathsDirectDevice(ctx, f.p.traversal, f.p.maxBounce, f.p.background, rays.get(), n, rng.get(), result.get(), scratch.get(), nullptr)) return 1;
    const int e = srt_launch_direct_sum(result.get<const int4>(), f.accum.get<float4>(), nPix, q.spp, grid, nullptr);
    if (e) return fail(ctx, "direct: launch failed: %s", hipGetErrorString((hipError_t)e));
  }
  if (hRgba) {
    const int e = srt_launch_adaptive_resolve(f.accum.get<const float4>(), f.rgba.get<uint8_t>(), (int)f.nPix, nullptr);
    if (e) return fail(ctx, "direct: launch failed: %s", hipGetErrorString((hipError_t)e));
  }
  if (f.finish()) return 1;
  return f.copyOut(hRgba, f.rgba, f.nPix * 4, "rgba") || f.copyOut(hAccum, f.accum, f.imageBytes, "accum");
}

/* include/srt_hip_test.h: the render kernel's own traversal, ray by ray */
int srtRenderAovImpl(SrtContext* ctx, const SrtRenderParams* pIn, int32_t depth, SrtAovRecord* hOut) {
  if (!ctx || !pIn || !hOut || depth < 0) return 1;
  FrameStage f(ctx, "aov", pIn);
  f.p.spp = 1;
  f.p.sppChunks = 1;
  f.p.countStats = 1;
  if (checkParams(ctx, &f.p) || f.begin()) return 1;
  DeviceBuffer aov;
  const size_t aovBytes = f.nPix * sizeof(SrtAovRecord);
  if (f.reserve(f.tiles, f.tileBytes) || f.reserve(aov, aovBytes)) return 1;
  if (hipMemset(aov.get(), 0, aovBytes) != hipSuccess) return fail(ctx, "aov: memset");
  if (srtRenderTilesImpl(ctx, &f.p, f.tiles.get(), nullptr, aov.get<SrtAovRecord>(), depth) || f.finish()) return 1;
  return f.copyOut(hOut, aov, aovBytes, "out");
}

}  // namespace

extern "C" {

int srtRenderImage(SrtContext* ctx, const SrtRenderParams* p, float* hAccum, uint8_t* hRgba) {
  if (!ctx || !p) return 1;
  return renderImage(ctx, p, hAccum, nullptr, hRgba, false);
}
int srtRenderImageMoments(SrtContext* ctx, const SrtRenderParams* p, float* hAccum, float* hMoments, uint8_t* hRgba) {
  SRT_GUARDED(ctx, srtRenderImageMomentsImpl(ctx, p, hAccum, hMoments, hRgba));
}
int srtRenderAdaptiveImage(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, float* hAccum, float* hMoments,
                           uint8_t* hRgba, SrtAdaptiveStats* stats) {
  SRT_GUARDED(ctx, srtRenderAdaptiveImageImpl(ctx, p, ap, hAccum, hMoments, hRgba, stats));
}
int srtRenderFeatureImage(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, float* const hPlanes[4]) {
  SRT_GUARDED(ctx, srtRenderFeatureImageImpl(ctx, p, planes, hPlanes));
}
int srtRenderMotionImage(SrtContext* ctx, const SrtRenderParams* p, float* hMotion) {
  SRT_GUARDED(ctx, srtRenderMotionImageImpl(ctx, p, hMotion));
}
int srtRenderDenoisedImage(SrtContext* ctx, const SrtRenderParams* p, const SrtDenoiseParams* d, float* hAccum,
                           float* hDenoised, uint8_t* hRgba) {
  SRT_GUARDED(ctx, srtRenderDenoisedImageImpl(ctx, p, d, hAccum, hDenoised, hRgba));
}
int srtRenderDenoisedImageMoments(SrtContext* ctx, const SrtRenderParams* p, const SrtDenoiseParams* d, float* hAccum,
                                  float* hMoments, float* hDenoised, uint8_t* hRgba) {
  SRT_GUARDED(ctx, srtRenderDenoisedImageImpl(ctx, p, d, hAccum, hDenoised, hRgba, true, hMoments));
}
int srtRenderAdaptiveDenoisedImage(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, const SrtDenoiseParams* d,
                                   float* hAccum, float* hMoments, float* hDenoised, uint8_t* hRgba, SrtAdaptiveStats* stats) {
  SRT_GUARDED(ctx, srtRenderAdaptiveDenoisedImageImpl(ctx, p, ap, d, hAccum, hMoments, hDenoised, hRgba, stats));
}
int srtRenderTemporalFrame(SrtContext* ctx, const SrtRenderParams* p, const SrtDenoiseParams* d, const SrtTemporalParams* t,
                           float* hAccum, float* hDenoised, uint8_t* hRgba, SrtTemporalStats* stats) {
  SRT_GUARDED(ctx, srtRenderTemporalFrameImpl(ctx, p, d, t, hAccum, hDenoised, hRgba, stats));
}
int srtRenderTemporalAdaptiveFrame(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, const SrtDenoiseParams* d,
                                   const SrtTemporalParams* t, float* hAccum, float* hDenoised, uint8_t* hRgba,
                                   SrtTemporalAdaptiveStats* stats) {
  SRT_GUARDED(ctx, srtRenderTemporalAdaptiveFrameImpl(ctx, p, ap, d, t, hAccum, hDenoised, hRgba, stats));
}
int srtRenderTemporalAdaptiveGuidedFrame(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap,
                                         const SrtDenoiseParams* d, const SrtTemporalParams* t, float* hAccum, float* hDenoised,
                                         uint8_t* hRgba, SrtTemporalAdaptiveStats* stats) {
  SRT_GUARDED(ctx, srtRenderTemporalAdaptiveFrameImpl(ctx, p, ap, d, t, hAccum, hDenoised, hRgba, stats, true));
}
int srtRenderDirectImage(SrtContext* ctx, const SrtRenderParams* p, int32_t samplesPerBatch, float* hAccum, uint8_t* hRgba) {
  SRT_GUARDED(ctx, srtRenderDirectImageImpl(ctx, p, samplesPerBatch, hAccum, hRgba));
}
int srtRenderAov(SrtContext* ctx, const SrtRenderParams* p, int32_t depth, SrtAovRecord* hOut) { SRT_GUARDED(ctx, srtRenderAovImpl(ctx, p, depth, hOut)); }

}  // extern "C"
