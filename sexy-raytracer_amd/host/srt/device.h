// device.h -- hipDevice: the working counterpart of the reference's disabled glDevice seam
// (gl.h:16-40: init / rtFrame / terminate; main.cpp:190-199,231).
//   init(w, h, world)                       flatten (populate) + upload to HBM
//   rtFrame(target, w, h, cam, bg, spp, b)  render the frame into the caller-owned RGBA8 target
//   rtFeatures(cam, bg, spp, seed, ...)     the feature pass of the same frame: albedo / normal / position / depth at
//                                           the first hit of the camera rays rtFrame traces (a denoiser's guides)
//   rtFrameDenoised(target, denoised, ...)  rtFrame's frame, its feature pass and the library's a-trous denoiser: the
//                                           noisy and the denoised RGBA8 frames of one render
//   rtFrameTemporal(denoised, ..., sampleFirst)  one frame of a sequence: rtFrameDenoised's frame accumulated onto the
//                                           reprojected history of the previous call before it is denoised
//                                           (include/srt_hip.h "Temporal accumulation"); temporalReset() starts over
//   rtFrameTemporalAdaptive(denoised, ..., sppMax, thr, sampleFirst)  rtFrameTemporal with rtFrameAdaptive's rounds deciding
//                                           on the frame's samples pooled with the reprojected history
//                                           (include/srt_hip.h "Temporal-adaptive frames")
//   rtFrameAdaptive(target, ..., sppMax, thr)  tile-adaptive sampling: numSamples everywhere, then more samples, doubling,
//                                           for the tiles that have not converged (include/srt_hip.h "Adaptive sampling")
//   rtFrameAdaptiveDenoised(target, denoised, ..., sppMax, thr)  rtFrameAdaptive's frame, guide planes from every one of its
//                                           samples and the denoiser with the sample variance
//                                           (include/srt_hip.h srtRenderAdaptiveDenoisedImage)
//   updateTriangles(first, tris) / updateSpheres(first, spheres) / refit()  moving geometry: new positions for
//                                           primitives of the uploaded scene (`triangles` keeps what init uploaded, in the
//                                           scene's order), then every tree's boxes refitted on the device
//                                           (include/srt_hip.h "Moving geometry"); nothing renders between the two
//   rebuild() / treeCost(item, cost)        srtRebuildScene / srtGetTreeCost.  This layer builds reference trees only (on
//                                           the host), and those a rebuild refits: here rebuild() IS refit().  treeCost
//                                           tells how far the motion has inflated an item's boxes
//   terminate()
//   uniqueId / initRanks                    multi-GPU: one process per GPU; rtFrame then renders this rank's
//                                           tiles, the library gathers them with ONE ncclGather and rank 0's
//                                           target receives the frame (include/srt_hip.h "Multi-GPU")
// Returns bool and reports on std::cerr like the reference.  There is no CPU fallback.
#ifndef SRT_HOST_DEVICE_H
#define SRT_HOST_DEVICE_H

#include <cmath>
#include <iostream>
#include <vector>

#include "camera.h"
#include "hittablelist.h"

class hipDevice {
 public:
  hipDevice() {}
  ~hipDevice() { terminate(); }
  hipDevice(const hipDevice&) = delete;

  bool init(int w, int h, const hittableList& world, int deviceOrdinal = 0) {
    width = w;
    height = h;
    if (srtCreate(deviceOrdinal, &ctx) != 0) {
      std::cerr << "ERROR: no usable HIP device\n";
      ctx = nullptr;
      return false;
    }
    sceneFlattener f;
    world.populate(f);
    SrtSceneDesc d = f.desc();
    if (srtUploadScene(ctx, &d) != 0) return error();
    numPrims = (int)f.prims.size();
    triangles = f.triangles;
    return true;
  }

  // Moving geometry (include/srt_hip.h srtUpdateTriangles / srtUpdateSpheres / srtRefitScene)
  bool updateTriangles(int first, const std::vector<SrtTriangleIn>& tris) {
    if (!ctx) return false;
    return srtUpdateTriangles(ctx, first, (int32_t)tris.size(), tris.data()) == 0 || error();
  }
  bool updateSpheres(int first, const std::vector<SrtSphereIn>& s) {
    if (!ctx) return false;
    return srtUpdateSpheres(ctx, first, (int32_t)s.size(), s.data()) == 0 || error();
  }
  bool refit() {
    if (!ctx) return false;
    return srtRefitScene(ctx, nullptr) == 0 || error();
  }
  // srtRebuildScene builds the device-built trees anew; init() uploads none (every item is a reference tree built on the
  // host), so this is a refit.  It is here for callers written against the library's moving-geometry loop.
  bool rebuild() {
    if (!ctx) return false;
    return srtRebuildScene(ctx, nullptr) == 0 || error();
  }
  // The sum of world item `item`'s node box areas over its root's (include/srt_hip.h srtGetTreeCost), after init or refit
  bool treeCost(int item, double& cost) {
    if (!ctx) return false;
    return srtGetTreeCost(ctx, item, &cost) == 0 || error();
  }

  // Motion tracking (include/srt_hip.h "Motion"): the geometry of the previous refit stays on the device, so that
  // rtFrameTemporal keeps its history across one update + refit and rtMotion has a displacement to report.  Call order:
  // init, setMotionTracking(true), then per frame updateTriangles / updateSpheres, refit, rtFrameTemporal.
  bool setMotionTracking(bool enable) {
    if (!ctx) return false;
    return srtSetMotionTracking(ctx, enable ? 1 : 0) == 0 || error();
  }
  // The motion plane of the frame rtFrameTemporal renders with the same numSamples, seed and sampleFirst: float[w*h*4] in
  // image order, xyz = the mean displacement back to the previous refit's geometry, w = the hit count.  Renders the size
  // init was given.
  bool rtMotion(const camera& cam, const color3f& background, int numSamples, uint64_t seed, int firstSample, std::vector<float>& motion) {
    if (!ctx) return false;
    if (srtSetCamera(ctx, &cam.data()) != 0) return error();
    SrtRenderParams p{};
    p.imageWidth = width; p.imageHeight = height; p.spp = numSamples; p.seed = seed;
    for (int i = 0; i < 3; ++i) p.background[i] = background(i);
    p.tMin = 0.001f;  // main.cpp:39
    p.traversal = SRT_TRAVERSE_FAITHFUL;
    p.tileFirst = 0; p.tileStride = 1;
    p.sampleFirst = firstSample;
    motion.assign((size_t)width * height * 4, 0.0f);
    return srtRenderMotionImage(ctx, &p, motion.data()) == 0 || error();
  }

  // Multi-GPU.  Rank 0 obtains an id (128 bytes) and hands it to the other processes by its own means;
  // every process then calls initRanks after init.  Single-process programs never call these.
  static bool uniqueId(void* id128) { return srtCommGetUniqueId(id128) == 0; }
  bool initRanks(const void* id128, int numRanks, int rank) {
    if (!ctx) return false;
    if (srtCommInit(ctx, id128, numRanks, rank) != 0) return error();
    ranks = numRanks;
    return true;
  }

  // the pixel loop main.cpp:200-227 for the whole frame; frameData = uint8[w*h*4] (main.cpp:182)
  bool rtFrame(void* frameData, int w, int h, const camera& cam, const color3f& background, int numSamples,
               int maxBounce, uint64_t seed = 1, float* accum = nullptr) {
    if (!ctx) return false;
    if (srtSetCamera(ctx, &cam.data()) != 0) return error();
    SrtRenderParams p{};
    p.imageWidth = w; p.imageHeight = h; p.spp = numSamples; p.maxBounce = maxBounce; p.seed = seed;
    for (int i = 0; i < 3; ++i) p.background[i] = background(i);
    p.tMin = 0.001f;  // main.cpp:39
    p.traversal = SRT_TRAVERSE_FAITHFUL;
    p.tileFirst = 0; p.tileStride = 1;
    p.sppChunks = sppChunks;
    if (ranks > 1) {  // collective: every rank renders its tiles, one gather, rank 0 fills its target
      if (srtRenderImageRanks(ctx, &p, accum, static_cast<uint8_t*>(frameData)) != 0) return error();
    } else if (srtRenderImage(ctx, &p, accum, static_cast<uint8_t*>(frameData)) != 0) {
      return error();
    }
    (void)srtLastKernelMs(ctx, &lastKernelMs);
    return true;
  }

  // rtFrame with direct light sampling (include/srt_hip.h srtRenderDirectImage): the same image in expectation from other
  // samples -- at every pbr hit one of the scene's solid-colour light spheres is sampled.  Single-process only.
  bool rtFrameDirect(void* frameData, int w, int h, const camera& cam, const color3f& background, int numSamples, int maxBounce,
                     uint64_t seed = 1, float* accum = nullptr) {
    if (!ctx) return false;
    if (ranks > 1) {
      std::cerr << "ERROR: rtFrameDirect renders on one GPU\n";
      return false;
    }
    if (srtSetCamera(ctx, &cam.data()) != 0) return error();
    SrtRenderParams p{};
    p.imageWidth = w; p.imageHeight = h; p.spp = numSamples; p.maxBounce = maxBounce; p.seed = seed;
    for (int i = 0; i < 3; ++i) p.background[i] = background(i);
    p.tMin = 0.001f;  // main.cpp:39
    p.traversal = SRT_TRAVERSE_FAITHFUL;
    p.tileFirst = 0; p.tileStride = 1;
    if (srtRenderDirectImage(ctx, &p, 0, accum, static_cast<uint8_t*>(frameData)) != 0) return error();
    return true;
  }

  // Tile-adaptive sampling (include/srt_hip.h "Adaptive sampling"): numSamples (>= 2) samples everywhere, then doubling rounds
  // for the tiles not yet converged to the display-space standard error `threshold`, up to sppMax samples a pixel.
  // frameData = uint8[w*h*4] (may be null), accum = float[w*h*4] sums with per-pixel counts (may be null), stats may be null.
  // Single-process only.
  bool rtFrameAdaptive(void* frameData, int w, int h, const camera& cam, const color3f& background, int numSamples,
                       int maxBounce, int sppMax, float threshold, uint64_t seed = 1, float* accum = nullptr,
                       SrtAdaptiveStats* stats = nullptr) {
    if (!ctx) return false;
    if (ranks > 1) {
      std::cerr << "ERROR: rtFrameAdaptive renders on one GPU\n";
      return false;
    }
    if (srtSetCamera(ctx, &cam.data()) != 0) return error();
    SrtRenderParams p{};
    p.imageWidth = w; p.imageHeight = h; p.spp = numSamples; p.maxBounce = maxBounce; p.seed = seed;
    for (int i = 0; i < 3; ++i) p.background[i] = background(i);
    p.tMin = 0.001f;  // main.cpp:39
    p.traversal = SRT_TRAVERSE_FAITHFUL;
    p.tileFirst = 0; p.tileStride = 1;
    p.sppChunks = sppChunks;
    SrtAdaptiveParams a{};
    a.sppMax = sppMax;
    a.threshold = threshold;
    if (srtRenderAdaptiveImage(ctx, &p, &a, accum, nullptr, static_cast<uint8_t*>(frameData), stats) != 0) return error();
    (void)srtLastKernelMs(ctx, &lastKernelMs);
    return true;
  }

  // rtFrameAdaptive plus the denoiser (include/srt_hip.h srtRenderAdaptiveDenoisedImage): the adaptive render, feature planes
  // that follow its rounds (every sample of a tile guides the filter) and srtDenoiseMoments on the sums.  frameData (may be
  // null) receives the frame rtFrameAdaptive would write, denoisedData (may be null) the denoised one; accum / denoised
  // (float[w*h*4], may be null) the sums with per-pixel counts and the denoised means.  d = null: the library's defaults.
  // Single-process only.
  bool rtFrameAdaptiveDenoised(void* frameData, void* denoisedData, int w, int h, const camera& cam, const color3f& background,
                               int numSamples, int maxBounce, int sppMax, float threshold, uint64_t seed = 1,
                               const SrtDenoiseParams* d = nullptr, float* accum = nullptr, float* denoised = nullptr,
                               SrtAdaptiveStats* stats = nullptr) {
    if (!ctx) return false;
    if (ranks > 1) {
      std::cerr << "ERROR: rtFrameAdaptiveDenoised renders on one GPU\n";
      return false;
    }
    if (srtSetCamera(ctx, &cam.data()) != 0) return error();
    SrtRenderParams p{};
    p.imageWidth = w; p.imageHeight = h; p.spp = numSamples; p.maxBounce = maxBounce; p.seed = seed;
    for (int i = 0; i < 3; ++i) p.background[i] = background(i);
    p.tMin = 0.001f;  // main.cpp:39
    p.traversal = SRT_TRAVERSE_FAITHFUL;
    p.tileFirst = 0; p.tileStride = 1;
    p.sppChunks = sppChunks;
    SrtAdaptiveParams a{};
    a.sppMax = sppMax;
    a.threshold = threshold;
    const SrtDenoiseParams defaults{};
    std::vector<float> sums;
    if (!accum && frameData) {
      sums.resize((size_t)w * h * 4);
      accum = sums.data();
    }
    if (srtRenderAdaptiveDenoisedImage(ctx, &p, &a, d ? d : &defaults, accum, nullptr, denoised, static_cast<uint8_t*>(denoisedData),
                                       stats) != 0)
      return error();
    (void)srtLastKernelMs(ctx, &lastKernelMs);
    if (frameData) {  // srtRenderAdaptive's quantisation of the sums, each pixel with its own count
      uint8_t* px = static_cast<uint8_t*>(frameData);
      for (size_t i = 0; i < (size_t)w * h; ++i) {
        const float scale = 1.0f / accum[4 * i + 3];
        for (int c = 0; c < 3; ++c) {
          const float g = std::sqrt(accum[4 * i + c] * scale);
          const float q = 256.0f * (g < 0.0f ? 0.0f : (g > 0.999f ? 0.999f : g));
          px[4 * i + c] = (q == q) ? (uint8_t)q : (uint8_t)0;  // NaN -> 0
        }
        px[4 * i + 3] = 255;
      }
    }
    return true;
  }

  // Feature planes of the frame rtFrame renders with the same numSamples and seed (include/srt_hip.h "Feature pass"):
  // each non-null vector receives float[w*h*4] in image order, xyz = the mean over the samples that counted, w = their
  // count.  Renders the size init was given.
  bool rtFeatures(const camera& cam, const color3f& background, int numSamples, uint64_t seed, std::vector<float>* albedo,
                  std::vector<float>* normal, std::vector<float>* position = nullptr, std::vector<float>* depth = nullptr) {
    if (!ctx) return false;
    if (srtSetCamera(ctx, &cam.data()) != 0) return error();
    SrtRenderParams p{};
    p.imageWidth = width; p.imageHeight = height; p.spp = numSamples; p.seed = seed;
    for (int i = 0; i < 3; ++i) p.background[i] = background(i);
    p.tMin = 0.001f;  // main.cpp:39
    p.traversal = SRT_TRAVERSE_FAITHFUL;
    p.tileFirst = 0; p.tileStride = 1;
    std::vector<float>* planes[4] = {albedo, normal, position, depth};
    float* out[4] = {nullptr, nullptr, nullptr, nullptr};
    int32_t mask = 0;
    for (int k = 0; k < 4; ++k) {
      if (!planes[k]) continue;
      planes[k]->assign((size_t)width * height * 4, 0.0f);
      out[k] = planes[k]->data();
      mask |= 1 << k;
    }
    if (mask == 0) return true;
    if (srtRenderFeatureImage(ctx, &p, mask, out) != 0) return error();
    return true;
  }

  // rtFrame plus the denoiser (include/srt_hip.h "Denoiser"): frameData (may be null) receives the frame rtFrame would
  // write, denoisedData (may be null) the denoised frame with the same quantisation; accum / denoised (float[w*h*4], may be
  // null) the sums with counts and the denoised means.  d = null: the library's defaults.  sampleVariance: the denoiser's
  // noise estimate from the render's own samples (srtRenderDenoisedImageMoments) instead of the spatial one; the frame and
  // the sums are the same either way.  Single-process only.
  bool rtFrameDenoised(void* frameData, void* denoisedData, int w, int h, const camera& cam, const color3f& background,
                       int numSamples, int maxBounce, uint64_t seed = 1, const SrtDenoiseParams* d = nullptr,
                       float* accum = nullptr, float* denoised = nullptr, bool sampleVariance = false) {
    if (!ctx) return false;
    if (ranks > 1) {
      std::cerr << "ERROR: rtFrameDenoised renders on one GPU\n";
      return false;
    }
    if (srtSetCamera(ctx, &cam.data()) != 0) return error();
    SrtRenderParams p{};
    p.imageWidth = w; p.imageHeight = h; p.spp = numSamples; p.maxBounce = maxBounce; p.seed = seed;
    for (int i = 0; i < 3; ++i) p.background[i] = background(i);
    p.tMin = 0.001f;  // main.cpp:39
    p.traversal = SRT_TRAVERSE_FAITHFUL;
    p.tileFirst = 0; p.tileStride = 1;
    p.sppChunks = sppChunks;
    p.sampleFirst = sampleFirst;
    const SrtDenoiseParams defaults{};
    std::vector<float> sums;
    if (!accum && frameData) {
      sums.resize((size_t)w * h * 4);
      accum = sums.data();
    }
    const int rc = sampleVariance ? srtRenderDenoisedImageMoments(ctx, &p, d ? d : &defaults, accum, nullptr, denoised,
                                                                  static_cast<uint8_t*>(denoisedData))
                                  : srtRenderDenoisedImage(ctx, &p, d ? d : &defaults, accum, denoised, static_cast<uint8_t*>(denoisedData));
    if (rc != 0) return error();
    (void)srtLastKernelMs(ctx, &lastKernelMs);
    if (frameData) {  // the resolve's quantisation (color.h:25-41) of the sums
      uint8_t* px = static_cast<uint8_t*>(frameData);
      const float scale = 1.0f / (float)numSamples;
      for (size_t i = 0; i < (size_t)w * h; ++i) {
        for (int c = 0; c < 3; ++c) {
          const float g = std::sqrt(accum[4 * i + c] * scale);
          const float q = 256.0f * (g < 0.0f ? 0.0f : (g > 0.999f ? 0.999f : g));
          px[4 * i + c] = (q == q) ? (uint8_t)q : (uint8_t)0;  // NaN -> 0
        }
        px[4 * i + 3] = 255;
      }
    }
    return true;
  }

  // One frame of a camera move (include/srt_hip.h srtRenderTemporalFrame): samples [sampleFirst, sampleFirst + numSamples)
  // with `cam`, accumulated onto the history the previous call left (reprojected from its camera), then denoised with the
  // sample variance.  denoisedData (may be null) receives the RGBA8 frame, accum / denoised (float[w*h*4], may be null)
  // this frame's own sums and the denoised means.  d, t = null: the library's defaults.  Callers advance sampleFirst by
  // numSamples per frame so that every frame draws fresh samples.  Single-process only.
  bool rtFrameTemporal(void* denoisedData, int w, int h, const camera& cam, const color3f& background, int numSamples,
                       int maxBounce, int sampleFirst, uint64_t seed = 1, const SrtDenoiseParams* d = nullptr,
                       const SrtTemporalParams* t = nullptr, float* accum = nullptr, float* denoised = nullptr,
                       SrtTemporalStats* stats = nullptr) {
    if (!ctx) return false;
    if (ranks > 1) {
      std::cerr << "ERROR: rtFrameTemporal renders on one GPU\n";
      return false;
    }
    if (srtSetCamera(ctx, &cam.data()) != 0) return error();
    SrtRenderParams p{};
    p.imageWidth = w; p.imageHeight = h; p.spp = numSamples; p.maxBounce = maxBounce; p.seed = seed;
    for (int i = 0; i < 3; ++i) p.background[i] = background(i);
    p.tMin = 0.001f;  // main.cpp:39
    p.traversal = SRT_TRAVERSE_FAITHFUL;
    p.tileFirst = 0; p.tileStride = 1;
    p.sppChunks = sppChunks;
    p.sampleFirst = sampleFirst;
    const SrtDenoiseParams ddefaults{};
    const SrtTemporalParams tdefaults{};
    if (srtRenderTemporalFrame(ctx, &p, d ? d : &ddefaults, t ? t : &tdefaults, accum, denoised, static_cast<uint8_t*>(denoisedData),
                               stats) != 0)
      return error();
    (void)srtLastKernelMs(ctx, &lastKernelMs);
    return true;
  }

  // rtFrameTemporal with history-steered sampling (include/srt_hip.h srtRenderTemporalAdaptiveFrame): numSamples (>= 2)
  // samples everywhere from sampleFirst, then doubling rounds, up to sppMax samples a pixel, for the tiles whose samples and
  // reprojected history together are not yet below the display-space standard error `threshold`.  Buffers, d and t as in
  // rtFrameTemporal; accum carries per-pixel counts.  Callers advance sampleFirst by sppMax per frame.  Frames of both
  // kinds may follow one another.  guided: the feature planes follow the rounds (srtRenderTemporalAdaptiveGuidedFrame), so
  // the closing accumulation, the new history and the denoiser see guides from all of a tile's samples.  Single-process only.
  bool rtFrameTemporalAdaptive(void* denoisedData, int w, int h, const camera& cam, const color3f& background, int numSamples,
                               int maxBounce, int sppMax, float threshold, int sampleFirst, uint64_t seed = 1,
                               const SrtDenoiseParams* d = nullptr, const SrtTemporalParams* t = nullptr, float* accum = nullptr,
                               float* denoised = nullptr, SrtTemporalAdaptiveStats* stats = nullptr, bool guided = false) {
    if (!ctx) return false;
    if (ranks > 1) {
      std::cerr << "ERROR: rtFrameTemporalAdaptive renders on one GPU\n";
      return false;
    }
    if (srtSetCamera(ctx, &cam.data()) != 0) return error();
    SrtRenderParams p{};
    p.imageWidth = w; p.imageHeight = h; p.spp = numSamples; p.maxBounce = maxBounce; p.seed = seed;
    for (int i = 0; i < 3; ++i) p.background[i] = background(i);
    p.tMin = 0.001f;  // main.cpp:39
    p.traversal = SRT_TRAVERSE_FAITHFUL;
    p.tileFirst = 0; p.tileStride = 1;
    p.sppChunks = sppChunks;
    p.sampleFirst = sampleFirst;
    SrtAdaptiveParams a{};
    a.sppMax = sppMax;
    a.threshold = threshold;
    const SrtDenoiseParams ddefaults{};
    const SrtTemporalParams tdefaults{};
    const auto entry = guided ? srtRenderTemporalAdaptiveGuidedFrame : srtRenderTemporalAdaptiveFrame;
    if (entry(ctx, &p, &a, d ? d : &ddefaults, t ? t : &tdefaults, accum, denoised, static_cast<uint8_t*>(denoisedData), stats) != 0)
      return error();
    (void)srtLastKernelMs(ctx, &lastKernelMs);
    return true;
  }
  bool temporalReset() { return ctx && srtTemporalReset(ctx) == 0; }

  bool trace(const std::vector<SrtRay>& rays, std::vector<SrtHit>& hits) {
    hits.resize(rays.size());
    if (!ctx || srtTraceRays(ctx, rays.data(), (int64_t)rays.size(), hits.data(), SRT_TRAVERSE_FAITHFUL) != 0) return error();
    return true;
  }

  void terminate() {
    if (ctx) srtDestroy(ctx);
    ctx = nullptr;
  }

 public:
  int sampleFirst = 0;  // rtFrameDenoised: the first sample index of the frame (frame k of a sequence: k * numSamples)
  int sppChunks = 0;  // 0 = library default; 1 = the reference's single running sum per pixel
  float lastKernelMs = 0;
  int numPrims = 0;
  std::vector<SrtTriangleIn> triangles;  // the uploaded scene's triangles, in its own order (updateTriangles' indices)

 private:
  bool error() {
    std::cerr << "ERROR: " << (ctx ? srtLastError(ctx) : "no context") << "\n";
    return false;
  }
  SrtContext* ctx = nullptr;
  int width = 0, height = 0;
  int ranks = 1;
};

#endif
