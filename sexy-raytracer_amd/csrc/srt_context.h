// srt_context.h -- the context behind the C ABI's SrtContext* and what the host translation units share around it: error
// reporting, and the device-level entries (srt_api.cpp, srt_render.cpp, srt_passes.cpp) that each other and the whole-frame
// entries (srt_frames.cpp) compose.  The entries on the caller's device buffers (srt_rays.cpp) use the context, the error
// reporting and checkSceneReady, and nothing composes them.  Internal: none of this is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "srt_buffer.h"
#include "srt_device.h"
#include "srt_plan.h"  // Tunables, the planner
#include "srt_scene.h"

// What belongs to the uploaded scene and is invalid for the next one.  srtUploadScene starts by assigning a fresh Upload,
// which also frees the previous scene's device memory; a member added here can therefore not survive into the next scene.
// (Work areas sized by need, the camera, the temporal history and the tunables are the context's, below.)
struct Upload {
  std::vector<DeviceBuffer> sceneBuffers;
  DevScene scene{};
  bool haveScene = false;
  // host copies for srtGetBvh
  std::vector<std::vector<SrtBvhNode>> itemNodes;
  std::vector<DeviceBuild> deviceBuilds;  // where the device-built trees live in scene.nodes (without their host refs)
  // srtRebuildScene builds them again as the upload did: each build's refs on the device (4 B per primitive), the PLOC
  // radius the upload read, and the depths over the host-built trees alone, to take the maxima again
  std::vector<DeviceBuffer> buildRefs;    // [k] belongs to deviceBuilds[k]
  int plocRadius = 0;
  int hostStackDepth = 0, hostBvhDepth = 0;
  std::vector<int32_t> hostTriPrimId, hostSphPrimId;
  // direct light sampling (srt_scene.h sampledLights): the table on the device -- device sphere indices, which the kernels
  // get beside their other arguments -- and as prims[] indices for srtGetSampledLights.  Materials never change in an
  // update, so it is the upload's
  const int32_t* sampledLights = nullptr;
  std::vector<int32_t> sampledLightPrims;
  int bvhDepth = 0;
  // srtUpdateTriangles / srtUpdateSpheres / srtRefitScene (srt_refit_host.cpp).  Every tree of the world list with its node
  // slots and times, the host tables the upload left (moved to the device by the first call that needs them), and the
  // refit's per-scene device tables: parent links, arrival counters, the hybrid records' renumbering.
  struct Tree {
    int32_t item, base, count;
    float time0, time1;
    bool deviceBuilt;
  };
  std::vector<Tree> trees;
  std::vector<int32_t> hostTriDevIndex, hostWfIndex;  // HostScene::triDevIndex, wfIndex
  std::vector<uint8_t> itemBoxesStale;                // per world item: itemNodes holds boxes from before a refit
  DeviceBuffer triDevIndex, wfIndex, refitUp, refitArrived;
  DeviceBuffer refitUpRg;           // the regrouped tree's parent links (scene.nodesRg): refitted in the same pass
  bool refitTables = false;         // refitUp, refitArrived (and wfIndex) exist for this scene
  bool refitLinksStale = false;     // refitUp is not of the current topology: srtRebuildScene has built trees since
  bool geometryDirty = false;       // an update since the last refit: nothing renders
  float pairTime0 = 0, pairTime1 = 0;  // the times the closest-hit pair records were made for
  int32_t fastDivOption = 0;        // SceneOptions::fastDiv of the upload: what fastDivScene is while the certificate holds
  // srtSetMotionTracking: triTest and spheres as of the previous srtRefitScene (or the upload), copied by the first update
  // of an epoch before its kernel, or by a refit that no update preceded.  48 B per triangle and per sphere.
  DeviceBuffer prevTriTest, prevSpheres;
  bool haveSnapshot = false;   // the two buffers hold a snapshot (until then "previous" is the current tables)
  bool epochSnapshot = false;  // ... taken since the last refit: later updates of the epoch leave it alone
};

struct SrtContext {
  int device = 0;
  std::string error;
  Tunables tun{};
  hipDeviceProp_t prop;
  Upload upload;  // the uploaded scene
  DevCamera cam{};
  bool haveCamera = false;
  // work areas
  DeviceBuffer refitFlag, refitStage;  // srtRefitScene's certificate flag word, the host update entries' staging
  DeviceBuffer costScratch;            // srtGetTreeCost: the partial sums of its levels
  DeviceBuffer dQueue;
  DeviceBuffer dStats;
  void* comm = nullptr;          // ncclComm_t (srt_comm.cpp)
  int commRanks[2] = {1, 0};     // number of ranks, this rank
  DeviceBuffer chunkScratch;
  DeviceBuffer attScratch;  // LDS-resident-tree kernel: the lanes' attenuation stacks (srt_render_kernel LDSTREE)
  DeviceBuffer wfPool, wfAttHi;  // path-pool kernel: contexts and upper attenuation levels (srt_wavefront.hip)
  int32_t* dWfError = nullptr;
  DeviceBuffer dFeatureCounter;  // the feature passes' tile counter (their own: a render's queues are never touched)
  DeviceBuffer denoiseScratch;   // srtDenoise: guide records, depth gradients, two colour buffers (56 B per pixel)
  DeviceBuffer tileTable;   // RenderArgs::tileXY for the image size and tile order below
  // srtRenderAdaptive: one launch's beauty and moments tiles, two tile lists (this launch's, the next one's), the per-tile
  // flags and the compaction's {count, pixels}
  DeviceBuffer adaptTiles, adaptList[2], adaptFlags, adaptCounts;
  // srtRenderTemporalFrame: the two histories (the one the last frame wrote, the one the next writes), what they belong to,
  // and the camera as srtSetCamera received it (DevCamera drops w)
  DeviceBuffer temporalHistory[2];
  DeviceBuffer temporalReprojected;  // srtRenderTemporalAdaptive: the frame's reprojected history (32 B per pixel)
  int32_t temporalCurrent = 0;  // index of the history the last frame wrote
  bool temporalValid = false;
  int32_t temporalKey[3] = {0, 0, 0};  // width, height, demodulate
  SrtCamera camFull{}, temporalCam{};
  bool motionTracking = false;     // srtSetMotionTracking: the context's, like the tunables
  int32_t temporalRefits = 0;      // srtRefitScene calls with tracking on since the last committed temporal frame
  int32_t tileTableKey[3] = {0, 0, 0};
  RenderPlan lastPlan{};  // the most recent render launch (srtGetLaunchInfo)
  int32_t lastGrid = 0;
  hipEvent_t evStart = nullptr, evStop = nullptr;
  bool timed = false;
};

// Records the text in the context (srtLastError), reports it on stderr and returns 1
int fail(SrtContext* ctx, const char* fmt, ...);

// A path-pool launch that gave up (a ring wait exceeded its bound, srt_wavefront.hip) has added to the context's error
// word: the frame is incomplete.  Checked wherever the host has waited for the device anyway.
int wfCheck(SrtContext* ctx);

#define HIP_OK(ctx, call)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) return fail(ctx, "%s -> %s", #call, hipGetErrorString(e_));       \
  } while (0)

// No exception crosses the C boundary (std::vector / std::string allocations may throw).
#define SRT_GUARDED(ctx, call)                                                  \
  try {                                                                         \
    return (call);                                                              \
  } catch (const std::exception& e) {                                           \
    return fail(ctx, "%s: %s", __func__, e.what());                             \
  } catch (...) {                                                               \
    return fail(ctx, "%s: unknown exception", __func__);                        \
  }

// srtRenderTemporalAdaptive: the decisions pool the frame's moments with this reprojected history (srt_temporal_adaptive.hip)
struct AdaptivePool {
  const float4* reprojected;  // two planes, SRT_TEMPORAL_REPROJECTED_BYTES_PER_PIXEL
  const float4* albedo;       // null unless the history is demodulated
};

// srtRenderAdaptiveGuided / srtRenderTemporalAdaptiveGuided: image-order feature planes that follow the rounds
// (srt_features_list.hip): after launch r its list and sample range go through the list kernel
struct AdaptiveGuides {
  int32_t planes;       // SRT_FEATURE_* bits
  void* const* images;  // [4], float4[W*H] for every selected bit
  bool storeFirst;      // round 0 is stored over the whole tile table; false: the planes hold round 0 already
};

// The fields a launch over the image shares (RenderArgs, FeatureArgs): the scene, the camera, the image, its samples and
// the tile split; everything else zero.
template <typename Args>
void setImageArgs(Args& a, const SrtContext* ctx, const SrtRenderParams* p) {
  memset(&a, 0, sizeof a);
  a.scene = ctx->upload.scene;
  a.cam = ctx->cam;
  a.imageWidth = p->imageWidth;
  a.imageHeight = p->imageHeight;
  a.tilesX = (p->imageWidth + SRT_TILE_W - 1) / SRT_TILE_W;
  a.tilesY = (p->imageHeight + SRT_TILE_H - 1) / SRT_TILE_H;
  a.tileBlock = std::max(1, ctx->tun.tileBlock);  // the tile order every render and srtResolveTiles use
  a.numTiles = srtNumTiles(p->imageWidth, p->imageHeight);
  a.spp = p->spp;
  a.sampleFirst = p->sampleFirst;
  a.seed = p->seed;
  memcpy(a.background, p->background, 12);
  a.tMin = p->tMin;
  a.tileFirst = p->tileFirst;
  a.tileStride = p->tileStride;
  a.numLocalTiles = srtNumLocalTiles(p->imageWidth, p->imageHeight, p->tileStride);
}

// The device-level entries behind the exported ones and their argument checks (srt_api.cpp, srt_render.cpp, srt_passes.cpp,
// where each is described)
int checkParams(SrtContext* ctx, const SrtRenderParams* p);
// "no scene uploaded", or an update that srtRefitScene has not followed: `what` names the entry.  Launches nothing.
int checkSceneReady(SrtContext* ctx, const char* what);
// The trees of the device-built items from the current records, and the scene's depths (srt_api.cpp).  Blocking.
int buildDeviceTrees(SrtContext* ctx);
int srtRenderTilesImpl(SrtContext* ctx, const SrtRenderParams* p, void* dAccumTiles, void* streamPtr,
                       SrtAovRecord* aov = nullptr, int32_t aovDepth = 0, void* dMoments = nullptr,
                       const uint32_t* dList = nullptr, int32_t listTiles = 0);
int checkAdaptive(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, bool device, const void* dAccum,
                  const void* dMoments);
int srtRenderAdaptiveImpl(SrtContext* ctx, const SrtRenderParams* pIn, const SrtAdaptiveParams* ap, void* dAccumImage,
                          void* dMomentsImage, void* dRgba, SrtAdaptiveStats* stats, void* streamPtr,
                          const AdaptivePool* pool = nullptr, const AdaptiveGuides* guides = nullptr);
int checkFeatureArgs(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, const void* const* buffers);
int srtRenderFeatureTilesImpl(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, void* const dPlanes[4], void* streamPtr);
int srtRenderFeatureTileListImpl(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, const void* dTileList,
                                 int32_t numListed, void* const dPlaneImages[4], int32_t accumulate, void* streamPtr);
int checkDenoiseParams(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, DenoiseArgs& a,
                       int& iterations, bool moments = false);
int srtDenoiseImpl(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, const void* dBeauty,
                   const void* const dPlanes[4], void* dOut, void* dRgba, void* streamPtr, bool moments = false,
                   const void* dMoments = nullptr);
int checkTemporalParams(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, TemporalArgs& a);
int srtRenderMotionTilesImpl(SrtContext* ctx, const SrtRenderParams* p, void* dMotionTiles, void* streamPtr);
// dMotion: the resolved motion plane (srtTemporalAccumulateMotion), or null for srtTemporalAccumulate
int srtTemporalAccumulateImpl(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* dBeauty,
                              const void* dMoments, const void* const dPlanes[4], const void* dMotion, const SrtCamera* cam,
                              const SrtCamera* prevCam, const void* dHistoryIn, void* dBeautyOut, void* dMomentsOut,
                              void* dHistoryOut, void* streamPtr);
int temporalStats(SrtContext* ctx, size_t nPix, const void* dCurrent, const void* dAccumulated, const void* dHistory,
                  SrtTemporalStats* stats);
int srtRenderTemporalAdaptiveImpl(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap,
                                  const SrtTemporalParams* t, const void* const dPlanes[4], const SrtCamera* prevCam,
                                  const void* dHistoryIn, void* dAccumImage, void* dMomentsImage, void* dBeautyOut,
                                  void* dMomentsOut, void* dHistoryOut, SrtTemporalAdaptiveStats* stats, void* streamPtr,
                                  bool guided = false);
