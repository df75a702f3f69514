// srt_plan.h -- how a render launch is shaped, as pure functions of plain inputs: which form of the render kernel runs and
// over which LDS layout (srt_lds_layout.h), the path-pool kernel's rings, pool and grid, the cut of the work into queues,
// units and chunks, the wave scheduler's defaults.  No SrtContext and no HIP call: srt_render.cpp gathers the inputs, asks
// here, and allocates and launches what the plan says; examples/plan_probe.cpp asks here without a device
// (tests/test_plan_host.py).  Internal.
#pragma once
#include <hip/hip_runtime.h>  // (float4 and friends of srt_device.h's structs; nothing is called)

#include "srt_device.h"

// Diagnostic tunables of the work distribution and the wave scheduler.  Environment variables give the
// defaults ONCE, at srtCreate; srtSetTunable (include/srt_hip_test.h) changes them per context.  -1 = the
// library's own rule.
struct Tunables {
  int tileBlock, unitTiles, queues;
  int shadeMin, primMin, hitMin, fuseMin, nodeBurst;
  int plocRadius, fastDiv;
  int chunkScratchMb;
  int primAgainMin;
  int keepEighths;
  int ldsTree;
  int wavefront, wfPool, wfSwapMin, wfSwapBig, wfProfile;
  int wfHybrid, wfResidentMax, wfFarRounds;
  int wfRegroup, wfHead;
  int denoiseLdsStep;
  int triCert;
  int pathsRefillMin;
};

// What the planner reads of the uploaded scene (DevScene)
struct SceneFacts {
  int32_t numNodes;
  int32_t wfResident;  // the hybrid records' nodes kept in LDS
  int32_t numWorld;
  int32_t stackDepth;
  bool threadLinks;    // DevScene::nodeThread: host-built trees, 15-bit references (srt_scene.cpp flattenScene)
  bool hybridRecords;  // DevScene::nodesWf
  bool classTable;     // DevScene::primClass
};
inline SceneFacts sceneFacts(const DevScene& sc) {
  return {sc.numNodes, sc.wfResident, sc.numWorld, sc.stackDepth, sc.nodeThread != nullptr, sc.nodesWf != nullptr, sc.primClass != nullptr};
}

// One render launch, whole: the kernel (RenderPlan), the work split and the scheduler thresholds as RenderArgs takes them,
// and for the path-pool forms their grid and pool.  Forms 0-2 get their grid from planGrid once the occupancy is known.
struct LaunchPlan {
  RenderPlan render;
  bool fitsLds;  // render.lds <= SRT_LDS_BYTES; otherwise nothing can be launched (a deep tree on the stack form)
  int32_t numLocalTiles;
  int32_t sppChunks;  // srtPlanSppChunks: -1 when an explicit count does not fit, and then nothing below is set
  int32_t unitTiles, numQueues, numUnits, numWork;
  int32_t shadeMin, primMin, hitMin, fuseMin, nodeBurst, primAgainMin, keepEighths;
  int32_t wfGrid, wfPoolSize, wfSwapMin, wfSwapBig, wfFarRounds;  // path-pool forms only
};

// moments: srtRenderTilesMoments -- the same form, grid, block and LDS, its MOMENTS instance (never counting or profiling).
// listTiles >= 0: a launch over a tile list of that length (srtRenderAdaptive) instead of the rank's share of the image.
RenderPlan planRender(const SceneFacts& sc, const Tunables& tun, int numCUs, const SrtRenderParams* p, bool moments, int32_t listTiles);
LaunchPlan planLaunch(const SceneFacts& sc, const Tunables& tun, int numCUs, const SrtRenderParams* p, bool moments, int32_t listTiles);
// persistent waves: enough workgroups to fill every CU, never more than there is work
int planGrid(int numCUs, int perCU, int32_t numWork, int32_t block);
// the plan's share of RenderArgs: the work split with what the kernels derive from it, and the scheduler thresholds
void setPlanArgs(RenderArgs& a, const LaunchPlan& lp);
// The grid of the kernels that serve one entry per thread, SRT_BLOCK threads a workgroup, striding over what eight
// workgroups per CU do not cover (srtTraceRays, the ray queries, the path steps)
int planEntryGrid(int numCUs, int64_t n);

// RenderArgs::fixLimit of a render of `chunks` chunks (srt_path.h toFixed36): exact chunk sums cannot wrap, partial sums of
// 2^26 / (chunk count rounded up to a power of two) or more count as infinite.  The render and srtTestChunkSum both ask here.
float chunkFixLimit(int32_t chunks);
