// srt_render.cpp -- the render launches of the C ABI (include/srt_hip.h): the launch srt_plan.cpp plans, over the rank's
// tiles or a tile list, the moments instance, the resolve, the ray-level test entries, and the rounds of tile-adaptive
// sampling.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "srt_context.h"
#include "srt_launch.h"
#include "srt_lds_layout.h"

int checkParams(SrtContext* ctx, const SrtRenderParams* p) {
  if (checkSceneReady(ctx, "render")) return 1;
  if (!ctx->haveCamera) return fail(ctx, "render: no camera set");
  if (p->imageWidth < 2 || p->imageHeight < 2) return fail(ctx, "render: image must be at least 2x2 (u,v divide by W-1,H-1)");
  if (p->imageWidth > 65535 * SRT_TILE_W || p->imageHeight > 65535 * SRT_TILE_H) return fail(ctx, "render: image larger than 65535 tiles a side");
  if (p->spp < 1) return fail(ctx, "render: spp must be >= 1");
  if (p->sampleFirst < 0 || (int64_t)p->sampleFirst + p->spp > 0x7fffffff) return fail(ctx, "render: bad sample range");
  if (p->maxBounce < 0 || p->maxBounce > SRT_MAX_BOUNCE) return fail(ctx, "render: maxBounce must be in [0,%d]", SRT_MAX_BOUNCE);
  if (p->tileStride < 1 || p->tileFirst < 0 || p->tileFirst >= p->tileStride) return fail(ctx, "render: bad tile split %d/%d", p->tileFirst, p->tileStride);
  if (p->sppChunks < 0 || p->sppChunks > p->spp) return fail(ctx, "render: sppChunks must be in [0, spp] (0 = library default)");
  return 0;
}

// The tile order as a device table (once per image size): the kernel's restart step looks a tile up instead of dividing
static int tileTableFor(SrtContext* ctx, const SrtRenderParams* p, const RenderArgs& a) {
  if (ctx->tileTableKey[0] == p->imageWidth && ctx->tileTableKey[1] == p->imageHeight && ctx->tileTableKey[2] == a.tileBlock && ctx->tileTable.get()) return 0;
  std::vector<uint32_t> table((size_t)a.numTiles);
  for (int32_t i = 0; i < a.numTiles; ++i) {
    int tx, ty;
    srtTileFromOrder(i, a.tilesX, a.tilesY, a.tileBlock, tx, ty);
    table[i] = (uint32_t)tx | (uint32_t)ty << 16;
  }
  ctx->tileTable = DeviceBuffer();  // freed first (as a size change always did), then allocated for this size
  HIP_OK(ctx, ctx->tileTable.reserve(std::max<size_t>(table.size() * 4, 16)));
  HIP_OK(ctx, hipMemcpy(ctx->tileTable.get(), table.data(), table.size() * 4, hipMemcpyHostToDevice));
  ctx->tileTableKey[0] = p->imageWidth;
  ctx->tileTableKey[1] = p->imageHeight;
  ctx->tileTableKey[2] = a.tileBlock;
  return 0;
}

// Where a launch of more than one chunk leaves its partial sums: a.out / a.chunkStride (scratch path, returns scratchPath =
// true) or a.fix (atomic path), and with `moments` a.mout / a.mfix behind them.
// Chunk sums are added exactly (srt_kernels.hip "Chunk sums").  Scratch path (a float4 slot per item, summed by
// srt_sum_chunks_kernel) while this rank's slots fit the budget, else the atomic path (32 B per pixel, 0.4-1 %
// slower); the two give the same bits, so the choice may differ from rank to rank.
static int chunkSumBuffers(SrtContext* ctx, RenderArgs& a, bool moments, size_t tilePixels, hipStream_t stream, bool& scratchPath) {
  // a moments launch sums its moments plane exactly as the beauty, on the same path: twice the slots or accumulators,
  // the beauty's first, the moments' behind them
  const size_t planes = moments ? 2 : 1;
  const size_t localSlots = planes * tilePixels * a.sppChunks * sizeof(float4);
  // budget: the tunable, and never more than a quarter of what the device has free right now (a smaller, shared or
  // partitioned GPU takes the atomic path -- same bits -- instead of failing)
  size_t budget = (size_t)std::max(0, ctx->tun.chunkScratchMb) * 1024 * 1024, freeB = 0, totalB = 0;
  if (ctx->chunkScratch.bytes() < localSlots && hipMemGetInfo(&freeB, &totalB) == hipSuccess) budget = std::min(budget, (freeB + ctx->chunkScratch.bytes()) / 4);
  scratchPath = localSlots <= budget;
  const size_t need = scratchPath ? localSlots : planes * tilePixels * sizeof(SrtFixedAccum);
  if (ctx->chunkScratch.reserve(need) != hipSuccess) {
    (void)hipGetLastError();
    if (!scratchPath) return fail(ctx, "render: cannot allocate %zu B for the pixel sums", need);
    scratchPath = false;  // the slots do not fit after all: 32 B per pixel on the atomic path
    HIP_OK(ctx, ctx->chunkScratch.reserve(planes * tilePixels * sizeof(SrtFixedAccum)));
  }
  if (scratchPath) {
    a.out = ctx->chunkScratch.get<float4>();
    a.chunkStride = (int32_t)tilePixels;
    if (moments) a.mout = a.out + tilePixels * a.sppChunks;
  } else {
    a.fix = ctx->chunkScratch.get<SrtFixedAccum>();
    if (moments) a.mfix = a.fix + tilePixels;
    HIP_OK(ctx, hipMemsetAsync(a.fix, 0, planes * tilePixels * sizeof(SrtFixedAccum), stream));
  }
  return 0;
}

// aov: srtRenderAov's per-pixel records of the ray at bounce aovDepth (counting launches only), else null.
// dMoments: srtRenderTilesMoments's plane (the MOMENTS instance of the planned form), else null.
// dList: a DEVICE table of listTiles tiles (tx | ty << 16) to render instead of the rank's share of the image
// (srtRenderAdaptive; p->tileFirst = 0, p->tileStride = 1): the output holds list position i where it holds local tile i,
// and the queues, the grid and the chunk scratch follow the list's length.  The render kernels see an ordinary launch
// whose tile table is the list.
int srtRenderTilesImpl(SrtContext* ctx, const SrtRenderParams* p, void* dAccumTiles, void* streamPtr, SrtAovRecord* aov,
                                    int32_t aovDepth, void* dMoments, const uint32_t* dList, int32_t listTiles) {
  // ---- check
  if (!ctx || !p || !dAccumTiles) return 1;
  if (checkParams(ctx, p)) return 1;
  if (dList && (listTiles < 1 || listTiles > srtNumTiles(p->imageWidth, p->imageHeight) || p->tileStride != 1))
    return fail(ctx, "render: bad tile list of %d tiles", listTiles);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  const bool moments = dMoments != nullptr;
  // ---- plan: the kernel and its LDS, the work split, the scheduler thresholds (srt_plan.cpp: arithmetic alone)
  const LaunchPlan lp = planLaunch(sceneFacts(ctx->upload.scene), ctx->tun, ctx->prop.multiProcessorCount, p, moments, dList ? listTiles : -1);
  const RenderPlan& plan = lp.render;
  RenderArgs a;
  setImageArgs(a, ctx, p);
  if (dList) a.numTiles = a.numLocalTiles = listTiles;
  a.maxBounce = p->maxBounce;
  if (lp.sppChunks < 1) return fail(ctx, "render: sppChunks %d x %d tiles exceeds 2^31 work items", p->sppChunks, a.numTiles);
  if (!lp.fitsLds) return fail(ctx, "render: BVH depth %d needs %zu B of LDS per workgroup", ctx->upload.scene.stackDepth, plan.lds);
  setPlanArgs(a, lp);
  // ---- tile table
  if (!dList && tileTableFor(ctx, p, a)) return 1;
  a.tileXY = dList ? dList : ctx->tileTable.get<const uint32_t>();
  a.queue = ctx->dQueue.get<int32_t>();
  // (a moments launch neither counts nor profiles: its mout / mfix take the places of aov / stats, RenderArgs)
  unsigned long long* const stats = !moments && (p->countStats || ctx->tun.wfProfile > 0) ? ctx->dStats.get<unsigned long long>() : nullptr;
  a.stats = stats;
  a.aov = p->countStats ? aov : nullptr;
  a.aovDepth = aovDepth;
  // ---- chunk-sum buffers
  const size_t tilePixels = (size_t)a.numLocalTiles * SRT_TILE_PIXELS;
  a.out = static_cast<float4*>(dAccumTiles);
  a.fix = nullptr;
  if (moments) a.mout = static_cast<float4*>(dMoments);
  a.chunkStride = 0;
  bool scratchPath = false;
  if (a.sppChunks > 1 && chunkSumBuffers(ctx, a, moments, tilePixels, stream, scratchPath)) return 1;
  // The regrouped tree (srt_regroup.h) is walked by the whole-tree path-pool form alone, never by a counting launch, and
  // only while every box is ordered (its lemma's condition: a refit may have lost it)
  if (plan.form != SRT_FORM_PATH_POOL || plan.count || ctx->tun.wfRegroup <= 0 || !a.scene.boxOrderedScene) a.scene.nodesRg = nullptr, a.scene.nodeThreadRg = nullptr;
  // Its walk sequence (tunable 2): the kernel's set-up copy takes the kept records alone, and walks start at the entry
  // words behind them, handed over in the world list's place (srt_wf_links.h: srtWfRootWord leaves an entry word as it is;
  // the path-pool kernel reads `world` for nothing else), so the kernel holds no value it did not hold before
  if (!a.scene.nodesRg || ctx->tun.wfRegroup < 2 || !a.scene.walkSeq)
    a.scene.walkSeq = nullptr, a.scene.numWalk = 0, a.scene.wfHead = 0;
  else
    a.scene.world = a.scene.walkSeq + 3 * (size_t)a.scene.numWalk;
  // ... and the head of its walks (DevScene::wfHead) goes with it, unless the tunable "wf_head" takes it out
  if (ctx->tun.wfHead <= 0) a.scene.wfHead = 0;
  const bool pathPool = srtFormIsPathPool(plan.form);
  const RenderKernel kernel = pathPool ? srt_render_wf_kernel_for(&plan) : srt_render_kernel_for(&plan);
  if (plan.lds > 64 * 1024)
    HIP_OK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
  // persistent waves: as many workgroups as the CUs hold (the path-pool kernel: one each, planned)
  int perCU = 1;
  if (!pathPool && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, plan.block, plan.lds) != hipSuccess || perCU < 1)) perCU = 1;
  const int grid = pathPool ? lp.wfGrid : planGrid(ctx->prop.multiProcessorCount, perCU, a.numWork, plan.block);
  // ---- pool buffers
  if (pathPool) {
    HIP_OK(ctx, ctx->wfPool.reserve((size_t)grid * lp.wfPoolSize * 128));
    const int hiLevels = std::max(0, p->maxBounce - 4);
    HIP_OK(ctx, ctx->wfAttHi.reserve(std::max<size_t>(16, (size_t)grid * 3 * hiLevels * lp.wfPoolSize * sizeof(float))));
    a.wfPool = ctx->wfPool.get<char>();
    a.wfAttHi = ctx->wfAttHi.get<float>();
    HIP_OK(ctx, hipHostGetDevicePointer((void**)&a.wfError, ctx->dWfError, 0));
  } else if (plan.form == SRT_FORM_LDS_TREE) {
    HIP_OK(ctx, ctx->attScratch.reserve((size_t)srtAttSlots(p->maxBounce) * grid * SRT_BLOCK_TREE * sizeof(float)));
    a.attScratch = ctx->attScratch.get<float>();
  }
  // ---- launch
  HIP_OK(ctx, hipMemsetAsync(a.queue, 0, sizeof(int32_t) * 16 * a.numQueues, stream));
  if (stats) HIP_OK(ctx, hipMemsetAsync(stats, 0, 96 * sizeof(unsigned long long), stream));
  HIP_OK(ctx, hipEventRecord(ctx->evStart, stream));
  ctx->lastPlan = plan;
  ctx->lastGrid = grid;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(plan.block), plan.lds, stream, a);
  int rc = (int)hipGetLastError();
  if (rc) return fail(ctx, "render launch failed: %s", hipGetErrorString((hipError_t)rc));
  HIP_OK(ctx, hipEventRecord(ctx->evStop, stream));
  ctx->timed = true;
  // ---- finalise: the exact sums of the chunks' partial sums
  if (a.fix) {
    rc = srt_launch_finalize(a.fix, static_cast<float4*>(dAccumTiles), (int)tilePixels, a.spp, stream);
    if (!rc && moments) rc = srt_launch_finalize(a.mfix, static_cast<float4*>(dMoments), (int)tilePixels, a.spp, stream);
    if (rc) return fail(ctx, "finalize launch failed: %s", hipGetErrorString((hipError_t)rc));
  } else if (scratchPath) {
    rc = srt_launch_sum_chunks(a.out, static_cast<float4*>(dAccumTiles), (int)tilePixels, a.sppChunks, a.fixLimit, stream);
    if (!rc && moments) rc = srt_launch_sum_chunks(a.mout, static_cast<float4*>(dMoments), (int)tilePixels, a.sppChunks, a.fixLimit, stream);
    if (rc) return fail(ctx, "chunk sum launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
  return 0;
}

// srtRenderTilesMoments's own checks, before anything is launched
static int checkMoments(SrtContext* ctx, const SrtRenderParams* p, const void* dMoments) {
  if (!ctx) return 1;
  if (!p) return fail(ctx, "render: null parameters");
  if (!dMoments) return fail(ctx, "render: null moments buffer");
  if (p->countStats) return fail(ctx, "render: the moments entries have no counting variant (countStats must be 0)");
  return 0;
}

static int srtRenderTilesMomentsImpl(SrtContext* ctx, const SrtRenderParams* p, void* dAccumTiles, void* dMomentTiles,
                                     void* streamPtr) {
  if (checkMoments(ctx, p, dMomentTiles)) return 1;
  if (!dAccumTiles) return fail(ctx, "render: null accumulator buffer");
  return srtRenderTilesImpl(ctx, p, dAccumTiles, streamPtr, nullptr, 0, dMomentTiles);
}

// ---------------------------------------------------------------- adaptive sampling (include/srt_hip.h)

// The schedule: b_0 = n_0, then b_r = min(n_{r-1}, sppMax - n_{r-1}) until n = sppMax.
static int adaptiveSchedule(int32_t n0, int32_t sppMax, int32_t* spp) {
  int rounds = 0;
  int32_t n = n0;
  spp[rounds++] = n0;
  while (n < sppMax && rounds < SRT_ADAPTIVE_MAX_ROUNDS) {
    const int32_t b = std::min(n, sppMax - n);
    spp[rounds++] = b;
    n += b;
  }
  return rounds;
}

int checkAdaptive(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, bool device,
                               const void* dAccum, const void* dMoments) {
  if (!ctx) return 1;
  if (!p || !ap) return fail(ctx, "adaptive: null parameters");
  if (device && (!dAccum || !dMoments)) return fail(ctx, "adaptive: the beauty and moments buffers are required");
  if (p->countStats) return fail(ctx, "adaptive: no counting variant (countStats must be 0)");
  if (p->tileFirst != 0 || p->tileStride != 1) return fail(ctx, "adaptive: renders on one GPU (tileFirst 0, tileStride 1)");
  if (p->spp < 2) return fail(ctx, "adaptive: spp (the first round) must be >= 2");
  if (ap->sppMax < p->spp || ap->sppMax > SRT_ADAPTIVE_MAX_SPP) return fail(ctx, "adaptive: sppMax must be in [spp, 2^24]");
  if (p->sampleFirst < 0 || (int64_t)p->sampleFirst + ap->sppMax > 0x7fffffff) return fail(ctx, "adaptive: bad sample range");
  if (!(ap->threshold >= 0.0f)) return fail(ctx, "adaptive: threshold must be >= 0 (+inf allowed)");
  if (checkParams(ctx, p)) return 1;
  // every launch's chunk plan, before anything is launched
  int32_t spp[SRT_ADAPTIVE_MAX_ROUNDS];
  const int rounds = adaptiveSchedule(p->spp, ap->sppMax, spp);
  for (int r = 0; r < rounds; ++r) {
    const int32_t chunks = p->sppChunks > 0 ? std::min(p->sppChunks, spp[r]) : 0;
    if (srtPlanSppChunks(p->imageWidth, p->imageHeight, spp[r], chunks) < 1)
      return fail(ctx, "adaptive: sppChunks %d x %d tiles exceeds 2^31 work items", chunks, srtNumTiles(p->imageWidth, p->imageHeight));
  }
  return 0;
}

int srtRenderAdaptiveImpl(SrtContext* ctx, const SrtRenderParams* pIn, const SrtAdaptiveParams* ap, void* dAccumImage,
                                       void* dMomentsImage, void* dRgba, SrtAdaptiveStats* stats, void* streamPtr,
                                       const AdaptivePool* pool, const AdaptiveGuides* guides) {
  if (checkAdaptive(ctx, pIn, ap, true, dAccumImage, dMomentsImage)) return 1;
  if (guides && checkFeatureArgs(ctx, pIn, guides->planes, guides->images)) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  const SrtRenderParams p0 = *pIn;
  const int W = p0.imageWidth, H = p0.imageHeight;
  const int32_t numTiles = srtNumTiles(W, H);
  const size_t tilePixels = (size_t)numTiles * SRT_TILE_PIXELS;
  HIP_OK(ctx, ctx->adaptTiles.reserve(2 * tilePixels * sizeof(float4)));
  for (auto& l : ctx->adaptList) HIP_OK(ctx, l.reserve((size_t)numTiles * sizeof(uint32_t)));
  HIP_OK(ctx, ctx->adaptFlags.reserve((size_t)numTiles * sizeof(int32_t)));
  HIP_OK(ctx, ctx->adaptCounts.reserve(2 * sizeof(int32_t)));
  float4* const beautyTiles = ctx->adaptTiles.get<float4>();
  float4* const momentTiles = beautyTiles + tilePixels;
  float4* const accum = static_cast<float4*>(dAccumImage);
  float4* const moments = static_cast<float4*>(dMomentsImage);
  const double thr = (double)ap->threshold;
  const double limit = 4.0 * (thr * thr);
  SrtAdaptiveStats st;
  memset(&st, 0, sizeof st);
  int32_t spp[SRT_ADAPTIVE_MAX_ROUNDS];
  const int plannedRounds = adaptiveSchedule(p0.spp, ap->sppMax, spp);
  // round 0: the whole frame, srtRenderImageMoments's launch and resolves
  const uint32_t* list = nullptr;  // this launch's tiles (round 0: the image's own tile table)
  int32_t listTiles = numTiles, listPixels = W * H;
  int32_t n = 0;
  for (int r = 0; r < plannedRounds; ++r) {
    SrtRenderParams q = p0;
    q.spp = spp[r];
    q.sampleFirst = p0.sampleFirst + n;
    q.sppChunks = p0.sppChunks > 0 ? std::min(p0.sppChunks, spp[r]) : 0;
    if (srtRenderTilesImpl(ctx, &q, beautyTiles, stream, nullptr, 0, momentTiles, list, list ? listTiles : 0)) return 1;
    n += spp[r];
    st.roundSpp[r] = spp[r];
    st.roundTiles[r] = listTiles;
    st.pixelSamples += (int64_t)listPixels * spp[r];
    st.rounds = r + 1;
    int rc = 0;
    const bool decide = n < ap->sppMax;
    if (r == 0) {
      if (srtResolveTiles(ctx, &q, beautyTiles, nullptr, accum, stream) || srtResolveTiles(ctx, &q, momentTiles, nullptr, moments, stream))
        return 1;
      list = ctx->tileTable.get<const uint32_t>();  // built for this size by the launch above
    }
    // the guide planes of the same tiles over the same samples: stored in round 0, added from round 1 on
    if (guides && (r > 0 || guides->storeFirst) &&
        srtRenderFeatureTileListImpl(ctx, &q, guides->planes, list, listTiles, guides->images, r > 0, stream))
      return 1;
    if (pool && decide)
      rc = srt_launch_temporal_adaptive_update(list, listTiles, beautyTiles, momentTiles, accum, moments, pool->reprojected,
                                               pool->albedo, ctx->adaptFlags.get<int32_t>(), W, H, limit, r > 0, stream);
    else if (r > 0 || decide)
      rc = srt_launch_adaptive_update(list, listTiles, beautyTiles, momentTiles, accum, moments, ctx->adaptFlags.get<int32_t>(),
                                      W, H, limit, r > 0, decide, stream);
    uint32_t* const next = ctx->adaptList[r & 1].get<uint32_t>();
    int32_t counts[2] = {0, 0};
    if (!rc && decide)
      rc = srt_launch_adaptive_compact(list, ctx->adaptFlags.get<const int32_t>(), listTiles, next, ctx->adaptCounts.get<int32_t>(),
                                       W, H, stream);
    if (rc) return fail(ctx, "adaptive launch failed: %s", hipGetErrorString((hipError_t)rc));
    if (decide) HIP_OK(ctx, hipMemcpyAsync(counts, ctx->adaptCounts.get(), sizeof counts, hipMemcpyDeviceToHost, stream));
    if (hipStreamSynchronize(stream) != hipSuccess) return fail(ctx, "render kernel failed: %s", hipGetErrorString(hipGetLastError()));
    if (wfCheck(ctx)) return 1;
    HIP_OK(ctx, hipEventElapsedTime(&st.roundMs[r], ctx->evStart, ctx->evStop));
    if (!decide || counts[0] == 0) break;
    list = next;
    listTiles = counts[0];
    listPixels = counts[1];
  }
  if (dRgba) {
    const int rc = srt_launch_adaptive_resolve(accum, static_cast<uint8_t*>(dRgba), W * H, stream);
    if (rc) return fail(ctx, "adaptive resolve launch failed: %s", hipGetErrorString((hipError_t)rc));
    if (hipStreamSynchronize(stream) != hipSuccess) return fail(ctx, "adaptive resolve failed: %s", hipGetErrorString(hipGetLastError()));
  }
  if (stats) *stats = st;
  return 0;
}

static int srtRenderAdaptiveGuidedImpl(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, int32_t planes,
                                       void* const dPlaneImages[4], void* dAccumImage, void* dMomentsImage, void* dRgba,
                                       SrtAdaptiveStats* stats, void* stream) {
  if (!ctx) return 1;
  const AdaptiveGuides guides{planes, dPlaneImages, true};
  return srtRenderAdaptiveImpl(ctx, p, ap, dAccumImage, dMomentsImage, dRgba, stats, stream, nullptr, &guides);
}

extern "C" {

int srtResolveTiles(SrtContext* ctx, const SrtRenderParams* p, const void* dGathered, void* dRgba, void* dAccumImage,
                    void* streamPtr) {
  if (!ctx || !p || !dGathered) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  ResolveArgs a;
  a.gathered = static_cast<const float4*>(dGathered);
  a.imageWidth = p->imageWidth;
  a.imageHeight = p->imageHeight;
  a.tilesX = (p->imageWidth + SRT_TILE_W - 1) / SRT_TILE_W;
  a.tileBlock = std::max(1, ctx->tun.tileBlock);
  a.tileStride = p->tileStride < 1 ? 1 : p->tileStride;
  a.numLocalTiles = srtNumLocalTiles(p->imageWidth, p->imageHeight, a.tileStride);
  a.spp = p->spp;
  a.rgba = static_cast<uint8_t*>(dRgba);
  a.accumImage = static_cast<float4*>(dAccumImage);
  int rc = srt_launch_resolve(&a, static_cast<hipStream_t>(streamPtr));
  if (rc) return fail(ctx, "resolve launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

int srtTraceRays(SrtContext* ctx, const SrtRay* rays, int64_t n, SrtHit* hits, int32_t traversal) {
  if (!ctx || !rays || !hits || n < 0) return 1;
  if (checkSceneReady(ctx, "trace")) return 1;
  if (n == 0) return 0;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  DeviceBuffer dRays, dHits;
  if (dRays.reserve(n * sizeof(SrtRay)) != hipSuccess || dHits.reserve(n * sizeof(SrtHit)) != hipSuccess) return fail(ctx, "trace: hipMalloc");
  if (hipMemcpy(dRays.get(), rays, n * sizeof(SrtRay), hipMemcpyHostToDevice) != hipSuccess) return fail(ctx, "trace: copy in");
  TraceArgs a;
  a.scene = ctx->upload.scene;
  a.rays = dRays.get<const SrtRay>();
  a.hits = dHits.get<SrtHit>();
  a.n = n;
  // srtTestGetTriUndecided's count of this call: a word of the statistics area that no render launch writes
  a.triUndecided = ctx->dStats.get<unsigned long long>() + SRT_STATS_TRI_UNDECIDED;
  if (hipMemset(a.triUndecided, 0, sizeof(unsigned long long)) != hipSuccess) return fail(ctx, "trace: clearing the undecided count");
  const size_t lds = srtTraverseStackBytes(ctx->upload.scene.stackDepth);
  int e = srt_launch_trace(&a, traversal, planEntryGrid(ctx->prop.multiProcessorCount, n), lds, nullptr);
  if (e) return fail(ctx, "trace launch failed: %s", hipGetErrorString((hipError_t)e));
  if (hipDeviceSynchronize() != hipSuccess) return fail(ctx, "trace kernel failed");
  if (hipMemcpy(hits, dHits.get(), n * sizeof(SrtHit), hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, "trace: copy out");
  return 0;
}

// srtTraceRaysDevice / srtOccludedDevice (include/srt_hip.h "Ray queries"): every check on the host, then one launch of
// srt_query.hip on the caller's stream.  Nothing of the context changes: no work area, no event, no plan.
// anyHit: srtOccludedDevice (dOccluded); otherwise `traversal` selects the walk (dHits, dRecords).
static int queryDevice(SrtContext* ctx, const char* what, const void* dRays, int64_t n, bool anyHit, int32_t traversal, void* dHits,
                       void* dRecords, void* dOccluded, void* streamPtr) {
  if (!ctx) return 1;
  if (checkSceneReady(ctx, what)) return 1;
  if (n < 0) return fail(ctx, "%s: n = %lld is negative", what, (long long)n);
  if (!anyHit && traversal != SRT_TRAVERSE_FAITHFUL && traversal != SRT_TRAVERSE_CLOSEST)
    return fail(ctx, "%s: traversal %d is neither SRT_TRAVERSE_FAITHFUL nor SRT_TRAVERSE_CLOSEST", what, traversal);
  const int mode = anyHit ? 2 : traversal;  // srt_launch_query's modes
  if (n == 0) return 0;
  if (!dRays) return fail(ctx, "%s: null rays", what);
  if (anyHit ? !dOccluded : (!dHits && !dRecords)) return fail(ctx, "%s: no output buffer", what);
  if ((uintptr_t)dRays % 4) return fail(ctx, "%s: the rays are not aligned to 4 bytes", what);
  if ((uintptr_t)dHits % 16) return fail(ctx, "%s: the hits are not aligned to 16 bytes", what);
  if ((uintptr_t)dRecords % 4) return fail(ctx, "%s: the records are not aligned to 4 bytes", what);
  const DevScene& sc = ctx->upload.scene;
  const size_t lds = srtQueryStackBytes(sc.stackDepth);
  if (lds > SRT_LDS_BYTES) return fail(ctx, "%s: BVH depth %d needs %zu B of LDS per workgroup", what, sc.stackDepth, lds);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  QueryArgs a;
  a.scene = sc;
  a.rays = static_cast<const float*>(dRays);
  a.hits = static_cast<int4*>(dHits);
  a.records = static_cast<SrtHit*>(dRecords);
  a.occluded = static_cast<uint8_t*>(dOccluded);
  a.n = n;
  const int e = srt_launch_query(&a, mode, planEntryGrid(ctx->prop.multiProcessorCount, n), lds, static_cast<hipStream_t>(streamPtr));
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

int srtTraceRaysDevice(SrtContext* ctx, const void* dRays, int64_t n, int32_t traversal, void* dHits, void* dRecords, void* stream) {
  SRT_GUARDED(ctx, queryDevice(ctx, "srtTraceRaysDevice", dRays, n, false, traversal, dHits, dRecords, nullptr, stream));
}

int srtOccludedDevice(SrtContext* ctx, const void* dRays, int64_t n, void* dOccluded, void* stream) {
  SRT_GUARDED(ctx, queryDevice(ctx, "srtOccludedDevice", dRays, n, true, 0, nullptr, nullptr, dOccluded, stream));
}

// srtCameraRaysDevice / srtScatterRaysDevice / srtPathStepDevice (include/srt_hip.h "Path steps on device buffers"):
// as queryDevice -- every check on the host, then one launch of srt_pathstep.hip on the caller's stream, and nothing of
// the context changes.

// srt_path.h mix64 on the host (the kernels' copy is device code); tests/test_pathstep_abi.py pins srtRngKey to the oracle
static uint64_t hostMix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

uint64_t srtRngKey(uint64_t seed, uint64_t pixel, uint64_t sample) {  // the low 32 bits of pixel and of sample
  return hostMix64(hostMix64(seed) ^ ((pixel << 32) | (sample & 0xffffffffull)));
}

static int pathGrid(const SrtContext* ctx, int64_t n) { return planEntryGrid(ctx->prop.multiProcessorCount, n); }

// a required device pointer of `what`: non-null and aligned
static int checkPointer(SrtContext* ctx, const char* what, const char* name, const void* p, int align) {
  if (!p) return fail(ctx, "%s: null %s", what, name);
  if ((uintptr_t)p % align) return fail(ctx, "%s: the %s are not aligned to %d bytes", what, name, align);
  return 0;
}

static int cameraRaysDevice(SrtContext* ctx, const SrtRenderParams* p, const void* dPixelSample, int64_t n, void* dRays, void* dRng,
                            void* streamPtr) {
  const char* what = "srtCameraRaysDevice";
  if (!ctx) return 1;
  if (!p) return fail(ctx, "%s: null parameters", what);
  if (!ctx->haveCamera) return fail(ctx, "%s: no camera set", what);
  if (p->imageWidth < 2 || p->imageHeight < 2) return fail(ctx, "%s: image must be at least 2x2 (u,v divide by W-1,H-1)", what);
  if (n < 0) return fail(ctx, "%s: n = %lld is negative", what, (long long)n);
  if (!dPixelSample) {
    if (p->spp < 1) return fail(ctx, "%s: spp must be >= 1 without a list", what);
    const int64_t all = (int64_t)p->imageWidth * p->imageHeight * p->spp;
    if (n != all) return fail(ctx, "%s: n = %lld without a list, the frame has %lld samples", what, (long long)n, (long long)all);
  }
  if (n == 0) return 0;
  if ((uintptr_t)dPixelSample % 4) return fail(ctx, "%s: the list is not aligned to 4 bytes", what);
  if (checkPointer(ctx, what, "rays", dRays, 4) || checkPointer(ctx, what, "rng states", dRng, 8)) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  CameraRaysArgs a;
  a.cam = ctx->cam;
  a.imageWidth = p->imageWidth;
  a.imageHeight = p->imageHeight;
  a.spp = std::max(p->spp, 1);
  a.sampleFirst = p->sampleFirst;
  a.seed = p->seed;
  a.tMin = p->tMin;
  a.pixelSample = static_cast<const int32_t*>(dPixelSample);
  a.rays = static_cast<float*>(dRays);
  a.rng = static_cast<uint64_t*>(dRng);
  a.n = n;
  const int e = srt_launch_camera_rays(&a, pathGrid(ctx, n), static_cast<hipStream_t>(streamPtr));
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

static int scatterDevice(SrtContext* ctx, const void* dRays, const void* dRecords, int64_t n, void* dRng, void* dOut, void* dRaysOut,
                         void* streamPtr) {
  const char* what = "srtScatterRaysDevice";
  if (!ctx) return 1;
  if (checkSceneReady(ctx, what)) return 1;
  if (n < 0) return fail(ctx, "%s: n = %lld is negative", what, (long long)n);
  if (n == 0) return 0;
  if (checkPointer(ctx, what, "rays", dRays, 4) || checkPointer(ctx, what, "records", dRecords, 4) ||
      checkPointer(ctx, what, "rng states", dRng, 8) || checkPointer(ctx, what, "outputs", dOut, 16) ||
      checkPointer(ctx, what, "scattered rays", dRaysOut, 4))
    return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  ScatterDeviceArgs a;
  a.scene = ctx->upload.scene;
  a.rays = static_cast<const float*>(dRays);
  a.records = static_cast<const SrtHit*>(dRecords);
  a.rng = static_cast<uint64_t*>(dRng);
  a.out = static_cast<int4*>(dOut);
  a.raysOut = static_cast<float*>(dRaysOut);
  a.n = n;
  const int e = srt_launch_scatter_device(&a, pathGrid(ctx, n), static_cast<hipStream_t>(streamPtr));
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

static int pathStepDevice(SrtContext* ctx, int32_t traversal, const void* dRays, int64_t n, const void* dActive, void* dRng, void* dOut,
                          void* dRaysOut, void* dHits, void* streamPtr) {
  const char* what = "srtPathStepDevice";
  if (!ctx) return 1;
  if (checkSceneReady(ctx, what)) return 1;
  if (n < 0) return fail(ctx, "%s: n = %lld is negative", what, (long long)n);
  if (traversal != SRT_TRAVERSE_FAITHFUL && traversal != SRT_TRAVERSE_CLOSEST)
    return fail(ctx, "%s: traversal %d is neither SRT_TRAVERSE_FAITHFUL nor SRT_TRAVERSE_CLOSEST", what, traversal);
  if (n == 0) return 0;
  if (checkPointer(ctx, what, "rays", dRays, 4) || checkPointer(ctx, what, "rng states", dRng, 8) ||
      checkPointer(ctx, what, "outputs", dOut, 16) || checkPointer(ctx, what, "scattered rays", dRaysOut, 4))
    return 1;
  if ((uintptr_t)dHits % 16) return fail(ctx, "%s: the hits are not aligned to 16 bytes", what);
  const DevScene& sc = ctx->upload.scene;
  const size_t lds = srtQueryStackBytes(sc.stackDepth);  // the walk's stacks, as queryDevice sizes and bounds them
  if (lds > SRT_LDS_BYTES) return fail(ctx, "%s: BVH depth %d needs %zu B of LDS per workgroup", what, sc.stackDepth, lds);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  PathStepArgs a;
  a.scene = sc;
  a.rays = static_cast<const float*>(dRays);
  a.active = static_cast<const uint8_t*>(dActive);
  a.rng = static_cast<uint64_t*>(dRng);
  a.out = static_cast<int4*>(dOut);
  a.raysOut = static_cast<float*>(dRaysOut);
  a.hits = static_cast<int4*>(dHits);
  a.n = n;
  const int e = srt_launch_path_step(&a, traversal, pathGrid(ctx, n), lds, static_cast<hipStream_t>(streamPtr));
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

// The range comparison of srtCompactPathsDevice and srtSortPathsDevice: no written range may overlap a range that is read
// or another written one, each taken at its full length; null ranges take no part.  maskOut == mask exactly is the one
// exception (an entry's byte is read before it is written).
struct PathRange {
  const char* name;
  uintptr_t at;
  uint64_t bytes;
  bool written;
};
static int checkPathRanges(SrtContext* ctx, const char* what, const PathRange* ranges, size_t count, const PathRange* mask,
                           const PathRange* maskOut) {
  for (const PathRange* w = ranges; w != ranges + count; ++w) {
    if (!w->written || !w->at) continue;
    for (const PathRange* r = ranges; r != ranges + count; ++r) {
      if (r == w || !r->at || (r->written && r < w)) continue;  // a pair of written ranges once
      if (w == maskOut && r == mask && w->at == r->at) continue;
      if (w->at < r->at + r->bytes && r->at < w->at + w->bytes) return fail(ctx, "%s: the %s overlap the %s", what, w->name, r->name);
    }
  }
  return 0;
}

// srtCompactPathsDevice: every check on the host, then srt_compact.hip's three launches on the caller's stream.  Needs no
// scene; nothing of the context changes.
static int64_t compactTiles(int64_t n) { return n <= 0 ? 0 : (n - 1) / SRT_COMPACT_TILE + 1; }

int64_t srtCompactPathsScratchBytes(int64_t n) { return 8 * compactTiles(n); }

static int compactPathsDevice(SrtContext* ctx, int64_t n, const void* dOut, const void* dActive, const void* dRays, const void* dRng,
                              const void* dSlot, void* dRaysOut, void* dRngOut, void* dSlotOut, void* dActiveOut, void* dCount,
                              void* dScratch, void* streamPtr) {
  const char* what = "srtCompactPathsDevice";
  if (!ctx) return 1;
  if (n < 0) return fail(ctx, "%s: n = %lld is negative", what, (long long)n);
  if (!dOut && !dActive) return fail(ctx, "%s: no predicate: the outputs and the mask are both null", what);
  if (checkPointer(ctx, what, "count", dCount, 8)) return 1;
  if (n == 0) return 0;
  if (checkPointer(ctx, what, "scratch", dScratch, 8)) return 1;
  if (dRaysOut && !dRays) return fail(ctx, "%s: compacted rays without rays", what);
  if (dRngOut && !dRng) return fail(ctx, "%s: compacted rng states without rng states", what);
  if ((uintptr_t)dOut % 16) return fail(ctx, "%s: the outputs are not aligned to 16 bytes", what);
  if ((dRaysOut && (uintptr_t)dRays % 4) || (uintptr_t)dRaysOut % 4) return fail(ctx, "%s: the rays are not aligned to 4 bytes", what);
  if ((dRngOut && (uintptr_t)dRng % 8) || (uintptr_t)dRngOut % 8) return fail(ctx, "%s: the rng states are not aligned to 8 bytes", what);
  if ((dSlotOut && (uintptr_t)dSlot % 4) || (uintptr_t)dSlotOut % 4) return fail(ctx, "%s: the slots are not aligned to 4 bytes", what);
  if (dSlotOut && n > 0x7fffffffll) return fail(ctx, "%s: n = %lld does not fit a 32-bit slot", what, (long long)n);
  // what the kernels write may overlap nothing else they read or write (dActiveOut may BE dActive: an entry owns its byte)
  const uint64_t un = (uint64_t)n;
  const PathRange ranges[] = {{"outputs", (uintptr_t)dOut, 32 * un, false},
                              {"mask", (uintptr_t)dActive, un, false},
                              {"rays", (uintptr_t)(dRaysOut ? dRays : nullptr), 36 * un, false},
                              {"rng states", (uintptr_t)(dRngOut ? dRng : nullptr), 8 * un, false},
                              {"slots", (uintptr_t)(dSlotOut ? dSlot : nullptr), 4 * un, false},
                              {"compacted rays", (uintptr_t)dRaysOut, 36 * un, true},
                              {"compacted rng states", (uintptr_t)dRngOut, 8 * un, true},
                              {"compacted slots", (uintptr_t)dSlotOut, 4 * un, true},
                              {"compacted mask", (uintptr_t)dActiveOut, un, true},
                              {"count", (uintptr_t)dCount, 8, true},
                              {"scratch", (uintptr_t)dScratch, (uint64_t)srtCompactPathsScratchBytes(n), true}};
  if (checkPathRanges(ctx, what, ranges, sizeof ranges / sizeof ranges[0], &ranges[1], &ranges[8])) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  CompactArgs a;
  a.out = static_cast<const int32_t*>(dOut);
  a.active = static_cast<const uint8_t*>(dActive);
  a.rays = static_cast<const uint32_t*>(dRays);
  a.rng = static_cast<const uint64_t*>(dRng);
  a.slot = static_cast<const int32_t*>(dSlot);
  a.raysOut = static_cast<uint32_t*>(dRaysOut);
  a.rngOut = static_cast<uint64_t*>(dRngOut);
  a.slotOut = static_cast<int32_t*>(dSlotOut);
  a.activeOut = static_cast<uint8_t*>(dActiveOut);
  a.count = static_cast<int64_t*>(dCount);
  a.tileOffset = static_cast<uint64_t*>(dScratch);
  a.n = n;
  a.numTiles = compactTiles(n);
  const int grid = (int)std::min<int64_t>(a.numTiles, (int64_t)ctx->prop.multiProcessorCount * 8);
  const int e = srt_launch_compact(&a, grid, static_cast<hipStream_t>(streamPtr));
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

int srtCompactPathsDevice(SrtContext* ctx, int64_t n, const void* dOut, const void* dActive, const void* dRays, const void* dRng,
                          const void* dSlot, void* dRaysOut, void* dRngOut, void* dSlotOut, void* dActiveOut, void* dCount,
                          void* dScratch, void* stream) {
  SRT_GUARDED(ctx, compactPathsDevice(ctx, n, dOut, dActive, dRays, dRng, dSlot, dRaysOut, dRngOut, dSlotOut, dActiveOut, dCount,
                                      dScratch, stream));
}

// srtSortPathsDevice: every check on the host, then srt_sort.hip's memset, key kernel, rocPRIM sort and gather kernel on the
// caller's stream.  Needs no scene; nothing of the context changes.  The scratch: four arrays of n 32-bit words (key and
// index, twice: the sort's double buffers), each rounded up to 256 bytes, and behind them the sort's temporary storage.
// srtSortPathsScratchBytes runs without a device, so that part is a bound that grows with n -- 4 bytes per entry and 64 KB:
// with double buffers rocPRIM asks for digit histograms and, per block of at least 256 entries, one 32-bit look-back
// word per digit or one merge partition -- and the call compares what the installed rocPRIM asks for with it.
static int64_t sortArrayBytes(int64_t n) { return (4 * n + 255) & ~(int64_t)255; }
static int64_t sortTempBytes(int64_t n) { return sortArrayBytes(n) + 65536; }

int64_t srtSortPathsScratchBytes(int64_t n) { return n <= 0 ? 0 : 4 * sortArrayBytes(n) + sortTempBytes(n); }

static int sortPathsDevice(SrtContext* ctx, int64_t n, int32_t cellBits, const void* dBox, const void* dOut, const void* dActive,
                           const void* dRays, const void* dRng, const void* dSlot, void* dRaysOut, void* dRngOut, void* dSlotOut,
                           void* dActiveOut, void* dCount, void* dScratch, int64_t scratchBytes, void* streamPtr) {
  const char* what = "srtSortPathsDevice";
  if (!ctx) return 1;
  if (n < 0) return fail(ctx, "%s: n = %lld is negative", what, (long long)n);
  if (n > 0x7fffffffll) return fail(ctx, "%s: n = %lld does not fit a 32-bit index", what, (long long)n);
  if (cellBits < 1 || cellBits > SRT_SORT_MAX_CELL_BITS)
    return fail(ctx, "%s: cellBits = %d is outside [1, %d]", what, cellBits, (int)SRT_SORT_MAX_CELL_BITS);
  if (checkPointer(ctx, what, "count", dCount, 8)) return 1;
  if (n == 0) return 0;
  if (checkPointer(ctx, what, "scratch", dScratch, 8) || checkPointer(ctx, what, "box", dBox, 4) ||
      checkPointer(ctx, what, "rays", dRays, 4))
    return 1;
  if (scratchBytes < srtSortPathsScratchBytes(n))
    return fail(ctx, "%s: the scratch holds %lld bytes, n = %lld needs %lld", what, (long long)scratchBytes, (long long)n,
                (long long)srtSortPathsScratchBytes(n));
  if (dRngOut && !dRng) return fail(ctx, "%s: sorted rng states without rng states", what);
  if ((uintptr_t)dOut % 16) return fail(ctx, "%s: the outputs are not aligned to 16 bytes", what);
  if ((uintptr_t)dRaysOut % 4) return fail(ctx, "%s: the rays are not aligned to 4 bytes", what);
  if ((dRngOut && (uintptr_t)dRng % 8) || (uintptr_t)dRngOut % 8) return fail(ctx, "%s: the rng states are not aligned to 8 bytes", what);
  if ((dSlotOut && (uintptr_t)dSlot % 4) || (uintptr_t)dSlotOut % 4) return fail(ctx, "%s: the slots are not aligned to 4 bytes", what);
  const uint64_t un = (uint64_t)n;
  const PathRange ranges[] = {{"outputs", (uintptr_t)dOut, 32 * un, false},
                              {"mask", (uintptr_t)dActive, un, false},
                              {"rays", (uintptr_t)dRays, 36 * un, false},
                              {"rng states", (uintptr_t)(dRngOut ? dRng : nullptr), 8 * un, false},
                              {"slots", (uintptr_t)(dSlotOut ? dSlot : nullptr), 4 * un, false},
                              {"box", (uintptr_t)dBox, 24, false},
                              {"sorted rays", (uintptr_t)dRaysOut, 36 * un, true},
                              {"sorted rng states", (uintptr_t)dRngOut, 8 * un, true},
                              {"sorted slots", (uintptr_t)dSlotOut, 4 * un, true},
                              {"sorted mask", (uintptr_t)dActiveOut, un, true},
                              {"count", (uintptr_t)dCount, 8, true},
                              {"scratch", (uintptr_t)dScratch, (uint64_t)srtSortPathsScratchBytes(n), true}};
  if (checkPathRanges(ctx, what, ranges, sizeof ranges / sizeof ranges[0], &ranges[1], &ranges[9])) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  size_t tempNeeded = 0;
  int e = srt_sort_temp_bytes(n, cellBits, stream, &tempNeeded);
  if (e) return fail(ctx, "%s: the sort's size query failed: %s", what, hipGetErrorString((hipError_t)e));
  if ((int64_t)tempNeeded > sortTempBytes(n))
    return fail(ctx, "%s: rocPRIM asks for %zu bytes of temporary storage, the scratch reserves %lld", what, tempNeeded,
                (long long)sortTempBytes(n));
  SortArgs a;
  a.out = static_cast<const int32_t*>(dOut);
  a.active = static_cast<const uint8_t*>(dActive);
  a.rays = static_cast<const uint32_t*>(dRays);
  a.rng = static_cast<const uint64_t*>(dRng);
  a.slot = static_cast<const int32_t*>(dSlot);
  a.box = static_cast<const float*>(dBox);
  a.raysOut = static_cast<uint32_t*>(dRaysOut);
  a.rngOut = static_cast<uint64_t*>(dRngOut);
  a.slotOut = static_cast<int32_t*>(dSlotOut);
  a.activeOut = static_cast<uint8_t*>(dActiveOut);
  a.count = static_cast<int64_t*>(dCount);
  char* base = static_cast<char*>(dScratch);
  const int64_t array = sortArrayBytes(n);
  a.keys = reinterpret_cast<uint32_t*>(base);
  a.keysSpare = reinterpret_cast<uint32_t*>(base + array);
  a.index = reinterpret_cast<uint32_t*>(base + 2 * array);
  a.indexSpare = reinterpret_cast<uint32_t*>(base + 3 * array);
  a.temp = base + 4 * array;
  a.tempBytes = (size_t)sortTempBytes(n);
  a.n = n;
  a.cellBits = cellBits;
  const int grid = (int)std::min<int64_t>((n - 1) / SRT_BLOCK + 1, (int64_t)ctx->prop.multiProcessorCount * 8);
  e = srt_launch_sort(&a, grid, stream);
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

int srtSortPathsDevice(SrtContext* ctx, int64_t n, int32_t cellBits, const void* dBox, const void* dOut, const void* dActive,
                       const void* dRays, const void* dRng, const void* dSlot, void* dRaysOut, void* dRngOut, void* dSlotOut,
                       void* dActiveOut, void* dCount, void* dScratch, int64_t scratchBytes, void* stream) {
  SRT_GUARDED(ctx, sortPathsDevice(ctx, n, cellBits, dBox, dOut, dActive, dRays, dRng, dSlot, dRaysOut, dRngOut, dSlotOut, dActiveOut,
                                   dCount, dScratch, scratchBytes, stream));
}

// srtTracePathsDevice: every check on the host, then srt_paths.hip's memset and its one kernel on the caller's stream.
// Nothing of the context changes.
static int tracePathsDevice(SrtContext* ctx, int32_t traversal, int32_t maxBounce, const float* background, const void* dRays, int64_t n,
                            void* dRng, void* dResult, void* dScratch, void* streamPtr) {
  const char* what = "srtTracePathsDevice";
  if (!ctx) return 1;
  if (checkSceneReady(ctx, what)) return 1;
  if (n < 0) return fail(ctx, "%s: n = %lld is negative", what, (long long)n);
  if (traversal != SRT_TRAVERSE_FAITHFUL && traversal != SRT_TRAVERSE_CLOSEST)
    return fail(ctx, "%s: traversal %d is neither SRT_TRAVERSE_FAITHFUL nor SRT_TRAVERSE_CLOSEST", what, traversal);
  if (maxBounce < 0 || maxBounce > SRT_MAX_BOUNCE) return fail(ctx, "%s: maxBounce = %d is outside [0, %d]", what, maxBounce, SRT_MAX_BOUNCE);
  if (!background) return fail(ctx, "%s: null background", what);
  if (n == 0) return 0;
  if (checkPointer(ctx, what, "rays", dRays, 4) || checkPointer(ctx, what, "rng states", dRng, 8) ||
      checkPointer(ctx, what, "results", dResult, 16) || checkPointer(ctx, what, "scratch", dScratch, 8))
    return 1;
  // what the kernel writes may overlap nothing else it reads or writes (srtCompactPathsDevice's range comparison)
  struct Range {
    const char* name;
    uintptr_t at;
    uint64_t bytes;
  };
  const uint64_t un = (uint64_t)n;
  const Range ranges[] = {{"rays", (uintptr_t)dRays, 36 * un},  // read only: compared with the three written ones
                          {"rng states", (uintptr_t)dRng, 8 * un},
                          {"results", (uintptr_t)dResult, 16 * un},
                          {"scratch", (uintptr_t)dScratch, SRT_PATHS_SCRATCH_BYTES}};
  for (int w = 1; w < 4; ++w)
    for (int r = 0; r < w; ++r)
      if (ranges[w].at < ranges[r].at + ranges[r].bytes && ranges[r].at < ranges[w].at + ranges[w].bytes)
        return fail(ctx, "%s: the %s overlap the %s", what, ranges[w].name, ranges[r].name);
  const DevScene& sc = ctx->upload.scene;
  const size_t lds = srtPathsLdsBytes(sc.stackDepth, maxBounce);
  if (lds > SRT_LDS_BYTES)
    return fail(ctx, "%s: BVH depth %d and %d bounces need %zu B of LDS per workgroup", what, sc.stackDepth, maxBounce, lds);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  TracePathsArgs a;
  a.scene = sc;
  a.rays = static_cast<const float*>(dRays);
  a.rng = static_cast<uint64_t*>(dRng);
  a.result = static_cast<int4*>(dResult);
  a.counter = static_cast<unsigned long long*>(dScratch);
  for (int c = 0; c < 3; ++c) a.background[c] = background[c];
  a.maxBounce = maxBounce;
  a.refillMin = std::min(std::max(ctx->tun.pathsRefillMin, 1), 64);
  a.n = n;
  const int e = srt_launch_paths(&a, traversal, ctx->prop.multiProcessorCount, lds, SRT_PATHS_SCRATCH_BYTES, static_cast<hipStream_t>(streamPtr));
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

int srtTracePathsDevice(SrtContext* ctx, int32_t traversal, int32_t maxBounce, const float background[3], const void* dRays, int64_t n,
                        void* dRng, void* dResult, void* dScratch, void* stream) {
  SRT_GUARDED(ctx, tracePathsDevice(ctx, traversal, maxBounce, background, dRays, n, dRng, dResult, dScratch, stream));
}

int srtCameraRaysDevice(SrtContext* ctx, const SrtRenderParams* p, const void* dPixelSample, int64_t n, void* dRays, void* dRng,
                        void* stream) {
  SRT_GUARDED(ctx, cameraRaysDevice(ctx, p, dPixelSample, n, dRays, dRng, stream));
}

int srtScatterRaysDevice(SrtContext* ctx, const void* dRays, const void* dRecords, int64_t n, void* dRng, void* dOut, void* dRaysOut,
                         void* stream) {
  SRT_GUARDED(ctx, scatterDevice(ctx, dRays, dRecords, n, dRng, dOut, dRaysOut, stream));
}

int srtPathStepDevice(SrtContext* ctx, int32_t traversal, const void* dRays, int64_t n, const void* dActive, void* dRng, void* dOut,
                      void* dRaysOut, void* dHits, void* stream) {
  SRT_GUARDED(ctx, pathStepDevice(ctx, traversal, dRays, n, dActive, dRng, dOut, dRaysOut, dHits, stream));
}

// test entries: material::scatter known answers through the kernels' own shade(), in the instance `form` selects
// (bit 0 WIDE, bit 1 COUNT: include/srt_hip_test.h)

int srtScatterRaysForm(SrtContext* ctx, const SrtRay* rays, const SrtHit* hits, int32_t n, uint64_t seed, int32_t form, float* out13,
                       uint32_t* outFetches) {
  if (!ctx || !rays || !hits || !out13 || n < 1) return 1;
  if (form < 0 || form > 3) return fail(ctx, "scatter: form %d is not one of 0-3", form);
  if (checkSceneReady(ctx, "scatter")) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  // the kernel indexes the shading records with the hit's material through a plain pointer
  const int32_t numMaterials = ctx->upload.scene.numMaterials;
  for (int i = 0; i < n; ++i) {
    if (hits[i].material < 0) return fail(ctx, "scatter: hit %d has no material", i);
    if (hits[i].material >= numMaterials) return fail(ctx, "scatter: hit %d names material %d of %d", i, hits[i].material, numMaterials);
  }
  DeviceBuffer dRays, dHits, dOut, dFetches;
  if (dRays.reserve(n * sizeof(SrtRay)) != hipSuccess || dHits.reserve(n * sizeof(SrtHit)) != hipSuccess ||
      dOut.reserve((size_t)n * 13 * 4) != hipSuccess || (outFetches && dFetches.reserve((size_t)n * 4) != hipSuccess))
    return fail(ctx, "scatter: hipMalloc");
  if (hipMemcpy(dRays.get(), rays, n * sizeof(SrtRay), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dHits.get(), hits, n * sizeof(SrtHit), hipMemcpyHostToDevice) != hipSuccess)
    return fail(ctx, "scatter: copy in");
  int e = srt_launch_scatter(&ctx->upload.scene, dRays.get<const SrtRay>(), dHits.get<const SrtHit>(), dOut.get<float>(),
                             outFetches ? dFetches.get<uint32_t>() : nullptr, seed, n, form, nullptr);
  if (e) return fail(ctx, "scatter launch failed");
  if (hipDeviceSynchronize() != hipSuccess) return fail(ctx, "scatter kernel failed");
  if (hipMemcpy(out13, dOut.get(), (size_t)n * 13 * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, "scatter: copy out");
  if (outFetches && hipMemcpy(outFetches, dFetches.get(), (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(ctx, "scatter: copy out");
  return 0;
}

int srtScatterRays(SrtContext* ctx, const SrtRay* rays, const SrtHit* hits, int32_t n, uint64_t seed, float* out13) {
  return srtScatterRaysForm(ctx, rays, hits, n, seed, 0, out13, nullptr);
}

// test entry: the exact chunk sum on caller-made partial sums, through the kernels and the limit a render uses
// (include/srt_hip_test.h).  Needs no scene.
int srtTestChunkSum(SrtContext* ctx, const float* hChunks, int32_t n, int32_t chunks, int32_t path, int32_t samples, float* hOut4) {
  if (!ctx) return 1;
  if (!hChunks) return fail(ctx, "chunk sum: null slots");
  if (!hOut4) return fail(ctx, "chunk sum: null output");
  if (n <= 0 || n > (1 << 20)) return fail(ctx, "chunk sum: n = %d is not in [1, 2^20]", n);
  if (chunks < 1) return fail(ctx, "chunk sum: chunks = %d, must be at least 1", chunks);
  // the largest count the planner lets any render use (the smallest image's; srtPlanSppChunks)
  if (srtPlanSppChunks(1, 1, chunks, chunks) < 1) return fail(ctx, "chunk sum: %d chunks are more than any render's plan allows", chunks);
  if (path != 0 && path != 1) return fail(ctx, "chunk sum: path %d is neither 0 (chunk slots) nor 1 (atomics)", path);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  const size_t slotBytes = (size_t)n * chunks * sizeof(float4), outBytes = (size_t)n * sizeof(float4);
  DeviceBuffer dSlots, dOut, dFix;
  if (dSlots.reserve(slotBytes) != hipSuccess || dOut.reserve(outBytes) != hipSuccess ||
      (path == 1 && dFix.reserve((size_t)n * sizeof(SrtFixedAccum)) != hipSuccess))
    return fail(ctx, "chunk sum: hipMalloc");
  if (hipMemcpy(dSlots.get(), hChunks, slotBytes, hipMemcpyHostToDevice) != hipSuccess) return fail(ctx, "chunk sum: copy in");
  const float limit = chunkFixLimit(chunks);
  int e;
  if (path == 0) {
    e = srt_launch_sum_chunks(dSlots.get<const float4>(), dOut.get<float4>(), n, chunks, limit, nullptr);
  } else {
    if (hipMemset(dFix.get(), 0, (size_t)n * sizeof(SrtFixedAccum)) != hipSuccess) return fail(ctx, "chunk sum: memset");
    e = srt_launch_test_commit(dSlots.get<const float4>(), dFix.get<SrtFixedAccum>(), n, chunks, limit, nullptr);
    if (!e) e = srt_launch_finalize(dFix.get<const SrtFixedAccum>(), dOut.get<float4>(), n, samples, nullptr);
  }
  if (e) return fail(ctx, "chunk sum launch failed: %s", hipGetErrorString((hipError_t)e));
  if (hipDeviceSynchronize() != hipSuccess) return fail(ctx, "chunk sum kernel failed");
  if (hipMemcpy(hOut4, dOut.get(), outBytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, "chunk sum: copy out");
  return 0;
}

int srtRenderTiles(SrtContext* ctx, const SrtRenderParams* p, void* dAccumTiles, void* streamPtr) { SRT_GUARDED(ctx, srtRenderTilesImpl(ctx, p, dAccumTiles, streamPtr)); }
int srtRenderTilesMoments(SrtContext* ctx, const SrtRenderParams* p, void* dAccumTiles, void* dMomentTiles, void* streamPtr) {
  SRT_GUARDED(ctx, srtRenderTilesMomentsImpl(ctx, p, dAccumTiles, dMomentTiles, streamPtr));
}
int srtRenderAdaptive(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, void* dAccumImage, void* dMomentsImage,
                      void* dRgba, SrtAdaptiveStats* stats, void* stream) {
  SRT_GUARDED(ctx, srtRenderAdaptiveImpl(ctx, p, ap, dAccumImage, dMomentsImage, dRgba, stats, stream));
}
int srtRenderAdaptiveGuided(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, int32_t planes,
                            void* const dPlaneImages[4], void* dAccumImage, void* dMomentsImage, void* dRgba,
                            SrtAdaptiveStats* stats, void* stream) {
  SRT_GUARDED(ctx, srtRenderAdaptiveGuidedImpl(ctx, p, ap, planes, dPlaneImages, dAccumImage, dMomentsImage, dRgba, stats, stream));
}

}  // extern "C"
