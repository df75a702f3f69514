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
