// srt_plan.cpp -- the planner of the render launches (srt_plan.h): tile counts and chunk plans (exported, include/srt_hip.h),
// the choice of the render kernel and its LDS, the work split, the scheduler defaults.  Integer arithmetic on its arguments
// alone; the LDS layouts are srt_lds_layout.h's.

#include "srt_plan.h"

#include <algorithm>

#include "srt_lds_layout.h"

extern "C" {

int32_t srtNumTiles(int32_t w, int32_t h) {
  return ((w + SRT_TILE_W - 1) / SRT_TILE_W) * ((h + SRT_TILE_H - 1) / SRT_TILE_H);
}
int32_t srtNumLocalTiles(int32_t w, int32_t h, int32_t stride) {
  if (stride < 1) stride = 1;
  return (srtNumTiles(w, h) + stride - 1) / stride;
}

// Work items per pixel when the caller leaves the choice to the library (sppChunks == 0): about 8 samples per
// item, at least 128 items per pixel when there are that many samples (down to one sample per item), at most 640.
// It depends on the sample count alone, so that the chunk boundaries -- and with them the image, bit for bit --
// are the same for every tile split and GPU count.  Many items per pixel keep the tiles in flight few (a queue's
// waves pull consecutive items, i.e. the chunks of one tile, then of its neighbour), and SMALL items keep the end
// of a launch short: the last items to finish are single pixels of the mesh, ten times the average pixel's cost,
// and a rank's share of a frame feels that tail most.  720p headline at 5000 spp on the LDS-resident-tree kernel
// (profiles/r02/chunk_policy.txt): whole frame 1069.9 / 1067.9 / 1066.7 / 1068.1 ms with 157 / 314 / 628 / 1250
// chunks (as long as the chunk slots fit the scratch budget; the atomic path costs 1.2 %); one of 8 ranks' share
// 148.5 / 142.5 / 139.5 / 138.3 ms (133.7 would be an eighth of the frame).  Low sample counts: 64 spp on the 240p
// spheres frame run at 4.3 / 5.2 / 6.2 / 7.1 / 7.8 Gsamples/s with 4 / 8 / 16 / 32 / 64 chunks.
int32_t srtDefaultSppChunks(int32_t spp) {
  const int32_t bySize = (spp + 7) / 8, byCount = std::min(128, spp);
  return std::max(1, std::min(640, std::max(bySize, byCount)));
}

// The chunk count a render of this size will use: `sppChunks` when the caller gives one, else srtDefaultSppChunks(spp),
// and -1 when an explicit count does not fit.  Work items and chunk slots are indexed with 32-bit integers in the
// kernels: the slots of one chunk over the WHOLE image (not a rank's share: the plan, and with it the image bit for
// bit, must not depend on the tile split), plus the padding a work queue's last unit can add (a unit is at most 1024
// tiles; every queue counts its own items).  1280 x 720 allows 2166 chunks, 1920 x 1080 1003: the default plan
// (at most 640) always fits images below about 3 Mpixels; beyond that the default is clamped.
int32_t srtPlanSppChunks(int32_t imageWidth, int32_t imageHeight, int32_t spp, int32_t sppChunks) {
  if (imageWidth < 1 || imageHeight < 1 || spp < 1 || sppChunks < 0 || sppChunks > spp) return -1;
  const int64_t perChunk = ((int64_t)srtNumTiles(imageWidth, imageHeight) + 1024 + 64) * SRT_TILE_PIXELS;
  const int64_t maxChunks = (int64_t)0x7fffffff / perChunk;
  if (maxChunks < 1) return -1;
  if (sppChunks > 0) return sppChunks <= maxChunks ? sppChunks : -1;
  return (int32_t)std::min<int64_t>(srtDefaultSppChunks(spp), maxChunks);
}

}  // extern "C"

float chunkFixLimit(int32_t chunks) {
  int pow2 = 1;
  while (pow2 < chunks) pow2 *= 2;
  return 0x1p26f / (float)pow2;
}

// The render launch for these parameters: the kernel form and the instance of it, workgroup and LDS size, the path-pool
// kernel's rings.  Every choice of kernel is made here; srtRenderTilesImpl allocates and launches what it says.
RenderPlan planRender(const SceneFacts& sc, const Tunables& tun, int numCUs, const SrtRenderParams* p, bool moments, int32_t listTiles) {
  RenderPlan plan{};
  const bool faithful = p->traversal == SRT_TRAVERSE_FAITHFUL;
  plan.closest = p->traversal == SRT_TRAVERSE_CLOSEST;
  plan.count = p->countStats != 0;
  plan.moments = moments;
  // FAITHFUL on a scene whose whole node array fits into a CU's LDS: the LDS-resident-tree kernel (srt_render_kernel
  // LDSTREE), one workgroup of 1024 threads per CU, walking the threaded copy of the tree (no per-lane stack).
  const size_t ldsTreeBytes = srtLdsTreeLayout(sc.numNodes, p->maxBounce, false).end;  // threaded tree: no stacks
  // (Even trees of a few dozen nodes gain: their frames are shading-bound, and the 128-register kernel keeps a hit's
  // texel loads in flight together where the 96-register one spills, profiles/r02/lds_tree.txt.)
  const bool ldsTree = faithful && tun.ldsTree > 0 && sc.numNodes >= tun.ldsTree && ldsTreeBytes <= SRT_LDS_BYTES &&
                       sc.threadLinks;  // thread links exist: host-built trees, 15-bit references (srtUploadScene)
  // ... and when the attenuation stacks fit behind them as well they stay in LDS (SRT_FORM_LDS_TREE_ATT): +2 to +5 % on the
  // small BASELINE scenes; the headline scene's tree leaves no room (SRT_FORM_LDS_TREE: they live in global memory)
  const size_t ldsTreeAttBytes = srtLdsTreeLayout(sc.numNodes, p->maxBounce, true).end;
  // The path-pool kernel (srt_wavefront.hip) serves what the LDS-resident tree serves, when its rings fit behind the
  // tree: one 1024-thread workgroup per CU, wfPool contexts each.  A counting launch runs the counting instance of the
  // kernel the same launch without counting runs: the counters belong to the kernel under test.
  // LDS behind the tree (srtWfLdsLayout): the control words, the rings, and per context the (t, primitive) its walk ended
  // at.  Ring capacity = pool size = the largest of kSrtWfRings that fits and does not exceed the tunable (the headline
  // scene's 129 KB tree leaves room for 1536).
  // Hybrid form: the tree's top in LDS, the rest read from global memory (scene.nodesWf, built at upload when the tree does
  // not fit or the tunable wf_resident_max asks for it).
  const bool hybrid = faithful && sc.hybridRecords && tun.wavefront > 0 && sc.classTable;
  const int resident = hybrid ? sc.wfResident : sc.numNodes;
  // ring counters are 32-bit and a 3 * 2^j ring cannot take their wrap-around: such rings only while a workgroup's
  // enqueues stay far below 2^32 (about three per sample)
  const int numLocalTiles = listTiles >= 0 ? listTiles : srtNumLocalTiles(p->imageWidth, p->imageHeight, p->tileStride);
  const double enqueuesPerGroup = 4.0 * (double)numLocalTiles * SRT_TILE_PIXELS * (double)p->spp / std::max(1, numCUs);
  for (const SrtWfRingGeom& r : kSrtWfRings) {
    if (r.cap > std::max(1024, tun.wfPool) || srtWfLdsBytes(resident, r.cap, hybrid) > SRT_LDS_BYTES) continue;
    if (r.mul3 && enqueuesPerGroup > 2.0e9) continue;
    plan.wfRingCap = r.cap;
    plan.wfRingShift = r.shift;
    plan.wfRingMul3 = r.mul3;
    break;
  }
  const bool wavefront = plan.wfRingCap > 0 && (hybrid || (ldsTree && tun.wavefront > 0 && sc.numNodes >= tun.wavefront && sc.classTable));
  if (wavefront) {
    plan.form = hybrid ? SRT_FORM_PATH_POOL_HYBRID : SRT_FORM_PATH_POOL;
    plan.block = SRT_BLOCK_TREE;
    plan.lds = srtWfLdsBytes(resident, plan.wfRingCap, hybrid);
    plan.profile = !plan.count && !plan.moments && tun.wfProfile > 0;  // a counting or moments launch takes no profile
    // (hybrid form: the single-root instance is worth +12 to +15 % on cache-resident trees and costs 5 % on the HBM-bound
    // soups of 4 M triangles and more, where the shorter visit only crowds the memory system: profiles/r03/hybrid.txt)
    plan.single = !plan.profile && sc.numWorld == 1 && (!hybrid || sc.numNodes <= (1 << 20));
    return plan;
  }
  plan.wfRingCap = plan.wfRingShift = plan.wfRingMul3 = 0;
  plan.form = !ldsTree ? SRT_FORM_STACK : ldsTreeAttBytes <= SRT_LDS_BYTES ? SRT_FORM_LDS_TREE_ATT : SRT_FORM_LDS_TREE;
  plan.block = ldsTree ? SRT_BLOCK_TREE : SRT_BLOCK;
  plan.lds = plan.form == SRT_FORM_LDS_TREE_ATT ? ldsTreeAttBytes
             : ldsTree                          ? ldsTreeBytes
                                                : srtStackFormLayout(sc.stackDepth, p->maxBounce).end;
  plan.single = !plan.count && sc.numWorld == 1;  // (the counting instances serve single-root worlds as well)
  return plan;
}

int planGrid(int numCUs, int perCU, int32_t numWork, int32_t block) {
  const int wgItems = SRT_TILE_PIXELS * (block / 64);
  return std::max(1, std::min(numCUs * perCU, (numWork + wgItems - 1) / wgItems));
}

int planEntryGrid(int numCUs, int64_t n) { return (int)std::min<int64_t>((n + SRT_BLOCK - 1) / SRT_BLOCK, (int64_t)numCUs * 8); }

LaunchPlan planLaunch(const SceneFacts& sc, const Tunables& tun, int numCUs, const SrtRenderParams* p, bool moments, int32_t listTiles) {
  LaunchPlan lp{};
  lp.render = planRender(sc, tun, numCUs, p, moments, listTiles);
  lp.fitsLds = lp.render.lds <= SRT_LDS_BYTES;
  lp.numLocalTiles = listTiles >= 0 ? listTiles : srtNumLocalTiles(p->imageWidth, p->imageHeight, p->tileStride);
  {
    // work queues (srt_render_kernel): units of >= 8 consecutive local tiles, about a dozen units per queue,
    // at most 64 queues.  Measured on the 720p headline frame (ms per launch, 1 rank / one of 8 ranks):
    // 1 queue 1916 / 253, 16 queues x 8 tiles 1818 / 238, 64 x 8: 1767 / 255, 64 x 16: 1744 / -.
    const auto pow2Floor = [](int v) { int r = 1; while (2 * r <= v) r *= 2; return r; };
    // (the queues are counted with the chunk count the caller asked for, before the clamp below)
    const int32_t askedChunks = p->sppChunks > 0 ? p->sppChunks : srtDefaultSppChunks(p->spp);
    int unit = 8;
    const int unitsAt8 = (lp.numLocalTiles + 7) / 8;
    if (unitsAt8 >= 2 * 12 * SRT_MAX_QUEUES) unit = 8 * pow2Floor(unitsAt8 / (12 * SRT_MAX_QUEUES));
    lp.unitTiles = std::min(1024, std::max(1, tun.unitTiles > 0 ? tun.unitTiles : unit));
    const int units = (lp.numLocalTiles + lp.unitTiles - 1) / lp.unitTiles;
    // ... and only while every wave still gets a few dozen groups: with few groups per wave (16 spp on a
    // 10 M-triangle soup: 14 400 groups for 5 120 waves) one counter balances better than stealing does.
    const int64_t groups = (int64_t)lp.numLocalTiles * askedChunks, waves = (int64_t)numCUs * 20;
    const int byUnits = pow2Floor(std::max(1, units / 12));
    const int byGroups = pow2Floor((int)std::max<int64_t>(1, std::min<int64_t>(SRT_MAX_QUEUES, groups / (2 * waves))));
    lp.numQueues = std::min(SRT_MAX_QUEUES, std::max(1, tun.queues > 0 ? tun.queues : std::min(byUnits, byGroups)));
    lp.numUnits = units;
  }
  // Scheduler defaults by traversal mode (profiles/r02/scheduler_sweep.txt).  FAITHFUL on cache-resident scenes:
  // node bursts go on while half of their lanes are still at nodes, up to 64 visits, restarts at 24 waiting lanes
  // (+6 % on the headline frame against 6/8, 32, 16).  The closest-hit traversal over the 64-byte records is bound by
  // memory latency on large scenes and wants shorter bursts that give up sooner (10 M triangles: 87.6 against 77.8
  // Msamples/s), and does not care on small ones.
  const bool closestMode = p->traversal == SRT_TRAVERSE_CLOSEST;
  lp.shadeMin = tun.shadeMin >= 0 ? tun.shadeMin : (closestMode ? 16 : 24);
  lp.primMin = tun.primMin;
  lp.hitMin = tun.hitMin;
  lp.fuseMin = tun.fuseMin;
  lp.nodeBurst = std::max(1, tun.nodeBurst > 0 ? tun.nodeBurst : (closestMode ? 32 : 64));
  lp.primAgainMin = std::max(1, tun.primAgainMin);
  lp.keepEighths = std::min(8, tun.keepEighths >= 0 ? tun.keepEighths : (closestMode ? 6 : 4));
  lp.sppChunks = srtPlanSppChunks(p->imageWidth, p->imageHeight, p->spp, p->sppChunks);
  if (lp.sppChunks < 1) return lp;
  lp.numWork = lp.numLocalTiles * lp.sppChunks * SRT_TILE_PIXELS;
  if (srtFormIsPathPool(lp.render.form)) {
    lp.wfGrid = planGrid(numCUs, 1, lp.numWork, lp.render.block);  // one workgroup owns a CU and its LDS
    // a workgroup never needs more contexts than it has work items
    const int64_t itemsPerGroup = ((int64_t)lp.numWork + lp.wfGrid - 1) / lp.wfGrid;
    lp.wfPoolSize = (int)std::max<int64_t>(64, std::min<int64_t>(lp.render.wfRingCap, itemsPerGroup + 63));
    lp.wfSwapMin = tun.wfSwapMin > 0 ? std::min(64, tun.wfSwapMin) : (lp.render.form == SRT_FORM_PATH_POOL_HYBRID ? 16 : 32);
    lp.wfFarRounds = tun.wfFarRounds > 0 ? std::min(4, tun.wfFarRounds) : (sc.numNodes <= (1 << 20) ? 2 : 1);
    lp.wfSwapBig = std::max(lp.wfSwapMin, std::min(64, tun.wfSwapBig));
  }
  return lp;
}

void setPlanArgs(RenderArgs& a, const LaunchPlan& lp) {
  a.unitTiles = lp.unitTiles;
  a.numQueues = lp.numQueues;
  a.numUnits = lp.numUnits;
  a.sppChunks = lp.sppChunks;
  a.fixLimit = chunkFixLimit(a.sppChunks);
  a.numWork = lp.numWork;
  a.sppBase = a.spp / a.sppChunks;
  a.sppRem = a.spp % a.sppChunks;
  a.unitGroups = a.unitTiles * a.sppChunks;
  a.rcpUnitGroups = 1.0f / (float)a.unitGroups;
  a.rcpChunks = 1.0f / (float)a.sppChunks;
  a.shadeMin = lp.shadeMin;
  a.primMin = lp.primMin;
  a.hitMin = lp.hitMin;
  a.fuseMin = lp.fuseMin;
  a.nodeBurst = lp.nodeBurst;
  a.primAgainMin = lp.primAgainMin;
  a.keepEighths = lp.keepEighths;
  if (srtFormIsPathPool(lp.render.form)) {
    a.wfPoolSize = lp.wfPoolSize;
    a.wfRingCap = lp.render.wfRingCap;
    a.wfRingShift = lp.render.wfRingShift;
    a.wfRingMul3 = lp.render.wfRingMul3;
    a.wfSwapMin = lp.wfSwapMin;
    a.wfFarRounds = lp.wfFarRounds;
    a.wfSwapBig = lp.wfSwapBig;
  }
}
