// srt_rays.cpp -- the device-buffer entries of the C ABI (include/srt_hip.h "Ray queries", "Path steps on device buffers"):
// queries, camera rays, scatter, the fused path step, compaction, the sort, whole paths and direct light sampling, on the
// caller's buffers and stream.  Each makes every check on the host and then launches its kernel file; nothing of the context changes -- no
// work area, no event, no plan.  The refusals several of them make are written once, ahead of them.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "srt_context.h"
#include "srt_launch.h"
#include "srt_lds_layout.h"

// ---------------------------------------------------------------- shared checks
static int checkCount(SrtContext* ctx, const char* what, int64_t n) {
  return n < 0 ? fail(ctx, "%s: n = %lld is negative", what, (long long)n) : 0;
}

static int checkTraversal(SrtContext* ctx, const char* what, int32_t traversal) {
  if (traversal == SRT_TRAVERSE_FAITHFUL || traversal == SRT_TRAVERSE_CLOSEST) return 0;
  return fail(ctx, "%s: traversal %d is neither SRT_TRAVERSE_FAITHFUL nor SRT_TRAVERSE_CLOSEST", what, traversal);
}

// The walk's LDS (its stacks; with bounces >= 0 srtTracePathsDevice's attenuation stack too) against what a workgroup has
static int checkWalkLds(SrtContext* ctx, const char* what, size_t lds, int32_t bounces = -1) {
  if (lds <= SRT_LDS_BYTES) return 0;
  char subject[48] = " needs";
  if (bounces >= 0) snprintf(subject, sizeof subject, " and %d bounces need", bounces);
  return fail(ctx, "%s: BVH depth %d%s %zu B of LDS per workgroup", what, ctx->upload.scene.stackDepth, subject, lds);
}

// a required device pointer of `what`: non-null and aligned
static int checkPointer(SrtContext* ctx, const char* what, const char* name, const void* p, int align) {
  if (!p) return fail(ctx, "%s: null %s", what, name);
  if ((uintptr_t)p % align) return fail(ctx, "%s: the %s are not aligned to %d bytes", what, name, align);
  return 0;
}

// No written range may overlap a range that is read or another written one, each taken at its full length; null ranges
// take no part.  A pair of written ranges is compared once and named in table order, or with laterFirst by the one that
// comes later in the table ("the results overlap the rng states": srtTracePathsDevice's texts; of two faults the one
// reported is then the first in its argument order, as before).  maskOut == mask exactly is the one exception (an entry's
// byte is read before it is written).
struct PathRange {
  const char* name;
  uintptr_t at;
  uint64_t bytes;
  bool written;
};
static int checkPathRanges(SrtContext* ctx, const char* what, const PathRange* ranges, size_t count, const PathRange* mask,
                           const PathRange* maskOut, bool laterFirst = false) {
  for (const PathRange* w = ranges; w != ranges + count; ++w) {
    if (!w->written || !w->at) continue;
    for (const PathRange* r = ranges; r != ranges + count; ++r) {
      if (r == w || !r->at || (r->written && (laterFirst ? r > w : r < w))) continue;  // a pair of written ranges once
      if (maskOut && w == maskOut && r == mask && w->at == r->at) continue;
      if (w->at < r->at + r->bytes && r->at < w->at + w->bytes) return fail(ctx, "%s: the %s overlap the %s", what, w->name, r->name);
    }
  }
  return 0;
}

static int pathGrid(const SrtContext* ctx, int64_t n) { return planEntryGrid(ctx->prop.multiProcessorCount, n); }

// ---------------------------------------------------------------- srtTraceRaysDevice / srtOccludedDevice
// One launch of srt_query.hip.  anyHit: srtOccludedDevice (dOccluded); otherwise `traversal` selects the walk (dHits, dRecords).
static int queryDevice(SrtContext* ctx, const char* what, const void* dRays, int64_t n, bool anyHit, int32_t traversal, void* dHits,
                       void* dRecords, void* dOccluded, void* streamPtr) {
  if (!ctx) return 1;
  if (checkSceneReady(ctx, what) || checkCount(ctx, what, n)) return 1;
  if (!anyHit && checkTraversal(ctx, what, traversal)) return 1;
  const int mode = anyHit ? 2 : traversal;  // srt_launch_query's modes
  if (n == 0) return 0;
  if (!dRays) return fail(ctx, "%s: null rays", what);
  if (anyHit ? !dOccluded : (!dHits && !dRecords)) return fail(ctx, "%s: no output buffer", what);
  if ((uintptr_t)dRays % 4) return fail(ctx, "%s: the rays are not aligned to 4 bytes", what);
  if ((uintptr_t)dHits % 16) return fail(ctx, "%s: the hits are not aligned to 16 bytes", what);
  if ((uintptr_t)dRecords % 4) return fail(ctx, "%s: the records are not aligned to 4 bytes", what);
  const DevScene& sc = ctx->upload.scene;
  const size_t lds = srtQueryStackBytes(sc.stackDepth);
  if (checkWalkLds(ctx, what, lds)) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  QueryArgs a;
  a.scene = sc;
  a.rays = static_cast<const float*>(dRays);
  a.hits = static_cast<int4*>(dHits);
  a.records = static_cast<SrtHit*>(dRecords);
  a.occluded = static_cast<uint8_t*>(dOccluded);
  a.n = n;
  const int e = srt_launch_query(&a, mode, pathGrid(ctx, n), lds, static_cast<hipStream_t>(streamPtr));
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

// ---------------------------------------------------------------- srtCameraRaysDevice / srtScatterRaysDevice / srtPathStepDevice
// One launch of srt_pathstep.hip each.

// srt_path.h mix64 on the host (the kernels' copy is device code); tests/test_pathstep_abi.py pins srtRngKey to the oracle
static uint64_t hostMix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static int cameraRaysDevice(SrtContext* ctx, const SrtRenderParams* p, const void* dPixelSample, int64_t n, void* dRays, void* dRng,
                            void* streamPtr) {
  const char* what = "srtCameraRaysDevice";
  if (!ctx) return 1;
  if (!p) return fail(ctx, "%s: null parameters", what);
  if (!ctx->haveCamera) return fail(ctx, "%s: no camera set", what);
  if (p->imageWidth < 2 || p->imageHeight < 2) return fail(ctx, "%s: image must be at least 2x2 (u,v divide by W-1,H-1)", what);
  if (checkCount(ctx, what, n)) return 1;
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
  if (checkSceneReady(ctx, what) || checkCount(ctx, what, n)) return 1;
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
  if (checkSceneReady(ctx, what) || checkCount(ctx, what, n) || checkTraversal(ctx, what, traversal)) return 1;
  if (n == 0) return 0;
  if (checkPointer(ctx, what, "rays", dRays, 4) || checkPointer(ctx, what, "rng states", dRng, 8) ||
      checkPointer(ctx, what, "outputs", dOut, 16) || checkPointer(ctx, what, "scattered rays", dRaysOut, 4))
    return 1;
  if ((uintptr_t)dHits % 16) return fail(ctx, "%s: the hits are not aligned to 16 bytes", what);
  const DevScene& sc = ctx->upload.scene;
  const size_t lds = srtQueryStackBytes(sc.stackDepth);  // the walk's stacks, as queryDevice sizes and bounds them
  if (checkWalkLds(ctx, what, lds)) return 1;
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

// ---------------------------------------------------------------- srtCompactPathsDevice / srtSortPathsDevice
// The payloads of both, filled here and nowhere else
static PathPayloads pathPayloads(int64_t n, const void* dOut, const void* dActive, const void* dRays, const void* dRng, const void* dSlot,
                                 void* dRaysOut, void* dRngOut, void* dSlotOut, void* dActiveOut, void* dCount) {
  PathPayloads p;
  p.out = static_cast<const int32_t*>(dOut);
  p.active = static_cast<const uint8_t*>(dActive);
  p.rays = static_cast<const uint32_t*>(dRays);
  p.rng = static_cast<const uint64_t*>(dRng);
  p.slot = static_cast<const int32_t*>(dSlot);
  p.raysOut = static_cast<uint32_t*>(dRaysOut);
  p.rngOut = static_cast<uint64_t*>(dRngOut);
  p.slotOut = static_cast<int32_t*>(dSlotOut);
  p.activeOut = static_cast<uint8_t*>(dActiveOut);
  p.count = static_cast<int64_t*>(dCount);
  p.n = n;
  return p;
}

// What the two ask of their payloads (n > 0): an output has its input, everything that is read or written is aligned, and
// what the kernels write overlaps nothing else they read or write (activeOut may BE the mask: an entry owns its byte).  An
// input whose output is null is not read and takes no part -- but for the rays of the sort (raysRead), which its key
// reads.  made: "compacted" or "sorted"; dBox: the sort's, else null.
static int checkPayloads(SrtContext* ctx, const char* what, const char* made, const PathPayloads& p, bool raysRead, const void* dBox,
                         const void* dScratch, int64_t scratchBytes) {
  if (p.raysOut && !p.rays) return fail(ctx, "%s: %s rays without rays", what, made);
  if (p.rngOut && !p.rng) return fail(ctx, "%s: %s rng states without rng states", what, made);
  raysRead = raysRead || p.raysOut;
  if ((uintptr_t)p.out % 16) return fail(ctx, "%s: the outputs are not aligned to 16 bytes", what);
  if ((raysRead && (uintptr_t)p.rays % 4) || (uintptr_t)p.raysOut % 4) return fail(ctx, "%s: the rays are not aligned to 4 bytes", what);
  if ((p.rngOut && (uintptr_t)p.rng % 8) || (uintptr_t)p.rngOut % 8) return fail(ctx, "%s: the rng states are not aligned to 8 bytes", what);
  if ((p.slotOut && (uintptr_t)p.slot % 4) || (uintptr_t)p.slotOut % 4) return fail(ctx, "%s: the slots are not aligned to 4 bytes", what);
  char names[4][40];
  const char* const payload[4] = {"rays", "rng states", "slots", "mask"};
  for (int k = 0; k < 4; ++k) snprintf(names[k], sizeof names[k], "%s %s", made, payload[k]);
  const uint64_t un = (uint64_t)p.n;
  const PathRange ranges[] = {{"outputs", (uintptr_t)p.out, 32 * un, false},
                              {"mask", (uintptr_t)p.active, un, false},
                              {"rays", raysRead ? (uintptr_t)p.rays : 0, 36 * un, false},
                              {"rng states", p.rngOut ? (uintptr_t)p.rng : 0, 8 * un, false},
                              {"slots", p.slotOut ? (uintptr_t)p.slot : 0, 4 * un, false},
                              {"box", (uintptr_t)dBox, 24, false},
                              {names[0], (uintptr_t)p.raysOut, 36 * un, true},
                              {names[1], (uintptr_t)p.rngOut, 8 * un, true},
                              {names[2], (uintptr_t)p.slotOut, 4 * un, true},
                              {names[3], (uintptr_t)p.activeOut, un, true},
                              {"count", (uintptr_t)p.count, 8, true},
                              {"scratch", (uintptr_t)dScratch, (uint64_t)scratchBytes, true}};
  return checkPathRanges(ctx, what, ranges, sizeof ranges / sizeof ranges[0], &ranges[1], &ranges[9]);
}

// srtCompactPathsDevice: srt_compact.hip's three launches.  Needs no scene.
static int64_t compactTiles(int64_t n) { return n <= 0 ? 0 : (n - 1) / SRT_COMPACT_TILE + 1; }

static int compactPathsDevice(SrtContext* ctx, const PathPayloads& p, void* dScratch, void* streamPtr) {
  const char* what = "srtCompactPathsDevice";
  if (!ctx) return 1;
  if (checkCount(ctx, what, p.n)) return 1;
  if (!p.out && !p.active) return fail(ctx, "%s: no predicate: the outputs and the mask are both null", what);
  if (checkPointer(ctx, what, "count", p.count, 8)) return 1;
  if (p.n == 0) return 0;
  if (checkPointer(ctx, what, "scratch", dScratch, 8)) return 1;
  if (p.slotOut && p.n > 0x7fffffffll) return fail(ctx, "%s: n = %lld does not fit a 32-bit slot", what, (long long)p.n);
  if (checkPayloads(ctx, what, "compacted", p, false, nullptr, dScratch, srtCompactPathsScratchBytes(p.n))) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  CompactArgs a;
  a.p = p;
  a.tileOffset = static_cast<uint64_t*>(dScratch);
  a.numTiles = compactTiles(p.n);
  const int grid = (int)std::min<int64_t>(a.numTiles, (int64_t)ctx->prop.multiProcessorCount * 8);
  const int e = srt_launch_compact(&a, grid, static_cast<hipStream_t>(streamPtr));
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

// srtSortPathsDevice: srt_sort.hip's memset, key kernel, rocPRIM sort and gather kernel.  Needs no scene.  The scratch: four
// arrays of n 32-bit words (key and index, twice: the sort's double buffers), each rounded up to 256 bytes, and behind them
// the sort's temporary storage.  srtSortPathsScratchBytes runs without a device, so that part is a bound that grows with n
// -- 4 bytes per entry and 64 KB: with double buffers rocPRIM asks for digit histograms and, per block of at least 256
// entries, one 32-bit look-back word per digit or one merge partition -- and the call compares what the installed rocPRIM
// asks for with it.
static int64_t sortArrayBytes(int64_t n) { return (4 * n + 255) & ~(int64_t)255; }
static int64_t sortTempBytes(int64_t n) { return sortArrayBytes(n) + 65536; }

static int sortPathsDevice(SrtContext* ctx, const PathPayloads& p, int32_t cellBits, const void* dBox, void* dScratch, int64_t scratchBytes,
                           void* streamPtr) {
  const char* what = "srtSortPathsDevice";
  const int64_t n = p.n;
  if (!ctx) return 1;
  if (checkCount(ctx, what, n)) return 1;
  if (n > 0x7fffffffll) return fail(ctx, "%s: n = %lld does not fit a 32-bit index", what, (long long)n);
  if (cellBits < 1 || cellBits > SRT_SORT_MAX_CELL_BITS)
    return fail(ctx, "%s: cellBits = %d is outside [1, %d]", what, cellBits, (int)SRT_SORT_MAX_CELL_BITS);
  if (checkPointer(ctx, what, "count", p.count, 8)) return 1;
  if (n == 0) return 0;
  if (checkPointer(ctx, what, "scratch", dScratch, 8) || checkPointer(ctx, what, "box", dBox, 4) ||
      checkPointer(ctx, what, "rays", p.rays, 4))
    return 1;
  if (scratchBytes < srtSortPathsScratchBytes(n))
    return fail(ctx, "%s: the scratch holds %lld bytes, n = %lld needs %lld", what, (long long)scratchBytes, (long long)n,
                (long long)srtSortPathsScratchBytes(n));
  if (checkPayloads(ctx, what, "sorted", p, true, dBox, dScratch, srtSortPathsScratchBytes(n))) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  size_t tempNeeded = 0;
  int e = srt_sort_temp_bytes(n, cellBits, stream, &tempNeeded);
  if (e) return fail(ctx, "%s: the sort's size query failed: %s", what, hipGetErrorString((hipError_t)e));
  if ((int64_t)tempNeeded > sortTempBytes(n))
    return fail(ctx, "%s: rocPRIM asks for %zu bytes of temporary storage, the scratch reserves %lld", what, tempNeeded,
                (long long)sortTempBytes(n));
  SortArgs a;
  a.p = p;
  a.box = static_cast<const float*>(dBox);
  char* base = static_cast<char*>(dScratch);
  const int64_t array = sortArrayBytes(n);
  a.keys = reinterpret_cast<uint32_t*>(base);
  a.keysSpare = reinterpret_cast<uint32_t*>(base + array);
  a.index = reinterpret_cast<uint32_t*>(base + 2 * array);
  a.indexSpare = reinterpret_cast<uint32_t*>(base + 3 * array);
  a.temp = base + 4 * array;
  a.tempBytes = (size_t)sortTempBytes(n);
  a.cellBits = cellBits;
  const int grid = (int)std::min<int64_t>((n - 1) / SRT_BLOCK + 1, (int64_t)ctx->prop.multiProcessorCount * 8);
  e = srt_launch_sort(&a, grid, stream);
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

// ---------------------------------------------------------------- srtTracePathsDevice / srtTracePathsDirectDevice
// srt_paths.hip's memset and its one kernel.  direct: the DIRECT instance, with the upload's sampled-light table.
static int tracePathsDevice(SrtContext* ctx, bool direct, int32_t traversal, int32_t maxBounce, const float* background, const void* dRays,
                            int64_t n, void* dRng, void* dResult, void* dScratch, void* streamPtr) {
  const char* what = direct ? "srtTracePathsDirectDevice" : "srtTracePathsDevice";
  if (!ctx) return 1;
  if (checkSceneReady(ctx, what) || checkCount(ctx, what, n) || checkTraversal(ctx, what, traversal)) return 1;
  if (maxBounce < 0 || maxBounce > SRT_MAX_BOUNCE) return fail(ctx, "%s: maxBounce = %d is outside [0, %d]", what, maxBounce, SRT_MAX_BOUNCE);
  if (!background) return fail(ctx, "%s: null background", what);
  if (n == 0) return 0;
  if (checkPointer(ctx, what, "rays", dRays, 4) || checkPointer(ctx, what, "rng states", dRng, 8) ||
      checkPointer(ctx, what, "results", dResult, 16) || checkPointer(ctx, what, "scratch", dScratch, 8))
    return 1;
  // what the kernel writes may overlap nothing else it reads or writes
  const uint64_t un = (uint64_t)n;
  const PathRange ranges[] = {{"rays", (uintptr_t)dRays, 36 * un, false},
                              {"rng states", (uintptr_t)dRng, 8 * un, true},
                              {"results", (uintptr_t)dResult, 16 * un, true},
                              {"scratch", (uintptr_t)dScratch, SRT_PATHS_SCRATCH_BYTES, true}};
  if (checkPathRanges(ctx, what, ranges, sizeof ranges / sizeof ranges[0], nullptr, nullptr, true)) return 1;
  const DevScene& sc = ctx->upload.scene;
  const size_t lds = direct ? srtPathsDirectLdsBytes(sc.stackDepth, maxBounce) : srtPathsLdsBytes(sc.stackDepth, maxBounce);
  if (checkWalkLds(ctx, what, lds, maxBounce)) return 1;
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
  int e;
  if (direct) {
    TracePathsDirectArgs d;
    d.p = a;
    d.lights = ctx->upload.sampledLights;
    d.numLights = (int32_t)ctx->upload.sampledLightPrims.size();
    e = srt_launch_paths_direct(&d, traversal, ctx->prop.multiProcessorCount, lds, SRT_PATHS_SCRATCH_BYTES, static_cast<hipStream_t>(streamPtr));
  } else {
    e = srt_launch_paths(&a, traversal, ctx->prop.multiProcessorCount, lds, SRT_PATHS_SCRATCH_BYTES, static_cast<hipStream_t>(streamPtr));
  }
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

// ---------------------------------------------------------------- srtGetSampledLights / srtDirectLightDevice / srtTestEvalScatterDevice
static int getSampledLights(SrtContext* ctx, int32_t* prims, int32_t capacity, int32_t* count) {
  const char* what = "srtGetSampledLights";
  if (!ctx) return 1;
  if (!ctx->upload.haveScene) return fail(ctx, "%s: no scene uploaded", what);
  if (!count) return fail(ctx, "%s: null count", what);
  const std::vector<int32_t>& lights = ctx->upload.sampledLightPrims;
  *count = (int32_t)lights.size();
  if (prims) {
    if (capacity < *count) return fail(ctx, "%s: capacity %d < %d", what, capacity, *count);
    std::copy(lights.begin(), lights.end(), prims);
  }
  return 0;
}

// One launch of srt_direct.hip
static int directLightDevice(SrtContext* ctx, int32_t traversal, const void* dRays, const void* dRecords, int64_t n, const void* dRng,
                             void* dDirect, void* streamPtr) {
  const char* what = "srtDirectLightDevice";
  if (!ctx) return 1;
  if (checkSceneReady(ctx, what) || checkCount(ctx, what, n) || checkTraversal(ctx, what, traversal)) return 1;
  if (n == 0) return 0;
  if (checkPointer(ctx, what, "rays", dRays, 4) || checkPointer(ctx, what, "records", dRecords, 4) ||
      checkPointer(ctx, what, "rng states", dRng, 8) || checkPointer(ctx, what, "direct terms", dDirect, 16))
    return 1;
  const uint64_t un = (uint64_t)n;
  const PathRange ranges[] = {{"rays", (uintptr_t)dRays, 36 * un, false},
                              {"records", (uintptr_t)dRecords, sizeof(SrtHit) * un, false},
                              {"rng states", (uintptr_t)dRng, 8 * un, false},
                              {"direct terms", (uintptr_t)dDirect, 32 * un, true}};
  if (checkPathRanges(ctx, what, ranges, sizeof ranges / sizeof ranges[0], nullptr, nullptr)) return 1;
  const DevScene& sc = ctx->upload.scene;
  const size_t lds = srtQueryStackBytes(sc.stackDepth);  // the shadow ray's walk, as queryDevice sizes and bounds it
  if (checkWalkLds(ctx, what, lds)) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  DirectLightArgs a;
  a.scene = sc;
  a.rays = static_cast<const float*>(dRays);
  a.records = static_cast<const SrtHit*>(dRecords);
  a.rng = static_cast<const uint64_t*>(dRng);
  a.direct = static_cast<int4*>(dDirect);
  a.lights = ctx->upload.sampledLights;
  a.numLights = (int32_t)ctx->upload.sampledLightPrims.size();
  a.n = n;
  const int e = srt_launch_direct_light(&a, traversal, pathGrid(ctx, n), lds, static_cast<hipStream_t>(streamPtr));
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

static int evalScatterDevice(SrtContext* ctx, const void* dRays, const void* dRecords, const void* dDirs, int64_t n, void* dAtt) {
  const char* what = "srtTestEvalScatterDevice";
  if (!ctx) return 1;
  if (checkSceneReady(ctx, what) || checkCount(ctx, what, n)) return 1;
  if (n == 0) return 0;
  if (checkPointer(ctx, what, "rays", dRays, 4) || checkPointer(ctx, what, "records", dRecords, 4) ||
      checkPointer(ctx, what, "directions", dDirs, 4) || checkPointer(ctx, what, "attenuations", dAtt, 4))
    return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  EvalScatterArgs a;
  a.scene = ctx->upload.scene;
  a.rays = static_cast<const float*>(dRays);
  a.records = static_cast<const SrtHit*>(dRecords);
  a.dirs = static_cast<const float*>(dDirs);
  a.att = static_cast<float*>(dAtt);
  a.n = n;
  const int e = srt_launch_eval_scatter(&a, pathGrid(ctx, n), nullptr);
  if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
  return 0;
}

extern "C" {

int srtTraceRaysDevice(SrtContext* ctx, const void* dRays, int64_t n, int32_t traversal, void* dHits, void* dRecords, void* stream) {
  SRT_GUARDED(ctx, queryDevice(ctx, "srtTraceRaysDevice", dRays, n, false, traversal, dHits, dRecords, nullptr, stream));
}

int srtOccludedDevice(SrtContext* ctx, const void* dRays, int64_t n, void* dOccluded, void* stream) {
  SRT_GUARDED(ctx, queryDevice(ctx, "srtOccludedDevice", dRays, n, true, 0, nullptr, nullptr, dOccluded, stream));
}

uint64_t srtRngKey(uint64_t seed, uint64_t pixel, uint64_t sample) {  // the low 32 bits of pixel and of sample
  return hostMix64(hostMix64(seed) ^ ((pixel << 32) | (sample & 0xffffffffull)));
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

int64_t srtCompactPathsScratchBytes(int64_t n) { return 8 * compactTiles(n); }

int srtCompactPathsDevice(SrtContext* ctx, int64_t n, const void* dOut, const void* dActive, const void* dRays, const void* dRng,
                          const void* dSlot, void* dRaysOut, void* dRngOut, void* dSlotOut, void* dActiveOut, void* dCount,
                          void* dScratch, void* stream) {
  SRT_GUARDED(ctx, compactPathsDevice(ctx, pathPayloads(n, dOut, dActive, dRays, dRng, dSlot, dRaysOut, dRngOut, dSlotOut, dActiveOut, dCount),
                                      dScratch, stream));
}

int64_t srtSortPathsScratchBytes(int64_t n) { return n <= 0 ? 0 : 4 * sortArrayBytes(n) + sortTempBytes(n); }

int srtSortPathsDevice(SrtContext* ctx, int64_t n, int32_t cellBits, const void* dBox, const void* dOut, const void* dActive,
                       const void* dRays, const void* dRng, const void* dSlot, void* dRaysOut, void* dRngOut, void* dSlotOut,
                       void* dActiveOut, void* dCount, void* dScratch, int64_t scratchBytes, void* stream) {
  SRT_GUARDED(ctx, sortPathsDevice(ctx, pathPayloads(n, dOut, dActive, dRays, dRng, dSlot, dRaysOut, dRngOut, dSlotOut, dActiveOut, dCount),
                                   cellBits, dBox, dScratch, scratchBytes, stream));
}

int srtTracePathsDevice(SrtContext* ctx, int32_t traversal, int32_t maxBounce, const float background[3], const void* dRays, int64_t n,
                        void* dRng, void* dResult, void* dScratch, void* stream) {
  SRT_GUARDED(ctx, tracePathsDevice(ctx, false, traversal, maxBounce, background, dRays, n, dRng, dResult, dScratch, stream));
}

int srtTracePathsDirectDevice(SrtContext* ctx, int32_t traversal, int32_t maxBounce, const float background[3], const void* dRays,
                              int64_t n, void* dRng, void* dResult, void* dScratch, void* stream) {
  SRT_GUARDED(ctx, tracePathsDevice(ctx, true, traversal, maxBounce, background, dRays, n, dRng, dResult, dScratch, stream));
}

int srtGetSampledLights(SrtContext* ctx, int32_t* prims, int32_t capacity, int32_t* count) {
  SRT_GUARDED(ctx, getSampledLights(ctx, prims, capacity, count));
}

int srtDirectLightDevice(SrtContext* ctx, int32_t traversal, const void* dRays, const void* dRecords, int64_t n, const void* dRng,
                         void* dDirect, void* stream) {
  SRT_GUARDED(ctx, directLightDevice(ctx, traversal, dRays, dRecords, n, dRng, dDirect, stream));
}

int srtTestEvalScatterDevice(SrtContext* ctx, const void* dRays, const void* dRecords, const void* dDirs, int64_t n, void* dAtt) {
  SRT_GUARDED(ctx, evalScatterDevice(ctx, dRays, dRecords, dDirs, n, dAtt));
}

}  // extern "C"
