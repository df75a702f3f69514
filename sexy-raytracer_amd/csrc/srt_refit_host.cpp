// srt_refit_host.cpp -- host side of the geometry updates (include/srt_hip.h srtUpdateTriangles / srtUpdateSpheres /
// srtRefitScene): argument checks, the device tables an uploaded scene needs for them (made by the first call that uses
// them, so an upload that is never updated pays nothing), and the launches of srt_refit.hip.  Also srtSetMotionTracking
// and the snapshot of the previous epoch's records that the motion pass reads (include/srt_hip.h "Motion"), srtRebuildScene
// (a refit behind new device builds) and srtGetTreeCost.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "srt_context.h"
#include "srt_launch.h"

namespace {

// Everything an update entry checks before it touches the device.  Returns 0 to go on, 1 for an error, 2 for the no-op.
int checkUpdate(SrtContext* ctx, const char* what, int32_t first, int32_t count, int32_t have, const void* in, size_t align) {
  if (!ctx->upload.haveScene) return fail(ctx, "%s: no scene uploaded", what);
  if (first < 0 || count < 0 || (int64_t)first + count > have)
    return fail(ctx, "%s: range [%d, %d + %d) lies outside the scene's %d records", what, first, first, count, have);
  if (count == 0) return 2;
  if (!in) return fail(ctx, "%s: null records", what);
  if ((uintptr_t)in % align) return fail(ctx, "%s: records must be aligned to %zu bytes", what, align);
  return 0;
}

// The scene-to-device triangle table, on the device (identity when the upload did not reorder: null)
int triangleTable(SrtContext* ctx, const int32_t** out) {
  *out = nullptr;
  if (ctx->upload.hostTriDevIndex.empty()) return 0;
  if (!ctx->upload.triDevIndex.get()) {  // (srtUploadScene drops the previous scene's)
    HIP_OK(ctx, ctx->upload.triDevIndex.reserve(ctx->upload.hostTriDevIndex.size() * sizeof(int32_t)));
    HIP_OK(ctx, hipMemcpy(ctx->upload.triDevIndex.get(), ctx->upload.hostTriDevIndex.data(), ctx->upload.hostTriDevIndex.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  *out = ctx->upload.triDevIndex.get<const int32_t>();
  return 0;
}

// srtSetMotionTracking's snapshot: triTest and spheres as they are now, into the buffers the upload owns, on `stream`.
// Taken once per epoch -- by its first update, ahead of that update's kernel, or by a refit that no update preceded.
int snapshotGeometry(SrtContext* ctx, hipStream_t stream) {
  Upload& up = ctx->upload;
  if (!ctx->motionTracking || up.epochSnapshot) return 0;
  const size_t triBytes = (size_t)up.scene.numTris * 48, sphBytes = (size_t)up.scene.numSpheres * 48;
  HIP_OK(ctx, up.prevTriTest.reserve(triBytes));
  HIP_OK(ctx, up.prevSpheres.reserve(sphBytes));
  if (triBytes) HIP_OK(ctx, hipMemcpyAsync(up.prevTriTest.get(), up.scene.triTest, triBytes, hipMemcpyDeviceToDevice, stream));
  if (sphBytes) HIP_OK(ctx, hipMemcpyAsync(up.prevSpheres.get(), up.scene.spheres, sphBytes, hipMemcpyDeviceToDevice, stream));
  up.haveSnapshot = up.epochSnapshot = true;
  return 0;
}

int setMotionTracking(SrtContext* ctx, int32_t enable) {
  if (!ctx) return 1;
  if (ctx->upload.geometryDirty) return fail(ctx, "srtSetMotionTracking: geometry was updated; call srtRefitScene first");
  ctx->motionTracking = enable != 0;
  if (!ctx->motionTracking) {
    (void)hipSetDevice(ctx->device);
    ctx->upload.prevTriTest = DeviceBuffer();
    ctx->upload.prevSpheres = DeviceBuffer();
    ctx->upload.haveSnapshot = ctx->upload.epochSnapshot = false;
    if (ctx->temporalRefits) ctx->temporalValid = false;  // a history kept across a refit is of no use without its motion
    ctx->temporalRefits = 0;
  }
  return 0;
}

int updateTrianglesDevice(SrtContext* ctx, int32_t first, int32_t count, const void* dIn, void* stream) {
  if (!ctx) return 1;
  const int rc = checkUpdate(ctx, "srtUpdateTriangles", first, count, ctx->upload.haveScene ? ctx->upload.scene.numTris : 0, dIn, 16);
  if (rc) return rc == 2 ? 0 : 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  const int32_t* table = nullptr;
  if (triangleTable(ctx, &table)) return 1;
  if (snapshotGeometry(ctx, static_cast<hipStream_t>(stream))) return 1;
  ctx->upload.geometryDirty = true;
  const int e = srt_launch_refit_triangles(dIn, first, count, table, const_cast<float4*>(ctx->upload.scene.triTest),
                                           const_cast<float4*>(ctx->upload.scene.triShade), const_cast<float4*>(ctx->upload.scene.triFast),
                                           static_cast<hipStream_t>(stream));
  if (e) return fail(ctx, "srtUpdateTriangles: launch failed: %s", hipGetErrorString((hipError_t)e));
  return 0;
}

int updateSpheresDevice(SrtContext* ctx, int32_t first, int32_t count, const void* dIn, void* stream) {
  if (!ctx) return 1;
  const int rc = checkUpdate(ctx, "srtUpdateSpheres", first, count, ctx->upload.haveScene ? ctx->upload.scene.numSpheres : 0, dIn, 4);
  if (rc) return rc == 2 ? 0 : 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  if (snapshotGeometry(ctx, static_cast<hipStream_t>(stream))) return 1;
  ctx->upload.geometryDirty = true;
  const int e = srt_launch_refit_spheres(dIn, first, count, const_cast<float4*>(ctx->upload.scene.spheres), static_cast<hipStream_t>(stream));
  if (e) return fail(ctx, "srtUpdateSpheres: launch failed: %s", hipGetErrorString((hipError_t)e));
  return 0;
}

// The host forms: the records staged in the context's own device buffer, then the device form on the null stream (which
// orders the next call's copy into the same buffer behind this call's kernel)
template <typename Device>
int updateHost(SrtContext* ctx, const char* what, int32_t first, int32_t count, int32_t have, const void* hIn, size_t recordBytes, Device device) {
  if (!ctx) return 1;
  const int rc = checkUpdate(ctx, what, first, count, ctx->upload.haveScene ? have : 0, hIn, 1);
  if (rc) return rc == 2 ? 0 : 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, ctx->refitStage.reserve((size_t)count * recordBytes));
  HIP_OK(ctx, hipMemcpy(ctx->refitStage.get(), hIn, (size_t)count * recordBytes, hipMemcpyHostToDevice));
  return device(ctx, first, count, ctx->refitStage.get(), nullptr);
}

// srtRefitScene, and srtRebuildScene (`rebuild`): the same, behind new trees for the device-built items
int refitScene(SrtContext* ctx, void* streamPtr, bool rebuild) {
  if (!ctx) return 1;
  const char* const what = rebuild ? "srtRebuildScene" : "srtRefitScene";
  if (!ctx->upload.haveScene) return fail(ctx, "%s: no scene uploaded", what);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  const int n = ctx->upload.scene.numNodes;
  int32_t flag = 0;
  if (snapshotGeometry(ctx, stream)) return 1;  // tracking on and no update since the last refit: motion is zero
  if (rebuild && !ctx->upload.deviceBuilds.empty()) {
    // The builders read the records on the null stream and block: the updates' stream has to have passed them first.  A
    // failed build leaves trees that are neither the old nor the new ones: nothing renders until a rebuild succeeds.
    ctx->upload.geometryDirty = true;
    HIP_OK(ctx, hipStreamSynchronize(stream));
    if (buildDeviceTrees(ctx)) return 1;
    ctx->upload.refitLinksStale = true;
  }
  const DevScene& s = ctx->upload.scene;  // (read after the builds: they set its stack depth)
  if (n > 0) {
    if (!ctx->upload.refitTables) {
      // once per upload: the parent links' and counters' memory, and the hybrid records' renumbering
      HIP_OK(ctx, ctx->upload.refitUp.reserve((size_t)n * sizeof(int32_t)));
      HIP_OK(ctx, ctx->upload.refitArrived.reserve((size_t)n * sizeof(int32_t)));
      HIP_OK(ctx, ctx->refitFlag.reserve(16));
      if (s.nodesWf) {
        if (ctx->upload.hostWfIndex.size() != (size_t)n) return fail(ctx, "%s: the hybrid records have no renumbering", what);
        HIP_OK(ctx, ctx->upload.wfIndex.reserve((size_t)n * sizeof(int32_t)));
        HIP_OK(ctx, hipMemcpy(ctx->upload.wfIndex.get(), ctx->upload.hostWfIndex.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
      }
      ctx->upload.refitTables = ctx->upload.refitLinksStale = true;
    }
    if (ctx->upload.refitLinksStale) {
      // the parent links: once per topology, that is per upload and per rebuild (over the whole array: one pass over the
      // reference words, next to a build's dozens)
      const int e = srt_launch_refit_links(s.nodes, n, ctx->upload.refitUp.get<int32_t>(), stream);
      if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
      ctx->upload.refitLinksStale = false;
      if (s.nodesRg) {  // (a regrouped tree exists only without device builds: its topology is the upload's for good)
        HIP_OK(ctx, ctx->upload.refitUpRg.reserve((size_t)n * sizeof(int32_t)));
        const int eRg = srt_launch_refit_links(s.nodesRg, n, ctx->upload.refitUpRg.get<int32_t>(), stream);
        if (eRg) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)eRg));
      }
    }
    HIP_OK(ctx, hipMemsetAsync(ctx->upload.refitArrived.get(), 0, (size_t)n * sizeof(int32_t), stream));
    HIP_OK(ctx, hipMemsetAsync(ctx->refitFlag.get(), 0, 16, stream));
    int e = 0;
    for (const Upload::Tree& t : ctx->upload.trees) {
      if (t.base < 0 || t.count < 1 || t.base + t.count > n) return fail(ctx, "%s: world item %d lies outside the node array", what, t.item);
      e = srt_launch_refit_nodes(&s, t.base, t.count, t.time0, t.time1, ctx->upload.refitUp.get<const int32_t>(), ctx->upload.refitArrived.get<int32_t>(),
                                 ctx->refitFlag.get<int32_t>(), t.deviceBuilt ? 1 : 0, stream);
      if (e) break;
    }
    if (!e && s.nodesRg) {
      // The regrouped tree (srt_regroup.h) in the same pass, by the same kernel as it stands: a copy of the scene whose
      // node array is the regrouped one, its own parent links, the counters zeroed again behind the first pass.  Leaf
      // boxes come from the same primitive records by the same arithmetic, inner boxes are unions of their children's: the
      // topology stays valid (any grouping of the leaf sequence is).  flag: host-built items set no bit in this kernel.
      DevScene rg = s;
      rg.nodes = s.nodesRg;
      e = (int)hipMemsetAsync(ctx->upload.refitArrived.get(), 0, (size_t)n * sizeof(int32_t), stream);
      for (const Upload::Tree& t : ctx->upload.trees) {
        if (e) break;
        e = srt_launch_refit_nodes(&rg, t.base, t.count, t.time0, t.time1, ctx->upload.refitUpRg.get<const int32_t>(),
                                   ctx->upload.refitArrived.get<int32_t>(), ctx->refitFlag.get<int32_t>(), 0, stream);
      }
    }
    if (!e) e = srt_launch_refit_derived(&s, s.nodesWf ? ctx->upload.wfIndex.get<const int32_t>() : nullptr, ctx->refitFlag.get<int32_t>(), stream);
    if (!e) e = srt_pair_nodes_async(&s, ctx->upload.pairTime0, ctx->upload.pairTime1, const_cast<float4*>(s.nodes2), stream);
    if (e) return fail(ctx, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
    HIP_OK(ctx, hipMemcpyAsync(&flag, ctx->refitFlag.get(), sizeof flag, hipMemcpyDeviceToHost, stream));
  }
  if (hipStreamSynchronize(stream) != hipSuccess) return fail(ctx, "%s: kernel failed: %s", what, hipGetErrorString(hipGetLastError()));
  ctx->upload.scene.fastDivScene = (flag & 3) == 0 ? ctx->upload.fastDivOption : 0;
  ctx->upload.scene.boxOrderedScene = (flag & 4) == 0 ? 1 : 0;
  // Without tracking, as srtUploadScene: the reprojection assumes the surfaces of the history's frame.  With it, the history
  // stays and srtRenderTemporalFrame decides by the count of refits since its last frame (srt_frames.cpp)
  if (ctx->motionTracking) {
    if (ctx->temporalRefits < 2) ctx->temporalRefits++;
    ctx->upload.epochSnapshot = false;
  } else {
    ctx->temporalValid = false;
  }
  std::fill(ctx->upload.itemBoxesStale.begin(), ctx->upload.itemBoxesStale.end(), (uint8_t)1);
  ctx->upload.geometryDirty = false;
  return 0;
}

// srtGetTreeCost.  The device takes the pairwise sum down to at most SRT_COST_BLOCK partials, level by level between two
// halves of the scratch; the host finishes over the copied partials in the same order and divides by the root's term.
int treeCost(SrtContext* ctx, int32_t item, double* cost) {
  if (!ctx) return 1;
  if (checkSceneReady(ctx, "srtGetTreeCost")) return 1;
  if (!cost) return fail(ctx, "srtGetTreeCost: null cost");
  if (item < 0 || item >= ctx->upload.scene.numWorld) return fail(ctx, "srtGetTreeCost: item %d out of range", item);
  const auto t = std::find_if(ctx->upload.trees.begin(), ctx->upload.trees.end(), [&](const Upload::Tree& x) { return x.item == item; });
  if (t == ctx->upload.trees.end()) return fail(ctx, "srtGetTreeCost: item %d is not a bvh", item);
  if (t->base < 0 || t->count < 1 || t->base + t->count > ctx->upload.scene.numNodes) return fail(ctx, "srtGetTreeCost: world item %d lies outside the node array", item);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  auto blocks = [](int values) { return (values + SRT_COST_BLOCK - 1) / SRT_COST_BLOCK; };
  int have = blocks(t->count);
  const size_t half = (size_t)have + 1;  // the first level's sums and the root's term behind them
  HIP_OK(ctx, ctx->costScratch.reserve(2 * half * sizeof(double)));
  double* cur = ctx->costScratch.get<double>();
  double* other = cur + half;
  const double* const rootTerm = cur + have;
  int e = srt_launch_tree_cost_nodes(ctx->upload.scene.nodes + 2 * (size_t)t->base, t->count, cur, nullptr);
  while (!e && have > SRT_COST_BLOCK) {
    e = srt_launch_tree_cost_partials(cur, have, other, nullptr);  // (never reaches the root's term: blocks(have) < have)
    have = blocks(have);
    std::swap(cur, other);
  }
  if (e) return fail(ctx, "srtGetTreeCost: launch failed: %s", hipGetErrorString((hipError_t)e));
  size_t width = 1;
  while (width < (size_t)have) width *= 2;
  std::vector<double> x(width, 0.0);
  double root = 0.0;
  HIP_OK(ctx, hipMemcpy(x.data(), cur, (size_t)have * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(ctx, hipMemcpy(&root, rootTerm, sizeof root, hipMemcpyDeviceToHost));
  for (; width > 1; width /= 2)
    for (size_t k = 0; k < width / 2; ++k) x[k] = x[2 * k] + x[2 * k + 1];
  *cost = x[0] / root;
  return 0;
}

}  // namespace

extern "C" {

int srtUpdateTrianglesDevice(SrtContext* ctx, int32_t first, int32_t count, const void* dIn, void* stream) {
  SRT_GUARDED(ctx, updateTrianglesDevice(ctx, first, count, dIn, stream));
}
int srtUpdateSpheresDevice(SrtContext* ctx, int32_t first, int32_t count, const void* dIn, void* stream) {
  SRT_GUARDED(ctx, updateSpheresDevice(ctx, first, count, dIn, stream));
}
int srtUpdateTriangles(SrtContext* ctx, int32_t first, int32_t count, const SrtTriangleIn* hTris) {
  SRT_GUARDED(ctx, updateHost(ctx, "srtUpdateTriangles", first, count, ctx ? ctx->upload.scene.numTris : 0, hTris, sizeof(SrtTriangleIn), updateTrianglesDevice));
}
int srtUpdateSpheres(SrtContext* ctx, int32_t first, int32_t count, const SrtSphereIn* hSpheres) {
  SRT_GUARDED(ctx, updateHost(ctx, "srtUpdateSpheres", first, count, ctx ? ctx->upload.scene.numSpheres : 0, hSpheres, sizeof(SrtSphereIn), updateSpheresDevice));
}
int srtRefitScene(SrtContext* ctx, void* stream) { SRT_GUARDED(ctx, refitScene(ctx, stream, false)); }
int srtRebuildScene(SrtContext* ctx, void* stream) { SRT_GUARDED(ctx, refitScene(ctx, stream, true)); }
int srtGetTreeCost(SrtContext* ctx, int32_t item, double* cost) { SRT_GUARDED(ctx, treeCost(ctx, item, cost)); }
int srtSetMotionTracking(SrtContext* ctx, int32_t enable) { SRT_GUARDED(ctx, setMotionTracking(ctx, enable)); }

}  // extern "C"
