// srt_api.cpp -- host side of the C ABI (include/srt_hip.h): the context (srt_context.h) and its tunables, the upload of a
// flattened scene (srt_scene.cpp) with the device BVH builds, the BVH queries, timing, statistics and the test hooks
// (include/srt_hip_test.h).  The render launches are in srt_render.cpp, the entries on the caller's device buffers (ray
// queries, path steps) in srt_rays.cpp, the passes over a rendered frame in srt_passes.cpp, and the entries that render a
// whole frame into host buffers compose those in srt_frames.cpp.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "srt_context.h"
#include "srt_launch.h"
#include "srt_regroup.h"
#include "srt_thread.h"

int fail(SrtContext* ctx, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->error = buf;
  fprintf(stderr, "srt_hip: %s\n", buf);  // the reference reports on std::cerr (texture.h:64-67, bvh.h:37-38)
  return 1;
}

int wfCheck(SrtContext* ctx) {
  if (ctx->dWfError && *(volatile int32_t*)ctx->dWfError != 0) {
    const int n = *(volatile int32_t*)ctx->dWfError;
    *(volatile int32_t*)ctx->dWfError = 0;
    return fail(ctx, "render: %d workgroup(s) of the path-pool kernel gave up waiting on a ring; the frame is incomplete", n);
  }
  return 0;
}

namespace {

template <typename T>
int uploadVec(SrtContext* ctx, const std::vector<T>& v, const T** out, size_t padBytes = 0) {
  DeviceBuffer b;
  HIP_OK(ctx, b.reserve(std::max<size_t>(v.size() * sizeof(T) + padBytes, 16)));
  HIP_OK(ctx, hipMemset(b.get(), 0, b.bytes()));
  if (!v.empty()) HIP_OK(ctx, hipMemcpy(b.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = b.get<const T>();
  ctx->upload.sceneBuffers.push_back(std::move(b));
  return 0;
}

int envInt(const char* name, int dflt) {
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : dflt;
}

struct TunableName {
  const char* name;
  const char* env;
  int Tunables::*field;
  int dflt;
};
const TunableName kTunables[] = {
    {"tile_block", nullptr, &Tunables::tileBlock, SRT_TILE_BLOCK},  // no environment override: ranks must agree (tiles.py)
    {"unit_tiles", "SRT_UNIT_TILES", &Tunables::unitTiles, -1},
    {"queues", "SRT_QUEUES", &Tunables::queues, -1},
    {"shade_min", "SRT_SHADE_MIN", &Tunables::shadeMin, -1},    // -1: by traversal mode, see srtRenderTiles
    {"prim_min", "SRT_PRIM_MIN", &Tunables::primMin, 12},
    {"hit_min", "SRT_HIT_MIN", &Tunables::hitMin, 24},
    {"fuse_min", "SRT_FUSE_MIN", &Tunables::fuseMin, 32},
    {"node_burst", "SRT_NODE_BURST", &Tunables::nodeBurst, -1},
    {"ploc_radius", "SRT_PLOC_RADIUS", &Tunables::plocRadius, 64},
    {"fast_div", "SRT_FAST_DIV", &Tunables::fastDiv, 1},
    {"prim_again_min", "SRT_PRIM_AGAIN_MIN", &Tunables::primAgainMin, 4},
    {"keep_eighths", "SRT_KEEP_EIGHTHS", &Tunables::keepEighths, -1},
    {"chunk_scratch_mb", "SRT_CHUNK_SCRATCH_MB", &Tunables::chunkScratchMb, 12288},  // budget of the chunk-slot path
    {"lds_tree", "SRT_LDS_TREE", &Tunables::ldsTree, 1},  // FAITHFUL: node records in LDS when the whole array fits and has this many nodes; 0 = never
    // the path-pool kernel (srt_wavefront.hip) for the launches the LDS-resident tree serves whose tree has at least this
    // many nodes (traversal-heavy frames gain, shading-heavy ones with tiny trees lose: profiles/r03/wavefront.txt); 0 = never
    {"wavefront", "SRT_WAVEFRONT", &Tunables::wavefront, 256},
    {"wf_pool", "SRT_WF_POOL", &Tunables::wfPool, 2048},       // path contexts per workgroup (1024 lanes traverse)
    // lanes without a walk before a wave swaps finished walks for READY contexts; 0 = 32, and 16 in the hybrid form, whose
    // lanes are worth more refilled than waiting (profiles/r03/hybrid.txt)
    {"wf_swap_min", "SRT_WF_SWAP_MIN", &Tunables::wfSwapMin, 0},
    {"wf_swap_big", "SRT_WF_SWAP_BIG", &Tunables::wfSwapBig, 32},
    {"wf_profile", "SRT_WF_PROFILE", &Tunables::wfProfile, 0},  // 1: the profiling variant (tools/wf_profile.py, srtGetWfProfile)
    // path-pool kernel over a tree that does not fit into LDS: its top (the boxes with the largest surface, closed upward)
    // stays in LDS, the rest is read from global memory (srt_wavefront.hip HYBRID).  wf_hybrid 0 = never (such scenes run
    // the 256-thread kernel); wf_resident_max > 0 caps the resident nodes, which also sends trees that WOULD fit down
    // this path (the parity tests set it to a few dozen).  Both are read at srtUploadScene.
    {"wf_hybrid", "SRT_WF_HYBRID", &Tunables::wfHybrid, 1},
    {"wf_resident_max", "SRT_WF_RESIDENT_MAX", &Tunables::wfResidentMax, 0},
    // hybrid form: node visits per round, 1..4 (srt_wavefront.hip): the first of two overlaps the other lanes' loads.
    // 0 = 2 for trees of up to 2^20 nodes (cache-resident: +10 % and more), 1 beyond (HBM-bound soups of 4 M and 10 M
    // triangles lose 5-10 % with 2) -- profiles/r03/hybrid.txt
    {"wf_far_rounds", "SRT_WF_FAR_ROUNDS", &Tunables::wfFarRounds, 0},
    // path-pool kernel over a whole tree: walk the regrouped tree (srt_regroup.h, DevScene::nodesRg) where the upload built
    // one.  2 = its walk sequence, the gates that rarely cull a ray elided (srtRegroupWalk); 1 = the binary regrouped tree;
    // 0 = the reference tree: the same accumulators from about twice the node visits.  Read at every launch.
    {"wf_regroup", "SRT_WF_REGROUP", &Tunables::wfRegroup, 2},
    // path-pool kernel walking the sequence (wf_regroup 2): where every walk begins at a leaf of spheres alone (the headline's
    // ground: DevScene::wfHead), the swap step tests that leaf for the rays it sets up and starts their walks behind it.
    // 0 = every walk starts at the sequence's entry.  The same accumulators either way.  Read at every launch.
    {"wf_head", "SRT_WF_HEAD", &Tunables::wfHead, 1},
    // srtDenoise: a-trous levels of step <= this stage their (16 + 4 step)^2 window in LDS, larger steps read through the
    // caches (srt_denoise.hip; 8 at most, 0 = never) -- profiles/r05/denoise_bench.json
    {"denoise_lds_step", "SRT_DENOISE_LDS_STEP", &Tunables::denoiseLdsStep, 4},
    // FAITHFUL render and trace kernels: the triangle test's edge signs from the certified one-FMA forms over the triFast
    // records, the exact test for the lanes they cannot decide (srt_tri_hit.h): the kernels over an LDS-resident tree and
    // srtTraceRays.  0 = every test is the exact one.  The image, t and every counter are the same either way.
    {"tri_cert", "SRT_TRI_CERT", &Tunables::triCert, 1},
    // srtTracePathsDevice (srt_paths.hip): a wave claims entries for its idle lanes when at least this many are idle, 1..64
    // (a wave that is idle altogether always does).  16 = a quarter of the wave: fewer atomics, and fresh coherent rays are
    // not mixed one by one into a wave of bounced ones; 1 = on every trip, 3-14 % slower on the mesh and 0.6 % faster on
    // the soup.  The radiance does not depend on it.  Read at every call.
    {"paths_refill_min", "SRT_PATHS_REFILL_MIN", &Tunables::pathsRefillMin, 16},
};

// DevScene::triWMax for the tunable "tri_cert": the certificate's overflow guard, or 0 = nothing is certified
float triWMaxFor(const SrtContext* ctx) { return ctx->tun.triCert ? SRT_TRI_W_MAX : 0.0f; }

}  // namespace

int checkSceneReady(SrtContext* ctx, const char* what) {
  if (!ctx->upload.haveScene) return fail(ctx, "%s: no scene uploaded", what);
  if (ctx->upload.geometryDirty) return fail(ctx, "%s: geometry was updated; call srtRefitScene before anything traverses the scene", what);
  return 0;
}

// Every device-built item's tree from the current primitive records into its node slots, and the scene's depths: the
// maxima over the host-built trees' and these.  Blocking (the builders work on the null stream and read their depth
// back).  srtUploadScene's builds and srtRebuildScene's are this one function.
int buildDeviceTrees(SrtContext* ctx) {
  Upload& up = ctx->upload;
  DevScene& s = up.scene;
  int stackDepth = up.hostStackDepth, bvhDepth = up.hostBvhDepth;
  for (size_t k = 0; k < up.deviceBuilds.size(); ++k) {
    const DeviceBuild& b = up.deviceBuilds[k];
    const int32_t* refs = up.buildRefs[k].get<int32_t>();
    const int n = (int)(up.buildRefs[k].bytes() / sizeof(int32_t));
    int depth = 0;
    const int rc = b.builder == SRT_BUILDER_PLOC
                       ? srt_ploc_build(&s, refs, n, b.time0, b.time1, const_cast<float4*>(s.nodes), const_cast<uint8_t*>(s.nodeAxis),
                                        b.base, up.plocRadius, &depth)
                       : srt_lbvh_build(&s, refs, n, b.time0, b.time1, const_cast<float4*>(s.nodes), const_cast<uint8_t*>(s.nodeAxis),
                                        b.base, &depth);
    if (rc) return fail(ctx, "device BVH build of world item %d failed: %s", b.item, hipGetErrorString((hipError_t)rc));
    stackDepth = std::max(stackDepth, depth);
    bvhDepth = std::max(bvhDepth, depth);
  }
  s.stackDepth = stackDepth;
  up.bvhDepth = bvhDepth;
  return 0;
}

static int srtUploadSceneImpl(SrtContext* ctx, const SrtSceneDesc* d) {
  if (!ctx || !d) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  // everything that belonged to the previous scene, its device memory included, goes before the new scene is flattened
  // and allocated: a failed upload leaves the context without a scene
  ctx->upload = Upload();
  ctx->temporalValid = false;  // a history belongs to its scene
  std::string err = validateScene(d);
  HostScene h;
  if (err.empty()) err = flattenScene(d, SceneOptions{ctx->tun.wfHybrid, ctx->tun.wfResidentMax, ctx->tun.fastDiv}, h);
  if (!err.empty()) return fail(ctx, "%s", err.c_str());

  DevScene& s = ctx->upload.scene;
  if (!h.nodeThread.empty() && uploadVec(ctx, h.nodeThread, &s.nodeThread)) return 1;
  if (!h.nodesRg.empty() && (uploadVec(ctx, h.nodesRg, &s.nodesRg) || uploadVec(ctx, h.nodeThreadRg, &s.nodeThreadRg))) return 1;
  if (!h.walkSeq.empty() && uploadVec(ctx, h.walkSeq, &s.walkSeq)) return 1;
  s.numWalk = h.walkSeq.empty() ? 0 : h.numWalk;
  s.wfHead = h.walkSeq.empty() ? 0 : h.wfHead;
  if (!h.nodesWf.empty() && (uploadVec(ctx, h.nodesWf, &s.nodesWf) || uploadVec(ctx, h.worldWf, &s.worldWf) || uploadVec(ctx, h.primSecond, &s.primSecond))) return 1;
  if (uploadVec(ctx, h.primClass, &s.primClass, 16) || uploadVec(ctx, h.nodeAxis, &s.nodeAxis, 64) || uploadVec(ctx, h.nodes, &s.nodes) ||
      uploadVec(ctx, h.triTest, &s.triTest) || uploadVec(ctx, h.triFast, &s.triFast) || uploadVec(ctx, h.triShade, &s.triShade) || uploadVec(ctx, h.spheres, &s.spheres) ||
      uploadVec(ctx, h.triPrimId, &s.triPrimId) || uploadVec(ctx, h.sphPrimId, &s.sphPrimId) || uploadVec(ctx, h.world, &s.world) ||
      uploadVec(ctx, h.materials, &s.materials) || uploadVec(ctx, h.shadeRecs, &s.shadeRecs) || uploadVec(ctx, h.textures, &s.textures) ||
      uploadVec(ctx, h.texels, &s.texels, 64))
    return 1;
  s.wfResident = h.wfResident;
  s.numPrimClass = (int32_t)h.primClass.size();
  s.numWorld = (int32_t)h.world.size();
  s.stackDepth = h.stackDepth;
  s.numNodes = (int32_t)(h.nodes.size() / 2);
  s.numTris = d->numTriangles;
  s.numSpheres = d->numSpheres;
  s.numMaterials = d->numMaterials;
  s.texelBytes = (int32_t)h.texels.size();
  s.fastDivScene = h.fastDivScene;
  s.boxOrderedScene = h.boxOrderedScene;
  s.triWMax = triWMaxFor(ctx);
  ctx->upload.bvhDepth = h.bvhDepth;
  // device-built trees (srt_lbvh.hip) into the node slots the flattening reserved.  Their refs stay on the device for
  // srtRebuildScene (buildDeviceTrees)
  ctx->upload.hostStackDepth = h.stackDepth;
  ctx->upload.hostBvhDepth = h.bvhDepth;
  ctx->upload.plocRadius = ctx->tun.plocRadius;
  for (DeviceBuild& b : h.deviceBuilds) {
    DeviceBuffer refs;
    HIP_OK(ctx, refs.reserve(b.refs.size() * sizeof(int32_t)));
    HIP_OK(ctx, hipMemcpy(refs.get(), b.refs.data(), b.refs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    ctx->upload.buildRefs.push_back(std::move(refs));
    b.refs = std::vector<int32_t>();
  }
  ctx->upload.deviceBuilds = std::move(h.deviceBuilds);
  if (buildDeviceTrees(ctx)) return 1;
  // the closest-hit traversal's records: both children's boxes per node (srt_lbvh.hip pairNodes), built on the device
  // from the finished node array (host-built and device-built trees alike)
  float t0 = d->world[0].time0, t1 = d->world[0].time1;
  for (int w = 1; w < d->numWorld; ++w) {
    t0 = std::min(t0, d->world[w].time0);
    t1 = std::max(t1, d->world[w].time1);
  }
  DeviceBuffer nodes2;
  HIP_OK(ctx, nodes2.reserve(std::max<size_t>((size_t)s.numNodes * 64, 64)));
  s.nodes2 = nodes2.get<const float4>();
  ctx->upload.sceneBuffers.push_back(std::move(nodes2));
  const int rc = srt_pair_nodes(&s, t0, t1, const_cast<float4*>(s.nodes2));
  if (rc) return fail(ctx, "pairing the node records failed: %s", hipGetErrorString((hipError_t)rc));
  ctx->upload.itemNodes = std::move(h.itemNodes);
  // what an update and a refit need of this upload (srt_refit_host.cpp)
  for (const HostTree& t : h.hostTrees) ctx->upload.trees.push_back(Upload::Tree{t.item, t.base, t.count, t.time0, t.time1, false});
  for (const DeviceBuild& b : ctx->upload.deviceBuilds) ctx->upload.trees.push_back(Upload::Tree{b.item, b.base, b.count, b.time0, b.time1, true});
  ctx->upload.hostTriDevIndex = std::move(h.triDevIndex);
  ctx->upload.hostWfIndex = std::move(h.wfIndex);
  ctx->upload.itemBoxesStale.assign(ctx->upload.itemNodes.size(), 0);
  ctx->upload.pairTime0 = t0;
  ctx->upload.pairTime1 = t1;
  ctx->upload.fastDivOption = ctx->tun.fastDiv;
  const std::vector<int32_t> lights = sampledLights(h);
  if (uploadVec(ctx, lights, &ctx->upload.sampledLights)) return 1;
  for (int32_t sphere : lights) ctx->upload.sampledLightPrims.push_back(h.sphPrimId[sphere]);
  ctx->upload.hostTriPrimId = std::move(h.triPrimId);
  ctx->upload.hostSphPrimId = std::move(h.sphPrimId);
  ctx->upload.haveScene = true;
  return 0;
}
// Host-only: build world item `item` exactly as srtUploadScene does, without a device.
static int srtBuildBvhImpl(const SrtSceneDesc* d, int32_t item, SrtBvhNode* out, int32_t capacity, int32_t* count, int32_t* stackDepth) {
  if (!d || !count) return 1;
  const std::string invalid = validateScene(d);
  if (!invalid.empty()) return fail(nullptr, "%s", invalid.c_str());
  if (item < 0 || item >= d->numWorld || d->world[item].kind != SRT_WORLD_BVH) return fail(nullptr, "srtBuildBvh: item %d is not a bvh", item);
  Builder b;
  buildItem(d, d->world[item], b);
  *count = (int32_t)b.nodes.size();
  if (stackDepth) *stackDepth = b.maxPending;
  if (out) {
    if (capacity < *count) return fail(nullptr, "srtBuildBvh: capacity too small");
    b.toBvhNodes(out);
  }
  return 0;
}

// The boxes of a tree's node records as they lie in DevScene::nodes (raw: two float4 per node) into its SrtBvhNode copy
static void copyBoxes(const std::vector<float4>& raw, std::vector<SrtBvhNode>& out) {
  for (size_t i = 0; i < raw.size() / 2; ++i) {
    out[i].bmin[0] = raw[2 * i].x; out[i].bmin[1] = raw[2 * i].y; out[i].bmin[2] = raw[2 * i].z;
    out[i].bmax[0] = raw[2 * i + 1].x; out[i].bmax[1] = raw[2 * i + 1].y; out[i].bmax[2] = raw[2 * i + 1].z;
  }
}

static int srtGetBvhImpl(SrtContext* ctx, int32_t item, SrtBvhNode* nodes, int32_t capacity, int32_t* count) {
  if (!ctx || !count) return 1;
  if (item < 0 || item >= (int32_t)ctx->upload.itemNodes.size()) return fail(ctx, "srtGetBvh: item %d out of range", item);
  const auto dt = std::find_if(ctx->upload.deviceBuilds.begin(), ctx->upload.deviceBuilds.end(), [&](const DeviceBuild& b) { return b.item == item; });
  if (ctx->upload.itemBoxesStale[item]) {
    // srtRefitScene has moved the boxes since this copy was made: a device-built tree is read back again (below), a
    // host-built one gets the device's boxes (its children stay in the host convention)
    ctx->upload.itemBoxesStale[item] = 0;
    auto& out = ctx->upload.itemNodes[item];
    const auto tr = std::find_if(ctx->upload.trees.begin(), ctx->upload.trees.end(), [&](const Upload::Tree& t) { return t.item == item; });
    if (dt != ctx->upload.deviceBuilds.end()) {
      out.clear();
    } else if (tr != ctx->upload.trees.end() && !out.empty()) {
      std::vector<float4> raw((size_t)tr->count * 2);
      HIP_OK(ctx, hipMemcpy(raw.data(), ctx->upload.scene.nodes + 2 * (size_t)tr->base, raw.size() * sizeof(float4), hipMemcpyDeviceToHost));
      copyBoxes(raw, out);
    }
  }
  if (dt != ctx->upload.deviceBuilds.end() && ctx->upload.itemNodes[item].empty()) {
    // device-built tree: read it back once, converting child refs to the host convention
    std::vector<float4> raw((size_t)dt->count * 2);
    HIP_OK(ctx, hipMemcpy(raw.data(), ctx->upload.scene.nodes + 2 * (size_t)dt->base, raw.size() * sizeof(float4), hipMemcpyDeviceToHost));
    auto& out = ctx->upload.itemNodes[item];
    out.resize(dt->count);
    auto conv = [&](float bits) -> int32_t {
      int32_t r;
      memcpy(&r, &bits, 4);
      if (r >= 0) return SRT_NODE_INDEX(r) - dt->base;
      int32_t pr = ~r;
      return ~((pr & 1) ? ctx->upload.hostSphPrimId[pr >> 1] : ctx->upload.hostTriPrimId[pr >> 1]);
    };
    copyBoxes(raw, out);
    for (int i = 0; i < dt->count; ++i) {
      out[i].left = conv(raw[2 * i].w);
      out[i].right = conv(raw[2 * i + 1].w);
    }
  }
  const auto& v = ctx->upload.itemNodes[item];
  *count = (int32_t)v.size();
  if (nodes) {
    if (capacity < (int32_t)v.size()) return fail(ctx, "srtGetBvh: capacity %d < %zu", capacity, v.size());
    memcpy(nodes, v.data(), v.size() * sizeof(SrtBvhNode));
  }
  return 0;
}

extern "C" {

int srtCreate(int deviceOrdinal, SrtContext** out) {
  if (!out) return 1;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(nullptr, "no HIP device available (%s)", hipGetErrorString(e));
  if (deviceOrdinal < 0 || deviceOrdinal >= n) return fail(nullptr, "device ordinal %d out of range [0,%d)", deviceOrdinal, n);
  SrtContext* ctx = new SrtContext();
  ctx->device = deviceOrdinal;
  for (const TunableName& t : kTunables) ctx->tun.*(t.field) = t.env ? envInt(t.env, t.dflt) : t.dflt;
  HIP_OK(ctx, hipSetDevice(deviceOrdinal));
  HIP_OK(ctx, hipGetDeviceProperties(&ctx->prop, deviceOrdinal));
  HIP_OK(ctx, ctx->dQueue.reserve(SRT_MAX_QUEUES * 16 * sizeof(int32_t)));
  HIP_OK(ctx, ctx->dStats.reserve(96 * sizeof(unsigned long long)));
  HIP_OK(ctx, hipEventCreate(&ctx->evStart));
  HIP_OK(ctx, hipEventCreate(&ctx->evStop));
  // the word a path-pool workgroup that gave up adds to: host memory the device writes, so that the host can look at it
  // without a synchronisation of its own (wfCheck)
  HIP_OK(ctx, hipHostMalloc((void**)&ctx->dWfError, sizeof(int32_t), hipHostMallocMapped));
  *ctx->dWfError = 0;
  *out = ctx;
  return 0;
}

int srtDestroy(SrtContext* ctx) {
  if (!ctx) return 0;
  (void)hipSetDevice(ctx->device);
  (void)srtCommDestroy(ctx);
  if (ctx->dWfError) (void)hipHostFree(ctx->dWfError);
  if (ctx->evStart) (void)hipEventDestroy(ctx->evStart);
  if (ctx->evStop) (void)hipEventDestroy(ctx->evStop);
  delete ctx;  // the device buffers free themselves, on the device set above
  return 0;
}

const char* srtLastError(const SrtContext* ctx) { return ctx ? ctx->error.c_str() : "no context"; }

int srtSetCamera(SrtContext* ctx, const SrtCamera* c) {
  if (!ctx || !c) return 1;
  DevCamera& d = ctx->cam;
  memcpy(d.origin, c->origin, 12); memcpy(d.lleft, c->lleft, 12); memcpy(d.horizontal, c->horizontal, 12);
  memcpy(d.vertical, c->vertical, 12); memcpy(d.hor, c->hor, 12); memcpy(d.vert, c->vert, 12);
  d.lensRadius = c->lensRadius;
  d.time0 = c->time0;
  d.time1 = c->time1;
  ctx->camFull = *c;
  ctx->haveCamera = true;
  return 0;
}

int srtUploadScene(SrtContext* ctx, const SrtSceneDesc* d) { SRT_GUARDED(ctx, srtUploadSceneImpl(ctx, d)); }
int srtBuildBvh(const SrtSceneDesc* d, int32_t item, SrtBvhNode* out, int32_t capacity, int32_t* count, int32_t* stackDepth) { SRT_GUARDED(nullptr, srtBuildBvhImpl(d, item, out, capacity, count, stackDepth)); }
int srtGetBvh(SrtContext* ctx, int32_t item, SrtBvhNode* nodes, int32_t capacity, int32_t* count) { SRT_GUARDED(ctx, srtGetBvhImpl(ctx, item, nodes, capacity, count)); }
int srtGetBvhDepth(SrtContext* ctx, int32_t* depth) {
  if (!ctx || !depth) return 1;
  *depth = ctx->upload.bvhDepth;
  return 0;
}

int srtLastKernelMs(SrtContext* ctx, float* ms) {
  if (!ctx || !ms) return 1;
  if (!ctx->timed) return fail(ctx, "no render has been launched");
  HIP_OK(ctx, hipEventSynchronize(ctx->evStop));
  HIP_OK(ctx, hipEventElapsedTime(ms, ctx->evStart, ctx->evStop));
  return wfCheck(ctx);
}

int srtGetStats(SrtContext* ctx, SrtStats* out) {
  if (!ctx || !out) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, hipDeviceSynchronize());
  unsigned long long v[18];
  HIP_OK(ctx, hipMemcpy(v, ctx->dStats.get(), sizeof v, hipMemcpyDeviceToHost));
  out->samples = v[0]; out->rays = v[1]; out->nodeVisits = v[2]; out->boxPasses = v[3];
  out->triTests = v[4]; out->sphereTests = v[5]; out->shadedTriHits = v[6]; out->texelFetches = v[7];
  out->cyclesNode = v[8]; out->cyclesPrim = v[9]; out->cyclesShade = v[10]; out->cyclesTotal = v[11];
  out->stepsNode = v[12]; out->stepsPrim = v[13]; out->stepsShade = v[14];
  out->lanesNode = v[15]; out->lanesPrim = v[16]; out->lanesShade = v[17];
  return 0;
}

int srtDeviceInfo(SrtContext* ctx, char* name, int32_t nameCap, int32_t* numCUs, int32_t* clockMHz) {
  if (!ctx) return 1;
  if (name && nameCap > 0) {
    snprintf(name, nameCap, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
  }
  if (numCUs) *numCUs = ctx->prop.multiProcessorCount;
  if (clockMHz) *clockMHz = ctx->prop.clockRate / 1000;
  return 0;
}

/* include/srt_hip_test.h: the most recent render-kernel launch */
int srtGetLaunchInfo(SrtContext* ctx, int32_t* out4) {
  if (!ctx || !out4) return 1;
  out4[0] = ctx->lastPlan.form;
  out4[1] = ctx->lastGrid;
  out4[2] = ctx->lastPlan.block;
  out4[3] = (int32_t)ctx->lastPlan.lds;
  return 0;
}
int srtGetWfProfile(SrtContext* ctx, uint64_t* out46) {
  if (!ctx || !out46) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, hipDeviceSynchronize());
  HIP_OK(ctx, hipMemcpy(out46, ctx->dStats.get<unsigned long long>() + 32, 46 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return 0;
}

// Host-only test hooks for srt_thread.h (no device needed): nodes8 = numNodes x 8 floats, the flattened records.
int srtTestThreadLinks16(const float* nodes8, int32_t numNodes, const int32_t* world, int32_t numWorld, int32_t numTriangles, int32_t numSpheres,
                         int32_t* outLinks) {
  if (!nodes8 || !world || !outLinks || numNodes < 0 || numWorld < 0) return -1;
  std::vector<float4> nodes(2 * (size_t)numNodes);
  if (numNodes) memcpy(nodes.data(), nodes8, nodes.size() * sizeof(float4));
  std::vector<int32_t> links;
  srtThreadLinks16(nodes, std::vector<int32_t>(world, world + numWorld), numTriangles, numSpheres, links);
  if (links.empty()) return 0;
  memcpy(outLinks, links.data(), links.size() * sizeof(int32_t));
  return 1;
}

int srtTestHybridRecords(const float* nodes8, int32_t numNodes, const int32_t* world, int32_t numWorld, int32_t numTriangles, int32_t numSpheres,
                         int32_t cap, float* outNodes8, int32_t* outWorld, int32_t* outSecond) {
  if (!nodes8 || !world || !outNodes8 || !outWorld || !outSecond || numNodes < 0 || numWorld < 0 || cap < 0) return -1;
  std::vector<float4> nodes(2 * (size_t)numNodes), wf;
  if (numNodes) memcpy(nodes.data(), nodes8, nodes.size() * sizeof(float4));
  std::vector<int32_t> w, second;
  const int32_t resident = srtHybridRecords(nodes, std::vector<int32_t>(world, world + numWorld), numTriangles, numSpheres, (size_t)cap, wf, w, second);
  if (resident <= 0) return 0;
  memcpy(outNodes8, wf.data(), wf.size() * sizeof(float4));
  memcpy(outWorld, w.data(), w.size() * sizeof(int32_t));
  memcpy(outSecond, second.data(), second.size() * sizeof(int32_t));
  return resident;
}

/* include/srt_hip_test.h: host-only hook for srt_regroup.h, and the uploaded scene's regrouped array as it lies on the device */
int srtTestRegroup(const float* nodes8, int32_t numNodes, const int32_t* world, int32_t numWorld, float* outNodes8) {
  if (!nodes8 || !world || !outNodes8 || numNodes < 0 || numWorld < 0) return -1;
  std::vector<float4> nodes(2 * (size_t)numNodes), out;
  if (numNodes) memcpy(nodes.data(), nodes8, nodes.size() * sizeof(float4));
  if (!srtRegroupNodes(nodes, std::vector<int32_t>(world, world + numWorld), out)) return 0;
  if (numNodes) memcpy(outNodes8, out.data(), out.size() * sizeof(float4));
  return 1;
}
int srtTestGetRegroup(SrtContext* ctx, float* outNodes8, int32_t* outLinks, int32_t capacity, int32_t* count) {
  if (!ctx || !count) return 1;
  if (!ctx->upload.haveScene) return fail(ctx, "srtTestGetRegroup: no scene uploaded");
  const DevScene& s = ctx->upload.scene;
  *count = s.nodesRg ? s.numNodes : 0;
  if (!s.nodesRg || (!outNodes8 && !outLinks)) return 0;
  if (capacity < s.numNodes) return fail(ctx, "srtTestGetRegroup: capacity %d < %d", capacity, s.numNodes);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, hipDeviceSynchronize());
  if (outNodes8) HIP_OK(ctx, hipMemcpy(outNodes8, s.nodesRg, (size_t)s.numNodes * 32, hipMemcpyDeviceToHost));
  if (outLinks) HIP_OK(ctx, hipMemcpy(outLinks, s.nodeThreadRg, (size_t)s.numNodes * sizeof(int32_t), hipMemcpyDeviceToHost));
  return 0;
}

/* include/srt_hip_test.h: host-only hook for srt_regroup.h srtRegroupWalk, and the uploaded scene's walk sequence as it lies on the device */
int srtTestRegroupWalk(const float* nodes8, int32_t numNodes, const int32_t* world, int32_t numWorld, uint8_t* outKeep, int32_t* outSrc,
                       int32_t* outLinks, int32_t* outEntry, int32_t* count) {
  if (!nodes8 || !world || !outKeep || !outSrc || !outLinks || !outEntry || !count || numNodes < 0 || numWorld < 0) return -1;
  std::vector<float4> nodes(2 * (size_t)numNodes);
  if (numNodes) memcpy(nodes.data(), nodes8, nodes.size() * sizeof(float4));
  SrtRegroupWalk walk;
  *count = 0;
  if (!srtRegroupWalk(nodes, std::vector<int32_t>(world, world + numWorld), walk)) return 0;
  *count = (int32_t)walk.src.size();
  if (numNodes) memcpy(outKeep, walk.keep.data(), walk.keep.size());
  if (*count) memcpy(outSrc, walk.src.data(), walk.src.size() * sizeof(int32_t));
  if (*count) memcpy(outLinks, walk.links.data(), walk.links.size() * sizeof(int32_t));
  if (numWorld) memcpy(outEntry, walk.entry.data(), walk.entry.size() * sizeof(int32_t));
  return 1;
}
/* include/srt_hip_test.h: host-only hook for SrtRegroupWalk::head over an array whose primitives are ~(index into kinds) */
int srtTestWfHead(const float* nodes8, int32_t numNodes, const int32_t* world, int32_t numWorld, const uint8_t* kinds, int32_t numKinds,
                  int32_t* outHead) {
  if (!nodes8 || !world || !kinds || !outHead || numNodes < 0 || numWorld < 0 || numKinds < 0) return -1;
  std::vector<float4> nodes(2 * (size_t)numNodes);
  if (numNodes) memcpy(nodes.data(), nodes8, nodes.size() * sizeof(float4));
  return srtRegroupHeadOfKinds(nodes, std::vector<int32_t>(world, world + numWorld), kinds, numKinds, *outHead) ? 1 : 0;
}
int srtTestGetRegroupWalk(SrtContext* ctx, uint8_t* outKeep, int32_t* outSrc, int32_t* outLinks, int32_t* outEntry, int32_t capacity, int32_t* count) {
  if (!ctx || !count) return 1;
  if (!ctx->upload.haveScene) return fail(ctx, "srtTestGetRegroupWalk: no scene uploaded");
  const DevScene& s = ctx->upload.scene;
  *count = s.walkSeq ? s.numWalk : 0;
  if (!s.walkSeq || (!outKeep && !outSrc && !outLinks && !outEntry)) return 0;
  if (capacity < s.numNodes) return fail(ctx, "srtTestGetRegroupWalk: capacity %d < %d", capacity, s.numNodes);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, hipDeviceSynchronize());
  std::vector<int32_t> seq(3 * (size_t)s.numWalk + (size_t)s.numWorld);
  HIP_OK(ctx, hipMemcpy(seq.data(), s.walkSeq, seq.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (outKeep) memset(outKeep, 0, (size_t)s.numNodes);
  for (int32_t j = 0; j < s.numWalk; ++j) {
    const int32_t src = seq[3 * (size_t)j];
    if (src < 0 || src >= s.numNodes) return fail(ctx, "srtTestGetRegroupWalk: record %d has source %d", j, src);
    if (outKeep) outKeep[src] = 1;
    if (outSrc) outSrc[j] = src;
    if (outLinks) outLinks[2 * (size_t)j] = seq[3 * (size_t)j + 1], outLinks[2 * (size_t)j + 1] = seq[3 * (size_t)j + 2];
  }
  if (outEntry) memcpy(outEntry, seq.data() + 3 * (size_t)s.numWalk, (size_t)s.numWorld * sizeof(int32_t));
  return 0;
}

/* include/srt_hip_test.h: world item `item`'s slice of DevScene::nodeAxis and DevScene::nodes2, read back as they are */
int srtTestGetTreeAux(SrtContext* ctx, int32_t item, uint8_t* outAxis, float* outPairs16, int32_t capacity, int32_t* count) {
  if (!ctx || !count) return 1;
  if (!ctx->upload.haveScene) return fail(ctx, "srtTestGetTreeAux: no scene uploaded");
  if (item < 0 || item >= (int32_t)ctx->upload.itemNodes.size()) return fail(ctx, "srtTestGetTreeAux: item %d out of range", item);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  int32_t ref = 0;
  HIP_OK(ctx, hipMemcpy(&ref, ctx->upload.scene.world + item, sizeof ref, hipMemcpyDeviceToHost));
  if (ref < 0) return fail(ctx, "srtTestGetTreeAux: item %d is not a tree", item);
  const auto dt = std::find_if(ctx->upload.deviceBuilds.begin(), ctx->upload.deviceBuilds.end(), [&](const DeviceBuild& b) { return b.item == item; });
  const int32_t base = SRT_NODE_INDEX(ref), n = dt != ctx->upload.deviceBuilds.end() ? dt->count : (int32_t)ctx->upload.itemNodes[item].size();
  if (base + n > ctx->upload.scene.numNodes) return fail(ctx, "srtTestGetTreeAux: item %d lies outside the node array", item);
  *count = n;
  if (!outAxis && !outPairs16) return 0;
  if (capacity < n) return fail(ctx, "srtTestGetTreeAux: capacity %d < %d", capacity, n);
  if (outAxis) HIP_OK(ctx, hipMemcpy(outAxis, ctx->upload.scene.nodeAxis + base, (size_t)n, hipMemcpyDeviceToHost));
  if (outPairs16) HIP_OK(ctx, hipMemcpy(outPairs16, ctx->upload.scene.nodes2 + 4 * (size_t)base, (size_t)n * 64, hipMemcpyDeviceToHost));
  return 0;
}

/* include/srt_hip_test.h: the certified slab test's scene conditions */
int srtTestGetSlabScene(SrtContext* ctx, int32_t* out2) {
  if (!ctx || !out2) return 1;
  if (!ctx->upload.haveScene) return fail(ctx, "srtTestGetSlabScene: no scene uploaded");
  out2[0] = ctx->upload.scene.fastDivScene;
  out2[1] = ctx->upload.scene.boxOrderedScene;
  return 0;
}

/* include/srt_hip_test.h: the refined reciprocal over a range of bit patterns (csrc/srt_slabtest.hip).  Needs no scene. */
int srtTestRefinedRcp(SrtContext* ctx, int64_t firstBits, int64_t count, uint64_t* out2) {
  if (!ctx) return 1;
  if (!out2) return fail(ctx, "srtTestRefinedRcp: null output");
  if (firstBits < 0 || firstBits > 0xffffffffll || count < 1 || count > (1ll << 32) || firstBits + count - 1 > 0xffffffffll)
    return fail(ctx, "srtTestRefinedRcp: patterns %lld .. + %lld are not 32-bit patterns", (long long)firstBits, (long long)count);
  const int64_t last = firstBits + count - 1;
  // one sign, and the largest magnitude still finite: neither an infinity nor a NaN in the range
  if ((firstBits >> 31) != (last >> 31) || (last & 0x7fffffffll) > 0x7f7fffffll)
    return fail(ctx, "srtTestRefinedRcp: patterns %lld .. %lld leave the finite floats of one sign", (long long)firstBits, (long long)last);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  DeviceBuffer dPartial;
  std::vector<unsigned long long> partial(2 * SRT_SLABTEST_RCP_WAVES);
  HIP_OK(ctx, dPartial.reserve(partial.size() * sizeof(unsigned long long)));
  const int e = srt_launch_slabtest_rcp((uint32_t)firstBits, count, dPartial.get<unsigned long long>(), nullptr);
  if (e) return fail(ctx, "srtTestRefinedRcp: launch failed: %s", hipGetErrorString((hipError_t)e));
  HIP_OK(ctx, hipDeviceSynchronize());
  HIP_OK(ctx, hipMemcpy(partial.data(), dPartial.get(), partial.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  double best = -1.0;
  uint64_t bestBits = 0;
  for (int w = 0; w < SRT_SLABTEST_RCP_WAVES; ++w) {
    double err;
    memcpy(&err, &partial[2 * w], sizeof err);
    if (err > best || (err == best && err >= 0.0 && partial[2 * w + 1] < bestBits)) {
      best = err;
      bestBits = partial[2 * w + 1];
    }
  }
  if (best < 0.0) return fail(ctx, "srtTestRefinedRcp: no wave reported");
  memcpy(&out2[0], &best, sizeof best);
  out2[1] = bestBits;
  return 0;
}

/* include/srt_hip_test.h: caller-made (box, ray) cases through the device compile of the certified slab test */
int srtTestSlabVisit(SrtContext* ctx, const float* hCases, int32_t n, float tMin, int32_t certifiedScene, float* hOut) {
  if (!ctx) return 1;
  if (!hCases) return fail(ctx, "srtTestSlabVisit: null cases");
  if (!hOut) return fail(ctx, "srtTestSlabVisit: null output");
  if (n < 1 || n > (1 << 20)) return fail(ctx, "srtTestSlabVisit: n = %d is not in [1, 2^20]", n);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  const size_t inBytes = (size_t)n * 13 * sizeof(float), outBytes = (size_t)n * 8 * sizeof(float);
  DeviceBuffer dIn, dOut;
  HIP_OK(ctx, dIn.reserve(inBytes));
  HIP_OK(ctx, dOut.reserve(outBytes));
  HIP_OK(ctx, hipMemcpy(dIn.get(), hCases, inBytes, hipMemcpyHostToDevice));
  const int e = srt_launch_slabtest_visit(dIn.get<const float>(), n, tMin, certifiedScene, dOut.get<float>(), nullptr);
  if (e) return fail(ctx, "srtTestSlabVisit: launch failed: %s", hipGetErrorString((hipError_t)e));
  HIP_OK(ctx, hipDeviceSynchronize());
  HIP_OK(ctx, hipMemcpy(hOut, dOut.get(), outBytes, hipMemcpyDeviceToHost));
  return 0;
}

/* include/srt_hip_test.h: the certified triangle test's read-outs */
int srtTestGetTriUndecided(SrtContext* ctx, uint64_t* out) {
  if (!ctx || !out) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, hipDeviceSynchronize());
  HIP_OK(ctx, hipMemcpy(out, ctx->dStats.get<unsigned long long>() + SRT_STATS_TRI_UNDECIDED, sizeof(uint64_t), hipMemcpyDeviceToHost));
  return 0;
}
int srtTestGetTriFast(SrtContext* ctx, float* out16, int32_t capacity, int32_t* count) {
  if (!ctx || !count) return 1;
  if (!ctx->upload.haveScene) return fail(ctx, "srtTestGetTriFast: no scene uploaded");
  const int32_t n = ctx->upload.scene.numTris;
  *count = n;
  if (!out16) return 0;
  if (capacity < n) return fail(ctx, "srtTestGetTriFast: capacity %d < %d", capacity, n);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, hipDeviceSynchronize());
  const std::vector<int32_t>& dev = ctx->upload.hostTriDevIndex;  // scene index -> device index, empty = identity
  std::vector<float4> raw((size_t)n * SRT_TRI_FAST_SLOTS);
  if (n) HIP_OK(ctx, hipMemcpy(raw.data(), ctx->upload.scene.triFast, raw.size() * sizeof(float4), hipMemcpyDeviceToHost));
  for (int32_t i = 0; i < n; ++i)
    memcpy(out16 + 16 * (size_t)i, &raw[SRT_TRI_FAST_SLOTS * (size_t)(dev.empty() ? i : dev[i])], 64);
  return 0;
}
/* host-only: the triFast record of one triangle as srtUploadScene makes it */
int srtTestTriFastRecord(const float* p9, float* out16) {
  if (!p9 || !out16) return 1;
  const float uv[6] = {0, 0, 0, 0, 0, 0};
  float4 test[3], shade[4], fast[SRT_TRI_FAST_SLOTS];
  triangleRecords(p9, uv, 0.0f, test, shade, fast);
  memcpy(out16, fast, 64);
  return 0;
}

int srtGetShadeProfile(SrtContext* ctx, uint64_t* out10) {
  if (!ctx || !out10) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, hipDeviceSynchronize());
  HIP_OK(ctx, hipMemcpy(out10, ctx->dStats.get<unsigned long long>() + 18, 10 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return 0;
}

/* include/srt_hip_test.h: per-context diagnostic tunables */
int srtSetTunable(SrtContext* ctx, const char* name, int32_t value) {
  if (!ctx || !name) return 1;
  for (const TunableName& t : kTunables)
    if (!strcmp(t.name, name)) {
      ctx->tun.*(t.field) = value;
      ctx->upload.scene.triWMax = triWMaxFor(ctx);  // (the uploaded scene follows "tri_cert" at once)
      return 0;
    }
  return fail(ctx, "srtSetTunable: unknown tunable '%s'", name);
}
int srtGetTunable(SrtContext* ctx, const char* name, int32_t* value) {
  if (!ctx || !name || !value) return 1;
  for (const TunableName& t : kTunables)
    if (!strcmp(t.name, name)) {
      *value = ctx->tun.*(t.field);
      return 0;
    }
  return fail(ctx, "srtGetTunable: unknown tunable '%s'", name);
}

}  // extern "C"
