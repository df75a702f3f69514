// srt_api.cpp -- host side of the C ABI (include/srt_hip.h): context (srt_context.h), device memory, the upload of a
// flattened scene (srt_scene.cpp) and the device BVH builds, launches and timing.  The entries that render a whole frame
// into host buffers compose these launches in srt_frames.cpp.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "srt_context.h"
#include "srt_thread.h"

extern "C" {
int srt_launch_finalize(const SrtFixedAccum* fix, float4* out, int n, int samples, hipStream_t stream);
int srt_launch_sum_chunks(const float4* buf, float4* out, int n, int chunks, float limit, hipStream_t stream);
int srt_launch_resolve(const ResolveArgs* a, hipStream_t stream);
int srt_launch_trace(const TraceArgs* a, int traversal, int grid, size_t ldsBytes, hipStream_t stream);
int srt_lbvh_build(const DevScene* sc, const int32_t* dRefs, int n, float time0, float time1, float4* outNodes,
                   uint8_t* outAxis, int base, int* depthOut);
int srt_ploc_build(const DevScene* sc, const int32_t* dRefs, int n, float time0, float time1, float4* outNodes,
                   uint8_t* outAxis, int base, int radius, int* depthOut);
int srt_pair_nodes(const DevScene* sc, float time0, float time1, float4* out);
int srt_pair_nodes_async(const DevScene* sc, float time0, float time1, float4* out, hipStream_t stream);
int srt_launch_scatter(const DevScene* sc, const SrtRay* rays, const SrtHit* hits, float* out, uint64_t seed, int n,
                       hipStream_t stream);
int srt_features_plan(int closest, int ldsTree, size_t lds, int* block, int* perCU);
int srt_launch_features(const FeatureArgs* a, int closest, int ldsTree, int grid, size_t lds, hipStream_t stream);
int srt_features_list_plan(int closest, int ldsTree, int accumulate, size_t lds, int* block, int* perCU);
int srt_launch_features_list(const FeatureListArgs* a, int closest, int ldsTree, int accumulate, int grid, size_t lds,
                             hipStream_t stream);
int srt_launch_denoise(const DenoiseArgs* a, int iterations, int ldsMaxStep, hipStream_t stream);
int srt_launch_adaptive_update(const uint32_t* list, int count, const float4* beautyTiles, const float4* momentTiles,
                               float4* accum, float4* moments, int32_t* flags, int width, int height, double limit,
                               bool accumulate, bool decide, hipStream_t stream);
int srt_launch_adaptive_compact(const uint32_t* list, const int32_t* flags, int count, uint32_t* out, int32_t* counts,
                                int width, int height, hipStream_t stream);
int srt_launch_adaptive_resolve(const float4* accum, uint8_t* rgba, int n, hipStream_t stream);
int srt_launch_temporal(const TemporalArgs* a, hipStream_t stream);
int srt_launch_temporal_reproject(const TemporalArgs* a, hipStream_t stream);
int srt_launch_temporal_adaptive_update(const uint32_t* list, int count, const float4* beautyTiles, const float4* momentTiles,
                                        float4* accum, float4* moments, const float4* reprojected, const float4* albedo,
                                        int32_t* flags, int width, int height, double limit, bool accumulate,
                                        hipStream_t stream);
}

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
  ctx->sceneBuffers.push_back(std::move(b));
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
    // srtDenoise: a-trous levels of step <= this stage their (16 + 4 step)^2 window in LDS, larger steps read through the
    // caches (srt_denoise.hip; 8 at most, 0 = never) -- profiles/r05/denoise_bench.json
    {"denoise_lds_step", "SRT_DENOISE_LDS_STEP", &Tunables::denoiseLdsStep, 4},
};

// The fields a launch over the image shares (RenderArgs, FeatureArgs): the scene, the camera, the image, its samples and
// the tile split; everything else zero.
template <typename Args>
void setImageArgs(Args& a, const SrtContext* ctx, const SrtRenderParams* p) {
  memset(&a, 0, sizeof a);
  a.scene = ctx->scene;
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

size_t ldsBytesFor(const SrtContext* ctx, int maxBounce, int stackDepth) {
  // per-thread stacks plus one word of queue state per wave (srt_render_kernel)
  return (size_t)(stackDepth + 2 + 3 * maxBounce + 3) * SRT_BLOCK * sizeof(int32_t) + 4 * sizeof(int32_t);
}

}  // namespace

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

static int srtUploadSceneImpl(SrtContext* ctx, const SrtSceneDesc* d) {
  if (!ctx || !d) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  ctx->sceneBuffers.clear();
  ctx->haveScene = false;
  ctx->temporalValid = false;  // a history belongs to its scene
  ctx->itemNodes.clear();
  ctx->deviceBuilds.clear();
  ctx->bvhDepth = 0;
  ctx->trees.clear();
  ctx->geometryDirty = false;
  ctx->refitTables = false;
  ctx->triDevIndex = DeviceBuffer();
  ctx->wfIndex = DeviceBuffer();
  ctx->refitUp = DeviceBuffer();
  ctx->refitArrived = DeviceBuffer();
  std::string err = validateScene(d);
  HostScene h;
  if (err.empty()) err = flattenScene(d, SceneOptions{ctx->tun.wfHybrid, ctx->tun.wfResidentMax, ctx->tun.fastDiv}, h);
  if (!err.empty()) return fail(ctx, "%s", err.c_str());

  DevScene& s = ctx->scene;
  memset(&s, 0, sizeof s);
  if (!h.nodeThread.empty() && uploadVec(ctx, h.nodeThread, &s.nodeThread)) return 1;
  if (!h.nodesWf.empty() && (uploadVec(ctx, h.nodesWf, &s.nodesWf) || uploadVec(ctx, h.worldWf, &s.worldWf) || uploadVec(ctx, h.primSecond, &s.primSecond))) return 1;
  if (uploadVec(ctx, h.primClass, &s.primClass, 16) || uploadVec(ctx, h.nodeAxis, &s.nodeAxis, 64) || uploadVec(ctx, h.nodes, &s.nodes) ||
      uploadVec(ctx, h.triTest, &s.triTest) || uploadVec(ctx, h.triShade, &s.triShade) || uploadVec(ctx, h.spheres, &s.spheres) ||
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
  ctx->bvhDepth = h.bvhDepth;
  // device-built trees (srt_lbvh.hip) into the node slots the flattening reserved
  for (DeviceBuild& b : h.deviceBuilds) {
    DeviceBuffer refs;
    HIP_OK(ctx, refs.reserve(b.refs.size() * sizeof(int32_t)));
    int rc = (int)hipMemcpy(refs.get(), b.refs.data(), b.refs.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    int depth = 0;
    if (rc == hipSuccess)
      rc = b.builder == SRT_BUILDER_PLOC
               ? srt_ploc_build(&s, refs.get<int32_t>(), (int)b.refs.size(), b.time0, b.time1, const_cast<float4*>(s.nodes),
                                const_cast<uint8_t*>(s.nodeAxis), b.base, ctx->tun.plocRadius, &depth)
               : srt_lbvh_build(&s, refs.get<int32_t>(), (int)b.refs.size(), b.time0, b.time1, const_cast<float4*>(s.nodes),
                                const_cast<uint8_t*>(s.nodeAxis), b.base, &depth);
    if (rc) return fail(ctx, "device BVH build of world item %d failed: %s", b.item, hipGetErrorString((hipError_t)rc));
    s.stackDepth = std::max(s.stackDepth, depth);
    ctx->bvhDepth = std::max(ctx->bvhDepth, depth);
    b.refs = std::vector<int32_t>();
  }
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
  ctx->sceneBuffers.push_back(std::move(nodes2));
  const int rc = srt_pair_nodes(&s, t0, t1, const_cast<float4*>(s.nodes2));
  if (rc) return fail(ctx, "pairing the node records failed: %s", hipGetErrorString((hipError_t)rc));
  ctx->itemNodes = std::move(h.itemNodes);
  ctx->deviceBuilds = std::move(h.deviceBuilds);
  // what an update and a refit need of this upload (srt_refit_host.cpp)
  for (const HostTree& t : h.hostTrees) ctx->trees.push_back(SrtContext::Tree{t.item, t.base, t.count, t.time0, t.time1, false});
  for (const DeviceBuild& b : ctx->deviceBuilds) ctx->trees.push_back(SrtContext::Tree{b.item, b.base, b.count, b.time0, b.time1, true});
  ctx->hostTriDevIndex = std::move(h.triDevIndex);
  ctx->hostWfIndex = std::move(h.wfIndex);
  ctx->itemBoxesStale.assign(ctx->itemNodes.size(), 0);
  ctx->pairTime0 = t0;
  ctx->pairTime1 = t1;
  ctx->fastDivOption = ctx->tun.fastDiv;
  ctx->hostTriPrimId = std::move(h.triPrimId);
  ctx->hostSphPrimId = std::move(h.sphPrimId);
  ctx->haveScene = true;
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

static int srtGetBvhImpl(SrtContext* ctx, int32_t item, SrtBvhNode* nodes, int32_t capacity, int32_t* count) {
  if (!ctx || !count) return 1;
  if (item < 0 || item >= (int32_t)ctx->itemNodes.size()) return fail(ctx, "srtGetBvh: item %d out of range", item);
  const auto dt = std::find_if(ctx->deviceBuilds.begin(), ctx->deviceBuilds.end(), [&](const DeviceBuild& b) { return b.item == item; });
  if (ctx->itemBoxesStale[item]) {
    // srtRefitScene has moved the boxes since this copy was made: a device-built tree is read back again (below), a
    // host-built one gets the device's boxes (its children stay in the host convention)
    ctx->itemBoxesStale[item] = 0;
    auto& out = ctx->itemNodes[item];
    const auto tr = std::find_if(ctx->trees.begin(), ctx->trees.end(), [&](const SrtContext::Tree& t) { return t.item == item; });
    if (dt != ctx->deviceBuilds.end()) {
      out.clear();
    } else if (tr != ctx->trees.end() && !out.empty()) {
      std::vector<float4> raw((size_t)tr->count * 2);
      HIP_OK(ctx, hipMemcpy(raw.data(), ctx->scene.nodes + 2 * (size_t)tr->base, raw.size() * sizeof(float4), hipMemcpyDeviceToHost));
      for (int i = 0; i < tr->count; ++i) {
        out[i].bmin[0] = raw[2 * i].x; out[i].bmin[1] = raw[2 * i].y; out[i].bmin[2] = raw[2 * i].z;
        out[i].bmax[0] = raw[2 * i + 1].x; out[i].bmax[1] = raw[2 * i + 1].y; out[i].bmax[2] = raw[2 * i + 1].z;
      }
    }
  }
  if (dt != ctx->deviceBuilds.end() && ctx->itemNodes[item].empty()) {
    // device-built tree: read it back once, converting child refs to the host convention
    std::vector<float4> raw((size_t)dt->count * 2);
    HIP_OK(ctx, hipMemcpy(raw.data(), ctx->scene.nodes + 2 * (size_t)dt->base, raw.size() * sizeof(float4), hipMemcpyDeviceToHost));
    auto& out = ctx->itemNodes[item];
    out.resize(dt->count);
    auto conv = [&](float bits) -> int32_t {
      int32_t r;
      memcpy(&r, &bits, 4);
      if (r >= 0) return SRT_NODE_INDEX(r) - dt->base;
      int32_t pr = ~r;
      return ~((pr & 1) ? ctx->hostSphPrimId[pr >> 1] : ctx->hostTriPrimId[pr >> 1]);
    };
    for (int i = 0; i < dt->count; ++i) {
      out[i].bmin[0] = raw[2 * i].x; out[i].bmin[1] = raw[2 * i].y; out[i].bmin[2] = raw[2 * i].z;
      out[i].bmax[0] = raw[2 * i + 1].x; out[i].bmax[1] = raw[2 * i + 1].y; out[i].bmax[2] = raw[2 * i + 1].z;
      out[i].left = conv(raw[2 * i].w);
      out[i].right = conv(raw[2 * i + 1].w);
    }
  }
  const auto& v = ctx->itemNodes[item];
  *count = (int32_t)v.size();
  if (nodes) {
    if (capacity < (int32_t)v.size()) return fail(ctx, "srtGetBvh: capacity %d < %zu", capacity, v.size());
    memcpy(nodes, v.data(), v.size() * sizeof(SrtBvhNode));
  }
  return 0;
}

int srtGetBvhDepth(SrtContext* ctx, int32_t* depth) {
  if (!ctx || !depth) return 1;
  *depth = ctx->bvhDepth;
  return 0;
}

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

extern "C++" int checkSceneReady(SrtContext* ctx, const char* what) {
  if (!ctx->haveScene) return fail(ctx, "%s: no scene uploaded", what);
  if (ctx->geometryDirty) return fail(ctx, "%s: geometry was updated; call srtRefitScene before anything traverses the scene", what);
  return 0;
}

extern "C++" int checkParams(SrtContext* ctx, const SrtRenderParams* p) {
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

// The render launch for these parameters: the kernel form and the instance of it, workgroup and LDS size, the path-pool
// kernel's rings.  Every choice of kernel is made here; srtRenderTilesImpl allocates and launches what it says.
// moments: srtRenderTilesMoments -- the same form, grid, block and LDS, its MOMENTS instance (never counting or profiling).
// listTiles >= 0: a launch over a tile list of that length (srtRenderAdaptive) instead of the rank's share of the image.
static RenderPlan renderPlan(const SrtContext* ctx, const SrtRenderParams* p, bool moments = false, int32_t listTiles = -1) {
  const DevScene& sc = ctx->scene;
  const Tunables& tun = ctx->tun;
  RenderPlan plan{};
  const bool faithful = p->traversal == SRT_TRAVERSE_FAITHFUL;
  plan.closest = p->traversal == SRT_TRAVERSE_CLOSEST;
  plan.count = p->countStats != 0;
  plan.moments = moments;
  // FAITHFUL on a scene whose whole node array fits into a CU's LDS: the LDS-resident-tree kernel (srt_render_kernel
  // LDSTREE), one workgroup of 1024 threads per CU, walking the threaded copy of the tree (no per-lane stack).
  const size_t ldsTreeBytes = (size_t)sc.numNodes * 32 + 16 * sizeof(int32_t);  // threaded tree: no stacks
  // (Even trees of a few dozen nodes gain: their frames are shading-bound, and the 128-register kernel keeps a hit's
  // texel loads in flight together where the 96-register one spills, profiles/r02/lds_tree.txt.)
  const bool ldsTree = faithful && tun.ldsTree > 0 && sc.numNodes >= tun.ldsTree && ldsTreeBytes <= 160 * 1024 &&
                       sc.nodeThread != nullptr;  // thread links exist: host-built trees, 15-bit references (srtUploadScene)
  // ... and when the attenuation stacks fit behind them as well they stay in LDS (form 2): +2 to +5 % on the small
  // BASELINE scenes; the headline scene's tree leaves no room (form 1: they live in global memory)
  const size_t attBytes = (size_t)(3 * p->maxBounce + 3) * SRT_BLOCK_TREE * sizeof(float);
  // The path-pool kernel (srt_wavefront.hip) serves what the LDS-resident tree serves, when its rings fit behind the
  // tree: one 1024-thread workgroup per CU, wfPool contexts each.  A counting launch runs the counting instance of the
  // kernel the same launch without counting runs: the counters belong to the kernel under test.
  // LDS behind the tree: 64 control words, six rings of 16-bit slots, and per context the (t, primitive) its walk ended at:
  // 18 bytes per context.  Ring capacity = pool size = the largest of 1024, 1536, 2048, 3072, 4096 that fits and does not
  // exceed the tunable (the headline scene's 129 KB tree leaves room for 1536).
  // Hybrid form: the tree's top in LDS, the rest read from global memory (scene.nodesWf, built at upload when the tree does
  // not fit or the tunable wf_resident_max asks for it).
  const bool hybrid = faithful && sc.nodesWf != nullptr && tun.wavefront > 0 && sc.primClass != nullptr;
  const size_t wfFixed = (size_t)(hybrid ? sc.wfResident : sc.numNodes) * 32 + 64 * sizeof(int32_t);
  const size_t wfPerContext = hybrid ? 20 : 18;  // six ring slots of 16 bits, t, the primitive (16 bits; 32 in the hybrid form)
  // ring counters are 32-bit and a 3 * 2^j ring cannot take their wrap-around: such rings only while a workgroup's
  // enqueues stay far below 2^32 (about three per sample)
  const int numLocalTiles = listTiles >= 0 ? listTiles : srtNumLocalTiles(p->imageWidth, p->imageHeight, p->tileStride);
  const double enqueuesPerGroup = 4.0 * (double)numLocalTiles * SRT_TILE_PIXELS * (double)p->spp / std::max(1, ctx->prop.multiProcessorCount);
  static const struct { int cap, shift, mul3; } kRings[] = {{4096, 12, 0}, {3072, 10, 1}, {2048, 11, 0}, {1536, 9, 1}, {1024, 10, 0}};
  for (const auto& r : kRings) {
    if (r.cap > std::max(1024, tun.wfPool) || wfFixed + wfPerContext * r.cap > 160 * 1024) continue;
    if (r.mul3 && enqueuesPerGroup > 2.0e9) continue;
    plan.wfRingCap = r.cap;
    plan.wfRingShift = r.shift;
    plan.wfRingMul3 = r.mul3;
    break;
  }
  const bool wavefront = plan.wfRingCap > 0 && (hybrid || (ldsTree && tun.wavefront > 0 && sc.numNodes >= tun.wavefront && sc.primClass != nullptr));
  if (wavefront) {
    plan.form = hybrid ? 4 : 3;
    plan.block = SRT_BLOCK_TREE;
    plan.lds = wfFixed + wfPerContext * plan.wfRingCap;
    plan.profile = !plan.count && !plan.moments && tun.wfProfile > 0;  // a counting or moments launch takes no profile
    // (hybrid form: the single-root instance is worth +12 to +15 % on cache-resident trees and costs 5 % on the HBM-bound
    // soups of 4 M triangles and more, where the shorter visit only crowds the memory system: profiles/r03/hybrid.txt)
    plan.single = !plan.profile && sc.numWorld == 1 && (!hybrid || sc.numNodes <= (1 << 20));
    return plan;
  }
  plan.wfRingCap = plan.wfRingShift = plan.wfRingMul3 = 0;
  plan.form = !ldsTree ? 0 : ldsTreeBytes + attBytes <= 160 * 1024 ? 2 : 1;
  plan.block = ldsTree ? SRT_BLOCK_TREE : SRT_BLOCK;
  plan.lds = plan.form == 2 ? ldsTreeBytes + attBytes : ldsTree ? ldsTreeBytes : ldsBytesFor(ctx, p->maxBounce, sc.stackDepth);
  plan.single = !plan.count && sc.numWorld == 1;  // (the counting instances serve single-root worlds as well)
  return plan;
}

// aov: srtRenderAov's per-pixel records of the ray at bounce aovDepth (counting launches only), else null.
// dMoments: srtRenderTilesMoments's plane (the MOMENTS instance of the planned form), else null.
// dList: a DEVICE table of listTiles tiles (tx | ty << 16) to render instead of the rank's share of the image
// (srtRenderAdaptive; p->tileFirst = 0, p->tileStride = 1): the output holds list position i where it holds local tile i,
// and the queues, the grid and the chunk scratch follow the list's length.  The render kernels see an ordinary launch
// whose tile table is the list.
extern "C++" int srtRenderTilesImpl(SrtContext* ctx, const SrtRenderParams* p, void* dAccumTiles, void* streamPtr, SrtAovRecord* aov,
                                    int32_t aovDepth, void* dMoments, const uint32_t* dList, int32_t listTiles) {
  if (!ctx || !p || !dAccumTiles) return 1;
  if (checkParams(ctx, p)) return 1;
  if (dList && (listTiles < 1 || listTiles > srtNumTiles(p->imageWidth, p->imageHeight) || p->tileStride != 1))
    return fail(ctx, "render: bad tile list of %d tiles", listTiles);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  RenderArgs a;
  setImageArgs(a, ctx, p);
  if (dList) a.numTiles = a.numLocalTiles = listTiles;
  a.maxBounce = p->maxBounce;
  a.sppChunks = p->sppChunks > 0 ? p->sppChunks : srtDefaultSppChunks(p->spp);
  {
    // work queues (srt_render_kernel): units of >= 8 consecutive local tiles, about a dozen units per queue,
    // at most 64 queues.  Measured on the 720p headline frame (ms per launch, 1 rank / one of 8 ranks):
    // 1 queue 1916 / 253, 16 queues x 8 tiles 1818 / 238, 64 x 8: 1767 / 255, 64 x 16: 1744 / -.
    const auto pow2Floor = [](int v) { int r = 1; while (2 * r <= v) r *= 2; return r; };
    int unit = 8;
    const int unitsAt8 = (a.numLocalTiles + 7) / 8;
    if (unitsAt8 >= 2 * 12 * SRT_MAX_QUEUES) unit = 8 * pow2Floor(unitsAt8 / (12 * SRT_MAX_QUEUES));
    a.unitTiles = std::min(1024, std::max(1, ctx->tun.unitTiles > 0 ? ctx->tun.unitTiles : unit));
    const int units = (a.numLocalTiles + a.unitTiles - 1) / a.unitTiles;
    // ... and only while every wave still gets a few dozen groups: with few groups per wave (16 spp on a
    // 10 M-triangle soup: 14 400 groups for 5 120 waves) one counter balances better than stealing does.
    const int64_t groups = (int64_t)a.numLocalTiles * a.sppChunks, waves = (int64_t)ctx->prop.multiProcessorCount * 20;
    const int byUnits = pow2Floor(std::max(1, units / 12));
    const int byGroups = pow2Floor((int)std::max<int64_t>(1, std::min<int64_t>(SRT_MAX_QUEUES, groups / (2 * waves))));
    a.numQueues = std::min(SRT_MAX_QUEUES, std::max(1, ctx->tun.queues > 0 ? ctx->tun.queues : std::min(byUnits, byGroups)));
  }
  {
    const int32_t planned = srtPlanSppChunks(p->imageWidth, p->imageHeight, p->spp, p->sppChunks);
    if (planned < 1) return fail(ctx, "render: sppChunks %d x %d tiles exceeds 2^31 work items", p->sppChunks, a.numTiles);
    a.sppChunks = planned;
  }
  {
    // exact chunk sums cannot wrap: partial sums of 2^26 / (chunk count rounded up to a power of two) or more count as infinite
    int pow2 = 1;
    while (pow2 < a.sppChunks) pow2 *= 2;
    a.fixLimit = 0x1p26f / (float)pow2;
  }
  a.numWork = a.numLocalTiles * a.sppChunks * SRT_TILE_PIXELS;
  a.sppBase = a.spp / a.sppChunks;
  a.sppRem = a.spp % a.sppChunks;
  a.numUnits = (a.numLocalTiles + a.unitTiles - 1) / a.unitTiles;
  a.unitGroups = a.unitTiles * a.sppChunks;
  a.rcpUnitGroups = 1.0f / (float)a.unitGroups;
  a.rcpChunks = 1.0f / (float)a.sppChunks;
  if (!dList && (ctx->tileTableKey[0] != p->imageWidth || ctx->tileTableKey[1] != p->imageHeight || ctx->tileTableKey[2] != a.tileBlock || !ctx->tileTable.get())) {
    // the tile order as a table (once per image size): the kernel's restart step looks a tile up instead of dividing
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
  }
  a.tileXY = dList ? dList : ctx->tileTable.get<const uint32_t>();
  // Scheduler defaults by traversal mode (profiles/r02/scheduler_sweep.txt).  FAITHFUL on cache-resident scenes:
  // node bursts go on while half of their lanes are still at nodes, up to 64 visits, restarts at 24 waiting lanes
  // (+6 % on the headline frame against 6/8, 32, 16).  The closest-hit traversal over the 64-byte records is bound by
  // memory latency on large scenes and wants shorter bursts that give up sooner (10 M triangles: 87.6 against 77.8
  // Msamples/s), and does not care on small ones.
  const bool closestMode = p->traversal == SRT_TRAVERSE_CLOSEST;
  a.shadeMin = ctx->tun.shadeMin >= 0 ? ctx->tun.shadeMin : (closestMode ? 16 : 24);
  a.primMin = ctx->tun.primMin;
  a.hitMin = ctx->tun.hitMin;
  a.fuseMin = ctx->tun.fuseMin;
  a.nodeBurst = std::max(1, ctx->tun.nodeBurst > 0 ? ctx->tun.nodeBurst : (closestMode ? 32 : 64));
  a.primAgainMin = std::max(1, ctx->tun.primAgainMin);
  a.keepEighths = std::min(8, ctx->tun.keepEighths >= 0 ? ctx->tun.keepEighths : (closestMode ? 6 : 4));
  a.queue = ctx->dQueue.get<int32_t>();
  const bool moments = dMoments != nullptr;
  // (a moments launch neither counts nor profiles: its mout / mfix take the places of aov / stats, RenderArgs)
  unsigned long long* const stats = !moments && (p->countStats || ctx->tun.wfProfile > 0) ? ctx->dStats.get<unsigned long long>() : nullptr;
  a.stats = stats;
  a.aov = p->countStats ? aov : nullptr;
  a.aovDepth = aovDepth;
  const size_t tilePixels = (size_t)a.numLocalTiles * SRT_TILE_PIXELS;
  a.out = static_cast<float4*>(dAccumTiles);
  a.fix = nullptr;
  if (moments) a.mout = static_cast<float4*>(dMoments);
  a.chunkStride = 0;
  bool scratchPath = false;
  // a moments launch sums its moments plane exactly as the beauty, on the same path: twice the slots or accumulators,
  // the beauty's first, the moments' behind them
  const size_t planes = moments ? 2 : 1;
  if (a.sppChunks > 1) {
    // Chunk sums are added exactly (srt_kernels.hip "Chunk sums").  Scratch path (a float4 slot per item, summed by
    // srt_sum_chunks_kernel) while this rank's slots fit the budget, else the atomic path (32 B per pixel, 0.4-1 %
    // slower); the two give the same bits, so the choice may differ from rank to rank.
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
  }
  const RenderPlan plan = renderPlan(ctx, p, moments, dList ? listTiles : -1);
  if (plan.lds > 160 * 1024) return fail(ctx, "render: BVH depth %d needs %zu B of LDS per workgroup", ctx->scene.stackDepth, plan.lds);
  const RenderKernel kernel = plan.form >= 3 ? srt_render_wf_kernel_for(&plan) : srt_render_kernel_for(&plan);
  if (plan.lds > 64 * 1024)
    HIP_OK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
  // persistent waves: enough workgroups to fill every CU (the path-pool kernel: one), never more than there is work
  int perCU = 1;
  if (plan.form < 3 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, plan.block, plan.lds) != hipSuccess || perCU < 1)) perCU = 1;
  const int wgItems = SRT_TILE_PIXELS * (plan.block / 64);
  int grid = std::min(ctx->prop.multiProcessorCount * perCU, (a.numWork + wgItems - 1) / wgItems);
  if (grid < 1) grid = 1;
  if (plan.form >= 3) {
    // a workgroup never needs more contexts than it has work items
    const int64_t itemsPerGroup = ((int64_t)a.numWork + grid - 1) / grid;
    const int wfPoolSize = (int)std::max<int64_t>(64, std::min<int64_t>(plan.wfRingCap, itemsPerGroup + 63));
    HIP_OK(ctx, ctx->wfPool.reserve((size_t)grid * wfPoolSize * 128));
    const int hiLevels = std::max(0, p->maxBounce - 4);
    HIP_OK(ctx, ctx->wfAttHi.reserve(std::max<size_t>(16, (size_t)grid * 3 * hiLevels * wfPoolSize * sizeof(float))));
    a.wfPool = ctx->wfPool.get<char>();
    a.wfAttHi = ctx->wfAttHi.get<float>();
    a.wfPoolSize = wfPoolSize;
    a.wfRingCap = plan.wfRingCap;
    a.wfRingShift = plan.wfRingShift;
    a.wfRingMul3 = plan.wfRingMul3;
    a.wfSwapMin = ctx->tun.wfSwapMin > 0 ? std::min(64, ctx->tun.wfSwapMin) : (plan.form == 4 ? 16 : 32);
    a.wfFarRounds = ctx->tun.wfFarRounds > 0 ? std::min(4, ctx->tun.wfFarRounds) : (ctx->scene.numNodes <= (1 << 20) ? 2 : 1);
    a.wfSwapBig = std::max(a.wfSwapMin, std::min(64, ctx->tun.wfSwapBig));
    HIP_OK(ctx, hipHostGetDevicePointer((void**)&a.wfError, ctx->dWfError, 0));
  } else if (plan.form == 1) {
    HIP_OK(ctx, ctx->attScratch.reserve((size_t)(3 * p->maxBounce + 3) * grid * SRT_BLOCK_TREE * sizeof(float)));
    a.attScratch = ctx->attScratch.get<float>();
  }
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

extern "C++" int checkAdaptive(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, bool device,
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

static int srtRenderFeatureTileListImpl(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, const void* dTileList,
                                        int32_t numListed, void* const dPlaneImages[4], int32_t accumulate, void* streamPtr);

extern "C++" int srtRenderAdaptiveImpl(SrtContext* ctx, const SrtRenderParams* pIn, const SrtAdaptiveParams* ap, void* dAccumImage,
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

int srtTraceRays(SrtContext* ctx, const SrtRay* rays, int64_t n, SrtHit* hits, int32_t traversal) {
  if (!ctx || !rays || !hits || n < 0) return 1;
  if (checkSceneReady(ctx, "trace")) return 1;
  if (n == 0) return 0;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  DeviceBuffer dRays, dHits;
  if (dRays.reserve(n * sizeof(SrtRay)) != hipSuccess || dHits.reserve(n * sizeof(SrtHit)) != hipSuccess) return fail(ctx, "trace: hipMalloc");
  if (hipMemcpy(dRays.get(), rays, n * sizeof(SrtRay), hipMemcpyHostToDevice) != hipSuccess) return fail(ctx, "trace: copy in");
  TraceArgs a;
  a.scene = ctx->scene;
  a.rays = dRays.get<const SrtRay>();
  a.hits = dHits.get<SrtHit>();
  a.n = n;
  size_t lds = (size_t)std::max(ctx->scene.stackDepth, 1) * 256 * sizeof(int32_t);
  int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->prop.multiProcessorCount * 8);
  int e = srt_launch_trace(&a, traversal, grid, lds, nullptr);
  if (e) return fail(ctx, "trace launch failed: %s", hipGetErrorString((hipError_t)e));
  if (hipDeviceSynchronize() != hipSuccess) return fail(ctx, "trace kernel failed");
  if (hipMemcpy(hits, dHits.get(), n * sizeof(SrtHit), hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, "trace: copy out");
  return 0;
}

// test entry: material::scatter known answers through the kernel's own shade()

int srtScatterRays(SrtContext* ctx, const SrtRay* rays, const SrtHit* hits, int32_t n, uint64_t seed, float* out13) {
  if (!ctx || !rays || !hits || !out13 || n < 1) return 1;
  if (checkSceneReady(ctx, "scatter")) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  for (int i = 0; i < n; ++i)
    if (hits[i].material < 0) return fail(ctx, "scatter: hit %d has no material", i);
  DeviceBuffer dRays, dHits, dOut;
  if (dRays.reserve(n * sizeof(SrtRay)) != hipSuccess || dHits.reserve(n * sizeof(SrtHit)) != hipSuccess ||
      dOut.reserve((size_t)n * 13 * 4) != hipSuccess)
    return fail(ctx, "scatter: hipMalloc");
  if (hipMemcpy(dRays.get(), rays, n * sizeof(SrtRay), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dHits.get(), hits, n * sizeof(SrtHit), hipMemcpyHostToDevice) != hipSuccess)
    return fail(ctx, "scatter: copy in");
  int e = srt_launch_scatter(&ctx->scene, dRays.get<const SrtRay>(), dHits.get<const SrtHit>(), dOut.get<float>(), seed, n, nullptr);
  if (e) return fail(ctx, "scatter launch failed");
  if (hipDeviceSynchronize() != hipSuccess) return fail(ctx, "scatter kernel failed");
  if (hipMemcpy(out13, dOut.get(), (size_t)n * 13 * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, "scatter: copy out");
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

int srtUploadScene(SrtContext* ctx, const SrtSceneDesc* d) { SRT_GUARDED(ctx, srtUploadSceneImpl(ctx, d)); }
int srtBuildBvh(const SrtSceneDesc* d, int32_t item, SrtBvhNode* out, int32_t capacity, int32_t* count, int32_t* stackDepth) { SRT_GUARDED(nullptr, srtBuildBvhImpl(d, item, out, capacity, count, stackDepth)); }
int srtGetBvh(SrtContext* ctx, int32_t item, SrtBvhNode* nodes, int32_t capacity, int32_t* count) { SRT_GUARDED(ctx, srtGetBvhImpl(ctx, item, nodes, capacity, count)); }
int srtRenderTiles(SrtContext* ctx, const SrtRenderParams* p, void* dAccumTiles, void* streamPtr) { SRT_GUARDED(ctx, srtRenderTilesImpl(ctx, p, dAccumTiles, streamPtr)); }
int srtRenderTilesMoments(SrtContext* ctx, const SrtRenderParams* p, void* dAccumTiles, void* dMomentTiles, void* streamPtr) {
  SRT_GUARDED(ctx, srtRenderTilesMomentsImpl(ctx, p, dAccumTiles, dMomentTiles, streamPtr));
}
int srtRenderAdaptive(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, void* dAccumImage, void* dMomentsImage,
                      void* dRgba, SrtAdaptiveStats* stats, void* stream) {
  SRT_GUARDED(ctx, srtRenderAdaptiveImpl(ctx, p, ap, dAccumImage, dMomentsImage, dRgba, stats, stream));
}
static int srtRenderAdaptiveGuidedImpl(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, int32_t planes,
                                       void* const dPlaneImages[4], void* dAccumImage, void* dMomentsImage, void* dRgba,
                                       SrtAdaptiveStats* stats, void* stream) {
  if (!ctx) return 1;
  const AdaptiveGuides guides{planes, dPlaneImages, true};
  return srtRenderAdaptiveImpl(ctx, p, ap, dAccumImage, dMomentsImage, dRgba, stats, stream, nullptr, &guides);
}
int srtRenderAdaptiveGuided(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, int32_t planes,
                            void* const dPlaneImages[4], void* dAccumImage, void* dMomentsImage, void* dRgba,
                            SrtAdaptiveStats* stats, void* stream) {
  SRT_GUARDED(ctx, srtRenderAdaptiveGuidedImpl(ctx, p, ap, planes, dPlaneImages, dAccumImage, dMomentsImage, dRgba, stats, stream));
}

/* Feature pass (srt_features.hip).  Reads the scene, the camera and the tile_block tunable; writes only the caller's planes
 * and its own tile counter, so a later render sees the context as it was. */
extern "C++" int checkFeatureArgs(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, const void* const* buffers) {
  if (!ctx) return 1;
  if (!p) return fail(ctx, "features: null parameters");
  if (planes <= 0 || (planes & ~SRT_FEATURE_ALL) != 0) return fail(ctx, "features: bad plane mask 0x%x", (unsigned)planes);
  SrtRenderParams q = *p;  // maxBounce, sppChunks and countStats do not apply
  q.maxBounce = 1;
  q.sppChunks = 0;
  q.countStats = 0;
  if (checkParams(ctx, &q)) return 1;
  if (!buffers) return fail(ctx, "features: null plane array");
  for (int k = 0; k < 4; ++k)
    if ((planes >> k & 1) && !buffers[k]) return fail(ctx, "features: null buffer for selected plane %d", 1 << k);
  return 0;
}

/* What the two feature passes do alike once their arguments are set: the traversal form and its LDS, the kernel's plan, a
 * grid of at most `work` waves, the tile counter reset, the launch.  plan and launch are the pass's own kernel's. */
extern "C++" template <typename Plan, typename Launch>
static int launchFeaturePass(SrtContext* ctx, const SrtRenderParams* p, FeatureArgs& a, int work, hipStream_t stream, Plan plan,
                             Launch launch) {
  const DevScene& sc = ctx->scene;
  // FAITHFUL over a threaded tree that fits a CU's LDS: the stackless walk out of LDS; otherwise the stack walk over
  // scene.nodes (stacks in LDS), which CLOSEST always takes
  const bool closest = p->traversal == SRT_TRAVERSE_CLOSEST;
  const size_t treeBytes = (size_t)sc.numNodes * 32;
  const bool ldsTree = !closest && sc.nodeThread != nullptr && treeBytes <= 160 * 1024;
  const size_t lds = ldsTree ? treeBytes : (size_t)std::max(sc.stackDepth, 1) * SRT_BLOCK * sizeof(int32_t);
  if (lds > 160 * 1024) return fail(ctx, "features: BVH depth %d needs %zu B of LDS per workgroup", sc.stackDepth, lds);
  int block = 0, perCU = 1;
  int rc = plan(closest, ldsTree, lds, &block, &perCU);
  if (rc) return fail(ctx, "features: kernel setup failed: %s", hipGetErrorString((hipError_t)rc));
  const int wavesPerGroup = block / 64;
  const int grid = std::max(1, std::min(ctx->prop.multiProcessorCount * perCU, (work + wavesPerGroup - 1) / wavesPerGroup));
  HIP_OK(ctx, ctx->dFeatureCounter.reserve(16 * sizeof(int32_t)));
  a.counter = ctx->dFeatureCounter.get<int32_t>();
  HIP_OK(ctx, hipMemsetAsync(a.counter, 0, sizeof(int32_t), stream));
  rc = launch(closest, ldsTree, grid, lds);
  if (rc) return fail(ctx, "features launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C++" int srtRenderFeatureTilesImpl(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, void* const dPlanes[4], void* streamPtr) {
  if (!ctx) return 1;
  if (checkFeatureArgs(ctx, p, planes, dPlanes)) return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  FeatureArgs a;
  setImageArgs(a, ctx, p);
  a.planes = planes;
  for (int k = 0; k < 4; ++k) a.out[k] = (planes >> k & 1) ? static_cast<float4*>(dPlanes[k]) : nullptr;
  return launchFeaturePass(ctx, p, a, a.numLocalTiles, stream, [&](bool closest, bool ldsTree, size_t lds, int* block, int* perCU) {
    return srt_features_plan(closest, ldsTree, lds, block, perCU);
  }, [&](bool closest, bool ldsTree, int grid, size_t lds) { return srt_launch_features(&a, closest, ldsTree, grid, lds, stream); });
}

int srtRenderFeatureTiles(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, void* const dPlanes[4], void* stream) {
  SRT_GUARDED(ctx, srtRenderFeatureTilesImpl(ctx, p, planes, dPlanes, stream));
}

/* Feature pass over a tile list (srt_features_list.hip), into image-order planes.  The feature pass's side effects: its own
 * counter and the caller's planes. */
static int srtRenderFeatureTileListImpl(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, const void* dTileList,
                                        int32_t numListed, void* const dPlaneImages[4], int32_t accumulate, void* streamPtr) {
  if (!ctx) return 1;
  if (checkFeatureArgs(ctx, p, planes, dPlaneImages)) return 1;
  if (p->tileFirst != 0 || p->tileStride != 1) return fail(ctx, "features: a tile list covers the whole image (tileFirst 0, tileStride 1)");
  if (numListed < 0 || numListed > srtNumTiles(p->imageWidth, p->imageHeight))
    return fail(ctx, "features: bad tile list of %d tiles", numListed);
  if (numListed > 0 && !dTileList) return fail(ctx, "features: null tile list");
  if (numListed == 0) return 0;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  FeatureListArgs a;
  setImageArgs(a.f, ctx, p);
  a.f.planes = planes;
  for (int k = 0; k < 4; ++k) a.f.out[k] = (planes >> k & 1) ? static_cast<float4*>(dPlaneImages[k]) : nullptr;
  a.list = static_cast<const uint32_t*>(dTileList);
  a.numListed = numListed;
  return launchFeaturePass(ctx, p, a.f, numListed, stream, [&](bool closest, bool ldsTree, size_t lds, int* block, int* perCU) {
    return srt_features_list_plan(closest, ldsTree, accumulate != 0, lds, block, perCU);
  }, [&](bool closest, bool ldsTree, int grid, size_t lds) {
    return srt_launch_features_list(&a, closest, ldsTree, accumulate != 0, grid, lds, stream);
  });
}
int srtRenderFeatureTileList(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, const void* dTileList, int32_t numListed,
                             void* const dPlaneImages[4], int32_t accumulate, void* stream) {
  SRT_GUARDED(ctx, srtRenderFeatureTileListImpl(ctx, p, planes, dTileList, numListed, dPlaneImages, accumulate, stream));
}

/* Denoiser (srt_denoise.hip).  Reads the tunable denoise_lds_step; writes only the caller's outputs and its own scratch. */
extern "C++" int checkDenoiseParams(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, DenoiseArgs& a,
                                    int& iterations, bool moments) {
  if (!d) return fail(ctx, "denoise: null parameters");
  if (width <= 0 || height <= 0) return fail(ctx, "denoise: image size %dx%d must be positive", width, height);
  if ((int64_t)width * height > 0x7fffffff) return fail(ctx, "denoise: image of %dx%d pixels is too large", width, height);
  iterations = d->iterations == 0 ? SRT_DENOISE_DEFAULT_ITERATIONS : d->iterations;
  if (iterations < 1 || iterations > SRT_DENOISE_MAX_ITERATIONS)
    return fail(ctx, "denoise: iterations %d not in [1, %d] (0 = %d)", d->iterations, SRT_DENOISE_MAX_ITERATIONS,
                SRT_DENOISE_DEFAULT_ITERATIONS);
  const float sig[3] = {d->sigmaLuminance, d->sigmaNormal, d->sigmaDepth};
  const float dflt[3] = {moments ? SRT_DENOISE_MOMENTS_DEFAULT_SIGMA_LUMINANCE : SRT_DENOISE_DEFAULT_SIGMA_LUMINANCE,
                         SRT_DENOISE_DEFAULT_SIGMA_NORMAL, SRT_DENOISE_DEFAULT_SIGMA_DEPTH};
  float use[3];
  for (int k = 0; k < 3; ++k) {
    if (!(sig[k] >= 0.0f && sig[k] < 1e30f)) return fail(ctx, "denoise: sigma %g must be finite and >= 0 (0 = default)", sig[k]);
    use[k] = sig[k] == 0.0f ? dflt[k] : sig[k];
  }
  memset(&a, 0, sizeof a);
  a.width = width;
  a.height = height;
  a.sigmaL = use[0];
  a.sigmaN = use[1];
  a.sigmaZ = use[2];
  return 0;
}

// srtDenoiseMoments (moments = true): dMoments may be null, and then this is srtDenoise bit for bit
extern "C++" int srtDenoiseImpl(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, const void* dBeauty,
                                const void* const dPlanes[4], void* dOut, void* dRgba, void* streamPtr, bool moments,
                                const void* dMoments) {
  if (!ctx) return 1;
  DenoiseArgs a;
  int iterations = 0;
  if (checkDenoiseParams(ctx, d, width, height, a, iterations, moments && dMoments)) return 1;
  if (!dBeauty) return fail(ctx, "denoise: null beauty buffer");
  if (!dPlanes) return fail(ctx, "denoise: null plane array");
  if (!dPlanes[1]) return fail(ctx, "denoise: the NORMAL plane is required");
  if (!dPlanes[3]) return fail(ctx, "denoise: the DEPTH plane is required");
  if (d->demodulate && !dPlanes[0]) return fail(ctx, "denoise: demodulate needs the ALBEDO plane");
  if (!dOut && !dRgba) return fail(ctx, "denoise: no output buffer");
  HIP_OK(ctx, hipSetDevice(ctx->device));
  const size_t nPix = (size_t)width * height;
  HIP_OK(ctx, ctx->denoiseScratch.reserve(nPix * SRT_DENOISE_SCRATCH_BYTES_PER_PIXEL));
  char* s = ctx->denoiseScratch.get<char>();
  a.beauty = static_cast<const float4*>(dBeauty);
  a.normal = static_cast<const float4*>(dPlanes[1]);
  a.depth = static_cast<const float4*>(dPlanes[3]);
  a.albedo = d->demodulate ? static_cast<const float4*>(dPlanes[0]) : nullptr;
  a.guide = reinterpret_cast<float4*>(s);
  a.col[0] = reinterpret_cast<float4*>(s + 16 * nPix);
  a.col[1] = reinterpret_cast<float4*>(s + 32 * nPix);
  a.grad = reinterpret_cast<float2*>(s + 48 * nPix);
  a.out = static_cast<float4*>(dOut);
  a.rgba = static_cast<uint8_t*>(dRgba);
  a.moments = moments ? static_cast<const float4*>(dMoments) : nullptr;
  const int rc = srt_launch_denoise(&a, iterations, std::max(0, ctx->tun.denoiseLdsStep), static_cast<hipStream_t>(streamPtr));
  if (rc) return fail(ctx, "denoise launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

int srtDenoise(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, const void* dBeauty,
               const void* const dPlanes[4], void* dOut, void* dRgba, void* stream) {
  SRT_GUARDED(ctx, srtDenoiseImpl(ctx, d, width, height, dBeauty, dPlanes, dOut, dRgba, stream));
}
int srtDenoiseMoments(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, const void* dBeauty,
                      const void* const dPlanes[4], const void* dMoments, void* dOut, void* dRgba, void* stream) {
  SRT_GUARDED(ctx, srtDenoiseImpl(ctx, d, width, height, dBeauty, dPlanes, dOut, dRgba, stream, true, dMoments));
}

/* Temporal accumulation (srt_temporal.hip).  Reads nothing of the context but the device ordinal; the frame entry keeps
 * the histories and the previous camera in the context. */
static bool sameProjection(const SrtCamera& a, const SrtCamera& b) {
  return !memcmp(a.origin, b.origin, 12) && !memcmp(a.lleft, b.lleft, 12) && !memcmp(a.horizontal, b.horizontal, 12) &&
         !memcmp(a.vertical, b.vertical, 12) && !memcmp(a.w, b.w, 12);
}

extern "C++" int checkTemporalParams(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, TemporalArgs& a) {
  if (!t) return fail(ctx, "temporal: null parameters");
  if (width < 2 || height < 2) return fail(ctx, "temporal: image size %dx%d must be at least 2x2", width, height);
  if ((int64_t)width * height > 0x7fffffff / 3) return fail(ctx, "temporal: image of %dx%d pixels is too large", width, height);
  if (!(t->normalCos >= 0.0f && t->normalCos <= 1.0f)) return fail(ctx, "temporal: normalCos %g must be in [0, 1] (0 = default)", t->normalCos);
  if (!(t->planeDist >= 0.0f)) return fail(ctx, "temporal: planeDist %g must be >= 0 (0 = default)", t->planeDist);
  if (!(t->maxHistory >= 0.0f)) return fail(ctx, "temporal: maxHistory %g must be >= 0 (0 = default, +inf = no cap)", t->maxHistory);
  memset(&a, 0, sizeof a);
  a.width = width;
  a.height = height;
  a.normalCos = t->normalCos == 0.0f ? SRT_TEMPORAL_DEFAULT_NORMAL_COS : t->normalCos;
  a.planeDist = t->planeDist == 0.0f ? SRT_TEMPORAL_DEFAULT_PLANE_DIST : t->planeDist;
  a.maxHistory = t->maxHistory == 0.0f ? SRT_TEMPORAL_DEFAULT_MAX_HISTORY : t->maxHistory;
  return 0;
}

// Everything srtTemporalAccumulate checks, and the kernel's arguments: nothing is launched
static int temporalArgs(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* dBeauty,
                        const void* dMoments, const void* const dPlanes[4], const SrtCamera* cam, const SrtCamera* prevCam,
                        const void* dHistoryIn, void* dBeautyOut, void* dMomentsOut, void* dHistoryOut, TemporalArgs& a) {
  if (!ctx) return 1;
  if (checkTemporalParams(ctx, t, width, height, a)) return 1;
  if (!dBeauty) return fail(ctx, "temporal: null beauty buffer");
  if (!dPlanes) return fail(ctx, "temporal: null plane array");
  if (!dPlanes[1]) return fail(ctx, "temporal: the NORMAL plane is required");
  if (!dPlanes[2]) return fail(ctx, "temporal: the POSITION plane is required");
  if (!dPlanes[3]) return fail(ctx, "temporal: the DEPTH plane is required");
  if (t->demodulate && !dPlanes[0]) return fail(ctx, "temporal: demodulate needs the ALBEDO plane");
  if (!dBeautyOut && !dMomentsOut) return fail(ctx, "temporal: no output buffer");
  if (!dHistoryOut) return fail(ctx, "temporal: null history output");
  if (dHistoryOut == dHistoryIn) return fail(ctx, "temporal: the history is not updated in place (dHistoryOut == dHistoryIn)");
  if (!cam || (dHistoryIn && !prevCam)) return fail(ctx, "temporal: null camera");
  HIP_OK(ctx, hipSetDevice(ctx->device));
  a.beauty = static_cast<const float4*>(dBeauty);
  a.moments = static_cast<const float4*>(dMoments);
  a.albedo = t->demodulate ? static_cast<const float4*>(dPlanes[0]) : nullptr;
  a.normal = static_cast<const float4*>(dPlanes[1]);
  a.position = static_cast<const float4*>(dPlanes[2]);
  a.depth = static_cast<const float4*>(dPlanes[3]);
  a.historyIn = static_cast<const float4*>(dHistoryIn);
  a.beautyOut = static_cast<float4*>(dBeautyOut);
  a.momentsOut = static_cast<float4*>(dMomentsOut);
  a.historyOut = static_cast<float4*>(dHistoryOut);
  a.cam = *cam;
  a.prev = dHistoryIn ? *prevCam : *cam;
  a.sameCamera = sameProjection(a.cam, a.prev) ? 1 : 0;
  return 0;
}

extern "C++" int srtTemporalAccumulateImpl(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height,
                                           const void* dBeauty, const void* dMoments, const void* const dPlanes[4], const SrtCamera* cam,
                                           const SrtCamera* prevCam, const void* dHistoryIn, void* dBeautyOut, void* dMomentsOut,
                                           void* dHistoryOut, void* streamPtr) {
  TemporalArgs a;
  if (temporalArgs(ctx, t, width, height, dBeauty, dMoments, dPlanes, cam, prevCam, dHistoryIn, dBeautyOut, dMomentsOut, dHistoryOut, a))
    return 1;
  const int rc = srt_launch_temporal(&a, static_cast<hipStream_t>(streamPtr));
  if (rc) return fail(ctx, "temporal launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// SrtTemporalStats from the finished frame's DEVICE buffers: this frame's sums, an accumulated plane (its w is the
// output count) and the new history
extern "C++" int temporalStats(SrtContext* ctx, size_t nPix, const void* dCurrent, const void* dAccumulated, const void* dHistory,
                               SrtTemporalStats* stats) {
  std::vector<float> cur(nPix * 4), acc(nPix * 4), hist(nPix * 4);
  if (hipMemcpy(cur.data(), dCurrent, nPix * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(acc.data(), dAccumulated, nPix * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(hist.data(), dHistory, nPix * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(ctx, "temporal: copy stats");
  stats->historyPixels = 0;
  double sum = 0.0;
  for (size_t i = 0; i < nPix; ++i) {
    if (acc[4 * i + 3] > cur[4 * i + 3]) stats->historyPixels++;
    sum += (double)hist[4 * i + 3];
  }
  stats->meanHistoryCount = sum / (double)nPix;
  return 0;
}

/* Temporal-adaptive frames (srt_temporal_adaptive.hip): the reprojected history once per frame, srtRenderAdaptive's rounds
 * deciding on the pooled moments, srtTemporalAccumulate of the final sums. */
static int srtTemporalReprojectImpl(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height,
                                    const void* const dPlanes[4], const SrtCamera* cam, const SrtCamera* prevCam,
                                    const void* dHistoryIn, void* dReprojected, void* streamPtr) {
  if (!ctx) return 1;
  if (!dReprojected) return fail(ctx, "temporal: null reprojected buffer");
  TemporalArgs a;
  // srtTemporalAccumulate's checks; the beauty and its outputs are not part of this entry (any non-null pointer passes)
  if (temporalArgs(ctx, t, width, height, dReprojected, nullptr, dPlanes, cam, prevCam, dHistoryIn, dReprojected, nullptr, dReprojected, a))
    return 1;
  a.beauty = nullptr;
  a.beautyOut = nullptr;
  const int rc = srt_launch_temporal_reproject(&a, static_cast<hipStream_t>(streamPtr));
  if (rc) return fail(ctx, "temporal reprojection launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C++" int srtRenderTemporalAdaptiveImpl(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap,
                                               const SrtTemporalParams* t, const void* const dPlanes[4], const SrtCamera* prevCam,
                                               const void* dHistoryIn, void* dAccumImage, void* dMomentsImage, void* dBeautyOut,
                                               void* dMomentsOut, void* dHistoryOut, SrtTemporalAdaptiveStats* stats, void* streamPtr,
                                               bool guided) {
  // every check of both halves before the first launch
  if (!ctx) return 1;
  if (checkAdaptive(ctx, p, ap, true, dAccumImage, dMomentsImage)) return 1;
  const int W = p->imageWidth, H = p->imageHeight;
  const size_t nPix = (size_t)W * H;
  TemporalArgs a;
  if (temporalArgs(ctx, t, W, H, dAccumImage, dMomentsImage, dPlanes, &ctx->camFull, prevCam, dHistoryIn, dBeautyOut, dMomentsOut,
                   dHistoryOut, a))
    return 1;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  HIP_OK(ctx, ctx->temporalReprojected.reserve(nPix * SRT_TEMPORAL_REPROJECTED_BYTES_PER_PIXEL));
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  TemporalArgs ra = a;
  ra.historyOut = ctx->temporalReprojected.get<float4>();
  int rc = srt_launch_temporal_reproject(&ra, stream);
  if (rc) return fail(ctx, "temporal reprojection launch failed: %s", hipGetErrorString((hipError_t)rc));
  AdaptivePool pool{ctx->temporalReprojected.get<const float4>(), a.albedo};
  SrtTemporalAdaptiveStats st;
  memset(&st, 0, sizeof st);
  // guided: the rounds from 1 on extend the caller's planes (they hold round 0).  The pooled decisions keep reading the
  // ALBEDO means of the first p->spp samples -- h was formed beside them -- from a copy that lives as long as this call
  AdaptiveGuides guides{0, const_cast<void* const*>(dPlanes), false};
  DeviceBuffer albedoFirst;
  if (guided) {
    for (int k = 0; k < 4; ++k)
      if (dPlanes[k]) guides.planes |= 1 << k;
    if (a.albedo) {
      if (albedoFirst.reserve(nPix * sizeof(float4)) != hipSuccess) return fail(ctx, "temporal: hipMalloc");
      HIP_OK(ctx, hipMemcpyAsync(albedoFirst.get(), a.albedo, nPix * sizeof(float4), hipMemcpyDeviceToDevice, stream));
      pool.albedo = albedoFirst.get<const float4>();
    }
  }
  if (srtRenderAdaptiveImpl(ctx, p, ap, dAccumImage, dMomentsImage, nullptr, &st.adaptive, streamPtr, &pool, guided ? &guides : nullptr))
    return 1;
  rc = srt_launch_temporal(&a, stream);
  if (rc) return fail(ctx, "temporal launch failed: %s", hipGetErrorString((hipError_t)rc));
  if (hipStreamSynchronize(stream) != hipSuccess) return fail(ctx, "temporal: kernel failed: %s", hipGetErrorString(hipGetLastError()));
  if (stats) {
    if (temporalStats(ctx, nPix, dAccumImage, dBeautyOut ? dBeautyOut : dMomentsOut, dHistoryOut, &st.temporal)) return 1;
    *stats = st;
  }
  return 0;
}

int srtTemporalAccumulate(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* dBeauty,
                          const void* dMoments, const void* const dPlanes[4], const SrtCamera* cam, const SrtCamera* prevCam,
                          const void* dHistoryIn, void* dBeautyOut, void* dMomentsOut, void* dHistoryOut, void* stream) {
  SRT_GUARDED(ctx, srtTemporalAccumulateImpl(ctx, t, width, height, dBeauty, dMoments, dPlanes, cam, prevCam, dHistoryIn, dBeautyOut,
                                             dMomentsOut, dHistoryOut, stream));
}
int srtTemporalReproject(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* const dPlanes[4],
                         const SrtCamera* cam, const SrtCamera* prevCam, const void* dHistoryIn, void* dReprojected, void* stream) {
  SRT_GUARDED(ctx, srtTemporalReprojectImpl(ctx, t, width, height, dPlanes, cam, prevCam, dHistoryIn, dReprojected, stream));
}
int srtRenderTemporalAdaptive(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, const SrtTemporalParams* t,
                              const void* const dPlanes[4], const SrtCamera* prevCam, const void* dHistoryIn, void* dAccumImage,
                              void* dMomentsImage, void* dBeautyOut, void* dMomentsOut, void* dHistoryOut,
                              SrtTemporalAdaptiveStats* stats, void* stream) {
  SRT_GUARDED(ctx, srtRenderTemporalAdaptiveImpl(ctx, p, ap, t, dPlanes, prevCam, dHistoryIn, dAccumImage, dMomentsImage, dBeautyOut,
                                                 dMomentsOut, dHistoryOut, stats, stream));
}
int srtRenderTemporalAdaptiveGuided(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap,
                                    const SrtTemporalParams* t, void* const dPlanes[4], const SrtCamera* prevCam,
                                    const void* dHistoryIn, void* dAccumImage, void* dMomentsImage, void* dBeautyOut,
                                    void* dMomentsOut, void* dHistoryOut, SrtTemporalAdaptiveStats* stats, void* stream) {
  SRT_GUARDED(ctx, srtRenderTemporalAdaptiveImpl(ctx, p, ap, t, dPlanes, prevCam, dHistoryIn, dAccumImage, dMomentsImage, dBeautyOut,
                                                 dMomentsOut, dHistoryOut, stats, stream, true));
}
int srtTemporalReset(SrtContext* ctx) {
  if (!ctx) return 1;
  (void)hipSetDevice(ctx->device);
  ctx->temporalValid = false;
  for (auto& h : ctx->temporalHistory) h = DeviceBuffer();
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

/* include/srt_hip_test.h: world item `item`'s slice of DevScene::nodeAxis and DevScene::nodes2, read back as they are */
int srtTestGetTreeAux(SrtContext* ctx, int32_t item, uint8_t* outAxis, float* outPairs16, int32_t capacity, int32_t* count) {
  if (!ctx || !count) return 1;
  if (!ctx->haveScene) return fail(ctx, "srtTestGetTreeAux: no scene uploaded");
  if (item < 0 || item >= (int32_t)ctx->itemNodes.size()) return fail(ctx, "srtTestGetTreeAux: item %d out of range", item);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  int32_t ref = 0;
  HIP_OK(ctx, hipMemcpy(&ref, ctx->scene.world + item, sizeof ref, hipMemcpyDeviceToHost));
  if (ref < 0) return fail(ctx, "srtTestGetTreeAux: item %d is not a tree", item);
  const auto dt = std::find_if(ctx->deviceBuilds.begin(), ctx->deviceBuilds.end(), [&](const DeviceBuild& b) { return b.item == item; });
  const int32_t base = SRT_NODE_INDEX(ref), n = dt != ctx->deviceBuilds.end() ? dt->count : (int32_t)ctx->itemNodes[item].size();
  if (base + n > ctx->scene.numNodes) return fail(ctx, "srtTestGetTreeAux: item %d lies outside the node array", item);
  *count = n;
  if (!outAxis && !outPairs16) return 0;
  if (capacity < n) return fail(ctx, "srtTestGetTreeAux: capacity %d < %d", capacity, n);
  if (outAxis) HIP_OK(ctx, hipMemcpy(outAxis, ctx->scene.nodeAxis + base, (size_t)n, hipMemcpyDeviceToHost));
  if (outPairs16) HIP_OK(ctx, hipMemcpy(outPairs16, ctx->scene.nodes2 + 4 * (size_t)base, (size_t)n * 64, hipMemcpyDeviceToHost));
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
