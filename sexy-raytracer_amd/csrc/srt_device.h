// srt_device.h -- HBM-resident scene layout shared by the host uploader and the kernels.
//
// Every record is a whole number of 16-byte slots so one lane fetches it with
// dwordx4 loads; arrays are separate buffers (nodes / triangle test records /
// triangle shading records / spheres / materials / textures / texels) instead of
// the reference's 160-byte hittableIndexed mega-struct (hittableindexed.h:24-38).
#ifndef SRT_DEVICE_H
#define SRT_DEVICE_H

#include <stdint.h>

#include "../../include/srt_hip.h"
#include "../../include/srt_hip_test.h"

// Child / world reference encoding on the device:
//   ref >= 0          BVH node: the BYTE OFFSET of its record in `nodes` (index * 32), so that a visit needs no
//                     address arithmetic; SRT_NODE_REF / SRT_NODE_INDEX convert
//   ref <  0          primitive: r = ~ref, (r & 1) = 1 sphere / 0 triangle, r >> 1 = index
//   SRT_REF_DONE      traversal sentinel (never a valid primitive)
#define SRT_REF_DONE ((int32_t)0x80000000)
#define SRT_NODE_REF(index) ((int32_t)(index) << 5)
#define SRT_NODE_INDEX(ref) ((int32_t)(ref) >> 5)
#define SRT_MAX_NODES (1 << 25) /* byte offsets (index * 64 in the closest-hit records) stay below 2^31 */
#define SRT_MAX_QUEUES 64
#define SRT_BLOCK 256        // threads per workgroup of the render kernel over node records read through the L1
#define SRT_BLOCK_TREE 1024  // ... over the LDS-resident tree, and of the path-pool kernel: one workgroup per CU
// a primitive's material word: material index, the material's type (SRT_MAT_*) and SRT_MAT_NEEDS_* flags,
// (spheres) bit 30 = moving
#define SRT_MAT_INDEX_MASK 0x00ffffff
#define SRT_MAT_TYPE_SHIFT 24   /* four bits: SRT_MAT_* (two bits) | SRT_MAT_TEXTURED */
#define SRT_MAT_TEXTURED 4      /* a pbr material with at least one texture slot in use */
#define SRT_MAT_FLAGS_SHIFT 28
// the mode of a texture slot of a material's shading record (DevScene::shadeRecs; the record's layout is in srt_path.h)
#define SRT_SLOT_NONE 0u
#define SRT_SLOT_SOLID 1u
#define SRT_SLOT_IMAGE 2u
#define SRT_SLOT_GENERIC 3u
#define SRT_SLOT_CHECKER2 7u  // SRT_SLOT_GENERIC | 4: albedo slot only, colours at +80 / +96 of the record

struct DevMaterial {  // 48 B
  int32_t type;
  int32_t albedoTex, normalTex, metallicTex, roughnessTex;
  float albedo[4];
  float metalness, roughness;  // METAL: metalness = fuzz; DIELECTRIC: metalness = ir
  int32_t flags;               // bit0: some texture of this material reads uv; bit1: it has a normal map
};

struct DevTexture {  // 48 B
  int32_t kind;
  int32_t width, height, bpp;
  int64_t offset;  // byte offset into texels (< 2^31); 3-byte images are stored 4 bytes per texel
  int32_t even, odd;
  float color[3];
  int32_t pad;
};

struct DevScene {
  // 2 x float4 per node: (bmin.xyz, left) (bmax.xyz, right), children as references (above)  -- 32 B / node visit
  const float4* nodes;
  // 3 x float4 per triangle: (v0.xyz, n.x) (v1.xyz, n.y) (v2.xyz, n.z), n = (v1-v0)x(v2-v0)  -- 48 B / test
  const float4* triTest;
  // 4 x float4 per triangle, one aligned 64-byte line: (v0.xyz, d) (n.xyz, k) (m0.xyz, kappa) (m1.xyz, kappa E + floor) --
  // what the certified triangle test of the FAITHFUL render and trace kernels reads (srt_tri_hit.h); triTest is read only
  // by the lanes it cannot decide.  -- 64 B / test
  const float4* triFast;
  // the certified test decides only where |p - v0|_1 is below this: SRT_TRI_W_MAX, or 0 while the tunable "tri_cert" is 0
  // (nothing is below 0: every lane that passes the plane conditions takes the exact test)
  float triWMax;
  // 1: every node box is ordered (min <= max on every axis, all finite).  The kernels whose slab test picks the near and
  // far planes by the ray's sign (srt_slab.h) certify a ray only with this AND fastDivScene (below); the min/max form does
  // not ask.  (Here, in the four bytes in front of the next pointer: no other field moves.)
  int32_t boxOrderedScene;
  // 4 x float4 per triangle, read once per shaded hit:
  // (N^.xyz, uv0.u) (T.xyz, uv0.v) (B.xyz, uv1.u) (uv1.v, uv2.u, uv2.v, material)
  const float4* triShade;
  // 3 x float4 per sphere: (c0.xyz, radius) (c1.xyz, material | moving<<30) (t0, t1, -, -)   -- 16..48 B / test
  const float4* spheres;
  // SRT_TRAVERSE_CLOSEST only: one 64-byte record per node holding BOTH children's boxes,
  // (lmin.xyz, left) (lmax.xyz, right) (rmin.xyz, -) (rmax.xyz, -), node children as byte offsets into this array
  // (index * 64); built from `nodes` on the device after upload (srt_lbvh.hip, srt_pair_nodes).  One 64-byte request
  // per visit tests two boxes; the 32-byte records use half of every request they cause.
  const float4* nodes2;
  // 1 byte per node: the axis its children are split on (left = lower side), 3 = unknown.  Read only by
  // SRT_TRAVERSE_CLOSEST, which visits the nearer child first; FAITHFUL keeps bvh.h's left-then-right.
  const uint8_t* nodeAxis;
  // The LDS-resident-tree kernel walks the tree without a stack (bvh.h:102-103 is a fixed left-then-right order): one
  // word per node, two 16-bit references -- low half: what follows a leaf's first object (its second object, or the high
  // half again for a single-object leaf); high half: where the traversal goes when this node's subtree is done (node
  // INDEX, primitive reference, or 0x8000 = done).  Null unless every tree was built on the host, every node's children
  // are two nodes or two primitives, and every reference fits 15 bits (srt_scene.cpp flattenScene).
  const int32_t* nodeThread;
  // path-pool kernel (srt_wavefront.hip): the material CLASS of every primitive, indexed by ~reference
  // (index << 1 | sphere): 0 triangle with a pbr material, 1 sphere with a pbr material that reads neither uv nor a normal
  // map, 2 anything else.  A hit goes to its class's ring, so a hit step runs one class's code.
  const uint8_t* primClass;
  int32_t numPrimClass;
  // path-pool kernel, hybrid form (a tree that does not fit into LDS): threaded records with 32-bit references --
  // (bmin.xyz, reference taken on a box hit) (bmax.xyz, successor << 2 | what follows a leaf's first object: 0 nothing,
  // 1 the next primitive of the same array, 2 primSecond[~first]) -- renumbered so that the wfResident nodes kept in LDS
  // come first (srt_scene.cpp: the boxes of largest surface, closed upward), the world list's roots in that numbering, and
  // the second object of the leaves whose objects are not neighbours in one array (indexed like primClass).  "Done" is
  // -2^29 here.  Null when the tree fits (or is not a host-built tree of two-node / two-primitive nodes).
  const float4* nodesWf;
  const int32_t* worldWf;
  const int32_t* primSecond;
  int32_t wfResident;
  const int32_t* triPrimId;  // device index -> index into the scene's prims[] list
  const int32_t* sphPrimId;
  const int32_t* world;  // refs, world-list order
  int32_t numWorld;
  int32_t stackDepth;  // max pending right children over all trees
  int32_t numNodes, numTris, numSpheres;  // record counts (buffer-resource extents)
  int32_t fastDivScene;  // 1: every box coordinate is 0 or in [2^-77, 2^30] (see fastDiv in srt_kernels.hip)
  const DevMaterial* materials;
  // what the hit step reads: 128 bytes per material -- scalars, a light's emit texture, the four pbr texture slots
  // resolved to (mode, width, height, texel offset); layout at srt_kernels.hip "materials"
  const uint4* shadeRecs;
  int32_t numMaterials;
  const DevTexture* textures;
  const uint8_t* texels;  // images of >= 3 bytes per pixel as one dword per texel (RGBA8), others as byte rows
  int32_t texelBytes;     // extent of `texels` (buffer-resource bound: reads past it return 0)
  // path-pool kernel, whole-tree form: the REGROUPED tree (srt_regroup.h) -- `nodes`' layout, size, node range per world
  // item and leaf records, other inner nodes over the same leaf sequence -- and its thread links, `nodeThread`'s format.
  // The production, moments and profiling instances copy it into LDS in place of the reference tree; every walk ends at
  // the same (t, primitive).  Null: not built (a tree beyond LDS, a caller-built tree, a box that is not ordered), or
  // switched off for the launch (tunable "wf_regroup", a counting launch, boxOrderedScene lost in a refit).
  const float4* nodesRg;
  const int32_t* nodeThreadRg;
  // ... and its WALK SEQUENCE (srt_regroup.h srtRegroupWalk, tunable "wf_regroup" 2): the regrouped tree without the gates
  // that rarely cull a ray.  Three words per kept record, numWalk records in pre-order: its source record in nodesRg (the
  // box is read there at every launch: a refit needs nothing here) and its two link words (srt_wf_links.h srtWfSeq*);
  // behind them one entry word per world item.  The set-up copy fills the first numWalk slots of the LDS tree from it, and
  // the launch hands the entry words to the kernel in `world`'s place.  Null / 0: not built, or not asked for.
  const int32_t* walkSeq;
  int32_t numWalk;
  // ... and the HEAD of its walks (SrtRegroupWalk::head, tunable "wf_head"): the leaf word of sequence record 0 where every
  // walk begins at that leaf and its objects are spheres, else 0.  A launch that does not walk the sequence hands over 0.
  // The kernel reads it from the argument segment inside its swap step.  (In the four bytes behind numWalk: no field moves.)
  int32_t wfHead;
};

struct DevCamera {
  float origin[3], lleft[3], horizontal[3], vertical[3], hor[3], vert[3];
  float lensRadius, time0, time1;
};

struct SrtFixedAccum {  // 32 B per pixel of a rank's tile buffer: exact sum of the items' partial sums (commitFixed)
  long long r, g, b;    // units of 2^-36
  uint32_t flags;       // bit k: a NaN partial sum in channel k; bit 3+k: +inf; bit 6+k: -inf
  uint32_t pad;
};

struct RenderArgs {
  DevScene scene;
  DevCamera cam;
  int32_t imageWidth, imageHeight, tilesX, tilesY, numTiles;
  int32_t spp, maxBounce, sampleFirst;
  uint64_t seed;
  float background[3];
  float tMin;
  int32_t tileFirst, tileStride, numLocalTiles;
  int32_t tileBlock;   // tile order: row-major inside tileBlock x tileBlock blocks of tiles (srtTileFromOrder)
  int32_t numQueues;   // work counters; a wave starts on queue blockIdx % numQueues
  int32_t unitTiles, numUnits;  // queue q owns units q, q+numQueues, ... of unitTiles consecutive local tiles
  int32_t sppChunks;
  int32_t sppBase, sppRem;  // chunk c renders samples [c * sppBase + min(c, sppRem), ...): spp = sppChunks * sppBase + sppRem
  int32_t numWork;  // numLocalTiles * sppChunks * 64 (one item = one pixel x one sample chunk)
  int32_t shadeMin, primMin, hitMin;  // wave scheduler thresholds (lanes waiting before that step kind runs)
  int32_t fuseMin;            // lanes at nodes after a primitive step for a node burst to follow in the same trip
  int32_t nodeBurst;          // max node visits per scheduling decision
  int32_t keepEighths;        // a node burst goes on while nNodes * keepEighths / 8 of its lanes are still at nodes
  int32_t primAgainMin;       // lanes at a primitive again after a primitive step for a second round in the same trip
  int32_t* queue;   // persistent-wave work counters, 16 ints apart (zeroed before launch)
  float4* out;      // sppChunks == 1: the caller's [localTile][64] buffer (the reference's float running sum, written
                    // directly); scratch path: chunk slots [chunk][localTile][64]
  int32_t chunkStride;  // scratch path: numLocalTiles * 64, else 0
  SrtFixedAccum* fix;   // atomic path: [localTile][64], items add their fixed-point partial sums here (null otherwise)
  float fixLimit;       // exact chunk sums: a partial sum of this much or more counts as infinite (toFixed36)
  // The moments instances (srtRenderTilesMoments) neither count nor profile: their two pointers share the places of the
  // counters and the AOV records, so that the struct -- and the code of every other instance -- stays as it was.
  union {
    unsigned long long* stats;  // 8 counters (SrtStats order) or nullptr
    SrtFixedAccum* mfix;        // moments instances, atomic path: the moments' exact sums, as `fix` (null otherwise)
  };
  union {
    SrtAovRecord* aov;  // counting variants only: per-pixel record of the ray at bounce aovDepth (srtRenderAov)
    float4* mout;       // moments instances: {sum l, sum l^2, 0, count} per item, laid out as `out`
  };
  int32_t aovDepth;
  float* attScratch;          // LDS-resident-tree variant: [3 * maxBounce + 3][grid * 1024] attenuation slots in global memory
  // work-item decomposition without divisions (restart step): groups of 64 items per unit, float reciprocals of
  // unitGroups and sppChunks, and srtTileFromOrder as a table over the image's tiles (tx | ty << 16)
  int32_t unitGroups;
  float rcpUnitGroups, rcpChunks;
  const uint32_t* tileXY;
  // path-pool kernel (srt_wavefront.hip): wfPoolSize contexts of 128 B per workgroup, the attenuation levels beyond
  // the four a context holds ([workgroup][level - 4][channel][context]), ring capacity (a power of two >= wfPoolSize),
  // lanes with nothing to traverse before a wave swaps finished walks for READY contexts (wfSwapMin when no full batch
  // waits to be served, wfSwapBig regardless), and the word a workgroup that gave up (bounded spin exceeded) adds to
  char* wfPool;
  float* wfAttHi;
  int32_t wfPoolSize, wfRingCap, wfSwapMin, wfSwapBig;
  int32_t wfRingShift, wfRingMul3;  // wfRingCap = (wfRingMul3 ? 3 : 1) << wfRingShift
  int32_t wfFarRounds;  // hybrid form: node visits per round (the last one serves the lanes outside LDS as well)
  int32_t* wfError;
};

// The form of the render kernel.  The values are srtGetLaunchInfo's codes (launch_info()["lds_tree_mode"]): they stay.
enum SrtRenderForm : int32_t {
  SRT_FORM_STACK = 0,             // srt_render_kernel over node records read through the L1, per-lane stacks in LDS
  SRT_FORM_LDS_TREE = 1,          // srt_render_kernel over the LDS-resident tree, attenuation stacks in global memory
  SRT_FORM_LDS_TREE_ATT = 2,      // ... attenuation stacks in LDS behind the tree
  SRT_FORM_PATH_POOL = 3,         // srt_render_wf_kernel over the LDS-resident tree
  SRT_FORM_PATH_POOL_HYBRID = 4,  // ... its hybrid form: the tree's top in LDS
};
inline bool srtFormIsPathPool(SrtRenderForm f) { return f == SRT_FORM_PATH_POOL || f == SRT_FORM_PATH_POOL_HYBRID; }
inline bool srtFormIsLdsTree(SrtRenderForm f) { return f == SRT_FORM_LDS_TREE || f == SRT_FORM_LDS_TREE_ATT; }

// One render launch, decided by srt_plan.cpp planRender.  closest, single, count and profile are the template arguments of
// the instance that runs (srt_launch.h srt_render_kernel_for, srt_render_wf_kernel_for).
struct RenderPlan {
  SrtRenderForm form;
  bool closest, single, count, profile;
  bool moments;   // srtRenderTilesMoments: the MOMENTS instance of the same form (never counting or profiling)
  int32_t block;  // threads per workgroup
  size_t lds;     // dynamic LDS bytes per workgroup
  int32_t wfRingCap, wfRingShift, wfRingMul3;  // forms 3 and 4: RenderArgs::wfRingCap = (wfRingMul3 ? 3 : 1) << wfRingShift
};
typedef void (*RenderKernel)(const RenderArgs);

// the context's statistics area (96 words): 0-17 SrtStats, 18-27 the shade profile, 32-77 the path-pool profile, and
#define SRT_STATS_TRI_UNDECIDED 80 /* srtTraceRays: triangle tests of the last call that the certificate left undecided */
struct TraceArgs {
  DevScene scene;
  const SrtRay* rays;
  SrtHit* hits;
  int64_t n;
  unsigned long long* triUndecided;  // the launch's triangle tests the certificate left to the exact test are added here
};

// srtTraceRaysDevice / srtOccludedDevice (srt_query.hip): every pointer is the caller's DEVICE memory
struct QueryArgs {
  DevScene scene;
  const float* rays;   // SrtRay[n] as nine floats each (4-byte aligned)
  int4* hits;          // SrtRayHit[n], or null
  SrtHit* records;     // SrtHit[n] with zero counters, or null
  uint8_t* occluded;   // the any-hit form's one output
  int64_t n;
};

// srtCameraRaysDevice / srtScatterRaysDevice / srtPathStepDevice (srt_pathstep.hip): every pointer is the caller's DEVICE
// memory; rays as nine floats each, rng = Pcg::state per entry, out = SrtPathOut as two int4 per entry
struct CameraRaysArgs {
  DevCamera cam;
  int32_t imageWidth, imageHeight, spp, sampleFirst;
  uint64_t seed;
  float tMin;
  const int32_t* pixelSample;  // {pixel index, absolute sample index} per entry, or null: entry i = (i / spp, sampleFirst + i % spp)
  float* rays;
  uint64_t* rng;
  int64_t n;
};
struct ScatterDeviceArgs {
  DevScene scene;
  const float* rays;
  const SrtHit* records;
  uint64_t* rng;
  int4* out;
  float* raysOut;  // may be `rays`
  int64_t n;
};
struct PathStepArgs {
  DevScene scene;
  const float* rays;
  const uint8_t* active;  // or null: every entry
  uint64_t* rng;
  int4* out;
  float* raysOut;  // may be `rays`
  int4* hits;      // SrtRayHit[n], or null
  int64_t n;
};

// srtRenderFeatureTiles (srt_features.hip): the first hit of every camera ray the beauty render traces, as feature planes
// in the beauty tiles' layout
struct FeatureArgs {
  DevScene scene;
  DevCamera cam;
  int32_t imageWidth, imageHeight, tilesX, tilesY, numTiles;
  int32_t spp, sampleFirst;
  uint64_t seed;
  float background[3];
  float tMin;
  int32_t tileFirst, tileStride, numLocalTiles, tileBlock;
  int32_t planes;     // SRT_FEATURE_* bits
  float4* out[4];     // [plane bit index][localTile][64], null for a plane not selected
  int32_t* counter;   // next local tile to take (zeroed before launch)
};

// srtRenderFeatureTileList (srt_features_list.hip): the feature pass of the listed tiles, into image-order planes.  Of f,
// tileFirst, tileStride, numLocalTiles, numTiles and tileBlock are not read; f.out[k] = float4[W*H] in image order.
// srtRenderMotionTiles (srt_motion.hip): the feature pass's launch (f.out[0] = the motion plane, f.planes is not read) with
// the primitive records of the previous srtRefitScene, laid out as scene.triTest and scene.spheres
struct MotionArgs {
  FeatureArgs f;
  const float4* prevTriTest;
  const float4* prevSpheres;
};

struct FeatureListArgs {
  FeatureArgs f;
  const uint32_t* list;  // tx | ty << 16 per listed tile (RenderArgs::tileXY's format)
  int32_t numListed;     // f.counter: the next list position to take (zeroed before launch)
};

// srtDenoise (srt_denoise.hip): the edge-aware a-trous filter over image-order planes.  Scratch in the context, 56 B per
// pixel: guide, gradient and the two colour buffers.
struct DenoiseArgs {
  int32_t width, height;
  const float4* beauty;  // rgb sums, w = sample count
  const float4* normal;  // sums with counts, as the resolve of a feature tile buffer gives them
  const float4* depth;
  const float4* albedo;  // null unless demodulating
  float sigmaL, sigmaN, sigmaZ;
  float4* guide;         // {n.xyz, z}; z NaN: a miss
  float2* grad;          // the depth gradient (zx, zy), centre-only
  float4* col[2];        // {e.rgb, v}; e.x NaN: not valid
  float4* out;           // may be null: rgb = denoised mean, w = the beauty count
  uint8_t* rgba;         // may be null
  const float4* moments; // srtDenoiseMoments: {sum l, sum l^2, 0, count} per pixel (image order), or null
};

// srtTemporalAccumulate (srt_temporal.hip): image-order planes in, accumulated planes and the new history out.  A
// history is three float4 planes one after the other (include/srt_hip.h).
struct TemporalArgs {
  int32_t width, height;
  const float4* beauty;
  const float4* moments;  // may be null
  const float4* albedo;   // null unless demodulating
  const float4* normal;
  const float4* position;
  const float4* depth;
  const float4* historyIn;  // null: the first frame
  float4* beautyOut;        // may be null
  float4* momentsOut;       // may be null
  float4* historyOut;
  SrtCamera cam, prev;
  int32_t sameCamera;  // cam and prev agree bit for bit in what the projection reads: every pixel is its own history
  float normalCos, planeDist, maxHistory;
  const float4* motion;  // srtTemporalAccumulateMotion: the resolved motion plane (sums with counts), else null
};

struct ResolveArgs {
  const float4* gathered;  // [rank][localTile][64]
  int32_t imageWidth, imageHeight, tilesX;
  int32_t tileStride, numLocalTiles;
  int32_t tileBlock;
  int32_t spp;
  uint8_t* rgba;      // may be null
  float4* accumImage;  // may be null
};


// ---- tile order.  Tiles are numbered along a blocked curve, not row-major: the image is cut into
// B x B blocks of tiles (edge blocks smaller), blocks row-major, tiles row-major inside a block with row
// iy rotated by iy.  Work is issued in this order (so the tiles in flight at any time form a compact 2-D
// patch and the rays in flight stay coherent) and ranks take every tileStride-th position of it (the
// rotation keeps a rank's tiles from lining up in columns).  B = 1 is plain row-major.
#if defined(__HIPCC__)
#define SRT_HD __host__ __device__
#else
#define SRT_HD
#endif
SRT_HD inline void srtTileFromOrder(int i, int tilesX, int tilesY, int B, int& tx, int& ty) {
  const int by = i / (B * tilesX), r = i - by * B * tilesX;
  const int bh = (tilesY - by * B) < B ? (tilesY - by * B) : B;
  const int bx = r / (B * bh), r2 = r - bx * B * bh;
  const int bw = (tilesX - bx * B) < B ? (tilesX - bx * B) : B;
  const int iy = r2 / bw, ixr = r2 - iy * bw;
  int ix = ixr - iy % bw;
  ix = ix < 0 ? ix + bw : ix;
  tx = bx * B + ix;
  ty = by * B + iy;
}
SRT_HD inline int srtOrderFromTile(int tx, int ty, int tilesX, int tilesY, int B) {
  const int by = ty / B, iy = ty - by * B, bx = tx / B, ix = tx - bx * B;
  const int bh = (tilesY - by * B) < B ? (tilesY - by * B) : B;
  const int bw = (tilesX - bx * B) < B ? (tilesX - bx * B) : B;
  return by * B * tilesX + bx * B * bh + iy * bw + (ix + iy) % bw;
}

// ---- the 8-bit quantisation of one channel's mean (color.h:25-41), the device's one copy: srt_resolve_kernel,
// srt_adaptive_resolve_kernel and the last denoise level call it, each with its own scale (1 / spp, 1 / w, none).
// sqrtf is the correctly rounded square root here (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; the
// intrinsic __fsqrt_rn is NOT: without OCML_BASIC_ROUNDED_OPERATIONS it is the native approximation).  The clamp is
// globals.h:17-24: a NaN passes both compares and the cast's undefined result is pinned to 0 (what x86 yields); a
// negative mean has a NaN root, -0.0 has the root -0.0 and gives 0; +inf clamps to 0.999 -> 255.
// tests/test_gpu_quantise.py pins every level boundary byte for byte against an integer square root.
#if defined(__HIPCC__)
__device__ __forceinline__ uint8_t srtQuantise8(float mean) {
  const float g = sqrtf(mean);
  const float q = 256.0f * (g < 0.0f ? 0.0f : (g > 0.999f ? 0.999f : g));
  return (q == q) ? (uint8_t)q : (uint8_t)0;
}
#endif

#endif
