/*
 * srt_hip.h -- C ABI of the MI355X-native path-tracing hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch
 * types.  It sits where the reference keeps its (disabled) device seam
 *
 *     glDevice::init(w, h, std::vector<hittableIndexed>&)       gl.h:28, gl.h:194-267
 *     glDevice::rtFrame(void* frame, w, h, objects)             gl.h:29, gl.h:269-320
 *     glDevice::terminate()                                     gl.h:30
 *     hittableVector::build(list) / hittable::populateVector    hittablevector.h:27-31, hittable.h:32
 *
 * and replaces the body of the integrator loop main.cpp:200-227 (pixel/sample
 * loop -> camera::getRay -> rayColor -> writeColorTarget).
 *
 * Conventions (the reference's: bool returns + text on stderr, caller-owned
 * pixel buffers, main.cpp:182,239): every entry point returns int, 0 = ok,
 * non-zero = error with text available from srtLastError().  No exceptions
 * cross this boundary.  One context per GPU; calls on one context are not
 * thread-safe; different contexts may be driven from different host threads.
 */
#ifndef SRT_HIP_H
#define SRT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ enums */
enum { SRT_PRIM_TRIANGLE = 0, SRT_PRIM_SPHERE = 1 };
/* material.h: pbrMetallicRoughness :23, metal :87, dielectric :104, diffuseLight :139 */
enum { SRT_MAT_PBR = 0, SRT_MAT_METAL = 1, SRT_MAT_DIELECTRIC = 2, SRT_MAT_LIGHT = 3 };
/* texture.h: solidColor :18, checker :34, imagePNG/image3bpp :109/:54 */
enum { SRT_TEX_SOLID = 0, SRT_TEX_CHECKER = 1, SRT_TEX_IMAGE = 2 };
enum { SRT_WORLD_PRIM = 0, SRT_WORLD_BVH = 1 };
/* who builds an SRT_WORLD_BVH item's tree when the caller supplies none:
 * REFERENCE = bvh.h:55-95 on the host (the tree FAITHFUL traversal semantics are defined on);
 * LBVH = a linear BVH built on the device (Morton order + Karras' hierarchy), PLOC = parallel
 * locally-ordered clustering on the device (surface-area driven, tighter trees, a few times the
 * LBVH's build time): both for SRT_TRAVERSE_CLOSEST rendering of large scenes. */
enum { SRT_BUILDER_REFERENCE = 0, SRT_BUILDER_LBVH = 1, SRT_BUILDER_PLOC = 2 };
/* traversal semantics: FAITHFUL = bvh.h:97-105 order with triangle::hit's
 * missing tMax test (model.h:128); CLOSEST adds the t < closest test. */
enum { SRT_TRAVERSE_FAITHFUL = 0, SRT_TRAVERSE_CLOSEST = 1 };

#define SRT_TILE_W 8
#define SRT_TILE_H 8
#define SRT_TILE_PIXELS 64
#define SRT_TILE_BLOCK 8 /* tiles are ordered in 8x8 blocks of tiles, see "Tiles" below */
#define SRT_MAX_BOUNCE 16
#define SRT_NO_HIT (-1)

/* ------------------------------------------------- scene description (in) */

/* One triangle with its vertex data already gathered through the mesh's u16
 * indices (model.h:108-111).  64 bytes. */
typedef struct SrtTriangleIn {
  float p[3][3];   /* positions  parentMesh->positions[vertices[i]]  */
  float uv[3][2];  /* texcoords  parentMesh->texcoords[vertices[i]]  */
  int32_t material;
} SrtTriangleIn;

/* sphere.h:11-15 ctor arguments. */
typedef struct SrtSphereIn {
  float center0[3];
  float center1[3];
  float time0, time1;
  float radius;
  int32_t material;
} SrtSphereIn;

/* One entry of a hittableList::objects vector (hittablelist.h:30), in list order. */
typedef struct SrtPrimRef {
  int32_t type;  /* SRT_PRIM_* */
  int32_t index; /* into triangles[] or spheres[] */
} SrtPrimRef;

/* One entry of the world list handed to rayColor (main.cpp:146,187):
 * a bare primitive, or a bvhNode over prims[first, first+count) with the
 * (time0,time1) given to its ctor (bvh.h:15-16).  nodes == NULL: the library
 * builds the tree (bvh.h:55-95, consuming the global generator); otherwise the
 * caller supplies an already built tree (e.g. from srtBuildBvh at bvhNode
 * construction time, or its own builder): numNodes records in pre-order, node 0
 * the root, child >= 0 a node index GREATER than its parent's, child < 0 a
 * primitive ~child inside [first, first+count). */
typedef struct SrtWorldItem {
  int32_t kind; /* SRT_WORLD_* */
  int32_t first;
  int32_t count;
  float time0, time1;
  int32_t numNodes;
  const struct SrtBvhNode* nodes;
  int32_t builder; /* SRT_BUILDER_* (ignored when nodes != NULL) */
  int32_t pad;
} SrtWorldItem;

/* material.h.  Field use per type:
 *   PBR        albedoTex/normalTex/metallicTex/roughnessTex (-1 = null ptr),
 *              albedo[4] = albedo factor, metalness, roughness
 *   METAL      albedo[0..2] = albedo, fuzz (already clamped to <=1 by the ctor, :89)
 *   DIELECTRIC ir
 *   LIGHT      albedoTex = emit texture                                        */
typedef struct SrtMaterialIn {
  int32_t type;
  int32_t albedoTex, normalTex, metallicTex, roughnessTex;
  float albedo[4];
  float metalness, roughness;
  float fuzz, ir;
  int32_t pad[3];
} SrtMaterialIn;

/* texture.h.  IMAGE: width*height*bpp bytes at texels + texelOffset, row
 * stride bpp*width (texture.h:122); width==0 means "failed to load" and
 * samples as (1,0,1) (texture.h:130-131).  CHECKER: even/odd are texture
 * ids of SOLID or IMAGE textures (texture.h:37-40). */
typedef struct SrtTextureIn {
  int32_t kind;
  int32_t width, height, bpp;
  int64_t texelOffset;
  int32_t even, odd;
  float color[3];
  int32_t pad;
} SrtTextureIn;

typedef struct SrtSceneDesc {
  int32_t numTriangles;
  const SrtTriangleIn* triangles;
  int32_t numSpheres;
  const SrtSphereIn* spheres;
  int32_t numPrims;
  const SrtPrimRef* prims; /* list order: decides BVH sort ties */
  int32_t numWorld;
  const SrtWorldItem* world;
  int32_t numMaterials;
  const SrtMaterialIn* materials;
  int32_t numTextures;
  const SrtTextureIn* textures;
  int64_t numTexelBytes;
  const uint8_t* texels;
} SrtSceneDesc;

/* camera.h:10-38 ctor arguments, and the members the ctor derives. */
typedef struct SrtCameraParams {
  float eye[3], lookAt[3], up[3];
  float vfovDegrees, aspect, aperture, focusDist, time0, time1;
} SrtCameraParams;

typedef struct SrtCamera {
  float origin[3], lleft[3], horizontal[3], vertical[3];
  float w[3], hor[3], vert[3];
  float lensRadius, time0, time1;
} SrtCamera;

/* ------------------------------------------------------ flattened BVH (out) */
/* 32 bytes: one node visit = two 16-byte loads.  child >= 0: node index in
 * the same array; child < 0: primitive, ~child = index into prims[]. */
typedef struct SrtBvhNode {
  float bmin[3];
  int32_t left;
  float bmax[3];
  int32_t right;
} SrtBvhNode;

/* ----------------------------------------------------------- fixed ray set */
typedef struct SrtRay {
  float o[3];
  float d[3];
  float time;
  float tMin, tMax;
} SrtRay;

/* hitRecord (hittable.h:9-22) plus what the reference never records: the
 * primitive id (index into prims[]) and traversal counters. */
typedef struct SrtHit {
  int32_t prim; /* SRT_NO_HIT on miss */
  float t;
  float p[3];
  float normal[3], tangent[3], bitangent[3];
  float uv[2];
  int32_t frontFace;
  int32_t material;
  int32_t nodeVisits, boxPasses, triTests, sphereTests;
} SrtHit;

/* ----------------------------------------------------------------- render */
typedef struct SrtRenderParams {
  int32_t imageWidth, imageHeight;
  int32_t spp;       /* numSamples, main.cpp:178 */
  int32_t maxBounce; /* main.cpp:180 */
  uint64_t seed;     /* counter RNG key; see DESIGN.md "RNG" */
  float background[3]; /* main.cpp:170 */
  float tMin;          /* 0.001f, main.cpp:39 */
  int32_t traversal;   /* SRT_TRAVERSE_* */
  /* multi-GPU tile split: this call renders tiles tileFirst, tileFirst+tileStride, ... */
  int32_t tileFirst, tileStride;
  /* One work item = one pixel x one chunk of its samples.  Samples are summed in index order inside a
   * chunk (a float running sum, main.cpp:217).  1 = a single running sum per pixel, the reference's order
   * (main.cpp:204-218), bit-reproducible against the oracle.  > 1: the chunks' float sums are added EXACTLY
   * (64-bit fixed point with 2^-36 resolution) and rounded to float once, so the pixel sum does not depend on
   * the order in which chunks finish, on the tile split or on the GPU count; it differs from the single
   * running sum only by the re-association of the float sum (<= 2e-5 relative), and a chunk sum of
   * 2^26 / (chunk count rounded up to a power of two) or more counts as infinite (the pixel is white either
   * way).  Device memory held by the context until srtDestroy: 16 bytes per pixel PER CHUNK of this rank's
   * tiles (one slot per work item, summed by a second kernel) while that fits a budget -- the smaller of
   * 12 GiB (tunable chunk_scratch_mb) and a quarter of the free device memory --, otherwise, or when that
   * allocation fails, 32 bytes per pixel whatever the chunk count (64-bit integer atomics, 0.4-1 % slower);
   * both give the same bits.  0 = library default, srtPlanSppChunks(width, height, spp, 0) (fastest). */
  int32_t sppChunks;
  int32_t countStats; /* 1: run the counting variant and fill srtGetStats() */
  /* progressive rendering: this call renders samples [sampleFirst, sampleFirst + spp) of every
   * pixel (RNG keys use the absolute sample index), so passes can be added up, checkpointed and
   * resumed; the reference only writes once at the very end (main.cpp:235-237). */
  int32_t sampleFirst;
} SrtRenderParams;

/* counters behind the algorithmic-bytes figure */
typedef struct SrtStats {
  uint64_t samples, rays;
  uint64_t nodeVisits, boxPasses, triTests, sphereTests;
  uint64_t shadedTriHits, texelFetches;
  /* wave-scheduler profile of the step-scheduler kernel's counting variant (diagnostics, not part of any parity claim):
   * shader clocks spent in, executions of, and lanes active in each step kind, summed over waves.  Zero after a counting
   * launch of the path-pool kernel (srtGetLaunchInfo mode 3 or 4; tunable "wavefront" = 0 selects the step scheduler) */
  uint64_t cyclesNode, cyclesPrim, cyclesShade, cyclesTotal;
  uint64_t stepsNode, stepsPrim, stepsShade;
  uint64_t lanesNode, lanesPrim, lanesShade;
} SrtStats;

typedef struct SrtContext SrtContext;

/* ------------------------------------------------------------ entry points */

/* replaces glDevice::init's context part (gl.h:194-215). */
int srtCreate(int deviceOrdinal, SrtContext** out);
/* replaces glDevice::terminate (gl.h:322-324). */
int srtDestroy(SrtContext* ctx);
const char* srtLastError(const SrtContext* ctx);

/* Host helper: camera ctor arithmetic, camera.h:10-38 (double tan, etc). */
int srtMakeCamera(const SrtCameraParams* in, SrtCamera* out);

/* The process-global default-seeded mt19937 the reference draws everything
 * from (globals.h:30-35).  The BVH builder consumes it exactly as
 * bvh.h:60 does; scene code may use it as randomFloat(). */
float srtHostRandomFloat(void);
void srtHostRandomReset(void);

/* replaces hittableVector::build + the SSBO upload (hittablevector.h:27-31,
 * gl.h:240-262): builds every SRT_WORLD_BVH with bvh.h:55-95 semantics,
 * precomputes per-triangle constants, copies everything to HBM.
 * Device memory: 32 B per node, 112 B per triangle, 48 B per sphere, the texels; trees too large for a compute
 * unit's LDS (more than about 4 500 nodes) get a second, threaded copy of the node array for the render kernel
 * that keeps their top in LDS: +32 B per node, +8 B per primitive. */
int srtUploadScene(SrtContext* ctx, const SrtSceneDesc* scene);
int srtSetCamera(SrtContext* ctx, const SrtCamera* cam);

/* Host-only (no GPU needed): the bvhNode build of world item `item`, exactly as
 * srtUploadScene performs it.  out may be NULL to query the node count. */
int srtBuildBvh(const SrtSceneDesc* scene, int32_t item, SrtBvhNode* out, int32_t capacity, int32_t* count,
                int32_t* stackDepth);

/* Flattened tree of world item `item` (host copy), for topology parity tests.
 * Call with nodes == NULL to get the count. */
int srtGetBvh(SrtContext* ctx, int32_t item, SrtBvhNode* nodes, int32_t capacity, int32_t* count);
int srtGetBvhDepth(SrtContext* ctx, int32_t* depth);

/* Tiles: the image is cut into 8x8-pixel tiles.  Tiles are numbered along a blocked curve: the tile
 * grid is cut into SRT_TILE_BLOCK x SRT_TILE_BLOCK blocks (edge blocks smaller), blocks row-major,
 * tiles row-major inside a block with row iy rotated by iy, so that tiles issued together form a
 * compact 2-D patch (coherent rays) and a rank's tiles do not line up in columns.  Positions of
 * this order are the unit of the multi-GPU split (rank r of N renders positions r, r+N, ...)
 * and of the output layout ([local position][64 pixels] float4); inside the kernel lanes pull
 * (pixel, sample chunk) work items.  srtResolveTiles undoes the order; callers never need it
 * (host mirror for tests: sexy-raytracer_amd/tiles.py).
 * srtNumLocalTiles gives the (rank-padded) tile count of one rank: ceil(numTiles / tileStride). */
int32_t srtNumTiles(int32_t imageWidth, int32_t imageHeight);
int32_t srtNumLocalTiles(int32_t imageWidth, int32_t imageHeight, int32_t tileStride);

int32_t srtDefaultSppChunks(int32_t spp);
/* The chunk count a render will use: sppChunks itself when > 0 (-1 if that many chunk slots over the whole image do
 * not fit the kernels' 32-bit work-item index: srtRenderTiles then fails), else srtDefaultSppChunks(spp), lowered only
 * for images beyond ~3 Mpixels.  A function of the image size and the sample count alone -- never of the tile split --
 * so that every rank of every split adds the same chunks.  Host only. */
int32_t srtPlanSppChunks(int32_t imageWidth, int32_t imageHeight, int32_t spp, int32_t sppChunks);

/* The hot path.  Asynchronous on `stream` (a hipStream_t, NULL = default).
 * dAccumTiles: DEVICE pointer, float4[numLocalTiles * 64], tile-major,
 * rgb = sum over samples of rayColor, a = sample count. */
int srtRenderTiles(SrtContext* ctx, const SrtRenderParams* p, void* dAccumTiles, void* stream);

/* Per-pixel sample moments: srtRenderTiles with a second plane that carries the luminance moments of the samples, the
 * per-pixel noise estimate a denoiser needs (srtDenoiseMoments) and a convergence check can use.
 * dAccumTiles comes out bit-identical to srtRenderTiles with the same parameters (any kernel form, chunk-sum path or tile
 * split).  dMomentTiles: DEVICE float4[numLocalTiles * 64] in the beauty tiles' layout and split:
 *   x = sum over the samples of l_s, y = sum of l_s * l_s, z = 0, w = the sample count (the beauty's w),
 *   l_s = 0.2126f * L.r + 0.7152f * L.g + 0.0722f * L.b of sample s's rayColor L, evaluated left to right in float.
 * Sums follow the beauty's rules channel by channel: a float running sum in sample-index order inside a work item, the exact
 * 2^-36 fixed-point sum of the chunk partials when sppChunks > 1 (independent of the tile split, the chunk-sum path and
 * the order in which chunks finish), NaN / infinite samples poison x and y as they poison rgb, and a chunk partial at or
 * beyond the fixed-point limit (SrtRenderParams.sppChunks) counts as +inf -- y, a sum of squares, reaches that limit long
 * before rgb does (a chunk whose mean luminance exceeds sqrt(limit / samples in the chunk)).
 * srtGatherTiles and srtResolveTiles(..., dRgba = NULL, dAccumImage) work on the moments plane unchanged.
 * The launch runs the same kernel form with the same grid, block and LDS as srtRenderTiles (srtLastKernelMs and
 * srtGetLaunchInfo describe it); it ignores the wf_profile tunable and leaves srtGetStats as it was.  countStats = 1 is an
 * error, as is a NULL dMomentTiles (no kernel launched).  Device memory held by the context: the chunk scratch of
 * SrtRenderParams.sppChunks doubles -- 32 bytes per pixel per chunk on the scratch path (which the moments launch takes
 * while twice the slots fit the same budget), 64 bytes per pixel on the atomic path.
 * srtRenderImageMoments: the blocking form, whole image, HOST buffers: hAccum / hRgba bit-identical to srtRenderImage,
 * hMoments = float[W*H*4] in image order (sums with counts, not means); each may be NULL. */
int srtRenderTilesMoments(SrtContext* ctx, const SrtRenderParams* p, void* dAccumTiles, void* dMomentTiles, void* stream);
int srtRenderImageMoments(SrtContext* ctx, const SrtRenderParams* p, float* hAccum, float* hMoments, uint8_t* hRgba);

/* color.h:25-41 (writeColorTarget) over a gathered, rank-major tile buffer
 * float4[tileStride][numLocalTiles*64]: un-permutes tiles into image order.
 * dRgba: DEVICE uint8[W*H*4] or NULL; dAccumImage: DEVICE float4[W*H] or NULL. */
int srtResolveTiles(SrtContext* ctx, const SrtRenderParams* p, const void* dGatheredTiles,
                    void* dRgba, void* dAccumImage, void* stream);

/* Feature pass: the guide images of a denoiser, sample-aligned with the beauty render.
 * Same SrtRenderParams as srtRenderTiles (size, spp, sampleFirst, seed, background, tMin, traversal, tileFirst,
 * tileStride); maxBounce, sppChunks and countStats are ignored.  For every pixel and every sample s in
 * [sampleFirst, sampleFirst + spp) the pass traces EXACTLY the camera ray the beauty render traces for that sample (same
 * counter RNG key (seed, pixel, s), same draw order u, v, lens disk, time) with the requested traversal and takes the
 * first hit's hit record.  Per sample:
 *   SRT_FEATURE_ALBEDO    every sample counts; a miss gives `background`.  pbr: base * albedo factor, base = the albedo
 *                         map's value / 255 when one is set, else the albedo factor (so squared: the colour that scales
 *                         the reference's diffuse term, material.h:156-245); metal: albedo; dielectric: (1, 1, 1);
 *                         diffuseLight: the emitted colour clamped to [0, 1] per channel
 *   SRT_FEATURE_NORMAL    hits: the normal the material's scatter uses (pbr with a normal map: the mapped normal,
 *                         else the hit record's normal after setFaceNormal)
 *   SRT_FEATURE_POSITION  hits: the hit point
 *   SRT_FEATURE_DEPTH     hits: (t, t*t, 0), t in units of the (unnormalised) camera ray direction
 * Texture lookups are the render kernels' own (failed loads, the 1-bpp quirk and checkers behave as in a render).
 * Output per selected plane: float4[numLocalTiles * 64] in the beauty tiles' layout and split, xyz = the float running
 * sum of the samples that count in sample-index order, w = how many counted.  srtGatherTiles and
 * srtResolveTiles(..., dRgba = NULL, dAccumImage) work on these planes unchanged.
 * A feature pass leaves what a later render reads untouched: tunables, the host generator, the chunk scratch, and
 * srtLastKernelMs / srtGetLaunchInfo, which keep describing the last srtRenderTiles launch.
 *   srtRenderFeatureTiles  asynchronous on `stream`; dPlanes[k] = DEVICE float4[numLocalTiles*64] for every selected
 *                          bit 1 << k, ignored otherwise
 *   srtRenderFeatureImage  blocking, whole image; hPlanes[k] = HOST float[W*H*4] in image order for every selected bit:
 *                          xyz = sum / w (0 where w == 0), w = count */
enum { SRT_FEATURE_ALBEDO = 1, SRT_FEATURE_NORMAL = 2, SRT_FEATURE_POSITION = 4, SRT_FEATURE_DEPTH = 8 };
#define SRT_FEATURE_ALL 15
int srtRenderFeatureTiles(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, void* const dPlanes[4], void* stream);
int srtRenderFeatureImage(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, float* const hPlanes[4]);

/* Feature pass over a tile list: the planes above for the listed tiles only, written straight into IMAGE-ORDER planes.
 * dTileList = DEVICE uint32[numListed], entry i = tx | ty << 16, the tile whose pixels are x in [8 tx, 8 tx + 8), y in
 * [8 ty, 8 ty + 8) (the format of the adaptive rounds' lists; any order).  dPlaneImages[k] = DEVICE float4[W*H] for every
 * selected bit 1 << k, ignored (may be NULL) otherwise.  For every in-image pixel i = y W + x of a listed tile and every
 * selected plane, with F = {xyz = the float running sum over the samples [sampleFirst, sampleFirst + spp) that count, in
 * sample-index order starting from 0; w = how many counted} -- exactly the record srtRenderFeatureTiles forms for that pixel:
 *   accumulate == 0:  plane[i] = F
 *   accumulate != 0:  plane[i] = {plane[i].x + F.x, plane[i].y + F.y, plane[i].z + F.z, plane[i].w + F.w}, one float add per
 *                     channel
 * Pixels of tiles that are not listed, and the padding of edge tiles (x >= W or y >= H), are neither read nor written.  An
 * entry with tx >= ceil(W / 8) or ty >= ceil(H / 8) is skipped whole.  A tile listed twice is a caller error (its two passes
 * race).  The full tile table with accumulate == 0 equals srtRenderFeatureTiles + srtResolveTiles(..., dAccumImage) bit for
 * bit.  Asynchronous on `stream`: one kernel and the memset of its counter; numListed == 0 returns 0 and launches nothing.
 * Errors (non-zero, message in srtLastError, nothing launched): what srtRenderFeatureTiles rejects, tileFirst != 0 or
 * tileStride != 1, numListed < 0 or > srtNumTiles, a NULL list with numListed > 0.  Side effects are the feature pass's: none
 * on the tunables, the host generator, the chunk scratch, srtLastKernelMs or srtGetLaunchInfo.  Device memory: nothing beyond
 * the feature pass's counter. */
int srtRenderFeatureTileList(SrtContext* ctx, const SrtRenderParams* p, int32_t planes, const void* dTileList, int32_t numListed,
                             void* const dPlaneImages[4], int32_t accumulate, void* stream);

/* Denoiser: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) in the spatial form of SVGF, guided by the
 * feature planes' normals and depths, luminance-stopped by a variance estimate carried from level to level, optionally
 * demodulated by albedo.  It works on one frame; the temporal part is srtTemporalAccumulate below, which feeds it buffers in
 * the same formats.  fp32 throughout.
 *
 * Inputs, every buffer image-order float4[W*H] as srtResolveTiles(..., dAccumImage) writes it: dBeauty = rgb sums, w = the
 * sample count; dPlanes[k] = the resolved feature plane of bit 1 << k (sums with counts).  NORMAL and DEPTH are required,
 * ALBEDO only when demodulating, POSITION is ignored.  Means are a float division, sum / count (0 where count == 0), as
 * srtRenderFeatureImage takes them.  Per pixel p:
 *   c_p = beauty.rgb / n; p is VALID if n > 0 and all three channels are finite
 *   a~_p = max(albedo mean, 1e-3) per channel when demodulating, else 1;  e_p = c_p / a~_p;
 *   l_p = 0.2126 e.r + 0.7152 e.g + 0.0722 e.b
 *   p is a HIT if the normal plane's count is > 0: n_p = the mean normal normalised (0 if its length is 0), z_p = the
 *   depth plane's mean x (t).  Depth gradient (zx, zy): per axis the one-sided difference to a hit neighbour with the
 *   smaller magnitude (a tie takes the backward one); 0 when no neighbour on that axis is a hit
 *   edge weights between p and q at pixel offset D (step included):
 *     w_n = max(0, n_p.n_q)^sigmaN if both are hits, 1 if both are misses, 0 otherwise
 *     a_z = |z_p - z_q| / (sigmaZ |zx D.x + zy D.y| + 1e-3 z_p) if both are hits, else 0
 *   level-0 variance: v_p = max(0, mu2 - mu1^2) over the valid pixels q of the 7x7 window, mu1 and mu2 the means of l
 *     and l^2 weighted by w_n exp(-a_z) at step 1 (0 when those weights sum to 0)
 *   level i = 0 .. iterations-1, step s = 2^i: the taps q = p + s (dx, dy), dx, dy in -2..2, inside the image and valid,
 *     w = h[dx] h[dy] exp(sigmaN ln(n_p.n_q) - a_z - a_l), h = [1, 4, 6, 4, 1] / 16 (w = 0 where w_n = 0; between two
 *     misses the normal and depth terms are 1), a_l = |l_p - l_q| / (sigmaL sqrt(g_p) + 1e-10), g_p = the 3x3
 *     [1, 2, 1]/4 blur of v around p (taps outside the image dropped, the rest renormalised); a_l = 0 for a centre that
 *     is not valid.  e'_p = sum w e_q / sum w, v'_p = sum w^2 v_q / (sum w)^2, and p becomes valid (NaN, inf and the
 *     white overflowed chunk sums are filled from their neighbours); if sum w = 0, e' = 0, v' = 0 and p stays invalid
 *   output: e' a~ after the last level (0 for a pixel still invalid)
 * Sums are taken about the centre (sum w (e_q - e_p), the moments of l about l_p; 0 for a centre that is not valid): the
 * same math, but a constant neighbourhood comes back exactly.
 * The kernel computes the exponentials as one v_exp_f32 and the normal power as one v_log_f32 per tap: it agrees with a
 * libm evaluation of these formulas within a few 1e-6 relative (measured: DESIGN.md 5.6).
 * Underflow: a tap's exponential (w_n exp(-a_z) in the level-0 variance, exp(sigmaN ln(n_p.n_q) - a_z - a_l) in a level)
 * below 2^-126, the smallest normal float, counts as 0; the products with h keep denormals.  A valid pixel never meets this
 * (its own tap has exponent 0), but a pixel that is not valid is filled only by taps whose exponentials reach 2^-126, and
 * "sum w = 0" above includes the sum of nothing but such zeros: the pixel stays invalid.  Whether an invalid pixel gets
 * filled is therefore ill-conditioned where every neighbour's weight lies near that threshold -- sigmas far from the
 * defaults, such as sigmaLuminance 1e-3 with sigmaNormal 1000: there a float and a double evaluation of these formulas
 * may fill different pixels.
 *
 * srtDenoise      DEVICE buffers, asynchronous on `stream`.  dOut (may be NULL) = float4[W*H]: rgb = the denoised mean
 *                 radiance, w = the beauty count; dRgba (may be NULL, not both) = uchar4[W*H], srtResolveTiles's
 *                 quantisation of that mean (sqrt, clamp to 0.999, x256 truncated, NaN -> 0, alpha 255).  The context holds
 *                 the scratch, SRT_DENOISE_SCRATCH_BYTES_PER_PIXEL bytes per pixel of the largest image denoised, until
 *                 srtDestroy; calls on one context share it, so they are ordered on one stream.
 * srtRenderDenoisedImage  blocking: the beauty render (hAccum is bit-identical to srtRenderImage's), the feature pass of
 *                 the same parameters, the denoiser; HOST buffers float[W*H*4], float[W*H*4] and uint8[W*H*4], each may be
 *                 NULL.
 * Errors (non-zero, message in srtLastError; no kernel launched): a missing NORMAL or DEPTH plane, demodulate without
 * ALBEDO, a size <= 0, iterations outside 0..8, a negative sigma.  Neither entry changes the tunables, the chunk scratch,
 * srtLastKernelMs or srtGetLaunchInfo beyond what the render and the feature pass of the blocking entry do. */
#define SRT_DENOISE_MAX_ITERATIONS 8
#define SRT_DENOISE_DEFAULT_ITERATIONS 5
#define SRT_DENOISE_DEFAULT_SIGMA_LUMINANCE 4.0f
#define SRT_DENOISE_DEFAULT_SIGMA_NORMAL 16.0f
#define SRT_DENOISE_DEFAULT_SIGMA_DEPTH 1.0f
#define SRT_DENOISE_SCRATCH_BYTES_PER_PIXEL 56
typedef struct SrtDenoiseParams { /* a field of 0 takes its default */
  int32_t iterations;   /* a-trous levels, step 2^i for level i: 1..8, default 5 */
  int32_t demodulate;   /* non-zero: filter beauty / albedo and multiply back (needs the ALBEDO plane) */
  float sigmaLuminance; /* default 4 */
  float sigmaNormal;    /* default 16 (128 keeps the noise of normal-mapped surfaces) */
  float sigmaDepth;     /* default 1 */
  int32_t pad[3];
} SrtDenoiseParams;
int srtDenoise(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, const void* dBeauty,
               const void* const dPlanes[4], void* dOut, void* dRgba, void* stream);
int srtRenderDenoisedImage(SrtContext* ctx, const SrtRenderParams* p, const SrtDenoiseParams* d, float* hAccum,
                           float* hDenoised, uint8_t* hRgba);

/* Sample variance: the denoiser with the level-0 variance taken from the render's own samples (srtRenderTilesMoments).
 * dMoments = the resolved moments plane, image-order float4[W*H] {S1 = sum l, S2 = sum l^2, 0, n}.  For a pixel with
 * n >= 2 and finite S1, S2
 *   v_p = max(0, S2 - S1^2 / n) / (n (n - 1)),  the subtraction in double,
 * the unbiased variance of the pixel's MEAN luminance (the units of the spatial estimate, a variance of means); when
 * demodulating it is divided by lum(a~_p)^2, a~_p the clamped albedo divisor above -- exact for grey noise, an
 * approximation otherwise.  Other pixels (n < 2, non-finite moments) keep the spatial 7x7 estimate.  Everything after
 * level 0 -- the 3x3 blur g, the w^2 propagation, the taps -- is the math above.  sigmaLuminance = 0 takes
 * SRT_DENOISE_MOMENTS_DEFAULT_SIGMA_LUMINANCE when dMoments is set.
 *   srtDenoiseMoments  as srtDenoise; dMoments == NULL: srtDenoise bit for bit
 *   srtRenderDenoisedImageMoments  as srtRenderDenoisedImage with the moments render (hAccum bit-identical to
 *                      srtRenderImage); hMoments (may be NULL) = float[W*H*4], the resolved moments plane */
#define SRT_DENOISE_MOMENTS_DEFAULT_SIGMA_LUMINANCE 4.0f
int srtDenoiseMoments(SrtContext* ctx, const SrtDenoiseParams* d, int32_t width, int32_t height, const void* dBeauty,
                      const void* const dPlanes[4], const void* dMoments, void* dOut, void* dRgba, void* stream);
int srtRenderDenoisedImageMoments(SrtContext* ctx, const SrtRenderParams* p, const SrtDenoiseParams* d, float* hAccum,
                                  float* hMoments, float* hDenoised, uint8_t* hRgba);

/* Adaptive sampling: more samples where the per-pixel sample moments (srtRenderTilesMoments) say the frame is still noisy.
 * The unit is the 8x8 tile; tiles are always rendered whole (no masking of pixels inside a tile).  n_0 = p->spp, n_r = the
 * samples every pixel of a tile still active after launch r has.
 *   round 0   the whole frame, p->spp = n_0 >= 2 samples from p->sampleFirst: exactly srtRenderTilesMoments + srtResolveTiles,
 *             so beauty and moments are bit-identical to srtRenderImageMoments(p)
 *   launch r >= 1 adds b_r = min(n_{r-1}, sppMax - n_{r-1}) samples (the count doubles: a logarithmic number of launches,
 *             each of which pays the render's tail of slow single-pixel items), samples [sampleFirst + n_{r-1},
 *             sampleFirst + n_r) of the active tiles, n_r = n_{r-1} + b_r, with the chunk plan of a full-frame render of that
 *             range: sppChunks = p->sppChunks > 0 ? min(p->sppChunks, b_r) : 0.  A listed tile's outputs are therefore
 *             bit-identical to the same tile of srtRenderTilesMoments over that range, whatever the list
 *   accumulation: after each launch its beauty and moments are added into the image-order float4 sums, one float add per
 *             channel, w included: ((pass0 + pass1) + pass2) + ... per pixel
 *   convergence of an in-image pixel after round r, in DOUBLE from its accumulated float moments S1 = x, S2 = y, n = w, in
 *             this order (no multiply-add forms):
 *               mu = S1 / n;  d = S2 - (S1 * S1) / n;  v = max(0, d) / (n * (n - 1));  limit = 4 * (thr * thr)
 *             converged iff S1 or S2 is not finite (more samples cannot repair it), or v < limit * max(mu, 2^-16).
 *             v is the variance of the mean; sqrt(v) / (2 sqrt(mu)) is the standard error of sqrt(mean), the gamma-2 value
 *             the resolve quantises: thr is a threshold in display units (1/256 = one display step), 2^-16 floors mu at one
 *             display step.  thr = +inf stops after round 0; thr = 0 refines every tile up to sppMax
 *   active set: a tile is active in launch r+1 iff it was active in launch r (every tile is in round 0), n_r < sppMax, and at
 *             least one in-image pixel of it is not converged after round r.  Convergence is sticky (a tile never comes
 *             back), so every pixel of an active tile has the same count.  The list keeps the ascending blocked-curve order of
 *             srtNumTiles (the results do not depend on it, the coherence of the rays does).  The render stops when the list
 *             is empty or n = sppMax
 *   RGBA:     srtResolveTiles's quantisation with the pixel's own count: sqrtf(c * (1.0f / w)), clamp to 0.999, x256
 *             truncated, NaN -> 0, alpha 255 (bit-identical to srtResolveTiles where every count is equal)
 *
 * srtRenderAdaptive       DEVICE image-order float4[W*H] sums with counts: dAccumImage (beauty) and dMomentsImage
 *                         ({S1, S2, 0, n}, srtRenderTilesMoments's plane), both required (the decisions read them);
 *                         dRgba = DEVICE uint8[W*H*4] or NULL.  Works on `stream`, and reads the next tile count back once
 *                         per round: it returns only after all of its work has finished.
 * srtRenderAdaptiveImage  blocking, HOST buffers float[W*H*4], float[W*H*4], uint8[W*H*4]; each may be NULL.
 * stats may be NULL in both.  Errors (non-zero, message in srtLastError; no kernel launched): spp < 2, sppMax < spp,
 * sppMax > 2^24 (counts stop being exact in float), sampleFirst + sppMax beyond int32, a negative or NaN threshold,
 * countStats != 0, tileFirst != 0 or tileStride != 1 (one GPU), NULL device buffers, and what srtRenderTiles rejects.
 * Neither entry changes the tunables or the host generator; srtLastKernelMs / srtGetLaunchInfo describe the last render
 * launch, as after any render.  Device memory held by the context until srtDestroy: SRT_ADAPTIVE_SCRATCH_BYTES_PER_PIXEL
 * bytes per pixel of the largest image (one launch's beauty and moments tiles) plus 12 bytes per tile (two tile lists and
 * the flags), besides the moments render's chunk scratch (srtRenderTilesMoments). */
#define SRT_ADAPTIVE_MAX_ROUNDS 32
#define SRT_ADAPTIVE_MAX_SPP (1 << 24)
#define SRT_ADAPTIVE_SCRATCH_BYTES_PER_PIXEL 32
typedef struct SrtAdaptiveParams {
  int32_t sppMax;  /* samples a pixel gets at most, >= spp */
  float threshold; /* thr: the standard error of the displayed (gamma-2) value a pixel must get below, in [0, +inf] */
  int32_t pad[2];
} SrtAdaptiveParams;
typedef struct SrtAdaptiveStats {
  int32_t rounds;                              /* launches, round 0 included */
  int32_t pad;
  int64_t pixelSamples;                        /* sum of w over the in-image pixels */
  int32_t roundSpp[SRT_ADAPTIVE_MAX_ROUNDS];   /* b_r (round 0: n_0) */
  int32_t roundTiles[SRT_ADAPTIVE_MAX_ROUNDS]; /* tiles launch r rendered (round 0: srtNumTiles) */
  float roundMs[SRT_ADAPTIVE_MAX_ROUNDS];      /* render kernel time of launch r (srtLastKernelMs of it) */
} SrtAdaptiveStats;
int srtRenderAdaptive(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, void* dAccumImage,
                      void* dMomentsImage, void* dRgba, SrtAdaptiveStats* stats, void* stream);
int srtRenderAdaptiveImage(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, float* hAccum,
                           float* hMoments, uint8_t* hRgba, SrtAdaptiveStats* stats);

/* Adaptive sampling with guide planes from every sample: srtRenderAdaptive whose feature planes follow the rounds.  After
 * launch r the same tile list and the same sample range [sampleFirst + n_{r-1}, sampleFirst + n_r) go through
 * srtRenderFeatureTileList: round 0 over the whole frame with accumulate = 0, launch r >= 1 over its list with accumulate = 1.
 *   planes    image-order sums with per-pixel counts, ((pass0 + pass1) + pass2) + ... per pixel and channel, as the beauty;
 *             round 0 equals srtRenderFeatureTiles + srtResolveTiles of p bit for bit, so threshold = +inf or sppMax == spp
 *             gives the plain feature sums of p.  ALBEDO's w (every sample counts) equals the beauty's w on every pixel
 *   beauty, moments, RGBA, stats and the decisions are srtRenderAdaptive's bit for bit: the planes are never read
 * srtRenderAdaptiveGuided         planes / dPlaneImages as srtRenderFeatureTileList (any non-empty subset), the rest as
 *                                 srtRenderAdaptive; returns after all of its work has finished.
 * srtRenderAdaptiveDenoisedImage  blocking, HOST buffers, each may be NULL: srtRenderAdaptiveGuided with all four planes, then
 *                                 srtDenoiseMoments (parameters d) on its sums, moments and planes.  hAccum, hMoments as
 *                                 srtRenderAdaptiveImage; hDenoised (rgb = the denoised mean, w = the pixel's count) and hRgba
 *                                 (of the denoised mean) as srtRenderDenoisedImageMoments, which threshold = +inf reproduces
 *                                 in every byte.
 * Errors (nothing launched): what srtRenderAdaptive, srtRenderFeatureTileList and (the image entry) srtDenoiseMoments reject.
 * Side effects as srtRenderAdaptive.  Device memory held by the context: srtRenderAdaptive's; nothing new beyond the feature
 * pass's counter. */
int srtRenderAdaptiveGuided(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, int32_t planes,
                            void* const dPlaneImages[4], void* dAccumImage, void* dMomentsImage, void* dRgba,
                            SrtAdaptiveStats* stats, void* stream);
int srtRenderAdaptiveDenoisedImage(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, const SrtDenoiseParams* d,
                                   float* hAccum, float* hMoments, float* hDenoised, uint8_t* hRgba, SrtAdaptiveStats* stats);

/* Temporal accumulation: the temporal half of SVGF (Schied et al. 2017) in front of the denoiser above.  The previous
 * frame's accumulated radiance and luminance moments are reprojected onto the current camera, kept where the surface is
 * the same, and the current frame's samples are added.  The scene is static; only the camera moves.  fp32 throughout, and
 * only + - * / sqrt, rint, floor and comparisons: the kernel agrees with a NumPy float32 evaluation of this text in this
 * operation order bit for bit (tests/temporal_ref.py), decisions included.
 *
 * Buffers, all DEVICE, image order, float4[W*H] unless said otherwise, sums with counts as srtResolveTiles(...,
 * dAccumImage) writes them: dBeauty (rgb sums, w = n); dMoments ({S1, S2, 0, n}, may be NULL); dPlanes[k] = the resolved
 * feature plane of bit 1 << k: NORMAL, POSITION and DEPTH required, ALBEDO only when demodulating.
 * A history is SRT_TEMPORAL_HISTORY_BYTES_PER_PIXEL bytes per pixel, three float4 planes one after the other:
 *   plane 0  {r, g, b, count}   accumulated radiance sums (divided by a~ when demodulating); count 0 = empty
 *   plane 1  {nx, ny, nz, S1}   the surface normal the pixel had when it was written; nx = NaN marks a miss
 *   plane 2  {Px, Py, Pz, S2}   the POSITION mean it had (0 for a miss)
 * It is caller-owned and belongs to (image size, demodulate, the scene, the camera it was written with).
 *
 * Per pixel p = (x, y), i = y W + x, with cur = the current camera, prev = the camera of the history:
 *   means       m(s, c) = s / c, 0 where c == 0.  p is a HIT if the NORMAL count is > 0.  n_p = the NORMAL mean divided by
 *               its length len = sqrt(nx nx + ny ny + nz nz) when 0 < len < inf, else 0.  tbar = m(DEPTH.x, DEPTH.w).
 *               Q_p = the POSITION mean (its own count).  a~ = max(m(ALBEDO), 1e-3) per channel and la = 0.2126 a~.r +
 *               0.7152 a~.g + 0.0722 a~.b when demodulating (the divisor of srtDenoiseMoments), else 1.
 *               p is USABLE if n > 0 and n, r, g, b (and S1, S2 when dMoments is given) are all finite
 *   ray         s_c = (x + 0.5) / (W - 1), t_c = ((H - y) + 0.5) / (H - 1): the render's own pixel mapping at the mean of
 *               its jitter.  d = ((cur.lleft + s_c cur.horizontal) + t_c cur.vertical) - cur.origin per component,
 *               dlen = sqrt(d.d) (dot products are (x x + y y) + z z everywhere)
 *   point       a hit: P = cur.origin + tbar d, v = P - prev.origin.  Depth is in units of d, and lens-offset rays meet
 *               planes parallel to the focus plane at the same parameter, so P is the centre of the pixel's footprint
 *               whatever the aperture, and it projects back onto the pixel centre when the camera has not moved (the
 *               POSITION mean, a mean over jittered samples, does not).  A miss: v = d (the sky has no parallax)
 *   projection  through prev's lens centre onto its focus plane: e = prev.origin - prev.lleft, f = e.w (the focus
 *               distance), z = -(v.w) with w = prev.w; z > 0 or there is no history (behind the camera); k = f / z;
 *               g = e + k v; s = (g.H) / (H.H), t = (g.V) / (V.V), H = prev.horizontal, V = prev.vertical;
 *               xf = s (W - 1) - 0.5, yf = (H + 0.5) - t (H - 1).  No history unless -1 < xf < W and -1 < yf < H
 *   snap        xr = rint(xf), yr = rint(yf) (ties to even).  If |xf - xr| <= SRT_TEMPORAL_SNAP and |yf - yr| <=
 *               SRT_TEMPORAL_SNAP there is one tap (xr, yr) of weight 1
 *   taps        otherwise x0 = floor(xf), fx = xf - x0 (y alike) and the taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1),
 *               in this order, with weights (1-fx)(1-fy), fx (1-fy), (1-fx) fy, fx fy.  A tap q is ACCEPTED iff its weight
 *               is > 0, it lies inside the image, its history count c is > 0 and finite, it is a hit iff p is, and for
 *               hits  n_p . n_q >= normalCos  and  |(Q_q - P) . n_p| <= (planeDist tbar) dlen  (n_q, Q_q from the history).
 *               Rejected taps are never read into a sum: a NaN in one cannot reach the output
 *   history     wsum = the accepted weights added in tap order; each accepted tap adds (w / wsum) times its r, g, b,
 *               count, S1, S2 to the reprojected history h, in tap order from 0.  If h.count > maxHistory: r, g, b, S1,
 *               S2 are multiplied by maxHistory / h.count and h.count = maxHistory (an exponential moving average with
 *               weight n / (n + maxHistory) for the new frame)
 *   output      no accepted tap: dBeautyOut = the current pixel, dMomentsOut = {S1, S2, 0, n}, bit for bit, and the new
 *               history is the current pixel (a disocclusion starts over).  Otherwise, for a USABLE pixel,
 *                 dBeautyOut  = {cur.rgb + a~ h.rgb, n + h.count}      dMomentsOut = {S1 + la h.S1, S2 + (la la) h.S2, 0, that count}
 *                 new history = {h.rgb + cur.rgb / a~, h.count + n}, S1' = h.S1 + S1 / la, S2' = h.S2 + S2 / (la la)
 *               one float add per channel, w included -- srtRenderAdaptive's rule; the multiplications and divisions are
 *               skipped when not demodulating, so K frames from one camera are the running sum ((f0 + f1) + f2) + ...
 *               The current frame's own sums never pass through the division.  Demodulation keeps bilinear history taps
 *               from blurring textures; like srtDenoiseMoments's divisor it is exact for grey noise only.
 *               A pixel that is not USABLE (the r = 0 ground's NaN samples, overflowed chunk sums) stays what it is in
 *               dBeautyOut and dMomentsOut, for the denoiser to fill, and its new history is h alone, or empty.
 *               The new history's planes 1 and 2 always describe the current frame's surface.
 *               dMoments == NULL: S1 = S2 = 0 everywhere (dMomentsOut's x and y are 0)
 * A camera that has not moved (cur and prev agree bit for bit in origin, lleft, horizontal, vertical and w): every pixel
 * is its own history -- the one tap (x, y) of weight 1, accepted iff its count is > 0 and finite, WITHOUT the hit, normal
 * and plane tests.  The footprint is the same, so those tests could only reject on the sampling noise of a few-sample
 * feature mean (a silhouette pixel that is a hit in one frame and a miss in the next), and K frames are the running sum on
 * every pixel.
 * dHistoryIn == NULL (the first frame): every pixel takes the "no accepted tap" branch; prev is not read.
 *
 * srtTemporalAccumulate   asynchronous on `stream`, one kernel.  dBeautyOut, dMomentsOut may be NULL (not both);
 *                 dHistoryOut is required and must not be dHistoryIn; outputs must not alias inputs.
 * srtRenderTemporalFrame  blocking, HOST buffers, each may be NULL: the moments render and the feature pass (all four
 *                 planes) of `p` with the camera currently set, srtTemporalAccumulate against the history and camera the
 *                 context kept from the previous call, srtDenoiseMoments (parameters d) on the accumulated buffers, then
 *                 the context keeps the new history and the camera.  hAccum = THIS frame's sums, bit-identical to
 *                 srtRenderImage(p); hDenoised / hRgba as srtRenderDenoisedImageMoments.  The first frame after a reset
 *                 equals srtRenderDenoisedImageMoments bit for bit.  Callers advance p->sampleFirst by p->spp per frame.
 *                 The history is dropped by srtTemporalReset, by srtUploadScene, and when the image size or
 *                 t->demodulate differs from the previous call's.  Device memory held by the context until srtDestroy
 *                 or srtTemporalReset: two histories, 2 x SRT_TEMPORAL_HISTORY_BYTES_PER_PIXEL bytes per pixel.
 * Errors (non-zero, message in srtLastError, nothing launched, outputs untouched): a missing NORMAL, POSITION or DEPTH
 * plane, demodulate without ALBEDO, a size <= 0 or below 2 x 2, dHistoryOut NULL or == dHistoryIn, both outputs NULL,
 * a negative or NaN parameter, normalCos > 1.  Neither entry changes the tunables, the chunk scratch, srtLastKernelMs,
 * srtGetLaunchInfo or the host generator beyond what the render of the blocking entry does.
 *
 * SRT_TEMPORAL_SNAP: the float32 round trip pixel -> P -> the same camera -> (xf, yf) of the text above, over every
 * pixel of 1920 x 1080 for the default camera and its orbit positions at 7, 20 and 45 degrees, depths 1e-2 .. 1e4, is off
 * by at most 3.10e-3 px (at depth 1e-2; 8.5e-4 px from depth 0.1 on): x 4 = 1.24e-2, rounded up to a power of two
 * (tests/test_temporal_abi.py repeats the measurement). */
#define SRT_TEMPORAL_HISTORY_BYTES_PER_PIXEL 48
#define SRT_TEMPORAL_SNAP 0.015625f /* 2^-6 px */
#define SRT_TEMPORAL_DEFAULT_NORMAL_COS 0.5f
#define SRT_TEMPORAL_DEFAULT_PLANE_DIST 0.02f
#define SRT_TEMPORAL_DEFAULT_MAX_HISTORY 64.0f
typedef struct SrtTemporalParams { /* a field of 0 takes its default */
  float normalCos;    /* taps need n_p . n_q >= this; in (0, 1]; default 0.5 (the sweep) */
  float planeDist;    /* taps need |(Q_q - P) . n_p| <= this x the pixel's distance tbar |d|; default 0.02 */
  float maxHistory;   /* samples of history kept at most, default 64; +inf = no cap (a plain running sum) */
  int32_t demodulate; /* non-zero: the history carries radiance / albedo (needs the ALBEDO plane) */
  int32_t pad[4];
} SrtTemporalParams;
typedef struct SrtTemporalStats {
  int64_t historyPixels;   /* pixels whose output count exceeds this frame's (history accepted) */
  double meanHistoryCount; /* mean over all pixels of the new history's count (samples behind a pixel) */
} SrtTemporalStats;
int srtTemporalAccumulate(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* dBeauty,
                          const void* dMoments, const void* const dPlanes[4], const SrtCamera* cam, const SrtCamera* prevCam,
                          const void* dHistoryIn, void* dBeautyOut, void* dMomentsOut, void* dHistoryOut, void* stream);
int srtRenderTemporalFrame(SrtContext* ctx, const SrtRenderParams* p, const SrtDenoiseParams* d, const SrtTemporalParams* t,
                           float* hAccum, float* hDenoised, uint8_t* hRgba, SrtTemporalStats* stats);
int srtTemporalReset(SrtContext* ctx);

/* Temporal-adaptive frames: "Adaptive sampling" deciding on the TEMPORALLY ACCUMULATED moments.  A tile stops once its
 * reprojected history and this frame's samples together are below the display-space threshold and keeps doubling while
 * they are not -- because it has just been disoccluded (no history: the frame's own few samples decide, as in
 * srtRenderAdaptive), or because the history disagrees with the new samples (the pooled variance grows, and buys samples).
 *
 * srtTemporalAccumulate is linear in the current frame's sums and its reprojected history h does not depend on them, so h
 * is computed once per frame and every round reads it back:
 *   reprojected history  SRT_TEMPORAL_REPROJECTED_BYTES_PER_PIXEL bytes per pixel, two image-order float4 planes one after
 *             the other: plane 0 = {h.r, h.g, h.b, h.count}, plane 1 = {h.S1, h.S2, 0, has ? 1 : 0}, has = the pixel has an
 *             accepted tap; all zeros where it has none.  h is the result of the "Temporal accumulation" rules through the
 *             maxHistory cap -- ray, point, projection, snap, taps, acceptance, normalisation in tap order, the cap, and the
 *             camera-not-moved rule -- in that text's operation order, bit for bit.  It reads the NORMAL and DEPTH planes, the two cameras and the
 *             history (the POSITION mean only reaches srtTemporalAccumulate's new history); never the beauty, the moments
 *             or the ALBEDO plane: h is in the history's (demodulated) units
 *   round 0   exactly srtRenderAdaptive's: dAccumImage and dMomentsImage are bit-identical to srtRenderImageMoments(p)
 *   pooled moments after launch r, per in-image pixel with the sums so far {r, g, b, n} and {S1, S2, 0, n}: what
 *             srtTemporalAccumulate would write to dMomentsOut,
 *               M~ = {S1 + la h.S1, S2 + (la la) h.S2, 0, n + h.count}   for a USABLE pixel with has
 *               M~ = {S1, S2, 0, n}                                      otherwise
 *             la = 1 and no multiplication when not demodulating; USABLE, a~ and la as in "Temporal accumulation"
 *   convergence  srtRenderAdaptive's test in double, in its operation order, on M~ instead of the frame's own moments
 *   active set, schedule b_r = min(n_{r-1}, sppMax - n_{r-1}), chunk plans, the per-launch float add into the image-order
 *             sums and the end of the render are srtRenderAdaptive's, unchanged; n_r counts THIS frame's samples only, and
 *             every pixel of an active tile still has the same current count
 *   end       dBeautyOut, dMomentsOut and dHistoryOut are srtTemporalAccumulate of the final sums, bit for bit
 * Consequences: threshold = +inf or sppMax == spp is srtRenderImageMoments followed by srtTemporalAccumulate; dHistoryIn ==
 * NULL gives srtRenderAdaptive's sums bit for bit, stats->adaptive.roundTiles included.
 * The feature planes are those of the frame's first p->spp samples: their means guide the reprojection (and, in the frame
 * entry, the denoiser) for every tile, however many samples the tile ends with.  Extra samples get no feature pass.
 *
 * srtTemporalReproject    asynchronous on `stream`, one kernel.  dReprojected = DEVICE float4[2][W*H].  dHistoryIn == NULL:
 *                 all zeros, prevCam is not read.  Plane requirements and errors are srtTemporalAccumulate's (ALBEDO is
 *                 required when t->demodulate is set although it is not read: one rule for both entries).
 * srtRenderTemporalAdaptive  DEVICE image-order buffers, one GPU, the camera currently set as cur.  dPlanes = the resolved
 *                 feature planes of samples [p->sampleFirst, p->sampleFirst + p->spp).  dAccumImage and dMomentsImage
 *                 (required) receive this frame's sums with per-pixel counts; dBeautyOut, dMomentsOut (either may be NULL,
 *                 not both) and dHistoryOut (required, not dHistoryIn) as in srtTemporalAccumulate.  Works on `stream` and
 *                 reads the next tile count back once per round, as srtRenderAdaptive: it returns after its work has
 *                 finished.  stats (may be NULL): adaptive as srtRenderAdaptive's, pixelSamples included; temporal as
 *                 srtRenderTemporalFrame's.
 * srtRenderTemporalAdaptiveFrame  blocking, HOST buffers, each may be NULL: the feature pass of `p` (all four planes,
 *                 p->spp samples), srtRenderTemporalAdaptive against the history and camera the context kept,
 *                 srtDenoiseMoments (parameters d) on the accumulated buffers, then the context keeps the new history and
 *                 the camera: srtRenderTemporalFrame's histories, ping-pong and reset rules, so frames of both kinds may
 *                 follow one another on one context.  hAccum = THIS frame's sums with per-pixel counts; hDenoised / hRgba as
 *                 srtRenderTemporalFrame.  Callers advance p->sampleFirst by ap->sppMax per frame.
 * Errors (non-zero, message in srtLastError, nothing launched, outputs untouched): what srtRenderAdaptive rejects and what
 * srtTemporalAccumulate rejects.  Tunables, the host generator, srtLastKernelMs and srtGetLaunchInfo are left as after
 * srtRenderAdaptive.  Device memory held by the context until srtDestroy: srtRenderAdaptive's, plus
 * SRT_TEMPORAL_REPROJECTED_BYTES_PER_PIXEL bytes per pixel of the largest image. */
#define SRT_TEMPORAL_REPROJECTED_BYTES_PER_PIXEL 32
typedef struct SrtTemporalAdaptiveStats {
  SrtAdaptiveStats adaptive;
  SrtTemporalStats temporal;
} SrtTemporalAdaptiveStats;
int srtTemporalReproject(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* const dPlanes[4],
                         const SrtCamera* cam, const SrtCamera* prevCam, const void* dHistoryIn, void* dReprojected, void* stream);
int srtRenderTemporalAdaptive(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, const SrtTemporalParams* t,
                              const void* const dPlanes[4], const SrtCamera* prevCam, const void* dHistoryIn, void* dAccumImage,
                              void* dMomentsImage, void* dBeautyOut, void* dMomentsOut, void* dHistoryOut,
                              SrtTemporalAdaptiveStats* stats, void* stream);
int srtRenderTemporalAdaptiveFrame(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap, const SrtDenoiseParams* d,
                                   const SrtTemporalParams* t, float* hAccum, float* hDenoised, uint8_t* hRgba,
                                   SrtTemporalAdaptiveStats* stats);

/* Temporal-adaptive frames with guide planes from every sample: the two entries above, except that the rounds extend the
 * feature planes.  dPlanes is IN/OUT in the device form: in = the resolved planes of the first p->spp samples, as above.
 *   decisions   the reprojected history h and every round's pooled decision read the planes of the first p->spp samples, as
 *             in the unguided entries (h is computed once, before the rounds; with demodulate the decisions read a copy of
 *             the incoming ALBEDO plane).  This frame's sums, stats->adaptive.roundTiles and pixelSamples are therefore the
 *             unguided entry's bit for bit
 *   planes    after launch r >= 1 its list and sample range go through srtRenderFeatureTileList with accumulate = 1 on every
 *             non-NULL plane: out = in + pass1 + pass2 + ... in that order, per-pixel counts in w
 *   end       dBeautyOut, dMomentsOut and dHistoryOut are srtTemporalAccumulate of the final sums with the EXTENDED planes:
 *             the closing accumulation recomputes its reprojection and acceptance from the extended means (so a pixel's
 *             accepted taps may differ from the ones h had), and the new history's normal and position describe all of a
 *             tile's samples.  In the frame entry srtDenoiseMoments reads the extended planes as well
 * threshold = +inf or sppMax == spp is the unguided entry in every byte.  Guided and unguided (and uniform) frames share the
 * context's histories, ping-pong and reset rules, so they may follow one another.  Errors and side effects are the unguided
 * entries'.  Device memory: nothing new is held by the context beyond the feature pass's counter; with demodulate the
 * device entry takes 16 bytes per pixel for the ALBEDO copy and releases them before it returns. */
int srtRenderTemporalAdaptiveGuided(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap,
                                    const SrtTemporalParams* t, void* const dPlanes[4], const SrtCamera* prevCam,
                                    const void* dHistoryIn, void* dAccumImage, void* dMomentsImage, void* dBeautyOut,
                                    void* dMomentsOut, void* dHistoryOut, SrtTemporalAdaptiveStats* stats, void* stream);
int srtRenderTemporalAdaptiveGuidedFrame(SrtContext* ctx, const SrtRenderParams* p, const SrtAdaptiveParams* ap,
                                         const SrtDenoiseParams* d, const SrtTemporalParams* t, float* hAccum, float* hDenoised,
                                         uint8_t* hRgba, SrtTemporalAdaptiveStats* stats);

/* Moving geometry: the primitive records of the uploaded scene rewritten in place, then every tree refitted on the
 * device.  Topology never changes: the trees, nodeAxis, the world list, the thread links, the stack depth, srtGetBvhDepth,
 * the triangles' device order, the material tables and every primitive's material stay as srtUploadScene left them.
 *
 * srtUpdateTriangles / srtUpdateSpheres   HOST records; `first`, `count` index the uploaded SrtSceneDesc's triangles[] /
 *             spheres[].  The records are staged in device memory the context keeps and handed to the device forms on the
 *             NULL stream; the host memory may be reused when the call returns.
 * srtUpdateTrianglesDevice / srtUpdateSpheresDevice   the same records in DEVICE memory (SrtTriangleIn aligned to 16 bytes,
 *             SrtSphereIn to 4), asynchronous on `stream`: dIn must stay untouched until the stream has passed the call.
 *   taken     a triangle's positions and uvs; a sphere's centres, times and radius.  From them the device computes what
 *             srtUploadScene computes on the host, in the same operations (the geometric normal, its unit vector, the tangent
 *             basis with its f == 0 -> f += epsilon rule; the sphere's "moving" bit from center0 != center1): the records
 *             are, bit for bit, those of an upload of the same data.
 *   ignored   the `material` field.  A primitive keeps its material, so the per-material tables stay valid.
 *   errors    no scene uploaded; first < 0, count < 0 or first + count beyond the scene's count; a NULL or misaligned
 *             pointer with count > 0.  Nothing is launched or changed then.  count == 0 (in range) is a no-op.
 *   after     any update that launched: every render / feature / trace / scatter entry returns an error ("geometry was
 *             updated; call srtRefitScene ...") WITHOUT launching anything until srtRefitScene has run -- the node boxes no
 *             longer contain their primitives.  Updates may follow one another freely (ranges may overlap: stream order).
 *
 * srtRefitScene   recomputes every node box of every SRT_WORLD_BVH item -- host-built, caller-supplied, LBVH and PLOC trees
 *             alike -- from the current primitive records: a primitive's box by the reference's boundingBox rules with its
 *             item's (time0, time1), a node's box the min / max union of its children's (bottom-up, one kernel per item, no
 *             waiting; the result does not depend on the order of arrival).  Then everything derived from boxes: the
 *             closest-hit pair records, the box halves of the path-pool kernel's hybrid records (the resident set chosen at
 *             upload stays: it decides only where a record is read from), the fast-division certificate (recomputed on the
 *             device over the node boxes and the device-built items' primitive boxes: the scene is certified exactly when an
 *             upload of the moved scene would have certified it), and what srtGetBvh returns (the refit boxes, read back
 *             when asked for).  Work is issued on `stream` -- the stream the updates went to, or one ordered behind them --
 *             and has FINISHED when the call returns: it reads the certificate's flag word back.
 *   FAITHFUL  after a refit FAITHFUL traversal means: bvh.h:97-105 on the UPLOADED topology with the new boxes -- what the
 *             reference's bvhNode::hit does on a tree whose boxes were recomputed -- not what a freshly constructed bvhNode
 *             over the moved primitives would do (its median splits would sort differently).  CLOSEST results do not
 *             depend on the tree; its speed does, see srtRebuildScene / srtGetTreeCost below and DESIGN.md 5.16.
 *   history   srtRefitScene drops the context's temporal history exactly as srtUploadScene does (the next
 *             srtRenderTemporalFrame is a first frame): the reprojection assumes static surfaces.  (srtSetMotionTracking,
 *             below, keeps it.)
 *   untouched the host generator, the tunables (fast_div as read at the upload), srtGetStats, and srtLastKernelMs / srtGetLaunchInfo,
 *             which keep describing the last render.
 *   errors    no scene uploaded; a failed launch.  A scene without trees (bare primitives only) just becomes renderable.
 * Device memory held by the context from the first call on, until the next srtUploadScene or srtDestroy: 4 bytes per
 * triangle (scene index -> device index, when the upload reordered), 8 bytes per node (parent links, arrival counters), 4
 * more per node with hybrid records, and the host forms' staging (the largest update's records). */
int srtUpdateTriangles(SrtContext* ctx, int32_t first, int32_t count, const SrtTriangleIn* hTriangles);
int srtUpdateSpheres(SrtContext* ctx, int32_t first, int32_t count, const SrtSphereIn* hSpheres);
int srtUpdateTrianglesDevice(SrtContext* ctx, int32_t first, int32_t count, const void* dTriangles, void* stream);
int srtUpdateSpheresDevice(SrtContext* ctx, int32_t first, int32_t count, const void* dSpheres, void* stream);
int srtRefitScene(SrtContext* ctx, void* stream);

/* Rebuilding: srtRefitScene, except that every world item whose tree srtUploadScene built on the device (SRT_BUILDER_LBVH
 * or SRT_BUILDER_PLOC without caller-supplied nodes) gets its tree built ANEW from the current primitive records, by the
 * same builder, into the same node slots (a device-built item has max(count - 1, 1) nodes whatever its topology).  So a
 * scene can move indefinitely without leaving the device, and srtGetTreeCost tells when a rebuild is due.
 *
 * srtRebuildScene   host-built and caller-supplied trees are refitted exactly as srtRefitScene refits them (constructing
 *             the reference's tree needs the host generator and std::sort, and stays an upload).
 *   result    after the call the node records of every device-built item (boxes and reference words), nodeAxis, the pair
 *             records, srtGetBvhDepth, the stack depth the kernels size their stacks by and the fast-division certificate
 *             equal, bit for bit, what srtUploadScene of a scene description holding the current geometry leaves: updated
 *             records are an upload's bit for bit, the builders read nothing but records and the item's primitive list,
 *             and their sort keys are unique.  The depths are the maxima over the host-built trees, as the upload had
 *             them before its device builds, and the new trees': they can grow as well as shrink.
 *   radius    PLOC's search radius is the ploc_radius tunable AS READ AT THE UPLOAD (like fast_div), not its current value.
 *   derived   as after srtRefitScene, and on the new topology: the refit's parent links are made again, the pair records
 *             and the certificate are recomputed over the whole node array, srtGetBvh reads the new trees back.
 *   ordering  the work is ordered behind `stream` -- the stream the updates went to -- and has FINISHED when the call
 *             returns.  (The builders are blocking and work on the NULL stream: the call waits for `stream` first.)
 *   history   a rebuild counts exactly as a refit: it takes srtSetMotionTracking's snapshot if no update preceded it, with
 *             tracking on it keeps the temporal history and counts as one refit, with tracking off it drops the history.
 *             The motion pass reads records, not trees, so a history survives one rebuild as it survives one refit.
 *   no device-built item   srtRefitScene, in every byte of device state.
 *   no update since the last refit   the call still rebuilds; the result is the same (idempotent).
 *   untouched what srtRefitScene leaves, the ploc_radius tunable included; the primitive records and their device order.
 *   errors    no scene uploaded; a failed build or launch, after which the scene counts as updated: render entries refuse
 *             until a rebuild has succeeded.
 * Device memory: the upload keeps every device-built item's primitive list (4 bytes per primitive of those items) until
 * the next srtUploadScene or srtDestroy, whether or not a rebuild ever follows; a build's own work area is allocated and
 * freed inside the call, as at the upload.
 *
 * srtGetTreeCost   the surface-area cost of world item `item`'s tree as it stands (after the upload, a refit or a rebuild):
 *             the sum of its node boxes' areas over the root's.  A tree whose boxes a refit has inflated costs more than
 *             the tree a rebuild gives; the ratio of the two is what a caller decides by.  Blocking; a streaming reduction
 *             over the item's node records on the device (32 B per node).  Defined exactly (tests/tree_cost_ref.py
 *             evaluates this text in NumPy float64 bit for bit):
 *   node i    of the item, in node order, its float32 box widened to double: dx = (double)max.x - (double)min.x, dy, dz
 *             likewise; a_i = (dx dy + dy dz) + dz dx, IEEE double, no contraction.
 *   sum       S = the pairwise sum of a_0 .. a_(n-1) padded with +0.0 to the next power of two: level by level element k
 *             becomes x[2k] + x[2k+1].  No floating-point atomics: S does not depend on any order of arrival.
 *   result    *cost = S / a_0 (node 0 is the item's root for every builder), an IEEE double division.  A root of zero
 *             area gives what the division gives (inf or NaN), not an error.  An item of one node costs 1.
 *   errors    (*cost untouched) no scene uploaded; geometry updated and not yet refitted or rebuilt; `item` out of range
 *             or not SRT_WORLD_BVH; a NULL cost.
 *   side effects   none, beyond a work area of the context's (16 bytes per 256 nodes of the largest item asked about). */
int srtRebuildScene(SrtContext* ctx, void* stream);
int srtGetTreeCost(SrtContext* ctx, int32_t item, double* cost);

/* Motion: the temporal history kept across a refit.  Opt-in; with tracking off (the default) every entry above behaves as
 * written there, srtRefitScene dropping the history included.
 *
 * srtSetMotionTracking   a flag of the context that, like the tunables, survives srtUploadScene.  An error while the
 *             geometry is updated but not yet refitted.  Disabling releases the snapshot (and drops a history that was
 *             being kept across a refit).  While it is on:
 *   snapshot  the first srtUpdate* call that launches after an upload or a refit first copies the scene's triangle test
 *             records (48 B per triangle, device order) and sphere records (48 B per sphere) into buffers the context keeps
 *             for the scene: device to device, on that call's stream, ahead of its own kernel.  Later updates of the same
 *             epoch do not copy again (issue them on that stream or on one ordered behind it: the copy reads both tables
 *             whole), and a srtRefitScene that no update preceded copies too.  So "previous" is always
 *             the geometry as of the previous srtRefitScene, or as of the upload; before any snapshot exists it is the
 *             current geometry (all displacements are exact zeros).
 *   history   srtRefitScene keeps the context's temporal history and counts the refits since the last temporal frame.
 *   memory    48 B per triangle and 48 B per sphere from the first update (or refit) on, until the next srtUploadScene or
 *             until tracking is disabled.
 *
 * srtRenderMotionTiles   asynchronous on `stream`; the parameters, tile layout, split, checks and side effects of
 *             srtRenderFeatureTiles (none on the tunables, the host generator, the chunk scratch, srtLastKernelMs or
 *             srtGetLaunchInfo), one plane; srtGatherTiles / srtResolveTiles work on dMotionTiles unchanged.
 * srtRenderMotionImage   blocking, into HOST float[W*H*4]: xyz = sum / w (0 where w == 0), w = count, as
 *             srtRenderFeatureImage returns its planes.
 *   Per sample, in sample-index order from 0, the pass traces the beauty render's camera ray (same RNG key, same draws)
 *   with the traversal `p` asks for.  A miss does not count.  A hit at p = o + t d adds the displacement m to a float
 *   running sum and 1 to the count w (the plane's w equals the NORMAL plane's).  Only + - * / in float32, no contraction,
 *   IEEE division; dot(a, b) = a.x b.x + (a.y b.y + a.z b.z), cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z,
 *   a.x b.y - a.y b.x): tests/motion_ref.py evaluates this text in NumPy float32 bit for bit.
 *   triangle  v0, v1, v2 and n = (v1 - v0) x (v2 - v0) from the current record, v0', v1', v2' from the snapshot's:
 *             d_i = v_i' - v_i;  e0 = dot(n, cross(v1 - v0, p - v0)), e1 = dot(n, cross(v2 - v1, p - v1)),
 *             e2 = dot(n, cross(v0 - v2, p - v2)) (the hit test's edge values; they weigh v2, v0 and v1);
 *             s = (e0 + e1) + e2;  b0 = e1 / s, b1 = e2 / s, b2 = e0 / s;  m = (b0 d0 + b1 d1) + b2 d2 per component;
 *             m = d0 unless s > 0.
 *   sphere    c, c' = the current and the snapshot record's centre at the ray's time (the moving sphere's interpolation,
 *             each with its own times), r, r' the radii:  m = (c' - c) + ((r' / r) - 1) (p - c) per component.  A
 *             sphere's rotation is not observable and gives no motion.
 *   An unmoved primitive gives m = 0 exactly: a scene in which nothing moved has an all-zero plane.
 *   errors    (nothing launched, outputs untouched) tracking off; anything srtRenderFeatureTiles rejects; a NULL output.
 *
 * srtTemporalAccumulateMotion / srtTemporalReprojectMotion   srtTemporalAccumulate / srtTemporalReproject with dMotion,
 *             the resolved motion plane in image order (DEVICE float4[W*H], sums with counts).  dMotion == NULL is the
 *             plain entry in every byte (the plain entries call these with NULL).  With dMotion the text of "Temporal
 *             accumulation" changes in exactly three places:
 *   mean      mbar = m(MOTION.xyz, MOTION.w) per component, 0 where the count is 0
 *   point     a hit: P = cur.origin + tbar d as before, P' = P + mbar per component, v = P' - prev.origin, and a tap's
 *             plane test is |(Q_q - P') . n_p| <= (planeDist tbar) dlen.  A miss: v = d, unchanged
 *   no camera-not-moved rule   every pixel goes through projection, snap, taps and acceptance even when the cameras agree
 *             bit for bit: a static pixel still snaps onto itself, and a pixel an object has just uncovered is rejected
 *             by the plane test instead of inheriting the object's radiance
 *             Everything else is as written there; a zero plane with two different cameras is srtTemporalAccumulate bit
 *             for bit.  A mean of affine images is the affine image of the mean: where all of a pixel's samples hit one
 *             rigidly or affinely moving body, mbar is that body's displacement at the POSITION mean up to rounding.
 *             Normals are not counter-rotated: the history's n_q is compared with the current n_p as it is, and the
 *             default normalCos 0.5 tolerates a rotation of 60 degrees per frame.
 *
 * srtRenderTemporalFrame with tracking on: after exactly one srtRefitScene since its last frame it also runs the motion
 * pass over `p`, resolves it and accumulates with srtTemporalAccumulateMotion against the kept history and camera.  No
 * refit: the frame as described above, byte for byte.  More than one refit: the snapshot spans only the last epoch, so the
 * history is dropped.  The temporal-adaptive frame entries drop the history after any refit, whatever the flag says. */
int srtSetMotionTracking(SrtContext* ctx, int32_t enable);
int srtRenderMotionTiles(SrtContext* ctx, const SrtRenderParams* p, void* dMotionTiles, void* stream);
int srtRenderMotionImage(SrtContext* ctx, const SrtRenderParams* p, float* hMotion);
int srtTemporalAccumulateMotion(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height, const void* dBeauty,
                                const void* dMoments, const void* const dPlanes[4], const void* dMotion, const SrtCamera* cam,
                                const SrtCamera* prevCam, const void* dHistoryIn, void* dBeautyOut, void* dMomentsOut,
                                void* dHistoryOut, void* stream);
int srtTemporalReprojectMotion(SrtContext* ctx, const SrtTemporalParams* t, int32_t width, int32_t height,
                               const void* const dPlanes[4], const void* dMotion, const SrtCamera* cam, const SrtCamera* prevCam,
                               const void* dHistoryIn, void* dReprojected, void* stream);

/* Multi-GPU: one process per GPU, the scene replicated, rank r of N renders tile positions
 * r, r+N, ... (SrtRenderParams.tileFirst / tileStride), and the path's only collective is ONE gather of the
 * ranks' equal-sized tile buffers to rank 0 over RCCL (ncclGather), after which rank 0 calls
 * srtResolveTiles.  The reference is single-device (gl.h:28-31); these entries extend its device seam.
 *   srtCommGetUniqueId  rank 0: 128 opaque bytes (an ncclUniqueId) to hand to the other ranks by the host
 *                       program's own means (file, MPI, a launcher's key-value store)
 *   srtCommInit         every rank: joins the communicator (collective: returns when all ranks have)
 *   srtGatherTiles      every rank: dLocalTiles = float4[numLocalTiles*64] (DEVICE); rank 0 also passes
 *                       dGathered = float4[numRanks][numLocalTiles*64] (DEVICE), others NULL.
 *                       Asynchronous on `stream`.  With one rank it degenerates to a device copy.
 *   srtRenderImageRanks the blocking main.cpp:182-227 form across the ranks (collective): render own tiles,
 *                       the one gather, rank 0 resolves into its caller-owned HOST buffers.  Before the gather the
 *                       ranks agree (a 4-byte all-reduce) that every one of them rendered: if one failed, ALL return
 *                       non-zero together instead of some waiting in the gather.  A rank that is lost altogether
 *                       leaves its peers in a collective: they then need srtCommDestroy (ncclCommAbort semantics).
 *   srtCommDestroy      also done by srtDestroy */
#define SRT_COMM_ID_BYTES 128
int srtCommGetUniqueId(void* id128);
int srtCommInit(SrtContext* ctx, const void* id128, int32_t numRanks, int32_t rank);
int srtGatherTiles(SrtContext* ctx, const SrtRenderParams* p, const void* dLocalTiles, void* dGathered, void* stream);
int srtRenderImageRanks(SrtContext* ctx, const SrtRenderParams* p, float* hAccum, uint8_t* hRgba);
int srtCommDestroy(SrtContext* ctx);

/* Blocking convenience with caller-owned HOST buffers: the main.cpp:182,224
 * `target` contract.  hAccum (float[W*H*4]) and hRgba (uint8[W*H*4]) may be NULL. */
int srtRenderImage(SrtContext* ctx, const SrtRenderParams* p, float* hAccum, uint8_t* hRgba);

/* Fixed-ray-set parity entry: world.hit(r, tMin, tMax, rec) for n rays. HOST pointers. */
int srtTraceRays(SrtContext* ctx, const SrtRay* rays, int64_t n, SrtHit* hits, int32_t traversal);

/* Ray queries: rays that sit in DEVICE memory -- written by a kernel or a torch op -- answered in DEVICE memory against
 * the uploaded scene, on the caller's stream.  (srtTraceRays above stays the parity entry: host pointers, a device round
 * trip per call, traversal counters.)
 *
 * srtTraceRaysDevice   the closest (or the reference's) hit of every ray.
 * srtOccludedDevice    whether anything at all is hit ("any hit"): shadow, visibility and ambient-occlusion rays.
 *   buffers   all DEVICE pointers.  dRays = SrtRay[n], aligned to 4 bytes (36 bytes each: a contiguous (n, 9) float32
 *             tensor).  dHits = SrtRayHit[n], aligned to 16 bytes, may be NULL.  dRecords = SrtHit[n], aligned to 4 bytes,
 *             may be NULL (not both): the full record as srtTraceRays fills it, its four counter fields written as 0.
 *             dOccluded = uint8_t[n], 0 / 1.  Output elements at index >= n are never written.
 *   async     both are asynchronous on `stream`, allocate nothing, do not synchronise and touch no scratch of the
 *             context's: one kernel.  The buffers must stay untouched until the stream has passed the call.  They read
 *             the trees as they stand: after the upload, a refit or a rebuild.
 *   untouched the tunables, the host generator, the chunk scratch, srtLastKernelMs, srtGetLaunchInfo, srtGetStats, the
 *             temporal history.
 *   n == 0    returns 0 and launches nothing.
 *   FAITHFUL  traversal == SRT_TRAVERSE_FAITHFUL: world.hit(r, tMin, tMax, rec) in the reference's order, exactly what
 *             srtTraceRays returns for FAITHFUL -- every field bit for bit, except the counters, which are 0.
 *   CLOSEST   traversal == SRT_TRAVERSE_CLOSEST: the tree-independent closest hit.  Every primitive has a CANDIDATE t for
 *             the ray's (tMin, tMax): a triangle's t when the triangle test accepts it (model.h:104-154, and t <= tMax,
 *             which the reference does not ask); a sphere's root as sphere.h:54-73 chooses it.  The result is the
 *             candidate of smallest t (float <); among equal t the primitive with the LARGEST prims[] index wins.  That
 *             is what a loop over prims[] in list order that keeps `t <= closest` returns, so the answer does not depend
 *             on the builder, on a refit or on a rebuild.  A hit with t == tMax is a hit.
 *   occluded  occluded[i] = 1 iff at least one primitive has a candidate for (tMin, tMax) in the CLOSEST sense: the
 *             CLOSEST query's prim != SRT_NO_HIT, whatever order the tree is walked in.
 *   one-sided triangles are hit from their front only, as in every render of this library (model.h:119-123): a ray that
 *             meets a triangle's back passes through, for the closest hit and for occlusion alike.
 *   condition the ray's `time` lies inside [time0, time1] of every world item (a box bounds a moving sphere only over its
 *             item's range: the reference's own contract); o is finite, d is finite and non-zero.  Otherwise the result
 *             is unspecified, but the call still terminates and writes element i only.
 *   errors    (non-zero, message in srtLastError, NOTHING launched, outputs untouched; all decided on the host) no scene
 *             uploaded; geometry updated and not yet refitted; n < 0; with n > 0 a NULL dRays, no output buffer or a
 *             misaligned pointer; a traversal that is neither value; a tree so deep that the per-lane stacks of a
 *             workgroup exceed 160 KB of LDS (1 KB per pending reference: a depth beyond 158). */
typedef struct SrtRayHit { /* 16 bytes per ray, one dwordx4 store */
  int32_t prim;            /* index into prims[], SRT_NO_HIT on a miss */
  float t;                 /* 0 on a miss */
  int32_t material;        /* -1 on a miss */
  int32_t frontFace;       /* 0 / 1; 0 on a miss */
} SrtRayHit;
int srtTraceRaysDevice(SrtContext* ctx, const void* dRays, int64_t n, int32_t traversal, void* dHits, void* dRecords,
                       void* stream);
int srtOccludedDevice(SrtContext* ctx, const void* dRays, int64_t n, void* dOccluded, void* stream);

/* Path steps on device buffers: the pieces of the render's per-sample loop on the caller's DEVICE buffers and stream --
 * the camera ray of a (pixel, sample), the shading of a hit record, and the two halves of a bounce fused into one kernel
 * -- with the counter RNG's state as a value the caller carries.  A loop over them in user land (below) is the library's
 * path tracer, and reproduces srtRenderImage bit for bit.
 *
 * srtRngKey             (host only) the state a render gives (pixel, sample) before its first draw:
 *                       mix64(mix64(seed) ^ (pixel << 32 | sample)), mix64 = the splitmix64 finaliser.  pixel and sample
 *                       are the renders' 32-bit indices; they are passed as uint64_t and only their low 32 bits are
 *                       used.  Callers seed streams of their own with it.
 * srtCameraRaysDevice   the camera ray of every (pixel, sample) entry, and the state after its draws.
 * srtScatterRaysDevice  material::scatter + material::emitted on every hit record (what srtScatterRays evaluates).
 * srtPathStepDevice     srtTraceRaysDevice followed by srtScatterRaysDevice in ONE kernel: the form a loop should call (a
 *                       path does not write an 88-byte SrtHit to memory and read it back between the two halves).
 * srtCompactPathsDevice the entries that scattered, moved to the front between two steps (its own block below).
 * srtSortPathsDevice    the same entries, ordered by origin cell and direction octant (its own block below).
 * srtTracePathsDevice   the whole loop in one kernel: the radiance of one path per ray (its own block below).
 *   buffers  all DEVICE pointers.  dRays, dRaysOut = SrtRay[n], aligned to 4 bytes.  dRng = uint64_t[n], aligned to 8:
 *             entry i is the generator state of path i (a PCG32 state: one 64-bit LCG step and an XSH-RR output per 32-bit
 *             draw; a float draw is float(u32) * 2^-32, clamped below 1).  Each entry reads it, advances it by exactly the
 *             draws its work makes, and writes it back.  dOut = SrtPathOut[n], aligned to 16.  dRecords = SrtHit[n],
 *             aligned to 4, as srtTraceRaysDevice(..., dRecords) writes it (the counters are ignored).  dHits =
 *             SrtRayHit[n], aligned to 16, may be NULL.  dActive = uint8_t[n], may be NULL.  dPixelSample = int32_t[n][2],
 *             aligned to 4, may be NULL.  Elements at index >= n are never written.
 *   async     all three are asynchronous on `stream`, allocate nothing, do not synchronise and touch no scratch of the
 *             context's: one kernel each.  The buffers must stay untouched until the stream has passed the call.
 *   untouched the tunables, the host generator, the chunk scratch, srtLastKernelMs, srtGetLaunchInfo, srtGetStats, the
 *             temporal history.
 *   n == 0    returns 0 and launches nothing.
 *   camera    dPixelSample[i] = {pixel index y * W + x, absolute sample index}.  With NULL, n must be W * H * p->spp and
 *             entry i is pixel i / spp, sample p->sampleFirst + i % spp.  Per entry, in this order: the state is keyed
 *             srtRngKey(p->seed, pixel, sample); r1 is drawn, u = (x + r1) / (W - 1); r2 is drawn,
 *             v = ((H - y) + r2) / (H - 1) (main.cpp:210-211); camera::getRay(u, v) (camera.h:40-46) of the camera set with
 *             srtSetCamera draws the lens disk (y, then x, repeated while x*x + y*y >= 1) and then the time.  Written:
 *             dRays[i] = {o, d, time, tMin = p->tMin, tMax = +inf} and dRng[i] = the state after those draws.  That is the
 *             ray the beauty render, the feature pass and the motion pass trace for that sample, bit for bit.  An entry
 *             whose pixel index lies outside [0, W * H) is left unwritten.  Of p only imageWidth, imageHeight, seed, tMin,
 *             spp and sampleFirst are read (the last two only without a list).
 *   scatter   per entry, from dRecords[i]:
 *               prim == SRT_NO_HIT         dOut[i] = {attenuation 0, SRT_PATH_MISS, emitted 0, prim SRT_NO_HIT}; dRng[i] and
 *                                          dRaysOut[i] are untouched, dRays[i] is not read.
 *               material outside [0, numMaterials)
 *                                          dOut[i] = {0, SRT_PATH_INVALID, 0, the record's prim}; nothing else is read or
 *                                          written (the kernel bounds the index itself: no record can make it read out of
 *                                          bounds).
 *               otherwise                  material::scatter on (dRays[i], the record) with the draws from dRng[i];
 *                                          emitted = material::emitted, always written; prim = the record's.
 *                 scatter returned false   status SRT_PATH_ENDED, attenuation 0; dRaysOut[i] untouched; dRng[i] advanced by
 *                                          what scatter drew before it gave up (a metal's fuzz sphere; nothing for a light).
 *                 scatter returned true    status SRT_PATH_SCATTERED, the attenuation, and dRaysOut[i] = {o = the hit point,
 *                                          d = the scattered direction, time = the incoming ray's, tMin and tMax copied
 *                                          from the incoming ray}.
 *             dRaysOut may equal dRays: an entry reads its ray before it writes it.  With dRng[i] = srtRngKey(seed, i, 0)
 *             the attenuation, the scattered ray, the flag and the emitted colour equal srtScatterRays' out13 bit for bit (a
 *             light's unspecified "scattered ray" excepted).
 *   step      for every entry with dActive == NULL or dActive[i] != 0: what srtTraceRaysDevice(traversal, dHits, records)
 *             of dRays[i] followed by srtScatterRaysDevice on its record leave in dOut[i], dRng[i], dRaysOut[i] and, where
 *             dHits is not NULL, dHits[i] -- byte for byte.  An inactive entry reads nothing but its byte and writes nothing.
 *             FAITHFUL and CLOSEST have the meanings, the tie rule and the conditions of "Ray queries" above.
 *   the loop  one sample of the render is at most maxBounce steps from its camera ray (active = the entries that
 *             SCATTERED in the step before).  Its terminal radiance is `background` after a MISS, `emitted` after ENDED and
 *             0 when maxBounce steps all scattered (or maxBounce is 0); its radiance is the terminal one unwound through
 *             the attenuations of its scattered steps, L = 0.0f + L * attenuation_j per channel (a separate multiply and
 *             add, no contraction) for j from the last scattered step down to 0 (main.cpp:49-51).  A pixel is the float
 *             running sum of its samples' L in sample-index order, with w their count (main.cpp:217).  With FAITHFUL
 *             steps that is srtRenderImage's accumulation buffer bit for bit (sppChunks = 1; more chunks add the same
 *             samples in the exact chunk sum's order).
 *   errors    (non-zero, message in srtLastError, NOTHING launched, outputs untouched; all decided on the host) scatter and
 *             step: no scene uploaded; geometry updated and not yet refitted.  All: n < 0; with n > 0 a NULL or misaligned
 *             required pointer (every buffer not called optional above).  Step: a traversal that is neither value; a tree
 *             too deep for the per-lane LDS stacks, as srtTraceRaysDevice refuses it.  Camera: no camera set; an image
 *             smaller than 2 x 2; without a list, spp < 1 or n != W * H * spp. */
enum { SRT_PATH_INVALID = -1, SRT_PATH_MISS = 0, SRT_PATH_ENDED = 1, SRT_PATH_SCATTERED = 2 };
typedef struct SrtPathOut { /* 32 bytes, aligned to 16: two dwordx4 stores */
  float attenuation[3];
  int32_t status;           /* SRT_PATH_* */
  float emitted[3];
  int32_t prim;             /* index into prims[], SRT_NO_HIT on a miss */
} SrtPathOut;
uint64_t srtRngKey(uint64_t seed, uint64_t pixel, uint64_t sample); /* pixel and sample are 32-bit values: their low 32 bits */
int srtCameraRaysDevice(SrtContext* ctx, const SrtRenderParams* p, const void* dPixelSample, int64_t n, void* dRays, void* dRng,
                        void* stream);
int srtScatterRaysDevice(SrtContext* ctx, const void* dRays, const void* dRecords, int64_t n, void* dRng, void* dOut,
                         void* dRaysOut, void* stream);
int srtPathStepDevice(SrtContext* ctx, int32_t traversal, const void* dRays, int64_t n, const void* dActive, void* dRng,
                      void* dOut, void* dRaysOut, void* dHits, void* stream);

/* srtTracePathsDevice     "the loop" above in ONE kernel: here are rays on the device, give me their path-traced radiance.
 *                         A lane carries a path from its first ray to its end, unwinds it and takes the next entry from
 *                         a counter: nothing passes through memory between bounces, no count is read back, and waves
 *                         are refilled without a compaction pass.
 *   per entry the path of "the loop" that starts at dRays[i] with the state dRng[i]: at most maxBounce steps of
 *             srtPathStepDevice(traversal), each on the scattered ray of the step before.  The terminal radiance is
 *             `background` after MISS, `emitted` after ENDED and 0 after INVALID or when every step scattered; it is
 *             unwound L = 0.0f + L * attenuation_j per channel (a separate multiply and add), innermost first.
 *             dResult[i] = {L, the number of steps that ran, the status of the last one}; dRng[i] = the state after the
 *             path's last draw.  dRays is only read.  With FAITHFUL steps and the rays of srtCameraRaysDevice, a pixel's
 *             float running sum of its samples' L in sample-index order is srtRenderImage's accumulation buffer bit for
 *             bit, as for the loop.
 *   buffers   all DEVICE pointers but `background`.  dRays = SrtRay[n], aligned to 4; dRng = uint64_t[n], aligned to 8;
 *             dResult = SrtPathRadiance[n], aligned to 16.  background: a HOST pointer to 3 floats, read during the call.
 *             maxBounce in [0, SRT_MAX_BOUNCE]; with 0 no step runs and every entry is {0, 0, SRT_PATH_SCATTERED}.
 *   scratch   dScratch, SRT_PATHS_SCRATCH_BYTES bytes aligned to 8, is the caller's.  The call zeroes it on `stream` itself,
 *             with a memset ahead of the kernel; its contents afterwards are unspecified.  Two calls on one stream may
 *             share it; calls on different streams need one each.
 *   async     on `stream`: one memset and one kernel, in which no wave waits for another one.  Allocates nothing, does not
 *             synchronise, touches no scratch of the context's, and leaves the tunables, the host generator, the chunk
 *             scratch, srtLastKernelMs, srtGetLaunchInfo, srtGetStats and the temporal history as they were.
 *   never written  elements at index >= n; anything outside the SRT_PATHS_SCRATCH_BYTES of scratch.
 *   n == 0    returns 0 and launches nothing.
 *   FAITHFUL and CLOSEST have the meanings, the tie rule and the conditions of "Ray queries" above: for a ray that is not
 *             finite the result is unspecified, but the call still terminates and writes element i only.
 *   errors    (non-zero, message in srtLastError, NOTHING launched, outputs untouched; all decided on the host) no scene
 *             uploaded; geometry updated and not yet refitted; n < 0; a traversal that is neither value; maxBounce outside
 *             [0, SRT_MAX_BOUNCE]; a NULL background; with n > 0 a NULL or misaligned dRays (4), dRng (8), dResult (16) or
 *             dScratch (8); an overlap of dResult, dScratch or dRng with one another or with dRays, each taken at its
 *             full length (range comparison, as srtCompactPathsDevice's); a tree so deep that the kernel's LDS -- 1 KB per
 *             pending reference as for the queries, and 3 KB per bounce of maxBounce -- exceeds 160 KB. */
enum { SRT_PATHS_SCRATCH_BYTES = 64 };
typedef struct SrtPathRadiance { /* 16 bytes, aligned to 16: one dwordx4 store */
  float radiance[3];             /* L of "the loop" above */
  int16_t steps;                 /* steps that ran: 0 .. maxBounce */
  int16_t status;                /* SRT_PATH_* of the last step that ran; SRT_PATH_SCATTERED: the bounce limit ended the path
                                    (also when maxBounce == 0 and no step ran) */
} SrtPathRadiance;
int srtTracePathsDevice(SrtContext* ctx, int32_t traversal, int32_t maxBounce, const float background[3],
                        const void* dRays, int64_t n, void* dRng, void* dResult, void* dScratch, void* stream);

/* Direct light sampling (next-event estimation) for device paths: at every pbr hit one of the scene's sampled lights is
 * chosen, a direction inside the cone it subtends is drawn, a shadow ray is walked and the material is evaluated for that
 * direction.  Opt-in: new entries only; srtRenderTiles and every entry above keep their bits.
 *
 * srtGetSampledLights       (host only) which primitives are sampled.
 * srtDirectLightDevice      the direct term of every hit record: the per-hit piece for a loop of one's own.
 * srtTracePathsDirectDevice srtTracePathsDevice with the term added at every pbr hit, in one kernel.
 *
 *   expectation  pbr's scatter draws sd = unit(n + randomUnitVector) -- cosine-weighted about the shading normal n, pdf
 *             cos / pi -- and returns att(sd) = (fd + fs) * NdotL WITHOUT dividing by that pdf.  The direct term carries the
 *             pdf as a weight, so that the estimator converges to the image of the plain one.  It is not the physically
 *             correct weight.
 *   lights    S = the spheres whose material is SRT_MAT_LIGHT with a solid-colour emit texture (or one that failed to load:
 *             magenta), in prims[] order; K = |S|, no cap.  A property of the upload: an update changes no material.
 *             srtGetSampledLights: *count = K; prims, where not NULL, receives the K prims[] indices (capacity >= K, else an
 *             error).  Centre, radius and whether the sphere moves are read from its device record where it is used: a light
 *             moved by srtUpdateSpheres + srtRefitScene is followed with no further call.  Never sampled, and exactly as
 *             without these entries: triangle lights; lights whose emit texture is an image or a checker; spheres with
 *             center0 != center1 (listed in S, but choosing one yields nothing and their emission is never dropped).
 *   the term  at a hit x of ray r whose material is a pbr one of the scene's, when K > 0; s = the path's generator state
 *             before the hit's scatter draws.  Float operations, each rounded, no contraction; lenSq(v) = (x*x + y*y) + z*z,
 *             dot3(a, b) = a.x*b.x + (a.y*b.y + a.z*b.z), a scalar times a vector per component.
 *               1  state = mix64(s ^ 0x5DEECE66D2545F49) seeds a generator of the term's own; s is not advanced.
 *               2  u is drawn; k = min((int)(u * (float)K), K - 1); c = the sphere's center0, rad its radius;
 *                  toC = c - x; d2 = lenSq(toC); r2 = rad * rad.  If the sphere moves or d2 <= r2: the term is 0,
 *                  light = -1, dir = 0, weight = 0, and nothing more is drawn.
 *               3  (a, b) = the lens disk's draw (y first: b, then a, each lo + (hi - lo) * u on (-1, 1), repeated while
 *                  (a*a + b*b) + 0*0 >= 1); sD = a*a + b*b; q = r2 / d2; oneMinus = q / (1 + sqrt(1 - q)) (1 - cos of the
 *                  cone's half angle, without cancellation); m = sD * oneMinus; cosT = 1 - m; sinT = sqrt(m * (2 - m));
 *                  root = sqrt(sD); (cPhi, sPhi) = sD == 0 ? (1, 0) : (a / root, b / root); w = toC / sqrt(d2) per component;
 *                  the basis of Duff et al. 2017 about w: sign = copysign(1, w.z); ka = -1 / (sign + w.z);
 *                  kb = (w.x * w.y) * ka; sx = sign * w.x; t1 = (1 + (sx * w.x) * ka, sign * kb, -sx);
 *                  t2 = (kb, sign + (w.y * w.y) * ka, -w.y); dir = ((cPhi * sinT) * t1 + (sPhi * sinT) * t2) + cosT * w.
 *               4  weight = ((float)K * (2 * oneMinus)) * max(dot3(n, dir), 0): K * the cone's solid angle * cos / pi, the
 *                  pi cancelled.  n = the normal scatter uses (the mapped one where there is a normal map).
 *               5  the shadow ray {o = x, d = dir, time, tMin, tMax of r} -- the ray scatter would have written had it
 *                  drawn dir -- is walked with `traversal`; the light is visible iff the walk returns exactly sphere k.
 *               6  term = visible ? (attEval(dir) * Le_k per channel) * weight : an exact 0.  attEval(dir) is pbr's
 *                  attenuation (fd + fs) * NdotL from viewVec on with sd = dir as given, on the hit's own texture
 *                  look-ups; Le_k the light's colour.  A NaN of a roughness-0 material is what the plain path makes too.
 *   direct    srtDirectLightDevice: dRays = SrtRay[n] (4), dRecords = SrtHit[n] (4) as srtTraceRaysDevice writes them, dRng =
 *             uint64_t[n] (8), only READ: entry i's state before its scatter draws -- call it before srtScatterRaysDevice.
 *             dDirect = SrtDirectOut[n], aligned to 16.  A miss, a record whose material is not pbr or not one of the
 *             scene's, and every entry when K = 0: {0, -1, 0, 0}.  Asynchronous on `stream`, one kernel, allocates nothing.
 *   whole     srtTracePathsDirectDevice has srtTracePathsDevice's signature, buffers, scratch, checks and guarantees.  The
 *             term's generator is its own, so every path's bounces, hits, attenuations, steps, status and final dRng are
 *             srtTracePathsDevice's bit for bit.  A step's hit on a sphere of S loses its emission (terminal 0, status still
 *             SRT_PATH_ENDED) iff the step before evaluated a term (its hit was pbr, K > 0), the sphere does not move and
 *             lenSq(c - o) > rad * rad with o the ray's origin: exactly when step 2 could have chosen it, whatever it
 *             chose.  Camera rays and rays leaving metal or glass keep a light's emission.  Unwinding: L = D_j + L * att_j
 *             per channel, a separate multiply and add, innermost first, D_j the term of scattered step j (0.0f where none
 *             was evaluated).  With K = 0 every byte equals srtTracePathsDevice's.  LDS: 6 KB per bounce of maxBounce
 *             instead of 3.
 *   errors    as srtPathStepDevice's and srtTracePathsDevice's, decided on the host, nothing launched.  srtDirectLightDevice
 *             also refuses dDirect overlapping an input.  srtGetSampledLights: no scene, a NULL count, capacity < K. */
typedef struct SrtDirectOut { /* 32 bytes, aligned to 16: two dwordx4 stores */
  float radiance[3];          /* the term */
  int32_t light;              /* the chosen light's prims[] index; -1: none was sampled */
  float dir[3];               /* the sampled direction (0 when light == -1) */
  float weight;
} SrtDirectOut;
int srtGetSampledLights(SrtContext* ctx, int32_t* prims, int32_t capacity, int32_t* count);
int srtDirectLightDevice(SrtContext* ctx, int32_t traversal, const void* dRays, const void* dRecords, int64_t n, const void* dRng,
                         void* dDirect, void* stream);
int srtTracePathsDirectDevice(SrtContext* ctx, int32_t traversal, int32_t maxBounce, const float background[3],
                              const void* dRays, int64_t n, void* dRng, void* dResult, void* dScratch, void* stream);
/* srtRenderDirectImage      the frame of p through those entries, blocking, HOST buffers as srtRenderImage's (either may be
 *             NULL): hAccum = W * H float4, the float running sum of every pixel's sample radiances in sample-index order
 *             with w their count; hRgba = W * H x 4 bytes, its 8-bit form as the adaptive entries quantise an image
 *             (mean = sum * (1 / w)).  Per batch of samplesPerBatch sample indices: srtCameraRaysDevice without a list
 *             (entries pixel-major), srtTracePathsDirectDevice(p->traversal, p->maxBounce, p->background), and one kernel
 *             that adds each pixel's samples in order.  A batch holds 60 bytes per (pixel, sample); samplesPerBatch = 0
 *             picks the largest count that keeps a batch at 2^22 entries (at least 1).  The batch size does not change the
 *             image.  With K = 0 and FAITHFUL steps the two outputs are srtRenderImage's (sppChunks = 1) in every byte.  Of p
 *             the tile split, sppChunks and countStats are not read.  Errors: srtRenderImage's and the two entries'; a
 *             negative samplesPerBatch; a batch of 2^31 entries or more. */
int srtRenderDirectImage(SrtContext* ctx, const SrtRenderParams* p, int32_t samplesPerBatch, float* hAccum, uint8_t* hRgba);

/* srtCompactPathsDevice   stable compaction of the live paths between two steps: the entries that go on move, in their
 *                         order, to the front of fresh ray, state and slot buffers, so that the next step runs on full
 *                         waves instead of on the few live lanes of nearly every wave.  Compaction moves bytes: nothing
 *                         is computed, and a loop that compacts between its steps renders the same bits.
 *   keep      keep[i] = (dActive == NULL || dActive[i] != 0) && (dOut == NULL || dOut[i].status == SRT_PATH_SCATTERED).
 *             dOut = SrtPathOut[n], aligned to 16, of which only the status dword is read; dActive = uint8_t[n].  Not both
 *             NULL.  An inactive entry's dOut[i] is stale by srtPathStepDevice's contract, which is why the mask of the
 *             step that wrote dOut takes part.  With dOut == NULL the mask alone is the caller's own predicate (Russian
 *             roulette, a path-length cut).
 *   order     stable.  With count = the number kept and rank(i) = the number of kept j < i, for every kept i:
 *             dRaysOut[rank(i)] = dRays[i] (36 bytes), dRngOut[rank(i)] = dRng[i] (8 bytes) and
 *             dSlotOut[rank(i)] = dSlot ? dSlot[i] : (int32_t)i.
 *   payloads  dRays / dRaysOut = SrtRay[n] aligned to 4, dRng / dRngOut = uint64_t[n] aligned to 8, dSlot / dSlotOut =
 *             int32_t[n] aligned to 4.  Each of the three is optional: an output whose input is NULL is refused -- except
 *             dSlotOut, which with dSlot == NULL receives the identity (the index an entry had before) -- and an input
 *             whose output is NULL is ignored.  Carrying dSlotOut from one compaction into the next as dSlot keeps the
 *             index every survivor had in the first buffer.
 *   dCount    int64_t[1] on the device, aligned to 8, required: receives count.
 *   dActiveOut  uint8_t[n] or NULL: dActiveOut[i] = (i < count) for every i < n.  The next step can be launched with the
 *             old n and this mask without reading dCount: the live entries are dense in the leading waves, and the whole
 *             waves behind them leave after one byte.  dActiveOut may be exactly dActive: each entry reads its byte
 *             before that byte is written.
 *   never written  elements at index >= count of dRaysOut, dRngOut and dSlotOut; elements at index >= n of dActiveOut;
 *             anything outside the documented scratch size.
 *   overlap   no output (dRaysOut, dRngOut, dSlotOut, dActiveOut, dCount, dScratch) may overlap any input that is read, or
 *             any other output, each taken at its full length of n elements (compaction in place races across
 *             workgroups); dActiveOut == dActive is the one exception.  Refused on the host by range comparison.
 *   scratch   dScratch, aligned to 8, is the caller's: srtCompactPathsScratchBytes(n) = 8 * ceil(n / SRT_COMPACT_TILE)
 *             bytes (one 64-bit word per tile of SRT_COMPACT_TILE entries: its kept count, then its offset), 0 for
 *             n <= 0.  Host only, needs no context.  Its contents afterwards are unspecified.
 *   async     on `stream`: three kernels (count per tile, a one-workgroup scan, scatter), none of which waits for another
 *             workgroup.  Allocates nothing, does not synchronise, touches no scratch of the context's, and leaves the
 *             tunables, the host generator, the chunk scratch, srtLastKernelMs, srtGetLaunchInfo, srtGetStats and the
 *             temporal history as they were.  Needs no uploaded scene.
 *   n == 0    returns 0 and launches nothing; dCount is NOT written.
 *   errors    (non-zero, message in srtLastError, NOTHING launched, outputs untouched; all decided on the host) n < 0;
 *             dOut and dActive both NULL; a NULL dCount; with n > 0 a NULL dScratch; dRaysOut without dRays or dRngOut
 *             without dRng; a misaligned pointer (rays and slots 4 bytes, rng states, dCount and dScratch 8, dOut 16);
 *             n > 2^31 - 1 with dSlotOut; an overlap as above. */
enum { SRT_COMPACT_TILE = 1024 }; /* entries a workgroup handles per trip */
int64_t srtCompactPathsScratchBytes(int64_t n);
int srtCompactPathsDevice(SrtContext* ctx, int64_t n, const void* dOut, const void* dActive, const void* dRays, const void* dRng,
                          const void* dSlot, void* dRaysOut, void* dRngOut, void* dSlotOut, void* dActiveOut, void* dCount,
                          void* dScratch, void* stream);

/* srtSortPathsDevice      srtCompactPathsDevice with an order: the entries that go on move to the front of fresh ray, state
 *                         and slot buffers, ordered by the cell of a grid their origin lies in and by the octant their
 *                         direction points into, so that the lanes of a wave of the next step ask for neighbouring parts
 *                         of the tree.  Sorting moves bytes: nothing that reaches a pixel is computed, and a loop that
 *                         sorts between its steps renders the same bits.  Compaction is the case of one key for all.
 *   keep      srtCompactPathsDevice's keep[i], except that dOut and dActive may BOTH be NULL: every entry is then kept
 *             (the form for a batch of shadow or ambient-occlusion rays).
 *   key       a 32-bit word per entry, from dRays[i] (o = its origin, d = its direction) and dBox.  dBox is a DEVICE
 *             pointer to 6 floats {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}, aligned to 4; the caller makes it on the stream,
 *             from bounds it holds or from the origins (a minimum and a maximum over the rows), without reading anything
 *             back.  cellBits in [1, SRT_SORT_MAX_CELL_BITS] is the number of grid bits per axis.  Per axis a, in float32,
 *             as three separate operations (no contraction):
 *               s   = float(1 << cellBits) / (hi_a - lo_a)      a correctly rounded division
 *               c   = (o_a - lo_a) * s
 *               q_a = 0 unless c >= 0; otherwise min((int)trunc(c), (1 << cellBits) - 1)
 *             The rule is total: a NaN c gives cell 0, +inf the last cell, a negative c cell 0 -- so an origin outside
 *             the box, an axis with hi_a == lo_a (s infinite: c is NaN on lo_a, +-inf elsewhere), an inverted box
 *             (s negative) and a box with a NaN or an infinity in it need no case of their own and are not errors.
 *             cell = the Morton interleave of q: bit k of q_x goes to bit 3k, of q_y to bit 3k + 1, of q_z to bit 3k + 2.
 *             octant = signbit(d_x) | signbit(d_y) << 1 | signbit(d_z) << 2 -- the sign BIT: -0 counts as negative, and a
 *             NaN has the sign its bit says.  A kept entry has key = cell << 3 | octant; an entry that is not kept has
 *             key = 1u << (3 * cellBits + 3), above every kept key, and its ray is not read.  The sort runs over bits
 *             [0, 3 * cellBits + 4) only: fewer cell bits make a cheaper sort.
 *   order     STABLE by key: entries with equal keys stay in index order.  With count = the number kept and rank(i) = the
 *             position of i in that order, for every kept i: dRaysOut[rank(i)] = dRays[i] (36 bytes),
 *             dRngOut[rank(i)] = dRng[i] (8 bytes) and dSlotOut[rank(i)] = dSlot ? dSlot[i] : (int32_t)i.  The
 *             permutation is a function of the inputs alone.
 *   payloads, dCount, dActiveOut, never written, overlap
 *             srtCompactPathsDevice's, word for word, with this call's scratch size, with dRays always read (it is
 *             required even without dRaysOut, aligned to 4) and with dBox as one more input that no output may overlap.
 *             dActiveOut may be exactly dActive here too.
 *   scratch   dScratch, aligned to 8, is the caller's: scratchBytes bytes, at least srtSortPathsScratchBytes(n) (key and
 *             index of every entry, twice, and the radix sort's temporary storage; about 20 bytes per entry).  That
 *             function is host only, needs no context, is 0 for n <= 0 and never decreases as n grows: a scratch sized for
 *             n serves every call with fewer entries.  Its contents afterwards are unspecified.
 *   async     on `stream`: a memset of dCount, the key kernel, rocPRIM's radix_sort_pairs over (key, index) and the gather
 *             kernel; no kernel of the library's own waits for another workgroup.  Allocates nothing, does not
 *             synchronise, touches no scratch of the context's, and leaves the tunables, the host generator, the chunk
 *             scratch, srtLastKernelMs, srtGetLaunchInfo, srtGetStats and the temporal history as they were.  Needs no
 *             uploaded scene.
 *   n == 0    returns 0 and launches nothing; dCount is NOT written.
 *   errors    (non-zero, message in srtLastError, NOTHING launched, outputs untouched; all decided on the host)
 *             srtCompactPathsDevice's -- but dOut and dActive both NULL is no error, and n > 2^31 - 1 is refused whether
 *             or not there is a dSlotOut -- and: cellBits outside [1, SRT_SORT_MAX_CELL_BITS]; with n > 0 a NULL or
 *             misaligned dBox, a NULL dRays, a scratchBytes below srtSortPathsScratchBytes(n). */
enum { SRT_SORT_MAX_CELL_BITS = 9 }; /* 27 cell bits, 3 octant bits: at most 31 key bits with the dropped entries' one */
int64_t srtSortPathsScratchBytes(int64_t n);
int srtSortPathsDevice(SrtContext* ctx, int64_t n, int32_t cellBits, const void* dBox, const void* dOut, const void* dActive,
                       const void* dRays, const void* dRng, const void* dSlot, void* dRaysOut, void* dRngOut, void* dSlotOut,
                       void* dActiveOut, void* dCount, void* dScratch, int64_t scratchBytes, void* stream);

/* material::scatter + material::emitted (material.h:15-21; texture::value through a light's emitted, texture.h:13-16) for
 * n (incoming ray, hit record) pairs, evaluated by the render kernels' own shading function.  hits[i].material indexes
 * the uploaded scene's materials; p, normal, tangent, bitangent, uv, t, frontFace are read as the reference's hitRecord
 * fields.  Random draws come from the counter RNG keyed (seed, i, 0) -- the reference draws from its process-global
 * generator.  out13 per entry: attenuation[3], scattered direction[3], scattered origin[3], scatter's bool (0 / 1),
 * emitted[3]; a light's scatter makes no scattered ray (material.h:144-146), and what the entry reports as one is not
 * specified.  A hit whose material is not one of the scene's is refused.  HOST pointers; blocking. */
int srtScatterRays(SrtContext* ctx, const SrtRay* rays, const SrtHit* hits, int32_t n, uint64_t seed, float* out13);

/* Duration of the most recent srtRenderTiles kernel, from HIP events recorded
 * on its stream (synchronises on the stop event). */
int srtLastKernelMs(SrtContext* ctx, float* ms);
int srtGetStats(SrtContext* ctx, SrtStats* out);
/* device properties the bench prints next to its numbers */
int srtDeviceInfo(SrtContext* ctx, char* name, int32_t nameCap, int32_t* numCUs, int32_t* clockMHz);

#ifdef __cplusplus
}
#endif
#endif /* SRT_HIP_H */
