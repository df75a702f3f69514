/*
 * srt_hip_test.h -- test hooks and diagnostics of libsrt_hip.so.
 *
 * NOT part of the drop-in boundary (include/srt_hip.h): nothing here is needed to render.  These entry
 * points let the parity tests reach device functions of the hot path in isolation (the kernel's own
 * shading function, the render kernel's own traversal per ray) and let the
 * measurement tools vary the work distribution.  HOST pointers throughout.
 */
#ifndef SRT_HIP_TEST_H
#define SRT_HIP_TEST_H

#include "srt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-ray view into the RENDER kernel's own traversal (not srtTraceRays' kernel): renders sample
 * p->sampleFirst of every pixel with the counting variant of the kernel the same launch without counting would run
 * (srt_render_kernel, or the path-pool kernel srt_render_wf_kernel in its whole-tree or hybrid form: srtGetLaunchInfo
 * tells which) and records, per pixel, the ray that path traced at bounce `depth` (0 = the camera ray) and what the
 * kernel's node / primitive steps made of it.  Feeding the recorded rays to the oracle's world.hit() checks the render
 * kernel's slab-test certificate, stack or thread-link handling and scheduler ray by ray.  hOut: W*H records in image
 * order. */
typedef struct SrtAovRecord {
  float o[3], d[3], time; /* the ray (tMin = p->tMin, tMax = +inf, main.cpp:39) */
  int32_t valid;          /* 0: the pixel's path ended before this bounce */
  int32_t prim;           /* index into prims[], SRT_NO_HIT on a miss */
  float t;
  int32_t nodeVisits, boxPasses, triTests, sphereTests;
  int32_t pad[2];
} SrtAovRecord;
int srtRenderAov(SrtContext* ctx, const SrtRenderParams* p, int32_t depth, SrtAovRecord* hOut);

/* What srtScatterRays does (include/srt_hip.h), through any instance of the kernels' shading function: bit 0 of `form` selects the
 * WIDE instance (all four texel loads of a pbr hit in flight at once: the path-pool kernel and the kernels over the
 * LDS-resident tree), bit 1 the COUNT instance (the counting launches).  Form 0 is srtScatterRays itself.  Entry i is keyed
 * (seed, i, 0).  outFetches: one uint32 per entry, the texel-fetch counter of the call (lookups of loaded images; stays 0
 * in a form without COUNT), or NULL.  Both entries refuse a hit whose material is not one of the scene's. */
int srtScatterRaysForm(SrtContext* ctx, const SrtRay* rays, const SrtHit* hits, int32_t n, uint64_t seed, int32_t form, float* out13,
                       uint32_t* outFetches);

/* pbr's attenuation for a direction of the caller's: what step 6 of "Direct light sampling" (include/srt_hip.h) calls
 * attEval -- the kernels' one statement of (fd + fs) * NdotL from viewVec on (csrc/srt_path.h pbrAttenuation, which shade()
 * evaluates for the direction it drew) on the hit's own texture look-ups.  DEVICE pointers, unlike the other hooks: dRays =
 * SrtRay[n] (4), dRecords = SrtHit[n] (4) as srtTraceRaysDevice writes them, dDirs = float[n][3] (4), dAtt = float[n][3] (4).
 * With the direction srtScatterRaysDevice wrote for the entry, dAtt[i] is that call's attenuation bit for bit.  0 for a miss
 * and for a record whose material is not pbr or not one of the scene's.  One kernel on the NULL stream; does not synchronise. */
int srtTestEvalScatterDevice(SrtContext* ctx, const void* dRays, const void* dRecords, const void* dDirs, int64_t n, void* dAtt);

/* The exact chunk sum on caller-made partial sums.  hChunks: chunks x n float4, slot [c][i] (rgb partial sums, w the slot's
 * sample count).  path 0: srt_sum_chunks_kernel over the uploaded slots.  path 1: the atomic path -- one thread per slot
 * calls commitFixed on a zeroed SrtFixedAccum[n], then srt_finalize_kernel(samples).  The limit is the one a render of
 * `chunks` chunks uses.  hOut4: n float4 (w: path 0 the float sum of the slot counts in slot order, path 1 (float)samples).
 * Host pointers; needs no scene.  Refuses, with an error text, n outside [1, 2^20], chunks < 1 or above the largest count
 * srtPlanSppChunks allows any image (30 812), a path other than 0 or 1, and null pointers. */
int srtTestChunkSum(SrtContext* ctx, const float* hChunks, int32_t n, int32_t chunks, int32_t path, int32_t samples, float* hOut4);

/* Reads back the denoiser's scratch (csrc/srt_denoise.hip) as the most recent srtDenoise / srtDenoiseMoments of a
 * width x height image on this context left it: synchronises the device, then copies the four regions to HOST buffers, any
 * of which may be NULL.  hGuide4: W*H x {n.xyz, z}, z = NaN for a miss.  hGrad2: W*H x {zx, zy}.  hCol0_4, hCol1_4: the two
 * ping-pong colour buffers, W*H x {e.rgb, v}; a pixel that is not valid has e.r = NaN (the prepare pass: all of e NaN; a
 * level: {NaN, 0, 0, 0}).  The prepare pass writes col[0] = {e, v} after 0 levels, level i reads col[i & 1] and writes
 * col[(i + 1) & 1], and the last level writes the caller's outputs instead.  So after a run of k + 1 levels col[k & 1] holds
 * {e, v} after k levels (col[0] after 0 levels when k = 0) and the other buffer the state after k - 1 levels, or what an
 * earlier call left when k = 0.  Launches nothing and changes nothing.  Fails, with an error text, for a size <= 0 and
 * when the context's scratch is smaller than width * height * SRT_DENOISE_SCRATCH_BYTES_PER_PIXEL bytes. */
int srtTestDenoiseScratch(SrtContext* ctx, int32_t width, int32_t height, float* hGuide4, float* hCol0_4, float* hCol1_4, float* hGrad2);

/* Sub-step profile of the most recent countStats launch of the step-scheduler kernel (shader clocks summed over waves,
 * diagnostics only; zero after one of the path-pool kernel, which a counting launch runs where the production launch would):
 * out10 = { hit step: hit record, textures, direction draw, BRDF + bookkeeping; restart step;
 *           hit-step executions, hit-step lanes, restart-step executions, restart-step lanes, reserved }. */
int srtGetShadeProfile(SrtContext* ctx, uint64_t* out10);

/* Step profile of the most recent launch of the path-pool kernel's profiling variant (tunable "wf_profile" = 1;
 * csrc/srt_wavefront.hip): out46 = { clocks[12], executions[12], lanes[12] } for the step kinds node visit, primitive
 * test, swap, hit step of class 0 / 1 / 2, restart, idle, lost claim, item pull, visit of a node outside LDS (hybrid form:
 * the clocks are the wait for the records plus the visit; whole-tree form: no clocks, its executions word counts the swap
 * steps that ran the head of the new rays' walks -- tunable "wf_head" -- and its lanes word those rays), and an eleventh
 * slot whose clocks word counts the primitive-step executions that ran the exact triangle test and whose executions word counts the lanes the triangle certificate left
 * undecided (its lanes word: the hybrid form's near lanes); scheduling clocks, total wave clocks; then what the
 * scheduling decisions that looked at the rings saw, summed: decisions, lanes at nodes / at primitives / finished / idle,
 * READY fill, fill of the fullest served ring, RESTART fill. */
int srtGetWfProfile(SrtContext* ctx, uint64_t* out46);

/* Host-only (no device): the thread links srtUploadScene builds for the stackless walks (csrc/srt_thread.h) from a
 * flattened node array -- nodes8 = numNodes x 8 floats, (bmin.xyz, left) (bmax.xyz, right), node references = index * 32,
 * primitives = ~(index << 1 | sphere) -- and the world list's references.
 * srtTestThreadLinks16: one word per node (DevScene::nodeThread) -> outLinks[numNodes]; returns 1, or 0 when the forest has
 * no 16-bit threaded form.
 * srtTestHybridRecords: the path-pool kernel's hybrid records (DevScene::nodesWf / worldWf / primSecond) with at most `cap`
 * resident nodes -> outNodes8[numNodes x 8], outWorld[numWorld], outSecond[2 * max(numTriangles, numSpheres) + 2]; returns
 * the number of resident nodes, or 0 when the forest has no threaded form.  Both return -1 on a null argument. */
int srtTestThreadLinks16(const float* nodes8, int32_t numNodes, const int32_t* world, int32_t numWorld, int32_t numTriangles, int32_t numSpheres,
                         int32_t* outLinks);
int srtTestHybridRecords(const float* nodes8, int32_t numNodes, const int32_t* world, int32_t numWorld, int32_t numTriangles, int32_t numSpheres,
                         int32_t cap, float* outNodes8, int32_t* outWorld, int32_t* outSecond);

/* The regrouped tree of the path-pool kernel's whole-tree form (csrc/srt_regroup.h; tunable "wf_regroup": 2, the default =
 * the kernel walks the regrouped tree's walk sequence, below; 1 = the binary regrouped tree; 0 = the reference tree): the
 * reference's leaf records in the reference's order under inner nodes rebuilt by a surface-area split over contiguous leaf
 * ranges.  Every walk ends at the same (t, primitive) under all three; accumulators are bit-identical.
 * srtTestRegroup (host only, no device): the regrouped array of a flattened node array (the format above) and its world
 * list -> outNodes8[numNodes x 8]; returns 1, 0 when a tree is not a pre-order tree of two-node / two-primitive nodes, -1 on a
 * null argument.
 * srtTestGetRegroup: the uploaded scene's regrouped array and its 16-bit thread links (DevScene::nodesRg / nodeThreadRg) as they
 * lie in device memory now (after srtRefitScene as well) -> outNodes8[count x 8], outLinks[count]; either may be NULL.
 * *count = 0 when the upload built none (a tree beyond LDS, a caller-built tree, device-built trees, a box that is not ordered). */
int srtTestRegroup(const float* nodes8, int32_t numNodes, const int32_t* world, int32_t numWorld, float* outNodes8);
int srtTestGetRegroup(SrtContext* ctx, float* outNodes8, int32_t* outLinks, int32_t capacity, int32_t* count);

/* The regrouped tree's WALK SEQUENCE (csrc/srt_regroup.h srtRegroupWalk; tunable "wf_regroup" 2): the regrouped array without
 * the gates that rarely cull a ray -- gate g with m effective children under its binary parent p is elided when
 * area(g) * m > area(p) * (m - 1), bottom-up, and so is every inner root; leaves are always kept.  The kept records are
 * numbered in array order; record j has its source record in the regrouped array (whose box it takes at every launch) and the
 * two link words of csrc/srt_wf_links.h (srtWfSeqHitWord, srtWfSeqMissWord); a world item has an entry word.
 * srtTestRegroupWalk (host only, no device): from a regrouped array (srtTestRegroup's output, the format above) and its world
 * list -> outKeep[numNodes] (1 = kept), outSrc[*count], outLinks[2 x *count] (hit word, miss word), outEntry[numWorld]; outSrc
 * and outLinks must hold numNodes records.  Returns 1, 0 for an array that is not one of pre-order trees of two-node /
 * two-primitive nodes, -1 on a null argument.
 * srtTestGetRegroupWalk: the uploaded scene's sequence as it lies in device memory now (after srtRefitScene as well), same
 * outputs, any of which may be NULL; `capacity` must be the node count of srtTestGetRegroup at least.  *count = 0 when the
 * upload built no regrouped tree. */
int srtTestRegroupWalk(const float* nodes8, int32_t numNodes, const int32_t* world, int32_t numWorld, uint8_t* outKeep, int32_t* outSrc,
                       int32_t* outLinks, int32_t* outEntry, int32_t* count);
int srtTestGetRegroupWalk(SrtContext* ctx, uint8_t* outKeep, int32_t* outSrc, int32_t* outLinks, int32_t* outEntry, int32_t capacity, int32_t* count);

/* The HEAD of the sequence's walks (csrc/srt_regroup.h SrtRegroupWalk::head; tunable "wf_head", default 1, 0 = off): where the
 * world list is one tree, record 0 of its sequence is a leaf and every object of that leaf is a sphere, every walk begins with
 * that leaf's box test, its one or two sphere tests and a jump to its miss word.  The path-pool kernel's whole-tree form then
 * runs these where its swap step sets a new ray up, for all the new rays of the wave at once, and starts their walks at the
 * miss word; the head word is the leaf word (csrc/srt_wf_links.h srtWfLeafWord), 0 = no head.  Accumulators are bit-identical.
 * srtTestWfHead (host only, no device): the word for a node array in srtTestRegroupWalk's format whose primitives are
 * ~index -- as the CPU oracle's trees have them -- a world list of the same references, and the kind of every primitive,
 * kinds[index] != 0 = a sphere.  The hook rewrites every reference to the device's ~(index << 1 | sphere) and asks
 * srtRegroupWalk -> *outHead.  Returns 1; 0 (and *outHead = 0) for an array srtTestRegroupWalk refuses, an index outside
 * kinds[] or beyond the 15 bits of a leaf word's half; -1 on a null argument. */
int srtTestWfHead(const float* nodes8, int32_t numNodes, const int32_t* world, int32_t numWorld, const uint8_t* kinds, int32_t numKinds,
                  int32_t* outHead);

/* Reads back what the near-child-first traversal walks for world item `item` (host-built and device-built trees alike), as
 * it lies in device memory: the item's slice of DevScene::nodeAxis -> outAxis[count] (the split axis of each node, 3 = none)
 * and of DevScene::nodes2 -> outPairs16[count x 16] (the 64-byte records of csrc/srt_lbvh.hip pairNodes: left child's box
 * min / max in floats 0-2 / 4-6, the right child's in 8-10 / 12-14, the left / right reference as int bits in floats 3 / 7:
 * a node's record offset (scene-wide index * 64) or a device primitive reference ~(index << 1 | sphere)).  Either output
 * may be NULL; with both NULL only *count is written.  Fails for an item that is not a tree, or when capacity < count. */
int srtTestGetTreeAux(SrtContext* ctx, int32_t item, uint8_t* outAxis, float* outPairs16, int32_t capacity, int32_t* count);

/* The certified triangle test of the FAITHFUL render and trace kernels (csrc/srt_tri_hit.h; tunable "tri_cert", default 1, 0 = every
 * triangle test is the exact one): the render kernels over an LDS-resident tree and srtTraceRays run it; the path-pool
 * kernel's hybrid form and the 256-thread kernel (trees beyond LDS) keep the exact test alone.
 * srtTestGetTriUndecided: how many triangle tests of the most recent srtTraceRays call on this context the certificate left
 * to the exact test (0 after a CLOSEST call; where "tri_cert" has the certificate off, every triangle test).
 * srtTestGetTriFast: the uploaded scene's triFast records as they lie in device memory now (after srtUpdateTriangles as
 * well), 16 floats per triangle, in the SCENE's triangle order -> out16[count x 16]; out16 NULL: only *count.
 * srtTestTriFastRecord (host only, no device): the record srtUploadScene makes of one triangle, p9 = its three vertices:
 * (v0.xyz, d) (n.xyz, k) (m0.xyz, kappa) (m1.xyz, kappa E + floor); kappa = +inf marks a triangle outside the certified
 * ranges. */
int srtTestGetTriUndecided(SrtContext* ctx, uint64_t* out);
int srtTestGetTriFast(SrtContext* ctx, float* out16, int32_t capacity, int32_t* count);
int srtTestTriFastRecord(const float* p9, float* out16);

/* The two scene conditions of the certified slab test (csrc/srt_slab.h) as the kernels read them now, after srtUploadScene,
 * srtRefitScene or srtRebuildScene: out2 = { the fast-division word (the "fast_div" tunable as read at the upload while every
 * box coordinate is 0 or in [2^-77, 2^30], else 0), 1 while every node box is ordered (min <= max on every axis, all finite) else
 * 0 }.  The path-pool kernel over a whole LDS-resident tree picks a box's near and far planes by the ray's sign and certifies
 * a ray only where both hold; every other kernel orders the two quotients itself and asks for the first alone. */
int srtTestGetSlabScene(SrtContext* ctx, int32_t* out2);

/* The certified slab test as the device compiles it, outside any walk (csrc/srt_slabtest.hip: two kernels of their own that call
 * the per-ray and per-visit functions of csrc/srt_path.h and csrc/srt_query_walk.h; tests/test_gpu_slab_cert.py).  Neither needs a
 * scene; host pointers.
 * The first hook: r = refinedRcp(d) for the `count` float bit patterns firstBits, firstBits + 1, ... and e = |r d - 1| evaluated in
 * double (two floats' product is exact there): out2 = { the bits of the largest e as a double (+inf where r d is a NaN: d = 0),
 * the pattern of the d that gave it (the lowest such pattern) }.  The certificate assumes e <= 3 * 2^-24 for every direction
 * component it certifies (2^-20 <= |d| <= 2^20).  Refuses, with an error text, a range that is not made of 32-bit patterns of one
 * sign or that reaches an infinity or a NaN, count < 1 and a null output.
 * The second hook: n <= 2^20 cases of 13 floats -- box min[3], box max[3], ray origin[3], ray direction[3], tMax -- and one tMin for
 * the launch, which the kernel takes as an argument: the UNIFORM_TMIN forms read it from its scalar register, as in the render
 * kernels.  Per case, what a kernel does per ray -- certified = certifiedScene != 0 and fastDivOperandOk on the three axes, the
 * three refined reciprocals, slabSetup and slabSetupSign -- and per visit.  hOut: 8 words per case,
 *   floats 0-2  the reciprocals;  float 3  tolAbs of slabSetup;  float 4  tolAbs of slabSetupSign;
 *   word 5      flags as int32 bits: bit 0 certified; 1 / 2 verdict / undecided of boxHitApprox<false>; 3 / 4 of boxHitApprox<true>;
 *               5 / 6 of boxHitSign<true>; 7 boxMaybeHit; 8 boxHit (the reference's divisions); 9 boxHitLoose; 10 boxHitOrGate with
 *               gate = true: the box judged as an inner node of the path-pool kernel's regrouped tree (closed, and no bound on t,
 *               on an axis with d = +-0);
 *   float 6     tEnter of boxMaybeHit;  float 7  tEnter of boxHitLoose.
 * Refuses n outside [1, 2^20] and null pointers. */
int srtTestRefinedRcp(SrtContext* ctx, int64_t firstBits, int64_t count, uint64_t* out2);
int srtTestSlabVisit(SrtContext* ctx, const float* hCases, int32_t n, float tMin, int32_t certifiedScene, float* hOut);

/* The most recent render-kernel launch: out4 = { 0 node records through the L1, 1 the step-scheduler kernel over the
 * LDS-resident threaded tree (FAITHFUL, node array small enough for a CU's LDS; tunable "lds_tree" = 0 switches it
 * off), 2 the same with the attenuation stacks in LDS as well, 3 the path-pool kernel over the same tree (tunable
 * "wavefront" = 0 switches it off), 4 the path-pool kernel's hybrid form for a tree that does not fit (its top in LDS, the
 * rest read from global memory; tunable "wf_hybrid" = 0 switches it off, "wf_resident_max" caps the resident nodes -- both
 * are read by srtUploadScene); workgroups; threads per workgroup; LDS bytes per workgroup }. */
int srtGetLaunchInfo(SrtContext* ctx, int32_t* out4);

/* Per-context diagnostic tunables of the work distribution and the wave scheduler ("queues", "unit_tiles",
 * "tile_block", "shade_min", "prim_min", "hit_min", "fuse_min", "node_burst", "ploc_radius", "fast_div",
 * "prim_again_min", "keep_eighths", "lds_tree", "chunk_scratch_mb": memory budget of the chunk-slot path of the exact chunk sum, 0 forces the atomic path).  Defaults come from the library (and, for the scheduler thresholds, from SRT_*
 * environment variables read ONCE at srtCreate); none of them changes the image
 * (tests/test_gpu_properties.py::test_image_independent_of_work_distribution).  "tile_block" has no
 * environment override: every rank and the host untile (tiles.py) must agree on it. */
int srtSetTunable(SrtContext* ctx, const char* name, int32_t value);
int srtGetTunable(SrtContext* ctx, const char* name, int32_t* value);

#ifdef __cplusplus
}
#endif
#endif /* SRT_HIP_TEST_H */
