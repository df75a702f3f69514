// srt_launch.h -- every C-linkage function a kernel file (.hip) defines and a host file (.cpp) calls, declared once.  The
// defining file and every caller include this header: C linkage does not mangle the parameter types into the symbol, so a
// definition that disagrees with a caller's idea of it would link and pass garbage; seen by both, it is "conflicting
// types" at compile time.  Each returns a hipError_t as int (0 = launched) unless it says otherwise.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include "srt_device.h"

extern "C" {

// srt_kernels.hip / srt_wavefront.hip: the instance of the render kernel a plan names (forms 0-2 / forms 3 and 4)
RenderKernel srt_render_kernel_for(const RenderPlan* p);
RenderKernel srt_render_wf_kernel_for(const RenderPlan* p);

// srt_kernels.hip
int srt_launch_finalize(const SrtFixedAccum* fix, float4* out, int n, int samples, hipStream_t stream);
int srt_launch_sum_chunks(const float4* buf, float4* out, int n, int chunks, float limit, hipStream_t stream);
int srt_launch_test_commit(const float4* buf, SrtFixedAccum* fix, int n, int chunks, float limit, hipStream_t stream);
int srt_launch_resolve(const ResolveArgs* a, hipStream_t stream);
int srt_launch_trace(const TraceArgs* a, int traversal, int grid, size_t ldsBytes, hipStream_t stream);
int srt_launch_scatter(const DevScene* sc, const SrtRay* rays, const SrtHit* hits, float* out, uint32_t* fetches, uint64_t seed,
                       int n, int form, hipStream_t stream);

// srt_query.hip: mode = SRT_TRAVERSE_FAITHFUL, SRT_TRAVERSE_CLOSEST or 2 (any hit, into a->occluded)
int srt_launch_query(const QueryArgs* a, int mode, int grid, size_t ldsBytes, hipStream_t stream);

// srt_slabtest.hip: the test hooks on the certified slab test (include/srt_hip_test.h srtTestRefinedRcp, srtTestSlabVisit).
// partial: 2 * SRT_SLABTEST_RCP_WAVES words, per wave {the bits of its largest |r d - 1| as a double, -1 for none; the pattern}
#define SRT_SLABTEST_RCP_WAVES 4096
int srt_launch_slabtest_rcp(uint32_t firstBits, int64_t count, unsigned long long* partial, hipStream_t stream);
int srt_launch_slabtest_visit(const float* cases, int n, float tMin, int certifiedScene, float* out, hipStream_t stream);

// srt_pathstep.hip: one kernel each; traversal = SRT_TRAVERSE_FAITHFUL or SRT_TRAVERSE_CLOSEST, ldsBytes as srt_launch_query's
int srt_launch_camera_rays(const CameraRaysArgs* a, int grid, hipStream_t stream);
int srt_launch_scatter_device(const ScatterDeviceArgs* a, int grid, hipStream_t stream);
int srt_launch_path_step(const PathStepArgs* a, int traversal, int grid, size_t ldsBytes, hipStream_t stream);

// What srtCompactPathsDevice and srtSortPathsDevice have in common: the predicate, the payloads in and out, the count.  The
// host fills and checks it in one place (srt_rays.cpp); srt_payloads.h holds the keep rule and the move of one entry.
struct PathPayloads {
  const int32_t* out;     // SrtPathOut[n] as dwords (the status is dword 3 of 8), or null
  const uint8_t* active;  // or null; compaction: not both.  The sort: both null keeps every entry
  const uint32_t* rays;   // payloads in: read only where the output beside them is not null (the sort's key always reads the rays)
  const uint64_t* rng;
  const int32_t* slot;    // null with slotOut: the identity
  uint32_t* raysOut;      // payloads out, each or null
  uint64_t* rngOut;
  int32_t* slotOut;
  uint8_t* activeOut;     // or null; may be `active`
  int64_t* count;
  int64_t n;
};

// srt_compact.hip (srtCompactPathsDevice): count, scan and scatter, three kernels on the stream; grid = the workgroups of
// the first and the last.  The scan is one workgroup of SRT_COMPACT_SCAN_BLOCK threads, a tile count each per trip.
#define SRT_COMPACT_SCAN_BLOCK 1024
struct CompactArgs {
  PathPayloads p;
  uint64_t* tileOffset;  // the caller's scratch: numTiles words
  int64_t numTiles;
};
int srt_launch_compact(const CompactArgs* a, int grid, hipStream_t stream);

// srt_sort.hip (srtSortPathsDevice): a memset of *count, the key kernel, rocPRIM's radix sort over (key, index) between the
// two halves of the scratch, and the gather kernel, all on the stream; grid = the workgroups of the two kernels.
// srt_sort_temp_bytes: what that sort asks for as temporary storage at this n and cellBits (host only, launches nothing).
struct SortArgs {
  PathPayloads p;    // rays required: the key reads the origin and the direction's sign bits
  uint32_t *keys, *keysSpare, *index, *indexSpare;  // the caller's scratch: n words each
  void* temp;        // and the sort's temporary storage behind them
  size_t tempBytes;
  const float* box;  // lo.xyz, hi.xyz on the device
  int32_t cellBits;
};
int srt_sort_temp_bytes(int64_t n, int cellBits, hipStream_t stream, size_t* bytes);
int srt_launch_sort(const SortArgs* a, int grid, hipStream_t stream);

// srt_paths.hip (srtTracePathsDevice): one memset of the counter and ONE persistent kernel on the stream.  The grid is
// the smaller of ceil(n / SRT_BLOCK) and numCUs * the workgroups of the kernel a CU holds at ldsBytes of dynamic LDS
// (srtPathsLdsBytes); no workgroup waits for another one, so a grid the device holds only in part is merely slower.
struct TracePathsArgs {
  DevScene scene;
  const float* rays;            // SrtRay[n]: read only
  uint64_t* rng;                // Pcg::state per entry: read when an entry is claimed, written when its path ends
  int4* result;                 // SrtPathRadiance[n]
  unsigned long long* counter;  // the next entry to claim: the first word of the caller's scratch, zeroed by the memset
  float background[3];
  int32_t maxBounce;
  int32_t refillMin;            // idle lanes of a wave before it claims entries, 1..64 (tunable paths_refill_min)
  int64_t n;
};
int srt_launch_paths(const TracePathsArgs* a, int traversal, int numCUs, size_t ldsBytes, size_t scratchBytes, hipStream_t stream);
// ... and its DIRECT instances (srtTracePathsDirectDevice): the same launch with the sampled-light table beside the plain
// arguments -- DevScene and TracePathsArgs stay as they are -- and ldsBytes = srtPathsDirectLdsBytes
struct TracePathsDirectArgs {
  TracePathsArgs p;
  const int32_t* lights;  // device sphere indices of the sampled lights, prims[] order (Upload::sampledLights)
  int32_t numLights;
};
int srt_launch_paths_direct(const TracePathsDirectArgs* a, int traversal, int numCUs, size_t ldsBytes, size_t scratchBytes, hipStream_t stream);

// srt_direct.hip (srtDirectLightDevice, srtTestEvalScatterDevice): one kernel each, one lane per entry; every pointer is the
// caller's DEVICE memory but `lights`.  traversal and ldsBytes as srt_launch_path_step's
struct DirectLightArgs {
  DevScene scene;
  const float* rays;       // SrtRay[n]
  const SrtHit* records;   // SrtHit[n]
  const uint64_t* rng;     // read only: the state before the hit's scatter draws
  int4* direct;            // SrtDirectOut[n] as two int4 per entry
  const int32_t* lights;   // as TracePathsDirectArgs::lights
  int32_t numLights;
  int64_t n;
};
int srt_launch_direct_light(const DirectLightArgs* a, int traversal, int grid, size_t ldsBytes, hipStream_t stream);
struct EvalScatterArgs {
  DevScene scene;
  const float* rays;
  const SrtHit* records;
  const float* dirs;  // float[n][3]: the scattered direction to evaluate
  float* att;         // float[n][3]
  int64_t n;
};
int srt_launch_eval_scatter(const EvalScatterArgs* a, int grid, hipStream_t stream);
// srtRenderDirectImage: the `count` SrtPathRadiance of every pixel of a pixel-major batch added to its float4 sum in order
int srt_launch_direct_sum(const int4* result, float4* accum, int64_t numPixels, int32_t count, int grid, hipStream_t stream);

// srt_lbvh.hip: the device tree builders (blocking) and the closest-hit traversal's pair records
int srt_lbvh_build(const DevScene* sc, const int32_t* dRefs, int n, float time0, float time1, float4* outNodes,
                   uint8_t* outAxis, int base, int* depthOut);
int srt_ploc_build(const DevScene* sc, const int32_t* dRefs, int n, float time0, float time1, float4* outNodes,
                   uint8_t* outAxis, int base, int radius, int* depthOut);
int srt_pair_nodes(const DevScene* sc, float time0, float time1, float4* out);
int srt_pair_nodes_async(const DevScene* sc, float time0, float time1, float4* out, hipStream_t stream);

// srt_refit.hip
int srt_launch_refit_triangles(const void* dIn, int first, int count, const int32_t* devIndex, float4* triTest, float4* triShade,
                               float4* triFast, hipStream_t stream);
int srt_launch_refit_spheres(const void* dIn, int first, int count, float4* spheres, hipStream_t stream);
int srt_launch_refit_links(const float4* nodes, int numNodes, int32_t* up, hipStream_t stream);
int srt_launch_refit_nodes(const DevScene* sc, int base, int count, float time0, float time1, const int32_t* up, int32_t* arrived,
                           int32_t* flag, int checkPrims, hipStream_t stream);
int srt_launch_refit_derived(const DevScene* sc, const int32_t* wfIndex, int32_t* flag, hipStream_t stream);
// srtGetTreeCost: one level of the pairwise sum each, SRT_COST_BLOCK values per workgroup (a power of two)
#define SRT_COST_BLOCK 256
int srt_launch_tree_cost_nodes(const float4* itemNodes, int count, double* out, hipStream_t stream);
int srt_launch_tree_cost_partials(const double* in, int count, double* out, hipStream_t stream);

// srt_features.hip, srt_features_list.hip: the kernel's workgroup size and workgroups per CU, then its launch
int srt_features_plan(int closest, int ldsTree, size_t lds, int* block, int* perCU);
int srt_launch_features(const FeatureArgs* a, int closest, int ldsTree, int grid, size_t lds, hipStream_t stream);
int srt_features_list_plan(int closest, int ldsTree, int accumulate, size_t lds, int* block, int* perCU);
int srt_launch_features_list(const FeatureListArgs* a, int closest, int ldsTree, int accumulate, int grid, size_t lds,
                             hipStream_t stream);

// srt_motion.hip: as srt_features.hip's pair
int srt_motion_plan(int closest, int ldsTree, size_t lds, int* block, int* perCU);
int srt_launch_motion(const MotionArgs* a, int closest, int ldsTree, int grid, size_t lds, hipStream_t stream);

// srt_denoise.hip
int srt_launch_denoise(const DenoiseArgs* a, int iterations, int ldsMaxStep, hipStream_t stream);

// srt_adaptive.hip
int srt_launch_adaptive_update(const uint32_t* list, int count, const float4* beautyTiles, const float4* momentTiles,
                               float4* accum, float4* moments, int32_t* flags, int width, int height, double limit,
                               bool accumulate, bool decide, hipStream_t stream);
int srt_launch_adaptive_compact(const uint32_t* list, const int32_t* flags, int count, uint32_t* out, int32_t* counts,
                                int width, int height, hipStream_t stream);
int srt_launch_adaptive_resolve(const float4* accum, uint8_t* rgba, int n, hipStream_t stream);

// srt_temporal.hip, srt_temporal_adaptive.hip
int srt_launch_temporal(const TemporalArgs* a, hipStream_t stream);
int srt_launch_temporal_reproject(const TemporalArgs* a, hipStream_t stream);
int srt_launch_temporal_adaptive_update(const uint32_t* list, int count, const float4* beautyTiles, const float4* momentTiles,
                                        float4* accum, float4* moments, const float4* reprojected, const float4* albedo,
                                        int32_t* flags, int width, int height, double limit, bool accumulate,
                                        hipStream_t stream);

}  // extern "C"
