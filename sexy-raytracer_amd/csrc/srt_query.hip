// srt_query.hip -- ray queries on device buffers (srtTraceRaysDevice, srtOccludedDevice; include/srt_hip.h "Ray
// queries"): rays that a kernel or a torch op left in device memory, answered in device memory on the caller's stream.
//
// One lane per ray, grid-stride over the ray set (the grid is capped at a few workgroups per CU, like srtTraceRays's).
// The walks themselves (FAITHFUL, CLOSEST, ANY) are srt_query_walk.h's, shared with the fused path step (srt_pathstep.hip).
// No wave scheduler here (the render kernels' step kinds): a query has no shading or restart step to batch, and its
// divergence is the node / primitive alternation of one loop.

#include "srt_path.h"
#include "srt_query_walk.h"
#include "srt_launch.h"

// Measurement switch (tools/query_bench.py through an experimental build); the library ships with 0.
#ifndef SRT_QUERY_LDS_RAYS
#define SRT_QUERY_LDS_RAYS 0  // 1: a workgroup's rays loaded as coalesced dwords and transposed through LDS
#endif

namespace {

template <int MODE>
__global__ __launch_bounds__(SRT_BLOCK) void srt_query_kernel(const QueryArgs a) {
  extern __shared__ int32_t lds[];
  const DevScene& sc = a.scene;
  const QueryWalk walk = queryWalkSetup<MODE>(sc, lds);  // [slot][thread]: stackDepth + 2 slots

  // every lane of a workgroup takes the same number of trips (the staged ray load below has barriers in it)
  for (int64_t base = (int64_t)blockIdx.x * SRT_BLOCK; base < a.n; base += (int64_t)gridDim.x * SRT_BLOCK) {
    const int64_t i = base + threadIdx.x;
#if SRT_QUERY_LDS_RAYS
    // the workgroup's 256 rays are 2 304 contiguous dwords: loaded coalesced, transposed through LDS (a lane's nine words
    // are 9 dwords apart: an odd stride, no bank conflicts)
    float* const staged = reinterpret_cast<float*>(lds + (sc.stackDepth + 2) * SRT_BLOCK);
    const int words = (int)(a.n - base < SRT_BLOCK ? a.n - base : SRT_BLOCK) * 9;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int at = k * SRT_BLOCK + threadIdx.x;
      if (at < words) staged[at] = a.rays[9 * base + at];
    }
    __syncthreads();
    if (i >= a.n) continue;
    const float* in = staged + 9 * threadIdx.x;
#else
    if (i >= a.n) continue;
    const float* in = a.rays + 9 * i;  // nine dword loads 36 bytes apart per lane
#endif
    Ray r;
    r.o = mk(in[0], in[1], in[2]);
    r.d = mk(in[3], in[4], in[5]);
    r.time = in[6];
    const float tMin = in[7], tMax = in[8];
    float closest;
    bool found;
    const int hitRef = queryWalk<MODE>(sc, walk, r, tMin, tMax, closest, found);
    if (MODE == Q_ANY) {
      a.occluded[i] = found ? 1 : 0;
      continue;
    }

    if (MODE != Q_ANY) {
      int4 h4 = make_int4(SRT_NO_HIT, 0, -1, 0);
      // (srt_trace_kernel's fill, written out: as one inlined function it changed the code of both kernels)
      SrtHit h;
      h.prim = SRT_NO_HIT;
      h.t = 0;
      for (int k = 0; k < 3; ++k) h.p[k] = h.normal[k] = h.tangent[k] = h.bitangent[k] = 0;
      h.uv[0] = h.uv[1] = 0;
      h.frontFace = 0;
      h.material = -1;
      h.nodeVisits = h.boxPasses = h.triTests = h.sphereTests = 0;
      if (hitRef != SRT_REF_DONE) {
        Record rec;
        const int pr = ~hitRef;
        const bool all = a.records != nullptr;  // uv and the tangent frame only where the full record is asked for
        if (pr & 1) {
          sphereRecord(sc, pr >> 1, r, closest, rec, all);
          h.prim = sc.sphPrimId[pr >> 1];
        } else {
          triRecord(sc, pr >> 1, r, closest, rec, all);
          h.prim = sc.triPrimId[pr >> 1];
        }
        h.t = rec.t;
        h.p[0] = rec.p.x; h.p[1] = rec.p.y; h.p[2] = rec.p.z;
        h.normal[0] = rec.normal.x; h.normal[1] = rec.normal.y; h.normal[2] = rec.normal.z;
        h.tangent[0] = rec.tangent.x; h.tangent[1] = rec.tangent.y; h.tangent[2] = rec.tangent.z;
        h.bitangent[0] = rec.bitangent.x; h.bitangent[1] = rec.bitangent.y; h.bitangent[2] = rec.bitangent.z;
        h.uv[0] = rec.u; h.uv[1] = rec.v;
        h.frontFace = rec.frontFace ? 1 : 0;
        h.material = rec.material;
        h4 = make_int4(h.prim, __float_as_int(h.t), h.material, h.frontFace);
      }
      if (a.hits) a.hits[i] = h4;  // one dwordx4 store
      if (a.records) a.records[i] = h;
    }
  }
}

}  // namespace

extern "C" {

// mode: SRT_TRAVERSE_FAITHFUL, SRT_TRAVERSE_CLOSEST, or 2 = any hit (a->occluded).  Allocates nothing, waits for nothing.
int srt_launch_query(const QueryArgs* a, int mode, int grid, size_t ldsBytes, hipStream_t stream) {
  void (*kernel)(const QueryArgs) = mode == Q_ANY ? srt_query_kernel<Q_ANY> : mode == Q_CLOSEST ? srt_query_kernel<Q_CLOSEST> : srt_query_kernel<Q_FAITHFUL>;
  if (SRT_QUERY_LDS_RAYS) ldsBytes += 9 * SRT_BLOCK * sizeof(float);
  if (ldsBytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SRT_BLOCK), ldsBytes, stream, *a);
  return (int)hipGetLastError();
}

}  // extern "C"
