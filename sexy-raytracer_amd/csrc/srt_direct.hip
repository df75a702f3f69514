// srt_direct.hip -- direct light sampling on device buffers (include/srt_hip.h "Direct light sampling"): the per-hit
// direct term for user-land loops (srtDirectLightDevice) and the test hook that evaluates a pbr material's attenuation for
// a direction of the caller's (include/srt_hip_test.h srtTestEvalScatterDevice).
//
// One lane per entry, 256 threads, grid-stride over the entries, as srt_pathstep.hip's kernels.  Nothing is restated: the
// record is read as srt_scatter_device_kernel reads it, the term is srt_direct.h's directTerm (which the DIRECT instances of
// srt_paths.hip call as well), its shadow ray is walked by srt_query_walk.h's queryWalk and the attenuation is srt_path.h's
// pbrAttenuation, the very statement shade() evaluates.

#include "srt_path.h"
#include "srt_query_walk.h"
#include "srt_step_rays.h"
#include "srt_direct.h"
#include "srt_launch.h"

namespace {

// a hit record as srt_scatter_device_kernel makes it; false for a miss and for a material that is not one of the scene's
__device__ __forceinline__ bool recordOf(const DevScene& sc, const SrtHit& h, Record& rec) {
  const int material = h.material;
  if (h.prim == SRT_NO_HIT || material < 0 || material >= sc.numMaterials) return false;
  rec.p = ld3(h.p); rec.normal = ld3(h.normal); rec.tangent = ld3(h.tangent); rec.bitangent = ld3(h.bitangent);
  rec.u = h.uv[0]; rec.v = h.uv[1]; rec.t = h.t; rec.frontFace = h.frontFace != 0; rec.material = material;
  rec.matType = (int)sc.shadeRecs[8 * material].x;
  rec.isTri = false;
  return true;
}

// SrtDirectOut: two dwordx4 stores
__device__ __forceinline__ void storeDirect(int4* out, V3 radiance, int light, V3 dir, float weight) {
  out[0] = make_int4(__float_as_int(radiance.x), __float_as_int(radiance.y), __float_as_int(radiance.z), light);
  out[1] = make_int4(__float_as_int(dir.x), __float_as_int(dir.y), __float_as_int(dir.z), __float_as_int(weight));
}

// ------------------------------------------------------------------ srtDirectLightDevice
template <int MODE>
__global__ __launch_bounds__(SRT_BLOCK) void srt_direct_light_kernel(const DirectLightArgs a) {
  extern __shared__ int32_t lds[];
  const DevScene& sc = a.scene;
  const QueryWalk walk = queryWalkSetup<MODE>(sc, lds);  // [slot][thread]: stackDepth + 2 slots
  const Rsrc rsTexels = makeRsrc(sc.texels, sc.texelBytes);
  const V3 zero = mk(0.0f, 0.0f, 0.0f);
  for (int64_t i = (int64_t)blockIdx.x * SRT_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * SRT_BLOCK) {
    Record rec;
    if (a.numLights <= 0 || !recordOf(sc, a.records[i], rec) || !directSamples(sc, rec)) {
      storeDirect(a.direct + 2 * i, zero, -1, zero, 0.0f);
      continue;
    }
    Ray r;
    float tMin, tMax;
    loadRay(a.rays + 9 * i, r, tMin, tMax);
    const DirectTerm d = directTerm<MODE, STEP_WIDE>(sc, walk, rsTexels, a.lights, a.numLights, r, tMin, tMax, rec, a.rng[i]);
    storeDirect(a.direct + 2 * i, d.radiance, d.light < 0 ? -1 : sc.sphPrimId[a.lights[d.light]], d.dir, d.weight);
  }
}

// ------------------------------------------------------------------ srtTestEvalScatterDevice
__global__ __launch_bounds__(SRT_BLOCK) void srt_eval_scatter_kernel(const EvalScatterArgs a) {
  const DevScene& sc = a.scene;
  const Rsrc rsTexels = makeRsrc(sc.texels, sc.texelBytes);
  for (int64_t i = (int64_t)blockIdx.x * SRT_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * SRT_BLOCK) {
    Record rec;
    V3 att = mk(0.0f, 0.0f, 0.0f);
    if (recordOf(sc, a.records[i], rec) && directSamples(sc, rec)) {
      Ray r;
      float tMin, tMax;
      loadRay(a.rays + 9 * i, r, tMin, tMax);
      att = pbrAttenuation(pbrInputsOf<STEP_WIDE>(sc, rsTexels, rec), r.d, ld3(a.dirs + 3 * i));
    }
    a.att[3 * i] = att.x;
    a.att[3 * i + 1] = att.y;
    a.att[3 * i + 2] = att.z;
  }
}

// ------------------------------------------------------------------ srtRenderDirectImage's running sum
// One lane per pixel: the pixel's `count` results of a pixel-major batch (entry pixel * count + k) are added to its float4
// sum in sample-index order, one float addition per channel and sample as main.cpp:217 adds them; w counts the samples.
__global__ __launch_bounds__(SRT_BLOCK) void srt_direct_sum_kernel(const int4* result, float4* accum, int64_t numPixels, int32_t count) {
  for (int64_t pixel = (int64_t)blockIdx.x * SRT_BLOCK + threadIdx.x; pixel < numPixels; pixel += (int64_t)gridDim.x * SRT_BLOCK) {
    float4 sum = accum[pixel];
    for (int32_t k = 0; k < count; ++k) {
      const int4 r = result[pixel * count + k];
      sum.x = sum.x + __int_as_float(r.x);
      sum.y = sum.y + __int_as_float(r.y);
      sum.z = sum.z + __int_as_float(r.z);
      sum.w = sum.w + 1.0f;
    }
    accum[pixel] = sum;
  }
}

}  // namespace

extern "C" {

int srt_launch_direct_sum(const int4* result, float4* accum, int64_t numPixels, int32_t count, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(srt_direct_sum_kernel, dim3(grid), dim3(SRT_BLOCK), 0, stream, result, accum, numPixels, count);
  return (int)hipGetLastError();
}

int srt_launch_direct_light(const DirectLightArgs* a, int traversal, int grid, size_t ldsBytes, hipStream_t stream) {
  void (*kernel)(const DirectLightArgs) = traversal == SRT_TRAVERSE_CLOSEST ? srt_direct_light_kernel<Q_CLOSEST> : srt_direct_light_kernel<Q_FAITHFUL>;
  if (ldsBytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SRT_BLOCK), ldsBytes, stream, *a);
  return (int)hipGetLastError();
}

int srt_launch_eval_scatter(const EvalScatterArgs* a, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(srt_eval_scatter_kernel, dim3(grid), dim3(SRT_BLOCK), 0, stream, *a);
  return (int)hipGetLastError();
}

}  // extern "C"
