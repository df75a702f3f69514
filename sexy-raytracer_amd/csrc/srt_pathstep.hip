// srt_pathstep.hip -- path steps on device buffers (srtCameraRaysDevice, srtScatterRaysDevice, srtPathStepDevice;
// include/srt_hip.h "Path steps on device buffers"): the pieces of the render's per-sample loop -- the camera ray of a
// (pixel, sample), the shading of a hit, and the two fused into one trace-and-shade step -- on the caller's device
// buffers and stream, with the counter RNG's state as a value the caller carries from step to step.
//
// One lane per entry, 256 threads, grid-stride over the entries (the grid is capped like the query kernels').  Nothing
// is restated: the camera ray is srt_path.h's cameraRay() behind the draws of the render kernels' restart step, the
// walk is srt_query_walk.h's (the very walk srt_query_kernel runs), the record is triRecord / sphereRecord and the
// shading is shade().  Lanes of a wave meet different materials in shade(); nothing is sorted or compacted here --
// inactive and finished lanes idle, and compaction between bounces is the caller's choice.

#include "srt_path.h"
#include "srt_query_walk.h"
#include "srt_step_rays.h"
#include "srt_launch.h"

namespace {

// SrtPathOut: two dwordx4 stores
__device__ __forceinline__ void storeOut(int4* out, V3 att, int status, V3 emitted, int prim) {
  out[0] = make_int4(__float_as_int(att.x), __float_as_int(att.y), __float_as_int(att.z), status);
  out[1] = make_int4(__float_as_int(emitted.x), __float_as_int(emitted.y), __float_as_int(emitted.z), prim);
}

// material::scatter and material::emitted on one record whose material is one of the scene's: the outputs of entry i.
// The lane has read its ray before this writes raysOut[i] (raysOut may be the input buffer).
__device__ __forceinline__ void shadeEntry(const DevScene& sc, Rsrc rsTexels, const Ray& r, float tMin, float tMax, const Record& rec,
                                           int prim, uint64_t* rngAt, int4* outAt, float* rayOutAt) {
  Pcg rng;
  rng.state = *rngAt;
  V3 att = mk(0.0f, 0.0f, 0.0f), emitted;
  Ray next;
  next.d = mk(0.0f, 0.0f, 0.0f);
  uint32_t fetches = 0;
  const bool scattered = shade<false, STEP_WIDE>(sc, rsTexels, r, rec, rng, att, next, emitted, fetches);
  *rngAt = rng.state;  // one 8-byte store: advanced by what scatter drew, also where it gave up
  if (scattered) storeRay(rayOutAt, next, tMin, tMax);
  storeOut(outAt, scattered ? att : mk(0.0f, 0.0f, 0.0f), scattered ? SRT_PATH_SCATTERED : SRT_PATH_ENDED, emitted, prim);
}

// ------------------------------------------------------------------ srtCameraRaysDevice
__global__ __launch_bounds__(SRT_BLOCK) void srt_camera_rays_kernel(const CameraRaysArgs a) {
  const uint64_t seedMixed = mix64(a.seed);
  const int64_t numPixels = (int64_t)a.imageWidth * a.imageHeight;
  for (int64_t i = (int64_t)blockIdx.x * SRT_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * SRT_BLOCK) {
    int64_t pixel;
    int32_t sample;
    if (a.pixelSample) {
      pixel = a.pixelSample[2 * i];
      sample = a.pixelSample[2 * i + 1];
    } else {
      pixel = i / a.spp;
      sample = a.sampleFirst + (int32_t)(i - pixel * a.spp);
    }
    if (pixel < 0 || pixel >= numPixels) continue;  // not a pixel of the image: the entry stays as it was
    const int px = (int)(pixel % a.imageWidth), py = (int)(pixel / a.imageWidth);
    Pcg rng;
    rng.key(seedMixed, (uint32_t)pixel, (uint32_t)sample);
    // the restart step's draws and operations (srt_kernels.hip; main.cpp:210-211)
    const float u = ((float)px + rng.uniform()) / (float)(a.imageWidth - 1);
    const float v = ((float)(a.imageHeight - py) + rng.uniform()) / (float)(a.imageHeight - 1);
    Ray r;
    cameraRay(a.cam, u, v, rng, r);
    storeRay(a.rays + 9 * i, r, a.tMin, SRT_INF);
    a.rng[i] = rng.state;
  }
}

// ------------------------------------------------------------------ srtScatterRaysDevice
__global__ __launch_bounds__(SRT_BLOCK) void srt_scatter_device_kernel(const ScatterDeviceArgs a) {
  const DevScene& sc = a.scene;
  const Rsrc rsTexels = makeRsrc(sc.texels, sc.texelBytes);
  for (int64_t i = (int64_t)blockIdx.x * SRT_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * SRT_BLOCK) {
    const SrtHit& h = a.records[i];
    const int prim = h.prim, material = h.material;
    const V3 zero = mk(0.0f, 0.0f, 0.0f);
    if (prim == SRT_NO_HIT) {
      storeOut(a.out + 2 * i, zero, SRT_PATH_MISS, zero, SRT_NO_HIT);
      continue;
    }
    // a caller-made record must not index the shading records out of bounds (the load below is a plain one)
    if (material < 0 || material >= sc.numMaterials) {
      storeOut(a.out + 2 * i, zero, SRT_PATH_INVALID, zero, prim);
      continue;
    }
    Ray r;
    float tMin, tMax;
    loadRay(a.rays + 9 * i, r, tMin, tMax);
    Record rec;  // as srt_scatter_kernel builds it (srt_kernels.hip)
    rec.p = ld3(h.p); rec.normal = ld3(h.normal); rec.tangent = ld3(h.tangent); rec.bitangent = ld3(h.bitangent);
    rec.u = h.uv[0]; rec.v = h.uv[1]; rec.t = h.t; rec.frontFace = h.frontFace != 0; rec.material = material;
    rec.matType = (int)sc.shadeRecs[8 * material].x;  // a hit record has no material word: type | SRT_MAT_TEXTURED from the record
    rec.isTri = false;
    shadeEntry(sc, rsTexels, r, tMin, tMax, rec, prim, a.rng + i, a.out + 2 * i, a.raysOut + 9 * i);
  }
}

// ------------------------------------------------------------------ srtPathStepDevice
// MODE: Q_FAITHFUL or Q_CLOSEST.  The query kernel's walk, then the record -- uv and the tangent frame only where the
// primitive's material word says the material reads them, as in the render kernels' hit step -- then shade().
template <int MODE>
__global__ __launch_bounds__(SRT_BLOCK) void srt_path_step_kernel(const PathStepArgs a) {
  extern __shared__ int32_t lds[];
  const DevScene& sc = a.scene;
  const QueryWalk walk = queryWalkSetup<MODE>(sc, lds);  // [slot][thread]: stackDepth + 2 slots
  const Rsrc rsTexels = makeRsrc(sc.texels, sc.texelBytes);
  for (int64_t i = (int64_t)blockIdx.x * SRT_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * SRT_BLOCK) {
    if (a.active && a.active[i] == 0) continue;  // reads nothing but its byte, writes nothing
    Ray r;
    float tMin, tMax;
    loadRay(a.rays + 9 * i, r, tMin, tMax);
    float closest;
    bool found;
    const int hitRef = queryWalk<MODE>(sc, walk, r, tMin, tMax, closest, found);
    const V3 zero = mk(0.0f, 0.0f, 0.0f);
    if (hitRef == SRT_REF_DONE) {
      if (a.hits) a.hits[i] = make_int4(SRT_NO_HIT, 0, -1, 0);
      storeOut(a.out + 2 * i, zero, SRT_PATH_MISS, zero, SRT_NO_HIT);
      continue;
    }
    Record rec;
    const int pr = ~hitRef;
    int prim;
    if (pr & 1) {
      sphereRecord(sc, pr >> 1, r, closest, rec, false);
      prim = sc.sphPrimId[pr >> 1];
    } else {
      triRecord(sc, pr >> 1, r, closest, rec, false);
      prim = sc.triPrimId[pr >> 1];
    }
    if (a.hits) a.hits[i] = make_int4(prim, __float_as_int(rec.t), rec.material, rec.frontFace ? 1 : 0);  // one dwordx4 store
    if (rec.material >= sc.numMaterials) {  // what srtScatterRaysDevice makes of such a record
      storeOut(a.out + 2 * i, zero, SRT_PATH_INVALID, zero, prim);
      continue;
    }
    shadeEntry(sc, rsTexels, r, tMin, tMax, rec, prim, a.rng + i, a.out + 2 * i, a.raysOut + 9 * i);
  }
}

}  // namespace

extern "C" {

int srt_launch_camera_rays(const CameraRaysArgs* a, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(srt_camera_rays_kernel, dim3(grid), dim3(SRT_BLOCK), 0, stream, *a);
  return (int)hipGetLastError();
}

int srt_launch_scatter_device(const ScatterDeviceArgs* a, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(srt_scatter_device_kernel, dim3(grid), dim3(SRT_BLOCK), 0, stream, *a);
  return (int)hipGetLastError();
}

// traversal: SRT_TRAVERSE_FAITHFUL or SRT_TRAVERSE_CLOSEST; ldsBytes: the walk's stacks, as srt_launch_query's
int srt_launch_path_step(const PathStepArgs* a, int traversal, int grid, size_t ldsBytes, hipStream_t stream) {
  void (*kernel)(const PathStepArgs) = traversal == SRT_TRAVERSE_CLOSEST ? srt_path_step_kernel<Q_CLOSEST> : srt_path_step_kernel<Q_FAITHFUL>;
  if (ldsBytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SRT_BLOCK), ldsBytes, stream, *a);
  return (int)hipGetLastError();
}

}  // extern "C"
