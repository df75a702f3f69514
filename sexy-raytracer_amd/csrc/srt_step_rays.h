// srt_step_rays.h -- what the kernels over the caller's ray buffers share beside the walk: how a 36-byte SrtRay row moves
// between memory and a lane, and the instance of shade() they run.  Included by srt_pathstep.hip (one step per launch) and
// srt_paths.hip (whole paths per launch), after srt_path.h.  Internal.
#ifndef SRT_STEP_RAYS_H
#define SRT_STEP_RAYS_H

#include "srt_path.h"

namespace {

// The instance of shade() these kernels run: one texel lookup after the other.  With all four in flight (WIDE) the step
// kernel takes 81 vector registers, one past the 80 that still fit six waves per SIMD; this instance takes 78 (`make
// resource-usage`).  Both instances compute the same bits (tests/test_shading.py).
constexpr bool STEP_WIDE = false;

__device__ __forceinline__ void loadRay(const float* in, Ray& r, float& tMin, float& tMax) {
  r.o = mk(in[0], in[1], in[2]);  // nine dword loads 36 bytes apart per lane
  r.d = mk(in[3], in[4], in[5]);
  r.time = in[6];
  tMin = in[7];
  tMax = in[8];
}
__device__ __forceinline__ void storeRay(float* out, const Ray& r, float tMin, float tMax) {
  out[0] = r.o.x; out[1] = r.o.y; out[2] = r.o.z;
  out[3] = r.d.x; out[4] = r.d.y; out[5] = r.d.z;
  out[6] = r.time;
  out[7] = tMin;
  out[8] = tMax;
}

}  // namespace

#endif
