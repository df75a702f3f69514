// srt_prim_box.h -- a primitive's bounding box on the device, by the reference's boundingBox rules (model.h:183-212 incl.
// the +-1e-4 padding of flat axes; sphere.h:85-94 incl. motion over [time0, time1]), read from the device records.  Shared
// by the device tree builders, the closest-hit pair records (srt_lbvh.hip) and the refit (srt_refit.hip): one restatement,
// so that a refit box carries the bits a build of the same records gives.
#pragma once
#include <hip/hip_runtime.h>

#include "srt_device.h"

__device__ __forceinline__ void primBox(const DevScene& sc, int ref, float time0, float time1, float* mn, float* mx) {
  int pr = ~ref;
  if (pr & 1) {  // sphere.h:85-94
    const float4* sp = sc.spheres + 3 * (pr >> 1);
    float4 s0 = sp[0], s1 = sp[1], s2 = sp[2];
    float c0[3] = {s0.x, s0.y, s0.z}, c1[3] = {s1.x, s1.y, s1.z};
    bool moving = __float_as_int(s1.w) & (1 << 30);
    for (int k = 0; k < 3; ++k) {
      float a = c0[k], b = c0[k];
      if (moving) {
        a = c0[k] + ((time0 - s2.x) / (s2.y - s2.x)) * (c1[k] - c0[k]);
        b = c0[k] + ((time1 - s2.x) / (s2.y - s2.x)) * (c1[k] - c0[k]);
      }
      mn[k] = fminf(a - s0.w, b - s0.w);
      mx[k] = fmaxf(a + s0.w, b + s0.w);
    }
  } else {  // model.h:183-212
    const float4* tr = sc.triTest + 3 * (pr >> 1);
    float4 q0 = tr[0], q1 = tr[1], q2 = tr[2];
    float v[3][3] = {{q0.x, q0.y, q0.z}, {q1.x, q1.y, q1.z}, {q2.x, q2.y, q2.z}};
    for (int k = 0; k < 3; ++k) {
      mn[k] = fminf(v[0][k], fminf(v[1][k], v[2][k]));
      mx[k] = fmaxf(v[0][k], fmaxf(v[1][k], v[2][k]));
      if (mn[k] == mx[k]) {
        mn[k] -= 0.0001f;
        mx[k] += 0.0001f;
      }
    }
  }
}
