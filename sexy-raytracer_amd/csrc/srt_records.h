// srt_records.h -- the arithmetic that turns caller geometry (SrtTriangleIn, SrtSphereIn) into device records, primitive
// boxes, box unions and the fast-division certificate: ONE statement of each rule for the host (srt_scene.cpp: flattening,
// the reference-order build) and the device (srt_lbvh.hip: builds and pair records; srt_refit.hip: updates and refits).
// Every file that includes this is built with -ffp-contract=off and IEEE division / sqrt, so a record or box made on
// either side carries the same bits.  The reference's operation order is kept throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "srt_device.h"
#include "srt_tri_hit.h"

struct Vec3 {
  float x, y, z;
};
SRT_HD inline Vec3 vec3(const float* p) { return Vec3{p[0], p[1], p[2]}; }
SRT_HD inline Vec3 operator+(Vec3 a, Vec3 b) { return Vec3{a.x + b.x, a.y + b.y, a.z + b.z}; }
SRT_HD inline Vec3 operator-(Vec3 a, Vec3 b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
SRT_HD inline Vec3 operator*(float s, Vec3 a) { return Vec3{s * a.x, s * a.y, s * a.z}; }
SRT_HD inline Vec3 operator/(Vec3 a, float s) { return Vec3{a.x / s, a.y / s, a.z / s}; }
SRT_HD inline bool operator!=(Vec3 a, Vec3 b) { return a.x != b.x || a.y != b.y || a.z != b.z; }
SRT_HD inline Vec3 cross(Vec3 a, Vec3 b) { return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
SRT_HD inline Vec3 unit(Vec3 v) {  // vec3.h:54-60 (lengthSquared: vec3.h:29-31)
  const float len = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
  if (len != 0) return v / len;
  return v;
}

struct Box {
  float mn[3], mx[3];
};
SRT_HD inline Box boxOf(Vec3 lo, Vec3 hi) { return Box{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}}; }

SRT_HD inline Box surrounding(const Box& a, const Box& b) {  // aabb.h:33-43
  Box r;
  for (int k = 0; k < 3; ++k) {
    r.mn[k] = fminf(a.mn[k], b.mn[k]);
    r.mx[k] = fmaxf(a.mx[k], b.mx[k]);
  }
  return r;
}

// fastDiv's operand certificate for the box coordinates (srt_kernels.hip): 0 or 2^-77 <= |c| <= 2^30
SRT_HD inline bool fastDivOperand(float c) {
  const float ac = fabsf(c);
  return c == 0.0f || (ac >= 0x1p-77f && ac <= 0x1p30f);
}
SRT_HD inline bool fastDivOperands(const Box& b) {
  bool ok = true;
  for (int k = 0; k < 3; ++k) ok = ok && fastDivOperand(b.mn[k]) && fastDivOperand(b.mx[k]);
  return ok;
}
// the sign form of the slab test (srt_slab.h) takes the near plane of an axis from the ray's sign: min <= max, both finite
SRT_HD inline bool srtBoxOrdered(const Box& b) {
  bool ok = true;
  for (int k = 0; k < 3; ++k) ok = ok && b.mn[k] <= b.mx[k] && fabsf(b.mn[k]) < INFINITY && fabsf(b.mx[k]) < INFINITY;
  return ok;
}

// ------------------------------------------------------------------ triangles
// p: the nine position floats, uv: the six texture coordinates (SrtTriangleIn's order) -> triTest (vertices, the
// geometric normal in the w words), triShade (unit normal, tangent, bitangent, the uvs, the caller's material word) and
// triFast (the certified test's 64-byte record, srt_tri_hit.h).
SRT_HD inline void triangleRecords(const float* p, const float* uv, float material, float4* test, float4* shade, float4* fast) {
  const Vec3 v0 = vec3(p), v1 = vec3(p + 3), v2 = vec3(p + 6);
  const Vec3 n = cross(v1 - v0, v2 - v0);  // getNormal, model.h:276-283
  test[0] = make_float4(v0.x, v0.y, v0.z, n.x);
  test[1] = make_float4(v1.x, v1.y, v1.z, n.y);
  test[2] = make_float4(v2.x, v2.y, v2.z, n.z);
  const float nf[3] = {n.x, n.y, n.z};
  srtTriFastRecord(p, p + 3, p + 6, nf, fast);
  const Vec3 nu = unit(n);  // model.h:172
  // calcTangentBasis, model.h:214-235
  const Vec3 e0 = v1 - v0, e1 = v2 - v0;
  const float du0 = uv[2] - uv[0], dv0 = uv[3] - uv[1];
  const float du1 = uv[4] - uv[0], dv1 = uv[5] - uv[1];
  float f = (du0 * dv1 - du1 * dv0);
  if (f == 0) f += 1.1920928955078125e-7f;  // std::numeric_limits<float>::epsilon()
  f = 1.0f / f;
  const Vec3 tg = unit(Vec3{f * (dv1 * e0.x - dv0 * e1.x), f * (dv1 * e0.y - dv0 * e1.y), f * (dv1 * e0.z - dv0 * e1.z)});
  const Vec3 bt = unit(Vec3{f * (-du1 * e0.x + du0 * e1.x), f * (-du1 * e0.y + du0 * e1.y), f * (-du1 * e0.z + du0 * e1.z)});
  shade[0] = make_float4(nu.x, nu.y, nu.z, uv[0]);
  shade[1] = make_float4(tg.x, tg.y, tg.z, uv[1]);
  shade[2] = make_float4(bt.x, bt.y, bt.z, uv[2]);
  shade[3] = make_float4(uv[3], uv[4], uv[5], material);
}

// model.h:183-212.  std::min / std::max folded over the vertices in order from +-infinity, as the reference writes it:
// of two zeros of opposite sign the first one seen stays.  An axis without extent is padded by 1e-4 on either side.
SRT_HD inline Box triangleBox(Vec3 v0, Vec3 v1, Vec3 v2) {
  const float v[3][3] = {{v0.x, v0.y, v0.z}, {v1.x, v1.y, v1.z}, {v2.x, v2.y, v2.z}};
  Box b;
  for (int a = 0; a < 3; ++a) {
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    for (int k = 0; k < 3; ++k) {
      mn = v[k][a] < mn ? v[k][a] : mn;
      mx = mx < v[k][a] ? v[k][a] : mx;
    }
    if (mn == mx) {
      mn -= 0.0001f;
      mx += 0.0001f;
    }
    b.mn[a] = mn;
    b.mx[a] = mx;
  }
  return b;
}

// ------------------------------------------------------------------ spheres
#define SRT_SPHERE_MOVING (1 << 30) /* in the material word of a sphere's second record */

// SrtSphereIn's fields -> the three records.  `bits`: the material word; its moving bit follows center0 != center1.
SRT_HD inline void sphereRecords(Vec3 c0, Vec3 c1, float time0, float time1, float radius, int32_t bits, float4* rec) {
  bits = (bits & ~SRT_SPHERE_MOVING) | (c0 != c1 ? SRT_SPHERE_MOVING : 0);
  float word;
  memcpy(&word, &bits, 4);
  rec[0] = make_float4(c0.x, c0.y, c0.z, radius);
  rec[1] = make_float4(c1.x, c1.y, c1.z, word);
  rec[2] = make_float4(time0, time1, 0.0f, 0.0f);
}

// sphere.h:47-52, 85-94: centre -+ radius at both ends of [t0, t1]; st0, st1 are the sphere's own times.
SRT_HD inline Box sphereBox(Vec3 c0, Vec3 c1, bool moving, float st0, float st1, float radius, float t0, float t1) {
  const Vec3 a = moving ? c0 + ((t0 - st0) / (st1 - st0)) * (c1 - c0) : c0;
  const Vec3 b = moving ? c0 + ((t1 - st0) / (st1 - st0)) * (c1 - c0) : c0;
  const Vec3 r{radius, radius, radius};
  return surrounding(boxOf(a - r, a + r), boxOf(b - r, b + r));
}

// ------------------------------------------------------------------ a device reference's box, from the device records
__device__ __forceinline__ void primBox(const DevScene& sc, int ref, float time0, float time1, float* mn, float* mx) {
  const int pr = ~ref;
  Box b;
  if (pr & 1) {
    const float4* sp = sc.spheres + 3 * (pr >> 1);
    const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2];
    b = sphereBox(Vec3{s0.x, s0.y, s0.z}, Vec3{s1.x, s1.y, s1.z}, __float_as_int(s1.w) & SRT_SPHERE_MOVING, s2.x, s2.y, s0.w, time0, time1);
  } else {
    const float4* tr = sc.triTest + 3 * (pr >> 1);
    const float4 q0 = tr[0], q1 = tr[1], q2 = tr[2];
    b = triangleBox(Vec3{q0.x, q0.y, q0.z}, Vec3{q1.x, q1.y, q1.z}, Vec3{q2.x, q2.y, q2.z});
  }
  for (int k = 0; k < 3; ++k) {
    mn[k] = b.mn[k];
    mx[k] = b.mx[k];
  }
}
