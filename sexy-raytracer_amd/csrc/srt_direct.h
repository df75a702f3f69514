// srt_direct.h -- the direct-light term of a pbr hit (include/srt_hip.h "Direct light sampling"): one of the scene's
// sampled lights is chosen, a direction inside the cone it subtends is drawn, the shadow ray is walked with the path's own
// traversal and the material's attenuation is evaluated for that direction.  Stated once for srt_direct.hip (the per-hit
// entry and the test hook) and srt_paths.hip (the DIRECT instances of the whole-path kernel).  The header fixes every
// operation and its association; tests/direct_ref.py replays the draws and the cone in NumPy float32.  Included after
// srt_path.h and srt_query_walk.h.  Internal.
#ifndef SRT_DIRECT_H
#define SRT_DIRECT_H

#include "srt_path.h"
#include "srt_query_walk.h"

namespace {

#define SRT_DIRECT_RNG_SALT 0x5DEECE66D2545F49ull

// what one evaluation leaves: SrtDirectOut with the light as a row of the table (-1: nothing was sampled)
struct DirectTerm {
  V3 radiance;
  int light;
  V3 dir;
  float weight;
};

// is this record's material a pbr one of the scene's?  (matType: the record's type bits, SRT_MAT_* | SRT_MAT_TEXTURED)
__device__ __forceinline__ bool directSamples(const DevScene& sc, const Record& rec) {
  return !(rec.material < 0) && !(rec.material >= sc.numMaterials) && (rec.matType & 3) == SRT_MAT_PBR;
}

// the material inputs of a pbr record, as shade() loads them ahead of its switch
template <bool WIDE>
__device__ __forceinline__ PbrInputs pbrInputsOf(const DevScene& sc, Rsrc rsTexels, const Record& rec) {
  const Rsrc rsMat = makeRsrc(sc.shadeRecs, sc.numMaterials * 128);
  const int at = rec.material * 128;
  const u32x4 head = __builtin_amdgcn_raw_buffer_load_b128(rsMat, at, 0, 0);
  const float4 albedo = bufLoad4(rsMat, at + 16);
  uint32_t fetches = 0;
  return pbrInputs<false, WIDE>(sc, rsTexels, rsMat, at, rec, albedo, __uint_as_float(head.z), __uint_as_float(head.w), fetches);
}

// Is sphere `idx` (a device index) one a hit's direct term could have chosen from origin o: a solid-colour light that does
// not move, seen from outside?  The drop rule of the whole-path entry asks this of the sphere a bounced ray hit.
__device__ __forceinline__ bool directCouldChoose(const DevScene& sc, int idx, V3 o) {
  const float4 s0 = sc.spheres[3 * idx], s1 = sc.spheres[3 * idx + 1];
  const int word = __float_as_int(s1.w);
  const int material = word & SRT_MAT_INDEX_MASK;
  if (((word >> SRT_MAT_TYPE_SHIFT) & 3) != SRT_MAT_LIGHT || material >= sc.numMaterials) return false;
  if (sc.shadeRecs[8 * material + 2].x != SRT_SLOT_SOLID) return false;
  if (word & (1 << 30)) return false;
  return lenSq(mk(s0.x, s0.y, s0.z) - o) > s0.w * s0.w;
}

// Steps 1-6 of the header at the hit x = rec.p of ray r, with the path's generator state `s` before the hit's scatter
// draws (not advanced: the term has a generator of its own).  lights: numLights > 0 device sphere indices, prims[] order.
template <int MODE, bool WIDE>
__device__ __forceinline__ DirectTerm directTerm(const DevScene& sc, const QueryWalk& walk, Rsrc rsTexels, const int32_t* lights, int numLights,
                                                 const Ray& r, float tMin, float tMax, const Record& rec, uint64_t s) {
  const V3 zero = mk(0.0f, 0.0f, 0.0f);
  DirectTerm out = {zero, -1, zero, 0.0f};
  const V3 x = rec.p;
  Pcg g;
  g.state = mix64(s ^ SRT_DIRECT_RNG_SALT);                          // 1
  const float u = g.uniform();                                       // 2
  const int k = min((int)(u * (float)numLights), numLights - 1);
  const int idx = lights[k];
  const float4 s0 = sc.spheres[3 * idx], s1 = sc.spheres[3 * idx + 1];
  const V3 c = mk(s0.x, s0.y, s0.z);
  const float radius = s0.w;
  const V3 toC = c - x;
  const float d2 = lenSq(toC);
  const float r2 = radius * radius;
  if ((__float_as_int(s1.w) & (1 << 30)) || d2 <= r2) return out;
  const PbrInputs m = pbrInputsOf<WIDE>(sc, rsTexels, rec);  // the texture look-ups: only where something is sampled
  float a, b;                                                        // 3
  g.inUnitDisk(a, b);
  const float sD = a * a + b * b;
  const float q = r2 / d2;
  const float oneMinus = q / (1.0f + sqrtf(1.0f - q));
  const float mm = sD * oneMinus;
  const float cosT = 1.0f - mm;
  const float sinT = sqrtf(mm * (2.0f - mm));
  const float root = sqrtf(sD);
  const float cPhi = sD == 0.0f ? 1.0f : a / root, sPhi = sD == 0.0f ? 0.0f : b / root;
  const V3 w = toC / sqrtf(d2);
  // Duff et al. 2017, "Building an Orthonormal Basis, Revisited"
  const float sign = copysignf(1.0f, w.z);
  const float ka = -1.0f / (sign + w.z);
  const float kb = (w.x * w.y) * ka;
  const float sx = sign * w.x;
  const V3 t1 = mk(1.0f + (sx * w.x) * ka, sign * kb, -sx);
  const V3 t2 = mk(kb, sign + (w.y * w.y) * ka, -w.y);
  const V3 dir = ((cPhi * sinT) * t1 + (sPhi * sinT) * t2) + cosT * w;
  const float weight = ((float)numLights * (2.0f * oneMinus)) * fmaxf(dot3(m.normal, dir), 0.0f);  // 4
  out.light = k;
  out.dir = dir;
  out.weight = weight;
  Ray shadow;                                                        // 5
  shadow.o = x;
  shadow.d = dir;
  shadow.time = r.time;
  float closest;
  bool found;
  const int hitRef = queryWalk<MODE>(sc, walk, shadow, tMin, tMax, closest, found);
  if (hitRef != ~((idx << 1) | 1)) return out;
  const int material = __float_as_int(s1.w) & SRT_MAT_INDEX_MASK;    // 6
  const uint4 le = sc.shadeRecs[8 * material + 2];                   // a light of the table: {SRT_SLOT_SOLID, r, g, b}
  const V3 att = pbrAttenuation(m, r.d, dir);
  out.radiance = mk(att.x * __uint_as_float(le.y), att.y * __uint_as_float(le.z), att.z * __uint_as_float(le.w)) * weight;
  return out;
}

}  // namespace

#endif
