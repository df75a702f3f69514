// srt_features_body.h -- what the two feature kernels share (srt_features.hip, srt_features_list.hip), one copy each: the
// walk of the LDS-resident threaded tree, the material's albedo and normal, and the host helpers that plan and launch one of
// a kernel's three traversal forms.  The kernels' LDS node fill and per-sample loop are still stated in both files: sharing
// either as an inlined function changed the register allocation of the compiled kernels.
#pragma once
#include "srt_path.h"

namespace {

// The FAITHFUL walk of the threaded tree in LDS (srt_render_kernel LDSTREE, bvh.h:97-105): a node's first link is its left
// child (node INDEX or primitive reference), its second packs two 16-bit references -- high half: where the walk goes when
// the subtree is done, low half: what follows a leaf's first object.  Box hit: the left child; miss: the high half.
__device__ __forceinline__ int threadedTraverse(const DevScene& sc, const char* ldsTree, const Ray& r, float tMin, float& tHit) {
  constexpr int32_t DONE = (int32_t)0xFFFF8000;  // the 16-bit "done", sign-extended
  constexpr int32_t DONE_PAIR = (int32_t)0x80008000;
  const float a = lenSq(r.d);  // sphere.h:56
  const bool certified = (sc.fastDivScene != 0) & fastDivOperandOk(r.o.x, r.d.x) & fastDivOperandOk(r.o.y, r.d.y) &
                         fastDivOperandOk(r.o.z, r.d.z);
  const V3 rcpD = mk(refinedRcp(r.d.x), refinedRcp(r.d.y), refinedRcp(r.d.z));
  V3 negOR;
  float slabTol;
  slabSetup(r.o, rcpD, certified, negOR, slabTol);
  float closest = SRT_INF;
  int hitRef = SRT_REF_DONE;
  for (int w = 0; w < sc.numWorld; ++w) {
    const int root = sc.world[w];
    int cur = root >= 0 ? SRT_NODE_INDEX(root) : root;
    int32_t link = DONE_PAIR;
    while (cur != DONE) {
      if (cur >= 0) {
        const float4 n0 = *reinterpret_cast<const float4*>(ldsTree + (cur << 5));
        const float4 n1 = *reinterpret_cast<const float4*>(ldsTree + (cur << 5) + 16);
        bool undecided;
        bool hitBox = boxHitApprox<false>(n0, n1, rcpD, negOR, slabTol, tMin, closest, undecided);
        if (undecided) hitBox = boxHit(n0, n1, r, tMin, closest);
        link = __float_as_int(n1.w);
        cur = hitBox ? __float_as_int(n0.w) : (link >> 16);
      } else {
        const int pr = ~cur;
        float t;
        const bool ok = (pr & 1) ? sphereHit(sc.spheres + 3 * (pr >> 1), r, a, tMin, closest, t)
                                 : triHit<false>(sc.triTest + 3 * (pr >> 1), r, tMin, closest, t);
        if (ok) {
          closest = t;
          hitRef = cur;
        }
        cur = (int32_t)(int16_t)link;  // what follows this object; the high half after that
        link >>= 16;
      }
    }
  }
  tHit = closest;
  return hitRef;
}

// The albedo and the normal the material's scatter works with (shade(), material.h:91-245), from the same material
// record and texture lookups.
__device__ __forceinline__ void surfaceFeatures(const DevScene& sc, Rsrc rsTexels, const Record& rec, V3& albedoOut, V3& normalOut) {
  const Rsrc rsMat = makeRsrc(sc.shadeRecs, sc.numMaterials * 128);
  const int at = rec.material * 128;
  uint32_t fetches = 0;
  normalOut = rec.normal;
  switch (rec.matType & 3) {
    case SRT_MAT_LIGHT: {  // the emitted colour, material.h:144-150, clamped to [0, 1]
      const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rsMat, at + 32, 0, 0);
      V3 e;
      if (t.x == SRT_SLOT_IMAGE) {
        const uint32_t px = __builtin_amdgcn_raw_buffer_load_b32(rsTexels, texelOffset((int)t.y, (int)t.z, (int)t.w, rec.u, rec.v), 0, 0);
        e = mk((float)(px & 0xffu), (float)((px >> 8) & 0xffu), (float)((px >> 16) & 0xffu));
      } else if (t.x == SRT_SLOT_SOLID) {
        e = mk(__uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w));
      } else {
        e = texValue<false>(sc, rsTexels, (int)t.y, rec.u, rec.v, rec.p, fetches);
      }
      albedoOut = mk(clampf(e.x, 0.0f, 1.0f), clampf(e.y, 0.0f, 1.0f), clampf(e.z, 0.0f, 1.0f));
      return;
    }
    case SRT_MAT_METAL: {
      const float4 albedo = bufLoad4(rsMat, at + 16);
      albedoOut = mk(albedo.x, albedo.y, albedo.z);
      return;
    }
    case SRT_MAT_DIELECTRIC:
      albedoOut = mk(1.0f, 1.0f, 1.0f);
      return;
    default: {  // pbrMetallicRoughness: base (the albedo map / 255, else the factor) times the factor, as fd is formed
      const float4 albedo = bufLoad4(rsMat, at + 16);
      V3 a0 = mk(albedo.x, albedo.y, albedo.z);
      if (rec.matType & SRT_MAT_TEXTURED) {
        const u32x4 tAN = __builtin_amdgcn_raw_buffer_load_b128(rsMat, at + 48, 0, 0);
        auto fetch = [&](uint32_t mw, uint32_t aux) {
          return (mw & 3u) != SRT_SLOT_IMAGE ? 0u : __builtin_amdgcn_raw_buffer_load_b32(rsTexels, slotTexelOffset(mw, aux, rec.u, rec.v), 0, 0);
        };
        if ((tAN.x & 7u) == SRT_SLOT_CHECKER2) {
          const float4 c = checkerOdd(rec.p) ? bufLoad4(rsMat, at + 96) : bufLoad4(rsMat, at + 80);
          a0 = mk(c.x * 255.0f, c.y * 255.0f, c.z * 255.0f) / 255.0f;
        } else if ((tAN.x & 3u) != SRT_SLOT_NONE) {
          a0 = slotValue<false>(sc, rsTexels, tAN.x, tAN.y, fetch(tAN.x, tAN.y), rec.u, rec.v, rec.p, fetches) / 255.0f;
        }
        if ((tAN.z & 3u) != SRT_SLOT_NONE) {
          V3 nt = slotValue<false>(sc, rsTexels, tAN.z, tAN.w, fetch(tAN.z, tAN.w), rec.u, rec.v, rec.p, fetches);
          nt = mk(nt.x - 128.0f, nt.y - 128.0f, nt.z - 128.0f) / 128.0f;  // vec3.h:103-110
          V3 w = mk(rec.tangent.x * nt.x + (rec.bitangent.x * nt.y + rec.normal.x * nt.z),
                    rec.tangent.y * nt.x + (rec.bitangent.y * nt.y + rec.normal.y * nt.z),
                    rec.tangent.z * nt.x + (rec.bitangent.z * nt.y + rec.normal.z * nt.z));
          normalOut = unitv(w);
        }
      }
      albedoOut = mk(a0.x * albedo.x, a0.y * albedo.y, a0.z * albedo.z);
      return;
    }
  }
}

// Host side.  A feature kernel has three traversal forms, in this order in its table: CLOSEST, the FAITHFUL walk of the
// LDS-resident threaded tree, FAITHFUL with stacks.
inline int featureForm(int closest, int ldsTree) { return closest ? 0 : ldsTree ? 1 : 2; }

// block = the form's threads per workgroup (SRT_BLOCK_TREE, else SRT_BLOCK); perCU = resident workgroups per CU for that
// LDS size (occupancy query)
inline int featurePlan(const void* k, int ldsTree, size_t lds, int* block, int* perCU) {
  *block = ldsTree ? SRT_BLOCK_TREE : SRT_BLOCK;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(perCU, k, *block, lds) != hipSuccess || *perCU < 1) *perCU = 1;
  return 0;
}

template <typename Args>
inline int featureLaunch(void (*k)(const Args), int ldsTree, const Args* a, int grid, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL(k, dim3(grid), dim3(ldsTree ? SRT_BLOCK_TREE : SRT_BLOCK), lds, stream, *a);
  return (int)hipGetLastError();
}

}  // namespace
