// srt_features_list.hip -- the feature pass over a tile list (include/srt_hip.h srtRenderFeatureTileList): the guide planes
// of the tiles an adaptive round rendered, over that round's sample range, added into image-order planes.
//
// srt_features_kernel's shape (srt_features.hip): one lane per pixel, one wave per 8x8 tile, waves take list positions from
// one atomic counter, the same three traversal forms and the same per-sample body -- the camera ray of the key (seed, pixel,
// s), the traversal, the render kernels' hit record, surfaceFeatures -- so a lane's running sum over [sampleFirst,
// sampleFirst + spp) is that kernel's, bit for bit.  Two differences:
//   tile source  list[i] = tx | ty << 16 (RenderArgs::tileXY, the adaptive lists); an entry outside the tile grid is skipped
//                whole.  A tile listed twice is a caller error: its two waves would race
//   output       straight into image-order float4[W*H] planes.  ACCUM: the pixel's record is read, the lane's sum added once
//                per channel (w included) and written back; else stored.  A pixel belongs to one tile: no atomics.  Padding
//                lanes of edge tiles neither read nor write
// threadedTraverse and surfaceFeatures are restated from srt_features.hip rather than shared (as srt_temporal_adaptive.hip
// restates the reprojection): that file's code objects stay what they were.
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

}  // namespace

template <bool CLOSEST, bool LDSTREE, bool ACCUM>
__global__ __launch_bounds__(LDSTREE ? SRT_BLOCK_TREE : SRT_BLOCK) void srt_features_list_kernel(const FeatureListArgs args) {
  static_assert(!(CLOSEST && LDSTREE), "the LDS-resident tree serves the FAITHFUL traversal");
  extern __shared__ int32_t lds[];
  const FeatureArgs& a = args.f;
  const DevScene& sc = a.scene;
  const int lane = threadIdx.x & 63;
  char* const ldsTree = reinterpret_cast<char*>(lds);
  // LDS: the node records (LDSTREE) or the lanes' traversal stacks, [slot][thread]
  if (LDSTREE) {
    // node records into LDS, node children as indices, the second link replaced by the thread links (srt_features_kernel)
    const Rsrc rsNodes = makeRsrc(sc.nodes, sc.numNodes * 32);
    float4* dst = reinterpret_cast<float4*>(ldsTree);
    for (int i = threadIdx.x; i < sc.numNodes * 2; i += blockDim.x) {
      float4 v = bufLoad4(rsNodes, 16 * i);
      const int r = __float_as_int(v.w);
      if (i & 1)
        v.w = __int_as_float(sc.nodeThread[i >> 1]);
      else if (r >= 0)
        v.w = __int_as_float(SRT_NODE_INDEX(r));
      dst[i] = v;
    }
    __syncthreads();
  }
  const Rsrc rsTexels = makeRsrc(sc.texels, sc.texelBytes);
  const uint64_t seedMixed = mix64(a.seed);
  const V3 background = ld3(a.background);
  const DevCamera& cam = a.cam;
  for (;;) {
    int taken = 0;
    if (lane == 0) taken = atomicAdd(a.counter, 1);
    const int at = __shfl(taken, 0);
    if (at >= args.numListed) break;
    const uint32_t txy = args.list[at];
    const int tx = (int)(txy & 0xffffu), ty = (int)(txy >> 16);
    if (tx >= a.tilesX || ty >= a.tilesY) continue;  // not a tile of this image (the whole wave: nothing read or written)
    const int px = tx * SRT_TILE_W + (lane & (SRT_TILE_W - 1)), py = ty * SRT_TILE_H + (lane >> 3);
    const bool valid = px < a.imageWidth && py < a.imageHeight;
    const uint32_t pixel = (uint32_t)(py * a.imageWidth + px);
    V3 sAlb = mk(0.0f, 0.0f, 0.0f), sNrm = sAlb, sPos = sAlb, sDep = sAlb;
    int nAlb = 0, nHit = 0;
    const int sEnd = valid ? a.sampleFirst + a.spp : a.sampleFirst;
    for (int s = a.sampleFirst; s < sEnd; ++s) {
      // the beauty render's camera ray of sample s (srt_kernels.hip restart step, main.cpp:204-216)
      Pcg rng;
      rng.key(seedMixed, pixel, (uint32_t)s);
      const float u = ((float)px + rng.uniform()) / (float)(a.imageWidth - 1);                      // main.cpp:210
      const float v = ((float)(a.imageHeight - py) + rng.uniform()) / (float)(a.imageHeight - 1);  // main.cpp:211
      Ray ray;
      cameraRay(cam, u, v, rng, ray);
      float tHit;
      int ref;
      if (LDSTREE) {
        ref = threadedTraverse(sc, ldsTree, ray, a.tMin, tHit);
      } else {
        Counters cnt = {0, 0, 0, 0};
        ref = traverse<CLOSEST, false>(sc, ray, a.tMin, SRT_INF, lds + threadIdx.x, tHit, cnt);
      }
      nAlb++;
      if (ref == SRT_REF_DONE) {  // main.cpp:39-40
        sAlb = sAlb + background;
        continue;
      }
      Record rec;
      const int pr = ~ref;
      if (pr & 1)
        sphereRecord(sc, pr >> 1, ray, tHit, rec, false);
      else
        triRecord(sc, pr >> 1, ray, tHit, rec, false);
      nHit++;
      if (a.planes & (SRT_FEATURE_ALBEDO | SRT_FEATURE_NORMAL)) {
        V3 alb, nrm;
        surfaceFeatures(sc, rsTexels, rec, alb, nrm);
        sAlb = sAlb + alb;
        sNrm = sNrm + nrm;
      }
      sPos = sPos + rec.p;
      sDep = sDep + mk(rec.t, rec.t * rec.t, 0.0f);
    }
    if (!valid) continue;  // padding lanes of an edge tile
    const float4 sums[4] = {make_float4(sAlb.x, sAlb.y, sAlb.z, (float)nAlb), make_float4(sNrm.x, sNrm.y, sNrm.z, (float)nHit),
                            make_float4(sPos.x, sPos.y, sPos.z, (float)nHit), make_float4(sDep.x, sDep.y, sDep.z, (float)nHit)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(a.planes >> k & 1)) continue;
      float4 v = sums[k];
      if (ACCUM) {
        const float4 o = a.out[k][pixel];
        v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
      }
      a.out[k][pixel] = v;
    }
  }
}

static const void* featuresListKernel(int closest, int ldsTree, int accumulate) {
#define SRT_FL_PICK(ACCUM)                                                                            \
  (closest   ? reinterpret_cast<const void*>(srt_features_list_kernel<true, false, ACCUM>)            \
   : ldsTree ? reinterpret_cast<const void*>(srt_features_list_kernel<false, true, ACCUM>)            \
             : reinterpret_cast<const void*>(srt_features_list_kernel<false, false, ACCUM>))
  return accumulate ? SRT_FL_PICK(true) : SRT_FL_PICK(false);
#undef SRT_FL_PICK
}

extern "C" {
// srt_api.cpp srtRenderFeatureTileList, as srt_features_plan: ldsTree = the FAITHFUL walk of the LDS-resident threaded
// tree; block = its threads per workgroup (SRT_BLOCK_TREE, else SRT_BLOCK); perCU = resident workgroups per CU for that
// LDS size (occupancy query)
int srt_features_list_plan(int closest, int ldsTree, int accumulate, size_t lds, int* block, int* perCU) {
  const void* k = featuresListKernel(closest, ldsTree, accumulate);
  *block = ldsTree ? SRT_BLOCK_TREE : SRT_BLOCK;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(perCU, k, *block, lds) != hipSuccess || *perCU < 1) *perCU = 1;
  return 0;
}

int srt_launch_features_list(const FeatureListArgs* a, int closest, int ldsTree, int accumulate, int grid, size_t lds,
                             hipStream_t stream) {
#define SRT_FL_LAUNCH(ACCUM)                                                                                                    \
  do {                                                                                                                          \
    if (closest)                                                                                                                \
      hipLaunchKernelGGL((srt_features_list_kernel<true, false, ACCUM>), dim3(grid), dim3(SRT_BLOCK), lds, stream, *a);         \
    else if (ldsTree)                                                                                                           \
      hipLaunchKernelGGL((srt_features_list_kernel<false, true, ACCUM>), dim3(grid), dim3(SRT_BLOCK_TREE), lds, stream, *a);    \
    else                                                                                                                        \
      hipLaunchKernelGGL((srt_features_list_kernel<false, false, ACCUM>), dim3(grid), dim3(SRT_BLOCK), lds, stream, *a);        \
  } while (0)
  if (accumulate)
    SRT_FL_LAUNCH(true);
  else
    SRT_FL_LAUNCH(false);
#undef SRT_FL_LAUNCH
  return (int)hipGetLastError();
}
}  // extern "C"
