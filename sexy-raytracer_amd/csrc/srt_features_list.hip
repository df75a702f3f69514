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
// threadedTraverse and surfaceFeatures are srt_features_body.h's, the one copy both kernels inline.  The LDS fill and the
// sample loop are stated here as in srt_features.hip: change one, change the other.
#include "srt_features_body.h"
#include "srt_launch.h"

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

// [accumulate][featureForm]
static void (*const featuresListKernels[2][3])(const FeatureListArgs) = {
    {srt_features_list_kernel<true, false, false>, srt_features_list_kernel<false, true, false>,
     srt_features_list_kernel<false, false, false>},
    {srt_features_list_kernel<true, false, true>, srt_features_list_kernel<false, true, true>,
     srt_features_list_kernel<false, false, true>}};

extern "C" {
// srt_passes.cpp srtRenderFeatureTileList, as srt_features_plan
int srt_features_list_plan(int closest, int ldsTree, int accumulate, size_t lds, int* block, int* perCU) {
  const void* k = reinterpret_cast<const void*>(featuresListKernels[accumulate != 0][featureForm(closest, ldsTree)]);
  return featurePlan(k, ldsTree, lds, block, perCU);
}

int srt_launch_features_list(const FeatureListArgs* a, int closest, int ldsTree, int accumulate, int grid, size_t lds,
                             hipStream_t stream) {
  return featureLaunch(featuresListKernels[accumulate != 0][featureForm(closest, ldsTree)], ldsTree, a, grid, lds, stream);
}
}  // extern "C"
