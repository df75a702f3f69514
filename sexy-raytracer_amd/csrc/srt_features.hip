// srt_features.hip -- the feature pass (include/srt_hip.h srtRenderFeatureTiles): albedo, shading normal, position and
// depth at the first hit of exactly the camera rays the beauty render traces, the guide images of a denoiser.
//
// One lane per pixel, one wave per 8x8 tile: a wave's 64 primary rays leave one lens through one small patch of the image
// and stay coherent through the tree.  A lane runs its pixel's samples in index order: the camera ray of srt_kernels.hip's
// restart step (same RNG key, same draws), the traversal the parameters ask for, the render kernels' hit record, then the
// material's albedo and normal from the same 128-byte material record and texture lookups shade() reads (threadedTraverse
// and surfaceFeatures: srt_features_body.h, shared with srt_features_list.hip).  Waves take tiles from one atomic counter
// (local tile order), so the tail of the frame stays balanced.
//
// Traversal, by the scene's tree and the requested semantics:
//   LDSTREE  FAITHFUL with the whole node array in a CU's LDS (DevScene::nodeThread set): the stackless walk of the
//            threaded copy, as srt_render_kernel LDSTREE does it -- one 1024-thread workgroup per CU fills the LDS copy
//   else     traverse<CLOSEST, false> (srt_path.h) over scene.nodes with the pending right children on a per-lane LDS
//            stack: FAITHFUL trees too large for LDS or without thread links, and SRT_TRAVERSE_CLOSEST (device-built
//            trees included) -- 256-thread workgroups (the stack's [slot][thread] stride is SRT_BLOCK)
// Nothing of the render kernels is shared beyond srt_path.h's device functions: their code objects do not change.
#include "srt_features_body.h"
#include "srt_launch.h"

template <bool CLOSEST, bool LDSTREE>
__global__ __launch_bounds__(LDSTREE ? SRT_BLOCK_TREE : SRT_BLOCK) void srt_features_kernel(const FeatureArgs a) {
  static_assert(!(CLOSEST && LDSTREE), "the LDS-resident tree serves the FAITHFUL traversal");
  extern __shared__ int32_t lds[];
  const DevScene& sc = a.scene;
  const int lane = threadIdx.x & 63;
  char* const ldsTree = reinterpret_cast<char*>(lds);
  // LDS: the node records (LDSTREE) or the lanes' traversal stacks, [slot][thread]
  if (LDSTREE) {
    // node records into LDS, node children as indices, the second link replaced by the thread links (srt_render_kernel)
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
    const int localTile = __shfl(taken, 0);
    if (localTile >= a.numLocalTiles) break;
    const int tile = a.tileFirst + localTile * a.tileStride;
    int tx = 0, ty = 0;
    if (tile < a.numTiles) srtTileFromOrder(tile, a.tilesX, a.tilesY, a.tileBlock, tx, ty);
    const int px = tx * SRT_TILE_W + (lane & (SRT_TILE_W - 1)), py = ty * SRT_TILE_H + (lane >> 3);
    const bool valid = tile < a.numTiles && px < a.imageWidth && py < a.imageHeight;
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
    const int o = localTile * SRT_TILE_PIXELS + lane;
    if (a.planes & SRT_FEATURE_ALBEDO) a.out[0][o] = make_float4(sAlb.x, sAlb.y, sAlb.z, (float)nAlb);
    if (a.planes & SRT_FEATURE_NORMAL) a.out[1][o] = make_float4(sNrm.x, sNrm.y, sNrm.z, (float)nHit);
    if (a.planes & SRT_FEATURE_POSITION) a.out[2][o] = make_float4(sPos.x, sPos.y, sPos.z, (float)nHit);
    if (a.planes & SRT_FEATURE_DEPTH) a.out[3][o] = make_float4(sDep.x, sDep.y, sDep.z, (float)nHit);
  }
}

static void (*const featuresKernels[3])(const FeatureArgs) = {srt_features_kernel<true, false>, srt_features_kernel<false, true>,
                                                              srt_features_kernel<false, false>};

extern "C" {
// srt_passes.cpp srtRenderFeatureTiles: ldsTree = the FAITHFUL walk of the LDS-resident threaded tree
int srt_features_plan(int closest, int ldsTree, size_t lds, int* block, int* perCU) {
  return featurePlan(reinterpret_cast<const void*>(featuresKernels[featureForm(closest, ldsTree)]), ldsTree, lds, block, perCU);
}

int srt_launch_features(const FeatureArgs* a, int closest, int ldsTree, int grid, size_t lds, hipStream_t stream) {
  return featureLaunch(featuresKernels[featureForm(closest, ldsTree)], ldsTree, a, grid, lds, stream);
}
}  // extern "C"
