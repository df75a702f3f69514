// srt_motion.hip -- the motion pass (include/srt_hip.h "Motion", srtRenderMotionTiles): per pixel, the displacement that
// takes the first hit of exactly the camera rays the beauty render traces back to where that surface point was at the
// previous srtRefitScene, summed over the samples that hit.  The plane srtTemporalAccumulateMotion reprojects with.
//
// The feature pass's structure (srt_features.hip): one lane per pixel, one wave per 8x8 tile, tiles from the feature
// passes' atomic counter, a lane's samples in index order, and its three traversal forms -- CLOSEST, the FAITHFUL walk of
// the LDS-resident threaded tree (srt_features_body.h threadedTraverse), FAITHFUL with stacks.  A hit reads no material:
// it loads the primitive's current record and its record in the snapshot (three more 16-byte loads) and evaluates the
// header's displacement, about 60 flops, in the header's operation order with srt_path.h's dot3 and cross3 (no
// contraction, IEEE division), so tests/motion_ref.py reproduces every bit in NumPy float32.
//
// In its own file: the code objects of srt_features.hip and srt_features_list.hip do not change.  The LDS node fill and
// the per-sample loop are stated here a third time for the reason srt_features_body.h gives.
#include "srt_features_body.h"
#include "srt_launch.h"

namespace {

// A triangle's displacement at p: the barycentric mix of the three vertex displacements, the weights from triHitV's three
// edge values (e0 weighs v2, e1 v0, e2 v1).  A degenerate current triangle (!(s > 0)) moves as its first vertex.
__device__ __forceinline__ V3 triMotion(const float4* cur, const float4* prev, V3 p) {
  const float4 q0 = cur[0], q1 = cur[1], q2 = cur[2];
  const float4 r0 = prev[0], r1 = prev[1], r2 = prev[2];
  const V3 v0 = mk(q0.x, q0.y, q0.z), v1 = mk(q1.x, q1.y, q1.z), v2 = mk(q2.x, q2.y, q2.z);
  const V3 n = mk(q0.w, q1.w, q2.w);
  const V3 d0 = mk(r0.x, r0.y, r0.z) - v0, d1 = mk(r1.x, r1.y, r1.z) - v1, d2 = mk(r2.x, r2.y, r2.z) - v2;
  const float e0 = dot3(n, cross3(v1 - v0, p - v0));
  const float e1 = dot3(n, cross3(v2 - v1, p - v1));
  const float e2 = dot3(n, cross3(v0 - v2, p - v2));
  const float s = (e0 + e1) + e2;
  const float b0 = e1 / s, b1 = e2 / s, b2 = e0 / s;
  const V3 m = (b0 * d0 + b1 * d1) + b2 * d2;
  return s > 0.0f ? m : d0;
}

// A sphere's displacement at p: its centre's (both at the ray's time) plus the radial part of a radius change
__device__ __forceinline__ V3 sphereMotion(const float4* cur, const float4* prev, V3 p, float time) {
  const float4 s0 = cur[0], s1 = cur[1];
  const float4 t0 = prev[0], t1 = prev[1];
  const V3 c = sphereCenter(cur, s0, s1, time);
  const V3 cp = sphereCenter(prev, t0, t1, time);
  return (cp - c) + ((t0.w / s0.w) - 1.0f) * (p - c);
}

}  // namespace

template <bool CLOSEST, bool LDSTREE>
__global__ __launch_bounds__(LDSTREE ? SRT_BLOCK_TREE : SRT_BLOCK) void srt_motion_kernel(const MotionArgs m) {
  static_assert(!(CLOSEST && LDSTREE), "the LDS-resident tree serves the FAITHFUL traversal");
  extern __shared__ int32_t lds[];
  const FeatureArgs& a = m.f;
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
  const uint64_t seedMixed = mix64(a.seed);
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
    V3 sMot = mk(0.0f, 0.0f, 0.0f);
    int nHit = 0;
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
      if (ref == SRT_REF_DONE) continue;  // a miss does not count
      const int pr = ~ref;
      const V3 p = ray.o + tHit * ray.d;  // ray.h:15-17, the hit record's p
      const V3 d = (pr & 1) ? sphereMotion(sc.spheres + 3 * (pr >> 1), m.prevSpheres + 3 * (pr >> 1), p, ray.time)
                            : triMotion(sc.triTest + 3 * (pr >> 1), m.prevTriTest + 3 * (pr >> 1), p);
      nHit++;
      sMot = sMot + d;
    }
    a.out[0][localTile * SRT_TILE_PIXELS + lane] = make_float4(sMot.x, sMot.y, sMot.z, (float)nHit);
  }
}

static void (*const motionKernels[3])(const MotionArgs) = {srt_motion_kernel<true, false>, srt_motion_kernel<false, true>,
                                                           srt_motion_kernel<false, false>};

extern "C" {
// srt_passes.cpp srtRenderMotionTiles: ldsTree = the FAITHFUL walk of the LDS-resident threaded tree
int srt_motion_plan(int closest, int ldsTree, size_t lds, int* block, int* perCU) {
  return featurePlan(reinterpret_cast<const void*>(motionKernels[featureForm(closest, ldsTree)]), ldsTree, lds, block, perCU);
}

int srt_launch_motion(const MotionArgs* a, int closest, int ldsTree, int grid, size_t lds, hipStream_t stream) {
  return featureLaunch(motionKernels[featureForm(closest, ldsTree)], ldsTree, a, grid, lds, stream);
}
}  // extern "C"
