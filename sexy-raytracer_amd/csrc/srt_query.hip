// srt_query.hip -- ray queries on device buffers (srtTraceRaysDevice, srtOccludedDevice; include/srt_hip.h "Ray
// queries"): rays that a kernel or a torch op left in device memory, answered in device memory on the caller's stream.
//
// One lane per ray, grid-stride over the ray set (the grid is capped at a few workgroups per CU, like srtTraceRays's).
//   FAITHFUL  world.hit in the reference's order: srt_path.h traverse<false, false> over the 32-byte node records, the
//             record through triRecord / sphereRecord -- what srt_trace_kernel computes, minus its counters.
//   CLOSEST   the tree-independent closest hit: a per-lane walk over the 64-byte pair records (DevScene::nodes2; one
//             request and two box tests per visit, the child entered nearer first, the other one on a per-lane LDS stack
//             laid out [slot][thread]).  A box is entered unless it is CERTAINLY missed for (tMin, closest): the one-FMA
//             intervals under the certificate's tolerance (boxMaybeHit), or, for a ray outside the certified operand
//             ranges (an axis-parallel direction ...), the reference's divisions under the relative part of the same
//             tolerance (boxHitLoose).  `closest` shrinks with every accepted candidate, so far subtrees are culled when
//             their record is popped.  A candidate with t == closest is kept in reach (neither box test rejects an
//             interval that merely touches) and replaces the current hit only if its prims[] index is larger: the
//             answer is min t, then max index, over all candidates -- no property of the tree.
//   ANY       the same walk with `closest` fixed at the caller's tMax, left at the first accepted candidate: one byte.
// No wave scheduler here (the render kernels' step kinds): a query has no shading or restart step to batch, and its
// divergence is the node / primitive alternation of one loop.

#include "srt_path.h"
#include "srt_launch.h"

// Measurement switches (tools/query_bench.py through an experimental build); the library ships with both 0.
#ifndef SRT_QUERY_LDS_RAYS
#define SRT_QUERY_LDS_RAYS 0  // 1: a workgroup's rays loaded as coalesced dwords and transposed through LDS
#endif
#ifndef SRT_QUERY_NODES32
#define SRT_QUERY_NODES32 0  // 1: CLOSEST through srt_path.h traverse<true, false> over the 32-byte records (no tie rule: speed only)
#endif

namespace {

enum { Q_FAITHFUL = 0, Q_CLOSEST = 1, Q_ANY = 2 };

// aabb.h:14-17's quotients, entered unless the interval is empty by more than 2^-21 relative: the box test of a ray
// whose reciprocals are not certified.  boxHit itself rejects an interval that only touches (tMax <= tMin), which would
// cut a candidate with t == closest out of reach; the magnitudes are clamped so that an infinite end (a zero direction
// component) still decides.
__device__ __forceinline__ bool boxHitLoose(float4 lo, float4 hi, const Ray& r, float tMin, float tMax, float& tEnter) {
  float a, b;
  a = (lo.x - r.o.x) / r.d.x;
  b = (hi.x - r.o.x) / r.d.x;
  float t0 = fmaxf(fminf(a, b), tMin), t1 = fminf(fmaxf(a, b), tMax);
  a = (lo.y - r.o.y) / r.d.y;
  b = (hi.y - r.o.y) / r.d.y;
  t0 = fmaxf(fminf(a, b), t0);
  t1 = fminf(fmaxf(a, b), t1);
  a = (lo.z - r.o.z) / r.d.z;
  b = (hi.z - r.o.z) / r.d.z;
  t0 = fmaxf(fminf(a, b), t0);
  t1 = fminf(fmaxf(a, b), t1);
  const float big = 0x1p100f;
  const float tol = 0x1p-21f * (fminf(fabsf(t1), big) + fminf(fabsf(t0), big));
  tEnter = t0;
  return !(t0 - t1 > tol);  // a NaN end: enter
}

template <int MODE>
__global__ __launch_bounds__(SRT_BLOCK) void srt_query_kernel(const QueryArgs a) {
  extern __shared__ int32_t lds[];
  const DevScene& sc = a.scene;
  int32_t* const stack = lds + threadIdx.x;  // [slot][thread]: stackDepth + 2 slots (FAITHFUL uses the first stackDepth)
  const int maxSlot = sc.stackDepth + 1;     // the spare slot the node step's unconditional store may reach
  const __amdgpu_buffer_rsrc_t rsNodes2 = makeRsrc(sc.nodes2, MODE == Q_FAITHFUL ? 0 : sc.numNodes * 64);
  const __amdgpu_buffer_rsrc_t rsTris = makeRsrc(sc.triTest, sc.numTris * 48);
  const __amdgpu_buffer_rsrc_t rsSpheres = makeRsrc(sc.spheres, sc.numSpheres * 48);
  if (MODE != Q_FAITHFUL) stack[0] = SRT_REF_DONE;  // popping the empty stack yields "done"; nothing stores to slot 0 again

  // every lane of a workgroup takes the same number of trips (the staged ray load below has barriers in it)
  for (int64_t base = (int64_t)blockIdx.x * SRT_BLOCK; base < a.n; base += (int64_t)gridDim.x * SRT_BLOCK) {
    const int64_t i = base + threadIdx.x;
#if SRT_QUERY_LDS_RAYS
    // the workgroup's 256 rays are 2 304 contiguous dwords: loaded coalesced, transposed through LDS (a lane's nine words
    // are 9 dwords apart: an odd stride, no bank conflicts)
    float* const staged = reinterpret_cast<float*>(lds + (sc.stackDepth + 2) * SRT_BLOCK);
    const int words = (int)(a.n - base < SRT_BLOCK ? a.n - base : SRT_BLOCK) * 9;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int at = k * SRT_BLOCK + threadIdx.x;
      if (at < words) staged[at] = a.rays[9 * base + at];
    }
    __syncthreads();
    if (i >= a.n) continue;
    const float* in = staged + 9 * threadIdx.x;
#else
    if (i >= a.n) continue;
    const float* in = a.rays + 9 * i;  // nine dword loads 36 bytes apart per lane
#endif
    Ray r;
    r.o = mk(in[0], in[1], in[2]);
    r.d = mk(in[3], in[4], in[5]);
    r.time = in[6];
    const float tMin = in[7], tMax = in[8];
    float closest = tMax;
    int hitRef = SRT_REF_DONE;

    if (MODE == Q_FAITHFUL) {
      Counters cnt = {0, 0, 0, 0};
      hitRef = traverse<false, false>(sc, r, tMin, tMax, stack, closest, cnt);
#if SRT_QUERY_NODES32
    } else if (MODE == Q_CLOSEST) {
      Counters cnt = {0, 0, 0, 0};
      hitRef = traverse<true, false>(sc, r, tMin, tMax, stack, closest, cnt);
#endif
    } else {
      const float rayA = lenSq(r.d);  // sphere.h:56
      const bool certified = (sc.fastDivScene != 0) & fastDivOperandOk(r.o.x, r.d.x) & fastDivOperandOk(r.o.y, r.d.y) &
                             fastDivOperandOk(r.o.z, r.d.z);
      const V3 rcpD = mk(refinedRcp(r.d.x), refinedRcp(r.d.y), refinedRcp(r.d.z));
      V3 negOR;
      float slabTol;
      slabSetup(r.o, rcpD, certified, negOR, slabTol);
      int hitId = -1;  // prims[] index of hitRef, looked up on the first tie only
      bool found = false;
      for (int w = 0; w < sc.numWorld && !(MODE == Q_ANY && found); ++w) {
        int cur = sc.world[w];
        if (cur >= 0) cur <<= 1;  // node references of this walk address the 64-byte records
        int sp = 0;               // slot of the top pending reference (0: the sentinel)
        while (cur != SRT_REF_DONE) {
          if (cur >= 0) {
            const float4 l0 = bufLoad4(rsNodes2, cur), l1 = bufLoad4(rsNodes2, cur + 16), r0 = bufLoad4(rsNodes2, cur + 32),
                         r1 = bufLoad4(rsNodes2, cur + 48);
            const int top = stack[sp * SRT_BLOCK];
            const int left = __float_as_int(l0.w), right = __float_as_int(l1.w);
            float tl, tr;
            bool hl, hr;
            if (slabTol == SRT_INF) {
              hl = boxHitLoose(l0, l1, r, tMin, closest, tl);
              hr = boxHitLoose(r0, r1, r, tMin, closest, tr);
            } else {
              hl = boxMaybeHit(l0, l1, rcpD, negOR, slabTol, tMin, closest, tl);
              hr = boxMaybeHit(r0, r1, rcpD, negOR, slabTol, tMin, closest, tr);
            }
            hr = hr && right != left;  // a one-object leaf names its object twice
            const bool both = hl && hr, leftFirst = !hr || (hl && !(tr < tl));
            const int nearRef = leftFirst ? left : right, farRef = leftFirst ? right : left;
            // the slot above the top is free; it becomes live only if sp is bumped.  Capacity: stackDepth pending
            // references in either visiting order (srt_scene.cpp Builder::build), checked here all the same
            stack[min(sp + 1, maxSlot) * SRT_BLOCK] = farRef;
            sp = (hl || hr) ? (both ? min(sp + 1, maxSlot) : sp) : max(sp - 1, 0);
            cur = (hl || hr) ? nearRef : top;
          } else {
            const int pr = ~cur;
            const int off = (pr >> 1) * 48;
            float t;
            bool ok;
            if (pr & 1) {
              const float4 s0 = bufLoad4(rsSpheres, off), s1 = bufLoad4(rsSpheres, off + 16);
              V3 center = mk(s0.x, s0.y, s0.z);
              if (__float_as_int(s1.w) & (1 << 30)) {  // sphere.h:47-52
                const float4 s2 = bufLoad4(rsSpheres, off + 32);
                center = center + ((r.time - s2.x) / (s2.y - s2.x)) * (mk(s1.x, s1.y, s1.z) - center);
              }
              ok = sphereHitV(center, s0.w, r, rayA, tMin, closest, t);
            } else {
              ok = triHitV<true>(bufLoad4(rsTris, off), bufLoad4(rsTris, off + 16), bufLoad4(rsTris, off + 32), r, tMin, closest, t);
            }
            if (MODE == Q_ANY) {
              if (ok && t <= closest) {  // (a NaN t passes the triangle's comparisons and is no candidate)
                found = true;
                break;
              }
            } else if (ok) {
              bool take = t < closest || hitRef == SRT_REF_DONE;
              if (!take && t == closest) {  // a tie: the larger prims[] index wins
                if (hitId < 0) {
                  const int hp = ~hitRef;
                  hitId = (hp & 1) ? sc.sphPrimId[hp >> 1] : sc.triPrimId[hp >> 1];
                }
                const int id = (pr & 1) ? sc.sphPrimId[pr >> 1] : sc.triPrimId[pr >> 1];
                take = id > hitId;
                if (take) hitId = id;
              } else if (take) {
                take = t <= closest;  // t == tMax is a hit; a NaN is not
                hitId = -1;
              }
              if (take) {
                closest = t;
                hitRef = cur;
              }
            }
            cur = stack[sp * SRT_BLOCK];
            sp = max(sp - 1, 0);
          }
        }
      }
      if (MODE == Q_ANY) {
        a.occluded[i] = found ? 1 : 0;
        continue;
      }
    }

    if (MODE != Q_ANY) {
      int4 h4 = make_int4(SRT_NO_HIT, 0, -1, 0);
      SrtHit h;
      h.prim = SRT_NO_HIT;
      h.t = 0;
      for (int k = 0; k < 3; ++k) h.p[k] = h.normal[k] = h.tangent[k] = h.bitangent[k] = 0;
      h.uv[0] = h.uv[1] = 0;
      h.frontFace = 0;
      h.material = -1;
      h.nodeVisits = h.boxPasses = h.triTests = h.sphereTests = 0;
      if (hitRef != SRT_REF_DONE) {
        Record rec;
        const int pr = ~hitRef;
        const bool all = a.records != nullptr;  // uv and the tangent frame only where the full record is asked for
        if (pr & 1) {
          sphereRecord(sc, pr >> 1, r, closest, rec, all);
          h.prim = sc.sphPrimId[pr >> 1];
        } else {
          triRecord(sc, pr >> 1, r, closest, rec, all);
          h.prim = sc.triPrimId[pr >> 1];
        }
        h.t = rec.t;
        h.p[0] = rec.p.x; h.p[1] = rec.p.y; h.p[2] = rec.p.z;
        h.normal[0] = rec.normal.x; h.normal[1] = rec.normal.y; h.normal[2] = rec.normal.z;
        h.tangent[0] = rec.tangent.x; h.tangent[1] = rec.tangent.y; h.tangent[2] = rec.tangent.z;
        h.bitangent[0] = rec.bitangent.x; h.bitangent[1] = rec.bitangent.y; h.bitangent[2] = rec.bitangent.z;
        h.uv[0] = rec.u; h.uv[1] = rec.v;
        h.frontFace = rec.frontFace ? 1 : 0;
        h.material = rec.material;
        h4 = make_int4(h.prim, __float_as_int(h.t), h.material, h.frontFace);
      }
      if (a.hits) a.hits[i] = h4;  // one dwordx4 store
      if (a.records) a.records[i] = h;
    }
  }
}

}  // namespace

extern "C" {

// mode: SRT_TRAVERSE_FAITHFUL, SRT_TRAVERSE_CLOSEST, or 2 = any hit (a->occluded).  Allocates nothing, waits for nothing.
int srt_launch_query(const QueryArgs* a, int mode, int grid, size_t ldsBytes, hipStream_t stream) {
  void (*kernel)(const QueryArgs) = mode == Q_ANY ? srt_query_kernel<Q_ANY> : mode == Q_CLOSEST ? srt_query_kernel<Q_CLOSEST> : srt_query_kernel<Q_FAITHFUL>;
  if (SRT_QUERY_LDS_RAYS) ldsBytes += 9 * SRT_BLOCK * sizeof(float);
  if (ldsBytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SRT_BLOCK), ldsBytes, stream, *a);
  return (int)hipGetLastError();
}

}  // extern "C"
