// srt_query_walk.h -- the walk of one ray of a device buffer through the uploaded trees: what srt_query.hip's kernels
// (srtTraceRaysDevice, srtOccludedDevice) and srt_pathstep.hip's fused step (srtPathStepDevice) both run, stated once.
//   FAITHFUL  world.hit in the reference's order: srt_path.h traverse<false, false> over the 32-byte node records.
//   CLOSEST   the tree-independent closest hit: a per-lane walk over the 64-byte pair records (DevScene::nodes2; one
//             request and two box tests per visit, the child entered nearer first, the other one on a per-lane LDS stack
//             laid out [slot][thread]).  A box is entered unless it is CERTAINLY missed for (tMin, closest): the one-FMA
//             intervals under the certificate's tolerance (boxMaybeHit), or, for a ray outside the certified operand
//             ranges (an axis-parallel direction ...), the reference's divisions under the relative part of the same
//             tolerance (boxHitLoose).  `closest` shrinks with every accepted candidate, so far subtrees are culled when
//             their record is popped.  A candidate with t == closest is kept in reach (neither box test rejects an
//             interval that merely touches) and replaces the current hit only if its prims[] index is larger: the
//             answer is min t, then max index, over all candidates -- no property of the tree.
//   ANY       the same walk with `closest` fixed at the caller's tMax, left at the first accepted candidate.
// Internal; included after srt_path.h by the two kernel files.
#ifndef SRT_QUERY_WALK_H
#define SRT_QUERY_WALK_H

#include "srt_path.h"

// Measurement switch (tools/query_bench.py through an experimental build); the library ships with 0.
#ifndef SRT_QUERY_NODES32
#define SRT_QUERY_NODES32 0  // 1: CLOSEST through srt_path.h traverse<true, false> over the 32-byte records (no tie rule: speed only)
#endif

namespace {

enum { Q_FAITHFUL = 0, Q_CLOSEST = 1, Q_ANY = 2 };

// aabb.h:14-17's quotients, entered unless the interval is empty by more than 2^-21 relative: the box test of a ray
// whose reciprocals are not certified.  boxHit itself rejects an interval that only touches (tMax <= tMin), which would
// cut a candidate with t == closest out of reach; the magnitudes are clamped so that an infinite end (a zero direction
// component) still decides.  A NaN quotient is 0 / 0 -- a zero direction component and the origin IN that plane of the box, so
// the ray lies in the (closed) slab -- or comes from a NaN or infinite operand: the axis then constrains nothing.  (fminf /
// fmaxf alone would keep the other plane's infinite quotient for both ends and cut off every primitive that touches the
// box's upper face: tests/test_gpu_slab_cert.py, rays lying in face planes.)
__device__ __forceinline__ void looseAxis(float a, float b, float& t0, float& t1) {
  const bool open = (a != a) | (b != b);
  t0 = fmaxf(open ? -SRT_INF : fminf(a, b), t0);
  t1 = fminf(open ? SRT_INF : fmaxf(a, b), t1);
}
__device__ __forceinline__ bool boxHitLoose(float4 lo, float4 hi, const Ray& r, float tMin, float tMax, float& tEnter) {
  float t0 = tMin, t1 = tMax;
  looseAxis((lo.x - r.o.x) / r.d.x, (hi.x - r.o.x) / r.d.x, t0, t1);
  looseAxis((lo.y - r.o.y) / r.d.y, (hi.y - r.o.y) / r.d.y, t0, t1);
  looseAxis((lo.z - r.o.z) / r.d.z, (hi.z - r.o.z) / r.d.z, t0, t1);
  const float big = 0x1p100f;
  const float tol = 0x1p-21f * (fminf(fabsf(t1), big) + fminf(fabsf(t0), big));
  tEnter = t0;
  return !(t0 - t1 > tol);  // a NaN end: enter
}

// What a kernel sets up once per lane: the buffer resources of the records the walk reads and the lane's LDS stack,
// [slot][thread] with stackDepth + 2 slots of SRT_BLOCK words (FAITHFUL uses the first stackDepth; otherwise slot 0 holds
// the sentinel that popping the empty stack yields and the last slot is the spare the node step's unconditional store
// may reach).
struct QueryWalk {
  __amdgpu_buffer_rsrc_t rsNodes2, rsTris, rsSpheres;
  int32_t* stack;
  int maxSlot;
};
template <int MODE>
__device__ __forceinline__ QueryWalk queryWalkSetup(const DevScene& sc, int32_t* lds) {
  QueryWalk q;
  q.stack = lds + threadIdx.x;
  q.maxSlot = sc.stackDepth + 1;
  q.rsNodes2 = makeRsrc(sc.nodes2, MODE == Q_FAITHFUL ? 0 : sc.numNodes * 64);
  q.rsTris = makeRsrc(sc.triTest, sc.numTris * 48);
  q.rsSpheres = makeRsrc(sc.spheres, sc.numSpheres * 48);
  if (MODE != Q_FAITHFUL) q.stack[0] = SRT_REF_DONE;  // nothing stores to slot 0 again
  return q;
}

// One ray.  FAITHFUL, CLOSEST: returns the reference of the primitive hit (SRT_REF_DONE: none) and its t in `closest`.
// ANY: returns SRT_REF_DONE and sets `found`.
template <int MODE>
__device__ __forceinline__ int queryWalk(const DevScene& sc, const QueryWalk& q, const Ray& r, float tMin, float tMax,
                                         float& closest, bool& found) {
  int32_t* const stack = q.stack;
  const int maxSlot = q.maxSlot;
  closest = tMax;
  found = false;
  int hitRef = SRT_REF_DONE;
  if (MODE == Q_FAITHFUL) {
    Counters cnt = {0, 0, 0, 0};
    return traverse<false, false>(sc, r, tMin, tMax, stack, closest, cnt);
  }
#if SRT_QUERY_NODES32
  if (MODE == Q_CLOSEST) {
    Counters cnt = {0, 0, 0, 0};
    return traverse<true, false>(sc, r, tMin, tMax, stack, closest, cnt);
  }
#endif
  const float rayA = lenSq(r.d);  // sphere.h:56
  const bool certified = (sc.fastDivScene != 0) & fastDivOperandOk(r.o.x, r.d.x) & fastDivOperandOk(r.o.y, r.d.y) &
                         fastDivOperandOk(r.o.z, r.d.z);
  const V3 rcpD = mk(refinedRcp(r.d.x), refinedRcp(r.d.y), refinedRcp(r.d.z));
  V3 negOR;
  float slabTol;
  slabSetup(r.o, rcpD, certified, negOR, slabTol);
  int hitId = -1;  // prims[] index of hitRef, looked up on the first tie only
  for (int w = 0; w < sc.numWorld && !(MODE == Q_ANY && found); ++w) {
    int cur = sc.world[w];
    if (cur >= 0) cur <<= 1;  // node references of this walk address the 64-byte records
    int sp = 0;               // slot of the top pending reference (0: the sentinel)
    while (cur != SRT_REF_DONE) {
      if (cur >= 0) {
        const float4 l0 = bufLoad4(q.rsNodes2, cur), l1 = bufLoad4(q.rsNodes2, cur + 16), r0 = bufLoad4(q.rsNodes2, cur + 32),
                     r1 = bufLoad4(q.rsNodes2, cur + 48);
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
          const float4 s0 = bufLoad4(q.rsSpheres, off), s1 = bufLoad4(q.rsSpheres, off + 16);
          V3 center = mk(s0.x, s0.y, s0.z);
          if (__float_as_int(s1.w) & (1 << 30)) {  // sphere.h:47-52
            const float4 s2 = bufLoad4(q.rsSpheres, off + 32);
            center = center + ((r.time - s2.x) / (s2.y - s2.x)) * (mk(s1.x, s1.y, s1.z) - center);
          }
          ok = sphereHitV(center, s0.w, r, rayA, tMin, closest, t);
        } else {
          ok = triHitV<true>(bufLoad4(q.rsTris, off), bufLoad4(q.rsTris, off + 16), bufLoad4(q.rsTris, off + 32), r, tMin, closest, t);
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
  return hitRef;
}

}  // namespace

#endif
