// srt_wavefront.hip -- the per-pixel path-tracing loop (main.cpp:200-227, rayColor main.cpp:33-52) with the paths
// kept in a POOL per workgroup instead of one per lane: lanes traverse, full waves shade.
//
// srt_kernels.hip's LDS-resident-tree kernel binds a path to a lane for its whole life, so every wave holds lanes at
// nodes, at primitives, waiting for a hit to be shaded and waiting for a restart, and each step kind runs at 29-39 of
// 64 lanes (profiles/r02/step_profile_lds_tree.txt); worse, a hit step serves whatever materials its ~38 lanes
// happen to have hit, so it executes the triangle record AND the sphere record, image lookups AND the checker, pbr AND
// metal AND light code on every execution.  Here, with one 1024-thread workgroup owning the CU and its LDS:
//
//   * a PATH CONTEXT (one work item in flight: pixel x sample chunk, its current ray, RNG, attenuations, partial
//     sum: one 128-byte line in global memory) belongs to no lane.  Each workgroup owns `poolSize` of them
//     (about 1.5 per lane).
//   * lanes are TRAVERSAL ENGINES: a lane holds only a ray and its walk of the threaded tree (DevScene::nodeThread,
//     bvh.h:97-105 in bvh.h's order).  When the walk ends it leaves (t, primitive) in the context's LDS slot, hands the
//     context to a queue and takes the next READY context (swap step: LDS traffic only, plus the new ray's one line).
//   * queues are rings of context ids in LDS: READY (a fresh ray to traverse), RESTART (path ended or ray missed:
//     main.cpp:39-40,49-51,217 and the next camera ray, main.cpp:204-216), NEWITEM (the item's last sample is in:
//     write its sum, pull the next work item with ONE atomic for the 64, main.cpp:200-203) and one HIT ring per
//     MATERIAL CLASS (triangle + pbr / sphere + pbr / everything else).  Any wave that finds 64 entries in a ring takes
//     them and runs that step for them: hit shading (main.cpp:42-51 + material.h), restarts and item pulls run at 64 of
//     64 lanes, and a hit step executes one class's code.  A wave with nothing to traverse serves partial batches,
//     which also drains the end of the frame.
//
// Same arithmetic as srt_kernels.hip (srt_path.h holds it), same samples in the same order per work item, the same
// exact chunk sums: accumulators are bit-identical to the step-scheduler kernels' (tests: node_path "wavefront").
// Termination: every spin on a ring slot is bounded; a wave that exceeds the bound raises the workgroup's abort word,
// every wave leaves at its next scheduling decision and the host reports the error (RenderArgs::wfError).  The
// grid drains when every context has found the work queues empty (live == 0).
#include "srt_path.h"
#include "srt_launch.h"
#include "srt_wf_links.h"
#include "srt_wf_rings.h"  // the rings, their control words, enqueue and claim
#include "srt_lds_layout.h"  // WF_CTL_WORDS; srtWfLdsLayout states the carve-up below for the host

#define WF_BLOCK 1024
#define WF_SET_OF(mask) std::integral_constant<uint32_t, (mask)>()  // the rings an enqueue site can produce
#define WF_CTX_BYTES 128
// Context line (global memory, one per context id):  +0 A = ray origin, time   +16 B = ray direction (terminal radiance
// once the path has ended), -   +32 C = RNG state (2 words), -, depth | pend << 8   +48 D = partial pixel sum, sample
// count of the item   +64 E = output index, next sample, end sample, px | py << 16   +80 attenuations of bounces 0..3.
// The moments instances keep the item's running sum of l_s in B.w and of l_s^2 in C.z (0 in the others): every store of
// B and C carries them, so they cost no traffic of their own.
// Control words (LDS, behind the tree): 0..15 the waves' current work queue; 16 + 2r ring r's tail (places reserved),
// 17 + 2r its head (places claimed) -- one 8-byte read gets both --, 28 live contexts, 29 abort; 32..55 the sphere records
// of the walks' head leaf (DevScene::wfHead != 0; the whole-tree instances that neither count nor are hybrid): the first
// object's three 16-byte quads of DevScene::spheres, then the second object's (zeros where the leaf holds one sphere),
// copied by the set-up of every launch and read-only afterwards.  The other words stay zero.  Behind them the rings
// (16-bit slots), then per context the t (float) and the primitive (16 bits) its last walk ended at.
#define WF_CTL_LIVE 28
#define WF_CTL_ABORT 29
#define WF_CTL_LEAFREC 32       // first word of the head leaf's two sphere records
#define WF_CTL_LEAFREC_WORDS 24  // 2 records x 48 bytes
static_assert(WF_CTL_LEAFREC > WF_CTL_ABORT && WF_CTL_LEAFREC > WF_CTL_LIVE && WF_CTL_LEAFREC > WF_CTL_HEAD(WF_RINGS - 1),
              "the head leaf's records lie behind the ring words, the live count and the abort word");
static_assert(WF_CTL_LEAFREC + WF_CTL_LEAFREC_WORDS <= WF_CTL_WORDS, "the head leaf's records lie inside the control block");
static_assert(WF_CTL_LEAFREC % 4 == 0, "the head leaf's records are read 16 bytes at a time (the block starts at a multiple of 32)");
#define WF_PEND_MISS 0      // context meta word: depth | pend << 8
#define WF_PEND_TERMINAL 2

namespace {
enum { W_NODE = 0, W_PRIM = 1, W_SWAP = 2, W_SERVE = 3 };

__device__ __forceinline__ void bufStore4(Rsrc r, int off, float4 v) {
  u32x4 u;
  u.x = __float_as_uint(v.x); u.y = __float_as_uint(v.y); u.z = __float_as_uint(v.z); u.w = __float_as_uint(v.w);
  __builtin_amdgcn_raw_buffer_store_b128(u, r, off, 0, 0);
}
__device__ __forceinline__ void bufStore1(Rsrc r, int off, uint32_t v) { __builtin_amdgcn_raw_buffer_store_b32(v, r, off, 0, 0); }
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const f32x4 LdsVec4;  // a 16-byte slot addressed by its LDS byte offset
__device__ __forceinline__ uint32_t bufLoad1(Rsrc r, int off) { return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0); }

// sphere::hit on a record's loaded quads s0 and s1; `quad2()` hands out the third, asked for where the sphere moves: the one
// statement for the primitive step and for the head of a walk (swapStep), which differ in where the quads come from
template <class Quad2>
__device__ __forceinline__ bool wfSphereHitOn(const float4 s0, const float4 s1, Quad2 quad2, const Ray& ray, float rayA, float tMin,
                                              float closest, float& t) {
  V3 center = mk(s0.x, s0.y, s0.z);
  if (__float_as_int(s1.w) & (1 << 30)) {  // sphere.h:47-52
    const float4 s2 = quad2();
    center = center + ((ray.time - s2.x) / (s2.y - s2.x)) * (mk(s1.x, s1.y, s1.z) - center);
  }
  return sphereHitV(center, s0.w, ray, rayA, tMin, closest, t);
}
// ... on the record at byte offset `off` of DevScene::spheres, through its buffer resource (the primitive step)
__device__ __forceinline__ bool wfSphereHit(Rsrc rsSpheres, int off, const Ray& ray, float rayA, float tMin, float closest, float& t) {
  const float4 s0 = bufLoad4(rsSpheres, off), s1 = bufLoad4(rsSpheres, off + 16);
  return wfSphereHitOn(s0, s1, [&]() { return bufLoad4(rsSpheres, off + 32); }, ray, rayA, tMin, closest, t);
}
// ... and on a record the set-up copied into LDS (the head): its three quads as read there, all of them asked for before
// the first is used
struct WfLdsSphere {
  f32x4 q0, q1, q2;
};
__device__ __forceinline__ WfLdsSphere wfLdsSphereLoad(const LdsVec4* rec) { return WfLdsSphere{rec[0], rec[1], rec[2]}; }
__device__ __forceinline__ bool wfSphereHit(const WfLdsSphere& s, const Ray& ray, float rayA, float tMin, float closest, float& t) {
  return wfSphereHitOn(make_float4(s.q0.x, s.q0.y, s.q0.z, s.q0.w), make_float4(s.q1.x, s.q1.y, s.q1.z, s.q1.w),
                       [&]() { return make_float4(s.q2.x, s.q2.y, s.q2.z, s.q2.w); }, ray, rayA, tMin, closest, t);
}

// DevScene::wfHead of the launch, read from the kernel-argument segment where it is called (the swap step): one scalar
// load per swap, and no scalar that lives across the traversal loop (the camera row)
__device__ __forceinline__ int32_t wfHeadFromKernarg() {
  typedef __attribute__((address_space(4))) const unsigned char ConstByte;
  typedef __attribute__((address_space(4))) const int32_t ConstWord;
  ConstByte* p = (ConstByte*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));  // not hoisted out of the loop it is called in
  return *(ConstWord*)(p + offsetof(RenderArgs, scene) + offsetof(DevScene, wfHead));
}
}  // namespace

// SINGLE: the world list is one tree (as in srt_render_kernel).  PROFILE (tunable wf_profile, tools/wf_profile.py): per
// step kind, the clocks the waves spent in it, its executions and the lanes they served -> RenderArgs::stats[32 + ...]
// (kinds: 0 node visit, 1 primitive test, 2 swap, 3-5 hit step per class, 6 restart, 7 idle, 8 lost claim, 9 item pull,
// 10 visit of a node outside LDS -- hybrid form: wait for the records + visit; its clocks are part of kind 0's as well;
// whole-tree form: no clocks, the swap steps that ran the head of the new rays' walks and the lanes they ran it for).
#define WF_PROF_KINDS 12
// HYBRID: the tree does not fit into LDS.  Its top -- the first `resident` records of DevScene::nodesWf, the boxes a ray is
// most likely to meet -- is kept there, the other records are read from global memory where the walk reaches them; a
// node round asks for the global lanes' records first and visits LDS nodes with the other lanes while they are on the way.
// COUNT (a countStats launch): the eight SrtStats counters with srt_render_kernel's definitions -> RenderArgs::stats[0..7],
// and with RenderArgs::aov set the srtRenderAov record of every walk at bounce aovDepth of sample sampleFirst.  A walk
// never leaves its lane before it ends (swapStep hands over finished walks only), so its counters stay in registers.
// MOMENTS (srtRenderTilesMoments): the item's luminance moments ride in the context line (B.w, C.z, see above) and are
// committed with its sum to RenderArgs::mout / mfix.  Every use is under `if constexpr` or a constant select.
template <bool SINGLE, bool PROFILE, bool HYBRID, bool COUNT, bool MOMENTS = false>
__global__ __launch_bounds__(WF_BLOCK, 4) void srt_render_wf_kernel(const RenderArgs a) {
  static_assert(!(MOMENTS && (COUNT || PROFILE)), "the moments instances neither count nor profile");

  // whole tree in LDS: the words of srt_wf_links.h -- a node is its record's LDS byte offset, a leaf one word that holds
  // both objects, a link the successor alone; hitRef and hitPrim[] hold 16-bit primitive references, sign-extended.
  // HYBRID: 32-bit references, DONE = -2^29, a link = successor << 2 | what follows a leaf's first object (srt_device.h)
  constexpr int32_t DONE = HYBRID ? -(1 << 29) : SRT_WF_DONE;
  constexpr int32_t DONE_PAIR = HYBRID ? (int32_t)0x80000000 : SRT_WF_DONE;  // "nothing follows, then done"
  typedef typename std::conditional<HYBRID, int32_t, uint16_t>::type PrimSlot;
  extern __shared__ int32_t lds[];
  const DevScene& sc = a.scene;
  char* const ldsTree = reinterpret_cast<char*>(lds);  // LDS offset 0 (the kernel has no other LDS): a node's offset is its address
  const int resident = HYBRID ? sc.wfResident : sc.numNodes;  // nodes [0, resident) are in LDS
  const int treeBytes = resident * 32;
  // (this carve-up must match srt_lds_layout.h srtWfLdsLayout(resident, RCAP, POOL, HYBRID): the host sizes the launch by it)
  int32_t* const ctl = reinterpret_cast<int32_t*>(ldsTree + treeBytes);
  const int RCAP = a.wfRingCap, POOL = a.wfPoolSize;
  uint16_t* const ringSlots = reinterpret_cast<uint16_t*>(ctl + WF_CTL_WORDS);
  float* const hitT = reinterpret_cast<float*>(ringSlots + WF_RINGS * RCAP);
  PrimSlot* const hitPrim = reinterpret_cast<PrimSlot*>(hitT + POOL);
  const int lane = threadIdx.x & 63;
  const unsigned long long laneBelow = (1ull << lane) - 1ull;  // (the hybrid instances' ring operations; unused in the others)
  const uint64_t seedMixed = mix64(a.seed);
  const V3 background = ld3(a.background);
  // The production, moments and profiling instances over a whole tree walk the REGROUPED tree where the launch has one
  // (DevScene::nodesRg, srt_regroup.h: the same leaves in the same order under other inner nodes -- the same (t, primitive)
  // at the end of every walk, about half the visits on the headline frame).  Wave-uniform, decided once, here.  The
  // counting instances always walk the reference tree: their counters and AOV records are the oracle's.
  const bool regroup = !HYBRID && !COUNT && sc.nodesRg != nullptr;
  const Rsrc rsNodes = makeRsrc(HYBRID ? sc.nodesWf : (regroup ? sc.nodesRg : sc.nodes), sc.numNodes * 32);
  const Rsrc rsTris = makeRsrc(sc.triTest, HYBRID ? sc.numTris * 48 : 0);  // (the whole-tree instances: where an undecided lane needs it)
  const Rsrc rsFast = makeRsrc(sc.triFast, HYBRID ? 0 : sc.numTris * 64);
  const Rsrc rsSpheres = makeRsrc(sc.spheres, sc.numSpheres * 48);
  const Rsrc rsTexels = makeRsrc(sc.texels, sc.texelBytes);
  const Rsrc rsClass = makeRsrc(sc.primClass, sc.numPrimClass);
  const Rsrc rsSecond = makeRsrc(sc.primSecond, HYBRID ? sc.numPrimClass * 4 : 0);
  // this workgroup's contexts: id << 7 is a context's byte offset; attenuation levels of bounces >= 4 live in
  // [level - 4][channel][id] in a second array
  const Rsrc rsPool = makeRsrc(a.wfPool + (size_t)blockIdx.x * POOL * WF_CTX_BYTES, POOL * WF_CTX_BYTES);
  const int hiLevels = a.maxBounce > 4 ? a.maxBounce - 4 : 0;
  const Rsrc rsAttHi = makeRsrc(a.wfAttHi + (size_t)blockIdx.x * 3 * hiLevels * POOL, 3 * hiLevels * POOL * 4);
  const bool singleRoot = SINGLE || sc.numWorld == 1;
  auto worldRef = [&](int k) {
    if (HYBRID) return sc.worldWf[k];
    return srtWfRootWord(sc.world[k]);
  };
  // the rings' capacity RCAP = 2^j or 3 * 2^j (the pool size rounded up to such a number): srtWfRingPos
  const SrtWfRingGeom ringGeom = {a.wfRingCap, a.wfRingShift, a.wfRingMul3};

  // ---- set-up: the threaded tree into LDS, at offset 0, its two link words per node re-encoded for this kernel's walk
  // (srt_wf_links.h; the hybrid form's records are stored ready-made), empty rings, every context waits for an item
  {
    float4* dst = reinterpret_cast<float4*>(ldsTree);
    const int32_t* const threads = regroup ? sc.nodeThreadRg : sc.nodeThread;
    // The regrouped tree's WALK SEQUENCE where the launch hands one over (DevScene::walkSeq, srt_regroup.h srtRegroupWalk:
    // the gates that rarely cull a ray elided): slot j takes its box from the regrouped array's record src[j], as a refit
    // left it, and its two words ready-made; the slots behind the sequence stay unwritten, no link leads there.  The walks
    // start at the sequence's entry words, which the launch put in the world list's place.  Nothing below knows of it.
    const int numSeq = regroup ? sc.numWalk : 0;
    for (int i = threadIdx.x; i < (numSeq > 0 ? numSeq : resident) * 2; i += WF_BLOCK) {
      float4 v;
      if (numSeq > 0) {
        const int32_t* const rec = sc.walkSeq + 3 * (i >> 1);
        v = bufLoad4(rsNodes, 32 * rec[0] + 16 * (i & 1));
        v.w = __int_as_float(rec[1 + (i & 1)]);
      } else {
        v = bufLoad4(rsNodes, 16 * i);
        if (!HYBRID) {  // nodesWf holds the threaded records already
          const int32_t thread = threads[i >> 1];
          v.w = __int_as_float((i & 1) ? srtWfMissWord(thread) : srtWfHitWord(__float_as_int(v.w), thread));
        }
      }
      dst[i] = v;
    }
    for (int i = threadIdx.x; i < WF_CTL_WORDS; i += WF_BLOCK) ctl[i] = 0;
    for (int i = threadIdx.x; i < WF_RINGS * RCAP; i += WF_BLOCK) ringSlots[i] = 0;
    __syncthreads();
    for (int id = threadIdx.x; id < POOL; id += WF_BLOCK) ringSlots[WF_RING_NEWITEM * RCAP + id] = (uint16_t)(id + 1);
    if (threadIdx.x == 0) {
      ctl[WF_CTL_TAIL(WF_RING_NEWITEM)] = POOL;
      ctl[WF_CTL_LIVE] = POOL;
    }
    if (threadIdx.x < 16) ctl[threadIdx.x] = (int)(blockIdx.x % (unsigned)a.numQueues);  // the waves' home work queue
    if constexpr (!HYBRID && !COUNT) {
      // The sphere records of the walks' head leaf (swapStep), as DevScene::spheres holds them at this launch -- an update of
      // the spheres between launches needs nothing more: one thread per 16-byte quad, the first object's three and, where the
      // leaf has a second object, its three (zeros otherwise).  Read-only from the barrier below on.
      const int32_t leaf = sc.wfHead;
      const int quad = (int)threadIdx.x - 64;  // (the second wave: the first has the words above to write)
      if (leaf != 0 && quad >= 0 && quad < (srtWfLeafHasSecond(leaf) ? 6 : 3)) {
        const int ref = quad < 3 ? srtWfLeafFirst(leaf) : srtWfLeafFirst(srtWfLeafRest(leaf));
        reinterpret_cast<float4*>(ctl + WF_CTL_LEAFREC)[quad] = bufLoad4(rsSpheres, (~ref >> 1) * 48 + 16 * (quad < 3 ? quad : quad - 3));
      }
    }
    __syncthreads();
  }
  int32_t* const waveQueue = ctl + (threadIdx.x >> 6);
  const int qHome = (int)(blockIdx.x % (unsigned)a.numQueues);
  const int unitItems = a.unitTiles * a.sppChunks * SRT_TILE_PIXELS;
  auto queueEnd = [&](int q) { return (q < a.numUnits ? (a.numUnits - q + a.numQueues - 1) / a.numQueues : 0) * unitItems; };

  auto raiseAbort = [&]() {
    if (__hip_atomic_exchange(&ctl[WF_CTL_ABORT], 1, __ATOMIC_RELAXED, WF_WG) == 0 && a.wfError) atomicAdd(a.wfError, 1);
  };
  // ---- rings.  A slot holds id + 1, 0 = empty.  Producers reserve places with one atomic per wave and fill them;
  // consumers claim places (compare-and-swap on the head, never beyond the tail) and take the ids, waiting the few
  // cycles a reserved place may still be unwritten.  Slots are re-used only after their consumer emptied them.
  // What a producer wrote for the context BEFORE (global stores: the caller fences; LDS: one wave's LDS operations
  // execute in order) is visible to the consumer that finds the id.
  // The two operations are srt_wf_rings.h's; a call site names the rings it can produce (`ring` < 0: this lane enqueues nothing).
  // The instances over an LDS-resident tree, bound by vector-ALU issue, take the forms specialised per call site; the hybrid
  // instances keep the generic ones.
  auto enqueue = [&](auto set, int ring, int id) {
    if constexpr (HYBRID)
      srtWfEnqueueGeneric(ctl, ringSlots, ringGeom, lane, laneBelow, ring, id, raiseAbort);
    else
      srtWfEnqueue<decltype(set)::value>(ctl, ringSlots, ringGeom, lane, ring, id, raiseAbort);
  };

  // ---- lane state: a traversal engine
  int path = -1;  // context id being traversed, -1 = idle
  int cur = DONE, hitRef = DONE, w = 0;
  int32_t link = DONE_PAIR;
  Ray ray;
  ray.o = ray.d = mk(0.0f, 0.0f, 0.0f);
  ray.time = 0.0f;
  float closest = SRT_INF, rayA = 0.0f, slabTol = SRT_INF;
  // The slab test's per-ray values.  The whole-tree instances, bound by vector-ALU issue, take the sign form (srt_slab.h:
  // twelve FMAs per visit and no min/max pairs) and keep the reciprocal split by its sign, rp = max(r, 0) and
  // rq = min(r, 0); the hybrid instances keep the min/max form, and the reciprocal itself in rp.
  constexpr bool SIGNFORM = !HYBRID;
  V3 rp = mk(0.0f, 0.0f, 0.0f), rq = mk(0.0f, 0.0f, 0.0f), negOR = mk(0.0f, 0.0f, 0.0f);
  auto atNode = [&]() { return cur >= 0; };
  auto atPrim = [&]() { return (uint32_t)cur > (uint32_t)DONE; };
  // COUNT: samples, rays, node visits, box passes, triangle / sphere tests, shaded triangle hits, texel fetches (SrtStats
  // order); the counters at the start of the lane's walk, and the pixel its walk is the srtRenderAov record of (-1: none).
  // Every use is under `if constexpr`: the other instances' lambdas capture none of it, and their code stays as it was.
  unsigned long long cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t walk0[4] = {0, 0, 0, 0};
  int aovPixel = -1;
  auto popNext = [&]() {
    int next;
    if (HYBRID) {
      const int follows = link & 3;
      next = link >> 2;
      if (follows == 1) next = cur - 2;                                                                   // the next primitive of the same array
      if (follows == 2) next = (int)__builtin_amdgcn_raw_buffer_load_b32(rsSecond, (~cur) << 2, 0, 0);  // any other pair (rare)
      link &= ~3;
    } else {
      next = srtWfLeafHasSecond(cur) ? srtWfLeafRest(cur) : link;
    }
    if (!SINGLE && !singleRoot && next == DONE && ++w < sc.numWorld) {
      next = worldRef(w);
      link = DONE_PAIR;
    }
    cur = next;
  };
  auto startTraversal = [&]() {  // world.hit(r, 0.001, infinity, rec)
    if constexpr (COUNT) {
      cnt[1]++;
      for (int k = 0; k < 4; ++k) walk0[k] = (uint32_t)cnt[2 + k];
    }
    rayA = lenSq(ray.d);
    const bool certified = (sc.fastDivScene != 0) & fastDivOperandOk(ray.o.x, ray.d.x) & fastDivOperandOk(ray.o.y, ray.d.y) &
                           fastDivOperandOk(ray.o.z, ray.d.z);
    const V3 rcp = mk(refinedRcp(ray.d.x), refinedRcp(ray.d.y), refinedRcp(ray.d.z));
    if constexpr (SIGNFORM) {
      // a scene with a box that is not ordered: no ray is certified, every visit takes the exact test
      slabSetupSign(ray.o, rcp, certified & (sc.boxOrderedScene != 0), rp, rq, negOR, slabTol);
    } else {
      rp = rcp;
      slabSetup(ray.o, rp, certified, negOR, slabTol);
    }
    closest = SRT_INF;
    hitRef = DONE;
    link = DONE_PAIR;
    w = 0;
    cur = worldRef(0);
  };
  // the next camera ray of a context (main.cpp:204-216): A, B, C of its line (MOMENTS: with the item's moments m1, m2)
  auto cameraRayInto = [&](int at, uint32_t pxy, int s, float m1 = 0.0f, float m2 = 0.0f) {
    const int px = (int)(pxy & 0xffffu), py = (int)(pxy >> 16);
    Pcg rng;
    rng.key(seedMixed, (uint32_t)(py * a.imageWidth + px), (uint32_t)s);
    const float u = ((float)px + rng.uniform()) / (float)(a.imageWidth - 1);                      // main.cpp:210
    const float v = ((float)(a.imageHeight - py) + rng.uniform()) / (float)(a.imageHeight - 1);  // main.cpp:211
    Ray r;
    const DevCamera cam = cameraFromKernarg();
    cameraRay(cam, u, v, rng, r);
    if constexpr (COUNT) cnt[0]++;
    bufStore4(rsPool, at, make_float4(r.o.x, r.o.y, r.o.z, r.time));
    bufStore4(rsPool, at + 16, make_float4(r.d.x, r.d.y, r.d.z, MOMENTS ? m1 : 0.0f));
    u32x4 Cn;
    Cn.x = (uint32_t)rng.state;
    Cn.y = (uint32_t)(rng.state >> 32);
    Cn.z = MOMENTS ? __float_as_uint(m2) : 0u;
    Cn.w = 0;  // depth 0, in flight (a miss unless a hit step says otherwise)
    __builtin_amdgcn_raw_buffer_store_b128(Cn, rsPool, at + 32, 0, 0);
  };

  int idleTrips = 0;  // consecutive decisions that found nothing to do (bounded: see "Termination" above)
  uint32_t tick = 0;
  unsigned long long pCyc[WF_PROF_KINDS], pRuns[WF_PROF_KINDS], pLanes[WF_PROF_KINDS], pSched = 0;
  // what the scheduling decisions that looked at the rings saw, summed: decisions, lanes at nodes / at primitives /
  // finished / idle, READY fill, fill of the fullest served ring, RESTART fill
  unsigned long long pSaw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < WF_PROF_KINDS; ++k) pCyc[k] = pRuns[k] = pLanes[k] = 0;
  const unsigned long long pStart = PROFILE ? clock64() : 0;
  unsigned long long pT = pStart;  // the clock at the end of the last step: what follows until the next step begins is scheduling
  auto prof = [&](int kind, int lanes) {  // closes the step that began at pT
    if (PROFILE) {
      const unsigned long long now = clock64();
      pCyc[kind] += now - pT;
      pRuns[kind]++;
      pLanes[kind] += lanes;
      pT = now;
    }
  };
  // ---- the two traversal steps (as srt_render_kernel's, over the threaded tree in LDS)
  auto primStep = [&]() -> int {  // returns the lanes at nodes afterwards
    int nNodes;
      // ------------------------------------------------ sphere::hit / triangle::hit (as srt_render_kernel)
      for (int round = 0; round < SRT_PRIM_ROUNDS; ++round) {
        if (round > 0 && __popcll(__ballot(atPrim())) < a.primAgainMin) break;
        if (PROFILE) {
          pRuns[1]++;
          pLanes[1] += __popcll(__ballot(atPrim()));
        }
        if (atPrim()) {
          const int ref = HYBRID ? cur : srtWfLeafFirst(cur);  // the object this lane stands on
          const int pr = ~ref;
          float t;
          bool ok;
          if (pr & 1) {
            if constexpr (COUNT) cnt[5]++;
            ok = wfSphereHit(rsSpheres, (pr >> 1) * 48, ray, rayA, a.tMin, closest, t);
          } else {
            if constexpr (COUNT) cnt[4]++;
            if constexpr (HYBRID) {
              // The hybrid form's walks wait for the caches or HBM, where the 64-byte record costs more than the arithmetic
              // saves: its instances keep the exact test, and their code.
              const int off = (pr >> 1) * 48;
              ok = triHitV<false>(bufLoad4(rsTris, off), bufLoad4(rsTris, off + 16), bufLoad4(rsTris, off + 32), ray, a.tMin, closest, t);
            } else {
              // the certified test on the triangle's one 64-byte line (srt_tri_hit.h); the exact test, on its triTest record,
              // for the lanes whose edge signs are not certain -- a block the wave enters only when some lane needs it
              bool unsure;
              const int off = (pr >> 1) * 64;
              ok = srtTriHitCert(bufLoad4(rsFast, off), bufLoad4(rsFast, off + 16), bufLoad4(rsFast, off + 32), bufLoad4(rsFast, off + 48),
                                 triRay(ray), a.tMin, sc.triWMax, t, unsure);
              const unsigned long long mu = __ballot(unsure);
              if (PROFILE) {  // lanes the certificate left undecided, and primitive-step executions that ran the exact test
                pRuns[11] += __popcll(mu);
                pCyc[11] += mu != 0 ? 1 : 0;
              }
              if (mu != 0) {
                if (unsure) {
                  const Rsrc rsExact = makeRsrc(sc.triTest, sc.numTris * 48);
                  const int at = (pr >> 1) * 48;
                  ok = triHitV<false>(bufLoad4(rsExact, at), bufLoad4(rsExact, at + 16), bufLoad4(rsExact, at + 32), ray, a.tMin, closest, t);
                }
              }
            }
          }
          if (ok) {
            closest = t;
            hitRef = ref;
          }
          popNext();
        }
      }
      nNodes = __popcll(__ballot(atNode()));
      if (PROFILE) {
        const unsigned long long now = clock64();
        pCyc[1] += now - pT;
        pT = now;
      }
      return nNodes;
  };
  auto nodeBurst = [&](int nNodes) -> int {  // returns the lanes at nodes afterwards
      // ------------------------------------------------ bvhNode::hit, bvh.h:97-105, over the threaded tree in LDS
      const int keep = (nNodes * a.keepEighths) >> 3;
      int budget = a.nodeBurst, left;
      auto visit = [&](const float4 n0, const float4 n1) {  // aabb::hit (certified slab test, IEEE when undecided), then on
        bool undecided;
        bool hitBox = SIGNFORM ? boxHitSign<true>(n0, n1, rp, rq, negOR, slabTol, a.tMin, closest, undecided)
                               : boxHitApprox<true>(n0, n1, rp, negOR, slabTol, a.tMin, closest, undecided);
        if (PROFILE) {  // how often the certificate cannot decide: lanes (-> lanes[8]) and wave visits that run the IEEE test (-> lanes[7])
          const unsigned long long mu = __ballot(undecided);
          pLanes[8] += __popcll(mu);
          pLanes[7] += mu != 0 ? 1 : 0;
        }
        if constexpr (HYBRID || COUNT) {
          if (undecided) hitBox = boxHit(n0, n1, ray, a.tMin, closest);
        } else {
          // An inner node of the regrouped tree is a GATE: what it decides is only whether the leaves below are looked at,
          // and it must pass wherever one of them would (boxHitOrGate, srt_path.h: closed on an axis with d == +-0).  Leaves,
          // and every node of the reference tree, get boxHit's own operations from the same call.
          if (undecided) hitBox = boxHitOrGate(n0, n1, ray, a.tMin, closest, regroup & (__float_as_int(n0.w) >= 0));
        }
        if constexpr (COUNT) {
          cnt[2]++;
          if (hitBox) cnt[3]++;
        }
        link = __float_as_int(n1.w);
        cur = hitBox ? __float_as_int(n0.w) : (HYBRID ? link >> 2 : link);
        if (!SINGLE && !singleRoot && cur == DONE && ++w < sc.numWorld) {
          cur = worldRef(w);
          link = DONE_PAIR;
        }
      };
      auto nodeVisit = [&](bool mine) {
        const bool here = HYBRID ? mine && (uint32_t)cur < (uint32_t)resident : cur >= 0;
        if (PROFILE) {
          pRuns[0]++;
          pLanes[0] += __popcll(__ballot(here));
        }
        if (here) {
          if constexpr (HYBRID) {
            const char* rec = ldsTree + (cur << 5);
            visit(*reinterpret_cast<const float4*>(rec), *reinterpret_cast<const float4*>(rec + 16));
          } else {
            // the tree sits at LDS offset 0: `cur` IS the record's LDS address (no base to add, not even a zero one)
            const LdsVec4* rec = (const LdsVec4*)(uintptr_t)(uint32_t)cur;
            const f32x4 n0 = rec[0], n1 = rec[1];
            visit(make_float4(n0.x, n0.y, n0.z, n0.w), make_float4(n1.x, n1.y, n1.z, n1.w));
          }
        }
      };
      do {
        if (HYBRID) {
          // the lanes at a node outside LDS ask for its record; the others visit LDS nodes meanwhile (wfFarRounds - 1 times,
          // or until none of them is at one) and then fetch one more record from LDS, so that the last visit of the round
          // serves both groups in one execution
          const bool far = cur >= resident;
          float4 g0, g1;  // (read only by the lanes that load them below)
          if (far) {
            g0 = bufLoad4(rsNodes, cur << 5);
            g1 = bufLoad4(rsNodes, (cur << 5) + 16);
          }
          // no loop here: a loop header makes the compiler wait for the loads above before the LDS visits begin
          if (a.wfFarRounds > 1) nodeVisit(!far);
          if (a.wfFarRounds > 2) nodeVisit(!far);
          if (a.wfFarRounds > 3) nodeVisit(!far);
          const bool near = !far && (uint32_t)cur < (uint32_t)resident;
          if (near) {
            const char* rec = ldsTree + (cur << 5);
            g0 = *reinterpret_cast<const float4*>(rec);
            g1 = *reinterpret_cast<const float4*>(rec + 16);
          }
          const unsigned long long f0 = PROFILE ? clock64() : 0;
          if (far || near) visit(g0, g1);
          if (PROFILE) {
            pRuns[10]++;
            pLanes[10] += __popcll(__ballot(far));
            pLanes[11] += __popcll(__ballot(near));
            pCyc[10] += clock64() - f0;
          }
        } else {
#pragma unroll
          for (int u = 0; u < SRT_NODE_UNROLL; ++u) nodeVisit(true);
        }
        budget -= HYBRID ? a.wfFarRounds : SRT_NODE_UNROLL;
        left = __popcll(__ballot(atNode()));
      } while (budget > 0 && left >= keep);
      if (PROFILE) {
        const unsigned long long now = clock64();
        pCyc[0] += now - pT;
        pT = now;
      }
      return left;
  };
  // ---- swap step: finished walks out, READY contexts in
  auto swapStep = [&]() {
      // ------------------------------------------------ finished walks out, READY contexts in.  The new rays' lines are
      // asked for first and arrive while the finished walks are handed over (LDS traffic only).
      const bool fin = cur == DONE && path >= 0;
      const bool hit = fin && hitRef != DONE;
      const bool need = path < 0 || fin;
      const unsigned long long mNeed = __ballot(need);
      int id = -1;
      // the class of the hit primitive's material picks the ring: asked for first, it is there when the claim is done
      int cls = 0;
      if (hit) cls = (int)__builtin_amdgcn_raw_buffer_load_b8(rsClass, ~hitRef, 0, 0);
      const unsigned long long q0 = PROFILE ? clock64() : 0;
      if (mNeed != 0) {
        if constexpr (HYBRID)
          srtWfClaimGeneric(ctl, ringSlots, ringGeom, lane, laneBelow, WF_RING_READY, mNeed, __popcll(mNeed), 1, id, raiseAbort);
        else
          srtWfClaim(ctl, ringSlots, ringGeom, lane, WF_RING_READY, need, mNeed, __popcll(mNeed), 1, id, raiseAbort);
      }
      const unsigned long long q1 = PROFILE ? clock64() : 0;
      float4 A = make_float4(0.0f, 0.0f, 0.0f, 0.0f), B = A;
      if (id >= 0) {
        A = bufLoad4(rsPool, id << 7);
        B = bufLoad4(rsPool, (id << 7) + 16);
      }
      if (hit) {
        // what the hit step needs beyond the ray: t and the primitive (LDS).  A miss leaves nothing: the context already
        // says "in flight, nothing hit".
        __hip_atomic_store(&hitT[path], closest, __ATOMIC_RELAXED, WF_WG);
        __hip_atomic_store(&hitPrim[path], (PrimSlot)hitRef, __ATOMIC_RELAXED, WF_WG);
      }
      asm volatile("" ::: "memory");  // the ring slot is written after them (one wave's LDS operations execute in order)
      enqueue(WF_SET_OF(WF_SET(WF_RING_RESTART) | WF_SET(WF_RING_HIT) | WF_SET(WF_RING_HIT + 1) | WF_SET(WF_RING_HIT + 2)),
              !fin ? -1 : (hit ? WF_RING_HIT + cls : WF_RING_RESTART), path);
      if constexpr (COUNT) {
        if (fin && aovPixel >= 0) {  // as srt_render_kernel's writeAov: the finished walk's ray, hit and counters
          SrtAovRecord r;
          r.o[0] = ray.o.x; r.o[1] = ray.o.y; r.o[2] = ray.o.z;
          r.d[0] = ray.d.x; r.d[1] = ray.d.y; r.d[2] = ray.d.z;
          r.time = ray.time;
          r.valid = 1;
          r.prim = SRT_NO_HIT;
          r.t = 0.0f;
          if (hitRef != DONE) {
            const int pr = ~hitRef;
            r.prim = (pr & 1) ? sc.sphPrimId[pr >> 1] : sc.triPrimId[pr >> 1];
            r.t = closest;
          }
          r.nodeVisits = (int32_t)((uint32_t)cnt[2] - walk0[0]);
          r.boxPasses = (int32_t)((uint32_t)cnt[3] - walk0[1]);
          r.triTests = (int32_t)((uint32_t)cnt[4] - walk0[2]);
          r.sphereTests = (int32_t)((uint32_t)cnt[5] - walk0[3]);
          r.pad[0] = r.pad[1] = 0;
          a.aov[aovPixel] = r;
        }
      }
      if (fin) {
        path = -1;
        hitRef = DONE;
      }
      const unsigned long long q2 = PROFILE ? clock64() : 0;
      // The HEAD of the walks (DevScene::wfHead; the instances that walk the sequence): a leaf word != 0 says that every walk
      // of this launch begins at that leaf -- no gate in front of it, spheres alone in it, its hit and miss words lead to the
      // same successor.  Its visit and its one or two sphere tests run here, for all the new rays at once and on wave-uniform
      // records (read from LDS, where the set-up put them: control words WF_CTL_LEAFREC..), and the walks start at its miss
      // word: what the loop would have done with these lanes in a node burst at partial fill and two primitive rounds shared
      // with lanes at triangles.  Same calls, same values, same order.
      const int32_t head = !HYBRID && !COUNT ? wfHeadFromKernarg() : 0;
      if (id >= 0) {
        ray.o = mk(A.x, A.y, A.z);
        ray.d = mk(B.x, B.y, B.z);
        ray.time = A.w;
        path = id;
        startTraversal();
        if constexpr (!HYBRID && !COUNT) {
          if (head != 0) {
            // visit()'s verdict for a leaf, bit for bit; `cur` is the entry word, the record's LDS address
            const LdsVec4* rec = (const LdsVec4*)(uintptr_t)(uint32_t)cur;
            const f32x4 r0 = rec[0], r1 = rec[1];
            // ... and the leaf's sphere records, from the control words the set-up copied them to: every lane reads the same
            // slots (a broadcast), and the requests go out with the box's, in front of the box test -- no load of the head
            // waits for a test, and none goes through the vector memory path
            const LdsVec4* leafRec = (const LdsVec4*)(ctl + WF_CTL_LEAFREC);
            // (both slots and the moving quads unconditionally: a branch around the second slot's reads made the compiler wait
            // for the first slot's before it issued them, a second round trip; a slot of zeros is read and not used)
            const WfLdsSphere sph1 = wfLdsSphereLoad(leafRec), sph2 = wfLdsSphereLoad(leafRec + 3);
            const float4 n0 = make_float4(r0.x, r0.y, r0.z, r0.w), n1 = make_float4(r1.x, r1.y, r1.z, r1.w);
            bool undecided;
            bool hitBox = boxHitSign<true>(n0, n1, rp, rq, negOR, slabTol, a.tMin, closest, undecided);
            if (__ballot(undecided)) {
              if (undecided) hitBox = boxHit(n0, n1, ray, a.tMin, closest);
            }
            if (hitBox) {
              float t;
              const int first = srtWfLeafFirst(head);
              if (wfSphereHit(sph1, ray, rayA, a.tMin, closest, t)) {
                closest = t;
                hitRef = first;
              }
              if (srtWfLeafHasSecond(head)) {
                const int second = srtWfLeafFirst(srtWfLeafRest(head));
                if (wfSphereHit(sph2, ray, rayA, a.tMin, closest, t)) {
                  closest = t;
                  hitRef = second;
                }
              }
            }
            cur = __float_as_int(n1.w);  // the leaf's miss word (DONE: a tree of this one leaf -- the next swap hands the walk over)
          }
        }
        if constexpr (COUNT) {
          // the new ray's bounce, sample and pixel (context words C.w, E.y, E.w): is its walk the AOV record of its pixel?
          aovPixel = -1;
          if (a.aov) {
            const uint32_t cw = bufLoad1(rsPool, (id << 7) + 44);
            const u32x4 E = __builtin_amdgcn_raw_buffer_load_b128(rsPool, (id << 7) + 64, 0, 0);
            const int px = (int)(E.w & 0xffffu), py = (int)(E.w >> 16);
            if ((int)(cw & 0xffu) == a.aovDepth && (int)E.y == a.sampleFirst) aovPixel = py * a.imageWidth + px;
          }
        }
      }
      if (PROFILE) {
        const unsigned long long q3 = clock64();
        pSaw[5] += q1 - q0;  // swap: claim
        pSaw[6] += q2 - q1;  // swap: hand-over of the finished walks
        pSaw[7] += q3 - q2;  // swap: new rays arrive, set-up (and the head of their walks)
        if (head != 0 && __ballot(id >= 0) != 0) {  // kind 10 in this form: swap steps that ran the head, and its lanes
          pRuns[10]++;
          pLanes[10] += __popcll(__ballot(id >= 0));
        }
      }
      prof(2, __popcll(__ballot(fin)) + __popcll(__ballot(id >= 0)));
  };
  // ---- serve step: up to 64 contexts of ring `bestRing` (none unless `serveAtLeast` are there); returns how many
  auto serveStep = [&](int bestRing, int serveAtLeast) -> int {
      // ------------------------------------------------ serve a ring: 64 contexts in the same state
      int id;
      const unsigned long long h0 = PROFILE ? clock64() : 0;
      int k;
      if constexpr (HYBRID)
        k = srtWfClaimGeneric(ctl, ringSlots, ringGeom, lane, laneBelow, bestRing, ~0ull, 64, serveAtLeast, id, raiseAbort);
      else
        k = srtWfClaimAll(ctl, ringSlots, ringGeom, lane, bestRing, 64, serveAtLeast, id, raiseAbort);
      if (k == 0) {  // another wave took them
        prof(8, 0);
        return 0;
      }
      const int at = id << 7;
      if (bestRing >= WF_RING_HIT && bestRing < WF_RING_HIT + WF_CLASSES) {
        // ---------------------------- rayColor's hit branch (main.cpp:42-51): one path vertex per lane
        bool toReady = false, toRestart = false;
        if (id >= 0) {
          const float4 A = bufLoad4(rsPool, at), B = bufLoad4(rsPool, at + 16);
          const u32x4 C = __builtin_amdgcn_raw_buffer_load_b128(rsPool, at + 32, 0, 0);
          const float tHit = __hip_atomic_load(&hitT[id], __ATOMIC_RELAXED, WF_WG);
          const int pr = HYBRID ? ~(int)__hip_atomic_load(&hitPrim[id], __ATOMIC_RELAXED, WF_WG)
                                : ~(int)(int16_t)__hip_atomic_load(&hitPrim[id], __ATOMIC_RELAXED, WF_WG);
          Ray rIn;
          rIn.o = mk(A.x, A.y, A.z);
          rIn.d = mk(B.x, B.y, B.z);
          rIn.time = A.w;
          Pcg rng;
          rng.state = (uint64_t)C.x | ((uint64_t)C.y << 32);
          int depth = (int)(C.w & 0xffu);
          Record rec;
          const unsigned long long h1 = PROFILE ? clock64() : 0;
          if (pr & 1)
            sphereRecord(sc, pr >> 1, rIn, tHit, rec, false);
          else
            triRecord(sc, pr >> 1, rIn, tHit, rec, false);
          V3 att, emitted;
          Ray next;
          uint32_t fetches = 0;
          if constexpr (COUNT) cnt[6] += rec.isTri ? 1 : 0;
          const unsigned long long h2 = PROFILE ? clock64() : 0;
          const bool scattered = shade<COUNT, true>(sc, rsTexels, rIn, rec, rng, att, next, emitted, fetches, nullptr);
          if constexpr (COUNT) cnt[7] += fetches;
          if (PROFILE && bestRing == WF_RING_HIT + 1) {  // the ground's class: claim + context / record / shade (lane 0's clocks)
            const unsigned long long h3 = clock64();
            pSaw[1] += h1 - h0;
            pSaw[2] += h2 - h1;
            pSaw[3] += h3 - h2;
            pSaw[4] += 1;
          }
          V3 terminal = emitted;  // main.cpp:46-47
          bool done = true;
          if (scattered) {
            // emitted is (0,0,0) for every scattering material (material.h:18-20): keep the attenuation of this level
            if (depth < 4) {
              bufStore1(rsPool, at + 80 + 12 * depth, __float_as_uint(att.x));
              bufStore1(rsPool, at + 84 + 12 * depth, __float_as_uint(att.y));
              bufStore1(rsPool, at + 88 + 12 * depth, __float_as_uint(att.z));
            } else {
              const int slot = (3 * (depth - 4) * POOL + id) * 4;
              bufStore1(rsAttHi, slot, __float_as_uint(att.x));
              bufStore1(rsAttHi, slot + POOL * 4, __float_as_uint(att.y));
              bufStore1(rsAttHi, slot + POOL * 8, __float_as_uint(att.z));
            }
            depth++;
            done = depth >= a.maxBounce;  // main.cpp:36-37: out of bounces -> black
            terminal = mk(0.0f, 0.0f, 0.0f);
          }
          u32x4 Cn;
          Cn.x = (uint32_t)rng.state;
          Cn.y = (uint32_t)(rng.state >> 32);
          Cn.z = MOMENTS ? C.z : 0u;  // (B.w and C.z: the item's moments, carried over)
          if (done) {
            // the path ends here: its terminal radiance takes the (dead) direction's place
            bufStore4(rsPool, at + 16, make_float4(terminal.x, terminal.y, terminal.z, MOMENTS ? B.w : 0.0f));
            Cn.w = (uint32_t)depth | (WF_PEND_TERMINAL << 8);
            toRestart = true;
          } else {
            bufStore4(rsPool, at, make_float4(next.o.x, next.o.y, next.o.z, next.time));
            bufStore4(rsPool, at + 16, make_float4(next.d.x, next.d.y, next.d.z, MOMENTS ? B.w : 0.0f));
            Cn.w = (uint32_t)depth;
            toReady = true;
          }
          __builtin_amdgcn_raw_buffer_store_b128(Cn, rsPool, at + 32, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        enqueue(WF_SET_OF(WF_SET(WF_RING_READY) | WF_SET(WF_RING_RESTART)), toReady ? WF_RING_READY : (toRestart ? WF_RING_RESTART : -1), id);
        prof(3 + bestRing - WF_RING_HIT, k);
      } else if (bestRing == WF_RING_RESTART) {
        // ---------------------------- a sample is in: miss / path end (main.cpp:39-40,49-51), pixel sum (main.cpp:217),
        // next camera ray of the item (main.cpp:204-216) -- or, after the item's last sample, its sum goes out and the
        // context goes for the next item
        bool toReady = false, toNewItem = false;
        if (id >= 0) {
          // the whole line at once: one round trip
          const float4 B = bufLoad4(rsPool, at + 16);
          const u32x4 C = __builtin_amdgcn_raw_buffer_load_b128(rsPool, at + 32, 0, 0);
          float4 D = bufLoad4(rsPool, at + 48);
          const u32x4 E = __builtin_amdgcn_raw_buffer_load_b128(rsPool, at + 64, 0, 0);
          const float4 F = bufLoad4(rsPool, at + 80), G = bufLoad4(rsPool, at + 96), H = bufLoad4(rsPool, at + 112);
          const int outIndex = (int)E.x, sEnd = (int)E.z;
          int s = (int)E.y;
          const int depth = (int)(C.w & 0xffu), pend = (int)((C.w >> 8) & 0xffu);
          V3 L = background;  // main.cpp:39-40 (the ray went out of the scene)
          if (pend == WF_PEND_TERMINAL) L = mk(B.x, B.y, B.z);
          // unwind the recursion: emitted + newColor * attenuation, innermost first (main.cpp:49-51)
          const float lv[12] = {F.x, F.y, F.z, F.w, G.x, G.y, G.z, G.w, H.x, H.y, H.z, H.w};
          for (int j = depth - 1; j >= 4; --j) {
            const int slot = (3 * (j - 4) * POOL + id) * 4;
            const float ax = __uint_as_float(bufLoad1(rsAttHi, slot)), ay = __uint_as_float(bufLoad1(rsAttHi, slot + POOL * 4)),
                        az = __uint_as_float(bufLoad1(rsAttHi, slot + POOL * 8));
            L = mk(0.0f + L.x * ax, 0.0f + L.y * ay, 0.0f + L.z * az);
          }
#pragma unroll
          for (int j = 3; j >= 0; --j)
            if (j < depth) L = mk(0.0f + L.x * lv[3 * j], 0.0f + L.y * lv[3 * j + 1], 0.0f + L.z * lv[3 * j + 2]);
          D.x += L.x;  // main.cpp:217
          D.y += L.y;
          D.z += L.z;
          float m1 = 0.0f, m2 = 0.0f;
          if constexpr (MOMENTS) {
            const float l = sampleLum(L);
            m1 = B.w + l;
            m2 = __uint_as_float(C.z) + l * l;
          }
          s++;
          if (s < sEnd) {
            bufStore4(rsPool, at + 48, D);
            bufStore1(rsPool, at + 68, (uint32_t)s);
            if constexpr (MOMENTS)
              cameraRayInto(at, E.w, s, m1, m2);
            else
              cameraRayInto(at, E.w, s);
            toReady = true;
          } else {
            // the item is complete: its partial sum goes out (exact chunk sums: srt_path.h)
            if (outIndex >= 0) {
              if (a.fix)
                commitFixed(a.fix + outIndex, mk(D.x, D.y, D.z), a.fixLimit);
              else
                a.out[outIndex] = D;
              if constexpr (MOMENTS) {
                if (a.mfix)
                  commitFixed(a.mfix + outIndex, mk(m1, m2, 0.0f), a.fixLimit);
                else
                  a.mout[outIndex] = make_float4(m1, m2, 0.0f, D.w);
              }
            }
            toNewItem = true;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        enqueue(WF_SET_OF(WF_SET(WF_RING_READY) | WF_SET(WF_RING_NEWITEM)), toReady ? WF_RING_READY : (toNewItem ? WF_RING_NEWITEM : -1), id);
        prof(6, k);
      } else {
        // ---------------------------- the next work item for every context here, with one atomic for the wave
        // (main.cpp:200-203: the pixel loop; work queues as in srt_render_kernel), and its first camera ray
        const bool need = id >= 0;
        const unsigned long long mF2 = __ballot(need);
        const int q = __builtin_amdgcn_readfirstlane(*waveQueue);
        bool gotItem = false, alive = true;
        int idx = 0;
        if (q >= 0) {
          int base = 0;
          if (lane == 0) base = atomicAdd(a.queue + 16 * q, __popcll(mF2));
          base = __builtin_amdgcn_readfirstlane(base);
          idx = HYBRID ? base + __popcll(mF2 & laneBelow) : (int)srtWfReservePlace((uint32_t)base, mF2, lane);
          const int qEnd = queueEnd(q);
          gotItem = need && idx < qEnd;
          if (base + __popcll(mF2) > qEnd) {
            // drained: lane 0 looks at every queue's counter, the wave moves to the fullest one (own XCD first)
            int nq = -1;
            if (lane == 0) {
              int bestLeft = 0;
              bool bestOwn = false;
              for (int kq = 0; kq < a.numQueues; ++kq) {
                const int left = queueEnd(kq) - __hip_atomic_load(a.queue + 16 * kq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool own = ((kq ^ qHome) & 7) == 0;
                if (left > 0 && ((own && !bestOwn) || (own == bestOwn && left > bestLeft))) {
                  bestLeft = left;
                  bestOwn = own;
                  nq = kq;
                }
              }
              *waveQueue = nq;
            }
            nq = __builtin_amdgcn_readfirstlane(nq);
            if (nq < 0) alive = false;
          }
        } else {
          alive = false;
        }
        bool toReady = false, again = false, retired = false;
        if (need) {
          if (!gotItem) {
            retired = !alive;  // nothing left anywhere: this context is done
            again = alive;     // the wave's queue ran dry under it: pull again from the new one
          } else {
            // idx -> (local tile, chunk, pixel of the tile), without integer divisions (as srt_render_kernel)
            const int group = idx >> 6, ln = idx & 63;
            int u = (int)((float)group * a.rcpUnitGroups);
            int inUnit = group - u * a.unitGroups;
            if (inUnit < 0) {
              u--;
              inUnit += a.unitGroups;
            } else if (inUnit >= a.unitGroups) {
              u++;
              inUnit -= a.unitGroups;
            }
            int tileInUnit = (int)((float)inUnit * a.rcpChunks);
            int chunk = inUnit - tileInUnit * a.sppChunks;
            if (chunk < 0) {
              tileInUnit--;
              chunk += a.sppChunks;
            } else if (chunk >= a.sppChunks) {
              tileInUnit++;
              chunk -= a.sppChunks;
            }
            const int localTile = (q + u * a.numQueues) * a.unitTiles + tileInUnit;  // may pad past numLocalTiles
            const int tile = a.tileFirst + localTile * a.tileStride;
            const uint32_t txy = a.tileXY[tile < a.numTiles ? tile : 0];
            const int px = (int)(txy & 0xffffu) * SRT_TILE_W + (ln & (SRT_TILE_W - 1));
            const int py = (int)(txy >> 16) * SRT_TILE_H + (ln >> 3);
            const uint32_t pxy = (uint32_t)px | ((uint32_t)py << 16);
            const int s0 = a.sampleFirst + chunk * a.sppBase + min(chunk, a.sppRem);
            const int s1 = s0 + a.sppBase + (chunk < a.sppRem ? 1 : 0);
            // maxBounce <= 0: rayColor returns black before tracing anything (main.cpp:36-37)
            const bool valid = localTile < a.numLocalTiles && tile < a.numTiles && px < a.imageWidth && py < a.imageHeight && a.maxBounce > 0;
            const int outIndex = localTile < a.numLocalTiles ? chunk * a.chunkStride + localTile * SRT_TILE_PIXELS + ln : -1;
            const float4 D = make_float4(0.0f, 0.0f, 0.0f, (float)(s1 - s0));
            if (valid) {
              bufStore4(rsPool, at + 48, D);
              u32x4 En;
              En.x = (uint32_t)outIndex;
              En.y = (uint32_t)s0;
              En.z = (uint32_t)s1;
              En.w = pxy;
              __builtin_amdgcn_raw_buffer_store_b128(En, rsPool, at + 64, 0, 0);
              cameraRayInto(at, pxy, s0);
              toReady = true;
            } else {
              // an item with nothing to trace (a pixel outside the image, or no bounces): its zero sum is written at once
              if (outIndex >= 0 && !a.fix) a.out[outIndex] = D;
              if constexpr (MOMENTS) {
                if (outIndex >= 0 && !a.mfix) a.mout[outIndex] = D;  // (0, 0, 0, count) as well
              }
              again = true;
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        enqueue(WF_SET_OF(WF_SET(WF_RING_READY) | WF_SET(WF_RING_NEWITEM)), toReady ? WF_RING_READY : (again ? WF_RING_NEWITEM : -1), id);
        const unsigned long long mR = __ballot(retired);
        if (mR != 0 && lane == __ffsll((long long)mR) - 1) __hip_atomic_fetch_sub(&ctl[WF_CTL_LIVE], __popcll(mR), __ATOMIC_RELAXED, WF_WG);
        prof(9, k);
      }
      return k;
  };
  auto flushProfile = [&]() {
  if (PROFILE && a.stats && lane == 0) {
      for (int k = 0; k < WF_PROF_KINDS; ++k) {
        atomicAdd(&a.stats[32 + k], pCyc[k]);
        atomicAdd(&a.stats[32 + WF_PROF_KINDS + k], pRuns[k]);
        atomicAdd(&a.stats[32 + 2 * WF_PROF_KINDS + k], pLanes[k]);
      }
      atomicAdd(&a.stats[32 + 3 * WF_PROF_KINDS], pSched);
      atomicAdd(&a.stats[32 + 3 * WF_PROF_KINDS + 1], (unsigned long long)(clock64() - pStart));
      for (int k = 0; k < 8; ++k) atomicAdd(&a.stats[32 + 3 * WF_PROF_KINDS + 2 + k], pSaw[k]);
    }
  };
  bool traverseFirst = false;  // the last decision was "go on traversing": one step before the rings are looked at again
  for (;;) {
    // ---- traverse for as long as the rings need no look: a tight loop of node bursts and primitive steps.  The rings are
    // looked at (below) when this wave has lanes to refill, nothing to traverse, or every fourth pass: with sixteen waves
    // deciding, a full batch is still seen within a fraction of the time it took to fill.  EVERY traversal step runs in
    // this loop (a decision that picks one comes back here with traverseFirst set): a second place to run them made the
    // compiler copy the lanes' whole state, forty registers, on its way back to the loop header.
    int nN, nP, free, nNknown = -1;  // (a step that ends with a count of the lanes at nodes hands it to the next pass)
    for (;;) {
      nN = nNknown >= 0 ? nNknown : __popcll(__ballot(atNode()));
      nP = __popcll(__ballot(atPrim()));
      free = 64 - nN - nP;  // lanes whose walk is over or that hold no context (cur == DONE either way)
      if (nN + nP == 0) break;
      if (!traverseFirst && (free >= a.wfSwapMin || (++tick & 3u) == 0)) break;
      traverseFirst = false;
      if (PROFILE) {
        const unsigned long long now = clock64();
        pSched += now - pT;
        pT = now;
      }
      if (nP >= a.primMin || nN == 0) {
        const int nNodes = primStep();
        nNknown = nNodes >= a.fuseMin ? nodeBurst(nNodes) : nNodes;
      } else {
        nNknown = nodeBurst(nN);
      }
    }
    // ---- scheduling decision with the rings in view
    const int nF = __popcll(__ballot(cur == DONE && path >= 0));
    int pick, serveAtLeast = 64, bestRing = WF_RING_RESTART;
    {
      unsigned long long* cw = reinterpret_cast<unsigned long long*>(ctl + 16);
      // relaxed 64-bit atomic loads: fresh values every time, two words per LDS read, broadcast to the wave
      const unsigned long long w0 = __hip_atomic_load(cw + 0, __ATOMIC_RELAXED, WF_WG), w1 = __hip_atomic_load(cw + 1, __ATOMIC_RELAXED, WF_WG),
                               w2 = __hip_atomic_load(cw + 2, __ATOMIC_RELAXED, WF_WG), w3 = __hip_atomic_load(cw + 3, __ATOMIC_RELAXED, WF_WG),
                               w4 = __hip_atomic_load(cw + 4, __ATOMIC_RELAXED, WF_WG), w5 = __hip_atomic_load(cw + 5, __ATOMIC_RELAXED, WF_WG),
                               w6 = __hip_atomic_load(cw + 6, __ATOMIC_RELAXED, WF_WG);
      // words 16 + 2r / 17 + 2r tail / head of ring r, 28 live, 29 abort
      if ((int)(w6 >> 32) != 0) break;  // abort
      auto fill = [](unsigned long long th) { return (int)((uint32_t)th - (uint32_t)(th >> 32)); };
      const int readyAvail = __builtin_amdgcn_readfirstlane(fill(w0));
      const int av[5] = {fill(w1), fill(w2), fill(w3), fill(w4), fill(w5)};  // RESTART, HIT 0..2, NEWITEM
      int bestAvail = av[0];
#pragma unroll
      for (int r = 1; r < 5; ++r)
        if (av[r] > bestAvail) {
          bestAvail = av[r];
          bestRing = WF_RING_RESTART + r;
        }
      bestRing = __builtin_amdgcn_readfirstlane(bestRing);
      bestAvail = __builtin_amdgcn_readfirstlane(bestAvail);
      // what a swap would move: finished walks out, READY contexts into the lanes without one
      const int swapGain = nF + (readyAvail < free ? readyAvail : free);
      if (bestAvail >= 64)
        pick = W_SERVE;  // a full batch is always worth a step (and feeds READY)
      else if (swapGain >= a.wfSwapMin)
        pick = W_SWAP;
      else if (nP >= a.primMin || (nN == 0 && nP > 0))
        pick = W_PRIM;
      else if (nN > 0)
        pick = W_NODE;
      else if (swapGain > 0)
        pick = W_SWAP;
      else if (bestAvail > 0) {
        pick = W_SERVE;  // nothing to traverse here and nothing READY: serve what there is
        serveAtLeast = 1;
      } else {
        if (__builtin_amdgcn_readfirstlane((int)w6) <= 0) break;  // every context has retired
        if (++idleTrips > WF_SPIN_LIMIT) {
          raiseAbort();
          break;
        }
        __builtin_amdgcn_s_sleep(8);
        prof(7, 0);
        continue;
      }
      idleTrips = 0;
      if (PROFILE) {
        pSaw[0]++;
        (void)readyAvail;
      }
    }
    if (PROFILE) {
      const unsigned long long now = clock64();
      pSched += now - pT;
      pT = now;
    }

    if (pick == W_PRIM || pick == W_NODE) {
      traverseFirst = true;  // (the loop above picks the step by the same rule)
    } else if (pick == W_SWAP) {
      swapStep();
    } else if (pick == W_SERVE) {
      serveStep(bestRing, serveAtLeast);
    }
  }
  flushProfile();
  if constexpr (COUNT) {  // (every lane of the wave is here: the loop above is left by wave-uniform decisions only)
    if (a.stats) {
      for (int k = 0; k < 8; ++k) {
        unsigned long long x = cnt[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        if (lane == 0) atomicAdd(&a.stats[k], x);
      }
    }
  }
}

extern "C" {
// the srt_render_wf_kernel instance a plan of form 3 or 4 names (srt_plan.cpp planRender)
RenderKernel srt_render_wf_kernel_for(const RenderPlan* p) {
  static_assert(WF_BLOCK == SRT_BLOCK_TREE, "srt_render.cpp launches the path-pool kernel with SRT_BLOCK_TREE threads");
  if (p->moments) {  // (never counting or profiling: srtRenderTilesMoments refuses countStats and ignores wf_profile)
    if (p->form == SRT_FORM_PATH_POOL_HYBRID) return p->single ? srt_render_wf_kernel<true, false, true, false, true> : srt_render_wf_kernel<false, false, true, false, true>;
    return p->single ? srt_render_wf_kernel<true, false, false, false, true> : srt_render_wf_kernel<false, false, false, false, true>;
  }
  if (p->form == SRT_FORM_PATH_POOL_HYBRID)
    return p->count     ? (p->single ? srt_render_wf_kernel<true, false, true, true> : srt_render_wf_kernel<false, false, true, true>)
           : p->profile ? srt_render_wf_kernel<false, true, true, false>
                        : (p->single ? srt_render_wf_kernel<true, false, true, false> : srt_render_wf_kernel<false, false, true, false>);
  return p->count     ? (p->single ? srt_render_wf_kernel<true, false, false, true> : srt_render_wf_kernel<false, false, false, true>)
         : p->profile ? srt_render_wf_kernel<false, true, false, false>
                      : (p->single ? srt_render_wf_kernel<true, false, false, false> : srt_render_wf_kernel<false, false, false, false>);
}
}
