// srt_paths.hip -- whole paths for the rays of a device buffer in ONE kernel (srtTracePathsDevice; include/srt_hip.h "Path
// steps on device buffers"): a lane carries a path from its first ray to its end, keeps the attenuations of its
// scattered steps on a per-lane LDS stack, unwinds them in the reference's order, writes the radiance and takes the next
// entry from a counter.  Nothing passes through memory between bounces and nothing is read back by the host.
//
// Persistent, 256 threads, and no wave ever waits for another wave or workgroup: no spin, no flag, no barrier.  The one
// thing waves share is the 64-bit counter of the next unclaimed entry (the first word of the caller's scratch, zeroed on
// the stream ahead of the launch).  At the top of a trip the idle lanes of a wave claim entries together, once there are
// refillMin of them (a quarter of the wave as shipped): one relaxed agent-scope atomic add of their number
// by one lane, the base broadcast, base + the lane's rank among the idle lanes (srt_compact.hip's ballot / mbcnt idiom)
// as the lane's entry.  The lanes of a claim hold consecutive entries, so the ray loads of a fresh wave coalesce as the
// step kernel's do.  The kernel ends because the counter only grows and every path makes at most maxBounce steps.
//
// One trip is srt_pathstep.hip's step on the lane's registers.  Shared with it, each written once: the walk
// (srt_query_walk.h queryWalk), the records (srt_path.h sphereRecord, triRecord), shade() and its instance, and the ray
// row's loads (srt_step_rays.h STEP_WIDE, loadRay).  Written out here as in srt_path_step_kernel: the branch from the
// walk's hit reference to one of the two records, without the step kernel's load of the prims[] index, and the
// material-range check behind it (one function for the two moved this kernel's registers, so each keeps its lines).  The
// kernel's own: the claim of entries, the attenuation stack and its unwinding, and the one store of the radiance where
// the step kernel stores an SrtPathOut per bounce.  LDS per workgroup: the walk's [slot][thread] stack (stackDepth + 2
// slots), then the attenuations [3 * level + channel][thread], 3 * maxBounce slots of the call's own maxBounce
// (srt_lds_layout.h srtPathsLdsBytes).  DESIGN.md 5.20.  The DIRECT instances (srtTracePathsDirectDevice) add srt_direct.h's
// direct-light term at every pbr hit and keep it beside the attenuation: 6 * maxBounce slots (srtPathsDirectLdsBytes).
// DESIGN.md 5.23.

#include <algorithm>
#include <type_traits>

#include "srt_path.h"
#include "srt_query_walk.h"
#include "srt_step_rays.h"
#include "srt_direct.h"
#include "srt_lds_layout.h"
#include "srt_launch.h"

namespace {

constexpr int WAVE = 64;

// SrtPathRadiance: one dwordx4 store; steps in the low half of the last dword, the status in its high half
__device__ __forceinline__ void storeRadiance(int4* out, V3 L, int steps, int status) {
  *out = make_int4(__float_as_int(L.x), __float_as_int(L.y), __float_as_int(L.z), (int)(((uint32_t)status << 16) | ((uint32_t)steps & 0xffffu)));
}

__device__ __forceinline__ const TracePathsArgs& plainArgs(const TracePathsArgs& a) { return a; }
__device__ __forceinline__ const TracePathsArgs& plainArgs(const TracePathsDirectArgs& a) { return a.p; }

// MODE: Q_FAITHFUL or Q_CLOSEST.  DIRECT (srtTracePathsDirectDevice): at a pbr hit the direct term of srt_direct.h is
// evaluated ahead of shade() from the generator's state as it is there, which it does not advance, and kept beside the
// step's attenuation -- six LDS slots per level instead of three (srt_lds_layout.h srtPathsDirectLdsBytes); a bounced
// ray that ends on a light the step before could have chosen drops that light's emission; the unwinding adds each level's
// term.  Claim, walk, records, shade() and the stores are the plain instance's lines.
template <int MODE, bool DIRECT = false>
__global__ __launch_bounds__(SRT_BLOCK) void srt_paths_kernel(const std::conditional_t<DIRECT, TracePathsDirectArgs, TracePathsArgs> args) {
  extern __shared__ int32_t lds[];
  const TracePathsArgs& a = plainArgs(args);
  constexpr int SLOTS = DIRECT ? 6 : 3;  // per level: the attenuation, and with DIRECT the direct term
  const DevScene& sc = a.scene;
  const QueryWalk walk = queryWalkSetup<MODE>(sc, lds);  // [slot][thread]: stackDepth + 2 slots
  float* const attStack = reinterpret_cast<float*>(lds) + srtQueryStackBytes(sc.stackDepth) / sizeof(int32_t) + threadIdx.x;
  const Rsrc rsTexels = makeRsrc(sc.texels, sc.texelBytes);
  const V3 zero = mk(0.0f, 0.0f, 0.0f), background = mk(a.background[0], a.background[1], a.background[2]);
  const int lane = threadIdx.x & (WAVE - 1);
  // the lane's path: its entry, the ray of its next step, the generator, the scattered steps so far
  int64_t i = 0;
  Ray r;
  r.o = r.d = zero;
  r.time = 0.0f;
  float tMin = 0.0f, tMax = 0.0f;
  Pcg rng;
  rng.state = 0;
  int depth = 0;
  bool have = false;
  bool sampledBefore = false;  // DIRECT: the step before evaluated a direct term
  bool dry = false;  // the counter has passed n: nothing is left to claim (the same in every lane of the wave)
  while (true) {
    // ---- refill: every lane of the wave is here, whatever it did in the trip before
    const unsigned long long idle = __ballot(!have);
    const int numIdle = __popcll(idle);
    if (!dry && numIdle >= a.refillMin) {  // refillMin <= 64: a wave that is idle altogether always claims
      unsigned long long base = 0;
      if (lane == 0) base = __hip_atomic_fetch_add(a.counter, (unsigned long long)numIdle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint64_t first = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) |
                             (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)base);
      dry = first + (uint64_t)numIdle >= (uint64_t)a.n;
      const int64_t mine = (int64_t)first + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
      if (!have && mine < a.n) {  // a lane whose index lies behind the last entry stays idle for good
        i = mine;
        loadRay(a.rays + 9 * i, r, tMin, tMax);
        rng.state = a.rng[i];
        depth = 0;
        sampledBefore = false;
        have = a.maxBounce > 0;
        if (!have) storeRadiance(a.result + i, zero, 0, SRT_PATH_SCATTERED);  // no step runs: black, the state as it was
      }
    }
    if (__ballot(have) == 0) {
      if (dry) break;
      continue;
    }
    // ---- one step of every lane that has a path: srt_path_step_kernel's body
    if (have) {
      float closest;
      bool found;
      const int hitRef = queryWalk<MODE>(sc, walk, r, tMin, tMax, closest, found);
      V3 L = background;  // the terminal radiance, should the path end here
      int status = SRT_PATH_MISS;
      bool goOn = false;
      if (hitRef != SRT_REF_DONE) {
        Record rec;
        const int pr = ~hitRef;
        if (pr & 1)
          sphereRecord(sc, pr >> 1, r, closest, rec, false);
        else
          triRecord(sc, pr >> 1, r, closest, rec, false);
        L = zero;
        status = SRT_PATH_INVALID;
        if (!(rec.material >= sc.numMaterials)) {
          V3 att = zero, emitted;
          Ray next;
          next.d = zero;
          uint32_t fetches = 0;
          V3 direct = zero;
          bool sampled = false;
          if constexpr (DIRECT) {
            if (args.numLights > 0 && (rec.matType & 3) == SRT_MAT_PBR) {
              direct = directTerm<MODE, STEP_WIDE>(sc, walk, rsTexels, args.lights, args.numLights, r, tMin, tMax, rec, rng.state).radiance;
              sampled = true;
            }
          }
          if (shade<false, STEP_WIDE>(sc, rsTexels, r, rec, rng, att, next, emitted, fetches)) {
            attStack[(SLOTS * depth + 0) * SRT_BLOCK] = att.x;  // depth < maxBounce: a path at the limit has ended
            attStack[(SLOTS * depth + 1) * SRT_BLOCK] = att.y;
            attStack[(SLOTS * depth + 2) * SRT_BLOCK] = att.z;
            if constexpr (DIRECT) {
              attStack[(SLOTS * depth + 3) * SRT_BLOCK] = direct.x;
              attStack[(SLOTS * depth + 4) * SRT_BLOCK] = direct.y;
              attStack[(SLOTS * depth + 5) * SRT_BLOCK] = direct.z;
            }
            r = next;
            depth++;
            status = SRT_PATH_SCATTERED;
            goOn = depth < a.maxBounce;  // out of bounces: black, through every attenuation (main.cpp:36-37)
          } else {
            status = SRT_PATH_ENDED;
            L = emitted;
            if constexpr (DIRECT) {  // the drop rule: the step before could have chosen this light, whatever it chose
              if (sampledBefore && (pr & 1) && directCouldChoose(sc, pr >> 1, r.o)) L = zero;
            }
          }
          sampledBefore = sampled;
        }
      }
      if (!goOn) {
        const int steps = depth + (status != SRT_PATH_SCATTERED ? 1 : 0);
        // unwind the recursion: emitted + newColor * attenuation with emitted = 0, innermost first (main.cpp:49-51)
        for (int j = depth - 1; j >= 0; --j) {
          const float ax = attStack[(SLOTS * j + 0) * SRT_BLOCK], ay = attStack[(SLOTS * j + 1) * SRT_BLOCK], az = attStack[(SLOTS * j + 2) * SRT_BLOCK];
          V3 D = zero;  // the plain instance's 0.0f
          if constexpr (DIRECT) D = mk(attStack[(SLOTS * j + 3) * SRT_BLOCK], attStack[(SLOTS * j + 4) * SRT_BLOCK], attStack[(SLOTS * j + 5) * SRT_BLOCK]);
          L = mk(D.x + L.x * ax, D.y + L.y * ay, D.z + L.z * az);
        }
        storeRadiance(a.result + i, L, steps, status);
        a.rng[i] = rng.state;  // one 8-byte store: the state after the path's last draw
        have = false;
      }
    }
  }
}

// the memset of the counter and the launch of one instance; p: the plain arguments inside a
template <typename Args>
int launchPaths(void (*kernel)(const Args), const Args& a, const TracePathsArgs& p, int numCUs, size_t ldsBytes, size_t scratchBytes, hipStream_t stream) {
  if (ldsBytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
    if (e != hipSuccess) return (int)e;
  }
  // the workgroups that are resident at once: more would only queue behind them and find the counter run out
  int perCU = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, SRT_BLOCK, ldsBytes) != hipSuccess || perCU < 1) perCU = 1;
  const int grid = (int)std::min<int64_t>((p.n + SRT_BLOCK - 1) / SRT_BLOCK, (int64_t)numCUs * perCU);
  const hipError_t e = hipMemsetAsync(p.counter, 0, scratchBytes, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SRT_BLOCK), ldsBytes, stream, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// traversal: SRT_TRAVERSE_FAITHFUL or SRT_TRAVERSE_CLOSEST; ldsBytes: srtPathsLdsBytes; scratchBytes: what the memset
// clears from a->counter on
int srt_launch_paths(const TracePathsArgs* a, int traversal, int numCUs, size_t ldsBytes, size_t scratchBytes, hipStream_t stream) {
  void (*kernel)(const TracePathsArgs) = traversal == SRT_TRAVERSE_CLOSEST ? srt_paths_kernel<Q_CLOSEST> : srt_paths_kernel<Q_FAITHFUL>;
  return launchPaths(kernel, *a, *a, numCUs, ldsBytes, scratchBytes, stream);
}

// the DIRECT instances; ldsBytes: srtPathsDirectLdsBytes
int srt_launch_paths_direct(const TracePathsDirectArgs* a, int traversal, int numCUs, size_t ldsBytes, size_t scratchBytes, hipStream_t stream) {
  void (*kernel)(const TracePathsDirectArgs) = traversal == SRT_TRAVERSE_CLOSEST ? srt_paths_kernel<Q_CLOSEST, true> : srt_paths_kernel<Q_FAITHFUL, true>;
  return launchPaths(kernel, *a, a->p, numCUs, ldsBytes, scratchBytes, stream);
}

}  // extern "C"
