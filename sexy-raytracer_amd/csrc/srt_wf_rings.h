// srt_wf_rings.h -- the rings of the path-pool kernel (srt_wavefront.hip): ONE statement of where a counter value lies in a
// ring, of the places a wave reserves, and of the two ring operations built on them, for the kernel and for a host program
// (examples/wf_rings_probe.cpp, tests/test_wf_rings.py).  The protocol and the LDS layout are the kernel's (its header
// comment): control words 16 + 2r / 17 + 2r are ring r's tail (places reserved) and head (places claimed), a slot is
// 16 bits and holds id + 1, 0 = empty.
//
// A wave that enqueues reserves, per ring, as many places as it has lanes for that ring with ONE atomic on the tail; its
// entries take these places in LANE ORDER.  With m_r the wave's lanes for ring r (a ballot, a scalar) and b_r what the
// atomic returned, lane l's place is b_r + popcount(m_r & below(l)): v_mbcnt on the device, with b_r as its addend.
// A call site names the rings it can produce as a compile-time SET; only those get a ballot, an atomic and a readlane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srt_device.h"

#define WF_CLASSES 3
#define WF_RING_READY 0
#define WF_RING_RESTART 1
#define WF_RING_HIT 2                   // + material class
#define WF_RING_NEWITEM (2 + WF_CLASSES)
#define WF_RINGS (3 + WF_CLASSES)
#define WF_SPIN_LIMIT (1 << 24)
#define WF_CTL_TAIL(r) (16 + 2 * (r))
#define WF_CTL_HEAD(r) (17 + 2 * (r))
#define WF_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define WF_SET(r) (1u << (r))
#define WF_SET_ALL ((1u << WF_RINGS) - 1u)

typedef uint16_t SrtWfRingSlot;  // id + 1, 0 = empty

// capacity = (mul3 ? 3 : 1) << shift
struct SrtWfRingGeom {
  int32_t cap, shift, mul3;
};
// Every ring a launch can get, largest first: the planner (srt_plan.cpp planRender) takes the first that fits behind the
// tree and does not exceed the tunable wf_pool
constexpr SrtWfRingGeom kSrtWfRings[] = {{4096, 12, 0}, {3072, 10, 1}, {2048, 11, 0}, {1536, 9, 1}, {1024, 10, 0}};

// place of counter value c in a ring: c mod cap.  2^j: exact for every 32-bit c, the counter's wrap included.  3 * 2^j:
// c = x * 2^j + low, x mod 3 by a multiply-shift that is exact for every 32-bit x; the counter's wrap is NOT a multiple of
// the capacity, so planRender admits these rings only while a workgroup's enqueues stay below 2 * 10^9.
SRT_HD inline uint32_t srtWfRingPos(uint32_t c, SrtWfRingGeom g) {
  if (!g.mul3) return c & (uint32_t)(g.cap - 1);
  const uint32_t x = c >> g.shift;
  const uint32_t x3 = x - 3u * (uint32_t)(((unsigned long long)x * 0xAAAAAAABull) >> 33);
  return (c & ((1u << g.shift) - 1u)) | (x3 << g.shift);
}

// ---- the reservation: how many places a wave takes in a ring, and which of them is lane l's
SRT_HD inline int srtWfReserveCount(unsigned long long mask) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(mask);
#else
  return __builtin_popcountll(mask);
#endif
}
// `lane`: the executing lane on the device (v_mbcnt counts below it by itself)
SRT_HD inline uint32_t srtWfReservePlace(uint32_t base, unsigned long long mask, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)lane;
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, base));
#else
  return base + (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
#endif
}

#if defined(__HIPCC__)
// v with lane R's value replaced by the wave-uniform c: one v_writelane_b32 (the compiler has no builtin for it; the
// instruction takes one scalar register, so the lane select is a literal)
template <int R>
__device__ __forceinline__ int srtWfWriteLane(int v, int c) {
  static_assert(WF_RINGS == 6 && R >= 0 && R < WF_RINGS, "one lane per ring");
  asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(c), "n"(R));
  return v;
}

// ---- enqueue: lane `lane` of the wave hands context `id` to ring `ring` -- a ring of SET, or < 0: nothing.  All lanes of the
// wave call it together.  One ballot per ring of the set, kept as a scalar mask; the counts go to lanes r of one register and
// the tails' atomics are issued side by side by those lanes: one LDS round trip whatever the set; the bases come back by
// readlane.  What the caller wrote for the context BEFORE (global stores: the caller fences; LDS: one wave's LDS operations
// execute in order) is visible to the consumer that finds the id.  `abort()`: the bounded spin ran out.
template <uint32_t SET, class Abort>
__device__ __forceinline__ void srtWfEnqueue(int32_t* ctl, uint16_t* ringSlots, SrtWfRingGeom g, int lane, int ring, int id, Abort&& abort) {
  static_assert(SET != 0 && (SET & ~WF_SET_ALL) == 0, "a set of rings");
  unsigned long long m[WF_RINGS];
  int n = 0;  // lane r: how many lanes of this wave enqueue to ring r
#pragma unroll
  for (int r = 0; r < WF_RINGS; ++r)
    if (SET >> r & 1u) {
      m[r] = __ballot(ring == r);
      const int c = srtWfReserveCount(m[r]);
      switch (r) {  // (r is a constant once the loop is unrolled; the lane select has to be a literal)
        case 0: n = srtWfWriteLane<0>(n, c); break;
        case 1: n = srtWfWriteLane<1>(n, c); break;
        case 2: n = srtWfWriteLane<2>(n, c); break;
        case 3: n = srtWfWriteLane<3>(n, c); break;
        case 4: n = srtWfWriteLane<4>(n, c); break;
        default: n = srtWfWriteLane<5>(n, c); break;
      }
    }
  int base = 0;
  if (n > 0) base = __hip_atomic_fetch_add(&ctl[WF_CTL_TAIL(lane)], n, __ATOMIC_RELAXED, WF_WG);
  uint32_t place = 0;
#pragma unroll
  for (int r = 0; r < WF_RINGS; ++r)
    if (SET >> r & 1u) {
      const uint32_t p = srtWfReservePlace((uint32_t)__builtin_amdgcn_readlane(base, r), m[r], lane);
      place = ring == r ? p : place;
    }
  if (ring >= 0) {
    // (the capacity's modulo once, on the lane's own place; ring * cap < 2^24)
    uint16_t* const s = ringSlots + (__umul24((uint32_t)ring, (uint32_t)g.cap) + srtWfRingPos(place, g));
    // (first look outside the loop: a loop header makes the compiler wait for every load the caller has in flight)
    if (__hip_atomic_load(s, __ATOMIC_RELAXED, WF_WG) != 0) {
      int spins = 0;
      while (__hip_atomic_load(s, __ATOMIC_RELAXED, WF_WG) != 0) {
        if (++spins > WF_SPIN_LIMIT) {
          abort();
          break;
        }
      }
    }
    __hip_atomic_store(s, (uint16_t)(id + 1), __ATOMIC_RELAXED, WF_WG);
  }
}

// ---- claim, in two halves shared by its forms.  srtWfClaimPlaces: lane 0 moves ring r's head by up to `want` places (by
// none unless at least `atLeast` are there); returns how many, wave-uniform, and in `first` the counter value of the first.
__device__ __forceinline__ int srtWfClaimPlaces(int32_t* ctl, int lane, int r, int want, int atLeast, uint32_t& first) {
  int h = 0, k = 0;
  if (lane == 0) {
    const unsigned long long th = __hip_atomic_load(reinterpret_cast<unsigned long long*>(&ctl[WF_CTL_TAIL(r)]), __ATOMIC_RELAXED, WF_WG);
    int t = (int)th;
    h = (int)(th >> 32);
    // first attempt outside the loop (as in enqueue: no loop header on the common path)
    bool again = false;
    {
      const int avail = (int)((uint32_t)t - (uint32_t)h);
      k = avail < want ? avail : want;
      if (k < atLeast || k <= 0) {
        k = 0;
      } else {
        int expected = h;
        if (!__hip_atomic_compare_exchange_strong(&ctl[WF_CTL_HEAD(r)], &expected, h + k, __ATOMIC_RELAXED, __ATOMIC_RELAXED, WF_WG)) {
          h = expected;  // another wave claimed meanwhile: the tail can only have grown
          again = true;
        }
      }
    }
    while (again) {
      t = __hip_atomic_load(&ctl[WF_CTL_TAIL(r)], __ATOMIC_RELAXED, WF_WG);
      const int avail = (int)((uint32_t)t - (uint32_t)h);
      k = avail < want ? avail : want;
      if (k < atLeast || k <= 0) {
        k = 0;
        break;
      }
      int expected = h;
      if (__hip_atomic_compare_exchange_strong(&ctl[WF_CTL_HEAD(r)], &expected, h + k, __ATOMIC_RELAXED, __ATOMIC_RELAXED, WF_WG)) break;
      h = expected;
    }
  }
  first = (uint32_t)__builtin_amdgcn_readfirstlane(h);
  return __builtin_amdgcn_readfirstlane(k);
}
// srtWfTake: the lanes with `take` empty the slot of counter value `place` of ring r, waiting the few cycles a reserved
// place may still be unwritten; returns the id it held (-1 for the other lanes).
template <class Abort>
__device__ __forceinline__ int srtWfTake(uint16_t* ringSlots, SrtWfRingGeom g, int r, bool take, uint32_t place, Abort&& abort) {
  int id = -1;
  if (take) {
    uint16_t* const s = ringSlots + (r * g.cap + srtWfRingPos(place, g));
    int v = __hip_atomic_load(s, __ATOMIC_RELAXED, WF_WG);
    if (v == 0) {
      int spins = 0;
      while ((v = __hip_atomic_load(s, __ATOMIC_RELAXED, WF_WG)) == 0) {
        if (++spins > WF_SPIN_LIMIT) {
          abort();
          break;
        }
      }
    }
    __hip_atomic_store(s, (uint16_t)0, __ATOMIC_RELAXED, WF_WG);
    id = v - 1;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return id;
}

// ---- claim for the lanes with `mine`, in lane order (`takers`: their ballot): returns how many entries the wave got, and
// in `id` the lane's (-1: none).  Wave-uniform call.
template <class Abort>
__device__ __forceinline__ int srtWfClaim(int32_t* ctl, uint16_t* ringSlots, SrtWfRingGeom g, int lane, int r, bool mine, unsigned long long takers,
                                          int want, int atLeast, int& id, Abort&& abort) {
  uint32_t first;
  const int k = srtWfClaimPlaces(ctl, lane, r, want, atLeast, first);
  const uint32_t place = srtWfReservePlace(first, takers, lane);
  id = srtWfTake(ringSlots, g, r, mine && (int)(place - first) < k, place, abort);
  return k;
}
// ---- claim for every lane of the wave (a serve step): a lane's rank is its number
template <class Abort>
__device__ __forceinline__ int srtWfClaimAll(int32_t* ctl, uint16_t* ringSlots, SrtWfRingGeom g, int lane, int r, int want, int atLeast, int& id,
                                             Abort&& abort) {
  uint32_t first;
  const int k = srtWfClaimPlaces(ctl, lane, r, want, atLeast, first);
  id = srtWfTake(ringSlots, g, r, lane < k, first + (uint32_t)lane, abort);
  return k;
}

// ---- the generic forms: a loop over every ring, the lane's own ballot as a 64-bit `mine`, ranks from `laneBelow`
// ((1 << lane) - 1, kept by the caller).  The same places and ids as the forms above (tests/test_wf_rings.py replays the arithmetic of both on the
// host; tests/test_gpu_wf_handover.py runs both on the device).
// The hybrid instances of the kernel keep these: their walks wait for memory, the vector ALU is not what bounds them, and
// the specialised forms measured 0.8 - 1.2 % SLOWER there, each of the two by itself (profiles/r20/ab_parts_*.txt,
// ab_hybrid_split_*.txt).
template <class Abort>
__device__ __forceinline__ void srtWfEnqueueGeneric(int32_t* ctl, uint16_t* ringSlots, SrtWfRingGeom g, int lane, unsigned long long laneBelow, int ring,
                                                    int id, Abort&& abort) {
  int n = 0;  // lane r < WF_RINGS: how many lanes of this wave enqueue to ring r
#pragma unroll
  for (int r = 0; r < WF_RINGS; ++r) {
    const int c = __popcll(__ballot(ring == r));
    n = lane == r ? c : n;
  }
  int base = 0;
  if (lane < WF_RINGS && n > 0) base = __hip_atomic_fetch_add(&ctl[WF_CTL_TAIL(lane)], n, __ATOMIC_RELAXED, WF_WG);
  int myBase = 0;
  unsigned long long mine = 0;
#pragma unroll
  for (int r = 0; r < WF_RINGS; ++r) {
    const int b = __builtin_amdgcn_readlane(base, r);
    const unsigned long long m = __ballot(ring == r);
    if (ring == r) {
      myBase = b;
      mine = m;
    }
  }
  if (ring >= 0) {
    uint16_t* const s = ringSlots + ring * g.cap + (int)srtWfRingPos((uint32_t)(myBase + __popcll(mine & laneBelow)), g);
    if (__hip_atomic_load(s, __ATOMIC_RELAXED, WF_WG) != 0) {
      int spins = 0;
      while (__hip_atomic_load(s, __ATOMIC_RELAXED, WF_WG) != 0) {
        if (++spins > WF_SPIN_LIMIT) {
          abort();
          break;
        }
      }
    }
    __hip_atomic_store(s, (uint16_t)(id + 1), __ATOMIC_RELAXED, WF_WG);
  }
}
// claim for the lanes of `takers` (every lane: ~0), membership and rank from `takers` and `laneBelow` alone
template <class Abort>
__device__ __forceinline__ int srtWfClaimGeneric(int32_t* ctl, uint16_t* ringSlots, SrtWfRingGeom g, int lane, unsigned long long laneBelow, int r,
                                                 unsigned long long takers, int want, int atLeast, int& id, Abort&& abort) {
  uint32_t first;
  const int k = srtWfClaimPlaces(ctl, lane, r, want, atLeast, first);
  const int rank = __popcll(takers & laneBelow);
  id = srtWfTake(ringSlots, g, r, ((takers >> lane) & 1ull) && rank < k, first + (uint32_t)rank, abort);
  return k;
}
#endif  // __HIPCC__
