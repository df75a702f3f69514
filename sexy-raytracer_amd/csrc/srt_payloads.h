// srt_payloads.h -- what the kernels over a PathPayloads (srt_launch.h) share: which entries go on, and how a kept entry
// moves to its rank.  Included by srt_compact.hip (count and scatter) and srt_sort.hip (key and gather).  Internal.
#ifndef SRT_PAYLOADS_H
#define SRT_PAYLOADS_H

#include "srt_launch.h"

namespace {

// keep[i] for i < p.n (the caller's bound), with both predicates optional.  Of SrtPathOut only the status dword is read.
__device__ __forceinline__ bool keepEntry(const PathPayloads& p, int64_t i) {
  if (p.active && p.active[i] == 0) return false;
  return !p.out || p.out[8 * i + 3] == SRT_PATH_SCATTERED;
}

// Entry i to rank `rank` of every payload asked for: the 36-byte ray row through registers, as the step kernels' loadRay /
// storeRay move it (nine dword loads, nine dword stores: lanes with consecutive ranks write consecutive rows), the
// generator state, and the slot -- the identity where no slots came in.
__device__ __forceinline__ void moveEntry(const PathPayloads& p, int64_t i, int64_t rank) {
  if (p.raysOut) {
    const uint32_t* in = p.rays + 9 * i;
    uint32_t* out = p.raysOut + 9 * rank;
    uint32_t row[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) row[c] = in[c];
#pragma unroll
    for (int c = 0; c < 9; ++c) out[c] = row[c];
  }
  if (p.rngOut) p.rngOut[rank] = p.rng[i];
  if (p.slotOut) p.slotOut[rank] = p.slot ? p.slot[i] : (int32_t)i;
}

}  // namespace

#endif
