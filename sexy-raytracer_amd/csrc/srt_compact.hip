// srt_compact.hip -- stable compaction of the live paths between two path steps (srtCompactPathsDevice; include/srt_hip.h
// "Path steps on device buffers"): the entries that scattered move, in their order, to the front of fresh ray, state and
// slot buffers, so that the next step runs on full waves.
//
// Three launches on the caller's stream, and no workgroup ever waits for another one:
//   count    per tile of SRT_COMPACT_TILE entries, the number kept -> tileOffset[tile]
//   scan     ONE workgroup: the exclusive scan of those counts in place (a 64-bit carry across its trips), the total ->
//            *count
//   scatter  per tile, the predicate again; a kept entry's rank is its tile's offset + the kept entries of the (row, wave)
//            units before its own in the tile + the kept lanes below it in its wave
// A tile is ROWS rows of SRT_BLOCK consecutive entries; lane t of the workgroup takes entry t of every row, so that the
// loads of a wave are consecutive and the units of a tile are ordered (row, wave).  The predicate is evaluated twice
// rather than left in scratch as ballots.  The predicate and the move of a kept entry are srt_payloads.h's
// keepEntry and moveEntry: the kept lanes of a wave write consecutive rows.

#include "srt_launch.h"
#include "srt_payloads.h"

namespace {

constexpr int WAVE = 64;
constexpr int ROWS = SRT_COMPACT_TILE / SRT_BLOCK;
constexpr int WAVES = SRT_BLOCK / WAVE;
static_assert(SRT_COMPACT_TILE % SRT_BLOCK == 0 && (SRT_COMPACT_TILE & (SRT_COMPACT_TILE - 1)) == 0, "a tile is whole rows, a power of two");
static_assert(SRT_COMPACT_SCAN_BLOCK % WAVE == 0 && SRT_COMPACT_SCAN_BLOCK <= 1024, "the scan workgroup");

// keep[i]; false behind the last entry
__device__ __forceinline__ bool keepBounded(const PathPayloads& p, int64_t i) { return i < p.n && keepEntry(p, i); }

__global__ __launch_bounds__(SRT_BLOCK) void srt_compact_count_kernel(const CompactArgs a) {
  __shared__ uint32_t waveCount[WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  for (int64_t tile = blockIdx.x; tile < a.numTiles; tile += gridDim.x) {
    const int64_t first = tile * SRT_COMPACT_TILE + threadIdx.x;
    uint32_t kept = 0;  // of this wave, over the tile's rows
#pragma unroll
    for (int k = 0; k < ROWS; ++k) kept += (uint32_t)__popcll(__ballot(keepBounded(a.p, first + (int64_t)k * SRT_BLOCK)));
    if (lane == 0) waveCount[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t sum = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) sum += waveCount[w];
      a.tileOffset[tile] = sum;  // a 32-bit count in the 64-bit word the scan turns into an offset
    }
    __syncthreads();  // the next trip writes waveCount again
  }
}

__global__ __launch_bounds__(SRT_COMPACT_SCAN_BLOCK) void srt_compact_scan_kernel(uint64_t* tileOffset, int64_t numTiles, int64_t* count) {
  constexpr int SCAN_WAVES = SRT_COMPACT_SCAN_BLOCK / WAVE;
  __shared__ uint32_t waveSum[SCAN_WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  uint64_t carry = 0;  // the tiles of the trips before this one; every thread keeps the same value
  for (int64_t first = 0; first < numTiles; first += SRT_COMPACT_SCAN_BLOCK) {
    const int64_t t = first + threadIdx.x;
    const uint32_t own = t < numTiles ? (uint32_t)tileOffset[t] : 0u;
    uint32_t incl = own;  // a trip sums at most SCAN_BLOCK * TILE = 2^20: 32 bits
#pragma unroll
    for (int d = 1; d < WAVE; d *= 2) {
      const uint32_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == WAVE - 1) waveSum[wave] = incl;
    __syncthreads();
    uint32_t below = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) {
      const uint32_t s = waveSum[w];
      below += w < wave ? s : 0u;
      all += s;
    }
    if (t < numTiles) tileOffset[t] = carry + below + (incl - own);
    carry += all;
    __syncthreads();  // the next trip writes waveSum again
  }
  if (threadIdx.x == 0) *count = (int64_t)carry;
}

__global__ __launch_bounds__(SRT_BLOCK) void srt_compact_scatter_kernel(const CompactArgs a) {
  __shared__ uint32_t unitCount[ROWS * WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int64_t total = *a.p.count;
  for (int64_t tile = blockIdx.x; tile < a.numTiles; tile += gridDim.x) {
    const int64_t first = tile * SRT_COMPACT_TILE + threadIdx.x;
    uint64_t ballot[ROWS];
    // every byte of the mask this lane will overwrite (activeOut may be the mask itself) is read here, before the stores
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
      ballot[k] = __ballot(keepBounded(a.p, first + (int64_t)k * SRT_BLOCK));
      if (lane == 0) unitCount[k * WAVES + wave] = (uint32_t)__popcll(ballot[k]);
    }
    __syncthreads();
    uint32_t before[ROWS], run = 0;  // the kept entries of the units before (row k, this wave)
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        if (w == wave) before[k] = run;
        run += unitCount[k * WAVES + w];
      }
    }
    const int64_t tileFirst = (int64_t)a.tileOffset[tile];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
      const int64_t i = first + (int64_t)k * SRT_BLOCK;
      if ((ballot[k] >> lane) & 1) {
        const uint32_t lo = (uint32_t)ballot[k], hi = (uint32_t)(ballot[k] >> 32);
        const int64_t rank = tileFirst + before[k] + __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
        moveEntry(a.p, i, rank);
      }
      if (a.p.activeOut && i < a.p.n) a.p.activeOut[i] = i < total ? 1 : 0;
    }
    __syncthreads();  // the next trip writes unitCount again
  }
}

}  // namespace

extern "C" {

int srt_launch_compact(const CompactArgs* a, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(srt_compact_count_kernel, dim3(grid), dim3(SRT_BLOCK), 0, stream, *a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(srt_compact_scan_kernel, dim3(1), dim3(SRT_COMPACT_SCAN_BLOCK), 0, stream, a->tileOffset, a->numTiles, a->p.count);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(srt_compact_scatter_kernel, dim3(grid), dim3(SRT_BLOCK), 0, stream, *a);
  return (int)hipGetLastError();
}

}  // extern "C"
