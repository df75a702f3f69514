// srt_sort.hip -- the live paths between two path steps, ordered by where they start and which way they point
// (srtSortPathsDevice; include/srt_hip.h "Path steps on device buffers"): srtCompactPathsDevice's kept entries, stably
// sorted by (Morton cell of the origin in the caller's box, octant of the direction), so that the lanes of a wave of the
// next step ask for neighbouring nodes of a tree that no longer sits in the caches.
//
// On the caller's stream, and no workgroup of these kernels ever waits for another one:
//   memset   *count = 0
//   key      one lane per entry: key[i] and index[i] = i into the scratch; a kept entry's key is cell << 3 | octant, a
//            dropped one's the one key above them all (its ray is not read).  The kept lanes of a wave are counted with a
//            ballot and added to *count by one lane, once per wave, when the wave has run out of entries: an integer sum,
//            so the order of the additions does not show.
//   sort     rocPRIM's radix_sort_pairs over (key, index) on bits [0, 3 * cellBits + 4), between the two halves of the
//            scratch's double buffers: stable, so equal keys stay in index order and the dropped entries end up behind
//            rank count in theirs.
//   gather   one lane per rank: rank r < count reads order[r] and moves that entry's 36-byte ray row, state and slot with
//            the moveEntry srt_compact.hip's scatter calls (srt_payloads.h) -- the stores of a wave consecutive rows; the
//            loads are scattered, which is what the call costs.  activeOut[r] = r < count: the mask was read by the
//            key kernel, a launch earlier on the stream, so activeOut may be the mask itself.

#include <rocprim/device/device_radix_sort.hpp>

#include "srt_launch.h"
#include "srt_payloads.h"

namespace {

constexpr int WAVE = 64;

// bit k of q -> bit 3k, for the low 10 bits
__device__ __forceinline__ uint32_t spread3(uint32_t q) {
  q = (q | (q << 16)) & 0x030000ffu;
  q = (q | (q << 8)) & 0x0300f00fu;
  q = (q | (q << 4)) & 0x030c30c3u;
  q = (q | (q << 2)) & 0x09249249u;
  return q;
}

// The cell of one coordinate: 0 unless c >= 0 (a NaN, a negative value), the last cell from there on (+inf too).  The
// subtraction and the multiplication are two operations: the library is built with -ffp-contract=off.
__device__ __forceinline__ uint32_t cellOf(float o, float lo, float scale, uint32_t last) {
  const float c = (o - lo) * scale;
  if (!(c >= 0.0f)) return 0u;
  return c >= (float)last ? last : (uint32_t)c;
}

__global__ __launch_bounds__(SRT_BLOCK) void srt_sort_key_kernel(const SortArgs a) {
  const PathPayloads& p = a.p;
  const int lane = threadIdx.x & (WAVE - 1);
  // the same for every lane of the wave, and outside the loop over its entries: six loads and three divisions per wave
  const float lo[3] = {a.box[0], a.box[1], a.box[2]};
  const float cells = (float)(1u << a.cellBits);
  const float scale[3] = {cells / (a.box[3] - lo[0]), cells / (a.box[4] - lo[1]), cells / (a.box[5] - lo[2])};
  const uint32_t last = (1u << a.cellBits) - 1u;
  const uint32_t dead = 1u << (3 * a.cellBits + 3);
  const int64_t stride = (int64_t)gridDim.x * SRT_BLOCK;
  uint32_t kept = 0;  // of this wave; every lane keeps the same value
  // a wave's trips are whole: lanes behind n wait in the ballot
  for (int64_t first = (int64_t)blockIdx.x * SRT_BLOCK + (threadIdx.x - lane); first < p.n; first += stride) {
    const int64_t i = first + lane;
    const bool keep = i < p.n && keepEntry(p, i);
    if (i < p.n) {
      uint32_t key = dead;
      if (keep) {
        const float* ray = reinterpret_cast<const float*>(p.rays + 9 * i);
        const uint32_t cell = spread3(cellOf(ray[0], lo[0], scale[0], last)) | spread3(cellOf(ray[1], lo[1], scale[1], last)) << 1 |
                              spread3(cellOf(ray[2], lo[2], scale[2], last)) << 2;
        const uint32_t octant = p.rays[9 * i + 3] >> 31 | (p.rays[9 * i + 4] >> 31) << 1 | (p.rays[9 * i + 5] >> 31) << 2;
        key = cell << 3 | octant;
      }
      a.keys[i] = key;
      a.index[i] = (uint32_t)i;
    }
    kept += (uint32_t)__popcll(__ballot(keep));
  }
  if (lane == 0 && kept) atomicAdd(reinterpret_cast<unsigned long long*>(p.count), (unsigned long long)kept);
}

__global__ __launch_bounds__(SRT_BLOCK) void srt_sort_gather_kernel(const SortArgs a, const uint32_t* order) {
  const PathPayloads& p = a.p;
  const int64_t total = *p.count;
  const int64_t end = p.activeOut ? p.n : total;
  const int64_t stride = (int64_t)gridDim.x * SRT_BLOCK;
  for (int64_t rank = (int64_t)blockIdx.x * SRT_BLOCK + threadIdx.x; rank < end; rank += stride) {
    if (rank < total) moveEntry(p, order[rank], rank);
    if (p.activeOut) p.activeOut[rank] = rank < total ? 1 : 0;
  }
}

// bits [0, endBit) of (key, index) between the double buffers; with temp == nullptr only *tempBytes is set
hipError_t sortPairs(void* temp, size_t* tempBytes, rocprim::double_buffer<uint32_t>& keys, rocprim::double_buffer<uint32_t>& index,
                     int64_t n, int endBit, hipStream_t stream) {
  return rocprim::radix_sort_pairs(temp, *tempBytes, keys, index, (size_t)n, 0u, (unsigned int)endBit, stream);
}

}  // namespace

extern "C" {

int srt_sort_temp_bytes(int64_t n, int cellBits, hipStream_t stream, size_t* bytes) {
  rocprim::double_buffer<uint32_t> keys(nullptr, nullptr), index(nullptr, nullptr);
  *bytes = 0;
  return (int)sortPairs(nullptr, bytes, keys, index, n, 3 * cellBits + 4, stream);
}

int srt_launch_sort(const SortArgs* a, int grid, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(a->p.count, 0, sizeof(int64_t), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(srt_sort_key_kernel, dim3(grid), dim3(SRT_BLOCK), 0, stream, *a);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  rocprim::double_buffer<uint32_t> keys(a->keys, a->keysSpare), index(a->index, a->indexSpare);
  size_t tempBytes = a->tempBytes;
  e = sortPairs(a->temp, &tempBytes, keys, index, a->p.n, 3 * a->cellBits + 4, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(srt_sort_gather_kernel, dim3(grid), dim3(SRT_BLOCK), 0, stream, *a, (const uint32_t*)index.current());
  return (int)hipGetLastError();
}

}  // extern "C"
