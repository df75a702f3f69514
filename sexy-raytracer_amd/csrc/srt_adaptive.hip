// srt_adaptive.hip -- the small kernels around the render launches of srtRenderAdaptive (include/srt_hip.h "Adaptive
// sampling"): the accumulate-scatter of a launch's tile outputs into the image-order sums, the convergence test with its
// per-tile reduction, the order-preserving compaction of the active tiles into the next launch's tile table, and the
// resolve with the per-pixel sample count.  The render kernels are not touched: a launch over a tile list is the plain
// render with RenderArgs::tileXY pointing at the list (srt_render.cpp srtRenderTilesImpl).
//
// All of them are HBM-bound and tiny next to a render: one wave per listed tile (64 lanes, 64 pixels) for the update,
// one 1024-thread workgroup for the compaction (a few bytes per tile), one thread per pixel for the resolve.
#include "srt_adaptive_common.h"
#include "srt_launch.h"

namespace {

constexpr int AD_COMPACT_THREADS = 1024;

// One wave per listed tile.  ACCUM: adds tile i's beauty and moments (the render's tile-major outputs, list position i)
// into the image-order sums, one float add per channel.  DECIDE: flags[i] = 1 iff an in-image pixel of the tile is not
// converged after that (the moments just written, or the resolved ones when not accumulating).
template <bool ACCUM, bool DECIDE>
__global__ __launch_bounds__(64 * AD_WAVES) void srt_adaptive_update_kernel(const uint32_t* list, int count,
                                                                             const float4* beautyTiles,
                                                                             const float4* momentTiles, float4* accum,
                                                                             float4* moments, int32_t* flags, int width,
                                                                             int height, double limit) {
  const int i = blockIdx.x * AD_WAVES + (int)(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= count) return;  // whole waves
  size_t idx;
  const bool inImage = listedTilePixel(list[i], lane, width, height, idx);
  float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (inImage) {
    if constexpr (ACCUM) {
      const float4 b = beautyTiles[(size_t)i * SRT_TILE_PIXELS + lane];
      const float4 t = momentTiles[(size_t)i * SRT_TILE_PIXELS + lane];
      float4 a = accum[idx];
      m = moments[idx];
      a.x = a.x + b.x;
      a.y = a.y + b.y;
      a.z = a.z + b.z;
      a.w = a.w + b.w;
      m.x = m.x + t.x;
      m.y = m.y + t.y;
      m.z = m.z + t.z;
      m.w = m.w + t.w;
      accum[idx] = a;
      moments[idx] = m;
    } else {
      m = moments[idx];
    }
  }
  if constexpr (DECIDE) {
    const bool open = inImage && !adaptiveConverged(m, limit);
    const bool any = __any(open);
    if (lane == 0) flags[i] = any ? 1 : 0;
  }
}

// Order-preserving compaction of list[0, count) by flags into out; counts[0] = how many, counts[1] = their in-image
// pixels.  One workgroup: each thread takes a contiguous run of positions, an exclusive scan of the runs' counts places
// them.  (A frame has at most a few 10^5 tiles: a few microseconds.)
__global__ __launch_bounds__(AD_COMPACT_THREADS) void srt_adaptive_compact_kernel(const uint32_t* list, const int32_t* flags,
                                                                                   int count, uint32_t* out, int32_t* counts,
                                                                                   int width, int height) {
  __shared__ int waveSums[AD_COMPACT_THREADS / 64];
  __shared__ int pixelSum;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int per = (count + AD_COMPACT_THREADS - 1) / AD_COMPACT_THREADS;
  const int first = min(count, t * per), last = min(count, first + per);
  int mine = 0, pixels = 0;
  for (int k = first; k < last; ++k) {
    if (!flags[k]) continue;
    const uint32_t txy = list[k];
    const int w = min(SRT_TILE_W, width - (int)(txy & 0xffffu) * SRT_TILE_W);
    const int h = min(SRT_TILE_H, height - (int)(txy >> 16) * SRT_TILE_H);
    mine++;
    pixels += w * h;
  }
  if (t == 0) pixelSum = 0;
  // inclusive scan inside the wave
  int incl = mine;
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  if (lane == 63) waveSums[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += waveSums[w];
  int pos = base + incl - mine;
  for (int k = first; k < last; ++k)
    if (flags[k]) out[pos++] = list[k];
  atomicAdd(&pixelSum, pixels);
  __syncthreads();
  if (t == AD_COMPACT_THREADS - 1) {
    counts[0] = base + incl;
    counts[1] = pixelSum;
  }
}

// srtResolveTiles's quantisation with the pixel's own count: sqrtf(c * (1 / w)), clamp to 0.999, x256 truncated, NaN -> 0.
__global__ void srt_adaptive_resolve_kernel(const float4* accum, uchar4* rgba, int n) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const float4 v = accum[idx];
  const float scale = 1.0f / v.w;
  rgba[idx] = make_uchar4(srtQuantise8(v.x * scale), srtQuantise8(v.y * scale), srtQuantise8(v.z * scale), 255);
}

}  // namespace

extern "C" {

// accumulate: add the launch's tile outputs; decide: write flags (then compact).  At least one of the two.
int srt_launch_adaptive_update(const uint32_t* list, int count, const float4* beautyTiles, const float4* momentTiles,
                               float4* accum, float4* moments, int32_t* flags, int width, int height, double limit,
                               bool accumulate, bool decide, hipStream_t stream) {
  if (count <= 0) return 0;
  const dim3 grid((count + AD_WAVES - 1) / AD_WAVES), block(64 * AD_WAVES);
  if (accumulate && decide)
    hipLaunchKernelGGL((srt_adaptive_update_kernel<true, true>), grid, block, 0, stream, list, count, beautyTiles, momentTiles,
                       accum, moments, flags, width, height, limit);
  else if (accumulate)
    hipLaunchKernelGGL((srt_adaptive_update_kernel<true, false>), grid, block, 0, stream, list, count, beautyTiles, momentTiles,
                       accum, moments, flags, width, height, limit);
  else
    hipLaunchKernelGGL((srt_adaptive_update_kernel<false, true>), grid, block, 0, stream, list, count, beautyTiles, momentTiles,
                       accum, moments, flags, width, height, limit);
  return (int)hipGetLastError();
}

int srt_launch_adaptive_compact(const uint32_t* list, const int32_t* flags, int count, uint32_t* out, int32_t* counts,
                                int width, int height, hipStream_t stream) {
  hipLaunchKernelGGL(srt_adaptive_compact_kernel, dim3(1), dim3(AD_COMPACT_THREADS), 0, stream, list, flags, count, out, counts,
                     width, height);
  return (int)hipGetLastError();
}

int srt_launch_adaptive_resolve(const float4* accum, uint8_t* rgba, int n, hipStream_t stream) {
  hipLaunchKernelGGL(srt_adaptive_resolve_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, accum,
                     reinterpret_cast<uchar4*>(rgba), n);
  return (int)hipGetLastError();
}

}  // extern "C"
