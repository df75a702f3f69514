// srt_temporal_adaptive.hip -- the two kernels of srtRenderTemporalAdaptive (include/srt_hip.h "Temporal-adaptive
// frames"): the reprojected history h of "Temporal accumulation" written out once per frame, and the per-round update
// that pools it with the frame's sums before srtRenderAdaptive's convergence test.
//
// srt_temporal_reproject_kernel is the first half of srt_temporal_kernel (srt_temporal.hip): both call srt_reproject.h's
// reprojectHistory, the one copy of the reprojection.  The update kernel's tile mapping and convergence test
// are srt_adaptive_common.h's, shared with srt_adaptive_update_kernel.  The header states the math; these files follow its
// operation order exactly (the library builds with -ffp-contract=off and IEEE division and sqrt), so
// tests/temporal_adaptive_ref.py reproduces every bit in NumPy float32.
//
// One thread per pixel over 16 x 16 tiles for the reprojection (a data-dependent gather of history records through the
// vector L1), one wave per listed 8 x 8 tile for the update (srt_adaptive_update_kernel's shape).  No LDS, no scratch
// memory, no atomics.
#include "srt_adaptive_common.h"
#include "srt_reproject.h"
#include "srt_launch.h"

namespace {

// Reads TemporalArgs's feature planes, cameras, historyIn and parameters; writes the two reprojected planes to
// historyOut: {h.r, h.g, h.b, h.count} and {h.S1, h.S2, 0, has}.  beauty, moments and albedo are not read.
__global__ __launch_bounds__(TP_TILE* TP_TILE) void srt_temporal_reproject_kernel(const TemporalArgs a) {
  const int x = (int)blockIdx.x * TP_TILE + (int)(threadIdx.x % TP_TILE);
  const int y = (int)blockIdx.y * TP_TILE + (int)(threadIdx.x / TP_TILE);
  const int W = a.width, H = a.height;
  if (x >= W || y >= H) return;
  const size_t nPix = (size_t)W * H;
  const size_t i = (size_t)y * W + x;

  float h[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // r, g, b, count, S1, S2
  bool has = false;
  if (a.historyIn) {
    bool hit;
    V3f np;
    float tbar;
    pixelSurface(a.normal[i], a.depth[i], hit, np, tbar);
    reprojectHistory(a, x, y, hit, np, tbar, h, has);
  }
  float4* const o0 = a.historyOut;
  o0[i] = make_float4(h[0], h[1], h[2], h[3]);  // h is all zeros without an accepted tap
  o0[nPix + i] = make_float4(h[4], h[5], 0.0f, has ? 1.0f : 0.0f);
}

// srtTemporalReprojectMotion (a.motion set): the kernel above with the motion-aware reprojection.  Stated a second time:
// as a template, or with the pixel's code in a shared inlined function, the kernel above lost its name or its instruction
// order against the build before this one (tools/isa_compare.py)
__global__ __launch_bounds__(TP_TILE* TP_TILE) void srt_temporal_reproject_motion_kernel(const TemporalArgs a) {
  const int x = (int)blockIdx.x * TP_TILE + (int)(threadIdx.x % TP_TILE);
  const int y = (int)blockIdx.y * TP_TILE + (int)(threadIdx.x / TP_TILE);
  const int W = a.width, H = a.height;
  if (x >= W || y >= H) return;
  const size_t nPix = (size_t)W * H;
  const size_t i = (size_t)y * W + x;

  float h[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  bool has = false;
  if (a.historyIn) {
    bool hit;
    V3f np;
    float tbar;
    pixelSurface(a.normal[i], a.depth[i], hit, np, tbar);
    reprojectHistory<true>(a, x, y, hit, np, tbar, h, has);
  }
  float4* const o0 = a.historyOut;
  o0[i] = make_float4(h[0], h[1], h[2], h[3]);
  o0[nPix + i] = make_float4(h[4], h[5], 0.0f, has ? 1.0f : 0.0f);
}

// One wave per listed tile.  ACCUM: adds tile i's beauty and moments (list position i of the launch's tile-major outputs)
// into the image-order sums, as srt_adaptive_update_kernel does.  Then the pooled moments M~ of the sums so far --
// srt_temporal_kernel's dMomentsOut, from the pixel's reprojected record instead of the gather -- go through the
// convergence test: flags[i] = 1 iff an in-image pixel of the tile is not converged.  DEMOD: the history is in
// demodulated units and is multiplied back by the pixel's albedo luminance.
template <bool ACCUM, bool DEMOD>
__global__ __launch_bounds__(64 * AD_WAVES) void srt_temporal_adaptive_update_kernel(
    const uint32_t* list, int count, const float4* beautyTiles, const float4* momentTiles, float4* accum, float4* moments,
    const float4* reprojected, const float4* albedo, int32_t* flags, int width, int height, double limit) {
  const int i = blockIdx.x * AD_WAVES + (int)(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= count) return;  // whole waves
  size_t idx;
  const bool inImage = listedTilePixel(list[i], lane, width, height, idx);
  bool open = false;
  if (inImage) {
    float4 b = accum[idx];
    float4 m = moments[idx];
    if constexpr (ACCUM) {  // as srt_adaptive_update_kernel adds them
      const float4 bt = beautyTiles[(size_t)i * SRT_TILE_PIXELS + lane];
      const float4 mt = momentTiles[(size_t)i * SRT_TILE_PIXELS + lane];
      b.x = b.x + bt.x;
      b.y = b.y + bt.y;
      b.z = b.z + bt.z;
      b.w = b.w + bt.w;
      m.x = m.x + mt.x;
      m.y = m.y + mt.y;
      m.z = m.z + mt.z;
      m.w = m.w + mt.w;
      accum[idx] = b;
      moments[idx] = m;
    }
    const float4 r0 = reprojected[idx];
    const float4 r1 = reprojected[(size_t)width * height + idx];
    const float S1 = m.x, S2 = m.y, n = b.w;
    const bool usable = n > 0.0f && finite(n) && finite(b.x) && finite(b.y) && finite(b.z) && finite(S1) && finite(S2);
    float4 pooled = make_float4(S1, S2, 0.0f, n);
    if (r1.w != 0.0f && usable) {
      AlbedoTerms al;
      if constexpr (DEMOD) al = albedoTerms(albedo[idx]);
      const float la = al.la, la2 = al.la2;
      pooled.x = S1 + (DEMOD ? la * r1.x : r1.x);
      pooled.y = S2 + (DEMOD ? la2 * r1.y : r1.y);
      pooled.w = n + r0.w;
    }
    open = !adaptiveConverged(pooled, limit);
  }
  const bool any = __any(open);
  if (lane == 0) flags[i] = any ? 1 : 0;
}

}  // namespace

extern "C" {

// a->historyOut receives the two reprojected planes; a->historyIn == nullptr writes zeros
int srt_launch_temporal_reproject(const TemporalArgs* a, hipStream_t stream) {
  const dim3 grid((a->width + TP_TILE - 1) / TP_TILE, (a->height + TP_TILE - 1) / TP_TILE), block(TP_TILE * TP_TILE);
  if (a->motion)
    hipLaunchKernelGGL(srt_temporal_reproject_motion_kernel, grid, block, 0, stream, *a);
  else
    hipLaunchKernelGGL(srt_temporal_reproject_kernel, grid, block, 0, stream, *a);
  return (int)hipGetLastError();
}

// accumulate: add the launch's tile outputs first; albedo != nullptr: the history is demodulated.  Always decides.
int srt_launch_temporal_adaptive_update(const uint32_t* list, int count, const float4* beautyTiles, const float4* momentTiles,
                                        float4* accum, float4* moments, const float4* reprojected, const float4* albedo,
                                        int32_t* flags, int width, int height, double limit, bool accumulate,
                                        hipStream_t stream) {
  if (count <= 0) return 0;
  const dim3 grid((count + AD_WAVES - 1) / AD_WAVES), block(64 * AD_WAVES);
#define SRT_TA_LAUNCH(ACCUM, DEMOD)                                                                                          \
  hipLaunchKernelGGL((srt_temporal_adaptive_update_kernel<ACCUM, DEMOD>), grid, block, 0, stream, list, count, beautyTiles, \
                     momentTiles, accum, moments, reprojected, albedo, flags, width, height, limit)
  if (accumulate && albedo)
    SRT_TA_LAUNCH(true, true);
  else if (accumulate)
    SRT_TA_LAUNCH(true, false);
  else if (albedo)
    SRT_TA_LAUNCH(false, true);
  else
    SRT_TA_LAUNCH(false, false);
#undef SRT_TA_LAUNCH
  return (int)hipGetLastError();
}

}  // extern "C"
