// srt_adaptive_common.h -- what the per-round update kernels share (srt_adaptive.hip, srt_temporal_adaptive.hip), one copy
// each: their workgroup shape, the pixel a lane of a listed tile owns and the convergence test.  The accumulate step is stated
// in each kernel: the two read their four records in different orders, and one shared text changes one kernel's code.
#pragma once
#include <hip/hip_runtime.h>

#include "srt_device.h"

namespace {

constexpr int AD_WAVES = 4;  // tiles (waves) per workgroup of an update kernel

// The pixel of lane `lane` of the listed tile txy = tx | ty << 16: its image-order index; false for the padding lanes of an
// edge tile, which are skipped.
__device__ __forceinline__ bool listedTilePixel(uint32_t txy, int lane, int width, int height, size_t& idx) {
  const int px = (int)(txy & 0xffffu) * SRT_TILE_W + (lane & (SRT_TILE_W - 1));
  const int py = (int)(txy >> 16) * SRT_TILE_H + (lane >> 3);
  idx = (size_t)py * width + px;
  return px < width && py < height;
}

// The convergence test of include/srt_hip.h, in double and in the header's operation order (the library builds with
// -ffp-contract=off: no multiply-add forms).  limit = 4 thr^2, computed on the host.
__device__ inline bool adaptiveConverged(const float4 m, double limit) {
  const double s1 = (double)m.x, s2 = (double)m.y, n = (double)m.w;
  if (!isfinite(s1) || !isfinite(s2)) return true;  // more samples cannot repair a NaN or an infinity
  const double mu = s1 / n;
  const double sq = s1 * s1;
  const double d = s2 - sq / n;
  const double v = (d > 0.0 ? d : 0.0) / (n * (n - 1.0));
  const double floorMu = mu > 0x1p-16 ? mu : 0x1p-16;
  return v < limit * floorMu;
}

}  // namespace
