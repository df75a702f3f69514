// srt_temporal.hip -- srtTemporalAccumulate (include/srt_hip.h "Temporal accumulation"): reproject the previous frame's
// accumulated radiance and moments onto the current camera, keep them where the surface is the same, add the current
// frame's samples.  The header states the math; this file follows its operation order exactly (the library builds with
// -ffp-contract=off and IEEE division and sqrt), so tests/temporal_ref.py reproduces every bit in NumPy float32.
//
// One thread per pixel over 16 x 16 tiles; every buffer is read and written as float4 records (the compiler narrows the
// loads of records it uses half of, the depth and moments planes).  The taps are a data-dependent gather of
// history records: neighbouring pixels gather neighbouring records, so they go through the vector L1.  No LDS, no scratch
// memory, no atomics.  The reprojection itself is srt_reproject.h's reprojectHistory, shared with srt_temporal_adaptive.hip.
// MOTION: srtTemporalAccumulateMotion's instances (a.motion set), the motion-aware form of the reprojection.
#include "srt_reproject.h"
#include "srt_launch.h"

namespace {

template <bool DEMOD, bool MOTION = false>
__global__ __launch_bounds__(TP_TILE* TP_TILE) void srt_temporal_kernel(const TemporalArgs a) {
  const int x = (int)blockIdx.x * TP_TILE + (int)(threadIdx.x % TP_TILE);
  const int y = (int)blockIdx.y * TP_TILE + (int)(threadIdx.x / TP_TILE);
  const int W = a.width, H = a.height;
  if (x >= W || y >= H) return;
  const size_t nPix = (size_t)W * H;
  const size_t i = (size_t)y * W + x;

  const float4 b = a.beauty[i];
  const float4 nm = a.normal[i], ps = a.position[i], dp = a.depth[i];
  float S1 = 0.0f, S2 = 0.0f;
  if (a.moments) {
    const float4 m = a.moments[i];
    S1 = m.x;
    S2 = m.y;
  }
  bool hit;
  V3f np;
  float tbar;
  pixelSurface(nm, dp, hit, np, tbar);
  const V3f Q{meanOf(ps.x, ps.w), meanOf(ps.y, ps.w), meanOf(ps.z, ps.w)};
  AlbedoTerms al;
  if constexpr (DEMOD) al = albedoTerms(a.albedo[i]);
  const V3f at = al.at;
  const float la = al.la, la2 = al.la2;
  const float n = b.w;
  const bool usable = n > 0.0f && finite(n) && finite(b.x) && finite(b.y) && finite(b.z) && finite(S1) && finite(S2);

  // ---- the reprojected history h
  float h[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // r, g, b, count, S1, S2
  bool has = false;
  reprojectHistory<MOTION>(a, x, y, hit, np, tbar, h, has);

  // ---- outputs
  const bool add = has && usable;
  if (a.beautyOut) {
    float4 o = b;
    if (add) {
      o.x = b.x + (DEMOD ? at.x * h[0] : h[0]);
      o.y = b.y + (DEMOD ? at.y * h[1] : h[1]);
      o.z = b.z + (DEMOD ? at.z * h[2] : h[2]);
      o.w = n + h[3];
    }
    a.beautyOut[i] = o;
  }
  if (a.momentsOut) {
    float4 o = make_float4(S1, S2, 0.0f, n);
    if (add) {
      o.x = S1 + (DEMOD ? la * h[4] : h[4]);
      o.y = S2 + (DEMOD ? la2 * h[5] : h[5]);
      o.w = n + h[3];
    }
    a.momentsOut[i] = o;
  }
  float r[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (usable) {
    const float cur[6] = {DEMOD ? b.x / at.x : b.x, DEMOD ? b.y / at.y : b.y, DEMOD ? b.z / at.z : b.z, n,
                          DEMOD ? S1 / la : S1,     DEMOD ? S2 / la2 : S2};
#pragma unroll
    for (int j = 0; j < 6; ++j) r[j] = has ? h[j] + cur[j] : cur[j];
  } else if (has) {
#pragma unroll
    for (int j = 0; j < 6; ++j) r[j] = h[j];
  }
  float4* const o0 = a.historyOut;
  o0[i] = make_float4(r[0], r[1], r[2], r[3]);
  o0[nPix + i] = hit ? make_float4(np.x, np.y, np.z, r[4]) : make_float4(__builtin_nanf(""), 0.0f, 0.0f, r[4]);
  o0[2 * nPix + i] = hit ? make_float4(Q.x, Q.y, Q.z, r[5]) : make_float4(0.0f, 0.0f, 0.0f, r[5]);
}

}  // namespace

extern "C" int srt_launch_temporal(const TemporalArgs* a, hipStream_t stream) {
  const dim3 grid((a->width + TP_TILE - 1) / TP_TILE, (a->height + TP_TILE - 1) / TP_TILE), block(TP_TILE * TP_TILE);
  if (a->motion && a->albedo)
    hipLaunchKernelGGL((srt_temporal_kernel<true, true>), grid, block, 0, stream, *a);
  else if (a->motion)
    hipLaunchKernelGGL((srt_temporal_kernel<false, true>), grid, block, 0, stream, *a);
  else if (a->albedo)
    hipLaunchKernelGGL(srt_temporal_kernel<true>, grid, block, 0, stream, *a);
  else
    hipLaunchKernelGGL(srt_temporal_kernel<false>, grid, block, 0, stream, *a);
  return (int)hipGetLastError();
}
