// srt_reproject.h -- what the temporal kernels share (srt_temporal.hip, srt_temporal_adaptive.hip), one copy each: the small
// vector helpers, a pixel's surface from its feature records, the albedo terms of the demodulated history, the tap test
// and reprojectHistory, the reprojected history h of include/srt_hip.h "Temporal accumulation".  srt_temporal_kernel and
// srt_temporal_reproject_kernel both inline reprojectHistory, so "the reprojected h is srtTemporalAccumulate's" is one text.
// The header states the math; this file follows its operation order exactly.
#pragma once
#include <hip/hip_runtime.h>

#include "srt_device.h"

namespace {

constexpr int TP_TILE = 16;
constexpr float TP_ALBEDO_MIN = 1e-3f;  // srt_denoise.hip's DN_ALBEDO_MIN: the same divisor

struct V3f {
  float x, y, z;
};
__device__ __forceinline__ float dot3(const V3f a, const V3f b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3f ld(const float* p) { return V3f{p[0], p[1], p[2]}; }
__device__ __forceinline__ float meanOf(float sum, float count) { return count != 0.0f ? sum / count : 0.0f; }
__device__ __forceinline__ bool finite(float v) { return __builtin_isfinite(v); }

// the hit, normal and plane tests of a tap whose history record is {c1 = (n_q, S1), c2 = (Q_q, S2)}
__device__ __forceinline__ bool tapMatches(bool hit, const V3f np, const V3f P, float planeLimit, float normalCos, const float4 c1,
                                           const float4 c2) {
  const bool hitQ = c1.x == c1.x;  // nx = NaN marks a miss
  if (hitQ != hit) return false;
  if (!hit) return true;
  const V3f nq{c1.x, c1.y, c1.z};
  const V3f dq{c2.x - P.x, c2.y - P.y, c2.z - P.z};
  return dot3(np, nq) >= normalCos && fabsf(dot3(dq, np)) <= planeLimit;
}

// A pixel's surface from its normal and depth sums: hit, the unit mean normal (zero where it has no length) and the mean
// hit distance.
__device__ __forceinline__ void pixelSurface(const float4 nm, const float4 dp, bool& hit, V3f& np, float& tbar) {
  hit = nm.w > 0.0f;
  np = V3f{meanOf(nm.x, nm.w), meanOf(nm.y, nm.w), meanOf(nm.z, nm.w)};
  const float len = sqrtf(dot3(np, np));
  if (len > 0.0f && len < __builtin_inff()) {
    np.x = np.x / len;
    np.y = np.y / len;
    np.z = np.z / len;
  } else {
    np = V3f{0.0f, 0.0f, 0.0f};
  }
  tbar = meanOf(dp.x, dp.w);
}

// The albedo a demodulated history is multiplied back by: the mean albedo at, floored, its luminance la and la^2 (for S1
// and S2).  All ones without demodulation.
struct AlbedoTerms {
  V3f at{1.0f, 1.0f, 1.0f};
  float la = 1.0f, la2 = 1.0f;
};
__device__ __forceinline__ AlbedoTerms albedoTerms(const float4 al) {
  AlbedoTerms t;
  t.at = V3f{fmaxf(meanOf(al.x, al.w), TP_ALBEDO_MIN), fmaxf(meanOf(al.y, al.w), TP_ALBEDO_MIN),
             fmaxf(meanOf(al.z, al.w), TP_ALBEDO_MIN)};
  t.la = 0.2126f * t.at.x + 0.7152f * t.at.y + 0.0722f * t.at.z;
  t.la2 = t.la * t.la;
  return t;
}

// The reprojected history of pixel (x, y), whose surface is (hit, np, tbar): reproject the pixel into the previous camera,
// choose the taps, test them, blend the accepted ones, cap the count.  h = r, g, b, count, S1, S2 and has come in as zeros
// and false and stay so without history or an accepted tap.  The tap loop keeps the form DESIGN.md 5.9 asks for: loads
// under nested conditions, taps in a plain float[4][6].
// MOTION (include/srt_hip.h "Motion"): a.motion is the resolved motion plane.  The hit point moves by the pixel's mean
// displacement before it is projected and before the taps' plane test, and the camera-not-moved rule does not apply.
template <bool MOTION = false>
__device__ __forceinline__ void reprojectHistory(const TemporalArgs& a, int x, int y, bool hit, const V3f np, float tbar,
                                                 float (&h)[6], bool& has) {
  const int W = a.width, H = a.height;
  const size_t nPix = (size_t)W * H;
  if (a.historyIn) {
    const float4* const h0 = a.historyIn;
    const float4* const h1 = h0 + nPix;
    const float4* const h2 = h1 + nPix;
    int bx = x, by = y;
    float wt[4] = {1.0f, 0.0f, 0.0f, 0.0f};
    bool ok = true;
    V3f P{0.0f, 0.0f, 0.0f};
    float dlen = 0.0f;
    const bool sameCamera = !MOTION && a.sameCamera;
    if (!sameCamera) {
      const float sc = ((float)x + 0.5f) / (float)(W - 1);
      const float tc = ((float)(H - y) + 0.5f) / (float)(H - 1);
      const V3f o = ld(a.cam.origin), ll = ld(a.cam.lleft), hz = ld(a.cam.horizontal), vt = ld(a.cam.vertical);
      const V3f d{((ll.x + sc * hz.x) + tc * vt.x) - o.x, ((ll.y + sc * hz.y) + tc * vt.y) - o.y,
                  ((ll.z + sc * hz.z) + tc * vt.z) - o.z};
      dlen = sqrtf(dot3(d, d));
      P = V3f{o.x + tbar * d.x, o.y + tbar * d.y, o.z + tbar * d.z};
      if constexpr (MOTION) {  // P' = P + mbar: where the pixel's surface was in the history's frame
        const float4 mv = a.motion[(size_t)y * W + x];
        P = V3f{P.x + meanOf(mv.x, mv.w), P.y + meanOf(mv.y, mv.w), P.z + meanOf(mv.z, mv.w)};
      }
      const V3f po = ld(a.prev.origin), pl = ld(a.prev.lleft), pw = ld(a.prev.w), pH = ld(a.prev.horizontal),
                pV = ld(a.prev.vertical);
      const V3f v = hit ? V3f{P.x - po.x, P.y - po.y, P.z - po.z} : d;
      const V3f e{po.x - pl.x, po.y - pl.y, po.z - pl.z};
      const float f = dot3(e, pw);
      const float z = -dot3(v, pw);
      const float k = f / z;
      const V3f g{e.x + k * v.x, e.y + k * v.y, e.z + k * v.z};
      const float s = dot3(g, pH) / dot3(pH, pH);
      const float t = dot3(g, pV) / dot3(pV, pV);
      const float xf = s * (float)(W - 1) - 0.5f;
      const float yf = ((float)H + 0.5f) - t * (float)(H - 1);
      ok = z > 0.0f && xf > -1.0f && xf < (float)W && yf > -1.0f && yf < (float)H;  // NaN: no history
      if (ok) {
        const float xr = rintf(xf), yr = rintf(yf);
        if (fabsf(xf - xr) <= SRT_TEMPORAL_SNAP && fabsf(yf - yr) <= SRT_TEMPORAL_SNAP) {
          bx = (int)xr;
          by = (int)yr;
        } else {
          const float x0 = floorf(xf), y0 = floorf(yf);
          const float fx = xf - x0, fy = yf - y0;
          const float gx = 1.0f - fx, gy = 1.0f - fy;
          bx = (int)x0;
          by = (int)y0;
          wt[0] = gx * gy;
          wt[1] = fx * gy;
          wt[2] = gx * fy;
          wt[3] = fx * fy;
        }
      }
    }
    if (ok) {
      const float planeLimit = (a.planeDist * tbar) * dlen;
      bool acc[4];
      float tv[4][6];  // an accepted tap's r, g, b, count, S1, S2
      float wsum = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int tx = bx + (k & 1), ty = by + (k >> 1);
        bool take = false;
        float4 c0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c1 = c0, c2 = c0;
        if (wt[k] > 0.0f && tx >= 0 && tx < W && ty >= 0 && ty < H) {  // zero weight or outside: never read
          const size_t q = (size_t)ty * W + tx;
          c0 = h0[q];
          if (c0.w > 0.0f && c0.w < __builtin_inff()) {
            c1 = h1[q];
            c2 = h2[q];
            take = sameCamera || tapMatches(hit, np, P, planeLimit, a.normalCos, c1, c2);
          }
        }
        acc[k] = take;
        tv[k][0] = c0.x;
        tv[k][1] = c0.y;
        tv[k][2] = c0.z;
        tv[k][3] = c0.w;
        tv[k][4] = c1.w;
        tv[k][5] = c2.w;
        if (take) wsum = wsum + wt[k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!acc[k]) continue;
        const float wn = wt[k] / wsum;
#pragma unroll
        for (int j = 0; j < 6; ++j) h[j] = h[j] + wn * tv[k][j];
        has = true;
      }
      if (has && h[3] > a.maxHistory) {
        const float scale = a.maxHistory / h[3];
        h[0] = h[0] * scale;
        h[1] = h[1] * scale;
        h[2] = h[2] * scale;
        h[4] = h[4] * scale;
        h[5] = h[5] * scale;
        h[3] = a.maxHistory;
      }
    }
  }
}

}  // namespace
