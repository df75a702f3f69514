// srt_temporal.hip -- srtTemporalAccumulate (include/srt_hip.h "Temporal accumulation"): reproject the previous frame's
// accumulated radiance and moments onto the current camera, keep them where the surface is the same, add the current
// frame's samples.  The header states the math; this file follows its operation order exactly (the library builds with
// -ffp-contract=off and IEEE division and sqrt), so tests/temporal_ref.py reproduces every bit in NumPy float32.
//
// One thread per pixel over 16 x 16 tiles; every buffer is read and written as float4 records (the compiler narrows the
// loads of records it uses half of, the depth and moments planes).  The taps are a data-dependent gather of
// history records: neighbouring pixels gather neighbouring records, so they go through the vector L1.  No LDS, no scratch
// memory, no atomics.
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

template <bool DEMOD>
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
  const bool hit = nm.w > 0.0f;
  V3f np{meanOf(nm.x, nm.w), meanOf(nm.y, nm.w), meanOf(nm.z, nm.w)};
  const float len = sqrtf(dot3(np, np));
  if (len > 0.0f && len < __builtin_inff()) {
    np.x = np.x / len;
    np.y = np.y / len;
    np.z = np.z / len;
  } else {
    np = V3f{0.0f, 0.0f, 0.0f};
  }
  const float tbar = meanOf(dp.x, dp.w);
  const V3f Q{meanOf(ps.x, ps.w), meanOf(ps.y, ps.w), meanOf(ps.z, ps.w)};
  V3f at{1.0f, 1.0f, 1.0f};
  float la = 1.0f, la2 = 1.0f;
  if constexpr (DEMOD) {
    const float4 al = a.albedo[i];
    at = V3f{fmaxf(meanOf(al.x, al.w), TP_ALBEDO_MIN), fmaxf(meanOf(al.y, al.w), TP_ALBEDO_MIN),
             fmaxf(meanOf(al.z, al.w), TP_ALBEDO_MIN)};
    la = 0.2126f * at.x + 0.7152f * at.y + 0.0722f * at.z;
    la2 = la * la;
  }
  const float n = b.w;
  const bool usable = n > 0.0f && finite(n) && finite(b.x) && finite(b.y) && finite(b.z) && finite(S1) && finite(S2);

  // ---- the reprojected history h
  float h[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // r, g, b, count, S1, S2
  bool has = false;
  if (a.historyIn) {
    const float4* const h0 = a.historyIn;
    const float4* const h1 = h0 + nPix;
    const float4* const h2 = h1 + nPix;
    int bx = x, by = y;
    float wt[4] = {1.0f, 0.0f, 0.0f, 0.0f};
    bool ok = true;
    V3f P{0.0f, 0.0f, 0.0f};
    float dlen = 0.0f;
    if (!a.sameCamera) {
      const float sc = ((float)x + 0.5f) / (float)(W - 1);
      const float tc = ((float)(H - y) + 0.5f) / (float)(H - 1);
      const V3f o = ld(a.cam.origin), ll = ld(a.cam.lleft), hz = ld(a.cam.horizontal), vt = ld(a.cam.vertical);
      const V3f d{((ll.x + sc * hz.x) + tc * vt.x) - o.x, ((ll.y + sc * hz.y) + tc * vt.y) - o.y,
                  ((ll.z + sc * hz.z) + tc * vt.z) - o.z};
      dlen = sqrtf(dot3(d, d));
      P = V3f{o.x + tbar * d.x, o.y + tbar * d.y, o.z + tbar * d.z};
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
            take = a.sameCamera || tapMatches(hit, np, P, planeLimit, a.normalCos, c1, c2);
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
  if (a->albedo)
    hipLaunchKernelGGL(srt_temporal_kernel<true>, grid, block, 0, stream, *a);
  else
    hipLaunchKernelGGL(srt_temporal_kernel<false>, grid, block, 0, stream, *a);
  return (int)hipGetLastError();
}
