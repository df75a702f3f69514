// srt_temporal_adaptive.hip -- the two kernels of srtRenderTemporalAdaptive (include/srt_hip.h "Temporal-adaptive
// frames"): the reprojected history h of "Temporal accumulation" written out once per frame, and the per-round update
// that pools it with the frame's sums before srtRenderAdaptive's convergence test.
//
// srt_temporal_reproject_kernel is the first half of srt_temporal_kernel (srt_temporal.hip), restated rather than shared:
// that kernel's device code stays what it was, and the tap loop keeps the form its compiler note asks for (loads under
// nested conditions, taps in a plain float[4][6]).  The header states the math; this file follows its
// operation order exactly (the library builds with -ffp-contract=off and IEEE division and sqrt), so
// tests/temporal_adaptive_ref.py reproduces every bit in NumPy float32.
//
// One thread per pixel over 16 x 16 tiles for the reprojection (a data-dependent gather of history records through the
// vector L1), one wave per listed 8 x 8 tile for the update (srt_adaptive_update_kernel's shape).  No LDS, no scratch
// memory, no atomics.
#include <hip/hip_runtime.h>

#include "srt_device.h"

namespace {

constexpr int TP_TILE = 16;
constexpr float TP_ALBEDO_MIN = 1e-3f;  // srt_temporal.hip's (and the denoiser's) albedo divisor
constexpr int AD_WAVES = 4;             // tiles (waves) per workgroup of the update kernel, as srt_adaptive.hip

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
    const float4 nm = a.normal[i], dp = a.depth[i];
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
  float4* const o0 = a.historyOut;
  o0[i] = make_float4(h[0], h[1], h[2], h[3]);  // h is all zeros without an accepted tap
  o0[nPix + i] = make_float4(h[4], h[5], 0.0f, has ? 1.0f : 0.0f);
}

// srt_adaptive.hip's convergence test, word for word: in double, in the header's operation order.  limit = 4 thr^2.
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
  const uint32_t txy = list[i];
  const int px = (int)(txy & 0xffffu) * SRT_TILE_W + (lane & (SRT_TILE_W - 1));
  const int py = (int)(txy >> 16) * SRT_TILE_H + (lane >> 3);
  const bool inImage = px < width && py < height;  // edge tiles: the padding lanes are skipped
  const size_t idx = (size_t)py * width + px;
  bool open = false;
  if (inImage) {
    float4 b = accum[idx];
    float4 m = moments[idx];
    if constexpr (ACCUM) {
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
      float la = 1.0f, la2 = 1.0f;
      if constexpr (DEMOD) {
        const float4 al = albedo[idx];
        const V3f at{fmaxf(meanOf(al.x, al.w), TP_ALBEDO_MIN), fmaxf(meanOf(al.y, al.w), TP_ALBEDO_MIN),
                     fmaxf(meanOf(al.z, al.w), TP_ALBEDO_MIN)};
        la = 0.2126f * at.x + 0.7152f * at.y + 0.0722f * at.z;
        la2 = la * la;
      }
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
