// srt_denoise.hip -- srtDenoise (include/srt_hip.h): an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) in the
// spatial form of SVGF, guided by the feature pass's normal and depth planes, luminance-stopped by a variance estimate
// carried from level to level, optionally demodulated by albedo.  The math is written out in the header; the NumPy
// reference tests/denoise_ref.py follows it operation by operation in the same order.
//
// Passes, all over 16x16 output tiles with one 256-thread workgroup per tile:
//   prepare  reads the four input planes once into a 22x22 LDS window (the tile and the 7x7 variance window's halo) as
//            {n.xyz, z} guide and {e.rgb, l} colour values, then per pixel writes the guide record, the depth gradient
//            (centre-only data, read once per pixel by the levels) and the first colour record {e.rgb, v}
//   level    one launch per a-trous level, ping-ponging between the two colour buffers.  A tap reads 32 B: the guide and
//            the colour record.  LDS form: the (16 + 4s)^2 window of both records staged first (s <= the denoise_lds_step
//            tunable, 8 at most: 73.7 KB); global form: the taps read through L1 / L2.  The last level writes the
//            caller's outputs instead of a colour record.
// A tap's weight is h[dx] h[dy] 2^t with ONE v_exp_f32, t summing every exponent: sigmaN log2(n_p.n_q) (ONE v_log_f32, no
// pow) minus (a_z + a_l) log2(e).  Nothing here is shared with the render kernels: their code objects do not change.
#include <hip/hip_runtime.h>

#include "srt_device.h"
#include "srt_launch.h"

namespace {

constexpr int DN_TILE = 16;
constexpr int DN_THREADS = DN_TILE * DN_TILE;
constexpr int PREP_HALO = 3;
constexpr int PREP_SIDE = DN_TILE + 2 * PREP_HALO;
constexpr float DN_LOG2E = 1.44269504088896340736f;
constexpr float DN_ALBEDO_MIN = 1e-3f;  // demodulation divides by max(albedo, this) per channel
constexpr float DN_DEPTH_EPS = 1e-3f;   // a_z's denominator: sigmaZ |grad z . delta| + this * z_p
constexpr float DN_LUM_EPS = 1e-10f;    // a_l's denominator: sigmaL sqrt(g_p) + this

__device__ __forceinline__ float meanOf(float sum, float count) { return count != 0.0f ? sum / count : 0.0f; }
__device__ __forceinline__ bool isHit(const float4& g) { return g.w == g.w; }      // a miss has z = NaN
__device__ __forceinline__ bool isValid(const float4& c) { return c.x == c.x; }    // not valid: e.x = NaN
__device__ __forceinline__ float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
__device__ __forceinline__ float4 nan4() { return make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")); }
__device__ __forceinline__ float albedoDiv(float sum, float count) { return fmaxf(meanOf(sum, count), DN_ALBEDO_MIN); }

// {n.xyz, z}: the normalised mean normal (0 if its length is 0) and the mean depth t of a hit; {0, 0, 0, NaN} for a miss
__device__ __forceinline__ float4 guideOf(const float4 nm, const float4 dp) {
  if (!(nm.w > 0.0f)) return make_float4(0.0f, 0.0f, 0.0f, __builtin_nanf(""));
  float nx = nm.x / nm.w, ny = nm.y / nm.w, nz = nm.z / nm.w;
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  if (len > 0.0f) {
    nx = nx / len;
    ny = ny / len;
    nz = nz / len;
  } else {
    nx = ny = nz = 0.0f;
  }
  return make_float4(nx, ny, nz, meanOf(dp.x, dp.w));
}

// {e.rgb, l}: the (demodulated) mean colour and its luminance; all NaN for a pixel that is not valid
__device__ __forceinline__ float4 colourOf(const DenoiseArgs& a, size_t i) {
  const float4 b = a.beauty[i];
  if (!(b.w > 0.0f)) return nan4();
  float r = b.x / b.w, g = b.y / b.w, bl = b.z / b.w;
  if (!__builtin_isfinite(r) || !__builtin_isfinite(g) || !__builtin_isfinite(bl)) return nan4();
  if (a.albedo) {
    const float4 al = a.albedo[i];
    r = r / albedoDiv(al.x, al.w);
    g = g / albedoDiv(al.y, al.w);
    bl = bl / albedoDiv(al.z, al.w);
  }
  return make_float4(r, g, bl, lum(r, g, bl));
}

// the one-sided depth difference along an axis with the smaller magnitude (ties: the backward one); 0 without a hit
// neighbour
__device__ __forceinline__ float oneSided(float zp, const float4& lo, const float4& hi) {
  const bool hl = isHit(lo), hh = isHit(hi);
  const float dl = zp - lo.w, dh = hi.w - zp;
  if (hl && hh) return fabsf(dh) < fabsf(dl) ? dh : dl;
  return hl ? dl : (hh ? dh : 0.0f);
}

// log2 of a tap's edge-stopping weight without the luminance term: sigmaN log2(max(0, n_p.n_q)) - a_z log2(e) between two
// hits, 0 between two misses; false between a hit and a miss (weight 0)
__device__ __forceinline__ bool geomLog2(const float4& gp, const float4& gq, float gradDelta, float zEps, float sigN,
                                         float sigZ, float& t) {
  const bool hp = isHit(gp);
  if (hp != isHit(gq)) return false;
  t = 0.0f;
  if (hp) {
    const float d = fmaxf(gp.x * gq.x + gp.y * gq.y + gp.z * gq.z, 0.0f);
    const float az = fabsf(gp.w - gq.w) * __builtin_amdgcn_rcpf(sigZ * fabsf(gradDelta) + zEps);
    t = sigN * __builtin_amdgcn_logf(d) - az * DN_LOG2E;  // log2(0) = -inf: weight 0
  }
  return true;
}

// MOMENTS (srtDenoiseMoments): the level-0 variance of a pixel with a usable moments record is the sample variance of its
// mean luminance instead of the spatial estimate (header: "Sample variance")
template <bool MOMENTS>
__global__ __launch_bounds__(DN_THREADS) void srt_denoise_prepare(const DenoiseArgs a) {
  __shared__ float4 sG[PREP_SIDE * PREP_SIDE];
  __shared__ float4 sC[PREP_SIDE * PREP_SIDE];  // {e.rgb, l}; cells outside the image: a miss that is not valid
  const int x0 = (int)blockIdx.x * DN_TILE - PREP_HALO, y0 = (int)blockIdx.y * DN_TILE - PREP_HALO;
  for (int c = threadIdx.x; c < PREP_SIDE * PREP_SIDE; c += DN_THREADS) {
    const int gx = x0 + c % PREP_SIDE, gy = y0 + c / PREP_SIDE;
    float4 g = make_float4(0.0f, 0.0f, 0.0f, __builtin_nanf("")), col = nan4();
    if (gx >= 0 && gy >= 0 && gx < a.width && gy < a.height) {
      const size_t i = (size_t)gy * a.width + gx;
      g = guideOf(a.normal[i], a.depth[i]);
      col = colourOf(a, i);
    }
    sG[c] = g;
    sC[c] = col;
  }
  __syncthreads();
  const int tx = threadIdx.x % DN_TILE, ty = threadIdx.x / DN_TILE;
  const int x = (int)blockIdx.x * DN_TILE + tx, y = (int)blockIdx.y * DN_TILE + ty;
  if (x >= a.width || y >= a.height) return;
  const int c = (ty + PREP_HALO) * PREP_SIDE + tx + PREP_HALO;
  const float4 gp = sG[c];
  float zx = 0.0f, zy = 0.0f;
  if (isHit(gp)) {
    zx = oneSided(gp.w, sG[c - 1], sG[c + 1]);
    zy = oneSided(gp.w, sG[c - PREP_SIDE], sG[c + PREP_SIDE]);
  }
  // level-0 variance of l over the valid pixels of the 7x7 window, weighted by the geometric edge stops at step 1
  // (moments about l_p, 0 for a centre that is not valid: a constant neighbourhood gives exactly 0)
  const float zEps = DN_DEPTH_EPS * gp.w;
  const float4 cp = sC[c];
  const float l0 = isValid(cp) ? cp.w : 0.0f;
  float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int dy = -PREP_HALO; dy <= PREP_HALO; ++dy) {
#pragma unroll
    for (int dx = -PREP_HALO; dx <= PREP_HALO; ++dx) {
      const float4 cq = sC[c + dy * PREP_SIDE + dx];
      if (!isValid(cq)) continue;
      float t;
      if (!geomLog2(gp, sG[c + dy * PREP_SIDE + dx], zx * (float)dx + zy * (float)dy, zEps, a.sigmaN, a.sigmaZ, t)) continue;
      const float w = __builtin_amdgcn_exp2f(t);
      const float dl = cq.w - l0;
      sw = sw + w;
      s1 = s1 + w * dl;
      s2 = s2 + w * (dl * dl);
    }
  }
  float v = 0.0f;
  if (sw > 0.0f) {
    const float m1 = s1 / sw, m2 = s2 / sw;
    v = m2 - m1 * m1;
    v = v > 0.0f ? v : 0.0f;
  }
  const size_t i = (size_t)y * a.width + x;
  if constexpr (MOMENTS) {
    // v_p = max(0, S2 - S1^2 / n) / (n (n - 1)), the subtraction in double (it cancels at high sample counts); divided by
    // lum(a~_p)^2 when demodulating
    const float4 m = a.moments[i];
    const float n = m.w;
    if (n >= 2.0f && __builtin_isfinite(m.x) && __builtin_isfinite(m.y)) {
      const double s1 = (double)m.x, nd = (double)n;
      double d = (double)m.y - s1 * s1 / nd;
      d = d > 0.0 ? d : 0.0;
      v = (float)(d / (nd * (nd - 1.0)));
      if (a.albedo) {
        const float4 al = a.albedo[i];
        const float la = lum(albedoDiv(al.x, al.w), albedoDiv(al.y, al.w), albedoDiv(al.z, al.w));
        v = v / (la * la);
      }
    }
  }
  a.guide[i] = gp;
  a.grad[i] = make_float2(zx, zy);
  a.col[0][i] = make_float4(cp.x, cp.y, cp.z, v);
}

// One a-trous level at step `step`: colour records `in` -> `outCol`, or the caller's outputs when `last`.
template <bool LDS>
__global__ __launch_bounds__(DN_THREADS) void srt_denoise_level(const DenoiseArgs a, const float4* __restrict__ in,
                                                               float4* __restrict__ outCol, int step, int last) {
  extern __shared__ float4 win[];  // LDS form: [side^2] guide records, then [side^2] colour records
  const int tx = threadIdx.x % DN_TILE, ty = threadIdx.x / DN_TILE;
  const int x = (int)blockIdx.x * DN_TILE + tx, y = (int)blockIdx.y * DN_TILE + ty;
  const int halo = 2 * step, side = DN_TILE + 2 * halo;
  if (LDS) {
    const int x0 = (int)blockIdx.x * DN_TILE - halo, y0 = (int)blockIdx.y * DN_TILE - halo;
    for (int c = threadIdx.x; c < side * side; c += DN_THREADS) {
      const int gx = x0 + c % side, gy = y0 + c / side;
      float4 g = make_float4(0.0f, 0.0f, 0.0f, __builtin_nanf("")), col = nan4();
      if (gx >= 0 && gy >= 0 && gx < a.width && gy < a.height) {
        const size_t i = (size_t)gy * a.width + gx;
        g = a.guide[i];
        col = in[i];
      }
      win[c] = g;
      win[side * side + c] = col;
    }
    __syncthreads();
  }
  if (x >= a.width || y >= a.height) return;
  const size_t i = (size_t)y * a.width + x;
  const int wc = (ty + halo) * side + tx + halo;  // the centre's cell in the LDS window
  const float4 gp = LDS ? win[wc] : a.guide[i];
  const float4 cp = LDS ? win[side * side + wc] : in[i];
  // g_p: the [1, 2, 1]/4 blur of v over the 3x3 neighbourhood, taps outside the image dropped and the rest renormalised
  const float k3[3] = {0.25f, 0.5f, 0.25f};
  float gs = 0.0f, ks = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      if (x + dx < 0 || x + dx >= a.width || y + dy < 0 || y + dy >= a.height) continue;
      const float k = k3[dx + 1] * k3[dy + 1];
      const float vq = LDS ? win[side * side + wc + dy * side + dx].w : in[i + (ptrdiff_t)dy * a.width + dx].w;
      gs = gs + k * vq;
      ks = ks + k;
    }
  }
  const float gvar = gs / ks;
  const bool validP = isValid(cp);
  const float lp = validP ? lum(cp.x, cp.y, cp.z) : 0.0f;
  // colour sums about e_p (0 for a centre that is not valid): a constant neighbourhood comes back exactly
  const float er = validP ? cp.x : 0.0f, eg = validP ? cp.y : 0.0f, eb = validP ? cp.z : 0.0f;
  const float rl = validP ? DN_LOG2E / (a.sigmaL * sqrtf(gvar) + DN_LUM_EPS) : 0.0f;  // invalid centre: a_l = 0
  const float2 gr = a.grad[i];
  const float zEps = DN_DEPTH_EPS * gp.w;
  const float h[5] = {1.0f / 16, 4.0f / 16, 6.0f / 16, 4.0f / 16, 1.0f / 16};
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = y + dy * step;
    if (qy < 0 || qy >= a.height) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + dx * step;
      if (qx < 0 || qx >= a.width) continue;
      const int qc = wc + (dy * side + dx) * step;
      const size_t q = (size_t)qy * a.width + qx;
      const float4 cq = LDS ? win[side * side + qc] : in[q];
      if (!isValid(cq)) continue;
      const float4 gq = LDS ? win[qc] : a.guide[q];
      float t;
      if (!geomLog2(gp, gq, gr.x * (float)(dx * step) + gr.y * (float)(dy * step), zEps, a.sigmaN, a.sigmaZ, t)) continue;
      t = t - fabsf(lp - lum(cq.x, cq.y, cq.z)) * rl;
      const float w = (h[dx + 2] * h[dy + 2]) * __builtin_amdgcn_exp2f(t);
      sw = sw + w;
      sr = sr + w * (cq.x - er);
      sg = sg + w * (cq.y - eg);
      sb = sb + w * (cq.z - eb);
      sv = sv + (w * w) * cq.w;
    }
  }
  const bool valid = sw > 0.0f;
  const float4 r = valid ? make_float4(er + sr / sw, eg + sg / sw, eb + sb / sw, sv / sw / sw) : make_float4(__builtin_nanf(""), 0.0f, 0.0f, 0.0f);
  if (!last) {
    outCol[i] = r;
    return;
  }
  float m[3] = {0.0f, 0.0f, 0.0f};
  if (valid) {
    m[0] = r.x;
    m[1] = r.y;
    m[2] = r.z;
    if (a.albedo) {
      const float4 al = a.albedo[i];
      m[0] = m[0] * albedoDiv(al.x, al.w);
      m[1] = m[1] * albedoDiv(al.y, al.w);
      m[2] = m[2] * albedoDiv(al.z, al.w);
    }
  }
  if (a.out) a.out[i] = make_float4(m[0], m[1], m[2], a.beauty[i].w);
  if (a.rgba) {
    // srt_resolve_kernel's quantisation of a mean
    reinterpret_cast<uchar4*>(a.rgba)[i] = make_uchar4(srtQuantise8(m[0]), srtQuantise8(m[1]), srtQuantise8(m[2]), 255);
  }
}

}  // namespace

extern "C" {

// The prepare pass and `iterations` levels on `stream`; levels of step <= ldsMaxStep (<= 8) stage their window in LDS.
int srt_launch_denoise(const DenoiseArgs* a, int iterations, int ldsMaxStep, hipStream_t stream) {
  const dim3 grid((a->width + DN_TILE - 1) / DN_TILE, (a->height + DN_TILE - 1) / DN_TILE), block(DN_THREADS);
  if (a->moments)
    hipLaunchKernelGGL(srt_denoise_prepare<true>, grid, block, 0, stream, *a);
  else
    hipLaunchKernelGGL(srt_denoise_prepare<false>, grid, block, 0, stream, *a);
  hipError_t e = hipGetLastError();
  for (int lv = 0; lv < iterations && e == hipSuccess; ++lv) {
    const int step = 1 << lv, last = lv == iterations - 1;
    const float4* in = a->col[lv & 1];
    float4* out = a->col[(lv + 1) & 1];
    if (step <= ldsMaxStep && step <= 8) {
      const int side = DN_TILE + 4 * step;
      const size_t lds = (size_t)side * side * 2 * sizeof(float4);
      if (lds > 64 * 1024) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(srt_denoise_level<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) break;
      }
      hipLaunchKernelGGL(srt_denoise_level<true>, grid, block, lds, stream, *a, in, out, step, last);
    } else {
      hipLaunchKernelGGL(srt_denoise_level<false>, grid, block, 0, stream, *a, in, out, step, last);
    }
    e = hipGetLastError();
  }
  return (int)e;
}

}  // extern "C"
