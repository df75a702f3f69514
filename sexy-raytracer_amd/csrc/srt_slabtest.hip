// srt_slabtest.hip -- two test hooks on the certified slab test as the device compiles it (include/srt_hip_test.h
// srtTestRefinedRcp, srtTestSlabVisit; tests/test_gpu_slab_cert.py).  A translation unit of its own: no kernel that renders or
// answers a query is built from this file, and none of them includes anything from it.  Both kernels call the functions of
// srt_path.h / srt_query_walk.h that the production kernels call per ray and per visit, not copies of them.

#include "srt_path.h"
#include "srt_query_walk.h"
#include "srt_launch.h"

namespace {

// The refined reciprocal over a range of float bit patterns: one lane per pattern, grid-stride.  e = |r d - 1| in double (the
// product of two floats is exact there); a NaN (d = 0: the Newton step makes one of 0 * inf) counts as +inf.  Every wave leaves
// its largest e and the pattern that gave it (the lowest one on a tie) in partial[2 * wave], [2 * wave + 1]; a wave without
// a pattern leaves e = -1.  The host takes the maximum of the SRT_SLABTEST_RCP_WAVES partials.
__global__ __launch_bounds__(SRT_BLOCK) void srt_slabtest_rcp_kernel(uint32_t firstBits, int64_t count, unsigned long long* partial) {
  double best = -1.0;
  uint32_t bestBits = 0;
  for (int64_t i = (int64_t)blockIdx.x * SRT_BLOCK + threadIdx.x; i < count; i += (int64_t)gridDim.x * SRT_BLOCK) {
    const uint32_t bits = firstBits + (uint32_t)i;
    const float d = __uint_as_float(bits);
    const float r = refinedRcp(d);
    double e = fabs((double)r * (double)d - 1.0);
    if (e != e) e = (double)SRT_INF;
    if (e > best) {  // (patterns ascend along a lane's trips: the first of equal errors stays)
      best = e;
      bestBits = bits;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double e2 = __shfl_xor(best, off, 64);
    const uint32_t b2 = __shfl_xor(bestBits, off, 64);
    if (e2 > best || (e2 == best && b2 < bestBits)) {
      best = e2;
      bestBits = b2;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    const int wave = blockIdx.x * (SRT_BLOCK / 64) + (threadIdx.x >> 6);  // < SRT_SLABTEST_RCP_WAVES: the launcher's grid
    partial[2 * wave] = (unsigned long long)__double_as_longlong(best);
    partial[2 * wave + 1] = bestBits;
  }
}

// One (box, ray) case per lane, as a kernel treats a ray (the certificate's per-ray setup in both forms) and one visit of a
// node with that box.  tMin is the kernel argument itself: boxHitApprox<true> and boxHitSign<true> read it from its scalar
// register, as in the render kernels (the other functions take it as a vector operand).  in: 13 floats per case; out: 8
// words per case (include/srt_hip_test.h).
__global__ __launch_bounds__(SRT_BLOCK) void srt_slabtest_visit_kernel(const float* __restrict__ cases, int n, float tMin, int certifiedScene,
                                                                      float* __restrict__ out) {
  const int i = blockIdx.x * SRT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float* in = cases + 13 * (size_t)i;
  const float4 n0 = make_float4(in[0], in[1], in[2], 0.0f), n1 = make_float4(in[3], in[4], in[5], 0.0f);
  Ray r;
  r.o = mk(in[6], in[7], in[8]);
  r.d = mk(in[9], in[10], in[11]);
  r.time = 0.0f;
  const float tMax = in[12];
  const bool certified = (certifiedScene != 0) & fastDivOperandOk(r.o.x, r.d.x) & fastDivOperandOk(r.o.y, r.d.y) & fastDivOperandOk(r.o.z, r.d.z);
  const V3 rcp = mk(refinedRcp(r.d.x), refinedRcp(r.d.y), refinedRcp(r.d.z));
  V3 m, mSign, rp, rq;
  float tolAbs, tolAbsSign;
  slabSetup(r.o, rcp, certified, m, tolAbs);
  slabSetupSign(r.o, rcp, certified, rp, rq, mSign, tolAbsSign);
  bool uLane, uUniform, uSign;
  const bool vLane = boxHitApprox<false>(n0, n1, rcp, m, tolAbs, tMin, tMax, uLane);
  const bool vUniform = boxHitApprox<true>(n0, n1, rcp, m, tolAbs, tMin, tMax, uUniform);
  const bool vSign = boxHitSign<true>(n0, n1, rp, rq, mSign, tolAbsSign, tMin, tMax, uSign);
  float tEnter, tEnterLoose;
  const bool maybe = boxMaybeHit(n0, n1, rcp, m, tolAbs, tMin, tMax, tEnter);
  const bool exact = boxHit(n0, n1, r, tMin, tMax);
  const bool loose = boxHitLoose(n0, n1, r, tMin, tMax, tEnterLoose);
  const bool gate = boxHitOrGate(n0, n1, r, tMin, tMax, true);  // the case's box as an inner node of the regrouped tree
  const uint32_t flags = (uint32_t)certified | (uint32_t)vLane << 1 | (uint32_t)uLane << 2 | (uint32_t)vUniform << 3 | (uint32_t)uUniform << 4 |
                         (uint32_t)vSign << 5 | (uint32_t)uSign << 6 | (uint32_t)maybe << 7 | (uint32_t)exact << 8 | (uint32_t)loose << 9 |
                         (uint32_t)gate << 10;
  float* o = out + 8 * (size_t)i;
  o[0] = rcp.x;
  o[1] = rcp.y;
  o[2] = rcp.z;
  o[3] = tolAbs;
  o[4] = tolAbsSign;
  o[5] = __uint_as_float(flags);
  o[6] = tEnter;
  o[7] = tEnterLoose;
}

}  // namespace

extern "C" {

// partial: 2 * SRT_SLABTEST_RCP_WAVES words
int srt_launch_slabtest_rcp(uint32_t firstBits, int64_t count, unsigned long long* partial, hipStream_t stream) {
  static_assert(SRT_SLABTEST_RCP_WAVES % (SRT_BLOCK / 64) == 0, "whole workgroups");
  hipLaunchKernelGGL(srt_slabtest_rcp_kernel, dim3(SRT_SLABTEST_RCP_WAVES / (SRT_BLOCK / 64)), dim3(SRT_BLOCK), 0, stream, firstBits, count, partial);
  return (int)hipGetLastError();
}

// cases: 13 n floats, out: 8 n words, n >= 1
int srt_launch_slabtest_visit(const float* cases, int n, float tMin, int certifiedScene, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(srt_slabtest_visit_kernel, dim3((n + SRT_BLOCK - 1) / SRT_BLOCK), dim3(SRT_BLOCK), 0, stream, cases, n, tMin, certifiedScene, out);
  return (int)hipGetLastError();
}

}  // extern "C"
