// srt_slab.h -- the certified slab test (aabb.h:11-27 decided from one-FMA plane quotients) for the host and the device:
// one statement of its two forms (srt_path.h's boxHitApprox / boxMaybeHit / boxHitSign call it; examples/slab_probe.cpp
// compiles it for the host).  Every file that includes this is built with -ffp-contract=off; the FMAs are written out.
//
// ---- the certificate (both forms)
// The reference computes a = fl(fl(n - o) / d) per plane (aabb.h:14-17).  With r = refinedRcp(d) (within
// 3u of 1/d, u = 2^-24) and m = fl(-o * r), both per ray, A = fma(n, r, m) satisfies
//   |A - a| <= 6.2u |A| + 1.03u |o/d|            (one rounding each in r, m, the fma and the reference's
//                                                  subtraction and division; operands certified normal)
// i.e. a relative part and an absolute part K <= 2^-23 M, M = max_k |m_k|.  x -> x +- (eps|x| + K) is
// monotone, so min/max carry the bound through: the approximate interval ends tMinA, tMaxA are within
// eps|t| + K of the reference's (tMin and the running closest t are exact), and the reference's decision
// (tMax <= tMin -> miss) is certain whenever |tMaxA - tMinA| > eps (|tMaxA| + |tMinA|) + 2K with
// eps = 2^-21 (1.3x the bound).  tolAbs = 2K = 2^-22 M per ray, or +inf for a ray outside fastDiv's
// operand ranges (every visit of such a ray is "undecided" and takes the IEEE divisions).
// Checked against the reference's divisions case by case (examples/slab_probe.cpp, tests/test_slab_host.py): with r anywhere
// in the band |r d - 1| <= 3u, over 1.8 * 10^7 axis cases, no decided verdict differs, and the observed error of the clamped
// ends, (|tMinA - tMin| + |tMaxA - tMax|) / tol, reaches 0.71 of the tolerance (the derivation above gives <= 1; with eps
// halved it reaches 1.23).  The hypothesis on r is measured on the device over every float with 2^-20 <= |d| <= 2^20
// (srtTestRefinedRcp, tests/test_gpu_slab_cert.py): the largest |r d - 1| is 1.0000u (just under u, first at
// |d| = 0x1.fffffep-20) -- refinedRcp is within one ulp of 1/d there, a third of the band.
//
// ---- the two forms of the per-axis near and far quotients
// MIN/MAX form: ax = fma(n0.x, r, m), bx = fma(n1.x, r, m); near.x = min(ax, bx), far.x = max(ax, bx).  Six FMAs and
// six min/max per box.
// SIGN form: an FMA is monotone in its first operand (rounding is monotone), so for an ORDERED box (n0.x <= n1.x, both
// finite) the order of ax and bx is the sign of r: r > 0 gives ax <= bx, r < 0 gives bx <= ax.  With rp = max(r, 0) and
// rq = min(r, 0), once per ray, one of the two is zero and
//   near.x = fma(n0.x, rp, fma(n1.x, rq, m))      far.x = fma(n1.x, rp, fma(n0.x, rq, m))
// are those two values: a finite plane times 0 is 0, m + 0 = m, and the outer FMA is the quotient's own.  Twelve FMAs, no
// min/max, and the same values (a zero may carry the other sign: no comparison below sees that).  The sign form needs the
// scene's boxes ordered (srtBoxOrdered, srt_records.h; DevScene::boxOrderedScene) as well as the min/max form's ranges: a
// kernel that takes it treats every ray of a scene without the condition as uncertified.
// Both forms end in the same max3 / max / min3 / min, tolerance and verdict.  On the device the minima and maxima are
// the hardware instructions, written directly: fminf/fmaxf make the compiler quiet possible signalling NaNs first (a
// `v_max_f32 x, x` per live-in operand per visit), which buys nothing here -- v_min/v_max already return the other operand
// when one is a NaN, and the result only feeds the two comparisons of the certificate.  On the host they are plain
// comparisons (a NaN can reach them only on an uncertified ray, whose tolAbs = +inf leaves every visit undecided).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "srt_device.h"

struct SrtSlab3 {
  float x, y, z;
};

#define SRT_SLAB_FN SRT_HD __forceinline__
#if defined(__HIP_DEVICE_COMPILE__)
#define SRT_SLAB_ASM2(op, a, b)          \
  float r;                               \
  asm(op " %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); \
  return r
#define SRT_SLAB_ASM3(op, a, b, c)       \
  float r;                               \
  asm(op " %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); \
  return r
#endif
SRT_SLAB_FN float srtSlabMin(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  SRT_SLAB_ASM2("v_min_f32", a, b);
#else
  return b < a ? b : a;
#endif
}
SRT_SLAB_FN float srtSlabMax(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  SRT_SLAB_ASM2("v_max_f32", a, b);
#else
  return b > a ? b : a;
#endif
}
SRT_SLAB_FN float srtSlabMin3(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  SRT_SLAB_ASM3("v_min3_f32", a, b, c);
#else
  return srtSlabMin(srtSlabMin(a, b), c);
#endif
}
SRT_SLAB_FN float srtSlabMax3(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  SRT_SLAB_ASM3("v_max3_f32", a, b, c);
#else
  return srtSlabMax(srtSlabMax(a, b), c);
#endif
}
// b: wave-uniform (a kernel argument), read from its scalar register
SRT_SLAB_FN float srtSlabMaxUniform(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_max_f32 %0, %2, %1" : "=v"(r) : "v"(a), "s"(b));
  return r;
#else
  return srtSlabMax(a, b);
#endif
}

// ---- per ray and axis: the operand ranges the error bound assumes -- direction components in [2^-20, 2^20]; origin
// components 0 or in [2^-77, 2^30] (the scene's box coordinates are certified at upload: fastDivOperands, srt_records.h)
SRT_SLAB_FN bool srtSlabOperandOk(float o, float d) {
  float ad = fabsf(d), ao = fabsf(o);
  // bitwise: no short-circuit branches (each would cost the wave scalar exec-mask bookkeeping)
  return (ad >= 0x1p-20f) & (ad <= 0x1p20f) & ((o == 0.0f) | ((ao >= 0x1p-77f) & (ao <= 0x1p30f)));
}

// ---- per ray: m = fl(-o * r) and the absolute part of the certificate's tolerance
SRT_SLAB_FN void srtSlabSetup(SrtSlab3 o, SrtSlab3 r, bool certified, SrtSlab3& m, float& tolAbs) {
  m = SrtSlab3{-(o.x * r.x), -(o.y * r.y), -(o.z * r.z)};
  const float M = fmaxf(fmaxf(fabsf(m.x), fabsf(m.y)), fabsf(m.z));
  tolAbs = certified ? 0x1p-22f * M : __builtin_inff();
}
// the sign form's: the reciprocal split by its sign (it is not kept), the same m and tolAbs
SRT_SLAB_FN void srtSlabSignSetup(SrtSlab3 o, SrtSlab3 r, bool certified, SrtSlab3& rp, SrtSlab3& rq, SrtSlab3& m, float& tolAbs) {
  srtSlabSetup(o, r, certified, m, tolAbs);
  rp = SrtSlab3{fmaxf(r.x, 0.0f), fmaxf(r.y, 0.0f), fmaxf(r.z, 0.0f)};
  rq = SrtSlab3{fminf(r.x, 0.0f), fminf(r.y, 0.0f), fminf(r.z, 0.0f)};
}

// ---- per box: two quotients per axis.  Min/max form (ORDERED = false): a, b = the quotients of the planes n0, n1, ordered
// where they are used.  Sign form (ORDERED = true): a = near, b = far already.
struct SrtSlabEnds {
  SrtSlab3 a, b;
};
SRT_SLAB_FN SrtSlabEnds srtSlabEndsMinMax(float4 n0, float4 n1, SrtSlab3 r, SrtSlab3 m) {
  SrtSlabEnds e;
  e.a.x = __builtin_fmaf(n0.x, r.x, m.x), e.b.x = __builtin_fmaf(n1.x, r.x, m.x);
  e.a.y = __builtin_fmaf(n0.y, r.y, m.y), e.b.y = __builtin_fmaf(n1.y, r.y, m.y);
  e.a.z = __builtin_fmaf(n0.z, r.z, m.z), e.b.z = __builtin_fmaf(n1.z, r.z, m.z);
  return e;
}
SRT_SLAB_FN SrtSlabEnds srtSlabEndsSign(float4 n0, float4 n1, SrtSlab3 rp, SrtSlab3 rq, SrtSlab3 m) {
  SrtSlabEnds e;
  e.a.x = __builtin_fmaf(n0.x, rp.x, __builtin_fmaf(n1.x, rq.x, m.x));
  e.b.x = __builtin_fmaf(n1.x, rp.x, __builtin_fmaf(n0.x, rq.x, m.x));
  e.a.y = __builtin_fmaf(n0.y, rp.y, __builtin_fmaf(n1.y, rq.y, m.y));
  e.b.y = __builtin_fmaf(n1.y, rp.y, __builtin_fmaf(n0.y, rq.y, m.y));
  e.a.z = __builtin_fmaf(n0.z, rp.z, __builtin_fmaf(n1.z, rq.z, m.z));
  e.b.z = __builtin_fmaf(n1.z, rp.z, __builtin_fmaf(n0.z, rq.z, m.z));
  return e;
}
// the largest near and the smallest far quotient of the three axes
template <bool ORDERED>
SRT_SLAB_FN float srtSlabNear(const SrtSlabEnds& e) {
  if (ORDERED) return srtSlabMax3(e.a.x, e.a.y, e.a.z);
  return srtSlabMax3(srtSlabMin(e.a.x, e.b.x), srtSlabMin(e.a.y, e.b.y), srtSlabMin(e.a.z, e.b.z));
}
template <bool ORDERED>
SRT_SLAB_FN float srtSlabFar(const SrtSlabEnds& e) {
  if (ORDERED) return srtSlabMin3(e.b.x, e.b.y, e.b.z);
  return srtSlabMin3(srtSlabMax(e.a.x, e.b.x), srtSlabMax(e.a.y, e.b.y), srtSlabMax(e.a.z, e.b.z));
}

// ---- eps, the relative part of the certificate's tolerance tol = eps (|tMaxA| + |tMinA|) + tolAbs on the clamped ends: the
// one statement of it (examples/slab_probe.cpp measures the observed error of the ends against tol)
#define SRT_SLAB_EPS 0x1p-21f

// ---- the verdict both forms end in.  Returns the approximate verdict and whether it is uncertain (the caller then runs
// the exact test).  UNIFORM_TMIN: tMin is wave-uniform (a kernel argument) and is read from its scalar register
template <bool UNIFORM_TMIN, bool ORDERED>
SRT_SLAB_FN bool srtSlabVerdict(const SrtSlabEnds& e, float tolAbs, float tMin, float tMax, bool& undecided) {
  const float lo = srtSlabNear<ORDERED>(e);
  tMin = UNIFORM_TMIN ? srtSlabMaxUniform(lo, tMin) : srtSlabMax(lo, tMin);
  tMax = srtSlabMin(srtSlabFar<ORDERED>(e), tMax);
  const float diff = tMax - tMin;
  const float tol = __builtin_fmaf(SRT_SLAB_EPS, fabsf(tMax) + fabsf(tMin), tolAbs);
  undecided = !(fabsf(diff) > tol);  // also when a NaN got in, and always when tolAbs = +inf
  return diff > tol;
}
// ---- the GATE form of the exact test (aabb.h:11-27 with the IEEE divisions), for an inner node of the path-pool kernel's
// regrouped tree (srt_regroup.h), where a box decides nothing but whether the leaves below it are looked at: it must pass
// wherever the reference's test passes on a box inside it.  On an axis with a finite non-zero d the reference's quotients
// are monotone in the plane, so its own arithmetic is nested and is kept.  On an axis with d == +-0 the reference passes
// min < o < max (quotients -inf, +inf) and the point interval min == max == o (both quotients NaN, which fminf / fmaxf
// drop), and misses min == o < max (NaN and +inf: tMin becomes +inf) -- not nested: a flat leaf box passes inside a box
// that misses.  The gate takes the closed interval there, min <= o <= max, written so that a NaN origin passes as it does
// in the reference; it puts no bound on t.  examples/regroup_probe.cpp checks "leaf passes => gate passes" at these edges.
// ONE body for both: `gate` false is aabb.h:11-27 operation for operation (srt_path.h boxHit); true switches the d == +-0
// axes to the closed interval.  The six divisions are shared, so a kernel that judges gates and leaves in one block carries
// them once (per lane: an inner node of the regrouped tree is a gate, a leaf is not).
SRT_SLAB_FN void srtSlabExactAxis(float n0, float n1, float o, float d, bool gate, float& tMin, float& tMax, bool& inside) {
  const float a = (n0 - o) / d, b = (n1 - o) / d;
  const float lo = fmaxf(fminf(a, b), tMin), hi = fminf(fmaxf(a, b), tMax);
  const bool closed = gate & (d == 0.0f);
  tMin = closed ? tMin : lo;
  tMax = closed ? tMax : hi;
  inside = inside & !(closed & ((o < n0) | (o > n1)));
}
SRT_SLAB_FN bool srtSlabExactOrGate(float4 n0, float4 n1, SrtSlab3 o, SrtSlab3 d, float tMin, float tMax, bool gate) {
  bool inside = true;
  srtSlabExactAxis(n0.x, n1.x, o.x, d.x, gate, tMin, tMax, inside);
  srtSlabExactAxis(n0.y, n1.y, o.y, d.y, gate, tMin, tMax, inside);
  srtSlabExactAxis(n0.z, n1.z, o.z, d.z, gate, tMin, tMax, inside);
  return inside & !(tMax <= tMin);
}
SRT_SLAB_FN bool srtSlabGateExact(float4 n0, float4 n1, SrtSlab3 o, SrtSlab3 d, float tMin, float tMax) {
  return srtSlabExactOrGate(n0, n1, o, d, tMin, tMax, true);
}

// Closest-hit traversal: the same intervals used CONSERVATIVELY -- a box is entered unless it is certainly missed
// (tMaxA - tMinA < -tol), so no exact fallback is needed: a box entered needlessly costs time, never a hit.
// Returns the approximate entry distance for near-first ordering.
template <bool ORDERED>
SRT_SLAB_FN bool srtSlabMaybe(const SrtSlabEnds& e, float tolAbs, float tMin, float tMax, float& tEnter) {
  const float t0 = srtSlabMax(srtSlabNear<ORDERED>(e), tMin);
  const float t1 = srtSlabMin(srtSlabFar<ORDERED>(e), tMax);
  const float tol = __builtin_fmaf(SRT_SLAB_EPS, fabsf(t1) + fabsf(t0), tolAbs);
  tEnter = t0;
  return !(t1 - t0 < -tol);  // NaN or tolAbs = +inf (uncertified ray): enter
}
