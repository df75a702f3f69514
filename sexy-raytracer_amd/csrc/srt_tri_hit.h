// srt_tri_hit.h -- triangle::hit (model.h:104-154) for the host and the device: the exact test, one statement of it
// (srt_path.h's triHitV calls it; examples/tri_cert_probe.cpp compiles it for the host), and the CERTIFIED test the
// FAITHFUL render and trace kernels run first: the three inside-edge decisions from two one-FMA dot products over the
// 64-byte triFast record (srtTriFastRecord below, called by srt_records.h's triangleRecords), with an error bound that
// says when the signs are certain.  A lane whose signs are not certain runs the exact test, so the verdict is always
// the exact test's; t and p are computed by the same operations in both and carry the same bits.
// Every file that includes this is built with -ffp-contract=off; the FMAs below are written out.
//
// ---- the certified edge test
// The reference decides edge i from  s_i = fl( n . fl( e_i x q_i ) ),  e_i = fl(v_{i+1} - v_i), q_i = fl(p - v_i), n the
// float normal of the record, dot and cross in vec3.h's operation order.  Only the sign of s_i is used (s_i < 0: outside).
// In real numbers n . (e x q) = (n x e) . q.  Write m_i* = n x e_i (exact), w = q_0 = fl(p - v0), and
//   N = max |n_c|,  E = max over the three edges |e_i,c|,  W = |w.x| + |w.y| + |w.z|,  u = 2^-24.
// The record holds m0 = fl(m_0*), m1 = fl(m_1*) and k = fl(m_1* . e_0), each computed in double and rounded ONCE
// (products of two floats are exact in double: relative error of m below u (1 + 2^-28), of k below u |k| + 2^-50 N E^2).
// The kernel computes, with a0 = fma(m0.x, w.x, fma(m0.y, w.y, fl(m0.z w.z))) and b1 likewise from m1,
//   c_0 = a0,      c_1 = fl(b1 - k),      c_2 = -fl(a0 + b1).
// Why c_i ~ s_i:
//   edge 0   q_0 = w: s_0* := m_0* . w is what c_0 approximates.
//   edge 1   p - v1 = (p - v0) - (v1 - v0), and each of w, e_0, q_1 is one rounding away from its difference, so
//            q_1 = w - e_0 + r_1 with |r_1|_1 <= 2u (W + 3E)(1 + 2u);  m_1* . q_1 = m_1* . w - k* + m_1* . r_1.
//   edge 2   likewise q_2 = w + e_2 + r_2 (e_2 = fl(v0 - v2)), and m_2* . e_2 = 0 exactly.  The exact edge vectors sum to
//            zero, the rounded ones to rho with |rho_c| <= 3uE, so m_2* = -(m_0* + m_1*) + n x rho and
//            m_2* . q_2 = -(m_0* . w + m_1* . w) + (n x rho) . w + m_2* . r_2.
// Rounding, with |m_i,c*| <= 2NE (two products of magnitude <= NE):
//   reference  s_i sums six terms n_a e_b q_c of total magnitude <= 2NE |q_i|_1, each through at most five roundings
//              (product, difference, product with n_a, two additions): |s_i - m_i* . q_i| <= 10.01 u N E |q_i|_1,
//              |q_0|_1 = W, |q_1|_1 and |q_2|_1 <= (W + 3E)(1 + 2u);
//   a0, b1     three terms of total magnitude <= 2NE W, at most three roundings each, plus the rounding of m: within
//              8.01 u N E W of m_i* . w;
//   c_1        + the rounding of k (6.01 u N E^2: |k*| <= 2NE 3E), + one subtraction (u (2NE W + 6NE^2)), + m_1* . r_1
//              (4.01 u N E (W + 3E));
//   c_2        + one addition (4 u N E W), + (n x rho) . w (6 u N E W), + m_2* . r_2 (4.01 u N E (W + 3E)).
// Totals, |c_i - s_i| in units of u N E:   edge 0: 18.02 W    edge 1: 24.03 W + 54.06 E    edge 2: 40.05 W + 42.06 E.
// The certificate uses  tol = 64 u N E (W + E) + floor  (>= 1.18 x the worst column; W is summed in float, the tolerance
// is one fma: both within 3u of their values).  With |c_i - s_i| <= tol for every i:
//   min c_i >  tol: every s_i > 0, all three edges pass;   min c_i < -tol: that edge's s_i < 0, the triangle is missed;
// so the verdict "!(min c_i < 0)" is the reference's whenever |min c_i| > tol, and the lane is UNDECIDED otherwise
// (x -> x +- tol is monotone: the minimum of the c_i is within tol of the minimum of the s_i).  The largest
// |c_i - s_i| / (u N E (W + E)) that examples/tri_cert_probe.cpp has seen over 2 10^7 pairs (sweep 1 2000000) is 8.7 (bound: 64).
// Ranges.  The bound assumes roundings with relative error u and no overflow.  At record time a triangle is certified
// only if every component of e_0, e_1, e_2 is 0 or in [2^-36, 2^30], every component of n 0 or in [2^-72, 2^60], and every
// component of m0, m1 and k 0 or in [2^-120, 2^124]; otherwise kappa = +inf and every test of the triangle is undecided.
// A test is undecided as well unless W < wMax = 2^30 (DevScene::triWMax; 0 switches the certificate off): then every intermediate of both computations stays below
// 8 N E (W + 3E) < 2^125, nothing overflows, and with finite certified operands no NaN can arise on a decided lane (the
// hardware minimum drops a NaN operand, so this matters).  A non-finite or NaN W fails "W < 2^30" by itself.
// Underflow, gradual or flushed (the bound holds for both): an operation whose result or operand is below 2^-126 is off
// by at most eta = 2^-126 absolute.  Followed through both computations that is at most 14 eta (1 + N)(1 + E) for the
// reference and 26 eta (1 + N)(1 + E) for c_i; floor = 64 eta (1 + N)(1 + E) = 2^-120 (1 + N)(1 + E) covers both, and
// kappa = 64 u N E >= 2^-126 is normal for every certified triangle with N E != 0 (N E >= 2^-108).
// Record: (v0.xyz, d) (n.xyz, k) (m0.xyz, kappa) (m1.xyz, kappa E + floor), d = -dot3(n, v0) in dot3's operation
// order -- the value the exact test computes per call, so t keeps its bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "srt_device.h"

#define SRT_TRI_EPS 1.1920928955078125e-07f /* FLT_EPSILON, globals.h:14 */
#define SRT_TRI_FAST_SLOTS 4                /* float4 per triFast record */
#define SRT_TRI_W_MAX 0x1p30f

struct SrtTriRay {
  float ox, oy, oz, dx, dy, dz;
};

// Eigen 3-vector dot: x*x' + (y*y' + z*z')
SRT_HD inline float srtTriDot3(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + (ay * by + az * bz); }
// n . (e x q), vec3.h's cross inside Eigen's dot
SRT_HD inline float srtTriEdge(float nx, float ny, float nz, float ex, float ey, float ez, float qx, float qy, float qz) {
  return srtTriDot3(nx, ny, nz, ey * qz - ez * qy, ez * qx - ex * qz, ex * qy - ey * qx);
}

// model.h:104-154 on the triTest record (v0.xyz, n.x) (v1.xyz, n.y) (v2.xyz, n.z).  n is precomputed with the operation
// order of getNormal (model.h:276-283).  CLOSEST adds the t > tMax rejection the reference lacks.  Straight-line form of
// the reference's early returns (same comparisons, same NaN behaviour).
template <bool CLOSEST>
SRT_HD inline bool srtTriHitExact(float4 q0, float4 q1, float4 q2, const SrtTriRay& r, float tMin, float tMax, float& tOut) {
  const float nx = q0.w, ny = q1.w, nz = q2.w;
  const float NdotDir = srtTriDot3(nx, ny, nz, r.dx, r.dy, r.dz);
  // model.h:119-123: parallel, then back-face (dot(dir, n) has the same bits as dot(n, dir))
  bool ok = !(fabsf(NdotDir) < SRT_TRI_EPS) && !(NdotDir > 0);
  const float d = -srtTriDot3(nx, ny, nz, q0.x, q0.y, q0.z);
  const float t = -(srtTriDot3(nx, ny, nz, r.ox, r.oy, r.oz) + d) / NdotDir;
  ok = ok && !(t < tMin);
  if (CLOSEST) ok = ok && !(t > tMax);
  const float px = r.ox + t * r.dx, py = r.oy + t * r.dy, pz = r.oz + t * r.dz;
  // the three inside-edge tests (model.h:135-154); a NaN passes, as in the reference
  ok = ok && !(srtTriEdge(nx, ny, nz, q1.x - q0.x, q1.y - q0.y, q1.z - q0.z, px - q0.x, py - q0.y, pz - q0.z) < 0);
  ok = ok && !(srtTriEdge(nx, ny, nz, q2.x - q1.x, q2.y - q1.y, q2.z - q1.z, px - q1.x, py - q1.y, pz - q1.z) < 0);
  ok = ok && !(srtTriEdge(nx, ny, nz, q0.x - q2.x, q0.y - q2.y, q0.z - q2.z, px - q2.x, py - q2.y, pz - q2.z) < 0);
  tOut = t;
  return ok;
}

SRT_HD inline float srtTriMin3(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;  // (fminf makes the compiler quiet its operands first; see srt_slab.h)
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  return fminf(fminf(a, b), c);
#endif
}

// The certified FAITHFUL test on the triFast record f0..f3.  Returns the verdict of the plane conditions and the cheap edge
// signs; `undecided` is raised only for a lane whose plane conditions passed (back faces, parallel rays and t < tMin never
// need the edges) and whose edge signs are not certain: the caller then runs srtTriHitExact<false> for it.  tOut is the
// exact test's t, bit for bit.  c[4] (optional, for the probe): the three cheap edge values, and 1 or 0 for the plane conditions.
SRT_HD inline bool srtTriHitCert(float4 f0, float4 f1, float4 f2, float4 f3, const SrtTriRay& r, float tMin, float wMax, float& tOut, bool& undecided,
                                 float* c = nullptr) {
  const float NdotDir = srtTriDot3(f1.x, f1.y, f1.z, r.dx, r.dy, r.dz);
  bool ok = !(fabsf(NdotDir) < SRT_TRI_EPS) & !(NdotDir > 0);
  const float t = -(srtTriDot3(f1.x, f1.y, f1.z, r.ox, r.oy, r.oz) + f0.w) / NdotDir;
  ok = ok & !(t < tMin);
  const float px = r.ox + t * r.dx, py = r.oy + t * r.dy, pz = r.oz + t * r.dz;
  const float wx = px - f0.x, wy = py - f0.y, wz = pz - f0.z;
  const float a0 = __builtin_fmaf(f2.x, wx, __builtin_fmaf(f2.y, wy, f2.z * wz));
  const float b1 = __builtin_fmaf(f3.x, wx, __builtin_fmaf(f3.y, wy, f3.z * wz));
  const float c1 = b1 - f1.w;
  const float s = a0 + b1;
  const float mn = srtTriMin3(a0, c1, -s);
  const float W = fabsf(wx) + fabsf(wy) + fabsf(wz);
  const float tol = __builtin_fmaf(f2.w, W, f3.w);
  // also undecided: a NaN in W or tol, kappa = +inf (an uncertified triangle), W beyond the overflow guard
  undecided = ok & !((fabsf(mn) > tol) & (W < wMax));
  if (c) {
    c[0] = a0;
    c[1] = c1;
    c[2] = -s;
    c[3] = ok ? 1.0f : 0.0f;
  }
  tOut = t;
  return ok & !(mn < 0);
}

// ---- the triFast record of a triangle (v0, v1, v2 and its float normal n as triTest holds it).  Double arithmetic, IEEE
// on the host and on the device: the same bits from srt_scene.cpp and from srt_refit.hip.
SRT_HD inline bool srtTriCertRange(float x, float lo, float hi) {
  const float ax = fabsf(x);
  return x == 0.0f || (ax >= lo && ax <= hi);
}
SRT_HD inline void srtTriFastRecord(const float* v0, const float* v1, const float* v2, const float* n, float4* fast) {
  float e[3][3];
  for (int c = 0; c < 3; ++c) {
    e[0][c] = v1[c] - v0[c];
    e[1][c] = v2[c] - v1[c];
    e[2][c] = v0[c] - v2[c];
  }
  const float d = -srtTriDot3(n[0], n[1], n[2], v0[0], v0[1], v0[2]);
  double md[2][3];
  float m[2][3];
  for (int i = 0; i < 2; ++i) {
    md[i][0] = (double)n[1] * (double)e[i][2] - (double)n[2] * (double)e[i][1];
    md[i][1] = (double)n[2] * (double)e[i][0] - (double)n[0] * (double)e[i][2];
    md[i][2] = (double)n[0] * (double)e[i][1] - (double)n[1] * (double)e[i][0];
    for (int c = 0; c < 3; ++c) m[i][c] = (float)md[i][c];
  }
  const float k = (float)(md[1][0] * (double)e[0][0] + md[1][1] * (double)e[0][1] + md[1][2] * (double)e[0][2]);
  float N = 0.0f, E = 0.0f;
  bool ok = srtTriCertRange(k, 0x1p-120f, 0x1p124f);
  for (int c = 0; c < 3; ++c) {
    N = fmaxf(N, fabsf(n[c]));
    ok = ok && srtTriCertRange(n[c], 0x1p-72f, 0x1p60f);
    for (int i = 0; i < 3; ++i) {
      E = fmaxf(E, fabsf(e[i][c]));
      ok = ok && srtTriCertRange(e[i][c], 0x1p-36f, 0x1p30f);
    }
    for (int i = 0; i < 2; ++i) ok = ok && srtTriCertRange(m[i][c], 0x1p-120f, 0x1p124f);
  }
  // a NaN or infinite coordinate fails a range above (NaN compares false, inf - inf is NaN, inf exceeds every range)
  const double kappa = 0x1p-18 * (double)N * (double)E;  // 64 u N E
  const double floorAbs = 0x1p-120 * (1.0 + (double)N) * (1.0 + (double)E);
  fast[0] = make_float4(v0[0], v0[1], v0[2], d);
  fast[1] = make_float4(n[0], n[1], n[2], k);
  fast[2] = make_float4(m[0][0], m[0][1], m[0][2], ok ? (float)kappa : __builtin_huge_valf());
  fast[3] = make_float4(m[1][0], m[1][1], m[1][2], ok ? (float)(kappa * (double)E + floorAbs) : __builtin_huge_valf());
}
