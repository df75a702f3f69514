// The certified slab test of csrc/srt_slab.h as a stand-alone host program (no GPU, no library): used by
// tests/test_slab_host.py, and the place for a sanitizer build of that header.
//   srt_slab_probe sweep <seed> <boxes per class>
//     seeded (ordered box, origin, direction, tMin, tMax) cases, class by class, three axis cases per box; per class one line
//       class <name> boxes <n> axes <n> certified <n> undecided <n> end_diff <n> verdict_diff <n> undecided_diff <n> decided_uncertified <n>
//             in_band <n> entered <n> wrong <n> maybe_wrong <n> max_ratio <x>
//     certified: boxes whose ray is inside srtSlabOperandOk's ranges on all three axes (the others get tolAbs = +inf);
//     undecided: boxes the min/max form leaves to the exact test; end_diff: axis cases whose sign-form near / far differ AS
//     FLOAT VALUES from min / max of the two one-FMA quotients (a NaN equals a NaN; certified rays only -- on the others the
//     verdict below is what counts); verdict_diff, undecided_diff: boxes on which the two forms' verdict / undecided differ;
//     decided_uncertified: uncertified boxes either form decides.  These four must be 0.
//     Against the reference's own arithmetic (aabb.h:14-22 restated here: float subtraction and division, fminf / fmaxf,
//     !(tMax <= tMin) after the three axes):
//     in_band: boxes whose three reciprocals satisfy the certificate's hypothesis |r d - 1| <= 3 * 2^-24 (the product of two
//     floats is exact in double); entered: boxes the reference enters; wrong: certified in-band boxes on which a form is
//     decided and its verdict is not the reference's; maybe_wrong: boxes (certified in-band ones and uncertified ones) on which
//     srtSlabMaybe<false> or <true> returns false while the reference's interval is not strictly empty (!(tMax < tMin));
//     max_ratio: over the certified in-band boxes with finite ends, the largest (|tMinA - tMin| + |tMaxA - tMax|) / tol in
//     double -- A: the clamped ends the verdict compares, tol: the verdict's own tolerance.  wrong and maybe_wrong must be 0
//     and max_ratio at most 1: what the header proves.
//     The reciprocal is drawn from the whole band of the hypothesis: fl(1 / d) moved outwards while the product stays inside
//     it, the two ends favoured.  The classes ulp2 and edges keep fl(1 / d) moved by -2 .. 2 ulps, as far as 5 * 2^-24: the
//     identity of the two forms holds for any r (the comparisons with the reference leave their out-of-band boxes out).  The
//     uncertified class also has 0, +-inf and NaN themselves.
//   srt_slab_probe replay <in> <out>
//     in: records of 18 words -- lo[3] hi[3] o[3] d[3] r[3] tMin tMax as float32 and an int32, the scene's fast-division word;
//     out: per record 8 words -- r[3], tolAbs of the min/max setup, tolAbs of the sign setup, an int32 of flags, tEnter of
//     srtSlabMaybe<false>, 0.  Flags: bit 0 certified, 1 / 2 verdict / undecided of srtSlabVerdict<false, false>, 3 / 4 of
//     <true, false>, 5 / 6 of <true, true>, 7 srtSlabMaybe<false>, 8 the reference's verdict as restated here, 10 the gate
//     form of the exact test on the same box (srtSlabExactOrGate, gate = true); 9 stays 0 (boxHitLoose is device code).  The
//     layout of srtTestSlabVisit (include/srt_hip_test.h), which runs the device compile of the same header on the same cases.
//   srt_slab_probe boxes
//     srtBoxOrdered (csrc/srt_records.h) on an ordered, a flat, an inverted and two non-finite boxes: `ordered <0|1>` each
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "srt_hip.h"
#include "srt_records.h"
#include "srt_slab.h"

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) * 0x1p-53; }  // [0, 1)
  double sym(double a) { return (2.0 * uni() - 1.0) * a; }   // (-a, a)
  int below(int n) { return (int)(next() % (uint64_t)n); }
  float sign() { return (next() & 1) ? 1.0f : -1.0f; }
  template <size_t N>
  float pick(const float (&v)[N]) { return v[below((int)N)]; }
};

struct Tally {
  const char* name;
  uint64_t boxes = 0, axes = 0, certified = 0, undecided = 0, endDiff = 0, verdictDiff = 0, undecidedDiff = 0, decidedUncertified = 0;
  uint64_t inBand = 0, entered = 0, wrong = 0, maybeWrong = 0;
  double maxRatio = 0.0;
};

bool sameValue(float a, float b) { return a == b || (std::isnan(a) && std::isnan(b)); }  // (-0 == +0: one value)

float ulps(float x, int k) {
  for (; k > 0; --k) x = nextafterf(x, INFINITY);
  for (; k < 0; ++k) x = nextafterf(x, -INFINITY);
  return x;
}

struct Case {
  float lo[3], hi[3], o[3], r[3], d[3], tMin, tMax;
};

// the hypothesis of the certificate on one reciprocal: |r d - 1| <= 3u, u = 2^-24 (two floats' product is exact in double)
bool inBand(float r, float d) { return fabs((double)r * (double)d - 1.0) <= 3.0 * 0x1p-24; }

// aabb.h:14-22 as the reference computes it; returns its verdict and leaves the interval after the three axes
bool reference(const Case& c, float& tMin, float& tMax) {
  tMin = c.tMin;
  tMax = c.tMax;
  for (int k = 0; k < 3; ++k) {
    const float a = (c.lo[k] - c.o[k]) / c.d[k], b = (c.hi[k] - c.o[k]) / c.d[k];
    tMin = fmaxf(fminf(a, b), tMin);
    tMax = fminf(fmaxf(a, b), tMax);
  }
  return !(tMax <= tMin);
}

// what the header makes of one case, as the kernels call it per ray and per visit
struct Eval {
  bool certified, va, ua, vt, ut, vb, ub, maybeA, maybeB;
  float tolAbs, tolAbs2, tEnterA, tEnterB;
  SrtSlab3 m, m2;
  SrtSlabEnds a, b;
};
Eval evaluate(const Case& c, bool certifiedScene) {
  Eval e;
  e.certified = certifiedScene & srtSlabOperandOk(c.o[0], c.d[0]) & srtSlabOperandOk(c.o[1], c.d[1]) & srtSlabOperandOk(c.o[2], c.d[2]);
  const SrtSlab3 o = {c.o[0], c.o[1], c.o[2]}, r = {c.r[0], c.r[1], c.r[2]};
  SrtSlab3 rp, rq;
  srtSlabSetup(o, r, e.certified, e.m, e.tolAbs);
  srtSlabSignSetup(o, r, e.certified, rp, rq, e.m2, e.tolAbs2);
  const float4 n0 = make_float4(c.lo[0], c.lo[1], c.lo[2], 0.0f), n1 = make_float4(c.hi[0], c.hi[1], c.hi[2], 0.0f);
  e.a = srtSlabEndsMinMax(n0, n1, r, e.m);
  e.b = srtSlabEndsSign(n0, n1, rp, rq, e.m2);
  e.va = srtSlabVerdict<false, false>(e.a, e.tolAbs, c.tMin, c.tMax, e.ua);
  e.vt = srtSlabVerdict<true, false>(e.a, e.tolAbs, c.tMin, c.tMax, e.ut);
  e.vb = srtSlabVerdict<true, true>(e.b, e.tolAbs2, c.tMin, c.tMax, e.ub);
  e.maybeA = srtSlabMaybe<false>(e.a, e.tolAbs, c.tMin, c.tMax, e.tEnterA);
  e.maybeB = srtSlabMaybe<true>(e.b, e.tolAbs2, c.tMin, c.tMax, e.tEnterB);
  return e;
}

void probe(const Case& c, Tally& y) {
  const Eval e = evaluate(c, true);
  const bool certified = e.certified;
  const SrtSlab3& m = e.m;
  const SrtSlabEnds &a = e.a, &b = e.b;
  const float tolAbs = e.tolAbs, tolAbs2 = e.tolAbs2;
  y.boxes++;
  y.axes += 3;
  y.certified += certified;
  if (certified) {
    // the min/max form's ends are min / max of the two quotients by construction; stated again here from the quotients
    const float qa[3] = {__builtin_fmaf(c.lo[0], c.r[0], m.x), __builtin_fmaf(c.lo[1], c.r[1], m.y), __builtin_fmaf(c.lo[2], c.r[2], m.z)};
    const float qb[3] = {__builtin_fmaf(c.hi[0], c.r[0], m.x), __builtin_fmaf(c.hi[1], c.r[1], m.y), __builtin_fmaf(c.hi[2], c.r[2], m.z)};
    const float nearB[3] = {b.a.x, b.a.y, b.a.z}, farB[3] = {b.b.x, b.b.y, b.b.z};
    const float nearA[3] = {srtSlabMin(a.a.x, a.b.x), srtSlabMin(a.a.y, a.b.y), srtSlabMin(a.a.z, a.b.z)};
    const float farA[3] = {srtSlabMax(a.a.x, a.b.x), srtSlabMax(a.a.y, a.b.y), srtSlabMax(a.a.z, a.b.z)};
    for (int k = 0; k < 3; ++k) {
      const float mn = qb[k] < qa[k] ? qb[k] : qa[k], mx = qb[k] > qa[k] ? qb[k] : qa[k];
      if (!sameValue(nearB[k], mn) || !sameValue(farB[k], mx) || !sameValue(nearA[k], mn) || !sameValue(farA[k], mx)) y.endDiff++;
    }
    if (tolAbs != tolAbs2) y.endDiff++;
  }
  // the two forms against each other: SrtSlabVerdict<false, false> and <false, true>, as before; the UNIFORM_TMIN instances are
  // the same functions on the host and must say the same
  bool ua, ub;
  const bool va = srtSlabVerdict<false, false>(a, tolAbs, c.tMin, c.tMax, ua), vb = srtSlabVerdict<false, true>(b, tolAbs2, c.tMin, c.tMax, ub);
  y.undecided += ua;
  if (va != vb || va != e.vt || vb != e.vb) y.verdictDiff++;
  if (ua != ub || ua != e.ut || ub != e.ub) y.undecidedDiff++;
  if (!certified && (!ua || !ub || va || vb)) y.decidedUncertified++;
  // ... and against the reference
  float tMinR, tMaxR;
  const bool vr = reference(c, tMinR, tMaxR);
  y.entered += vr;
  const bool band = inBand(c.r[0], c.d[0]) & inBand(c.r[1], c.d[1]) & inBand(c.r[2], c.d[2]);
  y.inBand += band;
  if (certified && !band) return;  // outside the hypothesis (the +-2 ulp classes): nothing is claimed
  if (!(tMaxR < tMinR) && (!e.maybeA || !e.maybeB)) y.maybeWrong++;
  if (!certified) return;
  if ((!ua && va != vr) || (!ub && vb != vr)) y.wrong++;
  for (int form = 0; form < 2; ++form) {
    // the clamped ends and the tolerance srtSlabVerdict compares, from the header's own pieces
    const float tMinA = srtSlabMax(form ? srtSlabNear<true>(b) : srtSlabNear<false>(a), c.tMin);
    const float tMaxA = srtSlabMin(form ? srtSlabFar<true>(b) : srtSlabFar<false>(a), c.tMax);
    const float tol = __builtin_fmaf(SRT_SLAB_EPS, fabsf(tMaxA) + fabsf(tMinA), form ? tolAbs2 : tolAbs);
    if (!std::isfinite(tMinA) || !std::isfinite(tMaxA) || !std::isfinite(tMinR) || !std::isfinite(tMaxR) || !(tol > 0.0f)) continue;
    const double ratio = (fabs((double)tMinA - (double)tMinR) + fabs((double)tMaxA - (double)tMaxR)) / (double)tol;
    if (ratio > y.maxRatio) y.maxRatio = ratio;
  }
}

void print(const Tally& y) {
  printf("class %s boxes %llu axes %llu certified %llu undecided %llu end_diff %llu verdict_diff %llu undecided_diff %llu decided_uncertified %llu", y.name,
         (unsigned long long)y.boxes, (unsigned long long)y.axes, (unsigned long long)y.certified, (unsigned long long)y.undecided,
         (unsigned long long)y.endDiff, (unsigned long long)y.verdictDiff, (unsigned long long)y.undecidedDiff, (unsigned long long)y.decidedUncertified);
  printf(" in_band %llu entered %llu wrong %llu maybe_wrong %llu max_ratio %.6f\n", (unsigned long long)y.inBand, (unsigned long long)y.entered,
         (unsigned long long)y.wrong, (unsigned long long)y.maybeWrong, y.maxRatio);
}

// an ordered pair of plane coordinates from two draws
void order(float a, float b, float& lo, float& hi) {
  lo = a <= b ? a : b;
  hi = a <= b ? b : a;
}
// |d| log-uniform over the certified range [2^-20, 2^20], either sign
float direction(Rng& g) { return g.sign() * (float)exp2(g.sym(20.0)); }
// fl(1 / d) moved by -2 .. 2 ulps: the classes ulp2 and edges
void reciprocalUlps(Rng& g, Case& c) {
  for (int k = 0; k < 3; ++k) c.r[k] = ulps(1.0f / c.d[k], g.below(5) - 2);
}
// a reciprocal from the whole band |r d - 1| <= 3u: fl(1 / d) moved outwards while the product stays inside; three draws in
// eight take the upper end, three the lower end, two any float between them
float bandReciprocal(Rng& g, float d) {
  const float r0 = 1.0f / d;
  if (!inBand(r0, d)) return r0;  // (d = 0, infinite, NaN or denormal: the uncertified class)
  int up = 0, down = 0;
  while (up < 8 && inBand(ulps(r0, up + 1), d)) ++up;
  while (down > -8 && inBand(ulps(r0, down - 1), d)) --down;
  const int how = g.below(8);
  return ulps(r0, how < 3 ? up : how < 6 ? down : down + g.below(up - down + 1));
}
void reciprocal(Rng& g, Case& c) {
  for (int k = 0; k < 3; ++k) c.r[k] = bandReciprocal(g, c.d[k]);
}
void interval(Rng& g, Case& c) {
  c.tMin = 0.001f;
  c.tMax = (g.next() & 3) ? INFINITY : (float)exp2(g.sym(12.0));
}
// the origin moved so that the ray meets a point of the box (plane coordinates clipped to [-bound, bound]) at parameter t; an
// origin component that falls outside the certified range becomes 0
void aimInside(Rng& g, Case& c, double t, double bound = 0x1p40) {
  for (int k = 0; k < 3; ++k) {
    const double lo = fmax((double)c.lo[k], -bound), hi = fmin((double)c.hi[k], bound);
    const double p = lo <= hi ? lo + g.uni() * (hi - lo) : (double)c.lo[k];
    c.o[k] = (float)(p - t * (double)c.d[k]);
    if (!srtSlabOperandOk(c.o[k], c.d[k])) c.o[k] = 0.0f;
  }
}
// ... or the direction: d = (p - o) / t, kept where it is inside the certified range
void aimDirection(Rng& g, Case& c, double t) {
  for (int k = 0; k < 3; ++k) {
    const double p = (double)c.lo[k] + g.uni() * ((double)c.hi[k] - (double)c.lo[k]);
    const float d = (float)((p - (double)c.o[k]) / t);
    if (srtSlabOperandOk(c.o[k], d)) c.d[k] = d;
  }
}

const float GROUND[] = {0.0f, -0.0f, 1000.0f, -1000.0f, -2000.0f};
const float ZEROS[] = {0.0f, -0.0f, 1.0f, -1.0f, 0x1p-77f, -0x1p-77f, 0x1p30f, -0x1p30f, 0.5f, -3.25f};
const float ORIGINS[] = {0.0f, -0.0f, 0x1p30f, -0x1p30f, 0x1p-77f, -0x1p-77f, 1.0f, -13.0f};
const float DIRS[] = {0x1p-20f, -0x1p-20f, 0x1p20f, -0x1p20f, 1.0f, -1.0f};

void sweep(uint64_t seed, uint64_t per) {
  Rng g{seed};
  Tally random{"random"}, zeros{"zeros"}, flat{"flat"}, ground{"ground"}, dEdges{"d_edges"}, oEdges{"o_edges"}, aimed{"aimed"}, uncert{"uncertified"}, edges{"edges"};
  Tally far{"far"}, touch{"touch"}, tminZero{"tmin_zero"}, ulp2{"ulp2"};
  Case c;
  for (uint64_t i = 0; i < per; ++i) {
    // random: boxes of every size near and far from the origin; half of the rays go through a point of the box
    const double scale = exp2(g.sym(10.0));
    for (int k = 0; k < 3; ++k) {
      order((float)g.sym(scale), (float)g.sym(scale), c.lo[k], c.hi[k]);
      c.o[k] = (float)g.sym(4.0 * scale);
      c.d[k] = direction(g);
    }
    if (i & 1) {  // (directions of moderate slope: the three axes' intervals overlap by far more than the tolerance)
      for (int k = 0; k < 3; ++k) c.d[k] = g.sign() * (float)exp2(g.sym(3.0));
      aimInside(g, c, scale * (exp2(g.sym(4.0)) + 1.0));
    }
    reciprocal(g, c);
    interval(g, c);
    probe(c, random);
    // ulp2: the same boxes and rays with fl(1 / d) moved by -2 .. 2 ulps, for the identity of the two forms
    reciprocalUlps(g, c);
    probe(c, ulp2);
    // zeros: planes at coordinate 0 of either sign and at the ends of the certified range
    for (int k = 0; k < 3; ++k) {
      order(g.pick(ZEROS), g.pick(ZEROS), c.lo[k], c.hi[k]);
      if (c.lo[k] == c.hi[k] && (g.next() & 1)) {  // (order() cannot tell -0 from +0: both orders of the two zeros)
        const float t = c.lo[k];
        c.lo[k] = c.hi[k];
        c.hi[k] = t;
      }
      c.o[k] = (g.next() & 1) ? (float)g.sym(8.0) : g.pick(ORIGINS);
      c.d[k] = direction(g);
    }
    if (i & 1) {  // through a point of the box no further out than 8
      for (int k = 0; k < 3; ++k) c.d[k] = g.sign() * (float)exp2(g.sym(3.0));
      aimInside(g, c, exp2(g.sym(4.0)) + 1.0, 8.0);
    }
    reciprocal(g, c);
    interval(g, c);
    probe(c, zeros);
    // flat: n0 == n1 on one, two or three axes
    for (int k = 0; k < 3; ++k) {
      order((float)g.sym(50.0), (float)g.sym(50.0), c.lo[k], c.hi[k]);
      if (k == 0 || (g.next() & 1)) c.hi[k] = c.lo[k];
      c.o[k] = (float)g.sym(100.0);
      c.d[k] = direction(g);
    }
    reciprocal(g, c);
    interval(g, c);
    probe(c, flat);
    // ground: the big sphere's box, coordinates +-1000 and -2000, seen from near its top
    for (int k = 0; k < 3; ++k) {
      order(g.pick(GROUND), g.pick(GROUND), c.lo[k], c.hi[k]);
      c.o[k] = (float)g.sym(30.0);
      c.d[k] = g.sign() * (float)exp2(g.sym(3.0));
    }
    if (i & 1) aimInside(g, c, exp2(g.sym(4.0)) + 1.0);
    reciprocal(g, c);
    interval(g, c);
    probe(c, ground);
    // d_edges: |d| at 2^-20 and 2^20
    for (int k = 0; k < 3; ++k) {
      order((float)g.sym(6.0), (float)g.sym(6.0), c.lo[k], c.hi[k]);
      c.o[k] = (float)g.sym(6.0);
      c.d[k] = (g.next() & 3) ? g.pick(DIRS) : direction(g);
    }
    if (i & 1) aimInside(g, c, exp2(g.sym(4.0)) + 1.0);
    reciprocal(g, c);
    interval(g, c);
    probe(c, dEdges);
    // o_edges: o = 0 and |o| = 2^30
    for (int k = 0; k < 3; ++k) {
      order((float)g.sym(2000.0), (float)g.sym(2000.0), c.lo[k], c.hi[k]);
      c.o[k] = g.pick(ORIGINS);
      c.d[k] = direction(g);
    }
    if (i & 1) aimDirection(g, c, 0x1p11 * (1.0 + g.uni()));  // (|d| = 2^30 / t stays below 2^20)
    reciprocal(g, c);
    interval(g, c);
    probe(c, oEdges);
    // aimed: the ray passes within a few ulps of a box corner or edge, where the certificate cannot decide
    {
      float p[3];
      double t = exp2(g.sym(4.0)) + 1.0;
      for (int k = 0; k < 3; ++k) {
        order((float)g.sym(5.0), (float)g.sym(5.0), c.lo[k], c.hi[k]);
        p[k] = (g.next() & 1) ? c.lo[k] : c.hi[k];
        c.d[k] = g.sign() * (float)exp2(g.sym(2.0));
        c.o[k] = ulps((float)((double)p[k] - t * (double)c.d[k]), g.below(5) - 2);
      }
      reciprocal(g, c);
      interval(g, c);
      probe(c, aimed);
    }
    // uncertified: a direction or origin component outside the ranges, a zero, infinite or NaN reciprocal
    {
      static const float BAD_D[] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, 0x1p-21f, -0x1p21f, 0x1p-130f, 0x1p-127f};
      static const float BAD_R[] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN};
      for (int k = 0; k < 3; ++k) {
        order((float)g.sym(6.0), (float)g.sym(6.0), c.lo[k], c.hi[k]);
        c.o[k] = (float)g.sym(6.0);
        c.d[k] = direction(g);
      }
      reciprocal(g, c);
      const int k = g.below(3), how = g.below(3);
      if (how == 0) {
        c.d[k] = g.pick(BAD_D);
        c.r[k] = (g.next() & 1) ? 1.0f / c.d[k] : g.pick(BAD_R);  // (the device's Newton step makes a NaN of 1 / 0)
      } else if (how == 1) {
        c.o[k] = g.sign() * ((g.next() & 1) ? 0x1p31f : 0x1p-80f);
      } else {
        c.o[k] = (g.next() & 1) ? NAN : g.sign() * INFINITY;
      }
      interval(g, c);
      probe(c, uncert);
    }
    // far: |o| from 2^10 to 2^30 and the box near zero, so the absolute part K of the tolerance dominates; three rays in
    // four are aimed at a point of the box
    {
      double big = 0.0;
      for (int k = 0; k < 3; ++k) {
        order((float)g.sym(4.0), (float)g.sym(4.0), c.lo[k], c.hi[k]);
        c.o[k] = g.sign() * (float)exp2(10.0 + 20.0 * g.uni());
        c.d[k] = direction(g);
        big = fmax(big, fabs((double)c.o[k]));
      }
      if (i & 3) aimDirection(g, c, big * exp2(-19.0 * g.uni()));  // (|d| <= 2^20 on the largest axis, >= 2^-20 on the smallest)
      reciprocal(g, c);
      interval(g, c);
      if (i & 3) c.tMax = INFINITY;
      probe(c, far);
    }
    // touch: tMax, tMin or both within 4 ulps of one of the box's own quotients on one axis, the other two axes open around
    // it -- `closest` after a hit on a primitive that lies in a box face
    {
      const int axis = g.below(3);
      const double t = exp2(g.sym(4.0)) + 1.0;
      for (int k = 0; k < 3; ++k) {
        const double half = k == axis ? 5.0 : 100.0;
        order((float)g.sym(half), (float)g.sym(half), c.lo[k], c.hi[k]);
        if (k != axis) c.lo[k] = (float)(-half - g.uni()), c.hi[k] = (float)(half + g.uni());
        c.d[k] = g.sign() * (float)exp2(k == axis ? 2.0 + 2.0 * g.uni() : -2.0 * g.uni());
      }
      aimInside(g, c, t, 5.0);
      reciprocal(g, c);
      const float qa = (c.lo[axis] - c.o[axis]) / c.d[axis], qb = (c.hi[axis] - c.o[axis]) / c.d[axis];
      const float qNear = fminf(qa, qb), qFar = fmaxf(qa, qb);
      const int how = g.below(4);
      c.tMin = 0.001f;
      c.tMax = INFINITY;
      if (how == 0) c.tMax = ulps((g.next() & 1) ? qNear : qFar, g.below(9) - 4);
      if (how == 1) c.tMin = ulps((g.next() & 1) ? qNear : qFar, g.below(9) - 4);
      if (how == 2) c.tMin = ulps(qNear, g.below(9) - 4), c.tMax = ulps(qFar, g.below(9) - 4);
      if (how == 3) c.tMin = ulps(qFar, g.below(9) - 4), c.tMax = ulps(qFar, g.below(9) - 4);
      probe(c, touch);
    }
    // tmin_zero: the caller's tMin at 0 and far along the ray
    {
      const bool zero = i & 1;
      const float tMin = zero ? 0.0f : 64.0f * (float)exp2(g.sym(3.0));
      for (int k = 0; k < 3; ++k) {
        order((float)g.sym(5.0), (float)g.sym(5.0), c.lo[k], c.hi[k]);
        c.o[k] = (float)g.sym(20.0);
        c.d[k] = g.sign() * (float)exp2(g.sym(4.0));
      }
      if (i & 2) aimInside(g, c, zero ? exp2(g.sym(4.0)) : (double)tMin * exp2(g.sym(1.0)));
      reciprocal(g, c);
      interval(g, c);
      c.tMin = tMin;
      if (!zero) c.tMax = (g.next() & 1) ? INFINITY : tMin * (float)exp2(2.0 * g.uni());
      probe(c, tminZero);
    }
  }
  // edges: every combination of the listed coordinates on one axis (the other two axes wide open around the ray)
  static const float PLANES[] = {0.0f, -0.0f, 1000.0f, -1000.0f, -2000.0f, 1.0f, -1.0f, 0x1p-77f, -0x1p-77f, 0x1p30f, -0x1p30f};
  for (float pa : PLANES)
    for (float pb : PLANES)
      for (float oo : ORIGINS)
        for (float dd : DIRS)
          for (int du = -2; du <= 2; ++du) {
            if (!(pa <= pb)) continue;  // (both orders of the two zeros pass)
            for (int k = 0; k < 3; ++k) {
              c.lo[k] = -0x1p29f;
              c.hi[k] = 0x1p29f;
              c.o[k] = 0.0f;
              c.d[k] = 1.0f;
              c.r[k] = 1.0f;
            }
            const int k = (int)(edges.boxes % 3);
            c.lo[k] = pa;
            c.hi[k] = pb;
            c.o[k] = oo;
            c.d[k] = dd;
            c.r[k] = ulps(1.0f / dd, du);
            c.tMin = 0.001f;
            c.tMax = INFINITY;
            probe(c, edges);
          }
  for (const Tally* y : {&random, &zeros, &flat, &ground, &dEdges, &oEdges, &aimed, &uncert, &edges, &far, &touch, &tminZero, &ulp2}) print(*y);
}

// replay: caller-made cases with the caller's reciprocals (the device's own, tests/test_gpu_slab_cert.py) through the host compile
int replay(const char* inPath, const char* outPath) {
  FILE* in = fopen(inPath, "rb");
  if (!in) return 1;
  FILE* out = fopen(outPath, "wb");
  if (!out) {
    fclose(in);
    return 1;
  }
  struct Record {
    float lo[3], hi[3], o[3], d[3], r[3], tMin, tMax;
    int32_t certifiedScene;
  } rec;
  static_assert(sizeof(Record) == 72, "18 words");
  while (fread(&rec, sizeof rec, 1, in) == 1) {
    Case c;
    memcpy(c.lo, rec.lo, sizeof c.lo);
    memcpy(c.hi, rec.hi, sizeof c.hi);
    memcpy(c.o, rec.o, sizeof c.o);
    memcpy(c.d, rec.d, sizeof c.d);
    memcpy(c.r, rec.r, sizeof c.r);
    c.tMin = rec.tMin;
    c.tMax = rec.tMax;
    const Eval e = evaluate(c, rec.certifiedScene != 0);
    float tMinR, tMaxR;
    const bool vr = reference(c, tMinR, tMaxR);
    const bool gate = srtSlabExactOrGate(make_float4(c.lo[0], c.lo[1], c.lo[2], 0.0f), make_float4(c.hi[0], c.hi[1], c.hi[2], 0.0f),
                                         SrtSlab3{c.o[0], c.o[1], c.o[2]}, SrtSlab3{c.d[0], c.d[1], c.d[2]}, c.tMin, c.tMax, true);
    const int32_t flags = (int32_t)e.certified | e.va << 1 | e.ua << 2 | e.vt << 3 | e.ut << 4 | e.vb << 5 | e.ub << 6 | e.maybeA << 7 | vr << 8 | gate << 10;
    float w[8] = {c.r[0], c.r[1], c.r[2], e.tolAbs, e.tolAbs2, 0.0f, e.tEnterA, 0.0f};
    memcpy(&w[5], &flags, 4);
    if (fwrite(w, sizeof w, 1, out) != 1) break;
  }
  const bool bad = ferror(in) || ferror(out);
  fclose(in);
  return (fclose(out) != 0 || bad) ? 1 : 0;
}

void boxes() {
  const Box list[] = {{{-1.0f, 0.0f, 2.0f}, {1.0f, 0.5f, 3.0f}},             // ordered
                      {{-1.0f, 0.25f, -0.0f}, {1.0f, 0.25f, 0.0f}},          // flat (and the two zeros)
                      {{-1.0f, 0.5f, 2.0f}, {1.0f, 0.25f, 3.0f}},            // inverted on y
                      {{-1.0f, 0.0f, 2.0f}, {INFINITY, 0.5f, 3.0f}},         // not finite
                      {{-1.0f, NAN, 2.0f}, {1.0f, 0.5f, 3.0f}}};
  for (const Box& b : list) printf("ordered %d\n", srtBoxOrdered(b) ? 1 : 0);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "sweep")) {
    sweep(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "boxes")) {
    boxes();
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "replay")) return replay(argv[2], argv[3]);
  fprintf(stderr, "usage: srt_slab_probe sweep <seed> <boxes per class> | replay <in> <out> | boxes\n");
  return 2;
}
