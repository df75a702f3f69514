// The certified slab test of csrc/srt_slab.h as a stand-alone host program (no GPU, no library): used by
// tests/test_slab_host.py, and the place for a sanitizer build of that header.
//   srt_slab_probe sweep <seed> <boxes per class>
//     seeded (ordered box, origin, direction, tMin, tMax) cases, class by class, three axis cases per box; per class one line
//       class <name> boxes <n> axes <n> certified <n> undecided <n> end_diff <n> verdict_diff <n> undecided_diff <n> decided_uncertified <n>
//     certified: boxes whose ray is inside srtSlabOperandOk's ranges on all three axes (the others get tolAbs = +inf);
//     undecided: boxes the min/max form leaves to the exact test; end_diff: axis cases whose sign-form near / far differ AS
//     FLOAT VALUES from min / max of the two one-FMA quotients (a NaN equals a NaN; certified rays only -- on the others the
//     verdict below is what counts); verdict_diff, undecided_diff: boxes on which the two forms' verdict / undecided differ;
//     decided_uncertified: uncertified boxes either form decides.  The last four must be 0.
//     The reciprocal is fl(1 / d) moved by -2 .. 2 ulps (the device's refined reciprocal is within 1.5 ulp of 1 / d; the
//     identity holds for any r), and for the uncertified class also 0, +-inf and NaN themselves.
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

void probe(const Case& c, Tally& y) {
  const bool certified = srtSlabOperandOk(c.o[0], c.d[0]) & srtSlabOperandOk(c.o[1], c.d[1]) & srtSlabOperandOk(c.o[2], c.d[2]);
  const SrtSlab3 o = {c.o[0], c.o[1], c.o[2]}, r = {c.r[0], c.r[1], c.r[2]};
  SrtSlab3 m, m2, rp, rq;
  float tolAbs, tolAbs2;
  srtSlabSetup(o, r, certified, m, tolAbs);
  srtSlabSignSetup(o, r, certified, rp, rq, m2, tolAbs2);
  const float4 n0 = make_float4(c.lo[0], c.lo[1], c.lo[2], 0.0f), n1 = make_float4(c.hi[0], c.hi[1], c.hi[2], 0.0f);
  const SrtSlabEnds a = srtSlabEndsMinMax(n0, n1, r, m), b = srtSlabEndsSign(n0, n1, rp, rq, m2);
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
  bool ua, ub;
  const bool va = srtSlabVerdict<false, false>(a, tolAbs, c.tMin, c.tMax, ua), vb = srtSlabVerdict<false, true>(b, tolAbs2, c.tMin, c.tMax, ub);
  y.undecided += ua;
  if (va != vb) y.verdictDiff++;
  if (ua != ub) y.undecidedDiff++;
  if (!certified && (!ua || !ub || va || vb)) y.decidedUncertified++;
}

void print(const Tally& y) {
  printf("class %s boxes %llu axes %llu certified %llu undecided %llu end_diff %llu verdict_diff %llu undecided_diff %llu decided_uncertified %llu\n", y.name,
         (unsigned long long)y.boxes, (unsigned long long)y.axes, (unsigned long long)y.certified, (unsigned long long)y.undecided,
         (unsigned long long)y.endDiff, (unsigned long long)y.verdictDiff, (unsigned long long)y.undecidedDiff, (unsigned long long)y.decidedUncertified);
}

// an ordered pair of plane coordinates from two draws
void order(float a, float b, float& lo, float& hi) {
  lo = a <= b ? a : b;
  hi = a <= b ? b : a;
}
// |d| log-uniform over the certified range [2^-20, 2^20], either sign
float direction(Rng& g) { return g.sign() * (float)exp2(g.sym(20.0)); }
void reciprocal(Rng& g, Case& c) {
  for (int k = 0; k < 3; ++k) c.r[k] = ulps(1.0f / c.d[k], g.below(5) - 2);
}
void interval(Rng& g, Case& c) {
  c.tMin = 0.001f;
  c.tMax = (g.next() & 3) ? INFINITY : (float)exp2(g.sym(12.0));
}

const float GROUND[] = {0.0f, -0.0f, 1000.0f, -1000.0f, -2000.0f};
const float ZEROS[] = {0.0f, -0.0f, 1.0f, -1.0f, 0x1p-77f, -0x1p-77f, 0x1p30f, -0x1p30f, 0.5f, -3.25f};
const float ORIGINS[] = {0.0f, -0.0f, 0x1p30f, -0x1p30f, 0x1p-77f, -0x1p-77f, 1.0f, -13.0f};
const float DIRS[] = {0x1p-20f, -0x1p-20f, 0x1p20f, -0x1p20f, 1.0f, -1.0f};

void sweep(uint64_t seed, uint64_t per) {
  Rng g{seed};
  Tally random{"random"}, zeros{"zeros"}, flat{"flat"}, ground{"ground"}, dEdges{"d_edges"}, oEdges{"o_edges"}, aimed{"aimed"}, uncert{"uncertified"}, edges{"edges"};
  Case c;
  for (uint64_t i = 0; i < per; ++i) {
    // random: boxes of every size near and far from the origin
    const double scale = exp2(g.sym(10.0));
    for (int k = 0; k < 3; ++k) {
      order((float)g.sym(scale), (float)g.sym(scale), c.lo[k], c.hi[k]);
      c.o[k] = (float)g.sym(4.0 * scale);
      c.d[k] = direction(g);
    }
    reciprocal(g, c);
    interval(g, c);
    probe(c, random);
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
    reciprocal(g, c);
    interval(g, c);
    probe(c, ground);
    // d_edges: |d| at 2^-20 and 2^20
    for (int k = 0; k < 3; ++k) {
      order((float)g.sym(6.0), (float)g.sym(6.0), c.lo[k], c.hi[k]);
      c.o[k] = (float)g.sym(6.0);
      c.d[k] = (g.next() & 3) ? g.pick(DIRS) : direction(g);
    }
    reciprocal(g, c);
    interval(g, c);
    probe(c, dEdges);
    // o_edges: o = 0 and |o| = 2^30
    for (int k = 0; k < 3; ++k) {
      order((float)g.sym(2000.0), (float)g.sym(2000.0), c.lo[k], c.hi[k]);
      c.o[k] = g.pick(ORIGINS);
      c.d[k] = direction(g);
    }
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
  for (const Tally* y : {&random, &zeros, &flat, &ground, &dEdges, &oEdges, &aimed, &uncert, &edges}) print(*y);
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
  fprintf(stderr, "usage: srt_slab_probe sweep <seed> <boxes per class> | boxes\n");
  return 2;
}
