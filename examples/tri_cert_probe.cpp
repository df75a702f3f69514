// The triangle tests of csrc/srt_tri_hit.h as a stand-alone host program (no GPU, no library): used by
// tests/test_tri_cert_host.py, and the place for a sanitizer build of that header.
//   srt_tri_cert_probe sweep <seed> <pairs per class>
//     seeded (triangle, ray) pairs, class by class; per class one line
//       class <name> pairs <n> plane_ok <n> undecided <n> diff <n> t_diff <n> max_ratio <x>
//     plane_ok: pairs whose plane conditions passed (only those ask the edges); undecided: of those, left to the exact
//     test; diff: DECIDED verdicts that differ from srtTriHitExact<false> (must be 0); t_diff: pairs whose t differs in bits
//     (must be 0); max_ratio: the largest |cheap - exact edge value| / (u N E (W + E)) over the finite ones (the header
//     proves 64).
//   srt_tri_cert_probe exact <in.bin> <out.bin>
//     in: 9 floats (one triangle), int32 n, n x { o[3], d[3], tMin }.  out: n x { int32 hit, float t, int32 certified
//     verdict, int32 undecided }: srtTriHitExact<false> and srtTriHitCert on the records triangleRecords makes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "srt_hip.h"
#include "srt_records.h"

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) * 0x1p-53; }            // [0, 1)
  double sym(double a) { return (2.0 * uni() - 1.0) * a; }             // (-a, a)
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Tri {
  float p[9];
  float4 test[3], fast[SRT_TRI_FAST_SLOTS];
  void make() {
    const float uv[6] = {0, 0, 1, 0, 0, 1};
    float4 shade[4];
    triangleRecords(p, uv, 0.0f, test, shade, fast);
  }
};

struct Tally {
  const char* name;
  uint64_t pairs = 0, planeOk = 0, undecided = 0, diff = 0, tDiff = 0;
  double maxRatio = 0;
};

uint32_t bits(float x) {
  uint32_t b;
  memcpy(&b, &x, 4);
  return b;
}

void probe(const Tri& tr, const SrtTriRay& r, float tMin, Tally& y) {
  float tE = 0, tC = 0, dbg[4];
  bool undecided;
  const bool exact = srtTriHitExact<false>(tr.test[0], tr.test[1], tr.test[2], r, tMin, 0.0f, tE);
  const bool cert = srtTriHitCert(tr.fast[0], tr.fast[1], tr.fast[2], tr.fast[3], r, tMin, SRT_TRI_W_MAX, tC, undecided, dbg);
  y.pairs++;
  if (bits(tE) != bits(tC)) y.tDiff++;
  if (dbg[3] == 0.0f) {  // the plane conditions failed: both say "miss", nobody asks the edges
    if (exact || cert || undecided) y.diff++;
    return;
  }
  y.planeOk++;
  if (undecided) {
    y.undecided++;
  } else if (exact != cert) {
    y.diff++;
  }
  // the edge values as the exact test computes them, against the cheap ones
  const float* v[3] = {&tr.test[0].x, &tr.test[1].x, &tr.test[2].x};
  const float n[3] = {tr.test[0].w, tr.test[1].w, tr.test[2].w};
  const float p[3] = {r.ox + tE * r.dx, r.oy + tE * r.dy, r.oz + tE * r.dz};
  double N = 0, E = 0, W = 0;
  for (int c = 0; c < 3; ++c) {
    N = fmax(N, fabs((double)n[c]));
    W += fabs((double)(p[c] - v[0][c]));
    for (int i = 0; i < 3; ++i) E = fmax(E, fabs((double)(v[(i + 1) % 3][c] - v[i][c])));
  }
  const double unit = 0x1p-24 * N * E * (W + E);
  if (!(unit > 0) || !std::isfinite(unit)) return;
  for (int i = 0; i < 3; ++i) {
    const float* a = v[i];
    const float* b = v[(i + 1) % 3];
    const float s = srtTriEdge(n[0], n[1], n[2], b[0] - a[0], b[1] - a[1], b[2] - a[2], p[0] - a[0], p[1] - a[1], p[2] - a[2]);
    const double ratio = fabs((double)s - (double)dbg[i]) / unit;
    if (std::isfinite(ratio) && std::isfinite(tr.fast[2].w) && ratio > y.maxRatio) y.maxRatio = ratio;
  }
}

// a triangle of edge length ~size around a centre within +-offset
Tri randomTri(Rng& g, double size, double offset) {
  Tri t;
  const double c[3] = {g.sym(offset), g.sym(offset), g.sym(offset)};
  for (int k = 0; k < 9; ++k) t.p[k] = (float)(c[k % 3] + g.sym(size));
  t.make();
  return t;
}

// a ray from `o` through `target`, its direction scaled to a length in [0.25, 4)
SrtTriRay through(Rng& g, const double* o, const double* target) {
  double d[3] = {target[0] - o[0], target[1] - o[1], target[2] - o[2]};
  const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const double s = len > 0 ? (0.25 + 3.75 * g.uni()) / len : 1.0;
  return SrtTriRay{(float)o[0], (float)o[1], (float)o[2], (float)(d[0] * s), (float)(d[1] * s), (float)(d[2] * s)};
}

// a point a v0 + b v1 + c v2 of the triangle's plane (double; the caller rounds)
void bary(const Tri& t, double a, double b, double c, double* out) {
  for (int k = 0; k < 3; ++k) out[k] = a * t.p[k] + b * t.p[3 + k] + c * t.p[6 + k];
}

// an origin on the side the normal points to (front face), `dist` away from the triangle's surroundings
void frontOrigin(Rng& g, const Tri& t, double dist, double* o) {
  double c[3];
  bary(t, 1.0 / 3, 1.0 / 3, 1.0 / 3, c);
  const double n[3] = {t.test[0].w, t.test[1].w, t.test[2].w};
  const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  for (int k = 0; k < 3; ++k) o[k] = c[k] + (len > 0 ? n[k] / len : 0.0) * dist * (0.2 + g.uni()) + g.sym(dist * 0.7);
}

const double kSizes[3] = {1e-3, 0.08, 1.0};

}  // namespace

static int sweep(uint64_t seed, int per) {
  Rng g{seed};
  std::vector<Tally> all;
  const int raysPerTri = 16;
  auto run = [&](const char* name, auto makeTri, auto makeRay) {
    Tally y;
    y.name = name;
    for (int i = 0; i < per; i += raysPerTri) {
      const Tri t = makeTri();
      for (int k = 0; k < raysPerTri; ++k) {
        float tMin = 0.001f;
        const SrtTriRay r = makeRay(t, tMin);
        probe(t, r, tMin, y);
      }
    }
    all.push_back(y);
  };
  auto boxTri = [&]() { return randomTri(g, kSizes[g.below(3)], 6.0); };
  // random rays in and around the triangle
  run("random", boxTri, [&](const Tri& t, float&) {
    double o[3] = {g.sym(6), g.sym(6), g.sym(6)}, q[3];
    const double a = -0.5 + 2.0 * g.uni(), b = -0.5 + 2.0 * g.uni();
    bary(t, 1 - a - b, a, b, q);
    return through(g, o, q);
  });
  // rays aimed at float points on an edge
  run("edge", boxTri, [&](const Tri& t, float&) {
    double o[3], q[3];
    frontOrigin(g, t, 3.0, o);
    const int e = g.below(3);
    const double s = g.uni();
    const double w[3] = {e == 0 ? 1 - s : (e == 2 ? s : 0), e == 0 ? s : (e == 1 ? 1 - s : 0), e == 1 ? s : (e == 2 ? 1 - s : 0)};
    bary(t, w[0], w[1], w[2], q);
    for (int k = 0; k < 3; ++k) q[k] = (double)(float)q[k];
    return through(g, o, q);
  });
  // rays aimed at a vertex
  run("vertex", boxTri, [&](const Tri& t, float&) {
    double o[3];
    frontOrigin(g, t, 3.0, o);
    const int v = g.below(3);
    const double q[3] = {t.p[3 * v], t.p[3 * v + 1], t.p[3 * v + 2]};
    return through(g, o, q);
  });
  // origins on the triangle's plane (tMin 0 for half of them: t ~ 0 passes)
  run("plane_origin", boxTri, [&](const Tri& t, float& tMin) {
    double o[3], q[3];
    bary(t, g.sym(1.5), g.sym(1.5), g.sym(1.5), q);
    const double a = -0.5 + 2.0 * g.uni(), b = -0.5 + 2.0 * g.uni();
    bary(t, 1 - a - b, a, b, o);
    for (int k = 0; k < 3; ++k) q[k] += g.sym(1.0);
    if (g.below(2)) tMin = (g.below(2) ? 0.0f : -1.0f);
    return through(g, o, q);
  });
  // |n . d| around FLT_EPSILON: an in-plane direction plus a little of the normal
  run("grazing", boxTri, [&](const Tri& t, float&) {
    double o[3], u[3], q[3];
    frontOrigin(g, t, 1.0, o);
    bary(t, g.sym(1), g.sym(1), 0, u);
    bary(t, 0, 0, 0, q);
    const double n[3] = {t.test[0].w, t.test[1].w, t.test[2].w};
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    double e1[3] = {t.p[3] - t.p[0], t.p[4] - t.p[1], t.p[5] - t.p[2]};
    const double want = -1.1920928955078125e-07 * (0.25 + 3.0 * g.uni()) * (g.below(8) ? 1.0 : -1.0);  // n . d
    double d[3];
    for (int k = 0; k < 3; ++k) d[k] = e1[k] * g.sym(4) + (nn > 0 ? n[k] * want / nn : 0.0);
    return SrtTriRay{(float)o[0], (float)o[1], (float)o[2], (float)d[0], (float)d[1], (float)d[2]};
  });
  // sizes 2^-40 .. 2^20 at offsets up to 2^20, rays aimed in and around and at edges
  run("scales", [&]() { return randomTri(g, ldexp(1.0, -40 + g.below(61)), g.below(4) ? ldexp(1.0, -20 + g.below(41)) : 0.0); },
      [&](const Tri& t, float&) {
        double o[3], q[3], c[3];
        bary(t, 1.0 / 3, 1.0 / 3, 1.0 / 3, c);
        const double far = fabs(c[0]) + fabs(c[1]) + fabs(c[2]) + fabs((double)t.p[0] - t.p[3]) + 1e-12;
        frontOrigin(g, t, far * ldexp(1.0, g.below(8) - 2), o);
        const double a = -0.25 + 1.5 * g.uni(), b = g.below(4) ? -0.25 + 1.5 * g.uni() : 0.0;
        bary(t, 1 - a - b, a, b, q);
        return through(g, o, q);
      });
  // collinear and repeated vertices
  run("degenerate",
      [&]() {
        Tri t = randomTri(g, kSizes[g.below(3)], 6.0);
        const int kind = g.below(3);
        if (kind == 0) memcpy(t.p + 3, t.p, 12);                                         // v1 == v0
        if (kind == 1) { memcpy(t.p + 3, t.p, 12); memcpy(t.p + 6, t.p, 12); }           // one point
        if (kind == 2) for (int k = 0; k < 3; ++k) t.p[6 + k] = t.p[k] + 2.0f * (t.p[3 + k] - t.p[k]);  // collinear (nearly)
        t.make();
        return t;
      },
      [&](const Tri& t, float&) {
        double o[3] = {g.sym(6), g.sym(6), g.sym(6)}, q[3];
        bary(t, g.uni(), g.uni(), g.uni(), q);
        return through(g, o, q);
      });
  // denormal and zero coordinates
  run("denormal_zero",
      [&]() {
        Tri t = randomTri(g, kSizes[g.below(3)], g.below(2) ? 1.0 : 0.0);
        for (int k = 0; k < 9; ++k) {
          const int what = g.below(6);
          if (what == 0) t.p[k] = 0.0f;
          if (what == 1) t.p[k] = -0.0f;
          if (what == 2) t.p[k] = (float)ldexp(g.sym(1), -127 - g.below(20));
        }
        if (g.below(4) == 0) for (int k = 0; k < 9; ++k) t.p[k] = (float)ldexp(g.sym(1), -120 - g.below(28));
        t.make();
        return t;
      },
      [&](const Tri& t, float& tMin) {
        double o[3], q[3];
        frontOrigin(g, t, g.below(2) ? 1.0 : 1e-38, o);
        const double a = -0.25 + 1.5 * g.uni(), b = -0.25 + 1.5 * g.uni();
        bary(t, 1 - a - b, a, b, q);
        if (g.below(2)) tMin = 0.0f;
        SrtTriRay r = through(g, o, q);
        if (g.below(4) == 0) r.ox = (float)ldexp(g.sym(1), -130);
        return r;
      });
  // direction components that are 0
  run("axis_directions", [&]() {
        Tri t = randomTri(g, kSizes[g.below(3)], 6.0);
        if (g.below(2)) { const int ax = g.below(3); t.p[3 + ax] = t.p[6 + ax] = t.p[ax]; t.make(); }  // axis-aligned plane
        return t;
      },
      [&](const Tri& t, float&) {
        double o[3], q[3];
        frontOrigin(g, t, 3.0, o);
        const double a = -0.25 + 1.5 * g.uni(), b = g.below(3) ? -0.25 + 1.5 * g.uni() : 0.0;
        bary(t, 1 - a - b, a, b, q);
        const int keep = g.below(3), also = g.below(2);
        for (int k = 0; k < 3; ++k)
          if (k != keep && (also || k == (keep + 1) % 3)) o[k] = (double)(float)q[k];  // that component of d is exactly 0
        SrtTriRay r = through(g, o, q);
        return r;
      });
  // origins at 1e30
  run("far_origin", boxTri, [&](const Tri& t, float&) {
    double o[3], q[3];
    const double a = -0.25 + 1.5 * g.uni(), b = -0.25 + 1.5 * g.uni();
    bary(t, 1 - a - b, a, b, q);
    const double n[3] = {t.test[0].w, t.test[1].w, t.test[2].w};
    for (int k = 0; k < 3; ++k) o[k] = (n[k] >= 0 ? 1e30 : -1e30) * (0.1 + g.uni());
    SrtTriRay r = through(g, o, q);
    if (g.below(2)) { r.dx *= 1e30f; r.dy *= 1e30f; r.dz *= 1e30f; }
    return r;
  });
  for (const Tally& y : all)
    printf("class %s pairs %llu plane_ok %llu undecided %llu diff %llu t_diff %llu max_ratio %.4f\n", y.name, (unsigned long long)y.pairs,
           (unsigned long long)y.planeOk, (unsigned long long)y.undecided, (unsigned long long)y.diff, (unsigned long long)y.tDiff, y.maxRatio);
  return 0;
}

static int exactMode(const char* inPath, const char* outPath) {
  FILE* in = fopen(inPath, "rb");
  Tri t;
  int32_t n = 0;
  if (!in || fread(t.p, 4, 9, in) != 9 || fread(&n, 4, 1, in) != 1 || n < 0) return 1;
  std::vector<float> rays((size_t)n * 7);
  if (fread(rays.data(), 4, rays.size(), in) != rays.size()) return 1;
  fclose(in);
  t.make();
  FILE* out = fopen(outPath, "wb");
  if (!out) return 1;
  for (int32_t i = 0; i < n; ++i) {
    const float* q = &rays[7 * (size_t)i];
    const SrtTriRay r{q[0], q[1], q[2], q[3], q[4], q[5]};
    float tE = 0, tC = 0;
    bool undecided;
    const bool exact = srtTriHitExact<false>(t.test[0], t.test[1], t.test[2], r, q[6], 0.0f, tE);
    const bool cert = srtTriHitCert(t.fast[0], t.fast[1], t.fast[2], t.fast[3], r, q[6], SRT_TRI_W_MAX, tC, undecided);
    const int32_t rec[4] = {exact ? 1 : 0, (int32_t)bits(tE), cert ? 1 : 0, undecided ? 1 : 0};
    fwrite(rec, sizeof rec, 1, out);
  }
  return fclose(out) ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "sweep")) return sweep(strtoull(argv[2], nullptr, 0), atoi(argv[3]));
  if (argc == 4 && !strcmp(argv[1], "exact")) return exactMode(argv[2], argv[3]);
  return 2;
}
