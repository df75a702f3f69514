// The regrouped tree's host code (csrc/srt_regroup.h) and the gate form of the exact slab test (csrc/srt_slab.h
// srtSlabGateExact) as a stand-alone host program (no GPU, no library): used by tests/test_regroup_host.py, and the place for
// a sanitizer build of both.
//   srt_regroup_probe regroup <in.bin> <out.bin>
//     in:  int32 numNodes, numWorld; the node records (2 x float4 each); the world list (int32 each)
//     out: int32 1 and the regrouped records, or int32 0 alone (a tree that is not a pre-order tree of two-node / two-primitive nodes)
//   srt_regroup_probe gate <in.bin> <out.bin>
//     in:  int32 n; n cases of 20 floats: the leaf box (min.xyz, max.xyz), the gate box (min.xyz, max.xyz), the ray's origin
//          and direction, tMin, tMax
//     out: per case three int32 -- the reference's test (aabb.h:11-27, restated below) on the leaf box, the same test on the
//          gate box, and the gate form on the gate box
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "srt_regroup.h"
#include "srt_slab.h"

// aabb.h:11-27 as it stands: per axis both quotients, fminf / fmaxf, the early out
static bool referenceBoxHit(const float* mn, const float* mx, const float* o, const float* d, float tMin, float tMax) {
  for (int axis = 0; axis < 3; axis++) {
    const float t0 = fminf((mn[axis] - o[axis]) / d[axis], (mx[axis] - o[axis]) / d[axis]);
    const float t1 = fmaxf((mn[axis] - o[axis]) / d[axis], (mx[axis] - o[axis]) / d[axis]);
    tMin = fmaxf(t0, tMin);
    tMax = fminf(t1, tMax);
    if (tMax <= tMin) return false;
  }
  return true;
}

static int regroup(FILE* in, FILE* out) {
  int32_t n[2];
  if (fread(n, 4, 2, in) != 2 || n[0] < 0 || n[1] < 0) return 1;
  std::vector<float4> nodes(2 * (size_t)n[0]), rg;
  std::vector<int32_t> world(n[1]);
  if (fread(nodes.data(), sizeof(float4), nodes.size(), in) != nodes.size()) return 1;
  if (fread(world.data(), 4, world.size(), in) != world.size()) return 1;
  const int32_t ok = srtRegroupNodes(nodes, world, rg) ? 1 : 0;
  fwrite(&ok, 4, 1, out);
  if (ok) fwrite(rg.data(), sizeof(float4), rg.size(), out);
  return 0;
}

static int gate(FILE* in, FILE* out) {
  int32_t n;
  if (fread(&n, 4, 1, in) != 1 || n < 0) return 1;
  std::vector<float> c(20 * (size_t)n);
  if (fread(c.data(), 4, c.size(), in) != c.size()) return 1;
  std::vector<int32_t> r(3 * (size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    const float* p = &c[20 * (size_t)i];
    r[3 * (size_t)i] = referenceBoxHit(p, p + 3, p + 12, p + 15, p[18], p[19]);
    r[3 * (size_t)i + 1] = referenceBoxHit(p + 6, p + 9, p + 12, p + 15, p[18], p[19]);
    r[3 * (size_t)i + 2] = srtSlabGateExact(make_float4(p[6], p[7], p[8], 0.0f), make_float4(p[9], p[10], p[11], 0.0f), SrtSlab3{p[12], p[13], p[14]},
                                            SrtSlab3{p[15], p[16], p[17]}, p[18], p[19]);
  }
  fwrite(r.data(), 4, r.size(), out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 1;
  int rc = 2;
  if (!strcmp(argv[1], "regroup")) rc = regroup(in, out);
  if (!strcmp(argv[1], "gate")) rc = gate(in, out);
  fclose(in);
  return fclose(out) ? 1 : rc;
}
