// The regrouped tree's host code (csrc/srt_regroup.h) and the gate form of the exact slab test (csrc/srt_slab.h
// srtSlabGateExact) as a stand-alone host program (no GPU, no library): used by tests/test_regroup_host.py, and the place for
// a sanitizer build of both.
//   srt_regroup_probe regroup <in.bin> <out.bin>
//     in:  int32 numNodes, numWorld; the node records (2 x float4 each); the world list (int32 each)
//     out: int32 1 and the regrouped records, or int32 0 alone (a tree that is not a pre-order tree of two-node / two-primitive nodes)
//   srt_regroup_probe walk <in.bin> <out.bin>
//     in:  as for `regroup` (a regrouped array, or any array of such trees)
//     out: int32 1, int32 count, the keep mask as one int32 per node, then src[count], links[2 x count] (hit word, miss word) and
//          entry[numWorld] -- the walk sequence of srtRegroupWalk with the link words of csrc/srt_wf_links.h -- or int32 0 alone.
//          Before it writes, the program follows the links from every entry and checks that it meets each of that tree's
//          kept records once, in order, that every node word lies inside the sequence, and that srtWfRootWord leaves the
//          entry words as they are (the launch hands them to the kernel in the world list's place); exit status 3 otherwise.
//   srt_regroup_probe head <in.bin> <out.bin>
//     in:  int32 numNodes, numWorld, numKinds; the node records and the world list with primitives as ~index; one byte per
//          index, != 0 = a sphere
//     out: int32 ok, int32 head -- srtRegroupHeadOfKinds: the head word of the sequence's walks over the device's references
//          ~(index << 1 | sphere), 0 where the walks have none; ok = 0 (and head 0) for an input it refuses.  Where there is a
//          head the program decodes it as the kernel does and checks that its one or two objects are spheres of the list;
//          exit status 3 otherwise.
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

static int walk(FILE* in, FILE* out) {
  int32_t n[2];
  if (fread(n, 4, 2, in) != 2 || n[0] < 0 || n[1] < 0) return 1;
  std::vector<float4> nodes(2 * (size_t)n[0]);
  std::vector<int32_t> world(n[1]);
  if (fread(nodes.data(), sizeof(float4), nodes.size(), in) != nodes.size()) return 1;
  if (fread(world.data(), 4, world.size(), in) != world.size()) return 1;
  SrtRegroupWalk w;
  const int32_t ok = srtRegroupWalk(nodes, world, w) ? 1 : 0;
  fwrite(&ok, 4, 1, out);
  if (!ok) return 0;
  const int32_t count = (int32_t)w.src.size();
  // the kernel's own decoding of the words: from each entry the walk in which every box passes (a gate: its hit link; a
  // leaf: its objects, then its miss link) meets the records of that tree one after the other and ends in DONE; a miss link
  // leads ahead, to a record of the sequence, or is DONE
  int32_t met = 0;
  for (size_t k = 0; k < world.size(); ++k) {
    int32_t cur = w.entry[k];
    if (srtWfRootWord(cur) != cur) return 3;
    if (world[k] < 0) {
      if (cur != srtWfRootWord(world[k]) || !srtWfAtPrim(srtWfLeafFirst(cur)) || srtWfLeafHasSecond(cur)) return 3;
      continue;
    }
    while (cur != SRT_WF_DONE) {
      if (met >= count || cur != SRT_NODE_REF(met)) return 3;
      const int32_t hit = w.links[2 * (size_t)met], miss = w.links[2 * (size_t)met + 1];
      if (miss != SRT_WF_DONE && (!srtWfAtNode(miss) || (miss & 31) || SRT_NODE_INDEX(miss) <= met || SRT_NODE_INDEX(miss) >= count)) return 3;
      if (!srtWfAtNode(hit) && (hit == SRT_WF_DONE || !srtWfAtPrim(srtWfLeafFirst(hit)))) return 3;
      // the record's own children, decoded as popNext does: a gate's hit link is a node, a leaf word gives back both objects
      const int32_t l = srt_regroup_detail::refOf(nodes, 2 * (size_t)w.src[met]), r = srt_regroup_detail::refOf(nodes, 2 * (size_t)w.src[met] + 1);
      if (srtWfAtNode(hit) != (l >= 0)) return 3;
      if (l < 0) {
        if (srtWfLeafFirst(hit) != l || srtWfLeafHasSecond(hit) != (l != r)) return 3;
        if (l != r && (srtWfLeafFirst(srtWfLeafRest(hit)) != r || srtWfLeafHasSecond(srtWfLeafRest(hit)))) return 3;
      }
      cur = srtWfAtNode(hit) ? hit : miss;
      met++;
    }
  }
  if (met != count) return 3;
  fwrite(&count, 4, 1, out);
  for (uint8_t k : w.keep) {
    const int32_t v = k;
    fwrite(&v, 4, 1, out);
  }
  fwrite(w.src.data(), 4, w.src.size(), out);
  fwrite(w.links.data(), 4, w.links.size(), out);
  fwrite(w.entry.data(), 4, w.entry.size(), out);
  return 0;
}

static int head(FILE* in, FILE* out) {
  int32_t n[3];
  if (fread(n, 4, 3, in) != 3 || n[0] < 0 || n[1] < 0 || n[2] < 0) return 1;
  std::vector<float4> nodes(2 * (size_t)n[0]);
  std::vector<int32_t> world(n[1]);
  std::vector<uint8_t> kinds(n[2]);
  if (fread(nodes.data(), sizeof(float4), nodes.size(), in) != nodes.size()) return 1;
  if (fread(world.data(), 4, world.size(), in) != world.size()) return 1;
  if (fread(kinds.data(), 1, kinds.size(), in) != kinds.size()) return 1;
  int32_t r[2] = {0, 0};
  r[0] = srtRegroupHeadOfKinds(nodes, world, kinds.data(), n[2], r[1]) ? 1 : 0;
  if (!r[0] && r[1] != 0) return 3;
  if (r[1] != 0) {
    auto sphereOfList = [&](int32_t ref) { return srtWfAtPrim(ref) && (~ref & 1) && (~ref >> 1) < n[2] && kinds[(size_t)(~ref >> 1)] != 0; };
    if (world.size() != 1 || !srtWfAtPrim(r[1]) || !sphereOfList(srtWfLeafFirst(r[1]))) return 3;
    if (srtWfLeafHasSecond(r[1]) && (!sphereOfList(srtWfLeafFirst(srtWfLeafRest(r[1]))) || srtWfLeafHasSecond(srtWfLeafRest(r[1])))) return 3;
  }
  fwrite(r, 4, 2, out);
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
  if (!strcmp(argv[1], "walk")) rc = walk(in, out);
  if (!strcmp(argv[1], "head")) rc = head(in, out);
  if (!strcmp(argv[1], "gate")) rc = gate(in, out);
  fclose(in);
  return fclose(out) ? 1 : rc;
}
