// srt_regroup.h -- host side of the path-pool kernel's REGROUPED tree: other inner nodes over the reference's leaves.
//
// In the reference a leaf's objects are tested if and only if the leaf's own box test passes with the running `closest` of
// that moment (bvh.h:97-105, aabb.h:11-27): an ancestor's box contains the leaf's, so by the monotonicity of
// fl(fl(p - o) / d) in the plane p an ancestor that misses is never one whose leaf would have passed (DESIGN section 6 has
// the proof and its one exception, an axis with d == +-0, which the kernel's gate form closes).  So ANY hierarchy whose inner
// boxes are unions of contiguous runs of the reference's leaf sequence, walked in that leaf order, ends every walk at the
// reference's (t, primitive), bit for bit.  bvh.h's median splits on a random axis are one such hierarchy and a poor one:
// with a sphere of radius 1000 among a mesh's triangles no ray is culled high in the tree.
//
// srtRegroupNodes rebuilds the inner nodes of every tree of the world list top-down over its leaves in walk order: a range
// of leaves is split at the k that minimises area(left) * k + area(right) * (n - k), ties to the lowest k.  The result has
// the same size and the same node range per tree (pre-order, root first: DevScene::world stays valid), the leaf records bit
// for bit, and goes to the device NEXT TO the reference array (DevScene::nodesRg) with thread links of its own: the
// reference array stays the canonical tree of srtGetBvh, every other kernel, the refit and the counters.
//
// Cost: prefix and suffix boxes make a split linear in its range, so a tree is quadratic in its leaves at worst (a chain).
// flattenScene therefore regroups only what the whole-tree form of the path-pool kernel can take -- a node array that fits a
// CU's LDS, about 4 400 nodes: a few milliseconds -- and larger trees (the hybrid form) wait for a sub-quadratic builder.
// Pure host code (no HIP calls): tests/test_regroup_host.py drives it through srtTestRegroup (include/srt_hip_test.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "srt_device.h"
#include "srt_records.h"
#include "srt_wf_links.h"

namespace srt_regroup_detail {
inline int32_t refOf(const std::vector<float4>& nodes, size_t slot) {
  int32_t r;
  memcpy(&r, &nodes[slot].w, 4);
  return r;
}
inline Box boxOfNode(const std::vector<float4>& nodes, size_t i) {
  return Box{{nodes[2 * i].x, nodes[2 * i].y, nodes[2 * i].z}, {nodes[2 * i + 1].x, nodes[2 * i + 1].y, nodes[2 * i + 1].z}};
}
inline double halfArea(const Box& b) {
  const double x = (double)b.mx[0] - b.mn[0], y = (double)b.mx[1] - b.mn[1], z = (double)b.mx[2] - b.mn[2];
  return x * y + y * z + z * x;
}
// The union as the refit makes it (srt_records.h surrounding: the reference's fminf / fmaxf).  Every plane of the result is
// a plane of one of the two, bit for bit: the planes of an inner box are planes of its leaves, so what flattenScene certified
// of the reference array's boxes (fastDivScene, boxOrderedScene) holds for this one.
inline Box unite(const Box& a, const Box& b) {
  const Box r = surrounding(a, b);
  for (int k = 0; k < 3; ++k) {
    assert(memcmp(&r.mn[k], &a.mn[k], 4) == 0 || memcmp(&r.mn[k], &b.mn[k], 4) == 0);
    assert(memcmp(&r.mx[k], &a.mx[k], 4) == 0 || memcmp(&r.mx[k], &b.mx[k], 4) == 0);
  }
  return r;
}
}  // namespace srt_regroup_detail

// nodes: the flattened array (2 x float4 per node: (bmin.xyz, left) (bmax.xyz, right), node references = index * 32,
// primitives negative); world: its roots.  A leaf is a node with two primitive children (one object: left == right).
// Returns false, with `out` empty, when a tree is not of two-node / two-primitive nodes laid out in pre-order over one
// contiguous range (bvh.h:55-95 builds nothing else).
inline bool srtRegroupNodes(const std::vector<float4>& nodes, const std::vector<int32_t>& world, std::vector<float4>& out) {
  using namespace srt_regroup_detail;
  const size_t n = nodes.size() / 2;
  out = nodes;  // leaves, and whatever no tree of the world list reaches, stay as they are
  std::vector<uint8_t> seen(n, 0);
  struct Range {
    int32_t me, lo, hi;  // node index, leaves [lo, hi) of the tree's sequence
  };
  std::vector<int32_t> leaves, todo;
  std::vector<Box> leafBox, prefix, suffix;
  std::vector<Range> ranges;
  for (int32_t wr : world) {
    if (wr < 0) continue;
    const int32_t root = SRT_NODE_INDEX(wr);
    // ---- the tree's leaves in walk order (left, then right), and its extent
    leaves.clear();
    todo.assign(1, root);
    int32_t count = 0, last = root;
    while (!todo.empty()) {
      const int32_t i = todo.back();
      todo.pop_back();
      if (i < 0 || (size_t)i >= n || seen[i]) return out.clear(), false;
      seen[i] = 1;
      count++;
      last = i > last ? i : last;
      const int32_t l = refOf(nodes, 2 * (size_t)i), r = refOf(nodes, 2 * (size_t)i + 1);
      if ((l >= 0) != (r >= 0)) return out.clear(), false;
      if (l >= 0) {
        todo.push_back(SRT_NODE_INDEX(r));
        todo.push_back(SRT_NODE_INDEX(l));
      } else {
        leaves.push_back(i);
      }
    }
    if (last - root + 1 != count || (size_t)count != 2 * leaves.size() - 1) return out.clear(), false;
    const int32_t numLeaves = (int32_t)leaves.size();
    leafBox.resize(numLeaves);
    for (int32_t k = 0; k < numLeaves; ++k) leafBox[k] = boxOfNode(nodes, (size_t)leaves[k]);
    prefix.resize(numLeaves);
    suffix.resize(numLeaves);
    // ---- top-down, pre-order: the node of leaves [lo, hi) at `me`, its left subtree (2 * nLeft - 1 nodes) right behind it
    ranges.assign(1, Range{root, 0, numLeaves});
    while (!ranges.empty()) {
      const Range g = ranges.back();
      ranges.pop_back();
      const int32_t span = g.hi - g.lo;
      if (span == 1) {
        out[2 * (size_t)g.me] = nodes[2 * (size_t)leaves[g.lo]];
        out[2 * (size_t)g.me + 1] = nodes[2 * (size_t)leaves[g.lo] + 1];
        continue;
      }
      prefix[g.lo] = leafBox[g.lo];
      for (int32_t k = g.lo + 1; k < g.hi; ++k) prefix[k] = unite(prefix[k - 1], leafBox[k]);
      suffix[g.hi - 1] = leafBox[g.hi - 1];
      for (int32_t k = g.hi - 2; k >= g.lo; --k) suffix[k] = unite(leafBox[k], suffix[k + 1]);
      int32_t bestK = 1;  // leaves in the left child
      double best = 0.0;
      for (int32_t k = 1; k < span; ++k) {
        const double cost = halfArea(prefix[g.lo + k - 1]) * k + halfArea(suffix[g.lo + k]) * (span - k);
        if (k == 1 || cost < best) {  // ties: the lowest k (and a NaN cost never wins)
          best = cost;
          bestK = k;
        }
      }
      const int32_t left = g.me + 1, right = g.me + 2 * bestK;
      const int32_t lRef = SRT_NODE_REF(left), rRef = SRT_NODE_REF(right);
      float lBits, rBits;
      memcpy(&lBits, &lRef, 4);
      memcpy(&rBits, &rRef, 4);
      out[2 * (size_t)g.me] = make_float4(0.0f, 0.0f, 0.0f, lBits);  // the box: below, bottom-up
      out[2 * (size_t)g.me + 1] = make_float4(0.0f, 0.0f, 0.0f, rBits);
      ranges.push_back(Range{right, g.lo + bestK, g.hi});
      ranges.push_back(Range{left, g.lo, g.lo + bestK});
    }
    // ---- the boxes bottom-up (pre-order: children lie behind their parent), each the union of its two children's as the
    // refit computes it (srt_refit.hip refitNodes), so that a refit of unchanged geometry leaves every bit in place
    for (int32_t i = root + count - 1; i >= root; --i) {
      const int32_t l = refOf(out, 2 * (size_t)i), r = refOf(out, 2 * (size_t)i + 1);
      if (l < 0) continue;
      const Box b = unite(boxOfNode(out, (size_t)SRT_NODE_INDEX(l)), boxOfNode(out, (size_t)SRT_NODE_INDEX(r)));
      out[2 * (size_t)i].x = b.mn[0], out[2 * (size_t)i].y = b.mn[1], out[2 * (size_t)i].z = b.mn[2];
      out[2 * (size_t)i + 1].x = b.mx[0], out[2 * (size_t)i + 1].y = b.mx[1], out[2 * (size_t)i + 1].z = b.mx[2];
    }
  }
  return true;
}

// ---- the walk sequence: the regrouped tree without the gates that rarely cull a ray (tunable "wf_regroup" 2).
//
// An inner node of the regrouped tree is a gate: it must pass wherever one of its leaves would, and nothing else is asked of
// it.  A gate that ALWAYS passes meets that, so deleting a gate and handing its children to its nearest kept ancestor is one
// more valid hierarchy over the same leaf sequence: every walk ends at the same (t, primitive).  A visit is the unit of cost,
// as in SAH's collapse rule: a gate g under its binary parent p, with m EFFECTIVE children -- per binary child one, or that
// child's own effective children where the child is an elided gate -- is worth its visit only while it fails often enough to
// save its m children's visits.  With the chance of "a ray that passed p passes g" taken as area(g) / area(p):
//     elide g  <=>  area(g) * m > area(p) * (m - 1)          (double halfArea, strict: a NaN area never elides)
// decided bottom-up (the children's verdicts first; p is the parent in the BINARY array whether or not it is kept), and every
// inner root is elided: nothing lies above it that a miss would save.  Leaves are always kept.
//
// The sequence is the kept records in the array's order (pre-order per tree), numbered 0, 1, ... over the whole array, with
// the link words of srt_wf_links.h (srtWfSeq*): a gate's hit link is the next record, a record's miss link the first kept
// record behind its subtree.  Boxes are NOT part of it: record j's box is nodesRg[src[j]]'s of the moment, so a refit needs
// no second pass, and the keep mask stays valid for any boxes (it is a property of the upload, like the grouping).
struct SrtRegroupWalk {
  std::vector<uint8_t> keep;   // per record of the binary array: 1 = in the sequence
  std::vector<int32_t> src;    // per record of the sequence: its record in the binary array
  std::vector<int32_t> links;  // per record of the sequence: its hit word, its miss word
  std::vector<int32_t> entry;  // per world item: where its walk starts (srtWfSeqEntryWord)
  // The HEAD of every walk (tunable "wf_head"): record 0's leaf word where the world list is ONE tree whose first kept record
  // is a leaf of spheres alone (one or two; ~reference & 1), else 0.  No gate stands in front of such a leaf and its hit and
  // miss words lead to the same successor, so every walk of the scene begins with its box test, its sphere tests and a jump
  // to its miss word: the path-pool kernel runs them where it sets a new ray up (srt_wavefront.hip swapStep).
  int32_t head = 0;
};

// rg: a regrouped array (srtRegroupNodes' output; any array of pre-order trees of two-node / two-primitive nodes will do);
// world: its roots.  Linear in the array.  Returns false, with `out` empty, for anything else.
inline bool srtRegroupWalk(const std::vector<float4>& rg, const std::vector<int32_t>& world, SrtRegroupWalk& out) {
  using namespace srt_regroup_detail;
  const size_t n = rg.size() / 2;
  out = SrtRegroupWalk();
  auto fail = [&]() { return out = SrtRegroupWalk(), false; };
  std::vector<uint8_t> keep(n, 0), seen(n, 0);
  std::vector<int32_t> parent(n, -1), end(n, 0), children(n, 1), count(world.size(), 0), todo;
  for (size_t wi = 0; wi < world.size(); ++wi) {
    if (world[wi] < 0) continue;
    const int32_t root = SRT_NODE_INDEX(world[wi]);
    // ---- the tree's extent and every node's binary parent; pre-order: the left child lies right behind its parent
    todo.assign(1, root);
    int32_t cnt = 0, last = root;
    while (!todo.empty()) {
      const int32_t i = todo.back();
      todo.pop_back();
      if (i < 0 || (size_t)i >= n || seen[i]) return fail();
      seen[i] = 1;
      cnt++;
      last = i > last ? i : last;
      const int32_t l = refOf(rg, 2 * (size_t)i), r = refOf(rg, 2 * (size_t)i + 1);
      if ((l >= 0) != (r >= 0)) return fail();
      if (l < 0) continue;
      const int32_t li = SRT_NODE_INDEX(l), ri = SRT_NODE_INDEX(r);
      if (li != i + 1 || ri <= li || (size_t)ri >= n) return fail();
      parent[li] = parent[ri] = i;
      todo.push_back(ri);
      todo.push_back(li);
    }
    if (last - root + 1 != cnt) return fail();
    count[wi] = cnt;
    // ---- the keep mask bottom-up (children lie behind their parent), and where every subtree ends
    for (int32_t i = root + cnt - 1; i >= root; --i) {
      const int32_t l = refOf(rg, 2 * (size_t)i), r = refOf(rg, 2 * (size_t)i + 1);
      if (l < 0) {
        keep[i] = 1;
        end[i] = i + 1;
        continue;
      }
      const int32_t li = SRT_NODE_INDEX(l), ri = SRT_NODE_INDEX(r);
      if (end[li] != ri) return fail();  // (the right child lies right behind the left subtree)
      end[i] = end[ri];
      const int32_t m = children[li] + children[ri];
      const bool elide = i == root || halfArea(boxOfNode(rg, (size_t)i)) * (double)m > halfArea(boxOfNode(rg, (size_t)parent[i])) * (double)(m - 1);
      keep[i] = elide ? 0 : 1;
      children[i] = elide ? m : 1;
    }
  }
  // ---- the sequence: numbers in array order, then per tree the links
  std::vector<int32_t> number(n + 1, -1);
  for (size_t i = 0; i < n; ++i)
    if (keep[i]) {
      number[i] = (int32_t)out.src.size();
      out.src.push_back((int32_t)i);
    }
  out.links.assign(2 * out.src.size(), SRT_WF_DONE);
  out.entry.resize(world.size());
  std::vector<int32_t>& next = end;  // (re-used below: end[i] is read before next[i] is written, i descending)
  for (size_t wi = 0; wi < world.size(); ++wi) {
    if (world[wi] < 0) {
      out.entry[wi] = srtWfSeqEntryWord(world[wi], -1);
      continue;
    }
    const int32_t root = SRT_NODE_INDEX(world[wi]), stop = root + count[wi];
    // next[i]: the number of the first kept record at or behind i in this tree, -1: none
    int32_t behind = -1;
    for (int32_t i = stop - 1; i >= root; --i) {
      const int32_t e = end[i];
      const int32_t after = e < stop ? next[e] : -1;
      if (keep[i]) {
        const int32_t j = number[i];
        out.links[2 * (size_t)j] = srtWfSeqHitWord(refOf(rg, 2 * (size_t)i), refOf(rg, 2 * (size_t)i + 1), j);
        out.links[2 * (size_t)j + 1] = srtWfSeqMissWord(after);
        behind = j;
      }
      next[i] = behind;
    }
    out.entry[wi] = srtWfSeqEntryWord(world[wi], next[root]);
  }
  if (world.size() == 1 && world[0] >= 0 && !out.src.empty()) {
    const size_t i = (size_t)out.src[0];
    const int32_t l = refOf(rg, 2 * i), r = refOf(rg, 2 * i + 1);
    if (l < 0 && (~l & 1) && (~r & 1)) out.head = srtWfLeafWord(l, r);
  }
  out.keep.swap(keep);
  return true;
}

// The head word of an array whose primitive references are ~index into a list of kinds (kinds[index] != 0: a sphere), as the
// CPU oracle's trees have them, worded over the device's references ~(index << 1 | sphere): srtTestWfHead
// (include/srt_hip_test.h) and examples/regroup_probe.cpp's mode `head`.  False, with head = 0, for what srtRegroupWalk
// refuses, an index outside the list or beyond the 15 bits of a leaf word's half (srt_wf_links.h).
inline bool srtRegroupHeadOfKinds(std::vector<float4> nodes, std::vector<int32_t> world, const uint8_t* kinds, int32_t numKinds, int32_t& head) {
  head = 0;
  auto deviceRef = [&](int32_t& ref) {
    const int32_t index = ~ref;
    if (index >= numKinds || index > 0x3ffe) return false;
    ref = ~(index << 1 | (kinds[index] ? 1 : 0));
    return true;
  };
  for (float4& v : nodes) {
    int32_t ref;
    memcpy(&ref, &v.w, 4);
    if (ref >= 0) continue;
    if (!deviceRef(ref)) return false;
    memcpy(&v.w, &ref, 4);
  }
  for (int32_t& ref : world)
    if (ref < 0 && !deviceRef(ref)) return false;
  SrtRegroupWalk walk;
  if (!srtRegroupWalk(nodes, world, walk)) return false;
  head = walk.head;
  return true;
}
