// srt_wf_links.h -- the link words of the path-pool kernel's LDS copy of the tree, whole-tree form (srt_wavefront.hip,
// HYBRID == false): ONE statement of their encoding for the kernel's prologue, which builds the copy from DevScene::nodes
// and DevScene::nodeThread, for its walk, which decodes them, and for a host program (examples/wf_links_probe.cpp,
// tests/test_wf_links.py).  The copy is private to the kernel; the one place outside it that holds such words is the regrouped
// tree's walk sequence (DevScene::walkSeq, at the end of this file), whose words the upload makes with the functions here.
//
// A lane's position `cur` and a node's two words are 32-bit values of four disjoint kinds:
//   x >= 0            a node: the BYTE OFFSET of its record in the LDS copy (index * 32; the copy sits at LDS offset 0, so
//                     the value is the LDS address and a visit needs no address arithmetic).  At most 2^15 nodes have
//                     thread links (srt_thread.h), so an offset stays below 2^20.
//   SRT_WF_DONE       0x80000000: the walk is over
//   a LEAF WORD       two 16-bit halves, both with their top bit set.  Low half: the leaf's first object as the low 16 bits
//                     of its primitive reference ~(index << 1 | sphere) -- 0x8002..0xffff, srtThreadLinks16 admits no
//                     others.  High half: 0x8000 when nothing follows it, else the second object's 16 bits MINUS ONE
//                     (0x8001..0xfffe).  So a leaf word lies in [0x80008002, 0xfffeffff].
//   a PRIMITIVE REF   0xffff8002..0xffffffff: the sign-extended reference itself.  The walk never stands on one: it is what
//                     srtWfLeafFirst gives, what hitRef and hitPrim[] hold and what the class lookup and the AOV record read.
// The minus one keeps the last two apart: without it the leaf "x, then triangle 0" would be x's own reference.
//   n0.w (taken on a box hit)   internal node: the left child's byte offset; leaf: its leaf word
//   n1.w (taken on a miss)      the successor's byte offset, or SRT_WF_DONE
// "At a node" is x >= 0 and "at a primitive" is (uint32_t)x > (uint32_t)SRT_WF_DONE: one compare each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srt_device.h"

#define SRT_WF_DONE ((int32_t)0x80000000)

SRT_HD inline bool srtWfAtNode(int32_t x) { return x >= 0; }
SRT_HD inline bool srtWfAtPrim(int32_t x) { return (uint32_t)x > (uint32_t)SRT_WF_DONE; }

// ---- encode.  `first`, `second`: primitive references (negative); second == first: a single-object leaf
SRT_HD inline int32_t srtWfLeafWord(int32_t first, int32_t second) {
  const uint32_t hi = second != first ? ((uint32_t)second & 0xffffu) - 1u : 0x8000u;
  return (int32_t)(hi << 16 | ((uint32_t)first & 0xffffu));
}
// n0.w of node i from DevScene::nodes[2 * i].w (`left`: a node's byte offset or the first object's reference) and
// DevScene::nodeThread[i] (`thread`: successor << 16 | what follows the first object, 16-bit references of srtThreadLinks16)
SRT_HD inline int32_t srtWfHitWord(int32_t left, int32_t thread) {
  if (left >= 0) return left;
  const uint32_t follows = (uint32_t)thread & 0xffffu, after = (uint32_t)thread >> 16;
  // (a successor is a node index or 0x8000, never a primitive's 16 bits: "follows == after" is the single-object leaf)
  return srtWfLeafWord(left, follows != after ? (int32_t)(follows | 0xffff0000u) : left);
}
// n1.w of node i from DevScene::nodeThread[i]
SRT_HD inline int32_t srtWfMissWord(int32_t thread) {
  const int32_t after = thread >> 16;  // sign-extended: a node index, or 0x8000 -> -32768
  return after >= 0 ? SRT_NODE_REF(after) : SRT_WF_DONE;
}
// a root of the world list (DevScene::world[k]: a node's byte offset, or a primitive's reference)
SRT_HD inline int32_t srtWfRootWord(int32_t ref) { return ref >= 0 ? ref : srtWfLeafWord(ref, ref); }

// ---- decode a leaf word
SRT_HD inline int32_t srtWfLeafFirst(int32_t leaf) { return (int32_t)(int16_t)leaf; }  // the first object's reference
SRT_HD inline bool srtWfLeafHasSecond(int32_t leaf) { return (uint32_t)leaf >= 0x80010000u; }
// the leaf word of the second object alone (only where srtWfLeafHasSecond)
SRT_HD inline int32_t srtWfLeafRest(int32_t leaf) { return (int32_t)((((uint32_t)leaf >> 16) | 0x80000000u) + 1u); }

// ---- the ELIDED walk sequence (srt_regroup.h srtRegroupWalk; tunable "wf_regroup" 2): the kept records of the regrouped
// tree, numbered in pre-order, in the first slots of the same LDS copy.  Record j's two words, the same four kinds as above:
//   n0.w   a gate: the record right behind it (the first kept record of its subtree: leaves are always kept);
//          a leaf: its leaf word
//   n1.w   the first kept record behind its subtree (`after`: its number, < 0: none), or SRT_WF_DONE
// and a world item's entry word: the first kept record of its tree, or the bare primitive's root word.  srtWfRootWord leaves
// an entry word as it is (a node's offset: itself; a single-object leaf word: the same word again), so a launch may hand
// the entry words to the kernel in the world list's place.
SRT_HD inline int32_t srtWfSeqHitWord(int32_t left, int32_t right, int32_t j) { return left >= 0 ? SRT_NODE_REF(j + 1) : srtWfLeafWord(left, right); }
SRT_HD inline int32_t srtWfSeqMissWord(int32_t after) { return after >= 0 ? SRT_NODE_REF(after) : SRT_WF_DONE; }
SRT_HD inline int32_t srtWfSeqEntryWord(int32_t ref, int32_t first) { return ref >= 0 ? SRT_NODE_REF(first) : srtWfRootWord(ref); }
