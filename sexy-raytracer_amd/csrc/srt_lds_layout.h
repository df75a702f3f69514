// srt_lds_layout.h -- how every kernel that asks for dynamic LDS carves it up, stated ONCE as byte arithmetic for the host
// (the planner srt_plan.cpp, the upload srt_scene.cpp, the launches of srt_render.cpp and srt_passes.cpp, the stand-alone
// examples/plan_probe.cpp) and as the constants the kernels' own pointer carve-ups are written in.  Plain integers, no HIP
// calls.  A kernel that restates a layout in its pointer arithmetic names the function here that it must match.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "srt_wf_rings.h"  // WF_RINGS, SrtWfRingSlot; SRT_HD and the workgroup sizes through srt_device.h

#define SRT_LDS_BYTES (160 * 1024) /* a CU's LDS (gfx950): what one workgroup can ask for */
#define SRT_NODE_BYTES 32          /* a node record in LDS: two 16-byte slots, as in DevScene::nodes */

// ---- the path-pool kernel (srt_wavefront.hip): the resident nodes at offset 0, WF_CTL_WORDS control words, WF_RINGS rings
// of `ringCap` slots, then per context of the pool the t (a float) and the primitive its walk ended at (16 bits; a 32-bit
// reference in the hybrid form)
#define WF_CTL_WORDS 64
struct SrtWfLdsLayout {
  size_t ctl, ringSlots, hitT, hitPrim, end;  // byte offsets
};
SRT_HD inline size_t srtWfPrimSlotBytes(bool hybrid) { return hybrid ? sizeof(int32_t) : sizeof(uint16_t); }
SRT_HD inline SrtWfLdsLayout srtWfLdsLayout(int residentNodes, int ringCap, int poolSize, bool hybrid) {
  SrtWfLdsLayout l;
  l.ctl = (size_t)residentNodes * SRT_NODE_BYTES;
  l.ringSlots = l.ctl + WF_CTL_WORDS * sizeof(int32_t);
  l.hitT = l.ringSlots + (size_t)WF_RINGS * ringCap * sizeof(SrtWfRingSlot);
  l.hitPrim = l.hitT + (size_t)poolSize * sizeof(float);
  l.end = l.hitPrim + (size_t)poolSize * srtWfPrimSlotBytes(hybrid);
  return l;
}
// What a context costs when the pool is as large as the rings, which is what a launch reserves: 18 bytes, 20 in the hybrid form
SRT_HD inline size_t srtWfContextBytes(bool hybrid) { return WF_RINGS * sizeof(SrtWfRingSlot) + sizeof(float) + srtWfPrimSlotBytes(hybrid); }
SRT_HD inline size_t srtWfLdsBytes(int residentNodes, int ringCap, bool hybrid) { return srtWfLdsLayout(residentNodes, ringCap, ringCap, hybrid).end; }
// The inverse: the largest node count that fits beside rings and a pool of `ringCap` contexts
SRT_HD inline int srtWfMaxResidentNodes(int ringCap, bool hybrid) {
  return (int)((SRT_LDS_BYTES - srtWfLdsBytes(0, ringCap, hybrid)) / SRT_NODE_BYTES);
}
// What the upload (srt_scene.cpp flattenScene) decides by: a tree of more nodes than the whole-tree form takes beside its
// smallest rings gets hybrid records, whose resident top is sized to leave room for a pool of SRT_WF_HYBRID_POOL contexts
#define SRT_WF_HYBRID_POOL 2048
inline int srtWfMaxWholeTreeNodes() { return srtWfMaxResidentNodes(kSrtWfRings[sizeof kSrtWfRings / sizeof kSrtWfRings[0] - 1].cap, false); }

// ---- srt_render_kernel over the LDS-resident tree (LDSTREE): every node at offset 0, SRT_LDS_TREE_QUEUE_WORDS words (one
// per wave: its current work queue), and with `attInLds` (ATTLDS) the lanes' attenuation stacks, [slot][thread]
#define SRT_LDS_TREE_QUEUE_WORDS (SRT_BLOCK_TREE / 64)
SRT_HD inline int srtAttSlots(int maxBounce) { return 3 * maxBounce + 3; }  // three per bounce, and the terminal radiance
struct SrtLdsTreeLayout {
  size_t queueWords, attStacks, end;
};
SRT_HD inline SrtLdsTreeLayout srtLdsTreeLayout(int numNodes, int maxBounce, bool attInLds) {
  SrtLdsTreeLayout l;
  l.queueWords = (size_t)numNodes * SRT_NODE_BYTES;
  l.attStacks = l.queueWords + SRT_LDS_TREE_QUEUE_WORDS * sizeof(int32_t);
  l.end = l.attStacks + (attInLds ? (size_t)srtAttSlots(maxBounce) * SRT_BLOCK_TREE * sizeof(float) : 0);
  return l;
}

// ---- srt_render_kernel's 256-thread form: per-thread slots [slot][thread] -- stackDepth + 2 traversal slots (slot 0 holds
// the sentinel, the last is the spare of the node step's unconditional store), the attenuation stack -- then a queue word
// per wave
struct SrtStackFormLayout {
  size_t attStacks, queueWords, end;
};
SRT_HD inline SrtStackFormLayout srtStackFormLayout(int stackDepth, int maxBounce) {
  SrtStackFormLayout l;
  l.attStacks = (size_t)(stackDepth + 2) * SRT_BLOCK * sizeof(int32_t);
  l.queueWords = l.attStacks + (size_t)srtAttSlots(maxBounce) * SRT_BLOCK * sizeof(float);
  l.end = l.queueWords + (SRT_BLOCK / 64) * sizeof(int32_t);
  return l;
}

// ---- the per-lane stacks [slot][thread] of the walks outside the render kernels, SRT_BLOCK threads each.
// srt_query.hip and srt_pathstep.hip (srt_query_walk.h): slot 0 holds the walk's sentinel, the last slot is the spare of its
// unconditional store
SRT_HD inline size_t srtQueryStackBytes(int stackDepth) { return (size_t)((stackDepth > 1 ? stackDepth : 1) + 2) * SRT_BLOCK * sizeof(int32_t); }
// srt_paths.hip: the same walk's slots, then the attenuations of a path's scattered steps [3 * level + channel][thread]
SRT_HD inline size_t srtPathsLdsBytes(int stackDepth, int maxBounce) {
  return srtQueryStackBytes(stackDepth) + (size_t)3 * (maxBounce > 0 ? maxBounce : 0) * SRT_BLOCK * sizeof(float);
}
// ... and its DIRECT instances: per level the attenuation and the direct term, [6 * level + channel][thread]
SRT_HD inline size_t srtPathsDirectLdsBytes(int stackDepth, int maxBounce) {
  return srtQueryStackBytes(stackDepth) + (size_t)6 * (maxBounce > 0 ? maxBounce : 0) * SRT_BLOCK * sizeof(float);
}
// the stack walk of the feature and motion passes and of srtTraceRays (srt_path.h traverse): stackDepth slots
SRT_HD inline size_t srtTraverseStackBytes(int stackDepth) { return (size_t)(stackDepth > 1 ? stackDepth : 1) * SRT_BLOCK * sizeof(int32_t); }
// ... which the passes leave for the stackless walk over the whole tree in LDS where that fits
SRT_HD inline size_t srtFeatureTreeBytes(int numNodes) { return (size_t)numNodes * SRT_NODE_BYTES; }
