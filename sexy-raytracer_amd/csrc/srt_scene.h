// srt_scene.h -- the host stage of srtUploadScene: validation, the reference-order BVH build and the flattening of a
// scene into the device record formats (srt_device.h).  Pure host code (srt_scene.cpp makes no HIP runtime calls);
// srt_api.cpp uploads what it produces and runs the device builds.  validateScene and flattenScene run as a stand-alone host
// program as well (examples/scene_probe.cpp), which tests/test_scene_host.py pins member by member.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "srt_device.h"
#include "srt_records.h"

// ------------------------------------------------------------------ bvh.h:55-95
struct BuildNode {
  Box box;
  int32_t left, right;  // >= 0 node, < 0 ~primListIndex
  uint8_t axis = 3;     // split axis (left child = lower box minimum on it), 3 = unknown
};

struct Builder {
  const SrtSceneDesc* d;
  float time0, time1;
  std::vector<float> sortKey;    // boundingBox(0,0).minimum per prim (boxCompare, bvh.h:34-41), 3 per prim
  std::vector<int32_t> objects;  // prim list indices; the reference's `objects` vector
  std::vector<BuildNode> nodes;
  int maxPending = 0;

  Box childBox(int32_t ref) const;
  int32_t build(size_t start, size_t end, int pending);
  void toBvhNodes(SrtBvhNode* out) const;  // the tree as srtBuildBvh and srtGetBvh report it
};

// make_shared<bvhNode>(objects, time0, time1) over one world item (main.cpp:146, bvh.h:15-16), or adoption of a
// caller-built tree (validated by validateScene).  Consumes the process-global generator (srtHostRandomFloat).
void buildItem(const SrtSceneDesc* d, const SrtWorldItem& it, Builder& b);

// Every index the kernels (and the host builder) will follow.  Returns the error text, empty when the scene is valid.
std::string validateScene(const SrtSceneDesc* d);

// The tunables the flattening reads (srtSetTunable names in parentheses).
struct SceneOptions {
  int wfHybrid;       // (wf_hybrid) hybrid records for trees that do not fit LDS
  int wfResidentMax;  // (wf_resident_max) cap on the hybrid form's resident nodes
  int fastDiv;        // (fast_div) the value DevScene::fastDivScene takes when the certificate holds
};

// A world item whose tree the device builds (srt_lbvh.hip) into node slots reserved for it.
struct DeviceBuild {
  int32_t item;         // world item
  int32_t base, count;  // first node slot, number of nodes
  int32_t builder;      // SRT_BUILDER_LBVH / SRT_BUILDER_PLOC
  float time0, time1;
  std::vector<int32_t> refs;  // the item's primitives as device references
};

// A world item whose tree the host built or adopted: where it lies in the node array, and the times its boxes are made
// for (srtRefitScene fits them again; DeviceBuild carries the same for the device-built ones).
struct HostTree {
  int32_t item;
  int32_t base, count;
  float time0, time1;
};

// Every array srtUploadScene uploads, in its final order and layout (DevScene's fields of the same names).
struct HostScene {
  std::vector<float4> nodes;  // device-built items' slots are zero until their build
  std::vector<uint8_t> nodeAxis;
  std::vector<int32_t> world;
  std::vector<float4> triTest, triShade, triFast, spheres;
  std::vector<int32_t> triPrimId, sphPrimId;  // device index -> primitive list index
  std::vector<DevMaterial> materials;
  std::vector<DevTexture> textures;
  std::vector<uint8_t> texels;
  std::vector<uint4> shadeRecs;
  std::vector<uint8_t> primClass;
  std::vector<int32_t> nodeThread;  // empty: no 16-bit thread links
  // the regrouped tree of the path-pool kernel's whole-tree form (srt_regroup.h): nodes' size and node ranges, other inner
  // nodes over the same leaves, and its own 16-bit thread links.  Empty: not built
  std::vector<float4> nodesRg;
  std::vector<int32_t> nodeThreadRg;
  // its walk sequence (srt_regroup.h srtRegroupWalk; DevScene::walkSeq): per kept record (source record in nodesRg, hit
  // word, miss word), numWalk of them, then one entry word per world item.  Empty with nodesRg
  std::vector<int32_t> walkSeq;
  int32_t numWalk = 0;
  int32_t wfHead = 0;  // SrtRegroupWalk::head: the leaf word every walk of the sequence begins with, 0 = none
  std::vector<float4> nodesWf;     // empty: no hybrid records
  std::vector<int32_t> worldWf, primSecond;
  int32_t wfResident = 0;
  std::vector<std::vector<SrtBvhNode>> itemNodes;  // per world item: its host-built tree (srtGetBvh)
  std::vector<DeviceBuild> deviceBuilds;
  std::vector<HostTree> hostTrees;
  std::vector<int32_t> triDevIndex;  // scene triangle index -> device index (the inverse of the reordering); empty: identity
  std::vector<int32_t> wfIndex;      // node index -> its record in nodesWf (srtHybridRecords' renumbering); empty with nodesWf
  int stackDepth = 0, bvhDepth = 0;  // over the host-built trees
  int32_t fastDivScene = 0;          // over the host-built nodes and the device-built items' primitive boxes
  int32_t boxOrderedScene = 0;       // (DevScene::boxOrderedScene) over the same boxes
};

// Flattens a scene that passed validateScene.  Returns the error text, empty on success.
std::string flattenScene(const SrtSceneDesc* d, const SceneOptions& o, HostScene& out);

// The lights direct sampling chooses from (include/srt_hip.h "Direct light sampling"), from what flattenScene made: device
// sphere indices in prims[] order.
std::vector<int32_t> sampledLights(const HostScene& h);
