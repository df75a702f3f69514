// srt_scene.cpp -- the host stage of srtUploadScene (srt_scene.h): scene validation, the reference-order BVH build,
// the flattening of a scene into the device record formats, and the host arithmetic of the C ABI (the global
// generator, srtMakeCamera).  No HIP runtime calls: everything here runs without a device, and validateScene and flattenScene
// are tested without one (examples/scene_probe.cpp, tests/test_scene_host.py: every array, bit for bit, and under sanitizers).
//
// Host arithmetic that feeds the kernels (BVH boxes, per-triangle normals and tangent frames, the camera frame) keeps
// the reference's operation order; this file is built with -ffp-contract=off and without -march so it rounds like the
// reference's x86-64 build.

#include "srt_scene.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "srt_lds_layout.h"
#include "srt_regroup.h"
#include "srt_thread.h"

namespace {

// ------------------------------------------------------------------ the global generator
// globals.h:30-35: function-local static default-seeded mt19937 + uniform_real_distribution<float>(0,1)
std::mt19937& hostGenerator() {
  static std::mt19937 generator;
  return generator;
}
float hostRandomFloat() {
  static std::uniform_real_distribution<float> distribution(0.0f, 1.0f);
  return distribution(hostGenerator());
}
int hostRandomInt(int lo, int hi) {  // globals.h:37-43
  float a = (float)lo, b = (float)(hi + 1);
  return static_cast<int>(a + (b - a) * hostRandomFloat());
}

// ------------------------------------------------------------------ primitives on the host (srt_records.h)
Box primBox(const SrtSceneDesc* d, int32_t prim, float t0, float t1) {
  const SrtPrimRef& pr = d->prims[prim];
  if (pr.type == SRT_PRIM_SPHERE) {
    const SrtSphereIn& s = d->spheres[pr.index];
    const Vec3 c0 = vec3(s.center0), c1 = vec3(s.center1);
    return sphereBox(c0, c1, c0 != c1, s.time0, s.time1, s.radius, t0, t1);
  }
  const SrtTriangleIn& t = d->triangles[pr.index];
  return triangleBox(vec3(t.p[0]), vec3(t.p[1]), vec3(t.p[2]));
}

std::string format(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
}

template <typename T>
T bitsAs(const void* p) {
  T v;
  memcpy(&v, p, sizeof v);
  return v;
}

}  // namespace

Box Builder::childBox(int32_t ref) const { return ref >= 0 ? nodes[ref].box : primBox(d, ~ref, time0, time1); }

// The reference copies the object vector at each node (bvh.h:57) and sorts [start,end) of the copy; sibling subtrees
// only touch disjoint sub-ranges, so one shared vector sorted in place gives the same tree.  Nodes are emitted in
// pre-order (the order populateVector walks them, bvh.h:112-148).
int32_t Builder::build(size_t start, size_t end, int pending) {
  int axis = hostRandomInt(0, 2);  // bvh.h:60: one draw per node, pre-order
  auto comparator = [this, axis](int32_t a, int32_t b) { return sortKey[3 * a + axis] < sortKey[3 * b + axis]; };
  int32_t me = (int32_t)nodes.size();
  nodes.emplace_back();
  size_t span = end - start;
  int32_t left, right;
  if (span == 1) {
    left = right = ~objects[start];
  } else if (span == 2) {
    if (comparator(objects[start], objects[start + 1])) {
      left = ~objects[start];
      right = ~objects[start + 1];
    } else {
      left = ~objects[start + 1];
      right = ~objects[start];
    }
    maxPending = std::max(maxPending, pending + 1);
  } else {
    std::sort(objects.begin() + start, objects.begin() + end, comparator);
    size_t mid = start + span / 2;
    maxPending = std::max(maxPending, pending + 1);
    // capacity must hold for either visiting order (CLOSEST descends into the near child first and
    // leaves the other one pending), so both children are entered with one more pending entry
    left = build(start, mid, pending + 1);
    right = build(mid, end, pending + 1);
  }
  BuildNode& n = nodes[me];
  n.left = left;
  n.right = right;
  n.axis = (uint8_t)axis;
  n.box = surrounding(childBox(left), childBox(right));  // bvh.h:88-94
  return me;
}

void Builder::toBvhNodes(SrtBvhNode* out) const {
  for (size_t i = 0; i < nodes.size(); ++i) {
    memcpy(out[i].bmin, nodes[i].box.mn, 12);
    memcpy(out[i].bmax, nodes[i].box.mx, 12);
    out[i].left = nodes[i].left;
    out[i].right = nodes[i].right;
  }
}

void buildItem(const SrtSceneDesc* d, const SrtWorldItem& it, Builder& b) {
  b.d = d;
  b.time0 = it.time0;
  b.time1 = it.time1;
  if (it.nodes) {
    b.nodes.resize(it.numNodes);
    std::vector<int> pending(it.numNodes, 0);  // stack entries held when the node is entered
    for (int i = 0; i < it.numNodes; ++i) {
      const SrtBvhNode& n = it.nodes[i];
      memcpy(b.nodes[i].box.mn, n.bmin, 12);
      memcpy(b.nodes[i].box.mx, n.bmax, 12);
      b.nodes[i].left = n.left;
      b.nodes[i].right = n.right;
      const bool two = n.right != n.left;
      if (two) b.maxPending = std::max(b.maxPending, pending[i] + 1);
      if (n.left >= 0) pending[n.left] = pending[i] + (two ? 1 : 0);
      if (two && n.right >= 0) pending[n.right] = pending[i] + 1;  // either child may be the one left pending
    }
    return;
  }
  b.sortKey.resize((size_t)d->numPrims * 3);
  b.objects.resize(it.count);
  for (int i = 0; i < it.count; ++i) {
    int prim = it.first + i;
    b.objects[i] = prim;
    Box bx = primBox(d, prim, 0, 0);  // boxCompare uses boundingBox(0, 0, ...) (bvh.h:37)
    for (int k = 0; k < 3; ++k) b.sortKey[3 * prim + k] = bx.mn[k];
  }
  b.nodes.reserve((size_t)it.count * 2);
  b.build(0, it.count, 0);
}

std::string validateScene(const SrtSceneDesc* d) {
  // counts and pointers first: everything below indexes these arrays and sizes std::vectors with the counts
  if (d->numTriangles < 0 || d->numSpheres < 0 || d->numPrims < 0 || d->numWorld < 0 || d->numMaterials < 0 ||
      d->numTextures < 0 || d->numTexelBytes < 0)
    return "scene: negative element count";
  if ((d->numTriangles > 0 && !d->triangles) || (d->numSpheres > 0 && !d->spheres) || (d->numPrims > 0 && !d->prims) ||
      (d->numWorld > 0 && !d->world) || (d->numMaterials > 0 && !d->materials) || (d->numTextures > 0 && !d->textures) ||
      (d->numTexelBytes > 0 && !d->texels))
    return "scene: null array with a non-zero count";
  if ((int64_t)d->numTriangles > 0x3fffffff || (int64_t)d->numSpheres > 0x3fffffff)
    return "scene: too many primitives for 31-bit device references";
  for (int i = 0; i < d->numTextures; ++i) {
    const SrtTextureIn& t = d->textures[i];
    if (t.kind == SRT_TEX_CHECKER) {
      for (int c : {t.even, t.odd})
        if (c < 0 || c >= d->numTextures || d->textures[c].kind == SRT_TEX_CHECKER)
          return format("texture %d: checker children must be solid or image textures", i);
    } else if (t.kind == SRT_TEX_IMAGE) {
      if (t.width < 0 || t.height < 0 || (t.width > 0 && (t.bpp < 1 || t.bpp > 4)))
        return format("texture %d: bad image dimensions", i);
      if (t.width > 0 && (t.texelOffset < 0 || t.texelOffset + (int64_t)t.width * t.height * t.bpp > d->numTexelBytes))
        return format("texture %d: texels out of range", i);
    } else if (t.kind != SRT_TEX_SOLID)
      return format("texture %d: unknown kind %d", i, t.kind);
  }
  auto texOk = [&](int id) { return id >= -1 && id < d->numTextures; };
  for (int i = 0; i < d->numMaterials; ++i) {
    const SrtMaterialIn& m = d->materials[i];
    if (m.type < SRT_MAT_PBR || m.type > SRT_MAT_LIGHT) return format("material %d: unknown type %d", i, m.type);
    if (!texOk(m.albedoTex) || !texOk(m.normalTex) || !texOk(m.metallicTex) || !texOk(m.roughnessTex))
      return format("material %d: texture id out of range", i);
    if (m.type == SRT_MAT_LIGHT && m.albedoTex < 0) return format("material %d: light without emit texture", i);
  }
  for (int i = 0; i < d->numTriangles; ++i)
    if (d->triangles[i].material < 0 || d->triangles[i].material >= d->numMaterials)
      return format("triangle %d: material out of range", i);
  for (int i = 0; i < d->numSpheres; ++i)
    if (d->spheres[i].material < 0 || d->spheres[i].material >= d->numMaterials)
      return format("sphere %d: material out of range", i);
  for (int i = 0; i < d->numPrims; ++i) {
    const SrtPrimRef& p = d->prims[i];
    int lim = p.type == SRT_PRIM_SPHERE ? d->numSpheres : p.type == SRT_PRIM_TRIANGLE ? d->numTriangles : -1;
    if (p.index < 0 || p.index >= lim) return format("prim %d: bad type/index", i);
  }
  if (d->numWorld < 1) return "scene has an empty world list";
  for (int w = 0; w < d->numWorld; ++w) {
    const SrtWorldItem& it = d->world[w];
    if (it.first < 0 || it.count < 1 || it.first + it.count > d->numPrims || (it.kind != SRT_WORLD_PRIM && it.kind != SRT_WORLD_BVH))
      return format("world item %d: bad range", w);
    if (it.kind == SRT_WORLD_BVH && it.nodes) {
      // a caller-built tree must be finite and acyclic: children point forward (pre-order)
      // ... and a tree: every node but the root has exactly one parent (the pending-stack capacity is
      // derived per node from its single parent, buildItem)
      if (it.numNodes < 1) return format("world item %d: prebuilt tree without nodes", w);
      std::vector<uint8_t> parents(it.numNodes, 0);
      for (int i = 0; i < it.numNodes; ++i) {
        const int32_t l = it.nodes[i].left, r = it.nodes[i].right;
        for (int32_t c : {l, r}) {
          if (c >= 0 ? (c <= i || c >= it.numNodes) : (~c < it.first || ~c >= it.first + it.count))
            return format("world item %d: prebuilt node %d has a bad child reference %d", w, i, c);
        }
        if (l >= 0 && ++parents[l] > 1) return format("world item %d: prebuilt node %d has more than one parent", w, l);
        if (r >= 0 && r != l && ++parents[r] > 1) return format("world item %d: prebuilt node %d has more than one parent", w, r);
        if (r >= 0 && r == l) return format("world item %d: prebuilt node %d lists one subtree twice", w, i);
      }
      for (int i = 1; i < it.numNodes; ++i)
        if (!parents[i]) return format("world item %d: prebuilt node %d is unreachable", w, i);
    }
  }
  return std::string();
}

// ------------------------------------------------------------------ the stages of flattenScene, in its order
namespace {

// ~primListIndex -> device prim ref.  triDevIndex (HostScene::triDevIndex): the device index of a triangle, empty = identity
int32_t devRef(const SrtSceneDesc* d, const std::vector<int32_t>& triDevIndex, int32_t listRef) {
  const SrtPrimRef& p = d->prims[~listRef];
  if (p.type == SRT_PRIM_SPHERE) return ~((p.index << 1) | 1);
  return ~((triDevIndex.empty() ? p.index : triDevIndex[p.index]) << 1);
}

// box of node i of a float4 node array (two records per node: min, max)
Box nodeBox(const std::vector<float4>& nodes, size_t i) {
  const float4 &mn = nodes[2 * i], &mx = nodes[2 * i + 1];
  return Box{{mn.x, mn.y, mn.z}, {mx.x, mx.y, mx.z}};
}

// Primitive records.  Device arrays are indexed by the scene's own triangle / sphere indices; the owning list index is
// kept for srtTraceRays' prim output.
void primitiveRecords(const SrtSceneDesc* d, HostScene& h) {
  h.triPrimId.assign(d->numTriangles, -1);
  h.sphPrimId.assign(d->numSpheres, -1);
  for (int i = 0; i < d->numPrims; ++i) {
    const SrtPrimRef& p = d->prims[i];
    (p.type == SRT_PRIM_SPHERE ? h.sphPrimId : h.triPrimId)[p.index] = i;
  }
  h.triTest.resize((size_t)d->numTriangles * 3);
  h.triShade.resize((size_t)d->numTriangles * 4);
  h.triFast.resize((size_t)d->numTriangles * SRT_TRI_FAST_SLOTS);
  for (int i = 0; i < d->numTriangles; ++i) {
    const SrtTriangleIn& t = d->triangles[i];
    triangleRecords(&t.p[0][0], &t.uv[0][0], bitsAs<float>(&t.material), &h.triTest[3 * (size_t)i], &h.triShade[4 * (size_t)i],
                    &h.triFast[SRT_TRI_FAST_SLOTS * (size_t)i]);
  }
  h.spheres.resize((size_t)d->numSpheres * 3);
  for (int i = 0; i < d->numSpheres; ++i) {
    const SrtSphereIn& s = d->spheres[i];
    sphereRecords(vec3(s.center0), vec3(s.center1), s.time0, s.time1, s.radius, s.material, &h.spheres[3 * (size_t)i]);
  }
}

// The world: builds each bvhNode (consumes the global generator in scene order), adopts the caller-built trees and reserves
// the node slots of the device-built ones.  Returns whether a tree was adopted: its inner boxes are the caller's, not unions
// of its leaves'.
bool buildTrees(const SrtSceneDesc* d, HostScene& h) {
  h.itemNodes.resize(d->numWorld);
  bool adopted = false;
  for (int w = 0; w < d->numWorld; ++w) {
    const SrtWorldItem& it = d->world[w];
    adopted = adopted || (it.kind == SRT_WORLD_BVH && it.nodes);
    if (it.kind == SRT_WORLD_PRIM) {
      h.world.push_back(devRef(d, h.triDevIndex, ~it.first));
      continue;
    }
    if (!it.nodes && (it.builder == SRT_BUILDER_LBVH || it.builder == SRT_BUILDER_PLOC)) {
      // device build (srt_lbvh.hip) after the primitive arrays are uploaded: reserve the node slots
      int32_t base = (int32_t)(h.nodes.size() / 2), cnt = std::max(it.count - 1, 1);
      h.nodes.resize(h.nodes.size() + 2 * (size_t)cnt, make_float4(0, 0, 0, 0));
      h.nodeAxis.resize(h.nodeAxis.size() + cnt, 3);
      h.deviceBuilds.push_back(DeviceBuild{w, base, cnt, it.builder, it.time0, it.time1, {}});
      h.world.push_back(SRT_NODE_REF(base));
      continue;
    }
    Builder b;
    buildItem(d, it, b);
    // (A device order with the two children of a node in one 64-byte line -- root, then sibling pairs depth-first --
    // was measured against this pre-order, where the LEFT child follows its parent: headline +0.3 %, 1 M-triangle
    // soup -5 %, 10 M +1.7 %, profiles/r02/node_pairs.txt.  Not kept.)
    int32_t base = (int32_t)(h.nodes.size() / 2);
    h.itemNodes[w].resize(b.nodes.size());
    b.toBvhNodes(h.itemNodes[w].data());
    for (const BuildNode& n : b.nodes) {
      int32_t l = n.left >= 0 ? SRT_NODE_REF(n.left + base) : devRef(d, h.triDevIndex, n.left);
      int32_t r = n.right >= 0 ? SRT_NODE_REF(n.right + base) : devRef(d, h.triDevIndex, n.right);
      h.nodes.push_back(make_float4(n.box.mn[0], n.box.mn[1], n.box.mn[2], bitsAs<float>(&l)));
      h.nodes.push_back(make_float4(n.box.mx[0], n.box.mx[1], n.box.mx[2], bitsAs<float>(&r)));
      h.nodeAxis.push_back(n.axis);
    }
    h.world.push_back(SRT_NODE_REF(base));
    h.hostTrees.push_back(HostTree{w, base, (int32_t)b.nodes.size(), it.time0, it.time1});
    h.stackDepth = std::max(h.stackDepth, b.maxPending);
    // tree depth for reporting: longest root->node chain
    std::vector<int> depth(b.nodes.size(), 1);
    for (size_t i = 0; i < b.nodes.size(); ++i) {  // pre-order: parents precede children
      h.bvhDepth = std::max(h.bvhDepth, depth[i]);
      if (b.nodes[i].left >= 0) depth[b.nodes[i].left] = depth[i] + 1;
      if (b.nodes[i].right >= 0) depth[b.nodes[i].right] = depth[i] + 1;
    }
  }
  return adopted;
}

// Materials, textures and texels; the error text.  typeBits: per material its type and SRT_MAT_TEXTURED, as the primitives'
// material words and the shading records carry them.
std::string materialRecords(const SrtSceneDesc* d, HostScene& h, std::vector<int32_t>& typeBits) {
  h.materials.resize(d->numMaterials);
  typeBits.resize(d->numMaterials);
  for (int i = 0; i < d->numMaterials; ++i) {
    const SrtMaterialIn& m = d->materials[i];
    DevMaterial& dm = h.materials[i];
    memset(&dm, 0, sizeof dm);
    dm.type = m.type;
    dm.albedoTex = m.albedoTex; dm.normalTex = m.normalTex; dm.metallicTex = m.metallicTex; dm.roughnessTex = m.roughnessTex;
    memcpy(dm.albedo, m.albedo, 16);
    dm.metalness = m.type == SRT_MAT_METAL ? (m.fuzz < 1.0f ? m.fuzz : 1.0f)  // material.h:89
                   : m.type == SRT_MAT_DIELECTRIC ? m.ir : m.metalness;
    dm.roughness = m.roughness;
    // which hitRecord fields this material can observe (srt_path.h sphereRecord/triRecord)
    auto readsUv = [&](int tex) {
      if (tex < 0) return false;
      const SrtTextureIn& t = d->textures[tex];
      if (t.kind == SRT_TEX_IMAGE) return true;
      if (t.kind == SRT_TEX_CHECKER) return d->textures[t.even].kind == SRT_TEX_IMAGE || d->textures[t.odd].kind == SRT_TEX_IMAGE;
      return false;
    };
    bool uv = readsUv(m.albedoTex);
    if (m.type == SRT_MAT_PBR) uv = uv || readsUv(m.normalTex) || readsUv(m.metallicTex) || readsUv(m.roughnessTex);
    dm.flags = (uv ? 1 : 0) | ((m.type == SRT_MAT_PBR && m.normalTex >= 0) ? 2 : 0);
    const bool textured = m.type == SRT_MAT_PBR && (m.albedoTex >= 0 || m.normalTex >= 0 || m.metallicTex >= 0 || m.roughnessTex >= 0);
    typeBits[i] = (m.type & 3) | (textured ? SRT_MAT_TEXTURED : 0);
  }
  // textures: 3-byte images are padded to one aligned dword per texel, so a lookup is one
  // buffer_load_dword; 1- and 2-byte images keep their byte rows (the 1-bpp quirk of texture.h:147 reads the
  // neighbouring texels), followed by two zero bytes: that read reaches up to two bytes past the image's last texel,
  // which are 0 by definition whatever texture comes next in this buffer
  h.textures.resize(d->numTextures);
  for (int i = 0; i < d->numTextures; ++i) {
    const SrtTextureIn& t = d->textures[i];
    DevTexture& dt = h.textures[i];
    memset(&dt, 0, sizeof dt);
    dt.kind = t.kind; dt.width = t.width; dt.height = t.height; dt.bpp = t.bpp;
    dt.even = t.even; dt.odd = t.odd;
    memcpy(dt.color, t.color, 12);
    if (t.kind != SRT_TEX_IMAGE || t.width == 0) continue;
    const size_t n = (size_t)t.width * t.height;
    const uint8_t* src = d->texels + t.texelOffset;
    h.texels.resize((h.texels.size() + 3) & ~(size_t)3);  // dword aligned
    dt.offset = (int64_t)h.texels.size();
    if (t.bpp == 3) {
      const size_t at = h.texels.size();
      h.texels.resize(at + 4 * n);
      for (size_t k = 0; k < n; ++k) {
        h.texels[at + 4 * k + 0] = src[3 * k + 0];
        h.texels[at + 4 * k + 1] = src[3 * k + 1];
        h.texels[at + 4 * k + 2] = src[3 * k + 2];
        h.texels[at + 4 * k + 3] = 255;
      }
    } else {
      h.texels.insert(h.texels.end(), src, src + n * t.bpp);
      if (t.bpp < 3) h.texels.insert(h.texels.end(), 2, (uint8_t)0);
    }
    if (h.texels.size() > (size_t)0x7fffff00) return "scene: more than 2 GiB of texels";
  }
  return std::string();
}

// The material's flags ride in every primitive's material word (srt_device.h SRT_MAT_FLAGS_SHIFT), and the hit step's
// 128-byte shading records (srt_path.h shade; their layout is under "materials" there); the error text.
std::string shadingRecords(const SrtSceneDesc* d, const std::vector<int32_t>& typeBits, HostScene& h) {
  if (d->numMaterials > SRT_MAT_INDEX_MASK) return format("scene: more than %d materials", SRT_MAT_INDEX_MASK);
  auto withFlags = [&](float& word) {
    int32_t bits = bitsAs<int32_t>(&word);
    const int32_t m = bits & SRT_MAT_INDEX_MASK;
    if (m < d->numMaterials) bits |= (h.materials[m].flags & 3) << SRT_MAT_FLAGS_SHIFT | typeBits[m] << SRT_MAT_TYPE_SHIFT;
    word = bitsAs<float>(&bits);
  };
  for (int i = 0; i < d->numTriangles; ++i) withFlags(h.triShade[4 * (size_t)i + 3].w);
  for (int i = 0; i < d->numSpheres; ++i) withFlags(h.spheres[3 * (size_t)i + 1].w);
  h.shadeRecs.assign((size_t)8 * d->numMaterials, make_uint4(0, 0, 0, 0));
  for (int i = 0; i < d->numMaterials; ++i) {
    const DevMaterial& m = h.materials[i];
    auto f2u = [](float f) { return bitsAs<uint32_t>(&f); };
    uint4* r = &h.shadeRecs[(size_t)8 * i];
    r[0] = make_uint4((uint32_t)typeBits[i], (uint32_t)m.flags, f2u(m.metalness), f2u(m.roughness));
    r[1] = make_uint4(f2u(m.albedo[0]), f2u(m.albedo[1]), f2u(m.albedo[2]), f2u(m.albedo[3]));
    const int32_t ids[4] = {m.albedoTex, m.normalTex, m.metallicTex, m.roughnessTex};
    // +32: the emit texture of a light, in full
    if (m.type == SRT_MAT_LIGHT && ids[0] >= 0) {
      const DevTexture& t = h.textures[ids[0]];
      if (t.kind == SRT_TEX_SOLID)
        r[2] = make_uint4(SRT_SLOT_SOLID, f2u(t.color[0]), f2u(t.color[1]), f2u(t.color[2]));
      else if (t.kind == SRT_TEX_IMAGE && t.width == 0)
        r[2] = make_uint4(SRT_SLOT_SOLID, f2u(1.0f), f2u(0.0f), f2u(1.0f));  // failed load: magenta (texture.h:130-131)
      else if (t.kind == SRT_TEX_IMAGE && t.bpp >= 3)
        r[2] = make_uint4(SRT_SLOT_IMAGE, (uint32_t)t.width, (uint32_t)t.height, (uint32_t)t.offset);
      else
        r[2] = make_uint4(SRT_SLOT_GENERIC, (uint32_t)ids[0], 0, 0);  // checker, 1- and 2-byte images: texValue
    }
    // +48, +64: the four pbr slots, two dwords each
    uint32_t packed[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) {
      if (ids[k] < 0) continue;  // SRT_SLOT_NONE
      const DevTexture& t = h.textures[ids[k]];
      if (t.kind == SRT_TEX_IMAGE && t.bpp >= 3 && t.width > 0 && t.width < 32768 && t.height < 32768) {
        packed[2 * k] = SRT_SLOT_IMAGE | (uint32_t)t.width << 2 | (uint32_t)t.height << 17;
        packed[2 * k + 1] = (uint32_t)t.offset;
      } else {
        packed[2 * k] = SRT_SLOT_GENERIC;  // everything else goes through texValue on the id
        packed[2 * k + 1] = (uint32_t)ids[k];
      }
    }
    // an albedo slot that is checker(solidColor, solidColor): both colours into the record (+80 even, +96 odd)
    if (m.type == SRT_MAT_PBR && ids[0] >= 0 && h.textures[ids[0]].kind == SRT_TEX_CHECKER) {
      const DevTexture& c = h.textures[ids[0]];
      if (c.even >= 0 && c.odd >= 0 && c.even < (int)h.textures.size() && c.odd < (int)h.textures.size() && h.textures[c.even].kind == SRT_TEX_SOLID &&
          h.textures[c.odd].kind == SRT_TEX_SOLID) {
        packed[0] = SRT_SLOT_CHECKER2;
        r[5] = make_uint4(f2u(h.textures[c.even].color[0]), f2u(h.textures[c.even].color[1]), f2u(h.textures[c.even].color[2]), 0);
        r[6] = make_uint4(f2u(h.textures[c.odd].color[0]), f2u(h.textures[c.odd].color[1]), f2u(h.textures[c.odd].color[2]), 0);
      }
    }
    r[3] = make_uint4(packed[0], packed[1], packed[2], packed[3]);
    r[4] = make_uint4(packed[4], packed[5], packed[6], packed[7]);
  }
  return std::string();
}

// Triangle records in tree order.  Device arrays were filled in the scene's own triangle order; a tree's leaves reference them
// at random (a mesh's index order has nothing to do with the median splits), and with millions of triangles every test is then
// a 48-byte gather from a cold place.  Renumber the triangles by their first appearance in the (pre-order) node arrays of the
// host-built trees: the two triangles of a leaf and the leaves of a subtree become neighbours in memory.  Triangles no
// host-built tree references keep their relative order behind them.  References are rewritten, nothing else changes (primitive
// ids reported by srtTraceRays go through triPrimId, which is permuted along).  Leaves the renumbering in h.triDevIndex.
void reorderTriangles(const SrtSceneDesc* d, HostScene& h) {
  if (d->numTriangles <= 1 || h.nodes.empty()) return;
  std::vector<int32_t> order(d->numTriangles, -1);
  int32_t next = 0;
  auto visit = [&](float bits) {
    const int32_t r = bitsAs<int32_t>(&bits);
    if (r >= 0 || r == SRT_REF_DONE) return;
    const int32_t pr = ~r;
    if ((pr & 1) == 0 && (pr >> 1) < d->numTriangles && order[pr >> 1] < 0) order[pr >> 1] = next++;
  };
  for (size_t i = 0; i + 1 < h.nodes.size(); i += 2) {
    visit(h.nodes[i].w);
    visit(h.nodes[i + 1].w);
  }
  if (next == 0) return;
  for (int32_t i = 0; i < d->numTriangles; ++i)
    if (order[i] < 0) order[i] = next++;
  auto remap = [&](int32_t r) {
    if (r >= 0 || r == SRT_REF_DONE || (~r & 1)) return r;
    return ~(order[~r >> 1] << 1);
  };
  for (float4& v : h.nodes) {
    const int32_t r = remap(bitsAs<int32_t>(&v.w));
    v.w = bitsAs<float>(&r);
  }
  for (int32_t& wr : h.world) wr = remap(wr);
  auto permute = [&](auto& records, size_t slots) {  // triangle i's `slots` elements to where triangle order[i]'s go
    typename std::remove_reference<decltype(records)>::type moved(records.size());
    for (int32_t i = 0; i < d->numTriangles; ++i) std::copy_n(&records[slots * (size_t)i], slots, &moved[slots * (size_t)order[i]]);
    records.swap(moved);
  };
  permute(h.triTest, 3);
  permute(h.triShade, 4);
  permute(h.triFast, SRT_TRI_FAST_SLOTS);
  permute(h.triPrimId, 1);
  h.triDevIndex.swap(order);
}

// What holds of every box of the scene, the host-built nodes' and the device-built items' primitives': every coordinate is a
// fastDivOperand, every box is srtBoxOrdered (srt_records.h)
struct BoxCertificates {
  bool certified, ordered;
};

// Device-built trees: their primitives as device references.  Their node boxes are unions of primitive boxes, so fastDiv's
// certificate covers those as well as the host-built nodes.  The sign form of the slab test asks for ordered boxes as well
// (a union of ordered boxes is ordered); the slots of the device-built items are zero here.
BoxCertificates certifyBoxes(const SrtSceneDesc* d, const SceneOptions& o, HostScene& h) {
  BoxCertificates c{true, true};
  for (size_t i = 0; i < h.nodes.size() / 2; ++i) {
    c.certified = c.certified && fastDivOperands(nodeBox(h.nodes, i));
    c.ordered = c.ordered && srtBoxOrdered(nodeBox(h.nodes, i));
  }
  for (DeviceBuild& db : h.deviceBuilds) {
    const SrtWorldItem& it = d->world[db.item];
    db.refs.resize(it.count);
    for (int i = 0; i < it.count; ++i) {
      db.refs[i] = devRef(d, h.triDevIndex, ~(it.first + i));
      const Box pb = primBox(d, it.first + i, it.time0, it.time1);
      c.certified = c.certified && fastDivOperands(pb);
      c.ordered = c.ordered && srtBoxOrdered(pb);
    }
  }
  h.fastDivScene = c.certified ? o.fastDiv : 0;
  h.boxOrderedScene = c.ordered ? 1 : 0;
  return c;
}

// What the LDS-resident-tree kernels walk, for a world of host-built trees only.  Thread links (srt_thread.h): the 16-bit
// form (DevScene::nodeThread), and for a tree that does not fit into LDS the path-pool kernel's hybrid records (32-bit
// references, resident nodes first).
void walkForms(const SrtSceneDesc* d, const SceneOptions& o, bool adopted, BoxCertificates c, HostScene& h) {
  if (!h.deviceBuilds.empty() || h.nodes.empty()) return;
  srtThreadLinks16(h.nodes, h.world, d->numTriangles, d->numSpheres, h.nodeThread);
  if (o.wfHybrid > 0) {
    const size_t n = h.nodes.size() / 2;
    const size_t fits = srtWfMaxResidentNodes(SRT_WF_HYBRID_POOL, true);  // beside the hybrid form's pool
    const size_t fitsWhole = srtWfMaxWholeTreeNodes();                    // the whole-tree form's smallest pool
    const size_t cap = o.wfResidentMax > 0 ? std::min<size_t>(fits, (size_t)o.wfResidentMax) : fits;
    if (n > (o.wfResidentMax > 0 ? cap : fitsWhole))
      h.wfResident = srtHybridRecords(h.nodes, h.world, d->numTriangles, d->numSpheres, cap, h.nodesWf, h.worldWf, h.primSecond, &h.wfIndex);
    if (h.nodesWf.empty()) h.wfIndex.clear();
  }
  // ---- the regrouped tree (srt_regroup.h) for the path-pool kernel's whole-tree form.  The builder is quadratic in a
  // tree's leaves at worst, so it runs only for what that form can take: thread links exist, no hybrid records were
  // made, and the node array fits a CU's LDS beside the smallest pool.  Its lemma wants the reference's inner boxes to
  // contain their leaves' (the trees built here; a caller-built tree promises nothing) and ordered boxes.  The planes of
  // its inner boxes are planes of the leaves, so fastDivScene and boxOrderedScene hold for it as they stand.
  if (h.nodeThread.empty() || !h.nodesWf.empty() || adopted || !c.ordered || h.nodes.size() / 2 > (size_t)srtWfMaxWholeTreeNodes() ||
      !srtRegroupNodes(h.nodes, h.world, h.nodesRg))
    return;
  srtThreadLinks16(h.nodesRg, h.world, d->numTriangles, d->numSpheres, h.nodeThreadRg);
  bool same = !h.nodeThreadRg.empty();
  for (size_t i = 0; same && i < h.nodesRg.size() / 2; ++i)
    same = (!c.certified || fastDivOperands(nodeBox(h.nodesRg, i))) && srtBoxOrdered(nodeBox(h.nodesRg, i));
  if (!same) {  // (cannot happen: see srt_regroup.h unite)
    h.nodesRg.clear();
    h.nodeThreadRg.clear();
  }
  // ---- its walk sequence: the gates that rarely cull a ray elided (linear in the array)
  SrtRegroupWalk walk;
  if (!h.nodesRg.empty() && srtRegroupWalk(h.nodesRg, h.world, walk)) {
    h.numWalk = (int32_t)walk.src.size();
    h.wfHead = walk.head;
    h.walkSeq.reserve(3 * walk.src.size() + walk.entry.size());
    for (size_t j = 0; j < walk.src.size(); ++j) h.walkSeq.insert(h.walkSeq.end(), {walk.src[j], walk.links[2 * j], walk.links[2 * j + 1]});
    h.walkSeq.insert(h.walkSeq.end(), walk.entry.begin(), walk.entry.end());
  }
}

// Material class per primitive reference (DevScene::primClass)
void primClasses(const SrtSceneDesc* d, HostScene& h) {
  auto classOf = [&](float word, bool sphere) -> uint8_t {
    const int32_t bits = bitsAs<int32_t>(&word);
    const int type = (bits >> SRT_MAT_TYPE_SHIFT) & 3, flags = (bits >> SRT_MAT_FLAGS_SHIFT) & 3;
    if (type != SRT_MAT_PBR) return 2;
    if (!sphere) return 0;
    // a sphere whose pbr material reads uv or a normal map (the textured iron sphere: acosf / atan2f, a tangent frame,
    // four lookups) would make every hit step of the plain spheres (the ground) run that code too: it goes with "the rest"
    return flags ? 2 : 1;
  };
  h.primClass.assign((size_t)2 * std::max(d->numTriangles, d->numSpheres) + 2, 2);
  for (int i = 0; i < d->numTriangles; ++i) h.primClass[(size_t)i << 1] = classOf(h.triShade[4 * (size_t)i + 3].w, false);
  for (int i = 0; i < d->numSpheres; ++i) h.primClass[((size_t)i << 1) | 1] = classOf(h.spheres[3 * (size_t)i + 1].w, true);
}

}  // namespace

// The stages in the one order that works; each call's comment says what it must follow.  (tests/test_scene_host.py pins
// every member they fill, bit for bit.)
std::string flattenScene(const SrtSceneDesc* d, const SceneOptions& o, HostScene& h) {
  primitiveRecords(d, h);
  const bool adopted = buildTrees(d, h);  // before reorderTriangles: h.triDevIndex is empty, references are in scene order
  if (h.nodes.size() / 2 > (size_t)SRT_MAX_NODES)
    return format("scene: %zu BVH nodes exceed the %d the device references can address", h.nodes.size() / 2, SRT_MAX_NODES);
  std::vector<int32_t> typeBits;
  std::string err = materialRecords(d, h, typeBits);
  if (err.empty()) err = shadingRecords(d, typeBits, h);  // after primitiveRecords and materialRecords: tags the material words
  if (!err.empty()) return err;
  reorderTriangles(d, h);                           // after buildTrees (its order is their leaves') and shadingRecords (tagged words move)
  const BoxCertificates c = certifyBoxes(d, o, h);  // after reorderTriangles: the device-built items' references go through it
  walkForms(d, o, adopted, c, h);                   // after certifyBoxes: regroups only what it certified, and checks the result by it
  primClasses(d, h);                                // after shadingRecords and reorderTriangles: the tagged words, in device order
  return std::string();
}

// From a flattened scene, nothing of which it changes: the spheres whose material is a light with a solid-colour emit slot
// (SRT_SLOT_SOLID in its shading record), as device sphere indices in prims[] order.  A moving sphere is listed too: whether
// it moves is read from its record where the table is used.
std::vector<int32_t> sampledLights(const HostScene& h) {
  std::vector<std::pair<int32_t, int32_t>> found;  // (prims[] index, device index)
  const int32_t numMaterials = (int32_t)(h.shadeRecs.size() / 8);
  for (size_t i = 0; i < h.sphPrimId.size(); ++i) {
    const int32_t word = bitsAs<int32_t>(&h.spheres[3 * i + 1].w);
    const int32_t m = word & SRT_MAT_INDEX_MASK;
    if (m >= numMaterials || h.materials[m].type != SRT_MAT_LIGHT || h.shadeRecs[(size_t)8 * m + 2].x != SRT_SLOT_SOLID) continue;
    found.emplace_back(h.sphPrimId[i], (int32_t)i);
  }
  std::sort(found.begin(), found.end());
  std::vector<int32_t> out;
  for (const auto& f : found) out.push_back(f.second);
  return out;
}

extern "C" {

float srtHostRandomFloat(void) { return hostRandomFloat(); }
void srtHostRandomReset(void) { hostGenerator().seed(std::mt19937::default_seed); }

// camera.h:10-38
int srtMakeCamera(const SrtCameraParams* in, SrtCamera* out) {
  if (!in || !out) return 1;
  const float pi = 3.1415926535897932385f;
  Vec3 eye = vec3(in->eye), lookAt = vec3(in->lookAt), up = vec3(in->up);
  float theta = in->vfovDegrees * pi / 180.0f;  // deg2rad, globals.h:26-28
  double h = tan((double)(theta / 2.0f));       // camera.h:20: tan(float) is the double overload
  double vpHeight = 2.0f * h;
  double vpWidth = in->aspect * vpHeight;
  Vec3 w = unit(eye - lookAt);
  Vec3 hor = unit(cross(up, w));
  Vec3 vert = unit(cross(w, hor));
  Vec3 horizontal = (float)(in->focusDist * vpWidth) * hor;  // Eigen casts the double scalar to float
  Vec3 vertical = (float)(in->focusDist * vpHeight) * vert;
  Vec3 lleft = eye - horizontal / 2.0f - vertical / 2.0f - in->focusDist * w;
  const Vec3* src[] = {&eye, &lleft, &horizontal, &vertical, &w, &hor, &vert};
  float* dst[] = {out->origin, out->lleft, out->horizontal, out->vertical, out->w, out->hor, out->vert};
  for (int i = 0; i < 7; ++i) {
    dst[i][0] = src[i]->x;
    dst[i][1] = src[i]->y;
    dst[i][2] = src[i]->z;
  }
  out->lensRadius = in->aperture / 2.0f;
  out->time0 = in->time0;
  out->time1 = in->time1;
  return 0;
}

}  // extern "C"
