// ref_harness.cpp -- runs the REFERENCE's own hot-path headers, unmodified, as g++ compiles them.
//
// TEST INFRASTRUCTURE ONLY.  A stand-alone program: the reference's generator is a function-local static
// (globals.h:30-35) that cannot be reseeded, so only a fresh process starts it at the default seed.  One job per
// invocation; inputs and outputs are binary files that tests/ref_harness.py writes and reads.
//
// The reference's headers are found with -I (oracle/Makefile), against the stand-ins of oracle/refshim/ for Eigen, stb
// and cgltf.  This file holds no line of the reference: what cannot be included -- the path loop and the pixel loop live
// in main.cpp next to gl.h -- is written here as the project's own code with the file:line it follows, the way oracle.cpp
// does.  Scenes are built with the reference's own constructors from the same abi.SceneBuilder content the oracle and
// the GPU get.  Built with g++ only: the draw order of vec3.h:42,46,90 is g++'s argument evaluation order.
//
// The binary goes to oracle/_ref/, which is never committed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

// this order
#include "globals.h"
#include "color.h"
#include "hittablelist.h"
#include "sphere.h"
#include "camera.h"
#include "material.h"
#include "bvh.h"
#include "model.h"

#include "../include/srt_hip.h"

static_assert(sizeof(vec3f) == 12 && sizeof(vec2f) == 8, "model.h:343,359 read the buffer as packed floats");

[[noreturn]] static void die(const std::string& what) {
  std::cerr << "ref_harness: " << what << "\n";
  std::exit(2);
}

static std::vector<uint8_t> readFile(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) die("cannot read " + path);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Out {
  std::ofstream f;
  explicit Out(const std::string& path) : f(path, std::ios::binary) {
    if (!f) die("cannot write " + path);
  }
  template <typename T>
  void put(const T& v) { f.write(reinterpret_cast<const char*>(&v), sizeof(T)); }
  void put(const void* p, size_t n) { f.write(static_cast<const char*>(p), (std::streamsize)n); }
};

struct In {
  std::vector<uint8_t> b;
  size_t at = 0;
  explicit In(const std::string& path) : b(readFile(path)) {}
  template <typename T>
  T get() {
    T v;
    take(&v, sizeof(T));
    return v;
  }
  void take(void* p, size_t n) {
    if (at + n > b.size()) die("input file too short");
    memcpy(p, b.data() + at, n);
    at += n;
  }
  template <typename T>
  std::vector<T> array(size_t n) {
    std::vector<T> v(n);
    if (n) take(v.data(), n * sizeof(T));
    return v;
  }
};

// ------------------------------------------------------------------ stb_image.h stand-in
// "<filename>.raw": int32 width, height, components, then the bytes as stb would return them for that many components
// (tests/ref_harness.py decodes with PIL).  A missing file is a failed load.  The block is the size stb would allocate
// plus two zero bytes: texture.h:147 reads pixel[1], pixel[2] of a 1-byte image's last texel from there.  texture.h:126
// releases it with `delete`, so it comes from operator new.
stbi_uc* stbi_load(char const* filename, int* x, int* y, int* channels_in_file, int desired_channels) {
  std::ifstream f(std::string(filename) + ".raw", std::ios::binary);
  if (!f) return nullptr;
  int32_t hdr[3];
  f.read(reinterpret_cast<char*>(hdr), sizeof(hdr));
  if (!f || hdr[2] != desired_channels) die(std::string("bad raw image ") + filename);
  size_t n = (size_t)hdr[0] * hdr[1] * hdr[2];
  stbi_uc* data = static_cast<stbi_uc*>(operator new(n + 2));
  f.read(reinterpret_cast<char*>(data), (std::streamsize)n);
  if (!f) die(std::string("short raw image ") + filename);
  data[n] = data[n + 1] = 0;
  *x = hdr[0];
  *y = hdr[1];
  *channels_in_file = hdr[2];
  return data;
}

// ------------------------------------------------------------------ cgltf.h stand-in
// "<path>.flat": the glTF's JSON flattened to whitespace-separated tokens by tests/ref_harness.py (floats as their
// binary32 bit patterns), "<path>.flat.buf<k>": buffer k's bytes.
struct FlatGltf {
  std::vector<cgltf_buffer> buffers;
  std::vector<std::vector<uint8_t>> bytes;
  std::vector<std::string> uris;
  std::vector<cgltf_image> images;
  std::vector<cgltf_texture> textures;
  std::vector<cgltf_material> materials;
  std::vector<cgltf_buffer_view> views;
  std::vector<cgltf_accessor> accessors;
  std::vector<cgltf_attribute> attributes;
  std::vector<cgltf_primitive> primitives;
  std::vector<cgltf_mesh> meshes;
  cgltf_data data;
};

static float bitsToFloat(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

cgltf_result cgltf_parse_file(const cgltf_options*, const char* path, cgltf_data** out) {
  std::ifstream f(std::string(path) + ".flat");
  if (!f) return cgltf_result_file_not_found;
  auto* g = new FlatGltf();
  std::string tag;
  size_t nBuffers, nImages, nMaterials, nViews, nAccessors, nAttributes, nPrimitives, nMeshes;
  f >> tag >> nBuffers;
  g->buffers.resize(nBuffers);
  g->bytes.resize(nBuffers);
  for (auto& b : g->buffers) { f >> b.size; b.data = nullptr; }
  f >> tag >> nImages;
  g->uris.resize(nImages);
  g->images.resize(nImages);
  g->textures.resize(nImages);  // one cgltf_texture per image: model.h only follows texture->image->uri
  for (size_t i = 0; i < nImages; i++) {
    f >> g->uris[i];
    g->images[i].uri = const_cast<char*>(g->uris[i].c_str());
    g->textures[i].image = &g->images[i];
  }
  auto texView = [&](long image) {
    cgltf_texture_view v;
    v.texture = image >= 0 ? &g->textures[(size_t)image] : nullptr;
    return v;
  };
  f >> tag >> nMaterials;
  g->materials.resize(nMaterials);
  for (auto& m : g->materials) {
    uint32_t bits[6];
    long base, normal, mr;
    f >> m.has_pbr_metallic_roughness;
    for (uint32_t& b : bits) f >> b;
    f >> base >> normal >> mr;
    for (int k = 0; k < 4; k++) m.pbr_metallic_roughness.base_color_factor[k] = bitsToFloat(bits[k]);
    m.pbr_metallic_roughness.metallic_factor = bitsToFloat(bits[4]);
    m.pbr_metallic_roughness.roughness_factor = bitsToFloat(bits[5]);
    m.pbr_metallic_roughness.base_color_texture = texView(base);
    m.pbr_metallic_roughness.metallic_roughness_texture = texView(mr);
    m.normal_texture = texView(normal);
  }
  f >> tag >> nViews;
  g->views.resize(nViews);
  for (auto& v : g->views) {
    size_t buffer;
    f >> buffer >> v.offset;
    v.buffer = &g->buffers.at(buffer);
  }
  f >> tag >> nAccessors;
  g->accessors.resize(nAccessors);
  for (auto& a : g->accessors) {
    int type;
    size_t view;
    f >> type >> a.count >> view;
    a.type = static_cast<cgltf_type>(type);
    a.buffer_view = &g->views.at(view);
  }
  f >> tag >> nAttributes;
  g->attributes.resize(nAttributes);
  for (auto& a : g->attributes) {
    int type;
    size_t accessor;
    f >> type >> accessor;
    a.type = static_cast<cgltf_attribute_type>(type);
    a.data = &g->accessors.at(accessor);
  }
  f >> tag >> nPrimitives;
  g->primitives.resize(nPrimitives);
  for (auto& p : g->primitives) {
    int type;
    long indices, material;
    size_t firstAttribute;
    f >> type >> indices >> material >> firstAttribute >> p.attributes_count;
    p.type = static_cast<cgltf_primitive_type>(type);
    p.indices = indices >= 0 ? &g->accessors.at((size_t)indices) : nullptr;
    p.material = material >= 0 ? &g->materials.at((size_t)material) : nullptr;
    p.attributes = g->attributes.data() + firstAttribute;
  }
  f >> tag >> nMeshes;
  g->meshes.resize(nMeshes);
  for (auto& m : g->meshes) {
    size_t firstPrimitive;
    f >> firstPrimitive >> m.primitives_count;
    m.primitives = g->primitives.data() + firstPrimitive;
  }
  f >> tag;
  if (!f || tag != "end") die(std::string("bad flattened glTF ") + path);
  g->data.meshes = g->meshes.data();
  g->data.meshes_count = nMeshes;
  g->data.owner = g;
  *out = &g->data;
  return cgltf_result_success;
}

cgltf_result cgltf_load_buffers(const cgltf_options*, cgltf_data* data, const char* path) {
  auto* g = static_cast<FlatGltf*>(data->owner);
  for (size_t k = 0; k < g->buffers.size(); k++) {
    g->bytes[k] = readFile(std::string(path) + ".flat.buf" + std::to_string(k));
    if (g->bytes[k].size() < g->buffers[k].size) return cgltf_result_io_error;
    g->buffers[k].data = g->bytes[k].data();
  }
  return cgltf_result_success;
}

void cgltf_free(cgltf_data* data) { delete static_cast<FlatGltf*>(data->owner); }

// ------------------------------------------------------------------ the generator's position
// The static generator cannot be read.  Four draws are taken and found again in a second default-seeded generator:
// the number of draws made before them.  Taking them moves the stream, so this is called once, last.
static uint64_t streamPosition() {
  float probe[4];
  for (float& p : probe) p = randomFloat();
  std::uniform_real_distribution<float> distribution(0.0f, 1.0f);
  std::mt19937 generator;
  float window[4];
  for (float& w : window) w = distribution(generator);
  for (uint64_t at = 0; at < (1ull << 36); at++) {
    if (!memcmp(window, probe, sizeof(probe))) return at;
    window[0] = window[1]; window[1] = window[2]; window[2] = window[3];
    window[3] = distribution(generator);
  }
  die("generator position not found");
}

// ------------------------------------------------------------------ scene
struct WorldItemIn {
  int32_t kind, first, count;
  float time0, time1;
  int32_t numNodes, builder;
};

struct Scene {
  uint64_t preDraws = 0;
  std::vector<shared_ptr<texture>> textures;
  std::vector<shared_ptr<material>> materials;
  std::vector<shared_ptr<hittable>> prims;  // list order
  std::vector<shared_ptr<mesh>> ownMeshes;  // the meshes made here for the scene file's triangles
  shared_ptr<model> gltfModel;
  std::unordered_map<const hittable*, int> primId;
  std::unordered_map<const material*, int> materialId;
  std::vector<shared_ptr<bvhNode>> roots;  // per BVH world item
  hittableList world;
};

static vec3f v3(const float* f) { return vec3f(f[0], f[1], f[2]); }

// Reads the scene file and builds it with the reference's constructors.  buildWorld = false stops before the world (no
// bvhNode, no draws): texture, emitted and scatter jobs.
static void loadScene(const std::string& path, Scene& s, bool buildWorld) {
  In in(path);
  if (in.get<uint32_t>() != 0x53525431u) die("not a scene file");
  int32_t nTri = in.get<int32_t>(), nSph = in.get<int32_t>(), nPrim = in.get<int32_t>(), nWorld = in.get<int32_t>();
  int32_t nMat = in.get<int32_t>(), nTex = in.get<int32_t>(), gltfLen = in.get<int32_t>();
  s.preDraws = in.get<uint64_t>();
  std::string gltfPath(gltfLen, ' ');
  in.take(&gltfPath[0], gltfLen);
  auto tris = in.array<SrtTriangleIn>(nTri);
  auto sphs = in.array<SrtSphereIn>(nSph);
  auto prims = in.array<SrtPrimRef>(nPrim);
  auto world = in.array<WorldItemIn>(nWorld);
  auto mats = in.array<SrtMaterialIn>(nMat);
  auto texs = in.array<SrtTextureIn>(nTex);

  // textures: solids and images first, checkers refer to them (abi.SceneBuilder.checker)
  s.textures.resize(nTex);
  for (int i = 0; i < nTex; i++) {
    const SrtTextureIn& t = texs[i];
    if (t.kind == SRT_TEX_SOLID)
      s.textures[i] = make_shared<solidColor>(color3f(t.color[0], t.color[1], t.color[2]));
    else if (t.kind == SRT_TEX_IMAGE)  // tests/ref_harness.py wrote ../data/tex<i>.raw unless the load is to fail
      s.textures[i] = make_shared<imagePNG>(("../data/tex" + std::to_string(i)).c_str(), t.bpp);
  }
  for (int i = 0; i < nTex; i++)
    if (texs[i].kind == SRT_TEX_CHECKER) s.textures[i] = make_shared<checker>(s.textures.at(texs[i].even), s.textures.at(texs[i].odd));
  auto tex = [&](int id) { return id >= 0 ? s.textures.at(id) : shared_ptr<texture>(); };

  for (int i = 0; i < nMat; i++) {
    const SrtMaterialIn& m = mats[i];
    shared_ptr<material> out;
    if (m.type == SRT_MAT_PBR) {
      // material.h:67-70 sets metalness, roughness and anisotropy (the shorter constructors leave them
      // uninitialised); the maps are public fields
      auto p = make_shared<pbrMetallicRoughness>(tex(m.albedoTex), vec4f(m.albedo[0], m.albedo[1], m.albedo[2], m.albedo[3]),
                                                 m.metalness, m.roughness);
      p->normalMap = tex(m.normalTex);
      p->metallicMap = tex(m.metallicTex);
      p->roughnessMap = tex(m.roughnessTex);
      out = p;
    } else if (m.type == SRT_MAT_METAL)
      out = make_shared<metal>(color3f(m.albedo[0], m.albedo[1], m.albedo[2]), m.fuzz);
    else if (m.type == SRT_MAT_DIELECTRIC)
      out = make_shared<dielectric>(m.ir);
    else
      out = make_shared<diffuseLight>(tex(m.albedoTex));
    s.materials.push_back(out);
    s.materialId[out.get()] = i;
  }
  if (!buildWorld) return;

  // the glTF model goes through model::create(...)->init(), i.e. gltfLoad (model.h:301-460); its triangles take the
  // place of the scene file's, which abi.SceneBuilder holds in the same order (main.cpp:82-86: every mesh, every triangle)
  std::vector<shared_ptr<hittable>> gltfTriangles;
  if (gltfLen) {
    s.gltfModel = model::create(gltfPath);
    if (!s.gltfModel->init()) die("gltfLoad failed on " + gltfPath);
    for (const auto& m : s.gltfModel->meshes) {
      if (!m->triangles.empty()) {
        size_t first = gltfTriangles.size();
        if (first >= tris.size()) die("glTF model has more triangles than the scene file");
        s.materialId[m->matPtr.get()] = tris[first].material;
      }
      for (const auto& t : m->triangles) gltfTriangles.push_back(t);
    }
    if ((int)gltfTriangles.size() != nTri) die("glTF model and scene file disagree on the triangle count");
  }

  // triangles: one mesh per run of one material, three vertices per triangle, 16-bit indices (model.h:46)
  shared_ptr<mesh> cur;
  int curMat = -1;
  for (int i = 0; i < nPrim; i++) {
    const SrtPrimRef& pr = prims[i];
    shared_ptr<hittable> h;
    if (pr.type == SRT_PRIM_TRIANGLE && gltfLen) {
      h = gltfTriangles.at(pr.index);
    } else if (pr.type == SRT_PRIM_TRIANGLE) {
      const SrtTriangleIn& t = tris.at(pr.index);
      if (!cur || curMat != t.material || cur->positions.size() + 3 > 65535) {
        cur = mesh::create();
        cur->matPtr = s.materials.at(t.material);
        curMat = t.material;
        s.ownMeshes.push_back(cur);
      }
      uint16_t base = (uint16_t)cur->positions.size();
      for (int k = 0; k < 3; k++) {
        cur->positions.push_back(vec3f(t.p[k][0], t.p[k][1], t.p[k][2]));
        cur->texcoords.push_back(vec2f(t.uv[k][0], t.uv[k][1]));
      }
      auto tri = triangle::create(base, (uint16_t)(base + 1), (uint16_t)(base + 2), cur);
      cur->triangles.push_back(tri);
      h = tri;
    } else {
      const SrtSphereIn& sp = sphs.at(pr.index);
      h = make_shared<sphere>(v3(sp.center0), v3(sp.center1), sp.time0, sp.time1, sp.radius, s.materials.at(sp.material));
    }
    s.prims.push_back(h);
    s.primId[h.get()] = i;
  }

  for (uint64_t k = 0; k < s.preDraws; k++) randomFloat();  // the scene's construction drew these first (main.cpp:92-122)
  for (const WorldItemIn& it : world) {
    if (it.kind == SRT_WORLD_PRIM) {
      s.world.add(s.prims.at(it.first));
    } else {
      if (it.numNodes || it.builder != SRT_BUILDER_REFERENCE) die("only the reference's own tree build can be compared");
      std::vector<shared_ptr<hittable>> objects(s.prims.begin() + it.first, s.prims.begin() + it.first + it.count);
      auto root = make_shared<bvhNode>(objects, 0, objects.size(), it.time0, it.time1);  // main.cpp:146
      s.roots.push_back(root);
      s.world.add(root);
    }
  }
}

// ------------------------------------------------------------------ the side-walk
// The reference's traversal once more over the public left/right/box members, with the reference's own box.hit and leaf
// hit, to read what hitRecord does not carry: the primitive and the four counters.  It follows hittablelist.h:33-47 and
// bvh.h:97-105; traceOne checks its record against world.hit's.
struct Walk {
  int prim = SRT_NO_HIT;
  int nodeVisits = 0, boxPasses = 0, triTests = 0, sphereTests = 0;
};

static bool walk(const Scene& s, const hittable* h, const ray& r, float tMin, float tMax, hitRecord& record, Walk& w) {
  if (const bvhNode* n = dynamic_cast<const bvhNode*>(h)) {
    w.nodeVisits++;
    if (!n->box.hit(r, tMin, tMax)) return false;
    w.boxPasses++;
    const bool single = n->left == n->right;  // bvh.h:67-69: the object is tested twice, counted once
    bool hitLeft = walk(s, n->left.get(), r, tMin, tMax, record, w);
    Walk afterLeft = w;
    bool hitRight = walk(s, n->right.get(), r, tMin, hitLeft ? record.t : tMax, record, w);
    if (single) {
      w.triTests = afterLeft.triTests;
      w.sphereTests = afterLeft.sphereTests;
    }
    return hitLeft || hitRight;
  }
  if (dynamic_cast<const triangle*>(h)) w.triTests++;
  else w.sphereTests++;
  if (!h->hit(r, tMin, tMax, record)) return false;
  w.prim = s.primId.at(h);
  return true;
}

static bool walkWorld(const Scene& s, const ray& r, float tMin, float tMax, hitRecord& record, Walk& w) {
  hitRecord temp;
  bool any = false;
  float closest = tMax;
  for (const auto& object : s.world.objects)
    if (walk(s, object.get(), r, tMin, closest, temp, w)) {  // a walk that misses leaves w.prim as it was
      any = true;
      closest = temp.t;
      record = temp;
    }
  return any;
}

static bool sameBits(const vec3f& a, const vec3f& b) { return !memcmp(&a, &b, sizeof(vec3f)); }

static void traceOne(const Scene& s, const SrtRay& in, SrtHit& out) {
  ray r(v3(in.o), v3(in.d), in.time);
  hitRecord viaWalk, viaWorld;
  Walk w;
  bool hitWalk = walkWorld(s, r, in.tMin, in.tMax, viaWalk, w);
  bool hitWorld = s.world.hit(r, in.tMin, in.tMax, viaWorld);
  if (hitWalk != hitWorld) die("side-walk and world.hit disagree on hit/miss");
  memset(&out, 0, sizeof(out));
  out.prim = SRT_NO_HIT;
  out.material = -1;
  out.nodeVisits = w.nodeVisits;
  out.boxPasses = w.boxPasses;
  out.triTests = w.triTests;
  out.sphereTests = w.sphereTests;
  if (!hitWorld) return;
  const hitRecord& a = viaWalk;
  const hitRecord& b = viaWorld;
  if (memcmp(&a.t, &b.t, 4) || !sameBits(a.p, b.p) || !sameBits(a.normal, b.normal) || !sameBits(a.tangent, b.tangent) ||
      !sameBits(a.bitangent, b.bitangent) || memcmp(&a.uv, &b.uv, 8) || a.frontFace != b.frontFace || a.matPtr != b.matPtr)
    die("side-walk and world.hit disagree on a record");
  out.prim = w.prim;
  out.t = b.t;
  for (int k = 0; k < 3; k++) {
    out.p[k] = b.p(k);
    out.normal[k] = b.normal(k);
    out.tangent[k] = b.tangent(k);
    out.bitangent[k] = b.bitangent(k);
  }
  out.uv[0] = b.uv(0);
  out.uv[1] = b.uv(1);
  out.frontFace = b.frontFace ? 1 : 0;
  out.material = s.materialId.at(b.matPtr.get());
}

// pre-order, in the product's SrtBvhNode format: a leaf child is ~(list index); a single-object node names it twice
static int flatten(const Scene& s, const hittable* h, std::vector<SrtBvhNode>& out, int depth, int& maxDepth) {
  const bvhNode* n = dynamic_cast<const bvhNode*>(h);
  if (!n) return ~s.primId.at(h);
  if (depth > maxDepth) maxDepth = depth;
  size_t at = out.size();
  out.emplace_back();
  int l = flatten(s, n->left.get(), out, depth + 1, maxDepth);
  int r = n->right == n->left ? l : flatten(s, n->right.get(), out, depth + 1, maxDepth);
  SrtBvhNode& o = out[at];
  for (int k = 0; k < 3; k++) {
    o.bmin[k] = n->box.minimum(k);
    o.bmax[k] = n->box.maximum(k);
  }
  o.left = l;
  o.right = r;
  return (int)at;
}

// ------------------------------------------------------------------ main.cpp:33-52, with the bounce limit's argument
static color3f rayColor(const ray& in, const color3f& sky, const hittable& world, int bouncesLeft) {
  if (bouncesLeft <= 0) return color3f(0, 0, 0);  // black, not the sky, when the bounces run out (main.cpp:36-37)
  hitRecord rec;
  if (!world.hit(in, 0.001f, infinity, rec)) return sky;  // main.cpp:39
  const color3f glow = rec.matPtr->emitted(rec.uv(0), rec.uv(1), rec.p);  // evaluated before scatter (main.cpp:44-46)
  ray out;
  color3f att;
  if (!rec.matPtr->scatter(in, rec, att, out)) return glow;
  const color3f deeper = rayColor(out, sky, world, bouncesLeft - 1);
  return glow + color3f(deeper(0) * att(0), deeper(1) * att(1), deeper(2) * att(2));  // main.cpp:49-51
}

// ------------------------------------------------------------------ jobs
static int jobRng(int n, const std::string& outPath) {  // the first n randomFloat() of a process
  Out out(outPath);
  for (int i = 0; i < n; i++) out.put(randomFloat());
  return 0;
}

static int jobVec3(const std::string& outPath) {  // randomVec3f(-1, 1) from process start
  Out out(outPath);
  vec3f v = randomVec3f(-1.0f, 1.0f);
  for (int k = 0; k < 3; k++) out.put(v(k));
  return 0;
}

static int jobTree(const std::string& scenePath, const std::string& outPath) {
  Scene s;
  loadScene(scenePath, s, true);
  Out out(outPath);
  out.put((int32_t)s.roots.size());
  for (const auto& root : s.roots) {
    std::vector<SrtBvhNode> nodes;
    int depth = 0;
    flatten(s, root.get(), nodes, 1, depth);
    out.put((int32_t)nodes.size());
    out.put((int32_t)depth);
    out.put(nodes.data(), nodes.size() * sizeof(SrtBvhNode));
  }
  out.put((uint64_t)streamPosition());  // preDraws + the draws of every bvhNode
  return 0;
}

static int jobTrace(const std::string& scenePath, const std::string& raysPath, const std::string& outPath) {
  Scene s;
  loadScene(scenePath, s, true);
  In in(raysPath);
  auto rays = in.array<SrtRay>(in.b.size() / sizeof(SrtRay));
  std::vector<SrtHit> hits(rays.size());
  for (size_t i = 0; i < rays.size(); i++) traceOne(s, rays[i], hits[i]);
  Out out(outPath);
  out.put(hits.data(), hits.size() * sizeof(SrtHit));
  return 0;
}

// The closest hit, which the reference itself never computes (its traversal can return a farther triangle); the
// project's closest-hit traversal mode is measured against it.  Two answers per ray, both with the reference's own leaf
// hit and the acceptance `t <= closest`:
//   tree   over the reference's tree, a node's children visited only where its own box.hit(r, tMin, closest) passes --
//          what any closest-hit traversal of this tree returns, whatever order it visits the children in (a tie apart);
//   brute  over every primitive of the list, no boxes.
// They differ where a box does not hold the hit: a hit exactly at tMax on a box face (aabb.h:22 culls tMax <= tMin), a
// ray grazing a face with a zero direction component (0 / 0 in aabb.h:14-17), a moving sphere outside [time0, time1].
// Answer per ray: int32 tree primitive, float tree t, int32 brute primitive, float brute t, int32 how many primitives
// hit at exactly the tree's t.
static void walkClosest(const Scene& s, const hittable* h, const ray& r, float tMin, float& closest, int32_t& prim, float& t) {
  if (const bvhNode* n = dynamic_cast<const bvhNode*>(h)) {
    if (!n->box.hit(r, tMin, closest)) return;
    walkClosest(s, n->left.get(), r, tMin, closest, prim, t);
    if (n->right != n->left) walkClosest(s, n->right.get(), r, tMin, closest, prim, t);
    return;
  }
  hitRecord temp;
  if (h->hit(r, tMin, closest, temp) && temp.t <= closest) {
    prim = s.primId.at(h);
    closest = t = temp.t;
  }
}

static int jobClosest(const std::string& scenePath, const std::string& raysPath, const std::string& outPath) {
  Scene s;
  loadScene(scenePath, s, true);
  In in(raysPath);
  auto rays = in.array<SrtRay>(in.b.size() / sizeof(SrtRay));
  Out out(outPath);
  for (const SrtRay& q : rays) {
    ray r(v3(q.o), v3(q.d), q.time);
    int32_t treePrim = SRT_NO_HIT, brutePrim = SRT_NO_HIT, ties = 0;
    float closest = q.tMax, treeT = 0, bruteT = 0;
    for (const auto& object : s.world.objects) walkClosest(s, object.get(), r, q.tMin, closest, treePrim, treeT);
    closest = q.tMax;
    hitRecord temp;
    for (size_t i = 0; i < s.prims.size(); i++) {
      if (s.prims[i]->hit(r, q.tMin, closest, temp) && temp.t <= closest) {
        brutePrim = (int32_t)i;
        closest = bruteT = temp.t;
      }
      if (treePrim != SRT_NO_HIT && s.prims[i]->hit(r, q.tMin, q.tMax, temp) && temp.t == treeT) ties++;
    }
    out.put(treePrim);
    out.put(treeT);
    out.put(brutePrim);
    out.put(bruteT);
    out.put(ties);
  }
  return 0;
}

// texture::value and material::emitted at given points.  Record: int32 kind (0 texture, 1 material), int32 id, float u,
// v, p[3]; answer: 3 floats.
struct ValueQuery {
  int32_t kind, id;
  float u, v, p[3];
};
static int jobValues(const std::string& scenePath, const std::string& queryPath, const std::string& outPath) {
  Scene s;
  loadScene(scenePath, s, false);
  In in(queryPath);
  auto qs = in.array<ValueQuery>(in.b.size() / sizeof(ValueQuery));
  Out out(outPath);
  for (const ValueQuery& q : qs) {
    color3f c = q.kind == 0 ? s.textures.at(q.id)->value(q.u, q.v, v3(q.p)) : s.materials.at(q.id)->emitted(q.u, q.v, v3(q.p));
    for (int k = 0; k < 3; k++) out.put(c(k));
  }
  return 0;
}

// material::scatter on (ray, hit record) pairs in order, in one process so the stream is continuous, after the scene
// file's preDraws.  Answer per pair: 13 floats laid out as orc_scatter's (attenuation, direction, origin, ok, emitted);
// then the scattered ray's time per pair; then the next randomFloat().
static int jobScatter(const std::string& scenePath, const std::string& pairsPath, const std::string& outPath) {
  Scene s;
  loadScene(scenePath, s, false);
  for (uint64_t k = 0; k < s.preDraws; k++) randomFloat();
  In in(pairsPath);
  size_t n = in.b.size() / (sizeof(SrtRay) + sizeof(SrtHit));
  auto rays = in.array<SrtRay>(n);
  auto hits = in.array<SrtHit>(n);
  std::vector<float> out13(13 * n), times(n);
  for (size_t i = 0; i < n; i++) {
    hitRecord rec;
    rec.p = v3(hits[i].p);
    rec.normal = v3(hits[i].normal);
    rec.tangent = v3(hits[i].tangent);
    rec.bitangent = v3(hits[i].bitangent);
    rec.uv = vec2f(hits[i].uv[0], hits[i].uv[1]);
    rec.t = hits[i].t;
    rec.frontFace = hits[i].frontFace != 0;
    rec.matPtr = s.materials.at(hits[i].material);
    ray rIn(v3(rays[i].o), v3(rays[i].d), rays[i].time), scattered;
    scattered.time = 0;
    color3f attenuation(0, 0, 0);
    color3f emitted = rec.matPtr->emitted(rec.uv(0), rec.uv(1), rec.p);
    bool ok = rec.matPtr->scatter(rIn, rec, attenuation, scattered);
    float* o = &out13[13 * i];
    for (int k = 0; k < 3; k++) {
      o[k] = attenuation(k);
      o[3 + k] = scattered.dir(k);
      o[6 + k] = scattered.o(k);
      o[10 + k] = emitted(k);
    }
    o[9] = ok ? 1.0f : 0.0f;
    times[i] = scattered.time;
  }
  Out out(outPath);
  out.put(out13.data(), out13.size() * sizeof(float));
  out.put(times.data(), times.size() * sizeof(float));
  out.put(randomFloat());
  return 0;
}

// The pixel loop of main.cpp:200-227 with width, height, samples and bounces as arguments.  Answer: float sums
// [H][W][4] (rgb, samples), RGBA8 [H][W][4], the stream position after the last sample.
static int jobRender(const std::string& scenePath, const std::string& framePath, const std::string& outPath) {
  Scene s;
  loadScene(scenePath, s, true);
  In in(framePath);
  SrtCameraParams c = in.get<SrtCameraParams>();
  SrtRenderParams p = in.get<SrtRenderParams>();
  if (p.tMin != 0.001f) die("main.cpp:39 fixes tMin at 0.001f");
  camera cam(v3(c.eye), v3(c.lookAt), v3(c.up), c.vfovDegrees, c.aspect, c.aperture, c.focusDist, c.time0, c.time1);
  const int W = p.imageWidth, H = p.imageHeight, spp = p.spp;
  const color3f sky(p.background[0], p.background[1], p.background[2]);
  std::vector<float> sums((size_t)W * H * 4);
  std::vector<uint8_t> target((size_t)W * H * 4);
  for (int y = 0; y < H; ++y)    // rows, then columns, then samples; u is drawn before v (main.cpp:200-211)
    for (int x = 0; x < W; ++x) {
      color3f sum(0, 0, 0);
      for (int k = 0; k < spp; ++k) {
        const float u = float(x + randomFloat()) / (W - 1);
        const float v = float((H - y) + randomFloat()) / (H - 1);  // H - y: row 0 is the image's top (main.cpp:211)
        sum += rayColor(cam.getRay(u, v), sky, s.world, p.maxBounce);
      }
      float* a = &sums[((size_t)y * W + x) * 4];
      a[0] = sum(0);
      a[1] = sum(1);
      a[2] = sum(2);
      a[3] = (float)spp;
      writeColorTarget(target.data(), x, y, W, H, 4, sum, spp);  // the reference's own color.h:25-41
    }
  Out out(outPath);
  out.put(sums.data(), sums.size() * sizeof(float));
  out.put(target.data(), target.size());
  out.put((uint64_t)streamPosition());
  return 0;
}

int main(int argc, char** argv) {
  std::vector<std::string> a(argv + 1, argv + argc);
  if (a.size() == 3 && a[0] == "rng") return jobRng(std::atoi(a[1].c_str()), a[2]);
  if (a.size() == 2 && a[0] == "vec3") return jobVec3(a[1]);
  if (a.size() == 3 && a[0] == "tree") return jobTree(a[1], a[2]);
  if (a.size() == 4 && a[0] == "trace") return jobTrace(a[1], a[2], a[3]);
  if (a.size() == 4 && a[0] == "closest") return jobClosest(a[1], a[2], a[3]);
  if (a.size() == 4 && a[0] == "values") return jobValues(a[1], a[2], a[3]);
  if (a.size() == 4 && a[0] == "scatter") return jobScatter(a[1], a[2], a[3]);
  if (a.size() == 4 && a[0] == "render") return jobRender(a[1], a[2], a[3]);
  std::cerr << "usage: ref_harness rng N OUT | vec3 OUT | tree SCENE OUT | trace SCENE RAYS OUT | closest SCENE RAYS OUT | values SCENE QUERIES OUT\n"
               "       | scatter SCENE PAIRS OUT | render SCENE FRAME OUT\n";
  return 1;
}
