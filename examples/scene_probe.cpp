// The host stage of srtUploadScene (csrc/srt_scene.cpp: validateScene, flattenScene) as a stand-alone host program (no GPU,
// no library): used by tests/test_scene_host.py, and the place for a sanitizer build of the file that indexes caller-supplied
// arrays by caller-supplied indices.
//   srt_scene_probe validate <in>
//     prints validateScene's message and a newline; the message is empty for a valid scene
//   srt_scene_probe flatten <in> <out>
//     srtHostRandomReset(), `draws` draws of srtHostRandomFloat(), validateScene, flattenScene; prints "flatten_ms <t>", the
//     time the two took.  out: one record per HostScene member, in declaration order --
//         u8 length + name, i64 count, i64 element size, count * size bytes          (a vector)
//         u8 length + name, i64 -1,    i64 4,            4 bytes                       (a scalar)
//     itemNodes is a record of element size 0 followed by one record per world item ("itemNodes[i]"); deviceBuilds is a record
//     of 24-byte elements (item, base, count, builder, time0, time1) followed by one record per build ("deviceBuilds[i].refs").
//     A refusal (of validateScene or flattenScene) writes the single record "error" instead: the text, element size 1.
//   in (tests/scene_probe_io.py writes it), little endian: the arrays of SrtSceneDesc in order, each as
//         i64 count, i64 bytes, the bytes            (bytes = 0: a null pointer, whatever the count says)
//     the world list item by item, an item whose `nodes` is not null followed by its max(numNodes, 0) SrtBvhNode records; then
//     four i32: SceneOptions' wfHybrid, wfResidentMax, fastDiv, and the number of generator draws to skip (hipdev.py
//     _reset_generator_for).
#include <chrono>
#include <cstdio>
#include <cstring>
#include <deque>

#include "srt_scene.h"

namespace {
struct Reader {
  std::vector<uint8_t> buf;
  size_t at = 0;
  bool take(void* dst, size_t n) {
    if (n > buf.size() - at) return false;
    if (n) memcpy(dst, buf.data() + at, n);
    at += n;
    return true;
  }
};

bool readFile(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  bool ok = !fseek(f, 0, SEEK_END);
  const long n = ok ? ftell(f) : -1;
  ok = n >= 0 && !fseek(f, 0, SEEK_SET);
  if (ok) out.resize((size_t)n);
  ok = ok && (n == 0 || fread(out.data(), 1, (size_t)n, f) == (size_t)n);
  fclose(f);
  return ok;
}

// The scene description of an input file, and the storage its pointers go to.
struct Input {
  std::vector<SrtTriangleIn> triangles;
  std::vector<SrtSphereIn> spheres;
  std::vector<SrtPrimRef> prims;
  std::vector<SrtWorldItem> world;
  std::deque<std::vector<SrtBvhNode>> itemNodes;
  std::vector<SrtMaterialIn> materials;
  std::vector<SrtTextureIn> textures;
  std::vector<uint8_t> texels;
  SrtSceneDesc desc;
  SceneOptions options;
  int32_t draws;
};

template <typename T, typename N>
bool readArray(Reader& r, std::vector<T>& store, N& count, const T*& ptr) {
  int64_t n, bytes;
  if (!r.take(&n, 8) || !r.take(&bytes, 8) || bytes < 0 || bytes % (int64_t)sizeof(T)) return false;
  count = (N)n;
  store.resize((size_t)bytes / sizeof(T) + 1);  // (+1: a present array of no elements is still not a null pointer)
  ptr = bytes ? store.data() : nullptr;
  return r.take(store.data(), (size_t)bytes);
}

bool readWorld(Reader& r, Input& in) {
  int64_t n, bytes;
  if (!r.take(&n, 8) || !r.take(&bytes, 8) || bytes < 0) return false;
  in.desc.numWorld = (int32_t)n;
  in.desc.world = nullptr;
  const size_t end = r.at + (size_t)bytes;
  while (r.at < end) {
    SrtWorldItem it;
    if (!r.take(&it, sizeof it)) return false;
    if (it.nodes) {
      in.itemNodes.emplace_back((size_t)(it.numNodes > 0 ? it.numNodes : 0) + 1);
      if (!r.take(in.itemNodes.back().data(), (in.itemNodes.back().size() - 1) * sizeof(SrtBvhNode))) return false;
      it.nodes = in.itemNodes.back().data();
    }
    in.world.push_back(it);
  }
  if (bytes) in.desc.world = in.world.data();
  return r.at == end;
}

bool readInput(const char* path, Input& in) {
  Reader r;
  if (!readFile(path, r.buf)) return false;
  SrtSceneDesc& d = in.desc;
  int32_t tail[4];
  const bool ok = readArray(r, in.triangles, d.numTriangles, d.triangles) && readArray(r, in.spheres, d.numSpheres, d.spheres) &&
                  readArray(r, in.prims, d.numPrims, d.prims) && readWorld(r, in) && readArray(r, in.materials, d.numMaterials, d.materials) &&
                  readArray(r, in.textures, d.numTextures, d.textures) && readArray(r, in.texels, d.numTexelBytes, d.texels) &&
                  r.take(tail, sizeof tail) && r.at == r.buf.size();
  in.options = SceneOptions{tail[0], tail[1], tail[2]};
  in.draws = tail[3];
  return ok;
}

void putRecord(FILE* f, const std::string& name, int64_t count, int64_t size, const void* data) {
  fputc((int)name.size(), f);
  fwrite(name.data(), 1, name.size(), f);
  fwrite(&count, 8, 1, f);
  fwrite(&size, 8, 1, f);
  const size_t bytes = (size_t)(count < 0 ? 1 : count) * (size_t)size;
  if (bytes) fwrite(data, 1, bytes, f);
}
template <typename T>
void put(FILE* f, const std::string& name, const std::vector<T>& v) {
  putRecord(f, name, (int64_t)v.size(), sizeof(T), v.data());
}
void put(FILE* f, const std::string& name, int32_t v) { putRecord(f, name, -1, 4, &v); }

// a member added to HostScene belongs into putScene below, at its place (26 vectors and 7 scalars, one of them padded)
static_assert(sizeof(HostScene) == 26 * sizeof(std::vector<int>) + 8 * sizeof(int32_t), "HostScene changed: update putScene");

void putScene(FILE* f, const HostScene& h) {
  put(f, "nodes", h.nodes);
  put(f, "nodeAxis", h.nodeAxis);
  put(f, "world", h.world);
  put(f, "triTest", h.triTest);
  put(f, "triShade", h.triShade);
  put(f, "triFast", h.triFast);
  put(f, "spheres", h.spheres);
  put(f, "triPrimId", h.triPrimId);
  put(f, "sphPrimId", h.sphPrimId);
  put(f, "materials", h.materials);
  put(f, "textures", h.textures);
  put(f, "texels", h.texels);
  put(f, "shadeRecs", h.shadeRecs);
  put(f, "primClass", h.primClass);
  put(f, "nodeThread", h.nodeThread);
  put(f, "nodesRg", h.nodesRg);
  put(f, "nodeThreadRg", h.nodeThreadRg);
  put(f, "walkSeq", h.walkSeq);
  put(f, "numWalk", h.numWalk);
  put(f, "wfHead", h.wfHead);
  put(f, "nodesWf", h.nodesWf);
  put(f, "worldWf", h.worldWf);
  put(f, "primSecond", h.primSecond);
  put(f, "wfResident", h.wfResident);
  putRecord(f, "itemNodes", (int64_t)h.itemNodes.size(), 0, nullptr);
  for (size_t i = 0; i < h.itemNodes.size(); ++i) put(f, "itemNodes[" + std::to_string(i) + "]", h.itemNodes[i]);
  struct Fixed {
    int32_t item, base, count, builder;
    float time0, time1;
  };
  std::vector<Fixed> builds;
  for (const DeviceBuild& b : h.deviceBuilds) builds.push_back(Fixed{b.item, b.base, b.count, b.builder, b.time0, b.time1});
  put(f, "deviceBuilds", builds);
  for (size_t i = 0; i < h.deviceBuilds.size(); ++i) put(f, "deviceBuilds[" + std::to_string(i) + "].refs", h.deviceBuilds[i].refs);
  put(f, "hostTrees", h.hostTrees);
  put(f, "triDevIndex", h.triDevIndex);
  put(f, "wfIndex", h.wfIndex);
  put(f, "stackDepth", h.stackDepth);
  put(f, "bvhDepth", h.bvhDepth);
  put(f, "fastDivScene", h.fastDivScene);
  put(f, "boxOrderedScene", h.boxOrderedScene);
}

int flatten(const Input& in, const char* outPath) {
  srtHostRandomReset();
  for (int32_t i = 0; i < in.draws; ++i) srtHostRandomFloat();
  HostScene h;
  const auto t0 = std::chrono::steady_clock::now();
  std::string err = validateScene(&in.desc);
  if (err.empty()) err = flattenScene(&in.desc, in.options, h);
  printf("flatten_ms %.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  FILE* f = fopen(outPath, "wb");
  if (!f) return 1;
  if (err.empty())
    putScene(f, h);
  else
    putRecord(f, "error", (int64_t)err.size(), 1, err.data());
  return fclose(f) ? 1 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  const bool doValidate = argc == 3 && !strcmp(argv[1], "validate"), doFlatten = argc == 4 && !strcmp(argv[1], "flatten");
  if (!doValidate && !doFlatten) return 2;
  Input in;
  if (!readInput(argv[2], in)) return 1;
  if (doFlatten) return flatten(in, argv[3]);
  printf("%s\n", validateScene(&in.desc).c_str());
  return 0;
}
