// The link words of the path-pool kernel's LDS tree (csrc/srt_wf_links.h) as a stand-alone host program (no GPU, no
// library): used by tests/test_wf_links.py, and the place for a sanitizer build of that header.  It builds the thread links
// as srtUploadScene does (csrc/srt_thread.h), encodes every record as the kernel's prologue does and decodes it as its walk does.
//   srt_wf_links_probe <in.bin> <out.bin>
// in:  int32 numNodes, numWorld, numTriangles, numSpheres; the node records (2 x float4 each); the world list (int32 each)
// out: int32 1 (0 and nothing else: no thread links for this world); per node eight int32 -- nodeThread, n0.w, n1.w, then
//      for a leaf the first object's reference, "a second follows", the second's reference, "a third follows" (0 for an
//      internal node), 0; per world root four int32 -- its word, and for a primitive root first, "a second follows", 0
#include <cstdio>
#include <vector>

#include "srt_wf_links.h"
#include "srt_thread.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  int32_t n[4];
  if (!in || fread(n, 4, 4, in) != 4 || n[0] < 0 || n[1] < 0) return 1;
  std::vector<float4> nodes(2 * (size_t)n[0]);
  std::vector<int32_t> world(n[1]);
  if (fread(nodes.data(), sizeof(float4), nodes.size(), in) != nodes.size()) return 1;
  if (fread(world.data(), 4, world.size(), in) != world.size()) return 1;
  fclose(in);
  std::vector<int32_t> thread;
  srtThreadLinks16(nodes, world, n[2], n[3], thread);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 1;
  const int32_t ok = thread.empty() ? 0 : 1;
  fwrite(&ok, 4, 1, out);
  if (ok) {
    for (size_t i = 0; i < thread.size(); ++i) {
      int32_t r[8] = {thread[i], srtWfHitWord(srt_thread_detail::refOf(nodes, 2 * i), thread[i]), srtWfMissWord(thread[i]), 0, 0, 0, 0, 0};
      if (srtWfAtPrim(r[1])) {
        r[3] = srtWfLeafFirst(r[1]);
        r[4] = srtWfLeafHasSecond(r[1]);
        if (r[4]) {
          const int32_t rest = srtWfLeafRest(r[1]);
          r[5] = srtWfLeafFirst(rest);
          r[6] = srtWfLeafHasSecond(rest);
        }
      }
      fwrite(r, sizeof r, 1, out);
    }
    for (int32_t wr : world) {
      int32_t r[4] = {srtWfRootWord(wr), 0, 0, 0};
      if (srtWfAtPrim(r[0])) {
        r[1] = srtWfLeafFirst(r[0]);
        r[2] = srtWfLeafHasSecond(r[0]);
      }
      fwrite(r, sizeof r, 1, out);
    }
  }
  return fclose(out) ? 1 : 0;
}
