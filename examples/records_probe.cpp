// The shared record and box arithmetic (csrc/srt_records.h) as a stand-alone host program (no GPU, no library): used by
// tests/test_records_host.py, and the place for a sanitizer build of that header.
//   srt_records_probe <in.bin> <out.bin> <time0> <time1>
// in:  int32 numTriangles, int32 numSpheres, the SrtTriangleIn records (64 B each), the SrtSphereIn records (40 B each)
// out: per triangle triTest (3 float4), triShade (4 float4), box (3 min, 3 max); then per sphere its records (3 float4)
//      and its box over [time0, time1]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "srt_hip.h"
#include "srt_records.h"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  FILE* in = fopen(argv[1], "rb");
  int32_t n[2];
  if (!in || fread(n, 4, 2, in) != 2 || n[0] < 0 || n[1] < 0) return 1;
  std::vector<SrtTriangleIn> tris(n[0]);
  std::vector<SrtSphereIn> spheres(n[1]);
  if (fread(tris.data(), sizeof(SrtTriangleIn), tris.size(), in) != tris.size()) return 1;
  if (fread(spheres.data(), sizeof(SrtSphereIn), spheres.size(), in) != spheres.size()) return 1;
  fclose(in);
  const float time0 = strtof(argv[3], nullptr), time1 = strtof(argv[4], nullptr);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 1;
  for (const SrtTriangleIn& t : tris) {
    float4 test[3], shade[4], fast[SRT_TRI_FAST_SLOTS];  // (triFast: examples/tri_cert_probe.cpp writes those out)
    float material;
    memcpy(&material, &t.material, 4);
    triangleRecords(&t.p[0][0], &t.uv[0][0], material, test, shade, fast);
    const Box b = triangleBox(vec3(t.p[0]), vec3(t.p[1]), vec3(t.p[2]));
    fwrite(test, sizeof test, 1, out);
    fwrite(shade, sizeof shade, 1, out);
    fwrite(&b, sizeof b, 1, out);
  }
  for (const SrtSphereIn& s : spheres) {
    float4 rec[3];
    const Vec3 c0 = vec3(s.center0), c1 = vec3(s.center1);
    sphereRecords(c0, c1, s.time0, s.time1, s.radius, s.material, rec);
    const Box b = sphereBox(c0, c1, c0 != c1, s.time0, s.time1, s.radius, time0, time1);
    fwrite(rec, sizeof rec, 1, out);
    fwrite(&b, sizeof b, 1, out);
  }
  return fclose(out) ? 1 : 0;
}
