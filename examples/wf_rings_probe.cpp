// The rings of the path-pool kernel (csrc/srt_wf_rings.h) as a stand-alone host program (no GPU, no library): used by
// tests/test_wf_rings.py, and the place for a sanitizer build of that header.
//   srt_wf_rings_probe pos <in.bin> <out.bin>
//     in:  int32 cap, shift, mul3, n; n uint32 counter values            out: n uint32 -- srtWfRingPos of each
//   srt_wf_rings_probe reserve <in.bin> <out.bin>
//     a host replay of enqueue's reservation.  A CALL is one wave's enqueue: 64 lanes, each with a ring of the call site's
//     set or -1.  The atomics on the tails are the only steps of different waves that can interleave; the input gives the
//     order in which they execute.
//     in:  int32 set (bit r: ring r), numCalls, numEvents; uint32 tail[6] (the tails at the start); numCalls x 64 int32
//          (ring per lane); numEvents x 2 int32 (call, ring): the atomics in execution order -- every (call, ring of the set
//          with lanes) exactly once
//     out: numCalls x 64 x 2 uint32: the lane's place by the form specialised for `set`, and by the generic form over all six rings
//          (0xffffffff, 0xffffffff for a lane that enqueues nothing); then uint32 tail[6] at the end
#include <cstdio>
#include <cstring>
#include <vector>

#include "srt_wf_rings.h"

namespace {
bool readAll(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

unsigned long long ballot(const int32_t* ring, int r) {
  unsigned long long m = 0;
  for (int l = 0; l < 64; ++l)
    if (ring[l] == r) m |= 1ull << l;
  return m;
}

int pos(FILE* in, FILE* out) {
  int32_t h[4];
  if (!readAll(in, h, sizeof h) || h[3] < 0) return 1;
  const SrtWfRingGeom g = {h[0], h[1], h[2]};
  std::vector<uint32_t> c((size_t)h[3]);
  if (!readAll(in, c.data(), 4 * c.size())) return 1;
  for (uint32_t& x : c) x = srtWfRingPos(x, g);
  return fwrite(c.data(), 4, c.size(), out) == c.size() ? 0 : 1;
}

int reserve(FILE* in, FILE* out) {
  int32_t h[3];
  uint32_t tail[WF_RINGS];
  if (!readAll(in, h, sizeof h) || !readAll(in, tail, sizeof tail) || h[1] < 0 || h[2] < 0) return 1;
  const uint32_t set = (uint32_t)h[0];
  if (set == 0 || (set & ~WF_SET_ALL)) return 1;
  const size_t calls = (size_t)h[1], events = (size_t)h[2];
  std::vector<int32_t> ring(64 * calls), ev(2 * events);
  if (!readAll(in, ring.data(), 4 * ring.size()) || !readAll(in, ev.data(), 4 * ev.size())) return 1;
  for (int32_t r : ring)
    if (r >= 0 && (r >= WF_RINGS || !(set >> r & 1u))) return 1;  // the call site cannot produce this ring
  // the atomics, in the given order: the base each call got per ring
  std::vector<uint32_t> base(WF_RINGS * calls, 0u);
  std::vector<char> done(WF_RINGS * calls, 0);
  for (size_t e = 0; e < events; ++e) {
    const int32_t c = ev[2 * e], r = ev[2 * e + 1];
    if (c < 0 || (size_t)c >= calls || r < 0 || r >= WF_RINGS || done[WF_RINGS * c + r]) return 1;
    const int n = srtWfReserveCount(ballot(&ring[64 * (size_t)c], r));
    if (n == 0) return 1;  // (the kernel issues no atomic for an empty ring)
    done[WF_RINGS * c + r] = 1;
    base[WF_RINGS * c + r] = tail[r];
    tail[r] += (uint32_t)n;
  }
  std::vector<uint32_t> place(2 * 64 * calls, 0xffffffffu);
  for (size_t c = 0; c < calls; ++c) {
    const int32_t* rg = &ring[64 * c];
    // ---- the arithmetic of the specialised form (srtWfEnqueue<SET>; the device code itself, v_mbcnt and v_writelane, does
    // not compile here): per ring of the set one ballot; place = base + the lanes below in it
    unsigned long long m[WF_RINGS];
    for (int r = 0; r < WF_RINGS; ++r)
      if (set >> r & 1u) {
        m[r] = ballot(rg, r);
        if (m[r] != 0 && !done[WF_RINGS * c + r]) return 1;  // an atomic the event list left out
      }
    for (int l = 0; l < 64; ++l) {
      uint32_t p = 0;
      for (int r = 0; r < WF_RINGS; ++r)
        if (set >> r & 1u) {
          const uint32_t q = srtWfReservePlace(base[WF_RINGS * c + r], m[r], l);
          p = rg[l] == r ? q : p;
        }
      if (rg[l] >= 0) place[2 * (64 * c + l)] = p;
    }
    // ---- the generic form: every ring, a 64-bit `mine` per lane
    for (int l = 0; l < 64; ++l) {
      uint32_t myBase = 0;
      unsigned long long mine = 0;
      for (int r = 0; r < WF_RINGS; ++r) {
        const unsigned long long mr = ballot(rg, r);
        if (rg[l] == r) {
          myBase = base[WF_RINGS * c + r];
          mine = mr;
        }
      }
      if (rg[l] >= 0) place[2 * (64 * c + l) + 1] = myBase + (uint32_t)__builtin_popcountll(mine & ((1ull << l) - 1ull));
    }
  }
  if (fwrite(place.data(), 4, place.size(), out) != place.size()) return 1;
  return fwrite(tail, 4, WF_RINGS, out) == WF_RINGS ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = in ? fopen(argv[3], "wb") : nullptr;
  if (!in || !out) return 1;
  int rc = 2;
  if (!strcmp(argv[1], "pos")) rc = pos(in, out);
  if (!strcmp(argv[1], "reserve")) rc = reserve(in, out);
  fclose(in);
  return fclose(out) ? 1 : rc;
}
