// The planner of the render launches (csrc/srt_plan.cpp over csrc/srt_lds_layout.h) as a stand-alone host program (no GPU,
// no library): used by tests/test_plan_host.py, and the place for a sanitizer build of the two.
//   srt_plan_probe limits
//     prints "name value" lines: SRT_LDS_BYTES, the path-pool kernel's bytes per context (whole tree, hybrid), what the
//     upload (srt_scene.cpp flattenScene) decides by -- the largest tree the whole-tree form takes, the hybrid form's
//     resident cap -- and the ring table as "ring cap shift mul3", in the planner's order
//   srt_plan_probe plan <in.txt> <out.txt>
//     in:  rows of 24 integers --
//          numNodes wfResident numWorld stackDepth threadLinks hybridRecords classTable        (SceneFacts)
//          lds_tree wavefront wf_pool wf_profile unit_tiles queues                             (tunables; the others at their defaults)
//          numCUs imageWidth imageHeight spp sppChunks maxBounce traversal countStats tileStride moments listTiles
//     out: per row 16 integers --
//          form block ldsBytes ringCap ringShift ringMul3 single profile unitTiles numQueues sppChunks wfPoolSize wfGrid
//          (the pool and grid of the path-pool forms, else 0 0; after sppChunks = -1 unitTiles and numQueues stand, the
//          rest of the split is 0)
//          fitsLds layoutEnd poolLayoutEnd: the plan fits SRT_LDS_BYTES; the end offset of the planned form's layout
//          (srt_lds_layout.h) for the reserved pool, and for the pool the launch really uses (path-pool forms, else the same)
#include <cstdio>
#include <cstring>

#include "srt_lds_layout.h"
#include "srt_plan.h"

namespace {
int limits() {
  printf("lds_bytes %d\n", SRT_LDS_BYTES);
  printf("context_bytes %zu\ncontext_bytes_hybrid %zu\n", srtWfContextBytes(false), srtWfContextBytes(true));
  printf("ctl_bytes %zu\n", srtWfLdsLayout(0, 0, 0, false).ringSlots);
  printf("whole_tree_max_nodes %d\n", srtWfMaxWholeTreeNodes());
  printf("hybrid_resident_max %d\n", srtWfMaxResidentNodes(SRT_WF_HYBRID_POOL, true));
  for (const SrtWfRingGeom& r : kSrtWfRings) printf("ring %d %d %d\n", r.cap, r.shift, r.mul3);
  return 0;
}

int plan(FILE* in, FILE* out) {
  int v[24];
  for (;;) {
    for (int i = 0; i < 24; ++i)
      if (fscanf(in, "%d", &v[i]) != 1) return i == 0 && feof(in) ? 0 : 1;
    const SceneFacts sc = {v[0], v[1], v[2], v[3], v[4] != 0, v[5] != 0, v[6] != 0};
    Tunables t;
    memset(&t, 0, sizeof t);
    t.tileBlock = SRT_TILE_BLOCK;
    t.shadeMin = t.nodeBurst = t.keepEighths = -1;
    t.primMin = 12, t.hitMin = 24, t.fuseMin = 32, t.primAgainMin = 4, t.wfSwapBig = 32;
    t.ldsTree = v[7], t.wavefront = v[8], t.wfPool = v[9], t.wfProfile = v[10], t.unitTiles = v[11], t.queues = v[12];
    SrtRenderParams p;
    memset(&p, 0, sizeof p);
    p.imageWidth = v[14], p.imageHeight = v[15], p.spp = v[16], p.sppChunks = v[17], p.maxBounce = v[18];
    p.traversal = v[19], p.countStats = v[20], p.tileStride = v[21];
    const LaunchPlan lp = planLaunch(sc, t, v[13], &p, v[22] != 0, v[23]);
    const RenderPlan& r = lp.render;
    size_t end, poolEnd;
    if (srtFormIsPathPool(r.form)) {
      const bool hybrid = r.form == SRT_FORM_PATH_POOL_HYBRID;
      const int resident = hybrid ? sc.wfResident : sc.numNodes;
      end = srtWfLdsLayout(resident, r.wfRingCap, r.wfRingCap, hybrid).end;
      poolEnd = srtWfLdsLayout(resident, r.wfRingCap, lp.wfPoolSize, hybrid).end;
    } else {
      end = srtFormIsLdsTree(r.form) ? srtLdsTreeLayout(sc.numNodes, p.maxBounce, r.form == SRT_FORM_LDS_TREE_ATT).end
                                     : srtStackFormLayout(sc.stackDepth, p.maxBounce).end;
      poolEnd = end;
    }
    fprintf(out, "%d %d %zu %d %d %d %d %d %d %d %d %d %d %d %zu %zu\n", (int)r.form, r.block, r.lds, r.wfRingCap, r.wfRingShift, r.wfRingMul3,
            (int)r.single, (int)r.profile, lp.unitTiles, lp.numQueues, lp.sppChunks, lp.wfPoolSize, lp.wfGrid, (int)lp.fitsLds, end, poolEnd);
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "limits")) return limits();
  if (argc != 4 || strcmp(argv[1], "plan")) return 2;
  FILE* in = fopen(argv[2], "r");
  FILE* out = in ? fopen(argv[3], "w") : nullptr;
  if (!in || !out) return 1;
  const int rc = plan(in, out);
  fclose(in);
  return fclose(out) ? 1 : rc;
}
