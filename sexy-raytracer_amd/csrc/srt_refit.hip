// srt_refit.hip -- geometry updates in place (include/srt_hip.h srtUpdateTriangles / srtUpdateSpheres / srtRefitScene):
// the primitive records rewritten from caller data, every node box refitted bottom-up over the uploaded topology, and
// what is derived from boxes refreshed.  Topology (the reference words of every record, nodeAxis, the thread links) is
// never written.  Records, boxes, unions and the certificate are srt_records.h's, the ones flattenScene (srt_scene.cpp)
// calls, so a record or box carries the bits an upload of the same data gives.  Also srtGetTreeCost's reduction over the
// node boxes (at the end).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srt_device.h"
#include "srt_records.h"
#include "srt_launch.h"

namespace {

// One lane per updated triangle: SrtTriangleIn (64 B, four 16-byte loads) -> triTest, triShade and triFast at the triangle's DEVICE
// index.  The material word (index, type and flag bits) stays.  devIndex: scene triangle index -> device index, null =
// identity.
__global__ void refitTriRecords(const float4* in, int first, int count, const int32_t* devIndex, float4* triTest, float4* triShade, float4* triFast) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const float4 a = in[4 * (size_t)i], b = in[4 * (size_t)i + 1], c = in[4 * (size_t)i + 2], d = in[4 * (size_t)i + 3];
  const float p[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x}, uv[6] = {c.y, c.z, c.w, d.x, d.y, d.z};
  const size_t j = (size_t)(devIndex ? devIndex[first + i] : first + i);
  float4 test[3], shade[4], fast[SRT_TRI_FAST_SLOTS];
  triangleRecords(p, uv, triShade[4 * j + 3].w, test, shade, fast);
  for (int k = 0; k < 3; ++k) triTest[3 * j + k] = test[k];
  for (int k = 0; k < SRT_TRI_FAST_SLOTS; ++k) triFast[SRT_TRI_FAST_SLOTS * j + k] = fast[k];
  for (int k = 0; k < 4; ++k) triShade[4 * j + k] = shade[k];
}

// One lane per updated sphere: SrtSphereIn (ten words) -> the sphere's three records.  The material word keeps everything
// but the "moving" bit.
__global__ void refitSphereRecords(const float* in, int first, int count, float4* spheres) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const float* s = in + 10 * (size_t)i;
  const size_t j = (size_t)(first + i);
  float4 rec[3];
  sphereRecords(vec3(s), vec3(s + 3), s[6], s[7], s[8], __float_as_int(spheres[3 * j + 1].w), rec);
  for (int k = 0; k < 3; ++k) spheres[3 * j + k] = rec[k];
}

// ---------------------------------------------------------------------------------------------------- refit
// up[node] = parent index | (the parent's number of node children) << 28, -1 for a root: the topology the refit climbs.
// Built once per uploaded scene from the node array's reference words (pure topology: a refit never changes it).
#define REFIT_NEED_SHIFT 28
#define REFIT_PARENT_MASK ((1 << REFIT_NEED_SHIFT) - 1) /* SRT_MAX_NODES = 2^25 */

__device__ __forceinline__ bool isNode(int32_t ref) { return ref >= 0; }

__global__ void refitLinks(const float4* nodes, int numNodes, int32_t* up) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numNodes) return;
  const int32_t l = __float_as_int(nodes[2 * (size_t)i].w), r = __float_as_int(nodes[2 * (size_t)i + 1].w);
  const int need = (isNode(l) ? 1 : 0) + (isNode(r) && r != l ? 1 : 0);
  const int32_t word = i | need << REFIT_NEED_SHIFT;
  if (isNode(l)) up[SRT_NODE_INDEX(l)] = word;
  if (isNode(r)) up[SRT_NODE_INDEX(r)] = word;
}

struct RefitArgs {
  DevScene scene;
  int32_t base, count;  // the item's node slots
  float time0, time1;   // the item's (bvh.h:15-16)
  const int32_t* up;
  int32_t* arrived;     // one counter per node, zero before the launch
  int32_t* flag;        // bit 0: a primitive box of a device-built item fails the fast-division certificate
  int32_t checkPrims;   // the item is device-built
};

// Bottom-up over one world item's tree, in the manner of lbvhFit (srt_lbvh.hip): one lane per node; the lanes of the nodes
// without node children start, fit their node and climb; at a parent the lane that completes its node children's count
// goes on, every other one stops.  Nobody waits.  A child's box is published by a release fence before the arrival is
// counted and read behind an acquire fence after it (agent scope: the compute dies have private L2s).  Unions are
// min / max, so the boxes do not depend on who arrives when.  The reference words of the records are written back as read.
__global__ void refitNodes(RefitArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.count) return;
  float4* const nodes = const_cast<float4*>(a.scene.nodes);
  int node = a.base + i;
  {
    const int32_t l = __float_as_int(nodes[2 * (size_t)node].w), r = __float_as_int(nodes[2 * (size_t)node + 1].w);
    if (isNode(l) || isNode(r)) return;
  }
  bool bad = false;
  for (;;) {
    const float4 n0 = nodes[2 * (size_t)node], n1 = nodes[2 * (size_t)node + 1];
    const int32_t link = a.up[node];  // read before the stores: nothing but the fence stands between them and the arrival
    const int32_t refs[2] = {__float_as_int(n0.w), __float_as_int(n1.w)};
    Box box = {};
    bool any = false;
    for (int c = 0; c < 2; ++c) {
      const int32_t ref = refs[c];
      if (ref == SRT_REF_DONE || (c == 1 && ref == refs[0])) continue;  // an unused slot; a single-object leaf
      Box child;
      if (isNode(ref)) {
        const size_t j = (size_t)SRT_NODE_INDEX(ref);
        const float4 c0 = nodes[2 * j], c1 = nodes[2 * j + 1];
        child = Box{{c0.x, c0.y, c0.z}, {c1.x, c1.y, c1.z}};
      } else {
        primBox(a.scene, ref, a.time0, a.time1, child.mn, child.mx);
        if (a.checkPrims) bad = bad || !fastDivOperands(child);
      }
      box = any ? surrounding(box, child) : child;
      any = true;
    }
    if (any) {
      nodes[2 * (size_t)node] = make_float4(box.mn[0], box.mn[1], box.mn[2], n0.w);
      nodes[2 * (size_t)node + 1] = make_float4(box.mx[0], box.mx[1], box.mx[2], n1.w);
    }
    if (link < 0) break;  // a root
    const int parent = link & REFIT_PARENT_MASK, need = link >> REFIT_NEED_SHIFT;
    __threadfence();
    if (atomicAdd(&a.arrived[parent], 1) + 1 < need) break;  // a sibling subtree is not finished: its last lane goes on
    __threadfence();
    node = parent;
  }
  if (bad) atomicOr(a.flag, 1);
}

// After the refit, one lane per node: the node boxes' share of the certificate (flag bit 1), whether they are ordered (flag
// bit 2 is raised by one that is not: the sign form of the slab test, srt_slab.h), and the box halves of the
// hybrid records (DevScene::nodesWf) through the renumbering of srtHybridRecords; their reference and link words stay.
__global__ void refitDerived(const float4* nodes, int numNodes, const int32_t* wfIndex, float4* nodesWf, int32_t* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numNodes) return;
  const float4 lo = nodes[2 * (size_t)i], hi = nodes[2 * (size_t)i + 1];
  const Box box = {{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
  if (!fastDivOperands(box)) atomicOr(flag, 2);
  if (!srtBoxOrdered(box)) atomicOr(flag, 4);  // (DevScene::boxOrderedScene)
  if (wfIndex) {
    const size_t j = (size_t)wfIndex[i];
    nodesWf[2 * j] = make_float4(lo.x, lo.y, lo.z, nodesWf[2 * j].w);
    nodesWf[2 * j + 1] = make_float4(hi.x, hi.y, hi.z, nodesWf[2 * j + 1].w);
  }
}

// ---------------------------------------------------------------------------------------------------- tree cost
// srtGetTreeCost (include/srt_hip.h): the pairwise sum of the node boxes' half areas.  Every workgroup owns COST_BLOCK
// consecutive values (an aligned power-of-two range of the zero-padded array) and leaves their pairwise sum: lane 0 of a
// wave after __shfl_down by 1, 2, .. 32 holds ((x0 + x1) + (x2 + x3)) + .., element k of a level being x[2k] + x[2k+1];
// the waves' four partials take the same two steps through LDS.  Values past `count` are +0.0, which changes no sum (no
// term and no partial is -0.0: x + (-x) rounds to +0.0, and of a box's three products at most two can be negative zeros).
// No atomics: nothing depends on who arrives when.
#define COST_BLOCK SRT_COST_BLOCK

__device__ __forceinline__ double pairwiseBlockSum(double v, double* waveSums) {
  for (int step = 1; step < 64; step <<= 1) v += __shfl_down(v, step);
  if ((threadIdx.x & 63) == 0) waveSums[threadIdx.x >> 6] = v;
  __syncthreads();
  v = threadIdx.x < COST_BLOCK / 64 ? waveSums[threadIdx.x] : 0.0;
  for (int step = 1; step < COST_BLOCK / 64; step <<= 1) v += __shfl_down(v, step);
  return v;  // thread 0's
}

// One lane per node of the item (32 B: two 16-byte loads): a_i = (dx dy + dy dz) + dz dx in double, the float box widened
// first.  out[block] = the block's sum; out[gridDim.x] = a_0, the root's.
__global__ __launch_bounds__(COST_BLOCK) void treeCostNodes(const float4* nodes, int count, double* out) {
  __shared__ double waveSums[COST_BLOCK / 64];
  const int i = blockIdx.x * COST_BLOCK + threadIdx.x;
  double a = 0.0;
  if (i < count) {
    const float4 lo = nodes[2 * (size_t)i], hi = nodes[2 * (size_t)i + 1];
    const double dx = (double)hi.x - (double)lo.x, dy = (double)hi.y - (double)lo.y, dz = (double)hi.z - (double)lo.z;
    a = (dx * dy + dy * dz) + dz * dx;
    if (i == 0) out[gridDim.x] = a;
  }
  const double sum = pairwiseBlockSum(a, waveSums);
  if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

// The next levels: COST_BLOCK partials per workgroup
__global__ __launch_bounds__(COST_BLOCK) void treeCostPartials(const double* in, int count, double* out) {
  __shared__ double waveSums[COST_BLOCK / 64];
  const int i = blockIdx.x * COST_BLOCK + threadIdx.x;
  const double sum = pairwiseBlockSum(i < count ? in[i] : 0.0, waveSums);
  if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

inline dim3 gridFor(int n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

extern "C" {

int srt_launch_refit_triangles(const void* dIn, int first, int count, const int32_t* devIndex, float4* triTest, float4* triShade,
                               float4* triFast, hipStream_t stream) {
  hipLaunchKernelGGL(refitTriRecords, gridFor(count), dim3(256), 0, stream, static_cast<const float4*>(dIn), first, count, devIndex,
                     triTest, triShade, triFast);
  return (int)hipGetLastError();
}

int srt_launch_refit_spheres(const void* dIn, int first, int count, float4* spheres, hipStream_t stream) {
  hipLaunchKernelGGL(refitSphereRecords, gridFor(count), dim3(256), 0, stream, static_cast<const float*>(dIn), first, count, spheres);
  return (int)hipGetLastError();
}

int srt_launch_refit_links(const float4* nodes, int numNodes, int32_t* up, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(up, 0xff, (size_t)numNodes * sizeof(int32_t), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(refitLinks, gridFor(numNodes), dim3(256), 0, stream, nodes, numNodes, up);
  return (int)hipGetLastError();
}

// One world item's tree.  arrived must be zero over the item's nodes.
int srt_launch_refit_nodes(const DevScene* sc, int base, int count, float time0, float time1, const int32_t* up, int32_t* arrived,
                           int32_t* flag, int checkPrims, hipStream_t stream) {
  RefitArgs a;
  a.scene = *sc;
  a.base = base;
  a.count = count;
  a.time0 = time0;
  a.time1 = time1;
  a.up = up;
  a.arrived = arrived;
  a.flag = flag;
  a.checkPrims = checkPrims;
  hipLaunchKernelGGL(refitNodes, gridFor(count), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

int srt_launch_refit_derived(const DevScene* sc, const int32_t* wfIndex, int32_t* flag, hipStream_t stream) {
  hipLaunchKernelGGL(refitDerived, gridFor(sc->numNodes), dim3(256), 0, stream, sc->nodes, sc->numNodes, wfIndex,
                     const_cast<float4*>(sc->nodesWf), flag);
  return (int)hipGetLastError();
}

// srtGetTreeCost's levels.  out: SRT_COST_BLOCK-th as many sums as values (rounded up); the node level adds the root's
// term behind them.
int srt_launch_tree_cost_nodes(const float4* itemNodes, int count, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(treeCostNodes, dim3((unsigned)((count + COST_BLOCK - 1) / COST_BLOCK)), dim3(COST_BLOCK), 0, stream, itemNodes, count, out);
  return (int)hipGetLastError();
}

int srt_launch_tree_cost_partials(const double* in, int count, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(treeCostPartials, dim3((unsigned)((count + COST_BLOCK - 1) / COST_BLOCK)), dim3(COST_BLOCK), 0, stream, in, count, out);
  return (int)hipGetLastError();
}

}  // extern "C"
