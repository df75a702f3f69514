// srt_comm.cpp -- multi-GPU side of the C ABI (include/srt_hip.h, "Multi-GPU"): one process per GPU,
// one RCCL communicator per context, and the path's ONLY data-path collective: one ncclGather of the
// ranks' equal-sized tile buffers to rank 0 (the reference has no multi-device code, its
// device seam gl.h:28-31 is single-GPU).  Pixels are independent (main.cpp:200-227 carries no state
// between pixels once the RNG is counter-based), the scene is replicated: nothing else is exchanged.
//
// The unique id is created by rank 0 (srtCommGetUniqueId) and handed to the other ranks by whatever
// the host program uses to start its processes (a file, MPI, torch.distributed's store); this library
// does not open sockets of its own.

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <cstring>

#include "srt_context.h"

extern "C" {

int srtCommGetUniqueId(void* id128) {
  if (!id128) return 1;
  static_assert(sizeof(ncclUniqueId) == SRT_COMM_ID_BYTES, "SRT_COMM_ID_BYTES must match ncclUniqueId");
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) {
    fprintf(stderr, "srt_hip: ncclGetUniqueId -> %s\n", ncclGetErrorString(r));
    return 1;
  }
  memcpy(id128, &id, sizeof id);
  return 0;
}

int srtCommInit(SrtContext* ctx, const void* id128, int32_t numRanks, int32_t rank) {
  if (!ctx || !id128) return 1;
  if (numRanks < 1 || rank < 0 || rank >= numRanks) return fail(ctx, "srtCommInit: rank out of range");
  if (ctx->comm) return fail(ctx, "srtCommInit: this context already has a communicator");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, "srtCommInit: hipSetDevice failed");
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  ncclComm_t comm = nullptr;
  ncclResult_t r = ncclCommInitRank(&comm, numRanks, id, rank);
  if (r != ncclSuccess)
    return fail(ctx, "srtCommInit: ncclCommInitRank(%d of %d) -> %s", rank, numRanks, ncclGetErrorString(r));
  ctx->comm = comm;
  ctx->commRanks[0] = numRanks;
  ctx->commRanks[1] = rank;
  return 0;
}

int srtCommDestroy(SrtContext* ctx) {
  if (!ctx) return 0;
  if (ctx->comm) {
    (void)hipSetDevice(ctx->device);
    (void)ncclCommDestroy(static_cast<ncclComm_t>(ctx->comm));
    ctx->comm = nullptr;
  }
  ctx->commRanks[0] = 1;
  ctx->commRanks[1] = 0;
  return 0;
}

// One gather: every rank sends its float4[numLocalTiles * 64] tile buffer (what srtRenderTiles wrote for
// tileFirst = rank, tileStride = numRanks); rank 0 receives float4[numRanks][numLocalTiles * 64], the layout
// srtResolveTiles un-permutes.  Asynchronous on `stream`.
int srtGatherTiles(SrtContext* ctx, const SrtRenderParams* p, const void* dLocalTiles, void* dGathered, void* streamPtr) {
  if (!ctx || !p || !dLocalTiles) return 1;
  const int numRanks = ctx->commRanks[0], rank = ctx->commRanks[1];
  if (p->tileStride != numRanks || p->tileFirst != rank)
    return fail(ctx, "srtGatherTiles: the tile split of the render parameters is not this communicator's (tileStride = ranks, tileFirst = rank)");
  const size_t count = (size_t)srtNumLocalTiles(p->imageWidth, p->imageHeight, p->tileStride) * SRT_TILE_PIXELS * 4;  // floats
  hipStream_t stream = static_cast<hipStream_t>(streamPtr);
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, "srtGatherTiles: hipSetDevice failed");
  if (numRanks == 1) {  // nothing to exchange: the gathered buffer is the local one
    if (dGathered && dGathered != dLocalTiles &&
        hipMemcpyAsync(dGathered, dLocalTiles, count * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess)
      return fail(ctx, "srtGatherTiles: copy failed");
    return 0;
  }
  ncclComm_t comm = static_cast<ncclComm_t>(ctx->comm);
  if (!comm) return fail(ctx, "srtGatherTiles: no communicator (srtCommInit)");
  if (rank == 0 && !dGathered) return fail(ctx, "srtGatherTiles: rank 0 needs the gathered buffer");
  ncclResult_t r = ncclGather(dLocalTiles, dGathered, count, ncclFloat32, 0, comm, stream);
  if (r != ncclSuccess) return fail(ctx, "srtGatherTiles: ncclGather -> %s", ncclGetErrorString(r));
  return 0;
}

// main.cpp:182-227 across the ranks of the communicator (collective: every rank calls it with the same
// parameters): each rank renders its tile positions, ONE gather, rank 0 resolves into the caller-owned
// HOST buffers (hAccum float[W*H*4], hRgba uint8[W*H*4]; either may be NULL, both are ignored on other ranks).
int srtRenderImageRanks(SrtContext* ctx, const SrtRenderParams* pIn, float* hAccum, uint8_t* hRgba) {
  if (!ctx || !pIn) return 1;
  const int numRanks = ctx->commRanks[0], rank = ctx->commRanks[1];
  SrtRenderParams p = *pIn;
  p.tileFirst = rank;
  p.tileStride = numRanks;
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, "srtRenderImageRanks: hipSetDevice failed");
  const size_t nPix = (size_t)p.imageWidth * p.imageHeight;
  const size_t localBytes = (size_t)srtNumLocalTiles(p.imageWidth, p.imageHeight, numRanks) * SRT_TILE_PIXELS * sizeof(float4);
  DeviceBuffer local, gathered, rgba, acc, agree;
  // Everything that can fail on ONE rank happens before the gather, and the ranks agree on it first: a rank that
  // returned here while the others entered ncclGather would leave them waiting for ever.  The agreement is a
  // 4-byte all-reduce (minimum of the ranks' status); only a rank that cannot even allocate those 4 bytes leaves
  // without taking part -- its peers then need ncclCommAbort (srtCommDestroy), as after any lost rank.
  if (numRanks > 1 && agree.reserve(sizeof(int32_t)) != hipSuccess) return fail(ctx, "srtRenderImageRanks: hipMalloc (4 bytes)");
  int32_t ok = 1;
  if (local.reserve(localBytes) != hipSuccess) { fail(ctx, "srtRenderImageRanks: hipMalloc"); ok = 0; }
  if (ok && rank == 0) {
    if (gathered.reserve(localBytes * numRanks) != hipSuccess) { fail(ctx, "srtRenderImageRanks: hipMalloc"); ok = 0; }
    if (ok && hRgba && rgba.reserve(nPix * 4) != hipSuccess) { fail(ctx, "srtRenderImageRanks: hipMalloc"); ok = 0; }
    if (ok && hAccum && acc.reserve(nPix * sizeof(float4)) != hipSuccess) { fail(ctx, "srtRenderImageRanks: hipMalloc"); ok = 0; }
  }
  if (ok && srtRenderTiles(ctx, &p, local.get(), nullptr)) ok = 0;
  if (ok && hipDeviceSynchronize() != hipSuccess) { fail(ctx, "srtRenderImageRanks: render kernel failed"); ok = 0; }
  if (numRanks > 1) {
    ncclComm_t comm = static_cast<ncclComm_t>(ctx->comm);
    int32_t agreed = 0;
    if (!comm) return fail(ctx, "srtRenderImageRanks: no communicator (srtCommInit)");
    if (hipMemcpy(agree.get(), &ok, sizeof ok, hipMemcpyHostToDevice) != hipSuccess ||
        ncclAllReduce(agree.get(), agree.get(), 1, ncclInt32, ncclMin, comm, nullptr) != ncclSuccess ||
        hipMemcpy(&agreed, agree.get(), sizeof agreed, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(ctx, "srtRenderImageRanks: the ranks could not agree on the render's status");
    if (!agreed) return ok ? fail(ctx, "srtRenderImageRanks: another rank failed before the gather") : 1;
  } else if (!ok) {
    return 1;
  }
  if (srtGatherTiles(ctx, &p, local.get(), gathered.get(), nullptr)) return 1;
  if (rank == 0 && srtResolveTiles(ctx, &p, gathered.get(), rgba.get(), acc.get(), nullptr)) return 1;
  if (hipDeviceSynchronize() != hipSuccess) return fail(ctx, "srtRenderImageRanks: gather or resolve failed");
  if (rank == 0) {
    if (hRgba && hipMemcpy(hRgba, rgba.get(), nPix * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, "srtRenderImageRanks: copy rgba");
    if (hAccum && hipMemcpy(hAccum, acc.get(), nPix * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, "srtRenderImageRanks: copy accum");
  }
  return 0;
}

}  // extern "C"
