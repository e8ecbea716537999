// k_vertex_ingest / k_rebuild_normals: caller-supplied vertices into the resident geometry, and the optional normal rebuild (pt_vertex_update.h).
// Both are memory-bound copies in k_deform's shape: the block's task record comes through the scalar cache, every stream access is a global
// (not flat) load or store, nothing lives in LDS or scratch.  The interleaved record and the tangent stream move 16 B per lane; the streams
// of 12-byte stride move 12.
// Compiled with the default IEEE flags (not PT_KERNELS_FP): the rebuild's sqrt and division are correctly rounded, as in the host restatement.
#include "pt_vertex_update.h"

namespace pt {

#if defined(__HIP_DEVICE_COMPILE__)
#define VU_GLOBAL __attribute__((address_space(1)))
#define VU_CONST __attribute__((address_space(4)))
#else  // (the host pass of hipcc parses the kernels too)
#define VU_GLOBAL
#define VU_CONST
#endif

namespace {

// The stream pointers come out of the task record: generic pointers to the compiler, whose accesses would be flat.  They all point to
// global memory; saying so gives global_load / global_store.
struct GlobalMem
{
  template <class T>
  static __host__ __device__ __forceinline__ T ld(const T* p, size_t i)
  {
    return *((const VU_GLOBAL T*)p + i);
  }
  template <class T>
  static __host__ __device__ __forceinline__ void st(T* p, size_t i, T v)
  {
    *((VU_GLOBAL T*)p + i) = v;
  }
};

}  // namespace

__global__ __launch_bounds__(VERTEX_UPDATE_BLOCK) void k_vertex_ingest(const VertexUpdateTask* __restrict__ tasks, const uint32_t* __restrict__ blockTask,
                                                                       uint32_t* __restrict__ rejected)
{
  const uint32_t         ti = __builtin_amdgcn_readfirstlane(blockTask[blockIdx.x]);
  const VertexUpdateTask T  = *((const VU_CONST VertexUpdateTask*)tasks + ti);  // block-uniform, constant: scalar loads
  const uint32_t         v  = (blockIdx.x - T.firstBlock) * VERTEX_UPDATE_BLOCK + threadIdx.x;
  const bool             in = v < T.vertexCount;
  VuVertex               r{};
  if(in)
    r = vertexLoad<GlobalMem>(T, v);
  const bool ok = in && vertexAcceptable(r);
  // the rejected vertices of this wave: one atomic, from the ballot (no lane has left yet)
  const unsigned long long bad = __ballot(in && !ok);
  if(bad != 0ull && (threadIdx.x & (warpSize - 1)) == uint32_t(__ffsll(bad) - 1))
    atomicAdd(rejected, uint32_t(__popcll(bad)));
  if(ok)
    vertexWrite<GlobalMem>(T, v, r);
}

__global__ __launch_bounds__(VERTEX_UPDATE_BLOCK) void k_rebuild_normals(const NormalRebuildTask* __restrict__ tasks, const uint32_t* __restrict__ blockTask)
{
  const uint32_t          ti = __builtin_amdgcn_readfirstlane(blockTask[blockIdx.x]);
  const NormalRebuildTask T  = *((const VU_CONST NormalRebuildTask*)tasks + ti);  // block-uniform, constant: scalar loads
  const uint32_t          v  = (blockIdx.x - T.firstBlock) * VERTEX_UPDATE_BLOCK + threadIdx.x;
  if(v < T.vertexCount)
    vertexRebuildNormal<GlobalMem>(T, v);
}

void launchVertexIngest(const VertexUpdateTask* tasks, const uint32_t* blockTask, uint32_t numBlocks, uint32_t* rejected, hipStream_t stream)
{
  if(numBlocks == 0)
    return;
  hipLaunchKernelGGL(k_vertex_ingest, dim3(numBlocks), dim3(VERTEX_UPDATE_BLOCK), 0, stream, tasks, blockTask, rejected);
}

void launchNormalRebuild(const NormalRebuildTask* tasks, const uint32_t* blockTask, uint32_t numBlocks, hipStream_t stream)
{
  if(numBlocks == 0)
    return;
  hipLaunchKernelGGL(k_rebuild_normals, dim3(numBlocks), dim3(VERTEX_UPDATE_BLOCK), 0, stream, tasks, blockTask);
}

}  // namespace pt
