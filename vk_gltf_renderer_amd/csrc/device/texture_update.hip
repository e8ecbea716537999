// k_texture_ingest / k_texture_mips: caller-supplied texture images into the resident RGBA8 pool, and their mip chains (pt_texture_update.h).
// Both are in k_vertex_ingest's shape: the block's task record comes through the scalar cache, every texel access is a 32-bit (ingest of
// RGBA32F: 128-bit) global load or store.  The decode and encode tables (3 KB) are staged in LDS once per block; the mip kernel reads them
// 16 + up to 24 times per texel.
// Compiled with the default IEEE flags (not PT_KERNELS_FP) and -ffp-contract=off: the chain must equal the host loader's byte for byte.
#include "pt_texture_update.h"

namespace pt {

#if defined(__HIP_DEVICE_COMPILE__)
#define TU_GLOBAL __attribute__((address_space(1)))
#define TU_CONST __attribute__((address_space(4)))
#else  // (the host pass of hipcc parses the kernels too)
#define TU_GLOBAL
#define TU_CONST
#endif

namespace {

// The texel pointers come out of the task record: generic pointers to the compiler, whose accesses would be flat.  They all point to
// global memory; saying so gives global_load / global_store.
struct GlobalMem
{
  template <class T>
  static __host__ __device__ __forceinline__ T ld(const T* p, size_t i)
  {
    return *((const TU_GLOBAL T*)p + i);
  }
  template <class T>
  static __host__ __device__ __forceinline__ void st(T* p, size_t i, T v)
  {
    *((TU_GLOBAL T*)p + i) = v;
  }
};

__device__ __forceinline__ void stageTables(float* s_tables, const float* __restrict__ tables)
{
  for(uint32_t i = threadIdx.x; i < uint32_t(TU_TABLE_FLOATS); i += TEXTURE_UPDATE_BLOCK)
    s_tables[i] = GlobalMem::ld(tables, i);
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(TEXTURE_UPDATE_BLOCK) void k_texture_ingest(const TextureIngestTask* __restrict__ tasks, const uint32_t* __restrict__ blockTask,
                                                                         const float* __restrict__ tables)
{
  __shared__ float        s_tables[TU_TABLE_FLOATS];
  const uint32_t          ti = __builtin_amdgcn_readfirstlane(blockTask[blockIdx.x]);
  const TextureIngestTask T  = *((const TU_CONST TextureIngestTask*)tasks + ti);  // block-uniform, constant: scalar loads
  const uint32_t          i  = (blockIdx.x - T.firstBlock) * TEXTURE_UPDATE_BLOCK + threadIdx.x;
  if(!(T.flags & TU_FLOAT))  // (block-uniform)
  {
    if(i < T.texelCount)
      GlobalMem::st(T.dst, i, GlobalMem::ld(static_cast<const uint32_t*>(T.src), i));
    return;
  }
  stageTables(s_tables, tables);
  if(i < T.texelCount)
    GlobalMem::st(T.dst, i, tuQuantise(s_tables, GlobalMem::ld(static_cast<const float4*>(T.src), i), (T.flags & TU_SRGB) != 0));
}

__global__ __launch_bounds__(TEXTURE_UPDATE_BLOCK) void k_texture_mips(const TextureMipTask* __restrict__ tasks, const uint32_t* __restrict__ blockTask,
                                                                       const float* __restrict__ tables)
{
  __shared__ float     s_tables[TU_TABLE_FLOATS];
  const uint32_t       ti = __builtin_amdgcn_readfirstlane(blockTask[blockIdx.x]);
  const TextureMipTask T  = *((const TU_CONST TextureMipTask*)tasks + ti);  // block-uniform, constant: scalar loads
  stageTables(s_tables, tables);
  const uint32_t i = (blockIdx.x - T.firstBlock) * TEXTURE_UPDATE_BLOCK + threadIdx.x;
  if(i < T.dw * T.dh)
    GlobalMem::st(T.dst, i, mipTexel<GlobalMem>(T, s_tables, i % T.dw, i / T.dw));
}

void launchTextureIngest(const TextureIngestTask* tasks, const uint32_t* blockTask, uint32_t numBlocks, const float* tables, hipStream_t stream)
{
  if(numBlocks == 0)
    return;
  hipLaunchKernelGGL(k_texture_ingest, dim3(numBlocks), dim3(TEXTURE_UPDATE_BLOCK), 0, stream, tasks, blockTask, tables);
}

void launchTextureMips(const TextureMipTask* tasks, const uint32_t* blockTask, uint32_t numBlocks, const float* tables, hipStream_t stream)
{
  if(numBlocks == 0)
    return;
  hipLaunchKernelGGL(k_texture_mips, dim3(numBlocks), dim3(TEXTURE_UPDATE_BLOCK), 0, stream, tasks, blockTask, tables);
}

}  // namespace pt
