// The six passes of an environment update (pt_env_update.h has the construction and its summation order): one kernel each, the body a
// function of that header run through DeviceBlock, whose phases end in a barrier.  The tile passes launch one 256-thread block per 1024
// texels; k_env_total and k_env_tile_scan are ONE block each and loop over the tile sums (65536 of them for 2^26 texels); k_env_alias is one
// thread per slot of the index lists.  The pointers come out of the argument record, which lies in the kernarg segment: global accesses.
// Compiled with the default IEEE flags (not PT_KERNELS_FP) and -ffp-contract=off: the double bookkeeping is rounded once per operation, as
// the host restatement of the tests is.
#include "pt_env_update.h"

namespace pt {

namespace {

struct DeviceBlock
{
  template <class F>
  __device__ __forceinline__ void phase(F f)
  {
    f(threadIdx.x);
    __syncthreads();
  }
  __device__ __forceinline__ void atomicAdd(uint32_t* p, uint32_t v) { ::atomicAdd(p, v); }
};

}  // namespace

__global__ __launch_bounds__(ENV_BLOCK) void k_env_ingest(const EnvArgs A)
{
  __shared__ EnvShared S;
  DeviceBlock          blk;
  euIngest(blk, S, A, blockIdx.x);
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_total(const EnvArgs A)
{
  __shared__ EnvShared S;
  DeviceBlock          blk;
  euTotal(blk, S, A);
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_classify(const EnvArgs A)
{
  __shared__ EnvShared S;
  DeviceBlock          blk;
  euClassify(blk, S, A, blockIdx.x);
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_tile_scan(const EnvArgs A)
{
  __shared__ EnvShared S;
  DeviceBlock          blk;
  euTileScan(blk, S, A);
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_compact(const EnvArgs A)
{
  __shared__ EnvShared S;
  DeviceBlock          blk;
  euCompact(blk, S, A, blockIdx.x);
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_alias(const EnvArgs A)
{
  euAlias(A, blockIdx.x * ENV_BLOCK + threadIdx.x);
}

void launchEnvUpdate(const EnvArgs& A, hipStream_t stream, void (*sync)(const char* pass, void* user), void* user)
{
  const dim3 block(ENV_BLOCK), tiles(A.numTiles), one(1), slots((A.n + ENV_BLOCK - 1u) / ENV_BLOCK);
  auto       done = [&](const char* pass) {
    if(sync)
      sync(pass, user);
  };
  hipLaunchKernelGGL(k_env_ingest, tiles, block, 0, stream, A);
  done("env ingest");
  hipLaunchKernelGGL(k_env_total, one, block, 0, stream, A);
  done("env total");
  hipLaunchKernelGGL(k_env_classify, tiles, block, 0, stream, A);
  done("env classify");
  hipLaunchKernelGGL(k_env_tile_scan, one, block, 0, stream, A);
  done("env tile scan");
  hipLaunchKernelGGL(k_env_compact, tiles, block, 0, stream, A);
  done("env compact");
  hipLaunchKernelGGL(k_env_alias, slots, block, 0, stream, A);
  done("env alias");
}

}  // namespace pt
