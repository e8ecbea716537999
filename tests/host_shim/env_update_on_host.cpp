// TEST INFRASTRUCTURE ONLY.  The passes of an environment update (csrc/device/pt_env_update.h: euIngest, euTotal, euClassify, euTileScan,
// euCompact, euAlias) compiled for the host through the stand-in <hip/hip_runtime.h> of this directory, with g++ -ffp-contract=off, and run
// block by block in the kernels' launch order: a phase of a block is a loop over its 256 threads where the kernels have a barrier.  So
// tests/test_env_update_on_host.py can check the table the construction makes, and its summation order, on the CPU.  Built by the test
// session only.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "pt_env_update.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

namespace {
struct HostBlock
{
  template <class F>
  void phase(F f)
  {
    for(uint32_t t = 0; t < ENV_BLOCK; ++t)
      f(t);
  }
  void atomicAdd(uint32_t* p, uint32_t v) { *p += v; }
};
}  // namespace

// What mi_pt_update_environment_device leaves resident for `src` (width x height texels of `channels` floats): rgba (4 floats per texel),
// accel, and info = {total, n / total, whole deficit, float(1 / total), light texels, sanitised texels}.  Returns the number of tiles.
EXPORT int dev_env_update(int width, int height, int channels, const float* src, float* rgba, MiEnvAccel* accel, double* info)
{
  const uint32_t         n = uint32_t(width) * uint32_t(height);
  const EnvScratchLayout L = euScratchLayout(n, uint32_t(height));
  std::vector<uint8_t>   scratch(L.bytes + 16, 0xcd);  // (the device's scratch is not cleared either)
  uint8_t* const         base = scratch.data() + ((16 - reinterpret_cast<uintptr_t>(scratch.data()) % 16) % 16);
  EnvArgs                A{};
  A.n          = n;
  A.width      = uint32_t(width);
  A.channels   = uint32_t(channels);
  A.numTiles   = euNumTiles(n);
  A.src        = src;
  A.pixels     = reinterpret_cast<float4*>(rgba);
  A.accel      = accel;
  A.rowArea    = reinterpret_cast<const double*>(base + L.rowArea);
  A.header     = reinterpret_cast<EnvHeader*>(base + L.header);
  A.tileImp    = reinterpret_cast<double*>(base + L.tileImp);
  A.tiles      = reinterpret_cast<EnvTriple*>(base + L.tiles);
  A.prefix     = reinterpret_cast<double*>(base + L.prefix);
  A.index      = reinterpret_cast<uint32_t*>(base + L.index);
  A.uniformPdf = euUniformPdf();
  euRowAreas(width, height, reinterpret_cast<double*>(base + L.rowArea));
  std::memset(base + L.header, 0, sizeof(EnvHeader));
  auto      S = std::make_unique<EnvShared>();
  HostBlock blk;
  for(uint32_t tile = 0; tile < A.numTiles; ++tile)
    euIngest(blk, *S, A, tile);
  euTotal(blk, *S, A);
  for(uint32_t tile = 0; tile < A.numTiles; ++tile)
    euClassify(blk, *S, A, tile);
  euTileScan(blk, *S, A);
  for(uint32_t tile = 0; tile < A.numTiles; ++tile)
    euCompact(blk, *S, A, tile);
  for(uint32_t k = 0; k < ((n + ENV_BLOCK - 1u) / ENV_BLOCK) * ENV_BLOCK; ++k)  // (the grid of k_env_alias, its idle threads included)
    euAlias(A, k);
  if(info)
  {
    info[0] = A.header->total;
    info[1] = A.header->scale;
    info[2] = A.header->totalDeficit;
    info[3] = double(A.header->invTotal);
    info[4] = double(A.header->numLight);
    info[5] = double(A.header->sanitised);
  }
  return int(A.numTiles);
}

// The scratch of a call in bytes (MiPtEnvironmentUpdateInfo::scratchBytes after a first call of this size).
EXPORT uint64_t dev_env_scratch_bytes(int width, int height)
{
  return euScratchLayout(uint32_t(width) * uint32_t(height), uint32_t(height)).bytes;
}
