// In-place refit of the 8-wide BVH for animated frames (mi_pt_set_accel_update: REFIT / AUTO).  The tree keeps its topology, slot
// assignment and triangle order; only the triangle records, the boxes and the quantised child bytes change:
//   1. k_refit_tris  : one thread per triangle slot -- the record and slot box of every slot whose render node moved or deformed
//   2. k_refit_level : one launch per level of the breadth-first node array, deepest first, one thread per node -- the union of its
//                      children's boxes, requantised (kernel boundaries publish a level to the next: no tickets, no fences)
//   3. k_sah_partial + k_sah_final : the SAH cost of the refitted tree, in a fixed reduction order (the AUTO policy compares it)
// The per-thread work lives in bvh_refit.h, shared with k_tri_setup and k_collapse_emit.
#include <hip/hip_runtime.h>

#include "bvh_refit.h"
#include "pt_build.h"

namespace pt {

namespace {

__global__ void __launch_bounds__(256) k_refit_tris(const MiGltfRenderNode* __restrict__ nodes, const DevPrim* __restrict__ prims,
                                                    const uint8_t* __restrict__ instFlags, const uint8_t* __restrict__ dirty,
                                                    const RefitBox* __restrict__ builtBox, DevTri* __restrict__ tris, RefitBox* __restrict__ slotBox,
                                                    uint32_t numTris)
{
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s < numTris)
    refitTriSlot(nodes, prims, instFlags, dirty, builtBox, tris, slotBox, s);
}

__global__ void __launch_bounds__(128) k_refit_level(Node8* __restrict__ nodes, const RefitBox* __restrict__ slotBox, RefitBox* __restrict__ nodeBox,
                                                     float* __restrict__ sahTerm, uint32_t levelStart, uint32_t levelCount)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= levelCount)
    return;
  const uint32_t n = levelStart + i;
  union
  {
    Node8 node;
    uint4 w[5];
  } N;
  const uint4* src = reinterpret_cast<const uint4*>(nodes) + size_t(n) * 5;
  for(int k = 0; k < 5; ++k)
    N.w[k] = src[k];
  RefitBox own;
  sahTerm[n] = refitNode8(N.node, slotBox, nodeBox, own);
  nodeBox[n] = own;
  uint4* dst = reinterpret_cast<uint4*>(nodes) + size_t(n) * 5;
  for(int k = 0; k < 5; ++k)
    dst[k] = N.w[k];
}

// Sum of the nodes' SAH terms: block b sums terms b, b + grid, ... per thread, then a tree in LDS -- the same order for the same node count
__global__ void __launch_bounds__(256) k_sah_partial(const float* __restrict__ sahTerm, uint32_t numNodes, double* __restrict__ partial)
{
  __shared__ double sum[256];
  double            acc = 0.0;
  for(uint32_t k = blockIdx.x * 256u + threadIdx.x; k < numNodes; k += gridDim.x * 256u)
    acc += double(sahTerm[k]);
  sum[threadIdx.x] = acc;
  __syncthreads();
  for(uint32_t w = 128; w > 0; w >>= 1)
  {
    if(threadIdx.x < w)
      sum[threadIdx.x] += sum[threadIdx.x + w];
    __syncthreads();
  }
  if(threadIdx.x == 0)
    partial[blockIdx.x] = sum[0];
}
// ... and of the partials, over the root's area: partial[REFIT_SAH_PARTIALS] = the cost
__global__ void __launch_bounds__(256) k_sah_final(uint32_t numPartials, const RefitBox* __restrict__ nodeBox, double* __restrict__ partial)
{
  __shared__ double sum[256];
  double            acc = 0.0;
  for(uint32_t k = threadIdx.x; k < numPartials; k += 256u)
    acc += partial[k];
  sum[threadIdx.x] = acc;
  __syncthreads();
  for(uint32_t w = 128; w > 0; w >>= 1)
  {
    if(threadIdx.x < w)
      sum[threadIdx.x] += sum[threadIdx.x + w];
    __syncthreads();
  }
  if(threadIdx.x == 0)
  {
    const RefitBox root = nodeBox[0];
    const float    area = refitBoxAreaOrZero(root.lo, root.hi);  // (resident mode: every render node hidden)
    partial[REFIT_SAH_PARTIALS] = area > 0.0f ? sum[0] / double(area) : 0.0;
  }
}

}  // namespace

void launchRefitTris(const MiGltfRenderNode* nodes, const DevPrim* prims, const uint8_t* instFlags, const uint8_t* dirty, const RefitBox* builtBox,
                     DevTri* tris, RefitBox* slotBox, uint32_t numTris, hipStream_t s)
{
  if(numTris == 0)
    return;
  hipLaunchKernelGGL(k_refit_tris, dim3((numTris + 255u) / 256u), dim3(256), 0, s, nodes, prims, instFlags, dirty, builtBox, tris, slotBox, numTris);
}

void launchRefitLevels(uint4* nodes, const std::vector<uint32_t>& levels, const RefitBox* slotBox, RefitBox* nodeBox, float* sahTerm, hipStream_t s)
{
  for(size_t l = levels.size() - 1; l-- > 0;)  // (levels holds the starts and, last, the node count)
  {
    const uint32_t start = levels[l], count = levels[l + 1] - levels[l];
    if(count == 0)
      continue;
    hipLaunchKernelGGL(k_refit_level, dim3((count + 127u) / 128u), dim3(128), 0, s, reinterpret_cast<Node8*>(nodes), slotBox, nodeBox, sahTerm, start, count);
  }
}

void launchSahCost(const float* sahTerm, uint32_t numNodes, const RefitBox* nodeBox, double* partial, hipStream_t s)
{
  const uint32_t blocks = std::min<uint32_t>(uint32_t(REFIT_SAH_PARTIALS), std::max<uint32_t>(1u, (numNodes + 255u) / 256u));
  hipLaunchKernelGGL(k_sah_partial, dim3(blocks), dim3(256), 0, s, sahTerm, numNodes, partial);
  hipLaunchKernelGGL(k_sah_final, dim3(1), dim3(256), 0, s, blocks, nodeBox, partial);
}

}  // namespace pt
