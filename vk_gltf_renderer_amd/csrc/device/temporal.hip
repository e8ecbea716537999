// Motion vectors and the temporal stage of the SVGF denoiser (pt_temporal.h holds the per-pixel arithmetic).
//   k_motion_vectors:       after a first-frame batch: first-hit records + the render nodes' current and previous matrices + viewProj / prevMVP
//                           -> the motion image (the reference's first-hit G-buffer lines, gltf_pathtrace.slang:228-241, :637-645)
//   k_snapshot_transforms:  current objectToWorld -> previous, once per rendered pose (the reference's snapshot_prev_transforms.comp.slang)
//   k_snapshot_positions:   vertex motion: resident positions of every deforming primitive -> their previous-pose copy, one launch, once per
//                           rendered pose that followed a deformation update
//   k_svgf_reproject:       history reprojected along the motion image and blended with this pose's colour -> (illumination, variance) for the
//                           a-trous iterations of denoise.hip, and the new history
// k_svgf_reproject is a stream: per pixel 68 B in (colour, albedo, normal, motion: 16 B each; depth 4 B) and 64 B out (three history records
// and the prepared image), plus four taps of three 16-byte history records that neighbouring pixels share (L2).
// k_snapshot_positions is a plain copy, 12 B in and 12 B out per vertex, moved as 16-byte words: both sides of a primitive are 16-byte aligned
// and padded to whole 16-byte words (the geometry pool's sub-allocations and the previous-position pool's).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_kernels.h"
#include "pt_temporal.h"

namespace pt {

namespace {

struct CameraPair
{
  float viewProj[16], prevMVP[16];
};

// one thread per PIXEL SLOT of the batch (the first-hit records are by slot, the motion image by pixel)
__global__ void __launch_bounds__(256) k_motion_vectors(const float4* __restrict__ firstHit, const uint4* __restrict__ firstHitTri,
                                                       const VertexMotionPrim* __restrict__ vmPrims, int numPrims, const uint32_t* __restrict__ ownedTiles,
                                                       uint32_t numSlots, int tileShift, int W, int H, const MiGltfRenderNode* __restrict__ nodes,
                                                       const float* __restrict__ prevObjectToWorld, int numNodes, CameraPair cam, float4* __restrict__ motion)
{
  const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
  int            px, py;
  if(slot >= numSlots || !pixelOfSlot(ownedTiles, tileShift, W, H, slot, px, py))
    return;
  const float4 fh = firstHit[slot];
  motion[size_t(py) * size_t(W) + size_t(px)] =
      firstHitTri ? motionRecordDeformed(fh, firstHitTri[slot], vmPrims, numPrims, nodes, prevObjectToWorld, numNodes, cam.viewProj, cam.prevMVP, float(W), float(H))
                  : motionRecord(fh, nodes, prevObjectToWorld, numNodes, cam.viewProj, cam.prevMVP, float(W), float(H));
}

// blockIdx.y: the deforming primitive (block-uniform: its record comes through the scalar cache); blockIdx.x: SNAPSHOT_WORDS 16-byte words of
// its position stream, four per thread a wave's width apart -- the loads of a thread are issued together, every access of a wave is 1 KB
constexpr uint32_t SNAPSHOT_WORDS = 256u * 4u;
#if defined(__HIP_DEVICE_COMPILE__)
#define SNAP_GLOBAL __attribute__((address_space(1)))
#else  // (the host pass of hipcc parses the kernel too)
#define SNAP_GLOBAL
#endif

__global__ void __launch_bounds__(256) k_snapshot_positions(const VertexMotionPrim* __restrict__ vmPrims, const uint32_t* __restrict__ ids)
{
  const VertexMotionPrim& vp    = vmPrims[ids[blockIdx.y]];
  const uint32_t          words = uint32_t((size_t(vp.vertexCount) * 3u + 3u) / 4u);
  const uint32_t          base  = blockIdx.x * SNAPSHOT_WORDS + threadIdx.x;
  if(blockIdx.x * SNAPSHOT_WORDS >= words)
    return;
  // (the pointers come out of the record: generic to the compiler, whose flat loads drain at every use; both are global memory)
  const SNAP_GLOBAL float4* src = (const SNAP_GLOBAL float4*)vp.positions;
  SNAP_GLOBAL float4*       dst = (SNAP_GLOBAL float4*)vp.prevPositions;
  if(blockIdx.x * SNAPSHOT_WORDS + SNAPSHOT_WORDS <= words)  // a whole block of words: the four loads in flight together
  {
    const float4 v0 = src[base], v1 = src[base + 256u], v2 = src[base + 512u], v3 = src[base + 768u];
    dst[base]        = v0;
    dst[base + 256u] = v1;
    dst[base + 512u] = v2;
    dst[base + 768u] = v3;
    return;
  }
  for(uint32_t i = base; i < words; i += 256u)  // the stream's last block
    dst[i] = src[i];
}

__global__ void __launch_bounds__(256) k_snapshot_transforms(const MiGltfRenderNode* __restrict__ nodes, float* __restrict__ prevObjectToWorld, uint32_t numFloats)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i < numFloats)
    prevObjectToWorld[i] = nodes[i >> 4].objectToWorld[i & 15u];
}

__global__ void __launch_bounds__(256) k_svgf_reproject(const float4* __restrict__ color, const float4* __restrict__ albedo, const float4* __restrict__ normal,
                                                       const float* __restrict__ depth, const float4* __restrict__ motion, TemporalHistory in,
                                                       TemporalHistory out, float4* __restrict__ illum, int W, int H, TemporalConsts tc, int haveHistory)
{
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if(x >= W || y >= H)
    return;
  illum[size_t(y) * W + x] = reprojectPixel(x, y, W, H, tc, haveHistory != 0, color, albedo, normal, depth, motion, in, out, nullptr);
}

}  // namespace

void launchMotionVectors(const float4* firstHit, const uint4* firstHitTri, const VertexMotionPrim* vmPrims, int numPrims, const uint32_t* ownedTiles,
                         uint32_t numSlots, int tileShift, int width, int height, const MiGltfRenderNode* nodes, float* prevObjectToWorld, int numNodes,
                         const float* viewProj, const float* prevMVP, float4* motion, hipStream_t s)
{
  CameraPair cam;
  for(int i = 0; i < 16; ++i)
  {
    cam.viewProj[i] = viewProj[i];
    cam.prevMVP[i]  = prevMVP[i];
  }
  if(numSlots > 0u)
    hipLaunchKernelGGL(k_motion_vectors, dim3((numSlots + 255u) / 256u), dim3(256), 0, s, firstHit, firstHitTri, vmPrims, numPrims, ownedTiles, numSlots,
                       tileShift, width, height, nodes, prevObjectToWorld, numNodes, cam, motion);
  launchSnapshotTransforms(nodes, prevObjectToWorld, numNodes, s);
}

void launchSnapshotTransforms(const MiGltfRenderNode* nodes, float* prevObjectToWorld, int numNodes, hipStream_t s)
{
  const uint32_t n = uint32_t(numNodes) * 16u;
  if(n > 0u)
    hipLaunchKernelGGL(k_snapshot_transforms, dim3((n + 255u) / 256u), dim3(256), 0, s, nodes, prevObjectToWorld, n);
}

void launchSnapshotPositions(const VertexMotionPrim* vmPrims, const uint32_t* ids, uint32_t numIds, uint32_t maxVertexCount, hipStream_t s)
{
  const uint32_t blocks = uint32_t(((size_t(maxVertexCount) * 3u + 3u) / 4u + SNAPSHOT_WORDS - 1u) / SNAPSHOT_WORDS);
  for(uint32_t first = 0; blocks > 0u && first < numIds; first += 65535u)  // (gridDim.y is 16-bit)
    hipLaunchKernelGGL(k_snapshot_positions, dim3(blocks, std::min(numIds - first, 65535u)), dim3(256), 0, s, vmPrims, ids + first);
}

void launchSvgfReproject(const float4* color, const float4* albedo, const float4* normal, const float* depth, const float4* motion, const TemporalHistory& in,
                         const TemporalHistory& out, float4* illum, int width, int height, const TemporalConsts& tc, bool haveHistory, hipStream_t s)
{
  dim3 grid((width + 15) / 16, (height + 15) / 16);
  hipLaunchKernelGGL(k_svgf_reproject, grid, dim3(256), 0, s, color, albedo, normal, depth, motion, in, out, illum, width, height, tc, haveHistory ? 1 : 0);
}

}  // namespace pt
