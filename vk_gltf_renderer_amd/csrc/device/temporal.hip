// Motion vectors and the temporal stage of the SVGF denoiser (pt_temporal.h holds the per-pixel arithmetic).
//   k_motion_vectors:       after a first-frame batch: first-hit records + the render nodes' current and previous matrices + viewProj / prevMVP
//                           -> the motion image (the reference's first-hit G-buffer lines, gltf_pathtrace.slang:228-241, :637-645)
//   k_snapshot_transforms:  current objectToWorld -> previous, once per rendered pose (the reference's snapshot_prev_transforms.comp.slang)
//   k_svgf_reproject:       history reprojected along the motion image and blended with this pose's colour -> (illumination, variance) for the
//                           a-trous iterations of denoise.hip, and the new history
// k_svgf_reproject is a stream: per pixel 68 B in (colour, albedo, normal, motion: 16 B each; depth 4 B) and 64 B out (three history records
// and the prepared image), plus four taps of three 16-byte history records that neighbouring pixels share (L2).
#include <hip/hip_runtime.h>

#include "pt_kernels.h"
#include "pt_temporal.h"

namespace pt {

namespace {

struct CameraPair
{
  float viewProj[16], prevMVP[16];
};

// one thread per PIXEL SLOT of the batch (the first-hit records are by slot, the motion image by pixel)
__global__ void __launch_bounds__(256) k_motion_vectors(const float4* __restrict__ firstHit, const uint32_t* __restrict__ ownedTiles, uint32_t numSlots,
                                                       int tileShift, int W, int H, const MiGltfRenderNode* __restrict__ nodes,
                                                       const float* __restrict__ prevObjectToWorld, int numNodes, CameraPair cam, float4* __restrict__ motion)
{
  const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
  int            px, py;
  if(slot >= numSlots || !pixelOfSlot(ownedTiles, tileShift, W, H, slot, px, py))
    return;
  motion[size_t(py) * size_t(W) + size_t(px)] = motionRecord(firstHit[slot], nodes, prevObjectToWorld, numNodes, cam.viewProj, cam.prevMVP, float(W), float(H));
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

void launchMotionVectors(const float4* firstHit, const uint32_t* ownedTiles, uint32_t numSlots, int tileShift, int width, int height,
                         const MiGltfRenderNode* nodes, float* prevObjectToWorld, int numNodes, const float* viewProj, const float* prevMVP, float4* motion,
                         hipStream_t s)
{
  CameraPair cam;
  for(int i = 0; i < 16; ++i)
  {
    cam.viewProj[i] = viewProj[i];
    cam.prevMVP[i]  = prevMVP[i];
  }
  if(numSlots > 0u)
    hipLaunchKernelGGL(k_motion_vectors, dim3((numSlots + 255u) / 256u), dim3(256), 0, s, firstHit, ownedTiles, numSlots, tileShift, width, height, nodes,
                       prevObjectToWorld, numNodes, cam, motion);
  launchSnapshotTransforms(nodes, prevObjectToWorld, numNodes, s);
}

void launchSnapshotTransforms(const MiGltfRenderNode* nodes, float* prevObjectToWorld, int numNodes, hipStream_t s)
{
  const uint32_t n = uint32_t(numNodes) * 16u;
  if(n > 0u)
    hipLaunchKernelGGL(k_snapshot_transforms, dim3((n + 255u) / 256u), dim3(256), 0, s, nodes, prevObjectToWorld, n);
}

void launchSvgfReproject(const float4* color, const float4* albedo, const float4* normal, const float* depth, const float4* motion, const TemporalHistory& in,
                         const TemporalHistory& out, float4* illum, int width, int height, const TemporalConsts& tc, bool haveHistory, hipStream_t s)
{
  dim3 grid((width + 15) / 16, (height + 15) / 16);
  hipLaunchKernelGGL(k_svgf_reproject, grid, dim3(256), 0, s, color, albedo, normal, depth, motion, in, out, illum, width, height, tc, haveHistory ? 1 : 0);
}

}  // namespace pt
