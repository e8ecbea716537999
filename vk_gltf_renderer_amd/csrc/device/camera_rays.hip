// Caller-supplied camera rays (include/mi_pt.h: mi_pt_set_camera_rays, mi_pt_set_camera_rays_device, mi_pt_make_camera_rays and its _device
// form).  While rays are bound a frame starts with k_generate_rays instead of k_generate / k_trace_primary: the path of a slot takes its ray
// from memory (pt_camera_rays.h) and every later stage -- the per-lane walk, shade, next-event estimation, accumulation -- runs unchanged.
//   k_generate_rays       one thread per path slot, k_generate's queue placement and counter initialisation; a dead ray starts no path
//                         and leaves the records k_finish_sample and the first-hit readers would otherwise find stale
//   k_export_camera_rays  the built-in camera's rays as MiPtRay records: what k_generate (pt_kernels.hip) wrote into queue 0, per (set, pixel)
//   k_selection_rays      the selection image of a first frame over the bound set, on the queries' walk and candidate test (pt_query.h)
// Compiled with pt_kernels.hip's floating-point options (csrc/Makefile: PT_KERNELS_FP) and its PT_FAST_SHADING_MATH: k_selection_rays walks like
// k_selection there.  Binding what k_export_camera_rays wrote reproduces the built-in camera's single-sample frames bit for bit.
#include <hip/hip_runtime.h>

#ifndef MI_PT_EXACT_FP
#define PT_FAST_SHADING_MATH 1
#endif
#include "pt_kernels.h"
#include "pt_bvh.h"
#include "pt_bvh8.h"
#include "pt_camera.h"
#include "pt_camera_rays.h"
#include "pt_lane_walk.h"
#include "pt_query.h"

namespace pt {

namespace {

constexpr int CAMERA_RAYS_SEL_BLOCK = 256;  // 24 KiB of LDS stack per block: [depth][lane], as in k_selection

__global__ void __launch_bounds__(256) k_generate_rays(FrameConsts fc, PathSoA P, Queues Q, const uint32_t* __restrict__ ownedTiles,
                                                        const MiPtRay* __restrict__ rays, uint32_t numSets, uint32_t unit, int sampleIndex,
                                                        StatCounters* stats)
{
  const uint32_t batchSlots = uint32_t(fc.numSlots) * uint32_t(fc.numFrames);
  const uint32_t slot       = blockIdx.x * blockDim.x + threadIdx.x;
  bool           valid = false, alive = false;
  CameraRayPath  cp{};
  if(slot < batchSlots)
  {
    uint32_t frame, pixelSlot;
    int      px, py;
    valid = slotFramePixel(fc, ownedTiles, slot, frame, pixelSlot, px, py);
    if(valid)
    {
      const uint32_t F = cameraRayFrame(fc.pc.frameCount, frame);
      const float4*  r = reinterpret_cast<const float4*>(rays + cameraRayIndex(cameraRaySet(F, numSets), fc.width, fc.height, px, py));
      const float4   a = r[0], b = r[1];
      const uint32_t stored = sampleIndex == 0 ? 0u : __float_as_uint(P.misc[slot].z);
      cp    = cameraRayPath(a, b, unit != 0u, px, py, F, sampleIndex, stored, cameraRayDraws(int(fc.frameInfo.flags)));
      alive = cp.alive;
      // (multi-sample frames: the guide records are sums over the samples, zeroed by sample 0 as generateCameraPath does; single-sample frames: written by
      //  the path's first shade, so only a slot without a path is zeroed)
      if(P.guideAlbedo && (fc.pc.numSamples > 1 ? sampleIndex == 0 : !alive))
      {
        P.guideAlbedo[slot] = make_float4(0, 0, 0, 0);
        P.guideNormal[slot] = make_float4(0, 0, 0, 0);
      }
      if(!alive)
      {
        // what k_finish_sample folds for this slot (radiance 0, not solid: alpha 0, NDC depth 1) and what the first-hit readers find (id 0)
        P.radiance[slot] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(RADW_NOT_SOLID));
        if(hasFlag(fc.pc.flags, MI_PT_FIRST_FRAME) && frame == 0u)
          P.firstHit[pixelSlot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
      if(P.misc)
        P.misc[slot] = make_float4(0.0f, __uint_as_float(alive ? uint32_t(PF_ALIVE) : uint32_t(PF_NOT_SOLID)), __uint_as_float(cp.seed), 0.0f);  // cone.width = 0
      if(alive && stats)
        atomicAdd(&stats->cameraPaths, 1ull);
    }
  }
  // Queue placement is a pure function of the slot (chunk = slot / QCHUNK goes to sub-queue chunk % NSUB): no atomics.
  if(slot < batchSlots)
  {
    const uint32_t chunk = slot / QCHUNK;
    const uint32_t pos   = (chunk % NSUB) * Q.subCap + (chunk / NSUB) * QCHUNK + (slot % QCHUNK);
    Q.active[0].slot[pos] = alive ? slot : QUEUE_DEAD;
    if(alive)
    {
      Q.active[0].org[pos] = make_float4(cp.origin.x, cp.origin.y, cp.origin.z, 0.0f);
      Q.active[0].dir[pos] = make_float4(cp.direction.x, cp.direction.y, cp.direction.z, __uint_as_float(cp.seed));  // .w: the path's seed (alpha draws of the walk)
      if(fc.stateInQueue)
        Q.active[0].misc[pos] = make_float4(0.0f, __uint_as_float(PF_ALIVE), __uint_as_float(cp.seed), 0.0f);  // the state travels with the ray (pt_scene.h)
    }
  }
  if(blockIdx.x == 0 && threadIdx.x < NSUB)
  {
    const uint32_t numChunks = batchSlots / QCHUNK;
    Q.counters[QC_PAIR0 + 2 * threadIdx.x] = QCHUNK * (numChunks / NSUB + (threadIdx.x < numChunks % NSUB ? 1u : 0u));
  }
  if(blockIdx.x == 0 && threadIdx.x < 8)
    Q.counters[QC_HEADS_TRACE + threadIdx.x] = 0;
}

// The built-in camera's rays as MiPtRay records.  The rays are k_generate's own (pt_kernels.hip), which launchExportCameraRays runs into queue 0
// first: a second inlined copy of generateCameraPath, here or beside k_generate, is scheduled and packed differently by the compiler and contracts
// the perspective camera's multiply-adds differently -- measured: the direction's last place differed at every seventh pixel -- while the export
// must be the ray queue 0 receives, bit for bit.  This kernel copies: one thread per path slot of the export batch (fc.numFrames sets of the
// pixels of `tiles`), the queue position a pure function of the slot as k_generate places it; frame f of the batch is set setBase + f of `out`.
__global__ void __launch_bounds__(256) k_export_camera_rays(FrameConsts fc, Queues Q, const uint32_t* __restrict__ tiles, MiPtRay* __restrict__ out, uint32_t setBase)
{
  const uint32_t batchSlots = uint32_t(fc.numSlots) * uint32_t(fc.numFrames);
  const uint32_t slot       = blockIdx.x * blockDim.x + threadIdx.x;
  if(slot >= batchSlots)
    return;
  uint32_t frame, pixelSlot;
  int      px, py;
  if(!slotFramePixel(fc, tiles, slot, frame, pixelSlot, px, py))
    return;
  const uint32_t chunk = slot / QCHUNK;
  const uint32_t pos   = (chunk % NSUB) * Q.subCap + (chunk / NSUB) * QCHUNK + (slot % QCHUNK);
  const float4   org = Q.active[0].org[pos], dir = Q.active[0].dir[pos];
  float4*        o   = reinterpret_cast<float4*>(out + cameraRayIndex(setBase + frame, fc.width, fc.height, px, py));
  o[0]               = make_float4(org.x, org.y, org.z, 0.0f);
  o[1]               = make_float4(dir.x, dir.y, dir.z, 3.402823466e+38f);
}

// One bound ray per pixel slot: a dead ray selects nothing; otherwise the closest hit of mi_pt_query_rays(CLOSEST) over the ray as given, tMin 0,
// no far bound.
template <bool WIDE>
__global__ void __launch_bounds__(CAMERA_RAYS_SEL_BLOCK) k_selection_rays(DevScene sc, FrameConsts fc, const uint32_t* ownedTiles, const MiPtRay* rays, uint32_t set,
                                                                          uint32_t* selection)
{
  __shared__ int s_stack[BVH_STACK_LDS * CAMERA_RAYS_SEL_BLOCK];
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  int            px, py;
  if(slot >= uint32_t(fc.numSlots) || !slotToPixel(fc, ownedTiles, slot, px, py))
    return;
  const float4* p = reinterpret_cast<const float4*>(rays + cameraRayIndex(set, fc.width, fc.height, px, py));
  const float4  a = p[0], b = p[1];
  const f3      o = mk3(a.x, a.y, a.z), d = mk3(b.x, b.y, b.z);
  uint32_t      id = 0u;
  if(!cameraRayDead(o, d))
  {
    const float    tMax = 3.402823466e+38f;
    const RaySetup r    = makeRaySetup(o, d);
    QueryBest      best = queryNoHit(tMax);
    if(sc.bvhRoot != BVH_EMPTY)
      laneWalk<WIDE, false, CAMERA_RAYS_SEL_BLOCK>(
          sc, r, fminf(tMax, 3.0e38f), s_stack, [&](int triIndex) { return queryTestTri(sc, r, triIndex, 0.0f, tMax, best); }, [&] { return best.t; });
    if(best.tri >= 0)
      id = best.rnode + 1u;
  }
  selection[size_t(py) * size_t(fc.width) + size_t(px)] = id;
}

}  // namespace

void launchGenerateRays(const LaunchCtx& c, const MiPtRay* rays, uint32_t numSets, bool unit, int sampleIndex)
{
  const unsigned grid = (unsigned(c.fc.numSlots) * unsigned(c.fc.numFrames) + 255u) / 256u;
  hipLaunchKernelGGL(k_generate_rays, dim3(grid), dim3(256), 0, c.stream, c.fc, c.paths, c.queues, c.ownedTiles, rays, numSets, unit ? 1u : 0u, sampleIndex,
                     c.collectCounters ? c.stats : nullptr);
}

void launchExportCameraRays(const LaunchCtx& c, MiPtRay* out, uint32_t setBase)
{
  const unsigned grid = (unsigned(c.fc.numSlots) * unsigned(c.fc.numFrames) + 255u) / 256u;
  launchGenerate(c, 0);
  hipLaunchKernelGGL(k_export_camera_rays, dim3(grid), dim3(256), 0, c.stream, c.fc, c.queues, c.ownedTiles, out, setBase);
}

void launchSelectionRays(const LaunchCtx& c, const MiPtRay* rays, uint32_t set, uint32_t* selection)
{
  const unsigned grid = (unsigned(c.fc.numSlots) + CAMERA_RAYS_SEL_BLOCK - 1) / CAMERA_RAYS_SEL_BLOCK;
  if(c.wide)
    hipLaunchKernelGGL(k_selection_rays<true>, dim3(grid), dim3(CAMERA_RAYS_SEL_BLOCK), 0, c.stream, c.scene, c.fc, c.ownedTiles, rays, set, selection);
  else
    hipLaunchKernelGGL(k_selection_rays<false>, dim3(grid), dim3(CAMERA_RAYS_SEL_BLOCK), 0, c.stream, c.scene, c.fc, c.ownedTiles, rays, set, selection);
}

}  // namespace pt
