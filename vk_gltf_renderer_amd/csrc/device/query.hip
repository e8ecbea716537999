// Ray queries and picking against the resident scene (include/mi_pt.h: mi_pt_query_rays, mi_pt_query_rays_device, mi_pt_pick and their _ex forms;
// replaces nvvk::RayPicker over the TLAS, reference src/ui_renderer.cpp:95-150).  One ray per lane with the ray taken from memory and a full hit
// record written; the walk is the per-lane walk of pt_lane_walk.h, which k_selection (pt_kernels.hip) shares, the per-ray work around it is
// pt_query.h's.  What is here: the kernels, which choose the candidate test and the culling bound, and the launchers.
// k_query_rays / k_pick_rays, the plain calls: RAY_FLAG_FORCE_OPAQUE, no culling, closest hit with the walks' tie rule, or the first accepted
// triangle (ANY).  k_query_rays_ex, the _ex calls under other than default options: the candidate test of pt_query.h's second half -- face culling,
// the alpha decision, a per-lane sorted list of the K nearest distinct triangles held in registers (K is a compile-time bound: 1, 2, 4, 8); the
// alpha mode and the cull mode are wave-uniform run-time values.  Default options take the plain kernels, which hold fewer registers and carry no
// such branches.
// Compiled with the plain options (IEEE division and square root): hit records want them, and the ray / triangle test and the camera ray are
// pinned to IEEE results in every translation unit anyway (divExact, normalizeExact).
#include <hip/hip_runtime.h>

#include "pt_kernels.h"
#include "pt_bvh.h"
#include "pt_bvh8.h"
#include "pt_camera.h"
#include "pt_lane_walk.h"
#include "pt_query.h"

namespace pt {

namespace {

constexpr int QUERY_BLOCK = 256;  // 24 KiB of LDS stack per block: [depth][lane], as in k_selection

// The walk of one ray.  `stack`: the block's LDS stack.
template <bool WIDE, bool ANY>
PT_DEV MiPtRayHit queryOne(const DevScene& sc, const MiPtRay& ray, int* stack)
{
  if(!queryRayValid(ray))
    return queryMiss(MI_PT_HIT_INVALID_RAY);
  const float    tMin = queryTMin(ray.tMin), tMax = ray.tMax;
  const RaySetup r    = makeRaySetup(mk3(ray.origin), mk3(ray.direction));
  QueryBest      best = queryNoHit(tMax);
  // the node tests cull with the ray's far bound until there is a hit, with the closest hit from then on
  if(sc.bvhRoot != BVH_EMPTY && tMin < tMax)
    laneWalk<WIDE, ANY, QUERY_BLOCK>(
        sc, r, fminf(tMax, 3.0e38f), stack, [&](int triIndex) { return queryTestTri(sc, r, triIndex, tMin, tMax, best); }, [&] { return best.t; });
  if(best.tri < 0)
    return queryMiss(0u);
  return fillHit(sc, best.tri, best.t, best.u, best.v, best.front, ray);
}

PT_DEV MiPtRay loadRay(const MiPtRay* rays, uint32_t i)
{
  const float4* p = reinterpret_cast<const float4*>(rays + i);
  const float4  a = p[0], b = p[1];
  MiPtRay       ray;
  ray.origin[0] = a.x; ray.origin[1] = a.y; ray.origin[2] = a.z; ray.tMin = a.w;
  ray.direction[0] = b.x; ray.direction[1] = b.y; ray.direction[2] = b.z; ray.tMax = b.w;
  return ray;
}
PT_DEV void storeHit(MiPtRayHit* hits, uint32_t i, const MiPtRayHit& h)
{
  float4* p = reinterpret_cast<float4*>(hits + i);
  p[0]      = make_float4(h.t, h.b1, h.b2, __uint_as_float(h.flags));
  p[1]      = make_float4(__int_as_float(h.renderNode), __int_as_float(h.renderPrimID), __uint_as_float(h.triangle), __int_as_float(h.materialID));
  p[2]      = make_float4(h.position[0], h.position[1], h.position[2], h.reserved0);
  p[3]      = make_float4(h.normal[0], h.normal[1], h.normal[2], h.reserved1);
}

// Lanes past numRays return at once: nobody waits for them (no barrier, no wave-wide operation below).
template <bool WIDE, bool ANY>
__global__ void __launch_bounds__(QUERY_BLOCK) k_query_rays(DevScene sc, const MiPtRay* rays, uint32_t numRays, MiPtRayHit* hits)
{
  __shared__ int s_stack[BVH_STACK_LDS * QUERY_BLOCK];
  const uint32_t i = blockIdx.x * uint32_t(QUERY_BLOCK) + threadIdx.x;
  if(i >= numRays)
    return;
  storeHit(hits, i, queryOne<WIDE, ANY>(sc, loadRay(rays, i), s_stack));
}

// Picking: the camera ray of the continuous pixel position p -- getRay(floor(p), frac(p)), tMin 0, no far bound.  (Inlined into each of its two
// kernels, where contraction may round the last place differently: a ray k_pick_rays walks need not be bit for bit the one k_pick_make_rays writes.)
PT_DEV MiPtRay pickRay(const FrameConsts& fc, float2 p)
{
  const float fx = floorf(p.x), fy = floorf(p.y);
  f3          origin, direction;
  getRay(fc, mk2(fx, fy), mk2(p.x - fx, p.y - fy), origin, direction);
  MiPtRay ray;
  ray.origin[0] = origin.x; ray.origin[1] = origin.y; ray.origin[2] = origin.z; ray.tMin = 0.0f;
  ray.direction[0] = direction.x; ray.direction[1] = direction.y; ray.direction[2] = direction.z; ray.tMax = __builtin_inff();
  return ray;
}
// ray i is the camera ray of xy[i]; closest hit
template <bool WIDE>
__global__ void __launch_bounds__(QUERY_BLOCK) k_pick_rays(DevScene sc, FrameConsts fc, const float2* xy, uint32_t numRays, MiPtRayHit* hits)
{
  __shared__ int s_stack[BVH_STACK_LDS * QUERY_BLOCK];
  const uint32_t i = blockIdx.x * uint32_t(QUERY_BLOCK) + threadIdx.x;
  if(i >= numRays)
    return;
  storeHit(hits, i, queryOne<WIDE, false>(sc, pickRay(fc, xy[i]), s_stack));
}

// ---- the _ex walks --------------------------------------------------------------------------------------------------------------------------------
// The walk of one ray into the list of its (at most) q.maxHits <= K nearest accepted distinct triangles.  ANY (K = 1): the first accepted one.
// Returns false for an invalid ray (the list stays empty).
template <bool WIDE, bool ANY, int K>
PT_DEV bool queryOneEx(const DevScene& sc, const MiPtRay& ray, uint32_t rayIndex, const QueryRules& q, int* stack, QueryList<K>& L)
{
  L = queryListEmpty<K>(ray.tMax);
  if(!queryRayValid(ray))
    return false;
  const float    tMin = queryTMin(ray.tMin), tMax = ray.tMax;
  const RaySetup r    = makeRaySetup(mk3(ray.origin), mk3(ray.direction));
  const uint32_t raySeed = querySeed(q.seed, rayIndex);
  // the node tests cull with the ray's far bound while the list is not full, with its last t from then on
  const float far = fminf(tMax, 3.0e38f);
  if(sc.bvhRoot != BVH_EMPTY && tMin < tMax)
    laneWalk<WIDE, ANY, QUERY_BLOCK>(
        sc, r, far, stack, [&](int triIndex) { return queryTestTriEx(sc, r, triIndex, tMin, tMax, q, raySeed, L); },
        [&] { return queryListBound(L, q.maxHits, far); });
  return true;
}

// Ray i owns records [i * maxHits, (i + 1) * maxHits): its list in ascending order, then miss records; an invalid ray says so in its first record.
template <bool WIDE, bool ANY, int K>
__global__ void __launch_bounds__(QUERY_BLOCK) k_query_rays_ex(DevScene sc, QueryRules q, const MiPtRay* rays, uint32_t numRays, MiPtRayHit* hits)
{
  __shared__ int s_stack[BVH_STACK_LDS * QUERY_BLOCK];
  const uint32_t i = blockIdx.x * uint32_t(QUERY_BLOCK) + threadIdx.x;
  if(i >= numRays)
    return;
  const MiPtRay ray = loadRay(rays, i);
  QueryList<K>  L;
  const bool    valid = queryOneEx<WIDE, ANY, K>(sc, ray, i, q, s_stack, L);
  MiPtRayHit*   out   = hits + size_t(i) * size_t(q.maxHits);
#pragma unroll
  for(int j = 0; j < K; ++j)
    if(j < q.maxHits)
      storeHit(out, uint32_t(j), j == 0 && !valid ? queryMiss(MI_PT_HIT_INVALID_RAY) : queryListRecord(sc, L, j, ray));
}

// mi_pt_pick_ex: the camera rays of k_pick_rays written out as MiPtRay records, for k_query_rays_ex to walk.
__global__ void __launch_bounds__(QUERY_BLOCK) k_pick_make_rays(FrameConsts fc, const float2* xy, uint32_t numRays, MiPtRay* rays)
{
  const uint32_t i = blockIdx.x * uint32_t(QUERY_BLOCK) + threadIdx.x;
  if(i >= numRays)
    return;
  const MiPtRay ray = pickRay(fc, xy[i]);
  float4*       o   = reinterpret_cast<float4*>(rays + i);
  o[0]              = make_float4(ray.origin[0], ray.origin[1], ray.origin[2], ray.tMin);
  o[1]              = make_float4(ray.direction[0], ray.direction[1], ray.direction[2], ray.tMax);
}

template <bool WIDE, bool ANY, int K>
void launchEx(const DevScene& scene, const QueryRules& q, const MiPtRay* rays, uint32_t numRays, MiPtRayHit* hits, hipStream_t s)
{
  const unsigned grid = (numRays + QUERY_BLOCK - 1) / QUERY_BLOCK;
  hipLaunchKernelGGL((k_query_rays_ex<WIDE, ANY, K>), dim3(grid), dim3(QUERY_BLOCK), 0, s, scene, q, rays, numRays, hits);
}
template <bool WIDE>
void launchExWidth(const DevScene& scene, bool any, const QueryRules& q, const MiPtRay* rays, uint32_t numRays, MiPtRayHit* hits, hipStream_t s)
{
  if(any)
    launchEx<WIDE, true, 1>(scene, q, rays, numRays, hits, s);
  else if(q.maxHits <= 1)
    launchEx<WIDE, false, 1>(scene, q, rays, numRays, hits, s);
  else if(q.maxHits <= 2)
    launchEx<WIDE, false, 2>(scene, q, rays, numRays, hits, s);
  else if(q.maxHits <= 4)
    launchEx<WIDE, false, 4>(scene, q, rays, numRays, hits, s);
  else
    launchEx<WIDE, false, 8>(scene, q, rays, numRays, hits, s);
}
// the plain kernels: opaque, unculled, one record per ray
void launchQueryRays(const DevScene& scene, bool wide, bool any, const MiPtRay* rays, uint32_t numRays, MiPtRayHit* hits, hipStream_t s)
{
  const unsigned grid = (numRays + QUERY_BLOCK - 1) / QUERY_BLOCK;
  if(wide)
  {
    if(any)
      hipLaunchKernelGGL((k_query_rays<true, true>), dim3(grid), dim3(QUERY_BLOCK), 0, s, scene, rays, numRays, hits);
    else
      hipLaunchKernelGGL((k_query_rays<true, false>), dim3(grid), dim3(QUERY_BLOCK), 0, s, scene, rays, numRays, hits);
  }
  else
  {
    if(any)
      hipLaunchKernelGGL((k_query_rays<false, true>), dim3(grid), dim3(QUERY_BLOCK), 0, s, scene, rays, numRays, hits);
    else
      hipLaunchKernelGGL((k_query_rays<false, false>), dim3(grid), dim3(QUERY_BLOCK), 0, s, scene, rays, numRays, hits);
  }
}
void launchPickRays(const DevScene& scene, const FrameConsts& fc, bool wide, const float2* xy, uint32_t numRays, MiPtRayHit* hits, hipStream_t s)
{
  const unsigned grid = (numRays + QUERY_BLOCK - 1) / QUERY_BLOCK;
  if(wide)
    hipLaunchKernelGGL(k_pick_rays<true>, dim3(grid), dim3(QUERY_BLOCK), 0, s, scene, fc, xy, numRays, hits);
  else
    hipLaunchKernelGGL(k_pick_rays<false>, dim3(grid), dim3(QUERY_BLOCK), 0, s, scene, fc, xy, numRays, hits);
}

}  // namespace

// Plain rules (queryRulesPlain, pt_query.h) run the plain kernels: fewer registers, no run-time alpha or cull branches.
void launchQueryRaysEx(const DevScene& scene, bool wide, bool any, const QueryRules& q, const MiPtRay* rays, uint32_t numRays, MiPtRayHit* hits, hipStream_t s)
{
  if(numRays == 0)
    return;
  if(queryRulesPlain(q))
    launchQueryRays(scene, wide, any, rays, numRays, hits, s);
  else if(wide)
    launchExWidth<true>(scene, any, q, rays, numRays, hits, s);
  else
    launchExWidth<false>(scene, any, q, rays, numRays, hits, s);
}

void launchPickRaysEx(const DevScene& scene, const FrameConsts& fc, bool wide, const QueryRules& q, const float2* xy, MiPtRay* rayScratch, uint32_t numRays,
                      MiPtRayHit* hits, hipStream_t s)
{
  if(numRays == 0)
    return;
  if(queryRulesPlain(q))
  {
    launchPickRays(scene, fc, wide, xy, numRays, hits, s);
    return;
  }
  hipLaunchKernelGGL(k_pick_make_rays, dim3((numRays + QUERY_BLOCK - 1) / QUERY_BLOCK), dim3(QUERY_BLOCK), 0, s, fc, xy, numRays, rayScratch);
  launchQueryRaysEx(scene, wide, false, q, rayScratch, numRays, hits, s);
}

}  // namespace pt
