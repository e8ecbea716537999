// Ray queries and picking against the resident scene (include/mi_pt.h: mi_pt_query_rays, mi_pt_query_rays_device, mi_pt_pick; replaces
// nvvk::RayPicker over the TLAS, reference src/ui_renderer.cpp:95-150).  One ray per lane, the per-lane walk of k_selection (pt_kernels.hip)
// with the ray taken from memory and a full hit record written: RAY_FLAG_FORCE_OPAQUE, no culling, closest hit with the walks' tie rule, or
// the first accepted triangle (ANY).  Compiled with the plain options (IEEE division and square root): hit records want them, and the ray /
// triangle test and the camera ray are pinned to IEEE results in every translation unit anyway (divExact, normalizeExact).
// The closest-hit walk's wave-wide triangle rounds and LDS node cache are left out on purpose: a lane never depends on another lane here, so a
// partially filled last wave needs no care and there is no barrier in the kernel at all.
// The _ex entry points (mi_pt_query_rays_ex, mi_pt_query_rays_device_ex, mi_pt_pick_ex) add k_query_rays_ex: the same walk with the candidate test
// of pt_query.h's second half -- face culling, the alpha decision, a per-lane sorted list of the K nearest distinct triangles held in registers
// (K is a compile-time bound: 1, 2, 4, 8).  The alpha mode and the cull mode are wave-uniform run-time values.  Default options take the kernels
// above; nothing of theirs changes.
#include <hip/hip_runtime.h>

#include "pt_kernels.h"
#include "pt_bvh.h"
#include "pt_bvh8.h"
#include "pt_camera.h"
#include "pt_query.h"

namespace pt {

namespace {

constexpr int QUERY_BLOCK = 256;  // 24 KiB of LDS stack per block: [depth][lane], as in k_selection

// The walk of one ray.  `stack`: the block's LDS stack; this lane touches its own column only.
template <bool WIDE, bool ANY>
PT_DEV MiPtRayHit queryOne(const DevScene& sc, const MiPtRay& ray, int* stack)
{
  if(!queryRayValid(ray))
    return queryMiss(MI_PT_HIT_INVALID_RAY);
  const float    tMin = queryTMin(ray.tMin), tMax = ray.tMax;
  const RaySetup r    = makeRaySetup(mk3(ray.origin), mk3(ray.direction));
  QueryBest      best = queryNoHit(tMax);
  // what the node tests cull with: the ray's far bound until there is a hit, the closest hit from then on (finite: the slab arithmetic forms
  // differences with it).  A triangle AT that distance is still visited -- the boxes are padded -- so that the tie rule sees it.
  float walkT = fminf(tMax, 3.0e38f);
  if(sc.bvhRoot != BVH_EMPTY && tMin < tMax)
  {
    if(WIDE)
    {
      LaneStack2 st2;
      uint32_t   stackOverflow[2 * BVH8_STACK_PRIV];
      st2.lds = stack; st2.tid = int(threadIdx.x); st2.stride = QUERY_BLOCK; st2.sp = 0;
      st2.privBase = stackOverflow; st2.privBits = stackOverflow + BVH8_STACK_PRIV;
      const uint32_t octinv = rayOctInv(r.idir);
      NodeGroup      G      = rootGroup(octinv);
      bool           done   = false;
      while(!done)
      {
        if((G.bits >> 8) == 0u)
        {
          if(st2.sp == 0)
            break;
          G = st2.pop();
        }
        const uint32_t child = groupPopChild(G, octinv);
        if(G.bits >> 8)
          st2.push(G);
        uint32_t tBase, tMask;
        bvh8Visit(sc, r, walkT, octinv, child, G, tBase, tMask, nullptr, 0u);
        while(leafPending(tMask))
        {
          const int k = int(leafPop(tMask, 0u));  // (offset from the node's first triangle)
          if(queryTestTri(sc, r, int(tBase) + k, tMin, tMax, best))
          {
            walkT = best.t;
            if(ANY)
            {
              done = true;
              break;
            }
          }
        }
      }
    }
    else
    {
      LaneStack st;
      int       stackOverflow[BVH_STACK_PRIV];
      st.lds = stack; st.tid = int(threadIdx.x); st.stride = QUERY_BLOCK; st.sp = 0; st.priv = stackOverflow;
      // (a scene of one triangle has no node: bvhRoot = ~0, which bvhWalk visits as a leaf)
      bvhWalk(sc, r, walkT, st, [&](int triIndex, float tmax) -> float {
        if(queryTestTri(sc, r, triIndex, tMin, tMax, best))
          return ANY ? -1.0f : best.t;
        return tmax;
      });
    }
  }
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

// Picking: ray i is the camera ray of the continuous pixel position xy[i] -- getRay(floor(xy), frac(xy)), tMin 0, no far bound, closest hit.
template <bool WIDE>
__global__ void __launch_bounds__(QUERY_BLOCK) k_pick_rays(DevScene sc, FrameConsts fc, const float2* xy, uint32_t numRays, MiPtRayHit* hits)
{
  __shared__ int s_stack[BVH_STACK_LDS * QUERY_BLOCK];
  const uint32_t i = blockIdx.x * uint32_t(QUERY_BLOCK) + threadIdx.x;
  if(i >= numRays)
    return;
  const float2 p  = xy[i];
  const float  fx = floorf(p.x), fy = floorf(p.y);
  f3           origin, direction;
  getRay(fc, mk2(fx, fy), mk2(p.x - fx, p.y - fy), origin, direction);
  MiPtRay ray;
  ray.origin[0] = origin.x; ray.origin[1] = origin.y; ray.origin[2] = origin.z; ray.tMin = 0.0f;
  ray.direction[0] = direction.x; ray.direction[1] = direction.y; ray.direction[2] = direction.z; ray.tMax = __builtin_inff();
  storeHit(hits, i, queryOne<WIDE, false>(sc, ray, s_stack));
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
  // the node tests cull with the ray's far bound while the list is not full, with its last t from then on; triangles AT that distance are still
  // visited (padded boxes), so that the tie rule sees them
  const float far   = fminf(tMax, 3.0e38f);
  float       walkT = far;
  if(sc.bvhRoot != BVH_EMPTY && tMin < tMax)
  {
    if(WIDE)
    {
      LaneStack2 st2;
      uint32_t   stackOverflow[2 * BVH8_STACK_PRIV];
      st2.lds = stack; st2.tid = int(threadIdx.x); st2.stride = QUERY_BLOCK; st2.sp = 0;
      st2.privBase = stackOverflow; st2.privBits = stackOverflow + BVH8_STACK_PRIV;
      const uint32_t octinv = rayOctInv(r.idir);
      NodeGroup      G      = rootGroup(octinv);
      bool           done   = false;
      while(!done)
      {
        if((G.bits >> 8) == 0u)
        {
          if(st2.sp == 0)
            break;
          G = st2.pop();
        }
        const uint32_t child = groupPopChild(G, octinv);
        if(G.bits >> 8)
          st2.push(G);
        uint32_t tBase, tMask;
        bvh8Visit(sc, r, walkT, octinv, child, G, tBase, tMask, nullptr, 0u);
        while(leafPending(tMask))
        {
          const int k = int(leafPop(tMask, 0u));  // (offset from the node's first triangle)
          if(queryTestTriEx(sc, r, int(tBase) + k, tMin, tMax, q, raySeed, L))
          {
            walkT = queryListBound(L, q.maxHits, far);
            if(ANY)
            {
              done = true;
              break;
            }
          }
        }
      }
    }
    else
    {
      LaneStack st;
      int       stackOverflow[BVH_STACK_PRIV];
      st.lds = stack; st.tid = int(threadIdx.x); st.stride = QUERY_BLOCK; st.sp = 0; st.priv = stackOverflow;
      bvhWalk(sc, r, walkT, st, [&](int triIndex, float tmax) -> float {
        if(queryTestTriEx(sc, r, triIndex, tMin, tMax, q, raySeed, L))
          return ANY ? -1.0f : queryListBound(L, q.maxHits, far);
        return tmax;
      });
    }
  }
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
  const float2 p  = xy[i];
  const float  fx = floorf(p.x), fy = floorf(p.y);
  f3           origin, direction;
  getRay(fc, mk2(fx, fy), mk2(p.x - fx, p.y - fy), origin, direction);
  float4* o = reinterpret_cast<float4*>(rays + i);
  o[0]      = make_float4(origin.x, origin.y, origin.z, 0.0f);
  o[1]      = make_float4(direction.x, direction.y, direction.z, __builtin_inff());
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
bool plainRules(const QueryRules& q) { return q.alpha == MI_PT_QUERY_ALPHA_OPAQUE && q.cull == MI_PT_QUERY_CULL_NONE && q.maxHits == 1; }

}  // namespace

void launchQueryRays(const DevScene& scene, bool wide, bool any, const MiPtRay* rays, uint32_t numRays, MiPtRayHit* hits, hipStream_t s)
{
  if(numRays == 0)
    return;
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
  if(numRays == 0)
    return;
  const unsigned grid = (numRays + QUERY_BLOCK - 1) / QUERY_BLOCK;
  if(wide)
    hipLaunchKernelGGL(k_pick_rays<true>, dim3(grid), dim3(QUERY_BLOCK), 0, s, scene, fc, xy, numRays, hits);
  else
    hipLaunchKernelGGL(k_pick_rays<false>, dim3(grid), dim3(QUERY_BLOCK), 0, s, scene, fc, xy, numRays, hits);
}

// any: MI_PT_QUERY_ANY (q.maxHits is 1 then).  Opaque, unculled single-hit queries are the kernels of launchQueryRays.
void launchQueryRaysEx(const DevScene& scene, bool wide, bool any, const QueryRules& q, const MiPtRay* rays, uint32_t numRays, MiPtRayHit* hits, hipStream_t s)
{
  if(numRays == 0)
    return;
  if(plainRules(q))
    launchQueryRays(scene, wide, any, rays, numRays, hits, s);
  else if(wide)
    launchExWidth<true>(scene, any, q, rays, numRays, hits, s);
  else
    launchExWidth<false>(scene, any, q, rays, numRays, hits, s);
}

// rayScratch: numRays ray records the camera rays are written to (unused under plain rules, which are k_pick_rays).
void launchPickRaysEx(const DevScene& scene, const FrameConsts& fc, bool wide, const QueryRules& q, const float2* xy, MiPtRay* rayScratch, uint32_t numRays,
                      MiPtRayHit* hits, hipStream_t s)
{
  if(numRays == 0)
    return;
  if(plainRules(q))
  {
    launchPickRays(scene, fc, wide, xy, numRays, hits, s);
    return;
  }
  hipLaunchKernelGGL(k_pick_make_rays, dim3((numRays + QUERY_BLOCK - 1) / QUERY_BLOCK), dim3(QUERY_BLOCK), 0, s, fc, xy, numRays, rayScratch);
  launchQueryRaysEx(scene, wide, false, q, rayScratch, numRays, hits, s);
}

}  // namespace pt
