// Ray queries against the resident scene (mi_pt_query_rays / mi_pt_query_rays_device / mi_pt_pick, include/mi_pt.h): everything per ray that
// is not the walk (pt_lane_walk.h) -- ray validation, the acceptance test, the closest-hit rule and the hit record.  Plain PT_DEV code: query.hip
// runs it per lane, tests/host_shim/query_on_host.cpp compiles it for the CPU.  The second half is the per-ray work of the _ex entry points (face
// culling, the alpha decision, the sorted list of the K nearest distinct triangles): tests/host_shim/query_ex_on_host.cpp.
// The two candidate tests (queryTestTri, queryTestTriEx) still open with the same intersect / accept / decode lines, and queryOne / queryOneEx
// (query.hip) with the same validation and setup, which the shims' `brute` functions re-type: folding either moved the register counts of the
// compiled kernels (LABNOTES.md, "One per-lane walk for the query calls and the selection pass"), so they stay as they are.
#pragma once
#include "pt_bvh.h"
#include "pt_shading.h"  // getOpacityFast

namespace pt {

static_assert(sizeof(MiPtRay) == 32 && sizeof(MiPtRayHit) == 64, "the query records are 32 and 64 bytes (include/mi_pt.h)");

// A ray the walk can take: finite origin and direction, a direction that is not zero, bounds that are not NaN (infinite bounds are fine).
// Denormal direction components are accepted: makeRaySetup replaces what it cannot invert by +-1e-30.
PT_DEV bool queryRayValid(const MiPtRay& ray)
{
  const f3   o = mk3(ray.origin), d = mk3(ray.direction);
  const bool nonZero = d.x != 0.0f || d.y != 0.0f || d.z != 0.0f;
  const bool bounds  = ray.tMin == ray.tMin && ray.tMax == ray.tMax;  // (not NaN)
  return isFinite3(o) && isFinite3(d) && nonZero && bounds;
}
// Nothing behind the origin is hit (the node tests clip at t = 0): a negative tMin acts as 0.
PT_DEV float queryTMin(float tMin) { return fmaxf(tMin, 0.0f); }
// The open interval: a hit AT a bound is not accepted.
PT_DEV bool queryAccept(float t, float tMin, float tMax) { return t > tMin && t < tMax; }

struct QueryBest
{
  float    t, u, v;
  int      tri;  // index into DevScene::tris, -1 = nothing yet
  uint32_t rnode, prim;
  bool     front;  // TriHit::front: the world-space winding faces the ray
};
PT_DEV QueryBest queryNoHit(float tMax)
{
  QueryBest b;
  b.t = tMax; b.u = b.v = 0.0f; b.tri = -1; b.rnode = b.prim = 0xffffffffu; b.front = false;
  return b;
}
// RAY_FLAG_FORCE_OPAQUE, no culling (k_selection's test): the triangle is a candidate iff intersectTri accepts it and tMin < t < tMax; among
// candidates the smallest t wins, exact ties go to the smaller (renderNode, triangle).  Returns whether the triangle was accepted at all.
PT_DEV bool queryTestTri(const DevScene& sc, const RaySetup& r, int triIndex, float tMin, float tMax, QueryBest& best)
{
  const DevTri T = sc.tris[triIndex];
  TriHit       h;
  if(!intersectTri(xyz(T.a), xyz(T.b), xyz(T.c), r.org, r.dir, h) || !queryAccept(h.t, tMin, tMax))
    return false;
  const uint32_t rnode = __float_as_uint(T.a.w), prim = __float_as_uint(T.b.w);
  if(best.tri < 0 || h.t < best.t || (h.t == best.t && (rnode < best.rnode || (rnode == best.rnode && prim < best.prim))))
  {
    best.t = h.t; best.u = h.u; best.v = h.v; best.tri = triIndex; best.rnode = rnode; best.prim = prim; best.front = h.front;
  }
  return true;
}

PT_DEV MiPtRayHit queryMiss(uint32_t flags)
{
  MiPtRayHit hit;
  memset(&hit, 0, sizeof(hit));
  hit.flags      = flags;
  hit.renderNode = -1;
  return hit;
}
// The record of an accepted hit: t, u, v and `front` as intersectTri returned them for triangle slot triIndex.
PT_DEV MiPtRayHit fillHit(const DevScene& sc, int triIndex, float t, float u, float v, bool front, const MiPtRay& ray)
{
#pragma clang fp contract(off)
  const DevTri      T = sc.tris[triIndex];
  const DevShadeTri S = sc.shadeTris[triIndex];
  MiPtRayHit        hit;
  memset(&hit, 0, sizeof(hit));
  hit.t  = t;
  hit.b1 = u;
  hit.b2 = v;
  // facing is decided in object space, like the walks' culling and the shade kernel's geometric normal (pt_shade_body.h, getHitState: the
  // object-space normal through worldToObject^T): TriHit::front is the WORLD-space winding, which a mirroring instance (INST_FLIP_FACING) inverts
  const bool frontFace = front != ((__float_as_uint(T.c.w) & INST_FLIP_FACING) != 0u);
  hit.flags        = MI_PT_HIT | (frontFace ? MI_PT_HIT_FRONT_FACE : 0u);
  hit.renderNode   = int32_t(S.rnode);
  hit.renderPrimID = S.renderPrimID;
  hit.triangle     = S.prim;
  hit.materialID   = S.materialID;
  hit.position[0]  = __fmaf_rn(t, ray.direction[0], ray.origin[0]);
  hit.position[1]  = __fmaf_rn(t, ray.direction[1], ray.origin[1]);
  hit.position[2]  = __fmaf_rn(t, ray.direction[2], ray.origin[2]);
  // unit geometric normal of the world-space triangle; the edges are brought to unit scale first so that neither a tiny nor a huge triangle
  // leaves the range of the squared length
  f3          e1 = xyz(T.b), e2 = xyz(T.c);
  const float m  = fmaxf(fmaxf(fmaxf(fabsf(e1.x), fabsf(e1.y)), fmaxf(fabsf(e1.z), fabsf(e2.x))), fmaxf(fabsf(e2.y), fabsf(e2.z)));
  const float s  = divExact(1.0f, m);
  e1 = e1 * s;
  e2 = e2 * s;
  f3 n = normalizeExact(crossFma(e1, e2));
  if(dotFma(n, mk3(ray.direction)) > 0.0f)
    n = -n;
  hit.normal[0] = n.x;
  hit.normal[1] = n.y;
  hit.normal[2] = n.z;
  return hit;
}

// ---- mi_pt_query_rays_ex / mi_pt_query_rays_device_ex / mi_pt_pick_ex ------------------------------------------------------------------------------
// What the candidate test reads of MiPtQueryOptions (validated by the host); the same for every ray of a call.
struct QueryRules
{
  int32_t  alpha, cull;  // MI_PT_QUERY_ALPHA_*, MI_PT_QUERY_CULL_*
  int32_t  maxHits;      // records per ray, 1..K of the kernel
  float    blendThreshold;
  uint32_t seed;
};
// The rules of the plain entry points -- every triangle opaque, no culling, one record per ray: the plain kernels serve them (query.hip), and a
// pick under them needs no ray scratch (mi_pt_api.hip).
inline bool queryRulesPlain(const QueryRules& q) { return q.alpha == MI_PT_QUERY_ALPHA_OPAQUE && q.cull == MI_PT_QUERY_CULL_NONE && q.maxHits == 1; }
// The frames' camera-ray rule (pt_kernels.hip, triRoundFinish): a triangle that shows the ray the back of its OBJECT-space winding is culled unless
// its instance disables culling.  worldFront: TriHit::front.
PT_DEV bool queryCullPasses(uint32_t instFlags, bool worldFront, int32_t cull)
{
  const bool frontFace = worldFront != ((instFlags & INST_FLIP_FACING) != 0u);
  return cull == MI_PT_QUERY_CULL_NONE || frontFace || (instFlags & INST_CULL_DISABLE) != 0u;
}
// The seed of ray `rayIndex` of a call: candidateRand(querySeed, renderNode, triangle) is the draw of one (ray, triangle) pair, whichever of the
// triangle's pre-split references the walk meets and however often.
PT_DEV uint32_t querySeed(uint32_t seed, uint32_t rayIndex) { return xxhash32(seed, rayIndex, 0u); }
// CUTOFF: opacity >= threshold (a MASK surface's opacity is 0 or 1 already: it follows its material's cutoff); STOCHASTIC: draw <= opacity, the
// closest-hit rule of the frames.
PT_DEV bool queryAlphaDecision(int32_t alpha, float opacity, float blendThreshold, float draw)
{
  return alpha == MI_PT_QUERY_ALPHA_CUTOFF ? opacity >= blendThreshold : draw <= opacity;
}
// instFlags: DevTri::c.w.  A triangle without INST_FORCE_OPAQUE / INST_ALPHA_PASSES implies DevScene::alphaTris (the host checks before it launches).
PT_DEV bool queryAlphaPasses(const DevScene& sc, int triIndex, uint32_t instFlags, uint32_t rnode, uint32_t prim, float u, float v, const QueryRules& q,
                             uint32_t raySeed)
{
  if(q.alpha == MI_PT_QUERY_ALPHA_OPAQUE || (instFlags & (INST_FORCE_OPAQUE | INST_ALPHA_PASSES)) != 0u)
    return true;
  const float opacity = getOpacityFast(sc, triIndex, mk3(1.0f - u - v, u, v));
  return queryAlphaDecision(q.alpha, opacity, q.blendThreshold, candidateRand(raySeed, int(rnode), int(prim)));
}

// a goes before b: smaller t, exact ties by (renderNode, triangle); an empty entry (tri < 0) goes after everything
PT_DEV bool queryBefore(const QueryBest& a, const QueryBest& b)
{
  return a.tri >= 0 && (b.tri < 0 || a.t < b.t || (a.t == b.t && (a.rnode < b.rnode || (a.rnode == b.rnode && a.prim < b.prim))));
}
// The K accepted distinct triangles with the smallest (t, renderNode, triangle), ascending; distinct by (renderNode, triangle), so a triangle the
// tree holds as several pre-split references (the same whole triangle in every slot: the same t) is listed once.  Every index below is a
// compile-time constant once the loops are unrolled: the list lives in registers.
template <int K>
struct QueryList
{
  QueryBest e[K];
};
template <int K>
PT_DEV QueryList<K> queryListEmpty(float tMax)
{
  QueryList<K> L;
#pragma unroll
  for(int j = 0; j < K; ++j)
    L.e[j] = queryNoHit(tMax);
  return L;
}
template <int K>
PT_DEV void queryListInsert(QueryList<K>& L, QueryBest c)
{
  bool listed = false;
#pragma unroll
  for(int j = 0; j < K; ++j)
    listed = listed || (L.e[j].tri >= 0 && L.e[j].rnode == c.rnode && L.e[j].prim == c.prim);
  if(listed)
    return;
#pragma unroll
  for(int j = 0; j < K; ++j)  // bubble through: c takes the place of the first entry it goes before, that entry moves on
  {
    if(queryBefore(c, L.e[j]))
    {
      const QueryBest moved = L.e[j];
      L.e[j]                = c;
      c                     = moved;
    }
  }
}
// What the node tests may cull with: the t of the maxHits-th entry once the list holds that many, `far` until then.
template <int K>
PT_DEV float queryListBound(const QueryList<K>& L, int maxHits, float far)
{
  float bound = far;
#pragma unroll
  for(int j = 0; j < K; ++j)
    if(j == maxHits - 1 && L.e[j].tri >= 0)
      bound = L.e[j].t;
  return bound;
}
// The candidate test of the _ex walks, in the order the header states: acceptance interval, culling, alpha; then the list.  Returns whether the
// triangle was accepted.
template <int K>
PT_DEV bool queryTestTriEx(const DevScene& sc, const RaySetup& r, int triIndex, float tMin, float tMax, const QueryRules& q, uint32_t raySeed,
                           QueryList<K>& L)
{
  const DevTri T = sc.tris[triIndex];
  TriHit       h;
  if(!intersectTri(xyz(T.a), xyz(T.b), xyz(T.c), r.org, r.dir, h) || !queryAccept(h.t, tMin, tMax))
    return false;
  const uint32_t rnode = __float_as_uint(T.a.w), prim = __float_as_uint(T.b.w), instFlags = __float_as_uint(T.c.w);
  if(!queryCullPasses(instFlags, h.front, q.cull) || !queryAlphaPasses(sc, triIndex, instFlags, rnode, prim, h.u, h.v, q, raySeed))
    return false;
  QueryBest c;
  c.t = h.t; c.u = h.u; c.v = h.v; c.tri = triIndex; c.rnode = rnode; c.prim = prim; c.front = h.front;
  queryListInsert(L, c);
  return true;
}
// Record j of a ray's maxHits records: entry j of the list, a miss record where the list ends.
template <int K>
PT_DEV MiPtRayHit queryListRecord(const DevScene& sc, const QueryList<K>& L, int j, const MiPtRay& ray)
{
  const QueryBest& b = L.e[j];
  return b.tri < 0 ? queryMiss(0u) : fillHit(sc, b.tri, b.t, b.u, b.v, b.front, ray);
}

}  // namespace pt
