// TEST INFRASTRUCTURE ONLY.  The per-ray work of the _ex ray queries (csrc/device/pt_query.h, second half: face culling, the alpha decision
// through getOpacityFast, the sorted list of the K nearest distinct triangles, the record fill) compiled for the host through the stand-in
// <hip/hip_runtime.h> of this directory, so that the CPU-only test tier (tests/test_query_ex_on_host.py, tests/test_query_ex_reference.py) runs
// the code the device runs.  Never loaded by the product.
#include <cstddef>

#include "pt_query.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// size and offsets of MiPtQueryOptions as the compiler lays it out, the new enum values, and the ABI version the header states
EXPORT void query_ex_layout(int32_t* out)
{
  int i = 0;
  out[i++] = int32_t(sizeof(MiPtQueryOptions));
  out[i++] = int32_t(offsetof(MiPtQueryOptions, mode));
  out[i++] = int32_t(offsetof(MiPtQueryOptions, alpha));
  out[i++] = int32_t(offsetof(MiPtQueryOptions, cull));
  out[i++] = int32_t(offsetof(MiPtQueryOptions, maxHits));
  out[i++] = int32_t(offsetof(MiPtQueryOptions, blendThreshold));
  out[i++] = int32_t(offsetof(MiPtQueryOptions, seed));
  out[i++] = int32_t(offsetof(MiPtQueryOptions, reserved));
  out[i++] = MI_PT_ABI_VERSION;
  out[i++] = MI_PT_QUERY_CLOSEST;
  out[i++] = MI_PT_QUERY_ANY;
  out[i++] = MI_PT_QUERY_NEAREST_K;
  out[i++] = MI_PT_QUERY_ALPHA_OPAQUE;
  out[i++] = MI_PT_QUERY_ALPHA_CUTOFF;
  out[i++] = MI_PT_QUERY_ALPHA_STOCHASTIC;
  out[i++] = MI_PT_QUERY_CULL_NONE;
  out[i++] = MI_PT_QUERY_CULL_MATERIAL;
  out[i++] = MI_PT_QUERY_MAX_HITS;
}

namespace {
DevScene sceneOf(const DevTri* tris, const DevShadeTri* shadeTris, const DevAlphaTri* alphaTris, const uchar4* texels)
{
  DevScene sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.tris      = tris;
  sc.shadeTris = shadeTris;
  sc.alphaTris = alphaTris;
  sc.texels    = texels;  // (texQuads stays NULL: getOpacityFast takes its four-fetch path, the same arithmetic)
  return sc;
}
// What a walk that visits every triangle slot of `order` returns for one ray: queryOneEx (query.hip) without the tree.
template <int K>
void brute(const DevScene& sc, const int32_t* order, int numTris, const MiPtRay& ray, uint32_t rayIndex, const QueryRules& q, bool any, MiPtRayHit* out)
{
  QueryList<K> L     = queryListEmpty<K>(ray.tMax);
  const bool   valid = queryRayValid(ray);
  if(valid)
  {
    const float    tMin = queryTMin(ray.tMin), tMax = ray.tMax;
    const RaySetup r    = makeRaySetup(mk3(ray.origin), mk3(ray.direction));
    const uint32_t raySeed = querySeed(q.seed, rayIndex);
    if(tMin < tMax)
      for(int i = 0; i < numTris; ++i)
        if(queryTestTriEx(sc, r, order[i], tMin, tMax, q, raySeed, L) && any)
          break;
  }
  for(int j = 0; j < q.maxHits; ++j)
    out[j] = j == 0 && !valid ? queryMiss(MI_PT_HIT_INVALID_RAY) : queryListRecord(sc, L, j, ray);
}
}  // namespace

// rules: alpha, cull, maxHits, blendThreshold, seed (QueryRules).  out: numRays x maxHits records.  K is chosen as the launcher chooses it.
EXPORT void query_ex_brute(const DevTri* tris, const DevShadeTri* shadeTris, const DevAlphaTri* alphaTris, const uchar4* texels, const int32_t* order,
                           int numTris, const MiPtRay* rays, int numRays, int firstRayIndex, const QueryRules* rules, int any, MiPtRayHit* out)
{
  const DevScene   sc = sceneOf(tris, shadeTris, alphaTris, texels);
  const QueryRules q  = *rules;
  for(int i = 0; i < numRays; ++i)
  {
    MiPtRayHit*    o  = out + size_t(i) * size_t(q.maxHits);
    const uint32_t ri = uint32_t(firstRayIndex + i);
    if(q.maxHits <= 1)
      brute<1>(sc, order, numTris, rays[i], ri, q, any != 0, o);
    else if(q.maxHits <= 2)
      brute<2>(sc, order, numTris, rays[i], ri, q, false, o);
    else if(q.maxHits <= 4)
      brute<4>(sc, order, numTris, rays[i], ri, q, false, o);
    else
      brute<8>(sc, order, numTris, rays[i], ri, q, false, o);
  }
}

EXPORT float query_ex_opacity(const DevAlphaTri* alphaTris, const uchar4* texels, int triIndex, float u, float v)
{
  const DevScene sc = sceneOf(nullptr, nullptr, alphaTris, texels);
  return getOpacityFast(sc, triIndex, mk3(1.0f - u - v, u, v));
}
EXPORT float    query_ex_draw(uint32_t seed, uint32_t rayIndex, uint32_t rnode, uint32_t prim) { return candidateRand(querySeed(seed, rayIndex), int(rnode), int(prim)); }
EXPORT int      query_ex_cull_passes(uint32_t instFlags, int worldFront, int cull) { return queryCullPasses(instFlags, worldFront != 0, cull) ? 1 : 0; }
EXPORT int      query_ex_alpha_decision(int alpha, float opacity, float threshold, float draw) { return queryAlphaDecision(alpha, opacity, threshold, draw) ? 1 : 0; }
