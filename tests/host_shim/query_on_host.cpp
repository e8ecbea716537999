// TEST INFRASTRUCTURE ONLY.  The per-ray work of the ray queries (csrc/device/pt_query.h: ray validation, the acceptance test, the closest-hit
// rule and fillHit) compiled for the host through the stand-in <hip/hip_runtime.h> of this directory, so that the CPU-only test tier
// (tests/test_query_on_host.py) runs the code the device runs.  Never loaded by the product.
#include <cstddef>

#include "pt_query.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// sizes and offsets of the public records as the compiler lays them out, and the ABI version the header states
EXPORT void query_layout(int32_t* out)
{
  int i = 0;
  out[i++] = int32_t(sizeof(MiPtRay));
  out[i++] = int32_t(offsetof(MiPtRay, origin));
  out[i++] = int32_t(offsetof(MiPtRay, tMin));
  out[i++] = int32_t(offsetof(MiPtRay, direction));
  out[i++] = int32_t(offsetof(MiPtRay, tMax));
  out[i++] = int32_t(sizeof(MiPtRayHit));
  out[i++] = int32_t(offsetof(MiPtRayHit, t));
  out[i++] = int32_t(offsetof(MiPtRayHit, b1));
  out[i++] = int32_t(offsetof(MiPtRayHit, b2));
  out[i++] = int32_t(offsetof(MiPtRayHit, flags));
  out[i++] = int32_t(offsetof(MiPtRayHit, renderNode));
  out[i++] = int32_t(offsetof(MiPtRayHit, renderPrimID));
  out[i++] = int32_t(offsetof(MiPtRayHit, triangle));
  out[i++] = int32_t(offsetof(MiPtRayHit, materialID));
  out[i++] = int32_t(offsetof(MiPtRayHit, position));
  out[i++] = int32_t(offsetof(MiPtRayHit, reserved0));
  out[i++] = int32_t(offsetof(MiPtRayHit, normal));
  out[i++] = int32_t(offsetof(MiPtRayHit, reserved1));
  out[i++] = MI_PT_ABI_VERSION;
  out[i++] = MI_PT_HIT;
  out[i++] = MI_PT_HIT_FRONT_FACE;
  out[i++] = MI_PT_HIT_INVALID_RAY;
  out[i++] = MI_PT_QUERY_CLOSEST;
  out[i++] = MI_PT_QUERY_ANY;
}

EXPORT int   query_ray_valid(const MiPtRay* ray) { return queryRayValid(*ray) ? 1 : 0; }
EXPORT int   query_accept(float t, float tMin, float tMax) { return queryAccept(t, tMin, tMax) ? 1 : 0; }
EXPORT float query_tmin(float tMin) { return queryTMin(tMin); }
// makeRaySetup of a ray: out6 = idir, ood
EXPORT void query_ray_setup(const MiPtRay* ray, float* out6)
{
  const RaySetup r = makeRaySetup(mk3(ray->origin), mk3(ray->direction));
  out6[0] = r.idir.x; out6[1] = r.idir.y; out6[2] = r.idir.z; out6[3] = r.ood.x; out6[4] = r.ood.y; out6[5] = r.ood.z;
}
EXPORT void query_miss(uint32_t flags, MiPtRayHit* out) { *out = queryMiss(flags); }
EXPORT void query_fill_hit(const DevTri* tris, const DevShadeTri* shadeTris, int triIndex, float t, float u, float v, int front, const MiPtRay* ray, MiPtRayHit* out)
{
  DevScene sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.tris      = tris;
  sc.shadeTris = shadeTris;
  *out         = fillHit(sc, triIndex, t, u, v, front != 0, *ray);
}
// What a walk that visits every triangle returns: the kernel's per-ray code (query.hip: queryOne) without the tree.  order: the triangle slots
// in the order a walk would meet them (numTris entries).
EXPORT void query_brute(const DevTri* tris, const DevShadeTri* shadeTris, const int32_t* order, int numTris, const MiPtRay* ray, int any, MiPtRayHit* out)
{
  DevScene sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.tris      = tris;
  sc.shadeTris = shadeTris;
  if(!queryRayValid(*ray))
  {
    *out = queryMiss(MI_PT_HIT_INVALID_RAY);
    return;
  }
  const float    tMin = queryTMin(ray->tMin), tMax = ray->tMax;
  const RaySetup r    = makeRaySetup(mk3(ray->origin), mk3(ray->direction));
  QueryBest      best = queryNoHit(tMax);
  for(int i = 0; i < numTris; ++i)
    if(queryTestTri(sc, r, order[i], tMin, tMax, best) && any)
      break;
  *out = best.tri < 0 ? queryMiss(0u) : fillHit(sc, best.tri, best.t, best.u, best.v, best.front, *ray);
}
