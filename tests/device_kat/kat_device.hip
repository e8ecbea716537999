// TEST INFRASTRUCTURE ONLY: known-answer launchers over the product's device headers, compiled for gfx950 with the flags of
// pt_kernels.o (csrc/Makefile: $(HIPFLAGS) $(PT_KERNELS_FP)) so that tests/test_gpu_device_kat.py sees the arithmetic that ships --
// hardware reciprocal, v_exp / v_log / v_sin / v_cos -- function by function.  The headers are included unmodified; nothing of
// libmi_pt.so is linked and that library gains nothing from this file.
//
// Built twice into one library (tests/device_kat/libmi_pt_kat.so): without KAT_IEEE every group below, exported as kat_<group>; with
// -DKAT_IEEE and WITHOUT $(PT_KERNELS_FP) the exact-math group alone, exported as kat_<group>_ieee -- divExact / sqrtExact /
// intersectTri / makeRaySetup promise the same bits "whatever the compile options".
//
// Every launcher takes HOST pointers, one case per thread, and returns the hipError_t (0 = success) of the first call that failed.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#ifndef KAT_IEEE
#define PT_FAST_SHADING_MATH 1  // as pt_kernels.hip defines it before its includes
#define KAT_NAME(x) x
#else
#define KAT_NAME(x) x##_ieee
#endif
#include "pt_shading.h"
#include "pt_bvh.h"
#include "pt_bvh8.h"
#include "../host_shim/material_from_array.h"  // (by path: that directory also holds a stand-in <hip/hip_runtime.h>)

using namespace pt;

namespace {
// host arrays -> device copies -> (kernel) -> results back; the first error sticks and later steps are skipped
struct Kat
{
  struct Buf
  {
    void*  dev;
    void*  hostOut;
    size_t bytes;
  };
  int              err = int(hipSuccess);
  std::vector<Buf> bufs;
  void* alloc(const void* hostIn, void* hostOut, size_t bytes)
  {
    void* d = nullptr;
    if(err == int(hipSuccess) && bytes)
      err = int(hipMalloc(&d, bytes));
    if(d)
      bufs.push_back({d, hostOut, bytes});
    if(d && err == int(hipSuccess))
      err = int(hostIn ? hipMemcpy(d, hostIn, bytes, hipMemcpyHostToDevice) : hipMemset(d, 0, bytes));
    return d;
  }
  template <typename T> const T* in(const T* h, size_t count) { return static_cast<const T*>(alloc(h, nullptr, count * sizeof(T))); }
  template <typename T> T*       out(T* h, size_t count) { return static_cast<T*>(alloc(nullptr, h, count * sizeof(T))); }
  bool ok() const { return err == int(hipSuccess); }
  int  finish()  // after the launch
  {
    if(ok()) err = int(hipGetLastError());
    if(ok()) err = int(hipDeviceSynchronize());
    for(const Buf& b : bufs)
    {
      if(ok() && b.hostOut)
        err = int(hipMemcpy(b.hostOut, b.dev, b.bytes, hipMemcpyDeviceToHost));
      (void)hipFree(b.dev);
    }
    bufs.clear();
    return err;
  }
};
constexpr int BLOCK = 64;
dim3 gridFor(int n) { return dim3(unsigned((n + BLOCK - 1) / BLOCK)); }
#define KAT_EXPORT extern "C" __attribute__((visibility("default")))
}  // namespace

// ---- exact class: both builds ----------------------------------------------------------------------------------------------
// op 0 divExact(a, b)  1 sqrtExact(a)  2 normalizeExact(a, b, c)  3 logExact(a)  4 sinExact(a)  5 cosExact(a)  6 powExact(a, b)  7 srgbOetf(a)
__global__ void KAT_NAME(k_kat_exact)(int n, int op, const float* __restrict__ in3, float* __restrict__ out3)
{
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if(i >= n)
    return;
  const float a = in3[3 * i], b = in3[3 * i + 1], c = in3[3 * i + 2];
  f3          r = mk3(0.0f);
  switch(op)
  {
    case 0: r.x = divExact(a, b); break;
    case 1: r.x = sqrtExact(a); break;
    case 2: r = normalizeExact(mk3(a, b, c)); break;
    case 3: r.x = logExact(a); break;
    case 4: r.x = sinExact(a); break;
    case 5: r.x = cosExact(a); break;
    case 6: r.x = powExact(a, b); break;
    case 7: r.x = srgbOetf(a); break;
  }
  out3[3 * i] = r.x; out3[3 * i + 1] = r.y; out3[3 * i + 2] = r.z;
}
KAT_EXPORT int KAT_NAME(kat_exact)(int n, int op, const float* in3, float* out3)
{
  if(n <= 0)
    return 0;
  Kat          k;
  const float* dIn  = k.in(in3, size_t(n) * 3);
  float*       dOut = k.out(out3, size_t(n) * 3);
  if(k.ok())
    hipLaunchKernelGGL(KAT_NAME(k_kat_exact), gridFor(n), dim3(BLOCK), 0, 0, n, op, dIn, dOut);
  return k.finish();
}

// in15 = v0 e1 e2 org dir; out5 = hit t u v front (0 / 1 as floats; t, u, v are 0 on a miss)
__global__ void KAT_NAME(k_kat_intersect_tri)(int n, const float* __restrict__ in15, float* __restrict__ out5)
{
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if(i >= n)
    return;
  const float* p = in15 + 15 * i;
  TriHit       h;
  h.t = h.u = h.v = 0.0f;
  h.front         = false;
  const bool hit  = intersectTri(mk3(p), mk3(p + 3), mk3(p + 6), mk3(p + 9), mk3(p + 12), h);
  float*     o    = out5 + 5 * i;
  o[0] = hit ? 1.0f : 0.0f;
  o[1] = hit ? h.t : 0.0f; o[2] = hit ? h.u : 0.0f; o[3] = hit ? h.v : 0.0f;
  o[4] = (hit && h.front) ? 1.0f : 0.0f;
}
KAT_EXPORT int KAT_NAME(kat_intersect_tri)(int n, const float* in15, float* out5)
{
  if(n <= 0)
    return 0;
  Kat          k;
  const float* dIn  = k.in(in15, size_t(n) * 15);
  float*       dOut = k.out(out5, size_t(n) * 5);
  if(k.ok())
    hipLaunchKernelGGL(KAT_NAME(k_kat_intersect_tri), gridFor(n), dim3(BLOCK), 0, 0, n, dIn, dOut);
  return k.finish();
}

// in6 = org dir; out6 = idir ood
__global__ void KAT_NAME(k_kat_ray_setup)(int n, const float* __restrict__ in6, float* __restrict__ out6)
{
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if(i >= n)
    return;
  const RaySetup r = makeRaySetup(mk3(in6 + 6 * i), mk3(in6 + 6 * i + 3));
  float*         o = out6 + 6 * i;
  o[0] = r.idir.x; o[1] = r.idir.y; o[2] = r.idir.z; o[3] = r.ood.x; o[4] = r.ood.y; o[5] = r.ood.z;
}
KAT_EXPORT int KAT_NAME(kat_ray_setup)(int n, const float* in6, float* out6)
{
  if(n <= 0)
    return 0;
  Kat          k;
  const float* dIn  = k.in(in6, size_t(n) * 6);
  float*       dOut = k.out(out6, size_t(n) * 6);
  if(k.ok())
    hipLaunchKernelGGL(KAT_NAME(k_kat_ray_setup), gridFor(n), dim3(BLOCK), 0, 0, n, dIn, dOut);
  return k.finish();
}

#ifndef KAT_IEEE
// ---- the node test of the 8-wide walk ---------------------------------------------------------------------------------------
// nodes: 20 words per case (the five uint4 of bvh8.hip's layout); planes: 48 floats per case, block 2 * axis + side (side 0 = lower
// planes), eight children each (DevScene::bvh8Planes); ray7 = org dir tmax.  out3 = mask of bvh8TestChildren, its leaf word, mask of
// bvh8TestChildrenPlanes with the near / far blocks chosen by the direction's sign as k_trace_primary does.
__global__ void k_kat_node_test(int n, const uint32_t* __restrict__ nodes, const float* __restrict__ planes, const float* __restrict__ ray7,
                                uint32_t* __restrict__ out3)
{
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if(i >= n)
    return;
  const uint32_t* w = nodes + 20 * i;
  const uint4     n0 = make_uint4(w[0], w[1], w[2], w[3]), n1 = make_uint4(w[4], w[5], w[6], w[7]), n2 = make_uint4(w[8], w[9], w[10], w[11]);
  const uint4     n3 = make_uint4(w[12], w[13], w[14], w[15]), n4 = make_uint4(w[16], w[17], w[18], w[19]);
  const float*    q  = ray7 + 7 * i;
  const RaySetup  r  = makeRaySetup(mk3(q), mk3(q + 3));
  const float     tmax = q[6];
  uint32_t        hm, leaf;
  bvh8TestChildren(n0, n1, n2, n3, n4, r, tmax, hm, leaf);
  const bool   neg[3] = {r.idir.x < 0.0f, r.idir.y < 0.0f, r.idir.z < 0.0f};
  const float* P      = planes + 48 * i;
  f32x8s       pn[3], pf[3];
  for(int a = 0; a < 3; ++a)
    for(int c = 0; c < 8; ++c)
    {
      pn[a][c] = P[(2 * a + (neg[a] ? 1 : 0)) * 8 + c];
      pf[a][c] = P[(2 * a + (neg[a] ? 0 : 1)) * 8 + c];
    }
  const uint32_t hmP = bvh8TestChildrenPlanes(n0, pn[0], pn[1], pn[2], pf[0], pf[1], pf[2], r, tmax, neg[0] ? 1.0f : -1.0f, neg[1] ? 1.0f : -1.0f,
                                              neg[2] ? 1.0f : -1.0f);
  out3[3 * i] = hm; out3[3 * i + 1] = leaf; out3[3 * i + 2] = hmP;
}
KAT_EXPORT int kat_node_test(int n, const uint32_t* nodes, const float* planes, const float* ray7, uint32_t* out3)
{
  if(n <= 0)
    return 0;
  Kat             k;
  const uint32_t* dN = k.in(nodes, size_t(n) * 20);
  const float*    dP = k.in(planes, size_t(n) * 48);
  const float*    dR = k.in(ray7, size_t(n) * 7);
  uint32_t*       dO = k.out(out3, size_t(n) * 3);
  if(k.ok())
    hipLaunchKernelGGL(k_kat_node_test, gridFor(n), dim3(BLOCK), 0, 0, n, dN, dP, dR, dO);
  return k.finish();
}

// ---- the layered BSDF -------------------------------------------------------------------------------------------------------
// mode 0 bsdfSample, 1 bsdfSampleSimple; mat: 29 floats per case (oracle/oracle_pt.h); out8 = k2 bsdf_over_pdf pdf event_type
__global__ void k_kat_bsdf_sample(int n, int mode, const float* __restrict__ mat, const float* __restrict__ k1, const float* __restrict__ xi,
                                  float* __restrict__ out8)
{
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if(i >= n)
    return;
  const PbrMaterial m = materialFromArray(mat + 29 * i);
  const BsdfSample  d = mode == 0 ? bsdfSample(mk3(k1 + 3 * i), mk3(xi + 3 * i), m) : bsdfSampleSimple(mk3(k1 + 3 * i), mk3(xi + 3 * i), m);
  float*            o = out8 + 8 * i;
  o[0] = d.k2.x; o[1] = d.k2.y; o[2] = d.k2.z;
  o[3] = d.bsdf_over_pdf.x; o[4] = d.bsdf_over_pdf.y; o[5] = d.bsdf_over_pdf.z; o[6] = d.pdf;
  o[7] = float(d.event_type);
}
KAT_EXPORT int kat_bsdf_sample(int n, int mode, const float* mat, const float* k1, const float* xi, float* out8)
{
  if(n <= 0)
    return 0;
  Kat          k;
  const float* dM = k.in(mat, size_t(n) * 29);
  const float* dK = k.in(k1, size_t(n) * 3);
  const float* dX = k.in(xi, size_t(n) * 3);
  float*       dO = k.out(out8, size_t(n) * 8);
  if(k.ok())
    hipLaunchKernelGGL(k_kat_bsdf_sample, gridFor(n), dim3(BLOCK), 0, 0, n, mode, dM, dK, dX, dO);
  return k.finish();
}
// out4 = bsdf (diffuse * occlusion + glossy, occlusion = 1) pdf
__global__ void k_kat_bsdf_eval(int n, const float* __restrict__ mat, const float* __restrict__ k1, const float* __restrict__ k2, const float* __restrict__ xi,
                                float* __restrict__ out4)
{
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if(i >= n)
    return;
  const BsdfEval e = bsdfEvaluate(mk3(k1 + 3 * i), mk3(k2 + 3 * i), mk3(xi + 3 * i), materialFromArray(mat + 29 * i));
  float*         o = out4 + 4 * i;
  o[0] = e.bsdf.x; o[1] = e.bsdf.y; o[2] = e.bsdf.z; o[3] = e.pdf;
}
KAT_EXPORT int kat_bsdf_eval(int n, const float* mat, const float* k1, const float* k2, const float* xi, float* out4)
{
  if(n <= 0)
    return 0;
  Kat          k;
  const float* dM  = k.in(mat, size_t(n) * 29);
  const float* dK1 = k.in(k1, size_t(n) * 3);
  const float* dK2 = k.in(k2, size_t(n) * 3);
  const float* dX  = k.in(xi, size_t(n) * 3);
  float*       dO  = k.out(out4, size_t(n) * 4);
  if(k.ok())
    hipLaunchKernelGGL(k_kat_bsdf_eval, gridFor(n), dim3(BLOCK), 0, 0, n, dM, dK1, dK2, dX, dO);
  return k.finish();
}

// ---- building blocks with closed forms --------------------------------------------------------------------------------------
// in8 / out4 per case.  op:
//  0 ior_fresnel(eta, cos)                         1 schlickFresnelIor(ior, cos)
//  2 fresnel_conductor(n_a, n_b, k_b, cos, max(0, 1 - cos^2)) -> Rs Rp
//  3 thin_film_factor(thickness, coatingIor, baseIor, incomingIor, cos) -> rgb
//  4 hvd_ggx_eval((1 / ax, 1 / ay) as given, h)    5 smith_shadow_mask(k, (ax, ay))       in: ax ay v.x v.y v.z
//  6 hvd_ggx_sample_vndf(k, (ax, ay), (u, v)) -> h                                        in: ax ay k.x k.y k.z u v
//  7 hvd_sheen_eval(invRoughness, nh)              8 henyeyGreensteinPdf(cos, g)
//  9 sampleHenyeyGreenstein((u, v), g, normalize(wi)) -> wo                               in: u v g wi.x wi.y wi.z
// 10 fresnel_dielectric(n_a, n_b, cos_a, cos_b) -> Rs Rp                              11 isTIR((ior1, ior2), kh) -> 0 / 1
__global__ void k_kat_blocks(int n, int op, const float* __restrict__ in8, float* __restrict__ out4)
{
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if(i >= n)
    return;
  const float* p = in8 + 8 * i;
  float        r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  switch(op)
  {
    case 0: r[0] = ior_fresnel(p[0], p[1]); break;
    case 1: r[0] = schlickFresnelIor(p[0], p[1]); break;
    case 2: {
      f2       ps, pc;
      const f2 R = fresnel_conductor(ps, pc, p[0], p[1], p[2], p[3], fmaxf(0.0f, 1.0f - p[3] * p[3]));
      r[0] = R.x; r[1] = R.y;
      break;
    }
    case 3: {
      const f3 c = thin_film_factor(p[0], p[1], p[2], p[3], p[4]);
      r[0] = c.x; r[1] = c.y; r[2] = c.z;
      break;
    }
    case 4: r[0] = hvd_ggx_eval(mk2(p[0], p[1]), mk3(p + 2)); break;
    case 5: r[0] = smith_shadow_mask(mk3(p + 2), mk2(p[0], p[1])); break;
    case 6: {
      const f3 h = hvd_ggx_sample_vndf(mk3(p + 2), mk2(p[0], p[1]), mk2(p[5], p[6]));
      r[0] = h.x; r[1] = h.y; r[2] = h.z;
      break;
    }
    case 7: r[0] = hvd_sheen_eval(p[0], p[1]); break;
    case 8: r[0] = henyeyGreensteinPdf(p[0], p[1]); break;
    case 9: {
      const f3 w = sampleHenyeyGreenstein(mk2(p[0], p[1]), p[2], normalize(mk3(p + 3)));
      r[0] = w.x; r[1] = w.y; r[2] = w.z;
      break;
    }
    case 10: {
      const f2 R = fresnel_dielectric(p[0], p[1], p[2], p[3]);
      r[0] = R.x; r[1] = R.y;
      break;
    }
    case 11: r[0] = isTIR(mk2(p[0], p[1]), p[2]) ? 1.0f : 0.0f; break;
  }
  float* o = out4 + 4 * i;
  o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
}
KAT_EXPORT int kat_blocks(int n, int op, const float* in8, float* out4)
{
  if(n <= 0)
    return 0;
  Kat          k;
  const float* dIn  = k.in(in8, size_t(n) * 8);
  float*       dOut = k.out(out4, size_t(n) * 4);
  if(k.ok())
    hipLaunchKernelGGL(k_kat_blocks, gridFor(n), dim3(BLOCK), 0, 0, n, op, dIn, dOut);
  return k.finish();
}

// ---- sky and lights ---------------------------------------------------------------------------------------------------------
// one set of sky parameters per launch; in5 = dir u v; out11 = evalPhysicalSky(dir) rgb, samplePhysicalSkyPDF(dir), samplePhysicalSky(u, v): dir pdf rgb.
// evalPhysicalSky reads its two tables through uniformConst (pt_scene.h): they must lie in GLOBAL memory at one address for the whole wave, as the product's
// do (DevScene) -- a per-thread copy on the stack is no valid argument.  So the precomputed table is written by a one-thread kernel first.
__global__ void k_kat_sky_precomp(const MiSkyPhysicalParameters* __restrict__ sky, SkyPrecomp* __restrict__ pre)
{
  if(blockIdx.x == 0 && threadIdx.x == 0)
    *pre = makeSkyPrecomp(*sky);
}
__global__ void k_kat_sky(int n, const MiSkyPhysicalParameters* __restrict__ sky, const SkyPrecomp* __restrict__ pre, const float* __restrict__ in5,
                          float* __restrict__ out11)
{
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if(i >= n)
    return;
  const MiSkyPhysicalParameters& s = *sky;
  const SkyPrecomp&              k = *pre;
  const float*                   p = in5 + 5 * i;
  const f3                       d = mk3(p);
  const float                    gamma = skyGamma(k, d);
  const f3                       c = evalPhysicalSky(s, k, d, gamma);
  f3                             sd, sr;
  float                          spdf;
  samplePhysicalSky(s, k, mk2(p[3], p[4]), sd, spdf, sr);
  float* o = out11 + 11 * i;
  o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = samplePhysicalSkyPDF(s, k, gamma);
  o[4] = sd.x; o[5] = sd.y; o[6] = sd.z; o[7] = spdf; o[8] = sr.x; o[9] = sr.y; o[10] = sr.z;
}
KAT_EXPORT int kat_sky(int n, const MiSkyPhysicalParameters* sky, const float* in5, float* out11)
{
  if(n <= 0)
    return 0;
  Kat                            k;
  const MiSkyPhysicalParameters* dS = k.in(sky, 1);
  SkyPrecomp*                    dP = k.out(static_cast<SkyPrecomp*>(nullptr), 1);
  const float*                   dI = k.in(in5, size_t(n) * 5);
  float*                         dO = k.out(out11, size_t(n) * 11);
  if(k.ok())
  {
    hipLaunchKernelGGL(k_kat_sky_precomp, dim3(1), dim3(1), 0, 0, dS, dP);
    hipLaunchKernelGGL(k_kat_sky, gridFor(n), dim3(BLOCK), 0, 0, n, dS, dP, dI, dO);
  }
  return k.finish();
}
// one light per case; in5 = pos xi; out8 = incidentVector distance intensity pdf
__global__ void k_kat_light(int n, const MiGltfLight* __restrict__ lights, const float* __restrict__ in5, float* __restrict__ out8)
{
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if(i >= n)
    return;
  const float*       p = in5 + 5 * i;
  const LightContrib c = singleLightContribution(lights[i], mk3(p), mk2(p[3], p[4]));
  float*             o = out8 + 8 * i;
  o[0] = c.incidentVector.x; o[1] = c.incidentVector.y; o[2] = c.incidentVector.z; o[3] = c.distance;
  o[4] = c.intensity.x; o[5] = c.intensity.y; o[6] = c.intensity.z; o[7] = c.pdf;
}
KAT_EXPORT int kat_light(int n, const MiGltfLight* lights, const float* in5, float* out8)
{
  if(n <= 0)
    return 0;
  Kat                k;
  const MiGltfLight* dL = k.in(lights, size_t(n));
  const float*       dI = k.in(in5, size_t(n) * 5);
  float*             dO = k.out(out8, size_t(n) * 8);
  if(k.ok())
    hipLaunchKernelGGL(k_kat_light, gridFor(n), dim3(BLOCK), 0, 0, n, dL, dI, dO);
  return k.finish();
}
#endif  // !KAT_IEEE
