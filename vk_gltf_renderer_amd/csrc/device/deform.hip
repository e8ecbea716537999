// k_deform: morph targets and skinning of every deforming render primitive in one launch (pt_deform.h).  Per vertex, in registers:
//   morph  p = base + sum_t w_t dp_t over the targets with w_t != 0; n and t.xyz likewise, then normalised (tangent w kept)
//          (reference: shaders/morph.comp.slang);
//   skin   p = sum_i w_i (J_i [p, 1]).xyz, n = normalize(sum_i w_i N_i n), t.xyz = normalize(sum_i w_i mat3(J_i) t.xyz) over the influences
//          with w_i > 0 and a joint inside the skin (reference: shaders/skinning.comp.slang);
//   a primitive that is both is morphed, normalised, then skinned: the reference's two passes over the vertex buffers, in one.
// The results go to the separate streams (builders, alpha records, guides) AND to the interleaved DevPrim::verts record the shade kernels
// read -- float4 0 whole, n.y / n.z of float4 1 (uv0 untouched), float4 2 -- so both agree with what mi_pt_create would upload.
// Compiled with the default IEEE flags (not PT_KERNELS_FP): sqrt and division are correctly rounded, as in the host restatement.
// Joint tables stay in global memory (L1 / L2), not LDS: see LABNOTES.md, "Skinning and morph targets on the device".
#include "pt_deform.h"

namespace pt {

#if defined(__HIP_DEVICE_COMPILE__)
#define DF_GLOBAL __attribute__((address_space(1)))
#define DF_CONST __attribute__((address_space(4)))
#else  // (the host pass of hipcc parses the kernel too)
#define DF_GLOBAL
#define DF_CONST
#endif

namespace {

// The stream pointers come out of the task record: generic pointers to the compiler, whose loads and stores would be flat (counted on
// both memory counters, a full drain at every use).  They all point to global memory; saying so gives global_load / global_store.
template <class T>
__device__ __forceinline__ T ld(const T* p, size_t i)
{
  return *((const DF_GLOBAL T*)p + i);
}
template <class T>
__device__ __forceinline__ void st(T* p, size_t i, T v)
{
  *((DF_GLOBAL T*)p + i) = v;
}

__device__ inline float3 normalized(float3 v)
{
  const float l = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
  return make_float3(v.x / l, v.y / l, v.z / l);
}

}  // namespace

__global__ __launch_bounds__(DEFORM_BLOCK) void k_deform(const DeformTask* __restrict__ tasks, const uint32_t* __restrict__ blockTask)
{
  const uint32_t   ti = __builtin_amdgcn_readfirstlane(blockTask[blockIdx.x]);
  const DeformTask T  = *((const DF_CONST DeformTask*)tasks + ti);  // block-uniform, constant: scalar loads
  const uint32_t   v  = (blockIdx.x - T.firstBlock) * DEFORM_BLOCK + threadIdx.x;
  if(v >= T.vertexCount)
    return;
  const uint32_t flags = T.flags;
  const float4   b0    = ld(T.base, size_t(v) * 3);
  float3         p     = make_float3(b0.x, b0.y, b0.z);
  float3         n     = make_float3(0.0f, 0.0f, 0.0f);
  float4         t     = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if(flags & DF_NORMALS)
  {
    const float4 b1 = ld(T.base, size_t(v) * 3 + 1);
    n               = make_float3(b0.w, b1.x, b1.y);
  }
  if(flags & DF_TANGENTS)
    t = ld(T.base, size_t(v) * 3 + 2);

  if(T.numTargets > 0)
  {
    const size_t vc = T.vertexCount;
    for(uint32_t k = 0; k < T.numTargets; ++k)
    {
      const float w = *((const DF_CONST float*)T.morphWeights + k);  // (block-uniform: scalar)
      if(w == 0.0f)
        continue;
      const size_t o = (size_t(k) * vc + v) * 3;
      p.x += w * ld(T.posDeltas, o);
      p.y += w * ld(T.posDeltas, o + 1);
      p.z += w * ld(T.posDeltas, o + 2);
      if(flags & DF_MORPH_N)
      {
        n.x += w * ld(T.nrmDeltas, o);
        n.y += w * ld(T.nrmDeltas, o + 1);
        n.z += w * ld(T.nrmDeltas, o + 2);
      }
      if(flags & DF_MORPH_T)
      {
        t.x += w * ld(T.tanDeltas, o);
        t.y += w * ld(T.tanDeltas, o + 1);
        t.z += w * ld(T.tanDeltas, o + 2);
      }
    }
    if(flags & DF_MORPH_N)
      n = normalized(n);
    if(flags & DF_MORPH_T)
    {
      const float3 u = normalized(make_float3(t.x, t.y, t.z));
      t              = make_float4(u.x, u.y, u.z, t.w);
    }
  }

  if(flags & DF_SKIN)
  {
    const uint2  jp = ld(T.joints, v);
    const float4 wv = ld(T.weights, v);
    const uint32_t ji[4] = {jp.x & 0xffffu, jp.x >> 16, jp.y & 0xffffu, jp.y >> 16};
    const float    wi[4] = {wv.x, wv.y, wv.z, wv.w};
    float3         sp = make_float3(0.0f, 0.0f, 0.0f), sn = sp, st = sp;
#pragma unroll
    for(int i = 0; i < 4; ++i)
    {
      const float w = wi[i];
      if(!(w > 0.0f) || ji[i] >= T.numJoints)
        continue;
      const size_t  M  = size_t(ji[i]) * 6;
      const float4  r0 = ld(T.jointTable, M), r1 = ld(T.jointTable, M + 1), r2 = ld(T.jointTable, M + 2);
      sp.x += w * (r0.x * p.x + r0.y * p.y + r0.z * p.z + r0.w);
      sp.y += w * (r1.x * p.x + r1.y * p.y + r1.z * p.z + r1.w);
      sp.z += w * (r2.x * p.x + r2.y * p.y + r2.z * p.z + r2.w);
      if(flags & DF_NORMALS)
      {
        const float4 n0 = ld(T.jointTable, M + 3), n1 = ld(T.jointTable, M + 4), n2 = ld(T.jointTable, M + 5);
        sn.x += w * (n0.x * n.x + n0.y * n.y + n0.z * n.z);
        sn.y += w * (n1.x * n.x + n1.y * n.y + n1.z * n.z);
        sn.z += w * (n2.x * n.x + n2.y * n.y + n2.z * n.z);
      }
      if(flags & DF_TANGENTS)
      {
        st.x += w * (r0.x * t.x + r0.y * t.y + r0.z * t.z);
        st.y += w * (r1.x * t.x + r1.y * t.y + r1.z * t.z);
        st.z += w * (r2.x * t.x + r2.y * t.y + r2.z * t.z);
      }
    }
    p = sp;
    n = normalized(sn);
    const float3 u = normalized(st);
    t              = make_float4(u.x, u.y, u.z, t.w);
  }

  const size_t v3 = size_t(v) * 3;
  st(T.outPositions, v3, p.x);
  st(T.outPositions, v3 + 1, p.y);
  st(T.outPositions, v3 + 2, p.z);
  st(T.outVerts, v3, make_float4(p.x, p.y, p.z, (flags & DF_NORMALS) ? n.x : b0.w));
  if(flags & DF_NORMALS)
  {
    st(T.outNormals, v3, n.x);
    st(T.outNormals, v3 + 1, n.y);
    st(T.outNormals, v3 + 2, n.z);
    st(reinterpret_cast<float2*>(T.outVerts + v3 + 1), 0, make_float2(n.y, n.z));  // (uv0, the other half of float4 1, stays)
  }
  if(flags & DF_TANGENTS)
  {
    st(reinterpret_cast<float4*>(T.outTangents), v, t);
    st(T.outVerts, v3 + 2, t);
  }
}

void launchDeform(const DeformTask* tasks, const uint32_t* blockTask, uint32_t numBlocks, hipStream_t stream)
{
  if(numBlocks == 0)
    return;
  hipLaunchKernelGGL(k_deform, dim3(numBlocks), dim3(DEFORM_BLOCK), 0, stream, tasks, blockTask);
}

}  // namespace pt
