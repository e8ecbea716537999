// Caller-driven vertices of resident render primitives (vertex_update.hip; C-ABI: mi_pt_set_vertex_updates / mi_pt_update_vertices /
// mi_pt_update_vertices_device).  Two kernels, both shaped like k_deform (pt_deform.h): ONE launch serves every primitive of a call, each
// primitive's vertex range padded to whole 256-thread blocks, so a block serves one task and reads its record through the scalar cache.
//   ingest   copies the caller's positions (+ normals, tangents) into the separate streams AND the interleaved DevPrim::verts record --
//            the bytes mi_pt_create would upload for the same arrays.  A vertex with a non-finite supplied component is REJECTED: it keeps
//            all its resident values, so a non-finite position never reaches the refit or the builder.
//   normals  (MI_PT_VERTICES_RECOMPUTE_NORMALS) rebuilds the vertex normals of the resident positions: the float32 sum of
//            cross(p1 - p0, p2 - p0) over the vertex's incident corners, ascending triangle then corner, divided by its length.
// The per-vertex and per-corner work lives here as plain functions over a memory policy `Mem` (ld / st of a typed element): the kernels
// pass address-space-qualified global accesses, tests/host_shim/vertex_update_on_host.cpp plain ones, so the CPU tier runs the same text.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace pt {

constexpr int VERTEX_UPDATE_BLOCK = 256;

enum : uint32_t
{
  VU_NORMALS  = 1u,  // the call supplies normals (written)
  VU_TANGENTS = 2u,  // the call supplies tangents (written, w included)
};

// Elements of the caller's arrays: tightly packed and 4-byte aligned, whatever the vertex index.
struct alignas(4) VuVec3
{
  float x, y, z;
};
struct alignas(4) VuVec4
{
  float x, y, z, w;
};
struct alignas(4) VuTri  // the three indices of a triangle
{
  uint32_t a, b, c;
};

// One primitive of an update call (block-uniform: loaded with scalar loads).
struct VertexUpdateTask
{
  const float* positions;     // the caller's arrays, device memory (the staging buffer for the host form)
  const float* normals;       // (VU_NORMALS)
  const float* tangents;      // (VU_TANGENTS)
  float*       outPositions;  // the resident streams (DevPrim)
  float*       outNormals;
  float*       outTangents;   // 16-byte aligned
  float4*      outVerts;      // DevPrim::verts
  uint32_t     vertexCount, firstBlock, flags, _pad;
};

// One primitive whose normals are rebuilt.  cornerEnd[v] = the end of vertex v's run in `corners` (it starts where vertex v - 1's ends);
// a corner is 3 * triangle + corner-in-triangle, runs in ascending order.
struct NormalRebuildTask
{
  const float*    positions;  // resident
  const uint32_t* indices;    // resident
  const uint32_t* cornerEnd;
  const uint32_t* corners;
  float*          outNormals;
  float4*         outVerts;
  uint32_t        vertexCount, firstBlock, _pad[2];
};

__host__ __device__ inline bool vuFinite(float v)
{
  return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u;  // (an integer test: no fast-math option can fold it away)
}

// Vertex v of the caller's arrays, each element loaded once; what the call does not supply is zero.
struct VuVertex
{
  VuVec3 p, n;
  VuVec4 t;
};
template <class Mem>
__host__ __device__ inline VuVertex vertexLoad(const VertexUpdateTask& T, uint32_t v)
{
  VuVertex r{};
  r.p = Mem::ld(reinterpret_cast<const VuVec3*>(T.positions), v);
  if(T.flags & VU_NORMALS)
    r.n = Mem::ld(reinterpret_cast<const VuVec3*>(T.normals), v);
  if(T.flags & VU_TANGENTS)
    r.t = Mem::ld(reinterpret_cast<const VuVec4*>(T.tangents), v);
  return r;
}

// Whether the vertex may be written: every supplied component is finite (the zeros of what is not supplied are).  No short circuit: one
// straight run of integer tests.
__host__ __device__ inline bool vertexAcceptable(const VuVertex& r)
{
  const float    c[10] = {r.p.x, r.p.y, r.p.z, r.n.x, r.n.y, r.n.z, r.t.x, r.t.y, r.t.z, r.t.w};
  uint32_t       bad   = 0;
  for(int i = 0; i < 10; ++i)
    bad |= uint32_t(!vuFinite(c[i]));
  return bad == 0u;
}

// The write of vertex v: the streams, and of the interleaved record float4 0 (its w only with normals), n.y / n.z of float4 1 (uv0, the other
// half, stays) and float4 2.  What is not supplied keeps its bytes.
template <class Mem>
__host__ __device__ inline void vertexWrite(const VertexUpdateTask& T, uint32_t v, const VuVertex& r)
{
  const size_t v3 = size_t(v) * 3;
  Mem::st(reinterpret_cast<VuVec3*>(T.outPositions), v, r.p);
  if(T.flags & VU_NORMALS)
  {
    Mem::st(reinterpret_cast<VuVec3*>(T.outNormals), v, r.n);
    Mem::st(T.outVerts, v3, make_float4(r.p.x, r.p.y, r.p.z, r.n.x));
    Mem::st(reinterpret_cast<float2*>(T.outVerts + v3 + 1), 0, make_float2(r.n.y, r.n.z));
  }
  else
    Mem::st(reinterpret_cast<VuVec3*>(T.outVerts + v3), 0, r.p);  // (n.x, the fourth word, stays)
  if(T.flags & VU_TANGENTS)
  {
    const float4 t4 = make_float4(r.t.x, r.t.y, r.t.z, r.t.w);
    Mem::st(reinterpret_cast<float4*>(T.outTangents), v, t4);
    Mem::st(T.outVerts, v3 + 2, t4);
  }
}

// cross(p1 - p0, p2 - p0): twice the triangle's area along its normal.
__host__ __device__ inline VuVec3 faceCross(VuVec3 p0, VuVec3 p1, VuVec3 p2)
{
  const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
  const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
  return VuVec3{ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
}

// sum / |sum| with IEEE sqrt and division; false (and `out` untouched) when the length is zero or not finite.
__host__ __device__ inline bool normalFromSum(VuVec3 s, VuVec3& out)
{
  const float l = sqrtf(s.x * s.x + s.y * s.y + s.z * s.z);
  if(!(l > 0.0f) || !vuFinite(l))
    return false;
  out = VuVec3{s.x / l, s.y / l, s.z / l};
  return true;
}

// The rebuilt normal of vertex v, written to the stream and the record; a vertex without one (no incident area) keeps its resident normal.
template <class Mem>
__host__ __device__ inline void vertexRebuildNormal(const NormalRebuildTask& T, uint32_t v)
{
  const uint32_t end = Mem::ld(T.cornerEnd, v);
  uint32_t       k   = v ? Mem::ld(T.cornerEnd, v - 1) : 0u;
  VuVec3         s{0.0f, 0.0f, 0.0f};
  for(; k < end; ++k)
  {
    const VuTri   t = Mem::ld(reinterpret_cast<const VuTri*>(T.indices), Mem::ld(T.corners, k) / 3u);
    const VuVec3* P = reinterpret_cast<const VuVec3*>(T.positions);
    const VuVec3  c = faceCross(Mem::ld(P, t.a), Mem::ld(P, t.b), Mem::ld(P, t.c));
    s.x += c.x;
    s.y += c.y;
    s.z += c.z;
  }
  VuVec3 n;
  if(!normalFromSum(s, n))
    return;
  const size_t v3 = size_t(v) * 3;
  Mem::st(reinterpret_cast<VuVec3*>(T.outNormals), v, n);
  Mem::st(reinterpret_cast<float*>(T.outVerts + v3) + 3, 0, n.x);
  Mem::st(reinterpret_cast<float2*>(T.outVerts + v3 + 1), 0, make_float2(n.y, n.z));
}

#if defined(__HIPCC__)
// tasks / blockTask: device arrays (blockTask[b] = the task of block b); numBlocks = sum of ceil(vertexCount / VERTEX_UPDATE_BLOCK).
// rejected: one device word the ingest adds its rejected vertices to (one atomic per wave that rejects any).
void launchVertexIngest(const VertexUpdateTask* tasks, const uint32_t* blockTask, uint32_t numBlocks, uint32_t* rejected, hipStream_t stream);
void launchNormalRebuild(const NormalRebuildTask* tasks, const uint32_t* blockTask, uint32_t numBlocks, hipStream_t stream);
#endif

}  // namespace pt
