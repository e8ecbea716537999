// TEST INFRASTRUCTURE ONLY.  The per-vertex and per-corner functions of caller-driven vertex updates (csrc/device/pt_vertex_update.h: vertexLoad,
// vertexAcceptable, vertexWrite, vertexRebuildNormal) compiled for the host through the stand-in <hip/hip_runtime.h> of this directory, over
// plain memory accesses where the kernels use address-space-qualified ones, so that tests/test_vertex_update_on_host.py can diff what they
// write against numpy restatements on the CPU.  Built by the test session only.
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "pt_vertex_update.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

namespace {
struct PlainMem
{
  template <class T>
  static T ld(const T* p, size_t i)
  {
    return p[i];
  }
  template <class T>
  static void st(T* p, size_t i, T v)
  {
    p[i] = v;
  }
};
}  // namespace

// What k_vertex_ingest does, vertex by vertex: returns the number of rejected vertices, rejected[v] = 1 for each (may be NULL).
EXPORT uint32_t dev_vertex_ingest(uint32_t vertexCount, const float* positions, const float* normals, const float* tangents, float* outPositions,
                                  float* outNormals, float* outTangents, float* outVerts, uint8_t* rejected)
{
  VertexUpdateTask T{};
  T.positions    = positions;
  T.normals      = normals;
  T.tangents     = tangents;
  T.outPositions = outPositions;
  T.outNormals   = outNormals;
  T.outTangents  = outTangents;
  T.outVerts     = reinterpret_cast<float4*>(outVerts);
  T.vertexCount  = vertexCount;
  T.flags        = (normals ? VU_NORMALS : 0u) | (tangents ? VU_TANGENTS : 0u);
  uint32_t bad   = 0;
  for(uint32_t v = 0; v < vertexCount; ++v)
  {
    const VuVertex r  = vertexLoad<PlainMem>(T, v);
    const bool     ok = vertexAcceptable(r);
    if(ok)
      vertexWrite<PlainMem>(T, v, r);
    else
      ++bad;
    if(rejected)
      rejected[v] = ok ? 0 : 1;
  }
  return bad;
}

// What k_rebuild_normals does, vertex by vertex.
EXPORT void dev_rebuild_normals(uint32_t vertexCount, const float* positions, const uint32_t* indices, const uint32_t* cornerEnd, const uint32_t* corners,
                                float* outNormals, float* outVerts)
{
  NormalRebuildTask T{};
  T.positions   = positions;
  T.indices     = indices;
  T.cornerEnd   = cornerEnd;
  T.corners     = corners;
  T.outNormals  = outNormals;
  T.outVerts    = reinterpret_cast<float4*>(outVerts);
  T.vertexCount = vertexCount;
  for(uint32_t v = 0; v < vertexCount; ++v)
    vertexRebuildNormal<PlainMem>(T, v);
}
