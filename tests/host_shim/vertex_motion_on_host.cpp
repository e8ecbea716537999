// TEST INFRASTRUCTURE ONLY.  The motion record of a hit on deforming geometry (csrc/device/pt_temporal.h: motionRecordDeformed) and the rigid
// one it falls back to (motionRecord), compiled for the host through the stand-in <hip/hip_runtime.h> of this directory, so that
// tests/test_vertex_motion_on_host.py can diff them against a float64 numpy restatement on the CPU.  Built by the test session only.
#include <cmath>
#include <cstddef>
#include <vector>

#include "pt_temporal.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// One render primitive as the test hands it over; prevPositions NULL = the primitive does not deform.
struct ShimPrim
{
  const float*    prevPositions;
  const float*    positions;
  const uint32_t* indices;
  uint32_t        numTriangles, vertexCount;
};

// n first-hit records + n triangle records (primitive, triangle, bits of b1, bits of b2) -> n motion records
EXPORT void dev_vertex_motion_records(int n, const float* firstHit, const uint32_t* tri, const ShimPrim* prims, int numPrims, const void* nodes,
                                      const float* prevObjectToWorld, int numNodes, const float* viewProj, const float* prevMVP, float width, float height,
                                      float* out)
{
  std::vector<VertexMotionPrim> table(size_t(numPrims > 0 ? numPrims : 0));
  for(int i = 0; i < numPrims; ++i)
    table[size_t(i)] = VertexMotionPrim{prims[i].prevPositions, prims[i].positions, prims[i].indices, prims[i].numTriangles, prims[i].vertexCount};
  for(int i = 0; i < n; ++i)
  {
    const float4 r = motionRecordDeformed(make_float4(firstHit[4 * i], firstHit[4 * i + 1], firstHit[4 * i + 2], firstHit[4 * i + 3]),
                                          make_uint4(tri[4 * i], tri[4 * i + 1], tri[4 * i + 2], tri[4 * i + 3]), table.data(), numPrims,
                                          static_cast<const MiGltfRenderNode*>(nodes), prevObjectToWorld, numNodes, viewProj, prevMVP, width, height);
    out[4 * i] = r.x, out[4 * i + 1] = r.y, out[4 * i + 2] = r.z, out[4 * i + 3] = r.w;
  }
}

// the rigid record of the same first hits: what the fallbacks must return byte for byte
EXPORT void dev_rigid_motion_records(int n, const float* firstHit, const void* nodes, const float* prevObjectToWorld, int numNodes, const float* viewProj,
                                     const float* prevMVP, float width, float height, float* out)
{
  for(int i = 0; i < n; ++i)
  {
    const float4 r = motionRecord(make_float4(firstHit[4 * i], firstHit[4 * i + 1], firstHit[4 * i + 2], firstHit[4 * i + 3]),
                                  static_cast<const MiGltfRenderNode*>(nodes), prevObjectToWorld, numNodes, viewProj, prevMVP, width, height);
    out[4 * i] = r.x, out[4 * i + 1] = r.y, out[4 * i + 2] = r.z, out[4 * i + 3] = r.w;
  }
}
