// TEST INFRASTRUCTURE ONLY.  The host collapse of the 8-wide BVH (csrc/device/bvh8_collapse_host.h) compiled for the host through the stand-in
// <hip/hip_runtime.h> of this directory, so that the CPU-only test tier (tests/test_bvh8_collapse_on_host.py) runs the code the builder runs
// behind MI_PT_HOST_COLLAPSE=1 and for a one-triangle scene.  Never loaded by the product.
#include "bvh8_collapse_host.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// nodes2: numInner BVH2 records of 4 x float4; nodesOut: room for max(numInner, 1) nodes; permOut: room for n.  Returns the node count, or -1
// where the permutation does not hold n entries (the builder's "lost triangles").
EXPORT int collapse_on_host(const float4* nodes2, int root, uint32_t numInner, uint32_t n, const float* loneLo, const float* loneHi, Node8* nodesOut,
                            uint32_t* permOut, uint32_t* numLevels)
{
  const Bvh8OnHost h = collapseBvh8OnHost(nodes2, root, numInner, n, loneLo, loneHi);
  if(h.perm.size() != n || h.nodes.size() > std::max(numInner, 1u))
    return -1;
  std::memcpy(nodesOut, h.nodes.data(), h.nodes.size() * sizeof(Node8));
  std::memcpy(permOut, h.perm.data(), h.perm.size() * sizeof(uint32_t));
  *numLevels = h.numLevels;
  return int(h.nodes.size());
}
