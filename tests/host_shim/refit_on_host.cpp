// TEST INFRASTRUCTURE ONLY.  The per-thread work of the BVH refit (csrc/device/bvh_refit.h: the triangle record of k_tri_setup / k_refit_tris,
// the quantisation of k_collapse_emit / k_refit_level) compiled for the host through the stand-in <hip/hip_runtime.h> of this directory, so
// that the CPU-only test tier (tests/test_bvh_refit_on_host.py) runs the code the device runs.  Never loaded by the product.
#include "bvh_refit.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// The builder's quantisation of one node: frame [lo, hi], child boxes clo / chi as [axis][slot], `used` slots.  node: 80 bytes in / out.
EXPORT void refit_quantise(Node8* node, const float* lo, const float* hi, const float* clo, const float* chi, uint32_t used)
{
  float l[3][8], h[3][8];
  for(int a = 0; a < 3; ++a)
    for(int s = 0; s < 8; ++s)
    {
      l[a][s] = clo[a * 8 + s];
      h[a][s] = chi[a * 8 + s];
    }
  quantiseNode8(*node, lo, hi, l, h, used);
}

// k_refit_level over every level, deepest first (levels: numLevels + 1 starts, the last = the node count)
EXPORT void refit_levels(Node8* nodes, const uint32_t* levels, int numLevels, const RefitBox* slotBox, RefitBox* nodeBox, float* sahTerm)
{
  for(int l = numLevels - 1; l >= 0; --l)
    for(uint32_t n = levels[l]; n < levels[l + 1]; ++n)
      sahTerm[n] = refitNode8(nodes[n], slotBox, nodeBox, nodeBox[n]);
}

// k_refit_tris over every slot; one primitive (prims[0]) shared by all render nodes
EXPORT void refit_tris(const MiGltfRenderNode* nodes, const uint32_t* indices, const float* positions, uint32_t opaqueTriangles, const uint8_t* instFlags,
                       const uint8_t* dirty, const RefitBox* builtBox, DevTri* tris, RefitBox* slotBox, uint32_t numSlots)
{
  DevPrim p;
  std::memset(&p, 0, sizeof(p));
  p.indices         = indices;
  p.positions       = positions;
  p.opaqueTriangles = opaqueTriangles;
  for(uint32_t s = 0; s < numSlots; ++s)
    refitTriSlot(nodes, &p, instFlags, dirty, builtBox, tris, slotBox, s);
}
