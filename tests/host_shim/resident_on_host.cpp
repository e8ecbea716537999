// TEST INFRASTRUCTURE ONLY.  The per-thread work of resident mode (mi_pt_set_accel_resident) compiled for the host through the stand-in
// <hip/hip_runtime.h> of this directory, so that the CPU-only test tier (tests/test_resident_on_host.py) runs the code the device runs: the
// refit with hidden slots (csrc/device/bvh_refit.h: REFIT_HIDDEN in refitTriSlot, emptiness in refitNode8) under the entry points of
// refit_on_host.cpp, and the material patch with shade records (csrc/device/material_patch.h: MATERIAL_PATCH_SHADE) next to the build-time
// function it must agree with (makeShadeRecord of k_shade_records).  Never loaded by the product.
#include "material_patch.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

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
    {
      RefitBox own;
      sahTerm[n] = refitNode8(nodes[n], slotBox, nodeBox, own);
      nodeBox[n] = own;
    }
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

// One render primitive as plain arrays, one resident texture (the layouts of material_patch_on_host.cpp)
struct ShimPrim
{
  const uint32_t* indices;
  const float*    positions;
  const uint32_t* colors;
  const float*    texCoords0;
  const float*    texCoords1;
  uint32_t        opaqueTriangles;
  uint32_t        pad;
};
struct ShimTexture
{
  uint32_t level0;
  uint16_t width, height;
  uint8_t  magFilter, wrapS, wrapT, pad;
};

namespace {
struct Tables
{
  std::vector<DevPrim>    prims;
  std::vector<DevTexture> textures;
  DevScene                sc;
};
Tables makeScene(const MiGltfRenderNode* nodes, int numNodes, const ShimPrim* prims, int numPrims, const MiGltfShadeMaterial* materials, int numMaterials,
                 const MiGltfTextureInfo* infos, const ShimTexture* textures, int numTextures)
{
  Tables t;
  t.prims.resize(size_t(numPrims));
  for(int i = 0; i < numPrims; ++i)
  {
    DevPrim& d = t.prims[size_t(i)];
    std::memset(&d, 0, sizeof(d));
    d.indices = prims[i].indices; d.positions = prims[i].positions; d.colors = prims[i].colors;
    d.texCoords0 = prims[i].texCoords0; d.texCoords1 = prims[i].texCoords1; d.opaqueTriangles = prims[i].opaqueTriangles;
  }
  t.textures.resize(size_t(numTextures));
  for(int i = 0; i < numTextures; ++i)
  {
    DevTexture& d = t.textures[size_t(i)];
    std::memset(&d, 0, sizeof(d));
    d.levelOffset[0] = textures[i].level0; d.width = textures[i].width; d.height = textures[i].height; d.numLevels = 1;
    d.magFilter = textures[i].magFilter; d.wrapS = textures[i].wrapS; d.wrapT = textures[i].wrapT;
  }
  std::memset(&t.sc, 0, sizeof(t.sc));
  t.sc.nodes = nodes; t.sc.numNodes = numNodes; t.sc.materials = materials; t.sc.numMaterials = numMaterials; t.sc.texInfos = infos;
  t.sc.numTextures = numTextures;
  return t;
}
}  // namespace

// The build: worldTriangle, makeAlphaRecord and makeShadeRecord for every slot.  tris / alphaTris: 48 bytes per slot, shadeTris: 32.
EXPORT void resident_build(const MiGltfRenderNode* nodes, int numNodes, const ShimPrim* prims, int numPrims, const MiGltfShadeMaterial* materials, int numMaterials,
                           const MiGltfTextureInfo* infos, const ShimTexture* textures, int numTextures, const uint8_t* instFlags, const int32_t* slotNode,
                           const uint32_t* slotTri, uint32_t numSlots, DevTri* tris, DevAlphaTri* alphaTris, DevShadeTri* shadeTris)
{
  Tables t   = makeScene(nodes, numNodes, prims, numPrims, materials, numMaterials, infos, textures, numTextures);
  t.sc.prims = t.prims.data(); t.sc.textures = t.textures.data(); t.sc.tris = tris;
  for(uint32_t s = 0; s < numSlots; ++s)
  {
    const int rn = slotNode[s];
    float     lo[3], hi[3];
    worldTriangle(nodes[rn], t.prims[size_t(nodes[rn].renderPrimID)], rn, slotTri[s], uint32_t(instFlags[rn]), tris[s], lo, hi);
  }
  for(uint32_t s = 0; s < numSlots; ++s)
  {
    alphaTris[s] = makeAlphaRecord(t.sc, tris[s]);
    shadeTris[s] = makeShadeRecord(t.sc, tris[s]);
  }
}

// k_patch_materials over every slot, under the NEW node table, tables and flags; alphaTris and shadeTris may be NULL
EXPORT void resident_patch(const MiGltfRenderNode* nodes, int numNodes, const ShimPrim* prims, int numPrims, const MiGltfShadeMaterial* materials, int numMaterials,
                           const MiGltfTextureInfo* infos, const ShimTexture* textures, int numTextures, const uint8_t* instFlags, const uint8_t* dirty,
                           uint32_t numSlots, DevTri* tris, DevAlphaTri* alphaTris, DevShadeTri* shadeTris)
{
  Tables t   = makeScene(nodes, numNodes, prims, numPrims, materials, numMaterials, infos, textures, numTextures);
  t.sc.prims = t.prims.data(); t.sc.textures = t.textures.data(); t.sc.tris = tris;
  for(uint32_t s = 0; s < numSlots; ++s)
    patchMaterialSlot(t.sc, instFlags, dirty, tris, alphaTris, shadeTris, s);
}
