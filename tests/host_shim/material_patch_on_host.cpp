// TEST INFRASTRUCTURE ONLY.  The per-thread work of the in-place material update (csrc/device/material_patch.h: patchMaterialSlot of
// k_patch_materials) and the build-time functions it must agree with (worldTriangle of k_tri_setup, makeAlphaRecord of k_alpha_records),
// compiled for the host through the stand-in <hip/hip_runtime.h> of this directory, so that the CPU-only test tier
// (tests/test_material_patch_on_host.py) runs the code the device runs.  Never loaded by the product.
#include "material_patch.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// One render primitive as plain arrays (colors / texCoords may be NULL)
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
// One resident texture: what makeAlphaRecord reads of its descriptor
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

// The build: worldTriangle for every slot (slotNode / slotTri: the render node and the triangle index of each slot) under instFlags, then
// makeAlphaRecord for every slot under the given tables.  tris / alphaTris: numSlots records of 48 bytes each.
EXPORT void patch_build(const MiGltfRenderNode* nodes, int numNodes, const ShimPrim* prims, int numPrims, const MiGltfShadeMaterial* materials, int numMaterials,
                        const MiGltfTextureInfo* infos, const ShimTexture* textures, int numTextures, const uint8_t* instFlags, const int32_t* slotNode,
                        const uint32_t* slotTri, uint32_t numSlots, DevTri* tris, DevAlphaTri* alphaTris)
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
    alphaTris[s] = makeAlphaRecord(t.sc, tris[s]);
}

// k_patch_materials over every slot, under the NEW tables and flags; alphaTris may be NULL
EXPORT void patch_slots(const MiGltfRenderNode* nodes, int numNodes, const ShimPrim* prims, int numPrims, const MiGltfShadeMaterial* materials, int numMaterials,
                        const MiGltfTextureInfo* infos, const ShimTexture* textures, int numTextures, const uint8_t* instFlags, const uint8_t* dirty,
                        uint32_t numSlots, DevTri* tris, DevAlphaTri* alphaTris)
{
  Tables t   = makeScene(nodes, numNodes, prims, numPrims, materials, numMaterials, infos, textures, numTextures);
  t.sc.prims = t.prims.data(); t.sc.textures = t.textures.data(); t.sc.tris = tris;
  for(uint32_t s = 0; s < numSlots; ++s)
    patchMaterialSlot(t.sc, instFlags, dirty, tris, alphaTris, s);
}
