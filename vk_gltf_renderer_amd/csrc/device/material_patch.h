// The per-thread work of the in-place material update (material_update.hip, mi_pt_update_materials): what a build bakes of a material into the
// per-triangle data -- the instance-flag word of the triangle record (DevTri::c.w), the alpha record (DevAlphaTri) and, when a render node
// takes ANOTHER material (mi_pt_update_render_nodes in resident mode), the material id of the shade record (DevShadeTri) -- rewritten for the
// slots of the render nodes whose material changed, from the SAME text the build runs (triangleFlagWord of bvh_refit.h, makeAlphaRecord and
// shadeRecordMaterial of pt_shading.h), so that a patched slot holds, byte for byte, what a fresh build over the new tables writes.  Compiles for the host as well
// (tests/host_shim/material_patch_on_host.cpp).
#pragma once
#include "bvh_refit.h"
#include "pt_shading.h"

namespace pt {

// What a triangle slot's render node owes after a material update (the dirty byte table of k_patch_materials); 0 = the slot stays as it is
enum : uint8_t
{
  MATERIAL_PATCH_FLAGS = 1,  // the instance flags of its material changed: the flag word of the triangle record
  MATERIAL_PATCH_ALPHA = 2,  // something makeAlphaRecord reads changed: the alpha record
  MATERIAL_PATCH_SHADE = 4,  // the render node's materialID changed: the material id of the shade record
};

// k_patch_materials, one triangle slot `s` (a pre-split reference is a slot like any other: every reference of a triangle carries the full
// record).  The record's render node and triangle index (DevTri a.w, b.w) and its geometry never change here.  `alphaTris` may be NULL
// (a scene without alpha records): the alpha bit is then ignored; so is the shade bit without `shadeTris`.
PT_DEV void patchMaterialSlot(const DevScene& sc, const uint8_t* instFlags, const uint8_t* dirty, DevTri* tris, DevAlphaTri* alphaTris, DevShadeTri* shadeTris,
                              uint32_t s)
{
  const int     rnode = __float_as_int(tris[s].a.w);
  const uint8_t what  = dirty[rnode];
  if(what == 0)
    return;
  if(what & MATERIAL_PATCH_FLAGS)
  {
    const uint32_t t = __float_as_uint(tris[s].b.w);
    tris[s].c.w      = __uint_as_float(triangleFlagWord(sc.prims[sc.nodes[rnode].renderPrimID], t, uint32_t(instFlags[rnode])));
  }
  if((what & MATERIAL_PATCH_ALPHA) && alphaTris)
    alphaTris[s] = makeAlphaRecord(sc, tris[s]);
  if((what & MATERIAL_PATCH_SHADE) && shadeTris)
    shadeTris[s].materialID = shadeRecordMaterial(sc.nodes[rnode]);
}
// ... without shade records (mi_pt_update_materials changes no render node's material id)
PT_DEV void patchMaterialSlot(const DevScene& sc, const uint8_t* instFlags, const uint8_t* dirty, DevTri* tris, DevAlphaTri* alphaTris, uint32_t s)
{
  patchMaterialSlot(sc, instFlags, dirty, tris, alphaTris, nullptr, s);
}

}  // namespace pt
