// In-place material update (mi_pt_update_materials, and the material-id changes of mi_pt_update_render_nodes in resident mode): the one kernel behind it.  The tables themselves are plain copies; what a build derived
// from them per triangle -- the flag word of the triangle record, the alpha record -- is patched here for the slots of the render nodes whose
// material changed, one thread per triangle slot of the active order.  A slot whose render node is clean reads 4 bytes of its record and one
// byte of the table and leaves; an update that changes no instance flag and nothing the alpha records hold does not launch this at all.
// The per-thread work lives in material_patch.h.
#include <hip/hip_runtime.h>

#include "material_patch.h"
#include "pt_kernels.h"

namespace pt {

namespace {

__global__ void __launch_bounds__(256) k_patch_materials(DevScene sc, const uint8_t* __restrict__ instFlags, const uint8_t* __restrict__ dirty, DevTri* tris,
                                                         DevAlphaTri* alphaTris, DevShadeTri* shadeTris, uint32_t numTris)
{
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s < numTris)
    patchMaterialSlot(sc, instFlags, dirty, tris, alphaTris, shadeTris, s);
}

}  // namespace

void launchPatchMaterials(const DevScene& scene, const uint8_t* instFlags, const uint8_t* dirty, DevTri* tris, DevAlphaTri* alphaTris, DevShadeTri* shadeTris,
                          uint32_t numTris, hipStream_t s)
{
  if(numTris == 0)
    return;
  hipLaunchKernelGGL(k_patch_materials, dim3((numTris + 255u) / 256u), dim3(256), 0, s, scene, instFlags, dirty, tris, alphaTris, shadeTris, numTris);
}

}  // namespace pt
