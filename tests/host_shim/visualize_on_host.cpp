// TEST INFRASTRUCTURE ONLY.  The debug views of the shade kernel (csrc/device/pt_visualize.h: applyVisualization, hashToColor)
// compiled for the host through the stand-in <hip/hip_runtime.h> of this directory, so that tests/test_visualize_on_host.py can
// diff them against a numpy restatement on the CPU.  Built by the test session only; never loaded by the product.
#include <cstddef>

#include "pt_visualize.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// PbrMaterial is plain floats: the test fills it as a float array, at the offsets (in floats) listed here in this order
EXPORT int dev_viz_material_layout(int* offsets)
{
  const size_t o[] = {offsetof(PbrMaterial, baseColor),   offsetof(PbrMaterial, opacity),       offsetof(PbrMaterial, roughness),
                      offsetof(PbrMaterial, metallic),    offsetof(PbrMaterial, emissive),      offsetof(PbrMaterial, occlusion),
                      offsetof(PbrMaterial, N),           offsetof(PbrMaterial, T),             offsetof(PbrMaterial, B),
                      offsetof(PbrMaterial, Ng),          offsetof(PbrMaterial, specular),      offsetof(PbrMaterial, specularColor),
                      offsetof(PbrMaterial, transmission), offsetof(PbrMaterial, clearcoat),    offsetof(PbrMaterial, clearcoatRoughness),
                      offsetof(PbrMaterial, Nc),          offsetof(PbrMaterial, iridescence),   offsetof(PbrMaterial, iridescenceThickness),
                      offsetof(PbrMaterial, sheenColor),  offsetof(PbrMaterial, sheenRoughness), offsetof(PbrMaterial, diffuseTransmissionFactor),
                      offsetof(PbrMaterial, diffuseTransmissionColor)};
  for(size_t i = 0; i < sizeof(o) / sizeof(o[0]); ++i)
    offsets[i] = int(o[i] / sizeof(float));
  return int(sizeof(PbrMaterial) / sizeof(float));
}

// mat: in / out (clay changes it in place); uv: uv0.xy, uv1.xy; colour: out
EXPORT int dev_apply_visualization(float* mat, const float* uv, int frontFace, int mode, int rprimID, int primitiveID, int ommState, float* colour)
{
  PbrMaterial m;
  std::memcpy(&m, mat, sizeof(m));
  HitState hit{};
  hit.uv0 = mk2(uv[0], uv[1]);
  hit.uv1 = mk2(uv[2], uv[3]);
  f3        c;
  const int r = applyVisualization(m, hit, frontFace != 0, mode, rprimID, primitiveID, ommState, c);
  std::memcpy(mat, &m, sizeof(m));
  colour[0] = c.x;
  colour[1] = c.y;
  colour[2] = c.z;
  return r;
}

EXPORT void dev_hash_to_color(uint32_t id, float* colour)
{
  const f3 c = hashToColor(id);
  colour[0]  = c.x;
  colour[1]  = c.y;
  colour[2]  = c.z;
}
