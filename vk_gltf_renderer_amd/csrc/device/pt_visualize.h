// Debug views of MiSceneFrameInfo::visualization (MI_VIZ_*): the device restatement of applyVisualization / hashToColor,
// shaders/common.h.slang:32-164.  Called by the visualization variant of the shade kernel (k_shade_viz, pt_kernels.hip) after the
// first-hit captures and the roughness ratchet (gltf_pathtrace.slang:270-287); the default kernels never include it.
#pragma once
#include "pt_bsdf.h"
#include "pt_shading.h"

namespace pt {

enum : int
{
  VIZ_RENDERED = 0,        // no override: shade as usual
  VIZ_COLOR_OVERRIDE,      // `colour` is the sample's radiance (first rays only; the path ends)
  VIZ_MATERIAL_OVERRIDE,   // the material was changed in place (clay); shading goes on with it
};

// 24-bit colour of an id: a PCG-style integer hash, one byte per channel
PT_DEV f3 hashToColor(uint32_t id)
{
  uint32_t h = id * 747796405u + 2891336453u;
  h          = ((h >> ((h >> 28u) + 4u)) ^ h) * 277803737u;
  h          = (h >> 22u) ^ h;
  return mk3(divExact(float(h & 0xffu), 255.0f), divExact(float((h >> 8) & 0xffu), 255.0f), divExact(float((h >> 16) & 0xffu), 255.0f));
}

PT_DEV f3 toSrgb(f3 c) { return mk3(srgbOetf(c.x), srgbOetf(c.y), srgbOetf(c.z)); }
PT_DEV float fract(float x) { return x - floorf(x); }

// mat: the hit's material after the roughness ratchet (changed in place by clay); frontFace: the ray met the triangle's front side
// (before getHitState turned the geometric normal towards the ray); rprimID / primitiveID: render primitive and triangle inside it;
// ommState: < 0 unknown (the mode renders), 0 resolved opaque at load time, > 0 alpha still tested by the walks.
PT_DEV int applyVisualization(PbrMaterial& mat, const HitState& hit, bool frontFace, int mode, int rprimID, int primitiveID, int ommState, f3& colour)
{
  colour = mk3(0.0f);
  switch(mode)
  {
    case MI_VIZ_BASE_COLOR: colour = toSrgb(mat.baseColor); break;
    case MI_VIZ_METALLIC: colour = toSrgb(mk3(mat.metallic)); break;
    case MI_VIZ_ROUGHNESS: colour = toSrgb(mk3(mat.roughness.x, mat.roughness.y, mat.roughness.x)); break;
    case MI_VIZ_NORMAL_SHADING: colour = toSrgb(mat.N * 0.5f + mk3(0.5f)); break;
    case MI_VIZ_NORMAL_GEOMETRIC: colour = mat.Ng * 0.5f + mk3(0.5f); break;
    case MI_VIZ_TANGENT: colour = mat.T * 0.5f + mk3(0.5f); break;
    case MI_VIZ_BITANGENT: colour = mat.B * 0.5f + mk3(0.5f); break;
    case MI_VIZ_EMISSIVE: colour = mat.emissive; break;
    case MI_VIZ_OPACITY: colour = mk3(mat.opacity * (1.0f - mat.transmission)); break;
    case MI_VIZ_TEXCOORD0: colour = mk3(fract(hit.uv0.x), fract(hit.uv0.y), 0.0f); break;
    case MI_VIZ_TEXCOORD1: colour = mk3(fract(hit.uv1.x), fract(hit.uv1.y), 0.0f); break;
    case MI_VIZ_CLAY:
      mat.baseColor = mk3(0.8f, 0.75f, 0.7f);
      mat.metallic  = 0.0f;
      mat.roughness = mk2(0.25f, 0.25f);  // roughness 0.5, squared
      mat.emissive  = mk3(0.0f);
      return VIZ_MATERIAL_OVERRIDE;
    case MI_VIZ_TRIANGLE_ID: colour = hashToColor(uint32_t(rprimID) * 65537u + uint32_t(primitiveID)); break;
    case MI_VIZ_FACE_ORIENTATION: colour = frontFace ? mk3(0.0f, 1.0f, 0.0f) : mk3(1.0f, 0.0f, 0.0f); break;
    case MI_VIZ_OCCLUSION: colour = mk3(mat.occlusion); break;
    case MI_VIZ_CLEARCOAT_FACTOR: colour = mk3(mat.clearcoat); break;
    case MI_VIZ_CLEARCOAT_ROUGHNESS: colour = mk3(mat.clearcoatRoughness); break;
    case MI_VIZ_CLEARCOAT_NORMAL: colour = mat.Nc * 0.5f + mk3(0.5f); break;
    case MI_VIZ_SHEEN_COLOR: colour = mat.sheenColor; break;
    case MI_VIZ_SHEEN_ROUGHNESS: colour = mk3(mat.sheenRoughness); break;
    case MI_VIZ_SPECULAR_FACTOR: colour = mk3(mat.specular); break;
    case MI_VIZ_SPECULAR_COLOR: colour = mat.specularColor; break;
    case MI_VIZ_TRANSMISSION_FACTOR: colour = mk3(mat.transmission); break;
    case MI_VIZ_IRIDESCENCE_FACTOR: colour = mk3(mat.iridescence); break;
    case MI_VIZ_IRIDESCENCE_THICKNESS: colour = mk3(divExact(mat.iridescenceThickness, 1200.0f)); break;  // the Khronos viewer's fixed scale
    case MI_VIZ_ANISOTROPY_STRENGTH:
    {
      // the strength is folded into roughness.x (evaluateMaterial); recovered from the inflation: strength^2 = (rx - ry) / (1 - ry)
      const float den = fmaxf(1.0f - mat.roughness.y, 1e-5f);
      colour          = mk3(sqrtExact(fminf(fmaxf(divExact(mat.roughness.x - mat.roughness.y, den), 0.0f), 1.0f)));
      break;
    }
    case MI_VIZ_DIFFUSE_TRANSMISSION_FACTOR: colour = mk3(mat.diffuseTransmissionFactor); break;
    case MI_VIZ_DIFFUSE_TRANSMISSION_COLOR: colour = mat.diffuseTransmissionColor; break;
    case MI_VIZ_OPACITY_MICROMAP:
      if(ommState < 0)
        return VIZ_RENDERED;
      colour = ommState > 0 ? mk3(0.90f, 0.80f, 0.10f) : mk3(0.15f, 0.75f, 0.15f);
      break;
    default: return VIZ_RENDERED;  // MI_VIZ_RENDERED and values the reference does not know
  }
  return VIZ_COLOR_OVERRIDE;
}

}  // namespace pt
