// TEST INFRASTRUCTURE ONLY.  The texture fetch and the material evaluation of the shade kernels (csrc/device/pt_shading.h: getTextureRef, the
// core-slot path coreTexPlan -> coreTexIssue -> coreTexFinish, evaluateMaterial) compiled for the host through the stand-in <hip/hip_runtime.h> of
// this directory, over tables the test passes in, so that tests/test_texture_on_host.py can diff them against the float64 reference of
// tests/texture_ref.py on the CPU.  Built by the test session only; never loaded by the product.
#include <cstddef>
#include <cstring>

#include "pt_shading.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// The tables of a fetch: texel pool (RGBA8 words), footprint records (or NULL: the four-gather path), DevTexRef[], the 256-entry sRGB table
struct ShimTexTables
{
  const uint32_t*  texels;
  const uint32_t*  quads;
  const DevTexRef* refs;
  const float*     lut;
};
static TexCtx ctxOf(const ShimTexTables* t)
{
  return TexCtx{t->refs, reinterpret_cast<const uchar4*>(t->texels), t->lut, reinterpret_cast<const uint4*>(t->quads)};
}

EXPORT int dev_tex_sizes(int* sizes)
{
  sizes[0] = int(sizeof(DevTexRef));
  sizes[1] = int(sizeof(DevCoreTex));
  sizes[2] = int(sizeof(MiGltfShadeMaterial));
  sizes[3] = int(sizeof(MiGltfTextureInfo));
  return 4;
}

// n fetches of texture-info slot `slot[i]` at tc[i] = {tc0.xy, tc1.xy} with footprint texGrad[i]: out[4 i ..] = rgba
EXPORT void dev_get_texture(const ShimTexTables* t, int n, const uint32_t* slot, const float* tc, const float* texGrad, float* out)
{
  const TexCtx ctx = ctxOf(t);
  for(int i = 0; i < n; ++i)
  {
    const f4 r = getTextureRef(ctx, slot[i], mk2(tc[4 * i], tc[4 * i + 1]), mk2(tc[4 * i + 2], tc[4 * i + 3]), texGrad[i]);
    out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
  }
}

// the same through a core record (DevCoreTex as four words; core[4 i ..]): plan, issue, finish.  path[i]: the plan's CP_* bits
EXPORT void dev_core_texture(const ShimTexTables* t, int n, const uint32_t* core, const uint32_t* slot, const float* tc, const float* texGrad, float* out,
                             uint32_t* path)
{
  const TexCtx ctx = ctxOf(t);
  for(int i = 0; i < n; ++i)
  {
    const f2      tc0 = mk2(tc[4 * i], tc[4 * i + 1]), tc1 = mk2(tc[4 * i + 2], tc[4 * i + 3]);
    const uint4   c   = make_uint4(core[4 * i], core[4 * i + 1], core[4 * i + 2], core[4 * i + 3]);
    const CoreTap p   = coreTexPlan(ctx, c, tc0, tc1, texGrad[i]);
    uint4         q0, q1;
    coreTexIssue(ctx, p, q0, q1);
    const f4 r = coreTexFinish(ctx, p, q0, q1, slot[i], tc0, tc1, texGrad[i]);
    out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
    path[i]    = p.bits;
  }
}

// PbrMaterial is plain floats: the offsets (in floats) of the fields the test reads, in this order; returns the size in floats
EXPORT int dev_tex_material_layout(int* offsets)
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

// evaluateMaterial<SIMPLE = false, CORE = core> of material `m` (its five core records at core5, as on the device: coreTex[5 * materialID]):
// in[] = tc0.xy tc1.xy texGrad vertexColour.rgba T.xyz B.xyz N.xyz (18 floats); out: the PbrMaterial as floats.  Returns the texture taps.
EXPORT int dev_evaluate_material(const ShimTexTables* t, const MiGltfShadeMaterial* m, const uint32_t* core5, int core, const float* in, float* out)
{
  DevScene sc;
  std::memset(&sc, 0, sizeof(sc));
  MeshState st;
  st.tc0 = mk2(in[0], in[1]);
  st.tc1 = mk2(in[2], in[3]);
  st.texGrad            = in[4];
  st.baseColorVertexMul = mk4(in[5], in[6], in[7], in[8]);
  st.T = mk3(in + 9); st.B = mk3(in + 12); st.N = mk3(in + 15); st.Ng = st.N;
  st.isInside = false;
  st.tex      = ctxOf(t);
  st.core0    = make_uint4(core5[0], core5[1], core5[2], core5[3]);
  unsigned          taps = 0;
  const PbrMaterial p    = core ? evaluateMaterial<false, true>(sc, *m, st, taps) : evaluateMaterial<false, false>(sc, *m, st, taps);
  std::memcpy(out, &p, sizeof(p));
  return int(taps);
}
