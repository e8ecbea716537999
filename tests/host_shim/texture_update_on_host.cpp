// TEST INFRASTRUCTURE ONLY.  The per-texel functions of texture image updates (csrc/device/pt_texture_update.h: mipTexel, tuQuantise, tuEncodeSrgb,
// tuEncodeLinear, and the host's table builder) compiled for the host through the stand-in <hip/hip_runtime.h> of this directory, with g++
// -ffp-contract=off and plain memory accesses where the kernels use address-space-qualified ones, so that tests/test_texture_update_on_host.py
// can diff the chain they make against the host loader's (mi_build_mip_chain) on the CPU.  Built by the test session only.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pt_texture_update.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

namespace {
struct PlainMem
{
  template <class T>
  static T ld(const T* p, size_t i)
  {
    return p[i];
  }
  template <class T>
  static void st(T* p, size_t i, T v)
  {
    p[i] = v;
  }
};
}  // namespace

// The tables as mi_pt_update_textures makes them (TU_TABLE_FLOATS floats).  encode: the encoder the thresholds are bisected from, or NULL for
// the restatement libmi_pt.so uses (tuHostLinearToSrgb8).
EXPORT void dev_texture_tables(float* tables, uint8_t (*encode)(float))
{
  if(encode)
    tuBuildTables(tables, encode);
  else
    tuBuildTables(tables, tuHostLinearToSrgb8);
}

// What the launches of k_texture_mips do for one texture: levels 1 .. numLevels - 1 from level 0, packed one after the other into `out`.
EXPORT void dev_texture_mip_chain(const float* tables, int width, int height, int numLevels, int srgb, const uint32_t* level0, uint32_t* out)
{
  std::vector<uint32_t> src(level0, level0 + size_t(width) * size_t(height));
  for(int l = 1; l < numLevels; ++l)
  {
    TextureMipTask T{};
    T.sw    = uint32_t(std::max(1, width >> (l - 1)));
    T.sh    = uint32_t(std::max(1, height >> (l - 1)));
    T.dw    = uint32_t(std::max(1, width >> l));
    T.dh    = uint32_t(std::max(1, height >> l));
    T.src   = src.data();
    T.dst   = out;
    T.flags = srgb ? TU_SRGB : 0u;
    for(uint32_t i = 0; i < T.dw * T.dh; ++i)  // (the kernel's thread i)
      PlainMem::st(T.dst, i, mipTexel<PlainMem>(T, tables, i % T.dw, i / T.dw));
    src.assign(out, out + size_t(T.dw) * T.dh);
    out += size_t(T.dw) * T.dh;
  }
}

// What k_texture_ingest does with RGBA32F texels.
EXPORT void dev_texture_quantise(const float* tables, const float* rgba, uint32_t texels, int srgb, uint32_t* out)
{
  for(uint32_t i = 0; i < texels; ++i)
    out[i] = tuQuantise(tables, float4{rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]}, srgb != 0);
}

EXPORT void dev_encode_srgb(const float* tables, const float* values, uint64_t count, uint8_t* out)
{
  for(uint64_t i = 0; i < count; ++i)
    out[i] = uint8_t(tuEncodeSrgb(tables + TU_ENCODE_SRGB, values[i]));
}

EXPORT void dev_encode_linear(const float* values, uint64_t count, uint8_t* out)
{
  for(uint64_t i = 0; i < count; ++i)
    out[i] = uint8_t(tuEncodeLinear(values[i]));
}

// lround(clamp(v, 0, 1) * 255) as the loader writes it (image_loader.cpp, downsample: the linear channels), for the rounding test.
EXPORT void host_encode_linear(const float* values, uint64_t count, uint8_t* out)
{
  for(uint64_t i = 0; i < count; ++i)
    out[i] = uint8_t(std::lround(std::min(std::max(values[i], 0.0f), 1.0f) * 255.0f));
}
