// Texture images of resident textures, updated in place (texture_update.hip; C-ABI: mi_pt_update_textures / mi_pt_update_textures_device).
// Two kernels over task tables, in the shape of k_vertex_ingest (pt_vertex_update.h): every texture's texel range is padded to whole
// 256-thread blocks, so a block serves one task and reads its record through the scalar cache.
//   ingest  level 0 of EVERY texture of a call in one launch: RGBA8 words are copied, RGBA32F texels quantised into the RGBA8 pool.
//   mip     one launch per level index, over that level of every texture of the call that generates its chain: the host loader's
//           downsample() (csrc/host/image_loader.cpp), byte for byte.  Level l reads the QUANTISED level l - 1, hence the launch per level.
// Byte for byte means: the same float32 operations in the same order, each rounded once.  Nothing here may be contracted into an fma (the
// host library is built for baseline x86-64, which has none): the arithmetic goes through tuMul / tuAdd / tuSub / tuDiv below, and
// texture_update.hip is compiled with -ffp-contract=off on top.  It matters for odd sizes only: for even ones tx = ty = 0.5 and every product is exact.
// Neither decode nor encode may depend on the device's powf: both go through tables the HOST makes (tuBuildTables) --
//   decode  256 floats of the sRGB EOTF (the loader's srgbToLinear), 256 floats i / 255.0f;
//   encode  sRGB: 255 thresholds, threshold k - 1 = the smallest float whose host encoding is >= k (found by bisection over the float's
//           bits; the host encoder is monotone over [0, 1]).  The code of v is the number of thresholds <= v: an 8-step search.
//           linear: round(clamp(v, 0, 1) * 255) half away from zero, as lround does (NOT rint, and not floor(x + 0.5): 0.49999997 + 0.5 = 1).
// The per-texel functions are plain functions over a memory policy `Mem` (ld / st of a typed element): the kernels pass
// address-space-qualified global accesses, tests/host_shim/texture_update_on_host.cpp plain ones, so the CPU tier runs the same text.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace pt {

constexpr int TEXTURE_UPDATE_BLOCK = 256;
// the tables, one array: [0, 256) sRGB decode, [256, 512) linear decode, [512, 767) encode thresholds, [767] = +inf (never read)
constexpr int TU_DECODE_SRGB = 0, TU_DECODE_LINEAR = 256, TU_ENCODE_SRGB = 512, TU_TABLE_FLOATS = 768;

enum : uint32_t
{
  TU_SRGB  = 1u,  // the texture's colour channels are sRGB-encoded (alpha never is)
  TU_FLOAT = 2u,  // (ingest) the source is RGBA32F, linear values
};

// Level 0 of one texture of an update call (block-uniform: loaded with scalar loads).
struct TextureIngestTask
{
  const void* src;  // the caller's level 0, device memory (the staging buffer for the host form): RGBA8 words, or float4 with TU_FLOAT
  uint32_t*   dst;  // the level's range of the pool
  uint32_t    texelCount, firstBlock, flags, _pad;
};

// One generated level of one texture: dst (dw x dh) from src (sw x sh), both ranges of the pool.
struct TextureMipTask
{
  const uint32_t* src;
  uint32_t*       dst;
  uint32_t        sw, sh, dw, dh, firstBlock, flags;
};

// ---- float32 operations that are rounded once each, whatever the contraction setting of the translation unit
__host__ __device__ inline float tuMul(float a, float b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a * b;
}
__host__ __device__ inline float tuAdd(float a, float b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a + b;
}
__host__ __device__ inline float tuSub(float a, float b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a - b;
}
__host__ __device__ inline float tuDiv(float a, float b)  // (IEEE division: the file is not compiled with the fast-division options)
{
  return a / b;
}

// ---- encode
// sRGB: the number of thresholds <= v.  thr[0 .. 254] ascending; v < 0 and NaN give 0, v > 1 gives 255 without a clamp.
__host__ __device__ inline uint32_t tuEncodeSrgb(const float* thr, float v)
{
  uint32_t pos = 0;
  for(uint32_t step = 128; step != 0; step >>= 1)  // (reads thr[pos + step - 1] <= thr[254])
    pos += thr[pos + step - 1] <= v ? step : 0u;
  return pos;
}

// linear: lround(clamp(v, 0, 1) * 255); NaN gives 0.  x - trunc(x) is exact, so the tie is seen exactly.
__host__ __device__ inline uint32_t tuEncodeLinear(float v)
{
  v = v > 0.0f ? v : 0.0f;  // (NaN: 0)
  v = v < 1.0f ? v : 1.0f;
  const float    x = tuMul(v, 255.0f);
  const uint32_t r = uint32_t(x);
  return r + (tuSub(x, float(r)) >= 0.5f ? 1u : 0u);
}

// One RGBA32F texel (linear values) as the pool's RGBA8 word.
__host__ __device__ inline uint32_t tuQuantise(const float* tables, float4 v, bool srgb)
{
  const float*   thr = tables + TU_ENCODE_SRGB;
  const uint32_t r = srgb ? tuEncodeSrgb(thr, v.x) : tuEncodeLinear(v.x);
  const uint32_t g = srgb ? tuEncodeSrgb(thr, v.y) : tuEncodeLinear(v.y);
  const uint32_t b = srgb ? tuEncodeSrgb(thr, v.z) : tuEncodeLinear(v.z);
  return r | (g << 8) | (b << 16) | (tuEncodeLinear(v.w) << 24);
}

// ---- the mip filter: destination texel (x, y) of a task, as downsample() computes it
struct TuAxis  // the two source texels of one axis and the weight of the second
{
  uint32_t i0, i1;
  float    t;
};
__host__ __device__ inline TuAxis tuAxis(uint32_t x, uint32_t s, uint32_t d)
{
  // destination texel centre in source texel space: (x + 0.5f) * float(s) / float(d) - 0.5f
  const float f  = tuSub(tuDiv(tuMul(tuAdd(float(int(x)), 0.5f), float(int(s))), float(int(d))), 0.5f);
  const int   i0 = int(floorf(f));
  TuAxis      a;
  a.t  = tuSub(f, float(i0));
  a.i1 = uint32_t(i0 + 1 < int(s) - 1 ? i0 + 1 : int(s) - 1);
  a.i0 = uint32_t(i0 > 0 ? i0 : 0);
  return a;
}

// (a (1 - tx) + b tx) (1 - ty) + (c (1 - tx) + d tx) ty, in that order
__host__ __device__ inline float tuBlend(float a, float b, float c, float d, float tx, float ty)
{
  const float ux = tuSub(1.0f, tx), uy = tuSub(1.0f, ty);
  const float top = tuAdd(tuMul(a, ux), tuMul(b, tx));
  const float bot = tuAdd(tuMul(c, ux), tuMul(d, tx));
  return tuAdd(tuMul(top, uy), tuMul(bot, ty));
}

template <class Mem>
__host__ __device__ inline uint32_t mipTexel(const TextureMipTask& T, const float* tables, uint32_t x, uint32_t y)
{
  const TuAxis   ax = tuAxis(x, T.sw, T.dw), ay = tuAxis(y, T.sh, T.dh);
  const uint32_t p00 = Mem::ld(T.src, size_t(ay.i0) * T.sw + ax.i0), p10 = Mem::ld(T.src, size_t(ay.i0) * T.sw + ax.i1);
  const uint32_t p01 = Mem::ld(T.src, size_t(ay.i1) * T.sw + ax.i0), p11 = Mem::ld(T.src, size_t(ay.i1) * T.sw + ax.i1);
  const bool     srgb = (T.flags & TU_SRGB) != 0;
  uint32_t       out  = 0;
  for(uint32_t c = 0; c < 4; ++c)
  {
    const bool   decode = srgb && c < 3;
    const float* lut    = tables + (decode ? TU_DECODE_SRGB : TU_DECODE_LINEAR);
    const uint32_t sh   = 8u * c;
    const float  v = tuBlend(lut[(p00 >> sh) & 0xffu], lut[(p10 >> sh) & 0xffu], lut[(p01 >> sh) & 0xffu], lut[(p11 >> sh) & 0xffu], ax.t, ay.t);
    out |= (decode ? tuEncodeSrgb(tables + TU_ENCODE_SRGB, v) : tuEncodeLinear(v)) << sh;
  }
  return out;
}

// ---- the tables (host functions).  `encode` is the host's linear-to-sRGB8 encoder.
// The loader's transfer functions (csrc/host/image_loader.cpp: srgbToLinear, linearToSrgb8), restated: libmi_pt.so does not link the loader.
inline float tuHostSrgbToLinear(int i)
{
  const float c = float(i) / 255.0f;
  return c <= 0.04045f ? c / 12.92f : std::pow((c + 0.055f) / 1.055f, 2.4f);
}
inline uint8_t tuHostLinearToSrgb8(float c)
{
  c             = c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f;
  const float s = c <= 0.0031308f ? c * 12.92f : 1.055f * std::pow(c, 1.0f / 2.4f) - 0.055f;
  return uint8_t(std::lround(s * 255.0f));
}
template <class Encode>
inline void tuBuildTables(float* tables, Encode encode)
{
  for(int i = 0; i < 256; ++i)
  {
    tables[TU_DECODE_SRGB + i]   = tuHostSrgbToLinear(i);
    tables[TU_DECODE_LINEAR + i] = float(i) / 255.0f;
  }
  for(uint32_t k = 1; k < 256; ++k)
  {
    uint32_t lo = 0u, hi = 0x3f800000u;  // bits of 0.0f (code 0 < k) and of 1.0f (code 255 >= k); positive floats order like their bits
    while(hi - lo > 1u)
    {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if(uint32_t(encode(__builtin_bit_cast(float, mid))) >= k)
        hi = mid;
      else
        lo = mid;
    }
    tables[TU_ENCODE_SRGB + k - 1] = __builtin_bit_cast(float, hi);
  }
  tables[TU_TABLE_FLOATS - 1] = __builtin_bit_cast(float, 0x7f800000u);
}

#if defined(__HIPCC__)
// tasks / blockTask: device arrays (blockTask[b] = the task of block b); numBlocks = sum of ceil(texels / TEXTURE_UPDATE_BLOCK).
// tables: TU_TABLE_FLOATS floats in device memory.
void launchTextureIngest(const TextureIngestTask* tasks, const uint32_t* blockTask, uint32_t numBlocks, const float* tables, hipStream_t stream);
void launchTextureMips(const TextureMipTask* tasks, const uint32_t* blockTask, uint32_t numBlocks, const float* tables, hipStream_t stream);
#endif

}  // namespace pt
