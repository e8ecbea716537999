// The HDR environment updated in place (env_update.hip; C-ABI: mi_pt_update_environment / mi_pt_update_environment_device): caller-supplied
// lat-long RGB(A)32F texels become the resident RGBA32F map with the sampling pdf in alpha, and its alias table is built on the device.
// The formulas are the host's (HdrEnvironment::buildAccel, csrc/host/gltf_scene.cpp): importance_i = float(area_row * double(max(r, g, b))),
// total = the double sum of the importances, alpha = max(r, g, b) * float(1 / total); the row areas come from the HOST (no device trig).
// The table is NOT built by Vose's sequential loop but by a prefix-sum construction, all of it in double, only the final q rounded to float
// (buildAccel's comment on float32 drift applies here too):
//   q_i = double(importance_i) * (n / total); texel i is LIGHT if q_i < 1, HEAVY otherwise; both classes are compacted in texel order;
//   Dx(a), a = 0 .. nL: the exclusive prefix of 1 - q over the lights (Dx(nL) = the whole deficit);
//   E(b),  b = 0 .. nH - 1: the inclusive prefix of q - 1 over the heavies;
//   light a: alias = heavy b, the smallest b with E(b) >= Dx(a), q = q_a (no such b -- through rounding only --: q = 1, alias = itself);
//   heavy b: c = #{a < nL : Dx(a) <= E(b)}, r = 1 + (E(b) - Dx(c)); r < 1 and heavy b + 1 exists: q = clamp(r, 0, 1), alias = heavy b + 1;
//            otherwise q = 1, alias = itself.
// (Lights with Dx(a) <= E(b) alias to heavies <= b, so heavies 0 .. b have received Dx(c) and could give E(b): r is what heavy b has left.)
//
// THE SUMMATION ORDER -- every floating sum below runs in this one order, whatever the scheduling; no floating atomics, no look-back:
//   thread  a thread owns ENV_ITEMS = 4 consecutive elements and adds them left to right: ((v0 + v1) + v2) + v3;
//   block   the ENV_BLOCK = 256 thread sums of a tile (ENV_TILE = 1024 elements) go through euBlockScan, a Hillis-Steele inclusive scan:
//           8 steps o = 1, 2, .. 128, in each x[t] = x[t - o] + x[t] (left operand first) for t >= o.  The tile's sum is x[255];
//   tiles   ONE block scans the tile sums (euTileScan): chunks of 256 in ascending order, euBlockScan inside a chunk, and a running carry:
//           exclusive[t] = carry + x[t - 1] (x[-1] = 0: carry itself), then carry = carry + x[255].  It loops: 2^26 texels are 65536 tile sums;
//   element exclusive prefix of element k of thread t of a tile = tileBase + (x[t - 1] + (v0 + .. + v(k-1))), the inner sum left to right.
// The passes (env_update.hip has one kernel each; tests/host_shim/env_update_on_host.cpp runs the same functions block by block):
//   euIngest    sanitise, write rgb, tile sums of the importance             euTotal    total, n / total, float(1 / total)
//   euClassify  alpha; per tile: light count, deficit sum, excess sum        euTileScan their exclusive scans over the tiles
//   euCompact   index lists and the two prefix arrays                        euAlias    the two batched binary searches, the table
// A map with total <= 0 gets the uniform table (q = 1, alias = i, alpha = float(1 / (4 pi)), integral 0) from euClassify; the later passes return.
// Everything between two barriers is a `phase` of a block policy: the kernels run it for threadIdx.x and __syncthreads(), the host shim for
// t = 0 .. 255 in turn.  State that outlives a phase lives in the block's shared arrays or in global memory, never in a thread's registers.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "mi_pt_shaderio.h"

namespace pt {

constexpr uint32_t ENV_BLOCK = 256, ENV_ITEMS = 4, ENV_TILE = ENV_BLOCK * ENV_ITEMS;
constexpr uint32_t ENV_MAX_TEXELS = 1u << 26;

// Device memory, written by the passes, read back by the call.
struct EnvHeader
{
  double   total;         // the sum of the importances
  double   scale;         // n / total
  double   totalDeficit;  // the sum of 1 - q over the lights
  float    invTotal;      // float(1 / total)
  uint32_t numLight;
  uint32_t sanitised;     // texels with a component replaced by 0 (integer atomic)
  uint32_t _pad;
};

// What the tile scans carry: deficit and excess sums and the light count.
struct EnvTriple
{
  double   d, e;
  uint32_t c, _pad;
};

struct EnvArgs
{
  uint32_t     n, width, channels, numTiles;
  const float* src;       // the caller's texels, `channels` floats each (may be `pixels` itself: every texel is read before it is written)
  float4*      pixels;    // the resident map
  MiEnvAccel*  accel;     // the resident table
  const double* rowArea;  // `height` doubles
  EnvHeader*   header;
  double*      tileImp;   // numTiles importance sums
  EnvTriple*   tiles;     // numTiles; sums after euClassify, exclusive scans after euTileScan
  double*      prefix;    // n + 1: Dx(0 .. nL), then E(0 .. nH - 1)
  uint32_t*    index;     // n: the lights in texel order, then the heavies
  float        uniformPdf;  // float(1 / (4 pi)), made by the host
};

// The shared arrays of a block (LDS in the kernels).
struct EnvShared
{
  double    a[ENV_BLOCK], b[ENV_BLOCK];
  EnvTriple ta[ENV_BLOCK], tb[ENV_BLOCK];
  double    carry;
  EnvTriple tcarry;
};

__host__ __device__ inline double    euAdd(double x, double y) { return x + y; }
__host__ __device__ inline EnvTriple euAdd(const EnvTriple& x, const EnvTriple& y) { return EnvTriple{x.d + y.d, x.e + y.e, x.c + y.c, 0u}; }

// Inclusive scan of x[0 .. 255]; y is the other half of the ping-pong.  8 steps, an even number: the result is in x.
template <class Block, class T>
__host__ __device__ inline void euBlockScan(Block& blk, T* x, T* y)
{
  for(uint32_t o = 1; o < ENV_BLOCK; o <<= 1)
  {
    blk.phase([&](uint32_t t) { y[t] = t >= o ? euAdd(x[t - o], x[t]) : x[t]; });
    T* s = x;
    x    = y;
    y    = s;
  }
}

// A caller's component as it becomes resident: a non-finite or negative one is 0 (NaN fails the first comparison; -0.0f stays).
__host__ __device__ inline float euSanitise(float v, bool& replaced)
{
  const bool ok = v >= 0.0f && v <= FLT_MAX;
  replaced      = replaced || !ok;
  return ok ? v : 0.0f;
}

__host__ __device__ inline float euMax3(float r, float g, float b)
{
  const float gb = g < b ? b : g;  // std::max(g, b)
  return r < gb ? gb : r;          // std::max(r, .)
}

__host__ __device__ inline float euImportance(const EnvArgs& A, uint32_t i, float m)
{
  return float(A.rowArea[i / A.width] * double(m));
}

// q of resident texel i (not yet rounded): recomputed by every pass that needs it, from the same operands by the same operations.
__host__ __device__ inline double euQ(const EnvArgs& A, uint32_t i, double scale)
{
  const float4 p = A.pixels[i];
  return double(euImportance(A, i, euMax3(p.x, p.y, p.z))) * scale;
}

// ---- pass 1: the caller's texels into the resident map, and the tile sums of the importance
template <class Block>
__host__ __device__ inline void euIngest(Block& blk, EnvShared& S, const EnvArgs& A, uint32_t tile)
{
  blk.phase([&](uint32_t t) {
    double   sum       = 0.0;
    uint32_t sanitised = 0;
    for(uint32_t k = 0; k < ENV_ITEMS; ++k)
    {
      const uint32_t i = tile * ENV_TILE + t * ENV_ITEMS + k;
      if(i >= A.n)
        break;
      const float* s        = A.src + size_t(i) * A.channels;
      bool         replaced = false;
      const float  r = euSanitise(s[0], replaced), g = euSanitise(s[1], replaced), b = euSanitise(s[2], replaced);
      A.pixels[i] = make_float4(r, g, b, 0.0f);
      sanitised += replaced ? 1u : 0u;
      sum = sum + double(euImportance(A, i, euMax3(r, g, b)));
    }
    S.a[t] = sum;
    if(sanitised)
      blk.atomicAdd(&A.header->sanitised, sanitised);
  });
  euBlockScan(blk, S.a, S.b);
  blk.phase([&](uint32_t t) {
    if(t == 0)
      A.tileImp[tile] = S.a[ENV_BLOCK - 1];
  });
}

// ---- pass 2 (one block): the total of the tile sums and what is derived from it
template <class Block>
__host__ __device__ inline void euTotal(Block& blk, EnvShared& S, const EnvArgs& A)
{
  blk.phase([&](uint32_t t) {
    if(t == 0)
      S.carry = 0.0;
  });
  for(uint32_t first = 0; first < A.numTiles; first += ENV_BLOCK)
  {
    blk.phase([&](uint32_t t) { S.a[t] = first + t < A.numTiles ? A.tileImp[first + t] : 0.0; });
    euBlockScan(blk, S.a, S.b);
    blk.phase([&](uint32_t t) {
      if(t == 0)
        S.carry = S.carry + S.a[ENV_BLOCK - 1];
    });
  }
  blk.phase([&](uint32_t t) {
    if(t != 0)
      return;
    const double total = S.carry;
    A.header->total    = total;
    A.header->scale    = total > 0.0 ? double(A.n) / total : 0.0;
    A.header->invTotal = total > 0.0 ? float(1.0 / total) : 0.0f;
  });
}

// What one thread's elements add to the tile: the same for euClassify (tile sums) and euCompact (prefixes).
__host__ __device__ inline EnvTriple euThreadSums(const EnvArgs& A, uint32_t tile, uint32_t t, double scale)
{
  EnvTriple s{0.0, 0.0, 0u, 0u};
  for(uint32_t k = 0; k < ENV_ITEMS; ++k)
  {
    const uint32_t i = tile * ENV_TILE + t * ENV_ITEMS + k;
    if(i >= A.n)
      break;
    const double q = euQ(A, i, scale);
    if(q < 1.0)
    {
      s.d = s.d + (1.0 - q);
      s.c += 1u;
    }
    else
      s.e = s.e + (q - 1.0);
  }
  return s;
}

// ---- pass 3: alpha, and the tile's light count, deficit and excess -- or, for a map without light, the uniform table
template <class Block>
__host__ __device__ inline void euClassify(Block& blk, EnvShared& S, const EnvArgs& A, uint32_t tile)
{
  const double total = A.header->total;
  if(!(total > 0.0))  // (uniform over the grid)
  {
    blk.phase([&](uint32_t t) {
      for(uint32_t k = 0; k < ENV_ITEMS; ++k)
      {
        const uint32_t i = tile * ENV_TILE + t * ENV_ITEMS + k;
        if(i >= A.n)
          break;
        float4 p    = A.pixels[i];
        p.w         = A.uniformPdf;
        A.pixels[i] = p;
        A.accel[i]  = MiEnvAccel{i, 1.0f};
      }
    });
    return;
  }
  const double scale    = A.header->scale;
  const float  invTotal = A.header->invTotal;
  blk.phase([&](uint32_t t) {
    for(uint32_t k = 0; k < ENV_ITEMS; ++k)
    {
      const uint32_t i = tile * ENV_TILE + t * ENV_ITEMS + k;
      if(i >= A.n)
        break;
      float4 p    = A.pixels[i];
      p.w         = euMax3(p.x, p.y, p.z) * invTotal;
      A.pixels[i] = p;
    }
    S.ta[t] = euThreadSums(A, tile, t, scale);
  });
  euBlockScan(blk, S.ta, S.tb);
  blk.phase([&](uint32_t t) {
    if(t == 0)
      A.tiles[tile] = S.ta[ENV_BLOCK - 1];
  });
}

// ---- pass 4 (one block): the tile sums become exclusive scans over the tiles; the totals go to the header and to Dx(nL)
template <class Block>
__host__ __device__ inline void euTileScan(Block& blk, EnvShared& S, const EnvArgs& A)
{
  if(!(A.header->total > 0.0))
    return;
  blk.phase([&](uint32_t t) {
    if(t == 0)
      S.tcarry = EnvTriple{0.0, 0.0, 0u, 0u};
  });
  for(uint32_t first = 0; first < A.numTiles; first += ENV_BLOCK)
  {
    blk.phase([&](uint32_t t) { S.ta[t] = first + t < A.numTiles ? A.tiles[first + t] : EnvTriple{0.0, 0.0, 0u, 0u}; });
    euBlockScan(blk, S.ta, S.tb);
    blk.phase([&](uint32_t t) {
      if(first + t < A.numTiles)
        A.tiles[first + t] = t ? euAdd(S.tcarry, S.ta[t - 1]) : S.tcarry;
    });
    blk.phase([&](uint32_t t) {
      if(t == 0)
        S.tcarry = euAdd(S.tcarry, S.ta[ENV_BLOCK - 1]);
    });
  }
  blk.phase([&](uint32_t t) {
    if(t != 0)
      return;
    A.header->numLight        = S.tcarry.c;
    A.header->totalDeficit    = S.tcarry.d;
    A.prefix[S.tcarry.c]      = S.tcarry.d;  // Dx(nL)
  });
}

// ---- pass 5: the compacted index lists and the prefix arrays
template <class Block>
__host__ __device__ inline void euCompact(Block& blk, EnvShared& S, const EnvArgs& A, uint32_t tile)
{
  if(!(A.header->total > 0.0))
    return;
  const double   scale    = A.header->scale;
  const uint32_t numLight = A.header->numLight;
  blk.phase([&](uint32_t t) { S.ta[t] = euThreadSums(A, tile, t, scale); });
  euBlockScan(blk, S.ta, S.tb);
  blk.phase([&](uint32_t t) {
    const EnvTriple base   = A.tiles[tile];
    const EnvTriple before = t ? S.ta[t - 1] : EnvTriple{0.0, 0.0, 0u, 0u};
    double          d = 0.0, e = 0.0;  // the thread's running sums, left to right
    uint32_t        c = 0;
    for(uint32_t k = 0; k < ENV_ITEMS; ++k)
    {
      const uint32_t i = tile * ENV_TILE + t * ENV_ITEMS + k;
      if(i >= A.n)
        break;
      const double q = euQ(A, i, scale);
      if(q < 1.0)
      {
        const uint32_t a = base.c + before.c + c;
        A.index[a]       = i;
        A.prefix[a]      = base.d + (before.d + d);  // exclusive
        d                = d + (1.0 - q);
        c += 1u;
      }
      else
      {
        // heavies before this one: the elements before it that are not light
        const uint32_t h = (tile * ENV_TILE - base.c) + (t * ENV_ITEMS + k - before.c - c);
        e                = e + (q - 1.0);
        A.index[numLight + h]       = i;
        A.prefix[numLight + 1u + h] = base.e + (before.e + e);  // inclusive
      }
    }
  });
}

// ---- pass 6: slot k of the index list writes its texel's entry
__host__ __device__ inline void euAlias(const EnvArgs& A, uint32_t k)
{
  if(k >= A.n || !(A.header->total > 0.0))
    return;
  const double   scale = A.header->scale;
  const uint32_t nL = A.header->numLight, nH = A.n - nL;
  const double*  Dx = A.prefix;
  const double*  E  = A.prefix + nL + 1u;
  const uint32_t i  = A.index[k];
  if(i >= A.n)  // (euCompact wrote every slot with a texel index; nothing else is ever written through)
    return;
  MiEnvAccel     out{i, 1.0f};
  if(k < nL)
  {
    const double x  = Dx[k];
    uint32_t     lo = 0, hi = nH;  // the smallest b with E(b) >= x
    while(lo < hi)
    {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if(E[mid] >= x)
        hi = mid;
      else
        lo = mid + 1u;
    }
    if(lo < nH)
      out = MiEnvAccel{A.index[nL + lo], float(euQ(A, i, scale))};
  }
  else
  {
    const uint32_t b  = k - nL;
    const double   x  = E[b];
    uint32_t       lo = 0, hi = nL;  // the number of a < nL with Dx(a) <= x
    while(lo < hi)
    {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if(Dx[mid] <= x)
        lo = mid + 1u;
      else
        hi = mid;
    }
    const double r = 1.0 + (x - Dx[lo]);
    if(r < 1.0 && b + 1u < nH)
      out = MiEnvAccel{A.index[k + 1u], float(r > 0.0 ? r : 0.0)};
  }
  A.accel[i] = out;
}

// ---- host side of a call
// The solid angle of a texel of row y, buildAccel's expression.
inline void euRowAreas(int width, int height, double* area)
{
  const double stepPhi   = 2.0 * M_PI / double(width);
  const double stepTheta = M_PI / double(height);
  for(int y = 0; y < height; ++y)
  {
    const double theta0 = double(y) * stepTheta;
    area[y]             = (std::cos(theta0) - std::cos(theta0 + stepTheta)) * stepPhi;
  }
}
inline float euUniformPdf()
{
  return float(1.0 / (4.0 * M_PI));
}
inline uint32_t euNumTiles(uint32_t n)
{
  return (n + ENV_TILE - 1u) / ENV_TILE;
}

// The scratch of a call, one allocation: offsets in bytes, 16-byte aligned.  The host form stages RGB32F texels at `prefix`: 12 n bytes fit into
// the prefix and index arrays, which the passes write only after euIngest has read the staged texels.
struct EnvScratchLayout
{
  size_t header, rowArea, tileImp, tiles, prefix, index, bytes;
};
inline EnvScratchLayout euScratchLayout(uint32_t n, uint32_t height)
{
  auto             up = [](size_t v) { return (v + 15u) & ~size_t(15); };
  const size_t     T  = euNumTiles(n);
  EnvScratchLayout L{};
  L.header  = 0;
  L.rowArea = up(sizeof(EnvHeader));
  L.tileImp = L.rowArea + up(size_t(height) * sizeof(double));
  L.tiles   = L.tileImp + up(T * sizeof(double));
  L.prefix  = L.tiles + up(T * sizeof(EnvTriple));
  L.index   = L.prefix + up((size_t(n) + 1u) * sizeof(double));
  L.bytes   = L.index + up(size_t(n) * sizeof(uint32_t));
  return L;
}

#if defined(__HIPCC__)
// The six launches of a call on `stream`; `sync`, when set, is called after each with the pass's name (diagnostic timing).
void launchEnvUpdate(const EnvArgs& args, hipStream_t stream, void (*sync)(const char* pass, void* user), void* user);
constexpr int ENV_UPDATE_LAUNCHES = 6;
#endif

}  // namespace pt
