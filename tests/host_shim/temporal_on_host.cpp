// TEST INFRASTRUCTURE ONLY.  The per-pixel arithmetic of the motion vectors and of the temporal reprojection (csrc/device/pt_temporal.h:
// motionRecord, reprojectPixel) compiled for the host through the stand-in <hip/hip_runtime.h> of this directory, so that
// tests/test_temporal_on_host.py can diff it against a float64 numpy restatement on the CPU.  Built by the test session only.
#include <cmath>
#include <cstddef>

#include "pt_temporal.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// n first-hit records -> n motion records; nodes: numNodes MiGltfRenderNode, prevObjectToWorld: 16 floats per node
EXPORT void dev_motion_records(int n, const float* firstHit, const void* nodes, const float* prevObjectToWorld, int numNodes, const float* viewProj,
                               const float* prevMVP, float width, float height, float* out)
{
  for(int i = 0; i < n; ++i)
  {
    const float4 r = motionRecord(make_float4(firstHit[4 * i], firstHit[4 * i + 1], firstHit[4 * i + 2], firstHit[4 * i + 3]),
                                  static_cast<const MiGltfRenderNode*>(nodes), prevObjectToWorld, numNodes, viewProj, prevMVP, width, height);
    out[4 * i] = r.x, out[4 * i + 1] = r.y, out[4 * i + 2] = r.z, out[4 * i + 3] = r.w;
  }
}

// one temporal stage over a W x H image.  consts: alpha, momentsAlpha, maxHistory, normalCos, depthTolerance; histIn / histOut: illum, moments,
// normal images (float4 per pixel); illum: the prepared (illumination, variance) image; taps: valid taps per pixel (0 = reset)
EXPORT void dev_reproject_image(int W, int H, const float* consts, int haveHistory, const float* color, const float* albedo, const float* normal,
                                const float* depth, const float* motion, float* const* histIn, float* const* histOut, float* illum, int* taps)
{
  const TemporalConsts  tc{consts[0], consts[1], consts[2], consts[3], consts[4]};
  auto                  f4p = [](const float* p) { return reinterpret_cast<float4*>(const_cast<float*>(p)); };
  const TemporalHistory in{f4p(histIn[0]), f4p(histIn[1]), f4p(histIn[2])}, out{f4p(histOut[0]), f4p(histOut[1]), f4p(histOut[2])};
  for(int y = 0; y < H; ++y)
    for(int x = 0; x < W; ++x)
      f4p(illum)[size_t(y) * W + x] =
          reprojectPixel(x, y, W, H, tc, haveHistory != 0, f4p(color), f4p(albedo), f4p(normal), depth, f4p(motion), in, out, &taps[size_t(y) * W + x]);
}

EXPORT int dev_pixel_of_slot(const uint32_t* ownedTiles, int tileShift, int width, int height, uint32_t slot, int* px, int* py)
{
  return pixelOfSlot(ownedTiles, tileShift, width, height, slot, *px, *py) ? 1 : 0;
}
