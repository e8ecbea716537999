// TEST INFRASTRUCTURE ONLY.  The per-path decision of caller-supplied camera rays (csrc/device/pt_camera_rays.h: which set a frame reads, dead or
// alive, the direction, the seed) compiled for the host through the stand-in <hip/hip_runtime.h> of this directory, so that
// tests/test_camera_rays_on_host.py can diff it against a numpy restatement on the CPU.  Built by the test session only.
#include <cmath>
#include <cstddef>
#include <hip/hip_runtime.h>

#include "pt_camera_rays.h"

using namespace pt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// n rays (8 floats each) at pixels pxy[2 i], pxy[2 i + 1] of frame F[i] -> alive[i], seed[i], origin + direction (6 floats)
EXPORT void dev_camera_ray_paths(int n, const float* rays, const int* pxy, const uint32_t* F, int unit, int sampleIndex, const uint32_t* storedSeed,
                                 int frameInfoFlags, int* alive, uint32_t* seed, float* out)
{
  for(int i = 0; i < n; ++i)
  {
    const float*        r = rays + 8 * size_t(i);
    const CameraRayPath p = cameraRayPath(make_float4(r[0], r[1], r[2], r[3]), make_float4(r[4], r[5], r[6], r[7]), unit != 0, pxy[2 * i], pxy[2 * i + 1],
                                          F[i], sampleIndex, storedSeed[i], cameraRayDraws(frameInfoFlags));
    alive[i] = p.alive ? 1 : 0;
    seed[i]  = p.seed;
    out[6 * i + 0] = p.origin.x, out[6 * i + 1] = p.origin.y, out[6 * i + 2] = p.origin.z;
    out[6 * i + 3] = p.direction.x, out[6 * i + 4] = p.direction.y, out[6 * i + 5] = p.direction.z;
  }
}

EXPORT uint32_t dev_camera_ray_set(int frameCount, uint32_t f, uint32_t numSets) { return cameraRaySet(cameraRayFrame(frameCount, f), numSets); }
EXPORT uint64_t dev_camera_ray_index(uint32_t set, int width, int height, int px, int py) { return uint64_t(cameraRayIndex(set, width, height, px, py)); }
