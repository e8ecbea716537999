// Caller-supplied camera rays (camera_rays.hip; C-ABI: mi_pt_set_camera_rays / mi_pt_set_camera_rays_device, include/mi_pt.h): what is decided
// per path when a frame starts from a bound MiPtRay instead of the built-in camera -- which ray of the bound sets the path takes, whether the ray
// starts a path at all, its direction and the path's random stream.  Plain functions over pt_math.h: k_generate_rays runs them per lane,
// tests/host_shim/camera_rays_on_host.cpp compiles them for the CPU.
#pragma once
#include "mi_pt_shaderio.h"  // MI_SCENE_IS_ORTHOGRAPHIC
#include "pt_math.h"

namespace pt {

// The set a frame reads: frame f of a batch whose first frame is numbered frameCount is frame F = frameCount + f of the accumulation and takes
// set F % numSets.  frameCount >= 0 and f < 1024 (mi_pt_render_frames), so F fits 32 unsigned bits up to frameCount = 2^31 - 1.
PT_DEV uint32_t cameraRayFrame(int frameCount, uint32_t f) { return uint32_t(frameCount) + f; }
PT_DEV uint32_t cameraRaySet(uint32_t F, uint32_t numSets) { return F % numSets; }
// ... and the record inside it: image order, row-major
PT_DEV size_t cameraRayIndex(uint32_t set, int width, int height, int px, int py)
{
  return (size_t(set) * size_t(height) + size_t(py)) * size_t(width) + size_t(px);
}

// (an integer test: no floating-point option of the translation unit can fold it away)
PT_DEV bool cameraRayFinite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// A ray that starts no path: a non-finite origin or direction component, or a zero direction -- the queries' invalid-ray rule (pt_query.h:
// queryRayValid) without its tMin / tMax part, which camera paths do not read.  A denormal direction is a direction.
PT_DEV bool cameraRayDead(f3 o, f3 d)
{
  const bool finite  = cameraRayFinite(o.x) && cameraRayFinite(o.y) && cameraRayFinite(o.z) && cameraRayFinite(d.x) && cameraRayFinite(d.y) && cameraRayFinite(d.z);
  const bool nonZero = d.x != 0.0f || d.y != 0.0f || d.z != 0.0f;
  return !(finite && nonZero);
}
// The direction a path starts with.  unit (MI_PT_CAMERA_RAYS_UNIT): the caller's bits.  Otherwise normalised ONCE with normalizeExact; a direction
// whose squared length leaves the float range (below 1e-15 or above 1e15 in its largest component) is first scaled by a power of two, which changes
// no bit of the quotient, so that the denormal and the huge direction come out unit as well instead of non-finite.
PT_DEV f3 cameraRayDirection(f3 d, bool unit)
{
  if(unit)
    return d;
  const float m = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
  if(m < 1.0e-15f)
    d = d * 0x1p+100f;
  else if(m > 1.0e15f)
    d = d * 0x1p-100f;
  return normalizeExact(d);
}
// The random stream: sample 0 of frame F starts from the built-in camera's hash of (pixel, frame), a later sample from the seed the path before it
// left; either way the draws the built-in camera of the frame info spends before its first walk are discarded, so that the first draw of the first
// shade is the one a built-in path makes there.  cameraDraws: four -- two for the jitter, two for the lens -- and two under
// MI_SCENE_IS_ORTHOGRAPHIC, whose camera has no lens and makes no lens draws (cameraRayDraws).
PT_DEV int cameraRayDraws(int frameInfoFlags) { return (frameInfoFlags & MI_SCENE_IS_ORTHOGRAPHIC) ? 2 : 4; }
PT_DEV uint32_t cameraRaySeed(int px, int py, uint32_t F, int sampleIndex, uint32_t storedSeed, int cameraDraws)
{
  uint32_t seed = sampleIndex == 0 ? xxhash32(uint32_t(px), uint32_t(py), F) : storedSeed;
  (void)pcg(seed);
  (void)pcg(seed);
  if(cameraDraws > 2)
  {
    (void)pcg(seed);
    (void)pcg(seed);
  }
  return seed;
}

struct CameraRayPath
{
  bool     alive;  // false: a dead ray -- no path; the pixel takes radiance 0, alpha 0 for this frame
  uint32_t seed;   // RNG state of the path's first shade
  f3       origin, direction;
};
// a, b: the two 16-byte words of the MiPtRay (origin + tMin, direction + tMax; the bounds are not read: camera paths are unbounded)
PT_DEV CameraRayPath cameraRayPath(float4 a, float4 b, bool unit, int px, int py, uint32_t F, int sampleIndex, uint32_t storedSeed, int cameraDraws)
{
  CameraRayPath p;
  const f3      o = mk3(a.x, a.y, a.z), d = mk3(b.x, b.y, b.z);
  p.alive         = !cameraRayDead(o, d);
  p.seed          = cameraRaySeed(px, py, F, sampleIndex, storedSeed, cameraDraws);
  p.origin        = o;
  p.direction     = p.alive ? cameraRayDirection(d, unit) : mk3(0.0f);
  return p;
}

}  // namespace pt
