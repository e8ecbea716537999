// The camera ray of a pixel position, shared by the path-trace kernels (pt_kernels.hip), the pick kernel (query.hip) and the export of the
// built-in camera's rays (camera_rays.hip): all must form the same ray bit for bit whatever their translation unit's floating-point options,
// so everything inexact in it goes through divExact / normalizeExact (pt_math.h).  Below getRay: the slot <-> pixel map and the start of a
// camera path (generateCameraPath), which k_generate / k_trace_primary (pt_kernels.hip) and k_export_camera_rays (camera_rays.hip) share.
#pragma once
#include "pt_scene.h"
#include "pt_shading.h"

namespace pt {

// ---- camera (pathtrace_functions.h.slang:784-811, gltf_pathtrace.slang:502-529) ------------------------------------------
PT_DEV void getRay(const FrameConsts& fc, f2 samplePos, f2 offset, f3& origin, f3& direction)
{
  const MiSceneFrameInfo& fi = fc.frameInfo;
  // (IEEE division / square root whatever the compile options -- divExact, normalizeExact: camera rays agree with the oracle bit for bit)
  f2 clip = mk2(divExact(samplePos.x + offset.x, float(fc.width)) * 2.0f - 1.0f, divExact(samplePos.y + offset.y, float(fc.height)) * 2.0f - 1.0f);
  f4 view = mulFull(fi.projInv, mk4(clip.x, clip.y, -1.0f, 1.0f));
  view    = mk4(divExact(view.x, view.w), divExact(view.y, view.w), divExact(view.z, view.w), divExact(view.w, view.w));
  if(hasFlag(fi.flags, MI_SCENE_IS_ORTHOGRAPHIC))
  {
    origin    = xyz(mulFull(fi.viewInv, view));
    direction = normalizeExact(xyz(mulFull(fi.viewInv, mk4(0, 0, -1, 0))));
  }
  else
  {
    origin    = mk3(fi.viewInv[12], fi.viewInv[13], fi.viewInv[14]);
    direction = normalizeExact(xyz(mulFull(fi.viewInv, view)) - origin);
  }
}

PT_DEV uint32_t laneId() { return __lane_id(); }

// ---- slot <-> pixel -----------------------------------------------------------------------------------------------------------
// Slots are tile-major; inside a tile 8x8 micro-tiles, so one 64-lane wave owns one 8x8 pixel block (coherent camera rays).
// ownedTiles[i] = x0 | y0 << 16 (pixel origin of the i-th tile this rank renders).
PT_DEV bool slotToPixel(const FrameConsts& fc, const uint32_t* ownedTiles, uint32_t slot, int& px, int& py)
{
  const uint32_t tile  = ownedTiles[slot >> (2 * fc.tileShift)];
  const uint32_t w     = slot & ((1u << (2 * fc.tileShift)) - 1u);
  const uint32_t micro = w >> 6, lane = w & 63u;
  const uint32_t mshift = uint32_t(fc.tileShift) - 3u;
  px                   = int((tile & 0xffffu) + (micro & ((1u << mshift) - 1u)) * 8u + (lane & 7u));
  py                   = int((tile >> 16) + (micro >> mshift) * 8u + (lane >> 3));
  return px < fc.width && py < fc.height;
}

// The slot -> (frame, pixel) map of generateCameraPath below on its own, for a generator that forms no ray (k_generate_rays, camera_rays.hip): the
// same per-wave scalar arithmetic in both slot layouts.  pixelSlot: index of the per-pixel records (pathSlotPixel).  Returns whether the slot maps
// to a pixel of the image.
PT_DEV bool slotFramePixel(const FrameConsts& fc, const uint32_t* ownedTiles, uint32_t slot, uint32_t& frame, uint32_t& pixelSlot, int& px, int& py)
{
  const uint32_t lane = laneId();
  const uint32_t base = __builtin_amdgcn_readfirstlane(slot - lane);
  uint32_t       pixelBase, inMicro;
  if(fc.slotLayout == 1)
  {
    const uint32_t pslot = __umulhi(base, fc.framesMagic) >> fc.framesShift;
    frame                = base - pslot * uint32_t(fc.numFrames) + lane;
    pixelBase            = pslot & ~63u;
    inMicro              = pslot & 63u;
  }
  else
  {
    const uint32_t waveIdx = base >> 6;
    const uint32_t mtile   = fc.numFrames > 1 ? (__umulhi(waveIdx, fc.framesMagic) >> fc.framesShift) : waveIdx;
    frame                  = waveIdx - mtile * uint32_t(fc.numFrames);
    pixelBase              = mtile * 64u;
    inMicro                = lane;
  }
  pixelSlot             = pixelBase + inMicro;
  const uint32_t tile   = ownedTiles[pixelBase >> (2 * fc.tileShift)];
  const uint32_t micro  = (pixelBase & ((1u << (2 * fc.tileShift)) - 1u)) >> 6;
  const uint32_t mshift = uint32_t(fc.tileShift) - 3u;
  px                    = int((tile & 0xffffu) + (micro & ((1u << mshift) - 1u)) * 8u + (inMicro & 7u));
  py                    = int((tile >> 16) + (micro >> mshift) * 8u + (inMicro >> 3));
  return px < fc.width && py < fc.height;
}

//================================================================================================================================
// Camera paths: seed, AA jitter, camera ray, thin-lens DoF  (gltf_pathtrace.slang:546-596, 502-529)
//================================================================================================================================
struct CameraPath
{
  bool     valid;  // the slot maps to a pixel of the image
  uint32_t frame;  // frame of the batch the slot belongs to (wave-uniform)
  uint32_t seed;   // RNG state after the camera draws
  f3       origin, direction;
};
// Start of sample `sampleIndex` of path slot `slot` (slot < batchSlots).  Resets the denoiser guides of the slot on sample 0; the
// caller stores the seed (PathSoA::misc).  PathTracerState{} of gltf_pathtrace.slang:443 is implicit: throughput 1, lastSamplePdf
// DIRAC, radiance 0, maxRoughness 0, not inside, depth 0 -- the bounce-0 shade launch knows it as constants (k_shade<FIRST>), the
// medium is written when a path first enters one, firstHit by the first shade of the path, pixelSum by k_finish_sample.
// Cost note: the bounce-0 kernel is bound by vector-instruction issue (2 500 per wave of 64 camera rays, of which this function
// was 900 in its first form).  What is wave-uniform runs on the scalar unit: a wave's 64 slots are consecutive and 64-aligned
// and the slots are micro-tile major (FrameConsts::numFrames), so the frame index, the tile and the micro-tile are computed once per
// wave (the division by numFrames is a multiply-high by FrameConsts::framesMagic).  With aperture = 0 (wave-uniform) the lens offset is
// (cos, sin) * sqrt(0) = 0 whatever the angle: the two draws still advance the seed, the sine and cosine are skipped.
// The arithmetic that forms the ray stays correctly rounded (IEEE division, square root) -- it is what makes the camera rays,
// and with them coverage, selection ids and the segment counters, agree with the oracle bit for bit; hardware reciprocals and
// v_sin / v_cos here bought 1 % more and moved silhouette samples (tried, dropped).
PT_DEV CameraPath generateCameraPath(const FrameConsts& fc, const PathSoA& P, const uint32_t* ownedTiles, uint32_t slot, int sampleIndex)
{
  CameraPath cp;
  cp.frame     = 0u;
  cp.seed      = 0u;
  cp.origin    = mk3(0.0f);
  cp.direction = mk3(0.0f);
  // ---- slot -> (frame, pixel): see slotToPixel; per wave
  const uint32_t lane      = laneId();
  const uint32_t base      = __builtin_amdgcn_readfirstlane(slot - lane);
  uint32_t frame, pixelBase, inMicro;
  if(fc.slotLayout == 1)
  {
    // pixel major: the wave is 64 consecutive frames of pixel slot base / numFrames
    const uint32_t pslot = __umulhi(base, fc.framesMagic) >> fc.framesShift;
    frame                = base - pslot * uint32_t(fc.numFrames) + lane;
    pixelBase            = pslot & ~63u;
    inMicro              = pslot & 63u;
  }
  else
  {
    // micro-tile major: wave w = base / 64 works on micro-tile w / numFrames of frame w % numFrames (pathSlot)
    const uint32_t waveIdx = base >> 6;
    const uint32_t mtile   = fc.numFrames > 1 ? (__umulhi(waveIdx, fc.framesMagic) >> fc.framesShift) : waveIdx;
    frame                  = waveIdx - mtile * uint32_t(fc.numFrames);
    pixelBase              = mtile * 64u;
    inMicro                = lane;
  }
  cp.frame                 = frame;
  const uint32_t tile      = ownedTiles[pixelBase >> (2 * fc.tileShift)];
  const uint32_t micro     = (pixelBase & ((1u << (2 * fc.tileShift)) - 1u)) >> 6;
  const uint32_t mshift    = uint32_t(fc.tileShift) - 3u;
  const int      px        = int((tile & 0xffffu) + (micro & ((1u << mshift) - 1u)) * 8u + (inMicro & 7u));
  const int      py        = int((tile >> 16) + (micro >> mshift) * 8u + (inMicro >> 3));
  cp.valid                 = px < fc.width && py < fc.height;
  if(!cp.valid)
    return cp;
  uint32_t seed;
  f2       jitter;
  if(sampleIndex == 0)
  {
    seed     = xxhash32(uint32_t(px), uint32_t(py), uint32_t(fc.pc.frameCount) + frame);
    float u1 = rnd(seed), u2 = rnd(seed);
    // sampleGaussian (Box-Muller), pathtrace_functions.h.slang:784-789
    float r     = sqrtExact(-2.0f * logExact(fmaxf(1e-38f, u1)));
    float theta = 2.0f * K_PI * u2;
    jitter      = mk2(0.5f + ANTIALIASING_STANDARD_DEVIATION * (r * cosExact(theta)), 0.5f + ANTIALIASING_STANDARD_DEVIATION * (r * sinExact(theta)));
    // (single-sample frames: the guide records are WRITTEN by the path's first shade -- or zeroed where a path has none -- instead of zeroed here and
    //  read, added to and written back there: 64 B per path less)
    if(P.guideAlbedo && fc.pc.numSamples > 1)
    {
      P.guideAlbedo[slot] = make_float4(0, 0, 0, 0);
      P.guideNormal[slot] = make_float4(0, 0, 0, 0);
    }
  }
  else
  {
    seed     = __float_as_uint(P.misc[slot].z);
    float u1 = rnd(seed), u2 = rnd(seed);
    jitter   = mk2(u1, u2);
  }
  // getRay (pathtrace_functions.h.slang:791-811)
  const MiSceneFrameInfo& fi = fc.frameInfo;
  const f2 clip = mk2(divExact(float(px) + jitter.x, float(fc.width)) * 2.0f - 1.0f, divExact(float(py) + jitter.y, float(fc.height)) * 2.0f - 1.0f);
  f4       view = mulFull(fi.projInv, mk4(clip.x, clip.y, -1.0f, 1.0f));
  view          = mk4(divExact(view.x, view.w), divExact(view.y, view.w), divExact(view.z, view.w), divExact(view.w, view.w));
  f3 origin, direction;
  if(hasFlag(fi.flags, MI_SCENE_IS_ORTHOGRAPHIC))
  {
    origin    = xyz(mulFull(fi.viewInv, view));
    direction = normalizeExact(xyz(mulFull(fi.viewInv, mk4(0, 0, -1, 0))));
  }
  else
  {
    origin    = mk3(fi.viewInv[12], fi.viewInv[13], fi.viewInv[14]);
    direction = normalizeExact(xyz(mulFull(fi.viewInv, view)) - origin);
    // thin lens (gltf_pathtrace.slang:502-529)
    const float* V          = fi.viewInv;
    f3           focalPoint = direction * fc.pc.focalDistance;
    float        cam_r1     = rnd(seed) * K_TWO_PI;
    float        cam_r2     = rnd(seed) * fc.pc.aperture;
    f3           aperturePos = mk3(0.0f);
    if(fc.pc.aperture != 0.0f)
    {
      f3 cam_right = mk3(V[0], V[4], V[8]);  // Slang mul(viewMatrixI, float4(1,0,0,0)) = M^T e0
      f3 cam_up    = mk3(V[1], V[5], V[9]);
      aperturePos  = (cam_right * cosExact(cam_r1) + cam_up * sinExact(cam_r1)) * sqrtExact(cam_r2);
    }
    direction = normalizeExact(focalPoint - aperturePos);
    origin += aperturePos;
  }
  cp.seed      = seed;
  cp.origin    = origin;
  cp.direction = normalizeExact(direction);  // pathTrace loop head, gltf_pathtrace.slang:447
  return cp;
}

}  // namespace pt
