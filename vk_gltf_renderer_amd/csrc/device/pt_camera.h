// The camera ray of a pixel position, shared by the path-trace kernels (pt_kernels.hip) and the pick kernel (query.hip): both must form
// the same ray bit for bit whatever their translation unit's floating-point options, so everything inexact in it goes through divExact /
// normalizeExact (pt_math.h).
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

}  // namespace pt
