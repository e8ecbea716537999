// C-ABI wrapper of the host scene front end (see include/mi_host.h).
#include "mi_host.h"
#include "mikktspace_tangents.hpp"

#include <cmath>
#include <cstring>
#include <string>

#include "gltf_scene.hpp"

namespace {
thread_local std::string g_hostError;
}

struct MiScene
{
  mihost::GltfScene scene;
};
struct MiHdr
{
  mihost::HdrEnvironment hdr;
};

extern "C" {

const char* mi_host_last_error(void)
{
  return g_hostError.c_str();
}

int mi_scene_load(const char* path, MiScene** out)
{
  if(!path || !out)
  {
    g_hostError = "mi_scene_load: null argument";
    return MI_PT_ERR_ARGUMENT;
  }
  MiScene* s = new MiScene();
  try
  {
    if(!s->scene.load(path))
    {
      g_hostError = s->scene.error();
      delete s;
      return MI_PT_ERR_IO;
    }
  }
  catch(const std::exception& e)
  {
    g_hostError = e.what();
    delete s;
    return MI_PT_ERR_IO;
  }
  *out = s;
  return MI_PT_OK;
}
void mi_scene_destroy(MiScene* scene)
{
  delete scene;
}
int mi_scene_recompute_tangents(MiScene* scene, int forceCreation, int mikktspace)
{
  if(!scene)
  {
    g_hostError = "mi_scene_recompute_tangents: null scene";
    return MI_PT_ERR_ARGUMENT;
  }
  try
  {
    return int(scene->scene.recomputeTangents(forceCreation != 0, mikktspace != 0));
  }
  catch(const std::exception& e)
  {
    g_hostError = e.what();
    return MI_PT_ERR_IO;
  }
}
int64_t mi_scene_cut_alpha(MiScene* scene, int subdivisions)
{
  if(!scene)
  {
    g_hostError = "mi_scene_cut_alpha: null scene";
    return MI_PT_ERR_ARGUMENT;
  }
  try
  {
    return int64_t(scene->scene.cutAlphaMasked(subdivisions));
  }
  catch(const std::exception& e)
  {
    g_hostError = e.what();
    return MI_PT_ERR_IO;
  }
}
int mi_scene_num_variants(const MiScene* scene)
{
  return scene ? scene->scene.numVariants() : 0;
}
int mi_scene_variant_name(const MiScene* scene, int index, char* name, int nameCapacity)
{
  if(!scene || index < 0 || index >= scene->scene.numVariants())
  {
    g_hostError = "mi_scene_variant_name: no such variant";
    return MI_PT_ERR_ARGUMENT;
  }
  if(name && nameCapacity > 0)
  {
    strncpy(name, scene->scene.variantName(index).c_str(), size_t(nameCapacity) - 1);
    name[nameCapacity - 1] = 0;
  }
  return MI_PT_OK;
}
int mi_scene_current_variant(const MiScene* scene)
{
  return scene ? scene->scene.currentVariant() : 0;
}
int mi_scene_set_variant(MiScene* scene, int variant)
{
  if(!scene)
  {
    g_hostError = "mi_scene_set_variant: null scene";
    return MI_PT_ERR_ARGUMENT;
  }
  const int changed = scene->scene.setVariant(variant);
  if(changed < 0)
  {
    g_hostError = "mi_scene_set_variant: " + scene->scene.error();
    return MI_PT_ERR_ARGUMENT;
  }
  return changed;
}
int mi_scene_num_animations(const MiScene* scene)
{
  return scene ? const_cast<MiScene*>(scene)->scene.numAnimations() : 0;
}
int mi_scene_animation_info(const MiScene* scene, int index, float* start, float* end, char* name, int nameCapacity)
{
  if(!scene || index < 0 || index >= const_cast<MiScene*>(scene)->scene.numAnimations())
  {
    g_hostError = "mi_scene_animation_info: no such animation";
    return MI_PT_ERR_ARGUMENT;
  }
  const mihost::AnimationInfo& info = const_cast<MiScene*>(scene)->scene.animationInfo(index);
  if(start)
    *start = info.start;
  if(end)
    *end = info.end;
  if(name && nameCapacity > 0)
  {
    strncpy(name, info.name.c_str(), size_t(nameCapacity) - 1);
    name[nameCapacity - 1] = 0;
  }
  return MI_PT_OK;
}
int mi_scene_update_animation(MiScene* scene, int index, float time)
{
  if(!scene || index < 0 || index >= scene->scene.numAnimations() || !std::isfinite(time))
  {
    g_hostError = "mi_scene_update_animation: no such animation, or a non-finite time";
    return MI_PT_ERR_ARGUMENT;
  }
  try
  {
    scene->scene.animationInfo(index).currentTime = time;
    const int r = scene->scene.updateAnimation(index);
    if(r < 0)
    {
      g_hostError = scene->scene.error();
      return MI_PT_ERR_ARGUMENT;
    }
    return r;
  }
  catch(const std::exception& e)
  {
    g_hostError = e.what();
    return MI_PT_ERR_IO;
  }
}
int mi_scene_animation_changes(const MiScene* scene)
{
  return scene ? scene->scene.lastAnimationChanges() : 0;
}
const MiPtDeformDesc* mi_scene_deformation(const MiScene* scene)
{
  return scene ? scene->scene.deformation() : nullptr;
}
int mi_scene_deform_on_host(MiScene* scene)
{
  if(!scene)
  {
    g_hostError = "mi_scene_deform_on_host: null scene";
    return MI_PT_ERR_ARGUMENT;
  }
  return scene->scene.deformOnHost();
}
int mi_mikktspace(const float* positions, const float* normals, const float* texCoords, uint32_t numVertices, const uint32_t* indices,
                  uint32_t numTriangles, float* cornerTangents)
{
  if(!positions || !normals || !texCoords || !indices || !cornerTangents)
  {
    g_hostError = "mi_mikktspace: null argument";
    return MI_PT_ERR_ARGUMENT;
  }
  for(size_t c = 0; c < size_t(numTriangles) * 3; ++c)
    if(indices[c] >= numVertices)
    {
      g_hostError = "mi_mikktspace: index out of range";
      return MI_PT_ERR_ARGUMENT;
    }
  try
  {
    std::vector<float> out;
    mihost::mikkTangentSpaces(positions, normals, texCoords, indices, numTriangles, out);
    std::memcpy(cornerTangents, out.data(), out.size() * sizeof(float));
  }
  catch(const std::exception& e)
  {
    g_hostError = e.what();
    return MI_PT_ERR_IO;
  }
  return MI_PT_OK;
}
const MiPtSceneDesc* mi_scene_desc(const MiScene* scene)
{
  return scene ? &scene->scene.desc() : nullptr;
}
int mi_scene_num_cameras(const MiScene* scene)
{
  return scene ? int(scene->scene.cameras().size()) : 0;
}
int mi_scene_camera(const MiScene* scene, int index, MiCamera* out)
{
  if(!scene || !out || index < 0 || index >= int(scene->scene.cameras().size()))
    return MI_PT_ERR_ARGUMENT;
  const mihost::RenderCamera& c = scene->scene.cameras()[size_t(index)];
  for(int i = 0; i < 3; ++i)
  {
    out->eye[i]    = float(c.eye[i]);
    out->center[i] = float(c.center[i]);
    out->up[i]     = float(c.up[i]);
  }
  out->znear        = float(c.znear);
  out->zfar         = float(c.zfar);
  out->orthographic = c.type == mihost::RenderCamera::eOrthographic ? 1 : 0;
  out->xmag         = float(c.xmag);
  out->ymag         = float(c.ymag);
  // reference: toManipulatorCamera, src/gltf_camera_utils.hpp:35-55
  out->fovDegrees = out->orthographic ? 45.0f : float(c.yfov * 180.0 / M_PI);
  return MI_PT_OK;
}
void mi_scene_bounds(const MiScene* scene, float bmin[3], float bmax[3])
{
  scene->scene.bounds(bmin, bmax);
}
uint64_t mi_scene_num_triangles(const MiScene* scene)
{
  return scene ? scene->scene.numTriangles() : 0;
}

int mi_hdr_load(const char* path, MiHdr** out)
{
  if(!path || !out)
    return MI_PT_ERR_ARGUMENT;
  MiHdr* h = new MiHdr();
  if(!h->hdr.load(path))
  {
    g_hostError = h->hdr.error();
    delete h;
    return MI_PT_ERR_IO;
  }
  *out = h;
  return MI_PT_OK;
}
int mi_hdr_from_pixels(int width, int height, const float* rgb, MiHdr** out)
{
  if(width <= 0 || height <= 0 || !rgb || !out)
    return MI_PT_ERR_ARGUMENT;
  MiHdr* h = new MiHdr();
  h->hdr.setPixels(width, height, rgb);
  *out = h;
  return MI_PT_OK;
}
void mi_hdr_destroy(MiHdr* hdr)
{
  delete hdr;
}
const MiPtEnvironment* mi_hdr_env(const MiHdr* hdr)
{
  return hdr ? &hdr->hdr.env() : nullptr;
}

void mi_default_sky(MiSkyPhysicalParameters* sky)
{
  MiSkyPhysicalParameters s{};
  s.rgbUnitConversion[0] = s.rgbUnitConversion[1] = s.rgbUnitConversion[2] = 1.0f / 80000.0f;
  s.multiplier                                                             = 0.1f;
  s.haze                                                                   = 0.1f;
  s.redblueshift                                                           = 0.1f;
  s.saturation                                                             = 1.0f;
  s.horizonHeight                                                          = 0.0f;
  s.groundColor[0] = s.groundColor[1] = s.groundColor[2] = 0.4f;
  s.horizonBlur                                          = 0.3f;
  s.nightColor[0] = s.nightColor[1] = s.nightColor[2] = 0.0f;
  s.sunDiskIntensity                                   = 1.0f;
  s.sunDirection[0] = s.sunDirection[1] = s.sunDirection[2] = 0.5773502691896258f;
  s.sunDiskScale                                             = 1.0f;
  s.sunGlowIntensity                                         = 1.0f;
  s.yIsUp                                                    = 1;
  *sky                                                       = s;
}

void mi_default_params(MiPathtraceParams* params)
{
  MiPathtraceParams p{};
  p.maxDepth              = 5;
  p.frameCount            = 0;
  p.fireflyClampThreshold = 10.0f;
  p.texGradScale          = 1.0f;
  p.numSamples            = 1;
  p.totalSamples          = 0;
  p.focalDistance         = 0.0f;
  p.aperture              = 0.0f;
  p.flags                 = 0;
  p.pixelAngle            = 0.0f;
  *params                 = p;
}

void mi_camera_frame_info(const MiCamera* cam, int width, int height, MiSceneFrameInfo* info, float* pixelAngle, float* focalDistance)
{
  mx::vec3 eye{cam->eye[0], cam->eye[1], cam->eye[2]}, center{cam->center[0], cam->center[1], cam->center[2]},
      up{cam->up[0], cam->up[1], cam->up[2]};
  mx::mat4 view   = mx::lookAt(eye, center, up);
  float    aspect = float(width) / float(height);
  mx::mat4 proj;
  if(cam->orthographic)
  {
    // nvutils::CameraManipulator orthographic: magnitudes scaled to the viewport aspect
    float xm = cam->xmag, ym = cam->ymag;
    proj = mx::orthoVk(-xm, xm, -ym, ym, cam->znear, cam->zfar);
  }
  else
    proj = mx::perspectiveVk(cam->fovDegrees * float(M_PI) / 180.0f, aspect, cam->znear, cam->zfar);
  mx::mat4 projInv  = mx::inverse(proj);
  mx::mat4 viewInv  = mx::inverse(view);
  mx::mat4 viewProj = mx::mul(proj, view);
  MiSceneFrameInfo f;
  memset(&f, 0, sizeof(f));
  memcpy(f.viewMatrix, view.m, 64);
  memcpy(f.projInv, projInv.m, 64);
  memcpy(f.viewInv, viewInv.m, 64);
  memcpy(f.viewProjMatrix, viewProj.m, 64);
  memcpy(f.prevMVP, viewProj.m, 64);
  f.imageSize[0] = float(width);
  f.imageSize[1] = float(height);
  f.flags        = cam->orthographic ? MI_SCENE_IS_ORTHOGRAPHIC : 0;
  // Settings defaults (reference: src/resources.hpp:82-131)
  f.envRotation               = 0.0f;
  f.envBlur                   = 0.0f;
  f.envIntensity              = 1.0f;
  f.visualization             = 0;
  f.infinitePlaneDistance     = 0.0f;
  f.infinitePlaneBaseColor[0] = f.infinitePlaneBaseColor[1] = f.infinitePlaneBaseColor[2] = 0.5f;
  f.infinitePlaneMetallic                                                                 = 0.0f;
  f.infinitePlaneRoughness                                                                = 0.5f;
  f.shadowCatcherDarkenAmount                                                             = 0.0f;
  *info                                                                                   = f;
  if(pixelAngle)
    *pixelAngle = 2.0f * std::fabs(projInv.at(1, 1)) / std::max(float(height), 1.0f);
  if(focalDistance)
    *focalDistance = mx::length(eye - center);
}
// Camera rays of a pose under a projection (include/mi_host.h): float64 arithmetic on the float matrices of mi_camera_frame_info, rounded once.
int mi_camera_rays(const MiCamera* cam, int projection, float fisheyeFovDegrees, int width, int height, const float* jitterXY, int numSets, MiPtRay* rays,
                   float* pixelAngle)
{
  const bool knownProjection = projection == MI_PROJECTION_PERSPECTIVE || projection == MI_PROJECTION_EQUIRECT || projection == MI_PROJECTION_FISHEYE;
  if(!cam || !rays || width <= 0 || height <= 0 || numSets < 1 || !knownProjection
     || (projection == MI_PROJECTION_FISHEYE && !(fisheyeFovDegrees > 0.0f && fisheyeFovDegrees <= 360.0f)))
  {
    g_hostError = "mi_camera_rays: need a camera, an output, width, height, numSets >= 1, a known projection and 0 < fisheyeFovDegrees <= 360";
    return MI_PT_ERR_ARGUMENT;
  }
  MiSceneFrameInfo fi;
  float            perspectiveAngle = 0.0f;
  mi_camera_frame_info(cam, width, height, &fi, &perspectiveAngle, nullptr);
  const float* V = fi.viewInv;
  const float* Pi = fi.projInv;
  const double W = double(width), H = double(height), pi = 3.14159265358979323846;
  const double right[3] = {V[0], V[1], V[2]}, up[3] = {V[4], V[5], V[6]}, forward[3] = {-double(V[8]), -double(V[9]), -double(V[10])};
  const double eye[3]   = {V[12], V[13], V[14]};
  const double fovRad   = double(fisheyeFovDegrees) * pi / 180.0;
  auto mul = [](const float* M, const double v[4], double r[4]) {
    for(int i = 0; i < 4; ++i)
      r[i] = double(M[i]) * v[0] + double(M[4 + i]) * v[1] + double(M[8 + i]) * v[2] + double(M[12 + i]) * v[3];
  };
  for(int s = 0; s < numSets; ++s)
  {
    const double jx = jitterXY ? double(jitterXY[2 * s]) : 0.5, jy = jitterXY ? double(jitterXY[2 * s + 1]) : 0.5;
    for(int py = 0; py < height; ++py)
      for(int px = 0; px < width; ++px)
      {
        const double x = double(px) + jx, y = double(py) + jy;
        double       o[3] = {eye[0], eye[1], eye[2]}, d[3] = {0.0, 0.0, 0.0};
        if(projection == MI_PROJECTION_PERSPECTIVE)
        {
          const double clip[4] = {x / W * 2.0 - 1.0, y / H * 2.0 - 1.0, -1.0, 1.0};
          double       view[4], world[4];
          mul(Pi, clip, view);
          for(int i = 0; i < 4; ++i)
            view[i] /= view[3];  // (view[3] last: it divides itself to 1)
          if(cam->orthographic)
          {
            const double axis[4] = {0.0, 0.0, -1.0, 0.0};
            mul(V, view, world);
            for(int i = 0; i < 3; ++i)
              o[i] = world[i];
            mul(V, axis, world);
            for(int i = 0; i < 3; ++i)
              d[i] = world[i];
          }
          else
          {
            mul(V, view, world);
            for(int i = 0; i < 3; ++i)
              d[i] = world[i] - eye[i];
          }
        }
        else if(projection == MI_PROJECTION_EQUIRECT)
        {
          const double phi = (x / W - 0.5) * 2.0 * pi, theta = (0.5 - y / H) * pi;
          for(int i = 0; i < 3; ++i)
            d[i] = std::cos(theta) * std::sin(phi) * right[i] + std::sin(theta) * up[i] + std::cos(theta) * std::cos(phi) * forward[i];
        }
        else
        {
          const double R = std::min(W, H) / 2.0, u = (x - W / 2.0) / R, v = (H / 2.0 - y) / R, r = std::sqrt(u * u + v * v);
          if(r <= 1.0)  // (outside the image circle: a dead ray, zero direction)
          {
            const double alpha = r * fovRad / 2.0;
            for(int i = 0; i < 3; ++i)
              d[i] = r > 0.0 ? std::sin(alpha) * (u * right[i] + v * up[i]) / r + std::cos(alpha) * forward[i] : forward[i];
          }
        }
        const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        MiPtRay&     ray = rays[(size_t(s) * size_t(height) + size_t(py)) * size_t(width) + size_t(px)];
        for(int i = 0; i < 3; ++i)
        {
          ray.origin[i]    = float(o[i]);
          ray.direction[i] = len > 0.0 ? float(d[i] / len) : 0.0f;
        }
        ray.tMin = 0.0f;
        ray.tMax = 3.402823466e+38f;
      }
  }
  if(pixelAngle)
    *pixelAngle = projection == MI_PROJECTION_PERSPECTIVE ? perspectiveAngle
                                                          : float(projection == MI_PROJECTION_EQUIRECT ? pi / H : fovRad / std::min(W, H));
  return MI_PT_OK;
}
// The loader's mip chain of one image (include/mi_host.h): buildMipChain, levels 1.. packed one after the other.
int mi_build_mip_chain(int width, int height, const uint8_t* rgba8, int srgb, uint8_t* outLevels1ToN)
{
  if(!rgba8 || width < 1 || height < 1 || width > 65535 || height > 65535)
  {
    g_hostError = "mi_build_mip_chain: need level 0 and a size of 1 .. 65535";
    return MI_PT_ERR_ARGUMENT;
  }
  if(!outLevels1ToN)
  {
    int n = 0;
    for(int w = width, h = height; w > 1 || h > 1; w = std::max(1, w / 2), h = std::max(1, h / 2))
      ++n;
    return n;
  }
  mihost::Image base;
  base.width  = width;
  base.height = height;
  base.rgba.assign(rgba8, rgba8 + size_t(width) * size_t(height) * 4);
  std::vector<std::vector<uint8_t>> levels;
  mihost::buildMipChain(base, srgb != 0, levels);
  for(size_t l = 1; l < levels.size(); ++l)
  {
    memcpy(outLevels1ToN, levels[l].data(), levels[l].size());
    outLevels1ToN += levels[l].size();
  }
  return int(levels.size()) - 1;
}
void mi_linear_to_srgb8(const float* values, uint64_t count, uint8_t* out)
{
  for(uint64_t i = 0; values && out && i < count; ++i)
    out[i] = mihost::linearToSrgb8(values[i]);
}
}
