// Keyframe animation: glTF 2.0 `animations` with translation / rotation / scale / weights channels and LINEAR, STEP and CUBICSPLINE
// samplers (glTF 2.0 specification, section 3.11 and appendix C), evaluated into per-node poses and per-mesh morph weights, from which
// the world matrices, the render-node table, the light placements and the deformation tables are recomputed in place.  Behaviour
// follows the reference's AnimationSystem (src/gltf_scene_animation.cpp:84-175 parse, :355-478 update / segment search, :484-700
// interpolation): a sampler needs two keyframes, a channel is applied only while the time lies inside its keyframe range, the
// clip's [start, end] is the hull of all sampler inputs, rotations are slerped (LINEAR) or spline-evaluated and normalised.  Weights
// channels are evaluated with all three samplers as the specification defines them (a CUBICSPLINE key holds in-tangents, values and
// out-tangents of every target); the reference interpolates LINEAR ones only.
// Skins and morph targets (parseDeformation, reference: src/gltf_scene_animation.cpp:196-320): the vertex data they change is deformed
// on the device (mi_pt_update_deformation, csrc/device/deform.hip) from the per-frame tables built here -- joint matrices
// inverse(world[refNode]) * world[joint] * IBM (reference: src/gltf_scene_animation_vk.cpp:454-478) and the mesh weights -- or on the
// host by deformOnHost, the CPU restatement of that kernel.
// KHR_animation_pointer (reference: src/gltf_animation_pointer.cpp, src/gltf_scene_animation.cpp:373-437): a channel whose target path is
// "pointer" addresses a property of the document by JSON pointer; SCALAR / VEC2 / VEC3 / VEC4 outputs, all three samplers componentwise.
// Pointers are resolved once, at parse (resolvePointer): materials, KHR_lights_punctual lights, cameras, KHR_node_visibility and -- which the
// reference parses but drops in syncNode (:371-397) although the extension allows them -- node translation / rotation / scale, routed into
// the pose code of the core channels (`weights` by pointer is not evaluated).  A material, light or camera value is written into the document
// (the reference's shadow JSON) and the ONE conversion of the loader runs again for that object, so every property the loader understands
// animates; the tables are rewritten in place.  Unresolvable pointers, out-of-range indices and outputs whose width does not fit the property
// are dropped at parse: scene files are untrusted.
#include <algorithm>
#include <cmath>
#include <map>
#include <cstring>
#include <limits>
#include <set>

#include "gltf_scene.hpp"
#include "mi_host.h"  // MI_SCENE_CHANGED_*

namespace mihost {

using mijson::Value;

float AnimationInfo::incrementTime(float deltaTime, bool loop)  // reference: src/gltf_scene.hpp:166-188
{
  currentTime += deltaTime;
  if(loop)
  {
    const float duration = end - start;
    if(!(duration > 0.0f))  // a clip with one keyframe (or none): fmod(x, 0) is NaN and would stick -- the clip has one pose
      return currentTime = start;
    float       wrapped  = std::fmod(currentTime - start, duration);
    if(wrapped < 0.0f)
      wrapped += duration;
    currentTime = start + wrapped;
  }
  else if(currentTime > end)
    currentTime = end;
  return currentTime;
}

namespace {

std::vector<std::string> splitPointer(const std::string& p)  // RFC 6901: "/a/b" -> {a, b}, ~1 = '/', ~0 = '~'
{
  std::vector<std::string> out;
  if(p.empty() || p[0] != '/')
    return out;
  std::string cur;
  for(size_t i = 1; i <= p.size(); ++i)
  {
    if(i == p.size() || p[i] == '/')
    {
      out.push_back(cur);
      cur.clear();
    }
    else if(p[i] == '~' && i + 1 < p.size() && (p[i + 1] == '0' || p[i + 1] == '1'))
      cur += p[++i] == '1' ? '/' : '~';
    else
      cur += p[i];
  }
  return out;
}
bool parseIndex(const std::string& s, size_t count, int& out)
{
  if(s.empty() || s.size() > 9)
    return false;
  for(char c : s)
    if(c < '0' || c > '9')
      return false;
  const long v = std::strtol(s.c_str(), nullptr, 10);
  if(size_t(v) >= count)
    return false;
  out = int(v);
  return true;
}
const Value* findKey(const Value& o, const std::string& key)
{
  return o.isObject() ? o.find(key) : nullptr;
}
// The components a material property takes when the document does not hold it yet (glTF 2.0 and the KHR_materials_* / KHR_texture_transform
// schemas): by its key, and by the object it lives in where a key has two meanings.
int materialPropertyWidth(const std::vector<std::string>& keys)
{
  const std::string& key    = keys.back();
  const std::string  parent = keys.size() >= 2 ? keys[keys.size() - 2] : std::string();
  if(parent == "KHR_texture_transform")
    return (key == "offset" || key == "scale") ? 2 : 1;
  if(key == "baseColorFactor" || key == "diffuseFactor")
    return 4;
  if(key == "specularFactor")
    return parent == "KHR_materials_pbrSpecularGlossiness" ? 3 : 1;
  if(key == "emissiveFactor" || key == "attenuationColor" || key == "specularColorFactor" || key == "sheenColorFactor"
     || key == "diffuseTransmissionColorFactor" || key == "multiscatterColor")
    return 3;
  return 1;
}
// Writes `n` floats at keys[from ...] below `at`, creating absent objects on the way (a number for n == 1, an array otherwise; a bool for
// `asBool`).  Array elements on the way must exist.  False (and nothing written) when the way leads through something that is not a container.
bool writeValue(Value& at, const std::vector<std::string>& keys, size_t from, const float* v, int n, bool asBool)
{
  Value* cur = &at;
  for(size_t k = from; k < keys.size(); ++k)
  {
    if(cur->type == Value::Array)
    {
      int i = 0;
      if(!parseIndex(keys[k], cur->arr.size(), i))
        return false;
      cur = &cur->arr[size_t(i)];
      continue;
    }
    if(cur->type == Value::Null)
      cur->type = Value::Object;
    if(cur->type != Value::Object)
      return false;
    Value* next = nullptr;
    for(auto& kv : cur->obj)
      if(kv.first == keys[k])
        next = &kv.second;
    if(!next)
    {
      cur->obj.emplace_back(keys[k], Value());
      next = &cur->obj.back().second;
    }
    cur = next;
  }
  Value out;
  if(asBool)
  {
    out.type = Value::Bool;
    out.b    = v[0] != 0.0f;  // (reference: src/gltf_animation_pointer.cpp:155)
  }
  else if(n == 1)
  {
    out.type = Value::Number;
    out.num  = double(v[0]);
  }
  else
  {
    out.type = Value::Array;
    out.arr.resize(size_t(n));
    for(int c = 0; c < n; ++c)
    {
      out.arr[size_t(c)].type = Value::Number;
      out.arr[size_t(c)].num  = double(v[c]);
    }
  }
  *cur = std::move(out);
  return true;
}

}  // namespace

// Resolves a KHR_animation_pointer target once (reference: parseResourceInfo, src/gltf_animation_pointer.cpp:103-139).  True: `ch` is a usable
// channel -- a pointer channel with target / index / keys, or, for /nodes/i/{translation, rotation, scale}, a core channel on node i.
bool GltfScene::resolvePointer(const std::string& pointer, int components, AnimationChannel& ch)
{
  const std::vector<std::string> keys = splitPointer(pointer);
  if(keys.size() < 3 || components < 1 || components > 4)
    return false;
  // the property as the document holds it, if it does: a number or an array of numbers, whose width the output must have
  auto widthInDocument = [&](int& width) -> bool {  // false: the way is blocked (not a container, or a value that is neither number nor array)
    const Value* cur = &m_doc;
    width            = 0;
    for(size_t k = 0; k < keys.size(); ++k)
    {
      if(cur->isArray())
      {
        int i = 0;
        if(!parseIndex(keys[k], cur->arr.size(), i))
          return false;
        cur = &cur->arr[size_t(i)];
      }
      else if(cur->isObject())
      {
        cur = findKey(*cur, keys[k]);
        if(!cur)
          return true;  // absent from here on: created at the first write
      }
      else
        return false;
    }
    if(cur->isNumber())
      width = 1;
    else if(cur->isArray() && !cur->arr.empty() && cur->arr.size() <= 4)
    {
      for(const Value& e : cur->arr)
        if(!e.isNumber())
          return false;
      width = int(cur->arr.size());
    }
    else if(cur->type == Value::Bool && ch.target == AnimationChannel::eVisibility)
      width = 1;
    else
      return false;
    return true;
  };
  int index = -1, width = 0;
  if(keys[0] == "materials" && parseIndex(keys[1], m_doc["materials"].size(), index))
  {
    ch.target = AnimationChannel::eMaterial;
    if(!widthInDocument(width))
      return false;
    if(width == 0)
      width = materialPropertyWidth(keys);
    if(width != components)
      return false;
    // its alpha state: never cut by cutAlphaMasked
    bool alpha = keys.back() == "alphaCutoff" || keys.back() == "alphaMode";
    for(const std::string& k : keys)
      alpha = alpha || k == "baseColorFactor" || k == "diffuseFactor" || k == "baseColorTexture" || k == "diffuseTexture";
    if(alpha)
    {
      m_alphaAnimated.resize(std::max(m_alphaAnimated.size(), m_materials.size()), 0);
      if(size_t(index) < m_alphaAnimated.size())
        m_alphaAnimated[size_t(index)] = 1;
    }
  }
  else if(keys[0] == "extensions" && keys.size() >= 5 && keys[1] == "KHR_lights_punctual" && keys[2] == "lights"
          && parseIndex(keys[3], m_doc["extensions"]["KHR_lights_punctual"]["lights"].size(), index))
  {
    ch.target = AnimationChannel::eLight;
    const std::string& k = keys[4];
    if(keys.size() == 5 && k == "color")
      width = 3;
    else if(keys.size() == 5 && (k == "intensity" || k == "range"))
      width = 1;
    else if(keys.size() == 6 && k == "spot" && (keys[5] == "innerConeAngle" || keys[5] == "outerConeAngle"))
      width = 1;
    else
      return false;
    if(width != components)
      return false;
  }
  else if(keys[0] == "cameras" && keys.size() == 4 && parseIndex(keys[1], m_doc["cameras"].size(), index))
  {
    ch.target = AnimationChannel::eCamera;
    const std::string &g = keys[2], &k = keys[3];
    const bool persp = g == "perspective" && (k == "yfov" || k == "aspectRatio" || k == "znear" || k == "zfar");
    const bool ortho = g == "orthographic" && (k == "xmag" || k == "ymag" || k == "znear" || k == "zfar");
    if((!persp && !ortho) || components != 1)
      return false;
  }
  else if(keys[0] == "nodes" && parseIndex(keys[1], m_doc["nodes"].size(), index))
  {
    if(keys.size() == 3 && (keys[2] == "translation" || keys[2] == "rotation" || keys[2] == "scale"))
    {
      ch.path = keys[2] == "translation" ? AnimationChannel::eTranslation : (keys[2] == "rotation" ? AnimationChannel::eRotation : AnimationChannel::eScale);
      ch.node = index;
      return true;  // (the caller checks the width like a core channel's)
    }
    if(!(keys.size() == 5 && keys[2] == "extensions" && keys[3] == "KHR_node_visibility" && keys[4] == "visible") || components != 1)
      return false;
    ch.target = AnimationChannel::eVisibility;
  }
  else
    return false;
  ch.index = index;
  ch.keys  = keys;
  return true;
}

void GltfScene::parseAnimations()
{
  m_alphaAnimated.assign(m_materials.size(), 0);
  const Value& anims = m_doc["animations"];
  for(size_t a = 0; a < anims.size(); ++a)
  {
    const Value& ga = anims[a];
    Animation    anim;
    anim.info.name = ga["name"].string("Animation" + std::to_string(a));
    const Value& samplers = ga["samplers"];
    for(size_t i = 0; i < samplers.size(); ++i)
    {
      const Value&     gs = samplers[i];
      AnimationSampler sm;
      const std::string ip = gs["interpolation"].string("LINEAR");
      sm.interpolation     = ip == "STEP" ? AnimationSampler::eStep : (ip == "CUBICSPLINE" ? AnimationSampler::eCubicSpline : AnimationSampler::eLinear);
      if(!gs["input"].isNumber() || !readAccessorFloats(gs["input"].integer(-1), 1, sm.inputs))
        sm.inputs.clear();
      if(!gs["output"].isNumber() || !readAccessorFloats(gs["output"].integer(-1), 0, sm.outputs, &sm.components) || sm.components <= 0)
      {
        sm.inputs.clear();
        sm.outputs.clear();
        sm.components = 1;
      }
      // key times and values of a usable sampler are finite (a NaN time would pass every range test below and pose the node at NaN)
      bool finite = true;
      for(float t : sm.inputs)
        finite = finite && std::isfinite(t);
      for(float v : sm.outputs)
        finite = finite && std::isfinite(v);
      if(!finite)
      {
        sm.inputs.clear();
        sm.outputs.clear();
      }
      for(float t : sm.inputs)
      {
        anim.info.start = std::min(anim.info.start, t);
        anim.info.end   = std::max(anim.info.end, t);
      }
      anim.samplers.push_back(std::move(sm));
    }
    const Value& channels = ga["channels"];
    for(size_t i = 0; i < channels.size(); ++i)
    {
      const Value&      gc   = channels[i];
      const std::string path = gc["target"]["path"].string("");
      AnimationChannel  ch;
      if(path == "translation")
        ch.path = AnimationChannel::eTranslation;
      else if(path == "rotation")
        ch.path = AnimationChannel::eRotation;
      else if(path == "scale")
        ch.path = AnimationChannel::eScale;
      else if(path == "weights")
        ch.path = AnimationChannel::eWeights;
      else if(path == "pointer")
        ch.path = AnimationChannel::ePointer;
      else
        continue;
      ch.node    = gc["target"]["node"].integer(-1);
      ch.sampler = gc["sampler"].integer(-1);
      if(ch.sampler < 0 || size_t(ch.sampler) >= anim.samplers.size())
        continue;
      if(ch.path == AnimationChannel::ePointer)
      {
        const Value& ptr = gc["target"]["extensions"]["KHR_animation_pointer"]["pointer"];
        if(!ptr.isString() || !resolvePointer(ptr.str, anim.samplers[size_t(ch.sampler)].components, ch))
          continue;
        if(ch.path == AnimationChannel::ePointer)  // (node TRS pointers became core channels and go on below)
        {
          anim.channels.push_back(ch);
          continue;
        }
      }
      if(ch.node < 0 || size_t(ch.node) >= m_nodePose.size())
        continue;
      if(ch.path == AnimationChannel::eWeights)
      {
        // the node's mesh takes the weights (node.weights is not evaluated, as in the reference); a key holds one value per target
        // (x3 for CUBICSPLINE), so the target count is what the output accessor holds per key
        const int               mesh = m_doc["nodes"][size_t(ch.node)]["mesh"].integer(-1);
        const AnimationSampler& sm   = anim.samplers[size_t(ch.sampler)];
        const size_t            keys = sm.inputs.size() * (sm.interpolation == AnimationSampler::eCubicSpline ? 3 : 1);
        if(mesh < 0 || size_t(mesh) >= m_doc["meshes"].size() || sm.components != 1 || keys == 0 || sm.outputs.size() % keys != 0
           || sm.outputs.empty())
          continue;
        ch.numWeights = int(sm.outputs.size() / keys);
        anim.channels.push_back(ch);
        continue;
      }
      const int need = ch.path == AnimationChannel::eRotation ? 4 : 3;
      if(anim.samplers[size_t(ch.sampler)].components != need)
        continue;
      anim.channels.push_back(ch);
    }
    if(anim.info.start > anim.info.end)  // no keyframes at all
      anim.info.start = anim.info.end = 0.0f;
    anim.info.currentTime = 0.0f;
    m_animations.push_back(std::move(anim));
  }
}

namespace {

// glm::slerp followed by glm::normalize (shortest path; nearly parallel quaternions are lerped)
void slerpNormalized(const float* a, const float* b, float t, float* out)
{
  float z[4]     = {b[0], b[1], b[2], b[3]};
  float cosTheta = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  if(cosTheta < 0.0f)
  {
    for(float& c : z)
      c = -c;
    cosTheta = -cosTheta;
  }
  if(cosTheta > 1.0f - std::numeric_limits<float>::epsilon())
  {
    for(int i = 0; i < 4; ++i)
      out[i] = a[i] + t * (z[i] - a[i]);
  }
  else
  {
    const float angle = std::acos(cosTheta);
    const float wa = std::sin((1.0f - t) * angle), wb = std::sin(t * angle), inv = 1.0f / std::sin(angle);
    for(int i = 0; i < 4; ++i)
      out[i] = (wa * a[i] + wb * z[i]) * inv;
  }
  const float len = std::sqrt(out[0] * out[0] + out[1] * out[1] + out[2] * out[2] + out[3] * out[3]);
  if(len > 0.0f)
    for(int i = 0; i < 4; ++i)
      out[i] /= len;
}

}  // namespace

int GltfScene::updateAnimation(int index)
{
  m_lastChanges = 0;
  if(index < 0 || size_t(index) >= m_animations.size())
    return 0;
  const Animation& anim = m_animations[size_t(index)];
  const float      time = anim.info.currentTime;
  bool             any  = false, anyWeights = false, anyPointer = false;

  // The value of a channel at `time` into vbuf (at least 4 floats; nc of them count): false when the time lies outside its keyframe range or
  // the sampler is unusable.
  auto sample = [&](const AnimationChannel& ch, std::vector<float>& vbuf, int& ncOut) -> bool {
    const AnimationSampler& sm = anim.samplers[size_t(ch.sampler)];
    const size_t            nk = sm.inputs.size();
    if(nk < 2)
      return false;
    // the segment [i, i+1] that holds `time` (first keyframe strictly after it, minus one)
    auto it = std::upper_bound(sm.inputs.begin(), sm.inputs.end(), time);
    if(it == sm.inputs.begin())
      return false;
    size_t i = size_t(it - sm.inputs.begin()) - 1;
    if(i + 1 >= nk)
      i = nk - 2;
    const float t0 = sm.inputs[i], t1 = sm.inputs[i + 1];
    if(!(time >= t0 && time <= t1))
      return false;
    const float keyDelta = t1 - t0;
    const float t        = std::fabs(keyDelta) < std::numeric_limits<float>::epsilon() ? 0.0f : std::min(std::max((time - t0) / keyDelta, 0.0f), 1.0f);
    const bool  weights  = ch.path == AnimationChannel::eWeights;
    const int   nc       = weights ? ch.numWeights : sm.components;
    const size_t numOut  = sm.outputs.size() / size_t(nc);
    vbuf.assign(size_t(std::max(nc, 4)), 0.0f);
    ncOut                = nc;
    float*      v        = vbuf.data();
    v[3]                 = weights ? v[3] : 1.0f;
    bool        have     = false;
    switch(sm.interpolation)
    {
      case AnimationSampler::eLinear:
        if(i + 1 < numOut)
        {
          const float* a = &sm.outputs[i * size_t(nc)];
          const float* b = a + nc;
          if(ch.path == AnimationChannel::eRotation)
            slerpNormalized(a, b, t, v);
          else
            for(int c = 0; c < nc; ++c)
              v[c] = a[c] * (1.0f - t) + b[c] * t;  // glm::mix
          have = true;
        }
        break;
      case AnimationSampler::eStep:
        if(i < numOut)
        {
          memcpy(v, &sm.outputs[i * size_t(nc)], sizeof(float) * size_t(nc));
          have = true;
        }
        break;
      case AnimationSampler::eCubicSpline:
        if(numOut > (i + 1) * 3 + 1)
        {
          // cubic Hermite spline, glTF 2.0 appendix C: per keyframe (in-tangent a, value v, out-tangent b)
          const float  t2 = t * t, t3 = t2 * t;
          const float  cV1 = -2 * t3 + 3 * t2, cV0 = 1 - cV1, cA = keyDelta * (t3 - t2), cB = keyDelta * (t3 - 2 * t2 + t);
          const float* k0 = &sm.outputs[(i * 3) * size_t(nc)];
          const float* k1 = &sm.outputs[((i + 1) * 3) * size_t(nc)];
          for(int c = 0; c < nc; ++c)
            v[c] = k0[nc + c] * cV0 + k1[c] * cA + k0[2 * nc + c] * cB + k1[nc + c] * cV1;
          if(ch.path == AnimationChannel::eRotation)
          {
            const float len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
            if(len > 0.0f)
              for(int c = 0; c < 4; ++c)
                v[c] /= len;
          }
          have = true;
        }
        break;
    }
    return have;
  };

  // ---- KHR_animation_pointer on materials, first: the one step that can fail, and nothing else may have changed when it does.  The values
  // go into the document, the dirty materials through the loader's conversion again, into the slots they hold.
  std::vector<float> vbuf;
  int                nc = 0;
  {
    auto materialJson = [&](int m) -> Value* {
      for(auto& kv : m_doc.obj)
        if(kv.first == "materials" && kv.second.isArray() && size_t(m) < kv.second.arr.size())
          return &kv.second.arr[size_t(m)];
      return nullptr;
    };
    std::map<int, Value> saved;  // the dirty materials as the document held them
    for(const AnimationChannel& ch : anim.channels)
    {
      if(ch.path != AnimationChannel::ePointer || ch.target != AnimationChannel::eMaterial || !sample(ch, vbuf, nc))
        continue;
      Value* json = materialJson(ch.index);
      if(!json || size_t(ch.index) + 1 >= m_materialFirstInfo.size())
        continue;
      if(!saved.count(ch.index))
        saved.emplace(ch.index, *json);
      writeValue(m_doc, ch.keys, 0, vbuf.data(), nc, false);
    }
    std::map<int, std::pair<MiGltfShadeMaterial, std::vector<MiGltfTextureInfo>>> converted;
    bool                                                                          fits = true;
    for(const auto& kv : saved)
    {
      const uint32_t first = m_materialFirstInfo[size_t(kv.first)], end = m_materialFirstInfo[size_t(kv.first) + 1];
      std::vector<MiGltfTextureInfo> infos(first);  // (placeholders: the material's slot indices come out as they are in the table)
      const MiGltfShadeMaterial      d = convertMaterial(*materialJson(kv.first), infos);
      fits                             = fits && infos.size() == end;
      converted[kv.first]              = {d, std::vector<MiGltfTextureInfo>(infos.begin() + std::min<size_t>(first, infos.size()), infos.end())};
    }
    if(!fits)
    {
      for(const auto& kv : saved)
        *materialJson(kv.first) = kv.second;
      m_error = "updateAnimation: a KHR_animation_pointer channel would change the number of texture infos";
      return -1;
    }
    for(const auto& kv : converted)
    {
      m_materials[size_t(kv.first)] = kv.second.first;
      std::copy(kv.second.second.begin(), kv.second.second.end(), m_textureInfos.begin() + m_materialFirstInfo[size_t(kv.first)]);
    }
    if(!converted.empty())
    {
      anyPointer = true;
      m_lastChanges |= MI_SCENE_CHANGED_MATERIALS;
    }
  }

  std::set<int> lightsDirty, camerasDirty;
  bool          visibilityDirty = false;
  for(const AnimationChannel& ch : anim.channels)
  {
    if(ch.path == AnimationChannel::ePointer && ch.target == AnimationChannel::eMaterial)
      continue;
    if(!sample(ch, vbuf, nc))
      continue;
    float*     v       = vbuf.data();
    const bool weights = ch.path == AnimationChannel::eWeights;
    if(ch.path == AnimationChannel::ePointer)
    {
      if(!writeValue(m_doc, ch.keys, 0, v, nc, ch.target == AnimationChannel::eVisibility))
        continue;
      if(ch.target == AnimationChannel::eLight)
        lightsDirty.insert(ch.index);
      else if(ch.target == AnimationChannel::eCamera)
        camerasDirty.insert(ch.index);
      else
        visibilityDirty = true;
      anyPointer = true;
      continue;
    }
    if(weights)
    {
      std::vector<float>& mw = m_meshWeights[size_t(m_doc["nodes"][size_t(ch.node)]["mesh"].integer(-1))];
      mw.assign(v, v + nc);  // (the reference resizes mesh.weights to the channel's count as well)
      anyWeights = true;
      continue;
    }
    NodePose& pose = m_nodePose[size_t(ch.node)];
    if(!pose.animated)
    {
      // first touch: start from the document's TRS
      const Value& node = m_doc["nodes"][size_t(ch.node)];
      auto         get  = [&](const char* key, int n, float* out) {
        const Value& a = node[key];
        if(a.isArray() && a.arr.size() == size_t(n))
          for(int c = 0; c < n; ++c)
            out[c] = float(a.arr[size_t(c)].number());
      };
      get("translation", 3, pose.t);
      get("rotation", 4, pose.q);
      get("scale", 3, pose.s);
      pose.animated = true;
    }
    float* dst = ch.path == AnimationChannel::eTranslation ? pose.t : (ch.path == AnimationChannel::eRotation ? pose.q : pose.s);
    memcpy(dst, v, sizeof(float) * size_t(nc));
    any = true;
  }
  // ---- what the pointer channels changed, through the loader's own conversions (placement stays with the node path)
  if(!lightsDirty.empty())
  {
    const Value& lights = m_doc["extensions"]["KHR_lights_punctual"]["lights"];
    for(size_t l = 0; l < m_lights.size(); ++l)
      if(lightsDirty.count(m_lightIndex[l]))
        lightProperties(lights[size_t(m_lightIndex[l])], m_lights[l]);
    m_lastChanges |= MI_SCENE_CHANGED_LIGHTS;
  }
  if(!camerasDirty.empty())
  {
    for(size_t c = 0; c < m_cameras.size(); ++c)
      if(camerasDirty.count(m_cameraIndex[c]))
        cameraIntrinsics(m_doc["cameras"][size_t(m_cameraIndex[c])], m_cameras[c]);
    m_lastChanges |= MI_SCENE_CHANGED_CAMERAS;
  }
  if(visibilityDirty)
  {
    // the cascade of the load-time traversal: a render node is visible when no node on its path says otherwise
    const Value& nodes = m_doc["nodes"];
    for(size_t n = 0; n < m_renderNodes.size(); ++n)
    {
      bool visible = true;
      for(int id : m_renderNodeSource[n].path)
      {
        const Value& vis = nodes[size_t(id)]["extensions"]["KHR_node_visibility"]["visible"];
        visible          = visible && !(vis.type == Value::Bool && !vis.b);
      }
      m_renderNodeVisible[n] = visible ? 1 : 0;
    }
    m_lastChanges |= MI_SCENE_CHANGED_VISIBILITY;
  }
  if(!any)
  {
    if(anyWeights)
    {
      updateDeformTables();
      m_lastChanges |= MI_SCENE_CHANGED_DEFORMATION;
    }
    return (anyWeights || anyPointer) ? 1 : 0;
  }
  m_lastChanges |= MI_SCENE_CHANGED_NODES | (m_lights.empty() ? 0 : MI_SCENE_CHANGED_LIGHTS) | (m_deform.empty() ? 0 : MI_SCENE_CHANGED_DEFORMATION);

  // World matrices (reference: Scene::updateNodeWorldMatrices), per PATH from a scene root: glTF hierarchies are strict trees, but
  // load-time traversal instantiates a node of a non-conforming file under every parent it is listed by -- each such render node
  // (and light) keeps the path it was reached by and is posed along it, with the multiplication order of traverse().
  std::map<std::vector<int>, mx::mat4> cache;  // (distinct paths are few: render nodes of one glTF node share theirs)
  auto worldOf = [&](const std::vector<int>& path) {
    auto it = cache.find(path);
    if(it != cache.end())
      return it->second;
    mx::mat4 w = mx::identity();
    for(size_t i = 0; i < path.size(); ++i)
      w = i == 0 ? localMatrix(path[i]) : mx::mul(w, localMatrix(path[i]));
    cache.emplace(path, w);
    return w;
  };
  for(size_t n = 0; n < m_renderNodes.size(); ++n)
  {
    const RenderNodeSource& src = m_renderNodeSource[n];
    mx::mat4                w   = worldOf(src.path);
    if(src.instance >= 0)
      w = mx::mul(w, m_gpuInstanceLocalMatrices.at(src.node)[size_t(src.instance)]);
    MiGltfRenderNode& rn = m_renderNodes[n];
    memcpy(rn.objectToWorld, w.m, sizeof(rn.objectToWorld));
    const mx::mat4 inv = mx::inverse(w);
    memcpy(rn.worldToObject, inv.m, sizeof(rn.worldToObject));
  }
  for(size_t l = 0; l < m_lights.size(); ++l)
    placeLight(m_lights[l], worldOf(m_lightPath[l]));
  updateDeformTables();
  return 1;
}

//----------------------------------------------------------------------------------------------------------------------
// Skins and morph targets
//----------------------------------------------------------------------------------------------------------------------

// World matrix of every node from the current poses, along the first path from a scene root that reaches it (a node outside the
// scene hierarchy keeps its local matrix).
std::vector<mx::mat4> GltfScene::nodeWorldMatrices() const
{
  const size_t          n = m_doc["nodes"].size();
  std::vector<mx::mat4> world(n);
  std::vector<uint8_t>  done(n, 0);
  for(size_t i = 0; i < n; ++i)
    world[i] = localMatrix(int(i));
  std::vector<std::pair<int, mx::mat4>> stack;
  for(int r : m_roots)
    if(r >= 0 && size_t(r) < n && !done[size_t(r)])
      stack.push_back({r, mx::identity()});
  while(!stack.empty())
  {
    auto [node, parent] = stack.back();
    stack.pop_back();
    if(done[size_t(node)])
      continue;
    done[size_t(node)]  = 1;
    world[size_t(node)] = mx::mul(parent, localMatrix(node));
    const Value& children = m_doc["nodes"][size_t(node)]["children"];
    for(size_t c = children.size(); c-- > 0;)
    {
      const int child = children[c].integer(-1);
      if(child >= 0 && size_t(child) < n && !done[size_t(child)])
        stack.push_back({child, world[size_t(node)]});
    }
  }
  return world;
}

// reference: AnimationSystem::parseSkinTasks / parseMorphPrimitives (src/gltf_scene_animation.cpp:196-320)
void GltfScene::parseDeformation()
{
  m_skins.clear();
  m_deform.clear();
  m_meshWeights.clear();
  const Value& meshes = m_doc["meshes"];
  for(size_t m = 0; m < meshes.size(); ++m)
  {
    std::vector<float> w;
    const Value&       mw = meshes[m]["weights"];
    for(size_t t = 0; t < mw.size(); ++t)
      w.push_back(float(mw[t].number()));
    m_meshWeights.push_back(std::move(w));
  }
  const Value& skins = m_doc["skins"];
  for(size_t k = 0; k < skins.size(); ++k)
  {
    Skin         sk;
    const Value& joints = skins[k]["joints"];
    for(size_t j = 0; j < joints.size(); ++j)
      sk.joints.push_back(joints[j].integer(-1));
    // a missing, unreadable or short inverseBindMatrices list leaves the remaining joints at identity (as the reference does)
    std::vector<float> ibm;
    if(skins[k]["inverseBindMatrices"].isNumber() && readAccessorFloats(skins[k]["inverseBindMatrices"].integer(-1), 16, ibm))
      for(size_t j = 0; j + 1 <= ibm.size() / 16 && j < sk.joints.size(); ++j)
      {
        mx::mat4 M;
        memcpy(M.m, &ibm[j * 16], sizeof(M.m));
        sk.inverseBind.push_back(M);
      }
    m_skins.push_back(std::move(sk));
  }

  std::vector<int> deformOf(m_primData.size(), -1);
  auto             entry = [&](int rp) -> DeformPrim& {
    if(deformOf[size_t(rp)] < 0)
    {
      deformOf[size_t(rp)] = int(m_deform.size());
      DeformPrim dp;
      dp.renderPrimID = rp;
      dp.meshID       = m_primData[size_t(rp)].meshID;
      m_deform.push_back(std::move(dp));
    }
    return m_deform[size_t(deformOf[size_t(rp)])];
  };
  auto primJson = [&](int rp) -> const Value& {
    const RenderPrimitiveData& d = m_primData[size_t(rp)];
    return meshes[size_t(std::max(d.meshID, 0))]["primitives"][size_t(std::max(d.meshPrimitive, 0))];
  };
  // morph targets: the primitive has targets AND its mesh a non-empty `weights` array (reference :211 -- a file that animates the weights
  // of a mesh without default weights is not morphed, a quirk kept for parity)
  for(size_t rp = 0; rp < m_primData.size(); ++rp)
  {
    const RenderPrimitiveData& d = m_primData[rp];
    if(d.meshID < 0 || d.vertexCount == 0 || d.positions.empty())
      continue;
    const Value& targets = primJson(int(rp))["targets"];
    if(targets.size() == 0 || m_meshWeights[size_t(d.meshID)].empty())
      continue;
    DeformPrim&    dp = entry(int(rp));
    const uint32_t nt = uint32_t(targets.size()), nv = d.vertexCount;
    dp.numTargets     = nt;
    for(size_t t = 0; t < nt; ++t)
    {
      dp.morphNormals  = dp.morphNormals || targets[t].has("NORMAL");
      dp.morphTangents = dp.morphTangents || targets[t].has("TANGENT");
    }
    dp.morphNormals  = dp.morphNormals && !d.normals.empty();  // deltas of a stream the primitive does not have are ignored
    dp.morphTangents = dp.morphTangents && !d.tangents.empty();
    auto readDeltas  = [&](const char* attr, std::vector<float>& out) {
      out.assign(size_t(nv) * 3 * nt, 0.0f);
      for(size_t t = 0; t < nt; ++t)
      {
        std::vector<float> a;
        // a missing, unreadable or short accessor contributes nothing (sparse accessors decode in readAccessorFloats)
        if(targets[t][attr].isNumber() && readAccessorFloats(targets[t][attr].integer(-1), 3, a) && a.size() == size_t(nv) * 3)
          for(size_t i = 0; i < a.size(); ++i)
            out[t * size_t(nv) * 3 + i] = std::isfinite(a[i]) ? a[i] : 0.0f;
      }
    };
    readDeltas("POSITION", dp.posDeltas);
    if(dp.morphNormals)
      readDeltas("NORMAL", dp.nrmDeltas);
    if(dp.morphTangents)
      readDeltas("TANGENT", dp.tanDeltas);
  }
  // skins: one task per unique skinned render primitive; the first render node that uses it supplies the skin and the reference node
  // (reference :270-320).  Instances of the primitive share that one deformation.
  std::set<int> seen;
  for(size_t n = 0; n < m_renderNodes.size(); ++n)
  {
    const int rp   = m_renderNodes[n].renderPrimID;
    const int node = m_renderNodeSource[n].node;
    const int skin = m_doc["nodes"][size_t(node)]["skin"].integer(-1);
    if(skin < 0 || size_t(skin) >= m_skins.size() || rp < 0 || size_t(rp) >= m_primData.size() || !seen.insert(rp).second)
      continue;
    const RenderPrimitiveData& d     = m_primData[size_t(rp)];
    const Value&               attrs = primJson(rp)["attributes"];
    std::vector<float>         j, w;
    if(d.vertexCount == 0 || d.positions.empty() || !attrs["JOINTS_0"].isNumber() || !attrs["WEIGHTS_0"].isNumber()
       || !readAccessorFloats(attrs["JOINTS_0"].integer(-1), 4, j) || !readAccessorFloats(attrs["WEIGHTS_0"].integer(-1), 4, w)
       || j.size() != size_t(d.vertexCount) * 4 || w.size() != size_t(d.vertexCount) * 4)
      continue;  // no usable influences: the primitive keeps its bind pose
    DeformPrim& dp = entry(rp);
    dp.skin        = skin;
    dp.refNode     = node;
    dp.joints.resize(j.size());
    dp.weights.resize(w.size());
    for(size_t i = 0; i < j.size(); ++i)
    {
      dp.joints[i]  = std::isfinite(j[i]) && j[i] >= 0.0f && j[i] <= 65535.0f ? uint16_t(j[i]) : uint16_t(65535);  // (out of range: skipped)
      dp.weights[i] = std::isfinite(w[i]) ? w[i] : 0.0f;
    }
  }
  finalizeDeformation();
}

void GltfScene::finalizeDeformation()
{
  uint32_t joints = 0, weights = 0;
  m_deformPrims.clear();
  for(DeformPrim& dp : m_deform)
  {
    const RenderPrimitiveData& d       = m_primData[size_t(dp.renderPrimID)];
    const bool                 skinned = dp.skin >= 0;
    dp.basePos                         = d.positions;
    dp.baseNrm.clear();
    dp.baseTan.clear();
    if(!d.normals.empty() && (skinned || dp.morphNormals))
      dp.baseNrm = d.normals;
    if(!d.tangents.empty() && (skinned || dp.morphTangents))
      dp.baseTan = d.tangents;
    if(dp.morphTangents && d.tangents.empty())  // (a tangent stream only ever appears, by recomputeTangents; deltas never lose theirs)
      dp.morphTangents = false;
    dp.jointOffset  = joints;
    dp.weightOffset = weights;
    if(skinned)
      joints += uint32_t(m_skins[size_t(dp.skin)].joints.size());
    weights += dp.numTargets;
    MiPtDeformPrimitive p{};
    p.renderPrimID      = dp.renderPrimID;
    p.vertexCount       = d.vertexCount;
    p.basePositions     = dp.basePos.data();
    p.baseNormals       = dp.baseNrm.empty() ? nullptr : dp.baseNrm.data();
    p.baseTangents      = dp.baseTan.empty() ? nullptr : dp.baseTan.data();
    p.joints            = skinned ? dp.joints.data() : nullptr;
    p.weights           = skinned ? dp.weights.data() : nullptr;
    p.numJoints         = skinned ? uint32_t(m_skins[size_t(dp.skin)].joints.size()) : 0;
    p.jointMatrixOffset = dp.jointOffset;
    p.numTargets        = dp.numTargets;
    p.morphWeightOffset = dp.weightOffset;
    p.positionDeltas    = dp.numTargets ? dp.posDeltas.data() : nullptr;
    p.normalDeltas      = dp.numTargets && dp.morphNormals ? dp.nrmDeltas.data() : nullptr;
    p.tangentDeltas     = dp.numTargets && dp.morphTangents && !dp.tanDeltas.empty() ? dp.tanDeltas.data() : nullptr;
    m_deformPrims.push_back(p);
  }
  m_jointMatrices.assign(size_t(joints) * 16, 0.0f);
  m_morphWeights.assign(weights, 0.0f);
  m_deformDesc                  = MiPtDeformDesc{};
  m_deformDesc.prims            = m_deformPrims.data();
  m_deformDesc.numPrims         = int(m_deformPrims.size());
  m_deformDesc.numJointMatrices = int(joints);
  m_deformDesc.numMorphWeights  = int(weights);
  m_deformDesc.jointMatrices    = m_jointMatrices.data();
  m_deformDesc.morphWeights     = m_morphWeights.data();
  updateDeformTables();
}

// The frame tables, in place: joint matrices inverse(world[refNode]) * world[joint] * IBM (reference: src/gltf_scene_animation_vk.cpp:454-478;
// a joint that names no node keeps identity) and the morph weights (mesh.weights, zero beyond its length).
void GltfScene::updateDeformTables()
{
  if(m_deform.empty())
    return;
  std::vector<mx::mat4> world;
  for(const DeformPrim& dp : m_deform)
  {
    if(dp.skin >= 0)
    {
      if(world.empty())
        world = nodeWorldMatrices();
      const Skin&    sk     = m_skins[size_t(dp.skin)];
      const mx::mat4 invRef = mx::inverse(world[size_t(dp.refNode)]);
      for(size_t j = 0; j < sk.joints.size(); ++j)
      {
        mx::mat4 J = mx::identity();
        if(sk.joints[j] >= 0 && size_t(sk.joints[j]) < world.size())
          J = mx::mul(mx::mul(invRef, world[size_t(sk.joints[j])]), j < sk.inverseBind.size() ? sk.inverseBind[j] : mx::identity());
        for(float& c : J.m)
          c = std::isfinite(c) ? c : 0.0f;  // (a singular reference node: no NaN reaches the device, which would refuse the frame)
        memcpy(&m_jointMatrices[(size_t(dp.jointOffset) + j) * 16], J.m, sizeof(J.m));
      }
    }
    if(dp.numTargets)
    {
      const std::vector<float>& mw = m_meshWeights[size_t(dp.meshID)];
      for(uint32_t t = 0; t < dp.numTargets; ++t)
        m_morphWeights[size_t(dp.weightOffset) + t] = t < mw.size() && std::isfinite(mw[t]) ? mw[t] : 0.0f;
    }
  }
}

namespace {
inline void normalize3(float* v)
{
  const float l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  v[0] /= l;
  v[1] /= l;
  v[2] /= l;
}
}  // namespace

// The CPU restatement of k_deform (csrc/device/deform.hip), with the same rules: morph (zero weights skipped, normal / tangent normalised
// when deltas moved them), then skin (influences with w > 0 and a joint inside the skin; the rest skipped; no renormalisation).
int GltfScene::deformOnHost()
{
  int count = 0;
  for(const DeformPrim& dp : m_deform)
  {
    RenderPrimitiveData& d   = m_primData[size_t(dp.renderPrimID)];
    const size_t         nv  = d.vertexCount;
    const bool           hasN = !dp.baseNrm.empty(), hasT = !dp.baseTan.empty();
    const float*         J    = m_jointMatrices.data() + size_t(dp.jointOffset) * 16;
    const uint32_t       nj   = dp.skin >= 0 ? uint32_t(m_skins[size_t(dp.skin)].joints.size()) : 0;
    // normal matrices transpose(inverse(mat3(J))) (the device computes them the same way, mi_pt_update_deformation)
    std::vector<float> N(size_t(nj) * 9);
    for(uint32_t j = 0; j < nj; ++j)
    {
      const float* M = J + size_t(j) * 16;  // column-major: M[c * 4 + r]
      const float  a = M[0], b = M[4], c = M[8], e = M[1], f = M[5], g = M[9], h = M[2], i = M[6], k = M[10];  // rows (a b c) (e f g) (h i k)
      const float  det = a * (f * k - g * i) - b * (e * k - g * h) + c * (e * i - f * h);
      const float  id  = 1.0f / det;
      // cofactor matrix / det == transpose(inverse); stored row-major: N[r * 3 + c]
      float* o = &N[size_t(j) * 9];
      o[0] = (f * k - g * i) * id; o[1] = -(e * k - g * h) * id; o[2] = (e * i - f * h) * id;
      o[3] = -(b * k - c * i) * id; o[4] = (a * k - c * h) * id; o[5] = -(a * i - b * h) * id;
      o[6] = (b * g - c * f) * id; o[7] = -(a * g - c * e) * id; o[8] = (a * f - b * e) * id;
    }
    for(size_t v = 0; v < nv; ++v)
    {
      float p[3] = {dp.basePos[v * 3], dp.basePos[v * 3 + 1], dp.basePos[v * 3 + 2]};
      float n[3] = {0, 0, 0}, t[4] = {0, 0, 0, 0};
      if(hasN)
        memcpy(n, &dp.baseNrm[v * 3], sizeof(n));
      if(hasT)
        memcpy(t, &dp.baseTan[v * 4], sizeof(t));
      if(dp.numTargets)
      {
        for(uint32_t k = 0; k < dp.numTargets; ++k)
        {
          const float w = m_morphWeights[size_t(dp.weightOffset) + k];
          if(w == 0.0f)
            continue;
          const size_t o = (size_t(k) * nv + v) * 3;
          for(int c = 0; c < 3; ++c)
            p[c] += w * dp.posDeltas[o + size_t(c)];
          if(hasN && dp.morphNormals)
            for(int c = 0; c < 3; ++c)
              n[c] += w * dp.nrmDeltas[o + size_t(c)];
          if(hasT && dp.morphTangents)
            for(int c = 0; c < 3; ++c)
              t[c] += w * dp.tanDeltas[o + size_t(c)];
        }
        if(hasN && dp.morphNormals)
          normalize3(n);
        if(hasT && dp.morphTangents)
          normalize3(t);
      }
      if(dp.skin >= 0)
      {
        float sp[3] = {0, 0, 0}, sn[3] = {0, 0, 0}, st[3] = {0, 0, 0};
        for(int i = 0; i < 4; ++i)
        {
          const float    w = dp.weights[v * 4 + size_t(i)];
          const uint32_t j = dp.joints[v * 4 + size_t(i)];
          if(!(w > 0.0f) || j >= nj)
            continue;
          const float* M  = J + size_t(j) * 16;
          const float* Nm = &N[size_t(j) * 9];
          for(int r = 0; r < 3; ++r)
          {
            sp[r] += w * (M[r] * p[0] + M[4 + r] * p[1] + M[8 + r] * p[2] + M[12 + r]);
            sn[r] += w * (Nm[r * 3] * n[0] + Nm[r * 3 + 1] * n[1] + Nm[r * 3 + 2] * n[2]);
            st[r] += w * (M[r] * t[0] + M[4 + r] * t[1] + M[8 + r] * t[2]);
          }
        }
        memcpy(p, sp, sizeof(sp));
        memcpy(n, sn, sizeof(sn));
        memcpy(t, st, sizeof(st));
        normalize3(n);
        normalize3(t);
      }
      memcpy(&d.positions[v * 3], p, sizeof(p));
      if(hasN)
        memcpy(&d.normals[v * 3], n, sizeof(n));
      if(hasT)
        memcpy(&d.tangents[v * 4], t, 3 * sizeof(float));  // (w kept)
    }
    ++count;
  }
  return count;
}

}  // namespace mihost
