// Vertex deformation of skinned and morphed render primitives (deform.hip; C-ABI: mi_pt_set_deformation / mi_pt_update_deformation).
// Reference: shaders/skinning.comp.slang and shaders/morph.comp.slang, dispatched once per primitive and pass by
// AnimationVk::dispatchAnimation (src/gltf_scene_animation_vk.cpp:413-592).  Here ONE launch serves every deforming primitive: each
// primitive's vertex range is padded to whole 256-thread blocks, so a block serves one task and reads its record through the scalar cache.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pt {

constexpr int DEFORM_BLOCK = 256;

enum : uint32_t
{
  DF_NORMALS  = 1u,   // the normal stream is deformed (written)
  DF_TANGENTS = 2u,   // the tangent stream is deformed (xyz written, w kept)
  DF_MORPH_N  = 4u,   // normal deltas: n = normalize(n + sum w dn) before skinning
  DF_MORPH_T  = 8u,   // tangent deltas: t.xyz = normalize(t.xyz + sum w dt)
  DF_SKIN     = 16u,  // four influences per vertex
};

// One deforming primitive (block-uniform: loaded with scalar loads).
struct DeformTask
{
  const float4*   base;          // the rest pose, 3 float4 per vertex in the layout of DevPrim::verts: {p.xyz, n.x} {n.y, n.z, -, -} {t}
  const uint2*    joints;        // 4 x u16 per vertex (DF_SKIN)
  const float4*   weights;       // 4 per vertex (DF_SKIN)
  const float*    posDeltas;     // 3 floats per vertex and target, [t][v] (numTargets > 0)
  const float*    nrmDeltas;     // (DF_MORPH_N)
  const float*    tanDeltas;     // (DF_MORPH_T)
  const float4*   jointTable;    // this primitive's joints, 6 float4 each: rows 0-2 of J (3 x 4), rows 0-2 of N = transpose(inverse(mat3(J)))
  const float*    morphWeights;  // this primitive's numTargets weights
  float*          outPositions;  // the resident streams (DevPrim)
  float*          outNormals;
  float*          outTangents;
  float4*         outVerts;      // DevPrim::verts
  uint32_t        vertexCount, firstBlock, numJoints, numTargets, flags, _pad[3];
};

// tasks / blockTask: device arrays (blockTask[b] = the task of block b); numBlocks = sum of ceil(vertexCount / DEFORM_BLOCK)
void launchDeform(const DeformTask* tasks, const uint32_t* blockTask, uint32_t numBlocks, hipStream_t stream);

}  // namespace pt
