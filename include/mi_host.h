/*
 * mi_host.h — C-ABI of the host-side scene front end (libmi_host.so): the callers of the path-trace hot path.
 * It produces exactly the tables mi_pt_create() / mi_pt_set_environment() / mi_pt_set_frame_info() consume, from the
 * same inputs the reference's application layer uses (a .gltf/.glb file, a Radiance .hdr file, a camera).
 * Reference counterparts: nvvkgltf::Scene::load (src/gltf_scene.cpp:298), GltfRenderer::createHDR
 * (src/renderer.cpp:1982), the SceneFrameInfo fill (src/renderer.cpp:675-705) and PathTracer::setupPushConstant
 * (src/renderer_pathtracer.cpp:1496-1574).
 */
#ifndef MI_HOST_H
#define MI_HOST_H

#include "mi_pt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct MiScene MiScene;
typedef struct MiHdr   MiHdr;

/* reference: nvutils::CameraManipulator::Camera as filled by toManipulatorCamera (src/gltf_camera_utils.hpp:35-55) */
typedef struct MiCamera
{
  float eye[3], center[3], up[3];
  float fovDegrees; /* vertical */
  float znear, zfar;
  int   orthographic;
  float xmag, ymag;
} MiCamera;

MI_PT_API int                  mi_scene_load(const char* path, MiScene** out);
MI_PT_API void                 mi_scene_destroy(MiScene* scene);
MI_PT_API const MiPtSceneDesc* mi_scene_desc(const MiScene* scene);
MI_PT_API int                  mi_scene_num_cameras(const MiScene* scene);
MI_PT_API int                  mi_scene_camera(const MiScene* scene, int index, MiCamera* out);
MI_PT_API void                 mi_scene_bounds(const MiScene* scene, float bmin[3], float bmax[3]);
MI_PT_API uint64_t             mi_scene_num_triangles(const MiScene* scene);
/* recomputeTangents(model, forceCreation, mikktspace) (reference: src/gltf_create_tangent.hpp:28-40, the UI's "Recreate Tangents"
 * items src/ui_renderer.cpp:855-875): simple UV-gradient tangents (mikktspace = 0) or Mikkelsen's tangent space with vertex
 * splitting at UV seams / mirrored UVs.  Returns the number of vertices added by the splitting (>= 0) or a negative MiPtStatus;
 * the MiPtSceneDesc of the scene changes (fetch mi_scene_desc again and re-create the renderer, as the reference re-creates
 * SceneVk / SceneRtx after a split). */
MI_PT_API int                  mi_scene_recompute_tangents(MiScene* scene, int forceCreation, int mikktspace);
/* The raw per-corner output of the Mikkelsen tangent-space computation for a triangle list (4 floats per corner: unit tangent, +1 /
 * -1 orientation), exposed so that tests can compare it with the reference's third_party/MikkTSpace on the same arrays. */
MI_PT_API int                  mi_mikktspace(const float* positions, const float* normals, const float* texCoords, uint32_t numVertices,
                                             const uint32_t* indices, uint32_t numTriangles, float* cornerTangents);

/* Load-time bake for alpha-MASK geometry, this renderer's counterpart of the reference's opacity micro-map bake
 * (src/gltf_scene_omm.cpp; UI switch "Use OMM" src/ui_renderer.cpp): every alpha-MASK triangle is cut adaptively along a
 * subdivisions x subdivisions barycentric grid (rounded up to 2, 4, 8 or 16; 4 is a good default) and the pieces on which the alpha test cannot pass -- no texel a fetch inside them may
 * touch reaches alphaCutoff -- are dropped, so that rays through the empty part of a leaf card meet no candidate at all; the pieces on
 * which it cannot FAIL are moved to the front of their primitive and counted in MiPtRenderPrimitive::opaqueTriangleCount (the walks skip
 * the alpha test for them).  The
 * image is unchanged up to float rounding of the interpolated vertices (and up to sub-ulp T-junction cracks where a merged coarse piece
 * meets refined ones: ~1e-7 of a card's area, csrc/host/alpha_cut.cpp); the selection image (TraceLow treats every triangle as
 * opaque) reports what is seen through a removed part instead of the alpha-tested instance itself.  Returns the number of (sub-)triangles dropped (>= 0)
 * or a negative MiPtStatus; the MiPtSceneDesc changes (fetch mi_scene_desc again, create the renderer afterwards).
 * Skinned and morphed primitives (mi_scene_deformation) are never cut: skinning does not commute with the cut's barycentric
 * re-interpolation of the vertices.  Neither is a material whose alpha state a KHR_animation_pointer channel of any clip animates
 * (alphaCutoff, alphaMode, the base or diffuse colour factor or texture): the classification would hold for one moment of the clip
 * only, and mi_pt_update_materials refuses an alpha change on cut geometry -- so the loader's own animations never meet that refusal. */
MI_PT_API int64_t              mi_scene_cut_alpha(MiScene* scene, int subdivisions);

/* KHR_materials_variants at run time (reference: Scene::setCurrentVariant, src/gltf_scene.cpp:2038-2072; the load resolves variant 0).
 * mi_scene_set_variant rewrites the materialID of the render-node table of mi_scene_desc() in place -- same pointers, same counts -- ready for
 * mi_pt_update_render_nodes(), like the matrices after an animation step.  Per primitive: the material of the first mapping whose `variants`
 * list holds the variant, else max(0, primitive.material), never beyond the material table; every render node made from the primitive gets
 * it, EXT_mesh_gpu_instancing instances included.  Returns the number of render nodes whose material changed (0 is a valid result), or
 * MI_PT_ERR_ARGUMENT with nothing changed: a variant outside [0, mi_scene_num_variants), or a switch that would give a primitive cut by
 * mi_scene_cut_alpha (opaqueTriangleCount > 0) a material with another alpha state (alphaMode, alphaCutoff, base / diffuse alpha factor or
 * texture) -- the cut classified its triangles under the old one and is applied once per loaded scene: load again, switch, then cut.
 * mi_scene_variant_name: MI_PT_ERR_ARGUMENT for an index out of range; the name is truncated to nameCapacity - 1 characters. */
MI_PT_API int                  mi_scene_num_variants(const MiScene* scene);
MI_PT_API int                  mi_scene_variant_name(const MiScene* scene, int index, char* name, int nameCapacity);
MI_PT_API int                  mi_scene_current_variant(const MiScene* scene);
MI_PT_API int                  mi_scene_set_variant(MiScene* scene, int variant);

/* Keyframe animation of node transforms (reference: nvvkgltf::AnimationSystem, src/gltf_scene_animation.hpp:93-122; AnimationInfo
 * src/gltf_scene.hpp:159-189; driven per frame by GltfRenderer::updateAnimation, src/renderer.cpp:2065-2170).  Translation /
 * rotation / scale channels and morph-target `weights` channels with LINEAR, STEP and CUBICSPLINE samplers.
 * KHR_animation_pointer channels (target path "pointer"; SCALAR, VEC2, VEC3 or VEC4 outputs, the three samplers componentwise, the same
 * segment search and keyframe-range rule; reference: src/gltf_animation_pointer.cpp, src/gltf_scene_animation.cpp:373-437) are
 * evaluated for: /materials/i/... (the value goes into the document and material i through the loader's conversion again, so every
 * property the loader reads animates, every KHR_materials_* factor and the KHR_texture_transform offset / scale / rotation of any texture
 * slot included; the material and texture-info tables of mi_scene_desc() are rewritten in place, same pointers and counts);
 * /extensions/KHR_lights_punctual/lights/i/{color, intensity, range, spot/innerConeAngle, spot/outerConeAngle} (the light table, in place;
 * placement stays with the node); /cameras/i/{perspective/{yfov, aspectRatio, znear, zfar}, orthographic/{xmag, ymag, znear, zfar}} (what
 * mi_scene_camera returns; aspectRatio is the viewport's, as in the reference); /nodes/i/extensions/KHR_node_visibility/visible (value != 0,
 * cascading to the children like at load, into renderNodeVisible in place); /nodes/i/{translation, rotation, scale}, routed into the pose
 * code of the core channels -- the reference parses these and then drops them (syncNode, src/gltf_scene_animation.cpp:371-397) although
 * the extension allows them.  `weights` by pointer is not evaluated.  A pointer that resolves to nothing, an index out of range or an
 * output whose width does not fit the property drops the channel at load.
 * mi_scene_update_animation poses the scene at `time` (seconds on the clip's own axis, [start, end] as reported by
 * mi_scene_animation_info) and rewrites the matrices of the render-node table and the light placements of mi_scene_desc() in
 * place -- same pointers, same counts -- ready for mi_pt_update_render_nodes() + mi_pt_update_lights(), and the per-frame tables of
 * mi_scene_deformation() (joint matrices, morph weights), ready for mi_pt_update_deformation().  Returns 1 when something moved
 * (a node, weights or pointer channel covered `time`), 0 when no channel covered `time`, or a negative MiPtStatus -- among them
 * MI_PT_ERR_ARGUMENT, with nothing changed, when a pointer channel would change the number of texture infos (it gives a material a
 * texture it did not have).
 * mi_scene_animation_changes: what the last mi_scene_update_animation changed, i.e. which device updates the caller owes: NODES or
 * VISIBILITY -> mi_pt_update_render_nodes, LIGHTS -> mi_pt_update_lights, DEFORMATION -> mi_pt_update_deformation, MATERIALS ->
 * mi_pt_update_materials, CAMERAS -> mi_scene_camera + the frame info again.  0 after an update that applied no channel. */
enum
{
  MI_SCENE_CHANGED_NODES       = 1,
  MI_SCENE_CHANGED_LIGHTS      = 2,
  MI_SCENE_CHANGED_DEFORMATION = 4,
  MI_SCENE_CHANGED_MATERIALS   = 8,
  MI_SCENE_CHANGED_CAMERAS     = 16,
  MI_SCENE_CHANGED_VISIBILITY  = 32
};
MI_PT_API int                  mi_scene_num_animations(const MiScene* scene);
MI_PT_API int                  mi_scene_animation_info(const MiScene* scene, int index, float* start, float* end, char* name, int nameCapacity);
MI_PT_API int                  mi_scene_update_animation(MiScene* scene, int index, float time);
MI_PT_API int                  mi_scene_animation_changes(const MiScene* scene); /* of the last mi_scene_update_animation */

/* Skins and morph targets (reference: AnimationSystem::parseSkinTasks / parseMorphPrimitives, src/gltf_scene_animation.cpp:196-320).
 * mi_scene_deformation: the tables mi_pt_set_deformation takes, NULL when the scene deforms nothing.  One entry per unique deforming render
 * primitive: skinned when a render node with a skin uses it and it has JOINTS_0 / WEIGHTS_0 (the first such node supplies the skin and the
 * reference node: instances share one deformation), morphed when it has targets AND its mesh has a non-empty `weights` array (the
 * reference's rule, kept).  Its frame arrays (joint matrices inverse(world[refNode]) * world[joint] * IBM, morph weights of mesh.weights
 * padded with zeros) are rewritten in place by every mi_scene_update_animation; the pointers stay valid until mi_scene_recompute_tangents,
 * which rebuilds the tables (re-fetch them).  Nothing is deformed at load.
 * mi_scene_deform_on_host: the CPU restatement of the device kernel (the reference's computeSkinning / computeMorphTargets, with the
 * device shaders' rules where the two differ): writes the posed vertices into the scene's own render-primitive streams, so that a renderer
 * created afterwards -- or the CPU oracle -- sees the pose.  Returns the number of primitives deformed. */
MI_PT_API const MiPtDeformDesc* mi_scene_deformation(const MiScene* scene);
MI_PT_API int                   mi_scene_deform_on_host(MiScene* scene);

MI_PT_API int                    mi_hdr_load(const char* path, MiHdr** out);
MI_PT_API int                    mi_hdr_from_pixels(int width, int height, const float* rgb, MiHdr** out);
MI_PT_API void                   mi_hdr_destroy(MiHdr* hdr);
MI_PT_API const MiPtEnvironment* mi_hdr_env(const MiHdr* hdr);

/* Defaults of `SkyPhysicalParameters{}` (reference: src/renderer.cpp:1328). */
MI_PT_API void mi_default_sky(MiSkyPhysicalParameters* sky);
/* Defaults of PathtracePushConstant + PathTracer members (reference: shaders/shaderio.h:179-196,
 * src/renderer_pathtracer.cpp:60-67). */
MI_PT_API void mi_default_params(MiPathtraceParams* params);
/* Fills view/proj matrices, imageSize, flags (orthographic bit) and zeroes/defaults the rest exactly as
 * GltfRenderer::onRender does with default Settings; also returns pixelAngle and the auto-focus focal distance
 * (reference: src/renderer.cpp:675-705, src/renderer_pathtracer.cpp:1508-1512,1570-1571). */
MI_PT_API void mi_camera_frame_info(const MiCamera* camera, int width, int height, MiSceneFrameInfo* info, float* pixelAngle,
                                    float* focalDistance);

/* Camera rays of a pose under a projection, for mi_pt_set_camera_rays: numSets x height x width MiPtRay records (image order, the sets outermost),
 * tMin 0, tMax FLT_MAX, unit directions (bind with MI_PT_CAMERA_RAYS_UNIT or without).  Computed in double on the matrices of
 * mi_camera_frame_info and rounded once to float.  The sample position of pixel (px, py) in set s is (x, y) = (px + jx, py + jy) with
 * (jx, jy) = jitterXY[2 s], jitterXY[2 s + 1], or (0.5, 0.5) when jitterXY is NULL; row 0 is the top row, as for the built-in camera.  right / up /
 * forward are columns 0, 1 and -2 of viewInv, the origin is its translation.
 *  - MI_PROJECTION_PERSPECTIVE: the built-in camera's ray through (x, y) -- orthographic when the camera is -- with no lens.
 *  - MI_PROJECTION_EQUIRECT: phi = (x / W - 1/2) 2 pi, theta = (1/2 - y / H) pi, d = cos theta sin phi right + sin theta up + cos theta cos phi forward.
 *  - MI_PROJECTION_FISHEYE (equidistant): R = min(W, H) / 2, u = (x - W / 2) / R, v = (H / 2 - y) / R, r = |(u, v)|; r > 1 is a DEAD ray (zero
 *    direction: the pixel stays black and transparent); alpha = r fov / 2, d = sin alpha (u right + v up) / r + cos alpha forward (forward at r = 0).
 *    0 < fisheyeFovDegrees <= 360; ignored by the other projections.
 * *pixelAngle (may be NULL): what belongs into MiPathtraceParams::pixelAngle -- mi_camera_frame_info's, pi / H, fov / min(W, H).
 * MI_PT_ERR_ARGUMENT, with nothing written: a NULL camera or output, width / height / numSets < 1, an unknown projection, a fisheye fov out of range. */
enum { MI_PROJECTION_PERSPECTIVE = 0, MI_PROJECTION_EQUIRECT = 1, MI_PROJECTION_FISHEYE = 2 };
MI_PT_API int mi_camera_rays(const MiCamera* camera, int projection, float fisheyeFovDegrees, int width, int height, const float* jitterXY, int numSets,
                             MiPtRay* hostRays, float* pixelAngle);

/* The mip chain the loader gives every image (one LINEAR 2:1 blit per level, the colour channels of an sRGB image filtered in linear light):
 * levels 1 .. N of a width x height RGBA8 level 0, tightly packed one after the other into outLevels1ToN, level i being max(1,width>>i) x
 * max(1,height>>i), down to 1 x 1.  What MiPtTexture::levels holds for a loaded image, and what mi_pt_update_textures makes on the device with
 * MI_PT_TEXTURE_GENERATE_MIPS.  Returns the number of levels written (0 for a 1 x 1 image); MI_PT_ERR_ARGUMENT for a NULL pointer or a
 * size outside 1 .. 65535.  outLevels1ToN may be NULL to get the count alone. */
MI_PT_API int mi_build_mip_chain(int width, int height, const uint8_t* rgba8, int srgb, uint8_t* outLevels1ToN);
/* The loader's linear-to-sRGB encoder (clamp, IEC 61966-2-1, rounded to 8 bits), over an array: what the mip chain of an sRGB image ends in. */
MI_PT_API void mi_linear_to_srgb8(const float* values, uint64_t count, uint8_t* out);

MI_PT_API const char* mi_host_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
