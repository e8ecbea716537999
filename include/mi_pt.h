/*
 * mi_pt.h — C-ABI of the MI355X-native wavefront path tracer (libmi_pt.so).
 *
 * This is the drop-in boundary for ONE path of nvpro-samples/vk_gltf_renderer: the `PathTracer : BaseRenderer`
 * plugin (reference: src/renderer_base.hpp:33-55, src/renderer_pathtracer.cpp:500-614) and the Slang megakernel it
 * dispatches (reference: shaders/gltf_pathtrace.slang:546-699).  Every entry point below names the reference
 * interface it replaces.  Plain pointers and sizes only; no Vulkan, torch or C++ types cross this line.
 *
 * Conventions: every function returns 0 on success, a negative MiPtStatus on failure, never throws; the caller owns
 * all memory it passes in (it may be freed as soon as the call returns), the library owns all device memory.
 * Not thread-safe per instance (like BaseRenderer::onRender, which runs on the app thread only).
 *
 * Environment: the library's behaviour does not depend on the environment in production.  A set of MI_PT_* variables selects A/B
 * variants and diagnostics ("Run-time switches (all of them)", lists every one with its default); they are read ONCE,
 * in mi_pt_create, into the instance -- a variable that appears or changes later cannot alter a live instance's slot layout, kernels
 * or scene.
 */
#ifndef MI_PT_H
#define MI_PT_H

#include "mi_pt_shaderio.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MI_PT_API __attribute__((visibility("default")))
#else
#define MI_PT_API
#endif

typedef enum MiPtStatus
{
  MI_PT_OK            = 0,
  MI_PT_ERR_ARGUMENT  = -1,
  MI_PT_ERR_NO_DEVICE = -2, /* no HIP device: the product path never falls back to the CPU */
  MI_PT_ERR_HIP       = -3,
  MI_PT_ERR_STATE     = -4,
  MI_PT_ERR_IO        = -5
} MiPtStatus;

/* ------------------------------------------------------------------------------------------------------------------
 * Scene tables handed to the renderer.  They are what `SceneVk` uploads and what `GltfScene` points at in the
 * reference (src/gltf_scene_vk.cpp:330-349 scene-desc, :365 materials, :531 render nodes, :741-870 vertex buffers,
 * :951-1098 textures, :1354-1392 lights), restated with host pointers.
 * ---------------------------------------------------------------------------------------------------------------- */

/* One RenderPrimitive: SoA attribute streams, NULL = attribute absent (reference: VertexBuffers,
 * shaders/gltf_scene_io.h.slang:50-64; indices are always u32 triplets, src/gltf_scene_vk.cpp:816-836; COLOR_0 is
 * packed unorm4x8, :766-798). */
typedef struct MiPtRenderPrimitive
{
  const uint32_t* indices; /* 3 * triangleCount */
  uint32_t        triangleCount;
  uint32_t        vertexCount;
  const float*    positions;  /* 3 floats / vertex */
  const float*    normals;    /* 3 floats / vertex or NULL */
  const uint32_t* colors;     /* unorm4x8 / vertex or NULL */
  const float*    tangents;   /* 4 floats / vertex or NULL */
  const float*    texCoords0; /* 2 floats / vertex or NULL */
  const float*    texCoords1; /* 2 floats / vertex or NULL */
  /* Triangles [0, opaqueTriangleCount) are known to pass their material's alpha test everywhere (alpha-MASK geometry classified at
   * load, mi_scene_cut_alpha -- the OPAQUE state of the reference's opacity micro-maps, src/gltf_scene_omm.cpp): the walks treat them
   * like triangles of a FORCE_OPAQUE instance.  0 = nothing known (every triangle of a non-opaque material is alpha-tested). */
  uint32_t        opaqueTriangleCount;
  uint32_t        reserved; /* 0 */
} MiPtRenderPrimitive;

enum MiPtFilter { MI_FILTER_NEAREST = 0, MI_FILTER_LINEAR = 1 };
enum MiPtWrap { MI_WRAP_REPEAT = 0, MI_WRAP_CLAMP_TO_EDGE = 1, MI_WRAP_MIRRORED_REPEAT = 2 };

/* One glTF *texture* (image + sampler), indexed by GltfTextureInfo.index (reference: src/renderer.cpp:1883-1912
 * bindless array; sampler mapping src/gltf_scene_vk.cpp:909-947; sRGB detection :1102-1154). RGBA8, full mip chain
 * supplied by the caller (the reference blits it at upload, src/gltf_scene_vk.cpp:1247-1347). */
typedef struct MiPtTexture
{
  const uint8_t* const* levels; /* numLevels pointers, level i is max(1,width>>i) x max(1,height>>i) RGBA8 */
  int                   width, height, numLevels;
  int                   srgb; /* 1: texels are sRGB-encoded colour (alpha linear) */
  int                   magFilter, minFilter, mipmapMode; /* MiPtFilter */
  int                   wrapS, wrapT;                     /* MiPtWrap */
} MiPtTexture;

typedef struct MiPtSceneDesc
{
  const MiGltfShadeMaterial* materials;
  int                        numMaterials;
  const MiGltfTextureInfo*   textureInfos; /* [0] is the reserved "no texture" slot */
  int                        numTextureInfos;
  const MiGltfRenderNode*    renderNodes;
  int                        numRenderNodes;
  const uint8_t*             renderNodeVisible; /* numRenderNodes flags or NULL (= all visible); invisible nodes get
                                                   no geometry, reference src/gltf_scene_rtx.cpp:319-323 */
  const MiPtRenderPrimitive* renderPrimitives;
  int                        numRenderPrimitives;
  const MiGltfLight*         lights;
  int                        numLights;
  const MiPtTexture*         textures;
  int                        numTextures;
} MiPtSceneDesc;

/* HDR environment as `nvvk::HdrIbl` prepares it (reference: src/renderer.cpp:1982-2017; consumed at
 * shaders/pathtrace_functions.h.slang:436-447,474-479): lat-long RGBA32F whose alpha holds the sampling pdf, plus the
 * alias table with one entry per texel. */
typedef struct MiPtEnvironment
{
  const float*      rgba; /* width*height*4 */
  const MiEnvAccel* accel; /* width*height */
  int               width, height;
  float             integral; /* luminance integral (HdrIbl::getIntegral) */
} MiPtEnvironment;

typedef struct MiPtCreateOptions
{
  int device;          /* HIP device ordinal */
  int collectCounters; /* 1: kernels export traversal/shading counters (slower) */
  int bvhBuilder;      /* bit 0: 0 = 8-wide compressed BVH (default), 1 = plain BVH2 (A/B, tests);
                        * bit 1: 0 = PLOC clustering over the Morton order (default), 1 = Karras LBVH topology (A/B) */
  int reserved[5];
} MiPtCreateOptions;

/* Work counters behind SURVEY §8(d)'s algorithmic-bytes model; totals since the last mi_pt_reset_stats. */
typedef struct MiPtStats
{
  uint64_t cameraPaths;     /* samples started */
  uint64_t segments;        /* closest-hit rays traced */
  uint64_t shadowRays;      /* shadow rays traced */
  uint64_t nodesClosest;    /* BVH nodes visited by closest-hit rays (needs collectCounters) */
  uint64_t trisClosest;     /* triangles tested by closest-hit rays */
  uint64_t nodesShadow;
  uint64_t trisShadow;
  uint64_t textureTaps;     /* getTexture() calls */
  uint64_t bvhNodeCount;    /* static: nodes in the traversal structure */
  uint64_t bvhTriangleCount;
  uint64_t bvhNodeBytes;    /* S_node */
  uint64_t bvhTriangleBytes;/* S_tri */
  uint64_t surfaceHits;     /* segments that ended on a surface (mesh or infinite plane) and were shaded; segments - surfaceHits
                             * left the scene (environment / backplate).  Needs collectCounters. */
  uint64_t nodesPrimary;    /* node / triangle records fetched by the bounce-0 packet walk: ONE per wave (64 camera rays) and visit, */
  uint64_t trisPrimary;     /* not contained in nodesClosest / trisClosest (which count one per ray and visit) */
} MiPtStats;

/* Per-kernel device time summed over every mi_pt_render_frame since mi_pt_enable_timing(pt, 1), measured with HIP events
 * recorded on the frame's stream around each launch; resolved (one device sync) by mi_pt_get_frame_timing. */
typedef struct MiPtFrameTiming
{
  float totalMs;
  float generateMs;
  float traceClosestMs;
  float sortMs;
  float shadeMs;
  float traceShadowMs;
  float accumulateMs;
  int   traceClosestLaunches;
  int   shadeLaunches;
  int   traceShadowLaunches;
  int   bounceIterations;
  /* the bounce-0 launches on their own (they are also contained in traceClosestMs / shadeMs and the launch counts above) */
  float tracePrimaryMs;   /* k_trace_primary: camera-ray generation + packet walk + end of the paths that leave the scene */
  float shadeFirstMs;     /* k_shade<FIRST> */
  int   tracePrimaryLaunches;
  int   shadeFirstLaunches;
} MiPtFrameTiming;

typedef struct MiPt MiPt;

/* replaces PathTracer::onAttach + SceneVk::create + SceneRtx BLAS/TLAS build
 * (reference: src/renderer_pathtracer.cpp:150-260, src/gltf_scene_vk.cpp:218, src/gltf_scene_rtx.cpp:173-385).
 * Uploads the tables, builds the BVH on the device.  MI_PT_ERR_ARGUMENT: inconsistent tables, a texture pool of 2^32 texels
 * or more, or -- with the default 8-wide BVH -- 2^26 or more flattened triangles (the BVH2 walk, bvhBuilder bit 0, has no such limit). */
MI_PT_API int mi_pt_create(const MiPtSceneDesc* scene, const MiPtCreateOptions* options, MiPt** out);

/* replaces the per-frame instance update of animated / edited scenes: SceneVk::updateRenderNodesBuffer + the TLAS update of
 * SceneRtx (reference: src/gltf_scene_transform_vk.cpp:534-639, src/gltf_scene_rtx.cpp:299-385).  Takes the render-node table
 * again (same length as at creation; matrices, material ids and visibility may have changed) and rebuilds the acceleration
 * structure over the resident geometry ON THE DEVICE -- flatten, Morton sort, PLOC, 8-wide collapse: ~20 ms for 2.8 M triangles,
 * which is why instances are flattened instead of kept behind a two-level structure.  Synchronises with the work in flight;
 * the caller restarts accumulation (MI_PT_FIRST_FRAME) like the reference does after a scene change. */
MI_PT_API int mi_pt_update_render_nodes(MiPt* pt, const MiGltfRenderNode* renderNodes, int numRenderNodes, const uint8_t* renderNodeVisible);

/* replaces the light half of the per-frame scene sync of animated scenes: SceneVk::syncFromScene(eSyncLights) -> uploadLights
 * (reference: src/gltf_scene_vk.hpp:96-103, called from GltfRenderer::updateAnimation, src/renderer.cpp:2118-2131).  Takes the
 * light table again (same length as at creation; placement, colour, intensity, cone may have changed).  Synchronises with the
 * work in flight; the caller restarts accumulation. */
MI_PT_API int mi_pt_update_lights(MiPt* pt, const MiGltfLight* lights, int numLights);

/* replaces the material half of the scene sync of edited and animated scenes: a material marked dirty by the inspector, by undo / redo, by a
 * variant or by a KHR_animation_pointer channel (reference: src/gltf_scene.cpp:1493, src/ui_inspector.cpp:1010) and uploaded record by record by
 * SceneVk (src/gltf_scene_vk.cpp:430-487).  Takes BOTH tables again, complete: numMaterials must be the count at creation, numTextureInfos may
 * differ (slot 0 stays the reserved "no texture" entry).  Textures themselves stay resident: their images and their count cannot change here (images: mi_pt_update_textures).
 * The call brings everything a build derives from the materials -- the instance-flag word of the triangle records, the alpha records, the
 * per-slot texture records, the scene-wide summaries that select kernels and optional buffers -- to the state mi_pt_create would give it on the
 * new tables: the next frames render bit for bit what a fresh instance renders.  It does so in place, without a build (one launch over the
 * triangle slots when an instance flag or an alpha record changed, none for factor or UV-transform changes), except: (1) the transmissive bit
 * of a material changes while the tree holds pre-split references, (2) the BVH2 walk (bvhBuilder bit 0) and a flag or alpha change; those
 * rebuild and count in MiPtAccelInfo::builds.  Refit data stays valid across an in-place update.
 * MI_PT_ERR_ARGUMENT, with NOTHING changed: a count mismatch, a material slot beyond the texture-info table, or a change of the alpha state
 * (alphaMode, alphaCutoff, base / diffuse alpha factor or texture) of a material used by geometry that mi_scene_cut_alpha cut at load
 * (opaqueTriangleCount > 0): that classification held for the old alpha state -- re-cut and re-create.  (mi_pt_create refuses no factor for
 * being non-finite and reads a texture-info `index` outside the textures as "no texture"; so does this call.)
 * Synchronises with the work in flight (queued frames render the old materials); the caller restarts accumulation. */
MI_PT_API int mi_pt_update_materials(MiPt* pt, const MiGltfShadeMaterial* materials, int numMaterials, const MiGltfTextureInfo* textureInfos,
                                     int numTextureInfos);

/* Vertex deformation of animated scenes: glTF skins (JOINTS_0 / WEIGHTS_0, four influences) and morph targets, evaluated on the device
 * into the resident geometry (reference: shaders/skinning.comp.slang, shaders/morph.comp.slang dispatched by AnimationVk::dispatchAnimation,
 * src/gltf_scene_animation_vk.cpp:413-592, from GltfRenderer::updateAnimation, src/renderer.cpp:2065-2170).  Per deforming render primitive:
 *   morph:  p = base + sum_t w_t dp_t (targets with w_t == 0 skipped), n / t.xyz likewise and then normalised (tangent w kept);
 *   skin:   p = sum_i w_i (J_i [p, 1]).xyz, n = normalize(sum_i w_i N_i n), t.xyz = normalize(sum_i w_i mat3(J_i) t.xyz) over the influences
 *           with w_i > 0 and 0 <= j_i < numJoints (an out-of-range joint is skipped; weights are not renormalised), N_i = transpose(inverse(mat3(J_i)));
 *   both:   morph, then skin, in one pass (the reference's two-pass composition, intermediate normalisation included).
 * All pointers are host memory, copied by the call. */
typedef struct MiPtDeformPrimitive
{
  int32_t         renderPrimID;    /* the render primitive whose streams are rewritten */
  uint32_t        vertexCount;     /* must equal the render primitive's */
  const float*    basePositions;   /* 3 floats / vertex: the rest pose (required) */
  const float*    baseNormals;     /* 3 floats / vertex, NULL = the normal stream is not deformed */
  const float*    baseTangents;    /* 4 floats / vertex, NULL = the tangent stream is not deformed */
  const uint16_t* joints;          /* 4 per vertex; NULL = not skinned */
  const float*    weights;         /* 4 per vertex; NULL = not skinned */
  uint32_t        numJoints;       /* joints of the skin: matrices [jointMatrixOffset, + numJoints) of the frame's packed table */
  uint32_t        jointMatrixOffset;
  uint32_t        numTargets;      /* 0 = not morphed; weights [morphWeightOffset, + numTargets) of the frame's packed table */
  uint32_t        morphWeightOffset;
  const float*    positionDeltas;  /* 3 floats per vertex and target, target-major ([t][v]); required when numTargets > 0 */
  const float*    normalDeltas;    /* ... or NULL (then requires baseNormals for non-NULL) */
  const float*    tangentDeltas;   /* ... or NULL (xyz deltas; requires baseTangents for non-NULL) */
} MiPtDeformPrimitive;

typedef struct MiPtDeformDesc
{
  const MiPtDeformPrimitive* prims;
  int                        numPrims;
  int                        numJointMatrices;
  int                        numMorphWeights;
  const float*               jointMatrices; /* this frame's values: 16 floats per matrix, column-major like objectToWorld */
  const float*               morphWeights;  /* this frame's values */
} MiPtDeformDesc;

enum { MI_PT_DEFORM_DEFER_BUILD = 1 }; /* mi_pt_update_deformation: leave the rebuild to the mi_pt_update_render_nodes call that follows */

/* Static upload of the deformation tables, once after mi_pt_create (a copy of base poses, influences and deltas; NULL releases them).
 * Every primitive is validated (render-primitive range, vertexCount equal to the resident primitive's, no duplicates, offsets within
 * the totals): MI_PT_ERR_ARGUMENT otherwise.  Nothing is deformed yet: the geometry stays the one of mi_pt_create. */
MI_PT_API int mi_pt_set_deformation(MiPt* pt, const MiPtDeformDesc* desc);
/* One animated frame: takes the packed joint matrices (numJointMatrices x 16 floats) and morph weights (numMorphWeights floats) of
 * mi_pt_set_deformation's layout, deforms every primitive in ONE launch, then rebuilds the acceleration structure -- unless flags holds
 * MI_PT_DEFORM_DEFER_BUILD, for a caller that calls mi_pt_update_render_nodes next (one rebuild per animated frame).  Non-finite
 * values: MI_PT_ERR_ARGUMENT, nothing changes.  Synchronises with the work in flight (queued frames render the old pose). */
MI_PT_API int mi_pt_update_deformation(MiPt* pt, const float* jointMatrices, const float* morphWeights, int flags);
/* How the acceleration structure follows an animated frame (mi_pt_update_render_nodes, and mi_pt_update_deformation without
 * MI_PT_DEFORM_DEFER_BUILD).  REBUILD (default): a full build, as always.  REFIT: the 8-wide tree keeps its topology and is refitted in
 * place -- the triangle records and boxes of what moved or deformed, then every node's boxes, level by level.  AUTO: refit while the
 * refitted tree's SAH cost stays within rebuildCostRatio x the cost right after the last full build, rebuild otherwise.  An update is
 * refitted only when the 8-wide walk is active (not bvhBuilder bit 0, not MI_PT_HOST_COLLAPSE) and the node table differs from the
 * resident one in objectToWorld / worldToObject alone (same primitives, materials and visibility); every other update rebuilds.  The
 * image does not depend on the tree: a refitted frame renders bit for bit what a fresh instance of the same pose renders.  Instances back
 * at the matrices of the last build get the boxes they were built with; a primitive deformed since that build keeps its refitted boxes
 * (pre-split references: their whole triangles' boxes) until the next build. */
enum
{
  MI_PT_ACCEL_REBUILD = 0,
  MI_PT_ACCEL_REFIT   = 1,
  MI_PT_ACCEL_AUTO    = 2
};
enum { MI_PT_ACCEL_LAST_BUILD = 0, MI_PT_ACCEL_LAST_REFIT = 1 }; /* MiPtAccelInfo::lastUpdate */
/* Unknown mode, or a ratio that is not finite or below 1: MI_PT_ERR_ARGUMENT.  Switching to REFIT or AUTO while the structure holds no
 * refit data rebuilds it once, here (a build), unless no build can keep any (BVH2 walk, MI_PT_HOST_COLLAPSE, an empty or one-reference
 * scene); switching to REBUILD frees the refit data at once.  Synchronises like an update. */
MI_PT_API int mi_pt_set_accel_update(MiPt* pt, int mode, float rebuildCostRatio);
typedef struct MiPtAccelInfo
{
  int32_t  mode;              /* MI_PT_ACCEL_* in force */
  int32_t  lastUpdate;        /* MI_PT_ACCEL_LAST_*: what the last build or update did (an AUTO refit it replaced by a rebuild counts as a build) */
  float    rebuildCostRatio;  /* AUTO's bound */
  int32_t  reserved;
  uint64_t builds;            /* full builds of this instance, the one of mi_pt_create included */
  uint64_t refits;
  double   sahCostAtBuild;    /* SAH cost of the tree right after the last full build, and now (0 without refit data); bit-reproducible: */
  double   sahCost;           /* the same inputs give the same cost, and so the same AUTO decision */
  uint64_t trianglesMoved;    /* triangles whose render node moved or whose primitive deformed, at the last refit */
  uint64_t refitBytes;        /* device memory of the refit data (counted in MiPtMemory::sceneBytes) */
} MiPtAccelInfo;
MI_PT_API int mi_pt_get_accel_info(MiPt* pt, MiPtAccelInfo* info);
/* Resident mode: visibility and material-id changes of mi_pt_update_render_nodes without a build (reference: a hidden instance keeps its
 * TLAS entry with blasAddress = 0, a material change is an instance-flag update, both through the TLAS update path;
 * src/gltf_scene_rtx.cpp:317-334).  Off by default; while it is off every update does what it did before.  In force when enabled AND the
 * structure holds refit data (mode REFIT or AUTO, 8-wide walk, no MI_PT_HOST_COLLAPSE): enabling under REBUILD is accepted and stays inert
 * until mi_pt_set_accel_update allows refits -- either order of the two calls ends in the same state.  In force,
 *  - the tree is built over EVERY render node that owns triangles, hidden ones included, as if all were visible; hidden nodes are then
 *    hidden by a refit: their triangle slots become degenerate records with empty boxes, children with nothing visible below them get the
 *    inverted boxes of empty slots, so the walks skip them.  The slots stay resident: a hidden triangle costs ~130 B of device memory (record,
 *    shade record, two refit boxes; 48 B more in a scene with alpha records), counts towards the 2^26-slot limit of the 8-wide walk and is
 *    counted by mi_pt_get_memory and MiPtStats::bvhTriangleCount.  sahCostAtBuild is the all-visible cost, which AUTO compares with;
 *  - a visibility change is a refit (a node that comes back takes its current matrices and pose; one that stays hidden costs nothing), a
 *    materialID change is a patch of the flag words, alpha records and shade records of that node's slots (the kernel of
 *    mi_pt_update_materials) that follows the scene-wide summaries like mi_pt_update_materials does; one update may carry matrices, visibility
 *    and material ids at once.  The next frames render bit for bit what a fresh instance of the same tables and visibility renders;
 *  - still a build (counted): a renderPrimID change; a material-id change that flips the transmissive bit of a node while the tree holds
 *    pre-split references; AUTO's cost bound.  A build in resident mode builds the resident tree;
 *  - MI_PT_ERR_ARGUMENT, with NOTHING changed: a material-id change that alters the alpha state of geometry mi_scene_cut_alpha cut at load
 *    (opaqueTriangleCount > 0), as in mi_pt_update_materials.
 * Enabling rebuilds once inside the call when it comes into force (a build, like the switch to REFIT); disabling rebuilds once over the
 * visible nodes.  Synchronises like an update. */
MI_PT_API int mi_pt_set_accel_resident(MiPt* pt, int enable);
typedef struct MiPtAccelResidentInfo
{
  int32_t  enabled;            /* as requested */
  int32_t  inForce;            /* the resident tree exists and updates use it */
  uint64_t residentTriangles;  /* triangle slots of the resident tree, hidden ones included (0 while not in force) */
  uint64_t hiddenTriangles;    /* triangles of the hidden render nodes among them (a pre-split triangle holds several slots and counts once) */
  uint64_t visibilityRefits;   /* updates whose visibility change was served by a refit */
  uint64_t materialPatches;    /* updates whose material-id change was served by a patch */
} MiPtAccelResidentInfo;
MI_PT_API int mi_pt_get_accel_resident_info(MiPt* pt, MiPtAccelResidentInfo* info);
/* Reads back the resident streams of a render primitive (vertexCount x 3 / 3 / 4 floats); any pointer may be NULL, and a stream the
 * primitive does not have is left untouched. */
MI_PT_API int mi_pt_read_vertices(MiPt* pt, int renderPrimID, float* positions, float* normals, float* tangents);

/* replaces PathTracer::onDetach (reference: src/renderer_base.hpp:40) */
MI_PT_API int mi_pt_destroy(MiPt* pt);

/* replaces GltfRenderer::createHDR (reference: src/renderer.cpp:1982-2017). NULL env = no HDR loaded. */
MI_PT_API int mi_pt_set_environment(MiPt* pt, const MiPtEnvironment* env);

/* replaces PathTracer::onResize (reference: src/renderer_base.hpp:41): (re)allocates eImgRendered / eImgSelection /
 * depth and the path-state queues; resets accumulation. */
MI_PT_API int mi_pt_resize(MiPt* pt, int width, int height);

/* replaces the vkCmdUpdateBuffer of bFrameInfo / bSkyParams (reference: src/renderer.cpp:675-708).
 * info->visualization: a debug view MI_VIZ_* (mi_pt_shaderio.h; the reference's SceneFrameInfo::visualization).  A colour view replaces the
 * sample of a first ray at its surface hit (misses, selection, depth and guides are the image's); MI_VIZ_CLAY shades with a clay material at
 * every hit; MI_VIZ_OPACITY_MICROMAP colours the closest hit with alpha-tested geometry taken as opaque by whether its alpha is still tested at
 * run time.  0 and any value outside 1..MI_VIZ_COUNT-1 render the image.  The shade counters of mi_pt_get_stats stay zero under a view. */
MI_PT_API int mi_pt_set_frame_info(MiPt* pt, const MiSceneFrameInfo* info);
MI_PT_API int mi_pt_set_sky(MiPt* pt, const MiSkyPhysicalParameters* sky);

/* Image-tile partition for multi-GPU runs (no counterpart in the reference, which is single-GPU): this instance
 * renders only tiles whose index satisfies (tileY * tilesX + tileX) % world == rank; other pixels of the accumulator
 * are left untouched (zero after resize) so a sum-reduce over ranks yields the full frame. world = 1 disables. */
MI_PT_API int mi_pt_set_tile_partition(MiPt* pt, int rank, int world, int tileSize);

/* Render into caller-owned device memory (width*height float4, e.g. a torch tensor) instead of the internal image. */
MI_PT_API int mi_pt_bind_accum(MiPt* pt, void* deviceRGBA32F);
/* The same for the images the denoiser reads next to the accumulator: first-hit albedo and normal guides (width*height float4
 * each) and the frame-0 NDC depth (width*height float).  NULL = the internal image.  A multi-GPU run binds zero-initialised
 * caller memory on every rank, sum-reduces it together with the accumulator (disjoint tiles: sum == gather) and denoises on the
 * rank that holds the sum. */
MI_PT_API int mi_pt_bind_guides(MiPt* pt, void* deviceAlbedoRGBA32F, void* deviceNormalRGBA32F, void* deviceDepthR32F);

/* replaces PathTracer::onRender = setupPushConstant + renderRayQuery (reference: src/renderer_pathtracer.cpp:500-614,
 * :1496-1574, :1404-1431): enqueues ONE frame (params->numSamples spp for every owned pixel, running-mean
 * accumulation, selection id + NDC depth when MI_PT_FIRST_FRAME is set) on `hipStream` (a hipStream_t, NULL = default
 * stream).  Asynchronous unless counters/timing are being collected. */
MI_PT_API int mi_pt_render_frame(MiPt* pt, const MiPathtraceParams* params, void* hipStream);

/* Frames in flight: the result (accumulator, guides, depth, selection) is bit-identical to `numFrames` successive
 * mi_pt_render_frame calls with params->frameCount + f, params->totalSamples + f * numSamples and MI_PT_FIRST_FRAME only
 * on f = 0 -- i.e. the frames GltfRenderer::onRender / updateFrameCounter would issue one after the other
 * (reference: src/renderer.cpp:1939-1977, src/renderer_pathtracer.cpp:1401, :1502-1505) -- but their paths share every
 * wavefront launch, so the short late-bounce queues and the launch overheads are paid once per batch.  Frames only
 * couple through the running mean, which the finish kernel folds in frame order.  1 <= numFrames <= 1024 (and frames x owned pixels < 2^31); the path-state
 * arrays grow (one synchronising reallocation) the first time a larger batch is requested: ~0.3 KB per pixel per frame. */
MI_PT_API int mi_pt_render_frames(MiPt* pt, const MiPathtraceParams* params, int numFrames, void* hipStream);

/* The same batching for a caller that keeps the reference's one-call-per-frame shape (GltfRenderer::onRender -> PathTracer::onRender once per app
 * frame, src/renderer.cpp:713-717, :1939-1977): with depth > 1, mi_pt_render_frame only RECORDS the frame; consecutive frames (frameCount + 1,
 * totalSamples + numSamples, everything else equal, same stream) are held back and issued as one mi_pt_render_frames batch when `depth` of them are
 * pending -- or as soon as any other entry point of this header is called on the instance (mi_pt_synchronize, every read / bind / set / update /
 * denoise / tonemap / statistics call): whatever a caller can observe is what depth 1 would have produced, bit for bit, only later in time.
 * A frame that does not continue the pending run (a reset: MI_PT_FIRST_FRAME, changed parameters) flushes the run and starts a new one.
 * depth 1 (the default) = every call launches its frame at once, as in the reference.  1 <= depth <= 1024. */
MI_PT_API int mi_pt_set_frame_queue(MiPt* pt, int depth);

/* Block until everything enqueued by this instance has finished. */
MI_PT_API int mi_pt_synchronize(MiPt* pt);

/* Read-backs (the reference reads gBuffers images back for screenshots: src/renderer.cpp:557-573). */
MI_PT_API int mi_pt_read_accum(MiPt* pt, float* hostRGBA32F);          /* eImgRendered   */
/* Upload an image INTO eImgRendered (width*height RGBA32F), e.g. to post-process (denoise / tonemap) a frame rendered elsewhere or
 * an accumulation restored from disk; the next frame without MI_PT_FIRST_FRAME continues the running mean from it. */
MI_PT_API int mi_pt_write_accum(MiPt* pt, const float* hostRGBA32F);
/* Denoiser guide layers accumulated while MI_PT_USE_OPTIX_DENOISER is set in params->flags (first-hit albedo.rgb + hit
 * fraction, first-hit shading normal.xyz; reference capture points: shaders/gltf_pathtrace.slang:228-264, the OptiX guide
 * images of src/optix_denoiser.hpp:128-153).  Either pointer may be NULL. */
MI_PT_API int mi_pt_read_guides(MiPt* pt, float* hostAlbedoRGBA32F, float* hostNormalRGBA32F);
MI_PT_API int mi_pt_read_selection(MiPt* pt, uint32_t* hostObjectIds); /* eImgSelection: renderNode+1, 0 = none */
MI_PT_API int mi_pt_read_depth(MiPt* pt, float* hostDepth);            /* NDC depth of frame 0 */
MI_PT_API void* mi_pt_accum_device_ptr(MiPt* pt);

/* a-trous edge-avoiding wavelet denoise of the accumulator using the first-hit albedo/normal guides captured when
 * MI_PT_USE_OPTIX_DENOISER is set (replaces OptiXDenoiser::denoiseImageBuffer I/O contract, reference:
 * src/optix_denoiser.hpp:128-153). Result in hostRGBA32F (may be NULL) and in the internal denoised image. */
MI_PT_API int mi_pt_denoise(MiPt* pt, int iterations, float sigmaColor, float sigmaNormal, float sigmaAlbedo,
                            float* hostRGBA32F, void* hipStream);

/* Variance-guided (SVGF-style) denoise of the accumulator: the same I/O contract as mi_pt_denoise, guided in addition by the
 * per-pixel variance of the mean -- from the second moment of the per-frame pixel luminance that the frames accumulate next to
 * the guides while MI_PT_USE_OPTIX_DENOISER is set (spatial estimate below 4 frames) -- and by the frame-0 depth; albedo is
 * demodulated before and re-applied after filtering.  The temporal half of SVGF is the running mean itself (the camera of a
 * progressive accumulation stands still), so there is no reprojection.  Asynchronous on hipStream unless hostRGBA32F is given. */
MI_PT_API int mi_pt_denoise_svgf(MiPt* pt, int iterations, float sigmaLuminance, float sigmaNormal, float sigmaDepth, float* hostRGBA32F, void* hipStream);

/* Motion vectors and temporal reprojection: the temporal half of SVGF (Schied et al. 2017, section 4.1) for scenes and cameras that move, fed by the
 * reference's first-hit G-buffer -- previous-frame position of the first hit under prevRenderNodeObjectToWorld (shaders/gltf_pathtrace.slang:228-241),
 * pixel-space motion vector with the background as points at infinity (:637-645, shaders/dlss_util.h:63-96), matrices snapshot once per rendered pose
 * (shaders/snapshot_prev_transforms.comp.slang).  It stands where the reference runs DLSS-RR; DLSS itself stays out of scope.
 * Call order per pose: update calls, mi_pt_set_frame_info (prevMVP = the viewProjMatrix of the pose before), a batch with MI_PT_FIRST_FRAME |
 * MI_PT_USE_OPTIX_DENOISER (more frames of the same pose may follow), mi_pt_denoise_temporal ONCE.  INTEGRATION.md, "Temporal reprojection". */

/* The record of the last MI_PT_FIRST_FRAME batch's first hit, four floats per pixel: xyz = world position (the ray direction where the id is 0), w = the
 * BITS of an id: renderNode + 1 on a mesh, 0 for a miss and for the infinite plane, 0xffffffff on the shadow-catcher path (no position).  Pixels another
 * rank owns read 0.  MI_PT_ERR_STATE before the first such batch (and after a resize or a larger mi_pt_render_frames batch, until the next one). */
MI_PT_API int mi_pt_read_first_hit(MiPt* pt, float* hostXYZW);
/* enable != 0: allocates the motion image (16 B per pixel), the history (96 B per pixel: two sets of three 16-byte records) and the previous objectToWorld
 * of every render node (64 B each, initialised to the current ones); from then on every MI_PT_FIRST_FRAME batch is followed, on its stream, by the motion
 * kernel and the snapshot of the matrices.  0 frees all of it.  Accumulator, guides, depth and selection do not depend on the setting. */
MI_PT_API int mi_pt_set_temporal(MiPt* pt, int enable);
/* The motion image of the last MI_PT_FIRST_FRAME batch, four floats per pixel: xy = (prevNDC - currNDC) * 0.5 * resolution in pixels (add to a pixel
 * centre to find where its point was; mesh hits move with their render node only -- skinned or morphed vertices relative to it count under
 * mi_pt_set_vertex_motion alone),
 * z = the NDC depth the point had under prevMVP (1 where the id is 0), w = the id bits as above (0xffffffff: zero motion).
 * MI_PT_ERR_STATE while the feature is off or before the first such batch. */
MI_PT_API int mi_pt_read_motion(MiPt* pt, float* hostRGBA32F);
typedef struct MiPtTemporalParams
{
  int   iterations;     /* a-trous iterations after the temporal stage, 0..8; 0 = the re-modulated temporal stage alone */
  float sigmaLuminance; /* as mi_pt_denoise_svgf */
  float sigmaNormal;
  float sigmaDepth;
  float alpha;          /* weight of the new pose in the illumination: max(alpha, 1 / history length); 0.2 */
  float momentsAlpha;   /* ... in the two luminance moments; 0.2 */
  float maxHistory;     /* the history length saturates here; 32 */
  float normalCos;      /* a history tap is valid when dot(normal then, normal now) >= normalCos ... */
  float depthTolerance; /* ... and its depth agrees with the reprojected one within this, relative */
} MiPtTemporalParams;
MI_PT_API void mi_pt_default_temporal(MiPtTemporalParams* params);
/* mi_pt_denoise_svgf with the temporal stage in front: the history is reprojected along the motion image (four bilinear taps, each valid when it lies
 * inside the image, carries this pixel's id, an agreeing normal and the depth the point had), blended with this pose's demodulated accumulator
 * (history length h = min(h + 1, maxHistory), weight max(alpha, 1 / h); no valid tap: h = 1), the variance comes from the blended luminance moments
 * from h = 4 on (the 7x7 spatial estimate below), then the a-trous iterations and the re-modulation run as in mi_pt_denoise_svgf.  Same I/O contract:
 * result in hostRGBA32F (may be NULL) and in the denoised image (mi_pt_tonemap source 1); alpha passes through.  Call it once per pose: every call
 * advances the history.  MI_PT_ERR_STATE: the feature is off, no first-frame batch since, or a tile partition with world > 1. */
MI_PT_API int mi_pt_denoise_temporal(MiPt* pt, const MiPtTemporalParams* params, float* hostRGBA32F, void* hipStream);
/* Forgets the history: the next mi_pt_denoise_temporal starts from its pose alone.  (mi_pt_resize, mi_pt_set_tile_partition, mi_pt_set_temporal and
 * mi_pt_set_vertex_motion do too.) */
MI_PT_API int mi_pt_reset_history(MiPt* pt);

/* Vertex motion: carries skinned and morphed vertices in the motion image (our own; the reference moves a mesh hit with its render node alone).
 * Off by default, and inert until mi_pt_set_temporal AND mi_pt_set_deformation (or mi_pt_set_vertex_updates) are in force too -- in any order; while it is not
 * in force nothing is allocated and every image, read-back and byte of memory is what it is without it.  In force:
 *   - every MI_PT_FIRST_FRAME batch records, next to the first hit, its triangle (16 B per owned pixel slot, in rendererBytes);
 *   - the object-space positions of the pose rendered before are kept for every deforming render primitive (12 B per vertex, each primitive's array
 *     padded to 16 B, + 32 B per render primitive of the scene + 4 B per deforming one, in sceneBytes), initialised to the resident positions here and by
 *     every mi_pt_set_deformation, and copied from the resident positions on the batch's stream after the motion kernel of a MI_PT_FIRST_FRAME batch --
 *     only when mi_pt_update_deformation (or mi_pt_update_vertices[_device]) ran since the last copy: they follow the RENDERED pose, not the update calls.
 *     The primitives declared by mi_pt_set_vertex_updates count as deforming ones here;
 *   - a mesh hit on such a primitive gets, as its previous world position, prevObjectToWorld x (b0 p0 + b1 p1 + b2 p2): p the previous positions of the
 *     hit triangle's vertices, b the hit's barycentrics.  A triangle whose nine previous floats equal its nine current ones BIT FOR BIT takes the rigid
 *     path instead (a still character, the first pose, an update with unchanged tables), so zero motion stays exactly zero; so do hits on primitives
 *     that do not deform.
 * Flushes the frame queue, synchronises and forgets the history like mi_pt_set_temporal.  enable == 0 frees everything again. */
MI_PT_API int mi_pt_set_vertex_motion(MiPt* pt, int enable);
/* The triangle of the last MI_PT_FIRST_FRAME batch's first hit, four words per pixel in image order: render primitive, triangle index inside it (the whole
 * source triangle, also where the acceleration structure holds pre-split references), the bits of the barycentrics b1 and b2 (b0 = 1 - b1 - b2) the hit's
 * attributes are interpolated with.  The first word is 0xffffffff where the id of mi_pt_read_first_hit is 0 or 0xffffffff, and on pixels another rank
 * owns.  MI_PT_ERR_STATE while vertex motion is not in force or before the first such batch after it came into force. */
MI_PT_API int mi_pt_read_first_hit_triangle(MiPt* pt, uint32_t* hostPrimTriB1B2);
/* The previous-pose positions of a deforming render primitive (vertexCount x 3 floats).  MI_PT_ERR_STATE while vertex motion is not in force,
 * MI_PT_ERR_ARGUMENT for a render primitive that neither the deformation tables deform nor mi_pt_set_vertex_updates declares. */
MI_PT_API int mi_pt_read_previous_positions(MiPt* pt, int renderPrimID, float* positions);

/* ------------------------------------------------------------------------------------------------------------------
 * Caller-driven vertices: new positions (and normals, tangents) for resident render primitives, from host or device memory -- a cloth or
 * soft-body step, a vertex cache, a procedural wave, a mesh a model moves on the same GPU (our own; the reference re-uploads the buffers of a
 * changed primitive).  The counterpart of mi_pt_read_vertices, and the front of the pipeline mi_pt_update_deformation feeds: the in-place
 * refit, the deferred build, the previous positions of vertex motion, queries that see the current pose.
 * A vertex write is exactly the bytes mi_pt_create would upload for the same arrays: the separate position / normal / tangent streams and the
 * interleaved record the shade kernels read.  A stream that is not supplied (and not rebuilt) keeps its bytes.  The frames and queries that
 * follow return, bit for bit, what a fresh instance created from the same tables with these vertices returns. */
enum { MI_PT_VERTICES_RECOMPUTE_NORMALS = 1 }; /* mi_pt_set_vertex_updates flags */
typedef struct MiPtVertexUpdate
{
  int32_t      renderPrimID;
  uint32_t     vertexCount; /* must equal the resident primitive's */
  const float* positions;   /* 3 / vertex, tightly packed, required */
  const float* normals;     /* 3 / vertex or NULL = keep (or rebuild, see flags) */
  const float* tangents;    /* 4 / vertex or NULL = keep */
  uint32_t     reserved[2]; /* 0 */
} MiPtVertexUpdate;
/* Declares, once, which render primitives the caller drives (count 0 or NULL releases the declaration and its tables).  Ids out of range or
 * repeated, a primitive of the deformation tables, a primitive without positions, unknown flag bits: MI_PT_ERR_ARGUMENT, nothing changed
 * (mi_pt_set_deformation in turn refuses a primitive declared here).  With MI_PT_VERTICES_RECOMPUTE_NORMALS the vertex-to-incident-corner
 * table of every declared primitive that has a normal stream is built from the resident index buffer and uploaded: 4 B per corner + 4 B per
 * vertex, in MiPtMemory::sceneBytes, reported as tableBytes (the task tables of the update calls, some tens of bytes per declared primitive
 * + 4 B per 256 vertices, are in sceneBytes too).  Flushes the frame queue and synchronises like mi_pt_set_deformation; nothing moves yet. */
MI_PT_API int mi_pt_set_vertex_updates(MiPt* pt, const int32_t* renderPrimIDs, int count, int flags);
/* New vertices for some or all of the declared primitives; the stream pointers are host memory.  MI_PT_ERR_STATE without a declaration.
 * MI_PT_ERR_ARGUMENT, with nothing changed: an undeclared or repeated primitive, a wrong vertexCount, NULL positions, normals / tangents for
 * a stream the primitive does not have, a non-zero reserved word, flag bits other than MI_PT_DEFORM_DEFER_BUILD, a non-finite component in
 * any supplied array.  All primitives of a call are written by ONE launch.  The arrays are staged through a device buffer allocated by the
 * first call and grown, never shrunk (in rendererBytes from then on).  A primitive declared with MI_PT_VERTICES_RECOMPUTE_NORMALS that has a
 * normal stream and gets normals == NULL has its normals rebuilt by a second launch: per vertex the float32 sum of cross(p1 - p0, p2 - p0) over
 * its incident corners (ascending triangle, then corner; unnormalised, so weighted by area) divided by its length; a vertex whose sum has zero
 * or non-finite length keeps its normal.  Tangents are never rebuilt: a caller whose normal-mapped surface bends supplies them.
 * Then the acceleration structure follows as after mi_pt_update_deformation (mi_pt_set_accel_update) -- unless flags holds
 * MI_PT_DEFORM_DEFER_BUILD, for a caller that calls mi_pt_update_render_nodes next.  Synchronises with the work in flight (queued frames
 * render the old vertices); the caller restarts accumulation. */
MI_PT_API int mi_pt_update_vertices(MiPt* pt, const MiPtVertexUpdate* updates, int numUpdates, int flags);
/* The same over device memory: `updates` itself is host memory, its stream pointers device memory of pt's device (4-byte aligned).  Allocates
 * nothing and makes no host copy of the streams.  The call's device synchronisation covers whatever stream produced the arrays: no stream
 * argument.  The host cannot validate device data, so the kernel rejects per vertex: a vertex with any non-finite supplied component keeps
 * ALL its resident values and is counted (MiPtVertexUpdateInfo::verticesRejected); the call succeeds.  A non-finite position never reaches
 * the refit or the builder. */
MI_PT_API int mi_pt_update_vertices_device(MiPt* pt, const MiPtVertexUpdate* updates, int numUpdates, int flags);
typedef struct MiPtVertexUpdateInfo
{
  uint64_t calls;            /* successful update calls of this instance, both forms */
  uint64_t verticesWritten;  /* vertices they wrote, in total */
  uint64_t verticesRejected; /* vertices the LAST call rejected (always 0 for the host form, which refuses the whole call instead) */
  uint64_t tableBytes;       /* the incident-corner tables of the declaration in force */
} MiPtVertexUpdateInfo;
MI_PT_API int mi_pt_get_vertex_update_info(MiPt* pt, MiPtVertexUpdateInfo* info);

/* ------------------------------------------------------------------------------------------------------------------
 * Texture images of resident textures, from host or device memory -- a video texture, a paint stroke, a texture a model optimises on the same
 * GPU (our own; the reference re-creates the image).  The shape is fixed: size, level count, sRGB flag, filters and wrap modes are those of
 * creation, only texels change; another size is a re-create.  Nothing of the acceleration structure is touched.
 * After a successful call, frames, guides, debug views and queries (the alpha-aware _ex forms included, which read level 0 through the alpha
 * records) return, bit for bit, what a fresh instance returns that was created from the same tables with these images in
 * MiPtTexture::levels; mi_pt_read_texture returns the same bytes for every level.  With MI_PT_TEXTURE_GENERATE_MIPS levels 1.. are made on
 * the device from level 0 and equal, byte for byte, the chain the host loader makes (mi_build_mip_chain, include/mi_host.h).  The bilinear
 * footprints of every updated level are rebuilt (unless MI_PT_DIAG_NO_QUADS left them unbuilt).
 * RGBA32F level 0 (only with GENERATE_MIPS) holds linear values: a colour channel of an sRGB texture is encoded as the loader encodes it
 * (IEC 61966-2-1, rounded to 8 bits), every other channel is round(clamp(v, 0, 1) * 255), halves away from zero; NaN becomes 0.  The mips are
 * then made from the quantised level 0, exactly as for RGBA8 input. */
enum { MI_PT_TEXELS_RGBA8 = 0, MI_PT_TEXELS_RGBA32F = 1 }; /* MiPtTextureUpdate::format */
enum { MI_PT_TEXTURE_GENERATE_MIPS = 1 };                   /* MiPtTextureUpdate::flags */
typedef struct MiPtTextureUpdate
{
  int32_t            texture;       /* index into MiPtSceneDesc::textures */
  int32_t            width, height; /* must equal the resident texture's */
  int32_t            numLevels;     /* without GENERATE_MIPS: must equal the resident count, and levels[] is complete; with it: 1, only levels[0] is read */
  int32_t            format;        /* MI_PT_TEXELS_*; RGBA32F only together with GENERATE_MIPS */
  uint32_t           flags;
  const void* const* levels;        /* level i is max(1,width>>i) x max(1,height>>i) texels, tightly packed */
  uint32_t           reserved[2];   /* 0 */
} MiPtTextureUpdate;
/* New images for some of the textures; `updates` and the level pointers are host memory.  MI_PT_ERR_ARGUMENT, with nothing changed: a texture
 * index out of range or repeated, a wrong size or level count, a NULL level, unknown format or flag bits, RGBA32F without GENERATE_MIPS, a
 * non-zero reserved word -- and a texture that is the alpha source of a material whose geometry mi_scene_cut_alpha cut at load (the base /
 * diffuse texture of a non-OPAQUE material, as mi_pt_update_materials finds it, on a render node whose primitive has opaqueTriangleCount > 0):
 * that classification held for the old alpha; re-cut and re-create.  numUpdates == 0 succeeds.  Level 0 of every texture of the call is
 * written by ONE launch, then one launch per generated level index (at most 15) covers that level of every texture, then the footprints.
 * The images are staged through a device buffer allocated by the first call and grown, never shrunk (in rendererBytes from then on).
 * Flushes the frame queue and synchronises the device like mi_pt_update_materials (queued frames render the old texels); the caller
 * restarts accumulation. */
MI_PT_API int mi_pt_update_textures(MiPt* pt, const MiPtTextureUpdate* updates, int numUpdates);
/* The same over device memory: `updates` and the levels[] arrays are host memory, the level pointers device memory of pt's device, 4-byte
 * aligned (16 for RGBA32F; anything else: MI_PT_ERR_ARGUMENT).  Allocates nothing beyond the small task tables and makes no host copy of the
 * images.  The call's device synchronisation covers whatever stream produced the images: no stream argument. */
MI_PT_API int mi_pt_update_textures_device(MiPt* pt, const MiPtTextureUpdate* updates, int numUpdates);
/* The resident texels of one level, max(1,width>>level) x max(1,height>>level) RGBA8: the counterpart of mi_pt_read_vertices. */
MI_PT_API int mi_pt_read_texture(MiPt* pt, int texture, int level, uint8_t* hostRGBA8);
typedef struct MiPtTextureUpdateInfo
{
  uint64_t calls;           /* successful update calls of this instance, both forms */
  uint64_t texelsWritten;   /* texels they wrote, generated levels included, in total */
  uint64_t levelsGenerated; /* levels made on the device, in total */
  uint64_t launches;        /* kernel launches of the LAST call: ingest, mips, footprints */
} MiPtTextureUpdateInfo;
MI_PT_API int mi_pt_get_texture_update_info(MiPt* pt, MiPtTextureUpdateInfo* info);

/* ------------------------------------------------------------------------------------------------------------------
 * The HDR environment from raw texels, host or device memory -- a video dome, a sky baked per frame, a map a model optimises on the same
 * GPU (our own; the reference re-creates the HdrIbl).  mi_pt_set_environment takes a FINISHED environment: pdf in alpha, alias table,
 * integral, all made by one host thread (mi_hdr_from_pixels).  These calls take the texels alone and make the rest on the device.
 * Resident state after a successful call: rgb = the caller's values, alpha = the sampling pdf, one alias entry per texel, with the host's
 * formulas (HdrEnvironment::buildAccel): importance_i = float(area_row * double(max(r,g,b))), the row areas computed in double on the host
 * and uploaded; total = the double sum of the importances; integral = float(total); alpha = max(r,g,b) * float(1.0 / total).  A map with
 * total <= 0 gets the uniform table: q = 1, alias = i, alpha = float(1 / (4 pi)), integral = 0.
 * The alias table is a prefix-sum construction in double (csrc/device/pt_env_update.h), not Vose's loop: it is a valid table of
 * the same distribution -- the slots q_i + sum of (1 - q_j) over alias_j = i reproduce importance_i / total to float rounding of q --
 * but not the host's table entry by entry; rgb equals the host route's bit for bit, integral within 1 float ulp, alpha within 2.
 * Every floating sum runs in one fixed order: the same texels give the same bytes, from either form, on every call.
 * A size equal to the resident environment's is written in place, nothing is allocated; another size, or no environment, allocates like
 * mi_pt_set_environment.  The scratch (about 12 bytes per texel: the index lists and prefix arrays) is allocated by the first call, grown,
 * never shrunk (in rendererBytes; MiPtEnvironmentUpdateInfo::scratchBytes).
 * Flushes the frame queue and synchronises the device like mi_pt_update_textures (queued frames render the old map; the synchronisation
 * covers whatever stream produced a device image: no stream argument); the caller restarts accumulation. */
typedef struct MiPtEnvironmentUpdate
{
  int32_t     width, height; /* >= 1; width*height <= 2^26 */
  int32_t     channels;      /* 3 (RGB32F) or 4 (RGBA32F, input alpha ignored) */
  uint32_t    flags;         /* 0 */
  const void* pixels;        /* lat-long, row 0 = +Y pole, tightly packed */
  uint32_t    reserved[2];   /* 0 */
} MiPtEnvironmentUpdate;
/* pixels: host memory.  MI_PT_ERR_ARGUMENT, with nothing changed: a NULL pointer, a size or channel count out of range, unknown flags, a
 * non-zero reserved word, a component (alpha apart) that is not finite or is negative.  The texels are staged inside the scratch and the
 * resident map, then the device form's kernels run: both forms leave the same bytes. */
MI_PT_API int mi_pt_update_environment(MiPt* pt, const MiPtEnvironmentUpdate* update);
/* pixels: device memory of pt's device, 4-byte aligned (16 for channels == 4; anything else: MI_PT_ERR_ARGUMENT), read where it lies.  The
 * values cannot be validated: the ingest kernel replaces a non-finite or negative component by 0 and counts the texel in texelsSanitised; a
 * NaN never reaches the sum. */
MI_PT_API int mi_pt_update_environment_device(MiPt* pt, const MiPtEnvironmentUpdate* update);
/* The resident environment, however it was set: width*height RGBA32F texels, as many alias entries, the size, the integral.  Any pointer may
 * be NULL.  MI_PT_ERR_STATE when no environment is resident. */
MI_PT_API int mi_pt_read_environment(MiPt* pt, float* hostRGBA, MiEnvAccel* hostAccel, int* width, int* height, float* integral);
typedef struct MiPtEnvironmentUpdateInfo
{
  uint64_t calls;           /* successful update calls of this instance, both forms */
  uint64_t texelsWritten;   /* texels they wrote, in total */
  uint64_t texelsSanitised; /* LAST call: texels with a component replaced by 0 (device form) */
  uint64_t launches;        /* LAST call: kernel launches */
  uint64_t lightTexels;     /* LAST call: texels with q < 1 (0 for the uniform table) */
  uint64_t heavyTexels;     /* LAST call: texels with q >= 1 (0 for the uniform table) */
  uint64_t scratchBytes;    /* the scratch as it stands */
  float    integral;        /* LAST call */
  uint32_t reserved;
} MiPtEnvironmentUpdateInfo;
MI_PT_API int mi_pt_get_environment_update_info(MiPt* pt, MiPtEnvironmentUpdateInfo* info);

/* ------------------------------------------------------------------------------------------------------------------
 * Ray queries and picking against the resident scene (replaces nvvk::RayPicker over the TLAS: reference src/ui_renderer.cpp:95-150).
 * The rays walk the acceleration structure the frames walk, in its CURRENT state: the pose after mi_pt_update_deformation, the tree after
 * a refit, the visibility and material ids of resident mode.
 *  - Geometry: every triangle of every visible render node, taken as OPAQUE, with no face culling -- the ray flags of the reference's
 *    selection ray (RAY_FLAG_FORCE_OPAQUE, pathtrace_functions.h.slang:813-820) and of the selection pass behind mi_pt_read_selection.
 *    Alpha-tested and transmissive surfaces are hit like any other; hidden nodes are never hit.  (Alpha-aware queries: the _ex calls below.)
 *  - Acceptance: a triangle is accepted iff the walks' ray / triangle test accepts it and tMin < t < tMax.  t is in units of |direction|
 *    (the direction need not be normalised).  Nothing behind the origin is hit: a negative tMin acts as 0.
 *  - MI_PT_QUERY_CLOSEST: the smallest t wins, exact ties go to the smaller (renderNode, triangle) -- the rule of the closest-hit walks.
 *    The record does not depend on the tree: BVH2, the 8-wide tree, a refitted and a freshly built tree return the same 64 bytes.
 *  - MI_PT_QUERY_ANY: the walk stops at the first accepted triangle.  MI_PT_HIT is set iff CLOSEST would set it; WHICH accepted triangle
 *    the record describes is unspecified.
 *  - A miss: flags == 0, renderNode == -1, every other field zero.
 *  - An invalid ray (a non-finite origin or direction component, a zero direction, NaN tMin or tMax) is not walked: flags ==
 *    MI_PT_HIT_INVALID_RAY, renderNode == -1, everything else zero.  The call still succeeds (device rays cannot be validated on the host).
 *  - MI_PT_HIT_FRONT_FACE: the ray met the side the triangle's OBJECT-space winding faces, the bit the shade kernel derives for the same hit:
 *    the sign of the world-space determinant of the ray / triangle test (positive = the world-space winding faces the ray), inverted for a
 *    render node whose objectToWorld mirrors (det < 0: world-space winding is the mirror of object-space winding).
 *  - b1, b2, triangle: of the WHOLE source triangle, also where the tree holds pre-split references (as mi_pt_read_first_hit_triangle).
 *  - materialID: the material the resident records shade the triangle with (max(0, GltfRenderNode::materialID) after variants / patches).
 * Queries leave MiPtStats and the frame timing untouched.  Like every entry point they flush a pending frame queue first. */
typedef struct MiPtRay /* 32 B */
{
  float origin[3];
  float tMin;
  float direction[3];
  float tMax;
} MiPtRay;
typedef struct MiPtRayHit /* 64 B */
{
  float    t;            /* in units of |direction|; zero on a miss */
  float    b1, b2;       /* barycentrics of vertices 1 and 2 of the whole source triangle (b0 = 1 - b1 - b2) */
  uint32_t flags;        /* MI_PT_HIT_* */
  int32_t  renderNode;   /* -1 on a miss */
  int32_t  renderPrimID;
  uint32_t triangle;     /* index inside the render primitive */
  int32_t  materialID;
  float    position[3];  /* fma(t, direction, origin) per component */
  float    reserved0;
  float    normal[3];    /* unit geometric normal of the world-space triangle, turned to face the ray (dot(normal, direction) <= 0) */
  float    reserved1;
} MiPtRayHit;
enum { MI_PT_HIT = 1, MI_PT_HIT_FRONT_FACE = 2, MI_PT_HIT_INVALID_RAY = 4 };
enum { MI_PT_QUERY_CLOSEST = 0, MI_PT_QUERY_ANY = 1 };
/* numRays rays from host memory, numRays records into host memory; synchronises.  The staging buffers are allocated on the first call and
 * grown, never before: an instance that never queries holds no memory for it; afterwards they count in MiPtMemory::rendererBytes.
 * numRays == 0 succeeds.  MI_PT_ERR_ARGUMENT: a negative count, a NULL pointer with a positive count, an unknown mode. */
MI_PT_API int mi_pt_query_rays(MiPt* pt, const MiPtRay* hostRays, int numRays, int mode, MiPtRayHit* hostHits);
/* The same over device memory (numRays x 32 B in, numRays x 64 B out, 16-byte aligned; e.g. torch tensors), asynchronous on hipStream
 * (NULL = the default stream); allocates nothing.  The scene must not be updated while the query is in flight (the update calls synchronise
 * the device, so a caller that issues both from one thread need not care). */
MI_PT_API int mi_pt_query_rays_device(MiPt* pt, const void* deviceRays, int numRays, int mode, void* deviceHits, void* hipStream);
/* Picking: pixelXY holds numPixels (x, y) pairs in continuous pixel coordinates under the current frame info and size; the ray of (x, y) is the
 * camera ray getRay(floor(xy), frac(xy)) with tMin = 0, tMax = infinity, CLOSEST -- so (px + 0.5, py + 0.5) is the selection ray of pixel
 * (px, py), and renderNode + 1 there is what mi_pt_read_selection holds after a first frame.  The tile partition does not matter (every rank
 * holds the whole scene).  MI_PT_ERR_STATE before mi_pt_resize / mi_pt_set_frame_info; a pixel outside the image (or not finite) is
 * MI_PT_ERR_ARGUMENT, with nothing written.  Synchronises; stages like mi_pt_query_rays. */
MI_PT_API int mi_pt_pick(MiPt* pt, const float* pixelXY, int numPixels, MiPtRayHit* hostHits);

/* ------------------------------------------------------------------------------------------------------------------
 * The same queries with options: face culling, alpha-aware acceptance, and the K nearest hits of a ray.  The three calls above keep their
 * contract; mi_pt_default_query_options + an _ex call returns their bytes.  Per candidate triangle, in this order:
 *  1. Acceptance interval: as above -- the walks' ray / triangle test accepts it and tMin < t < tMax.
 *  2. Culling.  MI_PT_QUERY_CULL_MATERIAL rejects a triangle that shows the ray its back (MI_PT_HIT_FRONT_FACE would be clear: object-space
 *     winding, inverted for a mirroring render node) unless its material is double sided, has a thickness or transmits (the instances the frames
 *     trace with culling disabled) -- the rule of the frames' camera rays.  MI_PT_QUERY_CULL_NONE: no triangle is culled.
 *  3. Alpha.  A triangle the frames never alpha-test is accepted untested: alphaMode OPAQUE (glass included), and the triangles
 *     mi_scene_cut_alpha classified opaque.  Otherwise o = the opacity the frames test with: the base-colour (or diffuse) alpha factor x the
 *     level-0 alpha texel (nearest or bilinear by the sampler's magnification filter, no UV transform) x the interpolated vertex-colour alpha;
 *     under alphaMode MASK, 1 if that reaches the material's alphaCutoff and 0 otherwise.
 *      - MI_PT_QUERY_ALPHA_OPAQUE: accepted whatever o is (the contract of the calls above).
 *      - MI_PT_QUERY_ALPHA_CUTOFF: accepted iff o >= blendThreshold.  A MASK surface follows its material's cutoff whatever the threshold, a BLEND
 *        surface the caller's threshold.
 *      - MI_PT_QUERY_ALPHA_STOCHASTIC: accepted iff draw <= o, draw = unit float of xxhash32(xxhash32(seed, i, 0), renderNode, triangle), i the
 *        ray's index in the call -- the closest-hit rule of the frames.  One decision per (ray, triangle), however often the walk meets the
 *        triangle: the same call twice returns the same bytes.
 *     o is computed in float32 with IEEE arithmetic; the frames compile the same text with fast division, so their o may differ in the last place.
 *  - MI_PT_QUERY_CLOSEST / MI_PT_QUERY_ANY: their rules above, over the accepted set.
 *  - MI_PT_QUERY_NEAREST_K: the maxHits accepted DISTINCT triangles with the smallest (t, renderNode, triangle), in ascending order.  Distinct is
 *    by (renderNode, triangle): a triangle the tree holds as several pre-split references appears once.  Unused records are miss records.
 *    maxHits == 1 returns the CLOSEST record.  There is no "more hits exist" flag: the walk culls behind the K-th hit and cannot know.  To
 *    continue, query again with tMin = the last t; this skips what ties exactly with that t.
 *  - Records: maxHits per ray under NEAREST_K, otherwise one; ray i owns records [i * K, (i + 1) * K).  An invalid ray: its first record has
 *    MI_PT_HIT_INVALID_RAY, its others are plain misses.
 *  - Every record is independent of the acceleration structure, bit for bit: BVH2, the 8-wide tree, a refitted tree, resident mode.
 *  - The current state counts, as above; alpha-aware queries see an in-place change of alphaCutoff or of an alpha factor
 *    (mi_pt_update_materials) at once -- on the 8-wide tree without a build: the patch rewrites the alpha records the queries read. */
enum { MI_PT_QUERY_NEAREST_K = 2 }; /* joins MI_PT_QUERY_CLOSEST, MI_PT_QUERY_ANY */
enum { MI_PT_QUERY_ALPHA_OPAQUE = 0, MI_PT_QUERY_ALPHA_CUTOFF = 1, MI_PT_QUERY_ALPHA_STOCHASTIC = 2 };
enum { MI_PT_QUERY_CULL_NONE = 0, MI_PT_QUERY_CULL_MATERIAL = 1 };
enum { MI_PT_QUERY_MAX_HITS = 8 };
typedef struct MiPtQueryOptions /* 32 B */
{
  int32_t  mode;           /* MI_PT_QUERY_* */
  int32_t  alpha;          /* MI_PT_QUERY_ALPHA_* */
  int32_t  cull;           /* MI_PT_QUERY_CULL_* */
  int32_t  maxHits;        /* NEAREST_K: 1..MI_PT_QUERY_MAX_HITS; otherwise 0 or 1 */
  float    blendThreshold; /* CUTOFF: in (0, 1] */
  uint32_t seed;           /* STOCHASTIC */
  int32_t  reserved[2];    /* 0 */
} MiPtQueryOptions;
/* CLOSEST, ALPHA_OPAQUE, CULL_NONE, maxHits 1, blendThreshold 0.5, seed 0 */
MI_PT_API void mi_pt_default_query_options(MiPtQueryOptions* options);
/* mi_pt_query_rays / mi_pt_query_rays_device / mi_pt_pick with options; numRays (numPixels) x K records out.  MI_PT_ERR_ARGUMENT, with nothing
 * written: whatever the plain call refuses, NULL options, an unknown mode / alpha / cull value, maxHits out of range, blendThreshold NaN or
 * outside (0, 1] under CUTOFF, a non-zero reserved word.  The host forms stage numRays x K records (MiPtMemory::rendererBytes).  mi_pt_pick_ex
 * takes every mode; it answers MI_PT_QUERY_ANY with the closest hit (one of the answers ANY allows).  Under non-default options it writes the camera
 * rays out and walks them like mi_pt_query_rays_ex; the kernel that forms them may round a ray differently in the last place than mi_pt_pick's. */
MI_PT_API int mi_pt_query_rays_ex(MiPt* pt, const MiPtRay* hostRays, int numRays, const MiPtQueryOptions* options, MiPtRayHit* hostHits);
MI_PT_API int mi_pt_query_rays_device_ex(MiPt* pt, const void* deviceRays, int numRays, const MiPtQueryOptions* options, void* deviceHits, void* hipStream);
MI_PT_API int mi_pt_pick_ex(MiPt* pt, const float* pixelXY, int numPixels, const MiPtQueryOptions* options, MiPtRayHit* hostHits);

/* ---- caller-supplied camera rays -----------------------------------------------------------------------------------------------------------
 * Any camera model: the frames that follow a bind start their paths from rays the caller gives (a panorama, a fisheye, a light-field slab,
 * probes, the output of a torch model) instead of the pinhole / orthographic camera of MiSceneFrameInfo.  Everything after the first ray is
 * unchanged: shading, next-event estimation, volumes, accumulation, guides, denoise, tonemap, the tile partition, the debug views.
 *  - Layout: numSets x height x width MiPtRay records in image order (row-major, row 0 the top row), the sets outermost.
 *  - Which ray: the path of pixel (px, py) in the frame numbered F = params->frameCount + f (as mi_pt_render_frames numbers frames) takes ray
 *    [(F % numSets) * width * height + py * width + px].  Every sample of a multi-sample frame takes the same ray: anti-aliasing and lens blur
 *    are the caller's -- bind several jittered sets.
 *  - Random stream: sample 0 starts from the built-in camera's seed xxhash32(px, py, F) and discards the draws that camera makes before its
 *    first walk: four (two jitter, two lens) -- two when the current frame info has MI_SCENE_IS_ORTHOGRAPHIC, whose camera has no lens and draws
 *    no lens sample; a later sample continues the stored seed and discards as many.  Together with MI_PT_CAMERA_RAYS_UNIT: binding what
 *    mi_pt_make_camera_rays wrote reproduces the built-in camera's single-sample frames bit for bit -- accumulator, guides, depth, first hit --
 *    on the route that starts frames the same way (the BVH2, or MI_PT_NO_PACKET=1).
 *  - Direction: normalised once (IEEE division and square root); with MI_PT_CAMERA_RAYS_UNIT the bits are used as given.
 *  - tMin / tMax are not read: camera paths are unbounded.  mi_pt_make_camera_rays writes 0 and FLT_MAX, so its output is a valid query input.
 *  - Dead rays: a ray with a non-finite origin or direction component or a zero direction (the queries' invalid-ray rule without its tMin / tMax
 *    part) starts no path -- usable as a mask, e.g. outside a fisheye circle.  Its pixel takes radiance 0 and alpha 0 for that frame, folded into
 *    the running mean like any sample; on a first frame also first-hit id 0, selection 0, depth 1 and zero guides.
 *  - Still MiSceneFrameInfo's: the depth image (first hit through viewProjMatrix), the environment rotation, the backplate, the infinite plane;
 *    mi_pt_pick stays the built-in camera's pick; params->pixelAngle (ray-cone texture footprint) is the caller's, as always.
 *  - Selection image of a first frame: from the set of frame params->frameCount, opaque and unculled on the queries' walk -- at every pixel
 *    renderNode + 1 of mi_pt_query_rays(MI_PT_QUERY_CLOSEST) over the same rays (with tMin 0, tMax FLT_MAX).
 *  - While bound, frames start with a generator kernel and the per-lane walk on both trees, never with the fused packet kernel
 *    (MiPtFrameTiming::tracePrimaryLaunches stays 0); unbinding restores it.
 * mi_pt_set_camera_rays copies the rays (counted in MiPtMemory::rendererBytes: numSets x width x height x 32, freed on unbind / destroy);
 * mi_pt_set_camera_rays_device borrows them: device memory, 16-byte aligned, valid and unchanged while frames that use it are in flight; it
 * allocates nothing.  rays == NULL with numSets == 0: back to the built-in camera.  Both flush the frame queue first.
 * MI_PT_ERR_STATE: before mi_pt_resize; while mi_pt_set_temporal is on (and mi_pt_set_temporal(1) while rays are bound): the motion image
 * assumes the projective camera.  After an mi_pt_resize that changed the size the render calls return MI_PT_ERR_STATE until the caller binds
 * or unbinds again -- there is no silent fall back to the built-in camera.
 * MI_PT_ERR_ARGUMENT, with the binding unchanged: numSets < 1 with a pointer, a pointer with numSets == 0 (or NULL with numSets != 0), unknown flag
 * bits, a device pointer that is not 16-byte aligned. */
enum { MI_PT_CAMERA_RAYS_UNIT = 1 }; /* directions are unit vectors already: used bit for bit, not normalised again */
MI_PT_API int mi_pt_set_camera_rays(MiPt* pt, const MiPtRay* hostRays, int numSets, uint32_t flags);
MI_PT_API int mi_pt_set_camera_rays_device(MiPt* pt, const void* deviceRays, int numSets, uint32_t flags);
/* Writes the rays the built-in camera generates for sample 0 of frames params->frameCount + k, k = 0..numSets-1, for EVERY pixel of the image
 * (whatever the tile partition), from the current frame info and size and params->aperture / focalDistance: origin and direction exactly as the
 * frame's first walk receives them (after jitter, lens and the final normalise), tMin 0, tMax FLT_MAX.  numSets x height x width records.  The
 * device form writes 16-byte aligned device memory on hipStream and allocates nothing.  Both run the frames' own generator kernel through the
 * instance's path queues: order the device form like a render call (the same stream as the frames, or synchronised with them).
 * MI_PT_ERR_STATE before mi_pt_resize / mi_pt_set_frame_info, and on an instance whose rank of the tile partition owns no tile;
 * MI_PT_ERR_ARGUMENT: NULL params or output, numSets < 1, an unaligned device pointer. */
MI_PT_API int mi_pt_make_camera_rays(MiPt* pt, const MiPathtraceParams* params, int numSets, MiPtRay* hostRays);
MI_PT_API int mi_pt_make_camera_rays_device(MiPt* pt, const MiPathtraceParams* params, int numSets, void* deviceRays, void* hipStream);

/* device address of the last denoise result (NULL before the first), valid until the next denoise / resize */
MI_PT_API const void* mi_pt_denoised_device_ptr(MiPt* pt);

/* replaces GltfRenderer::tonemap -> nvshaders::Tonemapper::runCompute (reference: src/renderer.cpp:992-1056): the HDR image
 * (source 0 = the accumulator eImgRendered, 1 = the denoised image of the last mi_pt_denoise, as the reference routes the OptiX
 * output: src/renderer.cpp:1006-1016) -> display-referred RGBA8, the eImgTonemapped image the headless run saves
 * (src/renderer.cpp:557-573).  Alpha passes through.  With tm->autoExposure the metering histogram and the exposure easing run on
 * the device too; dtSeconds is the time since the previous call (< 0: jump to the target).  hostRGBA8 may be NULL (result kept in
 * the internal image, mi_pt_tonemapped_device_ptr). */
MI_PT_API int mi_pt_tonemap(MiPt* pt, const MiTonemapperData* tm, int source, float dtSeconds, uint8_t* hostRGBA8, void* hipStream);
MI_PT_API void* mi_pt_tonemapped_device_ptr(MiPt* pt);
/* the reference's defaults: Filmic, active, exposure / brightness / contrast / saturation 1, vignette 0, autoExposure as given */
MI_PT_API void mi_pt_default_tonemapper(MiTonemapperData* tm, int autoExposure);

/* Device memory held by this instance, in bytes, split the way the reference's benchmark reports it (GltfRenderer::
 * benchmarkMemorySamples, src/renderer.cpp:530-555): "Scene" = geometry, textures, materials, environment and the acceleration
 * structure (SceneVk + SceneRtx trackers); "PathTracer" = everything the renderer owns (path state, queues, images). */
typedef struct MiPtMemory
{
  uint64_t sceneBytes;
  uint64_t rendererBytes;
  uint64_t deviceUsedBytes;  /* whole device, all processes: total - free as the driver reports it */
  uint64_t deviceTotalBytes;
  uint64_t pathStateBytes;   /* the part of rendererBytes that grows with the frames in flight: by-slot path records + the three ray queues (+ candidate pool) */
  uint64_t pathSlots;        /* owned pixel slots x frames in flight the arrays are sized for: pathStateBytes / pathSlots = bytes per path slot */
} MiPtMemory;
MI_PT_API int mi_pt_get_memory(MiPt* pt, MiPtMemory* memory);

MI_PT_API int mi_pt_get_stats(MiPt* pt, MiPtStats* stats);
MI_PT_API int mi_pt_reset_stats(MiPt* pt);
MI_PT_API int mi_pt_enable_timing(MiPt* pt, int enable);
MI_PT_API int mi_pt_get_frame_timing(MiPt* pt, MiPtFrameTiming* timing);

/* Human-readable description of the last failure on this thread ("" if none). */
MI_PT_API const char* mi_pt_last_error(void);
MI_PT_API const char* mi_pt_version(void);
/* Layout version of the public structs of this header.  It is bumped whenever a struct a caller allocates (MiPtMemory, MiPtStats, MiPtFrameTiming,
 * MiPathtraceParams, ...) grows or changes: the library writes every field of the struct it was compiled with, so a caller built against an older
 * header must refuse to run -- `if(mi_pt_abi_version() != MI_PT_ABI_VERSION) fail` right after loading the library.
 * 6: MiPtMemory grew pathStateBytes / pathSlots (round 5); mi_pt_render_frames refuses maxDepth 0; mi_pt_set_frame_queue.
 * 7: MiPtDeformPrimitive / MiPtDeformDesc and the deformation entry points (skins and morph targets on the device).
 * 8: MiPtAccelInfo and the refit entry points (mi_pt_set_accel_update, mi_pt_get_accel_info).
 * 9: MiPtTemporalParams and the motion / temporal entry points (mi_pt_read_first_hit, mi_pt_set_temporal, mi_pt_read_motion, mi_pt_denoise_temporal,
 *    mi_pt_reset_history).  (Still 9: mi_pt_set_vertex_motion, mi_pt_read_first_hit_triangle, mi_pt_read_previous_positions -- new entry points, no
 *    struct a caller allocates changed.  Still 9: MiPtRay / MiPtRayHit and mi_pt_query_rays, mi_pt_query_rays_device, mi_pt_pick -- new types and
 *    entry points, no struct a caller already allocates changed.  Still 9: MiPtQueryOptions and mi_pt_default_query_options, mi_pt_query_rays_ex,
 *    mi_pt_query_rays_device_ex, mi_pt_pick_ex -- again new types and entry points only.  Still 9: MiPtVertexUpdate / MiPtVertexUpdateInfo and
 *    mi_pt_set_vertex_updates, mi_pt_update_vertices, mi_pt_update_vertices_device, mi_pt_get_vertex_update_info -- new types and entry points only.
 *    Still 9: mi_pt_set_camera_rays, mi_pt_set_camera_rays_device, mi_pt_make_camera_rays, mi_pt_make_camera_rays_device -- new entry points only.
 *    Still 9: MiPtTextureUpdate / MiPtTextureUpdateInfo and mi_pt_update_textures, mi_pt_update_textures_device, mi_pt_read_texture,
 *    mi_pt_get_texture_update_info -- new types and entry points only.  Still 9: MiPtEnvironmentUpdate / MiPtEnvironmentUpdateInfo and
 *    mi_pt_update_environment, mi_pt_update_environment_device, mi_pt_read_environment, mi_pt_get_environment_update_info -- new types and
 *    entry points only.) */
#define MI_PT_ABI_VERSION 9
MI_PT_API int mi_pt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MI_PT_H */
