// Host-visible launch interface of the wavefront kernels (pt_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_scene.h"
#include "pt_temporal.h"

namespace pt {

struct LaunchCtx
{
  DevScene        scene;
  FrameConsts     fc;
  const DevScene*    sceneDev;  // device-resident copies of `scene` / `fc` for kernels that hand them to non-inlined helpers
  const FrameConsts* fcDev;
  PathSoA         paths;
  Queues          queues;
  const uint32_t* ownedTiles;
  StatCounters*   stats;
  hipStream_t     stream;
  unsigned        persistentBlocks;
  bool            hasAlpha;
  bool            hasAlphaClosest;  // hasAlpha and some instance needs a real alpha test (not INST_ALPHA_PASSES): the closest-hit walks carry the alpha machinery
  bool            hasTransmissive;  // some instance carries INST_TRANSMISSIVE (ordered shadow transmission needed)
  bool            simpleMaterials;  // no material needs the transmission / clearcoat / sheen / iridescence / anisotropy paths
  bool            wide;  // traverse the 8-wide compressed BVH (scene.bvh8Nodes) instead of the BVH2
  bool            collectCounters;
  bool            shadowDeposit;  // k_trace_shadow MODE 0 / 1 add an unoccluded ray's term where the ray ends; k_shadow_resolve<false> runs for catcher probes only (MI_PT_SHADOW_DEPOSIT)
  int             sortMode;  // per-bounce sort of the generic shade kernel: 0 off, 1 surface hits / others / dead, 2 hits grouped by material too
  bool            visualization;  // fc.frameInfo.visualization is a debug view (1 .. MI_VIZ_COUNT - 1): launchShade runs k_shade_viz
};

void launchBuildShadeRecords(const DevScene& scene, uint32_t numTris, DevShadeTri* out, hipStream_t s);
void launchBuildAlphaRecords(const DevScene& scene, uint32_t numTris, DevAlphaTri* out, hipStream_t s);
// material_update.hip: the flag word of the triangle records and the alpha records of the slots whose render node's byte in `dirty` is set
// (material_patch.h: MATERIAL_PATCH_*); `tris` is scene.tris, writable; alphaTris may be NULL, and so may shadeTris (the material ids of the shade
// records: MATERIAL_PATCH_SHADE)
void launchPatchMaterials(const DevScene& scene, const uint8_t* instFlags, const uint8_t* dirty, DevTri* tris, DevAlphaTri* alphaTris, DevShadeTri* shadeTris,
                          uint32_t numTris, hipStream_t s);
void dumpTraceProfile();  // prints the -DTRACE_PROFILE section timers (no-op in the product build)
void launchBvh8Planes(const uint4* nodes, uint32_t numNodes, float* planes, hipStream_t s);
void launchTextureQuads(const uchar4* texels, uint4* quads, uint32_t offset, int width, int height, int wrapS, int wrapT, hipStream_t s);
void launchResetCounters(const Queues& Q, hipStream_t s);
void launchSkyPrecomp(const MiSkyPhysicalParameters& sky, SkyPrecomp* out, hipStream_t stream);
void launchGenerate(const LaunchCtx& c, int sampleIndex);
void launchTraceClosest(const LaunchCtx& c, int cur);
void launchTracePrimary(const LaunchCtx& c, int sampleIndex);  // bounce 0 of an 8-wide-BVH scene: camera rays generated, packet-walked, misses finished, hits into queue 0
void launchShade(const LaunchCtx& c, int cur, bool first);  // first: bounce 0 (paths still carry k_generate's initial state)
void launchTraceShadow(const LaunchCtx& c, int nxt);  // nxt: active queue the preceding shade launch appended to
void launchFlushSurvivors(const LaunchCtx& c, int cur);  // cur: the active queue the last shade launch appended to (paths alive when the bounce loop stopped)
void launchFinishSample(const LaunchCtx& c, int sampleIndex, float4* accum, float* depth, float4* albedo, float4* normal);
void launchSelection(const LaunchCtx& c, uint32_t* selection);
// caller-supplied camera rays (camera_rays.hip, pt_camera_rays.h).  rays: numSets x height x width records in device memory, 16-byte aligned.
// launchGenerateRays stands where launchGenerate does: queue 0 and its counters, ready for launchTraceClosest; unit: MI_PT_CAMERA_RAYS_UNIT.
// launchSelectionRays: launchSelection over set `set` of the bound rays.  launchExportCameraRays: the built-in camera's sample-0 rays of the
// c.fc.numFrames frames from c.fc.pc.frameCount on, for the pixels of c.ownedTiles (c.fc.numSlots pixel slots), into sets setBase.. of `out`.  It
// runs launchGenerate(c, 0) into c.queues first (c.paths all NULL, c.fc.stateInQueue 0, c.collectCounters false: nothing but queue 0 and its
// counters is written) and needs c.fc.numSlots x c.fc.numFrames <= NSUB x c.queues.subCap.
void launchGenerateRays(const LaunchCtx& c, const MiPtRay* rays, uint32_t numSets, bool unit, int sampleIndex);
void launchSelectionRays(const LaunchCtx& c, const MiPtRay* rays, uint32_t set, uint32_t* selection);
void launchExportCameraRays(const LaunchCtx& c, MiPtRay* out, uint32_t setBase);
// ray queries and picking (query.hip, pt_query.h): one ray per lane over the resident structure (`wide`: the 8-wide tree) under the rules of a
// MiPtQueryOptions (pt_query.h: QueryRules -- face culling, alpha mode, q.maxHits records per ray: hits holds numRays x q.maxHits).  any:
// MI_PT_QUERY_ANY, stop at the first accepted triangle (q.maxHits is 1 then).  The plain entry points are these under queryRulesPlain rules, which
// run kernels of their own.  rays / xy / hits are device memory, 16 / 8 / 16-byte aligned.  launchPickRaysEx forms ray i as the camera ray of the
// continuous pixel position xy[i] under fc.frameInfo / fc.width / fc.height (nothing else of fc is read).  rayScratch: numRays ray records, 16-byte
// aligned, that it writes the camera rays to; not touched, and may be null, under plain rules.
struct QueryRules;
void launchQueryRaysEx(const DevScene& scene, bool wide, bool any, const QueryRules& q, const MiPtRay* rays, uint32_t numRays, MiPtRayHit* hits, hipStream_t s);
void launchPickRaysEx(const DevScene& scene, const FrameConsts& fc, bool wide, const QueryRules& q, const float2* xy, MiPtRay* rayScratch, uint32_t numRays,
                      MiPtRayHit* hits, hipStream_t s);

// a-trous edge-avoiding wavelet filter (denoise.hip)
void launchAtrous(const float4* in, float4* out, const float4* albedo, const float4* normal, int width, int height, int step, float sigmaColor,
                  float sigmaNormal, float sigmaAlbedo, hipStream_t s);

const float4* launchSvgf(const float4* color, const float4* albedo, const float4* normal, const float* depth, float4* bufA, float4* bufB, int width, int height,
                         int iterations, float frames, float sigmaLuminance, float sigmaNormal, float sigmaDepth, hipStream_t s);

// the a-trous iterations + re-modulation of the pass above over an (illumination, variance) image prepared elsewhere (the temporal stage)
const float4* launchSvgfFilter(float4* in, float4* other, const float4* color, const float4* albedo, const float4* normal, const float* depth, int width,
                               int height, int iterations, float sigmaLuminance, float sigmaNormal, float sigmaDepth, hipStream_t s);

// motion vectors and temporal reprojection (temporal.hip, pt_temporal.h).  launchMotionVectors: the motion image of a first-frame batch from its
// first-hit records (by pixel slot), then the snapshot of the render nodes' matrices as the next pose's "previous" ones.  firstHitTri (with
// vmPrims, one record per render primitive) non-NULL: vertex motion -- hits on deforming primitives move with their previous-pose vertices
void launchMotionVectors(const float4* firstHit, const uint4* firstHitTri, const VertexMotionPrim* vmPrims, int numPrims, const uint32_t* ownedTiles,
                         uint32_t numSlots, int tileShift, int width, int height, const MiGltfRenderNode* nodes, float* prevObjectToWorld, int numNodes,
                         const float* viewProj, const float* prevMVP, float4* motion, hipStream_t s);
void launchSnapshotTransforms(const MiGltfRenderNode* nodes, float* prevObjectToWorld, int numNodes, hipStream_t s);
// current resident positions -> previous-pose positions of the deforming primitives `ids` (indices into vmPrims), all in one launch;
// maxVertexCount: the largest vertexCount among them
void launchSnapshotPositions(const VertexMotionPrim* vmPrims, const uint32_t* ids, uint32_t numIds, uint32_t maxVertexCount, hipStream_t s);
void launchSvgfReproject(const float4* color, const float4* albedo, const float4* normal, const float* depth, const float4* motion, const TemporalHistory& in,
                         const TemporalHistory& out, float4* illum, int width, int height, const TemporalConsts& tc, bool haveHistory, hipStream_t s);

// tonemapper (tonemap.hip): optional auto-exposure metering (histogram: 256 u32, autoState: 2 floats) + the curve, RGBA32F -> RGBA8
void launchTonemap(const float4* in, uint32_t* outRgba8, int width, int height, const MiTonemapperData& tm, uint32_t* histogram, float* autoState,
                   float dtSeconds, hipStream_t s);

}  // namespace pt
