// C-ABI of libmi_pt.so (include/mi_pt.h): device resource management and the per-frame wavefront schedule.
// Host counterpart in the reference: PathTracer::{onAttach,onResize,onRender,setupPushConstant,renderRayQuery}
// (src/renderer_pathtracer.cpp:150-260, :500-614, :1404-1431, :1496-1574) plus the uploads of SceneVk / SceneRtx.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mi_pt.h"
#include "bvh_refit.h"
#include "dev_buf.h"
#include "material_patch.h"
#include "pt_build.h"
#include "pt_bvh.h"
#include "pt_bvh8.h"
#include "pt_deform.h"
#include "pt_env_update.h"
#include "pt_texture_update.h"
#include "pt_vertex_update.h"
#include "pt_kernels.h"
#include "pt_query.h"

namespace {

thread_local std::string g_lastError;

int fail(int code, const std::string& msg)
{
  g_lastError = msg;
  return code;
}

#define HIP_TRY(x)                                                                                                       \
  do                                                                                                                    \
  {                                                                                                                     \
    hipError_t e_ = (x);                                                                                                \
    if(e_ != hipSuccess)                                                                                                \
      return fail(MI_PT_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));                                       \
  } while(0)

using pt::DevBuf;

enum TimedKernel { TK_GENERATE, TK_TRACE, TK_SORT, TK_SHADE, TK_SHADOW, TK_ACCUM, TK_PRIMARY, TK_SHADE_FIRST, TK_COUNT };

}  // namespace

// Run-time switches (A/B and diagnostics; INTEGRATION.md lists them): read from the environment ONCE, in mi_pt_create, so that a
// variable that appears or changes later cannot alter an instance's slot layout, kernels or scene in the middle of an accumulation.
struct RunSwitches
{
  int    packetInterval = 1;       // MI_PT_PACKET_INTERVAL  0: per-ray node test in every camera-ray packet
  int    sortMode       = 2;       // MI_PT_SORT             window sort of the generic shade kernel: 0 | 1 | 2
  bool   noPacket       = false;   // MI_PT_NO_PACKET        k_generate + per-lane walk instead of k_trace_primary
  bool   stateBySlot    = false;   // MI_PT_STATE_BY_SLOT    path state gathered by slot in every launch (rounds 1-3) instead of travelling in the queue entry
  bool   traceSpans     = false;   // MI_PT_TRACE_SPANS      synchronising diagnostics
  int    overlapUpTo    = 32;      // MI_PT_OVERLAP          batches up to this many frames run a bounce's shadow stage on a second stream, next to the
                                   //                        following bounce's closest-hit walk (0 = one stream, as in rounds 1-3); same image
  int    overlapMinTris = 200000;  // MI_PT_OVERLAP_MIN_TRIS ... in scenes of at least this many (flattened) triangles
  bool   noPlanes       = false;   // MI_PT_DIAG_NO_PLANES   no float planes for the packet walk
  bool   noOpaqueTris   = false;   // MI_PT_DIAG_NO_OPAQUE_TRIS  alpha-test the OPAQUE class of the alpha cut too
  bool   noQuads        = false;   // MI_PT_DIAG_NO_QUADS    four texel gathers per bilinear tap instead of one footprint
  bool   shadowFarFirst = true;    // MI_PT_SHADOW_FAR_FIRST=0 any-hit shadow walks (k_trace_shadow MODE 0 / 1 / 3: order independent) take a node's children near end first,
                                   //                        as in rounds 1-4.  Default since round 5: from the ray's FAR end -- a ray that starts on a surface wades through the
                                   //                        boxes around its origin, its occluder is usually the large thing at the other end.  Same image bit for bit
                                   //                        (test_shadow_walk_from_the_far_end_changes_no_bit); atrium 604 -> 656, street 623 -> 661 Msamples/s (profiles/r05_staged_ab.txt)
  int    reinsert       = 16;      // MI_PT_REINSERT         reinsertion passes over the BVH2 before the 8-wide collapse at scene build (bvh_reinsert.h); 0 = the tree as clustered.
                                   //                        Same image bit for bit (test_reinsertion_changes_the_tree_not_the_image), a tenth fewer node visits per ray:
                                   //                        atrium 604 -> 633, street 623 -> 680 Msamples/s; both switches: 682 / 727 (profiles/r05_staged_ab.txt)
  int    reinsertUpdate = 0;       // MI_PT_REINSERT_UPDATE  ... at the rebuilds of mi_pt_update_render_nodes: 0, because a moving instance pays them every time and a pass costs
                                   //                        more than half of what the rest of a rebuild costs (2.8 M triangles: rebuild 15.7 ms, + 10 ms per pass;
                                   //                        profiles/r05_sweep_and_rebuild.txt).  A posed scene that is then accumulated for many frames
                                   //                        can ask for them
  int    reinsertRounds = 4;       // MI_PT_REINSERT_ROUNDS  lock / move rounds per pass
  float  splitFactor    = 4.0f;    // MI_PT_SPLIT            triangle pre-splitting (bvh_split.h): a triangle whose box area exceeds this x the scene's mean gets one
                                   //                        reference per part of a recursive bisection of its box; 0 = one reference per triangle (rounds 1-5).  Same image
                                   //                        bit for bit; sliver stand-in of the atrium 30.5 -> 9.5 triangle tests per secondary ray, 419 -> 594 Msamples/s
                                   //                        (0 / 64 / 16 / 4 / 1: 419 / 533 / 590 / 594 / 614; street sliver 679 / 703 / 719 / 723 / 696: profiles/r06_split_ab.txt)
  int    splitMaxDepth  = 8;       // MI_PT_SPLIT_DEPTH      ... at most 2^this references per triangle
  float  splitMinShare  = 0.1f;    // MI_PT_SPLIT_MIN_SHARE  ... only in scenes where triangles above 64 x the mean hold this share of the summed box area (0 = always):
                                   //                        the evenly tessellated stand-ins (share 0 / 0.05) keep their round-5 trees -- splitting perturbs them by -1 %
  bool   collapseGreedy = false;   // MI_PT_COLLAPSE=sah|greedy  how BVH2 subtrees become children of an 8-wide node (anything else: mi_pt_create fails)
  bool   collapseBad    = false;
  bool   hostCollapse   = false;   // MI_PT_HOST_COLLAPSE    collapse on the host (the greedy reference of the device collapse)
  bool   coreTex        = true;    // MI_PT_CORE_TEX=0: A/B switch -- the per-material slot records (pt_scene.h: DevCoreTex) send every fetch the general way
  bool   shadowDeposit  = true;    // MI_PT_SHADOW_DEPOSIT=0: A/B switch -- every shadow ray of the opaque / alpha-tested any-hit walks (k_trace_shadow MODE 0 / 1) leaves its
                                   //                        outcome in its queue entry and k_shadow_resolve adds the terms as a pass of its own, as in rounds 5-6.  Default: the walk
                                   //                        adds an unoccluded ray's term where the ray ends (three float atomics nobody waits for, pt_scene.h: shadowDepositAdd) and
                                   //                        the pass runs for catcher probes only.  Same image bit for bit (tests/test_gpu_shadow_deposit.py)
  int    maxItersDiag   = 0;       // MI_PT_DIAG_MAX_ITERS=N test hook: the bounce loop stops after N iterations whatever is still alive (the truncation a
                                   //                        volume-scatter scene meets at maxDepth * 66 + 512)
  int    failBuildAt    = 0;       // MI_PT_DIAG_FAIL_BUILD=N  test hook: the N-th acceleration REbuild of the instance fails after the old structure is gone
  bool   candPoolSet    = false;   // MI_PT_DIAG_CAND_POOL   entries of the transmissive-candidate pool (tests of the overflow path)
  size_t candPool       = 0;
  void   read()
  {
    auto flag = [](const char* n) { const char* e = getenv(n); return e != nullptr; };
    auto num  = [](const char* n, int d) { const char* e = getenv(n); return e ? atoi(e) : d; };
    packetInterval = num("MI_PT_PACKET_INTERVAL", 1);
    sortMode       = num("MI_PT_SORT", 2);
    noPacket       = flag("MI_PT_NO_PACKET");
    stateBySlot    = flag("MI_PT_STATE_BY_SLOT");
    traceSpans     = flag("MI_PT_TRACE_SPANS");
    overlapUpTo    = num("MI_PT_OVERLAP", 32);
    overlapMinTris = num("MI_PT_OVERLAP_MIN_TRIS", 200000);
    noPlanes       = flag("MI_PT_DIAG_NO_PLANES");
    noOpaqueTris   = flag("MI_PT_DIAG_NO_OPAQUE_TRIS");
    noQuads        = flag("MI_PT_DIAG_NO_QUADS");
    shadowFarFirst = num("MI_PT_SHADOW_FAR_FIRST", 1) != 0;
    reinsert       = std::max(0, num("MI_PT_REINSERT", 16));
    reinsertUpdate = std::max(0, num("MI_PT_REINSERT_UPDATE", 0));
    reinsertRounds = std::max(1, num("MI_PT_REINSERT_ROUNDS", 4));
    if(const char* e = getenv("MI_PT_SPLIT"))
      splitFactor = std::max(0.0f, float(atof(e)));
    if(const char* e = getenv("MI_PT_SPLIT_MIN_SHARE"))
      splitMinShare = std::max(0.0f, float(atof(e)));
    splitMaxDepth  = std::min(std::max(0, num("MI_PT_SPLIT_DEPTH", 8)), 10);  // (bvh_split.h: SPLIT_MAX_DEPTH)
    if(const char* e = getenv("MI_PT_COLLAPSE"))
    {
      collapseGreedy = strcmp(e, "greedy") == 0;
      collapseBad    = !collapseGreedy && strcmp(e, "sah") != 0;  // (a typo must not silently select the other collapse)
    }
    hostCollapse   = flag("MI_PT_HOST_COLLAPSE");
    maxItersDiag   = num("MI_PT_DIAG_MAX_ITERS", 0);
    coreTex        = num("MI_PT_CORE_TEX", 1) != 0;
    shadowDeposit  = num("MI_PT_SHADOW_DEPOSIT", 1) != 0;
    failBuildAt    = num("MI_PT_DIAG_FAIL_BUILD", 0);
    if(const char* e = getenv("MI_PT_DIAG_CAND_POOL"))
    {
      candPoolSet = true;
      candPool    = size_t(strtoull(e, nullptr, 10));
    }
  }
};

struct MiPt
{
  int device = 0;
  int numCUs = 256;
  RunSwitches sw;
  // mi_pt_set_frame_queue: consecutive mi_pt_render_frame calls held back and issued together (flushPending)
  struct FrameQueue
  {
    int               frameQueueDepth = 1;
    int               pendingFrames   = 0;
    MiPathtraceParams pendingFirst{};
    void*             pendingStream   = nullptr;
    // frame k of a batch is the first frame's parameters with frameCount + k and totalSamples + k * numSamples (mi_pt_render_frames): a call joins
    // the pending batch when it is exactly that, on the same stream, and does not start a new accumulation
    bool joins(const MiPathtraceParams& params, void* stream) const
    {
      MiPathtraceParams expect = pendingFirst;
      expect.frameCount += pendingFrames;
      expect.totalSamples += pendingFrames * expect.numSamples;
      expect.flags &= ~MI_PT_FIRST_FRAME;
      expect.mouseCoord[0] = params.mouseCoord[0];
      expect.mouseCoord[1] = params.mouseCoord[1];
      return pendingFrames > 0 && stream == pendingStream && memcmp(&expect, &params, sizeof(expect)) == 0;
    }
  } frameQueue;
  // scene
  DevBuf<MiGltfShadeMaterial> materials;
  DevBuf<MiGltfTextureInfo>   texInfos;
  DevBuf<pt::DevTexRef>       texRefs;
  DevBuf<pt::DevCoreTex>      coreTex;   // 5 per material (pt_scene.h)
  DevBuf<MiGltfRenderNode>    nodes;
  DevBuf<pt::DevPrim>         prims;
  DevBuf<MiGltfLight>         lights;
  DevBuf<pt::DevTexture>      textures;
  DevBuf<uchar4>              texels;
  DevBuf<uint4>               texQuads;  // bilinear footprints, one per texel of the pool (DevScene::texQuads)
  DevBuf<uint8_t>             geometry;  // all index / attribute streams, 16-byte aligned sub-allocations
  DevBuf<uint8_t>             instFlags;
  DevBuf<float>               srgbLut;
  DevBuf<float4>              envPixels;
  DevBuf<MiEnvAccel>          envAccel;
  pt::DevScene                scene{};
  bool                        hasAlpha = false, hasAlphaTest = false, hasVolumeScatter = false, simpleMaterials = true, hasTransmissive = false;
  // device-resident descriptor copies (see k_shade): the scene struct, re-uploaded when the environment changes, and a ring
  // of per-batch frame constants fed from pinned host memory (FrameConstsRing, with the owners of HIP handles at the end)
  DevBuf<pt::DevScene>        sceneDev;
  bool                        sceneDevDirty = true;
  struct SkyConstants
  {
    DevBuf<pt::SkyPrecomp>      skyPre;  // constants of the sky model for `skyPreFor` (k_sky_precomp)
    MiSkyPhysicalParameters     skyPreFor{};
    bool                        skyPreValid = false;
    // The constants are those of `sky`: k_sky_precomp runs only when the parameters changed since it last ran
    int upToDate(const MiSkyPhysicalParameters& sky, hipStream_t stream)
    {
      if(skyPreValid && memcmp(&skyPreFor, &sky, sizeof(sky)) == 0)
        return MI_PT_OK;
      // stream-ordered behind the batches that still read the previous values
      if(!skyPre.ptr)
        HIP_TRY(skyPre.alloc(1));
      pt::launchSkyPrecomp(sky, skyPre.ptr, stream);
      skyPreFor   = sky;
      skyPreValid = true;
      return MI_PT_OK;
    }
  } skyConsts;
  MiPtStats                   staticStats{};
  // host copies of what the acceleration structure is built from, kept so that mi_pt_update_render_nodes can rebuild it
  std::vector<MiGltfRenderNode> hostNodes;
  std::vector<uint8_t>          hostVisible;    // empty = all visible
  std::vector<uint8_t>          matInstFlags;   // per material: INST_FORCE_OPAQUE | INST_CULL_DISABLE | INST_TRANSMISSIVE | INST_ALPHA_PASSES
  std::vector<uint8_t>          matFeatures;    // per material: bit0 volume scatter, bit1 needs the generic shade kernel
  // host copies of the material and texture-info tables and of the resident textures' descriptors: what mi_pt_update_materials diffs a new
  // table against and re-derives texRefs / coreTex from
  std::vector<MiGltfShadeMaterial> hostMaterials;
  std::vector<MiGltfTextureInfo>   hostTexInfos;
  std::vector<pt::DevTexture>      hostTextures;
  DevBuf<uint8_t>               matDirty;       // per render node: pt::MATERIAL_PATCH_* of the material update in progress (k_patch_materials)
  std::vector<uint32_t>         primTriangles;  // per render primitive: triangle count, 0 when it has no usable geometry
  std::vector<pt::DevPrim>      hostPrims;      // the device addresses of every primitive's streams (mi_pt_read_vertices, deformation)
  std::vector<uint32_t>         primVertices;   // per render primitive: vertex count
  // ---- the state that exists only while a feature is in force: one struct per feature, reset by assigning a fresh value (a DevBuf's move
  // assignment releases what it held, in the order of the members), summed by its own bytes()
  // skins and morph targets (mi_pt_set_deformation): static tables, allocated only for a scene that deforms something
  struct Deformation
  {
    DevBuf<uint8_t>        pool;     // base poses, influences, deltas (16-byte aligned sub-allocations)
    DevBuf<pt::DeformTask> tasks;
    DevBuf<uint32_t>       blockTask;
    DevBuf<float4>         joints;   // 6 float4 per joint matrix (pt_deform.h)
    DevBuf<float>          weights;
    int                    jointCount = 0, weightCount = 0;
    uint32_t               blocks = 0;
    bool                   set = false;
    std::vector<int>       primIDs;  // the render primitives the deformation tables deform
    uint64_t               bytes() const { return pool.bytes() + tasks.bytes() + blockTask.bytes() + joints.bytes() + weights.bytes(); }
  } deform;
  // caller-driven vertices (mi_pt_set_vertex_updates): exists only while primitives are declared
  struct VertexUpdates
  {
    bool                          set = false;
    std::vector<int>              primIDs;      // the declared render primitives
    std::vector<uint8_t>          declared;     // per render primitive: declared
    std::vector<size_t>           cornerEnd, corners;  // per render primitive: word offsets of its incident-corner table in `table`, SIZE_MAX = none
    DevBuf<uint32_t>              table;        // the incident-corner tables (MI_PT_VERTICES_RECOMPUTE_NORMALS): per primitive V run ends, then 3 T corners
    DevBuf<pt::VertexUpdateTask>  tasks;        // task tables of an update call, sized for a call that carries every declared primitive
    DevBuf<pt::NormalRebuildTask> normalTasks;
    DevBuf<uint32_t>              blockTask;    // [0, blockCap): the ingest's blocks, [blockCap, 2 blockCap): the rebuild's; the last word: rejected vertices
    size_t                        blockCap = 0;
    uint64_t                      bytes() const { return table.bytes() + tasks.bytes() + normalTasks.bytes() + blockTask.bytes(); }
  } vu;
  DevBuf<uint8_t>               vuStaging;      // the host form's arrays: allocated by the first such call and grown (rendererBytes); outlives a declaration
  MiPtVertexUpdateInfo          vuInfo{};       // the counters of mi_pt_get_vertex_update_info (tableBytes is computed there); they outlive a declaration too
  // ---- texture image updates (mi_pt_update_textures[_device])
  DevBuf<uint8_t>               tuStaging;      // the host form's images: allocated by the first such call and grown (rendererBytes)
  DevBuf<float>                 tuTables;       // decode / encode tables of the mip generator (pt_texture_update.h), made by the first call (sceneBytes)
  MiPtTextureUpdateInfo         tuInfo{};       // the counters of mi_pt_get_texture_update_info
  // ---- environment updates (mi_pt_update_environment[_device])
  DevBuf<uint8_t>               euScratch;      // header, row areas, tile sums, prefix arrays, index lists (pt_env_update.h): grown, never shrunk (rendererBytes)
  float                         envIntegral = 0.0f;  // of the resident environment (mi_pt_read_environment)
  MiPtEnvironmentUpdateInfo     euInfo{};       // the counters of mi_pt_get_environment_update_info (scratchBytes is computed there)
  // ---- the acceleration structure: its arrays, the update policy, what the last build left and the counters, with the rules that tie them
  // together.  What it is built from (nodes, instFlags, hostNodes, hostVisible, primTriangles) and what the kernels see (scene) stay above.
  struct Accel
  {
    DevBuf<float4>              bvhNodes;    // the BVH2 (bvhBuilder bit 0), 4 float4 per node ...
    DevBuf<uint4>               bvh8Nodes;   // ... or the 8-wide BVH collapsed from it, 5 uint4 per node
    DevBuf<float>               bvh8Planes;  // the nodes' planes as floats for the packet walk (DevScene::bvh8Planes)
    DevBuf<pt::DevTri>          bvhTris;     // the triangle records, in the order of whichever of the two is resident
    DevBuf<pt::DevShadeTri>     shadeTris;
    DevBuf<pt::DevAlphaTri>     alphaTris;
    bool                        wide      = true;
    bool                        splitRefs = false;  // the resident tree holds pre-split references (more triangle slots than scene triangles)
    int                         bvhBuilder = 0;
    // acceleration updates (mi_pt_set_accel_update): the mode, and the refit data a build keeps when it is not REBUILD (bvh_refit.hip)
    int                         accelMode = MI_PT_ACCEL_REBUILD;
    float                       accelRatio = 1.5f;
    int                         lastUpdate = MI_PT_ACCEL_LAST_BUILD;
    bool                        switchBuild = false;  // the build of mi_pt_set_accel_update / mi_pt_set_accel_resident is running
    bool                        refitCapable = false; // the last build went through the device collapse: a build in REFIT / AUTO mode keeps refit data
    struct RefitData  // what a build keeps for the refits after it, and a build or a switch to REBUILD drops
    {
      DevBuf<pt::RefitBox>  slotBox, builtBox, nodeBox;  // per slot: current box, box the build filed; per node: its box
      DevBuf<float>         sah;         // per node: its SAH term
      DevBuf<double>        sahPartial;  // the cost reduction (pt::REFIT_SAH_PARTIALS + 1)
      DevBuf<uint8_t>       dirty;       // per render node: pt::REFIT_CLEAN / MOVED / HOME
      std::vector<uint32_t> levels;      // level starts of the node array + the node count; empty = no refit data
      double                sahAtBuild = 0.0, sahNow = 0.0;
      uint64_t              bytes() const { return slotBox.bytes() + builtBox.bytes() + nodeBox.bytes() + sah.bytes() + sahPartial.bytes() + dirty.bytes(); }
    } refit;
    std::vector<MiGltfRenderNode> builtNodes;     // the node table of the last full build
    std::vector<uint8_t>          primDirty;      // per render primitive: deformed since the last acceleration update ...
    std::vector<uint8_t>          primDeformed;   // ... since the last full build
    // resident mode (mi_pt_set_accel_resident): the tree holds the hidden render nodes too, so that visibility is a refit and a material id a patch
    bool                        accelResident = false;  // as requested
    bool                        residentTree  = false;  // the resident structure was built over every render node that owns triangles
    uint64_t                    hiddenTris = 0;         // triangles of the hidden render nodes in it
    int                         accelBuilds = 0;  // acceleration-structure builds of this instance so far (0 while the first one runs)
    uint64_t                    accelRefits = 0, trianglesMoved = 0;
    uint64_t                    visibilityRefits = 0, materialPatches = 0;

    uint64_t bytes() const { return bvhNodes.bytes() + bvh8Nodes.bytes() + bvh8Planes.bytes() + bvhTris.bytes() + shadeTris.bytes() + alphaTris.bytes() + refit.bytes(); }
    // An update can be a refit: the mode allows it and the resident tree is an 8-wide one that kept its refit data
    bool canRefit() const { return accelMode != MI_PT_ACCEL_REBUILD && !refit.levels.empty() && bvh8Nodes.ptr && wide; }
    // No build of this instance keeps refit data (the BVH2 walk, the host collapse): its updates build, and resident mode stays inert
    bool keepsNoRefitData(const RunSwitches& sw) const { return (bvhBuilder & 1) != 0 || sw.hostCollapse; }
    // What a build releases at its head.  The planes and the shade and alpha records are NOT among it: each is replaced when a build next
    // allocates it, so after a build over nothing (every node hidden) the old ones are still held, and still counted by bytes().
    void releaseTree() { bvhNodes.release(); bvhTris.release(); bvh8Nodes.release(); }
    // ... and what a failed build or refit releases: every array
    void releaseAll() { releaseTree(); bvh8Planes.release(); shadeTris.release(); alphaTris.release(); }
  } accel;
  // frame state
  int                     width = 0, height = 0;
  int                     tileRank = 0, tileWorld = 1, tileSize = 64;
  MiSceneFrameInfo        frameInfo{};
  MiSkyPhysicalParameters sky{};
  bool                    haveFrameInfo = false;
  DevBuf<uint32_t>        ownedTiles;
  int                     numSlots = 0, tilesX = 0, tilesY = 0;
  int                     framesCap = 1;  // frames in flight the path/queue arrays are sized for
  size_t                  queueCap  = 0;  // positions of one queue (NSUB x subCap)
  DevBuf<float4>          pathArrays;  // PathSoA::radiance: the one by-slot record every batch needs
  // ... and the by-slot records only some batches need, allocated the first time one does (ensureOptionalPathArrays): `optMisc` + `optPixelSum`
  // multi-sample frames, `optThroughput` (+ optMisc) frames whose state lives by slot (shadow-catcher plane, MI_PT_STATE_BY_SLOT), `optMedium` scenes with
  // volume materials (the generic shade kernel), `optGuides` batches that capture the denoiser guides, `optShadowAux2` shadow-catcher frames
  DevBuf<float4>          optThroughput, optMisc, optMedium, optPixelSum, optGuides, optShadowAux2;
  DevBuf<float4>          firstHit;    // PathSoA::firstHit: per PIXEL slot (frame 0 of a first-frame batch only)
  pt::PathSoA             paths{};
  DevBuf<uint32_t>        queueMem;
  DevBuf<float4>          queuePayload;
  DevBuf<float4>          candPool;   // recorded transmissive shadow candidates (Queues::candPool)
  DevBuf<uint32_t>        candLists;  // candNext + overflow list
  pt::Queues              queues{};
  DevBuf<float4>          accumOwn, albedo, normal, denoiseA, denoiseB;
  float4*                 albedoBound = nullptr;  // caller-owned guide / depth images (mi_pt_bind_guides), NULL = the internal ones
  float4*                 normalBound = nullptr;
  float*                  depthBound  = nullptr;
  float4*                 albedoImg() { return albedoBound ? albedoBound : albedo.ptr; }
  float4*                 normalImg() { return normalBound ? normalBound : normal.ptr; }
  float*                  depthImg() { return depthBound ? depthBound : depth.ptr; }
  float                   accumFrames = 0.0f;  // frames folded into the accumulator (variance of the mean, SVGF pass)
  float                   momentFrames = 0.0f; // frames folded into the luminance second moment (normal.w): only batches rendered with the guides on
                                               // feed it, so it may lag behind accumFrames -- the SVGF pass then falls back to its spatial variance
  const float4*           denoised = nullptr;  // result of the last mi_pt_denoise (one of denoiseA / denoiseB)
  // motion vectors and temporal reprojection (mi_pt_set_temporal; temporal.hip)
  bool                    temporal = false;      // as requested
  bool                    haveFirstHit = false;  // pt->firstHit holds the records of a first-frame batch
  struct Temporal  // what allocTemporal makes at the current size while `temporal` is on
  {
    DevBuf<float4> motion, history;       // history: 2 sets x 3 records x pixels
    DevBuf<float>  prevObjectToWorld;     // 16 floats per render node: the matrices of the pose rendered before
    bool           haveMotion = false, haveHistory = false;
    int            historyCur = 0;        // which of the two history sets the last mi_pt_denoise_temporal wrote
    uint64_t       bytes() const { return motion.bytes() + history.bytes() + prevObjectToWorld.bytes(); }
  } temporalData;
  std::vector<uint32_t>   ownedTilesHost;        // host copy of ownedTiles (mi_pt_read_first_hit)
  // vertex motion (mi_pt_set_vertex_motion): in force while temporal and deform.set (or vu.set) are too (vertexMotionActive); `vm` exists only then.
  // The first-hit triangle records follow the number of pixel slots as well (allocFirstHitTri): a lifetime of their own
  bool                    vertexMotion = false;  // as requested
  bool                    haveFirstHitTri = false;  // a first-frame batch wrote firstHitTri
  DevBuf<uint4>           firstHitTri;           // PathSoA::firstHitTri: per PIXEL slot
  struct VertexMotion
  {
    DevBuf<uint8_t>              prevPositions;    // previous-pose positions of the deforming primitives: 12 B per vertex, each primitive padded to 16 B
    DevBuf<pt::VertexMotionPrim> prims;            // one record per render primitive
    DevBuf<uint32_t>             deformIDs;        // the deforming render primitives (k_snapshot_positions)
    std::vector<size_t>          prevOffset;       // per render primitive: byte offset into prevPositions, SIZE_MAX = does not deform
    uint32_t                     maxVertices = 0;
    bool                         poseDirty = false;  // mi_pt_update_deformation ran since the last snapshot of the positions
    uint64_t                     bytes() const { return prevPositions.bytes() + prims.bytes() + deformIDs.bytes(); }
  } vm;
  DevBuf<uint32_t>        tonemapped, tmHistogram;
  DevBuf<float>           tmAutoState;
  float4*                 accum = nullptr;  // accumOwn.ptr or caller-bound memory
  DevBuf<float>           depth;
  DevBuf<uint32_t>        selection;
  // ray queries and picking (mi_pt_query_rays, mi_pt_pick): staging of the host forms, allocated by the first such call and grown, never before
  DevBuf<MiPtRay>         queryRays;  // (mi_pt_pick stages its pixel positions here: 8 of the 32 bytes per ray)
  DevBuf<MiPtRayHit>      queryHits;
  // caller-supplied camera rays (mi_pt_set_camera_rays, mi_pt_set_camera_rays_device): `cameraRays` non-NULL = bound
  DevBuf<MiPtRay>         cameraRaysOwn;      // the host form's copy; empty under the device form
  const MiPtRay*          cameraRays = nullptr;
  int                     cameraRaySets = 0, cameraRaysWidth = 0, cameraRaysHeight = 0;  // the size they were bound at
  uint32_t                cameraRayFlags = 0;
  // rays bound at another image size: the render calls refuse until the caller binds or unbinds again
  bool                    cameraRaysStale() const { return cameraRays && (cameraRaysWidth != width || cameraRaysHeight != height); }
  static constexpr const char* CAMERA_RAYS_STALE = "mi_pt_render_frame: the bound camera rays were bound at another image size -- bind or unbind them again";
  DevBuf<uint32_t>        allTiles;           // every tile of the image, for mi_pt_make_camera_rays under a tile partition (else ownedTiles is that)
  DevBuf<pt::StatCounters> stats;
  bool                    collectCounters = false;
  hipStream_t             lastStream = nullptr;
  // ---- the owners of the render path's HIP handles.  Each releases its own in its destructor and is never copied; they stand LAST so that
  // mi_pt_destroy releases the handles before the device buffers above (members are destroyed in reverse order): timer, ring, second stream.
  struct ShadowOverlap
  {
    hipStream_t             sideStream = nullptr;                    // the shadow stage of small batches (RunSwitches::overlapUpTo)
    hipEvent_t              evShaded = nullptr, evShadowed = nullptr;  // main -> side after a shade launch, side -> main after the shadow stage
    // The stream and its two events exist, made by the first batch that wants them; false: HIP made none, and the batch keeps one stream
    bool ready()
    {
      return sideStream
             || (hipStreamCreateWithFlags(&sideStream, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&evShaded, hipEventDisableTiming) == hipSuccess
                 && hipEventCreateWithFlags(&evShadowed, hipEventDisableTiming) == hipSuccess);
    }
    // Any early return of a batch (a failed queue poll, a launch error) must not leave shadow-stage work queued on the side stream behind the caller's
    // back: a caller that synchronises its own stream and then resizes or updates would race with kernels still adding into the radiance records.
    // On every exit taken while a shadow stage is outstanding the side stream is drained (error paths only: the ordinary path joins it by event).
    struct SideJoin
    {
      hipStream_t side        = nullptr;
      bool        outstanding = false;
      ~SideJoin()
      {
        if(outstanding && side)
          (void)hipStreamSynchronize(side);
      }
    };
    ShadowOverlap()                                = default;
    ShadowOverlap(const ShadowOverlap&)            = delete;
    ShadowOverlap& operator=(const ShadowOverlap&) = delete;
    ~ShadowOverlap()
    {
      if(sideStream)
        (void)hipStreamDestroy(sideStream);
      if(evShaded)
        (void)hipEventDestroy(evShaded);
      if(evShadowed)
        (void)hipEventDestroy(evShadowed);
    }
  } shadowOverlap;
  struct FrameConstsRing
  {
    static constexpr int        FC_RING = 32;
    DevBuf<pt::FrameConsts>     fcRing;
    pt::FrameConsts*            fcHost = nullptr;  // pinned, FC_RING entries
    hipEvent_t                  fcDone[FC_RING] = {};
    unsigned                    fcCursor = 0;
    // The next slot of the ring (made by the first call) holds `fc` for the batch about to be launched on `stream`: the call waits for the batch
    // that used the slot FC_RING calls ago, then copies stream-ordered.  `dev`: the constants on the device; recordDone(slot, stream) ends the claim
    int claim(const pt::FrameConsts& fc, hipStream_t stream, const pt::FrameConsts** dev, unsigned* slot)
    {
      if(!fcHost)
      {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&fcHost), sizeof(pt::FrameConsts) * FC_RING, hipHostMallocDefault));
        HIP_TRY(fcRing.alloc(FC_RING));
        for(hipEvent_t& e : fcDone)
          HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      }
      const unsigned fcSlot = fcCursor++ % unsigned(FC_RING);
      if(fcCursor > unsigned(FC_RING))
        HIP_TRY(hipEventSynchronize(fcDone[fcSlot]));  // the batch that used this slot FC_RING calls ago must have drained
      fcHost[fcSlot] = fc;
      HIP_TRY(hipMemcpyAsync(fcRing.ptr + fcSlot, fcHost + fcSlot, sizeof(pt::FrameConsts), hipMemcpyHostToDevice, stream));
      *dev  = fcRing.ptr + fcSlot;
      *slot = fcSlot;
      return MI_PT_OK;
    }
    // ... behind the batch's last launch
    int recordDone(unsigned slot, hipStream_t stream)
    {
      HIP_TRY(hipEventRecord(fcDone[slot], stream));
      return MI_PT_OK;
    }
    FrameConstsRing() = default;  // (never copied: DevBuf is move-only)
    ~FrameConstsRing()
    {
      for(hipEvent_t e : fcDone)
        if(e)
          (void)hipEventDestroy(e);
      if(fcHost)
        (void)hipHostFree(fcHost);
    }
  } fcConsts;
  struct LaunchTimer
  {
    bool                    timingEnabled   = false;
    // deferred timing: events are recorded per launch and only resolved in mi_pt_get_frame_timing (no per-frame sync)
    struct Span
    {
      int        kind;
      hipEvent_t a, b;
    };
    std::vector<Span>       pendingSpans;
    size_t                  evCursor = 0;
    MiPtFrameTiming         accTiming{};
    std::vector<hipEvent_t> eventPool;
    // The next event of the pool, which grows when the spans recorded since the last reset() have used them all
    hipEvent_t getEvent()
    {
      if(evCursor >= eventPool.size())
      {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        eventPool.push_back(e);
      }
      return eventPool[evCursor++];
    }
    // `launch` on `stream`, between two events when the timer is on: a span of `kind` (TimedKernel)
    template <typename Launch>
    void timed(hipStream_t stream, int kind, Launch&& launch)
    {
      if(timingEnabled)
      {
        hipEvent_t a = getEvent(), b = getEvent();
        (void)hipEventRecord(a, stream);
        launch();
        (void)hipEventRecord(b, stream);
        pendingSpans.push_back({kind, a, b});
      }
      else
        launch();
    }
    // No span is pending and every event of the pool is free again (accTiming stays)
    void reset()
    {
      pendingSpans.clear();
      evCursor = 0;
    }
    // The pending spans' times go into accTiming, after the device synchronisation of the caller
    void resolve()
    {
      MiPtFrameTiming& t = accTiming;
      for(const Span& sp : pendingSpans)
      {
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, sp.a, sp.b);
        switch(sp.kind)
        {
          case TK_GENERATE: t.generateMs += ms; break;
          case TK_TRACE: t.traceClosestMs += ms; break;
          case TK_SORT: t.sortMs += ms; break;
          case TK_SHADE: t.shadeMs += ms; break;
          case TK_PRIMARY: t.traceClosestMs += ms; t.tracePrimaryMs += ms; break;
          case TK_SHADE_FIRST: t.shadeMs += ms; t.shadeFirstMs += ms; break;
          case TK_SHADOW: t.traceShadowMs += ms; break;
          case TK_ACCUM: t.accumulateMs += ms; break;
          default: t.totalMs += ms; break;
        }
      }
      reset();
    }
    LaunchTimer()                              = default;
    LaunchTimer(const LaunchTimer&)            = delete;
    LaunchTimer& operator=(const LaunchTimer&) = delete;
    ~LaunchTimer()
    {
      for(hipEvent_t e : eventPool)
        (void)hipEventDestroy(e);
    }
  } timer;
};

namespace {

size_t align16(size_t v) { return (v + 15u) & ~size_t(15); }

// log2 of the tile size (a power of two: mi_pt_set_tile_partition)
int tileShiftOf(const MiPt* pt)
{
  int shift = 0;
  while((1 << shift) < pt->tileSize)
    ++shift;
  return shift;
}

// Pixel origin x0 | y0 << 16 of every tile of the image that `rank` of `world` renders (world <= 1: every tile)
std::vector<uint32_t> tileOrigins(const MiPt* pt, int rank, int world)
{
  const int             T = pt->tileSize;
  std::vector<uint32_t> origins;
  for(int t = 0; t < pt->tilesX * pt->tilesY; ++t)
    if(world <= 1 || (t % world) == rank)
      origins.push_back(uint32_t((t % pt->tilesX) * T) | (uint32_t((t / pt->tilesX) * T) << 16));
  return origins;
}

// Width, height and texel count of mip level `l` of a texture (MiPtTexture or pt::DevTexture)
struct LevelExtent
{
  int    w, h;
  size_t texels;
};
template <typename Texture>
LevelExtent levelExtent(const Texture& d, int l)
{
  const int w = std::max(1, int(d.width) >> l), h = std::max(1, int(d.height) >> l);
  return {w, h, size_t(w) * size_t(h)};
}

// The resident environment (envPixels / envAccel; empty = none) as the kernels see it
void publishEnvironment(MiPt* pt, int width, int height)
{
  pt->scene.envPixels = pt->envPixels.ptr;
  pt->scene.envAccel  = pt->envAccel.ptr;
  pt->scene.envWidth  = width;
  pt->scene.envHeight = height;
  pt->sceneDevDirty   = true;
}

// The host copy of the node table and the visibility flags (NULL = all visible) that the next build or refit reads
void keepNodeTable(MiPt* pt, const MiGltfRenderNode* renderNodes, int numRenderNodes, const uint8_t* renderNodeVisible)
{
  pt->hostNodes.assign(renderNodes, renderNodes + numRenderNodes);
  if(renderNodeVisible)
    pt->hostVisible.assign(renderNodeVisible, renderNodeVisible + numRenderNodes);
  else
    pt->hostVisible.clear();
}

// Diagnostics: wall time of the phases of the scene build and of every update on stderr.  The switch is read from the
// environment once; tools/build_time.py and tools/time_env_update.py parse the lines.
using BuildClock = std::chrono::steady_clock;
bool buildTiming()
{
  static const bool on = getenv("MI_PT_BUILD_TIMING") != nullptr;
  return on;
}
void printBuildTiming(const char* what, BuildClock::time_point since, int decimals = 2)
{
  if(buildTiming())
    fprintf(stderr, "[mi_pt build] %-28s %8.*f ms\n", what, decimals, std::chrono::duration<double, std::milli>(BuildClock::now() - since).count());
}

// The "whole image to host" step of the read-backs, behind the caller's refusals: `bytesPerPixel` per pixel of the current size from `src` into
// `host` (NULL: no copy -- an image of mi_pt_read_guides the caller does not want), after a device synchronisation unless an earlier image of
// the same call brought it
int readImage(MiPt* pt, const void* src, size_t bytesPerPixel, void* host, bool synchronise = true)
{
  if(synchronise)
  {
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(hipDeviceSynchronize());
  }
  if(host)
    HIP_TRY(hipMemcpy(host, src, size_t(pt->width) * size_t(pt->height) * bytesPerPixel, hipMemcpyDeviceToHost));
  return MI_PT_OK;
}
// The slot-to-pixel scatter of the first-hit read-backs: every byte of the image `fill`, then the 16-byte record of every slot that `keep`
// accepts and that lies inside the image (the slots of a tile cut by the border do not), at its pixel
template <typename Keep>
void scatterSlots(const MiPt* pt, const void* bySlot, size_t numSlots, int fill, void* host, Keep keep)
{
  memset(host, fill, size_t(pt->width) * size_t(pt->height) * 16);
  const int tileShift = tileShiftOf(pt);
  for(uint32_t slot = 0; slot < uint32_t(numSlots); ++slot)
  {
    int px, py;
    if(keep(slot) && pt::pixelOfSlot(pt->ownedTilesHost.data(), tileShift, pt->width, pt->height, slot, px, py))
      memcpy(static_cast<uint8_t*>(host) + 16 * (size_t(py) * size_t(pt->width) + size_t(px)), static_cast<const uint8_t*>(bySlot) + 16 * size_t(slot), 16);
  }
}

bool vertexMotionActive(const MiPt* pt) { return pt->vertexMotion && pt->temporal && (pt->deform.set || pt->vu.set); }

// The first-hit triangle records of vertex motion, at the current number of pixel slots; none while the feature is not in force.
int allocFirstHitTri(MiPt* pt)
{
  pt->firstHitTri.release();
  pt->paths.firstHitTri = nullptr;
  pt->haveFirstHitTri   = false;
  if(!vertexMotionActive(pt))
    return MI_PT_OK;
  const size_t n = std::max(size_t(std::max(pt->numSlots, 0)), size_t(1));
  HIP_TRY(pt->firstHitTri.alloc(n));
  HIP_TRY(hipMemset(pt->firstHitTri.ptr, 0xff, n * sizeof(uint4)));  // (no primitive: a record nobody wrote takes the rigid path)
  pt->paths.firstHitTri = pt->firstHitTri.ptr;
  return MI_PT_OK;
}

// Everything vertex motion owns, (re)made for the current switches, deformation tables and size: the triangle records, and the previous-pose
// positions initialised to the resident ones.  The caller has synchronised the device.
int allocVertexMotion(MiPt* pt)
{
  pt->vm = MiPt::VertexMotion{};
  if(int rc = allocFirstHitTri(pt))
    return rc;
  if(!vertexMotionActive(pt))
    return MI_PT_OK;
  const size_t numPrims = pt->hostPrims.size();
  pt->vm.prevOffset.assign(numPrims, SIZE_MAX);
  size_t                bytes = 0;
  std::vector<uint32_t> ids;
  std::vector<int> moving = pt->deform.primIDs;  // (the two lists are disjoint: each call refuses a primitive of the other)
  moving.insert(moving.end(), pt->vu.primIDs.begin(), pt->vu.primIDs.end());
  for(int id : moving)
  {
    pt->vm.prevOffset[size_t(id)] = bytes;
    bytes += align16(size_t(pt->primVertices[size_t(id)]) * 12);
    pt->vm.maxVertices = std::max(pt->vm.maxVertices, pt->primVertices[size_t(id)]);
    ids.push_back(uint32_t(id));
  }
  HIP_TRY(pt->vm.prevPositions.alloc(std::max<size_t>(bytes, 16)));
  std::vector<pt::VertexMotionPrim> table(numPrims);
  for(size_t i = 0; i < numPrims; ++i)
  {
    pt::VertexMotionPrim& v = table[i];
    v.prevPositions = pt->vm.prevOffset[i] != SIZE_MAX ? reinterpret_cast<const float*>(pt->vm.prevPositions.ptr + pt->vm.prevOffset[i]) : nullptr;
    v.positions     = pt->hostPrims[i].positions;
    v.indices       = pt->hostPrims[i].indices;
    v.numTriangles  = i < pt->primTriangles.size() ? pt->primTriangles[i] : 0u;
    v.vertexCount   = pt->primVertices[i];
  }
  HIP_TRY(pt->vm.prims.upload(table.data(), table.size()));
  HIP_TRY(pt->vm.deformIDs.upload(ids.data(), ids.size()));
  pt::launchSnapshotPositions(pt->vm.prims.ptr, pt->vm.deformIDs.ptr, uint32_t(ids.size()), pt->vm.maxVertices, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return MI_PT_OK;
}

// Path state and ray queues for `frames` frames in flight (path slots are micro-tile major: pt::pathSlot).
int allocPathResources(MiPt* pt, int frames)
{
  if(size_t(pt->numSlots) * size_t(frames) >= 0x7fffffffull)
    return fail(MI_PT_ERR_ARGUMENT, "too many path slots: reduce the frames in flight or the resolution");
  pt->framesCap          = frames;
  const size_t n         = std::max(size_t(pt->numSlots) * size_t(frames), size_t(1));
  // By slot: the radiance record alone (what k_finish_sample folds; a path's other state travels in its queue entry).  The optional
  // records of the previous size are dropped and come back on demand.
  HIP_TRY(pt->pathArrays.alloc(n));
  HIP_TRY(pt->firstHit.alloc(std::max(size_t(pt->numSlots), size_t(1))));
  pt->haveFirstHit = false;
  pt->optThroughput.release(); pt->optMisc.release(); pt->optMedium.release(); pt->optPixelSum.release(); pt->optGuides.release(); pt->optShadowAux2.release();
  pt::PathSoA& P = pt->paths;
  P              = pt::PathSoA{};
  P.radiance     = pt->pathArrays.ptr;
  P.firstHit     = pt->firstHit.ptr;
  if(int rc = allocFirstHitTri(pt))
    return rc;
  // sub-queue capacity: ceil(numChunks / NSUB) chunks (+1 of slack), see pt_scene.h
  const size_t numChunks = (n + pt::QCHUNK - 1) / pt::QCHUNK;
  const size_t subCap    = ((numChunks + pt::NSUB - 1) / pt::NSUB + 1) * pt::QCHUNK;
  const size_t qsize     = subCap * pt::NSUB;
  // path slots and queue positions are 31-bit: bit 31 of a shadow entry's slot field tells the two apart (pt_scene.h: SHADOW_TARGET_QUEUE),
  // 0xffffffff is QUEUE_DEAD, and the frame index of a slot is a 31-bit multiply-high (FrameConsts::framesMagic)
  if(qsize >= (size_t(1) << 31))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_render_frames: " + std::to_string(frames) + " frames in flight x " + std::to_string(pt->numSlots)
                                        + " pixel slots exceed 2^31 path slots");
  HIP_TRY(pt->queueMem.alloc(qsize * 3 + pt::QC_COUNT));
  // 14 records of 16 bytes per queue position: the two active queues' ray + state (org, dir, aux2, misc, rad), ONE hit record shared by both (the
  // closest-hit walk writes it, the shade launch of the same bounce reads it, and the next walk -- of the other queue -- starts after that launch:
  // the two queues' hit records are never alive together), the shadow queue's ray + contribution (org, dir, aux).  The shadow queue's aux2 exists
  // on shadow-catcher frames only (optShadowAux2).
  HIP_TRY(pt->queuePayload.alloc(qsize * 14));
  pt->queueCap = qsize;
  pt::RayQueue* qs[3] = {&pt->queues.active[0], &pt->queues.active[1], &pt->queues.shadow};
  for(int i = 0; i < 3; ++i)
    qs[i]->slot = pt->queueMem.ptr + qsize * size_t(i);
  for(int i = 0; i < 2; ++i)  // the living paths' ray and state, in queue order (pt_scene.h: RayQueue, FrameConsts::stateInQueue)
  {
    qs[i]->org  = pt->queuePayload.ptr + qsize * size_t(5 * i + 0);
    qs[i]->dir  = pt->queuePayload.ptr + qsize * size_t(5 * i + 1);
    qs[i]->aux2 = pt->queuePayload.ptr + qsize * size_t(5 * i + 2);
    qs[i]->misc = pt->queuePayload.ptr + qsize * size_t(5 * i + 3);
    qs[i]->rad  = pt->queuePayload.ptr + qsize * size_t(5 * i + 4);
    qs[i]->aux  = pt->queuePayload.ptr + qsize * 10;
  }
  pt->queues.shadow.org  = pt->queuePayload.ptr + qsize * 11;
  pt->queues.shadow.dir  = pt->queuePayload.ptr + qsize * 12;
  pt->queues.shadow.aux  = pt->queuePayload.ptr + qsize * 13;
  pt->queues.shadow.aux2 = nullptr;
  pt->queues.shadow.misc = pt->queues.shadow.rad = nullptr;
  pt->queues.counters = pt->queueMem.ptr + 3 * qsize;
  pt->queues.subCap   = uint32_t(subCap);
  // recorded transmissive shadow candidates (pt_scene.h): two pool entries per shadow-queue entry, and an overflow list as long as
  // the queue.  MI_PT_DIAG_CAND_POOL=<entries> shrinks the pool (tests of the overflow path); 0 disables recording.
  pt->queues.candPool = nullptr; pt->queues.candNext = nullptr; pt->queues.overflow = nullptr;
  pt->queues.candCap  = 0;
  size_t candCap = qsize * 2;
  if(pt->sw.candPoolSet)
    candCap = pt->sw.candPool;
  if(pt->hasTransmissive && pt->accel.wide && candCap > 0)
  {
    candCap = std::min(candCap, size_t(0x7fffffff));
    HIP_TRY(pt->candPool.alloc(candCap));
    HIP_TRY(pt->candLists.alloc(candCap + qsize));
    pt->queues.candPool = pt->candPool.ptr;
    pt->queues.candNext = pt->candLists.ptr;
    pt->queues.overflow = pt->candLists.ptr + candCap;
    pt->queues.candCap  = uint32_t(candCap);
  }
  HIP_TRY(hipMemset(pt->queues.counters, 0, sizeof(uint32_t) * pt::QC_COUNT));
  return MI_PT_OK;
}

// The by-slot / by-position records only some batches need (MiPt::opt*): allocated the first time a batch needs them, at the size of the
// current path resources, and kept until those are reallocated.  An allocation here synchronises the device once.
int ensureOptionalPathArrays(MiPt* pt, bool stateBySlot, bool multiSample, bool guides, bool catcher)
{
  const size_t n = std::max(size_t(pt->numSlots) * size_t(pt->framesCap), size_t(1));
  auto need = [&](DevBuf<float4>& b, size_t count) -> int {
    if(b.ptr)
      return MI_PT_OK;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(b.alloc(count));
    HIP_TRY(hipMemset(b.ptr, 0, count * sizeof(float4)));
    return MI_PT_OK;
  };
  pt::PathSoA& P = pt->paths;
  if(stateBySlot || multiSample)
  {
    if(int rc = need(pt->optMisc, n)) return rc;
    P.misc = pt->optMisc.ptr;
  }
  if(stateBySlot)
  {
    if(int rc = need(pt->optThroughput, n)) return rc;
    P.throughput = pt->optThroughput.ptr;
  }
  if(multiSample)
  {
    if(int rc = need(pt->optPixelSum, n)) return rc;
    P.pixelSum = pt->optPixelSum.ptr;
  }
  if(!pt->simpleMaterials)  // the generic shade kernel keeps the medium a path is inside of
  {
    if(int rc = need(pt->optMedium, n)) return rc;
    P.medium = reinterpret_cast<uint4*>(pt->optMedium.ptr);
  }
  if(guides)
  {
    if(int rc = need(pt->optGuides, 2 * n)) return rc;
    P.guideAlbedo = pt->optGuides.ptr;
    P.guideNormal = pt->optGuides.ptr + n;
  }
  if(catcher)
  {
    if(int rc = need(pt->optShadowAux2, pt->queueCap)) return rc;
    pt->queues.shadow.aux2 = pt->optShadowAux2.ptr;
  }
  return MI_PT_OK;
}

// The motion image, the history and the previous matrices of mi_pt_set_temporal, at the current size; nothing is valid afterwards.
int allocTemporal(MiPt* pt)
{
  pt->temporalData = MiPt::Temporal{};
  if(!pt->temporal)
    return allocVertexMotion(pt);
  const size_t px = size_t(std::max(pt->width, 0)) * size_t(std::max(pt->height, 0));
  HIP_TRY(pt->temporalData.motion.alloc(px));
  HIP_TRY(pt->temporalData.history.alloc(6 * px));
  HIP_TRY(pt->temporalData.prevObjectToWorld.alloc(pt->nodes.count * 16));
  if(px)
    HIP_TRY(hipMemset(pt->temporalData.motion.ptr, 0, px * sizeof(float4)));
  pt::launchSnapshotTransforms(pt->nodes.ptr, pt->temporalData.prevObjectToWorld.ptr, int(pt->nodes.count), nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return allocVertexMotion(pt);
}

int allocFrameResources(MiPt* pt)
{
  const int W = pt->width, H = pt->height, T = pt->tileSize;
  pt->tilesX = (W + T - 1) / T;
  pt->tilesY = (H + T - 1) / T;
  const std::vector<uint32_t> owned = tileOrigins(pt, pt->tileRank, pt->tileWorld);  // the tiles this rank renders
  pt->numSlots = int(owned.size()) * T * T;
  HIP_TRY(pt->ownedTiles.upload(owned.data(), owned.size()));
  pt->ownedTilesHost = owned;
  pt->allTiles.release();
  if(pt->tileWorld > 1)  // (mi_pt_make_camera_rays writes every pixel whatever the partition, and its device form may not allocate)
  {
    const std::vector<uint32_t> all = tileOrigins(pt, 0, 1);
    HIP_TRY(pt->allTiles.upload(all.data(), all.size()));
  }
  if(int rc = allocPathResources(pt, pt->framesCap))
    return rc;
  const size_t px = size_t(W) * size_t(H);
  HIP_TRY(pt->accumOwn.alloc(px));
  HIP_TRY(hipMemset(pt->accumOwn.ptr, 0, px * sizeof(float4)));
  pt->accum = pt->accumOwn.ptr;
  HIP_TRY(pt->albedo.alloc(px));
  HIP_TRY(pt->normal.alloc(px));
  HIP_TRY(hipMemset(pt->albedo.ptr, 0, px * sizeof(float4)));
  HIP_TRY(hipMemset(pt->normal.ptr, 0, px * sizeof(float4)));
  HIP_TRY(pt->depth.alloc(px));
  HIP_TRY(pt->selection.alloc(px));
  HIP_TRY(hipMemset(pt->selection.ptr, 0, px * sizeof(uint32_t)));
  {
    std::vector<float> ones(px, 1.0f);
    HIP_TRY(hipMemcpy(pt->depth.ptr, ones.data(), px * sizeof(float), hipMemcpyHostToDevice));
  }
  pt->denoiseA.release();
  pt->denoiseB.release();
  pt->tonemapped.release();
  pt->tmHistogram.release();
  pt->tmAutoState.release();
  return allocTemporal(pt);
}


// The structure's arrays as the kernels see them (all null once they are released); the per-triangle shade and alpha records are made from
// them afterwards (makeTriangleRecords)
void publishAcceleration(MiPt* pt)
{
  pt::DevScene& S = pt->scene;
  S.bvhNodes = pt->accel.bvhNodes.ptr; S.bvh8Nodes = pt->accel.bvh8Nodes.ptr; S.tris = pt->accel.bvhTris.ptr;
  S.bvh8Planes = pt->accel.bvh8Nodes.ptr ? pt->accel.bvh8Planes.ptr : nullptr;
  S.shadeTris = nullptr;
  S.alphaTris = nullptr;
  pt->sceneDevDirty = true;
}
// The state a failed build or refit leaves: an EMPTY structure, no refit data, the error message kept.
void dropAcceleration(MiPt* pt)
{
  const std::string why = g_lastError;  // (the frees below must not disturb the message)
  pt->accel.refit = MiPt::Accel::RefitData{};
  pt->accel.releaseAll();
  publishAcceleration(pt);
  pt::DevScene& S = pt->scene;
  S.numTris = 0; S.bvh8NumNodes = 0; S.bvhRoot = pt::BVH_EMPTY;
  pt->staticStats.bvhNodeCount = pt->staticStats.bvhTriangleCount = 0;
  g_lastError = why;
}
// Per render node: its material's instance flags, and INST_FLIP_FACING for a mirroring matrix (the triangle records carry them); sets the
// scene-wide material summaries (hasAlpha, ...) on the way.  The build and the refit both take them from here.
std::vector<uint8_t> instanceFlags(MiPt* pt)
{
  const int            numNodes = int(pt->hostNodes.size()), numMaterials = int(pt->matInstFlags.size());
  std::vector<uint8_t> flags(size_t(std::max(numNodes, 1)), 0);
  pt->hasAlpha = pt->hasAlphaTest = pt->hasTransmissive = pt->hasVolumeScatter = false;
  pt->simpleMaterials = true;
  for(int n = 0; n < numNodes; ++n)
  {
    const MiGltfRenderNode& rn = pt->hostNodes[size_t(n)];
    const int               m  = std::max(0, std::min(rn.materialID, numMaterials - 1));
    uint32_t                f  = pt->matInstFlags[size_t(m)];
    if(!(f & pt::INST_FORCE_OPAQUE))
      pt->hasAlpha = true;
    if(!(f & (pt::INST_FORCE_OPAQUE | pt::INST_ALPHA_PASSES)))
      pt->hasAlphaTest = true;  // some candidate's alpha test has an open outcome (MASK / BLEND materials)
    if(f & pt::INST_TRANSMISSIVE)
      pt->hasTransmissive = true;
    if(pt->matFeatures[size_t(m)] & 1u)
      pt->hasVolumeScatter = true;
    if(pt->matFeatures[size_t(m)] & 2u)
      pt->simpleMaterials = false;
    const float* M   = rn.objectToWorld;
    float        det = M[0] * (M[5] * M[10] - M[9] * M[6]) - M[4] * (M[1] * M[10] - M[9] * M[2]) + M[8] * (M[1] * M[6] - M[5] * M[2]);
    if(det < 0.0f)
      f |= pt::INST_FLIP_FACING;
    flags[size_t(n)] = uint8_t(f);
  }
  return flags;
}

// The SAH cost of the resident tree from the refit data (the node boxes and terms k_refit_level wrote), read back: one small copy
int readSahCost(MiPt* pt, double& cost)
{
  pt::launchSahCost(pt->accel.refit.sah.ptr, uint32_t(pt->scene.bvh8NumNodes), pt->accel.refit.nodeBox.ptr, pt->accel.refit.sahPartial.ptr, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(&cost, pt->accel.refit.sahPartial.ptr + pt::REFIT_SAH_PARTIALS, sizeof(double), hipMemcpyDeviceToHost));
  return MI_PT_OK;
}

// One refit pass over the `numNodes` nodes of the resident tree: every node from its children, level by level (`levels`: the build's own while it
// runs, pt->accel.refit.levels afterwards), the packet walk's planes where there are any, the SAH cost into `cost`
int refitPass(MiPt* pt, uint32_t numNodes, const std::vector<uint32_t>& levels, double& cost)
{
  pt::launchRefitLevels(pt->accel.bvh8Nodes.ptr, levels, pt->accel.refit.slotBox.ptr, pt->accel.refit.nodeBox.ptr, pt->accel.refit.sah.ptr, nullptr);
  if(pt->accel.bvh8Planes.ptr)
    pt::launchBvh8Planes(pt->accel.bvh8Nodes.ptr, numNodes, pt->accel.bvh8Planes.ptr, nullptr);
  HIP_TRY(hipGetLastError());
  return readSahCost(pt, cost);
}

// The device part of a refit over the render nodes' `dirty` bytes (pt::REFIT_*): the triangle records and slot boxes of the dirty nodes
// (k_refit_tris), every node level by level, the planes, the SAH cost into refit.sahNow.  `flags` (an update): the node table and these
// instance flags are uploaded first; NULL (the hide pass of a build): the build just uploaded both.
int refitOnDevice(MiPt* pt, const std::vector<uint8_t>& dirty, const std::vector<uint8_t>* flags)
{
  if(flags)
  {
    HIP_TRY(hipMemcpy(pt->nodes.ptr, pt->hostNodes.data(), sizeof(MiGltfRenderNode) * pt->hostNodes.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pt->instFlags.ptr, flags->data(), flags->size(), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(pt->accel.refit.dirty.ptr, dirty.data(), dirty.size(), hipMemcpyHostToDevice));
  pt::launchRefitTris(pt->nodes.ptr, pt->prims.ptr, pt->instFlags.ptr, pt->accel.refit.dirty.ptr, pt->accel.refit.builtBox.ptr, pt->accel.bvhTris.ptr,
                      pt->accel.refit.slotBox.ptr, uint32_t(pt->scene.numTris), nullptr);
  if(int rc = refitPass(pt, uint32_t(pt->scene.bvh8NumNodes), pt->accel.refit.levels, pt->accel.refit.sahNow))
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  return MI_PT_OK;
}

// Resident mode is wanted of a build when it is enabled and the build can keep refit data (residentInForce: it then did)
bool residentWanted(const MiPt* pt) { return pt->accel.accelResident && pt->accel.accelMode != MI_PT_ACCEL_REBUILD && !pt->accel.keepsNoRefitData(pt->sw); }
bool residentInForce(const MiPt* pt) { return pt->accel.residentTree && pt->accel.canRefit(); }

// The phases of a build follow, in the order buildStructure and buildAccelerationUnguarded run them.  The render-node instances a build is made over, flattened on the host: `entryNode` the render nodes that contribute triangles, `triOffset`
// where each one's triangles start (+ the total at the end).  `resident`: every render node that owns triangles, as if all were visible.
struct FlatInstances
{
  std::vector<uint32_t> triOffset;
  std::vector<int32_t>  entryNode;
  uint64_t              totalTris = 0, hiddenTris = 0;  // hiddenTris: of the hidden nodes among them (resident only)
};
int flattenInstances(const MiPt* pt, bool resident, FlatInstances& flat)
{
  const int numNodes = int(pt->hostNodes.size()), numPrims = int(pt->primTriangles.size());
  flat.triOffset.push_back(0);
  for(int n = 0; n < numNodes; ++n)
  {
    const MiGltfRenderNode& rn = pt->hostNodes[size_t(n)];
    const bool hidden = !pt->hostVisible.empty() && !pt->hostVisible[size_t(n)];
    if(hidden && !resident)
      continue;  // invisible nodes get no geometry (reference: src/gltf_scene_rtx.cpp:319-323)
    if(rn.renderPrimID < 0 || rn.renderPrimID >= numPrims || pt->primTriangles[size_t(rn.renderPrimID)] == 0)
      continue;
    if(hidden)
      flat.hiddenTris += pt->primTriangles[size_t(rn.renderPrimID)];
    flat.totalTris += pt->primTriangles[size_t(rn.renderPrimID)];
    if(flat.totalTris > 0x7fffffffull)
      return fail(MI_PT_ERR_ARGUMENT, "more than 2^31 flattened triangles");
    flat.entryNode.push_back(n);
    flat.triOffset.push_back(uint32_t(flat.totalTris));
  }
  return MI_PT_OK;
}

// What a build holds on the device while it runs and releases when it is over (in the reverse of this order)
struct TreeBuild
{
  DevBuf<uint32_t>   dOffset;
  DevBuf<int32_t>    dEntry;
  pt::BvhBuildOutput bo;
  pt::Bvh8Output     b8;  // empty under the BVH2 walk and for a scene without triangles
};
// The tree over `flat`: Morton sort + PLOC -> BVH2 -> (default) 8-wide collapse, its arrays into pt->accel, its figures into the scene
// descriptor and the statistics, the packet walk's planes.  The refit data stays in `t.b8` for keepRefitData.
int buildTree(MiPt* pt, const FlatInstances& flat, TreeBuild& t)
{
  HIP_TRY(t.dOffset.upload(flat.triOffset.data(), flat.triOffset.size()));
  HIP_TRY(t.dEntry.upload(flat.entryNode.data(), flat.entryNode.size()));
  pt::BvhBuildInput in{pt->nodes.ptr, pt->prims.ptr, pt->instFlags.ptr, t.dOffset.ptr, t.dEntry.ptr, int(flat.entryNode.size()), uint32_t(flat.totalTris)};
  in.karrasTopology = (pt->accel.bvhBuilder & 2) != 0;
  // (accelBuilds counts this build already.)  The build of a switch to REFIT / AUTO makes the tree the updates then refit: it runs the scene
  // build's passes, once, at a moment the caller chose.  The fallback and AUTO rebuilds of those modes happen during playback and run the
  // update's passes like every other rebuild -- 16 passes would add ~160 ms to a 17-ms rebuild at 2.8 M triangles (RunSwitches::reinsertUpdate)
  in.reinsertPasses = (pt->accel.accelBuilds == 1 || pt->accel.switchBuild) ? pt->sw.reinsert : pt->sw.reinsertUpdate;
  in.reinsertRounds = pt->sw.reinsertRounds;
  in.splitFactor    = pt->sw.splitFactor;
  in.splitMaxDepth  = pt->sw.splitMaxDepth;
  in.splitMinShare  = pt->sw.splitMinShare;
  // The BVH2 walk leaves one stack entry per level: its tree is no taller than that stack (buildBvh rebuilds a taller one).  The 8-wide walk
  // is bounded after the collapse, below.
  pt->accel.wide = (pt->accel.bvhBuilder & 1) == 0;
  in.maxHeight   = pt->accel.wide ? 0 : pt::BVH_STACK_LDS + pt::BVH_STACK_PRIV;
  pt::Bvh8Options b8opt;
  b8opt.sahCollapse = !pt->sw.collapseGreedy; b8opt.hostCollapse = pt->sw.hostCollapse;
  b8opt.keepRefit   = pt->accel.accelMode != MI_PT_ACCEL_REBUILD;
  std::string err;
  // the BVH2 from `in` and, for the 8-wide walk, the tree collapsed from it
  auto buildPair = [&]() -> int {
    pt::BvhBuildOutput& bo = t.bo;
    if(!pt::buildBvh(in, bo, nullptr, err))
      return fail(MI_PT_ERR_HIP, "BVH build failed: " + err);
    pt->scene.bvhRoot = bo.root;
    pt->scene.numTris = int(bo.numTris);
    pt->scene.bvh8NumNodes = 0;
    pt->staticStats.bvhNodeCount     = bo.numNodes;
    pt->staticStats.bvhTriangleCount = bo.numTris;
    pt->accel.splitRefs              = bo.numTris > bo.sceneTris;
    pt->staticStats.bvhNodeBytes     = 64;
    pt->staticStats.bvhTriangleBytes = sizeof(pt::DevTri);
    // the triangle rounds of the 8-wide walk pack (triangle index | owner lane << 26) into one word (pt_kernels.hip)
    if(pt->accel.wide && bo.numTris >= (1u << 26))
      return fail(MI_PT_ERR_ARGUMENT, "scene has 2^26 or more triangles: beyond what the 8-wide BVH walk indexes (select the BVH2 walk, bvhBuilder bit 0)");
    if(!pt->accel.wide || bo.numTris == 0)
      return MI_PT_OK;
    pt->accel.refitCapable = !pt->sw.hostCollapse && bo.numNodes > 0;  // (a one-reference scene takes the host collapse: bvh8.hip)
    if(!pt::buildBvh8(bo, t.b8, nullptr, err, b8opt))
      return fail(MI_PT_ERR_HIP, "BVH8 collapse failed: " + err);
    return MI_PT_OK;
  };
  if(int rc = buildPair())
    return rc;
  // A node visit of the 8-wide walk pushes at most one group (the visited node's other hit inner children), and none at a node without inner
  // children: a tree of L levels needs L - 1 stack slots at most.  One with more levels than the stack covers (LaneStack2 drops what it cannot
  // hold) is collapsed again from a BVH2 of that height at most -- an 8-wide node spans at least one BVH2 level -- which buildBvh makes with the
  // Morton-prefix topology or fails.  (The split references, and so the figures above, do not depend on the topology.)
  const uint32_t maxLevels = uint32_t(pt::BVH8_STACK_LDS + pt::BVH8_STACK_PRIV) + 1u;
  if(t.b8.numLevels > maxLevels)
  {
    if(buildTiming())
      fprintf(stderr, "[mi_pt build] 8-wide tree of %u levels (limit %u): rebuilt from a BVH2 of bounded height\n", t.b8.numLevels, maxLevels);
    in.karrasTopology = true;
    in.maxHeight      = int(maxLevels);
    t.b8              = pt::Bvh8Output();
    if(int rc = buildPair())
      return rc;
    if(t.b8.numLevels > maxLevels)
      return fail(MI_PT_ERR_HIP, "BVH8 collapse failed: more levels than the walk's stack covers");
  }
  if(!pt->accel.wide || t.bo.numTris == 0)
  {
    pt->accel.bvhNodes = std::move(t.bo.nodes);
    pt->accel.bvhTris  = std::move(t.bo.tris);
    return MI_PT_OK;
  }
  // the wide structure owns its own triangle order; the BVH2 arrays are no longer needed
  t.bo.nodes.release();
  t.bo.tris.release();
  pt->accel.bvhTris   = std::move(t.b8.tris);
  pt->accel.bvh8Nodes = std::move(t.b8.nodes);
  pt->scene.bvhRoot = 0;
  pt->scene.bvh8NumNodes = int(t.b8.numNodes);
  pt->staticStats.bvhNodeCount = t.b8.numNodes;
  pt->staticStats.bvhNodeBytes = 80;
  if(!pt->sw.noPlanes)  // A/B switch of the packet walk's float planes
  {
    HIP_TRY(pt->accel.bvh8Planes.alloc(size_t(t.b8.numNodes) * 48));
    pt::launchBvh8Planes(pt->accel.bvh8Nodes.ptr, t.b8.numNodes, pt->accel.bvh8Planes.ptr, nullptr);
    HIP_TRY(hipGetLastError());
  }
  return MI_PT_OK;
}

// The refit data of the 8-wide tree just built, where its collapse returned any (the host collapse keeps none: its updates rebuild)
int keepRefitData(MiPt* pt, pt::Bvh8Output& b8, bool resident, uint64_t hiddenTris)
{
  pt->accel.refit.slotBox = std::move(b8.slotBox);
  pt->accel.refit.nodeBox = std::move(b8.nodeBox);
  if(!pt->accel.refit.slotBox.ptr || !pt->accel.refit.nodeBox.ptr)
  {
    pt->accel.refit.slotBox.release();
    pt->accel.refit.nodeBox.release();
    return MI_PT_OK;
  }
  // the boxes the build filed the references under stay as they are (REFIT_HOME), the SAH cost of the tree as built.
  // The nodes are requantised once from the unions of those boxes (a BVH2 box may be looser than the union below it): the tree an
  // update refits back to the build's pose is then this one, byte for byte.
  HIP_TRY(pt->accel.refit.builtBox.alloc(b8.numTris));
  HIP_TRY(hipMemcpy(pt->accel.refit.builtBox.ptr, pt->accel.refit.slotBox.ptr, sizeof(pt::RefitBox) * size_t(b8.numTris), hipMemcpyDeviceToDevice));
  HIP_TRY(pt->accel.refit.sah.alloc(b8.numNodes));
  HIP_TRY(pt->accel.refit.sahPartial.alloc(pt::REFIT_SAH_PARTIALS + 1));
  HIP_TRY(pt->accel.refit.dirty.alloc(std::max<size_t>(pt->hostNodes.size(), 1)));
  if(int rc = refitPass(pt, b8.numNodes, b8.levels, pt->accel.refit.sahAtBuild))
    return rc;
  pt->accel.refit.sahNow = pt->accel.refit.sahAtBuild;
  pt->accel.refit.levels = std::move(b8.levels);
  pt->accel.builtNodes   = pt->hostNodes;
  pt->accel.primDirty.assign(pt->primTriangles.size(), 0);
  pt->accel.primDeformed.assign(pt->primTriangles.size(), 0);
  pt->accel.residentTree = resident;
  pt->accel.hiddenTris   = resident ? hiddenTris : 0;
  return MI_PT_OK;
}

// Every alpha record into the allocated pt->accel.alphaTris, as a build makes them (patchTriangleData: for a scene that had none)
int makeAlphaRecords(MiPt* pt)
{
  pt::launchBuildAlphaRecords(pt->scene, uint32_t(pt->scene.numTris), pt->accel.alphaTris.ptr, nullptr);
  HIP_TRY(hipGetLastError());
  pt->scene.alphaTris = pt->accel.alphaTris.ptr;
  return MI_PT_OK;
}
// The per-triangle shade and alpha records of the published structure
int makeTriangleRecords(MiPt* pt)
{
  pt::DevScene& S = pt->scene;
  if(S.numTris > 0)
  {
    HIP_TRY(pt->accel.shadeTris.alloc(size_t(S.numTris)));
    pt::launchBuildShadeRecords(S, uint32_t(S.numTris), pt->accel.shadeTris.ptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    S.shadeTris = pt->accel.shadeTris.ptr;
  }
  if(pt->hasAlpha && S.numTris > 0)
  {
    HIP_TRY(pt->accel.alphaTris.alloc(size_t(S.numTris)));
    if(int rc = makeAlphaRecords(pt))
      return rc;
    HIP_TRY(hipDeviceSynchronize());
  }
  return MI_PT_OK;
}

// The structure over the current node table, up to its refit data: the previous one is released on the way.
// `resident`: over every render node that owns triangles, as if all were visible; `hiddenTris`: the triangles of the hidden ones among them.
int buildStructure(MiPt* pt, bool resident, uint64_t& hiddenTris)
{
  pt->accel.refit        = MiPt::Accel::RefitData{};
  pt->accel.residentTree = false;
  pt->accel.hiddenTris   = 0;
  const std::vector<uint8_t> flags = instanceFlags(pt);
  FlatInstances              flat;
  if(int rc = flattenInstances(pt, resident, flat))
    return rc;
  hiddenTris = flat.hiddenTris;
  HIP_TRY(pt->nodes.upload(pt->hostNodes.data(), pt->hostNodes.size()));
  HIP_TRY(pt->instFlags.upload(flags.data(), flags.size()));
  pt->scene.nodes = pt->nodes.ptr;

  // release the previous structure (an update), then build
  pt->accel.releaseTree();
  pt->accel.refitCapable = false;
  if(pt->accel.accelBuilds++ == pt->sw.failBuildAt && pt->sw.failBuildAt > 0)  // test hook (armed at mi_pt_create): this REbuild fails after the old structure is gone
    return fail(MI_PT_ERR_HIP, "BVH build failed: MI_PT_DIAG_FAIL_BUILD");
  TreeBuild t;
  if(int rc = buildTree(pt, flat, t))
    return rc;
  return pt->accel.wide && pt->scene.numTris > 0 ? keepRefitData(pt, t.b8, resident, flat.hiddenTris) : MI_PT_OK;
}

// Flattens the visible render-node instances to world-space triangles and builds the acceleration structure over them on the
// device: Morton sort + PLOC -> BVH2 -> (default) 8-wide collapse, then the per-triangle shading / alpha records.  Everything it
// needs is resident (geometry pool, materials) or kept on the host in MiPt (node matrices, visibility), so it serves the scene
// build (mi_pt_create; reference: SceneRtx BLAS + TLAS build, src/gltf_scene_rtx.cpp:173-385) and the transform / visibility
// updates of animated scenes (mi_pt_update_render_nodes; reference: TLAS update, src/gltf_scene_transform_vk.cpp:534-639) alike.
// In resident mode (residentWanted) the structure is built over the hidden nodes too, which one refit pass then hides.
int buildAccelerationUnguarded(MiPt* pt)
{
  const bool resident   = residentWanted(pt);
  uint64_t   hiddenTris = 0;
  if(int rc = buildStructure(pt, resident, hiddenTris))
    return rc;
  if(resident && !pt->accel.residentTree && hiddenTris > 0)
  {
    // no refit data came of it (a one-reference scene: bvh8.hip), so nothing could hide them: over the visible nodes, as the same build
    --pt->accel.accelBuilds;
    if(int rc = buildStructure(pt, false, hiddenTris))
      return rc;
  }
  publishAcceleration(pt);
  if(int rc = makeTriangleRecords(pt))
    return rc;
  if(pt->accel.residentTree && pt->accel.hiddenTris > 0)
  {
    // the hide pass: the records above were made from the all-visible tree (they hold no geometry); sahAtBuild stays the all-visible cost
    std::vector<uint8_t> dirty(std::max<size_t>(pt->hostNodes.size(), 1), pt::REFIT_CLEAN);
    for(size_t n = 0; n < pt->hostNodes.size(); ++n)
      if(!pt->hostVisible[n])
        dirty[n] = pt::REFIT_HIDDEN;
    return refitOnDevice(pt, dirty, nullptr);
  }
  return MI_PT_OK;
}

// A failed (re)build must not leave the scene descriptor pointing at freed or half-built arrays: mi_pt_update_render_nodes runs
// this once per animated frame, and the next mi_pt_render_frame would walk them.  On any error the instance falls back to an
// EMPTY structure (frames render the environment only) and the error is returned to the caller.
int buildAcceleration(MiPt* pt)
{
  const auto t0 = BuildClock::now();
  const int  rc = buildAccelerationUnguarded(pt);
  if(buildTiming() && pt->accel.accelBuilds > 1)  // (the first build's phases are printed by mi_pt_create)
  {
    (void)hipDeviceSynchronize();
    printBuildTiming("rebuild", t0);
  }
  pt->accel.lastUpdate = MI_PT_ACCEL_LAST_BUILD;
  if(rc != MI_PT_OK)
    dropAcceleration(pt);
  return rc;
}

// The refit of an update: `moved` per render node = its matrices changed.  The triangle records and slot boxes of what moved or deformed
// (k_refit_tris: REFIT_HOME for geometry back in the pose of the last build, whose boxes are then the ones it was built with -- except a
// primitive deformed since that build: deformed vertices are not compared with the built ones, so its pre-split references keep their
// whole triangles' boxes until the next build, conservative and the same image), every node
// level by level, the packet walk's planes, the SAH cost.  AUTO rebuilds when that cost exceeds the ratio x the cost at the last build.
// `visWas`, resident mode only (else NULL): per render node, whether it was visible before this update.  A node that became hidden is
// REFIT_HIDDEN, one that stays hidden is clean whatever its matrices do, one that came back is HOME or MOVED by the same comparison.
int refitAcceleration(MiPt* pt, const std::vector<uint8_t>& moved, const std::vector<uint8_t>* visWas = nullptr)
{
  const auto           t0       = BuildClock::now();
  const size_t         numNodes = pt->hostNodes.size(), numPrims = pt->primTriangles.size();
  std::vector<uint8_t> dirty(std::max<size_t>(numNodes, 1), pt::REFIT_CLEAN);
  std::vector<uint8_t> visKept;
  if(!visWas && pt->accel.residentTree && !pt->hostVisible.empty())  // (a deformation update: what is hidden in the resident tree stays hidden)
  {
    visKept = pt->hostVisible;
    visWas  = &visKept;
  }
  uint64_t             movedTris = 0;
  for(size_t n = 0; n < numNodes; ++n)
  {
    const MiGltfRenderNode& rn       = pt->hostNodes[n];
    const bool              ownsPrim = rn.renderPrimID >= 0 && size_t(rn.renderPrimID) < numPrims;
    bool                    shown    = false;
    if(visWas)
    {
      const bool visNow = pt->hostVisible.empty() || pt->hostVisible[n];
      if(!visNow)
      {
        if((*visWas)[n])
          dirty[n] = pt::REFIT_HIDDEN;
        continue;
      }
      shown = !(*visWas)[n];
    }
    if(!shown && !moved[n] && !(ownsPrim && pt->accel.primDirty[size_t(rn.renderPrimID)]))
      continue;
    const bool home = memcmp(rn.objectToWorld, pt->accel.builtNodes[n].objectToWorld, sizeof(float) * 32) == 0 && !(ownsPrim && pt->accel.primDeformed[size_t(rn.renderPrimID)]);
    dirty[n]        = home ? pt::REFIT_HOME : pt::REFIT_MOVED;
    if(ownsPrim && (pt->hostVisible.empty() || pt->hostVisible[n]))
      movedTris += pt->primTriangles[size_t(rn.renderPrimID)];
  }
  const std::vector<uint8_t> flags = instanceFlags(pt);
  if(int rc = refitOnDevice(pt, dirty, &flags))
  {
    dropAcceleration(pt);
    return rc;
  }
  std::fill(pt->accel.primDirty.begin(), pt->accel.primDirty.end(), uint8_t(0));
  pt->sceneDevDirty = true;
  printBuildTiming("refit", t0);
  if(pt->accel.accelMode == MI_PT_ACCEL_AUTO && pt->accel.refit.sahNow > double(pt->accel.accelRatio) * pt->accel.refit.sahAtBuild)
    return buildAcceleration(pt);
  if(visWas)
  {
    pt->accel.hiddenTris = 0;
    for(size_t n = 0; n < numNodes; ++n)
    {
      const int prim = pt->hostNodes[n].renderPrimID;
      if(!pt->hostVisible.empty() && !pt->hostVisible[n] && prim >= 0 && size_t(prim) < numPrims)
        pt->accel.hiddenTris += pt->primTriangles[size_t(prim)];
    }
  }
  ++pt->accel.accelRefits;
  pt->accel.lastUpdate     = MI_PT_ACCEL_LAST_REFIT;
  pt->accel.trianglesMoved = movedTris;
  return MI_PT_OK;
}

// An update of the node table or of the deformed geometry: a refit when the mode and the resident structure allow one and the update
// keeps the topology (`sameTopology`: primitives, materials and visibility unchanged), a full build otherwise.
int updateAcceleration(MiPt* pt, bool sameTopology, const std::vector<uint8_t>& moved)
{
  if(sameTopology && pt->accel.canRefit())
    return refitAcceleration(pt, moved);
  return buildAcceleration(pt);
}
// The build of a switch of the mode or of resident mode: the tree the updates then refit, made with the scene build's passes (buildTree)
int buildForSwitch(MiPt* pt)
{
  pt->accel.switchBuild = true;
  const int rc          = buildAcceleration(pt);
  pt->accel.switchBuild = false;
  return rc;
}

// What makeAlphaRecord (pt_shading.h) reads of a material and its base / diffuse texture info, as it reads it: two materials with equal
// keys give equal alpha records for the same triangle.  (An OPAQUE material's record is the default one whatever else it holds.)
struct AlphaKey
{
  int32_t  alphaMode = MI_ALPHA_OPAQUE;
  float    cutoff = 0.0f, factorAlpha = 0.0f;
  uint32_t slot = 0;
  int32_t  index = 0, texCoord = 0;
};
AlphaKey alphaKey(const MiGltfShadeMaterial& mat, const MiGltfTextureInfo* infos)
{
  AlphaKey k;
  if(mat.alphaMode == MI_ALPHA_OPAQUE)
    return k;
  const bool sg = mat.pbrModel == MI_PBR_SPECULAR_GLOSSINESS;
  k.alphaMode   = mat.alphaMode;
  k.cutoff      = mat.alphaCutoff;
  k.factorAlpha = sg ? mat.pbrDiffuseFactor[3] : mat.pbrBaseColorFactor[3];
  k.slot        = sg ? mat.pbrDiffuseTexture : mat.pbrBaseColorTexture;
  if(k.slot > 0)
  {
    k.index    = infos[k.slot].index;
    k.texCoord = infos[k.slot].texCoord;
  }
  return k;
}

// What a material bakes into the triangles of the instances that use it (MiPt::matInstFlags; reference: getInstanceFlag, src/gltf_scene_rtx.cpp:271-295) ...
uint8_t materialInstFlags(const MiGltfShadeMaterial& mat)
{
  uint32_t f = 0;
  if(mat.transmissionFactor == 0.0f && mat.alphaMode == MI_ALPHA_OPAQUE && mat.diffuseTransmissionFactor == 0.0f)
    f |= pt::INST_FORCE_OPAQUE;
  if(mat.doubleSided == 1 || mat.thicknessFactor > 0.0f || mat.transmissionFactor > 0.0f)
    f |= pt::INST_CULL_DISABLE;
  if(mat.transmissionFactor > 0.01f)  // MIN_TRANSMISSION, shaders/pathtrace_functions.h.slang:36,256
    f |= pt::INST_TRANSMISSIVE;
  if(!(f & pt::INST_FORCE_OPAQUE) && mat.alphaMode == MI_ALPHA_OPAQUE)  // getOpacity == 1: the alpha draw always commits (pt_scene.h)
    f |= pt::INST_ALPHA_PASSES;
  return uint8_t(f);
}
// ... and what it asks of the shade kernels (MiPt::matFeatures)
uint8_t materialFeatures(const MiGltfShadeMaterial& mat)
{
  uint32_t g = 0;
  if(mat.multiscatterColorFactor[0] > 0.0f || mat.multiscatterColorFactor[1] > 0.0f || mat.multiscatterColorFactor[2] > 0.0f)
    g |= 1u;
  // the materials the specialised shade kernel cannot serve (see evaluateMaterial<SIMPLE>, pt_shading.h)
  if(mat.transmissionFactor != 0.0f || mat.diffuseTransmissionFactor != 0.0f || mat.clearcoatFactor != 0.0f || mat.iridescenceFactor != 0.0f
     || mat.anisotropyStrength > 0.0f || mat.retroreflectionFactor != 0.0f || mat.sheenColorFactor[0] != 0.0f || mat.sheenColorFactor[1] != 0.0f
     || mat.sheenColorFactor[2] != 0.0f)
    g |= 2u;
  return uint8_t(g);
}
// The 22 texture-info slots of every material must lie within the texture-info table: the kernels index it without further checks
bool materialSlotsInRange(const MiGltfShadeMaterial* materials, int numMaterials, int numTextureInfos, std::string& why)
{
  for(int m = 0; m < numMaterials; ++m)
  {
    const uint16_t* slots = &materials[m].pbrBaseColorTexture;  // the 22 texture-info slots are contiguous (mi_pt_shaderio.h)
    for(int k = 0; k < 22; ++k)
      if(int(slots[k]) >= numTextureInfos)
      {
        why = "material " + std::to_string(m) + " references texture info " + std::to_string(slots[k]) + " of " + std::to_string(numTextureInfos);
        return false;
      }
  }
  return true;
}
// Texture info + descriptor, flattened per texture slot (pt_scene.h: DevTexRef), and the five core map slots per material (DevCoreTex), in
// the order of the material's slot words: derived from the tables and the resident textures (MiPt::hostTextures), at creation and again at
// every material update (an animated uvTransform moves CT_TRANSFORM, a changed texCoord CT_TEXCOORD1).
void deriveTextureRecords(const MiPt* pt, const MiGltfShadeMaterial* materials, int numMaterials, const MiGltfTextureInfo* textureInfos, int numTextureInfos,
                          std::vector<pt::DevTexRef>& refs, std::vector<pt::DevCoreTex>& core)
{
  const int numTextures = int(pt->hostTextures.size());
  refs.assign(size_t(std::max(numTextureInfos, 1)), pt::DevTexRef{});
  memset(refs.data(), 0, refs.size() * sizeof(pt::DevTexRef));
  for(int i = 0; i < numTextureInfos; ++i)
  {
    const MiGltfTextureInfo& ti = textureInfos[i];
    pt::DevTexRef&           r  = refs[size_t(i)];
    memcpy(r.uv, ti.uvTransform, sizeof(r.uv));
    r.texCoord = uint8_t(ti.texCoord);
    if(ti.index >= 0 && ti.index < numTextures)
    {
      const pt::DevTexture& d = pt->hostTextures[size_t(ti.index)];
      r.level0 = d.levelOffset[0]; r.width = d.width; r.height = d.height; r.numLevels = d.numLevels; r.srgb = d.srgb;
      r.magFilter = d.magFilter; r.minFilter = d.minFilter; r.mipmapMode = d.mipmapMode; r.wrapS = d.wrapS; r.wrapT = d.wrapT;
    }
  }
  core.assign(size_t(std::max(numMaterials, 1)) * 5, pt::DevCoreTex{});
  memset(core.data(), 0, core.size() * sizeof(pt::DevCoreTex));
  static const float identityUv[6] = {1.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f};
  for(int m = 0; m < numMaterials; ++m)
  {
    const MiGltfShadeMaterial& M = materials[m];
    const uint16_t slots[5] = {M.pbrBaseColorTexture, M.normalTexture, M.pbrMetallicRoughnessTexture, M.emissiveTexture, M.occlusionTexture};
    for(int k = 0; k < 5; ++k)
    {
      pt::DevCoreTex& c = core[size_t(m) * 5 + size_t(k)];
      c.ref = slots[k];
      if(slots[k] == 0 || int(slots[k]) >= numTextureInfos)
        continue;
      const pt::DevTexRef& r = refs[slots[k]];
      c.level0 = r.level0;
      c.wh     = uint32_t(r.width) | (uint32_t(r.height) << 16);
      const bool fast = pt->sw.coreTex && r.width > 0 && r.magFilter == MI_FILTER_LINEAR && r.minFilter == MI_FILTER_LINEAR && r.wrapS != MI_WRAP_MIRRORED_REPEAT && r.wrapT != MI_WRAP_MIRRORED_REPEAT;
      c.flags  = (fast ? pt::CT_FAST : 0u) | (r.srgb ? pt::CT_SRGB : 0u) | (r.texCoord ? pt::CT_TEXCOORD1 : 0u) | (memcmp(r.uv, identityUv, sizeof(identityUv)) != 0 ? pt::CT_TRANSFORM : 0u)
                | (r.mipmapMode == MI_FILTER_LINEAR ? pt::CT_MIP_LINEAR : 0u) | (uint32_t(r.wrapS) << pt::CT_WRAPS_SHIFT) | (uint32_t(r.wrapT) << pt::CT_WRAPT_SHIFT)
                | (uint32_t(r.numLevels) << pt::CT_LEVELS_SHIFT);
    }
  }
}

// The scene-wide material summaries (instanceFlags sets them) select kernels and optional buffers: what an update that changed them -- the
// material tables (mi_pt_update_materials) or the render nodes' material ids (resident mode) -- owes the next render.  `hadTransmissive`,
// `wasSimple`: the summaries before the update.
int followSummaries(MiPt* pt, bool hadTransmissive, bool wasSimple)
{
  if(pt->simpleMaterials != wasSimple)  // the medium array comes back zeroed, on demand, when the generic shade kernel needs it (ensureOptionalPathArrays)
  {
    pt->optMedium.release();
    pt->paths.medium = nullptr;
  }
  if(pt->hasTransmissive != hadTransmissive)  // the candidate pool and lists are part of the path resources
  {
    pt->candPool.release();
    pt->candLists.release();
    if(pt->width > 0)
      return allocPathResources(pt, pt->framesCap);
  }
  return MI_PT_OK;
}

// The per-triangle data a build bakes of the materials, brought in place to what a build over the current tables writes: the instance flags
// `flags` (instanceFlags(pt), which also set pt->hasAlpha), the alpha-record buffer appearing or going with pt->hasAlpha, and one launch of
// k_patch_materials over the slots of the render nodes whose byte in `dirty` (pt::MATERIAL_PATCH_*, as wanted) is set -- none when no byte is.
// The alpha bit is dropped where there are no records to patch: none needed, or all of them made below as a build makes them.
int patchTriangleData(MiPt* pt, const std::vector<uint8_t>& flags, std::vector<uint8_t>& dirty)
{
  HIP_TRY(hipMemcpy(pt->instFlags.ptr, flags.data(), flags.size(), hipMemcpyHostToDevice));
  pt::DevScene& S          = pt->scene;
  const bool    hadRecords = pt->accel.alphaTris.ptr != nullptr;
  if(!pt->hasAlpha)
  {
    pt->accel.alphaTris.release();
    S.alphaTris = nullptr;
  }
  else if(!hadRecords)
    HIP_TRY(pt->accel.alphaTris.alloc(size_t(S.numTris)));
  bool anyDirty = false;
  for(uint8_t& d : dirty)
  {
    if(!(pt->hasAlpha && hadRecords))
      d &= uint8_t(~pt::MATERIAL_PATCH_ALPHA);
    anyDirty |= d != 0;
  }
  if(anyDirty)
  {
    if(pt->matDirty.count != dirty.size())
      HIP_TRY(pt->matDirty.alloc(dirty.size()));
    HIP_TRY(hipMemcpy(pt->matDirty.ptr, dirty.data(), dirty.size(), hipMemcpyHostToDevice));
    pt::launchPatchMaterials(S, pt->instFlags.ptr, pt->matDirty.ptr, pt->accel.bvhTris.ptr, hadRecords ? pt->accel.alphaTris.ptr : nullptr, pt->accel.shadeTris.ptr,
                             uint32_t(S.numTris), nullptr);
    HIP_TRY(hipGetLastError());
  }
  if(pt->hasAlpha && !hadRecords)  // the scene had no alpha records: all of them, as a build makes them
    if(int rc = makeAlphaRecords(pt))
      return rc;
  HIP_TRY(hipDeviceSynchronize());
  pt->sceneDevDirty = true;
  return MI_PT_OK;
}

// mi_pt_update_render_nodes in resident mode: matrices, visibility and material ids in one k_refit_tris pass, one level sweep and at most one
// patch launch; a build only for what the resident tree cannot take (a renderPrimID change, a transmissive bit under pre-split references,
// AUTO's cost bound).  The caller checked the arguments.
int updateRenderNodesResident(MiPt* pt, const MiGltfRenderNode* renderNodes, int numRenderNodes, const uint8_t* renderNodeVisible)
{
  const int            numMaterials = int(pt->matInstFlags.size()), numPrims = int(pt->hostPrims.size());
  const size_t         nn = size_t(numRenderNodes);
  std::vector<uint8_t> moved(nn, 0), visWas(nn, 1), matDirty(std::max<size_t>(nn, 1), 0);
  bool                 primChanged = false, visChanged = false, matChanged = false, anyMoved = false, transmissiveChanged = false;
  auto                 materialOf = [&](const MiGltfRenderNode& rn) { return size_t(std::max(0, std::min(rn.materialID, numMaterials - 1))); };
  for(size_t n = 0; n < nn; ++n)
  {
    const MiGltfRenderNode &was = pt->hostNodes[n], &now = renderNodes[n];
    visWas[n]         = pt->hostVisible.empty() || pt->hostVisible[n];
    const bool visNow = !renderNodeVisible || renderNodeVisible[n];
    visChanged |= (visWas[n] != 0) != visNow;
    primChanged |= was.renderPrimID != now.renderPrimID;
    moved[n] = memcmp(was.objectToWorld, now.objectToWorld, sizeof(float) * 32) != 0;
    anyMoved |= moved[n] != 0;
    if(was.materialID == now.materialID)
      continue;
    matChanged           = true;
    const size_t   mWas  = materialOf(was), mNow = materialOf(now);
    const AlphaKey kWas  = alphaKey(pt->hostMaterials[mWas], pt->hostTexInfos.data()), kNow = alphaKey(pt->hostMaterials[mNow], pt->hostTexInfos.data());
    const bool     alpha = memcmp(&kWas, &kNow, sizeof(AlphaKey)) != 0;
    const int      prim  = now.renderPrimID;
    // the OPAQUE class of the load-time alpha cut was found under the old alpha state (as in mi_pt_update_materials)
    if(alpha && prim >= 0 && prim < numPrims && pt->hostPrims[size_t(prim)].opaqueTriangles > 0)
      return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_render_nodes: material with another alpha state for geometry that was cut at load: re-cut and re-create (render node "
                                          + std::to_string(n) + ", material " + std::to_string(mNow) + ")");
    if(((pt->matInstFlags[mWas] ^ pt->matInstFlags[mNow]) & pt::INST_TRANSMISSIVE) != 0)
      transmissiveChanged = true;
    matDirty[n] = uint8_t(pt::MATERIAL_PATCH_SHADE | (alpha ? pt::MATERIAL_PATCH_ALPHA : 0));
  }
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // nothing in flight may still walk the old structure
  const bool                 hadTransmissive = pt->hasTransmissive, wasSimple = pt->simpleMaterials;
  const std::vector<uint8_t> flagsWas = matChanged ? instanceFlags(pt) : std::vector<uint8_t>();
  keepNodeTable(pt, renderNodes, numRenderNodes, renderNodeVisible);
  if(primChanged || (transmissiveChanged && pt->accel.splitRefs))
  {
    if(int rc = buildAcceleration(pt))
      return rc;
    return followSummaries(pt, hadTransmissive, wasSimple);
  }
  bool anyPrimDirty = false;
  for(uint8_t d : pt->accel.primDirty)
    anyPrimDirty |= d != 0;
  if(visChanged || anyMoved || anyPrimDirty || !matChanged)  // (an update that changes nothing refits, as it does outside resident mode)
  {
    if(int rc = refitAcceleration(pt, moved, &visWas))
      return rc;
    if(pt->accel.lastUpdate == MI_PT_ACCEL_LAST_BUILD)  // AUTO's bound: the build baked the materials
      return followSummaries(pt, hadTransmissive, wasSimple);
    if(visChanged)
      ++pt->accel.visibilityRefits;
  }
  if(!matChanged)
    return MI_PT_OK;
  const std::vector<uint8_t> flags = instanceFlags(pt);
  for(size_t n = 0; n < nn; ++n)
    if(matDirty[n] && flags[n] != flagsWas[n])
      matDirty[n] |= pt::MATERIAL_PATCH_FLAGS;
  // (the refit uploaded the node table; an update of material ids alone has not)
  HIP_TRY(hipMemcpy(pt->nodes.ptr, pt->hostNodes.data(), sizeof(MiGltfRenderNode) * nn, hipMemcpyHostToDevice));
  if(int rc = patchTriangleData(pt, flags, matDirty))
    return rc;
  ++pt->accel.materialPatches;
  pt->accel.lastUpdate = MI_PT_ACCEL_LAST_REFIT;
  return followSummaries(pt, hadTransmissive, wasSimple);
}

}  // namespace

extern "C" {

const char* mi_pt_last_error(void)
{
  return g_lastError.c_str();
}
// Issues the frames mi_pt_render_frame has been holding back (mi_pt_set_frame_queue) as ONE mi_pt_render_frames batch.  Every entry point that
// reads or changes what those frames depend on calls this first, so a caller never observes the deferral except through time.
static int flushPending(MiPt* pt)
{
  if(!pt || pt->frameQueue.pendingFrames == 0)
    return MI_PT_OK;
  const int n                  = pt->frameQueue.pendingFrames;
  pt->frameQueue.pendingFrames = 0;
  return mi_pt_render_frames(pt, &pt->frameQueue.pendingFirst, n, pt->frameQueue.pendingStream);
}
#define FLUSH_PENDING(pt)              \
  do                                   \
  {                                    \
    if(int rcFlush_ = flushPending(pt)) \
      return rcFlush_;                 \
  } while(0)

// ---- mi_pt_create in phases: the description is validated as a whole, then uploaded table by table ----------------------------------------
// Cross-table consistency (include/mi_pt.h: MI_PT_ERR_ARGUMENT for inconsistent tables).  The kernels index these tables
// without further checks, so a caller other than the in-tree loader gets an error here instead of a device fault.
// false: `why` is the message.  (The two limits on pool SIZES stand where the sizes are summed: uploadGeometry, uploadTextures.)
static bool validateSceneDesc(const MiPtSceneDesc* sd, std::string& why)
{
  auto refuse = [&](const std::string& message) {
    why = message;
    return false;
  };
  if(sd->numMaterials <= 0 || sd->numTextureInfos <= 0)
    return refuse("mi_pt_create: scene needs at least one material and the reserved texture-info slot 0");
  if(sd->numRenderNodes < 0 || sd->numRenderPrimitives < 0 || sd->numLights < 0 || sd->numTextures < 0 || sd->numMaterials > 65535 * 4
     || (sd->numRenderNodes > 0 && !sd->renderNodes) || (sd->numRenderPrimitives > 0 && !sd->renderPrimitives) || (sd->numLights > 0 && !sd->lights)
     || (sd->numTextures > 0 && !sd->textures) || !sd->materials || !sd->textureInfos)
    return refuse("mi_pt_create: negative table size or null table");
  for(int n = 0; n < sd->numRenderNodes; ++n)
  {
    const MiGltfRenderNode& rn = sd->renderNodes[n];
    if(rn.materialID >= sd->numMaterials)  // (negative ids mean "default material", reference: max(0, materialID))
      return refuse("mi_pt_create: render node " + std::to_string(n) + " references material " + std::to_string(rn.materialID) + " of "
                    + std::to_string(sd->numMaterials));
  }
  std::string slot;
  if(!materialSlotsInRange(sd->materials, sd->numMaterials, sd->numTextureInfos, slot))
    return refuse("mi_pt_create: " + slot);
  for(int i = 0; i < sd->numRenderPrimitives; ++i)
  {
    const MiPtRenderPrimitive& p = sd->renderPrimitives[i];
    if(p.vertexCount > 0 && !p.positions)
      return refuse("mi_pt_create: render primitive " + std::to_string(i) + " has vertices but no positions");
    if(p.triangleCount > 0 && !p.indices)
      return refuse("mi_pt_create: render primitive " + std::to_string(i) + " has triangles but no indices");
    for(size_t k = 0, n = size_t(p.triangleCount) * 3; k < n; ++k)
      if(p.indices[k] >= p.vertexCount)
        return refuse("mi_pt_create: render primitive " + std::to_string(i) + " has a vertex index beyond its vertexCount");
  }
  for(int i = 0; i < sd->numTextures; ++i)
  {
    const MiPtTexture& t = sd->textures[i];
    if(t.numLevels < 1 || t.numLevels > 16 || t.width < 1 || t.height < 1 || t.width > 65535 || t.height > 65535)
      return refuse("mi_pt_create: texture dimensions / level count out of range");
  }
  return true;
}

// The geometry pool: every index / attribute stream and the interleaved vertex copy, and the primitives' records that address them
static int uploadGeometry(MiPt* pt, const MiPtSceneDesc* sd)
{
  size_t geomBytes = 0;
  for(int i = 0; i < sd->numRenderPrimitives; ++i)
  {
    const MiPtRenderPrimitive& p = sd->renderPrimitives[i];
    geomBytes += align16(size_t(p.triangleCount) * 12);
    geomBytes += align16(size_t(p.vertexCount) * 12);
    if(p.normals) geomBytes += align16(size_t(p.vertexCount) * 12);
    if(p.colors) geomBytes += align16(size_t(p.vertexCount) * 4);
    if(p.tangents) geomBytes += align16(size_t(p.vertexCount) * 16);
    if(p.texCoords0) geomBytes += align16(size_t(p.vertexCount) * 8);
    if(p.texCoords1) geomBytes += align16(size_t(p.vertexCount) * 8);
    geomBytes += align16(size_t(p.vertexCount) * 48);  // interleaved copy (DevPrim::verts)
  }
  if(geomBytes / 16 >= (size_t(1) << 32))  // DevShadeTri addresses vertices as 32-bit float4 indices into this pool
    return fail(MI_PT_ERR_ARGUMENT, "the geometry pool exceeds 64 GiB");
  HIP_TRY(pt->geometry.alloc(std::max<size_t>(geomBytes, 16)));
  std::vector<uint8_t>     staging(std::max<size_t>(geomBytes, 16));
  std::vector<pt::DevPrim> devPrims(size_t(sd->numRenderPrimitives));
  {
    size_t off = 0;
    auto   put = [&](const void* src, size_t bytes) -> const uint8_t* {
      if(!src || bytes == 0)
        return nullptr;
      memcpy(staging.data() + off, src, bytes);
      const uint8_t* d = pt->geometry.ptr + off;
      off += align16(bytes);
      return d;
    };
    for(int i = 0; i < sd->numRenderPrimitives; ++i)
    {
      const MiPtRenderPrimitive& p = sd->renderPrimitives[i];
      pt::DevPrim&               d = devPrims[size_t(i)];
      d.indices    = reinterpret_cast<const uint32_t*>(put(p.indices, size_t(p.triangleCount) * 12));
      d.positions  = reinterpret_cast<const float*>(put(p.positions, size_t(p.vertexCount) * 12));
      d.normals    = reinterpret_cast<const float*>(put(p.normals, size_t(p.vertexCount) * 12));
      d.colors     = reinterpret_cast<const uint32_t*>(put(p.colors, size_t(p.vertexCount) * 4));
      d.tangents   = reinterpret_cast<const float*>(put(p.tangents, size_t(p.vertexCount) * 16));
      d.texCoords0 = reinterpret_cast<const float*>(put(p.texCoords0, size_t(p.vertexCount) * 8));
      d.texCoords1 = reinterpret_cast<const float*>(put(p.texCoords1, size_t(p.vertexCount) * 8));
      d.opaqueTriangles = pt->sw.noOpaqueTris ? 0u : std::min(p.opaqueTriangleCount, p.triangleCount);  // (test switch: alpha-test them all -- same image)
      d._pad            = 0;
      {
        std::vector<float> iv(size_t(p.vertexCount) * 12, 0.0f);
        for(uint32_t v = 0; v < p.vertexCount; ++v)
        {
          float* o = &iv[size_t(v) * 12];
          o[0] = p.positions[3 * size_t(v)]; o[1] = p.positions[3 * size_t(v) + 1]; o[2] = p.positions[3 * size_t(v) + 2];
          if(p.normals) { o[3] = p.normals[3 * size_t(v)]; o[4] = p.normals[3 * size_t(v) + 1]; o[5] = p.normals[3 * size_t(v) + 2]; }
          if(p.texCoords0) { o[6] = p.texCoords0[2 * size_t(v)]; o[7] = p.texCoords0[2 * size_t(v) + 1]; }
          if(p.tangents) memcpy(o + 8, p.tangents + 4 * size_t(v), 16);
        }
        d.verts = reinterpret_cast<const float4*>(put(iv.data(), iv.size() * sizeof(float)));
      }
    }
    HIP_TRY(hipMemcpy(pt->geometry.ptr, staging.data(), staging.size(), hipMemcpyHostToDevice));
  }
  HIP_TRY(pt->prims.upload(devPrims.data(), devPrims.size()));
  pt->hostPrims = devPrims;
  for(int i = 0; i < sd->numRenderPrimitives; ++i)
    pt->primVertices.push_back(sd->renderPrimitives[i].vertexCount);
  return MI_PT_OK;
}

// The host copies of what the acceleration structure is built from (see buildAcceleration) and of what the material updates diff against
static void keepHostTables(MiPt* pt, const MiPtSceneDesc* sd)
{
  pt->hostNodes.assign(sd->renderNodes, sd->renderNodes + sd->numRenderNodes);
  if(sd->renderNodeVisible)
    pt->hostVisible.assign(sd->renderNodeVisible, sd->renderNodeVisible + sd->numRenderNodes);
  pt->matInstFlags.resize(size_t(sd->numMaterials));
  pt->matFeatures.resize(size_t(sd->numMaterials));
  pt->hostMaterials.assign(sd->materials, sd->materials + sd->numMaterials);
  pt->hostTexInfos.assign(sd->textureInfos, sd->textureInfos + sd->numTextureInfos);
  for(int m = 0; m < sd->numMaterials; ++m)
  {
    pt->matInstFlags[size_t(m)] = materialInstFlags(sd->materials[m]);
    pt->matFeatures[size_t(m)]  = materialFeatures(sd->materials[m]);
  }
  pt->primTriangles.resize(size_t(sd->numRenderPrimitives));
  for(int i = 0; i < sd->numRenderPrimitives; ++i)
  {
    const MiPtRenderPrimitive& rp = sd->renderPrimitives[i];
    pt->primTriangles[size_t(i)]  = (rp.positions && rp.indices) ? rp.triangleCount : 0u;
  }
}

// Textures: one RGBA8 pool with all mip chains, the bilinear footprints, the per-slot records of the materials, and the sRGB table
static int uploadTextures(MiPt* pt, const MiPtSceneDesc* sd)
{
  std::vector<pt::DevTexture> dt(size_t(sd->numTextures));
  size_t                      totalTexels = 0;
  for(int i = 0; i < sd->numTextures; ++i)
    for(int l = 0; l < sd->textures[i].numLevels; ++l)  // (sizes and level counts are in range: validateSceneDesc)
      totalTexels += levelExtent(sd->textures[i], l).texels;
  if(totalTexels > 0xffffffffull)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_create: texture pool exceeds 2^32 texels");
  std::vector<uchar4> pool(std::max<size_t>(totalTexels, 1));
  size_t              off = 0;
  for(int i = 0; i < sd->numTextures; ++i)
  {
    const MiPtTexture& t = sd->textures[i];
    pt::DevTexture&    d = dt[size_t(i)];
    memset(&d, 0, sizeof(d));
    d.width = uint16_t(t.width); d.height = uint16_t(t.height); d.numLevels = uint8_t(t.numLevels); d.srgb = uint8_t(t.srgb ? 1 : 0);
    d.magFilter = uint8_t(t.magFilter); d.minFilter = uint8_t(t.minFilter); d.mipmapMode = uint8_t(t.mipmapMode);
    d.wrapS = uint8_t(t.wrapS); d.wrapT = uint8_t(t.wrapT);
    for(int l = 0; l < t.numLevels; ++l)
    {
      const size_t n   = levelExtent(t, l).texels;
      d.levelOffset[l] = uint32_t(off);
      memcpy(&pool[off], t.levels[l], n * 4);
      off += n;
    }
  }
  HIP_TRY(pt->textures.upload(dt.data(), dt.size()));
  HIP_TRY(pt->texels.upload(pool.data(), pool.size()));
  // bilinear footprints (pt_scene.h: texQuads), built on the device from the pool just uploaded; MI_PT_DIAG_NO_QUADS=1: A/B switch
  if(totalTexels > 0 && !pt->sw.noQuads)
  {
    HIP_TRY(pt->texQuads.alloc(pool.size()));
    for(const pt::DevTexture& d : dt)
      for(int l = 0; l < d.numLevels; ++l)
        pt::launchTextureQuads(pt->texels.ptr, pt->texQuads.ptr, d.levelOffset[l], levelExtent(d, l).w, levelExtent(d, l).h, d.wrapS, d.wrapT, nullptr);
    HIP_TRY(hipGetLastError());
  }
  pt->hostTextures = dt;
  std::vector<pt::DevTexRef>  refs;
  std::vector<pt::DevCoreTex> core;
  deriveTextureRecords(pt, sd->materials, sd->numMaterials, sd->textureInfos, sd->numTextureInfos, refs, core);
  HIP_TRY(pt->texRefs.upload(refs.data(), refs.size()));
  HIP_TRY(pt->coreTex.upload(core.data(), core.size()));
  // sRGB decode table of the texel fetch
  float lut[256];
  for(int i = 0; i < 256; ++i)
  {
    float c = float(i) / 255.0f;
    lut[i]  = c <= 0.04045f ? c / 12.92f : std::pow((c + 0.055f) / 1.055f, 2.4f);
  }
  HIP_TRY(pt->srgbLut.upload(lut, 256));
  return MI_PT_OK;
}

// The scene as the kernels see it; the acceleration structure's arrays follow with the build
static void describeScene(MiPt* pt, const MiPtSceneDesc* sd)
{
  pt::DevScene& S = pt->scene;
  S.materials = pt->materials.ptr; S.texInfos = pt->texInfos.ptr; S.nodes = pt->nodes.ptr; S.prims = pt->prims.ptr; S.lights = pt->lights.ptr;
  S.textures = pt->textures.ptr; S.texels = pt->texels.ptr; S.texQuads = pt->texQuads.ptr; S.envPixels = nullptr; S.envAccel = nullptr; S.bvhNodes = nullptr; S.bvh8Nodes = nullptr; S.bvh8Planes = nullptr; S.tris = nullptr;
  S.geomPool = reinterpret_cast<const float4*>(pt->geometry.ptr);
  S.texRefs = pt->texRefs.ptr; S.coreTex = reinterpret_cast<const uint4*>(pt->coreTex.ptr); S.alphaTris = nullptr; S.shadeTris = nullptr; S.srgbLut = pt->srgbLut.ptr; S.numMaterials = sd->numMaterials; S.numTextures = sd->numTextures;
  S.numLights = sd->numLights; S.numNodes = sd->numRenderNodes;
  S.envWidth = 0; S.envHeight = 0;
  S.packetInterval = pt->sw.packetInterval;  // A/B switch (LABNOTES.md section 2): 0 = the per-ray node test in every packet
  S.shadowOctFlip  = pt->sw.shadowFarFirst ? 7u : 0u;
}

// SkyPhysicalParameters{} defaults, so a caller that never calls mi_pt_set_sky still renders the default sky
static MiSkyPhysicalParameters defaultSky()
{
  MiSkyPhysicalParameters s{};
  s.rgbUnitConversion[0] = s.rgbUnitConversion[1] = s.rgbUnitConversion[2] = 1.0f / 80000.0f;
  s.multiplier = 0.1f; s.haze = 0.1f; s.redblueshift = 0.1f; s.saturation = 1.0f; s.groundColor[0] = s.groundColor[1] = s.groundColor[2] = 0.4f;
  s.horizonBlur = 0.3f; s.sunDiskIntensity = 1.0f; s.sunDirection[0] = s.sunDirection[1] = s.sunDirection[2] = 0.5773502691896258f;
  s.sunDiskScale = 1.0f; s.sunGlowIntensity = 1.0f; s.yIsUp = 1;
  return s;
}

int mi_pt_create(const MiPtSceneDesc* sd, const MiPtCreateOptions* options, MiPt** out)
{
  if(!sd || !out)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_create: null argument");
  int deviceCount = 0;
  if(hipGetDeviceCount(&deviceCount) != hipSuccess || deviceCount <= 0)
    return fail(MI_PT_ERR_NO_DEVICE, "mi_pt_create: no HIP device visible (this library has no CPU path)");
  const int device = options ? options->device : 0;
  if(device < 0 || device >= deviceCount)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_create: bad device ordinal");
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  std::string why;
  if(!validateSceneDesc(sd, why))
    return fail(MI_PT_ERR_ARGUMENT, why);

  // the phases of the scene build under the build-timing switch
  auto tPhase = BuildClock::now();
  auto phase  = [&](const char* what) {
    if(!buildTiming())
      return;
    (void)hipDeviceSynchronize();
    printBuildTiming(what, tPhase);
    tPhase = BuildClock::now();
  };

  std::unique_ptr<MiPt> pt(new MiPt());
  pt->sw.read();
  if(pt->sw.collapseBad)
    return fail(MI_PT_ERR_ARGUMENT, std::string("MI_PT_COLLAPSE=") + getenv("MI_PT_COLLAPSE") + " is neither \"sah\" nor \"greedy\"");
  pt->device          = device;
  pt->numCUs          = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  pt->collectCounters = options && options->collectCounters;

  HIP_TRY(pt->materials.upload(sd->materials, size_t(sd->numMaterials)));
  HIP_TRY(pt->texInfos.upload(sd->textureInfos, size_t(sd->numTextureInfos)));
  HIP_TRY(pt->nodes.upload(sd->renderNodes, size_t(sd->numRenderNodes)));
  HIP_TRY(pt->lights.upload(sd->lights, size_t(sd->numLights)));

  if(int rc = uploadGeometry(pt.get(), sd))
    return rc;
  phase("tables + geometry upload");

  keepHostTables(pt.get(), sd);
  pt->accel.bvhBuilder = options ? options->bvhBuilder : 0;
  if(int rc = uploadTextures(pt.get(), sd))
    return rc;
  phase("textures upload");

  describeScene(pt.get(), sd);
  if(int rc = buildAcceleration(pt.get()))
    return rc;
  phase("shade / alpha records");
  HIP_TRY(pt->stats.alloc(1));
  HIP_TRY(hipMemset(pt->stats.ptr, 0, sizeof(pt::StatCounters)));
  pt->sky = defaultSky();
  *out    = pt.release();
  return MI_PT_OK;
}

int mi_pt_update_render_nodes(MiPt* pt, const MiGltfRenderNode* renderNodes, int numRenderNodes, const uint8_t* renderNodeVisible)
{
  FLUSH_PENDING(pt);
  if(!pt || !renderNodes || numRenderNodes != int(pt->hostNodes.size()))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_render_nodes: the render-node count must be the one the instance was created with");
  for(int n = 0; n < numRenderNodes; ++n)
    if(renderNodes[n].materialID >= int(pt->matInstFlags.size()))
      return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_render_nodes: render node references a material beyond the table");
  if(residentInForce(pt))
    return updateRenderNodesResident(pt, renderNodes, numRenderNodes, renderNodeVisible);
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // nothing in flight may still walk the old structure
  // what changed: matrices only (a refit may follow), or primitives, materials or visibility (a rebuild)
  bool                 sameTopology = true;
  std::vector<uint8_t> moved(size_t(numRenderNodes), 0);
  for(int n = 0; n < numRenderNodes; ++n)
  {
    const MiGltfRenderNode &was = pt->hostNodes[size_t(n)], &now = renderNodes[n];
    const bool              visWas = pt->hostVisible.empty() || pt->hostVisible[size_t(n)], visNow = !renderNodeVisible || renderNodeVisible[n];
    if(was.materialID != now.materialID || was.renderPrimID != now.renderPrimID || visWas != visNow)
      sameTopology = false;
    moved[size_t(n)] = memcmp(was.objectToWorld, now.objectToWorld, sizeof(float) * 32) != 0;
  }
  keepNodeTable(pt, renderNodes, numRenderNodes, renderNodeVisible);
  return updateAcceleration(pt, sameTopology, moved);
}

int mi_pt_update_lights(MiPt* pt, const MiGltfLight* lights, int numLights)
{
  FLUSH_PENDING(pt);
  if(!pt || numLights != pt->scene.numLights || (numLights > 0 && !lights))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_lights: the light count must be the one the instance was created with");
  if(numLights == 0)
    return MI_PT_OK;
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // frames in flight still sample the old table
  HIP_TRY(hipMemcpy(pt->lights.ptr, lights, sizeof(MiGltfLight) * size_t(numLights), hipMemcpyHostToDevice));
  return MI_PT_OK;
}

int mi_pt_update_materials(MiPt* pt, const MiGltfShadeMaterial* materials, int numMaterials, const MiGltfTextureInfo* textureInfos, int numTextureInfos)
{
  FLUSH_PENDING(pt);
  if(!pt || !materials || !textureInfos || numMaterials != int(pt->hostMaterials.size()))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_materials: the material count must be the one the instance was created with");
  if(numTextureInfos <= 0)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_materials: the texture-info table needs the reserved slot 0");
  {
    std::string why;
    if(!materialSlotsInRange(materials, numMaterials, numTextureInfos, why))
      return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_materials: " + why);
  }
  // ---- the diff, per material: what of the per-triangle data a build baked from it is now stale
  const size_t         nm = size_t(numMaterials);
  std::vector<uint8_t> newFlags(nm), newFeatures(nm), alphaChanged(nm, 0), flagsChanged(nm, 0);
  bool                 anyAlpha = false, anyFlags = false, transmissiveChanged = false;
  for(size_t m = 0; m < nm; ++m)
  {
    newFlags[m]    = materialInstFlags(materials[m]);
    newFeatures[m] = materialFeatures(materials[m]);
    const AlphaKey was = alphaKey(pt->hostMaterials[m], pt->hostTexInfos.data()), now = alphaKey(materials[m], textureInfos);
    alphaChanged[m] = memcmp(&was, &now, sizeof(AlphaKey)) != 0;
    flagsChanged[m] = newFlags[m] != pt->matInstFlags[m];
    anyAlpha |= alphaChanged[m] != 0;
    anyFlags |= flagsChanged[m] != 0;
  }
  const int numNodes = int(pt->hostNodes.size()), numPrims = int(pt->hostPrims.size());
  auto      materialOf = [&](int n) { return size_t(std::max(0, std::min(pt->hostNodes[size_t(n)].materialID, numMaterials - 1))); };
  for(int n = 0; n < numNodes; ++n)
  {
    const size_t m    = materialOf(n);
    const int    prim = pt->hostNodes[size_t(n)].renderPrimID;
    // the OPAQUE class of the load-time alpha cut was found under the old alpha state: its triangles skip the alpha test for good
    if(alphaChanged[m] && prim >= 0 && prim < numPrims && pt->hostPrims[size_t(prim)].opaqueTriangles > 0)
      return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_materials: alpha state of a material whose geometry was cut at load: re-cut and re-create (material "
                                          + std::to_string(m) + ", render node " + std::to_string(n) + ")");
    if(((newFlags[m] ^ pt->matInstFlags[m]) & pt::INST_TRANSMISSIVE) != 0)
      transmissiveChanged = true;
  }
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // frames in flight still shade with the old tables
  // ---- the tables, and what is derived from them per texture slot and per material
  {
    std::vector<pt::DevTexRef>  refs;
    std::vector<pt::DevCoreTex> core;
    deriveTextureRecords(pt, materials, numMaterials, textureInfos, numTextureInfos, refs, core);
    if(size_t(numTextureInfos) != pt->texInfos.count)  // (the table grew or shrank: new buffers, taken over only when both exist)
    {
      DevBuf<MiGltfTextureInfo> infos;
      DevBuf<pt::DevTexRef>     drefs;
      HIP_TRY(infos.upload(textureInfos, size_t(numTextureInfos)));
      HIP_TRY(drefs.upload(refs.data(), refs.size()));
      std::swap(pt->texInfos.ptr, infos.ptr); std::swap(pt->texInfos.count, infos.count);
      std::swap(pt->texRefs.ptr, drefs.ptr); std::swap(pt->texRefs.count, drefs.count);
      pt->scene.texInfos = pt->texInfos.ptr;
      pt->scene.texRefs  = pt->texRefs.ptr;
    }
    else
    {
      HIP_TRY(hipMemcpy(pt->texInfos.ptr, textureInfos, sizeof(MiGltfTextureInfo) * size_t(numTextureInfos), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(pt->texRefs.ptr, refs.data(), sizeof(pt::DevTexRef) * refs.size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(pt->materials.ptr, materials, sizeof(MiGltfShadeMaterial) * nm, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pt->coreTex.ptr, core.data(), sizeof(pt::DevCoreTex) * core.size(), hipMemcpyHostToDevice));
  }
  pt->hostMaterials.assign(materials, materials + numMaterials);
  pt->hostTexInfos.assign(textureInfos, textureInfos + numTextureInfos);
  pt->matInstFlags = newFlags;
  pt->matFeatures  = newFeatures;
  pt->sceneDevDirty = true;
  // ---- the scene-wide summaries, and the buffers they call for at the next render
  const bool hadTransmissive = pt->hasTransmissive, wasSimple = pt->simpleMaterials;
  const std::vector<uint8_t> flags = instanceFlags(pt);
  // ---- what the resident structure cannot take in place is rebuilt: the BVH2 walk (no patch path), and a transmissive bit that changes
  // while the tree holds pre-split references (triangles of transmissive instances keep ONE reference: bvh_build.hip, k_split_refs)
  if((anyAlpha || anyFlags) && pt->scene.numTris > 0 && (!pt->accel.wide || (transmissiveChanged && pt->accel.splitRefs)))
  {
    if(int rc = buildAcceleration(pt))
      return rc;
    return followSummaries(pt, hadTransmissive, wasSimple);
  }
  if(pt->scene.numTris > 0)
  {
    // the dirty byte of every render node, from its material's classes; no launch when no byte is set (factor-only and UV-transform updates)
    std::vector<uint8_t> dirty(size_t(std::max(numNodes, 1)), 0);
    for(int n = 0; n < numNodes; ++n)
    {
      const size_t m = materialOf(n);
      dirty[size_t(n)] = uint8_t((flagsChanged[m] ? pt::MATERIAL_PATCH_FLAGS : 0) | (alphaChanged[m] ? pt::MATERIAL_PATCH_ALPHA : 0));
    }
    if(int rc = patchTriangleData(pt, flags, dirty))
      return rc;
  }
  return followSummaries(pt, hadTransmissive, wasSimple);
}

int mi_pt_set_deformation(MiPt* pt, const MiPtDeformDesc* desc)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_deformation: null instance");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  if(!desc)
  {
    pt->deform = MiPt::Deformation{};
    return allocVertexMotion(pt);
  }
  const int numPrims = int(pt->primVertices.size());
  if(desc->numPrims < 0 || desc->numJointMatrices < 0 || desc->numMorphWeights < 0 || (desc->numPrims > 0 && !desc->prims))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_deformation: negative count or null primitive table");
  // ---- validation: the kernel indexes everything below without further checks
  std::vector<uint8_t> seen(size_t(numPrims), 0);
  size_t               poolBytes = 0;
  uint64_t             blocks    = 0;
  for(int k = 0; k < desc->numPrims; ++k)
  {
    const MiPtDeformPrimitive& d   = desc->prims[k];
    const std::string          who = "mi_pt_set_deformation: primitive " + std::to_string(k) + ": ";
    if(d.renderPrimID < 0 || d.renderPrimID >= numPrims)
      return fail(MI_PT_ERR_ARGUMENT, who + "render primitive " + std::to_string(d.renderPrimID) + " out of range");
    if(seen[size_t(d.renderPrimID)]++)
      return fail(MI_PT_ERR_ARGUMENT, who + "render primitive " + std::to_string(d.renderPrimID) + " listed twice");
    if(pt->vu.set && pt->vu.declared[size_t(d.renderPrimID)])
      return fail(MI_PT_ERR_ARGUMENT, who + "render primitive " + std::to_string(d.renderPrimID) + " is driven by the caller (mi_pt_set_vertex_updates)");
    const pt::DevPrim& rp = pt->hostPrims[size_t(d.renderPrimID)];
    if(d.vertexCount != pt->primVertices[size_t(d.renderPrimID)])
      return fail(MI_PT_ERR_ARGUMENT, who + "vertexCount differs from the resident primitive's");
    if(!d.basePositions || !rp.positions)
      return fail(MI_PT_ERR_ARGUMENT, who + "no base positions");
    if((d.baseNormals && !rp.normals) || (d.baseTangents && !rp.tangents))
      return fail(MI_PT_ERR_ARGUMENT, who + "a base stream the resident primitive does not have");
    if(!d.joints != !d.weights)
      return fail(MI_PT_ERR_ARGUMENT, who + "joints and weights go together");
    if(d.joints && uint64_t(d.jointMatrixOffset) + d.numJoints > uint64_t(desc->numJointMatrices))
      return fail(MI_PT_ERR_ARGUMENT, who + "joint matrices beyond the table");
    if(d.numTargets > 0 && (!d.positionDeltas || uint64_t(d.morphWeightOffset) + d.numTargets > uint64_t(desc->numMorphWeights)))
      return fail(MI_PT_ERR_ARGUMENT, who + "morph targets without position deltas, or weights beyond the table");
    if((d.normalDeltas && !d.baseNormals) || (d.tangentDeltas && !d.baseTangents))
      return fail(MI_PT_ERR_ARGUMENT, who + "normal / tangent deltas need the base stream");
    if(!d.joints && d.numTargets == 0)
      return fail(MI_PT_ERR_ARGUMENT, who + "neither skinned nor morphed");
    const size_t nv = d.vertexCount;
    poolBytes += align16(nv * 48);
    if(d.joints)
      poolBytes += align16(nv * 8) + align16(nv * 16);
    const size_t deltaBytes = nv * 12 * d.numTargets;
    poolBytes += d.numTargets ? align16(deltaBytes) * (1 + (d.normalDeltas ? 1 : 0) + (d.tangentDeltas ? 1 : 0)) : 0;
    blocks += (nv + pt::DEFORM_BLOCK - 1) / pt::DEFORM_BLOCK;
  }
  if(blocks > 0x7fffffffull)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_deformation: too many vertices");
  pt->deform = MiPt::Deformation{};
  if(desc->numPrims == 0)
    return allocVertexMotion(pt);
  // ---- static upload: base poses (in the layout of DevPrim::verts, from the resident record: uv0 and the stream values that are not
  // deformed keep theirs), influences, deltas
  HIP_TRY(pt->deform.pool.alloc(std::max<size_t>(poolBytes, 16)));
  std::vector<uint8_t>        staging(std::max<size_t>(poolBytes, 16), 0);
  std::vector<pt::DeformTask> tasks(size_t(desc->numPrims));
  std::vector<uint32_t>       blockTask;
  size_t                      off = 0;
  auto                        put = [&](const void* src, size_t bytes) -> const uint8_t* {
    memcpy(staging.data() + off, src, bytes);
    const uint8_t* d = pt->deform.pool.ptr + off;
    off += align16(bytes);
    return d;
  };
  HIP_TRY(pt->deform.joints.alloc(size_t(std::max(desc->numJointMatrices, 1)) * 6));
  HIP_TRY(pt->deform.weights.alloc(size_t(std::max(desc->numMorphWeights, 1))));
  for(int k = 0; k < desc->numPrims; ++k)
  {
    const MiPtDeformPrimitive& d  = desc->prims[k];
    const pt::DevPrim&         rp = pt->hostPrims[size_t(d.renderPrimID)];
    const size_t               nv = d.vertexCount;
    std::vector<float>         base(nv * 12);
    HIP_TRY(hipMemcpy(base.data(), rp.verts, nv * 48, hipMemcpyDeviceToHost));
    for(size_t v = 0; v < nv; ++v)
    {
      float* o = &base[v * 12];
      memcpy(o, d.basePositions + v * 3, 12);
      if(d.baseNormals) { o[3] = d.baseNormals[v * 3]; o[4] = d.baseNormals[v * 3 + 1]; o[5] = d.baseNormals[v * 3 + 2]; }
      if(d.baseTangents) memcpy(o + 8, d.baseTangents + v * 4, 16);
    }
    pt::DeformTask& t = tasks[size_t(k)];
    memset(&t, 0, sizeof(t));
    t.base = reinterpret_cast<const float4*>(put(base.data(), nv * 48));
    if(d.joints)
    {
      t.joints  = reinterpret_cast<const uint2*>(put(d.joints, nv * 8));
      t.weights = reinterpret_cast<const float4*>(put(d.weights, nv * 16));
      t.flags |= pt::DF_SKIN;
      t.numJoints  = d.numJoints;
      t.jointTable = pt->deform.joints.ptr + size_t(d.jointMatrixOffset) * 6;
    }
    if(d.numTargets)
    {
      t.numTargets   = d.numTargets;
      t.morphWeights = pt->deform.weights.ptr + d.morphWeightOffset;
      t.posDeltas    = reinterpret_cast<const float*>(put(d.positionDeltas, nv * 12 * d.numTargets));
      if(d.normalDeltas)
      {
        t.nrmDeltas = reinterpret_cast<const float*>(put(d.normalDeltas, nv * 12 * d.numTargets));
        t.flags |= pt::DF_MORPH_N;
      }
      if(d.tangentDeltas)
      {
        t.tanDeltas = reinterpret_cast<const float*>(put(d.tangentDeltas, nv * 12 * d.numTargets));
        t.flags |= pt::DF_MORPH_T;
      }
    }
    if(d.baseNormals)
      t.flags |= pt::DF_NORMALS;
    if(d.baseTangents)
      t.flags |= pt::DF_TANGENTS;
    t.outPositions = const_cast<float*>(rp.positions);
    t.outNormals   = const_cast<float*>(rp.normals);
    t.outTangents  = const_cast<float*>(rp.tangents);
    t.outVerts     = const_cast<float4*>(rp.verts);
    t.vertexCount  = uint32_t(nv);
    t.firstBlock   = uint32_t(blockTask.size());
    for(size_t b = 0; b < (nv + pt::DEFORM_BLOCK - 1) / pt::DEFORM_BLOCK; ++b)
      blockTask.push_back(uint32_t(k));
  }
  HIP_TRY(hipMemcpy(pt->deform.pool.ptr, staging.data(), staging.size(), hipMemcpyHostToDevice));
  HIP_TRY(pt->deform.tasks.upload(tasks.data(), tasks.size()));
  HIP_TRY(pt->deform.blockTask.upload(blockTask.data(), blockTask.size()));
  pt->deform.jointCount  = desc->numJointMatrices;
  pt->deform.weightCount = desc->numMorphWeights;
  pt->deform.blocks      = uint32_t(blockTask.size());
  pt->deform.set         = true;
  for(int k = 0; k < desc->numPrims; ++k)
    pt->deform.primIDs.push_back(desc->prims[k].renderPrimID);
  return allocVertexMotion(pt);  // (new tables: the previous-pose positions of vertex motion start from the resident ones again)
}

int mi_pt_update_deformation(MiPt* pt, const float* jointMatrices, const float* morphWeights, int flags)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_deformation: null instance");
  if(!pt->deform.set)
    return fail(MI_PT_ERR_STATE, "mi_pt_update_deformation: no deformation set (mi_pt_set_deformation)");
  if((pt->deform.jointCount > 0 && !jointMatrices) || (pt->deform.weightCount > 0 && !morphWeights))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_deformation: null table");
  for(size_t i = 0, n = size_t(pt->deform.jointCount) * 16; i < n; ++i)
    if(!std::isfinite(jointMatrices[i]))
      return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_deformation: non-finite joint matrix");
  for(int i = 0; i < pt->deform.weightCount; ++i)
    if(!std::isfinite(morphWeights[i]))
      return fail(MI_PT_ERR_ARGUMENT, "mi_pt_update_deformation: non-finite morph weight");
  // joint table: rows 0-2 of J (the last row of J [p, 1] is never read) and of N = transpose(inverse(mat3(J))), the cofactor matrix / det
  std::vector<float4> table(size_t(std::max(pt->deform.jointCount, 1)) * 6, make_float4(0, 0, 0, 0));
  for(int j = 0; j < pt->deform.jointCount; ++j)
  {
    const float* M = jointMatrices + size_t(j) * 16;  // column-major: M[c * 4 + r]
    float4*      o = &table[size_t(j) * 6];
    for(int r = 0; r < 3; ++r)
      o[r] = make_float4(M[r], M[4 + r], M[8 + r], M[12 + r]);
    const float a = M[0], b = M[4], c = M[8], e = M[1], f = M[5], g = M[9], h = M[2], i = M[6], k = M[10];
    const float det = a * (f * k - g * i) - b * (e * k - g * h) + c * (e * i - f * h);
    const float id  = 1.0f / det;
    o[3] = make_float4((f * k - g * i) * id, -(e * k - g * h) * id, (e * i - f * h) * id, 0.0f);
    o[4] = make_float4(-(b * k - c * i) * id, (a * k - c * h) * id, -(a * i - b * h) * id, 0.0f);
    o[5] = make_float4((b * g - c * f) * id, -(a * g - c * e) * id, (a * f - b * e) * id, 0.0f);
  }
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // frames in flight still read the old pose
  const auto t0 = BuildClock::now();
  HIP_TRY(hipMemcpy(pt->deform.joints.ptr, table.data(), table.size() * sizeof(float4), hipMemcpyHostToDevice));
  if(pt->deform.weightCount > 0)
    HIP_TRY(hipMemcpy(pt->deform.weights.ptr, morphWeights, sizeof(float) * size_t(pt->deform.weightCount), hipMemcpyHostToDevice));
  pt::launchDeform(pt->deform.tasks.ptr, pt->deform.blockTask.ptr, pt->deform.blocks, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  printBuildTiming("deform", t0);
  pt->vm.poseDirty = true;  // (vertex motion: the next rendered pose is followed by a snapshot of the positions)
  for(int id : pt->deform.primIDs)  // (what the next acceleration update refits; sized by a build that kept refit data)
    if(size_t(id) < pt->accel.primDirty.size())
      pt->accel.primDirty[size_t(id)] = pt->accel.primDeformed[size_t(id)] = 1;
  if(flags & MI_PT_DEFORM_DEFER_BUILD)
    return MI_PT_OK;
  return updateAcceleration(pt, true, std::vector<uint8_t>(pt->hostNodes.size(), 0));
}

int mi_pt_set_vertex_updates(MiPt* pt, const int32_t* renderPrimIDs, int count, int flags)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_vertex_updates: null instance");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  if(count < 0 || (flags & ~MI_PT_VERTICES_RECOMPUTE_NORMALS))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_vertex_updates: negative count or unknown flag bits");
  if(count == 0 || !renderPrimIDs)
  {
    pt->vu = MiPt::VertexUpdates{};
    return allocVertexMotion(pt);
  }
  // ---- validation: the kernels index everything below without further checks
  const int            numPrims = int(pt->primVertices.size());
  std::vector<uint8_t> declared(size_t(numPrims), 0);
  uint64_t             blocks = 0, tableWords = 0;
  for(int k = 0; k < count; ++k)
  {
    const int         id  = renderPrimIDs[k];
    const std::string who = "mi_pt_set_vertex_updates: render primitive " + std::to_string(id);
    if(id < 0 || id >= numPrims)
      return fail(MI_PT_ERR_ARGUMENT, who + " out of range");
    if(declared[size_t(id)]++)
      return fail(MI_PT_ERR_ARGUMENT, who + " listed twice");
    if(std::find(pt->deform.primIDs.begin(), pt->deform.primIDs.end(), id) != pt->deform.primIDs.end())
      return fail(MI_PT_ERR_ARGUMENT, who + " is deformed by the deformation tables (mi_pt_set_deformation)");
    const pt::DevPrim& rp = pt->hostPrims[size_t(id)];
    if(!rp.positions || pt->primVertices[size_t(id)] == 0)
      return fail(MI_PT_ERR_ARGUMENT, who + " has no positions");
    blocks += (uint64_t(pt->primVertices[size_t(id)]) + pt::VERTEX_UPDATE_BLOCK - 1) / pt::VERTEX_UPDATE_BLOCK;
    if((flags & MI_PT_VERTICES_RECOMPUTE_NORMALS) && rp.normals && rp.indices && pt->primTriangles[size_t(id)] > 0)
      tableWords += uint64_t(pt->primVertices[size_t(id)]) + uint64_t(pt->primTriangles[size_t(id)]) * 3;
  }
  if(blocks > 0x3fffffffull || tableWords > 0xffffffffull)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_vertex_updates: too many vertices or corners");
  // ---- the incident-corner tables (CSR, triangles in ascending order), from the resident index buffers
  std::vector<uint32_t> table;
  table.reserve(size_t(tableWords));
  std::vector<size_t> cornerEnd(size_t(numPrims), SIZE_MAX), corners(size_t(numPrims), SIZE_MAX);
  for(int k = 0; k < count && tableWords; ++k)
  {
    const size_t       id = size_t(renderPrimIDs[k]);
    const pt::DevPrim& rp = pt->hostPrims[id];
    const size_t       nv = pt->primVertices[id], nc = size_t(pt->primTriangles[id]) * 3;
    if(!rp.normals || !rp.indices || nc == 0)
      continue;
    std::vector<uint32_t> idx(nc);
    HIP_TRY(hipMemcpy(idx.data(), rp.indices, nc * sizeof(uint32_t), hipMemcpyDeviceToHost));
    cornerEnd[id] = table.size();
    corners[id]   = table.size() + nv;
    table.resize(table.size() + nv + nc, 0u);
    uint32_t* end = table.data() + cornerEnd[id];
    uint32_t* out = table.data() + corners[id];
    for(size_t c = 0; c < nc; ++c)  // (mi_pt_create checked every index against vertexCount)
      ++end[idx[c]];
    for(size_t v = 1; v < nv; ++v)
      end[v] += end[v - 1];
    std::vector<uint32_t> cursor(nv);
    for(size_t v = 0; v < nv; ++v)
      cursor[v] = v ? end[v - 1] : 0u;
    for(size_t c = 0; c < nc; ++c)
      out[cursor[idx[c]]++] = uint32_t(c);
  }
  // ---- commit: the new declaration replaces the old one only once it holds all its buffers
  MiPt::VertexUpdates fresh;
  HIP_TRY(fresh.table.upload(table.data(), table.size()));
  HIP_TRY(fresh.tasks.alloc(size_t(count)));
  HIP_TRY(fresh.normalTasks.alloc(size_t(count)));
  HIP_TRY(fresh.blockTask.alloc(size_t(blocks) * 2 + 1));
  fresh.blockCap = size_t(blocks);
  fresh.set      = true;
  fresh.primIDs.assign(renderPrimIDs, renderPrimIDs + count);
  fresh.declared  = std::move(declared);
  fresh.cornerEnd = std::move(cornerEnd);
  fresh.corners   = std::move(corners);
  pt->vu          = std::move(fresh);
  return allocVertexMotion(pt);  // (the declared primitives' previous-pose positions start from the resident ones)
}

// Both forms of an update call.  `device`: the stream pointers are device memory, read by the kernel where they lie.
static int updateVertices(MiPt* pt, const MiPtVertexUpdate* updates, int numUpdates, int flags, bool device, const char* name)
{
  const std::string fn = name;
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, fn + ": null instance");
  if(!pt->vu.set)
    return fail(MI_PT_ERR_STATE, fn + ": no primitives declared (mi_pt_set_vertex_updates)");
  if(numUpdates < 0 || (numUpdates > 0 && !updates) || (flags & ~MI_PT_DEFORM_DEFER_BUILD))
    return fail(MI_PT_ERR_ARGUMENT, fn + ": negative count, null table or unknown flag bits");
  // ---- validation: nothing changes when any primitive of the call is refused
  std::vector<uint8_t> seen(pt->vu.declared.size(), 0);
  size_t               stagingBytes = 0;
  for(int k = 0; k < numUpdates; ++k)
  {
    const MiPtVertexUpdate& u   = updates[k];
    const std::string       who = fn + ": update " + std::to_string(k) + ": ";
    if(u.renderPrimID < 0 || size_t(u.renderPrimID) >= pt->vu.declared.size() || !pt->vu.declared[size_t(u.renderPrimID)])
      return fail(MI_PT_ERR_ARGUMENT, who + "render primitive " + std::to_string(u.renderPrimID) + " is not declared");
    if(seen[size_t(u.renderPrimID)]++)
      return fail(MI_PT_ERR_ARGUMENT, who + "render primitive " + std::to_string(u.renderPrimID) + " listed twice");
    const pt::DevPrim& rp = pt->hostPrims[size_t(u.renderPrimID)];
    if(u.vertexCount != pt->primVertices[size_t(u.renderPrimID)])
      return fail(MI_PT_ERR_ARGUMENT, who + "vertexCount differs from the resident primitive's");
    if(!u.positions)
      return fail(MI_PT_ERR_ARGUMENT, who + "no positions");
    if((u.normals && !rp.normals) || (u.tangents && !rp.tangents))
      return fail(MI_PT_ERR_ARGUMENT, who + "a stream the resident primitive does not have");
    if(u.reserved[0] || u.reserved[1])
      return fail(MI_PT_ERR_ARGUMENT, who + "reserved words must be 0");
    const size_t nv = u.vertexCount;
    if(device)
    {
      if((reinterpret_cast<uintptr_t>(u.positions) | reinterpret_cast<uintptr_t>(u.normals) | reinterpret_cast<uintptr_t>(u.tangents)) & 3u)
        return fail(MI_PT_ERR_ARGUMENT, who + "a device pointer that is not 4-byte aligned");
      continue;
    }
    auto finite = [](const float* a, size_t n) {
      for(size_t i = 0; i < n; ++i)
        if(!std::isfinite(a[i]))
          return false;
      return true;
    };
    if(!finite(u.positions, nv * 3) || (u.normals && !finite(u.normals, nv * 3)) || (u.tangents && !finite(u.tangents, nv * 4)))
      return fail(MI_PT_ERR_ARGUMENT, who + "a non-finite component");
    stagingBytes += align16(nv * 12) + (u.normals ? align16(nv * 12) : 0) + (u.tangents ? align16(nv * 16) : 0);
  }
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // frames in flight still read the old vertices; the caller's streams have produced the device arrays
  const auto t0 = BuildClock::now();
  if(stagingBytes > pt->vuStaging.count)
    HIP_TRY(pt->vuStaging.alloc(stagingBytes));
  // ---- task tables: every primitive's vertex range padded to whole blocks, one launch (and one for the normals that are rebuilt)
  std::vector<uint8_t>               staging(stagingBytes);
  std::vector<pt::VertexUpdateTask>  tasks;
  std::vector<pt::NormalRebuildTask> normalTasks;
  std::vector<uint32_t>              blockTask, normalBlockTask;
  size_t                             off = 0;
  uint64_t                           vertices = 0;
  auto                               stage = [&](const float* src, size_t bytes) -> const float* {
    if(!src)
      return nullptr;
    if(device)
      return src;
    memcpy(staging.data() + off, src, bytes);
    const uint8_t* d = pt->vuStaging.ptr + off;
    off += align16(bytes);
    return reinterpret_cast<const float*>(d);
  };
  for(int k = 0; k < numUpdates; ++k)
  {
    const MiPtVertexUpdate& u  = updates[k];
    const size_t            id = size_t(u.renderPrimID);
    const pt::DevPrim&      rp = pt->hostPrims[id];
    const size_t            nv = u.vertexCount;
    const size_t            nb = (nv + pt::VERTEX_UPDATE_BLOCK - 1) / pt::VERTEX_UPDATE_BLOCK;
    pt::VertexUpdateTask    t{};
    t.positions    = stage(u.positions, nv * 12);
    t.normals      = stage(u.normals, nv * 12);
    t.tangents     = stage(u.tangents, nv * 16);
    t.outPositions = const_cast<float*>(rp.positions);
    t.outNormals   = const_cast<float*>(rp.normals);
    t.outTangents  = const_cast<float*>(rp.tangents);
    t.outVerts     = const_cast<float4*>(rp.verts);
    t.vertexCount  = uint32_t(nv);
    t.firstBlock   = uint32_t(blockTask.size());
    t.flags        = (u.normals ? pt::VU_NORMALS : 0u) | (u.tangents ? pt::VU_TANGENTS : 0u);
    blockTask.insert(blockTask.end(), nb, uint32_t(tasks.size()));
    tasks.push_back(t);
    vertices += nv;
    if(!u.normals && pt->vu.cornerEnd[id] != SIZE_MAX)
    {
      pt::NormalRebuildTask n{};
      n.positions   = rp.positions;
      n.indices     = rp.indices;
      n.cornerEnd   = pt->vu.table.ptr + pt->vu.cornerEnd[id];
      n.corners     = pt->vu.table.ptr + pt->vu.corners[id];
      n.outNormals  = const_cast<float*>(rp.normals);
      n.outVerts    = const_cast<float4*>(rp.verts);
      n.vertexCount = uint32_t(nv);
      n.firstBlock  = uint32_t(normalBlockTask.size());
      normalBlockTask.insert(normalBlockTask.end(), nb, uint32_t(normalTasks.size()));
      normalTasks.push_back(n);
    }
  }
  uint32_t* rejectedDev = pt->vu.blockTask.ptr + 2 * pt->vu.blockCap;
  uint32_t  rejected    = 0;
  if(!tasks.empty())
  {
    if(stagingBytes)
      HIP_TRY(hipMemcpy(pt->vuStaging.ptr, staging.data(), stagingBytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pt->vu.tasks.ptr, tasks.data(), tasks.size() * sizeof(pt::VertexUpdateTask), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pt->vu.blockTask.ptr, blockTask.data(), blockTask.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(rejectedDev, 0, sizeof(uint32_t)));
    pt::launchVertexIngest(pt->vu.tasks.ptr, pt->vu.blockTask.ptr, uint32_t(blockTask.size()), rejectedDev, nullptr);
    HIP_TRY(hipGetLastError());
    if(!normalTasks.empty())  // (after the ingest, on the same stream: it reads resident positions, which are always finite)
    {
      HIP_TRY(hipMemcpy(pt->vu.normalTasks.ptr, normalTasks.data(), normalTasks.size() * sizeof(pt::NormalRebuildTask), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(pt->vu.blockTask.ptr + pt->vu.blockCap, normalBlockTask.data(), normalBlockTask.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      pt::launchNormalRebuild(pt->vu.normalTasks.ptr, pt->vu.blockTask.ptr + pt->vu.blockCap, uint32_t(normalBlockTask.size()), nullptr);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&rejected, rejectedDev, sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  printBuildTiming("vertex update", t0);
  ++pt->vuInfo.calls;
  pt->vuInfo.verticesWritten += vertices - rejected;
  pt->vuInfo.verticesRejected = rejected;
  if(tasks.empty())
    return MI_PT_OK;
  pt->vm.poseDirty = true;  // (vertex motion: the next rendered pose is followed by a snapshot of the positions)
  for(int k = 0; k < numUpdates; ++k)  // (what the next acceleration update refits; sized by a build that kept refit data)
    if(size_t(updates[k].renderPrimID) < pt->accel.primDirty.size())
      pt->accel.primDirty[size_t(updates[k].renderPrimID)] = pt->accel.primDeformed[size_t(updates[k].renderPrimID)] = 1;
  if(flags & MI_PT_DEFORM_DEFER_BUILD)
    return MI_PT_OK;
  return updateAcceleration(pt, true, std::vector<uint8_t>(pt->hostNodes.size(), 0));
}

int mi_pt_update_vertices(MiPt* pt, const MiPtVertexUpdate* updates, int numUpdates, int flags)
{
  FLUSH_PENDING(pt);
  return updateVertices(pt, updates, numUpdates, flags, false, "mi_pt_update_vertices");
}

int mi_pt_update_vertices_device(MiPt* pt, const MiPtVertexUpdate* updates, int numUpdates, int flags)
{
  FLUSH_PENDING(pt);
  return updateVertices(pt, updates, numUpdates, flags, true, "mi_pt_update_vertices_device");
}

int mi_pt_get_vertex_update_info(MiPt* pt, MiPtVertexUpdateInfo* out)
{
  if(!pt || !out)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_get_vertex_update_info: null argument");
  *out            = pt->vuInfo;
  out->tableBytes = pt->vu.table.bytes();
  return MI_PT_OK;
}

// Both forms of a texture update.  `device`: the level pointers are device memory, read by the kernels where they lie.
static int updateTextures(MiPt* pt, const MiPtTextureUpdate* updates, int numUpdates, bool device, const char* name)
{
  const std::string fn = name;
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, fn + ": null instance");
  if(numUpdates < 0 || (numUpdates > 0 && !updates))
    return fail(MI_PT_ERR_ARGUMENT, fn + ": negative count or null table");
  // ---- validation: nothing changes when any texture of the call is refused
  const int            numTextures = int(pt->hostTextures.size());
  std::vector<uint8_t> seen(size_t(numTextures), 0);
  size_t               stagingBytes = 0;
  for(int k = 0; k < numUpdates; ++k)
  {
    const MiPtTextureUpdate& u   = updates[k];
    const std::string        who = fn + ": update " + std::to_string(k) + ": ";
    if(u.texture < 0 || u.texture >= numTextures)
      return fail(MI_PT_ERR_ARGUMENT, who + "texture " + std::to_string(u.texture) + " out of range");
    if(seen[size_t(u.texture)]++)
      return fail(MI_PT_ERR_ARGUMENT, who + "texture " + std::to_string(u.texture) + " listed twice");
    const pt::DevTexture& d = pt->hostTextures[size_t(u.texture)];
    if(u.width != int(d.width) || u.height != int(d.height))
      return fail(MI_PT_ERR_ARGUMENT, who + "the size differs from the resident texture's (a new size is a re-create)");
    if((u.format != MI_PT_TEXELS_RGBA8 && u.format != MI_PT_TEXELS_RGBA32F) || (u.flags & ~uint32_t(MI_PT_TEXTURE_GENERATE_MIPS)))
      return fail(MI_PT_ERR_ARGUMENT, who + "unknown format or flag bits");
    const bool generate = (u.flags & MI_PT_TEXTURE_GENERATE_MIPS) != 0;
    if(u.format == MI_PT_TEXELS_RGBA32F && !generate)
      return fail(MI_PT_ERR_ARGUMENT, who + "RGBA32F only together with MI_PT_TEXTURE_GENERATE_MIPS");
    if(u.numLevels != (generate ? 1 : int(d.numLevels)))
      return fail(MI_PT_ERR_ARGUMENT, who + "numLevels must be 1 with MI_PT_TEXTURE_GENERATE_MIPS, the resident count without");
    if(u.reserved[0] || u.reserved[1])
      return fail(MI_PT_ERR_ARGUMENT, who + "reserved words must be 0");
    if(!u.levels)
      return fail(MI_PT_ERR_ARGUMENT, who + "no levels");
    const size_t texelBytes = u.format == MI_PT_TEXELS_RGBA32F ? 16 : 4;
    for(int l = 0; l < u.numLevels; ++l)
    {
      if(!u.levels[l])
        return fail(MI_PT_ERR_ARGUMENT, who + "level " + std::to_string(l) + " is NULL");
      if(device && (reinterpret_cast<uintptr_t>(u.levels[l]) & (texelBytes - 1)))
        return fail(MI_PT_ERR_ARGUMENT, who + "a device pointer that is not " + std::to_string(texelBytes) + "-byte aligned");
      if(!device)
        stagingBytes += align16(levelExtent(d, l).texels * texelBytes);
    }
  }
  // the OPAQUE class of the load-time alpha cut was found under the old texels: its triangles skip the alpha test for good
  {
    const int numMaterials = int(pt->hostMaterials.size()), numPrims = int(pt->hostPrims.size());
    for(size_t n = 0; n < pt->hostNodes.size() && numMaterials > 0; ++n)
    {
      const size_t   m    = size_t(std::max(0, std::min(pt->hostNodes[n].materialID, numMaterials - 1)));
      const int      prim = pt->hostNodes[n].renderPrimID;
      const AlphaKey key  = alphaKey(pt->hostMaterials[m], pt->hostTexInfos.data());
      if(key.alphaMode != MI_ALPHA_OPAQUE && key.slot > 0 && key.index >= 0 && key.index < numTextures && seen[size_t(key.index)] && prim >= 0 && prim < numPrims
         && pt->hostPrims[size_t(prim)].opaqueTriangles > 0)
        return fail(MI_PT_ERR_ARGUMENT, fn + ": texture " + std::to_string(key.index) + " is the alpha source of a material whose geometry was cut at load: re-cut and re-create (material "
                                            + std::to_string(m) + ", render node " + std::to_string(n) + ")");
    }
  }
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // frames in flight still sample the old texels; the caller's streams have produced the device images
  const auto t0 = BuildClock::now();
  if(numUpdates == 0)
  {
    ++pt->tuInfo.calls;
    pt->tuInfo.launches = 0;
    return MI_PT_OK;
  }
  if(!pt->tuTables.ptr)
  {
    std::vector<float> tables(size_t{pt::TU_TABLE_FLOATS});
    pt::tuBuildTables(tables.data(), pt::tuHostLinearToSrgb8);
    HIP_TRY(pt->tuTables.upload(tables.data(), tables.size()));
  }
  if(stagingBytes > pt->tuStaging.count)
    HIP_TRY(pt->tuStaging.alloc(stagingBytes));
  // ---- task tables.  Level 0 of every texture: one ingest launch.  A complete caller-supplied chain: its levels 1.. are ingest tasks of
  // the same launch.  Generated levels: the tasks of level index l of every texture lie together, one launch per l.
  std::vector<pt::TextureIngestTask> ingest;
  std::vector<uint32_t>              ingestBlocks;
  std::vector<pt::TextureMipTask>    mips[16];
  std::vector<uint32_t>              mipBlocks[16];
  size_t                             off = 0;
  uint64_t                           texels = 0, generated = 0;
  auto                               blocksOf = [](size_t n) { return (n + pt::TEXTURE_UPDATE_BLOCK - 1) / pt::TEXTURE_UPDATE_BLOCK; };
  for(int k = 0; k < numUpdates; ++k)
  {
    const MiPtTextureUpdate& u = updates[k];
    const pt::DevTexture&    d = pt->hostTextures[size_t(u.texture)];
    uint32_t* const          pool = reinterpret_cast<uint32_t*>(pt->texels.ptr);
    const bool               f32 = u.format == MI_PT_TEXELS_RGBA32F;
    for(int l = 0; l < u.numLevels; ++l)
    {
      const size_t          n = levelExtent(d, l).texels, bytes = n * (f32 ? 16 : 4);
      pt::TextureIngestTask t{};
      if(device)
        t.src = u.levels[l];
      else
      {
        t.src = pt->tuStaging.ptr + off;
        HIP_TRY(hipMemcpy(pt->tuStaging.ptr + off, u.levels[l], bytes, hipMemcpyHostToDevice));  // (straight from the caller's memory: no host copy)
        off += align16(bytes);
      }
      t.dst        = pool + d.levelOffset[l];
      t.texelCount = uint32_t(n);
      t.firstBlock = uint32_t(ingestBlocks.size());
      t.flags      = (d.srgb ? pt::TU_SRGB : 0u) | (f32 ? pt::TU_FLOAT : 0u);
      ingestBlocks.insert(ingestBlocks.end(), blocksOf(n), uint32_t(ingest.size()));
      ingest.push_back(t);
      texels += n;
    }
    if(u.flags & MI_PT_TEXTURE_GENERATE_MIPS)
      for(int l = 1; l < int(d.numLevels); ++l)
      {
        const LevelExtent  from = levelExtent(d, l - 1), to = levelExtent(d, l);
        pt::TextureMipTask t{};
        t.src        = pool + d.levelOffset[l - 1];
        t.dst        = pool + d.levelOffset[l];
        t.sw         = uint32_t(from.w);
        t.sh         = uint32_t(from.h);
        t.dw         = uint32_t(to.w);
        t.dh         = uint32_t(to.h);
        t.firstBlock = uint32_t(mipBlocks[l].size());
        t.flags      = d.srgb ? pt::TU_SRGB : 0u;
        mipBlocks[l].insert(mipBlocks[l].end(), blocksOf(to.texels), uint32_t(mips[l].size()));
        mips[l].push_back(t);
        texels += to.texels;
        ++generated;
      }
  }
  std::vector<pt::TextureMipTask> mipTasks;
  std::vector<uint32_t>           blockTask = ingestBlocks;
  size_t                          mipTaskAt[16] = {}, mipBlockAt[16] = {};
  for(int l = 1; l < 16; ++l)
  {
    mipTaskAt[l]  = mipTasks.size();
    mipBlockAt[l] = blockTask.size();
    mipTasks.insert(mipTasks.end(), mips[l].begin(), mips[l].end());
    blockTask.insert(blockTask.end(), mipBlocks[l].begin(), mipBlocks[l].end());
  }
  DevBuf<pt::TextureIngestTask> devIngest;
  DevBuf<pt::TextureMipTask>    devMips;
  DevBuf<uint32_t>              devBlockTask;
  HIP_TRY(devIngest.upload(ingest.data(), ingest.size()));
  HIP_TRY(devMips.upload(mipTasks.data(), mipTasks.size()));
  HIP_TRY(devBlockTask.upload(blockTask.data(), blockTask.size()));
  uint64_t launches = 0;
  pt::launchTextureIngest(devIngest.ptr, devBlockTask.ptr, uint32_t(ingestBlocks.size()), pt->tuTables.ptr, nullptr);
  launches += ingestBlocks.empty() ? 0 : 1;
  HIP_TRY(hipGetLastError());
  for(int l = 1; l < 16; ++l)  // (on the one stream: level l reads the quantised level l - 1)
    if(!mips[l].empty())
    {
      pt::launchTextureMips(devMips.ptr + mipTaskAt[l], devBlockTask.ptr + mipBlockAt[l], uint32_t(mipBlocks[l].size()), pt->tuTables.ptr, nullptr);
      ++launches;
    }
  HIP_TRY(hipGetLastError());
  // ---- the bilinear footprints of every level the call wrote, with the kernel of mi_pt_create
  if(pt->texQuads.ptr)
    for(int k = 0; k < numUpdates; ++k)
    {
      const pt::DevTexture& d = pt->hostTextures[size_t(updates[k].texture)];
      for(int l = 0; l < int(d.numLevels); ++l)
      {
        pt::launchTextureQuads(pt->texels.ptr, pt->texQuads.ptr, d.levelOffset[l], levelExtent(d, l).w, levelExtent(d, l).h, d.wrapS, d.wrapT, nullptr);
        ++launches;
      }
    }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());  // (the task tables are released on return)
  printBuildTiming("texture update", t0);
  ++pt->tuInfo.calls;
  pt->tuInfo.texelsWritten += texels;
  pt->tuInfo.levelsGenerated += generated;
  pt->tuInfo.launches = launches;
  return MI_PT_OK;
}

int mi_pt_update_textures(MiPt* pt, const MiPtTextureUpdate* updates, int numUpdates)
{
  FLUSH_PENDING(pt);
  return updateTextures(pt, updates, numUpdates, false, "mi_pt_update_textures");
}

int mi_pt_update_textures_device(MiPt* pt, const MiPtTextureUpdate* updates, int numUpdates)
{
  FLUSH_PENDING(pt);
  return updateTextures(pt, updates, numUpdates, true, "mi_pt_update_textures_device");
}

int mi_pt_read_texture(MiPt* pt, int texture, int level, uint8_t* hostRGBA8)
{
  FLUSH_PENDING(pt);
  if(!pt || !hostRGBA8 || texture < 0 || texture >= int(pt->hostTextures.size()) || level < 0 || level >= int(pt->hostTextures[size_t(texture)].numLevels))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_texture: no such texture or level, or a null destination");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  const pt::DevTexture& d = pt->hostTextures[size_t(texture)];
  HIP_TRY(hipMemcpy(hostRGBA8, pt->texels.ptr + d.levelOffset[level], levelExtent(d, level).texels * 4, hipMemcpyDeviceToHost));
  return MI_PT_OK;
}

int mi_pt_get_texture_update_info(MiPt* pt, MiPtTextureUpdateInfo* out)
{
  if(!pt || !out)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_get_texture_update_info: null argument");
  *out = pt->tuInfo;
  return MI_PT_OK;
}

// Both forms of an environment update.  `device`: u->pixels is device memory, read by the ingest kernel where it lies.
static int updateEnvironment(MiPt* pt, const MiPtEnvironmentUpdate* u, bool device, const char* name)
{
  const std::string fn = name;
  if(!pt || !u)
    return fail(MI_PT_ERR_ARGUMENT, fn + ": null instance or update");
  // ---- validation: nothing changes when the call is refused
  if(!u->pixels)
    return fail(MI_PT_ERR_ARGUMENT, fn + ": null pixels");
  if(u->width < 1 || u->height < 1 || uint64_t(u->width) * uint64_t(u->height) > uint64_t(pt::ENV_MAX_TEXELS))
    return fail(MI_PT_ERR_ARGUMENT, fn + ": need width, height >= 1 and width * height <= 2^26");
  if(u->channels != 3 && u->channels != 4)
    return fail(MI_PT_ERR_ARGUMENT, fn + ": channels must be 3 or 4");
  if(u->flags)
    return fail(MI_PT_ERR_ARGUMENT, fn + ": unknown flag bits");
  if(u->reserved[0] || u->reserved[1])
    return fail(MI_PT_ERR_ARGUMENT, fn + ": reserved words must be 0");
  const uint32_t n        = uint32_t(u->width) * uint32_t(u->height);
  const size_t   channels = size_t(u->channels);
  if(device && (reinterpret_cast<uintptr_t>(u->pixels) & (channels == 4 ? 15u : 3u)))
    return fail(MI_PT_ERR_ARGUMENT, fn + ": a device pointer that is not " + std::to_string(channels == 4 ? 16 : 4) + "-byte aligned");
  if(!device)
  {
    const float* px = static_cast<const float*>(u->pixels);
    for(size_t i = 0; i < n; ++i)
      for(size_t c = 0; c < 3; ++c)
      {
        const float v = px[i * channels + c];
        if(!(v >= 0.0f && v <= FLT_MAX))
          return fail(MI_PT_ERR_ARGUMENT, fn + ": texel " + std::to_string(i) + " has a component that is not finite or is negative");
      }
  }
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // frames in flight still read the old map; the caller's streams have produced the device image
  const auto t0 = BuildClock::now();
  // ---- memory: the scratch grows, the map and the table are replaced only when the texel count differs
  const pt::EnvScratchLayout L = pt::euScratchLayout(n, uint32_t(u->height));
  if(L.bytes > pt->euScratch.count)
    HIP_TRY(pt->euScratch.alloc(L.bytes));
  if(pt->envPixels.count != n || pt->envAccel.count != n)
  {
    DevBuf<float4>     pixels;
    DevBuf<MiEnvAccel> accel;
    HIP_TRY(pixels.alloc(n));
    HIP_TRY(accel.alloc(n));
    pt->envPixels = std::move(pixels);
    pt->envAccel  = std::move(accel);
  }
  publishEnvironment(pt, u->width, u->height);
  uint8_t* const  base = pt->euScratch.ptr;
  pt::EnvArgs     A{};
  A.n          = n;
  A.width      = uint32_t(u->width);
  A.channels   = uint32_t(channels);
  A.numTiles   = pt::euNumTiles(n);
  A.pixels     = pt->envPixels.ptr;
  A.accel      = pt->envAccel.ptr;
  A.rowArea    = reinterpret_cast<const double*>(base + L.rowArea);
  A.header     = reinterpret_cast<pt::EnvHeader*>(base + L.header);
  A.tileImp    = reinterpret_cast<double*>(base + L.tileImp);
  A.tiles      = reinterpret_cast<pt::EnvTriple*>(base + L.tiles);
  A.prefix     = reinterpret_cast<double*>(base + L.prefix);
  A.index      = reinterpret_cast<uint32_t*>(base + L.index);
  A.uniformPdf = pt::euUniformPdf();
  if(device)
    A.src = static_cast<const float*>(u->pixels);
  else
  {
    // RGBA32F goes straight into the resident map, which the ingest then rewrites texel by texel; RGB32F into the prefix and index arrays
    // (12 bytes per texel), which nothing writes before the ingest has read them
    void* const stage = channels == 4 ? static_cast<void*>(pt->envPixels.ptr) : static_cast<void*>(base + L.prefix);
    HIP_TRY(hipMemcpy(stage, u->pixels, size_t(n) * channels * sizeof(float), hipMemcpyHostToDevice));
    A.src = static_cast<const float*>(stage);
  }
  {
    std::vector<double> area(size_t(u->height));
    pt::euRowAreas(u->width, u->height, area.data());
    HIP_TRY(hipMemcpy(base + L.rowArea, area.data(), area.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemset(base + L.header, 0, sizeof(pt::EnvHeader)));
  struct Timing
  {
    BuildClock::time_point last;
    hipError_t             error = hipSuccess;
  } timing{BuildClock::now()};
  auto passDone = [](const char* pass, void* user) {
    Timing&          T = *static_cast<Timing*>(user);
    const hipError_t e = hipDeviceSynchronize();
    T.error            = T.error != hipSuccess ? T.error : e;
    printBuildTiming(pass, T.last, 3);
    T.last = BuildClock::now();
  };
  pt::launchEnvUpdate(A, nullptr, buildTiming() ? +passDone : nullptr, &timing);
  HIP_TRY(hipGetLastError());
  HIP_TRY(timing.error);
  pt::EnvHeader header{};
  HIP_TRY(hipMemcpy(&header, base + L.header, sizeof(header), hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceSynchronize());
  printBuildTiming("environment update", t0);
  const bool lit  = header.total > 0.0;
  pt->envIntegral = float(header.total);
  ++pt->euInfo.calls;
  pt->euInfo.texelsWritten += n;
  pt->euInfo.texelsSanitised = header.sanitised;
  pt->euInfo.launches  = uint64_t(pt::ENV_UPDATE_LAUNCHES);
  pt->euInfo.lightTexels     = lit ? header.numLight : 0u;
  pt->euInfo.heavyTexels     = lit ? n - header.numLight : 0u;
  pt->euInfo.integral  = pt->envIntegral;
  return MI_PT_OK;
}

int mi_pt_update_environment(MiPt* pt, const MiPtEnvironmentUpdate* update)
{
  FLUSH_PENDING(pt);
  return updateEnvironment(pt, update, false, "mi_pt_update_environment");
}

int mi_pt_update_environment_device(MiPt* pt, const MiPtEnvironmentUpdate* update)
{
  FLUSH_PENDING(pt);
  return updateEnvironment(pt, update, true, "mi_pt_update_environment_device");
}

int mi_pt_read_environment(MiPt* pt, float* hostRGBA, MiEnvAccel* hostAccel, int* width, int* height, float* integral)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_environment: null instance");
  if(!pt->envPixels.ptr || !pt->envAccel.ptr)
    return fail(MI_PT_ERR_STATE, "mi_pt_read_environment: no environment is resident");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t n = size_t(pt->scene.envWidth) * size_t(pt->scene.envHeight);
  if(hostRGBA)
    HIP_TRY(hipMemcpy(hostRGBA, pt->envPixels.ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
  if(hostAccel)
    HIP_TRY(hipMemcpy(hostAccel, pt->envAccel.ptr, n * sizeof(MiEnvAccel), hipMemcpyDeviceToHost));
  if(width)
    *width = pt->scene.envWidth;
  if(height)
    *height = pt->scene.envHeight;
  if(integral)
    *integral = pt->envIntegral;
  return MI_PT_OK;
}

int mi_pt_get_environment_update_info(MiPt* pt, MiPtEnvironmentUpdateInfo* out)
{
  if(!pt || !out)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_get_environment_update_info: null argument");
  *out              = pt->euInfo;
  out->scratchBytes = pt->euScratch.bytes();
  return MI_PT_OK;
}

int mi_pt_set_accel_update(MiPt* pt, int mode, float rebuildCostRatio)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_accel_update: null instance");
  if(mode != MI_PT_ACCEL_REBUILD && mode != MI_PT_ACCEL_REFIT && mode != MI_PT_ACCEL_AUTO)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_accel_update: unknown mode " + std::to_string(mode));
  if(!std::isfinite(rebuildCostRatio) || rebuildCostRatio < 1.0f)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_accel_update: the rebuild cost ratio must be finite and at least 1");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // frames in flight still walk the structure
  pt->accel.accelMode  = mode;
  pt->accel.accelRatio = rebuildCostRatio;
  if(mode == MI_PT_ACCEL_REBUILD)
  {
    pt->accel.refit = MiPt::Accel::RefitData{};
    return MI_PT_OK;
  }
  if(!pt->accel.refit.levels.empty() || !pt->accel.refitCapable)
    return MI_PT_OK;  // (refit data held already, or the structure can never keep any -- BVH2 walk, host collapse, empty or one-reference scene: no build)
  return buildForSwitch(pt);
}

int mi_pt_get_accel_info(MiPt* pt, MiPtAccelInfo* out)
{
  if(!pt || !out)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_get_accel_info: null argument");
  memset(out, 0, sizeof(*out));
  out->mode             = pt->accel.accelMode;
  out->lastUpdate       = pt->accel.lastUpdate;
  out->rebuildCostRatio = pt->accel.accelRatio;
  out->builds           = uint64_t(std::max(pt->accel.accelBuilds, 0));
  out->refits           = pt->accel.accelRefits;
  out->sahCostAtBuild   = pt->accel.refit.sahAtBuild;
  out->sahCost          = pt->accel.refit.sahNow;
  out->trianglesMoved   = pt->accel.trianglesMoved;
  out->refitBytes       = pt->accel.refit.bytes();
  return MI_PT_OK;
}

int mi_pt_set_accel_resident(MiPt* pt, int enable)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_accel_resident: null instance");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // frames in flight still walk the structure
  pt->accel.accelResident = enable != 0;
  // the tree the updates then refit: built once, here, when the request comes into force or leaves it (inert under REBUILD, the BVH2 walk
  // and the host collapse: their updates build anyway)
  if(residentWanted(pt) == pt->accel.residentTree || pt->accel.accelMode == MI_PT_ACCEL_REBUILD || pt->accel.keepsNoRefitData(pt->sw))
    return MI_PT_OK;
  return buildForSwitch(pt);
}

int mi_pt_get_accel_resident_info(MiPt* pt, MiPtAccelResidentInfo* out)
{
  if(!pt || !out)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_get_accel_resident_info: null argument");
  memset(out, 0, sizeof(*out));
  const bool inForce     = residentInForce(pt);
  out->enabled           = pt->accel.accelResident ? 1 : 0;
  out->inForce           = inForce ? 1 : 0;
  out->residentTriangles = inForce ? uint64_t(std::max(pt->scene.numTris, 0)) : 0;
  out->hiddenTriangles   = inForce ? pt->accel.hiddenTris : 0;
  out->visibilityRefits  = pt->accel.visibilityRefits;
  out->materialPatches   = pt->accel.materialPatches;
  return MI_PT_OK;
}

int mi_pt_read_vertices(MiPt* pt, int renderPrimID, float* positions, float* normals, float* tangents)
{
  FLUSH_PENDING(pt);
  if(!pt || renderPrimID < 0 || renderPrimID >= int(pt->hostPrims.size()))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_vertices: no such render primitive");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  const pt::DevPrim& p  = pt->hostPrims[size_t(renderPrimID)];
  const size_t       nv = pt->primVertices[size_t(renderPrimID)];
  if(positions && p.positions && nv)
    HIP_TRY(hipMemcpy(positions, p.positions, nv * 12, hipMemcpyDeviceToHost));
  if(normals && p.normals && nv)
    HIP_TRY(hipMemcpy(normals, p.normals, nv * 12, hipMemcpyDeviceToHost));
  if(tangents && p.tangents && nv)
    HIP_TRY(hipMemcpy(tangents, p.tangents, nv * 16, hipMemcpyDeviceToHost));
  return MI_PT_OK;
}

int mi_pt_destroy(MiPt* pt)
{
  if(!pt)
    return MI_PT_OK;
  pt->frameQueue.pendingFrames = 0;  // (frames still held back are dropped with the instance)
  (void)hipSetDevice(pt->device);
  (void)hipDeviceSynchronize();
  pt::dumpTraceProfile();
  delete pt;
  return MI_PT_OK;
}

int mi_pt_set_environment(MiPt* pt, const MiPtEnvironment* env)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_environment: null instance");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  if(!env || !env->rgba || !env->accel || env->width <= 0 || env->height <= 0)
  {
    pt->envPixels.release();
    pt->envAccel.release();
    publishEnvironment(pt, 0, 0);
    return MI_PT_OK;
  }
  const size_t n = size_t(env->width) * size_t(env->height);
  HIP_TRY(pt->envPixels.upload(reinterpret_cast<const float4*>(env->rgba), n));
  HIP_TRY(pt->envAccel.upload(env->accel, n));
  publishEnvironment(pt, env->width, env->height);
  pt->envIntegral = env->integral;
  return MI_PT_OK;
}

int mi_pt_resize(MiPt* pt, int width, int height)
{
  FLUSH_PENDING(pt);
  if(!pt || width <= 0 || height <= 0 || width > 32768 || height > 32768)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_resize: need 0 < width, height <= 32768");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  pt->width       = width;
  pt->height      = height;
  pt->denoised    = nullptr;
  pt->accumFrames = 0.0f;
  pt->momentFrames = 0.0f;
  return allocFrameResources(pt);
}

int mi_pt_set_frame_info(MiPt* pt, const MiSceneFrameInfo* info)
{
  if(!pt || !info)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_frame_info: null argument");
  // (the reference updates bFrameInfo / bSkyParams in EVERY onRender, changed or not -- src/renderer.cpp:675-708 -- and so does a drop-in caller: the same values again
  //  are no reason to issue the frames mi_pt_set_frame_queue is holding back)
  if(pt->haveFrameInfo && memcmp(&pt->frameInfo, info, sizeof(*info)) == 0)
    return MI_PT_OK;
  FLUSH_PENDING(pt);
  pt->frameInfo     = *info;
  pt->haveFrameInfo = true;
  return MI_PT_OK;
}
int mi_pt_set_sky(MiPt* pt, const MiSkyPhysicalParameters* sky)
{
  if(!pt || !sky)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_sky: null argument");
  if(memcmp(&pt->sky, sky, sizeof(*sky)) == 0)
    return MI_PT_OK;
  FLUSH_PENDING(pt);
  pt->sky = *sky;
  return MI_PT_OK;
}

int mi_pt_set_tile_partition(MiPt* pt, int rank, int world, int tileSize)
{
  FLUSH_PENDING(pt);
  if(!pt || world < 1 || rank < 0 || rank >= world || tileSize < 16 || tileSize > 4096 || (tileSize & (tileSize - 1)) != 0)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_tile_partition: need 0 <= rank < world and tileSize a power of two in [16, 4096]");
  pt->tileRank  = rank;
  pt->tileWorld = world;
  pt->tileSize  = tileSize;
  if(pt->width > 0)
  {
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(hipDeviceSynchronize());
    void* bound = (pt->accum != pt->accumOwn.ptr) ? pt->accum : nullptr;
    int   rc    = allocFrameResources(pt);
    if(rc == MI_PT_OK && bound)
      pt->accum = reinterpret_cast<float4*>(bound);
    return rc;
  }
  return MI_PT_OK;
}

int mi_pt_bind_accum(MiPt* pt, void* deviceRGBA32F)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_bind_accum: null instance");
  pt->accum = deviceRGBA32F ? reinterpret_cast<float4*>(deviceRGBA32F) : pt->accumOwn.ptr;
  return MI_PT_OK;
}

int mi_pt_bind_guides(MiPt* pt, void* albedoRGBA32F, void* normalRGBA32F, void* depthR32F)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_bind_guides: null instance");
  pt->albedoBound = reinterpret_cast<float4*>(albedoRGBA32F);
  pt->normalBound = reinterpret_cast<float4*>(normalRGBA32F);
  pt->depthBound  = reinterpret_cast<float*>(depthR32F);
  return MI_PT_OK;
}

int mi_pt_set_frame_queue(MiPt* pt, int depth)
{
  if(!pt || depth < 1 || depth > 1024)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_frame_queue: 1 <= depth <= 1024 required");
  FLUSH_PENDING(pt);
  pt->frameQueue.frameQueueDepth = depth;
  return MI_PT_OK;
}

// ---- the render calls.  Two refusals are shared by mi_pt_render_frame (a held-back frame is refused by the call that brings it, not by a
// later flush) and mi_pt_render_frames: each is written once and returns the code
static int refuseSamplesOrDepth(const MiPathtraceParams* params)
{
  // (maxDepth 0: the reference's loop `for(depth = 0; depth < maxDepth; ...)` never runs and the image is black; here no shade launch would run and
  //  the queued camera hits would keep the radiance and guide records of an earlier batch -- refused instead of special-cased)
  if(params->numSamples < 1 || params->maxDepth < 1 || params->maxDepth > 255)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_render_frame: numSamples >= 1 and 1 <= maxDepth <= 255 required");
  return MI_PT_OK;
}
static int refuseBeforeResize(const MiPt* pt)
{
  if(pt->width <= 0 || !pt->haveFrameInfo)
    return fail(MI_PT_ERR_STATE, "mi_pt_render_frame: call mi_pt_resize and mi_pt_set_frame_info first");
  return MI_PT_OK;
}

int mi_pt_render_frame(MiPt* pt, const MiPathtraceParams* params, void* hipStream)
{
  if(pt && params && pt->frameQueue.frameQueueDepth > 1)
  {
    MiPt::FrameQueue& q = pt->frameQueue;
    if(q.pendingFrames > 0)
    {
      if(q.joins(*params, hipStream))
      {
        if(++q.pendingFrames >= q.frameQueueDepth)
          return flushPending(pt);
        return MI_PT_OK;
      }
      FLUSH_PENDING(pt);
    }
    // argument errors are reported by THIS call, not by a later flush
    if(int rc = refuseSamplesOrDepth(params))
      return rc;
    if(int rc = refuseBeforeResize(pt))
      return rc;
    if(pt->cameraRaysStale())
      return fail(MI_PT_ERR_STATE, MiPt::CAMERA_RAYS_STALE);
    q.pendingFirst  = *params;
    q.pendingStream = hipStream;
    q.pendingFrames = 1;
    return MI_PT_OK;
  }

  return mi_pt_render_frames(pt, params, 1, hipStream);
}

// ---- mi_pt_render_frames in phases.  The entry point keeps every refusal and everything that allocates or synchronises; the phases launch.
// The path state lives by slot, not in the queue entry, on shadow-catcher frames (the plane's resolve pass may end a path) and under MI_PT_STATE_BY_SLOT
static bool catcherFrame(const MiPt* pt) { return (pt->frameInfo.flags & MI_SCENE_INFINITE_PLANE_SHADOW_CATCHER) != 0; }
static bool stateBySlot(const MiPt* pt) { return pt->sw.stateBySlot || catcherFrame(pt); }

// What every launch of the batch is given, but for the two device-resident descriptor copies (sceneDev, fcDev), which the entry point adds.
// Needs the sky constants up to date and the batch's optional path arrays allocated; moves accumFrames / momentFrames on by the batch.
static pt::LaunchCtx launchContextOf(MiPt* pt, const MiPathtraceParams* params, int numFrames, hipStream_t stream)
{
  pt::LaunchCtx c;
  c.scene = pt->scene;
  memset(&c.fc, 0, sizeof(c.fc));
  c.fc.frameInfo = pt->frameInfo;
  c.fc.sky       = pt->sky;
  c.fc.skyPre    = pt->skyConsts.skyPre.ptr;
  c.fc.pc        = *params;
  c.fc.width     = pt->width;
  c.fc.height    = pt->height;
  c.fc.tileSize  = pt->tileSize;
  c.fc.tileShift = tileShiftOf(pt);
  c.fc.numSlots  = pt->numSlots;
  c.fc.numFrames = numFrames;
  pt::divideMagic(uint32_t(std::max(numFrames, 2)), c.fc.framesMagic, c.fc.framesShift);
  c.fc.slotLayout   = numFrames % 64 == 0 ? 1 : 0;
  c.fc.stateInQueue = stateBySlot(pt) ? 0 : 1;
  c.sceneDev        = nullptr;
  c.fcDev           = nullptr;
  c.paths           = pt->paths;
  // optional records stay allocated (MiPt::opt*) once a batch needed them; THIS batch sees only the ones it needs itself -- a later
  // single-sample batch must not keep paying the by-slot writes of an earlier multi-sample or catcher batch
  const bool multiSample = params->numSamples > 1, guides = (params->flags & MI_PT_USE_OPTIX_DENOISER) != 0;
  if(!(stateBySlot(pt) || multiSample))
    c.paths.misc = nullptr;
  if(!stateBySlot(pt))
    c.paths.throughput = nullptr;
  if(!multiSample)
    c.paths.pixelSum = nullptr;
  pt->accumFrames = float(params->totalSamples) / float(params->numSamples) + float(numFrames);
  // the second moment covers the accumulation only if every batch since its start carried the guides
  if(guides && (params->totalSamples == 0 || pt->momentFrames == pt->accumFrames - float(numFrames)))
    pt->momentFrames = pt->accumFrames;
  else if(!guides || params->totalSamples == 0)
    pt->momentFrames = 0.0f;
  if(!guides)
  {
    c.paths.guideAlbedo = nullptr;
    c.paths.guideNormal = nullptr;
  }
  c.queues           = pt->queues;
  if(!catcherFrame(pt))
    c.queues.shadow.aux2 = nullptr;
  c.ownedTiles       = pt->ownedTiles.ptr;
  c.stats            = pt->stats.ptr;
  c.stream           = stream;
  c.persistentBlocks = unsigned(pt->numCUs) * 8u;
  c.hasAlpha         = pt->hasAlpha;
  // the closest-hit walks run their alpha machinery only where some alpha test has an open outcome: a scene whose non-opaque instances all have
  // alphaMode OPAQUE (transmissive glass) takes the plain kernels -- every candidate commits (INST_ALPHA_PASSES)
  c.hasAlphaClosest  = c.hasAlpha && pt->hasAlphaTest;
  // debug views (MiSceneFrameInfo::visualization, pt_visualize.h): their own shade kernel; a value the reference does not know renders the image
  c.visualization    = pt->frameInfo.visualization > MI_VIZ_RENDERED && pt->frameInfo.visualization < MI_VIZ_COUNT;
  // the opacity-micromap view colours the closest hit with alpha-tested geometry taken as opaque: the closest-hit walks run without their alpha rounds
  if(pt->frameInfo.visualization == MI_VIZ_OPACITY_MICROMAP)
    c.hasAlphaClosest = false;
  c.hasTransmissive  = pt->hasTransmissive;
  c.simpleMaterials  = pt->simpleMaterials;
  c.wide             = pt->accel.wide;
  c.collectCounters  = pt->collectCounters;
  c.shadowDeposit    = pt->sw.shadowDeposit;
  // Per-bounce sort of the shade kernel (k_shade): grouping the hits by material pays where the materials take different ways
  // through the BSDF (glass workload: generic shade kernel -11 %); where every material runs the same code (the SIMPLE
  // kernel, which therefore has no sort at all) it only cost (helmet +4 %, atrium +12 %, street +4 % of the shade kernel).
  // MI_PT_SORT = 0 | 1 | 2 is the A/B switch of the generic kernel.
  c.sortMode = pt->sw.sortMode;
  return c;
}

// Small batches: a bounce's shadow stage (any-hit walk + resolve) on a second stream, next to the NEXT bounce's closest-hit walk.  The two
// are independent -- the walk reads the continuation rays the shade launch wrote, the shadow stage adds into radiance records that only
// the next SHADE launch reads (which therefore waits for it) -- and with few frames in flight neither fills the 256 CUs: most
// workgroups of a persistent grid find no work and leave, so the other kernel's find room.  Needs the state in the queue entry (on
// catcher frames the resolve pass may end a path the walk is about to trace).
// ... and launches long enough to be worth two cross-stream hand-overs per bounce: measured (round 4, frames in flight 1 / 4 / 8 / 16 / 32 / 64 / 128)
// atrium-class (406 k triangles, depth 12) +15 / +8 / +6 / +3.5 / +1.7 / +1.0 / +0.3 %, street-class 4K +8 % at 1, +1.6 % at 8, +0.3 % from 32;
// helmet-class (74 k, 60 % of the camera paths leave at bounce 0) -6.5 / -0.4 / -0.8 / -0.6 %: scenes below 2e5 triangles keep one stream.
// Default up to 32 frames: the interactive range, where it pays; larger batches fill the device by themselves, and their per-launch times
// (bench.py's kernel table) stay those of kernels that have the device to themselves.
// Volume-scatter scenes run it at every batch size and triangle count: their random walks leave ~100 bounce iterations of a few thousand paths per
// batch, three dependent launches each, and taking the shadow stage off that chain measured +31 % for a single frame, +8.7 % at 32 and +2.2 % at 256
// frames in flight on the glass-class workload (the host's poll of the queue length every eighth iteration only waits for the main stream).
static bool wantsOverlap(const MiPt* pt, const pt::LaunchCtx& c)
{
  return pt->sw.overlapUpTo > 0 && ((c.fc.numFrames <= pt->sw.overlapUpTo && pt->scene.numTris >= pt->sw.overlapMinTris) || pt->hasVolumeScatter)
         && c.fc.stateInQueue != 0 && !pt->sw.traceSpans;
}

// The bound of a sample's bounce loop.  Every iteration either ends a path or consumes one unit of surfaceDepth, except volume scatter events
// (pathtrace_functions.h.slang:925-931), which are free for VOLUME_FREE_BUDGET bounces and then Russian-rouletted.
static int maxIterationsOf(const MiPt* pt, const MiPathtraceParams* params)
{
  int maxIters = params->maxDepth;
  // a shadow-catcher bounce does not consume surfaceDepth (eEarlyContinue) but is always followed by a miss or a surface hit
  if((pt->frameInfo.flags & MI_SCENE_USE_INFINITE_PLANE) && catcherFrame(pt))
    maxIters = 2 * params->maxDepth + 2;
  if(pt->hasVolumeScatter)
    maxIters = params->maxDepth * 66 + 512;
  if(pt->sw.maxItersDiag > 0)
    maxIters = std::min(maxIters, pt->sw.maxItersDiag);
  return maxIters;
}

// The poll of a volume-scatter scene's long loops: `drained` when the active queue `cur` is empty (synchronises the caller's stream)
static int queuesDrained(const pt::LaunchCtx& c, int cur, bool& drained)
{
  uint32_t counts[2 * pt::NSUB];
  HIP_TRY(hipMemcpyAsync(counts, &c.queues.counters[cur ? pt::QC_PAIR1 : pt::QC_PAIR0], sizeof(counts), hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  uint32_t remaining = 0;
  for(int q = 0; q < pt::NSUB; ++q)
    remaining += counts[2 * q];
  drained = remaining == 0;
  return MI_PT_OK;
}

// MI_PT_TRACE_SPANS=1: one bounce iteration with per-launch wall time and queue lengths on stderr (synchronising; diagnostics only)
static void traceSpansIteration(const MiPt* pt, const pt::LaunchCtx& c, const MiPathtraceParams* params, int it, int cur)
{
  const hipStream_t stream = c.stream;
  auto count = [&](int base) {  // base: first of 16 tails stored 2 words apart
    uint32_t v[2 * pt::NSUB];
    (void)hipMemcpy(v, &c.queues.counters[base], sizeof(uint32_t) * (2 * pt::NSUB - 1), hipMemcpyDeviceToHost);
    uint32_t t = 0;
    for(int q = 0; q < pt::NSUB; ++q) t += v[2 * q];
    return t;
  };
  auto span = [&](auto&& launch) {
    (void)hipStreamSynchronize(stream);
    auto t0 = std::chrono::steady_clock::now();
    launch();
    (void)hipStreamSynchronize(stream);
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  auto segs = [&]() {
    pt::StatCounters h{};
    (void)hipMemcpy(&h, pt->stats.ptr, sizeof(h), hipMemcpyDeviceToHost);
    return h;
  };
  uint32_t nIn = count(cur ? pt::QC_PAIR1 : pt::QC_PAIR0);
  const pt::StatCounters s0 = segs();
  double   tTrace = span([&] { pt::launchTraceClosest(c, cur); });
  const pt::StatCounters s1 = segs();
  double   tShade = span([&] { pt::launchShade(c, cur, it == 0); });
  uint32_t nSh    = count((cur ? pt::QC_PAIR0 : pt::QC_PAIR1) + 1);
  double   tShadow = span([&] { pt::launchTraceShadow(c, cur ^ 1); });
  const pt::StatCounters s2 = segs();
  fprintf(stderr, "[mi_pt span] frame %d it %2d rays %8u (traced %8llu, nodes %9llu tris %9llu) trace %8.3f ms shade %8.3f ms | shadow rays %8u (traced %8llu, nodes %9llu tris %9llu) %8.3f ms\n",
          params->frameCount, it, nIn, (unsigned long long)(s1.segments - s0.segments), (unsigned long long)(s1.nodesClosest - s0.nodesClosest),
          (unsigned long long)(s1.trisClosest - s0.trisClosest), tTrace, tShade, nSh, (unsigned long long)(s2.shadowRays - s1.shadowRays),
          (unsigned long long)(s2.nodesShadow - s1.nodesShadow), (unsigned long long)(s2.trisShadow - s1.trisShadow), tShadow);
}

// One sample of a batch: the primary stage, the bounce loop, the join of the side stream, the survivor flush and the fold into the accumulator.
// `iterations` counts the batch's bounce iterations: each is one closest-hit, one shade and one shadow launch
static int renderSample(MiPt* pt, const pt::LaunchCtx& c, const pt::LaunchCtx& cSide, const MiPathtraceParams* params, int s, bool overlap,
                        MiPt::ShadowOverlap::SideJoin& sideJoin, int& iterations)
{
  MiPt::LaunchTimer&         timer      = pt->timer;
  const MiPt::ShadowOverlap& side       = pt->shadowOverlap;
  const hipStream_t          stream     = c.stream;
  const bool                 debugSpans = pt->sw.traceSpans, guides = (params->flags & MI_PT_USE_OPTIX_DENOISER) != 0;
  pt::launchResetCounters(c.queues, stream);
  // 8-wide BVH: ONE kernel generates the camera rays, walks them as packets, finishes the paths that leave the scene and queues
  // the hits (k_trace_primary); BVH2 / MI_PT_NO_PACKET: k_generate writes the rays and the per-lane kernel walks them
  // bound camera rays: k_generate_rays takes the paths' rays from memory, then the per-lane walk, on both trees
  const bool boundRays    = pt->cameraRays != nullptr;
  const bool fusedPrimary = c.wide && !pt->sw.noPacket && !debugSpans && !boundRays;
  if(fusedPrimary)
  {
    timer.timed(stream, TK_PRIMARY, [&] { pt::launchTracePrimary(c, s); });
    if(timer.timingEnabled)
      ++timer.accTiming.tracePrimaryLaunches;
  }
  else if(boundRays)
    timer.timed(stream, TK_GENERATE, [&] { pt::launchGenerateRays(c, pt->cameraRays, uint32_t(pt->cameraRaySets), (pt->cameraRayFlags & MI_PT_CAMERA_RAYS_UNIT) != 0, s); });
  else
    timer.timed(stream, TK_GENERATE, [&] { pt::launchGenerate(c, s); });
  int       cur      = 0;
  const int maxIters = maxIterationsOf(pt, params);
  for(int it = 0; it < maxIters; ++it)
  {
    if(pt->hasVolumeScatter && it >= params->maxDepth && (it % 8) == 0)
    {
      bool drained = false;
      if(int rc = queuesDrained(c, cur, drained))
        return rc;
      if(drained)
        break;
    }
    if(debugSpans)
      traceSpansIteration(pt, c, params, it, cur);
    else
    {
      if(!(it == 0 && fusedPrimary))
        timer.timed(stream, TK_TRACE, [&] { pt::launchTraceClosest(c, cur); });
      if(overlap && it > 0)
        (void)hipStreamWaitEvent(stream, side.evShadowed, 0);  // the previous bounce's shadow terms are in before this shade launch reads them
      timer.timed(stream, it == 0 ? TK_SHADE_FIRST : TK_SHADE, [&] { pt::launchShade(c, cur, it == 0); });
      if(it == 0 && timer.timingEnabled)
        ++timer.accTiming.shadeFirstLaunches;
      if(overlap)
      {
        (void)hipEventRecord(side.evShaded, stream);
        (void)hipStreamWaitEvent(side.sideStream, side.evShaded, 0);
        timer.timed(side.sideStream, TK_SHADOW, [&] { pt::launchTraceShadow(cSide, cur ^ 1); });
        (void)hipEventRecord(side.evShadowed, side.sideStream);
        sideJoin.outstanding = true;
      }
      else
        timer.timed(stream, TK_SHADOW, [&] { pt::launchTraceShadow(c, cur ^ 1); });
    }
    ++iterations;
    cur ^= 1;
  }
  if(overlap && iterations > 0)
  {
    (void)hipStreamWaitEvent(stream, side.evShadowed, 0);  // the last bounce's shadow terms, before the sample is folded
    sideJoin.outstanding = false;                          // (joined: the caller's stream now orders everything after the side stream's work)
  }
  // paths the loop left alive (its iteration bound cut them: volume random walks) hand their radiance and seed over by slot
  if(c.fc.stateInQueue && (pt->hasVolumeScatter || pt->sw.maxItersDiag > 0))
    pt::launchFlushSurvivors(c, cur);
  timer.timed(stream, TK_ACCUM, [&] {
    pt::launchFinishSample(c, s, pt->accum, pt->depthImg(), guides ? pt->albedoImg() : nullptr, guides ? pt->normalImg() : nullptr);
  });
  return MI_PT_OK;
}

// What follows a first-frame batch: the selection image, and with motion vectors on the pose's motion image and the snapshot of its positions
static void afterFirstFrame(MiPt* pt, const pt::LaunchCtx& c, const MiPathtraceParams* params)
{
  const hipStream_t stream = c.stream;
  if(pt->cameraRays)  // (the set of the batch's first frame)
    pt::launchSelectionRays(c, pt->cameraRays, uint32_t(params->frameCount) % uint32_t(pt->cameraRaySets), pt->selection.ptr);
  else
    pt::launchSelection(c, pt->selection.ptr);
  pt->haveFirstHit = true;
  if(pt->temporal)  // the pose's motion image, then its matrices become the next pose's previous ones
  {
    pt::launchMotionVectors(pt->firstHit.ptr, pt->firstHitTri.ptr, pt->vm.prims.ptr, int(pt->vm.prims.count), pt->ownedTiles.ptr, uint32_t(pt->numSlots),
                            c.fc.tileShift, pt->width, pt->height, pt->nodes.ptr, pt->temporalData.prevObjectToWorld.ptr, int(pt->nodes.count),
                            pt->frameInfo.viewProjMatrix, pt->frameInfo.prevMVP, pt->temporalData.motion.ptr, stream);
    pt->temporalData.haveMotion = true;
    if(pt->firstHitTri.ptr)  // vertex motion: the rendered pose's positions become the next pose's previous ones, when an update changed them
    {
      pt->haveFirstHitTri = true;
      if(pt->vm.poseDirty)
        pt::launchSnapshotPositions(pt->vm.prims.ptr, pt->vm.deformIDs.ptr, uint32_t(pt->vm.deformIDs.count), pt->vm.maxVertices, stream);
      pt->vm.poseDirty = false;
    }
  }
}

int mi_pt_render_frames(MiPt* pt, const MiPathtraceParams* params, int numFrames, void* hipStream)
{
  FLUSH_PENDING(pt);
  if(!pt || !params)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_render_frame: null argument");
  if(numFrames < 1 || numFrames > 1024)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_render_frames: 1 <= numFrames <= 1024 required");
  if(int rc = refuseBeforeResize(pt))
    return rc;
  if(int rc = refuseSamplesOrDepth(params))
    return rc;
  if((pt->frameInfo.flags & MI_SCENE_USE_HDR_ENVIRONMENT) && !pt->scene.envPixels)
    return fail(MI_PT_ERR_STATE, "mi_pt_render_frame: HDR environment requested but none was set");
  if(pt->cameraRaysStale())
    return fail(MI_PT_ERR_STATE, MiPt::CAMERA_RAYS_STALE);
  HIP_TRY(hipSetDevice(pt->device));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hipStream);
  pt->lastStream     = stream;
  if(pt->numSlots == 0)
    return MI_PT_OK;
  if(numFrames > pt->framesCap)  // grow the path/queue arrays once; later batches of this size reuse them
  {
    HIP_TRY(hipDeviceSynchronize());
    if(int rc = allocPathResources(pt, numFrames))
      return rc;
  }

  if(int rc = pt->skyConsts.upToDate(pt->sky, stream))
    return rc;
  if(int rc = ensureOptionalPathArrays(pt, stateBySlot(pt), params->numSamples > 1, (params->flags & MI_PT_USE_OPTIX_DENOISER) != 0, catcherFrame(pt)))
    return rc;
  pt::LaunchCtx c = launchContextOf(pt, params, numFrames, stream);
  // descriptor copies for the kernels that read them through a pointer
  if(pt->sceneDevDirty)
  {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(pt->sceneDev.upload(&pt->scene, 1));
    pt->sceneDevDirty = false;
  }
  c.sceneDev      = pt->sceneDev.ptr;
  unsigned fcSlot = 0;
  if(int rc = pt->fcConsts.claim(c.fc, stream, &c.fcDev, &fcSlot))
    return rc;

  MiPt::LaunchTimer& timer  = pt->timer;
  hipEvent_t         frameA = nullptr, frameB = nullptr;
  if(timer.timingEnabled)
  {
    frameA = timer.getEvent();
    frameB = timer.getEvent();
    (void)hipEventRecord(frameA, stream);
  }
  const bool    overlap = wantsOverlap(pt, c) && pt->shadowOverlap.ready();
  pt::LaunchCtx cSide   = c;
  cSide.stream          = pt->shadowOverlap.sideStream;
  MiPt::ShadowOverlap::SideJoin sideJoin;
  sideJoin.side  = overlap ? pt->shadowOverlap.sideStream : nullptr;
  int iterations = 0;
  for(int s = 0; s < params->numSamples; ++s)
    if(int rc = renderSample(pt, c, cSide, params, s, overlap, sideJoin, iterations))
      return rc;
  if(params->flags & MI_PT_FIRST_FRAME)
    afterFirstFrame(pt, c, params);
  HIP_TRY(hipGetLastError());
  if(int rc = pt->fcConsts.recordDone(fcSlot, stream))
    return rc;
  if(timer.timingEnabled)
  {
    (void)hipEventRecord(frameB, stream);
    timer.pendingSpans.push_back({TK_COUNT, frameA, frameB});
    timer.accTiming.traceClosestLaunches += iterations;
    timer.accTiming.shadeLaunches += iterations;
    timer.accTiming.traceShadowLaunches += iterations;
    timer.accTiming.bounceIterations += iterations;
  }
  return MI_PT_OK;
}

int mi_pt_synchronize(MiPt* pt)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_synchronize: null instance");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  return MI_PT_OK;
}

int mi_pt_read_accum(MiPt* pt, float* host)
{
  FLUSH_PENDING(pt);
  if(!pt || !host || pt->width <= 0)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_accum: bad arguments");
  return readImage(pt, pt->accum, sizeof(float4), host);
}
int mi_pt_write_accum(MiPt* pt, const float* host)
{
  FLUSH_PENDING(pt);
  if(!pt || !host || pt->width <= 0)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_write_accum: bad arguments");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(pt->accum, host, size_t(pt->width) * size_t(pt->height) * sizeof(float4), hipMemcpyHostToDevice));
  pt->accumFrames  = 1.0f;  // a frame from elsewhere: denoisable, with no temporal moment behind it
  pt->momentFrames = 0.0f;
  return MI_PT_OK;
}
int mi_pt_read_guides(MiPt* pt, float* albedo, float* normal)
{
  FLUSH_PENDING(pt);
  if(!pt || pt->width <= 0)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_guides: bad arguments");
  if(int rc = readImage(pt, pt->albedoImg(), sizeof(float4), albedo))
    return rc;
  return readImage(pt, pt->normalImg(), sizeof(float4), normal, false);
}
int mi_pt_read_selection(MiPt* pt, uint32_t* host)
{
  FLUSH_PENDING(pt);
  if(!pt || !host || pt->width <= 0)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_selection: bad arguments");
  return readImage(pt, pt->selection.ptr, sizeof(uint32_t), host);
}
// ---- ray queries and picking (query.hip) --------------------------------------------------------------------------------------------------------
// Six entry points over three internal functions -- rays in host memory, rays in device memory, pixel positions.  A plain entry point is its _ex
// form under default options: it names itself in the messages, and differs in nothing else.
namespace {
// What an entry point asks for: its name (the prefix of its messages), whether its mode / options are ones the header accepts, and then their rules.
struct QueryCall
{
  const char*    who;
  bool           valid;
  pt::QueryRules rules;  // (rules.maxHits: the records per ray)
  bool           any;    // MI_PT_QUERY_ANY
};
QueryCall queryCallOfMode(const char* who, int mode)
{
  QueryCall c{};
  c.who                  = who;
  c.valid                = mode == MI_PT_QUERY_CLOSEST || mode == MI_PT_QUERY_ANY;
  c.rules.alpha          = MI_PT_QUERY_ALPHA_OPAQUE;
  c.rules.cull           = MI_PT_QUERY_CULL_NONE;
  c.rules.maxHits        = 1;
  c.rules.blendThreshold = 0.5f;
  c.any                  = mode == MI_PT_QUERY_ANY;
  return c;
}
QueryCall queryCallOf(const char* who, const MiPtQueryOptions* o)
{
  QueryCall c{};
  c.who = who;
  if(!o || o->reserved[0] != 0 || o->reserved[1] != 0)
    return c;
  if(o->mode != MI_PT_QUERY_CLOSEST && o->mode != MI_PT_QUERY_ANY && o->mode != MI_PT_QUERY_NEAREST_K)
    return c;
  if(o->alpha != MI_PT_QUERY_ALPHA_OPAQUE && o->alpha != MI_PT_QUERY_ALPHA_CUTOFF && o->alpha != MI_PT_QUERY_ALPHA_STOCHASTIC)
    return c;
  if(o->cull != MI_PT_QUERY_CULL_NONE && o->cull != MI_PT_QUERY_CULL_MATERIAL)
    return c;
  if(o->mode == MI_PT_QUERY_NEAREST_K ? (o->maxHits < 1 || o->maxHits > MI_PT_QUERY_MAX_HITS) : (o->maxHits != 0 && o->maxHits != 1))
    return c;
  if(o->alpha == MI_PT_QUERY_ALPHA_CUTOFF && !(o->blendThreshold > 0.0f && o->blendThreshold <= 1.0f))  // (NaN fails too)
    return c;
  c.valid                = true;
  c.rules.alpha          = o->alpha;
  c.rules.cull           = o->cull;
  c.rules.maxHits        = o->mode == MI_PT_QUERY_NEAREST_K ? o->maxHits : 1;
  c.rules.blendThreshold = o->blendThreshold;
  c.rules.seed           = o->seed;
  c.any                  = o->mode == MI_PT_QUERY_ANY;
  return c;
}
int failQuery(const QueryCall& c, int code, const std::string& what) { return fail(code, std::string(c.who) + ": " + what); }
// An alpha-aware walk reads the alpha record of every triangle without INST_FORCE_OPAQUE / INST_ALPHA_PASSES.  Such a triangle sets hasAlphaTest,
// hence hasAlpha, under which the build and the material patch keep the records (makeTriangleRecords, patchTriangleData): checked, not assumed.
bool queryAlphaRecordsMissing(const MiPt* pt, const pt::QueryRules& rules)
{
  return rules.alpha != MI_PT_QUERY_ALPHA_OPAQUE && pt->hasAlphaTest && pt->scene.numTris > 0 && !pt->scene.alphaTris;
}
const char* const QUERY_NO_ALPHA_RECORDS = "the scene has alpha-tested triangles but no alpha records";
int queryStaging(MiPt* pt, size_t numRays, size_t numHits)
{
  if(numRays > pt->queryRays.count)
    HIP_TRY(pt->queryRays.alloc(numRays));
  if(numHits > pt->queryHits.count)
    HIP_TRY(pt->queryHits.alloc(numHits));
  return MI_PT_OK;
}

int queryHostRays(MiPt* pt, const QueryCall& c, const MiPtRay* hostRays, int numRays, MiPtRayHit* hostHits)
{
  FLUSH_PENDING(pt);
  if(!pt || numRays < 0 || !c.valid || (numRays > 0 && (!hostRays || !hostHits)))
    return failQuery(c, MI_PT_ERR_ARGUMENT, "bad arguments");
  if(queryAlphaRecordsMissing(pt, c.rules))
    return failQuery(c, MI_PT_ERR_STATE, QUERY_NO_ALPHA_RECORDS);
  if(numRays == 0)
    return MI_PT_OK;
  const size_t numHits = size_t(numRays) * size_t(c.rules.maxHits);
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  if(int rc = queryStaging(pt, size_t(numRays), numHits))
    return rc;
  HIP_TRY(hipMemcpy(pt->queryRays.ptr, hostRays, size_t(numRays) * sizeof(MiPtRay), hipMemcpyHostToDevice));
  pt::launchQueryRaysEx(pt->scene, pt->accel.wide, c.any, c.rules, pt->queryRays.ptr, uint32_t(numRays), pt->queryHits.ptr, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(hostHits, pt->queryHits.ptr, numHits * sizeof(MiPtRayHit), hipMemcpyDeviceToHost));
  return MI_PT_OK;
}
int queryDeviceRays(MiPt* pt, const QueryCall& c, const void* deviceRays, int numRays, void* deviceHits, void* hipStream)
{
  FLUSH_PENDING(pt);
  if(!pt || numRays < 0 || !c.valid || (numRays > 0 && (!deviceRays || !deviceHits)))
    return failQuery(c, MI_PT_ERR_ARGUMENT, "bad arguments");
  if(numRays > 0 && ((reinterpret_cast<uintptr_t>(deviceRays) | reinterpret_cast<uintptr_t>(deviceHits)) & 15u))
    return failQuery(c, MI_PT_ERR_ARGUMENT, "rays and hits must be 16-byte aligned");
  if(queryAlphaRecordsMissing(pt, c.rules))
    return failQuery(c, MI_PT_ERR_STATE, QUERY_NO_ALPHA_RECORDS);
  if(numRays == 0)
    return MI_PT_OK;
  HIP_TRY(hipSetDevice(pt->device));
  pt::launchQueryRaysEx(pt->scene, pt->accel.wide, c.any, c.rules, static_cast<const MiPtRay*>(deviceRays), uint32_t(numRays), static_cast<MiPtRayHit*>(deviceHits),
                        reinterpret_cast<hipStream_t>(hipStream));
  HIP_TRY(hipGetLastError());
  return MI_PT_OK;
}
int queryPixels(MiPt* pt, const QueryCall& c, const float* pixelXY, int numPixels, MiPtRayHit* hostHits)
{
  FLUSH_PENDING(pt);
  if(!pt || numPixels < 0 || !c.valid || (numPixels > 0 && (!pixelXY || !hostHits)))
    return failQuery(c, MI_PT_ERR_ARGUMENT, "bad arguments");
  if(pt->width <= 0 || !pt->haveFrameInfo)
    return failQuery(c, MI_PT_ERR_STATE, "call mi_pt_resize and mi_pt_set_frame_info first");
  for(int i = 0; i < numPixels; ++i)
  {
    const float x = pixelXY[2 * i], y = pixelXY[2 * i + 1];
    if(!(x >= 0.0f && x < float(pt->width) && y >= 0.0f && y < float(pt->height)))  // (NaN fails too)
      return failQuery(c, MI_PT_ERR_ARGUMENT, "pixel " + std::to_string(i) + " lies outside the image");
  }
  if(queryAlphaRecordsMissing(pt, c.rules))
    return failQuery(c, MI_PT_ERR_STATE, QUERY_NO_ALPHA_RECORDS);
  if(numPixels == 0)
    return MI_PT_OK;
  // The pixel positions are staged in queryRays (8 bytes each: a quarter of a ray record): at its front under plain rules, which walk the camera
  // rays where they are formed; behind the numPixels ray records the camera rays are written to otherwise.
  const size_t n = size_t(numPixels), numHits = n * size_t(c.rules.maxHits);
  const bool   scratch = !pt::queryRulesPlain(c.rules);
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  if(int rc = queryStaging(pt, scratch ? n + (n + 3) / 4 : n, numHits))
    return rc;
  float2* xy = reinterpret_cast<float2*>(pt->queryRays.ptr + (scratch ? n : 0));
  HIP_TRY(hipMemcpy(xy, pixelXY, n * sizeof(float2), hipMemcpyHostToDevice));
  pt::FrameConsts fc;
  memset(&fc, 0, sizeof(fc));
  fc.frameInfo = pt->frameInfo;
  fc.width     = pt->width;
  fc.height    = pt->height;
  pt::launchPickRaysEx(pt->scene, fc, pt->accel.wide, c.rules, xy, scratch ? pt->queryRays.ptr : nullptr, uint32_t(numPixels), pt->queryHits.ptr, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(hostHits, pt->queryHits.ptr, numHits * sizeof(MiPtRayHit), hipMemcpyDeviceToHost));
  return MI_PT_OK;
}
}  // namespace

int mi_pt_query_rays(MiPt* pt, const MiPtRay* hostRays, int numRays, int mode, MiPtRayHit* hostHits)
{
  return queryHostRays(pt, queryCallOfMode("mi_pt_query_rays", mode), hostRays, numRays, hostHits);
}
int mi_pt_query_rays_device(MiPt* pt, const void* deviceRays, int numRays, int mode, void* deviceHits, void* hipStream)
{
  return queryDeviceRays(pt, queryCallOfMode("mi_pt_query_rays_device", mode), deviceRays, numRays, deviceHits, hipStream);
}
int mi_pt_pick(MiPt* pt, const float* pixelXY, int numPixels, MiPtRayHit* hostHits)
{
  return queryPixels(pt, queryCallOfMode("mi_pt_pick", MI_PT_QUERY_CLOSEST), pixelXY, numPixels, hostHits);
}
void mi_pt_default_query_options(MiPtQueryOptions* options)
{
  if(!options)
    return;
  memset(options, 0, sizeof(*options));
  options->mode           = MI_PT_QUERY_CLOSEST;
  options->alpha          = MI_PT_QUERY_ALPHA_OPAQUE;
  options->cull           = MI_PT_QUERY_CULL_NONE;
  options->maxHits        = 1;
  options->blendThreshold = 0.5f;
}
int mi_pt_query_rays_ex(MiPt* pt, const MiPtRay* hostRays, int numRays, const MiPtQueryOptions* options, MiPtRayHit* hostHits)
{
  return queryHostRays(pt, queryCallOf("mi_pt_query_rays_ex", options), hostRays, numRays, hostHits);
}
int mi_pt_query_rays_device_ex(MiPt* pt, const void* deviceRays, int numRays, const MiPtQueryOptions* options, void* deviceHits, void* hipStream)
{
  return queryDeviceRays(pt, queryCallOf("mi_pt_query_rays_device_ex", options), deviceRays, numRays, deviceHits, hipStream);
}
int mi_pt_pick_ex(MiPt* pt, const float* pixelXY, int numPixels, const MiPtQueryOptions* options, MiPtRayHit* hostHits)
{
  return queryPixels(pt, queryCallOf("mi_pt_pick_ex", options), pixelXY, numPixels, hostHits);
}
// ---- caller-supplied camera rays (camera_rays.hip) -----------------------------------------------------------------------------------------------
namespace {
int bindCameraRays(MiPt* pt, const char* who, const void* rays, int numSets, uint32_t flags, bool device)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, std::string(who) + ": null instance");
  if((rays && numSets < 1) || (!rays && numSets != 0) || (flags & ~uint32_t(MI_PT_CAMERA_RAYS_UNIT)) != 0u)
    return fail(MI_PT_ERR_ARGUMENT, std::string(who) + ": need numSets >= 1 with rays (NULL and 0 to unbind) and no unknown flag bits");
  if(rays && device && (reinterpret_cast<uintptr_t>(rays) & 15u))
    return fail(MI_PT_ERR_ARGUMENT, std::string(who) + ": rays must be 16-byte aligned");
  if(pt->width <= 0)
    return fail(MI_PT_ERR_STATE, std::string(who) + ": call mi_pt_resize first");
  if(rays && pt->temporal)
    return fail(MI_PT_ERR_STATE, std::string(who) + ": mi_pt_set_temporal is on -- the motion image assumes the projective camera");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());  // frames in flight may still read the rays bound before
  if(rays && !device)
  {
    const size_t    n = size_t(numSets) * size_t(pt->width) * size_t(pt->height);
    DevBuf<MiPtRay> copy;  // (taken over only once it holds the rays: a failed allocation leaves the binding unchanged)
    HIP_TRY(copy.upload(static_cast<const MiPtRay*>(rays), n));
    pt->cameraRaysOwn = std::move(copy);
    pt->cameraRays    = pt->cameraRaysOwn.ptr;
  }
  else
  {
    pt->cameraRaysOwn.release();
    pt->cameraRays = static_cast<const MiPtRay*>(rays);
  }
  pt->cameraRaySets    = rays ? numSets : 0;
  pt->cameraRayFlags   = rays ? flags : 0u;
  pt->cameraRaysWidth  = rays ? pt->width : 0;
  pt->cameraRaysHeight = rays ? pt->height : 0;
  return MI_PT_OK;
}
// sets [0, numSets) of `out` (device memory) on `stream`.  The rays are the ones k_generate writes (launchExportCameraRays), so the export goes
// through the instance's own queue 0 in pieces that fit it: some tiles of the image x at most 64 frames per piece.
int exportCameraRays(MiPt* pt, const char* who, const MiPathtraceParams* params, int numSets, MiPtRay* out, hipStream_t stream)
{
  const uint32_t* tiles     = pt->tileWorld > 1 ? pt->allTiles.ptr : pt->ownedTiles.ptr;
  const size_t    numTiles  = size_t(pt->tilesX) * size_t(pt->tilesY), tileSlots = size_t(pt->tileSize) * size_t(pt->tileSize);
  if(tileSlots > pt->queueCap)  // (only an instance whose rank owns no tile at all)
    return fail(MI_PT_ERR_STATE, std::string(who) + ": this rank of the tile partition owns no pixels -- its path queues hold no tile");
  pt::LaunchCtx c{};
  c.scene = pt->scene;
  memset(&c.fc, 0, sizeof(c.fc));
  c.fc.frameInfo = pt->frameInfo;
  c.fc.pc        = *params;
  c.fc.width     = pt->width;
  c.fc.height    = pt->height;
  c.fc.tileSize  = pt->tileSize;
  c.fc.tileShift = tileShiftOf(pt);
  c.queues = pt->queues;
  c.stream = stream;
  for(int done = 0; done < numSets;)
  {
    const int frames = int(std::min<size_t>(std::min<size_t>(size_t(numSets - done), 64), pt->queueCap / tileSlots));
    c.fc.numFrames   = frames;
    pt::divideMagic(uint32_t(std::max(frames, 2)), c.fc.framesMagic, c.fc.framesShift);
    c.fc.slotLayout    = frames % 64 == 0 ? 1 : 0;
    c.fc.pc.frameCount = params->frameCount + done;
    const size_t perPiece = pt->queueCap / (tileSlots * size_t(frames));
    for(size_t t = 0; t < numTiles; t += perPiece)
    {
      c.ownedTiles  = tiles + t;
      c.fc.numSlots = int(std::min(perPiece, numTiles - t) * tileSlots);
      pt::launchExportCameraRays(c, out, uint32_t(done));
    }
    done += frames;
  }
  HIP_TRY(hipGetLastError());
  return MI_PT_OK;
}
int makeCameraRays(MiPt* pt, const char* who, const MiPathtraceParams* params, int numSets, void* out, bool device, void* hipStream)
{
  FLUSH_PENDING(pt);
  if(!pt || !params || !out || numSets < 1)
    return fail(MI_PT_ERR_ARGUMENT, std::string(who) + ": need params, an output and numSets >= 1");
  if(device && (reinterpret_cast<uintptr_t>(out) & 15u))
    return fail(MI_PT_ERR_ARGUMENT, std::string(who) + ": rays must be 16-byte aligned");
  if(pt->width <= 0 || !pt->haveFrameInfo)
    return fail(MI_PT_ERR_STATE, std::string(who) + ": call mi_pt_resize and mi_pt_set_frame_info first");
  HIP_TRY(hipSetDevice(pt->device));
  if(device)
    return exportCameraRays(pt, who, params, numSets, static_cast<MiPtRay*>(out), reinterpret_cast<hipStream_t>(hipStream));
  HIP_TRY(hipDeviceSynchronize());  // (the export goes through the path queues: frames in flight on other streams first)
  const size_t    n = size_t(numSets) * size_t(pt->width) * size_t(pt->height);
  DevBuf<MiPtRay> tmp;
  HIP_TRY(tmp.alloc(n));
  if(int rc = exportCameraRays(pt, who, params, numSets, tmp.ptr, nullptr))
    return rc;
  HIP_TRY(hipMemcpy(out, tmp.ptr, n * sizeof(MiPtRay), hipMemcpyDeviceToHost));
  return MI_PT_OK;
}
}  // namespace

int mi_pt_set_camera_rays(MiPt* pt, const MiPtRay* hostRays, int numSets, uint32_t flags)
{
  return bindCameraRays(pt, "mi_pt_set_camera_rays", hostRays, numSets, flags, false);
}
int mi_pt_set_camera_rays_device(MiPt* pt, const void* deviceRays, int numSets, uint32_t flags)
{
  return bindCameraRays(pt, "mi_pt_set_camera_rays_device", deviceRays, numSets, flags, true);
}
int mi_pt_make_camera_rays(MiPt* pt, const MiPathtraceParams* params, int numSets, MiPtRay* hostRays)
{
  return makeCameraRays(pt, "mi_pt_make_camera_rays", params, numSets, hostRays, false, nullptr);
}
int mi_pt_make_camera_rays_device(MiPt* pt, const MiPathtraceParams* params, int numSets, void* deviceRays, void* hipStream)
{
  return makeCameraRays(pt, "mi_pt_make_camera_rays_device", params, numSets, deviceRays, true, hipStream);
}

int mi_pt_read_depth(MiPt* pt, float* host)
{
  FLUSH_PENDING(pt);
  if(!pt || !host || pt->width <= 0)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_depth: bad arguments");
  return readImage(pt, pt->depthImg(), sizeof(float), host);
}
void* mi_pt_accum_device_ptr(MiPt* pt)
{
  (void)flushPending(pt);
  return pt ? pt->accum : nullptr;
}

// The two ping-pong images of the denoise calls, at the current size (dropped by a resize: allocFrameResources)
static int denoiseScratch(MiPt* pt)
{
  const size_t px = size_t(pt->width) * size_t(pt->height);
  if(pt->denoiseA.count != px)
  {
    HIP_TRY(pt->denoiseA.alloc(px));
    HIP_TRY(pt->denoiseB.alloc(px));
  }
  return MI_PT_OK;
}
// The "result to host" step of the denoise calls: pt->denoised into `host` when one is given, behind `stream` unless the caller has
// synchronised it already.  Without a host destination the result stays on the device, in stream order.
static int denoisedToHost(MiPt* pt, float* host, hipStream_t stream, bool synchronised = false)
{
  if(!host)
    return MI_PT_OK;
  if(!synchronised)
    HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipMemcpy(host, pt->denoised, size_t(pt->width) * size_t(pt->height) * sizeof(float4), hipMemcpyDeviceToHost));
  return MI_PT_OK;
}

int mi_pt_denoise(MiPt* pt, int iterations, float sigmaColor, float sigmaNormal, float sigmaAlbedo, float* host, void* hipStream)
{
  FLUSH_PENDING(pt);
  if(!pt || pt->width <= 0 || iterations < 1 || iterations > 8)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_denoise: bad arguments");
  HIP_TRY(hipSetDevice(pt->device));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hipStream);
  if(int rc = denoiseScratch(pt))
    return rc;
  const float4* in  = pt->accum;
  float4*       out = pt->denoiseA.ptr;
  for(int i = 0; i < iterations; ++i)
  {
    pt::launchAtrous(in, out, pt->albedoImg(), pt->normalImg(), pt->width, pt->height, 1 << i, sigmaColor, sigmaNormal, sigmaAlbedo, stream);
    in  = out;
    out = (out == pt->denoiseA.ptr) ? pt->denoiseB.ptr : pt->denoiseA.ptr;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream));  // (this call always, the other two only for a host destination)
  pt->denoised = in;
  return denoisedToHost(pt, host, stream, true);
}

int mi_pt_denoise_svgf(MiPt* pt, int iterations, float sigmaLuminance, float sigmaNormal, float sigmaDepth, float* host, void* hipStream)
{
  FLUSH_PENDING(pt);
  if(!pt || pt->width <= 0 || iterations < 1 || iterations > 8 || !(sigmaLuminance > 0.0f) || !(sigmaDepth > 0.0f) || !(sigmaNormal >= 0.0f))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_denoise_svgf: bad arguments");
  if(!(pt->accumFrames >= 1.0f))
    return fail(MI_PT_ERR_STATE, "mi_pt_denoise_svgf: nothing rendered yet");
  HIP_TRY(hipSetDevice(pt->device));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hipStream);
  if(int rc = denoiseScratch(pt))
    return rc;
  // (mean and second moment must cover the same frames for E[l^2] - E[l]^2 to mean anything: otherwise -- guides switched on
  //  mid-accumulation, or an accumulator written by mi_pt_write_accum -- the pass estimates the variance spatially, as it does below 4 frames)
  const float varianceFrames = pt->momentFrames == pt->accumFrames ? pt->accumFrames : 1.0f;
  pt->denoised = pt::launchSvgf(pt->accum, pt->albedoImg(), pt->normalImg(), pt->depthImg(), pt->denoiseA.ptr, pt->denoiseB.ptr, pt->width, pt->height, iterations,
                                varianceFrames, sigmaLuminance, sigmaNormal, sigmaDepth, stream);
  HIP_TRY(hipGetLastError());
  return denoisedToHost(pt, host, stream);
}

int mi_pt_read_first_hit(MiPt* pt, float* host)
{
  FLUSH_PENDING(pt);
  if(!pt || !host || pt->width <= 0)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_first_hit: bad arguments");
  if(!pt->haveFirstHit)
    return fail(MI_PT_ERR_STATE, "mi_pt_read_first_hit: no MI_PT_FIRST_FRAME batch rendered at this size yet");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<float4> bySlot(size_t(std::max(pt->numSlots, 0)));
  if(!bySlot.empty())
    HIP_TRY(hipMemcpy(bySlot.data(), pt->firstHit.ptr, bySlot.size() * sizeof(float4), hipMemcpyDeviceToHost));
  scatterSlots(pt, bySlot.data(), bySlot.size(), 0, host, [](uint32_t) { return true; });
  return MI_PT_OK;
}

int mi_pt_set_temporal(MiPt* pt, int enable)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_temporal: null instance");
  if(enable && pt->cameraRays)
    return fail(MI_PT_ERR_STATE, "mi_pt_set_temporal: camera rays are bound (mi_pt_set_camera_rays) -- the motion image assumes the projective camera");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  pt->temporal = enable != 0;
  return allocTemporal(pt);
}

int mi_pt_read_motion(MiPt* pt, float* host)
{
  FLUSH_PENDING(pt);
  if(!pt || !host || pt->width <= 0)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_motion: bad arguments");
  if(!pt->temporal || !pt->temporalData.haveMotion)
    return fail(MI_PT_ERR_STATE, "mi_pt_read_motion: needs mi_pt_set_temporal and a MI_PT_FIRST_FRAME batch after it");
  return readImage(pt, pt->temporalData.motion.ptr, sizeof(float4), host);
}

void mi_pt_default_temporal(MiPtTemporalParams* p)
{
  if(!p)
    return;
  *p                = MiPtTemporalParams{};
  p->iterations     = 5;
  p->sigmaLuminance = 4.0f;
  p->sigmaNormal    = 128.0f;
  p->sigmaDepth     = 1.0f;
  p->alpha          = 0.2f;  // Schied et al. 2017, section 4.1
  p->momentsAlpha   = 0.2f;
  p->maxHistory     = 32.0f;
  p->normalCos      = 0.9f;  // (the spatial variance estimate's notion of "the same surface")
  p->depthTolerance = 0.1f;
}

int mi_pt_denoise_temporal(MiPt* pt, const MiPtTemporalParams* tp, float* host, void* hipStream)
{
  FLUSH_PENDING(pt);
  if(!pt || !tp || pt->width <= 0 || tp->iterations < 0 || tp->iterations > 8 || !(tp->sigmaLuminance > 0.0f) || !(tp->sigmaDepth > 0.0f) || !(tp->sigmaNormal >= 0.0f)
     || !(tp->alpha > 0.0f && tp->alpha <= 1.0f) || !(tp->momentsAlpha > 0.0f && tp->momentsAlpha <= 1.0f) || !(tp->maxHistory >= 1.0f)
     || !(tp->normalCos <= 1.0f) || !(tp->depthTolerance >= 0.0f))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_denoise_temporal: bad arguments");
  if(!pt->temporal || !pt->temporalData.haveMotion || !(pt->accumFrames >= 1.0f))
    return fail(MI_PT_ERR_STATE, "mi_pt_denoise_temporal: needs mi_pt_set_temporal and a MI_PT_FIRST_FRAME batch after it");
  if(pt->tileWorld > 1)
    return fail(MI_PT_ERR_STATE, "mi_pt_denoise_temporal: not under a tile partition (the history is not reduced across ranks)");
  HIP_TRY(hipSetDevice(pt->device));
  hipStream_t  stream = reinterpret_cast<hipStream_t>(hipStream);
  const size_t px     = size_t(pt->width) * size_t(pt->height);
  if(int rc = denoiseScratch(pt))
    return rc;
  auto set = [&](int i) {
    float4* base = pt->temporalData.history.ptr + size_t(i) * 3 * px;
    return pt::TemporalHistory{base, base + px, base + 2 * px};
  };
  const pt::TemporalConsts tc{tp->alpha, tp->momentsAlpha, tp->maxHistory, tp->normalCos, tp->depthTolerance};
  pt::launchSvgfReproject(pt->accum, pt->albedoImg(), pt->normalImg(), pt->depthImg(), pt->temporalData.motion.ptr, set(pt->temporalData.historyCur), set(pt->temporalData.historyCur ^ 1), pt->denoiseA.ptr,
                          pt->width, pt->height, tc, pt->temporalData.haveHistory, stream);
  pt->temporalData.historyCur ^= 1;
  pt->temporalData.haveHistory = true;
  pt->denoised    = pt::launchSvgfFilter(pt->denoiseA.ptr, pt->denoiseB.ptr, pt->accum, pt->albedoImg(), pt->normalImg(), pt->depthImg(), pt->width, pt->height,
                                         tp->iterations, tp->sigmaLuminance, tp->sigmaNormal, tp->sigmaDepth, stream);
  HIP_TRY(hipGetLastError());
  return denoisedToHost(pt, host, stream);
}

int mi_pt_reset_history(MiPt* pt)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_reset_history: null instance");
  pt->temporalData.haveHistory = false;
  return MI_PT_OK;
}

int mi_pt_set_vertex_motion(MiPt* pt, int enable)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_set_vertex_motion: null instance");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  pt->vertexMotion = enable != 0;
  pt->temporalData.haveHistory  = false;  // (the motion the history was reprojected along changes its meaning)
  return allocVertexMotion(pt);
}

int mi_pt_read_first_hit_triangle(MiPt* pt, uint32_t* host)
{
  FLUSH_PENDING(pt);
  if(!pt || !host || pt->width <= 0)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_first_hit_triangle: bad arguments");
  if(!vertexMotionActive(pt) || !pt->haveFirstHitTri || !pt->haveFirstHit)
    return fail(MI_PT_ERR_STATE, "mi_pt_read_first_hit_triangle: needs vertex motion in force (mi_pt_set_vertex_motion, mi_pt_set_temporal, "
                                 "mi_pt_set_deformation) and a MI_PT_FIRST_FRAME batch after it");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t        n = size_t(std::max(pt->numSlots, 0));
  std::vector<float4> hits(n);
  std::vector<uint4>  tris(n);
  if(n)
  {
    HIP_TRY(hipMemcpy(hits.data(), pt->firstHit.ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tris.data(), pt->firstHitTri.ptr, n * sizeof(uint4), hipMemcpyDeviceToHost));
  }
  scatterSlots(pt, tris.data(), n, 0xff, host, [&](uint32_t slot) {  // (a record only where the first hit is a surface)
    uint32_t id;
    memcpy(&id, &hits[slot].w, sizeof(id));
    return id != 0u && id != pt::TEMPORAL_ID_INVALID;
  });
  return MI_PT_OK;
}

int mi_pt_read_previous_positions(MiPt* pt, int renderPrimID, float* positions)
{
  FLUSH_PENDING(pt);
  if(!pt || !positions)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_previous_positions: bad arguments");
  if(!vertexMotionActive(pt))
    return fail(MI_PT_ERR_STATE, "mi_pt_read_previous_positions: vertex motion is not in force (mi_pt_set_vertex_motion, mi_pt_set_temporal, mi_pt_set_deformation or mi_pt_set_vertex_updates)");
  if(renderPrimID < 0 || size_t(renderPrimID) >= pt->vm.prevOffset.size() || pt->vm.prevOffset[size_t(renderPrimID)] == SIZE_MAX)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_read_previous_positions: render primitive " + std::to_string(renderPrimID) + " neither deforms nor is driven by the caller");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t nv = pt->primVertices[size_t(renderPrimID)];
  if(nv)
    HIP_TRY(hipMemcpy(positions, pt->vm.prevPositions.ptr + pt->vm.prevOffset[size_t(renderPrimID)], nv * 12, hipMemcpyDeviceToHost));
  return MI_PT_OK;
}

void mi_pt_default_tonemapper(MiTonemapperData* tm, int autoExposure)
{
  if(!tm)
    return;
  *tm                      = MiTonemapperData{};
  tm->method               = MI_TONEMAP_FILMIC;
  tm->isActive             = 1;
  tm->exposure             = 1.0f;
  tm->brightness           = 1.0f;
  tm->contrast             = 1.0f;
  tm->saturation           = 1.0f;
  tm->vignette             = 0.0f;
  tm->autoExposure         = autoExposure ? 1 : 0;
  tm->autoExposureSpeed    = 1.0f;
  tm->evMinValue           = -24.0f;
  tm->evMaxValue           = 8.0f;
  tm->enableCenterMetering = 0;
}

int mi_pt_tonemap(MiPt* pt, const MiTonemapperData* tm, int source, float dtSeconds, uint8_t* host, void* hipStream)
{
  FLUSH_PENDING(pt);
  if(!pt || !tm || pt->width <= 0 || source < 0 || source > 1)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_tonemap: bad arguments");
  if(tm->method < MI_TONEMAP_FILMIC || tm->method > MI_TONEMAP_KHRONOS_PBR || !(tm->brightness > 0.0f) || !(tm->evMaxValue > tm->evMinValue))
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_tonemap: method outside [0, 5], brightness <= 0 or an empty EV range");
  const size_t px = size_t(pt->width) * size_t(pt->height);
  if(source == 1 && (!pt->denoised || pt->denoiseA.count != px))
    return fail(MI_PT_ERR_STATE, "mi_pt_tonemap: source 1 needs a mi_pt_denoise result of the current size");
  HIP_TRY(hipSetDevice(pt->device));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hipStream);
  if(pt->tonemapped.count != px)
    HIP_TRY(pt->tonemapped.alloc(px));
  if(!pt->tmHistogram.ptr)
  {
    HIP_TRY(pt->tmHistogram.alloc(256));
    HIP_TRY(pt->tmAutoState.alloc(2));
    HIP_TRY(hipMemset(pt->tmAutoState.ptr, 0, 2 * sizeof(float)));
  }
  pt::launchTonemap(source == 1 ? pt->denoised : pt->accum, pt->tonemapped.ptr, pt->width, pt->height, *tm, pt->tmHistogram.ptr, pt->tmAutoState.ptr,
                    dtSeconds, stream);
  HIP_TRY(hipGetLastError());
  if(host)
  {
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(host, pt->tonemapped.ptr, px * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return MI_PT_OK;
}

const void* mi_pt_denoised_device_ptr(MiPt* pt)
{
  return pt ? pt->denoised : nullptr;
}

void* mi_pt_tonemapped_device_ptr(MiPt* pt)
{
  return pt ? pt->tonemapped.ptr : nullptr;
}

int mi_pt_get_memory(MiPt* pt, MiPtMemory* out)
{
  if(!pt || !out)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_get_memory: null argument");
  HIP_TRY(hipSetDevice(pt->device));
  // The feature groups sum themselves (MiPt::*::bytes()); every other buffer is named here.  Four small ones are in neither total, as they
  // never were: matDirty, skyConsts.skyPre, tmHistogram and tmAutoState.  Counting them is a change of what the totals report, not of this bookkeeping.
  const uint64_t scene = pt->materials.bytes() + pt->texInfos.bytes() + pt->nodes.bytes() + pt->prims.bytes() + pt->lights.bytes() + pt->textures.bytes() + pt->texels.bytes() + pt->texQuads.bytes()
                         + pt->geometry.bytes() + pt->instFlags.bytes() + pt->srgbLut.bytes() + pt->envPixels.bytes() + pt->envAccel.bytes() + pt->texRefs.bytes()
                         + pt->coreTex.bytes() + pt->deform.bytes() + pt->vm.bytes() + pt->vu.bytes() + pt->tuTables.bytes() + pt->accel.bytes();
  const uint64_t pathState = pt->pathArrays.bytes() + pt->optThroughput.bytes() + pt->optMisc.bytes() + pt->optMedium.bytes() + pt->optPixelSum.bytes() + pt->optGuides.bytes()
                             + pt->optShadowAux2.bytes() + pt->queueMem.bytes() + pt->queuePayload.bytes() + pt->candPool.bytes() + pt->candLists.bytes();
  const uint64_t renderer = pathState + pt->firstHit.bytes() + pt->accumOwn.bytes()
                            + pt->albedo.bytes() + pt->normal.bytes() + pt->denoiseA.bytes() + pt->denoiseB.bytes() + pt->tonemapped.bytes() + pt->depth.bytes()
                            + pt->selection.bytes() + pt->cameraRaysOwn.bytes() + pt->allTiles.bytes() + pt->queryRays.bytes() + pt->queryHits.bytes() + pt->vuStaging.bytes() + pt->tuStaging.bytes() + pt->euScratch.bytes() + pt->ownedTiles.bytes() + pt->sceneDev.bytes() + pt->fcConsts.fcRing.bytes() + pt->stats.bytes()
                            + pt->temporalData.bytes() + pt->firstHitTri.bytes();
  size_t freeB = 0, totalB = 0;
  HIP_TRY(hipMemGetInfo(&freeB, &totalB));
  out->sceneBytes       = scene;
  out->rendererBytes    = renderer;
  out->deviceUsedBytes  = uint64_t(totalB - freeB);
  out->deviceTotalBytes = uint64_t(totalB);
  out->pathStateBytes   = pathState;
  out->pathSlots        = uint64_t(std::max(pt->numSlots, 0)) * uint64_t(std::max(pt->framesCap, 1));
  return MI_PT_OK;
}

int mi_pt_get_stats(MiPt* pt, MiPtStats* out)
{
  FLUSH_PENDING(pt);
  if(!pt || !out)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_get_stats: null argument");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  pt::StatCounters h{};
  HIP_TRY(hipMemcpy(&h, pt->stats.ptr, sizeof(h), hipMemcpyDeviceToHost));
  *out              = pt->staticStats;
  out->cameraPaths  = h.cameraPaths;
  out->segments     = h.segments;
  out->shadowRays   = h.shadowRays;
  out->nodesClosest = h.nodesClosest;
  out->trisClosest  = h.trisClosest;
  out->nodesShadow  = h.nodesShadow;
  out->trisShadow   = h.trisShadow;
  out->textureTaps  = h.textureTaps;
  out->surfaceHits  = h.surfaceHits;
  out->nodesPrimary = h.nodesPrimary;
  out->trisPrimary  = h.trisPrimary;
  return MI_PT_OK;
}
int mi_pt_reset_stats(MiPt* pt)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_reset_stats: null instance");
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(pt->stats.ptr, 0, sizeof(pt::StatCounters)));
  return MI_PT_OK;
}
int mi_pt_enable_timing(MiPt* pt, int enable)
{
  FLUSH_PENDING(pt);
  if(!pt)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_enable_timing: null instance");
  pt->timer.timingEnabled = enable != 0;
  if(enable)
  {
    pt->timer.reset();
    pt->timer.accTiming = MiPtFrameTiming{};
  }
  return MI_PT_OK;
}
int mi_pt_get_frame_timing(MiPt* pt, MiPtFrameTiming* out)
{
  FLUSH_PENDING(pt);
  if(!pt || !out)
    return fail(MI_PT_ERR_ARGUMENT, "mi_pt_get_frame_timing: null argument");
  // Totals since mi_pt_enable_timing(1): resolves the recorded events (one device synchronisation, here, not per frame).
  HIP_TRY(hipSetDevice(pt->device));
  HIP_TRY(hipDeviceSynchronize());
  pt->timer.resolve();
  *out = pt->timer.accTiming;
  return MI_PT_OK;
}
}
