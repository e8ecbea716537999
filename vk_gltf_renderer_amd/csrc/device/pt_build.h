// Host-side interface of the on-device BVH builder (bvh_build.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "dev_buf.h"
#include "pt_scene.h"

namespace pt {

struct BvhBuildInput
{
  const MiGltfRenderNode* nodes;          // device
  const DevPrim*          prims;          // device
  const uint8_t*          instFlags;      // device, per render node
  const uint32_t*         nodeTriOffset;  // device, numEntries + 1
  const int32_t*          entryNode;      // device, numEntries
  int                     numEntries;
  uint32_t                numTris;
  bool                    karrasTopology = false;  // true: plain LBVH (Morton-prefix hierarchy); false: PLOC clustering
  int                     reinsertPasses = 0;      // parallel reinsertion over the finished BVH2 (bvh_reinsert.h): searches ...
  int                     reinsertRounds = 4;      // ... and lock / move rounds per search
  float                   splitFactor    = 0.0f;   // triangle pre-splitting (bvh_split.h): references for parts whose box area exceeds this x the mean; 0 = off
  int                     splitMaxDepth  = 8;      // ... at most 2^this references per triangle
  float                   splitMinShare  = 0.1f;   // ... and only in scenes where triangles above 64 x the mean hold at least this share of the summed box area (0 = always)
  int                     maxHeight      = 0;      // inner nodes above any leaf of the BVH2 handed out: what the walk's stack holds (0 = unbounded, unmeasured); a taller
                                                   // tree is built again with the Morton-prefix topology, then without reinsertion; still taller: the build fails
};
struct BvhBuildOutput
{
  DevBuf<float4> nodes;  // 4 float4 per node
  DevBuf<DevTri> tris;   // Morton order (leaf reference ~i = triangle i of this array)
  uint32_t numNodes = 0, numTris = 0;   // numTris = REFERENCES: a pre-split triangle appears once per reference (each a full copy of its record)
  uint32_t sceneTris = 0;               // triangles the references were made from
  int      root     = 0;
  uint32_t reinsertMoves = 0;   // subtrees the reinsertion passes moved
  uint32_t height        = 0;   // of the BVH2, measured only under BvhBuildInput::maxHeight
  float    centroidLo[3] = {0, 0, 0}, centroidHi[3] = {0, 0, 0};
};
bool buildBvh(const BvhBuildInput& in, BvhBuildOutput& out, hipStream_t stream, std::string& err);

struct RefitBox;  // bvh_refit.h

// 8-wide compressed BVH collapsed from the BVH2 above (bvh8.hip)
struct Bvh8Output
{
  DevBuf<uint4>  nodes;  // 5 uint4 per node
  DevBuf<DevTri> tris;   // node order (triangles of a node's leaf children are contiguous)
  uint32_t numNodes = 0, numTris = 0;
  uint32_t numLevels = 0;  // nodes on the longest path from the root
  // the refit data (Bvh8Options::keepRefit, device collapse only): per triangle slot the box the builder
  // filed that reference under, per node room for its box (left for k_refit_level to fill), and the start of every level of the
  // breadth-first node array (+ numNodes at the end)
  DevBuf<RefitBox>      nodeBox, slotBox;
  std::vector<uint32_t> levels;
};
struct Bvh8Options  // (MI_PT_COLLAPSE / MI_PT_HOST_COLLAPSE, read and validated once in mi_pt_create: RunSwitches)
{
  bool sahCollapse  = true;   // SAH-optimal dynamic programme (default) | greedy by surface area
  bool hostCollapse = false;  // the greedy host collapse (A/B reference of the device one)
  bool keepRefit    = false;  // also return the refit data (mi_pt_set_accel_update: REFIT / AUTO)
};

// In-place refit of the 8-wide BVH (bvh_refit.hip).  k_refit_tris: the triangle records and slot boxes of the slots whose render node's
// byte in `dirty` is not REFIT_CLEAN (bvh_refit.h); k_refit_level, one launch per level, deepest first: every node requantised from its
// children's boxes, its box into nodeBox and its SAH term into sahTerm; the SAH cost of the tree from those terms, in a fixed reduction order
// (bit-reproducible).
void launchRefitTris(const MiGltfRenderNode* nodes, const DevPrim* prims, const uint8_t* instFlags, const uint8_t* dirty, const RefitBox* builtBox,
                     DevTri* tris, RefitBox* slotBox, uint32_t numTris, hipStream_t s);
void launchRefitLevels(uint4* nodes, const std::vector<uint32_t>& levels, const RefitBox* slotBox, RefitBox* nodeBox, float* sahTerm, hipStream_t s);
constexpr int REFIT_SAH_PARTIALS = 1024;  // partial sums of the cost reduction (the `partial` array: this + 1 doubles)
void launchSahCost(const float* sahTerm, uint32_t numNodes, const RefitBox* nodeBox, double* partial, hipStream_t s);  // the cost -> partial[REFIT_SAH_PARTIALS]
bool buildBvh8(const BvhBuildOutput& b2, Bvh8Output& out, hipStream_t stream, std::string& err, const Bvh8Options& opt = Bvh8Options());

}  // namespace pt
