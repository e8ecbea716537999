// The single-threaded host collapse of a BVH2 into the 8-wide BVH (node layout and contract: bvh8.hip), as a function over plain arrays, and the
// texts it shares with the device collapse of bvh8.hip: how a BVH2 record is read and the surface area the greedy opening compares.  The child
// boxes are quantised by quantiseNode8 (bvh_refit.h), one text for both collapses and the refit; the octant-ordered slot assignment is the one
// statement the two collapses hold a copy each of (assignSlots8 below).  No HIP call in here: compiles for the host as well (tests/host_shim/collapse_on_host.cpp), where
// tests/test_bvh8_collapse_on_host.py checks the contract of the node array on trees written in numpy.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

#include "bvh_refit.h"

namespace pt {

// One rounding per operation where the bits decide a comparison both sides must take alike (__fadd_rn & co. have no host definition under hipcc).
#if defined(__HIP_DEVICE_COMPILE__)
PT_HOST_DEV float addOnce(float a, float b) { return __fadd_rn(a, b); }
PT_HOST_DEV float mulOnce(float a, float b) { return __fmul_rn(a, b); }
#else
PT_HOST_DEV float addOnce(float a, float b) { return a + b; }
PT_HOST_DEV float mulOnce(float a, float b) { return a * b; }
#endif

// A child an 8-wide node may take: a BVH2 subtree and the box its BVH2 parent holds for it.
struct Cand8
{
  int   ref;  // >= 0 BVH2 inner node, < 0 leaf (~triangle index in BVH2 order)
  float lo[3], hi[3];
};
// The BVH2 record (4 x float4 per inner node: bvh_build.hip, k_emit_nodes / k_ploc_emit): child references, triangles below, child boxes.
PT_HOST_DEV int floatAsInt(float f)  // (__float_as_int, which the host pass of hipcc does not have)
{
  int i;
  __builtin_memcpy(&i, &f, sizeof(i));
  return i;
}
PT_HOST_DEV int childRef2(const float4* nodes2, int node, int which)
{
  const float4 n3 = nodes2[size_t(node) * 4 + 3];
  return floatAsInt(which == 0 ? n3.x : n3.y);
}
PT_HOST_DEV uint32_t triCount2(const float4* nodes2, int ref) { return ref >= 0 ? uint32_t(floatAsInt(nodes2[size_t(ref) * 4 + 3].z)) : 1u; }
PT_HOST_DEV void childBox2(const float4* nodes2, int node, int which, float lo[3], float hi[3])
{
  const float4 n0 = nodes2[size_t(node) * 4 + 0], n1 = nodes2[size_t(node) * 4 + 1], n2 = nodes2[size_t(node) * 4 + 2];
  if(which == 0) { lo[0] = n0.x; hi[0] = n0.y; lo[1] = n0.z; hi[1] = n0.w; lo[2] = n2.x; hi[2] = n2.y; }
  else           { lo[0] = n1.x; hi[0] = n1.y; lo[1] = n1.z; hi[1] = n1.w; lo[2] = n2.z; hi[2] = n2.w; }
}
PT_HOST_DEV void childCand2(const float4* nodes2, int node, int which, Cand8& c)
{
  c.ref = childRef2(nodes2, node, which);
  childBox2(nodes2, node, which, c.lo, c.hi);
}
// half the surface area of a box (fixed association; NB __fmul_rn / __fadd_rn are a plain * and + in this ROCm and hipcc may still fuse them --
// bvh_reinsert.h: r2Area, where the bits matter, uses the pragma)
PT_HOST_DEV float boxArea8(const float lo[3], const float hi[3])
{
  const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  return addOnce(addOnce(mulOnce(ex, ey), mulOnce(ey, ez)), mulOnce(ez, ex));
}
// ---- the host collapse ------------------------------------------------------------------------------------------------------------
// Largest leaf child: 2 triangles (two bits of the node's valid mask belong to a slot, bvh8.hip).  A node then holds at most 16 leaf
// triangles, which its masks always have room for.
constexpr uint32_t BVH8_MAX_LEAF = 2;

// Octant-ordered slot assignment of the `count` children of a node with frame [lo, hi]: greedy on dot(centroid - centre, slot diagonal), ties by
// (candidate, slot) order.  candOfSlot[s]: the candidate in slot s, -1 for an empty slot.
// DEVICE TWIN: the slot loop of k_collapse_emit (bvh8.hip), which states the same operations through __fadd_rn / __fsub_rn / __fmul_rn; the
// kernel's code changes when it calls a function for them, so the two stand side by side (tests: configuration F of the builder matrix and
// test_device_bvh8_collapse_equals_host_collapse compare what they make).
inline void assignSlots8(const Cand8* cands, int count, const float lo[3], const float hi[3], int candOfSlot[8])
{
  bool slotUsed[8] = {false, false, false, false, false, false, false, false}, done[8] = {false, false, false, false, false, false, false, false};
  for(int s = 0; s < 8; ++s)
    candOfSlot[s] = -1;
  for(int round = 0; round < count; ++round)
  {
    float bestCost = -FLT_MAX;
    int   bc = -1, bs = -1;
    for(int c = 0; c < count; ++c)
    {
      if(done[c])
        continue;
      float d[3];
      for(int a = 0; a < 3; ++a)
        d[a] = 0.5f * (cands[c].lo[a] + cands[c].hi[a]) - 0.5f * (lo[a] + hi[a]);
      for(int s = 0; s < 8; ++s)
      {
        if(slotUsed[s])
          continue;
        const float cost = ((s & 1) ? d[0] : -d[0]) + ((s & 2) ? d[1] : -d[1]) + ((s & 4) ? d[2] : -d[2]);
        if(cost > bestCost)
        {
          bestCost = cost;
          bc       = c;
          bs       = s;
        }
      }
    }
    candOfSlot[bs] = bc;
    slotUsed[bs]   = true;
    done[bc]       = true;
  }
}
// The node over `count` children but for its children's indices: frame, slots, and the child boxes quantised from clo / chi / used built the
// way k_collapse_emit builds them.
inline void frameAndQuantise8(Node8& N, const Cand8* cands, int count, int candOfSlot[8])
{
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for(int k = 0; k < count; ++k)
    for(int a = 0; a < 3; ++a)
    {
      lo[a] = fminf(lo[a], cands[k].lo[a]);
      hi[a] = fmaxf(hi[a], cands[k].hi[a]);
    }
  assignSlots8(cands, count, lo, hi, candOfSlot);
  memset(&N, 0, sizeof(N));
  float    clo[3][8], chi[3][8];
  uint32_t used = 0;
  for(int sl = 0; sl < 8; ++sl)
  {
    const int c = candOfSlot[sl] < 0 ? 0 : candOfSlot[sl];
    for(int a = 0; a < 3; ++a) { clo[a][sl] = cands[c].lo[a]; chi[a][sl] = cands[c].hi[a]; }
    used |= candOfSlot[sl] < 0 ? 0u : 1u << sl;
  }
  quantiseNode8(N, lo, hi, clo, chi, used);  // (bvh_refit.h: one text with k_collapse_emit and the refit)
}

struct Bvh8OnHost
{
  std::vector<Node8>    nodes;  // breadth-first; node 0 is the root
  std::vector<uint32_t> perm;   // new triangle index -> BVH2 triangle index
  uint32_t              numLevels = 0;
};

// the (at most BVH8_MAX_LEAF) triangles below a small subtree, left to right
inline void appendTris8(const float4* nodes2, int ref, std::vector<uint32_t>& dst)
{
  if(ref < 0)
  {
    dst.push_back(uint32_t(~ref));
    return;
  }
  appendTris8(nodes2, childRef2(nodes2, ref, 0), dst);
  appendTris8(nodes2, childRef2(nodes2, ref, 1), dst);
}

// Breadth-first greedy collapse of the BVH2 `nodes2` (numInner records, n leaves, root `root`): every node opens its inner child of largest
// surface area that holds more than BVH8_MAX_LEAF triangles until it has eight children or nothing left to open -- the greedy tree of the
// device collapse (MI_PT_COLLAPSE=greedy), node for node.  numInner == 0: one triangle, whose box is [loneLo, loneHi].  perm.size() != n
// afterwards means the records lost triangles.
inline Bvh8OnHost collapseBvh8OnHost(const float4* nodes2, int root, uint32_t numInner, uint32_t n, const float loneLo[3], const float loneHi[3])
{
  Bvh8OnHost r;
  r.perm.reserve(n);
  struct Work
  {
    int      ref;    // the BVH2 node it is rooted at (the lone triangle: ~0)
    uint32_t level;  // nodes above it
  };
  std::vector<Work> queue{Work{root, 0u}};  // queue[i] becomes r.nodes[i]
  r.nodes.emplace_back();
  for(size_t qi = 0; qi < queue.size(); ++qi)
  {
    const Work w = queue[qi];
    r.numLevels  = std::max(r.numLevels, w.level + 1u);
    Cand8 cands[8];
    int   count = numInner ? 2 : 1;
    if(numInner)
      for(int k = 0; k < 2; ++k)
        childCand2(nodes2, w.ref, k, cands[k]);
    else
    {
      cands[0].ref = ~0;
      for(int a = 0; a < 3; ++a) { cands[0].lo[a] = loneLo[a]; cands[0].hi[a] = loneHi[a]; }
    }
    while(count < 8)
    {
      int   best  = -1;
      float bestA = -1.0f;
      for(int k = 0; k < count; ++k)
        if(cands[k].ref >= 0 && triCount2(nodes2, cands[k].ref) > BVH8_MAX_LEAF && boxArea8(cands[k].lo, cands[k].hi) > bestA)
        {
          bestA = boxArea8(cands[k].lo, cands[k].hi);
          best  = k;
        }
      if(best < 0)
        break;
      const int ref = cands[best].ref;
      childCand2(nodes2, ref, 0, cands[best]);
      childCand2(nodes2, ref, 1, cands[count++]);
    }
    Node8 N;
    int   candOfSlot[8];
    frameAndQuantise8(N, cands, count, candOfSlot);
    // children: inner ones get consecutive node indices in slot order, leaf ones consecutive triangles
    N.childBase = uint32_t(r.nodes.size());
    N.triBase   = uint32_t(r.perm.size());
    for(int s = 0; s < 8; ++s)
    {
      if(candOfSlot[s] < 0)
        continue;
      const Cand8&   c  = cands[candOfSlot[s]];
      const uint32_t tc = triCount2(nodes2, c.ref);
      if(tc > BVH8_MAX_LEAF)
      {
        N.imask |= uint8_t(1u << s);
        r.nodes.emplace_back();
        queue.push_back(Work{c.ref, w.level + 1u});
      }
      else
      {
        N.valid |= uint16_t((tc >= 2u ? 3u : 1u) << (2 * s));
        appendTris8(nodes2, c.ref, r.perm);
      }
    }
    r.nodes[qi] = N;
  }
  return r;
}

}  // namespace pt
