// BVH2 -> 8-wide compressed BVH (80-byte nodes) for incoherent traversal on gfx950.
//
// Why: with one ray per lane a BVH2 visit is 4 divergent dwordx4 loads (64 distinct cache lines per wave instruction);
// the profile shows the L1/TA request rate, not ALU, bounds the walk.  An 8-wide node with 8-bit quantised child boxes
// (layout after Ylitie, Karras, Laine 2017, "Efficient Incoherent Ray Traversal on GPUs Through Compressed Wide BVHs")
// needs ~3.5x fewer node visits per ray at 80 B per visit.
//
// Node (5 x uint4):
//   [0] p.x p.y p.z (float bits) | ex | ey<<8 | ez<<16 | imask<<24      quantisation frame: lo corner + per-axis 2^e
//   [1] childBase | triBase | valid16 | 0             valid16: bit 2s = leaf child in slot s has a triangle, bit 2s + 1 = it has two
//       (a leaf child's triangles follow those of the leaf children in lower slots: index = triBase + popcount(valid16 below its bit);
//        an inner child is a bit of imask, an empty slot is neither)
//   [2] qlo.x[0..7] qlo.y[0..7]   [3] qlo.z[0..7] qhi.x[0..7]   [4] qhi.y[0..7] qhi.z[0..7]
// Child boxes decode as fmaf(q, 2^e, p) — the builder checks with the same fmaf that every decoded box CONTAINS the true
// box, so the structure is conservative and the image cannot depend on it (parity contract).
// Internal children of a node are stored contiguously from childBase in slot order; the triangles of its leaf children
// are stored contiguously from triBase in slot order (<= 2 per child, <= 16 per node: the walk turns its 8-bit child hit mask into
// triangle bits with one bit-doubling spread and one AND, pt_bvh8.h).  Children sit in octant-ordered slots so that
// `slot ^ (7 ^ rayOctant)` is a front-to-back priority.
//
// The collapse runs ON THE DEVICE, level by level over the BVH2 the builder left in HBM (no download): one thread per 8-wide node of
// the level picks its (up to eight) children -- by default the SAH-optimal choice of Ylitie et al. 2017, read from tables a bottom-up
// dynamic programme over the BVH2 leaves behind (k_dp_solve); MI_PT_COLLAPSE=greedy opens BVH2 children by surface area instead --
// orders them by octant, quantises their boxes and writes the 80-byte record; a prefix sum over the level hands every node the indices of its inner children (= the next level's
// work list, breadth-first order) and the positions of its leaf triangles.  Two kernels and one scan per level, ~10 levels.  The
// single-threaded host collapse it replaces (0.6 s of a 0.86 s scene build at 2.6 M triangles in round 1) is kept behind
// MI_PT_HOST_COLLAPSE=1 as the A/B reference and serves the one-triangle scene; it lives in `bvh8_collapse_host.h` and is tested on the CPU
// (tests/test_bvh8_collapse_on_host.py).  Both emit the same node array from the greedy opening, quantised by one text (bvh_refit.h).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh8_collapse_host.h"
#include "bvh_refit.h"
#include "pt_build.h"
#include "pt_ticket.h"
#include "pt_bvh.h"

namespace pt {

namespace {

// (Node8, the 80-byte record: bvh_refit.h, shared with the refit; Cand8, childRef2, triCount2, childBox2, boxArea8: bvh8_collapse_host.h, one
//  text for this collapse and the host's)

// Largest leaf child: 2 triangles (BVH8_MAX_LEAF, bvh8_collapse_host.h: the host collapse opens by the same size).  Two bits of the node's 16-bit valid mask belong to
// a slot, so a leaf child holds one or two triangles -- which is also what measured best when the mask had room for three and four
// (round 2: 2 beats 1, 3 and 4 on the helmet, atrium and street workloads, +0.4 .. +2.5 % over 3).
// SAH-optimal collapse by default: against the greedy one (MI_PT_COLLAPSE=greedy) 40 % fewer, fuller nodes (atrium 68.8 k -> 44 k),
// node visits per secondary ray 19.74 -> 19.27 (atrium), 28.66 -> 27.55 (street), 8.01 -> 7.91 (helmet), and
// atrium 482 -> 490, street 512 -> 518, helmet 3799 -> 3878, glass 537 -> 551 Msamples/s (round 3)

__global__ void k_reorder_tris(uint32_t n, const uint32_t* perm, const DevTri* in, DevTri* out)
{
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i < n)
    out[i] = in[perm[i]];
}

// ---- device collapse: SAH-optimal collapse (Ylitie, Karras, Laine 2017, section 3.2) ------------------------------------------------------------
// cost[n][i], i = 1..7: the cheapest way to represent the BVH2 subtree n as AT MOST i children of some 8-wide node -- each such child
// either a leaf (the subtree has <= maxLeaf triangles; cost = area x C_TRI x triangles) or an inner 8-wide node (cost = area x 1 +
// the cheapest forest of <= 8 children below it).  C_TRI = 56 / 235: a triangle test against a node visit in vector instructions.
// split[n][i]: how many of the i roots go to the left BVH2 child (-1: the subtree stays one child); split[n][1]: 0 = leaf, 1 = inner
// node; split[n][0]: the left share of the inner node's eight.  Filled bottom-up (second arrival at a node solves it, like k_fit),
// read top-down by the level kernels instead of the greedy opening.
// (MI_PT_DP_C_TRI: bvh_refit.h, whose SAH cost of a refitted tree weighs triangles the same way)
constexpr float DP_C_TRI = MI_PT_DP_C_TRI;
struct DpTables
{
  float*  cost;   // numInner x 8 ([0] unused)
  int8_t* split;  // numInner x 8
};
__global__ void k_dp_parents(int numInner, const float4* nodes2, int* parent, int* leafParent, int root)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= numInner)
    return;
  for(int k = 0; k < 2; ++k)
  {
    const int c = childRef2(nodes2, i, k);
    if(c >= 0)
      parent[c] = i;
    else
      leafParent[~c] = i;
  }
  if(i == root)
    parent[i] = -1;
}
__device__ void d_dpSolve(const float4* nodes2, DpTables dp, int nd, uint32_t maxLeaf)
{
  int   ref[2];
  float leafCost[2];  // cost of a child that is a single triangle
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for(int k = 0; k < 2; ++k)
  {
    ref[k] = childRef2(nodes2, nd, k);
    float l[3], h[3];
    childBox2(nodes2, nd, k, l, h);
    leafCost[k] = boxArea8(l, h) * DP_C_TRI;
    for(int a = 0; a < 3; ++a)
    {
      lo[a] = fminf(lo[a], l[a]);
      hi[a] = fmaxf(hi[a], h[a]);
    }
  }
  const float area = boxArea8(lo, hi);
  // The cost tables are what one thread of this kernel writes and another (the solver of the parent, possibly on another XCD) reads: they go through
  // agent-scope relaxed atomic loads and stores (coherent past the per-XCD L2s), ordered against the ticket in k_dp_solve by the stores'
  // acknowledgement -- not through plain stores between two device-scope fences, which cost an L2 write-back + invalidate per thread and level
  // (round 5: the same change as the reinsertion refit, bvh_reinsert.h).  The split tables are read by later kernels only.
  float childCost[2][8];
  for(int k = 0; k < 2; ++k)
    for(int i = 1; i < 8; ++i)
      childCost[k][i] = ref[k] < 0 ? leafCost[k] : __hip_atomic_load(dp.cost + size_t(ref[k]) * 8 + size_t(i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  auto get = [&](int k, int i) { return childCost[k][min(i, 7)]; };
  float   c[8];
  int8_t* s = dp.split + size_t(nd) * 8;
  for(int i = 2; i <= 7; ++i)
  {
    float best = FLT_MAX;
    int   bk   = 1;
    for(int k = 1; k < i; ++k)
    {
      const float v = get(0, k) + get(1, i - k);
      if(v < best)
      {
        best = v;
        bk   = k;
      }
    }
    c[i] = best;
    s[i] = int8_t(bk);
  }
  float inner = FLT_MAX;
  int   bk    = 1;
  for(int k = 1; k < 8; ++k)
  {
    const float v = get(0, k) + get(1, 8 - k);
    if(v < inner)
    {
      inner = v;
      bk    = k;
    }
  }
  inner += area;
  const uint32_t cnt  = triCount2(nodes2, nd);
  const float    leaf = cnt <= maxLeaf ? area * DP_C_TRI * float(cnt) : FLT_MAX;
  c[0] = 0.0f;
  c[1] = leaf <= inner ? leaf : inner;
  s[1] = leaf <= inner ? 0 : 1;
  s[0] = int8_t(bk);
  for(int i = 2; i <= 7; ++i)
    if(c[1] < c[i])
    {
      c[i] = c[1];
      s[i] = -1;
    }
  for(int i = 0; i < 8; ++i)
    __hip_atomic_store(dp.cost + size_t(nd) * 8 + size_t(i), c[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void k_dp_solve(int numLeaves, const float4* nodes2, const int* parent, const int* leafParent, unsigned* arrive, DpTables dp, uint32_t maxLeaf)
{
  const int leaf = blockIdx.x * blockDim.x + threadIdx.x;
  if(leaf >= numLeaves)
    return;
  int cur = leafParent[leaf];
  while(cur >= 0)
  {
    // (this thread's write-through stores of d_dpSolve are acknowledged before its ticket, the ticket has returned before the tables are read: pt_ticket.h)
    if(pt::ticketArrive(&arrive[cur]) == 0u)
      return;  // first arrival: the sibling subtree finishes this node
    d_dpSolve(nodes2, dp, cur, maxLeaf);
    cur = parent[cur];
  }
}
// is the candidate an INNER child (an 8-wide node of its own) or a leaf child?  greedy: by its triangle count; DP: as the table decided
__device__ __forceinline__ bool d_isInner(const float4* nodes2, const DpTables& dp, int ref, uint32_t maxLeaf)
{
  if(ref < 0)
    return false;
  if(dp.split)
    return dp.split[size_t(ref) * 8 + 1] != 0;
  return triCount2(nodes2, ref) > maxLeaf;
}
// The children of the 8-wide node rooted at BVH2 node `ref` as the DP tables chose them.
__device__ int d_expandDp(const float4* nodes2, const DpTables& dp, int ref, Cand8 cands[8])
{
  struct Item
  {
    int ref, parentNode, which, share;
  };
  Item stack[16];
  int  sp = 0, count = 0;
  const int k0 = dp.split[size_t(ref) * 8 + 0];
  stack[sp++] = Item{childRef2(nodes2, ref, 1), ref, 1, 8 - k0};  // (right first: popped last, so the children come out left to right)
  stack[sp++] = Item{childRef2(nodes2, ref, 0), ref, 0, k0};
  while(sp > 0)
  {
    const Item it = stack[--sp];
    const int  sh = min(it.share, 7);
    const int  sv = it.ref >= 0 ? int(dp.split[size_t(it.ref) * 8 + size_t(sh)]) : -1;
    if(it.ref < 0 || sh <= 1 || sv < 0)
    {
      if(count < 8)
      {
        cands[count].ref = it.ref;
        childBox2(nodes2, it.parentNode, it.which, cands[count].lo, cands[count].hi);
        ++count;
      }
      continue;
    }
    if(sp + 2 <= 16)
    {
      stack[sp++] = Item{childRef2(nodes2, it.ref, 1), it.ref, 1, sh - sv};
      stack[sp++] = Item{childRef2(nodes2, it.ref, 0), it.ref, 0, sv};
    }
  }
  return count;
}
// The children of the 8-wide node that starts at BVH2 node `ref`: greedy, always open the inner child of largest surface area that
// holds more than maxLeaf triangles, until there are eight (or nothing left to open).  Returns how many, and the leaf size used.
__device__ int d_expand(const float4* nodes2, const DpTables& dp, int ref, uint32_t maxLeafIn, Cand8 cands[8], uint32_t& maxLeafOut)
{
  if(dp.split)
  {
    maxLeafOut = maxLeafIn;  // (<= 3 in this mode: eight leaf children always fit the node's triangle mask)
    return d_expandDp(nodes2, dp, ref, cands);
  }
  uint32_t maxLeaf = maxLeafIn;
  int      count;
  for(;;)
  {
    count = 2;
    for(int k = 0; k < 2; ++k)
    {
      cands[k].ref = childRef2(nodes2, ref, k);
      childBox2(nodes2, ref, k, cands[k].lo, cands[k].hi);
    }
    while(count < 8)
    {
      int   best  = -1;
      float bestA = -1.0f;
      for(int k = 0; k < count; ++k)
        if(cands[k].ref >= 0 && triCount2(nodes2, cands[k].ref) > maxLeaf)
        {
          const float a = boxArea8(cands[k].lo, cands[k].hi);
          if(a > bestA)
          {
            bestA = a;
            best  = k;
          }
        }
      if(best < 0)
        break;
      const int r = cands[best].ref;
      cands[best].ref = childRef2(nodes2, r, 0);
      childBox2(nodes2, r, 0, cands[best].lo, cands[best].hi);
      cands[count].ref = childRef2(nodes2, r, 1);
      childBox2(nodes2, r, 1, cands[count].lo, cands[count].hi);
      ++count;
    }
    uint32_t leafTris = 0;
    for(int k = 0; k < count; ++k)
    {
      const uint32_t tc = triCount2(nodes2, cands[k].ref);
      leafTris += cands[k].ref < 0 ? 1u : (tc <= maxLeaf ? tc : 0u);
    }
    if(leafTris <= 31u || maxLeaf <= 3u)
      break;
    maxLeaf = 3u;  // would not fit the node's triangle mask
  }
  maxLeafOut = maxLeaf;
  return count;
}
// pass 1 of a level: how many inner children (low word) and leaf triangles (high word) each node of the level will have
__global__ void k_collapse_count(int numItems, const int* items, const float4* nodes2, DpTables dp, uint32_t maxLeaf, unsigned long long* counts)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= numItems)
    return;
  Cand8    cands[8];
  uint32_t ml;
  const int count = d_expand(nodes2, dp, items[i], maxLeaf, cands, ml);
  uint32_t  inner = 0, tris = 0;
  for(int k = 0; k < count; ++k)
  {
    const uint32_t tc = triCount2(nodes2, cands[k].ref);
    if(d_isInner(nodes2, dp, cands[k].ref, ml))
      ++inner;
    else
      tris += tc;
  }
  counts[i] = (unsigned long long)inner | ((unsigned long long)tris << 32);
}
// pass 2: the node records, the next level's work list, the triangle permutation
__global__ void k_collapse_emit(int numItems, const int* items, const float4* nodes2, DpTables dp, uint32_t maxLeaf, const unsigned long long* counts,
                                const unsigned long long* offsets, uint32_t levelStart, uint32_t nextLevelStart, uint32_t triLevelBase, Node8* nodes8,
                                int* nextItems, uint32_t* perm, unsigned long long* totals, RefitBox* slotBox)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= numItems)
    return;
  if(i == numItems - 1)
    *totals = offsets[i] + counts[i];
  Cand8    cands[8];
  uint32_t ml;
  const int count = d_expand(nodes2, dp, items[i], maxLeaf, cands, ml);
  // node frame
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for(int k = 0; k < count; ++k)
    for(int a = 0; a < 3; ++a)
    {
      lo[a] = fminf(lo[a], cands[k].lo[a]);
      hi[a] = fmaxf(hi[a], cands[k].hi[a]);
    }
  // octant-ordered slot assignment (greedy on dot(centroid - centre, slot diagonal)), ties by (candidate, slot) order; host twin: assignSlots8
  int  candOfSlot[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  bool slotUsed[8] = {false, false, false, false, false, false, false, false}, done[8] = {false, false, false, false, false, false, false, false};
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
        d[a] = __fsub_rn(__fmul_rn(0.5f, __fadd_rn(cands[c].lo[a], cands[c].hi[a])), __fmul_rn(0.5f, __fadd_rn(lo[a], hi[a])));
      for(int sl = 0; sl < 8; ++sl)
      {
        if(slotUsed[sl])
          continue;
        const float cost = __fadd_rn(__fadd_rn((sl & 1) ? d[0] : -d[0], (sl & 2) ? d[1] : -d[1]), (sl & 4) ? d[2] : -d[2]);
        if(cost > bestCost)
        {
          bestCost = cost;
          bc       = c;
          bs       = sl;
        }
      }
    }
    candOfSlot[bs] = bc;
    slotUsed[bs]   = true;
    done[bc]       = true;
  }
  Node8 N;
  memset(&N, 0, sizeof(N));
  {
    float    clo[3][8], chi[3][8];
    uint32_t used = 0;
    for(int sl = 0; sl < 8; ++sl)
    {
      const int c = candOfSlot[sl] < 0 ? 0 : candOfSlot[sl];
      for(int a = 0; a < 3; ++a) { clo[a][sl] = cands[c].lo[a]; chi[a][sl] = cands[c].hi[a]; }
      used |= candOfSlot[sl] < 0 ? 0u : 1u << sl;
    }
    quantiseNode8(N, lo, hi, clo, chi, used);  // (bvh_refit.h: the refit requantises with the same text)
  }
  // children: inner ones get consecutive node indices in slot order (they are the next level's items), leaf ones consecutive triangles
  const unsigned long long off = offsets[i];
  uint32_t                 childAt = nextLevelStart + uint32_t(off), triAt = triLevelBase + uint32_t(off >> 32);
  N.childBase = childAt;
  N.triBase   = triAt;
  for(int sl = 0; sl < 8; ++sl)
  {
    if(candOfSlot[sl] < 0)
      continue;
    const Cand8&   c  = cands[candOfSlot[sl]];
    const uint32_t tc = triCount2(nodes2, c.ref);
    if(d_isInner(nodes2, dp, c.ref, ml))
    {
      N.imask |= uint8_t(1u << sl);
      nextItems[childAt - nextLevelStart] = c.ref;
      ++childAt;
    }
    else
    {
      N.valid |= uint16_t((tc >= 2u ? 3u : 1u) << (2 * sl));  // (tc <= 2: d_isInner opens anything larger)
      // the (at most 4) triangles below c.ref, left to right; `slotBox`: the box each was filed under (its box in its BVH2 parent)
      int stack[8], from[8], sp = 0;
      stack[sp] = c.ref; from[sp++] = -1;
      while(sp > 0)
      {
        --sp;
        const int r = stack[sp], f = from[sp];
        if(r < 0)
        {
          if(slotBox)
          {
            RefitBox b;
            if(f < 0)
              for(int a = 0; a < 3; ++a) { b.lo[a] = c.lo[a]; b.hi[a] = c.hi[a]; }
            else
              childBox2(nodes2, f >> 1, f & 1, b.lo, b.hi);
            slotBox[triAt] = b;
          }
          perm[triAt++] = uint32_t(~r);
        }
        else
        {
          stack[sp] = childRef2(nodes2, r, 1); from[sp++] = 2 * r + 1;
          stack[sp] = childRef2(nodes2, r, 0); from[sp++] = 2 * r;
        }
      }
    }
  }
  nodes8[levelStart + uint32_t(i)] = N;
}

// A failed call leaves what it was for and the HIP error's text in `err`; the DevBuf locals of the collapse that returns on it free what was allocated.
bool hipOk(hipError_t e, const char* what, std::string& err)
{
  if(e != hipSuccess)
    err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipSuccess;
}

// ---- device collapse, one level at a time (see the header comment): fills `r` from a BVH2 with at least one inner node -------
bool collapseOnDevice(const BvhBuildOutput& b2, const Bvh8Options& opt, hipStream_t stream, std::string& err, Bvh8Output& r)
{
  auto check = [&](hipError_t e, const char* what) { return hipOk(e, what, err); };
  const uint32_t n = b2.numTris, numInner = b2.numNodes;
  DevBuf<Node8>              dNodes;
  DevBuf<int>                itemsA, itemsB;
  DevBuf<uint32_t>           dPerm;
  DevBuf<unsigned long long> counts, offsets, totals;
  DevBuf<uint8_t>            scanTemp;
  size_t                     scanBytes = 0;
  uint32_t                   trisPlaced = 0;
  DpTables                   dp{nullptr, nullptr};
  DevBuf<float>              dpCost;
  DevBuf<int8_t>             dpSplit;
  DevBuf<int>                dpParent, dpLeafParent;
  DevBuf<unsigned>           dpArrive;
  // every 8-wide node is rooted at a distinct BVH2 inner node: numInner bounds their number and the length of any level
  if(!check(dNodes.alloc(numInner), "alloc BVH8 nodes (worst case)")) return false;
  if(!check(itemsA.alloc(numInner), "alloc level items")) return false;
  if(!check(itemsB.alloc(numInner), "alloc level items")) return false;
  if(!check(dPerm.alloc(n), "alloc perm")) return false;
  if(opt.keepRefit)  // the refit data (bvh_refit.hip): the box each triangle slot was filed under
    if(!check(r.slotBox.alloc(n), "alloc refit slot boxes")) return false;
  if(!check(counts.alloc(numInner), "alloc counts")) return false;
  if(!check(offsets.alloc(numInner), "alloc offsets")) return false;
  if(!check(totals.alloc(1), "alloc totals")) return false;
  if(!check(hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, counts.ptr, offsets.ptr, int(numInner), stream), "scan size")) return false;
  if(!check(scanTemp.alloc(scanBytes), "alloc scan")) return false;
  const int root = b2.root;
  if(!check(hipMemcpyAsync(itemsA.ptr, &root, sizeof(int), hipMemcpyHostToDevice, stream), "seed level 0")) return false;
  uint32_t levelStart = 0, levelCount = 1;
  uint32_t   maxLeaf = BVH8_MAX_LEAF;
  // which BVH2 subtrees become the children of an 8-wide node (Bvh8Options; the images do not depend on it)
  const bool sahDp   = opt.sahCollapse;
  if(sahDp)
  {
    maxLeaf = std::min(maxLeaf, 3u);
    if(!check(dpCost.alloc(8 * size_t(numInner)), "alloc DP cost")) return false;
    if(!check(dpSplit.alloc(8 * size_t(numInner)), "alloc DP split")) return false;
    if(!check(dpParent.alloc(numInner), "alloc DP parents")) return false;
    if(!check(dpLeafParent.alloc(n), "alloc DP leaf parents")) return false;
    if(!check(dpArrive.alloc(numInner), "alloc DP tickets")) return false;
    if(!check(hipMemsetAsync(dpArrive.ptr, 0, sizeof(unsigned) * size_t(numInner), stream), "clear DP tickets")) return false;
    dp = DpTables{dpCost.ptr, dpSplit.ptr};
    hipLaunchKernelGGL(k_dp_parents, dim3((numInner + 255u) / 256u), dim3(256), 0, stream, int(numInner), b2.nodes.ptr, dpParent.ptr, dpLeafParent.ptr, root);
    hipLaunchKernelGGL(k_dp_solve, dim3((n + 255u) / 256u), dim3(256), 0, stream, int(n), b2.nodes.ptr, dpParent.ptr, dpLeafParent.ptr, dpArrive.ptr, dp, maxLeaf);
    if(!check(hipGetLastError(), "DP kernels")) return false;
  }
  while(levelCount > 0)
  {
    const unsigned g = (levelCount + 127u) / 128u;
    hipLaunchKernelGGL(k_collapse_count, dim3(g), dim3(128), 0, stream, int(levelCount), itemsA.ptr, b2.nodes.ptr, dp, maxLeaf, counts.ptr);
    if(!check(hipcub::DeviceScan::ExclusiveSum(scanTemp.ptr, scanBytes, counts.ptr, offsets.ptr, int(levelCount), stream), "scan")) return false;
    hipLaunchKernelGGL(k_collapse_emit, dim3(g), dim3(128), 0, stream, int(levelCount), itemsA.ptr, b2.nodes.ptr, dp, maxLeaf, counts.ptr, offsets.ptr, levelStart,
                       levelStart + levelCount, trisPlaced, dNodes.ptr, itemsB.ptr, dPerm.ptr, totals.ptr, r.slotBox.ptr);
    r.levels.push_back(levelStart);
    unsigned long long t = 0;
    if(!check(hipGetLastError(), "collapse kernels")) return false;
    if(!check(hipMemcpyAsync(&t, totals.ptr, sizeof(t), hipMemcpyDeviceToHost, stream), "read level totals")) return false;
    if(!check(hipStreamSynchronize(stream), "sync level")) return false;
    levelStart += levelCount;
    levelCount = uint32_t(t);
    trisPlaced += uint32_t(t >> 32);
    if(levelStart + levelCount > numInner || trisPlaced > n)
    {
      err = "BVH8 collapse overran its bounds";
      return false;
    }
    std::swap(itemsA, itemsB);
  }
  const uint32_t numNodes8 = levelStart;
  if(trisPlaced != n)
  {
    err = "BVH8 collapse lost triangles";
    return false;
  }
  if(!check(r.nodes.alloc(5 * size_t(numNodes8)), "alloc BVH8 nodes")) return false;
  if(!check(hipMemcpyAsync(r.nodes.ptr, dNodes.ptr, sizeof(Node8) * size_t(numNodes8), hipMemcpyDeviceToDevice, stream), "copy BVH8 nodes")) return false;
  r.levels.push_back(numNodes8);
  if(opt.keepRefit)  // (filled by the first pass of k_refit_level, which the caller runs over the new tree)
    if(!check(r.nodeBox.alloc(numNodes8), "alloc refit node boxes")) return false;
  if(!check(r.tris.alloc(n), "alloc BVH8 triangles")) return false;
  hipLaunchKernelGGL(k_reorder_tris, dim3((n + 255) / 256), dim3(256), 0, stream, n, dPerm.ptr, b2.tris.ptr, r.tris.ptr);
  if(!check(hipGetLastError(), "k_reorder_tris") || !check(hipStreamSynchronize(stream), "sync")) return false;
  r.numNodes  = numNodes8;
  r.numTris   = n;
  r.numLevels = uint32_t(r.levels.size()) - 1u;
  return true;
}

// ---- host collapse (A/B reference, and the one-triangle scene): download the BVH2, collapse it (bvh8_collapse_host.h), upload ----
bool collapseOnHost(const BvhBuildOutput& b2, hipStream_t stream, std::string& err, Bvh8Output& r)
{
  auto check = [&](hipError_t e, const char* what) { return hipOk(e, what, err); };
  const uint32_t      n = b2.numTris, numInner = b2.numNodes;
  std::vector<float4> nodes2(size_t(numInner) * 4);
  if(numInner && !check(hipMemcpy(nodes2.data(), b2.nodes.ptr, nodes2.size() * sizeof(float4), hipMemcpyDeviceToHost), "download BVH2"))
    return false;
  float loneLo[3] = {0.0f, 0.0f, 0.0f}, loneHi[3] = {0.0f, 0.0f, 0.0f};
  if(numInner == 0)  // single triangle: need its bounds
  {
    DevTri T;
    if(!check(hipMemcpy(&T, b2.tris.ptr, sizeof(DevTri), hipMemcpyDeviceToHost), "download triangles")) return false;
    const float v[3][3] = {{T.a.x, T.a.y, T.a.z}, {T.a.x + T.b.x, T.a.y + T.b.y, T.a.z + T.b.z}, {T.a.x + T.c.x, T.a.y + T.c.y, T.a.z + T.c.z}};
    for(int a = 0; a < 3; ++a)
    {
      // one ulp of slack each way: the BVH2 path bounds the true vertices too (k_tri_setup)
      loneLo[a] = std::nextafter(std::min(v[0][a], std::min(v[1][a], v[2][a])), -FLT_MAX);
      loneHi[a] = std::nextafter(std::max(v[0][a], std::max(v[1][a], v[2][a])), FLT_MAX);
    }
  }
  const Bvh8OnHost h = collapseBvh8OnHost(nodes2.data(), b2.root, numInner, n, loneLo, loneHi);
  if(h.perm.size() != n)
  {
    err = "BVH8 collapse lost triangles";
    return false;
  }
  DevBuf<uint32_t> dPerm;
  if(!check(r.nodes.alloc(5 * h.nodes.size()), "alloc BVH8 nodes")) return false;
  if(!check(hipMemcpy(r.nodes.ptr, h.nodes.data(), h.nodes.size() * sizeof(Node8), hipMemcpyHostToDevice), "upload BVH8 nodes")) return false;
  if(!check(r.tris.alloc(n), "alloc BVH8 triangles")) return false;
  if(!check(dPerm.alloc(n), "alloc perm")) return false;
  if(!check(hipMemcpy(dPerm.ptr, h.perm.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice), "upload perm")) return false;
  hipLaunchKernelGGL(k_reorder_tris, dim3((n + 255) / 256), dim3(256), 0, stream, n, dPerm.ptr, b2.tris.ptr, r.tris.ptr);
  if(!check(hipGetLastError(), "k_reorder_tris") || !check(hipStreamSynchronize(stream), "sync")) return false;
  r.numNodes  = uint32_t(h.nodes.size());
  r.numTris   = n;
  r.numLevels = h.numLevels;
  return true;
}

}  // namespace

bool buildBvh8(const BvhBuildOutput& b2, Bvh8Output& out, hipStream_t stream, std::string& err, const Bvh8Options& opt)
{
  out = Bvh8Output();
  if(b2.numTris == 0)
    return true;
  Bvh8Output r;  // becomes `out` once the collapse has succeeded: a failure leaves `out` empty
  const bool onDevice = b2.numNodes > 0 && !opt.hostCollapse;  // (a one-triangle tree has no BVH2 node to seed the first level with)
  if(!(onDevice ? collapseOnDevice(b2, opt, stream, err, r) : collapseOnHost(b2, stream, err, r)))
    return false;
  out = std::move(r);
  return true;
}

}  // namespace pt
