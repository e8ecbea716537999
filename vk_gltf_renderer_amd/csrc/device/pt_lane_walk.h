// The per-lane walk: one ray per lane over either tree, every lane on its own -- no wave-wide triangle rounds, no LDS node cache, no barrier, so
// a partially filled wave needs no care.  The stack setup and the two tree loops, nothing else: what a candidate is and what the walk culls with
// are the caller's.  k_selection (pt_kernels.hip) and the query kernels (query.hip) are its callers; the wave-cooperative walks of k_trace_* are not.
#pragma once
#include "pt_bvh8.h"

namespace pt {

// WIDE: the 8-wide tree (bvh8Visit), else the BVH2 (bvhWalk).  ANY: the first accepted triangle ends the walk.  BLOCK: the block size, which strides
// the block's LDS stack `stack` (BVH_STACK_LDS * BLOCK ints, [depth][lane]: this lane touches its own column only).
// test(triIndex) -> accepted: the candidate test of one triangle slot.  bound() -> the t the node tests cull with from now on, asked after every
// accepted triangle; walkT until the first one.  Finite: the slab arithmetic forms differences with it.  A triangle AT that distance is still
// visited -- the boxes are padded -- so that a tie rule sees it.  The caller checks sc.bvhRoot != BVH_EMPTY.
// The two callables are taken by value on purpose: taken by reference, the K = 8 list kernel of query.hip spilled 214 scalar registers instead of 164
// and walked 255 instead of 330 Mrays/s (LABNOTES.md, "One per-lane walk for the query calls and the selection pass").
template <bool WIDE, bool ANY, int BLOCK, typename Test, typename Bound>
PT_DEV void laneWalk(const DevScene& sc, const RaySetup& r, float walkT, int* stack, Test test, Bound bound)
{
  if(WIDE)
  {
    LaneStack2 st2;
    uint32_t   stackOverflow[2 * BVH8_STACK_PRIV];
    st2.lds = stack; st2.tid = int(threadIdx.x); st2.stride = BLOCK; st2.sp = 0;
    st2.privBase = stackOverflow; st2.privBits = stackOverflow + BVH8_STACK_PRIV;
    const uint32_t octinv = rayOctInv(r.idir);
    NodeGroup      G      = rootGroup(octinv);
    bool           done   = false;
    while(!done)
    {
      if((G.bits >> 8) == 0u)
      {
        if(st2.sp == 0)
          break;
        G = st2.pop();
      }
      const uint32_t child = groupPopChild(G, octinv);
      if(G.bits >> 8)
        st2.push(G);
      uint32_t tBase, tMask;
      bvh8Visit(sc, r, walkT, octinv, child, G, tBase, tMask, nullptr, 0u);
      while(leafPending(tMask))
      {
        const int k = int(leafPop(tMask, 0u));  // (offset from the node's first triangle)
        if(test(int(tBase) + k))
        {
          walkT = bound();
          if(ANY)
          {
            done = true;
            break;
          }
        }
      }
    }
  }
  else
  {
    LaneStack st;
    int       stackOverflow[BVH_STACK_PRIV];
    st.lds = stack; st.tid = int(threadIdx.x); st.stride = BLOCK; st.sp = 0; st.priv = stackOverflow;
    // (a scene of one triangle has no node: bvhRoot = ~0, which bvhWalk visits as a leaf)
    bvhWalk(sc, r, walkT, st, [&](int triIndex, float tmax) -> float {
      if(test(triIndex))
        return ANY ? -1.0f : bound();
      return tmax;
    });
  }
}

}  // namespace pt
