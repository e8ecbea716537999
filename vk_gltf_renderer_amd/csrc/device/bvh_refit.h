// The per-thread work of the in-place refit of the 8-wide BVH (bvh_refit.hip) and what it shares with the builder: the world-space
// triangle record of k_tri_setup (bvh_build.hip) and the child-box quantisation of k_collapse_emit (bvh8.hip).  One text for both, so a
// refitted triangle record or node is, byte for byte, what a build writes from the same inputs.  Compiles for the host as well
// (tests/host_shim/refit_on_host.cpp).
#pragma once
#include <cfloat>
#include <cmath>

#include "pt_scene.h"

namespace pt {

struct Node8  // 80 bytes, layout: bvh8.hip
{
  float    p[3];
  uint8_t  e[3];
  uint8_t  imask;
  uint32_t childBase;
  uint32_t triBase;
  uint16_t valid;      // two bits per slot: triangles of its leaf child (see bvh8.hip)
  uint16_t reserved16;
  uint32_t reserved32;
  uint8_t  qlo[3][8];
  uint8_t  qhi[3][8];
};
static_assert(sizeof(Node8) == 80, "Node8 must be 80 bytes");

#ifndef MI_PT_DP_C_TRI
#define MI_PT_DP_C_TRI (56.0f / 235.0f)  // a triangle test against a node visit, in vector instructions (round 3's counts; see LABNOTES.md section 3 for the round-4 sweep)
#endif

#if defined(__HIP_DEVICE_COMPILE__)  // (the streams of a primitive are global memory: saying so gives global_load, not flat)
#define PT_GLOBAL_AS __attribute__((address_space(1)))
#else
#define PT_GLOBAL_AS
#endif

struct RefitBox  // 24 B
{
  float lo[3], hi[3];
};

// The flag word of triangle t's record (DevTri::c.w): its render node's instance flags, and FORCE_OPAQUE for a triangle the load-time
// classification found opaque (DevPrim::opaqueTriangles), which counts like a triangle of an opaque instance.  One text for the build, the
// refit and the material patch (material_patch.h).
PT_DEV uint32_t triangleFlagWord(const DevPrim& rp, uint32_t t, uint32_t instFlags)
{
  return instFlags | (t < rp.opaqueTriangles ? uint32_t(INST_FORCE_OPAQUE) : 0u);
}

// Triangle t of render node `rnode` in world space (fixed fmaf order, shared with the oracle) and the box it is filed under: what
// k_tri_setup writes for it, and what k_refit_tris rewrites.
PT_DEV void worldTriangle(const MiGltfRenderNode& rn, const DevPrim& rp, int rnode, uint32_t t, uint32_t instFlags, DevTri& tri, float lo[3], float hi[3])
{
  const PT_GLOBAL_AS uint32_t* idx = (const PT_GLOBAL_AS uint32_t*)rp.indices;
  const PT_GLOBAL_AS float*    pos = (const PT_GLOBAL_AS float*)rp.positions;
  const uint32_t               i0 = idx[3 * t], i1 = idx[3 * t + 1], i2 = idx[3 * t + 2];
  f3 p0 = mulPoint(rn.objectToWorld, mk3(pos[3 * size_t(i0)], pos[3 * size_t(i0) + 1], pos[3 * size_t(i0) + 2]));
  f3 p1 = mulPoint(rn.objectToWorld, mk3(pos[3 * size_t(i1)], pos[3 * size_t(i1) + 1], pos[3 * size_t(i1) + 2]));
  f3 p2 = mulPoint(rn.objectToWorld, mk3(pos[3 * size_t(i2)], pos[3 * size_t(i2) + 1], pos[3 * size_t(i2) + 2]));
  // Vertex buffers and instance matrices are untrusted bytes.  A triangle with a NaN, an infinity or a coordinate whose square
  // overflows would poison the scene bounds, the Morton keys and the surface areas the clustering compares; it becomes a point at
  // the origin instead -- zero area, so no ray hits it -- and the rest of the scene builds and renders as if it were not there.
  {
    const float big = 1.0e18f;
    const bool  ok  = fabsf(p0.x) < big && fabsf(p0.y) < big && fabsf(p0.z) < big && fabsf(p1.x) < big && fabsf(p1.y) < big && fabsf(p1.z) < big
                    && fabsf(p2.x) < big && fabsf(p2.y) < big && fabsf(p2.z) < big;  // false for NaN as well
    if(!ok)
      p0 = p1 = p2 = mk3(0.0f);
  }
  f3 e1 = p1 - p0, e2 = p2 - p0;
  tri.a = make_float4(p0.x, p0.y, p0.z, __int_as_float(rnode));
  tri.b = make_float4(e1.x, e1.y, e1.z, __int_as_float(int(t)));
  tri.c = make_float4(e2.x, e2.y, e2.z, __uint_as_float(triangleFlagWord(rp, t, instFlags)));
  // bounds from the same p0 + e arithmetic the intersector sees
  f3 q1 = p0 + e1, q2 = p0 + e2;
  lo[0] = fminf(p0.x, fminf(q1.x, q2.x)); hi[0] = fmaxf(p0.x, fmaxf(q1.x, q2.x));
  lo[1] = fminf(p0.y, fminf(q1.y, q2.y)); hi[1] = fmaxf(p0.y, fmaxf(q1.y, q2.y));
  lo[2] = fminf(p0.z, fminf(q1.z, q2.z)); hi[2] = fmaxf(p0.z, fmaxf(q1.z, q2.z));
  // include the true vertices too (p0+e may round inward)
  lo[0] = fminf(lo[0], fminf(p1.x, p2.x)); hi[0] = fmaxf(hi[0], fmaxf(p1.x, p2.x));
  lo[1] = fminf(lo[1], fminf(p1.y, p2.y)); hi[1] = fmaxf(hi[1], fmaxf(p1.y, p2.y));
  lo[2] = fminf(lo[2], fminf(p1.z, p2.z)); hi[2] = fmaxf(hi[2], fmaxf(p1.z, p2.z));
}

// What the host collapse (bvh8_collapse_host.h) runs as well is callable from the host pass of hipcc, where __fmaf_rn has no definition.
#define PT_HOST_DEV __host__ PT_DEV
PT_HOST_DEV float fmaOnce(float a, float b, float c)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmaf_rn(a, b, c);
#else
  return std::fmaf(a, b, c);
#endif
}

// Quantisation of one axis of an 8-wide node: frame from p = lo, children = the boxes [clo, chi] of the slots set in `used`.  An exponent
// grows until every child's decoded box fmaf(q, 2^e, p) contains its true box; empty slots hold an inverted box.  Returns e + 127.
PT_HOST_DEV uint8_t quantiseAxis8(float p, float lo, float hi, const float (&clo)[8], const float (&chi)[8], uint32_t used, uint8_t (&qlo)[8], uint8_t (&qhi)[8])
{
  const float ext = hi - lo;
  int         ex  = ext > 0.0f ? int(ceil(log2(double(ext) / 255.0))) : -126;
  ex              = max(-126, min(ex, 126));
  for(int sl = 0; sl < 8; ++sl)
  {
    qlo[sl] = 255;  // empty slot: inverted box (and no valid bit)
    qhi[sl] = 0;
  }
  for(;;)
  {
    const float scale = ldexpf(1.0f, ex);
    bool        fits  = true;
    for(int sl = 0; sl < 8 && fits; ++sl)
    {
      if(!((used >> sl) & 1u))
        continue;
      const double ql = floor((double(clo[sl]) - double(p)) / double(scale));
      const double qh = ceil((double(chi[sl]) - double(p)) / double(scale));
      int          il = int(fmax(0.0, fmin(255.0, ql))), ih = int(fmax(0.0, fmin(255.0, qh)));
      while(il > 0 && fmaOnce(float(il), scale, p) > clo[sl])
        --il;
      while(ih < 255 && fmaOnce(float(ih), scale, p) < chi[sl])
        ++ih;
      if(fmaOnce(float(il), scale, p) > clo[sl] || fmaOnce(float(ih), scale, p) < chi[sl])
        fits = false;
      qlo[sl] = uint8_t(il);
      qhi[sl] = uint8_t(ih);
    }
    if(fits || ex >= 126)
      break;
    ++ex;
  }
  return uint8_t(ex + 127);
}
// ... of the whole node: frame [lo, hi] (the union of its children), clo / chi per axis and slot.  Sets p, e, qlo and qhi.
// k_collapse_emit, the host collapse and k_refit_level all call this, so equal boxes give equal bytes.
PT_HOST_DEV void quantiseNode8(Node8& N, const float lo[3], const float hi[3], const float (&clo)[3][8], const float (&chi)[3][8], uint32_t used)
{
  for(int a = 0; a < 3; ++a)
  {
    N.p[a] = lo[a];
    N.e[a] = quantiseAxis8(lo[a], lo[a], hi[a], clo[a], chi[a], used, N.qlo[a], N.qhi[a]);
  }
}

PT_DEV float refitBoxArea(const float lo[3], const float hi[3])
{
  const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  return __fmaf_rn(ez, ex, __fmaf_rn(ey, ez, ex * ey));
}
// An EMPTY box -- nothing visible below it (resident mode: the slots of hidden render nodes) -- is the neutral element of the union,
// lo = FLT_MAX, hi = -FLT_MAX: fminf / fmaxf pass the other operand through, so a union needs no test for it.  What must not see
// +-FLT_MAX is the arithmetic: an empty box has area 0 and no place in a node's frame.
PT_DEV bool refitBoxEmpty(const float lo[3], const float hi[3])
{
  return lo[0] > hi[0];
}
PT_DEV float refitBoxAreaOrZero(const float lo[3], const float hi[3])
{
  return refitBoxEmpty(lo, hi) ? 0.0f : refitBoxArea(lo, hi);
}

// What a triangle slot's render node did since the last update (the dirty byte table of k_refit_tris)
enum : uint8_t
{
  REFIT_CLEAN = 0,  // unchanged: the slot keeps its record and box
  REFIT_MOVED = 1,  // moved or deformed: record and box from the current pose; a pre-split reference gets its whole triangle's box
  REFIT_HOME  = 2,  // changed, and back at the matrices of the last build with a primitive not deformed since: record from the current
                    // pose, box = the one the build filed (a deformed primitive is never HOME until the next build: its vertices are not compared)
  REFIT_HIDDEN = 3,  // became invisible (resident mode): a degenerate record -- a point at the origin, like a non-finite triangle -- that keeps
                     // its render node, triangle index and flag word, and an empty box.  A node that STAYS hidden is CLEAN; one that comes
                     // back is HOME or MOVED
};

// k_refit_tris, one triangle slot `s`: rewrites the record and the slot box of a slot whose render node is not clean.  The record's
// render node and triangle index (DevTri a.w, b.w) never change.  `builtBox`: the boxes the build filed the references under.
PT_DEV void refitTriSlot(const MiGltfRenderNode* nodes, const DevPrim* prims, const uint8_t* instFlags, const uint8_t* dirty, const RefitBox* builtBox,
                         DevTri* tris, RefitBox* slotBox, uint32_t s)
{
  const float4   a     = tris[s].a;
  const int      rnode = __float_as_int(a.w);
  const uint8_t  state = dirty[rnode];
  if(state == REFIT_CLEAN)
    return;
  if(state == REFIT_HIDDEN)
  {
    tris[s].a = make_float4(0.0f, 0.0f, 0.0f, a.w);
    tris[s].b = make_float4(0.0f, 0.0f, 0.0f, tris[s].b.w);
    tris[s].c = make_float4(0.0f, 0.0f, 0.0f, tris[s].c.w);
    RefitBox empty;
    for(int k = 0; k < 3; ++k) { empty.lo[k] = FLT_MAX; empty.hi[k] = -FLT_MAX; }
    slotBox[s] = empty;
    return;
  }
  const uint32_t          t  = uint32_t(__float_as_int(tris[s].b.w));
  const MiGltfRenderNode& rn = nodes[rnode];
  const DevPrim&          rp = prims[rn.renderPrimID];
  DevTri                  tri;
  RefitBox                box;
  worldTriangle(rn, rp, rnode, t, uint32_t(instFlags[rnode]), tri, box.lo, box.hi);
  tris[s] = tri;
  if(state == REFIT_HOME)
    slotBox[s] = builtBox[s];
  else
    slotBox[s] = box;
}

// k_refit_level, one node: takes the union of each child's boxes -- leaf children from the slot boxes at triBase, inner children from the
// node boxes at childBase --, requantises the node (slot assignment, childBase, triBase, valid and imask stay) and returns its box in `own`
// and its SAH term: area(node) + C_TRI x the summed area x triangles of its leaf children.
// Emptiness (refitBoxEmpty): an empty slot box drops out of its leaf child's union by itself; a child whose box is empty -- every triangle
// of a leaf child hidden, or an inner child with nothing visible below it -- is left out of `used` and so gets the inverted bytes 255 / 0 of
// an empty slot, which every walk's slab test misses, while valid, imask, childBase and triBase stay (the tree keeps its topology); it adds
// 0 to the SAH term.  A node with no child left reports an empty box upwards and keeps its p: the walks compute (p - org) * idir from it,
// so p is never +-FLT_MAX or non-finite.
PT_DEV float refitNode8(Node8& N, const RefitBox* slotBox, const RefitBox* nodeBox, RefitBox& own)
{
  float    clo[3][8], chi[3][8], lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX}, leafTerm = 0.0f;
  uint32_t used = 0, child = N.childBase, tri = N.triBase;
#pragma unroll
  for(int sl = 0; sl < 8; ++sl)
  {
    const uint32_t v = (uint32_t(N.valid) >> (2 * sl)) & 3u;
    const bool     inner = (N.imask >> sl) & 1u;
    RefitBox       b;
    if(inner)
      b = nodeBox[child++];
    else if(v)
    {
      const uint32_t count = (v & 2u) ? 2u : 1u;
      b                    = slotBox[tri];
      if(count == 2u)
      {
        const RefitBox c = slotBox[tri + 1];
        for(int a = 0; a < 3; ++a) { b.lo[a] = fminf(b.lo[a], c.lo[a]); b.hi[a] = fmaxf(b.hi[a], c.hi[a]); }
      }
      tri += count;
      leafTerm = __fmaf_rn(refitBoxAreaOrZero(b.lo, b.hi), float(count), leafTerm);
    }
    else
      for(int a = 0; a < 3; ++a) { b.lo[a] = 0.0f; b.hi[a] = 0.0f; }
    for(int a = 0; a < 3; ++a) { clo[a][sl] = b.lo[a]; chi[a][sl] = b.hi[a]; }
    if((inner || v) && !refitBoxEmpty(b.lo, b.hi))
    {
      used |= 1u << sl;
      for(int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], b.lo[a]); hi[a] = fmaxf(hi[a], b.hi[a]); }
    }
  }
  if(used)
    quantiseNode8(N, lo, hi, clo, chi, used);
  else
  {
    const float keep[3] = {N.p[0], N.p[1], N.p[2]};  // (a frame of no extent at the previous origin: every slot inverted)
    quantiseNode8(N, keep, keep, clo, chi, 0u);
  }
  for(int a = 0; a < 3; ++a) { own.lo[a] = lo[a]; own.hi[a] = hi[a]; }
  return __fmaf_rn(float(MI_PT_DP_C_TRI), leafTerm, refitBoxAreaOrZero(lo, hi));
}

}  // namespace pt
