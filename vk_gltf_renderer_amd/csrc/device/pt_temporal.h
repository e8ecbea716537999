// Temporal half of the SVGF denoiser (Schied et al. 2017, §4.1), fed by the reference's motion-vector definition: the per-pixel arithmetic
// of k_motion_vectors and k_svgf_reproject (temporal.hip) and the helpers they share with the spatial pass (denoise.hip).  Plain functions
// over pointers, so that tests/host_shim compiles them for the host and the CPU tier diffs them against a float64 restatement.
//   first-hit record (PathSoA::firstHit, one per pixel of a first-frame batch): xyz = world position of the first hit, or the ray direction
//   where w holds id 0; w = the BITS of an id: renderNode + 1 (mesh), 0 (miss and infinite plane), 0xffffffff (shadow-catcher path: no position).
//   motion record: xy = (prevNDC - currNDC) * 0.5 * resolution in pixels (the reference's calculateMotionVector, dlss_util.h:63-96: surfaces
//   are points (w = 1) carried by their node's previous objectToWorld, gltf_pathtrace.slang:228-241; id 0 are points at infinity (w = 0), so
//   that a camera translation cancels); z = the NDC depth the point had under prevMVP (1 for id 0); w = the id bits.
//   With vertex motion on (motionRecordDeformed, below) a hit on skinned or morphed geometry is carried by its triangle's previous-pose vertices.
#pragma once
#include "mi_pt_shaderio.h"
#include "pt_math.h"
#include "pt_scene.h"

namespace pt {

constexpr uint32_t TEMPORAL_ID_INVALID = 0xffffffffu;

// thresholds and blend factors of the reprojection (MiPtTemporalParams, include/mi_pt.h)
struct TemporalConsts
{
  float alpha, momentsAlpha, maxHistory, normalCos, depthTolerance;
};

// History of one pixel: three 16-byte records.
//   illum:   blended, unfiltered, demodulated illumination rgb; history length h
//   moments: first and second moment of its luminance; NDC depth of the pixel; id bits
//   normal:  first-hit shading normal xyz; 0
struct TemporalHistory
{
  float4* illum;
  float4* moments;
  float4* normal;
};

PT_DEV float lum709(float x, float y, float z)
{
  return 0.2126f * x + 0.7152f * y + 0.0722f * z;
}

PT_DEV f3 demodulator(const float4 a)
{
  return a.w > 0.5f ? mk3(fmaxf(a.x, 0.02f), fmaxf(a.y, 0.02f), fmaxf(a.z, 0.02f)) : mk3(1.0f, 1.0f, 1.0f);
}

// view-depth-like quantity from the stored NDC depth: proportional to the distance for a perspective projection with a far plane
// much further than the scene (1 - z ~ near / distance), monotonic for any other; only ratios of its differences are used
PT_DEV float depthKey(float ndc)
{
  return 1.0f / fmaxf(1.0f - ndc, 1e-7f);
}

// Variance of the demodulated luminance over the 7x7 neighbourhood of the same kind (geometry / background) with a similar normal: the
// spatial estimate that stands in for the temporal one while a pixel has fewer than 4 frames behind it (paper §4.2)
PT_DEV float spatialVariance7x7(const float4* __restrict__ color, const float4* __restrict__ albedo, const float4* __restrict__ normal, int W, int H, int x,
                                int y, const float4 ca, const float4 cn)
{
  float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
  for(int dy = -3; dy <= 3; ++dy)
    for(int dx = -3; dx <= 3; ++dx)
    {
      const int qx = x + dx, qy = y + dy;
      if(qx < 0 || qy < 0 || qx >= W || qy >= H)
        continue;
      const size_t q  = size_t(qy) * W + qx;
      const float4 qa = albedo[q];
      if((qa.w > 0.5f) != (ca.w > 0.5f))
        continue;
      const float4 qn = normal[q], qc = color[q];
      const float  w  = ca.w > 0.5f ? (fmaxf(0.0f, qn.x * cn.x + qn.y * cn.y + qn.z * cn.z) > 0.9f ? 1.0f : 0.0f) : 1.0f;
      const f3     qd = demodulator(qa);
      const float  l  = lum709(qc.x / qd.x, qc.y / qd.y, qc.z / qd.z);
      s1 += w * l;
      s2 += w * l * l;
      sw += w;
    }
  const float m = sw > 0.0f ? s1 / sw : 0.0f;
  return sw > 0.0f ? fmaxf(0.0f, s2 / sw - m * m) : 0.0f;
}

// pixel of a pixel slot (tile-major, 8x8 micro-tiles inside a tile; ownedTiles[i] = x0 | y0 << 16): what slotToPixel of pt_kernels.hip
// computes from the batch's FrameConsts, restated over plain arguments for the per-pixel records read after the batch (on the device by
// k_motion_vectors, on the host by mi_pt_read_first_hit)
__host__ PT_DEV bool pixelOfSlot(const uint32_t* ownedTiles, int tileShift, int width, int height, uint32_t slot, int& px, int& py)
{
  const uint32_t tile   = ownedTiles[slot >> (2 * tileShift)];
  const uint32_t w      = slot & ((1u << (2 * tileShift)) - 1u);
  const uint32_t micro  = w >> 6, lane = w & 63u;
  const uint32_t mshift = uint32_t(tileShift) - 3u;
  px                    = int((tile & 0xffffu) + (micro & ((1u << mshift) - 1u)) * 8u + (lane & 7u));
  py                    = int((tile >> 16) + (micro >> mshift) * 8u + (lane >> 3));
  return px < width && py < height;
}

// column-major M times (x, y, z, w) as explicit fused chains: the current and the previous projection of a point round the same way
// whatever the compiler contracts, so equal matrices and equal points give equal clip coordinates, bit for bit
PT_DEV f4 mulChain(const float* M, float x, float y, float z, float w)
{
  f4 r;
  r.x = __builtin_fmaf(M[12], w, __builtin_fmaf(M[8], z, __builtin_fmaf(M[4], y, M[0] * x)));
  r.y = __builtin_fmaf(M[13], w, __builtin_fmaf(M[9], z, __builtin_fmaf(M[5], y, M[1] * x)));
  r.z = __builtin_fmaf(M[14], w, __builtin_fmaf(M[10], z, __builtin_fmaf(M[6], y, M[2] * x)));
  r.w = __builtin_fmaf(M[15], w, __builtin_fmaf(M[11], z, __builtin_fmaf(M[7], y, M[3] * x)));
  return r;
}

// Projects the current point (the first-hit record's xyz) and the point `pp` it was in the previous pose; w = 1 for a surface point, 0 for a direction.
PT_DEV float4 motionOfPoints(const float4 fh, const f3 pp, uint32_t id, const float* viewProj, const float* prevMVP, float width, float height)
{
  const float w   = id != 0u ? 1.0f : 0.0f;
  const f4    cur = mulChain(viewProj, fh.x, fh.y, fh.z, w), prv = mulChain(prevMVP, pp.x, pp.y, pp.z, w);
  const float cx = divExact(cur.x, cur.w), cy = divExact(cur.y, cur.w), qx = divExact(prv.x, prv.w), qy = divExact(prv.y, prv.w);
  return make_float4((qx - cx) * 0.5f * width, (qy - cy) * 0.5f * height, id != 0u ? divExact(prv.z, prv.w) : 1.0f, fh.w);
}

// The motion record of a first-hit record.  prevObjectToWorld: 16 floats per render node, the matrices of the pose rendered before.
PT_DEV float4 motionRecord(const float4 fh, const MiGltfRenderNode* __restrict__ nodes, const float* __restrict__ prevObjectToWorld, int numNodes,
                           const float* viewProj, const float* prevMVP, float width, float height)
{
  const uint32_t id = __float_as_uint(fh.w);
  if(id == TEMPORAL_ID_INVALID || id > uint32_t(numNodes))
    return make_float4(0.0f, 0.0f, 1.0f, __uint_as_float(TEMPORAL_ID_INVALID));
  f3 pp = mk3(fh.x, fh.y, fh.z);  // where the point was in the previous pose
  if(id != 0u)
  {
    const MiGltfRenderNode& rn   = nodes[id - 1u];
    const float*            prev = prevObjectToWorld + size_t(id - 1u) * 16u;
    bool                    moved = false;
    for(int i = 0; i < 16; ++i)
      moved = moved || rn.objectToWorld[i] != prev[i];
    if(moved)  // (a node that stands still keeps the hit position itself: no round trip through object space, no rounding, zero motion)
    {
      const f4 obj = mulChain(rn.worldToObject, fh.x, fh.y, fh.z, 1.0f);
      pp           = xyz(mulChain(prev, obj.x, obj.y, obj.z, 1.0f));
    }
  }
  return motionOfPoints(fh, pp, id, viewProj, prevMVP, width, height);
}

// ---- vertex motion (mi_pt_set_vertex_motion): skinned and morphed vertices carried in the motion record -------------------------------
// first-hit triangle record (PathSoA::firstHitTri, next to the first-hit record): x = render primitive, y = triangle index inside it (the whole
// source triangle, also where the tree holds pre-split references), z, w = the BITS of the barycentrics b1, b2 the shade interpolates the
// attributes with (b0 = 1 - b1 - b2).  Written for mesh hits only: it means something where the first-hit id names a render node.

// What the motion kernel needs of a render primitive, indexed by render primitive.  prevPositions: the object-space positions of the pose
// rendered before (3 floats per vertex), NULL for a primitive that does not deform.
struct VertexMotionPrim
{
  const float*    prevPositions;
  const float*    positions;  // the resident stream (DevPrim::positions): the pose being rendered
  const uint32_t* indices;    // DevPrim::indices
  uint32_t        numTriangles, vertexCount;
};

// The motion record of a first hit on deforming geometry: the material point's previous position is the barycentric interpolation of its
// triangle's previous-pose vertices, carried by the node's previous objectToWorld.  A triangle whose nine previous floats equal its nine
// current ones bit for bit (a still character, the first pose, an update with unchanged tables) takes motionRecord's path -- and so does a
// record that names no deforming primitive -- so that zero motion stays exactly zero.
PT_DEV float4 motionRecordDeformed(const float4 fh, const uint4 tri, const VertexMotionPrim* __restrict__ prims, int numPrims,
                                   const MiGltfRenderNode* __restrict__ nodes, const float* __restrict__ prevObjectToWorld, int numNodes,
                                   const float* viewProj, const float* prevMVP, float width, float height)
{
  const uint32_t id = __float_as_uint(fh.w);
  if(id != 0u && id != TEMPORAL_ID_INVALID && id <= uint32_t(numNodes) && tri.x < uint32_t(numPrims))
  {
    const VertexMotionPrim& vp = prims[tri.x];
    if(vp.prevPositions && tri.y < vp.numTriangles)
    {
      // (the record's pointers are generic to the compiler; gat() reads them as the global memory they are, pt_scene.h)
      const uint32_t* ix = &gat(vp.indices, 3u * size_t(tri.y));
      const uint32_t  i0 = ix[0], i1 = ix[1], i2 = ix[2];
      if(i0 < vp.vertexCount && i1 < vp.vertexCount && i2 < vp.vertexCount)
      {
        const float *p0 = &gat(vp.prevPositions, 3u * size_t(i0)), *p1 = &gat(vp.prevPositions, 3u * size_t(i1)), *p2 = &gat(vp.prevPositions, 3u * size_t(i2));
        const float *c0 = &gat(vp.positions, 3u * size_t(i0)), *c1 = &gat(vp.positions, 3u * size_t(i1)), *c2 = &gat(vp.positions, 3u * size_t(i2));
        bool         deformed = false;
        for(int k = 0; k < 3; ++k)
          deformed = deformed || __float_as_uint(p0[k]) != __float_as_uint(c0[k]) || __float_as_uint(p1[k]) != __float_as_uint(c1[k])
                     || __float_as_uint(p2[k]) != __float_as_uint(c2[k]);
        if(deformed)
        {
          const float b1 = __uint_as_float(tri.z), b2 = __uint_as_float(tri.w), b0 = 1.0f - b1 - b2;
          const float ox = __builtin_fmaf(b2, p2[0], __builtin_fmaf(b1, p1[0], b0 * p0[0]));
          const float oy = __builtin_fmaf(b2, p2[1], __builtin_fmaf(b1, p1[1], b0 * p0[1]));
          const float oz = __builtin_fmaf(b2, p2[2], __builtin_fmaf(b1, p1[2], b0 * p0[2]));
          const f3    pp = xyz(mulChain(prevObjectToWorld + size_t(id - 1u) * 16u, ox, oy, oz, 1.0f));
          return motionOfPoints(fh, pp, id, viewProj, prevMVP, width, height);
        }
      }
    }
  }
  return motionRecord(fh, nodes, prevObjectToWorld, numNodes, viewProj, prevMVP, width, height);
}

// One pixel of the temporal stage: reprojects the history along the motion record, blends this pose's demodulated colour and luminance
// moments into it, writes the new history and returns (illumination rgb, variance) for the a-trous iterations.
//   1. previous position = pixel centre + motion; its four bilinear taps of the history
//   2. a tap is valid inside the image, with this pixel's id, an agreeing normal (dot >= normalCos; id 0 has none) and a stored depth that
//      agrees with the depth the point had (motion.z), relative, in depthKey
//   3. weights renormalised over the valid taps; none (or an invalid id, or no history): h = 1, alpha = 1
//   4. h = min(h_interpolated + 1, maxHistory), alpha = max(alpha, 1 / h)
//   5. variance = max(0, mu2 - mu1^2) from h >= 4, the 7x7 spatial estimate below
// validTaps (optional, for the tests): number of valid taps, 0 = reset.
PT_DEV float4 reprojectPixel(int x, int y, int W, int H, const TemporalConsts& tc, bool haveHistory, const float4* __restrict__ color,
                             const float4* __restrict__ albedo, const float4* __restrict__ normal, const float* __restrict__ depth,
                             const float4* __restrict__ motion, const TemporalHistory& in, const TemporalHistory& out, int* validTaps)
{
  const size_t   c  = size_t(y) * W + x;
  const float4   cc = color[c], ca = albedo[c], cn = normal[c], mv = motion[c];
  const uint32_t id = __float_as_uint(mv.w);
  const f3       dm = demodulator(ca);
  const f3       il = mk3(cc.x / dm.x, cc.y / dm.y, cc.z / dm.z);
  const float    l1 = lum709(il.x, il.y, il.z), l2 = l1 * l1;

  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sh = 0.0f, s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
  int   taps = 0;
  if(haveHistory && id != TEMPORAL_ID_INVALID)
  {
    const float fx = float(x) + mv.x, fy = float(y) + mv.y;  // (pixel centre + motion) - 0.5: in units of history texels
    const float bx = floorf(fx), by = floorf(fy);
    const float tx = fx - bx, ty = fy - by;
    const float kp = depthKey(mv.z);
    // (a motion far outside the image has no tap; the clamp keeps the conversion defined)
    const int x0 = int(fminf(fmaxf(bx, -2.0f), float(W))), y0 = int(fminf(fmaxf(by, -2.0f), float(H)));
    for(int j = 0; j < 2; ++j)
      for(int i = 0; i < 2; ++i)
      {
        const int qx = x0 + i, qy = y0 + j;
        if(qx < 0 || qy < 0 || qx >= W || qy >= H)
          continue;
        const size_t q  = size_t(qy) * W + qx;
        const float4 hm = in.moments[q];
        if(__float_as_uint(hm.w) != id)
          continue;
        if(!(fabsf(depthKey(hm.z) - kp) <= tc.depthTolerance * kp))
          continue;
        if(id != 0u)
        {
          const float4 hn = in.normal[q];
          if(!(hn.x * cn.x + hn.y * cn.y + hn.z * cn.z >= tc.normalCos))
            continue;
        }
        const float4 hi = in.illum[q];
        const float  w  = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
        ++taps;
        sr += w * hi.x;
        sg += w * hi.y;
        sb += w * hi.z;
        sh += w * hi.w;
        s1 += w * hm.x;
        s2 += w * hm.y;
        sw += w;
      }
  }
  float4 ni, nm;
  if(taps == 0 || !(sw > 0.0f))  // (valid taps of weight zero carry nothing)
  {
    taps = 0;
    ni   = make_float4(il.x, il.y, il.z, 1.0f);
    nm   = make_float4(l1, l2, depth[c], mv.w);
  }
  else
  {
    const float h  = fminf(sh / sw + 1.0f, tc.maxHistory);
    const float a  = fmaxf(tc.alpha, 1.0f / h), am = fmaxf(tc.momentsAlpha, 1.0f / h);
    ni             = make_float4(sr / sw * (1.0f - a) + il.x * a, sg / sw * (1.0f - a) + il.y * a, sb / sw * (1.0f - a) + il.z * a, h);
    nm             = make_float4(s1 / sw * (1.0f - am) + l1 * am, s2 / sw * (1.0f - am) + l2 * am, depth[c], mv.w);
  }
  const float var = ni.w >= 4.0f ? fmaxf(0.0f, nm.y - nm.x * nm.x) : spatialVariance7x7(color, albedo, normal, W, H, x, y, ca, cn);
  out.illum[c]    = ni;
  out.moments[c]  = nm;
  out.normal[c]   = make_float4(cn.x, cn.y, cn.z, 0.0f);
  if(validTaps)
    *validTaps = taps;
  return make_float4(ni.x, ni.y, ni.z, var);
}

}  // namespace pt
