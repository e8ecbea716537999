// The body of the shade kernels k_shade<COUNT, SIMPLE, FIRST> and k_shade_viz<SIMPLE, FIRST> (pt_kernels.hip), included inside each of them with
// COUNT, SIMPLE, FIRST and VIZ in scope (VIZ: the debug views of MiSceneFrameInfo::visualization, pt_visualize.h).  Text, not a function: held
// by a force-inlined device function, the same body compiles the eight k_shade kernels to other schedules and registers (tools/isa_census.py),
// and the path-traced image's kernels are to stay exactly as they were.  No include guard: it is included twice.
  // The scene / frame descriptors reach the non-inlined helpers (getTexture, sampleLights, the sky) by reference.  As
  // by-value kernel arguments they would be copied to scratch (their address escapes) and every field read would become a
  // memory round trip; as device-resident structs they are read through one uniform pointer.
  // ... and as CONSTANT memory (uniformConst): a read of `sc.` / `fc.` that follows a store or a call is otherwise a vector load of a
  // uniform address -- the compiler must assume the store or the callee wrote there -- and the loop is full of both.
  const DevScene&    sc = uniformConst(*scp);
  const FrameConsts& fc = uniformConst(*fcp);
  const bool         stateInQueue = fc.stateInQueue != 0;  // misc / throughput / radiance of a living path ride in its queue entry (pt_scene.h: RayQueue)
  __shared__ uint32_t s_prefix[NSUB + 1];
  __shared__ uint32_t s_push[4];
  __shared__ float    s_srgb[256];  // sRGB decode table next to the ALU: 3 lookups per texel, up to 8 texels per tap
#ifndef SHADE_NO_DEFERRED_MISS
  // Later bounces: the paths that left the scene are not finished where they are found -- by then 5 % (atrium) to 18 % (street) of a queue's rays miss,
  // spread evenly, and nearly every wave ran the environment evaluation (physical sky + sun disc or the HDR lookup, and the MIS weight: ~900 vector
  // instructions) for two or three of its lanes -- but listed in LDS and finished by the whole block, 256 at a time with every lane busy, once that many
  // have gathered (and at the block's end).  A first ray's miss (backplate) and any miss of a frame with the infinite plane stay inline.
  // (As a pass of its own -- a scan of the whole queue for the misses -- the gain was eaten by the scan: profiles/r06_ser_ab.txt.)
  constexpr bool DEFER_MISS = !FIRST;
#else
  constexpr bool DEFER_MISS = false;
#endif
  __shared__ uint32_t s_missPos[DEFER_MISS ? 2 * SHADE_BLOCK : 1];
  __shared__ uint32_t s_missCount;
  // ... and only where the environment is the physical sky: an HDR lookup is too cheap to be worth the list (helmet 5310 -> 5285, glass 551 -> 549 Msamples/s with it,
  // atrium 715 -> 727, street 764 -> 771: profiles/r06_deferred_miss_ab.txt)
  const bool          deferMiss = DEFER_MISS && !hasFlag(fc.frameInfo.flags, MI_SCENE_USE_INFINITE_PLANE) && !hasFlag(fc.frameInfo.flags, MI_SCENE_USE_HDR_ENVIRONMENT);
  if(threadIdx.x == 0)
    s_missCount = 0;  // (the barrier of queuePrefix below orders it)
  // finishes up to 256 listed misses: exactly what the inline branch does for a ray that is not a first ray (gltf_pathtrace.slang:139-156), through the same
  // non-inlined missEnvironmentCall.  Whole block; contains barriers.
  auto finishMisses = [&](bool all) {
    __syncthreads();
    const uint32_t n = s_missCount;
    if(n == 0u || (!all && n < uint32_t(SHADE_BLOCK)))
      return;
    const uint32_t take = min(n, uint32_t(SHADE_BLOCK)), base = n - take;
    uint32_t       pos = 0;
    if(threadIdx.x < take)
      pos = s_missPos[base + threadIdx.x];
    __syncthreads();
    if(threadIdx.x == 0)
      s_missCount = base;
    if(threadIdx.x < take)
    {
      const uint32_t slot  = Q.active[cur].slot[pos];
      const float4   d4    = Q.active[cur].dir[pos];
      const float4   misc4 = stateInQueue ? Q.active[cur].misc[pos] : P.misc[slot];
      const float4   tp4   = stateInQueue ? Q.active[cur].aux2[pos] : P.throughput[slot];
      const float4   rad4  = stateInQueue ? Q.active[cur].rad[pos] : P.radiance[slot];
      f3             radiance = xyz(rad4);
      f3             envColor;
      float          mis;
      missEnvironment(sc, fc, xyz(d4), tp4.w, envColor, mis);
      radiance += xyz(tp4) * mis * envColor;
      // the record an ended path leaves behind (see the end of the round below): flags without ALIVE -- and, from the SIMPLE kernel, without INSIDE
      uint32_t flags = __float_as_uint(misc4.y) & (PF_INSIDE | PF_NOT_SOLID | (0xffu << PF_DEPTH_SHIFT) | (0xffu << PF_SCATTER_SHIFT));
      if(SIMPLE)
        flags &= ~uint32_t(PF_INSIDE);
      const bool solid = !(flags & PF_NOT_SOLID);
      P.radiance[slot] = make_float4(radiance.x, radiance.y, radiance.z, __uint_as_float(__float_as_uint(fmaxf(fabsf(rad4.w), 0.0f)) | (solid ? 0u : RADW_NOT_SOLID)));
      if(P.misc)
        P.misc[slot] = make_float4(misc4.x, __uint_as_float(flags), misc4.z, misc4.w);
    }
    __syncthreads();
  };
  // The window sort exists in the generic kernel only (key: material).  Where every material runs the same code (SIMPLE) grouping by material buys
  // nothing, and a window keyed by next-event technique (rounds 3-4: fewer instructions, fuller waves, 6-15 % SLOWER -- the key costs a dependent gather
  // and the window two barriers, and this kernel waits on gather depth, not on issue) was removed in round 5 together with its registers: the
  // later-bounce SIMPLE kernel spilled 16 VGPRs for a feature that was off (LABNOTES.md).
  constexpr bool CAN_SORT = !SIMPLE;
  __shared__ uint32_t s_order[CAN_SORT ? SORT_WINDOW : 1];                   // queue positions of the window's live entries, sorted by bin
  __shared__ uint16_t s_segCount[CAN_SORT ? SORT_SEGMENTS : 1][SORT_BINS];   // entries of a bin in one (round, wave) segment -> exclusive prefix inside the bin
  __shared__ uint32_t s_binBase[SORT_BINS + 1];                 // first sorted index of each bin; [SORT_BINS] = live entries of the window
  static_assert(SHADE_BLOCK == 256, "one table entry per thread");
  if(blockIdx.x == 0 && threadIdx.x < 8)
  {
    Q.counters[QC_HEADS_TRACE + threadIdx.x] = 0;  // for the next iteration's k_trace_closest
    // ... and for this iteration's shadow stage (k_trace_shadow / k_shadow_resolve run after this launch and, the previous iteration's,
    // before it -- also when that stage runs on its own stream next to the following k_trace_closest)
    Q.counters[QC_HEADS_SHADOW + threadIdx.x]   = 0;
    Q.counters[QC_HEADS_OVERFLOW + threadIdx.x] = 0;
    if(threadIdx.x == 0)
      Q.counters[QC_CAND_POOL] = Q.counters[QC_RESOLVE] = Q.counters[QC_OVERFLOW] = 0;
  }
  queuePrefix(&Q.counters[cur ? QC_PAIR1 : QC_PAIR0], s_prefix);
  const uint32_t count      = s_prefix[NSUB];
  const int      nxt        = cur ^ 1;
  constexpr uint32_t ROUNDS = CAN_SORT ? SORT_ROUNDS : 1u;
  constexpr uint32_t WINDOW = ROUNDS * SHADE_BLOCK;
  const uint32_t     numWindows = (count + WINDOW - 1) / WINDOW;
  if(blockIdx.x >= numWindows)
    return;  // nothing for this block (late bounces launch the full grid on short or empty queues)
  s_srgb[threadIdx.x] = sc.srgbLut[threadIdx.x];
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for(uint32_t win = blockIdx.x; win < numWindows; win += gridDim.x)
  {
    // ---- Per-bounce sort of the queue, one SORT_WINDOW-entry window at a time, in LDS (no extra pass over HBM, no global atomics):
    // key = dead entries last, paths that left the scene (or reach the infinite plane) before them, surface hits first and grouped
    // by material -- so that a wave shades one kind of thing, the texture / material records it gathers are shared by its lanes,
    // and the dead entries the bounce-0 kernel leaves behind cost nothing.  Stable counting sort: a lane's rank inside its
    // (round, wave) segment comes from ballots over the distinct bins of the wave (usually one to three), the segments of a bin
    // are laid out in queue order.  Paths are independent, so the processing order cannot change any result.
    uint32_t live = min(WINDOW, count - win * WINDOW);  // no sort: the window as it is, dead entries and all
    if(CAN_SORT && sortMode != 0)
    {
    uint32_t myPos[SORT_ROUNDS], myBin[SORT_ROUNDS], myRank[SORT_ROUNDS];
    for(uint32_t t = threadIdx.x; t < SORT_SEGMENTS * SORT_BINS; t += SHADE_BLOCK)
      (&s_segCount[0][0])[t] = 0;
    __syncthreads();
#pragma unroll
    for(uint32_t k = 0; k < SORT_ROUNDS; ++k)
    {
      const uint32_t i = win * WINDOW + k * SHADE_BLOCK + threadIdx.x;
      uint32_t       bin = SORT_BIN_DEAD;
      myPos[k]           = 0u;
      if(i < count)
      {
        myPos[k]            = queuePos(Q.subCap, s_prefix, i);
        const uint32_t slot = Q.active[cur].slot[myPos[k]];
        if(slot != QUEUE_DEAD)
        {
          const int tri = __float_as_int(Q.active[cur].aux[myPos[k]].y);
          // sortMode 1: surface hits / the rest / dead; 2: surface hits grouped by material as well
          if(tri < 0)
            bin = SORT_BIN_MISS;
          else
            bin = sortMode >= 2 ? uint32_t(sc.shadeTris[tri].materialID) % SORT_BIN_MISS : 0u;
        }
      }
      myBin[k] = bin;
      // rank among the lanes of this wave with the same bin, and the segment's count of that bin
      uint32_t           rank = 0;
      unsigned long long todo = __ballot(bin != SORT_BIN_DEAD);
      while(todo != 0ull)
      {
        const uint32_t           b = uint32_t(__builtin_amdgcn_readlane(int(bin), __ffsll((long long)todo) - 1));
        const unsigned long long m = __ballot(bin == b);
        if(bin == b)
          rank = laneCountBelow(m);
        if(lane == 0)
          s_segCount[k * 4 + wave][b] = uint16_t(__popcll(m));
        todo &= ~m;
      }
      myRank[k] = rank;
    }
    __syncthreads();
    if(threadIdx.x < SORT_BINS)  // exclusive prefix of the segments inside each bin (queue order), and the bin totals
    {
      uint32_t acc = 0;
      for(uint32_t sgm = 0; sgm < SORT_SEGMENTS; ++sgm)
      {
        const uint32_t c = s_segCount[sgm][threadIdx.x];
        s_segCount[sgm][threadIdx.x] = uint16_t(acc);
        acc += c;
      }
      // bins are laid out in index order: surface hits by material, then misses; dead entries are not laid out at all
      uint32_t incl = acc;
#pragma unroll
      for(int d = 1; d < SORT_BINS; d <<= 1)
      {
        const uint32_t t = uint32_t(__shfl_up(int(incl), d));
        if(threadIdx.x >= uint32_t(d))
          incl += t;
      }
      s_binBase[threadIdx.x] = incl - acc;
      if(threadIdx.x == SORT_BINS - 1)
        s_binBase[SORT_BINS] = incl;
    }
    __syncthreads();
#pragma unroll
    for(uint32_t k = 0; k < SORT_ROUNDS; ++k)
      if(myBin[k] != SORT_BIN_DEAD)
        s_order[s_binBase[myBin[k]] + s_segCount[k * 4 + wave][myBin[k]] + myRank[k]] = myPos[k];
    __syncthreads();
    live = s_binBase[SORT_BINS];
    }
   for(uint32_t round = 0; round * SHADE_BLOCK < live; ++round)
   {
    const uint32_t chunk   = win * ROUNDS + round;  // 256 processed entries append to sub-queue chunk % NSUB, like a chunk of the queue
    const uint32_t e       = round * SHADE_BLOCK + threadIdx.x;
    const bool     inRange = e < live;
    const uint32_t inPos   = !inRange ? 0u : ((CAN_SORT && sortMode != 0) ? s_order[e] : queuePos(Q.subCap, s_prefix, win * WINDOW + e));
    uint32_t       slot    = inRange ? Q.active[cur].slot[inPos] : QUEUE_DEAD;
    bool           alive = false, pushShadow = false;
    unsigned       taps = 0;
    float4         nextOrg = make_float4(0, 0, 0, 0), nextDir = make_float4(0, 0, 0, 0);
    float4         nextRad = make_float4(0, 0, 0, 0), nextMisc = make_float4(0, 0, 0, 0), nextThr = make_float4(0, 0, 0, 0);  // state of a path that goes on
    float4         shOrg = make_float4(0, 0, 0, 0), shDir = make_float4(0, 0, 0, 0), shCon = make_float4(0, 0, 0, 0), shCon2 = make_float4(0, 0, 0, 0);
    bool           catcher = false;
#ifdef SHADE_PROFILE
    const unsigned long long sprofRound0 = __builtin_amdgcn_s_memtime();
#endif
    if(inRange && slot != QUEUE_DEAD)
    {
      SPROF_BEGIN();
      const float4 hit4 = Q.active[cur].aux[inPos], o4 = Q.active[cur].org[inPos], d4 = Q.active[cur].dir[inPos];
      // the path's state: records of its queue entry (unit stride, like the ray), or -- catcher frames / MI_PT_STATE_BY_SLOT -- gathered by slot
      // (round 6: the NEXT round's entry prefetched into registers across the append -- 28 VGPRs spilled at the 168-register budget: atrium 690.7 -> 686.7,
      //  helmet 5255 -> 5068 Msamples/s; and staged through LDS by global_load_lds together with its triangle's shade record (no register held: 37 KB of LDS
      //  per block, one more barrier, every later wait of the round a full drain): atrium 722.9 -> 717.3, helmet 5216 -> 5099; and only the first TWO levels of the next
      //  window's chain held -- position, hit triangle, 32-byte shade record, ten registers: later-bounce shade 0.661 -> 0.710 ms, atrium 730.9 -> 717.2 -- profiles/r06_shade_walk_ab.txt)
      const float4 misc4 = stateInQueue ? Q.active[cur].misc[inPos] : P.misc[slot];
      const float4 tp4   = FIRST ? make_float4(1.0f, 1.0f, 1.0f, DIRAC) : (stateInQueue ? Q.active[cur].aux2[inPos] : P.throughput[slot]);
      const float4 rad4  = FIRST ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : (stateInQueue ? Q.active[cur].rad[inPos] : P.radiance[slot]);
      f3       rayOrigin = xyz(o4), rayDir = xyz(d4);
      float    coneWidth = misc4.w;
      f3       throughput = xyz(tp4), radiance = xyz(rad4);
      float    lastSamplePdf = tp4.w;
      f2       maxRoughness  = mk2(fabsf(rad4.w), misc4.x);  // the sign of radiance.w is the path's !solid (PathSoA)
      uint32_t flags = __float_as_uint(misc4.y), seed = __float_as_uint(misc4.z);
      int      surfaceDepth   = int((flags >> PF_DEPTH_SHIFT) & 0xffu);
      int      scatterBounces = int((flags >> PF_SCATTER_SHIFT) & 0xffu);
      bool     isInside = !SIMPLE && (flags & PF_INSIDE) != 0u, solid = !(flags & PF_NOT_SOLID);
      const bool firstRay = (surfaceDepth == 0);
      bool       guideWritten = false;
      const int  maxDepth = fc.pc.maxDepth;
      // the first-hit position only feeds the NDC depth of a first frame (k_finish_sample), i.e. frame 0 of the batch
      const bool needFirstHit = hasFlag(fc.pc.flags, MI_PT_FIRST_FRAME) && pathSlotFrame(fc, slot) == 0u;

      float hitT   = hit4.x;
      int   triIdx = __float_as_int(hit4.y);
      bool  done   = false;  // eBreak
      bool  deferred = false;  // a miss handed to finishMisses
      bool  earlyContinue = false;

      HitState hit;
      uint4    core0 = make_uint4(0u, 0u, 0u, 0u);
      int      rnodeID = -1, primitiveID = -1, materialID = 0;
      (void)primitiveID;
      // (VIZ: what the debug views need besides the material.  The plane hit below does not set them: like the reference's checkInfinitePlaneIntersection,
      //  which leaves the payload alone, a plane in front of a mesh hit keeps that triangle's values; with no mesh hit they stay front face, opaque, no primitive)
      int      rprimID = -1, ommState = 0;
      bool     frontFace = true;
      const bool meshHit = triIdx >= 0;
      if(meshHit)
      {
        const DevShadeTri S = gat(sc.shadeTris, triIdx);
        rnodeID             = int(S.rnode);
        primitiveID         = int(S.prim);
        materialID          = S.materialID;
        if(!FIRST)  // (in flight next to the vertices: evaluateMaterial<SIMPLE, CORE> plans the base-colour fetch from it)
          core0 = gat(sc.coreTex, 5u * uint32_t(materialID));
        const MiGltfRenderNode& rn = gat(sc.nodes, rnodeID);
        // record -> vertices directly; the primitive's stream table only for the attributes that are not interleaved (uv1, colours)
        // (round 6: ONE 192-byte record per triangle -- its three vertices copied, the shade record's fields, the base-colour slot record -- so that vertices, material index
        //  and texel addresses are one round trip behind the queue entry instead of two: GPU suite green, later-bounce shade 0.659 -> 0.664 ms (atrium), 0.653 -> 0.676 (sliver
        //  atrium), helmet / street unchanged -- de-indexed vertices lose the lines neighbouring hits share.  Removed: profiles/r06_shade_walk_ab.txt)
        DevPrim rp{};
        u3      ti{0u, 0u, 0u};
        if(S.attrs & (SHADE_HAS_UV1 | SHADE_HAS_COLORS))
        {
          rp = gat(sc.prims, S.renderPrimID);
          ti = getTriangleIndices(rp, int(S.prim));
        }
        hit = getHitState(&gat(sc.geomPool, S.v0), &gat(sc.geomPool, S.v1), &gat(sc.geomPool, S.v2), S.attrs, &rp, ti,
                          mk3(1.0f - hit4.z - hit4.w, hit4.z, hit4.w), rn.worldToObject, rn.objectToWorld, rayDir, VIZ ? &frontFace : nullptr);
        // The triangle of the first-hit record (vertex motion), written here where the record and the barycentrics are at hand and nothing has to
        // stay alive for it: a first ray's mesh hit that needs the first hit either gets the mesh-hit `firstHit` store below from this same lane, or lies
        // behind the infinite plane, whose id 0 makes every reader ignore this record.
        if(P.firstHitTri && firstRay && needFirstHit)
          P.firstHitTri[pathSlotPixel(fc, slot)] = make_uint4(uint32_t(S.renderPrimID), S.prim, __float_as_uint(hit4.z), __float_as_uint(hit4.w));
        if constexpr(VIZ)
        {
          rprimID = S.renderPrimID;
          // opacity-micromap view: the walks ran without alpha (launchTraceClosest / launchTracePrimary), so this is the closest triangle with alpha-tested
          // geometry taken as opaque; it is "unknown" when the walks would still test its alpha at run time (no FORCE_OPAQUE in its triangle record)
          if(fc.frameInfo.visualization == MI_VIZ_OPACITY_MICROMAP)
            ommState = (__float_as_uint(gat(sc.tris, triIdx).c.w) & INST_FORCE_OPAQUE) ? 0 : 1;
        }
      }
      else
        hitT = INFINITE_F;
      SPROF_END(0);

      // checkInfinitePlaneIntersection, pathtrace_functions.h.slang:556-585
      bool hitInfinitePlane = false;
      {
        const float t = infinitePlaneT(fc, rayOrigin, rayDir, hitT);
        if(t > 0.0f)
        {
          hitT             = t;
          hit.pos          = rayOrigin + rayDir * hitT;
          hit.shadowPos    = hit.pos;
          hit.nrm          = mk3(0, 1, 0);
          hit.geonrm       = mk3(0, 1, 0);
          hit.tangent      = mk3(1, 0, 0);
          hit.bitangent    = mk3(0, 0, 1);
          hitInfinitePlane = true;
        }
      }

      if(deferMiss && hitT == INFINITE_F && !firstRay)  // finished by the whole block later (finishMisses): nothing else of this entry is touched
      {
        SPROF_BEGIN();
        s_missPos[atomicAdd(&s_missCount, 1u)] = inPos;
        deferred = true;
        done     = true;
        SPROF_END(6);
      }
      else if(hitT == INFINITE_F)  // gltf_pathtrace.slang:129-156
      {
        SPROF_BEGIN();
        bool backplate = false;
        if(firstRay)  // tryPrimaryMissBackplate, pathtrace_functions.h.slang:944-971
        {
          solid             = false;
          if(needFirstHit)
            P.firstHit[pathSlotPixel(fc, slot)] = make_float4(rayDir.x, rayDir.y, rayDir.z, 0.0f);  // (.w: id 0, a direction -- pt_temporal.h)
          backplate = primaryMissBackplate(sc, fc, rayDir, radiance);
        }
        if(!backplate)
        {
          f3    envColor;
          float mis;
          missEnvironment(sc, fc, rayDir, lastSamplePdf, envColor, mis);
          radiance += throughput * mis * envColor;
        }
        done = true;
        SPROF_END(6);
      }

      if(!done)
      {
        PbrMaterial pbrMat;
        // rayConeWorldFootprint, pathtrace_functions.h.slang:174-178
        float worldFoot = (coneWidth + fc.pc.pixelAngle * hitT) / fmaxf(fabsf(dot(hit.geonrm, -rayDir)), 1e-3f);
        bool  unlit     = false;
        bool  catcherPlane = false;  // shadow-catcher hit: the rest of the bounce is skipped (eBreak / eEarlyContinue)
        if(hitInfinitePlane)
        {
          pbrMat           = defaultPbrMaterial();
          pbrMat.baseColor = mk3(fc.frameInfo.infinitePlaneBaseColor);
          pbrMat.metallic  = fc.frameInfo.infinitePlaneMetallic;
          float r          = fc.frameInfo.infinitePlaneRoughness;
          pbrMat.roughness = mk2(r * r, r * r);
          pbrMat.N = hit.nrm; pbrMat.Ng = hit.nrm; pbrMat.Nc = hit.nrm;
          pbrMat.T = hit.tangent; pbrMat.B = hit.bitangent;
          // handleShadowCatcher, pathtrace_functions.h.slang:499-554 (called from gltf_pathtrace.slang:169-187).  The reference
          // needs the shadow factor inside the bounce; here the bounce is finished speculatively (the alpha draws of
          // TraceShadow do not advance the seed, §6, so the continuation sample is the same) and k_trace_shadow applies the
          // radiance terms and drops the continuation again when the point turns out to be unshadowed.
          if(hasFlag(fc.frameInfo.flags, MI_SCENE_INFINITE_PLANE_SHADOW_CATCHER))
          {
            catcherPlane = true;
            coneWidth    = worldFoot;
            if(FIRST && needFirstHit)  // the reference leaves SampleResult::hitPosition at its 1e34 default on this path
              P.firstHit[pathSlotPixel(fc, slot)] = make_float4(1e34f, 1e34f, 1e34f, __uint_as_float(TEMPORAL_ID_INVALID));
            DirectLight dl;
            sampleLights(sc, fc, hit.pos, seed, dl);
            const bool traceIt = dot(dl.direction, hit.nrm) > 0.0f && dl.pdf != 0.0f;
            f3         envColor;
            float      envPdf;
            sampleEnvironment(sc, fc, rayDir, envColor, envPdf);
            const float mis         = computeEnvHitMisWeight(sc, fc, lastSamplePdf, envPdf);
            const f3    unshadowed  = throughput * mis * envColor;
            if(!traceIt)
            {
              radiance += unshadowed;
              done = true;
            }
            else
            {
              shOrg = make_float4(hit.pos.x, hit.pos.y, hit.pos.z, INFINITE_F);
              shDir = make_float4(dl.direction.x, dl.direction.y, dl.direction.z, __uint_as_float(2u));
              shCon = make_float4(envColor.x, envColor.y, envColor.z, __uint_as_float(seed));
              shCon2     = make_float4(unshadowed.x, unshadowed.y, unshadowed.z, 0.0f);
              pushShadow = true;
              catcher    = true;
              float      r1 = rnd(seed), r2 = rnd(seed), r3 = rnd(seed);
              BsdfSample sd = bsdfSampleSimple(-rayDir, mk3(r1, r2, r3), pbrMat);
              if(sd.event_type == BSDF_EVENT_ABSORB)
                done = true;
              else
              {
                f3 offsetDir = dot(sd.k2, hit.geonrm) > 0.0f ? hit.geonrm : -hit.geonrm;
                rayOrigin    = safeOffsetRay(hit.pos, offsetDir);
                rayDir       = normalize(sd.k2);  // pathTrace loop head, gltf_pathtrace.slang:447
                throughput *= sd.bsdf_over_pdf;
                lastSamplePdf = sd.pdf;
              }
            }
          }
        }
        else
        {
          const MiGltfShadeMaterial& mat = gat(sc.materials, materialID);
          MeshState                  mesh;
          mesh.N = hit.nrm; mesh.T = hit.tangent; mesh.B = hit.bitangent; mesh.Ng = hit.geonrm;
          mesh.tc0 = hit.uv0; mesh.tc1 = hit.uv1;
          mesh.isInside           = isInside;
          mesh.texGrad            = worldFoot * hit.texelDensity * fc.pc.texGradScale;
          mesh.baseColorVertexMul = hit.color;
          mesh.tex                = TexCtx{sc.texRefs, sc.texels, s_srgb, sc.texQuads};
          mesh.core0              = core0;
          SPROF_BEGIN();
          pbrMat                  = evaluateMaterial<SIMPLE, !FIRST>(sc, mat, mesh, taps);  // (!FIRST: the base colour through its core record, pt_shading.h)
          unlit                   = mat.unlit > 0;
          SPROF_END(1);
        }
        if(!catcherPlane)
        {
          if(firstRay)  // gltf_pathtrace.slang:228-264
          {
            if(needFirstHit)
              // .w: the bits of the first hit's id for the motion vectors (pt_temporal.h): renderNode + 1; 0 on the infinite plane, tested first --
              // a plane in front of a mesh hit keeps that triangle's rnodeID
              P.firstHit[pathSlotPixel(fc, slot)] = make_float4(hit.pos.x, hit.pos.y, hit.pos.z, __uint_as_float(hitInfinitePlane ? 0u : uint32_t(rnodeID + 1)));
            if(P.guideAlbedo)
            {
              float4 ga = make_float4(0, 0, 0, 0), gn = ga;
              if(fc.pc.numSamples > 1)  // (the sum over the frame's samples, zeroed by sample 0: generateCameraPath)
              {
                ga = P.guideAlbedo[slot];
                gn = P.guideNormal[slot];
              }
              guideWritten        = true;
              P.guideAlbedo[slot] = make_float4(ga.x + pbrMat.baseColor.x, ga.y + pbrMat.baseColor.y, ga.z + pbrMat.baseColor.z, ga.w + 1.0f);
              P.guideNormal[slot] = make_float4(gn.x + pbrMat.N.x, gn.y + pbrMat.N.y, gn.z + pbrMat.N.z, 0.0f);
            }
          }
          maxRoughness     = mk2(fmaxf(pbrMat.roughness.x, maxRoughness.x), fmaxf(pbrMat.roughness.y, maxRoughness.y));  // :267-268
          pbrMat.roughness = maxRoughness;
          if constexpr(VIZ)  // :270-287: a flat colour ends a first ray here; clay changes the material of every hit and shading goes on
          {
            f3        vizColour;
            const int vr = applyVisualization(pbrMat, hit, frontFace, fc.frameInfo.visualization, rprimID, primitiveID, ommState, vizColour);
            if(vr == VIZ_COLOR_OVERRIDE && firstRay)
            {
              radiance = vizColour;
              done     = true;
            }
          }
          if(!VIZ || !done)
          {
            radiance += pbrMat.emissive * throughput;  // :293
            if(unlit)                                  // :298-304
            {
              radiance += pbrMat.baseColor;
              done = true;
            }
          }

          // processVolumeSegment, pathtrace_functions.h.slang:904-939
          bool volumeContinue = false;
          if(!SIMPLE && !done && isInside)
          {
            f3    ext, scat;
            float aniso;
            unpackMedium(P.medium[slot], ext, scat, aniso);
            if(maxComp(ext) > 0.0f || maxComp(scat) > 0.0f)
            {
              // handleVolumeScatter, :605-645
              bool  scattered  = false;
              float maxScatter = maxComp(scat);
              f3    wiBefore = rayDir, originBefore = rayOrigin;
              if(maxScatter > VOLUME_MIN_SCATTER)
              {
                float maxExt      = maxComp(ext);
                float scatterDist = -logf(fmaxf(rnd(seed), VOLUME_RAND_FLOOR)) / maxExt;
                if(scatterDist < hitT)
                {
                  throughput *= mk3(1.0f) - (ext - scat) / maxExt;
                  rayOrigin     = rayOrigin + rayDir * scatterDist;
                  float r1 = rnd(seed), r2 = rnd(seed);
                  rayDir        = sampleHenyeyGreenstein(mk2(r1, r2), aniso, wiBefore);
                  lastSamplePdf = henyeyGreensteinPdf(dot(wiBefore, rayDir), aniso);
                  scattered     = true;
                }
                else
                  throughput *= exp3((mk3(maxExt) - ext) * hitT);
              }
              else
                throughput *= exp3(ext * (-hitT));
              if(scattered)
              {
                scatterBounces = min(scatterBounces + 1, 255);
                coneWidth += fc.pc.pixelAngle * length(rayOrigin - originBefore);
                // volumeScatterNEE, :651-672 (the shadow ray is deferred to k_trace_shadow; initialInside = true)
                DirectLight dl;
                sampleLights(sc, fc, rayOrigin, seed, dl);
                if(dl.pdf > 0.0f)
                {
                  float phasePdf = henyeyGreensteinPdf(dot(wiBefore, dl.direction), aniso);
                  float mis      = dl.pdf / (dl.pdf + phasePdf);
                  f3    contrib  = throughput * dl.radianceOverPdf * mis * phasePdf;
                  shOrg = make_float4(rayOrigin.x, rayOrigin.y, rayOrigin.z, dl.distance);
                  shDir = make_float4(dl.direction.x, dl.direction.y, dl.direction.z, __uint_as_float(1u));
                  shCon = make_float4(contrib.x, contrib.y, contrib.z, __uint_as_float(seed));
                  pushShadow            = true;
                }
                if(scatterBounces >= VOLUME_FREE_BUDGET)
                {
                  float rrPcont = fminf(maxComp(throughput) + RR_PCONT_FLOOR, RR_PCONT_CAP);
                  if(rnd(seed) >= rrPcont)
                    done = true;
                  else
                    throughput /= rrPcont;
                }
                volumeContinue = !done;
                rayDir         = normalize(rayDir);
              }
            }
          }

          if(!done && !volumeContinue)
          {
            coneWidth = worldFoot;  // :313
            DirectLight dl;
#ifdef MI_PT_DIAG_NO_NEE  // cost-attribution build (tools/attribution.sh): wrong image, no next-event estimation
            dl = DirectLight{};
#else
            {
              SPROF_BEGIN();
              sampleLights(sc, fc, hit.pos, seed, dl);  // :319-320
              SPROF_END(2);
            }
#endif
            bool nextEventValid = (dot(dl.direction, hit.nrm) > 0.0f || pbrMat.diffuseTransmissionFactor > 0.0f) && dl.pdf != 0.0f;
            f3   contribution   = mk3(0.0f);
            if(nextEventValid)  // :330-351
            {
              SPROF_BEGIN();
              float    r1 = rnd(seed), r2 = rnd(seed), r3 = rnd(seed);
              BsdfEval ev = bsdfEvaluate(-rayDir, dl.direction, mk3(r1, r2, r3), pbrMat);
              if(ev.pdf > 0.0f)
              {
                float mis    = (dl.pdf == DIRAC) ? 1.0f : dl.pdf / (dl.pdf + ev.pdf);
                contribution = throughput * dl.radianceOverPdf * mis * ev.bsdf;
              }
              SPROF_END(3);
            }
            {  // :357-416
              SPROF_BEGIN();
              float      r1 = rnd(seed), r2 = rnd(seed), r3 = rnd(seed);
#ifdef MI_PT_DIAG_NO_SAMPLE  // cost-attribution build: mirror direction at half weight instead of the BSDF sample
              BsdfSample sd{};
              sd.k2 = rayDir - hit.nrm * (2.0f * dot(rayDir, hit.nrm)); sd.bsdf_over_pdf = mk3(0.5f * r1 + 0.25f); sd.pdf = 1.0f + r2 + r3;
              sd.event_type = BSDF_EVENT_GLOSSY_REFLECTION;
#else
              BsdfSample sd = bsdfSample(-rayDir, mk3(r1, r2, r3), pbrMat);
#endif
              throughput *= sd.bsdf_over_pdf;
              rayDir        = sd.k2;
              lastSamplePdf = sd.pdf;
              if(sd.event_type != BSDF_EVENT_ABSORB)
              {
                f3 offsetDir = dot(rayDir, hit.geonrm) > 0.0f ? hit.geonrm : -hit.geonrm;
                rayOrigin    = safeOffsetRay(hit.pos, offsetDir);
                if(!SIMPLE && (sd.event_type & BSDF_EVENT_TRANSMISSION))
                {
                  isInside = !isInside;
                  if(isInside)  // makeVolumeMedium, pathtrace_functions.h.slang:125-132
                    P.medium[slot] = packMedium(volumeExtinctionCoefficient(pbrMat), pbrMat.scatterCoefficient, pbrMat.scatterAnisotropy);
                }
              }
              else
                surfaceDepth = maxDepth;
              SPROF_END(4);
            }
            if(nextEventValid)  // :421-426 + the TraceShadow of pathTrace :462-471, deferred to k_trace_shadow
            {
              bool forward = dot(dl.direction, hit.nrm) > 0.0f;
              f3   sOrg    = safeOffsetRay(forward ? hit.shadowPos : hit.pos, forward ? hit.geonrm : -hit.geonrm);
              shOrg = make_float4(sOrg.x, sOrg.y, sOrg.z, dl.distance);
              shDir = make_float4(dl.direction.x, dl.direction.y, dl.direction.z, __uint_as_float(0u));
              shCon = make_float4(contribution.x, contribution.y, contribution.z, __uint_as_float(seed));
              pushShadow            = true;
            }
            // Russian roulette, :476-482
            if(surfaceDepth >= RR_MIN_DEPTH)
            {
              float rrPcont = fminf(maxComp(throughput) + 0.001f, 0.95f);
              if(rnd(seed) >= rrPcont)
                done = true;
              else
                throughput /= rrPcont;
            }
            if(!done)
            {
              surfaceDepth++;
              rayDir = normalize(rayDir);
            }
          }
        }
        (void)earlyContinue;
      }

      if(FIRST && P.guideAlbedo && !guideWritten && fc.pc.numSamples == 1)  // a path without a first surface hit (miss, catcher plane): empty guides
      {
        P.guideAlbedo[slot] = make_float4(0, 0, 0, 0);
        P.guideNormal[slot] = make_float4(0, 0, 0, 0);
      }
      alive = !done && surfaceDepth < maxDepth;
      flags = (isInside ? PF_INSIDE : 0u) | (solid ? 0u : PF_NOT_SOLID) | (alive ? PF_ALIVE : 0u) | (uint32_t(min(surfaceDepth, 255)) << PF_DEPTH_SHIFT)
              | (uint32_t(scatterBounces) << PF_SCATTER_SHIFT);
      // (fmaxf: a NaN or negative maxRoughness.x from degenerate material input must not collide with RADW_PRIMARY_MISS or the flag bit)
      nextRad  = make_float4(radiance.x, radiance.y, radiance.z, __uint_as_float(__float_as_uint(fmaxf(maxRoughness.x, 0.0f)) | (solid ? 0u : RADW_NOT_SOLID)));
      nextMisc = make_float4(maxRoughness.y, __uint_as_float(flags), __uint_as_float(seed), coneWidth);
      // A path that ends here leaves its radiance where k_finish_sample reads it and its seed where the next sample of a multi-sample
      // frame picks it up; one that goes on takes its state along in its queue entry (below, once the entry's position is known).
      if((!stateInQueue || !alive) && !deferred)
      {
        P.radiance[slot] = nextRad;
        if(P.misc)  // (null unless the frame has several samples or its state lives by slot: PathSoA)
          P.misc[slot] = nextMisc;
      }
      if(alive)
      {
        nextOrg = make_float4(rayOrigin.x, rayOrigin.y, rayOrigin.z, 0.0f);
        nextDir = make_float4(rayDir.x, rayDir.y, rayDir.z, __uint_as_float(seed));  // .w: the path's seed -- the walk's alpha draws start from it
        nextThr = make_float4(throughput.x, throughput.y, throughput.z, lastSamplePdf);
        if(!stateInQueue)
          P.throughput[slot] = nextThr;
      }
      if(COUNT && taps)
        atomicAdd(&stats->textureTaps, (unsigned long long)taps);
      if(COUNT && (meshHit || hitInfinitePlane))
        atomicAdd(&stats->surfaceHits, 1ull);
    }
#ifdef SHADE_PROFILE
    const unsigned long long sprofPush0 = __builtin_amdgcn_s_memtime();
#endif
    const PushPos  pp      = queuePushBlock2(alive, pushShadow, Q.subCap, &Q.counters[(nxt ? QC_PAIR1 : QC_PAIR0) + 2 * (chunk % NSUB)], chunk % NSUB, s_push);
    const uint32_t posNext = pp.next, posShadow = pp.shadow;
    if(alive)
    {
      Q.active[nxt].slot[posNext] = slot;
      Q.active[nxt].org[posNext]  = nextOrg;
      Q.active[nxt].dir[posNext]  = nextDir;
      if(stateInQueue)
      {
        Q.active[nxt].rad[posNext]  = nextRad;
        Q.active[nxt].misc[posNext] = nextMisc;
        Q.active[nxt].aux2[posNext] = nextThr;
      }
    }
    if(pushShadow)
    {
      // where the shadow stage (k_trace_shadow, or k_shadow_resolve) adds this ray's term: the path's next queue entry while it lives, PathSoA::radiance once it has ended
      Q.shadow.slot[posShadow] = (stateInQueue && alive) ? (posNext | SHADOW_TARGET_QUEUE) : slot;
      Q.shadow.org[posShadow]  = shOrg;
      Q.shadow.dir[posShadow]  = shDir;
      Q.shadow.aux[posShadow]  = shCon;
      if(catcher)
        Q.shadow.aux2[posShadow] = make_float4(shCon2.x, shCon2.y, shCon2.z, __uint_as_float(alive ? posNext : 0xffffffffu));
    }
#ifdef SHADE_PROFILE
    if(!FIRST && laneId() == 0)
    {
      const unsigned long long t_ = __builtin_amdgcn_s_memtime();
      atomicAdd(&g_shadeProf[14], t_ - sprofPush0);
      atomicAdd(&g_shadeProf[15], (t_ - sprofPush0) * (unsigned long long)__popcll(__ballot(alive || pushShadow)));
    }
    const unsigned long long sprofFin0 = __builtin_amdgcn_s_memtime();
#endif
    if(DEFER_MISS && deferMiss)
      finishMisses(false);  // (once 256 have gathered)
#ifdef SHADE_PROFILE
    if(!FIRST && laneId() == 0)
    {
      const unsigned long long t_ = __builtin_amdgcn_s_memtime();
      atomicAdd(&g_shadeProf[16], t_ - sprofFin0);
      atomicAdd(&g_shadeProf[18], t_ - sprofRound0);
      atomicAdd(&g_shadeProf[19], (t_ - sprofRound0) * (unsigned long long)__popcll(__ballot(inRange && slot != QUEUE_DEAD)));
    }
#endif
   }  // rounds of the window
   if(CAN_SORT)
     __syncthreads();  // s_order / s_segCount are rebuilt for the next window
  }
  if(DEFER_MISS && deferMiss)
  {
    finishMisses(true);
    finishMisses(true);  // (at most 511 were listed)
  }
