// TEST INFRASTRUCTURE ONLY (see kat_device.hip): known-answer launcher over LaneStack2 (pt_bvh8.h), the per-lane stack of node
// groups of the 8-wide walks -- 12 groups per lane in LDS, the rest in scratch.  pop() waits for its scratch words inside the
// overflow branch and nowhere else, so that loads the walk keeps in flight across a node step are not drained by every pop;
// this launcher walks every lane of a wave across that boundary, each lane at a depth of its own, with a global load in flight
// across the pops.  Part of tests/device_kat/libmi_pt_kat.so, compiled with the flags of pt_kernels.o.
//
// One wave per case.  depths: 64 ints per case (0 .. KAT_STACK_MAX_DEPTH), probe: 64 words per case.  Every lane
//   1. pushes depths[lane] groups {base, bits} = katGroup(case, lane, level),
//   2. requests probe[lane] (the load stays in flight: its value is not looked at before step 4),
//   3. pops until its stack is empty, lanes of one wave popping from different depths in the same pass,
//   4. pushes (KAT_STACK_MAX_DEPTH - depths[lane]) groups with level + 100 and pops those as well.
// out: per lane 2 * 2 * KAT_STACK_MAX_DEPTH words -- the groups in the order they were popped, first pass then second, unused
// entries 0xffffffff -- then the probe word and the final stack pointer.
#include <hip/hip_runtime.h>

#include <cstdint>

#define PT_FAST_SHADING_MATH 1  // as pt_kernels.hip defines it before its includes
#include "pt_shading.h"
#include "pt_bvh.h"
#include "pt_bvh8.h"

using namespace pt;

constexpr int KAT_STACK_MAX_DEPTH = 20;
constexpr int KAT_STACK_OUT_WORDS = 4 * KAT_STACK_MAX_DEPTH + 2;

namespace {
__device__ NodeGroup katGroup(uint32_t c, uint32_t lane, uint32_t level)
{
  NodeGroup g;
  g.base = 0x01000193u * (c + 1u) + 0x10000u * lane + level;
  g.bits = ~g.base ^ (level << 24);
  return g;
}

__global__ void __launch_bounds__(64) k_kat_lane_stack(const int* __restrict__ depths, const uint32_t* __restrict__ probe, uint32_t* __restrict__ out)
{
  __shared__ int s_stack[2 * BVH8_STACK_LDS * 64];
  uint32_t       overflow[2 * BVH8_STACK_PRIV];
  const uint32_t lane = threadIdx.x, c = blockIdx.x;
  LaneStack2     st;
  st.lds = s_stack; st.tid = int(lane); st.stride = 64; st.sp = 0;
  st.privBase = overflow; st.privBits = overflow + BVH8_STACK_PRIV;
  const int d = min(max(depths[c * 64u + lane], 0), KAT_STACK_MAX_DEPTH);
  uint32_t* o = out + size_t(c * 64u + lane) * KAT_STACK_OUT_WORDS;
  for(int i = 0; i < 4 * KAT_STACK_MAX_DEPTH; ++i)
    o[i] = 0xffffffffu;
  for(int pass = 0; pass < 2; ++pass)
  {
    const int      n   = pass == 0 ? d : KAT_STACK_MAX_DEPTH - d;
    const uint32_t tag = pass == 0 ? 0u : 100u;
#pragma unroll 1
    for(int i = 0; i < KAT_STACK_MAX_DEPTH; ++i)
      if(i < n)
        st.push(katGroup(c, lane, uint32_t(i) + tag));
    const uint32_t inFlight = probe[c * 64u + lane];
#pragma unroll 1
    for(int i = 0; i < KAT_STACK_MAX_DEPTH; ++i)
      if(st.sp > 0)
      {
        const NodeGroup g = st.pop();
        o[(pass * KAT_STACK_MAX_DEPTH + i) * 2]     = g.base;
        o[(pass * KAT_STACK_MAX_DEPTH + i) * 2 + 1] = g.bits;
      }
    if(pass == 0)
      o[4 * KAT_STACK_MAX_DEPTH] = inFlight;
  }
  o[4 * KAT_STACK_MAX_DEPTH + 1] = uint32_t(st.sp);
}
}  // namespace

extern "C" __attribute__((visibility("default"))) int kat_lane_stack(int cases, const int* depths, const uint32_t* probe, uint32_t* out)
{
  if(cases <= 0)
    return 0;
  const size_t nIn = size_t(cases) * 64, nOut = nIn * KAT_STACK_OUT_WORDS;
  int*      dDepths = nullptr;
  uint32_t *dProbe = nullptr, *dOut = nullptr;
  int       err = int(hipMalloc(&dDepths, nIn * sizeof(int)));
  if(err == int(hipSuccess)) err = int(hipMalloc(&dProbe, nIn * sizeof(uint32_t)));
  if(err == int(hipSuccess)) err = int(hipMalloc(&dOut, nOut * sizeof(uint32_t)));
  if(err == int(hipSuccess)) err = int(hipMemcpy(dDepths, depths, nIn * sizeof(int), hipMemcpyHostToDevice));
  if(err == int(hipSuccess)) err = int(hipMemcpy(dProbe, probe, nIn * sizeof(uint32_t), hipMemcpyHostToDevice));
  if(err == int(hipSuccess))
  {
    hipLaunchKernelGGL(k_kat_lane_stack, dim3(unsigned(cases)), dim3(64), 0, 0, dDepths, dProbe, dOut);
    err = int(hipGetLastError());
  }
  if(err == int(hipSuccess)) err = int(hipDeviceSynchronize());
  if(err == int(hipSuccess)) err = int(hipMemcpy(out, dOut, nOut * sizeof(uint32_t), hipMemcpyDeviceToHost));
  (void)hipFree(dDepths); (void)hipFree(dProbe); (void)hipFree(dOut);
  return err;
}
