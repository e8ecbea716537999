// TEST INFRASTRUCTURE ONLY (see kat_device.hip): known-answer launcher over shadowDepositAdd (pt_scene.h), the three float atomics
// with which the any-hit shadow walk adds an unoccluded ray's term to a radiance record.  The adds execute at the memory side, not
// in the compute unit: whether they round, overflow and treat zeros, infinities and denormals like the `+` of the load / add / store
// they replace is a property of the part, and this launcher asks it.  Part of tests/device_kat/libmi_pt_kat.so, compiled with the
// flags of pt_kernels.o.
//
// One launch of 64 threads.  rad: 64 float4 records (in / out), c: 64 x 3 floats.  Thread i adds c[i] to rad[i].xyz; .w must come back
// as it went in.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_scene.h"

using namespace pt;

namespace {
__global__ void __launch_bounds__(64) k_kat_atomic_deposit(float4* __restrict__ rad, const float* __restrict__ c)
{
  const uint32_t i = threadIdx.x;
  shadowDepositAdd(rad + i, mk3(c[3u * i], c[3u * i + 1u], c[3u * i + 2u]));
}
}  // namespace

extern "C" __attribute__((visibility("default"))) int kat_atomic_deposit(float* rad, const float* c)
{
  float4* dRad = nullptr;
  float*  dC   = nullptr;
  int     err  = int(hipMalloc(&dRad, 64 * sizeof(float4)));
  if(err == int(hipSuccess)) err = int(hipMalloc(&dC, 64 * 3 * sizeof(float)));
  if(err == int(hipSuccess)) err = int(hipMemcpy(dRad, rad, 64 * sizeof(float4), hipMemcpyHostToDevice));
  if(err == int(hipSuccess)) err = int(hipMemcpy(dC, c, 64 * 3 * sizeof(float), hipMemcpyHostToDevice));
  if(err == int(hipSuccess))
  {
    hipLaunchKernelGGL(k_kat_atomic_deposit, dim3(1), dim3(64), 0, 0, dRad, dC);
    err = int(hipGetLastError());
  }
  if(err == int(hipSuccess)) err = int(hipDeviceSynchronize());
  if(err == int(hipSuccess)) err = int(hipMemcpy(rad, dRad, 64 * sizeof(float4), hipMemcpyDeviceToHost));
  (void)hipFree(dRad); (void)hipFree(dC);
  return err;
}
