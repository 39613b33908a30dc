// i7m_mpc_sampled_multirate_tu.hip — k_sampled_multirate_step (i7m_mpc_sampled_multirate.h) in a
// translation unit of its own: i7m_api.hip's device code stays what it was, kernel for kernel,
// whatever this one does to the compiler's inlining and scheduling budget.  Default scheduler.
//
// The kernel headers define non-template kernels and device functions too; included inside an
// anonymous namespace, this unit's copies stay internal (as in i7m_lin_tu.hip).  What those headers
// include from outside the namespace (the standard library, the C-ABI header) is included here
// first.  The launcher is the only external symbol, with builtin parameter types only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/indy7_mpc.h"

#define I7M_SAMPLED_MULTIRATE_KERNEL
namespace {
#include "i7m_mpc_sampled_multirate.h"
}  // namespace

// One workgroup per group, H lanes rounded up to whole waves; model: DevModel*, args:
// SampledMultirateArgs* (i7m_mpc_sampled_multirate.h).
hipError_t i7m_launch_sampled_multirate_step(int ng, int H, hipStream_t s, const void* model, const void* args) {
  const i7m::SampledMultirateArgs& a = *static_cast<const i7m::SampledMultirateArgs*>(args);
  hipLaunchKernelGGL(i7m::k_sampled_multirate_step, dim3(ng), dim3((H + 63) / 64 * 64), 0, s,
                     static_cast<const i7m::DevModel*>(model), a);
  return hipGetLastError();
}
