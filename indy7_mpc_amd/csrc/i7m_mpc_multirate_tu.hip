// i7m_mpc_multirate_tu.hip — k_mpc_multirate_step (i7m_mpc_multirate.h) in a translation unit of its
// own: i7m_api.hip's device code stays what it was, kernel for kernel, whatever this one does to
// the compiler's inlining and scheduling budget.  Default scheduler.
//
// The kernel headers define non-template kernels and device functions too; included inside an
// anonymous namespace, this unit's copies stay internal (as in i7m_lin_tu.hip).  The launcher is the
// only external symbol, with builtin parameter types only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#define I7M_MULTIRATE_KERNEL
namespace {
#include "i7m_mpc_multirate.h"
}  // namespace

// One wave per instance; model: DevModel*, args: MultirateArgs* (i7m_mpc_multirate.h).
hipError_t i7m_launch_multirate_step(int n, hipStream_t s, const void* model, const void* args) {
  const i7m::MultirateArgs& a = *static_cast<const i7m::MultirateArgs*>(args);
  hipLaunchKernelGGL(i7m::k_mpc_multirate_step, dim3(n), dim3(64), 0, s, static_cast<const i7m::DevModel*>(model), n, a);
  return hipGetLastError();
}
