// i7m_mpc_policy_tu.hip — k_policy_gather and k_mpc_multirate_policy_step (i7m_mpc_policy.h) in a
// translation unit of their own: every other unit's device code, k_mpc_multirate_step's included,
// stays what it was, kernel for kernel.  Default scheduler.
//
// The kernel headers define non-template kernels and device functions too; included inside an
// anonymous namespace, this unit's copies stay internal (as in i7m_mpc_multirate_tu.hip).  The
// launchers are the only external symbols, with builtin parameter types only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#define I7M_POLICY_KERNELS
namespace {
#include "i7m_mpc_policy.h"
}  // namespace

// One workgroup per problem: K_out (B, n_k, 6, 13) from kbuf (B, N - 1, KBUF_STRIDE), device pointers.
hipError_t i7m_launch_policy_gather(int B, int N, int n_k, hipStream_t s, const double* kbuf, double* K_out) {
  hipLaunchKernelGGL(i7m::k_policy_gather, dim3(B), dim3(256), 0, s, N, n_k, kbuf, K_out);
  return hipGetLastError();
}

// One wave per instance; model: DevModel*, args: MultirateArgs* (i7m_mpc_multirate.h); knots:
// PolicyKnots*, this step's knot index per sub-step; kbuf: the launch's first instance's gains.
hipError_t i7m_launch_multirate_policy_step(int n, hipStream_t s, const void* model, const void* args, const void* knots,
                                            const double* kbuf) {
  const i7m::MultirateArgs& a = *static_cast<const i7m::MultirateArgs*>(args);
  const i7m::PolicyKnots& kn = *static_cast<const i7m::PolicyKnots*>(knots);
  hipLaunchKernelGGL(i7m::k_mpc_multirate_policy_step, dim3(n), dim3(64), 0, s, static_cast<const i7m::DevModel*>(model), n, a,
                     kn, kbuf);
  return hipGetLastError();
}
