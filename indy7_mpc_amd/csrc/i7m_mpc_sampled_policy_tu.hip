// i7m_mpc_sampled_policy_tu.hip — k_sampled_multirate_policy_step and k_ctrl_policy_copy
// (i7m_mpc_sampled_policy.h) in a translation unit of their own: every other unit's device code,
// k_sampled_multirate_step's included, stays what it was, kernel for kernel.  Default scheduler.
//
// The kernel headers define non-template kernels and device functions too; included inside an
// anonymous namespace, this unit's copies stay internal (as in i7m_mpc_sampled_multirate_tu.hip).
// What those headers include from outside the namespace is included here first.  The launchers are
// the only external symbols, with builtin parameter types only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/indy7_mpc.h"

#define I7M_SAMPLED_POLICY_KERNELS
namespace {
#include "i7m_mpc_sampled_policy.h"
}  // namespace

// One workgroup per group, H lanes rounded up to whole waves; model: DevModel*, args:
// SampledMultirateArgs*, knots: PolicyKnots* (this step's knot index per sub-step), kbuf: the gains of
// the launch's first row.
hipError_t i7m_launch_sampled_multirate_policy_step(int ng, int H, hipStream_t s, const void* model, const void* args,
                                                    const void* knots, const double* kbuf) {
  const i7m::SampledMultirateArgs& a = *static_cast<const i7m::SampledMultirateArgs*>(args);
  const i7m::PolicyKnots& kn = *static_cast<const i7m::PolicyKnots*>(knots);
  hipLaunchKernelGGL(i7m::k_sampled_multirate_policy_step, dim3(ng), dim3((H + 63) / 64 * 64), 0, s,
                     static_cast<const i7m::DevModel*>(model), a, kn, kbuf);
  return hipGetLastError();
}

// One workgroup per group: out (G, n_k, 96) from kbuf (G H, N - 1, KBUF_STRIDE), best (G) and xub
// (G, T), device pointers.
hipError_t i7m_launch_ctrl_policy_copy(int G, int H, int N, int n_k, hipStream_t s, const int* best, const double* kbuf,
                                       const double* xub, double* out) {
  hipLaunchKernelGGL(i7m::k_ctrl_policy_copy, dim3(G), dim3(256), 0, s, N, H, n_k, best, kbuf, xub, out);
  return hipGetLastError();
}
