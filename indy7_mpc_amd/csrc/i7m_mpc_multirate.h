// i7m_mpc_multirate.h — the multi-rate closed loops of the reference (MPC_GATO_Batch.run_mpc,
// src/gato_mpc_batch.py:76-217; MPC_GATO.run_mpc, src/gato_mpc.py:53-150) for B independent
// instances on the device: the plant advances sim_dt per solve against a knot grid of dt, a time
// accumulator carries the position inside the current knot from one MPC step to the next, a plant
// step is split where it crosses a knot boundary, and the warm start is shifted only when a knot
// completes, by as many knots as completed.  Per MPC step the batched SQP solve (i7m_api.hip
// run_sqp) and then k_mpc_multirate_step, ONE launch in the place of i7m_mpc.h's goal and advance
// kernels: the reference tests the goal after the solve (:146-168 / :94-115).
//
// The split of a step's plant time is the host's (multirate_schedule, i7m_plan.h): it depends on
// dt, sim_dt and the step index alone, so the kernel's sub-step loop runs over a list whose length
// is a launch argument.  The reference's current_interval (:179 / :125) is always 0 (the accumulator
// is reset at every boundary), so every sub-step is driven by knot 0's control: of the NEW trajectory
// in MPC_GATO_Batch (:185), of the PREVIOUS one in MPC_GATO (:126).
//
// Deliberately not reproduced (include/indy7_mpc.h says so too): src/gato_mpc_batch.py:213 with
// sim_steps == 0, whose slice `:-(0) or len(XU_batch)` ends at batch_size and overwrites the first
// batch_size warm-start entries of every row with row 0's (q_0[0] among them: the rows are
// identical there, so only entries 0 .. batch_size - 1 of an unshifted warm start would be touched,
// and :206 / :212 have just set them).  With no knot completed the warm start here stays the
// older trajectory apart from the pins, as :202-207 leave it.
#pragma once

#include "i7m_kernels.h"

namespace i7m {

// One launch's arguments; the instance pointers are already offset to the launch's first instance,
// the history pointers also to the step (xpath_out: to the step's first sub-step).
struct MultirateArgs {
  int N, n_endpoints;
  int n_sub;         // this step's plant sub-steps (multirate_schedule)
  int shift;         // knots this step completes
  int control_prev;  // 1: the plant's control is XU's (MPC_GATO), 0: xu_new's (MPC_GATO_Batch)
  long hist_stride;  // instances of the whole batch: xpath_out's sub-step s is at s * 6 * hist_stride
  double radius;
  const double* sub_dt;  // (n_sub) this step's rk4 step lengths
  double* xs;            // (n, 12)
  double* XU;            // (n, T) the warm start
  const double* xu_new;  // (n, T) this step's solve
  double* goals;         // (n, 3 N)
  const double* endpoints;
  int* goal_idx;
  int* alive;
  double* dist_out;   // (n)
  double* q_out;      // (n, 6)
  double* u_out;      // (n, 6)
  double* xpath_out;  // (n_sub, hist_stride, 6), this launch's instances from column 0
};

#ifdef I7M_MULTIRATE_KERNEL  // (i7m_mpc_multirate_tu.hip: the kernel lives in that unit alone)

// One wave per instance, in the reference's order after the solve (src/gato_mpc_batch.py:146-214):
//   distance   d = |fk(xcur q) - goal|, recorded; u_out = XU[12:18], the warm start's first control
//              before this step's update, which the reference logs as control_inputs (:153)
//   goal       d < radius: the next endpoint (not cyclic, the goal rows re-tiled), or at the last
//              one the instance stops here, before the plant: its q and xpath slots of this step
//              are NaN, as are all its slots of later steps
//   plant      lane 0: xcur = rk4(xcur, u, sub_dt[s]) for each sub-step, no wrench, u = knot 0's
//              control read before the shift overwrites it; xpath_out[s] = q
//   shift      s = shift > 0: XU[:T - 18 s] = xu_new[18 s:], the tail keeps its old values (:202-203);
//              s = 0: XU stays the older trajectory
//   pins       XU[:12] = xcur, XU[-12:] = [1]*6 + [0]*6 (:206-207)
__global__ void __launch_bounds__(64) k_mpc_multirate_step(const DevModel* __restrict__ Mg, int n, const MultirateArgs A) {
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= n) return;
  const int N = A.N, T = 18 * N - 6;
  const double nan = __builtin_nan("");
  const auto nan_path = [&]() {  // this step's q and xpath slots
    if (l < 6) {
      A.q_out[6L * b + l] = nan;
      for (int s = 0; s < A.n_sub; ++s) A.xpath_out[((long)s * A.hist_stride + b) * 6 + l] = nan;
    }
  };
  if (!A.alive[b]) {
    if (l == 0) A.dist_out[b] = nan;
    if (l < 6) A.u_out[6L * b + l] = nan;
    nan_path();
    return;
  }
  __shared__ double xn[12];
  __shared__ int s_switch, s_stop;
  double* X = A.XU + (long)b * T;
  const double* Xn = A.xu_new + (long)b * T;
  double* x = A.xs + 12L * b;
  double* g = A.goals + (long)b * 3 * N;
  if (l < 6) A.u_out[6L * b + l] = X[12 + l];
  if (l == 0) {
    double q[6], v[6], u[6], qo[6], vo[6], c[6], s[6], p[3];
    for (int r = 0; r < 6; ++r) {
      q[r] = x[r];
      v[r] = x[6 + r];
    }
    sincos6(q, c, s);
    fk_pos(*Mg, c, s, p);
    const double e0 = p[0] - g[0], e1 = p[1] - g[1], e2 = p[2] - g[2];
    const double d = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    A.dist_out[b] = d;
    int sw = -1, stop = 0;
    if (d < A.radius) {
      if (A.goal_idx[b] < A.n_endpoints - 1) {
        sw = A.goal_idx[b] + 1;
        A.goal_idx[b] = sw;
      } else {
        A.alive[b] = 0;
        stop = 1;
      }
    }
    s_switch = sw;
    s_stop = stop;
    if (!stop) {
      const double* up = (A.control_prev ? X : Xn) + 12;
      for (int r = 0; r < 6; ++r) u[r] = up[r];
#pragma nounroll
      for (int k = 0; k < A.n_sub; ++k) {
        rk4_step(*Mg, q, v, u, A.sub_dt[k], nullptr, false, qo, vo);
        double* xp = A.xpath_out + ((long)k * A.hist_stride + b) * 6;
        for (int r = 0; r < 6; ++r) {
          q[r] = qo[r];
          v[r] = vo[r];
          xp[r] = qo[r];
        }
      }
      for (int r = 0; r < 6; ++r) {
        xn[r] = q[r];
        xn[6 + r] = v[r];
      }
    }
  }
  __syncthreads();  // the controls X[12:18] are read (u_out, the plant) before the shift overwrites them
  if (s_stop) {
    nan_path();
    return;
  }
  const int sw = s_switch;
  if (sw >= 0)
    for (int e = l; e < 3 * N; e += 64) g[e] = A.endpoints[3 * sw + e % 3];
  const int sh = 18 * A.shift;
  if (sh > 0)
    for (int e = l; e < T - sh; e += 64) X[e] = Xn[e + sh];
  __syncthreads();
  if (l < 12) {
    x[l] = xn[l];
    X[l] = xn[l];
    X[T - 12 + l] = l < 6 ? 1.0 : 0.0;
  }
  if (l < 6) A.q_out[6L * b + l] = xn[l];
}

#endif  // I7M_MULTIRATE_KERNEL

}  // namespace i7m
