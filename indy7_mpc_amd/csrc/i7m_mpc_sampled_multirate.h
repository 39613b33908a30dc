// i7m_mpc_sampled_multirate.h — the sampled-wrench closed loops (i7m_mpc_sampled.h) with the
// multi-rate plant of i7m_mpc_multirate.h: MPC_GATO_Batch_Sample.run_mpc's inner while-loop
// (src/gato_mpc_batch_sample.py:163-193) and run_mpc_fig8 of notebooks/gato_mpc_indy7_fig8.ipynb,
// which steps the plant 0.02 s per solve against 10 ms knots.  G groups of H hypotheses, one launch
// of k_sampled_multirate_step between two solves, in k_sampled_step's order:
//
//   select(i-1)  select_resample, as k_sampled_step
//   plant(i)     x_last = xcur[g], u_last = XU_best[g][12:18] (recorded: u_out); the actual wrench is
//                converted to joint 6's frame ONCE, at x_last's q (:151-161), and held over the
//                step's sub-steps; xcur[g] = rk4(..., sub_dt[s]) for s = 0 .. n_sub-1, every one
//                driven by u_last (the reference's current_knot is always 0); xpath_out[s] = q
//   score(i)     err_h = |rk4(x_last, u_last, sim_dt, wrench row h) - xcur[g]|_2: ONE step of the whole
//                sim_dt (:284), the hypothesis converted at x_last's q; argmin as k_sampled_step
//   spread       every row of g: xs = xcur[g], XU = [xcur[g], XU_best[g][12:]]; with shift_warm_start
//                and s > 0 knots completed XU[e] = XU_best[g][e + 18 s] for 12 <= e < T - 18 s, the
//                tail keeps XU_best[g][e] (src/gato_mpc_batch.py:202-203); no terminal pin
//   goal / track as k_sampled_step; the tracking offset (the knots completed so far) is the host's
//
// The sub-step lengths are the host's (multirate_schedule, i7m_plan.h): a device array whose length
// is a launch argument, clamped to MULTIRATE_MAX_SUB, so the loop is bounded and the kernel does no
// schedule arithmetic.
//
// The two wrench conversions are ONE wrench_world_to_local call site (a loop of two passes that is
// not unrolled: the actual wrench, then lane h's hypothesis), and the plant's sub-steps and the
// score are ONE rk4_step call site in a loop that is not unrolled (n_sub plant passes, then the
// score).  On a step with one sub-step (sub_dt[0] == sim_dt) a hypothesis equal to the actual wrench
// therefore runs the same instructions on the same inputs twice and scores exactly 0, as in
// k_sampled_step.  On a step with several sub-steps the true hypothesis scores small but not 0:
// the plant took several steps, the score takes one.  That is the reference's behaviour.
//
// Not reproduced from the reference (include/indy7_mpc.h says so too): the random walk of the
// actual force (:244-250), the notebook's use of the world force as a local one, np.random's global
// draw order.
#pragma once

#include "i7m_mpc_sampled.h"

namespace i7m {

// One launch's arguments: k_sampled_step's (same meanings, same offsets), then the multi-rate part.
struct SampledMultirateArgs {
  SampledArgs S;
  int n_sub;             // this step's plant sub-steps (multirate_schedule)
  int shift;             // 18-entry knots the spread shifts the warm start by (0: none)
  long hist_stride;      // groups of the whole run: xpath_out's sub-step s is at s * 6 * hist_stride
  const double* sub_dt;  // (n_sub) this step's rk4 step lengths
  double* u_out;         // (ng, 6) plant step: u_last
  double* xpath_out;     // (n_sub, hist_stride, 6), this launch's groups from column 0, or null
};

#ifdef I7M_SAMPLED_MULTIRATE_KERNEL  // (i7m_mpc_sampled_multirate_tu.hip: the kernel lives in that unit alone)

// One workgroup per group, one lane per hypothesis (H lanes rounded up to whole waves, <= 4 waves).
__global__ void __launch_bounds__(256) k_sampled_multirate_step(const DevModel* __restrict__ Mg,
                                                                const SampledMultirateArgs M) {
  const SampledArgs& A = M.S;
  const int g = blockIdx.x, l = threadIdx.x, nt = blockDim.x;
  const int H = A.H, T = 18 * A.N - 6;
  const int ns = M.n_sub < MULTIRATE_MAX_SUB ? M.n_sub : MULTIRATE_MAX_SUB;  // the loops' bound
  if (!A.alive[g]) {  // a stopped group: its u and path are NaN too
    sampled_stopped(A, g, l);
    if (A.plant && l < 6) {
      const double nan = __builtin_nan("");
      M.u_out[6L * g + l] = nan;
      if (M.xpath_out)
        for (int s = 0; s < ns; ++s) M.xpath_out[((long)s * M.hist_stride + g) * 6 + l] = nan;
    }
    return;
  }
  const long r0 = (long)g * H;
  double* xub = A.xub + (long)g * T;
  const bool track = A.ref != nullptr;  // wave-uniform: the goal source of the launch
  const long ph = track && A.ref_phase ? A.ref_phase[g] : 0;
  sampled_select(A, g, l, nt, r0, xub);
  if (!A.plant) return;

  double xl[12], u[6], xn[12], err = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) xl[k] = A.xcur[12L * g + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) u[k] = xub[12 + k];
  if (l < 6) M.u_out[6L * g + l] = u[l];
  const int h = l < H ? l : H - 1;  // lanes past H repeat the last row; their error is dropped
  // the wrenches in joint 6's frame at x_last's q: the actual one, then lane h's hypothesis
  double fa[6], fh[6];
  {
    double c[6], s[6];
    sincos6(xl, c, s);
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
      const double* fp = pass == 0 ? A.f_actual + 6L * g : A.fext + (r0 + h) * 6;
      double f6[6], fo[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) f6[k] = fp[k];
      if (A.frame_world) {
        wrench_world_to_local(*Mg, c, s, f6, fo);
#pragma unroll
        for (int k = 0; k < 6; ++k) f6[k] = fo[k];
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (pass == 0) fa[k] = f6[k];
        fh[k] = f6[k];  // the second pass's stays
      }
    }
  }
  // every lane runs the plant (the same arithmetic: the lanes agree bit for bit), then its score
#pragma unroll
  for (int k = 0; k < 12; ++k) xn[k] = xl[k];
#pragma nounroll
  for (int k = 0; k <= ns; ++k) {
    const bool sc = k == ns;  // the last pass scores: one step of the whole sim_dt from x_last
    double xi[12], f6[6], qo[6], vo[6];
#pragma unroll
    for (int r = 0; r < 12; ++r) xi[r] = sc ? xl[r] : xn[r];
#pragma unroll
    for (int r = 0; r < 6; ++r) f6[r] = sc ? fh[r] : fa[r];
    const double ts = sc ? A.sim_dt : M.sub_dt[k];
    rk4_step(*Mg, xi, xi + 6, u, ts, f6, false, qo, vo);
    if (sc) {
      err = state_err(qo, vo, xn);
    } else {
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        xn[r] = qo[r];
        xn[6 + r] = vo[r];
      }
      if (l == 0 && M.xpath_out) {  // one lane stores the path
        double* xp = M.xpath_out + ((long)k * M.hist_stride + g) * 6;
#pragma unroll
        for (int r = 0; r < 6; ++r) xp[r] = qo[r];
      }
    }
  }
  sampled_finish(*Mg, A, g, l, nt, r0, xub, track, ph, 18 * M.shift, err, xn);
}

#endif  // I7M_SAMPLED_MULTIRATE_KERNEL

}  // namespace i7m
