// i7m_ctrl.h — one controller step on a measured state: the deployed controller's joint_callback
// (GATO_Controller.joint_callback, gato_controller.py:201-250) for G controllers of H wrench
// hypotheses, group g owning rows [g H, (g + 1) H), with the plant outside the device.  The state
// arrives from the caller (i7m_ctrl_step); around that step's solve (i7m_api.hip run_sqp) run two
// launches, one workgroup per group and one lane per hypothesis (H lanes rounded up to whole waves,
// <= 4 waves), as k_sampled_step:
//
//   k_ctrl_measure, before the solve (the scoring uses no result of the solve, as in
//   i7m_mpc_sampled.h):
//     score    err_h = |rk4(x_last, u_last, elapsed, wrench row h) - x_meas[g]|_2, best = the lowest
//              index among the minima (a NaN error never wins, all NaN -> 0); without an x_last
//              yet (the controller's constructor form, :205-206) x_last = x_meas, u_last = 0
//     spread   every row of g: xs = x_meas[g], XU = [x_meas[g], XU_best[g][12:]] (:217-218,249)
//     window   every row of g: goals[k] = ref[min(ph_g + off + k, L - 1)][0:3] (:214-216)
//     track    ee = fk(x_meas q), err = |ee - window[0]| (:242), into the group's record
//   k_ctrl_select, after it:
//     select   XU_best[g] = XU_new[g H + best]; u, best and the winning wrench into the record
//     resample with noise only, gato_controller.py:120-129's order (select_resample)
//     remember x_last = x_meas, u_last = u (:250)
//
// The record (CTRL_REC doubles per group, i7m_plan.h) is what a step copies back, in one copy.
// The select / resample, argmin, spread and window code is k_sampled_step's (i7m_mpc_sampled.h).
#pragma once

#include "i7m_mpc_sampled.h"

namespace i7m {

// Both launches' arguments; every pointer is the session's (group 0 / row 0).
struct CtrlArgs {
  int N, H;
  int frame_world;  // the hypotheses are world-frame wrenches
  int keep_best;
  int have_last;    // measure: x_last / u_last are set (else x_last = x_meas, u_last = 0)
  int initial;      // select: i7m_ctrl_begin's (row 0, no resample; x_meas may be null: no x_last yet)
  double elapsed, decay;
  // rows (G H)
  double* xs;            // (rows, 12)
  double* XU;            // (rows, T) the solve's warm start
  const double* xu_new;  // (rows, T) the solve's result
  double* goals;         // (rows, 3 N)
  double* fext;          // (rows, 6) the hypotheses (the handle's wrench buffer)
  const double* noise;   // (rows, 3) or null: no resampling this step
  // groups (G)
  const double* x_meas;  // (G, 12)
  double* x_last;        // (G, 12)
  double* u_last;        // (G, 6)
  double* xub;           // (G, T) XU_best
  int* best;             // (G) the scored hypothesis of the step in flight
  double* rec;           // (G, CTRL_REC)
  const double* ref;     // (L, ref_stride)
  const int* ref_phase;  // (G) or null (0)
  int L, ref_stride;
  int off;               // this step's window offset
};

__global__ void __launch_bounds__(256) k_ctrl_measure(const DevModel* __restrict__ Mg, const CtrlArgs A) {
  const int g = blockIdx.x, l = threadIdx.x, nt = blockDim.x;
  const int H = A.H, N = A.N, T = 18 * N - 6;
  __shared__ double s_x[12], s_err[4];
  __shared__ int s_idx[4];
  const long r0 = (long)g * H;
  const double* xub = A.xub + (long)g * T;
  const long ph = A.ref_phase ? A.ref_phase[g] : 0;

  double xm[12], xl[12], u[6];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    xm[k] = A.x_meas[12L * g + k];
    xl[k] = A.have_last ? A.x_last[12L * g + k] : xm[k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) u[k] = A.have_last ? A.u_last[6L * g + k] : 0.0;
  const int h = l < H ? l : H - 1;  // lanes past H repeat the last row; their error is dropped
  double f6[6], qo[6], vo[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) f6[k] = A.fext[(r0 + h) * 6 + k];
  rk4_step(*Mg, xl, xl + 6, u, A.elapsed, f6, A.frame_world != 0, qo, vo);
  double err = state_err(qo, vo, xm);
  int idx;
  group_argmin_park(err, idx, l, H, s_err, s_idx);
  if (l < 12) s_x[l] = A.x_meas[12L * g + l];
  __syncthreads();
  if (l == 0) {
    A.best[g] = group_argmin_merge(err, idx, nt, H, s_err, s_idx);
    // the tracking error of the measured state against the window's first point
    double c[6], s[6], p[3];
    sincos6(xm, c, s);
    fk_pos(*Mg, c, s, p);
    const double* gl = A.ref + track_index(ph, A.off, 0, A.L) * A.ref_stride;
    const double e0 = p[0] - gl[0], e1 = p[1] - gl[1], e2 = p[2] - gl[2];
    double* rec = A.rec + (long)g * CTRL_REC;
    rec[CREC_ERR] = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
#pragma unroll
    for (int k = 0; k < 3; ++k) rec[CREC_EE + k] = p[k];
  }
  spread_rows(A.XU + r0 * T, A.xs + r0 * 12, xub, s_x, H, T, l, nt);
  window_rows(A.goals + r0 * 3 * N, A.ref, ph, A.off, A.L, A.ref_stride, N, H, l, nt);
}

__global__ void __launch_bounds__(256) k_ctrl_select(const CtrlArgs A) {
  const int g = blockIdx.x, l = threadIdx.x, nt = blockDim.x;
  const int H = A.H, T = 18 * A.N - 6;
  const long r0 = (long)g * H;
  double* xub = A.xub + (long)g * T;
  double* rec = A.rec + (long)g * CTRL_REC;
  const int b = A.initial ? 0 : A.best[g];
  double fb[6];
  select_resample(xub, A.xu_new + r0 * T, A.fext + r0 * 6, A.noise ? A.noise + r0 * 3 : nullptr, b, H, T, l, nt, true,
                  A.keep_best != 0, A.decay, fb);
  if (l == 0) {
    rec[CREC_BEST] = (double)b;
#pragma unroll
    for (int k = 0; k < 6; ++k) rec[CREC_FBEST + k] = fb[k];
  }
  __syncthreads();  // XU_best is whole: its control is the step's result
  if (l < 6) {
    const double u = xub[12 + l];
    rec[CREC_U + l] = u;
    A.u_last[6L * g + l] = u;
  }
  if (A.x_meas && l < 12) A.x_last[12L * g + l] = A.x_meas[12L * g + l];
}

}  // namespace i7m
