// i7m_mpc_sampled.h — the sampled-wrench closed loop of the reference's external-force estimator
// (MPC_GATO_Batch_Sample.run_mpc, src/gato_mpc_batch_sample.py:106-300; GATO_Batch_Sample.
// find_best_idx / resample_f_ext_batch, gato_controller.py:109-129) on the device: G independent
// controllers ("groups") of H wrench hypotheses each, B = G H problem rows, group g owning rows
// [g H, (g + 1) H).  Per MPC step every row is solved with its own hypothesis wrench (i7m_api.hip
// run_sqp), and k_sampled_step, one launch between two solves, does the rest:
//
//   select(i-1)  XU_best[g] = XU_new[g H + best]; best and its wrench are recorded; the resample
//                rewrites the group's rows of the handle's wrench buffer in place
//                (gato_controller.py:120-129's order: rows = f_best; forces += noise; if keep_best
//                row[best] = f_best; torques = 0; row[0] = 0; rows *= decay)
//   plant(i)     x_last = xcur[g], u_last = XU_best[g][12:18]; xcur[g] = rk4(x_last, u_last,
//                sim_dt, f_actual) (:163-178)
//   score(i)     err_h = |rk4(x_last, u_last, sim_dt, wrench row h) - xcur[g]|_2, best = the lowest
//                index among the minima (:254-290; a NaN error never wins, all NaN -> 0)
//   spread       every row of g: xcur_row = xcur[g], XU_row = [xcur[g], XU_best[g][12:]] (:190-193)
//   goal         d = |fk(xcur q) - goal|; below 0.095 the next endpoint (not cyclic) or, at the last
//                one, the group stops (:203-217)
//
// With a reference trajectory (SampledArgs::ref, i7m_mpc_run_tracking: the deployed controller's
// loop, gato_controller.py:201-250) the goal phase is the other goal source:
//   goal         d = |fk(xcur q) - ref[min(ph + off, L - 1)]|, the tracking error the controller logs
//                (:242-246), and every row of the group gets the window ref[min(ph + off + k, L - 1)],
//                k = 0 .. N-1 (:214-216; held at the last point past the end); the group never stops
// ph = ref_phase[g] (or 0) and off, this step's offset, is a launch argument.  All lanes write the
// window with lane-contiguous columns, as the spread does; consecutive lanes read consecutive
// doubles of the reference (stride 3) or three of every six (stride 6).
//
// The score of step i needs only (x_last, u_last), the hypotheses and the plant's result, none of
// which the solve of step i changes, so it runs here, before that solve, and select(i) after the
// solve only takes row `best`: the same choice the reference makes after its solve (:231).
//
// Plant and score are ONE rk4_step call site run twice (a loop that is not unrolled): first every
// lane with the actual wrench, then lane h with hypothesis h.  A world-frame wrench is converted
// once at x_last's q by that same code in both (rk4_step, as i7m_rk4 does for I7M_WRENCH_WORLD),
// so a hypothesis equal to the actual wrench scores an error of exactly 0.
//
// Not reproduced from the reference (include/indy7_mpc.h says so too):
//   * the split of a plant step at a knot boundary (:170-187): with one rk4 step of sim_dt <= dt
//     per MPC step and no warm-start shift (the reference's is commented out, :194-201) the plant
//     never leaves knot 0;
//   * the random walk of the actual force (:244-250): the caller supplies its schedule.
#pragma once

#include "i7m_kernels.h"
#include "i7m_plan.h"

namespace i7m {

constexpr double SAMPLED_GOAL_RADIUS = 0.095;  // src/gato_mpc_batch_sample.py:208,215

// One launch's arguments; every pointer is already offset to the launch's first group / row, the
// history pointers also to the step they record.
struct SampledArgs {
  int N, H, n_endpoints;
  int select;       // 0: none (no solve yet); 1: take row best[g], record, resample; 2: take it only (initial solve)
  int plant;        // 1: plant, score, spread, goal
  int frame_world;  // the wrenches (hypotheses and actual) are world-frame
  int keep_best;
  double sim_dt, decay;
  // rows of the launch (ng H)
  double* xs;            // (rows, 12)
  double* XU;            // (rows, T) the solves' warm start
  const double* xu_new;  // (rows, T) the last solve's result
  double* goals;         // (rows, 3 N)
  double* fext;          // (rows, 6) the hypotheses (the handle's wrench buffer)
  // groups of the launch
  double* xcur;   // (ng, 12)
  double* xub;    // (ng, T) XU_best
  int* best;      // (ng) the scored hypothesis of the step in flight
  int* goal_idx;  // (ng)
  int* alive;     // (ng)
  const double* endpoints;  // (n_endpoints, 3)
  const double* f_actual;   // (ng, 6) this step's actual wrench (plant)
  const double* noise;      // (rows, 3) the resample's noise of the selected step, or null
  double* dist_out;         // (ng) plant step
  double* q_out;            // (ng, 6) plant step, or null
  int* best_out;            // (ng) selected step, or null
  double* fbest_out;        // (ng, 6) selected step, or null
  // the tracking goal source (ref != null; endpoints, goal_idx and n_endpoints are then unused)
  const double* ref;     // (L, ref_stride) the reference, the first three of each point read
  const int* ref_phase;  // (ng) or null (0)
  int L, ref_stride;
  int off;               // this step's window offset
  double* ee_out;        // (ng, 3) plant step: the EE position of the new state, or null
};

// (error, index) minimum over the wave, the lower index on a tie: xor butterfly, every lane ends
// with the result.
__device__ __forceinline__ void wave_argmin(double& e, int& i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double oe = __shfl_xor(e, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    if (oe < e || (oe == e && oi < i)) {
      e = oe;
      i = oi;
    }
  }
}

// ---- the pieces k_sampled_step and the controller step (i7m_ctrl.h) share: one workgroup per group,
// lane l of nt, every __syncthreads under a workgroup-uniform condition; the row pointers are
// already offset to the group's first row ------------------------------------------------------------

// select + resample: XU_best[g] = row b of the last solve; with `record`, fb = wrench row b, and with
// noise the group's wrench rows are rewritten in place in gato_controller.py:120-129's order.  The
// caller synchronises before anything reads XU_best or the rows.
__device__ __forceinline__ void select_resample(double* xub, const double* xu_new, double* fext, const double* noise,
                                                int b, int H, int T, int l, int nt, bool record, bool keep_best,
                                                double decay, double fb[6]) {
  const double* src = xu_new + (long)b * T;
  for (int e = l; e < T; e += nt) xub[e] = src[e];
  if (!record) return;
#pragma unroll
  for (int k = 0; k < 6; ++k) fb[k] = fext[b * 6 + k];
  if (noise) {
    __syncthreads();  // every lane has read row `best` before its lane rewrites it
    if (l < H) {
      double row[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) row[k] = fb[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) row[k] += noise[l * 3 + k];
      if (keep_best && l == b)
#pragma unroll
        for (int k = 0; k < 6; ++k) row[k] = fb[k];
#pragma unroll
      for (int k = 3; k < 6; ++k) row[k] = 0.0;
      if (l == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) row[k] = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) fext[l * 6 + k] = row[k] * decay;
    }
  }
}

// |[qo, vo] - xn|_2 over all 12 entries: a hypothesis's scoring error
__device__ __forceinline__ double state_err(const double qo[6], const double vo[6], const double xn[12]) {
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double dq = qo[k] - xn[k];
    ss += dq * dq;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double dv = vo[k] - xn[6 + k];
    ss += dv * dv;
  }
  return sqrt(ss);
}

// The group's argmin in two halves around the caller's __syncthreads: lane l's (err, l) reduced over
// its wave and parked (a NaN error and a lane past H never win), then lane 0 merges the waves into
// the winner: the lowest index among the minima, 0 if every error was NaN.
__device__ __forceinline__ void group_argmin_park(double& err, int& idx, int l, int H, double* s_err, int* s_idx) {
  const double inf = __builtin_inf();
  if (!(err < inf) || l >= H) err = inf;  // a NaN error never wins
  idx = l;
  wave_argmin(err, idx);
  if ((l & 63) == 0) {
    s_err[l >> 6] = err;
    s_idx[l >> 6] = idx;
  }
}
__device__ __forceinline__ int group_argmin_merge(double err, int idx, int nt, int H, const double* s_err,
                                                  const int* s_idx) {
  for (int w = 1; w < (nt >> 6); ++w)
    if (s_err[w] < err) {  // a later wave's indices are higher: it wins only if strictly lower
      err = s_err[w];
      idx = s_idx[w];
    }
  return idx < H ? idx : 0;
}

// spread: every row of the group gets xs = s_x and XU = [s_x, XU_best[12:]]; lane-contiguous
// columns, one load and H stores per column
__device__ __forceinline__ void spread_rows(double* XU, double* xs, const double* xub, const double* s_x, int H, int T,
                                            int l, int nt) {
  for (int e = l; e < T; e += nt) {
    const double v = e < 12 ? s_x[e] : xub[e];
    for (int hh = 0; hh < H; ++hh) XU[(long)hh * T + e] = v;
  }
  for (int e = l; e < 12 * H; e += nt) xs[e] = s_x[e % 12];
}

// spread_rows with the warm start shifted by sh = 18 s entries (s knots completed, the multi-rate
// loops' shift_warm_start): XU[e] = XU_best[e + sh] for 12 <= e < T - sh, the tail keeps XU_best[e]
__device__ __forceinline__ void spread_rows_shifted(double* XU, double* xs, const double* xub, const double* s_x, int H,
                                                    int T, int sh, int l, int nt) {
  for (int e = l; e < T; e += nt) {
    const double v = e < 12 ? s_x[e] : (e < T - sh ? xub[e + sh] : xub[e]);
    for (int hh = 0; hh < H; ++hh) XU[(long)hh * T + e] = v;
  }
  for (int e = l; e < 12 * H; e += nt) xs[e] = s_x[e % 12];
}

// the window: one load per column (knot e / 3, coordinate e % 3) and H stores
__device__ __forceinline__ void window_rows(double* goals, const double* ref, long ph, long off, int L, int ref_stride,
                                            int N, int H, int l, int nt) {
  for (int e = l; e < 3 * N; e += nt) {
    const double v = ref[track_index(ph, off, e / 3, L) * ref_stride + e % 3];
    for (int hh = 0; hh < H; ++hh) goals[(long)hh * 3 * N + e] = v;
  }
}

// ---- the pieces k_sampled_step and k_sampled_multirate_step (i7m_mpc_sampled_multirate.h) share:
// all but the plant and score pass between sampled_select and sampled_finish.  g the group, r0 its
// first row, xub its XU_best, track / ph the launch's goal source and the group's phase: loaded once
// by the kernel and passed in -------------------------------------------------------------------------

// a stopped group's records: NaN / -1 from the step after its stop on (the kernel then returns)
__device__ __forceinline__ void sampled_stopped(const SampledArgs& A, int g, int l) {
  const double nan = __builtin_nan("");
  if (A.select == 1) {
    if (A.best_out && l == 0) A.best_out[g] = -1;
    if (A.fbest_out && l < 6) A.fbest_out[6L * g + l] = nan;
  }
  if (A.plant) {
    if (l == 0) A.dist_out[g] = nan;
    if (A.q_out && l < 6) A.q_out[6L * g + l] = nan;
  }
}

// select(i - 1): select_resample of the scored row, recorded with its wrench, and the barrier
// before the plant and the score read XU_best and the resampled rows
__device__ __forceinline__ void sampled_select(const SampledArgs& A, int g, int l, int nt, long r0, double* xub) {
  if (!A.select) return;
  const int H = A.H, T = 18 * A.N - 6;
  const int b = A.best[g];
  double fb[6];
  select_resample(xub, A.xu_new + r0 * T, A.fext + r0 * 6, A.noise ? A.noise + r0 * 3 : nullptr, b, H, T, l, nt,
                  A.select == 1, A.keep_best != 0, A.decay, fb);
  if (A.select == 1 && l == 0) {
    if (A.best_out) A.best_out[g] = b;
    if (A.fbest_out)
#pragma unroll
      for (int k = 0; k < 6; ++k) A.fbest_out[6L * g + k] = fb[k];
  }
  __syncthreads();  // XU_best and the resampled rows are the plant's and the score's inputs
}

// The step after the plant and the score (every lane holds the new state xn, lane l its error err):
// the group's argmin into best[g]; the goal distance of the new state, the endpoint switch or the
// stop; xcur / q_out; the spread (warm start shifted by sh entries, 0: none); the window or the new
// endpoint re-tiled.
__device__ __forceinline__ void sampled_finish(const DevModel& M, const SampledArgs& A, int g, int l, int nt, long r0,
                                               const double* xub, bool track, long ph, int sh, double err,
                                               const double xn[12]) {
  __shared__ double s_x[12], s_err[4];
  __shared__ int s_idx[4], s_switch;
  const int H = A.H, N = A.N, T = 18 * N - 6;
  int idx;
  group_argmin_park(err, idx, l, H, s_err, s_idx);
  if (l == 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) s_x[k] = xn[k];
  }
  __syncthreads();
  if (l == 0) {
    A.best[g] = group_argmin_merge(err, idx, nt, H, s_err, s_idx);
    // the goal of the new state (src/gato_mpc_batch_sample.py:203-217), or the window's first point
    double c[6], s[6], p[3];
    sincos6(xn, c, s);
    fk_pos(M, c, s, p);
    const double* gl = track ? A.ref + track_index(ph, A.off, 0, A.L) * A.ref_stride : A.goals + r0 * 3 * N;
    const double e0 = p[0] - gl[0], e1 = p[1] - gl[1], e2 = p[2] - gl[2];
    const double d = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    A.dist_out[g] = d;
    if (A.ee_out)
#pragma unroll
      for (int k = 0; k < 3; ++k) A.ee_out[3L * g + k] = p[k];
    int sw = -1;
    if (!track && d < SAMPLED_GOAL_RADIUS) {
      if (A.goal_idx[g] < A.n_endpoints - 1) {
        sw = A.goal_idx[g] + 1;
        A.goal_idx[g] = sw;
      } else {
        A.alive[g] = 0;
      }
    }
    s_switch = sw;
  }
  if (l < 12) A.xcur[12L * g + l] = s_x[l];
  if (A.q_out && l < 6) A.q_out[6L * g + l] = s_x[l];
  if (sh > 0)
    spread_rows_shifted(A.XU + r0 * T, A.xs + r0 * 12, xub, s_x, H, T, sh, l, nt);
  else
    spread_rows(A.XU + r0 * T, A.xs + r0 * 12, xub, s_x, H, T, l, nt);
  __syncthreads();
  const int sw = s_switch;
  if (track) {
    window_rows(A.goals + r0 * 3 * N, A.ref, ph, A.off, A.L, A.ref_stride, N, H, l, nt);
  } else if (sw >= 0) {
    double* gl = A.goals + r0 * 3 * N;
    for (int e = l; e < 3 * N * H; e += nt) gl[e] = A.endpoints[3 * sw + e % 3];
  }
}

// One workgroup per group, one lane per hypothesis (H lanes rounded up to whole waves, <= 4 waves).
__global__ void __launch_bounds__(256) k_sampled_step(const DevModel* __restrict__ Mg, const SampledArgs A) {
  const int g = blockIdx.x, l = threadIdx.x, nt = blockDim.x;
  const int H = A.H, T = 18 * A.N - 6;
  if (!A.alive[g]) {
    sampled_stopped(A, g, l);
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
  const int h = l < H ? l : H - 1;  // lanes past H repeat the last row; their error is dropped
#pragma nounroll
  for (int pass = 0; pass < 2; ++pass) {
    const double* fp = pass == 0 ? A.f_actual + 6L * g : A.fext + (r0 + h) * 6;
    double f6[6], qo[6], vo[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) f6[k] = fp[k];
    rk4_step(*Mg, xl, xl + 6, u, A.sim_dt, f6, A.frame_world != 0, qo, vo);
    if (pass == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        xn[k] = qo[k];
        xn[6 + k] = vo[k];
      }
    } else {
      err = state_err(qo, vo, xn);
    }
  }
  sampled_finish(*Mg, A, g, l, nt, r0, xub, track, ph, 0, err, xn);
}

}  // namespace i7m
