// i7m_mpc_sampled_policy.h — the multi-rate sampled-wrench loops (i7m_mpc_sampled_multirate.h) with
// the plant under the feedback policy of the step's solve (I7M_CONTROL_POLICY), and the controller
// session's copy of the winner's policy.
//
// k_sampled_multirate_policy_step is k_sampled_multirate_step with select, resample, spread, goal,
// track, stop and the NaN / -1 layout taken from the shared pieces (sampled_select, sampled_finish,
// sampled_stopped, i7m_mpc_sampled.h) as they are.  The plant and the score differ:
//
//   plant(i)     sub-step s begins at plant state x with j = KN.j[s] knots of this step completed
//                (multirate_schedule's sub_knot) and is driven by
//                    u_s = XU_best[g].u_j + K_j (x - XU_best[g].x_j),
//                K_j the 6 x 12 gain of stage j in kbuf at row g H + best[g]: the row this launch's
//                select takes (row 0 after the initial solve).  The policy pass runs behind the solve
//                and before this launch, so it saw the wrenches the solve used on every row; the
//                resample of the select step rewrites them only now.  u_out stays XU_best[g][12:18],
//                the nominal first control; the actual wrench is converted once at x_last's q.
//   score(i)     the torque varies within the step, so one rk4 step of sim_dt under u_last no longer
//                predicts what was applied.  Hypothesis h replays the step: from x_last the same
//                sub-steps of the same lengths under the RECORDED controls u_s (the plant's, not
//                recomputed from the replayed state), wrench row h converted once at x_last's q;
//                err_h = |replay - xcur[g]|_2.
//
// K_j dx is formed as in k_mpc_multirate_policy_step (i7m_mpc_policy.h): lane 8 r + c of each wave
// holds t_c = K[r][c] dx[c] (+ K[r][c + 8] dx[c + 8] for c < 4), products and sums rounded on their
// own, and three plain shuffles give du[r] = ((t0 + t4) + (t2 + t6)) + ((t1 + t5) + (t3 + t7)).  Every
// lane of the workgroup carries the same plant state, so each of the up to four waves forms the same
// du for itself.
//
// Plant and replay are ONE rk4_step call site in ONE loop that is not unrolled: n_sub plant passes
// that park u_s in LDS (at most 66 x 6 doubles), a barrier, then n_sub replay passes that read them
// back (x_last is read again from xcur[g]).  One state is live at a time, beside the plant's end.
// A hypothesis equal to the actual wrench therefore runs the same instructions on the same inputs
// and scores exactly 0 on every step, multi-sub-step steps included.
#pragma once

#include "i7m_mpc_policy.h"
#include "i7m_mpc_sampled_multirate.h"

namespace i7m {

constexpr int CTRL_POLICY_REC = 96;  // doubles per group and stage of the session's policy buffer: K~ (78), then [x_k, u_k] (18)

#ifdef I7M_SAMPLED_POLICY_KERNELS  // (i7m_mpc_sampled_policy_tu.hip: the kernels live in that unit alone)

// One workgroup per group, one lane per hypothesis (H lanes rounded up to whole waves, <= 4 waves).
// kbuf: the gains of the launch's first row (N - 1 slots of KBUF_STRIDE per row).
__global__ void __launch_bounds__(256) k_sampled_multirate_policy_step(const DevModel* __restrict__ Mg,
                                                                       const SampledMultirateArgs M, const PolicyKnots KN,
                                                                       const double* __restrict__ kbuf) {
  const SampledArgs& A = M.S;
  const int g = blockIdx.x, l = threadIdx.x, nt = blockDim.x;
  const int H = A.H, N = A.N, T = 18 * N - 6;
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
  __shared__ double s_u[MULTIRATE_MAX_SUB * 6];
  const long r0 = (long)g * H;
  double* xub = A.xub + (long)g * T;
  const bool track = A.ref != nullptr;  // wave-uniform: the goal source of the launch
  const long ph = track && A.ref_phase ? A.ref_phase[g] : 0;
  // the selected row's gains: best[g] is the select's row until sampled_finish stores the new one
  const double* KB = kbuf + (r0 + A.best[g]) * (N - 1) * KBUF_STRIDE;
  sampled_select(A, g, l, nt, r0, xub);
  if (!A.plant) return;

  double xn[12], xf[12], err = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) xn[k] = xf[k] = A.xcur[12L * g + k];
  if (l < 6) M.u_out[6L * g + l] = xub[12 + l];
  const int h = l < H ? l : H - 1;  // lanes past H repeat the last row; their error is dropped
  // the wrenches in joint 6's frame at x_last's q: the actual one, then lane h's hypothesis
  double fa[6], fh[6];
  {
    double c[6], s[6];
    sincos6(xn, c, s);
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
  // every lane runs the plant (the same arithmetic: the lanes agree bit for bit), then its replay
  const int wl = l & 63, row = wl >> 3, c0 = wl & 7;
#pragma nounroll
  for (int k = 0; k < 2 * ns; ++k) {
    const bool rp = k >= ns;  // the replay passes
    const int sb = rp ? k - ns : k;
    if (k == ns) {  // workgroup-uniform: the plant is done, its controls are parked
#pragma unroll
      for (int r = 0; r < 12; ++r) {
        xf[r] = xn[r];
        xn[r] = A.xcur[12L * g + r];  // x_last again (sampled_finish stores the new state later)
      }
      __syncthreads();
    }
    double u[6], f6[6], qo[6], vo[6];
    if (!rp) {
      const int j = KN.j[sb];
      double p = 0.0;
      {
#pragma clang fp contract(off)
        // x[c0] and x[c0 + 8] of this lane's copy (selects: no dynamic register index)
        double xa = xn[0], xb = xn[8];
        for (int c = 1; c < 8; ++c) xa = c0 == c ? xn[c] : xa;
        for (int c = 1; c < 4; ++c) xb = c0 == c ? xn[8 + c] : xb;
        if (wl < 48) {
          const double* Kr = KB + (long)j * KBUF_STRIDE + 13 * row;
          const double* xj = xub + 18 * j;
          p = Kr[c0] * (xa - xj[c0]);
          if (c0 < 4) p = p + Kr[c0 + 8] * (xb - xj[c0 + 8]);
        }
        p += __shfl_xor(p, 4, 8);
        p += __shfl_xor(p, 2, 8);
        p += __shfl_xor(p, 1, 8);
#pragma unroll
        for (int r = 0; r < 6; ++r) u[r] = xub[18 * j + 12 + r] + __shfl(p, 8 * r);
      }
      if (l < 6) {  // one lane per entry parks the control
        double us = u[0];
        for (int r = 1; r < 6; ++r) us = l == r ? u[r] : us;
        s_u[6 * sb + l] = us;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 6; ++r) u[r] = s_u[6 * sb + r];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) f6[r] = rp ? fh[r] : fa[r];
    rk4_step(*Mg, xn, xn + 6, u, M.sub_dt[sb], f6, false, qo, vo);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      xn[r] = qo[r];
      xn[6 + r] = vo[r];
    }
    if (!rp && l == 0 && M.xpath_out) {  // one lane stores the path
      double* xp = M.xpath_out + ((long)sb * M.hist_stride + g) * 6;
#pragma unroll
      for (int r = 0; r < 6; ++r) xp[r] = qo[r];
    }
  }
  // xn: the replay's end (lane h's hypothesis), xf: the plant's
  if (ns > 0) err = state_err(xn, xn + 6, xf);
  sampled_finish(*Mg, A, g, l, nt, r0, xub, track, ph, 18 * M.shift, err, xf);
}

// The controller session's policy (i7m_ctrl_set_policy): out[g, k, 0:78] = K~_k of row g H + best[g]
// (kbuf's slot, its first 78 doubles) and out[g, k, 78:96] = XU_best[g][18 k : 18 k + 18] for k < n_k
// <= N - 1.  One workgroup per group; consecutive threads read and write consecutive doubles.
__global__ void __launch_bounds__(256) k_ctrl_policy_copy(int N, int H, int n_k, const int* __restrict__ best,
                                                          const double* __restrict__ kbuf, const double* __restrict__ xub,
                                                          double* __restrict__ out) {
  const long g = blockIdx.x;
  const int T = 18 * N - 6;
  const double* KB = kbuf + (g * H + best[g]) * (N - 1) * KBUF_STRIDE;
  const double* X = xub + g * T;
  double* o = out + g * n_k * CTRL_POLICY_REC;
  for (int e = threadIdx.x; e < n_k * CTRL_POLICY_REC; e += 256) {
    const int k = e / CTRL_POLICY_REC, i = e - k * CTRL_POLICY_REC;
    o[e] = i < POLICY_K ? KB[k * KBUF_STRIDE + i] : X[18 * k + (i - POLICY_K)];
  }
}

#endif  // I7M_SAMPLED_POLICY_KERNELS

}  // namespace i7m
