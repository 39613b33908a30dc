// i7m_mpc_policy.h — the QP's time-varying feedback policy and the multi-rate plant driven by it.
//
// Every exact solve computes the LQR policy of its QP: the backward sweep of riccati_mfma_body
// (i7m_riccati_mfma.h) stores K~_k = -H^-1 G~ (6 x 13: [K_k | kff_k]) of every stage k = 0 .. N - 2
// into kbuf for its own forward rollout, u_k = K~_k [x_k; 1] in absolute coordinates (the QP
// variable is XU itself).  The two kernels here read those gains after the sweep; neither changes
// a kernel that existed.  The reference has no counterpart: its plant holds knot 0's control until
// the next solve (i7m_mpc_multirate.h).
//
// kbuf in global memory, as the sweep's stores leave it (i7m_riccati_mfma.h: `kk[l] = sh[MO_KT + l]`
// for the 64 lanes and `kk[64 + l % 20] = sh[ko20]` for the tail; the rollout's loader fbase / fpos
// reads it back the same way): per problem N - 1 stage slots of KBUF_STRIDE = 84 doubles,
//     slot[13 r + c], r < 6, c < 13   K~_k[r][c] row-major: c < 12 the gain K_k, c = 12 kff_k
//     slot[78 + i],   i < 6           c_v[i], the stage's dynamics offset (not part of the policy)
// Entries 0 .. 63 are stored by lane l = entry, entries 64 .. 83 (K~'s last 14 and c_v) by the lanes
// l % 20: the "20-double tail".  The per-lane blocks of 20 doubles (lane m < 6: row m of K~) exist
// only in the rollout's LDS slot, not in global memory.
#pragma once

#include "i7m_mpc_multirate.h"

namespace i7m {

constexpr int POLICY_K = 78;  // doubles of K~ per stage in kbuf and in K_out
// One step's knot index per plant sub-step (multirate_schedule's sub_knot), a launch argument like
// the sub-step count: at most MULTIRATE_MAX_SUB (i7m_plan.h) entries, each <= N - 2 < 64.
constexpr int POLICY_MAX_SUB = 66;
struct PolicyKnots {
  unsigned char j[POLICY_MAX_SUB + 2];
};

#ifdef I7M_POLICY_KERNELS  // (i7m_mpc_policy_tu.hip: the kernels live in that unit alone)

// K_out[b, k, :, :] = K~_k of problem b for k < n_k (i7m_qp_policy).  One workgroup per problem;
// consecutive threads read consecutive doubles of a stage slot's first 78 and write consecutive
// doubles of K_out.
__global__ void __launch_bounds__(256) k_policy_gather(int N, int n_k, const double* __restrict__ kbuf,
                                                       double* __restrict__ K_out) {
  const long b = blockIdx.x;
  const double* KB = kbuf + b * (N - 1) * KBUF_STRIDE;
  double* o = K_out + b * n_k * POLICY_K;
  for (int e = threadIdx.x; e < n_k * POLICY_K; e += 256) {
    const int k = e / POLICY_K;
    o[e] = KB[k * KBUF_STRIDE + (e - k * POLICY_K)];
  }
}

// k_mpc_multirate_step (i7m_mpc_multirate.h) with the plant under the policy of this step's solve
// (I7M_CONTROL_POLICY): distance, goal, stop, NaN conventions, shift, pins, u_out and xpath_out as
// there.  Sub-step s begins at plant state x with j = KN.j[s] knots of this step completed
// (multirate_schedule) and is driven by
//     u = xu_new.u_j + K_j (x - xu_new.x_j),
// K_j the 6 x 12 gain of stage j in kbuf (the policy pass after the solve: linearised at xu_new
// with x_0 = xcur); the feedforward column is not used.  At x = xu_new.x_j every product is an
// exact zero and u is xu_new.u_j bit for bit: a step's first sub-step runs under I7M_CONTROL_NEW's control.
// The plant is the serial rk4 it was; K_j dx runs across lanes 0 .. 47, so the chain gains one add per
// control and sub-step instead of 72 fmas.  Lane 8 r + c holds t_c = K[r][c] dx[c] (+ K[r][c + 8]
// dx[c + 8] for c < 4), every product and sum rounded on its own (no fma), and three shuffles over
// the group of eight give du[r] = ((t0 + t4) + (t2 + t6)) + ((t1 + t5) + (t3 + t7)): a fixed tree, which
// a host loop built from the library's hooks can restate bit for bit
// (tests/test_gpu_multirate_policy.py).
__global__ void __launch_bounds__(64) k_mpc_multirate_policy_step(const DevModel* __restrict__ Mg, int n, const MultirateArgs A,
                                                                  const PolicyKnots KN, const double* __restrict__ kbuf) {
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
  const double* KB = kbuf + (long)b * (N - 1) * KBUF_STRIDE;
  double* x = A.xs + 12L * b;
  double* g = A.goals + (long)b * 3 * N;
  if (l < 6) A.u_out[6L * b + l] = X[12 + l];
  if (l == 0) {
    double q[6], c[6], s[6], p[3];
    for (int r = 0; r < 6; ++r) q[r] = x[r];
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
  }
  __syncthreads();
  if (s_stop) {
    nan_path();
    return;
  }
  // Every lane carries the plant's state and runs the same rk4 (the lanes agree bit for bit, as in
  // k_sampled_multirate_step): the sub-step loop has no barrier, no LDS and no lane-conditional
  // plant, so the compiler treats rk4_step here as it does in k_mpc_multirate_step's loop (the same
  // fma, mul and add counts per sub-step), and with K dx = 0 the run is that kernel's bit for bit.
  // Each lane takes its two terms of K_j dx from its own copy of x; du returns to every lane by shuffles.
  const int row = l >> 3, c0 = l & 7;
  double q[6], v[6], qo[6], vo[6], u[6];
  for (int r = 0; r < 6; ++r) {
    q[r] = x[r];
    v[r] = x[6 + r];
  }
#pragma nounroll
  for (int k = 0; k < A.n_sub; ++k) {
    const int j = KN.j[k];
    double p = 0.0;
    {
#pragma clang fp contract(off)
      // x[c0] and x[c0 + 8] of this lane's copy (selects: no dynamic register index)
      double xa = q[0], xb = v[2];
      for (int c = 1; c < 6; ++c) xa = c0 == c ? q[c] : xa;
      for (int c = 6; c < 8; ++c) xa = c0 == c ? v[c - 6] : xa;
      for (int c = 1; c < 4; ++c) xb = c0 == c ? v[2 + c] : xb;
      if (l < 48) {
        const double* Kr = KB + (long)j * KBUF_STRIDE + 13 * row;
        const double* xj = Xn + 18 * j;
        p = Kr[c0] * (xa - xj[c0]);
        if (c0 < 4) p = p + Kr[c0 + 8] * (xb - xj[c0 + 8]);
      }
    }
    p += __shfl_xor(p, 4, 8);
    p += __shfl_xor(p, 2, 8);
    p += __shfl_xor(p, 1, 8);
    for (int r = 0; r < 6; ++r) u[r] = Xn[18 * j + 12 + r] + __shfl(p, 8 * r);
    rk4_step(*Mg, q, v, u, A.sub_dt[k], nullptr, false, qo, vo);
    double* xp = A.xpath_out + ((long)k * A.hist_stride + b) * 6;
    for (int r = 0; r < 6; ++r) {
      q[r] = qo[r];
      v[r] = vo[r];
      if (l == 0) xp[r] = qo[r];
    }
  }
  if (l == 0)
    for (int r = 0; r < 6; ++r) {
      xn[r] = q[r];
      xn[6 + r] = v[r];
    }
  __syncthreads();  // the controls X[12:18] are read (u_out) before the shift overwrites them
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

#endif  // I7M_POLICY_KERNELS

}  // namespace i7m
