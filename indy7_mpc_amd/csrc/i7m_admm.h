// i7m_admm.h — ADMM mode (I7M_QP_ADMM): the reference's QP solver, OSQP, as a device kernel.
//
// The reference solves every SQP subproblem with one persistent osqp.OSQP() object
// (src/osqp_solver.py:38-40 setup, :137-143 update(Px), update(Ax), update(q, l, u), solve()).
// oracle/osqp_admm.py restates OSQP and is pinned by the notebook's printed closed loop (the
// first 12 goal distances of notebooks/pin_mpc_indy7.ipynb cell 2 to 1e-9); the C++ port
// (oracle/cpp/i7m_cpu.cpp, Solver::admm) runs it in the block form this kernel runs.
//
// This header holds the QP's preparation (k_admm_scale, k_admm_factor), the termination test
// (adm_check) and what both sides share; OSQP's iteration kernels are i7m_admm_iter.h.
//
// One wavefront per problem, the QP in three launches (k_admm_scale, k_admm_factor, k_admm_iter):
//   1. OSQP's Ruiz equilibration (10 passes) of [P A'; A 0] with the previous QP's q (the
//      reference re-scales inside update(Ax), before update(q)), then the new q = c D g and
//      l = u = E l;
//   2. the x-update's matrix M = P + sigma I + A' diag(rho) A, block tridiagonal (18 x 18 blocks
//      per knot (x_k, u_k), 12 x 18 couplings x_{k+1} <- z_k), factored by a block Cholesky
//      whose diagonal factors are kept inverted (Linv_k) and whose couplings C_k = M_{k+1,k}
//      Linv_k' are kept, so every solve is two sweeps of mat-vecs;
//   3. OSQP's iteration from the problem's warm start (x, z, y, rho carried in HBM from call to
//      call like the reference's OSQP object): the solve, relaxation alpha, projection onto
//      [l, u], dual update; every `check` iterations the unscaled residuals and (OSQP 1.x) the
//      duality gap; optional adaptive rho with a refactorisation.
// Every row of A is an equality row (l = u), so rho_vec = 1e3 rho (RHO_EQ_OVER_RHO_INEQ).
// Per-stage blocks live in HBM as one record per stage (ADM_REC below: Linv packed lower-triangular
// 180, scaled J compact 120 doubles; the coupling C is never stored) and reach LDS by DMA
// (DESIGN.md §4.7).
#pragma once

#include "i7m_kernels.h"

namespace i7m {

struct AdmmCfg {
  double rho0, sigma, alpha, eps_abs, eps_rel, adapt_tol;
  int max_iter, check, scaling, gap, adapt_interval, pad;
};

struct AdmmArgs {
  SolveParams P;
  AdmmCfg A;
  const double* lin;   // (B, N-1, 114) k_linearize
  const double* cost;  // (B, N, 10)
  const double* qpd;   // (B, N-1, 32): c_v
  const double* xu;    // (B, T) linearisation point
  const double* xs;    // (B, 12)
  const int* active;
  double* sol;         // (B, T) out: D x
  // OSQP state per problem (scaled x, z, y; the previous QP's q, unscaled; rho)
  double *sx, *sz, *sy, *sq, *srho;
  // scratch per problem
  double *Pq, *Pd, *I, *qs, *ls, *D, *E, *Dt, *Et, *R, *w;
  double* cs;  // (B) OSQP's cost scale c of the current QP (k_admm_prep -> k_admm_iter)
  int* iters;  // (B, I7M_MAX_SQP): OSQP iterations of SQP iteration `sqp_iter`
  int* status;  // (B, I7M_MAX_SQP): 1 solved, 2 solved inaccurate (OSQP's approximate test after max_iter), 0 max_iter reached
  int sqp_iter;
  int b0;      // first problem of this launch (chunked launches: problems [b0, b0 + grid))
  int ablate;  // I7M_DIAG builds only (I7M_ABLATE, timing variants, results invalid); 0 otherwise
  const double* abase;  // the handle's ADMM allocation (every array above lies in it) and its bytes (< 2 GiB)
  long abytes;
};

// HBM layout of the per-stage blocks (what every OSQP iteration streams): the inverted diagonal
// factor packed lower-triangular (171 of 324), the scaled J_k as its q rows' two diagonals
// (E_i D_i for I, E_i dt D_{6+i} for dt I) and its v rows (6 x 18): 120 of 216.  Staged to LDS
// unpacked, so the arithmetic is the dense form's (the dropped entries are exact zeros).
constexpr int ADMM_FSTRIDE = 19;  // the register factor's LDS row stride for S and C (18: 3-way bank conflicts on row reads)
constexpr int ADMM_SCALE_WPE = 2;  // (N <= 32: the linearisation magnitudes stay in registers for all ten passes)
constexpr int ADMM_FACTOR_WPE = 2;
// One record per stage, N per problem (problem b's at R + b N ADM_REC): [Linv_k | compact J_k]
// = 300 doubles (150 pieces of 16 B).  Linv_k's rows 0-15 are stored lower-triangular, each padded
// to an even width (a zero after the diagonal of the even rows: 144 doubles), rows 16 and 17 in full
// (36); J_k as its q rows' two diagonals (J[i][i], J[i][6 + i]) and its v rows (6 x 18).
// k_admm_iter streams the record twice per OSQP iteration (forward and backward sweep) into LDS,
// where its DMA lays Linv's rows 0-15 out at widths of four (A5_LREC: the extra pieces read as
// zeros), so every lane's row and column reads are a base plus a constant and the entries past a
// row's width are never read (the DPP fma's bank masks skip them).  The coupling
// C_k = M_{k+1,k} Linv_k' of the factor is never stored: the sweeps apply it as re I_{k+1} J_k and
// the triangular pair.
constexpr int ADM_REC = 300, REC_J = 180;
// entry (i, j) of Linv_k in the record, and the stored width of row i
__device__ __forceinline__ int adm_lw(int i) { return i < 16 ? 2 * ((i + 2) / 2) : 18; }
__device__ __forceinline__ int adm_lrow(int i) {
  const int h = i >> 1;  // rows 2h, 2h+1 have width 2h + 2
  return i < 16 ? 2 * h * (h + 1) + (i & 1) * (2 * h + 2) : 144 + 18 * (i - 16);
}
__device__ __forceinline__ int adm_lrec(int i, int j) { return adm_lrow(i) + j; }
// Buffer-resource access (k_admm_factor's and k_admm_iter's DMA and stores): a uniform base in
// SGPRs, 32-bit per-lane byte offsets, the hardware's range check (an offset past the range reads
// zeros and drops stores: A5_OOB masks lanes without branches)
constexpr unsigned A5_OOB = 0x7ff00000u;  // a byte offset past every allocation (< 2 GiB enforced by the host)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t a4_rsrc(const void* base, long bytes) {
  const unsigned long long u = (unsigned long long)base;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  const int nb = __builtin_amdgcn_readfirstlane((int)bytes);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), (short)0, nb, 0x00020000);
}
// dense 12 x 18 J_k into LDS from its compact form
__device__ __forceinline__ void adm_stage_J(double* sJ, const double* Jc, int l) {
  for (int e = l; e < 216; e += 64) {
    const int i = e / 18, j = e - 18 * i;
    double v;
    if (i < 6) v = j == i ? Jc[i] : (j == 6 + i ? Jc[6 + i] : 0.0);
    else v = Jc[12 + 18 * (i - 6) + j];
    sJ[e] = v;
  }
}

// init + sum_i a[sa i] b[sb i] over n LDS operands (the factor's dot products): every operand read
// is issued before the fma chain, so it pays one LDS latency instead of one per term; the terms are
// summed in i order (Linv's upper triangle and the padding of the last knot's 12 x 12 blocks are
// exact zeros, which add nothing)
template <int n>
__device__ __forceinline__ double adm_dot2(double init, const double* a, int sa, const double* b, int sb) {
  double av[n], bv[n];
#pragma unroll
  for (int i = 0; i < n; ++i) {
    av[i] = a[sa * i];
    bv[i] = b[sb * i];
  }
  double acc = init;
#pragma unroll
  for (int i = 0; i < n; ++i) acc += av[i] * bv[i];
  return acc;
}

// max / sum over groups of W lanes (W = 64: the wave; 16: a DPP row)
template <int W>
__device__ __forceinline__ double adm_max(double v) {
#pragma unroll
  for (int off = W / 2; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, W));
  return v;
}
template <int W>
__device__ __forceinline__ double adm_sum(double v) {
#pragma unroll
  for (int off = W / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, W);
  return v;
}
__device__ __forceinline__ double adm_wave_max(double v) { return adm_max<64>(v); }
__device__ __forceinline__ double adm_wave_sum(double v) { return adm_sum<64>(v); }
__device__ __forceinline__ double adm_limit(double v) { return v < 1e-4 ? 1.0 : (v > 1e4 ? 1e4 : v); }

// unscaled J_k = [[I, dt I, 0], [Aq, Av, Bu]] (rows of A's block k+1 on z_k; src/osqp_solver.py:
// 42-43, 70-81), from the linearisation record
__device__ __forceinline__ double adm_jk(const double* L, double dt, int i, int j) {
  if (i < 6) return j == i ? 1.0 : (j == 6 + i ? dt : 0.0);
  const int r = i - 6;
  return j < 6 ? L[6 * r + j] : (j < 12 ? L[36 + 6 * r + j - 6] : L[72 + 6 * r + j - 12]);
}

// All of a row's (column's) loads issued before its first product: one memory round trip, not
// the default schedule's one per eight loads.
#define ADM_CHK_LOADS_FIRST()                          \
  do {                                                 \
    __builtin_amdgcn_sched_group_barrier(0x020, 24, 0); \
    __builtin_amdgcn_sched_group_barrier(0x002, 96, 0); \
  } while (0)

// OSQP's check_termination on the unscaled residuals (+ the duality gap) and, for adapt_rho,
// the scaled residual ratios; x, z, y scaled.  Returns solved; rho_est gets the estimate.  The 16
// lanes of a DPP row share one problem (lane l of the row), as in the iteration kernels.
// es scales eps_abs and eps_rel: 1 OSQP's test, 10 its approximate one after max_iter ("solved
// inaccurate", oracle/osqp_admm.py OSQP._check(approximate=True)).
__device__ inline bool adm_check(const AdmmArgs& a, int N, int T, int m, double c, double rho, const double* x,
                                 const double* z, const double* y, const double* qs, const double* ls, const double* D,
                                 const double* E, const double* Jb, const double* Ib, const double* Pq, const double* Pd,
                                 double* rho_est, int l, double es = 1.0) {
  constexpr int W = 16;
  double pr = 0.0, zn = 0.0, an = 0.0, pri = 0.0, pn = 0.0;
  double dr = 0.0, qn = 0.0, atn = 0.0, pxn = 0.0, dua = 0.0, dn = 0.0, xPx = 0.0, qx = 0.0, sc = 0.0;
  // rows: block 0 = I x_0, block k+1 = J_k z_k + I x_{k+1}.  J's structural zeros are skipped
  // (a q row has two entries: J[i][i], J[i][6 + i]; a column at most one q-row entry); the other
  // terms keep their order, so the sums are the full loops' (0 * x adds nothing).
  for (int r = l; r < m; r += W) {
    const int k = r / 12, i = r - 12 * k;
    // Every operand is loaded up front, from clamped (always valid) addresses, and the branches
    // are selects: one memory round trip per row (the lanes of a wave take both paths anyway).
    const int kk = k > 0 ? k - 1 : 0, iq = i < 6 ? i : 0, iv = i < 6 ? 0 : i - 6;
    const double* G = Jb + ADM_REC * kk;
    const double* xk = x + 18 * kk;
    const double* Gr = G + 12 + 18 * iv;
    const double ib = Ib[r], xr = x[18 * k + i], er = E[r], zr = z[r], yr = y[r], lr = ls[r];
    const double ga = G[iq], gb = G[6 + iq], xa = xk[iq], xb = xk[6 + iq];
    double gv[18], xv[18];
#pragma unroll
    for (int j = 0; j < 18; ++j) {
      gv[j] = Gr[j];
      xv[j] = xk[j];
    }
    ADM_CHK_LOADS_FIRST();
    double aq = 0.0, av = 0.0;  // a q row's two entries, a v row's 18
    aq += ga * xa;
    aq += gb * xb;
#pragma unroll
    for (int j = 0; j < 18; ++j) av += gv[j] * xv[j];
    const double acc = i < 6 ? aq : av;
    const double ax = k == 0 ? ib * xr : acc + ib * xr;
    const double ei = 1.0 / er;
    pr = fmax(pr, fabs(ei * (ax - zr)));
    zn = fmax(zn, fabs(ei * zr));
    an = fmax(an, fabs(ei * ax));
    pri = fmax(pri, fabs(ax - zr));
    pn = fmax(pn, fmax(fabs(zr), fabs(ax)));
    sc += lr * fmax(yr, 0.0) + lr * fmin(yr, 0.0);
  }
  for (int e = l; e < T; e += W) {
    const int k = e / 18, j = e - 18 * k;
    // as the rows: clamped addresses, selects for the branches
    const int jq = j < 12 ? j : 0, jc = j < 6 ? j : 0, kc = k < N - 1 ? k : 0;
    const int jy = j < 6 ? j : (j < 12 ? j - 6 : 0);  // column j's q-row entry: row j or j - 6
    const double* G = Jb + ADM_REC * kc;
    const double* yk = y + 12 * (k < N - 1 ? k + 1 : 0);
    const double xe = x[e], de = D[e], qe = qs[e], pde = Pd[e], ibj = Ib[12 * k + jq], yj = y[12 * k + jq];
    const double gq = G[jq], yq = yk[jy];
    double pq[6], xq[6], gv[6], yv[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      pq[t] = Pq[36 * k + 6 * jc + t];
      xq[t] = x[18 * k + t];
      gv[t] = G[12 + 18 * t + j];
      yv[t] = yk[6 + t];
    }
    ADM_CHK_LOADS_FIRST();
    double pa = 0.0;
#pragma unroll
    for (int t = 0; t < 6; ++t) pa += pq[t] * xq[t];
    const double px = j < 6 ? pa : pde * xe;
    const double at0 = j < 12 ? ibj * yj : 0.0;
    double at1 = j < 12 ? at0 + gq * yq : at0;
#pragma unroll
    for (int t = 0; t < 6; ++t) at1 += gv[t] * yv[t];
    const double aty = k < N - 1 ? at1 : at0;
    const double di = 1.0 / de;
    dr = fmax(dr, fabs(di * ((qe + px) + aty)));
    qn = fmax(qn, fabs(di * qe));
    atn = fmax(atn, fabs(di * aty));
    pxn = fmax(pxn, fabs(di * px));
    dua = fmax(dua, fabs(qe + px + aty));
    dn = fmax(dn, fmax(fabs(qe), fmax(fabs(aty), fabs(px))));
    xPx += xe * px;
    qx += qe * xe;
  }
  pr = adm_max<W>(pr); zn = adm_max<W>(zn); an = adm_max<W>(an); pri = adm_max<W>(pri); pn = adm_max<W>(pn);
  dr = adm_max<W>(dr); qn = adm_max<W>(qn); atn = adm_max<W>(atn); pxn = adm_max<W>(pxn);
  dua = adm_max<W>(dua); dn = adm_max<W>(dn);
  xPx = adm_sum<W>(xPx); qx = adm_sum<W>(qx); sc = adm_sum<W>(sc);
  const double cinv = 1.0 / c;
  // OSQP compute_rho_estimate (scaled residuals)
  {
    const double p = pri / (pn + 1e-30), d = dua / (dn + 1e-30);
    double rn = rho * sqrt(p / (d + 1e-30));
    *rho_est = fmin(fmax(rn, 1e-6), 1e6);
  }
  dr *= cinv;
  const double ea = es * a.A.eps_abs, er = es * a.A.eps_rel;
  if (!(pr < ea + er * fmax(zn, an))) return false;
  if (!(dr < ea + er * cinv * fmax(qn, fmax(atn, pxn)))) return false;
  if (a.A.gap) {
    xPx *= cinv; qx *= cinv; sc *= cinv;
    const double gp = xPx + qx + sc;
    if (!(fabs(gp) < ea + er * fmax(fabs(xPx), fmax(fabs(qx), fabs(sc))))) return false;
  }
  return true;
}

// OSQP's scaling of the QP (src/osqp_solver.py:137-143: update(Px), update(Ax) rescale with the
// previous q; then update(q, l, u)), as oracle/cpp/i7m_cpu.cpp Solver::admm_setup: 10 Ruiz passes
// on [P A'; A 0] and the cost normalisation, then the scaled P blocks, J_k, the -I entries, q and l
// into HBM; returns the cost scale c.  D and E live in LDS during the passes; a lane owns columns
// e = l + 64 t (t < CT) and rows r = l + 64 t (t < 2 CT / 3), whose scale factors and q entries
// stay in its registers.  Every column's and row's inf-norm reads its entries unconditionally at
// clamped indices and selects (a P column: 6 entries of the quadratic block or the diagonal; an A
// column: the -I entry, J's identity / dt entry and 6 linearisation entries; an A row: its -I
// entry and 18 J entries), so the loads of all of a lane's columns issue together.  The products
// are the port's (|a_ij| D_j E_i in its order; max is exact), so D, E and c are the one-kernel
// version's to the bit, the cost sum's wave reduction aside.  Its LDS orderings are fences
// (wave_sync_fence): as compiler barriers (wave_sync) the kernel ran 0.59 -> 2.42 ms.
__device__ __forceinline__ double adm_pq(const double* w, int i, int j) { return w[6] * (w[i] * w[j]); }
template <int CT>
__device__ __forceinline__ double adm_scale(const AdmmArgs& a, int b, int N, int T, int m, const double* LIN,
                                            const double* CO, const double* QD, const double* X, double* qold,
                                            double* Pq, double* Pd, double* Jb, double* Ib, double* qs, double* ls,
                                            double* D, double* E, double* sD, double* sE, double* sDt, double* sRM, int l) {
  constexpr int RT = 2 * CT / 3;
  const double dt = a.P.dt;
  double qv[CT], etv[RT], dtv[CT <= 9 ? CT : 1];  // (a lane's q entries and its columns' / rows' pass factors)
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const int e = l + 64 * t;
    qv[t] = 0.0;
    if (e < T) {
      sD[e] = 1.0;
      qv[t] = qold[e];
    }
  }
#pragma unroll
  for (int t = 0; t < RT; ++t)
    if (l + 64 * t < m) sE[l + 64 * t] = 1.0;
  wave_sync_fence();
  double c = 1.0;
  // the P part of column e's inf-norm (knot k, index j in the knot): max_i |P_ij| D_i D_j c
  auto pcol = [&](const double* Cp, int k, int j, double dj) {
    const double* w = Cp + COST_STRIDE * k;
    const int jq = j < 6 ? j : 0;
    double mq = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) mq = fmax(mq, fabs(adm_pq(w, i, jq)) * (sD[18 * k + i] * dj) * c);
    const double pd = j < 12 ? w[7] : w[8];
    return j < 6 ? mq : fabs(pd) * (dj * dj) * c;
  };
  // N <= 32 (CT <= 9): the linearisation's 108 v-row entries of stage k live in the registers of
  // lanes 2k (rows 6-8 of block k + 1) and 2k + 1 (rows 9-11) for all passes, read once: each pass
  // forms their scaled magnitudes (E_i |a_ij|) D_j once, for both the row maxima (sRM) and, with the
  // partner lane's three rows, the column maxima (sDt); max is exact, so every norm is the port's.
  constexpr bool REG = CT <= 9;
  const int ks = l >> 1, hs = l & 1;
  const bool sv = REG && ks < N - 1;
  double av[REG ? 3 : 1][REG ? 18 : 1];
  if constexpr (REG) {
    const double* L = LIN + LIN_STRIDE * (sv ? ks : 0);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int j = 0; j < 18; ++j) {
        const int jb = j < 6 ? j : (j < 12 ? 30 + j : 60 + j);
        av[r][j] = sv ? L[jb + 6 * (3 * hs + r)] : 0.0;  // (signed: the J output below uses it too)
      }
  }
#ifdef I7M_DIAG
  // I7M_ABLATE 300000 + P (tools/step_stamps.py --scale): s_memtime at the parts of Ruiz pass P of
  // workgroup 0 (record area 5 of the timeline buffer)
  const int ss_p = a.ablate >= 300000 ? a.ablate - 300000 : -1;
  const bool ss_on = ss_p >= 0 && blockIdx.x == 0;
  unsigned long long ss_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
#define AS_STAMP(i) I7M_STAMP(ss_t, i, ss_on && pass == ss_p)
  for (int pass = 0; pass < a.A.scaling; ++pass) {
    AS_STAMP(0);
    // every pass recomputes its indices (hoisted out of the pass loop they would take ~300 VGPRs)
    const double* Lp = LIN;
    const double* Cp = CO;
    int lp = l;
    asm volatile("" : "+v"(lp));
    if constexpr (REG) {
      double cm[18];
#pragma unroll
      for (int j = 0; j < 18; ++j) cm[j] = 0.0;
      const int kq = sv ? ks : 0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double er = sE[12 * (kq + 1) + 6 + 3 * hs + r];
        double rm = 0.0;
#pragma unroll
        for (int j = 0; j < 18; ++j) {
          const double pv = er * fabs(av[r][j]) * sD[18 * kq + j];
          rm = fmax(rm, pv);
          cm[j] = fmax(cm[j], pv);
        }
        if (sv) sRM[12 * (kq + 1) + 6 + 3 * hs + r] = rm;
      }
      // the partner lane's rows (DPP quad_perm [1,0,3,2]), then lane h stores columns 9h..9h+8
#pragma unroll
      for (int j = 0; j < 18; ++j) {
        const long long u = __double_as_longlong(cm[j]);
        const int lo = __builtin_amdgcn_update_dpp(0, (int)u, 0xB1, 0xf, 0xf, true);
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), 0xB1, 0xf, 0xf, true);
        cm[j] = fmax(cm[j], __longlong_as_double(((long long)hi << 32) | (unsigned int)lo));
      }
      if (sv) {
#pragma unroll
        for (int j = 0; j < 9; ++j) sDt[18 * kq + 9 * hs + j] = hs ? cm[9 + j] : cm[j];
      }
      wave_sync_fence();
    }
    AS_STAMP(1);
#pragma unroll 3
    for (int t = 0; t < CT; ++t) {
      const int e = min(lp + 64 * t, T - 1), k = e / 18, j = e - 18 * k;
      const double dj = sD[e];
      double mx = pcol(Cp, k, j, dj);
      const double ei = sE[12 * k + (j < 12 ? j : 0)] * dj;
      if (j < 12) mx = fmax(mx, ei);
      // J_k's column j (rows of block k + 1; the last knot has none): the identity / dt entry, 6
      // linearisation entries
      const int kk = k < N - 1 ? k : N - 2;
      const double* L = Lp + LIN_STRIDE * kk;
      const double* Eb = sE + 12 * (kk + 1);
      const int jb = j < 6 ? j : (j < 12 ? 30 + j : 60 + j);
      const double eid = Eb[j < 6 ? j : (j < 12 ? j - 6 : 0)] * (j < 6 ? 1.0 : dt) * dj;
      double mj = j < 12 ? eid : 0.0;
      if constexpr (REG) {
        mj = fmax(mj, sDt[e]);  // (the stage owners' max over the six v rows)
      } else {
#pragma unroll
        for (int r = 0; r < 6; ++r) mj = fmax(mj, Eb[6 + r] * fabs(L[jb + 6 * r]) * dj);
      }
      if (k < N - 1) mx = fmax(mx, mj);
      // (a lane's own pass factors: registers at N <= 32, LDS at the wide variant's register count)
      if constexpr (REG) dtv[t] = 1.0 / sqrt(adm_limit(mx));
      else sDt[lp + 64 * t] = 1.0 / sqrt(adm_limit(mx));
    }
    AS_STAMP(2);
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int r = min(lp + 64 * t, m - 1), blk = r / 12, i = r - 12 * blk;
      const double er = sE[r];
      double mx = er * sD[18 * blk + i];
      // row i of J_{blk-1} (block 0's rows are -I on x_0 alone)
      const int kk = blk > 0 ? blk - 1 : 0;
      const double* Db = sD + 18 * kk;
      // rows 0-5: the identity and dt entries; rows 6-11: 18 linearisation entries (at N <= 32
      // their max from the stage owners)
      const int i6 = i < 6 ? i : i - 6;
      const double mi = fmax(er * 1.0 * Db[i6], er * dt * Db[6 + i6]);
      double ml = 0.0;
      if constexpr (REG) {
        ml = sRM[r];
      } else {
        const double* L = Lp + LIN_STRIDE * kk;
#pragma unroll
        for (int j = 0; j < 18; ++j) {
          const int jb = j < 6 ? j : (j < 12 ? 30 + j : 60 + j);
          ml = fmax(ml, er * fabs(L[jb + 6 * i6]) * Db[j]);
        }
      }
      const double mj = i < 6 ? mi : ml;
      if (blk > 0) mx = fmax(mx, mj);
      etv[t] = 1.0 / sqrt(adm_limit(mx));
    }
    AS_STAMP(3);
    wave_sync_fence();
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const int e = lp + 64 * t;
      double dtt;
      if constexpr (CT <= 9) dtt = dtv[t];
      else dtt = sDt[e];
      if (e < T) sD[e] = sD[e] * dtt;
      qv[t] = dtt * qv[t];
    }
#pragma unroll
    for (int t = 0; t < RT; ++t)
      if (lp + 64 * t < m) sE[lp + 64 * t] = sE[lp + 64 * t] * etv[t];
    wave_sync_fence();
    AS_STAMP(4);
    // cost normalisation: mean column norm of the scaled P, |q|
    double sm = 0.0, qm = 0.0;
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const int e = lp + 64 * t, ec = min(e, T - 1), k = ec / 18, j = ec - 18 * k;
      const double mx = pcol(Cp, k, j, sD[ec]);
      if (e < T) {
        sm += mx;
        qm = fmax(qm, fabs(qv[t]));
      }
    }
    sm = adm_wave_sum(sm);
    qm = adm_limit(adm_wave_max(qm));
    const double ct = 1.0 / adm_limit(fmax(sm / T, qm));
#pragma unroll
    for (int t = 0; t < CT; ++t) qv[t] = qv[t] * ct;
    c = c * ct;
    AS_STAMP(5);
  }
#undef AS_STAMP
#ifdef I7M_DIAG
  if (ss_on && l == 0) tl_write_stamps(ss_t, 6, a.ablate, 3);
#endif
  // scaled data: P <- c D P D, J <- E J D, I <- -E D, q <- c D g (update(q)), l <- E l
  for (int e = l; e < T; e += 64) D[e] = sD[e];
  for (int r = l; r < m; r += 64) E[r] = sE[r];
#pragma unroll 4
  for (int x = l; x < 36 * N; x += 64) {
    const int k = x / 36, q = x - 36 * k, i = q / 6, j = q - 6 * i;
    Pq[x] = adm_pq(CO + COST_STRIDE * k, i, j) * (sD[18 * k + i] * sD[18 * k + j]) * c;
  }
  if constexpr (REG) {
    // J_k by its stage owners, from the registers (rows 6 + 3h .. 8 + 3h, and q rows 3h .. 3h + 2)
    if (sv) {
      double* Jk = Jb + ADM_REC * ks;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int i = 3 * hs + r;
        const double ev = sE[12 * (ks + 1) + 6 + i];
#pragma unroll
        for (int j = 0; j < 18; ++j) Jk[12 + 18 * i + j] = ev * av[r][j] * sD[18 * ks + j];
        const double eq = sE[12 * (ks + 1) + i];
        Jk[i] = eq * 1.0 * sD[18 * ks + i];
        Jk[6 + i] = eq * dt * sD[18 * ks + 6 + i];
      }
    }
  } else {
#pragma unroll 4
    for (int x = l; x < 120 * (N - 1); x += 64) {
      const int k = x / 120, e = x - 120 * k;
      int i, j;
      if (e < 6) { i = e; j = e; }
      else if (e < 12) { i = e - 6; j = e; }
      else { i = 6 + (e - 12) / 18; j = (e - 12) % 18; }
      Jb[ADM_REC * k + e] = sE[12 * (k + 1) + i] * adm_jk(LIN + LIN_STRIDE * k, dt, i, j) * sD[18 * k + j];
    }
  }
  for (int r = l; r < m; r += 64) {
    const int k = r / 12, i = r - 12 * k;
    Ib[r] = -sE[r] * sD[18 * k + i];
    double lv;
    if (k == 0) lv = -a.xs[12 * (long)b + i];
    else lv = i < 6 ? 0.0 : -QD[QPD_STRIDE * (k - 1) + QPD_CV + i - 6];
    ls[r] = sE[r] * lv;
  }
  for (int e = l; e < T; e += 64) {
    const int k = e / 18, j = e - 18 * k;
    const double* w = CO + COST_STRIDE * k;
    const double dd = sD[e];
    Pd[e] = j < 6 ? 0.0 : (j < 12 ? w[7] : w[8]) * (dd * dd) * c;
    const double g = j < 6 ? w[6] * w[j] : (j < 12 ? w[7] * X[e] : w[8] * X[e]);
    qold[e] = g;
    qs[e] = c * (dd * g);
  }
  wave_sync_all();
  return c;
}

// M = P + sigma I + A' rho A, block Cholesky with inverted diagonal factors (as Solver::
// admm_factor of the port): Linv_k (packed) into record k, C_k into record k+1.  Per stage: the
// block S_k in LDS (all lanes, every dot product's operands loaded before its fma chain), its
// right-looking Cholesky with row i in lane i's registers (the pivot by readlane, the column
// through LDS: one round trip per pivot), Linv_k by forward substitution with column j in lane j's
// registers, then C_k.  The last knot's 12 x 12 block is factored padded with an identity, whose
// entries are stored as the zeros the port has there.  Same operations in the port's order (the
// zeros the padding and the triangles add are exact).
__device__ __forceinline__ double adm_readlane(double v, int lane) {
  const long long u = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)u, lane), hi = __builtin_amdgcn_readlane((int)(u >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// A stage's operands arrive one stage ahead by LDS DMA into `stg` (two buffers of 256 doubles:
// compact J_k 120 | P_k's quadratic block 36 | its diagonal 18 | I_k 12 | I_{k+1} 12), so no stage
// waits on a global load; the DMA (inline asm, the compiler does not see it) is waited for by a
// counted s_waitcnt at the next stage's start.
constexpr int AF_STG = 256;
__device__ __forceinline__ void adm_factor(const AdmmArgs& a, int N, double rho, const double* Pq, const double* Pd, const double* Ib,
                           double* Rb, double* sS, double* sJ, double* sL, double* sCp, double* stg, int l0) {
  const double re = 1e3 * rho, sigma = a.A.sigma;
  constexpr int FS = ADMM_FSTRIDE;  // row stride of S and C_{k-1} in LDS
  double* sCol = sL + 324;  // (the sweeps' C slot, free while factoring)
  const auto rA = a4_rsrc(a.abase, a.abytes);
  auto boff = [&](const double* q) { return (unsigned)__builtin_amdgcn_readfirstlane((int)((const char*)q - (const char*)a.abase)); };
  const unsigned oR = boff(Rb), oPq = boff(Pq), oPd = boff(Pd), oI = boff(Ib);
  const unsigned stg_lds = (unsigned)(unsigned long)(__attribute__((address_space(3))) void*)stg;
  // stage k's pieces: lane l's piece g = l (+ 64): [0, 60) J, [60, 78) Pq, [78, 87) Pd, [87, 93) I_k,
  // [93, 99) I_{k+1}, past 99 nothing
  auto fetch = [&](int k) {
    unsigned vo[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int g = 64 * u + l0;
      unsigned o;
      if (g < 60) o = oR + 8u * (unsigned)(ADM_REC * k + REC_J) + 16u * g;
      else if (g < 78) o = oPq + 8u * (unsigned)(36 * k) + 16u * (g - 60);
      else if (g < 87) o = oPd + 8u * (unsigned)(18 * k) + 16u * (g - 78);
      else if (g < 99) o = oI + 8u * (unsigned)(12 * k) + 16u * (g - 87);
      else o = A5_OOB;
      vo[u] = o - 1024u * u;
    }
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %2, %4, 0 offen lds\n\t"
        "buffer_load_dwordx4 %3, %4, 0 offen offset:1024 lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "s"(__builtin_amdgcn_readfirstlane(stg_lds + 8u * AF_STG * (k & 1))), "v"(vo[0]), "v"(vo[1]), "s"(rA)
        : "memory");
  };
  fetch(0);
#ifdef I7M_DIAG
  // I7M_ABLATE 200000 + K (tools/step_stamps.py --factor): s_memtime at the phases of stage K of
  // workgroup 0's factor (its own launch: the record area 5 of the timeline buffer)
  const int fs_k = a.ablate >= 200000 && a.ablate < 300000 ? a.ablate - 200000 : -1;
  const bool fs_on = fs_k >= 0 && blockIdx.x == 0;
  unsigned long long fs_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
#define AF_STAMP(i) I7M_STAMP(fs_t, i, fs_on && k == fs_k)
  for (int k = 0; k < N; ++k) {
    AF_STAMP(0);
    const int nk = k < N - 1 ? 18 : 12;
    // every stage recomputes the lane's indices (hoisted out of the stage loop they would take
    // more registers than the kernel has)
    int l = l0;
    asm volatile("" : "+v"(l));
    const int lr = l < 18 ? l : 17;  // lanes 18-63 shadow lane 17 (never read back)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stage k's operands have landed
    if (k + 1 < N) fetch(k + 1);
    const double* G = stg + AF_STG * (k & 1);
    if (k < N - 1) adm_stage_J(sJ, G, l);
    wave_sync();
    AF_STAMP(1);
    // S is symmetric to the bit (every term's products commute and sum in the same order), so the
    // lanes form its lower triangle (171 entries) and mirror it
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int e = l + 64 * t;
      if (e < 171) {
        int i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
        i = (i + 1) * (i + 2) / 2 <= e ? i + 1 : (i * (i + 1) / 2 > e ? i - 1 : i);
        const int j = e - i * (i + 1) / 2, ic = i < 12 ? i : 11, jc = j < 12 ? j : 11;
        const double pq = G[120 + 6 * (i < 6 ? i : 0) + (j < 6 ? j : 0)];
        const double pd = G[156 + i];  // (the last stage's rows past 12: overwritten below)
        const double ib = G[174 + ic];
        const double dj = adm_dot2<12>(0.0, sJ + i, 18, sJ + j, 18);
        const double dc = adm_dot2<18>(0.0, sCp + FS * ic, 1, sCp + FS * jc, 1);
        double v = i < 6 && j < 6 ? pq : (i == j && i >= 6 ? pd : 0.0);
        if (i == j) v += sigma;
        if (i == j && i < 12) v += re * (ib * ib);
        if (k < N - 1) v += re * dj;
        if (k > 0 && i < 12 && j < 12) v -= dc;
        if (i >= nk || j >= nk) v = i == j ? 1.0 : 0.0;
        sS[FS * i + j] = v;
        sS[FS * j + i] = v;
      }
    }
    wave_sync();
    AF_STAMP(2);
    double r[18];
#pragma unroll
    for (int j = 0; j < 18; ++j) r[j] = sS[FS * lr + j];
    double myid = 1.0;  // 1 / L_ll of this lane's row (the inverse multiplies by it)
#pragma unroll
    for (int p = 0; p < 18; ++p) {
      const double d = sqrt(adm_readlane(r[p], p));
      const double id = 1.0 / d;
      myid = l == p ? id : myid;
      r[p] = l == p ? d : (l > p ? r[p] * id : r[p]);
      if (p < 17) {
        // column p of L to the wave through LDS (double-buffered: no wait for the last reads)
        double* col = sCol + 32 * (p & 1);
        if (l < 18) col[l] = r[p];
        wave_sync();
#pragma unroll
        for (int j = p + 1; j < 18; ++j) r[j] = r[j] - r[p] * col[j];
      }
    }
    AF_STAMP(3);
    wave_sync();  // every lane has read S before L overwrites it
    static_assert(FS >= 19, "the row's spare column holds 1 / L_ii");
    if (l < 18) {
#pragma unroll
      for (int j = 0; j < 18; ++j) sS[FS * l + j] = r[j];
      sS[FS * l + 18] = myid;
    }
    wave_sync();
    AF_STAMP(4);
    double x[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) {
      // row i of L is read once x_{i-2} exists (two rows of loads in flight, not all 171)
      int o = FS * i;
      if (i >= 2) asm volatile("" : "+v"(o) : "v"(x[i - 2]));
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < i; ++q) acc += sS[o + q] * x[q];
      x[i] = ((i == lr ? 1.0 : 0.0) - acc) * sS[o + 18];  // (the port's order: by 1 / L_ii)
    }
    if (l < 18) {
#pragma unroll
      for (int i = 0; i < 18; ++i) {
        const double v = i < nk && l < nk ? x[i] : 0.0;
        sL[18 * i + l] = v;
        if (l < adm_lw(i)) Rb[ADM_REC * k + adm_lrec(i, l)] = v;  // (+0 above the diagonal)
      }
    }
    wave_sync();
    AF_STAMP(5);
    if (k < N - 1) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int e = l + 64 * t;
        if (e < 216) {
          const int i = e / 18, j = e - 18 * i;
          const double acc = adm_dot2<18>(0.0, sJ + 18 * i, 1, sL + 18 * j, 1);
          const double cv = re * G[186 + i] * acc;
          sCp[FS * i + j] = cv;
        }
      }
    }
    // (LDS only: the stage's global stores are read by no later stage, and the kernel's end or the
    // re-factoring caller's fence orders them; a global release here waited for them every stage)
    wave_sync_fence();
    AF_STAMP(6);
  }
#undef AF_STAMP
#ifdef I7M_DIAG
  if (fs_on && l0 == 0) tl_write_stamps(fs_t, 7, a.ablate, 2);
#endif
}

// k_admm_scale (PH 1: scaling, the new q and l; c to a.cs) and k_admm_factor (PH 8: the block
// Cholesky), one problem per wave; each compiled for its own registers and LDS.
template <int PH, int CT>
__device__ __forceinline__ void admm_body(const AdmmArgs& a) {
  const int b = a.b0 + blockIdx.x;
  const SolveParams& P = a.P;
  if (b >= P.B || (a.active && !a.active[b])) return;
  const int l = threadIdx.x, N = P.N, T = P.T, m = 12 * N;
  constexpr bool FAC = (PH & 8) != 0;
  __shared__ double sB[(PH & 1) ? 64 * CT : 756], sS[FAC ? 18 * ADMM_FSTRIDE : 1], sCp[FAC ? 12 * ADMM_FSTRIDE : 1];
  __shared__ double sD[(PH & 1) ? 64 * CT : 1], sE[(PH & 1) ? 64 * (2 * CT / 3) : 1], sRM[(PH & 1) ? 64 * (2 * CT / 3) : 1],
      sCO[(PH & 1) ? (64 * CT / 18 + 1) * COST_STRIDE : 1], sStg[FAC ? 2 * AF_STG : 1];
  double* sL = sB;
  double* sJ = sB + 540;
  const double* LIN = a.lin + (long)b * (N - 1) * LIN_STRIDE;
  const double* CO = a.cost + (long)b * N * COST_STRIDE;
  const double* QD = a.qpd + (long)b * (N - 1) * QPD_STRIDE;
  const double* X = a.xu + (long)b * T;
  double* qold = a.sq + (long)b * T;
  double* Pq = a.Pq + (long)b * N * 36;
  double* Pd = a.Pd + (long)b * T;
  double* Rb = a.R + (long)b * N * ADM_REC;
  double* Jb = Rb + REC_J;  // J_k at Jb + ADM_REC k
  double* Ib = a.I + (long)b * m;
  double* qs = a.qs + (long)b * T;
  double* ls = a.ls + (long)b * m;
  double* D = a.D + (long)b * T;
  double* E = a.E + (long)b * m;
  if constexpr (PH & 1) {
    // the cost blocks every pass reads, in LDS for the launch
    for (int e = l; e < N * COST_STRIDE; e += 64) sCO[e] = CO[e];
    const double c = adm_scale<CT>(a, b, N, T, m, LIN, sCO, QD, X, qold, Pq, Pd, Jb, Ib, qs, ls, D, E, sD, sE, sB, sRM, l);
    if (l == 0) a.cs[b] = c;
  }
  if constexpr (PH & 8) {
    adm_factor(a, N, a.srho[b], Pq, Pd, Ib, Rb, sS, sJ, sL, sCp, sStg, l);
  }
}

template <int CT>  // columns of [P; A] per lane: 9 for N <= 32, 18 for N <= 64
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ADMM_SCALE_WPE, ADMM_SCALE_WPE)))
k_admm_scale(AdmmArgs a) {
  admm_body<1, CT>(a);
}
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ADMM_FACTOR_WPE, ADMM_FACTOR_WPE)))
k_admm_factor(AdmmArgs a) {
  admm_body<8, 1>(a);
}

}  // namespace i7m
