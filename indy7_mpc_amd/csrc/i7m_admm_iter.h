// i7m_admm_iter.h — OSQP's iteration (step 3 of i7m_admm.h) as three kernels that run the same
// operations in the same order (bit-identical results): k_admm_iter<ADAPT> and k_admm_iter2 stream
// a three-slot LDS ring (admm_iter4: four or two problems per wave), k_admm_iter_res keeps one
// problem resident in LDS (admm_iter_res).  The step's arithmetic is written once (a4_forward,
// a4_forward_last, a4_backward and a4_block0 over a4_llt and a4_relax; a4_check, a4_closing_status,
// a4_finish, a4_solution); the two kernel bodies hold what differs: where a step's operands come
// from, where its results go, the DMA and wait schedule, and (admm_iter4 only) per-row termination
// and the adaptive-rho re-factor.
#pragma once

#include "i7m_admm.h"

namespace i7m {

// the LDS image of a stage record: rows 0-15 at widths 4, 8, 12, 16 (160 doubles), rows 16 and 17
// (36), J (120)
constexpr int A5_LREC = 316, A5_LJ = 196;
__device__ __forceinline__ int a5_lrow(int i) {
  const int g = i >> 2;
  return i < 16 ? 8 * g * (g + 1) + 4 * (g + 1) * (i - 4 * g) : 160 + 18 * (i - 16);
}

// ---- OSQP's iterations (k_admm_iter): four problems per wave, one per 16-lane DPP row --------
// Lane l works on problem b0 + 4 blockIdx.x + (l >> 4), row c = l & 15 of its 18-dim stage vectors:
// a stage vector v is (v_lo in lane c = v_c, c < 16; v16, v17 held by every lane of the row).  The
// sweeps are the block LDL' of M with S_k^-1 = Linv_k' Linv_k (oracle/cpp/i7m_cpu.cpp admm_solve):
//   forward   g_k = rhs_k - [re I_k (J_{k-1} h_{k-1}); 0],  h_k = Linv_k' (Linv_k g_k)
//   backward  xt_k = h_k - Linv_k' (Linv_k (J_k' (re I_{k+1} xt_{k+1}[:12])))
// then z~ = J_k xt_k + I_{k+1} xt_{k+1} for block k+1's rows, OSQP's relaxation, projection and dual
// update.  Every mat-vec is a chain of fma's whose broadcast operand comes from the row's own lanes
// by DPP (v_fmac_f64_dpp row_newbcast: no LDS round trip on the sweep's chain); the matrix operand
// is read from LDS, straight out of the stage record as HBM holds it (ADM_REC's padded rows make
// every read a base plus a constant).
//
// Every byte the sweeps read arrives by LDS DMA (buffer_load_dwordx4 ... lds): a step's four stage
// records (10 wave-instructions) and its vectors (3) land in one slot of a three-slot ring two steps
// before the step, so no register holds data in flight (a register ring costs 120 VGPRs, and a
// spilled or copied member waits for its load) and the wave's only waits on memory are one counted
// s_waitcnt vmcnt per step.  The DMA is issued from inline asm, so the compiler neither sees it nor
// drains it at its own waits; the ring's LDS reads are ordinary (compiler-scheduled) reads behind
// the asm's memory clobber.  All arrays are reached through one buffer resource over the handle's
// ADMM allocation (32-bit byte offsets; out-of-range offsets read zeros and drop stores, which
// masks finished and absent rows without branches).  Problems stop at their own termination test.
constexpr int A5_RI = 10;                      // record DMA wave-instructions per step (640 >= 4 x 158 pieces)
constexpr int A5_VI = 3;                       // vector DMA wave-instructions per step (192 >= 4 x 42 pieces)
constexpr int A5_VP = 42;                      // vector pieces per problem and step
constexpr int A5_RP = A5_LREC / 2;             // LDS record pieces per problem and stage (158)
template <int n>
__device__ __forceinline__ double a4_bc(double v) {  // lane n of the 16-lane row, to every lane of it
  return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + n, 0xf, 0xf, false);
}
__device__ __forceinline__ double a4_dpp32(double v, int ctrl_is_shl) {
  const long long u = __double_as_longlong(v);
  int lo = (int)u, hi = (int)(u >> 32);
  if (ctrl_is_shl) {
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x106, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x106, 0xf, 0xf, false);
  } else {
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x116, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x116, 0xf, 0xf, false);
  }
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// lane c gets lane c - 6's value (c >= 6 of the row), keeps its own below / lane c + 6's (c < 10)
__device__ __forceinline__ double a4_shr6(double v) { return a4_dpp32(v, 0); }
__device__ __forceinline__ double a4_shl6(double v) { return a4_dpp32(v, 1); }
struct A4Vec {
  double lo, h16, h17;
};
// acc += (lane n of the row's v) * coef: v_fmac_f64_dpp with the broadcast fused (DP DPP takes only
// row_newbcast); the asm opens with the two wait states a DPP read of a VGPR a VALU just wrote
// needs (the compiler pads no asm).  BM: the lanes written (bank b = lanes 4b..4b+3 of every row);
// masked lanes keep their sums.
// sum_{l < 16} coef[l] * v_l as four interleaved chains (l mod 4), combined (a0 + a1) + (a2 + a3):
// the device's and the port's order (oracle/cpp/i7m_cpu.cpp adm_dot16).  TRI 1: lane c takes
// terms l <= c only (a lower-triangular row: the terms of a group of four past lane c's bank are
// masked, those inside it read the row's zero padding); TRI 2: terms l >= c only (a column).  One
// asm statement: the compiler can put nothing between the fma's, so one pair of wait states (for
// a DPP read of v just written) serves all sixteen.
template <int TRI = 0>
__device__ __forceinline__ double a4_dot16(double v, const double* cf) {
  constexpr int M0 = TRI == 1 ? 0xf : TRI == 2 ? 0x1 : 0xf, M1 = TRI == 1 ? 0xe : TRI == 2 ? 0x3 : 0xf;
  constexpr int M2 = TRI == 1 ? 0xc : TRI == 2 ? 0x7 : 0xf, M3 = TRI == 1 ? 0x8 : 0xf;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#define A4_F(acc, op, n, m) "v_fmac_f64_dpp " acc ", %4, " op " row_newbcast:" #n " row_mask:0xf bank_mask:" m "\n\t"
  asm volatile(
      "s_nop 1\n\t"
      A4_F("%0", "%5", 0, "%21") A4_F("%1", "%6", 1, "%21") A4_F("%2", "%7", 2, "%21") A4_F("%3", "%8", 3, "%21")
      A4_F("%0", "%9", 4, "%22") A4_F("%1", "%10", 5, "%22") A4_F("%2", "%11", 6, "%22") A4_F("%3", "%12", 7, "%22")
      A4_F("%0", "%13", 8, "%23") A4_F("%1", "%14", 9, "%23") A4_F("%2", "%15", 10, "%23") A4_F("%3", "%16", 11, "%23")
      A4_F("%0", "%17", 12, "%24") A4_F("%1", "%18", 13, "%24") A4_F("%2", "%19", 14, "%24") A4_F("%3", "%20", 15, "%24")
      : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
      : "v"(v), "v"(cf[0]), "v"(cf[1]), "v"(cf[2]), "v"(cf[3]), "v"(cf[4]), "v"(cf[5]), "v"(cf[6]), "v"(cf[7]),
        "v"(cf[8]), "v"(cf[9]), "v"(cf[10]), "v"(cf[11]), "v"(cf[12]), "v"(cf[13]), "v"(cf[14]), "v"(cf[15]),
        "i"(M0), "i"(M1), "i"(M2), "i"(M3));
#undef A4_F
  return __dadd_rn(__dadd_rn(a0, a1), __dadd_rn(a2, a3));
}
// sum_{r = 6..11} coef[r - 6] * u_r as two chains (r even / odd), combined
__device__ __forceinline__ double a4_dot6(double u, const double* cf) {
  double a0 = 0.0, a1 = 0.0;
  asm volatile(
      "s_nop 1\n\t"
      "v_fmac_f64_dpp %0, %2, %3 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %1, %2, %4 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %2, %5 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %1, %2, %6 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %2, %7 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %1, %2, %8 row_newbcast:11 row_mask:0xf bank_mask:0xf"
      : "+v"(a0), "+v"(a1)
      : "v"(u), "v"(cf[0]), "v"(cf[1]), "v"(cf[2]), "v"(cf[3]), "v"(cf[4]), "v"(cf[5]));
  return __dadd_rn(a0, a1);
}
// sum over the row's 16 lanes of cf_c v_c (a pairwise tree: lane 15 gathers lanes 14, 12-13, 8-11,
// 0-7 by row_shr 1, 2, 4, 8; the first level fma(cf_c, v_c, p_{c-1})), broadcast to the row: the
// port's adm_rowsum order.  (bound_ctrl: lanes below the shift read 0; only lane 15 is kept)
template <int n>
__device__ __forceinline__ double a4_shr(double v) {
  const long long u = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)u, 0x110 + n, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), 0x110 + n, 0xf, 0xf, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double a4_rowsum(double cf, double v) {
  double p = __fma_rn(cf, v, a4_shr<1>(__dmul_rn(cf, v)));
  p = __dadd_rn(p, a4_shr<2>(p));
  p = __dadd_rn(p, a4_shr<4>(p));
  p = __dadd_rn(p, a4_shr<8>(p));
  return a4_bc<15>(p);
}
// A stage's coefficients, read from the ring slot in four sets, each just before the phase ahead
// of the one that uses it (the reads stay where they are written: the fma asm is volatile).  R is
// the problem's record in the slot.
struct A4CJ {
  double Jt[6], J16[6], J17[6], Jd;  // J column c (rows 6..11), columns 16, 17 (rows 6..11), J[c % 6][c]
};
struct A4CL {
  double L[16];          // Linv row c (l < 16; the entries past the padded row are never used)
  double Lc16, Lc17;     // Linv[16][c], Linv[17][c]
  double d66, d76, d77;  // Linv[16][16], Linv[17][16], Linv[17][17]
};
struct A4CT {
  double Lt[16];  // Linv column c (rows l < 16; rows whose padded width ends before c are never used)
};
struct A4CR {
  double Jr[18], Jq0, Jq1;  // J row c (v rows 6..11; clamped outside them), J[q][q], J[q][6 + q] (q = c < 6 ? c : 0)
};
__device__ __forceinline__ void a4_ldj(A4CJ& C, const double* R, int c) {
  const double* J = R + A5_LJ;  // [J[i][i] (6) | J[i][6 + i] (6) | v rows 6 x 18]
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    C.Jt[r] = J[12 + 18 * r + c];
    C.J16[r] = J[12 + 18 * r + 16];
    C.J17[r] = J[12 + 18 * r + 17];
  }
  C.Jd = c < 12 ? J[c] : 0.0;
}
__device__ __forceinline__ void a4_ldl(A4CL& C, const double* R, const double* Rrow, int c) {
#pragma unroll
  for (int l = 0; l < 16; ++l) C.L[l] = Rrow[l];
  C.Lc16 = R[160 + c];
  C.Lc17 = R[178 + c];
  C.d66 = R[176];
  C.d76 = R[194];
  C.d77 = R[195];
}
// row l's entry c: R + adm_lrow(l) + c (adm_lrow a constant per l)
__device__ __forceinline__ void a4_ldt(A4CT& C, const double* R, int c) {
  constexpr int rs[16] = {0, 4, 8, 12, 16, 24, 32, 40, 48, 60, 72, 84, 96, 112, 128, 144};
#pragma unroll
  for (int l = 0; l < 16; ++l) C.Lt[l] = R[rs[l] + c];
}
__device__ __forceinline__ void a4_ldr(A4CR& C, const double* R, int c) {
  const double* J = R + A5_LJ;
  const int rr = c < 6 ? 0 : (c < 12 ? c - 6 : 5);
#pragma unroll
  for (int l = 0; l < 18; ++l) C.Jr[l] = J[12 + 18 * rr + l];
  const int q = c < 6 ? c : 0;
  C.Jq0 = J[q];
  C.Jq1 = J[6 + q];
}
// y = Linv v (rows 16, 17: the row sums of Linv[16 or 17][c] v_c, then the (16, 17) block)
__device__ __forceinline__ A4Vec a4_lmul(const A4CL& C, const A4Vec& v) {
  const double lo = a4_dot16<1>(v.lo, C.L);
  const double s16 = a4_rowsum(C.Lc16, v.lo), s17 = a4_rowsum(C.Lc17, v.lo);
  const double b16 = __fma_rn(C.d66, v.h16, s16);
  const double b17 = __fma_rn(C.d77, v.h17, __fma_rn(C.d76, v.h16, s17));
  return {lo, b16, b17};
}
// y = Linv' v
__device__ __forceinline__ A4Vec a4_ltmul(const A4CL& L, const A4CT& C, const A4Vec& v) {
  double lo = a4_dot16<2>(v.lo, C.Lt);
  lo = __fma_rn(L.Lc16, v.h16, lo);
  lo = __fma_rn(L.Lc17, v.h17, lo);
  return {lo, __fma_rn(L.d76, v.h17, __dmul_rn(L.d66, v.h16)), __dmul_rn(L.d77, v.h17)};
}
// init + J' u: the q-row entry of column c (J[c % 6][c], zero for c >= 12) with u[c % 6], plus the
// v rows 6..11 (two chains); u in lanes 0..11, every lane's finite
__device__ __forceinline__ A4Vec a4_jtmul(const A4CJ& C, double u, A4Vec init) {
  const double us = a4_shr6(u);  // u[c - 6] for c >= 6, own below
  const double lo = __dadd_rn(__fma_rn(C.Jd, us, init.lo), a4_dot6(u, C.Jt));
  return {lo, __dadd_rn(init.h16, a4_dot6(u, C.J16)), __dadd_rn(init.h17, a4_dot6(u, C.J17))};
}
// (J v)_c, c < 12 (lanes 12-15: row 11's, unused)
__device__ __forceinline__ double a4_jmul(const A4CR& C, int c, const A4Vec& v) {
  double a = a4_dot16(v.lo, C.Jr);
  a = __fma_rn(C.Jr[16], v.h16, a);
  a = __fma_rn(C.Jr[17], v.h17, a);
  const double sp = __fma_rn(C.Jq1, a4_shl6(v.lo), __dmul_rn(C.Jq0, v.lo));
  return c < 6 ? sp : a;
}

typedef unsigned int a4u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double a5_ld(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
}
__device__ __forceinline__ void a5_st(double v, __amdgpu_buffer_rsrc_t r, unsigned off) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(a4u2, v), r, off, 0, 0);
}
// one step's DMA: 10 record wave-instructions (per-lane offsets ro[t], the stage in soffset) and 3
// vector ones (per-lane offsets vo[u]), to the slot at LDS byte address `lds`.  The instruction
// offset moves the LDS destination as well as the source (tools/probes/lds_dma_offset_probe), so
// M0 (saved and restored around) steps by 4 KB every four wave-instructions and the per-lane
// offsets carry -1 KB (t mod 4) (a5_dma_off).
__device__ __forceinline__ unsigned a5_dma_off(int t) { return 1024u * (unsigned)(t & 3); }
__device__ __forceinline__ void a5_dma(__amdgpu_buffer_rsrc_t r, unsigned lds, const unsigned (&ro)[A5_RI], unsigned so,
                                       const unsigned (&vo)[A5_VI]) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %2, %15, %16 offen lds\n\t"
      "buffer_load_dwordx4 %3, %15, %16 offen offset:1024 lds\n\t"
      "buffer_load_dwordx4 %4, %15, %16 offen offset:2048 lds\n\t"
      "buffer_load_dwordx4 %5, %15, %16 offen offset:3072 lds\n\t"
      "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %6, %15, %16 offen lds\n\t"
      "buffer_load_dwordx4 %7, %15, %16 offen offset:1024 lds\n\t"
      "buffer_load_dwordx4 %8, %15, %16 offen offset:2048 lds\n\t"
      "buffer_load_dwordx4 %9, %15, %16 offen offset:3072 lds\n\t"
      "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %10, %15, %16 offen lds\n\t"
      "buffer_load_dwordx4 %11, %15, %16 offen offset:1024 lds\n\t"
      "buffer_load_dwordx4 %12, %15, 0 offen offset:2048 lds\n\t"
      "buffer_load_dwordx4 %13, %15, 0 offen offset:3072 lds\n\t"
      "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %14, %15, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(ro[0]), "v"(ro[1]), "v"(ro[2]), "v"(ro[3]), "v"(ro[4]), "v"(ro[5]), "v"(ro[6]), "v"(ro[7]),
        "v"(ro[8]), "v"(ro[9]), "v"(vo[0]), "v"(vo[1]), "v"(vo[2]), "s"(r), "s"(__builtin_amdgcn_readfirstlane(so))
      : "memory");
}
// the step's slot has landed: at most 13 vector-memory operations in flight (the next step's DMA,
// or the stores issued after its first ones: every operation completes in issue order)
__device__ __forceinline__ void a5_wait() { asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); }
// two problems per wave (k_admm_iter2): 5 record and 2 vector wave-instructions per step
__device__ __forceinline__ void a5_dma2(__amdgpu_buffer_rsrc_t r, unsigned lds, const unsigned (&ro)[5], unsigned so,
                                        const unsigned (&vo)[2]) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %2, %9, %10 offen lds\n\t"
      "buffer_load_dwordx4 %3, %9, %10 offen offset:1024 lds\n\t"
      "buffer_load_dwordx4 %4, %9, %10 offen offset:2048 lds\n\t"
      "buffer_load_dwordx4 %5, %9, %10 offen offset:3072 lds\n\t"
      "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %6, %9, %10 offen lds\n\t"
      "buffer_load_dwordx4 %7, %9, 0 offen offset:1024 lds\n\t"
      "buffer_load_dwordx4 %8, %9, 0 offen offset:2048 lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(ro[0]), "v"(ro[1]), "v"(ro[2]), "v"(ro[3]), "v"(ro[4]),
        "v"(vo[0]), "v"(vo[1]), "s"(r), "s"(__builtin_amdgcn_readfirstlane(so))
      : "memory");
}
__device__ __forceinline__ void a5_wait2() { asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); }
__device__ __forceinline__ void a5_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The termination test of problem bq on the iterate in global memory, by the 16-lane row of lane c
// (adm_check's operands from the handle's arrays); rho_est gets OSQP's rho estimate.  N, T, m are
// the caller's copies of the problem sizes: re-read from `a` here, k_admm_iter<false> measured
// 0.6 % slower at B = 4096 (register allocation, the sweep loops' instructions unchanged).
__device__ __forceinline__ bool a4_check(const AdmmArgs& a, int N, int T, int m, long bq, double c_cost, double rho,
                                         int c, double* rho_est, double es = 1.0) {
  return adm_check(a, N, T, m, c_cost, rho, a.sx + bq * T, a.sz + bq * m, a.sy + bq * m, a.qs + bq * T, a.ls + bq * m,
                   a.D + bq * T, a.E + bq * m, a.R + bq * N * ADM_REC + REC_J, a.I + bq * m, a.Pq + bq * N * 36,
                   a.Pd + bq * T, rho_est, c, es);
}
// OSQP after max_iter without a passed test (oracle/osqp_admm.py OSQP.solve, :344-349): the test
// once more at the final iterate unless the last iteration ran it, then the approximate test
// (eps x 10): status 1 solved, 2 solved inaccurate, 0 max_iter reached.  The iterate is unchanged.
// (`solved`: the row passed a test in the loop; it runs the tests with its wave all the same)
__device__ __forceinline__ int a4_closing_status(const AdmmArgs& a, int N, int T, int m, long bq, double c_cost,
                                                 double rho, int c, bool solved) {
  auto test = [&](double es) {
    double rest = rho;
    return a4_check(a, N, T, m, bq, c_cost, rho, c, &rest, es);
  };
  const bool last_checked = a.A.check && a.A.max_iter % a.A.check == 0;
  const bool exact = last_checked ? false : test(1.0);
  const bool approx = exact ? false : test(10.0);
  return solved ? 1 : (exact ? 1 : (approx ? 2 : 0));
}
// The problem's record of this QP (one lane: `lead`): rho carried, OSQP's iteration count and status
__device__ __forceinline__ void a4_finish(const AdmmArgs& a, long b, bool lead, double rho, bool solved, int done_it,
                                          int status) {
  if (lead) {
    a.srho[b] = rho;
    if (a.iters) a.iters[b * 8 + a.sqp_iter] = solved ? done_it : a.A.max_iter;
    if (a.status) a.status[b * 8 + a.sqp_iter] = status;
  }
}
// ... and the unscaled solution sol = D x, entries e0, e0 + stride, ... of the scaled x
__device__ __forceinline__ void a4_solution(const AdmmArgs& a, long b, const double* x, int e0, int stride) {
  const int T = a.P.T;
  const double* D = a.D + b * T;
  double* sol = a.sol + b * T;
  for (int e = e0; e < T; e += stride) sol[e] = D[e] * x[e];
}

// The diagnostic build's stamps of one sweep step (I7M_ABLATE 100000 + 100 IT + S, tools/
// step_stamps.py: step S of OSQP iteration IT in workgroup 0); nothing in the release build.
struct A5Stamps {
#ifdef I7M_DIAG
  unsigned long long t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int it, s;        // the traced iteration (-1: none) and step
  bool on = false;  // the running step is the traced one
  __device__ __forceinline__ explicit A5Stamps(int ablate)
      : it(ablate >= 100000 && ablate < 200000 && blockIdx.x == 0 ? (ablate - 100000) / 100 : -1), s(ablate % 100) {}
  __device__ __forceinline__ void step(int i, int st) { on = i == it && st == s; }
  __device__ __forceinline__ void write(int ablate, int layout) const {
    if (it >= 0) tl_write_stamps(t, 9, ablate, layout);
  }
#else
  __device__ __forceinline__ explicit A5Stamps(int) {}
  __device__ __forceinline__ void step(int, int) {}
  __device__ __forceinline__ void write(int, int) const {}
#endif
};
#define A5_STAMP(st, i) I7M_STAMP((st).t, i, (st).on)

// ---- one sweep step's arithmetic, shared by admm_iter4 and admm_iter_res ---------------------
// A lane's constants (row c of its problem's stage vectors; rv = 1e3 rho on the equality rows, ri
// its inverse), a step's operands (v0, v1 with their u-part pairs hv0, hv1: x_k and q_k forward,
// h_k and x_{k+1} backward; block k+1's rows z1, y1, l1 and I entry ib1), its coefficient sets read
// from the record R, and what the steps carry (hc: forward J_{k-1} h_{k-1} in lanes 0..11,
// backward xt_{k+1}; block k's t and I entry; block 0's rows and x_0, the epilogue's alone).
struct A4K {
  int c;
  bool lo12;  // c < 12: a row of a 12-row block
  double rv, ri, sg, al, al1;
};
struct A4Op {
  double v0, v1, z1, y1, l1, ib1;
  double2 hv0, hv1;
};
struct A4Co {
  A4CJ J;
  A4CL L;
  A4CT T;
  A4CR Jr;
  const double* R;
};
struct A4Carry {
  A4Vec hc;
  double tk, ibk;
  double b0z, b0y, b0l, b0i, nx0;
  double2 nx0h;
};
// a block's rows after OSQP's relaxation, projection and dual update, and the relaxed x
struct A4New {
  double zn, yn, xn, xn16, xn17;
};
// t = rho_vec (z - y / rho_vec) of a block's rows (the right-hand side's A' part)
__device__ __forceinline__ double a4_t(const A4K& K, double z, double y) {
  return __dmul_rn(K.rv, __dsub_rn(z, __dmul_rn(K.ri, y)));
}
// the first two coefficient sets of a step (the other two are read behind the products ahead of
// their use: a4_llt)
__device__ __forceinline__ void a4_coef_begin(A4Co& C, const double* R, int c) {
  C.R = R;
  a4_ldj(C.J, R, c);
  a4_ldl(C.L, R, R + a5_lrow(c), c);
}
// Linv' Linv r, with J's row set read behind the first product when `jr` (stamps SB .. SB + 2)
template <int SB>
__device__ __forceinline__ A4Vec a4_llt(A4Co& C, const A4Vec& r, bool jr, int c, A5Stamps& st) {
  A5_STAMP(st, SB);
  a4_ldt(C.T, C.R, c);
  const A4Vec y = a4_lmul(C.L, r);
  A5_STAMP(st, SB + 1);
  if (jr) a4_ldr(C.Jr, C.R, c);
  const A4Vec o = a4_ltmul(C.L, C.T, y);
  A5_STAMP(st, SB + 2);
  return o;
}
// forward step k < N - 1: rhs, g, h = Linv' Linv g (put(h) stores it), the next coupling J_k h
template <int SB, class Put>
__device__ __forceinline__ void a4_forward(const A4K& K, const A4Op& o, A4Co& C, A4Carry& S, A5Stamps& st, Put&& put) {
  const double t1 = a4_t(K, o.z1, o.y1);
  const double init = K.lo12 ? __dmul_rn(S.ibk, S.tk) : 0.0;
  A4Vec r = a4_jtmul(C.J, t1, A4Vec{init, 0.0, 0.0});
  r.lo = __dadd_rn(__dsub_rn(__dmul_rn(K.sg, o.v0), o.v1), r.lo);
  r.h16 = __dadd_rn(__dsub_rn(__dmul_rn(K.sg, o.hv0.x), o.hv1.x), r.h16);
  r.h17 = __dadd_rn(__dsub_rn(__dmul_rn(K.sg, o.hv0.y), o.hv1.y), r.h17);
  const double rc = __dsub_rn(r.lo, __dmul_rn(__dmul_rn(K.rv, S.ibk), S.hc.lo));  // k = 0: hc = 0
  r.lo = K.lo12 ? rc : r.lo;
  const A4Vec h = a4_llt<SB>(C, r, true, K.c, st);
  put(h);
  A5_STAMP(st, SB + 3);
  S.hc.lo = a4_jmul(C.Jr, K.c, h);
  S.tk = t1;
  S.ibk = o.ib1;
  A5_STAMP(st, SB + 4);
}
// the last forward step (k = N - 1: 12 rows, no J, no u-part); the backward sweep starts from
// xt_{N-1} = h_{N-1}, left in hc
template <int SB>
__device__ __forceinline__ void a4_forward_last(const A4K& K, const A4Op& o, A4Co& C, A4Carry& S, A5Stamps& st) {
  A4Vec r{K.lo12 ? __dmul_rn(S.ibk, S.tk) : 0.0, 0.0, 0.0};
  r.lo = __dadd_rn(__dsub_rn(__dmul_rn(K.sg, o.v0), o.v1), r.lo);
  r.lo = __dsub_rn(r.lo, __dmul_rn(__dmul_rn(K.rv, S.ibk), S.hc.lo));
  r.lo = K.lo12 ? r.lo : 0.0;
  S.hc = a4_llt<SB>(C, r, false, K.c, st);
}
// OSQP's relaxation (alpha), projection onto [l, u] = {l} and dual update of a block's rows from
// z~ = zt, and the relaxed x from x~ = xt
__device__ __forceinline__ A4New a4_relax(const A4K& K, double zt, double z, double y, double l, const A4Vec& xt, double x,
                                          double x16, double x17) {
  const double zr = __dadd_rn(__dmul_rn(K.al, zt), __dmul_rn(K.al1, z));
  double zn = __dadd_rn(zr, __dmul_rn(K.ri, y));
  zn = fmin(fmax(zn, l), l);
  const double yn = __dadd_rn(y, __dmul_rn(K.rv, __dsub_rn(zr, zn)));
  const double xn = __dadd_rn(__dmul_rn(K.al, xt.lo), __dmul_rn(K.al1, x));
  const double xn16 = __dadd_rn(__dmul_rn(K.al, xt.h16), __dmul_rn(K.al1, x16));
  const double xn17 = __dadd_rn(__dmul_rn(K.al, xt.h17), __dmul_rn(K.al1, x17));
  return {zn, yn, xn, xn16, xn17};
}
// backward step k < N - 1: xt_k, then block k+1's rows and x_{k+1} (put(n) stores them)
template <int SB, class Put>
__device__ __forceinline__ void a4_backward(const A4K& K, const A4Op& o, A4Co& C, A4Carry& S, A5Stamps& st, Put&& put) {
  const double u = __dmul_rn(__dmul_rn(K.rv, o.ib1), S.hc.lo);
  const A4Vec s2 = a4_llt<SB>(C, a4_jtmul(C.J, u, A4Vec{0.0, 0.0, 0.0}), true, K.c, st);
  const A4Vec xt{__dsub_rn(o.v0, s2.lo), __dsub_rn(o.hv0.x, s2.h16), __dsub_rn(o.hv0.y, s2.h17)};
  const double zt = __dadd_rn(a4_jmul(C.Jr, K.c, xt), __dmul_rn(o.ib1, S.hc.lo));
  A5_STAMP(st, SB + 3);
  put(a4_relax(K, zt, o.z1, o.y1, o.l1, S.hc, o.v1, o.hv1.x, o.hv1.y));
  S.hc = xt;
  A5_STAMP(st, SB + 4);
}
// The sweep's epilogue: block 0's rows (z~ = I xt_0) and x_0 (put(n) stores them), then tk, ibk and
// hc for the next forward sweep.  Block 0's rows and x_0 ride in registers from epilogue to
// epilogue in both kernels: the resident kernel holds the same x_0 in LDS, but the compiler's
// fusing of the epilogue's products into its sum follows where the operand comes from, and read
// from LDS x_0's update rounded differently in the last place.
template <class Put>
__device__ __forceinline__ void a4_block0(const A4K& K, A4Carry& S, Put&& put) {
  const double zt = __dmul_rn(S.b0i, S.hc.lo);
  const A4New n = a4_relax(K, zt, S.b0z, S.b0y, S.b0l, S.hc, S.nx0, S.nx0h.x, S.nx0h.y);
  put(n);
  S.nx0 = n.xn;
  S.nx0h = make_double2(n.xn16, n.xn17);
  S.b0z = n.zn;
  S.b0y = n.yn;
  S.tk = a4_t(K, n.zn, n.yn);
  S.ibk = S.b0i;
  S.hc = A4Vec{0.0, 0.0, 0.0};
}

// OSQP's iteration loop of one wave (PW problems: 4, or 2 in k_admm_iter2, whose rows 2 and 3 idle
// so that the ring takes 21 KB and two waves can share a SIMD).  Per-lane state lives in registers.
template <bool ADAPT, int PW = 4>
__device__ __forceinline__ void admm_iter4(const AdmmArgs& a) {
  static_assert(PW == 4 || PW == 2, "four or two problems per wave");
  constexpr int RI = PW == 4 ? A5_RI : 5, VI = PW == 4 ? A5_VI : 2;  // record / vector DMA wave-instructions
  constexpr int SLOT = 64 * (RI + VI), VD = 2 * 64 * RI;
  constexpr int PL = PW - 1;  // the last real row (idle rows read its slot data)
  const SolveParams& P = a.P;
  const int N = P.N, T = P.T, m = 12 * N;
  const int l = threadIdx.x, p = l >> 4, c = l & 15;
  __shared__ double2 sRing[3 * SLOT];
  double* const ring = (double*)sRing;
  const unsigned ring_lds = (unsigned)(unsigned long)(__attribute__((address_space(3))) void*)sRing;
  const int bb = a.b0 + PW * (int)blockIdx.x;
  // the step stamps: start, slot landed, next DMA issued, reads issued, right-hand side, Linv r,
  // Linv' y, stores, end
  A5Stamps st(a.ablate);
  bool run = p < PW && bb + p < P.B && !(a.active && !a.active[bb + p]);
  const bool act = run;
  if (!__ballot(run)) return;
  // (idle rows shadow row PL's problem and rows past the batch the first one's: what they read and
  // discard belongs to this workgroup, not to one that is storing it)
  const int bown = bb + (p < PW ? p : PL), bq = bown < P.B ? bown : bb;
  // one resource over the whole allocation; every array as a byte offset in it
  const auto rA = a4_rsrc(a.abase, a.abytes);
  auto boff = [&](const double* q) { return (unsigned)__builtin_amdgcn_readfirstlane((int)((const char*)q - (const char*)a.abase)); };
  const unsigned oX = boff(a.sx), oZ = boff(a.sz), oY = boff(a.sy), oQ = boff(a.qs), oL = boff(a.ls), oI = boff(a.I);
  const unsigned oH = boff(a.w), oR = boff(a.R);
  // this lane's own rows (stores, the block-0 epilogue)
  const unsigned xT = oX + 8u * (unsigned)(bown * T), hT = oH + 8u * (unsigned)(bown * T);
  const unsigned zM = oZ + 8u * (unsigned)(bown * m), yM = oY + 8u * (unsigned)(bown * m);
  const unsigned lM = oL + 8u * (unsigned)(bown * m), iM = oI + 8u * (unsigned)(bown * m);
  const double c_cost = a.cs[bq];
  double rho = a.srho[bq];
  A4K K{c, c < 12, 1e3 * rho, 1.0 / (1e3 * rho), a.A.sigma, a.A.alpha, 1.0 - a.A.alpha};
  const int cc = c < 12 ? c : 11;
  const int c16 = 16 + (c & 1);  // lanes 0, 1 store the u-part pair (16, 17)
  const bool lo12 = K.lo12, lo2 = c < 2;
  // DMA source offsets of this lane's pieces (rows that do not run read nothing: out of range).
  // Records: piece g = 64 t + l of the four problems' 632; vectors: piece g = 64 u + l of their
  // 168, problem g / 42 piece j = g % 42: [0, 9) v0, [9, 18) v1, [18, 42) z, y, l, I (6 each).
  unsigned ro[RI], vF[VI], vB[VI], vD[VI], vZ[VI], vo[VI];
  int vcls[VI];
  auto offsets = [&]() {
    const unsigned long long rm = __ballot(run);
#pragma unroll
    for (int t = 0; t < RI; ++t) {
      const int g = 64 * t + l, q = g / A5_RP, j = g - A5_RP * q;
      const bool ok = q < PW && ((rm >> (16 * q)) & 1);
      // LDS piece j of the record -> its piece in HBM (rows 0-15 from width 4 to the stored even
      // width: the pieces past it read as zeros)
      int hp;
      if (j < 80) {
        int r = 0;
#pragma unroll
        for (int i = 1; i < 16; ++i) r = 2 * j >= a5_lrow(i) ? i : r;
        const int cp = 2 * j - a5_lrow(r);
        hp = cp < adm_lw(r) ? (adm_lrow(r) + cp) / 2 : -1;
      } else {
        hp = j - 8;  // rows 16, 17 and J: HBM piece 72 + (j - 80) / 90 + (j - 98)
      }
      ro[t] = (ok && hp >= 0 ? oR + 8u * (unsigned)((bb + q) * N * ADM_REC) + 16u * hp : A5_OOB) - a5_dma_off(t);
    }
#pragma unroll
    for (int u = 0; u < VI; ++u) {
      const int g = 64 * u + l, q = g / A5_VP, j = g - A5_VP * q;
      const bool ok = q < PW && ((rm >> (16 * q)) & 1);
      const unsigned rT = 8u * (unsigned)((bb + q) * T), rM = 8u * (unsigned)((bb + q) * m);
      unsigned f, bk;
      int cl;
      if (j < 9) {
        f = oX + rT + 16u * j; bk = oH + rT + 16u * j; cl = 0;
      } else if (j < 18) {
        f = oQ + rT + 16u * (j - 9); bk = oX + rT + 16u * (j - 9); cl = 1;
      } else {
        const int jj = j - 18, w = jj / 6;
        f = (w == 0 ? oZ + 0u : w == 1 ? oY + 0u : w == 2 ? oL + 0u : oI + 0u) + rM + 16u * (jj - 6 * w);
        bk = f; cl = w == 0 ? 3 : 2;
      }
      const unsigned o = a5_dma_off(RI + u);
      vF[u] = (ok ? f : A5_OOB) - o;
      vB[u] = (ok ? bk : A5_OOB) - o;
      vD[u] = ok ? (cl < 2 ? 144u : 96u) : 0u;  // bytes per stage
      vZ[u] = ok && cl == 3 ? oL - oZ : 0u;     // z's pieces from l's lines
      vcls[u] = cl;
    }
  };
  offsets();
  // step s's vector offsets from scratch (s < 2N): forward: x_k, q_k; backward: h_k, x_{k+1};
  // both: block k+1's z, y, l, I (the last stage's missing block reads block N-1's, unused).
  // (zl: the step is past the first iteration, where z = l: every block's projection onto its
  // equality rows, fmin(fmax(., l), l), is l itself, so z's pieces come from l's lines)
  auto vfull = [&](int s, bool zl) {
    const bool fwd = s < N;
    const int k = fwd ? s : 2 * N - 1 - s;
    const int k1 = k + 1 < N ? k + 1 : N - 1;
    const int kb = fwd ? k : k1;
#pragma unroll
    for (int u = 0; u < VI; ++u) {
      const unsigned st = vcls[u] == 0 ? 144u * k : (vcls[u] == 1 ? 144u * kb : 96u * k1);
      vo[u] = (fwd ? vF[u] + 0u : vB[u] + 0u) + (zl ? vZ[u] + st : st);
    }
  };
  // issue step s's DMA into ring slot `slot`: the vector offsets advance by one stage (forward
  // steps 1..N-2 and backward steps N+2.. are the previous step's one stage on) or are recomputed
  auto issue = [&](int s, int slot, bool zl) {
    const bool fwd = s < N;
    const int k = fwd ? s : 2 * N - 1 - s;
    if (s == 0 || s == N - 1 || s == N || s == N + 1) {
      vfull(s, zl);
    } else {
#pragma unroll
      for (int u = 0; u < VI; ++u) vo[u] = fwd ? vo[u] + vD[u] : vo[u] - vD[u];
    }
#ifdef I7M_DIAG
    // I7M_ABLATE 21: every step reads stage 0's record (L2-resident: the sweep without its stream)
    const unsigned so = 8u * (unsigned)(a.ablate == 21 ? 0 : k * ADM_REC);
#else
    const unsigned so = 8u * (unsigned)(k * ADM_REC);
#endif
    if constexpr (PW == 4)
      a5_dma(rA, ring_lds + 16u * SLOT * slot, ro, so, vo);
    else
      a5_dma2(rA, ring_lds + 16u * SLOT * slot, ro, so, vo);
  };
  issue(0, 0, false);
  issue(1, 1, false);
  int it = 1;
  // carried between steps; block 0's rows and x_0 (only the epilogue updates them)
  A4Carry S;
  S.hc = A4Vec{0.0, 0.0, 0.0};
  S.b0z = a5_ld(rA, zM + 8 * cc);
  S.b0y = a5_ld(rA, yM + 8 * cc);
  S.b0l = a5_ld(rA, lM + 8 * cc);
  S.b0i = a5_ld(rA, iM + 8 * cc);
  S.nx0 = a5_ld(rA, xT + 8 * c);
  S.nx0h = make_double2(a5_ld(rA, xT + 8 * 16), a5_ld(rA, xT + 8 * 17));
  S.tk = a4_t(K, S.b0z, S.b0y);
  S.ibk = S.b0i;
  // the state the backward sweep hands to the next forward sweep's first two steps (their DMA was
  // issued before the sweep wrote it)
  double nx1 = 0.0, nz1 = 0.0, ny1 = 0.0;
  double2 nx1h = make_double2(0.0, 0.0);
  int done_it = 0;
  bool solved = false;
  A4Op o;
  A4Co C;
  // one step's start: wait for its slot, issue step s + 2's DMA into the slot step s - 1 used, read
  // the step's vectors (rows ci of v0, cb of v1: the last stage's 12 rows clamped) and the first
  // two coefficient sets
  auto begin = [&](int s, int slot, int ci, int cb) {
    st.step(it, s);
    A5_STAMP(st, 0);
    if constexpr (PW == 4)
      a5_wait();
    else
      a5_wait2();
    A5_STAMP(st, 1);
    int sn = s + 2, sl = slot + 2;
    if (sn >= 2 * N) sn -= 2 * N;
    if (sl >= 3) sl -= 3;
    issue(sn, sl, it > 1 || sn < s);
    A5_STAMP(st, 2);
    const double* Sl = ring + 2 * SLOT * slot;
    const double* V = Sl + VD + 2 * A5_VP * (p < PW ? p : PL);  // [v0 18 | v1 18 | z 12 | y 12 | l 12 | I 12]
    o.v0 = V[ci];
    o.v1 = V[18 + cb];
    o.hv0 = make_double2(V[16], V[17]);
    o.hv1 = make_double2(V[34], V[35]);
    o.z1 = V[36 + cc];
    o.y1 = V[48 + cc];
    o.l1 = V[60 + cc];
    o.ib1 = V[72 + cc];
    a4_coef_begin(C, Sl + A5_LREC * (p < PW ? p : PL), c);
    A5_STAMP(st, 3);
  };
  // store offsets: masked (past the range) for rows that do not run
  auto so = [&](bool ok, unsigned off) { return run && ok ? off + 0u : A5_OOB + 0u; };
  // forward step k < N - 1: h_k to the scratch vector
  auto fwd = [&](int k) {
    a4_forward<4>(K, o, C, S, st, [&](const A4Vec& h) {
      a5_st(h.lo, rA, so(true, hT + 8u * (18 * k + c)));
      a5_st(c == 0 ? h.h16 + 0.0 : h.h17 + 0.0, rA, so(lo2, hT + 8u * (18 * k + c16)));
    });
  };
  // the last forward step (k = N - 1)
  auto fwd_last = [&]() {
    a4_forward_last<4>(K, o, C, S, st);
    a5_st(S.hc.lo, rA, so(lo12, hT + 8u * (18 * (N - 1) + c)));
  };
  // backward step k < N - 1: block k+1's rows and x_{k+1} to the carried state
  auto bwd = [&](int k) {
    a4_backward<4>(K, o, C, S, st, [&](const A4New& n) {
      const bool last1 = k + 1 == N - 1;  // x_{k+1} has no u-part
      const unsigned ob = 8u * (12 * (k + 1) + c);
      a5_st(n.zn, rA, so(lo12 && it == 1, zM + ob));  // (l from the second iteration on: already stored)
      a5_st(n.yn, rA, so(lo12, yM + ob));
      a5_st(n.xn, rA, so(!last1 || lo12, xT + 8u * (18 * (k + 1) + c)));
      a5_st(c == 0 ? n.xn16 + 0.0 : n.xn17 + 0.0, rA, so(!last1 && lo2, xT + 8u * (18 * (k + 1) + c16)));
      if (k == 0) {
        nx1 = n.xn;
        nx1h = make_double2(n.xn16, n.xn17);
        nz1 = n.zn;
        ny1 = n.yn;
      }
    });
  };
  // an iteration's 2N steps (ring slot `slot` = the step count mod 3): forward k = s < N - 1, the
  // last forward step (s = N - 1), the backward sweep's start (s = N: xt_{N-1} = h_{N-1}, already in
  // hc), backward k = 2N - 1 - s; each segment a loop of its own (no per-step dispatch)
  int slot = 0;
  auto next = [&]() { slot = slot == 2 ? 0 : slot + 1; };
  for (; it <= a.A.max_iter; ++it) {
    for (int s = 0; s < N - 1; ++s) {
      begin(s, slot, c, c);
      if (it > 1 && s == 0) {
        o.v0 = S.nx0; o.hv0 = S.nx0h; o.z1 = nz1; o.y1 = ny1;
      }
      if (it > 1 && s == 1) {
        o.v0 = nx1; o.hv0 = nx1h;
      }
      fwd(s);
      next();
    }
    begin(N - 1, slot, cc, cc);
    if (it > 1 && N == 2) o.v0 = nx1;  // (N = 2: the last forward step is stage 1)
    fwd_last();
    next();
    begin(N, slot, cc, cc);
    next();
    for (int s = N + 1; s < 2 * N; ++s) {
      begin(s, slot, c, s == N + 1 ? cc : c + 0);
      bwd(2 * N - 1 - s);
      next();
    }
    a4_block0(K, S, [&](const A4New& n) {
      a5_st(n.zn, rA, so(lo12 && it == 1, zM + 8u * c));
      a5_st(n.yn, rA, so(lo12, yM + 8u * c));
      a5_st(n.xn, rA, so(true, xT + 8u * c));
      a5_st(c == 0 ? n.xn16 + 0.0 : n.xn17 + 0.0, rA, so(lo2, xT + 8u * c16));
    });
    const bool chk = a.A.check && it % a.A.check == 0;
    const bool adapt = ADAPT && a.A.adapt_interval && it % a.A.adapt_interval == 0;
    if (chk || adapt) {
      a5_drain();
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      double rest = rho;
      const bool ok = a4_check(a, N, T, m, bq, c_cost, rho, c, &rest);
      bool fin = false;
      if (chk && ok && run) {
        run = false;
        solved = true;
        done_it = it;
        fin = true;
      }
      bool reload = false;
      if constexpr (ADAPT) {
        const bool moved = run && adapt && (rest > rho * a.A.adapt_tol || rest < rho / a.A.adapt_tol);
        const unsigned long long mv = __ballot(moved);
        if (mv) {
          if (moved) {
            rho = rest;
            K.rv = 1e3 * rho;
            K.ri = 1.0 / K.rv;
          }
          // re-factor the rows whose rho moved, one problem at a time on the whole wave (the
          // ring is the factor's scratch)
          for (int q = 0; q < PW; ++q) {
            if (!((mv >> (16 * q)) & 0xffff)) continue;
            const long bq2 = bb + q;
            const double rq = __shfl(rho, 16 * q, 64);
            double* scr = ring;
            adm_factor(a, N, rq, a.Pq + bq2 * N * 36, a.Pd + bq2 * T, a.I + bq2 * m, a.R + bq2 * N * ADM_REC, scr,
                       scr + 30 * ADMM_FSTRIDE + 388, scr + 30 * ADMM_FSTRIDE, scr + 18 * ADMM_FSTRIDE,
                       scr + 2048, l);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          S.tk = a4_t(K, S.b0z, S.b0y);
          reload = true;
        }
      }
      if (!__ballot(run)) break;
      if (__ballot(fin)) {  // finished rows read nothing from here on
        offsets();
        vfull(1, true);  // (the running vector offsets: the last issued step's)
      }
      if (reload) {
        slot = 0;
        issue(0, 0, true);
        issue(1, 1, true);
      }
    }
  }
  a5_drain();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  // the closing tests of the rows that passed none (the whole wave runs them: uniform reductions)
  int st_v = solved ? 1 : 0;
  if (__ballot(act && !solved)) st_v = a4_closing_status(a, N, T, m, bq, c_cost, rho, c, solved);
  if (l == 0) st.write(a.ablate, 0);
  a4_finish(a, bown, c == 0 && act, rho, solved, done_it, st_v);
  if (act) a4_solution(a, bown, a.sx + (long)bown * T, c, 16);
}

// ---- k_admm_iter_res: one problem per wave, everything it reads resident in LDS -------------
// The streaming kernel's step issues 13 (or 7) LDS-DMA wave-instructions and 2-4 buffer stores,
// and a lone wave's step is bound by their issue (tools/step_stamps.py: ~400 of ~1700 cycles for
// the DMA, ~70 per store).  A launch of at most a CU's worth of problems has the LDS for a better
// layout: one problem per workgroup, its N stage records (the streaming ring's image, 2.5 KB per
// stage) and its vectors x, q, h, z, y, l, I (0.8 KB per stage) copied into LDS once, the sweeps
// reading and writing LDS only (no DMA, no vector-memory wait in the loop), the vectors written
// back before each termination test (which reads global memory) and at the end.  All four 16-lane
// rows compute the problem (identical values to identical LDS addresses), so no lane is masked.
// The same operations in the same order as admm_iter4 (bit-identical: its register patches for
// data the ring loaded before the sweep wrote it read the same values from LDS here, except block
// 1's z, which the ring takes from l's lines after the first iteration, as here).  Horizons up to
// ARES_N (N = 32: 107 KB).
constexpr int ARES_N = 32;
__device__ __forceinline__ void a5_dma1(__amdgpu_buffer_rsrc_t r, unsigned lds, unsigned off) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %2, %3, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(off), "s"(r)
      : "memory");
}
template <int NR>
__device__ __forceinline__ void admm_iter_res(const AdmmArgs& a) {
  const SolveParams& P = a.P;
  const int N = P.N, T = P.T, m = 12 * N;
  const int l = threadIdx.x, c = l & 15;
  const int b = a.b0 + (int)blockIdx.x;
  if (b >= P.B || (a.active && !a.active[b])) return;
  __shared__ double2 sRec2[NR * A5_LREC / 2];
  __shared__ double2 sV2[(3 * 18 + 4 * 12) * NR / 2 + 8];
  double* const sRec = (double*)sRec2;
  double* const sX = (double*)sV2;  // x | q | h (18 per stage) | z | y | l | I (12 per stage) | 16 spare
  double* const sQ = sX + 18 * NR;
  double* const sH = sQ + 18 * NR;
  double* const sZ = sH + 18 * NR;
  double* const sY = sZ + 12 * NR;
  double* const sL = sY + 12 * NR;
  double* const sI = sL + 12 * NR;
  double* const sJunk = sI + 12 * NR;  // stores of lanes that have none
  auto lds = [](const void* q) { return (unsigned)(unsigned long)(__attribute__((address_space(3))) const void*)q; };
  const auto rA = a4_rsrc(a.abase, a.abytes);
  auto boff = [&](const double* q) { return (unsigned)__builtin_amdgcn_readfirstlane((int)((const char*)q - (const char*)a.abase)); };
  const unsigned oX = boff(a.sx + (long)b * T), oQ = boff(a.qs + (long)b * T), oZ = boff(a.sz + (long)b * m);
  const unsigned oY = boff(a.sy + (long)b * m), oL = boff(a.ls + (long)b * m), oI = boff(a.I + (long)b * m);
  const unsigned oR = boff(a.R + (long)b * N * ADM_REC);
  // the stage records, in the ring's image (piece j of a stage from its HBM piece, zeros past a
  // row's stored width), and the vectors; the stage-N-1 tails of x and q (never used) zeroed
  {
    const int np = N * A5_RP;
    for (int g0 = 0; g0 < np; g0 += 64) {
      const int g = g0 + l, k = g / A5_RP, j = g - A5_RP * k;
      int hp;
      if (j < 80) {
        int r = 0;
#pragma unroll
        for (int i = 1; i < 16; ++i) r = 2 * j >= a5_lrow(i) ? i : r;
        const int cp = 2 * j - a5_lrow(r);
        hp = cp < adm_lw(r) ? (adm_lrow(r) + cp) / 2 : -1;
      } else {
        hp = j - 8;
      }
      a5_dma1(rA, lds(sRec) + 16u * g0, g < np && hp >= 0 ? oR + 8u * (unsigned)(k * ADM_REC) + 16u * hp : A5_OOB);
    }
    auto copy = [&](double* dst, unsigned src, int n) {  // n doubles (even)
      for (int g0 = 0; g0 < n / 2; g0 += 64) a5_dma1(rA, lds(dst) + 16u * g0, g0 + l < n / 2 ? src + 16u * (g0 + l) : A5_OOB);
    };
    copy(sX, oX, T);
    copy(sQ, oQ, T);
    copy(sZ, oZ, m);
    copy(sY, oY, m);
    copy(sL, oL, m);
    copy(sI, oI, m);
    if (l < 6) {
      sX[T + l] = 0.0;
      sQ[T + l] = 0.0;
    }
    a5_drain();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  // the vectors the termination test reads, back to global memory (every lane a different entry)
  auto flush = [&]() {
    for (int e = l; e < T; e += 64) a5_st(sX[e], rA, oX + 8u * e);
    for (int e = l; e < m; e += 64) {
      a5_st(sZ[e], rA, oZ + 8u * e);
      a5_st(sY[e], rA, oY + 8u * e);
    }
    a5_drain();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  };
  const double c_cost = a.cs[b];
  const double rho = a.srho[b];
  const A4K K{c, c < 12, 1e3 * rho, 1.0 / (1e3 * rho), a.A.sigma, a.A.alpha, 1.0 - a.A.alpha};
  const int cc = c < 12 ? c : 11;
  const bool lo12 = K.lo12, lo2 = c < 2;
  double* const junk = sJunk + c;
  int it = 1;
  A4Carry S;
  S.hc = A4Vec{0.0, 0.0, 0.0};
  S.b0z = sZ[cc];
  S.b0y = sY[cc];
  S.b0l = sL[cc];
  S.b0i = sI[cc];
  S.nx0 = sX[c];
  S.nx0h = make_double2(sX[16], sX[17]);
  S.tk = a4_t(K, S.b0z, S.b0y);
  S.ibk = S.b0i;
  double nz1 = 0.0;
  int done_it = 0;
  bool solved = false;
  A4Op o;
  A4Co C;
  // the step stamps (tools/step_stamps.py --B 1): step start, its reads issued, right-hand side,
  // Linv r, Linv' y, stores, end
  A5Stamps st(a.ablate);
  // a step's operands (s: the step in admm_iter4's count): stage k's record, v0 / v1 (rows ci / cb)
  // from the given vectors, block k1's rows (z from l's lines after the first iteration), the first
  // two coefficient sets
  auto begin = [&](int s, int k, const double* V0, const double* V1, int k1, int ci, int cb) {
    st.step(it, s);
    A5_STAMP(st, 0);
    o.v0 = V0[ci];
    o.v1 = V1[cb];
    o.hv0 = make_double2(V0[16], V0[17]);
    o.hv1 = make_double2(V1[16], V1[17]);
    o.z1 = (it > 1 ? sL : sZ)[12 * k1 + cc];
    o.y1 = sY[12 * k1 + cc];
    o.l1 = sL[12 * k1 + cc];
    o.ib1 = sI[12 * k1 + cc];
    a4_coef_begin(C, sRec + A5_LREC * k, c);
    A5_STAMP(st, 1);
  };
  for (; it <= a.A.max_iter; ++it) {
    // forward steps k < N - 1: h_k to sH
    for (int k = 0; k < N - 1; ++k) {
      begin(k, k, sX + 18 * k, sQ + 18 * k, k + 1, c, c);
      if (it > 1 && k == 0) o.z1 = nz1;
      a4_forward<2>(K, o, C, S, st, [&](const A4Vec& h) {
        double* const H = sH + 18 * k;
        H[c] = h.lo;
        *(lo2 ? H + 16 + c : junk) = c == 0 ? h.h16 : h.h17;
      });
    }
    // the last forward step: xt_{N-1} = h_{N-1}, kept in registers
    begin(N - 1, N - 1, sX + 18 * (N - 1), sQ + 18 * (N - 1), N - 1, cc, cc);
    a4_forward_last<2>(K, o, C, S, st);
    // backward steps k = N - 2 .. 0: block k+1's rows and x_{k+1} to LDS
    for (int k = N - 2; k >= 0; --k) {
      const bool last1 = k + 1 == N - 1;  // x_{k+1} has no u-part
      begin(2 * N - 1 - k, k, sH + 18 * k, sX + 18 * (k + 1), k + 1, c, last1 ? cc : c);
      a4_backward<2>(K, o, C, S, st, [&](const A4New& n) {
        const int ob = 12 * (k + 1);
        *(lo12 && it == 1 ? sZ + ob + c : junk) = n.zn;
        *(lo12 ? sY + ob + c : junk) = n.yn;
        double* const X1 = sX + 18 * (k + 1);
        *(!last1 || lo12 ? X1 + c : junk) = n.xn;
        *(!last1 && lo2 ? X1 + 16 + c : junk) = c == 0 ? n.xn16 : n.xn17;
        if (k == 0) nz1 = n.zn;
      });
    }
    a4_block0(K, S, [&](const A4New& n) {
      *(lo12 && it == 1 ? sZ + c : junk) = n.zn;
      *(lo12 ? sY + c : junk) = n.yn;
      sX[c] = n.xn;
      *(lo2 ? sX + 16 + c : junk) = c == 0 ? n.xn16 : n.xn17;
    });
    if (a.A.check && it % a.A.check == 0) {
      flush();
      double rest = rho;
      if (a4_check(a, N, T, m, b, c_cost, rho, c, &rest)) {
        solved = true;
        done_it = it;
        break;
      }
    }
  }
  if (!solved) flush();
  int st_v = solved ? 1 : 0;
  if (!solved) st_v = a4_closing_status(a, N, T, m, b, c_cost, rho, c, false);
  if (l == 0) st.write(a.ablate, 1);
  a4_finish(a, b, l == 0, rho, solved, done_it, st_v);
  a4_solution(a, b, sX, l, 64);
}

// four problems per wave (grid = ceil(problems / 4))
template <bool ADAPT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) k_admm_iter(AdmmArgs a) {
  admm_iter4<ADAPT>(a);
}
// two problems per wave (grid = ceil(problems / 2)): a 21 KB ring, two waves per SIMD possible.  Per
// problem the same arithmetic (bit-identical); a step issues 7 DMA wave-instructions instead of 13,
// so a wave's step is shorter when the batch is small (launches of <= 512 problems use it), while
// at B = 4096 the doubled instruction count per problem costs more than the second wave hides
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) k_admm_iter2(AdmmArgs a) {
  admm_iter4<false, 2>(a);
}
// one problem per workgroup, records and vectors resident in LDS (grid = problems; N <= ARES_N)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) k_admm_iter_res(AdmmArgs a) {
  admm_iter_res<ARES_N>(a);
}
#undef A5_STAMP

}  // namespace i7m
