// i7m_plan.h — the launch plan of libindy7mpc.so as pure host code: which kernel variant a launch
// of a given size runs, whether a batch staggers, where its ranges and chunks begin, and how a
// closed loop's per-call workspace and a controller session's buffers are carved, and the argument
// check and refusal messages of the sampled-wrench entry points.  No HIP here (tests/host/ compiles
// it with a plain C++17 compiler); i7m_api.hip asks these selectors and only launches.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/indy7_mpc.h"

// functions a kernel calls too (track_index): host and device under hipcc, plain inline elsewhere
#if defined(__HIPCC__)
#define I7M_PLAN_HD __host__ __device__
#else
#define I7M_PLAN_HD
#endif

namespace i7m {

// The launch knobs of a handle: i7m_config's, overridden by the environment (tuning_from_env).
struct Tuning {
  int ls_waves = 0;  // waves per problem in k_linesearch: 0 automatic (4 for B <= 768), else I7M_LS_WAVES (1, 2 or 4)
  // I7M_LS_TAIL = r > 0: split line search — the first launch (one wave per problem) stops after r
  // rounds, a second launch with two waves per problem finishes the unresolved problems
  int ls_tail = 0;
  bool use_graph = false;  // I7M_GRAPH=1: capture the solve once per buffer set, replay it
                           // (measured 4-5 us slower per solve at B = 1 and 64, level at 4096)
  int ric_w2 = -1;               // k_riccati_mfma_w2 (two waves per problem): 1 / 0, -1 = by batch size
  int ric_bc = -1;               // k_riccati_mfma broadcast variant (BC bits), -1 = by batch size
  // host-to-host i7m_solve split into chunks on two streams, so the copies of one chunk overlap
  // the solve of another (0 = automatic, h2h_chunks_for; I7M_H2H_CHUNKS or cfg.h2h_chunks)
  int h2h_chunks = 0;
  // pipelined host-to-host chunks (h2h_pipe 1 / 2; I7M_H2H_PIPE=0: the first cut's two alternating
  // streams): per chunk, copy-in on cs[0] -> solve -> copy-out on cs[1]
  // 2 (default): the chunks' solves alternate over two streams, so one chunk's solve may overlap the
  // next one's start; 1: all solves on the handle's stream (A/B); 3: as 2, with the
  // copies out issued by a second host thread (pageable copies block the issuing thread)
  int h2h_pipe = 2;
  int h2h_taper = 1;  // I7M_H2H_TAPER=0: equal chunks (A/B)
  // ADMM mode, i7m_solve_device with B >= admm_stagger_min_b: the batch as two ranges on
  // streams of their own, the second started once the first has passed a mark (1: its first QP's
  // scaling and factor; 2: its first QP), so one range's latency-bound phases (the factor, the
  // OSQP iterations after the first termination check) overlap the other's stream-bound ones
  // (DESIGN.md §4.7).  0: one range.  I7M_ADMM_STAGGER, I7M_ADMM_STAGGER_MIN_B.
  int admm_stagger = 1;
  int admm_stagger_min_b = 3072;  // measured, two ranges: B = 8192 / 4096 / 3072 +9 / +17 / +5 %; 2048 / 1024 -8 / -11 %
  // k_admm_iter2 (two problems per wave) for launches of at most 512 problems: 3.5 % shorter at
  // B <= 256, level at 1 024, 19-32 % longer at 4 096 (profiles/r06p, r06q); I7M_ADMM_ITER2 = 0
  // never, 1 always, -1 (default) by that size
  int admm_iter2 = -1;
  // k_admm_iter_res (one problem per workgroup, its records and vectors resident in LDS) for
  // launches of at most admm_res_max problems at N <= ARES_N without rho adaptation; I7M_ADMM_RES
  // = 0 never, 1 whenever it fits, -1 (default) by that size
  int admm_res = -1;
  int admm_res_max = 256;
  // k_admm_scale / k_admm_factor as built under the max-ILP scheduler (i7m_admm_prep_tu.hip) for
  // launches of at most admm_prep_ilp_max problems, else this unit's: 6 % shorter at B <= 256, but
  // at config 3 (staggered ranges of 2048) the step 0.6 % longer beside the other range's
  // iteration (profiles/r06zn, r06zo); I7M_ADMM_PREP_ILP = 0 never, 1 always, -1 (default) by size
  int admm_prep_ilp = -1;
  int admm_prep_ilp_max = 1024;
  // box QP: 1 k_ipm_fused<false> (default), 0 I7M_IPM=delta (k_ipm_fused<true>: the corrector
  // reuses the predictor's factorisation; measured slower), 2 I7M_IPM=split
  int ipm_mode = 1;
  int pipeline = I7M_PIPE_AUTO;  // cfg.pipeline, or I7M_PIPE=split|fused|fused_iter
  bool generic = false;          // I7M_GENERIC=1: the generic kernels even for the baked-in Indy7 model
};

constexpr int RIC_W2_MAX_B = 128;     // two-wave Riccati up to this batch size (I7M_RIC_W2 forces): 43.9 -> 42.0 us at B = 1, 44.6 -> 42.7 at 64; slower from 512
// wave priority by progress once Riccati waves share SIMDs: from 768 problems (re-measured in round 3:
// 55.2 -> 52.4 us at B = 768, 42.5 -> 43.3 at 512; profiles/r03_ric_bc_retune_ab.txt)
constexpr int RIC_PRIO_MIN_B = 768;
// waves per problem of the line search (k_linesearch) and of k_sqp_fused
// (k_linesearch: 4 waves per problem up to 768 problems — re-measured in round 3: 28.2 -> 19.0 us at
// B = 384, 28.6 -> 19.8 at 512, 29.9 -> 28.8 at 768, 30.6 -> 35.2 at 1024, profiles/r03_ls_waves_ab.txt;
// k_sqp_fused keeps the 256 it was measured with)
constexpr int LS_W4_MAX_B = 768, FUSED_W4_MAX_B = 256;
constexpr int ADMM_ITER2_MAX_B = 512;  // k_admm_iter2 up to this launch size (Tuning::admm_iter2)
constexpr int ADMM_RES_MAX_N = 32;     // k_admm_iter_res is built for horizons up to this (ARES_N, i7m_admm_iter.h)
// chunks of a host-to-host solve of B problems: the handle's setting, else automatic — three
// (tapered) from 3 072 problems, two from 2 048, one piece below (config 3: 1.42 -> 1.21 ms;
// at B = 1 024 one piece is fastest; DESIGN.md §5 has the A/B)
constexpr int H2H_3_MIN_B = 3072, H2H_2_MIN_B = 2048;

// Fills *t from the config and the environment: the only getenv site of the knobs above.  False
// with *err set for a value out of range and for a retired A/B variable, so that an old A/B script
// does not silently measure the default.
inline bool tuning_from_env(const i7m_config& cfg, Tuning* t, std::string* err) {
  for (const char* name : {"I7M_ADMM_CHUNK", "I7M_DEV_RANGES", "I7M_ADMM_CHAINS", "I7M_ADMM_RANGES", "I7M_ADMM_SPLIT",
                           "I7M_STAGGER_MODES", "I7M_ADMM_ITER_DYN_LDS"})
    if (std::getenv(name)) {
      *err = std::string(name) + " is set, but this A/B knob was retired (it measured slower; DESIGN.md has the "
                                 "numbers): unset it";
      return false;
    }
  *t = Tuning{};
  if (const char* e = std::getenv("I7M_IPM"))
    t->ipm_mode = std::strcmp(e, "split") == 0 ? 2 : (std::strcmp(e, "delta") == 0 ? 0 : 1);
  if (const char* e = std::getenv("I7M_LS_TAIL")) t->ls_tail = std::min(std::max(std::atoi(e), 0), 3);
  if (const char* e = std::getenv("I7M_LS_WAVES")) t->ls_waves = std::atoi(e) == 4 ? 4 : (std::atoi(e) == 2 ? 2 : 1);
  if (const char* e = std::getenv("I7M_GRAPH")) t->use_graph = std::atoi(e) != 0;
  if (const char* e = std::getenv("I7M_RIC_W2")) t->ric_w2 = std::atoi(e) != 0;
  if (const char* e = std::getenv("I7M_RIC_BC")) {
    const int v = std::atoi(e) & 7;
    t->ric_bc = (v == 4 || v == 5) ? (v & 3) : v;  // instantiated: 0 1 2 3 6 7
  }
  t->h2h_chunks = cfg.h2h_chunks;
  if (const char* e = std::getenv("I7M_H2H_CHUNKS")) t->h2h_chunks = std::atoi(e);
  if (const char* e = std::getenv("I7M_H2H_PIPE")) t->h2h_pipe = std::min(std::max(std::atoi(e), 0), 3);
  if (const char* e = std::getenv("I7M_H2H_TAPER")) t->h2h_taper = std::atoi(e) != 0;
  if (const char* e = std::getenv("I7M_ADMM_STAGGER")) {
    t->admm_stagger = std::min(std::max(std::atoi(e), 0), 4);
    if (t->admm_stagger > 2) {
      *err = std::string("I7M_ADMM_STAGGER=") + e + ": the stagger marks 3 and 4 were retired (they measured "
                                                    "slower; DESIGN.md §4.7): use 0, 1 or 2";
      return false;
    }
  }
  if (const char* e = std::getenv("I7M_ADMM_STAGGER_MIN_B")) t->admm_stagger_min_b = std::max(std::atoi(e), 2);
  if (const char* e = std::getenv("I7M_ADMM_ITER2")) t->admm_iter2 = std::min(std::max(std::atoi(e), -1), 1);
  if (const char* e = std::getenv("I7M_ADMM_RES")) t->admm_res = std::min(std::max(std::atoi(e), -1), 1);
  if (const char* e = std::getenv("I7M_ADMM_RES_MAX")) t->admm_res_max = std::max(std::atoi(e), 0);
  if (const char* e = std::getenv("I7M_ADMM_PREP_ILP")) t->admm_prep_ilp = std::min(std::max(std::atoi(e), -1), 1);
  if (const char* e = std::getenv("I7M_ADMM_PREP_ILP_MAX")) t->admm_prep_ilp_max = std::max(std::atoi(e), 0);
  if (t->h2h_chunks < 0 || t->h2h_chunks > 64) {
    *err = "h2h_chunks must be in [0, 64]";
    return false;
  }
  t->pipeline = cfg.pipeline;
  if (const char* e = std::getenv("I7M_PIPE"))
    t->pipeline = std::strcmp(e, "fused") == 0 ? I7M_PIPE_FUSED
                  : std::strcmp(e, "fused_iter") == 0 ? I7M_PIPE_FUSED_ITER
                  : std::strcmp(e, "split") == 0 ? I7M_PIPE_SPLIT
                  : t->pipeline;
  if (const char* e = std::getenv("I7M_GENERIC")) t->generic = std::atoi(e) != 0;
  return true;
}

// An I7M_ABLATE value of the diagnostic (-DI7M_DIAG) library: one a kernel acts on, one whose
// timing variant was retired with the Riccati and line-search ablations (DESIGN.md §7 has their
// numbers; commit a2cf0e7 is the last tree that builds them), or one no kernel ever looked at.
// `msg` is null for a known value.  i7m_create refuses the other two, so that an old script does
// not silently time the default.
enum class Ablate { known, retired, unknown };
struct AblateStatus {
  Ablate kind;
  const char* msg;
};
inline AblateStatus ablate_status(int v) {
  // known: 0 none; 21 the OSQP sweep without its stream (i7m_admm_iter.h); 40..44 k_ipm_fused's
  // fixed iteration count and skipped parts (i7m_box.h); 100000 + 100 IT + S, 200000 + K,
  // 300000 + P the stamps of the OSQP iteration, the factor and the scaling (tools/step_stamps.py)
  if (v == 0 || v == 21 || (v >= 40 && v <= 44) || v >= 100000) return {Ablate::known, nullptr};
  for (int r : {1, 2, 4, 6, 8, 10, 11, 13, 18, 19})
    if (v == r)
      return {Ablate::retired, "I7M_ABLATE names a Riccati / line-search timing variant that was retired (DESIGN.md "
                               "§7 has its numbers; commit a2cf0e7 is the last tree that builds it): unset it"};
  return {Ablate::unknown, "I7M_ABLATE is set to a value that no kernel acts on: unset it"};
}

// ---- selectors: Tuning and sizes in, the decision out -------------------------------------------

// The OSQP iteration kernel of a launch of n problems at horizon N: k_admm_iter<true> (rho
// adaptation), k_admm_iter_res, k_admm_iter2, or k_admm_iter<false> (four problems per wave).
enum class AdmmIter { adapt, res, iter2, iter4 };
inline AdmmIter admm_iter_kernel(const Tuning& t, int N, bool adaptive_rho, int n) {
  if (adaptive_rho) return AdmmIter::adapt;
  if (N <= ADMM_RES_MAX_N && (t.admm_res > 0 || (t.admm_res < 0 && n <= t.admm_res_max))) return AdmmIter::res;
  if (t.admm_iter2 > 0 || (t.admm_iter2 < 0 && n <= ADMM_ITER2_MAX_B)) return AdmmIter::iter2;
  return AdmmIter::iter4;
}

// the max-ILP-scheduled scaling and factor (i7m_admm_prep_tu.hip) or i7m_api.hip's own?
inline bool admm_prep_ilp(const Tuning& t, int n) {
  return t.admm_prep_ilp > 0 || (t.admm_prep_ilp < 0 && n <= t.admm_prep_ilp_max);
}

// k_riccati_mfma's variant.
// cross-lane broadcasts (riccati_mfma_body BC): the rollout's and the pivots' by DPP at every
// batch size; I7M_RIC_BC=0..3 forces one (A/B)
// DPP pivot broadcasts at every batch size since the round-3 stage changes (re-measured: 57.9 -> 54.7 us
// at B = 1024, 44.3 -> 42.6 at 512, 41.4 -> 40.0 at 64, 40.7 -> 39.5 at B = 1; before them they
// cost ~4.5 us below 2048; profiles/r03_ric_bc_retune_ab.txt)
// wave priority by progress (BC bit 2) once SIMDs hold more than one wave: -6 % at B = 4096,
// -4 % at B = 1024 (uneven dispatch puts two waves on some SIMDs), +1 us at B = 64
// small batches: two waves per problem (k_riccati_mfma_w2), the stage's MFMA chains split; not
// with vout (i7m_qp_value: the one-wave kernel only)
struct RicVariant {
  bool w2;
  int bc;
};
inline RicVariant riccati_variant(const Tuning& t, int B, bool vout) {
  const int bc = t.ric_bc >= 0 ? t.ric_bc : 3 | (B >= RIC_PRIO_MIN_B ? 4 : 0);
  const bool w2 = !vout && (t.ric_w2 >= 0 ? t.ric_w2 != 0 : B <= RIC_W2_MAX_B);
  return {w2, bc};
}

// small batches leave most SIMDs idle: spend them on evaluating every candidate in one round
inline int ls_waves(const Tuning& t, int B) { return t.ls_waves > 0 ? t.ls_waves : (B <= LS_W4_MAX_B ? 4 : 1); }
inline int fused_waves(const Tuning& t, int B) { return t.ls_waves > 0 ? t.ls_waves : (B <= FUSED_W4_MAX_B ? 4 : 1); }

// Does this solve run as one k_sqp_fused launch?  (Direct QP only; the box mode's interior point
// has its own fused kernel between the Riccati and the line search.)  AUTO is the split pipeline
// at every batch size: the fused one measured 1.1-2.4x slower from B = 1 to 4096.
inline bool use_fused(const Tuning& t, int qp_mode) {
  return qp_mode == I7M_QP_DIRECT && (t.pipeline == I7M_PIPE_FUSED || t.pipeline == I7M_PIPE_FUSED_ITER);
}

// Does a batch of B run as two staggered ranges (Tuning::admm_stagger)?
inline bool stagger_applies(const Tuning& t, int qp_mode, int B) {
  return qp_mode == I7M_QP_ADMM && t.admm_stagger > 0 && B >= t.admm_stagger_min_b;
}
// The staggered ranges are [0, cut) and [cut, B): half the batch, rounded up to k_admm_iter's four
// problems per wave and clamped to the batch (the rounded split of a small B must not
// run past it); an empty second range is skipped.
inline long stagger_cut(int B) { return std::min<long>(((long)(B / 2) + 3) / 4 * 4, B); }
// The cut of a batch whose rows come in groups of H (a power of two; i7m_mpc_run_sampled): the
// smallest multiple of lcm(H, 4) that is >= B / 2, clamped to the batch, so that no group straddles
// it and the first range still fills k_admm_iter's waves.
inline long stagger_cut_grouped(int B, int H) {
  const long L = std::max(H, 4);
  return std::min<long>(((long)B + 2 * L - 1) / (2 * L) * L, B);
}

// How many chunks a host-to-host solve of B problems runs in.
inline int h2h_chunks_for(const Tuning& t, int qp_mode, int B) {
  int n;
  if (t.h2h_chunks > 0) n = t.h2h_chunks;
  // ADMM mode where the device solve staggers: two chunks, the second's solve behind the first's
  // mark (solve_h2h_pipelined), i.e. the staggered halves with the copies overlapped
  else if (stagger_applies(t, qp_mode, B)) n = 2;
  else n = B >= H2H_3_MIN_B ? 3 : (B >= H2H_2_MIN_B ? 2 : 1);
  return std::min(n, B);
}
// First problem of chunk i of nch (i = nch: B).
// taper (default; I7M_H2H_TAPER=0 for equal chunks): the first and the last chunk half the size
// of the others, so the copy-in before the first solve and the copy-out after the last are short
inline long chunk_lo(int B, int nch, int i, bool taper) {
  if (!taper || nch < 3) return (long)B * i / nch;
  if (i == 0) return 0;
  if (i == nch) return B;
  return (long)((double)B * (2 * i - 1) / (2.0 * (nch - 1)));
}

// ---- the per-call workspace of the closed loops ---------------------------------------------------

// n sub-buffers of bytes[i] bytes carved from one allocation: off[i] is where sub-buffer i begins,
// a multiple of WS_ALIGN; returns the size of the allocation.  A zero-sized request takes no room.
constexpr size_t WS_ALIGN = 256;
inline size_t carve(const size_t* bytes, int n, size_t* off) {
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    off[i] = total;
    total += (bytes[i] + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN;
  }
  return total;
}
// rows of a closed loop's per-step histories (one row even for a run of 0 steps)
inline size_t history_rows(int num_steps, int instances) { return (size_t)std::max(num_steps, 1) * instances; }
// i7m_mpc_run's request: the endpoints, the distance and q histories, goal index and alive flag per instance
enum { MPC_WS_EP, MPC_WS_DIST, MPC_WS_Q, MPC_WS_GI, MPC_WS_ALIVE, MPC_WS_COUNT };
inline void mpc_ws_bytes(int B, int n_endpoints, int num_steps, size_t bytes[MPC_WS_COUNT]) {
  const size_t hist = history_rows(num_steps, B);
  bytes[MPC_WS_EP] = 3 * 8 * (size_t)n_endpoints;
  bytes[MPC_WS_DIST] = 8 * hist;
  bytes[MPC_WS_Q] = 6 * 8 * hist;
  bytes[MPC_WS_GI] = bytes[MPC_WS_ALIVE] = 4 * (size_t)B;
}
// i7m_mpc_run_sampled's, G groups of H rows: the endpoints; per group the state, XU_best, the actual
// wrench schedule; the noise schedule; the distance, q and winning-wrench histories; the rows' rho;
// per group the winner, goal index and alive flag; the winners' history
enum { SWS_EP, SWS_XCUR, SWS_XUB, SWS_FACT, SWS_NOISE, SWS_DIST, SWS_Q, SWS_FB, SWS_RHO0, SWS_BEST, SWS_GI, SWS_ALIVE,
       SWS_BH, SAMPLED_WS_COUNT };
inline void sampled_ws_bytes(int G, int H, int N, int num_steps, int n_endpoints, int n_actual, bool noise,
                             size_t bytes[SAMPLED_WS_COUNT]) {
  const size_t hist = history_rows(num_steps, G), B = (size_t)G * H;
  bytes[SWS_EP] = 3 * 8 * (size_t)n_endpoints;
  bytes[SWS_XCUR] = 12 * 8 * (size_t)G;
  bytes[SWS_XUB] = 8 * (18 * (size_t)N - 6) * G;
  bytes[SWS_FACT] = 6 * 8 * (size_t)n_actual * G;
  bytes[SWS_NOISE] = noise ? 3 * 8 * (size_t)num_steps * B : 0;
  bytes[SWS_DIST] = 8 * hist;
  bytes[SWS_Q] = bytes[SWS_FB] = 6 * 8 * hist;
  bytes[SWS_RHO0] = 8 * B;
  bytes[SWS_BEST] = bytes[SWS_GI] = bytes[SWS_ALIVE] = 4 * (size_t)G;
  bytes[SWS_BH] = 4 * hist;
}

// ---- the multi-rate closed loop (i7m_mpc_run_multirate, i7m_mpc_multirate.h) ----------------------

// The plant's sub-steps of every MPC step and the knots each step completes: the reference's inner
// while-loop (src/gato_mpc_batch.py:171-199 = src/gato_mpc.py:118-140) run ahead of time.  It
// depends on dt, sim_dt and the step index alone, never on a state, so the kernel gets a bounded
// list and needs no open-ended loop.  Double arithmetic in the reference's order; the float
// residues are its behaviour and are kept: with dt = 0.01, sim_dt = 0.001 the tenth step is
// [0.001, 8.67e-19] (the accumulator reaches 0.01 - 8.67e-19 first), and that tiny sub-step is a
// real rk4 call and a real xpath entry there too.
// The reference's current_interval = int(time_accumulated / dt) (:179 / :125) is always 0: the
// accumulator is reset whenever it reaches dt, so it stays below dt.  Every sub-step is driven by
// knot 0's control and no knot index is carried (sub_knot below is I7M_CONTROL_POLICY's alone).
constexpr int MULTIRATE_MAX_SUB = 66;  // sub-steps of one MPC step: covers sim_dt <= 64 dt (64 whole knots, two partial)
struct MultirateSchedule {
  std::vector<int32_t> sub_start;  // (num_steps + 1) step i owns sub-steps [sub_start[i], sub_start[i + 1])
  std::vector<double> sub_dt;      // (S) rk4 step lengths
  std::vector<int32_t> shift;      // (num_steps) knots completed in step i: the warm-start shift
  std::vector<int32_t> sub_knot;   // (S) knots its step had completed when the sub-step began (I7M_CONTROL_POLICY)
  int total() const { return sub_start.empty() ? 0 : sub_start.back(); }
};
// False with *which = "sim_dt" (not finite or not positive), "shift" (step *at completes more than
// N - 1 knots) or "substeps" (step *at needs more than MULTIRATE_MAX_SUB sub-steps; this bound also
// ends the loop for any dt).  A refused schedule is left empty.
inline bool multirate_schedule(double dt, double sim_dt, int N, int num_steps, MultirateSchedule* out,
                               const char** which, long* at) {
  const auto no = [&](const char* w, long a) {
    *out = MultirateSchedule{};
    *which = w;
    *at = a;
    return false;
  };
  *out = MultirateSchedule{};
  if (!std::isfinite(sim_dt) || !(sim_dt > 0.0)) return no("sim_dt", 0);
  out->sub_start.push_back(0);
  double acc = 0.0;  // carried over all steps
  for (int i = 0; i < num_steps; ++i) {
    double rem = sim_dt;
    int shift = 0, n = 0;
    while (rem > 0.0) {
      if (++n > MULTIRATE_MAX_SUB) return no("substeps", i);
      const double ts = std::min(rem, dt - acc);
      acc += ts;
      rem -= ts;
      out->sub_dt.push_back(ts);
      out->sub_knot.push_back(shift);
      if (std::fabs(acc - dt) < 1e-10) {
        ++shift;
        acc = 0.0;
      }
    }
    if (shift > N - 1) return no("shift", i);
    out->shift.push_back(shift);
    out->sub_start.push_back((int32_t)out->sub_dt.size());
  }
  return true;
}
// The text of a refusal by multirate_schedule, for the entry point `who`.
inline std::string multirate_refusal(const std::string& who, const std::string& which, long at, double sim_dt, int N) {
  const std::string step = std::to_string(at), sd = std::to_string(sim_dt);
  if (which == "shift")
    return who + ": sim_dt = " + sd + " completes more than N - 1 = " + std::to_string(N - 1) + " knots in step " + step +
           " (the warm-start shift would pass the horizon)";
  if (which == "substeps")
    return who + ": sim_dt = " + sd + " needs more than MULTIRATE_MAX_SUB = " + std::to_string(MULTIRATE_MAX_SUB) +
           " plant sub-steps in step " + step;
  return who + ": sim_dt must be finite and > 0";
}
// I7M_CONTROL_POLICY drives sub-step s with knot sub_knot[s]'s control and gain, and knot N - 1 has
// neither: the first step that completes more than N - 2 knots, or -1.
inline long multirate_policy_bad_step(const MultirateSchedule& sch, int N) {
  for (size_t i = 0; i < sch.shift.size(); ++i)
    if (sch.shift[i] > N - 2) return (long)i;
  return -1;
}
inline std::string multirate_policy_refusal(const std::string& who, long at, double sim_dt, int N) {
  return who + ": sim_dt = " + std::to_string(sim_dt) + " completes more than N - 2 = " + std::to_string(N - 2) +
         " knots in step " + std::to_string(at) + " (control_from = I7M_CONTROL_POLICY: knot N - 1 has no control)";
}
// i7m_mpc_run_multirate's request: the endpoints; the distance, q and control histories (per step)
// and the path (per sub-step); the sub-step lengths; the instances' initial rho (I7M_QP_ADMM
// resets); goal index and alive flag per instance
enum { MRWS_EP, MRWS_DIST, MRWS_Q, MRWS_U, MRWS_XPATH, MRWS_SUBDT, MRWS_RHO0, MRWS_GI, MRWS_ALIVE, MULTIRATE_WS_COUNT };
inline void multirate_ws_bytes(int B, int n_endpoints, int num_steps, int n_sub, size_t bytes[MULTIRATE_WS_COUNT]) {
  const size_t hist = history_rows(num_steps, B);
  bytes[MRWS_EP] = 3 * 8 * (size_t)n_endpoints;
  bytes[MRWS_DIST] = 8 * hist;
  bytes[MRWS_Q] = bytes[MRWS_U] = 6 * 8 * hist;
  bytes[MRWS_XPATH] = 6 * 8 * history_rows(n_sub, B);
  bytes[MRWS_SUBDT] = 8 * (size_t)std::max(n_sub, 1);
  bytes[MRWS_RHO0] = 8 * (size_t)B;
  bytes[MRWS_GI] = bytes[MRWS_ALIVE] = 4 * (size_t)B;
}

// ---- the reference-tracking goal source of the sampled loop (i7m_mpc_run_tracking) ---------------

// Row of the reference (L points) that knot k of the window at phase ph and offset off reads: the
// window holds the last point once it runs past the end.  The kernel's goal phase
// (i7m_mpc_sampled.h) and the host's initial window use this one function.
I7M_PLAN_HD inline long track_index(long ph, long off, long k, long L) {
  const long i = ph + off + k;
  return i < L - 1 ? i : L - 1;
}
// The sampled loop's request with either goal source: sampled_ws_bytes' 13 sub-buffers, then the
// reference (L, ref_stride), the groups' phases and the EE history.  Endpoint mode (L = 0): those
// three are empty and take no room, so its allocation is what it was.
enum { TWS_REF = SAMPLED_WS_COUNT, TWS_PHASE, TWS_EE, TRACKING_WS_COUNT };
inline void tracking_ws_bytes(int G, int H, int N, int num_steps, int n_endpoints, int n_actual, bool noise, long L,
                              int ref_stride, bool phase, size_t bytes[TRACKING_WS_COUNT]) {
  sampled_ws_bytes(G, H, N, num_steps, n_endpoints, n_actual, noise, bytes);
  bytes[TWS_REF] = 8 * (size_t)L * ref_stride;
  bytes[TWS_PHASE] = L > 0 && phase ? 4 * (size_t)G : 0;
  bytes[TWS_EE] = L > 0 ? 3 * 8 * history_rows(num_steps, G) : 0;
}

// ---- the controller session (i7m_ctrl_begin / i7m_ctrl_step / i7m_ctrl_end, i7m_ctrl.h) ----------

// One group's record of a step, what a step's single device-to-host copy carries: the control, the
// winning wrench, the tracking error, the EE position and the winner's index (as a double: < 256).
enum { CREC_U = 0, CREC_FBEST = 6, CREC_ERR = 12, CREC_EE = 13, CREC_BEST = 16, CTRL_REC = 17 };
// The session's device buffers, all allocated by i7m_ctrl_begin: the reference and the groups'
// phases; per group XU_best, x_last, u_last and the scored hypothesis; the step's inputs (the
// measurement, the noise) and its output records; the rows' initial rho (I7M_QP_ADMM resets).
enum { CWS_REF, CWS_PHASE, CWS_XUB, CWS_XLAST, CWS_ULAST, CWS_BEST, CWS_XMEAS, CWS_NOISE, CWS_REC, CWS_RHO0,
       CTRL_WS_COUNT };
inline void ctrl_ws_bytes(int G, int H, int N, long L, int ref_stride, bool phase, size_t bytes[CTRL_WS_COUNT]) {
  const size_t B = (size_t)G * H;
  bytes[CWS_REF] = 8 * (size_t)L * ref_stride;
  bytes[CWS_PHASE] = phase ? 4 * (size_t)G : 0;
  bytes[CWS_XUB] = 8 * (18 * (size_t)N - 6) * G;
  bytes[CWS_XLAST] = bytes[CWS_XMEAS] = 12 * 8 * (size_t)G;
  bytes[CWS_ULAST] = 6 * 8 * (size_t)G;
  bytes[CWS_BEST] = 4 * (size_t)G;
  bytes[CWS_NOISE] = 3 * 8 * B;
  bytes[CWS_REC] = CTRL_REC * 8 * (size_t)G;
  bytes[CWS_RHO0] = 8 * B;
}
// The session's pinned host staging: the measurement and the noise on their way in, the records on
// their way out.
enum { CHS_XMEAS, CHS_NOISE, CHS_REC, CTRL_HS_COUNT };
inline void ctrl_host_bytes(int G, int H, size_t bytes[CTRL_HS_COUNT]) {
  bytes[CHS_XMEAS] = 12 * 8 * (size_t)G;
  bytes[CHS_NOISE] = 3 * 8 * (size_t)G * H;
  bytes[CHS_REC] = CTRL_REC * 8 * (size_t)G;
}

// ---- a call of the sampled-wrench family: its description, its one check, its refusal texts -------

// The goal source: the endpoints (i7m_mpc_run_sampled) or a reference trajectory and the caller's
// window schedule (i7m_mpc_run_tracking; i7m_ctrl_begin, whose offsets come with the steps).
struct GoalSource {
  const double* endpoints = nullptr;  // (n_endpoints, 3)
  int n_endpoints = 0;
  const double* ref = nullptr;  // (L, ref_stride)
  long L = 0;
  int ref_stride = 0;
  const int32_t* ref_phase = nullptr;   // (G) or null
  const int32_t* ref_offset = nullptr;  // (num_steps)
  static GoalSource of_endpoints(const double* endpoints, int n_endpoints) {
    GoalSource g;
    g.endpoints = endpoints;
    g.n_endpoints = n_endpoints;
    return g;
  }
  static GoalSource of_reference(const double* ref, long L, int ref_stride, const int32_t* ref_phase,
                                 const int32_t* ref_offset) {
    GoalSource g;
    g.ref = ref;
    g.L = L;
    g.ref_stride = ref_stride;
    g.ref_phase = ref_phase;
    g.ref_offset = ref_offset;
    return g;
  }
};
// A call of i7m_mpc_run_sampled (endpoints), i7m_mpc_run_tracking (tracking) or i7m_ctrl_begin
// (session): the handle's part, the sizes, the options, the goal source and the caller's required
// pointers (hist_out: dist_out / err_out).  The session has no steps and reads neither sim_dt nor
// n_actual; its start states are optional.
// The multi-rate kinds (i7m_mpc_run_sampled_multirate / i7m_mpc_run_tracking_multirate): sim_dt is
// finite and > 0 but not bounded by dt, shift_warm_start is 0 or 1, and the tracking window's
// schedule is the library's (the knots completed), so no ref_offset is asked for.
enum class SampledKind { endpoints, tracking, session, endpoints_multirate, tracking_multirate };
inline bool multirate_kind(SampledKind k) {
  return k == SampledKind::endpoints_multirate || k == SampledKind::tracking_multirate;
}
inline bool tracking_kind(SampledKind k) { return k != SampledKind::endpoints && k != SampledKind::endpoints_multirate; }
struct SampledCall {
  SampledKind kind = SampledKind::endpoints;
  int qp_mode = I7M_QP_DIRECT, max_batch = 0;
  double dt = 0.0;
  int G = 0, H = 0, num_steps = 0;
  i7m_sampled_opts o{};
  int shift_warm_start = 0;  // the multi-rate kinds only
  int control_from = I7M_CONTROL_NEW;  // or, the multi-rate kinds only, I7M_CONTROL_POLICY
  GoalSource goal;
  const double *xstart = nullptr, *fhyp = nullptr, *f_actual = nullptr;
  const double* hist_out = nullptr;
};
// The one argument check of the family, host reads only.  On a refusal *which names the argument
// and *at is the offending value; the entry for ref_phase and ref_offset; 0 for a null pointer (-1
// for a null ref_offset, whose entry 0 can be negative too).  The scans read G phases and num_steps
// offsets, no more: no groups reads no phases.
inline bool sampled_call_ok(const SampledCall& c, const char** which, long* at) {
  const auto no = [&](const char* w, long a) {
    *which = w;
    *at = a;
    return false;
  };
  const bool multi = multirate_kind(c.kind), loop = c.kind != SampledKind::session, track = tracking_kind(c.kind);
  const GoalSource& g = c.goal;
  if (c.qp_mode != I7M_QP_DIRECT && c.qp_mode != I7M_QP_ADMM) return no("qp_mode", c.qp_mode);
  if (c.H < 1 || c.H > 256 || (c.H & (c.H - 1))) return no("H", c.H);
  if (c.G < 0 || (long)c.G * c.H > c.max_batch) return no("G", (long)c.G * c.H);
  if (loop && !multi && (!(c.o.sim_dt > 0.0) || !(c.o.sim_dt <= c.dt))) return no("sim_dt", 0);
  if (multi && (!std::isfinite(c.o.sim_dt) || !(c.o.sim_dt > 0.0))) return no("sim_dt", 0);
  if (multi && c.shift_warm_start != 0 && c.shift_warm_start != 1) return no("shift_warm_start", c.shift_warm_start);
  // the policy-driven plant is the multi-rate kinds' alone; I7M_CONTROL_PREV (1) has no variant here
  if (c.control_from != I7M_CONTROL_NEW && !(multi && c.control_from == I7M_CONTROL_POLICY)) return no("control_from", c.control_from);
  if (c.o.frame != I7M_WRENCH_LOCAL && c.o.frame != I7M_WRENCH_WORLD) return no("frame", c.o.frame);
  if (c.o.reset_what & ~I7M_ADMM_RESET_ALL) return no("reset_what", c.o.reset_what);
  if (!track && g.n_endpoints < 1) return no("n_endpoints", g.n_endpoints);
  if (c.num_steps < 0) return no("num_steps", c.num_steps);
  if (track && g.L < 1) return no("L", g.L);
  if (track && g.ref_stride != 3 && g.ref_stride != 6) return no("ref_stride", g.ref_stride);
  if (loop && c.o.n_actual != 1 && c.o.n_actual != c.num_steps) return no("n_actual", c.o.n_actual);
  if (loop && !c.xstart) return no("xstart", 0);
  if (!track && !g.endpoints) return no("endpoints", 0);
  if (track && !g.ref) return no("ref", 0);
  if (!c.fhyp) return no("fhyp", 0);
  if (loop && !c.f_actual) return no("f_actual", 0);
  if (loop && !c.hist_out) return no(track ? "err_out" : "dist_out", 0);
  if (loop && track && !multi && c.num_steps > 0 && !g.ref_offset) return no("ref_offset", -1);
  for (int i = 0; track && g.ref_phase && i < c.G; ++i)
    if (g.ref_phase[i] < 0) return no("ref_phase", i);
  for (int i = 0; loop && track && !multi && i < c.num_steps; ++i)
    if (g.ref_offset[i] < 0) return no("ref_offset", i);
  return true;
}
// The text of a refusal by sampled_call_ok, for the entry point `who`.
inline std::string sampled_refusal(const std::string& who, const std::string& which, long at, int max_batch) {
  const std::string v = std::to_string(at);
  if (which == "qp_mode") return who + ": I7M_QP_BOX is not supported (I7M_QP_DIRECT or I7M_QP_ADMM)";
  if (which == "H") return who + ": H = " + v + " is not one of 1, 2, 4, ..., 256";
  if (which == "G") return who + ": G x H = " + v + " rows outside [0, max_batch=" + std::to_string(max_batch) + "]";
  if (which == "sim_dt") return who + ": sim_dt must be in (0, dt]";
  if (which == "frame") return who + ": frame must be I7M_WRENCH_LOCAL or I7M_WRENCH_WORLD";
  if (which == "reset_what") return who + ": reset_what has unknown I7M_ADMM_RESET_* bits";
  if (which == "n_endpoints") return who + ": n_endpoints = " + v + ", need >= 1 endpoint";
  if (which == "num_steps") return who + ": num_steps = " + v + ", need num_steps >= 0";
  if (which == "L") return who + ": L = " + v + ", the reference needs >= 1 point";
  if (which == "ref_stride") return who + ": ref_stride = " + v + " is not 3 or 6";
  if (which == "n_actual") return who + ": n_actual must be 1 or num_steps";
  if (which == "control_from")
    return who + ": control_from = " + v + " is not I7M_CONTROL_NEW (0) or, for a multi-rate loop, I7M_CONTROL_POLICY (2)";
  if (which == "ref_offset" && at < 0) return who + ": null ref_offset with num_steps > 0";
  if (which == "ref_phase" || which == "ref_offset") return who + ": " + which + "[" + v + "] is negative";
  return who + ": null " + which;
}

// The multi-rate kinds' check: the family's (sampled_call_ok with a multi-rate kind: everything it
// refuses for the single-rate loops but sim_dt > dt, and shift_warm_start), then the plant's
// schedule for the handle's horizon N (multirate_schedule: *which = "shift" or "substeps", *at the
// step), then under control_from = I7M_CONTROL_POLICY the N - 2 bound of i7m_mpc_run_multirate
// (multirate_policy_bad_step: *which = "policy_shift", *at the step).  On success *sch is the schedule
// the loop runs.
inline bool sampled_multirate_call_ok(const SampledCall& c, int N, MultirateSchedule* sch, const char** which, long* at) {
  *sch = MultirateSchedule{};
  if (!multirate_kind(c.kind)) {
    *which = "kind";
    *at = (long)c.kind;
    return false;
  }
  if (!sampled_call_ok(c, which, at)) return false;
  if (!multirate_schedule(c.dt, c.o.sim_dt, N, c.num_steps, sch, which, at)) return false;
  if (c.control_from == I7M_CONTROL_POLICY && (*at = multirate_policy_bad_step(*sch, N)) >= 0) {
    *sch = MultirateSchedule{};
    *which = "policy_shift";
    return false;
  }
  return true;
}
// The text of a refusal by sampled_multirate_call_ok, for the entry point `who`.
inline std::string sampled_multirate_refusal(const std::string& who, const std::string& which, long at,
                                             const SampledCall& c, int N) {
  if (which == "sim_dt" || which == "shift" || which == "substeps") return multirate_refusal(who, which, at, c.o.sim_dt, N);
  if (which == "policy_shift") return multirate_policy_refusal(who, at, c.o.sim_dt, N);
  if (which == "shift_warm_start") return who + ": shift_warm_start = " + std::to_string(at) + " is not 0 or 1";
  if (which == "kind") return who + ": not a multi-rate call";
  return sampled_refusal(who, which, at, c.max_batch);
}
// The window offsets of a multi-rate tracking run: off[i] = the knots completed by steps 0 .. i, the
// notebook's eepos_offset after step i's plant.
inline std::vector<int32_t> multirate_offsets(const MultirateSchedule& sch) {
  std::vector<int32_t> off(sch.shift.size());
  int32_t acc = 0;
  for (size_t i = 0; i < off.size(); ++i) off[i] = (acc += sch.shift[i]);
  return off;
}
// The multi-rate sampled loops' request: tracking_ws_bytes' sub-buffers, then the control history
// (per step), the path (per sub-step) and the sub-step lengths.
enum { SMWS_U = TRACKING_WS_COUNT, SMWS_XPATH, SMWS_SUBDT, SAMPLED_MULTIRATE_WS_COUNT };
inline void sampled_multirate_ws_bytes(int G, int H, int N, int num_steps, int n_sub, int n_endpoints, int n_actual,
                                       bool noise, long L, int ref_stride, bool phase,
                                       size_t bytes[SAMPLED_MULTIRATE_WS_COUNT]) {
  tracking_ws_bytes(G, H, N, num_steps, n_endpoints, n_actual, noise, L, ref_stride, phase, bytes);
  bytes[SMWS_U] = 6 * 8 * history_rows(num_steps, G);
  bytes[SMWS_XPATH] = 6 * 8 * history_rows(n_sub, G);
  bytes[SMWS_SUBDT] = 8 * (size_t)std::max(n_sub, 1);
}
// The one request of a loop of the family, whichever its kind: a multi-rate call's is
// sampled_multirate_ws_bytes with its schedule's n_sub sub-steps; a single-rate call's is
// tracking_ws_bytes, the three multi-rate sub-buffers empty, so they take no room and its allocation
// is what it was.
inline void sampled_call_ws_bytes(const SampledCall& c, int N, int n_sub, bool noise,
                                  size_t bytes[SAMPLED_MULTIRATE_WS_COUNT]) {
  const GoalSource& g = c.goal;
  if (multirate_kind(c.kind)) {
    sampled_multirate_ws_bytes(c.G, c.H, N, c.num_steps, n_sub, g.n_endpoints, c.o.n_actual, noise, g.L, g.ref_stride,
                               g.ref_phase != nullptr, bytes);
    return;
  }
  tracking_ws_bytes(c.G, c.H, N, c.num_steps, g.n_endpoints, c.o.n_actual, noise, g.L, g.ref_stride,
                    g.ref_phase != nullptr, bytes);
  bytes[SMWS_U] = bytes[SMWS_XPATH] = bytes[SMWS_SUBDT] = 0;
}

// i7m_ctrl_step's: the pointers, the clock, the offset, and a host scan of the measurement (a real
// sensor path must not poison the carried warm start).  *at: the non-finite entry of x_meas, the
// negative offset, -1 for a null pointer, else 0.
inline bool ctrl_step_args_ok(const double* x_meas, int G, double elapsed, int32_t ref_offset, const void* u_out,
                              const char** which, long* at) {
  const auto no = [&](const char* w, long a) {
    *which = w;
    *at = a;
    return false;
  };
  if (!x_meas) return no("x_meas", -1);
  if (!u_out) return no("u_out", -1);
  if (!std::isfinite(elapsed) || !(elapsed > 0.0)) return no("elapsed", 0);
  if (ref_offset < 0) return no("ref_offset", ref_offset);
  for (long e = 0; e < 12L * G; ++e)
    if (!std::isfinite(x_meas[e])) return no("x_meas", e);
  return true;
}
// The text of a refusal by ctrl_step_args_ok.
inline std::string ctrl_step_refusal(const std::string& who, const std::string& which, long at) {
  const std::string v = std::to_string(at);
  if (which == "elapsed") return who + ": elapsed must be finite and > 0";
  if (which == "ref_offset") return who + ": ref_offset = " + v + " is negative";
  if (which == "x_meas" && at >= 0) return who + ": x_meas[" + v + "] is not finite";
  return who + ": null " + which;
}


// ---- the controller session's policy (i7m_ctrl_set_policy / _get_policy / _set_applied) ----------

// One group's stage of the session's policy buffer: K~_k (6 x 13), then [x_k, u_k] of XU_best.
constexpr int CTRL_POLICY_K = 78, CTRL_POLICY_XU = 18, CTRL_POLICY_STAGE = CTRL_POLICY_K + CTRL_POLICY_XU;
// The three calls' argument checks, host reads only; `open`: a session is open.  *which names the
// argument ("session": none is open), *at the offending value or entry (-1: a null pointer).
inline bool ctrl_set_policy_ok(bool open, int n_k, int N, const char** which, long* at) {
  *which = !open ? "session" : "n_k";
  *at = n_k;
  return open && n_k >= 0 && n_k <= N - 1;
}
// on: n_k > 0; stepped: a step has run since the policy was turned on
inline bool ctrl_get_policy_ok(bool open, bool on, bool stepped, const char** which, long* at) {
  *which = !open ? "session" : !on ? "off" : "step";
  *at = 0;
  return open && on && stepped;
}
// have_last: a step or an x0 has set x_last
inline bool ctrl_set_applied_ok(bool open, bool have_last, const double* u_applied, int G, const char** which, long* at) {
  const auto no = [&](const char* w, long a) {
    *which = w;
    *at = a;
    return false;
  };
  if (!open) return no("session", 0);
  if (!u_applied) return no("u_applied", -1);
  if (!have_last) return no("x_last", 0);
  for (long e = 0; e < 6L * G; ++e)
    if (!std::isfinite(u_applied[e])) return no("u_applied", e);
  return true;
}
// The text of a refusal by one of the three.
inline std::string ctrl_policy_refusal(const std::string& who, const std::string& which, long at, int N) {
  const std::string v = std::to_string(at);
  if (which == "session") return who + ": no controller session is open on this handle (i7m_ctrl_begin)";
  if (which == "n_k") return who + ": n_k = " + v + " outside [0, N - 1 = " + std::to_string(N - 1) + "]";
  if (which == "off") return who + ": the session's policy is off (i7m_ctrl_set_policy with n_k > 0)";
  if (which == "step") return who + ": no i7m_ctrl_step has run since the policy was turned on";
  if (which == "x_last") return who + ": no x_last yet (a step, or i7m_ctrl_begin with x0, sets it): nothing to score u_applied against";
  if (which == "u_applied" && at >= 0) return who + ": u_applied[" + v + "] is not finite";
  return who + ": null " + which;
}

}  // namespace i7m
