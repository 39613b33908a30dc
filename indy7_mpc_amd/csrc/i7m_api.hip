// i7m_api.hip — C-ABI of libindy7mpc.so (declared in include/indy7_mpc.h).
//
// Host orchestration of the SQP of src/osqp_sqp.py:76-93 on MI355X: per SQP iteration
// k_linearize -> k_riccati -> k_linesearch on one HIP stream, all buffers device-resident,
// sized once at i7m_create for max_batch problems (the reference's OSQP setup-once analogue,
// src/osqp_solver.py:39-41).  No allocation or host sync inside i7m_solve_device.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/indy7_mpc.h"
#include "i7m_kernels.h"
#include "i7m_linearize.h"
#include "i7m_riccati_mfma.h"
#include "i7m_box.h"
#include "i7m_admm_iter.h"
#include "i7m_mpc.h"
#include "i7m_mpc_sampled.h"
#include "i7m_ctrl.h"
#include "i7m_mpc_multirate.h"
#include "i7m_mpc_sampled_multirate.h"
#include "i7m_mpc_policy.h"
#include "i7m_mpc_sampled_policy.h"
#include "i7m_plan.h"

// Source hash of the tree this library was built from (__graft_entry__.build passes it), so
// tests and smoke() can check that the loaded binary matches the sources they run against.
#ifndef I7M_SRC_HASH
#define I7M_SRC_HASH "unknown"
#endif
#ifdef I7M_DIAG
#define I7M_BUILD_KIND "diag"
#else
#define I7M_BUILD_KIND "release"
#endif

using namespace i7m;

// i7m_lin_tu.hip (its own translation unit: a different machine-scheduler setting)
void i7m_launch_linearize_kernel(bool spec, int grid, hipStream_t s, hipEvent_t ea, hipEvent_t eb, const void* model,
                                 const void* params, const double* xu, const double* goals, const double* fext,
                                 bool fext_world, const int* active, double* lin, double* cost, double* qpd,
                                 int* init_active, void* init_stats);

// i7m_admm_prep_tu.hip (the ADMM scaling and factor kernels under the max-ILP scheduler): kernel 0
// k_admm_scale<9>, 1 k_admm_scale<18>, 2 k_admm_factor; args: const AdmmArgs*
hipError_t i7m_launch_admm_prep(int kernel, int grid, hipStream_t s, hipEvent_t ea, hipEvent_t eb, const void* args);

// i7m_fused_tu.hip (k_sqp_fused in a unit of its own)
hipError_t i7m_launch_sqp_fused(bool spec, int W, bool fext_world, int it, hipStream_t s, hipEvent_t ea, hipEvent_t eb,
                                const void* model, const void* params, const double* xu_in, double* xu_out,
                                const double* xs, const double* goals, const double* fext, double* lin, double* cost,
                                double* qpd, double* kbuf, double* sol, int* active, void* stats);
hipError_t i7m_prepare_sqp_fused(int dev, int N);

// i7m_mpc_multirate_tu.hip (k_mpc_multirate_step in a unit of its own); args: const MultirateArgs*
hipError_t i7m_launch_multirate_step(int n, hipStream_t s, const void* model, const void* args);
// i7m_mpc_sampled_multirate_tu.hip (k_sampled_multirate_step); args: const SampledMultirateArgs*
hipError_t i7m_launch_sampled_multirate_step(int ng, int H, hipStream_t s, const void* model, const void* args);
// i7m_mpc_policy_tu.hip (k_policy_gather, k_mpc_multirate_policy_step); args: const MultirateArgs*,
// knots: const PolicyKnots*
hipError_t i7m_launch_policy_gather(int B, int N, int n_k, hipStream_t s, const double* kbuf, double* K_out);
hipError_t i7m_launch_multirate_policy_step(int n, hipStream_t s, const void* model, const void* args, const void* knots,
                                            const double* kbuf);

// i7m_mpc_sampled_policy_tu.hip (k_sampled_multirate_policy_step, k_ctrl_policy_copy); args: const
// SampledMultirateArgs*, knots: const PolicyKnots*
hipError_t i7m_launch_sampled_multirate_policy_step(int ng, int H, hipStream_t s, const void* model, const void* args,
                                                    const void* knots, const double* kbuf);
hipError_t i7m_launch_ctrl_policy_copy(int G, int H, int N, int n_k, hipStream_t s, const int* best, const double* kbuf,
                                       const double* xub, double* out);

static_assert(sizeof(i7m_problem_stats) == sizeof(ProblemStats), "stats layout");
static_assert(ADMM_RES_MAX_N == ARES_N, "i7m_plan.h: k_admm_iter_res's horizon");
static_assert(POLICY_MAX_SUB == MULTIRATE_MAX_SUB, "i7m_mpc_policy.h: PolicyKnots holds one step's sub-steps");
static_assert(CTRL_POLICY_REC == CTRL_POLICY_STAGE && POLICY_K == CTRL_POLICY_K, "i7m_plan.h: the session's policy record");

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPCHK(expr)                                                                             \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      return fail(I7M_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
  } while (0)

struct Timing {
  int kid;
  hipEvent_t a, b;
};

}  // namespace

// One allocation carved into 256-byte aligned sub-buffers (carve, i7m_plan.h): device memory, or
// pinned host memory.  Its owner releases it once nothing queued still uses it.
struct Carved {
  char* base = nullptr;
  bool pinned = false;
  std::vector<size_t> off;
  bool alloc(const size_t* bytes, int n, bool pinned_host) {
    off.resize(n);
    const size_t total = std::max(carve(bytes, n, off.data()), WS_ALIGN);
    pinned = pinned_host;
    const hipError_t e = pinned ? hipHostMalloc((void**)&base, total, hipHostMallocDefault) : hipMalloc((void**)&base, total);
    if (e != hipSuccess) base = nullptr;
    return base != nullptr;
  }
  void release() {
    if (base) (void)(pinned ? hipHostFree(base) : hipFree(base));
    base = nullptr;
  }
  template <class P> P* at(int i) const { return reinterpret_cast<P*>(base + off[i]); }
};

// A controller session (i7m_ctrl_begin .. i7m_ctrl_end): one device allocation and one pinned host
// allocation, carved by i7m_plan.h's ctrl_ws_bytes / ctrl_host_bytes, and what the steps carry.
struct CtrlSession {
  bool open = false;
  int G = 0, H = 0;
  bool have_last = false;  // x_last / u_last are set (i7m_ctrl_begin with x0, or a step has run)
  i7m_sampled_opts o{};
  Carved dev, host;
  CtrlArgs a{};  // the launches' arguments, all but the step's own (elapsed, off, noise, have_last, initial)
  // the winner's policy (i7m_ctrl_set_policy): n_k stages (0: off) of CTRL_POLICY_REC doubles per
  // group, on the device and in pinned staging; pol_stepped: a step has filled the staging
  int n_k = 0;
  bool pol_stepped = false;
  double *d_pol = nullptr, *h_pol = nullptr;
  std::vector<double> u_applied;  // i7m_ctrl_set_applied's staging: alive until the session ends
};

struct i7m_handle {
  i7m_config cfg;
  long N = 0, T = 0;  // the horizon and the length of an XU row, 18 N - 6
  int dev = 0;
  std::vector<void*> owned;  // every device allocation of the handle (dev_alloc); i7m_destroy frees them
  size_t scratch = 0;        // doubles in each of d_sol / d_aux / d_out (the query hooks chunk through them)
  hipStream_t own = nullptr, stream = nullptr;
  DevModel* d_model = nullptr;
  // batch buffers (max_batch problems)
  double *d_xu = nullptr, *d_xs = nullptr, *d_goal = nullptr, *d_sol = nullptr, *d_lin = nullptr,
         *d_cost = nullptr, *d_kbuf = nullptr, *d_aux = nullptr, *d_out = nullptr;
  double* d_qpd = nullptr;  // (max_batch, N-1, QPD_STRIDE) per-knot QP records (k_linearize -> k_riccati_mfma)
  int* d_active = nullptr;
  ProblemStats* d_stats = nullptr;
  double* d_fext = nullptr;   // (max_batch, 6) joint-6 wrench per problem, frame fext_frame
  int fext_frame = I7M_WRENCH_LOCAL;
  // I7M_QP_BOX (i7m_box.h): iterate, bound duals, Riccati inputs, predictor step; (max_batch, T)
  double *d_bx = nullptr, *d_bzl = nullptr, *d_bzu = nullptr, *d_bsig = nullptr, *d_bh = nullptr, *d_bdxa = nullptr;
  double *d_bhinv = nullptr, *d_bdh = nullptr;  // per-stage H^-1 (max_batch, N-1, 36); corrector dh (max_batch, T)
  IpmState* d_bst = nullptr;
  int* d_bact = nullptr;
  // I7M_QP_ADMM (i7m_admm.h): one allocation, per-problem OSQP state and k_admm scratch
  double* d_admm = nullptr;
  int* d_admm_it = nullptr;  // 2 x (max_batch, I7M_MAX_SQP): OSQP iterations, then OSQP status, per SQP iteration
  int ablate = 0;                  // I7M_DIAG builds only (I7M_ABLATE): timing variants, results invalid
  bool spec = false;               // model == kIndy7Model: use the kernels with the constants baked in
  bool has_fext = false;
  // I7M_POLICY_ZERO_K=1 at i7m_create (a test switch): I7M_CONTROL_POLICY steps with the policy
  // pass's gains zeroed, so the run must equal I7M_CONTROL_NEW's bit for bit
  bool policy_zero_k = false;
  size_t goal_cap = 0;
  // hipGraph replay of run_sqp (run_sqp_graphed): a few instantiated graphs keyed by the call
  struct GraphEntry {
    int B, goal_stride, has_fext;
    const void *xu_in, *xu, *xs, *goals, *st, *stream;
    hipGraphExec_t exec;
    unsigned long long last_use;
  };
  std::vector<GraphEntry> graphs;
  unsigned long long graph_clock = 0;
  CtrlSession ctrl;  // the controller session, if one is open
  Tuning tune;  // the launch knobs (i7m_plan.h: tuning_from_env at i7m_create)
  double* d_lsbase = nullptr;  // (max_batch) base merits handed to the second launch
  int* d_lspend = nullptr;     // (max_batch) pending flags
  hipEvent_t ev_rmark = nullptr;  // the staggered ranges' / chunks' mark (StaggerMark)
  hipStream_t cs[2] = {nullptr, nullptr};
  hipStream_t cs2 = nullptr;  // h2h_pipe >= 2: the second solve stream (created on first use)
  hipEvent_t ev_order = nullptr, ev_done[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> ev_in, ev_cmp;
  // timing
  bool timing = false;
  std::vector<Timing> ev;
  std::vector<hipEvent_t> pool;
  double ms_sum[I7M_K_COUNT] = {};
  int counts[I7M_K_COUNT] = {};
};

namespace {

DevModel make_dev_model(const i7m_model& m) {
  DevModel d;
  std::memset(&d, 0, sizeof(d));
  for (int i = 0; i < 6; ++i) {
    for (int k = 0; k < 9; ++k) d.Rp[i][k] = m.placement_R[i][k];
    for (int k = 0; k < 3; ++k) d.tp[i][k] = m.placement_t[i][k];
    const double mass = m.mass[i];
    const double* c = m.com[i];
    d.m[i] = mass;
    for (int k = 0; k < 3; ++k) d.h[i][k] = mass * c[k];
    // inertia about the joint origin: Ic + m (|c|^2 I - c c^T)
    const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    const double* I = m.inertia[i];
    d.Io[i][0] = I[0] + mass * (cc - c[0] * c[0]);
    d.Io[i][1] = I[1] - mass * c[0] * c[1];
    d.Io[i][2] = I[2] - mass * c[0] * c[2];
    d.Io[i][3] = I[3] + mass * (cc - c[1] * c[1]);
    d.Io[i][4] = I[4] - mass * c[1] * c[2];
    d.Io[i][5] = I[5] + mass * (cc - c[2] * c[2]);
    d.qlo[i] = m.q_lower[i];
    d.qhi[i] = m.q_upper[i];
    d.vlim[i] = m.v_limit[i];
    d.ulim[i] = m.effort_limit[i];
  }
  for (int k = 0; k < 3; ++k) d.g[k] = m.gravity[k];
  return d;
}

SolveParams params_of(const i7m_handle* h, int B, int goal_stride) {
  SolveParams P;
  P.N = (int)h->N;
  P.T = (int)h->T;
  P.B = B;
  P.goal_stride = goal_stride;
  P.regularize = h->cfg.regularize;
  P.max_iters = h->cfg.max_sqp_iters;
  P.dt = h->cfg.dt;
  P.dQ = h->cfg.dQ_cost;
  P.R = h->cfg.R_cost;
  P.QN = h->cfg.QN_cost;
  P.eps = h->cfg.eps;
  P.mu = h->cfg.mu;
  P.step_tol = h->cfg.step_tol;
  return P;
}

// What every entry point that would overwrite the rows, goals, wrenches or solver state a
// controller session carries answers while one is open.
int session_open() {
  return fail(I7M_EINVAL, "controller session open: this entry point would overwrite what the session carries "
                          "(i7m_ctrl_end first)");
}

int check_batch(const i7m_handle* h, int B, int goal_stride) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (h->ctrl.open) return session_open();
  if (B < 0 || B > h->cfg.max_batch)
    return fail(I7M_EINVAL, "batch " + std::to_string(B) + " outside [0, max_batch=" +
                                std::to_string(h->cfg.max_batch) + "]");
  if (goal_stride != 3 && goal_stride != 6) return fail(I7M_EINVAL, "goal_stride must be 3 or 6");
  return I7M_OK;
}

// The opening of a batch entry point: check_batch, then for B > 0 the caller's required pointers
// (`ptrs`: all non-null) and the device made current.  (B == 0 passes: the caller returns I7M_OK.)
int open_batch(i7m_handle* h, int B, int goal_stride, bool ptrs, const char* null_msg = "null pointer") {
  const int rc = check_batch(h, B, goal_stride);
  if (rc || B == 0) return rc;
  if (!ptrs) return fail(I7M_EINVAL, null_msg);
  HIPCHK(hipSetDevice(h->dev));
  return I7M_OK;
}

hipEvent_t get_event(i7m_handle* h) {
  if (!h->pool.empty()) {
    hipEvent_t e = h->pool.back();
    h->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// Per-kernel timing: the start / stop events ride on the kernel's own dispatch packet
// (hipExtLaunchKernelGGL), so timing adds no marker packets between launches; with timing off
// the events are null and the launch is a plain dispatch.  `launch(ea, eb)` does the launch.
template <class F>
int timed(i7m_handle* h, hipStream_t s, int kid, F&& launch) {
  hipEvent_t a = nullptr, b = nullptr;
  if (h->timing) {
    a = get_event(h);
    b = get_event(h);
    if (!a || !b) a = b = nullptr;
  }
  launch(a, b);
  HIPCHK(hipGetLastError());
  if (a && b) h->ev.push_back({kid, a, b});
  return I7M_OK;
}

// Every allocation of the handle: recorded on it, freed by i7m_destroy (also after a failed create).
template <class P>
bool dev_alloc(i7m_handle* h, P** p, size_t bytes) {
  void* q = nullptr;
  if (hipMalloc(&q, bytes ? bytes : 8) != hipSuccess) return false;
  h->owned.push_back(q);
  *p = static_cast<P*>(q);
  return true;
}

// The controller session's two allocations back (i7m_ctrl_end, i7m_destroy); nothing queued may
// still use them.
void ctrl_policy_release(CtrlSession& c) {
  if (c.d_pol) (void)hipFree(c.d_pol);
  if (c.h_pol) (void)hipHostFree(c.h_pol);
  c.d_pol = c.h_pol = nullptr;
  c.n_k = 0;
  c.pol_stepped = false;
}
void ctrl_release(i7m_handle* h) {
  ctrl_policy_release(h->ctrl);
  h->ctrl.dev.release();
  h->ctrl.host.release();
  h->ctrl = CtrlSession{};
}

// Per-problem work buffers of a contiguous range of problems [b0, b0 + B): every kernel indexes
// them by its local problem index, so a range is just offset base pointers (bufs_at).
struct Bufs {
  long b0;  // the range's first problem
  double* lin;
  double* cost;
  double* qpd;
  double* kbuf;
  double* sol;          // the QP's solution (T per problem)
  int* active;
  ProblemStats* stats;  // the handle's own stats rows (a caller of run_sqp may name others)
  double* lsbase;       // split line search: base merits handed to the second launch
  int* lspend;          // and the pending flags
  const double* fext;   // nullptr: no external wrench
  // box mode only (nullptr otherwise)
  double *bx, *bzl, *bzu, *bsig, *bh, *bdxa, *bhinv, *bdh;
  IpmState* bst;
  int* bact;
  // ADMM mode only: AdmmArgs' per-problem pointers for this range (P, A, sqp_iter filled at launch)
  AdmmArgs adm;
};

// The handle's ADMM allocation: an array of buffers, each (max_batch, size) row-major.  Per-problem
// sizes, each buffer's offset and the total, in doubles.
constexpr int ADM_NBUF = 15;
struct AdmmWalk {
  long sz[ADM_NBUF], off[ADM_NBUF], total;
};
AdmmWalk admm_walk(const i7m_handle* h) {
  const long Bm = h->cfg.max_batch, N = h->N, T = h->T, m = 12 * N;
  AdmmWalk w{{T, m, m, T, 1,              // x z y q rho (state)
              36 * N, T, m, T, m, T, m,   // Pq Pd I qs ls D E
              ADM_REC * N, T, 1},         // stage records, w (h), c
             {}, 0};
  for (int i = 0; i < ADM_NBUF; ++i) {
    w.off[i] = w.total;
    w.total += (Bm * w.sz[i] + 1) & ~1L;  // every buffer 16-byte aligned (k_admm_iter's 16-byte loads)
  }
  return w;
}
// AdmmArgs pointers of problems [b0, ...) in the handle's ADMM allocation
AdmmArgs admm_layout(const i7m_handle* h, long b0) {
  const long Bm = h->cfg.max_batch;
  const AdmmWalk w = admm_walk(h);
  double* p[ADM_NBUF];
  for (int i = 0; i < ADM_NBUF; ++i) p[i] = h->d_admm + w.off[i] + b0 * w.sz[i];
  AdmmArgs a{};
  a.sx = p[0]; a.sz = p[1]; a.sy = p[2]; a.sq = p[3]; a.srho = p[4];
  a.Pq = p[5]; a.Pd = p[6]; a.I = p[7]; a.qs = p[8]; a.ls = p[9]; a.D = p[10]; a.E = p[11];
  a.R = p[12]; a.w = p[13]; a.cs = p[14];
  a.iters = h->d_admm_it + b0 * I7M_MAX_SQP;
  a.status = h->d_admm_it + (Bm + b0) * I7M_MAX_SQP;
  a.abase = h->d_admm;  // k_admm_iter reaches every array through one buffer resource over the allocation
  a.abytes = w.total * 8;
  return a;
}

Bufs bufs_at(const i7m_handle* h, long b0) {
  const long N = h->N, T = h->T;
  Bufs W{};
  W.b0 = b0;
  W.lin = h->d_lin + b0 * (N - 1) * LIN_STRIDE;
  W.cost = h->d_cost + b0 * N * COST_STRIDE;
  W.qpd = h->d_qpd + b0 * (N - 1) * QPD_STRIDE;
  W.kbuf = h->d_kbuf + b0 * (N - 1) * KBUF_STRIDE;
  W.sol = h->d_sol + b0 * T;
  W.active = h->d_active + b0;
  W.stats = h->d_stats + b0;
  W.lsbase = h->d_lsbase + b0;
  W.lspend = h->d_lspend + b0;
  W.fext = h->has_fext ? h->d_fext + 6 * b0 : nullptr;
  if (h->cfg.qp_mode == I7M_QP_BOX) {
    W.bx = h->d_bx + b0 * T;
    W.bzl = h->d_bzl + b0 * T;
    W.bzu = h->d_bzu + b0 * T;
    W.bsig = h->d_bsig + b0 * T;
    W.bh = h->d_bh + b0 * T;
    W.bdxa = h->d_bdxa + b0 * T;
    W.bhinv = h->d_bhinv + b0 * (N - 1) * 36;
    W.bdh = h->d_bdh + b0 * T;
    W.bst = h->d_bst + b0;
    W.bact = h->d_bact + b0;
  }
  if (h->cfg.qp_mode == I7M_QP_ADMM) W.adm = admm_layout(h, b0);
  return W;
}

AdmmCfg admm_cfg_of(const i7m_config& c) {
  AdmmCfg A{};
  A.rho0 = c.admm_rho;
  A.sigma = c.admm_sigma;
  A.alpha = c.admm_alpha;
  A.eps_abs = c.admm_eps_abs;
  A.eps_rel = c.admm_eps_rel;
  A.adapt_tol = c.admm_adaptive_rho_tolerance;
  A.max_iter = c.admm_max_iter;
  A.check = c.admm_check_termination;
  A.scaling = c.admm_scaling;
  A.gap = c.admm_check_dualgap;
  A.adapt_interval = c.admm_adaptive_rho_interval;
  return A;
}

// init_active / init_stats (first SQP iteration only): the kernel marks every problem active
// and zeroes its stats, so a solve needs no separate memset launches.
int launch_linearize(i7m_handle* h, hipStream_t s, const Bufs& W, const SolveParams& P, const double* xu,
                     const double* goals, const int* active, int* init_active = nullptr,
                     ProblemStats* init_stats = nullptr) {
  const long knots = (long)P.B * P.N;
  if (knots == 0) return I7M_OK;
  const int grid = (int)((knots + KPW - 1) / KPW);
  return timed(h, s, I7M_K_LIN, [&](hipEvent_t ea, hipEvent_t eb) {
    i7m_launch_linearize_kernel(h->spec, grid, s, ea, eb, h->d_model, &P, xu, goals, W.fext,
                                h->fext_frame == I7M_WRENCH_WORLD, active, W.lin, W.cost, W.qpd, init_active, init_stats);
  });
}

// vout (i7m_qp_value): the first knot's cost-to-go V~_0 (B, 13, 13) instead of the rollout (one-wave
// kernel only)
int launch_riccati(i7m_handle* h, hipStream_t s, const Bufs& W, const SolveParams& P, const double* xu,
                   const double* xs, const int* active, double* sol, double* vout = nullptr) {
  if (P.B == 0) return I7M_OK;
  return timed(h, s, I7M_K_RICCATI, [&](hipEvent_t ea, hipEvent_t eb) {
    const RicVariant rv = riccati_variant(h->tune, P.B, vout != nullptr);
    if (rv.w2) {
      auto go2 = [&](auto kern) {
        hipExtLaunchKernelGGL(kern, dim3(P.B), dim3(128), 0, s, ea, eb, 0, P, xu, xs, W.lin, W.cost, W.qpd, active,
                              W.kbuf, sol);
      };
      if (rv.bc & 1) go2(k_riccati_mfma_w2<3>);
      else go2(k_riccati_mfma_w2<2>);
      return;
    }
    auto go = [&](auto kern) {
      hipExtLaunchKernelGGL(kern, dim3(P.B), dim3(64), 0, s, ea, eb, 0, P, xu, xs, W.lin, W.cost, W.qpd, active, W.kbuf,
                            sol, (const double*)nullptr, (const double*)nullptr, vout);
    };
    switch (rv.bc) {
      case 1: go(k_riccati_mfma<false, 1>); break;
      case 2: go(k_riccati_mfma<false, 2>); break;
      case 3: go(k_riccati_mfma<false, 3>); break;
      case 6: go(k_riccati_mfma<false, 6>); break;
      case 7: go(k_riccati_mfma<false, 7>); break;
      default: go(k_riccati_mfma<false, 0>);
    }
  });
}

// k_linesearch<spec, waves, world_wrench> (waves 1, 2 or 4; 64 threads per wave)
template <bool SPEC, bool FW>
auto ls_kernel_w(int waves) {
  return waves == 4 ? k_linesearch<SPEC, 4, FW> : waves == 2 ? k_linesearch<SPEC, 2, FW> : k_linesearch<SPEC, 1, FW>;
}
auto ls_kernel(bool spec, bool world_wrench, int waves) {
  if (spec) return world_wrench ? ls_kernel_w<true, true>(waves) : ls_kernel_w<true, false>(waves);
  return world_wrench ? ls_kernel_w<false, true>(waves) : ls_kernel_w<false, false>(waves);
}

// base_from_lin: lin/cost of W hold the linearisation of this xu (the SQP loop), so the base
// merit comes from them (k_linesearch); otherwise candidate 0 is evaluated.
// xu: the linearisation point; xu_out: where the updated XU goes (may be xu itself).
int launch_linesearch(i7m_handle* h, hipStream_t s, const Bufs& W, const SolveParams& P, const double* xu,
                      double* xu_out, const double* sol, const double* goals, int* active, ProblemStats* st,
                      double* alpha_out, int iter, int mode, bool base_from_lin) {
  if (P.B == 0) return I7M_OK;
  const int nw = ls_waves(h->tune, P.B);
  const size_t lds = ls_lds_bytes(P.T, nw);
  const double* ln = base_from_lin ? W.lin : nullptr;
  const double* cs = base_from_lin ? W.cost : nullptr;
  const bool fw = W.fext && h->fext_frame == I7M_WRENCH_WORLD;
  if (h->tune.ls_tail > 0 && nw == 1 && mode == 0 && base_from_lin) {
    // split search: r rounds of one wave per problem, then two waves per problem
    // for the problems that have not accepted a candidate
    const int R = P.N >= 64 ? 1 : 64 / P.N;
    const int c_split = 1 + R * h->tune.ls_tail;
    const LsSplit first{0, c_split, W.lsbase, W.lspend};
    const LsSplit second{c_split, 1 + NALPHA, W.lsbase, W.lspend};
    int rc = timed(h, s, I7M_K_LINESEARCH, [&](hipEvent_t ea, hipEvent_t eb) {
      hipExtLaunchKernelGGL(ls_kernel(h->spec, fw, 1), dim3(P.B), dim3(64), lds, s, ea, eb, 0, h->d_model, P, xu, xu_out, sol,
                            goals, W.fext, active, st, alpha_out, iter, mode, W.lin, W.cost, first);
    });
    if (rc) return rc;
    const size_t lds2 = ls_lds_bytes(P.T, 2);
    return timed(h, s, I7M_K_LINESEARCH_TAIL, [&](hipEvent_t ea, hipEvent_t eb) {
      hipExtLaunchKernelGGL(ls_kernel(h->spec, fw, 2), dim3(P.B), dim3(128), lds2, s, ea, eb, 0, h->d_model, P, xu, xu_out,
                            sol, goals, W.fext, active, st, alpha_out, iter, mode, W.lin, W.cost, second);
    });
  }
  return timed(h, s, I7M_K_LINESEARCH, [&](hipEvent_t ea, hipEvent_t eb) {
    // (two waves: A/B only, I7M_LS_WAVES=2)
    hipExtLaunchKernelGGL(ls_kernel(h->spec, fw, nw), dim3(P.B), dim3(64 * nw), lds, s, ea, eb, 0, h->d_model, P, xu, xu_out,
                          sol, goals, W.fext, active, st, alpha_out, iter, mode, ln, cs, LsSplit{});
  });
}

BoxParams box_params(const i7m_handle* h) {
  BoxParams BP;
  BP.mask = h->cfg.box_mask;
  BP.max_iters = h->cfg.box_max_iters;
  BP.tol = h->cfg.box_tol;
  BP.theta = 0.2;  // oracle/box_ipm.py::ipm_box defaults (6.9 vs 12.2 iterations
  BP.eta = 0.99;   // per config-4 QP against theta = 0.01, z = 1)
  BP.z0 = 0.1;
  return BP;
}

// The staggered ranges' mark (Tuning::admm_stagger): the first range's (or chunk's) first run_sqp
// records `ev` on its stream at point `at` — 1: after its first QP's scaling and factor, 2: after
// its first QP — and the second range waits for it iff it was recorded.
struct StaggerMark {
  hipEvent_t ev;
  int at;
  bool recorded;
};
int record_mark(StaggerMark* m, int at, hipStream_t s) {
  if (!m || m->recorded || m->at != at) return I7M_OK;
  HIPCHK(hipEventRecord(m->ev, s));
  m->recorded = true;
  return I7M_OK;
}

// The QP of one SQP iteration: the exact equality-constrained solve (k_riccati_mfma), and in
// box mode the interior-point iteration started from it (i7m_box.h; oracle/box_ipm.py).
// Returns where the minimiser is: `sol`, or W.bx in box mode.
int solve_qp(i7m_handle* h, hipStream_t s, const Bufs& W, const SolveParams& P, const double* xu, const double* xs,
             const int* active, double* sol, const double** out, int sqp_iter = 0, StaggerMark* mark = nullptr) {
  int rc;
  if (h->cfg.qp_mode == I7M_QP_ADMM) {
    // OSQP's iteration from the problems' carried state (i7m_admm_iter.h; oracle/osqp_admm.py)
    *out = sol;
    if (P.B == 0) return I7M_OK;
    AdmmArgs a = W.adm;
    a.P = P;
    a.A = admm_cfg_of(h->cfg);
    a.lin = W.lin;
    a.cost = W.cost;
    a.qpd = W.qpd;
    a.xu = xu;
    a.xs = xs;
    a.active = active;
    a.sol = sol;
    a.sqp_iter = sqp_iter;
#ifdef I7M_DIAG
    a.ablate = h->ablate;
#endif
    a.b0 = 0;
    const int n = P.B;
    hipError_t e = hipSuccess;
    rc = timed(h, s, I7M_K_ADMM_PREP, [&](hipEvent_t ea, hipEvent_t eb) {
      // scaling, then the factor (one event pair around both)
      // the max-ILP-scheduled copies (i7m_admm_prep_tu.hip) or this unit's (default scheduler)
      if (admm_prep_ilp(h->tune, n)) {
        e = i7m_launch_admm_prep(P.N <= 32 ? 0 : 1, n, s, ea, nullptr, &a);
        if (e == hipSuccess) e = i7m_launch_admm_prep(2, n, s, nullptr, eb, &a);
        return;
      }
      if (P.N <= 32)
        hipExtLaunchKernelGGL(k_admm_scale<9>, dim3(n), dim3(64), 0, s, ea, nullptr, 0, a);
      else
        hipExtLaunchKernelGGL(k_admm_scale<18>, dim3(n), dim3(64), 0, s, ea, nullptr, 0, a);
      hipExtLaunchKernelGGL(k_admm_factor, dim3(n), dim3(64), 0, s, nullptr, eb, 0, a);
    });
    if (rc) return rc;
    if (e != hipSuccess) return fail(I7M_EHIP, std::string("k_admm_scale / k_admm_factor launch: ") + hipGetErrorString(e));
    if ((rc = record_mark(mark, 1, s))) return rc;
    rc = timed(h, s, I7M_K_ADMM, [&](hipEvent_t ea, hipEvent_t eb) {
      const dim3 g((n + 3) / 4);  // four problems per wave, rows past the batch idle
      switch (admm_iter_kernel(h->tune, P.N, a.A.adapt_interval != 0, n)) {
        case AdmmIter::adapt: hipExtLaunchKernelGGL(k_admm_iter<true>, g, dim3(64), 0, s, ea, eb, 0, a); break;
        case AdmmIter::res: hipExtLaunchKernelGGL(k_admm_iter_res, dim3(n), dim3(64), 0, s, ea, eb, 0, a); break;
        case AdmmIter::iter2:  // two problems per wave
          hipExtLaunchKernelGGL(k_admm_iter2, dim3((n + 1) / 2), dim3(64), 0, s, ea, eb, 0, a);
          break;
        case AdmmIter::iter4: hipExtLaunchKernelGGL(k_admm_iter<false>, g, dim3(64), 0, s, ea, eb, 0, a); break;
      }
    });
    if (rc) return rc;
    return record_mark(mark, 2, s);
  }
  if ((rc = launch_riccati(h, s, W, P, xu, xs, active, sol))) return rc;
  *out = sol;
  if (h->cfg.qp_mode != I7M_QP_BOX || P.B == 0) return I7M_OK;
  const BoxParams BP = box_params(h);
  const dim3 g(P.B), blk(64);
  if (h->tune.ipm_mode != 2) {
    IpmFusedArgs fa{h->d_model, P, BP, xu, xs, W.lin, W.cost, W.qpd, active, W.kbuf, sol, sol,
                    W.bx, W.bzl, W.bzu, W.bsig, W.bh, W.bdxa, W.bst, W.bact, W.bhinv, W.bdh};
#ifdef I7M_DIAG
    fa.ablate = h->ablate;
#endif
    rc = timed(h, s, I7M_K_IPM_FUSED, [&](hipEvent_t ea, hipEvent_t eb) {
      if (h->tune.ipm_mode == 0)
        hipExtLaunchKernelGGL(k_ipm_fused<true>, g, blk, 0, s, ea, eb, 0, fa);
      else
        hipExtLaunchKernelGGL(k_ipm_fused<false>, g, blk, 0, s, ea, eb, 0, fa);
    });
    if (rc) return rc;
    *out = W.bx;
    return I7M_OK;
  }
  rc = timed(h, s, I7M_K_IPM, [&](hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(k_ipm_init, g, blk, 0, s, ea, eb, 0, h->d_model, P, BP, sol, active, W.bx, W.bzl, W.bzu, W.bsig, W.bh,
                       W.bst, W.bact);
  });
  if (rc) return rc;
  for (int it = 0; it < BP.max_iters; ++it) {
    for (int half = 0; half < 2; ++half) {
      rc = timed(h, s, I7M_K_RICCATI_BOX, [&](hipEvent_t ea, hipEvent_t eb) {
        hipExtLaunchKernelGGL((k_riccati_mfma<true>), g, blk, 0, s, ea, eb, 0, P, xu, xs, W.lin, W.cost, W.qpd, W.bact, W.kbuf,
                           sol, W.bsig, W.bh, (double*)nullptr);
      });
      if (rc) return rc;
      rc = timed(h, s, I7M_K_IPM, [&](hipEvent_t ea, hipEvent_t eb) {
        if (half == 0)
          hipExtLaunchKernelGGL(k_ipm_pred, g, blk, 0, s, ea, eb, 0, h->d_model, P, BP, sol, W.bx, W.bzl, W.bzu, W.bdxa, W.bh,
                             W.bst, W.bact);
        else
          hipExtLaunchKernelGGL(k_ipm_corr, g, blk, 0, s, ea, eb, 0, h->d_model, P, BP, sol, W.bx, W.bzl, W.bzu, W.bdxa, W.bsig,
                             W.bh, W.bst, W.bact);
      });
      if (rc) return rc;
    }
  }
  *out = W.bx;
  return I7M_OK;
}

// The policy pass (i7m_qp_policy, I7M_CONTROL_POLICY): linearise at xu with x_0 = xs, then the exact
// backward sweep and rollout, in every QP mode the launches of an I7M_QP_DIRECT QP.  Leaves the gains
// K~_k of the range's problems in W.kbuf and the QP's minimiser in W.sol; on an I7M_QP_ADMM handle
// the carried OSQP state (h->d_admm) is neither read nor written.
int policy_pass(i7m_handle* h, hipStream_t s, const Bufs& W, const SolveParams& P, const double* xu, const double* xs,
                const double* goals) {
  const int rc = launch_linearize(h, s, W, P, xu, goals, nullptr);
  if (rc) return rc;
  return launch_riccati(h, s, W, P, xu, xs, nullptr, W.sol);
}

int launch_fused(i7m_handle* h, hipStream_t s, const Bufs& W, const SolveParams& P, const double* xu_in, double* xu_out,
                 const double* xs, const double* goals, ProblemStats* st) {
  const int nw = fused_waves(h->tune, P.B);
  // I7M_PIPE_FUSED_ITER: one launch per SQP iteration, else one per solve
  const int launches = h->tune.pipeline == I7M_PIPE_FUSED_ITER ? h->cfg.max_sqp_iters : 1;
  for (int i = 0; i < launches; ++i) {
    hipError_t e = hipSuccess;
    const int rc = timed(h, s, I7M_K_SQP_FUSED, [&](hipEvent_t ea, hipEvent_t eb) {
      e = i7m_launch_sqp_fused(h->spec, nw, h->fext_frame == I7M_WRENCH_WORLD, launches > 1 ? i : -1, s, ea, eb, h->d_model,
                               &P, i == 0 ? xu_in : xu_out, xu_out, xs, goals, W.fext, W.lin, W.cost, W.qpd, W.kbuf,
                               W.sol, W.active, st);
    });
    if (rc) return rc;
    if (e != hipSuccess) return fail(I7M_EHIP, std::string("k_sqp_fused launch: ") + hipGetErrorString(e));
  }
  return I7M_OK;
}

// The SQP loop on device buffers: iteration 1 reads xu_in and its line search writes every
// row of xu_out; later iterations update xu_out in place (xu_in == xu_out is allowed).  The
// first linearisation also initialises the active flags and the stats (no memset launches).
// The B problems use the handle's per-problem work buffers from problem b0 on, and run on
// stream s (h->stream unless the host-to-host path splits the batch into chunks).
// (Splitting a device-resident batch into ranges on several streams, so that waves of different
// kernels share a SIMD, was measured at 2-4 ranges and gave nothing: DESIGN.md §7.)
// d_st: where the stats go; nullptr = the handle's own rows of these problems.
// mark: the staggered ranges' mark, recorded in this solve's first QP (ADMM mode; StaggerMark).
int run_sqp(i7m_handle* h, int B, const double* d_xu_in, double* d_xu, const double* d_xs, const double* d_goals,
            int goal_stride, ProblemStats* d_st, long b0 = 0, hipStream_t s = nullptr, StaggerMark* mark = nullptr) {
  const Bufs W = bufs_at(h, b0);
  const SolveParams P = params_of(h, B, goal_stride);
  if (!s) s = h->stream;
  if (!d_st) d_st = W.stats;
  int* act = W.active;
  double* qbuf = W.sol;
  if (use_fused(h->tune, h->cfg.qp_mode)) return launch_fused(h, s, W, P, d_xu_in, d_xu, d_xs, d_goals, d_st);
  if (h->cfg.qp_mode == I7M_QP_ADMM && B > 0) {
    // this solve's OSQP records start at -1 ("no QP"): a problem that stops after SQP iteration
    // 0 must not report an earlier call's counts for the iterations it did not run
    HIPCHK(hipMemsetAsync(W.adm.iters, 0xff, (size_t)B * I7M_MAX_SQP * sizeof(int), s));
    HIPCHK(hipMemsetAsync(W.adm.status, 0xff, (size_t)B * I7M_MAX_SQP * sizeof(int), s));
  }
  for (int it = 0; it < h->cfg.max_sqp_iters; ++it) {
    const double* xin = it == 0 ? d_xu_in : d_xu;
    int rc;
    if (it == 0)
      rc = launch_linearize(h, s, W, P, xin, d_goals, nullptr, act, d_st);
    else
      rc = launch_linearize(h, s, W, P, xin, d_goals, act);
    if (rc) return rc;
    const double* qsol = nullptr;
    if ((rc = solve_qp(h, s, W, P, xin, d_xs, act, qbuf, &qsol, it, mark))) return rc;
    // mode 2: the ADMM mode's QP solver carries state, so an alpha = 0 iteration is re-solved
    if ((rc = launch_linesearch(h, s, W, P, xin, d_xu, qsol, d_goals, act, d_st, nullptr, it,
                                h->cfg.qp_mode == I7M_QP_ADMM ? 2 : 0, true)))
      return rc;
  }
  return I7M_OK;
}

void drop_graphs(i7m_handle* h) {
  for (auto& g : h->graphs) (void)hipGraphExecDestroy(g.exec);
  h->graphs.clear();
}

// run_sqp through a cached hipGraph: the 6-8 launches of a solve become one graph launch, which
// removes the per-launch host cost and the dispatch gaps (what dominates small-batch latency).
// A graph is keyed by every argument that reaches a kernel; a miss captures the same launch
// sequence once.  Timing runs (events) and multi-range runs go direct.
int run_sqp_graphed(i7m_handle* h, int B, const double* d_xu_in, double* d_xu, const double* d_xs, const double* d_goals,
                    int goal_stride, ProblemStats* d_st) {
  if (!h->tune.use_graph || h->timing)
    return run_sqp(h, B, d_xu_in, d_xu, d_xs, d_goals, goal_stride, d_st);
  const int hf = h->has_fext ? 1 : 0;
  i7m_handle::GraphEntry* hit = nullptr;
  for (auto& g : h->graphs)
    if (g.B == B && g.goal_stride == goal_stride && g.has_fext == hf && g.xu_in == d_xu_in && g.xu == d_xu && g.xs == d_xs &&
        g.goals == d_goals && g.st == d_st && g.stream == (const void*)h->stream)
      hit = &g;
  if (!hit) {
    HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    const int rc = run_sqp(h, B, d_xu_in, d_xu, d_xs, d_goals, goal_stride, d_st);
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (rc) {
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    if (e != hipSuccess) return fail(I7M_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) return fail(I7M_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
    if (h->graphs.size() >= 4) {  // evict the least recently used
      size_t lru = 0;
      for (size_t i = 1; i < h->graphs.size(); ++i)
        if (h->graphs[i].last_use < h->graphs[lru].last_use) lru = i;
      (void)hipGraphExecDestroy(h->graphs[lru].exec);
      h->graphs.erase(h->graphs.begin() + lru);
    }
    h->graphs.push_back({B, goal_stride, hf, d_xu_in, d_xu, d_xs, d_goals, d_st, (const void*)h->stream, exec, 0});
    hit = &h->graphs.back();
  }
  hit->last_use = ++h->graph_clock;
  HIPCHK(hipGraphLaunch(hit->exec, h->stream));
  return I7M_OK;
}

int copy_in(i7m_handle* h, double* dst, const double* src, size_t n, hipStream_t s = nullptr) {
  if (n) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, s ? s : h->stream));
  return I7M_OK;
}
int copy_out(i7m_handle* h, double* dst, const double* src, size_t n, hipStream_t s = nullptr) {
  if (n) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, s ? s : h->stream));
  return I7M_OK;
}

// The inputs of problems [lo, lo + n) from the caller's host arrays (whole-batch pointers) into the
// handle's d_xu / d_xs / d_goal rows, on stream s (nullptr: the handle's).  xcur may be null.
int stage_in(i7m_handle* h, long lo, long n, const double* xu, const double* xcur, const double* goals, int goal_stride,
             hipStream_t s = nullptr) {
  const size_t T = h->T, G = (size_t)h->N * goal_stride;
  int rc;
  if ((rc = copy_in(h, h->d_xu + lo * T, xu + lo * T, n * T, s))) return rc;
  if (xcur && (rc = copy_in(h, h->d_xs + lo * 12, xcur + lo * 12, (size_t)n * 12, s))) return rc;
  return copy_in(h, h->d_goal + lo * G, goals + lo * G, n * G, s);
}
// The results of problems [lo, lo + n): d_xu's rows, and their stats if the caller asked for them.
int stage_out(i7m_handle* h, long lo, long n, double* xu_out, i7m_problem_stats* stats, hipStream_t s = nullptr) {
  const size_t T = h->T;
  if (!s) s = h->stream;
  const int rc = copy_out(h, xu_out + lo * T, h->d_xu + lo * T, n * T, s);
  if (rc) return rc;
  if (stats && n > 0)
    HIPCHK(hipMemcpyAsync(stats + lo, h->d_stats + lo, sizeof(ProblemStats) * (size_t)n, hipMemcpyDeviceToHost, s));
  return I7M_OK;
}
// run_sqp in place on the staged rows [lo, lo + n)
int solve_staged(i7m_handle* h, long lo, long n, int goal_stride, hipStream_t s, StaggerMark* mark = nullptr) {
  double* dxu = h->d_xu + lo * h->T;
  return run_sqp(h, (int)n, dxu, dxu, h->d_xs + lo * 12, h->d_goal + lo * h->N * goal_stride, goal_stride, nullptr, lo, s,
                 mark);
}

// Host-to-host solve in `nch` contiguous chunks of the batch, alternating over two streams: each
// chunk is H2D of its rows -> its SQP -> D2H of its rows and stats, so chunk i's solve runs while
// chunk i+1 is copied in and chunk i-1 copied out (PCIe is full duplex), instead of copy-in,
// solve, copy-out back to back.  Ordered after earlier work on h->stream; synchronous.
int solve_h2h_alternating(i7m_handle* h, int B, const double* xu_in, const double* xcur, const double* goals,
                          int goal_stride, double* xu_out, i7m_problem_stats* stats, int nch) {
  int rc;
  HIPCHK(hipEventRecord(h->ev_order, h->stream));
  for (int c = 0; c < 2; ++c) HIPCHK(hipStreamWaitEvent(h->cs[c], h->ev_order, 0));
  for (int i = 0; i < nch; ++i) {
    const long lo = chunk_lo(B, nch, i, false), hi = chunk_lo(B, nch, i + 1, false);
    const int n = (int)(hi - lo);
    if (n == 0) continue;
    hipStream_t s = h->cs[i & 1];
    if ((rc = stage_in(h, lo, n, xu_in, xcur, goals, goal_stride, s)) || (rc = solve_staged(h, lo, n, goal_stride, s)) ||
        (rc = stage_out(h, lo, n, xu_out, stats, s)))
      return rc;
  }
  for (int c = 0; c < 2; ++c) {
    HIPCHK(hipEventRecord(h->ev_done[c], h->cs[c]));
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_done[c], 0));
  }
  return i7m_synchronize(h);
}

// The chunks as a three-stage pipeline: copies in on cs[0], the solves on the handle's stream
// (h2h_pipe 1) or alternating between it and cs2 (2, default: a chunk's solve can start while the
// previous one drains), copies out on cs[1]; chunk i's solve waits only for its own copy-in, its
// copy-out only for its solve.  Issued in the order in(0) solve(0) [in(i) solve(i) out(i-1)]...
// out(n-1): with pinned host memory every call returns at once and the three queues overlap; with
// pageable memory (whose copies block the calling thread until done) the host still copies chunk
// i in, and chunk i-1 out, while the device solves the chunk before.  The alternating two-stream
// layout above issued all copy-ins at once: they shared the link and finished together, then the
// solves ran, then the copy-outs — no overlap.
int solve_h2h_pipelined(i7m_handle* h, int B, const double* xu_in, const double* xcur, const double* goals,
                        int goal_stride, double* xu_out, i7m_problem_stats* stats, int nch) {
  while ((int)h->ev_in.size() < nch) {
    hipEvent_t a = nullptr, b = nullptr;
    HIPCHK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
    if (hipEventCreateWithFlags(&b, hipEventDisableTiming) != hipSuccess) {
      (void)hipEventDestroy(a);
      return fail(I7M_EHIP, "chunk event creation failed");
    }
    h->ev_in.push_back(a);
    h->ev_cmp.push_back(b);
  }
  int rc;
  if (h->tune.h2h_pipe >= 2 && !h->cs2) HIPCHK(hipStreamCreateWithFlags(&h->cs2, hipStreamNonBlocking));
  HIPCHK(hipEventRecord(h->ev_order, h->stream));
  for (int c = 0; c < 2; ++c) HIPCHK(hipStreamWaitEvent(h->cs[c], h->ev_order, 0));
  if (h->tune.h2h_pipe >= 2) HIPCHK(hipStreamWaitEvent(h->cs2, h->ev_order, 0));
  auto sstream = [&](int i) { return (h->tune.h2h_pipe >= 2 && (i & 1)) ? h->cs2 : h->stream; };
  auto lo_of = [&](int i) { return chunk_lo(B, nch, i, h->tune.h2h_taper != 0); };
  // (each stage keeps its status in a local: with h2h_pipe 3 out() runs on another thread)
  auto in = [&](int i) -> int {
    const long lo = lo_of(i), n = lo_of(i + 1) - lo;
    const int r = stage_in(h, lo, n, xu_in, xcur, goals, goal_stride, h->cs[0]);
    if (r) return r;
    HIPCHK(hipEventRecord(h->ev_in[i], h->cs[0]));
    return I7M_OK;
  };
  // ADMM mode where the device solve staggers, in two chunks: the second chunk's solve also waits
  // for the first's mark (its first scaling + factor), as the staggered halves of i7m_solve_device
  const bool stag = nch == 2 && stagger_applies(h->tune, h->cfg.qp_mode, B);
  StaggerMark mark{h->ev_rmark, h->tune.admm_stagger, false};
  auto solve = [&](int i) -> int {
    const long lo = lo_of(i), n = lo_of(i + 1) - lo;
    const hipStream_t ss = sstream(i);
    HIPCHK(hipStreamWaitEvent(ss, h->ev_in[i], 0));
    if (i == 1 && mark.recorded) HIPCHK(hipStreamWaitEvent(ss, mark.ev, 0));
    const int r = n > 0 ? solve_staged(h, lo, n, goal_stride, ss, stag && i == 0 ? &mark : nullptr) : I7M_OK;
    if (r) return r;
    HIPCHK(hipEventRecord(h->ev_cmp[i], ss));
    return I7M_OK;
  };
  auto out = [&](int i) -> int {
    const long lo = lo_of(i), n = lo_of(i + 1) - lo;
    HIPCHK(hipStreamWaitEvent(h->cs[1], h->ev_cmp[i], 0));
    return stage_out(h, lo, n, xu_out, stats, h->cs[1]);
  };
  if (h->tune.h2h_pipe == 3) {
    // copies out on a second host thread: a pageable copy blocks the thread that issues it, so
    // with one thread every copy-out sat between two copy-ins and the link ran one direction at a
    // time; here the calling thread issues in(0) solve(0) in(1) solve(1) ... back to back while the
    // helper issues out(i) as soon as solve(i) has been issued (it then blocks in the copy until
    // the solve and the copy are done) — both directions of the link in flight together
    std::atomic<int> issued{0};
    int rc_out = I7M_OK;
    std::string err_out;
    std::thread helper([&] {
      if (hipSetDevice(h->dev) != hipSuccess) {
        rc_out = I7M_EHIP;
        err_out = "hipSetDevice failed (copy-out thread)";
        return;
      }
      int r = I7M_OK;
      for (int i = 0; i < nch && r == I7M_OK; ++i) {
        int k;
        while ((k = issued.load(std::memory_order_acquire)) <= i) {
          if (k < 0) return;  // the calling thread failed: nothing more to copy
          std::this_thread::yield();
        }
        r = out(i);
      }
      if (r != I7M_OK) {
        rc_out = r;
        err_out = g_err;  // thread_local: hand the message to the calling thread
      }
    });
    int r = I7M_OK;
    for (int i = 0; i < nch && r == I7M_OK; ++i) {
      if ((r = in(i)) == I7M_OK && (r = solve(i)) == I7M_OK) issued.store(i + 1, std::memory_order_release);
    }
    if (r != I7M_OK) issued.store(-1, std::memory_order_release);
    helper.join();
    if (r != I7M_OK) return r;
    if (rc_out != I7M_OK) return fail(rc_out, err_out);
  } else {
    if ((rc = in(0)) || (rc = solve(0))) return rc;
    for (int i = 1; i < nch; ++i)
      if ((rc = in(i)) || (rc = solve(i)) || (rc = out(i - 1))) return rc;
    if ((rc = out(nch - 1))) return rc;
  }
  HIPCHK(hipEventRecord(h->ev_done[1], h->cs[1]));
  HIPCHK(hipStreamWaitEvent(h->stream, h->ev_done[1], 0));
  return i7m_synchronize(h);
}

// Error exit of a chunked call: chunks already queued on cs[0], cs[1] and cs2 keep
// running after a failed call returns, and their copies out could land in caller memory after the
// error (or race the next call's copies in, which order only after h->stream).  So every error
// return waits for all the streams the chunks use (their own errors ignored; the first message kept).
int drain_after_error(i7m_handle* h, int rc) {
  if (rc == I7M_OK) return rc;
  const std::string msg = g_err;
  for (int c = 0; c < 2; ++c)
    if (h->cs[c]) (void)hipStreamSynchronize(h->cs[c]);
  if (h->cs2) (void)hipStreamSynchronize(h->cs2);
  (void)hipStreamSynchronize(h->stream);
  g_err = msg;
  return rc;
}
int solve_h2h_chunked(i7m_handle* h, int B, const double* xu_in, const double* xcur, const double* goals, int goal_stride,
                      double* xu_out, i7m_problem_stats* stats, int nch) {
  const auto body = h->tune.h2h_pipe ? solve_h2h_pipelined : solve_h2h_alternating;
  return drain_after_error(h, body(h, B, xu_in, xcur, goals, goal_stride, xu_out, stats, nch));
}

// body(lo, n, stream, mark) enqueues the work of problems [lo, lo + n).  Where the batch staggers
// (stagger_applies) it runs as two contiguous ranges on cs[0] and cs[1], the second started when
// the first has passed its mark (the first run_sqp of `body` records it; StaggerMark), both forked
// from and joined back into h->stream; otherwise the whole batch runs on h->stream.  Results are
// the one-range run's: the problems are independent.
// cut: where the second range begins; -1 = stagger_cut(B) (a caller whose problems come in groups
// passes a cut that splits none).
template <class Body>
int run_ranges(i7m_handle* h, int B, Body&& body, long cut = -1) {
  if (!stagger_applies(h->tune, h->cfg.qp_mode, B)) return body(0L, B, h->stream, (StaggerMark*)nullptr);
  const long cuts[3] = {0, cut < 0 ? stagger_cut(B) : cut, B};
  StaggerMark mark{h->ev_rmark, h->tune.admm_stagger, false};
  HIPCHK(hipEventRecord(h->ev_order, h->stream));
  for (int r = 0; r < 2; ++r) {
    const long lo = cuts[r], hi = cuts[r + 1];
    HIPCHK(hipStreamWaitEvent(h->cs[r], h->ev_order, 0));
    if (hi <= lo) continue;
    if (r == 1 && mark.recorded) HIPCHK(hipStreamWaitEvent(h->cs[1], mark.ev, 0));
    const int rc = body(lo, (int)(hi - lo), h->cs[r], r == 0 ? &mark : nullptr);
    if (rc) {
      // join the ranges already started back into h->stream before the error returns:
      // a caller that synchronises h->stream and then releases memory (Workspace) must not race them
      const std::string msg = g_err;
      for (int q = 0; q <= r; ++q) {
        (void)hipEventRecord(h->ev_done[q], h->cs[q]);
        (void)hipStreamWaitEvent(h->stream, h->ev_done[q], 0);
      }
      g_err = msg;
      return rc;
    }
  }
  for (int r = 0; r < 2; ++r) {
    HIPCHK(hipEventRecord(h->ev_done[r], h->cs[r]));
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_done[r], 0));
  }
  return I7M_OK;
}

// The checks every ADMM state accessor starts with; on I7M_OK with B > 0 the device is current and
// *a is the layout from problem 0.  (B == 0 passes: the caller returns I7M_OK without work.)
int admm_rows(i7m_handle* h, int B, AdmmArgs* a) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (h->cfg.qp_mode != I7M_QP_ADMM) return fail(I7M_EINVAL, "handle is not in I7M_QP_ADMM mode");
  if (B < 0 || B > h->cfg.max_batch) return fail(I7M_EINVAL, "batch outside [0, max_batch]");
  if (B == 0) return I7M_OK;
  HIPCHK(hipSetDevice(h->dev));
  *a = admm_layout(h, 0);
  return I7M_OK;
}

// The OSQP state of problems [lo, lo + n) afresh (what: I7M_ADMM_RESET_* bits), asynchronous on
// stream s.  rho: n values for these rows, copied as `kind` (from the host, or device to device).
int admm_reset_rows(i7m_handle* h, long lo, long n, int what, hipStream_t s, const double* rho, hipMemcpyKind kind) {
  const size_t T = h->T, m = 12 * (size_t)h->N;
  const AdmmArgs a = admm_layout(h, lo);
  if (what & I7M_ADMM_RESET_PRIMAL) {
    HIPCHK(hipMemsetAsync(a.sx, 0, n * T * 8, s));
    HIPCHK(hipMemsetAsync(a.sz, 0, n * m * 8, s));
    HIPCHK(hipMemsetAsync(a.sq, 0, n * T * 8, s));
  }
  if (what & I7M_ADMM_RESET_DUAL) HIPCHK(hipMemsetAsync(a.sy, 0, n * m * 8, s));
  if (what & I7M_ADMM_RESET_RHO) HIPCHK(hipMemcpyAsync(a.srho, rho, (size_t)n * 8, kind, s));
  return I7M_OK;
}
// A closed loop's reset before a solve: rows [lo, lo + n) afresh on stream s, their rho from the
// run's initial values d_rho0 (row 0 first).  Nothing outside I7M_QP_ADMM or for what = 0.
int loop_reset(i7m_handle* h, long lo, long n, int what, hipStream_t s, const double* d_rho0) {
  if (h->cfg.qp_mode != I7M_QP_ADMM || !what) return I7M_OK;
  return admm_reset_rows(h, lo, n, what, s, d_rho0 + lo, hipMemcpyDeviceToDevice);
}

// One closed-loop call's device memory beyond the handle's: a Carved (base null: the allocation
// failed) whose destructor synchronises the handle's stream before it frees, so on every return,
// error or not, nothing queued still uses the memory.
struct Workspace : Carved {
  i7m_handle* h;
  template <size_t NB>
  Workspace(i7m_handle* hh, const size_t (&bytes)[NB]) : h(hh) {
    alloc(bytes, (int)NB, false);
  }
  Workspace(const Workspace&) = delete;
  ~Workspace() {
    (void)hipStreamSynchronize(h->stream);
    release();
  }
};

// The start of a closed loop on the handle's stream (src/osqp_mpc.py:14-27,
// src/gato_mpc_batch_sample.py:111-128): every row's goal = endpoint 0 at every knot, XU = 0, the
// endpoints on the device, and per instance goal index 0 and alive.  The host staging is the
// LoopStart, which the caller keeps until its final synchronize.
struct LoopStart {
  size_t rows;
  std::vector<double> goals;
  std::vector<int> ones;
  LoopStart(const i7m_handle* h, size_t rows_, size_t instances, const double* endpoints)
      : rows(rows_), goals(rows_ * 3 * h->N), ones(instances, 1) {
    for (size_t k = 0; k < goals.size(); ++k) goals[k] = endpoints[k % 3];
  }
  // the tracking loop's start (gato_controller.py:180-183): every row of group g (H rows each) gets
  // the reference's window at the group's phase and offset 0
  LoopStart(const i7m_handle* h, size_t rows_, size_t instances, int H, const double* ref, long L, int ref_stride,
            const int32_t* ref_phase)
      : rows(rows_), goals(rows_ * 3 * h->N), ones(instances, 1) {
    const size_t W = 3 * h->N;
    for (size_t b = 0; b < rows; ++b)
      for (size_t e = 0; e < W; ++e)
        goals[b * W + e] = ref[track_index(ref_phase ? ref_phase[b / H] : 0, 0, (long)(e / 3), L) * ref_stride + e % 3];
  }
};
int loop_instances(i7m_handle* h, const LoopStart& st, const double* endpoints, int n_endpoints, double* d_ep, int* d_gi,
                   int* d_alive) {
  const int rc = copy_in(h, d_ep, endpoints, 3 * (size_t)n_endpoints);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(d_gi, 0, 4 * st.ones.size(), h->stream));
  HIPCHK(hipMemcpyAsync(d_alive, st.ones.data(), 4 * st.ones.size(), hipMemcpyHostToDevice, h->stream));
  return I7M_OK;
}
int loop_start(i7m_handle* h, const LoopStart& st, const double* endpoints, int n_endpoints, double* d_ep, int* d_gi,
               int* d_alive) {
  int rc;
  if ((rc = copy_in(h, h->d_goal, st.goals.data(), st.goals.size()))) return rc;
  if ((rc = loop_instances(h, st, endpoints, n_endpoints, d_ep, d_gi, d_alive))) return rc;
  HIPCHK(hipMemsetAsync(h->d_xu, 0, 8 * st.rows * h->T, h->stream));
  return I7M_OK;
}

// The start of the sampled-wrench family (the loops, the controller session): G groups of H rows,
// every row of group g at state x[g], or at the zero state where x is null.  The host staging of
// the goal rows, the rows' states and their initial rho; the caller keeps it until its synchronize.
struct GroupStart {
  LoopStart rows;
  std::vector<double> xrows, rho0;
  GroupStart(const i7m_handle* h, int G, int H, const double* x, const GoalSource& gs)
      : rows(gs.ref ? LoopStart(h, (size_t)G * H, G, H, gs.ref, gs.L, gs.ref_stride, gs.ref_phase)
                    : LoopStart(h, (size_t)G * H, G, gs.endpoints)),
        xrows((size_t)G * H * 12, 0.0), rho0((size_t)G * H, h->cfg.admm_rho) {
    for (size_t b = 0; x && b < rho0.size(); ++b)
      for (int r = 0; r < 12; ++r) xrows[b * 12 + r] = x[(b / H) * 12 + r];
  }
};
// Queues it on the handle's stream: d_xs, the goal rows, XU = [x, 0...], the rows' rho into d_rho0
// and, for a tracking source, the reference into d_ref and the groups' phases into d_phase (null
// without phases).
int stage_start(i7m_handle* h, const GroupStart& st, const GoalSource& gs, int G, double* d_rho0, double* d_ref,
                int* d_phase) {
  const size_t T = h->T, B = st.rho0.size();
  int rc;
  if ((rc = copy_in(h, h->d_xs, st.xrows.data(), st.xrows.size()))) return rc;
  if ((rc = copy_in(h, h->d_goal, st.rows.goals.data(), st.rows.goals.size()))) return rc;
  HIPCHK(hipMemsetAsync(h->d_xu, 0, 8 * B * T, h->stream));
  if (B > 0)
    HIPCHK(hipMemcpy2DAsync(h->d_xu, T * 8, st.xrows.data(), 12 * 8, 12 * 8, B, hipMemcpyHostToDevice, h->stream));
  if ((rc = copy_in(h, d_rho0, st.rho0.data(), B))) return rc;
  if (gs.ref && (rc = copy_in(h, d_ref, gs.ref, (size_t)gs.L * gs.ref_stride))) return rc;
  if (d_phase) HIPCHK(hipMemcpyAsync(d_phase, gs.ref_phase, 4 * (size_t)G, hipMemcpyHostToDevice, h->stream));
  return I7M_OK;
}

// The joint-6 wrenches of rows [0, B) (host, frame `frame`) as the handle's, the rows beyond them
// zero.  The handle's flags change, and the captured graphs (which hold the wrench kernel choice) go,
// only once the copy is known to have landed.
int install_wrench(i7m_handle* h, int B, const double* fext, int frame) {
  HIPCHK(hipMemsetAsync(h->d_fext, 0, (size_t)h->cfg.max_batch * 6 * 8, h->stream));
  const int rc = copy_in(h, h->d_fext, fext, (size_t)B * 6);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  h->has_fext = true;
  h->fext_frame = frame;
  drop_graphs(h);
  return I7M_OK;
}

// The query hooks' chunk loop: Bq queries, at most scratch / per_query a chunk.  Chunk rows of the
// inputs (w doubles per query each; a null host pointer keeps its slot and copies nothing) go to
// consecutive slots of d_aux, launch(n, in, out) runs, and the outputs come back from consecutive
// slots of d_sol, or from `dev` where an output names a buffer of its own.
struct QueryIn { const double* host; int w; };
struct QueryOut { double* host; int w; double* dev = nullptr; };
template <class Launch>
int query_chunks(i7m_handle* h, int Bq, int per_query, std::initializer_list<QueryIn> ins,
                 std::initializer_list<QueryOut> outs, Launch&& launch) {
  HIPCHK(hipSetDevice(h->dev));
  const size_t cap = h->scratch / per_query;
  int rc;
  for (size_t o = 0; o < (size_t)Bq; o += cap) {
    const size_t n = std::min(cap, (size_t)Bq - o);
    double *in[4], *out[4];
    size_t at = 0, k = 0;
    for (const QueryIn& q : ins) {
      in[k] = h->d_aux + at * n;
      if (q.host && (rc = copy_in(h, in[k], q.host + q.w * o, q.w * n))) return rc;
      at += q.w;
      ++k;
    }
    at = k = 0;
    for (const QueryOut& q : outs) {
      out[k++] = q.dev ? q.dev : h->d_sol + at * n;
      if (!q.dev) at += q.w;
    }
    launch((int)n, in, out);
    HIPCHK(hipGetLastError());
    k = 0;
    for (const QueryOut& q : outs) {
      if (q.host && (rc = copy_out(h, q.host + q.w * o, out[k], q.w * n))) return rc;
      ++k;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return I7M_OK;
}

}  // namespace

extern "C" {

const char* i7m_last_error(void) { return g_err.c_str(); }

#ifdef I7M_DIAG
// Diagnostic library only (not declared in include/indy7_mpc.h): point every instrumented
// kernel of both translation units at a per-wave timeline buffer (i7m_timeline.h; nullptr: off).
int i7m_lin_tu_set_timeline(void* p);
int i7m_admm_prep_tu_set_timeline(void* p);
int i7m_diag_timeline(void* p) {
  return (i7m::tl_set(p) == 0 && i7m_lin_tu_set_timeline(p) == 0 && i7m_admm_prep_tu_set_timeline(p) == 0) ? 0 : -1;
}
#endif

int i7m_abi_version(void) { return I7M_ABI_VERSION; }

const char* i7m_version(void) { return "indy7_mpc_amd 0.3 (gfx950, fp64, " I7M_BUILD_KIND ") src " I7M_SRC_HASH; }

int i7m_device_count(int* n) {
  if (!n) return fail(I7M_EINVAL, "null");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    return fail(I7M_ENODEV, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *n = c;
  return I7M_OK;
}

int i7m_config_default(i7m_config* c) {
  if (!c) return fail(I7M_EINVAL, "null config");
  i7m_model keep = c->model;
  std::memset(c, 0, sizeof(*c));
  c->model = keep;
  c->N = 32;
  c->regularize = 1;
  c->dt = 0.01;
  c->dQ_cost = 0.01;
  c->R_cost = 1e-5;
  c->QN_cost = 100.0;
  c->eps = 1.0;
  c->mu = 10.0;
  c->step_tol = 1e-3;
  c->max_sqp_iters = 2;
  c->max_batch = 1;
  c->device_id = 0;
  c->qp_mode = I7M_QP_DIRECT;
  c->box_mask = I7M_BOX_Q | I7M_BOX_V | I7M_BOX_U;
  c->box_max_iters = 30;
  c->box_tol = 1e-8;
  // OSQP's defaults, with the duality-gap test and no rho adaptation: the settings that reproduce
  // the reference's printed closed loop (oracle/osqp_admm.py)
  c->admm_rho = 0.1;
  c->admm_sigma = 1e-6;
  c->admm_alpha = 1.6;
  c->admm_eps_abs = 1e-3;
  c->admm_eps_rel = 1e-3;
  c->admm_max_iter = 4000;
  c->admm_check_termination = 25;
  c->admm_scaling = 10;
  c->admm_check_dualgap = 1;
  c->admm_adaptive_rho_interval = 0;
  c->admm_adaptive_rho_tolerance = 5.0;
  c->precision = I7M_PREC_F64;
  return I7M_OK;
}

int i7m_create(const i7m_config* cfg, i7m_handle** out) {
  if (!cfg || !out) return fail(I7M_EINVAL, "null argument");
  *out = nullptr;
  if (cfg->N < 2 || cfg->N > I7M_MAX_N) return fail(I7M_EINVAL, "N must be in [2, 64]");
  if (cfg->max_batch < 1) return fail(I7M_EINVAL, "max_batch must be >= 1");
  if (cfg->precision != I7M_PREC_F64)
    return fail(I7M_EINVAL, cfg->precision == I7M_PREC_F32
                                ? "precision I7M_PREC_F32 is not built: every kernel computes in double (I7M_PREC_F64)"
                                : "unknown precision");
  if (cfg->max_sqp_iters < 1 || cfg->max_sqp_iters > I7M_MAX_SQP) return fail(I7M_EINVAL, "max_sqp_iters in [1, 8]");
  if (cfg->qp_mode != I7M_QP_DIRECT && cfg->qp_mode != I7M_QP_BOX && cfg->qp_mode != I7M_QP_ADMM)
    return fail(I7M_EINVAL, "unsupported qp_mode");
  if (cfg->qp_mode == I7M_QP_ADMM) {
    if (!(cfg->admm_rho > 0.0) || !(cfg->admm_sigma > 0.0)) return fail(I7M_EINVAL, "admm_rho and admm_sigma must be > 0");
    if (!(cfg->admm_alpha > 0.0 && cfg->admm_alpha < 2.0)) return fail(I7M_EINVAL, "admm_alpha must be in (0, 2)");
    if (!(cfg->admm_eps_abs >= 0.0) || !(cfg->admm_eps_rel >= 0.0)) return fail(I7M_EINVAL, "admm eps must be >= 0");
    if (cfg->admm_max_iter < 1 || cfg->admm_max_iter > 1000000) return fail(I7M_EINVAL, "admm_max_iter in [1, 1e6]");
    if (cfg->admm_check_termination < 0 || cfg->admm_scaling < 0 || cfg->admm_scaling > 100 ||
        cfg->admm_adaptive_rho_interval < 0)
      return fail(I7M_EINVAL, "admm_check_termination / admm_adaptive_rho_interval >= 0, admm_scaling in [0, 100]");
    if (!(cfg->admm_adaptive_rho_tolerance >= 1.0)) return fail(I7M_EINVAL, "admm_adaptive_rho_tolerance must be >= 1");
  }
  if (cfg->pipeline < I7M_PIPE_AUTO || cfg->pipeline > I7M_PIPE_FUSED_ITER) return fail(I7M_EINVAL, "unsupported pipeline");
  if (cfg->qp_mode == I7M_QP_BOX) {
    if (cfg->box_mask < 0 || cfg->box_mask > 7) return fail(I7M_EINVAL, "box_mask must be a subset of Q|V|U (0..7)");
    if (cfg->box_max_iters < 1 || cfg->box_max_iters > 200) return fail(I7M_EINVAL, "box_max_iters in [1, 200]");
    if (!(cfg->box_tol > 0.0)) return fail(I7M_EINVAL, "box_tol must be > 0");
  }
  if (!(cfg->dt > 0.0)) return fail(I7M_EINVAL, "dt must be > 0");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) return fail(I7M_ENODEV, "no HIP device available");
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(I7M_EINVAL, "device_id out of range");
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, cfg->device_id));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(I7M_ENODEV, std::string("built for gfx950, device is ") + prop.gcnArchName);

  i7m_handle* h = new i7m_handle();
  h->cfg = *cfg;
  h->dev = cfg->device_id;
  auto bail = [&](int rc) {
    i7m_destroy(h);
    return rc;
  };
  if (hipSetDevice(h->dev) != hipSuccess) return bail(fail(I7M_EHIP, "hipSetDevice failed"));
  // the handle's own stream is a blocking one: it orders with the legacy null stream, so a caller
  // that fills the inputs on the default (null) stream and never calls i7m_set_stream still has
  // its copies ordered before the solve and the solve before its reads
  if (hipStreamCreateWithFlags(&h->own, hipStreamDefault) != hipSuccess)
    return bail(fail(I7M_EHIP, "hipStreamCreate failed"));
  h->stream = h->own;
#ifdef I7M_DIAG
  if (const char* e = std::getenv("I7M_ABLATE")) {
    h->ablate = std::atoi(e);
    const AblateStatus as = ablate_status(h->ablate);
    if (as.kind != Ablate::known) return bail(fail(I7M_EINVAL, std::string("I7M_ABLATE=") + e + ": " + as.msg));
  }
#else
  if (std::getenv("I7M_ABLATE"))
    return bail(fail(I7M_EINVAL, "I7M_ABLATE is set, but this is the release library: the ablation "
                                 "timing kernels exist only in the -DI7M_DIAG build (tools/)"));
#endif
  if (const char* e = std::getenv("I7M_POLICY_ZERO_K")) h->policy_zero_k = std::atoi(e) != 0;
  std::string tune_err;
  if (!tuning_from_env(*cfg, &h->tune, &tune_err)) return bail(fail(I7M_EINVAL, tune_err));
  if (hipStreamCreateWithFlags(&h->cs[0], hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&h->cs[1], hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_order, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_done[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_done[1], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_rmark, hipEventDisableTiming) != hipSuccess)
    return bail(fail(I7M_EHIP, "chunk stream / event creation failed"));
  if (h->tune.pipeline == I7M_PIPE_FUSED || h->tune.pipeline == I7M_PIPE_FUSED_ITER) {
    const hipError_t ef = i7m_prepare_sqp_fused(h->dev, cfg->N);
    if (ef != hipSuccess) return bail(fail(I7M_EHIP, std::string("k_sqp_fused LDS limit: ") + hipGetErrorString(ef)));
  }
  h->N = cfg->N;
  h->T = 18 * h->N - 6;
  const size_t Bm = (size_t)cfg->max_batch, N = (size_t)h->N, T = (size_t)h->T;
  // scratch for the query hooks: >= 114 doubles for each of >= 256 queries
  h->scratch = std::max(Bm * T, (size_t)256 * 114);
  bool ok = true;
  auto need = [&](auto** p, size_t bytes) { ok = ok && dev_alloc(h, p, bytes); };
  need(&h->d_model, sizeof(DevModel));
  need(&h->d_xu, Bm * T * 8);
  need(&h->d_xs, Bm * 12 * 8);
  need(&h->d_goal, Bm * N * 6 * 8);
  need(&h->d_sol, h->scratch * 8);
  need(&h->d_lin, Bm * (N - 1) * LIN_STRIDE * 8);
  need(&h->d_cost, Bm * N * COST_STRIDE * 8);
  need(&h->d_kbuf, Bm * (N - 1) * KBUF_STRIDE * 8);
  need(&h->d_aux, h->scratch * 8);
  need(&h->d_qpd, Bm * (N - 1) * QPD_STRIDE * 8);
  need(&h->d_out, h->scratch * 8);
  need(&h->d_active, Bm * sizeof(int));
  need(&h->d_stats, Bm * sizeof(ProblemStats));
  need(&h->d_fext, Bm * 6 * 8);
  need(&h->d_lsbase, Bm * 8);
  need(&h->d_lspend, Bm * sizeof(int));
  if (cfg->qp_mode == I7M_QP_BOX) {
    for (double** p : {&h->d_bx, &h->d_bzl, &h->d_bzu, &h->d_bsig, &h->d_bh, &h->d_bdxa}) need(p, Bm * T * 8);
    need(&h->d_bhinv, Bm * (N - 1) * 36 * 8);
    need(&h->d_bdh, Bm * T * 8);
    need(&h->d_bst, Bm * sizeof(IpmState));
    need(&h->d_bact, Bm * sizeof(int));
  }
  if (ok && cfg->qp_mode == I7M_QP_ADMM) {
    // k_admm_iter addresses the allocation with 32-bit byte offsets below its 0x7ff00000 marker
    const size_t admm_bytes = (size_t)admm_walk(h).total * 8;
    if (admm_bytes >= 0x7ff00000ull)
      return bail(fail(I7M_EINVAL, "ADMM mode: max_batch=" + std::to_string(cfg->max_batch) + " at N=" + std::to_string(N) +
                                       " needs over 2 GiB of ADMM state; use a smaller max_batch per handle"));
    need(&h->d_admm, admm_bytes);
    need(&h->d_admm_it, 2 * Bm * I7M_MAX_SQP * sizeof(int));
    if (ok && i7m_admm_reset(h, cfg->max_batch, I7M_ADMM_RESET_ALL) != I7M_OK) ok = false;
  }
  if (!ok) return bail(fail(I7M_ENOMEM, "hipMalloc failed for max_batch=" + std::to_string(cfg->max_batch)));
  DevModel dm = make_dev_model(cfg->model);
  // the Indy7-specialised kernels are used only for a model bit-identical to the baked one
  h->spec = std::memcmp(&dm, &kIndy7Model, sizeof(DevModel)) == 0 && !h->tune.generic;
  if (hipMemcpy(h->d_model, &dm, sizeof(dm), hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail(I7M_EHIP, "model upload failed"));
  *out = h;
  return I7M_OK;
}

void i7m_destroy(i7m_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->dev);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : h->owned) (void)hipFree(p);
  ctrl_release(h);
  for (auto& t : h->ev) {
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  for (auto e : h->pool) (void)hipEventDestroy(e);
  for (auto e : h->ev_in) (void)hipEventDestroy(e);
  for (auto e : h->ev_cmp) (void)hipEventDestroy(e);
  drop_graphs(h);
  if (h->cs2) {
    (void)hipStreamSynchronize(h->cs2);
    (void)hipStreamDestroy(h->cs2);
  }
  for (int c = 0; c < 2; ++c) {
    if (h->cs[c]) {
      (void)hipStreamSynchronize(h->cs[c]);
      (void)hipStreamDestroy(h->cs[c]);
    }
    if (h->ev_done[c]) (void)hipEventDestroy(h->ev_done[c]);
  }
  if (h->ev_order) (void)hipEventDestroy(h->ev_order);
  if (h->ev_rmark) (void)hipEventDestroy(h->ev_rmark);
  if (h->own) (void)hipStreamDestroy(h->own);
  delete h;
}

int i7m_set_stream(i7m_handle* h, void* stream) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (h->ctrl.open) return session_open();
  h->stream = stream ? (hipStream_t)stream : h->own;
  return I7M_OK;
}

int i7m_set_external_wrench(i7m_handle* h, int32_t B, const double* fext, int32_t frame) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (h->ctrl.open) return session_open();
  if (!fext) {
    h->has_fext = false;
    drop_graphs(h);  // captured graphs hold the wrench kernel choice
    return I7M_OK;
  }
  if (frame != I7M_WRENCH_LOCAL && frame != I7M_WRENCH_WORLD)
    return fail(I7M_EINVAL, "frame must be I7M_WRENCH_LOCAL or I7M_WRENCH_WORLD");
  if (B < 1 || B > h->cfg.max_batch) return fail(I7M_EINVAL, "external wrench batch outside [1, max_batch]");
  HIPCHK(hipSetDevice(h->dev));
  return install_wrench(h, B, fext, frame);
}

int i7m_reset(i7m_handle* h) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (h->ctrl.open) return session_open();
  HIPCHK(hipSetDevice(h->dev));
  HIPCHK(hipStreamSynchronize(h->stream));
  drop_graphs(h);
  if (h->cfg.qp_mode == I7M_QP_ADMM) {
    const int rc = i7m_admm_reset(h, h->cfg.max_batch, I7M_ADMM_RESET_ALL);
    if (rc) return rc;
  }
  return i7m_reset_kernel_times(h);
}

int i7m_admm_reset(i7m_handle* h, int32_t B, int32_t what) {
  if (h && h->ctrl.open) return session_open();
  AdmmArgs a{};
  int rc = admm_rows(h, B, &a);
  if (rc) return rc;
  if (what & ~I7M_ADMM_RESET_ALL) return fail(I7M_EINVAL, "unknown I7M_ADMM_RESET_* bits");
  if (B == 0) return I7M_OK;
  const std::vector<double> rho((size_t)B, h->cfg.admm_rho);
  if ((rc = admm_reset_rows(h, 0, B, what, h->stream, rho.data(), hipMemcpyHostToDevice))) return rc;
  HIPCHK(hipMemsetAsync(a.iters, 0xff, (size_t)B * I7M_MAX_SQP * sizeof(int), h->stream));
  HIPCHK(hipMemsetAsync(a.status, 0xff, (size_t)B * I7M_MAX_SQP * sizeof(int), h->stream));
  return i7m_synchronize(h);
}

int i7m_get_admm_stats(i7m_handle* h, int32_t B, int32_t* iters, double* rho) {
  AdmmArgs a{};
  const int rc = admm_rows(h, B, &a);
  if (rc || B == 0) return rc;
  if (iters) HIPCHK(hipMemcpyAsync(iters, a.iters, (size_t)B * I7M_MAX_SQP * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (rho) HIPCHK(hipMemcpyAsync(rho, a.srho, (size_t)B * 8, hipMemcpyDeviceToHost, h->stream));
  return i7m_synchronize(h);
}

int i7m_get_admm_status(i7m_handle* h, int32_t B, int32_t* status) {
  if (!h || !status) return fail(I7M_EINVAL, "null handle or output");
  AdmmArgs a{};
  const int rc = admm_rows(h, B, &a);
  if (rc || B == 0) return rc;
  HIPCHK(hipMemcpyAsync(status, a.status, (size_t)B * I7M_MAX_SQP * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return i7m_synchronize(h);
}

int i7m_get_admm_dual(i7m_handle* h, int32_t B, double* y) {
  if (!h || !y) return fail(I7M_EINVAL, "null handle or output");
  AdmmArgs a{};
  int rc = admm_rows(h, B, &a);
  if (rc || B == 0) return rc;
  const long m = 12 * h->N;
  std::vector<double> e((size_t)B * m), c((size_t)B);
  if ((rc = copy_out(h, y, a.sy, (size_t)B * m)) || (rc = copy_out(h, e.data(), a.E, (size_t)B * m)) ||
      (rc = copy_out(h, c.data(), a.cs, (size_t)B)))
    return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  // OSQP's unscale_solution: y = E y_s / c, with the scaling of each problem's last QP
  for (long b = 0; b < B; ++b)
    for (long r = 0; r < m; ++r) y[b * m + r] = e[b * m + r] * y[b * m + r] / c[b];
  return I7M_OK;
}

int i7m_get_admm_state(i7m_handle* h, int32_t B, double* x, double* z, double* y, double* q, double* rho) {
  AdmmArgs a{};
  int rc = admm_rows(h, B, &a);
  if (rc || B == 0) return rc;
  const size_t T = h->T, m = 12 * (size_t)h->N;
  if (x && (rc = copy_out(h, x, a.sx, (size_t)B * T))) return rc;
  if (z && (rc = copy_out(h, z, a.sz, (size_t)B * m))) return rc;
  if (y && (rc = copy_out(h, y, a.sy, (size_t)B * m))) return rc;
  if (q && (rc = copy_out(h, q, a.sq, (size_t)B * T))) return rc;
  if (rho && (rc = copy_out(h, rho, a.srho, (size_t)B))) return rc;
  return i7m_synchronize(h);
}

int i7m_synchronize(i7m_handle* h) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  HIPCHK(hipStreamSynchronize(h->stream));
  return I7M_OK;
}

int i7m_solve_device(i7m_handle* h, int32_t B, const double* d_xu_in, const double* d_xcur, const double* d_goals,
                     int32_t goal_stride, double* d_xu_out, i7m_problem_stats* d_stats) {
  int rc = open_batch(h, B, goal_stride, d_xu_in && d_xcur && d_goals && d_xu_out, "null device pointer");
  if (rc || B == 0) return rc;
  ProblemStats* st = d_stats ? reinterpret_cast<ProblemStats*>(d_stats) : h->d_stats;
  return run_ranges(h, B, [&](long lo, int n, hipStream_t s, StaggerMark* mark) {
    // the whole batch on the handle's stream goes through the graph cache
    if (s == h->stream) return run_sqp_graphed(h, B, d_xu_in, d_xu_out, d_xcur, d_goals, goal_stride, st);
    return run_sqp(h, n, d_xu_in + lo * h->T, d_xu_out + lo * h->T, d_xcur + lo * 12, d_goals + lo * h->N * goal_stride,
                   goal_stride, st + lo, lo, s, mark);
  });
}

int i7m_solve(i7m_handle* h, int32_t B, const double* xu_in, const double* xcur, const double* goals,
              int32_t goal_stride, double* xu_out, i7m_problem_stats* stats) {
  int rc = open_batch(h, B, goal_stride, xu_in && xcur && goals && xu_out);
  if (rc || B == 0) return rc;
  const int nch = h2h_chunks_for(h->tune, h->cfg.qp_mode, B);
  if (nch > 1) return solve_h2h_chunked(h, B, xu_in, xcur, goals, goal_stride, xu_out, stats, nch);
  if ((rc = stage_in(h, 0, B, xu_in, xcur, goals, goal_stride))) return rc;
  if ((rc = run_sqp_graphed(h, B, h->d_xu, h->d_xu, h->d_xs, h->d_goal, goal_stride, h->d_stats))) return rc;
  if ((rc = stage_out(h, 0, B, xu_out, stats))) return rc;
  return i7m_synchronize(h);
}

int i7m_qp(i7m_handle* h, int32_t B, const double* xu, const double* xcur, const double* goals, int32_t goal_stride,
           double* sol) {
  int rc = open_batch(h, B, goal_stride, xu && xcur && goals && sol);
  if (rc || B == 0) return rc;
  const SolveParams P = params_of(h, B, goal_stride);
  const Bufs W = bufs_at(h, 0);
  if ((rc = stage_in(h, 0, B, xu, xcur, goals, goal_stride))) return rc;
  if ((rc = launch_linearize(h, h->stream, W, P, h->d_xu, h->d_goal, nullptr))) return rc;
  const double* qsol = nullptr;
  if ((rc = solve_qp(h, h->stream, W, P, h->d_xu, h->d_xs, nullptr, W.sol, &qsol))) return rc;
  if ((rc = copy_out(h, sol, qsol, (size_t)B * h->T))) return rc;
  return i7m_synchronize(h);
}

int i7m_qp_value(i7m_handle* h, int32_t B, const double* xu, const double* xcur, const double* goals, int32_t goal_stride,
                 double* V0) {
  int rc = open_batch(h, B, goal_stride, xu && xcur && goals && V0);
  if (rc || B == 0) return rc;
  if (h->cfg.qp_mode != I7M_QP_DIRECT) return fail(I7M_EINVAL, "i7m_qp_value: the equality-constrained QP only");
  // (B x 169 doubles in the solution buffer: T = 18 N - 6 >= 169 from N = 10) — a precondition,
  // checked before any copy or launch
  if (h->T < 169) return fail(I7M_EINVAL, "i7m_qp_value needs N >= 10");
  const SolveParams P = params_of(h, B, goal_stride);
  const Bufs W = bufs_at(h, 0);
  if ((rc = stage_in(h, 0, B, xu, xcur, goals, goal_stride))) return rc;
  if ((rc = launch_linearize(h, h->stream, W, P, h->d_xu, h->d_goal, nullptr))) return rc;
  double* vbuf = W.sol;
  if ((rc = launch_riccati(h, h->stream, W, P, h->d_xu, h->d_xs, nullptr, W.sol, vbuf))) return rc;
  if ((rc = copy_out(h, V0, vbuf, (size_t)B * 169))) return rc;
  return i7m_synchronize(h);
}

int i7m_qp_policy(i7m_handle* h, int32_t B, const double* xu, const double* xcur, const double* goals, int32_t goal_stride,
                  int32_t n_k, double* K_out, double* sol_out) {
  const std::string who = "i7m_qp_policy";
  int rc = check_batch(h, B, goal_stride);
  if (rc) return rc;
  // the box mode's corrector steps overwrite kbuf's feedforward column (riccati_mfma_body, kff_only)
  if (h->cfg.qp_mode == I7M_QP_BOX) return fail(I7M_EINVAL, who + ": I7M_QP_BOX is not supported (I7M_QP_DIRECT or I7M_QP_ADMM)");
  const int N = (int)h->N;
  if (n_k < 1 || n_k > N - 1)
    return fail(I7M_EINVAL, who + ": n_k = " + std::to_string(n_k) + " outside [1, N - 1 = " + std::to_string(N - 1) + "]");
  if (!K_out) return fail(I7M_EINVAL, who + ": null K_out");
  if (B == 0) return I7M_OK;
  if (!xu) return fail(I7M_EINVAL, who + ": null xu");
  if (!xcur) return fail(I7M_EINVAL, who + ": null xcur");
  if (!goals) return fail(I7M_EINVAL, who + ": null goals");
  HIPCHK(hipSetDevice(h->dev));
  const SolveParams P = params_of(h, B, goal_stride);
  const Bufs W = bufs_at(h, 0);
  if ((rc = stage_in(h, 0, B, xu, xcur, goals, goal_stride))) return rc;
  if ((rc = policy_pass(h, h->stream, W, P, h->d_xu, h->d_xs, h->d_goal))) return rc;
  // gathered into the linearisation's rows, dead once the sweep and rollout have run:
  // B n_k 78 <= max_batch (N - 1) LIN_STRIDE doubles
  double* kout = W.lin;
  HIPCHK(i7m_launch_policy_gather(B, N, n_k, h->stream, W.kbuf, kout));
  if ((rc = copy_out(h, K_out, kout, (size_t)B * n_k * POLICY_K))) return rc;
  if (sol_out && (rc = copy_out(h, sol_out, W.sol, (size_t)B * h->T))) return rc;
  return i7m_synchronize(h);
}

int i7m_get_box_stats(i7m_handle* h, int32_t B, int32_t* iters, int32_t* converged, double* mu) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (h->cfg.qp_mode != I7M_QP_BOX) return fail(I7M_EINVAL, "handle is not in I7M_QP_BOX mode");
  if (B < 0 || B > h->cfg.max_batch) return fail(I7M_EINVAL, "batch outside [0, max_batch]");
  HIPCHK(hipSetDevice(h->dev));
  std::vector<IpmState> st((size_t)B);
  if (B) HIPCHK(hipMemcpyAsync(st.data(), h->d_bst, sizeof(IpmState) * (size_t)B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int b = 0; b < B; ++b) {
    if (iters) iters[b] = st[b].iters;
    if (converged) converged[b] = st[b].converged;
    if (mu) mu[b] = st[b].mu;
  }
  return I7M_OK;
}

int i7m_linearize(i7m_handle* h, int32_t B, const double* xu, const double* goals, int32_t goal_stride, double* lin,
                  double* cost) {
  int rc = open_batch(h, B, goal_stride, xu && goals);
  if (rc || B == 0) return rc;
  const size_t N = h->N;
  const SolveParams P = params_of(h, B, goal_stride);
  if ((rc = stage_in(h, 0, B, xu, nullptr, goals, goal_stride))) return rc;
  if ((rc = launch_linearize(h, h->stream, bufs_at(h, 0), P, h->d_xu, h->d_goal, nullptr))) return rc;
  if (lin && (rc = copy_out(h, lin, h->d_lin, (size_t)B * (N - 1) * LIN_STRIDE))) return rc;
  if (cost && (rc = copy_out(h, cost, h->d_cost, (size_t)B * N * COST_STRIDE))) return rc;
  return i7m_synchronize(h);
}

int i7m_merit(i7m_handle* h, int32_t B, const double* xu, const double* xu_ref, const double* goals,
              int32_t goal_stride, double* out) {
  int rc = open_batch(h, B, goal_stride, xu && xu_ref && goals && out);
  if (rc || B == 0) return rc;
  const SolveParams P = params_of(h, B, goal_stride);
  if ((rc = stage_in(h, 0, B, xu, nullptr, goals, goal_stride))) return rc;
  if ((rc = copy_in(h, h->d_aux, xu_ref, (size_t)B * h->T))) return rc;
  hipLaunchKernelGGL(k_merit, dim3(B), dim3(64), 0, h->stream, h->d_model, P, h->d_xu, h->d_aux, h->d_goal,
                     h->has_fext ? h->d_fext : nullptr, (int)(h->fext_frame == I7M_WRENCH_WORLD), h->d_out);
  HIPCHK(hipGetLastError());
  if ((rc = copy_out(h, out, h->d_out, (size_t)B * 5))) return rc;
  return i7m_synchronize(h);
}

int i7m_linesearch(i7m_handle* h, int32_t B, const double* xu, const double* xu_full, const double* goals,
                   int32_t goal_stride, double* alpha) {
  int rc = open_batch(h, B, goal_stride, xu && xu_full && goals && alpha);
  if (rc || B == 0) return rc;
  const SolveParams P = params_of(h, B, goal_stride);
  if ((rc = stage_in(h, 0, B, xu, nullptr, goals, goal_stride))) return rc;
  if ((rc = copy_in(h, h->d_sol, xu_full, (size_t)B * h->T))) return rc;
  if ((rc = launch_linesearch(h, h->stream, bufs_at(h, 0), P, h->d_xu, h->d_xu, h->d_sol, h->d_goal, nullptr, h->d_stats,
                              h->d_out, 0, 1, false)))
    return rc;
  if ((rc = copy_out(h, alpha, h->d_out, (size_t)B))) return rc;
  return i7m_synchronize(h);
}

// ---- query hooks: chunk through the scratch buffers (query_chunks), <= 36 doubles per query and
// buffer, 114 for the derivatives' outputs ---------------------------------------------------------
int i7m_eepos(i7m_handle* h, int32_t Bq, const double* q, double* p_out, double* J_out) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (Bq < 0 || !q || !p_out) return fail(I7M_EINVAL, "bad arguments");
  return query_chunks(h, Bq, 36, {{q, 6}}, {{p_out, 3}, {J_out, 18, h->d_out}}, [&](int n, double** in, double** out) {
    hipLaunchKernelGGL(k_eepos, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_model, n, in[0], out[0],
                       J_out ? out[1] : nullptr);
  });
}

int i7m_aba(i7m_handle* h, int32_t Bq, const double* q, const double* v, const double* tau, const double* fext,
            int32_t frame, double* a_out) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (Bq < 0 || !q || !v || !tau || !a_out) return fail(I7M_EINVAL, "bad arguments");
  const auto launch = [&](int n, double** in, double** out) {
    hipLaunchKernelGGL(k_aba, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_model, n, in[0], in[1], in[2],
                       fext ? in[3] : nullptr, (int)(frame == I7M_WRENCH_WORLD), out[0]);
  };
  return query_chunks(h, Bq, 36, {{q, 6}, {v, 6}, {tau, 6}, {fext, 6}}, {{a_out, 6}}, launch);
}

int i7m_aba_derivatives(i7m_handle* h, int32_t Bq, const double* q, const double* v, const double* tau, double* dq_out,
                        double* dv_out, double* Minv_out, double* a_out) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (Bq < 0 || !q || !v || !tau || !dq_out || !dv_out || !Minv_out || !a_out)
    return fail(I7M_EINVAL, "bad arguments");
  const auto launch = [&](int n, double** in, double** out) {
    const long nthr = 12L * n;
    hipLaunchKernelGGL(k_abad, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, h->stream, h->d_model, n, in[0], in[1],
                       in[2], out[0], out[1], out[2], out[3]);
  };
  // the outputs need 3*36+6 doubles per query
  return query_chunks(h, Bq, 114, {{q, 6}, {v, 6}, {tau, 6}}, {{dq_out, 36}, {dv_out, 36}, {Minv_out, 36}, {a_out, 6}},
                      launch);
}

int i7m_rk4(i7m_handle* h, int32_t Bq, const double* q, const double* v, const double* u, double dt,
            const double* fext, int32_t frame, double* q_out, double* v_out) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (Bq < 0 || !q || !v || !u || !q_out || !v_out) return fail(I7M_EINVAL, "bad arguments");
  const auto launch = [&](int n, double** in, double** out) {
    hipLaunchKernelGGL(k_rk4, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_model, n, in[0], in[1], in[2], dt,
                       fext ? in[3] : nullptr, (int)(frame == I7M_WRENCH_WORLD), out[0], out[1]);
  };
  return query_chunks(h, Bq, 36, {{q, 6}, {v, 6}, {u, 6}, {fext, 6}}, {{q_out, 6}, {v_out, 6}}, launch);
}

int i7m_mpc_run(i7m_handle* h, int32_t B, const double* xstart, const double* endpoints, int32_t n_endpoints,
                int32_t num_steps, double* dist_out, double* q_out, double* xcur_out, double* xu_out) {
  int rc = check_batch(h, B, 3);
  if (rc) return rc;
  if (n_endpoints < 1 || num_steps < 0 || !endpoints || !xstart || !dist_out)
    return fail(I7M_EINVAL, "mpc_run: need xstart, >= 1 endpoint, num_steps >= 0, dist_out");
  // MPC_OSQP has no external wrench (src/osqp_mpc.py:56 calls rk4 without f_ext): with one set
  // on the handle the planner (run_sqp) would use it and the plant (k_mpc_advance) would not
  if (h->has_fext)
    return fail(I7M_EINVAL, "mpc_run: the handle has an external wrench set; MPC_OSQP's closed loop has none "
                            "(clear it with i7m_set_external_wrench(h, 0, NULL, 0))");
  if (B == 0) return I7M_OK;
  HIPCHK(hipSetDevice(h->dev));
  const int N = (int)h->N;
  const size_t T = h->T;
  // per-run state beyond the handle's buffers (this is a whole closed-loop run, not the solve
  // hot path): endpoints, goal index, alive flag, the distance and q histories
  size_t bytes[MPC_WS_COUNT];
  mpc_ws_bytes(B, n_endpoints, num_steps, bytes);
  const LoopStart start(h, B, B, endpoints);  // (declared first: destroyed after the workspace's synchronize)
  Workspace ws(h, bytes);
  if (!ws.base) return fail(I7M_ENOMEM, "mpc_run: device allocation failed");
  double *d_ep = ws.at<double>(MPC_WS_EP), *d_dist = ws.at<double>(MPC_WS_DIST), *d_q = ws.at<double>(MPC_WS_Q);
  int *d_gi = ws.at<int>(MPC_WS_GI), *d_alive = ws.at<int>(MPC_WS_ALIVE);
  // src/osqp_mpc.py:14-27: goal = endpoint 0 tiled, XU = 0, XU = sqp(xcur, goal, XU)
  if ((rc = copy_in(h, h->d_xs, xstart, (size_t)B * 12))) return rc;
  if ((rc = loop_start(h, start, endpoints, n_endpoints, d_ep, d_gi, d_alive))) return rc;
  // the instances [lo, lo + n) through every MPC step on stream s (the whole batch on the
  // handle's stream, or, where the solve staggers, each range on its own: the instances are
  // independent, so a range runs its steps without waiting for the other; its first solve
  // records the staggered ranges' mark)
  rc = run_ranges(h, B, [&](long lo, int n, hipStream_t s, StaggerMark* mark) -> int {
    double *xu = h->d_xu + lo * T, *out = h->d_out + lo * T, *xs = h->d_xs + lo * 12, *g = h->d_goal + lo * 3 * N;
    int rc3;
    if ((rc3 = run_sqp(h, n, xu, xu, xs, g, 3, nullptr, lo, s, mark))) return rc3;
    for (int i = 0; i < num_steps; ++i) {
      hipLaunchKernelGGL(k_mpc_goal, dim3((n + 255) / 256), dim3(256), 0, s, h->d_model, n, N, xs, g, d_ep, n_endpoints,
                         d_gi + lo, d_alive + lo, d_dist + (size_t)i * B + lo);
      HIPCHK(hipGetLastError());
      // xu_new = sqp(xcur, goal, XU) into the scratch buffer d_out (XU itself is read only)
      if ((rc3 = run_sqp(h, n, xu, out, xs, g, 3, nullptr, lo, s))) return rc3;
      hipLaunchKernelGGL(k_mpc_advance, dim3(n), dim3(64), 0, s, h->d_model, n, N, h->cfg.dt, xs, xu, out, d_alive + lo,
                         d_q + ((size_t)i * B + lo) * 6);
      HIPCHK(hipGetLastError());
    }
    return I7M_OK;
  });
  if (rc) return rc;
  if (num_steps > 0) {
    if ((rc = copy_out(h, dist_out, d_dist, (size_t)num_steps * B))) return rc;
    if (q_out && (rc = copy_out(h, q_out, d_q, (size_t)num_steps * B * 6))) return rc;
  }
  if (xcur_out && (rc = copy_out(h, xcur_out, h->d_xs, (size_t)B * 12))) return rc;
  if (xu_out && (rc = copy_out(h, xu_out, h->d_xu, (size_t)B * T))) return rc;
  return i7m_synchronize(h);
}

int i7m_multirate_opts_default(i7m_multirate_opts* o) {
  if (!o) return fail(I7M_EINVAL, "null opts");
  o->sim_dt = 0.001;      // MPC_GATO_Batch.run_mpc's default, src/gato_mpc_batch.py:76
  o->goal_radius = 0.1;   // :158
  o->control_from = I7M_CONTROL_NEW;    // :185
  o->reset_what = I7M_ADMM_RESET_ALL;  // solver.reset() before every solve, :116
  return I7M_OK;
}

int i7m_multirate_substeps(double dt, double sim_dt, int32_t N, int32_t num_steps, int32_t* n_sub) {
  const std::string who = "multirate_substeps";
  if (!n_sub) return fail(I7M_EINVAL, who + ": null n_sub");
  if (num_steps < 0) return fail(I7M_EINVAL, who + ": num_steps = " + std::to_string(num_steps) + ", need num_steps >= 0");
  MultirateSchedule sch;
  const char* which = "";
  long at = 0;
  if (!multirate_schedule(dt, sim_dt, N, num_steps, &sch, &which, &at))
    return fail(I7M_EINVAL, multirate_refusal(who, which, at, sim_dt, N));
  *n_sub = sch.total();
  return I7M_OK;
}

int i7m_multirate_knots(double dt, double sim_dt, int32_t N, int32_t num_steps, int32_t control_from, int32_t* knot_out) {
  const std::string who = "multirate_knots";
  if (num_steps < 0) return fail(I7M_EINVAL, who + ": num_steps = " + std::to_string(num_steps) + ", need num_steps >= 0");
  if (control_from != I7M_CONTROL_NEW && control_from != I7M_CONTROL_PREV && control_from != I7M_CONTROL_POLICY)
    return fail(I7M_EINVAL, who + ": control_from must be I7M_CONTROL_NEW, I7M_CONTROL_PREV or I7M_CONTROL_POLICY");
  MultirateSchedule sch;
  const char* which = "";
  long at = 0;
  if (!multirate_schedule(dt, sim_dt, N, num_steps, &sch, &which, &at))
    return fail(I7M_EINVAL, multirate_refusal(who, which, at, sim_dt, N));
  if (control_from == I7M_CONTROL_POLICY && (at = multirate_policy_bad_step(sch, N)) >= 0)
    return fail(I7M_EINVAL, multirate_policy_refusal(who, at, sim_dt, N));
  if (knot_out) std::copy(sch.sub_knot.begin(), sch.sub_knot.end(), knot_out);
  return I7M_OK;
}

int i7m_mpc_run_multirate(i7m_handle* h, int32_t B, const double* xstart, const double* endpoints, int32_t n_endpoints,
                          int32_t num_steps, const i7m_multirate_opts* opts, double* dist_out, double* q_out,
                          double* u_out, double* xpath_out, double* xcur_out, double* xu_out) {
  const std::string who = "mpc_run_multirate";
  int rc = check_batch(h, B, 3);
  if (rc) return rc;
  i7m_multirate_opts o;
  (void)i7m_multirate_opts_default(&o);
  if (opts) o = *opts;
  if (h->cfg.qp_mode != I7M_QP_DIRECT && h->cfg.qp_mode != I7M_QP_ADMM)
    return fail(I7M_EINVAL, who + ": I7M_QP_BOX is not supported (I7M_QP_DIRECT or I7M_QP_ADMM)");
  if (n_endpoints < 1) return fail(I7M_EINVAL, who + ": n_endpoints = " + std::to_string(n_endpoints) + ", need >= 1 endpoint");
  if (num_steps < 0) return fail(I7M_EINVAL, who + ": num_steps = " + std::to_string(num_steps) + ", need num_steps >= 0");
  if (o.control_from != I7M_CONTROL_NEW && o.control_from != I7M_CONTROL_PREV && o.control_from != I7M_CONTROL_POLICY)
    return fail(I7M_EINVAL, who + ": control_from must be I7M_CONTROL_NEW, I7M_CONTROL_PREV or I7M_CONTROL_POLICY");
  if (o.reset_what & ~I7M_ADMM_RESET_ALL) return fail(I7M_EINVAL, who + ": reset_what has unknown I7M_ADMM_RESET_* bits");
  if (!std::isfinite(o.goal_radius)) return fail(I7M_EINVAL, who + ": goal_radius must be finite");
  if (!xstart) return fail(I7M_EINVAL, who + ": null xstart");
  if (!endpoints) return fail(I7M_EINVAL, who + ": null endpoints");
  if (!dist_out) return fail(I7M_EINVAL, who + ": null dist_out");
  // neither driver's plant has an external wrench (src/gato_mpc_batch.py:188, src/gato_mpc.py:129
  // call rk4 without f_ext): with one set the planner would use it and the plant would not
  if (h->has_fext)
    return fail(I7M_EINVAL, who + ": the handle has an external wrench set; the multi-rate closed loops have none "
                                  "(clear it with i7m_set_external_wrench(h, 0, NULL, 0))");
  const int N = (int)h->N;
  MultirateSchedule sch;
  const char* which = "";
  long at = 0;
  if (!multirate_schedule(h->cfg.dt, o.sim_dt, N, num_steps, &sch, &which, &at))
    return fail(I7M_EINVAL, multirate_refusal(who, which, at, o.sim_dt, N));
  const bool policy = o.control_from == I7M_CONTROL_POLICY;
  if (policy && (at = multirate_policy_bad_step(sch, N)) >= 0)
    return fail(I7M_EINVAL, multirate_policy_refusal(who, at, o.sim_dt, N));
  if (B == 0) return I7M_OK;
  HIPCHK(hipSetDevice(h->dev));
  const size_t T = h->T;
  const int n_sub = sch.total();
  size_t bytes[MULTIRATE_WS_COUNT];
  multirate_ws_bytes(B, n_endpoints, num_steps, n_sub, bytes);
  // host staging, declared first: alive until the workspace's final synchronize
  const LoopStart start(h, B, B, endpoints);
  const std::vector<double> rho0((size_t)B, h->cfg.admm_rho);
  Workspace ws(h, bytes);
  if (!ws.base) return fail(I7M_ENOMEM, who + ": device allocation failed");
  double *d_ep = ws.at<double>(MRWS_EP), *d_dist = ws.at<double>(MRWS_DIST), *d_q = ws.at<double>(MRWS_Q),
         *d_u = ws.at<double>(MRWS_U), *d_xp = ws.at<double>(MRWS_XPATH), *d_sub = ws.at<double>(MRWS_SUBDT),
         *d_rho0 = ws.at<double>(MRWS_RHO0);
  int *d_gi = ws.at<int>(MRWS_GI), *d_alive = ws.at<int>(MRWS_ALIVE);
  // src/gato_mpc_batch.py:84-100: goal = endpoint 0 tiled, XU = [xstart, 0...], XU = sqp(xcur, goal, XU)
  if ((rc = copy_in(h, h->d_xs, xstart, (size_t)B * 12))) return rc;
  if ((rc = loop_start(h, start, endpoints, n_endpoints, d_ep, d_gi, d_alive))) return rc;
  HIPCHK(hipMemcpy2DAsync(h->d_xu, T * 8, xstart, 12 * 8, 12 * 8, B, hipMemcpyHostToDevice, h->stream));
  if ((rc = copy_in(h, d_rho0, rho0.data(), (size_t)B))) return rc;
  if (n_sub > 0 && (rc = copy_in(h, d_sub, sch.sub_dt.data(), (size_t)n_sub))) return rc;
  // the instances [lo, lo + n) through every MPC step on stream s, as i7m_mpc_run's ranges
  rc = run_ranges(h, B, [&](long lo, int n, hipStream_t s, StaggerMark* mark) -> int {
    double *xu = h->d_xu + lo * T, *out = h->d_out + lo * T, *xs = h->d_xs + lo * 12, *g = h->d_goal + lo * 3 * N;
    MultirateArgs a{};
    a.N = N;
    a.n_endpoints = n_endpoints;
    a.control_prev = o.control_from == I7M_CONTROL_PREV;
    a.hist_stride = B;
    a.radius = o.goal_radius;
    a.xs = xs;
    a.XU = xu;
    a.xu_new = out;
    a.goals = g;
    a.endpoints = d_ep;
    a.goal_idx = d_gi + lo;
    a.alive = d_alive + lo;
    int rc3;
    if ((rc3 = loop_reset(h, lo, n, I7M_ADMM_RESET_ALL, s, d_rho0))) return rc3;
    if ((rc3 = run_sqp(h, n, xu, xu, xs, g, 3, nullptr, lo, s, mark))) return rc3;
    for (int i = 0; i < num_steps; ++i) {
      if ((rc3 = loop_reset(h, lo, n, o.reset_what, s, d_rho0))) return rc3;
      // xu_new = sqp(xcur, goal, XU) into the scratch buffer d_out (XU itself is read only)
      if ((rc3 = run_sqp(h, n, xu, out, xs, g, 3, nullptr, lo, s))) return rc3;
      a.n_sub = sch.sub_start[i + 1] - sch.sub_start[i];
      a.shift = sch.shift[i];
      a.sub_dt = d_sub + sch.sub_start[i];
      a.dist_out = d_dist + (size_t)i * B + lo;
      a.q_out = d_q + ((size_t)i * B + lo) * 6;
      a.u_out = d_u + ((size_t)i * B + lo) * 6;
      a.xpath_out = d_xp + ((size_t)sch.sub_start[i] * B + lo) * 6;
      if (policy) {
        // the gains of this step's solve: the QP at xu_new with x_0 = xcur, on this range's rows and
        // stream behind its solve (in I7M_QP_ADMM the exact QP's, which OSQP's iterate approximates)
        const Bufs W = bufs_at(h, lo);
        if ((rc3 = policy_pass(h, s, W, params_of(h, n, 3), out, xs, g))) return rc3;
        if (h->policy_zero_k) HIPCHK(hipMemsetAsync(W.kbuf, 0, (size_t)n * (N - 1) * KBUF_STRIDE * 8, s));
        PolicyKnots kn{};
        for (int e = 0; e < a.n_sub; ++e) kn.j[e] = (unsigned char)sch.sub_knot[sch.sub_start[i] + e];
        HIPCHK(i7m_launch_multirate_policy_step(n, s, h->d_model, &a, &kn, W.kbuf));
        continue;
      }
      HIPCHK(i7m_launch_multirate_step(n, s, h->d_model, &a));
    }
    return I7M_OK;
  });
  if (rc) return rc;
  if (num_steps > 0) {
    if ((rc = copy_out(h, dist_out, d_dist, (size_t)num_steps * B))) return rc;
    if (q_out && (rc = copy_out(h, q_out, d_q, (size_t)num_steps * B * 6))) return rc;
    if (u_out && (rc = copy_out(h, u_out, d_u, (size_t)num_steps * B * 6))) return rc;
    if (xpath_out && (rc = copy_out(h, xpath_out, d_xp, (size_t)n_sub * B * 6))) return rc;
  }
  if (xcur_out && (rc = copy_out(h, xcur_out, h->d_xs, (size_t)B * 12))) return rc;
  if (xu_out && (rc = copy_out(h, xu_out, h->d_xu, (size_t)B * T))) return rc;
  return i7m_synchronize(h);
}

int i7m_sampled_opts_default(i7m_sampled_opts* o) {
  if (!o) return fail(I7M_EINVAL, "null opts");
  o->sim_dt = 0.001;  // run_mpc's default, src/gato_mpc_batch_sample.py:106
  o->decay = 1.0;
  o->frame = I7M_WRENCH_WORLD;
  o->reset_what = I7M_ADMM_RESET_ALL;  // reset() + resetRho() before every solve, :222-223
  o->keep_best = 0;
  o->n_actual = 1;
  return I7M_OK;
}

}  // extern "C"

namespace {

// The description of a call of the sampled-wrench family on this handle (i7m_plan.h).  opts: the
// options every kind shares (null: the defaults); shift_warm_start: the multi-rate kinds' flag.
SampledCall describe_call(const i7m_handle* h, SampledKind kind, int G, int H, int num_steps, const i7m_sampled_opts* opts,
                          int shift_warm_start, const GoalSource& goal, const double* xstart, const double* fhyp,
                          const double* f_actual, const double* hist_out, int control_from = I7M_CONTROL_NEW) {
  SampledCall c;
  c.kind = kind;
  c.qp_mode = h->cfg.qp_mode;
  c.max_batch = h->cfg.max_batch;
  c.dt = h->cfg.dt;
  c.G = G;
  c.H = H;
  c.num_steps = num_steps;
  (void)i7m_sampled_opts_default(&c.o);
  if (opts) c.o = *opts;
  c.shift_warm_start = shift_warm_start;
  c.control_from = control_from;
  c.goal = goal;
  c.xstart = xstart;
  c.fhyp = fhyp;
  c.f_actual = f_actual;
  c.hist_out = hist_out;
  return c;
}
// The family's one argument check, before the device is touched and before any handle state
// changes: sampled_call_ok, or for a multi-rate kind sampled_multirate_call_ok, which also leaves
// the plant's schedule for the handle's horizon in *sch (untouched for the other kinds).
int check_call(const std::string& who, const SampledCall& c, int N, MultirateSchedule* sch) {
  const char* which = "";
  long at = 0;
  if (multirate_kind(c.kind)) {
    if (sampled_multirate_call_ok(c, N, sch, &which, &at)) return I7M_OK;
    return fail(I7M_EINVAL, sampled_multirate_refusal(who, which, at, c, N));
  }
  if (sampled_call_ok(c, &which, &at)) return I7M_OK;
  return fail(I7M_EINVAL, sampled_refusal(who, which, at, c.max_batch));
}

// Where a loop of the family leaves its results (host, each but hist may be null): the histories
// per step (hist: dist_out / err_out; ee: the tracking kinds'; u, xpath, off: the multi-rate kinds')
// and the final state.
struct SampledOut {
  double* hist = nullptr;
  int32_t* best = nullptr;
  double *q = nullptr, *u = nullptr, *xpath = nullptr, *ee = nullptr;
  int32_t* off = nullptr;
  double *fbest = nullptr, *xcur = nullptr, *xu_best = nullptr, *fhyp = nullptr;
};

// The sampled-wrench closed loop of the family's four entry points (`who` names the one in the
// messages).  A multi-rate kind owns the plant's schedule and the tracking window's offsets derived
// from it (the knots completed so far), splits the plant at knot boundaries
// (k_sampled_multirate_step) and records u and the path; a single-rate kind has neither, reads the
// caller's ref_offset and launches k_sampled_step.
int sampled_loop(i7m_handle* h, const std::string& who, const SampledCall& c, const double* noise, const SampledOut& out) {
  if (h->ctrl.open) return session_open();
  const int N = (int)h->N;
  const bool multi = multirate_kind(c.kind), track = tracking_kind(c.kind);
  const bool policy = multi && c.control_from == I7M_CONTROL_POLICY;
  MultirateSchedule sch;
  int rc;
  if ((rc = check_call(who, c, N, &sch))) return rc;
  const int G = c.G, H = c.H, num_steps = c.num_steps;
  const i7m_sampled_opts& o = c.o;
  const GoalSource& gs = c.goal;
  const std::vector<int32_t> sch_offs = multirate_offsets(sch);
  const int32_t* offs = multi ? sch_offs.data() : gs.ref_offset;
  if (multi && track && out.off)
    for (int i = 0; i < num_steps; ++i) out.off[i] = offs[i];
  if (G == 0) return I7M_OK;
  HIPCHK(hipSetDevice(h->dev));
  const int B = G * H, n_sub = sch.total();
  const size_t T = h->T;
  // per-run state beyond the handle's buffers: per group the state, XU_best, the scored
  // hypothesis, goal index and alive flag; the schedules and the histories; the tracking kinds'
  // reference, phases and EE history; the multi-rate kinds' controls, path and sub-step lengths
  size_t bytes[SAMPLED_MULTIRATE_WS_COUNT];
  sampled_call_ws_bytes(c, N, n_sub, noise != nullptr, bytes);
  // host staging, declared first: alive until the workspace's final synchronize
  const GroupStart start(h, G, H, c.xstart, gs);
  Workspace ws(h, bytes);
  if (!ws.base) return fail(I7M_ENOMEM, who + ": device allocation failed");
  double *d_ep = ws.at<double>(SWS_EP), *d_xcur = ws.at<double>(SWS_XCUR), *d_xub = ws.at<double>(SWS_XUB),
         *d_fact = ws.at<double>(SWS_FACT), *d_noise = bytes[SWS_NOISE] ? ws.at<double>(SWS_NOISE) : nullptr,
         *d_dist = ws.at<double>(SWS_DIST), *d_q = ws.at<double>(SWS_Q), *d_fb = ws.at<double>(SWS_FB),
         *d_rho0 = ws.at<double>(SWS_RHO0), *d_ref = track ? ws.at<double>(TWS_REF) : nullptr,
         *d_ee = track ? ws.at<double>(TWS_EE) : nullptr, *d_u = ws.at<double>(SMWS_U),
         *d_xp = ws.at<double>(SMWS_XPATH), *d_sub = ws.at<double>(SMWS_SUBDT);
  int *d_best = ws.at<int>(SWS_BEST), *d_gi = ws.at<int>(SWS_GI), *d_alive = ws.at<int>(SWS_ALIVE),
      *d_bh = ws.at<int>(SWS_BH), *d_phase = bytes[TWS_PHASE] ? ws.at<int>(TWS_PHASE) : nullptr;
  const size_t hist = history_rows(num_steps, G);
  // src/gato_mpc_batch_sample.py:111-128: goal = endpoint 0 tiled (tracking: the window at offset
  // 0), XU = [xstart, 0...], every row of a group at the group's start state, the hypotheses set
  // on the solver; the multi-rate plant's sub-step lengths
  if ((rc = stage_start(h, start, gs, G, d_rho0, d_ref, d_phase))) return rc;
  if ((rc = loop_instances(h, start.rows, gs.endpoints, gs.n_endpoints, d_ep, d_gi, d_alive))) return rc;
  if ((rc = copy_in(h, d_xcur, c.xstart, (size_t)G * 12))) return rc;
  if ((rc = copy_in(h, d_fact, c.f_actual, 6 * (size_t)o.n_actual * G))) return rc;
  if (d_noise && (rc = copy_in(h, d_noise, noise, 3 * (size_t)num_steps * B))) return rc;
  if (n_sub > 0 && (rc = copy_in(h, d_sub, sch.sub_dt.data(), (size_t)n_sub))) return rc;
  HIPCHK(hipMemsetAsync(d_best, 0, 4 * (size_t)G, h->stream));  // the initial solve's XU_best is row 0, :128
  if ((rc = install_wrench(h, B, c.fhyp, o.frame))) return rc;
  // the rows [lo, lo + n) (whole groups) through every MPC step on stream s, as i7m_mpc_run's
  // ranges: the groups are independent, so a staggered range runs its steps on its own
  rc = run_ranges(h, B, [&](long lo, int n, hipStream_t s, StaggerMark* mark) -> int {
    const long glo = lo / H;
    const int ng = n / H;
    double *xu = h->d_xu + lo * T, *xu_new = h->d_out + lo * T, *xs = h->d_xs + lo * 12, *g = h->d_goal + lo * 3 * N;
    SampledMultirateArgs m{};  // (a single-rate kind launches with m.S alone)
    SampledArgs& a = m.S;
    a.N = N;
    a.H = H;
    a.n_endpoints = gs.n_endpoints;
    a.frame_world = o.frame == I7M_WRENCH_WORLD;
    a.keep_best = o.keep_best != 0;
    a.sim_dt = o.sim_dt;
    a.decay = o.decay;
    a.xs = xs;
    a.XU = xu;
    a.xu_new = xu_new;
    a.goals = g;
    a.fext = h->d_fext + lo * 6;
    a.xcur = d_xcur + glo * 12;
    a.xub = d_xub + glo * T;
    a.best = d_best + glo;
    a.goal_idx = d_gi + glo;
    a.alive = d_alive + glo;
    a.endpoints = track ? nullptr : d_ep;
    a.ref = d_ref;
    a.ref_phase = d_phase ? d_phase + glo : nullptr;
    a.L = (int)gs.L;
    a.ref_stride = gs.ref_stride;
    m.hist_stride = G;
    int rc3;
    // I7M_CONTROL_POLICY: the gains of the solve just run, the QP at xu_new with x_0 = xs, on this
    // range's rows and stream behind that solve and before the step launch: the rows' wrenches are
    // still the ones the solve used (the select step resamples them afterwards), so row `best`'s
    // slots of kbuf are the winner's policy
    const Bufs W = bufs_at(h, lo);
    const auto gains = [&]() -> int {
      if (!policy) return I7M_OK;
      const int r = policy_pass(h, s, W, params_of(h, n, 3), xu_new, xs, g);
      if (r) return r;
      if (h->policy_zero_k) HIPCHK(hipMemsetAsync(W.kbuf, 0, (size_t)n * (N - 1) * KBUF_STRIDE * 8, s));
      return I7M_OK;
    };
    if ((rc3 = loop_reset(h, lo, n, I7M_ADMM_RESET_ALL, s, d_rho0))) return rc3;
    if ((rc3 = run_sqp(h, n, xu, xu_new, xs, g, 3, nullptr, lo, s, mark))) return rc3;
    if ((rc3 = gains())) return rc3;
    // launch i: select(i - 1) (i = 0: the initial solve's row 0), then plant(i) ... goal(i);
    // the last launch only selects
    for (int i = 0; i <= num_steps; ++i) {
      a.select = i == 0 ? 2 : 1;
      a.plant = i < num_steps;
      const size_t rec = ((size_t)std::max(i - 1, 0)) * G + glo, cur = (size_t)std::min(i, std::max(num_steps - 1, 0)) * G + glo;
      a.noise = d_noise && i > 0 ? d_noise + ((size_t)(i - 1) * B + lo) * 3 : nullptr;
      a.best_out = d_bh + rec;
      a.fbest_out = d_fb + rec * 6;
      a.f_actual = d_fact + ((size_t)(o.n_actual > 1 ? std::min(i, o.n_actual - 1) : 0) * G + glo) * 6;
      a.dist_out = d_dist + cur;
      a.q_out = d_q + cur * 6;
      a.off = track && a.plant ? offs[i] : 0;
      a.ee_out = track ? d_ee + cur * 3 : nullptr;
      if (multi) {
        const int s0 = a.plant ? sch.sub_start[i] : 0;
        m.n_sub = a.plant ? sch.sub_start[i + 1] - s0 : 0;
        m.shift = a.plant && c.shift_warm_start ? sch.shift[i] : 0;
        m.sub_dt = d_sub + s0;
        m.u_out = d_u + cur * 6;
        m.xpath_out = d_xp + ((size_t)s0 * G + glo) * 6;
        if (policy) {
          PolicyKnots kn{};
          for (int e = 0; e < m.n_sub; ++e) kn.j[e] = (unsigned char)sch.sub_knot[s0 + e];
          HIPCHK(i7m_launch_sampled_multirate_policy_step(ng, H, s, h->d_model, &m, &kn, W.kbuf));
        } else {
          HIPCHK(i7m_launch_sampled_multirate_step(ng, H, s, h->d_model, &m));
        }
      } else {
        hipLaunchKernelGGL(k_sampled_step, dim3(ng), dim3((H + 63) / 64 * 64), 0, s, h->d_model, a);
        HIPCHK(hipGetLastError());
      }
      if (!a.plant) break;
      if ((rc3 = loop_reset(h, lo, n, o.reset_what, s, d_rho0))) return rc3;
      if ((rc3 = run_sqp(h, n, xu, xu_new, xs, g, 3, nullptr, lo, s))) return rc3;
      if ((rc3 = gains())) return rc3;
    }
    return I7M_OK;
  }, stagger_cut_grouped(B, H));
  if (rc) return rc;
  if (num_steps > 0) {
    if ((rc = copy_out(h, out.hist, d_dist, hist))) return rc;
    if (out.q && (rc = copy_out(h, out.q, d_q, hist * 6))) return rc;
    if (multi && out.u && (rc = copy_out(h, out.u, d_u, hist * 6))) return rc;
    if (multi && out.xpath && (rc = copy_out(h, out.xpath, d_xp, (size_t)n_sub * G * 6))) return rc;
    if (track && out.ee && (rc = copy_out(h, out.ee, d_ee, hist * 3))) return rc;
    if (out.fbest && (rc = copy_out(h, out.fbest, d_fb, hist * 6))) return rc;
    if (out.best) HIPCHK(hipMemcpyAsync(out.best, d_bh, 4 * hist, hipMemcpyDeviceToHost, h->stream));
  }
  if (out.xcur && (rc = copy_out(h, out.xcur, d_xcur, (size_t)G * 12))) return rc;
  if (out.xu_best && (rc = copy_out(h, out.xu_best, d_xub, (size_t)G * T))) return rc;
  if (out.fhyp && (rc = copy_out(h, out.fhyp, h->d_fext, (size_t)B * 6))) return rc;
  return i7m_synchronize(h);
}

// A multi-rate call's options as the family's shared ones and the shift flag (null: the defaults).
struct SharedOpts {
  i7m_sampled_opts o;
  int shift_warm_start = 0, control_from = I7M_CONTROL_NEW;
  explicit SharedOpts(const i7m_sampled_multirate_opts* m) {
    (void)i7m_sampled_opts_default(&o);
    if (!m) return;
    o = i7m_sampled_opts{m->sim_dt, m->decay, m->frame, m->reset_what, m->keep_best, m->n_actual};
    shift_warm_start = m->shift_warm_start;
    control_from = m->control_from;
  }
};

}  // namespace

extern "C" {

int i7m_mpc_run_sampled(i7m_handle* h, int32_t G, int32_t H, const double* xstart, const double* endpoints,
                        int32_t n_endpoints, int32_t num_steps, const double* fhyp, const double* f_actual,
                        const double* noise, const i7m_sampled_opts* opts, double* dist_out, int32_t* best_out,
                        double* q_out, double* fbest_out, double* xcur_out, double* xu_best_out, double* fhyp_out) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  const SampledCall c = describe_call(h, SampledKind::endpoints, G, H, num_steps, opts, 0,
                                      GoalSource::of_endpoints(endpoints, n_endpoints), xstart, fhyp, f_actual, dist_out);
  SampledOut out;
  out.hist = dist_out;
  out.best = best_out;
  out.q = q_out;
  out.fbest = fbest_out;
  out.xcur = xcur_out;
  out.xu_best = xu_best_out;
  out.fhyp = fhyp_out;
  return sampled_loop(h, "mpc_run_sampled", c, noise, out);
}

int i7m_mpc_run_tracking(i7m_handle* h, int32_t G, int32_t H, const double* xstart, const double* ref, int32_t L,
                         int32_t ref_stride, const int32_t* ref_phase, const int32_t* ref_offset, int32_t num_steps,
                         const double* fhyp, const double* f_actual, const double* noise, const i7m_sampled_opts* opts,
                         double* err_out, int32_t* best_out, double* q_out, double* ee_out, double* fbest_out,
                         double* xcur_out, double* xu_best_out, double* fhyp_out) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  const SampledCall c = describe_call(h, SampledKind::tracking, G, H, num_steps, opts, 0,
                                      GoalSource::of_reference(ref, L, ref_stride, ref_phase, ref_offset), xstart, fhyp,
                                      f_actual, err_out);
  SampledOut out;
  out.hist = err_out;
  out.best = best_out;
  out.q = q_out;
  out.ee = ee_out;
  out.fbest = fbest_out;
  out.xcur = xcur_out;
  out.xu_best = xu_best_out;
  out.fhyp = fhyp_out;
  return sampled_loop(h, "mpc_run_tracking", c, noise, out);
}

int i7m_sampled_multirate_opts_default(i7m_sampled_multirate_opts* o) {
  if (!o) return fail(I7M_EINVAL, "null opts");
  i7m_sampled_opts s;
  (void)i7m_sampled_opts_default(&s);
  o->sim_dt = s.sim_dt;
  o->decay = s.decay;
  o->frame = s.frame;
  o->reset_what = s.reset_what;
  o->keep_best = s.keep_best;
  o->n_actual = s.n_actual;
  o->shift_warm_start = 0;  // the reference's shift is commented out, src/gato_mpc_batch_sample.py:194-201
  o->control_from = I7M_CONTROL_NEW;
  return I7M_OK;
}

int i7m_mpc_run_sampled_multirate(i7m_handle* h, int32_t G, int32_t H, const double* xstart, const double* endpoints,
                                  int32_t n_endpoints, int32_t num_steps, const double* fhyp, const double* f_actual,
                                  const double* noise, const i7m_sampled_multirate_opts* opts, double* dist_out,
                                  int32_t* best_out, double* q_out, double* u_out, double* xpath_out, double* fbest_out,
                                  double* xcur_out, double* xu_best_out, double* fhyp_out) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  const SharedOpts so(opts);
  const SampledCall c = describe_call(h, SampledKind::endpoints_multirate, G, H, num_steps, &so.o, so.shift_warm_start,
                                      GoalSource::of_endpoints(endpoints, n_endpoints), xstart, fhyp, f_actual, dist_out,
                                      so.control_from);
  SampledOut out;
  out.hist = dist_out;
  out.best = best_out;
  out.q = q_out;
  out.u = u_out;
  out.xpath = xpath_out;
  out.fbest = fbest_out;
  out.xcur = xcur_out;
  out.xu_best = xu_best_out;
  out.fhyp = fhyp_out;
  return sampled_loop(h, "mpc_run_sampled_multirate", c, noise, out);
}

int i7m_mpc_run_tracking_multirate(i7m_handle* h, int32_t G, int32_t H, const double* xstart, const double* ref,
                                   int32_t L, int32_t ref_stride, const int32_t* ref_phase, int32_t num_steps,
                                   const double* fhyp, const double* f_actual, const double* noise,
                                   const i7m_sampled_multirate_opts* opts, double* err_out, int32_t* best_out,
                                   double* q_out, double* u_out, double* xpath_out, double* ee_out, int32_t* off_out,
                                   double* fbest_out, double* xcur_out, double* xu_best_out, double* fhyp_out) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  const SharedOpts so(opts);
  const SampledCall c = describe_call(h, SampledKind::tracking_multirate, G, H, num_steps, &so.o, so.shift_warm_start,
                                      GoalSource::of_reference(ref, L, ref_stride, ref_phase, nullptr), xstart, fhyp,
                                      f_actual, err_out, so.control_from);
  SampledOut out;
  out.hist = err_out;
  out.best = best_out;
  out.q = q_out;
  out.u = u_out;
  out.xpath = xpath_out;
  out.ee = ee_out;
  out.off = off_out;
  out.fbest = fbest_out;
  out.xcur = xcur_out;
  out.xu_best = xu_best_out;
  out.fhyp = fhyp_out;
  return sampled_loop(h, "mpc_run_tracking_multirate", c, noise, out);
}

}  // extern "C"

namespace {

// The session's solve: opts->reset_what on every row (I7M_QP_ADMM), then the rows' SQP from XU into
// d_out, one range on the handle's stream.
int ctrl_solve(i7m_handle* h, int what) {
  const CtrlSession& c = h->ctrl;
  const int B = c.G * c.H;
  const int rc = loop_reset(h, 0, B, what, h->stream, c.dev.at<double>(CWS_RHO0));
  if (rc) return rc;
  return run_sqp(h, B, h->d_xu, h->d_out, h->d_xs, h->d_goal, 3, nullptr);
}

void ctrl_launch_select(i7m_handle* h, const CtrlArgs& a) {
  hipLaunchKernelGGL(k_ctrl_select, dim3(h->ctrl.G), dim3((h->ctrl.H + 63) / 64 * 64), 0, h->stream, a);
}

}  // namespace

extern "C" {

int i7m_ctrl_begin(i7m_handle* h, int32_t G, int32_t H, const double* x0, const double* ref, int32_t L,
                   int32_t ref_stride, const int32_t* ref_phase, const double* fhyp, const i7m_sampled_opts* opts,
                   double* u_out) {
  const std::string who = "ctrl_begin";
  if (!h) return fail(I7M_EINVAL, "null handle");
  if (h->ctrl.open) return fail(I7M_EINVAL, who + ": a controller session is already open on this handle");
  const SampledCall call = describe_call(h, SampledKind::session, G, H, 0, opts, 0,
                                         GoalSource::of_reference(ref, L, ref_stride, ref_phase, nullptr), x0, fhyp, nullptr,
                                         nullptr);
  int rc;
  if ((rc = check_call(who, call, (int)h->N, nullptr))) return rc;
  const i7m_sampled_opts& o = call.o;
  HIPCHK(hipSetDevice(h->dev));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int N = (int)h->N;
  CtrlSession& c = h->ctrl;
  size_t db[CTRL_WS_COUNT], hb[CTRL_HS_COUNT];
  ctrl_ws_bytes(G, H, N, L, ref_stride, ref_phase != nullptr, db);
  ctrl_host_bytes(G, H, hb);
  if (!c.dev.alloc(db, CTRL_WS_COUNT, false)) {
    ctrl_release(h);
    return fail(I7M_ENOMEM, who + ": device allocation failed");
  }
  if (!c.host.alloc(hb, CTRL_HS_COUNT, true)) {
    ctrl_release(h);
    return fail(I7M_ENOMEM, who + ": pinned host allocation failed");
  }
  c.G = G;
  c.H = H;
  c.o = o;
  c.have_last = x0 != nullptr;
  CtrlArgs& a = c.a;
  a.N = N;
  a.H = H;
  a.frame_world = o.frame == I7M_WRENCH_WORLD;
  a.keep_best = o.keep_best != 0;
  a.decay = o.decay;
  a.xs = h->d_xs;
  a.XU = h->d_xu;
  a.xu_new = h->d_out;
  a.goals = h->d_goal;
  a.fext = h->d_fext;
  a.x_meas = c.dev.at<double>(CWS_XMEAS);
  a.x_last = c.dev.at<double>(CWS_XLAST);
  a.u_last = c.dev.at<double>(CWS_ULAST);
  a.xub = c.dev.at<double>(CWS_XUB);
  a.best = c.dev.at<int>(CWS_BEST);
  a.rec = c.dev.at<double>(CWS_REC);
  a.ref = c.dev.at<double>(CWS_REF);
  a.ref_phase = ref_phase ? c.dev.at<int>(CWS_PHASE) : nullptr;
  a.L = L;
  a.ref_stride = ref_stride;
  // gato_controller.py:174-185: the window at offset 0, XU = [x0, 0...] (x0 NULL: the zero state),
  // the hypotheses set on the solver, its state afresh, one solve, XU_best = row 0 of every group
  const GroupStart start(h, G, H, x0, call.goal);
  const auto stage = [&]() -> int {
    int r;
    if ((r = stage_start(h, start, call.goal, G, c.dev.at<double>(CWS_RHO0), c.dev.at<double>(CWS_REF),
                         ref_phase ? c.dev.at<int>(CWS_PHASE) : nullptr)))
      return r;
    if (x0 && (r = copy_in(h, c.dev.at<double>(CWS_XMEAS), x0, (size_t)G * 12))) return r;
    if ((r = install_wrench(h, G * H, fhyp, o.frame))) return r;
    if (G == 0) return I7M_OK;
    if ((r = ctrl_solve(h, I7M_ADMM_RESET_ALL))) return r;
    CtrlArgs s = a;
    s.initial = 1;
    s.noise = nullptr;
    s.x_meas = x0 ? a.x_meas : nullptr;
    ctrl_launch_select(h, s);
    HIPCHK(hipGetLastError());
    if ((r = copy_out(h, c.host.at<double>(CHS_REC), a.rec, (size_t)G * CTRL_REC))) return r;
    HIPCHK(hipStreamSynchronize(h->stream));
    return I7M_OK;
  };
  if ((rc = stage())) {
    const std::string msg = g_err;
    (void)hipStreamSynchronize(h->stream);
    ctrl_release(h);
    g_err = msg;
    return rc;
  }
  for (int g = 0; u_out && g < G; ++g)
    for (int k = 0; k < 6; ++k) u_out[6 * g + k] = c.host.at<double>(CHS_REC)[(size_t)g * CTRL_REC + CREC_U + k];
  c.open = true;
  return I7M_OK;
}

int i7m_ctrl_step(i7m_handle* h, const double* x_meas, double elapsed, int32_t ref_offset, const double* noise,
                  double* u_out, int32_t* best_out, double* fbest_out, double* err_out, double* ee_out) {
  const std::string who = "ctrl_step";
  if (!h) return fail(I7M_EINVAL, "null handle");
  CtrlSession& c = h->ctrl;
  if (!c.open) return fail(I7M_EINVAL, who + ": no controller session is open on this handle (i7m_ctrl_begin)");
  const char* which = "";
  long at = 0;
  if (!ctrl_step_args_ok(x_meas, c.G, elapsed, ref_offset, u_out, &which, &at))
    return fail(I7M_EINVAL, ctrl_step_refusal(who, which, at));
  if (c.G == 0) return I7M_OK;
  HIPCHK(hipSetDevice(h->dev));
  const size_t G = c.G, B = G * c.H;
  // the whole step as one range on the handle's stream: copy-in, measure, reset, solve, select, one
  // copy-out, one synchronisation
  double *px = c.host.at<double>(CHS_XMEAS), *pn = c.host.at<double>(CHS_NOISE), *pr = c.host.at<double>(CHS_REC);
  std::memcpy(px, x_meas, 8 * 12 * G);
  if (noise) std::memcpy(pn, noise, 8 * 3 * B);
  int rc;
  if ((rc = copy_in(h, c.dev.at<double>(CWS_XMEAS), px, 12 * G))) return rc;
  if (noise && (rc = copy_in(h, c.dev.at<double>(CWS_NOISE), pn, 3 * B))) return rc;
  CtrlArgs a = c.a;
  a.elapsed = elapsed;
  a.off = ref_offset;
  a.have_last = c.have_last;
  a.initial = 0;
  a.noise = noise ? c.dev.at<double>(CWS_NOISE) : nullptr;
  hipLaunchKernelGGL(k_ctrl_measure, dim3(c.G), dim3((c.H + 63) / 64 * 64), 0, h->stream, h->d_model, a);
  HIPCHK(hipGetLastError());
  if ((rc = ctrl_solve(h, c.o.reset_what))) return rc;
  // the policy on: the gains of every row behind the solve, while the rows' wrenches are the solve's
  if (c.n_k > 0 && (rc = policy_pass(h, h->stream, bufs_at(h, 0), params_of(h, (int)B, 3), h->d_out, h->d_xs, h->d_goal)))
    return rc;
  ctrl_launch_select(h, a);
  HIPCHK(hipGetLastError());
  if (c.n_k > 0) {
    HIPCHK(i7m_launch_ctrl_policy_copy(c.G, c.H, (int)h->N, c.n_k, h->stream, a.best, h->d_kbuf, a.xub, c.d_pol));
    if ((rc = copy_out(h, c.h_pol, c.d_pol, G * c.n_k * CTRL_POLICY_REC))) return rc;
  }
  if ((rc = copy_out(h, pr, a.rec, G * CTRL_REC))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  c.have_last = true;
  c.pol_stepped = c.n_k > 0;
  for (size_t g = 0; g < G; ++g) {
    const double* r = pr + g * CTRL_REC;
    for (int k = 0; k < 6; ++k) u_out[6 * g + k] = r[CREC_U + k];
    if (best_out) best_out[g] = (int32_t)r[CREC_BEST];
    for (int k = 0; fbest_out && k < 6; ++k) fbest_out[6 * g + k] = r[CREC_FBEST + k];
    if (err_out) err_out[g] = r[CREC_ERR];
    for (int k = 0; ee_out && k < 3; ++k) ee_out[3 * g + k] = r[CREC_EE + k];
  }
  return I7M_OK;
}

int i7m_ctrl_set_policy(i7m_handle* h, int32_t n_k) {
  const std::string who = "ctrl_set_policy";
  if (!h) return fail(I7M_EINVAL, "null handle");
  CtrlSession& c = h->ctrl;
  const char* which = "";
  long at = 0;
  if (!ctrl_set_policy_ok(c.open, n_k, (int)h->N, &which, &at)) return fail(I7M_EINVAL, ctrl_policy_refusal(who, which, at, (int)h->N));
  HIPCHK(hipSetDevice(h->dev));
  HIPCHK(hipStreamSynchronize(h->stream));  // nothing queued still uses the old buffers
  ctrl_policy_release(c);
  if (n_k == 0 || c.G == 0) {
    c.n_k = n_k;
    return I7M_OK;
  }
  const size_t bytes = 8 * (size_t)c.G * n_k * CTRL_POLICY_REC;
  if (hipMalloc((void**)&c.d_pol, bytes) != hipSuccess) {
    c.d_pol = nullptr;
    return fail(I7M_ENOMEM, who + ": device allocation failed");
  }
  if (hipHostMalloc((void**)&c.h_pol, bytes, hipHostMallocDefault) != hipSuccess) {
    c.h_pol = nullptr;
    ctrl_policy_release(c);
    return fail(I7M_ENOMEM, who + ": pinned host allocation failed");
  }
  c.n_k = n_k;
  return I7M_OK;
}

int i7m_ctrl_get_policy(i7m_handle* h, double* K_out, double* xu_ref_out) {
  const std::string who = "ctrl_get_policy";
  if (!h) return fail(I7M_EINVAL, "null handle");
  const CtrlSession& c = h->ctrl;
  const char* which = "";
  long at = 0;
  if (!ctrl_get_policy_ok(c.open, c.n_k > 0, c.pol_stepped || (c.n_k > 0 && c.G == 0), &which, &at))
    return fail(I7M_EINVAL, ctrl_policy_refusal(who, which, at, (int)h->N));
  // the staging of the last step, whose synchronisation has passed: a host copy
  for (size_t e = 0; e < (size_t)c.G * c.n_k; ++e) {
    const double* r = c.h_pol + e * CTRL_POLICY_REC;
    if (K_out) std::memcpy(K_out + e * CTRL_POLICY_K, r, 8 * CTRL_POLICY_K);
    if (xu_ref_out) std::memcpy(xu_ref_out + e * CTRL_POLICY_XU, r + CTRL_POLICY_K, 8 * CTRL_POLICY_XU);
  }
  return I7M_OK;
}

int i7m_ctrl_set_applied(i7m_handle* h, const double* u_applied) {
  const std::string who = "ctrl_set_applied";
  if (!h) return fail(I7M_EINVAL, "null handle");
  CtrlSession& c = h->ctrl;
  const char* which = "";
  long at = 0;
  if (!ctrl_set_applied_ok(c.open, c.have_last, u_applied, c.G, &which, &at))
    return fail(I7M_EINVAL, ctrl_policy_refusal(who, which, at, (int)h->N));
  if (c.G == 0) return I7M_OK;
  HIPCHK(hipSetDevice(h->dev));
  // u_last of the next step's scoring; that step's select stores its own control over it
  c.u_applied.assign(u_applied, u_applied + 6 * (size_t)c.G);
  return copy_in(h, c.a.u_last, c.u_applied.data(), 6 * (size_t)c.G);
}

int i7m_ctrl_end(i7m_handle* h, double* xu_best_out, double* fhyp_out) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  CtrlSession& c = h->ctrl;
  if (!c.open) return fail(I7M_EINVAL, "ctrl_end: no controller session is open on this handle (i7m_ctrl_begin)");
  HIPCHK(hipSetDevice(h->dev));
  const size_t G = c.G, B = G * c.H;
  int rc = I7M_OK;
  if (xu_best_out) rc = copy_out(h, xu_best_out, c.a.xub, G * h->T);
  if (!rc && fhyp_out) rc = copy_out(h, fhyp_out, h->d_fext, B * 6);
  const std::string msg = g_err;
  const hipError_t e = hipStreamSynchronize(h->stream);
  ctrl_release(h);  // the session closes whatever the copies did
  if (rc) return fail(rc, msg);
  if (e != hipSuccess) return fail(I7M_EHIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
  return I7M_OK;
}

int i7m_set_timing(i7m_handle* h, int enable) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  h->timing = enable != 0;
  return I7M_OK;
}

int i7m_get_kernel_times(i7m_handle* h, double* ms_sum, int32_t* counts, int32_t n) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  HIPCHK(hipStreamSynchronize(h->stream));
  for (auto& t : h->ev) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, t.a, t.b));
    h->ms_sum[t.kid] += ms;
    h->counts[t.kid] += 1;
    h->pool.push_back(t.a);
    h->pool.push_back(t.b);
  }
  h->ev.clear();
  for (int i = 0; i < n && i < I7M_K_COUNT; ++i) {
    if (ms_sum) ms_sum[i] = h->ms_sum[i];
    if (counts) counts[i] = h->counts[i];
  }
  return I7M_OK;
}

int i7m_reset_kernel_times(i7m_handle* h) {
  if (!h) return fail(I7M_EINVAL, "null handle");
  int rc = i7m_get_kernel_times(h, nullptr, nullptr, 0);
  if (rc) return rc;
  for (int i = 0; i < I7M_K_COUNT; ++i) {
    h->ms_sum[i] = 0;
    h->counts[i] = 0;
  }
  return I7M_OK;
}

}  // extern "C"
