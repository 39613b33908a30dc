/*
 * indy7_mpc.h — C-ABI of the MI355X-native batched SQP-MPC solver (libindy7mpc.so).
 *
 * Plain C: pointers, sizes, int status codes. No torch / HIP types in any signature
 * (streams are passed as opaque `void*` = hipStream_t).
 *
 * Each entry point replaces a piece of the reference's Python/pinocchio/OSQP hot path
 * (reference A2R-Lab/indy7-mpc @ 2025-05-23, paths relative to its root):
 *
 *   i7m_create / i7m_destroy   OSQPSolver.__init__            src/osqp_solver.py:7-46
 *                              (dims, costs, templates, osqp.setup once; here: device
 *                               buffers for max_batch problems, model constants)
 *   i7m_solve / _device        SQP_OSQP.sqp                   src/osqp_sqp.py:76-93
 *                              — the whole <=2-iteration SQP (linearise, QP, line search,
 *                               step) for B independent problems, batch axis of
 *                               src/gato_mpc_batch.py:38-43,97-99
 *   i7m_qp                     OSQPSolver.setup_and_solve_qp  src/osqp_solver.py:137-143
 *                              (returns the QP minimiser sol.x, solved exactly; with
 *                               qp_mode = I7M_QP_BOX the QP also carries box rows on q, v, u
 *                               — SURVEY.md §8d config 4, an extension without a reference
 *                               counterpart; see oracle/box_ipm.py for its definition; with
 *                               qp_mode = I7M_QP_ADMM it is OSQP's iterate, as the reference's
 *                               osqp.solve() returns it, src/osqp_solver.py:38-40,140-143)
 *   i7m_admm_reset             a fresh OSQP object / batch_sqp resetRho, resetLambda
 *                                                             gato_controller.py:132-138
 *   i7m_linearize              update_constraint_matrix + update_cost_matrix
 *                                                             src/osqp_solver.py:70-135
 *   i7m_merit                  SQP_OSQP.eepos_cost + integrator_err
 *                                                             src/osqp_sqp.py:13-47
 *   i7m_linesearch             SQP_OSQP.linesearch            src/osqp_sqp.py:49-74
 *   i7m_eepos                  OSQPSolver.eepos / d_eepos     src/osqp_solver.py:146-155
 *   i7m_aba                    pin.aba (+f_ext)               src/osqp_sqp.py:40, src/utils.py:5
 *   i7m_aba_derivatives        pin.computeABADerivatives      src/osqp_solver.py:71,76
 *   i7m_rk4                    utils.rk4 (plant)              src/utils.py:3-18
 *   i7m_set_external_wrench    batch_sqp.set_external_wrench_batch  gato_controller.py:129
 *   i7m_mpc_run                MPC_OSQP.run_mpc over B instances     src/osqp_mpc.py:14-72
 *                              (one 0.01 s plant step per solve; the batch axis is that of
 *                               src/gato_mpc_batch.py:84-100, the loop is not)
 *   i7m_mpc_run_multirate      MPC_GATO_Batch.run_mpc over B instances   src/gato_mpc_batch.py:76-217
 *                              (control_from = I7M_CONTROL_NEW), and
 *                              MPC_GATO.run_mpc over B instances         src/gato_mpc.py:53-150
 *                              (sim_dt 0.02, goal_radius 1e-2, control_from = I7M_CONTROL_PREV)
 *   i7m_multirate_substeps     the inner while-loop of both, counted     src/gato_mpc_batch.py:171-199
 *   i7m_mpc_run_sampled        MPC_GATO_Batch_Sample.run_mpc over G controllers of H wrench
 *                              hypotheses       src/gato_mpc_batch_sample.py:106-300
 *                              (find_best_idx / resample_f_ext_batch, gato_controller.py:109-129)
 *   i7m_mpc_run_tracking       GATO_Controller.joint_callback: that loop tracking a reference
 *                              trajectory                     gato_controller.py:201-250
 *   i7m_mpc_run_sampled_multirate   that loop with the plant step split at knot boundaries
 *                              (sim_dt not bounded by dt)     src/gato_mpc_batch_sample.py:163-193
 *   i7m_mpc_run_tracking_multirate  MPC_GATO_Batch_Sample.run_mpc_fig8, the figure-8 tracking run
 *                              under an unknown force         notebooks/gato_mpc_indy7_fig8.ipynb
 *   i7m_ctrl_begin / _step / _end   GATO_Controller.__init__ / joint_callback on a state measured
 *                              outside the device             gato_controller.py:174-185,201-250
 *
 * Layouts (all fp64, C-contiguous, row = problem):
 *   XU    (B, T)  T = 18N-6, [x_0,u_0,x_1,u_1,...,x_{N-1}], x=[q(6),v(6)]  src/osqp_solver.py:22
 *   xcur  (B, 12)
 *   goals (B, N*goal_stride), goal_stride 3 (OSQP surface, src/osqp_solver.py:111) or
 *         6 (batch_sqp surface, gato_controller.py:180-183; first 3 of each 6 used)
 *
 * QP modes (SURVEY.md §8(b) `qp_mode {direct, admm}`):
 *   - I7M_QP_DIRECT solves each SQP subproblem QP exactly (the optimum OSQP's ADMM approximates to
 *     eps 1e-3, src/osqp_solver.py:39-41) and keeps no state between calls;
 *   - I7M_QP_ADMM runs OSQP's algorithm itself (oracle/osqp_admm.py, pinned by the reference's
 *     printed closed loop): per problem a solver state (iterates, rho, the previous QP's linear
 *     cost) carried from call to call like the reference's osqp.OSQP object — i7m_reset or
 *     i7m_admm_reset start it afresh;
 *   - I7M_QP_BOX (config 4) adds box rows, solved by an interior point whose Newton steps are the
 *     exact solve (ADMM needed 40-4700 iterations on those problems).
 * Precision: i7m_config.precision exists; only I7M_PREC_F64 is built, and
 * i7m_create refuses I7M_PREC_F32 with I7M_EINVAL — every kernel computes in fp64.  The drop-in
 * batch_sqp module keeps the reference's SQPSolverfloat_* class names (gato_controller.py:54-62)
 * so callers run unchanged, but it also solves (and returns) fp64.
 *
 * Status: 0 = OK, <0 = error (see I7M_E*), message via i7m_last_error() (thread-local).
 * Threading: a handle is not re-entrant (like the reference's stateful OSQPSolver);
 * use one handle per (host thread, device).
 */
#ifndef INDY7_MPC_H
#define INDY7_MPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define I7M_NJ 6
#define I7M_NX 12
#define I7M_NU 6
#define I7M_MAX_SQP 8
#define I7M_MAX_N 64

/* ABI revision, returned by i7m_abi_version(); bumped whenever an existing signature, struct
 * layout, field meaning or enum count changes.  12: i7m_sampled_multirate_opts' former `pad` is
 * `control_from` (same layout; 0 is what every earlier caller wrote there and means what it did),
 * i7m_ctrl_set_policy / i7m_ctrl_get_policy / i7m_ctrl_set_applied (appended; nothing existing
 * changed).  11: i7m_qp_policy, i7m_multirate_knots and the value
 * I7M_CONTROL_POLICY of i7m_multirate_opts.control_from, which ABI 10 refused (appended; nothing
 * existing changed).  10: i7m_sampled_multirate_opts_default /
 * i7m_mpc_run_sampled_multirate / i7m_mpc_run_tracking_multirate (appended; nothing existing
 * changed).  9: i7m_multirate_opts_default /
 * i7m_multirate_substeps / i7m_mpc_run_multirate (appended; nothing existing changed).  8: i7m_ctrl_begin / i7m_ctrl_step / i7m_ctrl_end
 * (appended; nothing existing changed).  7: i7m_mpc_run_tracking (appended; nothing
 * existing changed) (0.7 builds).  6: i7m_get_admm_status has the value 2 ("solved
 * inaccurate") and, after admm_max_iter, runs OSQP's closing tests (0.6 builds).  5: i7m_get_admm_status and i7m_get_admm_dual
 * (appended); i7m_get_admm_stats' iteration record is reset to -1 at the start of every solve
 * (0.5 builds).  4: I7M_QP_ADMM and i7m_config's admm_* fields
 * (appended), I7M_K_COUNT 10 (I7M_K_ADMM, I7M_K_ADMM_PREP), i7m_admm_reset / i7m_get_admm_stats /
 * i7m_get_admm_state, the `precision` field in the former admm_pad slot (0.4 builds).  3: i7m_config's former `pad` is `h2h_chunks` (a
 * nonzero value changes how i7m_solve runs; outside [0, 64] it is refused) and I7M_K_COUNT is 8
 * (I7M_K_LINESEARCH_TAIL added) — size timing arrays from I7M_K_COUNT of this header (0.3 builds).
 * 2: i7m_aba / i7m_rk4 take a wrench `frame` before their outputs and i7m_set_external_wrench a
 * trailing `frame` (0.2 builds); 1 had neither.  A caller built against another revision must not
 * call through this library: compare first. */
#define I7M_ABI_VERSION 12

#define I7M_OK 0
#define I7M_EINVAL -1   /* bad argument (size, null pointer, unsupported N) */
#define I7M_EHIP -2     /* HIP runtime error */
#define I7M_ENOMEM -3   /* device allocation failed */
#define I7M_ENODEV -4   /* no usable gfx950 device */

enum { I7M_QP_DIRECT = 0, I7M_QP_BOX = 1, I7M_QP_ADMM = 2 };
/* How a solve is launched (I7M_QP_DIRECT): FUSED = one kernel per solve (a workgroup per
 * problem runs every SQP iteration's linearisation, QP and line search), FUSED_ITER = that kernel
 * once per SQP iteration, SPLIT = three kernels per SQP iteration; AUTO = SPLIT at every batch
 * size (the fused kernel measured slower at every size).  Bit-identical results
 * in every mode. */
enum { I7M_PIPE_AUTO = 0, I7M_PIPE_SPLIT = 1, I7M_PIPE_FUSED = 2, I7M_PIPE_FUSED_ITER = 3 };
enum { I7M_PREC_F64 = 0, I7M_PREC_F32 = 1 };
#define I7M_BOX_Q 1     /* q_lower <= q <= q_upper    description/indy7.urdf:203-238 <limit> */
#define I7M_BOX_V 2     /* |v| <= velocity limit */
#define I7M_BOX_U 4     /* |u| <= effort limit */

/* 6-DOF serial chain of revolute joints about local +z. Layout == RobotModel.packed(). */
typedef struct i7m_model {
  double placement_R[6][9];   /* joint frame in parent joint frame, row-major */
  double placement_t[6][3];
  double mass[6];
  double com[6][3];           /* in the joint frame */
  double inertia[6][6];       /* about the COM: xx xy xz yy yz zz */
  double gravity[3];          /* (0,0,-9.81), src/osqp_mpc.py:8-9 */
  double q_lower[6], q_upper[6], v_limit[6], effort_limit[6];
} i7m_model;

typedef struct i7m_config {
  int32_t N;            /* knot points (<= I7M_MAX_N), default 32   src/osqp_solver.py:7 */
  int32_t regularize;   /* default 1 */
  double dt;            /* default 0.01 */
  double dQ_cost;       /* default 0.01 */
  double R_cost;        /* default 1e-5 */
  double QN_cost;       /* default 100 */
  double eps;           /* default 1 */
  double mu;            /* merit penalty, 10          src/osqp_sqp.py:50 */
  double step_tol;      /* SQP break tolerance, 1e-3  src/osqp_sqp.py:90 */
  int32_t max_sqp_iters;/* 2                          src/osqp_sqp.py:77 */
  int32_t max_batch;    /* device buffers are sized for this many problems */
  int32_t device_id;
  int32_t qp_mode;      /* I7M_QP_DIRECT: exact block-tridiagonal (Riccati) KKT solve;
                           I7M_QP_BOX: + box rows on q, v, u (interior point, Riccati Newton steps);
                           I7M_QP_ADMM: OSQP's ADMM with its warm-started state */
  i7m_model model;
  /* I7M_QP_BOX only (appended: the offsets above are unchanged) */
  int32_t box_mask;     /* which rows: I7M_BOX_Q | I7M_BOX_V | I7M_BOX_U (default all) */
  int32_t box_max_iters;/* interior-point iterations per QP, default 30 */
  double box_tol;       /* stop when mu < tol and the residuals shrank by tol, default 1e-8 */
  int32_t pipeline;     /* I7M_PIPE_* (appended), default I7M_PIPE_AUTO */
  int32_t h2h_chunks;   /* i7m_solve (host buffers): split the batch into this many chunks, copies in,
                           solves and copies out pipelined on three streams so copies overlap
                           solves; 0 = automatic (was `pad`: same layout) */
  /* I7M_QP_ADMM only (appended): OSQP's settings; defaults (i7m_config_default) are OSQP's own
     with the duality-gap test on and no rho adaptation — the combination that reproduces the
     reference's printed closed loop (oracle/osqp_admm.py) */
  double admm_rho;              /* 0.1; equality rows use 1e3 rho (all of this QP's rows) */
  double admm_sigma;            /* 1e-6 */
  double admm_alpha;            /* relaxation, 1.6 */
  double admm_eps_abs;          /* 1e-3 */
  double admm_eps_rel;          /* 1e-3 */
  int32_t admm_max_iter;        /* 4000 */
  int32_t admm_check_termination; /* 25: residuals are tested every this many iterations */
  int32_t admm_scaling;         /* Ruiz passes, 10 */
  int32_t admm_check_dualgap;   /* 1: OSQP 1.x's duality-gap test */
  int32_t admm_adaptive_rho_interval; /* 0: never adapt rho; else every this many iterations */
  int32_t precision;    /* arithmetic of every kernel (SURVEY.md 8b's ABI sketch): I7M_PREC_F64 (0, the
                           only one built: the reference's OSQP path computes in double);
                           I7M_PREC_F32 (GATO's float, gato_controller.py:54-62) is refused by
                           i7m_create with I7M_EINVAL.  (Was admm_pad: same layout.) */
  double admm_adaptive_rho_tolerance; /* 5 */
} i7m_config;

/* Per-problem SQP statistics (keys of SQP_OSQP.stats, src/osqp_sqp.py:7-11). */
typedef struct i7m_problem_stats {
  int32_t qp_iters;                 /* qp+1 at loop exit                 */
  int32_t n_alphas;                 /* entries of linesearch_alphas       */
  int32_t n_steps;                  /* entries of sqp_stepsizes           */
  int32_t pad;
  double alphas[I7M_MAX_SQP];
  double stepsizes[I7M_MAX_SQP];
} i7m_problem_stats;

typedef struct i7m_handle i7m_handle;

const char* i7m_last_error(void);
const char* i7m_version(void);
int i7m_abi_version(void);                        /* == I7M_ABI_VERSION of the header it was built with */
int i7m_config_default(i7m_config* cfg);          /* fills everything but `model` */
int i7m_device_count(int* n);

/* In ADMM mode the handle's OSQP state (about 4 KB x N per problem) must stay under 2 GiB: the
   iteration kernel addresses it with 32-bit offsets; a larger max_batch x N is refused with
   I7M_EINVAL (shard the batch over handles instead). */
int i7m_create(const i7m_config* cfg, i7m_handle** out);
void i7m_destroy(i7m_handle* h);
/* NULL -> the handle's own stream, a blocking stream (ordered with the legacy null stream) */
int i7m_set_stream(i7m_handle* h, void* stream);
/* Back to the post-create solver state (batch_sqp reset / resetRho / resetLambda,
 * gato_controller.py:132-138): waits for the handle's stream, drops captured solve graphs and
 * zeroes the kernel timing sums; I7M_QP_ADMM: every problem's OSQP state starts afresh
 * (i7m_admm_reset(h, max_batch, I7M_ADMM_RESET_ALL)).  The exact modes carry no warm start,
 * penalty or dual state across calls.  The external wrench is caller input like the model and is
 * kept: clear it with i7m_set_external_wrench(h, 0, NULL, 0). */
int i7m_reset(i7m_handle* h);
int i7m_synchronize(i7m_handle* h);

/* External wrench [force; torque] acting on joint 6's body.  Frames:
 *   I7M_WRENCH_WORLD  a spatial force in the WORLD frame, about the world origin, as the
 *                     reference's callers draw it (gato_controller.py:77-81,120-129;
 *                     src/gato_mpc_batch_sample.py:37-40).  Every dynamics evaluation converts
 *                     it to joint 6's frame at that evaluation's configuration with
 *                     oMi[6].actInv (src/gato_mpc_batch_sample.py:151-161,270-279), and the
 *                     linearisation differentiates that conversion too.  i7m_rk4 converts once
 *                     at the start configuration and holds it over the four stages, as the
 *                     reference's host plant does (:270-279).
 *   I7M_WRENCH_LOCAL  constant in joint 6's LOCAL frame (pinocchio's f_ext[6] as it is). */
#define I7M_WRENCH_LOCAL 0
#define I7M_WRENCH_WORLD 1
/* One wrench per problem, used by every dynamics evaluation of subsequent solves
 * (linearisation and merit).  fext (B, 6); NULL clears it.  Backs
 * batch_sqp.set_external_wrench_batch (gato_controller.py:129). */
int i7m_set_external_wrench(i7m_handle* h, int32_t B, const double* fext, int32_t frame);

/* Full SQP solve, host buffers in/out (H2D + kernels + D2H, synchronous). */
int i7m_solve(i7m_handle* h, int32_t B, const double* xu_in, const double* xcur, const double* goals,
              int32_t goal_stride, double* xu_out, i7m_problem_stats* stats);

/* Full SQP solve on device-resident buffers, asynchronous on the handle's stream.
 * d_stats may be NULL. xu_in may alias xu_out (in-place); otherwise xu_in is only read and every
 * row of xu_out is written (no staging copy). */
int i7m_solve_device(i7m_handle* h, int32_t B, const double* d_xu_in, const double* d_xcur,
                     const double* d_goals, int32_t goal_stride, double* d_xu_out,
                     i7m_problem_stats* d_stats);

/* One QP (linearise at xu, solve exactly): sol (B, T). */
int i7m_qp(i7m_handle* h, int32_t B, const double* xu, const double* xcur, const double* goals,
           int32_t goal_stride, double* sol);

/* The QP's optimal cost-to-go at the first knot (the Riccati value function V~_0 in homogeneous
 * coordinates x~ = [x_0; 1], as the backward sweep ends with it): V0 (B, 13, 13) row-major, the
 * quadratic form the exact solve of i7m_qp minimises over the rest of the trajectory given x_0
 * — its 12 x 12 block is d^2 J* / d x_0^2 (the sensitivity of the optimal QP cost to the initial
 * state, the derivative of the equality multiplier of the x_0 rows l[:12] = -xs of
 * src/osqp_solver.py:85), its last column the linear part.  Diagnostic / test hook (the reference
 * has no counterpart; OSQP returns the multipliers `y`, src/osqp_solver.py:143).  Returned as
 * the recursion computes it except row 12, which the kernel mirrors from column 12 (the linear
 * part); the 12 x 12 block is symmetric only to the recursion's accuracy.  I7M_QP_DIRECT only,
 * N >= 10 (checked before any work). */
int i7m_qp_value(i7m_handle* h, int32_t B, const double* xu, const double* xcur, const double* goals,
                 int32_t goal_stride, double* V0);

/* The QP's feedback policy (ABI 11): the time-varying LQR gains the exact solve's backward Riccati
 * sweep computes, K~_k = -H^-1 G~ (6 x 13) of stages k = 0 .. n_k - 1, for the QP linearised at xu
 * with xcur as the x_0 row, exactly as i7m_qp.  K_out (B, n_k, 6, 13) row-major: K_out[b, k, :, :12]
 * is the gain K_k, K_out[b, k, :, 12] the feedforward, and the QP's minimiser satisfies u_k =
 * K~_k [x_k; 1] in absolute coordinates (the QP variable is XU itself, l[:12] = -xs of
 * src/osqp_solver.py:85), so that between solves u = u_k + K_k (x - x_k) is the QP's own answer to a
 * state x off the planned x_k.  sol_out (B, T) or NULL: the minimiser, the buffer i7m_qp returns on
 * an I7M_QP_DIRECT handle, bit for bit.  The reference has no counterpart: OSQP returns an iterate,
 * not a policy.  I7M_QP_DIRECT and I7M_QP_ADMM: on an ADMM handle this is the exact QP's policy at
 * that linearisation, which OSQP's iterate approximates, and the carried OSQP state is left
 * untouched.  I7M_EINVAL with a message naming the argument, before any device work: an I7M_QP_BOX
 * handle (its corrector steps overwrite the stored feedforward); n_k outside [1, N - 1]; null K_out,
 * xu, xcur or goals; an open controller session.  Synchronous. */
int i7m_qp_policy(i7m_handle* h, int32_t B, const double* xu, const double* xcur, const double* goals,
                  int32_t goal_stride, int32_t n_k, double* K_out /* (B, n_k, 6, 13) */,
                  double* sol_out /* (B, T) or NULL */);

/* I7M_QP_BOX: interior-point record of the most recent QP of problems [0, B) (the last
 * i7m_qp, or the last SQP iteration of i7m_solve): corrector steps taken, 1 if converged
 * (mu < box_tol and residuals reduced by box_tol), final mu.  Any output may be NULL. */
int i7m_get_box_stats(i7m_handle* h, int32_t B, int32_t* iters, int32_t* converged, double* mu);

/* I7M_QP_ADMM: start the OSQP state of problems [0, B) afresh.  what: I7M_ADMM_RESET_RHO (rho back
 * to admm_rho; batch_sqp resetRho), _DUAL (y = 0; resetLambda), _PRIMAL (x = z = 0 and the
 * remembered linear cost = 0), _ALL (a new OSQP object: the state right after create). */
#define I7M_ADMM_RESET_RHO 1
#define I7M_ADMM_RESET_DUAL 2
#define I7M_ADMM_RESET_PRIMAL 4
#define I7M_ADMM_RESET_ALL 7
int i7m_admm_reset(i7m_handle* h, int32_t B, int32_t what);
/* I7M_QP_ADMM: OSQP iterations of every SQP iteration of the last solve (B, I7M_MAX_SQP; -1 where
 * the problem ran no QP) and the current rho (B).  Either may be NULL. */
int i7m_get_admm_stats(i7m_handle* h, int32_t B, int32_t* iters, double* rho);
/* I7M_QP_ADMM: the carried OSQP state of problems [0, B) in OSQP's scaled coordinates: x (B, T),
 * z, y (B, 12N), the previous QP's linear cost, unscaled (B, T), rho (B).  Any may be NULL. */
int i7m_get_admm_state(i7m_handle* h, int32_t B, double* x, double* z, double* y, double* q, double* rho);
/* I7M_QP_ADMM (ABI 6): OSQP's result status of every SQP iteration's QP in the last solve
 * (B, I7M_MAX_SQP): 1 "solved" (its termination test passed), 2 "solved inaccurate" and 0
 * "maximum iterations reached" (admm_max_iter came first: as OSQP, the test is run once more at
 * the final iterate unless the last iteration ran it, then with eps_abs and eps_rel x 10, which
 * gives 2), -1 the problem ran no QP at that iteration.  The reference's solve() returns it in
 * .info.status (src/osqp_solver.py:143). */
int i7m_get_admm_status(i7m_handle* h, int32_t B, int32_t* status);
/* I7M_QP_ADMM (ABI 5): the dual y of each problem's last QP, unscaled as OSQP returns it in
 * result.y (y = E y_s / c: the carried scaled y with that QP's row scaling E and cost scale c),
 * (B, 12N). */
int i7m_get_admm_dual(i7m_handle* h, int32_t B, double* y);

/* Raw linearisation at xu.  lin (B, N-1, 114): per knot Aq(6x6,row-major, =dt*da/dq),
 * Av (=I+dt*da/dv), Bu (=dt*Minv), a (=ABA(q,v,u)); cost (B, N, 10): j = J^T e (6),
 * Qm, dQm, Rm, |e|.  Either output may be NULL. */
int i7m_linearize(i7m_handle* h, int32_t B, const double* xu, const double* goals, int32_t goal_stride,
                  double* lin, double* cost);

/* Merit pieces of XU (relative to XU_ref for the initial-state term): out (B, 5) =
 * qcost, vcost, ucost, integrator_err, |XU[:12]-XU_ref[:12]|. */
int i7m_merit(i7m_handle* h, int32_t B, const double* xu, const double* xu_ref, const double* goals,
              int32_t goal_stride, double* out);

/* Backtracking line search of src/osqp_sqp.py:49-74 (no step applied): alpha (B). */
int i7m_linesearch(i7m_handle* h, int32_t B, const double* xu, const double* xu_full,
                   const double* goals, int32_t goal_stride, double* alpha);

/* Kinematics / dynamics hooks, Bq independent queries (q,v,tau: (Bq,6)). */
int i7m_eepos(i7m_handle* h, int32_t Bq, const double* q, double* p_out, double* J_out /*(Bq,3,6) or NULL*/);
int i7m_aba(i7m_handle* h, int32_t Bq, const double* q, const double* v, const double* tau,
            const double* fext /*(Bq,6) spatial force on joint 6, or NULL*/, int32_t frame /*I7M_WRENCH_**/,
            double* a_out);
int i7m_aba_derivatives(i7m_handle* h, int32_t Bq, const double* q, const double* v, const double* tau,
                        double* dq /*(Bq,6,6)*/, double* dv, double* Minv, double* a);
int i7m_rk4(i7m_handle* h, int32_t Bq, const double* q, const double* v, const double* u, double dt,
            const double* fext, int32_t frame, double* q_out, double* v_out);

/* Closed-loop MPC of B independent instances on the device: MPC_OSQP.run_mpc
 * (src/osqp_mpc.py:14-72) per instance — goal = endpoints[0] tiled, XU = 0, an initial solve,
 * then per step: goal distance of xcur (cyclic switch below 0.1, the instance stops above 1.1),
 * xu_new = SQP solve, the rk4 plant over 0.01 s with the PREVIOUS trajectory's controls, the
 * warm-start shift and the first / last state pins — all batched, state resident in HBM (the
 * loop of src/gato_mpc_batch.py:76-217 itself is i7m_mpc_run_multirate).  xstart (B, 12), endpoints (E, 3);
 * dist_out (num_steps, B) goal distances (NaN once an instance has stopped); q_out
 * (num_steps, B, 6) q after each step's plant, xcur_out (B, 12), xu_out (B, T) the final state
 * and warm start: each may be NULL but dist_out.  Synchronous.  I7M_EINVAL if the handle has an
 * external wrench set (MPC_OSQP's loop has none, src/osqp_mpc.py:56). */
int i7m_mpc_run(i7m_handle* h, int32_t B, const double* xstart, const double* endpoints, int32_t n_endpoints,
                int32_t num_steps, double* dist_out, double* q_out, double* xcur_out, double* xu_out);

/* Options of i7m_mpc_run_multirate; fill with i7m_multirate_opts_default, then change fields. */
#define I7M_CONTROL_NEW 0   /* the plant is driven by this step's solve: MPC_GATO_Batch, src/gato_mpc_batch.py:185 */
#define I7M_CONTROL_PREV 1  /* by the warm start the solve started from: MPC_GATO, src/gato_mpc.py:126 */
/* (ABI 11) by this step's solve under its own feedback policy; the reference has no counterpart.
 * After the solve a policy pass linearises at xu_new with x_0 = xcur and runs the exact backward
 * sweep (i7m_qp_policy's launches, in both QP modes); the sub-step that begins at plant state x with
 * j knots of this step completed is driven by u = xu_new.u_j + K_j (x - xu_new.x_j), K_j the 6 x 12
 * gain of stage j.  j advances where the schedule places a knot boundary (i7m_multirate_knots).  At
 * x = xu_new.x_j the control is xu_new.u_j bit for bit, so a step's first sub-step runs under
 * I7M_CONTROL_NEW's control.  Everything else of the step is as described below.  Refused in addition: a step
 * that completes more than N - 2 knots (knot N - 1 has no control). */
#define I7M_CONTROL_POLICY 2
typedef struct i7m_multirate_opts {
  double sim_dt;        /* plant time per solve, finite and > 0, not bounded by dt; default 0.001
                           (src/gato_mpc_batch.py:76; MPC_GATO hard-codes 0.02, src/gato_mpc.py:76) */
  double goal_radius;   /* default 0.1 (src/gato_mpc_batch.py:158; MPC_GATO: 1e-2, src/gato_mpc.py:106) */
  int32_t control_from; /* I7M_CONTROL_*; default NEW */
  int32_t reset_what;   /* I7M_QP_ADMM: I7M_ADMM_RESET_* bits applied to every instance before each
                           step's solve; default ALL (solver.reset(), :116); 0 carries the OSQP state */
} i7m_multirate_opts;
int i7m_multirate_opts_default(i7m_multirate_opts* opts);

/* Pure host: the total number of plant sub-steps of a run of num_steps MPC steps, to size
 * xpath_out; I7M_EINVAL with i7m_mpc_run_multirate's refusals of sim_dt. */
int i7m_multirate_substeps(double dt, double sim_dt, int32_t N, int32_t num_steps, int32_t* n_sub);
/* Pure host (ABI 11): knot_out[s] (n_sub entries, or NULL) = the knots its MPC step had completed when
 * plant sub-step s began, 0 .. shift of the step: the knot whose control and gain drive the sub-step
 * under I7M_CONTROL_POLICY.  I7M_EINVAL with i7m_mpc_run_multirate's refusals of sim_dt and
 * control_from for that control_from, the N - 2 bound of I7M_CONTROL_POLICY among them. */
int i7m_multirate_knots(double dt, double sim_dt, int32_t N, int32_t num_steps, int32_t control_from, int32_t* knot_out);

/* Multi-rate closed loop of B independent instances on the device: MPC_GATO_Batch.run_mpc
 * (src/gato_mpc_batch.py:76-217) and, with other options, MPC_GATO.run_mpc (src/gato_mpc.py:53-150).
 * The plant advances opts->sim_dt per solve against the handle's knot grid dt: ten solves per knot
 * with 0.001 / 0.01, two knots per solve with 0.02 / 0.01.
 *   init    goal = endpoints[0] tiled; XU = 0 but XU[:12] = xstart; the solver state afresh;
 *           XU = sqp(XU) (:84-100)
 *   step i, every instance still running, in the reference's order:
 *     reset    I7M_QP_ADMM: opts->reset_what on every instance (:116)
 *     solve    xu_new = sqp(xcur, goal, XU), against the goal before any switch of this step (:121)
 *     distance d = |eepos(xcur q) - goal|, dist_out[i, b] = d; u_out[i, b] = XU[12:18], the warm
 *              start's first control before this step's update (the reference's control_inputs, :153)
 *     goal     d < goal_radius: the next endpoint, goal rows re-tiled (not cyclic, :158-165); at the
 *              last endpoint the instance stops here, before the plant (:166-168): q_out[i, b] and
 *              this step's xpath slots are NaN.  There is no stop at 1.1.
 *     plant    the step's sim_dt is split where it crosses a knot boundary: a time accumulator,
 *              carried over all steps, holds the position inside the current knot; each sub-step
 *              ts = min(remaining, dt - accumulated) is one rk4 step without a wrench, and a knot
 *              completes when |accumulated - dt| < 1e-10 (:171-199).  The split depends on dt,
 *              sim_dt and i alone and is computed on the host in the reference's double arithmetic;
 *              its float residues are kept (dt 0.01, sim_dt 0.001: step 9 is [0.001, 8.67e-19], the
 *              second a real rk4 call and a real xpath entry).  Every sub-step is driven by knot
 *              0's control, u = xu_new[12:18] (I7M_CONTROL_NEW, :185) or XU[12:18] (I7M_CONTROL_PREV,
 *              src/gato_mpc.py:126): the reference's current_interval is always 0, because the
 *              accumulator is reset at every boundary.  xpath_out[s, b] = q after sub-step s (the
 *              reference's self.xpath), q_out[i, b] = q after the last one.
 *     shift    with s > 0 knots completed XU[:T - 18 s] = xu_new[18 s:], the tail keeping its old
 *              values (:202-203); with s = 0 XU stays the OLDER trajectory: xu_new drove the plant
 *              only.  Then XU[:12] = xcur, XU[-12:] = [1]*6 + [0]*6 (:206-207).
 * An instance that stopped at step i has dist_out[i] and u_out[i] recorded and q_out[i], its xpath
 * slots of step i NaN; from step i + 1 on all four are NaN.
 * Deliberately not reproduced: src/gato_mpc_batch.py:213 with no knot completed, whose slice
 * `:-(0) or len(XU_batch)` ends at batch_size and overwrites the first batch_size warm-start
 * entries of every row with row 0's.
 * xstart (B, 12), endpoints (E, 3); opts NULL = the defaults.  Outputs: dist_out (num_steps, B)
 * required; q_out and u_out (num_steps, B, 6), xpath_out (n_sub, B, 6) with n_sub from
 * i7m_multirate_substeps(dt, sim_dt, N, num_steps), xcur_out (B, 12), xu_out (B, T): each may be
 * NULL.  num_steps = 0 reduces to the initial solve.  Synchronous.  A large I7M_QP_ADMM batch runs
 * as its two staggered ranges, as i7m_mpc_run's.  I7M_QP_DIRECT and I7M_QP_ADMM; I7M_EINVAL with a
 * message naming the argument, before any device work: I7M_QP_BOX; an external wrench set on the
 * handle (neither driver's plant has one); sim_dt not finite or not positive; a step that completes
 * more than N - 1 knots (N - 2 under I7M_CONTROL_POLICY); a step of more than 66 sub-steps (sim_dt > 64 dt); a bad control_from or
 * reset_what; null xstart, endpoints or dist_out. */
int i7m_mpc_run_multirate(i7m_handle* h, int32_t B, const double* xstart, const double* endpoints, int32_t n_endpoints,
                          int32_t num_steps, const i7m_multirate_opts* opts, double* dist_out /* (steps,B) required */,
                          double* q_out /* (steps,B,6) */, double* u_out /* (steps,B,6) */,
                          double* xpath_out /* (n_sub,B,6) */, double* xcur_out, double* xu_out);

/* Options of i7m_mpc_run_sampled; fill with i7m_sampled_opts_default, then change fields. */
typedef struct i7m_sampled_opts {
  double sim_dt;        /* the plant's and the scoring's one rk4 step per MPC step, 0 < sim_dt <= dt;
                           default 0.001 (src/gato_mpc_batch_sample.py:106) */
  double decay;         /* the resampled hypotheses are scaled by this; default 1 (0.97: gato_controller.py:128) */
  int32_t frame;        /* I7M_WRENCH_* of fhyp, f_actual and the wrench left on the handle; default WORLD */
  int32_t reset_what;   /* I7M_QP_ADMM: I7M_ADMM_RESET_* bits applied to every row before each step's
                           solve; default ALL (the reference's reset() + resetRho(), :222-223); 0
                           carries the OSQP state from step to step */
  int32_t keep_best;    /* resample: the winning row keeps the winning wrench; default 0 */
  int32_t n_actual;     /* f_actual is (n_actual, G, 6): 1 (held for the run) or num_steps; default 1 */
} i7m_sampled_opts;
int i7m_sampled_opts_default(i7m_sampled_opts* opts);

/* Sampled-wrench closed loop of G independent controllers with H wrench hypotheses each on the
 * device: MPC_GATO_Batch_Sample.run_mpc (src/gato_mpc_batch_sample.py:106-300) with the
 * controller's selection and resampling rule (gato_controller.py:109-129).  The B = G H problem
 * rows are laid out so that group g owns rows [g H, (g + 1) H); H in {1, 2, 4, ..., 256} (the
 * SQPSolverfloat_* sizes), B <= max_batch.
 *   init    goal = endpoints[0] tiled; XU rows = 0 but XU[:, :12] = xstart[g] (:124-126); the rows'
 *           wrenches = fhyp (B, 6) in opts->frame; the solver state afresh; XU_new = sqp(rows);
 *           XU_best[g] = XU_new[g H] (:127-128)
 *   step i, every group still running:
 *     plant    x_last = xcur[g], u_last = XU_best[g][12:18]; xcur[g] = rk4(x_last, u_last, sim_dt,
 *              f_actual[i or 0][g]) (:163-178): one step, a world wrench converted once at
 *              x_last's q as i7m_rk4 does; q_out[i, g] = xcur[g][:6]
 *     spread   every row of g: xcur_row = xcur[g], XU_row = [xcur[g], XU_best[g][12:]] (:190-193;
 *              no warm-start shift: the reference's is commented out)
 *     goal     d = |eepos(xcur q) - goal|, dist_out[i, g] = d; d < 0.095: the next endpoint (not
 *              cyclic, :208-214), or at the last endpoint the group stops here (:215-217)
 *     reset    I7M_QP_ADMM: opts->reset_what on every row
 *     solve    XU_new = sqp(rows), each row under its own hypothesis wrench
 *     select   err_h = |rk4(x_last, u_last, sim_dt, wrench row h) - xcur[g]|_2 over all 12 entries;
 *              best = the lowest index among the minima (:287's `<`; a NaN error never wins, all
 *              NaN -> 0); best_out[i, g] = best, fbest_out[i, g] = wrench row best, XU_best[g] =
 *              XU_new[g H + best].  Plant and scoring run the same code, so a hypothesis equal to
 *              the actual wrench scores exactly 0.
 *     resample only with noise (num_steps, B, 3), in gato_controller.py:120-129's order: rows =
 *              f_best; rows[:, :3] += noise[i]; if keep_best: row[best] = f_best; rows[:, 3:] = 0;
 *              row[0] = 0; rows *= decay.  (keep_best = 1, decay = 0.97: the controller's rule;
 *              keep_best = 0, decay = 1: src/gato_mpc_batch_sample.py:291-298.)
 * A group that stopped at step i has best_out[i] = -1 and fbest_out[i] = NaN (no selection was
 * made), and from step i + 1 on dist_out / q_out / fbest_out are NaN and best_out is -1.
 * Deliberately not reproduced: the reference splits a plant step at a knot boundary (:170-187),
 * which with one step of sim_dt <= dt and no shift never happens (the plant stays in knot 0); and
 * it random-walks the actual force (:244-250), where here the caller supplies the schedule
 * f_actual (opts->n_actual, G, 6).
 * xstart (G, 12), endpoints (E, 3); noise may be NULL (no resampling); opts NULL = the defaults.
 * Outputs: dist_out (num_steps, G) required; best_out (num_steps, G) int32, q_out and fbest_out
 * (num_steps, G, 6), xcur_out (G, 12), xu_best_out (G, T) the final XU_best, fhyp_out (B, 6) the
 * final hypotheses: each may be NULL.  Synchronous.  I7M_QP_DIRECT and I7M_QP_ADMM; I7M_EINVAL
 * before any work for I7M_QP_BOX, another H, G H > max_batch, sim_dt outside (0, dt] and null
 * required pointers.  After the run the handle's external wrench is the final hypothesis set in
 * opts->frame (as after i7m_set_external_wrench(h, B, fhyp_out, frame)): i7m_mpc_run keeps
 * refusing the handle until it is cleared. */
int i7m_mpc_run_sampled(i7m_handle* h, int32_t G, int32_t H, const double* xstart, const double* endpoints,
                        int32_t n_endpoints, int32_t num_steps, const double* fhyp, const double* f_actual,
                        const double* noise, const i7m_sampled_opts* opts, double* dist_out, int32_t* best_out,
                        double* q_out, double* fbest_out, double* xcur_out, double* xu_best_out, double* fhyp_out);

/* The sampled-wrench closed loop tracking a reference trajectory: the deployed controller's loop
 * (GATO_Controller.joint_callback, gato_controller.py:201-250) over G controllers of H hypotheses.  It is
 * i7m_mpc_run_sampled (same options, same init / plant / spread / reset / solve / select / resample
 * order, same staggered ranges, same wrench left on the handle) with the goal source replaced:
 *   init    every row of group g is solved against the window at offset 0,
 *           goals[k] = ref[min(ph_g + k, L - 1)][0:3], k = 0 .. N-1 (:180-183), ph_g = ref_phase[g]
 *           or 0
 *   step i, in the goal's place:
 *     track    err_out[i, g] = |eepos(xcur q) - ref[min(ph_g + ref_offset[i], L - 1)]|, the tracking
 *              error the controller logs against the window's first point (:242-246);
 *              ee_out[i, g] = eepos(xcur q); then every row of g gets the window
 *              goals[k] = ref[min(ph_g + ref_offset[i] + k, L - 1)][0:3] (:214-216).  A window that
 *              runs past the end of the reference holds its last point (the controller's slice
 *              would come up short there).  No radius test: a tracking group never stops.
 * ref is (L, ref_stride), ref_stride 3 or 6 (the controller stores [x y z 0 0 0] per point; the
 * first three are read).  ref_offset (num_steps) int32 is the caller's window schedule, like
 * f_actual and noise; the controller's rule int(sum of elapsed / dt) is one.  ref_phase (G) int32
 * may be NULL.  With L = 1 the loop is i7m_mpc_run_sampled's with that one endpoint, as long as
 * that one does not reach it.
 * Outputs as i7m_mpc_run_sampled's, err_out (num_steps, G) required, ee_out (num_steps, G, 3)
 * optional.  Synchronous.  I7M_EINVAL before any work for i7m_mpc_run_sampled's refusals and for
 * L < 1, ref_stride other than 3 or 6, a negative ref_offset or ref_phase entry, and null ref,
 * ref_offset (with num_steps > 0) or err_out. */
int i7m_mpc_run_tracking(i7m_handle* h, int32_t G, int32_t H, const double* xstart, const double* ref, int32_t L,
                         int32_t ref_stride, const int32_t* ref_phase, const int32_t* ref_offset, int32_t num_steps,
                         const double* fhyp, const double* f_actual, const double* noise, const i7m_sampled_opts* opts,
                         double* err_out, int32_t* best_out, double* q_out, double* ee_out, double* fbest_out,
                         double* xcur_out, double* xu_best_out, double* fhyp_out);

/* Options of i7m_mpc_run_sampled_multirate / i7m_mpc_run_tracking_multirate; fill with
 * i7m_sampled_multirate_opts_default, then change fields.  The first six are i7m_sampled_opts'
 * fields with the same meanings and defaults, but for sim_dt's bound. */
typedef struct i7m_sampled_multirate_opts {
  double sim_dt;        /* plant time per solve, finite and > 0, NOT bounded by dt; default 0.001 */
  double decay;         /* default 1 */
  int32_t frame;        /* I7M_WRENCH_*; default WORLD */
  int32_t reset_what;   /* I7M_ADMM_RESET_* bits before each step's solve; default ALL */
  int32_t keep_best;    /* default 0 */
  int32_t n_actual;     /* f_actual is (n_actual, G, 6): 1 or num_steps; default 1 */
  int32_t shift_warm_start; /* 1: the rows' warm start is shifted by the knots a step completes
                           (src/gato_mpc_batch.py:202-203's rule); default 0, as the reference's shift
                           is commented out (src/gato_mpc_batch_sample.py:194-201) */
  int32_t control_from; /* (ABI 12, was `pad`: same layout) I7M_CONTROL_NEW (0, default): the plant holds
                           XU_best's first control over the step; I7M_CONTROL_POLICY (2): the plant runs
                           under the winner's feedback policy, see below.  Anything else, I7M_CONTROL_PREV
                           included (these loops have no such variant), is refused */
} i7m_sampled_multirate_opts;
int i7m_sampled_multirate_opts_default(i7m_sampled_multirate_opts* opts);

/* The sampled-wrench closed loops with a multi-rate plant: i7m_mpc_run_sampled and
 * i7m_mpc_run_tracking where the plant advances opts->sim_dt per solve against the knot grid dt and
 * a plant step is split where it crosses a knot boundary (src/gato_mpc_batch_sample.py:163-193;
 * MPC_GATO_Batch_Sample.run_mpc_fig8 of notebooks/gato_mpc_indy7_fig8.ipynb, which steps 0.02 s per
 * solve against 10 ms knots).  Init, groups and rows, H in {1, ..., 256}, reset, solve, the select
 * and resample rule, the wrench left on the handle and the staggered ranges cut on a group boundary
 * are i7m_mpc_run_sampled's / i7m_mpc_run_tracking's.  The schedule of sub-steps and completed knots
 * is i7m_mpc_run_multirate's (computed on the host in the reference's double arithmetic, float
 * residues kept: dt 0.01, sim_dt 0.001 gives step 9 the sub-steps [0.001, 8.67e-19]).
 *   step i, every group still running:
 *     plant    x_last = xcur[g], u_last = XU_best[g][12:18], u_out[i, g] = u_last.  The actual
 *              wrench f_actual[i or 0][g], if world-frame, is converted to joint 6's frame ONCE, at
 *              x_last's q, and held over all of the step's sub-steps (:151-161).  Each sub-step s
 *              is one rk4 step of its length driven by u_last (the reference's current_knot is
 *              always 0: the accumulator is reset at every boundary).  xpath_out[s, g] = q after
 *              sub-step s, q_out[i, g] = q after the step's last.
 *     spread   shift_warm_start = 0: every row of g gets xs = xcur[g], XU = [xcur[g], XU_best[g][12:]].
 *              shift_warm_start = 1 and s = the knots this step completed > 0:
 *              XU[e] = XU_best[g][e + 18 s] for 12 <= e < T - 18 s, the tail keeps XU_best[g][e]
 *              (src/gato_mpc_batch.py:202-203).  No terminal pin.
 *     goal     (endpoints) as i7m_mpc_run_sampled: radius 0.095, the next endpoint or the stop,
 *              after the plant.  A group that stops at step i has dist / q / u / xpath of step i
 *              recorded, best_out[i] = -1 and fbest_out[i] NaN; from step i + 1 on dist, q, u,
 *              xpath and fbest are NaN and best is -1.
 *     track    (reference) the window's offset is off_i = the knots completed by steps 0 .. i, the
 *              notebook's eepos_offset; off_out[i] = off_i; err_out[i, g] = |eepos(xcur q) -
 *              ref[min(ph_g + off_i, L - 1)]|, ee_out[i, g], and the rows' window at ph_g + off_i,
 *              as i7m_mpc_run_tracking with ref_offset[i] = off_i.  A tracking group never stops.
 *     reset, solve   as the existing loops
 *     select   err_h = |rk4(x_last, u_last, sim_dt, wrench row h) - xcur[g]|_2: ONE rk4 step of the
 *              whole sim_dt, not split (:284, the notebook's sim_forward(x_last, u_last, sim_dt)),
 *              the hypothesis converted at x_last's q.  On a step with several sub-steps the true
 *              hypothesis therefore scores small but not 0: the reference's behaviour.  On a step
 *              with one sub-step plant and score are the same computation (the same conversion,
 *              then the same rk4 code), and a hypothesis equal to the actual wrench scores as in
 *              i7m_mpc_run_sampled.  The lowest index wins a tie, a NaN error never wins; then the
 *              resample.
 * opts->control_from = I7M_CONTROL_POLICY (ABI 12; the reference has no counterpart): behind every
 * solve, the initial one included, the policy pass of i7m_qp_policy runs on every row (the QP at
 * that solve's result with x_0 = the row's state and the row's own wrench: the resample comes
 * later, in the select), and plant and score of a step change:
 *     plant    sub-step s begins at plant state x with j = the knots this step has completed
 *              (i7m_multirate_knots) and is driven by u_s = XU_best[g].u_j + K_j (x - XU_best[g].x_j),
 *              K_j the gain of stage j of row g H + best (row 0 after the initial solve), K_j dx in
 *              the fixed order of i7m_mpc_run_multirate's policy plant.  u_out[i, g] stays
 *              XU_best[g][12:18], the nominal first control.
 *     select   the torque varies within the step, so hypothesis h is scored by REPLAYING the step:
 *              from x_last the same sub-steps of the same lengths under the recorded controls u_s
 *              (the plant's, not recomputed from the replayed state), wrench row h converted once at
 *              x_last's q; err_h = |replay - xcur[g]|_2.  Plant and replay are the same code: a
 *              hypothesis equal to the actual wrench scores exactly 0 on every step.
 * Refused in addition: a step that completes more than N - 2 knots (knot N - 1 has no control), with
 * i7m_mpc_run_multirate's text.  I7M_POLICY_ZERO_K=1 at i7m_create zeroes the gains here too.  The
 * single-rate entry points i7m_mpc_run_sampled / i7m_mpc_run_tracking have no such option.
 * Deliberately not reproduced: the actual force's random walk (:244-250; the caller supplies
 * f_actual); the notebook's use of the world force as a local one (its actInv is commented out);
 * np.random's global draw order.
 * Outputs: dist_out / err_out (num_steps, G) required; best_out (num_steps, G) int32; q_out, u_out,
 * fbest_out (num_steps, G, 6); xpath_out (n_sub, G, 6) with n_sub from i7m_multirate_substeps(dt,
 * sim_dt, N, num_steps); ee_out (num_steps, G, 3); off_out (num_steps) int32; xcur_out (G, 12),
 * xu_best_out (G, T), fhyp_out (G H, 6): each may be NULL.  num_steps = 0 reduces to the initial
 * solve.  Synchronous.  I7M_EINVAL with the argument named, before any device work: everything
 * i7m_mpc_run_sampled / i7m_mpc_run_tracking refuse except sim_dt > dt; sim_dt not finite or not
 * positive; a step of more than 66 sub-steps; a step that completes more than N - 1 knots;
 * shift_warm_start not 0 or 1; control_from other than I7M_CONTROL_NEW or I7M_CONTROL_POLICY; an
 * open controller session; I7M_QP_BOX. */
int i7m_mpc_run_sampled_multirate(i7m_handle* h, int32_t G, int32_t H, const double* xstart, const double* endpoints,
                                  int32_t n_endpoints, int32_t num_steps, const double* fhyp, const double* f_actual,
                                  const double* noise, const i7m_sampled_multirate_opts* opts,
                                  double* dist_out /* (steps,G) required */, int32_t* best_out, double* q_out,
                                  double* u_out /* (steps,G,6) */, double* xpath_out /* (n_sub,G,6) */,
                                  double* fbest_out, double* xcur_out, double* xu_best_out, double* fhyp_out);
int i7m_mpc_run_tracking_multirate(i7m_handle* h, int32_t G, int32_t H, const double* xstart, const double* ref,
                                   int32_t L, int32_t ref_stride, const int32_t* ref_phase, int32_t num_steps,
                                   const double* fhyp, const double* f_actual, const double* noise,
                                   const i7m_sampled_multirate_opts* opts, double* err_out /* (steps,G) required */,
                                   int32_t* best_out, double* q_out, double* u_out, double* xpath_out, double* ee_out,
                                   int32_t* off_out /* (steps) */, double* fbest_out, double* xcur_out,
                                   double* xu_best_out, double* fhyp_out);

/* A controller session: GATO_Controller itself (gato_controller.py:144-250), one control step per
 * call on a state MEASURED by the caller (a robot, a simulator), where i7m_mpc_run_tracking owns
 * the plant.  G controllers of H hypotheses, group g owning rows [g H, (g + 1) H) as there; the
 * session lives on a handle in I7M_QP_DIRECT or I7M_QP_ADMM mode, one at a time.
 *
 * i7m_ctrl_begin (:174-185) copies ref (L, ref_stride) and ref_phase (G, or NULL = 0) into device
 * memory of the handle, sets the rows' wrenches to fhyp (G H, 6) in opts->frame, starts the solver
 * state afresh, sets every row of group g to XU = [x0[g], 0...], xs = x0[g] and its goals to the
 * window at offset 0 (goals[k] = ref[min(ph_g + k, L - 1)][0:3]), solves once, sets XU_best[g] =
 * row g H and writes XU_best[g][12:18] to u_out (G, 6; may be NULL).  opts NULL = the defaults; its
 * sim_dt and n_actual are ignored.  x0 has two forms:
 *   x0 (G, 12)  the session remembers x_last[g] = x0[g], u_last[g] = that u_out, which the caller
 *               applies to its plant: i7m_mpc_run_tracking's start;
 *   x0 NULL     the controller's constructor: the rows start at the zero state (:181-183) and
 *               x_last is unset; the first step sets x_last = x_meas, u_last = 0 before it scores
 *               (:205-206): each hypothesis is then scored by the change of state it predicts
 *               over `elapsed` under zero torque, not against a control that was applied.
 *
 * i7m_ctrl_step (:213-250), x_meas (G, 12) the measured states, `elapsed` the time since the
 * state x_last was measured (one clock for all groups; finite, > 0, not bounded by dt: it is the
 * scoring step, not a knot), ref_offset >= 0 the window's offset (the controller's is
 * int(sum of elapsed / dt)):
 *   window   every row of g: goals[k] = ref[min(ph_g + ref_offset + k, L - 1)][0:3]
 *   spread   every row of g: xs = x_meas[g], XU = [x_meas[g], XU_best[g][12:]] (:217-218,249)
 *   track    ee_out[g] = eepos(x_meas[g] q) (the model's FK; the controller reads it from the
 *            simulator's message), err_out[g] = |ee - window[0]| (:242)
 *   score    err_h = |rk4(x_last[g], u_last[g], elapsed, wrench row h) - x_meas[g]|_2 over all 12
 *            entries: one rk4 step of length elapsed, a world wrench converted once at x_last's q
 *            as i7m_rk4 does, the hypotheses those before this step's resample (:225); best = the
 *            lowest index among the minima (a NaN error never wins, all NaN -> 0), where the
 *            controller's `<=` (:115) takes the highest: tied rows are identical hypotheses
 *   reset    I7M_QP_ADMM: opts->reset_what on every row (default ALL, :221-223)
 *   solve    XU_new = sqp(rows)
 *   select   best_out[g] = best, fbest_out[g] = wrench row best, XU_best[g] = XU_new[g H + best],
 *            u_out[g] = XU_best[g][12:18]
 *   resample only with noise (G H, 3), by gato_controller.py:120-129's order with opts->keep_best
 *            and opts->decay, as i7m_mpc_run_sampled does it
 *   remember x_last = x_meas, u_last = u_out
 * The scoring uses no result of the solve and runs before it.  u_out (G, 6) is required; best_out
 * (G) int32, fbest_out (G, 6), err_out (G), ee_out (G, 3) may be NULL.  A step allocates nothing:
 * everything it needs, pinned host staging included, is allocated by i7m_ctrl_begin.  It runs as
 * ONE range on the handle's stream (a session gets no two-stream stagger, whatever G H is), ends
 * with one device-to-host copy (two with the policy on, below) and one synchronisation, and
 * captures no graph.
 *
 * The winner's feedback policy (ABI 12).  A torque loop that runs faster than the solver has one
 * torque vector per step to apply; the session can hand out the time-varying gains of the winning
 * row so that it applies u_k + K_k (x - x_k) between solves instead.
 *   i7m_ctrl_set_policy(h, n_k)   n_k in [0, N - 1]; 0 is off, the state after i7m_ctrl_begin.
 *            Allocates a device buffer (G, n_k, 96) and pinned staging of that size, recorded on the
 *            session and freed by i7m_ctrl_end / i7m_destroy (a step still allocates nothing).  With
 *            the policy on, a step runs the policy pass of i7m_qp_policy over all G H rows behind
 *            its solve and before the select (the rows' wrenches are still the solve's), and after
 *            the select one small launch copies, for k < n_k, K~_k of row g H + best and
 *            XU_best[g][18 k : 18 k + 18] into that buffer; the step then ends with two
 *            device-to-host copies and still one synchronisation.  Off, the step is what it was,
 *            launch for launch.
 *   i7m_ctrl_get_policy(h, K_out (G, n_k, 6, 13), xu_ref_out (G, n_k, 18))   a host copy from the
 *            staging of the last step; either pointer may be NULL.  K_out as i7m_qp_policy's
 *            ([K_k | kff_k]); xu_ref_out[g, k] = [x_k (12), u_k (6)].  Refused with the policy off or
 *            when no step has run since it was turned on.
 *   i7m_ctrl_set_applied(h, u_applied (G, 6))   a caller that applies the feedback itself reports
 *            the time-average torque it applied since the last measurement; it replaces u_last for
 *            the NEXT step's scoring only (that step's select stores its own control again).
 *            Without it the feedback torque that fights the unknown force is invisible to the
 *            estimator.  Entries finite; refused before a step or an x0 has set x_last.  One small
 *            host-to-device copy on the handle's stream.
 * All three: I7M_EINVAL with the argument named, before any device work, without an open session
 * or on a bad argument.  Box-mode gains are out of scope (the session refuses I7M_QP_BOX).
 *
 * i7m_ctrl_end copies out the final XU_best (G, T) and hypotheses (G H, 6) (each may be NULL) and
 * closes the session; the final hypotheses stay the handle's external wrench in opts->frame, as
 * after i7m_mpc_run_tracking.  i7m_destroy on a handle with an open session frees it.
 *
 * I7M_EINVAL with a message naming the argument, before any device work: an I7M_QP_BOX handle; H
 * not in {1, 2, 4, ..., 256}; G H outside [0, max_batch]; L < 1; ref_stride other than 3 or 6; a
 * negative ref_phase entry; a bad frame or reset_what; null ref, fhyp, x_meas or u_out (of a step);
 * i7m_ctrl_begin while a session is open; i7m_ctrl_step / i7m_ctrl_end without one; a non-finite or
 * non-positive elapsed; a negative ref_offset; a non-finite entry of x_meas (a host scan of 12 G
 * doubles: a sensor fault must not poison the carried warm start).  A refused step leaves the
 * session as it was.
 * While a session is open the entry points that would overwrite its rows, goals, wrenches or
 * solver state are refused ("controller session open"): i7m_solve, i7m_solve_device, i7m_qp,
 * i7m_qp_value, i7m_qp_policy, i7m_linearize, i7m_merit, i7m_linesearch, the six i7m_mpc_run*,
 * i7m_set_external_wrench, i7m_reset, i7m_admm_reset, i7m_set_stream.  The getters, the timing
 * calls, i7m_synchronize, i7m_ctrl_set_policy / i7m_ctrl_get_policy / i7m_ctrl_set_applied and the
 * query hooks (i7m_eepos, i7m_aba, i7m_aba_derivatives, i7m_rk4: they use scratch the session does
 * not rely on between steps) stay available. */
int i7m_ctrl_begin(i7m_handle* h, int32_t G, int32_t H, const double* x0 /* (G,12) or NULL */, const double* ref,
                   int32_t L, int32_t ref_stride, const int32_t* ref_phase /* (G) or NULL */,
                   const double* fhyp /* (G H,6) */, const i7m_sampled_opts* opts, double* u_out /* (G,6) or NULL */);
int i7m_ctrl_step(i7m_handle* h, const double* x_meas /* (G,12) */, double elapsed, int32_t ref_offset,
                  const double* noise /* (G H,3) or NULL */, double* u_out /* (G,6) */, int32_t* best_out /* (G) */,
                  double* fbest_out /* (G,6) */, double* err_out /* (G) */, double* ee_out /* (G,3) */);
int i7m_ctrl_end(i7m_handle* h, double* xu_best_out /* (G,T) or NULL */, double* fhyp_out /* (G H,6) or NULL */);
int i7m_ctrl_set_policy(i7m_handle* h, int32_t n_k);
int i7m_ctrl_get_policy(i7m_handle* h, double* K_out /* (G,n_k,6,13) or NULL */, double* xu_ref_out /* (G,n_k,18) or NULL */);
int i7m_ctrl_set_applied(i7m_handle* h, const double* u_applied /* (G,6) */);

/* Per-kernel device timing with HIP events on the launch stream. */
enum { I7M_K_LIN = 0, I7M_K_RICCATI = 1, I7M_K_LINESEARCH = 2, I7M_K_RICCATI_BOX = 3, I7M_K_IPM = 4, I7M_K_IPM_FUSED = 5,
       I7M_K_SQP_FUSED = 6, I7M_K_LINESEARCH_TAIL = 7 /* second launch of a split line search */, I7M_K_ADMM = 8 /* OSQP iterations */,
       I7M_K_ADMM_PREP = 9 /* the QP's scaling and factor */, I7M_K_COUNT = 10 };
int i7m_set_timing(i7m_handle* h, int enable);
/* Sums (ms) and launch counts per kernel id since the last reset; synchronises. */
int i7m_get_kernel_times(i7m_handle* h, double* ms_sum, int32_t* counts, int32_t n);
int i7m_reset_kernel_times(i7m_handle* h);

#ifdef __cplusplus
}
#endif

#endif /* INDY7_MPC_H */
