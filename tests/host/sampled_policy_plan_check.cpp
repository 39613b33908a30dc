// Host check of the feedback policy's plan (indy7_mpc_amd/csrc/i7m_plan.h): the control_from check of
// the sampled-wrench family (sampled_call_ok) and its refusal text, the N - 2 bound of a policy-driven
// multi-rate call (sampled_multirate_call_ok, multirate_policy_refusal's text), and the argument
// checks and texts of the controller session's three policy calls (ctrl_set_policy_ok,
// ctrl_get_policy_ok, ctrl_set_applied_ok, ctrl_policy_refusal).
#include <cstdio>
#include <limits>

#include "../../indy7_mpc_amd/csrc/i7m_plan.h"

using namespace i7m;

static int bad = 0;
#define CHECK(c)                                      \
  do {                                                \
    if (!(c)) {                                       \
      std::printf("line %d: %s\n", __LINE__, #c);     \
      ++bad;                                          \
    }                                                 \
  } while (0)

static const double X[24] = {0}, EP[6] = {0}, REF[60] = {0}, F[48] = {0};
static double OUT[8];

// a call every check passes: G = 2, H = 4, 3 steps of 0.02 s against 10 ms knots
static SampledCall good(SampledKind kind) {
  SampledCall c;
  c.kind = kind;
  c.qp_mode = I7M_QP_ADMM;
  c.max_batch = 8;
  c.dt = 0.01;
  c.G = 2;
  c.H = 4;
  c.num_steps = 3;
  c.o.sim_dt = kind == SampledKind::endpoints || kind == SampledKind::tracking ? 0.01 : 0.02;
  c.o.decay = 1.0;
  c.o.frame = I7M_WRENCH_WORLD;
  c.o.reset_what = I7M_ADMM_RESET_ALL;
  c.o.keep_best = 0;
  c.o.n_actual = 1;
  static const int32_t offs[3] = {1, 2, 3};
  const bool track = kind != SampledKind::endpoints && kind != SampledKind::endpoints_multirate;
  c.goal = track ? GoalSource::of_reference(REF, 10, 6, nullptr, offs) : GoalSource::of_endpoints(EP, 2);
  c.xstart = X;
  c.fhyp = F;
  c.f_actual = F;
  c.hist_out = OUT;
  return c;
}

static bool refused(const SampledCall& c, int N, const char* want, long want_at) {
  MultirateSchedule s;
  const char* which = "";
  long at = -99;
  if (sampled_multirate_call_ok(c, N, &s, &which, &at)) return false;
  if (std::string(which) != want || at != want_at) {
    std::printf("refused for %s at %ld, expected %s at %ld\n", which, at, want, want_at);
    return false;
  }
  return s.total() == 0 && s.sub_dt.empty();
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const char* which = "";
  long at = -99;
  // a default-constructed call carries I7M_CONTROL_NEW
  CHECK(SampledCall{}.control_from == I7M_CONTROL_NEW);
  // ---- control_from: the multi-rate kinds take NEW and POLICY ------------------------------------
  for (SampledKind kind : {SampledKind::endpoints_multirate, SampledKind::tracking_multirate}) {
    MultirateSchedule s;
    SampledCall c = good(kind);
    CHECK(sampled_multirate_call_ok(c, 8, &s, &which, &at) && s.total() == 6);
    c.control_from = I7M_CONTROL_POLICY;
    CHECK(sampled_multirate_call_ok(c, 8, &s, &which, &at) && s.total() == 6);
    CHECK(s.sub_knot == (std::vector<int32_t>{0, 1, 0, 1, 0, 1}));
    for (int v : {I7M_CONTROL_PREV, -1, 3, 7}) {
      c.control_from = v;
      CHECK(refused(c, 8, "control_from", v));
    }
    CHECK(sampled_multirate_refusal("mpc_run_x", "control_from", I7M_CONTROL_PREV, c, 8) ==
          "mpc_run_x: control_from = 1 is not I7M_CONTROL_NEW (0) or, for a multi-rate loop, I7M_CONTROL_POLICY (2)");
    // an earlier refusal keeps its place: a bad shift_warm_start is named first
    c.shift_warm_start = 2;
    CHECK(refused(c, 8, "shift_warm_start", 2));
    // ---- the N - 2 bound: 7 knots per step at N = 8 run under NEW, not under POLICY ---------------
    c = good(kind);
    c.o.sim_dt = 0.07;
    CHECK(sampled_multirate_call_ok(c, 8, &s, &which, &at) && s.shift == (std::vector<int32_t>{7, 7, 7}));
    c.control_from = I7M_CONTROL_POLICY;
    CHECK(refused(c, 8, "policy_shift", 0));
    CHECK(sampled_multirate_refusal("mpc_run_x", "policy_shift", 0, c, 8) == multirate_policy_refusal("mpc_run_x", 0, 0.07, 8));
    CHECK(sampled_multirate_refusal("mpc_run_x", "policy_shift", 0, c, 8) ==
          "mpc_run_x: sim_dt = 0.070000 completes more than N - 2 = 6 knots in step 0 (control_from = I7M_CONTROL_POLICY: knot "
          "N - 1 has no control)");
    c.o.sim_dt = 0.06;
    CHECK(sampled_multirate_call_ok(c, 8, &s, &which, &at) && s.shift == (std::vector<int32_t>{6, 6, 6}));
    // the first step over the bound is named: 0.025 s completes 2, 3, 2 knots, and N = 4 allows 2
    c.o.sim_dt = 0.025;
    CHECK(refused(c, 4, "policy_shift", 1));
    c.control_from = I7M_CONTROL_NEW;
    CHECK(sampled_multirate_call_ok(c, 4, &s, &which, &at));
    // the schedule's own refusals come before the policy's
    c.control_from = I7M_CONTROL_POLICY;
    c.o.sim_dt = 0.08;
    CHECK(refused(c, 8, "shift", 0));
    c.o.sim_dt = nan;
    CHECK(refused(c, 8, "sim_dt", 0));
    c.o.sim_dt = inf;
    CHECK(refused(c, 8, "sim_dt", 0));
    c = good(kind);
    c.control_from = I7M_CONTROL_POLICY;
    c.num_steps = 0;
    CHECK(sampled_multirate_call_ok(c, 8, &s, &which, &at) && s.total() == 0);
  }
  // ---- the single-rate kinds and the session have no such option: anything but NEW is refused -----
  for (SampledKind kind : {SampledKind::endpoints, SampledKind::tracking, SampledKind::session}) {
    SampledCall c = good(kind);
    CHECK(sampled_call_ok(c, &which, &at));
    for (int v : {I7M_CONTROL_PREV, I7M_CONTROL_POLICY, -1}) {
      c.control_from = v;
      which = "";
      at = -99;
      CHECK(!sampled_call_ok(c, &which, &at) && std::string(which) == "control_from" && at == v);
    }
    CHECK(sampled_refusal("mpc_run_sampled", "control_from", 2, 8) ==
          "mpc_run_sampled: control_from = 2 is not I7M_CONTROL_NEW (0) or, for a multi-rate loop, I7M_CONTROL_POLICY (2)");
  }
  // ---- i7m_ctrl_set_policy -------------------------------------------------------------------------
  for (int n_k : {0, 1, 6, 7}) CHECK(ctrl_set_policy_ok(true, n_k, 8, &which, &at));
  for (int n_k : {-1, 8, 64}) {
    CHECK(!ctrl_set_policy_ok(true, n_k, 8, &which, &at) && std::string(which) == "n_k" && at == n_k);
  }
  CHECK(!ctrl_set_policy_ok(false, 3, 8, &which, &at) && std::string(which) == "session");
  CHECK(ctrl_policy_refusal("ctrl_set_policy", "n_k", 8, 8) == "ctrl_set_policy: n_k = 8 outside [0, N - 1 = 7]");
  CHECK(ctrl_policy_refusal("ctrl_set_policy", "session", 0, 8) ==
        "ctrl_set_policy: no controller session is open on this handle (i7m_ctrl_begin)");
  // ---- i7m_ctrl_get_policy -------------------------------------------------------------------------
  CHECK(ctrl_get_policy_ok(true, true, true, &which, &at));
  CHECK(!ctrl_get_policy_ok(false, true, true, &which, &at) && std::string(which) == "session");
  CHECK(!ctrl_get_policy_ok(true, false, false, &which, &at) && std::string(which) == "off");
  CHECK(!ctrl_get_policy_ok(true, false, true, &which, &at) && std::string(which) == "off");
  CHECK(!ctrl_get_policy_ok(true, true, false, &which, &at) && std::string(which) == "step");
  CHECK(ctrl_policy_refusal("ctrl_get_policy", "off", 0, 8) ==
        "ctrl_get_policy: the session's policy is off (i7m_ctrl_set_policy with n_k > 0)");
  CHECK(ctrl_policy_refusal("ctrl_get_policy", "step", 0, 8) ==
        "ctrl_get_policy: no i7m_ctrl_step has run since the policy was turned on");
  // ---- i7m_ctrl_set_applied: the scan reads 6 G entries, no more -----------------------------------
  {
    std::vector<double> u(12, 0.5);  // G = 2, exactly (the sanitized build sees a read past it)
    CHECK(ctrl_set_applied_ok(true, true, u.data(), 2, &which, &at));
    CHECK(ctrl_set_applied_ok(true, true, u.data(), 0, &which, &at));
    CHECK(!ctrl_set_applied_ok(false, true, u.data(), 2, &which, &at) && std::string(which) == "session");
    CHECK(!ctrl_set_applied_ok(true, true, nullptr, 2, &which, &at) && std::string(which) == "u_applied" && at == -1);
    CHECK(!ctrl_set_applied_ok(true, false, u.data(), 2, &which, &at) && std::string(which) == "x_last");
    for (double v : {nan, inf, -inf}) {
      u[11] = v;
      CHECK(!ctrl_set_applied_ok(true, true, u.data(), 2, &which, &at) && std::string(which) == "u_applied" && at == 11);
      u[11] = 0.5;
    }
    u[7] = nan;
    CHECK(ctrl_set_applied_ok(true, true, u.data(), 1, &which, &at));  // entry 7 is group 1's
    CHECK(ctrl_policy_refusal("ctrl_set_applied", "u_applied", 11, 8) == "ctrl_set_applied: u_applied[11] is not finite");
    CHECK(ctrl_policy_refusal("ctrl_set_applied", "u_applied", -1, 8) == "ctrl_set_applied: null u_applied");
    CHECK(ctrl_policy_refusal("ctrl_set_applied", "x_last", 0, 8).find("no x_last yet") != std::string::npos);
  }
  static_assert(CTRL_POLICY_STAGE == 96, "the session's policy record");
  if (bad) return 1;
  std::printf("sampled_policy_plan_check OK\n");
  return 0;
}
