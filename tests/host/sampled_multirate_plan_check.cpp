// Host check of the multi-rate sampled-wrench loops' plan (indy7_mpc_amd/csrc/i7m_plan.h):
// sampled_multirate_call_ok and its texts (everything the family's check refuses but sim_dt > dt,
// the schedule's refusals, shift_warm_start), sampled_call_ok unchanged for the single-rate kinds,
// multirate_offsets, sampled_multirate_ws_bytes, and the loops' one request, sampled_call_ws_bytes.
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
  c.o.sim_dt = 0.02;
  c.o.decay = 1.0;
  c.o.frame = I7M_WRENCH_WORLD;
  c.o.reset_what = I7M_ADMM_RESET_ALL;
  c.o.keep_best = 0;
  c.o.n_actual = 1;
  const bool track = kind != SampledKind::endpoints && kind != SampledKind::endpoints_multirate;
  c.goal = track ? GoalSource::of_reference(REF, 10, 6, nullptr, nullptr) : GoalSource::of_endpoints(EP, 2);
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
  for (SampledKind kind : {SampledKind::endpoints_multirate, SampledKind::tracking_multirate}) {
    const bool track = kind == SampledKind::tracking_multirate;
    MultirateSchedule s;
    const char* which = "";
    long at = -1;
    SampledCall c = good(kind);
    CHECK(sampled_multirate_call_ok(c, 8, &s, &which, &at));
    CHECK(s.total() == 6 && s.shift == (std::vector<int32_t>{2, 2, 2}));
    // sim_dt below dt, equal to it and far above it all pass; no ref_offset is asked for
    for (double v : {0.001, 0.01, 0.011, 0.025, 0.07}) {
      c.o.sim_dt = v;
      CHECK(sampled_multirate_call_ok(c, 8, &s, &which, &at));
    }
    c.num_steps = 0;
    CHECK(sampled_multirate_call_ok(c, 8, &s, &which, &at) && s.total() == 0 && s.sub_start.size() == 1);
    // the schedule's refusals
    for (double v : {0.0, -0.02, inf, -inf, nan}) {
      c = good(kind);
      c.o.sim_dt = v;
      CHECK(refused(c, 8, "sim_dt", 0));
    }
    c = good(kind);
    c.o.sim_dt = 0.08;
    CHECK(refused(c, 8, "shift", 0));
    c.o.sim_dt = 0.025;
    CHECK(refused(c, 3, "shift", 1));
    c.o.sim_dt = 0.661;
    CHECK(refused(c, 64, "substeps", 0));
    // shift_warm_start
    c = good(kind);
    c.shift_warm_start = 1;
    CHECK(sampled_multirate_call_ok(c, 8, &s, &which, &at));
    for (int v : {-1, 2, 7}) {
      c.shift_warm_start = v;
      CHECK(refused(c, 8, "shift_warm_start", v));
    }
    // the family's refusals
    c = good(kind);
    c.qp_mode = I7M_QP_BOX;
    CHECK(refused(c, 8, "qp_mode", I7M_QP_BOX));
    for (int H : {0, 3, 512}) {
      c = good(kind);
      c.H = H;
      CHECK(refused(c, 8, "H", H));
    }
    c = good(kind);
    c.G = 3;
    CHECK(refused(c, 8, "G", 12));
    c = good(kind);
    c.G = -1;
    CHECK(refused(c, 8, "G", -4));
    c = good(kind);
    c.o.frame = 2;
    CHECK(refused(c, 8, "frame", 2));
    c = good(kind);
    c.o.reset_what = 8;
    CHECK(refused(c, 8, "reset_what", 8));
    c = good(kind);
    c.num_steps = -1;
    CHECK(refused(c, 8, "num_steps", -1));
    c = good(kind);
    c.o.n_actual = 2;
    CHECK(refused(c, 8, "n_actual", 2));
    c.o.n_actual = 3;  // = num_steps
    CHECK(sampled_multirate_call_ok(c, 8, &s, &which, &at));
    c = good(kind);
    c.xstart = nullptr;
    CHECK(refused(c, 8, "xstart", 0));
    c = good(kind);
    c.fhyp = nullptr;
    CHECK(refused(c, 8, "fhyp", 0));
    c = good(kind);
    c.f_actual = nullptr;
    CHECK(refused(c, 8, "f_actual", 0));
    c = good(kind);
    c.hist_out = nullptr;
    CHECK(refused(c, 8, track ? "err_out" : "dist_out", 0));
    if (track) {
      c = good(kind);
      c.goal.L = 0;
      CHECK(refused(c, 8, "L", 0));
      c = good(kind);
      c.goal.ref_stride = 4;
      CHECK(refused(c, 8, "ref_stride", 4));
      c = good(kind);
      c.goal.ref = nullptr;
      CHECK(refused(c, 8, "ref", 0));
      const int32_t ph[2] = {3, -1};
      c = good(kind);
      c.goal.ref_phase = ph;
      CHECK(refused(c, 8, "ref_phase", 1));
    } else {
      c = good(kind);
      c.goal.n_endpoints = 0;
      CHECK(refused(c, 8, "n_endpoints", 0));
      c = good(kind);
      c.goal.endpoints = nullptr;
      CHECK(refused(c, 8, "endpoints", 0));
    }
  }
  // a single-rate kind is not a multi-rate call
  CHECK(refused(good(SampledKind::endpoints), 8, "kind", (long)SampledKind::endpoints));

  // sampled_call_ok for the existing kinds is what it was: sim_dt > dt refused, shift_warm_start
  // not looked at, a tracking loop still needs its ref_offset
  {
    const char* which = "";
    long at = -1;
    SampledCall c = good(SampledKind::endpoints);
    CHECK(!sampled_call_ok(c, &which, &at) && std::string(which) == "sim_dt");
    c.o.sim_dt = 0.01;
    c.shift_warm_start = 5;
    CHECK(sampled_call_ok(c, &which, &at));
    c = good(SampledKind::tracking);
    c.o.sim_dt = 0.011;
    CHECK(!sampled_call_ok(c, &which, &at) && std::string(which) == "sim_dt");
    c.o.sim_dt = 0.01;
    CHECK(!sampled_call_ok(c, &which, &at) && std::string(which) == "ref_offset" && at == -1);
    const int32_t ro[3] = {1, 2, -3};
    c.goal.ref_offset = ro;
    CHECK(!sampled_call_ok(c, &which, &at) && std::string(which) == "ref_offset" && at == 2);
    c = good(SampledKind::session);
    c.o.sim_dt = 5.0;  // a session reads no sim_dt
    CHECK(sampled_call_ok(c, &which, &at));
  }

  // the texts
  const SampledCall c = good(SampledKind::endpoints_multirate);
  CHECK(sampled_multirate_refusal("f", "sim_dt", 0, c, 8) == "f: sim_dt must be finite and > 0");
  CHECK(sampled_multirate_refusal("f", "shift", 1, c, 8).find("more than N - 1 = 7 knots in step 1") != std::string::npos);
  CHECK(sampled_multirate_refusal("f", "substeps", 0, c, 8).find("MULTIRATE_MAX_SUB = 66") != std::string::npos);
  CHECK(sampled_multirate_refusal("f", "shift_warm_start", 2, c, 8) == "f: shift_warm_start = 2 is not 0 or 1");
  CHECK(sampled_multirate_refusal("f", "qp_mode", 1, c, 8) == sampled_refusal("f", "qp_mode", 1, 8));
  CHECK(sampled_multirate_refusal("f", "G", 12, c, 8) == sampled_refusal("f", "G", 12, 8));
  CHECK(sampled_multirate_refusal("f", "dist_out", 0, c, 8) == "f: null dist_out");

  // the offsets: the knots completed by steps 0 .. i
  {
    MultirateSchedule s;
    const char* which = "";
    long at = -1;
    CHECK(multirate_schedule(0.01, 0.025, 8, 3, &s, &which, &at));
    CHECK(multirate_offsets(s) == (std::vector<int32_t>{2, 5, 7}));
    CHECK(multirate_schedule(0.01, 0.001, 8, 12, &s, &which, &at));
    CHECK(multirate_offsets(s) == (std::vector<int32_t>{0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1}));
    CHECK(multirate_schedule(0.01, 0.02, 8, 0, &s, &which, &at));
    CHECK(multirate_offsets(s).empty());
  }

  // the workspace: the tracking request's sub-buffers unchanged, then u, the path and the lengths
  {
    size_t by[SAMPLED_MULTIRATE_WS_COUNT], tr[TRACKING_WS_COUNT], off[SAMPLED_MULTIRATE_WS_COUNT];
    sampled_multirate_ws_bytes(5, 4, 8, 10, 23, 2, 1, true, 50, 6, true, by);
    tracking_ws_bytes(5, 4, 8, 10, 2, 1, true, 50, 6, true, tr);
    for (int i = 0; i < TRACKING_WS_COUNT; ++i) CHECK(by[i] == tr[i]);
    CHECK(by[SMWS_U] == 48 * 50 && by[SMWS_XPATH] == 48 * 23 * 5 && by[SMWS_SUBDT] == 8 * 23);
    const size_t total = carve(by, SAMPLED_MULTIRATE_WS_COUNT, off);
    for (int i = 0; i < SAMPLED_MULTIRATE_WS_COUNT; ++i) {
      CHECK(off[i] % WS_ALIGN == 0);
      CHECK(off[i] + by[i] <= (i + 1 < SAMPLED_MULTIRATE_WS_COUNT ? off[i + 1] : total));
    }
    sampled_multirate_ws_bytes(3, 2, 8, 0, 0, 1, 1, false, 0, 0, false, by);  // no steps: one row of each
    CHECK(by[SMWS_U] == 144 && by[SMWS_XPATH] == 144 && by[SMWS_SUBDT] == 8 && by[TWS_REF] == 0);
  }

  // the loops' one request (sampled_call_ws_bytes): a single-rate kind's offsets and total are
  // tracking_ws_bytes', a multi-rate kind's sampled_multirate_ws_bytes'; without noise, phases or a
  // reference those sub-buffers take no room, and a single-rate call's multi-rate ones never do
  {
    const int32_t ph[5] = {0, 1, 2, 3, 4};
    const int N = 8, n_sub = 23;
    for (SampledKind kind : {SampledKind::endpoints, SampledKind::tracking, SampledKind::endpoints_multirate,
                             SampledKind::tracking_multirate})
      for (int variant = 0; variant < 8; ++variant) {
        const bool multi = multirate_kind(kind), track = tracking_kind(kind);
        const bool noise = variant & 1, phase = track && (variant & 2), steps = variant & 4;
        SampledCall c = good(kind);
        c.G = 5;
        c.num_steps = steps ? 10 : 0;
        c.o.n_actual = steps ? 10 : 1;
        c.goal.n_endpoints = track ? 0 : 3;
        c.goal.L = track ? 50 : 0;
        c.goal.ref_phase = phase ? ph : nullptr;
        size_t by[SAMPLED_MULTIRATE_WS_COUNT], off[SAMPLED_MULTIRATE_WS_COUNT], want[SAMPLED_MULTIRATE_WS_COUNT],
            want_off[SAMPLED_MULTIRATE_WS_COUNT];
        sampled_call_ws_bytes(c, N, multi && steps ? n_sub : 0, noise, by);
        const size_t total = carve(by, SAMPLED_MULTIRATE_WS_COUNT, off);
        size_t want_total;
        if (multi) {
          sampled_multirate_ws_bytes(c.G, c.H, N, c.num_steps, steps ? n_sub : 0, c.goal.n_endpoints, c.o.n_actual, noise,
                                     c.goal.L, c.goal.ref_stride, phase, want);
          want_total = carve(want, SAMPLED_MULTIRATE_WS_COUNT, want_off);
          for (int i = 0; i < SAMPLED_MULTIRATE_WS_COUNT; ++i) CHECK(by[i] == want[i] && off[i] == want_off[i]);
        } else {
          tracking_ws_bytes(c.G, c.H, N, c.num_steps, c.goal.n_endpoints, c.o.n_actual, noise, c.goal.L,
                            c.goal.ref_stride, phase, want);
          want_total = carve(want, TRACKING_WS_COUNT, want_off);
          for (int i = 0; i < TRACKING_WS_COUNT; ++i) CHECK(by[i] == want[i] && off[i] == want_off[i]);
          // max(n_sub, 1) lengths and history_rows of u and the path do not leak into this call
          for (int i : {(int)SMWS_U, (int)SMWS_XPATH, (int)SMWS_SUBDT}) CHECK(by[i] == 0 && off[i] == total);
        }
        CHECK(total == want_total);
        CHECK((by[SWS_NOISE] != 0) == (noise && steps));  // (no steps: no noise rows either)
        CHECK((by[TWS_PHASE] != 0) == phase);
        CHECK((by[TWS_REF] != 0) == track && (by[TWS_EE] != 0) == track);
        for (int i : {(int)SWS_NOISE, (int)TWS_REF, (int)TWS_PHASE, (int)TWS_EE})
          if (by[i] == 0) CHECK(off[i + 1] == off[i]);  // (none of them is the last sub-buffer)
      }
  }

  if (bad) return 1;
  std::printf("sampled_multirate_plan_check OK\n");
  return 0;
}
