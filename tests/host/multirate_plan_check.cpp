// Host check of the multi-rate loop's plan (indy7_mpc_amd/csrc/i7m_plan.h): multirate_schedule
// against three schedules written out element for element, float residues included (the values
// are what the reference's while-loop, src/gato_mpc_batch.py:171-199, gives in double arithmetic),
// sub_start monotone, the refusals and their texts, and multirate_ws_bytes.
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

static void expect(double dt, double sim_dt, int N, const std::vector<int32_t>& sub_start, const std::vector<double>& sub_dt,
                   const std::vector<int32_t>& shift) {
  MultirateSchedule s;
  const char* which = "";
  long at = -1;
  CHECK(multirate_schedule(dt, sim_dt, N, (int)shift.size(), &s, &which, &at));
  CHECK(s.sub_start == sub_start);
  CHECK(s.shift == shift);
  CHECK(s.sub_dt.size() == sub_dt.size());
  for (size_t k = 0; k < sub_dt.size() && k < s.sub_dt.size(); ++k)
    if (s.sub_dt[k] != sub_dt[k]) {  // bit for bit: the residues are the behaviour
      std::printf("dt %g sim_dt %g: sub_dt[%zu] = %.17g, expected %.17g\n", dt, sim_dt, k, s.sub_dt[k], sub_dt[k]);
      ++bad;
    }
  CHECK(s.total() == (int)sub_dt.size());
}

static bool refused(double dt, double sim_dt, int N, int steps, const char* want, long want_at) {
  MultirateSchedule s;
  const char* which = "";
  long at = -1;
  if (multirate_schedule(dt, sim_dt, N, steps, &s, &which, &at)) return false;
  return std::string(which) == want && at == want_at && s.sub_start.empty() && s.sub_dt.empty() && s.shift.empty() &&
         s.total() == 0;
}

int main() {
  // ten solves per knot: nine steps without a shift, the tenth in two pieces, the second a residue
  expect(0.01, 0.001, 8, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11},
         {0.001, 0.001, 0.001, 0.001, 0.001, 0.001, 0.001, 0.001, 0.001, 0.0009999999999999992, 8.673617379884035e-19},
         {0, 0, 0, 0, 0, 0, 0, 0, 0, 1});
  // two and a half knots per solve: shifts of 2 and 3, the accumulator carried into the second step
  expect(0.01, 0.025, 8, {0, 3, 7},
         {0.01, 0.01, 0.005000000000000001, 0.004999999999999999, 0.01, 0.01, 3.469446951953614e-18}, {2, 3});
  // a knot grid other than 0.01
  expect(0.015, 0.02, 8, {0, 2, 4, 7, 9, 11},
         {0.015, 0.005000000000000001, 0.009999999999999998, 0.010000000000000002, 0.0049999999999999975, 0.015,
          3.469446951953614e-18, 0.014999999999999996, 0.0050000000000000044, 0.009999999999999995,
          0.010000000000000005},
         {1, 1, 2, 1, 1});
  // MPC_GATO's: two whole knots per solve, no residue
  expect(0.01, 0.02, 16, {0, 2, 4, 6}, {0.01, 0.01, 0.01, 0.01, 0.01, 0.01}, {2, 2, 2});
  // no steps: one offset, nothing else
  expect(0.01, 0.001, 8, {0}, {}, {});

  // sub_start strictly increasing (every step has at least one sub-step), every length in (0, dt],
  // the lengths of a step summing to sim_dt within rounding, the shifts to the knots passed
  for (double dt : {0.01, 0.015, 0.003})
    for (double sim_dt : {0.001, 0.004, 0.0123, 0.02, 0.025, 0.1}) {
      MultirateSchedule s;
      const char* which = "";
      long at = -1;
      const int steps = 200;
      CHECK(multirate_schedule(dt, sim_dt, 64, steps, &s, &which, &at));
      CHECK((int)s.sub_start.size() == steps + 1 && (int)s.shift.size() == steps && s.sub_start[0] == 0);
      long knots = 0;
      for (int i = 0; i < steps && i + 1 < (int)s.sub_start.size(); ++i) {
        CHECK(s.sub_start[i + 1] > s.sub_start[i]);
        CHECK(s.sub_start[i + 1] - s.sub_start[i] <= MULTIRATE_MAX_SUB);
        double sum = 0.0;
        for (int k = s.sub_start[i]; k < s.sub_start[i + 1]; ++k) {
          CHECK(s.sub_dt[k] > 0.0 && s.sub_dt[k] <= dt);
          sum += s.sub_dt[k];
        }
        CHECK(std::fabs(sum - sim_dt) < 1e-12);
        knots += s.shift[i];
      }
      CHECK(std::fabs((double)knots - steps * sim_dt / dt) <= 1.0);
    }

  // the refusals: which argument, which step, and the schedule left empty
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (double v : {0.0, -0.001, inf, -inf, nan}) CHECK(refused(0.01, v, 8, 3, "sim_dt", 0));
  CHECK(refused(0.01, 0.2, 8, 3, "shift", 0));      // 20 knots in a step at N = 8
  CHECK(refused(0.01, 0.025, 3, 4, "shift", 1));    // shifts 2, 3: the second passes N - 1 = 2
  CHECK(!refused(0.01, 0.07, 8, 3, "shift", 0));    // 7 = N - 1 knots is the most that fits
  CHECK(refused(0.01, 0.08, 8, 3, "shift", 0));
  CHECK(refused(0.01, 0.661, 64, 2, "substeps", 0));  // 67 sub-steps
  CHECK(refused(1e-300, 0.01, 64, 1, "substeps", 0)); // the bound also ends the loop for a dt this small
  {
    MultirateSchedule s;
    const char* which = "";
    long at = -1;
    CHECK(multirate_schedule(0.01, 0.64, 65, 2, &s, &which, &at));  // sim_dt = 64 dt fits MULTIRATE_MAX_SUB
    CHECK(s.total() <= 2 * MULTIRATE_MAX_SUB);
  }
  CHECK(multirate_refusal("f", "sim_dt", 0, 0.0, 8) == "f: sim_dt must be finite and > 0");
  CHECK(multirate_refusal("f", "shift", 2, 0.2, 8).find("more than N - 1 = 7 knots in step 2") != std::string::npos);
  CHECK(multirate_refusal("f", "shift", 2, 0.2, 8).find("sim_dt") != std::string::npos);
  CHECK(multirate_refusal("f", "substeps", 1, 0.7, 64).find("MULTIRATE_MAX_SUB = 66 plant sub-steps in step 1") !=
        std::string::npos);

  // the workspace: sizes by name, and a run of 0 steps still gets one row of every history
  size_t by[MULTIRATE_WS_COUNT], off[MULTIRATE_WS_COUNT];
  multirate_ws_bytes(5, 2, 10, 11, by);
  CHECK(by[MRWS_EP] == 48 && by[MRWS_DIST] == 8 * 50 && by[MRWS_Q] == 48 * 50 && by[MRWS_U] == 48 * 50);
  CHECK(by[MRWS_XPATH] == 48 * 55 && by[MRWS_SUBDT] == 88 && by[MRWS_RHO0] == 40 && by[MRWS_GI] == 20 &&
        by[MRWS_ALIVE] == 20);
  const size_t total = carve(by, MULTIRATE_WS_COUNT, off);
  for (int i = 0; i < MULTIRATE_WS_COUNT; ++i) {
    CHECK(off[i] % WS_ALIGN == 0);
    CHECK(off[i] + by[i] <= (i + 1 < MULTIRATE_WS_COUNT ? off[i + 1] : total));
  }
  multirate_ws_bytes(3, 1, 0, 0, by);
  CHECK(by[MRWS_DIST] == 24 && by[MRWS_Q] == 144 && by[MRWS_U] == 144 && by[MRWS_XPATH] == 144 && by[MRWS_SUBDT] == 8);

  if (bad) return 1;
  std::printf("multirate_plan_check OK\n");
  return 0;
}
