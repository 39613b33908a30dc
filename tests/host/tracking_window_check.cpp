// Host check of the tracking goal source's plan (indy7_mpc_amd/csrc/i7m_plan.h): the window-index
// clamp track_index that the kernel and the host's initial window share, the schedule validation
// (sampled_call_ok's scans of the phases and the offsets),
// and the workspace request of i7m_mpc_run_tracking against hand-computed bytes, with the endpoint
// request (i7m_mpc_run_sampled) unchanged.
#include <cstdio>

#include "../../indy7_mpc_amd/csrc/i7m_plan.h"

static int g_failed = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAILED: " __VA_ARGS__); \
      std::printf("\n");                 \
      ++g_failed;                        \
    }                                    \
  } while (0)

int main() {
  using namespace i7m;
  // the clamp: L = 100 points, the last index 99
  const long L = 100;
  for (int withph = 0; withph < 2; ++withph) {
    const long ph = withph ? 17 : 0;
    // off + k chosen so that ph + off + k is L - 2, L - 1, L, and far beyond
    CHECK(track_index(ph, L - 2 - ph - 5, 5, L) == L - 2, "L - 2 with phase %ld", ph);
    CHECK(track_index(ph, L - 1 - ph - 5, 5, L) == L - 1, "L - 1 with phase %ld", ph);
    CHECK(track_index(ph, L - ph - 5, 5, L) == L - 1, "L clamps with phase %ld", ph);
    CHECK(track_index(ph, 2147483647L, 63, L) == L - 1, "far beyond with phase %ld", ph);
    CHECK(track_index(ph, 0, 0, L) == ph, "the window's first point with phase %ld", ph);
    CHECK(track_index(ph, 3, 4, L) == ph + 7, "inside with phase %ld", ph);
  }
  // the largest arguments the int32 ABI can pass do not overflow
  CHECK(track_index(2147483647L, 2147483647L, 63, 2147483647L) == 2147483646L, "largest int32 arguments");
  // L = 1: every knot of every window reads point 0
  for (long ph : {0L, 5L})
    for (long off : {0L, 1L, 1000L})
      for (long k : {0L, 1L, 63L}) CHECK(track_index(ph, off, k, 1) == 0, "L = 1 at %ld %ld %ld", ph, off, k);
  // every index of a run past the end stays inside [0, L)
  for (long Lr = 1; Lr <= 12; ++Lr)
    for (long off = 0; off < 20; ++off)
      for (long k = 0; k < 8; ++k) {
        const long i = track_index(2, off, k, Lr);
        CHECK(i >= 0 && i < Lr && (2 + off + k >= Lr ? i == Lr - 1 : i == 2 + off + k), "L %ld off %ld k %ld -> %ld", Lr, off, k, i);
      }

  // the schedule
  const char* which = "";
  long at = -1;
  const int32_t ph_ok[3] = {0, 17, 50}, ph_bad[3] = {0, -1, 50}, off_ok[4] = {0, 0, 1, 2}, off_bad[4] = {1, 2, 3, -4};
  const double some[1] = {0};
  const auto schedule_ok = [&](const int32_t* ref_phase, int G, const int32_t* ref_offset, int num_steps) {
    SampledCall c;
    c.kind = SampledKind::tracking;
    c.max_batch = G;
    c.dt = c.o.sim_dt = 0.01;
    c.G = G;
    c.H = 1;
    c.num_steps = num_steps;
    c.o.frame = I7M_WRENCH_WORLD;
    c.o.n_actual = 1;
    c.goal.ref = c.xstart = c.fhyp = c.f_actual = c.hist_out = some;
    c.goal.L = 1;
    c.goal.ref_stride = 3;
    c.goal.ref_phase = ref_phase;
    c.goal.ref_offset = ref_offset;
    return sampled_call_ok(c, &which, &at);
  };
  CHECK(schedule_ok(ph_ok, 3, off_ok, 4), "a valid schedule is refused");
  CHECK(schedule_ok(nullptr, 3, off_ok, 4), "no phases is refused");
  CHECK(schedule_ok(nullptr, 3, nullptr, 0), "no steps reads no offsets");
  CHECK(!schedule_ok(ph_bad, 3, off_ok, 4) && std::string(which) == "ref_phase" && at == 1,
        "negative phase: %s[%ld]", which, at);
  CHECK(!schedule_ok(ph_ok, 3, off_bad, 4) && std::string(which) == "ref_offset" && at == 3,
        "negative offset: %s[%ld]", which, at);

  // the workspace of a tracking request, (G, H, N, steps) = (3, 4, 8, 6), L = 300, stride 6, phases,
  // noise, one actual wrench: by hand
  {
    size_t b[TRACKING_WS_COUNT];
    tracking_ws_bytes(3, 4, 8, 6, 0, 1, true, 300, 6, true, b);
    CHECK(TRACKING_WS_COUNT == SAMPLED_WS_COUNT + 3, "tracking request has %d sub-buffers", (int)TRACKING_WS_COUNT);
    CHECK(b[SWS_EP] == 0, "no endpoints: %zu", b[SWS_EP]);
    CHECK(b[SWS_XCUR] == 3 * 12 * 8 && b[SWS_XUB] == 3 * 138 * 8 && b[SWS_FACT] == 3 * 6 * 8, "per-group state");
    CHECK(b[SWS_NOISE] == 6 * 12 * 3 * 8, "noise %zu", b[SWS_NOISE]);
    CHECK(b[SWS_DIST] == 18 * 8 && b[SWS_Q] == 18 * 48 && b[SWS_FB] == 18 * 48 && b[SWS_BH] == 18 * 4, "histories");
    CHECK(b[SWS_RHO0] == 12 * 8 && b[SWS_BEST] == 12 && b[SWS_GI] == 12 && b[SWS_ALIVE] == 12, "rows and flags");
    CHECK(b[TWS_REF] == 300 * 6 * 8, "reference %zu", b[TWS_REF]);
    CHECK(b[TWS_PHASE] == 12, "phases %zu", b[TWS_PHASE]);
    CHECK(b[TWS_EE] == 18 * 24, "ee history %zu", b[TWS_EE]);
    size_t off[TRACKING_WS_COUNT];
    // 256-byte slots: 0 + 512 + 3328 + 256 + 1792 + 256 + 1024 + 1024 + 256 + 4 x 256 = 9472, then
    // 14592 + 256 + 512
    CHECK(carve(b, TRACKING_WS_COUNT, off) == 24832, "carved total %zu", carve(b, TRACKING_WS_COUNT, off));
    CHECK(off[TWS_REF] == 9472 && off[TWS_PHASE] == 24064 && off[TWS_EE] == 24320, "offsets %zu %zu %zu", off[TWS_REF],
          off[TWS_PHASE], off[TWS_EE]);
    // stride 3, no phases, no noise, no steps: one history row
    tracking_ws_bytes(1, 16, 64, 0, 0, 1, false, 1, 3, false, b);
    CHECK(b[TWS_REF] == 24 && b[TWS_PHASE] == 0 && b[TWS_EE] == 24 && b[SWS_NOISE] == 0 && b[SWS_DIST] == 8, "smallest request");
  }
  // the endpoint request: the parent's formula in its 13 sub-buffers, nothing after them, and the
  // same allocation
  for (int noise = 0; noise < 2; ++noise) {
    const int G = 256, H = 16, N = 32, steps = 20, E = 2;
    size_t b[TRACKING_WS_COUNT], p[SAMPLED_WS_COUNT], offb[TRACKING_WS_COUNT], offp[SAMPLED_WS_COUNT];
    tracking_ws_bytes(G, H, N, steps, E, 1, noise != 0, 0, 0, false, b);
    sampled_ws_bytes(G, H, N, steps, E, 1, noise != 0, p);
    const size_t hist = (size_t)steps * G, B = (size_t)G * H;
    const size_t want[SAMPLED_WS_COUNT] = {24u * E, 96u * G, 8u * (18 * N - 6) * G, 48u * G, noise ? 24 * steps * B : 0,
                                           8 * hist, 48 * hist, 48 * hist, 8 * B, 4u * G, 4u * G, 4u * G, 4 * hist};
    for (int i = 0; i < SAMPLED_WS_COUNT; ++i)
      CHECK(b[i] == want[i] && p[i] == want[i], "endpoint sub-buffer %d: %zu / %zu, expected %zu", i, b[i], p[i], want[i]);
    CHECK(b[TWS_REF] == 0 && b[TWS_PHASE] == 0 && b[TWS_EE] == 0, "endpoint mode carries tracking bytes");
    CHECK(carve(b, TRACKING_WS_COUNT, offb) == carve(p, SAMPLED_WS_COUNT, offp), "endpoint allocation changed");
    for (int i = 0; i < SAMPLED_WS_COUNT; ++i) CHECK(offb[i] == offp[i], "endpoint offset %d moved", i);
  }
  if (g_failed) {
    std::printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("tracking_window_check OK\n");
  return 0;
}
