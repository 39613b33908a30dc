// Host check of the controller session's plan (indy7_mpc_amd/csrc/i7m_plan.h): the buffer request
// of i7m_ctrl_begin against hand-computed bytes (ctrl_ws_bytes, ctrl_host_bytes, the record layout)
// and the argument checks of i7m_ctrl_begin / i7m_ctrl_step (ctrl_begin_args_ok, ctrl_step_args_ok).
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

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
  // the record: u(6) fbest(6) err ee(3) best, contiguous
  CHECK(CREC_U == 0 && CREC_FBEST == 6 && CREC_ERR == 12 && CREC_EE == 13 && CREC_BEST == 16 && CTRL_REC == 17,
        "record layout");
  // (G, H, N) = (3, 4, 8), L = 300, stride 6, phases: by hand
  {
    size_t b[CTRL_WS_COUNT], off[CTRL_WS_COUNT];
    ctrl_ws_bytes(3, 4, 8, 300, 6, true, b);
    CHECK(b[CWS_REF] == 300 * 6 * 8 && b[CWS_PHASE] == 12, "reference %zu phases %zu", b[CWS_REF], b[CWS_PHASE]);
    CHECK(b[CWS_XUB] == 3 * 138 * 8 && b[CWS_XLAST] == 288 && b[CWS_XMEAS] == 288 && b[CWS_ULAST] == 144 && b[CWS_BEST] == 12,
          "per-group state");
    CHECK(b[CWS_NOISE] == 12 * 24 && b[CWS_REC] == 3 * 17 * 8 && b[CWS_RHO0] == 96, "noise %zu record %zu rho %zu",
          b[CWS_NOISE], b[CWS_REC], b[CWS_RHO0]);
    // 256-byte slots: 14592 + 256 + 3328 + 512 + 256 + 256 + 512 + 512 + 512 + 256
    const size_t total = carve(b, CTRL_WS_COUNT, off);
    CHECK(total == 20992, "carved total %zu", total);
    CHECK(off[CWS_REF] == 0 && off[CWS_PHASE] == 14592 && off[CWS_XUB] == 14848 && off[CWS_REC] == 20224, "offsets");
    for (int i = 0; i < CTRL_WS_COUNT; ++i) {
      CHECK(off[i] % WS_ALIGN == 0, "sub-buffer %d misaligned", i);
      CHECK(i + 1 == CTRL_WS_COUNT || off[i] + b[i] <= off[i + 1], "sub-buffer %d overlaps the next", i);
    }
    CHECK(off[CTRL_WS_COUNT - 1] + b[CTRL_WS_COUNT - 1] <= total, "the last sub-buffer runs past the allocation");
    size_t hb[CTRL_HS_COUNT], hoff[CTRL_HS_COUNT];
    ctrl_host_bytes(3, 4, hb);
    CHECK(hb[CHS_XMEAS] == 288 && hb[CHS_NOISE] == 288 && hb[CHS_REC] == 408, "host staging");
    CHECK(carve(hb, CTRL_HS_COUNT, hoff) == 512 + 512 + 512, "host staging total");
    // the staging mirrors the device buffers it is copied to / from
    CHECK(hb[CHS_XMEAS] == b[CWS_XMEAS] && hb[CHS_NOISE] == b[CWS_NOISE] && hb[CHS_REC] == b[CWS_REC], "staging sizes");
  }
  // the deployed shape, stride 3, no phases; and the largest: 256 hypotheses at N = 64
  {
    size_t b[CTRL_WS_COUNT];
    ctrl_ws_bytes(1, 16, 64, 1, 3, false, b);
    CHECK(b[CWS_REF] == 24 && b[CWS_PHASE] == 0 && b[CWS_XUB] == 1146 * 8 && b[CWS_NOISE] == 16 * 24 && b[CWS_REC] == 136,
          "deployed shape");
    ctrl_ws_bytes(0, 4, 8, 5, 3, true, b);
    CHECK(b[CWS_PHASE] == 0 && b[CWS_XUB] == 0 && b[CWS_REC] == 0 && b[CWS_NOISE] == 0, "no groups: only the reference");
    ctrl_ws_bytes(64, 256, 64, 2147483647L, 6, true, b);
    CHECK(b[CWS_REF] == (size_t)48 * 2147483647u && b[CWS_NOISE] == 24u * 16384u, "large request without overflow");
  }

  // i7m_ctrl_begin's arguments
  const char* which = "";
  long at = -7;
  const double ref[6] = {0}, fh[6] = {0};
  const int32_t ph_ok[3] = {0, 17, 50}, ph_bad[3] = {0, 17, -2};
  const auto begin = [&](int mode, int mb, int G, int H, long L, int stride, const void* r, const int32_t* ph, const void* f,
                         int frame, int what) {
    which = "";
    at = -7;
    return ctrl_begin_args_ok(mode, mb, G, H, L, stride, r, ph, f, frame, what, &which, &at);
  };
  const auto named = [&](const char* w, long a) { return std::string(which) == w && at == a; };
  CHECK(begin(I7M_QP_DIRECT, 12, 3, 4, 300, 6, ref, ph_ok, fh, I7M_WRENCH_WORLD, I7M_ADMM_RESET_ALL), "a valid begin");
  CHECK(begin(I7M_QP_ADMM, 12, 3, 4, 1, 3, ref, nullptr, fh, I7M_WRENCH_LOCAL, 0), "a valid begin without phases");
  CHECK(begin(I7M_QP_ADMM, 12, 0, 4, 1, 3, ref, ph_bad, fh, I7M_WRENCH_LOCAL, 0), "no groups reads no phases");
  CHECK(!begin(I7M_QP_BOX, 12, 3, 4, 300, 6, ref, ph_ok, fh, 1, 7) && named("qp_mode", I7M_QP_BOX), "box: %s %ld", which, at);
  for (int H : {0, 3, 12, 512, -4})
    CHECK(!begin(I7M_QP_DIRECT, 4096, 1, H, 300, 6, ref, nullptr, fh, 1, 7) && named("H", H), "H = %d: %s %ld", H, which, at);
  for (int H : {1, 2, 4, 8, 16, 32, 64, 128, 256})
    CHECK(begin(I7M_QP_DIRECT, 256, 1, H, 300, 6, ref, nullptr, fh, 1, 7), "H = %d refused", H);
  CHECK(!begin(I7M_QP_DIRECT, 12, 4, 4, 300, 6, ref, nullptr, fh, 1, 7) && named("G", 16), "rows: %s %ld", which, at);
  CHECK(!begin(I7M_QP_DIRECT, 12, -1, 4, 300, 6, ref, nullptr, fh, 1, 7) && named("G", -4), "negative G: %s %ld", which, at);
  CHECK(!begin(I7M_QP_DIRECT, 2147483647, 2147483647, 256, 300, 6, ref, nullptr, fh, 1, 7) && std::string(which) == "G",
        "G H past int32: %s", which);
  CHECK(!begin(I7M_QP_DIRECT, 12, 3, 4, 0, 6, ref, nullptr, fh, 1, 7) && named("L", 0), "L: %s %ld", which, at);
  for (int st : {0, 2, 4, 5, 7})
    CHECK(!begin(I7M_QP_DIRECT, 12, 3, 4, 300, st, ref, nullptr, fh, 1, 7) && named("ref_stride", st), "stride %d", st);
  CHECK(!begin(I7M_QP_DIRECT, 12, 3, 4, 300, 6, ref, nullptr, fh, 5, 7) && named("frame", 5), "frame: %s %ld", which, at);
  CHECK(!begin(I7M_QP_DIRECT, 12, 3, 4, 300, 6, ref, nullptr, fh, 1, 8) && named("reset_what", 8), "reset: %s %ld", which, at);
  CHECK(!begin(I7M_QP_DIRECT, 12, 3, 4, 300, 6, nullptr, nullptr, fh, 1, 7) && named("ref", 0), "null ref: %s", which);
  CHECK(!begin(I7M_QP_DIRECT, 12, 3, 4, 300, 6, ref, nullptr, nullptr, 1, 7) && named("fhyp", 0), "null fhyp: %s", which);
  CHECK(!begin(I7M_QP_DIRECT, 12, 3, 4, 300, 6, ref, ph_bad, fh, 1, 7) && named("ref_phase", 2), "phase: %s %ld", which, at);

  // i7m_ctrl_step's
  std::vector<double> x(36, 0.25);
  double u[18];
  const auto step = [&](const double* xm, double el, int32_t off, const void* uo) {
    which = "";
    at = -7;
    return ctrl_step_args_ok(xm, 3, el, off, uo, &which, &at);
  };
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(step(x.data(), 0.01, 0, u), "a valid step");
  CHECK(step(x.data(), 5.0, 2147483647, u), "elapsed is not bounded by dt");
  CHECK(step(x.data(), 1e-300, 0, u), "a tiny elapsed is positive");
  CHECK(!step(nullptr, 0.01, 0, u) && named("x_meas", -1), "null x_meas: %s %ld", which, at);
  CHECK(!step(x.data(), 0.01, 0, nullptr) && named("u_out", -1), "null u_out: %s %ld", which, at);
  for (double el : {0.0, -0.01, inf, -inf, nan})
    CHECK(!step(x.data(), el, 0, u) && named("elapsed", 0), "elapsed %g: %s", el, which);
  CHECK(!step(x.data(), 0.01, -1, u) && named("ref_offset", -1), "offset: %s %ld", which, at);
  for (double bad : {nan, inf, -inf})
    for (long e : {0L, 17L, 35L}) {
      std::vector<double> y = x;
      y[e] = bad;
      CHECK(!step(y.data(), 0.01, 0, u) && named("x_meas", e), "x_meas[%ld] = %g: %s %ld", e, bad, which, at);
    }
  // the scan stops at 12 G: entry 36 belongs to nobody
  x.push_back(nan);
  CHECK(step(x.data(), 0.01, 0, u), "the scan reads past 12 G");

  if (g_failed) {
    std::printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("ctrl_plan_check OK\n");
  return 0;
}
