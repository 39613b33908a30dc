// Host check of the controller session's plan (indy7_mpc_amd/csrc/i7m_plan.h): the buffer request
// of i7m_ctrl_begin against hand-computed bytes (ctrl_ws_bytes, ctrl_host_bytes, the record layout),
// the one argument check of the sampled-wrench family (sampled_call_ok: i7m_mpc_run_sampled,
// i7m_mpc_run_tracking, i7m_ctrl_begin) with its refusal texts (sampled_refusal), and i7m_ctrl_step's
// (ctrl_step_args_ok, ctrl_step_refusal).
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
  const auto begin = [&](int mode, int mb, int G, int H, long L, int stride, const double* r, const int32_t* ph,
                         const double* f, int frame, int what) {
    which = "";
    at = -7;
    SampledCall c;
    c.kind = SampledKind::session;
    c.qp_mode = mode;
    c.max_batch = mb;
    c.G = G;
    c.H = H;
    c.o.frame = frame;
    c.o.reset_what = what;
    c.goal.ref = r;
    c.goal.L = L;
    c.goal.ref_stride = stride;
    c.goal.ref_phase = ph;
    c.fhyp = f;
    return sampled_call_ok(c, &which, &at);
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

  // the two loops through the same check: a valid call of each, then one bad argument at a time
  const double xs[36] = {0}, ends[6] = {0}, fa[18] = {0};
  double hist[12];
  const std::vector<int32_t> ph3 = {0, 17, 50}, off4 = {0, 0, 1, 2};  // heap arrays of exactly G and num_steps entries
  const auto loop_call = [&](SampledKind kind) {
    SampledCall c;
    c.kind = kind;
    c.qp_mode = I7M_QP_ADMM;
    c.max_batch = 12;
    c.dt = 0.01;
    c.G = 3;
    c.H = 4;
    c.num_steps = 4;
    c.o.sim_dt = 0.001;
    c.o.decay = 1.0;
    c.o.frame = I7M_WRENCH_WORLD;
    c.o.reset_what = I7M_ADMM_RESET_ALL;
    c.o.keep_best = 0;
    c.o.n_actual = 1;
    if (kind == SampledKind::endpoints) {
      c.goal.endpoints = ends;
      c.goal.n_endpoints = 2;
    } else {
      c.goal.ref = ref;
      c.goal.L = 300;
      c.goal.ref_stride = 6;
      c.goal.ref_phase = ph3.data();
      c.goal.ref_offset = off4.data();
    }
    c.xstart = xs;
    c.fhyp = fh;
    c.f_actual = fa;
    c.hist_out = hist;
    return c;
  };
  const auto ok = [&](const SampledCall& c) {
    which = "";
    at = -7;
    return sampled_call_ok(c, &which, &at);
  };
  for (SampledKind kind : {SampledKind::endpoints, SampledKind::tracking}) {
    const bool track = kind == SampledKind::tracking;
    const SampledCall good = loop_call(kind);
    SampledCall c = good;
    CHECK(ok(c), "a valid loop call (tracking %d): %s %ld", (int)track, which, at);
    c.qp_mode = I7M_QP_BOX;
    CHECK(!ok(c) && named("qp_mode", I7M_QP_BOX), "loop box: %s %ld", which, at);
    c = good, c.H = 3;
    CHECK(!ok(c) && named("H", 3), "loop H: %s %ld", which, at);
    c = good, c.G = 4;
    CHECK(!ok(c) && named("G", 16), "loop rows: %s %ld", which, at);
    // sim_dt in (0, dt], dt itself accepted
    c = good, c.o.sim_dt = c.dt;
    CHECK(ok(c), "sim_dt == dt refused: %s", which);
    for (double sd : {0.0, -0.001, 0.011, std::numeric_limits<double>::quiet_NaN()}) {
      c = good, c.o.sim_dt = sd;
      CHECK(!ok(c) && std::string(which) == "sim_dt", "sim_dt %g: %s", sd, which);
    }
    c = good, c.o.frame = 5;
    CHECK(!ok(c) && named("frame", 5), "loop frame: %s %ld", which, at);
    c = good, c.o.reset_what = 8;
    CHECK(!ok(c) && named("reset_what", 8), "loop reset: %s %ld", which, at);
    // n_actual in {1, num_steps}
    c = good, c.o.n_actual = 4;
    CHECK(ok(c), "n_actual == num_steps refused: %s", which);
    for (int na : {0, 2, 3, 5, -1}) {
      c = good, c.o.n_actual = na;
      CHECK(!ok(c) && named("n_actual", na), "n_actual %d: %s %ld", na, which, at);
    }
    c = good, c.num_steps = -1;
    CHECK(!ok(c) && named("num_steps", -1), "negative num_steps: %s %ld", which, at);
    // no steps: n_actual 1 only, and no offsets read
    c = good, c.num_steps = 0, c.goal.ref_offset = nullptr;
    CHECK(ok(c), "no steps refused: %s %ld", which, at);
    // each required pointer
    c = good, c.xstart = nullptr;
    CHECK(!ok(c) && named("xstart", 0), "null xstart: %s %ld", which, at);
    c = good, c.fhyp = nullptr;
    CHECK(!ok(c) && named("fhyp", 0), "null fhyp: %s %ld", which, at);
    c = good, c.f_actual = nullptr;
    CHECK(!ok(c) && named("f_actual", 0), "null f_actual: %s %ld", which, at);
    c = good, c.hist_out = nullptr;
    CHECK(!ok(c) && named(track ? "err_out" : "dist_out", 0), "null history: %s %ld", which, at);
    if (!track) {
      c = good, c.goal.endpoints = nullptr;
      CHECK(!ok(c) && named("endpoints", 0), "null endpoints: %s %ld", which, at);
      for (int ne : {0, -1}) {
        c = good, c.goal.n_endpoints = ne;
        CHECK(!ok(c) && named("n_endpoints", ne), "n_endpoints %d: %s %ld", ne, which, at);
      }
      c = good, c.goal.n_endpoints = 1;
      CHECK(ok(c), "one endpoint refused: %s", which);
      // the endpoint loop reads nothing of a reference
      c = good, c.goal.L = 0, c.goal.ref_stride = 4, c.goal.ref_phase = ph_bad;
      CHECK(ok(c), "the endpoint loop looked at the reference: %s", which);
    } else {
      c = good, c.goal.ref = nullptr;
      CHECK(!ok(c) && named("ref", 0), "loop null ref: %s %ld", which, at);
      c = good, c.goal.ref_offset = nullptr;
      CHECK(!ok(c) && named("ref_offset", -1), "null ref_offset with steps: %s %ld", which, at);
      c = good, c.goal.L = 0;
      CHECK(!ok(c) && named("L", 0), "loop L: %s %ld", which, at);
      c = good, c.goal.ref_stride = 4;
      CHECK(!ok(c) && named("ref_stride", 4), "loop stride: %s %ld", which, at);
      c = good, c.goal.ref_phase = nullptr;
      CHECK(ok(c), "no phases refused: %s", which);
      c = good, c.goal.ref_phase = ph_bad;
      CHECK(!ok(c) && named("ref_phase", 2), "loop phase: %s %ld", which, at);
      std::vector<int32_t> off_bad = off4;
      off_bad[3] = -4;
      c = good, c.goal.ref_offset = off_bad.data();
      CHECK(!ok(c) && named("ref_offset", 3), "negative offset: %s %ld", which, at);
      // the scans stop at G and num_steps: a bad entry beyond them belongs to nobody
      c = good, c.G = 2, c.goal.ref_phase = ph_bad;
      CHECK(ok(c), "the phase scan reads past G: %s %ld", which, at);
      c = good, c.num_steps = 3, c.o.n_actual = 1, c.goal.ref_offset = off_bad.data();
      CHECK(ok(c), "the offset scan reads past num_steps: %s %ld", which, at);
      c = good, c.G = 0, c.goal.ref_phase = ph_bad;
      CHECK(ok(c), "no groups reads no phases (loop): %s %ld", which, at);
    }
  }
  // the session reads neither sim_dt nor n_actual, has no steps and needs no start states
  {
    SampledCall c = loop_call(SampledKind::tracking);
    c.kind = SampledKind::session;
    c.o.sim_dt = 0.0;
    c.o.n_actual = 3;
    c.xstart = c.f_actual = c.hist_out = nullptr;
    c.goal.ref_offset = nullptr;
    CHECK(ok(c), "session: %s %ld", which, at);
  }

  // the refusal texts: the fragment of every `which` that callers and tests match
  const auto text = [&](const char* w, long a) { return sampled_refusal("who", w, a, 12); };
  const auto has = [&](const std::string& msg, const char* frag) { return msg.find(frag) != std::string::npos; };
  CHECK(has(text("qp_mode", I7M_QP_BOX), "who: ") && has(text("qp_mode", I7M_QP_BOX), "I7M_QP_BOX"), "qp_mode text");
  CHECK(has(text("H", 3), "H = 3"), "H text");
  CHECK(has(text("G", 16), "G x H = 16") && has(text("G", 16), "max_batch=12"), "G text");
  CHECK(has(text("L", 0), "L = 0"), "L text");
  CHECK(has(text("ref_stride", 4), "ref_stride = 4"), "ref_stride text");
  CHECK(has(text("ref_offset", 1), "ref_offset[1]"), "ref_offset entry text");
  CHECK(has(text("ref_phase", 0), "ref_phase[0]") && has(text("ref_phase", 1), "ref_phase[1]"), "ref_phase text");
  CHECK(has(text("sim_dt", 0), "sim_dt"), "sim_dt text");
  CHECK(has(text("frame", 5), "frame"), "frame text");
  CHECK(has(text("reset_what", 8), "RESET"), "reset_what text");
  CHECK(has(text("n_actual", 3), "n_actual"), "n_actual text");
  CHECK(has(text("n_endpoints", 0), "endpoint") && has(text("num_steps", -1), "num_steps"), "counts text");
  CHECK(has(text("ref", 0), "null ref") && has(text("fhyp", 0), "null fhyp"), "null ref / fhyp text");
  CHECK(has(text("ref_offset", -1), "null ref_offset"), "null ref_offset text");
  CHECK(has(text("err_out", 0), "null err_out") && has(text("dist_out", 0), "null dist_out"), "history text");
  for (const char* w : {"xstart", "endpoints", "f_actual"}) CHECK(has(text(w, 0), (std::string("null ") + w).c_str()), "null %s text", w);
  CHECK(has(ctrl_step_refusal("who", "x_meas", 13), "x_meas[13]") && has(ctrl_step_refusal("who", "x_meas", -1), "null x_meas") &&
            has(ctrl_step_refusal("who", "u_out", -1), "null u_out") && has(ctrl_step_refusal("who", "elapsed", 0), "elapsed") &&
            has(ctrl_step_refusal("who", "ref_offset", -1), "ref_offset = -1"),
        "step texts");

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
