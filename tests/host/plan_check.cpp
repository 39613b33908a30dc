// plan_check.cpp — the launch plan (indy7_mpc_amd/csrc/i7m_plan.h) checked on the host: range and
// chunk coverage, the pinned size thresholds, the retired environment variables, and the closed
// loops' workspace carve.  A stand-alone program (tests/test_plan_host.py builds it with the host
// compiler under -fsanitize=address,undefined and runs it); prints every failed check, exit status
// 1 on any.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../indy7_mpc_amd/csrc/i7m_plan.h"

using namespace i7m;

static int g_failed = 0;
#define CHECK(cond, ...)                               \
  do {                                                 \
    if (!(cond)) {                                     \
      ++g_failed;                                      \
      std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                        \
      std::printf("\n");                               \
    }                                                  \
  } while (0)

// boundaries b[0..n]: start at 0, end at B, monotone, never past B
static void check_cover(const std::vector<long>& b, int B, const char* what, int nch) {
  CHECK(b.front() == 0, "%s B=%d nch=%d starts at %ld", what, B, nch, b.front());
  CHECK(b.back() == B, "%s B=%d nch=%d ends at %ld", what, B, nch, b.back());
  for (size_t i = 0; i + 1 < b.size(); ++i)
    CHECK(b[i] <= b[i + 1] && b[i + 1] <= B, "%s B=%d nch=%d boundary %zu: %ld then %ld", what, B, nch, i, b[i], b[i + 1]);
}

static void coverage() {
  std::vector<int> sizes;
  for (int B = 1; B <= 40; ++B) sizes.push_back(B);
  for (int B : {3071, 3072, 3073, 4096, 8192}) sizes.push_back(B);
  for (int B : sizes) {
    check_cover({0, stagger_cut(B), B}, B, "stagger", 2);
    for (int nch = 1; nch <= 6; ++nch)
      for (int taper = 0; taper < 2; ++taper) {
        std::vector<long> b;
        for (int i = 0; i <= nch; ++i) b.push_back(chunk_lo(B, nch, i, taper != 0));
        check_cover(b, B, taper ? "tapered chunks" : "equal chunks", nch);
      }
  }
}

static void pinned() {
  const Tuning t;  // the defaults
  // ADMM iteration kernel
  CHECK(admm_iter_kernel(t, 32, false, 256) == AdmmIter::res, "N=32 n=256");
  CHECK(admm_iter_kernel(t, 32, false, 257) == AdmmIter::iter2, "N=32 n=257");
  CHECK(admm_iter_kernel(t, 32, false, 512) == AdmmIter::iter2, "N=32 n=512");
  CHECK(admm_iter_kernel(t, 32, false, 513) == AdmmIter::iter4, "N=32 n=513");
  CHECK(admm_iter_kernel(t, 64, false, 16) == AdmmIter::iter2, "N=64 n=16");
  for (int n : {1, 256, 513, 4096}) {
    CHECK(admm_iter_kernel(t, 32, true, n) == AdmmIter::adapt, "adaptive rho N=32 n=%d", n);
    CHECK(admm_iter_kernel(t, 64, true, n) == AdmmIter::adapt, "adaptive rho N=64 n=%d", n);
  }
  Tuning res1 = t;
  res1.admm_res = 1;  // forced, but N = 64 does not fit: the iter2 rule decides
  CHECK(admm_iter_kernel(res1, 64, false, 16) == AdmmIter::iter2, "res=1 N=64 n=16");
  CHECK(admm_iter_kernel(res1, 64, false, 513) == AdmmIter::iter4, "res=1 N=64 n=513");
  CHECK(admm_iter_kernel(res1, 32, false, 4096) == AdmmIter::res, "res=1 N=32 n=4096");
  // prep
  CHECK(admm_prep_ilp(t, 1024), "prep n=1024");
  CHECK(!admm_prep_ilp(t, 1025), "prep n=1025");
  // Riccati
  CHECK(riccati_variant(t, 128, false).w2, "w2 B=128");
  CHECK(!riccati_variant(t, 129, false).w2, "w2 B=129");
  CHECK(!riccati_variant(t, 1, true).w2, "w2 with vout");
  CHECK(riccati_variant(t, 767, false).bc == 3, "bc B=767");
  CHECK(riccati_variant(t, 768, false).bc == 7, "bc B=768");
  // line search
  CHECK(ls_waves(t, 768) == 4 && ls_waves(t, 769) == 1, "line-search waves at 768 / 769");
  CHECK(fused_waves(t, 256) == 4 && fused_waves(t, 257) == 1, "fused waves at 256 / 257");
  // stagger
  CHECK(!stagger_applies(t, I7M_QP_ADMM, 3071), "stagger at 3071");
  CHECK(stagger_applies(t, I7M_QP_ADMM, 3072), "stagger at 3072");
  CHECK(!stagger_applies(t, I7M_QP_DIRECT, 4096) && !stagger_applies(t, I7M_QP_BOX, 4096), "stagger outside ADMM mode");
  Tuning off = t;
  off.admm_stagger = 0;
  CHECK(!stagger_applies(off, I7M_QP_ADMM, 4096), "stagger 0");
  CHECK(stagger_cut(4096) == 2048, "cut(4096) = %ld", stagger_cut(4096));
  CHECK(stagger_cut(3073) == 1536, "cut(3073) = %ld", stagger_cut(3073));
  Tuning min2 = t;
  min2.admm_stagger_min_b = 2;
  CHECK(stagger_applies(min2, I7M_QP_ADMM, 5) && stagger_cut(5) == 4, "cut(5) = %ld", stagger_cut(5));
  CHECK(stagger_applies(min2, I7M_QP_ADMM, 2) && stagger_cut(2) == 2, "cut(2) = %ld (second range empty)", stagger_cut(2));
  CHECK(stagger_cut(13) == 8, "cut(13) = %ld", stagger_cut(13));
  // host-to-host chunks
  CHECK(h2h_chunks_for(t, I7M_QP_DIRECT, 4096) == 3, "direct 4096 chunks");
  const long want[4] = {0, 1024, 3072, 4096};
  for (int i = 0; i <= 3; ++i)
    CHECK(chunk_lo(4096, 3, i, t.h2h_taper != 0) == want[i], "direct 4096 boundary %d = %ld", i, chunk_lo(4096, 3, i, true));
  CHECK(h2h_chunks_for(t, I7M_QP_DIRECT, 2048) == 2, "direct 2048 chunks");
  CHECK(h2h_chunks_for(t, I7M_QP_DIRECT, 2047) == 1, "direct 2047 chunks");
  CHECK(h2h_chunks_for(t, I7M_QP_ADMM, 3072) == 2, "ADMM 3072 chunks");
  Tuning six = t;
  six.h2h_chunks = 6;
  CHECK(h2h_chunks_for(six, I7M_QP_ADMM, 4096) == 6 && h2h_chunks_for(six, I7M_QP_DIRECT, 4) == 4, "explicit chunks");
}

static const char* const kKnobs[] = {
    "I7M_IPM", "I7M_LS_TAIL", "I7M_LS_WAVES", "I7M_GRAPH", "I7M_RIC_W2", "I7M_RIC_BC", "I7M_H2H_CHUNKS", "I7M_H2H_PIPE",
    "I7M_H2H_TAPER", "I7M_ADMM_STAGGER", "I7M_ADMM_STAGGER_MIN_B", "I7M_ADMM_ITER2", "I7M_ADMM_RES", "I7M_ADMM_RES_MAX",
    "I7M_ADMM_PREP_ILP", "I7M_ADMM_PREP_ILP_MAX", "I7M_PIPE", "I7M_GENERIC"};
static const char* const kRetired[] = {"I7M_ADMM_CHUNK", "I7M_DEV_RANGES", "I7M_ADMM_CHAINS", "I7M_ADMM_RANGES",
                                       "I7M_ADMM_SPLIT", "I7M_STAGGER_MODES", "I7M_ADMM_ITER_DYN_LDS"};

static void environment() {
  for (const char* k : kKnobs) unsetenv(k);
  for (const char* k : kRetired) unsetenv(k);
  i7m_config cfg{};
  Tuning t;
  std::string err;
  CHECK(tuning_from_env(cfg, &t, &err), "clean environment: %s", err.c_str());
  CHECK(t.admm_stagger == 1 && t.admm_stagger_min_b == 3072 && t.h2h_pipe == 2 && t.h2h_taper == 1 && t.ric_bc == -1 &&
            t.ric_w2 == -1 && t.admm_res == -1 && t.admm_res_max == 256 && t.admm_iter2 == -1 && t.admm_prep_ilp == -1 &&
            t.admm_prep_ilp_max == 1024 && t.ipm_mode == 1 && t.ls_waves == 0 && t.ls_tail == 0 && !t.use_graph &&
            !t.generic && t.h2h_chunks == 0 && t.pipeline == I7M_PIPE_AUTO,
        "defaults");
  auto retired = [&](const char* name, const char* value) {
    setenv(name, value, 1);
    std::string e;
    Tuning tt;
    const bool ok = tuning_from_env(cfg, &tt, &e);
    CHECK(!ok, "%s=%s accepted", name, value);
    CHECK(e.find(name) != std::string::npos && e.find("retired") != std::string::npos, "%s=%s message: %s", name, value,
          e.c_str());
    unsetenv(name);
  };
  for (const char* k : kRetired) retired(k, "2");
  retired("I7M_ADMM_STAGGER", "3");
  retired("I7M_ADMM_STAGGER", "4");
  // the surviving values parse as before
  setenv("I7M_RIC_BC", "5", 1);
  setenv("I7M_ADMM_STAGGER", "2", 1);
  setenv("I7M_ADMM_STAGGER_MIN_B", "1", 1);
  CHECK(tuning_from_env(cfg, &t, &err), "surviving knobs: %s", err.c_str());
  CHECK(t.ric_bc == 1 && riccati_variant(t, 4096, false).bc == 1, "I7M_RIC_BC=5 -> %d", t.ric_bc);
  CHECK(t.admm_stagger == 2 && t.admm_stagger_min_b == 2, "stagger %d min_b %d", t.admm_stagger, t.admm_stagger_min_b);
  for (const char* k : {"I7M_RIC_BC", "I7M_ADMM_STAGGER", "I7M_ADMM_STAGGER_MIN_B"}) unsetenv(k);
  cfg.h2h_chunks = 65;
  CHECK(!tuning_from_env(cfg, &t, &err) && err.find("h2h_chunks") != std::string::npos, "h2h_chunks = 65 accepted");
}

// I7M_ABLATE values of the diagnostic library: the retired Riccati / line-search ones say so, the
// OSQP and interior-point ones stay known, one that no kernel ever looked at is unknown
static void ablation_values() {
  for (int v : {1, 2, 4, 6, 8, 10, 11, 13, 18, 19}) {
    const AblateStatus s = ablate_status(v);
    CHECK(s.kind == Ablate::retired && s.msg && std::string(s.msg).find("retired") != std::string::npos,
          "ablate %d: kind %d message %s", v, (int)s.kind, s.msg ? s.msg : "(none)");
  }
  for (int v : {0, 21, 40, 41, 42, 43, 44, 100000 + 100 * 3 + 2, 200000 + 5, 300000 + 4}) {
    const AblateStatus s = ablate_status(v);
    CHECK(s.kind == Ablate::known && !s.msg, "ablate %d: kind %d", v, (int)s.kind);
  }
  for (int v : {3, 5, 20, 39, 45, -1}) {
    const AblateStatus s = ablate_status(v);
    CHECK(s.kind == Ablate::unknown && s.msg && std::string(s.msg).find("retired") == std::string::npos,
          "ablate %d: kind %d message %s", v, (int)s.kind, s.msg ? s.msg : "(none)");
  }
}

// carve: every offset a multiple of 256, no two sub-buffers overlapping, the total covering the last
static void check_carve(const std::vector<size_t>& bytes, const char* what) {
  std::vector<size_t> off(bytes.size(), ~(size_t)0);
  const size_t total = carve(bytes.data(), (int)bytes.size(), off.data());
  for (size_t i = 0; i < bytes.size(); ++i) {
    CHECK(off[i] % 256 == 0, "%s: offset %zu = %zu", what, i, off[i]);
    CHECK(off[i] + bytes[i] <= total, "%s: sub-buffer %zu [%zu, +%zu) past the total %zu", what, i, off[i], bytes[i], total);
    for (size_t j = 0; j < i; ++j)
      CHECK(off[j] + bytes[j] <= off[i] || off[i] + bytes[i] <= off[j], "%s: sub-buffers %zu and %zu overlap", what, j, i);
  }
}

static void workspace() {
  check_carve({}, "no request");
  check_carve({0}, "one empty request");
  check_carve({0, 1, 0, 255, 256, 257, 0}, "sizes around the alignment");
  // the sampled loop's 13 sub-buffers at (G, H, N, steps): the smallest call, and the timed shape
  const int shapes[2][4] = {{1, 1, 2, 0}, {256, 16, 32, 20}};
  for (const auto& s : shapes)
    for (int noise = 0; noise < 2; ++noise) {
      size_t bytes[SAMPLED_WS_COUNT];
      sampled_ws_bytes(s[0], s[1], s[2], s[3], 2, 1, noise != 0, bytes);
      CHECK(SAMPLED_WS_COUNT == 13, "sampled request has %d sub-buffers", (int)SAMPLED_WS_COUNT);
      CHECK((bytes[SWS_NOISE] == 0) == (noise == 0 || s[3] == 0), "noise bytes %zu", bytes[SWS_NOISE]);
      CHECK(bytes[SWS_DIST] >= 8 * (size_t)s[0], "a run of 0 steps still has one history row");
      check_carve(std::vector<size_t>(bytes, bytes + SAMPLED_WS_COUNT), "sampled loop");
    }
  size_t bytes[MPC_WS_COUNT];
  mpc_ws_bytes(3, 2, 0, bytes);
  check_carve(std::vector<size_t>(bytes, bytes + MPC_WS_COUNT), "mpc_run");
}

int main() {
  coverage();
  pinned();
  environment();
  ablation_values();
  workspace();
  if (g_failed) {
    std::printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("plan_check OK\n");
  return 0;
}
