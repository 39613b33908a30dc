// Host check of stagger_cut_grouped (indy7_mpc_amd/csrc/i7m_plan.h): the cut of a batch of G groups
// of H rows falls on a group boundary and on k_admm_iter's four-problem wave boundary, is the
// smallest such row count >= B / 2, and never runs past the batch.
#include <cstdio>

#include "../../indy7_mpc_amd/csrc/i7m_plan.h"

int main() {
  using namespace i7m;
  int bad = 0;
  for (int H = 1; H <= 256; H *= 2)
    for (int G = 1; G <= 300; ++G) {
      const long B = (long)G * H, L = H > 4 ? H : 4, cut = stagger_cut_grouped((int)B, H);
      const bool ok = cut >= 0 && cut <= B && cut % H == 0 && (cut == B || cut % L == 0) && 2 * cut >= B &&
                      (cut == B || 2 * (cut - L) < B);
      if (!ok) {
        std::printf("G %d H %d: cut %ld of %ld\n", G, H, cut, B);
        ++bad;
      }
    }
  // the issue's example and the test's case
  if (stagger_cut_grouped(4096, 16) != 2048 || stagger_cut_grouped(28, 4) != 16 || stagger_cut_grouped(6, 2) != 4) ++bad;
  // the default cut of existing callers is untouched
  if (stagger_cut(4096) != 2048 || stagger_cut(10) != 8) ++bad;
  if (bad) return 1;
  std::printf("sampled_cut_check OK\n");
  return 0;
}
