"""Per-kernel launch durations under the diagnostic library's I7M_ABLATE values (results invalid,
timing only) at small and large batch, one SQP iteration per solve so that every launch
works on every problem whatever the ablation does to the results: python tools/ablate_ab.py [ablate ...]

The values the library still acts on are those of the OSQP iteration and of k_ipm_fused (21, 40..44;
ablate_status in csrc/i7m_plan.h).  The Riccati and line-search values (1, 2, 4, 6, 8, 10, 11, 13,
18, 19) were retired and are refused by i7m_create; DESIGN.md §7 keeps what they measured."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.small_batch_ab import run  # noqa: E402

if __name__ == "__main__":
    for a in (sys.argv[1:] or ["0"]):
        for B in (1, 64, 4096):
            r = run(B, 32, {"I7M_ABLATE": a}, steps=100 if B == 1 else 20, max_sqp_iters=1)
            print("ablate", a, "B=%d" % B, r["kernels_us"], flush=True)
