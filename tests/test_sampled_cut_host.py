"""CPU: the staggered ranges' cut of the sampled closed loop (i7m_plan.h stagger_cut_grouped) never
splits a group; tests/host/sampled_cut_check.cpp, built with the host compiler (plain, and under
AddressSanitizer + UBSan), holds the checks."""
from test_plan_host import run_host_check


def test_grouped_stagger_cut(tmp_path):
    for sanitize in (False, True):
        run_host_check(tmp_path, "sampled_cut_check", sanitize)
