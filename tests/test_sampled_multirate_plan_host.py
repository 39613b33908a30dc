"""CPU: the multi-rate sampled-wrench loops' host plan and argument check (i7m_plan.h
sampled_multirate_call_ok, sampled_multirate_refusal, multirate_offsets, sampled_multirate_ws_bytes);
tests/host/sampled_multirate_plan_check.cpp, a stand-alone program built with the host compiler,
holds the checks: every refusal with the argument it names, sim_dt above dt accepted, sampled_call_ok
unchanged for the single-rate kinds, the window offsets, the workspace sizes.  It is built twice:
plain, and under AddressSanitizer + UBSan."""
import pytest

from test_plan_host import run_host_check


@pytest.mark.parametrize("sanitize", [False, True])
def test_sampled_multirate_check_offsets_and_workspace(tmp_path, sanitize):
    run_host_check(tmp_path, "sampled_multirate_plan_check", sanitize)
