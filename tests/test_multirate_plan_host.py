"""CPU: the multi-rate closed loop's host plan (i7m_plan.h multirate_schedule, multirate_refusal,
multirate_ws_bytes); tests/host/multirate_plan_check.cpp, a stand-alone program built with the host
compiler, holds the checks: three schedules element for element with their float residues,
sub_start monotone, the refusals, the workspace sizes.  It is built twice: plain, and under
AddressSanitizer + UBSan (the schedule grows three vectors inside a loop that only the sub-step
bound ends for a degenerate dt)."""
import pytest

from test_plan_host import run_host_check


@pytest.mark.parametrize("sanitize", [False, True])
def test_multirate_schedule_refusals_and_workspace(tmp_path, sanitize):
    run_host_check(tmp_path, "multirate_plan_check", sanitize)
