"""CPU: the controller session's host plan (i7m_plan.h ctrl_ws_bytes, ctrl_host_bytes) and the
argument checks and refusal texts of the sampled-wrench entry points (sampled_call_ok,
sampled_refusal, ctrl_step_args_ok, ctrl_step_refusal); tests/host/ctrl_plan_check.cpp, a stand-alone
program built with the host compiler, holds the checks.  It is built twice: plain, and under
AddressSanitizer + UBSan (the argument checks read caller memory: the scans must stop at G phases,
num_steps offsets and 12 G entries of x_meas)."""
import pytest

from test_plan_host import run_host_check


@pytest.mark.parametrize("sanitize", [False, True])
def test_ctrl_plan_and_argument_checks(tmp_path, sanitize):
    run_host_check(tmp_path, "ctrl_plan_check", sanitize)
