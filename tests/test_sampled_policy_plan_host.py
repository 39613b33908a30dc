"""CPU: the feedback policy's host plan (i7m_plan.h): the control_from check of the sampled-wrench
family and its refusal texts, the N - 2 bound of a policy-driven multi-rate call, and the argument
checks of i7m_ctrl_set_policy / i7m_ctrl_get_policy / i7m_ctrl_set_applied;
tests/host/sampled_policy_plan_check.cpp, a stand-alone program built with the host compiler, holds
the checks.  It is built twice: plain, and under AddressSanitizer + UBSan (the scan of u_applied reads
caller memory: it must stop at 6 G entries)."""
import pytest

from test_plan_host import run_host_check


@pytest.mark.parametrize("sanitize", [False, True])
def test_policy_plan_and_argument_checks(tmp_path, sanitize):
    run_host_check(tmp_path, "sampled_policy_plan_check", sanitize)
