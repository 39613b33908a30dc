"""CPU: the tracking goal source's host plan (i7m_plan.h track_index, the schedule scans of
sampled_call_ok, tracking_ws_bytes); tests/host/tracking_window_check.cpp, built with the host
compiler (plain, and under AddressSanitizer + UBSan), holds the checks."""
from test_plan_host import run_host_check


def test_tracking_window_and_workspace(tmp_path):
    for sanitize in (False, True):
        run_host_check(tmp_path, "tracking_window_check", sanitize)
