"""CPU: the tracking goal source's host plan (i7m_plan.h track_index, track_schedule_ok,
tracking_ws_bytes); tests/host/tracking_window_check.cpp, built with the host compiler, holds the
checks."""
import os
import subprocess

from test_plan_host import _host_compiler

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "tracking_window_check.cpp")


def test_tracking_window_and_workspace(tmp_path):
    exe = str(tmp_path / "tracking_window_check")
    cc = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "tracking_window_check OK" in run.stdout
