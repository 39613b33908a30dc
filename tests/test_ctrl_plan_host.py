"""CPU: the controller session's host plan (i7m_plan.h ctrl_ws_bytes, ctrl_host_bytes,
ctrl_begin_args_ok, ctrl_step_args_ok); tests/host/ctrl_plan_check.cpp, a stand-alone program built
with the host compiler, holds the checks.  It is built twice: plain, and under AddressSanitizer +
UBSan (the argument checks read caller memory: the scan of x_meas must stop at 12 G)."""
import os
import subprocess

import pytest

from test_plan_host import _host_compiler

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "ctrl_plan_check.cpp")


@pytest.mark.parametrize("sanitize", [False, True])
def test_ctrl_plan_and_argument_checks(tmp_path, sanitize):
    exe = str(tmp_path / "ctrl_plan_check")
    cxx = _host_compiler()
    flags = []
    if sanitize:
        # the sanitizer runtimes linked statically (clang's default), so the program stands alone
        static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ctrl_plan_check OK" in run.stdout
