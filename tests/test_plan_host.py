"""CPU: the launch plan (indy7_mpc_amd/csrc/i7m_plan.h: which kernel variant a launch of a given
size runs, the staggered ranges, the host-to-host chunks, the environment knobs) is pure host
code.  tests/host/plan_check.cpp holds the checks; here it is built with the host compiler under
AddressSanitizer + UBSan and run as a child process."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "plan_check.cpp")


def _host_compiler():
    for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no host C++ compiler found (g++, clang++, /opt/rocm/llvm/bin/clang++)")


def test_launch_plan_host_checks(tmp_path):
    exe = str(tmp_path / "plan_check")
    cxx = _host_compiler()
    # the sanitizer runtimes linked statically (clang's default), so the program stands alone
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", *static, SRC, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    # a clean environment for the knobs: the program sets and unsets them itself
    env = {k: v for k, v in os.environ.items() if not k.startswith("I7M_")}
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_check OK" in run.stdout
