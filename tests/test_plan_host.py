"""CPU: the launch plan (indy7_mpc_amd/csrc/i7m_plan.h: which kernel variant a launch of a given
size runs, the staggered ranges, the host-to-host chunks, the environment knobs) is pure host
code.  tests/host/plan_check.cpp holds the checks; here it is built with the host compiler under
AddressSanitizer + UBSan and run as a child process.  run_host_check is the driver of every
stand-alone program under tests/host/."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_compiler():
    for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no host C++ compiler found (g++, clang++, /opt/rocm/llvm/bin/clang++)")


def run_host_check(tmp_path, name, sanitize, env=None, timeout=60):
    """Builds tests/host/<name>.cpp (a program with its own main) with the host compiler, plain or
    under AddressSanitizer + UBSan, runs it as a child process and expects its "<name> OK" line."""
    exe = str(tmp_path / (name + ("_san" if sanitize else "")))
    cxx = _host_compiler()
    flags = []
    if sanitize:
        # the sanitizer runtimes linked statically (clang's default), so the program stands alone
        static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags,
                         os.path.join(HERE, "host", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=timeout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert name + " OK" in run.stdout


def test_launch_plan_host_checks(tmp_path):
    # a clean environment for the knobs: the program sets and unsets them itself
    env = {k: v for k, v in os.environ.items() if not k.startswith("I7M_")}
    run_host_check(tmp_path, "plan_check", sanitize=True, env=env, timeout=120)
