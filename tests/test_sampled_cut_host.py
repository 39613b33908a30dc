"""CPU: the staggered ranges' cut of the sampled closed loop (i7m_plan.h stagger_cut_grouped) never
splits a group; tests/host/sampled_cut_check.cpp, built with the host compiler, holds the checks."""
import os
import subprocess

from test_plan_host import _host_compiler

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "sampled_cut_check.cpp")


def test_grouped_stagger_cut(tmp_path):
    exe = str(tmp_path / "sampled_cut_check")
    cc = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sampled_cut_check OK" in run.stdout
