"""The consensus batch's host planning (babble_amd/csrc/hge_plan.h): R_c per call,
DecideFame's windows, the control block's layout and contents, the results block's
layout, and the coordinate step's control block (layout, sweep segment list,
contents) -- against brute-force restatements (tests/abi/hge_plan_test.cpp).  Plain
host C++, no engine and no device: this runs in the CPU suite."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_against_brute_force():
    exe = os.path.join(ROOT, "build", "hge_plan_test")
    assert os.path.exists(exe), "built by __graft_entry__.build() (tests/abi/Makefile)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 10000
