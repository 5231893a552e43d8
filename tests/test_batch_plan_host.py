"""The batch engine's launch plan and pool layout (babble_amd/csrc/hge_batch_plan.h, what
hge_batch's run and both stages branch and size on) on the CPU
(tests/abi/hge_batch_plan_test.cpp): every row of DESIGN.md §4.8's table of instances at
its boundary and on both sides of it, at 256 compute units and at an odd count, under
HGB_SERIAL and with delivery; the layout of three hand-written batches; and the capacity
errors at INT32_MAX rounds or calls and at a chain of 2^24 events, from counts alone.
Plain host C++, no engine and no device: this runs in the CPU suite."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_rules_and_layout():
    exe = os.path.join(ROOT, "build", "hge_batch_plan_test")
    assert os.path.exists(exe), "built by __graft_entry__.build() (babble_amd/csrc/Makefile)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 5000
