"""The host event log (babble_amd/csrc/hge_hostlog.h): admission (hashgraph.go:366-396)
on the insertion cases of the reference's hashgraph_test.go, each with the code and the
message the engine returns, then seeded random streams whose chain lists, last events,
known counts and packed upload records are compared with a brute-force restatement, and
a fresh-assigned log with a newly constructed one (tests/abi/hge_hostlog_test.cpp).
Plain host C++, no engine and no device: this runs in the CPU suite."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hostlog_cases_and_brute_force():
    exe = os.path.join(ROOT, "build", "hge_hostlog_test")
    assert os.path.exists(exe), "built by __graft_entry__.build() (tests/abi/Makefile)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 10000
