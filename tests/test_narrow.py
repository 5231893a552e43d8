"""The direct rounds kernel's 8-bit frontier-relative compare
(babble_amd/csrc/hge_narrow.h, shared by host and device) against its plain statement,
LA >= FD per column (tests/abi/hge_narrow_test.cpp): every pair of 7-bit fields in every
lane under the guard-bit subtract, and (LA, FD, base) triples -- unset values, values
below the base, 124 .. 128 above it, positions near 65,533 -- where the encoded compare
must equal the 16-bit one unless the encoders raise the round's flag, and the flag must
be raised exactly when a window value saturates or a finite FD lies below its base.
Plain host C++, no engine and no device: this runs in the CPU suite."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_narrow_compare_against_plain_statement():
    exe = os.path.join(ROOT, "build", "hge_narrow_test")
    assert os.path.exists(exe), "built by __graft_entry__.build() (babble_amd/csrc/Makefile)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.startswith("ok "), out.stdout
    # 4 lanes x 128 x 128 x 25 neighbour kinds for the guard bits alone
    assert int(out.stdout.split()[1]) > 4 * 128 * 128 * 25
