"""The direct rounds kernel's 8-bit compare with both sides encoded against the PREVIOUS
frontier (babble_amd/csrc/hge_narrow.h; the producer of a member row stages it encoded,
before it knows the other chains' new positions), and the layout of the staged narrow
rows (tests/abi/hge_narrow_prev_test.cpp): for (LA, FD, previous base <= base) the
encoded compare equals LA >= FD unless a flag is raised, the flags are raised exactly
when a window value saturates or a finite FD lies below the previous base, and
nar_mb_word is a bijection onto the block at the three geometries, with every consuming
thread's words inside its own member's row.  Plain host C++: this runs in the CPU suite."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_narrow_compare_against_previous_base_and_staging_layout():
    exe = os.path.join(ROOT, "build", "hge_narrow_prev_test")
    assert os.path.exists(exe), "built by __graft_entry__.build() (babble_amd/csrc/Makefile)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.startswith("ok "), out.stdout
    # 400,000 random groups, and one check per word of the three blocks (twice)
    assert int(out.stdout.split()[1]) > 400000 + 2 * (64 * 16 + 128 * 32 + 256 * 64)
