"""The owning buffer of the device back-ends (babble_amd/csrc/hge_own.h) over a memory
policy that counts blocks (tests/abi/hge_own_test.cpp): need's minimum capacity and its
empty state after a refused allocation; grow_keep's 1.5x rule, kept prefix and fill;
regrow_rows at every byte geometry the engine's chain tables use (4- and 8-byte elements,
packed words, uint16 rows behind an int32 element type, the run layout in an int32-sized
block, 1-byte tile flags), with a refused allocation or wait keeping the old block; moves,
swap and adopt; no block freed twice and none alive after its scope.
Plain host C++, no engine and no device: this runs in the CPU suite."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owning_buffer_rules():
    exe = os.path.join(ROOT, "build", "hge_own_test")
    assert os.path.exists(exe), "built by __graft_entry__.build() (babble_amd/csrc/Makefile)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.startswith("ok "), out.stdout
    # every byte of each regrown table alone, with and without a fill: the eight
    # geometries' blocks at 3 rows or blocks of 128 positions come to 24,192 bytes
    assert int(out.stdout.split()[1]) > 2 * 24192
