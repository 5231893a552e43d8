"""The order stage's packed sort word (babble_amd/csrc/hge_sortkey.h, shared by host and
device) against the order it stands for, (roundReceived, consensus timestamp, top 32 bits
of S) inside one call's bucket (tests/abi/hge_sortkey_test.cpp): buckets whose ranges need
wr + wc = 31, 32 and 33 bits in every split, span 0, rr_min = rr_max, timestamps across the
sign flip and one jump of 2^33 ns -- the bucket must be packable exactly when
wr + wc <= 32, and in a packable bucket every pair of keys must compare by word as by the
triple and the word must decode back to it.  Plain host C++, no engine and no device:
this runs in the CPU suite."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sort_word_order_and_packable_decision():
    exe = os.path.join(ROOT, "build", "hge_sortkey_test")
    assert os.path.exists(exe), "built by __graft_entry__.build() (babble_amd/csrc/Makefile)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.startswith("ok "), out.stdout
    # several hundred buckets of ~50 keys, every pair compared
    assert int(out.stdout.split()[1]) > 500 * 50 * 50
