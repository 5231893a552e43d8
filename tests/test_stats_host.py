"""The bin rules and the spec check of the batch statistics (babble_amd/csrc/hge_stats.h,
shared by host and device) at their boundaries (tests/abi/hge_stats_test.cpp): every
clamp, the lag division, dts at ts_lo - 1, ts_lo and the last bin's end +- 1,
ts_lo = INT64_MIN with dts = INT64_MAX, hist_len and every refusal of the spec check.
Plain host C++, no engine and no device: this runs in the CPU suite."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bin_rules_and_spec_check():
    exe = os.path.join(ROOT, "build", "hge_stats_test")
    assert os.path.exists(exe), "built by __graft_entry__.build() (babble_amd/csrc/Makefile)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 3000


def test_spec_mirror_matches_the_header():
    """StatsSpec is hge_stats_spec: the library's own check and length through it."""
    from babble_amd.engine import STATS_FIELDS, StatsSpec
    s = StatsSpec()
    assert s.check() == 0 and s.hist_len() == 16 + 64 + 64 + 64 + 2
    assert len(STATS_FIELDS) == 24
    for bad in (dict(round_bins=0), dict(call_bins=257), dict(lag_bin=0), dict(ts_bin=-1), dict(x_lo=-1),
                dict(x_lo=5, x_hi=4)):
        b = StatsSpec(**bad)
        assert b.check() == -8 and b.hist_len() == -8, bad
    e = StatsSpec(ts_lo=-(1 << 63), x_lo=7, x_hi=7, round_bins=1, call_bins=1, lag_bins=1, ts_bins=256)
    assert e.check() == 0 and e.hist_len() == 261
