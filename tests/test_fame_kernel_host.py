"""The host side of tests/abi/hge_fame_kernel_test.hip, on the CPU: the generator's
tables keep the engine's invariants and take the plain DecideFame loop through coin-bit
votes and decisions after a coin round at all 13 (kernel, N) cases; three wrong readings
of the coin branch (another witness's coin, a coin round that decides, the coin of x)
each change decisions at every case, so the device comparison can tell them apart; and
the plain loop equals the Go-faithful oracle's fame on the one-shot streams that take
coin-bit votes.  The kernels themselves run in test_gpu_fame_kernel.py."""
import os
import subprocess

import pytest

import fame_tables as ft


def test_generator_reaches_the_coin_branch_and_tells_wrong_readings_apart():
    assert os.path.exists(ft.EXE), "built by __graft_entry__.build() (babble_amd/csrc/Makefile)"
    out = subprocess.run([ft.EXE, "--host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    seen = []
    for line in out.stdout.splitlines():
        f = line.split()
        if f[0] != "host":
            continue
        kv = dict(x.split("=") for x in f[2:])
        seen.append((f[1].split("<")[0], int(kv["N"])))
        assert int(kv["pairs"]) == ft.PAIRS
        for key in ("coin_votes", "post_coin_decisions", "dec0", "dec1", "dec2", "differ_coin_slot0",
                    "differ_coin_decides", "differ_coin_of_x"):
            assert int(kv[key]) > 0, line
    assert seen == [("k_fame_decide_blk", n) for n in ft.BLK_N] + [("k_fame_decide", n) for n in ft.ITEM_N]
    assert out.stdout.splitlines()[-1].startswith("ok ")


@pytest.mark.parametrize("stream", ft.COIN_VOTE_STREAMS, ids=lambda s: f"n{s[0]}_e{s[1]}_s{s[2]}")
def test_host_loop_equals_oracle_on_coin_vote_streams(stream, tmp_path):
    o, blob = ft.oracle_tables(*stream)
    assert o.stats()["coin_votes"] > 0
    path = tmp_path / "tables.bin"
    path.write_bytes(blob)
    res = ft.run_tables(str(path), host=True)
    assert res["coin_votes"] > 0
    ft.check_against_oracle(o, res["ref"], "the host loop's decisions")
