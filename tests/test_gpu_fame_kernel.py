"""DecideFame's kernels alone on the device (tests/abi/hge_fame_kernel_test.hip):
k_fame_decide_blk<NWT> at N = 64, 128, 192, 256 and k_fame_decide<NWT> at N = 5, 16, 33,
63, 65, 96, 130, 200, 255, on synthetic witness tables whose tallies stay below the
supermajority through coin rounds (no stream reaches that at wide N: DESIGN.md,
testing), slot by slot against a plain host loop; as a whole launch, as a split part's
launch (p0 > 0, offset windows) and, for the block kernel, over a pair list.  The host
loop, and the kernel the engine picks, are then pinned to the oracle's fame on tables
built from the three one-shot streams that take coin-bit votes."""
import subprocess

import pytest

import fame_tables as ft

pytestmark = pytest.mark.gpu


def test_fame_kernels_on_split_tallies():
    out = subprocess.run([ft.EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.splitlines()
    cases = [ln.split() for ln in lines if ln.startswith("case ")]
    assert [(f[1].split("<")[0], int(f[2].split("=")[1])) for f in cases] == \
        [("k_fame_decide_blk", n) for n in ft.BLK_N] + [("k_fame_decide", n) for n in ft.ITEM_N]
    for f in cases:
        kv = dict(x.split("=") for x in f[2:])
        assert int(kv["coin_votes"]) > 0 and int(kv["post_coin_decisions"]) > 0, f
        blk = f[1].startswith("k_fame_decide_blk")
        assert kv["forms"] == ("full,part,part,plist" if blk else "full,part,part")
        assert int(kv["slots"]) == ft.PAIRS * int(kv["N"]) * (4 if blk else 3)
    assert lines[-1].startswith("ok "), out.stdout
    assert int(lines[-1].split()[1]) >= ft.compared_slots_floor()


@pytest.mark.parametrize("stream", ft.COIN_VOTE_STREAMS, ids=lambda s: f"n{s[0]}_e{s[1]}_s{s[2]}")
def test_kernel_and_host_loop_equal_oracle_on_coin_vote_streams(stream, tmp_path):
    o, blob = ft.oracle_tables(*stream)
    assert o.stats()["coin_votes"] > 0
    path = tmp_path / "tables.bin"
    path.write_bytes(blob)
    res = ft.run_tables(str(path), host=False)
    assert res["coin_votes"] > 0
    assert res["kernel"] == "k_fame_decide<1>"  # N = 5, 8: not a multiple of 64
    ft.check_against_oracle(o, res["ref"], "the host loop's decisions")
    ft.check_against_oracle(o, res["gpu"], "the kernel's decisions")
