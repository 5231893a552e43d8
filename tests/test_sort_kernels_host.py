"""The host side of tests/abi/hge_sort_kernel_test.hip and hge_batch_sort_kernel_test.hip, on
the CPU: the generated buckets give what each kind promises (sorted neighbours with equal
packed words or prefixes, real keys that pack to the padding word in a padded bucket,
buckets on both sides of the packing and prefix rules, two-half buckets with one half of
each verdict), the host model of each sort equals std::sort over the full key, and every
wrong reading of a rule (timestamps compared unsigned, ties settled by the id without
S's lower limbs, padding before a real key of equal word, packable at wr + wc <= 33, a
prefix at a round span of 16 or a timestamp span of 2^28, the timestamp span taken in
wrapped signed 64-bit) changes the order of some bucket, so the device comparison can
tell them apart.  The kernels themselves run in test_gpu_sort_kernels.py."""
import os
import subprocess

import sort_kernel_cases as sc


def host_lines(exe):
    assert os.path.exists(exe), "built by __graft_entry__.build() (babble_amd/csrc/Makefile)"
    out = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.splitlines()
    assert lines[-1].startswith("ok "), out.stdout
    kinds = {}
    for ln in lines:
        if ln.startswith("host kind="):
            _, kv = sc.fields(ln)
            kinds[kv["kind"]] = kv
    return kinds, int(lines[-1].split()[1])


def test_main_generator_reaches_the_edges_and_tells_wrong_readings_apart():
    kinds, keys = host_lines(sc.MAIN_EXE)
    assert list(kinds) == sc.MAIN_KINDS
    assert keys == sc.main_keys()
    for name, kv in kinds.items():
        sizes = sc.main_sizes_of(name)
        assert (kv["buckets"], kv["keys"]) == (len(sizes), sum(sizes)), name
    parts = lambda name: sum(1 if n <= 8192 else 2 for n in sc.main_sizes_of(name) if 512 < n <= 16384)
    for name in sc.MAIN_W32:  # on the boundary, packed: a real key packs to the padding word beside padding
        kv = kinds[name]
        assert kv["packable"] == parts(name) and kv["unpackable"] == 0 and kv["padword"] > 0, kv
        assert kv["differ_padding_first"] > 0, kv
    for name in sc.MAIN_W33:  # one bit past it: the index sort
        kv = kinds[name]
        assert kv["unpackable"] == parts(name) and kv["packable"] == 0 and kv["differ_packable_at_33"] > 0, kv
    assert kinds["cts_sign"]["differ_cts_unsigned"] > 0 and kinds["cts_sign"]["unpackable"] > 0
    assert kinds["equal_words"]["eqpairs"] > 0 and kinds["equal_words"]["differ_ties_by_id"] > 0
    for name in sc.MAIN_HALVES:
        kv = kinds[name]
        assert kv["mixed_halves"] == kv["buckets"] == 5 and kv["packable"] == kv["unpackable"] == 5, kv


def test_batch_generator_reaches_the_edges_and_tells_wrong_readings_apart():
    kinds, keys = host_lines(sc.BATCH_EXE)
    assert list(kinds) == sc.BATCH_KINDS
    assert keys == sc.batch_keys()
    lds = sum(1 for n in sc.BATCH_SIZES if n <= 4096)
    for name, kv in kinds.items():
        assert (kv["buckets"], kv["keys"]) == (len(sc.BATCH_SIZES), sum(sc.BATCH_SIZES)), name
        assert kv["hbm"] == len(sc.BATCH_SIZES) - lds and kv["fits"] + kv["unfit"] == lds, kv
    for name in ("plain", "round_span_15", "cts_span_2p28_less_1", "equal_prefix"):
        assert kinds[name]["fits"] == lds, kinds[name]
    for name in ("round_span_16", "round_span_40", "cts_span_2p28", "cts_min_max", "cts_span_past_2p63"):
        assert kinds[name]["unfit"] > 0, kinds[name]
    assert kinds["equal_prefix"]["eqpairs"] > 0
    for reading, where in sc.BATCH_READINGS.items():
        for name in where:
            assert kinds[name]["differ_" + reading] > 0, (reading, kinds[name])
