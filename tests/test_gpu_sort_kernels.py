"""The sort kernels alone on the device (tests/abi/hge_sort_kernel_test.hip,
hge_batch_sort_kernel_test.hip): k_bucket_sort (skip_big), k_bucket_sort_big and
k_bucket_sort_all (packed and with force_index) over one list of buckets of 1 .. 20,000
keys on every size switch, and kb_sort<64,0,1024>, kb_sort<256,0,1024> and
kb_sort<256,1024,4096> with and without delivery over a work list of buckets of 1 .. 8,193
keys in three graphs; the keys' ranges on the packing rule wr + wc = 32 / 33 and the prefix
rule (a round span of 15 / 16, a timestamp span of 2^28 - 1 / 2^28), timestamps across the
sign and 2^63 ns and more apart, keys equal in everything but the low limbs of S or the
id.  Every output slot against std::sort over the full key; slots outside the buckets a
launch sorts keep their sentinel.  A stream reaches none of this by
choice: a bucket's size and spans are whatever the gossip gives."""
import subprocess

import pytest

import sort_kernel_cases as sc

pytestmark = pytest.mark.gpu


def run(exe, timeout):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.splitlines()
    assert lines[-1].startswith("ok "), out.stdout
    return [sc.fields(ln) for ln in lines if ln.startswith("case ")], int(lines[-1].split()[1])


def test_main_engine_bucket_sorts_at_size_and_packing_edges():
    cases, slots = run(sc.MAIN_EXE, 120)
    assert [tuple(head) for head, _ in cases] == sc.MAIN_FORMS
    for head, kv in cases:
        form = tuple(head)
        assert (kv["buckets"], kv["keys"]) == sc.main_buckets(form), form
        if form[0] == "k_bucket_sort":
            continue  # (no path counters)
        big = sc.main_buckets(("k_bucket_sort_big", ""))[0]
        assert kv["packed"] + kv["index"] == big, (form, kv)
        if form[1] == "force_index":
            assert kv["packed"] == 0, (form, kv)
        else:
            assert kv["packed"] > 0 and kv["index"] > 0, (form, kv)
    assert slots >= sc.main_compared_slots_floor()


def test_batch_engine_bucket_sorts_at_size_and_prefix_edges():
    cases, slots = run(sc.BATCH_EXE, 120)
    assert [(head[0], kv["dlv"]) for head, kv in cases] == sc.BATCH_FORMS
    for head, kv in cases:
        form = (head[0], kv["dlv"])
        assert (kv["buckets"], kv["keys"]) == sc.batch_buckets(form), form
        assert kv["packed"] > 0 and kv["index"] > 0, (form, kv)  # buckets with and without the prefix
        assert kv["packed"] + kv["index"] + kv["hbm"] == kv["buckets"], (form, kv)
        assert (kv["hbm"] > 0) == (form[0] == "kb_sort<256,1024,4096>"), (form, kv)
    assert slots >= sc.batch_compared_slots_floor()
