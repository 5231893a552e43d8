"""What tests/abi/hge_sort_kernel_test.hip and hge_batch_sort_kernel_test.hip are expected to
run, stated a second time: the sizes, the kinds and the launch forms, and from them the
least number of slots a full run compares.  test_sort_kernels_host.py and
test_gpu_sort_kernels.py check the programs' output against this."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN_EXE = os.path.join(ROOT, "build", "hge_sort_kernel_test")
BATCH_EXE = os.path.join(ROOT, "build", "hge_batch_sort_kernel_test")

# ---- the main engine's call-bucket sorts (hge_kernels.hip) ----
MAIN_SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096,
              4097, 8191, 8192, 8193, 8194, 12289, 16383, 16384, 16385, 16896, 16897, 20000]
MAIN_PLAIN = ["plain_random", "plain_ascending", "plain_descending", "plain_organ_pipe"]
MAIN_W32 = ["w32_0_32", "w32_4_28", "w32_16_16", "w32_31_1"]      # wr + wc = 32: packed
MAIN_W33 = ["w33_0_33", "w33_4_29", "w33_16_17", "w33_31_2"]      # wr + wc = 33: the index sort
MAIN_HALVES = ["halves_second_unpackable", "halves_first_unpackable"]
MAIN_KINDS = MAIN_PLAIN + MAIN_W32 + MAIN_W33 + ["cts_sign", "equal_words"] + MAIN_HALVES
MAIN_READINGS = ["cts_unsigned", "ties_by_id", "padding_first", "packable_at_33"]
# (kernel, form): does the form sort the buckets of up to 512 and past 16,384 keys
# (k_bucket_sort's paths), those between (k_bucket_sort_big's), and which counters move
MAIN_FORMS = [("k_bucket_sort", "skip_big"), ("k_bucket_sort_big", "packed"), ("k_bucket_sort_big", "force_index"),
              ("k_bucket_sort_all", "packed"), ("k_bucket_sort_all", "force_index")]


def main_sizes_of(kind):
    if kind in MAIN_W32 + MAIN_W33:
        return [n for n in MAIN_SIZES if 512 < n <= 16384]
    if kind in MAIN_HALVES:
        return [n for n in MAIN_SIZES if 8192 < n <= 16384]
    return MAIN_SIZES


def main_buckets(form):
    """(buckets, keys) a form sorts."""
    kernel, _ = form
    live = {"k_bucket_sort": lambda n: n <= 512 or n > 16384, "k_bucket_sort_big": lambda n: 512 < n <= 16384,
            "k_bucket_sort_all": lambda n: True}[kernel]
    sizes = [n for kind in MAIN_KINDS for n in main_sizes_of(kind) if live(n)]
    return len(sizes), sum(sizes)


def main_keys():
    return sum(sum(main_sizes_of(kind)) for kind in MAIN_KINDS)


def main_compared_slots_floor():
    # every form compares every bucket's slots (the order or the sentinel) and those between
    return len(MAIN_FORMS) * main_keys()


# ---- the batch engine's kb_sort (hge_batch_bulk.hip) ----
BATCH_SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5000,
               8192, 8193]
BATCH_KINDS = ["plain", "round_span_15", "round_span_16", "round_span_40", "cts_span_2p28_less_1", "cts_span_2p28",
               "cts_min_max", "cts_span_past_2p63", "equal_prefix"]
BATCH_READINGS = {"cts_unsigned": ["cts_min_max"], "ties_by_id": ["equal_prefix"],
                  "fits_round_span_16": ["round_span_16"], "fits_cts_span_2p28": ["cts_span_2p28"],
                  "cts_span_wrapped": ["cts_min_max", "cts_span_past_2p63"]}
BATCH_FORMS = [(k, d) for k in ("kb_sort<64,0,1024>", "kb_sort<256,0,1024>", "kb_sort<256,1024,4096>") for d in (0, 1)]


def batch_buckets(form):
    first = form[0] != "kb_sort<256,1024,4096>"
    sizes = [n for _ in BATCH_KINDS for n in BATCH_SIZES if (n <= 1024) == first]
    return len(sizes), sum(sizes)


def batch_keys():
    return len(BATCH_KINDS) * sum(BATCH_SIZES)


def batch_compared_slots_floor():
    # the ids in every form, and the two record tables with delivery
    return sum((3 if dlv else 1) * batch_keys() for _, dlv in BATCH_FORMS)


def fields(line):
    """'case NAME [word] k=v ...' -> (the words without '=', {k: v}) with v an int where it is one"""
    f = line.split()
    head = [x for x in f[1:] if "=" not in x]
    kv = dict(x.split("=") for x in f[1:] if "=" in x)
    return head, {k: int(v) if v.lstrip("-").isdigit() else v for k, v in kv.items()}
