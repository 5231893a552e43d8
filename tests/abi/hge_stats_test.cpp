// The bin rules and the spec check of the batch statistics (babble_amd/csrc/hge_stats.h,
// shared by host and device) at their boundaries: every clamp, the lag division, the
// timestamp bins around ts_lo and the last bin's end, ts_lo = INT64_MIN with
// dts = INT64_MAX (the difference is taken unsigned), hist_len and every refusal of the
// spec check.  Plain host C++: links nothing of the engine (tests/test_stats_host.py).
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../babble_amd/csrc/hge_stats.h"

using namespace hge_stats;

static long checks = 0, failed = 0;
#define CHECK(got, want)                                                                                   \
  do {                                                                                                     \
    const long long g_ = (long long)(got), w_ = (long long)(want);                                         \
    checks++;                                                                                              \
    if (g_ != w_) {                                                                                        \
      failed++;                                                                                            \
      fprintf(stderr, "line %d: %s = %lld, want %lld\n", __LINE__, #got, g_, w_);                          \
    }                                                                                                      \
  } while (0)

// the rule as the issue states it, in 128-bit arithmetic
static int ts_ref(int64_t dts, int64_t lo, int64_t w, int32_t bins) {
  if (dts < lo) return 0;
  const __int128 q = ((__int128)dts - (__int128)lo) / (__int128)w;
  return 1 + (int)(q < bins ? q : bins);
}

int main() {
  const hge_stats_spec ok = {16, 64, 64, 64, 100, 10000, 0, 0, INT64_MAX};
  // ---- the clamps: round and call ----
  for (int32_t bins : {1, 2, 3, 16, HGE_STATS_MAX_BINS}) {
    for (int64_t v = 0; v <= bins + 2; v++) {
      const int want = v < bins - 1 ? (int)v : bins - 1;
      CHECK(round_bin(v, bins), want);
      CHECK(call_bin(v, bins), want);
    }
    CHECK(round_bin(INT64_MAX, bins), bins - 1);
    CHECK(call_bin((int64_t)INT32_MAX + 5, bins), bins - 1);
  }
  // ---- lag: the division, then the clamp ----
  for (int64_t w : {(int64_t)1, (int64_t)2, (int64_t)100, (int64_t)4096, INT64_MAX})
    for (int32_t bins : {1, 2, 4, HGE_STATS_MAX_BINS}) {
      const int64_t vs[] = {0, 1, w - 1, w, w < INT64_MAX ? w + 1 : w, 2 * (w / 2), (bins - 1) * (w / bins),
                            w < INT64_MAX / bins ? w * (bins - 1) - 1 : 0, w < INT64_MAX / bins ? w * (bins - 1) : 0,
                            w < INT64_MAX / bins ? w * bins : 0, INT64_MAX};
      for (int64_t v : vs) {
        if (v < 0) continue;
        const int64_t q = v / w;
        CHECK(lag_bin(v, w, bins), q < bins - 1 ? q : bins - 1);
      }
    }
  CHECK(lag_bin(99, 100, 4), 0);
  CHECK(lag_bin(100, 100, 4), 1);
  CHECK(lag_bin(299, 100, 4), 2);
  CHECK(lag_bin(300, 100, 4), 3);
  CHECK(lag_bin(400, 100, 4), 3);
  // ---- ts: below ts_lo, at it, the last bin's end +- 1 ----
  for (int64_t lo : {(int64_t)0, (int64_t)-5000, (int64_t)1 << 31, -((int64_t)1 << 40), INT64_MIN, INT64_MIN + 1,
                     INT64_MAX - 1000, INT64_MAX})
    for (int64_t w : {(int64_t)1, (int64_t)3, (int64_t)10000, (int64_t)1 << 31, (int64_t)1 << 62, INT64_MAX})
      for (int32_t bins : {1, 3, 64, HGE_STATS_MAX_BINS}) {
        const __int128 end = (__int128)lo + (__int128)w * bins;  // the first value past the bins
        const __int128 cand[] = {(__int128)lo - 1, lo, (__int128)lo + 1, (__int128)lo + w - 1, (__int128)lo + w,
                                 end - 1, end, end + 1, INT64_MIN, -1, 0, 1, INT64_MAX};
        for (__int128 c : cand) {
          if (c < INT64_MIN || c > INT64_MAX) continue;
          const int64_t dts = (int64_t)c;
          CHECK(ts_bin(dts, lo, w, bins), ts_ref(dts, lo, w, bins));
        }
        if (lo > INT64_MIN) CHECK(ts_bin(lo - 1, lo, w, bins), 0);
        CHECK(ts_bin(lo, lo, w, bins), 1);
        if (end - 1 <= INT64_MAX) CHECK(ts_bin((int64_t)(end - 1), lo, w, bins), bins);
        if (end <= INT64_MAX) CHECK(ts_bin((int64_t)end, lo, w, bins), bins + 1);
        if (end + 1 <= INT64_MAX) CHECK(ts_bin((int64_t)(end + 1), lo, w, bins), bins + 1);
      }
  CHECK(ts_bin(INT64_MAX, INT64_MIN, 1, 3), 4);                      // 2^64 - 1 bins of 1 past ts_lo: the overflow bin
  CHECK(ts_bin(INT64_MAX, INT64_MIN, INT64_MAX, 3), 1 + 2);          // (2^64 - 1) / (2^63 - 1) = 2
  CHECK(ts_bin(INT64_MAX, INT64_MIN, (int64_t)1 << 62, 64), 1 + 3);  // (2^64 - 1) >> 62 = 3
  CHECK(ts_bin(INT64_MIN, INT64_MIN, 1, 3), 1);
  CHECK(ts_bin(INT64_MIN, INT64_MIN + 1, 1, 3), 0);
  // ---- the array's layout and length ----
  CHECK(hist_len(ok), 16 + 64 + 64 + 64 + 2);
  CHECK(round_at(ok), 0);
  CHECK(call_at(ok), 16);
  CHECK(lag_at(ok), 80);
  CHECK(ts_at(ok), 144);
  {
    hge_stats_spec s = ok;
    s.round_bins = s.call_bins = s.lag_bins = s.ts_bins = 1;
    CHECK(hist_len(s), 6);
    s.round_bins = s.call_bins = s.lag_bins = s.ts_bins = HGE_STATS_MAX_BINS;
    CHECK(hist_len(s), 4 * HGE_STATS_MAX_BINS + 2);
    CHECK(spec_ok(&s), 1);
  }
  // ---- the spec check: what passes, and every refusal ----
  CHECK(spec_ok(&ok), 1);
  CHECK(spec_ok(nullptr), 0);
  {
    int32_t hge_stats_spec::*const bins[4] = {&hge_stats_spec::round_bins, &hge_stats_spec::call_bins,
                                              &hge_stats_spec::lag_bins, &hge_stats_spec::ts_bins};
    for (auto m : bins) {
      for (int32_t v : {0, -1, HGE_STATS_MAX_BINS + 1, INT32_MIN, INT32_MAX}) {
        hge_stats_spec s = ok;
        s.*m = v;
        CHECK(spec_ok(&s), 0);
      }
      for (int32_t v : {1, HGE_STATS_MAX_BINS}) {
        hge_stats_spec s = ok;
        s.*m = v;
        CHECK(spec_ok(&s), 1);
      }
    }
    int64_t hge_stats_spec::*const widths[2] = {&hge_stats_spec::lag_bin, &hge_stats_spec::ts_bin};
    for (auto m : widths) {
      for (int64_t v : {(int64_t)0, (int64_t)-1, INT64_MIN}) {
        hge_stats_spec s = ok;
        s.*m = v;
        CHECK(spec_ok(&s), 0);
      }
      for (int64_t v : {(int64_t)1, INT64_MAX}) {
        hge_stats_spec s = ok;
        s.*m = v;
        CHECK(spec_ok(&s), 1);
      }
    }
    hge_stats_spec s = ok;
    s.x_lo = -1;
    CHECK(spec_ok(&s), 0);
    s.x_lo = 5, s.x_hi = 4;
    CHECK(spec_ok(&s), 0);
    s.x_lo = 5, s.x_hi = 5;  // an empty range is a range
    CHECK(spec_ok(&s), 1);
    s.x_lo = INT64_MAX, s.x_hi = INT64_MAX;
    CHECK(spec_ok(&s), 1);
    s = ok;
    s.ts_lo = INT64_MIN;  // any ts_lo passes
    CHECK(spec_ok(&s), 1);
    s.ts_lo = INT64_MAX;
    CHECK(spec_ok(&s), 1);
  }
  if (failed) {
    fprintf(stderr, "%ld of %ld checks failed\n", failed, checks);
    return 1;
  }
  printf("ok %ld\n", checks);
  return 0;
}
