// The packed sort word of the order stage's call buckets
// (babble_amd/csrc/hge_sortkey.h) on the CPU, against the order it stands for: the
// lexicographic order by (rr, b, top 32 bits of S), which is okless restricted to its
// leading fields inside one call's bucket.
//   1. buckets of random and adversarial (rr, b, S) triples whose ranges need
//      wr + wc = 31, 32 and 33 bits (every split of them), span 0, rr_min = rr_max,
//      b across the sign flip (b = cts ^ sign: around 2^63) and at both ends of the
//      64-bit range: the bucket is packable exactly when wr + wc <= 32;
//   2. in a packable bucket every pair of keys compares by word as by the triple
//      (less, equal, greater), the word decodes back to (rr, b, S top), and no word
//      of a key with S top < 2^32 - 1 equals the padding word.
// Prints "ok <checks>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../babble_amd/csrc/hge_sortkey.h"

using namespace hge_sortkey;

static long checks = 0;
static void fail(const char* what, unsigned long long a, unsigned long long b, unsigned long long c) {
  printf("FAIL %s %llu %llu %llu\n", what, a, b, c);
  exit(1);
}

struct Key {
  uint32_t rr;
  uint64_t b, s0;
};

// the order the word stands for: -1, 0, 1
static int cmp3(const Key& x, const Key& y) {
  if (x.rr != y.rr) return x.rr < y.rr ? -1 : 1;
  if (x.b != y.b) return x.b < y.b ? -1 : 1;
  const uint32_t sx = (uint32_t)(x.s0 >> 32), sy = (uint32_t)(y.s0 >> 32);
  if (sx != sy) return sx < sy ? -1 : 1;
  return 0;
}

// bits of a span, stated without the header's loop
static int span_bits(uint64_t x) { return x == 0 ? 0 : 64 - __builtin_clzll(x); }

static void check_bucket(const std::vector<Key>& ks, int expect_packable /* -1: whatever the spans say */) {
  uint32_t rmin = 0xFFFFFFFFu, rmax = 0;
  uint64_t bmin = ~0ull, bmax = 0;
  for (const Key& k : ks) {
    rmin = k.rr < rmin ? k.rr : rmin;
    rmax = k.rr > rmax ? k.rr : rmax;
    bmin = k.b < bmin ? k.b : bmin;
    bmax = k.b > bmax ? k.b : bmax;
  }
  const SkPlan p = sk_plan(rmin, rmax, bmin, bmax);
  const int wr = span_bits(rmax - rmin), wc = span_bits(bmax - bmin);
  checks++;
  if (p.wr != wr || p.wc != wc) fail("widths", p.wr, p.wc, wr * 100 + wc);
  if (p.packable != (wr + wc <= 32)) fail("packable decision", wr, wc, p.packable);
  if (expect_packable >= 0 && (int)p.packable != expect_packable) fail("expected decision", wr, wc, p.packable);
  if (!p.packable) return;
  std::vector<uint64_t> w(ks.size());
  for (size_t i = 0; i < ks.size(); i++) {
    w[i] = sk_word(p, ks[i].rr, ks[i].b, ks[i].s0);
    // decodes back: the packing loses nothing of the three fields
    const uint64_t lead = w[i] >> 32;
    const uint64_t bm = p.wc == 0 ? 0 : (~0ull >> (64 - p.wc));
    checks++;
    if ((uint32_t)(lead >> p.wc) + p.rr_min != ks[i].rr) fail("rr decode", i, ks[i].rr, lead);
    if ((lead & bm) + p.b_min != ks[i].b) fail("b decode", i, ks[i].b, lead);
    if ((uint32_t)w[i] != (uint32_t)(ks[i].s0 >> 32)) fail("s decode", i, ks[i].s0, w[i]);
    if ((uint32_t)(ks[i].s0 >> 32) != 0xFFFFFFFFu && w[i] == kSkPad) fail("padding word", i, ks[i].s0, w[i]);
  }
  for (size_t i = 0; i < ks.size(); i++)
    for (size_t j = 0; j < ks.size(); j++) {
      const int c = cmp3(ks[i], ks[j]);
      const int cw = w[i] < w[j] ? -1 : w[i] > w[j] ? 1 : 0;
      checks++;
      if (c != cw) fail("order", i, j, (unsigned long long)(c + 1) * 10 + (cw + 1));
    }
}

static std::mt19937_64 rng(12345);

// a bucket whose rr span needs exactly wr bits and whose b span exactly wc bits, from
// rr0 and b0 up; both ends of each range present, the rest random and at the edges
static std::vector<Key> make_bucket(uint32_t rr0, int wr, uint64_t b0, int wc, int n) {
  const uint64_t rspan = wr == 0 ? 0 : ((1ull << (wr - 1)) | (rng() & ((1ull << (wr - 1)) - 1)));
  const uint64_t bspan = wc == 0 ? 0 : wc == 64 ? ((1ull << 63) | (rng() >> 1))
                                                : ((1ull << (wc - 1)) | (rng() & ((1ull << (wc - 1)) - 1)));
  std::vector<Key> ks;
  auto rnd_s = [&]() -> uint64_t {
    switch (rng() % 6) {
      case 0: return 0;
      case 1: return ~0ull;
      case 2: return 0xFFFFFFFFull;            // top 32 bits zero, low bits set
      case 3: return (rng() % 4) << 32 | rng() % 4;  // few distinct tops: ties
      default: return rng();
    }
  };
  auto pick = [&](uint64_t span) -> uint64_t {
    switch (rng() % 5) {
      case 0: return 0;
      case 1: return span;
      case 2: return span ? span - 1 : 0;
      case 3: return span ? 1 : 0;
      default: return span == ~0ull ? rng() : rng() % (span + 1);
    }
  };
  ks.push_back({rr0, b0, rnd_s()});
  ks.push_back({(uint32_t)(rr0 + rspan), b0 + bspan, rnd_s()});
  ks.push_back({rr0, b0 + bspan, rnd_s()});
  ks.push_back({(uint32_t)(rr0 + rspan), b0, rnd_s()});
  while ((int)ks.size() < n) ks.push_back({(uint32_t)(rr0 + pick(rspan)), b0 + pick(bspan), rnd_s()});
  // some exact duplicates of the leading fields
  for (int d = 0; d < 4; d++) {
    Key k = ks[rng() % ks.size()];
    if (d & 1) k.s0 ^= 1;  // same top 32 bits
    ks.push_back(k);
  }
  return ks;
}

int main() {
  const uint64_t SIGN = 0x8000000000000000ull;
  // bases: small, around the sign flip of b = cts ^ sign (cts = 0 is b = 2^63), real
  // timestamps (1.7e18 ns), and the ends of the range
  const uint64_t bbases[] = {0ull, 1ull, SIGN - 5, SIGN, SIGN + 1700000000000000000ull, SIGN - (1ull << 31)};
  const uint32_t rbases[] = {0u, 1u, 2836u, 0x7FFFFFF0u};
  for (int total : {0, 1, 12, 31, 32, 33, 40})
    for (int wr = 0; wr <= total && wr <= 32; wr++) {
      const int wc = total - wr;
      for (uint64_t b0 : bbases)
        for (uint32_t r0 : rbases) {
          // keep the ranges inside the types
          if (wr == 32 && r0 != 0) continue;
          if (wr > 0 && wr < 32 && (uint64_t)r0 + (1ull << wr) > 0xFFFFFFFFull) continue;
          if (wc < 64 && b0 + ((1ull << wc) - 1) < b0) continue;
          check_bucket(make_bucket(r0, wr, b0, wc, 48), total <= 32 ? 1 : 0);
        }
    }
  // b across the sign flip with a span that straddles it: cts from -k to +k
  for (int wc = 1; wc <= 33; wc++) {
    const uint64_t half = 1ull << (wc - 1);
    std::vector<Key> ks;
    for (int i = 0; i < 40; i++) {
      const int64_t cts = (int64_t)(rng() % (2 * half)) - (int64_t)half;  // [-half, half)
      ks.push_back({(uint32_t)(100 + i % 2), (uint64_t)cts ^ SIGN, rng()});
    }
    ks.push_back({100, (uint64_t)(-(int64_t)half) ^ SIGN, 0});
    ks.push_back({101, (uint64_t)((int64_t)half - 1) ^ SIGN, ~0ull});
    check_bucket(ks, -1);
  }
  // the widest spans: never packable
  check_bucket({{0, 0, 1}, {0xFFFFFFFFu, ~0ull, 2}}, 0);
  check_bucket({{7, 0, 1}, {7, ~0ull, 2}}, 0);
  check_bucket({{0, 5, 1}, {0xFFFFFFFFu, 5, 2}}, 1);  // wr = 32, wc = 0
  check_bucket({{3, 5, 1}, {3, 5 + 0xFFFFFFFFull, 2}}, 1);  // wr = 0, wc = 32
  check_bucket({{3, 5, 1}, {3, 5 + 0x100000000ull, 2}}, 0);  // wr = 0, wc = 33
  check_bucket({{3, 5, 1}, {4, 5 + 0xFFFFFFFFull, 2}}, 0);   // wr = 1, wc = 32
  // one timestamp jump of 2^33 ns inside a bucket of close timestamps
  {
    std::vector<Key> ks;
    for (int i = 0; i < 64; i++)
      ks.push_back({2000u, (SIGN + 1700000000000000000ull + (uint64_t)i * 1000 + (i >= 32 ? (1ull << 33) : 0)), rng()});
    check_bucket(ks, 0);
  }
  // random buckets like a replay's: a few rounds, timestamps within seconds
  for (int it = 0; it < 300; it++) {
    std::vector<Key> ks;
    const uint32_t r0 = (uint32_t)(rng() % 3000);
    const uint64_t t0 = SIGN + 1700000000000000000ull + rng() % 1000000000ull;
    const int nr = 1 + (int)(rng() % 4);
    for (int i = 0; i < 64; i++) ks.push_back({r0 + (uint32_t)(rng() % nr), t0 + rng() % 4000000000ull, rng()});
    check_bucket(ks, -1);
  }
  printf("ok %ld\n", checks);
  return 0;
}
