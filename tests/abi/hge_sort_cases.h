// hge_sort_cases.h — what the two sort-kernel harnesses share (hge_sort_kernel_test.hip for
// the main engine's call-bucket sorts, hge_batch_sort_kernel_test.hip for the batch
// engine's kb_sort): the key as FindOrder defines it, its order written out, the bucket
// generators, and the host-side models of a sort that reads one of its rules wrongly.
// Plain host C++: nothing of the engine is used here.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

namespace sortcase {

struct Rng {
  uint64_t s;
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return next() % n; }
};

// One event's sort key: roundReceived, consensusTimestamp, S as four limbs (most
// significant first), and the id that settles what is left.
struct Key {
  uint32_t rr;
  int64_t cts;
  uint64_t s[4];
  uint32_t id;
};

// The order (consensus_sorter.go:36-59 with PRN = 0, then the id): written out here, the
// kernels' own comparators are not called.
inline bool ref_less(const Key& x, const Key& y) {
  if (x.rr != y.rr) return x.rr < y.rr;
  if (x.cts != y.cts) return x.cts < y.cts;  // signed
  for (int l = 0; l < 4; l++)
    if (x.s[l] != y.s[l]) return x.s[l] < y.s[l];  // unsigned
  return x.id < y.id;
}

// Wrong readings of the comparator (the models below take one): the timestamp compared
// unsigned; ties after the leading 32 bits of S settled by the id; ties after limb 0 of S
// settled by the id.
enum CmpMode { kCmpRight = 0, kCmpCtsUnsigned, kCmpIdAfterWord, kCmpIdAfterLimb0 };
inline bool mode_less(const Key& x, const Key& y, int mode) {
  if (mode == kCmpRight) return ref_less(x, y);
  if (x.rr != y.rr) return x.rr < y.rr;
  if (x.cts != y.cts) return mode == kCmpCtsUnsigned ? (uint64_t)x.cts < (uint64_t)y.cts : x.cts < y.cts;
  if (mode == kCmpIdAfterWord) {
    if ((x.s[0] >> 32) != (y.s[0] >> 32)) return x.s[0] < y.s[0];
    return x.id < y.id;
  }
  if (x.s[0] != y.s[0]) return x.s[0] < y.s[0];
  if (mode == kCmpIdAfterLimb0) return x.id < y.id;
  for (int l = 1; l < 4; l++)
    if (x.s[l] != y.s[l]) return x.s[l] < y.s[l];
  return x.id < y.id;
}

// bits needed for x: 0 for 0, 64 with the top bit set
inline int bits_of(uint64_t x) {
  int n = 0;
  for (; x; x >>= 1) n++;
  return n;
}

// ---------------------------------------------------------------------------
// Generators.  Each returns n keys in input order with id = 0; the caller deals the ids.
// ---------------------------------------------------------------------------
inline Key random_key(Rng& g, uint32_t rr, int64_t cts) {
  Key k;
  k.rr = rr;
  k.cts = cts;
  for (auto& l : k.s) l = g.next();
  k.id = 0;
  return k;
}

// plain: three rounds, timestamps within 2^20 ns of a real clock
inline std::vector<Key> gen_plain(int n, Rng& g) {
  std::vector<Key> k;
  const uint32_t r0 = 100 + (uint32_t)g.below(1000);
  const int64_t c0 = 1700000000000000000ll + (int64_t)g.below(1ull << 40);
  for (int i = 0; i < n; i++) k.push_back(random_key(g, r0 + (uint32_t)g.below(3), c0 + (int64_t)g.below(1ull << 20)));
  return k;
}

// Rounds spanning exactly rspan and timestamps spanning exactly cspan (< 2^63), both
// extremes present.  The corners come first, as many as fit: the least key with leading S
// bits 0, the greatest with leading S bits all ones, then (first round, last timestamp)
// and (second round, first timestamp), the pair that a timestamp field one bit too
// narrow for the span confuses.  The rest is uniform inside the ranges; a tenth repeats
// a corner's (round, timestamp).
inline std::vector<Key> gen_span(int n, uint32_t r0, uint32_t rspan, int64_t c0, uint64_t cspan, Rng& g) {
  std::vector<Key> k;
  const uint32_t r1 = r0 + rspan, rs = rspan ? r0 + 1 : r0;
  const int64_t c1 = (int64_t)((uint64_t)c0 + cspan);
  auto with_hi = [&](uint32_t rr, int64_t c, uint32_t hi) {
    Key x = random_key(g, rr, c);
    x.s[0] = ((uint64_t)hi << 32) | (x.s[0] & 0xFFFFFFFFull);
    return x;
  };
  const Key corner[4] = {with_hi(r0, c0, 0), with_hi(r1, c1, 0xFFFFFFFFu), with_hi(r0, c1, 0xFFFFFFF0u),
                         with_hi(rs, c0, 1)};
  for (int i = 0; i < n; i++) {
    if (i < 4) {
      k.push_back(corner[i]);
      continue;
    }
    if (g.below(10) == 0) {
      const Key& c = corner[g.below(4)];
      k.push_back(random_key(g, c.rr, c.cts));
      continue;
    }
    const uint32_t rr = r0 + (uint32_t)(rspan == 0xFFFFFFFFu ? g.next() : g.below((uint64_t)rspan + 1));
    const uint64_t dc = cspan == ~0ull ? g.next() : g.below(cspan + 1);
    k.push_back(random_key(g, rr, (int64_t)((uint64_t)c0 + dc)));
  }
  return k;
}

// timestamps over the whole signed range, INT64_MIN and INT64_MAX present (n >= 2), and
// the neighbours of 0
inline std::vector<Key> gen_sign(int n, Rng& g) {
  std::vector<Key> k;
  const int64_t fixed[6] = {INT64_MIN, INT64_MAX, -1, 0, 1, INT64_MIN + 1};
  const uint32_t r0 = 7;
  for (int i = 0; i < n; i++) {
    const int64_t c = i < 6 ? fixed[i] : (int64_t)g.next();
    k.push_back(random_key(g, r0 + (i < 6 ? 0 : (uint32_t)g.below(2)), c));
  }
  return k;
}

// Equal leading fields everywhere: round, timestamp and the top 32 bits of S constant.
// A fifth of the keys each differs first in the low half of limb 0, in limb 1, in limb 2,
// in limb 3, or in the id alone.
inline std::vector<Key> gen_equal(int n, Rng& g) {
  std::vector<Key> k;
  Key base = random_key(g, 41, 1700000000123456789ll);
  for (int i = 0; i < n; i++) {
    Key x = base;
    const int cls = i % 5;  // the first field that may differ from base
    if (cls == 0) x.s[0] = (base.s[0] & ~0xFFFFFFFFull) | (g.next() & 0xFFFFFFFFull);
    for (int l = 1; l < 4; l++)
      if (cls <= l && cls != 4) x.s[l] = g.next();
    k.push_back(x);
  }
  return k;
}

inline void shuffle(std::vector<Key>& k, Rng& g) {
  for (size_t i = k.size(); i > 1; i--) std::swap(k[i - 1], k[g.below(i)]);
}

// ids dealt as base + a permutation of 0 .. n - 1: unique in the bucket, unrelated to the order
inline void deal_ids(std::vector<Key>& k, uint32_t base, Rng& g) {
  std::vector<uint32_t> p(k.size());
  for (size_t i = 0; i < p.size(); i++) p[i] = (uint32_t)i;
  for (size_t i = p.size(); i > 1; i--) std::swap(p[i - 1], p[g.below(i)]);
  for (size_t i = 0; i < k.size(); i++) k[i].id = base + p[i];
}

// input orders: 0 as generated (random), 1 ascending, 2 descending, 3 organ-pipe
inline void arrange(std::vector<Key>& k, int order) {
  if (order == 0) return;
  std::sort(k.begin(), k.end(), ref_less);
  if (order == 2) std::reverse(k.begin(), k.end());
  if (order == 3) {  // rising over the even ranks, falling over the odd ones
    std::vector<Key> o(k.size());
    size_t lo = 0, hi = k.size();
    for (size_t i = 0; i < k.size(); i++) {
      if (i % 2 == 0) o[lo++] = k[i];
      else o[--hi] = k[i];
    }
    k = o;
  }
}

}  // namespace sortcase
