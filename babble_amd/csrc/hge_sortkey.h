// hge_sortkey.h — the packed sort word of the order stage's call buckets
// (packed_bitonic in hge_kernels.hip).  Plain functions that compile
// for the host and the device: the kernel plans and packs with them,
// tests/abi/hge_sortkey_test.cpp checks them on the CPU.
//
// A bucket's keys share their call, so the leading fields of the order are
//   rr  = roundReceived (low word of OKey::a),
//   b   = consensusTimestamp ^ sign (OKey::b, unsigned order),
//   s   = the top 32 bits of S (OKey::s0 >> 32).
// Inside one bucket rr and b span little: with rr_min, rr_max, b_min, b_max of the
// bucket, wr = bits(rr_max - rr_min) and wc = bits(b_max - b_min), the bucket is
// packable when wr + wc <= 32, and the sort word is
//   ((rr - rr_min) << wc | (b - b_min)) << 32 | s
// whose unsigned order is the order by (rr, b, s).  Keys with equal words are ordered
// by the full key.  Padding is the all-ones word with an index >= n; a real key may
// pack to all ones too, and then orders before the padding by its index.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGE_SK_HD __host__ __device__ __forceinline__
#else
#define HGE_SK_HD inline
#endif

namespace hge_sortkey {

constexpr uint64_t kSkPad = ~0ull;

// bits needed for x: 0 for 0, 64 for the top bit set
HGE_SK_HD int sk_bits(uint64_t x) {
  int n = 0;
  while (x) {
    n++;
    x >>= 1;
  }
  return n;
}

struct SkPlan {
  uint32_t rr_min;
  uint64_t b_min;
  int wr, wc;
  bool packable;
};

HGE_SK_HD SkPlan sk_plan(uint32_t rr_min, uint32_t rr_max, uint64_t b_min, uint64_t b_max) {
  SkPlan p;
  p.rr_min = rr_min;
  p.b_min = b_min;
  p.wr = sk_bits((uint64_t)(rr_max - rr_min));
  p.wc = sk_bits(b_max - b_min);
  p.packable = p.wr + p.wc <= 32;
  return p;
}

// the sort word of a key of a packable bucket (rr, b inside the plan's ranges)
HGE_SK_HD uint64_t sk_word(const SkPlan& p, uint32_t rr, uint64_t b, uint64_t s0) {
  // wr + wc <= 32: the leading part fits 32 bits (wc = 32 only with wr = 0, rr - rr_min = 0)
  const uint64_t lead = ((uint64_t)(rr - p.rr_min) << p.wc) | (b - p.b_min);
  return (lead << 32) | (s0 >> 32);
}

}  // namespace hge_sortkey
