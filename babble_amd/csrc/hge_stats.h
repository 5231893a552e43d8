// hge_stats.h — the definitions of the batch engine's consensus-latency statistics
// (hge_batch_stats in include/hge.h).  Plain functions that compile for
// the host and the device: the reduction kernel (hge_batch_stats.hip) bins with them,
// tests/abi/hge_stats_test.cpp checks them on the CPU.
//
// For an accepted event x of a graph that the last run ordered (rr[x] >= 0):
//   dround = rr[x] - round[x]            (>= 1: DecideRoundReceived starts at round + 1,
//                                         hashgraph.go:676-721)
//   icall  = the first call c with calls[c] > x (calls: accepted counts at the call points)
//   ccall  = the call whose batch committed x
//   dcall  = ccall - icall               (>= 0)
//   lag    = calls[ccall] - 1 - x        (events accepted after x when it was committed)
//   dts    = cts[x] - ts[x]              (signed 64-bit)
// and the histograms, laid out round | call | lag | ts in one array of hist_len() bins:
//   round  bin min(dround, round_bins - 1)
//   call   bin min(dcall, call_bins - 1)
//   lag    bin min(lag / lag_bin, lag_bins - 1)
//   ts     ts_bins + 2 bins: bin 0 below ts_lo, else 1 + min((dts - ts_lo) / ts_bin, ts_bins),
//          the difference taken after the comparison and unsigned, so that it is exact
//          for every int64 dts and ts_lo
#pragma once

#include <stdint.h>

#include "../../include/hge.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGE_ST_HD __host__ __device__ __forceinline__
#else
#define HGE_ST_HD inline
#endif

namespace hge_stats {

// (values below 0 cannot occur on an ordered event; they land in bin 0)
HGE_ST_HD int32_t clamp_bin(int64_t v, int32_t bins) {
  return v < 0 ? 0 : v < (int64_t)bins - 1 ? (int32_t)v : bins - 1;
}
HGE_ST_HD int32_t round_bin(int64_t dround, int32_t round_bins) { return clamp_bin(dround, round_bins); }
HGE_ST_HD int32_t call_bin(int64_t dcall, int32_t call_bins) { return clamp_bin(dcall, call_bins); }
HGE_ST_HD int32_t lag_bin(int64_t lag, int64_t width, int32_t lag_bins) {
  return lag < 0 ? 0 : clamp_bin(lag / width, lag_bins);
}
HGE_ST_HD int32_t ts_bin(int64_t dts, int64_t ts_lo, int64_t width, int32_t ts_bins) {
  if (dts < ts_lo) return 0;
  const uint64_t q = ((uint64_t)dts - (uint64_t)ts_lo) / (uint64_t)width;
  return 1 + (q < (uint64_t)ts_bins ? (int32_t)q : ts_bins);
}

// where each histogram starts in the array
HGE_ST_HD int32_t round_at(const hge_stats_spec& s) { return 0; }
HGE_ST_HD int32_t call_at(const hge_stats_spec& s) { return s.round_bins; }
HGE_ST_HD int32_t lag_at(const hge_stats_spec& s) { return s.round_bins + s.call_bins; }
HGE_ST_HD int32_t ts_at(const hge_stats_spec& s) { return s.round_bins + s.call_bins + s.lag_bins; }

HGE_ST_HD bool spec_ok(const hge_stats_spec* s) {
  if (!s) return false;
  const int32_t b[4] = {s->round_bins, s->call_bins, s->lag_bins, s->ts_bins};
  for (int k = 0; k < 4; k++)
    if (b[k] < 1 || b[k] > HGE_STATS_MAX_BINS) return false;
  if (s->lag_bin < 1 || s->ts_bin < 1) return false;
  return s->x_lo >= 0 && s->x_lo <= s->x_hi;
}
// round + call + lag + ts + 2 bins (the spec must be spec_ok)
HGE_ST_HD int64_t hist_len(const hge_stats_spec& s) {
  return (int64_t)s.round_bins + s.call_bins + s.lag_bins + s.ts_bins + 2;
}

}  // namespace hge_stats
