// hge_commit.hip — FindOrder's commit records read back on demand (hge_commit_records).
//
// FindOrder hands its caller events, each with its roundReceived and consensusTimestamp
// (hashgraph.go:723-760), the timestamp being the source event's own Body.Timestamp
// (MedianTimestamp, hashgraph.go:762-770).  The records are a read of persisted state, taken
// after the order exists: rr and cts are stored per event, and the fame of a round at or
// below LastConsensusRound is final (the argument on k_cts_source, hge_kernels.hip), so a
// record read later equals the record at commit time.  No ordering kernel changes for it and
// nothing here runs unless a caller asks.
//
// The kernels read through la_at / fd_at and the chain tables only: one body serves the int32
// LA/FD rows (N <= 32), LA16 with int32 FD, LA16 with FD16 and the int32 positions of
// hge_wide32.hip.  FDTD / FDTW are never read: after a bulk replay at N > 128 they are stale
// (fdtd_stale), and a record read must not pay ensure_fdtd()'s full pass.
#pragma once

namespace hge {

// Records without sources: one thread per record, two gathers.
__global__ void __launch_bounds__(256) k_commit_records_plain(const int32_t* __restrict__ ids, int n,
                                                              const int32_t* __restrict__ rr,
                                                              const int64_t* __restrict__ cts,
                                                              int32_t* __restrict__ rr_out,
                                                              int64_t* __restrict__ cts_out) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int x = ids[q];
  if (rr_out) rr_out[q] = rr[x];
  if (cts_out) cts_out[q] = cts[x];
}

// Records with sources: record q of the log range goes to a group of G = min(64, next power
// of two >= N) lanes, lane = creator d, so a wave handles 64 / G records (group-masked
// ballots); above N = 64 the one group of a wave strides over d by 64 as k_cts_source does.
// The source rule is k_cts_source's: the candidates are (d, FD[x][d]) for the famous
// witnesses W[rr][d] that see x, the source the candidate of lowest d whose own timestamp is
// cts[x] (-1: none, an event with no round received).  Consecutive records share rr (a batch
// is sorted by round received first): the W / fame row of a group's round is the same row for
// the groups next to it.
template <int G>
__global__ void __launch_bounds__(256) k_commit_records(Tables t, const int32_t* __restrict__ ids, int n,
                                                        const int32_t* __restrict__ rr,
                                                        const int64_t* __restrict__ cts,
                                                        int32_t* __restrict__ rr_out,
                                                        int64_t* __restrict__ cts_out,
                                                        int32_t* __restrict__ src_out) {
  constexpr int PER = 256 / G;  // records per block
  const int lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane & ~(G - 1);
  const int q = blockIdx.x * PER + (int)(threadIdx.x / G);
  const bool on = q < n;  // (every lane of the wave takes every ballot)
  const uint64_t gmask = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1)) << gbase;
  int x = 0, r = -1, cx = 0, ix = 0;
  int64_t c = 0;
  if (on) {
    x = ids[q];
    r = rr[x];
    c = cts[x];
    cx = t.creator[x];
    ix = t.index[x];
  }
  int src = -1;
  bool done = r < 0;
  for (int d0 = 0; d0 < t.N; d0 += G) {  // one pass at N <= 64
    const int d = d0 + gl;
    bool hit = false;
    int p = 0;
    if (!done && d < t.N) {
      const int w = t.W[(size_t)r * t.N + d];
      if (w >= 0 && t.fame[(size_t)r * t.N + d] == 1 && la_at(t, d, t.index[w], cx) >= ix) {
        p = fd_at(t, (size_t)cx * t.ccap + ix, d);
        hit = p != INF32 && t.tsch[(size_t)d * t.ccap + p] == c;
      }
    }
    const uint64_t b = __ballot(hit) & gmask;
    // the wave's lane of the group's lowest hit d (none: the lane itself), outside any branch
    const int l = b ? __ffsll((unsigned long long)b) - 1 : lane;
    const int pl = __shfl(p, l);
    if (b) {  // group-uniform; a group that is done casts no hit
      src = t.chain[(size_t)(d0 + (l - gbase)) * t.ccap + pl];
      done = true;
    }
    if (G == 64 && done) break;  // (one group: wave-uniform)
  }
  if (on && gl == 0) {
    if (rr_out) rr_out[q] = r;
    if (cts_out) cts_out[q] = c;
    src_out[q] = src;
  }
}

}  // namespace hge
