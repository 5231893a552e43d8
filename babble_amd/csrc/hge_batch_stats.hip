// hge_batch_stats.hip — a run's consensus-latency statistics reduced on the device
// (hge_batch_stats in include/hge.h; the definitions: hge_stats.h).
// Included by hge_batch.hip inside namespace hgb.
//
// After a run every input is in HBM: round, rr, cts, ts, cr and ix per event, the
// accepted counts at the call points, the witness and fame tables and the scalars.  The
// call that committed an event is rcall (chain layout, at (cr[x], ix[x])) where the bulk
// path ordered the graph and xcc (event layout, written by kb_consensus) where the graph
// was replayed call by call; `path` says which per graph.  The kernels never read the
// commit stream (order, counts, ord_rr, ord_cts): with delivery on it lies in host memory.
//
//   ks_events   one streaming pass, grid (nb, graphs): a workgroup takes `span` events of
//               one graph, counts the four histograms in LDS (uint32), reduces the sums
//               and extremes per wave and per workgroup, and stores both as its own
//               partial row part[g][b][KS_ROW + hist_len] with plain stores.  No
//               workgroup adds into memory another one writes: nothing to clear, no
//               atomics outside LDS, and the result is the same bytes on every call.
//   ks_finish   one workgroup per graph: the graph's row (its partials combined, the
//               witness / fame counts, the scalars) and its histogram slab [g][hist_len].
//   ks_total    the slabs summed over the graphs, a thread per (bin, stripe of graphs):
//               coalesced along the bins.
// A batch of many graphs runs nb = 1 (config 5: 1,024 workgroups of ~10k events each); few
// large graphs are cut so that the device is filled (hge_batch::stats).

#include "hge_stats.h"

constexpr int KS_ROW = HGE_STATS_GRAPH_FIELDS;
constexpr int KS_BINS = 4 * HGE_STATS_MAX_BINS + 2;  // the longest histogram array
constexpr int KS_CALLS = 2048;                       // call points staged in LDS (K = 1 tests: ~1,200; config 5: ~330)
constexpr int KS_NT = 256;

struct ST {
  hge_stats_spec s;
  int N, ccap, G, nb;  // nb: workgroups per graph
  int64_t span;        // events per workgroup
  const GDesc* gd;
  const int32_t *round, *rr, *cr, *ix, *rcall, *xcc, *W, *path;
  const int64_t *cts, *ts, *calls, *scal;
  const int8_t* fame;
  int64_t* part;  // [g][b][KS_ROW + hist_len]
  int64_t* out;   // [hist_len] totals | [g][KS_ROW] rows | [g][hist_len] slabs
};

__device__ __forceinline__ int64_t mx64(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t mn64(int64_t a, int64_t b) { return a < b ? a : b; }

// the raw accumulators of a partial row, at the final row's indices; the extremes keep
// their identities while HGE_STATS_ORDERED is 0 (ks_finish writes zeros then)
__global__ __launch_bounds__(KS_NT) void ks_events(ST t) {
  const int g = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const GDesc d = t.gd[g];
  const hge_stats_spec s = t.s;
  const int HL = (int)hge_stats::hist_len(s), K = d.K;
  __shared__ uint32_t h[KS_BINS];
  __shared__ int32_t s_calls[KS_CALLS];
  __shared__ int64_t red[KS_NT / 64][10];
  for (int j = tid; j < HL; j += KS_NT) h[j] = 0;
  const int KS = min(K, KS_CALLS);
  for (int k = tid; k < KS; k += KS_NT) s_calls[k] = (int32_t)t.calls[d.co + k];
  __syncthreads();
  auto call_at = [&](int k) -> int64_t { return k < KS_CALLS ? (int64_t)s_calls[k] : t.calls[d.co + k]; };
  const int64_t eo = d.eo, cb = (int64_t)g * t.N * t.ccap;
  const bool replayed = t.path[g] != 0;
  // this workgroup's events [lo, hi), hi <= E; lo is cut to hi (x_lo may be INT64_MAX:
  // lo + tid below must not pass the end of int64)
  const int64_t hi = mn64(mn64(s.x_hi, (int64_t)d.E), ((int64_t)b + 1) * t.span);
  const int64_t lo = mn64(mx64(s.x_lo, (int64_t)b * t.span), hi);
  const int ra = hge_stats::round_at(s), ca = hge_stats::call_at(s), la = hge_stats::lag_at(s), ta = hge_stats::ts_at(s);
  int64_t n = 0, s_dr = 0, s_dc = 0, s_lg = 0, m_dr = INT64_MIN, m_dc = INT64_MIN, m_lg = INT64_MIN;
  uint64_t s_dt = 0;
  int64_t mn_dt = INT64_MAX, mx_dt = INT64_MIN;
  for (int64_t x = lo + tid; x < hi; x += KS_NT) {
    const int rr = t.rr[eo + x];
    if (rr < 0) continue;
    const int64_t dround = (int64_t)rr - t.round[eo + x];
    const int64_t dts = (int64_t)((uint64_t)t.cts[eo + x] - (uint64_t)t.ts[eo + x]);
    int ic = 0;  // the first call with more than x events (K >= 1: something was ordered)
    for (int top = K - 1; ic < top;) {
      const int mid = (ic + top) >> 1;
      if (call_at(mid) > x) top = mid;
      else ic = mid + 1;
    }
    int cc = replayed ? t.xcc[eo + x] : t.rcall[cb + (int64_t)t.cr[eo + x] * t.ccap + t.ix[eo + x]];
    if ((unsigned)cc >= (unsigned)K) cc = ic;  // (never on a finished run: keeps call_at in bounds)
    const int64_t dcall = cc - ic, lag = call_at(cc) - 1 - x;
    atomicAdd(&h[ra + hge_stats::round_bin(dround, s.round_bins)], 1u);
    atomicAdd(&h[ca + hge_stats::call_bin(dcall, s.call_bins)], 1u);
    atomicAdd(&h[la + hge_stats::lag_bin(lag, s.lag_bin, s.lag_bins)], 1u);
    atomicAdd(&h[ta + hge_stats::ts_bin(dts, s.ts_lo, s.ts_bin, s.ts_bins)], 1u);
    n++;
    s_dr += dround;
    s_dc += dcall;
    s_lg += lag;
    s_dt += (uint64_t)dts;
    m_dr = mx64(m_dr, dround);
    m_dc = mx64(m_dc, dcall);
    m_lg = mx64(m_lg, lag);
    mn_dt = mn64(mn_dt, dts);
    mx_dt = mx64(mx_dt, dts);
  }
  {
    const int64_t v[10] = {wave_sum64(n),    wave_sum64(s_dr),  wave_max64(m_dr),           wave_sum64(s_dc),  wave_max64(m_dc),
                           wave_sum64(s_lg), wave_max64(m_lg),  wave_sum64((int64_t)s_dt),  wave_min64(mn_dt), wave_max64(mx_dt)};
    if (lane == 0)
      for (int k = 0; k < 10; k++) red[wv][k] = v[k];
  }
  __syncthreads();
  int64_t* row = t.part + ((int64_t)g * t.nb + b) * (KS_ROW + HL);
  if (tid < KS_ROW) {
    // accumulator k of red lands in field f; 0 sum, 1 max, 2 min
    int k = -1, op = 0;
    switch (tid) {
      case HGE_STATS_ORDERED: k = 0; break;
      case HGE_STATS_DROUND_SUM: k = 1; break;
      case HGE_STATS_DROUND_MAX: k = 2, op = 1; break;
      case HGE_STATS_DCALL_SUM: k = 3; break;
      case HGE_STATS_DCALL_MAX: k = 4, op = 1; break;
      case HGE_STATS_LAG_SUM: k = 5; break;
      case HGE_STATS_LAG_MAX: k = 6, op = 1; break;
      case HGE_STATS_DTS_SUM: k = 7; break;
      case HGE_STATS_DTS_MIN: k = 8, op = 2; break;
      case HGE_STATS_DTS_MAX: k = 9, op = 1; break;
      default: break;
    }
    int64_t v = 0;
    if (k >= 0) {
      v = red[0][k];
      for (int w = 1; w < KS_NT / 64; w++) {
        const int64_t u = red[w][k];
        v = op == 0 ? (int64_t)((uint64_t)v + (uint64_t)u) : op == 1 ? mx64(v, u) : mn64(v, u);
      }
    }
    row[tid] = v;
  }
  for (int j = tid; j < HL; j += KS_NT) row[KS_ROW + j] = (int64_t)h[j];
}

__global__ __launch_bounds__(KS_NT) void ks_finish(ST t) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const GDesc d = t.gd[g];
  const hge_stats_spec s = t.s;
  const int HL = (int)hge_stats::hist_len(s), C = KS_ROW + HL;
  const int64_t* part = t.part + (int64_t)g * t.nb * C;
  int64_t* rows = t.out + HL + (int64_t)g * KS_ROW;
  int64_t* slab = t.out + HL + (int64_t)t.G * KS_ROW + (int64_t)g * HL;
  __shared__ int32_t wcnt[4];
  if (tid < 4) wcnt[tid] = 0;
  __syncthreads();
  for (int j = tid; j < HL; j += KS_NT) {
    int64_t v = 0;
    for (int b = 0; b < t.nb; b++) v += part[(int64_t)b * C + KS_ROW + j];
    slab[j] = v;
  }
  // witnesses of rounds [0, Rounds()) and their fame (0 undecided, 1 famous, 2 not famous)
  const int64_t R = t.scal[(int64_t)g * 8 + 0];
  int32_t c[4] = {0, 0, 0, 0};
  for (int64_t e = tid; e < R * t.N; e += KS_NT)
    if (t.W[(int64_t)d.ro * t.N + e] >= 0) {
      c[0]++;
      const int f = t.fame[(int64_t)d.ro * t.N + e];
      c[f == 1 ? 1 : f == 2 ? 2 : 3]++;
    }
  for (int k = 0; k < 4; k++)
    if (c[k]) atomicAdd(&wcnt[k], c[k]);
  __syncthreads();
  if (tid < KS_ROW) {
    int64_t v = 0;
    const int64_t in_range = mn64(s.x_hi, (int64_t)d.E) - mn64(s.x_lo, (int64_t)d.E);
    int64_t ordered = 0;
    for (int b = 0; b < t.nb; b++) ordered += part[(int64_t)b * C + HGE_STATS_ORDERED];
    switch (tid) {
      case HGE_STATS_EVENTS: v = d.E; break;
      case HGE_STATS_IN_RANGE: v = in_range; break;
      case HGE_STATS_ORDERED: v = ordered; break;
      case HGE_STATS_CENSORED: v = in_range - ordered; break;
      case HGE_STATS_ROUNDS: v = R; break;
      case HGE_STATS_LCR: v = t.scal[(int64_t)g * 8 + 1]; break;
      case HGE_STATS_WITNESSES: v = wcnt[0]; break;
      case HGE_STATS_FAMOUS: v = wcnt[1]; break;
      case HGE_STATS_NOT_FAMOUS: v = wcnt[2]; break;
      case HGE_STATS_UNDECIDED: v = wcnt[3]; break;
      case HGE_STATS_PATH: v = t.path[g] != 0; break;
      case HGE_STATS_DROUND_SUM:
      case HGE_STATS_DCALL_SUM:
      case HGE_STATS_LAG_SUM:
      case HGE_STATS_DTS_SUM: {
        uint64_t u = 0;
        for (int b = 0; b < t.nb; b++) u += (uint64_t)part[(int64_t)b * C + tid];
        v = (int64_t)u;
        break;
      }
      case HGE_STATS_DROUND_MAX:
      case HGE_STATS_DCALL_MAX:
      case HGE_STATS_LAG_MAX:
      case HGE_STATS_DTS_MAX:
        v = INT64_MIN;
        for (int b = 0; b < t.nb; b++) v = mx64(v, part[(int64_t)b * C + tid]);
        if (!ordered) v = 0;
        break;
      case HGE_STATS_DTS_MIN:
        v = INT64_MAX;
        for (int b = 0; b < t.nb; b++) v = mn64(v, part[(int64_t)b * C + tid]);
        if (!ordered) v = 0;
        break;
      default: break;
    }
    rows[tid] = v;
  }
}

// totals[j] = the sum over the graphs of slab[g][j]: 64 bins a workgroup, 16 stripes of graphs
__global__ __launch_bounds__(1024) void ks_total(ST t) {
  const int HL = (int)hge_stats::hist_len(t.s);
  const int lane = threadIdx.x & 63, st = threadIdx.x >> 6, j = blockIdx.x * 64 + lane;
  const int64_t* slab = t.out + HL + (int64_t)t.G * KS_ROW;
  __shared__ int64_t acc[16][64];
  int64_t v = 0;
  if (j < HL)
    for (int g = st; g < t.G; g += 16) v += slab[(int64_t)g * HL + j];
  acc[st][lane] = v;
  __syncthreads();
  if (st == 0 && j < HL) {
    for (int k = 1; k < 16; k++) v += acc[k][lane];
    t.out[j] = v;
  }
}
