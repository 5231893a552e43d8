// hge_plan.h — the host planning of one batch as plain C++.  The consensus calls: R_c
// per call, DecideFame's (round, call) windows, the control block's layout and
// contents, the results block's layout.  The coordinate and rounds step before them:
// its control block's layout and contents, the sweep segment list, the words of the
// rounds readback.  No HIP, no engine state: vectors and ints in, small structs out
// (hge_engine.hip includes it, and the kernels take the readback's constants from it;
// tests/abi/hge_plan_test.cpp checks it on the CPU against brute-force restatements).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace hge_plan {

constexpr int32_t kInf32 = 0x7FFFFFFF;

// R_c = Rounds() after the DivideRounds of call c = #{r : minw[r] < n_c}
// (one merge pass over the ascending calls and first witnesses: 39k binary searches
// were ~0.5 ms of idle GPU at the start of a 256/10M replay's consensus)
inline std::vector<int32_t> rounds_at_calls(const std::vector<int64_t>& calls, const std::vector<int32_t>& minw) {
  const int ncalls = (int)calls.size();
  std::vector<int32_t> Rc(ncalls);
  for (int c = 0, r = 0; c < ncalls; c++) {
    if (c > 0 && calls[c] < calls[c - 1])  // (not ascending: search afresh)
      r = (int)(std::lower_bound(minw.begin(), minw.end(), calls[c],
                                 [](int32_t m, int64_t n) { return (int64_t)m < n; }) -
                minw.begin());
    while (r < (int)minw.size() && (int64_t)minw[r] < calls[c]) r++;
    Rc[c] = r;
  }
  return Rc;
}

// DecideFame's windows: window k decides round[k] over the calls [cf[k], cf[k] + len[k]),
// its pairs at [off[k], off[k] + len[k]) of the decision table
struct FameWindows {
  std::vector<int32_t> round, off, cf, len;
  int npairs = 0;
  int nrounds() const { return (int)round.size(); }
};

// The processed rounds are lcr < i <= R_c - 2 of the last call.  Round i's window
// starts at the first call with R_c >= i + 2 (rounds no call reaches have none) and
// ends at the last call with R_c <= i + 2 + spec, never before its first call.
// spec_of(k): the width of window k.
template <typename SpecOf>
inline FameWindows plan_fame_windows_by(const std::vector<int32_t>& Rc, int lcr, SpecOf spec_of) {
  FameWindows w;
  const int ncalls = (int)Rc.size();
  if (ncalls == 0) return w;
  const int i_lo = lcr + 1, i_hi = Rc[ncalls - 1] - 2;
  int cfp = 0;
  for (int i = i_lo; i <= i_hi; i++) {
    while (cfp < ncalls && Rc[cfp] < i + 2) cfp++;
    if (cfp >= ncalls) break;
    const int sp = spec_of(w.nrounds());
    // last call with R_c <= i + 2 + sp
    int a = cfp, b = ncalls - 1;
    while (a < b) {
      int mid = (a + b + 1) / 2;
      if (Rc[mid] <= i + 2 + sp) a = mid;
      else b = mid - 1;
    }
    w.round.push_back(i);
    w.off.push_back(w.npairs);
    w.cf.push_back(cfp);
    w.len.push_back(a - cfp + 1);
    w.npairs += a - cfp + 1;
  }
  return w;
}
// one width for every round
inline FameWindows plan_fame_windows(const std::vector<int32_t>& Rc, int lcr, int spec) {
  return plan_fame_windows_by(Rc, lcr, [spec](int) { return spec; });
}
// a width per window (the selective widening's passes: the round set does not change)
inline FameWindows plan_fame_windows(const std::vector<int32_t>& Rc, int lcr, const std::vector<int>& spec_r) {
  return plan_fame_windows_by(Rc, lcr, [&spec_r](int k) { return spec_r.at(k); });
}

// The control block (int32 words): n_c (int64 each) | R_c | L_c | 4 flags | the four
// window arrays (round, off, cf, len: nrounds each) | the order pass's round -> window
// map (nr) | the per-round segment capacity offsets (nr + 1).  A widening pass keeps
// everything below `pr` and uploads [pr, total) again.
struct CtlLayout {
  int ncalls = 0, nrounds = 0, nr = 0;
  size_t Rc = 0, Lc = 0, flags = 0, pr = 0, pidx = 0, sgo = 0, total = 0;
  size_t pr_round() const { return pr; }
  size_t pr_off() const { return pr + nrounds; }
  size_t pr_cf() const { return pr + 2 * (size_t)nrounds; }
  size_t pr_len() const { return pr + 3 * (size_t)nrounds; }
};
inline CtlLayout ctl_layout(int ncalls, int nrounds, int nr) {
  CtlLayout L;
  L.ncalls = ncalls;
  L.nrounds = nrounds;
  L.nr = nr;
  L.Rc = 2 * (size_t)ncalls;
  L.Lc = L.Rc + ncalls;
  L.flags = L.Lc + ncalls;
  L.pr = L.flags + 4;
  L.pidx = L.pr + 4 * (size_t)nrounds;
  L.sgo = L.pidx + nr;
  L.total = L.sgo + nr + 1;
  return L;
}

// The order pass examines the rounds [rr_lo, rr_lo + nr).  pidx[q]: the window of round
// rr_lo + q, or -1.  sgo[q]: where the round's segments start; a round's segments start
// at call 0, at a witness arrival (<= N distinct calls), at the window start or at a
// processed call of its fame window, so its capacity is N + 2 + len.  sgo[nr] is the
// total, clamped to INF32.  Returns the total (nslot) unclamped.
inline int64_t fill_order_map(const FameWindows& w, int rr_lo, int nr, int N, int32_t* pidx, int32_t* sgo) {
  for (int q = 0; q < nr; q++) pidx[q] = -1;
  for (int k = 0; k < w.nrounds(); k++) {
    const int i = w.round[k];
    if (i >= rr_lo && i < rr_lo + nr) pidx[i - rr_lo] = k;
  }
  int64_t nslot = 0;
  for (int q = 0; q < nr; q++) {
    sgo[q] = (int32_t)nslot;
    const int k = pidx[q];
    nslot += N + 2 + (k >= 0 ? w.len[k] : 0);
  }
  sgo[nr] = (int32_t)std::min<int64_t>(nslot, kInf32);
  return nslot;
}

// The control block's contents for layout L (= ctl_layout(calls, w.nrounds(), nr)):
// the whole block (L_c = -1, flags 0), or from L.pr on when windows_only (a widening
// pass: cc holds the previous pass's block of the same layout).  Returns nslot.
inline int64_t fill_ctl(std::vector<int32_t>& cc, const CtlLayout& L, const int64_t* calls,
                        const std::vector<int32_t>& Rc, const FameWindows& w, int rr_lo, int N, bool windows_only) {
  const size_t ncalls = (size_t)L.ncalls, nrounds = (size_t)L.nrounds;
  if (!windows_only) {
    cc.assign(L.total, 0);
    memcpy(cc.data(), calls, 8 * ncalls);
    memcpy(&cc[L.Rc], Rc.data(), 4 * ncalls);
    std::fill(cc.begin() + L.Lc, cc.begin() + L.flags, -1);
  }
  if (nrounds) {
    memcpy(&cc[L.pr_round()], w.round.data(), 4 * nrounds);
    memcpy(&cc[L.pr_off()], w.off.data(), 4 * nrounds);
    memcpy(&cc[L.pr_cf()], w.cf.data(), 4 * nrounds);
    memcpy(&cc[L.pr_len()], w.len.data(), 4 * nrounds);
  }
  return fill_order_map(w, rr_lo, L.nr, N, &cc[L.pidx], &cc[L.sgo]);
}

// The results block (int32 words): an 8-word header | per-call counts | the order's
// ids (nids: the candidates when the batch orders, else 0) | per-block transaction
// sums (ntxb uint64, 8-byte aligned)
struct ResultsLayout {
  enum : size_t { kReceived = 0, kUndetermined = 1, kLcrEvents = 2, kLcr = 3, kTx = 4, kCounts = 8 };
  int ncalls = 0, ntxb = 0;
  size_t ids = 0, o_tx = 0;
  size_t header() const { return ids; }  // the header and the per-call counts
  size_t total() const { return o_tx + 2 * (size_t)ntxb; }
};
inline ResultsLayout results_layout(int ncalls, int nids) {
  ResultsLayout L;
  L.ncalls = ncalls;
  L.ids = ResultsLayout::kCounts + (size_t)ncalls;
  L.o_tx = (L.ids + (size_t)nids + 1) & ~(size_t)1;
  L.ntxb = (nids + 255) / 256;
  return L;
}

// a results block read back: `ho` the block (at least its header), `htx` the
// transaction sums (ho + o_tx when the whole block came back)
struct Results {
  int32_t nrecv = 0, n_und = 0, lcr = 0, lcr_events = 0;
  const int32_t* ids = nullptr;
  const int32_t* counts = nullptr;
  unsigned long long ntx = 0;
};
inline Results parse_results(const ResultsLayout& L, const int32_t* ho, const int32_t* htx) {
  Results r;
  r.nrecv = ho[ResultsLayout::kReceived];
  r.n_und = ho[ResultsLayout::kUndetermined];
  r.lcr_events = ho[ResultsLayout::kLcrEvents];
  r.lcr = ho[ResultsLayout::kLcr];
  r.counts = ho + ResultsLayout::kCounts;
  r.ids = ho + L.ids;
  for (int b = 0; htx && b < L.ntxb; b++) {
    unsigned long long v = 0;
    memcpy(&v, htx + 2 * (size_t)b, 8);
    r.ntx += v;
  }
  return r;
}

// ---------------------------------------------------------------------------
// The coordinate and rounds step (the half of a batch before the consensus calls)
// ---------------------------------------------------------------------------

// rstate, the first words of the step's control block: {R, overflow, new witnesses}.
// The overflow word: 0, or why the kernels after the walk stand down
constexpr int32_t kRoundsFull = 1;       // the rounds table is full: grow it, walk again
constexpr int32_t kRoundsStoodDown = 4;  // the wide walk's hand-off timed out (set with the error flag)

// The rounds readback rides behind the Rcap first-witness ids of the minw table, word
// Rcap + k: one copy brings the round count and the rounds' first witnesses back
constexpr int kTailRounds = 0;      // the round count (rstate[0])
constexpr int kTailOverflow = 1;    // rstate's overflow word
constexpr int kTailMinRound = 2;    // the lowest round of the next batch's candidates
constexpr int kTailHandoffErr = 3;  // the wide walk's hand-off error flag
constexpr int kTailPartial = 4;     // the fixed words end; k_round_tail's partial minima from here
// the tail read back (`tail`: the words from Rcap on, `mr` partial minima folded in)
struct RoundsTail {
  int32_t R = 0, overflow = 0, min_round = 0, handoff_err = 0;
};
inline RoundsTail parse_rounds_tail(const int32_t* tail, int mr) {
  RoundsTail r{tail[kTailRounds], tail[kTailOverflow], tail[kTailMinRound], tail[kTailHandoffErr]};
  for (int b = 0; b < mr; b++) r.min_round = std::min(r.min_round, tail[kTailPartial + b]);
  return r;
}

// a sweep segment: SEG positions of one chain from `pos` (the kernels read it as int2)
struct Seg {
  int32_t chain, pos;
};
inline int seg_count(int olen, int len, int SEG) { return len > olen ? (len - olen + SEG - 1) / SEG : 0; }
// The fixed-point sweeps' segment list: every chain's new positions [olen, len) in
// pieces of SEG, in position-major order (workgroups are dispatched roughly in index
// order, so early positions of every chain are swept first and later segments read
// rows already updated in this sweep: Gauss-Seidel in time order); chains keep their
// order at equal positions.
inline void sweep_segments(std::vector<Seg>& segs, const std::vector<int32_t>& olen, const std::vector<int32_t>& len,
                           int SEG) {
  segs.clear();
  for (int c = 0; c < (int)len.size(); c++)
    for (int k = olen[c]; k < len[c]; k += SEG) segs.push_back(Seg{c, k});
  std::stable_sort(segs.begin(), segs.end(), [](const Seg& a, const Seg& b) { return a.pos < b.pos; });
}

// The step's control block (int32 words, one upload): rstate (4 words) | the chains'
// old lengths, new lengths | plo (where the runs kernel starts) | qlo (where the FD
// transpose starts: written by the device past a fresh state) | the fss rows' first
// position per chain, their offsets, their total | the segment list (8-byte aligned)
// | the segments' chain-major bases | a split part's candidate bounds (low, high) |
// the one-window lastAncestors pass's risky id | an online call's packed event
// records (16-byte aligned).  up_words = 0 means "no packed upload": the block then
// ends at the risky id.  A packed upload is never empty (the step has new events and
// the upload holds exactly them), which the engine checks before it asks for a layout.
struct CoordsCtl {
  int N = 0;
  size_t nsegs = 0, up_words = 0;
  size_t len = 0, plo = 0, qlo = 0, fss = 0, segs = 0, segbase = 0, cand = 0, risky = 0, up = 0, total = 0;
  static constexpr size_t rstate = 0;
  size_t olen() const { return len; }
  size_t nlen() const { return len + N; }
  size_t fss_lo() const { return fss; }
  size_t fss_off() const { return fss + N; }
  size_t fss_total() const { return fss + 2 * (size_t)N; }
  size_t cand_lo() const { return cand; }
  size_t cand_hi() const { return cand + N; }
};
inline CoordsCtl coords_ctl_layout(int N, size_t nsegs, size_t up_words) {
  CoordsCtl L;
  L.N = N;
  L.nsegs = nsegs;
  L.up_words = up_words;
  L.len = 4;
  L.plo = L.len + 2 * (size_t)N;
  L.qlo = L.plo + N;
  L.fss = L.qlo + N;
  L.segs = (L.fss + 2 * (size_t)N + 1 + 1) & ~(size_t)1;
  L.segbase = L.segs + 2 * nsegs;
  L.cand = L.segbase + N;
  L.risky = L.cand + 2 * (size_t)N;
  L.up = (L.risky + 1 + 3) & ~(size_t)3;
  L.total = up_words ? L.up + up_words : L.risky + 1;
  return L;
}

// The block's contents for layout L (= coords_ctl_layout(N, segs.size(), ...)), the
// upload's words left zero: rstate = {R, 0, 0}; plo = olen - 1, never below 0; the fss
// entries of a walk from a fresh state (rows from position 0 of every chain; qlo = 0
// too); segment bases for pieces of SEG; `cand`: a split part's N low then N high
// bounds (empty: not a split part, zeros); the risky id -1.  Returns the fresh walk's
// fss total (every chain's length).
inline int fill_coords_ctl(std::vector<int32_t>& kc, const CoordsCtl& L, int R, const std::vector<int32_t>& olen,
                           const std::vector<int32_t>& len, const std::vector<Seg>& segs, int SEG,
                           const std::vector<int32_t>& cand) {
  const int N = L.N;
  kc.assign(L.total, 0);
  kc[CoordsCtl::rstate] = R;
  int tot = 0;
  for (int c = 0, b = 0; c < N; c++) {
    kc[L.olen() + c] = olen[c];
    kc[L.nlen() + c] = len[c];
    kc[L.plo + c] = std::max(olen[c] - 1, 0);
    kc[L.fss_off() + c] = tot;
    tot += len[c];
    kc[L.segbase + c] = b;
    b += seg_count(olen[c], len[c], SEG);
    if (!cand.empty()) {
      kc[L.cand_lo() + c] = cand[c];
      kc[L.cand_hi() + c] = cand[N + c];
    }
  }
  kc[L.fss_total()] = tot;
  if (!segs.empty()) memcpy(&kc[L.segs], segs.data(), sizeof(Seg) * segs.size());
  kc[L.risky] = -1;
  return tot;
}

}  // namespace hge_plan
