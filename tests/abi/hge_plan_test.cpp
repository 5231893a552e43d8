// The host planning of a batch (babble_amd/csrc/hge_plan.h: the consensus calls'
// windows and blocks, the coordinate step's control block) against brute-force
// restatements: linear scans, no bisection, no merge pass, no sort.  Host only, links nothing
// of the engine (tests/test_plan.py runs it).  Prints "ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../babble_amd/csrc/hge_plan.h"

using namespace hge_plan;

static long checks = 0, fails = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    checks++;                                                            \
    if (!(c)) {                                                          \
      if (fails++ < 20) fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); \
    }                                                                    \
  } while (0)

typedef std::vector<int32_t> V32;
typedef std::vector<int64_t> V64;

// ---- rounds_at_calls: R_c = #{r : minw[r] < n_c}
static void check_rounds_at_calls(const V64& calls, const V32& minw) {
  const V32 Rc = rounds_at_calls(calls, minw);
  CHECK(Rc.size() == calls.size());
  for (size_t c = 0; c < calls.size() && c < Rc.size(); c++) {
    int n = 0;
    for (int32_t m : minw) n += (int64_t)m < calls[c] ? 1 : 0;
    CHECK(Rc[c] == n);
  }
}

// ---- plan_fame_windows (spec_of(k): the width of the k-th window)
template <typename SpecOf>
static void check_windows(const V32& Rc, int lcr, const FameWindows& w, SpecOf spec_of) {
  const int ncalls = (int)Rc.size();
  int k = 0, off = 0;
  bool reachable = true;
  for (int i = lcr + 1; ncalls > 0 && i <= Rc.back() - 2; i++) {
    int cf = -1;
    for (int c = 0; c < ncalls && cf < 0; c++)
      if (Rc[c] >= i + 2) cf = c;
    if (cf < 0) {  // no call reaches the round: it and every later one is absent
      reachable = false;
      continue;
    }
    CHECK(reachable);
    CHECK(k < w.nrounds());
    if (k >= w.nrounds()) return;
    int last = cf;
    for (int c = ncalls - 1; c > cf; c--)
      if (Rc[c] <= i + 2 + spec_of(k)) {
        last = c;
        break;
      }
    CHECK(w.round[k] == i);
    CHECK(w.cf[k] == cf);
    CHECK(w.len[k] == last - cf + 1);
    CHECK(w.len[k] >= 1);
    CHECK(w.off[k] == off);
    off += last - cf + 1;
    k++;
  }
  CHECK(k == w.nrounds());
  CHECK(w.npairs == off);
  CHECK(w.off.size() == w.round.size() && w.cf.size() == w.round.size() && w.len.size() == w.round.size());
}
static void check_uniform(const V32& Rc, int lcr, int spec) {
  check_windows(Rc, lcr, plan_fame_windows(Rc, lcr, spec), [spec](int) { return spec; });
}

// ---- ctl_layout / fill_order_map / fill_ctl
static void check_ctl_layout(int ncalls, int nrounds, int nr) {
  const CtlLayout L = ctl_layout(ncalls, nrounds, nr);
  // n_c (int64) | R_c | L_c | flags | windows | pidx | sgo: disjoint, in order, covering [0, total)
  CHECK(L.Rc == 2 * (size_t)ncalls);
  CHECK(L.Lc == L.Rc + ncalls);
  CHECK(L.flags == L.Lc + ncalls);
  CHECK(L.pr == L.flags + 4);
  CHECK(L.pr_round() == L.pr && L.pr_off() == L.pr + nrounds && L.pr_cf() == L.pr + 2 * (size_t)nrounds &&
        L.pr_len() == L.pr + 3 * (size_t)nrounds);
  CHECK(L.pidx == L.pr + 4 * (size_t)nrounds);
  CHECK(L.sgo == L.pidx + nr);
  CHECK(L.total == L.sgo + nr + 1);
}
static void check_order_map(const FameWindows& w, int rr_lo, int nr, int N) {
  V32 pidx(nr + 1, 12345), sgo(nr + 1, 12345);
  const int64_t nslot = fill_order_map(w, rr_lo, nr, N, pidx.data(), sgo.data());
  int64_t sum = 0;
  for (int q = 0; q < nr; q++) {
    int k = -1;
    for (int j = 0; j < w.nrounds(); j++)
      if (w.round[j] == rr_lo + q) k = j;
    CHECK(pidx[q] == k);
    if (sum <= kInf32) CHECK(sgo[q] == (int32_t)sum);
    sum += N + 2 + (k >= 0 ? w.len[k] : 0);
  }
  CHECK(nslot == sum);
  CHECK(sgo[nr] == (sum <= kInf32 ? (int32_t)sum : kInf32));  // clamped only past INF32
  CHECK(pidx[nr] == 12345);
}
static V32 full_block(const V64& calls, const V32& Rc, const FameWindows& w, int rr_lo, int nr, int N, int64_t* nslot) {
  V32 cc;
  const CtlLayout L = ctl_layout((int)calls.size(), w.nrounds(), nr);
  *nslot = fill_ctl(cc, L, calls.data(), Rc, w, rr_lo, N, false);
  return cc;
}
static void check_block(const V64& calls, const V32& Rc, const FameWindows& w, int rr_lo, int nr, int N) {
  int64_t nslot = 0;
  const V32 cc = full_block(calls, Rc, w, rr_lo, nr, N, &nslot);
  const int ncalls = (int)calls.size(), nrounds = w.nrounds();
  const CtlLayout L = ctl_layout(ncalls, nrounds, nr);
  CHECK(cc.size() == L.total);
  for (int c = 0; c < ncalls; c++) {
    int64_t v;
    memcpy(&v, &cc[2 * (size_t)c], 8);
    CHECK(v == calls[c]);
    CHECK(cc[L.Rc + c] == Rc[c]);
    CHECK(cc[L.Lc + c] == -1);
  }
  for (int f = 0; f < 4; f++) CHECK(cc[L.flags + f] == 0);
  for (int k = 0; k < nrounds; k++) {
    CHECK(cc[L.pr_round() + k] == w.round[k]);
    CHECK(cc[L.pr_off() + k] == w.off[k]);
    CHECK(cc[L.pr_cf() + k] == w.cf[k]);
    CHECK(cc[L.pr_len() + k] == w.len[k]);
  }
  V32 pidx(nr + 1), sgo(nr + 1);
  CHECK(fill_order_map(w, rr_lo, nr, N, pidx.data(), sgo.data()) == nslot);
  for (int q = 0; q < nr; q++) CHECK(cc[L.pidx + q] == pidx[q]);
  for (int q = 0; q <= nr; q++) CHECK(cc[L.sgo + q] == sgo[q]);
}

// ---- results
static void check_results_layout(int ncalls, int ncand, bool ord) {
  const ResultsLayout L = results_layout(ncalls, ord ? ncand : 0);
  CHECK(L.o_tx % 2 == 0);
  CHECK(L.o_tx >= 8 + (size_t)ncalls + (ord ? ncand : 0));
  CHECK(L.o_tx == ((8 + (size_t)ncalls + (ord ? ncand : 0) + 1) & ~(size_t)1));
  CHECK(L.ntxb == (ord ? (ncand + 255) / 256 : 0));
  CHECK(L.ids == 8 + (size_t)ncalls && L.header() == L.ids);
  CHECK(L.total() == L.o_tx + 2 * (size_t)L.ntxb);
  CHECK(ResultsLayout::kReceived == 0 && ResultsLayout::kUndetermined == 1 && ResultsLayout::kLcrEvents == 2 &&
        ResultsLayout::kLcr == 3 && ResultsLayout::kTx == 4 && ResultsLayout::kCounts == 8);
}

// ---- the coordinate step's control block
// the arithmetic the layout replaces, as the engine used to write it inline
static void check_coords_layout(int N, size_t nsegs, size_t up_words) {
  const CoordsCtl L = coords_ctl_layout(N, nsegs, up_words);
  const size_t n = (size_t)N;
  const size_t o_len = 4, o_plo = o_len + 2 * n, o_qlo = o_plo + n, o_lo = o_qlo + n;
  const size_t o_seg = (o_lo + 2 * n + 1 + 1) & ~(size_t)1;
  const size_t o_sb = o_seg + 2 * nsegs, o_fd = o_sb + n, size = o_fd + 2 * n + 1;
  const size_t o_up = (size + 3) & ~(size_t)3;
  CHECK(CoordsCtl::rstate == 0);
  CHECK(L.olen() == o_len && L.nlen() == o_len + n);
  CHECK(L.plo == o_plo && L.qlo == o_qlo);
  CHECK(L.fss_lo() == o_lo && L.fss_off() == o_lo + n && L.fss_total() == o_lo + 2 * n);
  CHECK(L.segs == o_seg && L.segbase == o_sb);
  CHECK(L.cand_lo() == o_fd && L.cand_hi() == o_fd + n && L.risky == o_fd + 2 * n);
  CHECK(L.up == o_up);
  CHECK(L.total == (up_words ? o_up + up_words : size));
  // regions (start, words) in order, disjoint, inside the total
  const size_t reg[][2] = {{CoordsCtl::rstate, 3}, {L.olen(), n},    {L.nlen(), n},    {L.plo, n},
                           {L.qlo, n},             {L.fss_lo(), n},  {L.fss_off(), n}, {L.fss_total(), 1},
                           {L.segs, 2 * nsegs},    {L.segbase, n},   {L.cand_lo(), n}, {L.cand_hi(), n},
                           {L.risky, 1},           {L.up, up_words}};
  size_t end = 0;
  for (const auto& r : reg) {
    if (r[1] == 0) continue;
    CHECK(r[0] >= end);
    end = r[0] + r[1];
  }
  CHECK(end <= L.total);
  CHECK(L.segs % 2 == 0);  // int2 entries
  CHECK(L.up % 4 == 0);    // 16-byte aligned records
}
// position-major, chains ascending at equal positions: a naive double loop
static std::vector<Seg> naive_segments(const V32& olen, const V32& len, int SEG) {
  std::vector<Seg> out;
  int maxlen = 0;
  for (int32_t l : len) maxlen = std::max(maxlen, (int)l);
  for (int p = 0; p < maxlen; p++)
    for (int c = 0; c < (int)len.size(); c++)
      if (p >= olen[c] && p < len[c] && (p - olen[c]) % SEG == 0) out.push_back(Seg{c, p});
  return out;
}
static void check_segments(const V32& olen, const V32& len, int SEG) {
  std::vector<Seg> segs(3, Seg{-1, -1});  // (cleared by the call)
  sweep_segments(segs, olen, len, SEG);
  const std::vector<Seg> ref = naive_segments(olen, len, SEG);
  CHECK(segs.size() == ref.size());
  for (size_t i = 0; i < segs.size() && i < ref.size(); i++)
    CHECK(segs[i].chain == ref[i].chain && segs[i].pos == ref[i].pos);
  int total = 0;
  for (size_t c = 0; c < len.size(); c++) total += seg_count(olen[c], len[c], SEG);
  CHECK((size_t)total == ref.size());
}
static void check_coords_fill(int R, const V32& olen, const V32& len, int SEG, bool with_segs, bool split,
                              size_t up_words) {
  const int N = (int)len.size();
  std::vector<Seg> segs;
  if (with_segs) sweep_segments(segs, olen, len, SEG);
  V32 clo(N), chi(N), cand;
  for (int c = 0; c < N; c++) {
    clo[c] = 1000 + 3 * c;
    chi[c] = 5000 + 7 * c;
  }
  if (split) {
    cand = clo;
    cand.insert(cand.end(), chi.begin(), chi.end());
  }
  const CoordsCtl L = coords_ctl_layout(N, segs.size(), up_words);
  V32 kc(5, 77);
  const int tot = fill_coords_ctl(kc, L, R, olen, len, segs, SEG, cand);
  CHECK(kc.size() == L.total);
  if (kc.size() != L.total) return;
  // the naive fill: every word of the block from its definition, zero elsewhere
  V32 ref(L.total, 0);
  ref[0] = R;
  int64_t sum = 0;
  for (int c = 0; c < N; c++) {
    ref[4 + c] = olen[c];
    ref[4 + N + c] = len[c];
    ref[4 + 2 * N + c] = olen[c] > 0 ? olen[c] - 1 : 0;
    // (qlo: zero as uploaded) the fss rows of a fresh walk: from position 0, chain after chain
    ref[4 + 4 * N + c] = 0;
    ref[4 + 5 * N + c] = (int32_t)sum;
    sum += len[c];
    int before = 0;  // segments of the chains below c
    for (int d = 0; d < c; d++)
      for (int k = olen[d]; k < len[d]; k += SEG) before++;
    ref[L.segbase + c] = before;
    if (split) {
      ref[L.cand_lo() + c] = clo[c];
      ref[L.cand_hi() + c] = chi[c];
    }
  }
  ref[4 + 6 * N] = (int32_t)sum;
  for (size_t i = 0; i < segs.size(); i++) {
    ref[L.segs + 2 * i] = segs[i].chain;
    ref[L.segs + 2 * i + 1] = segs[i].pos;
  }
  ref[L.risky] = -1;
  CHECK(tot == (int)sum);
  CHECK(kc == ref);
  // with segments, base[c] is where chain c's segment k sits once the list is chain-major
  if (with_segs) {
    std::vector<Seg> cm = segs;
    std::stable_sort(cm.begin(), cm.end(), [](const Seg& a, const Seg& b) { return a.chain < b.chain; });
    for (size_t i = 0; i < cm.size(); i++)
      CHECK((int)i == kc[L.segbase + cm[i].chain] + (cm[i].pos - olen[cm[i].chain]) / SEG);
  }
}

int main() {
  std::mt19937_64 rng(12345);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };

  // ---------------- the coordinate step: layout, segment list, contents
  static_assert(kTailRounds == 0 && kTailOverflow == 1 && kTailMinRound == 2 && kTailHandoffErr == 3 &&
                    kTailPartial == 4,
                "the rounds tail: four fixed words, then the partial minima");
  static_assert(kRoundsFull == 1 && kRoundsStoodDown == 4, "rstate's overflow codes");
  static_assert(sizeof(Seg) == 8, "two int32 (the kernels' int2)");
  {
    const int32_t tail[7] = {41, 0, 17, 1, 19, 12, 30};
    const RoundsTail a = parse_rounds_tail(tail, 0), b = parse_rounds_tail(tail, 3);
    CHECK(a.R == 41 && a.overflow == 0 && a.min_round == 17 && a.handoff_err == 1);
    CHECK(b.R == 41 && b.min_round == 12);  // the partial minima folded in
  }
  for (int N = 1; N <= 300; N++)
    for (int segs = 0; segs < 2; segs++)
      for (int up = 0; up < 2; up++)
        check_coords_layout(N, segs ? (size_t)rnd(1, 5000) : 0, up ? (size_t)rnd(1, 400) * 14 : 0);
  check_coords_layout(256, 156250, 0);  // a 256/10M replay's segments
  for (int it = 0; it < 600; it++) {
    const int N = it < 300 ? it + 1 : rnd(1, 300);
    const int SEG = it % 2 ? 16 : 64;
    V32 olen(N), len(N);
    for (int c = 0; c < N; c++) {
      olen[c] = it % 3 == 0 ? 0 : rnd(0, 300);                   // a fresh state | mid-stream
      len[c] = olen[c] + (rnd(0, 3) == 0 ? 0 : rnd(0, 5 * SEG));  // some chains without a new event
    }
    check_segments(olen, len, SEG);
    check_coords_fill(rnd(0, 1000), olen, len, SEG, it % 4 != 1, it % 5 == 0, it % 2 ? (size_t)rnd(1, 64) * 14 : 0);
  }
  check_segments({0, 0}, {0, 0}, 16);  // nothing new
  check_segments({5}, {6}, 64);        // one event
  check_segments({0, 63, 64, 65}, {128, 128, 128, 128}, 64);

  // ---------------- rounds_at_calls
  {
    const V32 minw = {0, 40, 90, 130, 200};
    check_rounds_at_calls({10, 50, 100, 150, 250}, minw);  // ascending
    check_rounds_at_calls({50, 50, 50, 131, 131}, minw);   // repeated
    check_rounds_at_calls({10, 150, 91, 200, 201}, minw);  // one non-ascending pair
    check_rounds_at_calls({10, 50, 100}, {});              // no round yet
    check_rounds_at_calls({1000, 2000, 1LL << 40}, minw);  // beyond every witness
    check_rounds_at_calls({0, 0, 1}, minw);                // before and at the first witness
    check_rounds_at_calls({}, minw);
  }
  for (int it = 0; it < 2000; it++) {
    V32 minw(rnd(0, 40));
    int v = 0;
    for (auto& m : minw) m = (v += rnd(1, 50)) - 1;
    V64 calls(rnd(1, 30));
    for (auto& c : calls) c = rnd(0, v + 60);
    const int mode = it % 3;  // ascending | one non-ascending pair | any order
    if (mode < 2) std::sort(calls.begin(), calls.end());
    if (mode == 1 && calls.size() > 2) std::swap(calls[calls.size() / 2], calls[calls.size() / 2 - 1]);
    check_rounds_at_calls(calls, minw);
  }

  // ---------------- plan_fame_windows
  {
    // one call: every window has length 1 and ends at the last call
    const FameWindows w = plan_fame_windows(V32{9}, 2, 3);
    CHECK(w.nrounds() == 5 && w.npairs == 5);
    for (int k = 0; k < w.nrounds(); k++) CHECK(w.round[k] == 3 + k && w.cf[k] == 0 && w.len[k] == 1 && w.off[k] == k);
    check_uniform({9}, 2, 3);
    // R_c jumping by more than spec + 1 in one call: the window is its first call alone
    const V32 jump = {2, 3, 12, 13, 14};
    const FameWindows wj = plan_fame_windows(jump, -1, 3);
    CHECK(wj.nrounds() == 13 && wj.cf[2] == 2 && wj.len[2] == 1);  // round 2: R_c = 12 > 2 + 2 + 3
    check_uniform(jump, -1, 3);
    check_uniform(jump, -1, 1);
    check_uniform({2, 2, 3, 4, 4, 5, 7, 8}, -1, 3);              // lcr = -1
    CHECK(plan_fame_windows(V32{3, 4, 6}, 4, 3).nrounds() == 0);  // lcr >= Rc.back() - 2: no rounds
    CHECK(plan_fame_windows(V32{3, 4, 6}, 9, 3).nrounds() == 0);
    CHECK(plan_fame_windows(V32{3, 4, 6}, 3, 3).nrounds() == 1);
    check_uniform({3, 4, 6}, 4, 3);
    CHECK(plan_fame_windows(V32{}, -1, 3).nrounds() == 0);
    CHECK(plan_fame_windows(V32{0, 1, 1}, -1, 3).nrounds() == 0);
    // per-round widths of 1, 2, 4 mixed
    const V32 Rc = {2, 3, 3, 4, 5, 6, 6, 7, 9, 10, 11, 12};
    const std::vector<int> mixed = {1, 2, 4, 1, 2, 4, 4, 2, 1, 1, 2};
    const FameWindows wm = plan_fame_windows(Rc, -1, mixed);
    CHECK(wm.nrounds() == 11);
    check_windows(Rc, -1, wm, [&](int k) { return mixed[k]; });
  }
  for (int it = 0; it < 3000; it++) {
    V32 Rc(rnd(1, 40));
    int r = rnd(0, 4);
    for (auto& x : Rc) x = (r += (rnd(0, 9) == 0 ? rnd(0, 8) : rnd(0, 2)));
    const int lcr = rnd(-1, std::max(0, Rc.back()));
    check_uniform(Rc, lcr, it % 2 ? 3 : 1 << rnd(0, 3));
    // a selective pass and its widening: the round set and cf stay, no len shrinks
    const FameWindows a = plan_fame_windows(Rc, lcr, 1);
    std::vector<int> spec_r(a.nrounds(), 1);
    check_windows(Rc, lcr, plan_fame_windows(Rc, lcr, spec_r), [](int) { return 1; });
    for (int pass = 0; pass < 2; pass++) {
      const FameWindows before = plan_fame_windows(Rc, lcr, spec_r);
      for (auto& s : spec_r)
        if (rnd(0, 2) == 0) s *= 2;
      const FameWindows wide = plan_fame_windows(Rc, lcr, spec_r);
      check_windows(Rc, lcr, wide, [&](int k) { return spec_r[k]; });
      CHECK(wide.round == before.round);
      CHECK(wide.cf == before.cf);
      for (int k = 0; k < wide.nrounds() && k < before.nrounds(); k++) CHECK(wide.len[k] >= before.len[k]);
      // the control blocks of the two passes differ only in [pr, total); a windows-only
      // fill over the first block gives the second
      V64 calls(Rc.size());
      for (size_t c = 0; c < calls.size(); c++) calls[c] = 100 * (int64_t)c + 7;
      const int rr_lo = rnd(0, 6), nr = rnd(0, 20), N = rnd(1, 256);
      int64_t ns0 = 0, ns1 = 0;
      V32 c0 = full_block(calls, Rc, before, rr_lo, nr, N, &ns0);
      const V32 c1 = full_block(calls, Rc, wide, rr_lo, nr, N, &ns1);
      const CtlLayout L = ctl_layout((int)calls.size(), wide.nrounds(), nr);
      CHECK(c0.size() == c1.size() && c1.size() == L.total);
      for (size_t i = 0; i < L.pr && i < c0.size() && i < c1.size(); i++) CHECK(c0[i] == c1[i]);
      CHECK(fill_ctl(c0, L, calls.data(), Rc, wide, rr_lo, N, true) == ns1);
      CHECK(c0 == c1);
    }
  }

  // ---------------- ctl_layout
  for (int R = 0; R < 40; R++)
    for (int Q = 0; Q < 40; Q += 3) {
      const CtlLayout L = ctl_layout(1, R, Q);  // the online call's block
      CHECK(L.Rc == 2 && L.Lc == 3 && L.flags == 4 && L.pr == 8 && L.pidx == 8 + 4 * (size_t)R &&
            L.sgo == 8 + 4 * (size_t)R + Q && L.total == 8 + 4 * (size_t)R + 2 * (size_t)Q + 1);
    }
  for (int it = 0; it < 2000; it++) check_ctl_layout(rnd(1, 50000), rnd(0, 4000), rnd(0, 4000));

  // ---------------- pidx / sgo / nslot, and the whole block
  for (int it = 0; it < 2000; it++) {
    V32 Rc(rnd(1, 30));
    int r = rnd(0, 4);
    for (auto& x : Rc) x = (r += rnd(0, 2));
    const int lcr = rnd(-1, 6);
    const FameWindows w = it % 7 == 0 ? FameWindows() : plan_fame_windows(Rc, lcr, 1 << rnd(0, 2));
    const int rr_lo = rnd(0, 8), nr = rnd(0, 25), N = rnd(1, 256);
    check_order_map(w, rr_lo, nr, N);
    V64 calls(Rc.size());
    for (size_t c = 0; c < calls.size(); c++) calls[c] = ((int64_t)1 << 33) + 1000 * (int64_t)c;
    check_block(calls, Rc, w, rr_lo, nr, N);
  }
  {
    const FameWindows w = plan_fame_windows(V32{4, 5, 6, 9}, -1, 3);
    check_order_map(w, 0, 0, 16);   // no round to examine: sgo[0] = 0
    check_order_map(w, 3, 9, 16);   // rounds past the last window
    check_order_map(w, 20, 4, 16);  // no window among them
    // totals at and past INF32 (a width chosen to land on it): clamped only past it
    check_order_map(FameWindows(), 0, 1, kInf32 - 2);
    check_order_map(FameWindows(), 0, 2, kInf32 - 2);
    check_order_map(FameWindows(), 0, 3000, 1 << 20);
  }

  // ---------------- results
  for (int ncalls = 1; ncalls < 40; ncalls++)
    for (int ncand = 0; ncand < 600; ncand += 7) {
      check_results_layout(ncalls, ncand, true);
      check_results_layout(ncalls, ncand, false);
    }
  check_results_layout(39063, 10000000, true);
  {
    const ResultsLayout L = results_layout(2, 300);
    V32 blk(L.total(), 0);
    blk[0] = 3;
    blk[1] = 297;
    blk[2] = 11;
    blk[3] = 5;
    blk[8] = 1;
    blk[9] = 2;
    blk[10] = 70;
    blk[11] = 71;
    blk[12] = 72;
    const unsigned long long tx[2] = {(1ull << 33) + 5, 9};
    memcpy(&blk[L.o_tx], tx, 16);
    const Results r = parse_results(L, blk.data(), blk.data() + L.o_tx);
    CHECK(r.nrecv == 3 && r.n_und == 297 && r.lcr_events == 11 && r.lcr == 5);
    CHECK(r.counts[0] == 1 && r.counts[1] == 2);
    CHECK(r.ids[0] == 70 && r.ids[2] == 72);
    CHECK(L.ntxb == 2 && r.ntx == (1ull << 33) + 14);
    CHECK(parse_results(L, blk.data(), nullptr).ntx == 0);  // (the header alone came back)
  }

  if (fails) {
    fprintf(stderr, "%ld of %ld checks failed\n", fails, checks);
    return 1;
  }
  printf("ok %ld\n", checks);
  return 0;
}
