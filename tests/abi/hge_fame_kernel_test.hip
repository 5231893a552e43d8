// hge_fame_kernel_test.hip — DecideFame's kernels (k_fame_decide<NWT>,
// k_fame_decide_blk<NWT>: hge_kernels.hip) driven directly with synthetic witness
// tables whose tallies straddle the supermajority through coin rounds, against a plain
// host loop written from hashgraph.go:598-664.  Streams cannot reach this regime at
// wide N: in a one-shot call DecideFame's break leaves only the first voter of a
// deciding round with a vote, so from diff = 4 on every tally is all-nay and every
// coin round is entered with a supermajority (testing).
//
//   hge_fame_kernel_test            every (kernel, N) case, every launch form, on the device
//   hge_fame_kernel_test --host     the generator and the host loop only (no device):
//                                   the reference's coin-vote and post-coin-decision
//                                   counts, and how many decisions three wrong readings
//                                   of the coin branch would change (all must be > 0)
//   hge_fame_kernel_test --tables FILE [--host]
//                                   one table set from a file (tests/test_gpu_fame_kernel.py
//                                   writes it from a live oracle run): prints the host
//                                   loop's decisions ("ref") and the kernel's ("gpu")
//
// The file: int32 {N, rounds, ids, calls}, W int32[rounds][N], seeb then ssb
// uint64[rounds][N][NW], coin uint8[ids], n_c int64[calls], R_c int32[calls].
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>

#include "hge_plan.h"

#include "hge_kernels.hip"

#define HIPCHK(e)                                                                               \
  do {                                                                                          \
    hipError_t e_ = (e);                                                                        \
    if (e_ != hipSuccess) {                                                                     \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #e, hipGetErrorString(e_));        \
      exit(2);                                                                                  \
    }                                                                                           \
  } while (0)

namespace {

constexpr uint8_t kSentinel = 0xEE;  // a decision slot no launch may have touched

struct Rng {
  uint64_t s;
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Tab {
  int N = 0, NW = 1, SM = 1, R = 0;
  std::vector<int32_t> W;           // [R][N]
  std::vector<uint64_t> seeb, ssb;  // [R][N][NW]
  std::vector<uint8_t> coin;        // per witness id
  std::vector<int64_t> nc;
  std::vector<int32_t> Rc;
  hge_plan::FameWindows w;
  int w_at(int r, int d) const { return W[(size_t)r * N + d]; }
  bool bit(const std::vector<uint64_t>& b, int r, int d, int s) const {
    return (b[((size_t)r * N + d) * NW + (s >> 6)] >> (s & 63)) & 1ull;
  }
  void set(std::vector<uint64_t>& b, int r, int d, int s) { b[((size_t)r * N + d) * NW + (s >> 6)] |= 1ull << (s & 63); }
};

// ---------------------------------------------------------------------------
// The generator.  Slots fall into two camps, fixed over the rounds.  A voter of an
// ordinary round strongly sees its whole camp and just enough of the other one to
// reach SM slots, so a witness x whose first votes follow the camps stays split with
// no tally at SM, round after round, up to its coin round (diff = N), where every
// voter takes its coin bit.  Round N + 4 mixes (its voters share a core of SM slots):
// the votes round 3's coin round left collapse to the core's majority and decisions
// follow; for round 5 it is the round before the coin round, which is then entered
// with a supermajority nobody has decided on.
// Rounds 1 and 2 (and some later ones at N >= 16) have empty slots.
// ---------------------------------------------------------------------------
Tab generate(int N) {
  Tab T;
  T.N = N;
  T.NW = (N + 63) / 64;
  T.SM = 2 * N / 3 + 1;  // hge_engine.hip (hashgraph.go:78-80)
  T.R = 2 * N + 8;
  const int R = T.R, SM = T.SM;
  Rng g{0x5EEDull * 1000003ull + (uint64_t)N};
  T.W.assign((size_t)R * N, -1);
  T.seeb.assign((size_t)R * N * T.NW, 0);
  T.ssb.assign((size_t)R * N * T.NW, 0);
  std::vector<int64_t> first_id(R + 1), mid_id(R);
  int id = 0;
  for (int r = 0; r < R; r++) {
    int drop = 0;
    if (r == 1 || r == 2) drop = std::max(1, N / 8);
    else if (r > 6 && r % 7 == 0) drop = N >= 64 ? 3 : N >= 16 ? 1 : 0;
    drop = std::min(drop, N - SM);
    std::vector<uint8_t> gone(N, 0);
    for (int k = 0; k < drop;) {
      const int d = g.below(N);
      if (!gone[d]) gone[d] = 1, k++;
    }
    first_id[r] = id;
    mid_id[r] = id + std::max(1, (N - drop) / 2);  // ids run along the slots of a round
    for (int d = 0; d < N; d++)
      if (!gone[d]) T.W[(size_t)r * N + d] = id++;
  }
  first_id[R] = id;
  T.coin.resize(id);
  for (auto& c : T.coin) c = (uint8_t)(g.next() & 1);
  // camp 1 (the yes camp of a split) is the smaller one when N is odd: a tie counts as yes
  std::vector<uint8_t> camp(N, 0);
  for (int k = 0; k < N / 2;) {
    const int d = g.below(N);
    if (!camp[d]) camp[d] = 1, k++;
  }
  const int mix = N + 4;
  for (int r = 1; r < R; r++) {
    std::vector<int> prev;  // slots of round r - 1 that hold a witness
    for (int s = 0; s < N; s++)
      if (T.w_at(r - 1, s) >= 0) prev.push_back(s);
    // what kind of first votes each witness of round r - 1 gets
    std::vector<int> kind(N, 0);
    // (the round's first three witnesses: one of each kind that can stay undecided)
    for (int s : prev) {
      int u = g.below(N >= 128 ? 32 : 16);
      if (s == prev[0]) u = 0;
      if (prev.size() > 1 && s == prev[1]) u = N >= 128 ? 3 : 6;
      if (prev.size() > 2 && s == prev[2]) u = N >= 128 ? 2 : 4;
      if (N >= 128) kind[s] = u < 2 ? 0 : u < 3 ? 1 : u < 4 ? 2 : u < 18 ? 3 : 4;
      else kind[s] = u < 4 ? 0 : u < 6 ? 1 : u < 9 ? 2 : u < 13 ? 3 : 4;
    }
    std::vector<int> core = prev;
    std::vector<uint8_t> in_core(N, 0);
    while ((int)core.size() > SM) {
      const int q = g.below((int)core.size());
      core[q] = core.back();
      core.pop_back();
    }
    for (int s : core) in_core[s] = 1;
    for (int d = 0; d < N; d++) {
      if (T.w_at(r, d) < 0) continue;
      // strongly-see set over round r - 1: at least SM slots
      std::vector<int> own, other;
      for (int s : prev) (camp[s] == camp[d] ? own : other).push_back(s);
      if (r == mix) {  // the round's common core of SM slots, and up to two more
        own = core;
        other.clear();
        for (int s : prev)
          if (!in_core[s]) other.push_back(s);
      }
      int want = SM + (r == mix ? g.below(3) : N >= 12 ? g.below(2) : 0);
      want = std::min(want, (int)prev.size());
      for (int s : own) T.set(T.ssb, r, d, s);
      for (int k = (int)own.size(); k < want && !other.empty(); k++) {
        const int q = g.below((int)other.size());
        T.set(T.ssb, r, d, other[q]);
        other[q] = other.back();
        other.pop_back();
      }
      // first votes See(y, x)
      for (int s : prev) {
        bool v;
        switch (kind[s]) {
          case 0: v = camp[d] == 1; break;
          case 1: v = camp[d] == 0; break;
          case 2: v = g.below(2) == 0; break;
          case 3: v = g.below(8) != 0; break;
          default: v = g.below(8) == 0; break;
        }
        if (v) T.set(T.seeb, r, d, s);
      }
    }
  }
  // the calls: (rounds known, events inserted); "cut" calls end inside their last round,
  // so some witnesses of the last voting round are not inserted yet (y >= n)
  const int Rs[8] = {3, 5, N + 2, N + 4, N + 6, N + 8, 2 * N + 4, 2 * N + 8};
  const bool cut[8] = {false, true, false, true, false, true, true, false};
  for (int c = 0; c < 8; c++) {
    T.Rc.push_back(Rs[c]);
    T.nc.push_back(cut[c] ? mid_id[Rs[c] - 1] : first_id[Rs[c]]);
  }
  // the windows: round 1 (R <= i + 2, then up to R - i = N + 3), round 2 (empty slots on
  // both sides), round 3 (R - i = 2, N - 1, N + 1, .., 2N + 1, 2N + 5), round 5 (N - 1,
  // N + 1, .., 2N + 3)
  const int wr[4] = {1, 2, 3, 5}, wcf[4] = {0, 1, 1, 2}, wlen[4] = {4, 2, 7, 6};
  for (int k = 0; k < 4; k++) {
    T.w.round.push_back(wr[k]);
    T.w.off.push_back(T.w.npairs);
    T.w.cf.push_back(wcf[k]);
    T.w.len.push_back(wlen[k]);
    T.w.npairs += wlen[k];
  }
  return T;
}

// the invariants the kernels rely on (no index out of range): checked for every table
// set before it reaches the device
bool check_tables(const Tab& T, std::string& why) {
  const int N = T.N;
  auto fail = [&](const std::string& s) {
    why = s;
    return false;
  };
  if (N < 1 || N > 256 || T.NW != (N + 63) / 64 || T.R < 1) return fail("sizes");
  if (T.W.size() != (size_t)T.R * N || T.ssb.size() != (size_t)T.R * N * T.NW || T.seeb.size() != T.ssb.size())
    return fail("table sizes");
  std::vector<int> last(N, -1);  // along a slot (a creator's chain) ids increase with the round
  for (int r = 0; r < T.R; r++) {
    for (int d = 0; d < N; d++) {
      const int x = T.w_at(r, d);
      if (x < -1 || x >= (int)T.coin.size()) return fail("witness id out of range");
      if (x >= 0 && x <= last[d]) return fail("witness ids do not increase with the round");
      if (x >= 0) last[d] = x;
    }
    for (int d = 0; d < N; d++)
      for (int s = 0; s < 64 * T.NW; s++) {
        const bool ok = r > 0 && s < N && T.w_at(r, d) >= 0 && T.w_at(r - 1, s) >= 0;
        if (!ok && (T.bit(T.ssb, r, d, s) || T.bit(T.seeb, r, d, s))) return fail("a bit outside round r - 1's witnesses");
      }
  }
  for (uint8_t c : T.coin)
    if (c > 1) return fail("coin not 0/1");
  if (T.nc.size() != T.Rc.size() || T.nc.empty()) return fail("calls");
  for (size_t c = 0; c < T.Rc.size(); c++)
    if (T.Rc[c] < 0 || T.Rc[c] > T.R || T.nc[c] < 0) return fail("a call's rounds out of range");
  const auto& w = T.w;
  for (int k = 0; k < w.nrounds(); k++) {
    if (w.round[k] < 0 || w.round[k] + 1 >= T.R) return fail("a window's round out of range");
    if (w.cf[k] < 0 || w.len[k] < 1 || w.cf[k] + w.len[k] > (int)T.Rc.size()) return fail("a window's calls");
    if (w.off[k] != (k ? w.off[k - 1] + w.len[k - 1] : 0)) return fail("window offsets");
  }
  return true;
}

// ---------------------------------------------------------------------------
// The host loop: hashgraph.go:598-664 for one (round i, call) pair.  votes[r][slot] is
// the vote of round r's witness in that slot on x (Go's votes[y][x]; a missing vote
// reads false); y in ascending slot order; break leaves the y loop only; the last
// decision over j stands.  Counting goes slot by slot.
// wrong: 0 the algorithm; 1 every voter takes the coin of slot 0's witness of its
// round; 2 a coin round decides like a normal one; 3 the coin of x instead of y.
// ---------------------------------------------------------------------------
struct Counts {
  long coin_votes = 0;     // (x, j, y) that took the coin-bit vote
  long post_coin_dec = 0;  // decisions at diff > N on an x that had taken a coin-bit vote
};

// ss: the strongly-see rows as one byte per slot, [round][voter slot][slot]
void ref_pair(const Tab& T, const std::vector<uint8_t>& ss, int i, int64_t n, int R, uint8_t* out, Counts& cnt,
              int wrong) {
  const int N = T.N, SM = T.SM;
  std::vector<uint8_t> votes((size_t)T.R * N), here((size_t)T.R * N, 0);
  for (int r = 0; r < std::min(R, T.R); r++)
    for (int d = 0; d < N; d++) here[(size_t)r * N + d] = T.w_at(r, d) >= 0 && T.w_at(r, d) < n;
  for (int xd = 0; xd < N; xd++) {
    out[xd] = 0;
    const int x = T.w_at(i, xd);
    if (x < 0 || x >= n) continue;  // not a witness of round i at this call
    std::fill(votes.begin(), votes.end(), 0);
    bool coin_voted = false;
    for (int j = i + 1; j < R; j++) {
      const int diff = j - i;
      for (int d = 0; d < N; d++) {
        if (!here[(size_t)j * N + d]) continue;
        const int y = T.w_at(j, d);
        uint8_t& vote = votes[(size_t)j * N + d];
        if (diff == 1) {
          vote = T.bit(T.seeb, j, d, xd);
          continue;
        }
        int yays = 0, nays = 0;
        const uint8_t* row = &ss[((size_t)j * N + d) * N];
        const uint8_t* pv = &votes[(size_t)(j - 1) * N];
        const uint8_t* ph = &here[(size_t)(j - 1) * N];
        for (int s = 0; s < N; s++) {
          const int sees = row[s] & ph[s];
          yays += sees & pv[s];
          nays += sees & (pv[s] ^ 1);
        }
        bool v = false;
        int t = nays;
        if (yays >= nays) v = true, t = yays;
        const bool normal = wrong == 2 ? true : (diff % N) > 0;
        if (normal) {
          if (t >= SM) {
            out[xd] = v ? 1 : 2;
            if (diff > N && coin_voted) cnt.post_coin_dec++;
            break;
          }
          vote = v;
        } else if (t >= SM) {
          vote = v;
        } else {
          int c = T.coin[y];
          if (wrong == 1) c = T.w_at(j, 0) >= 0 ? T.coin[T.w_at(j, 0)] : 0;
          if (wrong == 3) c = T.coin[x];
          vote = (uint8_t)c;
          cnt.coin_votes++;
          coin_voted = true;
        }
      }
    }
  }
}

// every pair of the windows, in parallel over the pairs
Counts ref_all(const Tab& T, std::vector<uint8_t>& dec, int wrong) {
  const auto& w = T.w;
  dec.assign((size_t)w.npairs * T.N, 0);
  std::vector<Counts> per(w.npairs);
  std::vector<uint8_t> ss((size_t)T.R * T.N * T.N);
  for (int j = 0; j < T.R; j++)
    for (int d = 0; d < T.N; d++)
      for (int s = 0; s < T.N; s++) ss[((size_t)j * T.N + d) * T.N + s] = T.bit(T.ssb, j, d, s);
  std::atomic<int> nextp{0};
  auto work = [&]() {
    for (int p; (p = nextp++) < w.npairs;) {
      int k = w.nrounds() - 1;
      while (w.off[k] > p) k--;
      const int c = w.cf[k] + (p - w.off[k]);
      ref_pair(T, ss, w.round[k], T.nc[c], T.Rc[c], &dec[(size_t)p * T.N], per[p], wrong);
    }
  };
  const int nt = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (int q = 1; q < nt; q++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  Counts tot;
  for (const auto& c : per) tot.coin_votes += c.coin_votes, tot.post_coin_dec += c.post_coin_dec;
  return tot;
}

// ---------------------------------------------------------------------------
// The device side
// ---------------------------------------------------------------------------
template <typename T>
T* upload(const std::vector<T>& v) {
  T* p = nullptr;
  HIPCHK(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

struct Dev {
  hge::Tables t;
  int32_t *W, *pr, *Rc, *plist = nullptr;
  uint64_t *ssb, *seeb;
  uint8_t *coin, *dec;
  int64_t* nc;
  int nrounds, npairs, N, NW;
  bool blk;
};

Dev to_device(const Tab& T, bool blk) {
  Dev D;
  memset(&D.t, 0, sizeof(D.t));
  D.N = T.N, D.NW = T.NW, D.blk = blk;
  D.W = upload(T.W);
  D.ssb = upload(T.ssb);
  D.seeb = upload(T.seeb);
  D.coin = upload(T.coin);
  D.nc = upload(T.nc);
  D.Rc = upload(T.Rc);
  std::vector<int32_t> pr;  // round | off | cf, as the control block holds them
  pr.insert(pr.end(), T.w.round.begin(), T.w.round.end());
  pr.insert(pr.end(), T.w.off.begin(), T.w.off.end());
  pr.insert(pr.end(), T.w.cf.begin(), T.w.cf.end());
  D.pr = upload(pr);
  D.nrounds = T.w.nrounds();
  D.npairs = T.w.npairs;
  HIPCHK(hipMalloc(&D.dec, (size_t)D.npairs * T.N));
  D.t.N = T.N, D.t.NW = T.NW, D.t.SM = T.SM, D.t.Rcap = T.R;
  D.t.W = D.W, D.t.ssb = D.ssb, D.t.seeb = D.seeb, D.t.coin = D.coin;
  return D;
}
void release(Dev& D) {
  HIPCHK(hipFree(D.W));
  HIPCHK(hipFree(D.ssb));
  HIPCHK(hipFree(D.seeb));
  HIPCHK(hipFree(D.coin));
  HIPCHK(hipFree(D.nc));
  HIPCHK(hipFree(D.Rc));
  HIPCHK(hipFree(D.pr));
  HIPCHK(hipFree(D.dec));
  if (D.plist) HIPCHK(hipFree(D.plist));
}

template <int NWT>
void launch_t(const Dev& D, int win_lo, int win_hi, int p0, int p1, int nlist) {
  const int nr = D.nrounds;
  const int32_t *pr_round = D.pr + win_lo, *pr_off = D.pr + nr + win_lo, *pr_cf = D.pr + 2 * nr + win_lo;
  if (D.blk) {
    const int32_t* pl = nlist ? D.plist : nullptr;
    hge::k_fame_decide_blk<NWT><<<dim3(nlist ? nlist : p1 - p0), dim3(D.N)>>>(D.t, pr_round, pr_off, pr_cf, win_hi - win_lo, p0,
                                                                                p1, D.nc, D.Rc, D.dec, pl);
  } else {
    hge::k_fame_decide<NWT><<<dim3(((p1 - p0) * D.N + 255) / 256), dim3(256)>>>(D.t, pr_round, pr_off, pr_cf, win_hi - win_lo,
                                                                                 p0, p1, D.nc, D.Rc, D.dec);
  }
  HIPCHK(hipGetLastError());
}

// one launch over the windows [win_lo, win_hi) (or the listed pairs); the decision
// table is pre-filled with the sentinel.  Returns the table.
std::vector<uint8_t> run(Dev& D, const Tab& T, int win_lo, int win_hi, const std::vector<int32_t>& list) {
  const auto& w = T.w;
  const int p0 = list.empty() ? w.off[win_lo] : 0;
  const int p1 = list.empty() && win_hi < w.nrounds() ? w.off[win_hi] : w.npairs;
  HIPCHK(hipMemset(D.dec, kSentinel, (size_t)D.npairs * D.N));
  if (!list.empty()) {
    if (D.plist) HIPCHK(hipFree(D.plist));
    D.plist = upload(list);
  }
  const int nl = (int)list.size();
  switch (D.NW) {
    case 1: launch_t<1>(D, win_lo, win_hi, p0, p1, nl); break;
    case 2: launch_t<2>(D, win_lo, win_hi, p0, p1, nl); break;
    case 3: launch_t<3>(D, win_lo, win_hi, p0, p1, nl); break;
    case 4: launch_t<4>(D, win_lo, win_hi, p0, p1, nl); break;
    default: fprintf(stderr, "NW %d\n", D.NW); exit(2);
  }
  HIPCHK(hipDeviceSynchronize());
  std::vector<uint8_t> got((size_t)D.npairs * D.N);
  HIPCHK(hipMemcpy(got.data(), D.dec, got.size(), hipMemcpyDeviceToHost));
  return got;
}

std::string kname(bool blk, int NW) {
  return std::string(blk ? "k_fame_decide_blk<" : "k_fame_decide<") + std::to_string(NW) + ">";
}

// every slot: the reference where the launch decides the pair, the sentinel elsewhere
long compare(const Tab& T, bool blk, const char* form, const std::vector<uint8_t>& got, const std::vector<uint8_t>& want,
             const std::vector<uint8_t>& live) {
  for (int p = 0; p < T.w.npairs; p++)
    for (int d = 0; d < T.N; d++) {
      const uint8_t g = got[(size_t)p * T.N + d], e = live[p] ? want[(size_t)p * T.N + d] : kSentinel;
      if (g != e) {
        int k = T.w.nrounds() - 1;
        while (T.w.off[k] > p) k--;
        const int c = T.w.cf[k] + (p - T.w.off[k]);
        printf("MISMATCH N=%d %s %s: pair %d (round %d, call %d: n=%lld R=%d) slot %d: got %d want %d%s\n", T.N,
               kname(blk, T.NW).c_str(), form, p, T.w.round[k], c, (long long)T.nc[c], T.Rc[c], d, g, e,
               live[p] ? "" : " (a pair this launch does not decide)");
        exit(1);
      }
    }
  return (long)T.w.npairs * T.N;
}

const int kBlkN[] = {64, 128, 192, 256};
const int kItemN[] = {5, 16, 33, 63, 65, 96, 130, 200, 255};

int run_cases(bool host_only) {
  long total = 0;
  std::vector<std::pair<int, bool>> cases;
  for (int n : kBlkN) cases.push_back({n, true});
  for (int n : kItemN) cases.push_back({n, false});
  for (auto [N, blk] : cases) {
    Tab T = generate(N);
    std::string why;
    if (!check_tables(T, why)) {
      printf("N=%d: the generated tables break an invariant: %s\n", N, why.c_str());
      return 1;
    }
    std::vector<uint8_t> want;
    const Counts cnt = ref_all(T, want, 0);
    long decided[3] = {0, 0, 0};
    for (uint8_t v : want) decided[v]++;
    if (cnt.coin_votes == 0 || cnt.post_coin_dec == 0) {
      printf("N=%d: the reference takes %ld coin-bit votes and decides %ld times after a coin round: both must be > 0\n",
             N, cnt.coin_votes, cnt.post_coin_dec);
      return 1;
    }
    if (host_only) {
      // the cases tell the algorithm from three wrong readings of the coin branch
      long differ[4] = {0, 0, 0, 0};
      for (int wrong = 1; wrong <= 3; wrong++) {
        std::vector<uint8_t> other;
        ref_all(T, other, wrong);
        for (size_t q = 0; q < want.size(); q++) differ[wrong] += other[q] != want[q];
      }
      printf("host %s N=%d pairs=%d coin_votes=%ld post_coin_decisions=%ld dec0=%ld dec1=%ld dec2=%ld "
             "differ_coin_slot0=%ld differ_coin_decides=%ld differ_coin_of_x=%ld\n",
             kname(blk, T.NW).c_str(), N, T.w.npairs, cnt.coin_votes, cnt.post_coin_dec, decided[0], decided[1],
             decided[2], differ[1], differ[2], differ[3]);
      if (!differ[1] || !differ[2] || !differ[3]) {
        printf("N=%d: a wrong reading of the coin branch would go unnoticed\n", N);
        return 1;
      }
      total += (long)want.size();
      continue;
    }
    Dev D = to_device(T, blk);
    const int nr = T.w.nrounds();
    std::vector<uint8_t> live(T.w.npairs, 1);
    long slots = compare(T, blk, "full", run(D, T, 0, nr, {}), want, live);
    // a split part's launches: the last rounds' pairs, then the middle ones (p0 > 0,
    // pr_* offset, pairs after the part's left alone)
    const int parts[2][2] = {{2, nr}, {1, 3}};
    for (auto& pt : parts) {
      for (int p = 0; p < T.w.npairs; p++) live[p] = p >= T.w.off[pt[0]] && (pt[1] >= nr || p < T.w.off[pt[1]]);
      slots += compare(T, blk, "part", run(D, T, pt[0], pt[1], {}), want, live);
    }
    if (blk) {  // a widening pass's launch: a strict, unordered list of pairs
      const std::vector<int32_t> list = {17, 3, 12, 9, 0, 18, 6, 10};
      std::fill(live.begin(), live.end(), 0);
      for (int p : list) live[p] = 1;
      slots += compare(T, blk, "plist", run(D, T, 0, nr, list), want, live);
    }
    release(D);
    printf("case %s N=%d pairs=%d slots=%ld coin_votes=%ld post_coin_decisions=%ld dec0=%ld dec1=%ld dec2=%ld forms=%s\n",
           kname(blk, T.NW).c_str(), N, T.w.npairs, slots, cnt.coin_votes, cnt.post_coin_dec, decided[0], decided[1],
           decided[2], blk ? "full,part,part,plist" : "full,part,part");
    total += slots;
  }
  printf("ok %ld\n", total);
  return 0;
}

template <typename T>
bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int run_file(const char* path, bool host_only) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    return 2;
  }
  int32_t h[4];
  Tab T;
  bool ok = fread(h, 4, 4, f) == 4 && h[0] >= 1 && h[0] <= 256 && h[1] >= 1 && h[1] < (1 << 20) && h[2] >= 0 && h[3] >= 1;
  if (ok) {
    T.N = h[0], T.NW = (h[0] + 63) / 64, T.SM = 2 * h[0] / 3 + 1, T.R = h[1];
    const size_t rows = (size_t)T.R * T.N;
    ok = read_vec(f, T.W, rows) && read_vec(f, T.seeb, rows * T.NW) && read_vec(f, T.ssb, rows * T.NW) &&
         read_vec(f, T.coin, (size_t)h[2]) && read_vec(f, T.nc, (size_t)h[3]) && read_vec(f, T.Rc, (size_t)h[3]);
  }
  fclose(f);
  if (!ok) {
    fprintf(stderr, "%s: short or malformed\n", path);
    return 2;
  }
  // every round that has a next one, at every call
  const int ncalls = h[3];
  for (int i = 0; i + 1 < T.R; i++) {
    T.w.round.push_back(i);
    T.w.off.push_back(T.w.npairs);
    T.w.cf.push_back(0);
    T.w.len.push_back(ncalls);
    T.w.npairs += ncalls;
  }
  std::string why;
  if (T.w.npairs == 0 || !check_tables(T, why)) {
    fprintf(stderr, "%s: the tables break an invariant: %s\n", path, why.c_str());
    return 2;
  }
  auto show = [&](const char* tag, const std::vector<uint8_t>& dec) {
    std::string s(dec.size(), '0');
    for (size_t q = 0; q < dec.size(); q++) s[q] = dec[q] <= 2 ? (char)('0' + dec[q]) : '?';
    printf("%s %d %d %s\n", tag, T.w.npairs, T.N, s.c_str());
  };
  std::vector<uint8_t> want;
  const Counts cnt = ref_all(T, want, 0);
  printf("coin_votes %ld\n", cnt.coin_votes);
  show("ref", want);
  if (host_only) return 0;
  const bool blk = T.N == 64 * T.NW;  // the kernel the engine launches at this N
  Dev D = to_device(T, blk);
  const std::vector<uint8_t> got = run(D, T, 0, T.w.nrounds(), {});
  release(D);
  printf("kernel %s\n", kname(blk, T.NW).c_str());
  show("gpu", got);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  bool host_only = false;
  const char* file = nullptr;
  for (int a = 1; a < argc; a++) {
    const std::string s = argv[a];
    if (s == "--host") host_only = true;
    else if (s == "--tables" && a + 1 < argc) file = argv[++a];
    else {
      fprintf(stderr, "usage: %s [--host] [--tables FILE]\n", argv[0]);
      return 2;
    }
  }
  return file ? run_file(file, host_only) : run_cases(host_only);
}
