// The host event log (babble_amd/csrc/hge_hostlog.h): the insertion cases of the
// reference's hashgraph_test.go with the code and message the engine returns for each,
// and seeded random streams against a brute-force restatement (linear scans over the
// list of accepted events: no chain tails, no counters).  Host only, links nothing of
// the engine (tests/test_hostlog_host.py runs it).  Prints "ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "../../babble_amd/csrc/hge_hostlog.h"

using hge::HostLog;
using hge::UpEv;

static long checks = 0, fails = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    checks++;                                                            \
    if (!(c)) {                                                          \
      if (fails++ < 20) fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); \
    }                                                                    \
  } while (0)

static const char* kCreator = "Could not find fake creator id";
static const char* kSpUnknown = "Self-parent not known";
static const char* kSpCreator = "Self-parent has different creator";
static const char* kOpUnknown = "Other-parent not known";
static const char* kSpNotLast = "Self-parent not last known event by creator";
static const char* kIndex = "Event index does not match the creator's chain position";

static hge_event mk(int creator, int index, int sp, int op, uint64_t salt = 0) {
  hge_event e;
  memset(&e, 0, sizeof e);
  e.creator = creator;
  e.index = index;
  e.self_parent = sp;
  e.other_parent = op;
  e.timestamp_ns = 1000 + (int64_t)(salt % 1000003) * 7;
  for (int b = 0; b < 32; b++) {
    e.s[b] = (uint8_t)(salt * 131 + b * 17 + 1);
    e.hash[b] = (uint8_t)(salt * 29 + b);
  }
  e.hash[16] = (uint8_t)(salt % 3 == 0 ? 0 : salt);
  e.n_tx = (int32_t)(salt % 5);
  return e;
}

// one insertion as the engine does it: admit, then append when accepted
static int insert(HostLog& log, const hge_event& e, std::string& err) {
  err.clear();
  const int r = log.admit(e, e.self_parent, e.other_parent, err);
  if (r == HGE_OK) log.append(e, e.self_parent, e.other_parent);
  return r;
}
#define EXPECT(log, ev, code, msg)             \
  do {                                         \
    std::string err_;                          \
    CHECK(insert(log, ev, err_) == (code));    \
    CHECK(err_ == (msg));                      \
  } while (0)

// ---- the reference's insertion cases (hashgraph_test.go: TestFork, TestInsertEvent's
// graph, and the rules of hashgraph.go:366-396 one by one)
static void reference_cases() {
  HostLog log(3, INT32_MAX);
  // first event rules: empty parents and nothing known of the creator; index 0
  EXPECT(log, mk(0, 1, HGE_NONE, HGE_NONE), HGE_ERR_INDEX, kIndex);
  EXPECT(log, mk(0, 0, HGE_NONE, HGE_NONE, 1), HGE_OK, "");  // e0 = 0
  EXPECT(log, mk(1, 0, HGE_NONE, HGE_NONE, 2), HGE_OK, "");  // e1 = 1
  EXPECT(log, mk(2, 0, HGE_NONE, HGE_NONE, 3), HGE_OK, "");  // e2 = 2
  CHECK(log.n_events == 3);
  // TestFork: 'a', a second root of node 2 (its self-parent "" is not known)
  EXPECT(log, mk(2, 0, HGE_NONE, HGE_NONE, 4), HGE_ERR_SELF_PARENT_UNKNOWN, kSpUnknown);
  // e01 = (e0, a): a was refused, so the other-parent cannot be resolved
  EXPECT(log, mk(0, 1, 0, HGE_UNKNOWN, 5), HGE_ERR_OTHER_PARENT_UNKNOWN, kOpUnknown);
  // e20 = (e2, e01): e01 was refused
  EXPECT(log, mk(2, 1, 2, HGE_UNKNOWN, 6), HGE_ERR_OTHER_PARENT_UNKNOWN, kOpUnknown);
  CHECK(log.n_events == 3);
  // unknown self-parent: unresolved, and an id past the log
  EXPECT(log, mk(0, 1, HGE_UNKNOWN, 1), HGE_ERR_SELF_PARENT_UNKNOWN, kSpUnknown);
  EXPECT(log, mk(0, 1, 3, 1), HGE_ERR_SELF_PARENT_UNKNOWN, kSpUnknown);
  // an empty self-parent with an other-parent is not a first event
  EXPECT(log, mk(0, 1, HGE_NONE, 1), HGE_ERR_SELF_PARENT_UNKNOWN, kSpUnknown);
  // foreign self-parent
  EXPECT(log, mk(0, 1, 1, 2), HGE_ERR_SELF_PARENT_CREATOR, kSpCreator);
  // unknown other-parent: empty, unresolved, past the log
  EXPECT(log, mk(0, 1, 0, HGE_NONE), HGE_ERR_OTHER_PARENT_UNKNOWN, kOpUnknown);
  EXPECT(log, mk(0, 1, 0, 17), HGE_ERR_OTHER_PARENT_UNKNOWN, kOpUnknown);
  // bad creator: both ends
  EXPECT(log, mk(3, 0, HGE_NONE, HGE_NONE), HGE_ERR_CREATOR, kCreator);
  EXPECT(log, mk(-1, 0, HGE_NONE, HGE_NONE), HGE_ERR_CREATOR, kCreator);
  // index lies (the engine's own rule, include/hge.h)
  EXPECT(log, mk(0, 2, 0, 1), HGE_ERR_INDEX, kIndex);
  EXPECT(log, mk(0, 0, 0, 1), HGE_ERR_INDEX, kIndex);
  // TestInsertEvent's e01 = (e0, e1), e20 = (e2, e01), e12 = (e1, e20)
  EXPECT(log, mk(0, 1, 0, 1, 7), HGE_OK, "");  // 3
  EXPECT(log, mk(2, 1, 2, 3, 8), HGE_OK, "");  // 4
  EXPECT(log, mk(1, 1, 1, 4, 9), HGE_OK, "");  // 5
  // self-parent not last: a fork on e0 after e01
  EXPECT(log, mk(0, 1, 0, 5), HGE_ERR_SELF_PARENT_NOT_LAST, kSpNotLast);
  // the order of the checks: a foreign self-parent is reported before an unknown
  // other-parent, an unknown other-parent before a stale self-parent, that before the index
  EXPECT(log, mk(0, 9, 1, HGE_UNKNOWN), HGE_ERR_SELF_PARENT_CREATOR, kSpCreator);
  EXPECT(log, mk(0, 9, 0, HGE_UNKNOWN), HGE_ERR_OTHER_PARENT_UNKNOWN, kOpUnknown);
  EXPECT(log, mk(0, 9, 0, 5), HGE_ERR_SELF_PARENT_NOT_LAST, kSpNotLast);
  CHECK(log.n_events == 6);
  CHECK(log.chain_len[0] == 2 && log.chain_len[1] == 2 && log.chain_len[2] == 2);
  CHECK(log.chain_last[0] == 3 && log.chain_last[1] == 5 && log.chain_last[2] == 4);

  // the chain limit: a fine event on a chain of chain_limit events is reported, not
  // refused (the engine decides), and the refusal's text names the limit
  HostLog small(2, 2);
  EXPECT(small, mk(0, 0, HGE_NONE, HGE_NONE, 1), HGE_OK, "");
  EXPECT(small, mk(1, 0, HGE_NONE, HGE_NONE, 2), HGE_OK, "");
  EXPECT(small, mk(0, 1, 0, 1, 3), HGE_OK, "");
  std::string err;
  CHECK(insert(small, mk(0, 2, 2, 1, 4), err) == HostLog::kAtLimit);
  CHECK(small.n_events == 3);
  CHECK(insert(small, mk(0, 3, 2, 1, 4), err) == HGE_ERR_INDEX);  // (the index rule comes first)
  CHECK(small.capacity_error(err) == HGE_ERR_CAPACITY);
  CHECK(err == "Chain capacity exceeded: at most 2 events per creator");
  small.chain_limit = INT32_MAX;  // the engine lifted it
  EXPECT(small, mk(0, 2, 2, 1, 4), HGE_OK, "");
}

// ---- brute force: what a list of accepted events says
struct Acc {
  hge_event e;
};
static int brute_admit(int N, const std::vector<Acc>& acc, const hge_event& e, int limit) {
  if (e.creator < 0 || e.creator >= N) return HGE_ERR_CREATOR;
  int known = 0, last = -1;
  for (size_t i = 0; i < acc.size(); i++)
    if (acc[i].e.creator == e.creator) {
      known++;
      last = (int)i;
    }
  const int sp = e.self_parent, op = e.other_parent, n = (int)acc.size();
  if (sp == HGE_NONE && op == HGE_NONE && known == 0) return e.index == 0 ? HGE_OK : HGE_ERR_INDEX;
  if (sp < 0 || sp >= n) return HGE_ERR_SELF_PARENT_UNKNOWN;
  if (acc[sp].e.creator != e.creator) return HGE_ERR_SELF_PARENT_CREATOR;
  if (op < 0 || op >= n) return HGE_ERR_OTHER_PARENT_UNKNOWN;
  if (sp != last) return HGE_ERR_SELF_PARENT_NOT_LAST;
  if (e.index != known) return HGE_ERR_INDEX;
  return known >= limit ? HostLog::kAtLimit : HGE_OK;
}

static bool same_log(const HostLog& a, const HostLog& b) {
  return a.N == b.N && a.h_creator == b.h_creator && a.h_index == b.h_index && a.h_sp == b.h_sp &&
         a.h_op == b.h_op && a.h_ntx == b.h_ntx && a.h_ts == b.h_ts && a.h_S == b.h_S && a.h_coin == b.h_coin &&
         a.chain_len == b.chain_len && a.chain_last == b.chain_last && a.h_chain == b.h_chain &&
         a.n_events == b.n_events && a.chain_limit == b.chain_limit;
}

static void check_against_brute(const HostLog& log, int N, const std::vector<Acc>& acc, std::mt19937_64& rng) {
  const int n = (int)acc.size();
  CHECK(log.n_events == n);
  CHECK((int)log.h_creator.size() == n && (int)log.h_S.size() == 4 * n);
  int longest = 0;
  for (int c = 0; c < N; c++) {
    std::vector<int32_t> ch;
    for (int i = 0; i < n; i++)
      if (acc[i].e.creator == c) ch.push_back(i);
    CHECK(log.h_chain[c] == ch);
    CHECK(log.chain_len[c] == (int)ch.size());  // hge_known's counts
    CHECK(log.chain_last[c] == (ch.empty() ? -1 : ch.back()));
    longest = std::max(longest, (int)ch.size());
  }
  CHECK(log.max_chain() == longest);
  // the packed records of a random range, field by field from the events as handed over
  if (n == 0) return;
  const int64_t a = (int64_t)(rng() % (uint64_t)n), m = 1 + (int64_t)(rng() % (uint64_t)(n - a));
  const std::vector<UpEv> up = log.pack(a, m);
  CHECK((int64_t)up.size() == m);
  for (int64_t i = 0; i < m && i < (int64_t)up.size(); i++) {
    const hge_event& e = acc[(size_t)(a + i)].e;
    const UpEv& r = up[(size_t)i];
    bool ok = r.creator == e.creator && r.index == e.index && r.sp == e.self_parent && r.op == e.other_parent &&
              r.ntx == e.n_tx && r.ts == e.timestamp_ns && r.coin == (e.hash[16] != 0 ? 1 : 0);
    for (int k = 0; k < 4; k++) {
      uint64_t v = 0;
      for (int b = 0; b < 8; b++) v = v * 256 + e.s[8 * k + b];  // big-endian limbs
      ok = ok && r.S[k] == v;
    }
    CHECK(ok);
  }
}

// a seeded stream: gossip-like events, one in five bent into one of the refusals
static void random_stream(uint64_t seed) {
  std::mt19937_64 rng(seed);
  const int N = 1 + (int)(rng() % 9);
  const int limit = rng() % 4 == 0 ? 3 + (int)(rng() % 6) : INT32_MAX;
  const int steps = 20 + (int)(rng() % 200);
  HostLog log(N, limit);
  std::vector<Acc> acc;
  std::vector<int> last(N, -1), len(N, 0);
  for (int t = 0; t < steps; t++) {
    const int c = (int)(rng() % (uint64_t)N);
    hge_event e = len[c] == 0 ? mk(c, 0, HGE_NONE, HGE_NONE, rng())
                              : mk(c, len[c], last[c], (int)(rng() % acc.size()), rng());
    if (rng() % 5 == 0) {
      switch (rng() % 8) {
        case 0: e.creator = rng() % 2 ? N + (int)(rng() % 3) : -1 - (int)(rng() % 3); break;
        case 1: e.index += 1 + (int)(rng() % 3); break;
        case 2: e.index -= 1; break;
        case 3: e.self_parent = rng() % 2 ? HGE_UNKNOWN : (int)acc.size() + (int)(rng() % 4); break;
        case 4: e.other_parent = rng() % 2 ? HGE_UNKNOWN : (int)acc.size() + (int)(rng() % 4); break;
        case 5: if (!acc.empty()) e.self_parent = (int)(rng() % acc.size()); break;  // foreign or stale
        case 6: e.self_parent = HGE_NONE; break;
        case 7: e.other_parent = HGE_NONE; break;
      }
    }
    const int want = brute_admit(N, acc, e, log.chain_limit);
    std::string err;
    const int got = log.admit(e, e.self_parent, e.other_parent, err);
    CHECK(got == want);
    CHECK((got == HGE_OK || got == HostLog::kAtLimit) == err.empty());
    if (got == HostLog::kAtLimit && rng() % 2) log.chain_limit = INT32_MAX;  // the engine goes on in int32
    if (got == HGE_OK || (got == HostLog::kAtLimit && log.chain_limit == INT32_MAX)) {
      log.append(e, e.self_parent, e.other_parent);
      acc.push_back({e});
      last[c] = (int)acc.size() - 1;
      len[c]++;
    }
    if (t % 16 == 0) check_against_brute(log, N, acc, rng);
  }
  check_against_brute(log, N, acc, rng);
  // a fresh log assigned over a used one equals a newly constructed one
  const int N2 = 1 + (int)(rng() % 9);
  log = HostLog(N2, limit);
  CHECK(same_log(log, HostLog(N2, limit)));
  CHECK(log.h_creator.empty() && log.n_events == 0 && (int)log.h_chain.size() == N2);
  std::string err;
  CHECK(insert(log, mk(0, 0, HGE_NONE, HGE_NONE, seed), err) == HGE_OK);  // ... and takes a first event
}

int main() {
  reference_cases();
  for (uint64_t seed = 1; seed <= 400; seed++) random_stream(seed);
  if (fails) {
    fprintf(stderr, "%ld of %ld checks failed\n", fails, checks);
    return 1;
  }
  printf("ok %ld\n", checks);
  return 0;
}
