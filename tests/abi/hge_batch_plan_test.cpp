// The batch engine's launch plan and pool layout (babble_amd/csrc/hge_batch_plan.h).
// The plan is checked against the table of DESIGN.md §4.8, "Instances chosen by the
// batch's size", tabulated below from the document: every boundary and its neighbours at
// 256 compute units and at an odd count (77).  The layout is checked on three
// hand-written batches (offsets, Rcap, ccap, Emax, the sums) and at its capacity limits,
// from counts alone.  Plain host C++: links nothing of the engine
// (tests/test_batch_plan_host.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../babble_amd/csrc/hge_batch_plan.h"

using namespace hgb;

static long checks = 0, failed = 0;
#define CHECK(got, want)                                                                                   \
  do {                                                                                                     \
    const long long g_ = (long long)(got), w_ = (long long)(want);                                         \
    checks++;                                                                                              \
    if (g_ != w_) {                                                                                        \
      failed++;                                                                                            \
      fprintf(stderr, "line %d: %s = %lld, want %lld\n", __LINE__, #got, g_, w_);                          \
    }                                                                                                      \
  } while (0)

// §4.8's rows on the number of graphs: G, then `coords`, `front_threads`, `ns`
struct GRow {
  int ncu, G, coords, front, ns;
};
static const GRow G_ROWS[] = {
    // 256 compute units: 2G <= ncu up to 128; G <= ncu up to 256; G <= 2 ncu up to 512
    {256, 1, 0, 1024, 3},   {256, 127, 0, 1024, 3}, {256, 128, 0, 1024, 3}, {256, 129, 1, 1024, 3},
    {256, 255, 1, 1024, 3}, {256, 256, 1, 1024, 3}, {256, 257, 1, 512, 3},  {256, 511, 1, 512, 3},
    {256, 512, 1, 512, 3},  {256, 513, 2, 256, 2},  {256, 1024, 2, 256, 2}, {256, 1 << 20, 2, 256, 2},
    // 77: 2G = 76 and 78 lie on either side of ncu; G = ncu, ncu + 1, 2 ncu, 2 ncu + 1
    {77, 1, 0, 1024, 3},    {77, 37, 0, 1024, 3},   {77, 38, 0, 1024, 3},   {77, 39, 1, 1024, 3},
    {77, 76, 1, 1024, 3},   {77, 77, 1, 1024, 3},   {77, 78, 1, 512, 3},    {77, 153, 1, 512, 3},
    {77, 154, 1, 512, 3},   {77, 155, 2, 256, 2},   {77, 156, 2, 256, 2},
};
// ... on the calls in all: `sort_threads` (Ktot <= 16 ncu: 256, above: 64)
struct KRow {
  int ncu;
  int64_t Ktot;
  int sort;
};
static const KRow K_ROWS[] = {
    {256, 0, 256},  {256, 1, 256},   {256, 4095, 256}, {256, 4096, 256}, {256, 4097, 64}, {256, (int64_t)1 << 40, 64},
    {77, 1231, 256}, {77, 1232, 256}, {77, 1233, 64},   {77, 1234, 64},
};
// ... on the fallback graphs: `consensus_occ` (none: 0, F <= 2 ncu: 1, above: 4)
struct FRow {
  int ncu;
  int64_t F;
  int occ;
};
static const FRow F_ROWS[] = {
    {256, 0, 0}, {256, 1, 1}, {256, 511, 1}, {256, 512, 1}, {256, 513, 4}, {256, (int64_t)1 << 33, 4},
    {77, 0, 0},  {77, 1, 1},  {77, 153, 1},  {77, 154, 1},  {77, 155, 4},
};

static void plan_checks() {
  for (const GRow& r : G_ROWS)
    for (int N : {1, 5, 32, 33, 64})
      for (int serial = 0; serial < 2; serial++)
        for (int dlv = 0; dlv < 2; dlv++)
          for (int k = 0; k < 3; k++) {  // Ktot = 1, 16 ncu, 16 ncu + 1: sort_threads 256, 256, 64
            const int64_t Ktot = k == 0 ? 1 : (int64_t)16 * r.ncu + (k - 1);
            const int sort = k == 2 ? 64 : 256;
            const BatchPlan p = batch_stage_plan(N, r.G, Ktot, r.ncu, serial != 0, dlv != 0);
            CHECK(p.nm, N <= 32 ? 32 : 64);  // NM is 32 for N <= 32, else 64
            CHECK(p.coords, r.coords);
            CHECK(p.front_threads, r.front);
            CHECK(p.ns, serial ? 0 : r.ns);  // under HGB_SERIAL ns and sort_threads are 0
            CHECK(p.sort_threads, serial ? 0 : sort);
            CHECK(p.consensus_occ, 0);  // the fallback pass's, known after the stages
            CHECK(p.dlv, dlv);
          }
  for (const KRow& r : K_ROWS)
    for (int G : {1, r.ncu, 2 * r.ncu + 1}) {
      CHECK(batch_stage_plan(32, G, r.Ktot, r.ncu, false, false).sort_threads, r.sort);
      CHECK(batch_stage_plan(64, G, r.Ktot, r.ncu, false, true).sort_threads, r.sort);
      CHECK(batch_stage_plan(32, G, r.Ktot, r.ncu, true, false).sort_threads, 0);
    }
  for (const FRow& r : F_ROWS) CHECK(batch_consensus_occ(r.F, r.ncu), r.occ);
  CHECK(batch_stage_plan(32, 7, 9, 256, false, false).nm, 32);
  CHECK(batch_stage_plan(33, 7, 9, 256, false, false).nm, 64);
}

static void check_desc(const GDesc& d, int64_t eo, int E, int co, int K, int ro, int Rcap) {
  CHECK(d.eo, eo);
  CHECK(d.E, E);
  CHECK(d.co, co);
  CHECK(d.K, K);
  CHECK(d.ro, ro);
  CHECK(d.Rcap, Rcap);
  CHECK(d.pad, 0);
}

static void check_sums(const BatchPools& p, size_t G, int64_t Etot, int64_t Ktot, int64_t Rtot, int64_t Stot, int ccap,
                       int Emax) {
  CHECK(p.hd.size(), G);
  CHECK(p.Etot, Etot);
  CHECK(p.Ktot, Ktot);
  CHECK(p.Rtot, Rtot);
  CHECK(p.Stot, Stot);
  CHECK(p.ccap, ccap);
  CHECK(p.Emax, Emax);
}

static void layout_checks() {
  // no graphs at all: a stage of an empty batch
  check_sums(layout(3, nullptr, 0), 0, 0, 0, 0, 0, 1, 0);
  {  // empty graphs (N = 4, SM = 3): two round rows each, a chain row of one
    const GraphSize gs[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    const BatchPools p = layout(3, gs, 3);
    check_sums(p, 3, 0, 0, 6, 0, 1, 0);
    for (int g = 0; g < 3; g++) check_desc(p.hd[g], 0, 0, 0, 0, 2 * g, 2);
  }
  {  // one graph with fewer events than a supermajority (N = 6, SM = 5)
    const GraphSize gs[1] = {{3, 1, 2, 0}};
    const BatchPools p = layout(5, gs, 1);
    check_sums(p, 1, 3, 1, 2, 0, 2, 3);
    check_desc(p.hd[0], 0, 3, 0, 1, 0, 2);
  }
  {  // irregular sizes, an empty graph between them, submissions as a generated batch has them
    const GraphSize gs[4] = {{10, 3, 4, 12}, {0, 0, 0, 0}, {7, 1, 7, 9}, {100, 25, 40, 130}};
    const BatchPools p = layout(3, gs, 4);
    check_sums(p, 4, 117, 29, 5 + 2 + 4 + 35, 151, 40, 100);
    check_desc(p.hd[0], 0, 10, 0, 3, 0, 5);     // 10 / 3 + 2
    check_desc(p.hd[1], 10, 0, 3, 0, 5, 2);
    check_desc(p.hd[2], 10, 7, 3, 1, 7, 4);     // 7 / 3 + 2
    check_desc(p.hd[3], 17, 100, 4, 25, 11, 35);  // 100 / 3 + 2
  }
  {  // SM = 1 (N = 1): a round per event and two
    const GraphSize gs[2] = {{5, 5, 5, 5}, {1, 1, 1, 1}};
    const BatchPools p = layout(1, gs, 2);
    check_sums(p, 2, 6, 6, 7 + 3, 6, 5, 5);
    check_desc(p.hd[1], 5, 1, 5, 1, 7, 3);
  }
}

// 0: laid out; else the error's code, its message compared with `msg`
static int refused(int SM, std::initializer_list<GraphSize> gs, const char* msg) {
  const std::vector<GraphSize> v(gs);
  try {
    (void)layout(SM, v.data(), (int)v.size());
  } catch (const hge::Error& e) {
    CHECK(strcmp(e.msg.c_str(), msg), 0);
    return e.code;
  }
  return 0;
}

static void capacity_checks() {
  const char* large = "batch too large";
  const char* chain = "batch graph with a chain of 2^24 events or more";
  const int32_t M = INT32_MAX;
  // Ktot: INT32_MAX - 1 calls are laid out, INT32_MAX are not, in one graph or summed
  CHECK(refused(3, {{0, M - 1, 0, 0}}, large), 0);
  CHECK(refused(3, {{0, M, 0, 0}}, large), HGE_ERR_CAPACITY);
  CHECK(refused(3, {{0, 1 << 30, 0, 0}, {0, (1 << 30) - 3, 0, 0}, {0, 1, 0, 0}}, large), 0);
  CHECK(refused(3, {{0, 1 << 30, 0, 0}, {0, (1 << 30) - 2, 0, 0}, {0, 1, 0, 0}}, large), HGE_ERR_CAPACITY);
  CHECK(refused(3, {{0, 1 << 30, 0, 0}, {0, 1 << 30, 0, 0}, {0, 1 << 30, 0, 0}}, large), HGE_ERR_CAPACITY);
  // Rtot, SM = 1: Rcap = E + 2
  CHECK(refused(1, {{M - 3, 0, 1, 0}}, large), 0);
  CHECK(refused(1, {{M - 2, 0, 1, 0}}, large), HGE_ERR_CAPACITY);
  CHECK(refused(1, {{1 << 30, 0, 1, 0}, {(1 << 30) - 6, 0, 1, 0}}, large), 0);
  CHECK(refused(1, {{1 << 30, 0, 1, 0}, {(1 << 30) - 5, 0, 1, 0}}, large), HGE_ERR_CAPACITY);
  CHECK(refused(1, {{1 << 30, 0, 1, 0}, {1 << 30, 0, 1, 0}, {5, 5, 5, 5}}, large), HGE_ERR_CAPACITY);
  // the longest chain: 2^24 - 1 positions fit the kernels' packed (creator, index), 2^24 do not
  CHECK(refused(3, {{1 << 25, 1, (1 << 24) - 1, 0}}, chain), 0);
  CHECK(refused(3, {{1 << 25, 1, 1 << 24, 0}}, chain), HGE_ERR_CAPACITY);
  CHECK(refused(3, {{4, 1, 2, 0}, {1 << 25, 1, 1 << 24, 1 << 25}}, chain), HGE_ERR_CAPACITY);
  {  // at the limit the sums are the counts
    const GraphSize gs[1] = {{M - 3, M - 1, (1 << 24) - 1, (int64_t)1 << 40}};
    const BatchPools p = layout(1, gs, 1);
    check_sums(p, 1, M - 3, M - 1, M - 1, (int64_t)1 << 40, (1 << 24) - 1, M - 3);
  }
}

int main() {
  static_assert(sizeof(GDesc) == 32, "the kernels' view of a graph's blocks");
  plan_checks();
  layout_checks();
  capacity_checks();
  if (failed) {
    fprintf(stderr, "%ld of %ld checks failed\n", failed, checks);
    return 1;
  }
  printf("ok %ld checks\n", checks);
  return 0;
}
