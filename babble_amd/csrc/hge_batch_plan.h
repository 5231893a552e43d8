// hge_batch_plan.h — the batch engine's two host decisions that need no device: which
// kernel instances a run launches ("Instances chosen by the batch's
// size") and where each graph lies in the pooled tables.  Plain host C++ without HIP:
// hge_batch_host.hip branches on a BatchPlan and sizes every table from a BatchPools;
// tests/abi/hge_batch_plan_test.cpp checks both on the CPU.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/hge.h"
#include "hge_own.h"

namespace hgb {

// One graph's blocks in the pooled tables; the kernels read it as it is (BT::gd).
struct GDesc {
  int64_t eo;    // first event of the graph in the per-event pools
  int32_t E;     // accepted events
  int32_t co;    // first call in the per-call pools
  int32_t K;     // calls
  int32_t ro;    // first round row in the per-round pools
  int32_t Rcap;  // rounds the graph may reach (E / SM + 2)
  int32_t pad;
};
static_assert(sizeof(GDesc) == 32, "GDesc is a kernel argument layout");

// The kernel instances of a run (hge_batch_launch_plan); 0: the stage did not launch.
struct BatchPlan {
  int32_t nm = 0, coords = 0, front_threads = 0, ns = 0, sort_threads = 0, consensus_occ = 0, dlv = 0;
};

// The stages before the fallback pass, for G > 0 graphs of N participants with Ktot calls
// in all on ncu compute units.  serial (HGB_SERIAL): the bulk fame and order stages do
// not launch.
inline BatchPlan batch_stage_plan(int N, int G, int64_t Ktot, int ncu, bool serial, bool dlv) {
  BatchPlan p;
  p.nm = N <= 32 ? 32 : 64;
  // levelled by kb_levels while two graphs fit a CU; the columns split over two
  // workgroups while both still get a CU of their own (128 graphs: 0.46 -> 0.43 ms; at
  // 256 graphs, two per CU, 0.49 -> 0.51; four 8-column parts: 0.45 / 0.55)
  p.coords = 2 * G <= ncu ? 0 : G <= 2 * ncu ? 1 : 2;
  // a workgroup of 1,024 threads per graph while each has a CU, 512 while two fit one
  p.front_threads = G > 2 * ncu ? 256 : G > ncu ? 512 : 1024;
  p.ns = serial ? 0 : G > 2 * ncu ? 2 : 3;
  // call buckets of up to 1,024 keys: one wave each, a workgroup of four while the
  // batch has few buckets
  p.sort_threads = serial ? 0 : Ktot > 16 * (int64_t)ncu ? 64 : 256;
  p.dlv = dlv;
  return p;
}

// kb_consensus over the F graphs the bulk fold could not hold; 0: not launched
inline int32_t batch_consensus_occ(int64_t F, int ncu) { return F <= 0 ? 0 : F > 2 * (int64_t)ncu ? 4 : 1; }

// What the layout needs of a graph: accepted events, calls, its longest chain, and for
// a generated graph its submissions.
struct GraphSize {
  int32_t E, K, chain;
  int64_t subs;
};

// The staged layout: every graph's GDesc, the pools' lengths, the chain tables' row
// length (ccap >= 1) and the largest graph.
struct BatchPools {
  std::vector<GDesc> hd;
  int64_t Etot = 0, Ktot = 0, Rtot = 0, Stot = 0;
  int ccap = 0, Emax = 0;
};

// Both sources of graphs lay out here (hge_batch::stage, stage_generated).  The chain
// check cannot fire for generated graphs (HGE_GOSSIP_MAX_EVENTS is 3,000,000 < 2^24);
// applying it to both changes nothing.
inline BatchPools layout(int SM, const GraphSize* gs, int G) {
  BatchPools p;
  p.hd.assign((size_t)G, GDesc{});
  p.ccap = 1;
  for (int g = 0; g < G; g++) {
    GDesc& d = p.hd[(size_t)g];
    d.eo = p.Etot;
    d.E = gs[g].E;
    d.co = (int32_t)p.Ktot;
    d.K = gs[g].K;
    d.ro = (int32_t)p.Rtot;
    // a round r + 1 exists only once >= SM witnesses of round r do: R <= E / SM + 1
    d.Rcap = d.E / SM + 2;
    p.Etot += d.E;
    p.Ktot += d.K;
    p.Rtot += d.Rcap;
    p.Stot += gs[g].subs;
    p.ccap = std::max(p.ccap, (int)gs[g].chain);
    p.Emax = std::max(p.Emax, d.E);
    if (p.Rtot >= INT32_MAX || p.Ktot >= INT32_MAX) throw hge::Error{HGE_ERR_CAPACITY, "batch too large"};
  }
  if (p.ccap >= (1 << 24)) throw hge::Error{HGE_ERR_CAPACITY, "batch graph with a chain of 2^24 events or more"};
  return p;
}

}  // namespace hgb
