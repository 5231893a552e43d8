// hge_batch.hip — many independent small hashgraphs replayed together
// (BASELINE config 5: a Monte Carlo batch of 32-participant graphs with
// Byzantine forkers).  C ABI: hge_batch_* in include/hge.h.
//
// The single-graph engine (hge_engine.hip) sizes its grids from one graph and
// makes a few host round trips per replay; driving 1,024 of them means ~50k
// launches per batch from host threads (58M ev/s, the
// host bound).  Here every stage is ONE launch over the whole batch, and the
// graph's whole call schedule runs inside the consensus kernel:
//
//   kb_coords     lastAncestors rows in insertion order (hashgraph.go:399-463), one
//                 256-thread workgroup per graph: runs of mutually independent
//                 events computed together, a row the max of its parents' rows
//                 (from an LDS ring of the chunk or a snapshot of the chain heads).
//   kb_fd         firstDescendants in run layout FDT[j][c][p], one wave per (graph,
//                 chain j): chain-j event k is the first chain-j descendant of
//                 chain-c positions (LA[(j,k-1)][c], LA[(j,k)][c]] (hashgraph.go:466-494);
//   kb_fdrows     ... transposed to rows FD[c][p][j] through LDS tiles.
//   kb_front      Round / Witness of every event (hashgraph.go:220-305) by the round
//                 frontier: C_{r+1}[c] = the SM-th smallest over the round-r
//                 members d of the first position of chain c that strongly sees d,
//                 one 1024-thread workgroup per graph; each witness's strongly-see /
//                 see bitsets over the previous round's witnesses (the vote adjacency
//                 of DecideFame).
//   kb_consensus  for every call point in order, one 4-wave workgroup per graph:
//                 DivideRounds' bookkeeping, DecideFame (hashgraph.go:598-664: lane
//                 = voter y, witnesses x over the waves, a vote set a 64-bit mask,
//                 the `break` as the first y whose tally reaches SM, missing votes as
//                 nays, coin rounds), DecideRoundReceived (hashgraph.go:676-721: x is
//                 seen by more than half of the famous witnesses iff index(x) <=
//                 theta(round, creator(x)), the (|F|/2+1)-th largest lastAncestor of
//                 the famous witnesses), MedianTimestamp (:762-770) and the
//                 ConsensusSorter sort of the call's batch (consensus_sorter.go:36-59,
//                 PRN = 0) in LDS.
//
// Opt-in (hge_batch_set_delivery): the kernels that write the order (kb_sort,
// kb_consensus) write it, the per-call batch sizes and, in their DLV instances, the
// ordered events' round received and consensus timestamp into mapped pinned host
// memory, so a run ends with every graph's commit stream on the host
// (tests/test_gpu_batch_commit.py).
//
// Everything on the path is integer; results are bit-exact with the oracle
// (tests/test_gpu_batch.py, tests/test_gpu_mc.py: every graph's full-state digest).
//
// This file holds the kernels (with hge_batch_bulk.hip, hge_batch_gen.hip and
// hge_batch_stats.hip).  The host side, struct hge_batch in parts by lifetime and the C
// ABI, is hge_batch_host.hip, included at the end: one translation unit.  Which instance
// of a kernel a run launches and where a graph lies in the pools are decided in
// hge_batch_plan.h (host only, tested on the CPU).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/hge.h"
#include "hge_hip.h"
#include "hge_batch_plan.h"  // GDesc, the launch plan, the pools' layout

namespace hgb {

constexpr int32_t INF = 0x7fffffff;

// batch tables (device pointers); per-graph blocks are addressed through GDesc
struct BT {
  int N, SM, ccap;
  const GDesc* gd;
  const int32_t *cr, *ix, *sp, *op, *oc, *ntx, *clen;  // oc: the other-parent's creator
  const int64_t* ts;
  const uint64_t* S;  // 4 limbs per event, most significant first
  const uint8_t* coin;
  const int32_t* chain;  // [g][N][ccap] local event ids
  const int64_t* tsch;   // [g][N][ccap] timestamps in chain layout
  const int64_t* calls;  // accepted-event count at each call point
  int32_t* LA;           // [eo + x][N] lastAncestors (positions; -1 none)
  int32_t* FDT;          // [g][j][c][ccap] firstDescendants in run layout (INF none)
  int32_t* FD;           // [g][c][p][N] firstDescendants rows of chain positions (INF none)
  const uint64_t* Sch;   // [g][c][p] limb 0 of S in chain layout (the sort key)
  const int32_t* ntxch;  // [g][c][p] transaction counts in chain layout
  int32_t* round;
  uint8_t* wit;
  int32_t* rr;
  int64_t* cts;
  int32_t *W, *WIX, *WFD;      // [ro + r][N] witness id / its index, [ro + r][N][N] its FD row
  uint8_t* WCOIN;              // [ro + r][N] the witness's coin (middleBit)
  uint64_t *ssb, *seeb;        // [ro + r][N] bitsets over round r-1's witness creators
  int8_t* fame;                // [ro + r][N] 0 undefined, 1 true, 2 false (persisted)
  int32_t *rcnt, *ver, *thv;   // [ro + r] events in the round so far, fame/witness version, theta's version
  int32_t* th;                 // [ro + r][N] receive thresholds
  int32_t *U, *Ur, *Ucp;       // [eo + k] undetermined list past LDS: id, round, creator << 24 | index
  // The commit stream (with ord_rr / ord_cts at the end).  Store-only: with delivery on
  // (hge_batch_set_delivery) these point into mapped host memory, so no kernel may
  // load from them.
  int32_t* order;              // [eo + k] consensus order
  int64_t* counts;             // [co + c] batch size of call c
  int64_t* scal;               // [g][8] R, LCR, LCRE, transactions, ordered, undetermined, error
  int32_t* krr;                // [2 eo + k] sort scratch for call batches past the LDS keys
  int64_t* kct;
  uint64_t* ks0;
  int32_t* kid;
  uint64_t* dbg;               // diagnostics: per-graph section cycles (null: off)
  // the bulk call schedule (hge_batch_bulk.hip)
  const int32_t* glist;  // kb_consensus: the graphs it replays (null: every graph)
  const int32_t* cg;     // [co + c] the graph of each call
  int32_t *Rc, *xcall;   // [co + c] Rounds() after call c's DivideRounds; [eo + x] x's insertion call
  int32_t* rfirst;       // [ro + r] the first call with R_c >= r (r <= the last call's R)
  uint64_t* arr;         // [eo + k] the witnesses in insertion order: call << 32 | round << 8 | creator
  uint64_t* Dp;          // [((co + c) * NS + s) * 2 + {0, 1}], NS <= BNS DecideFame's decided / famous masks
  int32_t* gx;           // [g][16] per-graph internals (GX_*)
  int4* ivh;             // [(ro + r) * BVCAP + k] receive intervals: first call, end call, theta slot
  uint64_t* ivF;         // ... and their famous witnesses
  int32_t *nivl, *fsuf;  // [ro + r] intervals per round; the suffix minimum of their first starts
  int32_t *thp, *thR;    // [g * BICAP + s][N] receive thresholds; [g * BICAP + s] their round
  uint64_t* thF;         // [g * BICAP + s] their famous witnesses
  // chain layout [g][c][p] (kb_receive's lanes are consecutive positions of a chain)
  int32_t* roundch;      // rounds
  int32_t *rcall, *rrank;  // the call that receives the event (-1 none), its slot in that call's bucket
  int32_t* rrch;         // round received
  int32_t* rslot;        // the receiving interval's threshold slot (-1 none)
  int64_t* ctsch;        // consensus timestamps
  int32_t *bcnt, *boff;  // [co + c] call buckets: size, offset
  int4* wl;              // the non-empty buckets (graph, size, offset in the graph's order)
  int32_t* wlc;          // their count
  int64_t* gctx;         // [g] ConsensusTransactions
  int2* cinf;            // [eo + x] kb_levels' records for kb_coords
  // The commit stream's records beside `order` (store-only like it; null: not delivered).
  // Only the DLV instances of kb_sort and kb_consensus touch them: as a run-time pointer
  // test the extra stores cost kb_sort<256, 0, 1024> a wave per SIMD and
  // kb_consensus<32, 4> scratch (profiles/batch_commit/resource_usage.txt).  Last, so
  // that every other field keeps its offset in the kernels' arguments.
  int32_t* ord_rr;       // [eo + k] round received of order[eo + k]
  int64_t* ord_cts;      // [eo + k] its consensus timestamp
  // kb_consensus: the call whose batch committed x (the bulk path's is rcall), read by the
  // statistics pass (hge_batch_stats.hip).  After ord_cts for the same reason.
  int32_t* xcc;          // [eo + x]
};

__device__ __forceinline__ int rl(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint64_t rl64(uint64_t v, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ int64_t rl64s(int64_t v, int l) { return (int64_t)rl64((uint64_t)v, l); }
__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// mutable per-graph state in global memory is written and read by different
// lanes of the graph's wave: device-coherent loads bypass a stale L1 line
template <typename T>
__device__ __forceinline__ T ld(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T, typename V>
__device__ __forceinline__ void st(T* p, V v) {
  __hip_atomic_store(p, (T)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wsync() { __builtin_amdgcn_wave_barrier(); }
// a workgroup barrier ordering LDS accesses only: no wait for outstanding global stores
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// ---------------------------------------------------------------------------
// A graph's work is a dependent chain (insertion order, rounds, the call schedule),
// so each kernel below gives one graph one workgroup and hides its latency inside
// it: the chain's independent steps spread over the waves, the next chunk's loads
// issued before the current one is consumed, and the consensus kernel's state of
// the last RW rounds (witnesses, vote bitsets, fame, thresholds) and the
// undetermined list kept in LDS.

// lastAncestors (InitEventCoordinates, hashgraph.go:399-463): in insertion order,
// LA[x] = max(LA[sp], LA[op]) with LA[x][creator] = index.  The events go in chunks of
// 64.  kb_levels gives every event of every chunk, all graphs at once, its level inside
// its chunk (one above its in-chunk parents) and its parents' row sources; kb_coords
// (one workgroup per graph) then walks the chunks, one step per level.
//
// kb_levels: one wave per (graph, chunk), lane = event.  A parent's row source is a
// row of the chunk's LDS ring (the parent is in the chunk), the chain head as of the
// chunk's start (the parent is its chain's last event before the chunk: the
// self-parent always is, admission "Self-parent not last known", hashgraph.go:390-393,
// and the other-parent nearly always), or HBM.  cinf[x] = {srcA | srcB << 8 |
// level << 16 | last << 23 | levels << 24, creator | index << 8}; last: x is its
// chain's last event in the chunk (its row becomes that chain's head).
__global__ __launch_bounds__(256) void kb_levels(BT t) {
  const int g = blockIdx.y, lane = threadIdx.x & 63;
  const GDesc d = t.gd[g];
  const int base = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  if (base >= d.E) return;
  const int N = t.N, cc = t.ccap, i = base + lane;
  const bool on = i < d.E;
  const int sp = on ? t.sp[d.eo + i] : -1, op = on ? t.op[d.eo + i] : -1;
  const int cr = on ? t.cr[d.eo + i] : 0, oc = on ? t.oc[d.eo + i] : 0, ix = on ? t.ix[d.eo + i] : 0;
  const int32_t* chg = t.chain + (int64_t)g * N * cc;
  const int32_t* lng = t.clen + (int64_t)g * N;
  // the event after position q of chain c (INF: none)
  auto next = [&](int c, int q) { return q + 1 < lng[c] ? chg[(int64_t)c * cc + q + 1] : INF; };
  auto src = [&](int p, int c) -> int {
    if (p < 0) return -1;
    if (p >= base) return p - base;
    return next(c, t.ix[d.eo + p]) >= base ? 64 + c : -2;
  };
  const int sa = src(sp, cr), sb = src(op, oc);
  const bool last = on && next(cr, ix) >= base + 64;
  const int ps = on && sp >= base ? sp - base : -1, po = on && op >= base ? op - base : -1;
  int lvl = 0;
  while (true) {  // parents precede their children: settles after the chunk's depth
    const int x = __shfl(lvl, ps < 0 ? 0 : ps), y = __shfl(lvl, po < 0 ? 0 : po);
    const int nl = max(ps >= 0 ? x + 1 : 0, po >= 0 ? y + 1 : 0);
    const bool ch = nl != lvl;
    lvl = nl;
    if (!ballot(ch)) break;
  }
  const int nlev = wave_max(on ? lvl : 0) + 1;
  if (on)
    t.cinf[d.eo + i] = make_int2((sa & 0xFF) | (sb & 0xFF) << 8 | lvl << 16 | (last ? 1 << 23 : 0) | nlev << 24,
                                 cr | ix << 8);
}

// kb_coords: one workgroup per graph (SPLIT = 1) or per (graph, 1/SPLIT of the columns:
// every column's recurrence is independent of the others), NT threads; thread (s, k) owns column k of the
// chunk's events s, s + SL, ... (SL = NT / NM), their kb_levels records in registers
// (the next chunk's loaded while this one runs).  A step computes one level: every
// event of it reads its parents' rows from LDS (ring or heads) or HBM and writes its
// own; one LDS-scoped barrier per step (the row stores to HBM are never waited for
// inside a chunk).  After the chunk the chains' last events' rows become the heads,
// behind a full barrier (which also completes the chunk's HBM stores).
// LV = false (past two graphs per CU: the chip is full, and kb_levels' extra pass
// measured 1.04 -> 1.42 ms at 1,024 graphs), the earlier form: wave 0 levels each chunk
// itself, and a step computes up to SL events of one level together (their rows depend
// only on rows already final).  The parents' row sources are found the same way (the
// heads' ids kept in LDS); wave 0 loads the next chunk's event records while this
// chunk's steps run.
template <int NM, int NT, bool LV, int SPLIT = 1>
__global__ __launch_bounds__(NT) void kb_coords(BT t) {
  if constexpr (LV) {
  constexpr int CPW = NM / SPLIT, SL = NT / CPW, EPT = 64 / SL;
  static_assert(EPT >= 1 && SL * EPT == 64, "slots tile the chunk");
  const GDesc d = t.gd[blockIdx.x / SPLIT];
  const int part = blockIdx.x % SPLIT;
  const int N = t.N, tid = threadIdx.x, s = tid / CPW, kl = tid - (tid / CPW) * CPW, k = part * CPW + kl;
  // rows 0..63: the chunk's ring; 64 + c: chain c's head row as of the chunk's start
  // (this workgroup's CPW columns: the recurrence is column by column)
  __shared__ int32_t rows[64 + NM][CPW];
  for (int i = tid; i < NM * CPW; i += NT) rows[64 + i / CPW][i - (i / CPW) * CPW] = -1;
  __syncthreads();
  int32_t* LA = t.LA + d.eo * N;
  const int2* ci = t.cinf + d.eo;
  int2 nx[EPT];
  int nlv = 0;
  auto fetch = [&](int b) {
#pragma unroll
    for (int u = 0; u < EPT; u++) {
      const int e = b + s + SL * u;
      nx[u] = e < d.E ? ci[e] : make_int2(0, 0);
    }
    nlv = b < d.E ? ci[b].x >> 24 : 0;  // the chunk's level count (its first event's record)
  };
  fetch(0);
  for (int base = 0; base < d.E; base += 64) {
    int2 in[EPT];
#pragma unroll
    for (int u = 0; u < EPT; u++) in[u] = nx[u];
    const int nlev = nlv;
    if (base + 64 < d.E) fetch(base + 64);
    int val[EPT];
    for (int l = 0; l < nlev; l++) {
#pragma unroll
      for (int u = 0; u < EPT; u++) {
        const int e = s + SL * u;
        if (base + e < d.E && k < N && ((in[u].x >> 16) & 63) == l) {
          const int sa = (int)(int8_t)(in[u].x & 0xFF), sb = (int)(int8_t)((in[u].x >> 8) & 0xFF);
          const int a = sa >= 0 ? rows[sa][kl] : sa == -1 ? -1 : ld(&LA[(int64_t)t.sp[d.eo + base + e] * N + k]);
          const int b = sb >= 0 ? rows[sb][kl] : sb == -1 ? -1 : ld(&LA[(int64_t)t.op[d.eo + base + e] * N + k]);
          const int v = k == (in[u].y & 0xFF) ? in[u].y >> 8 : max(a, b);
          val[u] = v;
          rows[e][kl] = v;
          LA[(int64_t)(base + e) * N + k] = v;
        }
      }
      lds_barrier();
    }
    // the heads after the chunk (every read of the old heads is behind the last barrier)
#pragma unroll
    for (int u = 0; u < EPT; u++)
      if (base + s + SL * u < d.E && k < N && (in[u].x >> 23 & 1)) rows[64 + (in[u].y & 0xFF)][kl] = val[u];
    __syncthreads();  // also: the chunk's row stores are complete before the next one reads HBM
  }
  } else {
  constexpr int SL = NT / NM;  // event slots per step
  const GDesc d = t.gd[blockIdx.x];
  const int N = t.N, tid = threadIdx.x, s = tid / NM, k = tid - (tid / NM) * NM;
  // rows 0..63: the chunk's ring; 64 + c: chain c's head row as of the chunk's start
  __shared__ int32_t rows[64 + NM][NM];
  __shared__ int32_t headid[NM];
  // per event of the chunk: its parents' row sources (a row of `rows`, -1 none,
  // -2 HBM), creator, index; the parents' ids for the HBM case
  __shared__ int4 einfo[64];
  __shared__ int32_t msp[64], mop[64];
  __shared__ int32_t ord[64];     // the chunk's events by level
  __shared__ int32_t gst[130];    // the steps: ord[gst[i] .. gst[i + 1])
  __shared__ int32_t clast[NM];   // the chunk's last event per chain (-1)
  __shared__ int s_ng;
  for (int i = tid; i < NM * NM; i += NT) rows[64 + i / NM][i - (i / NM) * NM] = -1;
  if (tid < NM) headid[tid] = -1;
  __syncthreads();
  int32_t* LA = t.LA + d.eo * N;
  // wave 0 holds the next chunk's event records (loaded while this chunk's steps run)
  int nsp = -1, nop = -1, ncr = 0, noc = 0, nix = 0;
  auto fetch = [&](int b) {
    const int i = b + tid;
    const bool on = i < d.E;
    nsp = on ? t.sp[d.eo + i] : -1;
    nop = on ? t.op[d.eo + i] : -1;
    ncr = on ? t.cr[d.eo + i] : 0;
    noc = on ? t.oc[d.eo + i] : 0;
    nix = on ? t.ix[d.eo + i] : 0;
  };
  if (tid < 64) fetch(0);
  for (int base = 0; base < d.E; base += 64) {
    const int cnt = min(64, d.E - base);
    if (tid < 64) {
      const int sp = nsp, op = nop, cr = ncr, oc = noc;
      const bool on = base + tid < d.E;
      auto src = [&](int p, int c) -> int {
        return p < 0 ? -1 : p >= base ? p - base : headid[c] == p ? 64 + c : -2;
      };
      einfo[tid] = make_int4(src(sp, cr), src(op, oc), cr, nix);
      msp[tid] = sp;
      mop[tid] = op;
      if (tid < NM) clast[tid] = -1;
      wsync();
      if (on) atomicMax(&clast[cr], tid);
      // levels inside the chunk: one above the in-chunk parents (parents precede
      // their children, so the passes settle after the chunk's depth); the events of
      // a level are independent and take the steps of that level, SL at a time
      const int ps = on && sp >= base ? sp - base : -1, po = on && op >= base ? op - base : -1;
      int lvl = 0;
      while (true) {
        const int a = __shfl(lvl, ps < 0 ? 0 : ps), b = __shfl(lvl, po < 0 ? 0 : po);
        const int nl = max(ps >= 0 ? a + 1 : 0, po >= 0 ? b + 1 : 0);
        const bool ch = nl != lvl;
        lvl = nl;
        if (!ballot(ch)) break;
      }
      const int maxl = wave_max(on ? lvl : 0);
      const uint64_t below = tid ? (~0ull >> (64 - tid)) : 0ull;
      int pos = 0, ng = 0;
      for (int l = 0; l <= maxl; l++) {
        const uint64_t m = ballot(on && lvl == l);
        const int c_l = __popcll(m);
        if (on && lvl == l) ord[pos + __popcll(m & below)] = tid;
        for (int q = 0; q < c_l; q += SL) {
          if (tid == 0) gst[ng] = pos + q;
          ng++;
        }
        pos += c_l;
      }
      if (tid == 0) {
        gst[ng] = cnt;
        s_ng = ng;
      }
      if (base + 64 < d.E) fetch(base + 64);
    }
    __syncthreads();
    const int ng = s_ng;
    for (int gi = 0; gi < ng; gi++) {
      const int q0 = gst[gi], q1 = gst[gi + 1];
      const bool on = q0 + s < q1 && k < N;
      if (on) {
        const int e = ord[q0 + s];
        const int4 ei = einfo[e];
        const int a = ei.x >= 0 ? rows[ei.x][k] : ei.x == -1 ? -1 : ld(&LA[(int64_t)msp[e] * N + k]);
        const int b = ei.y >= 0 ? rows[ei.y][k] : ei.y == -1 ? -1 : ld(&LA[(int64_t)mop[e] * N + k]);
        const int val = k == ei.z ? ei.w : max(a, b);
        rows[e][k] = val;
        LA[(int64_t)(base + e) * N + k] = val;
      }
      lds_barrier();
    }
    // the heads after the chunk
    if (k < N)
      for (int c = s; c < N; c += SL) {
        const int l = clast[c];
        if (l >= 0) rows[64 + c][k] = rows[l][k];
      }
    if (tid < N && clast[tid] >= 0) headid[tid] = base + clast[tid];
    __syncthreads();  // also: the chunk's row stores are complete before the next one reads HBM
  }
  }
}


// The per-replay resets of the pooled tables in one launch (14 stream fills cost ~5 µs
// of launch each, ~70 µs of a 128-graph replay): segment k gets its 4-byte pattern,
// 16-byte stores over its whole 16-byte units, then the tail bytes.
struct ClrSeg {
  void* p;
  uint64_t bytes;
  uint32_t pat;
};
struct ClrList {
  ClrSeg s[16];
  int n;
};
__global__ __launch_bounds__(256) void kb_clear(ClrList L) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (uint64_t)gridDim.x * blockDim.x;
  for (int k = 0; k < L.n; k++) {
    const ClrSeg sg = L.s[k];
    const uint64_t n16 = sg.bytes >> 4;
    const uint4 v = make_uint4(sg.pat, sg.pat, sg.pat, sg.pat);
    uint4* q = (uint4*)sg.p;
    for (uint64_t i = tid; i < n16; i += nth) q[i] = v;
    for (uint64_t b = (n16 << 4) + tid; b < sg.bytes; b += nth) ((uint8_t*)sg.p)[b] = (uint8_t)sg.pat;
  }
}

// ---------------------------------------------------------------------------
// firstDescendants in run layout (UpdateAncestorFirstDescendant, hashgraph.go:466-494):
// chain-j event k is the first chain-j descendant of the chain-c positions
// (LA[(j,k-1)][c], LA[(j,k)][c]]; positions no chain-j event sees keep INF
// (MaxInt64).  One wave per (graph, chain j, slice of FCW columns): lane r holds row
// k0 + r of chain j (the slice's columns, registers); for each column c the 64 rows'
// runs tile one contiguous range of chain c's positions, so the stores of a column
// are contiguous across the lanes.  The next 64 rows' loads are in flight meanwhile.
// (Slices of 16 columns: a wave holding all 32 columns took 176 VGPRs, two waves per SIMD.)
constexpr int FCW = 16;
template <int NM>
__global__ __launch_bounds__(64 * (NM / FCW)) void kb_fd(BT t) {
  constexpr int NS_ = NM / FCW;
  // a (graph, chain) per workgroup, one wave per slice: the slices read the same LA rows
  // (one 128-byte line at N = 32) together on one CU instead of on two XCDs
  const int N = t.N, cc = t.ccap, lane = threadIdx.x & 63;
  const int w = blockIdx.x * NS_ + (threadIdx.x >> 6), g = w / (N * NS_), j = (w / NS_) % N, c0 = (w % NS_) * FCW;
  if (c0 >= N) return;
  const GDesc d = t.gd[g];
  const int32_t* LA = t.LA + d.eo * N;
  const int lenc = lane < N ? t.clen[g * N + lane] : 0;  // lane c's chain length (the INF tails)
  {
    const int lenj = t.clen[g * N + j];
    const int32_t* ch = t.chain + ((int64_t)g * N + j) * cc;
    int32_t* outj = t.FDT + ((int64_t)g * N + j) * N * cc;  // + c * cc + p
    const bool vec = (N & 3) == 0 && c0 + FCW <= N;  // 16-byte aligned slices
    int row[FCW], nrow[FCW];
    int carry[FCW];  // the last row's value of column c0 + c before the chunk (uniform)
#pragma unroll
    for (int c = 0; c < FCW; c++) carry[c] = -1;
    auto load = [&](int k0, int (&v)[FCW]) {
      const bool ok = k0 + lane < lenj;
      const int x = ok ? ch[k0 + lane] : 0;
      const int32_t* r = LA + (int64_t)x * N + c0;
      if (vec) {
#pragma unroll
        for (int c = 0; c < FCW; c += 4) {
          const int4 q = ok ? *(const int4*)(r + c) : make_int4(-1, -1, -1, -1);
          v[c] = q.x;
          v[c + 1] = q.y;
          v[c + 2] = q.z;
          v[c + 3] = q.w;
        }
      } else {
#pragma unroll
        for (int c = 0; c < FCW; c++) v[c] = ok && c0 + c < N ? r[c] : -1;
      }
    };
    if (lenj > 0) load(0, row);
    for (int k0 = 0; k0 < lenj; k0 += 64) {
      const bool more = k0 + 64 < lenj;
      if (more) load(k0 + 64, nrow);
      const bool ok = k0 + lane < lenj;
      const int last = min(64, lenj - k0) - 1;  // the chunk's last valid lane
#pragma unroll
      for (int c = 0; c < FCW; c++) {
        if (c0 + c < N) {
          const int up = __shfl_up(row[c], 1);
          const int a = lane == 0 ? carry[c] : up;  // positions (a, b] take k0 + lane
          const int b = ok ? row[c] : a;
          int32_t* out = outj + (int64_t)(c0 + c) * cc;
          for (int p = a + 1; p <= b; p++) out[p] = k0 + lane;
          carry[c] = rl(row[c], last);
        }
      }
      if (more) {
#pragma unroll
        for (int c = 0; c < FCW; c++) row[c] = nrow[c];
      }
    }
    // chain c's positions no chain-j event sees: one coalesced sweep per column
#pragma unroll
    for (int c = 0; c < FCW; c++) {
      if (c0 + c < N) {
        const int lc = rl(lenc, c0 + c);
        int32_t* out = outj + (int64_t)(c0 + c) * cc;
        for (int p = carry[c] + 1 + lane; p < lc; p += 64) out[p] = INF;
      }
    }
  }
}

// firstDescendants as rows in chain layout: FD[g][c][p][j] = FDT[j][c][p], through an
// LDS tile of 64 positions x N chains per step.  One workgroup per (graph, chain c).
template <int NM>
__global__ __launch_bounds__(256) void kb_fdrows(BT t) {
  const int g = blockIdx.x / t.N, c = blockIdx.x % t.N;
  const int N = t.N, cc = t.ccap, tid = threadIdx.x;
  __shared__ int32_t tile[NM][65];
  const int len = t.clen[g * N + c];
  for (int p0 = 0; p0 < len; p0 += 64) {
    for (int e = tid; e < N * 64; e += 256) {  // read along positions
      const int j = e >> 6, p = e & 63;
      tile[j][p] = p0 + p < len ? t.FDT[(((int64_t)g * N + j) * N + c) * cc + p0 + p] : INF;
    }
    __syncthreads();
    for (int e = tid; e < N * 64; e += 256) {  // write event rows
      const int p = e / N, j = e % N;
      if (p0 + p < len) t.FD[(((int64_t)g * N + c) * cc + p0 + p) * N + j] = tile[j][p];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Round / Witness by the round frontier, one 1024-thread workgroup per graph.
// Round(x) is a function of x's ancestry alone: the witnesses x strongly sees are
// its ancestors, so "the witnesses of the parent round inserted so far"
// (hashgraph.go:263-285) are all it can count.  With C_r[c] the first position of
// chain c whose round is >= r (rounds never decrease along a chain):
//   round(x) >= r + 1  <=>  x strongly sees >= SM of the members (d, C_r[d]),
//   fss_c(w) = the first position of chain c that strongly sees w
//            = SM-th smallest over i of FD[(i, FD[w][i])][c]
//     (x on chain c sees w's first descendant on chain i iff pos(x) >= that entry;
//     StronglySee counts those i, hashgraph.go:189-208),
//   C_{r+1}[c] = SM-th smallest over d of fss_c(C_r[d])  (the own-chain term at
//     least C_r[c] + 1: an event never strongly sees itself; matters at N = 1).
// The single-graph engine walks the same recurrence (k_fss / k_rounds_fss,
// hge_kernels.hip).  Per round: thread (member d, chain c) gathers the N rows
// FD[(i, FD[w_d][i])] at column c (one 128-byte row per half wave) and selects;
// then chain c's thread selects over the members.  Chain c's round-r events are
// the positions [C_r[c], C_{r+1}[c]), the first of them the witness; a witness's
// strongly-see bits over round r-1's witnesses are fss_c(w) <= its position, its
// see bits LA[x][d] >= index(w) (the vote adjacency of DecideFame).
template <int M>
__device__ __forceinline__ int kth_smallest(const int (&v)[M], int k) {
  // bisection over the value range: the smallest t with #{v <= t} >= k (INF when
  // fewer than k values are finite); positions span a few hundred, so ~9 counting
  // passes of M compares, register-light (a bitonic network held M values plus its
  // temporaries, ~88 VGPRs in kb_front: one 1,024-thread workgroup per CU)
  int lo = INF, hi = INT32_MIN, fin = 0;
#pragma unroll
  for (int i = 0; i < M; i++) {
    if (v[i] != INF) {
      lo = min(lo, v[i]);
      hi = max(hi, v[i]);
      fin++;
    }
  }
  if (fin < k) return INF;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < M; i++) cnt += v[i] <= mid;
    if (cnt >= k) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// NT: 1024 threads while the graphs fit one workgroup per CU; 512 past that, so two
// graphs share a CU (the kernel's ~88 VGPRs hold one 1024-thread workgroup per CU)
template <int NM, int NT>
__global__ __launch_bounds__(NT) void kb_front(BT t) {
  constexpr int NW = NT / 64;
  const int g = blockIdx.x;
  const GDesc d = t.gd[g];
  const int N = t.N, SM = t.SM, cc = t.ccap, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  __shared__ int32_t zrow[NM][NM];     // [member d][i]: the FD row of (d, C_r[d])
  __shared__ int32_t fssL[3][NM][NM];  // [r % 3][member d][chain c]: fss_c((d, C_r[d])), INF: no member
  __shared__ int32_t Cl[3][NM];        // C_{r-1}, C_r, C_{r+1} by r mod 3 (INF: none)
  __shared__ int32_t lenL[NM];
  __shared__ int s_more;
  const int32_t* FDg = t.FD + (int64_t)g * N * cc * N;  // [c][p][N]
  const int32_t* chg = t.chain + (int64_t)g * N * cc;   // [c][p] -> id
  const int32_t* LA = t.LA + d.eo * N;
  if (tid < N) {
    const int ln = t.clen[g * N + tid];
    lenL[tid] = ln;
    Cl[0][tid] = ln > 0 ? 0 : INF;  // the first event of a chain has no parents: round 0
    Cl[2][tid] = INF;
  }
  __syncthreads();
  // round r's outputs once C_{r+1} is known: the frontier ranges' rounds and witness
  // flags, the witness rows, and (r >= 1) each witness's bits over round r-1's
  auto outputs = [&](int r) {
    const int* Cp = Cl[(r + 2) % 3];
    const int* Cc = Cl[r % 3];
    const int* Cn = Cl[(r + 1) % 3];
    const int64_t row = (int64_t)(d.ro + r) * N;
    const int per = NT / N;  // threads per chain
    if (tid < per * N) {
      const int c = tid % N, k = tid / N;
      const int lo = Cc[c], hi = min(Cn[c], lenL[c]);
      if (lo != INF)
        for (int p = lo + k; p < hi; p += per) {
          const int x = chg[(int64_t)c * cc + p];
          t.round[d.eo + x] = r;
          t.roundch[(int64_t)g * N * cc + (int64_t)c * cc + p] = r;
          t.wit[d.eo + x] = p == lo;
          if (p == lo) {
            t.W[row + c] = x;
            t.WIX[row + c] = lo;
            t.WCOIN[row + c] = t.coin[d.eo + x];
          }
        }
    }
    if (r >= 1)
      for (int c = wv; c < N; c += NW) {  // one wave per witness of round r, lane = d
        const int lo = Cc[c], hi = min(Cn[c], lenL[c]);
        if (lo == INF || lo >= hi) continue;
        bool ss = false, see = false;
        if (lane < N) {
          const int pw = Cp[lane];
          if (pw != INF && pw < min(Cc[lane], lenL[lane])) {  // (lane, pw) is a witness of round r-1
            ss = fssL[(r + 2) % 3][lane][c] <= lo;
            const int x = chg[(int64_t)c * cc + lo];
            see = LA[(int64_t)x * N + lane] >= pw;
          }
        }
        const uint64_t bss = ballot(ss), bsee = ballot(see);
        if (lane == 0) {
          t.ssb[row + c] = bss;
          t.seeb[row + c] = bsee;
        }
      }
  };
  for (int r = 0;; r++) {
    if (r >= d.Rcap) {  // never for a consistent graph (R <= E / SM + 1)
      if (tid == 0) t.scal[(int64_t)g * 8 + 6] = 1;
      return;
    }
    const int* Cc = Cl[r % 3];
    int* Cn = Cl[(r + 1) % 3];
    // the members' FD rows
    for (int e = tid; e < N * N; e += NT) {
      const int dd = e / N, i = e - (e / N) * N;
      const int P = Cc[dd];
      zrow[dd][i] = P != INF ? FDg[((int64_t)dd * cc + P) * N + i] : INF;
    }
    __syncthreads();
    // fss_c of every member (c fastest: a half wave reads one 128-byte row; reading
    // the run layout FDT here instead, with no FD rows built, took 1.82 -> 2.69 ms at
    // 1,024 graphs)
    // One (member, chain) pair per thread (N^2 <= NT): round r - 1's outputs go out
    // while this round's gathers are in flight (its chain-id loads overlap them; the
    // outputs' reads of C_{r-2} and fss(r - 2) precede the barrier after which the
    // select overwrites C_{r-2}'s slot, and fssL holds three rounds).
    const bool one = N * N <= NT;
    if (one) {
      const int e = tid, dd = e / N, c = e - (e / N) * N;
      const bool act = e < N * N && Cc[dd] != INF;
      int v[NM];
#pragma unroll
      for (int i = 0; i < NM; i++) {
        const int z = act && i < N ? zrow[dd][i] : INF;
        v[i] = z != INF ? FDg[((int64_t)i * cc + z) * N + c] : INF;
      }
      if (r > 0) outputs(r - 1);
      int f = INF;
      if (act) {
        f = kth_smallest<NM>(v, SM);
        if (dd == c && f != INF) f = max(f, Cc[c] + 1);
      }
      if (e < N * N) fssL[r % 3][dd][c] = f;
    } else {
      for (int e = tid; e < N * N; e += NT) {
        const int dd = e / N, c = e - (e / N) * N;
        int f = INF;
        if (Cc[dd] != INF) {
          int v[NM];
#pragma unroll
          for (int i = 0; i < NM; i++) {
            const int z = i < N ? zrow[dd][i] : INF;
            v[i] = z != INF ? FDg[((int64_t)i * cc + z) * N + c] : INF;
          }
          f = kth_smallest<NM>(v, SM);
          if (dd == c && f != INF) f = max(f, Cc[c] + 1);
        }
        fssL[r % 3][dd][c] = f;
      }
    }
    __syncthreads();
    // the next frontier
    if (wv == 0) {
      int nxt = INF;
      if (lane < N && Cc[lane] != INF) {
        int v[NM];
#pragma unroll
        for (int dd = 0; dd < NM; dd++) v[dd] = dd < N ? fssL[r % 3][dd][lane] : INF;
        const int sel = kth_smallest<NM>(v, SM);
        nxt = sel < lenL[lane] ? sel : INF;
      }
      if (lane < N) Cn[lane] = nxt;
      const uint64_t any = ballot(lane < N && nxt != INF);
      if (lane == 0) s_more = any != 0;
    }
    __syncthreads();
    if (!one) outputs(r);
    if (!s_more) {  // uniform: written before the barrier above
      if (one) outputs(r);
      break;
    }
  }
}

// ---------------------------------------------------------------------------
// consensus sorter keys (consensus_sorter.go:36-59 with PRN = 0): roundReceived,
// consensus timestamp, S (4 limbs), then the id (S never ties for real signatures)
__device__ __forceinline__ bool key_less(const BT& t, int64_t eo, int ra, int64_t ca, uint64_t sa, int ia,
                                         int rb, int64_t cb, uint64_t sb, int ib) {
  if (ra != rb) return ra < rb;
  if (ca != cb) return ca < cb;
  if (sa != sb) return sa < sb;
  for (int l = 1; l < 4; l++) {
    const uint64_t a = t.S[(eo + ia) * 4 + l], b = t.S[(eo + ib) * 4 + l];
    if (a != b) return a < b;
  }
  return ia < ib;
}

// Bitonic networks over the whole workgroup.  Stage (size, stride): thread q of the
// pair loop compares a = 2q - (q & (stride - 1)) and a + stride; for stride <= 64 a
// wave's 64 pairs stay inside its own 128 slots (also on the next pass of the q
// loop, 2 blockDim slots further), so two consecutive such stages need only the
// wave's own sync; a block barrier brackets every wider stage.
__device__ __forceinline__ void stage_sync(int size, int stride) {
  const int next = stride > 1 ? stride >> 1 : size;  // the next stage's stride
  if (stride > 64 || next > 64) __syncthreads();
  else wsync();
}

// n keys (padded to a power of two with sentinels, id INF, that order after every
// key) in the graph's global scratch (device-coherent accesses: threads exchange
// keys between stages)
__device__ void sort_keys_g(const BT& t, int64_t eo, int n, int32_t* kr, int64_t* kc, uint64_t* ks, int32_t* ki) {
  const int tid = threadIdx.x, NT = blockDim.x;
  int P = 1;
  while (P < n) P <<= 1;
  for (int p = n + tid; p < P; p += NT) st(ki + p, INF);
  __threadfence_block();
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int q = tid; q < P / 2; q += NT) {
        const int a = 2 * q - (q & (stride - 1));
        const int b = a + stride;
        const bool up = (a & size) == 0;
        const int ia = ld(ki + a), ib = ld(ki + b);
        if (ia == INF && ib == INF) continue;
        int ra = 0, rb = 0;
        int64_t ca = 0, cb = 0;
        uint64_t sa = 0, sb = 0;
        if (ia != INF) {
          ra = ld(kr + a);
          ca = ld(kc + a);
          sa = ld(ks + a);
        }
        if (ib != INF) {
          rb = ld(kr + b);
          cb = ld(kc + b);
          sb = ld(ks + b);
        }
        const bool b_lt_a = ib == INF ? false : (ia == INF ? true : key_less(t, eo, rb, cb, sb, ib, ra, ca, sa, ia));
        const bool a_lt_b = ia == INF ? false : (ib == INF ? true : key_less(t, eo, ra, ca, sa, ia, rb, cb, sb, ib));
        if (up ? b_lt_a : a_lt_b) {
          st(kr + a, rb);
          st(kr + b, ra);
          st(kc + a, cb);
          st(kc + b, ca);
          st(ks + a, sb);
          st(ks + b, sa);
          st(ki + a, ib);
          st(ki + b, ia);
        }
      }
      __threadfence_block();
      stage_sync(size, stride);
    }
  }
}

// the same network in LDS over packed keys: kri = roundReceived << 16 | id (both
// below 65,535: the host checks, sentinel 0xFFFFFFFF), n padded to a power of two
// P <= the arrays' size
__device__ void sort_keys_lds(const BT& t, int64_t eo, int n, uint32_t* kri, int64_t* kc, uint64_t* ks) {
  const int tid = threadIdx.x, NT = blockDim.x;
  int P = 1;
  while (P < n) P <<= 1;
  for (int p = n + tid; p < P; p += NT) kri[p] = 0xFFFFFFFFu;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int q = tid; q < P / 2; q += NT) {
        const int a = 2 * q - (q & (stride - 1));
        const int b = a + stride;
        const bool up = (a & size) == 0;
        const uint32_t pa = kri[a], pb = kri[b];
        const bool na = pa == 0xFFFFFFFFu, nb_ = pb == 0xFFFFFFFFu;
        if (na && nb_) continue;
        const int ra = (int)(pa >> 16), ia = (int)(pa & 0xFFFFu), rb = (int)(pb >> 16), ib = (int)(pb & 0xFFFFu);
        const int64_t ca = na ? 0 : kc[a], cb = nb_ ? 0 : kc[b];
        const uint64_t sa = na ? 0 : ks[a], sb = nb_ ? 0 : ks[b];
        const bool b_lt_a = nb_ ? false : (na ? true : key_less(t, eo, rb, cb, sb, ib, ra, ca, sa, ia));
        const bool a_lt_b = na ? false : (nb_ ? true : key_less(t, eo, ra, ca, sa, ia, rb, cb, sb, ib));
        if (up ? b_lt_a : a_lt_b) {
          kri[a] = pb;
          kri[b] = pa;
          kc[a] = cb;
          kc[b] = ca;
          ks[a] = sb;
          ks[b] = sa;
        }
      }
      stage_sync(size, stride);
    }
  }
}

// ascending bitonic sorting networks over M register values (M a power of two)
template <int M>
__device__ __forceinline__ void sort_regs32(int32_t (&v)[M]) {
#pragma unroll
  for (int size = 2; size <= M; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1)
#pragma unroll
      for (int i = 0; i < M; i++) {
        const int j = i ^ stride;
        if (j > i) {
          const bool up = (i & size) == 0;
          const int32_t a = v[i], b = v[j];
          v[i] = up ? min(a, b) : max(a, b);
          v[j] = up ? max(a, b) : min(a, b);
        }
      }
}
template <int M>
__device__ __forceinline__ void sort_regs(int64_t (&v)[M]) {
#pragma unroll
  for (int size = 2; size <= M; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1)
#pragma unroll
      for (int i = 0; i < M; i++) {
        const int j = i ^ stride;
        if (j > i) {
          const bool up = (i & size) == 0;
          const int64_t a = v[i], b = v[j];
          const bool sw = up ? a > b : a < b;
          v[i] = sw ? b : a;
          v[j] = sw ? a : b;
        }
      }
}

// ---------------------------------------------------------------------------
// The graph's call schedule in order, one workgroup of NWV waves per graph.  LDS
// holds the state of the rounds [R - RW, R) (witnesses and their indexes, vote
// bitsets, coins, fame, event counts, versions, receive thresholds and famous
// masks) and the undetermined list with each event's round, creator and index;
// rounds below the window and lists past UL entries live in global memory, where
// every mutation is also written.  Per call:
//   DivideRounds    wave 0 (the other waves compute the same scalars from the same
//                   loads: R, the list length, its lowest round);
//   DecideFame      rounds i split over the waves (each round's fame is decided from
//                   the vote adjacency alone), LastConsensusRound = the highest
//                   decided round, folded through LDS;
//   thresholds      rounds split over the waves;
//   round received  the list in spans of NWV x CPW chunks of 64: pass 1 loads a
//                   span's entries into registers and finds each one's round
//                   received, a prefix over the chunks' counts places the call's
//                   batch and the remaining entries (compacted in place: a span's
//                   entries move only below its own start), pass 2 takes the median
//                   timestamps and writes both;
//   FindOrder       the batch's bitonic sort over the whole workgroup.
// OCC: workgroups per CU the register budget is sized for.  One graph per CU
// leaves the compiler its 230 VGPRs; with more graphs than two per CU, 4 per CU
// (128 VGPRs, a few spills) take the whole batch in one pass.
template <int NM, int OCC, bool DLV>
__global__ __launch_bounds__(256, OCC) void kb_consensus(BT t) {
  // KB: the LDS sort's capacity, a power of two (the network pads to one)
  constexpr int NWV = 4, RW = 8, UL = 1536, KB = 1024, CPW = 2, NCH = NWV * CPW, SPAN = 64 * NCH;
  const int g = t.glist ? t.glist[blockIdx.x] : blockIdx.x;
  const GDesc d = t.gd[g];
  const int N = t.N, SM = t.SM, cc = t.ccap;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, NT = NWV * 64;
  const int64_t eo = d.eo;
  const int32_t* LA = t.LA + eo * N;
  const int32_t* FDg = t.FD + (int64_t)g * N * cc * N;  // [c][p][N]
  const int64_t* tschg = t.tsch + (int64_t)g * N * cc;
  __shared__ int32_t wid[RW][NM], wix[RW][NM], thL[RW][NM];
  __shared__ uint64_t ssbL[RW][NM], seebL[RW][NM];
  __shared__ uint64_t coinL[RW], fmL[RW];
  __shared__ int8_t fameL[RW][NM];
  __shared__ int32_t rcntL[RW], verL[RW], thvL[RW];
  // the undetermined list: creator << 24 | index, and round (the id is chain[c][index])
  __shared__ int32_t Ur_s[UL], Ucp_s[UL];
  __shared__ uint32_t kri[KB];  // roundReceived << 16 | id
  __shared__ int64_t kc[KB];
  __shared__ uint64_t ks[KB];
  __shared__ int32_t cntR[NCH], cntK[NCH];  // a span's chunks: received / kept entries
  __shared__ int32_t wred[3][NWV];          // per-wave partials: decided round, thresholds changed, kept minimum
  __shared__ int64_t wtx[NWV];              // per-wave transaction counts of the call's batch
  if (t.scal[(int64_t)g * 8 + 6]) return;  // the rounds pass failed: nothing to decide
  // packed LDS keys need ids and rounds below 65,535 (else the global-scratch sort)
  const bool lds_keys = d.E < 0xFFFF && d.Rcap < 0xFFFF;
  int R = 0, lcr = -1, lcre = 0, nord = 0, nU = 0, n_prev = 0;
  int umin = INF;  // the lowest round in the undetermined list
  int64_t ctx = 0;
  uint64_t cyc[6] = {0, 0, 0, 0, 0, 0};
  uint64_t t0_ = t.dbg ? __builtin_amdgcn_s_memtime() : 0;
#define HGB_STAMP(i)                                      \
  if (t.dbg && wv == 0) {                                 \
    const uint64_t t1_ = __builtin_amdgcn_s_memtime();    \
    cyc[i] += t1_ - t0_;                                  \
    t0_ = t1_;                                            \
  }
  bool ug = false;  // the undetermined list lives in global memory
  int32_t *Urg = t.Ur + eo, *Ucpg = t.Ucp + eo;
  const int32_t* chg = t.chain + (int64_t)g * N * cc;  // [c][p] -> id
  auto uget = [&](const int32_t* ls, const int32_t* gs, int i) -> int { return ug ? ld(&gs[i]) : ls[i]; };
  auto uput = [&](int32_t* ls, int32_t* gs, int i, int v) {
    if (ug) st(&gs[i], v);
    else ls[i] = v;
  };
  // ---- round accessors: LDS for [R - RW, R), global below ----
  auto res = [&](int r) { return r >= 0 && r < R && r >= R - RW; };
  auto row = [&](int r) { return (int64_t)(d.ro + r) * N; };
  auto W_ = [&](int r, int c) -> int { return res(r) ? wid[r & (RW - 1)][c] : t.W[row(r) + c]; };
  auto WIX_ = [&](int r, int c) -> int { return res(r) ? wix[r & (RW - 1)][c] : t.WIX[row(r) + c]; };
  auto fame_ = [&](int r, int c) -> int { return res(r) ? fameL[r & (RW - 1)][c] : ld(&t.fame[row(r) + c]); };
  auto rcnt_ = [&](int r) -> int { return res(r) ? rcntL[r & (RW - 1)] : ld(&t.rcnt[d.ro + r]); };
  auto ver_ = [&](int r) -> int { return res(r) ? verL[r & (RW - 1)] : ld(&t.ver[d.ro + r]); };
  auto thv_ = [&](int r) -> int { return res(r) ? thvL[r & (RW - 1)] : ld(&t.thv[d.ro + r]); };
  // single-writer updates (lane 0 or the lane of column c of the owning wave), written through
  auto set_rcnt = [&](int r, int v) {
    if (res(r)) rcntL[r & (RW - 1)] = v;
    st(&t.rcnt[d.ro + r], v);
  };
  auto set_ver = [&](int r, int v) {
    if (res(r)) verL[r & (RW - 1)] = v;
    st(&t.ver[d.ro + r], v);
  };
  for (int c = 0; c < d.K; c++) {
    const int n_c = (int)t.calls[d.co + c];
    const int nU0 = nU, umin0 = umin;  // the list before this call's events
    int rnmin;                         // the lowest round among the call's new events
    // ---- DivideRounds (hashgraph.go:573-588): the new events join the store ----
    {
      const int nn = n_c - n_prev;
      // the first 64 new events stay in registers (K <= 64: every call's)
      const bool on0 = lane < nn;
      const int x0 = n_prev + lane;
      const int r0 = on0 ? t.round[eo + x0] : -1;
      int rmax = r0, rlo = on0 ? r0 : INF;
      for (int b0 = n_prev + 64; b0 < n_c; b0 += 64)
        if (b0 + lane < n_c) {
          const int r = t.round[eo + b0 + lane];
          rmax = max(rmax, r);
          rlo = min(rlo, r);
        }
      rmax = wave_max(rmax);
      rnmin = wave_min(rlo);
      umin = min(umin, rnmin);
      const int Rnew = nn > 0 ? max(R, rmax + 1) : R;
      const int Rold = R;
      R = Rnew;
      const bool ug_new = !ug && nU + nn > UL;  // past the LDS list: it moves to global memory for good
      if (wv == 0) {
        // rounds entering the window: their immutable rows, fresh mutable state
        for (int r = max(Rold, Rnew - RW); r < Rnew; r++) {
          const int s = r & (RW - 1);
          const bool cl = lane < N;
          const int64_t rw_ = (int64_t)(d.ro + r) * N;
          const int w = cl ? t.W[rw_ + lane] : -1;
          if (cl) {
            wid[s][lane] = w;
            wix[s][lane] = t.WIX[rw_ + lane];
            ssbL[s][lane] = t.ssb[rw_ + lane];
            seebL[s][lane] = t.seeb[rw_ + lane];
            fameL[s][lane] = 0;
          }
          const uint64_t cm = ballot(cl && w >= 0 && t.WCOIN[rw_ + lane]);
          if (lane == 0) {
            coinL[s] = cm;
            fmL[s] = 0;
            rcntL[s] = 0;
            verL[s] = 0;
            thvL[s] = -1;
          }
        }
        wsync();
        // RoundEvents counts and witness versions, one writer per round; the
        // undetermined list grows by the new events in insertion order
        if (ug_new) {
          for (int i = lane; i < nU; i += 64) {
            st(&Urg[i], Ur_s[i]);
            st(&Ucpg[i], Ucp_s[i]);
          }
          ug = true;
        }
        const int w0 = on0 ? t.wit[eo + x0] : 0;
        const int cp0 = on0 ? (t.cr[eo + x0] << 24 | t.ix[eo + x0]) : 0;
        for (int b0 = n_prev; b0 < n_c; b0 += 64) {
          const int x = b0 + lane;
          const bool on = x < n_c;
          const int r = b0 == n_prev ? r0 : (on ? t.round[eo + x] : -1);
          const int w = b0 == n_prev ? w0 : (on ? t.wit[eo + x] : 0);
          const int cp = b0 == n_prev ? cp0 : (on ? (t.cr[eo + x] << 24 | t.ix[eo + x]) : 0);
          if (on) {
            uput(Ur_s, Urg, nU + (x - n_prev), r);
            uput(Ucp_s, Ucpg, nU + (x - n_prev), cp);
          }
          uint64_t rem = ballot(on);
          while (rem) {
            const int rr0 = rl(r, __ffsll((unsigned long long)rem) - 1);
            const uint64_t same = ballot(on && r == rr0);
            const bool nw = ballot(on && r == rr0 && w) != 0;
            if (lane == 0) {
              set_rcnt(rr0, rcnt_(rr0) + __popcll(same));
              if (nw) set_ver(rr0, ver_(rr0) + 1);
            }
            rem &= ~same;
            wsync();
          }
        }
        __threadfence_block();
      }
      ug = ug || ug_new;
      nU += nn;
      n_prev = n_c;
    }
    __syncthreads();
    HGB_STAMP(0)
    // ---- DecideFame (hashgraph.go:598-664) ----
    // Lane y is a voter of round j (y = lane, or lane & 31 with two half waves at
    // N <= 32); the witnesses x of round i are spread over the waves and half
    // waves, KX per lane group.  For one x and one j every present y's yays / nays
    // come at once (popcounts of its strongly-see bits against x's votes from round
    // j-1), the y loop's `break` is the first y whose tally reaches SM (a ballot's
    // lowest bit): x's votes from round j are the v of the y before it, its fame the
    // v of that y; later j decide again and the last decision stays.  Coin rounds
    // (diff % N == 0) vote the middle bit where no supermajority.  Missing votes are
    // nays.  Per round, the waves' "changed" / "undecided" flags meet in LDS.
    int mydec = -1;
    {
      constexpr int HV = NM <= 32 ? 2 : 1, XS = NWV * HV, KX = (NM + XS - 1) / XS;
      const int h = HV == 2 ? lane >> 5 : 0, y = HV == 2 ? lane & 31 : lane;
      const int xb = wv * HV + h;
      auto half = [&](uint64_t m) -> uint64_t { return HV == 2 ? (m >> (32 * h)) & 0xFFFFFFFFull : m; };
      for (int i = lcr + 1; i < R - 1; i++) {
        bool px[KX];
        int fv[KX], fv0[KX];
        uint64_t prev[KX];
#pragma unroll
        for (int k = 0; k < KX; k++) {
          const int x = xb + XS * k;
          const int xid = x < N ? W_(i, x) : -1;
          px[k] = xid >= 0 && xid < n_c;
          fv0[k] = px[k] ? fame_(i, x) : 0;
          fv[k] = fv0[k];
          prev[k] = 0;
        }
        for (int j = i + 1; j < R; j++) {
          const int diff = j - i;
          const bool rj = res(j);
          const int sj = j & (RW - 1);
          const int yid = y < N ? W_(j, y) : -1;
          const bool py = yid >= 0 && yid < n_c;
          uint64_t yb = 0;
          bool ycoin = false;
          if (py) {
            yb = diff == 1 ? (rj ? seebL[sj][y] : t.seeb[row(j) + y]) : (rj ? ssbL[sj][y] : t.ssb[row(j) + y]);
            ycoin = rj ? (coinL[sj] >> y) & 1 : t.WCOIN[row(j) + y] != 0;
          }
          const int tot = __popcll(yb);
#pragma unroll
          for (int k = 0; k < KX; k++) {
            const int x = xb + XS * k;
            uint64_t cur;
            if (diff == 1) {
              cur = half(ballot(py && ((yb >> x) & 1)));  // setVote(y, x, See(y, x))
            } else {
              const int yays = __popcll(yb & prev[k]), nays = tot - yays;
              const bool v = yays >= nays;
              const int tt = v ? yays : nays;
              if (diff % N != 0) {  // normal round: SetFame(x, v) and break at the first tt >= SM
                const uint64_t dm = half(ballot(py && tt >= SM));
                const uint64_t vm = half(ballot(py && v));
                if (dm) {
                  const int ys = __ffsll((unsigned long long)dm) - 1;
                  if (px[k]) fv[k] = (vm >> ys) & 1 ? 1 : 2;
                  cur = vm & ((1ull << ys) - 1);
                } else {
                  cur = vm;
                }
              } else {  // coin round: the middle bit of y's hash when no supermajority
                cur = half(ballot(py && (tt >= SM ? v : ycoin)));
              }
            }
            prev[k] = cur;
          }
        }
        bool chg = false, und = false;
#pragma unroll
        for (int k = 0; k < KX; k++) {
          const int x = xb + XS * k;
          const bool ch = px[k] && fv[k] != fv0[k];
          if (ch && y == 0) {
            if (res(i)) fameL[i & (RW - 1)][x] = (int8_t)fv[k];
            st(&t.fame[row(i) + x], (int8_t)fv[k]);
          }
          chg = chg || ch;
          und = und || (px[k] && fv[k] == 0);
        }
        const uint64_t bc = ballot(chg), bu = ballot(und);
        if (lane == 0) wred[0][wv] = (bc ? 1 : 0) | (bu ? 2 : 0);
        __threadfence_block();
        __syncthreads();
        int fl = 0;
        for (int w = 0; w < NWV; w++) fl |= wred[0][w];
        if ((fl & 1) && tid == 0) set_ver(i, ver_(i) + 1);
        if (!(fl & 2)) mydec = i;  // WitnessesDecided (roundInfo.go:78-85)
        __syncthreads();           // wred[0] is the next round's
      }
    }
    {
      // setLastConsensusRound (hashgraph.go:666-673): i runs upwards from lcr + 1 and
      // every decided i is past the last one set, so the highest decided round wins
      if (mydec >= 0) {
        lcr = mydec;
        lcre = mydec >= 1 ? rcnt_(mydec - 1) : 0;
      }
    }
    __syncthreads();  // the versions set above, for the thresholds
    HGB_STAMP(1)
    // ---- DecideRoundReceived (hashgraph.go:676-721) ----
    const int rmin = umin == INF ? R : umin;
    // decided rounds past the lowest undetermined round: the famous mask and the
    // thresholds theta (kept while the round's version holds: every fame change and
    // every new witness bumps the version, so thv == ver means decided and current)
    bool thchg = false;
    for (int i = rmin + 1 + wv; i < R; i += NWV) {
      const int v = ver_(i);
      if (thv_(i) == v) continue;
      const int w = lane < N ? W_(i, lane) : -1;
      const bool pw = w >= 0 && w < n_c;
      const int f = pw ? fame_(i, lane) : 0;
      if (ballot(pw && f == 0)) continue;  // not decided
      thchg = true;
      const uint64_t fm = ballot(pw && f == 1);
      const int m = __popcll(fm);
      int th = -2;  // no famous witness: nothing is received in the round
      if (lane < N && m > 0) {
        int vals[NM];
#pragma unroll
        for (int dd = 0; dd < NM; dd++) vals[dd] = (fm >> dd) & 1 ? LA[(int64_t)rl(w, dd) * N + lane] : -1;
        const int need = m / 2 + 1;  // len(s) > len(fws)/2
        int lo = -1, hi = t.clen[g * N + lane] - 1;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          int cnt = 0;
#pragma unroll
          for (int dd = 0; dd < NM; dd++) cnt += ((fm >> dd) & 1) && vals[dd] >= mid;
          if (cnt >= need) lo = mid;
          else hi = mid - 1;
        }
        th = lo;
      }
      if (lane < N) {
        if (res(i)) thL[i & (RW - 1)][lane] = th;
        st(&t.th[row(i) + lane], th);
      }
      wsync();
      if (lane == 0) {
        if (res(i)) {
          thvL[i & (RW - 1)] = v;
          fmL[i & (RW - 1)] = fm;
        }
        st(&t.thv[d.ro + i], v);
      }
      wsync();
    }
    if (lane == 0) wred[1][wv] = thchg;
    __threadfence_block();
    __syncthreads();
    for (int w = 0; w < NWV; w++) thchg = thchg || wred[1][w];
    HGB_STAMP(2)
    // the undetermined events in order: received ones become the call's batch (keys
    // to LDS, and to global scratch past KB), the rest stay (compacted in place).
    // With no thresholds (re)computed in this call no earlier entry can be received
    // now (a round leaving the decided state only removes candidates), so only the
    // call's new events are examined.
    // Nor can a new event be, unless some round above it is decided: then the call
    // receives nothing and the list only grew.
    bool scan = thchg;
    for (int i = rnmin == INF ? R : rnmin + 1; i < R && !scan; i++) scan = thv_(i) == ver_(i);
    const int u0 = thchg ? 0 : nU0;
    int nb = 0, nk = scan ? u0 : nU, kmin = INF;
    int64_t tx = 0;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int sb = u0; scan && sb < nU; sb += SPAN) {
      // pass 1: the span's entries (chunk k * NWV + wv of the span is this wave's k-th)
      int er[CPW], ecp[CPW], ef[CPW];
#pragma unroll
      for (int k = 0; k < CPW; k++) {
        const int e = sb + (k * NWV + wv) * 64 + lane;
        const bool on = e < nU;
        er[k] = on ? uget(Ur_s, Urg, e) : 0;
        ecp[k] = on ? uget(Ucp_s, Ucpg, e) : 0;
        int found = -1;
        if (on) {
          const int cx = ecp[k] >> 24, px = ecp[k] & 0xFFFFFF;
          for (int i = er[k] + 1; i < R; i++) {
            int th;
            if (res(i)) {
              const int s = i & (RW - 1);
              if (thvL[s] != verL[s]) continue;  // not decided (or thresholds stale: never here)
              th = thL[s][cx];
            } else {
              if (ld(&t.thv[d.ro + i]) != ld(&t.ver[d.ro + i])) continue;
              th = ld(&t.th[row(i) + cx]);
            }
            if (th != -2 && px <= th) {
              found = i;
              break;
            }
          }
        }
        ef[k] = found;
        const int nr = __popcll(ballot(found >= 0)), nkp = __popcll(ballot(on && found < 0));
        if (lane == 0) {
          cntR[k * NWV + wv] = nr;
          cntK[k * NWV + wv] = nkp;
        }
      }
      __syncthreads();
      int preR[CPW], preK[CPW], totR = 0, totK = 0;
#pragma unroll
      for (int k = 0; k < CPW; k++) preR[k] = preK[k] = 0;
      for (int q = 0; q < NCH; q++) {
#pragma unroll
        for (int k = 0; k < CPW; k++)
          if (q == k * NWV + wv) {
            preR[k] = totR;
            preK[k] = totK;
          }
        totR += cntR[q];
        totK += cntK[q];
      }
      // pass 2: medians and keys of the received entries, the kept ones compacted
#pragma unroll
      for (int k = 0; k < CPW; k++) {
        const int e = sb + (k * NWV + wv) * 64 + lane;
        const bool on = e < nU;
        const int found = ef[k];
        const int cx = ecp[k] >> 24, px = ecp[k] & 0xFFFFFF;
        const uint64_t rec = ballot(found >= 0), keep = ballot(on && found < 0);
        if (found >= 0) {
          // MedianTimestamp over OldestSelfAncestorToSee(w, x) of the famous witnesses w
          // that see x (hashgraph.go:704-709, 762-770), the upper median.  w = (d, i_w)
          // sees x iff FD[x][d] <= i_w, and FD[x][d] is then OldestSelfAncestorToSee
          const int64_t cpos = (int64_t)cx * cc + px;
          const int x = chg[cpos];
          const uint64_t s0 = t.Sch[(int64_t)g * N * cc + cpos];
          tx += t.ntxch[(int64_t)g * N * cc + cpos];
          uint64_t fm;
          if (res(found)) {
            fm = fmL[found & (RW - 1)];
          } else {
            fm = 0;
            for (int dd = 0; dd < N; dd++) {
              const int w = t.W[row(found) + dd];
              if (w >= 0 && w < n_c && ld(&t.fame[row(found) + dd]) == 1) fm |= 1ull << dd;
            }
          }
          // the timestamps as int32 offsets from x's own (a register sort of 32-bit
          // values); an offset outside int32 takes the exact 64-bit count below
          const int64_t tsx = tschg[cpos];
          int32_t vals[NM];
          int m = 0;
          bool ovf = false;
#pragma unroll
          for (int dd = 0; dd < NM; dd++) {
            const int q = dd < N && ((fm >> dd) & 1) ? FDg[cpos * N + dd] : INF;
            vals[dd] = INT32_MAX;  // fillers sort last (a real INT32_MAX ties with them)
            if (q != INF && q <= WIX_(found, dd)) {
              const int64_t o = tschg[(int64_t)dd * cc + q] - tsx;
              ovf = ovf || o < -(int64_t)INT32_MAX || o > (int64_t)INT32_MAX;
              vals[dd] = (int32_t)o;
              m++;
            }
          }
          const int want = m / 2;  // the upper median
          int64_t med = 0;
          if (!ovf) {
            sort_regs32<NM>(vals);
#pragma unroll
            for (int a = 0; a < NM; a++)
              if (a == want) med = tsx + vals[a];
          } else {
            // the value whose rank among the m timestamps covers `want`
            auto tv = [&](int dd, int64_t& v) -> bool {
              if (!((fm >> dd) & 1)) return false;
              const int q = FDg[cpos * N + dd];
              if (q == INF || q > WIX_(found, dd)) return false;
              v = tschg[(int64_t)dd * cc + q];
              return true;
            };
            for (int a = 0; a < N; a++) {
              int64_t va;
              if (!tv(a, va)) continue;
              int lt = 0, eq = 0;
              for (int b = 0; b < N; b++) {
                int64_t vb;
                if (!tv(b, vb)) continue;
                lt += vb < va;
                eq += vb == va;
              }
              if (lt <= want && want < lt + eq) {
                med = va;
                break;
              }
            }
          }
          t.rr[eo + x] = found;
          t.cts[eo + x] = med;
          t.xcc[eo + x] = c;
          const int p = nb + preR[k] + __popcll(rec & below);
          if (p < KB && lds_keys) {
            kri[p] = (uint32_t)found << 16 | (uint32_t)x;
            kc[p] = med;
            ks[p] = s0;
          } else {
            const int64_t so = 2 * eo + nord + p;
            st(&t.krr[so], found);
            st(&t.kct[so], med);
            st(&t.ks0[so], s0);
            st(&t.kid[so], x);
          }
        }
        if (on && found < 0) {
          const int p = nk + preK[k] + __popcll(keep & below);
          uput(Ur_s, Urg, p, er[k]);
          uput(Ucp_s, Ucpg, p, ecp[k]);
          kmin = min(kmin, er[k]);
        }
      }
      nb += totR;
      nk += totK;
      __threadfence_block();
      __syncthreads();  // cntR / cntK are the next span's; its entries lie past every write above
    }
    nU = nk;
    {
      const int km = wave_min(kmin);
      const int64_t tw = wave_sum64(tx);
      if (lane == 0) {
        wred[2][wv] = km;
        wtx[wv] = tw;
      }
    }
    __syncthreads();
    {
      int km = INF;
      for (int w = 0; w < NWV; w++) {
        km = min(km, wred[2][w]);
        ctx += wtx[w];
      }
      if (scan) umin = min(thchg ? INF : umin0, km);
    }
    HGB_STAMP(3)
    // ---- FindOrder (hashgraph.go:723-760): sort the batch, append it ----
    if (nb > 0) {
      if (nb <= KB && lds_keys) {
        sort_keys_lds(t, eo, nb, kri, kc, ks);
        __syncthreads();
        for (int p = tid; p < nb; p += NT) t.order[eo + nord + p] = (int32_t)(kri[p] & 0xFFFFu);
        if (DLV)  // the commit records beside the ids
          for (int p = tid; p < nb; p += NT) {
            t.ord_rr[eo + nord + p] = (int32_t)(kri[p] >> 16);
            t.ord_cts[eo + nord + p] = kc[p];
          }
      } else {
        // past KB keys: the same network on the graph's global scratch (2E entries
        // from 2 eo: nord + the padded size stays below 2E); the first KB keys are in LDS
        const int64_t so = 2 * eo + nord;
        if (lds_keys)
          for (int p = tid; p < KB; p += NT) {
            st(&t.krr[so + p], (int32_t)(kri[p] >> 16));
            st(&t.kct[so + p], kc[p]);
            st(&t.ks0[so + p], ks[p]);
            st(&t.kid[so + p], (int32_t)(kri[p] & 0xFFFFu));
          }
        __threadfence_block();
        __syncthreads();
        sort_keys_g(t, eo, nb, t.krr + so, t.kct + so, t.ks0 + so, t.kid + so);
        __syncthreads();
        for (int p = tid; p < nb; p += NT) t.order[eo + nord + p] = ld(&t.kid[so + p]);
        if (DLV)
          for (int p = tid; p < nb; p += NT) {
            t.ord_rr[eo + nord + p] = ld(&t.krr[so + p]);
            t.ord_cts[eo + nord + p] = ld(&t.kct[so + p]);
          }
      }
    }
    if (tid == 0) t.counts[d.co + c] = nb;
    nord += nb;
    __syncthreads();  // kri and the window state are the next call's
    HGB_STAMP(4)
  }
#undef HGB_STAMP
  if (t.dbg && tid == 0)
    for (int i = 0; i < 5; i++) t.dbg[(int64_t)g * 8 + i] = cyc[i];
  // the undetermined list for the host
  for (int i = tid; i < nU; i += NT) {
    const int cp = uget(Ucp_s, Ucpg, i);
    t.U[eo + i] = chg[(int64_t)(cp >> 24) * cc + (cp & 0xFFFFFF)];
  }
  if (tid == 0) {
    int64_t* s = t.scal + (int64_t)g * 8;
    s[0] = R;
    s[1] = lcr;
    s[2] = lcre;
    s[3] = ctx;
    s[4] = nord;
    s[5] = nU;
  }
}

#include "hge_batch_bulk.hip"
#include "hge_batch_gen.hip"
#include "hge_batch_stats.hip"

}  // namespace hgb

// host side: struct hge_batch and the C ABI
#include "hge_batch_host.hip"
