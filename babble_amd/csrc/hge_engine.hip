// hge_engine.hip — host side of the MI355X hashgraph engine (C ABI in include/hge.h).
//
// Orchestrates the kernels of hge_kernels.hip over one HIP stream.  The host
// keeps only control state: the FromParentsLatest admission check (O(1) per
// event over per-creator chain tails, hashgraph.go:366-396), the consensus log
// and a handful of scalars (Rounds(), LastConsensusRound, ...).  Every table
// the ordering path reads lives in HBM.
//
// A "batch" is the unit of device work: it absorbs the events inserted since
// the previous batch and replays a list of RunConsensus calls (each at an
// event count n_c).  The online API runs one call per batch; hge_replay runs a
// whole schedule in one batch.  Both produce identical results (tests).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/hge.h"
#include "hge_hip.h"
#include "hge_plan.h"
#include "hge_hostlog.h"
#include "hge_hooks.h"
#include "hge_launch.h"
#include "hge_xfer.h"
#include "hge_kernels.hip"
#include "hge_median_rows.hip"
#include "hge_wide32.hip"
#include "hge_coords.hip"
#include "hge_coords_win.hip"
#include "hge_rounds_coop.hip"
#include "hge_rounds_direct.hip"
#include "hge_walk_spec.hip"
#include "hge_commit.hip"

using namespace hge;

namespace {

inline int div_up(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static const int32_t kInf = INF32;

}  // namespace

struct hge_engine {
  // ==== State, grouped by lifetime (DESIGN.md §State and lifetimes) ====================
  // Every data member is declared in this block, in the part whose reset it follows.
  // Resetting a part is assigning a fresh one, so a new member needs nothing else.

  // ---- what the parts hold: a pending coordinate step, a split plan ----
  // coords_a (the control block, lastAncestors, firstDescendants) then coords_b (the
  // rounds frontier and what follows).  What their stages share is a CoordStep: coords_a
  // makes it, coords_b (or online_fast) takes it, and in between the step is pending
  // (cons.cstep has a value): the cross-GPU split (hge_split_*) runs a walker there.
  struct CoordStep {
    bool fresh = false;      // nothing had coordinates or rounds before
    int64_t n0 = 0, n1 = 0;  // the new ids
    int maxnew = 0;          // most new positions on one chain, + 1
    int tot0 = 0;            // a fresh walk's fss rows (every chain's length)
    int SEG = 0, nseg = 0;   // the sweeps' segment length and count
    int maxlen = 0, minlen = 0;  // the longest and the shortest chain
    enum class La { Windows, Seq, Sweeps } la = La::Sweeps;  // how lastAncestors are computed
    // the control block's regions in s_kctl (bind_kctl)
    int32_t *rstate = nullptr, *olen = nullptr, *len = nullptr, *plo = nullptr, *qlo = nullptr;
    int32_t *fss_lo = nullptr, *fss_off = nullptr, *fss_total = nullptr, *segbase = nullptr;
    const int2* segs = nullptr;
    int32_t *cand_lo = nullptr, *cand_hi = nullptr;  // a split part's candidates (else null)
    int32_t* risky1 = nullptr;  // the one-window lastAncestors pass's risky id (-1 as uploaded)
    const UpEv* up = nullptr;   // the chain-table fill's source: the packed upload, or null (the tables)
    UpDst up_dst{};
    // what earlier kernels of the step did already
    bool frontier_started = false;  // k_frontier_start's block (k_chain_fill_qlo, k_la_seq)
    bool qlo_done = false;          // k_fd_qlo's blocks (the same two)
    bool fd_done = false;           // the FD rows and FDT runs (k_la_seq, N <= 16)
    // the FD rows without their timestamp offsets (k_fd_rows16): a fresh bulk replay whose
    // median reads the rows itself (k_median_rows)
    bool fd_rows_only = false;
    bool take_frontier_start() { return std::exchange(frontier_started, false); }  // (a later attempt starts again)
  };
  // One hashgraph sharded across GPUs by time (hge_split_plan): part
  // p owns the events [a_p, a_{p+1}) and the calls [cb_p, cb_{p+1}).  Every part
  // computes the coordinates and walks the rounds recurrence (sequential: it cannot
  // be split exactly); part p then decides the fame of the rounds whose
  // first witness it owns and commits the events its calls receive (candidates from
  // cand_lo_p, the only FD timestamp rows it writes), and the parts exchange fame
  // decisions and ordered slices through the caller's all-gather (hge_split_exchange).
  struct SplitPlan {
    int part = 0, nparts = 0;
    std::vector<int64_t> a;     // event bounds, nparts + 1
    std::vector<int32_t> cb;    // call bounds, nparts + 1
    std::vector<int64_t> clo;   // first candidate of every part
  };

  // ---- engine lifetime: never reset ----
  int N = 0, NW = 1, SM = 1;
  int device = 0;
  // declared before every buffer and event, so destroyed after them
  Stream st;
  std::string err;
  HostPhases hp;
  Xfer xfer{st, hp};    // the pinned staging arena (hge_xfer.h)
  KernelProf prof{st};  // per-kernel HIP-event timing on the engine stream (hge_set_profiling)
  int64_t cache_size = 0;   // Store.CacheSize() for the rolling views (0 = unbounded)
  int32_t chain_limit0 = INT32_MAX;  // every stream's first chain limit (init)
  // the caller's all-gather of a split replay (hge_split_exchange)
  hge_exchange_fn x_fn = nullptr;
  void* x_ctx = nullptr;
  // measurement aid (hge_split_emulate): an unsplit replay records what every part
  // of a split contributes to the exchanges (the fame decisions of every fame
  // iteration, the order, per-call batches, round received / timestamps, the
  // undetermined list); a split part run without an exchange then takes the other
  // parts' slots from the record, so one GPU times each part of a G-way split alone.
  // Kept on purpose: only hge_split_emulate starts a record or drops one, so it outlives
  // the replays that use it; the caller records again after staging another stream.
  bool rec_on = false, rec_have = false;
  std::vector<std::vector<uint8_t>> rec_dec;
  std::vector<int32_t> rec_order, rec_rr, rec_left;
  std::vector<int64_t> rec_counts, rec_cts;
  // hooks read at create (hge_hooks.h)
  // test hook (HGE_TEST_W32_FAIL=k): to_wide32 fails once after its stage k.  Stages count
  // in the order to_wide32 runs them, not by bit value: 1 the int32 LA table allocated
  // (bit 4), 2 the runs widened (bit 1), 3 the FD rows widened (bit 2)
  int test_w32_fail = hge_hooks::test_w32_fail();
  // test hook (HGE_TEST_MEDIAN_ROWS_FALLBACK=1): the coordinate step skips the timestamps
  // but the median takes k_median_wave, so ensure_fdtd()'s full pass runs
  bool test_rows_fallback = hge_hooks::test_median_rows_fallback();
  bool dbg_on = hge_hooks::stamps();
  // launch geometry and residency, asked of the device once
  int ncu_cache = 0;
  int walk_chk[2] = {448, 2};        // checker threads, poll pause
  bool coop_checked = false;
  int coop_nb = 0, coop_ncu = 0, coop_spec_nb = -1, coop_spec_bs = 0;
  std::vector<std::pair<std::pair<const void*, int>, int>> resident_nb;  // launch_resident's blocks per CU
  bool frontier_fallback = false;  // k_round_step32 for good after a hand-off timeout
  int64_t n_frontier_fallbacks = 0;
  // These tag or address device memory that no reset clears (the walkers' epoch-tagged
  // histories, the two-slot path counters), so they keep counting across streams.
  uint32_t walk_epoch = 0, coop_epoch = 0;
  int walk_seq = 0, sort_seq = 0;
  bool sort_counted = false;  // the last order stage launched a counting kernel (hge_sort_paths)
  // what the last step did, for the readers of hge_coordinate_sweeps and hge_stage_times
  int n_sweeps = 0;
  float stage_ms[7] = {};
  Event ev[8];
  // host staging of the control blocks and the sweeps' segments (rebuilt by every step)
  std::vector<int32_t> h_cctl, h_kctl;
  std::vector<hge_plan::Seg> h_segs;
  // A replay delivers its order to host memory inside hge_replay_run: one DMA copy from
  // the results block into a pinned buffer sized at hge_replay_prepare (pin_ord), the
  // log's last cons.cons_pin_n ids.  Readers take it from there (hge_replay_order: a view,
  // hge_replay_fetch: one copy); the log's vector gets them on first use
  // (consensus_sync), outside the replay.
  PBuf<int32_t> pin_ord;
  int32_t* pin_ord_dev = nullptr;  // its device-side address (the sorts write there)

  // ---- device tables ----
  int64_t Ecap = 0;
  int ccap = 0, Rcap = 0;
  DBuf<int32_t> d_creator, d_index, d_sp, d_op, d_ntx, d_round, d_rr, d_und;
  DBuf<int64_t> d_ts, d_cts;
  DBuf<uint64_t> d_S;
  DBuf<uint8_t> d_coin, d_wit;
  DBuf<int32_t> d_chain, d_LA, d_FD, d_FSS;
  DBuf<uint32_t> d_LA16;  // N > 32: the sweeps' packed (LA + 1) table (hge_coords.hip)
  DBuf<int2> d_opcp;  // [N][ccap] other-parent coordinates (k_chain_fill)
  DBuf<int64_t> d_tsch;  // [N][ccap] timestamps in chain layout (k_chain_fill)
  DBuf<int32_t> d_C, d_W, d_rcnt, d_minw;
  DBuf<uint64_t> d_ssb, d_seeb;
  DBuf<uint8_t> d_fame;
  DBuf<int32_t> d_FDT;   // FD in run layout [N][N][ccap] (persistent)
  DBuf<int32_t> d_FDTD;  // N > 16: timestamp offsets at the FD positions (the wide median)
  DBuf<uint8_t> d_FDTW;  // N > 16: per (row, 64-column tile) out-of-range flags of d_FDTD
  DBuf<int32_t> d_WLA;   // N > 16: round frontier rows transposed (k_witness_la)
  DBuf<uint16_t> d_WLR;  // N > 64, packed path: the same rows row-major as LA + 1 (theta)
  DBuf<uint64_t> d_ssc;
  // ---- scratch ----
  DBuf<int32_t> s_w32, s_w32a;  // to_wide32 / rounds_step32 scratch
  DBuf<int32_t> s_small, s_newwit;
  DBuf<int32_t> s_LCR, s_clast;
  DBuf<uint8_t> s_dec, s_decbit;
  DBuf<int32_t> s_segcnt, s_segcall, s_seground, s_theta;
  DBuf<uint8_t> s_segdec;
  DBuf<uint64_t> s_segfws;
  DBuf<int32_t> s_recv, s_rr, s_fund, s_upos, s_und2, s_bpos, s_vis;
  DBuf<int64_t> s_cts;
  DBuf<unsigned char> s_keys, s_keys2;
  DBuf<int32_t> s_part, s_fst, s_relay, s_rfail;
  DBuf<uint8_t> s_dec2;  // selective fame widening: the new layout's decisions
  // coordinate sweeps: scratch
  DBuf<int32_t> s_chg, s_bar, s_dirty;
  DBuf<int32_t> s_src;  // hge_consensus_timestamp_sources: ids, then their sources
  // hge_commit_records: one chunk's consensus timestamps, then (as int32) its ids, rounds
  // received and sources; sized by the chunk, not by the log
  DBuf<int64_t> s_rec;
  // windowed lastAncestors (hge_coords_win.hip): chunk plans, row sums, starting rows
  DBuf<int4> s_lwplan;
  DBuf<uint32_t> s_lwsum, s_lwinit;
  DBuf<int32_t> s_lwpos, s_lwrisky;
  DBuf<int32_t> s_fdlo;     // [2N]: the first position to refresh per chain, then the chains' lengths
  DBuf<uint64_t> s_gran;
  DBuf<int32_t> s_bseg;
  DBuf<uint64_t> s_H;                // speculative walk: epoch-tagged histories
  DBuf<int32_t> s_hn, s_hres;        // rows written + progress hints, merge results
  DBuf<uint64_t> s_cH, s_cS, s_cT, s_cM;  // speculative wide walk: rows, ssc bits, tables, merges
  DBuf<uint32_t> s_mb;                    // direct rounds: staged member rows (two parity blocks)
  DBuf<int32_t> s_cn;
  // consensus control block (one upload) and results block (one readback)
  DBuf<int32_t> s_cctl, s_out;
  // the coordinate step's control block (hge_plan::CoordsCtl, bound in CoordStep)
  DBuf<int32_t> s_kctl;
  DBuf<uint64_t> s_dbg;   // diagnostic stamps (HGE_STAMPS=1)
  DBuf<uint64_t> s_wdbg;  // HGE_WALK_DEBUG: the walkers' cycle stamps
  // cross-GPU split: a walker's rows (hge_frontier_walk), the exchange of an emulated
  // part, every part's ordered ids and their offsets
  DBuf<int32_t> s_hist, s_hstate;
  DBuf<uint64_t> s_hssc;
  DBuf<uint8_t> s_xbuf;
  DBuf<int32_t> s_sord;
  DBuf<int64_t> s_soff;
  // The walk's select-path counters (hge_walk_select_paths): two slots of {narrow, exact},
  // cleared once.  Walk k adds to slot k & 1 and clears the other slot as it ends,
  // for the walk after it on the stream: no clearing launch per walk (an online call is a
  // few hundred microseconds, a memset node was ~10 of them).
  DBuf<unsigned long long> s_wpaths;
  // The order stage's sort-path counters (hge_sort_paths): two slots of {packed, index,
  // k_bucket_sort_big's next bucket, unused}, handed over like the walk's.  An order stage
  // without a bucket past 512 keys launches no counting kernel and reports (0, 0).
  DBuf<unsigned long long> s_spaths;

  // ---- stream lifetime: fresh at hge_reset and hge_replay_prepare (reset_state) ----
  struct StreamState {
    // the accepted events and the admission state; log.chain_limit is the longest chain
    // of the uint16 wide path (then: to_wide32)
    HostLog log;
    int64_t n_dev = 0;  // uploaded
    // a packed upload of the events [up_n0, up_n1) waiting for k_chain_fill (upload())
    std::vector<UpEv> h_up;  // the packed records, uploaded with coords_a's control block
    int64_t up_n0 = -1, up_n1 = -1;
    // N > 32 past chain_limit: int32 positions for good (hge_wide32.hip); pending until
    // the next coordinate step converts the packed table.  A new stream starts packed.
    bool wide32 = false, wide32_pending = false;
    // to_wide32's progress bits: 1 the runs widened, 2 the FD rows, 4 the int32 LA table allocated
    int w32_done = 0;
    // what failed, when an internal failure left the host and device state apart (empty:
    // none): every later consensus call refuses (HGE_ERR_INTERNAL) until a new stream
    std::string failed;
    int R_set = 0;  // rounds recorded by hge_set_round (Store.SetRound)
    std::vector<int64_t> replay_calls;  // n_c per call (accepted counts)
    // a plan belongs to the stream it was made for (it is checked against replay_calls)
    SplitPlan sp;
    bool sp_active = false;  // during hge_split_run
    // hge_replay_run: this replay's coordinate step may skip the timestamps.  Set around
    // replay_begin, which assigns the consensus part: so it lives here.
    bool rows_bulk = false;
    StreamState() = default;
    StreamState(int n, int32_t chain_limit) : log(n, chain_limit) {}
  } strm;

  // ---- consensus lifetime: fresh at the two above and at every replay (replay_begin) ----
  struct ConsensusState {
    int64_t n_coords = 0;     // coordinates + rounds computed
    int64_t n_divided = 0;    // visible to DecideFame / FindOrder (DivideRounds)
    std::vector<int32_t> coords_len;  // chain lengths at n_coords
    int R = 0;                // Store.Rounds()
    int R_div = 0;            // Rounds() as seen by the consensus calls (DivideRounds)
    std::vector<int32_t> h_minw;  // first witness id per round (read back by coords)
    bool minw_full = true;   // d_minw's rows are stale: the next rounds tail recomputes all
    int lcr = -1;             // LastConsensusRound (-1 nil)
    int lcre = 0;             // LastCommitedRoundEvents
    int64_t ctx = 0;          // ConsensusTransactions
    std::vector<int32_t> consensus;  // the consensus log (unbounded)
    int64_t cons_pin_n = 0;   // ... and its tail still in the pinned order buffer (pin_ord)
    bool lazy_order = false;  // during a replay's batch: the order goes to pin_ord
    int64_t n_und = 0;
    bool und_fresh = false;  // the candidate list is every event of a fresh replay
    // the candidates' lowest round, read back with the round count (coords_b) for the
    // undetermined list of n_und = key[0] + key[2] - key[1] events after the divide
    // that raises n_divided from key[1] to key[2] (key[0] < 0: none)
    int32_t mnr_pre = 0;
    int64_t mnr_key[3] = {-1, 0, 0};
    std::optional<CoordStep> cstep;  // the pending coordinate step
    bool dividing = false, und_appended = false;  // DivideRounds in progress (divide)
    // cross-GPU split: the joined frontier rows of the walkers (hge_split_finish)
    bool ext_on = false, ext_natural = false;
    int ext_rows = 0;
    std::vector<int32_t> ext_C;
    std::vector<uint64_t> ext_ssc;
    // A fresh bulk replay at uint16 positions writes the FD rows alone (k_fd_rows16) and
    // takes its median from them (k_median_rows): d_FDTD / d_FDTW then hold no row of the
    // current coordinates (fdtd_stale) until k_fd_transpose_ts has run over the positions a
    // reader needs.  Every reader of the two tables calls ensure_fdtd() first; the replay
    // itself ends with that pass over the still-undetermined events' rows (fdtd_tail).
    bool fdtd_stale = false;
    int fdtd_maxlen = 0;      // the longest chain of the stale coordinates
    std::vector<int64_t> replay_counts;  // the last replay's per-call batches
    int x_iter = 0;  // fame iteration of the current batch (the emulation record's index)
    bool vis_all = false;  // this batch: one call seeing every event (no visibility table)
    std::chrono::steady_clock::time_point w_start;  // the replay's start (hge_stage_times)
    // the consensus control block's regions in s_cctl (bind_ctl, every batch)
    int64_t* c_nc = nullptr;
    int32_t *c_Rc = nullptr, *c_Lc = nullptr, *c_flags = nullptr, *c_pr = nullptr, *c_pidx = nullptr;
    int32_t* c_sgo = nullptr;
    const int32_t* segoff_p = nullptr;  // segment offsets used by k_round_received
    ConsensusState() = default;
    explicit ConsensusState(int n) : coords_len(n, 0) {}
  } cons;

  // ==== end of state: member functions only from here on (and the step structs) ====

  int64_t consensus_size() const { return (int64_t)cons.consensus.size() + cons.cons_pin_n; }
  void consensus_sync() {
    if (!cons.cons_pin_n) return;
    cons.consensus.insert(cons.consensus.end(), pin_ord.p, pin_ord.p + cons.cons_pin_n);
    cons.cons_pin_n = 0;
  }
  void ensure_pin_ord(size_t n) {
    if (n <= pin_ord.n && pin_ord.p) return;
    consensus_sync();
    pin_ord_dev = nullptr;
    pin_ord.need(std::max<size_t>(n, 1));
    pin_ord_dev = PinnedMem::device_ptr(pin_ord.p);
  }
  int n_cu() {
    if (!ncu_cache) HGE_HIPCHK(hipDeviceGetAttribute(&ncu_cache, hipDeviceAttributeMultiprocessorCount, device));
    return ncu_cache;
  }
  const void* coop_spec_fn() const {
    return coop_spec_bs == 1024 ? (const void*)k_rounds_coop_spec<1024> : (const void*)k_rounds_coop_spec<512>;
  }

  Tables tables() const {
    Tables t;
    t.N = N;
    t.NW = NW;
    t.SM = SM;
    t.ccap = ccap;
    t.Rcap = Rcap;
    t.creator = d_creator.p;
    t.index = d_index.p;
    t.sp = d_sp.p;
    t.op = d_op.p;
    t.ts = d_ts.p;
    t.S = d_S.p;
    t.coin = d_coin.p;
    t.ntx = d_ntx.p;
    t.chain = d_chain.p;
    t.opcp = d_opcp.p;
    t.tsch = d_tsch.p;
    t.LA = d_LA.p;
    t.NW2 = (N + 1) / 2;
    t.LA16 = sweep16() ? d_LA16.p : nullptr;  // null: int32 rows (la_row)
    t.FD = fdt16() ? nullptr : d_FD.p;
    t.FD16 = fdt16() ? (uint16_t*)d_FD.p : nullptr;
    t.FDTD = d_FDTD.p;
    t.FDTW = d_FDTW.p;
    t.WLA = wla16() ? nullptr : d_WLA.p;
    t.WLA16 = wla16() ? (uint16_t*)d_WLA.p : nullptr;
    t.WLR = (N > 64 && !strm.wide32) ? d_WLR.p : nullptr;
    t.round = d_round.p;
    t.wit = d_wit.p;
    t.C = d_C.p;
    t.W = d_W.p;
    t.ssb = d_ssb.p;
    t.seeb = d_seeb.p;
    t.fame = d_fame.p;
    t.rcnt = d_rcnt.p;
    return t;
  }

  // ------------------------------------------------------------------------
  void init(int n, int64_t cap, int dev) {
    N = n;
    NW = (N + 63) / 64;
    SM = 2 * N / 3 + 1;  // hashgraph.go:78-80
    device = dev;
    HGE_HIPCHK(hipSetDevice(device));
    st.create();
    for (auto& e : ev) e.create();
    // the wide kernels keep chain positions as uint16 (LA16, the rounds walk, theta):
    // a longer chain switches the engine to int32 positions (to_wide32).
    // HGE_CHAIN_LIMIT (tests) lowers the switch point.
    chain_limit0 = hge_hooks::chain_limit(N > 32 ? 0xFFFE : INT32_MAX);
    strm = StreamState(N, chain_limit0);
    cons = ConsensusState(N);
    // chain tables: a creator's chain is ~cap/N long (binomial, sd ~ sqrt(cap/N));
    // rounds: a round spans >= ~4N events in gossip.  Both grow on demand.
    const int64_t c0 = std::max<int64_t>(cap, 1024);
    ensure_events(c0);
    ensure_ccap(c0 / N + c0 / (8 * N) + 64);
    ensure_rcap(c0 / (2 * N) + 64);
    s_small.need(16);
  }


  // diagnostic stamps (HGE_STAMPS=1): per-section cycle counters of some kernels
  uint64_t* dbg_p() {
    if (!dbg_on) return nullptr;
    if (!s_dbg.p) {
      s_dbg.need(16);
      HGE_HIPCHK(hipMemsetAsync(s_dbg.p, 0, 16 * 8, st));
    }
    return s_dbg.p;
  }
  void dbg_dump() {
    if (!dbg_on || !s_dbg.p) return;
    uint64_t v[16];
    readback(v, s_dbg.p, 16);
    fprintf(stderr, "[hge stamps]");
    for (int i = 0; i < 16; i++) fprintf(stderr, " %llu", (unsigned long long)v[i]);
    fprintf(stderr, "\n");
  }

  // only what must come before the members die: the stream drained (then the buffers and
  // events free themselves, the stream last) and the HGE_HOST_PHASES line
  ~hge_engine() {
    if (st) (void)hipStreamSynchronize(st);
    if (hge_hooks::host_phases() && hp.calls) {
      const double c = (double)hp.calls;
      fprintf(stderr,
              "{\"hge_host_phases\": {\"calls\": %lld, \"launches_per_call\": %.2f, \"copies_per_call\": %.2f, "
              "\"insert_us\": %.2f, \"consensus_us\": %.2f, \"sync_wait_us\": %.2f}}\n",
              (long long)hp.calls, hp.launches / c, hp.copies / c, hp.insert_ns / c / 1e3, hp.call_ns / c / 1e3,
              hp.wait_ns / c / 1e3);
    }
  }

  void ensure_events(int64_t m) {
    if (m <= Ecap) return;
    int64_t cap = std::max<int64_t>(m, Ecap + Ecap / 2);
    d_creator.grow_keep(cap, strm.n_dev, st);
    d_index.grow_keep(cap, strm.n_dev, st);
    d_sp.grow_keep(cap, strm.n_dev, st);
    d_op.grow_keep(cap, strm.n_dev, st);
    d_ntx.grow_keep(cap, strm.n_dev, st);
    d_ts.grow_keep(cap, strm.n_dev, st);
    d_S.grow_keep(4 * cap, 4 * strm.n_dev, st);
    d_coin.grow_keep(cap, strm.n_dev, st);
    d_round.grow_keep(cap, cons.n_coords, st);
    d_wit.grow_keep(cap, cons.n_coords, st);
    d_rr.grow_keep(cap, cons.n_coords, st, 0xFF);
    d_cts.grow_keep(cap, cons.n_coords, st, 0);
    d_und.grow_keep(cap, cons.n_und, st);
    Ecap = cap;
  }

  // The chain tables hold ccap positions per row: grown to nc positions one table at a
  // time (the peak is one table twice), each row copied to the head of its longer row
  // (hge::Buf::regrow_rows).  Every call states its table's geometry: rows, bytes per
  // position of a row, total bytes, the resulting n.  A failure between two tables leaves
  // them at different row pitches while ccap is unchanged.
  void ensure_ccap(int64_t m) {
    if (m <= ccap) return;
    // a multiple of 64 positions: the uint16 run table's rows stay 8-byte aligned
    const int64_t nc = (std::max<int64_t>(m, (int64_t)ccap + ccap / 2) + 63) & ~(int64_t)63;
    const size_t n = N, oc = ccap, c = nc;
    auto regrow = [&](auto& b, size_t rows, size_t pos_bytes, size_t total_bytes, size_t n_after, int fill = -1) {
      b.regrow_rows(rows, pos_bytes * oc, pos_bytes * c, total_bytes, n_after, ccap > 0, st, fill);
      sync();  // a table regrown is a host wait (hge_host_syncs); queued downloads land
    };
    regrow(d_chain, n, sizeof(int32_t), sizeof(int32_t) * n * c, n * c, 0xFF);
    regrow(d_opcp, n, sizeof(int2), sizeof(int2) * n * c, n * c);
    regrow(d_tsch, n, sizeof(int64_t), sizeof(int64_t) * n * c, n * c);
    // row-major [N][ccap][N]: a chain's block is one row
    if (!sweep16()) regrow(d_LA, n, sizeof(int32_t) * n, sizeof(int32_t) * n * c * n, n * c * n);
    if (N > 32) {  // (kept across a switch to int32: a later stream starts packed again)
      const size_t w = (n + 1) / 2;
      regrow(d_LA16, n, sizeof(uint32_t) * w, sizeof(uint32_t) * n * c * w, n * c * w);
    }
    if (fdt16())  // uint16 FD rows: a chain's block is ccap * N halves
      regrow(d_FD, n, sizeof(uint16_t) * n, sizeof(uint16_t) * n * c * n, n * c * n / 2);
    else
      regrow(d_FD, n, sizeof(int32_t) * n, sizeof(int32_t) * n * c * n, n * c * n);
    if (N > 16) {  // FD timestamp rows below a batch's qlo are kept
      regrow(d_FDTD, n, sizeof(int32_t) * n, sizeof(int32_t) * n * c * n, n * c * n);
      const size_t NT = (n + 63) / 64;
      regrow(d_FDTW, n, NT, n * c * NT, n * c * NT);
    }
    // first-strong-seer rows (N <= 32): int32 rows of N, or uint16 rows padded to
    // 16/32 columns for the LDS walk; rebuilt from the frontier on, never kept
    if (N <= 32) d_FSS.need(n * c * std::max(N, 16));
    // persistent: FD in run layout [N][N][ccap]; uint16 runs are rows of ccap halves (the
    // buffer keeps int32 capacity)
    regrow(d_FDT, n * n, fdt16() ? sizeof(uint16_t) : sizeof(int32_t), sizeof(int32_t) * n * c * n, n * c * n);
    ccap = (int)nc;
  }

  void ensure_rcap(int64_t m) {
    if (m <= Rcap) return;
    int64_t nr = std::max<int64_t>(m, (int64_t)Rcap + Rcap / 2);
    const size_t oldn = (size_t)Rcap * N;
    d_C.grow_keep(nr * N, oldn, st, 0x7F);  // 0x7F7F7F7F is not INF32: fixed below
    d_W.grow_keep(nr * N, oldn, st, 0xFF);
    d_ssb.grow_keep(nr * N * NW, oldn * NW, st, 0);
    d_seeb.grow_keep(nr * N * NW, oldn * NW, st, 0);
    if (N > 32) d_ssc.grow_keep(nr * N * NW, oldn * NW, st, 0);
    d_fame.grow_keep(nr * N, oldn, st, 0);
    d_rcnt.grow_keep(nr, Rcap, st, 0);
    // + round count, overflow flag, lowest candidate round, hand-off error and up to 16
    // partial lowest rounds (k_round_minw)
    d_minw.need(nr + 20);
    cons.minw_full = true;  // (need() does not keep the rows' first witnesses)
    // C must be INF32 beyond the old rows
    fill_i32(d_C.p + oldn, (int64_t)(nr - Rcap) * N, INF32);
    sync();
    Rcap = (int)nr;
  }

  // a new stream (hge_reset, hge_replay_prepare): fresh stream and consensus parts, and
  // the device tables a stream starts from
  void reset_state() {
    sync();
    strm = StreamState(N, chain_limit0);
    cons = ConsensusState(N);
    reset_rounds();
    HGE_HIPCHK(hipMemsetAsync(d_chain.p, 0xFF, (size_t)N * ccap * 4, st));
    sync();
  }


  // fresh per-round tables (C, W, bitsets, fame, counts) and received rounds: one launch
  void reset_rounds() {
    const int64_t nrow = (int64_t)Rcap * N, nbits = nrow * NW;
    const int64_t most = std::max<int64_t>(std::max(nbits, Ecap), Rcap);
    KLAUNCH(k_reset_rounds, dim3(std::min(div_up(most, 256), 4096)), dim3(256), 0, st, tables(), nrow,
            nbits, Ecap, d_rr.p);
  }

  // ---------------- admission (hashgraph.go:366-396, hge_hostlog.h) ----------------
  // The log checks the event; the one device question is the engine's: a chain at the
  // limit of the uint16 positions goes on in int32 if the int32 table fits.
  int admit(const hge_event& e, int32_t sp, int32_t op) {
    HostLog& log = strm.log;
    const int r = log.admit(e, sp, op, err);
    if (r != HostLog::kAtLimit) return r;
    if (!(N > 32 && N <= 256 && !strm.wide32)) return log.capacity_error(err);
    // past the uint16 positions: int32 from here on
    // the int32 LA table must fit beside what is allocated: else refuse
    // the event here (the stream stops, as at any rejection) rather than lift
    // the cap and fail at the next coordinate step
    // to_wide32's peak: the int32 LA table, plus (uint16 runs and FD rows) one
    // int32 table being widened while the other's old copy is still held
    size_t free_b = 0, total_b = 0;
    const size_t tab = sizeof(int32_t) * (size_t)N * N * (size_t)std::max(ccap, log.chain_len[e.creator] + 2);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < (fdt16() ? 2 : 1) * tab + (64u << 20)) {
      err = "Chain capacity exceeded: the int32 position tables past 65,534 events per creator do not fit";
      return HGE_ERR_CAPACITY;
    }
    strm.wide32_pending = true;
    log.chain_limit = INT32_MAX;
    return HGE_OK;
  }


  void upload() {
    if (strm.n_dev == strm.log.n_events) return;
    ensure_events(strm.log.n_events);
    ensure_ccap(strm.log.max_chain() + 1);
    const int64_t a = strm.n_dev, m = strm.log.n_events - strm.n_dev;
    if (m <= 16384 && a == cons.n_coords) {
      // a small batch (an online call): one packed record per event through the
      // pinned arena, unpacked by the coordinate step's k_chain_fill (eight copies
      // from pageable memory were ~25 us of an online call)
      if (strm.up_n0 >= 0) throw Error(HGE_ERR_INTERNAL, "packed upload pending twice");
      // (they travel with the coordinate step's control block: one copy for both)
      strm.h_up = strm.log.pack(a, m);
      strm.up_n0 = a;
      strm.up_n1 = strm.log.n_events;
      strm.n_dev = strm.log.n_events;
      return;
    }
    HGE_HIPCHK(hipMemcpyAsync(d_creator.p + a, strm.log.h_creator.data() + a, 4 * m, hipMemcpyHostToDevice, st));
    HGE_HIPCHK(hipMemcpyAsync(d_index.p + a, strm.log.h_index.data() + a, 4 * m, hipMemcpyHostToDevice, st));
    HGE_HIPCHK(hipMemcpyAsync(d_sp.p + a, strm.log.h_sp.data() + a, 4 * m, hipMemcpyHostToDevice, st));
    HGE_HIPCHK(hipMemcpyAsync(d_op.p + a, strm.log.h_op.data() + a, 4 * m, hipMemcpyHostToDevice, st));
    HGE_HIPCHK(hipMemcpyAsync(d_ntx.p + a, strm.log.h_ntx.data() + a, 4 * m, hipMemcpyHostToDevice, st));
    HGE_HIPCHK(hipMemcpyAsync(d_ts.p + a, strm.log.h_ts.data() + a, 8 * m, hipMemcpyHostToDevice, st));
    HGE_HIPCHK(hipMemcpyAsync(d_S.p + 4 * a, strm.log.h_S.data() + 4 * a, 32 * m, hipMemcpyHostToDevice, st));
    HGE_HIPCHK(hipMemcpyAsync(d_coin.p + a, strm.log.h_coin.data() + a, m, hipMemcpyHostToDevice, st));
    strm.n_dev = strm.log.n_events;
  }

  void fill_iota(int32_t* p, int64_t n, int32_t base) {
    if (n > 0) KLAUNCH(k_iota, dim3(div_up(n, 256)), dim3(256), 0, st, p, n, base);
  }

  void fill_i32(int32_t* p, int64_t n, int32_t v) {
    if (n > 0) KLAUNCH(k_fill_i32, dim3(div_up(n, 256)), dim3(256), 0, st, p, n, v);
  }

  // ---- host <-> device staging through the pinned arena (hge_xfer.h) ----
  // (forwarders: some eighty call sites, here and in the C ABI, name these)
  void h2d(void* dev, const void* host, size_t bytes) { xfer.h2d(dev, host, bytes); }
  void d2h(void* host, const void* dev, size_t bytes) { xfer.d2h(host, dev, bytes); }
  size_t d2h_pinned(const void* dev, size_t bytes) { return xfer.d2h_pinned(dev, bytes); }
  void sync() { xfer.sync(); }
  template <typename F>
  void readback(F* host, const F* dev, size_t n) {
    xfer.readback(host, dev, n);
  }


  // ---------------- coordinates + rounds for [n_coords, n_events) ----------------
  // coords_a (the control block, lastAncestors, firstDescendants) then coords_b (the
  // rounds frontier and what follows).  What their stages share is a CoordStep: coords_a
  // makes it, coords_b (or online_fast) takes it, and in between the step is pending
  // (cstep has a value): the cross-GPU split (hge_split_*) runs a walker there.
  // what one attempt's rounds walk did besides walking
  struct Walk {
    bool assigned = false;   // the new events' rounds (k_round_assign's work)
    bool tail_done = false;  // ... and k_round_tail's work
    const int32_t* err_src = nullptr;  // a wide walk's hand-off error flag (it comes back with the rounds tail)
    bool host_err = false;             // ... or the host saw the error already
  };
  void bind_kctl(CoordStep& s, const hge_plan::CoordsCtl& L) const {
    int32_t* p = s_kctl.p;
    s.rstate = p + L.rstate, s.olen = p + L.olen(), s.len = p + L.nlen();
    s.plo = p + L.plo, s.qlo = p + L.qlo;
    s.fss_lo = p + L.fss_lo(), s.fss_off = p + L.fss_off(), s.fss_total = p + L.fss_total();
    s.segs = (const int2*)(p + L.segs), s.segbase = p + L.segbase;
    s.cand_lo = split_on() ? p + L.cand_lo() : nullptr;
    s.cand_hi = split_on() ? p + L.cand_hi() : nullptr;
    s.risky1 = p + L.risky;
    s.up = L.up_words ? (const UpEv*)(p + L.up) : nullptr;
  }
  bool split_on() const { return strm.sp_active && strm.sp.nparts > 1; }
  bool emulating() const { return split_on() && !x_fn && rec_have; }
  // a device buffer of nparts slots of `bytes` (the caller's memory: its collectives
  // write into it), then the all-gather: this part's slot is filled and the stream drained
  void* x_buf(int64_t bytes) {
    sync();  // the caller may hand out (or move) the memory of the previous exchange
    if (emulating()) {
      s_xbuf.need((size_t)bytes * strm.sp.nparts);
      return s_xbuf.p;
    }
    void* b = nullptr;
    if (!x_fn) throw Error(HGE_ERR_ARG, "split replay: no exchange (hge_split_exchange)");
    if (x_fn(x_ctx, 0, bytes, &b) != 0 || !b) throw Error(HGE_ERR_DEVICE, "split exchange: no buffer");
    return b;
  }
  void x_gather(int64_t bytes, void* b) {
    sync();
    if (emulating()) return;  // the caller fills the other parts' slots from the record
    if (x_fn(x_ctx, 1, bytes, &b) != 0) throw Error(HGE_ERR_DEVICE, "split exchange failed");
  }
  // fame rounds of part g: the pr_* indices [win_lo, win_hi) whose round's first witness
  // lies in the part's events (h_minw is ascending in the round)
  void split_rounds_of(int g, const std::vector<int32_t>& pr_round, int& win_lo, int& win_hi) const {
    const int nr = (int)pr_round.size();
    auto first_at = [&](int64_t ev) {
      int lo = 0, hi = nr;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)cons.h_minw[pr_round[mid]] < ev) lo = mid + 1;
        else hi = mid;
      }
      return lo;
    };
    win_lo = g == 0 ? 0 : first_at(strm.sp.a[g]);
    win_hi = g == strm.sp.nparts - 1 ? nr : first_at(strm.sp.a[g + 1]);
  }
  void coords() {
    if (coords_a()) coords_b();
  }
  // the wide kernels' tile width; the lanes per witness of the bitset kernels
  int npow() const { return N <= 64 ? 64 : N <= 128 ? 128 : 256; }
  int wit_group() const {
    int G = 1;
    while (G < std::min(N, 64)) G <<= 1;
    return G;
  }

  // the step's first half; leaves it pending (cstep); false: no new event
  bool coords_a() {
    cons.cstep.reset();
    upload();
    if (strm.wide32_pending) to_wide32();
    if (strm.log.n_events == cons.n_coords) return false;
    CoordStep s;
    plan_step(s);
    const Tables t = tables();
    chain_fill(t, s);
    last_ancestors(t, s);
    first_descendants(t, s);
    cons.cstep = s;
    return true;
  }
  // the control block (hge_plan::CoordsCtl), one upload
  void plan_step(CoordStep& s) {
    s.n0 = cons.n_coords;
    s.n1 = strm.log.n_events;
    // segment length: latency-bound sweeps (small N) like short segments, bandwidth-bound
    // ones (large N) long ones (fewer stale carries)
    s.SEG = N <= 32 ? 16 : 64;
    // only the fixed-point sweeps read the segment list: 156k segments and their sort
    // were ~3 ms of host time at the start of a 256/10M replay
    s.la = sweep16() && la_windows() ? CoordStep::La::Windows
           : la_seq_ok(s.n1 - s.n0)  ? CoordStep::La::Seq
                                     : CoordStep::La::Sweeps;
    const bool sweeps = s.la == CoordStep::La::Sweeps;
    h_segs.clear();
    if (sweeps) hge_plan::sweep_segments(h_segs, cons.coords_len, strm.log.chain_len, s.SEG);
    s.nseg = sweeps ? (int)h_segs.size() : 1;
    s.fresh = cons.R == 0;
    s.minlen = INT32_MAX;
    for (int c = 0; c < N; c++) {
      s.maxnew = std::max(s.maxnew, strm.log.chain_len[c] - cons.coords_len[c] + 1);
      s.fresh = s.fresh && cons.coords_len[c] == 0;
      s.maxlen = std::max(s.maxlen, strm.log.chain_len[c]);
      s.minlen = std::min(s.minlen, strm.log.chain_len[c]);
    }
    s.fd_rows_only = strm.rows_bulk && s.fresh && s.n0 == 0 && fdt16() && !split_on() && !rec_on && !cons.ext_on;
    std::vector<int32_t> cand;
    if (split_on()) {
      // FD timestamp rows (the median's input) of the ids [cand_lo, the part's end)
      const int64_t A = strm.sp.clo[strm.sp.part], B = strm.sp.a[strm.sp.part + 1];
      cand.resize(2 * (size_t)N);
      for (int c = 0; c < N; c++) {
        const std::vector<int32_t>& ch = strm.log.h_chain[c];
        cand[c] = (int)(std::lower_bound(ch.begin(), ch.end(), (int32_t)A) - ch.begin());
        cand[N + c] = (int)(std::lower_bound(ch.begin(), ch.end(), (int32_t)B) - ch.begin());
      }
    }
    // the packed event records (an online call's upload) ride in the same copy
    const bool packed = strm.up_n0 == s.n0 && strm.up_n1 == s.n1;
    if (packed && strm.h_up.empty()) throw Error(HGE_ERR_INTERNAL, "packed upload without records");
    static_assert(sizeof(UpEv) % 4 == 0, "records are whole words");
    static_assert(sizeof(hge_plan::Seg) == sizeof(int2), "the kernels read segments as int2");
    const hge_plan::CoordsCtl L =
        hge_plan::coords_ctl_layout(N, h_segs.size(), packed ? sizeof(UpEv) * strm.h_up.size() / 4 : 0);
    s.tot0 = hge_plan::fill_coords_ctl(h_kctl, L, cons.R, cons.coords_len, strm.log.chain_len, h_segs, s.SEG, cand);
    if (packed) memcpy(&h_kctl[L.up], strm.h_up.data(), sizeof(UpEv) * strm.h_up.size());
    s_kctl.need(h_kctl.size());
    h2d(s_kctl.p, h_kctl.data(), 4 * h_kctl.size());
    bind_kctl(s, L);
    s.up_dst = UpDst{d_creator.p, d_index.p, d_sp.p, d_op.p, d_ntx.p, d_ts.p, d_S.p, d_coin.p};
    strm.up_n0 = strm.up_n1 = -1;
    strm.h_up.clear();
  }
  // the chain table for the new ids, unless k_la_seq will fill it; past a fresh state
  // with k_fd_qlo's blocks and, for the wide rounds walk, k_frontier_start's
  void chain_fill(const Tables& t, CoordStep& s) {
    if (s.la == CoordStep::La::Seq) return;
    const int nfb = div_up((int)(s.n1 - s.n0), 256);
    if (!s.fresh && N <= 256) {
      const bool fst = N > 32 && !strm.wide32 && !frontier_fallback && !split_on() && !cons.ext_on;
      if (fst) {
        s_fst.need(N + 1);
        s_bar.need(2);
        s_gran.need(2 * (size_t)N);
      }
      KLAUNCH(k_chain_fill_qlo, dim3(nfb + N + (fst ? 1 : 0)), dim3(256), 0, st, t, (int)s.n0, (int)s.n1,
              s.up, s.up_dst, nfb, (const int32_t*)s.olen, (const int32_t*)s.len, s.qlo,
              fst ? s_fst.p : (int32_t*)nullptr, fst ? s_bar.p : (int32_t*)nullptr,
              fst ? (uint64_t*)s_gran.p : (uint64_t*)nullptr, 2 * N);
      s.frontier_started = fst;
      s.qlo_done = true;
    } else {
      KLAUNCH(k_chain_fill, dim3(nfb), dim3(256), 0, st, t, (int)s.n0, (int)s.n1, s.up, s.up_dst);
    }
  }
  // what a single-block rounds walk does after walking: the rounds of the new events
  // [n0, n1) (k_round_assign's work; und_appended: their ids appended to the
  // undetermined list) and, with `tail`, k_round_tail's work
  RoundAssign round_assign(const CoordStep& s, bool tail) {
    s_newwit.need(s.n1 - s.n0);
    RoundAssign ra{(int)s.n0, (int)s.n1, s_newwit.p, s.rstate + 2, cons.und_appended ? d_und.p + cons.n_und : (int32_t*)nullptr};
    if (tail) {
      ra.minw = d_minw.p;
      ra.G = wit_group();
      ra.und = d_und.p;
      ra.n_und = (int)cons.n_und;
      ra.lo = (int)cons.n_divided;
      ra.hi = (int)s.n1;
      ra.r_from = cons.minw_full ? 0 : -1;
      ra.rlo_dev = s_fst.p;
    }
    return ra;
  }
  // The step's second half: the rounds walk, the new events' rounds, the rounds tail,
  // then ONE round trip for the round count and minw.  The kernels stand down if the
  // rounds table overflowed or a wide walk's hand-off timed out: the loop mends that
  // and walks again.
  enum class RoundsOutcome { Done, Grow, HandoffTimeout };
  void coords_b() {
    CoordStep s = *cons.cstep;
    cons.cstep.reset();
    for (bool retry = false;; retry = true) {
      // the wide frontier grids stay on the device until the readback's sync: two such
      // grids on one device must not overlap (frontier_lock)
      std::unique_lock<std::mutex> flk;
      if (N > 32) flk = frontier_lock();
      const int32_t rs[3] = {cons.R, 0, 0};
      if (retry) h2d(s.rstate, rs, 12);
      const Walk w = walk_rounds(s);
      assign_rounds(s, w);
      const RoundsOutcome o = read_rounds(s, w, rounds_tail(s, w));
      if (o == RoundsOutcome::HandoffTimeout) {
        // the walk's workgroups were not all resident (another grid on the device, e.g.
        // one engine per rank on a shared GPU).  The engine walks again with
        // k_round_step32, one launch per round, which needs no co-residency, and keeps
        // that walk from here on.  Rows at and past the rounds this batch started from
        // are recomputed from scratch.
        frontier_fallback = true;
        n_frontier_fallbacks++;
        HGE_HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(d_C.p + (size_t)cons.R * N), INF32, (size_t)(Rcap - cons.R) * N, st));
      } else if (o == RoundsOutcome::Grow) {
        ensure_rcap((int64_t)Rcap * 2);
      } else {
        break;
      }
    }
    cons.n_coords = s.n1;
    cons.coords_len = strm.log.chain_len;
    prof.collect();
  }
  Walk walk_rounds(CoordStep& s) {
    if (N > 32 && (strm.wide32 || frontier_fallback)) return rounds_step32(s);
    if (N > 32) return rounds_coop(s);
    if (!s.fresh && s.maxlen < 0xFFFF) return walk_online(s);
    return walk_fss(s);
  }
  // The N <= 32 walks' kernels for rows of 16 or 32 columns, each under the name
  // KLAUNCH gives the instantiation (hge_kernel_stats keys on it)
  struct WalkKernels {
    int NPC;
    decltype(&k_fss<16>) fss;
    decltype(&k_rounds_walk<16, 4, 256>) walk;
    decltype(&k_walk_spec<16, 4, 256>) spec;
    decltype(&k_rounds_fss<16>) rounds_fss;
    const char *fss_name, *walk_name, *spec_name, *rounds_fss_name;
  };
  const WalkKernels& walk_kernels() const {
    static const WalkKernels k16{16, k_fss<16>, k_rounds_walk<16, 4, 256>, k_walk_spec<16, 4, 256>, k_rounds_fss<16>,
                                 "k_fss<16>", "(k_rounds_walk<16, 4, 256>)", "(k_walk_spec<16, 4, 256>)",
                                 "k_rounds_fss<16>"};
    static const WalkKernels k32{32, k_fss<32>, k_rounds_walk<32, 2, 64>, k_walk_spec<32, 2, 64>, k_rounds_fss<32>,
                                 "k_fss<32>", "(k_rounds_walk<32, 2, 64>)", "(k_walk_spec<32, 2, 64>)",
                                 "k_rounds_fss<32>"};
    return N <= 16 ? k16 : k32;
  }

  // N <= 32 past a fresh state, positions below 65,535 (an online call): the walk's
  // first round, its k_fss rows and their count stay on the device (k_frontier_start
  // writes them; k_fss loops over the count, k_rounds_walk stands down at INF32): no
  // round trip.  The walk's block also does k_round_assign's work and, for up to
  // 65,536 candidates, k_round_tail's.
  Walk walk_online(CoordStep& s) {
    const Tables t = tables();
    const WalkKernels& k = walk_kernels();
    s_fst.need(N + 1);
    if (!s.take_frontier_start())  // (else k_la_seq's last block wrote them)
      KLAUNCH(k_frontier_start, dim3(1), dim3(256), 0, st, t, s.olen, s.len, s_fst.p, s.fss_lo,
              (int32_t*)nullptr, (uint64_t*)nullptr, 0);
    const int64_t guess = (s.n1 - s.n0) + 16 * (int64_t)N;  // the grid loops past it
    cons.und_appended = cons.dividing && cons.n_divided == s.n0;
    Walk w;
    w.assigned = true;
    w.tail_done = cons.n_und + (s.n1 - cons.n_divided) <= 65536;
    const RoundAssign ra = round_assign(s, w.tail_done);
    KLAUNCH_AS(k.fss_name, k.fss, dim3((unsigned)std::min<int64_t>(1024, div_up(guess * k.NPC, 256))), dim3(256), 0,
               st, t, s.fss_lo, s.fss_off, 0, (int32_t*)nullptr, (uint16_t*)d_FSS.p, (const int32_t*)s.fss_total);
    KLAUNCH_AS(k.walk_name, k.walk, dim3(1), dim3(1024), 0, st, t, (const uint16_t*)d_FSS.p, s.olen, s.len, s.rstate,
               0, cons.R, dbg_p(), (const int32_t*)s_fst.p, ra);
    return w;
  }

  // N <= 32 from a fresh state (the frontier starts at round 0, position 0), or with a
  // chain of 65,535 events or more: first-strong-seer rows for every event that can
  // still be a frontier member, sized by the host (one round trip past a fresh state)
  Walk walk_fss(CoordStep& s) {
    const Tables t = tables();
    const WalkKernels& k = walk_kernels();
    const int Rprev = cons.R;  // C rows >= Rprev are empty before this batch
    std::vector<int32_t> fst(N + 1, 0);
    if (!s.fresh) {
      s_fst.need(N + 1);
      KLAUNCH(k_frontier_start, dim3(1), dim3(256), 0, st, t, s.olen, s.len, s_fst.p, (int32_t*)nullptr,
              (int32_t*)nullptr, (uint64_t*)nullptr, 0);
      readback(fst.data(), s_fst.p, N + 1);
    }
    const int rlo = fst[0];
    if (rlo == INF32) return {};
    int tot = s.fresh ? s.tot0 : 0;
    if (!s.fresh) {
      std::vector<int32_t> lo_off(2 * N + 1);
      for (int c = 0; c < N; c++) {
        lo_off[c] = fst[1 + c];
        lo_off[N + c] = tot;
        tot += std::max(0, strm.log.chain_len[c] - fst[1 + c]);
      }
      lo_off[2 * N] = tot;
      h2d(s.fss_lo, lo_off.data(), 4 * (2 * N + 1));
    }
    if (tot <= 0) return {};
    // the LDS walk keeps chain positions as uint16; longer chains take the register
    // walk over the global int32 fss rows
    const bool long_chain = s.maxlen >= 0xFFFF;
    KLAUNCH_AS(k.fss_name, k.fss, dim3(div_up((int64_t)tot * k.NPC, 256)), dim3(256), 0, st, t, s.fss_lo, s.fss_off, tot,
               long_chain ? d_FSS.p : (int32_t*)nullptr, long_chain ? (uint16_t*)nullptr : (uint16_t*)d_FSS.p,
               (const int32_t*)nullptr);
    if (long_chain) {
      KLAUNCH_AS(k.rounds_fss_name, k.rounds_fss, dim3(1), dim3(64), 0, st, t, d_FSS.p, s.olen, s.len, s.rstate, rlo);
      return {};
    }
    const int nw = s.fresh ? spec_walkers(s.minlen) : 0;
    const int32_t* resume = nw > 1 ? spec_walk(t, s, k, nw) : nullptr;
    KLAUNCH_AS(k.walk_name, k.walk, dim3(1), dim3(1024), 0, st, t, (const uint16_t*)d_FSS.p, s.olen, s.len, s.rstate,
               resume ? 0 : rlo, resume ? 0 : Rprev, dbg_p(), resume, RoundAssign{});
    if (resume && hge_hooks::walk_debug()) walk_debug(nw);
    return {};
  }
  // the speculative walkers (hge_walk_spec.hip) and their join; returns the join's resume row
  const int32_t* spec_walk(const Tables& t, const CoordStep& s, const WalkKernels& k, int nw) {
    const int Hcap = hge_hooks::walk_hcap(std::max(256, std::min(Rcap, 3 * (Rcap / nw) + 256)));
    if ((size_t)nw * Hcap * N > s_H.n) {
      s_H.need((size_t)nw * Hcap * N);  // epoch 0 never matches a launch's tag
      HGE_HIPCHK(hipMemsetAsync(s_H.p, 0, s_H.n * sizeof(uint64_t), st));
    }
    s_hres.need(4 * (size_t)nw + 1);
    s_hn.need(2 * (size_t)nw);
    KLAUNCH_AS(k.spec_name, k.spec, dim3(nw), dim3(1024), 0, st, t, (const uint16_t*)d_FSS.p, s.len, nw, Hcap, s_H.p,
               s_hn.p, s_hn.p + nw, (int4*)s_hres.p, ++walk_epoch, walk_chk[0], walk_chk[1], walk_dbg(nw));
    int32_t* resume = s_hres.p + 4 * nw;
    KLAUNCH(k_walk_join, dim3(64), dim3(256), 0, st, t, (const uint64_t*)s_H.p, (const int32_t*)s_hn.p,
            (const int4*)s_hres.p, nw, Hcap, s.rstate, resume);
    return resume;
  }
  // rounds and witnesses of the new events, unless the walk's block assigned them
  void assign_rounds(const CoordStep& s, const Walk& w) {
    const Tables t = tables();
    const int m = (int)(s.n1 - s.n0);
    s_newwit.need(m);
    if (s.fresh) {
      s_newwit.need((size_t)Rcap * N);
      KLAUNCH(k_round_ranges, dim3(div_up((int64_t)Rcap * N, 256)), dim3(256), 0, st, t, s.len,
              (const int32_t*)s.rstate, s_newwit.p, s.rstate + 2);
    } else if (!w.assigned) {
      // DivideRounds right after (divide()) with nothing coordinated but undivided:
      // the new ids join the undetermined list here (no k_iota launch)
      cons.und_appended = cons.dividing && cons.n_divided == s.n0;
      KLAUNCH(k_round_assign, dim3(div_up(m, 256)), dim3(256), 0, st, t, (int)s.n0, (int)s.n1,
              (const int32_t*)s.rstate, s_newwit.p, s.rstate + 2, cons.und_appended ? d_und.p + cons.n_und : (int32_t*)nullptr);
    }
  }
  // k_round_tail, unless the walk's block did its work: the new witnesses' see /
  // strongly-see bitsets, the first witness per round, the round count, and the lowest
  // round of the next batch's candidates (the undetermined list and the events the next
  // divide appends; none to read on a fresh replay).  An online call's few candidates
  // are reduced by `mr` extra blocks (returned), more by the k_min_round pair.
  int rounds_tail(const CoordStep& s, const Walk& w) {
    if (w.tail_done) return 0;
    const Tables t = tables();
    const int m = (int)(s.n1 - s.n0), G = wit_group();
    const int64_t n_mr = cons.n_und + (s.n1 - cons.n_divided);
    const int mr = !s.fresh && n_mr <= 65536 ? (int)std::max<int64_t>(1, std::min<int64_t>(16, div_up(n_mr, 2048))) : 0;
    const int64_t wmax = std::min<int64_t>(m, (int64_t)Rcap * N);  // witnesses <= both
    const int nb_wb = std::max(1, std::min(div_up(wmax * NW * G, 256), 8192));
    KLAUNCH(k_round_tail, dim3(nb_wb + div_up(Rcap, 4) + mr), dim3(256), 0, st, t, s_newwit.p, s.rstate + 2,
            N > 32 ? (const uint64_t*)d_ssc.p : nullptr, G, nb_wb, (const int32_t*)s.rstate, d_minw.p, w.err_src, mr,
            (const int32_t*)d_und.p, (int)cons.n_und, (int)cons.n_divided, (int)s.n1);
    if (!s.fresh && !mr) {
      int32_t* mnr = d_minw.p + Rcap + hge_plan::kTailMinRound;
      if (cons.n_und > 0)
        KLAUNCH(k_min_round, dim3(div_up(cons.n_und, 256)), dim3(256), 0, st, d_round.p, d_und.p, (int)cons.n_und, mnr);
      if (s.n1 > cons.n_divided)
        KLAUNCH(k_min_round_range, dim3(div_up(s.n1 - cons.n_divided, 256)), dim3(256), 0, st, d_round.p,
                (int)cons.n_divided, (int)s.n1, mnr);
    }
    return mr;
  }
  // the one readback: the rounds' first witnesses and the tail words behind them
  RoundsOutcome read_rounds(const CoordStep& s, const Walk& w, int mr) {
    cons.h_minw.resize(Rcap + hge_plan::kTailPartial + mr);
    d2h(cons.h_minw.data(), d_minw.p, 4 * cons.h_minw.size());
    sync();
    cons.minw_full = false;  // every round's first witness is in d_minw now
    const hge_plan::RoundsTail r = hge_plan::parse_rounds_tail(cons.h_minw.data() + Rcap, mr);
    if (!s.fresh) cons.mnr_pre = r.min_round;
    cons.mnr_key[0] = s.fresh ? -1 : cons.n_und;
    cons.mnr_key[1] = cons.n_divided;
    cons.mnr_key[2] = s.n1;
    if (w.err_src ? r.handoff_err != 0 : w.host_err) return RoundsOutcome::HandoffTimeout;
    if (r.overflow) return RoundsOutcome::Grow;
    cons.R = r.R;
    cons.h_minw.resize(cons.R);
    return RoundsOutcome::Done;
  }

  // Walkers of the speculative frontier walk (hge_walk_spec.hip) for a fresh
  // state: one per ~192 positions of the shortest chain, up to 32 (HGE_WALKERS
  // overrides; 0 or 1 = the sequential walk).  Short graphs walk sequentially.
  int spec_walkers(int minlen) {
    const int env = hge_hooks::walkers();
    const int nw = env >= 0 ? env : (minlen >= 4 * 192 ? std::min(32, minlen / 192) : 0);
    return std::max(0, std::min(nw, 64));
  }

  // HGE_WALK_DEBUG: per-walker rows, merge results and cycle stamps on stderr
  uint64_t* walk_dbg(int nw) {
    if (!hge_hooks::walk_debug()) return nullptr;
    s_wdbg.need(4 * (size_t)nw);
    return s_wdbg.p;
  }
  void walk_debug(int nw) {
    std::vector<int32_t> res(4 * nw + 1), hn(nw);
    std::vector<uint64_t> wd(4 * nw);
    readback(res.data(), s_hres.p, res.size());
    readback(hn.data(), s_hn.p, hn.size());
    readback(wd.data(), s_wdbg.p, wd.size());
    fprintf(stderr, "walk: nw=%d resume=%d |", nw, res[4 * nw]);
    for (int w = 0; w < nw; w++)
      fprintf(stderr, " %d:%d[%d,%d,%d,%d](%llu/%llu/%llu)", w, hn[w], res[4 * w], res[4 * w + 1],
              res[4 * w + 2], res[4 * w + 3], (unsigned long long)wd[4 * w],
              (unsigned long long)wd[4 * w + 1], (unsigned long long)wd[4 * w + 2]);
    fprintf(stderr, "\n");
  }

  // Speculative walkers of the wide walk (fresh state, N <= 128): as many
  // N-workgroup walkers as stay co-resident, up to 8; HGE_COOP_WALKERS overrides
  // (read per call: the tests vary it; 0 or 1 = the sequential kernel alone).
  int coop_walkers(int minlen) {
    // walker block size: 512 threads x 2 per CU at N <= 64, 1024 x 1 above (means over
    // seeds 1-3, profiles/r01/specbs: 113.3 vs 106.4M ev/s at 64/1M, 60.8 vs 62.9M at 128/1M)
    const int sbs = N > 64 ? 1024 : COOP_SPEC_BS;
    if (sbs != coop_spec_bs) {
      coop_spec_bs = sbs;
      HGE_HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&coop_spec_nb, coop_spec_fn(), sbs, 0));
    }
    const int cap = (int)std::min<int64_t>(16, (int64_t)coop_spec_nb * coop_ncu / N);
    // above N = 128 only 2 walkers fit, and the 512-thread sequential kernel is faster
    // than 2 walkers sharing each CU (22.5 vs 33.6 ms at 256/2M, profiles/r01r_*)
    int nw = hge_hooks::coop_walkers(minlen >= 1024 && N <= 128 ? 8 : 0);
    nw = std::min(nw, cap);
    return nw >= 2 ? nw : 0;
  }

  // Launch of a grid whose workgroups hand data to each other (the frontier
  // kernels).  Co-residency is checked once with the occupancy API
  // (coop_checked, coop_walkers); a plain launch of such a grid gets the same
  // residency as a cooperative one (MI355X_MICROARCH.md, Residency), and
  // hipLaunchCooperativeKernel puts the work on a separate device queue whose
  // teardown at process exit crashed under rocprofv3 (profiles/r02_exit_segv.md).
  // Every such launch first checks, for the exact kernel instantiation and block
  // size, that the whole grid fits on the device at once; a grid that cannot be
  // co-resident is refused before anything is written.  The caller holds
  // frontier_lock(): two of these grids on one device (two wide engines driven
  // by different host threads) could each hold part of the CUs and wait on each
  // other's missing workgroups, so one process runs them one at a time.  (Grids of
  // other processes on the same device are not covered: wide engines need the
  // device to themselves)
  hipError_t launch_resident(const void* fn, dim3 grid, dim3 block, void** args) {
    const int bs = (int)(block.x * block.y * block.z);
    int nb = -1;
    for (auto& e : resident_nb)
      if (e.first.first == fn && e.first.second == bs) nb = e.second;
    if (nb < 0) {
      HGE_HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, bs, 0));
      resident_nb.push_back({{fn, bs}, nb});
    }
    const int64_t blocks = (int64_t)grid.x * grid.y * grid.z;
    if ((int64_t)nb * n_cu() < blocks)
      throw Error(HGE_ERR_DEVICE, "frontier grid of " + std::to_string(blocks) + " workgroups x " +
                                            std::to_string(bs) + " threads cannot be co-resident (" +
                                            std::to_string(nb) + " per CU x " + std::to_string(n_cu()) + " CUs)");
    return hipLaunchKernel(fn, grid, block, args, 0, st);
  }
  static std::mutex& frontier_mutex(int dev) {
    static std::mutex m[64];
    return m[dev & 63];
  }
  std::unique_lock<std::mutex> frontier_lock() { return std::unique_lock<std::mutex>(frontier_mutex(device)); }

  // Wide rounds step: strongly-see tiles on the coordinate rows
  // (hge_rounds_direct.hip) for N % 4 == 0, else the FDT-gather selection of
  // hge_rounds_coop.hip.
  bool direct_rounds() const { return (N & 3) == 0; }

  // rounds of a wide hashgraph: the frontier start, a split run's joined rows or the speculative
  // walkers, then the walk's one grid (the caller holds frontier_lock() until the stream has drained)
  Walk rounds_coop(CoordStep& s) {
    const Tables t = tables();
    s_fst.need(N + 1);
    // (the hand-off flags and granules are zeroed by k_frontier_start)
    s_bar.need(2);
    s_gran.need(2 * (size_t)N);
    if (!s.take_frontier_start())  // (else the chain fill's last block ran it)
      KLAUNCH(k_frontier_start, dim3(1), dim3(256), 0, st, t, s.olen, s.len, s_fst.p, (int32_t*)nullptr,
              s_bar.p, (uint64_t*)s_gran.p, 2 * N);
    // the lowest round to recompute: read back for a fresh state (the walkers and the
    // joined rows need it on the host), else read by the frontier kernel itself,
    // which stands down at INF32 (no round trip)
    int32_t rlo = s.fresh ? INF32 : 0;
    const int32_t* rlo_dev = s.fresh ? nullptr : s_fst.p;
    if (s.fresh) readback(&rlo, s_fst.p, 1);
    if (rlo == INF32) return {};
    const int Rprev = cons.R;
    if (!coop_resident()) {  // a device too small for the walk's grid
      frontier_fallback = true;
      return rounds_step32(s);
    }
    // admission switches the engine to int32 positions (to_wide32) before a chain
    // passes 65,534 events, so this packed walk never sees one; the check guards it
    if (s.maxlen >= 0xFFFF)
      throw Error(HGE_ERR_INTERNAL, "packed rounds walk reached a chain past 65,534 events");
    const bool from_zero = s.fresh && rlo == 0 && Rprev == 0;
    if (cons.ext_on && from_zero && install_ext_rows(s, rlo)) return {};
    Walk w;
    const int nw = from_zero && rlo == 0 ? coop_walkers(s.minlen) : 0;  // (the joined rows may have moved rlo)
    if (nw >= 2) {
      const int resume = coop_spec_walk(t, s, nw, Rprev, w);
      if (resume < 0) return w;
      rlo = resume;
    }
    wide_walk(t, s, rlo, rlo_dev, Rprev);
    // the hand-off error flag comes back with the round count (read_rounds, k_round_tail)
    w.err_src = s_bar.p + 1;
    dbg_dump();
    return w;
  }
  // the walk's grid must fit the device at once: checked once with the occupancy API
  bool coop_resident() {
    if (coop_checked) return true;
    int nb = 0, ncu = 0, coop = 0;
    HGE_HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)k_rounds_coop, COOP_BS, 0));
    HGE_HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    HGE_HIPCHK(hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, device));
    if (!coop || (int64_t)nb * ncu < N) return false;
    coop_nb = nb;
    coop_ncu = ncu;
    coop_checked = true;
    return true;
  }
  // frontier rows joined from the walkers of all ranks (babble_amd/dist.py); true:
  // nothing is left to walk (rstate says why), else rlo is the row to resume from
  bool install_ext_rows(const CoordStep& s, int32_t& rlo) {
    const int K = cons.ext_rows;  // true rows 0 .. K-1
    if (K + 1 >= Rcap) {  // the rounds table must hold them: overflow, grow, come back
      const int32_t ov[2] = {0, hge_plan::kRoundsFull};
      h2d(s.rstate, ov, 8);
      return true;
    }
    cons.ext_on = false;
    h2d(d_C.p, cons.ext_C.data(), sizeof(int32_t) * (size_t)K * N);
    if (K > 1) h2d(d_ssc.p + (size_t)N * NW, cons.ext_ssc.data() + (size_t)N * NW, sizeof(uint64_t) * (size_t)(K - 1) * N * NW);
    if (cons.ext_natural) {  // the walk ended: row K is the empty frontier
      const int32_t rs0 = K;
      h2d(s.rstate, &rs0, 4);
      return true;
    }
    rlo = K - 1;  // the sequential walk resumes from the last true row
    return false;
  }
  // the wide walk's speculative walkers and their join; returns the row to resume from,
  // < 0: nothing left to walk (every round covered, or a hand-off timeout: w.host_err)
  int coop_spec_walk(Tables t, const CoordStep& s, int nw, int Rprev, Walk& w) {
    const int32_t* FDT = d_FDT.p;
    const int32_t* olen = s.olen;
    const int32_t* len = s.len;
    int32_t* err = s_bar.p + 1;
    const int Hcap = std::min(0xFFFF, hge_hooks::walk_hcap(std::min(Rcap, std::max(256, 3 * (Rcap / nw) + 256))));
    int TS = 64;
    while (TS < 2 * Hcap) TS <<= 1;
    const size_t nh = (size_t)nw * Hcap * N, nt = (size_t)nw * TS;
    const size_t hn0 = s_cH.n, tn0 = s_cT.n;  // a new allocation holds arbitrary words
    s_cH.need(nh);
    s_cT.need(nt);
    bool clear = s_cH.n != hn0 || s_cT.n != tn0;
    if (++coop_epoch >= 0x7FFFFFFFu) {  // tags wrap: clear, restart at 1
      coop_epoch = 1;
      clear = true;
    }
    if (clear) {
      HGE_HIPCHK(hipMemsetAsync(s_cH.p, 0, s_cH.n * sizeof(uint64_t), st));
      HGE_HIPCHK(hipMemsetAsync(s_cT.p, 0, s_cT.n * sizeof(uint64_t), st));
    }
    s_cS.need(nh * NW);
    s_cM.need(nw);
    s_cn.need(2 * (size_t)nw + 1);
    HGE_HIPCHK(hipMemsetAsync(s_cM.p, 0xFF, (size_t)nw * sizeof(uint64_t), st));
    int64_t nev = 0;
    for (int c = 0; c < N; c++) nev += strm.log.chain_len[c];
    // guesses (measured over seeds 1-3, profiles/r01/guess128): time cuts at N <= 64,
    // alternating length/time cuts above
    const int guess = N <= 64 ? 1 : 2;
    CoopSpec cs{s_cH.p, s_cS.p, s_cT.p, (unsigned long long*)s_cM.p, s_cn.p, nw, Hcap, TS,
                coop_epoch, nev, guess};
    void* sargs[] = {&t, &FDT, &olen, &len, &cs, &err};
    prof.begin("k_rounds_coop_spec");
    HGE_HIPCHK(launch_resident(coop_spec_fn(), dim3(nw * N), dim3(coop_spec_bs), sargs));
    prof.end();
    int32_t* resume = s_cn.p + 2 * nw;
    KLAUNCH(k_coop_join, dim3(64), dim3(256), 0, st, t, cs, d_ssc.p, s.rstate, resume);
    int32_t hres[2] = {0, 0};
    readback(&hres[0], err, 1);
    if (hres[0]) {  // co-residency failure: coords_b falls back to k_round_step32
      const int32_t down[2] = {Rprev, hge_plan::kRoundsStoodDown};
      h2d(s.rstate, down, 8);
      w.host_err = true;
      return -1;
    }
    readback(&hres[1], resume, 1);
    if (hge_hooks::walk_debug()) {
      std::vector<int32_t> hn(2 * nw);
      std::vector<uint64_t> mg(nw);
      readback(hn.data(), s_cn.p, hn.size());
      readback(mg.data(), s_cM.p, mg.size());
      fprintf(stderr, "coop walk: nw=%d Hcap=%d resume=%d |", nw, Hcap, hres[1]);
      for (int i = 0; i < nw; i++)
        fprintf(stderr, " %d:%d%s->(%d,w%d:%d)", i, hn[i], hn[nw + i] ? "e" : "",
                mg[i] == ~0ull ? -1 : (int)(mg[i] >> 32),
                mg[i] == ~0ull ? -1 : i + (int)((mg[i] >> 16) & 0xFFFF), (int)(mg[i] & 0xFFFF));
      fprintf(stderr, "\n");
    }
    return hres[1];
  }
  // the wide walk's one grid: direct (N % 4 == 0) or the FDT-gather selection
  void wide_walk(Tables t, const CoordStep& s, int32_t rlo, const int32_t* rlo_dev, int Rprev) {
    const int32_t* FDT = d_FDT.p;
    const int32_t* olen = s.olen;
    const int32_t* len = s.len;
    int32_t* rstate = s.rstate;
    int32_t* err = s_bar.p + 1;
    uint64_t* gran = s_gran.p;
    uint64_t* ssc = d_ssc.p;
    uint64_t* dbg = dbg_p();
    if (direct_rounds()) {
      uint32_t* mb = walk_mb();
      unsigned long long* paths = walk_paths();
      unsigned long long* paths_next = s_wpaths.p + 2 * ((walk_seq + 1) & 1);
      const int32_t* nostart = nullptr;
      int32_t* nohist = nullptr;
      int hmax = 0, extra = 0;
      // tests: the walk stalls at this hand-off epoch (chain 0 never publishes it)
      int stall_ep = hge_hooks::test_handoff_stall();
      int force_exact = walk_force_exact();
      // tests: at this hand-off epoch chain 1 flags its staged member row (a fine one)
      int mflag_ep = hge_hooks::test_dir_member_flag();
      void* dargs[] = {&t, &olen, &len, &rstate, &rlo, &rlo_dev, &Rprev, &gran, &err, &ssc, &mb, &dbg,
                       &nostart, &nohist, &hmax, &nostart, &extra, &stall_ep, &force_exact, &mflag_ep, &paths,
                       &paths_next};
      prof.begin("k_rounds_direct");
      HGE_HIPCHK(launch_resident(direct_fn(), dim3(N), dim3(1024), dargs));
      prof.end();
    } else {
      void* args[] = {&t, &FDT, &olen, &len, &rstate, &rlo, &rlo_dev, &Rprev, &gran, &err, &ssc, &dbg};
      prof.begin("k_rounds_coop");
      HGE_HIPCHK(launch_resident((const void*)k_rounds_coop, dim3(N), dim3(COOP_BS), args));
      prof.end();
    }
    if (hge_hooks::test_handoff_fail()) {  // tests: the walk reports a hand-off timeout
      const int32_t one = 1, down = hge_plan::kRoundsStoodDown;
      h2d(err, &one, 4);
      h2d(rstate + 1, &down, 4);
    }
  }
  // the direct walk's staged member rows: two parity blocks of npow rows x npow/2 packed
  // words, then two of npow x npow bytes, the same rows in 8-bit form (hge_narrow.h)
  uint32_t* walk_mb() {
    s_mb.need((size_t)npow() * npow() + (size_t)npow() * npow() / 2);
    return s_mb.p;
  }
  // The walk's select-path counters (hge_walk_select_paths): two slots of {narrow, exact},
  // cleared once here.  Walk k adds to slot k & 1 and clears the other slot as it ends,
  // for the walk after it on the stream: no clearing launch per walk (an online call is a
  // few hundred microseconds, a memset node was ~10 of them).
  unsigned long long* walk_paths() {
    if (!s_wpaths.p) {
      s_wpaths.need(4);
      HGE_HIPCHK(hipMemsetAsync(s_wpaths.p, 0, 4 * sizeof(unsigned long long), st));
    }
    walk_seq++;
    return s_wpaths.p + 2 * (walk_seq & 1);
  }
  // The order stage's sort-path counters (hge_sort_paths): two slots of {packed, index,
  // k_bucket_sort_big's next bucket, unused}, handed over like the walk's.  An order stage without a bucket past 512 keys launches
  // no counting kernel and reports (0, 0).
  SortCtl sort_ctl() {
    if (!s_spaths.p) {
      s_spaths.need(8);
      // on the engine's stream (it does not wait for the null stream): cleared before the
      // first stage deals buckets from the counter
      HGE_HIPCHK(hipMemsetAsync(s_spaths.p, 0, 8 * sizeof(unsigned long long), st));
    }
    sort_seq++;
    sort_counted = true;
    return SortCtl{s_spaths.p + 4 * (sort_seq & 1), s_spaths.p + 4 * ((sort_seq + 1) & 1),
                   hge_hooks::test_sort_index()};
  }
  // tests (HGE_TEST_DIR_EXACT=1): every round of the walk takes the 16-bit select
  static int walk_force_exact() { return hge_hooks::test_dir_exact(); }
  const void* direct_fn() const {
    return N <= 64 ? (const void*)k_rounds_direct<1024, 64>
         : N <= 128 ? (const void*)k_rounds_direct<1024, 128>
                    : (const void*)k_rounds_direct<1024, 256>;
  }

  // N > 32: lastAncestors live in the packed 16-bit table while every chain holds at
  // most 65,534 events; a longer chain switches the engine to int32 LA rows for good
  // (to_wide32 below), which the N <= 32 path uses from the start
  bool sweep16() const { return N > 32 && !strm.wide32; }
  // the median's threshold rows as uint16 (k_witness_la, k_median_wave's 4-witness lanes)
  bool wla16() const { return N > 192 && (N & 3) == 0 && !strm.wide32; }

  // the switch to int32 positions (hge_wide32.hip): the int32 LA rows of every event
  // with coordinates, unpacked from LA16; from here on the N <= 32 sweeps and
  // transposes, k_round_step32 and k_seg_theta32 take the wide path's place
  // Runs at the next coordinate step after admission lifted the cap.  The pending
  // flag is cleared only once the int32 tables exist: a failed allocation leaves the
  // engine refusing every later step (the packed tables can no longer hold the
  // positions) instead of packing positions past 65,534 into uint16.
  // A retry after a failed allocation resumes where the last attempt stopped: the int32
  // LA table comes first (nothing is converted before it exists), and each uint16 table
  // widened is marked in w32_done, so a retry never reads a widened table as uint16.
  void to_wide32() {
    auto test_stop = [&](int stage) {  // HGE_TEST_W32_FAIL=stage: one failure after that stage
      if (test_w32_fail == stage) {
        test_w32_fail = 0;
        throw Error(HGE_ERR_DEVICE, "test: to_wide32 stopped after stage " + std::to_string(stage));
      }
    };
    ensure_fdtd();  // (the pass reads the uint16 runs)
    if (!(strm.w32_done & 4)) {
      const size_t n = (size_t)N * ccap * N;  // [N][ccap][N], written by k_la16_to_la32 below
      d_LA.regrow_rows(0, 0, 0, sizeof(int32_t) * n, n, false, st);
      sync();
      strm.w32_done |= 4;
      test_stop(1);
    }
    if (fdt16()) {  // the runs and FD rows continue in int32 from here: widen the kept ones
      const size_t n = (size_t)N * N * ccap;
      for (int which = 0; which < 2; which++) {
        if (strm.w32_done & (1 << which)) continue;
        DBuf<int32_t>& b = which ? d_FD : d_FDT;
        DBuf<int32_t> q;
        q.need(n);
        KLAUNCH(k_fdt16_to32, dim3((unsigned)std::min<size_t>(div_up(n, 256), 65536)), dim3(256), 0, st,
                (const uint16_t*)b.p, q.p, n, which);
        sync();
        b.adopt(std::move(q));
        strm.w32_done |= 1 << which;
        test_stop(2 + which);
      }
    }
    s_w32.need(N);
    h2d(s_w32.p, cons.coords_len.data(), 4 * (size_t)N);
    strm.wide32 = true;
    strm.wide32_pending = false;
    strm.w32_done = 0;
    Tables t = tables();
    int64_t most = 1;
    for (int c = 0; c < N; c++) most = std::max<int64_t>(most, (int64_t)cons.coords_len[c] * N);
    KLAUNCH(k_la16_to_la32, dim3((unsigned)std::min<int64_t>(div_up(most, 256), 4096), N), dim3(256), 0, st, t,
            (const uint32_t*)d_LA16.p, (const int32_t*)s_w32.p);
  }

  // rounds with int32 positions: k_round_step32 round by round from the first round
  // to recompute, 32 launches between readbacks of their "row exists" flags
  Walk rounds_step32(const CoordStep& s) {
    Tables t = tables();
    s_fst.need(N + 1);
    KLAUNCH(k_frontier_start, dim3(1), dim3(256), 0, st, t, s.olen, s.len, s_fst.p, (int32_t*)nullptr,
            (int32_t*)nullptr, (uint64_t*)nullptr, 0);
    int32_t rlo = INF32;
    readback(&rlo, s_fst.p, 1);
    if (rlo == INF32) return {};
    const int Rprev = cons.R, NB = 32;
    s_w32a.need(NB);
    for (int r = rlo;;) {
      HGE_HIPCHK(hipMemsetAsync(s_w32a.p, 0, 4 * NB, st));
      int k = 0;
      for (; k < NB && r + k + 1 < Rcap; k++)
        KLAUNCH(k_round_step32, dim3(N), dim3(256), 0, st, t, (const int32_t*)s.olen, (const int32_t*)s.len,
                r + k, Rprev, d_ssc.p, s_w32a.p + k);
      std::vector<int32_t> alive(NB, 0);
      readback(alive.data(), s_w32a.p, NB);
      for (int q = 0; q < k; q++)
        if (!alive[q]) {  // row r + q + 1 is empty: the rounds end there
          const int32_t rs[2] = {std::max(cons.R, r + q + 1), 0};
          h2d(s.rstate, rs, 8);
          return {};
        }
      r += k;
      if (k < NB) {  // the rounds table is full: grown by the caller, walked again
        const int32_t rs[2] = {cons.R, hge_plan::kRoundsFull};
        h2d(s.rstate, rs, 8);
        return {};
      }
    }
  }

  // N > 128, N % 4 == 0, uint16 positions: the FDT runs as uint16 (k_la16_rows_runs<uint16_t>,
  // k_fd_transpose_ts<uint16_t>: half the run table's bytes written and read).  Neither the
  // direct walk nor theta reads FDT; the speculative walkers (N <= 128) and the
  // FDT-gather walk (N % 4 != 0) read int32 runs.
  bool fdt16() const { return N > 128 && (N & 3) == 0 && !strm.wide32; }

  // 32 < N <= 256: lastAncestors by windowed exact propagation (hge_coords_win.hip)
  // instead of the sweeps
  bool la_windows() const { return N > 32 && N <= 256 && !strm.wide32; }

  // passes over windows of the new ids until one changes no row (n_sweeps = passes
  // run); one window is exact in its first pass (its starting rows are final)
  void la_windows_run(const Tables& t, const CoordStep& s) {
    const int32_t* olen = s.olen;
    const int32_t* len = s.len;
    const int64_t n0 = s.n0, n1 = s.n1, ne = n1 - n0;
    const int npow = this->npow();
    // k_la_win: one 1024-thread workgroup per window (a barrier-free wave-per-slice
    // variant measured 2x slower: DESIGN.md §4.1)
    const int W = t.NW2;
    const int64_t WMIN = 4096;  // ids per window at least
    const int per_cu = npow == 256 ? 1 : 2;
    int64_t G = std::min<int64_t>((int64_t)n_cu() * per_cu, std::max<int64_t>(1, ne / WMIN));
    G = hge_hooks::lw_windows(G);
    int64_t WN = (div_up(ne, G) + LW_K - 1) / LW_K * LW_K;
    G = div_up(ne, WN);
    s_lwplan.need(ne);
    s_lwsum.need(ne);
    s_lwinit.need((size_t)G * N * W);
    s_lwpos.need((size_t)G * N);
    s_lwrisky.need(G);
    const int MAXP = 64;
    s_chg.need(MAXP);
    // one window (an online call): its chain start positions are the chains' old
    // lengths and its risky id starts at -1 in the control block, so k_lw_pos is not
    // needed (one launch less per call)
    const int32_t* wpos = G == 1 ? olen : s_lwpos.p;
    int32_t* risky = G == 1 ? s.risky1 : s_lwrisky.p;
    if (G > 1)
      KLAUNCH(k_lw_pos, dim3(div_up(std::max<int64_t>(G * N, MAXP), 256)), dim3(256), 0, st, t, n0, (int)WN, (int)G,
              len, s_lwpos.p, s_lwrisky.p, s_chg.p, MAXP);
    // one window: its workgroup plans its own chunks (k_la_win's plan_len)
    if (G > 1)
      KLAUNCH(k_lw_plan, dim3(div_up(div_up(ne, LW_K), 4)), dim3(256), 0, st, t, n0, n1, (int)WN, len, s_lwplan.p,
              risky);
    int p = 0;
    for (int group = G == 1 ? 1 : 3;; group = 2) {
      for (int g = 0; g < group; g++, p++) {
        if (p >= MAXP) throw Error(HGE_ERR_INTERNAL, "lastAncestors windows did not converge");
        const int32_t* prev = p > 0 ? s_chg.p + p - 1 : nullptr;
        const int pass = p + 1;
#define LWIN(NP)                                                                                         \
  KLAUNCH(k_la_win<NP>, dim3(G), dim3(1024), 0, st, t, s_lwplan.p, n0, n1, (int)WN, wpos, olen,          \
          s_lwinit.p, risky, s_lwsum.p, pass, prev, s_chg.p + p,                                        \
          G == 1 && p == 0 ? len : (const int32_t*)nullptr)
        if (npow == 64) LWIN(64);
        else if (npow == 128) LWIN(128);
        else LWIN(256);
#undef LWIN
      }
      if (G == 1) {
        n_sweeps = 1;
        break;
      }
      std::vector<int32_t> flags(p);
      readback(flags.data(), s_chg.p, p);
      if (!flags[p - 1]) {
        n_sweeps = (int)(std::find(flags.begin(), flags.end(), 0) - flags.begin()) + 1;
        break;
      }
    }
  }

  // the one-pass lastAncestors kernel (k_la_seq) takes batches of m new events at N <= 32
  bool la_seq_ok(int64_t m) const {
    return !sweep16() && N <= 32 && m > 0 && m * (N <= 16 ? 16 : 32) <= LASEQ_MAX && !hge_hooks::no_laseq();
  }
  // lastAncestors of the new events: windows, one pass, or sweeps to the fixed point
  static constexpr int MAXSW = 4096;  // sweeps at most
  void last_ancestors(const Tables& t, CoordStep& s) {
    s_chg.need(MAXSW);  // the passes' "changed" flags
    if (s.la == CoordStep::La::Windows) {
      la_windows_run(t, s);
    } else if (s.la == CoordStep::La::Seq) {
      la_seq_run(t, s);
    } else {
      la_sweeps_run(t, s);
    }
  }
  // a small batch (an online call): one exact pass in insertion order, the chain table
  // filled by the same kernel
  void la_seq_run(const Tables& t, CoordStep& s) {
    // past a fresh state: + k_fd_qlo's N blocks, + k_frontier_start's block when coords_b walks as an online
    // call; at N <= 16 the batch's firstDescendants in the same launch instead (no runs, transpose, k_fd_qlo)
    const bool q = !s.fresh, fst = q && s.maxlen < 0xFFFF;
    const bool fd = q && N <= 16 && !hge_hooks::no_fd_direct();
    if (fst) s_fst.need(N + 1);
    int32_t* fp = fst ? s_fst.p : (int32_t*)nullptr;
    int32_t* fl = fst ? s.fss_lo : (int32_t*)nullptr;
    const int nq = q && !fd ? N : 0;
    const int nb = 1 + nq + (fst ? 1 : 0);
    if (N <= 16)
      KLAUNCH(k_la_seq<16>, dim3(nb), dim3(256), 0, st, t, (int)s.n0, (int)s.n1, s.up, s.up_dst,
              (const int32_t*)s.olen, (const int32_t*)s.len, nq ? s.qlo : (int32_t*)nullptr, fp, fl,
              fd ? d_FDT.p : (int32_t*)nullptr);
    else
      KLAUNCH(k_la_seq<32>, dim3(nb), dim3(256), 0, st, t, (int)s.n0, (int)s.n1, s.up, s.up_dst,
              (const int32_t*)s.olen, (const int32_t*)s.len, nq ? s.qlo : (int32_t*)nullptr, fp, fl,
              (int32_t*)nullptr);
    s.frontier_started = fst;
    s.qlo_done = q;
    s.fd_done = fd;
    n_sweeps = 1;
  }
  // sweeps until one changes nothing; queued in groups, checked once per group
  // (a sweep after a quiet one returns at once); k_la_clear zeroes the flags
  void la_sweeps_run(const Tables& t, const CoordStep& s) {
    const int32_t* olen = s.olen;
    const int32_t* len = s.len;
    const int nseg = s.nseg, SEG = s.SEG, maxnew = s.maxnew;
    const bool p16 = sweep16();
    // the packed sweeps skip segments whose inputs did not change in the previous sweep
    if (p16) s_dirty.need(nseg);
    int32_t* dirty = p16 ? s_dirty.p : nullptr;
    if (p16)
      KLAUNCH(k_la_clear16, dim3(std::max(1, std::min(64, div_up((int64_t)maxnew * t.NW2, 256))), N),
              dim3(256), 0, st, t, olen, len, s_chg.p, MAXSW, dirty, nseg);
    else
      KLAUNCH(k_la_clear, dim3(std::max(1, std::min(64, div_up((int64_t)maxnew * N, 256))), N),
              dim3(256), 0, st, t, olen, len, s_chg.p, MAXSW);
    const int NPt = p16 ? (t.NW2 <= 32 ? 32 : t.NW2 <= 64 ? 64 : 128)
                        : (N <= 16 ? 16 : N <= 32 ? 32 : N <= 64 ? 64 : N <= 128 ? 128 : 256);
    int sw = 0;
    for (int group = 12;; group = 8) {
      for (int g = 0; g < group; g++, sw++) {
        if (sw >= MAXSW) throw Error(HGE_ERR_INTERNAL, "lastAncestors sweeps did not converge");
        const int32_t* prev = sw > 0 ? s_chg.p + sw - 1 : nullptr;
        if (p16) {
          switch (NPt) {
#define SW16(NPV)                                                                                \
  case NPV:                                                                                      \
    KLAUNCH(k_la_sweep16<NPV>, dim3(div_up(nseg, 256 / NPV)), dim3(256), 0, st, t, s.segs, nseg, \
            SEG, len, prev, s_chg.p + sw, olen, s.segbase, dirty, sw);                          \
    break;
            SW16(32)
            SW16(64)
            SW16(128)
#undef SW16
          }
        } else {
          switch (NPt) {
#define SW(NPV)                                                                                  \
  case NPV:                                                                                      \
    KLAUNCH(k_la_sweep<NPV>, dim3(div_up(nseg, 256 / NPV)), dim3(256), 0, st, t, s.segs, nseg,   \
            SEG, len, prev, s_chg.p + sw);                                                       \
    break;
            SW(16)
            SW(32)
            SW(64)
            SW(128)
            SW(256)
#undef SW
          }
        }
      }
      std::vector<int32_t> flags(sw);
      readback(flags.data(), s_chg.p, sw);
      if (!flags[sw - 1]) {
        // sweeps that did work: up to and including the first one that changed nothing
        n_sweeps = (int)(std::find(flags.begin(), flags.end(), 0) - flags.begin()) + 1;
        break;
      }
    }
  }
  // k_fd_transpose_ts over the stale rows of d_FDTD / d_FDTW from s_fdlo[c] on (the FD
  // rows it writes again hold the same values); zgrid: position tiles per chain in the
  // grid (the kernel loops past it)
  void fdtd_pass(const char* name, int zgrid) {
    const Tables t = tables();
    KLAUNCH_AS(name, (k_fd_transpose_ts<uint16_t>), dim3(N, div_up(N, 64), std::max(1, std::min(zgrid, 65535))),
               dim3(256), 0, st, t, (const uint16_t*)d_FDT.p, (const int32_t*)s_fdlo.p,
               (const int32_t*)(s_fdlo.p + N), (const int32_t*)nullptr, (const int32_t*)nullptr);
  }
  // every reader of d_FDTD / d_FDTW: the whole table, when a bulk replay left it stale
  void ensure_fdtd() {
    if (!cons.fdtd_stale) return;
    if (!fdt16()) throw Error(HGE_ERR_INTERNAL, "stale FD timestamp rows past the uint16 runs");
    HGE_HIPCHK(hipMemsetAsync(s_fdlo.p, 0, 4 * (size_t)N, st));
    fdtd_pass("fdtd_ensure (k_fd_transpose_ts<uint16_t>)", div_up(std::max(cons.fdtd_maxlen, 1), 64));
    cons.fdtd_stale = false;
  }
  // firstDescendants: the FDT runs from the LA rows, then FDT -> FD rows
  void first_descendants(const Tables& t, const CoordStep& s) {
    if (s.fd_done) return;  // (k_la_seq wrote the FD rows and FDT runs)
    if (!s.fresh) ensure_fdtd();  // (the stale rows' runs and lengths are the old ones)
    const int32_t* olen = s.olen;
    const int32_t* len = s.len;
    const int maxnew = s.maxnew;
    if (fdt16()) {
      KLAUNCH((k_la16_rows_runs<uint16_t>), dim3(div_up(maxnew + 1, 64), div_up(N, 64), N), dim3(256), 0, st, t,
              (uint16_t*)d_FDT.p, s.plo, olen, len);
    } else if (sweep16()) {
      // LA16 -> the int32 LA rows and the FDT runs from the same tiles (no LAT)
      KLAUNCH((k_la16_rows_runs<int32_t>), dim3(div_up(maxnew + 1, 64), div_up(N, 64), N), dim3(256), 0, st, t,
              d_FDT.p, s.plo, olen, len);
    } else {
      // the int32 LA rows -> the runs of the new events (and the new positions with no
      // descendant yet) through 64 x 64 LDS tiles (one launch; round 3's LA -> LAT
      // transpose + k_fdt_runs took two and the LAT table)
      KLAUNCH((k_la16_rows_runs<int32_t, true>), dim3(div_up(maxnew + 1, 64), div_up(N, 64), N), dim3(256), 0,
              st, t, d_FDT.p, s.plo, olen, len);
    }
    // FDT -> FD rows for every chain-c position a new event can have touched
    // (from a fresh state: every row, qlo = 0 as uploaded; no round trip)
    // (the rows' lower bounds stay on the device: the transposes loop over position
    // tiles past their grid, sized here for the new positions plus a tile)
    int span = 1;
    if (!s.fresh) {
      if (!s.qlo_done) KLAUNCH(k_fd_qlo, dim3(N), dim3(256), 0, st, t, olen, len, s.qlo);
      span = maxnew + 64;
    } else {
      span = std::max(span, s.maxlen);
    }
    // (a split part writes the timestamp rows of its own candidates only)
    if (s.fresh) cons.fdtd_stale = false;  // (every row is written again below, or marked)
    if (s.fd_rows_only) {
      // the FD rows alone: the timestamp table is stale from position 0 of every chain
      KLAUNCH(k_fd_rows16, dim3(N, div_up(N, 64), std::min(div_up(span, 64), 65535)), dim3(256), 0, st, t,
              (const uint16_t*)d_FDT.p, (const int32_t*)s.qlo, len);
      s_fdlo.need(2 * (size_t)N);
      h2d(s_fdlo.p + N, strm.log.chain_len.data(), 4 * (size_t)N);
      cons.fdtd_maxlen = s.maxlen;
      cons.fdtd_stale = true;
    } else if (fdt16())
      KLAUNCH((k_fd_transpose_ts<uint16_t>), dim3(N, div_up(N, 64), std::min(div_up(span, 64), 65535)), dim3(256),
              0, st, t, (const uint16_t*)d_FDT.p, s.qlo, len, (const int32_t*)s.cand_lo,
              (const int32_t*)s.cand_hi);
    else if (N > 16)
      KLAUNCH((k_fd_transpose_ts<int32_t>), dim3(N, div_up(N, 64), std::min(div_up(span, 64), 65535)), dim3(256),
              0, st, t, (const int32_t*)d_FDT.p, s.qlo, len, (const int32_t*)s.cand_lo,
              (const int32_t*)s.cand_hi);
    else
      KLAUNCH(k_transpose, dim3(div_up(span, 64), div_up(N, 64), N), dim3(256), 0, st, t, d_FDT.p,
              (int32_t*)nullptr, s.qlo, len, 1);
  }

  // ---------------- one batch of consensus calls ----------------
  // calls: event counts n_c (<= n_divided), ascending.
  // Host round trips: the fame-window coverage flags, the lowest candidate round
  // of an online batch, the segment count for N > 64, and one closing readback.
  // Control data goes up as one block (s_cctl, hge_plan::CtlLayout), results come back
  // as one block (s_out, hge_plan::ResultsLayout: counters, per-call counts, order).

  // how the order's stages were launched
  enum class OrderRan {
    Stages,     // every stage as its own grid
    CallFront,  // all of them in one block (k_order_call front = 1, or k_consensus_call)
    CallTail,   // the stage grids up to round received, then k_order_call front = 0
  };
  // what one batch's stages share
  struct Batch {
    const int64_t* calls = nullptr;
    int ncalls = 0;
    bool do_fame = false, do_order = false, commit = false;
    std::vector<int32_t>* order_out = nullptr;
    std::vector<int64_t>* counts_out = nullptr;
    // ---- the prologue's
    std::vector<int32_t> Rc;   // Rounds() at each call
    bool fresh_und = false;    // the candidates are every event of a fresh replay
    bool ord = false;          // there are candidates to order
    bool spl = false;          // a split part: the candidates of its own range
    int32_t* cand = nullptr;
    int ncand = 0;
    int rr_lo = 0, R_last = 0, nr = 0;  // the order pass examines rounds [rr_lo, rr_lo + nr)
    hge_plan::ResultsLayout out;
    // ---- decide_fame's
    hge_plan::FameWindows w;
    hge_plan::CtlLayout ctl;
    int64_t nslot = 0;
    bool hdr_done = false;  // the fame launch wrote the results header
    // every round's window reaches the last call (always so for one call: the online
    // path), so none can widen: the coverage flags stay on the device, and the new
    // LastConsensusRound comes back with the batch's closing readback
    bool lcr_dev = false;
    int lcr_new = -1, c_set = -1;  // !lcr_dev: the new LastConsensusRound and the call that set it
    bool lcr_up = false;
    // N <= 16: k_fame_call waits to run with the order (k_consensus_call)
    std::optional<FameCall> fame_pending;
    // ---- the order's
    SegInfo si{};
    OrderRan order_ran = OrderRan::Stages;
    bool wla_done = false;
    bool got_order = false;
    bool wrote_direct = false;  // the bucket sorts wrote the ids into the pinned order buffer
    bool split_done = false;
  };
  int32_t* out_counts() const { return s_out.p + hge_plan::ResultsLayout::kCounts; }
  int32_t* out_ids(const Batch& b) const { return s_out.p + b.out.ids; }
  unsigned long long* out_tx(const Batch& b) const { return (unsigned long long*)(s_out.p + b.out.o_tx); }
  int32_t* out_word(size_t k) const { return s_out.p + k; }
  // the new LastConsensusRound for the results header, when the device holds it
  const int32_t* lcr_src(const Batch& b) const { return b.lcr_dev ? (const int32_t*)(cons.c_flags + 1) : nullptr; }
  void out_init(const Batch& b) {
    const int nh = (int)b.out.header();
    KLAUNCH(k_out_init, dim3(div_up(nh, 256)), dim3(256), 0, st, s_out.p, nh, lcr_src(b));
  }
  // the control block's regions in s_cctl (host-built, or k_consensus_dyn's to fill)
  void bind_ctl(const hge_plan::CtlLayout& L) {
    cons.c_nc = (int64_t*)s_cctl.p;
    cons.c_Rc = s_cctl.p + L.Rc;
    cons.c_Lc = s_cctl.p + L.Lc;
    cons.c_flags = s_cctl.p + L.flags;
    cons.c_pr = s_cctl.p + L.pr;
    cons.c_pidx = s_cctl.p + L.pidx;
    cons.c_sgo = s_cctl.p + L.sgo;
  }

  void consensus_batch(const std::vector<int64_t>& calls, bool do_fame, bool do_order, bool commit,
                       std::vector<int32_t>* order_out, std::vector<int64_t>* counts_out) {
    if (calls.empty()) return;
    int64_t tp[5] = {now_ns(), 0, 0, 0, 0};
    Batch b;
    b.calls = calls.data();
    b.ncalls = (int)calls.size();
    b.do_fame = do_fame;
    b.do_order = do_order;
    b.commit = commit;
    b.order_out = order_out;
    b.counts_out = counts_out;
    prologue(b, calls);
    tp[1] = now_ns();
    decide_fame(b);
    tp[2] = now_ns();
    if (b.ord) {
      order_stages(b);
      bucket_and_sort(b);
    } else {  // nothing to order: the results header alone
      s_out.need(b.out.total());
      launch_pending_fame(b);
      if (!b.hdr_done) out_init(b);
    }
    if (b.fame_pending) throw Error(HGE_ERR_INTERNAL, "DecideFame's launch left pending");
    persist_fame(b);
    if (b.spl && b.got_order) {  // the parts' ordered slices, joined in call order
      split_commit(s_out.p, out_counts(), out_ids(b), b.out.ntxb, out_tx(b), order_out, counts_out);
      b.got_order = false;
      b.split_done = true;
    }
    fdtd_tail(b);
    tp[3] = now_ns();
    close_batch(b);
    tp[4] = now_ns();
    if (b.ncalls > 1000 && hge_hooks::host_phases()) phases_line(tp);
    prof.collect();
  }
  void phases_line(const int64_t* tp) const {
    fprintf(stderr, "[hge consensus] prologue %.3f ms, fame %.3f ms (incl. syncs), order enqueue %.3f ms, closing %.3f ms\n",
            (tp[1] - tp[0]) / 1e6, (tp[2] - tp[1]) / 1e6, (tp[3] - tp[2]) / 1e6, (tp[4] - tp[3]) / 1e6);
  }

  // R_c, the candidates and their lowest round, the order pass's rounds, the results layout
  void prologue(Batch& b, const std::vector<int64_t>& calls) {
    consensus_sync();  // (the results block is reused below)
    cons.x_iter = 0;
    b.Rc = hge_plan::rounds_at_calls(calls, cons.h_minw);
    b.fresh_und = cons.und_fresh;
    cons.und_fresh = false;
    b.ord = b.do_order && cons.n_und > 0;
    b.ncand = (int)cons.n_und;
    b.cand = d_und.p;
    // a split part's candidates: the events [cand_lo, its end) of the fresh list (identity)
    b.spl = split_on() && b.ord && b.fresh_und;
    if (b.spl) {
      b.cand = d_und.p + strm.sp.clo[strm.sp.part];
      b.ncand = (int)(strm.sp.a[strm.sp.part + 1] - strm.sp.clo[strm.sp.part]);
    }
    // lowest candidate round (a fresh replay's candidates include event 0, round 0)
    int32_t mnr = 0;
    const bool pre = cons.mnr_key[0] >= 0 && !b.spl && cons.n_divided == cons.mnr_key[2] &&
                     cons.n_und == cons.mnr_key[0] + (cons.mnr_key[2] - cons.mnr_key[1]);
    cons.mnr_key[0] = -1;
    if (b.ord && !b.fresh_und && pre) {
      mnr = cons.mnr_pre;
    } else if (b.ord && (!b.fresh_und || b.spl)) {
      h2d(s_small.p + 7, &kInf, 4);
      KLAUNCH(k_min_round, dim3(div_up(b.ncand, 256)), dim3(256), 0, st, d_round.p, b.cand, b.ncand,
              s_small.p + 7);
      readback(&mnr, s_small.p + 7, 1);
    }
    b.rr_lo = mnr + 1;
    // a split part's calls end at its last one: later rounds receive nothing it commits
    b.R_last = b.spl ? b.Rc[strm.sp.cb[strm.sp.part + 1] - 1] : b.Rc[b.ncalls - 1];
    b.nr = b.ord ? std::max(0, b.R_last - b.rr_lo) : 0;
    // the results block's size is known before DecideFame: the single-call fame kernel
    // writes its header
    b.out = hge_plan::results_layout(b.ncalls, b.ord ? b.ncand : 0);
  }

  FameCall fame_call_args(const Batch& b, int32_t* hdr) const {
    const int nrounds = b.w.nrounds();
    FameCall f{};
    f.pr_round = cons.c_pr;
    f.pr_off = cons.c_pr + nrounds;
    f.pr_cf = cons.c_pr + 2 * nrounds;
    f.pr_len = cons.c_pr + 3 * nrounds;
    f.nrounds = nrounds;
    f.npairs = b.w.npairs;
    f.nc = cons.c_nc;
    f.Rc = cons.c_Rc;
    f.dec = s_dec.p;
    f.decbit = s_decbit.p;
    f.Lc = cons.c_Lc;
    f.ncalls = b.ncalls;
    f.lcr_start = cons.lcr;
    f.LCR = s_LCR.p;
    f.clast = s_clast.p;
    f.flags = cons.c_flags;
    f.out = hdr;
    f.nout = (int)b.out.header();
    return f;
  }

  // DecideFame's single-block launch that waited for the order's, on its own after all
  void launch_pending_fame(Batch& b) {
    if (!b.fame_pending) return;
    KLAUNCH((k_fame_call<16, 1, true>), dim3(1), dim3(1024), 0, st, tables(), *b.fame_pending);
    b.fame_pending.reset();
  }

  // DecideFame: plan the (round, call) windows on the host, upload the control block,
  // decide, scan for the new LastConsensusRound; widen and go again while a round stays
  // undecided past its window.
  // Speculative fame window: calls up to R_c <= i + 2 + SPEC, widened when a round
  // stays undecided past it (narrower windows re-dispatch more often: slower).
  // Selective widening (N >= 192 a multiple of 64, no split or record; smaller N pay
  // more for the passes' round trips than the fame work they save): every window starts
  // at SPEC = 1 and only the rounds whose decision came past their window are
  // widened and re-decided (their new pairs alone; the other rounds' decisions are
  // moved to the new layout).  At 256/10M 517 of 2,836 rounds go to SPEC = 2 and 6
  // of those to 4; a uniform SPEC = 3 decides twice the pairs.
  void decide_fame(Batch& b) {
    const Tables t = tables();
    const int ncalls = b.ncalls;
    b.lcr_new = cons.lcr;
    const bool selective = b.do_fame && N % 64 == 0 && N >= 192 && !split_on() && !rec_on && ncalls > 1;
    std::vector<int> spec_r;
    hge_plan::FameWindows old;  // a widening pass: the layout it widens
    for (int SPEC = selective ? 1 : 3, iter = 0;; SPEC *= 2, iter++) {
      // a widening pass keeps the calls, R_c and their offsets (the round set is the
      // same): only the window arrays are rewritten and uploaded, L_c and the flags are
      // reset on the device (k_dec_relayout)
      const bool widening = selective && iter > 0;
      if (!b.do_fame) b.w = hge_plan::FameWindows();
      else if (widening) b.w = hge_plan::plan_fame_windows(b.Rc, cons.lcr, spec_r);
      else b.w = hge_plan::plan_fame_windows(b.Rc, cons.lcr, SPEC);
      if (selective && iter == 0) spec_r.assign(b.w.nrounds(), SPEC);
      const hge_plan::FameWindows& w = b.w;
      const int nrounds = w.nrounds(), npairs = w.npairs;
      b.ctl = hge_plan::ctl_layout(ncalls, nrounds, b.nr);
      b.nslot = hge_plan::fill_ctl(h_cctl, b.ctl, b.calls, b.Rc, w, b.rr_lo, N, widening);
      if (widening) {
        h2d(s_cctl.p + b.ctl.pr, h_cctl.data() + b.ctl.pr, 4 * (b.ctl.total - b.ctl.pr));
      } else {
        s_cctl.need(b.ctl.total);
        h2d(s_cctl.p, h_cctl.data(), 4 * b.ctl.total);
      }
      bind_ctl(b.ctl);
      if (nrounds == 0) break;
      if (!widening) s_dec.need((size_t)npairs * N);  // (a widening moves them first)
      s_decbit.need(npairs);
      s_LCR.need(ncalls);
      s_clast.need(nrounds);
      bool full = true;
      for (int k = 0; k < nrounds && full; k++) full = w.cf[k] + w.len[k] == ncalls;
      // one call at N < 64 (an online call): decide, timeline, LCR and the results
      // header in one single-block launch (their grids were a block or two each)
      const int Gf = group_lanes();
      const bool one = ncalls == 1 && full && !split_on() && !rec_on && (int64_t)nrounds * Gf <= 8192;
      if (one && N >= 64) {
        // the pairs by k_fame_decide_blk, then the timeline, LCR and the results header
        // in one single-block launch (in place of k_fame_timeline_g, k_lcr_scan, k_out_init)
        s_out.need(b.out.total());
        fame_decide(t, w, npairs, false);
        const FameCall fc = fame_call_args(b, s_out.p);
        KLAUNCH_NW(NW, NW_PATC, k_fame_call, 64, false, dim3(1), dim3(1024), 0, st, t, fc);
        b.hdr_done = true;
        cons.x_iter++;
        b.lcr_dev = true;
        break;
      }
      if (one && N < 64 && (int64_t)npairs * N <= 8192) {
        s_out.need(b.out.total());
        b.fame_pending = fame_call_args(b, s_out.p);
        // G = 16: launched with the order's stages when they run as one block (k_consensus_call)
        if (Gf == 32) {
          KLAUNCH((k_fame_call<32, 1, true>), dim3(1), dim3(1024), 0, st, t, *b.fame_pending);
          b.fame_pending.reset();
        } else if (Gf == 64) {
          KLAUNCH((k_fame_call<64, 1, true>), dim3(1), dim3(1024), 0, st, t, *b.fame_pending);
          b.fame_pending.reset();
        }
        b.hdr_done = true;
        cons.x_iter++;
        b.lcr_dev = true;
        break;
      }
      if (widening) {
        widen_decisions(t, old, w, ncalls);
        // the timeline over the whole layout again
        fame_decide(t, w, 0);
      } else {
        fame_decide(t, w, npairs);
      }
      if (rec_on && !split_on()) {
        rec_dec.emplace_back((size_t)npairs * N);
        readback(rec_dec.back().data(), s_dec.p, (size_t)npairs * N);
      }
      cons.x_iter++;
      s_rfail.need(nrounds);
      KLAUNCH(k_lcr_scan, dim3(1), dim3(1024), 0, st, cons.c_Lc, ncalls, cons.lcr, s_LCR.p, cons.c_pr,
              cons.c_pr + 2 * nrounds, cons.c_pr + 3 * nrounds, nrounds, s_clast.p, cons.c_flags,
              selective ? s_rfail.p : (int32_t*)nullptr);
      if (full) {
        b.lcr_dev = true;
        break;
      }
      int32_t fl[3];
      std::vector<int32_t> rf(selective ? nrounds : 0);
      if (selective) d2h(rf.data(), s_rfail.p, 4 * (size_t)nrounds);
      readback(fl, cons.c_flags, 3);
      if (fl[0]) {  // a round stayed undecided past its window: widen (those rounds only)
        if (selective) {
          for (int k = 0; k < nrounds; k++)
            if (rf[k]) spec_r[k] *= 2;
          old = std::move(b.w);
        }
        continue;
      }
      b.lcr_new = fl[1];
      if (b.lcr_new > cons.lcr) b.c_set = fl[2];
      break;
    }
  }
  // a selective widening pass: the previous layout's decisions moved into the new one,
  // then the widened rounds' new pairs decided
  void widen_decisions(const Tables& t, const hge_plan::FameWindows& old, const hge_plan::FameWindows& w, int ncalls) {
    const int nrounds = w.nrounds();
    s_dec2.need((size_t)w.npairs * N);
    std::vector<int32_t> rel(2 * (size_t)nrounds);
    std::vector<int32_t> plist;
    for (int k = 0; k < nrounds; k++) {
      rel[k] = old.off[k];
      rel[nrounds + k] = old.len[k];
      for (int q = old.len[k]; q < w.len[k]; q++) plist.push_back(w.off[k] + q);
    }
    s_relay.need(rel.size() + plist.size() + 1);
    h2d(s_relay.p, rel.data(), 4 * rel.size());
    if (!plist.empty()) h2d(s_relay.p + rel.size(), plist.data(), 4 * plist.size());
    KLAUNCH(k_dec_relayout, dim3(nrounds), dim3(256), 0, st, (const uint8_t*)s_dec.p, s_dec2.p,
            (const int32_t*)s_relay.p, (const int32_t*)(s_relay.p + nrounds), (const int32_t*)(cons.c_pr + nrounds),
            N, cons.c_Lc, ncalls, cons.c_flags);
    std::swap(s_dec, s_dec2);
    if (!plist.empty())
      KLAUNCH_NW(NW, NW_PT, k_fame_decide_blk, dim3((unsigned)plist.size()), dim3(N), 0, st, t, cons.c_pr,
                 cons.c_pr + nrounds, cons.c_pr + 2 * nrounds, nrounds, 0, w.npairs, cons.c_nc, cons.c_Rc, s_dec.p,
                 (const int32_t*)(s_relay.p + rel.size()));
  }

  // the single-block order kernel's arguments (k_order_call, k_consensus_call, and
  // k_consensus_dyn, which fills the round scalars and control pointers itself), with
  // the scratch they name
  OrderCall order_call(const Batch& b, int front) {
    const int ncalls = b.ncalls, ncand = b.ncand;
    s_recv.need(ncand);
    s_rr.need(ncand);
    s_cts.need(ncand);
    s_fund.need(ncand);
    s_upos.need(ncand);
    s_bpos.need(2 * (size_t)ncalls + 2);
    s_und2.need(d_und.n);
    s_keys.need((size_t)ncand * sizeof(OKey));
    s_keys2.need((size_t)ncand * sizeof(OKey));
    OrderCall oc{};
    oc.si = b.si;
    oc.rr_lo = b.rr_lo;
    oc.nr = b.nr;
    oc.segoff = cons.c_sgo;
    oc.segcnt = s_segcnt.p;
    oc.seg_call = s_segcall.p;
    oc.seg_round = s_seground.p;
    oc.seg_dec = s_segdec.p;
    oc.seg_fws = s_segfws.p;
    oc.theta = s_theta.p;
    oc.cand = b.cand;
    oc.ncand = ncand;
    oc.R_last = b.R_last;
    oc.recv = s_recv.p;
    oc.rr = s_rr.p;
    oc.cts = s_cts.p;
    oc.cnt = out_counts();
    oc.bpos = s_bpos.p;
    oc.total = out_word(hge_plan::ResultsLayout::kReceived);
    oc.blist = s_bpos.p + ncalls;
    oc.nblist = s_bpos.p + 2 * ncalls;
    oc.f_und = s_fund.p;
    oc.upos = s_upos.p;
    oc.nund = out_word(hge_plan::ResultsLayout::kUndetermined);
    oc.und_out = s_und2.p;
    oc.k1 = (OKey*)s_keys.p;
    oc.k2 = (OKey*)s_keys2.p;
    oc.ev_rr = d_rr.p;
    oc.ev_cts = d_cts.p;
    oc.ntx = out_tx(b);
    oc.ntxb = b.out.ntxb;
    oc.ids = out_ids(b);
    oc.pr = cons.c_pr;
    oc.nrounds = b.do_fame ? b.w.nrounds() : 0;
    oc.clast = s_clast.p;
    oc.dec = s_dec.p;
    oc.nc = cons.c_nc;
    oc.flags = cons.c_flags;
    oc.lcr_old = cons.lcr;
    oc.n_lo = (int)std::min<int64_t>(b.calls[0], cons.n_coords);
    oc.n1 = (int)cons.n_coords;
    oc.lcre_out = out_word(hge_plan::ResultsLayout::kLcrEvents);
    oc.front = front;
    oc.sort = sort_ctl();
    return oc;
  }

  // the frontier rows transposed (WLA) for the batch's rounds: theta (N > 64) and the
  // median (N > 16) read them
  void ensure_wla(Batch& b) {
    if (b.wla_done || N <= 16 || b.R_last <= b.rr_lo) return;
    b.wla_done = true;
    d_WLA.need((size_t)Rcap * N * N);
    if (N > 64 && !strm.wide32) d_WLR.need((size_t)Rcap * N * N);
    const Tables tw = tables();
    KLAUNCH(k_witness_la, dim3(div_up(N, 64), div_up(N, 64), b.R_last - b.rr_lo), dim3(256), 0, st, tw, b.rr_lo);
  }

  // DecideRoundReceived: visibility, the rounds' segments with theta, round received and
  // the median as their own grids -- or all of it and the rest of the order in one
  // block (k_order_call / k_consensus_call: an online call at N <= 16).  Leaves s_recv.
  void order_stages(Batch& b) {
    const int ncalls = b.ncalls, ncand = b.ncand, nr = b.nr, nrounds = b.w.nrounds();
    s_out.need(b.out.total());
    // an online call at N <= 16: the order's stages in one single-block launch
    // (k_order_call: segments, round received with its median, the call's bucket, the
    // undetermined list, keys, the sort, the persisted fame), with DecideFame's block
    // in front when it waited (k_consensus_call)
    const bool ocall = nr > 0 && ncalls == 1 && b.calls[0] >= cons.n_coords && b.commit && N <= 16 && !b.spl &&
                       ncand <= SCAN_LDS && (int64_t)nr * group_lanes() <= 65536 && (nrounds == 0 || b.lcr_dev) &&
                       !hge_hooks::no_order_call();
    if (!ocall) launch_pending_fame(b);
    if (nr == 0) {
      // the results header zeroed, with the new LastConsensusRound when the device holds
      // it (one launch in place of a memset and a copy)
      if (!b.hdr_done) out_init(b);
      s_recv.need(ncand);
      HGE_HIPCHK(hipMemsetAsync(s_recv.p, 0xFF, 4 * ncand, st));
      return;
    }
    SegInfo& si = b.si;
    si.pr_index = cons.c_pidx;
    if (nrounds > 0) {
      si.pr_off = cons.c_pr + nrounds;
      si.pr_cf = cons.c_pr + 2 * nrounds;
      si.pr_len = cons.c_pr + 3 * nrounds;
      si.clast = s_clast.p;
      si.dec = s_dec.p;
    }
    s_segcnt.need(nr);
    // first call at which each event is visible (arrivals, round received); one call
    // that sees every event (an online call) needs no table: 0 for all, and the
    // header is zeroed alone (a table of every event per call grew with the stream)
    cons.vis_all = ncalls == 1 && b.calls[0] >= cons.n_coords;
    if (cons.vis_all) {
      if (!b.hdr_done) out_init(b);
    } else {  // (the header's zeroing folded into k_visibility's launch)
      const int nh = (int)b.out.header();
      s_vis.need(std::max<int64_t>(cons.n_coords, 1));
      KLAUNCH(k_visibility, dim3(div_up(cons.n_coords, 256) + div_up(nh, 256)), dim3(256), 0, st,
              (const int64_t*)cons.c_nc, ncalls, (int)cons.n_coords, s_vis.p, s_out.p, nh, lcr_src(b));
    }
    const int32_t* visp = cons.vis_all ? (const int32_t*)nullptr : (const int32_t*)s_vis.p;
    // one pass into per-round capacity slots (no count round trip); theta inline
    // for N <= 64, by k_seg_theta_wide past it
    const size_t ns = (size_t)std::max<int64_t>(b.nslot, 1);
    s_segcall.need(ns);
    s_seground.need(ns);
    s_segdec.need(ns);
    s_segfws.need(ns * NW);
    s_theta.need(ns * N);
    cons.segoff_p = cons.c_sgo;
    if (ocall) {
      const OrderCall oc = order_call(b, 1);
      if (b.fame_pending) {
        KLAUNCH(k_consensus_call<16>, dim3(1), dim3(1024), 0, st, tables(), *b.fame_pending, oc);
        b.fame_pending.reset();
      } else {
        KLAUNCH(k_order_call<16>, dim3(1), dim3(1024), 0, st, tables(), oc);
      }
      std::swap(d_und, s_und2);
      b.got_order = true;
      b.order_ran = OrderRan::CallFront;
      if (hge_hooks::seg_debug()) seg_debug(b);
      return;
    }
    ensure_wla(b);
    const Tables t = tables();
    const int G = group_lanes();
    const dim3 sgrid(div_up((int64_t)nr * G, 256));
    const int32_t* sgo = cons.c_sgo;
    if (G == 16) {
      KLAUNCH((k_segments_1p<16, 1>), sgrid, dim3(256), 0, st, t, b.rr_lo, nr, ncalls, visp, si, sgo, s_segcnt.p,
              s_segcall.p, s_seground.p, s_segdec.p, s_segfws.p, s_theta.p);
    } else if (G == 32) {
      KLAUNCH((k_segments_1p<32, 1>), sgrid, dim3(256), 0, st, t, b.rr_lo, nr, ncalls, visp, si, sgo, s_segcnt.p,
              s_segcall.p, s_seground.p, s_segdec.p, s_segfws.p, s_theta.p);
    } else {
      KLAUNCH_NW(NW, NW_PAT, k_segments_1p, 64, sgrid, dim3(256), 0, st, t, b.rr_lo, nr, ncalls, visp, si, sgo,
                 s_segcnt.p, s_segcall.p, s_seground.p, s_segdec.p, s_segfws.p, s_theta.p);
    }
    if (NW > 1 && strm.wide32) {
      KLAUNCH_NW2(NW, NW_T, k_seg_theta32, dim3(std::min(nr, 4096)), dim3(256), 0, st, t,
                  (const int32_t*)s_seground.p, (const int32_t*)cons.c_sgo, (const int32_t*)s_segcnt.p, nr,
                  (const uint64_t*)s_segfws.p, s_theta.p);
    } else if (NW > 1) {
      KLAUNCH_NW2(NW, NW_T, k_seg_theta_wide, dim3(std::min(nr, 4096), nr < 64 ? 8 : 2), dim3(1024), 0, st, t,
                  (const int32_t*)s_seground.p, (const int32_t*)cons.c_sgo, (const int32_t*)s_segcnt.p, nr,
                  (const uint64_t*)s_segfws.p, s_theta.p, dbg_p());
    }
    if (hge_hooks::seg_debug()) seg_debug(b);
    // round-received per candidate
    s_recv.need(ncand);
    s_rr.need(ncand);
    s_cts.need(ncand);
    recv_dispatch(b);
  }
  // diagnostics (HGE_SEG_DEBUG): the segments theta walks this batch
  void seg_debug(const Batch& b) {
    std::vector<int32_t> sc(b.nr);
    readback(sc.data(), s_segcnt.p, b.nr);
    int tot = 0, mx = 0;
    for (int v : sc) {
      tot += v;
      mx = std::max(mx, v);
    }
    fprintf(stderr, "[hge seg] calls %d rounds %d segments %d max per round %d\n", b.ncalls, b.nr, tot, mx);
    if (dbg_on && s_dbg.p) {
      uint64_t v[16];
      readback(v, s_dbg.p, 16);
      fprintf(stderr, "[hge theta] segments %llu cycles: rows %llu staging %llu bisection %llu\n",
              (unsigned long long)v[15], (unsigned long long)v[12], (unsigned long long)v[13],
              (unsigned long long)v[14]);
    }
  }

  // FindOrder from s_recv on: (a split part's filter,) the received events into their
  // calls' buckets, keys, the sorts, the new undetermined list -- or one call's bucket,
  // list, keys, sort and persisted fame as one single-block launch at any N
  // (k_order_call, front = 0) when the order's first stages ran as their own grids.
  // The received count stays on the device (the results header).
  void bucket_and_sort(Batch& b) {
    const int ncalls = b.ncalls, ncand = b.ncand;
    int32_t* const cand = b.cand;
    const Tables t = tables();
    if (b.spl) {  // keep what this part's calls receive (k_split_filter)
      const int p = strm.sp.part;
      const int32_t guard = p + 1 < strm.sp.nparts ? (int32_t)strm.sp.clo[p + 1] : INT32_MIN;
      HGE_HIPCHK(hipMemsetAsync(s_small.p + 8, 0, 4, st));
      KLAUNCH(k_split_filter, dim3(div_up(ncand, 256)), dim3(256), 0, st, (const int32_t*)cand, ncand,
              s_recv.p, strm.sp.cb[p], strm.sp.cb[p + 1] - 1, guard, s_small.p + 8);
    }
    if (b.order_ran == OrderRan::CallFront) return;
    const bool tail_ok = b.commit && ncalls == 1 && !b.spl && ncand <= SCAN_LDS &&
                         (!b.do_fame || b.w.nrounds() == 0 || b.lcr_dev) && !hge_hooks::no_order_call();
    if (tail_ok) {
      const OrderCall oc = order_call(b, 0);
      KLAUNCH(k_order_call<16>, dim3(1), dim3(1024), 0, st, t, oc);
      std::swap(d_und, s_und2);
      b.got_order = true;
      b.order_ran = OrderRan::CallTail;
      return;
    }
    int32_t* const o_cnt = s_out.p;  // the results header: received [0], undetermined [1]
    int32_t* const o_cc = out_counts();
    int32_t* const o_und = out_word(hge_plan::ResultsLayout::kUndetermined);
    s_fund.need(ncand);
    s_upos.need(ncand);
    s_rr.need(ncand);
    s_cts.need(ncand);
    // an online call's flags, buckets and undetermined list: one launch (k_recv_list_und below)
    const bool rlu = b.commit && ncand <= 16384 && ncalls <= 8;
    if (!rlu)
      KLAUNCH(k_recv_flags, dim3(div_up(ncand, 256)), dim3(256), 0, st, s_recv.p, ncand,
              (int32_t*)nullptr, s_fund.p, b.commit ? 1 : 0, b.commit ? o_cc : (int32_t*)nullptr);
    if (!b.commit) {
      KLAUNCH(k_set_rr, dim3(div_up(ncand, 256)), dim3(256), 0, st, t, cand, ncand, s_recv.p,
              s_rr.p, s_cts.p, d_rr.p, d_cts.p, (unsigned long long*)out_word(hge_plan::ResultsLayout::kTx), 0);
      return;
    }
    s_bpos.need(2 * (size_t)ncalls + 2);
    int32_t* blist = s_bpos.p + ncalls;     // non-empty buckets
    int32_t* nblist = s_bpos.p + 2 * ncalls;  // their count
    // a small candidate set: the undetermined list's scan and scatter ride with the
    // call buckets (k_list_und; the list swap below is the same)
    const bool lu = ncand <= 16384;
    s_und2.need(d_und.n);
    if (rlu)
      KLAUNCH(k_recv_list_und, dim3(2), dim3(1024), 0, st, (const int32_t*)s_recv.p, (int)ncand, o_cc, ncalls,
              s_bpos.p, o_cnt, blist, nblist, s_fund.p, s_upos.p, o_und, cand, s_und2.p);
    else if (lu)
      KLAUNCH(k_list_und, dim3(2), dim3(1024), 0, st, (const int32_t*)o_cc, ncalls, s_bpos.p, o_cnt, blist,
              nblist, (const int32_t*)s_fund.p, s_upos.p, (int)ncand, o_und, cand, s_und2.p);
    else
      KLAUNCH(k_bucket_list, dim3(1), dim3(1024), 0, st, (const int32_t*)o_cc, ncalls, s_bpos.p,
              o_cnt, blist, nblist);
    s_keys.need((size_t)ncand * sizeof(OKey));
    s_keys2.need((size_t)ncand * sizeof(OKey));
    OKey* k1 = (OKey*)s_keys.p;
    OKey* k2 = (OKey*)s_keys2.p;
    KLAUNCH(k_bucket_keys, dim3(div_up(ncand, 256)), dim3(256), 0, st, t, cand, ncand, s_recv.p,
            s_rr.p, s_cts.p, s_bpos.p, k1, d_rr.p, d_cts.p, out_tx(b));
    // a replay's sorts write the order straight into the pinned order buffer (host
    // memory mapped into the device: the writes cross PCIe while the later buckets
    // sort; no copy after the replay)
    int32_t* ids_dst = out_ids(b);
    if (cons.lazy_order && !b.order_out && !b.spl && pin_ord_dev) {
      ids_dst = pin_ord_dev;
      b.wrote_direct = true;
    }
    sort_counted = false;
    if (ncalls <= 8) {
      // a few buckets (an online call): one launch, each bucket to the path its size takes
      KLAUNCH(k_bucket_sort_all, dim3(ncalls), dim3(1024), 0, st, (const int32_t*)s_bpos.p,
              (const int32_t*)o_cc, (const int32_t*)blist, (const int32_t*)nblist, k1, k2, ids_dst, sort_ctl());
    } else {
      // buckets of 513 .. 2 * BIG_SORT keys in LDS (k_bucket_sort_big), the rest here
      KLAUNCH(k_bucket_sort, dim3(std::min(ncalls, 2048)), dim3(256), 0, st,
              (const int32_t*)s_bpos.p, (const int32_t*)o_cc, (const int32_t*)blist,
              (const int32_t*)nblist, k1, k2, ids_dst, 1);
      if (ncand > 512)  // (no bucket past 512 keys otherwise)
        KLAUNCH(k_bucket_sort_big, dim3(std::min(ncalls, n_cu())), dim3(1024), 0, st,
                (const int32_t*)s_bpos.p, (const int32_t*)o_cc, (const int32_t*)blist,
                (const int32_t*)nblist, (const OKey*)k1, k2, ids_dst, sort_ctl());
    }
    // new undetermined list (in candidate order), scattered into the spare list
    // (same capacity) and swapped: no device copy
    if (!lu) {
      scan_large(s_fund.p, s_upos.p, ncand, o_und);
      KLAUNCH(k_scatter_und, dim3(div_up(ncand, 256)), dim3(256), 0, st, cand, ncand, s_fund.p, s_upos.p,
              s_und2.p);
    }
    std::swap(d_und, s_und2);
    b.got_order = true;
  }

  // the decided rounds' fame into the tables, and RoundEvents(LCR - 1) (k_order_call
  // did both when it ran)
  void persist_fame(Batch& b) {
    const int nrounds = b.w.nrounds();
    if (!b.do_fame || nrounds == 0 || b.order_ran != OrderRan::Stages) return;
    const Tables t = tables();
    int32_t* const lcre_out = out_word(hge_plan::ResultsLayout::kLcrEvents);
    if (b.lcr_dev) {
      // the persisted fame and RoundEvents(LCR - 1) as below (the new LCR and its
      // call read on the device) in one launch
      const int64_t nfrom = std::min<int64_t>(b.calls[0], cons.n_coords);
      const int nb_fp = (int)div_up((int64_t)nrounds * N, 256);
      KLAUNCH(k_fame_persist_lcre, dim3(nb_fp + std::max(1, div_up(cons.n_coords - nfrom, 256))), dim3(256), 0, st, t,
              (const int32_t*)cons.c_pr, (const int32_t*)(cons.c_pr + nrounds), (const int32_t*)(cons.c_pr + 2 * nrounds),
              (const int32_t*)(cons.c_pr + 3 * nrounds), nrounds, (const int32_t*)s_clast.p, (const uint8_t*)s_dec.p,
              nb_fp, (const int64_t*)cons.c_nc, (const int32_t*)cons.c_flags, cons.lcr, (int)nfrom, (int)cons.n_coords, lcre_out);
      return;
    }
    fame_persist(t, nrounds);
    if (b.lcr_new > cons.lcr) {
      // RoundEvents(lcr_new - 1) at call c_set: events of that round minus the
      // ones inserted after that call
      b.lcr_up = true;
      const int r = b.lcr_new - 1;
      if (r >= 0) {
        const int64_t nfrom = std::min<int64_t>(b.calls[b.c_set], cons.n_coords);
        KLAUNCH(k_lcre, dim3(std::max(1, div_up(cons.n_coords - nfrom, 256))), dim3(256), 0, st, t,
                (int)nfrom, (int)cons.n_coords, r, lcre_out);
      }
    }
  }

  // what a results block says, into the host state: the log (unless the ids were
  // delivered to the pinned order buffer), ConsensusTransactions, the undetermined count
  void commit_order(const hge_plan::Results& r, int ncalls, bool to_log, std::vector<int32_t>* order_out,
                    std::vector<int64_t>* counts_out) {
    if (to_log) cons.consensus.insert(cons.consensus.end(), r.ids, r.ids + r.nrecv);
    cons.ctx += (int64_t)r.ntx;
    if (order_out) order_out->insert(order_out->end(), r.ids, r.ids + r.nrecv);
    if (counts_out)
      for (int c = 0; c < ncalls; c++) counts_out->push_back(r.counts[c]);
    cons.n_und = r.n_und;
  }
  void commit_lcr(int lcr_new, int lcr_events) {
    cons.lcr = lcr_new;
    cons.lcre = lcr_new - 1 >= 0 ? lcr_events : 0;
  }

  // hge_commit_records: entries [from, from + m) of the log (the vector, then the tail a
  // replay left in the pinned order buffer) as records, a read of persisted state
  // (hge_commit.hip).  Chunks of at most kRecordsChunk records, each one launch and one
  // wait: the device scratch and the arena's pieces are a chunk's, whatever the log's length.
  // A chunk's ids from the vector go up through the arena; the pinned tail is copied from
  // where it lies.  Nothing runs on the device for the ids alone.
  static constexpr int64_t kRecordsChunk = 1 << 20;
  void commit_records(int64_t from, int64_t m, int32_t* ids_out, int32_t* rr_out, int64_t* cts_out, int32_t* src_out) {
    const int64_t V = (int64_t)cons.consensus.size();
    auto host_ids = [&](int64_t a, int64_t k, auto&& piece) {  // [a, a + k) as its (at most two) pieces
      const int64_t kv = std::max<int64_t>(0, std::min(a + k, V) - a);
      if (kv > 0) piece((int64_t)0, cons.consensus.data() + a, kv, false);
      if (k > kv) piece(kv, (const int32_t*)pin_ord.p + (a + kv - V), k - kv, true);
    };
    if (ids_out)
      host_ids(from, m, [&](int64_t at, const int32_t* p, int64_t k, bool) { memcpy(ids_out + at, p, 4 * (size_t)k); });
    if (!rr_out && !cts_out && !src_out) return;
    const int64_t CH = hge_hooks::test_records_chunk(kRecordsChunk);
    for (int64_t a = from; a < from + m; a += CH) {
      const int k = (int)std::min<int64_t>(CH, from + m - a);
      s_rec.need(3 * (size_t)k);  // cts[k] | ids[k] rr[k] | src[k] ...
      int64_t* const d_c = s_rec.p;
      int32_t* const d_i = (int32_t*)(s_rec.p + k);
      int32_t *const d_r = d_i + k, *const d_s = d_i + 2 * (size_t)k;
      // the chunk's pieces of the arena in one go: no drain between them (a call's records
      // cost one host wait)
      xfer.reserve(((4 * (size_t)k + 255) & ~(size_t)255) * (1 + (rr_out ? 1 : 0) + (src_out ? 1 : 0)) +
                   (cts_out ? (8 * (size_t)k + 255) & ~(size_t)255 : 0));
      host_ids(a, k, [&](int64_t at, const int32_t* p, int64_t kk, bool pinned) {
        if (pinned) {  // (already pinned: the copy waits for nothing)
          hp.copies++;
          HGE_HIPCHK(hipMemcpyAsync(d_i + at, p, 4 * (size_t)kk, hipMemcpyHostToDevice, st));
        } else {
          h2d(d_i + at, p, 4 * (size_t)kk);
        }
      });
      int32_t* const rr_o = rr_out ? d_r : nullptr;
      int64_t* const cts_o = cts_out ? d_c : nullptr;
      if (!src_out) {
        KLAUNCH(k_commit_records_plain, dim3((unsigned)div_up(k, 256)), dim3(256), 0, st, (const int32_t*)d_i, k,
                (const int32_t*)d_rr.p, (const int64_t*)d_cts.p, rr_o, cts_o);
      } else {
#define HGE_RECORDS(G)                                                                                        \
  KLAUNCH(k_commit_records<G>, dim3((unsigned)div_up(k, 256 / G)), dim3(256), 0, st, tables(), (const int32_t*)d_i, k, \
          (const int32_t*)d_rr.p, (const int64_t*)d_cts.p, rr_o, cts_o, d_s)
        // a record's lane group: min(64, the next power of two >= N)
        if (N > 32) HGE_RECORDS(64);
        else if (N > 16) HGE_RECORDS(32);
        else if (N > 8) HGE_RECORDS(16);
        else if (N > 4) HGE_RECORDS(8);
        else if (N > 2) HGE_RECORDS(4);
        else if (N > 1) HGE_RECORDS(2);
        else HGE_RECORDS(1);
#undef HGE_RECORDS
      }
      const int64_t o = a - from;
      if (rr_out) d2h(rr_out + o, d_r, 4 * (size_t)k);
      if (cts_out) d2h(cts_out + o, d_c, 8 * (size_t)k);
      if (src_out) d2h(src_out + o, d_s, 4 * (size_t)k);
      sync();
    }
    prof.collect();
  }

  // the batch's one closing round trip (read in place from the pinned arena); a
  // replay's order stays in HBM (lazy: counters, per-call counts and transaction sums only)
  void close_batch(Batch& b) {
    const bool lazy = b.got_order && cons.lazy_order && !b.order_out;
    const size_t off = d2h_pinned(s_out.p, 4 * (b.got_order && !lazy ? b.out.total() : b.out.header()));
    const size_t off_tx = lazy ? d2h_pinned(s_out.p + b.out.o_tx, 4 * 2 * (size_t)b.out.ntxb) : 0;
    sync();
    const int32_t* ho = (const int32_t*)xfer.at(off);
    const int32_t* htx = !b.got_order ? nullptr : lazy ? (const int32_t*)xfer.at(off_tx) : ho + b.out.o_tx;
    const hge_plan::Results r = hge_plan::parse_results(b.out, ho, htx);
    if (b.got_order) {
      if (lazy) {  // delivered into the pinned order buffer (sized at hge_replay_prepare)
        if ((size_t)r.nrecv > pin_ord.n) throw Error(HGE_ERR_INTERNAL, "order buffer below the ordered count");
        const int64_t td = now_ns();
        if (!b.wrote_direct && r.nrecv) {
          HGE_HIPCHK(hipMemcpyAsync(pin_ord.p, out_ids(b), 4 * (size_t)r.nrecv, hipMemcpyDeviceToHost, st));
          sync();
        }
        // the delivery's wall time after the sorts (hge_stage_times [5]; ~0 when written direct)
        stage_ms[5] = (float)((now_ns() - td) / 1e6);
        cons.cons_pin_n = r.nrecv;
      }
      commit_order(r, b.ncalls, !lazy, b.order_out, b.counts_out);
    } else if (b.do_order && b.counts_out && !b.split_done) {
      for (int c = 0; c < b.ncalls; c++) b.counts_out->push_back(0);
    }
    if (b.lcr_dev && r.lcr > cons.lcr) {
      b.lcr_up = true;
      b.lcr_new = r.lcr;
    }
    if (b.lcr_up) commit_lcr(b.lcr_new, r.lcr_events);
  }

  // split replay: the parts' fame decisions (each part's pairs [P0, P1)) all-gathered
  void split_exchange_dec(const std::vector<int32_t>& pr_round, const std::vector<int32_t>& pr_off, int npairs) {
    const int G = strm.sp.nparts, nr = (int)pr_round.size();
    std::vector<int64_t> P0(G), P1(G);
    int64_t mx = 1;
    for (int g = 0; g < G; g++) {
      int klo = 0, khi = 0;
      split_rounds_of(g, pr_round, klo, khi);
      P0[g] = klo < nr ? pr_off[klo] : npairs;
      P1[g] = khi < nr ? pr_off[khi] : npairs;
      mx = std::max(mx, P1[g] - P0[g]);
    }
    const int64_t bytes = (mx * N + 255) / 256 * 256;
    uint8_t* buf = (uint8_t*)x_buf(bytes);
    const int p = strm.sp.part;
    if (P1[p] > P0[p])
      HGE_HIPCHK(hipMemcpyAsync(buf + (size_t)p * bytes, s_dec.p + (size_t)P0[p] * N, (size_t)(P1[p] - P0[p]) * N,
                            hipMemcpyDeviceToDevice, st));
    x_gather(bytes, buf);
    if (emulating()) {  // the other parts' decisions of this fame iteration, from the record
      const std::vector<uint8_t>& rd = rec_dec.at((size_t)cons.x_iter);
      for (int g = 0; g < G; g++)
        if (g != p && P1[g] > P0[g]) h2d(buf + (size_t)g * bytes, rd.data() + (size_t)P0[g] * N, (size_t)(P1[g] - P0[g]) * N);
    }
    for (int g = 0; g < G; g++)
      if (g != p && P1[g] > P0[g])
        HGE_HIPCHK(hipMemcpyAsync(s_dec.p + (size_t)P0[g] * N, buf + (size_t)g * bytes, (size_t)(P1[g] - P0[g]) * N,
                              hipMemcpyDeviceToDevice, st));
  }

  // split replay: this part's ordered slice (its calls' buckets, round received,
  // consensus timestamps, left candidates) all-gathered; every part then holds the
  // whole order, the per-call batches and the undetermined list (the last part's)
  void split_commit(const int32_t* o_cnt, const int32_t* o_cc, const int32_t* o_ids, int ntxb,
                    const unsigned long long* ntx_part, std::vector<int32_t>* order_out,
                    std::vector<int64_t>* counts_out) {
    const int G = strm.sp.nparts, p = strm.sp.part;
    int maxcalls = 0;
    int64_t cap = 1;
    for (int g = 0; g < G; g++) {
      maxcalls = std::max(maxcalls, strm.sp.cb[g + 1] - strm.sp.cb[g]);
      cap = std::max(cap, strm.sp.a[g + 1] - strm.sp.clo[g]);
    }
    const SplitSlot L = SplitSlot::make(maxcalls, cap);
    const int64_t bytes = 4 * L.words;
    int32_t* buf = (int32_t*)x_buf(bytes);
    KLAUNCH(k_split_pack, dim3(std::min(div_up(cap, 256), 4096)), dim3(256), 0, st, o_cnt, o_cc, strm.sp.cb[p],
            strm.sp.cb[p + 1] - strm.sp.cb[p], o_ids, (const int32_t*)d_und.p, (const int32_t*)d_rr.p,
            (const int64_t*)d_cts.p, ntx_part, ntxb, (const int32_t*)(s_small.p + 8), L,
            buf + (size_t)p * L.words);
    x_gather(bytes, buf);
    if (emulating()) {  // the other parts' slots from the record
      int64_t off0 = 0;
      for (int g = 0; g < G; g++) {
        int64_t nord = 0;
        for (int c = strm.sp.cb[g]; c < strm.sp.cb[g + 1]; c++) nord += rec_counts[c];
        if (g != p) {
          const bool last = g == G - 1;
          std::vector<int32_t> sl((size_t)L.words, 0);
          unsigned long long tx = 0;
          for (int64_t i = 0; i < nord; i++) {
            const int32_t x = rec_order[off0 + i];
            sl[L.ids + i] = x;
            sl[L.rr + i] = rec_rr[x];
            memcpy(&sl[L.cts + 2 * i], &rec_cts[x], 8);
            tx += (unsigned long long)strm.log.h_ntx[x];
          }
          const int64_t nleft = last ? (int64_t)rec_left.size() : 0;
          for (int64_t i = 0; i < nleft; i++) sl[L.left + i] = rec_left[i];
          for (int c = strm.sp.cb[g]; c < strm.sp.cb[g + 1]; c++) sl[L.counts + (c - strm.sp.cb[g])] = (int32_t)rec_counts[c];
          sl[0] = (int32_t)nord;
          sl[1] = (int32_t)nleft;
          sl[4] = (int32_t)(uint32_t)tx;
          sl[5] = (int32_t)(uint32_t)(tx >> 32);
          h2d(buf + (size_t)g * L.words, sl.data(), 4 * (size_t)L.words);
        }
        off0 += nord;
      }
    }
    // every part's header and call counts
    std::vector<int32_t> hd((size_t)G * L.ids);
    for (int g = 0; g < G; g++) d2h(&hd[(size_t)g * L.ids], buf + (size_t)g * L.words, 4 * (size_t)L.ids);
    sync();
    std::vector<int64_t> off(G + 1, 0);
    bool bad = false;
    unsigned long long ntx = 0;
    for (int g = 0; g < G; g++) {
      const int32_t* h0 = &hd[(size_t)g * L.ids];
      bad = bad || h0[2] != 0;
      off[g + 1] = off[g] + h0[0];
      ntx += (unsigned long long)(uint32_t)h0[4] | ((unsigned long long)(uint32_t)h0[5] << 32);
    }
    if (bad) throw Error(HGE_ERR_SPLIT, "split replay: an event is received outside every part's range");
    const int64_t tot = off[G];
    s_sord.need((size_t)std::max<int64_t>(tot, 1));
    s_soff.need((size_t)G + 1);
    h2d(s_soff.p, off.data(), 8 * ((size_t)G + 1));
    KLAUNCH(k_split_unpack, dim3(std::min(div_up(cap, 256), 1024), G), dim3(256), 0, st, (const int32_t*)buf, L, G,
            (const int64_t*)s_soff.p, s_sord.p, d_rr.p, d_cts.p);
    // the undetermined list: the last part's left candidates
    const int nleft = hd[(size_t)(G - 1) * L.ids + 1];
    if (nleft > 0)
      HGE_HIPCHK(hipMemcpyAsync(d_und.p, buf + (size_t)(G - 1) * L.words + L.left, 4 * (size_t)nleft,
                            hipMemcpyDeviceToDevice, st));
    const size_t po = d2h_pinned(s_sord.p, 4 * (size_t)tot);
    sync();
    const int32_t* ids = (const int32_t*)xfer.at(po);
    cons.consensus.insert(cons.consensus.end(), ids, ids + tot);
    if (order_out) order_out->insert(order_out->end(), ids, ids + tot);
    cons.ctx += (int64_t)ntx;
    cons.n_und = nleft;
    if (counts_out)
      for (int g = 0; g < G; g++)
        for (int c = strm.sp.cb[g]; c < strm.sp.cb[g + 1]; c++) counts_out->push_back(hd[(size_t)g * L.ids + 8 + (c - strm.sp.cb[g])]);
  }

  void scan_large(const int32_t* in, int32_t* out, int n, int32_t* total) {
    if (n <= 16384) {  // one block (an online call's candidates): one launch, not three
      KLAUNCH(k_scan_small, dim3(1), dim3(1024), 0, st, in, out, n, total);
      return;
    }
    const int nb = div_up(n, 1024);
    s_part.need(2 * (size_t)nb + 2);
    KLAUNCH(k_scan_blocks, dim3(nb), dim3(256), 0, st, in, out, n, s_part.p);
    KLAUNCH(k_scan_small, dim3(1), dim3(1024), 0, st, s_part.p, s_part.p + nb, nb, total);
    KLAUNCH(k_scan_add, dim3(div_up(n, 256)), dim3(256), 0, st, out, n, s_part.p + nb);
  }

  // lanes per round in the group-scan kernels (a lane holds NW slots when N > 64)
  int group_lanes() const { return N <= 16 ? 16 : N <= 32 ? 32 : 64; }

  // the windows' pairs [.., npairs) decided (k_fame_decide; a split part: the pairs of
  // its rounds, then the parts' decisions all-gathered) and, with `timeline`, the
  // per-round timeline (else k_fame_call<.., false> takes it)
  void fame_decide(const Tables& t, const hge_plan::FameWindows& w, int npairs, bool timeline = true) {
    const int nrounds = w.nrounds();
    int win_lo = 0, win_hi = nrounds;
    if (split_on()) split_rounds_of(strm.sp.part, w.round, win_lo, win_hi);
    const int p0 = win_lo < nrounds ? w.off[win_lo] : npairs;
    const int p1 = win_hi < nrounds ? w.off[win_hi] : npairs;
    if (p1 > p0 && N == 64 * NW) {
      KLAUNCH_NW(NW, NW_PT, k_fame_decide_blk, dim3(p1 - p0), dim3(N), 0, st, t, cons.c_pr + win_lo,
                 cons.c_pr + nrounds + win_lo, cons.c_pr + 2 * nrounds + win_lo, win_hi - win_lo, p0, p1, cons.c_nc, cons.c_Rc, s_dec.p,
                 (const int32_t*)nullptr);
    } else if (p1 > p0) {
      KLAUNCH_NW(NW, NW_PT, k_fame_decide, dim3(div_up((p1 - p0) * N, 256)), dim3(256), 0, st, t, cons.c_pr + win_lo,
                 cons.c_pr + nrounds + win_lo, cons.c_pr + 2 * nrounds + win_lo, win_hi - win_lo, p0, p1, cons.c_nc, cons.c_Rc, s_dec.p);
    }
    if (split_on()) split_exchange_dec(w.round, w.off, npairs);
    if (!timeline) return;
    const int G = group_lanes();
    const dim3 tgrid(div_up((int64_t)nrounds * G, 256));
    const int32_t *pr_off = cons.c_pr + nrounds, *pr_cf = cons.c_pr + 2 * nrounds, *pr_len = cons.c_pr + 3 * nrounds;
    if (G == 16) {
      KLAUNCH((k_fame_timeline_g<16, 1>), tgrid, dim3(256), 0, st, t, cons.c_pr, pr_off, pr_cf, pr_len, nrounds, cons.c_nc,
              s_dec.p, s_decbit.p, cons.c_Lc);
    } else if (G == 32) {
      KLAUNCH((k_fame_timeline_g<32, 1>), tgrid, dim3(256), 0, st, t, cons.c_pr, pr_off, pr_cf, pr_len, nrounds, cons.c_nc,
              s_dec.p, s_decbit.p, cons.c_Lc);
    } else {
      KLAUNCH_NW(NW, NW_PAT, k_fame_timeline_g, 64, tgrid, dim3(256), 0, st, t, cons.c_pr, pr_off, pr_cf, pr_len,
                 nrounds, cons.c_nc, s_dec.p, s_decbit.p, cons.c_Lc);
    }
  }
  void fame_persist(const Tables& t, int nrounds) {
    KLAUNCH(k_fame_persist, dim3(div_up((int64_t)nrounds * N, 256)), dim3(256), 0, st, t, cons.c_pr, cons.c_pr + nrounds,
            cons.c_pr + 2 * nrounds, cons.c_pr + 3 * nrounds, nrounds, s_clast.p, s_dec.p);
  }

  // the end of a bulk replay that took its median from the FD rows: the rows of the
  // still-undetermined events (a later online call's k_median_wave reads them), from the
  // lowest such position of every chain.  The new undetermined list and its count are on
  // the device (bucket_and_sort): no round trip.
  void fdtd_tail(const Batch& b) {
    if (!cons.fdtd_stale) return;
    if (!b.got_order || b.spl || !b.commit) {  // (no new list on the device: all of it)
      ensure_fdtd();
      return;
    }
    HGE_HIPCHK(hipMemcpyAsync(s_fdlo.p, s_fdlo.p + N, 4 * (size_t)N, hipMemcpyDeviceToDevice, st));
    KLAUNCH(k_und_low, dim3(std::max(1, std::min(div_up(b.ncand, 256), 1024))), dim3(256), 0, st,
            (const int32_t*)d_creator.p, (const int32_t*)d_index.p, (const int32_t*)d_und.p,
            (const int32_t*)out_word(hge_plan::ResultsLayout::kUndetermined), s_fdlo.p);
    // (mostly a tile or two per chain; the kernel loops where more is left)
    fdtd_pass("fdtd_tail (k_fd_transpose_ts<uint16_t>)", std::min(div_up(std::max(cons.fdtd_maxlen, 1), 64), 4));
    cons.fdtd_stale = false;
  }

  // round received per candidate and its consensus timestamp.  N > 16: the median is a
  // wave-wide radix select (k_median_wave) over coalesced rows: the round frontier rows
  // transposed (WLA, ensure_wla, for every round a candidate can receive) and the FD
  // timestamp offsets (FDTD).  A fresh replay's candidate list is the identity
  // (candidate q = event q).
  void recv_dispatch(Batch& b) {
    const bool wmed = N > 16;
    const bool ident = b.fresh_und && b.cand == d_und.p && (int64_t)b.ncand == strm.log.n_events;
    int32_t* bseg = nullptr;
    if (wmed) {
      s_bseg.need(b.ncand);
      bseg = s_bseg.p;
      ensure_wla(b);
    }
    const Tables t = tables();
    KLAUNCH_NW(NW, NW_T, k_round_received, dim3(div_up(b.ncand, 256)), dim3(256), 0, st, t, b.cand, b.ncand,
               cons.vis_all ? (const int32_t*)nullptr : (const int32_t*)s_vis.p, b.ncalls, 0, b.rr_lo, b.R_last,
               cons.segoff_p, s_segcnt.p, s_segcall.p, s_segdec.p, s_segfws.p, s_theta.p, s_recv.p, s_rr.p, s_cts.p,
               bseg);
    if (wmed && ident && cons.fdtd_stale && !test_rows_fallback) {
      // a bulk replay whose coordinate step skipped the timestamps: the median from the FD rows
      // (16 positions x 512 threads measured fastest of seven shapes)
      constexpr int TQ = 16, NT = 512;
      const int64_t nb = (int64_t)N * div_up(cons.fdtd_maxlen, TQ);
      KLAUNCH_AS("k_median_rows<16, 512>", (k_median_rows<TQ, NT>), dim3((unsigned)nb), dim3(NT),
                 sizeof(int32_t) * TQ * (N + 4), st, t, (const int32_t*)(s_fdlo.p + N), (const int32_t*)s_recv.p,
                 (const int32_t*)s_rr.p, (const int32_t*)bseg, (const uint64_t*)s_segfws.p, s_cts.p);
    } else if (wmed) {
      ensure_fdtd();
      KLAUNCH_NW(NW, NW_T, k_median_wave, dim3(div_up(b.ncand, 4 * MED_EPW)), dim3(256), 0, st, t,
                 ident ? (const int32_t*)nullptr : b.cand, b.ncand, s_recv.p, s_rr.p, bseg, s_segfws.p, s_cts.p);
    }
  }

  // DivideRounds: everything inserted becomes visible to the consensus calls
  void divide() {
    cons.dividing = true;
    cons.und_appended = false;
    try {
      coords();
    } catch (...) {
      cons.dividing = false;
      throw;
    }
    cons.dividing = false;
    if (cons.n_divided < cons.n_coords) {
      // append the newly divided events to the undetermined list (insertion order),
      // unless k_round_assign already did
      const int64_t a = cons.n_divided, m = cons.n_coords - cons.n_divided;
      ensure_events(cons.n_coords);
      if (!cons.und_appended) KLAUNCH(k_iota, dim3(div_up(m, 256)), dim3(256), 0, st, d_und.p + cons.n_und, m, (int32_t)a);
      cons.n_und += m;
      cons.n_divided = cons.n_coords;
    }
    update_rdiv();
  }

  // An online RunConsensus at N <= 16 with ONE host round trip: the coordinate and
  // rounds launches of divide() (k_la_seq with the frontier start and the batch's FD,
  // k_fss, the rounds walk with the assignment and tail), then k_consensus_dyn, whose
  // control block the device builds from the walk's round count and the candidates'
  // lowest round; the results and the rounds' first witnesses come back together.
  // The rounds table is grown first so that the walk cannot overflow it (R grows by
  // at most one per new event).  Returns false (nothing done) when the call does not
  // fit this path.
  bool online_fast(std::vector<int32_t>& order) {
    const int64_t n0 = cons.n_coords, n1 = strm.log.n_events, m = n1 - n0;
    if (N > 16 || m <= 0 || cons.R == 0 || cons.cstep || split_on() || rec_on || cons.ext_on || strm.sp_active) return false;
    if (cons.n_divided != n0 || !la_seq_ok(m) || cons.n_und + m > 65536 || cons.n_und + m > SCAN_LDS) return false;
    if (hge_hooks::no_online_fast()) return false;
    if (*std::max_element(strm.log.chain_len.begin(), strm.log.chain_len.end()) + 1 >= 0xFFFF) return false;
    consensus_sync();
    ensure_rcap((int64_t)cons.R + m + 4);
    // ---- divide(): coordinates and rounds, no readback
    cons.dividing = true;
    cons.und_appended = false;
    if (!coords_a()) {
      cons.dividing = false;
      throw Error(HGE_ERR_INTERNAL, "online call: no coordinates to compute");
    }
    if (!cons.cstep || !cons.cstep->frontier_started)
      throw Error(HGE_ERR_INTERNAL, "online call: frontier start not fused");
    CoordStep s = *cons.cstep;
    cons.cstep.reset();
    // (n_divided == n0 and at most 65,536 candidates: the walk's block appends the new
    // ids, assigns their rounds and does the rounds tail)
    walk_online(s);
    cons.dividing = false;
    cons.n_coords = n1;
    cons.coords_len = strm.log.chain_len;
    cons.n_und += m;
    cons.n_divided = cons.n_coords;
    cons.und_fresh = false;
    // ---- consensus of the one call, control built on the device
    const int Rmax = cons.R + (int)m + 1;
    const int nround_max = std::max(1, Rmax - 2 - cons.lcr), nr_max = std::max(1, Rmax);
    Batch b;
    b.calls = &cons.n_divided;
    b.ncalls = 1;
    b.do_fame = b.do_order = b.commit = b.ord = true;
    b.cand = d_und.p;
    b.ncand = (int)cons.n_und;
    b.out = hge_plan::results_layout(1, b.ncand);
    b.ctl = hge_plan::ctl_layout(1, nround_max, nr_max);
    s_cctl.need(b.ctl.total);
    bind_ctl(b.ctl);
    s_dec.need((size_t)nround_max * N);
    s_decbit.need(nround_max);
    s_LCR.need(1);
    s_clast.need(nround_max);
    const size_t nslot = (size_t)nr_max * (N + 3);
    s_segcnt.need(nr_max);
    s_segcall.need(nslot);
    s_seground.need(nslot);
    s_segdec.need(nslot);
    s_segfws.need(nslot * NW);
    s_theta.need(nslot * N);
    s_out.need(b.out.total());
    DynCall dc{};
    dc.lcr = cons.lcr;
    dc.ncand = b.ncand;
    dc.Rcap = Rcap;
    dc.n_c = cons.n_divided;
    dc.rstate = s.rstate;
    dc.minw = d_minw.p;
    dc.c_nc = cons.c_nc;
    dc.c_Rc = cons.c_Rc;
    dc.c_Lc = cons.c_Lc;
    dc.c_flags = cons.c_flags;
    dc.c_pr = cons.c_pr;
    dc.c_pidx = cons.c_pidx;
    dc.c_sgo = cons.c_sgo;
    dc.dec = s_dec.p;
    dc.decbit = s_decbit.p;
    dc.LCR = s_LCR.p;
    dc.clast = s_clast.p;
    dc.out = s_out.p;
    dc.o = order_call(b, 1);  // (the buffers; the kernel sets the rounds, the windows and front)
    KLAUNCH(k_consensus_dyn<16>, dim3(1), dim3(1024), 0, st, tables(), dc);
    std::swap(d_und, s_und2);
    // ---- the one round trip: the results block and the rounds' first witnesses
    const size_t off = d2h_pinned(s_out.p, 4 * b.out.total());
    const size_t offw = d2h_pinned(d_minw.p, 4 * ((size_t)Rcap + hge_plan::kTailPartial));
    sync();
    const int32_t* hw = (const int32_t*)xfer.at(offw);
    const hge_plan::RoundsTail rt = hge_plan::parse_rounds_tail(hw + Rcap, 0);
    if (rt.overflow) {  // (unreachable: ensure_rcap covers R + m + 4) the host state has moved on: refuse later calls
      strm.failed = "online call: rounds table overflow past its bound";
      throw Error(HGE_ERR_INTERNAL, strm.failed);
    }
    cons.R = rt.R;
    cons.h_minw.assign(hw, hw + cons.R);
    cons.minw_full = false;
    cons.mnr_key[0] = -1;
    update_rdiv();
    const int32_t* ho = (const int32_t*)xfer.at(off);
    const hge_plan::Results r = hge_plan::parse_results(b.out, ho, ho + b.out.o_tx);
    commit_order(r, 1, true, &order, nullptr);
    if (r.lcr > cons.lcr) commit_lcr(r.lcr, r.lcr_events);
    prof.collect();
    return true;
  }

  // first witness id of every round (host copy: Rounds() as seen at any event count)
  void update_rdiv() {
    // h_minw was read back together with the round count (coords)
    cons.h_minw.resize(cons.R);
    if (cons.R == 0) {
      cons.R_div = 0;
      return;
    }
    cons.R_div = (int)(std::lower_bound(cons.h_minw.begin(), cons.h_minw.end(),
                                   (int32_t)std::min<int64_t>(cons.n_divided, INF32)) -
                  cons.h_minw.begin());
  }

  // A fresh replay in two halves: replay_begin (reset + coordinates) and
  // replay_end (rounds frontier, DivideRounds/DecideFame/FindOrder at every call);
  // the cross-GPU split runs the walkers and their join between the two.
  void replay_begin() {
    // fresh consensus state over the staged events (they stay resident in HBM)
    cons = ConsensusState(N);
    cons.w_start = std::chrono::steady_clock::now();
    reset_rounds();
    HGE_HIPCHK(hipEventRecord(ev[0], st));
    coords_a();
  }

  void replay_end(int64_t* n_ordered) {
    const int64_t keep = strm.log.n_events;
    if (cons.cstep) coords_b();
    HGE_HIPCHK(hipEventRecord(ev[1], st));
    const auto w1 = std::chrono::steady_clock::now();
    cons.n_divided = keep;
    update_rdiv();
    if (keep > 0) fill_iota(d_und.p, keep, 0);
    cons.n_und = keep;
    cons.und_fresh = keep > 0;
    cons.replay_counts.clear();
    // the consensus log (fresh since replay_begin) is the replay's order, delivered to the
    // pinned order buffer in one copy (not staged through the arena into the log's vector)
    cons.lazy_order = pin_ord.n >= (size_t)keep;
    try {
      consensus_batch(strm.replay_calls, true, true, true, nullptr, &cons.replay_counts);
    } catch (...) {
      cons.lazy_order = false;
      throw;
    }
    cons.lazy_order = false;
    HGE_HIPCHK(hipEventRecord(ev[2], st));
    HGE_HIPCHK(hipEventSynchronize(ev[2]));
    const auto w2 = std::chrono::steady_clock::now();
    float a = 0, b = 0;
    HGE_HIPCHK(hipEventElapsedTime(&a, ev[0], ev[1]));
    HGE_HIPCHK(hipEventElapsedTime(&b, ev[1], ev[2]));
    auto ms = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) {
      return (float)std::chrono::duration<double, std::milli>(y - x).count();
    };
    // [0] coordinates+rounds on the GPU, [1] their wall time, [2] consensus wall time,
    // [3] consensus on the GPU, [4] replay wall time, [5] the order's delivery to host
    // memory (wall, inside [2]), [6] GPU total
    stage_ms[0] = a;
    stage_ms[1] = ms(cons.w_start, w1);
    stage_ms[2] = ms(w1, w2);
    stage_ms[3] = b;
    stage_ms[4] = ms(cons.w_start, w2);
    stage_ms[6] = a + b;
    if (n_ordered) *n_ordered = consensus_size();
    dbg_dump();
  }

};

#include "hge_engine_abi.hip"
