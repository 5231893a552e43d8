// hge_batch_host.hip — the batch engine's host side: struct hge_batch and the C ABI
// (hge_batch_* in include/hge.h).  Part of hge_batch.hip's translation unit, included at
// its end after the kernels.
//
// Every data member is declared in one block at the top of the struct, in the part whose
// lifetime it shares ("State and lifetimes").  A device part declares its
// tables, sizes them from the staged layout (need), binds them to the kernels' argument
// structs (bind) and, where a run clears them, lists the clears, on adjacent lines.  The
// launch plan and the layout are hge_batch_plan.h's: no size rule is stated here.
using namespace hgb;

namespace {

using hge::DBuf;
using hge::Error;

inline size_t at_least_1(int64_t n) { return (size_t)std::max<int64_t>(n, 1); }

// A host array of the commit stream: mapped pinned memory the kernels store to
// (dev: its device-side address), or pageable memory that a copy fills after the run
// when the pinned allocation fails.
template <typename T>
struct HostField {
  T* h = nullptr;
  T* dev = nullptr;
  size_t cap = 0;
  bool pinned = false;
  void need(size_t n, bool try_pin) {
    if (h && n <= cap) return;
    pin_ = hge::PBuf<T>();
    page_.reset();
    h = dev = nullptr;
    cap = 0;
    pinned = false;
    n = std::max<size_t>(n, 1);
    if (try_pin) {
      try {
        pin_.need(n);
        dev = hge::PinnedMem::device_ptr(pin_.p);
      } catch (const Error&) {
      }
      if (dev) {
        h = pin_.p;
        pinned = true;
      } else {
        pin_ = hge::PBuf<T>();
        (void)hipGetLastError();  // not an error of the run: the copy path takes over
      }
    }
    if (!h) {
      page_.reset(new (std::nothrow) T[n]);
      if (!page_) throw Error{HGE_ERR_INTERNAL, "commit stream: host allocation failed"};
      h = page_.get();
    }
    cap = n;
  }

 private:
  hge::PBuf<T> pin_;
  std::unique_ptr<T[]> page_;
};

// ---- the graphs of the batch: reset by clear().  Added ones keep a host mirror, generated
// ones (hge_batch_generate, hge_batch_gen.hip) their parameters; a batch holds one or the other.
struct Graph {
  std::vector<int32_t> cr, ix, sp, op, oc, ntx;
  std::vector<int64_t> ts;
  std::vector<uint64_t> S;
  std::vector<uint8_t> coin;
  std::vector<int64_t> calls;  // accepted counts at the call points
  std::vector<std::vector<int32_t>> chain;
};
struct Source {
  std::vector<Graph> gs;
  std::vector<GenG> gen;
  int graphs() const { return gen.empty() ? (int)gs.size() : (int)gen.size(); }
};

// ---- the staged layout: from a stage until the batch changes (add, generate, clear)
struct Staged {
  bool ok = false;
  BatchPools p;
  std::vector<int32_t> h_gcnt;  // generated graphs: [g][4] submissions, accepted events, longest chain
};

// ---- what the last run left on the host.  A run starts from a fresh one and clear()
// leaves a fresh one; a batch that changes without a run (add, generate) only turns
// `ran` and `stats_ok` off: results, commits and statistics are refused and delivery
// reads 0, while the plan and the fallback count still describe the last run.  stage()
// turns `stats_ok` off alone.
struct LastRun {
  bool ran = false;       // hge_batch_info / results / commits_view answer
  bool stats_ok = false;  // hge_batch_stats answers
  std::vector<int64_t> h_scal;
  std::vector<int32_t> h_path;  // which graphs kb_consensus replayed (the source of an event's commit call)
  int64_t n_fallback = 0;       // their number
  BatchPlan plan;               // the kernel instances chosen from the batch's size (hge_batch_launch_plan)
  int32_t delivered = 0;        // 0 not delivered, 1 written by the kernels, 2 copied after the run
  uint32_t delivered_what = 0;  // the request as of the run
};

// ---- device: the graphs as the kernels read them, uploaded by stage() or written by
// kg_walk + kg_fill (stage_generated)
struct Inputs {
  DBuf<GDesc> d_gd;
  DBuf<int32_t> d_cr, d_ix, d_sp, d_op, d_oc, d_ntx, d_cg, d_clen, d_chain, d_ntxch;
  DBuf<int64_t> d_ts, d_calls, d_tsch;
  DBuf<uint64_t> d_S, d_Sch;
  DBuf<uint8_t> d_coin;
  // one rule for added and generated graphs: an empty pool is sized as one element
  void need(const BatchPools& p, int N, int G) {
    const size_t E1 = at_least_1(p.Etot), K1 = at_least_1(p.Ktot), CH = (size_t)G * N * p.ccap;
    d_gd.need(G);
    for (DBuf<int32_t>* b : {&d_cr, &d_ix, &d_sp, &d_op, &d_oc, &d_ntx}) b->need(E1);
    d_ts.need(E1);
    d_S.need(4 * E1);
    d_coin.need(E1);
    d_calls.need(K1);
    d_cg.need(K1);
    d_clen.need((size_t)G * N);
    d_chain.need(CH);
    d_tsch.need(CH);
    d_Sch.need(CH);
    d_ntxch.need(CH);
  }
  template <typename T>  // BT and GenT name them alike
  void bind(T& t) const {
    t.gd = d_gd.p;
    t.cr = d_cr.p;
    t.ix = d_ix.p;
    t.sp = d_sp.p;
    t.op = d_op.p;
    t.oc = d_oc.p;
    t.ntx = d_ntx.p;
    t.clen = d_clen.p;
    t.ts = d_ts.p;
    t.S = d_S.p;
    t.coin = d_coin.p;
    t.chain = d_chain.p;
    t.tsch = d_tsch.p;
    t.calls = d_calls.p;
    t.Sch = d_Sch.p;
    t.ntxch = d_ntxch.p;
    t.cg = d_cg.p;
  }
  void bind(ST& t) const {
    t.gd = d_gd.p;
    t.cr = d_cr.p;
    t.ix = d_ix.p;
    t.ts = d_ts.p;
    t.calls = d_calls.p;
  }
};

// ---- device: the tables a run writes
struct RunTables {
  DBuf<int32_t> d_LA, d_FDT, d_FD, d_round, d_rr, d_U, d_Ur, d_Ucp, d_order, d_krr, d_kid, d_W, d_WIX, d_WFD, d_th,
      d_rcnt, d_ver, d_thv;
  DBuf<int64_t> d_cts, d_kct, d_counts, d_scal;
  DBuf<uint64_t> d_ks0, d_ssb, d_seeb, d_dbg;  // d_dbg: HGB_STAMPS only
  DBuf<uint8_t> d_wit, d_WCOIN;
  DBuf<int8_t> d_fame;
  // the bulk call schedule (hge_batch_bulk.hip); d_xcc for the statistics pass (hge_batch_stats.hip)
  DBuf<int32_t> d_glist, d_Rc, d_rfirst, d_xcall, d_gx, d_nivl, d_fsuf, d_thp, d_thR, d_roundch, d_rcall, d_rrank,
      d_rrch, d_rslot, d_bcnt, d_boff, d_wlc, d_xcc;
  DBuf<uint64_t> d_arr, d_Dp, d_ivF, d_thF;
  DBuf<int64_t> d_ctsch, d_gctx;
  DBuf<int4> d_ivh, d_wl;
  DBuf<int2> d_cinf;
  void need(const BatchPools& p, int N, int G, bool dbg) {
    const size_t E1 = at_least_1(p.Etot);
    d_LA.need(E1 * N);
    d_FDT.need((size_t)G * N * N * p.ccap);
    d_FD.need((size_t)G * N * p.ccap * N);
    d_round.need(E1);
    d_wit.need(E1);
    d_rr.need(E1);
    d_cts.need(E1);
    d_U.need(E1);
    d_Ur.need(E1);
    d_Ucp.need(E1);
    d_order.need(E1);
    d_krr.need(2 * E1 + 64);
    d_kct.need(2 * E1 + 64);
    d_ks0.need(2 * E1 + 64);
    d_kid.need(2 * E1 + 64);
    const size_t RN = at_least_1(p.Rtot) * N;
    d_W.need(RN);
    d_WIX.need(RN);
    d_WFD.need(RN * N);
    d_WCOIN.need(RN);
    d_ssb.need(RN);
    d_seeb.need(RN);
    d_fame.need(RN);
    d_th.need(RN);
    d_rcnt.need(RN / N);
    d_ver.need(RN / N);
    d_thv.need(RN / N);
    d_counts.need(at_least_1(p.Ktot));
    d_scal.need((size_t)G * 8);
    if (dbg) d_dbg.need((size_t)G * 8);
    const size_t K1 = at_least_1(p.Ktot);
    d_glist.need(G);
    d_Rc.need(K1);
    d_rfirst.need(RN / N);
    d_xcall.need(E1);
    d_arr.need(E1);
    d_Dp.need(K1 * BNS * 2);
    d_gx.need((size_t)G * 16);
    d_ivh.need(RN / N * BVCAP);
    d_ivF.need(RN / N * BVCAP);
    d_nivl.need(RN / N);
    d_fsuf.need(RN / N);
    d_thp.need((size_t)G * BICAP * N);
    d_thR.need((size_t)G * BICAP);
    d_thF.need((size_t)G * BICAP);
    const size_t CH = (size_t)G * N * p.ccap;
    d_roundch.need(CH);
    d_rcall.need(CH);
    d_rrank.need(CH);
    d_rrch.need(CH);
    d_rslot.need(CH);
    d_ctsch.need(CH);
    d_bcnt.need(K1);
    d_boff.need(K1);
    d_wl.need(K1);
    d_wlc.need(1);
    d_gctx.need(G);
    d_cinf.need(E1);
    d_xcc.need(E1);
  }
  // what a run expects cleared, one kb_clear launch (at most 16 segments)
  void clears(ClrList& cl, const BatchPools& p, int N, int G) const {
    const size_t RN = at_least_1(p.Rtot) * N, E1 = at_least_1(p.Etot), K1 = at_least_1(p.Ktot);
    auto seg = [&](void* q, size_t bytes, uint32_t pat) { cl.s[cl.n++] = ClrSeg{q, (uint64_t)bytes, pat}; };
    seg(d_W.p, RN * 4, ~0u);
    seg(d_WIX.p, RN * 4, ~0u);
    seg(d_ssb.p, RN * 8, 0);
    seg(d_seeb.p, RN * 8, 0);
    seg(d_fame.p, RN, 0);
    seg(d_rcnt.p, RN / N * 4, 0);
    seg(d_ver.p, RN / N * 4, 0);
    seg(d_thv.p, RN / N * 4, ~0u);
    seg(d_rr.p, E1 * 4, ~0u);
    seg(d_cts.p, E1 * 8, 0);
    seg(d_scal.p, (size_t)G * 64, 0);
    seg(d_bcnt.p, K1 * 4, 0);
    seg(d_wlc.p, 4, 0);
    seg(d_gctx.p, (size_t)G * 8, 0);
  }
  void bind(BT& t, bool dbg) const {
    t.LA = d_LA.p;
    t.FDT = d_FDT.p;
    t.FD = d_FD.p;
    t.round = d_round.p;
    t.wit = d_wit.p;
    t.rr = d_rr.p;
    t.cts = d_cts.p;
    t.W = d_W.p;
    t.WIX = d_WIX.p;
    t.WFD = d_WFD.p;
    t.WCOIN = d_WCOIN.p;
    t.ssb = d_ssb.p;
    t.seeb = d_seeb.p;
    t.fame = d_fame.p;
    t.rcnt = d_rcnt.p;
    t.ver = d_ver.p;
    t.thv = d_thv.p;
    t.th = d_th.p;
    t.U = d_U.p;
    t.Ur = d_Ur.p;
    t.Ucp = d_Ucp.p;
    t.order = d_order.p;
    t.counts = d_counts.p;
    t.ord_rr = nullptr;  // Delivery::bind's
    t.ord_cts = nullptr;
    t.scal = d_scal.p;
    t.krr = d_krr.p;
    t.kct = d_kct.p;
    t.ks0 = d_ks0.p;
    t.kid = d_kid.p;
    t.dbg = dbg ? d_dbg.p : nullptr;
    t.glist = nullptr;  // the fallback pass's
    t.Rc = d_Rc.p;
    t.rfirst = d_rfirst.p;
    t.xcall = d_xcall.p;
    t.arr = d_arr.p;
    t.Dp = d_Dp.p;
    t.gx = d_gx.p;
    t.ivh = d_ivh.p;
    t.ivF = d_ivF.p;
    t.nivl = d_nivl.p;
    t.fsuf = d_fsuf.p;
    t.thp = d_thp.p;
    t.thR = d_thR.p;
    t.thF = d_thF.p;
    t.roundch = d_roundch.p;
    t.rcall = d_rcall.p;
    t.rrank = d_rrank.p;
    t.rrch = d_rrch.p;
    t.rslot = d_rslot.p;
    t.ctsch = d_ctsch.p;
    t.bcnt = d_bcnt.p;
    t.boff = d_boff.p;
    t.wl = d_wl.p;
    t.wlc = d_wlc.p;
    t.gctx = d_gctx.p;
    t.cinf = d_cinf.p;
    t.xcc = d_xcc.p;
  }
  void bind(ST& t) const {
    t.round = d_round.p;
    t.rr = d_rr.p;
    t.rcall = d_rcall.p;
    t.xcc = d_xcc.p;
    t.W = d_W.p;
    t.cts = d_cts.p;
    t.scal = d_scal.p;
    t.fame = d_fame.p;
  }
};

// ---- device, generated batches only: the parameters, the submission -> id map, the sizes
// the counting walk found, the raw submission pools, the accepted events' steps
struct GenTables {
  DBuf<GenG> d_gg;
  DBuf<int32_t> d_gmap, d_gcnt, d_scr, d_six, d_ssp, d_sop, d_sstep, d_sst, d_sacc, d_estep;
  DBuf<hge_event> d_raw;  // hge_batch_submissions' readback, sized there
  void need_count(int G, int64_t mtot) {  // before the layout is known
    d_gg.need(G);
    d_gcnt.need((size_t)G * 4);
    d_gmap.need((size_t)mtot);
  }
  void need(const BatchPools& p, int N) {
    const size_t E1 = at_least_1(p.Etot), S1 = at_least_1(p.Stot);
    for (DBuf<int32_t>* b : {&d_scr, &d_six, &d_ssp, &d_sop, &d_sstep, &d_sst, &d_sacc}) b->need(S1);
    d_estep.need(E1);
  }
  void bind(GenT& t) const {
    t.gg = d_gg.p;
    t.map = d_gmap.p;
    t.cnt = d_gcnt.p;
    t.s_cr = d_scr.p;
    t.s_ix = d_six.p;
    t.s_sp = d_ssp.p;
    t.s_op = d_sop.p;
    t.s_step = d_sstep.p;
    t.s_st = d_sst.p;
    t.s_acc = d_sacc.p;
    t.estep = d_estep.p;
  }
};

// ---- the commit stream in host memory (hge_batch_set_delivery), pooled like the device
// tables: ids / rr / cts at GDesc::eo, counts at GDesc::co.  Sized from the staged pools,
// kept across runs.  `what`: bit 0 order and counts, bit 1 rr and cts as well.
struct Delivery {
  HostField<int32_t> h_ids, h_orr;
  HostField<int64_t> h_octs, h_counts;
  DBuf<int32_t> d_orr;  // the copy path's device side of rr / cts (ids and counts: d_order, d_counts)
  DBuf<int64_t> d_octs;
  void ensure(const BatchPools& p, uint32_t what, bool no_pin) {
    if (!(what & 1)) return;
    const size_t E1 = at_least_1(p.Etot), K1 = at_least_1(p.Ktot);
    h_ids.need(E1, !no_pin);
    h_counts.need(K1, !no_pin);
    bool pin = h_ids.pinned && h_counts.pinned;
    if (what & 2) {
      h_orr.need(E1, !no_pin);
      h_octs.need(E1, !no_pin);
      pin = pin && h_orr.pinned && h_octs.pinned;
      if (!pin) {
        d_orr.need(E1);
        d_octs.need(E1);
      }
    }
  }
  bool pinned(uint32_t what) const {
    return h_ids.pinned && h_counts.pinned && (!(what & 2) || (h_orr.pinned && h_octs.pinned));
  }
  // The sorts and kb_consensus store the commit stream into mapped host memory (the
  // fallback pass into the same slots); it is the host's after the run's last
  // synchronise.  Returns the mode: 0 off, 1 stored by the kernels, 2 copied after the run.
  int bind(BT& t, uint32_t what) const {
    const int mode = !(what & 1) ? 0 : pinned(what) ? 1 : 2;
    if (mode == 1) {
      t.order = h_ids.dev;
      t.counts = h_counts.dev;
    }
    if (mode && (what & 2)) {
      t.ord_rr = mode == 1 ? h_orr.dev : d_orr.p;
      t.ord_cts = mode == 1 ? h_octs.dev : d_octs.p;
    }
    return mode;
  }
  // mode 2, no pinned memory: one pooled copy per field
  void copy_back(const BatchPools& p, uint32_t what, const RunTables& rt) {
    HGE_HIPCHK(hipMemcpy(h_ids.h, rt.d_order.p, (size_t)p.Etot * 4, hipMemcpyDeviceToHost));
    HGE_HIPCHK(hipMemcpy(h_counts.h, rt.d_counts.p, (size_t)p.Ktot * 8, hipMemcpyDeviceToHost));
    if (what & 2) {
      HGE_HIPCHK(hipMemcpy(h_orr.h, d_orr.p, (size_t)p.Etot * 4, hipMemcpyDeviceToHost));
      HGE_HIPCHK(hipMemcpy(h_octs.h, d_octs.p, (size_t)p.Etot * 8, hipMemcpyDeviceToHost));
    }
  }
};

// ---- the statistics pass (hge_batch_stats, hge_batch_stats.hip): grow-only scratch and results
struct StatsScratch {
  DBuf<int64_t> d_spart, d_sout;
  DBuf<int32_t> d_path;
  std::vector<int64_t> h_sout;
  void need(int G, int nb, int64_t HL) {
    const int64_t C = KS_ROW + HL;
    d_spart.need((size_t)G * nb * C);
    d_sout.need((size_t)(HL + (int64_t)G * C));
    d_path.need((size_t)G);
  }
  void bind(ST& t) const {
    t.path = d_path.p;
    t.part = d_spart.p;
    t.out = d_sout.p;
  }
};

}  // namespace

struct hge_batch {
  // the batch: never reset
  int N = 0, SM = 1, device = 0, ncu = 256;
  hge::Stream st;  // declared before every buffer and event: destroyed after them
  hge::Event ev[9];
  std::string err;
  bool dbg_on = getenv("HGB_STAMPS") != nullptr;
  bool serial = getenv("HGB_SERIAL") != nullptr;       // test hook: every graph through kb_consensus
  bool no_pin = getenv("HGB_TEST_NO_PIN") != nullptr;  // test hook: delivery takes the copy path
  uint32_t deliver = 0;                                // the request; the next stage or run takes it up
  static constexpr int NK = 8;  // coords, fd, fdrows, front, fame (prep + pairs), fold (+ theta), receive, order
  float kms[NK] = {};           // the last run that got as far (hge_batch_kernel_ms)
  // the parts (above)
  Source src;
  Staged stg;
  LastRun last;
  Inputs in;
  RunTables rt;
  GenTables gt;
  Delivery dl;
  StatsScratch ss;

  int graphs() const { return src.graphs(); }

  // the stream drained before the members die
  ~hge_batch() {
    if (st) (void)hipStreamSynchronize(st);
  }

  // The one way a kernel is launched here: every launch checked.
  template <typename K, typename... A>
  void launch(K kern, dim3 grid, dim3 block, const A&... args) {
    hipLaunchKernelGGL(kern, grid, block, 0, st, args...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw Error{HGE_ERR_DEVICE, std::string("batch launch: ") + hipGetErrorString(e)};
  }

  // the batch changed without a run (LastRun's comment)
  void changed() {
    stg = Staged{};
    last.ran = false;
    last.stats_ok = false;
  }

  // FromParentsLatest (hashgraph.go:366-396) and the index rule of the engine
  // (hge_engine.hip admit: index-lying events are refused, HGE_ERR_INDEX)
  int admit(Graph& G, const std::vector<int32_t>& tails, const hge_event& e, int32_t sp, int32_t op) {
    const int c = e.creator;
    if (c < 0 || c >= N) return HGE_ERR_CREATOR;
    const int known = (int)G.chain[c].size();
    const int64_t E = (int64_t)G.cr.size();
    if (sp == HGE_NONE && op == HGE_NONE && known == 0) return e.index == 0 ? HGE_OK : HGE_ERR_INDEX;
    if (sp < 0 || sp >= E) return HGE_ERR_SELF_PARENT_UNKNOWN;
    if (G.cr[sp] != c) return HGE_ERR_SELF_PARENT_CREATOR;
    if (op < 0 || op >= E) return HGE_ERR_OTHER_PARENT_UNKNOWN;
    if (sp != tails[c]) return HGE_ERR_SELF_PARENT_NOT_LAST;
    if (e.index != known) return HGE_ERR_INDEX;
    return HGE_OK;
  }

  int add(const hge_event* ev, int64_t n_sub, const int64_t* cp, int64_t n_calls, int32_t* status) {
    for (int64_t c = 0; c < n_calls; c++)
      if (cp[c] < 1 || cp[c] > n_sub || (c > 0 && cp[c] <= cp[c - 1]))
        throw Error{HGE_ERR_ARG, "hge_batch_add: call points must be strictly ascending within [1, n_sub]"};
    if (n_sub >= INT32_MAX / 2) throw Error{HGE_ERR_ARG, "hge_batch_add: stream too long for a batch graph"};
    if (!src.gen.empty())
      throw Error{HGE_ERR_ARG, "hge_batch_add: the batch holds generated graphs (hge_batch_clear first)"};
    src.gs.emplace_back();
    Graph& G = src.gs.back();
    G.chain.assign(N, {});
    std::vector<int32_t> tails(N, -1), idmap(n_sub, -1);
    int64_t nc = 0;
    for (int64_t i = 0; i < n_sub; i++) {
      const int32_t s = ev[i].self_parent, o = ev[i].other_parent;
      const int32_t sp = s < 0 ? HGE_NONE : (s < i && idmap[s] >= 0 ? idmap[s] : HGE_UNKNOWN);
      const int32_t op = o < 0 ? HGE_NONE : (o < i && idmap[o] >= 0 ? idmap[o] : HGE_UNKNOWN);
      const int r = admit(G, tails, ev[i], sp, op);
      if (r == HGE_OK) {
        const int32_t id = (int32_t)G.cr.size();
        idmap[i] = id;
        G.cr.push_back(ev[i].creator);
        G.ix.push_back(ev[i].index);
        G.sp.push_back(sp);
        G.op.push_back(op);
        G.oc.push_back(op >= 0 ? G.cr[op] : 0);
        G.ntx.push_back(ev[i].n_tx);
        G.ts.push_back(ev[i].timestamp_ns);
        for (int k = 0; k < 4; k++) {
          uint64_t v = 0;
          for (int b = 0; b < 8; b++) v = (v << 8) | ev[i].s[8 * k + b];
          G.S.push_back(v);
        }
        G.coin.push_back(ev[i].hash[16] != 0);
        G.chain[ev[i].creator].push_back(id);
        tails[ev[i].creator] = id;
      }
      if (status) status[i] = r == HGE_OK ? idmap[i] : r;
      while (nc < n_calls && cp[nc] == i + 1) {
        G.calls.push_back((int64_t)G.cr.size());
        nc++;
      }
    }
    changed();
    return (int)src.gs.size() - 1;
  }

  void generate(const hge_gossip_params& p, int32_t n_graphs, uint64_t seed0) {
    if (!src.gs.empty())
      throw Error{HGE_ERR_ARG, "hge_batch_generate: the batch holds added graphs (hge_batch_clear first)"};
    GenG q{};
    q.tf = (uint64_t)(p.fork_p * 4294967296.0);
    q.tc = (uint64_t)(p.cascade_p * 4294967296.0);
    q.events = (int32_t)p.events;
    q.k = std::min<int64_t>(p.k, 5 * p.events);  // past the stream's length: one call
    q.forkers = p.forkers;
    q.op_lag = p.op_lag;
    for (int32_t i = 0; i < n_graphs; i++) {
      q.seed = seed0 + (uint64_t)i;
      src.gen.push_back(q);
    }
    changed();
  }

  // every graph forgotten, every allocation kept
  void clear() {
    src = Source{};
    stg = Staged{};
    last = LastRun{};
  }

  template <typename T>
  void up(DBuf<T>& b, const std::vector<T>& h) {
    if (!h.empty()) HGE_HIPCHK(hipMemcpyAsync(b.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
  }

  // What both sources stage around their own filling of the inputs.  Before it: the
  // pools laid out, the inputs sized, the descriptors on their way (kg_walk<true> and
  // kg_fill read them).  After it: the run's tables sized, one wait.
  const BatchPools& staged_head(const std::vector<GraphSize>& sz) {
    const int G = (int)sz.size();
    stg.p = layout(SM, sz.data(), G);
    in.need(stg.p, N, G);
    HGE_HIPCHK(hipMemcpyAsync(in.d_gd.p, stg.p.hd.data(), sizeof(GDesc) * G, hipMemcpyHostToDevice, st));
    return stg.p;
  }
  void staged_tail(int G) {
    const BatchPools& p = stg.p;
    rt.need(p, N, G, dbg_on);
    HGE_HIPCHK(hipStreamSynchronize(st));
    dl.ensure(p, deliver, no_pin);
    stg.ok = true;
  }

  void stage() {
    last.stats_ok = false;
    if (stg.ok) {
      dl.ensure(stg.p, deliver, no_pin);
      return;
    }
    HGE_HIPCHK(hipSetDevice(device));
    if (!src.gen.empty()) {
      stage_generated();
      return;
    }
    const std::vector<Graph>& gs = src.gs;
    const int G = (int)gs.size();
    std::vector<GraphSize> sz((size_t)G);
    for (int g = 0; g < G; g++) {
      size_t longest = 0;
      for (int c = 0; c < N; c++) longest = std::max(longest, gs[g].chain[c].size());
      sz[g] = GraphSize{(int32_t)gs[g].cr.size(), (int32_t)gs[g].calls.size(), (int32_t)longest, 0};
    }
    const BatchPools& p = staged_head(sz);
    const int ccap = p.ccap;
    std::vector<int32_t> cr, ix, sp, op, oc, ntx, clen((size_t)G * N), chain((size_t)G * N * ccap, -1), cgv;
    for (int g = 0; g < G; g++) cgv.insert(cgv.end(), (size_t)p.hd[g].K, g);
    std::vector<int64_t> ts, tsch((size_t)G * N * ccap, 0), calls;
    std::vector<uint64_t> Sch((size_t)G * N * ccap, 0);
    std::vector<int32_t> ntxch((size_t)G * N * ccap, 0);
    std::vector<uint64_t> S;
    std::vector<uint8_t> coin;
    cr.reserve(p.Etot);
    for (int g = 0; g < G; g++) {
      const Graph& gr = gs[g];
      cr.insert(cr.end(), gr.cr.begin(), gr.cr.end());
      ix.insert(ix.end(), gr.ix.begin(), gr.ix.end());
      sp.insert(sp.end(), gr.sp.begin(), gr.sp.end());
      op.insert(op.end(), gr.op.begin(), gr.op.end());
      oc.insert(oc.end(), gr.oc.begin(), gr.oc.end());
      ntx.insert(ntx.end(), gr.ntx.begin(), gr.ntx.end());
      ts.insert(ts.end(), gr.ts.begin(), gr.ts.end());
      S.insert(S.end(), gr.S.begin(), gr.S.end());
      coin.insert(coin.end(), gr.coin.begin(), gr.coin.end());
      calls.insert(calls.end(), gr.calls.begin(), gr.calls.end());
      for (int c = 0; c < N; c++) {
        clen[(size_t)g * N + c] = (int32_t)gr.chain[c].size();
        for (size_t q = 0; q < gr.chain[c].size(); q++) {
          chain[((size_t)g * N + c) * ccap + q] = gr.chain[c][q];
          tsch[((size_t)g * N + c) * ccap + q] = gr.ts[gr.chain[c][q]];
          Sch[((size_t)g * N + c) * ccap + q] = gr.S[4 * (size_t)gr.chain[c][q]];
          ntxch[((size_t)g * N + c) * ccap + q] = gr.ntx[gr.chain[c][q]];
        }
      }
    }
    up(in.d_cr, cr);
    up(in.d_ix, ix);
    up(in.d_sp, sp);
    up(in.d_op, op);
    up(in.d_oc, oc);
    up(in.d_ntx, ntx);
    up(in.d_ts, ts);
    up(in.d_S, S);
    up(in.d_coin, coin);
    up(in.d_calls, calls);
    up(in.d_clen, clen);
    up(in.d_chain, chain);
    up(in.d_tsch, tsch);
    up(in.d_Sch, Sch);
    up(in.d_ntxch, ntxch);
    up(in.d_cg, cgv);
    staged_tail(G);
  }

  GenT gen_tables() const {
    GenT t{};
    t.N = N;
    t.ccap = stg.p.ccap;
    gt.bind(t);
    in.bind(t);
    return t;
  }

  // The generated graphs' staging: what stage() uploads, written by kernels.  The pools'
  // offsets need every graph's submission, accepted and call counts and the longest
  // chain: a counting instance of the walk finds them (the walk is deterministic), one
  // readback of 16 bytes per graph brings them to the host, and the walk runs again
  // into pools laid out exactly.  An upper bound instead (5 submissions a step, all
  // accepted, one chain) would size the E x N and chain tables of every later stage
  // five and N times too large.
  void stage_generated() {
    std::vector<GenG>& gen = src.gen;
    const int G = (int)gen.size();
    int64_t mtot = 0;
    for (GenG& q : gen) {
      q.mo = mtot;
      q.so = 0;
      mtot += 5 * (int64_t)q.events;
    }
    gt.need_count(G, mtot);
    HGE_HIPCHK(hipMemcpyAsync(gt.d_gg.p, gen.data(), sizeof(GenG) * G, hipMemcpyHostToDevice, st));
    launch(kg_walk<false>, dim3(G), dim3(64), gen_tables());
    std::vector<int32_t>& h_gcnt = stg.h_gcnt;
    h_gcnt.resize((size_t)G * 4);
    HGE_HIPCHK(hipMemcpyAsync(h_gcnt.data(), gt.d_gcnt.p, (size_t)G * 16, hipMemcpyDeviceToHost, st));
    HGE_HIPCHK(hipStreamSynchronize(st));
    std::vector<GraphSize> sz((size_t)G);
    int Kmax = 0;
    int64_t so = 0;
    for (int g = 0; g < G; g++) {
      const int64_t nsub = h_gcnt[(size_t)g * 4], k = gen[g].k;
      sz[g] = GraphSize{h_gcnt[(size_t)g * 4 + 1], (int32_t)((nsub + k - 1) / k), h_gcnt[(size_t)g * 4 + 2], nsub};
      Kmax = std::max(Kmax, sz[g].K);
      gen[g].so = so;
      so += nsub;
    }
    const BatchPools& p = staged_head(sz);
    HGE_HIPCHK(hipMemcpyAsync(gt.d_gg.p, gen.data(), sizeof(GenG) * G, hipMemcpyHostToDevice, st));
    gt.need(p, N);
    // the chain tables past a chain's length, as stage() uploads them
    const size_t CH = (size_t)G * N * p.ccap;
    HGE_HIPCHK(hipMemsetAsync(in.d_chain.p, 0xFF, CH * 4, st));
    HGE_HIPCHK(hipMemsetAsync(in.d_tsch.p, 0, CH * 8, st));
    HGE_HIPCHK(hipMemsetAsync(in.d_Sch.p, 0, CH * 8, st));
    HGE_HIPCHK(hipMemsetAsync(in.d_ntxch.p, 0, CH * 4, st));
    const GenT t = gen_tables();
    launch(kg_walk<true>, dim3(G), dim3(64), t);
    const int fx = (std::max(p.Emax, Kmax) + 255) / 256;
    if (fx > 0) launch(kg_fill, dim3((unsigned)fx, (unsigned)G), dim3(256), t);
    staged_tail(G);
  }

  // graph g's raw stream and admission results, read back from the staged pools
  int64_t submissions(int32_t g, hge_event* ev_out, int32_t* status_out, int64_t cap) {
    if (src.gen.empty() || !stg.ok) throw Error{HGE_ERR_ARG, "hge_batch_submissions: no staged generated graphs"};
    const int64_t nsub = stg.h_gcnt[(size_t)g * 4];
    if (cap < nsub || nsub == 0) return nsub;
    HGE_HIPCHK(hipSetDevice(device));
    if (ev_out) {
      gt.d_raw.need((size_t)nsub);
      launch(kg_raw, dim3((unsigned)((nsub + 255) / 256)), dim3(256), gen_tables(), g, gt.d_raw.p);
      HGE_HIPCHK(hipMemcpyAsync(ev_out, gt.d_raw.p, (size_t)nsub * sizeof(hge_event), hipMemcpyDeviceToHost, st));
    }
    if (status_out)
      HGE_HIPCHK(hipMemcpyAsync(status_out, gt.d_sst.p + src.gen[g].so, (size_t)nsub * 4, hipMemcpyDeviceToHost, st));
    HGE_HIPCHK(hipStreamSynchronize(st));
    return nsub;
  }

  BT tables() const {
    BT t;
    t.N = N;
    t.SM = SM;
    t.ccap = stg.p.ccap;
    in.bind(t);
    rt.bind(t, dbg_on);
    return t;
  }

  // the stages of a run before the fallback pass, each the instance `plan` names
  template <int NM, bool DLV>
  void run_stages(int G, const BT& t, const BatchPlan& plan) {
    const BatchPools& p = stg.p;
    const dim3 per_graph(G);
    if (plan.coords != 2) {
      if (p.Emax > 0) launch(kb_levels, dim3((unsigned)((p.Emax + 255) / 256), (unsigned)G), dim3(256), t);
      if (plan.coords == 0) launch(kb_coords<NM, 512, true, 2>, dim3(G * 2), dim3(512), t);
      else launch(kb_coords<NM, 1024, true>, per_graph, dim3(1024), t);
    } else {
      launch(kb_coords<NM, 512, false>, per_graph, dim3(512), t);
    }
    HGE_HIPCHK(hipEventRecord(ev[1], st));
    launch(kb_fd<NM>, dim3(G * N), dim3(64 * (NM / FCW)), t);
    HGE_HIPCHK(hipEventRecord(ev[2], st));
    launch(kb_fdrows<NM>, dim3(G * N), dim3(256), t);  // rows for kb_front (kb_median reads the run layout)
    HGE_HIPCHK(hipEventRecord(ev[3], st));
    if (plan.front_threads == 256) launch(kb_front<NM, 256>, per_graph, dim3(256), t);
    else if (plan.front_threads == 512) launch(kb_front<NM, 512>, per_graph, dim3(512), t);
    else launch(kb_front<NM, 1024>, per_graph, dim3(1024), t);
    HGE_HIPCHK(hipEventRecord(ev[4], st));
    if (serial) {  // every graph through kb_consensus, after the run's readback
      for (int k = 5; k < 9; k++) HGE_HIPCHK(hipEventRecord(ev[k], st));
      return;
    }
    launch(kb_prep<NM>, per_graph, dim3(1024), t);
    if (plan.ns == 2) launch(kb_pairs<NM, 2>, dim3(8, (unsigned)G), dim3(256), t);
    else launch(kb_pairs<NM, 3>, dim3(8, (unsigned)G), dim3(256), t);
    HGE_HIPCHK(hipEventRecord(ev[5], st));
    if (plan.ns == 2) launch(kb_fold<NM, 2>, per_graph, dim3(64), t);
    else launch(kb_fold<NM, 3>, per_graph, dim3(64), t);
    launch(kb_theta<NM>, per_graph, dim3(256), t);
    HGE_HIPCHK(hipEventRecord(ev[6], st));
    if (p.Emax > 0) {
      launch(kb_receive<NM>, dim3((unsigned)N, (unsigned)G), dim3(256), t);
      launch(kb_median<NM>, dim3((unsigned)(N * ((p.ccap + 255) / 256)), (unsigned)G), dim3(256), t);
    }
    HGE_HIPCHK(hipEventRecord(ev[7], st));
    launch(kb_order_prep<NM>, per_graph, dim3(1024), t);
    // the first class's grid: a bucket each up to 16 per CU; larger buckets a workgroup each
    const int nbk = (int)std::min<int64_t>(std::max<int64_t>(p.Ktot, 1), (int64_t)ncu * 16);
    if (plan.sort_threads == 64) launch(kb_sort<64, 0, 1024, DLV>, dim3(nbk), dim3(64), t, 0);
    else launch(kb_sort<256, 0, 1024, DLV>, dim3(nbk), dim3(256), t, 0);
    launch(kb_sort<256, 1024, 4096, DLV>, dim3(ncu), dim3(256), t, 1);
    HGE_HIPCHK(hipEventRecord(ev[8], st));
  }

  // the fallback pass: the F graphs of t.glist call by call
  template <int NM>
  void run_consensus(int F, const BT& t, const BatchPlan& plan) {
    auto replay = [&](auto kern_off, auto kern_on) {
      plan.dlv ? launch(kern_on, dim3(F), dim3(256), t) : launch(kern_off, dim3(F), dim3(256), t);
    };
    if (plan.consensus_occ == 4) replay(kb_consensus<NM, 4, false>, kb_consensus<NM, 4, true>);
    else replay(kb_consensus<NM, 1, false>, kb_consensus<NM, 1, true>);
  }

  int64_t run() {
    stage();
    last = LastRun{};
    const BatchPools& p = stg.p;
    const int G = graphs();
    if (G == 0) {
      last.stats_ok = true;
      return 0;
    }
    ClrList cl{};
    rt.clears(cl, p, N, G);
    launch(kb_clear, dim3((unsigned)std::min<size_t>(2048, (at_least_1(p.Etot) * 8 / 16 + 255) / 256 + 1)), dim3(256), cl);
    BT t = tables();
    const int mode = dl.bind(t, deliver);
    HGE_HIPCHK(hipEventRecord(ev[0], st));
    // dlv: the kernel instances that store rr / cts in commit order
    BatchPlan& plan = last.plan = batch_stage_plan(N, G, p.Ktot, ncu, serial, t.ord_rr != nullptr);
    if (plan.nm == 32) plan.dlv ? run_stages<32, true>(G, t, plan) : run_stages<32, false>(G, t, plan);
    else plan.dlv ? run_stages<64, true>(G, t, plan) : run_stages<64, false>(G, t, plan);
    std::vector<int64_t>& h_scal = last.h_scal;
    h_scal.resize((size_t)G * 8);
    HGE_HIPCHK(hipMemcpyAsync(h_scal.data(), rt.d_scal.p, (size_t)G * 64, hipMemcpyDeviceToHost, st));
    HGE_HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < NK; k++) HGE_HIPCHK(hipEventElapsedTime(&kms[k], ev[k], ev[k + 1]));
    // graphs the bulk fold could not hold: replayed by kb_consensus (their outputs untouched so far)
    std::vector<int32_t> fb;
    for (int g = 0; g < G; g++)
      if (serial || (h_scal[(size_t)g * 8 + 7] && !h_scal[(size_t)g * 8 + 6])) fb.push_back(g);
    last.n_fallback = (int64_t)fb.size();
    last.h_path.assign((size_t)G, 0);
    for (int32_t g : fb) last.h_path[(size_t)g] = 1;
    plan.consensus_occ = batch_consensus_occ(last.n_fallback, ncu);
    if (plan.consensus_occ) {
      HGE_HIPCHK(hipMemcpyAsync(rt.d_glist.p, fb.data(), fb.size() * 4, hipMemcpyHostToDevice, st));
      t.glist = rt.d_glist.p;
      float ms = 0;
      HGE_HIPCHK(hipEventRecord(ev[7], st));
      if (plan.nm == 32) run_consensus<32>((int)fb.size(), t, plan);
      else run_consensus<64>((int)fb.size(), t, plan);
      HGE_HIPCHK(hipEventRecord(ev[8], st));
      HGE_HIPCHK(hipMemcpyAsync(h_scal.data(), rt.d_scal.p, (size_t)G * 64, hipMemcpyDeviceToHost, st));
      HGE_HIPCHK(hipStreamSynchronize(st));
      HGE_HIPCHK(hipEventElapsedTime(&ms, ev[7], ev[8]));
      kms[NK - 1] += ms;
    }
    if (dbg_on) {  // section cycles of kb_consensus, summed over the graphs
      std::vector<uint64_t> hd_((size_t)G * 8);
      HGE_HIPCHK(hipMemcpy(hd_.data(), rt.d_dbg.p, (size_t)G * 64, hipMemcpyDeviceToHost));
      double sum[5] = {};
      for (int g = 0; g < G; g++)
        for (int i = 0; i < 5; i++) sum[i] += (double)hd_[(size_t)g * 8 + i];
      fprintf(stderr, "[hgb stamps] per graph cycles: divide %.0f fame %.0f thresholds %.0f receive %.0f order %.0f\n",
              sum[0] / G, sum[1] / G, sum[2] / G, sum[3] / G, sum[4] / G);
    }
    int64_t tot = 0;
    for (int g = 0; g < G; g++) {
      if (h_scal[(size_t)g * 8 + 6])
        throw Error{HGE_ERR_INTERNAL, "batch graph " + std::to_string(g) + ": round capacity exceeded"};
      tot += h_scal[(size_t)g * 8 + 4];
    }
    if (mode == 2) dl.copy_back(p, deliver, rt);
    last.delivered = mode;
    last.delivered_what = deliver;
    last.ran = true;
    last.stats_ok = true;
    return tot;
  }

  // The last run's statistics: three launches over the state in HBM, one copy, one wait.
  // A graph is cut into nb spans while the batch alone would leave compute units idle.
  void stats(const hge_stats_spec& s, int64_t* rows, int64_t* hist, int64_t* ghist) {
    const int G = graphs();
    const int64_t HL = hge_stats::hist_len(s);
    if (G == 0) {
      memset(hist, 0, (size_t)HL * 8);
      return;
    }
    HGE_HIPCHK(hipSetDevice(device));
    const int Emax = stg.p.Emax;
    const int64_t per = (4 * (int64_t)ncu + G - 1) / G, cut = ((int64_t)Emax + 4095) / 4096;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(per, cut), 1024));
    ss.need(G, nb, HL);
    HGE_HIPCHK(hipMemcpyAsync(ss.d_path.p, last.h_path.data(), (size_t)G * 4, hipMemcpyHostToDevice, st));
    ST t{};
    t.s = s;
    t.N = N;
    t.ccap = stg.p.ccap;
    t.G = G;
    t.nb = nb;
    t.span = std::max<int64_t>(1, ((int64_t)Emax + nb - 1) / nb);
    in.bind(t);
    rt.bind(t);
    ss.bind(t);
    launch(ks_events, dim3((unsigned)nb, (unsigned)G), dim3(KS_NT), t);
    launch(ks_finish, dim3((unsigned)G), dim3(KS_NT), t);
    launch(ks_total, dim3((unsigned)((HL + 63) / 64)), dim3(1024), t);
    // totals | rows | slabs: the prefix the caller asked for
    const size_t n = (size_t)(HL + (rows || ghist ? (int64_t)G * KS_ROW : 0) + (ghist ? (int64_t)G * HL : 0));
    std::vector<int64_t>& h_sout = ss.h_sout;
    h_sout.resize(n);
    HGE_HIPCHK(hipMemcpyAsync(h_sout.data(), ss.d_sout.p, n * 8, hipMemcpyDeviceToHost, st));
    HGE_HIPCHK(hipStreamSynchronize(st));
    memcpy(hist, h_sout.data(), (size_t)HL * 8);
    if (rows) memcpy(rows, h_sout.data() + HL, (size_t)G * KS_ROW * 8);
    if (ghist) memcpy(ghist, h_sout.data() + HL + (size_t)G * KS_ROW, (size_t)G * HL * 8);
  }

  template <typename T>
  void down(T* host, const T* dev, size_t n) {
    if (host && n) HGE_HIPCHK(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost));
  }
};

#define BGUARD_BEGIN try {
#define BGUARD_END(b)                 \
  }                                   \
  catch (Error & e) {                 \
    (b)->err = e.msg;                 \
    return e.code;                    \
  }                                   \
  catch (std::exception & e) {        \
    (b)->err = e.what();              \
    return HGE_ERR_INTERNAL;          \
  }

extern "C" {

int hge_batch_create(int32_t n_participants, int32_t device, hge_batch** out) {
  if (!out || n_participants < 1 || n_participants > 64) return HGE_ERR_ARG;
  hge_batch* b = new hge_batch();
  b->N = n_participants;
  b->SM = 2 * n_participants / 3 + 1;  // hashgraph.go:78-80
  b->device = device;
  try {
    HGE_HIPCHK(hipSetDevice(device));
    HGE_HIPCHK(hipDeviceGetAttribute(&b->ncu, hipDeviceAttributeMultiprocessorCount, device));
    b->st.create();
    for (auto& e : b->ev) e.create();
  } catch (Error& e) {
    delete b;
    return e.code;
  }
  *out = b;
  return HGE_OK;
}

void hge_batch_destroy(hge_batch* b) {
  delete b;
}

const char* hge_batch_last_error(hge_batch* b) { return b ? b->err.c_str() : "null handle"; }

int hge_batch_add(hge_batch* b, const hge_event* ev, int64_t n_sub, const int64_t* call_points, int64_t n_calls,
                  int32_t* status_out, int32_t* graph_out) {
  if (!b) return HGE_ERR_ARG;
  BGUARD_BEGIN
  if (n_sub < 0 || (n_sub > 0 && !ev) || n_calls < 0 || (n_calls > 0 && !call_points))
    throw Error{HGE_ERR_ARG, "hge_batch_add: bad argument"};
  const int g = b->add(ev, n_sub, call_points, n_calls, status_out);
  if (graph_out) *graph_out = g;
  return HGE_OK;
  BGUARD_END(b)
}

int hge_batch_stage(hge_batch* b) {
  if (!b) return HGE_ERR_ARG;
  BGUARD_BEGIN
  b->stage();
  return HGE_OK;
  BGUARD_END(b)
}

int hge_batch_run(hge_batch* b, int64_t* n_ordered) {
  if (!b) return HGE_ERR_ARG;
  BGUARD_BEGIN
  const int64_t m = b->run();
  if (n_ordered) *n_ordered = m;
  return HGE_OK;
  BGUARD_END(b)
}

int32_t hge_batch_graphs(hge_batch* b) { return b ? (int32_t)b->graphs() : -1; }

int hge_batch_info(hge_batch* b, int32_t g, int64_t* info) {
  if (!b || !info || g < 0 || g >= b->graphs()) return HGE_ERR_ARG;
  if (!b->last.ran) {
    b->err = "hge_batch_info: no replay yet (hge_batch_run)";
    return HGE_ERR_ARG;
  }
  const int64_t* s = &b->last.h_scal[(size_t)g * 8];
  info[0] = b->stg.p.hd[g].E;  // the staged graph's: generated graphs have no host mirror
  info[1] = b->stg.p.hd[g].K;
  for (int k = 0; k < 6; k++) info[2 + k] = s[k];
  return HGE_OK;
}

int hge_batch_results(hge_batch* b, int32_t g, int32_t* order, int64_t* counts, int32_t* round, uint8_t* witness,
                      int32_t* rr, int64_t* cts, int8_t* fame, int32_t* undetermined) {
  if (!b || g < 0 || g >= b->graphs()) return HGE_ERR_ARG;
  BGUARD_BEGIN
  if (!b->last.ran) throw Error{HGE_ERR_ARG, "hge_batch_results: no replay yet (hge_batch_run)"};
  const GDesc& d = b->stg.p.hd[g];
  const RunTables& rt = b->rt;
  const int64_t* s = &b->last.h_scal[(size_t)g * 8];
  const int N = b->N;
  if (b->last.delivered) {  // the last run delivered them: they are in host memory already
    if (order && s[4]) memcpy(order, b->dl.h_ids.h + d.eo, (size_t)s[4] * sizeof(int32_t));
    if (counts && d.K) memcpy(counts, b->dl.h_counts.h + d.co, (size_t)d.K * sizeof(int64_t));
  } else {
    b->down(order, rt.d_order.p + d.eo, (size_t)s[4]);
    b->down(counts, rt.d_counts.p + d.co, (size_t)d.K);
  }
  b->down(round, rt.d_round.p + d.eo, (size_t)d.E);
  b->down(witness, rt.d_wit.p + d.eo, (size_t)d.E);
  b->down(rr, rt.d_rr.p + d.eo, (size_t)d.E);
  b->down(cts, rt.d_cts.p + d.eo, (size_t)d.E);
  b->down(undetermined, rt.d_U.p + d.eo, (size_t)s[5]);
  if (fame && s[0] > 0) {
    const size_t RN = (size_t)s[0] * N;
    std::vector<int32_t> w(RN);
    std::vector<int8_t> f(RN);
    b->down(w.data(), rt.d_W.p + (size_t)d.ro * N, RN);
    b->down(f.data(), rt.d_fame.p + (size_t)d.ro * N, RN);
    for (size_t k = 0; k < RN; k++) fame[k] = w[k] >= 0 ? f[k] : (int8_t)-1;
  }
  return HGE_OK;
  BGUARD_END(b)
}

int64_t hge_batch_fallbacks(hge_batch* b) { return b ? b->last.n_fallback : -1; }

int hge_batch_set_delivery(hge_batch* b, uint32_t what) {
  if (!b) return HGE_ERR_ARG;
  if (what > 3 || what == 2) {
    b->err = "hge_batch_set_delivery: what is 0, 1 or 3 (bit 1 needs bit 0)";
    return HGE_ERR_ARG;
  }
  b->deliver = what;
  return HGE_OK;
}

int32_t hge_batch_delivery(hge_batch* b) { return b && b->last.ran ? b->last.delivered : 0; }

int hge_batch_commits_view(hge_batch* b, int32_t g, hge_batch_commits* out) {
  if (!b || !out || g < 0 || g >= b->graphs()) return HGE_ERR_ARG;
  if (!b->last.ran || !b->last.delivered) {
    b->err = "hge_batch_commits_view: the last run did not deliver (hge_batch_set_delivery, then hge_batch_run)";
    return HGE_ERR_ARG;
  }
  const GDesc& d = b->stg.p.hd[g];
  const Delivery& dl = b->dl;
  const bool rec = (b->last.delivered_what & 2) != 0;
  out->ids = dl.h_ids.h + d.eo;
  out->rr = rec ? dl.h_orr.h + d.eo : nullptr;
  out->cts = rec ? dl.h_octs.h + d.eo : nullptr;
  out->counts = dl.h_counts.h + d.co;
  out->ordered = b->last.h_scal[(size_t)g * 8 + 4];
  out->calls = d.K;
  return HGE_OK;
}

int hge_gossip_params_check(int32_t n_participants, const hge_gossip_params* p, int32_t n_graphs) {
  if (!p || n_participants < 1 || n_participants > 64 || n_graphs < 1) return HGE_ERR_ARG;
  if (p->events < n_participants || p->events > HGE_GOSSIP_MAX_EVENTS || p->forkers < 0 || p->k < 1) return HGE_ERR_ARG;
  if (!(p->fork_p >= 0.0 && p->fork_p <= 1.0) || !(p->cascade_p >= 0.0 && p->cascade_p <= 1.0)) return HGE_ERR_ARG;
  if (p->op_lag < 0 || p->op_lag > HGE_GOSSIP_MAX_OP_LAG) return HGE_ERR_ARG;
  return HGE_OK;
}

int hge_batch_generate(hge_batch* b, const hge_gossip_params* p, int32_t n_graphs, uint64_t seed0) {
  if (!b) return HGE_ERR_ARG;
  BGUARD_BEGIN
  static_assert(HGE_GOSSIP_MAX_OP_LAG < GLAG && 5ll * HGE_GOSSIP_MAX_EVENTS < (1 << 24), "kg_walk's ring and map entry");
  if (hge_gossip_params_check(b->N, p, n_graphs) != HGE_OK)
    throw Error{HGE_ERR_ARG, "hge_batch_generate: bad argument (hge_gossip_params_check)"};
  b->generate(*p, n_graphs, seed0);
  return HGE_OK;
  BGUARD_END(b)
}

int hge_stats_spec_check(const hge_stats_spec* s) { return hge_stats::spec_ok(s) ? HGE_OK : HGE_ERR_ARG; }

int64_t hge_stats_hist_len(const hge_stats_spec* s) {
  return hge_stats::spec_ok(s) ? hge_stats::hist_len(*s) : (int64_t)HGE_ERR_ARG;
}

int hge_batch_stats(hge_batch* b, const hge_stats_spec* s, int64_t* graph_rows, int64_t* hist, int64_t* graph_hist) {
  if (!b) return HGE_ERR_ARG;
  BGUARD_BEGIN
  if (!hge_stats::spec_ok(s)) throw Error{HGE_ERR_ARG, "hge_batch_stats: bad spec (hge_stats_spec_check)"};
  if (!hist) throw Error{HGE_ERR_ARG, "hge_batch_stats: hist is NULL"};
  if (!b->last.stats_ok)
    throw Error{HGE_ERR_ARG, "hge_batch_stats: no run since the batch last changed (hge_batch_run)"};
  b->stats(*s, graph_rows, hist, graph_hist);
  return HGE_OK;
  BGUARD_END(b)
}

int hge_batch_clear(hge_batch* b) {
  if (!b) return HGE_ERR_ARG;
  BGUARD_BEGIN
  if (b->st) HGE_HIPCHK(hipStreamSynchronize(b->st));
  b->clear();
  return HGE_OK;
  BGUARD_END(b)
}

int64_t hge_batch_submissions(hge_batch* b, int32_t g, hge_event* ev_out, int32_t* status_out, int64_t cap) {
  if (!b || g < 0 || g >= b->graphs()) return HGE_ERR_ARG;
  BGUARD_BEGIN
  return b->submissions(g, ev_out, status_out, cap);
  BGUARD_END(b)
}

int hge_batch_launch_plan(hge_batch* b, int32_t* out, int32_t cap) {
  if (!b || (!out && cap > 0)) return HGE_ERR_ARG;
  const BatchPlan& p = b->last.plan;
  const int32_t f[] = {b->ncu, p.nm, p.coords, p.front_threads, p.ns, p.sort_threads, p.consensus_occ, p.dlv};
  const int n = (int)(sizeof(f) / sizeof(f[0]));
  for (int k = 0; k < n && k < cap; k++) out[k] = f[k];
  return n;
}

int hge_batch_kernel_ms(hge_batch* b, float* ms, int32_t cap) {
  if (!b || (!ms && cap > 0)) return HGE_ERR_ARG;
  for (int k = 0; k < hge_batch::NK && k < cap; k++) ms[k] = b->kms[k];
  return hge_batch::NK;
}

}  // extern "C"

// diagnostics (not part of the C ABI): graph g's lastAncestors (which 0) or
// firstDescendants (which 1) rows after a run, E x N int32 into out
extern "C" int hgb_debug_rows(hge_batch* b, int32_t g, int32_t which, int32_t* out) {
  if (!b || !out || g < 0 || g >= b->graphs() || !b->last.ran) return HGE_ERR_ARG;
  BGUARD_BEGIN
  const GDesc& d = b->stg.p.hd[g];
  const int N = b->N, ccap = b->stg.p.ccap;
  if (which == 2)  // the run layout FDT[j][c][p], N x N x ccap
    b->down(out, b->rt.d_FDT.p + (size_t)g * N * N * ccap, (size_t)N * N * ccap);
  else
    b->down(out, b->rt.d_LA.p + d.eo * N, (size_t)d.E * N);
  return HGE_OK;
  BGUARD_END(b)
}
