// hge_engine_abi.hip — the C ABI of include/hge.h over hge_engine.  Included at the end
// of hge_engine.hip: the same translation unit, split off for reading.
// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
#define GUARD_BEGIN try {
#define REFUSE_IF_FAILED(h) \
  if (!(h)->strm.failed.empty()) throw Error(HGE_ERR_INTERNAL, "engine state inconsistent since: " + (h)->strm.failed);
#define GUARD_END(h)                 \
  }                                  \
  catch (Error & e) {                \
    (h)->err = e.msg;                \
    return e.code;                   \
  }                                  \
  catch (std::exception & e) {       \
    (h)->err = e.what();             \
    return HGE_ERR_INTERNAL;         \
  }

extern "C" {

int hge_create(int32_t n_participants, int64_t capacity_events, int32_t device, uint32_t flags,
               hge_engine** out) {
  (void)flags;
  if (!out || n_participants < 1 || n_participants > 256) return HGE_ERR_ARG;
  hge_engine* h = new hge_engine();
  try {
    h->init(n_participants, capacity_events, device);
  } catch (Error& e) {
    fprintf(stderr, "hge_create: %s\n", e.msg.c_str());
    delete h;
    *out = nullptr;
    return e.code;
  }
  *out = h;
  return HGE_OK;
}

void hge_destroy(hge_engine* h) {
  delete h;
}

const char* hge_last_error(hge_engine* h) { return h ? h->err.c_str() : "null handle"; }

int hge_reset(hge_engine* h) {
  GUARD_BEGIN
  h->reset_state();
  return HGE_OK;
  GUARD_END(h)
}

int hge_insert_events(hge_engine* h, const hge_event* ev, int64_t n, int32_t* status_out,
                      int64_t* n_accepted) {
  GUARD_BEGIN
  REFUSE_IF_FAILED(h)
  const int64_t c0 = now_ns();
  int64_t acc = 0;
  int rc = HGE_OK;
  for (int64_t i = 0; i < n; i++) {
    const int32_t sp = ev[i].self_parent, op = ev[i].other_parent;
    int r = h->admit(ev[i], sp, op);
    if (r != HGE_OK) {
      if (status_out) status_out[i] = r;
      rc = r;
      break;
    }
    if (status_out) status_out[i] = (int32_t)h->strm.log.n_events;
    h->strm.log.append(ev[i], sp, op);
    acc++;
  }
  if (n_accepted) *n_accepted = acc;
  h->hp.insert_ns += now_ns() - c0;
  return rc;
  GUARD_END(h)
}

int hge_divide_rounds(hge_engine* h) {
  GUARD_BEGIN
  REFUSE_IF_FAILED(h)
  h->divide();
  return HGE_OK;
  GUARD_END(h)
}

int hge_decide_fame(hge_engine* h) {
  GUARD_BEGIN
  REFUSE_IF_FAILED(h)
    h->consensus_batch({h->cons.n_divided}, true, false, false, nullptr, nullptr);
  return HGE_OK;
  GUARD_END(h)
}

int hge_decide_round_received(hge_engine* h) {
  GUARD_BEGIN
  REFUSE_IF_FAILED(h)
    h->consensus_batch({h->cons.n_divided}, false, true, false, nullptr, nullptr);
  return HGE_OK;
  GUARD_END(h)
}

int hge_find_order(hge_engine* h, int32_t* ids_out, int64_t cap, int64_t* n_out) {
  GUARD_BEGIN
  REFUSE_IF_FAILED(h)
    std::vector<int32_t> order;
  h->consensus_batch({h->cons.n_divided}, false, true, true, &order, nullptr);
  for (int64_t i = 0; i < (int64_t)order.size() && i < cap && ids_out; i++) ids_out[i] = order[i];
  if (n_out) *n_out = (int64_t)order.size();
  return HGE_OK;
  GUARD_END(h)
}

int hge_run_consensus(hge_engine* h, int32_t* ids_out, int64_t cap, int64_t* n_out) {
  GUARD_BEGIN
  REFUSE_IF_FAILED(h)
  const int64_t c0 = now_ns();
  std::vector<int32_t> order;
  if (!h->online_fast(order)) {
    h->divide();
    h->consensus_batch({h->cons.n_divided}, true, true, true, &order, nullptr);
  }
  for (int64_t i = 0; i < (int64_t)order.size() && i < cap && ids_out; i++) ids_out[i] = order[i];
  if (n_out) *n_out = (int64_t)order.size();
  h->hp.calls++;
  h->hp.call_ns += now_ns() - c0;
  return HGE_OK;
  GUARD_END(h)
}

int hge_replay_prepare(hge_engine* h, const hge_event* ev, int64_t n_sub,
                       const int64_t* call_points, int64_t n_calls, int32_t* status_out) {
  GUARD_BEGIN
  if (n_sub < 0 || (n_sub > 0 && !ev) || n_calls < 0 || (n_calls > 0 && !call_points)) {
    h->err = "hge_replay_prepare: bad argument";
    return HGE_ERR_ARG;
  }
  // call points: strictly ascending submission counts in [1, n_sub]
  for (int64_t c = 0; c < n_calls; c++) {
    if (call_points[c] < 1 || call_points[c] > n_sub || (c > 0 && call_points[c] <= call_points[c - 1])) {
      h->err = "hge_replay_prepare: call points must be strictly ascending within [1, n_sub]";
      return HGE_ERR_ARG;
    }
  }
  h->reset_state();
  std::vector<int32_t> idmap(n_sub, -1);
  int64_t nc = 0;
  for (int64_t i = 0; i < n_sub; i++) {
    const int32_t s = ev[i].self_parent, o = ev[i].other_parent;
    int32_t sp = s < 0 ? HGE_NONE : (s < i && idmap[s] >= 0 ? idmap[s] : HGE_UNKNOWN);
    int32_t op = o < 0 ? HGE_NONE : (o < i && idmap[o] >= 0 ? idmap[o] : HGE_UNKNOWN);
    int r = h->admit(ev[i], sp, op);
    if (r == HGE_OK) {
      idmap[i] = (int32_t)h->strm.log.n_events;
      h->strm.log.append(ev[i], sp, op);
    }
    if (status_out) status_out[i] = r == HGE_OK ? idmap[i] : r;
    while (nc < n_calls && call_points[nc] == i + 1) {
      h->strm.replay_calls.push_back(h->strm.log.n_events);
      nc++;
    }
  }
  h->upload();
  h->ensure_pin_ord((size_t)h->strm.log.n_events);  // the replay's order is delivered here
  HGE_HIPCHK(hipStreamSynchronize(h->st));
  return HGE_OK;
  GUARD_END(h)
}

int hge_replay_run(hge_engine* h, int64_t* n_ordered) {
  GUARD_BEGIN
  REFUSE_IF_FAILED(h)
  h->strm.sp_active = false;
  if (h->rec_on) h->rec_dec.clear();
  struct Bulk {  // the coordinate step of this replay alone
    hge_engine* h;
    ~Bulk() { h->strm.rows_bulk = false; }
  } bulk{h};
  h->strm.rows_bulk = true;
  h->replay_begin();
  h->strm.rows_bulk = false;
  h->replay_end(n_ordered);
  if (h->rec_on) {  // hge_split_emulate: the rest of the record
    const int64_t E = h->strm.log.n_events;
    h->consensus_sync();
    h->rec_order = h->cons.consensus;
    h->rec_counts = h->cons.replay_counts;
    h->rec_rr.resize(E);
    h->rec_cts.resize(E);
    h->readback(h->rec_rr.data(), h->d_rr.p, (size_t)E);
    h->readback(h->rec_cts.data(), h->d_cts.p, (size_t)E);
    h->rec_left.resize(h->cons.n_und);
    if (h->cons.n_und) h->readback(h->rec_left.data(), h->d_und.p, (size_t)h->cons.n_und);
    h->rec_on = false;
    h->rec_have = true;
  }
  return HGE_OK;
  GUARD_END(h)
}

// ---- cross-GPU split of one hashgraph's rounds walk (babble_amd/dist.py) ----
int hge_split_plan(hge_engine* h, int32_t part, int32_t nparts, const int64_t* ev_bounds,
                   const int32_t* call_bounds, const int64_t* cand_lo) {
  if (!h) return HGE_ERR_ARG;
  GUARD_BEGIN
  if (nparts <= 1) {
    h->strm.sp = hge_engine::SplitPlan();
    return HGE_OK;
  }
  auto bad = [&](const char* why) {
    h->err = std::string("hge_split_plan: ") + why;
    return HGE_ERR_ARG;
  };
  if (h->N <= 32 || !h->direct_rounds() || h->strm.wide32 || h->strm.wide32_pending)
    return bad("needs the wide direct rounds path (N > 32, N % 4 == 0, chains below 65,535 events)");
  if (part < 0 || part >= nparts || !ev_bounds || !call_bounds || !cand_lo) return bad("bad argument");
  const int64_t E = h->strm.log.n_events;
  const int ncalls = (int)h->strm.replay_calls.size();
  if (ev_bounds[0] != 0 || ev_bounds[nparts] != E || call_bounds[0] != 0 || call_bounds[nparts] != ncalls)
    return bad("the bounds must cover the staged stream and its calls");
  for (int g = 0; g < nparts; g++) {
    if (ev_bounds[g + 1] < ev_bounds[g] || call_bounds[g + 1] <= call_bounds[g])
      return bad("bounds must ascend and every part needs a call");
    if (cand_lo[g] < 0 || cand_lo[g] > ev_bounds[g] || cand_lo[g] >= ev_bounds[g + 1])
      return bad("cand_lo[p] must lie in [0, ev_bounds[p]] below ev_bounds[p + 1]");
  }
  if (E > INT32_MAX) return bad("stream too long");
  h->strm.sp.part = part;
  h->strm.sp.nparts = nparts;
  h->strm.sp.a.assign(ev_bounds, ev_bounds + nparts + 1);
  h->strm.sp.cb.assign(call_bounds, call_bounds + nparts + 1);
  h->strm.sp.clo.assign(cand_lo, cand_lo + nparts);
  return HGE_OK;
  GUARD_END(h)
}

int hge_split_exchange(hge_engine* h, hge_exchange_fn fn, void* ctx) {
  if (!h) return HGE_ERR_ARG;
  h->x_fn = fn;
  h->x_ctx = ctx;
  return HGE_OK;
}

int hge_split_emulate(hge_engine* h, int32_t on) {
  if (!h) return HGE_ERR_ARG;
  h->rec_on = on != 0;
  h->rec_have = false;
  h->rec_dec.clear();
  return HGE_OK;
}

int hge_split_run(hge_engine* h, int64_t* n_ordered) {
  if (!h) return HGE_ERR_ARG;
  GUARD_BEGIN
  if (h->strm.sp.nparts <= 1) {
    h->err = "hge_split_run: no split plan (hge_split_plan)";
    return HGE_ERR_ARG;
  }
  if (!h->x_fn && !h->rec_have) {
    h->err = "hge_split_run: no exchange (hge_split_exchange) and no record (hge_split_emulate)";
    return HGE_ERR_ARG;
  }
  struct Off {  // the plan applies to this replay only
    hge_engine* h;
    ~Off() { h->strm.sp_active = false; }
  } off{h};
  h->strm.sp_active = true;
  h->replay_begin();
  h->replay_end(n_ordered);
  return HGE_OK;
  GUARD_END(h)
}

int hge_split_begin(hge_engine* h) {
  GUARD_BEGIN
  if (h->N <= 32 || !h->direct_rounds() || h->strm.wide32 || h->strm.wide32_pending) {
    h->err = "the split walk needs the wide direct rounds path (N > 32, N % 4 == 0)";
    return HGE_ERR_ARG;
  }
  h->strm.sp_active = false;  // the walk-only split: every part computes everything else
  h->replay_begin();
  if (!h->cons.cstep) {
    h->err = "nothing staged (hge_replay_prepare first)";
    return HGE_ERR_ARG;
  }
  return HGE_OK;
  GUARD_END(h)
}

int hge_frontier_guess(hge_engine* h, int32_t part, int32_t nparts, int32_t* start_out) {
  if (!h) return HGE_ERR_ARG;
  GUARD_BEGIN
  if (!start_out || nparts < 1 || part < 0 || part >= nparts) {
    h->err = "hge_frontier_guess: bad argument";
    return HGE_ERR_ARG;
  }
  // part 0: the true first frontier (every chain's first event); part p: the time
  // cut at event p * E / nparts (the first event of each chain inserted at or after it)
  // with a split plan of nparts parts: its event bound of the part
  const int64_t T = h->strm.sp.nparts == nparts ? h->strm.sp.a[part] : h->strm.log.n_events * (int64_t)part / nparts;
  for (int c = 0; c < h->N; c++) {
    const std::vector<int32_t>& ch = h->strm.log.h_chain[c];
    const size_t k = std::lower_bound(ch.begin(), ch.end(), (int32_t)T) - ch.begin();
    start_out[c] = k < ch.size() ? (int32_t)k : INF32;
  }
  return HGE_OK;
  GUARD_END(h)
}

int hge_frontier_walk(hge_engine* h, const int32_t* start, const int32_t* stopcut, int32_t extra,
                      int32_t hmax, int32_t* rows_out, uint64_t* ssc_out, int32_t* nrows,
                      int32_t* natural) {
  GUARD_BEGIN
  if (!h->cons.cstep || !start || hmax < 2) return HGE_ERR_ARG;
  const int N = h->N, NW = h->NW;
  h->s_hist.need((size_t)hmax * N + N);
  h->s_hssc.need((size_t)hmax * N * NW);
  h->s_hstate.need(N + 4);
  h->h2d(h->s_hstate.p, start, 4 * (size_t)N);
  int32_t* cut = nullptr;
  if (stopcut) {
    h->s_hist.need((size_t)hmax * N + 2 * N);
    cut = h->s_hist.p + (size_t)hmax * N + N;
    h->h2d(cut, stopcut, 4 * (size_t)N);
  }
  int32_t* rstate = h->s_hstate.p + N;
  HGE_HIPCHK(hipMemsetAsync(rstate, 0, 16, h->st));
  h->s_bar.need(2);
  h->s_gran.need(2 * (size_t)N);
  HGE_HIPCHK(hipMemsetAsync(h->s_bar.p, 0, 8, h->st));
  HGE_HIPCHK(hipMemsetAsync(h->s_gran.p, 0, 16 * (size_t)N, h->st));
  auto lk = h->frontier_lock();  // until the walk has drained (the sync below)
  Tables t = h->tables();
  const int32_t* olen = h->cons.cstep->olen;
  const int32_t* len = h->cons.cstep->len;
  int rlo = 0, Rprev = 0;
  const int32_t* rlo_dev = nullptr;
  uint64_t* gran = h->s_gran.p;
  int32_t* err = h->s_bar.p + 1;
  uint64_t* ssc = h->s_hssc.p;
  uint32_t* mb = h->walk_mb();
  unsigned long long* paths = h->walk_paths();
  unsigned long long* paths_next = h->s_wpaths.p + 2 * ((h->walk_seq + 1) & 1);
  uint64_t* dbg = nullptr;
  const int32_t* st0 = h->s_hstate.p;
  int32_t* hist = h->s_hist.p;
  int hm = hmax, ex = std::max(0, (int)extra), nostall = 0, force_exact = hge_engine::walk_force_exact();
  int nomflag = 0;
  void* args[] = {&t, &olen, &len, &rstate, &rlo, &rlo_dev, &Rprev, &gran, &err, &ssc, &mb, &dbg,
                  &st0, &hist, &hm, &cut, &ex, &nostall, &force_exact, &nomflag, &paths, &paths_next};
  h->prof.begin("k_rounds_direct_walk");
  HGE_HIPCHK(h->launch_resident(h->direct_fn(), dim3(N), dim3(1024), args));
  h->prof.end();
  int32_t rs[2] = {0, 0}, e = 0;
  h->d2h(rs, rstate, 8);
  h->d2h(&e, err, 4);
  h->sync();
  if (e) throw Error(HGE_ERR_DEVICE, "rounds frontier hand-off timed out");
  const int n = std::max(1, std::min(rs[0], hmax));
  if (rows_out) h->readback(rows_out, h->s_hist.p, (size_t)n * N);
  if (ssc_out) h->readback(ssc_out, h->s_hssc.p, (size_t)n * N * NW);
  if (nrows) *nrows = n;
  if (natural) *natural = rs[1] == 0 ? 1 : 0;
  return HGE_OK;
  GUARD_END(h)
}

int hge_frontier_rows(hge_engine* h, int32_t from, int32_t n, int32_t* rows_out, uint64_t* ssc_out) {
  GUARD_BEGIN
  const int N = h->N, NW = h->NW;
  if (from < 0 || n < 0 || (size_t)(from + n) * N > h->s_hist.n) return HGE_ERR_ARG;
  if (rows_out && n) h->d2h(rows_out, h->s_hist.p + (size_t)from * N, 4 * (size_t)n * N);
  if (ssc_out && n) h->d2h(ssc_out, h->s_hssc.p + (size_t)from * N * NW, 8 * (size_t)n * N * NW);
  h->sync();
  return HGE_OK;
  GUARD_END(h)
}

int hge_split_finish(hge_engine* h, const int32_t* rows, const uint64_t* ssc, int32_t nrows,
                     int32_t natural, int64_t* n_ordered) {
  GUARD_BEGIN
  if (!h->cons.cstep || !rows || nrows < 1 || (nrows > 1 && !ssc)) return HGE_ERR_ARG;
  const int N = h->N, NW = h->NW;
  h->cons.ext_on = true;
  h->cons.ext_natural = natural != 0;
  h->cons.ext_rows = nrows;
  h->cons.ext_C.assign(rows, rows + (size_t)nrows * N);
  h->cons.ext_ssc.assign((size_t)nrows * N * NW, 0);
  if (nrows > 1) std::copy(ssc + (size_t)N * NW, ssc + (size_t)nrows * N * NW, h->cons.ext_ssc.begin() + (size_t)N * NW);
  h->replay_end(n_ordered);
  return HGE_OK;
  GUARD_END(h)
}

int hge_replay_fetch(hge_engine* h, int32_t* order_out, int64_t cap, int64_t* call_counts_out) {
  GUARD_BEGIN
  if (order_out) {
    // the log's vector, then the delivered tail in the pinned buffer: one copy each
    const int64_t a = std::min<int64_t>((int64_t)h->cons.consensus.size(), std::max<int64_t>(cap, 0));
    if (a > 0) memcpy(order_out, h->cons.consensus.data(), 4 * (size_t)a);
    const int64_t b = std::min<int64_t>(h->cons.cons_pin_n, std::max<int64_t>(cap - a, 0));
    // (one copy thread moves ~12 GB/s: a 40 MB order takes 8 in parallel)
    const int nt = b >= (1 << 20) ? 8 : 1;
    std::vector<std::thread> th;
    for (int k = 1; k < nt; k++)
      th.emplace_back([=] {
        const int64_t lo = b * k / nt, hi = b * (k + 1) / nt;
        memcpy(order_out + a + lo, h->pin_ord.p + lo, 4 * (size_t)(hi - lo));
      });
    if (b > 0) memcpy(order_out + a, h->pin_ord.p, 4 * (size_t)(b / nt));
    for (auto& x : th) x.join();
  }
  if (call_counts_out)
    for (size_t c = 0; c < h->cons.replay_counts.size(); c++) call_counts_out[c] = h->cons.replay_counts[c];
  return HGE_OK;
  GUARD_END(h)
}

int hge_replay_order(hge_engine* h, const int32_t** ids, int64_t* n) {
  if (!h || !ids || !n) return HGE_ERR_ARG;
  GUARD_BEGIN
  if (!h->cons.consensus.empty() || !h->cons.cons_pin_n) h->consensus_sync();  // the whole log in one place
  if (h->cons.cons_pin_n) {
    *ids = h->pin_ord.p;
    *n = h->cons.cons_pin_n;
  } else {
    *ids = h->cons.consensus.data();
    *n = (int64_t)h->cons.consensus.size();
  }
  return HGE_OK;
  GUARD_END(h)
}

int hge_replay(hge_engine* h, const hge_event* ev, int64_t n_sub, const int64_t* call_points,
               int64_t n_calls, int32_t* status_out, int32_t* order_out, int64_t cap,
               int64_t* n_ordered, int64_t* call_counts_out) {
  int rc = hge_replay_prepare(h, ev, n_sub, call_points, n_calls, status_out);
  if (rc) return rc;
  rc = hge_replay_run(h, n_ordered);
  if (rc) return rc;
  return hge_replay_fetch(h, order_out, cap, call_counts_out);
}

int64_t hge_event_count(hge_engine* h) { return h->strm.log.n_events; }
int32_t hge_participants(hge_engine* h) { return h->N; }
int32_t hge_device(hge_engine* h) { return h->device; }
int32_t hge_rounds(hge_engine* h) { return std::max(h->cons.R_div, h->strm.R_set); }
int32_t hge_last_consensus_round(hge_engine* h) { return h->cons.lcr; }
int32_t hge_last_committed_round_events(hge_engine* h) { return h->cons.lcre; }
int64_t hge_consensus_transactions(hge_engine* h) { return h->cons.ctx; }
int64_t hge_consensus_count(hge_engine* h) { return h->consensus_size(); }
// RollingList window (common/rolling_list.go:55-67): Add rolls the list back to
// its last `size` items once it holds 2*size, so after `tot` adds it holds
static int64_t window_len(int64_t tot, int64_t size) {
  if (size <= 0 || tot <= 2 * size) return tot;
  return size + (tot - 2 * size - 1) % size + 1;
}
int64_t hge_consensus_events(hge_engine* h, int32_t* ids_out, int64_t cap) {
  try {
    h->consensus_sync();
  } catch (const Error& e) {
    h->err = e.msg;
    return -1;
  }
  const int64_t tot = (int64_t)h->cons.consensus.size(), w = window_len(tot, h->cache_size);
  for (int64_t i = 0; i < w && i < cap && ids_out; i++) ids_out[i] = h->cons.consensus[tot - w + i];
  return w;
}
int64_t hge_consensus_log(hge_engine* h, int64_t from, int32_t* ids_out, int64_t cap) {
  try {
    h->consensus_sync();
  } catch (const Error& e) {
    h->err = e.msg;
    return -1;
  }
  const int64_t tot = (int64_t)h->cons.consensus.size();
  if (from < 0) from = 0;
  for (int64_t i = from; i < tot && i - from < cap && ids_out; i++) ids_out[i - from] = h->cons.consensus[i];
  return std::max<int64_t>(0, tot - from);
}
int64_t hge_undetermined(hge_engine* h, int32_t* ids_out, int64_t cap) {
  try {
    if (ids_out && h->cons.n_und > 0) {
      int64_t m = std::min<int64_t>(cap, h->cons.n_und);
      h->readback(ids_out, h->d_und.p, m);
    }
  } catch (Error& e) {
    h->err = e.msg;
    return e.code;
  }
  return h->cons.n_und;
}
int hge_known(hge_engine* h, int32_t* counts_out) {
  for (int c = 0; c < h->N; c++) counts_out[c] = h->strm.log.chain_len[c];
  return HGE_OK;
}

static int32_t read1(hge_engine* h, const int32_t* p) {
  int32_t v = -1;
  h->readback(&v, p, 1);
  return v;
}

int32_t hge_round_of(hge_engine* h, int32_t id) {
  try {
    if (id < 0 || id >= h->strm.log.n_events) return -1;
    h->coords();
    return read1(h, h->d_round.p + id);
  } catch (Error& e) {
    h->err = e.msg;
    return e.code;
  }
}
int32_t hge_is_witness(hge_engine* h, int32_t id) {
  try {
    if (id < 0 || id >= h->strm.log.n_events) return 0;
    h->coords();
    uint8_t v = 0;
    h->readback(&v, h->d_wit.p + id, 1);
    return v;
  } catch (Error& e) {
    h->err = e.msg;
    return e.code;
  }
}
int32_t hge_round_witness(hge_engine* h, int32_t round, int32_t creator) {
  try {
    if (round < 0 || round >= h->cons.R || creator < 0 || creator >= h->N) return -1;
    int32_t w = read1(h, h->d_W.p + (size_t)round * h->N + creator);
    if (w >= h->cons.n_divided) return -1;
    return w;
  } catch (Error& e) {
    h->err = e.msg;
    return e.code;
  }
}
int32_t hge_fame(hge_engine* h, int32_t round, int32_t creator) {
  try {
    if (hge_round_witness(h, round, creator) < 0) return -1;
    uint8_t v = 0;
    h->readback(&v, h->d_fame.p + (size_t)round * h->N + creator, 1);
    return v;
  } catch (Error& e) {
    h->err = e.msg;
    return e.code;
  }
}
int32_t hge_round_events(hge_engine* h, int32_t round) {
  try {
    if (round < 0 || round >= h->cons.R) return 0;
    return read1(h, h->d_rcnt.p + round);
  } catch (Error& e) {
    h->err = e.msg;
    return e.code;
  }
}
// Store.GetRound's events (RoundInfo.Events, roundInfo.go:24-60): every event of
// round r in insertion order with its witness flag (the first event of round r is
// its first witness: ids below h_minw[r] are not scanned)
int hge_round_event_ids(hge_engine* h, int32_t round, int32_t* ids_out, uint8_t* witness_out, int64_t cap,
                        int64_t* n_out) {
  if (!h || !n_out) return HGE_ERR_ARG;
  GUARD_BEGIN
  *n_out = 0;
  h->coords();
  if (round < 0 || round >= h->cons.R || h->cons.n_coords == 0) return HGE_OK;
  const int64_t lo = round < (int)h->cons.h_minw.size() ? std::max<int64_t>(0, h->cons.h_minw[round]) : 0;
  const int64_t n = h->cons.n_coords - lo;
  if (n <= 0) return HGE_OK;
  std::vector<int32_t> rd((size_t)n);
  std::vector<uint8_t> wd((size_t)n);
  h->d2h(rd.data(), h->d_round.p + lo, 4 * (size_t)n);
  h->d2h(wd.data(), h->d_wit.p + lo, (size_t)n);
  h->sync();
  int64_t k = 0;
  for (int64_t i = 0; i < n; i++) {
    if (rd[(size_t)i] != round) continue;
    if (k < cap) {
      if (ids_out) ids_out[k] = (int32_t)(lo + i);
      if (witness_out) witness_out[k] = wd[(size_t)i];
    }
    k++;
  }
  *n_out = k;
  return HGE_OK;
  GUARD_END(h)
}

int32_t hge_round_received(hge_engine* h, int32_t id) {
  try {
    if (id < 0 || id >= h->strm.log.n_events) return -1;
    return read1(h, h->d_rr.p + id);
  } catch (Error& e) {
    h->err = e.msg;
    return e.code;
  }
}
int64_t hge_consensus_timestamp(hge_engine* h, int32_t id) {
  try {
    if (id < 0 || id >= h->strm.log.n_events) return 0;
    int64_t v = 0;
    h->readback(&v, h->d_cts.p + id, 1);
    return v;
  } catch (Error& e) {
    h->err = e.msg;
    return e.code;
  }
}

int hge_coordinates(hge_engine* h, int32_t id, int32_t* la_out, int32_t* fd_out) {
  GUARD_BEGIN
  if (id < 0 || id >= h->strm.log.n_events) return HGE_ERR_ARG;
  h->coords();
  const size_t off = ((size_t)h->strm.log.h_creator[id] * h->ccap + h->strm.log.h_index[id]) * h->N;
  if (la_out) {
    if (h->sweep16()) {  // N > 32: unpack the LA16 row (LA + 1 as uint16 pairs)
      const size_t w = (size_t)(h->N + 1) / 2;
      std::vector<uint32_t> row(w);
      h->readback(row.data(), h->d_LA16.p + ((size_t)h->strm.log.h_creator[id] * h->ccap + h->strm.log.h_index[id]) * w, w);
      for (int c = 0; c < h->N; c++) la_out[c] = (int32_t)((row[c >> 1] >> ((c & 1) * 16)) & 0xFFFFu) - 1;
    } else {
      h->readback(la_out, h->d_LA.p + off, h->N);
    }
  }
  if (fd_out && h->fdt16()) {  // packed rows: FD + 1, 0xFFFF = none
    std::vector<uint16_t> row(h->N);
    h->readback(row.data(), (const uint16_t*)h->d_FD.p + off, h->N);
    for (int c = 0; c < h->N; c++) fd_out[c] = row[c] == 0xFFFFu ? INF32 : (int32_t)row[c] - 1;
    return HGE_OK;
  }
  if (fd_out) h->readback(fd_out, h->d_FD.p + off, h->N);
  return HGE_OK;
  GUARD_END(h)
}

// predicates on the materialised coordinates (hashgraph.go:83-208)
int32_t hge_ancestor(hge_engine* h, int32_t x, int32_t y) {
  if (x < 0 || x >= h->strm.log.n_events || y < 0 || y >= h->strm.log.n_events) return 0;
  if (x == y) return 1;
  std::vector<int32_t> la(h->N);
  if (hge_coordinates(h, x, la.data(), nullptr)) return 0;
  return la[h->strm.log.h_creator[y]] >= h->strm.log.h_index[y] ? 1 : 0;
}
int32_t hge_self_ancestor(hge_engine* h, int32_t x, int32_t y) {
  if (x < 0 || x >= h->strm.log.n_events || y < 0 || y >= h->strm.log.n_events) return 0;
  if (x == y) return 1;
  return (h->strm.log.h_creator[x] == h->strm.log.h_creator[y] && h->strm.log.h_index[x] >= h->strm.log.h_index[y]) ? 1 : 0;
}
int32_t hge_see(hge_engine* h, int32_t x, int32_t y) { return hge_ancestor(h, x, y); }
int32_t hge_strongly_see(hge_engine* h, int32_t x, int32_t y) {
  if (x < 0 || x >= h->strm.log.n_events || y < 0 || y >= h->strm.log.n_events) return 0;
  std::vector<int32_t> la(h->N), fd(h->N);
  if (hge_coordinates(h, x, la.data(), nullptr)) return 0;
  if (hge_coordinates(h, y, nullptr, fd.data())) return 0;
  int c = 0;
  for (int i = 0; i < h->N; i++) c += la[i] >= fd[i];
  return c >= h->SM ? 1 : 0;
}
int32_t hge_oldest_self_ancestor_to_see(hge_engine* h, int32_t x, int32_t y) {
  if (x < 0 || x >= h->strm.log.n_events || y < 0 || y >= h->strm.log.n_events) return -1;
  std::vector<int32_t> fd(h->N);
  if (hge_coordinates(h, y, nullptr, fd.data())) return -1;
  const int cx = h->strm.log.h_creator[x];
  const int32_t a = fd[cx];
  if (a <= h->strm.log.h_index[x]) {
    try {
      return read1(h, h->d_chain.p + (size_t)cx * h->ccap + a);
    } catch (Error& e) {
      h->err = e.msg;
      return -1;
    }
  }
  return -1;
}

// ---- Store semantics and sync-path reads ----------------------------------
int hge_set_cache_size(hge_engine* h, int64_t size) {
  if (!h || size < 0) return HGE_ERR_ARG;
  h->cache_size = size;
  return HGE_OK;
}
int64_t hge_cache_size(hge_engine* h) { return h->cache_size; }

int hge_participant_events(hge_engine* h, int32_t creator, int64_t skip, int32_t* ids_out,
                           int64_t cap, int64_t* n_out) {
  if (n_out) *n_out = 0;
  if (creator < 0 || creator >= h->N) {
    h->err = "not found";
    return HGE_ERR_NOT_FOUND;
  }
  const std::vector<int32_t>& ch = h->strm.log.h_chain[creator];
  const int64_t tot = (int64_t)ch.size();
  if (skip >= tot) return HGE_OK;
  const int64_t oldest = tot - window_len(tot, h->cache_size);
  if (skip < oldest) {
    h->err = "too late";
    return HGE_ERR_TOO_LATE;
  }
  if (skip < 0) skip = 0;
  for (int64_t k = skip; k < tot && k - skip < cap && ids_out; k++) ids_out[k - skip] = ch[k];
  if (n_out) *n_out = tot - skip;
  return HGE_OK;
}

int32_t hge_participant_event(hge_engine* h, int32_t creator, int64_t index) {
  if (!h || creator < 0 || creator >= h->N) return HGE_ERR_NOT_FOUND;
  const std::vector<int32_t>& ch = h->strm.log.h_chain[creator];
  const int64_t tot = (int64_t)ch.size();
  // RollingList.GetItem (common/rolling_list.go:42-53): index < oldestCached (>= 0),
  // a negative index included, is ErrTooLate
  if (index < 0 || index < tot - window_len(tot, h->cache_size)) return HGE_ERR_TOO_LATE;
  if (index >= tot) return HGE_ERR_NOT_FOUND;
  return ch[index];
}

int32_t hge_last_from(hge_engine* h, int32_t creator) {
  if (creator < 0 || creator >= h->N) return HGE_ERR_NOT_FOUND;
  return h->strm.log.chain_last[creator];
}

int hge_diff(hge_engine* h, const int32_t* known, int32_t* ids_out, int64_t cap, int64_t* n_out) {
  if (n_out) *n_out = 0;
  if (!known) return HGE_ERR_ARG;
  std::vector<int32_t> ids;
  for (int c = 0; c < h->N; c++) {
    const std::vector<int32_t>& ch = h->strm.log.h_chain[c];
    const int64_t tot = (int64_t)ch.size(), skip = known[c];
    if (skip >= tot) continue;
    if (skip < tot - window_len(tot, h->cache_size)) {
      h->err = "too late";
      return HGE_ERR_TOO_LATE;
    }
    for (int64_t k = std::max<int64_t>(skip, 0); k < tot; k++) ids.push_back(ch[k]);
  }
  std::sort(ids.begin(), ids.end());  // ByTopologicalOrder: ids are insertion order
  for (int64_t i = 0; i < (int64_t)ids.size() && i < cap && ids_out; i++) ids_out[i] = ids[i];
  if (n_out) *n_out = (int64_t)ids.size();
  return HGE_OK;
}

int hge_wire_info(hge_engine* h, int32_t id, int32_t* out) {
  if (id < 0 || id >= h->strm.log.n_events || !out) return HGE_ERR_ARG;
  const int32_t sp = h->strm.log.h_sp[id], op = h->strm.log.h_op[id];
  out[0] = sp >= 0 ? h->strm.log.h_index[sp] : -1;
  out[1] = op >= 0 ? h->strm.log.h_creator[op] : -1;
  out[2] = op >= 0 ? h->strm.log.h_index[op] : -1;
  out[3] = h->strm.log.h_creator[id];
  return HGE_OK;
}

int hge_read_wire_parents(hge_engine* h, int32_t creator_id, int32_t self_parent_index,
                          int32_t other_parent_creator_id, int32_t other_parent_index,
                          int32_t* sp_out, int32_t* op_out) {
  if (creator_id < 0 || creator_id >= h->N) return HGE_ERR_NOT_FOUND;
  int32_t sp = HGE_NONE, op = HGE_NONE;
  if (self_parent_index >= 0) {
    sp = hge_participant_event(h, creator_id, self_parent_index);
    if (sp < 0) return sp;
  }
  if (other_parent_index >= 0) {
    op = hge_participant_event(h, other_parent_creator_id, other_parent_index);
    if (op < 0) return op;
  }
  if (sp_out) *sp_out = sp;
  if (op_out) *op_out = op;
  return HGE_OK;
}

// ---- bulk state reads ------------------------------------------------------
int hge_event_rounds(hge_engine* h, int32_t* round_out, uint8_t* witness_out, int64_t cap) {
  GUARD_BEGIN
  h->coords();
  const int64_t m = std::min<int64_t>(cap, h->strm.log.n_events);
  if (m > 0 && round_out) h->d2h(round_out, h->d_round.p, 4 * (size_t)m);
  if (m > 0 && witness_out) h->d2h(witness_out, h->d_wit.p, (size_t)m);
  h->sync();
  return HGE_OK;
  GUARD_END(h)
}

int hge_event_received(hge_engine* h, int32_t* rr_out, int64_t* cts_out, int64_t cap) {
  GUARD_BEGIN
  const int64_t m = std::min<int64_t>(cap, h->strm.log.n_events);
  if (m > 0 && rr_out) h->d2h(rr_out, h->d_rr.p, 4 * (size_t)m);
  if (m > 0 && cts_out) h->d2h(cts_out, h->d_cts.p, 8 * (size_t)m);
  h->sync();
  return HGE_OK;
  GUARD_END(h)
}

int hge_consensus_timestamp_sources(hge_engine* h, const int32_t* ids, int64_t n, int32_t* src_out) {
  if (!h || n < 0 || (n > 0 && (!ids || !src_out))) return HGE_ERR_ARG;
  GUARD_BEGIN
  if (n == 0) return HGE_OK;
  for (int64_t i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= h->strm.log.n_events) throw Error(HGE_ERR_ARG, "hge_consensus_timestamp_sources: unknown id");
  h->s_src.need((size_t)n * 2);
  h->h2d(h->s_src.p, ids, 4 * (size_t)n);
  hipLaunchKernelGGL(k_cts_source, dim3((unsigned)div_up(n, 4)), dim3(256), 0, h->st, h->tables(),
                     (const int32_t*)h->s_src.p, (int)n, (const int32_t*)h->d_rr.p, (const int64_t*)h->d_cts.p,
                     h->s_src.p + n);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) throw Error(HGE_ERR_DEVICE, std::string("launch k_cts_source: ") + hipGetErrorString(le));
  h->readback(src_out, h->s_src.p + n, (size_t)n);
  return HGE_OK;
  GUARD_END(h)
}

// FindOrder's records of the log range [from, from + cap) (hashgraph.go:723-760), read from
// persisted state (hge_engine::commit_records).  The log is not folded into its vector for
// this: a replay's tail is read where hge_replay_run delivered it.
int64_t hge_commit_records(hge_engine* h, int64_t from, int64_t cap, int32_t* ids_out, int32_t* rr_out,
                           int64_t* cts_out, int32_t* src_out) {
  if (!h) return HGE_ERR_ARG;
  GUARD_BEGIN
  if (from < 0 || cap < 0) throw Error(HGE_ERR_ARG, "hge_commit_records: negative range");
  const int64_t left = std::max<int64_t>(0, h->consensus_size() - from);
  const int64_t m = std::min(cap, left);
  if (m > 0) h->commit_records(from, m, ids_out, rr_out, cts_out, src_out);
  return left;
  GUARD_END(h)
}

// the batch an order call just committed (the log's last n entries) as records
static void batch_records(hge_engine* h, int64_t n, int64_t cap, int32_t* ids_out, int32_t* rr_out, int64_t* cts_out,
                          int32_t* src_out) {
  const int64_t m = std::min(std::max<int64_t>(cap, 0), n);
  if (m > 0) h->commit_records(h->consensus_size() - n, m, ids_out, rr_out, cts_out, src_out);
}

int hge_find_order_records(hge_engine* h, int64_t cap, int32_t* ids_out, int32_t* rr_out, int64_t* cts_out,
                           int32_t* src_out, int64_t* n_out) {
  if (!h) return HGE_ERR_ARG;
  int64_t n = 0;
  const int rc = hge_find_order(h, nullptr, 0, &n);
  if (rc != HGE_OK) return rc;
  GUARD_BEGIN
  batch_records(h, n, cap, ids_out, rr_out, cts_out, src_out);
  if (n_out) *n_out = n;
  return HGE_OK;
  GUARD_END(h)
}

int hge_run_consensus_records(hge_engine* h, int64_t cap, int32_t* ids_out, int32_t* rr_out, int64_t* cts_out,
                              int32_t* src_out, int64_t* n_out) {
  if (!h) return HGE_ERR_ARG;
  int64_t n = 0;
  const int rc = hge_run_consensus(h, nullptr, 0, &n);
  if (rc != HGE_OK) return rc;
  GUARD_BEGIN
  batch_records(h, n, cap, ids_out, rr_out, cts_out, src_out);
  if (n_out) *n_out = n;
  return HGE_OK;
  GUARD_END(h)
}

int32_t hge_fame_table(hge_engine* h, int32_t rounds, int8_t* fame_out) {
  if (!h) return HGE_ERR_ARG;
  GUARD_BEGIN
  const int R = std::min<int>(std::max(rounds, 0), std::min(h->cons.R, h->Rcap));
  if (R == 0 || !fame_out) return 0;
  const size_t n = (size_t)R * h->N;
  std::vector<int32_t> w(n);
  std::vector<uint8_t> f(n);
  h->d2h(w.data(), h->d_W.p, 4 * n);
  h->d2h(f.data(), h->d_fame.p, n);
  h->sync();
  for (size_t i = 0; i < n; i++)
    fame_out[i] = (w[i] >= 0 && w[i] < h->cons.n_divided) ? (int8_t)f[i] : (int8_t)-1;
  return R;
  GUARD_END(h)
}

// ---- round predicates (hashgraph.go:211-326) --------------------------------
int32_t hge_parent_round(hge_engine* h, int32_t x) {
  if (x < 0 || x >= h->strm.log.n_events) return -1;
  const int32_t sp = h->strm.log.h_sp[x], op = h->strm.log.h_op[x];
  if (sp < 0 && op < 0) return 0;
  if (sp < 0 || op < 0) return 0;  // a missing parent (GetEvent error) reads as 0
  const int32_t a = hge_round_of(h, sp), b = hge_round_of(h, op);
  return std::max(a, b);
}

int32_t hge_round_inc(hge_engine* h, int32_t x) {
  if (x < 0 || x >= h->strm.log.n_events) return 0;
  const int32_t pr = hge_parent_round(h, x);
  if (pr < 0 || hge_rounds(h) < pr + 1) return 0;
  try {
    h->coords();
    if (pr >= h->Rcap) return 0;
    std::vector<int32_t> w(h->N);
    h->readback(w.data(), h->d_W.p + (size_t)pr * h->N, h->N);
    int c = 0;
    for (int i = 0; i < h->N; i++)
      if (w[i] >= 0 && w[i] < h->strm.log.n_events) c += hge_strongly_see(h, x, w[i]);
    return c >= h->SM ? 1 : 0;
  } catch (Error& e) {
    h->err = e.msg;
    return 0;
  }
}

int hge_round_diff(hge_engine* h, int32_t x, int32_t y, int32_t* out) {
  if (x < 0 || x >= h->strm.log.n_events || y < 0 || y >= h->strm.log.n_events || !out) return HGE_ERR_ARG;
  const int32_t a = hge_round_of(h, x), b = hge_round_of(h, y);
  if (a < 0 || b < 0) return HGE_ERR_INTERNAL;
  *out = a - b;
  return HGE_OK;
}

int hge_set_round(hge_engine* h, int32_t round, const int32_t* ids, const uint8_t* witness,
                  const uint8_t* fame, int32_t n) {
  GUARD_BEGIN
  if (round < 0 || n < 0 || (n > 0 && !ids)) return HGE_ERR_ARG;
  h->coords();
  h->ensure_rcap((int64_t)round + 1);
  for (int32_t i = 0; i < n; i++) {
    const int32_t x = ids[i];
    if (x < 0 || x >= h->strm.log.n_events) return HGE_ERR_ARG;
    if (witness && !witness[i]) continue;
    const size_t slot = (size_t)round * h->N + h->strm.log.h_creator[x];
    h->h2d(h->d_W.p + slot, &ids[i], 4);
    const uint8_t f = fame ? fame[i] : 0;
    h->h2d(h->d_fame.p + slot, &f, 1);
    h->sync();
  }
  h->strm.R_set = std::max(h->strm.R_set, round + 1);
  return HGE_OK;
  GUARD_END(h)
}

int hge_set_profiling(hge_engine* h, int on) {
  h->prof.on = on != 0;
  return HGE_OK;
}

int hge_reset_kernel_stats(hge_engine* h) {
  h->prof.clear_stats();
  return HGE_OK;
}

int hge_kernel_stats(hge_engine* h, int k, char* name, int namecap, double* total_ms,
                     int64_t* launches) {
  const int n = (int)h->prof.names.size();
  if (k < 0 || k >= n) return n;
  if (name && namecap > 0) {
    snprintf(name, namecap, "%s", h->prof.names[k].c_str());
  }
  if (total_ms) *total_ms = h->prof.ms[k];
  if (launches) *launches = h->prof.cnt[k];
  return n;
}

int32_t hge_coordinate_sweeps(hge_engine* h) { return h ? h->n_sweeps : -1; }

int hge_walk_select_paths(hge_engine* h, int64_t* narrow, int64_t* exact) {
  GUARD_BEGIN
  unsigned long long v[2] = {0, 0};
  if (h->s_wpaths.p && h->walk_seq > 0) {
    h->d2h(v, h->s_wpaths.p + 2 * (h->walk_seq & 1), 16);
    h->sync();
  }
  if (narrow) *narrow = (int64_t)v[0];
  if (exact) *exact = (int64_t)v[1];
  return HGE_OK;
  GUARD_END(h)
}

int hge_sort_paths(hge_engine* h, int64_t* packed, int64_t* index) {
  GUARD_BEGIN
  unsigned long long v[2] = {0, 0};
  if (h->s_spaths.p && h->sort_counted) {
    h->d2h(v, h->s_spaths.p + 4 * (h->sort_seq & 1), 16);
    h->sync();
  }
  if (packed) *packed = (int64_t)v[0];
  if (index) *index = (int64_t)v[1];
  return HGE_OK;
  GUARD_END(h)
}

int64_t hge_host_syncs(hge_engine* h) { return h ? h->xfer.n_syncs : -1; }

int hge_stage_times(hge_engine* h, float* ms_out, int cap) {
  int n = std::min(cap, 7);
  for (int i = 0; i < n; i++) ms_out[i] = h->stage_ms[i];
  return n;
}

int64_t hge_frontier_fallbacks(hge_engine* h) {
  if (!h) return HGE_ERR_ARG;
  return h->n_frontier_fallbacks;
}

}  // extern "C"
