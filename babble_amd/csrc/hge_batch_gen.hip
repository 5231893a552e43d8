// hge_batch_gen.hip — the batch engine's device front: a batch's graphs generated,
// admitted and laid out in the staged tables by kernels, from a few parameters and a
// seed (hge_batch_generate).  Included by hge_batch.hip inside
// namespace hgb.
//
// The stream family is babble_amd/gossip.py's counter_gossip, restated word for word:
// every random decision is a word of _bytes32(seed, family, row), SplitMix64 keyed by
// seed, family, row and word, so a decision depends on (seed, step) alone.
//
//   kg_walk   one wave per graph, sequential over the honest steps.  Lane l computes the
//             draws of step t0 + l for 64 steps at once; the serial loop then keeps the
//             generator's chain state (lane c: chain c's length and head), builds each
//             submission and admits it with hge_batch::admit's rules in admit's order,
//             through a submission -> id map: the last GW entries in LDS, all of them in
//             global scratch.  A chunk of 64 submissions' / accepted events' structural
//             fields is buffered one per lane and stored coalesced.  Its counting
//             instance stores the map alone and gives the sizes the pools are laid
//             out from.
//   kg_fill   one thread per accepted event: timestamp, S, coin and the chain-layout
//             tables from the event's recorded step and kind; one thread per call: its
//             accepted count and graph.
//   kg_raw    hge_batch_submissions: one thread per submission of one graph, the
//             hge_event record as counter_gossip states it.

constexpr int GW = 256;   // the submission -> id map's window in LDS
constexpr int GLAG = 32;  // each chain's last positions kept for lagging other-parents (op_lag < GLAG)
constexpr int64_t G_TS_BASE = 1500000000000000000ll;  // gossip.py TS_BASE
enum { FAM_S = 1, FAM_HASH, FAM_TWIN_S, FAM_TWIN_HASH, FAM_DOOMED_S, FAM_DOOMED_HASH, FAM_STEP, FAM_CASCADE, FAM_FORKER };
enum { KIND_HONEST = 0, KIND_TWIN, KIND_REC1, KIND_REC2, KIND_REC3, KIND_REC3_LATE };

// one generated graph
struct GenG {
  uint64_t seed;
  uint64_t tf, tc;  // Bernoulli thresholds floor(p 2^32) of fork_p, cascade_p
  int64_t mo;       // its block of the map scratch (5 events entries: every step at most 5 submissions)
  int64_t so;       // its first submission in the per-submission pools
  int64_t k;        // RunConsensus after every k submissions and after the last
  int32_t events, forkers, op_lag, pad;
};

struct GenT {
  int N, ccap;
  const GenG* gg;
  const GDesc* gd;
  int32_t* map;  // [mo + i] accepted: id | creator << 24; refused: -1
  int32_t* cnt;  // [g][4] submissions, accepted events, longest chain
  // per submission [so + i]: the raw stream, step * 8 + kind, the admission result (id or
  // hge_status) and the accepted count after it
  int32_t *s_cr, *s_ix, *s_sp, *s_op, *s_step, *s_st, *s_acc;
  // the staged tables (BT's), and each accepted event's step * 8 + kind
  int32_t *cr, *ix, *sp, *op, *oc, *ntx, *estep, *clen, *chain, *ntxch, *cg;
  int64_t *ts, *tsch, *calls;
  uint64_t *S, *Sch;
  uint8_t* coin;
};

__device__ __forceinline__ uint64_t gen_base(uint64_t seed, int family) {
  return (seed * 0x100000001B3ull + (uint64_t)family * 0x9E3779B1ull) * 7919ull;
}
// word k of _bytes32(seed, family, .)[row]
__device__ __forceinline__ uint64_t gen_word(uint64_t base, uint64_t row, int k) {
  uint64_t z = row * 4 + (uint64_t)k + base + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// a 32-bit u mapped to [0, m)
__device__ __forceinline__ int gen_pick(uint32_t u, int m) { return (int)(((uint64_t)u * (uint32_t)m) >> 32); }

// the S / hash families, their row and the timestamp of a submission of `kind` at step t
__device__ __forceinline__ void gen_fields(int t, int kind, int& fs, int& fh, uint64_t& row, int64_t& ts) {
  const int place = kind <= KIND_REC2 ? kind : kind - 1;  // twin + 1, a record at place k + 2 + k
  ts = G_TS_BASE + 1000ll * t + place;
  row = (uint64_t)t;
  if (kind == KIND_HONEST) fs = FAM_S, fh = FAM_HASH;
  else if (kind == KIND_TWIN) fs = FAM_TWIN_S, fh = FAM_TWIN_HASH;
  else fs = FAM_DOOMED_S, fh = FAM_DOOMED_HASH, row = 4ull * t + (uint64_t)min(kind - 1, 3);
}

template <bool EMIT>
__global__ __launch_bounds__(64) void kg_walk(GenT t) {
  __shared__ int32_t win[GW];
  __shared__ int32_t ring[64 * GLAG];
  const int g = blockIdx.x, lane = threadIdx.x, N = t.N;
  const GenG p = t.gg[g];
  int32_t* gmap = t.map + p.mo;
  const int64_t so = p.so, eo = EMIT ? t.gd[g].eo : 0;

  // the forkers: the min(forkers, N) creators of smallest (score, creator)
  const uint64_t score = gen_word(gen_base(p.seed, FAM_FORKER), (uint64_t)lane, 0);
  int rank = 0;
  for (int c = 0; c < N; c++) {
    const uint64_t s = rl64(score, c);
    rank += s < score || (s == score && c < lane);
  }
  const uint64_t fmask = ballot(lane < N && rank < min(p.forkers, N));
  const uint64_t bstep = gen_base(p.seed, FAM_STEP), bcasc = gen_base(p.seed, FAM_CASCADE);

  // lane c: the generator's chain c (honest events: length, head's submission) and
  // admission's (known events, the last one's id)
  int glen = 0, ghead = -1, alen = 0, alast = -1;
  int nsub = 0, E = 0;
  // one chunk of submissions / of accepted events, an entry per lane
  int r_map = -1, r_cr = 0, r_ix = 0, r_sp = 0, r_op = 0, r_step = 0, r_st = 0, r_acc = 0;
  int e_cr = 0, e_ix = 0, e_sp = 0, e_op = 0, e_oc = 0, e_step = 0;

  auto flush_raw = [&](int base, int n) {
    if (lane < n) {
      gmap[base + lane] = r_map;
      if (EMIT) {
        const int64_t q = so + base + lane;
        t.s_cr[q] = r_cr;
        t.s_ix[q] = r_ix;
        t.s_sp[q] = r_sp;
        t.s_op[q] = r_op;
        t.s_step[q] = r_step;
        t.s_st[q] = r_st;
        t.s_acc[q] = r_acc;
      }
    }
    // the map's entries are read back (ld) once they have left the LDS window
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    wsync();
  };
  auto flush_ev = [&](int base, int n) {
    if (EMIT && lane < n) {
      const int64_t q = eo + base + lane;
      t.cr[q] = e_cr;
      t.ix[q] = e_ix;
      t.sp[q] = e_sp;
      t.op[q] = e_op;
      t.oc[q] = e_oc;
      t.estep[q] = e_step;
    }
  };
  // a parent given as a submission index, resolved as hge_batch::add resolves it: the
  // map's entry, HGE_NONE or HGE_UNKNOWN
  auto entry = [&](int s, int i) -> int {
    if (s < 0) return HGE_NONE;
    if (s >= i) return HGE_UNKNOWN;
    int e = i - s <= GW ? win[s & (GW - 1)] : ld(gmap + s);
    e = __builtin_amdgcn_readfirstlane(e);
    return e < 0 ? HGE_UNKNOWN : e;
  };
  // one submission: hge_batch::admit's rules in admit's order, then the bookkeeping
  auto submit = [&](int kind, int step, int c, int idx, int sp, int op) {
    const int i = nsub;
    const int esp = entry(sp, i), eop = entry(op, i);
    const int isp = esp < 0 ? esp : esp & 0xFFFFFF, iop = eop < 0 ? eop : eop & 0xFFFFFF;
    int r = HGE_OK;
    if (c < 0 || c >= N) {
      r = HGE_ERR_CREATOR;
    } else {
      const int known = rl(alen, c), last = rl(alast, c);
      if (isp == HGE_NONE && iop == HGE_NONE && known == 0) r = idx == 0 ? HGE_OK : HGE_ERR_INDEX;
      else if (isp < 0) r = HGE_ERR_SELF_PARENT_UNKNOWN;
      else if ((esp >> 24) != c) r = HGE_ERR_SELF_PARENT_CREATOR;
      else if (iop < 0) r = HGE_ERR_OTHER_PARENT_UNKNOWN;
      else if (isp != last) r = HGE_ERR_SELF_PARENT_NOT_LAST;
      else if (idx != known) r = HGE_ERR_INDEX;
    }
    int me = -1;
    if (r == HGE_OK) {
      const int id = E;
      me = id | c << 24;
      if (lane == c) {
        alen++;
        alast = id;
      }
      if (EMIT && lane == (id & 63)) {
        e_cr = c;
        e_ix = idx;
        e_sp = isp;
        e_op = iop;
        e_oc = iop >= 0 ? eop >> 24 : 0;
        e_step = step * 8 + kind;
      }
      E++;
      if ((E & 63) == 0) flush_ev(E - 64, 64);
    }
    win[i & (GW - 1)] = me;
    if (lane == (i & 63)) {
      r_map = me;
      if (EMIT) {
        r_cr = c;
        r_ix = idx;
        r_sp = sp;
        r_op = op;
        r_step = step * 8 + kind;
        r_st = r == HGE_OK ? E - 1 : r;
        r_acc = E;
      }
    }
    nsub++;
    if ((nsub & 63) == 0) flush_raw(nsub - 64, 64);
  };

  const int events = p.events;
  for (int t0 = 0; t0 < events; t0 += 64) {
    // the draws of steps t0 .. t0 + 63, lane l those of step t0 + l, packed in two words
    const uint64_t tl = (uint64_t)(t0 + lane);
    const uint64_t w0 = gen_word(bstep, tl, 0), w1 = gen_word(bstep, tl, 1);
    const uint64_t c0 = gen_word(bcasc, tl, 0), c1 = gen_word(bcasc, tl, 1), c2w = gen_word(bcasc, tl, 2);
    const int da = gen_pick((uint32_t)(w0 >> 32), N);
    int db = da;
    if (N > 1) {
      db = gen_pick((uint32_t)w0, N - 1);
      db += db >= da;
    }
    const int dlag = gen_pick((uint32_t)(w1 >> 32), p.op_lag + 1);
    const bool dfork = (fmask >> da & 1) && (uint64_t)(uint32_t)w1 < p.tf;
    const bool dcasc = N > 1 && (c0 >> 32) < p.tc;
    int dc2 = gen_pick((uint32_t)c0, N - 1);
    dc2 += dc2 >= da;
    int dother = gen_pick((uint32_t)c1, N - 1);
    dother += dother >= da;
    int dc3 = gen_pick((uint32_t)c2w, N - 2);
    dc3 += dc3 >= min(da, dc2);
    dc3 += dc3 >= max(da, dc2);
    const bool df2 = c1 >> 63, df3 = (c2w >> 63) && N > 2;
    const int d0 = da | db << 6 | dlag << 12 | (dc2 & 63) << 17 | (dother & 63) << 23;
    const int d1 = (dc3 & 63) | dfork << 6 | dcasc << 7 | df2 << 8 | df3 << 9;

    const int nl = min(64, events - t0);
    for (int l = 0; l < nl; l++) {
      const int step = t0 + l;
      const int x0 = rl(d0, l), x1 = rl(d1, l);
      int c, idx, sp, op;
      if (step < N) {  // the initial events
        c = step;
        idx = 0;
        sp = op = HGE_NONE;
      } else {
        const int b = x0 >> 6 & 63, lag = x0 >> 12 & 31;
        c = x0 & 63;
        idx = rl(glen, c);
        sp = rl(ghead, c);
        const int lb = rl(glen, b), pos = max(0, lb - 1 - lag);
        op = pos == lb - 1 ? rl(ghead, b) : __builtin_amdgcn_readfirstlane(ring[b * GLAG + (pos & (GLAG - 1))]);
      }
      ring[c * GLAG + (idx & (GLAG - 1))] = nsub;
      if (lane == c) {
        glen++;
        ghead = nsub;
      }
      submit(KIND_HONEST, step, c, idx, sp, op);
      if (step >= N && (x1 >> 6 & 1)) {
        const int twin = nsub;
        submit(KIND_TWIN, step, c, idx, sp, op);
        if (x1 >> 7 & 1) {
          const int c2 = x0 >> 17 & 63, rec1 = nsub, l2 = rl(glen, c2);
          const bool late = x1 >> 8 & 1;
          submit(KIND_REC1, step, c2, l2, rl(ghead, c2), twin);
          if (late) submit(KIND_REC2, step, c2, l2 + 1, rec1, rl(ghead, x0 >> 23 & 63));
          if (x1 >> 9 & 1) {
            const int c3 = x1 & 63;
            submit(late ? KIND_REC3_LATE : KIND_REC3, step, c3, rl(glen, c3), rl(ghead, c3), rec1);
          }
        }
      }
    }
  }
  flush_raw(nsub & ~63, nsub & 63);
  flush_ev(E & ~63, E & 63);
  if (EMIT) {
    if (lane < N) t.clen[(int64_t)g * N + lane] = alen;
  } else {
    const int longest = wave_max(lane < N ? alen : 0);
    if (lane == 0) {
      t.cnt[g * 4 + 0] = nsub;
      t.cnt[g * 4 + 1] = E;
      t.cnt[g * 4 + 2] = longest;
      t.cnt[g * 4 + 3] = 0;
    }
  }
}

// grid (ceil(max(Emax, Kmax) / 256), graphs): thread x is accepted event x and call x
__global__ __launch_bounds__(256) void kg_fill(GenT t) {
  const int g = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
  const GDesc d = t.gd[g];
  const GenG p = t.gg[g];
  if (x < d.E) {
    const int64_t q = d.eo + x;
    const int step = t.estep[q];
    int fs, fh;
    uint64_t row;
    int64_t ts;
    gen_fields(step >> 3, step & 7, fs, fh, row, ts);
    const uint64_t bs = gen_base(p.seed, fs);
    const uint64_t s0 = gen_word(bs, row, 0);
    t.ts[q] = ts;
    t.S[4 * q] = s0;
    for (int k = 1; k < 4; k++) t.S[4 * q + k] = gen_word(bs, row, k);
    t.coin[q] = (gen_word(gen_base(p.seed, fh), row, 2) >> 56) != 0;  // hash[16] != 0
    t.ntx[q] = 1;
    const int64_t slot = ((int64_t)g * t.N + t.cr[q]) * t.ccap + t.ix[q];  // an accepted event's index is its position
    t.chain[slot] = x;
    t.tsch[slot] = ts;
    t.Sch[slot] = s0;
    t.ntxch[slot] = 1;
  }
  if (x < d.K) {
    const int nsub = t.cnt[g * 4];
    const int64_t pt = min(((int64_t)x + 1) * p.k, (int64_t)nsub);
    t.calls[d.co + x] = t.s_acc[p.so + pt - 1];
    t.cg[d.co + x] = g;
  }
}

// graph g's submissions as hge_event records (reserved: the submission's kind)
__global__ __launch_bounds__(256) void kg_raw(GenT t, int g, hge_event* out) {
  const GenG p = t.gg[g];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= t.cnt[g * 4]) return;
  const int64_t q = p.so + i;
  const int step = t.s_step[q];
  int fs, fh;
  uint64_t row;
  int64_t ts;
  gen_fields(step >> 3, step & 7, fs, fh, row, ts);
  hge_event e;
  e.creator = t.s_cr[q];
  e.index = t.s_ix[q];
  e.self_parent = t.s_sp[q];
  e.other_parent = t.s_op[q];
  e.timestamp_ns = ts;
  const uint64_t bs = gen_base(p.seed, fs), bh = gen_base(p.seed, fh);
  for (int k = 0; k < 4; k++) {
    const uint64_t ws = gen_word(bs, row, k), wh = gen_word(bh, row, k);
    for (int b = 0; b < 8; b++) {  // big-endian
      e.s[8 * k + b] = (uint8_t)(ws >> (56 - 8 * b));
      e.hash[8 * k + b] = (uint8_t)(wh >> (56 - 8 * b));
    }
  }
  e.n_tx = 1;
  e.reserved = step & 7;
  out[i] = e;
}
