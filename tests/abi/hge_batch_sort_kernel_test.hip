// hge_batch_sort_kernel_test.hip — the batch engine's call-bucket sorts (kb_sort<64, 0,
// 1024>, kb_sort<256, 0, 1024> and kb_sort<256, 1024, 4096>, each with and without
// delivery: hge_batch_bulk.hip, through hge_batch.hip included as it is) driven directly
// on a work list of synthetic buckets over three graphs, against std::sort over the full
// key with the order written out in hge_sort_cases.h.  The sizes sit on the switches at
// 1,024 and 4,096 keys (past 4,096 the last class sorts in HBM); the spans sit on the
// prefix rule (a round span under 16 and a timestamp span under 2^28 ns) and beyond it,
// up to timestamps 2^63 ns and more apart.
//
//   hge_batch_sort_kernel_test          every instance as a run launches it, every slot compared
//   hge_batch_sort_kernel_test --host   the generator and the host models only (no device)
//
// The tables hold only what kb_sort reads: wlc, wl, gd[].eo, krr, kct, ks0, kid, S,
// order, and with delivery ord_rr / ord_cts (null pointers without it).
#include "hge_batch.hip"

#include "hge_sort_cases.h"

#define HIPCHK(e)                                                                               \
  do {                                                                                          \
    hipError_t e_ = (e);                                                                        \
    if (e_ != hipSuccess) {                                                                     \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #e, hipGetErrorString(e_));        \
      exit(2);                                                                                  \
    }                                                                                           \
  } while (0)

namespace {

using namespace sortcase;

constexpr int32_t kSentinel = 0x5E5E5E5E;  // an output slot no launch may have touched
constexpr int64_t kSentinel64 = 0x5E5E5E5E5E5E5E5Ell;
constexpr int kFirstCap = 1024, kLdsCap = 4096;  // the size switches, as documented
constexpr int kGraphs = 3;

const int kSizes[] = {1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5000, 8192, 8193};

enum Kind { kPlain = 0, kR15, kR16, kR40, kTBelow, kTAt, kMinMax, kFar, kEqual, kNKinds };
const char* const kKindName[kNKinds] = {"plain", "round_span_15", "round_span_16", "round_span_40", "cts_span_2p28_less_1",
                                        "cts_span_2p28", "cts_min_max", "cts_span_past_2p63", "equal_prefix"};

std::vector<Key> generate(int kind, int n, Rng& g) {
  const int64_t c0 = 1700000000000000000ll;
  std::vector<Key> k;
  switch (kind) {
    case kPlain: k = gen_plain(n, g); break;
    case kR15: k = gen_span(n, 200, 15, c0, 1ull << 20, g); break;
    case kR16: k = gen_span(n, 200, 16, c0, 1ull << 20, g); break;
    case kR40: k = gen_span(n, 200, 40, c0, 1ull << 20, g); break;
    case kTBelow: k = gen_span(n, 200, 2, c0, (1ull << 28) - 1, g); break;
    case kTAt: k = gen_span(n, 200, 2, c0, 1ull << 28, g); break;
    case kMinMax: k = gen_sign(n, g); break;
    case kFar:  // one timestamp at -8e18 beside real-clock ones spread over 2^40 ns: 2^63 ns and more apart
      for (int i = 0; i < n; i++) k.push_back(random_key(g, 300 + (uint32_t)g.below(3), c0 + (int64_t)g.below(1ull << 40)));
      if (n >= 2) k[0].cts = -8000000000000000000ll;
      break;
    default: k = gen_equal(n, g); break;
  }
  shuffle(k, g);
  return k;
}

struct Bucket {
  int n = 0, kind = 0, g = 0, base = 0;
  std::vector<Key> keys;      // input order
  std::vector<int> want;      // input positions in the order of ref_less
  bool fits = false;          // by the documented rule, of a bucket of up to 4,096 keys
};

// What kb_sort would give under a reading of its rules (0: all right): the 64-bit prefix
//   (rr - rmin) << 60 | (cts - cmin) << 32 | S >> 32   where the bucket fits, else 0,
// then the full key.  Past 4,096 keys the full key alone.
enum Reading { kRight = 0, kCtsUnsigned, kTiesById, kRound16, kSpanAt, kSpanWrapped, kNReadings };
const char* const kReadingName[kNReadings] = {"right", "cts_unsigned", "ties_by_id", "fits_round_span_16", "fits_cts_span_2p28",
                                              "cts_span_wrapped"};

bool fits_under(const std::vector<Key>& k, int reading, uint32_t& rmn, int64_t& cmn) {
  uint32_t rmx = k[0].rr;
  int64_t cmx = k[0].cts;
  rmn = rmx, cmn = cmx;
  for (const Key& x : k) {
    rmn = std::min(rmn, x.rr), rmx = std::max(rmx, x.rr);
    cmn = std::min(cmn, x.cts), cmx = std::max(cmx, x.cts);
  }
  const uint32_t rspan = rmx - rmn;
  const uint64_t cspan = (uint64_t)cmx - (uint64_t)cmn;  // the true span: up to 2^64 - 1
  const bool rfit = reading == kRound16 ? rspan <= 16 : rspan < 16;
  bool cfit = reading == kSpanAt ? cspan <= (1ull << 28) : cspan < (1ull << 28);
  if (reading == kSpanWrapped) cfit = (int64_t)cspan < ((int64_t)1 << 28);  // a span past 2^63 reads negative
  return rfit && cfit;
}

std::vector<int> model_sort(const Bucket& B, int reading, long* eqpairs = nullptr) {
  const int cmp = reading == kCtsUnsigned ? kCmpCtsUnsigned : reading == kTiesById ? kCmpIdAfterLimb0 : kCmpRight;
  std::vector<uint64_t> pre((size_t)B.n, 0);
  uint32_t rmn;
  int64_t cmn;
  if (B.n <= kLdsCap && fits_under(B.keys, reading, rmn, cmn))
    for (int i = 0; i < B.n; i++) {
      const Key& x = B.keys[i];
      pre[i] = ((uint64_t)(x.rr - rmn) << 60) | (((uint64_t)x.cts - (uint64_t)cmn) << 32) | (x.s[0] >> 32);
    }
  std::vector<int> ix;
  for (int i = 0; i < B.n; i++) ix.push_back(i);
  std::sort(ix.begin(), ix.end(), [&](int x, int y) {
    if (pre[x] != pre[y]) return pre[x] < pre[y];
    return mode_less(B.keys[x], B.keys[y], cmp);
  });
  for (int i = 0; i + 1 < B.n && eqpairs; i++) *eqpairs += pre[ix[i]] == pre[ix[i + 1]];
  return ix;
}

struct Cases {
  std::vector<Bucket> bk;
  int64_t eo[kGraphs];
  int E[kGraphs];
  int64_t Etot = 0;  // events of the pools, the slots between the graphs included
  long keys = 0;
};

Cases make_cases() {
  Cases C;
  Rng g{0xBA7C4ull};
  int pos[kGraphs] = {3, 0, 11};  // slots before a graph's first bucket
  for (int kind = 0; kind < kNKinds; kind++)
    for (int n : kSizes) {
      Bucket B;
      B.n = n, B.kind = kind, B.g = (int)(C.bk.size() % kGraphs);
      pos[B.g] += (int)(C.bk.size() % 5);  // slots between the buckets
      B.base = pos[B.g];
      B.keys = generate(kind, n, g);
      deal_ids(B.keys, (uint32_t)B.base, g);  // graph-local ids, unique in the graph
      for (int i = 0; i < n; i++) B.want.push_back(i);
      std::sort(B.want.begin(), B.want.end(), [&](int x, int y) { return ref_less(B.keys[x], B.keys[y]); });
      uint32_t rmn;
      int64_t cmn;
      B.fits = n <= kLdsCap && fits_under(B.keys, kRight, rmn, cmn);
      pos[B.g] += n;
      C.keys += n;
      C.bk.push_back(std::move(B));
    }
  // irregular graph offsets: the first graph does not start the pools, and the graphs do not touch
  int64_t at = 13;
  for (int q = 0; q < kGraphs; q++) {
    C.eo[q] = at;
    C.E[q] = pos[q] + 6;
    at += C.E[q] + 29 * (q + 1);
  }
  C.Etot = at;
  return C;
}

int run_host(const Cases& C) {
  struct Stat {
    long buckets = 0, keys = 0, eqpairs = 0, fit = 0, unfit = 0, hbm = 0;
    long differ[kNReadings] = {0, 0, 0, 0, 0, 0};
  };
  std::vector<Stat> st(kNKinds);
  for (const Bucket& B : C.bk) {
    Stat& s = st[B.kind];
    s.buckets++, s.keys += B.n;
    if (model_sort(B, kRight, B.n <= kLdsCap && B.fits ? &s.eqpairs : nullptr) != B.want) {
      printf("n=%d kind=%s: the host model of the sort differs from std::sort over the full key\n", B.n, kKindName[B.kind]);
      return 1;
    }
    if (B.n > kLdsCap) s.hbm++;
    else (B.fits ? s.fit : s.unfit)++;
    const bool on[kNReadings] = {false, B.kind == kMinMax, B.kind == kEqual, B.kind == kR16, B.kind == kTAt,
                                 B.kind == kMinMax || B.kind == kFar};
    for (int r = 1; r < kNReadings; r++)
      if (on[r]) s.differ[r] += model_sort(B, r) != B.want;
  }
  long total = 0;
  for (int kind = 0; kind < kNKinds; kind++) {
    const Stat& s = st[kind];
    printf("host kind=%s buckets=%ld keys=%ld eqpairs=%ld fits=%ld unfit=%ld hbm=%ld", kKindName[kind], s.buckets, s.keys, s.eqpairs,
           s.fit, s.unfit, s.hbm);
    for (int r = 1; r < kNReadings; r++) printf(" differ_%s=%ld", kReadingName[r], s.differ[r]);
    printf("\n");
    total += s.keys;
    bool ok = s.buckets > 0 && s.hbm > 0;
    if (kind == kPlain || kind == kR15 || kind == kTBelow || kind == kEqual) ok = ok && s.fit > 0 && s.unfit == 0;
    if (kind == kR16) ok = ok && s.unfit > 0 && s.differ[kRound16] > 0;
    if (kind == kR40) ok = ok && s.unfit > 0;
    if (kind == kTAt) ok = ok && s.unfit > 0 && s.differ[kSpanAt] > 0;
    if (kind == kMinMax) ok = ok && s.unfit > 0 && s.differ[kCtsUnsigned] > 0 && s.differ[kSpanWrapped] > 0;
    if (kind == kFar) ok = ok && s.unfit > 0 && s.differ[kSpanWrapped] > 0;
    if (kind == kEqual) ok = ok && s.eqpairs > 0 && s.differ[kTiesById] > 0;
    if (!ok) {
      printf("kind=%s: the generator does not give what the kind promises\n", kKindName[kind]);
      return 1;
    }
  }
  printf("ok %ld\n", total);
  return 0;
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
template <typename T>
void put(T* d, const std::vector<T>& v) {
  HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}

struct Form {
  const char* name;
  int cls;  // 0: <64, 0, 1024>, 1: <256, 0, 1024>, 2: <256, 1024, 4096>
  bool dlv;
};
const Form kForms[6] = {{"kb_sort<64,0,1024>", 0, false},   {"kb_sort<64,0,1024>", 0, true},    {"kb_sort<256,0,1024>", 1, false},
                        {"kb_sort<256,0,1024>", 1, true},   {"kb_sort<256,1024,4096>", 2, false}, {"kb_sort<256,1024,4096>", 2, true}};

int run_device(const Cases& C) {
  using namespace hgb;
  Rng g{0xD1Full};
  const size_t E = (size_t)C.Etot;
  // the key pools ([2 eo + k]) and S ([eo + x][4]); outside the buckets values of no key
  std::vector<int32_t> krr(2 * E), kid(2 * E);
  std::vector<int64_t> kct(2 * E);
  std::vector<uint64_t> ks0(2 * E), S(4 * E);
  for (size_t q = 0; q < 2 * E; q++) krr[q] = (int32_t)g.below(1000), kid[q] = 0, kct[q] = (int64_t)g.next(), ks0[q] = g.next();
  for (auto& v : S) v = g.next();
  std::vector<int4> wl;
  for (const Bucket& B : C.bk) {
    const int64_t eo = C.eo[B.g], so = 2 * eo + B.base;
    if (B.base < 0 || B.base + B.n > C.E[B.g] || (size_t)(so + B.n) > 2 * E || (size_t)(eo + B.base + B.n) > E) {
      printf("bucket of %d keys: out of the pools' bounds\n", B.n);
      return 1;
    }
    for (int i = 0; i < B.n; i++) {
      const Key& x = B.keys[i];
      krr[(size_t)so + i] = (int32_t)x.rr;
      kct[(size_t)so + i] = x.cts;
      ks0[(size_t)so + i] = x.s[0];
      kid[(size_t)so + i] = (int32_t)x.id;
      for (int l = 0; l < 4; l++) S[((size_t)eo + x.id) * 4 + l] = x.s[l];
    }
    wl.push_back(make_int4(B.g, B.n, B.base, 0));
  }
  std::vector<int> perm(wl.size());  // the work list in no order; perm[w] = the bucket of entry w
  for (size_t i = 0; i < perm.size(); i++) perm[i] = (int)i;
  for (size_t i = perm.size(); i > 1; i--) std::swap(perm[i - 1], perm[g.below(i)]);
  std::vector<int4> wls;
  for (int b : perm) wls.push_back(wl[(size_t)b]);
  std::vector<GDesc> gd(kGraphs, GDesc{});
  for (int q = 0; q < kGraphs; q++) gd[q].eo = C.eo[q], gd[q].E = C.E[q];
  BT t;
  memset(&t, 0, sizeof(t));
  t.N = 4, t.SM = 3, t.ccap = 1;
  GDesc* d_gd = upload(gd);
  int4* d_wl = upload(wls);
  int32_t* d_wlc = upload(std::vector<int32_t>{(int32_t)wls.size()});
  int32_t *d_krr = upload(krr), *d_kid = upload(kid);
  int64_t* d_kct = upload(kct);
  uint64_t *d_ks0 = upload(ks0), *d_S = upload(S);
  int32_t *d_order = nullptr, *d_orr = nullptr;
  int64_t* d_octs = nullptr;
  HIPCHK(hipMalloc(&d_order, E * sizeof(int32_t)));
  HIPCHK(hipMalloc(&d_orr, E * sizeof(int32_t)));
  HIPCHK(hipMalloc(&d_octs, E * sizeof(int64_t)));
  t.gd = d_gd, t.wl = d_wl, t.wlc = d_wlc, t.krr = d_krr, t.kid = d_kid, t.kct = d_kct, t.ks0 = d_ks0, t.S = d_S, t.order = d_order;
  std::vector<int32_t> order(E), orr(E);
  std::vector<int64_t> octs(E);
  long total = 0;
  for (const Form& f : kForms) {
    put(d_krr, krr), put(d_kid, kid), put(d_kct, kct), put(d_ks0, ks0);  // (the HBM sort moves the keys)
    HIPCHK(hipMemset(d_order, 0x5E, E * sizeof(int32_t)));
    HIPCHK(hipMemset(d_orr, 0x5E, E * sizeof(int32_t)));
    HIPCHK(hipMemset(d_octs, 0x5E, E * sizeof(int64_t)));
    t.ord_rr = f.dlv ? d_orr : nullptr;
    t.ord_cts = f.dlv ? d_octs : nullptr;
    // grids smaller than the work list; the classes as a run launches them: the first with last = 0
    if (f.cls == 0) f.dlv ? kb_sort<64, 0, 1024, true><<<dim3(24), dim3(64)>>>(t, 0) : kb_sort<64, 0, 1024, false><<<dim3(24), dim3(64)>>>(t, 0);
    else if (f.cls == 1) f.dlv ? kb_sort<256, 0, 1024, true><<<dim3(24), dim3(256)>>>(t, 0) : kb_sort<256, 0, 1024, false><<<dim3(24), dim3(256)>>>(t, 0);
    else f.dlv ? kb_sort<256, 1024, 4096, true><<<dim3(16), dim3(256)>>>(t, 1) : kb_sort<256, 1024, 4096, false><<<dim3(16), dim3(256)>>>(t, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(order.data(), d_order, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(orr.data(), d_orr, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(octs.data(), d_octs, E * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::vector<uint8_t> covered(E, 0);
    long buckets = 0, keys = 0, packed = 0, index = 0, hbm = 0;
    for (const Bucket& B : C.bk) {
      const bool live = f.cls == 2 ? B.n > kFirstCap : B.n <= kFirstCap;
      if (live) {
        buckets++, keys += B.n;
        if (B.n > kLdsCap) hbm++;
        else (B.fits ? packed : index)++;
      }
      const size_t o = (size_t)(C.eo[B.g] + B.base);
      for (int i = 0; i < B.n; i++) {
        covered[o + i] = 1;
        const Key& w = B.keys[(size_t)B.want[i]];
        const int32_t e = live ? (int32_t)w.id : kSentinel, v = order[o + i];
        if (v != e) {
          printf("MISMATCH %s dlv=%d: a bucket of %d keys, kind %s, graph %d, slot %d: got id %d want id %d%s\n", f.name, (int)f.dlv,
                 B.n, kKindName[B.kind], B.g, i, v, e, live ? "" : " (a bucket this launch must leave alone)");
          return 1;
        }
        const int32_t er = live && f.dlv ? (int32_t)w.rr : kSentinel;
        const int64_t ec = live && f.dlv ? w.cts : kSentinel64;
        if (orr[o + i] != er || octs[o + i] != ec) {
          printf("MISMATCH %s dlv=%d: a bucket of %d keys, kind %s, graph %d, slot %d (id %d): the record is (%d, %lld), want (%d, %lld)\n",
                 f.name, (int)f.dlv, B.n, kKindName[B.kind], B.g, i, v, orr[o + i], (long long)octs[o + i], er, (long long)ec);
          return 1;
        }
      }
    }
    for (size_t q = 0; q < E; q++)
      if (!covered[q] && (order[q] != kSentinel || orr[q] != kSentinel || octs[q] != kSentinel64)) {
        printf("MISMATCH %s dlv=%d: slot %zu outside every bucket was written\n", f.name, (int)f.dlv, q);
        return 1;
      }
    printf("case %s dlv=%d buckets=%ld keys=%ld packed=%ld index=%ld hbm=%ld slots=%zu\n", f.name, (int)f.dlv, buckets, keys, packed,
           index, hbm, (f.dlv ? 3 : 1) * E);
    total += (long)((f.dlv ? 3 : 1) * E);  // the ids, and with delivery the two record tables
  }
  HIPCHK(hipFree(d_gd));
  HIPCHK(hipFree(d_wl));
  HIPCHK(hipFree(d_wlc));
  HIPCHK(hipFree(d_krr));
  HIPCHK(hipFree(d_kid));
  HIPCHK(hipFree(d_kct));
  HIPCHK(hipFree(d_ks0));
  HIPCHK(hipFree(d_S));
  HIPCHK(hipFree(d_order));
  HIPCHK(hipFree(d_orr));
  HIPCHK(hipFree(d_octs));
  printf("ok %ld\n", total);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  bool host_only = false;
  for (int a = 1; a < argc; a++) {
    if (std::string(argv[a]) == "--host") host_only = true;
    else {
      fprintf(stderr, "usage: %s [--host]\n", argv[0]);
      return 2;
    }
  }
  const Cases C = make_cases();
  return host_only ? run_host(C) : run_device(C);
}
