// hge_sort_kernel_test.hip — the order stage's call-bucket sorts (k_bucket_sort,
// k_bucket_sort_big, k_bucket_sort_all: hge_kernels.hip, included as it is) driven
// directly on synthetic buckets whose sizes sit on every size switch (512 / 513, 1,024,
// 2,048, 4,096, 8,192, 16,384) and whose ranges sit on the packing rule wr + wc <= 32
// (hge_sortkey.h), against std::sort over the full key with the order written out in
// hge_sort_cases.h.  A stream cannot choose a bucket's size or its spans.
//
//   hge_sort_kernel_test          every launch form on the device, every output slot compared
//   hge_sort_kernel_test --host   the generator and the host models only (no device): the
//                                 statistics each kind promises, and how many buckets a
//                                 sort that read one rule wrongly would order differently
//                                 (all must be > 0)
//
// One list of many buckets per launch, in the launch forms of the order stage
// (hge_engine.hip): k_bucket_sort with skip_big = 1 at 256 threads; k_bucket_sort_big at
// 1,024 threads on a grid smaller than the list; k_bucket_sort_all with at most 8 buckets
// a launch; the last two again with force_index = 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hge_plan.h"

#include "hge_kernels.hip"

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
constexpr int kSmall = 512, kWhole = 8192, kBig = 16384;  // the size switches, as documented

const int kSizes[] = {1,    2,    3,    63,   64,   65,   255,   256,   257,   511,   512,   513,   1023,  1024, 1025, 2047,
                      2048, 2049, 4095, 4096, 4097, 8191, 8192,  8193,  8194,  12289, 16383, 16384, 16385, 16896, 16897, 20000};

// (wr, wc) of the boundary kinds: wr + wc = 32 exactly, and the same with one more
// timestamp bit (33: the index path)
const int kSplit[4][2] = {{0, 32}, {4, 28}, {16, 16}, {31, 1}};

enum Kind {
  kPlainRandom = 0, kPlainAsc, kPlainDesc, kPlainOrgan,
  kW32a, kW32b, kW32c, kW32d,
  kW33a, kW33b, kW33c, kW33d,
  kSign, kEqual, kHalfSecondFar, kHalfFirstFar, kNKinds
};
const char* const kKindName[kNKinds] = {"plain_random", "plain_ascending", "plain_descending", "plain_organ_pipe",
                                        "w32_0_32", "w32_4_28", "w32_16_16", "w32_31_1",
                                        "w33_0_33", "w33_4_29", "w33_16_17", "w33_31_2",
                                        "cts_sign", "equal_words", "halves_second_unpackable", "halves_first_unpackable"};

bool kind_at_size(int kind, int n) {
  if (kind <= kPlainOrgan || kind == kSign || kind == kEqual) return true;
  if (kind >= kW32a && kind <= kW33d) return n > kSmall && n <= kBig;  // where a bucket is packed or not
  return n > kWhole && n <= kBig;                                       // where a bucket is two halves
}

// the ranges of keys[lo, lo + len) and the verdict of the packing rule at `limit` bits
struct Plan {
  uint32_t rmin, rmax;
  int64_t cmin, cmax;
  int wr, wc;
  bool packable;
};
Plan plan_of(const std::vector<Key>& k, int lo, int len, int limit) {
  Plan p{k[lo].rr, k[lo].rr, k[lo].cts, k[lo].cts, 0, 0, false};
  for (int i = lo; i < lo + len; i++) {
    p.rmin = std::min(p.rmin, k[i].rr), p.rmax = std::max(p.rmax, k[i].rr);
    p.cmin = std::min(p.cmin, k[i].cts), p.cmax = std::max(p.cmax, k[i].cts);
  }
  p.wr = bits_of(p.rmax - p.rmin);
  p.wc = bits_of((uint64_t)p.cmax - (uint64_t)p.cmin);
  p.packable = p.wr + p.wc <= limit;
  return p;
}
// the packed word as hge_sortkey.h documents it: ((rr - rr_min) << wc | (cts - cts_min)) << 32 | S's top 32 bits
uint64_t word_of(const Plan& p, const Key& k) {
  const uint64_t lead = ((uint64_t)(k.rr - p.rmin) << p.wc) | ((uint64_t)k.cts - (uint64_t)p.cmin);
  return (lead << 32) | (k.s[0] >> 32);
}
int slots_of(int len) {  // the power of two a part is padded to
  int P = 1024;
  while (P < len) P <<= 1;
  return P;
}

struct Bucket {
  int n = 0, kind = 0, b = 0, start = 0;
  std::vector<Key> keys;      // input order
  std::vector<int32_t> want;  // the ids in the order of ref_less
  int path = 0;               // 0: up to 512 keys, 1: 513 .. 16,384 (whole or two halves), 2: past 16,384
  int nparts = 0, off[2] = {0, 0}, len[2] = {0, 0};
  bool pack[2] = {false, false};
  bool packed() const { return path == 1 && pack[0] && (nparts == 1 || pack[1]); }
};

// What a sort of this bucket would give that read one rule wrongly (0: all rules right).
enum Reading { kRight = 0, kCtsUnsigned, kTiesById, kPadFirst, kPack33, kNReadings };
const char* const kReadingName[kNReadings] = {"right", "cts_unsigned", "ties_by_id", "padding_first", "packable_at_33"};

// a part on the packed path: P slots of (word, index), padding the all-ones word at an
// index >= len; equal words by the full key, padding by its index (after every real key)
void model_part(const Bucket& B, int lo, int len, int reading, std::vector<int32_t>& out, long* eqpairs, long* padword) {
  const int cmp = reading == kCtsUnsigned ? kCmpCtsUnsigned : reading == kTiesById ? kCmpIdAfterWord : kCmpRight;
  const Plan p = plan_of(B.keys, lo, len, reading == kPack33 ? 33 : 32);
  std::vector<int> ix;
  if (!p.packable) {
    for (int i = 0; i < len; i++) ix.push_back(i);
    std::sort(ix.begin(), ix.end(), [&](int x, int y) { return mode_less(B.keys[lo + x], B.keys[lo + y], cmp); });
  } else {
    const int P = slots_of(len);
    std::vector<uint64_t> w((size_t)P, ~0ull);
    for (int i = 0; i < len; i++) w[i] = word_of(p, B.keys[lo + i]);
    for (int i = 0; i < P; i++) ix.push_back(i);
    std::sort(ix.begin(), ix.end(), [&](int x, int y) {
      if (w[x] != w[y]) return w[x] < w[y];
      if (x >= len || y >= len) {
        if (reading == kPadFirst && (x >= len) != (y >= len)) return x >= len;
        return x < y;
      }
      return mode_less(B.keys[lo + x], B.keys[lo + y], cmp);
    });
    ix.resize(len);
    for (int i = 0; i + 1 < len && eqpairs; i++) *eqpairs += ix[i] < len && ix[i + 1] < len && w[ix[i]] == w[ix[i + 1]];
    for (int i = 0; i < len && padword && P > len; i++) *padword += w[i] == ~0ull;
  }
  for (int i : ix) out.push_back(i < len ? (int32_t)B.keys[lo + i].id : -1);
}
std::vector<int32_t> model_sort(const Bucket& B, int reading, long* eqpairs = nullptr, long* padword = nullptr) {
  const int cmp = reading == kCtsUnsigned ? kCmpCtsUnsigned : reading == kTiesById ? kCmpIdAfterWord : kCmpRight;
  std::vector<int32_t> out;
  if (B.path != 1) {
    std::vector<Key> k = B.keys;
    std::sort(k.begin(), k.end(), [&](const Key& x, const Key& y) { return mode_less(x, y, cmp); });
    for (const Key& x : k) out.push_back((int32_t)x.id);
    return out;
  }
  std::vector<int32_t> part[2];
  for (int h = 0; h < B.nparts; h++) model_part(B, B.off[h], B.len[h], reading, part[h], eqpairs, padword);
  if (B.nparts == 1) return part[0];
  // the halves merged by the full key (a padding slot taken for a key stays where it fell)
  std::vector<const Key*> by_id((size_t)B.n, nullptr);
  // (ids are start + a permutation of 0 .. n - 1)
  auto key_of = [&](int32_t id) -> const Key* {
    if (id < 0) return nullptr;
    return by_id[(size_t)(id - B.start)];
  };
  for (const Key& x : B.keys) by_id[(size_t)((int32_t)x.id - B.start)] = &x;
  size_t i = 0, j = 0;
  while (i < part[0].size() || j < part[1].size()) {
    bool takeA;
    if (j >= part[1].size()) takeA = true;
    else if (i >= part[0].size()) takeA = false;
    else {
      const Key *x = key_of(part[0][i]), *y = key_of(part[1][j]);
      takeA = !x || !y ? x == nullptr : mode_less(*x, *y, cmp);
    }
    out.push_back(takeA ? part[0][i++] : part[1][j++]);
  }
  return out;
}

std::vector<Key> generate(int kind, int n, Rng& g) {
  std::vector<Key> k;
  if (kind <= kPlainOrgan) {
    k = gen_plain(n, g);
  } else if (kind >= kW32a && kind <= kW33d) {
    const int q = (kind - kW32a) & 3;
    const int wr = kSplit[q][0], wc = kSplit[q][1] + (kind >= kW33a ? 1 : 0);
    const uint32_t rspan = wr ? (uint32_t)((1ull << wr) - 1) : 0;
    const uint64_t cspan = (1ull << wc) - 1;
    k = gen_span(n, wr == 31 ? 0 : 1000, rspan, 1700000000000000000ll, cspan, g);
    if (n > kWhole) {  // two halves: the second one gets the corners too
      std::vector<Key> h2 = gen_span(n - ((n + 1) >> 1), wr == 31 ? 0 : 1000, rspan, 1700000000000000000ll, cspan, g);
      std::copy(h2.begin(), h2.end(), k.begin() + ((n + 1) >> 1));
    }
    // the corners stay where the halves' split needs them; the rest is in random order already
    return k;
  } else if (kind == kSign) {
    k = gen_sign(n, g);
  } else if (kind == kEqual) {
    k = gen_equal(n, g);
  } else {
    // one far timestamp on the chosen side of the documented split (nb + 1) >> 1
    k = gen_plain(n, g);
    const int na = (n + 1) >> 1;
    k[kind == kHalfSecondFar ? na : na - 1].cts += 1ll << 40;
    return k;
  }
  shuffle(k, g);
  return k;
}

struct Cases {
  std::vector<Bucket> bk;     // by bucket id; every ninth one is empty
  std::vector<int32_t> bend, bcnt, list;
  int total = 0;              // slots, gaps included
  long keys = 0;
  int npacked = 0, nindex = 0;  // of the buckets of 513 .. 16,384 keys
};

Cases make_cases() {
  Cases C;
  Rng g{0x50F7ull};
  int pos = 5;  // slots before the first bucket
  for (int kind = 0; kind < kNKinds; kind++)
    for (int n : kSizes) {
      if (!kind_at_size(kind, n)) continue;
      if (C.bk.size() % 9 == 4) {  // an empty bucket: never listed
        Bucket E;
        E.b = (int)C.bk.size();
        E.start = pos;
        C.bk.push_back(E);
      }
      Bucket B;
      B.n = n, B.kind = kind, B.b = (int)C.bk.size();
      pos += B.b % 4;  // slots between the buckets
      B.start = pos;
      B.keys = generate(kind, n, g);
      deal_ids(B.keys, (uint32_t)B.start, g);
      if (kind >= kPlainAsc && kind <= kPlainOrgan) arrange(B.keys, kind - kPlainRandom);  // (the ids are part of the order)
      std::vector<Key> s = B.keys;
      std::sort(s.begin(), s.end(), ref_less);
      for (const Key& x : s) B.want.push_back((int32_t)x.id);
      B.path = n <= kSmall ? 0 : n <= kBig ? 1 : 2;
      if (B.path == 1) {
        B.nparts = n <= kWhole ? 1 : 2;
        B.len[0] = B.nparts == 1 ? n : (n + 1) >> 1;
        B.off[1] = B.len[0], B.len[1] = n - B.len[0];
        for (int h = 0; h < B.nparts; h++) B.pack[h] = plan_of(B.keys, B.off[h], B.len[h], 32).packable;
        (B.packed() ? C.npacked : C.nindex)++;
      }
      pos += n;
      C.keys += n;
      C.bk.push_back(std::move(B));
    }
  C.total = pos + 7;  // and slots after the last one
  for (const Bucket& B : C.bk) {
    C.bend.push_back(B.start + B.n);
    C.bcnt.push_back(B.n);
    if (B.n) C.list.push_back(B.b);
  }
  for (size_t i = C.list.size(); i > 1; i--) std::swap(C.list[i - 1], C.list[g.below(i)]);  // in no order
  return C;
}

// ---------------------------------------------------------------------------
// --host: what the kinds promise, and that the wrong readings would show
// ---------------------------------------------------------------------------
int run_host(const Cases& C) {
  struct Stat {
    long buckets = 0, keys = 0, eqpairs = 0, padword = 0, packable = 0, unpackable = 0, mixed = 0;
    long differ[kNReadings] = {0, 0, 0, 0, 0};
  };
  std::vector<Stat> st(kNKinds);
  for (const Bucket& B : C.bk) {
    if (!B.n) continue;
    Stat& s = st[B.kind];
    s.buckets++, s.keys += B.n;
    if (model_sort(B, kRight, &s.eqpairs, &s.padword) != B.want) {
      printf("n=%d kind=%s: the host model of the sort differs from std::sort over the full key\n", B.n, kKindName[B.kind]);
      return 1;
    }
    if (B.path == 1) {
      for (int h = 0; h < B.nparts; h++) (B.pack[h] ? s.packable : s.unpackable)++;
      s.mixed += B.nparts == 2 && B.pack[0] != B.pack[1];
      if (B.kind == kHalfSecondFar && !(B.pack[0] && !B.pack[1])) s.mixed = -1000000;
      if (B.kind == kHalfFirstFar && !(!B.pack[0] && B.pack[1])) s.mixed = -1000000;
    }
    // each wrong reading on the kinds that are there to tell it apart
    const bool w32 = B.kind >= kW32a && B.kind <= kW32d, w33 = B.kind >= kW33a && B.kind <= kW33d;
    const bool on[kNReadings] = {false, B.kind == kSign, B.kind == kEqual, w32, w33};
    for (int r = 1; r < kNReadings; r++)
      if (on[r]) s.differ[r] += model_sort(B, r) != B.want;
  }
  long total = 0;
  for (int kind = 0; kind < kNKinds; kind++) {
    const Stat& s = st[kind];
    printf("host kind=%s buckets=%ld keys=%ld eqpairs=%ld padword=%ld packable=%ld unpackable=%ld mixed_halves=%ld", kKindName[kind],
           s.buckets, s.keys, s.eqpairs, s.padword, s.packable, s.unpackable, s.mixed);
    for (int r = 1; r < kNReadings; r++) printf(" differ_%s=%ld", kReadingName[r], s.differ[r]);
    printf("\n");
    total += s.keys;
    const bool w32 = kind >= kW32a && kind <= kW32d, w33 = kind >= kW33a && kind <= kW33d;
    bool ok = s.buckets > 0;
    if (kind == kEqual) ok = ok && s.eqpairs > 0 && s.differ[kTiesById] > 0;
    if (kind == kSign) ok = ok && s.differ[kCtsUnsigned] > 0 && s.unpackable > 0;
    if (w32) ok = ok && s.padword > 0 && s.packable > 0 && s.unpackable == 0 && s.differ[kPadFirst] > 0;
    if (w33) ok = ok && s.unpackable > 0 && s.packable == 0 && s.differ[kPack33] > 0;
    if (kind == kHalfSecondFar || kind == kHalfFirstFar) ok = ok && s.mixed == s.buckets;
    if (!ok) {
      printf("kind=%s: the generator does not give what the kind promises\n", kKindName[kind]);
      return 1;
    }
  }
  printf("host buckets packed=%d index=%d list=%zu slots=%d\n", C.npacked, C.nindex, C.list.size(), C.total);
  if (C.npacked == 0 || C.nindex == 0) return 1;
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

enum Form { kFormSmall = 0, kFormBig, kFormBigIndex, kFormAll, kFormAllIndex, kNForms };
const char* const kFormName[kNForms] = {"k_bucket_sort skip_big", "k_bucket_sort_big packed", "k_bucket_sort_big force_index",
                                        "k_bucket_sort_all packed", "k_bucket_sort_all force_index"};

int run_device(const Cases& C) {
  using hge::OKey;
  // the keys as k_bucket_keys scatters them: call << 32 | rr, cts ^ sign; between the
  // buckets keys of no bucket
  Rng g{0xD1Full};
  std::vector<OKey> hk((size_t)C.total);
  for (OKey& k : hk) {
    k.a = 0xFFFFull << 32 | (g.next() & 0xFFFF);
    k.b = g.next(), k.s0 = g.next(), k.s1 = g.next(), k.s2 = g.next(), k.s3 = g.next();
    k.id = 0x7FFFFFFFu, k.pad = 0;
  }
  for (const Bucket& B : C.bk)
    for (int i = 0; i < B.n; i++) {
      const Key& x = B.keys[i];
      OKey& k = hk[(size_t)B.start + i];
      k.a = ((uint64_t)(uint32_t)B.b << 32) | x.rr;
      k.b = (uint64_t)x.cts ^ 0x8000000000000000ull;
      k.s0 = x.s[0], k.s1 = x.s[1], k.s2 = x.s[2], k.s3 = x.s[3];
      k.id = x.id, k.pad = 0;
    }
  const int nlist = (int)C.list.size();
  OKey *d_keys = nullptr, *d_tmp = nullptr;
  int32_t* d_ids = nullptr;
  HIPCHK(hipMalloc(&d_keys, hk.size() * sizeof(OKey)));
  HIPCHK(hipMalloc(&d_tmp, hk.size() * sizeof(OKey)));
  HIPCHK(hipMalloc(&d_ids, hk.size() * sizeof(int32_t)));
  int32_t *d_bend = upload(C.bend), *d_bcnt = upload(C.bcnt), *d_list = upload(C.list);
  std::vector<int32_t> group_n;  // k_bucket_sort_all's launches: at most 8 listed buckets each
  for (int o = 0; o < nlist; o += 8) group_n.push_back(std::min(8, nlist - o));
  group_n.push_back(nlist);  // (the last entry: the whole list)
  int32_t* d_nl = upload(group_n);
  const int32_t* d_nlist = d_nl + (group_n.size() - 1);
  unsigned long long* d_ctl = nullptr;
  HIPCHK(hipMalloc(&d_ctl, 8 * sizeof(unsigned long long)));
  std::vector<int32_t> got(hk.size());
  std::vector<OKey> keys_after(hk.size());
  long total = 0;
  for (int form = 0; form < kNForms; form++) {
    HIPCHK(hipMemcpy(d_keys, hk.data(), hk.size() * sizeof(OKey), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_tmp, 0xA5, hk.size() * sizeof(OKey)));
    HIPCHK(hipMemset(d_ids, 0x5E, hk.size() * sizeof(int32_t)));
    // cur = {packed, index, next bucket, unused} zeroed as the stage before leaves it; next to be cleared
    const unsigned long long ctl0[8] = {0, 0, 0, 0, 77, 77, 77, 77};
    HIPCHK(hipMemcpy(d_ctl, ctl0, sizeof(ctl0), hipMemcpyHostToDevice));
    const bool fi = form == kFormBigIndex || form == kFormAllIndex;
    const hge::SortCtl ctl{d_ctl, d_ctl + 4, fi ? 1 : 0};
    if (form == kFormSmall) {
      hge::k_bucket_sort<<<dim3(64), dim3(256)>>>(d_bend, d_bcnt, d_list, d_nlist, d_keys, d_tmp, d_ids, 1);
    } else if (form == kFormBig || form == kFormBigIndex) {
      hge::k_bucket_sort_big<<<dim3(40), dim3(1024)>>>(d_bend, d_bcnt, d_list, d_nlist, (const OKey*)d_keys, d_tmp, d_ids, ctl);
    } else {
      for (size_t q = 0; q + 1 < group_n.size(); q++) {
        hge::k_bucket_sort_all<<<dim3(8), dim3(1024)>>>(d_bend, d_bcnt, d_list + 8 * q, d_nl + q, d_keys, d_tmp, d_ids, ctl);
        HIPCHK(hipGetLastError());
      }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(got.data(), d_ids, got.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    unsigned long long ctl1[8];
    HIPCHK(hipMemcpy(ctl1, d_ctl, sizeof(ctl1), hipMemcpyDeviceToHost));
    // every slot: the order where this form sorts the bucket, the sentinel elsewhere
    std::vector<uint8_t> covered(hk.size(), 0);
    long buckets = 0, keys = 0;
    for (const Bucket& B : C.bk) {
      if (!B.n) continue;
      const bool live = form == kFormSmall ? B.path != 1 : form <= kFormBigIndex ? B.path == 1 : true;
      buckets += live, keys += live ? B.n : 0;
      for (int i = 0; i < B.n; i++) {
        const int32_t e = live ? B.want[i] : kSentinel, v = got[(size_t)B.start + i];
        covered[(size_t)B.start + i] = 1;
        if (v != e) {
          printf("MISMATCH %s: bucket %d of %d keys, kind %s, slot %d: got id %d want id %d%s\n", kFormName[form], B.b, B.n,
                 kKindName[B.kind], i, v, e, live ? "" : " (a bucket this launch must leave alone)");
          return 1;
        }
      }
    }
    for (size_t q = 0; q < got.size(); q++)
      if (!covered[q] && got[q] != kSentinel) {
        printf("MISMATCH %s: slot %zu outside every bucket was written: %d\n", kFormName[form], q, got[q]);
        return 1;
      }
    long packed = 0, index = 0;
    if (form != kFormSmall) {
      packed = (long)ctl1[0], index = (long)ctl1[1];
      const long wp = fi ? 0 : C.npacked, wi = fi ? C.npacked + C.nindex : C.nindex;
      if (packed != wp || index != wi) {
        printf("MISMATCH %s: the path counters are packed=%ld index=%ld, the spans give packed=%ld index=%ld\n", kFormName[form],
               packed, index, wp, wi);
        return 1;
      }
      if (ctl1[4] || ctl1[5] || ctl1[6]) {
        printf("MISMATCH %s: the next stage's counters were not cleared\n", kFormName[form]);
        return 1;
      }
    }
    if (form == kFormBig || form == kFormBigIndex) {
      HIPCHK(hipMemcpy(keys_after.data(), d_keys, hk.size() * sizeof(OKey), hipMemcpyDeviceToHost));
      if (memcmp(keys_after.data(), hk.data(), hk.size() * sizeof(OKey)) != 0) {
        printf("MISMATCH %s: the keys were changed\n", kFormName[form]);
        return 1;
      }
    }
    printf("case %s buckets=%ld keys=%ld packed=%ld index=%ld slots=%zu\n", kFormName[form], buckets, keys, packed, index, got.size());
    total += (long)got.size();
  }
  HIPCHK(hipFree(d_keys));
  HIPCHK(hipFree(d_tmp));
  HIPCHK(hipFree(d_ids));
  HIPCHK(hipFree(d_bend));
  HIPCHK(hipFree(d_bcnt));
  HIPCHK(hipFree(d_list));
  HIPCHK(hipFree(d_nl));
  HIPCHK(hipFree(d_ctl));
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
  // the bounds every launch relies on, checked before anything reaches the device
  for (const Bucket& B : C.bk)
    if (B.start < 0 || B.start + B.n > C.total || C.bend[B.b] - C.bcnt[B.b] != B.start || (int)B.want.size() != B.n) {
      printf("bucket %d: out of the tables' bounds\n", B.b);
      return 1;
    }
  return host_only ? run_host(C) : run_device(C);
}
