// The owning buffer of the device back-ends (babble_amd/csrc/hge_own.h) on the CPU, over
// a memory policy that counts: live blocks and bytes, copies and waits; it refuses its
// k-th allocation or wait on request and aborts on a free of a block it does not know
// (so no block is ever freed twice).  New blocks come poisoned (0xA5), so a byte that
// nothing wrote is told from a fill and from a copy.
//   1. need: the minimum of 64 elements, no reallocation below the capacity, a refused
//      allocation leaves the buffer empty and throws Error{HGE_ERR_DEVICE};
//   2. grow_keep: the 1.5x rule, [0, keep) kept, the rest filled where asked, a refusal
//      leaves the old block owned and intact;
//   3. regrow_rows at every byte geometry the engine's ensure_ccap states (3 rows or
//      blocks, 64 -> 128 positions a row): rows land at the new pitch, the bytes past the
//      old row hold the fill, keep = false and "no old block" copy nothing, a refused
//      allocation or wait keeps the old block and frees the new one;
//   4. ownership: move construction and assignment, self-assignment, swap, adopt; every
//      scope ends with no live block.
// Prints "ok <checks>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../babble_amd/csrc/hge_own.h"

static long checks = 0;
#define CHECK(c)                                        \
  do {                                                  \
    checks++;                                           \
    if (!(c)) {                                         \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                          \
    }                                                   \
  } while (0)

static const unsigned char kPoison = 0xA5;
static int stream_tag;  // the opaque stream: the policy checks that it gets this one back
#define ST ((void*)&stream_tag)

struct CountMem {
  static std::map<void*, size_t>& live() {
    static std::map<void*, size_t> m;
    return m;
  }
  static inline size_t live_bytes = 0;
  static inline long allocs = 0, frees = 0, fills = 0, copies = 0, waits = 0;
  static inline long fail_alloc = 0, fail_wait = 0;  // k: the k-th from now is refused
  static void* alloc(size_t bytes) {
    if (fail_alloc && --fail_alloc == 0) throw hge::Error(HGE_ERR_DEVICE, "test: allocation refused");
    void* p = malloc(bytes ? bytes : 1);
    if (!p) abort();
    memset(p, kPoison, bytes);
    live()[p] = bytes;
    live_bytes += bytes;
    allocs++;
    return p;
  }
  static void free(void* p) {
    auto it = live().find(p);
    if (it == live().end()) abort();  // unknown block, or freed twice
    live_bytes -= it->second;
    live().erase(it);
    frees++;
    ::free(p);
  }
  static void in_block(const void* p, size_t bytes) {
    for (auto& kv : live())
      if ((const char*)p >= (const char*)kv.first && (const char*)p + bytes <= (const char*)kv.first + kv.second) return;
    abort();  // out of every live block
  }
  static void fill(void* p, int byte, size_t bytes, void* s) {
    if (s != ST) abort();
    in_block(p, bytes);
    memset(p, byte, bytes);
    fills++;
  }
  static void copy(void* dst, const void* src, size_t bytes, void* s) {
    if (s != ST) abort();
    in_block(dst, bytes);
    in_block(src, bytes);
    memcpy(dst, src, bytes);
    copies++;
  }
  static void copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t row_bytes, size_t rows,
                     void* s) {
    if (s != ST) abort();
    for (size_t r = 0; r < rows; r++) {
      in_block((char*)dst + r * dpitch, row_bytes);
      in_block((const char*)src + r * spitch, row_bytes);
      memcpy((char*)dst + r * dpitch, (const char*)src + r * spitch, row_bytes);
    }
    copies++;
  }
  static void wait(void* s) {
    if (s != ST) abort();
    if (fail_wait && --fail_wait == 0) throw hge::Error(HGE_ERR_DEVICE, "test: wait refused");
    waits++;
  }
};

template <class T>
using B = hge::Buf<T, CountMem>;

static_assert(!std::is_copy_constructible<B<int32_t>>::value, "Buf must not be copy-constructible");
static_assert(!std::is_copy_assignable<B<int32_t>>::value, "Buf must not be copy-assignable");
static_assert(std::is_nothrow_move_constructible<B<int32_t>>::value, "Buf moves");

static size_t blocks() { return CountMem::live().size(); }

template <class F>
static bool refused(F&& f) {
  try {
    f();
  } catch (const hge::Error& e) {
    CHECK(e.code == HGE_ERR_DEVICE);
    CHECK(!e.msg.empty());
    return true;
  }
  return false;
}

static void test_need() {
  {
    B<int32_t> b;
    CHECK(b.p == nullptr && b.n == 0);
    b.need(0);
    CHECK(b.p == nullptr && b.n == 0 && blocks() == 0);
    b.need(1);
    CHECK(b.p && b.n == 64 && blocks() == 1 && CountMem::live_bytes == 64 * 4);
    int32_t* p0 = b.p;
    const long a0 = CountMem::allocs;
    for (size_t m : {1, 16, 63, 64}) {
      b.need(m);
      CHECK(b.p == p0 && b.n == 64 && CountMem::allocs == a0);
    }
    b.need(65);  // contents are not kept: the old block goes first
    CHECK(b.n == 65 && blocks() == 1 && CountMem::live_bytes == 65 * 4 && CountMem::allocs == a0 + 1);
    b.need(1000);
    CHECK(b.n == 1000 && blocks() == 1 && CountMem::live_bytes == 4000);
    CountMem::fail_alloc = 1;
    CHECK(refused([&] { b.need(1001); }));
    CHECK(b.p == nullptr && b.n == 0 && blocks() == 0 && CountMem::live_bytes == 0);
    b.need(3);  // usable again
    CHECK(b.p && b.n == 64 && blocks() == 1);
  }
  CHECK(blocks() == 0 && CountMem::live_bytes == 0);
}

static void test_grow_keep() {
  for (int fill : {-1, 0, 0xFF, 0x7F}) {
    B<uint16_t> b;
    b.grow_keep(10, 0, ST, fill);  // from empty: no 64 minimum here, max(m, n + n / 2)
    CHECK(b.n == 10 && blocks() == 1);
    b.need(64);
    for (size_t i = 0; i < 64; i++) b.p[i] = (uint16_t)(i * 3 + 1);
    uint16_t* p0 = b.p;
    b.grow_keep(64, 64, ST, fill);
    CHECK(b.p == p0 && b.n == 64);
    const long c0 = CountMem::copies, w0 = CountMem::waits;
    b.grow_keep(65, 40, ST, fill);
    CHECK(b.n == 96 && blocks() == 1 && CountMem::live_bytes == 96 * 2);  // 64 + 64 / 2
    CHECK(CountMem::copies == c0 + 1 && CountMem::waits == w0 + 1);
    for (size_t i = 0; i < 40; i++) CHECK(b.p[i] == (uint16_t)(i * 3 + 1));
    const unsigned char* raw = (const unsigned char*)b.p;
    for (size_t i = 80; i < 96 * 2; i++) CHECK(raw[i] == (fill >= 0 ? (unsigned char)fill : kPoison));
    b.grow_keep(500, 40, ST, fill);  // past 1.5x: what was asked
    CHECK(b.n == 500 && blocks() == 1);
    for (size_t i = 0; i < 40; i++) CHECK(b.p[i] == (uint16_t)(i * 3 + 1));
    b.grow_keep(501, 0, ST, fill);  // keep = 0: nothing copied
    CHECK(b.n == 750);
    raw = (const unsigned char*)b.p;
    for (size_t i = 0; i < 750 * 2; i++) CHECK(raw[i] == (fill >= 0 ? (unsigned char)fill : kPoison));
    // a refusal (of the block, of the wait) leaves the old block owned and intact
    for (size_t i = 0; i < 750; i++) b.p[i] = (uint16_t)(i ^ 0x55);
    p0 = b.p;
    for (int what = 0; what < 2; what++) {
      (what ? CountMem::fail_wait : CountMem::fail_alloc) = 1;
      CHECK(refused([&] { b.grow_keep(751, 750, ST, fill); }));
      CHECK(b.p == p0 && b.n == 750 && blocks() == 1 && CountMem::live_bytes == 1500);
      for (size_t i = 0; i < 750; i++) CHECK(b.p[i] == (uint16_t)(i ^ 0x55));
    }
  }
  CHECK(blocks() == 0 && CountMem::live_bytes == 0);
}

// one table of ensure_ccap: `rows` rows of pos_bytes * positions bytes, in a block of
// total(positions) bytes that the buffer reports as n(positions) elements
template <class T, class Tot, class Cnt>
static void geometry(size_t rows, size_t pos_bytes, Tot total, Cnt count) {
  const size_t oc = 64, nc = 128;
  const size_t orb = pos_bytes * oc, nrb = pos_bytes * nc;
  auto pat = [](size_t r, size_t j) { return (unsigned char)((r * 31 + j * 7) % 97); };  // never the fill or the poison
  for (int fill : {-1, 0xFF}) {
    const unsigned char rest = fill >= 0 ? (unsigned char)fill : kPoison;
    {
      B<T> b;
      // no old block: nothing is copied, whatever keep says (the engine's first call: ccap = 0)
      const long c0 = CountMem::copies;
      b.regrow_rows(rows, 0, orb, total(oc), count(oc), true, ST, fill);
      CHECK(CountMem::copies == c0 && b.p && b.n == count(oc) && blocks() == 1);
      CHECK(CountMem::live_bytes == total(oc) && total(oc) >= rows * orb);
      unsigned char* raw = (unsigned char*)b.p;
      for (size_t i = 0; i < total(oc); i++) CHECK(raw[i] == rest);
      for (size_t r = 0; r < rows; r++)
        for (size_t j = 0; j < orb; j++) raw[r * orb + j] = pat(r, j);
      // regrown: every old row at its new pitch, the fill behind it and behind the rows
      const long w0 = CountMem::waits;
      b.regrow_rows(rows, orb, nrb, total(nc), count(nc), true, ST, fill);
      CHECK(CountMem::copies == c0 + 1 && CountMem::waits == w0 + 1);
      CHECK(b.n == count(nc) && blocks() == 1 && CountMem::live_bytes == total(nc) && total(nc) >= rows * nrb);
      raw = (unsigned char*)b.p;
      for (size_t r = 0; r < rows; r++)
        for (size_t j = 0; j < nrb; j++) CHECK(raw[r * nrb + j] == (j < orb ? pat(r, j) : rest));
      for (size_t i = rows * nrb; i < total(nc); i++) CHECK(raw[i] == rest);
      // a refused allocation, a refused wait: the old block stays, the new one is not leaked
      T* p0 = b.p;
      for (int what = 0; what < 2; what++) {
        (what ? CountMem::fail_wait : CountMem::fail_alloc) = 1;
        CHECK(refused([&] { b.regrow_rows(rows, nrb, 2 * nrb, 2 * total(nc), 2 * count(nc), true, ST, fill); }));
        CHECK(b.p == p0 && b.n == count(nc) && blocks() == 1 && CountMem::live_bytes == total(nc));
        for (size_t r = 0; r < rows; r++)
          for (size_t j = 0; j < orb; j++) CHECK(((unsigned char*)b.p)[r * nrb + j] == pat(r, j));
      }
      // keep = false: a fresh block, nothing copied into it
      const long c1 = CountMem::copies;
      b.regrow_rows(rows, nrb, nrb, total(nc), count(nc), false, ST, fill);
      CHECK(CountMem::copies == c1 && b.n == count(nc) && blocks() == 1);
      raw = (unsigned char*)b.p;
      for (size_t i = 0; i < total(nc); i++) CHECK(raw[i] == rest);
    }
    CHECK(blocks() == 0 && CountMem::live_bytes == 0);
  }
}

static void test_regrow_rows() {
  const size_t N = 3;
  // 4-byte elements, N rows (the chain ids, filled 0xFF)
  geometry<int32_t>(N, 4, [=](size_t c) { return 4 * N * c; }, [=](size_t c) { return N * c; });
  // 8-byte elements, N rows (other-parent coordinates, chain timestamps)
  geometry<int64_t>(N, 8, [=](size_t c) { return 8 * N * c; }, [=](size_t c) { return N * c; });
  // int32 rows of N per position, a chain's block is one row (LA, FD, the FD timestamp offsets)
  geometry<int32_t>(N, 4 * N, [=](size_t c) { return 4 * N * c * N; }, [=](size_t c) { return N * c * N; });
  // (N + 1) / 2 packed words per position (the 16-bit LA table)
  const size_t w = (N + 1) / 2;
  geometry<uint32_t>(N, 4 * w, [=](size_t c) { return 4 * N * c * w; }, [=](size_t c) { return N * c * w; });
  // uint16 rows of N behind an int32 element type: n = N * nc * N / 2
  geometry<int32_t>(N, 2 * N, [=](size_t c) { return 2 * N * c * N; }, [=](size_t c) { return N * c * N / 2; });
  // the run layout: N * N rows; int32 runs, and uint16 runs of ccap halves in an int32-sized block
  geometry<int32_t>(N * N, 4, [=](size_t c) { return 4 * N * c * N; }, [=](size_t c) { return N * c * N; });
  geometry<int32_t>(N * N, 2, [=](size_t c) { return 4 * N * c * N; }, [=](size_t c) { return N * c * N; });
  // 1-byte tile flags, (N + 63) / 64 a position
  const size_t NT = (N + 63) / 64;
  geometry<uint8_t>(N, NT, [=](size_t c) { return N * c * NT; }, [=](size_t c) { return N * c * NT; });
}

static void test_ownership() {
  {
    B<int32_t> a;
    a.need(100);
    a.p[0] = 7;
    int32_t* pa = a.p;
    B<int32_t> b(std::move(a));  // move construction: the source is empty
    CHECK(a.p == nullptr && a.n == 0 && b.p == pa && b.n == 100 && blocks() == 1);
    B<int32_t> c;
    c.need(200);
    int32_t* pc = c.p;
    CHECK(blocks() == 2);
    const long f0 = CountMem::frees;
    c = std::move(b);  // onto a non-empty buffer: its old block is freed, once
    CHECK(CountMem::frees == f0 + 1 && blocks() == 1 && c.p == pa && c.n == 100 && b.p == nullptr && b.n == 0);
    CHECK(CountMem::live().count(pc) == 0);
    B<int32_t>& alias = c;
    c = std::move(alias);  // self-assignment keeps the block
    CHECK(c.p == pa && c.n == 100 && blocks() == 1 && CountMem::frees == f0 + 1);
    B<int32_t> d;
    d.need(300);
    int32_t* pd = d.p;
    c.swap(d);
    CHECK(c.p == pd && c.n == 300 && d.p == pa && d.n == 100 && blocks() == 2);
    std::swap(c, d);  // as the engine's call sites spell it
    CHECK(c.p == pa && c.n == 100 && d.p == pd && d.n == 300 && blocks() == 2 && CountMem::frees == f0 + 1);
    swap(c, d);
    CHECK(c.p == pd && d.p == pa && blocks() == 2 && CountMem::frees == f0 + 1);
    B<int32_t> e;
    std::swap(c, e);  // with an empty one
    CHECK(c.p == nullptr && c.n == 0 && e.p == pd && e.n == 300 && blocks() == 2);
    {
      B<int32_t> q;  // adopt: a block that something else filled replaces the old one
      q.need(400);
      q.p[399] = 42;
      int32_t* pq = q.p;
      d.adopt(std::move(q));
      CHECK(d.p == pq && d.n == 400 && d.p[399] == 42 && q.p == nullptr && q.n == 0);
      CHECK(blocks() == 2 && CountMem::live().count(pa) == 0);
    }
    CHECK(blocks() == 2);
    std::vector<B<int32_t>> v;  // movable into a container that grows
    for (int i = 0; i < 9; i++) {
      v.emplace_back();
      v.back().need(10 + i);
    }
    CHECK(blocks() == 11);
  }
  CHECK(blocks() == 0 && CountMem::live_bytes == 0);
  CHECK(CountMem::allocs == CountMem::frees);
}

int main() {
  test_need();
  test_grow_keep();
  test_regrow_rows();
  test_ownership();
  CHECK(CountMem::live().empty() && CountMem::live_bytes == 0 && CountMem::allocs == CountMem::frees);
  printf("ok %ld\n", checks);
  return 0;
}
