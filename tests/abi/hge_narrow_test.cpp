// The 8-bit frontier-relative compare of the direct rounds kernel
// (babble_amd/csrc/hge_narrow.h) on the CPU, against the plain statement of what it
// stands for: column i passes when LA >= FD.
//   1. every pair (a, b) of 7-bit fields in every lane, beside every kind of
//      neighbour: the guard bit is [a >= b] and no lane disturbs another;
//   2. (LA, FD, base) triples, random and at the edges (unset FD, values below the
//      base, 124 .. 128 above it, positions near 65,533, chains without a base): the
//      encoded compare equals LA >= FD whenever the encoders raise no flag, and
//      they raise one whenever a window value saturates (LA - base + 2 >= 126) or a
//      finite FD lies below its base.
// Prints "ok <checks>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../babble_amd/csrc/hge_narrow.h"

using namespace hge_narrow;

static long checks = 0;
static void fail(const char* what, long a, long b, long c) {
  printf("FAIL %s %ld %ld %ld\n", what, a, b, c);
  exit(1);
}

static const int32_t INF = kNarInf32;
// the kernel's 16-bit operands
static uint32_t lae(int32_t la, bool row) { return row ? (uint32_t)(la + 2) : 0u; }  // LA >= -1
static uint32_t fde(int32_t fd) { return fd == INF ? 0xFFFFu : (uint32_t)(fd + 1); }

static void guard_bits() {
  const uint32_t others[] = {0u, 127u, 1u, 126u, 85u};
  for (int lane = 0; lane < 4; lane++)
    for (uint32_t a = 0; a < 128; a++)
      for (uint32_t b = 0; b < 128; b++)
        for (uint32_t oa : others)
          for (uint32_t ob : others) {
            uint32_t aw = kNarGuard, bw = 0;
            for (int l = 0; l < 4; l++) {
              aw |= (l == lane ? a : oa) << (8 * l);
              bw |= (l == lane ? b : ob) << (8 * l);
            }
            const uint32_t ge = nar_ge4(aw, bw);
            for (int l = 0; l < 4; l++) {
              const bool want = l == lane ? a >= b : oa >= ob;
              if ((((ge >> (8 * l + 7)) & 1) != 0) != want) fail("guard", lane, a, b);
              if ((ge >> (8 * l)) & 0x7F) fail("guard junk", lane, a, b);
            }
            checks++;
          }
}

struct Col {
  int32_t la;   // lastAncestor of the window row (>= -1)
  bool row;     // the row exists
  int32_t fd;   // firstDescendant of the member, INF = unset
  int32_t base; // frontier position of the column, INF = none
};

// one group of four columns through the encoders, each column checked
static void check4(const Col (&c)[4]) {
  uint32_t la[2], fd[2], cb[2];
  for (int h = 0; h < 2; h++) {
    la[h] = lae(c[2 * h].la, c[2 * h].row) | (lae(c[2 * h + 1].la, c[2 * h + 1].row) << 16);
    fd[h] = fde(c[2 * h].fd) | (fde(c[2 * h + 1].fd) << 16);
    cb[h] = nar_base16(c[2 * h].base) | (nar_base16(c[2 * h + 1].base) << 16);
  }
  uint32_t mx = 0, mn = 0xFFFFFFFFu;
  const uint32_t aw = nar_enc_window4(la[0], la[1], cb[0], cb[1], mx);
  const uint32_t bw = nar_enc_member4(fd[0], fd[1], cb[0], cb[1], mn);
  const bool flag = nar_window_flag(mx) || nar_member_flag(mn);
  const uint32_t ge = nar_ge4(aw, bw);
  // the conditions as the kernel's documentation states them
  bool sat = false, low = false;
  for (int k = 0; k < 4; k++) {
    const int64_t b = c[k].base;  // INF: every finite FD is "below"
    if (c[k].row && c[k].base != INF && (int64_t)c[k].la - b + 2 >= 126) sat = true;
    if (c[k].fd != INF && (int64_t)c[k].fd < b) low = true;
  }
  if ((sat || low) && !flag) fail("flag missing", c[0].la, c[0].fd, c[0].base);
  if (flag && !(sat || low)) fail("flag without cause", c[0].la, c[0].fd, c[0].base);
  if (!flag) {
    if ((aw & kNarGuard) != kNarGuard) fail("window guard", aw, 0, 0);
    if (bw & kNarGuard) fail("member field", bw, 0, 0);
    for (int k = 0; k < 4; k++) {
      const bool want = c[k].row && c[k].fd != INF && c[k].la >= c[k].fd;
      if ((((ge >> (8 * k + 7)) & 1) != 0) != want) fail("compare", c[k].la, c[k].fd, c[k].base);
    }
  }
  checks++;
}

int main() {
  guard_bits();
  std::mt19937_64 rng(12345);
  auto rnd = [&](int64_t lo, int64_t hi) { return (int32_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
  // bases the kernel encodes against: 0 .. kNarBaseMax (a larger one sends the round to
  // the 16-bit select before any encode) and "none"
  const int32_t bases[] = {0, 1, 2, 100, 1000, 30000, 65000, 65270, 65399, kNarBaseMax, INF};
  const int32_t offs[] = {-3, -2, -1, 0, 1, 2, 60, 122, 123, 124, 125, 126, 127, 128, 129, 300};
  // a quiet column: far inside the range, never flags
  auto quiet = [&](int32_t base) {
    Col q;
    q.base = base == INF ? 500 : base;
    q.la = q.base + 5;
    q.row = true;
    q.fd = q.base + 7;
    return q;
  };
  // edges, one edge column among quiet ones, in every lane
  for (int32_t base : bases)
    for (int32_t ol : offs)
      for (int32_t of : offs)
        for (int kind = 0; kind < 3; kind++)
          for (int lane = 0; lane < 4; lane++) {
            Col e;
            e.base = base;
            const int64_t b0 = base == INF ? 40000 : base;
            int64_t la = b0 + ol, fd = b0 + of;
            if (la < -1) la = -1;
            if (la > 65533) la = 65533;
            if (fd < 0) fd = 0;
            if (fd > 65533) fd = 65533;
            e.la = (int32_t)la;
            e.fd = kind == 1 ? INF : (int32_t)fd;
            e.row = kind != 2;
            Col c[4] = {quiet(base), quiet(base), quiet(base), quiet(base)};
            c[lane] = e;
            check4(c);
          }
  // positions near 65,533 on a base the narrow form takes and on the last it takes
  for (int32_t base : {65270, 65399, kNarBaseMax})
    for (int32_t la = 65380; la <= 65533; la++)
      for (int32_t fd : {65390, 65400, 65401, 65500, 65532, 65533, INF}) {
        Col c[4] = {quiet(base), {la, true, fd, base}, quiet(base), {la, true, INF, base}};
        check4(c);
      }
  // random triples: values around the base, below it, far above it, unset
  for (int it = 0; it < 400000; it++) {
    Col c[4];
    for (int k = 0; k < 4; k++) {
      const int m = (int)(rng() % 16);
      c[k].base = m == 0 ? INF : rnd(0, kNarBaseMax);
      const int64_t b0 = c[k].base == INF ? rnd(0, 65000) : c[k].base;
      const int spread = (rng() % 8) == 0 ? 2000 : (rng() % 4) == 0 ? 130 : 90;
      int64_t la = b0 + rnd(-spread / 2, spread), fd = b0 + rnd((rng() % 16) == 0 ? -50 : 0, spread);
      if (la < -1) la = -1;
      if (la > 65533) la = 65533;
      if (fd < 0) fd = 0;
      if (fd > 65533) fd = 65533;
      c[k].la = (int32_t)la;
      c[k].row = (rng() % 10) != 0;
      c[k].fd = (rng() % 6) == 0 ? INF : (int32_t)fd;
    }
    check4(c);
  }
  // the base limit itself
  if (nar_base_too_large(kNarBaseMax) || !nar_base_too_large(kNarBaseMax + 1) || nar_base_too_large(INF))
    fail("base limit", 0, 0, 0);
  printf("ok %ld\n", checks);
  return 0;
}
