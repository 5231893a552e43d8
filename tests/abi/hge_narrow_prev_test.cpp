// The direct rounds kernel's 8-bit compare with the base moved back by one round
// (babble_amd/csrc/hge_narrow.h: both sides of round r are encoded against the previous
// frontier C_{r-1} <= C_r), and the layout of the staged narrow member rows, on the CPU:
//   1. (LA, FD, previous base, base) with previous base <= base -- unset values, values
//      124 .. 128 above the base, positions near 65,533, chains without a base: the
//      compare encoded against the previous base equals LA >= FD unless a flag is
//      raised, and the flags are raised exactly under (i) a window value saturates
//      (LA - previous base + 2 >= 126) and (ii) a finite FD lies below the previous base;
//   2. nar_mb_word for the three geometries (1024 threads; 64, 128, 256 wide): a
//      bijection onto the block's words, every consuming thread's words belong to one
//      member and are the words of its slice in order, and the producer's word pairs
//      (lanes 2m, 2m + 1) are adjacent and 8-byte aligned.
// Prints "ok <checks>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../babble_amd/csrc/hge_narrow.h"

using namespace hge_narrow;

static long checks = 0;
static void fail(const char* what, long a, long b, long c, long d) {
  printf("FAIL %s %ld %ld %ld %ld\n", what, a, b, c, d);
  exit(1);
}

static const int32_t INF = kNarInf32;
static uint32_t lae(int32_t la, bool row) { return row ? (uint32_t)(la + 2) : 0u; }  // LA >= -1
static uint32_t fde(int32_t fd) { return fd == INF ? 0xFFFFu : (uint32_t)(fd + 1); }

struct Col {
  int32_t la;    // lastAncestor of the window row (>= -1)
  bool row;      // the row exists
  int32_t fd;    // firstDescendant of the member, INF = unset
  int32_t prev;  // the column's previous frontier position: what both sides are encoded against
};

static void check4(const Col (&c)[4]) {
  uint32_t la[2], fd[2], cb[2];
  for (int h = 0; h < 2; h++) {
    la[h] = lae(c[2 * h].la, c[2 * h].row) | (lae(c[2 * h + 1].la, c[2 * h + 1].row) << 16);
    fd[h] = fde(c[2 * h].fd) | (fde(c[2 * h + 1].fd) << 16);
    cb[h] = nar_base16(c[2 * h].prev) | (nar_base16(c[2 * h + 1].prev) << 16);
  }
  uint32_t mx = 0, mn = 0xFFFFFFFFu;
  const uint32_t aw = nar_enc_window4(la[0], la[1], cb[0], cb[1], mx);  // the consumer's side
  const uint32_t bw = nar_enc_member4(fd[0], fd[1], cb[0], cb[1], mn);  // the producer's side
  const bool wflag = nar_window_flag(mx), mflag = nar_member_flag(mn);
  bool sat = false, low = false;
  for (int k = 0; k < 4; k++) {
    const int64_t b = c[k].prev;  // INF: every finite FD is "below"
    if (c[k].row && c[k].prev != INF && (int64_t)c[k].la - b + 2 >= 126) sat = true;
    if (c[k].fd != INF && (int64_t)c[k].fd < b) low = true;
  }
  if (sat != wflag) fail("window flag", c[0].la, c[0].fd, c[0].prev, sat);
  if (low != mflag) fail("member flag", c[0].la, c[0].fd, c[0].prev, low);
  if (!wflag && !mflag) {
    if ((aw & kNarGuard) != kNarGuard) fail("window guard", aw, 0, 0, 0);
    if (bw & kNarGuard) fail("member field", bw, 0, 0, 0);
    const uint32_t ge = nar_ge4(aw, bw);
    for (int k = 0; k < 4; k++) {
      const bool want = c[k].row && c[k].fd != INF && c[k].la >= c[k].fd;
      if ((((ge >> (8 * k + 7)) & 1) != 0) != want) fail("compare", c[k].la, c[k].fd, c[k].prev, k);
    }
  }
  checks++;
}

static int64_t clampi(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : x > hi ? hi : x; }

static void compare_prev_base() {
  std::mt19937_64 rng(424242);
  auto rnd = [&](int64_t lo, int64_t hi) { return (int32_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
  auto quiet = [&](int32_t prev) {
    Col q;
    q.prev = prev == INF ? 500 : prev;
    q.la = q.prev + 5;
    q.row = true;
    q.fd = q.prev + 7;
    return q;
  };
  // (base, advance of the column over the last round): previous base = base - advance
  const int32_t bases[] = {0, 1, 40, 1000, 30000, 65000, 65270, 65399, kNarBaseMax};
  const int32_t advs[] = {0, 1, 2, 14, 33, 60, 121, 122, 123, 124, 125, 126, 127, 128, 200};
  const int32_t offs[] = {-3, -2, -1, 0, 1, 2, 60, 122, 123, 124, 125, 126, 127, 128, 129, 300};  // above the base
  for (int32_t base : bases)
    for (int32_t adv : advs) {
      if (adv > base) continue;
      const int32_t prev = base - adv;
      for (int32_t ol : offs)
        for (int32_t of : offs)
          for (int kind = 0; kind < 3; kind++)
            for (int lane = 0; lane < 4; lane++) {
              Col e;
              e.prev = prev;
              e.la = (int32_t)clampi((int64_t)base + ol, -1, 65533);
              e.fd = kind == 1 ? INF : (int32_t)clampi((int64_t)base + of, 0, 65533);
              e.row = kind != 2;
              Col c[4] = {quiet(prev), quiet(prev), quiet(prev), quiet(prev)};
              c[lane] = e;
              check4(c);
            }
    }
  // a finite FD below the PREVIOUS base (it cannot happen for a round-r member, and must
  // be flagged if it does), and between the two bases (fine)
  for (int32_t base : {200, 30000, kNarBaseMax})
    for (int32_t adv : {0, 1, 14, 33})
      for (int32_t dfd = -40; dfd <= 2; dfd++)
        for (int32_t dla = -40; dla <= 40; dla += 5) {
          Col e = {base + dla, true, base + dfd, base - adv};
          Col c[4] = {quiet(base - adv), e, quiet(base - adv), {base + dla, true, INF, base - adv}};
          check4(c);
        }
  // positions near 65,533
  for (int32_t prev : {65270, 65380, 65399, kNarBaseMax})
    for (int32_t la = 65380; la <= 65533; la++)
      for (int32_t fd : {65390, 65400, 65401, 65500, 65532, 65533, INF}) {
        Col c[4] = {quiet(prev), {la, true, fd, prev}, quiet(prev), {la, true, INF, prev}};
        check4(c);
      }
  // chains without a frontier position, then and now
  for (int32_t la : {-1, 0, 1, 100, 65533})
    for (int32_t fd : {0, 5, 65533, INF})
      for (int row = 0; row < 2; row++) {
        Col c[4] = {{la, row != 0, fd, INF}, quiet(100), {la, true, INF, INF}, quiet(100)};
        check4(c);
      }
  // random: previous base <= base, values around the base
  for (int it = 0; it < 400000; it++) {
    Col c[4];
    for (int k = 0; k < 4; k++) {
      const int32_t base = rnd(0, kNarBaseMax);
      const int32_t adv = (rng() % 8) == 0 ? rnd(0, 140) : rnd(0, 35);
      const int32_t prev = (rng() % 16) == 0 ? INF : (int32_t)clampi((int64_t)base - adv, 0, kNarBaseMax);
      const int spread = (rng() % 8) == 0 ? 2000 : (rng() % 4) == 0 ? 130 : 90;
      c[k].prev = prev;
      c[k].la = (int32_t)clampi((int64_t)base + rnd(-spread / 2, spread), -1, 65533);
      c[k].fd = (rng() % 6) == 0 ? INF : (int32_t)clampi((int64_t)base + rnd((rng() % 16) == 0 ? -50 : 0, spread), 0, 65533);
      c[k].row = (rng() % 10) != 0;
    }
    check4(c);
  }
}

static void staging_layout(int bs, int npow) {
  const int tpm = bs / npow, ncw = nar_mb_ncw(bs, npow), vw = nar_mb_vw(bs, npow);
  const int words = npow * npow / 4, rw = npow / 4;  // block words, words per member row
  if (ncw * tpm != rw || ncw % vw != 0 || bs * ncw != words) fail("geometry", bs, npow, ncw, vw);
  std::vector<int> owner(words, -1), cwof(words, -1);
  for (int m = 0; m < npow; m++)
    for (int cw = 0; cw < rw; cw++) {
      const uint32_t x = nar_mb_word(bs, npow, m, cw);
      if (x >= (uint32_t)words) fail("out of the block", npow, m, cw, x);
      if (owner[x] != -1) fail("two words in one place", npow, m, cw, x);
      owner[x] = m;
      cwof[x] = cw;
      checks++;
    }
  // the consumer: thread tid's load k reads words [(k * bs + tid) * vw, + vw)
  for (int tid = 0; tid < bs; tid++) {
    const int m = tid / tpm, part = tid - m * tpm;
    for (int k = 0; k < ncw / vw; k++)
      for (int s = 0; s < vw; s++) {
        const int x = (k * bs + tid) * vw + s;
        if (owner[x] != m) fail("another member's bytes", npow, tid, k, owner[x]);
        if (cwof[x] != part * ncw + k * vw + s) fail("slice order", npow, tid, k, cwof[x]);
        checks++;
      }
  }
  // the producer: lanes 2m, 2m + 1 (column words cw, cw + 1) store one aligned 8 bytes
  for (int m = 0; m < npow; m++)
    for (int cw = 0; cw < rw; cw += 2) {
      const uint32_t x = nar_mb_word(bs, npow, m, cw);
      if ((x & 1) || nar_mb_word(bs, npow, m, cw + 1) != x + 1) fail("pair", npow, m, cw, x);
      checks++;
    }
}

int main() {
  compare_prev_base();
  staging_layout(1024, 64);
  staging_layout(1024, 128);
  staging_layout(1024, 256);
  // the granule's flag bit leaves the epoch intact
  for (uint32_t ep : {1u, 2u, 2837u, 0x7FFFFFFFu}) {
    if (((ep | kNarGranFlag) & ~kNarGranFlag) != ep || (ep & kNarGranFlag)) fail("granule flag", ep, 0, 0, 0);
    checks++;
  }
  printf("ok %ld\n", checks);
  return 0;
}
