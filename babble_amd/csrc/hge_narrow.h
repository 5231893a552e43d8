// hge_narrow.h — the 8-bit frontier-relative form of the direct rounds kernel's
// strongly-see compare (hge_rounds_direct.hip).  Plain functions
// over packed words that compile for the host and the device: the kernel encodes
// and counts with them, tests/abi/hge_narrow_test.cpp checks them on the CPU.
//
// The kernel's 16-bit operands are LAe = LA + 2 (0 = no row) and FDe = FD + 1
// (0xFFFF = unset / no member), two columns per word; a column passes when
// LAe > FDe (LA >= FD).  Per column i the narrow form is relative to a base B[i]
// that both sides share (kept as a uint16, nar_base16):
//   window value  a = min(LAe -sat B, 126)      = clamp(LA - B + 2, 0, 126)
//   member value  b = min(FDe -sat B, 126) + 1  = clamp(FD - B + 2, 1, 127)
// four columns per word, each 7-bit value under a guard bit: the window words are
// stored with the guard bits set, so aw - bw never borrows across fields and leaves
// [a >= b] in each guard bit (nar_ge4).
//
// a >= b equals LAe > FDe, whatever the base, unless
//   (i)  some a saturates (LAe - B >= 126: the row runs past the range), or
//   (ii) a finite FD lies below its base (FDe <= B: the clamp at 1 loses the order),
// which the encoders report (nar_window_flag, nar_member_flag); the kernel then
// takes the 16-bit select for that round.  An unset FDe = 0xFFFF must encode as 127,
// which holds while B <= kNarBaseMax; the kernel checks the bases for that.  A
// chain without a frontier position has the base kNarBaseNone: its window values
// are at most 1, an unset member value is 2 and a finite one raises (ii).
//
// The base of round r is the PREVIOUS frontier, B_r[i] = C_{r-1}[i] (the walk's first
// round: C_r itself): the workgroup that stages a member row for round r does so
// before it knows the other chains' C_r, but it holds C_{r-1} in full, so it stages
// the row already encoded (nar_mb_word says where) and no consumer encodes it again.
// (ii) cannot get worse by that: a finite FD[m_d][i] of a round-r member is the
// position of a descendant of a round-r event, hence >= C_r[i] >= C_{r-1}[i].  The
// window values grow by one round's advance of the column (at most ~33 at 256
// participants), towards (i).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGE_NAR_HD __host__ __device__ __forceinline__
#else
#define HGE_NAR_HD inline
#endif

namespace hge_narrow {

constexpr uint32_t kNarGuard = 0x80808080u;
constexpr uint32_t kNarAMax = 126;         // a window value at 126 counts as saturated
constexpr uint32_t kNarBaseNone = 0xFFFEu; // base of a chain without a frontier position
constexpr int32_t kNarBaseMax = 65400;     // 0xFFFF - C >= 126 for every base up to here
constexpr int32_t kNarInf32 = 0x7FFFFFFF;

HGE_NAR_HD uint32_t nar_base16(int32_t P) { return P == kNarInf32 ? kNarBaseNone : (uint32_t)P; }
// a frontier position the narrow form cannot take as a base
HGE_NAR_HD bool nar_base_too_large(int32_t P) { return P != kNarInf32 && P > kNarBaseMax; }

// per 16-bit half: x -sat c, min, max
HGE_NAR_HD uint32_t nar_sub_sat2(uint32_t x, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 r = __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, x), __builtin_bit_cast(u16x2, c));
  return __builtin_bit_cast(uint32_t, r);
#else
  const uint32_t xl = x & 0xFFFFu, cl = c & 0xFFFFu, xh = x >> 16, ch = c >> 16;
  return (xl > cl ? xl - cl : 0u) | ((xh > ch ? xh - ch : 0u) << 16);
#endif
}
HGE_NAR_HD uint32_t nar_min2(uint32_t x, uint32_t y) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 r = __builtin_elementwise_min(__builtin_bit_cast(u16x2, x), __builtin_bit_cast(u16x2, y));
  return __builtin_bit_cast(uint32_t, r);
#else
  const uint32_t xl = x & 0xFFFFu, yl = y & 0xFFFFu, xh = x >> 16, yh = y >> 16;
  return (xl < yl ? xl : yl) | ((xh < yh ? xh : yh) << 16);
#endif
}
HGE_NAR_HD uint32_t nar_max2(uint32_t x, uint32_t y) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 r = __builtin_elementwise_max(__builtin_bit_cast(u16x2, x), __builtin_bit_cast(u16x2, y));
  return __builtin_bit_cast(uint32_t, r);
#else
  const uint32_t xl = x & 0xFFFFu, yl = y & 0xFFFFu, xh = x >> 16, yh = y >> 16;
  return (xl > yl ? xl : yl) | ((xh > yh ? xh : yh) << 16);
#endif
}
// the low bytes of the four halves of (x0, x1) as one word: columns 0, 1 from x0, 2, 3 from x1
HGE_NAR_HD uint32_t nar_pack4(uint32_t x0, uint32_t x1) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(x1, x0, 0x06040200u);
#else
  return (x0 & 0xFFu) | ((x0 >> 8) & 0xFF00u) | ((x1 & 0xFFu) << 16) | ((x1 << 8) & 0xFF000000u);
#endif
}

// four window columns: (la0, la1) = LAe pairs, (c0, c1) = their bases.  Returns the
// word to store (guard bits set); mx accumulates the per-half maximum of LAe -sat C
// for nar_window_flag (start it at 0).
HGE_NAR_HD uint32_t nar_enc_window4(uint32_t la0, uint32_t la1, uint32_t c0, uint32_t c1, uint32_t& mx) {
  const uint32_t cap = kNarAMax | (kNarAMax << 16);
  const uint32_t x0 = nar_sub_sat2(la0, c0), x1 = nar_sub_sat2(la1, c1);
  mx = nar_max2(mx, nar_max2(x0, x1));
  return nar_pack4(nar_min2(x0, cap), nar_min2(x1, cap)) | kNarGuard;
}
// condition (i) fails: some encoded window value reached 126
HGE_NAR_HD bool nar_window_flag(uint32_t mx) { return (mx & 0xFFFFu) >= kNarAMax || (mx >> 16) >= kNarAMax; }

// four member columns: (fd0, fd1) = FDe pairs.  mn accumulates the per-half minimum
// of FDe -sat C for nar_member_flag (start it at 0xFFFFFFFF).
HGE_NAR_HD uint32_t nar_enc_member4(uint32_t fd0, uint32_t fd1, uint32_t c0, uint32_t c1, uint32_t& mn) {
  const uint32_t cap = kNarAMax | (kNarAMax << 16);
  const uint32_t t0 = nar_sub_sat2(fd0, c0), t1 = nar_sub_sat2(fd1, c1);
  mn = nar_min2(mn, nar_min2(t0, t1));
  return nar_pack4(nar_min2(t0, cap), nar_min2(t1, cap)) + 0x01010101u;
}
// condition (ii) fails: some FDe <= C
HGE_NAR_HD bool nar_member_flag(uint32_t mn) { return (mn & 0xFFFFu) == 0 || (mn >> 16) == 0; }

// [a >= b] of the four fields in their guard bits (aw with guard bits set, bw without)
HGE_NAR_HD uint32_t nar_ge4(uint32_t aw, uint32_t bw) { return (aw - bw) & kNarGuard; }

// The staged narrow member rows (one block of npow x npow bytes per round parity), laid
// out by consuming thread, chunk-major: thread tid = member * tpm + part of a workgroup
// of bs threads holds the ncw words of columns [part * 4 ncw, (part + 1) * 4 ncw) of its
// member's row, and loads them vw words at a time; word (k * bs + tid) * vw + s of the
// block is word k * vw + s of that slice.  Load k of a wave is then one contiguous
// stretch, and a thread's loads hold bytes of its own member only.
// cw = column / 4: the word's place in the member's row.
HGE_NAR_HD int nar_mb_ncw(int bs, int npow) { return npow / 4 / (bs / npow); }
HGE_NAR_HD int nar_mb_vw(int bs, int npow) {
  const int ncw = nar_mb_ncw(bs, npow);
  return ncw % 4 == 0 ? 4 : ncw % 2 == 0 ? 2 : 1;
}
HGE_NAR_HD uint32_t nar_mb_word(int bs, int npow, int member, int cw) {
  const int tpm = bs / npow, ncw = nar_mb_ncw(bs, npow), vw = nar_mb_vw(bs, npow);
  const int part = cw / ncw, j = cw - part * ncw, k = j / vw;
  return (uint32_t)((k * bs + member * tpm + part) * vw + (j - k * vw));
}

// The member row's condition-(ii) flag travels in the hand-off granule: the top bit of
// its epoch word (epochs stay far below 2^31).
constexpr uint32_t kNarGranFlag = 0x80000000u;

}  // namespace hge_narrow
