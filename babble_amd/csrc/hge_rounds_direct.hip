// hge_rounds_direct.hip — DivideRounds for wide hashgraphs (N > 32) by batched
// strongly-see tiles: the frontier recurrence of DESIGN.md §4.2 evaluated
// directly on the coordinate rows, one co-resident workgroup per chain.
//
//   C_{r+1}[c] = min { p >= C_r[c] : #{d : StronglySee((c, p), m_d)} >= SM },
//   StronglySee(x, m) = #{i : LA[x][i] >= FD[m][i]} >= SM   (hashgraph.go:180-208)
//
// where m_d = (d, C_r[d]) are the round-r frontier members.  StronglySee is
// monotone along a chain (LA rows only grow), so the first position is found
// by bisection over a window of candidate rows of chain c.
//
// Per round and workgroup (target chain c):
//   * thread (d, part) holds its slice of member row FD[m_d] in registers as
//     packed uint16 (FD + 1, 0xFFFF = unset / no member);
//   * the candidate rows LA[(c, p)], p in [C_r[c], C_r[c] + W), sit in LDS as
//     packed uint16 (LA + 2), staged while the previous round's hand-off was in
//     flight (they are chain c's own rows: known as soon as C_{r+1}[c] is);
//   * a probe of position p is one pass of packed saturating subtractions
//     (la + 2 -sat m + 1 > 0  <=>  la >= m) over the member slice, a sum over
//     the TPM lanes of a member, a wave ballot of the members that pass and
//     one LDS add per wave: a W x N x N strongly-see tile costs log2(W) + 1
//     probes, all compares on registers and LDS (no gathers).
// The strongly-see bits of the selected event against every member (ssc: the
// vote adjacency k_witness_bits consumes) are one more probe.
// The narrow widths (HGE_DIR_NARROW_*) run the same search over 8-bit copies of both
// sides, relative to the previous frontier (hge_narrow.h): the member slice arrives in
// that form from its producer, the window's first half is encoded after the pick, and
// the 16-bit slice is loaded only by the rare paths that need it.
//
// The frontier hand-off between workgroups is the granule protocol of
// hge_rounds_coop.hip (8-byte {epoch, value} granules, relaxed agent-scope
// stores and loads, double-buffered by round parity; cdna_hip_programming.md
// Guideline 16, R2).  Chain positions must fit uint16 with room for the +2
// encoding: the engine runs this kernel only while every chain holds at most
// 65,534 events; a longer chain switches it to int32 positions for good
// (hge_wide32.hip, k_round_step32).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hge_narrow.h"

// Widths whose select runs over the 8-bit frontier-relative rows (hge_narrow.h): a
// width built with 0 keeps the 16-bit select of every round (DESIGN.md §4.2 says which
// widths ended where, and why).
#ifndef HGE_DIR_NARROW_64
#define HGE_DIR_NARROW_64 1
#endif
#ifndef HGE_DIR_NARROW_128
#define HGE_DIR_NARROW_128 1
#endif
#ifndef HGE_DIR_NARROW_256
#define HGE_DIR_NARROW_256 1
#endif

namespace hge {

// section stamps (HGE_STAMPS) are compiled in only with -DHGE_DIR_STAMPS: the
// accumulators otherwise cost registers (and spills) in the round loop
#ifdef HGE_DIR_STAMPS
constexpr bool kDirStamps = true;
#else
constexpr bool kDirStamps = false;
#endif
constexpr int DIR_MAXP = 16;  // probe counters per window (2 + log2(W) are used)
constexpr int DIR_CH = 32;    // rows per fetch chunk (a round advances ~EPR/N ~ 14 rows)

template <int BS, int NPOW>
struct DirGeo {
  // candidate rows staged per window: 64 for 1024-thread workgroups (one per CU), 32 for
  // 512-thread ones (two per CU, e.g. two walkers of one hashgraph side by side)
  static constexpr int W = BS >= 1024 ? 64 : 32;
  static constexpr int TPM = BS / NPOW;       // threads per member
  static constexpr int CPT = NPOW / TPM;      // columns per thread (NPOW^2 / BS)
  static constexpr int CW = CPT / 2;          // packed words per thread
  static constexpr int VW = (CW % 4 == 0) ? 4 : 2;  // words per LDS read (b128 / b64)
  static constexpr int PS = CW + VW;          // LDS words per (row, part): parts on distinct banks
  static constexpr int RS = TPM * PS;         // LDS words per candidate row
  static constexpr int WIN_INTS = W * NPOW;      // ints of a full window (N = NPOW)
  static constexpr int PREF = (DIR_CH * NPOW / 4 + BS - 1) / BS;  // int4 per thread and chunk
  static constexpr int MBW = NPOW / 2;        // staged member row: packed words
  static constexpr int MVW = (CW % 4 == 0) ? 4 : 2;  // MB words per thread chunk (16 / 8 bytes)
  // the narrow copy (hge_narrow.h): the first H window rows, four columns per word
  static constexpr bool NARROW = NPOW <= 64 ? HGE_DIR_NARROW_64 != 0
                               : NPOW <= 128 ? HGE_DIR_NARROW_128 != 0 : HGE_DIR_NARROW_256 != 0;
  static constexpr int H = W / 2;             // rows the per-member bisection covers
  static constexpr int NCW = CW / 2;          // narrow words per thread
  static constexpr int NVW = (NCW % 4 == 0) ? 4 : (NCW % 2 == 0) ? 2 : 1;  // words per LDS read
  static constexpr int NPS = NCW + NVW;       // LDS words per (row, part), padded like PS
  static constexpr int NRS = TPM * NPS;       // LDS words per narrow row
  static constexpr int NENC = (H * NPOW / 4 + BS - 1) / BS;  // narrow words a thread re-encodes per round
};

// threadIdx.x, opaque to the optimiser: what a section of the round loop derives from it
// (row and column of a fetch slot, LDS and table addresses) is then formed in that
// section, and not held in registers across the whole loop.  The <1024, 256> kernel
// sits at the 128 VGPRs of 16 waves per CU; held addresses were what spilled.
__device__ __forceinline__ int dir_tid() {
  int x = threadIdx.x;
  asm volatile("" : "+v"(x));
  return x;
}

template <int BS, int NPOW>
struct DirLDS {
  int sP[256];
  uint32_t sLA[DirGeo<BS, NPOW>::W * DirGeo<BS, NPOW>::RS] __attribute__((aligned(16)));
  int sCnt[DIR_MAXP];
  int sCntW[DIR_MAXP][BS / 64] __attribute__((aligned(16)));  // per-wave passing members of a probe
  int sHist[DirGeo<BS, NPOW>::W / 2];  // members by first passing offset (dir_select_pm)
  uint32_t sBits[8];
  // the narrow select's copy: the frontier positions as packed uint16 bases, laid out
  // like one ring row (part * PS + word), by round parity (sB16[r & 1] = C_r: what round
  // r encodes against, for round r + 1, while its poll already writes the other one),
  // and rows [lo, lo + H) of the ring encoded against the previous frontier
  uint32_t sB16[2][DirGeo<BS, NPOW>::NARROW ? DirGeo<BS, NPOW>::RS : 4] __attribute__((aligned(16)));
  uint32_t sN[DirGeo<BS, NPOW>::NARROW ? DirGeo<BS, NPOW>::H * DirGeo<BS, NPOW>::NRS : 4] __attribute__((aligned(16)));
  int sEx[2];            // per round parity: nonzero = the narrow form is not exact this round
  int sBig;              // sticky: some frontier position was too large to be a base
  int sFlag[2];          // per round parity: 1 = some member exists, 2 = some chain below stopcut, 4 = hand-off failed
  int s_stamp;          // HGE_STAMPS: thread 0 accumulates probe phases into sdbg
  uint64_t sdbg[2];     // [0] count (LDS reads + VALU), [1] reduce + barrier + read
};

__device__ __forceinline__ uint32_t dir_pack_la(int a, int b) {
  return (uint32_t)(a + 2) | ((uint32_t)(b + 2) << 16);
}
__device__ __forceinline__ uint32_t dir_pack_fd(int a, int b) {
  const uint32_t lo = a == INF32 ? 0xFFFFu : (uint32_t)(a + 1);
  const uint32_t hi = b == INF32 ? 0xFFFFu : (uint32_t)(b + 1);
  return lo | (hi << 16);
}

// The candidate rows live in an LDS ring of W rows: row p of chain c sits in
// slot p % W, and the ring holds [lo, lo + W) for the current lo.  Moving
// the window from lo to lo' only fetches rows [max(lo + W, lo'), lo' + W): ~EPR/N
// rows per round instead of W.
// dir_fetch: rows [p0, p0 + min(nr, DIR_CH)) of chain c into registers (8-byte slices of
// the contiguous chain-major packed rows; rows >= lenc become "no row").  N % 4 == 0
// (the host takes the gather path of hge_rounds_coop.hip otherwise).
template <int BS, int NPOW>
__device__ __forceinline__ void dir_fetch(const Tables& t, int c, int p0, int nr, int lenc,
                                          uint2 (&v)[DirGeo<BS, NPOW>::PREF]) {
  using G = DirGeo<BS, NPOW>;
  const int N = t.N;
  nr = min(nr, DIR_CH);
  const int have = (p0 == INF32 || nr <= 0) ? 0 : max(0, min(nr, lenc - p0));
  if (have == 0) return;  // block-uniform
  // the packed rows (LA + 1 as uint16 pairs, N / 2 words per row): 4 columns = 8 bytes
  const uint32_t* base = t.LA16 + ((size_t)c * t.ccap + p0) * (size_t)t.NW2;
  // unconditional loads (rows past `have` re-read the last fetched row; dir_store
  // drops them): no value select behind each load, so all of them stay in flight
  const int qmax = have * N / 4 - 1;
  const int tx = dir_tid();
#pragma unroll
  for (int m = 0; m < G::PREF; m++) {
    const int q = min(tx + m * BS, qmax);  // 4-column group in the fetched rows
    v[m] = *(const uint2*)(base + 2 * (size_t)q);
  }
}

// the fetched rows [p0, p0 + nr) -> their ring slots (caller syncs before a
// probe); rows at or past lenc are stored as "no row" (0: never >= a member value)
template <int BS, int NPOW>
__device__ __forceinline__ void dir_store(const Tables& t, DirLDS<BS, NPOW>& L, int p0, int nr, int lenc,
                                          uint2 (&v)[DirGeo<BS, NPOW>::PREF]) {
  using G = DirGeo<BS, NPOW>;
  const int N = t.N;
  if (p0 == INF32 || nr <= 0) return;
  nr = min(nr, DIR_CH);
  const int have = max(0, min(nr, lenc - p0));
  const int tx = dir_tid();
#pragma unroll
  for (int m = 0; m < G::PREF; m++) {
    const int q = tx + m * BS;
    const int row = (4 * q) / N;
    if (row >= nr) continue;
    // LA16 + 1 per half = the LA + 2 encoding (LA <= 65,533: no carry); a row past the
    // chain's end is "no row" (0)
    const bool hv = row < have;
    // the 4 columns lie in one part (CPT is a multiple of 4).  Columns past N are
    // never written: their member values are 0xFFFF, which no row value passes.
    const int col = 4 * q - row * N;
    const int part = col / G::CPT, w = (col - part * G::CPT) / 2;
    const int slot = (p0 + row) & (DirGeo<BS, NPOW>::W - 1);
    uint2* dst = (uint2*)(L.sLA + slot * G::RS + part * G::PS + w);
    *dst = hv ? make_uint2(v[m].x + 0x00010001u, v[m].y + 0x00010001u) : make_uint2(0u, 0u);
  }
}

// rows [p0, p0 + nr) into their ring slots, chunk by chunk (caller syncs before a probe)
template <int BS, int NPOW>
__device__ __forceinline__ void dir_load(const Tables& t, DirLDS<BS, NPOW>& L, int c, int p0, int nr, int lenc,
                                         uint2 (&v)[DirGeo<BS, NPOW>::PREF]) {
  if (p0 == INF32) return;
  for (int q = 0; q < nr; q += DIR_CH) {
    dir_fetch<BS, NPOW>(t, c, p0 + q, nr - q, lenc, v);
    dir_store<BS, NPOW>(t, L, p0 + q, nr - q, lenc, v);
  }
}

// member slice of thread (d, part) for the first round: FD[(d, Pd)][part * CPT, +CPT)
// packed (FD + 1); N % 4 == 0, so every int4 is wholly inside or past the row
template <int BS, int NPOW>
__device__ __forceinline__ void dir_members_fd(const Tables& t, int d, int part, int Pd,
                                               uint32_t (&mw)[DirGeo<BS, NPOW>::CW]) {
  using G = DirGeo<BS, NPOW>;
  const int N = t.N;
  const int c0 = part * G::CPT;
  const bool act = d < N && Pd != INF32;
  if (t.FD16) {  // the rows are stored packed already (FD + 1, 0xFFFF = none)
    const uint16_t* row = t.FD16 + rowoff(t, act ? d : 0, act ? Pd : 0);
#pragma unroll
    for (int k = 0; k < G::CW / 2; k++) {
      uint2 a = *(const uint2*)(row + min(c0 + 4 * k, N - 4));
      if (!act || c0 + 4 * k >= N) a = make_uint2(~0u, ~0u);
      mw[2 * k] = a.x;
      mw[2 * k + 1] = a.y;
    }
    return;
  }
  const int32_t* row = t.FD + rowoff(t, act ? d : 0, act ? Pd : 0);
#pragma unroll
  for (int k = 0; k < G::CW / 2; k++) {
    // unconditional loads from a valid address, then the select
    int4 a = *(const int4*)(row + min(c0 + 4 * k, N - 4));
    if (!act || c0 + 4 * k >= N) a = make_int4(INF32, INF32, INF32, INF32);
    mw[2 * k] = dir_pack_fd(a.x, a.y);
    mw[2 * k + 1] = dir_pack_fd(a.z, a.w);
  }
}

// Member rows after the first round come from the staging block MB[parity]:
// the workgroup of chain d packs its next frontier row FD[(d, C_{r+1}[d])] there
// (wave 0, write-through 8-byte stores, vmcnt(0), then the granule).  MB is laid
// out by consuming thread, chunk-major: word (k * BS + tid) * MVW + s holds word
// k * MVW + s of thread tid's slice, so load k of a wave reads one contiguous
// 64 * 4 * MVW bytes (a row-major block made every wave load touch 64 cache
// lines for 16 bytes each: TA-bound, ~13k cycles per round at N = 256).  The
// granule poll is the flag; every load of the block is an sc1 load, as the
// granule protocol requires (MI355X_MICROARCH.md, Valid forms, row 1).
template <int BS, int NPOW>
__device__ __forceinline__ void dir_members_mb(const uint32_t* mb, uint32_t (&mw)[DirGeo<BS, NPOW>::CW]) {
  using G = DirGeo<BS, NPOW>;
  constexpr int MVW = G::MVW;
  // buffer_load sc1 (aux bit 4; the table row allows 4-, 8- and 16-byte loads of
  // 8-byte sc1 stores); 8-byte loads run at 0.54-0.70x the 16-byte rate
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)mb, 0, BS * G::CW * 4, 0x00020000);
  const int tx = dir_tid();
#pragma unroll
  for (int k = 0; k < G::CW / MVW; k++) {
    const int off = (k * BS + tx) * MVW * 4;
    if constexpr (MVW == 4) {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16);
      mw[4 * k] = x.x;
      mw[4 * k + 1] = x.y;
      mw[4 * k + 2] = x.z;
      mw[4 * k + 3] = x.w;
    } else {
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      const u32x2 x = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 16);
      mw[2 * k] = x.x;
      mw[2 * k + 1] = x.y;
    }
  }
}

// The narrow slice of the thread from the narrow staging block (hge_narrow.h,
// nar_mb_word): the same sc1 buffer loads, half the bytes, nothing to encode.
template <int BS, int NPOW>
__device__ __forceinline__ void dir_members_nb(const uint32_t* nb, uint32_t (&nw)[DirGeo<BS, NPOW>::NCW]) {
  using G = DirGeo<BS, NPOW>;
  constexpr int NVW = G::NVW;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)nb, 0, BS * G::NCW * 4, 0x00020000);
  const int tx = dir_tid();
#pragma unroll
  for (int k = 0; k < G::NCW / NVW; k++) {
    const int off = (k * BS + tx) * NVW * 4;
    if constexpr (NVW == 4) {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16);
      nw[4 * k] = x.x;
      nw[4 * k + 1] = x.y;
      nw[4 * k + 2] = x.z;
      nw[4 * k + 3] = x.w;
    } else if constexpr (NVW == 2) {
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      const u32x2 x = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 16);
      nw[2 * k] = x.x;
      nw[2 * k + 1] = x.y;
    } else {
      nw[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 16);
    }
  }
}

// wave 0 of chain c's workgroup: stage FD[(c, p)] (p = INF32: no member) into MB,
// read from HBM after the pick.  (Round 3 staged every window row's FD row in LDS
// ahead of the pick so the stage read LDS: ~10 GB of the kernel's traffic per
// 256/10M replay for no measured time, 24.57-24.68 vs 24.62-24.69 ms in a
// same-box A/B, profiles/r04/abfd_*.)
// Lane l packs columns 4l .. 4l + 3 into row words 2l, 2l + 1 (one part, one chunk).
// nb != nullptr (the narrow widths): the row also goes out in its 8-bit form, encoded
// against `bases` (the frontier this workgroup holds in full, L.sB16 of the round that
// publishes: the next round's base), one word per lane; the even lane of a pair takes
// its neighbour's word by DPP, so these are 8-byte stores of the same kind.  Returns
// whether the row breaks condition (ii) (wave-uniform; it travels in the granule).
template <int BS, int NPOW>
__device__ __forceinline__ bool dir_stage_member(const Tables& t, uint32_t* mb, uint32_t* nb, const uint32_t* bases,
                                                 int c, int p) {
  using G = DirGeo<BS, NPOW>;
  constexpr int MVW = G::MVW;
  int lane = threadIdx.x;  // < 64
  // (opaque to the optimiser: the row addresses below are then formed here, once per
  // round in one wave, and not kept in registers across the whole round loop)
  asm volatile("" : "+v"(lane));
  const int N = t.N;
  const bool act = 4 * lane < NPOW;
  uint2 a = make_uint2(~0u, ~0u);
  if (act) {
    if (t.FD16) {  // stored packed already
      if (p != INF32 && 4 * lane < N) a = *(const uint2*)(t.FD16 + rowoff(t, c, p) + 4 * lane);
    } else {
      int4 f = make_int4(INF32, INF32, INF32, INF32);
      if (p != INF32 && 4 * lane < N) f = *(const int4*)(t.FD + rowoff(t, c, p) + 4 * lane);
      a = make_uint2(dir_pack_fd(f.x, f.y), dir_pack_fd(f.z, f.w));
    }
    const int w = 2 * lane, part = w / G::CW, wp = w - part * G::CW;
    const int k = wp / MVW, sub = wp - k * MVW;
    const size_t word = ((size_t)k * BS + (size_t)c * G::TPM + part) * MVW + sub;
    const unsigned long long x = (unsigned long long)a.x | ((unsigned long long)a.y << 32);
    __hip_atomic_store((gu64_t*)(mb + word), x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if constexpr (G::NARROW) {
    if (nb) {
      uint32_t mn = 0xFFFFFFFFu, word = 0;
      if (act) {
        const int w = 2 * lane, part = w / G::CW;
        const uint2 cb = *(const uint2*)(bases + part * G::PS + (w - part * G::CW));
        word = hge_narrow::nar_enc_member4(a.x, a.y, cb.x, cb.y, mn);
      }
      // every lane of the wave is here: lanes 2m and 2m + 1 are both staging or both idle
      const uint32_t odd = (uint32_t)__builtin_amdgcn_mov_dpp((int)word, 0xF5, 0xF, 0xF, false);  // quad_perm [1, 1, 3, 3]
      if (act && (lane & 1) == 0) {
        const unsigned long long x = (unsigned long long)word | ((unsigned long long)odd << 32);
        __hip_atomic_store((gu64_t*)(nb + hge_narrow::nar_mb_word(BS, NPOW, c, lane)), x, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      return __ballot(act && hge_narrow::nar_member_flag(mn)) != 0;
    }
  }
  return false;
}

// strongly-see count of candidate position p (in the ring) against this
// thread's member slice, summed over the member's TPM lanes
template <int BS, int NPOW>
__device__ __forceinline__ int dir_count(const DirLDS<BS, NPOW>& L, int p, int part,
                                         const uint32_t (&mw)[DirGeo<BS, NPOW>::CW]) {
  using G = DirGeo<BS, NPOW>;
  const uint32_t* src = L.sLA + (p & (DirGeo<BS, NPOW>::W - 1)) * G::RS + part * G::PS;
  uint32_t acc0 = 0, acc1 = 0;
  const uint32_t ones = 0x00010001u;
  static_assert(G::CW % 2 == 0, "member slices are whole word pairs");
  static_assert(G::CW % G::VW == 0, "LDS reads cover whole slices");
  // one LDS read of VW words, then its word pairs: only VW row words are live at a
  // time (a 512-thread workgroup holds 64 member words per thread)
#pragma unroll
  for (int k0 = 0; k0 < G::CW; k0 += G::VW) {
    uint32_t la[G::VW];
    if constexpr (G::VW == 4) {
      const uint4 q = *(const uint4*)(src + k0);
      la[0] = q.x;
      la[1] = q.y;
      la[2] = q.z;
      la[3] = q.w;
    } else {
      const uint2 q = *(const uint2*)(src + k0);
      la[0] = q.x;
      la[1] = q.y;
    }
#pragma unroll
    for (int k = 0; k < G::VW; k += 2) {
      // (la + 2) -sat (m + 1) is nonzero <=> la >= m (v_pk_sub_u16 clamp saturates at 0);
      // min(., 1) per half, then a packed add: 3 VALU ops per 2 columns.  Two words per
      // asm statement and two accumulators (no dependent chain, and the compiler's
      // hazard padding between asm statements falls on every other word pair at most)
      uint32_t d0, d1;
      asm("v_pk_sub_u16 %0, %4, %6 clamp\n\t"
          "v_pk_sub_u16 %1, %5, %7 clamp\n\t"
          "v_pk_min_u16 %0, %0, %8\n\t"
          "v_pk_min_u16 %1, %1, %8\n\t"
          "v_pk_add_u16 %2, %2, %0\n\t"
          "v_pk_add_u16 %3, %3, %1"
          : "=&v"(d0), "=&v"(d1), "+v"(acc0), "+v"(acc1)
          : "v"(la[k]), "v"(la[k + 1]), "v"(mw[k0 + k]), "v"(mw[k0 + k + 1]), "v"(ones));
    }
  }
  int cnt = (int)(acc0 & 0xFFFFu) + (int)(acc0 >> 16) + (int)(acc1 & 0xFFFFu) + (int)(acc1 >> 16);
  // sum over the member's TPM consecutive lanes by DPP (no LDS permutes): quad_perm
  // xor 1 and xor 2, then row_half_mirror (quads of an 8) and row_mirror (8s of a row)
  if constexpr (G::TPM > 1) cnt += __builtin_amdgcn_mov_dpp(cnt, 0xB1, 0xF, 0xF, false);
  if constexpr (G::TPM > 2) cnt += __builtin_amdgcn_mov_dpp(cnt, 0x4E, 0xF, 0xF, false);
  if constexpr (G::TPM > 4) cnt += __builtin_amdgcn_mov_dpp(cnt, 0x141, 0xF, 0xF, false);
  if constexpr (G::TPM > 8) cnt += __builtin_amdgcn_mov_dpp(cnt, 0x140, 0xF, 0xF, false);
  static_assert(G::TPM <= 16, "a member's lanes lie in one DPP row");
  return cnt;
}

// ---- the narrow form (hge_narrow.h): the same counts over 8-bit fields relative to the
// column's frontier position, four columns per word and compare ----

// where column d's uint16 base sits in L.sB16 (halves; the row layout of the ring)
template <int BS, int NPOW>
__device__ __forceinline__ int dir_base_slot(int d) {
  using G = DirGeo<BS, NPOW>;
  const int w = d >> 1, part = w / G::CW;
  return 2 * (part * G::PS + (w - part * G::CW)) + (d & 1);
}

// rows [lo, lo + H) of the 16-bit ring encoded into L.sN against `bases` (row k =
// position lo + k; "no row" entries and columns past N become 0, which passes no
// member value).  Returns the accumulator for nar_window_flag.
template <int BS, int NPOW>
__device__ __forceinline__ uint32_t dir_encode_window(const Tables& t, DirLDS<BS, NPOW>& L, const uint32_t* bases,
                                                      int lo) {
  using G = DirGeo<BS, NPOW>;
  constexpr int GPR = NPOW / 4;  // 4-column groups per row
  uint32_t mx = 0;
  const int tx = dir_tid();
#pragma unroll
  for (int m = 0; m < G::NENC; m++) {
    const int q = tx + m * BS;
    if (q >= G::H * GPR) continue;
    const int k = q / GPR, col = 4 * (q - k * GPR);
    const int part = col / G::CPT, cp = col - part * G::CPT;
    const int off = part * G::PS + cp / 2;
    uint32_t word = hge_narrow::kNarGuard;
    if (col < t.N) {
      const uint2 la = *(const uint2*)(L.sLA + ((lo + k) & (G::W - 1)) * G::RS + off);
      const uint2 cb = *(const uint2*)(bases + off);
      word = hge_narrow::nar_enc_window4(la.x, la.y, cb.x, cb.y, mx);
    }
    L.sN[k * G::NRS + part * G::NPS + cp / 4] = word;
  }
  return mx;
}

// the thread's 16-bit member slice encoded against the bases of its columns (the walk's
// first round: later rounds' rows are staged encoded, dir_stage_member); returns the
// accumulator for nar_member_flag
template <int BS, int NPOW>
__device__ __forceinline__ uint32_t dir_encode_members(const uint32_t* bases, int part,
                                                       const uint32_t (&mw)[DirGeo<BS, NPOW>::CW],
                                                       uint32_t (&nw)[DirGeo<BS, NPOW>::NCW]) {
  using G = DirGeo<BS, NPOW>;
  const uint32_t* src = bases + part * G::PS;
  uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
  for (int k0 = 0; k0 < G::CW; k0 += G::VW) {
    uint32_t cb[G::VW];
    if constexpr (G::VW == 4) {
      const uint4 q = *(const uint4*)(src + k0);
      cb[0] = q.x;
      cb[1] = q.y;
      cb[2] = q.z;
      cb[3] = q.w;
    } else {
      const uint2 q = *(const uint2*)(src + k0);
      cb[0] = q.x;
      cb[1] = q.y;
    }
#pragma unroll
    for (int k = 0; k < G::VW; k += 2)
      nw[(k0 + k) / 2] = hge_narrow::nar_enc_member4(mw[k0 + k], mw[k0 + k + 1], cb[k], cb[k + 1], mn);
  }
  return mn;
}

// dir_count over the narrow rows: window offset k (position lo + k, k < H) against the
// narrow member slice.  One subtract, one mask and one population count per 4 columns.
template <int BS, int NPOW>
__device__ __forceinline__ int dir_count_n(const DirLDS<BS, NPOW>& L, int k, int part,
                                           const uint32_t (&nw)[DirGeo<BS, NPOW>::NCW]) {
  using G = DirGeo<BS, NPOW>;
  const uint32_t* src = L.sN + k * G::NRS + part * G::NPS;
  // v_bcnt_u32_b32 adds its count to an operand (left to the compiler, the sums are
  // reassociated into a count, a count and a three-way add per two words); two
  // accumulators, as in dir_count
  uint32_t acc0 = 0, acc1 = 0;
#pragma unroll
  for (int k0 = 0; k0 < G::NCW; k0 += G::NVW) {
    uint32_t a[G::NVW];
    if constexpr (G::NVW == 4) {
      const uint4 q = *(const uint4*)(src + k0);
      a[0] = q.x;
      a[1] = q.y;
      a[2] = q.z;
      a[3] = q.w;
    } else if constexpr (G::NVW == 2) {
      const uint2 q = *(const uint2*)(src + k0);
      a[0] = q.x;
      a[1] = q.y;
    } else {
      a[0] = src[k0];
    }
#pragma unroll
    for (int j = 0; j < G::NVW; j++) {
      const uint32_t ge = hge_narrow::nar_ge4(a[j], nw[k0 + j]);
      if (j & 1) asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc1) : "v"(ge));
      else asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc0) : "v"(ge));
    }
  }
  int cnt = (int)(acc0 + acc1);
  if constexpr (G::TPM > 1) cnt += __builtin_amdgcn_mov_dpp(cnt, 0xB1, 0xF, 0xF, false);
  if constexpr (G::TPM > 2) cnt += __builtin_amdgcn_mov_dpp(cnt, 0x4E, 0xF, 0xF, false);
  if constexpr (G::TPM > 4) cnt += __builtin_amdgcn_mov_dpp(cnt, 0x141, 0xF, 0xF, false);
  if constexpr (G::TPM > 8) cnt += __builtin_amdgcn_mov_dpp(cnt, 0x140, 0xF, 0xF, false);
  return cnt;
}

// The 16-bit member slice of round r, for the paths that need it (the exact select,
// dir_probe_search, a kept frontier row outside the narrow rows): from MB[r & 1],
// which no producer writes before this workgroup has published round r + 1, or in
// the walk's first round from the FD table.  Call it before the round's publish.
template <int BS, int NPOW>
__device__ __forceinline__ void dir_members_reload(const Tables& t, const DirLDS<BS, NPOW>& L, const uint32_t* mb,
                                                   bool first, int d, int part,
                                                   uint32_t (&mw)[DirGeo<BS, NPOW>::CW]) {
  using G = DirGeo<BS, NPOW>;
  if (first) {
    // (opaque to the optimiser, as in dir_stage_member: the table addresses of a rare
    // path are formed here and not kept in registers across the round loop)
    asm volatile("" : "+v"(d), "+v"(part));
    dir_members_fd<BS, NPOW>(t, d, part, d < t.N ? L.sP[d] : INF32, mw);
  } else {
    dir_members_mb<BS, NPOW>(mb, mw);
  }
  if (d >= t.N) {
#pragma unroll
    for (int k = 0; k < G::CW; k++) mw[k] = 0xFFFFFFFFu;
  }
}

// one probe: number of members strongly seen by candidate position p; `pass` =
// this thread's member is strongly seen
template <int BS, int NPOW>
__device__ __forceinline__ int dir_probe(const Tables& t, DirLDS<BS, NPOW>& L, int p, int part, int slot,
                                         const uint32_t (&mw)[DirGeo<BS, NPOW>::CW], bool& pass) {
  const bool st = kDirStamps && L.s_stamp && threadIdx.x == 0;
  const uint64_t t0 = st ? stamp() : 0;
  const int cnt = dir_count<BS, NPOW>(L, p, part, mw);
  pass = cnt >= t.SM;
  const uint64_t t1 = st ? stamp() : 0;
  // each wave stores its own count (no same-address LDS atomics serialising the
  // waves ahead of the barrier), then every thread sums the BS / 64 counts
  const uint64_t b = __ballot(part == 0 && pass);
  if ((threadIdx.x & 63) == 0) L.sCntW[slot][threadIdx.x >> 6] = (int)__builtin_popcountll(b);
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int w = 0; w < BS / 64; w += 4) {
    const int4 q = *(const int4*)&L.sCntW[slot][w];
    r += q.x + q.y + q.z + q.w;
  }
  if (st) {
    L.sdbg[0] += t1 - t0;
    L.sdbg[1] += stamp() - t1;
  }
  return r;
}

// dir_probe over the narrow rows: window offset k < H against the narrow member slice
template <int BS, int NPOW>
__device__ __forceinline__ int dir_probe_n(const Tables& t, DirLDS<BS, NPOW>& L, int k, int part, int slot,
                                           const uint32_t (&nw)[DirGeo<BS, NPOW>::NCW], bool& pass) {
  pass = dir_count_n<BS, NPOW>(L, k, part, nw) >= t.SM;
  const uint64_t b = __ballot(part == 0 && pass);
  if ((threadIdx.x & 63) == 0) L.sCntW[slot][threadIdx.x >> 6] = (int)__builtin_popcountll(b);
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int w = 0; w < BS / 64; w += 4) {
    const int4 q = *(const int4*)&L.sCntW[slot][w];
    r += q.x + q.y + q.z + q.w;
  }
  return r;
}

// Probe bisection for the first passing row at or after window offset a (the
// fallback of dir_select: rare).  Every probe counts all members at one row (a
// barrier each); the window's last row is probed first, and when it fails the
// next window is loaded.  pb = this thread's member pass flag at the returned row.
template <int BS, int NPOW>
__device__ int dir_probe_search(const Tables& t, int c, int lenc, DirLDS<BS, NPOW>& L, int part,
                                const uint32_t (&mw)[DirGeo<BS, NPOW>::CW], int& slot,
                                uint2 (&pv)[DirGeo<BS, NPOW>::PREF], int& lo, bool& pb, int a) {
  constexpr int W = DirGeo<BS, NPOW>::W;
  const int SM = t.SM;
  for (;;) {
    const int last = min(W, lenc - lo) - 1;
    if (a <= last) {
      bool ps;
      int b = last;
      if (dir_probe<BS, NPOW>(t, L, lo + b, part, slot++, mw, ps) >= SM) {
        pb = ps;
        while (a < b) {
          const int mid = (a + b) >> 1;
          if (dir_probe<BS, NPOW>(t, L, lo + mid, part, slot++, mw, ps) >= SM) {
            b = mid;
            pb = ps;
          } else {
            a = mid + 1;
          }
        }
        return lo + a;
      }
    }
    if (lo + W >= lenc) return INF32;
    // the answer lies past the window: the whole next window, fresh counters
    lo += W;
    __syncthreads();  // every thread has read this window's counters
    dir_load<BS, NPOW>(t, L, c, lo, W, lenc, pv);
    if (threadIdx.x < DIR_MAXP) L.sCnt[threadIdx.x] = 0;
    slot = 0;
    __syncthreads();
    a = 0;
  }
}

// C_{r+1}[c] before the end-of-chain clamp (INF32 = none yet) from the frontier
// in L.sP, the member slice mw and the window staged at lo (== L.sP[c]).
//
// Per member, not per probe: C_{r+1}[c] - lo is the SM-th smallest of the
// members' first passing offsets T_d = min{k : StronglySee((c, lo + k), m_d)}
// (StronglySee is monotone along the chain, so "count(k) >= SM" <=> "at least
// SM members have T_d <= k").  The TPM lanes of member d bisect T_d over the
// first half of the window on their own -- log2(W/2) counts of their slice
// against rows of the LDS ring, summed over the member's lanes by DPP, no
// barrier between steps -- and one LDS histogram of the T_d plus a wave prefix
// scan gives the SM-th smallest.  The last offset searched, e = min(W/2, rows
// left on the chain) - 1, also stands for "later" (not verified), so an answer
// there (or none) falls back to probe bisection from e on (dir_probe_search).  Round 2's probe bisection paid
// a workgroup barrier, an LDS count exchange and a ballot per probe (five to
// six per round, ~2.5k cycles each at N = 256); the counts here are the same
// N^2 compares per step, with one barrier per round.
// pb = this thread's member is strongly seen by the returned row.
//
// NAR: mw is the narrow slice and the counts are dir_count_n over L.sN (the caller
// has established that the narrow form is exact this round); the fallback reloads
// the 16-bit slice (dir_members_reload: mb, first).
template <int BS, int NPOW, bool NAR>
__device__ int dir_select(const Tables& t, int c, int lenc, DirLDS<BS, NPOW>& L, int d, int part,
                          const uint32_t (&mw)[NAR ? DirGeo<BS, NPOW>::NCW : DirGeo<BS, NPOW>::CW], int& slot,
                          uint2 (&pv)[DirGeo<BS, NPOW>::PREF], int& lo, bool& pb, const uint32_t* mb, bool first) {
  constexpr int H = DirGeo<BS, NPOW>::W / 2;
  constexpr int STEPS = H == 32 ? 5 : H == 16 ? 4 : 3;
  static_assert((1 << STEPS) == H, "window half is a power of two");
  const int SM = t.SM;
  if (lo == INF32 || lo >= lenc) return INF32;
  // bisect over real rows only: the ring's "no row" entries past the chain's end
  // fail every count, which would break the monotonicity the bisection needs
  const int e = min(H - 1, lenc - lo - 1);
  const bool st = kDirStamps && L.s_stamp && threadIdx.x == 0;
  const uint64_t t0 = st ? stamp() : 0;
  int a = 0, b = e;
#pragma unroll
  for (int s = 0; s < STEPS; s++) {
    const int mid = (a + b) >> 1;
    int cnt;
    if constexpr (NAR) cnt = dir_count_n<BS, NPOW>(L, mid, part, mw);
    else cnt = dir_count<BS, NPOW>(L, lo + mid, part, mw);
    if (cnt >= SM) b = mid;
    else a = mid + 1;
  }
  // a == b == T_d, exact below e (e stands for "e or later"); members past N do not count
  if (part == 0 && d < t.N) atomicAdd(&L.sHist[a], 1);
  uint64_t t1 = 0;
  if (st) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    t1 = stamp();
  }
  __syncthreads();
  if (st) {  // HGE_STAMPS: [9] this wave's steps, [10] the wait for the other waves
    L.sdbg[0] += t1 - t0;
    L.sdbg[1] += stamp() - t1;
  }
  // every wave: inclusive prefix over the H bins (DPP, HGE_DPP_SCAN: no LDS
  // permutes on the round's critical path), the first bin reaching SM
  int lane = threadIdx.x & 63;
  asm volatile("" : "+v"(lane));  // (as in dir_stage_member: the bin's address is formed here)
  int v = lane < H ? L.sHist[lane] : 0;
  HGE_DPP_SCAN(v, dpp_add, 0);
  const uint64_t ge = __ballot(lane < H && v >= SM);
  const int ks = ge ? (int)__builtin_ctzll(ge) : H;
  if (ks < e) {
    pb = a <= ks;
    return lo + ks;
  }
  if constexpr (NAR) {
    // The chain ends inside the half window (every call's last rounds: most chains have
    // no next frontier row yet): offset e is its last row and is in the narrow rows, so
    // one narrow probe settles it as dir_probe_search would (that row, or none), without
    // loading the 16-bit slice again.
    if (lenc - lo <= H) {
      bool ps;
      if (dir_probe_n<BS, NPOW>(t, L, e, part, slot++, mw, ps) >= SM) {
        pb = ps;
        return lo + e;
      }
      return INF32;
    }
    uint32_t mx[DirGeo<BS, NPOW>::CW];
    dir_members_reload<BS, NPOW>(t, L, mb, first, d, part, mx);
    return dir_probe_search<BS, NPOW>(t, c, lenc, L, part, mx, slot, pv, lo, pb, e);
  } else {
    return dir_probe_search<BS, NPOW>(t, c, lenc, L, part, mw, slot, pv, lo, pb, e);
  }
}

template <int BS, int NPOW>
__global__ void __launch_bounds__(BS, 4) k_rounds_direct(Tables t, const int32_t* olen, const int32_t* len,
                                                      int32_t* rstate, int rlo, const int32_t* rlo_dev,
                                                      int Rprev, uint64_t* gran,
                                                      int32_t* err, uint64_t* ssc, uint32_t* mbuf,
                                                      uint64_t* dbg, const int32_t* start, int32_t* hist,
                                                      int hmax, const int32_t* stopcut, int extra, int stall_ep,
                                                      int force_exact, int mflag_ep, unsigned long long* paths,
                                                      unsigned long long* paths_next) {
  // History mode (hist != nullptr; a walker of the cross-GPU split, babble_amd/dist.py):
  // the walk starts at the frontier `start` (rlo = 0, Rprev = 0), writes frontier
  // row j to hist[j * N + c] instead of C, the ssc bits of row j to ssc row j, and
  // stops after row hmax - 1 (rstate[1] = 1), `extra` rows after its frontier
  // first reached stopcut on every chain (the next walker's start; rstate[1] = 2),
  // or at the empty frontier; rstate[0] = rows written.
  // stall_ep > 0 (tests, HGE_TEST_HANDOFF_STALL): at hand-off epoch stall_ep chain 0
  // does not publish and every workgroup gives up at once, as on a timed-out poll, so
  // the other chains' rows of that round are written and chain 0's is not.
  // force_exact (tests, HGE_TEST_DIR_EXACT): every round takes the 16-bit select.
  // mflag_ep > 0 (tests, HGE_TEST_DIR_MEMBER_FLAG): at hand-off epoch mflag_ep chain 1
  // raises its staged row's condition-(ii) flag although the row is fine: the round
  // that consumes it takes the 16-bit select on every chain, with the same result.
  // paths[0], paths[1] += this chain's rounds selected over the narrow rows / by the
  // 16-bit select (one add per workgroup, at exit); chain 0 clears paths_next[0..1], the
  // counters of the next walk on the stream.
  using G = DirGeo<BS, NPOW>;
  // rlo_dev: the first round to recompute, read here (INF32: nothing to do)
  if (rlo_dev) {
    rlo = *rlo_dev;
    if (rlo == INF32) {
      if (blockIdx.x == 0 && threadIdx.x == 0 && paths) paths_next[0] = paths_next[1] = 0;
      return;
    }
  }
  // HGE_STAMPS diagnostics (workgroup 0, thread 0): cycles per section into dbg[0..8]
  // (6 = probes; 7, 8 = member-load issue and arrival inside section 0)
  uint64_t st_t = 0, st_acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const bool stamping = kDirStamps && dbg && blockIdx.x == 0 && threadIdx.x == 0;
#define DSTAMP(k)                  \
  if (stamping) {                  \
    const uint64_t now_ = stamp(); \
    st_acc[(k)] += now_ - st_t;    \
    st_t = now_;                   \
  }
#define DSTAMP_START                \
  if (stamping) st_t = stamp();
  __shared__ DirLDS<BS, NPOW> L;
  const int N = t.N, NW = t.NW;
  const int c = blockIdx.x, tid = threadIdx.x;
  const int d = tid / G::TPM, part = tid - d * G::TPM;
  const int lenc = len[c];
  gu64_t* gr[2] = {(gu64_t*)gran, (gu64_t*)(gran + N)};
  uint32_t* mbp[2] = {mbuf, mbuf + (size_t)NPOW * G::MBW};
  // the narrow blocks (NPOW x NPOW bytes each) lie behind the two 16-bit ones
  uint32_t* nbp[2] = {nullptr, nullptr};
  if constexpr (G::NARROW) {
    nbp[0] = mbuf + 2 * (size_t)NPOW * G::MBW;
    nbp[1] = nbp[0] + (size_t)NPOW * NPOW / 4;
  }
  if (tid < N) {
    int P;
    if (hist) {
      P = start[tid];
      if (c == 0) hist[tid] = P;
    } else {
      P = t.C[(size_t)rlo * N + tid];
      if (rlo == 0 && olen[tid] == 0 && len[tid] > 0) P = 0;
      if (c == 0 && rlo == 0 && olen[tid] == 0 && len[tid] > 0) t.C[tid] = 0;
    }
    L.sP[tid] = P;
  }
  if constexpr (G::NARROW) {  // every column's base (columns past N: 0, their member values are unset)
    // (both parities: columns past N are never written again)
    if (tid < NPOW) {
      const uint16_t b = tid < N ? (uint16_t)hge_narrow::nar_base16(L.sP[tid]) : 0;
      ((uint16_t*)L.sB16[0])[dir_base_slot<BS, NPOW>(tid)] = b;
      ((uint16_t*)L.sB16[1])[dir_base_slot<BS, NPOW>(tid)] = b;
    }
  }
  if (tid == 0) {
    L.s_stamp = stamping ? 1 : 0;
    L.sdbg[0] = L.sdbg[1] = 0;
    L.sEx[0] = L.sEx[1] = 0;
    L.sBig = 0;
  }
  __syncthreads();
  if constexpr (G::NARROW) {
    if (tid < N && hge_narrow::nar_base_too_large(L.sP[tid])) {
      L.sEx[rlo & 1] = 1;
      L.sBig = 1;
    }
  }
  int n_nar = 0, n_ex = 0;  // this chain's rounds by select path
  const int rcap = hist ? hmax : t.Rcap;
  int extra_left = -1;  // history mode: rows still to walk after passing stopcut
  uint2 pv[G::PREF];
  int lo = L.sP[c];
  dir_load<BS, NPOW>(t, L, c, lo, DirGeo<BS, NPOW>::W, lenc, pv);
  int f0 = INF32, fn = 0;  // rows fetched for the next round: [f0, f0 + fn)
  // members of the first round from the FD table; later rounds' members are loaded
  // by each wave right after its own poll of the previous round (below).  The narrow
  // widths keep the 8-bit slice nw across the loop and form the 16-bit one only where a
  // rare path needs it; the others keep the 16-bit slice mw.
  uint32_t mw[G::NARROW ? 1 : G::CW];
  uint32_t nw[G::NARROW ? G::NCW : 1];
  // nar: L.sN holds rows [lo, lo + H) encoded against this round's bases (block-uniform)
  bool nar = false;
  if constexpr (G::NARROW) {
    // the first round's base is its own frontier: window and members are encoded here
    __syncthreads();  // the first window is stored
    nar = lo != INF32 && lo < lenc && !force_exact;
    if (nar) {
      uint32_t m16[G::CW];
      dir_members_fd<BS, NPOW>(t, d, part, d < N ? L.sP[d] : INF32, m16);
      if (d >= N) {
#pragma unroll
        for (int k = 0; k < G::CW; k++) m16[k] = 0xFFFFFFFFu;
      }
      const uint32_t mx = dir_encode_window<BS, NPOW>(t, L, L.sB16[rlo & 1], lo);
      const uint32_t mn = dir_encode_members<BS, NPOW>(L.sB16[rlo & 1], part, m16, nw);
      if (hge_narrow::nar_window_flag(mx) || hge_narrow::nar_member_flag(mn)) L.sEx[rlo & 1] = 1;
    }
  } else {
    dir_members_fd<BS, NPOW>(t, d, part, d < N ? L.sP[d] : INF32, mw);
  }
  for (int r = rlo;; r++) {
    if (r + 1 >= rcap) {
      if (c == 0 && tid == 0) {
        rstate[1] = 1;
        if (hist) rstate[0] = r + 1;  // rows written
      }
      break;
    }
    DSTAMP_START
    if constexpr (G::NARROW) {
      if (d >= N) {  // no member: 127 in every field, which no window value reaches
#pragma unroll
        for (int k = 0; k < G::NCW; k++) nw[k] = 0x7F7F7F7Fu;
      }
    } else {
      if (d >= N) {
#pragma unroll
        for (int k = 0; k < G::CW; k++) mw[k] = 0xFFFFFFFFu;
      }
    }
    if (tid < DIR_MAXP) L.sCnt[tid] = 0;
    if (tid < 8) L.sBits[tid] = 0;
    if (tid < DirGeo<BS, NPOW>::W / 2) L.sHist[tid] = 0;
    if (tid == 0) {
      L.sFlag[(r + 1) & 1] = 0;  // read after the previous round's poll barrier
      // (set from this round's first barrier on, read after the next round's first one;
      // round r + 1 encodes against C_r: too large a base there is known since the last
      // poll, and stays)
      L.sEx[(r + 1) & 1] = L.sBig;
    }
    const int Pc = L.sP[c];
    const int cur = (r + 1 < Rprev) ? t.C[(size_t)(r + 1) * N + c] : INF32;
    // The narrow rows of this round were written before the poll barrier (the window by
    // this workgroup after its pick, the member slice by its producers), both against
    // the previous frontier: nothing is encoded here.
    __syncthreads();  // counters clear
    DSTAMP(0);
    int slot = 0;
    int nxt = INF32;
    bool pb = false;
    const bool stall = stall_ep > 0 && r - rlo + 1 == stall_ep;
    // publish C_{r+1}[c]: wave 0 stages the next member row, drains its stores,
    // then lane 0 stores the granule
    auto publish = [&]() {
      DSTAMP(1);
      if (stamping) st_acc[6] += slot;
      if (tid < 64 && !(stall && c == 0)) {
        // (the narrow row against C_r, this round's L.sB16: the next round's base)
        bool mflag = dir_stage_member<BS, NPOW>(t, mbp[(r + 1) & 1], nbp[(r + 1) & 1], L.sB16[r & 1], c, nxt);
        if (mflag_ep > 0 && c == 1 && r - rlo + 1 == mflag_ep) mflag = true;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // both blocks' stores
        if (tid == 0) {
          if (hist) hist[(size_t)(r + 1) * N + c] = nxt;
          else if (nxt != INF32 && cur == INF32) t.C[(size_t)(r + 1) * N + c] = nxt;
          const uint32_t epw = (uint32_t)(r - rlo + 1) | (mflag ? hge_narrow::kNarGranFlag : 0u);
          const uint64_t g = ((uint64_t)epw << 32) | (uint32_t)nxt;
          __hip_atomic_store(gr[(r + 1) & 1] + c, (unsigned long long)g, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    };
    if (Pc == INF32) {
      publish();
    } else if (cur != INF32) {
      // a frontier row kept from an earlier batch: no select, one count for its
      // strongly-see bits
      nxt = cur;
      if constexpr (G::NARROW) {
        // over the narrow rows when the row is among them and the round is unflagged;
        // otherwise over the 16-bit slice, loaded before the publish (dir_members_reload)
        if (nar && L.sEx[r & 1] == 0 && nxt >= lo && nxt - lo < G::H) {  // block-uniform
          publish();
          pb = dir_count_n<BS, NPOW>(L, nxt - lo, part, nw) >= t.SM;
        } else {
          uint32_t m16[G::CW];
          dir_members_reload<BS, NPOW>(t, L, mbp[r & 1], r == rlo, d, part, m16);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the slice is in registers
          __syncthreads();                                  // ... of every wave, before wave 0 publishes
          publish();
          if (nxt < lo || nxt >= lo + DirGeo<BS, NPOW>::W) {
            __syncthreads();
            lo = nxt;
            dir_load<BS, NPOW>(t, L, c, lo, DirGeo<BS, NPOW>::W, lenc, pv);
            __syncthreads();
          }
          pb = dir_count<BS, NPOW>(L, nxt, part, m16) >= t.SM;
        }
      } else {
        publish();
        if (nxt < lo || nxt >= lo + DirGeo<BS, NPOW>::W) {
          __syncthreads();
          lo = nxt;
          dir_load<BS, NPOW>(t, L, c, lo, DirGeo<BS, NPOW>::W, lenc, pv);
          __syncthreads();
        }
        pb = dir_count<BS, NPOW>(L, nxt, part, mw) >= t.SM;
      }
    } else {
      int s;
      if constexpr (G::NARROW) {
        const uint32_t* mbr = mbp[r & 1];
        if (nar && L.sEx[r & 1] == 0) {
          n_nar++;
          s = dir_select<BS, NPOW, true>(t, c, lenc, L, d, part, nw, slot, pv, lo, pb, mbr, r == rlo);
        } else {  // a round whose narrow form is not exact, or the test hook
          n_ex++;
          uint32_t m16[G::CW];
          dir_members_reload<BS, NPOW>(t, L, mbr, r == rlo, d, part, m16);
          s = dir_select<BS, NPOW, false>(t, c, lenc, L, d, part, m16, slot, pv, lo, pb, mbr, r == rlo);
        }
      } else {
        n_ex++;
        s = dir_select<BS, NPOW, false>(t, c, lenc, L, d, part, mw, slot, pv, lo, pb, nullptr, false);
      }
      nxt = s < lenc ? s : INF32;
      publish();
    }
    // strongly-see bits of C_{r+1}[c] against the members of round r
    if (nxt != INF32) {
      if (part == 0 && d < N && pb) atomicOr(&L.sBits[d >> 5], 1u << (d & 31));
      __syncthreads();  // also: every wave is done with this round's window
      if (tid < NW)
        ssc[((size_t)(r + 1) * N + c) * NW + tid] =
            (uint64_t)L.sBits[2 * tid] | ((uint64_t)L.sBits[2 * tid + 1] << 32);
    }
    DSTAMP(2);
    // the rows the next round's window [nxt, nxt + W) lacks, into their ring slots
    // (slots of rows below nxt: no wave reads them again; fn > 0 only if nxt is
    // a row, and then the barrier above has passed)
    if (nxt == INF32) {
      f0 = INF32;
      fn = 0;
    } else {
      f0 = (lo != INF32 && nxt < lo + DirGeo<BS, NPOW>::W) ? lo + DirGeo<BS, NPOW>::W : nxt;
      fn = nxt + DirGeo<BS, NPOW>::W - f0;
    }
    // The next round's narrow window, rows [nxt, nxt + H) against C_r (its base): every
    // wave is done with this round's L.sN since the strongly-see barrier, and the rows
    // are in the ring already unless the window outruns it (rare: then behind the
    // stores and one barrier).  Encoded while the fetch is in flight; sets condition
    // (i)'s flag of the next round.
    bool late = false;
    if constexpr (G::NARROW) {
      nar = nxt != INF32 && !force_exact;
      late = nar && fn > DirGeo<BS, NPOW>::W - G::H;  // nxt + H > (the ring's end) = f0
    }
    lo = nxt;
    dir_fetch<BS, NPOW>(t, c, f0, fn, lenc, pv);
    if constexpr (G::NARROW) {
      if (nar && !late) {
        const uint32_t mx = dir_encode_window<BS, NPOW>(t, L, L.sB16[r & 1], nxt);
        if (hge_narrow::nar_window_flag(mx)) L.sEx[(r + 1) & 1] = 1;
      }
    }
    dir_store<BS, NPOW>(t, L, f0, fn, lenc, pv);
    if (fn > DIR_CH) {  // rare: the LA rows past the first chunk (the FD rows are in flight)
      for (int q = DIR_CH; q < fn; q += DIR_CH) {
        dir_fetch<BS, NPOW>(t, c, f0 + q, fn - q, lenc, pv);
        dir_store<BS, NPOW>(t, L, f0 + q, fn - q, lenc, pv);
      }
    }
    if constexpr (G::NARROW) {
      if (late) {  // block-uniform
        __syncthreads();  // the rows past the old ring are stored
        const uint32_t mx = dir_encode_window<BS, NPOW>(t, L, L.sB16[r & 1], nxt);
        if (hge_narrow::nar_window_flag(mx)) L.sEx[(r + 1) & 1] = 1;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's FD rows have landed
    DSTAMP(3);
    // collect C_{r+1}: every wave polls the granules (epoch r - rlo + 1) of its OWN
    // members and, once they match, loads their staged rows for the next round
    // right away -- the rows of early chains load while the late ones are still
    // being selected (round 2's single polling wave let the whole 128 KB block
    // load only after the slowest chain had published).  Each wave loads only
    // bytes whose flags it polled itself (MI355X_MICROARCH.md, Valid forms, row 1).
    {
      const int tp = dir_tid();
      const int d = tp / G::TPM, part = tp - d * G::TPM;  // (formed here, see dir_tid)
      const unsigned ep = (unsigned)(r - rlo + 1);
      const gu64_t* g = gr[(r + 1) & 1];
      unsigned spins = 0;
      bool fail = false, mflag = false;
      int P = INF32;
      for (;;) {
        bool ok = true;
        if (d < N) {
          const unsigned long long x = __hip_atomic_load(g + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if constexpr (G::NARROW) {  // the epoch word's top bit: the staged row breaks condition (ii)
            ok = ((unsigned)(x >> 32) & ~hge_narrow::kNarGranFlag) == ep;
            mflag = ((unsigned)(x >> 32) & hge_narrow::kNarGranFlag) != 0;
          } else {
            ok = (unsigned)(x >> 32) == ep;
          }
          P = (int)(uint32_t)x;
        }
        if (__all(ok)) break;
        if (stall || ++spins > (1u << 21)) {  // never a normal wait (~2 s): co-residency failure
          fail = true;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (part == 0 && d < N) {
        L.sP[d] = P;
        // (the other parity: waves of this workgroup may still encode against C_r)
        if constexpr (G::NARROW)
          ((uint16_t*)L.sB16[(r + 1) & 1])[dir_base_slot<BS, NPOW>(d)] = (uint16_t)hge_narrow::nar_base16(P);
      }
      if constexpr (G::NARROW) {
        // a member row that breaks condition (ii): the next round selects in 16 bits;
        // a base the narrow form cannot take: every round from the one after it on
        if (__ballot(d < N && mflag) != 0 && (threadIdx.x & 63) == 0) L.sEx[(r + 1) & 1] = 1;
        if (__ballot(part == 0 && d < N && hge_narrow::nar_base_too_large(P)) != 0 && (threadIdx.x & 63) == 0)
          L.sBig = 1;
      }
      const bool any = __ballot(d < N && P != INF32) != 0;
      const bool notpast = stopcut && __ballot(part == 0 && d < N && P < stopcut[d]) != 0;  // INF32 passes
      if ((threadIdx.x & 63) == 0 && (any || notpast || fail))
        atomicOr(&L.sFlag[(r + 1) & 1], (any ? 1 : 0) | (notpast ? 2 : 0) | (fail ? 4 : 0));
      if (fail && (threadIdx.x & 63) == 0) {  // the host falls back to k_round_step32
        atomicOr(err, 1);
        atomicOr(rstate + 1, 4);  // the downstream kernels stand down, as on overflow
      }
      if constexpr (G::NARROW) {
        if (!fail) {
          dir_members_nb<BS, NPOW>(nbp[(r + 1) & 1], nw);
        } else {  // (the walk ends below: no round reads the slice again, so it need not stay in registers)
#pragma unroll
          for (int k = 0; k < G::NCW; k++) nw[k] = 0;
        }
      } else {
        if (!fail) {
          dir_members_mb<BS, NPOW>(mbp[(r + 1) & 1], mw);
        } else {
#pragma unroll
          for (int k = 0; k < G::CW; k++) mw[k] = 0;
        }
      }
    }
    __syncthreads();  // every wave has polled (and stored its window rows)
    DSTAMP(4);
    const int fl = L.sFlag[(r + 1) & 1];
    const int stop = (fl & 4) ? 2 : ((fl & 1) ? 0 : 1);
    if (stop) {
      if (stop == 1 && c == 0 && tid == 0) rstate[0] = hist ? r + 2 : max(rstate[0], r + 1);
      break;
    }
    if (stopcut) {
      if (extra_left < 0 && !(fl & 2)) extra_left = extra;
      if (extra_left >= 0 && extra_left-- == 0) {
        if (c == 0 && tid == 0) {
          rstate[0] = r + 2;  // rows 0 .. r + 1
          rstate[1] = 2;
        }
        break;
      }
    }
  }
  if (tid == 0 && paths) {
    atomicAdd(paths, (unsigned long long)n_nar);
    atomicAdd(paths + 1, (unsigned long long)n_ex);
    if (c == 0) paths_next[0] = paths_next[1] = 0;
  }
  if (stamping) {
    for (int q = 0; q < 9; q++) dbg[q] += st_acc[q];
    dbg[9] += L.sdbg[0];
    dbg[10] += L.sdbg[1];
  }
#undef DSTAMP
#undef DSTAMP_START
}

template __global__ void k_rounds_direct<1024, 64>(Tables, const int32_t*, const int32_t*, int32_t*, int, const int32_t*, int,
    uint64_t*, int32_t*, uint64_t*, uint32_t*, uint64_t*, const int32_t*, int32_t*, int, const int32_t*, int, int, int, int, unsigned long long*, unsigned long long*);
template __global__ void k_rounds_direct<1024, 128>(Tables, const int32_t*, const int32_t*, int32_t*, int, const int32_t*, int,
    uint64_t*, int32_t*, uint64_t*, uint32_t*, uint64_t*, const int32_t*, int32_t*, int, const int32_t*, int, int, int, int, unsigned long long*, unsigned long long*);
template __global__ void k_rounds_direct<1024, 256>(Tables, const int32_t*, const int32_t*, int32_t*, int, const int32_t*, int,
    uint64_t*, int32_t*, uint64_t*, uint32_t*, uint64_t*, const int32_t*, int32_t*, int, const int32_t*, int, int, int, int, unsigned long long*, unsigned long long*);

}  // namespace hge
