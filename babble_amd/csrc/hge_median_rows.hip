// hge_median_rows.hip — the wide median of a fresh bulk replay, taken from the FD rows
// themselves.  Included by hge_engine.hip after hge_kernels.hip.
//
// k_median_wave reads a row of timestamp offsets FDTD[x][.] that k_fd_transpose_ts wrote
// for it: at 256/10M that table is 10 GB written and 10 GB read back once.  Here a
// workgroup holds the FD16 rows of TQ consecutive positions of one chain in LDS, gathers
// the timestamps with lanes running along the positions (FD is non-decreasing along a
// chain: a wave touches a few lines of tsch per chain j, the transpose's pattern) and
// selects on the spot.  The table is never written (k_fd_rows16 writes the FD rows alone).
#pragma once

namespace hge {

// One workgroup per (chain c, TQ consecutive positions from q0); the candidate list is
// the identity (candidate = event id), so recv_call / rr_in / bseg are indexed by the
// event at (c, q).  len[c]: the chain's length.  Results as k_median_wave<4>'s, by the
// same two selects over the same values.
// LDS: the packed rows (TQ x (N + 2) halves), then in their place the offsets
// (TQ x (N + 4) ints: every thread holds its FD values in registers across the switch).
template <int TQ, int NT>
__global__ void __launch_bounds__(NT) k_median_rows(Tables t, const int32_t* len, const int32_t* recv_call,
                                                    const int32_t* rr_in, const int32_t* bseg,
                                                    const uint64_t* seg_fws, int64_t* cts_out) {
  constexpr int NWV = NT / 64;          // waves
  constexpr int RPW = TQ / NWV;         // rows per wave
  constexpr int PER = 256 * TQ / NT;    // (position, chain) cells per thread at N = 256
  constexpr int LDP = 256 * TQ / 4 / NT;  // 8-byte row pieces per thread at N = 256
  static_assert(TQ % NWV == 0 && RPW <= 8 && (256 * TQ) % (4 * NT) == 0 && NT % TQ == 0, "tile shape");
  extern __shared__ __attribute__((aligned(16))) int32_t s_tile[];  // TQ * (N + 4) ints
  __shared__ __attribute__((aligned(16))) int s_mhist[NWV][256];    // each wave's select bins
  __shared__ int64_t s_own[TQ];
  __shared__ int s_x[TQ], s_rr[TQ], s_sg[TQ], s_wide[TQ];
  const int N = t.N, NW = t.NW;
  const size_t ccap = t.ccap;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // consecutive workgroups take the same positions of neighbouring chains (their first
  // descendants lie in the same stretch of every chain j), dealt to the XCDs in
  // contiguous ranges as in k_fd_transpose_ts
  const int64_t lb = xcd_block(blockIdx.x, gridDim.x);
  const int c = (int)(lb % N), q0 = (int)(lb / N) * TQ;
  const int pend = len[c];
  if (q0 >= pend) return;
  const int rows = min(TQ, pend - q0);
  const int RS16 = N + 2;  // halves per staged row: an odd number of words
  const int RS32 = N + 4;  // ints per offsets row: 16-byte aligned rows
  // the tile of FD16 rows is contiguous: 8-byte pieces (N % 4 == 0: none straddles a row)
  const uint16_t* src = t.FD16 + rowoff(t, c, q0);
  const int npiece = rows * (N >> 2);
  uint2 pw[LDP];
#pragma unroll
  for (int i = 0; i < LDP; i++) {
    const int p = tid + NT * i;
    pw[i] = p < npiece ? *(const uint2*)(src + 4 * (size_t)p) : make_uint2(~0u, ~0u);
  }
  // the positions' events
  int lv = 0;
  if (tid < TQ) {
    const int q = q0 + tid;
    int x = 0, rr = 0, sg = 0;
    int64_t own = 0;
    if (q < pend) {
      x = t.chain[(size_t)c * ccap + q];
      own = t.tsch[(size_t)c * ccap + q];
      // (all three in flight together; an event not received keeps row 0 and segment 0)
      const int rc = recv_call[x], rr0 = rr_in[x], sg0 = bseg[x];
      lv = rc >= 0;
      rr = lv ? rr0 : 0;
      sg = lv ? sg0 : 0;
    }
    s_x[tid] = lv ? x : -1;
    s_rr[tid] = rr;
    s_sg[tid] = sg;
    s_own[tid] = own;
    s_wide[tid] = 0;
  }
  uint16_t* const t16 = (uint16_t*)s_tile;
#pragma unroll
  for (int i = 0; i < LDP; i++) {
    const int p = tid + NT * i;
    if (p < npiece) {
      const int e = 4 * p, q = e / N, j = e - q * N;
      uint32_t* d = (uint32_t*)(t16 + q * RS16 + j);  // (RS16 and j are even)
      d[0] = pw[i].x;
      d[1] = pw[i].y;
    }
  }
  if (!__syncthreads_or(lv)) return;  // no position of the tile was received
  // this wave's rows: thresholds and fame words, in flight across the gather below
  const int l4 = min(lane, (N >> 2) - 1);
  // (WLA16: LA + 1 as uint16, N > 192; else the int32 rows)
  int th[RPW][4];
  uint32_t fw[RPW];  // the fame bits of the lane's 4 witnesses
#pragma unroll
  for (int k = 0; k < RPW; k++) {
    const int r = wv + NWV * k;
    const bool on = s_x[r] >= 0;
    const size_t o = ((size_t)(on ? s_rr[r] : 0) * N + c) * N + 4 * l4;
    if (t.WLA16) {
      const uint2 tw = *(const uint2*)(t.WLA16 + o);
      th[k][0] = (int)(tw.x & 0xFFFFu) - 1;
      th[k][1] = (int)(tw.x >> 16) - 1;
      th[k][2] = (int)(tw.y & 0xFFFFu) - 1;
      th[k][3] = (int)(tw.y >> 16) - 1;
    } else {
      const int4 tw = *(const int4*)(t.WLA + o);
      th[k][0] = tw.x;
      th[k][1] = tw.y;
      th[k][2] = tw.z;
      th[k][3] = tw.w;
    }
    // (lanes past N / 4 are masked)
    fw[k] = (uint32_t)(seg_fws[(size_t)(on ? s_sg[r] : 0) * NW + min(lane >> 4, NW - 1)] >> ((4 * lane) & 63)) & 15u;
  }
  // lanes along the positions for a fixed chain j: cell i of the thread is
  // (q, j) = (idx % TQ, idx / TQ), idx = tid + NT i
  int kv[PER];
#pragma unroll
  for (int i = 0; i < PER; i++) {
    const int idx = tid + NT * i, q = idx % TQ, j = idx / TQ;
    const uint32_t v = (j < N && q < rows) ? t16[q * RS16 + j] : 0xFFFFu;
    kv[i] = v == 0xFFFFu ? INF32 : (int)v - 1;
  }
  __syncthreads();  // the rows are in registers: the offsets take their place
  constexpr int GB = PER < 8 ? PER : 8;  // gathers in flight per thread
#pragma unroll
  for (int h = 0; h < PER; h += GB) {
    int64_t tv[GB];
#pragma unroll
    for (int i = 0; i < GB; i++) {
      const int j = (tid + NT * (h + i)) / TQ;
      tv[i] = kv[h + i] != INF32 ? t.tsch[(size_t)(j < N ? j : 0) * ccap + kv[h + i]] : 0;
    }
#pragma unroll
    for (int i = 0; i < GB; i++) {
      const int idx = tid + NT * (h + i), q = idx % TQ, j = idx / TQ;
      if (j < N) {
        const int64_t dlt = tv[i] - s_own[q];
        const bool esc = kv[h + i] != INF32 && (dlt < -(int64_t)INT32_MAX || dlt > (int64_t)INT32_MAX);
        s_tile[q * RS32 + j] = kv[h + i] == INF32 ? 0 : (int32_t)dlt;
        if (esc) s_wide[q] = 1;  // an offset outside int32: the row gathers exact timestamps
      }
    }
  }
  // which of the lane's witnesses count, 4 bits per row: famous, and seeing the row's event
  uint32_t inm = 0;
#pragma unroll
  for (int k = 0; k < RPW; k++) {
    const int ix = q0 + wv + NWV * k;
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (4 * lane + e < N && ((fw[k] >> e) & 1u) && th[k][e] >= ix) inm |= 1u << (4 * k + e);
  }
  __syncthreads();
  // one wave per row: lane l takes the witnesses d = 4l .. 4l + 3
#pragma unroll
  for (int k = 0; k < RPW; k++) {
    const int r = wv + NWV * k;
    const int x = __builtin_amdgcn_readfirstlane(s_x[r]);
    if (x < 0) continue;  // not received (or past the chain)
    const int ix = q0 + r;
    const int4 ow = *(const int4*)(s_tile + r * RS32 + 4 * l4);
    const int32_t o4[4] = {ow.x, ow.y, ow.z, ow.w};
    bool in[4];
#pragma unroll
    for (int e = 0; e < 4; e++) in[e] = (inm >> (4 * k + e)) & 1u;
    int64_t med;
    if (!__builtin_amdgcn_readfirstlane(s_wide[r])) {
      // int32 offsets: the median of (base + o) is base + the median of o
      uint32_t v[4];
#pragma unroll
      for (int e = 0; e < 4; e++) v[e] = in[e] ? ((uint32_t)o4[e] ^ 0x80000000u) : ~0u;
      med = s_own[r] + (int64_t)(int32_t)(wave_upper_median32_r8<4>(v, in, s_mhist[wv]) ^ 0x80000000u);
    } else {
      const size_t rw = (size_t)c * ccap + ix;
      uint64_t v[4];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int dd = min(4 * lane + e, N - 1);
        const int f = fd_at(t, rw, dd);
        const int64_t ts = f != INF32 ? t.tsch[(size_t)dd * ccap + f] : 0;
        v[e] = in[e] ? ((uint64_t)ts ^ 0x8000000000000000ull) : ~0ull;
      }
      med = wave_upper_median<4>(v, in);
    }
    if (lane == 0) cts_out[x] = med;
  }
}

// The lowest chain position of a still-undetermined event, per chain: lo[c] (set to the
// chain's length beforehand) takes the minimum over the undetermined list, whose count
// the device holds (the batch's results header).
__global__ void k_und_low(const int32_t* creator, const int32_t* index, const int32_t* und, const int32_t* n_und,
                          int32_t* lo) {
  const int n = *n_und;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int x = und[i];
    atomicMin(&lo[creator[x]], index[x]);
  }
}

}  // namespace hge
