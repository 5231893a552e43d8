// hge_hostlog.h — the host's record of one event stream: the FromParentsLatest admission
// check (O(1) per event over per-creator chain tails, hashgraph.go:366-396), the accepted
// events' fields as arrays, and the packed records a small batch is uploaded as.  Plain
// C++ with no device in it (tests/abi/hge_hostlog_test.cpp drives it on the CPU).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/hge.h"

namespace hge {

// A small batch's event fields uploaded as one packed record per event (one copy
// instead of eight; hge_engine.hip upload()), unpacked by k_chain_fill.
struct UpEv {
  int32_t creator, index, sp, op, ntx, coin;
  int64_t ts;
  uint64_t S[4];
};

struct HostLog {
  int N = 0;
  std::vector<int32_t> h_creator, h_index, h_sp, h_op, h_ntx;
  std::vector<int64_t> h_ts;
  std::vector<uint64_t> h_S;
  std::vector<uint8_t> h_coin;
  std::vector<int32_t> chain_len, chain_last;
  std::vector<std::vector<int32_t>> h_chain;  // participantEventsCache: ids per creator
  int64_t n_events = 0;                       // accepted
  // the longest chain admit() passes without asking (kAtLimit): the engine's uint16 wide
  // path ends there, and the engine lifts it when it goes on with int32 positions
  int32_t chain_limit = INT32_MAX;

  HostLog() = default;
  HostLog(int n, int32_t limit)
      : N(n), chain_len(n, 0), chain_last(n, -1), h_chain(n), chain_limit(limit) {}

  // admit()'s answer beside the hge_status codes: the event is fine but its chain has
  // chain_limit events already.  The caller decides (lift the limit and admit, or refuse
  // with capacity_error()).
  static constexpr int kAtLimit = 1;
  int admit(const hge_event& e, int32_t sp, int32_t op, std::string& err) const {
    const int c = e.creator;
    if (c < 0 || c >= N) {
      err = "Could not find fake creator id";
      return HGE_ERR_CREATOR;
    }
    const int known = chain_len[c];
    if (sp == HGE_NONE && op == HGE_NONE && known == 0) {
      if (e.index != 0) {
        err = "Event index does not match the creator's chain position";
        return HGE_ERR_INDEX;
      }
      return HGE_OK;
    }
    if (sp < 0 || sp >= n_events) {
      err = "Self-parent not known";
      return HGE_ERR_SELF_PARENT_UNKNOWN;
    }
    if (h_creator[sp] != c) {
      err = "Self-parent has different creator";
      return HGE_ERR_SELF_PARENT_CREATOR;
    }
    if (op < 0 || op >= n_events) {
      err = "Other-parent not known";
      return HGE_ERR_OTHER_PARENT_UNKNOWN;
    }
    if (sp != chain_last[c]) {
      err = "Self-parent not last known event by creator";
      return HGE_ERR_SELF_PARENT_NOT_LAST;
    }
    if (e.index != known) {
      err = "Event index does not match the creator's chain position";
      return HGE_ERR_INDEX;
    }
    return known >= chain_limit ? kAtLimit : HGE_OK;
  }
  int capacity_error(std::string& err) const {
    err = "Chain capacity exceeded: at most " + std::to_string(chain_limit) + " events per creator";
    return HGE_ERR_CAPACITY;
  }

  void append(const hge_event& e, int32_t sp, int32_t op) {
    const int64_t id = n_events++;
    h_creator.push_back(e.creator);
    h_index.push_back(e.index);
    h_sp.push_back(sp);
    h_op.push_back(op);
    h_ntx.push_back(e.n_tx);
    h_ts.push_back(e.timestamp_ns);
    for (int k = 0; k < 4; k++) {
      uint64_t v = 0;
      for (int b = 0; b < 8; b++) v = (v << 8) | e.s[8 * k + b];
      h_S.push_back(v);
    }
    h_coin.push_back(e.hash[16] != 0 ? 1 : 0);
    h_chain[e.creator].push_back((int32_t)id);
    chain_len[e.creator]++;
    chain_last[e.creator] = (int32_t)id;
  }

  int max_chain() const {
    int m = 0;
    for (int c = 0; c < N; c++) m = m > chain_len[c] ? m : chain_len[c];
    return m;
  }

  // the packed upload records of the events [a, a + m)
  std::vector<UpEv> pack(int64_t a, int64_t m) const {
    std::vector<UpEv> up((size_t)m);
    for (int64_t i = 0; i < m; i++) {
      UpEv& r = up[(size_t)i];
      const size_t x = (size_t)(a + i);
      r.creator = h_creator[x];
      r.index = h_index[x];
      r.sp = h_sp[x];
      r.op = h_op[x];
      r.ntx = h_ntx[x];
      r.coin = h_coin[x];
      r.ts = h_ts[x];
      for (int k = 0; k < 4; k++) r.S[k] = h_S[4 * x + k];
    }
    return up;
  }
};

}  // namespace hge
