// hge_hooks.h — every environment hook of the engine (hge_engine.hip), one named
// function each.  A hook's comment says what it forces and when it is read: "at create"
// (once, in a member initialiser of the engine) or "per use" (every time the code path
// runs: the tests flip those on a live engine).  DESIGN.md §State and lifetimes has the
// same list as a table.
#pragma once

#include <algorithm>
#include <cstdlib>

namespace hge_hooks {

inline bool is_set(const char* name) { return getenv(name) != nullptr; }
// the hook's number, or `unset` without it
inline int num(const char* name, int unset) {
  const char* v = getenv(name);
  return v ? atoi(v) : unset;
}
inline bool nonzero(const char* name) { return num(name, 0) != 0; }

// HGE_CHAIN_LIMIT=k: lowers the longest chain of the uint16 wide path from `limit` to k (tests: the switch to int32 positions comes early).  At create.
inline int chain_limit(int limit) { return is_set("HGE_CHAIN_LIMIT") ? std::max(1, std::min(limit, num("HGE_CHAIN_LIMIT", 0))) : limit; }
// HGE_TEST_W32_FAIL=k: to_wide32 fails once after its stage k.  At create.
inline int test_w32_fail() { return num("HGE_TEST_W32_FAIL", 0); }
// HGE_TEST_MEDIAN_ROWS_FALLBACK: the median takes k_median_wave although the coordinate step skipped the timestamps.  At create.
inline bool test_median_rows_fallback() { return is_set("HGE_TEST_MEDIAN_ROWS_FALLBACK"); }
// HGE_STAMPS: per-section cycle counters of some kernels, dumped on stderr.  At create.
inline bool stamps() { return is_set("HGE_STAMPS"); }
// HGE_HOST_PHASES: where the host time goes, one line on stderr.  At destroy, and per batch of more than 1,000 calls.
inline bool host_phases() { return is_set("HGE_HOST_PHASES"); }

// HGE_WALKERS=k: walkers of the speculative walk at N <= 32 (0 or 1: sequential); < 0: unset.  Per use: the tests vary it on one engine.
inline int walkers() { return num("HGE_WALKERS", -1); }
// HGE_COOP_WALKERS=k: the same for the wide walk; unset: `dflt`.  Per use: the tests vary it.
inline int coop_walkers(int dflt) { return num("HGE_COOP_WALKERS", dflt); }
// HGE_WALK_HCAP=k: k (at least 2) rows per walker's history in place of `rows` (tests: the capacity fallback).  Per use.
inline int walk_hcap(int rows) { return is_set("HGE_WALK_HCAP") ? std::max(2, num("HGE_WALK_HCAP", 0)) : rows; }
// HGE_WALK_DEBUG: per-walker rows, merge results and cycle stamps on stderr.  Per use.
inline bool walk_debug() { return is_set("HGE_WALK_DEBUG"); }
// HGE_LW_G=k: k (at least 1) windows in the windowed lastAncestors pass in place of `windows`.  Per use.
inline long long lw_windows(long long windows) { return is_set("HGE_LW_G") ? std::max(1, num("HGE_LW_G", 0)) : windows; }
// HGE_NO_LASEQ: no one-pass lastAncestors kernel (the sweeps instead).  Per use.
inline bool no_laseq() { return is_set("HGE_NO_LASEQ"); }
// HGE_NO_FD_DIRECT: k_la_seq does not write the batch's firstDescendants at N <= 16.  Per use.
inline bool no_fd_direct() { return is_set("HGE_NO_FD_DIRECT"); }
// HGE_NO_ONLINE_FAST: no one-round-trip online call at N <= 16.  Per use.
inline bool no_online_fast() { return is_set("HGE_NO_ONLINE_FAST"); }
// HGE_NO_ORDER_CALL: the order's stages as their own grids, never one block.  Per use (per batch, the online hot path).
inline bool no_order_call() { return is_set("HGE_NO_ORDER_CALL"); }
// HGE_SEG_DEBUG: the segments theta walks, one line per batch on stderr.  Per use.
inline bool seg_debug() { return is_set("HGE_SEG_DEBUG"); }
// HGE_TEST_DIR_EXACT=1: every round of the direct walk takes the 16-bit select.  Per use.
inline int test_dir_exact() { return nonzero("HGE_TEST_DIR_EXACT") ? 1 : 0; }
// HGE_TEST_DIR_MEMBER_FLAG=e: at hand-off epoch e chain 1 flags its staged member row.  Per use.
inline int test_dir_member_flag() { return num("HGE_TEST_DIR_MEMBER_FLAG", 0); }
// HGE_TEST_HANDOFF_STALL=e: the walk stalls at hand-off epoch e.  Per use.
inline int test_handoff_stall() { return num("HGE_TEST_HANDOFF_STALL", 0); }
// HGE_TEST_HANDOFF_FAIL: the walk reports a hand-off timeout.  Per use.
inline bool test_handoff_fail() { return is_set("HGE_TEST_HANDOFF_FAIL"); }
// HGE_TEST_SORT_INDEX=1: every bucket of the order stage takes the index sort.  Per use.
inline int test_sort_index() { return nonzero("HGE_TEST_SORT_INDEX") ? 1 : 0; }
// HGE_TEST_RECORDS_CHUNK=k: hge_commit_records works in chunks of k (at least 1, at most `chunk`) records (tests: several chunks at test sizes).  Per use.
inline long long test_records_chunk(long long chunk) { return is_set("HGE_TEST_RECORDS_CHUNK") ? std::max<long long>(1, std::min<long long>(chunk, num("HGE_TEST_RECORDS_CHUNK", 0))) : chunk; }

}  // namespace hge_hooks
