// hge_launch.h — how the engine launches and times its kernels: the per-kernel HIP-event
// profiler (hge_set_profiling, hge_kernel_stats) and the launch macros over it.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "hge_hip.h"

namespace hge {

// per-kernel HIP-event timing on one stream: begin / end around a launch record a pair of
// events, collect() (after the step, one wait) adds the pairs up under the launches' names
struct KernelProf {
  const Stream& st;
  bool on = false;
  std::vector<Event> pool;
  std::vector<std::pair<std::string, int>> rec;  // this step's launches: name, first event's slot
  std::vector<std::string> names;                // totals, in order of first appearance
  std::vector<double> ms;
  std::vector<int64_t> cnt;
  explicit KernelProf(const Stream& s) : st(s) {}

  void begin(const char* name) {
    if (!on) return;
    const int slot = (int)rec.size() * 2;
    while ((int)pool.size() < slot + 2) {
      pool.emplace_back();
      pool.back().create();
    }
    HGE_HIPCHK(hipEventRecord(pool[slot], st));
    rec.push_back({name, slot});
  }
  void end() {
    if (!on) return;
    HGE_HIPCHK(hipEventRecord(pool[rec.back().second + 1], st));
  }
  void collect() {
    if (rec.empty()) return;
    HGE_HIPCHK(hipStreamSynchronize(st));
    for (auto& r : rec) {
      float t = 0;
      HGE_HIPCHK(hipEventElapsedTime(&t, pool[r.second], pool[r.second + 1]));
      size_t k = 0;
      while (k < names.size() && names[k] != r.first) k++;
      if (k == names.size()) {
        names.push_back(r.first);
        ms.push_back(0);
        cnt.push_back(0);
      }
      ms[k] += t;
      cnt[k] += 1;
    }
    rec.clear();
  }
  void clear_stats() {
    names.clear();
    ms.clear();
    cnt.clear();
  }
};

}  // namespace hge

// every launch is checked: a launch the runtime refuses (e.g. too much LDS)
// must fail the call, never leave a table silently unwritten
// KLAUNCH_ON: the launch counted in `counter` and timed by `prof` (a KernelProf) under `name`
#define KLAUNCH_ON(prof, counter, name, kern, ...)                                     \
  do {                                                                                 \
    (counter)++;                                                                       \
    (prof).begin(name);                                                                \
    hipLaunchKernelGGL(kern, __VA_ARGS__);                                             \
    const hipError_t le_ = hipGetLastError();                                          \
    if (le_ != hipSuccess)                                                             \
      throw hge::Error(HGE_ERR_DEVICE, std::string("launch ") + name + ": " + hipGetErrorString(le_)); \
    (prof).end();                                                                      \
  } while (0)
// the engine's own launches: its profiler and its launch counter (hge_engine members)
// KLAUNCH_AS: a kernel pointer chosen at run time (WalkKernels) under its instantiation's name
#define KLAUNCH_AS(name, kern, ...) KLAUNCH_ON(this->prof, this->hp.launches, name, kern, __VA_ARGS__)
#define KLAUNCH(kern, ...) KLAUNCH_AS(#kern, kern, __VA_ARGS__)

// Run-time NW (1..4) -> template argument, the one place that does it:
//   KLAUNCH_NW(NW, SHAPE, kernel, [template arguments around the width,] launch arguments...)
// SHAPE says where the width goes and whether the name is parenthesised, so that each
// case hands KLAUNCH the kernel with the number in place and hge_kernel_stats keeps
// reporting "k_median_wave<4>" and "(k_fame_call<64, 4, false>)" (bench.py reads them).
// KLAUNCH_NW2: N > 64 only (no <1> instance of the kernel exists).
#define NW_T(B, kern, ...) KLAUNCH(kern<B>, __VA_ARGS__)
#define NW_PT(B, kern, ...) KLAUNCH((kern<B>), __VA_ARGS__)
#define NW_PAT(B, kern, A, ...) KLAUNCH((kern<A, B>), __VA_ARGS__)
#define NW_PATC(B, kern, A, C, ...) KLAUNCH((kern<A, B, C>), __VA_ARGS__)
#define NW_SWITCH_(nw, CASE1, SHAPE, ...)                          \
  switch (nw) {                                                    \
    CASE1                                                          \
    case 2:                                                        \
      SHAPE(2, __VA_ARGS__);                                       \
      break;                                                       \
    case 3:                                                        \
      SHAPE(3, __VA_ARGS__);                                       \
      break;                                                       \
    case 4:                                                        \
      SHAPE(4, __VA_ARGS__);                                       \
      break;                                                       \
    default:                                                       \
      throw hge::Error(HGE_ERR_INTERNAL, "unsupported N");         \
  }
#define KLAUNCH_NW(nw, SHAPE, ...) NW_SWITCH_(nw, case 1 : SHAPE(1, __VA_ARGS__); break;, SHAPE, __VA_ARGS__)
#define KLAUNCH_NW2(nw, SHAPE, ...) NW_SWITCH_(nw, , SHAPE, __VA_ARGS__)
