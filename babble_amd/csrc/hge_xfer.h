// hge_xfer.h — host <-> device staging through pinned memory, on one stream.
//
// A copy from pageable memory makes the runtime wait for the stream, so every
// small control upload would be a hidden round trip.  Control data goes through
// a pinned arena instead: uploads are enqueued without waiting, downloads are
// queued and land in their host destinations at the next sync(), which also
// recycles the arena (everything enqueued before it has completed).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "hge_hip.h"

namespace hge {

// where an online call's host time goes (HGE_HOST_PHASES=1: printed at destroy):
// calls, launches, copies, ns spent inside hipStreamSynchronize, ns in the calls
struct HostPhases {
  int64_t calls = 0, launches = 0, copies = 0, wait_ns = 0, call_ns = 0, insert_ns = 0;
};

inline int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Xfer {
  const Stream& st;
  HostPhases& hp;
  PBuf<char> pin;
  size_t pin_used = 0;
  struct Pending {
    void* dst;
    size_t off, bytes;
  };
  std::vector<Pending> pending;
  int64_t n_syncs = 0;  // host waits on the stream (hge_host_syncs)
  Xfer(const Stream& s, HostPhases& h) : st(s), hp(h) {}

  // 256-byte pieces; a full arena is drained first (sync) and regrown only when the one
  // piece does not fit an empty arena
  char* pin_take(size_t bytes) {
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (pin_used + need > pin.n) {
      sync();
      if (need > pin.n) pin.need(std::max<size_t>(need, std::max<size_t>(2 * pin.n, 1 << 16)));
    }
    char* q = pin.p + pin_used;
    pin_used += need;
    return q;
  }
  // room for pieces of `bytes` in all (each rounded up by its caller) without a drain
  // between them: an idle arena is regrown as it is, a used one is drained first
  void reserve(size_t bytes) {
    if (pin_used + bytes <= pin.n) return;
    if (pin_used || !pending.empty()) sync();
    if (bytes > pin.n) pin.need(std::max<size_t>(bytes, std::max<size_t>(2 * pin.n, 1 << 16)));
  }
  void h2d(void* dev, const void* host, size_t bytes) {
    if (!bytes) return;
    char* q = pin_take(bytes);
    memcpy(q, host, bytes);
    hp.copies++;
    HGE_HIPCHK(hipMemcpyAsync(dev, q, bytes, hipMemcpyHostToDevice, st));
  }
  void d2h(void* host, const void* dev, size_t bytes) {
    if (!bytes) return;
    char* q = pin_take(bytes);
    hp.copies++;
    HGE_HIPCHK(hipMemcpyAsync(q, dev, bytes, hipMemcpyDeviceToHost, st));
    pending.push_back({host, (size_t)(q - pin.p), bytes});
  }
  // download into the arena itself: the returned offset stays readable after the
  // next sync() until the arena is used again (no second host copy)
  size_t d2h_pinned(const void* dev, size_t bytes) {
    char* q = pin_take(bytes);
    if (bytes) hp.copies++;
    if (bytes) HGE_HIPCHK(hipMemcpyAsync(q, dev, bytes, hipMemcpyDeviceToHost, st));
    return (size_t)(q - pin.p);
  }
  const char* at(size_t off) const { return pin.p + off; }
  void sync() {
    n_syncs++;
    const int64_t w0 = now_ns();
    HGE_HIPCHK(hipStreamSynchronize(st));
    hp.wait_ns += now_ns() - w0;
    for (const Pending& pd : pending) memcpy(pd.dst, pin.p + pd.off, pd.bytes);
    pending.clear();
    pin_used = 0;
  }
  template <typename F>
  void readback(F* host, const F* dev, size_t n) {
    d2h(host, dev, n * sizeof(F));
    sync();
  }
};

}  // namespace hge
