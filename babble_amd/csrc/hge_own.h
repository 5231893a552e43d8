// hge_own.h — who frees what on the host side of the device back-ends (hge_engine.hip,
// hge_batch.hip, hge_verify.hip): one error type and one owning,
// move-only buffer.  Host only and free of HIP: the memory behind a buffer is a policy
// class (hge_hip.h has the real ones), so tests/abi/hge_own_test.cpp checks every rule
// below on the CPU with a policy that counts blocks.
//
// A policy Mem gives, all static; a failure throws hge::Error, `stream` is opaque:
//   void* alloc(size_t bytes)          void free(void* p)
//   void fill(void* p, int byte, size_t bytes, void* stream)
//   void copy(void* dst, const void* src, size_t bytes, void* stream)
//   void copy2d(void* dst, size_t dst_pitch, const void* src, size_t src_pitch,
//               size_t row_bytes, size_t rows, void* stream)
//   void wait(void* stream)
#pragma once

#include <stddef.h>

#include <algorithm>
#include <string>
#include <utility>

#include "../../include/hge.h"

namespace hge {

struct Error {
  int code;
  std::string msg;
  Error(int c, std::string m = {}) : code(c), msg(std::move(m)) {}
};

template <class T, class Mem>
struct Buf {
  T* p = nullptr;
  size_t n = 0;  // capacity in elements (the regrown chain tables: what their caller states)

  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(o.p), n(o.n) {
    o.p = nullptr;
    o.n = 0;
  }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      free_();
      p = o.p;
      n = o.n;
      o.p = nullptr;
      o.n = 0;
    }
    return *this;
  }
  ~Buf() { free_(); }
  void swap(Buf& o) noexcept {
    std::swap(p, o.p);
    std::swap(n, o.n);
  }
  friend void swap(Buf& a, Buf& b) noexcept { a.swap(b); }
  // take over a block that something else filled (a kernel: to_wide32)
  void adopt(Buf&& o) noexcept { *this = std::move(o); }

  // grow without preserving contents; a failed allocation leaves the buffer empty
  void need(size_t m) {
    if (m <= n) return;
    free_();
    const size_t cap = std::max<size_t>(m, 64);
    p = (T*)Mem::alloc(cap * sizeof(T));
    n = cap;
  }
  // grow preserving contents [0, keep); the new block is filled first where asked
  void grow_keep(size_t m, size_t keep, void* stream, int fill_byte = -1) {
    if (m <= n) return;
    const size_t cap = std::max<size_t>(m, n + n / 2);
    Buf q;
    q.p = (T*)Mem::alloc(cap * sizeof(T));
    q.n = cap;
    if (fill_byte >= 0) Mem::fill(q.p, fill_byte, cap * sizeof(T), stream);
    if (p && keep) Mem::copy(q.p, p, keep * sizeof(T), stream);
    Mem::wait(stream);
    *this = std::move(q);
  }
  // A table of `rows` rows regrown at a longer row: a new block of total_bytes, filled
  // where asked; the old rows (old_row_bytes each) copied to the heads of the new ones
  // (new_row_bytes apart) when keep is set and there is an old block; then the old block
  // is freed and the buffer holds the new one as n_after elements.  The caller states the
  // byte geometry: some tables hold uint16 rows behind an int32 element type.
  void regrow_rows(size_t rows, size_t old_row_bytes, size_t new_row_bytes, size_t total_bytes, size_t n_after,
                   bool keep, void* stream, int fill_byte = -1) {
    Buf q;
    q.p = (T*)Mem::alloc(total_bytes);
    q.n = n_after;
    if (fill_byte >= 0) Mem::fill(q.p, fill_byte, total_bytes, stream);
    if (keep && p) Mem::copy2d(q.p, new_row_bytes, p, old_row_bytes, old_row_bytes, rows, stream);
    Mem::wait(stream);
    *this = std::move(q);
  }
  // (a throw above unwinds through q, which frees the new block: the old one stays owned)

 private:
  void free_() {
    if (p) Mem::free(p);
    p = nullptr;
    n = 0;
  }
};

}  // namespace hge
