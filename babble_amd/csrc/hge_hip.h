// hge_hip.h — the HIP side of hge_own.h: the one check macro, the memory policies behind
// hge::Buf (device memory, pinned host memory) and owners of a stream and an event.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "hge_own.h"

#define HGE_HIPCHK(x)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) throw hge::Error(HGE_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace hge {

struct DeviceMem {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    HGE_HIPCHK(hipMalloc(&p, bytes));
    return p;
  }
  static void free(void* p) { (void)hipFree(p); }
  static void fill(void* p, int byte, size_t bytes, void* stream) {
    HGE_HIPCHK(hipMemsetAsync(p, byte, bytes, (hipStream_t)stream));
  }
  static void copy(void* dst, const void* src, size_t bytes, void* stream) {
    HGE_HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  static void copy2d(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t row_bytes, size_t rows,
                     void* stream) {
    HGE_HIPCHK(hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, row_bytes, rows, hipMemcpyDeviceToDevice,
                                (hipStream_t)stream));
  }
  static void wait(void* stream) { HGE_HIPCHK(hipStreamSynchronize((hipStream_t)stream)); }
};

// pinned host memory: the copies and the wait are the device's (same address space)
struct PinnedMem : DeviceMem {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    HGE_HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    return p;
  }
  static void free(void* p) { (void)hipHostFree(p); }
  // the address the kernels store to (null: not mapped)
  template <class T>
  static T* device_ptr(T* host) {
    void* dp = nullptr;
    return host && hipHostGetDevicePointer(&dp, host, 0) == hipSuccess ? (T*)dp : nullptr;
  }
};

template <class T>
using DBuf = Buf<T, DeviceMem>;
template <class T>
using PBuf = Buf<T, PinnedMem>;

// a stream / an event: created on demand, destroyed with its owner, read as the handle
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  void create() {
    if (!s) HGE_HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  }
  operator hipStream_t() const { return s; }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  void create() {
    if (!e) HGE_HIPCHK(hipEventCreate(&e));
  }
  operator hipEvent_t() const { return e; }
};

}  // namespace hge
