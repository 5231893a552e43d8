// hge_verify.hip — Event.Verify on the device: SHA-256 of the event bodies
// (EventBody.Hash, hashgraph/event.go:60-66) and ECDSA P-256 verification of the signatures
// over those hashes (Event.Verify, event.go:140-150 -> crypto.Verify -> ecdsa.Verify,
// crypto/utils.go:60-64), one thread per event, with the arithmetic of hge_p256.h.
//
// The opt-in counterpart of hge_ingest.cpp's host pipeline, which stays the default and the
// reference.  Three kernels, none of which talks to another workgroup:
//   k_sha256_bodies       one thread per body, hashes to HBM;
//   k_p256_key_tables     one thread per distinct key: elliptic.Unmarshal's checks
//                         (crypto.ToECDSAPub, crypto/utils.go:40-46), then the key's window
//                         table 1Q .. 15Q in affine Montgomery form and a valid flag;
//   k_ecdsa_p256_verify   one thread per event: Shamir's interleaved 4-bit windows over G's
//                         table (computed once on the host with the same header) and the
//                         key's table, both read from HBM through L2.
// Every entry point is synchronous, owns its buffers and its stream, and works through the
// events in chunks of at most 2^20 so device memory stays bounded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/hge.h"
#include "hge_hip.h"
#include "hge_p256.h"

namespace {

using namespace hge_p256;

constexpr int64_t kChunkEvents = 1 << 20;
constexpr int kShaThreads = 256;
constexpr int kVerifyThreads = 64;  // one wave per workgroup: the register budget of a lone wave

__global__ __launch_bounds__(kShaThreads) void k_sha256_bodies(int64_t n, const uint8_t* __restrict__ data,
                                                                const int64_t* __restrict__ off, int64_t base,
                                                                uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kShaThreads + threadIdx.x;
  if (i >= n) return;
  uint8_t h[32];
  sha256(data + (off[i] - base), (uint64_t)(off[i + 1] - off[i]), h);
  uint32_t* o = reinterpret_cast<uint32_t*>(out + 32 * i);
#pragma unroll
  for (int w = 0; w < 8; w++)
    o[w] = (uint32_t)h[4 * w] | ((uint32_t)h[4 * w + 1] << 8) | ((uint32_t)h[4 * w + 2] << 16) |
           ((uint32_t)h[4 * w + 3] << 24);
}

__global__ __launch_bounds__(kVerifyThreads) void k_p256_key_tables(int32_t n_keys, const uint8_t* __restrict__ keys,
                                                                    affine* __restrict__ tabs,
                                                                    int32_t* __restrict__ valid) {
  const int32_t k = (int32_t)(blockIdx.x * kVerifyThreads + threadIdx.x);
  if (k >= n_keys) return;
  affine q;
  const bool ok = p256_key_decode(keys + 65 * (size_t)k, q);
  affine* tab = tabs + (size_t)kTableEntries * k;
  if (ok) {
    p256_window_table(q, tab);
  } else {
    for (int d = 0; d < kTableEntries; d++) tab[d] = q;  // (0, 0): never read, the flag stops the event
  }
  valid[k] = ok ? 1 : 0;
}

__global__ __launch_bounds__(kVerifyThreads) void k_ecdsa_p256_verify(
    int64_t n, const uint8_t* __restrict__ digests, const int32_t* __restrict__ key_idx,
    const uint8_t* __restrict__ sigs, const affine* __restrict__ gtab, const affine* __restrict__ qtabs,
    const int32_t* __restrict__ valid, int32_t* __restrict__ ok) {
  const int64_t i = (int64_t)blockIdx.x * kVerifyThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t k = key_idx[i];  // in [0, n_keys): checked on the host before the launch
  int v = 0;
  if (valid[k]) v = p256_ecdsa_verify_tables(digests + 32 * i, gtab, qtabs + (size_t)kTableEntries * k, sigs + 64 * i);
  ok[i] = v;
}

using hge::DBuf;
using hge::Error;

// G's window table, once per process, by the code the device runs for the keys
const affine* generator_table() {
  static affine tab[kTableEntries];
  static std::once_flag once;
  std::call_once(once, [] { p256_window_table(p256_generator(), tab); });
  return tab;
}

// one device, one stream, the buffers of one chunk
class Verifier {
 public:
  explicit Verifier(int device) {
    if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
    HGE_HIPCHK(hipSetDevice(device));
    s_.create();
    e0_.create();
    e1_.create();
  }
  ~Verifier() {
    if (prev_ >= 0) (void)hipSetDevice(prev_);
  }
  double device_ms() const { return ms_; }

  void set_keys(const uint8_t* keys, int32_t n_keys) {
    keys_.need(65 * (size_t)n_keys);
    tabs_.need((size_t)kTableEntries * n_keys);
    valid_.need(n_keys);
    gtab_.need(kTableEntries);
    HGE_HIPCHK(hipMemcpyAsync(keys_.p, keys, 65 * (size_t)n_keys, hipMemcpyHostToDevice, s_));
    HGE_HIPCHK(hipMemcpyAsync(gtab_.p, generator_table(), sizeof(affine) * kTableEntries, hipMemcpyHostToDevice, s_));
    HGE_HIPCHK(hipEventRecord(e0_, s_));
    k_p256_key_tables<<<(n_keys + kVerifyThreads - 1) / kVerifyThreads, kVerifyThreads, 0, s_>>>(n_keys, keys_.p,
                                                                                                tabs_.p, valid_.p);
    HGE_HIPCHK(hipGetLastError());
    HGE_HIPCHK(hipEventRecord(e1_, s_));
    finish();
  }

  // SHA-256 of n strings; out on the host
  void hash(int64_t n, const uint8_t* data, const int64_t* off, uint8_t* out) {
    for (int64_t lo = 0; lo < n; lo += kChunkEvents) {
      const int64_t m = std::min(kChunkEvents, n - lo);
      upload_bodies(m, data, off + lo);
      HGE_HIPCHK(hipEventRecord(e0_, s_));
      launch_sha(m, off[lo]);
      HGE_HIPCHK(hipEventRecord(e1_, s_));
      HGE_HIPCHK(hipMemcpyAsync(out + 32 * lo, dig_.p, 32 * (size_t)m, hipMemcpyDeviceToHost, s_));
      finish();
    }
  }
  // signatures over given digests (set_keys first; key_idx checked by the caller)
  void verify_digests(int64_t n, const uint8_t* digests, const int32_t* key_idx, const uint8_t* sigs,
                      int32_t* ok_out) {
    for (int64_t lo = 0; lo < n; lo += kChunkEvents) {
      const int64_t m = std::min(kChunkEvents, n - lo);
      dig_.need(32 * (size_t)m);
      HGE_HIPCHK(hipMemcpyAsync(dig_.p, digests + 32 * lo, 32 * (size_t)m, hipMemcpyHostToDevice, s_));
      upload_sigs(m, key_idx + lo, sigs + 64 * lo);
      HGE_HIPCHK(hipEventRecord(e0_, s_));
      launch_verify(m);
      HGE_HIPCHK(hipEventRecord(e1_, s_));
      HGE_HIPCHK(hipMemcpyAsync(ok_out + lo, ok_.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, s_));
      finish();
    }
  }
  // Event.Verify: hash, then the signature over the hash
  void verify_events(int64_t n, const uint8_t* bodies, const int64_t* off, const int32_t* key_idx,
                     const uint8_t* sigs, uint8_t* hash_out, int32_t* ok_out) {
    for (int64_t lo = 0; lo < n; lo += kChunkEvents) {
      const int64_t m = std::min(kChunkEvents, n - lo);
      upload_bodies(m, bodies, off + lo);
      upload_sigs(m, key_idx + lo, sigs + 64 * lo);
      HGE_HIPCHK(hipEventRecord(e0_, s_));
      launch_sha(m, off[lo]);
      launch_verify(m);
      HGE_HIPCHK(hipEventRecord(e1_, s_));
      if (hash_out) HGE_HIPCHK(hipMemcpyAsync(hash_out + 32 * lo, dig_.p, 32 * (size_t)m, hipMemcpyDeviceToHost, s_));
      HGE_HIPCHK(hipMemcpyAsync(ok_out + lo, ok_.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, s_));
      finish();
    }
  }

 private:
  // the chunk's bytes data[off[0] .. off[m]) and its m + 1 offsets
  void upload_bodies(int64_t m, const uint8_t* data, const int64_t* off) {
    const size_t bytes = (size_t)(off[m] - off[0]);
    data_.need(bytes);
    off_.need((size_t)m + 1);
    dig_.need(32 * (size_t)m);
    if (bytes) HGE_HIPCHK(hipMemcpyAsync(data_.p, data + off[0], bytes, hipMemcpyHostToDevice, s_));
    HGE_HIPCHK(hipMemcpyAsync(off_.p, off, sizeof(int64_t) * ((size_t)m + 1), hipMemcpyHostToDevice, s_));
  }
  void upload_sigs(int64_t m, const int32_t* key_idx, const uint8_t* sigs) {
    kidx_.need(m);
    sigs_.need(64 * (size_t)m);
    ok_.need(m);
    HGE_HIPCHK(hipMemcpyAsync(kidx_.p, key_idx, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, s_));
    HGE_HIPCHK(hipMemcpyAsync(sigs_.p, sigs, 64 * (size_t)m, hipMemcpyHostToDevice, s_));
  }
  void launch_sha(int64_t m, int64_t base) {
    k_sha256_bodies<<<(unsigned)((m + kShaThreads - 1) / kShaThreads), kShaThreads, 0, s_>>>(m, data_.p, off_.p, base,
                                                                                              dig_.p);
    HGE_HIPCHK(hipGetLastError());
  }
  void launch_verify(int64_t m) {
    k_ecdsa_p256_verify<<<(unsigned)((m + kVerifyThreads - 1) / kVerifyThreads), kVerifyThreads, 0, s_>>>(
        m, dig_.p, kidx_.p, sigs_.p, gtab_.p, tabs_.p, valid_.p, ok_.p);
    HGE_HIPCHK(hipGetLastError());
  }
  // wait for the chunk (the host buffers are the caller's: nothing may be in flight on return)
  void finish() {
    HGE_HIPCHK(hipStreamSynchronize(s_));
    float ms = 0;
    HGE_HIPCHK(hipEventElapsedTime(&ms, e0_, e1_));
    ms_ += ms;
  }

  int prev_ = -1;
  hge::Stream s_;  // before the buffers: destroyed after them
  hge::Event e0_, e1_;
  double ms_ = 0;
  DBuf<uint8_t> keys_, data_, dig_, sigs_;
  DBuf<affine> tabs_, gtab_;
  DBuf<int32_t> valid_, kidx_, ok_;
  DBuf<int64_t> off_;
};

bool offsets_ascend(int64_t n, const int64_t* off) {
  if (off[0] < 0) return false;
  for (int64_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return false;
  return true;
}
bool key_idx_in_range(int64_t n, const int32_t* key_idx, int32_t n_keys) {
  for (int64_t i = 0; i < n; i++)
    if (key_idx[i] < 0 || key_idx[i] >= n_keys) return false;
  return true;
}

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const Error& e) {
    return e.code;
  } catch (const std::bad_alloc&) {
    return HGE_ERR_INTERNAL;
  }
}

}  // namespace

extern "C" {

int hge_sha256_batch_device(int64_t n, const uint8_t* data, const int64_t* off, int32_t device, uint8_t* out) {
  if (n < 0 || device < 0 || (n > 0 && (!data || !off || !out))) return HGE_ERR_ARG;
  if (n == 0) return HGE_OK;
  if (!offsets_ascend(n, off)) return HGE_ERR_ARG;
  return guarded([&] {
    Verifier v(device);
    v.hash(n, data, off, out);
    return (int)HGE_OK;
  });
}

int hge_ecdsa_p256_verify_digests_device(int64_t n, const uint8_t* digests, const uint8_t* keys, int32_t n_keys,
                                         const int32_t* key_idx, const uint8_t* sigs, int32_t device,
                                         int32_t* ok_out) {
  if (n < 0 || device < 0 || n_keys < 0 || (n > 0 && (!digests || !keys || !key_idx || !sigs || !ok_out)))
    return HGE_ERR_ARG;
  if (n == 0) return HGE_OK;
  if (!key_idx_in_range(n, key_idx, n_keys)) return HGE_ERR_ARG;
  return guarded([&] {
    Verifier v(device);
    v.set_keys(keys, n_keys);
    v.verify_digests(n, digests, key_idx, sigs, ok_out);
    return (int)HGE_OK;
  });
}

int hge_verify_events_device(int64_t n, const uint8_t* bodies, const int64_t* body_off, const uint8_t* keys,
                             int32_t n_keys, const int32_t* key_idx, const uint8_t* sigs, int32_t device,
                             uint8_t* body_hash_out, int32_t* ok_out, double* device_ms) {
  if (device_ms) *device_ms = 0;
  if (n < 0 || device < 0 || n_keys < 0 || (n > 0 && (!bodies || !body_off || !keys || !key_idx || !sigs || !ok_out)))
    return HGE_ERR_ARG;
  if (n == 0) return HGE_OK;
  if (!offsets_ascend(n, body_off) || !key_idx_in_range(n, key_idx, n_keys)) return HGE_ERR_ARG;
  return guarded([&] {
    Verifier v(device);
    v.set_keys(keys, n_keys);
    v.verify_events(n, bodies, body_off, key_idx, sigs, body_hash_out, ok_out);
    if (device_ms) *device_ms = v.device_ms();
    return (int)HGE_OK;
  });
}

int hge_ingest_device(hge_engine* h, const hge_event* ev, int64_t n, const uint8_t* bodies, const int64_t* body_off,
                      const uint8_t* keys, const uint8_t* sigs, int64_t k, int64_t verify_block,
                      int32_t* status_out, int64_t* n_accepted, double* times_out) {
  if (!h || n < 0 || k <= 0 || (n > 0 && (!ev || !bodies || !body_off || !keys || !sigs))) return HGE_ERR_ARG;
  if (n > 0 && !offsets_ascend(n, body_off)) return HGE_ERR_ARG;
  if (n_accepted) *n_accepted = 0;
  const int32_t N = hge_participants(h);
  int64_t vb = verify_block <= 0 ? 65536 : verify_block;
  vb = (vb + k - 1) / k * k;  // a block is whole batches
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  double verify_ms = 0, device_ms = 0;
  int64_t acc = 0;
  const int rc = guarded([&] {
    int rc = HGE_OK;
    if (n == 0) return rc;
    Verifier v(hge_device(h));
    const auto tk = clk::now();
    v.set_keys(keys, N);
    verify_ms += std::chrono::duration<double, std::milli>(clk::now() - tk).count();
    const int64_t span = std::min(vb, n);
    std::vector<int32_t> kidx(span), ok(span);
    for (int64_t b0 = 0; b0 < n && rc == HGE_OK; b0 += vb) {
      const int64_t b1 = std::min(n, b0 + vb);
      // the whole block's signatures, to completion, before its first event is inserted: the
      // verify kernels never share the device with the consensus kernels
      const auto tv = clk::now();
      for (int64_t e = b0; e < b1; e++) {
        const int32_t c = ev[e].creator;
        kidx[e - b0] = (c < 0 || c >= N) ? 0 : c;
      }
      v.verify_events(b1 - b0, bodies, body_off + b0, kidx.data(), sigs + 64 * b0, nullptr, ok.data());
      // no key for this id: let admission refuse it ("Could not find fake creator id")
      for (int64_t e = b0; e < b1; e++)
        if (ev[e].creator < 0 || ev[e].creator >= N) ok[e - b0] = 1;
      verify_ms += std::chrono::duration<double, std::milli>(clk::now() - tv).count();
      for (int64_t lo = b0; lo < b1 && rc == HGE_OK; lo += k) {
        const int64_t hi = std::min(b1, lo + k);
        int64_t m = lo;
        while (m < hi && ok[m - b0]) m++;  // InsertEvent stops at the first invalid signature
        const auto td = clk::now();
        int64_t got = 0;
        if (m > lo) rc = hge_insert_events(h, ev + lo, m - lo, status_out ? status_out + lo : nullptr, &got);
        acc += got;
        if (rc == HGE_OK) rc = hge_run_consensus(h, nullptr, 0, nullptr);
        device_ms += std::chrono::duration<double, std::milli>(clk::now() - td).count();
        if (rc == HGE_OK && m < hi) {
          if (status_out) status_out[m] = HGE_ERR_SIGNATURE;
          rc = HGE_ERR_SIGNATURE;
        }
      }
    }
    return rc;
  });
  if (n_accepted) *n_accepted = acc;
  if (times_out) {
    times_out[0] = verify_ms;  // the device verify blocks, copies included: none of it is hidden
    times_out[1] = device_ms;  // insert + consensus calls
    times_out[2] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  }
  return rc;
}

}  // extern "C"
