// hge_p256.h — SHA-256 and ECDSA P-256 verification (Event.Verify, hashgraph/event.go:140-150:
// crypto.Verify -> ecdsa.Verify on elliptic.P256(), crypto/utils.go:40-64) as plain functions
// that compile for the host and the device: hge_verify.hip's kernels run them one thread per
// event, tests/abi/hge_p256_test.cpp checks them on the CPU against OpenSSL.  DESIGN.md §4.9.
//
// Numbers are 256-bit, eight 32-bit limbs, least significant first; products are
// (uint64_t)a * b plus adds (one 64-bit multiply-add on the device).  Both moduli, the field
// prime p and the group order n, go through one Montgomery multiplication (CIOS, R = 2^256):
// a field or scalar value "in Montgomery form" is x R mod m.  For p the per-row factor
// -p^-1 mod 2^32 is 1 and five of p's limbs are 0 or 1, which the compiler folds.  Points are
// Jacobian (X, Y, Z) over Montgomery-form coordinates, infinity is Z = 0; an affine point is
// (x, y) in Montgomery form with (0, 0) standing for infinity (it is not on the curve).
//
// Every loop over limbs, bits or windows has a trip count fixed at compile time (inversion
// is the fixed exponentiation x^(m-2)); the one loop whose count is data is SHA-256's over
// the 64-byte blocks of its message.  The inputs are public: nothing here is constant-time.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGE_P256_HD __host__ __device__ __forceinline__
#else
#define HGE_P256_HD inline
#endif
#if defined(__clang__)
#define HGE_P256_UNROLL _Pragma("unroll")
#define HGE_P256_NOUNROLL _Pragma("nounroll")
#elif defined(__GNUC__)
#define HGE_P256_UNROLL _Pragma("GCC unroll 16")
#define HGE_P256_NOUNROLL _Pragma("GCC unroll 1")
#else
#define HGE_P256_UNROLL
#define HGE_P256_NOUNROLL
#endif

namespace hge_p256 {

constexpr int kWindowBits = 4;                    // Shamir's fixed window
constexpr int kTableEntries = 1 << kWindowBits;   // entry d = d Q; entry 0 is never read

struct alignas(16) u256 {  // (aligned so a table entry loads as four-limb vectors)
  uint32_t v[8];
};
struct affine {  // Montgomery form; (0, 0) = infinity
  u256 x, y;
};
struct jac {  // Montgomery form; Z = 0 = infinity
  u256 X, Y, Z;
};

// ---- the moduli ---------------------------------------------------------------------------
// m: the modulus; r2: R^2 mod m (into Montgomery form); one: R mod m; em2: m - 2 (Fermat);
// n0 = -m^-1 mod 2^32
struct ModP {
  static HGE_P256_HD uint32_t m(int i) {
    constexpr uint32_t k[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u,
                               0x00000000u, 0x00000000u, 0x00000001u, 0xFFFFFFFFu};
    return k[i];
  }
  static HGE_P256_HD uint32_t r2(int i) {
    constexpr uint32_t k[8] = {0x00000003u, 0x00000000u, 0xFFFFFFFFu, 0xFFFFFFFBu,
                               0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFDu, 0x00000004u};
    return k[i];
  }
  static HGE_P256_HD uint32_t one(int i) {
    constexpr uint32_t k[8] = {0x00000001u, 0x00000000u, 0x00000000u, 0xFFFFFFFFu,
                               0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu, 0x00000000u};
    return k[i];
  }
  static HGE_P256_HD uint32_t em2(int i) {
    constexpr uint32_t k[8] = {0xFFFFFFFDu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u,
                               0x00000000u, 0x00000000u, 0x00000001u, 0xFFFFFFFFu};
    return k[i];
  }
  static constexpr uint32_t n0 = 0x00000001u;
};
struct ModN {
  static HGE_P256_HD uint32_t m(int i) {
    constexpr uint32_t k[8] = {0xFC632551u, 0xF3B9CAC2u, 0xA7179E84u, 0xBCE6FAADu,
                               0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu};
    return k[i];
  }
  static HGE_P256_HD uint32_t r2(int i) {
    constexpr uint32_t k[8] = {0xBE79EEA2u, 0x83244C95u, 0x49BD6FA6u, 0x4699799Cu,
                               0x2B6BEC59u, 0x2845B239u, 0xF3D95620u, 0x66E12D94u};
    return k[i];
  }
  static HGE_P256_HD uint32_t one(int i) {
    constexpr uint32_t k[8] = {0x039CDAAFu, 0x0C46353Du, 0x58E8617Bu, 0x43190552u,
                               0x00000000u, 0x00000000u, 0xFFFFFFFFu, 0x00000000u};
    return k[i];
  }
  static HGE_P256_HD uint32_t em2(int i) {
    constexpr uint32_t k[8] = {0xFC63254Fu, 0xF3B9CAC2u, 0xA7179E84u, 0xBCE6FAADu,
                               0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu};
    return k[i];
  }
  static constexpr uint32_t n0 = 0xEE00BC4Fu;
};
// the curve's b and the base point, plain (FIPS 186-4 D.1.2.3)
HGE_P256_HD uint32_t curve_b(int i) {
  constexpr uint32_t k[8] = {0x27D2604Bu, 0x3BCE3C3Eu, 0xCC53B0F6u, 0x651D06B0u,
                             0x769886BCu, 0xB3EBBD55u, 0xAA3A93E7u, 0x5AC635D8u};
  return k[i];
}
HGE_P256_HD uint32_t curve_gx(int i) {
  constexpr uint32_t k[8] = {0xD898C296u, 0xF4A13945u, 0x2DEB33A0u, 0x77037D81u,
                             0x63A440F2u, 0xF8BCE6E5u, 0xE12C4247u, 0x6B17D1F2u};
  return k[i];
}
HGE_P256_HD uint32_t curve_gy(int i) {
  constexpr uint32_t k[8] = {0x37BF51F5u, 0xCBB64068u, 0x6B315ECEu, 0x2BCE3357u,
                             0x7C0F9E16u, 0x8EE7EB4Au, 0xFE1A7F9Bu, 0x4FE342E2u};
  return k[i];
}

// ---- 256-bit integers -----------------------------------------------------------------------
HGE_P256_HD u256 u256_zero() {
  u256 r;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) r.v[i] = 0;
  return r;
}
template <class M>
HGE_P256_HD u256 mod_value() {
  u256 r;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) r.v[i] = M::m(i);
  return r;
}
// 32 big-endian bytes
HGE_P256_HD u256 u256_load_be(const uint8_t* b) {
  u256 r;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = b + 4 * (7 - i);
    r.v[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
  }
  return r;
}
HGE_P256_HD void u256_store_be(const u256& a, uint8_t* b) {
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) {
    uint8_t* q = b + 4 * (7 - i);
    q[0] = (uint8_t)(a.v[i] >> 24);
    q[1] = (uint8_t)(a.v[i] >> 16);
    q[2] = (uint8_t)(a.v[i] >> 8);
    q[3] = (uint8_t)a.v[i];
  }
}
HGE_P256_HD bool u256_is_zero(const u256& a) {
  uint32_t o = 0;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) o |= a.v[i];
  return o == 0;
}
HGE_P256_HD bool u256_eq(const u256& a, const u256& b) {
  uint32_t o = 0;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i];
  return o == 0;
}
// r = a + b, returns the carry out
HGE_P256_HD uint32_t u256_add(u256& r, const u256& a, const u256& b) {
  uint64_t c = 0;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a.v[i] + b.v[i];
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)c;
}
// r = a - b, returns the borrow out (1 iff a < b)
HGE_P256_HD uint32_t u256_sub(u256& r, const u256& a, const u256& b) {
  uint64_t br = 0;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)a.v[i] - b.v[i] - br;
    r.v[i] = (uint32_t)d;
    br = (d >> 32) & 1;
  }
  return (uint32_t)br;
}
HGE_P256_HD bool u256_lt(const u256& a, const u256& b) {
  u256 d;
  return u256_sub(d, a, b) != 0;
}
// limb idx by selects: an index the compiler cannot fold must not send the number to memory
HGE_P256_HD uint32_t u256_limb(const u256& a, int idx) {
  uint32_t r = 0;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) r = idx == i ? a.v[i] : r;
  return r;
}
HGE_P256_HD u256 u256_select(bool c, const u256& a, const u256& b) {
  u256 r;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// ---- arithmetic modulo m (M = ModP or ModN) ---------------------------------------------------
// a mod m for any a < 2^256 (2^256 < 2m for both moduli: one subtraction)
template <class M>
HGE_P256_HD u256 mod_reduce(const u256& a) {
  u256 d;
  const uint32_t br = u256_sub(d, a, mod_value<M>());
  return u256_select(br != 0, a, d);
}
template <class M>
HGE_P256_HD u256 mod_add(const u256& a, const u256& b) {  // a, b < m
  u256 s, d;
  const uint32_t c = u256_add(s, a, b);
  const uint32_t br = u256_sub(d, s, mod_value<M>());
  return u256_select(c != 0 || br == 0, d, s);
}
template <class M>
HGE_P256_HD u256 mod_sub(const u256& a, const u256& b) {  // a, b < m
  u256 d, e;
  const uint32_t br = u256_sub(d, a, b);
  u256_add(e, d, mod_value<M>());
  return u256_select(br != 0, e, d);
}
// Montgomery product a b R^-1 mod m (CIOS): a < m or b < m, the other < 2^256; result < m
template <class M>
HGE_P256_HD u256 mont_mul(const u256& a, const u256& b) {
  uint32_t t[10];
  HGE_P256_UNROLL
  for (int i = 0; i < 10; i++) t[i] = 0;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
    HGE_P256_UNROLL
    for (int j = 0; j < 8; j++) {
      const uint64_t acc = (uint64_t)a.v[j] * b.v[i] + t[j] + c;
      t[j] = (uint32_t)acc;
      c = acc >> 32;
    }
    uint64_t acc = (uint64_t)t[8] + c;
    t[8] = (uint32_t)acc;
    t[9] = (uint32_t)(acc >> 32);
    const uint32_t q = t[0] * M::n0;
    acc = (uint64_t)q * M::m(0) + t[0];
    c = acc >> 32;
    HGE_P256_UNROLL
    for (int j = 1; j < 8; j++) {
      acc = (uint64_t)q * M::m(j) + t[j] + c;
      t[j - 1] = (uint32_t)acc;
      c = acc >> 32;
    }
    acc = (uint64_t)t[8] + c;
    t[7] = (uint32_t)acc;
    t[8] = t[9] + (uint32_t)(acc >> 32);
  }
  u256 r, d;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) r.v[i] = t[i];
  const uint32_t br = u256_sub(d, r, mod_value<M>());
  return u256_select(t[8] != 0 || br == 0, d, r);
}
template <class M>
HGE_P256_HD u256 mont_sqr(const u256& a) {
  return mont_mul<M>(a, a);
}
template <class M>
HGE_P256_HD u256 mont_one() {
  u256 r;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) r.v[i] = M::one(i);
  return r;
}
template <class M>
HGE_P256_HD u256 to_mont(const u256& a) {  // a < 2^256
  u256 r2;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) r2.v[i] = M::r2(i);
  return mont_mul<M>(a, r2);
}
template <class M>
HGE_P256_HD u256 from_mont(const u256& a) {
  u256 one = u256_zero();
  one.v[0] = 1;
  return mont_mul<M>(a, one);
}
// a^-1 in Montgomery form (a in Montgomery form, a != 0; 0 gives 0): a^(m-2), 256 squarings
template <class M>
HGE_P256_HD u256 mont_inv(const u256& a) {
  u256 r = mont_one<M>();
  HGE_P256_NOUNROLL
  for (int i = 255; i >= 0; i--) {
    r = mont_sqr<M>(r);
    if ((M::em2(i >> 5) >> (i & 31)) & 1u) r = mont_mul<M>(r, a);
  }
  return r;
}
// plain-value forms (the host test's view of the arithmetic): operands < m
template <class M>
HGE_P256_HD u256 mod_mul(const u256& a, const u256& b) {
  return mont_mul<M>(to_mont<M>(a), b);
}
template <class M>
HGE_P256_HD u256 mod_inv(const u256& a) {
  return from_mont<M>(mont_inv<M>(to_mont<M>(a)));
}

// ---- points (a = -3) ---------------------------------------------------------------------------
typedef ModP Fp;
HGE_P256_HD jac jac_infinity() {
  jac r;
  r.X = mont_one<Fp>();
  r.Y = mont_one<Fp>();
  r.Z = u256_zero();
  return r;
}
HGE_P256_HD bool jac_is_infinity(const jac& p) { return u256_is_zero(p.Z); }
HGE_P256_HD bool affine_is_infinity(const affine& q) { return u256_is_zero(q.x) && u256_is_zero(q.y); }
HGE_P256_HD jac jac_from_affine(const affine& q) {
  jac r;
  r.X = q.x;
  r.Y = q.y;
  r.Z = mont_one<Fp>();
  if (affine_is_infinity(q)) r = jac_infinity();
  return r;
}
// 2P (dbl-2001-b).  Z = 0 gives Z3 = 0; no point of this curve has Y = 0 (the order is odd).
HGE_P256_HD jac jac_double(const jac& p) {
  const u256 delta = mont_sqr<Fp>(p.Z);
  const u256 gamma = mont_sqr<Fp>(p.Y);
  const u256 beta = mont_mul<Fp>(p.X, gamma);
  const u256 t0 = mod_sub<Fp>(p.X, delta);
  const u256 t1 = mod_add<Fp>(p.X, delta);
  const u256 t2 = mont_mul<Fp>(t0, t1);
  const u256 alpha = mod_add<Fp>(mod_add<Fp>(t2, t2), t2);
  const u256 beta2 = mod_add<Fp>(beta, beta);
  const u256 beta4 = mod_add<Fp>(beta2, beta2);
  const u256 beta8 = mod_add<Fp>(beta4, beta4);
  jac r;
  r.X = mod_sub<Fp>(mont_sqr<Fp>(alpha), beta8);
  const u256 yz = mod_add<Fp>(p.Y, p.Z);
  r.Z = mod_sub<Fp>(mod_sub<Fp>(mont_sqr<Fp>(yz), gamma), delta);
  const u256 g2 = mont_sqr<Fp>(gamma);
  const u256 g2_2 = mod_add<Fp>(g2, g2);
  const u256 g2_4 = mod_add<Fp>(g2_2, g2_2);
  const u256 g2_8 = mod_add<Fp>(g2_4, g2_4);
  r.Y = mod_sub<Fp>(mont_mul<Fp>(alpha, mod_sub<Fp>(beta4, r.X)), g2_8);
  return r;
}
// the tail shared by both adds: H = U2 - U1 != 0, Rr = S2 - S1, result Z3 = zh H
HGE_P256_HD jac jac_add_tail(const u256& U1, const u256& S1, const u256& H, const u256& Rr, const u256& zh) {
  const u256 HH = mont_sqr<Fp>(H);
  const u256 HHH = mont_mul<Fp>(H, HH);
  const u256 V = mont_mul<Fp>(U1, HH);
  jac r;
  r.X = mod_sub<Fp>(mod_sub<Fp>(mont_sqr<Fp>(Rr), HHH), mod_add<Fp>(V, V));
  r.Y = mod_sub<Fp>(mont_mul<Fp>(Rr, mod_sub<Fp>(V, r.X)), mont_mul<Fp>(S1, HHH));
  r.Z = mont_mul<Fp>(zh, H);
  return r;
}
// P + Q, Q affine: infinity on either side, P = Q (the doubling) and P = -Q (infinity) included
HGE_P256_HD jac jac_madd(const jac& p, const affine& q) {
  if (affine_is_infinity(q)) return p;
  if (jac_is_infinity(p)) return jac_from_affine(q);
  const u256 zz = mont_sqr<Fp>(p.Z);
  const u256 U2 = mont_mul<Fp>(q.x, zz);
  const u256 S2 = mont_mul<Fp>(q.y, mont_mul<Fp>(p.Z, zz));
  const u256 H = mod_sub<Fp>(U2, p.X);
  const u256 Rr = mod_sub<Fp>(S2, p.Y);
  if (u256_is_zero(H)) return u256_is_zero(Rr) ? jac_double(p) : jac_infinity();
  return jac_add_tail(p.X, p.Y, H, Rr, p.Z);
}
// P + Q, both Jacobian, the same cases included
HGE_P256_HD jac jac_add(const jac& p, const jac& q) {
  if (jac_is_infinity(p)) return q;
  if (jac_is_infinity(q)) return p;
  const u256 z1z1 = mont_sqr<Fp>(p.Z), z2z2 = mont_sqr<Fp>(q.Z);
  const u256 U1 = mont_mul<Fp>(p.X, z2z2), U2 = mont_mul<Fp>(q.X, z1z1);
  const u256 S1 = mont_mul<Fp>(p.Y, mont_mul<Fp>(q.Z, z2z2));
  const u256 S2 = mont_mul<Fp>(q.Y, mont_mul<Fp>(p.Z, z1z1));
  const u256 H = mod_sub<Fp>(U2, U1);
  const u256 Rr = mod_sub<Fp>(S2, S1);
  if (u256_is_zero(H)) return u256_is_zero(Rr) ? jac_double(p) : jac_infinity();
  return jac_add_tail(U1, S1, H, Rr, mont_mul<Fp>(p.Z, q.Z));
}
// the affine form (one field inversion); infinity gives (0, 0)
HGE_P256_HD affine jac_to_affine(const jac& p) {
  affine r;
  r.x = u256_zero();
  r.y = u256_zero();
  if (jac_is_infinity(p)) return r;
  const u256 zi = mont_inv<Fp>(p.Z);
  const u256 zi2 = mont_sqr<Fp>(zi);
  r.x = mont_mul<Fp>(p.X, zi2);
  r.y = mont_mul<Fp>(p.Y, mont_mul<Fp>(zi, zi2));
  return r;
}
HGE_P256_HD bool affine_on_curve(const affine& q) {  // y^2 = x^3 - 3x + b
  u256 b;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) b.v[i] = curve_b(i);
  const u256 bm = to_mont<Fp>(b);
  const u256 x2 = mont_sqr<Fp>(q.x);
  const u256 x3 = mont_mul<Fp>(x2, q.x);
  const u256 x_3 = mod_add<Fp>(mod_add<Fp>(q.x, q.x), q.x);
  const u256 rhs = mod_add<Fp>(mod_sub<Fp>(x3, x_3), bm);
  return u256_eq(mont_sqr<Fp>(q.y), rhs);
}
HGE_P256_HD affine p256_generator() {
  u256 x, y;
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) {
    x.v[i] = curve_gx(i);
    y.v[i] = curve_gy(i);
  }
  affine g;
  g.x = to_mont<Fp>(x);
  g.y = to_mont<Fp>(y);
  return g;
}

// elliptic.Unmarshal (crypto.ToECDSAPub, crypto/utils.go:40-46): 0x04 || X || Y, both below p,
// the point on the curve; anything else is no key
HGE_P256_HD bool p256_key_decode(const uint8_t* pub, affine& out) {
  out.x = u256_zero();
  out.y = u256_zero();
  if (pub[0] != 0x04) return false;
  const u256 x = u256_load_be(pub + 1), y = u256_load_be(pub + 33);
  const u256 p = mod_value<Fp>();
  if (!u256_lt(x, p) || !u256_lt(y, p)) return false;
  affine q;
  q.x = to_mont<Fp>(x);
  q.y = to_mont<Fp>(y);
  if (!affine_on_curve(q)) return false;
  out = q;
  return true;
}

// the window table of Q: tab[d] = d Q for d in [1, 2^w), tab[0] = infinity (never read by the
// ladder).  2Q comes out of the mixed add's doubling case.
HGE_P256_HD void p256_window_table(const affine& q, affine* tab) {
  tab[0].x = u256_zero();
  tab[0].y = u256_zero();
  tab[1] = q;
  jac acc = jac_from_affine(q);
  HGE_P256_NOUNROLL
  for (int d = 2; d < kTableEntries; d++) {
    acc = jac_madd(acc, q);
    tab[d] = jac_to_affine(acc);
  }
}

// u1 G + u2 Q by interleaved fixed windows (Shamir): 64 rounds of four doublings and up to
// two mixed adds; a zero digit skips its add.  u1, u2 plain scalars.
HGE_P256_HD jac p256_shamir(const u256& u1, const u256& u2, const affine* gtab, const affine* qtab) {
  jac r = jac_infinity();
  HGE_P256_NOUNROLL
  for (int i = 256 / kWindowBits - 1; i >= 0; i--) {
    HGE_P256_NOUNROLL
    for (int k = 0; k < kWindowBits; k++) r = jac_double(r);
    const int limb = (i * kWindowBits) >> 5, sh = (i * kWindowBits) & 31;
    HGE_P256_NOUNROLL
    for (int t = 0; t < 2; t++) {
      const uint32_t d = (u256_limb(t == 0 ? u1 : u2, limb) >> sh) & (uint32_t)(kTableEntries - 1);
      if (d != 0) r = jac_madd(r, (t == 0 ? gtab : qtab)[d]);
    }
  }
  return r;
}

// ecdsa.Verify (crypto.Verify, crypto/utils.go:60-64) over the two window tables: sig = r || s
// big-endian, digest = the 32-byte hash (no truncation on P-256).  1 iff valid.
HGE_P256_HD int p256_ecdsa_verify_tables(const uint8_t* digest, const affine* gtab, const affine* qtab,
                                         const uint8_t* sig) {
  const u256 r = u256_load_be(sig), s = u256_load_be(sig + 32);
  const u256 n = mod_value<ModN>();
  if (u256_is_zero(r) || u256_is_zero(s) || !u256_lt(r, n) || !u256_lt(s, n)) return 0;
  const u256 e = mod_reduce<ModN>(u256_load_be(digest));
  const u256 w = mont_inv<ModN>(to_mont<ModN>(s));  // s^-1 R
  const u256 u1 = mont_mul<ModN>(e, w);             // e s^-1, plain
  const u256 u2 = mont_mul<ModN>(r, w);
  const jac R = p256_shamir(u1, u2, gtab, qtab);
  if (jac_is_infinity(R)) return 0;
  // R.x mod n == r without the inversion: X = x Z^2 with x = r, or x = r + n when that is < p
  const u256 zz = mont_sqr<Fp>(R.Z);
  if (u256_eq(R.X, mont_mul<Fp>(to_mont<Fp>(r), zz))) return 1;
  u256 rn;
  const uint32_t carry = u256_add(rn, r, n);
  if (carry == 0 && u256_lt(rn, mod_value<Fp>()) && u256_eq(R.X, mont_mul<Fp>(to_mont<Fp>(rn), zz))) return 1;
  return 0;
}
// the same from the key point alone: builds both tables (the host test's entry; a caller with
// many signatures per key builds the tables once)
HGE_P256_HD int p256_ecdsa_verify_digest(const uint8_t* digest, const affine& key, const uint8_t* sig) {
  affine gtab[kTableEntries], qtab[kTableEntries];
  p256_window_table(p256_generator(), gtab);
  p256_window_table(key, qtab);
  return p256_ecdsa_verify_tables(digest, gtab, qtab, sig);
}

// ---- SHA-256 (FIPS 180-4) ------------------------------------------------------------------------
HGE_P256_HD uint32_t sha256_k(int i) {
  constexpr uint32_t k[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  return k[i];
}
HGE_P256_HD uint32_t sha256_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
// byte i of the padded message: the data, 0x80, zeros, the bit length in the last 8 bytes
HGE_P256_HD uint32_t sha256_padded_byte(const uint8_t* data, uint64_t len, uint64_t total, uint64_t i) {
  if (i < len) return data[i];
  if (i == len) return 0x80u;
  if (i + 8 < total) return 0u;
  return (uint32_t)(((len << 3) >> (8 * (total - 1 - i))) & 0xFFu);
}
HGE_P256_HD void sha256(const uint8_t* data, uint64_t len, uint8_t* out) {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  const uint64_t total = ((len + 9 + 63) >> 6) << 6;
  for (uint64_t base = 0; base < total; base += 64) {
    uint32_t w[16];
    if (base + 64 <= len) {
      HGE_P256_UNROLL
      for (int i = 0; i < 16; i++) {
        const uint8_t* q = data + base + 4 * i;
        w[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
      }
    } else {
      HGE_P256_UNROLL
      for (int i = 0; i < 16; i++) {
        const uint64_t o = base + 4 * i;
        w[i] = (sha256_padded_byte(data, len, total, o) << 24) | (sha256_padded_byte(data, len, total, o + 1) << 16) |
               (sha256_padded_byte(data, len, total, o + 2) << 8) | sha256_padded_byte(data, len, total, o + 3);
      }
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    HGE_P256_UNROLL
    for (int i = 0; i < 64; i++) {
      if (i >= 16) {
        const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
        const uint32_t s0 = sha256_rotr(w15, 7) ^ sha256_rotr(w15, 18) ^ (w15 >> 3);
        const uint32_t s1 = sha256_rotr(w2, 17) ^ sha256_rotr(w2, 19) ^ (w2 >> 10);
        w[i & 15] += s0 + w[(i + 9) & 15] + s1;
      }
      const uint32_t S1 = sha256_rotr(e, 6) ^ sha256_rotr(e, 11) ^ sha256_rotr(e, 25);
      const uint32_t ch = (e & f) ^ (~e & g);
      const uint32_t t1 = hh + S1 + ch + sha256_k(i) + w[i & 15];
      const uint32_t S0 = sha256_rotr(a, 2) ^ sha256_rotr(a, 13) ^ sha256_rotr(a, 22);
      const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
      const uint32_t t2 = S0 + mj;
      hh = g;
      g = f;
      f = e;
      e = d + t1;
      d = c;
      c = b;
      b = a;
      a = t1 + t2;
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
    h[5] += f;
    h[6] += g;
    h[7] += hh;
  }
  HGE_P256_UNROLL
  for (int i = 0; i < 8; i++) {
    out[4 * i] = (uint8_t)(h[i] >> 24);
    out[4 * i + 1] = (uint8_t)(h[i] >> 16);
    out[4 * i + 2] = (uint8_t)(h[i] >> 8);
    out[4 * i + 3] = (uint8_t)h[i];
  }
}

}  // namespace hge_p256
