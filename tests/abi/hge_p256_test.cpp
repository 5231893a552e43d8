// hge_p256.h (the arithmetic hge_verify.hip's kernels run) against OpenSSL on the CPU:
// field and scalar arithmetic, point arithmetic with its exceptional cases, the windowed
// double-scalar multiplication, key decoding, ECDSA verification and SHA-256.
// Host only; links libcrypto and nothing of the engine.  Prints "ok <checks>".
#include <openssl/bn.h>
#include <openssl/ec.h>
#include <openssl/ecdsa.h>
#include <openssl/obj_mac.h>
#include <openssl/sha.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../babble_amd/csrc/hge_p256.h"

using namespace hge_p256;

static long g_checks = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);         \
      exit(1);                                                    \
    }                                                             \
    g_checks++;                                                   \
  } while (0)

static std::mt19937_64 rng(20240611);
static BN_CTX* ctx;
static EC_GROUP* grp;
static BIGNUM *bn_p, *bn_n;

static u256 rand256() {
  u256 r;
  for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)rng();
  return r;
}
static BIGNUM* to_bn(const u256& a) {
  uint8_t b[32];
  u256_store_be(a, b);
  return BN_bin2bn(b, 32, nullptr);
}
static u256 from_bn(const BIGNUM* a) {
  uint8_t b[32];
  if (BN_bn2binpad(a, b, 32) != 32) {
    printf("FAIL: BIGNUM wider than 256 bits\n");
    exit(1);
  }
  return u256_load_be(b);
}
static u256 small(uint32_t x) {
  u256 r = u256_zero();
  r.v[0] = x;
  return r;
}

// ---- field and scalar arithmetic -----------------------------------------------------------
template <class M>
static void test_mod(const BIGNUM* m) {
  const u256 mv = mod_value<M>();
  CHECK(u256_eq(mv, from_bn(m)));
  std::vector<u256> ops;
  u256 t;
  ops.push_back(u256_zero());
  ops.push_back(small(1));
  ops.push_back(small(2));
  u256_sub(t, mv, small(1));
  ops.push_back(t);  // m - 1
  u256_sub(t, mv, small(2));
  ops.push_back(t);
  ops.push_back(mod_reduce<M>(from_bn(bn_p)));  // p mod m (0 for p) ...
  u256_sub(t, from_bn(bn_p), small(1));
  ops.push_back(mod_reduce<M>(t));  // p - 1
  u256_sub(t, from_bn(bn_n), small(1));
  ops.push_back(mod_reduce<M>(t));  // n - 1
  u256 ones;
  for (int i = 0; i < 8; i++) ones.v[i] = 0xFFFFFFFFu;
  ops.push_back(mod_reduce<M>(ones));  // every limb 0xFFFFFFFF, reduced
  for (int i = 0; i < 8; i++) {        // one set limb: carries
    u256 a = u256_zero();
    a.v[i] = 0xFFFFFFFFu;
    ops.push_back(mod_reduce<M>(a));
    a.v[i] = 1u;
    ops.push_back(mod_reduce<M>(a));
    a.v[i] = 0x80000000u;
    ops.push_back(mod_reduce<M>(a));
  }
  const size_t n_special = ops.size();
  for (int i = 0; i < 300; i++) ops.push_back(mod_reduce<M>(rand256()));
  // mod_reduce itself
  for (const u256& a : ops) CHECK(u256_lt(a, mv));
  BIGNUM* r = BN_new();
  auto pair = [&](const u256& a, const u256& b) {
    BIGNUM *ba = to_bn(a), *bb = to_bn(b);
    BN_mod_mul(r, ba, bb, m, ctx);
    CHECK(u256_eq(mod_mul<M>(a, b), from_bn(r)));
    CHECK(u256_eq(from_mont<M>(mont_mul<M>(to_mont<M>(a), to_mont<M>(b))), from_bn(r)));
    BN_mod_add(r, ba, bb, m, ctx);
    CHECK(u256_eq(mod_add<M>(a, b), from_bn(r)));
    BN_mod_sub(r, ba, bb, m, ctx);
    CHECK(u256_eq(mod_sub<M>(a, b), from_bn(r)));
    BN_free(ba);
    BN_free(bb);
  };
  for (size_t i = 0; i < n_special; i++)
    for (size_t j = 0; j < n_special; j++) pair(ops[i], ops[j]);
  for (size_t i = n_special; i + 1 < ops.size(); i++) {
    pair(ops[i], ops[i + 1]);
    pair(ops[i], ops[i]);
    pair(ops[i], ops[i % n_special]);
  }
  for (size_t i = 0; i < ops.size(); i++) {
    if (i >= n_special + 60) break;  // an inversion is 400 multiplications
    const u256& a = ops[i];
    CHECK(u256_eq(from_mont<M>(to_mont<M>(a)), a));
    if (u256_is_zero(a)) {
      CHECK(u256_is_zero(mod_inv<M>(a)));
      continue;
    }
    BIGNUM* ba = to_bn(a);
    CHECK(BN_mod_inverse(r, ba, m, ctx) != nullptr);
    CHECK(u256_eq(mod_inv<M>(a), from_bn(r)));
    BN_free(ba);
  }
  // byte order and compare
  uint8_t be[32];
  for (int i = 0; i < 32; i++) be[i] = (uint8_t)i;
  const u256 ld = u256_load_be(be);
  CHECK(ld.v[7] == 0x00010203u && ld.v[0] == 0x1C1D1E1Fu);
  uint8_t back[32];
  u256_store_be(ld, back);
  CHECK(memcmp(be, back, 32) == 0);
  CHECK(u256_lt(small(1), small(2)) && !u256_lt(small(2), small(2)) && !u256_lt(mv, small(5)));
  u256 s;
  CHECK(u256_add(s, ones, small(1)) == 1 && u256_is_zero(s));
  CHECK(u256_sub(s, u256_zero(), small(1)) == 1 && u256_eq(s, ones));
  BN_free(r);
}

// ---- points ---------------------------------------------------------------------------------
static affine affine_of(const EC_POINT* pt) {
  affine a;
  a.x = u256_zero();
  a.y = u256_zero();
  if (EC_POINT_is_at_infinity(grp, pt)) return a;
  BIGNUM *x = BN_new(), *y = BN_new();
  EC_POINT_get_affine_coordinates(grp, pt, x, y, ctx);
  a.x = to_mont<ModP>(from_bn(x));
  a.y = to_mont<ModP>(from_bn(y));
  BN_free(x);
  BN_free(y);
  return a;
}
static bool same_point(const jac& j, const EC_POINT* pt) {
  const affine a = jac_to_affine(j), b = affine_of(pt);
  if (jac_is_infinity(j) != (EC_POINT_is_at_infinity(grp, pt) == 1)) return false;
  return u256_eq(a.x, b.x) && u256_eq(a.y, b.y);
}
static EC_POINT* rand_point() {
  EC_POINT* pt = EC_POINT_new(grp);
  BIGNUM* k = to_bn(mod_reduce<ModN>(rand256()));
  EC_POINT_mul(grp, pt, k, nullptr, nullptr, ctx);
  BN_free(k);
  return pt;
}
// the same point with another Z: (X l^2, Y l^3, Z l)
static jac rescale(const jac& p) {
  const u256 l = to_mont<ModP>(mod_reduce<ModP>(rand256()));
  const u256 l2 = mont_sqr<ModP>(l);
  jac r;
  r.X = mont_mul<ModP>(p.X, l2);
  r.Y = mont_mul<ModP>(p.Y, mont_mul<ModP>(l, l2));
  r.Z = mont_mul<ModP>(p.Z, l);
  return r;
}

static void test_points() {
  EC_POINT* sum = EC_POINT_new(grp);
  EC_POINT* inf = EC_POINT_new(grp);
  EC_POINT_set_to_infinity(grp, inf);
  const affine ainf = affine_of(inf);
  CHECK(affine_is_infinity(ainf) && jac_is_infinity(jac_infinity()) && jac_is_infinity(jac_from_affine(ainf)));
  CHECK(affine_on_curve(p256_generator()));
  CHECK(same_point(jac_from_affine(p256_generator()), EC_GROUP_get0_generator(grp)));
  for (int it = 0; it < 60; it++) {
    EC_POINT *P = rand_point(), *Q = rand_point();
    const affine ap = affine_of(P), aq = affine_of(Q);
    CHECK(affine_on_curve(ap));
    const jac jp = jac_from_affine(ap), jq = jac_from_affine(aq);
    const jac jp2 = rescale(jp), jq2 = rescale(jq);  // Z != 1
    CHECK(same_point(jp2, P));
    // double
    EC_POINT_dbl(grp, sum, P, ctx);
    CHECK(same_point(jac_double(jp), sum));
    CHECK(same_point(jac_double(jp2), sum));
    // P + P through both adds: the doubling case, with equal and with different Z
    CHECK(same_point(jac_add(jp, jp), sum));
    CHECK(same_point(jac_add(jp2, jp), sum));
    CHECK(same_point(jac_add(jp2, rescale(jp)), sum));
    CHECK(same_point(jac_madd(jp, ap), sum));
    CHECK(same_point(jac_madd(jp2, ap), sum));
    // P + Q
    EC_POINT_add(grp, sum, P, Q, ctx);
    CHECK(same_point(jac_add(jp, jq), sum));
    CHECK(same_point(jac_add(jp2, jq2), sum));
    CHECK(same_point(jac_add(jq2, jp), sum));
    CHECK(same_point(jac_madd(jp, aq), sum));
    CHECK(same_point(jac_madd(jp2, aq), sum));
    CHECK(same_point(jac_madd(jq2, ap), sum));
    // P + (-P)
    EC_POINT* N = EC_POINT_dup(P, grp);
    EC_POINT_invert(grp, N, ctx);
    const affine an = affine_of(N);
    EC_POINT_add(grp, sum, P, N, ctx);
    CHECK(EC_POINT_is_at_infinity(grp, sum) == 1);
    CHECK(jac_is_infinity(jac_add(jp, jac_from_affine(an))));
    CHECK(jac_is_infinity(jac_add(jp2, rescale(jac_from_affine(an)))));
    CHECK(jac_is_infinity(jac_madd(jp, an)));
    CHECK(jac_is_infinity(jac_madd(jp2, an)));
    // infinity on either side
    CHECK(same_point(jac_add(jp2, jac_infinity()), P));
    CHECK(same_point(jac_add(jac_infinity(), jp2), P));
    CHECK(same_point(jac_madd(jp2, ainf), P));
    CHECK(same_point(jac_madd(jac_infinity(), ap), P));
    CHECK(jac_is_infinity(jac_add(jac_infinity(), jac_infinity())));
    CHECK(jac_is_infinity(jac_madd(jac_infinity(), ainf)));
    CHECK(jac_is_infinity(jac_double(jac_infinity())));
    // a zero-Z point with other X, Y is infinity too
    jac z = jp2;
    z.Z = u256_zero();
    CHECK(jac_is_infinity(jac_double(z)));
    CHECK(same_point(jac_add(z, jq2), Q));
    EC_POINT_free(N);
    EC_POINT_free(P);
    EC_POINT_free(Q);
  }
  EC_POINT_free(sum);
  EC_POINT_free(inf);
}

// ---- scalar multiplication -------------------------------------------------------------------
static std::vector<u256> scalars() {
  std::vector<u256> s;
  u256 t;
  s.push_back(u256_zero());
  s.push_back(small(1));
  s.push_back(small(15));
  s.push_back(small(16));
  u256_sub(t, mod_value<ModN>(), small(1));
  s.push_back(t);  // n - 1
  u256 a;
  for (int i = 0; i < 8; i++) a.v[i] = 0xFFFFFFFFu;  // every window 2^w - 1 (>= n: OpenSSL reduces, the ladder need not)
  s.push_back(a);
  a.v[7] = 0x0FFFFFFFu;  // the same below n
  s.push_back(a);
  for (int i = 0; i < 8; i++) a.v[i] = 0xF0F0F0F0u;  // whole zero windows between full ones
  a.v[7] = 0x00F0F0F0u;
  s.push_back(a);
  for (int i = 0; i < 8; i++) a.v[i] = 0x000F0001u;
  s.push_back(a);
  a = u256_zero();
  a.v[7] = 0x10000000u;  // only the top window
  s.push_back(a);
  a = u256_zero();
  a.v[3] = 0x000F0000u;  // one window in the middle
  s.push_back(a);
  for (int i = 0; i < 12; i++) s.push_back(mod_reduce<ModN>(rand256()));
  return s;
}

static void test_scalar_mult() {
  affine gtab[kTableEntries];
  p256_window_table(p256_generator(), gtab);
  // the table itself: d G
  EC_POINT* pt = EC_POINT_new(grp);
  for (int d = 1; d < kTableEntries; d++) {
    BIGNUM* k = to_bn(small((uint32_t)d));
    EC_POINT_mul(grp, pt, k, nullptr, nullptr, ctx);
    CHECK(same_point(jac_from_affine(gtab[d]), pt));
    BN_free(k);
  }
  const std::vector<u256> sc = scalars();
  for (int key = 0; key < 3; key++) {
    EC_POINT* Q = key == 0 ? EC_POINT_dup(EC_GROUP_get0_generator(grp), grp) : rand_point();
    if (key == 1) EC_POINT_invert(grp, Q, ctx);
    affine qtab[kTableEntries];
    p256_window_table(affine_of(Q), qtab);
    for (size_t i = 0; i < sc.size(); i++) {
      BIGNUM* k1 = to_bn(sc[i]);
      if (key == 0) {  // k G alone
        EC_POINT_mul(grp, pt, k1, nullptr, nullptr, ctx);
        CHECK(same_point(p256_shamir(sc[i], u256_zero(), gtab, qtab), pt));
        EC_POINT_mul(grp, pt, nullptr, Q, k1, ctx);
        CHECK(same_point(p256_shamir(u256_zero(), sc[i], gtab, qtab), pt));
      }
      for (size_t j = 0; j < sc.size(); j++) {
        BIGNUM* k2 = to_bn(sc[j]);
        EC_POINT_mul(grp, pt, k1, Q, k2, ctx);
        CHECK(same_point(p256_shamir(sc[i], sc[j], gtab, qtab), pt));
        BN_free(k2);
      }
      BN_free(k1);
    }
    EC_POINT_free(Q);
  }
  EC_POINT_free(pt);
}

// ---- key decoding ---------------------------------------------------------------------------------
static bool openssl_decodes(const uint8_t* pub) {
  EC_POINT* pt = EC_POINT_new(grp);
  // elliptic.Unmarshal takes only the uncompressed form (hge_ingest.cpp's rule)
  const bool ok = pub[0] == 0x04 && EC_POINT_oct2point(grp, pt, pub, 65, ctx) == 1;
  EC_POINT_free(pt);
  return ok;
}
static void check_key(const uint8_t* pub, bool want) {
  affine a;
  CHECK(openssl_decodes(pub) == want);
  CHECK(p256_key_decode(pub, a) == want);
  if (!want) CHECK(affine_is_infinity(a));
}
static void pub_of(const EC_POINT* pt, uint8_t* pub) {
  if (EC_POINT_point2oct(grp, pt, POINT_CONVERSION_UNCOMPRESSED, pub, 65, ctx) != 65) {
    printf("FAIL: point2oct\n");
    exit(1);
  }
}

static void test_key_decode() {
  for (int it = 0; it < 20; it++) {
    EC_POINT* P = rand_point();
    uint8_t pub[65], bad[65];
    pub_of(P, pub);
    check_key(pub, true);
    affine a;
    p256_key_decode(pub, a);
    CHECK(same_point(jac_from_affine(a), P));
    memcpy(bad, pub, 65);
    bad[64] ^= 1;  // a y bit
    check_key(bad, false);
    memcpy(bad, pub, 65);
    bad[1 + (it % 32)] ^= 0x40;  // an x bit: off the curve (or another point; OpenSSL decides)
    {
      affine b;
      CHECK(p256_key_decode(bad, b) == openssl_decodes(bad));
    }
    memcpy(bad, pub, 65);
    bad[0] = 2;
    check_key(bad, false);
    bad[0] = 3;
    check_key(bad, false);
    bad[0] = 0;
    check_key(bad, false);
    memcpy(bad, pub, 65);
    u256_store_be(mod_value<ModP>(), bad + 1);  // X = p
    check_key(bad, false);
    memcpy(bad, pub, 65);
    u256_store_be(mod_value<ModP>(), bad + 33);  // Y = p
    check_key(bad, false);
    EC_POINT_free(P);
  }
  uint8_t z[65];
  memset(z, 0, 65);
  check_key(z, false);
  z[0] = 4;  // the all-zero point
  check_key(z, false);
  // x = 0 has a square root on this curve (b is a square): a valid key with a zero coordinate
  {
    EC_POINT* P = EC_POINT_new(grp);
    BIGNUM* zero = BN_new();
    BN_zero(zero);
    if (EC_POINT_set_compressed_coordinates(grp, P, zero, 0, ctx) == 1) {
      uint8_t pub[65];
      pub_of(P, pub);
      check_key(pub, true);
    }
    BN_free(zero);
    EC_POINT_free(P);
  }
}

// ---- ECDSA ---------------------------------------------------------------------------------------
struct Key {
  EC_KEY* k;
  uint8_t pub[65];
  affine pt;
  affine tab[kTableEntries];
};
static affine g_gtab[kTableEntries];

static void key_finish(Key& key) {
  pub_of(EC_KEY_get0_public_key(key.k), key.pub);
  if (!p256_key_decode(key.pub, key.pt)) {
    printf("FAIL: key does not decode\n");
    exit(1);
  }
  p256_window_table(key.pt, key.tab);
}
static Key key_from_point(const EC_POINT* pt) {
  Key key;
  key.k = EC_KEY_new_by_curve_name(NID_X9_62_prime256v1);
  EC_KEY_set_public_key(key.k, pt);
  key_finish(key);
  return key;
}
static int openssl_verify(const uint8_t* dg, const uint8_t* sig, const Key& key) {
  ECDSA_SIG* es = ECDSA_SIG_new();
  ECDSA_SIG_set0(es, BN_bin2bn(sig, 32, nullptr), BN_bin2bn(sig + 32, 32, nullptr));
  const int v = ECDSA_do_verify(dg, 32, es, key.k);
  ECDSA_SIG_free(es);
  return v == 1 ? 1 : 0;
}
// both forms of the header's verify against OpenSSL, and against the expected verdict
static void check_sig(const uint8_t* dg, const uint8_t* sig, const Key& key, int want, bool slow_too = false) {
  CHECK(openssl_verify(dg, sig, key) == want);
  CHECK(p256_ecdsa_verify_tables(dg, g_gtab, key.tab, sig) == want);
  if (slow_too) CHECK(p256_ecdsa_verify_digest(dg, key.pt, sig) == want);
}
static void sign(const uint8_t* dg, const Key& key, uint8_t* sig) {
  ECDSA_SIG* es = ECDSA_do_sign(dg, 32, key.k);
  const BIGNUM *r, *s;
  ECDSA_SIG_get0(es, &r, &s);
  BN_bn2binpad(r, sig, 32);
  BN_bn2binpad(s, sig + 32, 32);
  ECDSA_SIG_free(es);
}

static void test_ecdsa() {
  p256_window_table(p256_generator(), g_gtab);
  Key keys[4];
  for (Key& key : keys) {
    key.k = EC_KEY_new_by_curve_name(NID_X9_62_prime256v1);
    EC_KEY_generate_key(key.k);
    key_finish(key);
  }
  uint8_t nb[32], zero[32];
  u256_store_be(mod_value<ModN>(), nb);
  memset(zero, 0, 32);
  for (int it = 0; it < 320; it++) {
    const Key& key = keys[it % 4];
    uint8_t dg[32], sig[64], bad[64], dg2[32];
    u256_store_be(rand256(), dg);
    if (it % 16 == 5) memset(dg, 0xFF, 32);  // e >= n: reduced
    if (it % 16 == 6) memset(dg, 0, 32);     // digest 0: u1 = 0
    sign(dg, key, sig);
    check_sig(dg, sig, key, 1, it < 24);
    if (it >= 80) continue;
    memcpy(bad, sig, 64);
    bad[it % 32] ^= (uint8_t)(1u << (it % 8));  // an r bit
    check_sig(dg, bad, key, 0);
    memcpy(bad, sig, 64);
    bad[32 + it % 32] ^= (uint8_t)(1u << (it % 7));  // an s bit
    check_sig(dg, bad, key, 0);
    memcpy(dg2, dg, 32);
    dg2[(it * 7) % 32] ^= 0x20;
    check_sig(dg2, sig, key, 0);
    check_sig(dg, sig, keys[(it + 1) % 4], 0);  // another key
    memcpy(bad, sig, 64);
    memcpy(bad, zero, 32);  // r = 0
    check_sig(dg, bad, key, 0);
    memcpy(bad, nb, 32);  // r = n
    check_sig(dg, bad, key, 0);
    memcpy(bad, sig, 64);
    memcpy(bad + 32, zero, 32);  // s = 0
    check_sig(dg, bad, key, 0);
    memcpy(bad + 32, nb, 32);  // s = n
    check_sig(dg, bad, key, 0);
    memset(bad, 0xFF, 64);  // both above n
    check_sig(dg, bad, key, 0);
  }
  // Q = G with e = r: s = 2 r / k makes u1 = u2, so the ladder's first two adds are
  // G-multiple + the same G-multiple (the doubling case); the signature is valid.
  // Q = -G with e = r: u1 G + u2 Q is infinity whatever s is; it must be refused.
  Key kg = key_from_point(EC_GROUP_get0_generator(grp));
  EC_POINT* ng = EC_POINT_dup(EC_GROUP_get0_generator(grp), grp);
  EC_POINT_invert(grp, ng, ctx);
  Key kn = key_from_point(ng);
  for (int it = 0; it < 12; it++) {
    BIGNUM* k = to_bn(mod_reduce<ModN>(rand256()));
    EC_POINT* kp = EC_POINT_new(grp);
    EC_POINT_mul(grp, kp, k, nullptr, nullptr, ctx);
    BIGNUM *x = BN_new(), *r = BN_new(), *s = BN_new(), *ki = BN_new();
    EC_POINT_get_affine_coordinates(grp, kp, x, nullptr, ctx);
    BN_nnmod(r, x, bn_n, ctx);
    BN_mod_inverse(ki, k, bn_n, ctx);
    BN_mod_add(s, r, r, bn_n, ctx);
    BN_mod_mul(s, s, ki, bn_n, ctx);
    uint8_t dg[32], sig[64];
    BN_bn2binpad(r, dg, 32);
    BN_bn2binpad(r, sig, 32);
    BN_bn2binpad(s, sig + 32, 32);
    check_sig(dg, sig, kg, 1, it < 2);
    check_sig(dg, sig, kn, 0, it < 2);
    u256_store_be(mod_reduce<ModN>(rand256()), sig + 32);
    if (!u256_is_zero(u256_load_be(sig + 32))) check_sig(dg, sig, kn, 0);
    BN_free(k);
    BN_free(x);
    BN_free(r);
    BN_free(s);
    BN_free(ki);
    EC_POINT_free(kp);
  }
  EC_POINT_free(ng);
  EC_KEY_free(kg.k);
  EC_KEY_free(kn.k);
  for (Key& key : keys) EC_KEY_free(key.k);
}

static void test_sha256() {
  uint8_t buf[400], a[32], b[32];
  for (int i = 0; i < 400; i++) buf[i] = (uint8_t)rng();
  for (int len = 0; len <= 130; len++) {
    SHA256(buf + (len % 3), (size_t)len, a);
    sha256(buf + (len % 3), (uint64_t)len, b);
    CHECK(memcmp(a, b, 32) == 0);
  }
  for (int len : {161, 191, 192, 193, 255, 256, 300, 399}) {
    SHA256(buf, (size_t)len, a);
    sha256(buf, (uint64_t)len, b);
    CHECK(memcmp(a, b, 32) == 0);
  }
  sha256(nullptr, 0, b);
  SHA256(buf, 0, a);
  CHECK(memcmp(a, b, 32) == 0);
}

int main() {
  ctx = BN_CTX_new();
  grp = EC_GROUP_new_by_curve_name(NID_X9_62_prime256v1);
  bn_p = BN_new();
  bn_n = BN_new();
  EC_GROUP_get_curve(grp, bn_p, nullptr, nullptr, ctx);
  EC_GROUP_get_order(grp, bn_n, ctx);
  test_mod<ModP>(bn_p);
  test_mod<ModN>(bn_n);
  test_points();
  test_scalar_mult();
  test_key_decode();
  test_ecdsa();
  test_sha256();
  BN_free(bn_p);
  BN_free(bn_n);
  EC_GROUP_free(grp);
  BN_CTX_free(ctx);
  printf("ok %ld\n", g_checks);
  return 0;
}
