// kh_host.h -- host-side arithmetic shared by the C-ABI translation units (kh_capi*.cpp): 256-bit
// scalars mod n, libbloom2 sizing and the host bloom, searchbinary, the comb table and batch inversion.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "kh_kernels.h"
#include "kh_math.h"

namespace kh_host {
using namespace kh;

// ==============================================================================================
// 256-bit scalars (mod n) on the host
// ==============================================================================================
typedef unsigned __int128 u128;
struct u256 {
  uint64_t v[4];
};
const u256 ORDER_N = {{0xBFD25E8CD0364141ULL, 0xBAAEDCE6AF48A03BULL, 0xFFFFFFFFFFFFFFFEULL, 0xFFFFFFFFFFFFFFFFULL}};

inline u256 u256_from_be(const uint8_t b[32]) {
  u256 r;
  for (int i = 0; i < 4; i++) {
    uint64_t w = 0;
    for (int j = 0; j < 8; j++) w = (w << 8) | b[(3 - i) * 8 + j];
    r.v[i] = w;
  }
  return r;
}
inline void u256_to_be(uint8_t b[32], const u256 &a) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 8; j++) b[(3 - i) * 8 + j] = (uint8_t)(a.v[i] >> (56 - 8 * j));
}
inline u256 u256_from_u128(u128 x) { return u256{{(uint64_t)x, (uint64_t)(x >> 64), 0, 0}}; }
inline u256 u256_u64(uint64_t x) { return u256{{x, 0, 0, 0}}; }
inline int u256_cmp(const u256 &a, const u256 &b) {
  for (int i = 3; i >= 0; i--) {
    if (a.v[i] < b.v[i]) return -1;
    if (a.v[i] > b.v[i]) return 1;
  }
  return 0;
}
// st + count*stride >= n as plain integers (a key span that reaches the group order)
inline bool reaches_order(const u256 &st, const u256 &stride, uint64_t count) {
  u256 r;
  unsigned __int128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (unsigned __int128)stride.v[i] * count + st.v[i];
    r.v[i] = (uint64_t)c;
    c >>= 64;
  }
  return c != 0 || u256_cmp(r, ORDER_N) >= 0;
}
inline bool u256_is_zero(const u256 &a) { return (a.v[0] | a.v[1] | a.v[2] | a.v[3]) == 0; }
inline uint64_t u256_add_raw(u256 &r, const u256 &a, const u256 &b) {
  u128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (u128)a.v[i] + b.v[i];
    r.v[i] = (uint64_t)c;
    c >>= 64;
  }
  return (uint64_t)c;
}
inline uint64_t u256_sub_raw(u256 &r, const u256 &a, const u256 &b) {
  uint64_t br = 0;
  for (int i = 0; i < 4; i++) {
    u128 t = (u128)a.v[i] - b.v[i] - br;
    r.v[i] = (uint64_t)t;
    br = (uint64_t)(t >> 64) & 1;
  }
  return br;
}
inline u256 sc_reduce(u256 a) {
  while (u256_cmp(a, ORDER_N) >= 0) u256_sub_raw(a, a, ORDER_N);
  return a;
}
inline u256 sc_add(const u256 &a, const u256 &b) {
  u256 r;
  uint64_t c = u256_add_raw(r, a, b);
  if (c || u256_cmp(r, ORDER_N) >= 0) u256_sub_raw(r, r, ORDER_N);
  return r;
}
inline u256 sc_neg(const u256 &a) {
  if (u256_is_zero(a)) return a;
  u256 r;
  u256_sub_raw(r, ORDER_N, a);
  return r;
}
inline u256 sc_sub(const u256 &a, const u256 &b) { return sc_add(a, sc_neg(b)); }
// x * m mod n for x < n, m < 2^128: double-and-add over the bits of m
inline u256 sc_mul_u128(const u256 &x, u128 m) {
  u256 r = u256_u64(0), y = x;
  for (; m; m >>= 1) {
    if (m & 1) r = sc_add(r, y);
    y = sc_add(y, y);
  }
  return r;
}
// a * b mod n (double-and-add; only used per confirmed hit)
inline u256 sc_mul(const u256 &a, const u256 &b) {
  u256 r = u256_u64(0), x = a;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 64; j++) {
      if ((b.v[i] >> j) & 1) r = sc_add(r, x);
      x = sc_add(x, x);
    }
  return r;
}
// a^-1 mod n (Fermat, a^(n-2); a != 0).  Host only, per chunk at most
inline u256 sc_inv(const u256 &a) {
  u256 e;
  u256_sub_raw(e, ORDER_N, u256_u64(2));
  u256 r = u256_u64(1), x = a;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 64; j++) {
      if ((e.v[i] >> j) & 1) r = sc_mul(r, x);
      x = sc_mul(x, x);
    }
  return r;
}
inline void u256_to_limbs(uint32_t out[8], const u256 &a) {
  for (int i = 0; i < 4; i++) {
    out[2 * i] = (uint32_t)a.v[i];
    out[2 * i + 1] = (uint32_t)(a.v[i] >> 32);
  }
}

// ==============================================================================================
// libbloom2 sizing, exactly as bloom/bloom.cpp:154-187 computes it (long double, bpe as double)
// ==============================================================================================
inline bloom_desc bloom_size(uint64_t entries) {
  long double num = -logl((long double)0.000001);
  long double denom = 0.480453013918201;
  double bpe = (double)(num / denom);
  long double allbits = (long double)entries * bpe;
  bloom_desc d;
  memset(&d, 0, sizeof d);
  d.bits = (uint64_t)allbits;
  d.bytes = d.bits / 8 + ((d.bits % 8) ? 1 : 0);
  d.hashes = (uint32_t)(uint8_t)ceil(0.693147180559945 * bpe);
  d.recip = ~0ULL / d.bits;
  d.stride = d.bytes;
  return d;
}
// keyhunt's entry count rule: initBloomFilter uses max(10000, items) (keyhunt.cpp:7608)
inline uint64_t bloom_entries(uint64_t items) { return items <= 10000 ? 10000 : items; }

inline void host_bloom_hash(const uint8_t *buf, int len, uint64_t &a, uint64_t &b) {
  if (len == 32) {
    uint64_t in[4];
    for (int k = 0; k < 4; k++) {
      uint64_t v = 0;
      for (int q = 7; q >= 0; q--) v = (v << 8) | buf[8 * k + q];
      in[k] = v;
    }
    a = xxh64_32(in, KH_BLOOM_SEED);
    b = xxh64_32(in, a);
  } else {  // 20 bytes, or a shorter hash160 prefix (vanity)
    uint8_t p[20] = {0};
    memcpy(p, buf, (size_t)std::min(len, 20));
    uint32_t w[5];
    for (int k = 0; k < 5; k++)
      w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) |
             ((uint32_t)p[4 * k + 3] << 24);
    if (len == 20) {
      a = xxh64_20(w, KH_BLOOM_SEED);
      b = xxh64_20(w, a);
    } else {
      a = xxh64_prefix(w, (uint32_t)len, KH_BLOOM_SEED);
      b = xxh64_prefix(w, (uint32_t)len, a);
    }
  }
}
inline void host_bloom_add(uint8_t *bf, const bloom_desc &d, const uint8_t *buf, int len) {
  uint64_t a, b;
  host_bloom_hash(buf, len, a, b);
  uint64_t h = a;
  for (uint32_t i = 0; i < d.hashes; i++) {
    uint64_t x = h % d.bits;
    bf[x >> 3] |= (uint8_t)(1u << (x & 7));
    h += b;
  }
}
inline bool host_bloom_check(const uint8_t *bf, const bloom_desc &d, const uint8_t *buf, int len) {
  uint64_t a, b;
  host_bloom_hash(buf, len, a, b);
  uint64_t h = a;
  for (uint32_t i = 0; i < d.hashes; i++) {
    uint64_t x = h % d.bits;
    if (!((bf[x >> 3] >> (x & 7)) & 1)) return false;
    h += b;
  }
  return true;
}

// searchbinary (keyhunt.cpp:3065-3089): the reference's own midpoint loop
inline bool searchbinary(const uint8_t *rows, int64_t n, const uint8_t *key, int width, int key_off) {
  int64_t half = n, min = 0, max = n, cur = 0;
  while (half >= 1) {
    half = (max - min) / 2;
    int c = memcmp(key + key_off, rows + (cur + half) * width, width);
    if (c == 0) return true;
    if (c < 0)
      max = max - half;
    else
      min = min + half;
    cur = min;
  }
  return false;
}

// ==============================================================================================
// host EC with the comb table (the same table the setup kernel reads)
// ==============================================================================================
inline ge G_POINT() {
  ge g;
  const uint64_t gx[4] = {0x59F2815B16F81798ULL, 0x029BFCDB2DCE28D9ULL, 0x55A06295CE870B07ULL, 0x79BE667EF9DCBBACULL};
  const uint64_t gy[4] = {0x9C47D08FFB10D4B8ULL, 0xFD17B448A6855419ULL, 0x5DA4FBFC0E1108A8ULL, 0x483ADA7726A3C465ULL};
  fe_from_u64(g.x, gx);
  fe_from_u64(g.y, gy);
  return g;
}

struct comb_table {
  std::vector<ge> t;  // 32 * 256 (entry v = 0 unused)
  void build() {
    t.assign(32 * 256, ge{});
    ge base = G_POINT();
    for (int j = 0; j < 32; j++) {
      t[j * 256 + 1] = base;
      ge_double(t[j * 256 + 2], base);
      for (int v = 3; v < 256; v++) ge_add(t[j * 256 + v], t[j * 256 + v - 1], base);
      if (j < 31) {
        ge b = base;
        for (int k = 0; k < 8; k++) ge_double(b, b);
        base = b;
      }
    }
  }
  // k*G (k reduced mod n, k != 0); returns false for k == 0
  bool mult(ge &r, const u256 &k_in) const {
    u256 k = sc_reduce(k_in);
    if (u256_is_zero(k)) return false;
    gej acc;
    acc.inf = true;
    for (int j = 0; j < 32; j++) {
      uint32_t v = (uint32_t)(k.v[j >> 3] >> ((j & 7) * 8)) & 0xFF;
      if (v) gej_add_ge(acc, t[j * 256 + v]);
    }
    gej_to_ge(r, acc);
    return true;
  }
};

// the process's own comb table, built on first use (hosts without a context: the CLI's hit text, tests)
inline const comb_table &host_comb() {
  static const comb_table c = [] {
    comb_table t;
    t.build();
    return t;
  }();
  return c;
}

// BIP-341 key-path output key of the internal key P = (x, y) (no script tree, BIP-86): out32 = x(Q),
// Q = P' + t*G with P' = P of even Y (lift_x(x); y spares the square root) and t = SHA-256_TapTweak(x)
// read big-endian.  false where BIP-341 fails: t >= n, or Q the point at infinity (t*G = -P').  The twin
// of k_tap_keys on the host comb: the scan's hit confirmation and the CLI's hit text use it.
inline bool taproot_output_x(const comb_table &comb, const fe &x, const fe &y, uint8_t out32[32]) {
  uint32_t st[8];
  taptweak_hash(x, st);
  u256 t;
  for (int i = 0; i < 4; i++) t.v[i] = ((uint64_t)st[6 - 2 * i] << 32) | st[7 - 2 * i];
  if (u256_cmp(t, ORDER_N) >= 0) return false;
  ge p{x, y};
  if (y.d[0] & 1u) fe_neg(p.y, y);
  ge q = p;
  ge tg;
  if (comb.mult(tg, t)) {
    if (fe_eq(tg.x, p.x)) {
      if (!fe_eq(tg.y, p.y)) return false;
      ge_double(q, p);
    } else {
      ge_add(q, tg, p);
    }
  }
  fe_to_be(out32, q.x);
  return true;
}
inline bool taproot_output_x(const fe &x, const fe &y, uint8_t out32[32]) {
  return taproot_output_x(host_comb(), x, y, out32);
}

// Montgomery-trick batch inversion (IntGroup::ModInv); zero elements are skipped (left 0)
inline void batch_inv(std::vector<fe> &a) {
  size_t n = a.size();
  std::vector<fe> pre(n);
  fe acc;
  fe_set_u32(acc, 1);
  for (size_t i = 0; i < n; i++) {
    if (!fe_is_zero(a[i])) fe_mul(acc, acc, a[i]);
    pre[i] = acc;
  }
  fe inv;
  fe_inv(inv, acc);
  for (size_t i = n; i-- > 0;) {
    if (fe_is_zero(a[i])) continue;
    fe prev;
    if (i == 0)
      fe_set_u32(prev, 1);
    else
      prev = pre[i - 1];
    fe t;
    fe_mul(t, inv, prev);
    fe_mul(inv, inv, a[i]);
    a[i] = t;
  }
}

}  // namespace kh_host
