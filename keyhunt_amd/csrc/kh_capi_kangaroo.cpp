// kh_capi_kangaroo.cpp -- Pollard's lambda ("kangaroo") search for one public key in a bounded interval:
// the herd on the device (k_kang_step, kh_kernels.hip), its placement through the lane-setup kernel, and the
// host table of distinguished points with the collision's resolution.  The reference has no such search.
#include <array>

#include "kh_ctx.h"

namespace {

constexpr uint32_t KANG_MAX_HERD = 1u << 24;
// The default herd: 2^23 kangaroos, 2^18 lanes of KH_KANG_BATCH = 32 -- one wave in each of the chip's 4096 wave
// slots at 4 waves/SIMD.  The walk is bound by latency and its rate grows with the herd: 0.59, 1.98, 7.5, 10.2
// and 12.4 G jumps/s at 2^17, 2^19, 2^21, 2^22 and 2^23 (profiles/kangaroo_rate_ab.json); a range too narrow
// for such a herd gets a smaller one (default_herd)
constexpr uint32_t KANG_HERD = 1u << 23;
constexpr uint32_t KANG_PLACE_CHUNK = 1u << 20;  // kangaroos placed per k_setup pass
constexpr uint32_t KANG_REC_CAP0 = 1u << 16;     // kh_kang_solve: records per launch the device keeps at least

int bitlen(const u256 &a) {
  for (int i = 3; i >= 0; i--)
    if (a.v[i]) return 64 * i + 64 - __builtin_clzll(a.v[i]);
  return 0;
}
u256 shl(const u256 &a, int s) {  // s < 256
  u256 r{};
  const int q = s / 64, b = s % 64;
  for (int i = 3; i >= q; i--) {
    r.v[i] = a.v[i - q] << b;
    if (b && i - q - 1 >= 0) r.v[i] |= a.v[i - q - 1] >> (64 - b);
  }
  return r;
}
u256 shr1(const u256 &a) {
  u256 r;
  for (int i = 0; i < 4; i++) r.v[i] = (a.v[i] >> 1) | (i < 3 ? a.v[i + 1] << 63 : 0);
  return r;
}
// h mod m, m != 0: subtract m's shifts from the top
u256 mod(u256 h, const u256 &m) {
  for (int s = bitlen(h) - bitlen(m); s >= 0; s--) {
    const u256 t = shl(m, s);
    if (u256_cmp(h, t) >= 0) u256_sub_raw(h, h, t);
  }
  return h;
}
// (8 v)^2 <= W, v < 2^60: v <= sqrt(W) / 8
bool fits_sqrt8(uint64_t v, const u256 &W) {
  const u128 q = (u128)(8 * v) * (8 * v);
  return u256_cmp(u256_from_u128(q), W) <= 0;
}
uint32_t default_dp(uint32_t N, const u256 &W) {
  uint32_t dp = 0;
  while (dp < 32 && fits_sqrt8((uint64_t)N << (dp + 1), W)) dp++;
  return dp;
}
// Jumps per kangaroo per launch: what kh_kang_set_launch gave, else the largest power of two up to
// KH_KANG_STEPS that keeps a launch of the whole herd below sqrt(W)/16 jumps, so that a search of about
// 2 sqrt(W) jumps overshoots its end by a few per cent at the most
uint32_t launch_steps(const kang_state &K) {
  if (K.steps_per_launch) return K.steps_per_launch;
  uint32_t s = 1;
  while (s < KH_KANG_STEPS && K.N && fits_sqrt8((uint64_t)K.N * s * 4, K.W)) s *= 2;
  return s;
}
uint32_t default_herd(const u256 &W) {
  uint32_t n = 64;
  // a sixteenth of the sqrt(W)/8 that herd and distinguished points share: the automatic dp_bits stays >= 4
  while (n < KANG_HERD && fits_sqrt8((uint64_t)n * 2 * 16, W)) n *= 2;
  return n;
}

u256 digest_int(const uint8_t *msg, size_t n) {
  uint8_t d[32];
  sha256_bytes(msg, n, d);
  return u256_from_be(d);
}
void default_jumps(const u256 &W, u256 out[KH_KANG_JUMPS]) {
  const int jb = bitlen(W) / 2 + 1;  // <= 97
  u256 mask = shl(u256_u64(1), jb);
  u256_sub_raw(mask, mask, u256_u64(1));
  for (int j = 0; j < KH_KANG_JUMPS; j++) {
    uint8_t msg[18];
    memcpy(msg, "kh-kangaroo-jump", 16);
    msg[16] = (uint8_t)j;
    msg[17] = (uint8_t)jb;
    u256 d = digest_int(msg, 18);
    for (int i = 0; i < 4; i++) d.v[i] &= mask.v[i];
    if (u256_is_zero(d)) d = u256_u64(1);
    for (bool again = true; again;) {
      again = false;
      for (int i = 0; i < j; i++)
        if (u256_cmp(out[i], d) == 0) {
          u256_add_raw(d, d, u256_u64(1));
          again = true;
        }
    }
    out[j] = d;
  }
}
// the seeding rule: kangaroo `index` at its generation `gen`
u256 seed_dist(const kang_state &K, uint32_t index, uint32_t gen) {
  uint8_t msg[16];
  for (int i = 0; i < 8; i++) msg[i] = (uint8_t)(K.seed >> (8 * i));
  for (int i = 0; i < 4; i++) msg[8 + i] = (uint8_t)(index >> (8 * i));
  for (int i = 0; i < 4; i++) msg[12 + i] = (uint8_t)(gen >> (8 * i));
  const u256 h = digest_int(msg, 16);
  u256 r;
  if (index & 1u) {  // wild: 1 + h mod W
    u256_add_raw(r, mod(h, K.W), u256_u64(1));
  } else {           // tame: floor(W/2) + h mod (W + 1)
    u256 w1;
    u256_add_raw(w1, K.W, u256_u64(1));
    u256_add_raw(r, mod(h, w1), shr1(K.W));
  }
  return r;
}

bool on_curve(const fe &x, const fe &y) {
  fe l, r, seven;
  fe_sqr(l, y);
  fe_sqr(r, x);
  fe_mul(r, r, x);
  fe_set_u32(seven, 7);
  fe_add(r, r, seven);
  return fe_eq(l, r);
}
bool fe_be_canonical(const uint8_t b[32], fe &out) {
  fe_from_be(out, b);
  return !fe_geq_p(out);
}

// k = a + k' for the candidates k' = t - w and -(t + w); true and the key for the one with k*G = Q
bool resolve(const comb_table &comb, const u256 &t, const u256 &w, const u256 &a, const ge &Q, u256 &key) {
  const u256 tr = sc_reduce(t), wr = sc_reduce(w);
  const u256 cand[2] = {sc_sub(tr, wr), sc_neg(sc_add(tr, wr))};
  for (const u256 &kp : cand) {
    const u256 k = sc_add(sc_reduce(a), kp);
    ge P;
    if (comb.mult(P, k) && fe_eq(P.x, Q.x) && fe_eq(P.y, Q.y)) {
      key = k;
      return true;
    }
  }
  return false;
}

int upload_jumps(kh_ctx *c) {
  kang_state &K = c->kang;
  std::vector<uint32_t> h(KH_KANG_TAB_WORDS * KH_KANG_JUMPS);
  for (int j = 0; j < KH_KANG_JUMPS; j++) {
    ge J;
    if (!c->comb.mult(J, K.jd[j])) return KH_E_ARG;
    uint32_t d[8];
    u256_to_limbs(d, K.jd[j]);
    for (int w = 0; w < 8; w++) {
      h[(size_t)w * KH_KANG_JUMPS + j] = J.x.d[w];
      h[(size_t)(8 + w) * KH_KANG_JUMPS + j] = J.y.d[w];
    }
    for (int w = 0; w < 4; w++) h[(size_t)(16 + w) * KH_KANG_JUMPS + j] = d[w];
  }
  return upload(c, K.d_jumps, h.data(), h.size());
}

// the herd's buffers for N kangaroos; a new size starts an empty herd, table and statistics
int resize_herd(kh_ctx *c, uint32_t N) {
  kang_state &K = c->kang;
  if (N == K.N) return KH_OK;
  K.N = 0;
  K.d_x.reset();
  K.d_y.reset();
  K.d_dist.reset();
  K.d_unplaced.reset();
  K.d_pad.reset();
  KHTRY(K.d_x.reserve(c, (size_t)N * 8));
  KHTRY(K.d_y.reserve(c, (size_t)N * 8));
  KHTRY(K.d_dist.reserve(c, (size_t)N * 8));
  KHTRY(K.d_unplaced.reserve(c, N));
  // unplaced kangaroos of a herd that is only partly set sit at (0, 0) with distance 0 and are stalled
  HIPCHK(c, hipMemsetAsync(K.d_x.get(), 0, (size_t)N * 32, c->stream));
  HIPCHK(c, hipMemsetAsync(K.d_y.get(), 0, (size_t)N * 32, c->stream));
  HIPCHK(c, hipMemsetAsync(K.d_dist.get(), 0, (size_t)N * 32, c->stream));
  HIPCHK(c, hipMemsetAsync(K.d_unplaced.get(), 0xff, (size_t)N * 4, c->stream));
  KHTRY(K.d_count.reserve(c, 1));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // kh_kang_get_herd copies on the null stream
  K.N = N;
  K.gen.assign(N, 0);
  K.table.clear();
  K.stats = kh_kang_stats{};
  if (K.dp_auto) K.dp_bits = default_dp(N, K.W);
  return KH_OK;
}

// Kangaroos idx[i] (or first + i when idx is null), i < n, to the distances d[i]: the tames' points dist*G
// and the wilds' Q' + dist*G from two k_setup launches on buffers of their own, then k_kang_place
int place(kh_ctx *c, const uint32_t *idx, uint32_t first, uint32_t n, const u256 *d) {
  kang_state &K = c->kang;
  for (uint32_t lo = 0; lo < n; lo += KANG_PLACE_CHUNK) {
    const uint32_t m = std::min(KANG_PLACE_CHUNK, n - lo);
    std::vector<uint32_t> sc[2], dl((size_t)m * 8), ids;
    if (idx) ids.assign(idx + lo, idx + lo + m);
    for (uint32_t i = 0; i < m; i++) {
      const uint32_t e = idx ? idx[lo + i] : first + lo + i;
      u256_to_limbs(&dl[(size_t)i * 8], d[lo + i]);
      uint32_t s[8];
      u256_to_limbs(s, sc_reduce(d[lo + i]));
      sc[e & 1u].insert(sc[e & 1u].end(), s, s + 8);
    }
    const uint32_t cnt[2] = {(uint32_t)(sc[0].size() / 8), (uint32_t)(sc[1].size() / 8)};
    dev_buf<uint32_t> d_sc[2], d_px[2], d_py[2], d_bad, d_q, d_dl, d_ids, d_rk;
    std::vector<uint32_t> rank;
    if (idx) {
      // a list mixes the herds freely: entry i's rank among those of its kind
      rank.resize(m);
      uint32_t r[2] = {0, 0};
      for (uint32_t i = 0; i < m; i++) rank[i] = r[ids[i] & 1u]++;
    }
    KHTRY(upload(c, d_dl, dl.data(), dl.size()));
    KHTRY(d_bad.reserve(c, std::max(1u, cnt[1])));
    HIPCHK(c, hipMemsetAsync(d_bad.get(), 0, (size_t)std::max(1u, cnt[1]) * 4, c->stream));
    uint32_t qw[16];
    memcpy(qw, K.Qp.x.d, 32);
    memcpy(qw + 8, K.Qp.y.d, 32);
    KHTRY(upload(c, d_q, qw, 16));
    HIPCHK(c, hipEventRecord(c->ev_a.get(), c->stream));
    for (int k = 0; k < 2; k++) {
      if (!cnt[k]) continue;
      KHTRY(upload(c, d_sc[k], sc[k].data(), sc[k].size()));
      KHTRY(d_px[k].reserve(c, (size_t)cnt[k] * 8));
      KHTRY(d_py[k].reserve(c, (size_t)cnt[k] * 8));
      setup_args A;
      memset(&A, 0, sizeof A);
      A.scalars = d_sc[k].get();
      A.comb = c->d_comb.get();
      A.L = cnt[k];
      A.cx = d_px[k].get();
      A.cy = d_py[k].get();
      if (k == 1) {
        A.q = d_q.get();
        A.has_q = 1;
        A.bad = d_bad.get();
      }
      HIPCHK(c, launch_setup(A, c->stream));
    }
    kang_place_args P;
    memset(&P, 0, sizeof P);
    P.x = K.d_x.get();
    P.y = K.d_y.get();
    P.dist = K.d_dist.get();
    P.flags = K.d_unplaced.get();
    P.N = K.N;
    P.first = first + lo;
    P.n = m;
    P.tx = d_px[0].get();
    P.ty = d_py[0].get();
    P.wx = d_px[1].get();
    P.wy = d_py[1].get();
    P.n_tame = cnt[0];
    P.n_wild = cnt[1];
    P.wbad = d_bad.get();
    P.dists = d_dl.get();
    if (idx) {
      KHTRY(upload(c, d_ids, ids.data(), ids.size()));
      KHTRY(upload(c, d_rk, rank.data(), rank.size()));
      P.idx = d_ids.get();
      P.rank = d_rk.get();
    }
    HIPCHK(c, launch_kang_place(P, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_b.get(), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tm[4].add(c->ev_a.get(), c->ev_b.get(), 2, m);
  }
  return KH_OK;
}

void rec_to_dp(kh_kang_dp &o, const kang_rec &r) {
  fe x, d;
  memcpy(x.d, r.x, 32);
  memcpy(d.d, r.dist, 32);
  fe_to_be(o.x, x);
  fe_to_be(o.dist, d);
  o.index = r.index;
  o.kind = r.kind;
}

// `steps` jumps of every kangaroo in launches of steps_per_launch; the records of all of them land in
// c->kang.h_recs (at most cap, which also sizes the device buffer), *total = what the head counted.  One
// epoch per call: a kangaroo that does not move is reported by the first launch that meets it only.
int run_steps(kh_ctx *c, uint32_t steps, uint32_t cap, uint64_t *total) {
  kang_state &K = c->kang;
  *total = 0;
  K.h_recs.clear();
  if (K.no_walk || !steps) return KH_OK;
  const uint32_t T = kang_lanes(K.N);
  KHTRY(K.d_recs.reserve(c, std::max(1u, cap)));
  KHTRY(K.d_pad.reserve(c, (size_t)KH_KANG_BATCH * T * 2));
  kang_args A;
  memset(&A, 0, sizeof A);
  A.x = K.d_x.get();
  A.y = K.d_y.get();
  A.dist = K.d_dist.get();
  A.flags = K.d_unplaced.get();
  K.epoch = K.epoch >= 0x7ffffffeu ? 1 : K.epoch + 1;
  A.epoch = K.epoch;
  A.N = K.N;
  A.dp_bits = K.dp_bits;
  A.jumps = K.d_jumps.get();
  A.pad = K.d_pad.get();
  A.dp_count = K.d_count.get();
  A.dps = K.d_recs.get();
  A.dp_cap = cap;
  const uint32_t spl = launch_steps(K);
  HIPCHK(c, hipMemsetAsync(K.d_count.get(), 0, sizeof(unsigned long long), c->stream));
  uint32_t launches = 0;
  HIPCHK(c, hipEventRecord(c->ev_a.get(), c->stream));
  for (uint32_t done = 0; done < steps; done += spl, launches++) {
    A.steps = std::min(spl, steps - done);
    HIPCHK(c, launch_kang_step(A, c->stream));
  }
  HIPCHK(c, hipEventRecord(c->ev_b.get(), c->stream));
  unsigned long long cnt = 0;
  HIPCHK(c, hipMemcpyAsync(&cnt, K.d_count.get(), sizeof cnt, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->tm[8].add(c->ev_a.get(), c->ev_b.get(), launches, (uint64_t)K.N * steps);
  K.stats.jumps += (uint64_t)K.N * steps;
  *total = cnt;
  const size_t got = (size_t)std::min<unsigned long long>(cnt, cap);
  K.h_recs.resize(got);
  if (got) HIPCHK(c, hipMemcpy(K.h_recs.data(), K.d_recs.get(), got * sizeof(kang_rec), hipMemcpyDeviceToHost));
  return KH_OK;
}

// the table logic on records already in (index, dist) order; places the kangaroos to restart at the end
int add_records(kh_ctx *c, const kh_kang_dp *dps, uint32_t n) {
  kang_state &K = c->kang;
  std::vector<uint32_t> again;  // kangaroos to place afresh, in the order met
  auto restart = [&](uint32_t index) {
    if (index < K.N && std::find(again.begin(), again.end(), index) == again.end()) again.push_back(index);
  };
  for (uint32_t i = 0; i < n && !K.found; i++) {
    const kh_kang_dp &r = dps[i];
    if (std::find(again.begin(), again.end(), r.index) != again.end()) continue;  // its path has ended
    if (r.kind & KH_KANG_STALL) {
      K.stats.stalls++;
      restart(r.index);
      continue;
    }
    K.stats.dps++;
    const u256 xv = u256_from_be(r.x), dist = u256_from_be(r.dist);
    const std::array<uint64_t, 4> key = {xv.v[0], xv.v[1], xv.v[2], xv.v[3]};
    auto it = K.table.find(key);
    if (it == K.table.end()) {
      K.table.emplace(key, kang_state::entry{dist, r.index, r.kind});
      continue;
    }
    const kang_state::entry &o = it->second;
    if (o.kind != r.kind) {
      const bool r_tame = r.kind == KH_KANG_TAME;
      if (resolve(c->comb, r_tame ? dist : o.dist, r_tame ? o.dist : dist, K.a, K.Q, K.key))
        K.found = true;
      else
        K.stats.bad++;
    } else if (o.index != r.index) {
      K.stats.same_herd++;
      restart(r.index);
    }
  }
  if (again.empty() || K.found || K.no_walk || !K.N) return KH_OK;
  std::vector<u256> d(again.size());
  for (size_t i = 0; i < again.size(); i++) d[i] = seed_dist(K, again[i], ++K.gen[again[i]]);
  K.stats.reseeds += again.size();
  return place(c, again.data(), 0, (uint32_t)again.size(), d.data());
}

void sort_dps(std::vector<kh_kang_dp> &v) {
  std::sort(v.begin(), v.end(), [](const kh_kang_dp &a, const kh_kang_dp &b) {
    if (a.index != b.index) return a.index < b.index;
    return memcmp(a.dist, b.dist, 32) < 0;
  });
}

}  // namespace

extern "C" {

int kh_kang_setup(kh_ctx *ctx, const uint8_t pub_xy[64], const uint8_t start[32], const uint8_t end[32], uint32_t dp_bits,
                  const uint8_t *jumps_or_null) {
  if (!ctx || !pub_xy || !start || !end || (dp_bits > 32 && dp_bits != KH_KANG_DP_AUTO)) return KH_E_ARG;
  const u256 a = u256_from_be(start), b = u256_from_be(end);
  u256 W;
  if (u256_cmp(b, ORDER_N) >= 0 || u256_sub_raw(W, b, a) || bitlen(W) <= 16 || bitlen(W) > 192) {
    ctx->err = "kangaroo: the width must lie in [2^16, 2^192) and the range below the group order";
    return KH_E_RANGE;
  }
  ge Q;
  if (!fe_be_canonical(pub_xy, Q.x) || !fe_be_canonical(pub_xy + 32, Q.y) || !on_curve(Q.x, Q.y)) {
    ctx->err = "kangaroo: the target is not a point of the curve";
    return KH_E_ARG;
  }
  u256 jd[KH_KANG_JUMPS];
  if (jumps_or_null) {
    for (int j = 0; j < KH_KANG_JUMPS; j++) {
      jd[j] = u256_from_be(jumps_or_null + 32 * j);
      if (u256_is_zero(jd[j]) || jd[j].v[2] || jd[j].v[3]) {
        ctx->err = "kangaroo: a jump distance is 0 or not below 2^128";
        return KH_E_ARG;
      }
    }
  } else {
    default_jumps(W, jd);
  }
  (void)hipSetDevice(ctx->device);
  const uint32_t spl = ctx->kang.steps_per_launch;
  ctx->kang = kang_state();
  kang_state &K = ctx->kang;
  K.steps_per_launch = spl;
  K.a = a;
  K.W = W;
  K.Q = Q;
  K.dp_auto = dp_bits == KH_KANG_DP_AUTO;
  K.dp_bits = K.dp_auto ? 0 : dp_bits;
  for (int j = 0; j < KH_KANG_JUMPS; j++) K.jd[j] = jd[j];
  // Q' = Q - a*G
  ge aG;
  K.Qp = Q;
  if (ctx->comb.mult(aG, a)) {
    if (fe_eq(aG.x, Q.x)) {
      if (fe_eq(aG.y, Q.y)) {  // Q = a*G: the key is the range's start
        K.found = K.no_walk = true;
        K.key = a;
      } else {
        ge_double(K.Qp, Q);    // Q = -a*G
      }
    } else {
      fe_neg(aG.y, aG.y);
      ge_add(K.Qp, aG, Q);
    }
  }
  if (!K.no_walk) KHTRY(upload_jumps(ctx));
  K.ready = true;
  return KH_OK;
}

int kh_kang_jumps(kh_ctx *ctx, uint8_t out[32 * 32]) {
  if (!ctx || !out) return KH_E_ARG;
  if (!ctx->kang.ready) return KH_E_STATE;
  for (int j = 0; j < KH_KANG_JUMPS; j++) u256_to_be(out + 32 * j, ctx->kang.jd[j]);
  return KH_OK;
}

int kh_kang_geometry(kh_ctx *ctx, uint32_t *batch, uint32_t *steps_per_launch, uint32_t *herd, uint32_t *dp_bits) {
  if (!ctx) return KH_E_ARG;
  const kang_state &K = ctx->kang;
  if (batch) *batch = KH_KANG_BATCH;
  if (steps_per_launch) *steps_per_launch = launch_steps(K);
  if (herd) *herd = K.N;
  if (dp_bits) *dp_bits = K.dp_auto && !K.N ? KH_KANG_DP_AUTO : K.dp_bits;
  return KH_OK;
}

int kh_kang_set_launch(kh_ctx *ctx, uint32_t steps_per_launch) {
  if (!ctx || steps_per_launch > (1u << 20)) return KH_E_ARG;
  ctx->kang.steps_per_launch = steps_per_launch;
  return KH_OK;
}

int kh_kang_set_herd(kh_ctx *ctx, uint32_t total, uint32_t first, uint32_t n, const uint8_t *dists) {
  if (!ctx || !total || total > KANG_MAX_HERD || (uint64_t)first + n > total || (n && !dists)) return KH_E_ARG;
  kang_state &K = ctx->kang;
  if (!K.ready) return KH_E_STATE;
  std::vector<u256> d(n);
  for (uint32_t i = 0; i < n; i++) {
    d[i] = u256_from_be(dists + (size_t)i * 32);
    if (!((first + i) & 1u) && u256_is_zero(sc_reduce(d[i]))) {  // 0 or the group order: place() reduces mod n
      ctx->err = "kangaroo: a tame kangaroo at a distance of 0 mod n has no point";
      return KH_E_ARG;
    }
  }
  if (K.no_walk) return KH_OK;
  (void)hipSetDevice(ctx->device);
  ctx->cont_valid = false;
  KHTRY(resize_herd(ctx, total));
  return n ? place(ctx, nullptr, first, n, d.data()) : KH_OK;
}

int kh_kang_seed(kh_ctx *ctx, uint64_t seed, uint32_t n_kangaroos) {
  if (!ctx || n_kangaroos > KANG_MAX_HERD) return KH_E_ARG;
  kang_state &K = ctx->kang;
  if (!K.ready) return KH_E_STATE;
  K.seed = seed;
  if (K.no_walk) return KH_OK;
  (void)hipSetDevice(ctx->device);
  ctx->cont_valid = false;
  const uint32_t N = n_kangaroos ? n_kangaroos : default_herd(K.W);
  KHTRY(resize_herd(ctx, N));
  K.gen.assign(N, 0);
  K.table.clear();
  K.stats = kh_kang_stats{};
  std::vector<u256> d(N);
  parallel_for(N, host_threads(ctx), [&](uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) d[i] = seed_dist(K, (uint32_t)i, 0);
  });
  return place(ctx, nullptr, 0, N, d.data());
}

int kh_kang_step(kh_ctx *ctx, uint32_t steps, kh_kang_dp *dps, uint32_t cap, uint32_t *n_dps, uint64_t *lost) {
  if (!ctx || !n_dps || !lost || (!dps && cap)) return KH_E_ARG;
  kang_state &K = ctx->kang;
  if (!K.ready || (!K.N && !K.no_walk)) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  uint64_t total = 0;
  KHTRY(run_steps(ctx, steps, cap, &total));
  for (size_t i = 0; i < K.h_recs.size(); i++) rec_to_dp(dps[i], K.h_recs[i]);
  *n_dps = (uint32_t)K.h_recs.size();
  *lost = total > cap ? total - cap : 0;
  K.stats.lost += *lost;
  return KH_OK;
}

int kh_kang_get_herd(kh_ctx *ctx, uint32_t first, uint32_t n, uint8_t *xy, uint8_t *dist) {
  if (!ctx || !n) return KH_E_ARG;
  kang_state &K = ctx->kang;
  if (!K.ready || !K.N) return KH_E_STATE;
  if ((uint64_t)first + n > K.N) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  std::vector<uint32_t> w[3];
  const uint32_t *src[3] = {K.d_x.get(), K.d_y.get(), K.d_dist.get()};
  for (int k = 0; k < 3; k++) {
    if (k < 2 ? !xy : !dist) continue;
    w[k].resize((size_t)n * 8);
    for (int i = 0; i < 8; i++)
      HIPCHK(ctx, hipMemcpy(&w[k][(size_t)i * n], src[k] + (size_t)i * K.N + first, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  for (uint32_t e = 0; e < n; e++) {
    for (int k = 0; k < 3; k++) {
      if (w[k].empty()) continue;
      fe v;
      for (int i = 0; i < 8; i++) v.d[i] = w[k][(size_t)i * n + e];
      fe_to_be(k == 2 ? dist + 32 * (size_t)e : xy + 64 * (size_t)e + 32 * k, v);
    }
  }
  return KH_OK;
}

int kh_kang_add_dps(kh_ctx *ctx, const kh_kang_dp *dps, uint32_t n, uint8_t key[32], uint32_t *found) {
  if (!ctx || !found || !key || (!dps && n)) return KH_E_ARG;
  kang_state &K = ctx->kang;
  if (!K.ready) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  std::vector<kh_kang_dp> v(dps, dps + n);
  sort_dps(v);
  KHTRY(add_records(ctx, v.data(), n));
  *found = K.found;
  if (K.found) u256_to_be(key, K.key);
  return KH_OK;
}

int kh_kang_resolve(const uint8_t tame_dist[32], const uint8_t wild_dist[32], const uint8_t start[32],
                    const uint8_t pub_xy[64], uint8_t key[32]) {
  if (!tame_dist || !wild_dist || !start || !pub_xy || !key) return KH_E_ARG;
  ge Q;
  fe_from_be(Q.x, pub_xy);
  fe_from_be(Q.y, pub_xy + 32);
  u256 k;
  if (!resolve(host_comb(), u256_from_be(tame_dist), u256_from_be(wild_dist), u256_from_be(start), Q, k)) return 0;
  u256_to_be(key, k);
  return 1;
}

int kh_kang_solve(kh_ctx *ctx, uint64_t max_jumps, uint8_t key[32], uint32_t *found, kh_kang_stats *stats) {
  if (!ctx || !key || !found) return KH_E_ARG;
  kang_state &K = ctx->kang;
  if (!K.ready) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  if (!K.N && !K.no_walk) KHTRY(kh_kang_seed(ctx, 0, 0));
  const uint32_t spl = launch_steps(K);
  // the records a launch is expected to write, four times over: what does not fit is counted in `lost`, and a
  // stalled kangaroo whose record did not fit reports again in the next launch
  const uint64_t expect = ((uint64_t)K.N * spl) >> K.dp_bits;
  const uint32_t cap = (uint32_t)std::min<uint64_t>(1u << 24, std::max<uint64_t>(KANG_REC_CAP0, 4 * expect));
  std::vector<kh_kang_dp> v;
  for (uint64_t done = 0; !K.found && done < max_jumps; done += (uint64_t)K.N * spl) {
    uint64_t total = 0;
    KHTRY(run_steps(ctx, spl, cap, &total));
    if (total > cap) K.stats.lost += total - cap;
    v.resize(K.h_recs.size());
    for (size_t i = 0; i < v.size(); i++) rec_to_dp(v[i], K.h_recs[i]);
    sort_dps(v);
    KHTRY(add_records(ctx, v.data(), (uint32_t)v.size()));
  }
  *found = K.found;
  if (K.found) u256_to_be(key, K.key);
  if (stats) *stats = K.stats;
  return KH_OK;
}

}  // extern "C"
