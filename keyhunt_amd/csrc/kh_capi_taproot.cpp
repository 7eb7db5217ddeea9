// kh_capi_taproot.cpp -- taproot key-path targets (BIP-341 / BIP-86): the witness program of a bc1p...
// address is the x-coordinate of the tweaked key Q = lift_x(P.x) + SHA-256_TapTweak(P.x)*G, no key hash,
// so no walk can probe it directly.  A window of keys is walked with KM_DUMP into device buffers and
// k_tap_keys tweaks every point of it (kh_kernels.hip).  The reference has no such search.
#include <array>

#include "kh_ctx.h"

namespace {

// Points per window.  The walk that fills a window has one lane per 1024 points and is bound by one
// lane's latency, not by throughput: it took 2.6-2.7 ms for 2^20 points and for 2^24 alike, so the larger
// the window, the smaller its share (54 %, 27 %, 10 % of a window at 2^20, 2^22, 2^24; DESIGN.md 4 "Taproot
// targets").  2^24 points are 1 GB of X and Y and 2^14 lanes (a 256 MB inversion pad).
constexpr uint64_t TAP_WINDOW = 1ull << 24;
constexpr uint64_t TAP_WINDOW_MAX = 1ull << 24;

// k_tap_keys over the n points in d_tap_x / d_tap_y (or xs / ys); with a filter the device hits land in c->h_hits
int tap_keys(kh_ctx *c, const uint32_t *xs, const uint32_t *ys, uint32_t n, uint64_t idx0, bool probe, uint32_t *d_out8,
             uint32_t &nd) {
  nd = 0;
  KHTRY(c->d_hits.reserve(c, kh_ctx::HIT_CAP0));  // held since kh_open, unless a grow failed
  tap_keys_args A;
  memset(&A, 0, sizeof A);
  A.xs = xs;
  A.ys = ys;
  A.n = n;
  A.idx0 = idx0;
  A.comb = c->d_comb.get();
  A.tblk = probe ? c->d_tap_blk.get() : nullptr;
  A.tblocks = c->tap_blocks;
  A.out8 = d_out8;
  for (;;) {
    A.hit_count = c->d_hit_count.get();
    A.hits = c->d_hits.get();
    A.hit_cap = (uint32_t)c->d_hits.cap();
    HIPCHK(c, hipMemsetAsync(c->d_hit_count.get(), 0, 4, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_a.get(), c->stream));
    HIPCHK(c, launch_tap_keys(A, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_b.get(), c->stream));
    int r = fetch_hits(c, nd);
    c->tm[7].add(c->ev_a.get(), c->ev_b.get(), 1, n);
    if (r != KH_E_OVERFLOW) return r;
    // more filter hits than the buffer holds (a dense target set): grow it, tweak the window again
    uint32_t cnt = 0;
    HIPCHK(c, hipMemcpy(&cnt, c->d_hit_count.get(), 4, hipMemcpyDeviceToHost));
    KHTRY(grow_hits(c, cnt, 1u << 26, &c->d_hits));
  }
}

// The blocked filter of the programs' first 20 bytes, laid out as upload_tblk lays out the rows' (block
// from word 0, bits from words 1 and 2), sized like it from the reference's bloom geometry for n items
int upload_tap_blk(kh_ctx *c) {
  const uint64_t blocks = (bloom_size(bloom_entries(c->n_tap)).bits * KH_BLK_BITS_MUL + 127) / 128;
  std::vector<uint4> words(blocks, make_uint4(0, 0, 0, 0));
  for (uint64_t r = 0; r < c->n_tap; r++) {
    const uint8_t *p = &c->tap_progs[r * 32];
    uint32_t w[3];
    for (int k = 0; k < 3; k++)
      w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) |
             ((uint32_t)p[4 * k + 3] << 24);
    const uint64_t blk = ((uint64_t)w[0] * blocks) >> 32;
    uint32_t m[4];
    kh_blk_masks(w[1], w[2], m);
    words[blk].x |= m[0];
    words[blk].y |= m[1];
    words[blk].z |= m[2];
    words[blk].w |= m[3];
  }
  c->d_tap_blk.reset();
  c->tap_blocks = (uint32_t)blocks;
  return upload(c, c->d_tap_blk, words.data(), words.size());
}

}  // namespace

extern "C" {

int kh_taproot_set_targets(kh_ctx *ctx, const uint8_t *progs32, uint64_t n) {
  if (!ctx || (!progs32 && n)) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  std::vector<std::array<uint8_t, 32>> v(n);
  for (uint64_t i = 0; i < n; i++) memcpy(v[i].data(), progs32 + i * 32, 32);
  std::sort(v.begin(), v.end());  // bytewise, as memcmp orders them
  ctx->tap_progs.resize(n * 32);
  for (uint64_t i = 0; i < n; i++) memcpy(&ctx->tap_progs[i * 32], v[i].data(), 32);
  ctx->n_tap = n;
  if (!n) {
    ctx->d_tap_blk.reset();
    ctx->tap_blocks = 0;
    return KH_OK;
  }
  return upload_tap_blk(ctx);
}

int kh_taproot_set_window(kh_ctx *ctx, uint64_t points) {
  if (!ctx || points % (2 * KH_WALK_H) || points > TAP_WINDOW_MAX) return KH_E_ARG;
  ctx->tap_window = points;
  return KH_OK;
}

int kh_taproot_scan(kh_ctx *ctx, const uint8_t start[32], const uint8_t stride_be[32], uint64_t n_keys, kh_hit *hits,
                    uint32_t cap, uint32_t *n_hits) {
  const int H = KH_WALK_H;
  if (!ctx || !start || !n_hits || (!hits && cap) || n_keys == 0 || n_keys % (2 * H)) return KH_E_ARG;
  const u256 st = u256_from_be(start);
  const u256 stride = stride_be ? u256_from_be(stride_be) : u256_u64(1);
  if (u256_is_zero(stride) || u256_is_zero(st)) return KH_E_ARG;
  if (!ctx->n_tap || !ctx->d_tap_blk) return KH_E_STATE;
  // every key of the chunk is a key: below the group order as plain integers, so no lane centre and no
  // group member is the point at infinity
  if (reaches_order(st, stride, n_keys)) {
    ctx->err = "taproot scan: the chunk reaches the group order";
    return KH_E_RANGE;
  }
  (void)hipSetDevice(ctx->device);
  const uint32_t *tab = nullptr;
  KHTRY(get_table(ctx, stride, &tab, H));
  const uint64_t W = ctx->tap_window ? ctx->tap_window : TAP_WINDOW;
  const u256 lane_step = sc_mul_u128(stride, (u128)(2 * H));
  std::vector<kh_hit> out;
  ctx->tap_dev_hits = 0;
  for (uint64_t pos = 0; pos < n_keys; pos += W) {
    const uint64_t wn = std::min<uint64_t>(W, n_keys - pos);
    // one lane per 1024-point group of the window: lane g's centre is key st + (pos + 1024 g + 512) stride.
    // The walk moves the lanes, so nothing a kh_scan or a BSGS call left on them can be resumed.
    job_geom jg;
    jg.L = (uint32_t)(wn / (2 * H));
    jg.gpl = 1;
    ctx->cont_valid = false;
    KHTRY(ensure_lanes(ctx, jg.L, H));
    KHTRY(run_setup_prog(ctx, sc_add(st, sc_mul_u128(stride, (u128)pos + H)), lane_step, jg.L));
    KHTRY(ctx->d_tap_x.reserve(ctx, wn * 8));
    KHTRY(ctx->d_tap_y.reserve(ctx, wn * 8));
    walk_args A = walk_on_lanes(ctx, tab, jg, H);
    A.n_points = wn;
    A.dump_x = ctx->d_tap_x.get();
    A.dump_y = ctx->d_tap_y.get();
    KHTRY(run_walk(ctx, KM_DUMP, 0, A, jg.gpl, 4, H));
    uint32_t nd = 0;
    KHTRY(tap_keys(ctx, ctx->d_tap_x.get(), ctx->d_tap_y.get(), (uint32_t)wn, pos, true, nullptr, nd));
    ctx->tap_dev_hits += nd;
    // confirm the filter's hits: the whole 32-byte output key against the sorted programs
    std::vector<kh_dev_hit> dh(ctx->h_hits.begin(), ctx->h_hits.begin() + nd);
    std::sort(dh.begin(), dh.end(), [](const kh_dev_hit &a, const kh_dev_hit &b) { return a.idx < b.idx; });
    for (const auto &h : dh) {
      const u256 k = sc_add(st, sc_mul_u128(stride, (u128)h.idx));
      ge P;
      uint8_t q[32];
      if (!ctx->comb.mult(P, k) || !taproot_output_x(ctx->comb, P.x, P.y, q)) continue;
      if (!searchbinary(ctx->tap_progs.data(), (int64_t)ctx->n_tap, q, 32, 0)) continue;
      kh_hit o;
      memset(&o, 0, sizeof o);
      // the BIP-340 secret key of the internal key: the one whose public key has an even Y
      u256_to_be(o.key, (P.y.d[0] & 1u) ? sc_neg(k) : k);
      o.offset = h.idx;
      o.kind = KH_KIND_TAPROOT;
      o.compressed = 1;
      out.push_back(o);
    }
  }
  *n_hits = (uint32_t)out.size();
  for (uint32_t i = 0; i < out.size() && i < cap; i++) hits[i] = out[i];
  return out.size() > cap ? KH_E_OVERFLOW : KH_OK;
}

int kh_taproot_outputs(kh_ctx *ctx, const uint8_t *xy, uint32_t n, uint8_t *out32) {
  if (!ctx || !xy || !out32 || !n || n > TAP_WINDOW_MAX) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  std::vector<uint32_t> hx((size_t)n * 8), hy((size_t)n * 8);
  for (uint32_t i = 0; i < n; i++) {
    fe x, y;
    fe_from_be(x, xy + 64 * (size_t)i);
    fe_from_be(y, xy + 64 * (size_t)i + 32);
    memcpy(&hx[(size_t)i * 8], x.d, 32);
    memcpy(&hy[(size_t)i * 8], y.d, 32);
  }
  dev_buf<uint32_t> dx, dy, dout;
  KHTRY(upload(ctx, dx, hx.data(), hx.size()));
  KHTRY(upload(ctx, dy, hy.data(), hy.size()));
  KHTRY(dout.reserve(ctx, (size_t)n * 8));
  // a point the kernel skips (t >= n) leaves its 32 bytes zero
  HIPCHK(ctx, hipMemset(dout.get(), 0, (size_t)n * 32));
  uint32_t nd = 0;
  KHTRY(tap_keys(ctx, dx.get(), dy.get(), n, 0, false, dout.get(), nd));
  return download(ctx, (uint32_t *)out32, dout, (size_t)n * 8);
}

int kh_taproot_stats(kh_ctx *ctx, uint32_t *batch, uint32_t *device_hits) {
  if (!ctx) return KH_E_ARG;
  if (batch) *batch = KH_TAP_BATCH;
  if (device_hits) *device_hits = ctx->tap_dev_hits;
  return KH_OK;
}

}  // extern "C"
