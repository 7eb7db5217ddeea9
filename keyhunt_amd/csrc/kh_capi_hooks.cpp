// kh_capi_hooks.cpp -- measurement, parity and test hooks of include/kh_gpu.h.
#include "kh_ctx.h"

namespace {

// the shape of the kernel hooks: launch(dout) starts one test kernel that writes n elements; wait
// for it and fetch them.  The hook's inputs are owners of its own, uploaded before.
template <class T, class L>
int run_test(kh_ctx *ctx, T *out, size_t n, L launch) {
  dev_buf<T> dout;
  KHTRY(dout.reserve(ctx, n));
  HIPCHK(ctx, launch(dout.get()));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return download(ctx, out, dout, n);
}

// n big-endian field elements at a + i*stride as device limbs
std::vector<uint32_t> fe_words(const uint8_t *a, size_t stride, uint32_t n) {
  std::vector<uint32_t> h((size_t)n * 8);
  for (uint32_t i = 0; i < n; i++) {
    fe x;
    fe_from_be(x, a + stride * i);
    memcpy(&h[(size_t)i * 8], x.d, 32);
  }
  return h;
}

// a kernel over n pairs of field elements that writes `words` words per pair
typedef hipError_t (*pair_kernel)(const uint32_t *, const uint32_t *, uint32_t, uint32_t *, hipStream_t);
int run_pairs(kh_ctx *ctx, const std::vector<uint32_t> &ha, const std::vector<uint32_t> &hb, uint32_t n,
              std::vector<uint32_t> &ho, pair_kernel launch) {
  dev_buf<uint32_t> da, db;
  KHTRY(upload(ctx, da, ha.data(), ha.size()));
  KHTRY(upload(ctx, db, hb.data(), hb.size()));
  return run_test(ctx, ho.data(), ho.size(),
                  [&](uint32_t *dout) { return launch(da.get(), db.get(), n, dout, ctx->stream); });
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------------------------
int kh_bloom_add(uint8_t *bf, uint64_t bits, uint32_t hashes, const uint8_t *items, uint64_t n, uint32_t len) {
  if (!bf || !bits || (!items && n) || !len || len > 32 || (len > 20 && len != 32)) return KH_E_ARG;
  bloom_desc d;
  memset(&d, 0, sizeof d);
  d.bits = bits;
  d.hashes = hashes;
  for (uint64_t i = 0; i < n; i++) host_bloom_add(bf, d, items + i * len, (int)len);
  return KH_OK;
}

int kh_bsgs_layer_bits(kh_ctx *ctx, uint32_t layer, uint64_t bits, uint32_t hashes, uint64_t bytes, uint8_t *shards) {
  if (!ctx || layer < 1 || layer > 3 || !bits || !bytes || !shards || bits > bytes * 8) return KH_E_ARG;
  if (!ctx->bsgs_built) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  const kh_bsgs_info &I = ctx->info;
  const uint64_t count = layer == 1 ? I.m : layer == 2 ? I.m2 : I.m3;
  bloom_desc d;
  memset(&d, 0, sizeof d);
  d.bits = bits;
  d.bytes = bytes;
  d.stride = (bytes + 255) / 256 * 256;
  d.recip = ~0ULL / bits;
  d.hashes = hashes;
  std::vector<uint8_t> h(256 * d.stride, 0);
  for (int i = 0; i < 256; i++) memcpy(&h[(size_t)i * d.stride], shards + (size_t)i * bytes, bytes);
  dev_buf<uint8_t> dev;
  KHTRY(dev.reserve(ctx, h.size() + 4));
  HIPCHK(ctx, hipMemcpy(dev.get(), h.data(), h.size(), hipMemcpyHostToDevice));
  KHTRY(build_walk(ctx, KM_BUILD, dev.get(), d, nullptr, nullptr, count, true));
  KHTRY(download(ctx, h.data(), dev, h.size()));
  for (int i = 0; i < 256; i++) memcpy(shards + (size_t)i * bytes, &h[(size_t)i * d.stride], bytes);
  return KH_OK;
}

int kh_bsgs_table_rows(kh_ctx *ctx, const uint8_t **rows, uint64_t *n_rows) {
  if (!ctx || !rows || !n_rows) return KH_E_ARG;
  if (!ctx->bsgs_built) return KH_E_STATE;
  *rows = ctx->h_rows.data();
  *n_rows = ctx->h_rows.size() / 16;
  return KH_OK;
}

int kh_bsgs_set_base_check(kh_ctx *ctx, int enable) {
  if (!ctx) return KH_E_ARG;
  ctx->base_check = enable != 0;
  return KH_OK;
}

int kh_bsgs_log_candidates(kh_ctx *ctx, int enable) {
  if (!ctx) return KH_E_ARG;
  ctx->log_cands = enable != 0;
  ctx->cand_log_base.clear();
  ctx->cand_log_a.clear();
  ctx->cand_log_mask.clear();
  return KH_OK;
}

int kh_bsgs_get_candidates(kh_ctx *ctx, uint64_t *base_index, uint32_t *a, uint32_t *mask, uint64_t cap,
                           uint64_t *n) {
  if (!ctx || !n) return KH_E_ARG;
  *n = ctx->cand_log_base.size();
  for (uint64_t i = 0; i < *n && i < cap; i++) {
    if (base_index) base_index[i] = ctx->cand_log_base[i];
    if (a) a[i] = ctx->cand_log_a[i];
    if (mask) mask[i] = ctx->cand_log_mask[i];
  }
  return *n > cap ? KH_E_OVERFLOW : KH_OK;
}

int kh_bsgs_second_masks(kh_ctx *ctx, uint32_t target, const uint8_t *base_keys, uint32_t n, uint32_t *gpu_mask,
                         uint32_t *host_mask) {
  if (!ctx || !base_keys || !gpu_mask || !host_mask) return KH_E_ARG;
  if (!ctx->bsgs_built || target >= ctx->targets.size()) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  if (n == 0) return KH_OK;
  const ge &Q = ctx->targets[target];
  std::vector<uint32_t> lw((size_t)n * 8);
  std::vector<kh_dev_hit> c(n);
  for (uint32_t j = 0; j < n; j++) {
    u256 k = sc_reduce(u256_from_be(base_keys + (size_t)j * 32));
    u256_to_limbs(&lw[(size_t)j * 8], k);
    c[j].idx = j;  // list mode with one point per base: t = j -> base j, a = 0
    c[j].kind = 4;
    c[j].aux = 0xFFFFFFFFu;
    host_mask[j] = second_mask(ctx, k, Q);
  }
  uint32_t Qw[16];
  memcpy(Qw, Q.x.d, 32);
  memcpy(Qw + 8, Q.y.d, 32);
  dev_buf<uint32_t> d_list, d_q, d_cnt;
  dev_buf<kh_dev_hit> d_c;
  KHTRY(upload(ctx, d_list, lw.data(), lw.size()));
  KHTRY(upload(ctx, d_q, Qw, 16));
  KHTRY(upload(ctx, d_cnt, &n, 1));
  KHTRY(upload(ctx, d_c, c.data(), n));
  refine_args Ra;
  memset(&Ra, 0, sizeof Ra);
  Ra.cands = d_c.get();
  Ra.count = d_cnt.get();
  Ra.cap = n;
  Ra.list_mode = 1;
  Ra.a_pts = 1;
  Ra.two_n = 2 * ctx->info.n;
  Ra.two_m = 2 * ctx->info.m;
  Ra.start = ctx->d_ref_start.get();
  Ra.list = d_list.get();
  Ra.comb = ctx->d_comb.get();
  Ra.q = d_q.get();
  Ra.amp2 = ctx->d_amp2.get();
  Ra.bloom2 = ctx->d_bl[1].get();
  Ra.bd2 = ctx->bd[1];
  HIPCHK(ctx, launch_refine(Ra, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  KHTRY(download(ctx, c.data(), d_c, n));
  for (uint32_t j = 0; j < n; j++) gpu_mask[j] = c[j].aux;
  return KH_OK;
}

// kh_bsgs_second_masks over k_refine's own index arithmetic: candidate j has giant index t = t_round +
// idx[j], base b = t / a_pts and a = t % a_pts, and its base key is base(b) + a*2M with base(b) =
// start + b*two_n (list == null) or list[b].  Every b is checked against n_bases before the launch.
int kh_bsgs_refine_masks(kh_ctx *ctx, uint32_t target, const uint8_t start[32], const uint8_t *list, uint64_t n_bases,
                         uint64_t t_round, uint64_t a_pts, uint64_t two_n, uint64_t two_m_raw, const uint64_t *idx,
                         uint32_t n, uint32_t *gpu_mask, uint32_t *host_mask) {
  if (!ctx || (!start && !list) || !idx || !gpu_mask || !host_mask || !a_pts || (list && !n_bases)) return KH_E_ARG;
  if (!ctx->bsgs_built || target >= ctx->targets.size()) return KH_E_STATE;
  if (n == 0) return KH_OK;
  (void)hipSetDevice(ctx->device);
  const ge &Q = ctx->targets[target];
  const uint64_t two_m = two_m_raw ? two_m_raw : 2 * ctx->info.m;
  // the bases go to the device as given; the kernel's sum is right mod n for any 256-bit base, since base
  // + offset < 2^256 + 2^129 < 2n (the engine itself sends reduced ones)
  const u256 st = start ? u256_from_be(start) : u256{};
  std::vector<uint32_t> lw;
  if (list) {
    lw.resize((size_t)n_bases * 8);
    for (uint64_t b = 0; b < n_bases; b++) u256_to_limbs(&lw[(size_t)b * 8], u256_from_be(list + b * 32));
  }
  std::vector<kh_dev_hit> c(n);
  for (uint32_t j = 0; j < n; j++) {
    const u128 t = (u128)t_round + idx[j];
    if (t >> 64) return KH_E_ARG;  // the kernel's 64-bit sum would wrap
    const uint64_t b = (uint64_t)t / a_pts, a = (uint64_t)t % a_pts;
    if (list && b >= n_bases) {
      ctx->err = "kh_bsgs_refine_masks: candidate " + std::to_string(j) + " lies in base " + std::to_string(b) +
                 " of " + std::to_string(n_bases);
      return KH_E_ARG;
    }
    u256 k;
    if (list) {
      memcpy(&k, &lw[(size_t)b * 8], 32);  // 8 LE u32 limbs = 4 LE u64 limbs
      k = sc_reduce(k);
    } else {
      k = sc_add(sc_reduce(st), sc_reduce(u256_from_u128((u128)b * two_n)));
    }
    k = sc_add(k, sc_reduce(u256_from_u128((u128)a * two_m)));
    c[j].idx = idx[j];
    c[j].kind = 4;
    c[j].aux = 0xFFFFFFFFu;
    host_mask[j] = second_mask(ctx, k, Q);
  }
  uint32_t Qw[16], sw[8];
  memcpy(Qw, Q.x.d, 32);
  memcpy(Qw + 8, Q.y.d, 32);
  u256_to_limbs(sw, st);
  dev_buf<uint32_t> d_list, d_start, d_q, d_cnt;
  dev_buf<kh_dev_hit> d_c;
  if (list) KHTRY(upload(ctx, d_list, lw.data(), lw.size()));
  KHTRY(upload(ctx, d_start, sw, 8));
  KHTRY(upload(ctx, d_q, Qw, 16));
  KHTRY(upload(ctx, d_cnt, &n, 1));
  KHTRY(upload(ctx, d_c, c.data(), n));
  refine_args Ra;
  memset(&Ra, 0, sizeof Ra);
  Ra.cands = d_c.get();
  Ra.count = d_cnt.get();
  Ra.cap = n;
  Ra.list_mode = list ? 1 : 0;
  Ra.t_round = t_round;
  Ra.a_pts = a_pts;
  Ra.two_n = two_n;
  Ra.two_m = two_m;
  Ra.start = d_start.get();
  Ra.list = d_list.get();
  Ra.comb = ctx->d_comb.get();
  Ra.q = d_q.get();
  Ra.amp2 = ctx->d_amp2.get();
  Ra.bloom2 = ctx->d_bl[1].get();
  Ra.bd2 = ctx->bd[1];
  HIPCHK(ctx, launch_refine(Ra, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  KHTRY(download(ctx, c.data(), d_c, n));
  for (uint32_t j = 0; j < n; j++) gpu_mask[j] = c[j].aux;
  return KH_OK;
}

int kh_kernel_time(kh_ctx *ctx, uint32_t kind, uint64_t *launches, double *ms, uint64_t *points) {
  if (!ctx || kind > 8) return KH_E_ARG;
  if (launches) *launches = ctx->tm[kind].launches;
  if (ms) *ms = ctx->tm[kind].ms;
  if (points) *points = ctx->tm[kind].points;
  return KH_OK;
}

int kh_kernel_time_reset(kh_ctx *ctx) {
  if (!ctx) return KH_E_ARG;
  for (auto &t : ctx->tm) t = timing();
  return KH_OK;
}

// ---------------------------------------------------------------------------------------------
// parity hooks
// ---------------------------------------------------------------------------------------------
int kh_pubkeys(kh_ctx *ctx, const uint8_t *scalars, uint32_t n, uint8_t *xy) {
  if (!ctx || !scalars || !xy || !n) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  std::vector<u256> s(n);
  for (uint32_t i = 0; i < n; i++) {
    s[i] = sc_reduce(u256_from_be(scalars + 32 * i));
    if (u256_is_zero(s[i])) return KH_E_ARG;
  }
  KHTRY(run_setup(ctx, s, nullptr));
  std::vector<uint32_t> cx((size_t)n * 8), cy((size_t)n * 8);
  for (int w = 0; w < 8; w++) {
    HIPCHK(ctx, hipMemcpy(&cx[(size_t)w * n], ctx->d_cx.get() + (size_t)w * n, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(&cy[(size_t)w * n], ctx->d_cy.get() + (size_t)w * n, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  for (uint32_t i = 0; i < n; i++) {
    fe x, y;
    for (int w = 0; w < 8; w++) {
      x.d[w] = cx[(size_t)w * n + i];
      y.d[w] = cy[(size_t)w * n + i];
    }
    fe_to_be(xy + 64 * i, x);
    fe_to_be(xy + 64 * i + 32, y);
  }
  return KH_OK;
}

// k_setup on buffers of the hook's own: the context's lanes, pad and kept state are not touched.  Every
// index the kernel forms is checked here first: scalars and centres hold L entries, and the list form
// reads base (t_round + g*lane_pts) / a_pts for g < L, the largest at g = L - 1.
int kh_setup_centres(kh_ctx *ctx, const kh_setup_form *f, const uint8_t *q, uint8_t *xy) {
  if (!ctx || !f || !xy || !f->L || f->L > (1u << 22) || f->prog > 2) return KH_E_ARG;
  const uint32_t L = f->L;
  std::vector<uint32_t> up;  // prog 0: the scalars; prog 2: the list
  setup_args A;
  memset(&A, 0, sizeof A);
  u256 st{};
  if (f->prog == 0) {
    if (!f->scalars) return KH_E_ARG;
    up.resize((size_t)L * 8);
    for (uint32_t g = 0; g < L; g++) {
      const u256 k = sc_reduce(u256_from_be(f->scalars + (size_t)g * 32));
      if (u256_is_zero(k)) return KH_E_ARG;
      u256_to_limbs(&up[(size_t)g * 8], k);
    }
  } else if (f->prog == 1) {
    u256_to_limbs(A.s0, sc_reduce(u256_from_be(f->s0)));
    u256_to_limbs(A.step, sc_reduce(u256_from_be(f->step)));
  } else {
    // 2*(a0 + h) + 1 with a0 < a_pts must fit 64 bits, and so must the last lane's giant index
    if (!f->lane_pts || !f->a_pts || !f->m || f->a_pts >> 61 || (f->list && !f->n_bases)) return KH_E_ARG;
    const u128 t_last = (u128)f->t_round + (u128)(L - 1) * f->lane_pts;
    if (t_last >> 64) return KH_E_ARG;
    if (f->list && (uint64_t)t_last / f->a_pts >= f->n_bases) {
      ctx->err = "kh_setup_centres: the last lane lies in base " + std::to_string((uint64_t)t_last / f->a_pts) +
                 " of " + std::to_string(f->n_bases);
      return KH_E_ARG;
    }
    // the bases go to the device as given: the kernel's sum is right mod n for any 256-bit base, since
    // base + offset < 2^256 + 2^129 < 2n (the engine itself sends reduced ones)
    st = u256_from_be(f->start);
    if (f->list) {
      up.resize((size_t)f->n_bases * 8);
      for (uint64_t b = 0; b < f->n_bases; b++) u256_to_limbs(&up[(size_t)b * 8], u256_from_be(f->list + b * 32));
    }
    // a centre key of 0 mod n has no point (the engine keeps such rounds on the host)
    for (uint32_t g = 0; g < L; g++) {
      const uint64_t t0 = f->t_round + (uint64_t)g * f->lane_pts, b = t0 / f->a_pts, a0 = t0 % f->a_pts;
      u256 k;
      if (f->list) {
        memcpy(&k, &up[(size_t)b * 8], 32);  // 8 LE u32 limbs = 4 LE u64 limbs
        k = sc_reduce(k);
      } else {
        k = sc_add(sc_reduce(st), sc_reduce(u256_from_u128((u128)b * f->two_n)));
      }
      k = sc_add(k, sc_reduce(u256_from_u128((u128)f->m * (2 * (a0 + f->h) + 1))));
      if (u256_is_zero(k)) {
        ctx->err = "kh_setup_centres: lane " + std::to_string(g) + " has centre key 0 mod n";
        return KH_E_ARG;
      }
    }
  }
  (void)hipSetDevice(ctx->device);
  dev_buf<uint32_t> d_up, d_start, d_q, d_zero, d_cx, d_cy;
  if (!up.empty()) KHTRY(upload(ctx, d_up, up.data(), up.size()));
  KHTRY(d_cx.reserve(ctx, (size_t)L * 8));
  KHTRY(d_cy.reserve(ctx, (size_t)L * 8));
  A.comb = ctx->d_comb.get();
  A.L = L;
  A.cx = d_cx.get();
  A.cy = d_cy.get();
  A.prog = f->prog;
  if (f->prog == 0) A.scalars = d_up.get();
  if (f->prog == 1) {
    const uint32_t zero = 0;
    KHTRY(upload(ctx, d_zero, &zero, 1));
    A.zero_flag = d_zero.get();
  }
  if (f->prog == 2) {
    uint32_t sw[8];
    u256_to_limbs(sw, st);
    KHTRY(upload(ctx, d_start, sw, 8));
    A.start = d_start.get();
    A.list = f->list ? d_up.get() : nullptr;
    A.t_round = f->t_round;
    A.lane_pts = f->lane_pts;
    A.a_pts = f->a_pts;
    A.two_n = f->two_n;
    A.m = f->m;
    A.h = f->h;
  }
  if (q) {
    uint32_t Qw[16];
    fe x, y;
    fe_from_be(x, q);
    fe_from_be(y, q + 32);
    memcpy(Qw, x.d, 32);
    memcpy(Qw + 8, y.d, 32);
    KHTRY(upload(ctx, d_q, Qw, 16));
    A.q = d_q.get();
    A.has_q = 1;
  }
  HIPCHK(ctx, launch_setup(A, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (f->prog == 1) {
    uint32_t zero = 0;
    KHTRY(download(ctx, &zero, d_zero, 1));
    if (zero) {
      ctx->err = "lane centre scalar is 0 mod n";
      return KH_E_ARG;
    }
  }
  std::vector<uint32_t> cx((size_t)L * 8), cy((size_t)L * 8);
  KHTRY(download(ctx, cx.data(), d_cx, cx.size()));
  KHTRY(download(ctx, cy.data(), d_cy, cy.size()));
  for (uint32_t i = 0; i < L; i++) {
    fe x, y;
    for (int w = 0; w < 8; w++) {
      x.d[w] = cx[(size_t)w * L + i];
      y.d[w] = cy[(size_t)w * L + i];
    }
    fe_to_be(xy + 64 * (size_t)i, x);
    fe_to_be(xy + 64 * (size_t)i + 32, y);
  }
  return KH_OK;
}

int kh_walk_points(kh_ctx *ctx, const uint8_t start[32], const uint8_t stride_be[32], uint64_t n_points,
                   uint8_t *out_x, uint8_t *out_y) {
  if (!ctx || !start || !out_x || !n_points || n_points % (2 * KH_WALK_H)) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  const int H = KH_WALK_H;
  u256 st = sc_reduce(u256_from_be(start));
  u256 stride = stride_be ? sc_reduce(u256_from_be(stride_be)) : u256_u64(1);
  const uint32_t *tab = nullptr;
  KHTRY(get_table(ctx, stride, &tab));
  job_geom jg = plan(ctx, n_points / (2 * H), 0);
  std::vector<u256> s(jg.L);
  for (uint32_t g = 0; g < jg.L; g++) s[g] = sc_add(st, sc_mul_u128(stride, (u128)g * jg.gpl * 2 * H + H));
  KHTRY(run_setup(ctx, s, nullptr));
  dev_buf<uint32_t> dx, dy;
  KHTRY(dx.reserve(ctx, n_points * 8));
  if (out_y) KHTRY(dy.reserve(ctx, n_points * 8));
  walk_args A = walk_on_lanes(ctx, tab, jg, H);
  A.n_points = n_points;
  A.dump_x = dx.get();
  A.dump_y = dy.get();
  KHTRY(run_walk(ctx, KM_DUMP, 0, A, jg.gpl, 4));
  std::vector<uint32_t> hx(n_points * 8), hy(out_y ? n_points * 8 : 0);
  KHTRY(download(ctx, hx.data(), dx, hx.size()));
  if (out_y) KHTRY(download(ctx, hy.data(), dy, hy.size()));
  for (uint64_t i = 0; i < n_points; i++) {
    fe x;
    memcpy(x.d, &hx[i * 8], 32);
    fe_to_be(out_x + 32 * i, x);
    if (out_y) {
      fe y;
      memcpy(y.d, &hy[i * 8], 32);
      fe_to_be(out_y + 32 * i, y);
    }
  }
  return KH_OK;
}

int kh_hash160(kh_ctx *ctx, const uint8_t *xy, uint32_t n, uint8_t *out60) {
  if (!ctx || !xy || !out60 || !n) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  std::vector<uint32_t> ho((size_t)n * 15);
  KHTRY(run_pairs(ctx, fe_words(xy, 64, n), fe_words(xy + 32, 64, n), n, ho, launch_test_hash160));
  memcpy(out60, ho.data(), (size_t)n * 60);
  return KH_OK;
}

int kh_field_ops(kh_ctx *ctx, const uint8_t *a, const uint8_t *b, uint32_t n, uint8_t *out160) {
  if (!ctx || !a || !b || !out160 || !n) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  std::vector<uint32_t> ho((size_t)n * 40);
  KHTRY(run_pairs(ctx, fe_words(a, 32, n), fe_words(b, 32, n), n, ho, launch_test_field));
  for (uint32_t i = 0; i < n; i++)
    for (int k = 0; k < 5; k++) {
      fe r;
      memcpy(r.d, &ho[(size_t)i * 40 + 8 * k], 32);
      fe_to_be(out160 + 160 * i + 32 * k, r);
    }
  return KH_OK;
}

int kh_digests(kh_ctx *ctx, const uint8_t *xy, uint32_t n, uint8_t *out80) {
  if (!ctx || !xy || !out80 || !n) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  std::vector<uint32_t> ho((size_t)n * 20);
  KHTRY(run_pairs(ctx, fe_words(xy, 64, n), fe_words(xy + 32, 64, n), n, ho, launch_test_digests));
  memcpy(out80, ho.data(), (size_t)n * 80);
  return KH_OK;
}

int kh_digests_nested(kh_ctx *ctx, const uint8_t *xy, uint32_t n, uint8_t *out40) {
  if (!ctx || !xy || !out40 || !n) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  std::vector<uint32_t> ho((size_t)n * 10);
  KHTRY(run_pairs(ctx, fe_words(xy, 64, n), fe_words(xy + 32, 64, n), n, ho, launch_test_digests_nested));
  memcpy(out40, ho.data(), (size_t)n * 40);
  return KH_OK;
}

int kh_filter_keys(kh_ctx *ctx, const uint8_t *items, uint32_t n, uint32_t len, uint64_t *ab) {
  if (!ctx || !items || !ab || !n || len == 0 || len > 20) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  dev_buf<uint8_t> ditems;
  KHTRY(upload(ctx, ditems, items, (size_t)n * 20));
  return run_test(ctx, ab, (size_t)n * 2, [&](uint64_t *dout) {
    return launch_test_filter_keys(ditems.get(), n, len, dout, ctx->stream);
  });
}

int kh_tblk_check(kh_ctx *ctx, const uint8_t *items, uint32_t n, uint8_t *out) {
  if (!ctx || !items || !out || !n) return KH_E_ARG;
  if (ctx->vanity || !ctx->d_tblk || !ctx->tblocks) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  dev_buf<uint8_t> ditems;
  KHTRY(upload(ctx, ditems, items, (size_t)n * 20));
  std::vector<uint32_t> ho(n);
  KHTRY(run_test(ctx, ho.data(), ho.size(), [&](uint32_t *dout) {
    return launch_test_tblk(ditems.get(), n, ctx->d_tblk.get(), ctx->tblocks, dout, ctx->stream);
  }));
  for (uint32_t i = 0; i < n; i++) out[i] = (uint8_t)ho[i];
  return KH_OK;
}

int kh_scan_device_hits(kh_ctx *ctx, uint32_t *device_hits, uint32_t *redos) {
  if (!ctx || !device_hits || !redos) return KH_E_ARG;
  *device_hits = ctx->scan_dev_hits;
  *redos = ctx->scan_redos;
  return KH_OK;
}

int kh_bloom_check(kh_ctx *ctx, uint32_t layer, const uint8_t *items, uint32_t n, uint32_t len, uint8_t *out) {
  return kh_bloom_check2(ctx, layer, items, n, len, out, nullptr);
}

int kh_bloom_check2(kh_ctx *ctx, uint32_t layer, const uint8_t *items, uint32_t n, uint32_t len, uint8_t *out,
                    uint8_t *out_lazy) {
  if (!ctx || !items || !out || !n || layer > 3) return KH_E_ARG;
  // a prefix length (1..19) keys the target bloom only (vanity); the BSGS layers hold 32-byte X's or 20
  if (len != 20 && len != 32 && !(layer == 0 && len >= 1 && len < 20)) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  const size_t item_bytes = len == 32 ? 32 : 20;
  const uint8_t *bl;
  bloom_desc d;
  if (layer == 0) {
    if (!ctx->d_tbloom) return KH_E_STATE;
    bl = ctx->d_tbloom.get();
    d = ctx->tbd;
  } else {
    if (!ctx->bsgs_ready) return KH_E_STATE;
    bl = ctx->d_bl[layer - 1].get();
    d = ctx->bd[layer - 1];
  }
  uint32_t blocked = (layer == 1 && ctx->info.layer1_layout == KH_LAYER1_BLOCKED) ? 1 : 0;
  if (blocked && len != 32) return KH_E_ARG;  // the blocked layer reads X[8..24)
  dev_buf<uint8_t> ditems;
  KHTRY(upload(ctx, ditems, items, (size_t)n * item_bytes));
  std::vector<uint32_t> ho((size_t)n * 2, 0);  // n eager answers, then n lazy ones
  KHTRY(run_test(ctx, ho.data(), ho.size(), [&](uint32_t *dout) {
    return launch_test_bloom(ditems.get(), n, len, bl, d, layer ? 1 : 0, blocked, dout, out_lazy ? dout + n : nullptr,
                             ctx->stream);
  }));
  for (uint32_t i = 0; i < n; i++) out[i] = (uint8_t)ho[i];
  if (out_lazy)
    for (uint32_t i = 0; i < n; i++) out_lazy[i] = (uint8_t)ho[(size_t)n + i];
  return KH_OK;
}

int kh_get_bloom(kh_ctx *ctx, uint32_t layer, uint8_t *buf, uint64_t cap, uint64_t *bytes) {
  if (!ctx || layer > 3 || !bytes) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  if (layer == 0) {
    if (!ctx->d_tbloom) return KH_E_STATE;
    *bytes = ctx->tbd.bytes;
    if (!buf) return KH_OK;
    if (cap < ctx->tbd.bytes) return KH_E_OVERFLOW;
    return download(ctx, buf, ctx->d_tbloom, ctx->tbd.bytes);
  }
  if (!ctx->bsgs_ready) return KH_E_STATE;
  const bloom_desc &d = ctx->bd[layer - 1];
  *bytes = 256 * d.bytes;
  if (!buf) return KH_OK;
  if (cap < 256 * d.bytes) return KH_E_OVERFLOW;
  HIPCHK(ctx, hipMemcpy2D(buf, d.bytes, ctx->d_bl[layer - 1].get(), d.stride, d.bytes, 256, hipMemcpyDeviceToHost));
  return KH_OK;
}

// kh_get_bloom's counterpart for BSGS layers 1 and 2: the caller's 256 unpadded shards onto the device
// layer at its stride (layer 1: in the layout kh_bsgs_setup chose).  The lanes a scan kept stay valid
// (they do not depend on the layers).  The host holds no copy of layer 1; its copy of layer 2, which
// second_mask reads, is replaced with the device's.  kh_bsgs_save would write these bits (or rebuild a
// blocked layer 1), so it refuses until the next kh_bsgs_build / _load.
int kh_bsgs_set_bloom(kh_ctx *ctx, uint32_t layer, const uint8_t *buf, uint64_t bytes) {
  if (!ctx || !buf) return KH_E_ARG;
  if (!ctx->bsgs_built) return KH_E_STATE;
  if (layer != 1 && layer != 2) {
    ctx->err = "kh_bsgs_set_bloom takes layer 1 or 2";
    return KH_E_ARG;
  }
  const bloom_desc &d = ctx->bd[layer - 1];
  if (bytes != 256 * d.bytes) {
    ctx->err = "kh_bsgs_set_bloom takes kh_get_bloom's byte count (" + std::to_string(256 * d.bytes) + ")";
    return KH_E_ARG;
  }
  (void)hipSetDevice(ctx->device);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->side) HIPCHK(ctx, hipStreamSynchronize(ctx->side));
  HIPCHK(ctx, hipMemcpy2D(ctx->d_bl[layer - 1].get(), d.stride, buf, d.bytes, d.bytes, 256, hipMemcpyHostToDevice));
  if (layer == 2) {
    std::vector<uint8_t> &h = ctx->h_bl[1];
    h.assign(256 * d.stride, 0);
    for (int i = 0; i < 256; i++) memcpy(&h[(size_t)i * d.stride], buf + (size_t)i * d.bytes, d.bytes);
  }
  ctx->layer_replaced = true;
  return KH_OK;
}

int kh_get_bsgs_table(kh_ctx *ctx, uint8_t *buf, uint64_t cap_rows, uint64_t *rows) {
  if (!ctx || !rows) return KH_E_ARG;
  if (!ctx->bsgs_built) return KH_E_STATE;
  *rows = ctx->info.m3;
  if (!buf) return KH_OK;
  if (cap_rows < ctx->info.m3) return KH_E_OVERFLOW;
  memcpy(buf, ctx->h_rows.data(), ctx->h_rows.size());
  return KH_OK;
}

// --load-ptable (keyhunt.cpp:1871-1892): the rows come from the caller's file, as the reference's
// mapping of that file replaces the table thread_bPload would have written (5404, 5587).  Like
// the reference, the rows are taken as they are: neither checked nor re-sorted.
int kh_bsgs_set_table(kh_ctx *ctx, const uint8_t *rows, uint64_t n_rows) {
  if (!ctx || !rows) return KH_E_ARG;
  if (!ctx->bsgs_built) return KH_E_STATE;
  if (n_rows != ctx->info.m3) {
    ctx->err = "bP table rows " + std::to_string(n_rows) + " != M3 " + std::to_string(ctx->info.m3);
    return KH_E_ARG;
  }
  ctx->h_rows.assign(rows, rows + n_rows * 16);
  return KH_OK;
}

}  // extern "C"
