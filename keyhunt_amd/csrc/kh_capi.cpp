// kh_capi.cpp -- implementation of include/kh_gpu.h: the context, the shared launch helpers, targets,
// kh_scan and the target files.  (BSGS: kh_capi_bsgs.cpp; minikeys: kh_capi_minikeys.cpp; taproot
// targets: kh_capi_taproot.cpp; parity hooks and timing: kh_capi_hooks.cpp.)
//
// Host side of the MI355X engine: device memory layout, lane partitioning, launches, the
// reference-exact host steps around the kernels (bloom sizing, table sort + searchbinary,
// compressed-key parity fix-up, BSGS second/third check), and event timing.  Every scan and
// build runs on the GPU kernels in kh_kernels.hip; there is no CPU fallback.
#include <array>

#include "kh_ctx.h"

int kh::hip_fail(kh_ctx *c, const char *what, hipError_t e) {
  c->err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? KH_E_NOMEM : KH_E_HIP;
}

kh_ctx::~kh_ctx() {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  if (side) {
    (void)hipStreamSynchronize(side);
    (void)hipStreamDestroy(side);
  }
  if (stream) (void)hipStreamDestroy(stream);
}

namespace kh_host {

int ensure_lanes(kh_ctx *c, uint32_t L, int H) {
  if (L <= c->lanes_alloc() && H <= c->scratch_h()) return KH_OK;
  L = std::max(L, c->lanes_alloc());
  H = std::max(H, c->scratch_h());
  c->cont_valid = false;
  c->release_lanes();
  int r = c->d_cx.reserve(c, (size_t)L * 8);
  if (!r) r = c->d_cy.reserve(c, (size_t)L * 8);
  if (!r) r = c->d_scalars.reserve(c, (size_t)L * 8);
  if (!r) r = c->d_scratch.reserve(c, (size_t)L * H * 2);
  if (r) c->release_lanes();
  return r;
}

int get_table(kh_ctx *c, const u256 &d, const uint32_t **out, const int H, uint64_t jump) {
  uint8_t be[32];
  u256_to_be(be, d);
  std::string key((const char *)be, 32);
  key += std::to_string(H) + "/" + std::to_string(jump);
  for (auto &t : c->tables)
    if (t.first == key) {
      *out = t.second.get();
      return KH_OK;
    }
  std::vector<uint32_t> h((size_t)(H + 1) * 16);
  ge D;
  if (!c->comb.mult(D, d)) {
    c->err = "delta scalar is 0";
    return KH_E_ARG;
  }
  ge cur = D;
  for (int i = 0; i < H; i++) {
    if (i == 1) ge_double(cur, D);
    if (i >= 2) ge_add(cur, cur, D);
    memcpy(&h[(size_t)i * 16], cur.x.d, 32);
    memcpy(&h[(size_t)i * 16 + 8], cur.y.d, 32);
  }
  ge d2;
  if (jump == 1) {
    ge_double(d2, cur);  // 2H * D
  } else if (!c->comb.mult(d2, sc_mul_u128(d, (u128)jump * 2 * (uint64_t)H))) {  // (jump * 2H) * d mod n
    c->err = "group jump scalar is 0";
    return KH_E_ARG;
  }
  memcpy(&h[(size_t)H * 16], d2.x.d, 32);
  memcpy(&h[(size_t)H * 16 + 8], d2.y.d, 32);
  dev_buf<uint32_t> dev;
  KHTRY(upload(c, dev, h.data(), h.size()));
  *out = dev.get();
  c->tables.emplace_back(key, std::move(dev));
  return KH_OK;
}

setup_args setup_on_lanes(kh_ctx *c, uint32_t L) {
  setup_args A;
  memset(&A, 0, sizeof A);
  A.comb = c->d_comb.get();
  A.L = L;
  A.cx = c->d_cx.get();
  A.cy = c->d_cy.get();
  return A;
}

walk_args walk_on_lanes(kh_ctx *c, const uint32_t *tab, const job_geom &jg, int H) {
  walk_args A;
  memset(&A, 0, sizeof A);
  A.tab = tab;
  A.cx = c->d_cx.get();
  A.cy = c->d_cy.get();
  A.scratch = c->d_scratch.get();
  A.L = jg.L;
  A.lane_stride = jg.gpl * 2 * H;
  return A;
}

int run_setup(kh_ctx *c, const std::vector<u256> &s, const ge *q) {
  uint32_t L = (uint32_t)s.size();
  c->cont_valid = false;  // the lane centres are about to be replaced
  KHTRY(ensure_lanes(c, L));
  c->h_scalars.resize((size_t)L * 8);
  for (uint32_t g = 0; g < L; g++) u256_to_limbs(&c->h_scalars[(size_t)g * 8], s[g]);
  HIPCHK(c, hipMemcpyAsync(c->d_scalars.get(), c->h_scalars.data(), (size_t)L * 32, hipMemcpyHostToDevice, c->stream));
  setup_args A = setup_on_lanes(c, L);
  A.scalars = c->d_scalars.get();
  dev_buf<uint32_t> dq;
  if (q) {
    KHTRY(dq.reserve(c, 16));
    HIPCHK(c, hipMemcpyAsync(dq.get(), q->x.d, 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dq.get() + 8, q->y.d, 32, hipMemcpyHostToDevice, c->stream));
    A.q = dq.get();
    A.has_q = 1;
  }
  HIPCHK(c, hipEventRecord(c->ev_a.get(), c->stream));
  HIPCHK(c, launch_setup(A, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_b.get(), c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev_b.get()));
  c->tm[4].add(c->ev_a.get(), c->ev_b.get(), 1, L);
  return KH_OK;
}

// Lane centres C_g = s_g * G for the progression s_g = s0 + g * step (mod n), g < L: the scalars are
// derived on the device (k_setup's prog mode), so a chunk whose lanes restart (-R, the first chunk)
// costs no host loop over 2^20 lanes and no 32 MB upload.  A lane scalar of 0 (its centre would be the
// point at infinity) fails the call, as the host check did.
int run_setup_prog(kh_ctx *c, const u256 &s0, const u256 &step, uint32_t L) {
  c->cont_valid = false;
  KHTRY(ensure_lanes(c, L));
  setup_args A = setup_on_lanes(c, L);
  A.prog = 1;
  u256_to_limbs(A.s0, s0);
  u256_to_limbs(A.step, step);
  A.zero_flag = c->d_zero_flag.get();
  HIPCHK(c, hipMemsetAsync(c->d_zero_flag.get(), 0, 4, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_a.get(), c->stream));
  HIPCHK(c, launch_setup(A, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_b.get(), c->stream));
  uint32_t zero = 0;
  HIPCHK(c, hipMemcpyAsync(&zero, c->d_zero_flag.get(), 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->tm[4].add(c->ev_a.get(), c->ev_b.get(), 1, L);
  if (zero) {
    c->err = "lane centre scalar is 0 mod n";
    return KH_E_ARG;
  }
  return KH_OK;
}

job_geom plan(kh_ctx *c, uint64_t total_groups, uint64_t gpl_divides, uint32_t lanes) {
  job_geom g;
  if (!lanes) lanes = c->lanes_max;
  uint64_t gpl = (total_groups + lanes - 1) / lanes;
  if (gpl == 0) gpl = 1;
  if (gpl_divides) {
    while (gpl < gpl_divides && gpl_divides % gpl) gpl++;
    if (gpl > gpl_divides) gpl = gpl_divides;
  }
  g.gpl = gpl;
  g.L = (uint32_t)((total_groups + gpl - 1) / gpl);
  return g;
}

int run_walk(kh_ctx *c, int mode, int kind, walk_args A, uint64_t gpl, uint32_t default_gpl_launch, int H) {
  uint32_t per = c->groups_per_launch ? c->groups_per_launch : default_gpl_launch;
  for (uint64_t gb = 0; gb < gpl; gb += per) {
    A.group_base = gb;
    A.groups = (uint32_t)std::min<uint64_t>(per, gpl - gb);
    HIPCHK(c, hipEventRecord(c->ev_a.get(), c->stream));
    HIPCHK(c, launch_walk(mode, A, c->stream, H));
    HIPCHK(c, hipEventRecord(c->ev_b.get(), c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev_b.get()));
    c->tm[kind].add(c->ev_a.get(), c->ev_b.get(), 1, (uint64_t)A.L * A.groups * 2 * H);
  }
  return KH_OK;
}

int fetch_hits(kh_ctx *c, uint32_t &n) {
  uint32_t cnt = 0;
  HIPCHK(c, hipMemcpyAsync(&cnt, c->d_hit_count.get(), 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (cnt > c->d_hits.cap()) {
    c->err = "device hit buffer overflow";
    return KH_E_OVERFLOW;
  }
  c->h_hits.resize(cnt);
  if (cnt) {
    HIPCHK(c, hipMemcpyAsync(c->h_hits.data(), c->d_hits.get(), (size_t)cnt * sizeof(kh_dev_hit), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  n = cnt;
  return KH_OK;
}

int grow_hits(kh_ctx *c, uint64_t cap, uint64_t limit, dev_buf<kh_dev_hit> *d, pinned_buf<kh_dev_hit> *h, int n) {
  if (cap > limit) return KH_E_OVERFLOW;
  auto drop = [&]() {
    for (int i = 0; i < n; i++) {
      d[i].reset();
      if (h) h[i].reset();
    }
  };
  drop();
  int r = KH_OK;
  for (int i = 0; i < n && !r; i++) {
    r = d[i].reserve(c, cap);
    if (!r && h) r = h[i].reserve(c, cap);
  }
  if (r) drop();
  return r;
}

// struct bloom as bloom_init2 leaves it (bloom/bloom.cpp:154-187): entries, bits, bytes, hashes,
// error (x87 long double), ready = 1, version 2.201, bpe; the pointers and chunk fields are 0 here
// (the reference writes its own heap pointer into `bf` and replaces it on reading)
void bloom_header(uint8_t h[KH_BLOOM_STRUCT], uint64_t entries, const bloom_desc &d) {
  memset(h, 0, KH_BLOOM_STRUCT);
  memcpy(h + 0, &entries, 8);
  memcpy(h + 8, &d.bits, 8);
  memcpy(h + 16, &d.bytes, 8);
  h[24] = (uint8_t)d.hashes;
  const long double err = 0.000001;
  memcpy(h + 32, &err, 10);
  h[48] = 1;
  h[49] = 2;
  h[50] = 201;
  const long double num = -logl(err), denom = 0.480453013918201;
  const double bpe = (double)(num / denom);
  memcpy(h + 56, &bpe, 8);
}

unsigned host_threads(kh_ctx *c) {
  if (!c->refine_threads) {
    unsigned hw = std::thread::hardware_concurrency();
    c->refine_threads = std::max(1u, std::min(16u, hw ? hw : 4u));
  }
  return c->refine_threads;
}

void sha256_bytes(const uint8_t *p, size_t n, uint8_t out[32]) {
  uint32_t st[8], w[16];
  sha256_init(st);
  uint8_t blk[64];
  size_t off = 0;
  auto compress = [&](const uint8_t *b) {
    for (int i = 0; i < 16; i++)
      w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
    sha256_transform(st, w);
  };
  for (; off + 64 <= n; off += 64) compress(p + off);
  size_t rem = n - off;
  memset(blk, 0, 64);
  memcpy(blk, p + off, rem);
  blk[rem] = 0x80;
  if (rem >= 56) {
    compress(blk);
    memset(blk, 0, 64);
  }
  const uint64_t bits = (uint64_t)n * 8;
  for (int i = 0; i < 8; i++) blk[56 + i] = (uint8_t)(bits >> (56 - 8 * i));
  compress(blk);
  for (int i = 0; i < 8; i++) {
    out[4 * i] = (uint8_t)(st[i] >> 24);
    out[4 * i + 1] = (uint8_t)(st[i] >> 16);
    out[4 * i + 2] = (uint8_t)(st[i] >> 8);
    out[4 * i + 3] = (uint8_t)st[i];
  }
}

// The blocked target filter the walk probes for exact targets (kh_kernels.hip tblk_probe): 16-byte
// blocks, KH_BLK_BITS_MUL x the reference bloom's bits; row words w = little-endian u32s of the
// 20 bytes: block (w0 * blocks) >> 32, bits from w1, w2 as kh_blk_masks (kh_kernels.h).
int upload_tblk(kh_ctx *c) {
  const uint64_t blocks = (c->tbd.bits * KH_BLK_BITS_MUL + 127) / 128;
  std::vector<uint4> words(blocks, make_uint4(0, 0, 0, 0));
  for (uint64_t r = 0; r < c->n_rows; r++) {
    const uint8_t *p = &c->rows[r * 20];
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
  c->d_tblk.reset();
  c->tblocks = (uint32_t)blocks;
  return upload(c, c->d_tblk, words.data(), words.size());
}

}  // namespace kh_host

// the reference-layout target bloom (h_tbloom, tbd) on the device, replacing the previous targets'
static int upload_target_bloom(kh_ctx *c) {
  c->d_tbloom.reset();
  KHTRY(c->d_tbloom.reserve(c, c->tbd.bytes + 4));
  HIPCHK(c, hipMemcpy(c->d_tbloom.get(), c->h_tbloom.data(), c->tbd.bytes, hipMemcpyHostToDevice));
  return KH_OK;
}

// m * stride mod n (m < 2^128)
static u256 mul_stride(const u256 &stride, u128 m) {
  return u256_cmp(stride, u256_u64(1)) == 0 ? sc_reduce(u256_from_u128(m)) : sc_mul_u128(stride, m);
}

// the walk kernel's mode for the ABI's mode (without KH_MODE_ENDO) and search
static int walk_mode(uint32_t mode, uint32_t search, bool endo) {
  int km = mode == KH_MODE_XPOINT ? KM_XPOINT
         : mode == KH_MODE_ETH ? KM_ETH
         : search == KH_SEARCH_COMPRESS ? KM_H160C
         : search == KH_SEARCH_UNCOMPRESS ? KM_H160U
                                          : KM_H160B;
  return endo ? km | KM_ENDO : km;
}

// ==============================================================================================
// C ABI
// ==============================================================================================
extern "C" {

int kh_abi_version(void) { return KH_ABI_VERSION; }

const char *kh_strerror(int code) {
  switch (code) {
    case KH_OK: return "ok";
    case KH_E_ARG: return "invalid argument";
    case KH_E_HIP: return "HIP runtime error";
    case KH_E_NOMEM: return "out of memory";
    case KH_E_STATE: return "call out of order";
    case KH_E_OVERFLOW: return "output buffer too small";
    case KH_E_BSGS_N: return "BSGS n has no exact square root or sqrt(n) is not a multiple of 1024";
    case KH_E_RANGE: return "the given range is small";
    case KH_E_IO: return "file missing, short or not writable";
    case KH_E_FORMAT: return "file does not match the BSGS geometry or its checksum";
    default: return "unknown error";
  }
}

const char *kh_last_error(kh_ctx *ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int kh_device_count(int *count) {
  if (!count) return KH_E_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return KH_OK;
}

int kh_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return KH_E_HIP;
  if (hipSetDevice(device) != hipSuccess) return KH_E_HIP;
  size_t f = 0, t = 0;
  if (hipMemGetInfo(&f, &t) != hipSuccess) return KH_E_HIP;
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return KH_OK;
}

// kh_open's device part; the caller deletes the context on failure
static int open_device(kh_ctx *c) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  int lo = 0, hi = 0;
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
  HIPCHK(c, hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, hi));
  KHTRY(c->ev_a.create(c));
  KHTRY(c->ev_b.create(c));
  c->comb.build();
  std::vector<uint32_t> h((size_t)32 * 256 * 16, 0);
  for (int i = 0; i < 32 * 256; i++) {
    if (i % 256 == 0) continue;
    memcpy(&h[(size_t)i * 16], c->comb.t[i].x.d, 32);
    memcpy(&h[(size_t)i * 16 + 8], c->comb.t[i].y.d, 32);
  }
  KHTRY(upload(c, c->d_comb, h.data(), h.size()));
  // test hook: a small initial BSGS candidate buffer exercises the grow-and-redo path
  if (const char *e = getenv("KH_CAND_CAP")) c->cand_cap0 = std::max<uint32_t>(1, (uint32_t)strtoul(e, nullptr, 0));
  // A/B and parity hook: KH_REFINE=host runs the second check on host threads instead of k_refine
  if (const char *e = getenv("KH_REFINE")) c->refine_host = strcmp(e, "host") == 0;
  KHTRY(c->d_hit_count.reserve(c, 1));
  KHTRY(c->d_zero_flag.reserve(c, 1));
  return c->d_hits.reserve(c, kh_ctx::HIT_CAP0);
}

int kh_open(int device, kh_ctx **out) {
  if (!out) return KH_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return KH_E_HIP;
  kh_ctx *c = new kh_ctx();
  c->device = device;
  memcpy(c->mk_alpha, KH_MINIKEY_ALPHABET, 58);
  int r = open_device(c);
  if (r) {
    delete c;
    return r;
  }
  *out = c;
  return KH_OK;
}

int kh_close(kh_ctx *ctx) {
  delete ctx;
  return KH_OK;
}

int kh_release_walk(kh_ctx *ctx) {
  if (!ctx) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  ctx->release_lanes();
  ctx->cont_valid = false;
  ctx->kang = kang_state();  // the kangaroo search's herd, table and buffers
  return KH_OK;
}

int kh_bsgs_geometry(kh_ctx *ctx, uint32_t *lanes, double rates[2]) {
  if (!ctx) return KH_E_ARG;
  if (lanes) *lanes = ctx->lanes_pick;
  if (rates) {
    rates[0] = ctx->cal_rate[0];
    rates[1] = ctx->cal_rate[1];
  }
  return KH_OK;
}

int kh_bsgs_placement(kh_ctx *ctx, double rates[4]) {
  if (!ctx || !rates) return KH_E_ARG;
  rates[0] = ctx->cal_rate[0];
  rates[1] = ctx->cal_rate[1];
  rates[2] = rates[3] = 0.0;  // no layer-1 stage
  return ctx->bsgs_calibrated ? 1 : 0;
}

int kh_set_geometry(kh_ctx *ctx, uint32_t lanes, uint32_t groups_per_launch) {
  if (!ctx) return KH_E_ARG;
  ctx->lanes_max = lanes ? lanes : (1u << 18);
  ctx->lanes_hb = lanes ? lanes : KH_LANES_HB;
  ctx->lanes_bsgs = lanes ? lanes : KH_BSGS_LANES;
  ctx->groups_per_launch = groups_per_launch;
  // an explicit geometry overrides an earlier calibration's pick (and a default one calibrates again)
  ctx->lanes_pick = 0;
  ctx->bsgs_calibrated = false;
  for (double &x : ctx->cal_rate) x = 0;
  return KH_OK;
}

int kh_set_rmd_batch(kh_ctx *ctx, uint32_t group) {
  if (!ctx) return KH_E_ARG;
  if (group == 0 || group == 2 * KH_WALK_H) {
    ctx->rmd_batch = 0;
    return KH_OK;
  }
  if (group < 4 || group > 2 * KH_WALK_H || group % 4) {
    ctx->err = "rmd batch size: a multiple of 4 in [4, 1024] (keyhunt.cpp:815-829 clamps to that)";
    return KH_E_ARG;
  }
  ctx->rmd_batch = group;
  ctx->cont_valid = false;
  return KH_OK;
}

int kh_synchronize(kh_ctx *ctx) {
  if (!ctx) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->side));
  return KH_OK;
}

// ---------------------------------------------------------------------------------------------
// address / rmd160 / xpoint
// ---------------------------------------------------------------------------------------------
int kh_set_targets(kh_ctx *ctx, const uint8_t *rows, uint64_t n, uint64_t bloom_items) {
  if (!ctx || (!rows && n)) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  std::vector<std::array<uint8_t, 20>> v(n);
  for (uint64_t i = 0; i < n; i++) memcpy(v[i].data(), rows + i * 20, 20);
  std::sort(v.begin(), v.end(), [](const std::array<uint8_t, 20> &a, const std::array<uint8_t, 20> &b) {
    return memcmp(a.data(), b.data(), 20) < 0;
  });
  ctx->rows.resize(n * 20);
  for (uint64_t i = 0; i < n; i++) memcpy(&ctx->rows[i * 20], v[i].data(), 20);
  ctx->n_rows = n;
  ctx->vanity = false;
  ctx->cont_valid = false;  // the next walk may need another pad (dense vs sparse): start its lanes again
  ctx->probe_len = 20;
  ctx->v_ranges.clear();
  ctx->t_entries = bloom_entries(bloom_items ? bloom_items : n);
  ctx->tbd = bloom_size(ctx->t_entries);
  ctx->h_tbloom.assign(ctx->tbd.bytes, 0);
  for (uint64_t i = 0; i < n; i++) host_bloom_add(ctx->h_tbloom.data(), ctx->tbd, &ctx->rows[i * 20], 20);
  KHTRY(upload_target_bloom(ctx));
  return upload_tblk(ctx);
}

int kh_set_vanity(kh_ctx *ctx, const uint8_t *ranges, uint64_t n, uint32_t probe_len, uint64_t bloom_items) {
  if (!ctx || (!ranges && n) || probe_len == 0 || probe_len > 20) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  ctx->v_ranges.assign(ranges, ranges + n * 40);
  ctx->rows.clear();
  ctx->n_rows = 0;
  ctx->vanity = true;
  ctx->cont_valid = false;  // a vanity walk writes the dense pad: never resume an exact-target walk's lanes
  ctx->probe_len = probe_len;
  ctx->d_tblk.reset();  // prefixes probe the reference-layout bloom
  // processOneVanity / readFileVanity (keyhunt.cpp:6970-7035): bloom over A's first probe_len bytes
  ctx->t_entries = bloom_entries(bloom_items ? bloom_items : n);
  ctx->tbd = bloom_size(ctx->t_entries);
  ctx->h_tbloom.assign(ctx->tbd.bytes, 0);
  for (uint64_t i = 0; i < n; i++) host_bloom_add(ctx->h_tbloom.data(), ctx->tbd, &ctx->v_ranges[i * 40], (int)probe_len);
  KHTRY(upload_target_bloom(ctx));
  return upload_tblk(ctx);
}

int kh_scan_memory(uint64_t n_keys, uint32_t mode, uint32_t search, uint64_t *needed_bytes) {
  if (!needed_bytes || n_keys == 0) return KH_E_ARG;
  const bool endo = (mode & KH_MODE_ENDO) != 0;
  mode &= ~(uint32_t)(KH_MODE_ENDO | KH_MODE_P2SH);  // the nested probes walk the plain form's geometry
  if (mode > KH_MODE_ETH || search > KH_SEARCH_BOTH) return KH_E_ARG;
  const int km = walk_mode(mode, search, endo);
  // kh_scan's choice at the default geometry (a chunk that reaches the order keeps the small groups,
  // which need less): exact targets, so -m xpoint probes the blocked filter with the sparse pad
  const int H = (km == KM_XPOINT || km == KM_H160C) && n_keys % (2 * KH_WALK_HB) == 0 ? KH_WALK_HB : KH_WALK_H;
  const uint64_t lanes = H == KH_WALK_HB ? KH_LANES_HB : (1u << 18);
  const uint64_t groups = (n_keys + 2 * H - 1) / (2 * H);
  const uint64_t gpl = (groups + lanes - 1) / lanes, L = (groups + gpl - 1) / gpl;
  *needed_bytes = L * (uint64_t)walk_pad_rows(km, true, H) * 32 + L * 32 * 3 + (512u << 10) +
                  (uint64_t)65536 * sizeof(kh_dev_hit);
  return KH_OK;
}

// Confirm each bloom hit of a kh_scan (the first nd of ctx->h_hits) against the sorted table and
// resolve the key: parity fix-up (keyhunt.cpp:3619-3636); with -e the image e gives key * lambda^e,
// and the 04 variants with -Y the negated key (keyhunt.cpp:3525-3700, 3765-3800).  Hits come out in
// the order one reference thread prints them: per point, compressed variants (image-major), then
// uncompressed, then xpoint.
static std::vector<kh_hit> resolve_hits(kh_ctx *ctx, uint32_t nd, const u256 &st, const u256 &stride, uint32_t mode,
                                        bool endo, uint32_t zg, int H, bool p2sh = false) {
  auto order = [p2sh](uint32_t kind) {
    uint32_t base = kind & 15u, e = (kind >> KH_DKIND_ENDO_SHIFT) & 3u, neg = (kind & KH_DKIND_NEG) ? 1u : 0u;
    // KH_MODE_P2SH: per image plain 02, plain 03, nested 02, nested 03; the 04 hits follow as without it
    if (p2sh) return base < 2 ? 4 * e + base + ((kind & KH_DKIND_P2SH) ? 2u : 0u) : 12 + 2 * e + neg;
    return base < 2 ? 2 * e + base : base == 2 || base == KH_KIND_ETH ? 6 + 2 * e + neg : 12 + e;
  };
  std::vector<kh_dev_hit> dh(ctx->h_hits.begin(), ctx->h_hits.begin() + nd);
  // -e -c eth: a hit on (beta X, Y) is also the reference's slot-4 hit (keyhunt.cpp:3533), whose key
  // it derives as lambda^2 k, checks against the image, and so negates (3736-3744): added as kind
  // ETH | ENDO2 (an image the GPU never probes in this mode) before the sort, whose order puts it
  // between the point's slot-3 eth(-beta P) and slot-5 eth(-beta^2 P) hits (3706-3745)
  if (endo && mode == KH_MODE_ETH) {
    for (size_t i = 0, n = dh.size(); i < n; i++)
      if (dh[i].kind == (KH_KIND_ETH | (1u << KH_DKIND_ENDO_SHIFT))) {
        kh_dev_hit t = dh[i];
        t.kind = KH_KIND_ETH | (2u << KH_DKIND_ENDO_SHIFT);
        dh.push_back(t);
      }
  }
  std::sort(dh.begin(), dh.end(), [&](const kh_dev_hit &a, const kh_dev_hit &b) {
    return a.idx != b.idx ? a.idx < b.idx : order(a.kind) < order(b.kind);
  });
  static const u256 LAMBDA[3] = {
      u256_u64(1),
      u256{{0xdf02967c1b23bd72ULL, 0x122e22ea20816678ULL, 0xa5261c028812645aULL, 0x5363ad4cc05c30e0ULL}},
      u256{{0xe0cfc810b51283ceULL, 0xa880b9fc8ec739c2ULL, 0x5ad9e3fd77ed9ba4ULL, 0xac9c52b33fa3cf1fULL}}};
  static const fe BETA[3] = {
      fe{{1, 0, 0, 0, 0, 0, 0, 0}},
      fe{{0x719501eeu, 0xc1396c28u, 0x12f58995u, 0x9cf04975u, 0xac3434e9u, 0x6e64479eu, 0x657c0710u, 0x7ae96a2bu}},
      fe{{0x8e6afa40u, 0x3ec693d6u, 0xed0a766au, 0x630fb68au, 0x53cbcb16u, 0x919bb861u, 0x9a83f8efu, 0x851695d4u}}};
  std::vector<kh_hit> out;
  for (auto &h : dh) {
    const u256 k = sc_add(st, mul_stride(stride, (u128)h.idx));
    ge P;
    if (!ctx->comb.mult(P, k)) continue;
    const uint32_t base = h.kind & 15u, e = (h.kind >> KH_DKIND_ENDO_SHIFT) & 3u;
    const bool neg = (h.kind & KH_DKIND_NEG) != 0;
    if (e > 2) continue;
    // the point the walk produced at this slot: k*G, or with --rmd-batch-size < 1024 and a slot
    // other than its group's centre, x = -(C.x + (i+1)D.x), y = -+(i+1)D.y (k_walk_zinv)
    ge S = P;
    bool garbage = false;
    if (zg && h.idx % zg != (uint64_t)H) {
      const uint64_t grp = h.idx / zg, t = h.idx % zg;
      const uint64_t i = t > (uint64_t)H ? t - H - 1 : H - t - 1;
      ge C, Di;
      if (!ctx->comb.mult(C, sc_add(st, mul_stride(stride, (u128)grp * zg + H))) ||
          !ctx->comb.mult(Di, mul_stride(stride, (u128)(i + 1))))
        continue;
      fe sx;
      fe_add(sx, C.x, Di.x);
      fe_neg(S.x, sx);
      S.y = Di.y;
      if (t > (uint64_t)H) fe_neg(S.y, Di.y);
      garbage = true;
    }
    fe xe = S.x, ye = S.y;
    if (e) fe_mul(xe, S.x, BETA[e]);
    if (neg) fe_neg(ye, S.y);
    uint8_t probe[20];
    uint32_t w[5];
    bool compressed = false;
    if (base == KH_KIND_02 || base == KH_KIND_03) {
      hash160_comp(xe, 2 + base, w);
      if (h.kind & KH_DKIND_P2SH) {  // the nested digest of that hash is what the filter matched
        uint32_t hn[5];
        hash160_nested(w, hn);
        memcpy(w, hn, 20);
      }
      compressed = true;
    } else if (base == KH_KIND_04) {
      hash160_uncomp(xe, ye, w);
    } else if (base == KH_KIND_ETH) {
      if (endo && e == 2 && !neg)  // the slot-4 twin: its image is eth(beta P)
        fe_mul(xe, S.x, BETA[1]);
      eth_address(xe, ye, w);
    } else {
      for (int j = 0; j < 5; j++) w[j] = bswap32(xe.d[7 - j]);
    }
    memcpy(probe, w, 20);
    if (ctx->vanity && base != KH_KIND_XPOINT && base != KH_KIND_ETH) {
      // vanityrmdmatch (keyhunt.cpp:6677-6703): inside any [A, B] range
      bool in = false;
      for (size_t j = 0; j < ctx->v_ranges.size() && !in; j += 40)
        in = memcmp(&ctx->v_ranges[j], probe, 20) <= 0 && memcmp(&ctx->v_ranges[j + 20], probe, 20) >= 0;
      if (!in) continue;
    } else if (!searchbinary(ctx->rows.data(), (int64_t)ctx->n_rows, probe, 20, 0)) {
      continue;
    }
    kh_hit o;
    memset(&o, 0, sizeof o);
    u256 kr = e ? sc_mul(k, LAMBDA[e]) : k;  // (beta^e x, y) = lambda^e * (x, y)
    if (base == KH_KIND_ETH && endo && e == 2 && !neg) {
      kr = sc_neg(kr);  // the slot-4 twin: lambda^2 k gives (beta^2 X, Y), not the image: negated
    } else if (garbage && (compressed ? !endo : endo)) {
      // where the reference checks the found key's own image against the hit -- compressed without
      // -e (keyhunt.cpp:3619-3636), 04 and eth with -e (3652-3680, 3714-3744) -- a point that is no
      // multiple of G never matches it: negated
      kr = sc_neg(kr);
    } else if (compressed) {
      uint32_t odd = P.y.d[0] & 1;  // the image keeps Y; -e: the slot key's parity (3565-3600)
      if (odd != (base == KH_KIND_03 ? 1u : 0u)) kr = sc_neg(kr);
    } else if (neg) {
      kr = sc_neg(kr);
    }
    u256_to_be(o.key, kr);
    o.offset = h.idx;
    o.kind = h.kind;
    o.compressed = compressed ? 1 : 0;
    out.push_back(o);
  }
  return out;
}

int kh_scan(kh_ctx *ctx, const uint8_t start[32], const uint8_t stride_be[32], uint64_t n_keys, uint32_t mode,
            uint32_t search, kh_hit *hits, uint32_t cap, uint32_t *n_hits) {
  if (!ctx || !start || !n_hits || n_keys == 0) return KH_E_ARG;
  // --rmd-batch-size below 1024: groups of zg slots (kh_set_rmd_batch, k_walk_zinv)
  const uint32_t zg = ctx->rmd_batch;
  if (!zg && n_keys % (2 * KH_WALK_H)) return KH_E_ARG;
  const bool endo = (mode & KH_MODE_ENDO) != 0;
  const bool p2sh = (mode & KH_MODE_P2SH) != 0;
  mode &= ~(uint32_t)(KH_MODE_ENDO | KH_MODE_P2SH);
  if (mode > KH_MODE_ETH || search > KH_SEARCH_BOTH) return KH_E_ARG;
  if (p2sh && (mode != KH_MODE_ADDRESS || search == KH_SEARCH_UNCOMPRESS || ctx->vanity || zg)) {
    ctx->err = mode != KH_MODE_ADDRESS           ? "KH_MODE_P2SH applies to KH_MODE_ADDRESS only (not xpoint, not eth)"
               : search == KH_SEARCH_UNCOMPRESS ? "KH_MODE_P2SH needs compressed keys: a P2SH-P2WPKH key is compressed by rule"
               : ctx->vanity                    ? "KH_MODE_P2SH needs exact targets, not vanity prefixes"
                                                : "KH_MODE_P2SH does not walk --rmd-batch-size groups below 1024";
    return KH_E_ARG;
  }
  if (zg && (mode == KH_MODE_XPOINT || ctx->vanity)) {
    ctx->err = "--rmd-batch-size applies to -m rmd160 (hash160 or -c eth) with exact targets only";
    return KH_E_ARG;
  }
  if (!ctx->d_tbloom) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  if (zg) {
    // k_walk_zinv centres group m on offset zg/2 + m*zg and reaches it by C += T[H] from the previous
    // centre (or, a lane's first, by a scalar multiplication).  A centre whose key is 0 mod n -- offset
    // k0 = -start * stride^-1 mod n -- is the point at infinity, from which the reference builds its
    // group out of its own infinity representation; this engine does not restate that group.  The
    // groups before it are scanned (and their hits returned), then the call reports KH_E_RANGE.
    const u256 st0 = sc_reduce(u256_from_be(start));
    const u256 sd0 = stride_be ? sc_reduce(u256_from_be(stride_be)) : u256_u64(1);
    if (u256_is_zero(sd0)) return KH_E_ARG;
    const u256 k0 = u256_cmp(sd0, u256_u64(1)) == 0 ? sc_neg(st0) : sc_mul(sc_neg(st0), sc_inv(sd0));
    const uint64_t half = zg / 2, groups = (n_keys + zg - 1) / zg;
    if (k0.v[1] == 0 && k0.v[2] == 0 && k0.v[3] == 0 && k0.v[0] >= half && (k0.v[0] - half) % zg == 0 &&
        (k0.v[0] - half) / zg < groups) {
      const uint64_t m_bad = (k0.v[0] - half) / zg;
      uint32_t nh = 0;
      int r0 = KH_OK;
      if (m_bad) {
        r0 = kh_scan(ctx, start, stride_be, m_bad * zg, mode | (endo ? KH_MODE_ENDO : 0), search, hits, cap, &nh);
        if (r0 && r0 != KH_E_OVERFLOW) return r0;
      }
      *n_hits = nh;
      ctx->err = "--rmd-batch-size below 1024: a group centred on the key 0 mod n (the reference builds it "
                 "from its point at infinity); the groups before it were scanned";
      return r0 == KH_E_OVERFLOW ? r0 : KH_E_RANGE;
    }
  }
  const int km = walk_mode(mode, search, endo) | (p2sh ? KM_P2SH : 0);
  u256 st = sc_reduce(u256_from_be(start));
  u256 stride = stride_be ? sc_reduce(u256_from_be(stride_be)) : u256_u64(1);
  if (u256_is_zero(stride)) return KH_E_ARG;
  // xpoint and compressed rmd160/address (configs 2-3) walk 4096-point groups when the chunk holds
  // whole ones (the default 2^32-key chunk does): one inversion per 4096 points.  A chunk that
  // reaches the group order keeps the reference's 1024-key groups: there a centre can equal
  // -(i+1)*stride*G, whose zero difference collapses the group's batch inversion (parity note 4),
  // and only the reference's own geometry collapses the same groups (fixtures *_near_order)
  const int H = zg ? (int)(zg / 2)
                : ((km == KM_XPOINT || (km & ~KM_P2SH) == KM_H160C) && n_keys % (2 * KH_WALK_HB) == 0 &&
                   !reaches_order(st, stride, n_keys + 4 * KH_WALK_HB) && !getenv("KH_NO_BIG_GROUPS"))
                    ? KH_WALK_HB
                    : KH_WALK_H;
  const uint32_t *tab = nullptr;
  int r;

  // the reference's do-while runs whole groups (keyhunt.cpp:3350, 3836): a chunk that is no
  // multiple of the group overshoots its end
  uint64_t total_groups = (n_keys + 2 * H - 1) / (2 * H);
  const uint64_t n_points = total_groups * 2 * H;
  job_geom jg = plan(ctx, total_groups, 0, H == KH_WALK_HB ? ctx->lanes_hb : 0);
  // large-group modes interleave lanes (lane g walks groups g, g + L, ...) when the lanes divide
  // the chunk: after the call every lane sits on its group of the chunk that follows, so a call
  // starting there continues them without a lane setup
  const bool inter = H == KH_WALK_HB && (uint64_t)jg.L * jg.gpl == total_groups;
  KHTRY(get_table(ctx, stride, &tab, H, inter ? jg.L : 1));
  // the pad's rows per lane (the walk below probes the blocked target filter exactly when A.tblk is
  // set): a resumed walk must find at least that many rows, since the exact-target (sparse) pad is half
  // the dense one a vanity or reference-bloom walk writes
  const bool tblk = !(ctx->vanity || getenv("KH_REF_TARGET_BLOOM")) && ctx->d_tblk;
  const int pad_rows = zg ? H : walk_pad_rows(km, tblk, H);  // km keeps KM_ENDO: as launch_walk sees it
  const bool resume = inter && ctx->cont_valid && ctx->cont_kind == 1 && ctx->cont_km == km &&
                      ctx->cont_L == jg.L && ctx->cont_H == H && ctx->scratch_h() >= pad_rows &&
                      ctx->lanes_alloc() >= jg.L && u256_cmp(ctx->cont_next, st) == 0 &&
                      u256_cmp(ctx->cont_stride, stride) == 0;
  ctx->cont_valid = false;
  // lane g's first centre: offset H + g * lane_step, lane_step = 2H (interleaved) or gpl * 2H; the
  // scalars s0 + g * (lane_step * stride) are derived on the device (run_setup_prog: a -R chunk
  // restarts 2^20 lanes)
  const u256 lane_step = mul_stride(stride, inter ? (u128)(2 * H) : (u128)jg.gpl * (2 * H));
  const u256 s0 = sc_add(st, mul_stride(stride, (u128)H));
  if (!resume) {
    KHTRY(ensure_lanes(ctx, jg.L, pad_rows));  // before the centres are set
    KHTRY(run_setup_prog(ctx, s0, lane_step, jg.L));
  }
  KHTRY(ctx->d_hits.reserve(ctx, kh_ctx::HIT_CAP0));  // held since kh_open, unless a grow failed

  walk_args A = walk_on_lanes(ctx, tab, jg, H);
  A.interleave = inter ? 1 : 0;
  A.n_points = n_points;
  A.zhalf = zg ? (uint32_t)H : 0;
  A.bloom = ctx->d_tbloom.get();
  A.bd = ctx->tbd;
  A.tblk = tblk ? ctx->d_tblk.get() : nullptr;
  A.tblocks = ctx->tblocks;
  A.hit_count = ctx->d_hit_count.get();
  A.probe_len = mode == KH_MODE_XPOINT || mode == KH_MODE_ETH ? 20 : ctx->probe_len;
  uint32_t nd = 0;
  ctx->scan_dev_hits = 0;
  ctx->scan_redos = 0;
  for (;;) {
    A.hits = ctx->d_hits.get();
    A.hit_cap = (uint32_t)ctx->d_hits.cap();
    HIPCHK(ctx, hipMemsetAsync(ctx->d_hit_count.get(), 0, 4, ctx->stream));
    KHTRY(run_walk(ctx, km, mode == KH_MODE_XPOINT ? 1 : 0, A, jg.gpl, 2, H));
    r = fetch_hits(ctx, nd);
    if (r != KH_E_OVERFLOW) break;
    // more bloom hits than the buffer holds (short vanity prefixes): grow it, redo the chunk
    uint32_t need = 0;
    HIPCHK(ctx, hipMemcpy(&need, ctx->d_hit_count.get(), 4, hipMemcpyDeviceToHost));
    uint64_t cap2 = ctx->d_hits.cap();
    while (cap2 < need) cap2 *= 2;
    KHTRY(grow_hits(ctx, cap2, 1u << 26, &ctx->d_hits));
    ctx->scan_redos++;
    KHTRY(run_setup_prog(ctx, s0, lane_step, jg.L));  // the walk moved the lane centres on: start them again
  }
  if (r) return r;
  ctx->scan_dev_hits = nd;
  if (inter) {  // the lanes now sit on the chunk that starts at st + n_keys * stride
    ctx->cont_valid = true;
    ctx->cont_kind = 1;
    ctx->cont_km = km;
    ctx->cont_L = jg.L;
    ctx->cont_H = H;
    ctx->cont_stride = stride;
    ctx->cont_next = sc_add(st, sc_mul_u128(stride, n_keys));
  }
  const std::vector<kh_hit> out = resolve_hits(ctx, nd, st, stride, mode, endo, zg, H, p2sh);
  *n_hits = (uint32_t)out.size();
  if (hits)
    for (uint32_t i = 0; i < out.size() && i < cap; i++) hits[i] = out[i];
  return out.size() > cap ? KH_E_OVERFLOW : KH_OK;
}

// ==============================================================================================
// Target files (-S for address/rmd160/xpoint): data_<hex>.dat as readFileAddress reads it
// (keyhunt.cpp:7033-7210) and writeFileIfNeeded writes it (7756-7855):
//   sha256(bloom bits) | struct bloom (112 B) | bloom bits | sha256(table) | u64 table bytes |
//   the sorted 20-byte rows (struct address_value).
// ==============================================================================================
int kh_targets_save(kh_ctx *ctx, const char *path) {
  if (!ctx || !path) return KH_E_ARG;
  if (!ctx->d_tbloom || ctx->vanity) return KH_E_STATE;
  FILE *f = fopen(path, "wb");
  if (!f) {
    ctx->err = std::string("can't create the file ") + path;
    return KH_E_IO;
  }
  uint8_t ckb[32], ckd[32], h[KH_BLOOM_STRUCT];
  sha256_bytes(ctx->h_tbloom.data(), ctx->tbd.bytes, ckb);
  bloom_header(h, ctx->t_entries, ctx->tbd);
  const uint64_t data_size = ctx->n_rows * 20;
  sha256_bytes(ctx->rows.data(), data_size, ckd);
  bool ok = fwrite(ckb, 1, 32, f) == 32 && fwrite(h, 1, KH_BLOOM_STRUCT, f) == KH_BLOOM_STRUCT &&
            fwrite(ctx->h_tbloom.data(), 1, ctx->tbd.bytes, f) == ctx->tbd.bytes && fwrite(ckd, 1, 32, f) == 32 &&
            fwrite(&data_size, 1, 8, f) == 8 && fwrite(ctx->rows.data(), 1, data_size, f) == data_size;
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    ctx->err = std::string("error writing the file ") + path;
    return KH_E_IO;
  }
  return KH_OK;
}

int kh_targets_load(kh_ctx *ctx, const char *path, uint32_t flags) {
  if (!ctx || !path) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  FILE *f = fopen(path, "rb");
  if (!f) {
    ctx->err = std::string("can't open the file ") + path;
    return KH_E_IO;
  }
  uint8_t ckb[32], ckd[32], h[KH_BLOOM_STRUCT], ck[32];
  std::vector<uint8_t> bits, rows;
  uint64_t entries = 0, nbits = 0, nbytes = 0, data_size = 0;
  int rc = KH_OK;
  if (fread(ckb, 1, 32, f) != 32 || fread(h, 1, KH_BLOOM_STRUCT, f) != KH_BLOOM_STRUCT) rc = KH_E_IO;
  if (!rc) {
    memcpy(&entries, h + 0, 8);
    memcpy(&nbits, h + 8, 8);
    memcpy(&nbytes, h + 16, 8);
    // the reader trusts bits/bytes/hashes of the stored struct (keyhunt.cpp:7076-7081)
    if (nbits == 0 || h[24] == 0 || nbytes != nbits / 8 + ((nbits % 8) ? 1 : 0)) rc = KH_E_FORMAT;
  }
  if (!rc) {
    bits.resize(nbytes);
    if (fread(bits.data(), 1, nbytes, f) != nbytes || fread(ckd, 1, 32, f) != 32 || fread(&data_size, 1, 8, f) != 8)
      rc = KH_E_IO;
  }
  if (!rc && data_size % 20) rc = KH_E_FORMAT;
  if (!rc) {
    rows.resize(data_size);
    if (fread(rows.data(), 1, data_size, f) != data_size) rc = KH_E_IO;
  }
  fclose(f);
  if (!rc && !(flags & KH_LOAD_SKIP_CHECKSUM)) {  // FLAGSKIPCHECKSUM (keyhunt.cpp:7129-7146, 7193-7200)
    sha256_bytes(bits.data(), nbytes, ck);
    if (memcmp(ck, ckb, 32)) rc = KH_E_FORMAT;
    sha256_bytes(rows.data(), data_size, ck);
    if (!rc && memcmp(ck, ckd, 32)) rc = KH_E_FORMAT;
  }
  if (rc) {
    ctx->err = std::string(rc == KH_E_IO ? "error reading the file " : "checksum or format mismatch in ") + path;
    return rc;
  }
  bloom_desc d;
  memset(&d, 0, sizeof d);
  d.bits = nbits;
  d.bytes = nbytes;
  d.hashes = h[24];
  d.recip = ~0ULL / d.bits;
  d.stride = d.bytes;
  ctx->rows.swap(rows);
  ctx->n_rows = data_size / 20;
  ctx->vanity = false;
  ctx->probe_len = 20;
  ctx->v_ranges.clear();
  ctx->t_entries = entries;
  ctx->tbd = d;
  ctx->h_tbloom.swap(bits);
  ctx->d_tblk.reset();  // the previous targets' blocked filter: these probe the file's bloom
  return upload_target_bloom(ctx);
}

}  // extern "C"
