// kh_capi_bsgs.cpp -- BSGS: setup, build, table files, the host second and third checks, the
// giant-step scan and its calibration.
#include <atomic>

#include "kh_ctx.h"

extern "C" int kh_bsgs_setup(kh_ctx *ctx, uint64_t n, uint64_t k, kh_bsgs_info *info) {
  if (ctx) ctx->cont_valid = false;
  if (!ctx || !k) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  // keyhunt.cpp:1454-1661
  uint64_t m = (uint64_t)sqrtl((long double)n);
  while (m * m > n) m--;
  while ((m + 1) * (m + 1) <= n) m++;
  if (m * m != n || m % 1024) return KH_E_BSGS_N;
  m *= k;
  uint64_t m2 = m / 32 + (m % 32 ? 1 : 0);
  uint64_t m3 = m2 / 32 + (m2 % 32 ? 1 : 0);
  uint64_t aux = n / m;
  if (n % m) n = m * aux;
  kh_bsgs_info &I = ctx->info;
  memset(&I, 0, sizeof I);
  ctx->entries[0] = ctx->entries[1] = ctx->entries[2] = 0;
  I.n = n;
  I.m = m;
  I.m2 = m2;
  I.m3 = m3;
  I.aux = aux;
  I.cycles = aux / 1024 + (aux % 1024 ? 1 : 0);
  uint64_t it[3];
  it[0] = (m / 256 > 10000) ? (m / 256 + (m % 256 ? 1 : 0)) : 1000;
  it[1] = (m2 / 256 > 1000) ? (m2 / 256 + (m2 % 256 ? 1 : 0)) : 1000;
  it[2] = (m3 / 256 > 1000) ? (m3 / 256 + (m3 % 256 ? 1 : 0)) : 1000;
  for (int l = 0; l < 3; l++) {
    // initBloomFilter's entry count (keyhunt.cpp:7608): the 10000 floor, else -z x items
    ctx->entries[l] = it[l] <= 10000 ? 10000 : (uint64_t)ctx->bloom_mult * it[l];
    ctx->bd[l] = bloom_size(ctx->entries[l]);
    ctx->bd_ref1 = l == 0 ? ctx->bd[0] : ctx->bd_ref1;
    ctx->bd_ref1.stride = (ctx->bd_ref1.bytes + 255) & ~255ULL;
    if (l == 0 && ctx->l1_layout == KH_LAYER1_BLOCKED) {
      // 3x the reference's bits per shard in whole 128-bit blocks (kh_kernels.h); desc.bits = blocks
      uint64_t blocks = (ctx->bd[0].bits * KH_BLK_BITS_MUL + 127) / 128;
      // the probe record carries the block index within a shard and the shard byte, and addresses a
      // shard by a 32-bit stride (k_walk blk_record / blk_load): shards must stay below 4 GB
      if (((blocks * 16 + 255) & ~255ULL) >> 32) {
        ctx->err = "blocked layer 1 needs shards below 4 GB (M < ~2^36.6; the reference layout's shards reach the "
                   "2^32-bit probe limit below that, at M ~2^35.1)";
        return KH_E_ARG;
      }
      ctx->bd[0].bits = blocks;
      ctx->bd[0].recip = ~0ULL / blocks;
      ctx->bd[0].bytes = blocks * 16;
    }
    ctx->bd[l].stride = (ctx->bd[l].bytes + 255) & ~255ULL;
    if (ctx->bd[l].bits >> 32) {  // shards of 2^32 bits or more (M >= ~2^35.1 in layer 1) are refused
      ctx->err = "a bloom shard of 2^32 bits or more (M >= ~2^35.1) is outside the engine's tested probe range";
      return KH_E_ARG;
    }
    I.bloom_bits[l] = (l == 0 && ctx->l1_layout == KH_LAYER1_BLOCKED) ? ctx->bd[0].bits * 128 : ctx->bd[l].bits;
    I.bloom_bytes[l] = ctx->bd[l].bytes;
    I.bloom_hashes[l] = (l == 0 && ctx->l1_layout == KH_LAYER1_BLOCKED) ? 16u : ctx->bd[l].hashes;
  }
  I.layer1_layout = ctx->l1_layout;
  for (int l = 0; l < 3; l++) {
    size_t bytes = 256 * ctx->bd[l].stride + 4;
    // (fine-grained and uncached memory types for layer 1 were measured in round 4: no gain, the
    // probes still cost the same power, profiles/r04e_alloc_ab.json)
    ctx->d_bl[l].reset();
    KHTRY(ctx->d_bl[l].reserve(ctx, bytes));
    HIPCHK(ctx, hipMemset(ctx->d_bl[l].get(), 0, bytes));
  }
  // AMP2[i] = -(M2 + 2i*M2)G, AMP3[i] = -(M3 + 2i*M3)G  (keyhunt.cpp:1818-1842)
  ctx->amp2.resize(32);
  ctx->amp3.resize(32);
  for (int i = 0; i < 32; i++) {
    ge a;
    ctx->comb.mult(a, u256_u64(m2 * (2 * (uint64_t)i + 1)));
    fe_neg(a.y, a.y);
    ctx->amp2[i] = a;
    ctx->comb.mult(a, u256_u64(m3 * (2 * (uint64_t)i + 1)));
    fe_neg(a.y, a.y);
    ctx->amp3[i] = a;
  }
  {
    std::vector<uint32_t> w(32 * 16);
    for (int i = 0; i < 32; i++) {
      memcpy(&w[i * 16], ctx->amp2[i].x.d, 32);
      memcpy(&w[i * 16 + 8], ctx->amp2[i].y.d, 32);
    }
    KHTRY(ctx->d_amp2.reserve(ctx, w.size()));
    KHTRY(ctx->d_ref_start.reserve(ctx, 8));
    HIPCHK(ctx, hipMemcpy(ctx->d_amp2.get(), w.data(), w.size() * 4, hipMemcpyHostToDevice));
  }
  ctx->second_hits = 0;
  ctx->bsgs_ready = true;
  ctx->bsgs_built = false;
  ctx->layer_replaced = false;
  ctx->candidates = 0;
  ctx->second_hits = 0;
  if (info) *info = I;
  return KH_OK;
}

extern "C" int kh_bsgs_set_layer1(kh_ctx *ctx, uint32_t layout) {
  if (!ctx || layout > KH_LAYER1_BLOCKED) return KH_E_ARG;
  ctx->l1_layout = layout;
  return KH_OK;
}

extern "C" int kh_bsgs_set_bloom_multiplier(kh_ctx *ctx, uint32_t mult) {
  if (!ctx || !mult) return KH_E_ARG;
  ctx->bloom_mult = mult;
  return KH_OK;
}

// the baby-step walk (thread_bPload, keyhunt.cpp:5284-5472): babies (i+1)G, i < M, into layer 1
// (bl1/bd1, reference or blocked layout by `mode`), layers 2/3 (the context's) and the bP rows
// baby steps 1..count (count = M unless a single layer is rebuilt) into bl1 with bd1 and, for the
// first M2 / M3 of them, into layers 2 / 3 and the bP rows (m2 = m3 = 0: layer bl1 alone)
int kh_host::build_walk(kh_ctx *ctx, int mode, uint8_t *bl1, const bloom_desc &bd1, uint64_t *d_key, uint32_t *d_val,
                        uint64_t count, bool one_layer) {
  const int H = KH_WALK_H;
  ctx->cont_valid = false;
  const kh_bsgs_info &I = ctx->info;
  if (!count) count = I.m;
  const uint32_t *tab = nullptr;
  KHTRY(get_table(ctx, u256_u64(1), &tab));
  uint64_t total_groups = (count + 2 * H - 1) / (2 * H);
  job_geom jg = plan(ctx, total_groups, 0);
  std::vector<u256> s(jg.L);
  for (uint32_t g = 0; g < jg.L; g++) s[g] = u256_u64(1 + (uint64_t)g * jg.gpl * 2 * H + H);  // baby i <-> key i+1
  KHTRY(run_setup(ctx, s, nullptr));
  walk_args A = walk_on_lanes(ctx, tab, jg, H);
  A.n_points = count;
  A.bl1 = bl1;
  A.bl2 = ctx->d_bl[1].get();
  A.bl3 = ctx->d_bl[2].get();
  A.bd = bd1;
  A.bd2 = ctx->bd[1];
  A.bd3 = ctx->bd[2];
  A.m2 = one_layer ? 0 : I.m2;
  A.m3 = one_layer ? 0 : I.m3;
  A.rows_key = d_key;
  A.rows_val = d_val;
  return run_walk(ctx, mode, 3, A, jg.gpl, 4);
}

extern "C" int kh_bsgs_memory(kh_ctx *ctx, uint64_t *needed_bytes, uint64_t *held_bytes) {
  if (!ctx) return KH_E_ARG;
  if (!ctx->bsgs_ready) return KH_E_STATE;
  uint64_t layers = 0;
  for (int l = 0; l < 3; l++) layers += 256 * ctx->bd[l].stride + 4;
  const uint64_t L = ctx->lanes_max;
  // the giant walk's pad (L x KH_WALK_HB entries of 32 B), lane centres and scalars, the comb, the two
  // rounds' candidate buffers at their current size (16 B per entry, plus the first list's copy), the
  // base list of a kh_bsgs_scan_list call of up to 2^16 bases (32 B each: bsgsd's batch; a longer
  // list adds 32 B per base), and the build's transient row keys (m3 x 12 B).  A round whose
  // candidates overflow doubles its buffers on demand (up to 2^28 entries), which this figure cannot
  // foresee.
  const uint64_t walk = L * (uint64_t)walk_pad_rows(KM_BSGSB, false, KH_WALK_HB) * 32 + L * 32 * 3 + (512u << 10) + 4ull * ctx->cand_cap() * 16 +
                        (1ull << 16) * 32 + ctx->info.m3 * 12;
  if (needed_bytes) *needed_bytes = layers + walk;
  if (held_bytes)
    *held_bytes = layers + (uint64_t)ctx->lanes_alloc() * ctx->scratch_h() * 32 + (uint64_t)ctx->lanes_alloc() * 32 * 3;
  return KH_OK;
}

extern "C" int kh_bsgs_build(kh_ctx *ctx) {
  if (!ctx) return KH_E_ARG;
  if (!ctx->bsgs_ready) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  const kh_bsgs_info &I = ctx->info;
  dev_buf<uint64_t> d_key;
  dev_buf<uint32_t> d_val;
  KHTRY(d_key.reserve(ctx, I.m3));
  KHTRY(d_val.reserve(ctx, I.m3));
  KHTRY(build_walk(ctx, ctx->l1_layout == KH_LAYER1_BLOCKED ? KM_BUILDB : KM_BUILD, ctx->d_bl[0].get(), ctx->bd[0],
                   d_key.get(), d_val.get()));
  // bsgs_sort (keyhunt.cpp:4412-4508): order rows by the 6 value bytes (ties by index)
  std::vector<uint64_t> keys(I.m3);
  std::vector<uint32_t> vals(I.m3);
  KHTRY(download(ctx, keys.data(), d_key, I.m3));
  KHTRY(download(ctx, vals.data(), d_val, I.m3));
  d_key.reset();
  d_val.reset();
  std::vector<uint64_t> order(I.m3);
  for (uint64_t i = 0; i < I.m3; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    return keys[a] != keys[b] ? keys[a] < keys[b] : vals[a] < vals[b];
  });
  ctx->h_rows.assign(I.m3 * 16, 0);
  for (uint64_t i = 0; i < I.m3; i++) {
    uint64_t kk = keys[order[i]];
    uint8_t *row = &ctx->h_rows[i * 16];
    for (int b = 0; b < 6; b++) row[b] = (uint8_t)(kk >> (40 - 8 * b));
    uint64_t idx = vals[order[i]];
    memcpy(row + 8, &idx, 8);
  }
  // layers 2 and 3 on the host for the refinement steps
  for (int l = 1; l < 3; l++) {
    ctx->h_bl[l].resize(256 * ctx->bd[l].stride);
    KHTRY(download(ctx, ctx->h_bl[l].data(), ctx->d_bl[l], ctx->h_bl[l].size()));
  }
  ctx->bsgs_built = true;
  ctx->layer_replaced = false;
  return KH_OK;
}

// ==============================================================================================
// BSGS table files (-S, keyhunt.cpp:1983-2230 read, 2504-2652 write): per layer 256 records of
// {struct bloom (112 B), bit array, checksumsha256 {sha256(bits), same again}} in
// keyhunt_bsgs_4_<M>.blm / _6_<M2>.blm / _7_<M3>.blm, and the sorted bP rows + sha256 in
// keyhunt_bsgs_2_<M3>.tbl.
// ==============================================================================================
namespace {

struct table_path {
  std::string s;
  table_path(const char *dir, int kind, uint64_t m, const char *ext) {
    char name[96];
    snprintf(name, sizeof name, "keyhunt_bsgs_%d_%llu.%s", kind, (unsigned long long)m, ext);
    s = std::string((dir && *dir) ? dir : ".") + "/" + name;
  }
};

// one layer (256 shards at d.stride in `bits`) -> .blm
int write_blm(kh_ctx *c, const std::string &path, const uint8_t *bits, const bloom_desc &d, uint64_t entries) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) {
    c->err = "can't create the file " + path;
    return KH_E_IO;
  }
  uint8_t h[KH_BLOOM_STRUCT], ck[64];
  bloom_header(h, entries, d);
  bool ok = true;
  for (int i = 0; i < 256 && ok; i++) {
    const uint8_t *bf = bits + (size_t)i * d.stride;
    sha256_bytes(bf, d.bytes, ck);
    memcpy(ck + 32, ck, 32);
    ok = fwrite(h, KH_BLOOM_STRUCT, 1, f) == 1 && fwrite(bf, d.bytes, 1, f) == 1 && fwrite(ck, 64, 1, f) == 1;
  }
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    c->err = "error writing the file " + path;
    return KH_E_IO;
  }
  return KH_OK;
}

// .blm -> one layer (256 shards at d.stride in `bits`); headers must carry this geometry
int read_blm(kh_ctx *c, const std::string &path, uint8_t *bits, const bloom_desc &d, uint64_t entries, bool verify) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) {
    c->err = "missing file " + path;
    return KH_E_IO;
  }
  uint8_t h[KH_BLOOM_STRUCT], ck[64], sum[32];
  int rc = KH_OK;
  for (int i = 0; i < 256 && rc == KH_OK; i++) {
    uint8_t *bf = bits + (size_t)i * d.stride;
    if (fread(h, KH_BLOOM_STRUCT, 1, f) != 1) {
      rc = KH_E_IO;
      break;
    }
    uint64_t fe_, fb, fy;
    memcpy(&fe_, h, 8);
    memcpy(&fb, h + 8, 8);
    memcpy(&fy, h + 16, 8);
    if (fe_ != entries || fb != d.bits || fy != d.bytes || h[24] != (uint8_t)d.hashes || h[48] != 1) {
      c->err = "bloom geometry in " + path + " does not match this N/k";
      rc = KH_E_FORMAT;
      break;
    }
    if (fread(bf, d.bytes, 1, f) != 1 || fread(ck, 64, 1, f) != 1) {
      rc = KH_E_IO;
      break;
    }
    if (verify) {
      sha256_bytes(bf, d.bytes, sum);
      if (memcmp(ck, sum, 32) != 0 || memcmp(ck + 32, sum, 32) != 0) {
        c->err = "checksum file mismatch! " + path;
        rc = KH_E_FORMAT;
      }
    }
  }
  if (rc == KH_E_IO) c->err = "error reading the file " + path;
  fclose(f);
  return rc;
}

// layer 1 in the reference layout on the host: the device layer itself, or (blocked layout) a
// reference-layout baby walk into a temporary buffer
int ref_layer1(kh_ctx *c, std::vector<uint8_t> &out) {
  const bloom_desc &d = c->bd_ref1;
  out.assign(256 * d.stride, 0);
  if (c->l1_layout == KH_LAYER1_REFERENCE) return download(c, out.data(), c->d_bl[0], out.size());
  dev_buf<uint8_t> tmp;
  dev_buf<uint64_t> d_key;
  dev_buf<uint32_t> d_val;
  KHTRY(tmp.reserve(c, out.size() + 4));
  KHTRY(d_key.reserve(c, c->info.m3));
  KHTRY(d_val.reserve(c, c->info.m3));
  HIPCHK(c, hipMemset(tmp.get(), 0, out.size() + 4));
  KHTRY(build_walk(c, KM_BUILD, tmp.get(), d, d_key.get(), d_val.get()));
  return download(c, out.data(), tmp, out.size());
}

}  // namespace

extern "C" int kh_bsgs_save(kh_ctx *ctx, const char *dir) {
  if (!ctx) return KH_E_ARG;
  if (!ctx->bsgs_built) return KH_E_STATE;
  if (ctx->layer_replaced) {
    ctx->err = "a layer was replaced by kh_bsgs_set_bloom: build or load the tables again before saving them";
    return KH_E_STATE;
  }
  (void)hipSetDevice(ctx->device);
  const kh_bsgs_info &I = ctx->info;
  std::vector<uint8_t> l1;
  KHTRY(ref_layer1(ctx, l1));
  KHTRY(write_blm(ctx, table_path(dir, 4, I.m, "blm").s, l1.data(), ctx->bd_ref1, ctx->entries[0]));
  l1.clear();
  l1.shrink_to_fit();
  KHTRY(write_blm(ctx, table_path(dir, 6, I.m2, "blm").s, ctx->h_bl[1].data(), ctx->bd[1], ctx->entries[1]));
  KHTRY(write_blm(ctx, table_path(dir, 7, I.m3, "blm").s, ctx->h_bl[2].data(), ctx->bd[2], ctx->entries[2]));
  const std::string tp = table_path(dir, 2, I.m3, "tbl").s;
  FILE *f = fopen(tp.c_str(), "wb");
  if (!f) {
    ctx->err = "can't create the file " + tp;
    return KH_E_IO;
  }
  uint8_t ck[32];
  sha256_bytes(ctx->h_rows.data(), ctx->h_rows.size(), ck);
  bool ok = fwrite(ctx->h_rows.data(), ctx->h_rows.size(), 1, f) == 1 && fwrite(ck, 32, 1, f) == 1;
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    ctx->err = "error writing the file " + tp;
    return KH_E_IO;
  }
  return KH_OK;
}

extern "C" int kh_bsgs_load(kh_ctx *ctx, const char *dir, uint32_t flags) {
  if (!ctx) return KH_E_ARG;
  if (!ctx->bsgs_ready) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  const kh_bsgs_info &I = ctx->info;
  const bool verify = !(flags & KH_LOAD_SKIP_CHECKSUM);
  ctx->bsgs_built = false;
  // bP table
  const std::string tp = table_path(dir, 2, I.m3, "tbl").s;
  std::vector<uint8_t> rows(I.m3 * 16);
  {
    FILE *f = fopen(tp.c_str(), "rb");
    if (!f) {
      ctx->err = "missing file " + tp;
      return KH_E_IO;
    }
    uint8_t ck[32], sum[32];
    bool ok = fread(rows.data(), rows.size(), 1, f) == 1 && fread(ck, 32, 1, f) == 1;
    fclose(f);
    if (!ok) {
      ctx->err = "error reading the file " + tp;
      return KH_E_IO;
    }
    if (verify) {
      sha256_bytes(rows.data(), rows.size(), sum);
      if (memcmp(ck, sum, 32) != 0) {
        ctx->err = "checksum file mismatch! " + tp;
        return KH_E_FORMAT;
      }
    }
  }
  // layers 2 and 3 (host copies serve the refinement)
  for (int l = 1; l < 3; l++) {
    std::vector<uint8_t> &h = ctx->h_bl[l];
    h.assign(256 * ctx->bd[l].stride, 0);
    KHTRY(read_blm(ctx, table_path(dir, l == 1 ? 6 : 7, l == 1 ? I.m2 : I.m3, "blm").s, h.data(), ctx->bd[l],
                   ctx->entries[l], verify));
    HIPCHK(ctx, hipMemcpy(ctx->d_bl[l].get(), h.data(), h.size(), hipMemcpyHostToDevice));
  }
  // layer 1: the file's bits for the reference layout; the blocked layout is rebuilt on the GPU
  // (its bits are not in any reference file), after checking the file all the same
  {
    std::vector<uint8_t> l1(256 * ctx->bd_ref1.stride, 0);
    KHTRY(read_blm(ctx, table_path(dir, 4, I.m, "blm").s, l1.data(), ctx->bd_ref1, ctx->entries[0], verify));
    if (ctx->l1_layout == KH_LAYER1_REFERENCE) {
      HIPCHK(ctx, hipMemcpy(ctx->d_bl[0].get(), l1.data(), l1.size(), hipMemcpyHostToDevice));
    } else {
      dev_buf<uint64_t> d_key;
      dev_buf<uint32_t> d_val;
      KHTRY(d_key.reserve(ctx, I.m3));
      KHTRY(d_val.reserve(ctx, I.m3));
      HIPCHK(ctx, hipMemset(ctx->d_bl[0].get(), 0, 256 * ctx->bd[0].stride + 4));
      int r = build_walk(ctx, KM_BUILDB, ctx->d_bl[0].get(), ctx->bd[0], d_key.get(), d_val.get());
      d_key.reset();
      d_val.reset();
      if (r) return r;
    }
  }
  ctx->h_rows.swap(rows);
  ctx->bsgs_built = true;
  ctx->layer_replaced = false;
  return KH_OK;
}

extern "C" int kh_bsgs_set_targets(kh_ctx *ctx, const uint8_t *xy, uint32_t n) {
  if (!ctx || (!xy && n)) return KH_E_ARG;
  ctx->cont_valid = false;
  ctx->targets.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    fe_from_be(ctx->targets[i].x, xy + 64 * i);
    fe_from_be(ctx->targets[i].y, xy + 64 * i + 32);
  }
  ctx->found.assign(n, 0);
  return KH_OK;
}

extern "C" int kh_bsgs_reset_found(kh_ctx *ctx) {
  if (!ctx) return KH_E_ARG;
  std::fill(ctx->found.begin(), ctx->found.end(), 0);
  return KH_OK;
}

extern "C" int kh_bsgs_refine_stats(kh_ctx *ctx, uint64_t *first_level, uint64_t *second_level) {
  if (!ctx || !first_level || !second_level) return KH_E_ARG;
  *first_level = ctx->candidates;
  *second_level = ctx->second_hits;
  return KH_OK;
}

extern "C" int kh_bsgs_candidates(kh_ctx *ctx, uint64_t *count) {
  if (!ctx || !count) return KH_E_ARG;
  *count = ctx->candidates;
  return KH_OK;
}

namespace {

bool rows_search(const kh_ctx *c, const uint8_t x32[32], uint64_t &idx) {
  // bsgs_searchbinary (keyhunt.cpp:4510-4544), no bucket cache
  const uint8_t *rows = c->h_rows.data();
  int64_t n = (int64_t)c->info.m3, min = 0, max = n, cur = 0, half = n;
  while (half >= 1) {
    half = (max - min) / 2;
    const uint8_t *row = rows + (cur + half) * 16;
    int cmp = memcmp(x32 + 16, row, 6);
    if (cmp == 0) {
      memcpy(&idx, row + 8, 8);
      return true;
    }
    if (cmp < 0)
      max = max - half;
    else
      min = min + half;
    cur = min;
  }
  return false;
}

// S + A[i] for i < 32, X only, one batched inversion.  AddDirect with dx == 0 yields
// x = -S.x - A.x in the reference (inverse of 0 is 0); reproduced.
void add32_x(const ge &S, const std::vector<ge> &A, fe out[32]) {
  std::vector<fe> dx(32);
  for (int i = 0; i < 32; i++) fe_sub(dx[i], A[i].x, S.x);
  batch_inv(dx);
  for (int i = 0; i < 32; i++) {
    fe dy, s, x;
    fe_sub(dy, A[i].y, S.y);
    fe_mul(s, dy, dx[i]);
    fe_sqr(x, s);
    fe_sub(x, x, S.x);
    fe_sub(x, x, A[i].x);
    out[i] = x;
  }
}

// bsgs_thirdcheck (keyhunt.cpp:5186-5248)
bool third_check(const kh_ctx *c, const u256 &base_key, uint32_t a, const ge &Q, u256 &key) {
  const kh_bsgs_info &I = c->info;
  u256 base3 = sc_add(base_key, sc_reduce(u256_from_u128((u128)a * 2 * I.m2)));
  ge bp;
  if (!c->comb.mult(bp, base3)) return false;
  fe_neg(bp.y, bp.y);
  ge S;
  ge_add(S, Q, bp);
  fe xs[32];
  add32_x(S, c->amp3, xs);
  for (int i = 0; i < 32; i++) {
    uint8_t xr[32];
    fe_to_be(xr, xs[i]);
    u256 calc = u256_u64(i == 0 ? I.m3 : (uint64_t)i * 2 * I.m3 + I.m3);
    if (host_bloom_check(c->h_bl[2].data() + (size_t)xr[0] * c->bd[2].stride, c->bd[2], xr, 32)) {
      uint64_t j;
      if (rows_search(c, xr, j)) {
        for (int sgn = 0; sgn < 2; sgn++) {
          u256 jj = u256_u64(j + 1);
          u256 k = sgn == 0 ? sc_add(calc, jj) : sc_sub(calc, jj);
          k = sc_add(k, base3);
          ge chk;
          if (c->comb.mult(chk, k) && fe_eq(chk.x, Q.x)) {
            key = k;
            return true;
          }
        }
      }
    } else if (fe_eq(S.x, c->amp3[i].x)) {
      key = sc_add(calc, base3);
      return true;
    }
  }
  return false;
}

// bsgs_secondcheck (keyhunt.cpp:5151-5184) in two halves.  second_mask: the layer-2 hits of the
// 32 points S + AMP2[i] (S = Q - base_key*G) as a bit mask -- the host twin of k_refine;
// second_finish: the reference's loop over those hits, calling bsgs_thirdcheck in order.
u256 second_base_key(const kh_ctx *c, const u256 &base, uint64_t a) {
  return sc_add(base, sc_reduce(u256_from_u128((u128)a * 2 * c->info.m)));
}
bool second_finish(const kh_ctx *c, const u256 &base_key, uint32_t mask, const ge &Q, u256 &key) {
  for (int i = 0; i < 32; i++)
    if (((mask >> i) & 1) && third_check(c, base_key, (uint32_t)i, Q, key)) return true;
  return false;
}

}  // namespace

uint32_t kh_host::second_mask(const kh_ctx *c, const u256 &base_key, const ge &Q) {
  ge bp;
  if (!c->comb.mult(bp, base_key)) return 0;
  fe_neg(bp.y, bp.y);
  ge S;
  ge_add(S, Q, bp);
  fe xs[32];
  add32_x(S, c->amp2, xs);
  uint32_t mask = 0;
  for (int i = 0; i < 32; i++) {
    uint8_t xr[32];
    fe_to_be(xr, xs[i]);
    if (host_bloom_check(c->h_bl[1].data() + (size_t)xr[0] * c->bd[1].stride, c->bd[1], xr, 32)) mask |= 1u << i;
  }
  return mask;
}

namespace {

// the two rounds' candidate buffers, pinned mirrors, events and host scalar arrays, and the lanes
int ensure_pipeline(kh_ctx *c, uint32_t L, int H) {
  const uint32_t cand = c->cand_cap();
  for (int i = 0; i < 2; i++) {
    KHTRY(c->d_cnt2[i].reserve(c, 1));
    KHTRY(c->d_hits2[i].reserve(c, cand));
    KHTRY(c->h_cnt2[i].reserve(c, 1));
    KHTRY(c->h_hits2[i].reserve(c, cand));
    for (int j = 0; j < 4; j++) KHTRY(c->ev_round[i][j].create(c));
  }
  for (int i = 0; i < 2; i++) KHTRY(c->h_scal2[i].reserve(c, (size_t)L * 8));
  return ensure_lanes(c, L, walk_pad_rows(KM_BSGSB, false, H));  // the giant walks' sparse pad
}

// candidates copied back with each round's count; more are fetched on demand
constexpr uint32_t KH_CAND_EAGER = 4096;

struct bsgs_round {
  uint64_t g0, rg;   // rounds over bases: walk groups [g0, g0 + rg) of this call;
                     // continuous mode: groups [g0, g0 + rg) of every lane
  uint64_t t_round;  // giant index of the round's point 0 (continuous mode: 0, indices are global)
  uint32_t L;
  uint64_t gpl;
  uint32_t launches;
  uint64_t points;
  bool setup;        // the round (re)started its lanes
};

// giant points per pipelined round of continuous mode: 2^34 (2^21 lanes x 2 groups of 4096, one
// launch).  Every launch starts its first batch of waves in phase; two groups per lane per launch
// walked 41.1 G giant points/s against 40.05 at one (2^33) and 40.7 at four (2^35), three repeats each,
// spread 0.05 % (profiles/r05ae_round_ab.json); in the bench's BSGS leg four groups ran 43.0 vs 40.1
// at one on another box (r05ab_bench_round_points.json); eight groups per launch lost 1-14 %
constexpr uint64_t KH_BSGS_ROUND_POINTS = 1ULL << 34;

// The giant-step scan behind kh_bsgs_scan (bases start + b*2N) and kh_bsgs_scan_list (any bases): one
// call's constants, the round state of the target being walked, and the keys found.  run() goes
// through geometry(), bases() and, per target, scan_target() (enqueue / finish, pipelined).
struct bsgs_scan {
  // the call
  kh_ctx *const ctx;
  const u256 st;
  const std::vector<u256> *const list;
  const uint64_t n_bases;
  kh_bsgs_found *const found;
  const uint32_t cap;
  const kh_bsgs_info &I;
  const uint64_t A_pts;  // giant points walked per base (cycles x 1024)
  // Continuous mode: when a base's walk ends exactly where the next base's starts (cycles*1024 ==
  // aux, every power-of-two k), P_t = Q - (start + M + 2M t)G is ONE progression over the whole
  // call.  Lanes then own long runs of t, start once, and every round just continues them.
  // Otherwise (bases overlap, SURVEY parity note 13) rounds restart lanes per base run.
  const bool cont;
  // group half-size: the large groups (one inversion per 2*KH_WALK_HB points) whenever a base holds
  // whole ones (every power-of-two k >= 16); otherwise the reference's 1024-point group
  const int H;
  // giant points of this call: t in [0, n_bases*A); t -> base b = t / A, a = t % A; the centre
  // of a group whose first point is t sits at key base_b + M + 2M*(a + H).
  const uint64_t gpb;  // walk groups per base
  const uint64_t total_groups;
  // second check on the GPU: the kernel derives base_key from the candidate's giant index
  const bool gpu_refine;
  // geometry()
  const uint32_t *tab = nullptr;
  uint32_t per_launch = 2, lanes = 0;
  job_geom jc{};
  uint64_t gpr = 0;  // continuous mode: groups per lane per round
  bool keep_lanes = false;
  // bases()
  bool dev_centres = false;
  // the target being walked
  uint32_t tgt = 0;
  ge Q{};
  uint64_t g_end = 0, g0 = 0;
  bool need_setup = true, done = false;
  bsgs_round rounds[2];
  // keys found
  uint32_t nf = 0;

  bsgs_scan(kh_ctx *c, const u256 &start, const std::vector<u256> *bases_list, uint64_t n, kh_bsgs_found *out,
            uint32_t out_cap)
      : ctx(c), st(start), list(bases_list), n_bases(n), found(out), cap(out_cap), I(c->info),
        A_pts(I.cycles * 1024), cont(!list && A_pts == I.aux),
        H((A_pts % (2 * KH_WALK_HB) == 0 && !getenv("KH_NO_BIG_GROUPS")) ? KH_WALK_HB : KH_WALK_H),
        gpb(A_pts / (2 * H)), total_groups(n_bases * gpb), gpu_refine(!c->refine_host) {}

  u256 base_of(uint64_t b) const {
    return list ? (*list)[b] : sc_add(st, sc_reduce(u256_from_u128((u128)b * 2 * I.n)));
  }
  u256 centre_scalar(uint64_t t0) const {  // -(key of the centre of the group starting at t0)
    uint64_t b = t0 / A_pts, a0 = t0 % A_pts;
    u256 kb = sc_add(base_of(b), sc_reduce(u256_from_u128((u128)I.m + (u128)2 * I.m * (a0 + H))));
    return sc_neg(kb);
  }
  u256 key_of(const bsgs_round &R, const kh_dev_hit &h) const {  // base key of a first-level candidate
    uint64_t t = R.t_round + h.idx;
    return second_base_key(ctx, base_of(t / A_pts), t % A_pts);
  }

  // lanes per launch: lanes_bsgs (2^21: eight waves per wave slot in turn, kh_kernels.h) for the
  // large groups when the call holds that many groups and the device has room for their pad, else
  // the largest power of two below it that fits (down to lanes_max, 2^18: one wave per slot).  The
  // count must tile the call (geometry()): plan()'s balanced count for a 7274496-base call (1039214
  // lanes) walked 6 % slower than 2^20 (profiles/r05q_geom_lanes_count.json)
  void pick_lanes() {
    lanes = ctx->lanes_max;
    uint32_t wide = ctx->lanes_force ? ctx->lanes_force : ctx->lanes_pick ? ctx->lanes_pick : ctx->lanes_bsgs;
    if (const char *e = getenv("KH_BSGS_LANES")) wide = (uint32_t)strtoul(e, nullptr, 0);  // A/B knob
    if (getenv("KH_BSGS_NARROW")) wide = lanes;
    if (H == KH_WALK_HB) {
      // a wider geometry is taken only if it leaves 32 GB of the device free for other contexts (their
      // tables are built while this one walks: `-g N` on one GPU)
      const uint64_t rows = (uint64_t)walk_pad_rows(KM_BSGSB, false, H);
      const uint64_t have =
          ctx->lanes_alloc() >= lanes ? (uint64_t)ctx->lanes_alloc() * ((uint64_t)ctx->scratch_h() * 32 + 96) : 0;
      size_t fr = 0, tot = 0;
      const bool known = hipMemGetInfo(&fr, &tot) == hipSuccess;
      for (uint32_t w = wide; w > lanes; w >>= 1) {
        if (total_groups < w) continue;
        const uint64_t need = (uint64_t)w * (rows * 32 + 96);
        if (known && need > have && fr + have < need + (32ull << 30)) continue;
        if (ensure_pipeline(ctx, w, H) == KH_OK) {
          lanes = w;
          break;
        }
        (void)hipGetLastError();  // out of device memory (other contexts): a smaller geometry
        ctx->err.clear();
      }
    }
    ctx->lanes_used = H == KH_WALK_HB ? lanes : 0;
  }

  // step 1: the delta table, groups per launch, lanes, and continuous mode's tiling of the call
  int geometry() {
    // GSn[i] = -(i+1)*2M*G  (keyhunt.cpp:1797-1816)
    KHTRY(get_table(ctx, sc_neg(u256_u64(2 * I.m)), &tab, H));
    // two groups per lane per launch (KH_BSGS_ROUND_POINTS above): per-base rounds too
    per_launch = ctx->groups_per_launch ? ctx->groups_per_launch : 2;
    if (const char *e = getenv("KH_BSGS_GROUPS_PER_LAUNCH")) per_launch = std::max(1u, (uint32_t)strtoul(e, nullptr, 0));  // A/B knob
    pick_lanes();
    if (!cont) {
      ctx->cont_valid = false;
      return KH_OK;
    }
    // interleaved lanes: lane g walks groups g, g + L, g + 2L, ... of the call, so after the call
    // it sits on group g of the call that starts where this one ends (kept across calls)
    jc = plan(ctx, total_groups, 0, lanes);
    // keep the power-of-two lane count when the ragged last round (lanes past the call's end walk
    // unprobed) costs at most 1/32 of the call: the balanced count plan() picks otherwise (e.g.
    // 1039214 lanes for a 7274496-base call) walked 6 % slower than 2^20 lanes, interleaved on one
    // box (profiles/r05q_geom_lanes_count.json)
    if (total_groups >= lanes) {
      const uint64_t gpl = (total_groups + lanes - 1) / lanes;
      if ((gpl * lanes - total_groups) * 32 <= total_groups) {
        jc.L = lanes;
        jc.gpl = gpl;
      }
    }
    uint64_t round_pts = KH_BSGS_ROUND_POINTS;
    if (const char *e = getenv("KH_BSGS_ROUND_POINTS")) round_pts = strtoull(e, nullptr, 0);  // A/B knob
    gpr = std::max<uint64_t>(1, round_pts / ((uint64_t)jc.L * 2 * H));
    gpr = std::min<uint64_t>(gpr, jc.gpl);
    KHTRY(get_table(ctx, sc_neg(u256_u64(2 * I.m)), &tab, H, jc.L));
    // lane g ends the call on group g + gpl*L of it: the first group of the next call only when the
    // lanes tile the call exactly (else a following call starts its lanes again)
    keep_lanes = ctx->targets.size() == 1 && (uint64_t)jc.L * jc.gpl == total_groups;
    return KH_OK;
  }

  // step 2: where the lane centres' scalars are derived, and the start / the base list on the device
  int bases() {
    // per-base rounds derive their lane scalars on the device (k_setup prog 2) unless a centre key can
    // reach n (key = base + M + 2M*(a0 + H) <= base + vmax; 0 mod n only at base + v = n) or
    // KH_HOST_CENTRES is set; the host loop cost ~50 ns per lane, 2^18 lanes a round
    dev_centres = !cont && !getenv("KH_HOST_CENTRES");
    const u256 vmax = u256_from_u128((u128)I.m * (2 * (A_pts + H) + 1));
    if (dev_centres && !list) {
      u256 top;
      dev_centres = !u256_add_raw(top, st, vmax) && !reaches_order(top, u256_from_u128((u128)2 * I.n), n_bases - 1);
    }
    if (list) {
      // the bases as device limbs, packed on the host threads into a pinned buffer (a serial pass over
      // 2^20 bases and a pageable copy took ~15 ms of each CLI call), with the centre-key check
      if (n_bases * 8 > ctx->d_ref_list.cap() || n_bases * 8 > ctx->h_ref_list.cap()) {
        ctx->d_ref_list.reset();
        ctx->h_ref_list.reset();
        KHTRY(ctx->d_ref_list.reserve(ctx, (size_t)n_bases * 8));
        KHTRY(ctx->h_ref_list.reserve(ctx, (size_t)n_bases * 8));
      }
      u256 thr;
      u256_sub_raw(thr, ORDER_N, vmax);
      std::atomic<bool> risky{false};
      uint32_t *hl = ctx->h_ref_list.get();
      parallel_for(n_bases, host_threads(ctx), [&](uint64_t lo, uint64_t hi) {
        bool r = false;
        for (uint64_t b = lo; b < hi; b++) {
          u256_to_limbs(hl + b * 8, (*list)[b]);
          r |= u256_cmp((*list)[b], thr) >= 0;
        }
        if (r) risky = true;
      });
      if (risky) dev_centres = false;
    }
    if (gpu_refine || dev_centres) {
      uint32_t sl[8];
      u256_to_limbs(sl, st);
      HIPCHK(ctx, hipMemcpyAsync(ctx->d_ref_start.get(), sl, 32, hipMemcpyHostToDevice, ctx->stream));
      if (list)
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_ref_list.get(), ctx->h_ref_list.get(), (size_t)n_bases * 32,
                                   hipMemcpyHostToDevice, ctx->stream));
    }
    return KH_OK;
  }

  // (re)start the round's lanes on their first centres: C_g = Q - (centre key)*G
  int start_lanes(int slot, const bsgs_round &R) {
    setup_args S = setup_on_lanes(ctx, R.L);
    if (dev_centres) {
      S.prog = 2;
      S.list = list ? ctx->d_ref_list.get() : nullptr;
      S.start = ctx->d_ref_start.get();
      S.t_round = R.t_round;
      S.lane_pts = R.gpl * 2 * H;
      S.a_pts = A_pts;
      S.two_n = 2 * I.n;
      S.m = I.m;
      S.h = (uint32_t)H;
    } else {
      uint32_t *hs = ctx->h_scal2[slot].get();
      for (uint32_t g = 0; g < R.L; g++) {
        uint64_t t0 = cont ? (R.g0 * jc.L + g) * 2 * H : R.t_round + (uint64_t)g * R.gpl * 2 * H;
        u256_to_limbs(hs + (size_t)g * 8, centre_scalar(t0));
      }
      HIPCHK(ctx, hipMemcpyAsync(ctx->d_scalars.get(), hs, (size_t)R.L * 32, hipMemcpyHostToDevice, ctx->stream));
    }
    S.scalars = ctx->d_scalars.get();
    S.q = ctx->d_q.get();
    S.has_q = 1;
    HIPCHK(ctx, hipEventRecord(ctx->ev_round[slot][0].get(), ctx->stream));
    HIPCHK(ctx, launch_setup(S, ctx->stream));
    return KH_OK;
  }

  // the round's giant walk: per_launch groups per lane a launch, candidates into the slot's buffer
  int walk_round(int slot, bsgs_round &R) {
    walk_args Aw = walk_on_lanes(ctx, tab, job_geom{R.L, R.gpl}, H);
    Aw.interleave = cont ? 1 : 0;
    Aw.n_points = cont ? total_groups * 2 * H : R.rg * 2 * H;
    Aw.bloom = ctx->d_bl[0].get();
    Aw.bd = ctx->bd[0];
    Aw.bstride32 = (uint32_t)ctx->bd[0].stride;  // < 2^32: checked by kh_bsgs_setup
    Aw.hit_count = ctx->d_cnt2[slot].get();
    Aw.hits = ctx->d_hits2[slot].get();
    Aw.hit_cap = ctx->cand_cap();
    R.launches = 0;
    R.points = 0;
    const uint64_t gb0 = cont ? R.g0 : 0, gb1 = cont ? R.g0 + R.rg : R.gpl;
    for (uint64_t gb = gb0; gb < gb1; gb += per_launch) {
      Aw.group_base = gb;
      Aw.groups = (uint32_t)std::min<uint64_t>(per_launch, gb1 - gb);
      HIPCHK(ctx, launch_walk(ctx->info.layer1_layout == KH_LAYER1_BLOCKED ? KM_BSGSB : KM_BSGS, Aw, ctx->stream, H));
      R.launches++;
      // probed points: continuous mode's ragged last round walks lanes past the call unprobed
      uint64_t real = (uint64_t)R.L * Aw.groups;
      if (cont) {
        const uint64_t lo = gb * R.L, hi = std::min<uint64_t>((gb + Aw.groups) * R.L, total_groups);
        real = hi > lo ? hi - lo : 0;
      }
      R.points += real * 2 * H;
    }
    return KH_OK;
  }

  // on the side stream: the second check of the round's candidates, in place (aux = layer-2 mask),
  // and the copies of their count and the first KH_CAND_EAGER of them
  int refine_round(int slot, const bsgs_round &R) {
    if (gpu_refine) {
      refine_args Ra;
      memset(&Ra, 0, sizeof Ra);
      Ra.cands = ctx->d_hits2[slot].get();
      Ra.count = ctx->d_cnt2[slot].get();
      Ra.cap = ctx->cand_cap();
      Ra.list_mode = list ? 1 : 0;
      Ra.t_round = R.t_round;
      Ra.a_pts = A_pts;
      Ra.two_n = 2 * I.n;
      Ra.two_m = 2 * I.m;
      Ra.start = ctx->d_ref_start.get();
      Ra.list = ctx->d_ref_list.get();
      Ra.comb = ctx->d_comb.get();
      Ra.q = ctx->d_q.get();
      Ra.amp2 = ctx->d_amp2.get();
      Ra.bloom2 = ctx->d_bl[1].get();
      Ra.bd2 = ctx->bd[1];
      HIPCHK(ctx, launch_refine(Ra, ctx->side));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_cnt2[slot].get(), ctx->d_cnt2[slot].get(), 4, hipMemcpyDeviceToHost, ctx->side));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_hits2[slot].get(), ctx->d_hits2[slot].get(),
                               (size_t)std::min(ctx->cand_cap(), KH_CAND_EAGER) * sizeof(kh_dev_hit),
                               hipMemcpyDeviceToHost, ctx->side));
    return KH_OK;
  }

  // step 3a: plan the round that starts at group g0 and put it on the streams
  int enqueue(int slot) {
    bsgs_round &R = rounds[slot];
    job_geom jg;
    if (cont) {
      R.rg = std::min<uint64_t>(g_end - g0, gpr);
      jg = jc;
      R.t_round = 0;
    } else {
      // per-base rounds (list mode, overlapping bases): up to `lanes` bases per round, each lane
      // walking a divisor of gpb groups (plan), so large calls start one lane per base and small
      // ones still fill ~lanes_max lanes
      R.rg = std::min<uint64_t>(g_end - g0, (uint64_t)lanes * gpb);
      jg = plan(ctx, R.rg, gpb, lanes);  // a lane's run never crosses a base
      R.t_round = g0 * 2 * H;
    }
    R.g0 = g0;
    R.L = jg.L;
    R.gpl = jg.gpl;
    KHTRY(ensure_pipeline(ctx, jg.L, H));
    R.setup = !cont || need_setup;
    if (R.setup) {
      KHTRY(start_lanes(slot, R));
      need_setup = false;
    } else {
      HIPCHK(ctx, hipEventRecord(ctx->ev_round[slot][0].get(), ctx->stream));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_round[slot][1].get(), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_cnt2[slot].get(), 0, 4, ctx->stream));
    KHTRY(walk_round(slot, R));
    HIPCHK(ctx, hipEventRecord(ctx->ev_round[slot][2].get(), ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_round[slot][2].get(), 0));
    KHTRY(refine_round(slot, R));
    HIPCHK(ctx, hipEventRecord(ctx->ev_round[slot][3].get(), ctx->side));
    g0 += R.rg;
    return KH_OK;
  }

  // layer-2 masks on host threads (KH_REFINE=host)
  void host_masks(const bsgs_round &R, std::vector<kh_dev_hit> &dh) {
    std::atomic<size_t> next{0};
    auto work = [&]() {
      for (;;) {
        size_t i = next++;
        if (i >= dh.size()) break;
        dh[i].aux = second_mask(ctx, key_of(R, dh[i]), Q);
      }
    };
    unsigned nt = std::min<unsigned>(host_threads(ctx), (unsigned)dh.size());
    if (nt <= 1) {
      work();
    } else {
      std::vector<std::thread> th;
      for (unsigned k = 0; k < nt; k++) th.emplace_back(work);
      for (auto &x : th) x.join();
    }
  }

  // the round's candidates (sorted by giant index, aux = layer-2 mask): third checks for the (rare)
  // layer-2 hits, in giant-step order; the first candidate that refines to a key ends the target
  void refine(const bsgs_round &R, const std::vector<kh_dev_hit> &dh) {
    if (ctx->log_cands)
      for (auto &h : dh) {
        const uint64_t t = R.t_round + h.idx;
        ctx->cand_log_base.push_back(t / A_pts);
        ctx->cand_log_a.push_back((uint32_t)(t % A_pts));
        ctx->cand_log_mask.push_back(h.aux);
      }
    u256 key{};
    for (size_t i = 0; i < dh.size() && !done; i++) {
      const uint64_t t = R.t_round + dh[i].idx;
      if (ctx->base_check && t % A_pts == 0) {
        // bsgsd's test of each base point against the target (bsgsd.cpp:2544-2561): a key at the
        // very start of a base is a candidate at a = 0 whose S = Q - base*G is the point at
        // infinity, which no second check can refine (the CLI misses it, bsgsd reports it)
        const u256 b = base_of(t / A_pts);
        ge bp;
        if (ctx->comb.mult(bp, b) && fe_eq(bp.x, Q.x) && fe_eq(bp.y, Q.y)) {
          key = b;
          done = true;
          break;
        }
      }
      if (!dh[i].aux) continue;
      ctx->second_hits += (uint64_t)__builtin_popcount(dh[i].aux);
      done = second_finish(ctx, key_of(R, dh[i]), dh[i].aux, Q, key);
    }
    if (!done) return;
    ctx->found[tgt] = 1;
    if (found && nf < cap) {
      found[nf].target = tgt;
      found[nf].pad = 0;
      u256_to_be(found[nf].key, key);
    }
    nf++;
  }

  // step 3b: wait for round `slot`, account its time, refine its candidates.  Returns 1 when the
  // round overflowed the candidate buffer: the buffers were grown and the caller redoes it.
  int finish(int slot) {
    const bsgs_round &R = rounds[slot];
    gpu_event *ev = ctx->ev_round[slot];
    // ev[3] follows the walk and the candidate copies of this round only
    HIPCHK(ctx, hipEventSynchronize(ev[3].get()));
    if (R.setup) ctx->tm[4].add(ev[0].get(), ev[1].get(), 1, R.L);
    ctx->tm[2].add(ev[1].get(), ev[2].get(), R.launches, R.points);
    const uint32_t cnt = *ctx->h_cnt2[slot].get();
    if (cnt > ctx->cand_cap()) {
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // drain the speculative next round
      HIPCHK(ctx, hipStreamSynchronize(ctx->side));
      uint64_t grown = ctx->cand_cap();
      while (grown < (uint64_t)cnt * 2) grown *= 2;
      int rr = grow_hits(ctx, grown, 1u << 28, ctx->d_hits2, ctx->h_hits2, 2);
      if (rr == KH_E_OVERFLOW) ctx->err = "first-level candidates per round exceed 2^28";
      return rr ? rr : 1;
    }
    kh_dev_hit *hh = ctx->h_hits2[slot].get();
    if (cnt > KH_CAND_EAGER)
      HIPCHK(ctx, hipMemcpy(hh + KH_CAND_EAGER, ctx->d_hits2[slot].get() + KH_CAND_EAGER,
                            (size_t)(cnt - KH_CAND_EAGER) * sizeof(kh_dev_hit), hipMemcpyDeviceToHost));
    std::vector<kh_dev_hit> dh(hh, hh + cnt);
    std::sort(dh.begin(), dh.end(), [](const kh_dev_hit &x, const kh_dev_hit &y) { return x.idx < y.idx; });
    ctx->candidates += cnt;
    if (!gpu_refine) host_masks(R, dh);
    refine(R, dh);
    return KH_OK;
  }

  // step 3: one target.  Rounds are pipelined: the GPU walks round r+1 while the host refines round
  // r's first-level candidates.  Step 4: lanes that walked the whole call are handed to the next one.
  int scan_target() {
    Q = ctx->targets[tgt];
    g_end = cont ? jc.gpl : total_groups;
    g0 = 0;
    // continuous mode: (re)start the lanes at group g0, unless the previous call left them here
    need_setup = !(keep_lanes && ctx->cont_valid && ctx->cont_kind == 0 && ctx->cont_tgt == tgt &&
                   ctx->cont_L == jc.L && ctx->cont_H == H && u256_cmp(ctx->cont_next, st) == 0);
    ctx->cont_valid = false;
    done = false;
    int cur = 0, pending = -1;
    uint32_t Qw[16];
    memcpy(Qw, Q.x.d, 32);
    memcpy(Qw + 8, Q.y.d, 32);
    KHTRY(ctx->d_q.reserve(ctx, 16));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_q.get(), Qw, 64, hipMemcpyHostToDevice, ctx->stream));
    while ((g0 < g_end || pending >= 0) && !done) {
      int nxt = -1;
      if (g0 < g_end) {
        KHTRY(enqueue(cur));
        nxt = cur;
        cur ^= 1;
      }
      if (pending >= 0) {
        const uint64_t redo = rounds[pending].g0;
        int r = finish(pending);
        if (r == 1) {  // overflowed: walk again from that round with the larger buffers
          g0 = redo;
          need_setup = true;  // continuous mode: the lanes already moved past it
          pending = -1;
          continue;
        }
        if (r) return r;
      }
      pending = nxt;
    }
    if (pending >= 0 && done) {  // drain the speculative round
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipStreamSynchronize(ctx->side);
    }
    if (keep_lanes && !done && g0 == g_end) {  // every lane walked all its groups of this call
      ctx->cont_valid = true;
      ctx->cont_kind = 0;
      ctx->cont_next = sc_add(st, sc_reduce(u256_from_u128((u128)n_bases * 2 * I.n)));
      ctx->cont_tgt = tgt;
      ctx->cont_L = jc.L;
      ctx->cont_H = H;
    }
    return KH_OK;
  }

  int run() {
    KHTRY(geometry());
    KHTRY(bases());
    for (tgt = 0; tgt < ctx->targets.size(); tgt++)
      if (!ctx->found[tgt]) KHTRY(scan_target());
    return KH_OK;
  }
};

int bsgs_scan_one(kh_ctx *ctx, const u256 &st, const std::vector<u256> *list, uint64_t n_bases, kh_bsgs_found *found,
                  uint32_t cap, uint32_t *n_found) {
  if (!ctx->bsgs_built) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  *n_found = 0;
  if (n_bases == 0) return KH_OK;
  bsgs_scan s(ctx, st, list, n_bases, found, cap);
  KHTRY(s.run());
  *n_found = s.nf;
  return s.nf > cap ? KH_E_OVERFLOW : KH_OK;
}

// The giant walk's rate depends on where its 64-GB inversion pad (and on some boxes its layer 1) land in
// physical memory and on the box: the same process walks 1-8 % faster on one allocation of the pad than
// on another, with identical instruction and request counts; the slow placements show only longer L2
// request latencies in cycles at a higher clock (DESIGN.md §2 "Placement", profiles/r06f_state_counters.json,
// r06j_buffer_replacement.json).  A context's first continuous call of at least 2^23 walk groups therefore
// calibrates: it walks the call's four parts on two candidate placements in the order A B B A, so a
// linear drift of clock or power cancels, times each part on the walk's events and keeps the faster.
// The candidates are 2^21 and 2^20 lanes on the one pad (2^20 lanes walk its first half: other
// physical pages) -- the form that measured best over five boxes (profiles/r06n..r06q_calibration_ab.json:
// 41.2 G giant points/s mean against 40.7 uncalibrated, never below 39.4).
// KH_BSGS_CALIBRATE=0, KH_BSGS_LANES or kh_set_geometry's lanes switch the calibration off.  Every base
// is walked once either way, so keys and candidates are those of an uncalibrated call.
int bsgs_scan_impl(kh_ctx *ctx, const u256 &st, const std::vector<u256> *list, uint64_t n_bases, kh_bsgs_found *found,
                   uint32_t cap, uint32_t *n_found) {
  if (!ctx->bsgs_built) return KH_E_STATE;
  const kh_bsgs_info &I = ctx->info;
  const uint64_t A_pts = I.cycles * 1024;
  const uint64_t gpb = A_pts / (2 * KH_WALK_HB);
  const uint32_t hi = ctx->lanes_bsgs, lo = ctx->lanes_bsgs / 2;
  const uint64_t tile = std::max<uint64_t>(1, hi / std::max<uint64_t>(1, gpb));  // bases per 2^21 groups
  const char *cal = getenv("KH_BSGS_CALIBRATE");
  const bool calibrate = !ctx->bsgs_calibrated && !list && A_pts == I.aux && A_pts % (2 * KH_WALK_HB) == 0 &&
                         hi == KH_BSGS_LANES && lo > ctx->lanes_max && !(cal && atoi(cal) == 0) &&
                         !getenv("KH_BSGS_LANES") && !getenv("KH_BSGS_NARROW") && !getenv("KH_NO_BIG_GROUPS") &&
                         n_bases * gpb >= 4ull * hi && ctx->targets.size() == 1 && !ctx->found[0];
  if (!calibrate) return bsgs_scan_one(ctx, st, list, n_bases, found, cap, n_found);
  // the pad at 2^21 lanes first (bsgs_scan_one would take it too): with no room, or with fewer than four
  // tiles of bases (a base of more than 2^21 groups), no calibration
  {
    size_t fr = 0, tot = 0;
    const uint64_t lane_bytes = (uint64_t)hi * (walk_pad_rows(KM_BSGSB, false, KH_WALK_HB) * 32 + 96);
    const uint64_t have = ctx->lanes_alloc() >= hi ? lane_bytes : 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr + have < lane_bytes + (32ull << 30) ||
        ensure_pipeline(ctx, hi, KH_WALK_HB) != KH_OK || n_bases < 4 * tile) {
      (void)hipGetLastError();
      ctx->err.clear();
      return bsgs_scan_one(ctx, st, list, n_bases, found, cap, n_found);
    }
  }
  const uint32_t lanes[4] = {hi, lo, lo, hi};
  double ms[2] = {0, 0}, pts[2] = {0, 0};  // [0]: hi, [1]: lo
  const uint64_t nbq = std::max<uint64_t>(tile, (n_bases / 4) / tile * tile);
  uint32_t nf_all = 0;
  uint64_t done_b = 0;
  bool exact = true;
  int r = KH_OK;
  for (int q = 0; q < 4 && done_b < n_bases; q++) {
    const int k = lanes[q] == lo;
    const uint64_t nb = q == 3 ? n_bases - done_b : std::min(nbq, n_bases - done_b);
    const u256 s = sc_add(st, sc_reduce(u256_from_u128((u128)done_b * 2 * I.n)));
    ctx->lanes_force = lanes[q];
    const timing t0 = ctx->tm[2];
    uint32_t nf = 0;
    const uint32_t off = std::min(nf_all, cap);
    r = bsgs_scan_one(ctx, s, nullptr, nb, found ? found + off : nullptr, cap - off, &nf);
    ctx->lanes_force = 0;
    if (ctx->lanes_used != lanes[q]) exact = false;
    ms[k] += ctx->tm[2].ms - t0.ms;
    pts[k] += (double)(ctx->tm[2].points - t0.points);
    nf_all += nf;
    done_b += nb;
    if ((r && r != KH_E_OVERFLOW) || ctx->found[0]) break;  // an error, or the key ended the call
  }
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipStreamSynchronize(ctx->side);
  *n_found = nf_all;
  if (r && r != KH_E_OVERFLOW) return r;
  if (exact && ms[0] > 0 && pts[0] > 0 && ms[1] > 0 && pts[1] > 0) {
    const int best = pts[1] / ms[1] > pts[0] / ms[0];
    ctx->lanes_pick = best ? lo : hi;
    ctx->cal_rate[0] = pts[best] / ms[best] * 1e3;
    ctx->cal_rate[1] = pts[!best] / ms[!best] * 1e3;
    ctx->bsgs_calibrated = true;
  } else if (!ctx->found[0]) {  // a part could not take its lane count: give up (lanes_pick stays 0);
    ctx->bsgs_calibrated = true;  // when the key ended the call, the next eligible call calibrates
  }
  return nf_all > cap ? KH_E_OVERFLOW : r;
}

}  // namespace

extern "C" int kh_bsgs_scan(kh_ctx *ctx, const uint8_t start[32], uint64_t n_bases, kh_bsgs_found *found, uint32_t cap,
                            uint32_t *n_found) {
  if (!ctx || !start || !n_found) return KH_E_ARG;
  return bsgs_scan_impl(ctx, sc_reduce(u256_from_be(start)), nullptr, n_bases, found, cap, n_found);
}

extern "C" int kh_bsgs_scan_list(kh_ctx *ctx, const uint8_t *bases, uint64_t n_bases, kh_bsgs_found *found,
                                 uint32_t cap, uint32_t *n_found) {
  if (!ctx || (!bases && n_bases) || !n_found) return KH_E_ARG;
  std::vector<u256> list(n_bases);
  parallel_for(n_bases, host_threads(ctx), [&](uint64_t lo, uint64_t hi) {
    for (uint64_t b = lo; b < hi; b++) list[b] = sc_reduce(u256_from_be(bases + 32 * b));
  });
  return bsgs_scan_impl(ctx, u256{}, &list, n_bases, found, cap, n_found);
}
