// kh_capi_minikeys.cpp -- minikeys (thread_process_minikeys, keyhunt.cpp:3094-3259)
#include "kh_ctx.h"

namespace {

// candidates per filter launch at most: 2^28 (about 2^20 valid ones; offsets within a launch fit 32 bits)
constexpr uint64_t MK_WINDOW_MAX = 1ull << 28;

bool mk_digits_ok(const uint8_t base[21]) {
  for (int i = 0; i < 21; i++)
    if (base[i] > 57) return false;
  return true;
}

mini_base mk_base(const kh_ctx *c, const uint8_t base[21]) {
  mini_base b;
  for (int i = 0; i < 21; i++) b.digit[i] = base[i];
  for (int i = 0; i < 58; i++) b.alpha[i] = (uint8_t)c->mk_alpha[i];
  return b;
}

// the 22 characters of candidate base + off (the odometer wraps past the top digit)
void mk_text(const kh_ctx *c, const uint8_t base[21], uint64_t off, char out[24]) {
  uint64_t v = off;
  memset(out, 0, 24);
  out[0] = 'S';
  for (int i = 20; i >= 0; i--) {
    uint32_t t = base[i] + (uint32_t)(v % 58);
    v /= 58;
    if (t >= 58) {
      t -= 58;
      v++;
    }
    out[1 + i] = c->mk_alpha[t];
  }
}

int mk_queue_reserve(kh_ctx *c, uint32_t cap) {
  KHTRY(c->d_mkq.reserve(c, cap));
  return c->d_mk_count.reserve(c, 1);
}

// k_mini_filter over candidates (pos, pos + wn]: the valid ones' offsets land in d_mkq, unordered.
// A queue too small for them is grown and the window done again, as kh_scan does with its hit buffer.
int mk_filter(kh_ctx *c, const mini_base &b, uint64_t pos, uint64_t wn, uint32_t &count) {
  // one candidate in 256 is valid: wn/200 is 28 % above the mean, far outside its spread
  KHTRY(mk_queue_reserve(c, c->mk_q_user ? c->mk_q_user : (uint32_t)(wn / 200 + 1024)));
  mini_filter_args A;
  A.b = b;
  A.row0 = (b.digit[20] + pos + 1) / 58;
  A.rows = (uint32_t)((b.digit[20] + pos + wn) / 58 - A.row0 + 1);
  A.win_start = pos;
  A.win_n = wn;
  for (;;) {
    const uint32_t qcap = (uint32_t)c->d_mkq.cap();
    A.count = c->d_mk_count.get();
    A.queue = c->d_mkq.get();
    A.cap = qcap;
    HIPCHK(c, hipMemsetAsync(c->d_mk_count.get(), 0, 4, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_a.get(), c->stream));
    HIPCHK(c, launch_mini_filter(A, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_b.get(), c->stream));
    uint32_t cnt = 0;
    HIPCHK(c, hipMemcpyAsync(&cnt, c->d_mk_count.get(), 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tm[5].add(c->ev_a.get(), c->ev_b.get(), 1, wn);
    if (cnt <= qcap) {
      count = cnt;
      return KH_OK;
    }
    c->mk_redos++;
    KHTRY(mk_queue_reserve(c, (uint32_t)std::max<uint64_t>(cnt, std::min<uint64_t>(2ull * qcap, 1u << 30))));
  }
}

// k_mini_keys over the first n queue entries; with targets the device hits land in c->h_hits
int mk_keys(kh_ctx *c, const mini_base &b, uint32_t n, uint64_t limit, bool probe, uint32_t *d_out13, uint32_t &nd) {
  nd = 0;
  if (!n) return KH_OK;
  KHTRY(c->d_hits.reserve(c, kh_ctx::HIT_CAP0));  // held since kh_open, unless a grow failed
  mini_keys_args A;
  A.b = b;
  A.queue = c->d_mkq.get();
  A.n = n;
  A.limit = limit;
  A.comb = c->d_comb.get();
  A.tblk = probe ? c->d_tblk.get() : nullptr;
  A.tblocks = c->tblocks;
  A.out13 = d_out13;
  for (;;) {
    A.hit_count = c->d_hit_count.get();
    A.hits = c->d_hits.get();
    A.hit_cap = (uint32_t)c->d_hits.cap();
    HIPCHK(c, hipMemsetAsync(c->d_hit_count.get(), 0, 4, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_a.get(), c->stream));
    HIPCHK(c, launch_mini_keys(A, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_b.get(), c->stream));
    int r = fetch_hits(c, nd);
    c->tm[6].add(c->ev_a.get(), c->ev_b.get(), 1, n);
    if (r != KH_E_OVERFLOW) return r;
    uint32_t cnt = 0;
    HIPCHK(c, hipMemcpy(&cnt, c->d_hit_count.get(), 4, hipMemcpyDeviceToHost));
    KHTRY(grow_hits(c, cnt, 1u << 26, &c->d_hits));
  }
}

int mk_fetch_queue(kh_ctx *c, uint32_t n, std::vector<uint64_t> &q) {
  q.resize(n);
  return n ? download(c, q.data(), c->d_mkq, n) : KH_OK;
}
}  // namespace

extern "C" {

int kh_minikeys_set_alphabet(kh_ctx *ctx, const char alphabet[58]) {
  if (!ctx) return KH_E_ARG;
  memcpy(ctx->mk_alpha, alphabet ? alphabet : KH_MINIKEY_ALPHABET, 58);
  return KH_OK;
}

int kh_minikeys_set_window(kh_ctx *ctx, uint64_t candidates_per_launch, uint32_t queue_entries) {
  if (!ctx) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  ctx->mk_window = std::min<uint64_t>((candidates_per_launch + 3) & ~3ull, MK_WINDOW_MAX);
  ctx->mk_q_user = queue_entries;
  // the next launch allocates the queue at the size asked for (or the automatic one)
  ctx->d_mkq.reset();
  return KH_OK;
}

int kh_minikeys_queue(kh_ctx *ctx, uint32_t *entries, uint32_t *redos) {
  if (!ctx || !entries || !redos) return KH_E_ARG;
  *entries = (uint32_t)ctx->d_mkq.cap();
  *redos = ctx->mk_redos;
  return KH_OK;
}

int kh_minikeys_scan(kh_ctx *ctx, const uint8_t base[21], uint64_t need_valid, kh_minikey_hit *hits, uint32_t cap,
                     uint32_t *n_hits, uint64_t *n_candidates, uint64_t *n_valid) {
  if (!ctx || !base || !n_hits || need_valid == 0 || !mk_digits_ok(base)) return KH_E_ARG;
  if (ctx->vanity || !ctx->d_tbloom) return KH_E_STATE;
  (void)hipSetDevice(ctx->device);
  if (!ctx->d_tblk) KHTRY(upload_tblk(ctx));  // targets from a file (kh_targets_load): build their blocked filter now
  const mini_base b = mk_base(ctx, base);
  ctx->mk_redos = 0;
  std::vector<kh_minikey_hit> out;
  std::vector<uint64_t> q;
  uint64_t seen = 0, pos = 0, end = 0;
  while (!end) {
    // Window: the fixed one (kh_minikeys_set_window), or 15/16 of the candidates the missing valid keys
    // are expected to take -- so the windows shrink towards the stopping point and the work past it, the
    // rest of the last window, stays small -- between 2^16 and 2^28 candidates, a multiple of 4.
    uint64_t wn = ctx->mk_window;
    if (!wn) {
      const uint64_t est = need_valid - seen > (MK_WINDOW_MAX >> 7) ? MK_WINDOW_MAX : (need_valid - seen) * 256;
      wn = std::min<uint64_t>(MK_WINDOW_MAX, std::max<uint64_t>(1u << 16, (est - est / 16 + 3) & ~3ull));
    }
    if (pos + wn < pos) return KH_E_ARG;
    uint32_t cnt = 0, nd = 0;
    KHTRY(mk_filter(ctx, b, pos, wn, cnt));
    bool have_q = false;
    uint64_t limit = pos + wn;
    if (seen + cnt >= need_valid) {
      // the chunk ends in this window: at the group of 4 that holds the need_valid-th valid candidate
      KHTRY(mk_fetch_queue(ctx, cnt, q));
      have_q = true;
      std::vector<uint64_t> s(q);
      const size_t k = (size_t)(need_valid - seen - 1);
      std::nth_element(s.begin(), s.begin() + k, s.end());
      end = (s[k] + 3) & ~3ull;
      limit = end;
    }
    KHTRY(mk_keys(ctx, b, cnt, limit, true, nullptr, nd));
    if (nd && !have_q) KHTRY(mk_fetch_queue(ctx, cnt, q));
    // confirm the filter's hits against the sorted table (bloom_check + searchbinary, keyhunt.cpp:3221-3223)
    std::vector<kh_dev_hit> dh(ctx->h_hits.begin(), ctx->h_hits.begin() + nd);
    std::sort(dh.begin(), dh.end(), [](const kh_dev_hit &a, const kh_dev_hit &b2) { return a.idx < b2.idx; });
    for (const auto &h : dh) {
      kh_minikey_hit o;
      memset(&o, 0, sizeof o);
      mk_text(ctx, base, h.idx, o.minikey);
      sha256_bytes((const uint8_t *)o.minikey, 22, o.key);
      ge P;
      if (!ctx->comb.mult(P, u256_from_be(o.key))) continue;
      uint32_t w[5];
      hash160_uncomp(P.x, P.y, w);
      uint8_t probe[20];
      memcpy(probe, w, 20);
      if (!searchbinary(ctx->rows.data(), (int64_t)ctx->n_rows, probe, 20, 0)) continue;
      o.offset = h.idx;
      uint64_t before = 0;
      for (uint64_t v : q) before += v < h.idx;
      o.ordinal = seen + before;
      out.push_back(o);
    }
    if (end) {
      uint64_t in = 0;
      for (uint64_t v : q) in += v <= end;
      seen += in;
    } else {
      seen += cnt;
      pos += wn;
    }
  }
  if (n_candidates) *n_candidates = end;
  if (n_valid) *n_valid = seen;
  *n_hits = (uint32_t)out.size();
  if (hits)
    for (uint32_t i = 0; i < out.size() && i < cap; i++) hits[i] = out[i];
  return out.size() > cap ? KH_E_OVERFLOW : KH_OK;
}

int kh_minikeys_valid(kh_ctx *ctx, const uint8_t base[21], uint64_t n_candidates, uint64_t *offsets, uint64_t cap,
                      uint64_t *n) {
  if (!ctx || !base || !n || !mk_digits_ok(base)) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  const mini_base b = mk_base(ctx, base);
  ctx->mk_redos = 0;
  std::vector<uint64_t> all, q;
  for (uint64_t pos = 0; pos < n_candidates;) {
    const uint64_t wn = std::min<uint64_t>(ctx->mk_window ? ctx->mk_window : MK_WINDOW_MAX, n_candidates - pos);
    uint32_t cnt = 0;
    KHTRY(mk_filter(ctx, b, pos, wn, cnt));
    KHTRY(mk_fetch_queue(ctx, cnt, q));
    all.insert(all.end(), q.begin(), q.end());
    pos += wn;
  }
  std::sort(all.begin(), all.end());
  *n = all.size();
  if (offsets)
    for (uint64_t i = 0; i < all.size() && i < cap; i++) offsets[i] = all[i];
  return all.size() > cap ? KH_E_OVERFLOW : KH_OK;
}

int kh_minikeys_keys(kh_ctx *ctx, const uint8_t base[21], const uint64_t *offsets, uint32_t n, uint8_t *out52) {
  if (!ctx || !base || !offsets || !out52 || !n || !mk_digits_ok(base)) return KH_E_ARG;
  (void)hipSetDevice(ctx->device);
  const mini_base b = mk_base(ctx, base);
  KHTRY(mk_queue_reserve(ctx, n));
  dev_buf<uint32_t> dout;
  uint32_t nd = 0;
  KHTRY(dout.reserve(ctx, (size_t)n * 13));
  // an entry the kernel skips (key = 0 mod n) leaves its hash160 zero
  HIPCHK(ctx, hipMemset(dout.get(), 0, (size_t)n * 52));
  HIPCHK(ctx, hipMemcpy(ctx->d_mkq.get(), offsets, (size_t)n * 8, hipMemcpyHostToDevice));
  KHTRY(mk_keys(ctx, b, n, ~0ull, false, dout.get(), nd));
  return download(ctx, (uint32_t *)out52, dout, (size_t)n * 13);
}

}  // extern "C"
