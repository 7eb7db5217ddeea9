// kh_ctx.h -- the context behind include/kh_gpu.h and the helpers its translation units share:
// kh_capi.cpp (open/close, targets, kh_scan, target files), kh_capi_bsgs.cpp, kh_capi_minikeys.cpp,
// kh_capi_taproot.cpp, kh_capi_kangaroo.cpp and kh_capi_hooks.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdio.h>
#include <array>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "kh_gpu.h"
#include "kh_buf.h"
#include "kh_host.h"

using namespace kh;
using namespace kh_host;

struct timing {
  uint64_t launches = 0, points = 0;
  double ms = 0;
  // n launches over pts points between the (completed) events a and b
  void add(hipEvent_t a, hipEvent_t b, uint64_t n, uint64_t pts) {
    float t = 0;
    (void)hipEventElapsedTime(&t, a, b);
    launches += n;
    ms += t;
    points += pts;
  }
};

// ==============================================================================================
// kangaroo search (kh_capi_kangaroo.cpp): empty until kh_kang_setup, emptied by kh_release_walk
// ==============================================================================================
struct kang_state {
  bool ready = false;     // kh_kang_setup succeeded
  bool found = false;     // the key is known (at setup when Q = a*G, else by a resolved collision)
  bool no_walk = false;   // Q = a*G: Q' is the point at infinity, nothing is ever launched
  u256 a{}, W{}, key{};
  ge Q{}, Qp{};           // the target and Q' = Q - a*G
  bool dp_auto = false;
  uint32_t dp_bits = 0;
  u256 jd[KH_KANG_JUMPS]{};  // the jump distances
  uint32_t N = 0;         // herd size
  uint64_t seed = 0;
  std::vector<uint32_t> gen;  // per kangaroo: how often it was placed afresh
  uint32_t steps_per_launch = 0;  // 0 = automatic (kh_capi_kangaroo.cpp launch_steps)
  uint32_t epoch = 0;             // of the last kh_kang_step / solve launch group (kang_args.epoch)
  kh_kang_stats stats{};
  struct entry {
    u256 dist;
    uint32_t index, kind;
  };
  struct xhash {
    size_t operator()(const std::array<uint64_t, 4> &x) const { return (size_t)(x[0] ^ (x[1] * 0x9E3779B97F4A7C15ULL)); }
  };
  std::unordered_map<std::array<uint64_t, 4>, entry, xhash> table;  // distinguished points by x
  // the herd (SoA over N, kh_kernels.h kang_args), the jump table, the prefix products' pad, the records
  dev_buf<uint32_t> d_x, d_y, d_dist, d_unplaced, d_jumps;
  dev_buf<unsigned long long> d_count;
  dev_buf<uint4> d_pad;
  dev_buf<kang_rec> d_recs;
  std::vector<kang_rec> h_recs;
};

// ==============================================================================================
// context
// ==============================================================================================
struct kh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // BSGS rounds: the second check and the candidate copies of round r run on this high-priority
  // stream, so they start alongside round r+1's walk instead of in front of it
  hipStream_t side = nullptr;
  std::string err;
  comb_table comb;
  dev_buf<uint32_t> d_comb;

  // lanes: lanes_max for the 1024-point-group walks and the BSGS giant walk; lanes_hb for the
  // address family's 4096-point groups (several waves per SIMD slot in one launch, DESIGN.md §2
  // "Launch geometry").  kh_set_geometry(lanes != 0) sets both.
  uint32_t lanes_max = 1u << 18;
  uint32_t lanes_hb = KH_LANES_HB;
  uint32_t lanes_bsgs = KH_BSGS_LANES;  // the BSGS walk's large calls
  // lanes the BSGS walk's large calls use once the context's first large call has timed the two
  // candidates against each other (bsgs_calibrated); lanes_force: one call's forced count
  uint32_t lanes_pick = 0, lanes_force = 0;
  uint32_t lanes_used = 0;  // lanes the last large-group BSGS call walked (the calibration checks it)
  bool bsgs_calibrated = false;
  // giant points/s of the calibration's two candidates: [0] the one kept, [1] the other
  double cal_rate[2] = {0, 0};
  uint32_t groups_per_launch = 0;
  // continuous BSGS lanes kept across kh_bsgs_scan calls: valid while the lane centres sit at the
  // first group of the call that would start at cont_next (same target, lanes and group size)
  bool cont_valid = false;
  int cont_kind = 0;        // 0: BSGS giant walk (target cont_tgt), 1: kh_scan (walk mode cont_km, stride)
  u256 cont_next{};
  u256 cont_stride{};
  uint32_t cont_L = 0, cont_tgt = 0;
  int cont_H = 0, cont_km = 0;
  dev_buf<uint32_t> d_q;  // the current BSGS target {x[8], y[8]}
  // lane centres and scalars (8 words per lane) and the inversion pad (ensure_lanes allocates the four
  // together: 2 uint4 per lane and pad row)
  dev_buf<uint32_t> d_cx, d_cy, d_scalars;
  dev_buf<uint4> d_scratch;
  uint32_t lanes_alloc() const { return (uint32_t)(d_cx.cap() / 8); }
  // inversion-pad entries per lane in d_scratch
  int scratch_h() const { return d_cx.cap() ? (int)(d_scratch.cap() / 2 / lanes_alloc()) : 0; }
  void release_lanes() {
    d_cx.reset();
    d_cy.reset();
    d_scalars.reset();
    d_scratch.reset();
  }
  std::vector<uint32_t> h_scalars;

  // walk delta tables: key -> device table ((H+1) x 16 words)
  std::vector<std::pair<std::string, dev_buf<uint32_t>>> tables;

  // hits: d_hits.cap() is the capacity the kernels are given
  static constexpr uint32_t HIT_CAP0 = 1u << 16;
  dev_buf<uint32_t> d_hit_count;
  dev_buf<uint32_t> d_zero_flag;  // k_setup's progression mode: a lane scalar was 0 mod n
  dev_buf<kh_dev_hit> d_hits;
  std::vector<kh_dev_hit> h_hits;
  uint32_t scan_dev_hits = 0;  // kh_scan_device_hits: filter hits the device reported in the last kh_scan ...
  uint32_t scan_redos = 0;     // ... and how often that scan grew the hit buffer and redid its chunk

  // address targets
  std::vector<uint8_t> rows;  // sorted, 20 B each
  uint64_t n_rows = 0;
  // vanity targets (kh_set_vanity): hash160 ranges [A, B] (40 B each), bloom keyed on A's prefix
  bool vanity = false;
  std::vector<uint8_t> v_ranges;
  uint32_t probe_len = 20;
  uint32_t rmd_batch = 0;  // kh_set_rmd_batch: 0 = the ordinary walk, else the reference's group < 1024
  bloom_desc tbd{};
  uint64_t t_entries = 0;  // the target bloom's struct bloom `entries`
  std::vector<uint8_t> h_tbloom;
  dev_buf<uint8_t> d_tbloom;
  dev_buf<uint4> d_tblk;  // blocked target filter (exact targets only)
  uint32_t tblocks = 0;

  // bsgs
  uint32_t l1_layout = KH_LAYER1_BLOCKED;
  uint32_t bloom_mult = 1;   // -z (FLAGBLOOMMULTIPLIER) for the BSGS shards, kh_bsgs_set_bloom_multiplier
  bool bsgs_ready = false, bsgs_built = false;
  bool layer_replaced = false;  // kh_bsgs_set_bloom put a test's layer 1 or 2 in place: kh_bsgs_save refuses
  kh_bsgs_info info{};
  bloom_desc bd[3]{};
  bloom_desc bd_ref1{};      // layer 1 in the reference layout (what its files hold)
  uint64_t entries[3]{};     // bloom_init2 entries per layer (file headers)
  dev_buf<uint8_t> d_bl[3];
  std::vector<uint8_t> h_bl[3];  // layers 2 and 3 on the host for refinement (index 1, 2)
  std::vector<uint8_t> h_rows;   // sorted 16-byte bsgs_xvalue rows
  std::vector<ge> amp2, amp3;
  std::vector<ge> targets;
  std::vector<uint8_t> found;
  uint64_t candidates = 0;
  // parity hook (kh_bsgs_log_candidates): every first-level candidate of the scans that follow
  bool log_cands = false;
  bool base_check = false;  // kh_bsgs_set_base_check: the daemon's per-base Q == base*G test
  std::vector<uint64_t> cand_log_base;
  std::vector<uint32_t> cand_log_a, cand_log_mask;
  uint64_t second_hits = 0;          // layer-2 positives of the second check (all candidates)
  // second check on the GPU (k_refine) unless KH_REFINE=host
  bool refine_host = false;
  dev_buf<uint32_t> d_amp2;          // 32 x {x[8], y[8]}
  dev_buf<uint32_t> d_ref_start;     // 8 limbs
  dev_buf<uint32_t> d_ref_list;      // list mode bases, 8 limbs each
  pinned_buf<uint32_t> h_ref_list;   // their pinned staging copy

  // minikeys: alphabet (-8), launch window and initial queue size (0 = automatic), the device queue of
  // valid candidates' offsets and its head, how often the last call grew the queue and redid a window
  char mk_alpha[58];
  uint64_t mk_window = 0;
  uint32_t mk_q_user = 0, mk_redos = 0;
  dev_buf<uint64_t> d_mkq;
  dev_buf<uint32_t> d_mk_count;

  // taproot (kh_capi_taproot.cpp): the sorted 32-byte witness programs, the blocked filter of their first
  // 20 bytes (its own, beside d_tblk), the points per window (0 = the default), the window's X and Y in
  // the KM_DUMP layout, and the filter hits the device reported in the last kh_taproot_scan
  std::vector<uint8_t> tap_progs;
  uint64_t n_tap = 0;
  dev_buf<uint4> d_tap_blk;
  uint32_t tap_blocks = 0;
  uint64_t tap_window = 0;
  dev_buf<uint32_t> d_tap_x, d_tap_y;
  uint32_t tap_dev_hits = 0;

  kang_state kang;

  // timing
  gpu_event ev_a, ev_b;
  timing tm[9];  // kh_kernel_time kinds 0..8

  // pipelined BSGS rounds: double-buffered hit buffers, pinned host mirrors, host scalar arrays
  dev_buf<uint32_t> d_cnt2[2];
  dev_buf<kh_dev_hit> d_hits2[2];
  pinned_buf<uint32_t> h_cnt2[2];
  pinned_buf<kh_dev_hit> h_hits2[2];
  // candidates per round: cand_cap0 until the buffers exist; grown (and the round redone) on overflow
  uint32_t cand_cap0 = 1u << 16;
  uint32_t cand_cap() const { return d_hits2[0] ? (uint32_t)d_hits2[0].cap() : cand_cap0; }
  pinned_buf<uint32_t> h_scal2[2];  // 8 limbs per lane
  gpu_event ev_round[2][4];
  unsigned refine_threads = 0;  // 0 until host_threads() sets it

  ~kh_ctx();
};

#define HIPCHK(ctx, call)                                                                    \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
      return KH_E_HIP;                                                                       \
    }                                                                                        \
  } while (0)

// a step that reports KH_* codes itself
#define KHTRY(call)         \
  do {                      \
    int r_ = (call);        \
    if (r_) return r_;      \
  } while (0)

// ==============================================================================================
// shared helpers (defined in kh_capi.cpp)
// ==============================================================================================
namespace kh_host {

// lane centres for L lanes and an inversion pad of H rows per lane (walk_pad_rows: half the group for
// the sparse-pad walks)
int ensure_lanes(kh_ctx *c, uint32_t L, int H = KH_WALK_H);
// delta table T[i] = (i+1)*D, i < H, and T[H] = 2H*D, for D = d*G (d a scalar, may be "negative")
// jump > 1 (interleaved lanes): the last entry is the jump between a lane's groups, jump*2H*D
int get_table(kh_ctx *c, const u256 &d, const uint32_t **out, const int H = KH_WALK_H, uint64_t jump = 1);
// Lane centres: C_g = [Q +] s_g*G.  s: L scalars (already reduced, non-zero)
int run_setup(kh_ctx *c, const std::vector<u256> &s, const ge *q);
int run_setup_prog(kh_ctx *c, const u256 &s0, const u256 &step, uint32_t L);

struct job_geom {
  uint32_t L;
  uint64_t gpl;  // groups per lane in the job
};
// lanes cover total_groups groups; gpl must divide `gpl_divides` when non-zero
job_geom plan(kh_ctx *c, uint64_t total_groups, uint64_t gpl_divides, uint32_t lanes = 0);
// zeroed kernel arguments with the context's lanes filled in: comb, centres, L (and pad, table, stride)
setup_args setup_on_lanes(kh_ctx *c, uint32_t L);
walk_args walk_on_lanes(kh_ctx *c, const uint32_t *tab, const job_geom &jg, int H);
// walk all lanes through `gpl` groups in launches of groups_per_launch; kind = timing slot
int run_walk(kh_ctx *c, int mode, int kind, walk_args A, uint64_t gpl, uint32_t default_gpl_launch, int H = KH_WALK_H);
int fetch_hits(kh_ctx *c, uint32_t &n);
// Replaces n hit buffers (and their pinned mirrors, if h) by ones of `cap` entries, KH_E_OVERFLOW above
// `limit`.  All are freed before any is allocated; a failure leaves every one of them empty.
int grow_hits(kh_ctx *c, uint64_t cap, uint64_t limit, dev_buf<kh_dev_hit> *d, pinned_buf<kh_dev_hit> *h = nullptr,
              int n = 1);
// the blocked target filter of the context's rows (kh_kernels.hip tblk_probe)
int upload_tblk(kh_ctx *c);
// host threads for the refinement and the list packing
unsigned host_threads(kh_ctx *c);
// SHA-256 of a byte string (the reference's sha256(), hash/sha256.cpp), on kh_math.h's compression
void sha256_bytes(const uint8_t *p, size_t n, uint8_t out[32]);
constexpr size_t KH_BLOOM_STRUCT = 112;  // sizeof(struct bloom) on x86-64 (bloom/bloom.h:26-49)
void bloom_header(uint8_t h[KH_BLOOM_STRUCT], uint64_t entries, const bloom_desc &d);
// the baby-step walk (kh_capi_bsgs.cpp)
int build_walk(kh_ctx *ctx, int mode, uint8_t *bl1, const bloom_desc &bd1, uint64_t *d_key, uint32_t *d_val,
               uint64_t count = 0, bool one_layer = false);
// bsgs_secondcheck's layer-2 mask on the host, the twin of k_refine (kh_capi_bsgs.cpp)
uint32_t second_mask(const kh_ctx *c, const u256 &base_key, const ge &Q);

// n elements host -> a device buffer sized for them, and back
template <class T>
int upload(kh_ctx *c, dev_buf<T> &d, const T *src, size_t n) {
  KHTRY(d.reserve(c, n));
  HIPCHK(c, hipMemcpy(d.get(), src, n * sizeof(T), hipMemcpyHostToDevice));
  return KH_OK;
}
template <class T>
int download(kh_ctx *c, T *dst, const dev_buf<T> &d, size_t n) {
  HIPCHK(c, hipMemcpy(dst, d.get(), n * sizeof(T), hipMemcpyDeviceToHost));
  return KH_OK;
}

// f(lo, hi) over [0, n) split across up to `threads` host threads (serial below 2^16 items)
template <class F>
void parallel_for(uint64_t n, unsigned threads, F f) {
  if (n < (1u << 16) || threads <= 1) {
    f(0, n);
    return;
  }
  const uint64_t per = (n + threads - 1) / threads;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < threads; t++) {
    const uint64_t lo = t * per, hi = std::min<uint64_t>(n, lo + per);
    if (lo >= hi) break;
    th.emplace_back(f, lo, hi);
  }
  for (auto &x : th) x.join();
}

}  // namespace kh_host
