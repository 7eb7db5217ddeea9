// kh_kernels.h -- kernel argument blocks and launch helpers shared by kh_kernels.hip and the
// C-ABI implementation (kh_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kh_math.h"

// Group half-size H: a group is 2H points around one centre (the reference uses 512,
// keyhunt.cpp:299 CPU_GRP_SIZE/2).  Scratch per lane = H * 32 bytes.
#ifndef KH_WALK_H
#define KH_WALK_H 512
#endif
static_assert(KH_WALK_H >= 64 && KH_WALK_H <= 512 && (512 % KH_WALK_H) == 0,
              "2H must divide the reference's 1024-point group so lanes never straddle a BSGS base");

// Large group half-size for the continuous BSGS giant walk (KM_BSGS / KM_BSGSB): lanes there own
// long runs, so a group may span 4096 points and its one Fermat inversion is shared 4x wider.
// Scratch per lane = KH_WALK_HB * 32 bytes; the delta table holds KH_WALK_HB + 1 points.
#ifndef KH_WALK_HB
#define KH_WALK_HB 2048
#endif
// Lanes of the address family's 4096-point-group walks (xpoint, compressed address/rmd160): 2^20, so
// one 2^32-key chunk is one launch of 16384 waves -- four per wave slot of the xpoint walk (128 VGPRs,
// 4 waves/SIMD) and 5.3 per slot of the hash walk (168 VGPRs, 3 waves/SIMD).  Waves that start as
// others end run out of phase with them, so the pad and inversion phases of some overlap the field
// math of others; with 2^18 lanes (one wave per slot, all in phase) xpoint ran 50.5 vs 57.9 G points/s
// and rmd160 7.66 vs 8.00 (profiles/r04a_geom_ab.json).  Pad: 2^20 x 4096 x 32 B / 2 = 64 GB.
#ifndef KH_LANES_HB
#define KH_LANES_HB (1u << 20)
#endif
// Lanes of the BSGS giant walk's large calls: 2^21, eight waves per wave slot in turn.  The walk
// waits on its random probes (0.76 of the quad model), and the more batches of waves a launch
// holds, the further their phases drift apart: in bench.py's BSGS leg, interleaved on one box, 2^21
// lanes ran 41.9 G giant points/s (spread 0.2 %) against 38.5-40.3 at 2^20 and ~39.7 at 2^18
// (profiles/r05x_bench_lanes_2m.json).  Pad: 2^21 x 1024 rows x 32 B = 64 GB.
#ifndef KH_BSGS_LANES
#define KH_BSGS_LANES (1u << 21)
#endif

// minimum waves per SIMD requested for the walk kernel: XPOINT/BSGS/BUILD modes (KH_WALK_LB) and
// the hash160 modes (KH_WALK_LB_HASH).  256 / LB VGPRs per lane at most; see DESIGN.md.
#ifndef KH_WALK_LB
#define KH_WALK_LB 4
#endif
// KH_WALK_LB_H160CB: the compressed exact-target hash walk (the bench's rmd160 leg) at 4 waves/SIMD.  Since
// the hash IVs fold (round 5) it fits 128 VGPRs with no spill in its per-point loop: +0.3 % in an
// interleaved A/B, spreads disjoint (profiles/r05g_ab_hash_4waves.json); round 4 measured -1.1 % with the
// constants still in VGPRs.  The other hash modes (Y, uncompressed, eth) keep KH_WALK_LB_HASH.
#ifndef KH_WALK_LB_H160CB
#define KH_WALK_LB_H160CB 4
#endif
#ifndef KH_WALK_LB_HASH
#define KH_WALK_LB_HASH 3
#endif
// KH_WALK_LB_P2SH: the blocked-filter KM_P2SH walk (k_walk<KM_H160CB | KM_P2SH>) at KH_WALK_LB_HASH's 3
// waves/SIMD like every other KM_P2SH walk: at the plain compress walk's 4 it spills 55 VGPRs (224 B of
// scratch per lane, against 12 and 52 B at 3) and measured 0.2-0.4 % slower (DESIGN.md 4 "Segwit targets",
// profiles/segwit_rate_ab.json).
#ifndef KH_WALK_LB_P2SH
#define KH_WALK_LB_P2SH KH_WALK_LB_HASH
#endif

// Blocked layer-1 bloom (KH_LAYER1_BLOCKED), a split-block filter: per shard X[0], `blocks` 16-byte
// blocks, blocks = ceil(KH_BLK_BITS_MUL x reference bits / 128).  An item X (an x-coordinate, so
// already uniform) uses its own bits instead of a hash: with u = big-endian u32 of X[8..12), the
// block is (u * blocks) >> 32; its 16 bit positions come from X[12..20) (kh_blk_masks below).  An
// item is present iff every little-endian u32 word of the block covers its mask.  3x the
// reference's bits: FP 6.6e-7 (Poisson block load) vs the reference's 1e-6; one 16-byte load per
// probe, no hashing.
#define KH_BLK_BITS_MUL 3

// Bit positions of the split-block filters (blocked layer 1 above, and the exact-target filter of
// kh_kernels.hip tblk_probe), from an item's position words s0, s1 (layer 1: the big-endian u32s of
// X[12..16), X[16..20); targets: w1, w2).  Block word w (< 4) gets 4 bits, 2 in each 16-bit half: with
// s = s_{w/2}, a = s >> 8*(w%2) and b = a >> 4, the bits
//   a & 15,  16 + ((a >> 16) & 15),  b & 15,  16 + ((b >> 16) & 15)
// -- each pair is one v_pk_lshlrev_b16 of 0x00010001, so the 16 positions cost 6 shifts and 8 packed
// shifts.  Every bit of s0 and s1 is used once; per 16-bit half the FP model is the same as per 32-bit
// word.
// (1 << (a & 15)) | (1 << (16 + ((a >> 16) & 15)))
KH_HD uint32_t kh_pk_bits(uint32_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_pk_lshlrev_b16 %0, %1, %2" : "=v"(r) : "v"(a), "s"(0x00010001u));
  return r;
#else
  return (1u << (a & 15u)) | (1u << (16u + ((a >> 16) & 15u)));
#endif
}
KH_HD void kh_blk_masks(uint32_t s0, uint32_t s1, uint32_t m[4]) {
  m[0] = kh_pk_bits(s0) | kh_pk_bits(s0 >> 4);
  m[1] = kh_pk_bits(s0 >> 8) | kh_pk_bits(s0 >> 12);
  m[2] = kh_pk_bits(s1) | kh_pk_bits(s1 >> 4);
  m[3] = kh_pk_bits(s1 >> 8) | kh_pk_bits(s1 >> 12);
}

enum kh_walk_mode {
  KM_H160C = 0,   // hash160(02||X), hash160(03||X)          -l compress
  KM_H160U = 1,   // hash160(04||X||Y)                       -l uncompress
  KM_H160B = 2,   // both                                    -l both (default)
  KM_XPOINT = 3,  // X[0..20)                                -m xpoint
  KM_BSGS = 4,    // 32-byte X into the 256-shard layer-1 bloom
  KM_BUILD = 5,   // BSGS baby-step table build
  KM_DUMP = 6,    // X/Y dump (parity tests)
  KM_BSGSB = 7,   // giant steps against the blocked layer-1 bloom (one 16-B block per probe)
  KM_BUILDB = 8,  // baby-step build with the blocked layer-1 bloom
  KM_ETH = 9,     // Keccak-256(X||Y)[12..32): Ethereum address -> target bloom (-c eth)
  KM_XPOINTB = 10,  // KM_XPOINT with the blocked target filter, deferred probes (launch_walk picks it)
  KM_H160CB = 11,   // KM_H160C with the blocked target filter only (launch_walk picks it)
  // flag on KM_H160C/U/B and KM_XPOINT: also probe the endomorphism images (beta*x, y) and
  // (beta^2*x, y), i.e. keys lambda*k and lambda^2*k (-e, keyhunt.cpp:3408-3440, 3476-3830)
  KM_ENDO = 16,
  // flag on KM_H160C/B (and KM_H160CB): each plain compressed digest h is probed, then its nested
  // P2SH-P2WPKH script hash hash160(00 14 || h) against the same filter (KH_MODE_P2SH)
  KM_P2SH = 32,
};
// device hit kinds: base kind (0: 02||X, 1: 03||X, 2: 04||X||Y, 3: xpoint, 4: bsgs, 5: eth, 6: taproot) plus, with
// KM_ENDO, the image e (0: X, 1: beta*X, 2: beta^2*X) << 4 and, for 04 hashes, the Y sign << 6
#define KH_DKIND_ENDO_SHIFT 4
#define KH_DKIND_NEG 0x40u
// KM_P2SH: the filter hit was the nested digest of the 02/03 hash (the ABI's KH_KIND_P2SH)
#define KH_DKIND_P2SH 0x80u

struct kh_dev_hit {
  uint64_t idx;   // point index within the job
  uint32_t kind;  // 0: 02||X, 1: 03||X, 2: 04||X||Y, 3: xpoint, 4: bsgs candidate
  uint32_t aux;
};

struct walk_args {
  const uint32_t *tab;   // (H+1) entries of {x[8], y[8]} (LE u32 limbs)
  uint32_t *cx, *cy;     // lane centres, SoA: word w of lane g at [w*L + g]
  uint4 *scratch;        // H * L * 32 bytes
  uint32_t L;            // lanes
  uint32_t groups;       // groups per lane in this launch
  uint64_t lane_stride;  // points per lane in the job
  uint64_t group_base;   // groups each lane already walked in this job
  uint64_t n_points;     // points in the job (indices >= n_points are not probed)
  uint32_t interleave;   // 0: lane g owns groups [g*gpl, (g+1)*gpl); 1: groups g, g+L, g+2L, ...
                         // (the table's last entry is then the L*2H*D jump)
  // probe target (target bloom, or BSGS layer 1 / build layer 1)
  const uint8_t *bloom;
  kh::bloom_desc bd;
  uint32_t *hit_count;
  kh_dev_hit *hits;
  uint32_t hit_cap;
  uint32_t probe_len;  // hash160 modes: bytes of the hash the bloom keys on (20; vanity: the prefix length)
  // exact targets: the blocked target filter probed instead of the reference-layout bloom (see
  // kh_kernels.hip tblk_probe); null for vanity prefixes
  const uint4 *tblk;
  uint32_t tblocks;
  uint32_t bstride32;  // BSGS blocked layer 1: shard stride in bytes (< 2^32, kh_bsgs_setup checks)
  // BSGS build
  uint8_t *bl1, *bl2, *bl3;
  kh::bloom_desc bd2, bd3;
  uint64_t m2, m3;
  uint64_t *rows_key;
  uint32_t *rows_val;
  // dump
  uint32_t *dump_x, *dump_y;
  // k_walk_zinv: half of the --rmd-batch-size group (groups of 2 * zhalf slots)
  uint32_t zhalf;
};

struct setup_args {
  const uint32_t *scalars;  // L x 8 LE u32 limbs (unless prog)
  const uint32_t *comb;     // 32 x 256 x 16 words
  const uint32_t *q;        // optional point added to every lane: {x[8], y[8]}
  uint32_t has_q;
  uint32_t L;
  uint32_t *cx, *cy;
  // prog == 1: the lane scalars are the progression s_g = s0 + g * step (mod n), derived on the device (no
  // host loop, no upload); a lane whose scalar is 0 sets *zero_flag
  uint32_t prog;
  uint32_t s0[8], step[8];  // LE u32 limbs, both < n
  uint32_t *zero_flag;
  // prog == 2, BSGS per-base rounds: lane g starts at giant index t0 = t_round + g*lane_pts of the call
  // (base b = t0 / a_pts, a0 = t0 % a_pts) and its scalar is -(base(b) + m*(2*(a0 + h) + 1)) mod n,
  // base(b) = list[b] (list != null) or start + b*two_n
  const uint32_t *list, *start;  // 8 LE u32 limbs per base, < n
  uint64_t t_round, lane_pts, a_pts, two_n, m;
  uint32_t h;
  // with q, or null: bad[g] = 1 for a lane whose s_g*G is +-Q (the dx = 0 case below); a lane scalar of 0
  // then stands for the point at infinity and its centre is Q itself (the kangaroo herds' placement)
  uint32_t *bad;
};

// BSGS second check on the GPU (bsgs_secondcheck, keyhunt.cpp:5151-5184).  Per first-level
// candidate (giant index t = t_round + idx, base b = t / a_pts, a = t % a_pts):
// base_key = base(b) + a*2M (mod n), S = Q - base_key*G, and the 32 points S + AMP2[i] are probed
// against layer 2 (reference layout); the candidate's aux receives the mask of layer-2 hits.
// The host then runs bsgs_thirdcheck for the set bits only, in bit order.
struct refine_args {
  kh_dev_hit *cands;       // in: idx; out: aux = layer-2 mask
  const uint32_t *count;   // candidates recorded in the round (device)
  uint32_t cap;            // entries in cands
  uint32_t list_mode;      // 0: base(b) = start + b*2N; 1: base(b) = list[b]
  uint64_t t_round;        // giant index of the round's point 0
  uint64_t a_pts;          // giant points walked per base
  uint64_t two_n, two_m;
  const uint32_t *start;   // 8 LE u32 limbs, < n
  const uint32_t *list;    // list mode: bases x 8 LE u32 limbs, each < n
  const uint32_t *comb;    // 32 x 256 x 16 words
  const uint32_t *q;       // target {x[8], y[8]}
  const uint32_t *amp2;    // 32 x {x[8], y[8]}: BSGS_AMP2 (keyhunt.cpp:1818-1842)
  const uint8_t *bloom2;   // layer 2, 256 shards at bd2.stride
  kh::bloom_desc bd2;
};

// -m minikeys (thread_process_minikeys, keyhunt.cpp:3094-3259).  A minikey is 'S' plus 21 characters
// of a 58-character alphabet, held as 21 raw digits (most significant first); candidate c (1-based)
// of a chunk is base + c on that base-58 odometer, wrapping to all zeros past the top digit.
// A ROW is the 58 candidates that share their upper 20 digits: row r (relative to the base's own
// row) holds candidates c = 58 r + j - base[20], j < 58.
#define KH_MINI_STAGE 256  // k_mini_filter: valid candidates a block stages in LDS before its one queue atomic
#define KH_MINI_BATCH 8    // k_mini_keys: keys per lane that share one field inversion
struct mini_base {
  uint32_t digit[21];  // raw digits 0..57
  uint32_t alpha[58];  // the alphabet's characters
};
// k_mini_filter: one row per lane; candidates of the window (win_start, win_start + win_n] whose
// SHA-256(22 characters || '?') starts with a zero byte go to the queue as absolute offsets c
struct mini_filter_args {
  mini_base b;
  uint64_t row0;       // the window's first row
  uint32_t rows;       // lanes
  uint64_t win_start, win_n;
  uint32_t *count;     // queue head: counts every valid candidate, also those past cap
  uint64_t *queue;
  uint32_t cap;
};
// k_mini_keys: KH_MINI_BATCH queue entries per lane: key = SHA-256(22 characters), P = key*G (comb),
// one inversion per lane for its batch, hash160(04||X||Y), blocked target filter, device hit (idx = c)
struct mini_keys_args {
  mini_base b;
  const uint64_t *queue;
  uint32_t n;          // entries
  uint64_t limit;      // entries with c > limit are skipped (work past the chunk's stopping point)
  const uint32_t *comb;
  const uint4 *tblk;   // null: no probe (parity hook)
  uint32_t tblocks;
  uint32_t *hit_count;
  kh_dev_hit *hits;
  uint32_t hit_cap;
  uint32_t *out13;     // parity hook (or null): per entry the key's 8 words and the hash160's 5, as bytes in memory
};

// Taproot key-path targets (BIP-341 / BIP-86, k_tap_keys).  Per point P = (x, y) of a KM_DUMP walk: the
// tweak t = SHA-256_TapTweak(x) read big-endian (a t >= n is skipped, as BIP-341 fails there), P' = P with
// its Y made even, Q = P' + t*G (comb, Jacobian), one inversion per lane for its KH_TAP_BATCH points, then
// Q.x[0..20) against a blocked target filter; device hit kind KH_DKIND_TAPROOT, idx = idx0 + the point's index
#define KH_TAP_BATCH 8
#define KH_DKIND_TAPROOT 6u
struct tap_keys_args {
  const uint32_t *xs, *ys;  // n points in the KM_DUMP layout: 8 LE limbs per coordinate, point i at word 8*i
  uint32_t n;
  uint64_t idx0;            // the job's index of point 0
  const uint32_t *comb;
  const uint4 *tblk;        // null: no probe (parity hook)
  uint32_t tblocks;
  uint32_t *hit_count;
  kh_dev_hit *hits;
  uint32_t hit_cap;
  uint32_t *out8;           // parity hook (or null): per point Q.x as its 32 big-endian bytes in memory; a
                            // skipped point's 8 words are left as they were
};

// Pollard's lambda walk (-m kangaroo, k_kang_step).  The herd lives on the device as SoA: word w of kangaroo
// e at [w*N + e], for the affine point (x, y) and the travelled distance (a plain 256-bit integer).  Lane g
// of T owns the KH_KANG_BATCH kangaroos e = t*T + g, t < KH_KANG_BATCH, which share one inversion per step.
// One jump: j = x mod 32, P += J[j], dist += d[j]; the new point is distinguished when the top dp_bits bits
// of x are zero, and a distinguished point appends a kang_rec through the counting head dp_count.
#define KH_KANG_JUMPS 32
// Batch 32, streamed, 4 waves/SIMD: the fastest of nine forms once the herd fills the chip, 12.4 G jumps/s at
// 2^23 kangaroos against 9.9 for batch 16 and 7.0 for batch 8 (profiles/kangaroo_rate_ab.json)
#ifndef KH_KANG_BATCH
#define KH_KANG_BATCH 32
#endif
#ifndef KH_KANG_LB
#define KH_KANG_LB 4
#endif
#ifndef KH_KANG_STEPS
#define KH_KANG_STEPS 256  // jumps per kangaroo per launch
#endif
#define KH_DKANG_STALL 0x10u  // the ABI's KH_KANG_STALL
#define KH_KANG_TAB_WORDS 20  // per jump: x[8], y[8], d[4] (d < 2^128)
struct kang_rec {
  uint32_t x[8], dist[8];  // LE u32 limbs
  uint32_t index, kind;    // kind: index & 1 (0 tame, 1 wild), | KH_DKANG_STALL
};
struct kang_args {
  uint32_t *x, *y, *dist;    // 8 words each per kangaroo, SoA over N
  uint32_t *flags;           // per kangaroo: bit 0 = its point could not be formed (dist*G = +-Q'), stalled for
                             // good; bits 1..31 = the epoch of the call that last reported it stalled
  uint32_t epoch;            // this call's, 1 .. 2^31 - 2: one stall report per kangaroo and call
  uint32_t N;
  uint32_t steps;            // jumps per kangaroo in this launch
  uint32_t dp_bits;          // 0..32
  const uint32_t *jumps;     // word-major: word w (< KH_KANG_TAB_WORDS) of jump j at [w*32 + j]
  uint4 *pad;                // the prefix products: KH_KANG_BATCH rows x T lanes x 2
  unsigned long long *dp_count;  // counts every record, also those past dp_cap
  kang_rec *dps;
  uint32_t dp_cap;
};
// k_kang_place: kangaroo e = first + i (or idx[i]), i < n, takes its point from the k_setup output of its
// herd -- entry i/2 (or rank[i]) of the tame (even e) or wild (odd e) centres, SoA over n_tame / n_wild
// lanes -- and its distance
struct kang_place_args {
  uint32_t *x, *y, *dist, *flags;
  uint32_t N, first, n;
  const uint32_t *idx, *rank;         // a list of kangaroos and each one's rank among those of its kind, or null
  const uint32_t *tx, *ty, *wx, *wy;  // k_setup centres of the tames and the wilds among first .. first+n-1
  uint32_t n_tame, n_wild;
  const uint32_t *wbad;               // per wild: k_setup met dx = 0 (dist*G = +-Q')
  const uint32_t *dists;              // n x 8 LE u32 limbs
};

namespace kh {
// lanes (a multiple of 64) that walk a herd of N
inline uint32_t kang_lanes(uint32_t N, uint32_t batch = KH_KANG_BATCH) {
  return (uint32_t)(((uint64_t)N + 64ull * batch - 1) / (64ull * batch)) * 64u;
}
hipError_t launch_kang_step(const kang_args &A, hipStream_t st);
hipError_t launch_kang_place(const kang_place_args &A, hipStream_t st);
hipError_t launch_mini_filter(const mini_filter_args &A, hipStream_t st);
hipError_t launch_mini_keys(const mini_keys_args &A, hipStream_t st);
hipError_t launch_tap_keys(const tap_keys_args &A, hipStream_t st);
hipError_t launch_walk(int mode, const walk_args &A, hipStream_t st, int H = KH_WALK_H);
// The sparse-pad walks -- the BSGS giant walks and -m xpoint against the blocked target filter -- keep
// only the even prefix products in the inversion pad (kh_kernels.hip k_walk)
constexpr bool walk_sparse(int mode) { return mode == KM_BSGSB || mode == KM_BSGS || mode == KM_XPOINTB; }
// Inversion-pad rows per lane the walk launch_walk runs for (mode, blocked target filter) touches:
// rows [0, H/2) for a sparse-pad walk, all H otherwise
inline int walk_pad_rows(int mode, bool tblk, int H) {
  if (mode == KM_XPOINT && tblk) mode = KM_XPOINTB;
  return walk_sparse(mode) ? H / 2 : H;
}
hipError_t launch_walk_zinv(int mode, const walk_args &A, hipStream_t st);
hipError_t launch_refine(const refine_args &A, hipStream_t st);
hipError_t launch_setup(const setup_args &A, hipStream_t st);
hipError_t launch_test_hash160(const uint32_t *xs, const uint32_t *ys, uint32_t n, uint32_t *out, hipStream_t st);
hipError_t launch_test_field(const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out, hipStream_t st);
hipError_t launch_test_bloom(const uint8_t *items, uint32_t n, uint32_t len, const uint8_t *bloom,
                             const bloom_desc &bd, uint32_t sharded, uint32_t blocked, uint32_t *out, uint32_t *out_lazy,
                             hipStream_t st);
// probe-path parity kernels: hash160_comp2 / hash160_uncomp / eth_address per point (20 words), the
// filter key pair (a, b) of a digest's first len bytes, tblk_probe against the blocked target filter
hipError_t launch_test_digests(const uint32_t *xs, const uint32_t *ys, uint32_t n, uint32_t *out, hipStream_t st);
// per point the KM_P2SH walks' nested digests of hash160(02||X) and hash160(03||X) (10 words; ys unused)
hipError_t launch_test_digests_nested(const uint32_t *xs, const uint32_t *ys, uint32_t n, uint32_t *out,
                                      hipStream_t st);
hipError_t launch_test_filter_keys(const uint8_t *items, uint32_t n, uint32_t len, uint64_t *out, hipStream_t st);
hipError_t launch_test_tblk(const uint8_t *items, uint32_t n, const uint4 *tblk, uint32_t tblocks, uint32_t *out,
                            hipStream_t st);
}  // namespace kh
