/*
 * kh_gpu.h -- C ABI of the MI355X keyhunt engine (libkh_gpu.so).
 *
 * The reference (naanprofit/keyhunt) has no plugin API: its hot path is file-static C++ driven by
 * globals.  The seams this ABI replaces are the bodies of its worker threads:
 *
 *   kh_scan            <- thread_process, one N_SEQUENTIAL_MAX chunk      keyhunt.cpp:3265-3861
 *                         (group walk 3349-3461, hash160/xpoint probes 3475-3830, bloom_check +
 *                          searchbinary 3065-3089, parity fix-up 3619-3636)
 *   kh_set_targets     <- readFileAddress/forceReadFileAddress/...XPoint  keyhunt.cpp:7239-7490
 *                         + initBloomFilter 7605-7626 + _sort 1359-1364
 *   kh_minikeys_scan   <- thread_process_minikeys, one chunk of N valid minikeys  keyhunt.cpp:3184-3255
 *   kh_taproot_scan    <- nothing: the reference has no taproot search (its TODO lists bech32 addresses)
 *   kh_kang_solve      <- nothing in the reference: its README sends public-key puzzles this wide to "another
 *                         tools like kangaroo"
 *   kh_bsgs_setup      <- BSGS parameter block                            keyhunt.cpp:1454-1842
 *   kh_bsgs_build      <- thread_bPload / thread_bPload_2blooms + bsgs_sort keyhunt.cpp:5284-5644, 2466-2503
 *   kh_bsgs_scan       <- thread_process_bsgs (sequential), bases of 2N   keyhunt.cpp:4549-4888
 *                         with bsgs_secondcheck (GPU) / bsgs_thirdcheck    keyhunt.cpp:5151-5248
 *
 * Conventions: plain C types only; 256-bit scalars and coordinates are 32-byte BIG-endian
 * (Int::Get32Bytes); every call returns 0 on success or a negative KH_E* code (never exits);
 * calls on one context are not re-entrant, contexts on different devices are independent;
 * the host owns every buffer passed in, the library owns device memory inside the context.
 * The engine never falls back to the CPU: if the HIP code object cannot run, calls fail.
 */
#ifndef KH_GPU_H
#define KH_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KH_ABI_VERSION 1

/* error codes */
#define KH_OK 0
#define KH_E_ARG -1        /* invalid argument */
#define KH_E_HIP -2        /* HIP runtime error (see kh_last_error) */
#define KH_E_NOMEM -3      /* device or host allocation failed */
#define KH_E_STATE -4      /* call out of order (e.g. scan before targets) */
#define KH_E_OVERFLOW -5   /* caller's output array too small (count is still reported) */
#define KH_E_BSGS_N -6     /* BSGS: n has no exact square root / sqrt(n) not a multiple of 1024 */
#define KH_E_RANGE -7      /* BSGS: range smaller than N ("[E] the given range is small"); kangaroo: width outside
                              [2^16, 2^192) or a range that reaches the group order */
#define KH_E_IO -8         /* table file missing, short or not writable (see kh_last_error) */
#define KH_E_FORMAT -9     /* table file of another N/k, or its sha256 checksum does not match */

/* scan modes (-m) and search kinds (-l) */
#define KH_MODE_ADDRESS 0  /* -m address / -m rmd160: hash160 probes */
#define KH_MODE_XPOINT 1   /* -m xpoint: X[0..20) probes */
#define KH_MODE_ETH 2      /* -m address|rmd160 -c eth: Keccak-256(X||Y)[12..32) probes (the search kind is
                              ignored; keyhunt.cpp:3524-3548, 3703-3760, 5663-5669).  With KH_MODE_ENDO the
                              reference's six images: eth of P, -P, beta P, -beta P, beta P (again, its
                              slip at 3533) and -beta^2 P, each hit keyed as 3736-3744 derives it */
#define KH_MODE_ENDO 0x10  /* OR into the mode: -e, also probe (beta*X, Y) and (beta^2*X, Y), i.e. keys
                              lambda*k and lambda^2*k (keyhunt.cpp:3408-3440, 3476-3830) */
#define KH_MODE_P2SH 0x20  /* OR into KH_MODE_ADDRESS: segwit targets.  Each compressed digest h = hash160(02/03||X)
                              is probed as without the flag, then its nested P2SH-P2WPKH (BIP-49) script hash
                              hash160(00 14 || h) against the same rows: a row matches whichever digest equals
                              it (a bech32 P2WPKH program is h itself).  KH_SEARCH_COMPRESS or _BOTH, with or
                              without KH_MODE_ENDO, exact targets, no kh_set_rmd_batch group below 1024:
                              anything else is KH_E_ARG.  The reference has no such mode. */
#define KH_SEARCH_COMPRESS 0
#define KH_SEARCH_UNCOMPRESS 1
#define KH_SEARCH_BOTH 2   /* reference default (FLAGSEARCH = 2) */

/* layer-1 (bloom_bP) layouts for kh_bsgs_set_layer1 */
#define KH_LAYER1_REFERENCE 0  /* the reference's bit layout (bloom/bloom.cpp): bit-identical tables */
#define KH_LAYER1_BLOCKED 1    /* default: split-block filter, an item's 16 bits in one 16-byte block chosen by
                                  the x-coordinate's own words (3x the bits per shard, FP 6.6e-7 vs 1e-6); one
                                  16-B load per probe.  Layers 2/3 stay in the reference layout, so refinement
                                  and found keys are unchanged */

/* hit kinds */
#define KH_KIND_02 0       /* hash160(02||X) matched */
#define KH_KIND_03 1       /* hash160(03||X) matched */
#define KH_KIND_04 2       /* hash160(04||X||Y) matched */
#define KH_KIND_XPOINT 3   /* X[0..20) matched */
#define KH_KIND_ETH 5      /* Ethereum address matched (key printed by writekeyeth) */
#define KH_KIND_TAPROOT 6  /* kh_taproot_scan: the taproot output key of the point matched a witness program */
/* with KH_MODE_ENDO, kind also carries the image and (for 04 hashes) the Y sign: */
#define KH_KIND_ENDO1 0x10 /* matched on (beta*X, Y): key = lambda*k (+- as reported) */
#define KH_KIND_ENDO2 0x20 /* matched on (beta^2*X, Y): key = lambda^2*k */
#define KH_KIND_NEGY 0x40  /* 04||X||-Y (or, -c eth, -Y) matched: key negated */
/* with KH_MODE_P2SH, OR'ed into KH_KIND_02 / KH_KIND_03 (and the image bits): */
#define KH_KIND_P2SH 0x80  /* hash160(00 14 || hash160(02/03||X)) matched; the key is the plain hit's.  Per
                              point and image: plain 02, plain 03, nested 02, nested 03 */
/* -e -c eth: ETH | ENDO2 without NEGY is the reference's repeated beta P image (slot 4), reported
   after its ETH | ENDO1 twin with key n - lambda^2 k, as the reference prints it */

typedef struct kh_ctx kh_ctx;

/* one confirmed hit of kh_scan: the private key as the reference would print it */
typedef struct {
  uint8_t key[32];      /* big-endian; already negated (n - k) where the reference negates */
  uint64_t offset;      /* key offset from the chunk start (before negation) */
  uint32_t kind;        /* KH_KIND_* */
  uint32_t compressed;  /* 1 -> writekey(true, ...), 0 -> writekey(false, ...) */
} kh_hit;

/* BSGS parameters exactly as the reference derives them */
typedef struct {
  uint64_t n;           /* BSGS_N (rounded down to a multiple of M) */
  uint64_t m, m2, m3;   /* bsgs_m, bsgs_m2, bsgs_m3 */
  uint64_t aux;         /* bsgs_aux = N / M */
  uint64_t cycles;      /* ceil(aux / 1024) 1024-point groups per base */
  uint64_t bloom_bits[3], bloom_bytes[3];  /* per shard, layers 1..3 */
  uint32_t bloom_hashes[3];
  uint32_t layer1_layout; /* KH_LAYER1_*; for BLOCKED, bloom_bits[0] is the bit count rounded to whole blocks */
} kh_bsgs_info;

/* one key found by kh_bsgs_scan */
typedef struct {
  uint32_t target;      /* index into the targets given to kh_bsgs_set_targets */
  uint32_t pad;
  uint8_t key[32];      /* big-endian private key */
} kh_bsgs_found;

/* ---- context ------------------------------------------------------------------------------ */
int kh_device_count(int *count);
/* free and total device memory of `device` (hipMemGetInfo): hosts that stack several contexts on
 * one device check kh_bsgs_memory against it before building their tables */
int kh_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);
int kh_open(int device, kh_ctx **out);
int kh_close(kh_ctx *ctx);
const char *kh_strerror(int code);
const char *kh_last_error(kh_ctx *ctx);
int kh_abi_version(void);
/* lanes per walk launch (0 = automatic); groups (of 1024 points) per lane per launch (0 = auto) */
int kh_set_geometry(kh_ctx *ctx, uint32_t lanes, uint32_t groups_per_launch);
/* free the walks' device buffers (lane centres, scalars, inversion pad: up to 64 GB) between jobs;
 * the next scan allocates them again and starts its lanes afresh.  Tables and targets stay. */
int kh_release_walk(kh_ctx *ctx);
/* the BSGS walk's placement calibration (DESIGN.md §2 "Placement"): a context's first large call walks
 * its four parts at 2^21, 2^20, 2^20 and 2^21 lanes on the one inversion pad (2^20 lanes walk its first
 * half) and keeps the faster.  *lanes = the lane count kept (0 = not yet decided), rates[0] = giant
 * points/s of the lane count kept, rates[1] = of the other one */
int kh_bsgs_geometry(kh_ctx *ctx, uint32_t *lanes, double rates[2]);
/* the same calibration: rates[0..1] as kh_bsgs_geometry's; rates[2..3] are always 0 (there is no
 * layer-1 stage any more).  Returns 1 when the calibration is complete (decided or given up), 0 while
 * a later call may still calibrate. */
int kh_bsgs_placement(kh_ctx *ctx, double rates[4]);
int kh_synchronize(kh_ctx *ctx);

/* ---- address / rmd160 / xpoint ------------------------------------------------------------ */
/* rows: n x 20 bytes (hash160s, or X[0..20) for xpoint), any order.  bloom_items: the element
 * count the reference sizes its bloom with (numberItems), 0 -> n.  Sorts the table, builds the
 * reference-layout bloom (bloom_init2(max(10000, items), 1e-6)) and uploads both. */
int kh_set_targets(kh_ctx *ctx, const uint8_t *rows, uint64_t n, uint64_t bloom_items);
/* -m vanity targets instead (addvanity / processOneVanity, keyhunt.cpp:6739-6866, 6970-7035):
 * ranges = n x {A[20], B[20]} hash160 bounds (inclusive), probe_len = the prefix length the bloom
 * keys on (vanity_rmd_minimun_bytes_check_length, 1..20), bloom_items = the reference's item count
 * (vanity_rmd_total).  Following kh_scan calls in the hash160 modes report every point whose
 * hash lies in a range (vanityrmdmatch, 6677-6703), with the same key resolution as -m address.
 * kh_set_targets switches back to exact targets. */
int kh_set_vanity(kh_ctx *ctx, const uint8_t *ranges, uint64_t n, uint32_t probe_len, uint64_t bloom_items);
/* Scan keys start + i*stride, i in [0, n_keys) (n_keys a multiple of 1024; stride NULL -> 1).
 * Returns the confirmed hits in the order one reference thread prints them.  A call that starts
 * where the previous kh_scan of this context ended (same mode, stride and n_keys) reuses its
 * lanes instead of starting them again: sequential chunks are cheaper, results are the same. */
int kh_scan(kh_ctx *ctx, const uint8_t start[32], const uint8_t stride[32], uint64_t n_keys, uint32_t mode,
            uint32_t search, kh_hit *hits, uint32_t cap, uint32_t *n_hits);
/* The device bytes one context's kh_scan of n_keys-key chunks holds at the default geometry, exact
 * targets (the inversion pad -- 2^20 lanes x 4096-point groups for the 2^32-key chunks of -m xpoint and
 * -l compress, half of it for xpoint's sparse pad -- lane centres, comb, hit buffer; target tables come
 * on top).  Hosts that stack contexts on one device check it against kh_device_memory first.  With
 * --rmd-batch-size (kh_set_rmd_batch) a chunk needs less. */
int kh_scan_memory(uint64_t n_keys, uint32_t mode, uint32_t search, uint64_t *needed_bytes);
/* -m rmd160 --rmd-batch-size (keyhunt.cpp:815-829, 3301-3307): group = the reference's clamped
 * rmd_batch_size (a multiple of 4 in [4, 1024]; 1024 or 0 = the ordinary walk).  Below 1024 the
 * following hash160 kh_scan calls reproduce the reference's groups of `group` keys exactly as it
 * computes them: its batch inversion then runs over a partly zero IntGroup and returns 0 for every
 * inverse, so each group holds one real point (its centre, slot group/2) and group - 1 points
 * x = -(C.x + (i+1)D.x) that are no multiples of G; a chunk of n_keys becomes ceil(n_keys/group)
 * whole groups (it overshoots its end like the reference's do-while), and hits on those points
 * carry the key of their slot with the reference's key resolution.  KH_MODE_ADDRESS and
 * KH_MODE_ETH (-m rmd160 -c eth), exact targets. */
int kh_set_rmd_batch(kh_ctx *ctx, uint32_t group);

/* ---- minikeys ----------------------------------------------------------------------------- */
/* -m minikeys (thread_process_minikeys, keyhunt.cpp:3094-3259).  A minikey is 'S' plus 21 characters of a
 * 58-character alphabet (Ccoinbuffer, -8), held as 21 raw digits 0..57, most significant first.  From a
 * base the worker walks candidates base+1, base+2, ... on that base-58 odometer (the top digit wraps to
 * all zeros), 4 at a time; a candidate is VALID when SHA-256(22 characters || '?') starts with a zero
 * byte; a valid candidate's key is SHA-256(22 characters) read big-endian, and hash160(04||X||Y) of
 * key*G is looked up in the targets of kh_set_targets / kh_targets_load. */
#define KH_MINIKEY_ALPHABET "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
typedef struct {
  uint8_t key[32];      /* SHA-256(minikey) as the reference prints it: not reduced mod n */
  uint64_t offset;      /* candidate number, 1-based from the base */
  uint64_t ordinal;     /* 0-based index among the call's valid candidates (need_valid can be 2^32) */
  char minikey[24];     /* the 22 characters, NUL-terminated */
} kh_minikey_hit;
/* -8: the 58 characters (NULL = KH_MINIKEY_ALPHABET) */
int kh_minikeys_set_alphabet(kh_ctx *ctx, const char alphabet[58]);
/* candidates per filter launch (rounded up to a multiple of 4, at most 2^28) and the device queue's
 * initial size in valid candidates; 0 = automatic (windows that shrink towards the stopping point, a
 * queue of 1/200 of the window).  A queue too small for a window's valid candidates is grown and the
 * window done again. */
int kh_minikeys_set_window(kh_ctx *ctx, uint64_t candidates_per_launch, uint32_t queue_entries);
/* One chunk of one reference thread: walk the groups of 4 candidates from base until at least need_valid
 * valid ones have been seen.  *n_candidates = the candidates walked (a multiple of 4), *n_valid = the
 * valid ones among them (need_valid .. need_valid + 3), every one of which is checked against the
 * targets.  hits: the confirmed ones in candidate order; those with ordinal >= need_valid belong to the
 * group the reference carries into its next chunk, where it processes them first.  Work past the
 * stopping point -- the rest of the last launch window -- is discarded. */
int kh_minikeys_scan(kh_ctx *ctx, const uint8_t base[21], uint64_t need_valid, kh_minikey_hit *hits, uint32_t cap,
                     uint32_t *n_hits, uint64_t *n_candidates, uint64_t *n_valid);
/* parity hooks: the valid candidates among base+1 .. base+n_candidates (ascending, 1-based), from the
 * filter kernel; per given candidate offset key[32] | hash160(04||X||Y)[20], from the key kernel (a key
 * that is 0 mod n leaves its hash160 zero); the device queue's size and how often the last scan / valid
 * call grew it and redid a window */
int kh_minikeys_valid(kh_ctx *ctx, const uint8_t base[21], uint64_t n_candidates, uint64_t *offsets, uint64_t cap,
                      uint64_t *n);
int kh_minikeys_keys(kh_ctx *ctx, const uint8_t base[21], const uint64_t *offsets, uint32_t n, uint8_t *out52);
int kh_minikeys_queue(kh_ctx *ctx, uint32_t *entries, uint32_t *redos);

/* ---- taproot ------------------------------------------------------------------------------ */
/* P2TR key-path targets (bc1p... addresses, BIP-341 / BIP-86).  The witness program of such an address is
 * no key hash: it is the x-coordinate of the tweaked key Q = lift_x(P.x) + t*G, t = SHA-256(tag || tag ||
 * P.x) read big-endian with tag = SHA-256("TapTweak"), P = k*G the internal key.  Only outputs without a
 * script tree (key-path-only, what BIP-86 wallets hand out) can be found: with a script tree the tweak
 * also covers the tree's root, which no key search knows.
 * kh_taproot_set_targets: n 32-byte witness programs, any order.  They are kept beside the rows of
 * kh_set_targets / kh_targets_load, which they do not replace: one context can hold both and serve
 * kh_scan and kh_taproot_scan in turn.  n = 0 drops them. */
int kh_taproot_set_targets(kh_ctx *ctx, const uint8_t *progs32, uint64_t n);
/* Keys start + i*stride, i in [0, n_keys) (n_keys a multiple of 1024; stride NULL -> 1), in windows of
 * kh_taproot_set_window points: the lanes are set up and walked with X and Y kept on the device, and the
 * tweak kernel (k_tap_keys) computes every point's output key and probes a blocked filter of the programs'
 * first 20 bytes; the host confirms each filter hit on all 32 bytes.  hits, in offset order: key = the
 * BIP-340 secret key of the internal key (k if P.y is even, else n - k: what a tr(KEY) descriptor takes),
 * offset = i, kind = KH_KIND_TAPROOT, compressed = 1.  More hits than cap: KH_E_OVERFLOW with *n_hits the
 * true count.  KH_E_ARG: null pointers, start or stride 0, n_keys 0 or no multiple of 1024; KH_E_STATE: no
 * programs set; KH_E_RANGE, before any launch: start + n_keys*stride reaches the group order.  The call
 * moves the context's lanes: a following kh_scan or kh_bsgs_scan starts its lanes afresh. */
int kh_taproot_scan(kh_ctx *ctx, const uint8_t start[32], const uint8_t stride[32], uint64_t n_keys, kh_hit *hits,
                    uint32_t cap, uint32_t *n_hits);
/* points per window: a multiple of 1024, at most 2^24; 0 = the default, 2^24 (1 GB of X and Y on the device) */
int kh_taproot_set_window(kh_ctx *ctx, uint64_t points);
/* parity hook: the tweak kernel on n given points {x[32], y[32]} (big-endian; at most 2^24) with no filter ->
 * per point the 32-byte output key, or 32 zero bytes where BIP-341 fails (t >= n).  The points are taken as
 * given: Y decides the sign of P', the curve equation is not checked. */
int kh_taproot_outputs(kh_ctx *ctx, const uint8_t *xy, uint32_t n, uint8_t *out32);
/* the tweak kernel's compiled batch (points per lane that share one inversion), and the filter hits the
 * device reported in the last kh_taproot_scan, before the host's confirmation */
int kh_taproot_stats(kh_ctx *ctx, uint32_t *batch, uint32_t *device_hits);

/* ---- kangaroo ----------------------------------------------------------------------------- */
/* Pollard's lambda method for one target Q whose key lies in a known interval [a, b] of width W = b - a: about
 * 2*sqrt(W) group operations and almost no memory, where BSGS time grows with W itself.  With Q' = Q - a*G
 * (key k' = k - a in [0, W]) a herd of N kangaroos jumps P += J[x(P) mod 32], dist += d[x(P) mod 32] over 32
 * fixed jumps J[j] = d_j*G.  An even index is TAME, P = dist*G; an odd one WILD, P = Q' + dist*G.  A point
 * whose x has its top dp_bits bits zero is DISTINGUISHED and goes to a host table keyed on x; a tame and a
 * wild meeting there give k' = t - w or -(t + w).  Distances are plain 256-bit integers that never wrap
 * (W < 2^192).  All 32-byte values are big-endian. */
#define KH_KANG_TAME 0
#define KH_KANG_WILD 1
#define KH_KANG_STALL 0x10  /* OR'ed into kind: the kangaroo sits on +-J[j] (or its point could not be formed) and
                               does not move; kh_kang_add_dps places it afresh */
#define KH_KANG_DP_AUTO 0xffffffffu
typedef struct { uint8_t x[32], dist[32]; uint32_t index, kind; } kh_kang_dp;
typedef struct { uint64_t jumps, dps, same_herd, reseeds, stalls, lost, bad; } kh_kang_stats;
/* Target pub_xy = {x[32], y[32]}, inclusive range [start, end].  KH_E_RANGE: end < start, W < 2^16, W >= 2^192,
 * or end reaches the group order; KH_E_ARG: Q not on the curve, or a bad jump.  Q = start*G records the key
 * `start` as found (kh_kang_solve returns it) and nothing is ever launched.  jumps_or_null: 32 distances of
 * 32 bytes, each non-zero and below 2^128; NULL: with jb = floor(bitlen(W)/2) + 1, d_j = SHA-256(
 * "kh-kangaroo-jump" || byte j || byte jb) mod 2^jb, a 0 made 1, a value equal to an earlier one incremented
 * until it is distinct.  dp_bits: 0..32, or KH_KANG_DP_AUTO: the largest dp with N*2^dp <= sqrt(W)/8 once the
 * herd's size N is known.  Drops the previous search's herd, table and statistics. */
int kh_kang_setup(kh_ctx *ctx, const uint8_t pub_xy[64], const uint8_t start[32], const uint8_t end[32],
                  uint32_t dp_bits, const uint8_t *jumps_or_null);
/* the 32 jump distances in use */
int kh_kang_jumps(kh_ctx *ctx, uint8_t out[32 * 32]);
/* kangaroos per lane that share one inversion (KH_KANG_BATCH as built), jumps per kangaroo per launch (unless
 * set: the largest power of two up to 256 that keeps a launch of the whole herd below sqrt(W)/16 jumps), the
 * herd's size (0: none yet) and the dp_bits in use (KH_KANG_DP_AUTO until a herd exists); any pointer may be
 * null */
int kh_kang_geometry(kh_ctx *ctx, uint32_t *batch, uint32_t *steps_per_launch, uint32_t *herd, uint32_t *dp_bits);
/* jumps per kangaroo per launch for the following steps (0 = automatic, see kh_kang_geometry) */
int kh_kang_set_launch(kh_ctx *ctx, uint32_t steps_per_launch);
/* A herd of `total` kangaroos (1..2^24; a first call, or another total, resizes the herd and empties the table):
 * kangaroos first .. first+n-1 are placed at dists (n x 32 bytes) through the lane-setup kernel; a distance
 * at or above the group order n is kept as given and its point formed from dist mod n.  KH_E_ARG, with the
 * herd as it was: a tame distance that is 0 mod n (0 or n itself: no point), first + n > total.  A wild with
 * dist*G = +-Q' has no point: it is marked stalled and the next step reports it. */
int kh_kang_set_herd(kh_ctx *ctx, uint32_t total, uint32_t first, uint32_t n, const uint8_t *dists);
/* The same with the library's distances for all n_kangaroos (0: the default herd, never more than sqrt(W)/128
 * rounded down to a power of two -- a sixteenth of the sqrt(W)/8 bound, so that the automatic dp_bits is 4 or
 * more -- and at least 64): with h = SHA-256(seed u64 LE || index u32 LE || generation u32
 * LE) read big-endian, a tame starts at floor(W/2) + h mod (W+1), a wild at 1 + h mod W.  The generation is 0
 * and grows by one each time kh_kang_add_dps places the kangaroo afresh.  Empties table and statistics. */
int kh_kang_seed(kh_ctx *ctx, uint64_t seed, uint32_t n_kangaroos);
/* Every kangaroo makes `steps` jumps (in launches of steps_per_launch).  dps: the distinguished points and
 * stall records (one per stalled kangaroo and call, however many launches), in any order, at most cap of them (which also bounds what the device writes); *lost = how
 * many more there were.  The herd has advanced either way. */
int kh_kang_step(kh_ctx *ctx, uint32_t steps, kh_kang_dp *dps, uint32_t cap, uint32_t *n_dps, uint64_t *lost);
/* parity hook: the points {x[32], y[32]} and distances of kangaroos first .. first+n-1 (either may be null) */
int kh_kang_get_herd(kh_ctx *ctx, uint32_t first, uint32_t n, uint8_t *xy, uint8_t *dist);
/* Feed n records to the context's table, which takes them in (index, dist) order whatever order they come
 * in (a host with several contexts feeds one table this way).  Same x, other kind: the collision is resolved (kh_kang_resolve; neither candidate: `bad`).  Same
 * x, same kind, another index: `same_herd`, and the kangaroo of the record that came later is placed afresh
 * at its next generation; so is a stalled one.  The rest of a call's records of a kangaroo placed afresh are
 * dropped.  *found = 1 and key once the key is known. */
int kh_kang_add_dps(kh_ctx *ctx, const kh_kang_dp *dps, uint32_t n, uint8_t key[32], uint32_t *found);
/* context-free, host only: k' = t - w or -(t + w) (mod n), k = start + k'; 1 and the key for the candidate with
 * k*G = Q, else 0 */
int kh_kang_resolve(const uint8_t tame_dist[32], const uint8_t wild_dist[32], const uint8_t start[32],
                    const uint8_t pub_xy[64], uint8_t key[32]);
/* step -> add_dps -> place afresh, until the key is found or at least max_jumps more jumps are done (whole
 * launches); a following call continues.  Seeds the default herd (seed 0) when there is none.  stats (or null):
 * the totals since kh_kang_setup / kh_kang_seed. */
int kh_kang_solve(kh_ctx *ctx, uint64_t max_jumps, uint8_t key[32], uint32_t *found, kh_kang_stats *stats);

/* ---- BSGS --------------------------------------------------------------------------------- */
/* layer-1 layout for the next kh_bsgs_setup (KH_LAYER1_BLOCKED unless changed) */
int kh_bsgs_set_layer1(kh_ctx *ctx, uint32_t layout);
/* -z (FLAGBLOOMMULTIPLIER, keyhunt.cpp:1111-1117) for the next kh_bsgs_setup: initBloomFilter sizes a
 * shard of more than 10000 items for mult x items entries (keyhunt.cpp:7608), so the three layers'
 * geometry -- and their -S files -- follow it as the reference's do.  Default 1. */
int kh_bsgs_set_bloom_multiplier(kh_ctx *ctx, uint32_t mult);
int kh_bsgs_setup(kh_ctx *ctx, uint64_t n, uint64_t k, kh_bsgs_info *info);
/* after kh_bsgs_setup: the device bytes this context holds once its tables are built and it scans
 * (the three layers, the bP rows, the inversion pad of the giant walk, lane state, candidate buffers
 * at their current size, a kh_bsgs_scan_list of up to 2^16 bases), and how many of them it holds
 * already.  A lower bound: longer lists (32 B per base) and candidate buffers grown on overflow come
 * on top.  The pad counted is the 2^18-lane one (8 GB); a call of >= 2^21 walk groups widens it to
 * 2^21 lanes (64 GB; 2^20: 32 GB) only while 32 GB of the device stay free after it */
int kh_bsgs_memory(kh_ctx *ctx, uint64_t *needed_bytes, uint64_t *held_bytes);
int kh_bsgs_build(kh_ctx *ctx);                  /* baby-step blooms + sorted bP table on the GPU */
/* -S table files in the reference's formats (keyhunt.cpp:2504-2652 write, 1983-2230 read), in dir
 * (NULL -> "."): keyhunt_bsgs_4_<M>.blm, keyhunt_bsgs_6_<M2>.blm, keyhunt_bsgs_7_<M3>.blm (256 x
 * {struct bloom, bits, sha256 x2}) and keyhunt_bsgs_2_<M3>.tbl (sorted 16-byte rows + sha256).
 * Files are byte-identical to the reference's except the heap pointer it stores in each struct
 * bloom.  kh_bsgs_save needs kh_bsgs_build (or _load) first; with the blocked layer 1 it builds the
 * reference-layout layer 1 for the file.  kh_bsgs_load replaces kh_bsgs_build after kh_bsgs_setup;
 * with the blocked layout it checks the layer-1 file and rebuilds the blocked layer on the GPU. */
#define KH_LOAD_SKIP_CHECKSUM 1   /* the reference's -6 */
int kh_bsgs_save(kh_ctx *ctx, const char *dir);
int kh_bsgs_load(kh_ctx *ctx, const char *dir, uint32_t flags);

/* -S for -m address|rmd160|xpoint (and -c eth): the target file cache data_<hex>.dat, named by the
 * CLI from the first 4 bytes of the target file's sha256 (keyhunt.cpp:7043-7049).  Layout:
 * sha256(bloom bits) | struct bloom (112 B) | bloom bits | sha256(rows) | u64 row bytes | sorted
 * 20-byte rows.  kh_targets_save writes the context's targets (after kh_set_targets), replacing
 * writeFileIfNeeded (keyhunt.cpp:7756-7855); kh_targets_load stands in for kh_set_targets and takes
 * the bloom geometry and bits from the file, as readFileAddress does (keyhunt.cpp:7033-7210), so a
 * file the reference wrote probes identically.  flags: KH_LOAD_SKIP_CHECKSUM. */
int kh_targets_save(kh_ctx *ctx, const char *path);
int kh_targets_load(kh_ctx *ctx, const char *path, uint32_t flags);
/* targets: n x {x[32], y[32]} affine points (big-endian) */
int kh_bsgs_set_targets(kh_ctx *ctx, const uint8_t *xy, uint32_t n);
/* Walk n_bases bases start, start + 2N, ... for every target not yet found.  Keys already found
 * are skipped (like bsgs_found[]).  found: keys found by THIS call.  With one target, a call that
 * starts at the base after the previous call's last one (same n_bases) continues its lanes. */
int kh_bsgs_scan(kh_ctx *ctx, const uint8_t start[32], uint64_t n_bases, kh_bsgs_found *found, uint32_t cap,
                 uint32_t *n_found);
/* Same for an arbitrary list of bases (n_bases x 32-byte big-endian keys), e.g. the -B backward /
 * both / random / dance schedules (keyhunt.cpp:5953, 6211, 4893, 5674): each base walks its own
 * 2N keys exactly as in kh_bsgs_scan. */
int kh_bsgs_scan_list(kh_ctx *ctx, const uint8_t *bases, uint64_t n_bases, kh_bsgs_found *found, uint32_t cap,
                      uint32_t *n_found);
int kh_bsgs_reset_found(kh_ctx *ctx);
/* first-level bloom candidates seen so far (for stats / parity tests) */
int kh_bsgs_candidates(kh_ctx *ctx, uint64_t *count);
/* first-level candidates and layer-2 hits of their second checks (bsgs_secondcheck's bloom_check
 * positives, keyhunt.cpp:5177-5180) since kh_bsgs_setup.  The second check runs on the GPU
 * (k_refine) unless the environment sets KH_REFINE=host at kh_open; both give the same counts. */
int kh_bsgs_refine_stats(kh_ctx *ctx, uint64_t *first_level, uint64_t *second_level);

/* ---- measurement -------------------------------------------------------------------------- */
/* Accumulated device time of walk launches of one kind since the last reset, measured with
 * HIP events on the context's stream.  kind: 0 address/rmd160, 1 xpoint, 2 bsgs giant,
 * 3 bsgs build, 4 lane setup (scalar mult), 5 minikeys filter (points = candidates), 6 minikeys keys
 * (points = valid candidates), 7 taproot tweak kernel (kh_taproot_scan's walks count under 0 and 4),
 * 8 kangaroo walk (points = jumps; the herds' placement counts under 4). */
int kh_kernel_time(kh_ctx *ctx, uint32_t kind, uint64_t *launches, double *ms, uint64_t *points);
int kh_kernel_time_reset(kh_ctx *ctx);

/* ---- parity hooks (used by tests/) -------------------------------------------------------- */
/* k*G for n scalars (big-endian 32 B each) -> n x {x,y} (big-endian), through the lane-setup kernel */
int kh_pubkeys(kh_ctx *ctx, const uint8_t *scalars, uint32_t n, uint8_t *xy);
/* The lane-setup kernel (k_setup) in each of its forms, on buffers of the hook's own: the centres
 * C_g = [Q +] s_g*G of L lanes (at most 2^22) -> L x {x,y} (big-endian).  q: the point Q as {x[32], y[32]}
 * or null.  The context's lanes and whatever a scan kept are untouched, and no BSGS tables are needed.
 *   prog 0: s_g = scalars[g] (L x 32 B big-endian, none 0 mod n);
 *   prog 1: s_g = s0 + g*step (mod n), derived on the device; KH_E_ARG when a lane's scalar is 0 mod n;
 *   prog 2: the BSGS centres.  Lane g starts at giant index t0 = t_round + g*lane_pts, base b = t0 / a_pts,
 *           a0 = t0 % a_pts, and s_g = -(base(b) + m*(2*(a0 + h) + 1)) mod n with base(b) = list[b]
 *           (n_bases x 32 B big-endian) or, with list null, start + b*two_n.  All values are taken raw (a
 *           base in [n, 2^256) is summed right mod n, though the engine never sends one).
 * Every index the kernel will form is checked first: KH_E_ARG when the last lane's base is not below
 * n_bases (list form), when a sum leaves 64 bits, or when a lane's centre key is 0 mod n. */
typedef struct kh_setup_form {
  uint32_t prog, L;
  const uint8_t *scalars;          /* prog 0 */
  uint8_t s0[32], step[32];        /* prog 1 */
  const uint8_t *list;             /* prog 2: list form, or null */
  uint64_t n_bases;
  uint8_t start[32];               /* prog 2: continuous form */
  uint64_t t_round, lane_pts, a_pts, two_n, m;
  uint32_t h;
} kh_setup_form;
int kh_setup_centres(kh_ctx *ctx, const kh_setup_form *form, const uint8_t *q, uint8_t *xy);
/* X (and Y if out_y) of points start + i*stride, i < n_points (multiple of 1024), via the walk */
int kh_walk_points(kh_ctx *ctx, const uint8_t start[32], const uint8_t stride[32], uint64_t n_points,
                   uint8_t *out_x, uint8_t *out_y);
/* per input point: hash160(02||X), hash160(03||X), hash160(04||X||Y) -> 60 bytes */
int kh_hash160(kh_ctx *ctx, const uint8_t *xy, uint32_t n, uint8_t *out60);
/* field ops on the device: per pair (a,b) -> mul, sqr(a), inv(a), add, sub (5 x 32 B) */
int kh_field_ops(kh_ctx *ctx, const uint8_t *a, const uint8_t *b, uint32_t n, uint8_t *out160);
/* bloom_check of n items (len 20 or 32) against the target bloom (layer 0) or BSGS layer 1..3.  Layer 0
 * also takes len 1..19: the items stay 20 bytes apart and the filter is keyed on their first len bytes,
 * as a vanity walk probes it (kh_set_vanity's probe_len). */
int kh_bloom_check(kh_ctx *ctx, uint32_t layer, const uint8_t *items, uint32_t n, uint32_t len, uint8_t *out);
/* the same with both device probe forms side by side: out = the eager probe (both hashes up front, as
 * kh_bloom_check), out_lazy = the walks' own probe, which stops at the first clear bit and computes
 * the second hash only after bit 0 (the blocked layer 1 has one form: both are its answer) */
int kh_bloom_check2(kh_ctx *ctx, uint32_t layer, const uint8_t *items, uint32_t n, uint32_t len, uint8_t *out,
                    uint8_t *out_lazy);
/* per input point, the digests as the walks compute them: hash160(02||X) and hash160(03||X) from the
 * interleaved pair form, hash160(04||X||Y), the Ethereum address -> 80 bytes.  Any (x, y) is hashed,
 * on the curve or not. */
int kh_digests(kh_ctx *ctx, const uint8_t *xy, uint32_t n, uint8_t *out80);
/* per input point, the nested digests as the KH_MODE_P2SH walks compute them (the pair form):
 * hash160(00 14 || hash160(02||X)) and hash160(00 14 || hash160(03||X)) -> 40 bytes.  Any (x, y) is hashed. */
int kh_digests_nested(kh_ctx *ctx, const uint8_t *xy, uint32_t n, uint8_t *out40);
/* per 20-byte item, the filter key pair the walks derive from its first len (1..20) bytes:
 * ab[2i] = XXH64(item[0..len), bloom seed), ab[2i+1] = XXH64(item[0..len), ab[2i]) */
int kh_filter_keys(kh_ctx *ctx, const uint8_t *items, uint32_t n, uint32_t len, uint64_t *ab);
/* the walks' probe of n 20-byte items against the blocked target filter of the exact targets
 * (kh_set_targets / kh_targets_load); KH_E_STATE without exact targets */
int kh_tblk_check(kh_ctx *ctx, const uint8_t *items, uint32_t n, uint8_t *out);
/* the last kh_scan: the filter hits the device reported (before the host's exact confirmation), and
 * how many times the scan grew its hit buffer and redid the chunk */
int kh_scan_device_hits(kh_ctx *ctx, uint32_t *device_hits, uint32_t *redos);
/* copy a bloom back: layer 0 = target bloom, 1..3 = BSGS layers (256 shards concatenated, unpadded) */
int kh_get_bloom(kh_ctx *ctx, uint32_t layer, uint8_t *buf, uint64_t cap, uint64_t *bytes);
/* kh_get_bloom's counterpart for BSGS layers 1 and 2: after kh_bsgs_build / _load, replace the layer by
 * buf -- 256 shards concatenated, unpadded, exactly kh_get_bloom's byte count (layer 1: in the layout
 * kh_bsgs_setup chose).  A test puts a denser layer there (the built bits OR'ed with random ones), so that
 * the first-level candidate list pins the giant walk at every offset (layer 1) and the second check's
 * masks pin all 32 of its points (layer 2).  The other layers, the bP rows and lanes kept for a following
 * call are untouched.  The host holds no copy of layer 1; its copy of layer 2 (the host second check's)
 * is replaced along with the device's.  kh_bsgs_save, which would write or rebuild the layer, returns
 * KH_E_STATE afterwards until the next kh_bsgs_build / _load.  KH_E_STATE before the tables exist,
 * KH_E_ARG for layer 3 (or any other) or another byte count. */
int kh_bsgs_set_bloom(kh_ctx *ctx, uint32_t layer, const uint8_t *buf, uint64_t bytes);
/* The context's own sorted bP rows (16 B each, the reference's bsgs_xvalue layout), valid until the
 * next kh_bsgs_build / _load / _set_table / kh_close: --ptable writes them to its file without a copy. */
int kh_bsgs_table_rows(kh_ctx *ctx, const uint8_t **rows, uint64_t *n_rows);

/* Memory-mapped bloom files (--mapped, keyhunt.cpp:724-806, 7630-7706; bloom/bloom.cpp:491-747): the
 * file is the raw bit array of a filter whose geometry the reference derives from the entry count or,
 * when it reloads an existing file, from the file size (bits = bytes * 8).
 * kh_bloom_add: bloom_add of n items of len bytes (20, a shorter hash160 prefix, or 32) into the flat
 * bit array bf of that geometry (host only, no GPU).
 * kh_bsgs_layer_bits: after kh_bsgs_build / _load, OR the baby-step X's of layer 1, 2 or 3 (the first
 * M, M2 or M3 babies) into 256 contiguous shards of bytes each, with the given bits and hashes. */
int kh_bloom_add(uint8_t *bf, uint64_t bits, uint32_t hashes, const uint8_t *items, uint64_t n, uint32_t len);
int kh_bsgs_layer_bits(kh_ctx *ctx, uint32_t layer, uint64_t bits, uint32_t hashes, uint64_t bytes, uint8_t *shards);

/* bsgsd semantics (bsgsd.cpp:2544-2561): the daemon's worker also tests every base point against the
 * target, so a key that is exactly a base (offset 0, which the giant/baby steps reach only through the
 * point at infinity) is found there; keyhunt's own worker (keyhunt.cpp:4625-4640) has no such test and
 * misses it.  Off by default (the CLI's behaviour); bsgsd-amd turns it on. */
int kh_bsgs_set_base_check(kh_ctx *ctx, int enable);

/* Parity hook: with logging enabled (cleared on every call), kh_bsgs_scan / _list record every
 * first-level candidate -- layer-1 bloom positive, keyhunt.cpp:4819-4823 -- as (base ordinal within
 * its call, giant index a = 1024 j + i within the base, layer-2 mask of its second check), in
 * giant-step order per round.  kh_bsgs_get_candidates copies up to cap of them. */
int kh_bsgs_log_candidates(kh_ctx *ctx, int enable);
int kh_bsgs_get_candidates(kh_ctx *ctx, uint64_t *base_index, uint32_t *a, uint32_t *mask, uint64_t cap,
                           uint64_t *n);
/* bsgs_secondcheck's layer-2 hit mask for n base keys (32-byte big-endian each) against target
 * `target`, from the GPU kernel (k_refine) and from the host code: bit i set when the point
 * Q - base_key*G + AMP2[i] passes bloom_bPx2nd (keyhunt.cpp:5151-5184) */
int kh_bsgs_second_masks(kh_ctx *ctx, uint32_t target, const uint8_t *base_keys, uint32_t n, uint32_t *gpu_mask,
                         uint32_t *host_mask);
/* The same through the kernel's own index arithmetic, in both of its forms.  Candidate j has giant index
 * t = t_round + idx[j], base b = t / a_pts, a = t % a_pts and base key base(b) + a*2M (mod n), with base(b)
 * = list[b] (n_bases x 32 B big-endian) or, with list null, start + b*two_n.  gpu_mask: k_refine's masks;
 * host_mask: the host code's for the same base keys, computed with 256-bit host arithmetic.  A base key of
 * 0 mod n has no point: both masks are 0.  two_m = 0 stands for the tables' 2M; start, the list and two_m
 * are taken raw (a base in [n, 2^256) is summed right mod n, though the engine never sends one).  KH_E_ARG
 * when a candidate's base is not below n_bases (list form) or t leaves 64 bits; nothing is launched then. */
int kh_bsgs_refine_masks(kh_ctx *ctx, uint32_t target, const uint8_t start[32], const uint8_t *list, uint64_t n_bases,
                         uint64_t t_round, uint64_t a_pts, uint64_t two_n, uint64_t two_m, const uint64_t *idx,
                         uint32_t n, uint32_t *gpu_mask, uint32_t *host_mask);
/* sorted bP table as the reference's 16-byte bsgs_xvalue rows {value[6], pad[2], index u64 LE} */
int kh_get_bsgs_table(kh_ctx *ctx, uint8_t *buf, uint64_t cap_rows, uint64_t *rows);
/* --ptable FILE --load-ptable (keyhunt.cpp:1847-1956): after kh_bsgs_build (or _load), replace the
 * sorted bP table with n_rows = M3 rows of the same 16-byte layout taken from the reference's raw
 * table file.  The rows are used as given, as the reference's read-only mapping is. */
int kh_bsgs_set_table(kh_ctx *ctx, const uint8_t *rows, uint64_t n_rows);

#ifdef __cplusplus
}
#endif
#endif /* KH_GPU_H */
