// keyhunt_cli.cpp -- command-line host of the MI355X engine (bin/keyhunt-amd).
//
// Keeps the reference's interface for the hot-path modes: -m address|rmd160|xpoint|bsgs, -f, -r,
// -b, -k, -n, -l, -q, -s, -I (stride), plus -g (GPUs to use; one host thread + kh_ctx each, like one
// pthread per -t in the reference, keyhunt.cpp:2717-2839).  Hit text, KEYFOUNDKEYFOUND.txt records
// and the stats line follow keyhunt.cpp:6891-6923 (writekey), 4825-4858 (BSGS) and 2850-2962.
// Sequential scans consume the range in whole N_SEQUENTIAL_MAX chunks (keyhunt.cpp:3314-3330) and
// BSGS in whole 2N bases (keyhunt.cpp:4600-4617), exactly as the reference's cursors do.
// BSGS base schedules -B sequential|backward|both|random|dance|angrygiant and random chunks (-R)
// follow the reference's cursors (see take_bases).  -e (address/rmd160/xpoint), -c eth (address/rmd160)
// -m vanity, and -S / -6 (the BSGS table files and the address/rmd160/xpoint data_<hex>.dat target
// cache, in the reference's formats) and -B ggsb / --bsgs-block-count / --bsgs-block-size are
// provided.  Built with -DKH_WITH_MINIKEYS (bin/minikeys-amd) the same source also takes -m minikeys
// with -C and -8 (thread_process_minikeys, keyhunt.cpp:3094-3259); bin/keyhunt-amd rejects that mode.
// -m kangaroo is the engine's own mode (the reference has none): Pollard's lambda search for the public keys
// of FILE in a bounded range, with --dp, --herd and --seed (run_kangaroo).
#include <getopt.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <random>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kh_gpu.h"
#include "../csrc/kh_math.h"
#include "../csrc/kh_host.h"
#include "kh_bsgs_files.h"
#include "kh_host_util.h"
#include "kh_mapped.h"

using namespace kh;
using namespace khh;

namespace {

const char *VERSION = "keyhunt-amd 0.1 (MI355X engine for keyhunt 0.2.230519 hot paths)";

// ---------------------------------------------------------------------------------------------
// options and shared state
// ---------------------------------------------------------------------------------------------
// MODE_MINIKEYS is a mode name of the build with KH_WITH_MINIKEYS only (bin/minikeys-amd)
enum { MODE_ADDRESS, MODE_RMD160, MODE_XPOINT, MODE_BSGS, MODE_VANITY, MODE_KANGAROO, MODE_MINIKEYS };
struct options {
  int mode = MODE_ADDRESS;
  const char *file = nullptr;
  int search = KH_SEARCH_BOTH;
  bool have_range = false, have_bits = false;
  U start, end;
  int bits = 0;
  uint64_t kfactor = 1;
  bool flag_n = false;
  uint64_t n = 0x100000000000ULL;  // -n (keyhunt.cpp:1173-1183: validated in every mode)
  int gpus = 0;
  bool quiet = false;
  int seconds = 30;
  U stride = u_from_u64(1);
  bool matrix = false;
  uint32_t layer1 = KH_LAYER1_BLOCKED;
  bool random = false;  // -R
  bool endo = false;    // -e
  bool stride_set = false;
  int bsgs_mode = 0;    // -B, index into BSGS_MODES
  bool eth = false;            // -c eth (keyhunt.cpp:874-891)
  vanity_set vanity;           // -m vanity targets (-v, -f)
  bool save_read = false;      // -S: read the table files if present, else build and write them
  bool skip_checksum = false;  // -6
  int bloom_mult = 1;          // -z (FLAGBLOOMMULTIPLIER)
  // GGSB (keyhunt.cpp:1477-1499, 1617-1627): -B ggsb or --bsgs-block-count/--bsgs-block-size
  bool ggsb = false;
  uint64_t ggsb_count = 0, ggsb_size = 0;
  // --ptable FILE / --ptable-size S / --load-ptable (keyhunt.cpp:772-787, 1847-1956)
  const char *ptable = nullptr;
  uint64_t ptable_size = 0;
  bool load_ptable = false;
  bool ptable_cache = false;  // --ptable-cache: FILE.md5 + FILE.cache (keyhunt.cpp:1958-1981, 2655-2700)
  // memory-mapped bloom files (keyhunt.cpp:493-499, 724-806); mapped::cfg holds their other options
  bool mapped = false;         // FLAGMAPPED
  bool create_mapped = false;  // FLAGCREATEMAPPED
  int rmd_batch = 1024;  // --rmd-batch-size (keyhunt.cpp:301, 815-829), -m rmd160 only
  bool crypto_given = false;      // -c (FLAGCRYPTO set): no "Setting search for btc" line
  std::string range_start_str, range_end_str;  // -r as typed (BSGS prints them so, keyhunt.cpp:1529-1531)
  // -m minikeys: -C (the base, 'S' + 21 characters) and -8 (the alphabet; NULL = the default)
  bool have_minikey = false;
  std::string minikey_str;
  const char *alphabet = nullptr;
  // --segwit (-m address; the reference has no such option): bc1q... lines are targets, a 3... line
  // turns the nested P2SH-P2WPKH probes on (KH_MODE_P2SH), hits print their segwit forms
  bool segwit = false;
  // --taproot (-m address; the reference has no such option): bc1p... lines are targets, searched by
  // kh_taproot_scan after each chunk's kh_scan.  Key-path-only outputs (BIP-86, no script tree) only.
  bool taproot = false;
  // -m kangaroo: --dp BITS (default: the library's), --herd N (0: the library's), --seed U64 (default: from the
  // OS); and which of the options the mode refuses were given
  uint32_t kang_dp = KH_KANG_DP_AUTO, kang_herd = 0;
  uint64_t kang_seed = 0;
  bool kang_seed_given = false;
  bool k_given = false, l_given = false, B_given = false, mapped_given = false, ptable_given = false;
} opt;
// --segwit: what the target reader saw -- bech32 P2WPKH rows, base58 lines of version byte 05
uint64_t g_seg_bech32 = 0, g_seg_p2sh = 0;
// --taproot: the 32-byte witness programs of the file's bc1p... lines
std::vector<uint8_t> g_tap_progs;
// keyhunt.cpp:419; ggsb and angrygiant walk like sequential (ggsb with BSGS_STEP = 2 x block size)
const char *BSGS_MODES[7] = {"sequential", "backward", "both", "random", "dance", "ggsb", "angrygiant"};
enum { BM_SEQUENTIAL, BM_BACKWARD, BM_BOTH, BM_RANDOM, BM_DANCE, BM_GGSB, BM_ANGRYGIANT };

std::mutex g_keys_mtx, g_cursor_mtx;
std::atomic<uint64_t> g_groups_done{0};  // groups walked (address family): 1024 keys each in the stats
std::atomic<uint64_t> g_bases_done{0};   // BSGS bases
std::atomic<int> g_running{0};
U g_cursor;
U g_end;

// ---------------------------------------------------------------------------------------------
// hit output
// ---------------------------------------------------------------------------------------------
// What every hit record starts from: the key as GetBase16 prints it, its public key's text and hash160.
struct hit_text {
  std::string k, pub;
  uint8_t xy[64], rmd[20];
  hit_text(kh_ctx *ctx, const uint8_t key[32], bool compressed) : k(u_hex(u_from_be32(key))) {
    kh_pubkeys(ctx, key, 1, xy);
    pub = pubkey_text(xy, compressed);
    pubkey_hash160(xy, compressed, rmd);
  }
};
// the record appended to `file`, and printed after `lead`
void emit_hit(const char *file, const char *lead, const std::string &text) {
  std::lock_guard<std::mutex> lk(g_keys_mtx);
  FILE *f = fopen(file, "a+");
  if (f) {
    fputs(text.c_str(), f);
    fclose(f);
  }
  printf("%s%s", lead, text.c_str());
  fflush(stdout);
}

// keyhunt.cpp:6891-6923.  nested (--segwit, a KH_KIND_P2SH hit): Address and rmd160 are the P2SH-P2WPKH
// ones, base58check of 05 || hash160(00 14 || hash160(pubkey)).  Under --segwit a plain compressed hit gets
// a fifth line, the key's bech32 P2WPKH address.
void writekey(kh_ctx *ctx, bool compressed, const uint8_t key[32], bool nested = false) {
  hit_text h(ctx, key, compressed);
  std::string fifth;
  if (opt.segwit && compressed && !nested) fifth = "bech32 " + bech32_p2wpkh_encode(h.rmd) + "\n";
  if (nested) {
    uint32_t hw[5], hn[5];
    memcpy(hw, h.rmd, 20);
    hash160_nested(hw, hn);
    memcpy(h.rmd, hn, 20);
  }
  emit_hit("KEYFOUNDKEYFOUND.txt", "\nHit! ",
           "Private Key: " + h.k + "\npubkey: " + h.pub + "\nAddress " + rmd_to_address(h.rmd, nested ? 5 : 0) + "\nrmd160 " +
               hex(h.rmd, 20) + "\n" + fifth);
}

// --taproot: a kh_taproot_scan hit.  The key is the BIP-340 secret key of the internal key, so its public
// key has an even Y and prints as 02 || X; the address is the bech32m form of the output key, which takes
// rmd160's line.
void write_taproot_key(kh_ctx *ctx, const uint8_t key[32]) {
  const hit_text h(ctx, key, true);
  fe x, y;
  fe_from_be(x, h.xy);
  fe_from_be(y, h.xy + 32);
  uint8_t q[32];
  if (!kh_host::taproot_output_x(x, y, q)) return;  // a confirmed hit has an output key
  emit_hit("KEYFOUNDKEYFOUND.txt", "\nHit! ",
           "Private Key: " + h.k + "\npubkey: " + h.pub + "\nAddress " + bech32m_p2tr_encode(q) + "\ntaproot output key " +
               hex(q, 32) + "\n");
}

// keyhunt.cpp:6925-6950: Ethereum hits
void writekeyeth(kh_ctx *ctx, const uint8_t key[32]) {
  const hit_text h(ctx, key, false);
  fe x, y;
  fe_from_be(x, h.xy);
  fe_from_be(y, h.xy + 32);
  uint32_t w[5];
  eth_address(x, y, w);
  uint8_t a[20];
  memcpy(a, w, 20);
  emit_hit("KEYFOUNDKEYFOUND.txt", "\n Hit!!!! ", "Private Key: " + h.k + "\naddress: 0x" + hex(a, 20) + "\n");
}

// keyhunt.cpp:6705-6737: vanity hits
void writevanitykey(kh_ctx *ctx, bool compressed, const uint8_t key[32]) {
  const hit_text h(ctx, key, compressed);
  emit_hit("VANITYKEYFOUND.txt", "\n",
           "Vanity Private Key: " + h.k + "\npubkey: " + h.pub + "\nAddress " + rmd_to_address(h.rmd) + "\nrmd160 " +
               hex(h.rmd, 20) + "\n");
}

// keyhunt.cpp:3226-3241: minikey hits (the key through GetBase16: no leading zeros)
void write_minikey(kh_ctx *ctx, const kh_minikey_hit &m) {
  const hit_text h(ctx, m.key, false);
  emit_hit("KEYFOUNDKEYFOUND.txt", "\nHIT!! ",
           "Private Key: " + h.k + "\npubkey: " + h.pub + "\nminikey: " + m.minikey + "\naddress: " + rmd_to_address(h.rmd) +
               "\n");
}

// ---------------------------------------------------------------------------------------------
// target files
// ---------------------------------------------------------------------------------------------
// readFileVanity (keyhunt.cpp:6990-7035): base58 prefixes, one per line, added to the -v ones
bool read_vanity(const char *fn) {
  FILE *f = fn ? fopen(fn, "r") : nullptr;
  if (f) {
    char line[1024];
    while (fgets(line, sizeof line, f)) {
      trim(line);
      const size_t len = strlen(line);
      if (len > 0 && len < 36) {
        if (is_base58(line))
          addvanity(line, opt.vanity);
        else
          fprintf(stderr, "[E] the string \"%s\" is not valid Base58, omiting it\n", line);
      }
    }
    fclose(f);
  }
  if (opt.vanity.targets == 0) {
    fprintf(stderr, "[E] There aren't any vanity targets\n");
    return false;
  }
  return true;
}

// initBloomFilter's lines (keyhunt.cpp:7605-7626): the item count it was given and the size of the
// filter it makes, bloom_init2(max(10000, items) (x -z above the floor), 1e-6).  The --mapped path
// prints its own (kh_mapped.h).
void print_bloom_init(uint64_t items) {
  if (opt.mapped) return;
  const uint64_t total = items <= 10000 ? 10000 : (uint64_t)opt.bloom_mult * items;
  printf("[+] Bloom filter for %llu elements.\n", (unsigned long long)items);
  printf("[+] Loading data to the bloomfilter total: %.2f MB\n", (double)mapped::bytes_for(total, 0.000001L) / 1048576.0);
}

// forceReadFileAddressEth (keyhunt.cpp:7312-7384): 40 hex digits, or 0x and 40 hex digits
bool read_targets_eth(const char *fn, std::vector<uint8_t> &rows, uint64_t &bloom_items,
                      std::vector<uint8_t> *adds = nullptr) {
  FILE *f = fopen(fn, "r");
  if (!f) {
    fprintf(stderr, "[E] Error opening the file %s\n", fn);
    return false;
  }
  char line[1024];
  std::vector<std::string> lines;
  uint64_t counted = 0;
  while (fgets(line, sizeof line, f)) {
    trim(line);
    if (strlen(line) >= 40) counted++;
    lines.push_back(line);
  }
  fclose(f);
  bloom_items = counted;
  printf("[+] Allocating memory for %llu elements: %.2f MB\n", (unsigned long long)counted,
         (double)(counted * 20) / 1048576.0);
  print_bloom_init(counted);
  for (auto &ln : lines) {
    uint8_t raw[20];
    const size_t r = ln.size();
    if (r == 40 && is_hex(ln.c_str()) && hex2bin(ln.c_str(), raw, 20)) {
      rows.insert(rows.end(), raw, raw + 20);
      if (adds) adds->insert(adds->end(), raw, raw + 20);
    } else if (r == 42 && is_hex(ln.c_str() + 2) && hex2bin(ln.c_str() + 2, raw, 20)) {
      rows.insert(rows.end(), raw, raw + 20);
      if (adds) adds->insert(adds->end(), raw, raw + 20);
    } else if (r >= 40) {
      fprintf(stderr, "[I] Ommiting invalid line %s\n", ln.c_str());
    }
  }
  return true;
}

// forceReadFileAddress (keyhunt.cpp:7239-7310) / forceReadFileXPoint (7392-7490)
// The reference's line reads: fgets(buf, cap) pieces of at most cap - 1 characters (a longer line
// is read as several pieces), trimmed of " \t\n\r" (util.c:217).
std::vector<std::string> fgets_pieces(FILE *f, size_t cap) {
  std::vector<std::string> out;
  std::vector<char> buf(cap);
  while (fgets(buf.data(), (int)cap, f)) {
    trim(buf.data());
    out.emplace_back(buf.data());
  }
  return out;
}

// -m address / rmd160 / xpoint target files, with the reference's reading quirks.
//  address, rmd160 (forceReadFileAddress, keyhunt.cpp:7239-7305): items = lines longer than 20
//    characters; then lines are consumed in order while i < items, a line that is not a 25-byte
//    base58 address or 40 hex digits printing "[I] Ommiting invalid line" and lowering items by one,
//    so valid lines after short or blank ones can go unread.  The base58 decode is b58tobin into a
//    25-byte buffer whose result length alone decides (its return value is ignored, as there).
//  xpoint (forceReadFileXPoint, keyhunt.cpp:7392-7490): items = lines of 40+ characters; the first
//    `items` lines are table rows in order, an unusable one a zero row; lines missing at the end of
//    the file lower the count.  (A blank line among them crashes the reference: strlen(NULL).)
bool read_targets(const char *fn, int mode, std::vector<uint8_t> &rows, uint64_t &bloom_items,
                  std::vector<uint8_t> *adds = nullptr) {
  g_seg_bech32 = g_seg_p2sh = 0;  // --segwit: the counts describe the file read by this call alone
  g_tap_progs.clear();
  FILE *f = fopen(fn, "r");
  if (!f) {
    fprintf(stderr, "[E] Error opening the file %s\n", fn);
    return false;
  }
  const bool xp = mode == MODE_XPOINT;
  std::vector<std::string> lines = fgets_pieces(f, xp ? 1000 : 100);
  fclose(f);
  uint64_t counted = 0;
  for (auto &ln : lines)
    if ((xp && ln.size() >= 40) || (!xp && ln.size() > 20)) counted++;
  bloom_items = counted;
  printf("[+] Allocating memory for %llu elements: %.2f MB\n", (unsigned long long)counted,
         (double)(counted * 20) / 1048576.0);
  print_bloom_init(counted);
  uint8_t raw[100] = {0};
  size_t next = 0;
  if (xp) {
    for (uint64_t i = 0; i < counted; i++) {
      if (next >= lines.size()) {  // fgets hit the end of the file: "Omiting line", N--
        fprintf(stderr, "[E] Omiting line : \n");
        continue;
      }
      const std::string &ln = lines[next++];
      std::string tok = ln.substr(0, ln.find_first_of(" \t:"));
      if (!is_hex(tok.c_str())) {
        fprintf(stderr, "[E] Ignoring invalid hexvalue %s\n", tok.c_str());  // aux after strtok
        rows.insert(rows.end(), 20, 0);  // the row stays zero (keyhunt.cpp:7433)
        continue;
      }
      // the bloom gets the first 20 bytes of what was decoded: 04||X[0..19) for an uncompressed key
      // while its table row is X[1..21) (keyhunt.cpp:7462-7467, SURVEY 8a parity note 9)
      if (tok.size() == 64 && hex2bin(tok.c_str(), raw, 32)) rows.insert(rows.end(), raw, raw + 20);
      else if (tok.size() == 66 && hex2bin(tok.c_str() + 2, raw, 32)) rows.insert(rows.end(), raw, raw + 20);
      else if (tok.size() == 130 && hex2bin(tok.c_str(), raw, 65)) rows.insert(rows.end(), raw + 2, raw + 22);
      else {
        fprintf(stderr, "[E] Omiting line unknow length size %zu: %s\n", tok.size(), tok.c_str());
        rows.insert(rows.end(), 20, 0);
        continue;
      }
      if (adds) adds->insert(adds->end(), raw, raw + 20);
    }
    return true;
  }
  uint64_t items = counted, i = 0;
  while (i < items) {
    const std::string ln = next < lines.size() ? lines[next++] : std::string();
    const size_t r = ln.size();
    bool ok = false;
    if (opt.segwit && r == 42 && bech32_p2wpkh_decode(ln.c_str(), raw)) {
      // --segwit: a mainnet P2WPKH address; its witness program is hash160(02/03||X), a plain row
      rows.insert(rows.end(), raw, raw + 20);
      if (adds) adds->insert(adds->end(), raw, raw + 20);
      g_seg_bech32++;
      ok = true;
    }
    if (opt.taproot && r == 62 && bech32m_p2tr_decode(ln.c_str(), raw)) {
      // --taproot: a mainnet P2TR address; its witness program is an output key, no row of the table
      g_tap_progs.insert(g_tap_progs.end(), raw, raw + 32);
      ok = true;
    }
    if (r > 0 && r <= 40) {
      if (r < 40 && is_base58(ln.c_str())) {
        size_t len = 25;
        b58tobin_ref(raw, &len, ln.c_str(), r);
        if (len == 25) {
          rows.insert(rows.end(), raw + 1, raw + 21);
          if (adds) adds->insert(adds->end(), raw + 1, raw + 21);
          if (opt.segwit && raw[0] == 5) g_seg_p2sh++;  // a 3... address: the run probes nested digests
          ok = true;
        }
      }
      if (r == 40 && is_hex(ln.c_str()) && hex2bin(ln.c_str(), raw, 20)) {
        rows.insert(rows.end(), raw, raw + 20);
        if (adds) adds->insert(adds->end(), raw, raw + 20);
        ok = true;
      }
    }
    if (ok) {
      i++;
    } else {
      fprintf(stderr, "[I] Ommiting invalid line %s\n", ln.c_str());
      items--;
    }
  }
  return true;
}


// ---------------------------------------------------------------------------------------------
// --mapped bloom files (keyhunt.cpp:1131-1172, 1700-1785, 7630-7706; bloom/bloom.cpp:454-747).
// A mapped filter is its raw bit array in NAME (or NAME.0 .. NAME.<c-1> with --mapped-chunks c,
// flat concatenation); the reference keeps it mapped MAP_SHARED, so the bits its loaders add reach
// the file.  Here every GPU context searches with its usual tables (the hits are decided by the
// exact table / bP-table checks, which these filters only gate), and the files are written with
// exactly the bits the reference leaves in them: a fresh file gets bloom_init_mmap's geometry; an
// existing one (without a size override) is reloaded with bloom_load_mmap's, bits = bytes * 8 and
// the hash count entries_hashes_for_bytes derives from the size, and the items are added again on
// top of its bits.  With chunks, the reference's bit -> chunk map (byte / chunk_bytes) equals the
// concatenation except for bytes past c * chunk_bytes, which it indexes out of bounds.
// ---------------------------------------------------------------------------------------------
// the mapped bloom files live in kh_mapped.h (shared with bsgsd-amd); parse_options writes their
// options straight into mapped::cfg

// ---------------------------------------------------------------------------------------------
// stats (keyhunt.cpp:2850-2962)
// ---------------------------------------------------------------------------------------------
void print_stats(uint64_t secs, const U &total) {
  static const char *pfx[7] = {"Mkeys/s", "Gkeys/s", "Tkeys/s", "Pkeys/s", "Ekeys/s", "Zkeys/s", "Ykeys/s"};
  uint64_t rem;
  U per = u_divmod_u64(total, secs ? secs : 1, &rem);
  U lim[7];
  U l = u_from_u64(1000000);
  for (int i = 0; i < 7; i++) {
    lim[i] = l;
    l = u_mul_u64(l, 1000);
  }
  // -M (FLAGMATRIX) prints the line as a line of its own; otherwise it overwrites itself in place
  const char *lead = opt.matrix ? "" : "\r", *tail = opt.matrix ? "\n" : "\r";
  if (u_cmp(per, lim[0]) < 0) {
    printf("%s[+] Total %s keys in %llu seconds: %s keys/s%s", lead, u_dec(total).c_str(), (unsigned long long)secs,
           u_dec(per).c_str(), tail);
  } else {
    int i = 0;
    while (i < 6 && u_cmp(per, lim[i + 1]) >= 0) i++;
    uint64_t div = 1;
    for (int k = 0; k < 6 + 3 * i && k < 18; k++) div *= 10;
    U d = per;
    for (int k = 0; k < i; k++) d = u_divmod_u64(d, 1000, nullptr);
    d = u_divmod_u64(d, 1000000, nullptr);
    printf("%s[+] Total %s keys in %llu seconds: ~%s %s (%s keys/s)%s", lead, u_dec(total).c_str(),
           (unsigned long long)secs, u_dec(d).c_str(), pfx[i], u_dec(per).c_str(), tail);
  }
  fflush(stdout);
}

U keys_done(const U &twoN) {
  if (opt.mode == MODE_BSGS) {
    U t = u_mul_u64(twoN, g_bases_done.load());
    return t;
  }
  U t = u_mul_u64(u_from_u64(1024), g_groups_done.load());
  if (opt.endo)  // keyhunt.cpp:2883-2891
    t = u_mul_u64(t, opt.mode == MODE_XPOINT ? 3 : 6);
  else if (opt.search == KH_SEARCH_COMPRESS)
    t = u_mul_u64(t, 2);
  return t;
}

// ---------------------------------------------------------------------------------------------
// workers
// ---------------------------------------------------------------------------------------------
struct addr_job {
  int device;
  int index = 0;  // worker number (the reference's thread_number)
  const std::vector<uint8_t> *rows;
  uint64_t bloom_items;
  uint64_t nseq;
  uint32_t mode = 0;                // the run's kh_scan mode (scan_mode)
  const char *data_file = nullptr;  // -S: data_<hex>.dat to read (or, with save_data, to write)
  bool save_data = false;
  int rc = 0;
};

// -S target cache name (readFileAddress / writeFileIfNeeded, keyhunt.cpp:7043-7049, 7765-7770):
// data_ + hex of the first 4 bytes of the target file's sha256
bool data_file_name(const char *fn, std::string &name) {
  FILE *f = fopen(fn, "rb");
  if (!f) return false;
  std::vector<uint8_t> buf;
  uint8_t chunk[1 << 16];
  size_t n;
  while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
  fclose(f);
  uint8_t ck[32];
  sha256(buf.data(), buf.size(), ck);
  char hex[9];
  snprintf(hex, sizeof hex, "%02x%02x%02x%02x", ck[0], ck[1], ck[2], ck[3]);
  name = std::string("data_") + hex + ".dat";
  return true;
}

// writeFileIfNeeded (keyhunt.cpp:7756-7855) when the target filter lives in a mapped file (-S with
// --mapped): sha256(bits) | that filter's struct bloom (kh_mapped.h struct_bloom) | its bits |
// sha256(rows) | u64 row bytes | the 20-byte rows sorted.  (Without --mapped the engine writes the
// file from its own filter, kh_targets_save.)
bool write_mapped_data_file(const std::string &path, const mapped::filter &F, const std::vector<uint8_t> &rows) {
  const size_t n = rows.size() / 20;
  std::vector<uint32_t> ix(n);
  for (size_t i = 0; i < n; i++) ix[i] = (uint32_t)i;
  std::sort(ix.begin(), ix.end(), [&](uint32_t a, uint32_t b) { return memcmp(&rows[20 * (size_t)a], &rows[20 * (size_t)b], 20) < 0; });
  std::vector<uint8_t> srt(rows.size());
  for (size_t i = 0; i < n; i++) memcpy(&srt[20 * i], &rows[20 * (size_t)ix[i]], 20);
  const uint64_t data_size = srt.size();
  uint8_t ckb[32], ckd[32], h[112];
  sha256(F.bf.data(), F.bytes, ckb);
  sha256(srt.data(), srt.size(), ckd);
  mapped::struct_bloom(F, h);
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return false;
  bool ok = fwrite(ckb, 1, 32, f) == 32 && fwrite(h, 1, 112, f) == 112 &&
            (F.bytes == 0 || fwrite(F.bf.data(), 1, F.bytes, f) == F.bytes) && fwrite(ckd, 1, 32, f) == 32 &&
            fwrite(&data_size, 1, 8, f) == 8 && (data_size == 0 || fwrite(srt.data(), 1, data_size, f) == data_size);
  ok = fclose(f) == 0 && ok;
  return ok;
}

// The kh_scan mode of the run, from -m, -c eth, -e and --segwit once the targets are read (a 3... target
// in the file makes every chunk probe the nested digests too): the memory check's, the scan's and its
// retry's
uint32_t scan_mode() {
  const uint32_t mode = opt.mode == MODE_XPOINT                                                  ? KH_MODE_XPOINT
                        : (opt.eth && (opt.mode == MODE_ADDRESS || opt.mode == MODE_RMD160)) ? KH_MODE_ETH
                                                                                               : KH_MODE_ADDRESS;
  return mode | (opt.endo ? KH_MODE_ENDO : 0) | (mode == KH_MODE_ADDRESS && opt.segwit && g_seg_p2sh ? KH_MODE_P2SH : 0);
}

// a worker's context with the job's targets set (or read from / written to the -S cache)
int open_with_targets(addr_job *j, kh_ctx **out) {
  kh_ctx *ctx = nullptr;
  int r = kh_open(j->device, &ctx);
  if (r) {
    fprintf(stderr, "[E] GPU %d: %s\n", j->device, kh_strerror(r));
    return r;
  }
  *out = ctx;
  if (opt.mode == MODE_VANITY)
    r = kh_set_vanity(ctx, opt.vanity.ranges.data(), opt.vanity.ranges.size() / 40, (uint32_t)opt.vanity.min_bytes,
                      opt.vanity.total);
  else if (j->data_file && !j->save_data)
    r = kh_targets_load(ctx, j->data_file, opt.skip_checksum ? KH_LOAD_SKIP_CHECKSUM : 0);
  else
    r = kh_set_targets(ctx, j->rows->data(), j->rows->size() / 20, j->bloom_items);
  if (!r && !g_tap_progs.empty()) r = kh_taproot_set_targets(ctx, g_tap_progs.data(), g_tap_progs.size() / 32);
  if (!r && j->save_data) {
    printf("[D] size data %llu\n", (unsigned long long)(j->rows->size()));  // keyhunt.cpp:7773
    printf("[+] Writing file %s ........\n", j->data_file);
    r = kh_targets_save(ctx, j->data_file);
  }
  return r;
}

// -m minikeys (keyhunt.cpp:1293-1323, 3094-3259, 6502-6559).  The shared cursor is the raw base, 21
// digits 0..57; a chunk takes it and advances it by 253 N candidates (increment_minikey_N: one valid
// minikey in 256 candidates, so chunks overlap by about 3 N of them).
uint8_t g_mk_raw[21];
uint8_t g_mk_n[22];  // minikeyN: the base-58 digits of 253 N, filled from index 20 down
int g_mk_limit = 0;  // minikey_n_limit: one more than their count
void minikey_n_init(uint64_t nseq) {
  memset(g_mk_n, 0, sizeof g_mk_n);  // the reference's malloc: the one digit read past those it sets is 0
  unsigned __int128 aux = (unsigned __int128)nseq * 253;
  int i = 20;
  while (aux != 0 && i > 0) {
    g_mk_n[i] = (uint8_t)(aux % 58);
    aux /= 58;
    i--;
  }
  g_mk_limit = 21 - i;
}
void increment_minikey_n(uint8_t raw[21]) {
  int i = 20, k = 0;
  while (i > 0 && k < g_mk_limit) {
    raw[i] = (uint8_t)(raw[i] + g_mk_n[i]);
    if (raw[i] > 57) {
      raw[i] = raw[i] % 58;
      raw[i - 1]++;
    }
    i--;
    k++;
  }
  // the last carry can leave a digit at 58, which indexes the reference's alphabet at its terminator;
  // here it is carried upward (and out of the top digit, as the odometer wraps)
  for (i = 20; i > 0; i--)
    if (raw[i] > 57) {
      raw[i] = (uint8_t)(raw[i] - 58);
      raw[i - 1]++;
    }
  raw[0] %= 58;
}

void mini_worker(addr_job *j) {
  kh_ctx *ctx = nullptr;
  int r = open_with_targets(j, &ctx);
  if (!ctx) {
    j->rc = r;
    g_running--;
    return;
  }
  if (!r && opt.alphabet) r = kh_minikeys_set_alphabet(ctx, opt.alphabet);
  if (r) fprintf(stderr, "[E] GPU %d: %s (%s)\n", j->device, kh_strerror(r), kh_last_error(ctx));
  const char *alpha = opt.alphabet ? opt.alphabet : B58;
  std::vector<kh_minikey_hit> hits(1 << 12), carried;
  uint64_t carry = 0;  // valid minikeys of the previous chunk's last group of 4 (count_valid, 3187-3210)
  std::random_device rd;
  while (!r) {
    uint8_t base[21];
    {
      std::lock_guard<std::mutex> lk(g_cursor_mtx);
      if (opt.random) {  // counter.Rand(256), each byte % 58 (3122-3127)
        for (int k = 0; k < 21; k++) base[k] = (uint8_t)((rd() & 0xFF) % 58);
      } else {
        memcpy(base, g_mk_raw, 21);
        increment_minikey_n(g_mk_raw);
      }
    }
    char text[24] = {0};
    text[0] = 'S';
    for (int k = 0; k < 21; k++) text[1 + k] = alpha[base[k]];
    text[22] = '?';
    if (opt.matrix) {
      printf("[+] Base minikey: %s     \n", text);
      fflush(stdout);
    } else if (!opt.quiet) {
      printf("\r[+] Base minikey: %s     \r", text);
      fflush(stdout);
    }
    // the carried group's minikeys are the first this chunk processes
    for (const auto &h : carried) write_minikey(ctx, h);
    carried.clear();
    const uint64_t need = j->nseq - carry;
    uint32_t nh = 0;
    uint64_t ncand = 0, nvalid = 0;
    r = kh_minikeys_scan(ctx, base, need, hits.data(), (uint32_t)hits.size(), &nh, &ncand, &nvalid);
    if (r == KH_E_OVERFLOW && nh > hits.size()) {
      hits.resize(nh);
      r = kh_minikeys_scan(ctx, base, need, hits.data(), (uint32_t)hits.size(), &nh, &ncand, &nvalid);
    }
    if (r) {
      fprintf(stderr, "[E] kh_minikeys_scan: %s (%s)\n", kh_strerror(r), kh_last_error(ctx));
      break;
    }
    for (uint32_t i = 0; i < nh; i++) {
      if (hits[i].ordinal < need)
        write_minikey(ctx, hits[i]);
      else
        carried.push_back(hits[i]);
    }
    carry = nvalid - need;
    g_groups_done += j->nseq / 1024;  // steps[thread]++ per 1024 valid minikeys (3253-3254)
  }
  j->rc = r;
  kh_close(ctx);
  g_running--;
}

void addr_worker(addr_job *j) {
  kh_ctx *ctx = nullptr;
  int r = open_with_targets(j, &ctx);
  if (!ctx) {
    j->rc = r;
    g_running--;
    return;
  }
  // --rmd-batch-size below 1024: the reference's groups of that size (thread_process,
  // keyhunt.cpp:3301-3307 -- FLAGMODE == MODE_RMD160 only), each counted as 1024 keys in the stats
  // (steps[] x CPU_GRP_SIZE, 2847-2880) like every group
  const uint64_t group = opt.mode == MODE_RMD160 ? (uint64_t)opt.rmd_batch : 1024;
  if (!r && group != 1024) r = kh_set_rmd_batch(ctx, (uint32_t)group);
  if (r) fprintf(stderr, "[E] GPU %d: %s (%s)\n", j->device, kh_strerror(r), kh_last_error(ctx));
  std::vector<kh_hit> hits(1 << 16);
  uint8_t st_be[32], stride_be[32];
  u_to_be32(opt.stride, stride_be);
  const U span = u_mul_u64(opt.stride, j->nseq);
  while (!r) {
    U base;
    {
      std::lock_guard<std::mutex> lk(g_cursor_mtx);
      if (opt.random) {
        base = u_rand_range(g_cursor, g_end);  // key_mpz.Rand(start, end) per chunk (keyhunt.cpp:3309-3311)
      } else {
        if (u_cmp(g_cursor, g_end) >= 0) break;
        base = g_cursor;
        g_cursor = u_add(g_cursor, span);
      }
    }
    // the chunk's progress line (thread_process, keyhunt.cpp:3333-3346): one line per chunk with -M,
    // else (without -q) overwritten in place; "thread" is this worker's index, as the reference's
    if (opt.matrix) {
      printf("Base key: %s thread %i\n", u_hex(base).c_str(), j->index);
      fflush(stdout);
    } else if (!opt.quiet) {
      printf("\rBase key: %s     \r", u_hex(base).c_str());
      fflush(stdout);
    }
    u_to_be32(base, st_be);
    uint32_t nh = 0;
    // --taproot: a file of bc1p... lines alone has no row for kh_scan to look for
    const bool plain = !opt.taproot || !j->rows->empty();
    if (plain)
      r = kh_scan(ctx, st_be, stride_be, j->nseq, j->mode, (uint32_t)opt.search, hits.data(), (uint32_t)hits.size(), &nh);
    if (r == KH_E_OVERFLOW && nh > hits.size()) {  // a short vanity prefix: take them all
      hits.resize(nh);
      r = kh_scan(ctx, st_be, stride_be, j->nseq, j->mode, (uint32_t)opt.search, hits.data(), (uint32_t)hits.size(), &nh);
    }
    // KH_E_RANGE (--rmd-batch-size, a group centred on the key 0 mod n): the hits of the groups
    // before it are reported, then the worker stops
    if (r && r != KH_E_RANGE) {
      fprintf(stderr, "[E] kh_scan: %s (%s)\n", kh_strerror(r), kh_last_error(ctx));
      break;
    }
    for (uint32_t i = 0; i < nh && i < hits.size(); i++) {
      if ((hits[i].kind & 15u) == KH_KIND_ETH)
        writekeyeth(ctx, hits[i].key);
      else if (opt.mode == MODE_VANITY)
        writevanitykey(ctx, hits[i].compressed != 0, hits[i].key);
      else
        writekey(ctx, hits[i].compressed != 0, hits[i].key, (hits[i].kind & KH_KIND_P2SH) != 0);
    }
    if (r) {
      fprintf(stderr, "[E] kh_scan: %s (%s)\n", kh_strerror(r), kh_last_error(ctx));
      break;
    }
    if (!g_tap_progs.empty()) {  // --taproot: the same chunk's keys against the bc1p... programs
      r = kh_taproot_scan(ctx, st_be, stride_be, j->nseq, hits.data(), (uint32_t)hits.size(), &nh);
      if (r == KH_E_OVERFLOW && nh > hits.size()) {
        hits.resize(nh);
        r = kh_taproot_scan(ctx, st_be, stride_be, j->nseq, hits.data(), (uint32_t)hits.size(), &nh);
      }
      if (r) {
        fprintf(stderr, "[E] kh_taproot_scan: %s (%s)\n", kh_strerror(r), kh_last_error(ctx));
        break;
      }
      for (uint32_t i = 0; i < nh; i++) write_taproot_key(ctx, hits[i].key);
    }
    g_groups_done += (j->nseq + group - 1) / group;
  }
  j->rc = r;
  kh_close(ctx);
  g_running--;
}

struct bsgs_job {
  int device;
  const std::vector<fe> *tx, *ty;
  const std::vector<bool> *comp;
  uint64_t n, k;
  uint64_t bases_per_call;       // consecutive bases of 2N (one counted progression per call)
  uint64_t list_bases_per_call;  // listed bases (-B backward|both|random|dance, ggsb): the host lists,
                                 // sorts and uploads each one, so calls stay at ~2^31 giant points
  bool first = false;  // the first GPU's worker (writes the -S files)
  int rc = 0;
};
std::vector<uint8_t> g_found;  // bsgs_found[]
std::mutex g_found_mtx;

// Base schedules of -B (one call takes up to `want` bases under the cursor lock, as the
// reference's threads take one each):
//   sequential / angrygiant  BSGS_CURRENT += 2N while < end           keyhunt.cpp:4600-4617
//   backward                 end -= 2N; base = max(end, start)          keyhunt.cpp:5995-6014
//   both                     rand()%2 picks TOP (as backward, against BSGS_CURRENT) or BOTTOM
//                            (as sequential, against the moving end)    keyhunt.cpp:6257-6300
//   random                   Rand(start, end), endless                  keyhunt.cpp:4934-4952
//   dance                    rand()%3: TOP, BOTTOM or Rand(current, end) keyhunt.cpp:5706-5750
// g_cursor plays BSGS_CURRENT (and n_range_start), g_top n_range_end.
U g_top;
U g_step;  // BSGS_STEP
// step = BSGS_STEP: 2N, or 2 x the GGSB block size when the babies are split into several blocks
bool take_bases(const U &twoN, uint64_t want, std::vector<U> &out) {
  out.clear();
  std::lock_guard<std::mutex> lk(g_cursor_mtx);
  auto top = [&]() {
    if (u_cmp(g_top, g_cursor) <= 0) return false;
    g_top = u_sub(g_top, twoN);
    out.push_back(u_cmp(g_top, g_cursor) < 0 ? g_cursor : g_top);
    return true;
  };
  auto bottom = [&]() {
    if (u_cmp(g_cursor, g_top) >= 0) return false;
    out.push_back(g_cursor);
    g_cursor = u_add(g_cursor, twoN);
    return true;
  };
  int mode = opt.bsgs_mode;
  if (mode == BM_SEQUENTIAL || mode == BM_ANGRYGIANT || mode == BM_BACKWARD || mode == BM_GGSB) {
    while (out.size() < want && (mode == BM_BACKWARD ? top() : bottom())) {
    }
    return !out.empty();
  }
  if (mode == BM_RANDOM) {
    while (out.size() < want) out.push_back(u_rand_range(g_cursor, g_top));
    return true;
  }
  // both / dance: one draw per batch (the reference draws per base; the set of bases is the same)
  int pick = rand() % (mode == BM_DANCE ? 3 : 2);
  if (pick == 2) {
    while (out.size() < want) out.push_back(u_rand_range(g_cursor, g_top));
    return true;
  }
  while (out.size() < want && (pick == 0 ? top() : bottom())) {
  }
  if (out.empty()) {  // this side is exhausted; the other may not be
    while (out.size() < want && (pick == 0 ? bottom() : top())) {
    }
  }
  return !out.empty();
}

// One engine call's bases of a listed schedule: `drawn` in the reference's order (the progress
// lines); a run 2N apart, ascending or descending (backward, both), goes through kh_bsgs_scan from its
// lowest base, any other set through kh_bsgs_scan_list in drawn order (the engine needs no order)
struct list_batch {
  bool ok = false;
  std::vector<U> drawn;
  bool consecutive = false;
  uint8_t st_be[32];
  std::vector<uint8_t> be;
};

void prepare_batch(const U &twoN, uint64_t want, list_batch &B) {
  B.ok = take_bases(twoN, want, B.drawn);
  B.be.clear();
  if (!B.ok) return;
  const size_t n = B.drawn.size();
  bool up = true, down = true;
  for (size_t i = 1; i < n && (up || down); i++) {
    if (up) up = u_cmp(B.drawn[i], B.drawn[i - 1]) > 0 && u_cmp(u_sub(B.drawn[i], B.drawn[i - 1]), twoN) == 0;
    if (down) down = u_cmp(B.drawn[i - 1], B.drawn[i]) > 0 && u_cmp(u_sub(B.drawn[i - 1], B.drawn[i]), twoN) == 0;
  }
  B.consecutive = up || down;
  if (B.consecutive) {
    u_to_be32(up ? B.drawn[0] : B.drawn[n - 1], B.st_be);
    return;
  }
  B.be.resize(32 * n);
  for (size_t i = 0; i < n; i++) u_to_be32(B.drawn[i], &B.be[32 * i]);
}

// The sequential schedules (sequential, angrygiant, ggsb) as one progression: up to `want` bases
// from the cursor, step apart, while below the end -- the bases take_bases would list, counted
// instead of listed (a call of 2^20 bases spent ~9 % of the GPU's time listing, sorting and
// checking them on the host between calls)
bool take_progression(const U &step, uint64_t want, U &start, uint64_t &count) {
  std::lock_guard<std::mutex> lk(g_cursor_mtx);
  if (u_cmp(g_cursor, g_top) >= 0) return false;
  start = g_cursor;
  const U rem = u_sub(g_top, g_cursor);
  uint64_t n = want;
  if (step.v[1] == 0 && step.v[2] == 0 && step.v[3] == 0 && step.v[4] == 0 && step.v[0]) {
    uint64_t r = 0;
    const U q = u_divmod_u64(rem, step.v[0], &r);  // bases below the end: ceil(rem / step)
    if (u_bitlen(q) < 63) n = std::min<uint64_t>(want, q.v[0] + (r ? 1 : 0));
    count = n;
    g_cursor = u_add(g_cursor, u_mul_u64(step, n));
    return true;
  }
  for (count = 0; count < want && u_cmp(g_cursor, g_top) < 0; count++) g_cursor = u_add(g_cursor, step);
  return true;
}

// --ptable-cache: FILE.md5 holds the file's MD5 as hex text; FILE.cache the 257 bucket starts of
// the rows by value[0] under that MD5 (struct bptable_cache_file, keyhunt.cpp:137-143, 186-241).
// Two phases, where the reference has them: with --load-ptable, before the tables are built, an
// existing FILE.md5 is trusted, else the MD5 is computed from the file and written (1956-1981);
// after the tables (and the -S files), the MD5 is computed if it is not known yet, and the cache
// file is checked and rebuilt when it is of another MD5 or size (2655-2700).  Only the files are
// produced: the engine's third check does not need the buckets.
uint8_t g_md5[16];
bool g_md5_ready = false;

void ptable_md5_loaded() {
  if (!opt.ptable_cache || !opt.load_ptable || !opt.ptable) return;
  const std::string md5_path = std::string(opt.ptable) + ".md5";
  if (read_md5_file(md5_path.c_str(), g_md5)) {
    g_md5_ready = true;
    printf("[+] bP table MD5 loaded (%s)\n", md5_path.c_str());
  } else {
    g_md5_ready = md5_refresh(opt.ptable, g_md5, true);
  }
}

void ptable_cache(const uint8_t *rows, uint64_t m3) {
  if (!opt.ptable_cache) return;
  if (!g_md5_ready) g_md5_ready = md5_refresh(opt.ptable, g_md5, false);
  if (g_md5_ready) bptable_cache_refresh(opt.ptable, g_md5, rows, m3);
}

// --ptable FILE (keyhunt.cpp:1847-1956): the reference maps FILE (grown to max(M3 x 16 B,
// --ptable-size), never shrunk) as its bP table, so the baby-step workers (or -S's .tbl read) leave
// the sorted rows in it.  The rows are built on the GPU here, and the first worker writes them.
// With --load-ptable the existing FILE is mapped read-only and its first M3 rows are the table.
int bsgs_ptable(kh_ctx *ctx, const kh_bsgs_info &info, bool first) {
  if (!opt.ptable) return KH_OK;
  const uint64_t bytes = info.m3 * 16;
  auto fail = [](const char *what) {
    fprintf(stderr, "[E] %s\n", what);
    return KH_E_IO;
  };
  if (opt.load_ptable) {
    // the first M3 rows go straight from the mapping into the context's table
    ptable_rows map;
    switch (ptable_load_rows(opt.ptable, bytes, map)) {
      case PT_OK: break;
      case PT_OPEN: return fail("Cannot open bP table file");
      case PT_STAT: return fail("Cannot stat bP table file");
      case PT_SMALL: return fail("Existing bP table file too small");
      default: return fail("mmap failed for bP table");
    }
    int r = kh_bsgs_set_table(ctx, map.data, info.m3);
    if (!r && first) ptable_cache(map.data, info.m3);
    if (r) fprintf(stderr, "[E] %s\n", kh_last_error(ctx));
    return r;
  }
  if (!first) return KH_OK;
  // the context's own sorted rows, written without another host copy
  const uint8_t *rows = nullptr;
  uint64_t nrows = 0;
  int r = kh_bsgs_table_rows(ctx, &rows, &nrows);
  if (r) return r;
  const ptable_err e = ptable_prepare(opt.ptable, bytes, opt.ptable_size);
  if (e == PT_OPEN) return fail("Cannot create bP table file");
  if (e == PT_RESIZE) return fail("Cannot resize bP table file");
  if (e || !ptable_write_rows(opt.ptable, rows, bytes)) return fail("Cannot write bP table file");
  ptable_cache(rows, info.m3);
  return KH_OK;
}

// The reference's table-setup lines, which the first context's worker prints in the reference's order
// (keyhunt.cpp:1631-1845, 2225-2503); every number follows from M, M2, M3 and the shard geometry.
// The other workers wait for them (setup_done / setup_wait) before they print a base line.
//
// The three layers as initBloomFilter reports them (1687-1781 with 7605-7626): per layer the element
// count, then per shard its item count and bloom_init2 size, then the layer's total.  The --mapped
// path prints the same lines as it opens the shard files (kh_mapped.h bsgs_layers).
void print_layer_lines(const kh_bsgs_info &I) {
  const uint64_t ms[3] = {I.m, I.m2, I.m3}, floor_[3] = {10000, 1000, 1000};
  for (int l = 0; l < 3; l++) {
    const uint64_t items = ms[l] / 256 > floor_[l] ? ms[l] / 256 + (ms[l] % 256 ? 1 : 0) : 1000;
    const uint64_t bytes = mapped::init2_bytes(items <= 10000 ? 10000 : (uint64_t)opt.bloom_mult * items);
    printf("[+] Bloom filter for %llu elements ", (unsigned long long)ms[l]);
    for (int i = 0; i < 256; i++) {
      printf("[+] Bloom filter for %llu elements.\n", (unsigned long long)items);
      printf("[+] Loading data to the bloomfilter total: %.2f MB\n", (double)bytes / 1048576.0);
    }
    printf(": %.2f MB\n", mapped::layer_mb(256 * bytes));
  }
}

// 1845: the bP table's size, in whole MB (the integer division is the reference's)
void print_allocating(const kh_bsgs_info &I) {
  printf("[+] Allocating %.2f MB for %llu bP Points\n", (double)(I.m3 * 16 / 1048576), (unsigned long long)I.m3);
}

// The baby-step build (2362-2503): its progress lines as one reference thread (-t 1) prints them -- the
// count before the work units start, again at the loop's first pass, after each finished unit of
// THREADBPWORKLOAD = 1048576 babies (93, clamped to M) but the last, then the 100 % line (2457) -- the
// checksums of the three layers, and the sort of the bP rows (not with --load-ptable, 2495).  With more
// threads the reference's count lines depend on its threads' timing; these are the single-thread ones.
void print_build_lines(const kh_bsgs_info &I) {
  const uint64_t m = I.m, w = std::min<uint64_t>(1048576, m), units = m / w + (m % w ? 1 : 0);
  auto count = [&](uint64_t f) {
    printf("\r[+] processing %llu/%llu bP points : %i%%\r", (unsigned long long)f, (unsigned long long)m,
           (int)(((double)f / (double)m) * 100));
  };
  count(0);
  for (uint64_t u = 0; u < units; u++) count(u * w);
  printf("\r[+] processing %llu/%llu bP points : 100%%     \n", (unsigned long long)m, (unsigned long long)m);
  printf("[+] Making checkums .. ... done\n");
  if (!opt.load_ptable) printf("[+] Sorting %llu elements... Done!\n", (unsigned long long)I.m3);
}

std::mutex g_setup_mtx;
std::condition_variable g_setup_cv;
bool g_setup_done = false;
void setup_done() {
  fflush(stdout);
  {
    std::lock_guard<std::mutex> lk(g_setup_mtx);
    g_setup_done = true;
  }
  g_setup_cv.notify_all();
}
void setup_wait() {
  std::unique_lock<std::mutex> lk(g_setup_mtx);
  g_setup_cv.wait(lk, [] { return g_setup_done; });
}

// -S (keyhunt.cpp:1983-2230, 2504-2652): the files of this N/k in the working directory are read
// when they are all there, else the tables are built and (by the first GPU's worker) written.
// -S with --mapped (keyhunt.cpp:1983 skips the reads, 2504-2652 still writes): the table files hold the
// mapped shard filters -- each shard's struct bloom as the mapping left it, its bits and their sha256
// twice -- and the sorted bP rows with their sha256, in the reference's order 4, 6, 2, 7
int write_mapped_tables(kh_ctx *ctx, const kh_bsgs_info &info, const std::vector<std::vector<mapped::filter>> &F) {
  const bsgs_names nm = bsgs_file_names(info.m, info.m2, info.m3);
  const std::string *blm[3] = {&nm.blm4, &nm.blm6, &nm.blm7};
  auto layer = [&](int l) {
    const char *fn = blm[l]->c_str();
    FILE *f = fopen(fn, "wb");
    if (!f) {
      fprintf(stderr, "[E] Error can't create the file %s\n", fn);
      return false;
    }
    bool ok = true;
    for (int i = 0; i < 256 && ok; i++) {
      uint8_t h[112], ck[32];
      mapped::struct_bloom(F[l][i], h);
      sha256(F[l][i].bf.data(), F[l][i].bytes, ck);
      ok = fwrite(h, 1, 112, f) == 112 && (F[l][i].bytes == 0 || fwrite(F[l][i].bf.data(), 1, F[l][i].bytes, f) == F[l][i].bytes) &&
           fwrite(ck, 1, 32, f) == 32 && fwrite(ck, 1, 32, f) == 32;
    }
    ok = fclose(f) == 0 && ok;
    if (!ok) fprintf(stderr, "[E] Error writing the file %s\n", fn);
    else printf("[+] Writing bloom filter to file %s .... Done!\n", fn);
    return ok;
  };
  if (!layer(0) || !layer(1)) return KH_E_IO;
  if (opt.load_ptable) return layer(2) ? KH_OK : KH_E_IO;  // no .tbl with --load-ptable (2588)
  const uint8_t *rows = nullptr;
  uint64_t n = 0;
  int r = kh_bsgs_table_rows(ctx, &rows, &n);
  if (r) return r;
  const char *fn = nm.tbl.c_str();
  FILE *f = fopen(fn, "wb");
  if (!f) {
    fprintf(stderr, "[E] Error can't create the file %s\n", fn);
    return KH_E_IO;
  }
  uint8_t ck[32];
  sha256(rows, n * 16, ck);
  bool ok = (n == 0 || fwrite(rows, 1, n * 16, f) == n * 16) && fwrite(ck, 1, 32, f) == 32;
  ok = fclose(f) == 0 && ok;
  if (!ok) {
    fprintf(stderr, "[E] Error writing the file %s\n", fn);
    return KH_E_IO;
  }
  printf("[+] Writing bP Table to file %s .. Done!\n", fn);
  return layer(2) ? KH_OK : KH_E_IO;
}

int bsgs_tables(kh_ctx *ctx, const kh_bsgs_info &info, bool first) {
  if (opt.mapped) {  // -S is skipped with --mapped (keyhunt.cpp:1983); the shards live in files
    int r = kh_bsgs_build(ctx);
    std::vector<std::vector<mapped::filter>> F;
    if (!r && first && !mapped::bsgs_layers(ctx, info, opt.save_read ? &F : nullptr)) r = KH_E_IO;
    if (!r && first) {
      print_allocating(info);
      ptable_md5_loaded();
      print_build_lines(info);
      if (opt.save_read) r = write_mapped_tables(ctx, info, F);
    }
    return r;
  }
  if (first) {
    print_layer_lines(info);
    print_allocating(info);
    ptable_md5_loaded();
  }
  if (!opt.save_read) {
    int r = kh_bsgs_build(ctx);
    if (!r && first) print_build_lines(info);
    return r;
  }
  const bsgs_names nm = bsgs_file_names(info.m, info.m2, info.m3);
  const char *f4 = nm.blm4.c_str(), *f6 = nm.blm6.c_str(), *f7 = nm.blm7.c_str(), *f2 = nm.tbl.c_str();
  if (opt.load_ptable) {
    // -S with --load-ptable (keyhunt.cpp:2153-2186): the reference reads the .tbl into its
    // read-only mapping of the --ptable file, which fails, or reports the .tbl missing; it never
    // writes the .tbl (2588)
    if (access(f2, F_OK) == 0) {
      fprintf(stderr, "[E] Error reading the file %s\n", f2);
    } else {
      fprintf(stderr, "[E] Missing bP table file %s\n", f2);
      fprintf(stderr, "    Remove --loadptable or generate the table first.\n");
    }
    return KH_E_IO;
  }
  static std::mutex mtx;
  static int decided = 0;  // 1: every worker reads the files, 2: every worker builds, the first writes
  {
    std::lock_guard<std::mutex> lk(mtx);
    if (!decided) {
      bool all = true;
      for (const char *f : {f4, f6, f7, f2}) all = all && access(f, R_OK) == 0;
      decided = all ? 1 : 2;
    }
  }
  if (decided == 1) {
    int r = kh_bsgs_load(ctx, ".", opt.skip_checksum ? KH_LOAD_SKIP_CHECKSUM : 0);
    if (r) {
      fprintf(stderr, "[E] %s\n", kh_last_error(ctx));
      return r;
    }
    if (first) {  // 1994-2225: a dot per 64 shards; nothing is built, checked or sorted after it
      printf("[+] Reading bloom filter from file %s .... Done!\n", f4);
      printf("[+] Reading bloom filter from file %s .... Done!\n", f6);
      printf("[+] Reading bP Table from file %s .... Done!\n", f2);
      printf("[+] Reading bloom filter from file %s .... Done!\n", f7);
    }
    return KH_OK;
  }
  int r = kh_bsgs_build(ctx);
  if (r || !first) return r;
  print_build_lines(info);
  r = kh_bsgs_save(ctx, ".");
  if (r) {
    fprintf(stderr, "[E] %s\n", kh_last_error(ctx));
    return r;
  }
  printf("[+] Writing bloom filter to file %s .... Done!\n", f4);
  printf("[+] Writing bloom filter to file %s .... Done!\n", f6);
  printf("[+] Writing bP Table to file %s .. Done!\n", f2);
  printf("[+] Writing bloom filter to file %s .... Done!\n", f7);
  return KH_OK;
}

// One found target, printed and recorded as the reference's worker does (keyhunt.cpp:4790-4830);
// returns true when every target is now found (the run then ends, 4811-4814)
bool print_found(kh_ctx *ctx, const bsgs_job *j, const kh_bsgs_found &fd) {
  uint32_t t = fd.target;
  {
    std::lock_guard<std::mutex> lk(g_found_mtx);
    if (g_found[t]) return false;
    g_found[t] = 1;
  }
  std::string k = u_hex(u_from_be32(fd.key));
  uint8_t pxy[64];
  kh_pubkeys(ctx, fd.key, 1, pxy);
  const std::string pub = pubkey_text(pxy, (*j->comp)[t]);
  {
    std::lock_guard<std::mutex> lk2(g_keys_mtx);
    // each BSGS worker of the reference has its own format: the sequential one (also -B ggsb and
    // angrygiant) continues its string over a backslash-newline, so no newline is printed
    // (keyhunt.cpp:4826-4827); random 5079, dance 5885, backward 6144, both 6429
    const int bm = opt.bsgs_mode;
    printf(bm == BM_SEQUENTIAL || bm == BM_GGSB || bm == BM_ANGRYGIANT ? "[+] Thread Key found privkey %s   "
           : bm == BM_RANDOM                                          ? "[+] Thread Key found privkey %s    \n"
                                                                      : "[+] Thread Key found privkey %s   \n",
           k.c_str());
    printf("[+] Publickey %s\n", pub.c_str());
    FILE *f = fopen("KEYFOUNDKEYFOUND.txt", "a");
    if (f) {
      fprintf(f, "Key found privkey %s\nPublickey %s\n", k.c_str(), pub.c_str());
      fclose(f);
    }
    fflush(stdout);
  }
  std::lock_guard<std::mutex> lk(g_found_mtx);
  return std::all_of(g_found.begin(), g_found.end(), [](uint8_t v) { return v != 0; });
}

// The per-base progress lines of the reference's BSGS workers, each printed as the worker takes the
// base (keyhunt.cpp:4618-4633; random 4955-4968, dance 5762-5774, backward 6023-6035, both
// 6308-6320): "[+] Thread 0x%s \n" with -M, else, unless -q, "\r[+] Thread 0x%s   \r" overwritten in
// place (the random worker pads with two spaces).  A call walks many bases: with -M every base's
// line is printed in the reference's order, each before the keys found in that base; otherwise the
// lines of a run of bases would overwrite one another, so the run's overlay is printed once -- what
// they leave on the terminal (the last line, completed by any longer earlier line).
struct base_lines {
  const bool on = opt.matrix || !opt.quiet;
  const char *sp = opt.bsgs_mode == BM_RANDOM ? "  " : opt.matrix ? " " : "   ";
  std::string overlay;  // the pending in-place lines, rendered
  void add(const U &base) {
    if (!on) return;
    const std::string ln = "[+] Thread 0x" + u_hex(base) + sp;
    if (opt.matrix) {
      printf("%s\n", ln.c_str());
      return;
    }
    if (ln.size() >= overlay.size())
      overlay = ln;
    else
      overlay.replace(0, ln.size(), ln);
  }
  void flush() {
    if (!overlay.empty()) printf("\r%s\r", overlay.c_str());
    overlay.clear();
    fflush(stdout);
  }
};

// The bases of one call, in the order the reference's worker takes them: `count` bases from `start`
// `step` apart, or an explicit list.  Each found key is reported after the progress line of the
// first base whose window (base, base + 2M * cycles * 1024] holds it -- the base a single reference
// thread finds it in.  Exits (status 1) when every target is found.
void report_call(kh_ctx *ctx, const bsgs_job *j, const kh_bsgs_info &info, const U &start, const U &step,
                 uint64_t count, const std::vector<U> *list, const std::vector<kh_bsgs_found> &found, uint32_t nf) {
  const uint64_t W = 2 * info.m * info.cycles * 1024;
  auto base_at = [&](uint64_t i) { return list ? (*list)[i] : u_add(start, u_mul_u64(step, i)); };
  std::vector<std::pair<uint64_t, uint32_t>> at;  // (base position, found index)
  for (uint32_t f = 0; f < nf && f < found.size(); f++) {
    const U key = u_from_be32(found[f].key);
    const uint64_t none = ~0ULL;
    uint64_t pos = none;
    if (list) {
      for (uint64_t i = 0; i < count; i++) {
        const U b = (*list)[i];
        if (u_cmp(key, b) > 0 && u_cmp(u_sub(key, b), u_from_u64(W)) <= 0) {
          pos = i;
          break;
        }
      }
    } else if (u_cmp(key, start) > 0 && step.v[1] == 0 && step.v[2] == 0 && step.v[3] == 0 && step.v[4] == 0 &&
               step.v[0]) {
      const U rel = u_sub(key, start);  // smallest b with rel <= b * step + W
      if (u_cmp(rel, u_from_u64(W)) > 0) {
        uint64_t rem = 0;
        const U q = u_divmod_u64(u_sub(rel, u_from_u64(W)), step.v[0], &rem);
        if (u_bitlen(q) < 63 && q.v[0] + (rem ? 1 : 0) < count) pos = q.v[0] + (rem ? 1 : 0);
      } else {
        pos = 0;
      }
    }
    if (pos == none) {
      // no base of the call holds the key in its window (base, base + W]: the engine found a key the
      // reference's per-base windows do not cover; it is printed after the call's last base line
      fprintf(stderr, "[W] key %s lies outside every base window of its call; printed after the call's last base\n",
              u_hex(key).c_str());
      pos = count ? count - 1 : 0;
    }
    at.push_back({pos, f});
  }
  std::sort(at.begin(), at.end());
  base_lines bl;
  uint64_t next = 0;
  for (auto &p : at) {
    if (bl.on) {
      for (; next <= p.first && next < count; next++) bl.add(base_at(next));
      bl.flush();
    }
    if (print_found(ctx, j, found[p.second])) {
      printf("All points were found\n");
      fflush(stdout);
      _exit(EXIT_FAILURE);  // keyhunt.cpp:4811-4814
    }
  }
  if (bl.on) {
    for (; next < count; next++) bl.add(base_at(next));
    bl.flush();
  }
}

void bsgs_worker(bsgs_job *j) {
  kh_ctx *ctx = nullptr;
  int r = kh_open(j->device, &ctx);
  if (r) {
    j->rc = r;
    if (j->first) setup_done();
    g_running--;
    return;
  }
  kh_bsgs_info info;
  r = kh_bsgs_set_layer1(ctx, opt.layer1);
  if (!r) r = kh_bsgs_set_bloom_multiplier(ctx, (uint32_t)opt.bloom_mult);
  if (!r) r = kh_bsgs_setup(ctx, j->n, j->k, &info);
  if (!r) r = bsgs_tables(ctx, info, j->first);
  if (!r) r = bsgs_ptable(ctx, info, j->first);
  // the first worker has printed the setup lines (or failed): the others' base lines follow them
  if (j->first)
    setup_done();
  else
    setup_wait();
  size_t nt = j->tx->size();
  std::vector<uint8_t> xy(64 * nt);
  for (size_t i = 0; i < nt; i++) {
    fe_to_be(&xy[64 * i], (*j->tx)[i]);
    fe_to_be(&xy[64 * i + 32], (*j->ty)[i]);
  }
  if (!r) r = kh_bsgs_set_targets(ctx, xy.data(), (uint32_t)nt);
  const U twoN = u_mul_u64(u_from_u64(info.n), 2);
  std::vector<kh_bsgs_found> found(nt + 1);
  std::vector<uint8_t> list_be;
  const bool progression = opt.bsgs_mode == BM_SEQUENTIAL || opt.bsgs_mode == BM_ANGRYGIANT || opt.bsgs_mode == BM_GGSB;
  // listed schedules (backward, both, random, dance): the next call's bases are drawn and packed on a
  // helper thread while the GPU walks the current call's (drawing, checking and packing 2^20 bases
  // took ~1/4 of a call's time on the host between calls)
  list_batch cur, nxt;
  if (!progression && !r) prepare_batch(twoN, j->list_bases_per_call, cur);
  while (!r) {
    if (!progression) {
      if (!cur.ok) break;
      std::thread pre([&]() { prepare_batch(twoN, j->list_bases_per_call, nxt); });
      const uint64_t nb = cur.drawn.size();
      uint32_t nf = 0;
      if (cur.consecutive)
        r = kh_bsgs_scan(ctx, cur.st_be, nb, found.data(), (uint32_t)found.size(), &nf);
      else
        r = kh_bsgs_scan_list(ctx, cur.be.data(), nb, found.data(), (uint32_t)found.size(), &nf);
      pre.join();
      if (r) {
        fprintf(stderr, "[E] kh_bsgs_scan: %s (%s)\n", kh_strerror(r), kh_last_error(ctx));
        break;
      }
      g_bases_done += nb;
      report_call(ctx, j, info, U{}, g_step, nb, &cur.drawn, found, nf);
      std::swap(cur, nxt);
      continue;
    }
    {
      U st;
      uint64_t nb = 0;
      if (!take_progression(g_step, u_cmp(g_step, twoN) == 0 ? j->bases_per_call : j->list_bases_per_call, st, nb))
        break;
      uint8_t st_be[32];
      u_to_be32(st, st_be);
      uint32_t nf = 0;
      if (u_cmp(g_step, twoN) == 0) {
        r = kh_bsgs_scan(ctx, st_be, nb, found.data(), (uint32_t)found.size(), &nf);
      } else {  // ggsb: bases 2 x block size apart, each walking its own 2N keys
        list_be.resize(32 * nb);
        U b = st;
        for (uint64_t i = 0; i < nb; i++, b = u_add(b, g_step)) u_to_be32(b, &list_be[32 * i]);
        r = kh_bsgs_scan_list(ctx, list_be.data(), nb, found.data(), (uint32_t)found.size(), &nf);
      }
      if (r) {
        fprintf(stderr, "[E] kh_bsgs_scan: %s (%s)\n", kh_strerror(r), kh_last_error(ctx));
        break;
      }
      g_bases_done += nb;
      report_call(ctx, j, info, st, g_step, nb, nullptr, found, nf);
    }
  }
  j->rc = r;
  kh_close(ctx);
  g_running--;
}

void usage(const char *p) {
  printf("Usage: %s -m address|rmd160|xpoint|bsgs -f FILE [-b BITS | -r START:END] [-l compress|uncompress|both]\n"
         "       [-n N] [-k K] [-I STRIDE] [-g GPUS] [-q] [-s SECONDS] [-M] [-L blocked|reference]\n"
         "       [-e] [-c btc|eth] [-R] [-B sequential|backward|both|random|dance|angrygiant] [-S] [-6]\n"
         "       [-z MULT] [-m vanity -v PREFIX ...] [--rmd-batch-size N] [--segwit] [--taproot] [-d] [-h]\n"
         "       --taproot (-m address): bc1p... lines of FILE are targets.  Only key-path-only outputs (BIP-86, no\n"
         "       script tree) can be found; a hit's key is the BIP-340 key of the internal key (tr(KEY)).\n"
#ifdef KH_WITH_MINIKEYS
         "       -m minikeys -f FILE [-C MINIKEY] [-8 ALPHABET] [-n N] [-R]\n"
#endif
         "       -m kangaroo -f FILE (-r START:END | -b BITS) [--dp BITS] [--herd N] [--seed U64] [-q]\n"
         "       Pollard's lambda search for the public keys of FILE (as -m bsgs reads it), one after another, in a\n"
         "       range of width 2^16 .. 2^192: about 2*sqrt(width) jumps whatever the width.  One GPU.\n"
         , p);
}

// ---------------------------------------------------------------------------------------------
// main's steps
// ---------------------------------------------------------------------------------------------
const U ORDER = [] {
  U o;
  u_from_hex(ORDER_HEX, o);
  return o;
}();

// The command line into opt and mapped::cfg, with the lines the reference prints as it reads each
// option.  False when the program ends here, with `status`.
bool parse_options(int argc, char **argv, int &status) {
  const char *mode_names[] = {"address", "rmd160", "xpoint", "bsgs", "vanity", "kangaroo", "minikeys"};
  static const struct option long_opts[] = {{"bsgs-block-count", required_argument, 0, 1},
                                           {"bsgs-block-size", required_argument, 0, 2},
                                           {"ptable", required_argument, 0, 3},
                                           {"ptable-size", required_argument, 0, 4},
                                           {"load-ptable", no_argument, 0, 5},
                                           {"ptable-cache", no_argument, 0, 6},
                                           {"mapped", optional_argument, 0, 7},
                                           {"mapped-size", required_argument, 0, 8},
                                           {"mapped-chunks", required_argument, 0, 9},
                                           {"bloom-file", required_argument, 0, 10},
                                           {"load-bloom", no_argument, 0, 11},
                                           {"bloom-bytes", required_argument, 0, 12},
                                           {"create-mapped", optional_argument, 0, 13},
                                           {"tmpdir", required_argument, 0, 14},
                                           {"rmd-batch-size", required_argument, 0, 15},
                                           {"segwit", no_argument, 0, 16},
                                           {"taproot", no_argument, 0, 17},
                                           {"dp", required_argument, 0, 18},
                                           {"herd", required_argument, 0, 19},
                                           {"seed", required_argument, 0, 20},
                                           {0, 0, 0, 0}};
  // --mapped-size / --bloom-bytes / --create-mapped N: the entry count and error the byte budget
  // allows (bloom_entries_for_bytes, keyhunt.cpp:7510-7530)
  auto size_override = [](uint64_t bytes) {
    uint32_t k;
    mapped::entries_for(bytes, &mapped::cfg.entries, &k);
    mapped::cfg.error = powl(0.5L, (long double)k);
  };
  auto fail = [&]() {
    status = EXIT_FAILURE;
    return false;
  };
#ifdef KH_WITH_MINIKEYS
  const char *short_opts = "m:f:l:r:b:k:n:t:g:qs:I:L:MRec:B:S6v:z:dhC:8:";
  const int n_modes = 7;
#else
  const char *short_opts = "m:f:l:r:b:k:n:t:g:qs:I:L:MRec:B:S6v:z:dh";
  const int n_modes = 6;
#endif
  int c;
  while ((c = getopt_long(argc, argv, short_opts, long_opts, nullptr)) != -1) {
    switch (c) {
#ifdef KH_WITH_MINIKEYS
      case 'C':  // keyhunt.cpp:896-919: the raw digits through the alphabet as it stands (a -8 before it counts)
        if (strlen(optarg) == 22) {
          const char *alpha = opt.alphabet ? opt.alphabet : B58;
          opt.have_minikey = true;
          opt.minikey_str = optarg;
          for (int i = 0; i < 21; i++) {
            const char *p = strchr(alpha, optarg[i + 1]);
            if (!p) {
              fprintf(stderr, "[E] invalid character in minikey\n");
              return fail();
            }
            g_mk_raw[i] = (uint8_t)((p - alpha) % 58);
          }
        } else {
          fprintf(stderr, "[E] Invalid Minikey length %li : %s\n", (long)strlen(optarg), optarg);
          return fail();
        }
        break;
      case '8':  // keyhunt.cpp:1102-1110
        if (strlen(optarg) == 58) {
          opt.alphabet = optarg;
          printf("[+] Base58 for Minikeys %s\n", opt.alphabet);
        } else {
          fprintf(stderr, "[E] The base58 alphabet must be 58 characters long.\n");
          return fail();
        }
        break;
#endif
      case 1:  // keyhunt.cpp:809-811: implies GGSB
        opt.ggsb_count = strtoull(optarg, NULL, 10);
        opt.ggsb = opt.ggsb_count > 0;
        break;
      case 2:  // keyhunt.cpp:812-814
        opt.ggsb_size = strtoull(optarg, NULL, 10);
        opt.ggsb = opt.ggsb_size > 0;
        break;
      case 3: opt.ptable = optarg; break;                    // keyhunt.cpp:772-773
      case 4: opt.ptable_size = parse_size(optarg); opt.ptable_given = true; break;   // keyhunt.cpp:774-785
      case 5: opt.load_ptable = true; break;                 // keyhunt.cpp:786-787
      case 6: opt.ptable_cache = true; break;                // keyhunt.cpp:788-789
      case 7:                                                // keyhunt.cpp:744-748
        opt.mapped = true;
        if (optarg) mapped::cfg.name = optarg;
        break;
      case 8:  // keyhunt.cpp:749-765, with the k/m/g/t suffixes
        opt.mapped = true;
        size_override(parse_size(optarg));
        break;
      case 9:  // keyhunt.cpp:766-768
        opt.mapped = true;
        mapped::cfg.chunks = (uint32_t)strtoul(optarg, NULL, 10);
        break;
      case 10: mapped::cfg.name = optarg; opt.mapped_given = true; break;      // keyhunt.cpp:768-769 (does not set --mapped)
      case 11: mapped::cfg.load_bloom = true; opt.mapped_given = true; break;  // keyhunt.cpp:770-771
      case 12:                                        // keyhunt.cpp:790-796
        opt.mapped = true;
        size_override(strtoull(optarg, NULL, 10));
        break;
      case 13:  // keyhunt.cpp:797-806
        opt.mapped = true;
        opt.create_mapped = true;
        if (optarg) size_override(strtoull(optarg, NULL, 10));
        break;
      case 14: break;  // --tmpdir: where the reference puts an unnamed bP table mapping; unused here
      case 15: {       // keyhunt.cpp:815-829: clamped to [4, 1024], rounded down to a multiple of 4
        long v = strtol(optarg, NULL, 10);
        if (v < 4) v = 4;
        if (v > 1024) v = 1024;
        if (v % 4) {
          v -= v % 4;
          if (v < 4) v = 4;
        }
        opt.rmd_batch = (int)v;
        break;
      }
      case 18: opt.kang_dp = (uint32_t)strtoul(optarg, NULL, 10); break;   // checked in check_kangaroo
      case 19: opt.kang_herd = (uint32_t)strtoul(optarg, NULL, 10); break;
      case 20:
        opt.kang_seed = strtoull(optarg, NULL, 0);
        opt.kang_seed_given = true;
        break;
      case 17: opt.taproot = true; break;  // -m address: bc1p... targets (checked in check_options)
      case 16: opt.segwit = true; break;  // -m address: bech32 and P2SH-P2WPKH targets (checked in check_options)
      case 'm': {
        int m = -1;
        for (int i = 0; i < n_modes; i++)
          if (!strcmp(optarg, mode_names[i])) m = i;
        if (m < 0) {
          fprintf(stderr, "[E] Unsupported mode %s (engine covers address, rmd160, xpoint, bsgs, vanity)\n", optarg);
          return fail();
        }
        opt.mode = m;
        if (m != MODE_BSGS) printf("[+] Mode %s\n", optarg);  // BSGS: "[+] Mode BSGS <schedule>" later
        break;
      }
      case 'f': opt.file = optarg; break;
      case 'v':  // keyhunt.cpp:1083-1100
        if (is_base58(optarg)) {
          if (addvanity(optarg, opt.vanity) > 0)
            printf("[+] Added Vanity search : %s\n", optarg);
          else
            printf("[+] Vanity search \"%s\" was NOT Added\n", optarg);
        } else {
          fprintf(stderr, "[+] The string \"%s\" is not Valid Base58\n", optarg);
        }
        break;
      case 'l':
        // keyhunt.cpp:945-960
        opt.l_given = true;
        if (!strcmp(optarg, "compress")) { opt.search = KH_SEARCH_COMPRESS; printf("[+] Search compress only\n"); }
        else if (!strcmp(optarg, "uncompress")) { opt.search = KH_SEARCH_UNCOMPRESS; printf("[+] Search uncompress only\n"); }
        else if (!strcmp(optarg, "both")) { opt.search = KH_SEARCH_BOTH; printf("[+] Search both compress and uncompress\n"); }
        else { fprintf(stderr, "[E] Unknow search type %s\n", optarg); return fail(); }
        break;
      case 'r': {  // keyhunt.cpp:1024-1055: START[:END]; START alone runs to the group order
        std::string s(optarg);
        size_t p = s.find(':');
        const std::string a = s.substr(0, p), b = p == std::string::npos ? std::string(ORDER_HEX) : s.substr(p + 1);
        if (!u_from_hex(a.c_str(), opt.start)) {
          fprintf(stderr, p == std::string::npos ? "[E] Invalid hexstring : %s.\n" : "[E] Invalid hexstring : %s\n",
                  a.c_str());
        } else if (!u_from_hex(b.c_str(), opt.end)) {
          fprintf(stderr, "[E] Invalid hexstring : %s\n", b.c_str());
        } else {
          opt.have_range = true;
          opt.range_start_str = a;
          opt.range_end_str = p == std::string::npos ? std::string() : b;  // empty: the order
        }
        break;
      }
      case 'b':
        opt.bits = atoi(optarg);
        if (opt.bits > 0 && opt.bits <= 256) {
          opt.have_bits = true;
        } else {
          fprintf(stderr, "[E] invalid bits param: %s.\n", optarg);
        }
        break;
      case 'k': opt.k_given = true; opt.kfactor = strtoull(optarg, nullptr, 10); if (!opt.kfactor) opt.kfactor = 1; printf("[+] K factor %llu\n", (unsigned long long)opt.kfactor); break;
      case 'n': opt.flag_n = true; opt.n = parse_n(optarg); break;
      case 't': {  // host threads: one per GPU context here (see -g); echoed as keyhunt.cpp:1076-1082 does
        long t = strtol(optarg, NULL, 10);
        if (t <= 0) t = 1;
        printf(t > 1 ? "[+] Threads : %u\n" : "[+] Thread : %u\n", (unsigned)t);
        break;
      }
      case 'g': opt.gpus = atoi(optarg); break;
      case 'q': opt.quiet = true; printf("[+] Quiet thread output\n"); break;
      case 's':  // keyhunt.cpp:1059-1072
        opt.seconds = atoi(optarg);
        if (opt.seconds < 0) opt.seconds = 30;
        if (opt.seconds == 0)
          printf("[+] Turn off stats output\n");
        else
          printf("[+] Stats output every %d seconds\n", opt.seconds);
        break;
      case 'I': {
        U s;
        bool ok = (optarg[0] == '0' && optarg[1] == 'x') ? u_from_hex(optarg, s) : u_from_dec(optarg, s);
        if (!ok || u_is_zero(s)) { fprintf(stderr, "[E] invalid stride %s\n", optarg); return fail(); }
        opt.stride = s;
        opt.stride_set = true;
        break;
      }
      case 'M': opt.matrix = true; printf("[+] Matrix screen\n"); break;  // keyhunt.cpp:960-963
      case 'L':  // BSGS layer-1 layout on the GPU (engine option; the reference has one layout)
        if (!strcmp(optarg, "reference")) opt.layer1 = KH_LAYER1_REFERENCE;
        else if (!strcmp(optarg, "blocked")) opt.layer1 = KH_LAYER1_BLOCKED;
        else { fprintf(stderr, "[E] -L reference|blocked\n"); return fail(); }
        break;
      case 'R':  // keyhunt.cpp:1019-1023
        printf("[+] Random mode\n");
        opt.random = true;
        opt.bsgs_mode = BM_RANDOM;
        break;
      case 'B': {  // keyhunt.cpp:841-853
        opt.B_given = true;
        int idx = -1;
        for (int i = 0; i < 7; i++)
          if (!strcmp(optarg, BSGS_MODES[i])) idx = i;
        if (idx < 0) {
          fprintf(stderr, "[W] Ignoring unknow bsgs mode %s\n", optarg);
        } else {
          opt.bsgs_mode = idx;  // GGSB reuses the sequential worker (keyhunt.cpp:2764-2767)
          if (idx == BM_GGSB) opt.ggsb = true;
        }
        break;
      }
      case 'e':  // keyhunt.cpp:925-931
        opt.endo = true;
        printf("[+] Endomorphism enabled\n");
        break;
      case 'S': opt.save_read = true; break;  // keyhunt.cpp:1073-1075
      case '6':  // keyhunt.cpp:837-840
        opt.skip_checksum = true;
        fprintf(stderr, "[W] Skipping checksums on files\n");
        break;
      case 'c':  // keyhunt.cpp:874-891
        opt.crypto_given = true;
        if (!strcmp(optarg, "btc")) {
          opt.eth = false;
        } else if (!strcmp(optarg, "eth")) {
          opt.eth = true;
          printf("[+] Setting search for ETH adddress.\n");
        } else {
          fprintf(stderr, "[E] Unknow crypto value %s\n", optarg);
          return fail();
        }
        break;
      case 'z':  // keyhunt.cpp:1112-1118: bloom entries = multiplier x items above 10000 (7608)
        opt.bloom_mult = (int)strtol(optarg, NULL, 10);
        if (opt.bloom_mult <= 0) opt.bloom_mult = 1;
        mapped::cfg.bloom_mult = opt.bloom_mult;
        printf("[+] Bloom Size Multiplier %i\n", opt.bloom_mult);
        break;
      case 'd':  // keyhunt.cpp:1019-1022
        printf("[+] Flag DEBUG enabled\n");
        break;
      case 'h':
        usage(argv[0]);
        status = EXIT_SUCCESS;
        return false;
      default: usage(argv[0]); return fail();
    }
  }
  if (opt.load_ptable && !opt.ptable) {  // keyhunt.cpp:1126-1129
    fprintf(stderr, "--load-ptable requires --ptable <file>\n");
    return fail();
  }
  if (opt.create_mapped && opt.mode != MODE_KANGAROO) {  // keyhunt.cpp:1131-1172: make the file(s) from the whole command line and exit
    status = mapped::create();
    return false;
  }
  return true;
}

// -m kangaroo takes -f, -r / -b, -g 1, -q, -s, -t and its own --dp, --herd, --seed; every option that shapes
// another mode's search is refused, one line each, before any GPU is opened
bool check_kangaroo() {
  const char *why = opt.endo                                                  ? "-e (endomorphism) doesn't work with -m kangaroo"
                    : opt.stride_set                                          ? "-I (stride) doesn't work with -m kangaroo"
                    : opt.B_given                                             ? "-B (BSGS schedule) doesn't work with -m kangaroo"
                    : opt.k_given                                             ? "-k (BSGS k factor) doesn't work with -m kangaroo"
                    : opt.flag_n                                              ? "-n doesn't work with -m kangaroo"
                    : opt.save_read                                           ? "-S doesn't work with -m kangaroo (there are no tables to save)"
                    : opt.crypto_given                                        ? "-c doesn't work with -m kangaroo (the targets are public keys)"
                    : opt.l_given                                             ? "-l doesn't work with -m kangaroo (the targets are public keys)"
                    : opt.segwit                                              ? "--segwit doesn't work with -m kangaroo"
                    : opt.taproot                                             ? "--taproot doesn't work with -m kangaroo"
                    : (opt.mapped || opt.create_mapped || opt.mapped_given)   ? "the mapped bloom options don't work with -m kangaroo"
                    : (opt.ptable || opt.load_ptable || opt.ptable_cache || opt.ptable_given)
                        ? "the ptable options don't work with -m kangaroo"
                    : opt.gpus > 1                                            ? "-m kangaroo runs on one GPU (-g 1)"
                    : (opt.kang_dp > 32 && opt.kang_dp != KH_KANG_DP_AUTO)    ? "--dp takes 0 .. 32"
                    : opt.kang_herd > (1u << 24)                              ? "--herd takes at most 16777216"
                    : (!opt.have_bits && !opt.have_range)
                        ? "-m kangaroo needs a bounded range: -r START:END or -b BITS"
                        : nullptr;
  if (why) {
    fprintf(stderr, "[E] %s\n", why);
    return false;
  }
  return true;
}

// The checks on the options together, and the lines that follow them (keyhunt.cpp:1173-1220)
bool check_options() {
  if (!opt.file && !(opt.mode == MODE_VANITY && opt.vanity.targets)) {
    fprintf(stderr, "[E] -f FILE is required\n");
    return false;
  }
  if (opt.mode == MODE_KANGAROO) return check_kangaroo();
  if (!validate_nk(opt.n, opt.kfactor)) return false;  // keyhunt.cpp:1173-1183: applied to every mode
  // keyhunt.cpp:1185-1193 compares the -B index with MODE_BSGS (2), i.e. these two guards fire
  // for -B both whatever -m is (SURVEY 8a parity note 7); BSGS itself ignores -e and -I
  if (opt.bsgs_mode == BM_BOTH && opt.endo) {
    fprintf(stderr, "[E] Endomorphism doesn't work with BSGS\n");
    return false;
  }
  if (opt.bsgs_mode == BM_BOTH && opt.stride_set) {
    fprintf(stderr, "[E] Stride doesn't work with BSGS\n");
    return false;
  }
  // --segwit: -m address with compressed keys only, and no -S (the data_<hex>.dat cache keeps no address
  // type, so a run that reads it could not know whether to probe the nested digests)
  if (opt.segwit) {
    const char *why = opt.mode != MODE_ADDRESS         ? "--segwit works with -m address only"
                      : opt.eth                        ? "--segwit doesn't work with -c eth"
                      : opt.search == KH_SEARCH_UNCOMPRESS ? "--segwit doesn't work with -l uncompress (segwit keys are compressed)"
                      : opt.save_read                  ? "--segwit doesn't work with -S (the data file keeps no address type)"
                                                       : nullptr;
    if (why) {
      fprintf(stderr, "[E] %s\n", why);
      return false;
    }
  }
  // --taproot: -m address with bitcoin targets; no -e (each image would need its own tweak) and no -S (the
  // data_<hex>.dat cache keeps 20-byte rows only)
  if (opt.taproot) {
    const char *why = opt.mode != MODE_ADDRESS ? "--taproot works with -m address only"
                      : opt.eth                ? "--taproot doesn't work with -c eth"
                      : opt.endo               ? "--taproot doesn't work with -e (each image would need its own tweak)"
                      : opt.save_read          ? "--taproot doesn't work with -S (the data file keeps no witness programs)"
                                               : nullptr;
    if (why) {
      fprintf(stderr, "[E] %s\n", why);
      return false;
    }
  }
  if (opt.stride_set) printf("[+] Stride : %s\n", u_dec(opt.stride).c_str());  // keyhunt.cpp:1195-1203
  if (opt.mode == MODE_BSGS) printf("[+] Mode BSGS %s\n", BSGS_MODES[opt.bsgs_mode]);  // keyhunt.cpp:1209-1211
  if (opt.mode == MODE_ADDRESS && !opt.crypto_given) printf("[+] Setting search for btc adddress\n");  // 1217-1220
  return true;
}

// opt.start / opt.end and the cursors from -b, -r or neither (keyhunt.cpp:854-873, 1221-1269)
void setup_range() {
  if (opt.have_bits) {
    opt.start = u_shl1(opt.bits - 1);
    opt.end = u_shl1(opt.bits);
    if (u_cmp(opt.end, ORDER) > 0) opt.end = ORDER;
  } else if (opt.have_range) {
    if (u_is_zero(opt.start)) opt.start = u_from_u64(1);
    if (u_cmp(opt.start, opt.end) == 0) {
      fprintf(stderr, "[E] Start and End range can't be the same\nFallback to random mode!\n");
      opt.have_range = false;
    } else if (u_cmp(opt.start, ORDER) >= 0 || u_cmp(opt.end, ORDER) > 0) {
      fprintf(stderr, "[E] Start and End range can't be great than N\nFallback to random mode!\n");
      opt.have_range = false;
    } else {
      if (u_cmp(opt.start, opt.end) > 0) {
        fprintf(stderr, "[W] Opps, start range can't be great than end range. Swapping them\n");
        std::swap(opt.start, opt.end);
      }
    }
  }
  if (!opt.have_bits && !opt.have_range) {
    // no usable range (keyhunt.cpp:1250-1255, 1534-1540): the address family walks sequentially
    // from 1 to the group order; BSGS starts at a random key below the order and walks up
    opt.start = opt.mode == MODE_BSGS ? u_rand_range(u_from_u64(1), ORDER) : u_from_u64(1);
    opt.end = ORDER;
  }
  g_cursor = opt.start;
  g_end = opt.end;
  g_top = opt.end;
}

// the range lines: the address family prints them after "[+] N =" with the range as used
// (keyhunt.cpp:1325-1339); BSGS after reading its targets, with -r's strings as typed and nothing
// for a random start (1517-1540)
void print_range() {
  if (opt.mode == MODE_BSGS && !opt.have_bits && !opt.have_range) return;
  printf(opt.have_bits ? "[+] Bit Range %d\n" : "[+] Range \n", opt.bits);
  if (opt.mode == MODE_BSGS && !opt.have_bits)
    printf("[+] -- from : 0x%s\n[+] -- to   : 0x%s\n", opt.range_start_str.c_str(),
           opt.range_end_str.empty() ? u_hex(ORDER).c_str() : opt.range_end_str.c_str());
  else
    printf("[+] -- from : 0x%s\n[+] -- to   : 0x%s\n", u_hex(opt.start).c_str(), u_hex(opt.end).c_str());
}

// What the worker threads read until they are joined.
// -g contexts: one host thread + kh_ctx each, on device d % ndev.  More contexts than devices
// share a device (as the reference's -t threads share the host's cores); each keeps its own
// tables and lanes, and they all take work from the one cursor (keyhunt.cpp:3321-3324, 4600-4617).
struct run {
  int ndev = 0, gpus = 0;
  std::vector<addr_job> aj;
  std::vector<bsgs_job> bj;
  std::vector<std::thread> th;
  std::vector<uint8_t> rows;
  std::string data_file;  // -S target cache
  std::vector<fe> tx, ty;
  std::vector<bool> comp;
  U twoN;
};

// The devices are counted once the targets are read, so the reference's lines come first.
bool open_devices(run &R) {
  kh_device_count(&R.ndev);
  if (R.ndev < 1) {
    fprintf(stderr, "[E] no GPU found\n");
    return false;
  }
  R.gpus = opt.gpus > 0 ? opt.gpus : R.ndev;
  printf("[+] GPUs : %d (%d context%s)\n", std::min(R.gpus, R.ndev), R.gpus, R.gpus == 1 ? "" : "s");
  R.aj.resize(R.gpus);
  R.bj.resize(R.gpus);
  g_running = R.gpus;
  return true;
}

// -m address / rmd160 / xpoint / vanity / minikeys: the targets (from the file, or -S's data file), the
// mapped filter, the memory check, then one worker per context.  0 when they run, else the exit status.
int run_address_family(run &R) {
  std::vector<uint8_t> &rows = R.rows;
  std::string &data_file = R.data_file;
  uint64_t nseq = 0x100000000ULL;  // N_SEQUENTIAL_MAX (keyhunt.cpp:464, 1272-1292)
  if (opt.flag_n) {
    nseq = opt.n;
    if (nseq < 1024 || nseq % 1024) nseq = 0x100000000ULL;
  }
  printf("[+] N = %p\n", (void *)nseq);
  if (opt.mode == MODE_MINIKEYS) {  // keyhunt.cpp:1293-1323: the base if given, no range lines
    if (opt.have_minikey) {
      printf("[+] Base Minikey : %s\n", opt.minikey_str.c_str());
    } else {  // a random base (3148-3157), drawn here instead of by the first worker
      std::random_device rd;
      for (int k = 0; k < 21; k++) g_mk_raw[k] = (uint8_t)((rd() & 0xFF) % 58);
    }
    minikey_n_init(nseq);
  } else {
    print_range();
  }
  uint64_t items = 0;
  // -S: read the target cache if it exists (FLAGREADEDFILE1), else read the file and write it
  bool have_data = false;
  if (opt.save_read && opt.mode != MODE_VANITY) {
    if (!data_file_name(opt.file, data_file)) {
      fprintf(stderr, "[E] sha256_file error\n");
      return EXIT_FAILURE;
    }
    FILE *df = fopen(data_file.c_str(), "rb");
    if (df) {
      fseeko(df, 0, SEEK_END);
      const off_t size = ftello(df);
      fclose(df);
      have_data = true;
      printf("[+] Reading file %s\n", data_file.c_str());
      // a file too short for the bloom checksum or its struct bloom fails the reference's first two
      // reads (readFileAddress, keyhunt.cpp:7068, 7076; the caller's message at 1347): e.g. the empty
      // data file an -S --mapped-chunks N>1 run leaves behind (below)
      if (size < 32 + 112) {  // checksum + struct bloom (112 B, kh_mapped.h struct_bloom)
        fprintf(stderr, "[E] %s reading file, code line %d\n", size < 32 ? "Errore" : "Error", size < 32 ? 7068 : 7076);
        fprintf(stderr, "[E] Unenexpected error\n");
        return EXIT_FAILURE;
      }
    }
  }
  // -S with --mapped and no cache yet: the target filter is the mapped file's (bloom.dat, or the
  // --mapped / --bloom-file name), and that filter -- its struct bloom and bits -- goes into the
  // data file (keyhunt.cpp:7033-7049, 7630-7706, 7756-7855).  With --mapped-chunks above 1 the
  // reference writes bloom.bytes from its FIRST chunk's mapping (bloom.bf = bf_chunks[0],
  // bloom.cpp:395), past that mapping's end (handled below)
  const bool mapped_data = opt.mapped && opt.save_read && opt.mode != MODE_VANITY && !have_data;
  const bool mapped_data_chunked = mapped_data && mapped::cfg.chunks > 1;
  mapped::filter tf;
  std::vector<uint8_t> adds;  // the items the reference adds to its (mapped) target bloom
  std::vector<uint8_t> *addp = opt.mapped ? &adds : nullptr;
  if (have_data) {
    // rows and bloom come from the file, in each GPU's kh_targets_load
  } else if (opt.mode == MODE_VANITY) {
    if (!read_vanity(opt.file)) return EXIT_FAILURE;
  } else if (opt.eth && opt.mode == MODE_ADDRESS) {
    if (!read_targets_eth(opt.file, rows, items, addp)) return EXIT_FAILURE;
  } else if (!read_targets(opt.file, opt.mode, rows, items, addp)) {
    return EXIT_FAILURE;
  }
  if (opt.segwit)
    printf("[+] Segwit targets: %llu bech32, %llu P2SH-P2WPKH\n", (unsigned long long)g_seg_bech32,
           (unsigned long long)g_seg_p2sh);
  if (opt.taproot) printf("[+] Taproot targets: %llu\n", (unsigned long long)(g_tap_progs.size() / 32));
  if (opt.mapped) {
    bool ok;
    if (opt.mode == MODE_VANITY) {  // the vanity bloom: the first min_bytes bytes of every A
      const uint32_t L = (uint32_t)opt.vanity.min_bytes;
      for (size_t j = 0; j < opt.vanity.ranges.size(); j += 40)
        adds.insert(adds.end(), opt.vanity.ranges.begin() + j, opt.vanity.ranges.begin() + j + L);
      ok = mapped::targets(opt.vanity.total, adds, L);
    } else {
      ok = mapped::targets(items, adds, 20, mapped_data && !mapped_data_chunked ? &tf : nullptr);
    }
    if (!ok) return EXIT_FAILURE;
  }
  if (mapped_data_chunked) {
    // The reference maps and fills the chunk files, opens data_<hex>.dat for writing, then hashes
    // bloom.bytes from the first chunk's mapping and dies of SIGBUS past its end (writeFileIfNeeded,
    // keyhunt.cpp:7770-7809): the chunk files hold the filter, the data file is left empty, and the next
    // -S run fails reading it (tests/golden/ref_mapped.json "rmd160_S_mapped_chunks").  This CLI leaves
    // the same files and exits with an error status instead of the signal.
    FILE *f = fopen(data_file.c_str(), "wb");
    if (f) fclose(f);
    fflush(stdout);
    fprintf(stderr, "[E] -S with --mapped-chunks %u: the data file would be written from the first chunk's mapping "
                    "past its end (the reference dies of SIGBUS there); %s left empty\n",
            (unsigned)mapped::cfg.chunks, data_file.c_str());
    return EXIT_FAILURE;
  }
  if (!have_data)
    printf("[+] Sorting data ... done! %llu values were loaded and sorted\n", (unsigned long long)(rows.size() / 20));
  if (mapped_data) {
    printf("[D] size data %llu\n", (unsigned long long)rows.size());
    if (!write_mapped_data_file(data_file, tf, rows)) {
      fprintf(stderr, "[E] Error writing file %s\n", data_file.c_str());
      return EXIT_FAILURE;
    }
    printf("[+] Writing file %s ........\n", data_file.c_str());
    data_file.clear();  // the contexts take their targets from the rows
  }
  if (!open_devices(R)) return EXIT_FAILURE;
  // contexts stacked on one device must fit its free memory (each holds its own inversion pad,
  // kh_scan_memory): checked before any is opened, as bsgsd-amd checks its BSGS tables
  // (-m minikeys has no walk and no pad: a queue of a few MB per context)
  const uint32_t mode = scan_mode();
  uint64_t need = 0;
  if (opt.mode != MODE_MINIKEYS && kh_scan_memory(nseq, mode, (uint32_t)opt.search, &need) == KH_OK) {
    std::vector<uint64_t> dev_free(R.ndev, 0);
    for (int dev = 0; dev < R.ndev && dev < R.gpus; dev++)
      if (kh_device_memory(dev, &dev_free[dev], nullptr) != KH_OK) dev_free[dev] = 0;
    if (!contexts_fit(R.gpus, R.ndev, need, dev_free, "-n")) return EXIT_FAILURE;
  }
  for (int d = 0; d < R.gpus; d++) {
    addr_job &j = R.aj[d];
    j.device = d % R.ndev;
    j.index = d;
    j.rows = &rows;
    // initBloomFilter (keyhunt.cpp:7608): max(10000, items), times -z above the floor
    const uint64_t nitems = items ? items : rows.size() / 20;
    j.bloom_items = nitems <= 10000 ? nitems : nitems * (uint64_t)opt.bloom_mult;
    j.nseq = nseq;
    j.mode = mode;
    if (!data_file.empty()) {
      j.data_file = data_file.c_str();
      j.save_data = !have_data && d == 0;  // one GPU writes the cache
    }
    R.th.emplace_back(opt.mode == MODE_MINIKEYS ? mini_worker : addr_worker, &j);
  }
  return 0;
}

// keyhunt.cpp:1369-1446: N = lines of 66+ characters; each such line's first token (separators
// " \t:") is a public key of 66 or 130 characters (ParsePublicKeyHex), else "Invalid length".
// 0, or the exit status.
int read_bsgs_targets(run &R) {
  FILE *f = fopen(opt.file, "r");
  if (!f) {
    fprintf(stderr, "[E] Can't open file %s\n", opt.file);
    return EXIT_FAILURE;
  }
  printf("[+] Opening file %s\n", opt.file);
  std::vector<std::string> lines = fgets_pieces(f, 1022);
  fclose(f);
  size_t counted = 0;
  for (auto &ln : lines) counted += ln.size() >= 66;
  if (!counted) {
    fprintf(stderr, "[E] There is no valid data in the file\n");
    return EXIT_FAILURE;
  }
  for (auto &ln : lines) {
    if (ln.size() < 66) continue;
    std::vector<char> buf(ln.begin(), ln.end());
    buf.push_back(0);
    char *tok = strtok(buf.data(), " \t:");
    const size_t tl = tok ? strlen(tok) : 0;
    fe x, y;
    bool cp = false;
    if (tl == 66 || tl == 130) {
      const int r = parse_pubkey_hex_ref(tok, x, y, cp);
      if (r < 0) return 255;  // the reference's exit(-1)
      if (r > 0) {
        R.tx.push_back(x);
        R.ty.push_back(y);
        R.comp.push_back(cp);
      }
    } else {
      printf("Invalid length: %s\n", tok ? tok : "");
    }
  }
  if (R.tx.empty()) {
    fprintf(stderr, "[E] The file don't have any valid publickeys\n");
    return EXIT_FAILURE;
  }
  printf("[+] Added %zu points from file\n", R.tx.size());
  return 0;
}

// -m bsgs: the targets, N and the GGSB geometry with their lines, then one worker per context.
// 0 when they run, else the exit status.
int run_bsgs(run &R) {
  if (int rc = read_bsgs_targets(R)) return rc;
  print_range();
  g_found.assign(R.tx.size(), 0);
  // BSGS N: -n or 2^44 (keyhunt.cpp:1454-1471); the library validates sqrt / 1024 and derives M
  const uint64_t n = opt.n;
  if (u_cmp(u_sub(opt.end, opt.start), u_from_u64(n)) < 0) {
    fprintf(stderr, "[E] the given range is small\n");
    return EXIT_FAILURE;
  }
  uint64_t m = 1;
  while ((m + 1) * (m + 1) <= n) m++;
  const uint64_t M = m * opt.kfactor, Nr = (n / M) * M;
  R.twoN = u_mul_u64(u_from_u64(Nr), 2);
  printf("[+] N = 0x%llx\n", (unsigned long long)Nr);
  // GGSB block geometry from sqrt(N) (keyhunt.cpp:1477-1499) and the base step (1617-1627)
  g_step = R.twoN;
  uint64_t ggsb_blocks = 1, ggsb_babies = M;
  if (opt.ggsb) {
    uint64_t bc = opt.ggsb_count, bs = opt.ggsb_size;
    if (bc == 0 && bs == 0) bc = 1;
    if (bc > 0 && bs == 0)
      bs = (m + bc - 1) / bc;
    else if (bs > 0 && bc == 0)
      bc = (m + bs - 1) / bs;
    if (bc == 0) bc = 1;
    if (bs == 0) bs = m;
    if (bc > 1 && bs) g_step = u_mul_u64(u_from_u64(bs), 2);
    ggsb_blocks = bc > 1 ? bc : 1;
    if (bs) ggsb_babies = bs;
  }
  {
    // keyhunt.cpp:1663-1685 (stderr): the build's layout and the expected layer / table sizes
    const uint64_t items = M / 256 > 10000 ? M / 256 + (M % 256 ? 1 : 0) : 1000;
    const long double err = opt.mapped && mapped::cfg.error ? mapped::cfg.error : 0.000001L;
    const double shard_mb = (double)mapped::bytes_for(items, err) / 1048576.0;
    fprintf(stderr, "[i] BSGS table build: %s layout, creating %llu block(s) of %llu babies each.\n",
            ggsb_blocks > 1 ? "GGSB" : "classic", (unsigned long long)ggsb_blocks, (unsigned long long)ggsb_babies);
    fprintf(stderr, "[i] Expected sizes: each bloom layer ~%.2f MB (256 shards), bPtable ~%.2f MB per block (%.2f MB total).\n",
            shard_mb * 256.0, (double)(ggsb_babies * 16) / 1048576.0, (double)(M * 16) / 1048576.0);
  }
  if (opt.mapped && opt.save_read && mapped::cfg.chunks > 1) {
    // the reference writes each shard's bits from its first chunk's mapping, past that mapping's end
    fprintf(stderr, "[E] -S with --mapped-chunks above 1: the reference writes the table files from each shard's "
                    "first chunk mapping past its end; not provided\n");
    return EXIT_FAILURE;
  }
  if (!open_devices(R)) return EXIT_FAILURE;
  // ~2^35 giant points per engine call (16 pipelined rounds, ~1 s): the end of a call drains
  // the pipeline (the last round's second check, the hit copies), which at 2^31 points per call
  // cost 7 % of the rate (profiles/r03f_cli_rate_bsgs.json); a call returns as soon as every
  // target is found.  Listed schedules take calls of the same size (at 2^31 points per call,
  // -B random ran 17 % and -B both 9 % below sequential: profiles/r05k_cli_rate_bsgs_*.json).
  // A range of fewer bases than that is dealt out evenly over the contexts (the reference's
  // threads take one base each, keyhunt.cpp:4600-4617)
  const uint64_t aux = Nr / M, pts = ((aux + 1023) / 1024) * 1024;
  uint64_t per_call = std::max<uint64_t>(1, (1ULL << 35) / pts);
  if (g_step.v[1] == 0 && g_step.v[2] == 0 && g_step.v[3] == 0 && g_step.v[4] == 0) {
    uint64_t rem = 0;
    const U nb = u_divmod_u64(u_sub(opt.end, opt.start), g_step.v[0], &rem);
    if (u_bitlen(nb) <= 40) {
      const uint64_t bases = nb.v[0] + (rem ? 1 : 0), share = (bases + R.gpus - 1) / R.gpus;
      per_call = std::max<uint64_t>(1, std::min(per_call, share));
    }
  }
  for (int d = 0; d < R.gpus; d++) {
    bsgs_job &j = R.bj[d];
    j.device = d % R.ndev;
    j.first = d == 0;
    j.tx = &R.tx;
    j.ty = &R.ty;
    j.comp = &R.comp;
    j.n = n;
    j.k = opt.kfactor;
    j.bases_per_call = j.list_bases_per_call = per_call;
    R.th.emplace_back(bsgs_worker, &j);
  }
  return 0;
}

// -m kangaroo: the range as the inclusive interval [a, b] the library takes (-b BITS: 2^(BITS-1) .. 2^BITS - 1; -r
// A:B as typed; an end at the group order stops one below it), or false with the message when its width
// is outside the method's limits
bool kangaroo_range(U &a, U &b) {
  if (!opt.have_bits && !opt.have_range) {  // setup_range refused -r's values
    fprintf(stderr, "[E] -m kangaroo needs a bounded range: -r START:END or -b BITS\n");
    return false;
  }
  a = opt.start;
  b = opt.have_bits || u_cmp(opt.end, ORDER) >= 0 ? u_sub(opt.end, u_from_u64(1)) : opt.end;
  const int wl = u_cmp(b, a) > 0 ? u_bitlen(u_sub(b, a)) : 0;
  if (wl <= 16 || wl > 192) {
    fprintf(stderr, "[E] -m kangaroo needs a range at least 2^16 and less than 2^192 keys wide\n");
    return false;
  }
  return true;
}

// -m kangaroo: the targets as -m bsgs reads them, then one kh_kang_solve loop per target, in file order, on
// one context.  A found key is printed and recorded as the sequential BSGS worker's.  The exit status.
int run_kangaroo(run &R, const U &a, const U &b) {
  if (int rc = read_bsgs_targets(R)) return rc;
  print_range();
  if (!open_devices(R)) return EXIT_FAILURE;
  kh_ctx *ctx = nullptr;
  int r = kh_open(0, &ctx);
  if (r) {
    fprintf(stderr, "[E] kh_open: %s\n", kh_strerror(r));
    return EXIT_FAILURE;
  }
  const uint64_t seed = opt.kang_seed_given ? opt.kang_seed : ((uint64_t)std::random_device{}() << 32) | std::random_device{}();
  uint8_t ab[32], bb[32];
  u_to_be32(a, ab);
  u_to_be32(b, bb);
  long double sqrt_w = 0;
  {
    const U w = u_sub(b, a);
    for (int i = 3; i >= 0; i--) sqrt_w = sqrt_w * 18446744073709551616.0L + (long double)w.v[i];
    sqrt_w = sqrtl(sqrt_w);
  }
  printf("[+] Kangaroo seed %llu\n", (unsigned long long)seed);
  int rc = EXIT_SUCCESS;
  for (size_t t = 0; t < R.tx.size() && rc == EXIT_SUCCESS; t++) {
    uint8_t pub[64], key[32];
    fe_to_be(pub, R.tx[t]);
    fe_to_be(pub + 32, R.ty[t]);
    if (!r) r = kh_kang_setup(ctx, pub, ab, bb, opt.kang_dp, nullptr);
    if (!r) r = kh_kang_seed(ctx, seed, opt.kang_herd);
    uint32_t herd = 0, dp = 0, spl = 0, found = 0;
    if (!r) r = kh_kang_geometry(ctx, nullptr, &spl, &herd, &dp);
    if (!r && herd) printf("[+] Kangaroo target %zu: herd %u, dp %u\n", t + 1, herd, dp);
    // calls of about a second: one launch first, then as many jumps as the measured rate does in that time
    uint64_t per_call = (uint64_t)herd * spl;
    kh_kang_stats st{};
    const auto t0 = std::chrono::steady_clock::now();
    while (!r && !found) {
      const auto c0 = std::chrono::steady_clock::now();
      const uint64_t before = st.jumps;
      r = kh_kang_solve(ctx, per_call, key, &found, &st);
      const auto c1 = std::chrono::steady_clock::now();
      const double dt = std::chrono::duration<double>(c1 - c0).count(), all = std::chrono::duration<double>(c1 - t0).count();
      if (dt > 0 && st.jumps > before) per_call = std::max<uint64_t>((uint64_t)herd * spl, (uint64_t)((st.jumps - before) / dt));
      if (!opt.quiet && !r) {
        printf("\r[+] Kangaroo: %.3e jumps, %.3e jumps/s, %llu DPs, %.2Lf x sqrt(W)   %s", (double)st.jumps,
               all > 0 ? st.jumps / all : 0.0, (unsigned long long)st.dps, sqrt_w > 0 ? st.jumps / sqrt_w : 0.0L,
               found ? "\n" : "\r");
        fflush(stdout);
      }
    }
    if (r) {
      fprintf(stderr, "[E] kangaroo: %s (%s)\n", kh_strerror(r), kh_last_error(ctx));
      rc = EXIT_FAILURE;
      break;
    }
    const std::string k = u_hex(u_from_be32(key));
    uint8_t pxy[64];
    kh_pubkeys(ctx, key, 1, pxy);
    const std::string pubt = pubkey_text(pxy, R.comp[t]);
    printf("[+] Thread Key found privkey %s   ", k.c_str());  // the sequential BSGS worker's lines (print_found)
    printf("[+] Publickey %s\n", pubt.c_str());
    FILE *f = fopen("KEYFOUNDKEYFOUND.txt", "a");
    if (f) {
      fprintf(f, "Key found privkey %s\nPublickey %s\n", k.c_str(), pubt.c_str());
      fclose(f);
    }
    fflush(stdout);
  }
  kh_close(ctx);
  printf("\nEnd\n");
  return rc;
}

// the stats loop (keyhunt.cpp:2850-2962) until every worker has ended; the program's exit status
int wait_for_workers(run &R) {
  uint64_t secs = 0;
  while (g_running > 0) {
    sleep(1);
    secs++;
    if (opt.seconds > 0 && secs % opt.seconds == 0) print_stats(secs, keys_done(R.twoN));
  }
  for (auto &t : R.th) t.join();
  int rc = 0;
  for (int d = 0; d < R.gpus; d++) rc |= (opt.mode == MODE_BSGS ? R.bj[d].rc : R.aj[d].rc);
  printf("\nEnd\n");
  return rc ? EXIT_FAILURE : EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char **argv) {
  printf("[+] Version %s\n", VERSION);
  int status = EXIT_FAILURE;
  if (!parse_options(argc, argv, status)) return status;
  if (!check_options()) return EXIT_FAILURE;
  setup_range();
  run R;
  if (opt.mode == MODE_KANGAROO) {
    U a, b;
    if (!kangaroo_range(a, b)) return EXIT_FAILURE;
    return run_kangaroo(R, a, b);
  }
  if (int rc = opt.mode == MODE_BSGS ? run_bsgs(R) : run_address_family(R)) return rc;
  return wait_for_workers(R);
}
