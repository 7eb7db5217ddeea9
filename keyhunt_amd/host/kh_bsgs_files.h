// kh_bsgs_files.h -- the files a BSGS start reads and writes besides the mapped bloom files (kh_mapped.h):
// the names of the -S table files, the --ptable file (keyhunt.cpp:1847-1956; bsgsd.cpp:1314-1470) and
// --ptable-cache's FILE.md5 and FILE.cache (keyhunt.cpp:137-143, 186-241, 1958-1981, 2655-2700;
// bsgsd.cpp:255-360, 1444-1462, 1648-1665).  The steps only: bin/keyhunt-amd and bin/bsgsd-amd call them
// in the order of their own reference program, each with its own error texts.  No GPU calls.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "kh_host_util.h"

namespace khh {

// -S: the three layers' filters and the sorted bP rows of a table set (M, M2, M3)
struct bsgs_names {
  std::string blm4, blm6, blm7, tbl;
};
inline bsgs_names bsgs_file_names(uint64_t m, uint64_t m2, uint64_t m3) {
  return {"keyhunt_bsgs_4_" + std::to_string(m) + ".blm", "keyhunt_bsgs_6_" + std::to_string(m2) + ".blm",
          "keyhunt_bsgs_7_" + std::to_string(m3) + ".blm", "keyhunt_bsgs_2_" + std::to_string(m3) + ".tbl"};
}

// where a step on the --ptable file stopped
enum ptable_err { PT_OK, PT_OPEN, PT_STAT, PT_SMALL, PT_MAP, PT_RESIZE, PT_WRITE };

// --ptable FILE before the rows are known: created if missing, grown to max(rows_bytes, ptable_size) and
// never shrunk; a file of less than 1 MiB is then zeroed (keyhunt.cpp:1941-1951; bsgsd.cpp:1424-1431), a
// larger one keeps its bytes.  PT_WRITE: the zeroes could not be written
inline ptable_err ptable_prepare(const char *path, uint64_t rows_bytes, uint64_t ptable_size) {
  const uint64_t map_bytes = std::max(rows_bytes, ptable_size);
  int fd = open(path, O_RDWR | O_CREAT, 0600);
  if (fd < 0) return PT_OPEN;
  struct stat st;
  ptable_err e = PT_OK;
  if (fstat(fd, &st) != 0 || ((uint64_t)st.st_size < map_bytes && ftruncate(fd, (off_t)map_bytes) != 0)) {
    e = PT_RESIZE;
  } else if (map_bytes < (1ull << 20)) {
    std::vector<uint8_t> zero(map_bytes, 0);
    if (pwrite(fd, zero.data(), map_bytes, 0) != (ssize_t)map_bytes) e = PT_WRITE;
  }
  if (close(fd) != 0 && !e) e = PT_WRITE;
  return e;
}

// the sorted rows into the head of the prepared file; the bytes after them stay
inline bool ptable_write_rows(const char *path, const uint8_t *rows, uint64_t rows_bytes) {
  int fd = open(path, O_RDWR);
  if (fd < 0) return false;
  bool ok = true;
  for (uint64_t o = 0; ok && o < rows_bytes;) {
    ssize_t w = pwrite(fd, rows + o, rows_bytes - o, (off_t)o);
    ok = w > 0;
    if (ok) o += (uint64_t)w;
  }
  return close(fd) == 0 && ok;
}

// --load-ptable: the first rows_bytes of FILE mapped read-only, as the reference maps them
// (keyhunt.cpp:1880-1900); the file is never written
struct ptable_rows {
  const uint8_t *data = nullptr;
  uint64_t bytes = 0;
  ptable_rows() = default;
  ptable_rows(const ptable_rows &) = delete;
  ptable_rows &operator=(const ptable_rows &) = delete;
  ~ptable_rows() {
    if (data) munmap((void *)data, bytes);
  }
};
inline ptable_err ptable_load_rows(const char *path, uint64_t rows_bytes, ptable_rows &out) {
  int fd = open(path, O_RDONLY);
  if (fd < 0) return PT_OPEN;
  struct stat st;
  ptable_err e = PT_OK;
  if (fstat(fd, &st) != 0) {
    e = PT_STAT;
  } else if ((uint64_t)st.st_size < rows_bytes) {
    e = PT_SMALL;
  } else if (rows_bytes) {
    void *m = mmap(nullptr, rows_bytes, PROT_READ, MAP_SHARED, fd, 0);
    if (m == MAP_FAILED) {
      e = PT_MAP;
    } else {
      out.data = (const uint8_t *)m;
      out.bytes = rows_bytes;
    }
  }
  close(fd);
  return e;
}

// FILE.md5 as keyhunt writes and reads it: the hex MD5 and a newline (keyhunt.cpp:186-241)
inline bool read_md5_file(const char *path, uint8_t out[16]) {
  char buf[64] = {0};
  FILE *f = fopen(path, "r");
  if (!f) return false;
  size_t n = fread(buf, 1, sizeof buf - 1, f);
  fclose(f);
  buf[n] = 0;
  if (char *nl = strchr(buf, '\n')) *nl = 0;
  if (strlen(buf) < 32) return false;
  buf[32] = 0;
  return hex2bin(buf, out, 16);
}
inline bool write_md5_file(const char *path, const uint8_t md5[16]) {
  FILE *f = fopen(path, "w");
  bool ok = f && fprintf(f, "%s\n", hex(md5, 16).c_str()) > 0;
  if (f) ok = fclose(f) == 0 && ok;
  return ok;
}
// MD5 of `path` into md5 and into path.md5; with `report`, an earlier path.md5 is compared first
// (keyhunt.cpp:1956-1981; bsgsd.cpp:1444-1462, 1648-1665).  False when the file cannot be read
inline bool md5_refresh(const std::string &path, uint8_t md5[16], bool report) {
  const std::string md5_path = path + ".md5";
  if (!md5_of_file(path.c_str(), md5)) {
    fprintf(stderr, "[W] Unable to compute MD5 for bP table %s\n", path.c_str());
    return false;
  }
  uint8_t disk[16];
  if (report && read_md5_file(md5_path.c_str(), disk))
    printf(memcmp(disk, md5, 16) == 0 ? "[+] bP table MD5 verified (%s)\n" : "[W] bP table MD5 mismatch (%s); refreshing\n",
           md5_path.c_str());
  if (!write_md5_file(md5_path.c_str(), md5)) fprintf(stderr, "[W] Unable to write bP table MD5 file %s\n", md5_path.c_str());
  return true;
}

// FILE.cache: struct bptable_cache_file {magic 'BPTC', version 1, entries, md5, 257 bucket starts by
// value[0] of the 16-byte rows} (keyhunt.cpp:137-143, 186-241; bsgsd.cpp:255-360)
#pragma pack(push, 1)
struct bptable_cache_file {
  uint32_t magic, version;
  uint64_t entries;
  uint8_t md5[16];
  uint64_t boundaries[257];
};
#pragma pack(pop)
static_assert(sizeof(bptable_cache_file) == 2088, "struct bptable_cache_file");
// 1: a cache of this MD5 and row count, -1: another one, 0: none readable
inline int bptable_cache_status(const char *path, const uint8_t md5[16], uint64_t m3) {
  bptable_cache_file disk;
  FILE *f = fopen(path, "rb");
  if (!f) return 0;
  int st = 0;
  if (fread(&disk, sizeof disk, 1, f) == 1)
    st = disk.magic == 0x42505443u && disk.version == 1 && disk.entries == m3 && !memcmp(disk.md5, md5, 16) ? 1 : -1;
  fclose(f);
  return st;
}
inline bool bptable_cache_write(const char *path, const uint8_t md5[16], const uint8_t *rows, uint64_t m3) {
  bptable_cache_file fc;
  memset(&fc, 0, sizeof fc);
  fc.magic = 0x42505443u;
  fc.version = 1;
  fc.entries = m3;
  memcpy(fc.md5, md5, 16);
  uint64_t pos = 0;
  for (int bucket = 0; bucket < 256; bucket++) {
    while (pos < m3 && rows[pos * 16] < bucket) pos++;
    fc.boundaries[bucket] = pos;
  }
  fc.boundaries[256] = m3;
  FILE *f = fopen(path, "wb");
  bool ok = f && fwrite(&fc, sizeof fc, 1, f) == 1;
  if (f) ok = fclose(f) == 0 && ok;
  return ok;
}
// target.cache against the target's MD5 and row count: kept when it is of both, else (re)built from the rows
inline void bptable_cache_refresh(const std::string &target, const uint8_t md5[16], const uint8_t *rows, uint64_t m3) {
  const std::string cache = target + ".cache";
  const int st = bptable_cache_status(cache.c_str(), md5, m3);
  if (st == 1) {
    printf("[+] bP table cache hit (%s)\n", cache.c_str());
    return;
  }
  printf(st < 0 ? "[W] bP table cache mismatch (%s); rebuilding\n" : "[I] bP table cache not found (%s); creating\n",
         cache.c_str());
  if (bptable_cache_write(cache.c_str(), md5, rows, m3))
    printf("[+] bP table cache refreshed (%s)\n", cache.c_str());
  else
    printf("[W] Unable to write bP table cache to %s\n", cache.c_str());
}

}  // namespace khh
