"""The file-level steps both host programs share (host/kh_bsgs_files.h: the -S names, ptable_prepare /
ptable_write_rows / ptable_load_rows, md5_refresh, bptable_cache_refresh) and the argument parsers
(host/kh_host_util.h parse_size / parse_n), without a GPU: compiled into a stand-alone program under
AddressSanitizer and UBSan and compared with hashlib.md5 and the struct bptable_cache_file model
(tests/_bptable.py)."""
import hashlib
import os
import shutil
import struct
import subprocess

import pytest

from _bptable import cache_model
from keyhunt_amd import engine as E

PT_OK, PT_OPEN, PT_STAT, PT_SMALL, PT_MAP, PT_RESIZE, PT_WRITE = range(7)
ROWS = bytes((7 * i + 1) & 0xFF for i in range(128))          # 8 rows, as the driver's `fill` writes them
MIB = 1 << 20

DRIVER = r'''
#include "kh_bsgs_files.h"
using namespace khh;
int main(int n, char **v) {
  const std::string cmd = n > 1 ? v[1] : "";
  if (cmd == "size") {
    for (int i = 2; i < n; i++) printf("%llu\n", (unsigned long long)parse_size(v[i]));
  } else if (cmd == "n") {
    for (int i = 2; i < n; i++) printf("%llu\n", (unsigned long long)parse_n(v[i]));
  } else if (cmd == "names") {
    const bsgs_names nm = bsgs_file_names(strtoull(v[2], 0, 10), strtoull(v[3], 0, 10), strtoull(v[4], 0, 10));
    printf("%s %s %s %s\n", nm.blm4.c_str(), nm.blm6.c_str(), nm.blm7.c_str(), nm.tbl.c_str());
  } else if (cmd == "fill") {  // PATH ROWS_BYTES PTABLE_SIZE: prepare, then the rows (7 i + 1) mod 256
    const uint64_t bytes = strtoull(v[3], 0, 10);
    std::vector<uint8_t> rows(bytes);
    for (uint64_t i = 0; i < bytes; i++) rows[i] = (uint8_t)(7 * i + 1);
    const int e = ptable_prepare(v[2], bytes, parse_size(v[4]));
    printf("%d %d\n", e, e ? 0 : (int)ptable_write_rows(v[2], rows.data(), bytes));
  } else if (cmd == "load") {  // PATH ROWS_BYTES
    ptable_rows r;
    const int e = ptable_load_rows(v[2], strtoull(v[3], 0, 10), r);
    printf("%d %s\n", e, e ? "-" : hex(r.data, (int)r.bytes).c_str());
  } else if (cmd == "md5") {  // PATH REPORT
    uint8_t m[16] = {0};
    const bool ok = md5_refresh(v[2], m, atoi(v[3]) != 0);
    printf("%d %s\n", (int)ok, hex(m, 16).c_str());
  } else if (cmd == "cache") {  // TARGET (a file of whole rows): its MD5, then TARGET.cache checked
    ptable_rows r;
    struct stat st;
    uint8_t m[16];
    if (stat(v[2], &st) || ptable_load_rows(v[2], (uint64_t)st.st_size, r) || !md5_of_file(v[2], m)) return 2;
    bptable_cache_refresh(v[2], m, r.data, (uint64_t)st.st_size / 16);
  } else {
    return 3;
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("bsgs_files")
    src, exe = d / "d.cpp", d / "d"
    src.write_text(DRIVER)
    inc = os.path.join(os.path.dirname(E.PKG), "include")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(E.PKG, "host"), "-I", inc, "-o", str(exe), str(src)], check=True)

    def run(*args, stderr=""):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, check=True)
        assert r.stderr == stderr
        return r.stdout
    return run


def test_parse_size(drv):
    got = drv("size", "4k", "3M", "2g", "1T", "12345", "7x", "5K", "0").split()
    assert [int(g) for g in got] == [4 << 10, 3 << 20, 2 << 30, 1 << 40, 12345, 7, 5 << 10, 0]


def test_parse_n(drv):
    got = drv("n", "1048576", "0x100000", "0X1000000", "0", "0xfF").split()
    assert [int(g) for g in got] == [1048576, 0x100000, 0x1000000, 0, 255]


def test_table_file_names(drv):
    assert drv("names", 4096, 204, 10) == ("keyhunt_bsgs_4_4096.blm keyhunt_bsgs_6_204.blm keyhunt_bsgs_7_10.blm "
                                           "keyhunt_bsgs_2_10.tbl\n")


def test_new_ptable_file_is_the_rows(drv, tmp_path):
    f = tmp_path / "bp.tbl"
    assert drv("fill", f, 128, 0) == "0 1\n"
    assert f.read_bytes() == ROWS
    assert (f.stat().st_mode & 0o777) == 0o600 & ~_umask()


def _umask():
    m = os.umask(0)
    os.umask(m)
    return m


def test_ptable_size_grows_with_zeros(drv, tmp_path):
    f = tmp_path / "bp.tbl"
    assert drv("fill", f, 128, "4k") == "0 1\n"
    assert f.read_bytes() == ROWS + bytes(4096 - 128)


def test_existing_file_is_not_shrunk(drv, tmp_path):
    """What is zeroed is the mapping, max(rows, --ptable-size) bytes; a longer file keeps the rest."""
    f = tmp_path / "bp.tbl"
    f.write_bytes(b"\xAA" * 8192)
    assert drv("fill", f, 128, 0) == "0 1\n"
    assert f.read_bytes() == ROWS + b"\xAA" * (8192 - 128)
    assert drv("fill", f, 128, "4k") == "0 1\n"
    assert f.read_bytes() == ROWS + bytes(4096 - 128) + b"\xAA" * 4096


@pytest.mark.parametrize("size,kept", [(MIB - 16, False), (MIB, True), (MIB + 16, True)])
def test_one_mib_rule(drv, tmp_path, size, kept):
    """A mapping of less than 1 MiB is zeroed before the rows go in; from exactly 1 MiB on its bytes stay."""
    f = tmp_path / "bp.tbl"
    f.write_bytes(b"\xAA" * size)
    assert drv("fill", f, 128, size) == "0 1\n"
    assert f.read_bytes() == ROWS + (b"\xAA" if kept else b"\0") * (size - 128)
    if kept:  # and so without --ptable-size, where the mapping is the rows alone
        f.write_bytes(b"\xAA" * size)
        assert drv("fill", f, 128, 0) == "0 1\n"
        assert f.read_bytes() == ROWS + b"\xAA" * (size - 128)


def test_load_rows_failures_are_distinct(drv, tmp_path):
    assert drv("load", tmp_path / "missing.tbl", 128) == f"{PT_OPEN} -\n"
    (tmp_path / "short.tbl").write_bytes(bytes(100))
    assert drv("load", tmp_path / "short.tbl", 128) == f"{PT_SMALL} -\n"


def test_load_rows_leaves_the_file_alone(drv, tmp_path):
    f = tmp_path / "bp.tbl"
    data = ROWS + b"\x55" * 72
    f.write_bytes(data)
    os.utime(f, ns=(10**18, 10**18))
    assert drv("load", f, 128) == f"{PT_OK} {ROWS.hex()}\n"
    assert f.read_bytes() == data and f.stat().st_mtime_ns == 10**18


def test_md5_refresh(drv, tmp_path):
    f, m = tmp_path / "bp.tbl", tmp_path / "bp.tbl.md5"
    f.write_bytes(ROWS * 3)
    want = hashlib.md5(ROWS * 3).hexdigest()
    assert drv("md5", f, 1) == f"1 {want}\n"                                           # no .md5 yet: no line
    assert m.read_text() == want + "\n"
    assert drv("md5", f, 1) == f"[+] bP table MD5 verified ({m})\n1 {want}\n"
    m.write_text("0" * 32 + "\n")
    assert drv("md5", f, 1) == f"[W] bP table MD5 mismatch ({m}); refreshing\n1 {want}\n"
    assert m.read_text() == want + "\n"
    m.write_text("0" * 32 + "\n")
    assert drv("md5", f, 0) == f"1 {want}\n"                                           # no report, still rewritten
    assert m.read_text() == want + "\n"
    gone = tmp_path / "none.tbl"
    assert drv("md5", gone, 1, stderr=f"[W] Unable to compute MD5 for bP table {gone}\n") == f"0 {'00' * 16}\n"
    assert not (tmp_path / "none.tbl.md5").exists()


def test_cache_refresh(drv, tmp_path):
    f, c = tmp_path / "c.tbl", tmp_path / "c.tbl.cache"
    rows = b"".join(bytes([v]) + bytes(15) for v in (0, 0, 3, 3, 3, 9, 200, 255))        # sorted by value[0]
    f.write_bytes(rows)
    model = cache_model(rows)
    made = f"[I] bP table cache not found ({c}); creating\n[+] bP table cache refreshed ({c})\n"
    rebuilt = f"[W] bP table cache mismatch ({c}); rebuilding\n[+] bP table cache refreshed ({c})\n"
    assert drv("cache", f) == made and c.read_bytes() == model
    assert struct.unpack_from("<257Q", model, 32)[:5] == (0, 2, 2, 2, 5)
    assert drv("cache", f) == f"[+] bP table cache hit ({c})\n" and c.read_bytes() == model
    c.write_bytes(cache_model(bytes([1]) + rows[1:]))                                  # another MD5, same M3
    assert drv("cache", f) == rebuilt and c.read_bytes() == model
    other_m3 = bytearray(model)
    struct.pack_into("<Q", other_m3, 8, 7)                                             # this MD5, another M3
    c.write_bytes(bytes(other_m3))
    assert drv("cache", f) == rebuilt and c.read_bytes() == model
