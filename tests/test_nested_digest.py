"""hash160_nested (kh_math.h): the P2SH-P2WPKH (BIP-49) script hash RIPEMD160(SHA256(00 14 || h)) of a
key hash h, as the KH_MODE_P2SH walks and resolve_hits compute it.

The header is compiled for the host into a stand-alone program that reads 20-byte digests as hex lines
and prints hash160_nested of each, and the pair form hash160_nested2 of each line with its successor.
Checked against the public vectors (BIP-173's key 1, BIP-49's account key), the oracle's SHA-256 and
RIPEMD-160 on 1,000 seeded random inputs, and the inputs whose bytes 0, 1, 18, 19 -- the ones that cross
the 16-bit shift of the block packing -- are 00, 80 and ff.  The same program is built once more with
-fsanitize=address,undefined and run on the whole input."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "keyhunt_amd", "csrc")

PROGRAM = r'''
#include <stdio.h>
#include <string.h>
#include "kh_math.h"
using namespace kh;
static bool rd(uint32_t w[5], const char *s) {
  uint8_t b[20];
  if (strlen(s) < 40) return false;
  for (int i = 0; i < 20; i++) { unsigned v; if (sscanf(s + 2 * i, "%2x", &v) != 1) return false; b[i] = (uint8_t)v; }
  memcpy(w, b, 20);   // 5 little-endian words = the 20 digest bytes in order
  return true;
}
static void pr(const uint32_t w[5]) {
  uint8_t b[20];
  memcpy(b, w, 20);
  for (int i = 0; i < 20; i++) printf("%02x", b[i]);
}
int main() {
  static char line[128];
  uint32_t prev[5], cur[5], o[5], oa[5], ob[5];
  bool have = false;
  while (fgets(line, sizeof line, stdin)) {
    if (!rd(cur, line)) return 2;
    hash160_nested(cur, o);
    pr(o);
    if (have) {   // the pair form on (previous, this): both outputs
      hash160_nested2(prev, cur, oa, ob);
      printf(" "); pr(oa); printf(" "); pr(ob);
    }
    printf("\n");
    memcpy(prev, cur, 20);
    have = true;
  }
  return 0;
}
'''

# key, hash160(compressed pubkey), nested
VECTORS = [
    (1, "751e76e8199196d454941c45d1b3a323f1433bd6", "bcfeb728b584253d5f3f70bcb780e9ef218a68f4"),
    (0xc9bdb49cfbaedca21c4b1f3a7803c34636b1d7dc55a717132443fc3f4c5867e8,
     "38971f73930f6c141d977ac4fd4a727c854935b3", "336caa13e08b96080a32b5d818d59b4ab3b36742"),
]


def _inputs():
    rng = random.Random(0x5e9517)
    ins = [bytes.fromhex(v[1]) for v in VECTORS]
    ins += [rng.randbytes(20) for _ in range(1000)]
    for e in itertools.product((0x00, 0x80, 0xff), repeat=4):   # bytes 0, 1, 18, 19
        b = bytearray(rng.randbytes(20))
        b[0], b[1], b[18], b[19] = e
        ins.append(bytes(b))
    ins += [bytes(20), bytes([0xff] * 20), bytes([0x80] * 20)]
    return ins


def _build(tmp_path, name, flags):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = tmp_path / (name + ".cpp")
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-I", CSRC, *flags, "-o", str(exe), str(src)], check=True)
    return exe


def _run(exe, ins):
    out = subprocess.run([str(exe)], input="".join(h.hex() + "\n" for h in ins), capture_output=True, text=True,
                         check=True)
    assert out.stderr == ""
    return [ln.split() for ln in out.stdout.splitlines()]


def _check(oracle, ins, got):
    want = [oracle.ripemd160(oracle.sha256(b"\x00\x14" + h)).hex() for h in ins]
    assert len(got) == len(ins)
    for i, g in enumerate(got):
        assert g[0] == want[i], ins[i].hex()
        if i:
            assert g[1:] == [want[i - 1], want[i]], ins[i].hex()   # the pair form


def test_oracle_composition_gives_the_public_vectors(oracle):
    for k, h, nested in VECTORS:
        x, y = oracle.pubkey(k)
        assert oracle.hash160_comp(x, 2 + (y & 1)).hex() == h
        assert oracle.ripemd160(oracle.sha256(b"\x00\x14" + bytes.fromhex(h))).hex() == nested
    # the addresses of the nested hashes: base58check(05 || nested)
    assert oracle.address_decode("3JvL6Ymt8MVWiCNHC7oWU6nLeHNJKLZGLN")[1:21].hex() == VECTORS[0][2]
    assert oracle.address_decode("36NvZTcMsMowbt78wPzJaHHWaNiyR73Y4g")[1:21].hex() == VECTORS[1][2]


def test_hash160_nested_vectors_random_and_shift_edges(oracle, tmp_path):
    ins = _inputs()
    assert len(ins) == 2 + 1000 + 81 + 3
    got = _run(_build(tmp_path, "nested", ["-O1"]), ins)
    assert got[0][0] == VECTORS[0][2] and got[1][0] == VECTORS[1][2]
    _check(oracle, ins, got)


def test_hash160_nested_under_address_and_undefined_sanitizers(oracle, tmp_path):
    ins = _inputs()
    exe = _build(tmp_path, "nested_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _check(oracle, ins, _run(exe, ins))
