"""The host's BIP-173 codec for mainnet P2WPKH (host/kh_host_util.h bech32_p2wpkh_decode / _encode), as
--segwit's target reader and hit text use it: compiled into a stand-alone program and compared with the
public vectors and with BIP-173's reference algorithm as tests/_segwit.py restates it."""
import os
import shutil
import subprocess

import pytest

from keyhunt_amd import engine as E
from _segwit import BECH32M, encode

# hash160(compressed pubkey) -> bc1q... : BIP-173's own vector (key 1) and BIP-49's account key
VECTORS = [("751e76e8199196d454941c45d1b3a323f1433bd6", "bc1qw508d6qejxtdg4y5r3zarvary0c5xw7kv8f3t4"),
           ("38971f73930f6c141d977ac4fd4a727c854935b3", "bc1q8zt37uunpakpg8vh0tz06jnj0jz5jddn7ayctz")]


@pytest.fixture(scope="module")
def codec(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("bech32")
    src = d / "b.cpp"
    # each argument: decoded program as hex and its re-encoding, or "-" when the decoder refuses it
    src.write_text('#include "kh_host_util.h"\nint main(int n, char **v) {\n'
                   '  for (int i = 1; i < n; i++) { uint8_t p[20];\n'
                   '    if (!khh::bech32_p2wpkh_decode(v[i], p)) { printf("-\\n"); continue; }\n'
                   '    printf("%s %s\\n", khh::hex(p, 20).c_str(), khh::bech32_p2wpkh_encode(p).c_str()); }\n'
                   '  return 0; }\n')
    exe = d / "b"
    inc = os.path.join(os.path.dirname(E.PKG), "include")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(E.PKG, "host"), "-I", inc, "-o", str(exe), str(src)], check=True)

    def run(*strings):
        r = subprocess.run([str(exe), *strings], capture_output=True, text=True, check=True)
        assert r.stderr == ""
        return [ln.split() for ln in r.stdout.splitlines()]
    return run


def test_restated_reference_algorithm_gives_the_public_vectors():
    for h, addr in VECTORS:
        assert encode("bc", 0, bytes.fromhex(h)) == addr


def test_decode_and_encode_of_the_vectors(codec):
    for h, addr in VECTORS:
        assert codec(addr) == [[h, addr]]


def test_upper_case_form_is_accepted_and_encodes_lower(codec):
    for h, addr in VECTORS:
        assert codec(addr.upper()) == [[h, addr]]


def test_round_trip_of_edge_programs(codec):
    progs = [bytes(20), bytes([0xff] * 20), bytes(range(1, 21)), bytes([0x80] + [0] * 18 + [0x01])]
    addrs = [encode("bc", 0, p) for p in progs]
    assert all(len(a) == 42 for a in addrs)
    assert codec(*addrs) == [[p.hex(), a] for p, a in zip(progs, addrs)]


def test_rejected_strings(codec):
    h = bytes.fromhex(VECTORS[0][0])
    good = VECTORS[0][1]
    mixed = good[:10] + good[10:].upper()
    flipped = [good[:i] + ("q" if good[i] != "q" else "p") + good[i + 1:] for i in (4, 20, 41)]
    tb = encode("tb", 0, h)                                   # testnet hrp, valid checksum, 42 characters
    p2wsh = encode("bc", 0, bytes(range(32)))                 # 62-character v0 program
    bc1p_m = encode("bc", 1, h, BECH32M)                      # 42 characters, version 1, bech32m
    bc1p_plain = encode("bc", 1, h)                           # version 1 under the bech32 constant
    v0_m = encode("bc", 0, h, BECH32M)                        # version 0 under the bech32m constant
    taproot = "bc1p0xlxvlhemja6c4dqv22uapctqupfhlxm9h8z3k2e72q4k9hcz7vqzk5jj0"   # BIP-350's vector
    short, long_ = encode("bc", 0, h[:19] + b""), good + "q"
    assert len(tb) == 42 and len(p2wsh) == 62 and len(bc1p_m) == 42 and bc1p_m.startswith("bc1p")
    assert len(good[:41]) == 41 and len(long_) == 43 and len(short) != 42
    bad = [mixed, *flipped, tb, p2wsh, bc1p_m, bc1p_plain, v0_m, taproot, good[:41], long_, short,
           "bc1" + "b" * 39, "1BgGZ9tcN4rm9KBzDn7KprQz87SZ26SAMH", ""]
    assert codec(*bad) == [["-"]] * len(bad)
