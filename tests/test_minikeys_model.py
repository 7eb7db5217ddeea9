"""-m minikeys without a GPU: the Python model (tests/_minikeys_model.py) against the reference CLI's own
two-chunk run (tests/golden/ref_minikeys.json, tests/golden/make_minikeys_golden.py), and the argument
handling and header of bin/minikeys-amd, which is keyhunt-amd's source built with -DKH_WITH_MINIKEYS."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import tempfile

import keyhunt_amd
from keyhunt_amd import engine as E
from conftest import DATA, GOLDEN

import _minikeys_model as M

REF = json.load(open(os.path.join(GOLDEN, "ref_minikeys.json")))
CLI = os.path.join(E.PKG, "bin", "minikeys-amd")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
BASE_LINE = re.compile(r"\[\+\] Base minikey: (S[^?\n]{21})\?     \n")


def records(text: str) -> list[dict]:
    return [dict(zip(("key", "pubkey", "minikey", "address"), m.groups())) for m in re.finditer(
        r"Private Key: ([0-9a-f]+)\npubkey: ([0-9a-f]+)\nminikey: (\S+)\naddress: (\S+)\n", text)]


def header_lines(text: str) -> list[str]:
    """The lines before the first chunk's base line, without the version line and the device count."""
    m = BASE_LINE.search(text)
    return [l for l in (text[:m.start()] if m else text).split("\n")
            if l and not l.startswith("[+] Version") and not l.startswith("[+] GPUs : ")]


def run(argv, cwd=None, env=None):
    return subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=cwd, env=env, timeout=60)


def test_base_advance_matches_reference():
    """increment_minikey_N: the second chunk's base line of the reference's run is base + 253 N."""
    bases = BASE_LINE.findall(REF["stdout"])
    assert bases[0] == REF["base"] and len(bases) == 2
    d = M.digits_of(REF["base"])
    assert M.text_of(M.advance(d, REF["n"])) == bases[1]
    assert M.value_of(M.advance(d, REF["n"])) - M.value_of(d) == 253 * REF["n"]
    mn, limit = M.minikey_n(REF["n"])
    assert limit == 6 and M.value_of(mn[:21]) == 253 * REF["n"]


def test_known_answer_and_overlap_records():
    """The model's key, public key and address of the README's known answer and of the overlap target
    equal the reference's records; the overlap target is recorded twice, once per chunk that meets it."""
    d = M.digits_of(REF["base"])
    assert M.candidate(d, 3000) == REF["known"] and M.is_valid(REF["known"])
    assert [o for o in M.valid_offsets(d, 3000)].index(3000) == 4
    recs = records(REF["keyfound"])
    assert recs == [M.record_of(REF["known"]), M.record_of(REF["overlap"]), M.record_of(REF["overlap"])]
    assert len(recs[0]["key"]) == 63  # GetBase16 drops the leading zero
    second = M.advance(d, REF["n"])
    off = M.value_of(M.digits_of(REF["overlap"])) - M.value_of(second)
    assert 0 < off < 3 * REF["n"] - (1 << 20) and M.is_valid(REF["overlap"])
    targets = open(os.path.join(DATA, "minikeys.txt")).read().split()
    assert targets == [recs[0]["address"], recs[1]["address"]]


def test_model_scan_stops_at_group_of_four():
    d = M.digits_of(REF["base"])
    v = M.valid_offsets(d, 4096)
    assert v[:5] == [204, 586, 1648, 2023, 3000]
    known = {M.h160_of_key(M.key_of(REF["known"]))}
    assert M.scan(d, 5, known) == (3000, 5, [(3000, 4, REF["known"], M.key_of(REF["known"]))])
    assert M.scan(d, 4, known) == (2024, 4, [])
    # the odometer's top-digit wrap
    w = M.digits_of("Szzzzzzzzzzzzzzzzzzzzp")
    assert [mk for _, mk in M.walk(w, 11)][9:11] == ["Szzzzzzzzzzzzzzzzzzzzz", "S111111111111111111111"]


def test_cli_argument_errors():
    r = run(["-m", "minikeys", "-f", "x", "-C", "SG64GZqySYwBm9KxE3wH8"])
    assert r.returncode == 1 and "[E] Invalid Minikey length 21 : SG64GZqySYwBm9KxE3wH8\n" in r.stderr
    r = run(["-m", "minikeys", "-f", "x", "-C", "SG64GZqySYwBm9KxE3wH80"])  # '0' is no base-58 character
    assert r.returncode == 1 and "[E] invalid character in minikey\n" in r.stderr
    r = run(["-m", "minikeys", "-f", "x", "-8", "abc"])
    assert r.returncode == 1 and "[E] The base58 alphabet must be 58 characters long.\n" in r.stderr
    r = run(["-m", "minikeys", "-f", "x", "-C", REF["base"], "-n", "0x400"])
    assert r.returncode == 1 and "n must be at least 2^20" in r.stderr
    # a permuted alphabet is echoed, and -C is read through it
    alpha = M.ALPHABET[::-1]
    r = run(["-8", alpha, "-m", "minikeys", "-f", "x", "-C", REF["base"]])
    assert f"[+] Base58 for Minikeys {alpha}\n" in r.stdout and "[+] Base Minikey : " + REF["base"] in r.stdout


def test_cli_header_matches_reference_and_needs_a_gpu():
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(os.path.join(DATA, "minikeys.txt"), td)
        r = run(REF["argv"] + ["-t", "1", "-s", "0"], cwd=td, env=NO_GPU)
    assert r.returncode == 1 and "no GPU found" in r.stderr
    want = header_lines(REF["stdout"])
    assert "[+] Mode minikeys" in want and "[+] Base Minikey : " + REF["base"] in want
    assert not any(l.startswith("[+] -- from") or l.startswith("[+] Range") for l in want)
    assert header_lines(r.stdout) == want


def test_keyhunt_amd_still_refuses_the_mode():
    r = subprocess.run([os.path.join(E.PKG, "bin", "keyhunt-amd"), "-m", "minikeys", "-f", "x", "-C", REF["base"]],
                       capture_output=True, text=True)
    assert r.returncode == 1 and ("Unsupported mode" in r.stderr or "invalid option" in r.stderr)


def test_null_context_is_rejected():
    L = keyhunt_amd.lib()
    n, nc, nv = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
    assert L.kh_minikeys_scan(None, bytes(21), 1, None, 0, ctypes.byref(n), ctypes.byref(nc), ctypes.byref(nv)) == -1
    assert L.kh_minikeys_valid(None, bytes(21), 4, None, 0, ctypes.byref(nc)) == -1
    assert L.kh_minikeys_set_alphabet(None, None) == -1 and L.kh_minikeys_set_window(None, 0, 0) == -1


# -- the dense construction and the 2^32 crossing (tests/test_gpu_minikeys_dense.py) -----------------------
# A many-to-one alphabet: digits 8..57 all spell 'A', so every candidate whose changed digits are >= 8
# spells the same string, and one valid string makes a whole run of candidates valid.
DENSE_ALPHA = M.ALPHABET[:8] + "A" * 50
DENSE_BASE = [16, 0, 3, 41, 52, 35, 57, 22, 38, 41, 37, 28, 38, 33, 46, 31, 15, 10, 0, 0, 0]  # raw digits
DENSE_KEY = "SA14AAAAAAAAAAAAAAAAAA"
FILTER_BLOCK = 58 * 256  # candidates of one k_mini_filter block: 256 rows of 58
EXAMPLE = "SG64GZqySYwBm9KxE3wH8R"
X32 = 1 << 32
_cache = {}


def dense_valid() -> list[int]:
    """The model's valid candidates of the first 2^18 from DENSE_BASE: computed once, never changed."""
    if "dense" not in _cache:
        _cache["dense"] = tuple(M.valid_offsets(DENSE_BASE, 1 << 18, DENSE_ALPHA))
    return list(_cache["dense"])


def around_x32() -> list[tuple[int, str]]:
    """(offset, minikey) of the example base's valid candidates in (2^32 - 2^15, 2^32 + 2^15], from the
    base shifted by 2^32 - 2^15."""
    if "x32" not in _cache:
        lo = X32 - (1 << 15)
        shifted = M.digits_from_value(M.value_of(M.digits_of(EXAMPLE)) + lo)
        _cache["x32"] = tuple((lo + o, mk) for o, mk in M.walk(shifted, 1 << 16) if M.is_valid(mk))
    return list(_cache["x32"])


def test_dense_construction_counts():
    """What the dense GPU tests rest on: blocks of the first launch that overflow the filter's 256-entry
    stage beside blocks that do not."""
    assert M.text_of(DENSE_BASE, DENSE_ALPHA) == "SA14AAAAAAAAAAAAAAA111" and M.is_valid(DENSE_KEY)
    v = dense_valid()
    assert len(v) == 157987 and sum(o <= 1 << 16 for o in v) == 29148
    # DENSE_BASE[20] == 0: block k of the window (0, 2^18] holds candidates [k * 14848, (k + 1) * 14848)
    per_block = [0] * 18
    for o in v:
        per_block[o // FILTER_BLOCK] += 1
    assert ((1 << 18) + FILTER_BLOCK) // FILTER_BLOCK == 18
    assert (min(per_block), max(per_block)) == (51, 11400) and sum(n > 256 for n in per_block) == 16
    assert (per_block[0], per_block[2]) == (51, 11050)  # one-block windows: from the base, and from base + 2 blocks
    # every candidate whose last three digits are all >= 8 spells the dense key
    assert all(M.candidate(DENSE_BASE, o, DENSE_ALPHA) == DENSE_KEY
               for o in (8 * 58 * 58 + 8 * 58 + 8, 57 * 58 * 58 + 57 * 58 + 57))
    strings = {M.candidate(DENSE_BASE, o, DENSE_ALPHA) for o in v if o <= 1 << 16}
    assert len(strings) == 4 and DENSE_KEY in strings
    # the dense scan: the 4096-th valid candidate, inside the first 2^16
    assert v[4095] == 32416 and M.scan(DENSE_BASE, 4096, set(), DENSE_ALPHA)[:2] == (32416, 4096)


def test_valid_candidates_around_2_to_32():
    got = around_x32()
    assert len(got) == 275 and [o for o, _ in got] == sorted(o for o, _ in got)
    below = [(o, mk) for o, mk in got if o <= X32]
    assert below[-1] == (4294966823, "SG64GZqySYwBm9KxLbU78Y") and got[len(below)] == (4294967552, "SG64GZqySYwBm9KxLbU7M7")
    assert all(M.candidate(M.digits_of(EXAMPLE), o) == mk for o, mk in (got[0], below[-1], got[len(below)], got[-1]))


def test_minikey_hit_layout():
    """kh_minikey_hit: ordinal is 64 bits (need_valid can be 2^32); the struct keeps its 72 bytes."""
    H = keyhunt_amd.KhMinikeyHit
    assert ctypes.sizeof(H) == 72
    assert (H.key.offset, H.offset.offset, H.ordinal.offset, H.ordinal.size) == (0, 32, 40, 8)
    assert (H.minikey.offset, H.minikey.size) == (48, 24)
