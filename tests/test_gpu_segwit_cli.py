"""keyhunt-amd -m address --segwit end to end: a target file of two bech32 lines (one upper case), two
3... lines, one 1... line and one bc1p... line, for keys in a 2^20-key range scanned as one chunk (the
smallest -n the CLI accepts).  With the option five keys are found, the P2SH hits print their 3...
address and nested hash, the plain compressed hits carry a fifth `bech32` line; without it the reader
and the hit text are the reference's (this half passes with or without the feature)."""
import os
import re
import subprocess

import pytest

from _segwit import BECH32M, base58check, encode
from conftest import REPO

pytestmark = pytest.mark.gpu

CLI = os.path.join(REPO, "keyhunt_amd", "bin", "keyhunt-amd")
START = 0x5A17C0DE00000000
OFFS = [0x00003, 0x2F0A1, 0x7FFFF, 0xC0FFE, 0xFFFFF]      # bech32, BECH32, 3..., 3..., 1...
BLOCK = re.compile(r"Private Key: ([0-9a-f]+)\npubkey: ([0-9a-f]+)\nAddress (\S+)\nrmd160 ([0-9a-f]+)\n"
                   r"(?:bech32 (\S+)\n)?")


@pytest.fixture(scope="module")
def case(oracle):
    keys = [START + o for o in OFFS]
    pts = [oracle.pubkey(k) for k in keys]
    h = [oracle.hash160_comp(x, 2 + (y & 1)) for x, y in pts]
    nest = [oracle.ripemd160(oracle.sha256(b"\x00\x14" + d)) for d in h]
    taproot = encode("bc", 1, h[0], BECH32M)
    assert len(taproot) == 42 and taproot.startswith("bc1p")
    lines = [encode("bc", 0, h[0]), encode("bc", 0, h[1]).upper(), base58check(5, nest[2]), base58check(5, nest[3]),
             base58check(0, h[4]), taproot]
    assert [ln[:4].lower() for ln in lines[:2]] == ["bc1q"] * 2 and [ln[0] for ln in lines[2:5]] == ["3", "3", "1"]
    pub = ["%02x%064x" % (2 + (y & 1), x) for x, y in pts]
    return keys, h, nest, lines, pub


def _run(tmp_path, lines, *extra):
    (tmp_path / "t.txt").write_text("".join(ln + "\n" for ln in lines))
    r = subprocess.run([CLI, "-m", "address", "-l", "compress", *extra, "-t", "1", "-s", "0", "-q", "-n", "0x100000",
                        "-f", "t.txt", "-r", "%x:%x" % (START, START + (1 << 20))], cwd=tmp_path, capture_output=True,
                       text=True, timeout=120)
    kf = tmp_path / "KEYFOUNDKEYFOUND.txt"
    return r, (kf.read_text() if kf.exists() else "")


def test_segwit_run_finds_all_five(case, tmp_path):
    keys, h, nest, lines, pub = case
    r, found = _run(tmp_path, lines, "--segwit")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "[+] Segwit targets: 2 bech32, 2 P2SH-P2WPKH\n" in r.stdout
    assert [ln for ln in r.stderr.splitlines() if "Ommiting" in ln] == [f"[I] Ommiting invalid line {lines[5]}"]
    want = []
    for i, k in enumerate(keys):
        if i in (2, 3):   # the P2SH-P2WPKH hits: their 3... address and the nested hash, no fifth line
            want.append(("%x" % k, pub[i], lines[i], nest[i].hex(), ""))
        else:             # plain compressed hits: the reference's four lines and the key's bech32 address
            want.append(("%x" % k, pub[i], base58check(0, h[i]), h[i].hex(), encode("bc", 0, h[i])))
    assert BLOCK.findall(found) == want
    assert [m for m in BLOCK.findall(r.stdout)] == want
    assert r.stdout.count("\nHit! Private Key: ") == 5
    assert found.count("Private Key: ") == 5


def test_without_the_option_only_the_p2pkh_key_in_the_reference_form(case, tmp_path):
    keys, h, nest, lines, pub = case
    r, found = _run(tmp_path, lines)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Segwit" not in r.stdout
    assert [ln for ln in r.stderr.splitlines() if "Ommiting" in ln] == \
        [f"[I] Ommiting invalid line {lines[i]}" for i in (0, 1, 5)]
    text = "Private Key: %x\npubkey: %s\nAddress %s\nrmd160 %s\n" % (keys[4], pub[4], lines[4], h[4].hex())
    assert found == text
    assert r.stdout.count("Hit! Private Key: ") == 1 and ("\nHit! " + text) in r.stdout and "bech32" not in r.stdout
