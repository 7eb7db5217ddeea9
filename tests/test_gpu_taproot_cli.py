"""keyhunt-amd -m address --taproot end to end, over a 2^20-key range scanned as one chunk (the smallest -n
the CLI accepts): with --segwit a file of a 1..., a bc1q..., a 3... and two bc1p... lines whose internal keys
have opposite Y parity; --taproot alone over a file of bc1p... lines only; and two contexts on one device."""
import os
import re
import subprocess

import pytest

import _taproot as T
from _segwit import base58check, encode
from conftest import REPO

pytestmark = pytest.mark.gpu

CLI = os.path.join(REPO, "keyhunt_amd", "bin", "keyhunt-amd")
START = 0x7A9207AB00000000
PLAIN = re.compile(r"Private Key: ([0-9a-f]+)\npubkey: ([0-9a-f]+)\nAddress (\S+)\nrmd160 ([0-9a-f]+)\n(?:bech32 (\S+)\n)?")
TAP = re.compile(r"Private Key: ([0-9a-f]+)\npubkey: ([0-9a-f]+)\nAddress (\S+)\ntaproot output key ([0-9a-f]{64})\n")


@pytest.fixture(scope="module")
def taps():
    """two keys of the range whose points have an even and an odd Y, and what their hits must print:
    (BIP-340 key, 02 || X, bc1p... address, output key)"""
    found = {}
    k = START + 0x1D00D
    while len(found) < 2:
        qx, addr, d, pt = T.key_output(k)
        found.setdefault(pt[1] & 1, ("%x" % d, "02%064x" % pt[0], addr, "%064x" % qx))
        k += 0x10101
    assert k < START + (1 << 20)
    span = range(START, START + (1 << 20))
    assert int(found[0][0], 16) in span and T.N - int(found[1][0], 16) in span     # the key kept, and negated
    return [found[0], found[1]]


def _run(tmp_path, lines, *extra, chunks=1):
    (tmp_path / "t.txt").write_text("".join(ln + "\n" for ln in lines))
    r = subprocess.run([CLI, "-m", "address", *extra, "-t", "1", "-s", "0", "-q", "-n", "0x100000", "-f", "t.txt", "-r",
                        "%x:%x" % (START, START + (chunks << 20))], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    kf = tmp_path / "KEYFOUNDKEYFOUND.txt"
    return r, (kf.read_text() if kf.exists() else "")


def test_segwit_and_taproot_in_one_run(taps, oracle, tmp_path):
    keys = [START + o for o in (0x00011, 0x80000, 0xFFFFE)]            # 1..., bc1q..., 3...
    pts = [oracle.pubkey(k) for k in keys]
    h = [oracle.hash160_comp(x, 2 + (y & 1)) for x, y in pts]
    nest = oracle.ripemd160(oracle.sha256(b"\x00\x14" + h[2]))
    pub = ["%02x%064x" % (2 + (y & 1), x) for x, y in pts]
    lines = [base58check(0, h[0]), encode("bc", 0, h[1]), base58check(5, nest), taps[0][2], taps[1][2].upper()]
    r, found = _run(tmp_path, lines, "-l", "compress", "--segwit", "--taproot")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "[+] Segwit targets: 1 bech32, 1 P2SH-P2WPKH\n" in r.stdout and "[+] Taproot targets: 2\n" in r.stdout
    assert "Ommiting" not in r.stderr
    want_plain = [("%x" % keys[0], pub[0], lines[0], h[0].hex(), encode("bc", 0, h[0])),
                  ("%x" % keys[1], pub[1], base58check(0, h[1]), h[1].hex(), lines[1]),
                  ("%x" % keys[2], pub[2], lines[2], nest.hex(), "")]
    want_tap = sorted(taps, key=lambda t: min(int(t[0], 16), T.N - int(t[0], 16)))      # offset order
    for text in (found, r.stdout):
        assert PLAIN.findall(text) == want_plain
        assert TAP.findall(text) == want_tap
    assert r.stdout.count("\nHit! Private Key: ") == 5 and found.count("Private Key: ") == 5
    # a chunk's kh_scan hits are written before its taproot hits
    assert found.index("rmd160 " + nest.hex()) < found.index("taproot output key")


def test_taproot_alone_over_a_file_of_bc1p_lines(taps, tmp_path):
    r, found = _run(tmp_path, [taps[1][2], taps[0][2]], "--taproot")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "[+] Taproot targets: 2\n" in r.stdout and "Segwit" not in r.stdout and "Ommiting" not in r.stderr
    want = sorted(taps, key=lambda t: min(int(t[0], 16), T.N - int(t[0], 16)))
    assert TAP.findall(found) == want and TAP.findall(r.stdout) == want
    assert found.count("Private Key: ") == 2 and "rmd160" not in found


def test_two_contexts_split_the_chunks(taps, tmp_path):
    """-g 2 on one device over four chunks: each context holds the programs and both hits are found once."""
    r, found = _run(tmp_path, [taps[0][2], taps[1][2]], "--taproot", "-g", "2", chunks=4)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "(2 contexts)" in r.stdout
    assert sorted(TAP.findall(found)) == sorted(taps)
    assert found.count("Private Key: ") == 2
