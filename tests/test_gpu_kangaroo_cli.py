"""keyhunt-amd -m kangaroo end to end: puzzle 63's public key in a 2^40 range, its hit lines and
KEYFOUNDKEYFOUND.txt record byte for byte what -m bsgs writes for the same key and file, and a file of two
targets solved in file order."""
import os
import re
import shutil
import subprocess

import pytest

import _kangaroo as K
from conftest import DATA, REPO

pytestmark = pytest.mark.gpu
CLI = os.path.join(REPO, "keyhunt_amd", "bin", "keyhunt-amd")
RANGE = "7cce5e0000000000:7cce5effffffffff"
FOUND = re.compile(r"\[\+\] Thread Key found privkey [0-9a-f]+ *\n?\[\+\] Publickey [0-9a-f]+\n")


def _run(cwd, *argv):
    r = subprocess.run([CLI, *argv, "-q", "-s", "0"], cwd=cwd, capture_output=True, text=True, timeout=300)
    kf = os.path.join(cwd, "KEYFOUNDKEYFOUND.txt")
    return r, (open(kf).read() if os.path.exists(kf) else "")


def test_puzzle_63_prints_what_bsgs_prints(tmp_path):
    for d in ("k", "b"):
        os.mkdir(tmp_path / d)
        shutil.copy(os.path.join(DATA, "63.pub"), tmp_path / d)
    k, k_found = _run(tmp_path / "k", "-m", "kangaroo", "-f", "63.pub", "-r", RANGE, "--seed", "1")
    assert k.returncode == 0, k.stdout[-2000:] + k.stderr[-2000:]
    b, b_found = _run(tmp_path / "b", "-m", "bsgs", "-f", "63.pub", "-r", RANGE, "-n", "0x1000000", "-k", "4", "-t", "1")
    assert "All points were found" in b.stdout, b.stdout[-2000:] + b.stderr[-2000:]
    assert k_found == b_found == ("Key found privkey 7cce5efdaccf6808\nPublickey "
                                  "0365ec2994b8cc0a20d40dd69edfe55ca32a54bcbbaa6b0ddcff36049301a54579\n")
    assert FOUND.findall(k.stdout) == FOUND.findall(b.stdout) and len(FOUND.findall(k.stdout)) == 1
    assert k.stdout.endswith("\nEnd\n")


def test_two_targets_are_solved_in_file_order(tmp_path):
    a = 0x4000000000
    keys = [a + 0x2F0F0F0F0F, a + 0x0000012345]
    lines = []
    for i, key in enumerate(keys):
        x, y = K.pub_of(key)
        lines.append("%02x%064x" % (2 + (y & 1), x) if i == 0 else "04%064x%064x" % (x, y))
    (tmp_path / "two.txt").write_text("".join(ln + "\n" for ln in lines))
    r, found = _run(tmp_path, "-m", "kangaroo", "-f", "two.txt", "-b", "39", "--seed", "7", "--herd", "4096", "--dp", "3")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert found == "".join("Key found privkey %x\nPublickey %s\n" % (key, ln) for key, ln in zip(keys, lines))
    assert [m for m in re.findall(r"found privkey ([0-9a-f]+)", r.stdout)] == ["%x" % key for key in keys]
    assert "[+] Kangaroo target 1: herd 4096, dp 3\n" in r.stdout and "[+] Kangaroo target 2: herd 4096, dp 3\n" in r.stdout
