"""-m kangaroo's option handling in keyhunt-amd and minikeys-amd, without a GPU: every refusal exits 1 with its
[E] line before a device is looked for, the accepted form reads its targets and gets as far as needing a GPU,
-h names the mode, and keyhunt-amd still refuses -m minikeys."""
import os
import shutil
import subprocess

import pytest

from conftest import DATA
from keyhunt_amd import engine as E

NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
RANGE = "7cce5e0000000000:7cce5effffffffff"


@pytest.fixture(params=["keyhunt-amd", "minikeys-amd"])
def cli(request):
    return os.path.join(E.PKG, "bin", request.param)


def _run(cli, tmp_path, *argv, rng=("-r", RANGE)):
    shutil.copy(os.path.join(DATA, "63.pub"), tmp_path)
    return subprocess.run([cli, "-m", "kangaroo", "-f", "63.pub", *rng, *argv], capture_output=True, text=True,
                          cwd=tmp_path, env=NO_GPU, timeout=60)


@pytest.mark.parametrize("argv, message", [
    (["-e"], "-e (endomorphism) doesn't work with -m kangaroo"),
    (["-I", "2"], "-I (stride) doesn't work with -m kangaroo"),
    (["-B", "both"], "-B (BSGS schedule) doesn't work with -m kangaroo"),
    (["-k", "4"], "-k (BSGS k factor) doesn't work with -m kangaroo"),
    (["-n", "0x100000"], "-n doesn't work with -m kangaroo"),
    (["-S"], "-S doesn't work with -m kangaroo"),
    (["-c", "btc"], "-c doesn't work with -m kangaroo"),
    (["-l", "compress"], "-l doesn't work with -m kangaroo"),
    (["--segwit"], "--segwit doesn't work with -m kangaroo"),
    (["--taproot"], "--taproot doesn't work with -m kangaroo"),
    (["--mapped"], "the mapped bloom options don't work with -m kangaroo"),
    (["--create-mapped"], "the mapped bloom options don't work with -m kangaroo"),
    (["--bloom-file", "b.dat"], "the mapped bloom options don't work with -m kangaroo"),
    (["--ptable", "p.tbl"], "the ptable options don't work with -m kangaroo"),
    (["--ptable-cache"], "the ptable options don't work with -m kangaroo"),
    (["-g", "2"], "-m kangaroo runs on one GPU"),
    (["--dp", "33"], "--dp takes 0 .. 32"),
    (["--herd", "16777217"], "--herd takes at most 16777216"),
])
def test_refusals(cli, tmp_path, argv, message):
    r = _run(cli, tmp_path, *argv)
    assert r.returncode == 1
    assert f"[E] {message}" in r.stderr
    assert len([ln for ln in r.stderr.splitlines() if ln.startswith("[E]")]) == 1
    assert "no GPU found" not in r.stderr and "Opening file" not in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["63.pub"]


@pytest.mark.parametrize("rng, message", [
    ((), "-m kangaroo needs a bounded range: -r START:END or -b BITS"),
    (("-r", "1000:10fff"), "-m kangaroo needs a range at least 2^16 and less than 2^192 keys wide"),
    (("-r", "1:1000000000000000000000000000000000000000000000001"),
     "-m kangaroo needs a range at least 2^16 and less than 2^192 keys wide"),
    (("-b", "194"), "-m kangaroo needs a range at least 2^16 and less than 2^192 keys wide"),
    (("-b", "17"), "-m kangaroo needs a range at least 2^16 and less than 2^192 keys wide"),
])
def test_range_refusals(cli, tmp_path, rng, message):
    r = _run(cli, tmp_path, rng=rng)
    assert r.returncode == 1
    assert f"[E] {message}" in r.stderr
    assert "no GPU found" not in r.stderr and "Opening file" not in r.stdout


@pytest.mark.parametrize("rng", [("-r", RANGE), ("-b", "63"), ("-b", "18"), ("-b", "193"), ("-r", "1000:11000")])
def test_accepted_form_gets_as_far_as_the_gpu(cli, tmp_path, rng):
    r = _run(cli, tmp_path, "--dp", "4", "--herd", "4096", "--seed", "1", "-q", rng=rng)
    assert r.returncode == 1
    assert "[+] Mode kangaroo\n" in r.stdout
    assert "[+] Opening file 63.pub\n[+] Added 1 points from file\n" in r.stdout
    assert r.stderr.strip().splitlines()[-1] == "[E] no GPU found"


def test_target_file_messages_are_the_bsgs_reader_s(cli, tmp_path):
    (tmp_path / "empty.txt").write_text("nothing\n")
    r = subprocess.run([cli, "-m", "kangaroo", "-f", "empty.txt", "-b", "63"], capture_output=True, text=True, cwd=tmp_path,
                       env=NO_GPU, timeout=60)
    b = subprocess.run([cli, "-m", "bsgs", "-f", "empty.txt", "-b", "63"], capture_output=True, text=True, cwd=tmp_path,
                       env=NO_GPU, timeout=60)
    assert r.returncode == b.returncode == 1
    assert "[E] There is no valid data in the file" in r.stderr and "[E] There is no valid data in the file" in b.stderr
    r = subprocess.run([cli, "-m", "kangaroo", "-f", "missing.txt", "-b", "63"], capture_output=True, text=True, cwd=tmp_path,
                       env=NO_GPU, timeout=60)
    assert r.returncode == 1 and "[E] Can't open file missing.txt" in r.stderr


def test_help_names_the_mode(cli):
    r = subprocess.run([cli, "-h"], capture_output=True, text=True, env=NO_GPU, timeout=60)
    assert r.returncode == 0
    assert "-m kangaroo -f FILE (-r START:END | -b BITS) [--dp BITS] [--herd N] [--seed U64] [-q]" in r.stdout


def test_keyhunt_amd_still_refuses_minikeys(tmp_path):
    r = subprocess.run([os.path.join(E.PKG, "bin", "keyhunt-amd"), "-m", "minikeys"], capture_output=True, text=True,
                       cwd=tmp_path, env=NO_GPU, timeout=60)
    assert r.returncode == 1
    assert "[E] Unsupported mode minikeys (engine covers address, rmd160, xpoint, bsgs, vanity)" in r.stderr
    r = subprocess.run([os.path.join(E.PKG, "bin", "keyhunt-amd"), "-m", "lambda"], capture_output=True, text=True,
                       cwd=tmp_path, env=NO_GPU, timeout=60)
    assert r.returncode == 1 and "[E] Unsupported mode lambda" in r.stderr
