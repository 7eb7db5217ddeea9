"""--segwit's option handling in keyhunt-amd and minikeys-amd, without a GPU: the four refusals (each
exits 1 with its [E] line before a device is looked for) and the accepted form, which reads its targets
-- bech32 lines included -- and gets as far as needing a GPU."""
import os
import subprocess

import pytest

from keyhunt_amd import engine as E

NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
TARGETS = ["bc1qw508d6qejxtdg4y5r3zarvary0c5xw7kv8f3t4",
           "BC1Q8ZT37UUNPAKPG8VH0TZ06JNJ0JZ5JDDN7AYCTZ",
           "3JvL6Ymt8MVWiCNHC7oWU6nLeHNJKLZGLN",
           "36NvZTcMsMowbt78wPzJaHHWaNiyR73Y4g",
           "1BgGZ9tcN4rm9KBzDn7KprQz87SZ26SAMH",
           "bc1p0xlxvlhemja6c4dqv22uapctqupfhlxm9h8z3k2e72q4k9hcz7vqzk5jj0"[:42],
           "bc1qw508d6qejxtdg4y5r3zarvary0c5xw7kv8f3t5"]          # last character changed: bad checksum


@pytest.fixture(params=["keyhunt-amd", "minikeys-amd"])
def cli(request):
    path = os.path.join(E.PKG, "bin", request.param)
    if not os.path.exists(path):
        pytest.skip("CLI not built")
    return path


def _run(cli, tmp_path, *argv):
    f = tmp_path / "t.txt"
    f.write_text("".join(t + "\n" for t in TARGETS))
    return subprocess.run([cli, "-f", str(f), "-r", "1:100000", *argv], capture_output=True, text=True, cwd=tmp_path,
                          env=NO_GPU)


@pytest.mark.parametrize("argv, message", [
    (["-m", "rmd160"], "--segwit works with -m address only"),
    (["-m", "xpoint"], "--segwit works with -m address only"),
    (["-m", "bsgs"], "--segwit works with -m address only"),
    (["-m", "address", "-c", "eth"], "--segwit doesn't work with -c eth"),
    (["-m", "address", "-l", "uncompress"], "--segwit doesn't work with -l uncompress"),
    (["-m", "address", "-l", "compress", "-S"], "--segwit doesn't work with -S"),
])
def test_refusals(cli, tmp_path, argv, message):
    r = _run(cli, tmp_path, "--segwit", *argv)
    assert r.returncode == 1
    assert f"[E] {message}" in r.stderr
    # refused before the targets are read and before any device is looked for
    assert "no GPU found" not in r.stderr and "Allocating memory" not in r.stdout
    assert not list(tmp_path.glob("data_*.dat"))


@pytest.mark.parametrize("extra", [[], ["-e"], ["-R"], ["-I", "3"], ["-g", "2"]])
@pytest.mark.parametrize("search", ["compress", "both"])
def test_accepted_up_to_the_gpu(cli, tmp_path, search, extra):
    r = _run(cli, tmp_path, "-m", "address", "-l", search, "--segwit", "-t", "1", "-s", "0", "-q", *extra)
    assert r.returncode == 1 and "no GPU found" in r.stderr
    assert "segwit" not in r.stderr
    assert "[+] Segwit targets: 2 bech32, 2 P2SH-P2WPKH\n" in r.stdout
    assert "[+] Sorting data ... done! 5 values were loaded and sorted" in r.stdout
    omitted = [ln for ln in r.stderr.splitlines() if ln.startswith("[I] Ommiting invalid line")]
    assert omitted == [f"[I] Ommiting invalid line {TARGETS[5]}", f"[I] Ommiting invalid line {TARGETS[6]}"]


def test_without_the_option_the_reader_is_the_reference_one(cli, tmp_path):
    r = _run(cli, tmp_path, "-m", "address", "-l", "compress", "-t", "1", "-s", "0", "-q")
    assert r.returncode == 1 and "no GPU found" in r.stderr
    assert "Segwit" not in r.stdout
    assert "[+] Sorting data ... done! 3 values were loaded and sorted" in r.stdout
    omitted = [ln for ln in r.stderr.splitlines() if ln.startswith("[I] Ommiting invalid line")]
    assert omitted == [f"[I] Ommiting invalid line {TARGETS[i]}" for i in (0, 1, 5, 6)]
