"""--taproot without a GPU: the Python model of BIP-340/341 (tests/_taproot.py) against the published
vectors; the host's tweak (csrc/kh_host.h taproot_output_x) and its bech32m P2TR codec
(host/kh_host_util.h), each compiled into a stand-alone program under the address and undefined-behaviour
sanitizers and compared with the model; the CLI's option checks; the null-context refusals of the ABI."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import pytest

import keyhunt_amd
from keyhunt_amd import engine as E
import _taproot as T
from _segwit import BECH32M, encode

INC = os.path.join(os.path.dirname(E.PKG), "include")
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
GOOD = [v[2] for v in T.VECTORS]


def _build(d, name, text, *flags):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src, exe = d / (name + ".cpp"), d / name
    src.write_text(text)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *flags,
                    "-I", os.path.join(E.PKG, "host"), "-I", os.path.join(E.PKG, "csrc"), "-I", INC, "-o", str(exe),
                    str(src)], check=True)

    def run(*args):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True, check=True)
        assert r.stderr == ""
        return r.stdout.split()
    return run


# ---- the model --------------------------------------------------------------------------------------
def test_model_reproduces_the_published_vectors():
    for internal, output, addr in T.VECTORS:
        qx = T.output_x(int(internal, 16))
        assert "%064x" % qx == output
        assert T.address_of_x(qx) == addr
    assert hashlib.sha256(b"TapTweak").hexdigest() == "e80fe1639c9ca050e3af1b39c143c63e429cbceb15d940fbb5c5a1f4af57c5e9"


def test_model_addresses_of_small_keys_and_the_tweaked_secret():
    for k, addr in T.SMALL_KEYS.items():
        qx, a, d, pt = T.key_output(k)   # key_output asserts (d + t) G has x = Q.x
        assert a == addr
        assert d == (k if pt[1] % 2 == 0 else T.N - k)
    assert T.mul_g(0xDEADBEEF12345) == T.mul(0xDEADBEEF12345)


# ---- the host tweak ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tweak_prog(tmp_path_factory):
    if not os.path.isdir(os.path.join(ROCM_INC, "hip")):
        pytest.skip("no HIP headers")
    # arguments: pairs x y (hex) -> the output key as hex, or "-" where taproot_output_x returns false
    return _build(tmp_path_factory.mktemp("taptweak"), "t",
                  '#include <stdio.h>\n#include "kh_host.h"\n#include "kh_host_util.h"\n'
                  'int main(int n, char **v) {\n'
                  '  for (int i = 1; i + 1 < n; i += 2) { uint8_t bx[32], by[32], q[32]; kh::fe x, y;\n'
                  '    if (!khh::hex2bin(v[i], bx, 32) || !khh::hex2bin(v[i + 1], by, 32)) return 2;\n'
                  '    kh::fe_from_be(x, bx); kh::fe_from_be(y, by);\n'
                  '    if (!kh_host::taproot_output_x(x, y, q)) { printf("-\\n"); continue; }\n'
                  '    printf("%s\\n", khh::hex(q, 32).c_str()); }\n'
                  '  return 0; }\n', "-D__HIP_PLATFORM_AMD__", "-I", ROCM_INC)


def test_host_tweak_matches_the_model(tweak_prog):
    pts = []
    for internal, _, _ in T.VECTORS:
        x, y = T.lift_x(int(internal, 16))
        pts += [(x, y), (x, T.P - y)]
    # 32 further points: 16 keys, each with both signs of Y (so both parities, the same output key)
    for k in [1, 2, 3, 7, 0xFFFF, 2**64 + 5, 2**128 - 1, 2**200 + 12345, T.N - 1, T.N - 2, T.N // 2, T.N // 3,
              0x123456789ABCDEF0123456789ABCDEF, 0xC0FFEE, 2**255 - 19, 0x5A17C0DE00000003]:
        x, y = T.mul_g(k)
        pts += [(x, y), (x, T.P - y)]
    assert len(pts) == 36 and {y & 1 for _, y in pts} == {0, 1}
    args = []
    for x, y in pts:
        args += ["%064x" % x, "%064x" % y]
    want = ["%064x" % T.output_x(x) for x, _ in pts]
    assert tweak_prog(*args) == want
    assert want[0] == T.VECTORS[0][1] and want[1] == T.VECTORS[0][1] and want[2] == T.VECTORS[1][1]


# ---- the bech32m decoder ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec(tmp_path_factory):
    # each argument: decoded program as hex and its re-encoding, or "-" when the decoder refuses it
    return _build(tmp_path_factory.mktemp("bech32m"), "b",
                  '#include "kh_host_util.h"\nint main(int n, char **v) {\n'
                  '  for (int i = 1; i < n; i++) { uint8_t p[32];\n'
                  '    if (!khh::bech32m_p2tr_decode(v[i], p)) { printf("-\\n"); continue; }\n'
                  '    printf("%s %s\\n", khh::hex(p, 32).c_str(), khh::bech32m_p2tr_encode(p).c_str()); }\n'
                  '  return 0; }\n')


def test_decoder_accepts_the_vectors_and_the_small_keys(codec):
    for _, output, addr in T.VECTORS:
        assert codec(addr) == [output, addr]
        assert codec(addr.upper()) == [output, addr]
    for k, addr in T.SMALL_KEYS.items():
        assert codec(addr) == ["%064x" % T.key_output(k)[0], addr]
    edge = [bytes(32), bytes([0xff] * 32), bytes(range(32)), bytes([0x80] + [0] * 30 + [0x01])]
    for p in edge:
        a = encode("bc", 1, p, BECH32M)
        assert len(a) == 62 and codec(a) == [p.hex(), a]


def test_decoder_refusals(codec):
    prog = bytes.fromhex(T.VECTORS[0][1])
    good = GOOD[0]
    plain = encode("bc", 1, prog)                    # bc1p... under the bech32 constant
    v0 = encode("bc", 0, prog, BECH32M)              # version 0 under the bech32m constant (62 characters)
    v2 = encode("bc", 2, prog, BECH32M)              # another version
    tb = encode("tb", 1, prog, BECH32M)              # testnet
    short = encode("bc", 1, prog[:20], BECH32M)      # 42 characters
    long_ = good + "q"                               # 63 characters
    mixed = good[:10] + good[10:].upper()
    assert [len(s) for s in (plain, v0, v2, tb, short, long_)] == [62, 62, 62, 62, 42, 63]
    assert plain.startswith("bc1p") and tb.startswith("tb1p")
    bad = [plain, v0, v2, tb, short, long_, mixed, good[:61], "", "bc1p" + "b" * 58]
    assert codec(*bad) == ["-"] * len(bad)
    # every single-character flip of one good address (the checksum finds any one substitution)
    flips = [good[:i] + ("q" if good[i] != "q" else "p") + good[i + 1:] for i in range(62)]
    assert codec(*flips) == ["-"] * 62


# ---- the CLI's option checks --------------------------------------------------------------------------
TARGETS = ["1BgGZ9tcN4rm9KBzDn7KprQz87SZ26SAMH", GOOD[0], GOOD[1].upper(), GOOD[0][:61] + "q",
           "bc1qw508d6qejxtdg4y5r3zarvary0c5xw7kv8f3t4"]


@pytest.fixture(params=["keyhunt-amd", "minikeys-amd"])
def cli(request):
    path = os.path.join(E.PKG, "bin", request.param)
    if not os.path.exists(path):
        pytest.skip("CLI not built")
    return path


def _run(cli, tmp_path, *argv, targets=TARGETS):
    f = tmp_path / "t.txt"
    f.write_text("".join(t + "\n" for t in targets))
    return subprocess.run([cli, "-f", str(f), "-r", "1:100000", *argv], capture_output=True, text=True, cwd=tmp_path,
                          env=NO_GPU)


@pytest.mark.parametrize("argv, message", [
    (["-m", "rmd160"], "--taproot works with -m address only"),
    (["-m", "xpoint"], "--taproot works with -m address only"),
    (["-m", "bsgs"], "--taproot works with -m address only"),
    (["-m", "address", "-c", "eth"], "--taproot doesn't work with -c eth"),
    (["-m", "address", "-e"], "--taproot doesn't work with -e"),
    (["-m", "address", "-S"], "--taproot doesn't work with -S"),
])
def test_cli_refusals(cli, tmp_path, argv, message):
    r = _run(cli, tmp_path, "--taproot", *argv)
    assert r.returncode == 1
    assert [ln for ln in r.stderr.splitlines() if "--taproot" in ln] == \
        [ln for ln in r.stderr.splitlines() if ln.startswith(f"[E] {message}")] != []   # its own message, once
    assert "no GPU found" not in r.stderr and "Allocating memory" not in r.stdout
    assert not list(tmp_path.glob("data_*.dat"))


@pytest.mark.parametrize("extra", [[], ["--segwit"], ["-l", "compress"], ["-R"], ["-I", "3"], ["-g", "2"]])
def test_cli_accepted_up_to_the_gpu(cli, tmp_path, extra):
    r = _run(cli, tmp_path, "-m", "address", "--taproot", "-t", "1", "-s", "0", "-q", *extra)
    assert r.returncode == 1 and "no GPU found" in r.stderr
    assert "taproot" not in r.stderr
    assert "[+] Taproot targets: 2\n" in r.stdout
    seg = "--segwit" in extra
    assert f"[+] Sorting data ... done! {2 if seg else 1} values were loaded and sorted" in r.stdout
    omitted = [ln for ln in r.stderr.splitlines() if ln.startswith("[I] Ommiting invalid line")]
    assert omitted == [f"[I] Ommiting invalid line {TARGETS[i]}" for i in ((3,) if seg else (3, 4))]


def test_cli_file_of_taproot_lines_alone_is_valid(cli, tmp_path):
    r = _run(cli, tmp_path, "-m", "address", "--taproot", "-t", "1", "-s", "0", "-q", targets=GOOD)
    assert r.returncode == 1 and "no GPU found" in r.stderr
    assert "[+] Taproot targets: 2\n" in r.stdout and "Ommiting" not in r.stderr


def test_cli_without_the_option_omits_taproot_lines(cli, tmp_path):
    for extra in ([], ["--segwit", "-l", "compress"]):
        r = _run(cli, tmp_path, "-m", "address", "-t", "1", "-s", "0", "-q", *extra)
        assert r.returncode == 1 and "no GPU found" in r.stderr
        assert "Taproot" not in r.stdout
        omitted = [ln for ln in r.stderr.splitlines() if ln.startswith("[I] Ommiting invalid line")]
        keep = (1, 2, 3) if extra else (1, 2, 3, 4)
        assert omitted == [f"[I] Ommiting invalid line {TARGETS[i]}" for i in keep]


def test_help_names_the_key_path_limit(cli):
    r = subprocess.run([cli, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--taproot" in r.stdout and "key-path-only" in r.stdout


# ---- the ABI ------------------------------------------------------------------------------------------
def test_null_context_is_rejected_by_the_taproot_calls():
    L = keyhunt_amd.lib()
    n = ctypes.c_uint32()
    hits = (E.KhHit * 1)()
    out = ctypes.create_string_buffer(32)
    assert L.kh_taproot_set_targets(None, b"\0" * 32, 1) == E.KH_E_ARG
    assert L.kh_taproot_scan(None, E.be32(1), None, 1024, hits, 1, ctypes.byref(n)) == E.KH_E_ARG
    assert L.kh_taproot_set_window(None, 1024) == E.KH_E_ARG
    assert L.kh_taproot_outputs(None, b"\0" * 64, 1, out) == E.KH_E_ARG
    assert L.kh_taproot_stats(None, None, None) == E.KH_E_ARG
    assert {"kh_taproot_set_targets", "kh_taproot_scan", "kh_taproot_set_window", "kh_taproot_outputs"} <= \
        set(keyhunt_amd.header_symbols())
