"""The value of the reference's AddDirect where its two points share an x (dx = 0), pinned three ways.

Secp256K1::AddDirect (SECP256K1.cpp:455-478) has no special cases: ModInv of 0 leaves 0, so s = 0,
rx = -p1.x - p2.x and ry = s*(p2.x - rx) - p2.y = -p2.y -- the y of the SECOND operand.  bsgs_secondcheck
calls it as AddDirect(Q, -base_key*G) (keyhunt.cpp:5171), so a base key equal to the target's key gives
S = (-2 Q.x, +Q.y) and all 32 points S + AMP2[i] follow from that value.  tests/golden/ref_vectors.json
"add_direct_dx0" holds what the reference's own code returns (oracle/ref_golden.cpp); the oracle's
restatement (kh_oracle.c ge_add_direct) and the Python one below must equal it."""
import json
import os

from conftest import GOLDEN, REPO

P = 2**256 - 2**32 - 977
VEC = json.load(open(os.path.join(GOLDEN, "ref_vectors.json")))["add_direct_dx0"]


def add_direct(p1, p2):
    """SECP256K1.cpp:455-478, line by line (463-466, 468-471, 473-475)."""
    dy, dx = (p2[1] - p1[1]) % P, (p2[0] - p1[0]) % P
    s = dy * pow(dx, P - 2, P) % P                 # ModInv: 0 stays 0
    rx = (s * s - p1[0] - p2[0]) % P
    ry = ((p2[0] - rx) * s - p2[1]) % P
    return rx, ry


def _cases():
    for v in VEC:
        pt = (int(v["x"], 16), int(v["y"], 16))
        ng = (pt[0], P - pt[1])
        yield pt, pt, tuple(int(c, 16) for c in v["pp"])
        yield pt, ng, tuple(int(c, 16) for c in v["pn"])
        yield pt, ng, tuple(int(c, 16) for c in v["qn"])


def test_reference_values_have_the_second_operands_y():
    assert len(VEC) == 3
    for p1, p2, want in _cases():
        assert want == ((-p1[0] - p2[0]) % P, (-p2[1]) % P)


def test_python_restatement_equals_reference():
    for p1, p2, want in _cases():
        assert add_direct(p1, p2) == want


def test_oracle_add_direct_equals_reference(oracle):
    for v in VEC:
        assert oracle.pubkey(int(v["k"], 16)) == (int(v["x"], 16), int(v["y"], 16))
    for p1, p2, want in _cases():
        assert oracle.add_direct(p1, p2) == want


def test_restatements_agree_with_the_ordinary_sum_where_dx_is_not_zero(oracle):
    a, b = oracle.pubkey(0x1234567), oracle.pubkey(0x7654321FFF)
    assert add_direct(a, b) == oracle.add_direct(a, b) == oracle.point_add(a, b) == oracle.pubkey(0x1234567 + 0x7654321FFF)


def test_engine_ge_add_is_the_literal_add_direct(tmp_path):
    """kh_math.h's ge_add, which k_setup's and k_refine's h == 0 branches and the host twins call for
    exactly this value, compiled for the host: equal to the reference on the dx = 0 cases and to the
    ordinary sum elsewhere."""
    import shutil
    import subprocess
    import pytest
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = tmp_path / "a.cpp"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "kh_math.h"\nusing namespace kh;\n'
                   'static void rd(fe &r, const char *h) { uint8_t b[32]; for (int i = 0; i < 32; i++) {\n'
                   '  unsigned v; sscanf(h + 2 * i, "%2x", &v); b[i] = (uint8_t)v; } fe_from_be(r, b); }\n'
                   'static void pr(const fe &a) { uint8_t b[32]; fe_to_be(b, a); for (int i = 0; i < 32; i++)\n'
                   '  printf("%02x", b[i]); }\n'
                   'int main(int, char **v) { ge p, q, r; rd(p.x, v[1]); rd(p.y, v[2]); rd(q.x, v[3]); rd(q.y, v[4]);\n'
                   '  ge_add(r, p, q); pr(r.x); printf(" "); pr(r.y); printf("\\n");\n'
                   '  ge_add(q, p, q); pr(q.x); printf(" "); pr(q.y); printf("\\n"); return 0; }\n')   # aliased, as k_setup calls it
    exe = tmp_path / "a"
    csrc = os.path.join(REPO, "keyhunt_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", csrc, "-o", str(exe), str(src)], check=True)
    a, b = (int(VEC[1]["x"], 16), int(VEC[1]["y"], 16)), (int(VEC[2]["x"], 16), int(VEC[2]["y"], 16))
    for p1, p2, want in list(_cases()) + [(a, b, add_direct(a, b))]:
        out = subprocess.run([str(exe)] + ["%064x" % c for c in (*p1, *p2)], capture_output=True, text=True,
                             check=True).stdout.split()
        assert (int(out[0], 16), int(out[1], 16)) == want
        assert (int(out[2], 16), int(out[3], 16)) == want
