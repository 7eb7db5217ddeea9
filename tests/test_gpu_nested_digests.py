"""kh_digests_nested: the nested P2SH-P2WPKH digests of a point's two compressed key hashes, as the
KH_MODE_P2SH walks compute them on the device (hash160_comp2, then the pair form hash160_nested2),
against the oracle's composition of hash160_comp, SHA-256 and RIPEMD-160."""
import random

import pytest

pytestmark = pytest.mark.gpu

P = 2**256 - 2**32 - 977
VECTOR_KEYS = [1, 0xc9bdb49cfbaedca21c4b1f3a7803c34636b1d7dc55a717132443fc3f4c5867e8]
VECTOR_NESTED = ["bcfeb728b584253d5f3f70bcb780e9ef218a68f4", "336caa13e08b96080a32b5d818d59b4ab3b36742"]


def _want(oracle, x):
    return tuple(oracle.ripemd160(oracle.sha256(b"\x00\x14" + oracle.hash160_comp(x, pfx))) for pfx in (2, 3))


def test_nested_digests_of_random_points_vectors_and_off_curve_points(engine, oracle):
    rng = random.Random(0x4E57ED)
    # any (x, y) is hashed: 4,096 random coordinate pairs (none on the curve, but for luck), the two
    # vector keys' points, and x values at the ends of the field with y arbitrary
    pts = [(rng.randrange(P), rng.randrange(P)) for _ in range(4096)]
    pts += [oracle.pubkey(k) for k in VECTOR_KEYS]
    pts += [(0, 0), (1, 0), (P - 1, 1), (1 << 255, 7), ((1 << 256) - 1 - 2**32 - 977, P - 1), (0x80 << 248, 0)]
    got = engine.digests_nested(pts)
    assert len(got) == len(pts)
    for (x, _), g in zip(pts, got):
        assert g == _want(oracle, x), hex(x)
    # the vector keys: the nested hash of the key's own prefix is the published one
    for k, (x, y), g, nested in zip(VECTOR_KEYS, pts[4096:4098], got[4096:4098], VECTOR_NESTED):
        assert g[y & 1].hex() == nested, hex(k)


def test_nested_digests_nest_what_kh_digests_reports(engine, oracle):
    """The inner digests are kh_digests' own 02 / 03 outputs."""
    pts = [oracle.pubkey(k) for k in (2, 3, 0xDEADBEEF, 1 << 200)]
    plain, nest = engine.digests(pts), engine.digests_nested(pts)
    for p, n in zip(plain, nest):
        assert n == tuple(oracle.ripemd160(oracle.sha256(b"\x00\x14" + h)) for h in p[:2])
