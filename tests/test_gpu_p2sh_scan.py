"""kh_scan with KH_MODE_P2SH: every compressed digest is probed as without the flag, then nested
(hash160(00 14 || h), the P2SH-P2WPKH script hash) and probed again against the same rows.

The reference has no such mode.  The yardstick is the engine's own plain path, which other tests pin to
the reference: a scan for rows r_i without the flag and a scan for rows nested(r_i) with it must report
the same keys at the same offsets in the same order, the kinds differing by KH_KIND_P2SH alone.  The
nested rows themselves come from the oracle's SHA-256 and RIPEMD-160.

Two chunk shapes -- 2^16 keys from 2^67 + c (sixteen 4096-point groups under -l compress) and 5 * 1024
keys from 2^66 + c (1024-point groups) -- each with the default geometry and with 512 lanes, against the
blocked target filter and against the reference-layout bloom.  64 keys are planted per chunk at seeded
offsets that include the first and the last key."""
import random

import pytest

pytestmark = pytest.mark.gpu

P = 2**256 - 2**32 - 977
BETA = 0x7ae96a2b657c07106e64479eac3434e99cf0497512f58995c1396c28719501ee
MODE_ADDRESS, MODE_XPOINT, MODE_ETH, ENDO, P2SH = 0, 1, 2, 0x10, 0x20
COMPRESS, UNCOMPRESS, BOTH = 0, 1, 2
KIND_P2SH = 0x80
KH_E_ARG = -1
SHAPES = {"big": ((1 << 67) + 0x2B5A7C91D3E4F, 1 << 16), "small": ((1 << 66) + 0x19C8E7F6A5B4D, 5 * 1024)}
N_PLANT = 64


def nested(oracle, h):
    return oracle.ripemd160(oracle.sha256(b"\x00\x14" + h))


@pytest.fixture(scope="module")
def planted(oracle):
    """Per shape: (start, n_keys, [(key, offset, x, y)]) by ascending offset, computed once."""
    out = {}
    for name, (start, n) in SHAPES.items():
        rng = random.Random(0x5E6 + n)
        offs = sorted({0, n - 1} | set(rng.sample(range(1, n - 1), N_PLANT - 2)))
        pts = [(start + o, o) + oracle.pubkey(start + o) for o in offs]
        assert len(pts) == N_PLANT
        assert {y & 1 for _, _, _, y in pts} == {0, 1}          # both 02 and 03 occur
        out[name] = (start, n, pts)
    return out


def plain_row(oracle, x, y, e=0):
    """hash160 of the compressed image e of the point: (beta^e x, y) keeps y, so the key's own prefix."""
    return oracle.hash160_comp(x * pow(BETA, e, P) % P, 2 + (y & 1))


@pytest.fixture(scope="module")
def engine512():
    import keyhunt_amd
    with keyhunt_amd.Engine(0, 512, 0) as e:
        yield e


@pytest.fixture(params=["default", "lanes512"])
def eng(request, engine, engine512):
    return engine if request.param == "default" else engine512


@pytest.fixture(params=["blocked_filter", "reference_bloom"])
def filt(request, monkeypatch):
    if request.param == "reference_bloom":
        monkeypatch.setenv("KH_REF_TARGET_BLOOM", "1")
    else:
        monkeypatch.delenv("KH_REF_TARGET_BLOOM", raising=False)
    return request.param


def _tuples(hits):
    return [(h.key, h.offset, h.compressed, h.kind) for h in hits]


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
@pytest.mark.parametrize("search", [COMPRESS, BOTH], ids=["compress", "both"])
@pytest.mark.parametrize("shape", ["big", "small"])
def test_differential_against_the_plain_path(eng, filt, planted, oracle, shape, search, endo):
    start, n, pts = planted[shape]
    # -e: the rows come from all three images in turn, so every image's nested probe is hit
    rows = [plain_row(oracle, x, y, i % 3 if endo else 0) for i, (_, _, x, y) in enumerate(pts)]
    mode = MODE_ADDRESS | (ENDO if endo else 0)
    eng.set_targets(rows)
    plain = _tuples(eng.scan(start, n, mode=mode, search=search))
    assert len(plain) == N_PLANT and [t[1] for t in plain] == [o for _, o, _, _ in pts]
    if not endo:
        assert [t[0] for t in plain] == [k for k, _, _, _ in pts]
    else:
        assert {(t[3] >> 4) & 3 for t in plain} == {0, 1, 2}
    assert all(c for _, _, c, _ in plain) and {t[3] & 15 for t in plain} == {0, 1}
    eng.set_targets([nested(oracle, r) for r in rows])
    got = _tuples(eng.scan(start, n, mode=mode | P2SH, search=search))
    assert got == [(k, o, c, kind | KIND_P2SH) for k, o, c, kind in plain]
    # the nested rows without the flag: nothing computes them
    assert eng.scan(start, n, mode=mode, search=search) == []


@pytest.mark.parametrize("search", [COMPRESS, BOTH], ids=["compress", "both"])
@pytest.mark.parametrize("shape", ["big", "small"])
def test_mixed_plain_and_nested_rows(eng, filt, planted, oracle, shape, search):
    """Half the keys as plain rows (a bech32 or P2PKH target), half as nested ones, in one scan: every
    key once, with its kind, by offset."""
    start, n, pts = planted[shape]
    rows, want = [], []
    for i, (k, o, x, y) in enumerate(pts):
        r = plain_row(oracle, x, y)
        rows.append(nested(oracle, r) if i % 2 else r)
        want.append((k, o, True, (y & 1) | (KIND_P2SH if i % 2 else 0)))
    eng.set_targets(rows)
    assert _tuples(eng.scan(start, n, mode=MODE_ADDRESS | P2SH, search=search)) == want


@pytest.mark.parametrize("shape", ["big", "small"])
def test_order_within_a_point(eng, filt, planted, oracle, shape):
    """A point whose plain and nested digests are both rows, for all three images: per image plain
    then nested (02 / 03 by the key's parity), the uncompressed hit of -l both after them."""
    start, n, pts = planted[shape]
    some = pts[:3] + pts[-3:]
    rows = []
    for _, _, x, y in some:
        for e in range(3):
            rows += [plain_row(oracle, x, y, e), nested(oracle, plain_row(oracle, x, y, e))]
        rows.append(oracle.hash160_uncomp(x, y))
    eng.set_targets(rows)
    got = eng.scan(start, n, mode=MODE_ADDRESS | ENDO | P2SH, search=BOTH)
    want = []
    for _, o, x, y in some:
        want += [(o, (y & 1) | (e << 4) | nest) for e in range(3) for nest in (0, KIND_P2SH)] + [(o, 2)]
    assert [(h.offset, h.kind) for h in got] == want
    # without -e only image 0, in the same order
    got = eng.scan(start, n, mode=MODE_ADDRESS | P2SH, search=BOTH)
    assert [(h.offset, h.kind) for h in got] == [w for w in want if not w[1] & 0x30]
    assert [h.key for h in got] == [k for k, _, _, _ in some for _ in range(3)]


@pytest.mark.parametrize("shape", ["big", "small"])
def test_negatives(eng, filt, planted, oracle, shape):
    start, n, pts = planted[shape]
    # the nested digest of an UNCOMPRESSED key hash is never computed (a segwit key is compressed by rule)
    eng.set_targets([nested(oracle, oracle.hash160_uncomp(x, y)) for _, _, x, y in pts])
    assert eng.scan(start, n, mode=MODE_ADDRESS | P2SH, search=BOTH) == []
    assert eng.scan(start, n, mode=MODE_ADDRESS | P2SH | ENDO, search=BOTH) == []


def test_flag_is_refused_where_it_has_no_meaning(eng, planted, oracle):
    start, n, pts = planted["small"]
    rows = [nested(oracle, plain_row(oracle, x, y)) for _, _, x, y in pts]
    eng.set_targets(rows)
    for mode, search in [(MODE_ADDRESS, UNCOMPRESS), (MODE_XPOINT, COMPRESS), (MODE_XPOINT, BOTH), (MODE_ETH, BOTH),
                         (MODE_ADDRESS | ENDO, UNCOMPRESS), (MODE_XPOINT | ENDO, COMPRESS), (MODE_ETH | ENDO, BOTH)]:
        st, hits = eng.scan_status(start, n, mode=mode | P2SH, search=search)
        assert st == KH_E_ARG and hits == [], (mode, search)
    try:
        eng.set_rmd_batch(512)
        assert eng.scan_status(start, n, mode=MODE_ADDRESS | P2SH, search=COMPRESS)[0] == KH_E_ARG
    finally:
        eng.set_rmd_batch(0)
    eng.set_vanity([(b"\x00" * 20, b"\x00" * 19 + b"\x01")], 20)
    assert eng.scan_status(start, n, mode=MODE_ADDRESS | P2SH, search=COMPRESS)[0] == KH_E_ARG
    eng.set_targets(rows)
    st, hits = eng.scan_status(start, n, mode=MODE_ADDRESS | P2SH, search=COMPRESS)
    assert st == 0 and len(hits) == N_PLANT


def test_scan_memory_accepts_the_flag():
    import ctypes
    from keyhunt_amd.engine import lib
    for n, mode, search in [(1 << 32, 0, 0), (1 << 32, 0, 2), (1 << 20, 0x10, 0)]:
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        assert lib().kh_scan_memory(n, mode, search, ctypes.byref(a)) == 0
        assert lib().kh_scan_memory(n, mode | P2SH, search, ctypes.byref(b)) == 0
        assert a.value == b.value > 0


def test_lanes_continue_across_p2sh_chunks(engine, filt, planted, oracle):
    """Two consecutive chunks of the first shape, the keys in the second: the second call continues the
    first one's lanes (one lane setup) and reports what a scan starting there reports.  The mode bit is
    part of what must match: after a plain chunk the P2SH chunk starts its lanes again."""
    from keyhunt_amd.engine import TIME_SETUP
    start2, n, pts = planted["big"]
    start1 = start2 - n
    engine.set_targets([nested(oracle, plain_row(oracle, x, y)) for _, _, x, y in pts])
    fresh = _tuples(engine.scan(start2, n, mode=MODE_ADDRESS | P2SH, search=COMPRESS))
    assert len(fresh) == N_PLANT
    engine.kernel_time_reset()
    assert engine.scan(start1, n, mode=MODE_ADDRESS | P2SH, search=COMPRESS) == []
    assert _tuples(engine.scan(start2, n, mode=MODE_ADDRESS | P2SH, search=COMPRESS)) == fresh
    assert engine.kernel_time(TIME_SETUP)[0] == 1
    engine.kernel_time_reset()
    assert engine.scan(start1, n, mode=MODE_ADDRESS, search=COMPRESS) == []
    assert _tuples(engine.scan(start2, n, mode=MODE_ADDRESS | P2SH, search=COMPRESS)) == fresh
    assert engine.kernel_time(TIME_SETUP)[0] == 2
