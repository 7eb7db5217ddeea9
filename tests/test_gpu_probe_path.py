"""The device probe path bit for bit: point -> 20-byte digest -> filter key -> filter answer.

Every check is exact equality against the CPU oracle (pinned to the reference's own hash and bloom
code, tests/test_oracle.py and tests/test_probe_model.py) or against the written specification of the
blocked exact-target filter (tests/_probe_model.py).  The filters are overfilled on purpose, so the
models themselves answer "yes" to a visible share of non-members: a probe that says "yes" too often,
stops early, or reads the wrong words disagrees with them item by item."""
import json
import os
import random
import struct

import pytest

import _probe_model as pm
from conftest import GOLDEN
from keyhunt_amd.engine import KhError

pytestmark = pytest.mark.gpu
VEC = json.load(open(os.path.join(GOLDEN, "ref_vectors.json")))
SEED = 0x59F2815B16F81798
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
# the smallest scalars whose x-coordinate starts with 3 and with 4 zero bytes (a CPU search over k*G,
# k = 1, 2, ...; the 1- and 2-byte ones are searched for below)
K_X_3_ZERO_BYTES, K_X_4_ZERO_BYTES = 0x8459ED, 0xB990305


# ---------------------------------------------------------------------------------------------
# digests
# ---------------------------------------------------------------------------------------------
def _leading_zero_bytes(x):
    return 32 - (x.bit_length() + 7) // 8


@pytest.fixture(scope="module")
def digest_points(oracle):
    """(points, oracle digests): seeded k*G, structured points, reference points, off-curve pairs."""
    rng = random.Random(2024)
    ks = [rng.randrange(1, N) for _ in range(4096)]
    # x with 1 and 2 leading zero bytes: the first such k = 1, 2, ... (a walk over 2^16 keys)
    xs, _ = oracle.walk_points(1, 64)
    small = {}
    for i in range(64 * 1024):
        z = 0
        while xs[32 * i + z] == 0:
            z += 1
        if z and z not in small:
            small[z] = 1 + i
    assert sorted(small)[:2] == [1, 2]
    zero_ks = [small[1], small[2], K_X_3_ZERO_BYTES, K_X_4_ZERO_BYTES]
    for z, k in enumerate(zero_ks, 1):
        assert _leading_zero_bytes(oracle.pubkey(k)[0]) == z
    ks += zero_ks + [N - k for k in zero_ks]          # k and -k: the same x with both y parities
    ks += [int(v["k"], 16) for v in VEC["pubkeys"]]   # the 25 reference points
    pts = [oracle.pubkey(k) for k in ks]
    assert {y & 1 for _, y in pts[-33:-25]} == {0, 1}
    # arbitrary (x, y), not on the curve: byte patterns real points do not show
    full = (1 << 256) - 1
    pat = [0, full, 1, 1 << 255, 0x80, 0xFF << 248, int("55" * 32, 16), int("aa" * 32, 16)]
    pat += [0xFFFFFFFF << (32 * i) for i in range(8)] + [full ^ (0xFFFFFFFF << (32 * i)) for i in range(8)]
    off = [(x, y) for x in pat[:8] for y in pat[:8]] + [(p, pat[(i * 7) % len(pat)]) for i, p in enumerate(pat)]
    off += [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(300 - len(off))]
    pts += off
    ref = [(oracle.hash160_comp(x, 2), oracle.hash160_comp(x, 3), oracle.hash160_uncomp(x, y),
            oracle.eth_address(x, y)) for x, y in pts]
    return pts, ref


def test_digests_vs_oracle(engine, digest_points):
    """hash160_comp2 (the interleaved pair every compressed walk computes), hash160_uncomp and
    eth_address equal the oracle's digests on every point."""
    pts, ref = digest_points
    got = engine.digests(pts)
    assert len(got) == len(ref)
    for p, g, r in zip(pts, got, ref):
        assert g == r, (hex(p[0]), hex(p[1]))


def test_pair_digest_equals_single_chain_digest(engine, digest_points):
    """hash160_comp2's two outputs equal the device's own single-chain hash160_comp (and the
    uncompressed digests of the two entry points agree)."""
    pts, ref = digest_points
    single = engine.hash160(pts)
    pair = engine.digests(pts)
    for s, d, r in zip(single, pair, ref):
        assert s == d[:3]
        assert s == r[:3]


def test_reference_points_digests(engine):
    """The 25 reference points against the digests the reference itself printed."""
    pts = [(int(v["x"], 16), int(v["y"], 16)) for v in VEC["pubkeys"]]
    for v, d in zip(VEC["pubkeys"], engine.digests(pts)):
        assert (d[0].hex(), d[1].hex(), d[2].hex()) == (v["h02"], v["h03"], v["h04"])
    pts = [(int(v["xy"][:64], 16), int(v["xy"][64:], 16)) for v in VEC["eth"]]
    for v, d in zip(VEC["eth"], engine.digests(pts)):
        assert d[3].hex() == v["address"]


# ---------------------------------------------------------------------------------------------
# filter keys
# ---------------------------------------------------------------------------------------------
def test_filter_keys_every_prefix_length(engine, oracle):
    """(a, b) as the walks derive them equal XXH64(item[:len], seed) and XXH64(item[:len], a) for
    len 1..20: the 8-byte loop, the 4-byte step, the byte tail and the whole-digest form."""
    rng = random.Random(77)
    items = [rng.randbytes(20) for _ in range(512)]
    items += [bytes(20), b"\xff" * 20]
    items += [bytes(i) + bytes([v]) + bytes(19 - i) for i in range(20) for v in (0x01, 0x80, 0xFF)]
    for ln in range(1, 21):
        got = engine.filter_keys(items, ln)
        for it, (a, b) in zip(items, got):
            ea = oracle.xxh64(it[:ln], SEED)
            assert (a, b) == (ea, oracle.xxh64(it[:ln], ea)), (ln, it.hex())


# ---------------------------------------------------------------------------------------------
# reference-layout probe
# ---------------------------------------------------------------------------------------------
WINDOW = (0.01, 0.15)   # the share of non-members the model itself must answer "yes" to


@pytest.fixture(scope="module")
def bloom_rows():
    """26,000 members and 50,000 non-members.  The members' first byte comes from 20 values: a
    1-byte prefix filter holds at most 256 keys (5,120 of its 287,551 bits), so it has no false
    positives to show, and the non-members' "yes" answers at that length are those that share a
    member's first byte -- 20/256 of them, inside the window."""
    rng = random.Random(4242)
    first = rng.sample(range(256), 20)
    members = list(dict.fromkeys(bytes([rng.choice(first)]) + rng.randbytes(19) for _ in range(26000)))
    mset = set(members)
    assert len(members) == 26000
    strangers = []
    while len(strangers) < 50000:
        s = rng.randbytes(20)
        if s not in mset:
            strangers.append(s)
    return members, strangers


def _bloom_expect(model, members, strangers, ln):
    """The model's answers for members + strangers keyed on their first ln bytes, after the check that
    gives the comparison its teeth: every member passes, and so does a visible share of strangers."""
    exp = [model.check(p[:ln]) for p in members + strangers]
    assert all(exp[:len(members)])
    share = sum(exp[len(members):]) / len(strangers)
    assert WINDOW[0] <= share <= WINDOW[1], share
    return exp


def _check_probe(engine, model, members, strangers, ln):
    probes = members + strangers
    exp = _bloom_expect(model, members, strangers, ln)
    eager, lazy = engine.bloom_check2(0, probes, probe_len=ln if ln < 20 else 0)
    assert eager == exp
    assert lazy == exp


def test_reference_bloom_probe_exact_on_non_members(engine, oracle, bloom_rows):
    """26,000 rows in a filter sized for 10,000 (287,551 bits, 20 hashes, fill about 0.84): the eager
    and the lazy device probe each equal oracle.Bloom's answer on every member and non-member."""
    members, strangers = bloom_rows
    model = oracle.Bloom(10000)
    assert (model.bits, model.hashes) == (287551, 20)
    for m in members:
        model.add(m)
    engine.set_targets(members, bloom_items=10000)
    assert engine.get_bloom(0) == model.raw()
    _check_probe(engine, model, members, strangers, 20)
    # the plain entry point still answers as before
    assert engine.bloom_check(0, strangers[:2000]) == [model.check(s) for s in strangers[:2000]]


@pytest.mark.parametrize("ln", [1, 3, 4, 7, 8, 11, 12, 19])
def test_prefix_bloom_probe_exact_on_non_members(engine, oracle, bloom_rows, ln):
    """The same through set_vanity at prefix length ln: the host's insert (get_bloom(0) byte-equal to a
    model filled with A[:ln]) and both device probes keyed on the first ln bytes of 20-byte items."""
    members, strangers = bloom_rows
    model = oracle.Bloom(10000)
    for m in members:
        model.add(m[:ln])
    engine.set_vanity([(m, m) for m in members], ln, bloom_items=10000)
    assert engine.get_bloom(0) == model.raw()
    _check_probe(engine, model, members, strangers, ln)
    with pytest.raises(KhError, match="out of order"):
        engine.tblk_check(members[:4])   # no exact targets: KH_E_STATE


# ---------------------------------------------------------------------------------------------
# blocked target filter
# ---------------------------------------------------------------------------------------------
def test_blocked_target_filter_exact_on_non_members_and_edges(engine, oracle):
    """85,000 rows (and crafted edge rows) in the blocked filter sized for 10,000 items (6,740 blocks):
    tblk_probe equals the specification model on every member and on 50,000 non-members, among them
    rows one nibble of w1 or w2 away from a member."""
    members, strangers, exp = _blocked_case(oracle)
    engine.set_targets(members, bloom_items=10000)
    got = engine.tblk_check(members + strangers)
    assert all(got[:len(members)])            # no member may get a "no"
    assert got == exp


def _blocked_case(oracle):
    """(members, strangers, the model's answers for members + strangers)."""
    rng = random.Random(555)
    blocks = pm.tblk_blocks(oracle, 10000)
    assert blocks == 6740
    w0s = [0, 1, 0xFFFFFFFF, 0xFFFFFFFE]
    for k in (1, 2, 3370, 6739):
        lo = -((-k << 32) // blocks)   # ceil(k * 2^32 / blocks)
        w0s += [lo, lo - 1]
    # all nibbles 0 / 15, equal nibbles (the two picks of a half coincide), halves one nibble apart
    pats = [0x00000000, 0xFFFFFFFF, 0x11111111, 0x77777777, 0xABCDABCE, 0x12341234]
    crafted = [struct.pack("<5I", w0, w1, w2, rng.getrandbits(32), rng.getrandbits(32))
               for w0 in w0s for w1 in pats for w2 in pats]
    members = list(dict.fromkeys([rng.randbytes(20) for _ in range(85000)] + crafted))
    mset = set(members)
    model = pm.TargetBlockFilter(blocks)
    for m in members:
        model.add(m)

    def nibble_off(row):
        w = list(pm.words(row))
        w[rng.choice((1, 2))] ^= rng.randrange(1, 16) << (4 * rng.randrange(8))
        return struct.pack("<5I", *w)

    strangers = [nibble_off(m) for m in crafted] + [nibble_off(rng.choice(members)) for _ in range(1500)]
    # the edge block words with other position words
    strangers += [struct.pack("<5I", w0, rng.getrandbits(32), rng.getrandbits(32), 0, 0) for w0 in w0s for _ in range(8)]
    strangers = [s for s in strangers if s not in mset]
    while len(strangers) < 50000:
        s = rng.randbytes(20)
        if s not in mset:
            strangers.append(s)
    exp_m = [model.check(m) for m in members]
    exp_s = [model.check(s) for s in strangers]
    assert all(exp_m)
    share = sum(exp_s) / len(exp_s)
    assert WINDOW[0] <= share <= WINDOW[1], share
    return members, strangers, exp_m + exp_s


# ---------------------------------------------------------------------------------------------
# vanity walk at every prefix length
# ---------------------------------------------------------------------------------------------
WALK_KEYS = 4096
KINDS = {0: ("c",), 1: ("u",), 2: ("c", "u")}   # KH_SEARCH_*: compressed forms, uncompressed form


@pytest.fixture(scope="module")
def walk_chunk(oracle):
    """A seeded 70-bit start and, per key of the chunk, its three digests (02, 03, 04)."""
    rng = random.Random(7070)
    start = (1 << 69) | rng.getrandbits(69)
    dig = []
    for i in range(WALK_KEYS):
        x, y = oracle.pubkey(start + i)
        dig.append((oracle.hash160_comp(x, 2), oracle.hash160_comp(x, 3), oracle.hash160_uncomp(x, y), y & 1))
    return start, dig


@pytest.mark.parametrize("probe_len", range(1, 21))
def test_vanity_walk_every_prefix_length(engine, oracle, walk_chunk, probe_len):
    """kh_set_vanity's contract at probe_len: a point is reported iff hash[:probe_len] passes the bloom of
    the A[:probe_len] prefixes and the hash lies in some [A, B]; key, kind and order as for exact targets
    equal to the matching hashes."""
    start, _ = walk_chunk
    for search in (0, 1, 2):
        ranges, ref = _vanity_case(oracle, walk_chunk, probe_len, search)
        engine.set_vanity(ranges, probe_len)
        got = engine.scan(start, WALK_KEYS, mode=0, search=search)
        assert [(h.key, h.compressed, h.kind) for h in got] == ref, (probe_len, search)


def _vanity_case(oracle, walk_chunk, probe_len, search):
    """(ranges, expected hit list) of one scan: four ranges planted on true hashes of chunk keys (A the
    hash with the bytes from probe_len on zeroed, B with them 0xFF) and one range whose B leaves A's
    prefix, with a true hash under B's prefix only -- in the range, but not in the bloom."""
    start, dig = walk_chunk
    rng = random.Random(1000 + probe_len)
    offs = rng.sample(range(WALK_KEYS), 5)

    def true_hash(i, j):
        h02, h03, h04, odd = dig[i]
        if search == 1 or (search == 2 and j % 2):
            return h04
        return h03 if odd else h02

    planted = [true_hash(i, j) for j, i in enumerate(offs[:4])]
    tail = 20 - probe_len
    ranges = [(h[:probe_len] + bytes(tail), h[:probe_len] + b"\xff" * tail) for h in planted]
    hx = true_hash(offs[4], 0)
    px = int.from_bytes(hx[:probe_len], "big")
    assert px > 0
    ranges.append(((px - 1).to_bytes(probe_len, "big") + bytes(tail), hx[:probe_len] + b"\xff" * tail))
    model = oracle.Bloom(len(ranges))
    for a, _ in ranges:
        model.add(a[:probe_len])
    match = set()
    for h02, h03, h04, _ in dig:
        for h in ((h02, h03) if "c" in KINDS[search] else ()) + ((h04,) if "u" in KINDS[search] else ()):
            if model.check(h[:probe_len]) and any(a <= h <= b for a, b in ranges):
                match.add(h)
    assert set(planted) <= match
    if not any(a[:probe_len] == hx[:probe_len] for a, _ in ranges):
        assert hx not in match      # the model has no false positive on it: the bloom gates the range
    ref = oracle.scan_chunk(oracle.MODE_ADDRESS, search, start, WALK_KEYS, sorted(match))
    assert len(ref) >= 4
    return ranges, ref


# ---------------------------------------------------------------------------------------------
# hit-buffer overflow and redo
# ---------------------------------------------------------------------------------------------
def test_scan_hit_buffer_overflow_redo(oracle):
    """256 one-byte prefixes make the device report every hash of a 2^15-key chunk (3 x 2^15 = 98,304
    against a buffer of 65,536): kh_scan grows the buffer, starts the lanes again, redoes the chunk and
    returns exactly the planted hits; an exact-target scan on the same engine afterwards is exact.  A
    fresh engine, so the buffer is at its initial size whatever ran before."""
    import keyhunt_amd
    rng = random.Random(31337)
    n_keys = 1 << 15
    start = (1 << 69) | rng.getrandbits(69)
    k1, k2 = start + rng.randrange(n_keys), start + rng.randrange(n_keys)
    x1, y1 = oracle.pubkey(k1)
    x2, y2 = oracle.pubkey(k2)
    planted = [oracle.hash160_comp(x1, 2 + (y1 & 1)), oracle.hash160_uncomp(x2, y2)]
    ranges = [(bytes([v]) + bytes(19), bytes([v]) + bytes(19)) for v in range(256)] + [(h, h) for h in planted]
    ref = oracle.scan_chunk(oracle.MODE_ADDRESS, 2, start, n_keys, planted)
    assert sorted(k for k, _, _ in ref) == sorted([k1, k2])
    with keyhunt_amd.Engine(0) as e:
        e.set_vanity(ranges, 1)
        got = e.scan(start, n_keys, mode=0, search=2)
        assert [(h.key, h.compressed, h.kind) for h in got] == ref
        assert e.scan_device_hits() == (3 * n_keys, 1)
        # the same chunk again fits the grown buffer: no redo, the same hits
        got = e.scan(start, n_keys, mode=0, search=2)
        assert [(h.key, h.compressed, h.kind) for h in got] == ref
        assert e.scan_device_hits() == (3 * n_keys, 0)
        # an ordinary exact-target scan afterwards: the lanes were started again correctly
        keys = sorted(start + rng.randrange(n_keys) for _ in range(6))
        rows = []
        for j, k in enumerate(keys):
            x, y = oracle.pubkey(k)
            rows.append(oracle.hash160_uncomp(x, y) if j % 2 else oracle.hash160_comp(x, 2 + (y & 1)))
        e.set_targets(rows)
        got = e.scan(start, n_keys, mode=0, search=2)
        ref2 = oracle.scan_chunk(oracle.MODE_ADDRESS, 2, start, n_keys, rows)
        assert [(h.key, h.compressed, h.kind) for h in got] == ref2
        assert sorted(h.key for h in got) == keys
        assert e.scan_device_hits()[1] == 0
