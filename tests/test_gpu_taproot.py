"""Taproot key-path targets on the GPU: the tweak kernel (k_tap_keys) against the Python model of
BIP-340/341 (tests/_taproot.py) point by point, and kh_taproot_scan -- windows, strides, the Y-parity rule
of the reported key, the host's 32-byte confirmation, the hit buffer and the context's other state."""
import pytest

import keyhunt_amd
from keyhunt_amd import KH_E_OVERFLOW, KH_E_RANGE, KH_E_STATE, KH_KIND_TAPROOT, KH_MODE_ADDRESS, KH_SEARCH_COMPRESS
import _taproot as T

pytestmark = pytest.mark.gpu

MIXED = [5, 6, 7, 8, 9, 10, 11, 12, 0xFFFF, 0x10000, 2**32 - 1, 2**64 + 5, 2**64 + 6, 2**128 - 1, 2**200 + 12345,
         T.N - 1, T.N - 2, T.N - 3, T.N // 2, T.N // 3, 0xC0FFEE, 0xC0FFEF, 2**255 - 19, 0x5A17C0DE00000003]


def prog(qx: int) -> bytes:
    return qx.to_bytes(32, "big")


@pytest.fixture(scope="module")
def base_points():
    """The points of the parity test and their output keys, computed once: the two published vectors'
    points with both signs of Y, keys 1, 2, 3 and 24 keys of mixed Y parity."""
    pts = []
    for internal, _, _ in T.VECTORS:
        x, y = T.lift_x(int(internal, 16))
        pts += [(x, y), (x, T.P - y)]
    pts += [T.mul_g(k) for k in (1, 2, 3)]
    mixed = [T.mul_g(k) for k in MIXED]
    assert len(mixed) == 24 and 6 <= sum(y & 1 for _, y in mixed) <= 18
    pts += mixed
    want = [prog(T.output_x(x)) for x, _ in pts]
    assert want[0].hex() == want[1].hex() == T.VECTORS[0][1] and want[2].hex() == want[3].hex() == T.VECTORS[1][1]
    assert [T.address_of_x(int.from_bytes(w, "big")) for w in want[4:7]] == list(T.SMALL_KEYS.values())
    return pts, want


def test_outputs_match_the_model_at_every_batch_slot(engine, base_points):
    """n = 1, 63, 65 and 64 batch + 1: one lane with one point, a wave short of and past 64 points (lanes
    with partly empty batches), and every slot of every lane of a first block plus one lane of a second."""
    pts, want = base_points
    batch, _ = engine.taproot_stats()
    assert batch >= 1
    for n in (1, 63, 65, 64 * batch + 1):
        # rotate so that the same point meets different lanes and slots at each n
        idx = [(i * 7 + n) % len(pts) for i in range(n)]
        got = engine.taproot_outputs([pts[j] for j in idx])
        assert got == [want[j] for j in idx], n


@pytest.fixture(scope="module")
def dense():
    """One chunk of 1024 keys from a start above 2^64, walked P += G by the model: per key the output
    key and the BIP-340 secret key."""
    start = (1 << 68) + 0x1234567
    out = []
    for i, pt in enumerate(T.walk(start, 1, 1024)):
        k = start + i
        out.append((prog(T.output_x(pt[0])), k if pt[1] % 2 == 0 else T.N - k))
    return start, out


def test_dense_chunk_every_key_is_found_with_its_bip340_key(engine, dense):
    start, out = dense
    engine.taproot_set_window(0)
    engine.taproot_set_targets([p for p, _ in out])
    hits = engine.taproot_scan(start, 1024)
    assert [h.offset for h in hits] == list(range(1024))
    assert [h.key for h in hits] == [d for _, d in out]
    assert all(h.kind == KH_KIND_TAPROOT and h.compressed for h in hits)
    # the parity rule, per hit: the key's own public key has an even Y, and both parities occurred
    negated = sum(1 for i, h in enumerate(hits) if h.key != start + i)
    assert 384 < negated < 640
    for i in (0, 1, 511, 512, 1023):
        assert T.mul_g(hits[i].key)[1] % 2 == 0


def _planted(start, stride, offsets):
    """programs, and the hits (key, offset) the scan must report, of keys start + o stride"""
    progs, want = [], []
    for o in offsets:
        k = start + o * stride
        qx, _, d, _ = T.key_output(k)
        progs.append(prog(qx))
        want.append((d, o))
    return progs, want


def test_windows_of_1024_over_3072_keys_equal_the_default_window(engine):
    start = 0x7A9000000000 + 77
    progs, want = _planted(start, 1, [0, 1023, 1024, 2047, 3071])
    absent = prog(T.key_output(start + 3072)[0])      # the first key past the chunk
    engine.taproot_set_targets(progs + [absent])
    engine.taproot_set_window(1024)
    small = engine.taproot_scan(start, 3072)
    engine.taproot_set_window(0)
    default = engine.taproot_scan(start, 3072)
    assert [(h.key, h.offset) for h in small] == want
    assert small == default


def test_stride_and_a_start_above_2_64(engine):
    start, stride = (1 << 100) + 0xABCDEF, 7
    progs, want = _planted(start, stride, [0, 1, 5, 512, 1023, 1024, 2047])
    engine.taproot_set_window(1024)
    engine.taproot_set_targets(progs)
    hits = engine.taproot_scan(start, 2048, stride=stride)
    engine.taproot_set_window(0)
    assert [(h.key, h.offset) for h in hits] == want


def test_a_chunk_that_reaches_the_group_order_is_refused(engine):
    engine.taproot_set_targets([prog(T.key_output(T.N - 5)[0])])
    r, hits, n = engine.taproot_scan_status(T.N - 1024, 1024)
    assert r == KH_E_RANGE and not hits
    r, hits, n = engine.taproot_scan_status(T.N - 7 * 1024, 1024, stride=7)
    assert r == KH_E_RANGE and not hits
    # the last whole chunk below the order is scanned
    hits = engine.taproot_scan(T.N - 1025, 1024)
    assert [(h.key, h.offset) for h in hits] == [(T.key_output(T.N - 5)[2], 1020)]


def test_host_confirms_all_32_bytes(engine):
    start = 0x31337000000
    real = prog(T.key_output(start + 300)[0])
    fake = real[:25] + bytes([real[25] ^ 0x40]) + real[26:]
    engine.taproot_set_targets([fake])
    assert engine.taproot_scan(start, 1024) == []
    assert engine.taproot_stats()[1] >= 1            # the device did report the 20-byte match
    engine.taproot_set_targets([fake, real])
    assert [h.offset for h in engine.taproot_scan(start, 1024)] == [300]


def test_hit_buffer_overflow_reports_the_true_count(engine):
    start = 0x5EED0000000
    progs, want = _planted(start, 1, [10, 500, 1000])
    engine.taproot_set_targets(progs)
    r, hits, n = engine.taproot_scan_status(start, 1024, cap=1)
    assert r == KH_E_OVERFLOW and n == 3
    assert [(h.key, h.offset) for h in hits] == want[:1]


def test_argument_and_state_checks(engine):
    import ctypes
    L = keyhunt_amd.lib()
    n = ctypes.c_uint32()
    hits = (keyhunt_amd.engine.KhHit * 4)()
    be32 = keyhunt_amd.engine.be32
    engine.taproot_set_targets([bytes(32)])
    scan = lambda st, sd, nk, h=hits, nh=ctypes.byref(n): L.kh_taproot_scan(engine._ctx, st, sd, nk, h, 4, nh)
    assert scan(be32(1), be32(0), 1024) == -1        # stride 0
    assert scan(be32(1), None, 1000) == -1           # no multiple of 1024
    assert scan(be32(1), None, 0) == -1
    assert scan(None, None, 1024) == -1
    assert scan(be32(1), None, 1024, None) == -1     # no array for cap 4
    assert scan(be32(1), None, 1024, hits, None) == -1
    assert L.kh_taproot_set_window(engine._ctx, 1000) == -1
    assert scan(be32(1), None, 1024) == 0
    engine.taproot_set_targets([])                   # no programs: the scan is out of order
    assert scan(be32(1), None, 1024) == KH_E_STATE


def test_kh_scan_is_the_same_before_and_after_a_taproot_scan(engine, oracle):
    """kh_scan's rows stay as they were and its kept lanes are not resumed: two consecutive 2^16-key chunks
    (interleaved 4096-point groups, so the first leaves a continuation) with a taproot scan in between give
    what a fresh context gives for them."""
    start, n = 0x6B00000000, 1 << 16
    keys = [start + o for o in (3, 4095, 4096, n - 1, n, n + 4464, 2 * n - 1)]
    rows = []
    for k in keys:
        x, y = oracle.pubkey(k)
        rows.append(oracle.hash160_comp(x, 2 + (y & 1)))
    tprog, twant = _planted(start + 100, 1, [0, 2047])

    def chunks(e, between):
        a = e.scan(start, n, KH_MODE_ADDRESS, KH_SEARCH_COMPRESS)
        t = between(e)
        b = e.scan(start + n, n, KH_MODE_ADDRESS, KH_SEARCH_COMPRESS)
        return a, t, b

    with keyhunt_amd.Engine(0) as fresh:
        fresh.set_targets(rows)
        fa, _, fb = chunks(fresh, lambda e: None)
    assert sorted(h.key for h in fa + fb) == sorted(keys)
    engine.set_targets(rows)
    engine.taproot_set_targets(tprog)
    a, t, b = chunks(engine, lambda e: e.taproot_scan(start + 100, 2048))
    assert [(h.key, h.offset) for h in t] == twant
    assert (a, b) == (fa, fb)
