"""The KH_MODE_P2SH walks pinned dense: a target on every in-group offset under every image class.

tests/test_gpu_p2sh_scan.py plants 64 keys per chunk and compares with the engine's own plain path, so a
position error the plain and the nested instantiations share cancels out, and most (offset, image, prefix,
plain / nested) combinations are never visited.  Here the expected lists never come from the engine:

A1  18 x 1024 keys above 2^65, every slot a target under class (offset + group) mod C of its case
    (tests/_p2sh_rows.py: the classes of tests/_endo_rows.py, each "c" class plain and nested).  The list
    is oracle.scan_chunk's for the slots' UN-nested rows, one record per slot, with KH_KIND_P2SH or-ed
    into the kind where the slot's class is nested.  compress: k_walk<KM_H160CB|KM_P2SH> (reference bloom:
    k_walk<KM_H160C|KM_P2SH>), both: k_walk<KM_H160B|KM_P2SH>, compress_e: k_walk<KM_H160C|KM_P2SH|KM_ENDO>,
    both_e: k_walk<KM_H160B|KM_P2SH|KM_ENDO>; each at the default geometry and on four lanes (a lane walks
    five groups in turn, the last lane past the chunk's end).
A2  one group whose every slot has all 18 rows as targets: the order within a point.
A3  four groups with a stride of 7919.
A4  2^22 keys in 4096-point groups, all 4096 offsets under each of the four classes of -l compress:
    k_walk<KM_H160CB|KM_P2SH, KH_WALK_HB> and k_walk<KM_H160C|KM_P2SH, KH_WALK_HB>, one group per lane, two
    groups per lane interleaved (512 lanes) and three per lane with the last lane past the chunk (384)."""
import random

import pytest

from _endo_rows import kind_of
from _p2sh_rows import (BOTH, CASES, COMPRESS, KIND_P2SH, MODE_ADDRESS, MODE_P2SH, first_difference, kind4, nested,
                        plain_row, records, row4, survives4)

pytestmark = pytest.mark.gpu

N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GRP = 1024
START, N_GROUPS = (1 << 65) + 0x2C4E6A8B0D1F3, 18           # A1, A2
START_STRIDE, STRIDE, N_STRIDE = (1 << 66) + 0x1B3D5F7092A4C, 7919, 4 * GRP   # A3
START_BIG, N_BIG, G_BIG = (1 << 67) + 0x3A5C7E9F1B2D4, 1 << 22, 4096  # A4
TIME_ADDRESS = 0
# the reference's record order within one point under -l both -e (tests/test_gpu_endo_dense.py)
POINT_ORDER = [0x00, 0x01, 0x10, 0x11, 0x20, 0x21, 0x02, 0x42, 0x12, 0x52, 0x22, 0x62]


@pytest.fixture(scope="module")
def points(oracle):
    """The small-group chunks' points, computed once: keys START + t and START_STRIDE + 7919 t."""
    return {"unit": [oracle.pubkey(START + t) for t in range(N_GROUPS * GRP)],
            "stride": [oracle.pubkey(START_STRIDE + t * STRIDE) for t in range(N_STRIDE)]}


@pytest.fixture(scope="module")
def memo():
    """Rows and expected lists shared by the geometries and filters of a case."""
    return {}


@pytest.fixture(params=[0, 4], ids=["default", "lanes4"])
def geom(request, engine):
    engine.set_geometry(request.param, 0)
    try:
        yield engine
    finally:
        engine.set_geometry(0, 0)


@pytest.fixture(params=["blocked_filter", "reference_bloom"])
def filt(request, monkeypatch):
    if request.param == "reference_bloom":
        monkeypatch.setenv("KH_REF_TARGET_BLOOM", "1")
    else:
        monkeypatch.delenv("KH_REF_TARGET_BLOOM", raising=False)
    return request.param


def _cls(t, C):
    """The class of chunk offset t: (in-group offset + group) mod C."""
    return (t % GRP + t // GRP) % C


def _dense(oracle, memo, case, pts, start, stride):
    """Per slot its class; the engine's rows (one per slot, then the negative controls); the expected
    (key, compressed, kind) per slot, from the oracle's scan for the slots' un-nested rows."""
    key = (case, start)
    if key not in memo:
        search, endo, classes = CASES[case]
        C, n = len(classes), len(pts)
        cls = [classes[_cls(t, C)] for t in range(n)]
        plain = [plain_row(oracle, cls[t], pts[t]) for t in range(n)]
        assert len(set(plain)) == n
        ref = oracle.scan_chunk(MODE_ADDRESS, search, start, n, plain, cap=4 * n, endo=endo, stride=stride)
        # the reference's precondition: one record per slot, slot t's being the image its row was built from
        assert len(ref) == n
        assert [r[2] for r in ref] == [kind_of(c[:3]) for c in cls]
        want = [(k, comp, kind | (KIND_P2SH if cls[t][3] else 0)) for t, (k, comp, kind) in enumerate(ref)]
        rows = [row4(oracle, cls[t], pts[t]) for t in range(n)]
        assert len(set(rows)) == n
        # negative controls: the nested digest of a 04 hash is never computed
        rows += [nested(oracle, oracle.hash160_uncomp(*pts[t])) for t in range(0, n, 97)]
        memo[key] = (cls, rows, want)
    return memo[key]


def _check(got, want, offsets):
    diff = first_difference(got, want)
    assert diff is None, diff
    assert [h.offset for h in got] == offsets


def _run_dense(e, oracle, memo, case, pts, start, stride):
    search, endo, classes = CASES[case]
    C, n = len(classes), len(pts)
    cls, rows, want = _dense(oracle, memo, case, pts, start, stride)
    e.set_targets(rows)
    scan = lambda mode, en: e.scan(start, n, mode=mode, search=search, stride=stride, cap=4 * n, endo=en)
    got = scan(MODE_ADDRESS | MODE_P2SH, endo)
    _check(got, want, list(range(n)))       # one record per slot: the controls hit nothing
    if n >= C * GRP:                        # every (in-group offset, class) pair, from the hit list
        for c in classes:
            assert {h.offset % GRP for h in got if h.kind == kind4(c)} == set(range(GRP)), c
    # the same rows without the flag: the plain classes alone
    idx = [t for t in range(n) if not cls[t][3]]
    _check(scan(MODE_ADDRESS, endo), [want[t] for t in idx], idx)
    if endo:
        # without -e image 0 alone, nested or not; and without either
        idx = [t for t in range(n) if survives4(cls[t])]
        _check(scan(MODE_ADDRESS | MODE_P2SH, False), [want[t] for t in idx], idx)
        idx = [t for t in idx if not cls[t][3]]
        _check(scan(MODE_ADDRESS, False), [want[t] for t in idx], idx)


@pytest.mark.parametrize("case", list(CASES))
def test_small_groups_every_offset_every_class(geom, filt, oracle, points, memo, case):
    """A1."""
    _run_dense(geom, oracle, memo, case, points["unit"], START, 1)


@pytest.mark.parametrize("case", ["compress", "both_e"])
def test_small_groups_every_offset_with_a_stride(geom, filt, oracle, points, memo, case):
    """A3: the table holds multiples of 7919 G and slot keys advance by 7919."""
    _run_dense(geom, oracle, memo, case, points["stride"], START_STRIDE, STRIDE)


@pytest.fixture(scope="module")
def one_group(oracle, points):
    """A2: all 18 rows of every slot of the first group, and the expected list: the oracle's for the 12
    plain rows of each point, the compressed pair [a, b] of each image expanded to [a, b, a|0x80, b|0x80]
    (resolve_hits' order: 4e + base + 2 nested, then 12 + 2e + neg), the 04 records as they are."""
    _, _, classes = CASES["both_e"]
    pts = points["unit"][:GRP]
    flat = [c for c in classes if not c[3]]
    assert [kind_of(c[:3]) for c in flat] == POINT_ORDER
    plain = [plain_row(oracle, c, pt) for pt in pts for c in flat]
    assert len(set(plain)) == 12 * GRP
    ref = oracle.scan_chunk(MODE_ADDRESS, BOTH, START, GRP, plain, cap=4 * len(plain), endo=True)
    assert len(ref) == 12 * GRP
    want = []
    for t in range(GRP):
        rec = ref[12 * t:12 * t + 12]
        assert [r[2] for r in rec] == POINT_ORDER
        for e in range(3):
            a, b = rec[2 * e], rec[2 * e + 1]
            want += [(t,) + a, (t,) + b, (t, a[0], a[1], a[2] | KIND_P2SH), (t, b[0], b[1], b[2] | KIND_P2SH)]
        want += [(t,) + r for r in rec[6:]]
    rows = [row4(oracle, c, pt) for pt in pts for c in classes]
    assert len(set(rows)) == 18 * GRP == len(want)
    return rows, want


def test_one_group_every_class_on_every_slot(engine, filt, one_group):
    """A2: 18 432 rows, 18 432 hits (below the device buffer's 2^16 entries: no redo), the records of each
    point in order, a nested record carrying the plain record's key; without -e image 0 alone."""
    rows, want = one_group
    engine.set_targets(rows)
    got = engine.scan(START, GRP, mode=MODE_ADDRESS | MODE_P2SH, search=BOTH, cap=4 * len(rows), endo=True)
    _check(got, [w[1:] for w in want], [w[0] for w in want])
    assert engine.scan_device_hits()[1] == 0
    by = {(h.offset, h.kind): h.key for h in got}
    assert all(by[(o, k & ~KIND_P2SH)] == key for (o, k), key in by.items() if k & KIND_P2SH)
    got = engine.scan(START, GRP, mode=MODE_ADDRESS | MODE_P2SH, search=BOTH, cap=4 * len(rows))
    want0 = [w for w in want if not w[3] & 0x70]
    assert len(want0) == 5 * GRP
    _check(got, [w[1:] for w in want0], [w[0] for w in want0])


# ---- A4: 4096-point groups --------------------------------------------------------------------------
BIG_CLASSES = [(s, nest) for s in (0, 1) for nest in (0, 1)]


def _big_offsets():
    """chunk offset -> class index: for each in-group offset o and class c one key in group perm_c[o],
    perm_c four seeded shuffles of the 1024 groups laid end to end (4096 entries); where two classes of an
    offset drew the same group the offset's four groups are drawn again, distinct.  Plus the chunk's
    first and last key."""
    groups = N_BIG // G_BIG
    rng = random.Random(0xA4)
    perms = []
    for _ in BIG_CLASSES:
        p = []
        for _ in range(G_BIG // groups):
            q = list(range(groups))
            rng.shuffle(q)
            p += q
        perms.append(p)
    slots = {}
    for o in range(G_BIG):
        gs = [p[o] for p in perms]
        while len(set(gs)) != len(gs):
            gs = [rng.randrange(groups) for _ in gs]
        for c, g in enumerate(gs):
            slots[g * G_BIG + o] = c
    slots.setdefault(0, 0)
    slots.setdefault(N_BIG - 1, 3)
    return slots


@pytest.fixture(scope="module")
def big(oracle):
    """(rows, expected hits by offset) of A4; the expected list in closed form: the key by the parity
    rule of keyhunt.cpp:3619-3636 (k where the key's own prefix is the class's, else n - k)."""
    slots = _big_offsets()
    assert 4 * G_BIG <= len(slots) <= 4 * G_BIG + 2
    for c in range(len(BIG_CLASSES)):    # every one of the 4096 residues under each class
        assert {t % G_BIG for t, cc in slots.items() if cc == c} == set(range(G_BIG))
    assert len({t // G_BIG for t in slots}) == N_BIG // G_BIG   # and every group holds a key
    rows, want = [], []
    for t in sorted(slots):
        s, nest = BIG_CLASSES[slots[t]]
        k = START_BIG + t
        x, y = oracle.pubkey(k)
        h = oracle.hash160_comp(x, 2 + s)
        rows.append(nested(oracle, h) if nest else h)
        want.append((k if (y & 1) == s else N_ORDER - k, t, True, s | nest << 7))
    assert len(set(rows)) == len(rows)
    return rows, want


@pytest.mark.parametrize("lanes", [0, 512, 384], ids=["default", "lanes512", "lanes384"])
def test_large_groups_every_offset_every_class(engine, filt, big, lanes):
    """A4.  The walk's launch count and point count (kh_kernel_time) are those of 4096-point groups: two
    groups per launch, so 1, 1 and 2 launches, and 342 lanes x 3 groups at 384 lanes (1024-point groups
    would take 4 and 6 launches at 512 and 384 lanes; at the default geometry the figures are the same)."""
    rows, want = big
    gpl = {0: 1, 512: 2, 384: 3}[lanes]
    L = -(-(N_BIG // G_BIG) // gpl)
    assert (L * gpl == N_BIG // G_BIG) == (lanes != 384)      # 384: the non-interleaved path, past the chunk
    engine.set_geometry(lanes, 0)
    try:
        engine.set_targets(rows)
        engine.kernel_time_reset()
        got = engine.scan(START_BIG, N_BIG, mode=MODE_ADDRESS | MODE_P2SH, search=COMPRESS, cap=2 * len(rows))
        launches, _, pts = engine.kernel_time(TIME_ADDRESS)
    finally:
        engine.set_geometry(0, 0)
    have = [(h.key, h.offset, h.compressed, h.kind) for h in got]
    if have != want:
        miss, extra = sorted(set(want) - set(have)), sorted(set(have) - set(want))
        raise AssertionError(
            f"{len(have)} hits, {len(want)} expected; missing {len(miss)} (offset mod 4096, kind) "
            f"{[(w[1] % G_BIG, hex(w[3])) for w in miss[:16]]}, extra {len(extra)} "
            f"{[(w[1] % G_BIG, hex(w[3])) for w in extra[:16]]}, the same records out of order: "
            f"{sorted(have) == sorted(want)}")
    assert (launches, pts) == ((gpl + 1) // 2, L * gpl * G_BIG)
