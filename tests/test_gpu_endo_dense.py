"""The -e walks and the --rmd-batch-size walks pinned dense: a target on every image of every slot.

tests/test_gpu_walk_offsets.py plants a key at every in-group offset of the walks without -e; the -e
instantiations of k_walk (H160C/U/B, XPOINT, ETH), every k_walk_zinv instantiation (H160C/U/B and ETH,
each with and without -e) and the host's key rules (resolve_hits in keyhunt_amd/csrc/kh_capi.cpp: the
lambda power, the sign by base kind / image / degenerate slot / -e, the eth slot-4 twin, the per-point
sort) were pinned by a handful of hits each.  Here every slot of a chunk is a target under one image
class, class = (offset + group) mod C (small groups: (slot + 5 group) mod C), so every (in-group offset, image)
pair occurs; rows are built in closed form (tests/_endo_rows.py) and the engine's whole hit list --
key, compressed flag, kind, order -- must equal oracle.scan_chunk's, which the reference CLI pins
(tests/test_oracle.py: the eth -e, eth -e batch 8 / 512 and stride fixtures).  Each case runs at the
default geometry and on four lanes (a lane then walks several groups in turn)."""
import pytest

from _endo_rows import CASES, ETH_BETA, TWIN, check_hits, kind_of, plant, row, survives_without_e, triples, zinv_point

pytestmark = pytest.mark.gpu

START = (1 << 65) + 0x1A2B3C4D5E6F7            # case a, b, c: 12 groups of 1024 keys
N_GROUPS, GRP = 12, 1024
START_STRIDE, STRIDE, N_STRIDE = (1 << 66) + 0x0F0E0D0C0B0A9, 7919, 4 * 1024
START_ZINV = (1 << 67) + 0x123456789ABCD
ZINV = {4: 64, 8: 48, 100: 12, 512: 4, 1020: 3}   # group size -> groups
ENDO_CASES = ["compress_e", "uncompress_e", "both_e", "xpoint_e", "eth_e"]
ZINV_CASES = ["both", "both_e", "compress_e", "uncompress_e", "eth", "eth_e"]


@pytest.fixture(scope="module")
def points(oracle):
    """The chunks' points, computed once: keys START + t and START_STRIDE + 7919 t."""
    return {"unit": [oracle.pubkey(START + t) for t in range(N_GROUPS * GRP)],
            "stride": [oracle.pubkey(START_STRIDE + t * STRIDE) for t in range(N_STRIDE)]}


@pytest.fixture(scope="module")
def memo():
    """Rows and oracle lists shared by the two geometries of a case."""
    return {}


@pytest.fixture(params=[0, 4], ids=["default", "lanes4"])
def geom(request, engine):
    engine.set_geometry(request.param, 0)
    try:
        yield engine
    finally:
        engine.set_geometry(0, 0)


def _cls(t, C):
    """The class of chunk offset t: (in-group offset + group) mod C."""
    return (t % GRP + t // GRP) % C


def _dense(oracle, memo, case, pts, start, stride):
    """Every slot a target under class (offset + group) mod C, the negative controls of the case, and
    the oracle's lists with and without -e."""
    key = ("dense", case, start)
    if key not in memo:
        mode, search, _, classes = CASES[case]
        C, n = len(classes), len(pts)
        rows, planted = plant(oracle, classes, [(t, pts[t], _cls(t, C)) for t in range(n)])
        n_planted_rows = len(rows)
        assert n_planted_rows == n
        # negative controls: 04 rows under -l compress, (beta^2 x, +y) under -c eth -e
        if case == "compress_e":
            rows += [row(oracle, ("u", e, 0), pts[t]) for e in range(3) for t in range(0, n, 97)]
        if case == "eth_e":
            rows += [row(oracle, ("eth", 2, 0), pts[t]) for t in range(0, n, 97)]
        cap = 4 * n
        ref = oracle.scan_chunk(mode, search, start, n, rows, cap=cap, endo=True, stride=stride)
        ref0 = oracle.scan_chunk(mode, search, start, n, rows, cap=cap, stride=stride)
        memo[key] = (rows, planted, ref, ref0)
    return memo[key]


def _run_dense(e, oracle, memo, case, pts, start, stride):
    mode, search, _, classes = CASES[case]
    C, n = len(classes), len(pts)
    rows, planted, ref, ref0 = _dense(oracle, memo, case, pts, start, stride)
    kinds = [kind_of(c) for c in classes] + ([TWIN] if case == "eth_e" else [])
    e.set_targets(rows)
    got = e.scan(start, n, mode=mode, search=search, stride=stride, cap=4 * n, endo=True)
    check_hits(got, ref, planted, kinds)
    # one record per slot, and the slot-4 twin of every eth(beta S) plant: the controls hit nothing
    twins = sum(1 for _, k in planted if k == ETH_BETA) if case == "eth_e" else 0
    assert len(got) == n + twins
    assert {h.offset % GRP for h in got} == set(range(GRP))
    for k in kinds:  # every (in-group offset, kind) pair occurs when the chunk has C groups or more
        if n >= C * GRP and k != TWIN:
            assert {h.offset % GRP for h in got if h.kind == k} == set(range(GRP)), hex(k)
    # without -e only the plain images of the same targets are found
    got0 = e.scan(start, n, mode=mode, search=search, stride=stride, cap=4 * n)
    assert triples(got0) == ref0
    assert [h.offset for h in got0] == [t for t in range(n) if survives_without_e(classes[_cls(t, C)])]


@pytest.mark.parametrize("case", ENDO_CASES)
def test_endo_walk_every_offset_every_image(geom, oracle, points, memo, case):
    """a, b: 12 x 1024 keys above 2^65, k_walk<... | KM_ENDO> in 1024-point groups: slots 0, 511, 512,
    513 and 1023 included, each under every image."""
    _run_dense(geom, oracle, memo, case, points["unit"], START, 1)


@pytest.mark.parametrize("case", ["both_e", "eth_e"])
def test_endo_walk_every_offset_with_a_stride(geom, oracle, points, memo, case):
    """d: four groups with -I 7919 (the table holds multiples of 7919 G, slot keys advance by 7919)."""
    _run_dense(geom, oracle, memo, case, points["stride"], START_STRIDE, STRIDE)


# the reference's record order within one point (the oracle restates it; written out here)
POINT_ORDER = {
    "compress_e": [0x00, 0x01, 0x10, 0x11, 0x20, 0x21],
    "uncompress_e": [0x02, 0x42, 0x12, 0x52, 0x22, 0x62],
    "both_e": [0x00, 0x01, 0x10, 0x11, 0x20, 0x21, 0x02, 0x42, 0x12, 0x52, 0x22, 0x62],
    "xpoint_e": [0x03, 0x13, 0x23],
    "eth_e": [0x05, 0x45, 0x15, 0x55, 0x25, 0x65],
}


@pytest.mark.parametrize("case", ENDO_CASES)
def test_endo_walk_all_images_of_one_point(engine, oracle, points, case):
    """c: three keys -- a group's slot 0, a centre, a slot 1023 -- take every image of their point as
    targets (12, 6, 6, 3 or 5 rows each): the records of each point come in the reference's order (the
    host's sort; the eth twin between slots 3 and 5), and every key's own public key is a target."""
    mode, search, _, classes = CASES[case]
    n = 4 * GRP
    offs = [1 * GRP, 2 * GRP + 512, 3 * GRP + 1023]
    rows, planted = plant(oracle, classes, [(t, points["unit"][t], None) for t in offs])
    assert len(rows) == 3 * len(classes) == 3 * {"both_e": 12, "xpoint_e": 3, "eth_e": 5}.get(case, 6)
    engine.set_targets(rows)
    got = engine.scan(START, n, mode=mode, search=search, cap=4 * n, endo=True)
    ref = oracle.scan_chunk(mode, search, START, n, rows, cap=4 * n, endo=True)
    check_hits(got, ref, planted, POINT_ORDER[case])
    assert [(h.offset, h.kind) for h in got] == [(t, k) for t in offs for k in POINT_ORDER[case]]
    for h in got:  # the key reported for an image is the key of that image
        x, y = oracle.pubkey(h.key)
        own = ("c", 0, y & 1) if h.compressed else (classes[-1][0], 0, 0)
        assert row(oracle, own, (x, y)) in rows, (h.offset, hex(h.kind))
    # the twin's key is the negated lambda^2 multiple: the key of the slot-5 image
    if case == "eth_e":
        assert [h.key for h in got if h.kind == TWIN] == [h.key for h in got if h.kind == 0x65]


def _zinv(oracle, memo, case, G):
    key = ("zinv", case, G)
    if key not in memo:
        mode, search, endo, classes = CASES[case]
        groups, half, C = ZINV[G], G // 2, len(classes)
        mult = memo.setdefault("mult", [oracle.pubkey(i + 1) for i in range(510)])
        # the five eth -e images: 5 g is 0 mod 5 and would leave a slot the same image in every group
        # (and G = 4 without any eth(-beta^2 S) plant), so there the class moves by 1 per group
        step = 1 if C % 5 == 0 else 5
        slots = []
        for g in range(groups):
            centre = oracle.pubkey(START_ZINV + g * G + half)
            slots += [(g * G + t, zinv_point(centre, mult, G, t), (t + step * g) % C) for t in range(G)]
        rows, planted = plant(oracle, classes, slots)
        n = groups * G
        ref = oracle.scan_chunk(mode, search, START_ZINV, n, rows, cap=4 * n, endo=endo, group=G)
        memo[key] = (rows, planted, ref)
    return memo[key]


@pytest.mark.parametrize("G", sorted(ZINV))
@pytest.mark.parametrize("case", ZINV_CASES)
def test_rmd_batch_walk_every_slot_every_image(geom, oracle, memo, case, G):
    """e: k_walk_zinv, all eight instantiations: groups of G slots, each slot's target the point the
    reference produces there (the centre's real point, else the degenerate one), under class
    (slot + 5 group) mod C (-c eth -e, C = 5: slot + group).  The two slots G/2 +- (i+1) share an x, so a row planted for one is an image
    of the other too: up to twice as many hits as rows, all equal to the oracle's, in its order."""
    mode, search, endo, classes = CASES[case]
    rows, planted, ref = _zinv(oracle, memo, case, G)
    n = ZINV[G] * G
    kinds = [kind_of(c) for c in classes] + ([TWIN] if case == "eth_e" else [])
    geom.set_targets(rows)
    geom.set_rmd_batch(G)
    try:
        got = geom.scan(START_ZINV, n, mode=mode, search=search, cap=4 * n, endo=endo)
    finally:
        geom.set_rmd_batch(1024)
    check_hits(got, ref, planted, kinds)
    assert {h.offset for h in got} == set(range(n))
    assert len(rows) <= len(got) <= 2 * len(rows) + sum(1 for h in got if h.kind == TWIN)
