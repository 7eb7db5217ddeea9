"""The CPU oracle (oracle/kh_oracle.c) pinned against the reference: primitive vectors printed by the
reference's own code (tests/golden/ref_vectors.json) and the reference CLI's hit sets on
known-answer windows (tests/golden/ref_e2e.json)."""
import hashlib
import json
import os
import random

import pytest

from conftest import GOLDEN

VEC = json.load(open(os.path.join(GOLDEN, "ref_vectors.json")))
E2E = json.load(open(os.path.join(GOLDEN, "ref_e2e.json")))
P = 2**256 - 2**32 - 977


def h(x):
    return int(x, 16)


def test_field_vs_reference(oracle):
    for v in VEC["field"]:
        a, b = h(v["a"]), h(v["b"])
        assert oracle.fe_mul(a, b) == h(v["mul"]) % P
        assert oracle.fe_mul(a, a) == h(v["sqr"]) % P
        assert oracle.fe_inv(a) == h(v["inv"])


def test_pubkeys_and_hash160_vs_reference(oracle):
    for v in VEC["pubkeys"]:
        x, y = oracle.pubkey(h(v["k"]))
        assert (x, y) == (h(v["x"]), h(v["y"]))
        assert oracle.hash160_comp(x, 2).hex() == v["h02"]
        assert oracle.hash160_comp(x, 3).hex() == v["h03"]
        assert oracle.hash160_uncomp(x, y).hex() == v["h04"]
        assert oracle.decompress(x, y & 1) == y


def test_xxh64_vs_reference(oracle):
    for v in VEC["xxh64"]:
        buf = bytes.fromhex(v["buf"])
        a = oracle.xxh64(buf, 0x59F2815B16F81798)
        assert a == h(v["a"])
        assert oracle.xxh64(buf, a) == h(v["b"])


def test_bloom_sizing_vs_reference(oracle):
    for v in VEC["bloom_params"]:
        assert oracle.bloom_params(v["entries"]) == (v["bits"], v["bytes"], v["hashes"])


def test_bloom_fill_vs_reference(oracle):
    fill = VEC["bloom_fill"]
    b = oracle.Bloom(fill["entries"])
    items = [bytes.fromhex(x) for x in fill["items"]]
    for it in items:
        b.add(it)
    assert hashlib.sha256(b.raw()).hexdigest() == fill["sha256"]
    assert all(b.check(it) for it in items)


def test_group_walk_vs_reference(oracle):
    for gw in VEC["group_walk"]:
        xs, _ = oracle.walk_points(h(gw["start"]), gw["n"] // 1024)
        assert hashlib.sha256(xs).hexdigest() == gw["sha256_walk"] == gw["sha256_direct"]


@pytest.mark.parametrize("cfg", VEC["bsgs_build"][:2], ids=lambda c: f"n{c['n']:x}_k{c['k']}")
def test_bsgs_build_vs_reference(oracle, cfg):
    p = oracle.bsgs_params(cfg["n"], cfg["k"])
    assert (p.m, p.m2, p.m3) == (cfg["m"], cfg["m2"], cfg["m3"])
    t = oracle.BsgsTables(p)
    assert hashlib.sha256(t.bf1.raw).hexdigest() == cfg["sha256_l1"]
    assert hashlib.sha256(t.bf2.raw).hexdigest() == cfg["sha256_l2"]
    assert hashlib.sha256(t.bf3.raw).hexdigest() == cfg["sha256_l3"]
    assert hashlib.sha256(t.table_bytes()).hexdigest() == cfg["sha256_table"]


def test_bsgs_params_configs(oracle):
    """BASELINE configs 4/5 geometry."""
    p = oracle.bsgs_params(2**44, 128)
    assert (p.m, p.m2, p.m3, p.cycles) == (2**29, 2**24, 2**19, 32)
    assert (p.bits[0], p.bytes[0], p.hashes[0]) == (60303973, 7537997, 20)
    assert (p.bytes[1], p.bytes[2]) == (235563, 35944)
    p = oracle.bsgs_params(2**44, 512)
    assert (p.m, p.m2, p.m3, p.cycles) == (2**31, 2**26, 2**21, 8)
    assert (p.bytes[0], p.bytes[1]) == (30151987, 942250)


def _read_rows(oracle, fn, mode):
    from conftest import DATA
    rows = []
    for line in open(os.path.join(DATA, fn)):
        s = line.strip()
        if mode == "xpoint":
            if len(s) in (64, 66):
                rows.append(bytes.fromhex(s[-64:])[:20])
            continue
        if len(s) == 40:
            rows.append(bytes.fromhex(s))
        elif 20 < len(s) < 40:
            raw = oracle.address_decode(s)
            if raw:
                rows.append(raw[1:21])
    return rows


@pytest.mark.parametrize("name,fn,mode,search,endo", [
    ("rmd160_1to32_compress_2p20", "1to32.rmd", 0, 0, False),
    ("xpoint_1to63_65_2p20", "1to63_65.txt", 1, 2, False),
    ("rmd160_1to32_compress_2p20_endo", "1to32.rmd", 0, 0, True),
    ("xpoint_1to63_65_2p20_endo", "1to63_65.txt", 1, 2, True),
    ("address_endo_targets", "endo_addr.txt", 0, 2, True),
    ("address_endo_targets_no_e", "endo_addr.txt", 0, 2, False),
    ("xpoint_endo_targets", "endo_x.txt", 1, 2, True),
])
def test_oracle_scan_vs_reference_cli(oracle, name, fn, mode, search, endo):
    """Keys 1..2^20 (one 2^20 chunk): the oracle's hit list equals the reference CLI's, with and
    without -e (endo_*.txt hold lambda-multiples of small keys, tests/golden/make_endo_targets.py)."""
    rows = _read_rows(oracle, fn, "xpoint" if mode == 1 else "addr")
    hits = oracle.scan_chunk(mode, search, 1, 1 << 20, rows, endo=endo)
    assert [f"{k:x}" for k in sorted(k for k, _, _ in hits)] == [x["key"] for x in E2E[name]["hits"]]


@pytest.mark.parametrize("name,search,endo,group", [
    ("rmd160_batch512_compress", 0, False, 512),
    ("rmd160_batch512_both", 2, False, 512),
    ("rmd160_batch512_both_endo", 2, True, 512),
    ("rmd160_batch1000_compress", 0, False, 1000),
    ("rmd160_batch1000_both", 2, False, 1000),
    ("rmd160_batch1001_compress_endo", 0, True, 1000),  # the reference rounds 1001 down to 1000
    ("rmd160_batch1024_both", 2, False, 1024),
])
def test_oracle_rmd_batch_vs_reference_cli(oracle, name, search, endo, group):
    """-m rmd160 --rmd-batch-size G over 0x10000..0x20ffff in two 2^20 chunks: the oracle's walk
    (the reference's partly zero batch inversion restated, kh_oracle.c walk_group_n) finds exactly
    the reference CLI's keys -- group centres, and the negated or nominal slot keys of the points
    that are no multiples of G (tests/golden/make_rmd_batch_targets.py)."""
    assert E2E[name]["argv"][E2E[name]["argv"].index("--rmd-batch-size") + 1] in (str(group), str(group + 1))
    rows = _read_rows(oracle, "rmd_batch.rmd", "addr")
    keys = []
    for chunk in range(2):
        keys += [k for k, _, _ in oracle.scan_chunk(0, search, 0x10000 + chunk * (1 << 20), 1 << 20, rows,
                                                    endo=endo, group=group)]
    assert [f"{k:x}" for k in sorted(keys)] == [x["key"] for x in E2E[name]["hits"]]


def _keys_vs_fixture(name, hits):
    """The oracle's keys equal the fixture's as a sorted list; for a one-thread fixture
    ("hits_in_order") the oracle's own order is the reference's record order too."""
    ref = E2E[name]
    assert ref["exit"] == 0
    assert [f"{k:x}" for k in sorted(k for k, _, _ in hits)] == [x["key"] for x in ref["hits"]]
    if "hits_in_order" in ref:
        assert [f"{k:x}" for k, _, _ in hits] == [x["key"] for x in ref["hits_in_order"]]


@pytest.mark.parametrize("name,fn", [
    ("address_eth_2p20_endo", "eth_targets.txt"),
    ("address_eth_endo_2p20", "eth_endo.txt"),
    ("address_eth_endo_pair_t1", "eth_endo_pair.txt"),
])
def test_oracle_eth_endo_vs_reference_cli(oracle, name, fn):
    """-c eth -e over 1..2^20: the oracle's six slots per point (keyhunt.cpp:3524-3536, slot 4 the
    beta image again) and its per-slot keys (3714-3744) give the reference CLI's records; for the
    one-thread pair fixture also in its order (the slot-4 record between slots 3 and 5)."""
    from conftest import DATA
    rows = [bytes.fromhex(s.strip()[-40:]) for s in open(os.path.join(DATA, fn)) if len(s.strip()) in (40, 42)]
    hits = oracle.scan_chunk(oracle.MODE_ETH, 2, 1, 1 << 20, rows, endo=True)
    assert all(c is False and kind & 15 == 5 for _, c, kind in hits)
    if name == "address_eth_endo_pair_t1":
        assert "hits_in_order" in E2E[name]
        # key 9999: slots 2, 3 and the slot-4 twin; key 77777: slots 2, 4 and 5
        assert [kind for _, _, kind in hits] == [0x15, 0x55, 0x25, 0x15, 0x25, 0x65]
    _keys_vs_fixture(name, hits)


@pytest.mark.parametrize("name,fn,group,n_hits", [
    ("rmd160_eth_endo_batch8_t1", "eth_endo_batch8.rmd", 8, 51),
    ("rmd160_eth_endo_batch512_t1", "eth_endo_batch512.rmd", 512, 14),
])
def test_oracle_eth_endo_rmd_batch_vs_reference_cli(oracle, name, fn, group, n_hits):
    """-m rmd160 -c eth -e --rmd-batch-size G over 1..2^20 on one thread: the reference ran these argv
    (exit 0) and its records, in order, are the oracle's -- centres and degenerate slots (both sides of
    a centre, slot 0, the last slot) under each of the five distinct images, the six records of a
    centre whose five images are all targets, and nothing for a (beta^2 x, +y) row
    (tests/golden/make_eth_endo_batch_targets.py)."""
    argv = E2E[name]["argv"]
    assert argv[argv.index("--rmd-batch-size") + 1] == str(group) and argv[argv.index("-t") + 1] == "1"
    assert "hits_in_order" in E2E[name] and len(E2E[name]["hits"]) == n_hits
    rows = _read_rows(oracle, fn, "addr")
    hits = oracle.scan_chunk(oracle.MODE_ETH, 2, 1, 1 << 20, rows, endo=True, group=group)
    _keys_vs_fixture(name, hits)
    if group == 8:
        # every slot kind occurs, and group 97's centre (key 1 + 97 * 8 + 4) gives six records in slot order
        assert {kind for _, _, kind in hits} == {0x05, 0x45, 0x15, 0x55, 0x25, 0x65}
        at = [i for i, (k, _, kind) in enumerate(hits) if (k, kind) == (1 + 97 * 8 + 4, 0x05)]
        assert len(at) == 1
        assert [kind for _, _, kind in hits[at[0]:at[0] + 6]] == [0x05, 0x45, 0x15, 0x55, 0x25, 0x65]
    # without -e only the plain image is probed: a subset of the -e records
    plain = oracle.scan_chunk(oracle.MODE_ETH, 2, 1, 1 << 20, rows, group=group)
    assert plain and all(kind == 5 for _, _, kind in plain) and len(plain) < len(hits)


def test_oracle_endo_stride_vs_reference_cli(oracle):
    """-m address -l both -e -I 7919 over 2^20 slots from key 1 on one thread (the reference ran this
    argv, exit 0): the oracle's stride path (walk table of multiples of 7919 G, slot keys 1 + 7919 t)
    gives the reference's records in its order -- lambda and lambda^2 multiples and negations of slot
    keys, 02/03 and 04; the key between two slots is not found."""
    name = "address_endo_stride_t1"
    argv = E2E[name]["argv"]
    assert argv[argv.index("-I") + 1] == "7919" and "hits_in_order" in E2E[name]
    rows = _read_rows(oracle, "endo_stride.txt", "addr")
    assert len(rows) == 10
    hits = oracle.scan_chunk(0, 2, 1, 1 << 20, rows, endo=True, stride=7919)
    assert len(hits) == 9
    _keys_vs_fixture(name, hits)
    # stride 1 over keys 1..2^20 holds two of the planted keys: lambda * 1 and the one between two slots
    lam = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
    assert [k for k, _, _ in oracle.scan_chunk(0, 2, 1, 1 << 20, rows, endo=True)] == [lam, 1 + 5 * 7919 + 1]


@pytest.mark.parametrize("case", ["both_e", "eth_e"])
def test_dense_endo_comparison_fails_on_a_wrong_hit_list(oracle, case):
    """The comparison of tests/test_gpu_endo_dense.py (_endo_rows.check_hits), fed on the CPU: one group
    with every slot a target under class offset mod C, and one point under every image.  The oracle's own
    list (with each record's offset recovered from its key) passes; a list with one record's
    image or sign bits swapped, one record dropped, two records of a point exchanged, or a negated key
    fails."""
    from collections import namedtuple
    from _endo_rows import CASES, TWIN, check_hits, kind_of, plant
    Hit = namedtuple("Hit", "key offset kind compressed")
    mode, search, _, classes = CASES[case]
    start, n, C = (1 << 65) + 12345, 1024, len(classes)
    slots = [(t, oracle.pubkey(start + t), t % C) for t in range(n)]
    rows, planted = plant(oracle, classes, slots)
    rows += plant(oracle, classes, [(700, slots[700][1], None)])[0]  # one point under every image
    rows = list(dict.fromkeys(rows))
    planted += [(700, kind_of(c)) for c in classes]
    ref = oracle.scan_chunk(mode, search, start, n, rows, cap=4 * n, endo=True)
    kinds = [kind_of(c) for c in classes] + ([TWIN] if case == "eth_e" else [])
    lam = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
    inv = [1, pow(lam, -1, oracle.SECP_N), pow(lam * lam, -1, oracle.SECP_N)]

    def offset(key, kind):  # the slot key is +-key / lambda^e
        return min((sign * key * inv[kind >> 4 & 3] - start) % oracle.SECP_N for sign in (1, -1))
    good = [Hit(key, offset(key, kind), kind, comp) for key, comp, kind in ref]
    assert [h.offset for h in good] == sorted(h.offset for h in good) and good[-1].offset == n - 1
    assert len(good) == n + len(classes) - 1 + sum(1 for h in good if h.kind == TWIN)
    check_hits(good, ref, planted, kinds)

    def bad(i, **kw):
        return good[:i] + [good[i]._replace(**kw)] + good[i + 1:]
    i = next(j for j, h in enumerate(good) if h.offset == 700)
    wrong = [bad(5, kind=good[5].kind ^ 0x10), bad(5, kind=good[5].kind ^ 0x30),
             bad(i + 1, kind=good[i + 1].kind ^ 0x40), good[:300] + good[301:],
             good[:i] + [good[i + 1], good[i]] + good[i + 2:], bad(9, key=oracle.SECP_N - good[9].key)]
    for w in wrong:
        with pytest.raises(AssertionError):
            check_hits(w, ref, planted, kinds)


def test_oracle_scan_window_66(oracle):
    rows = _read_rows(oracle, "66.rmd", "addr")
    start = 0x2832ED74F2B5E0000
    hits = oracle.scan_chunk(0, 0, start, 1 << 16, rows)
    assert [(f"{k:x}", c) for k, c, _ in hits] == [("2832ed74f2b5e35ee", True)]
    assert [x["key"] for x in E2E["rmd160_66_window"]["hits"]] == ["2832ed74f2b5e35ee"]


def test_oracle_bsgs_known_answer_small_n(oracle):
    """-m bsgs -f 63.pub -n 0x1000000 -k 4 -r 7cce5efdac000000:7cce5efdad000000 (reference: found)."""
    p = oracle.bsgs_params(1 << 24, 4)
    t = oracle.BsgsTables(p)
    q = oracle.parse_pubkey_hex(open(os.path.join(GOLDEN, "data", "63.pub")).read().split()[0])
    key, cands = t.scan(0x7CCE5EFDAC000000, 1, q)
    assert f"{key:x}" == E2E["bsgs_63_small_n_k4"]["hits"][0]["key"]
    assert len(cands) >= 1


def test_searchbinary_is_membership(oracle):
    """keyhunt's midpoint loop (keyhunt.cpp:3065-3089) answers exact membership on sorted tables."""
    rng = random.Random(3)
    for n in list(range(1, 40)) + [100, 1000, 4097]:
        rows = sorted({rng.getrandbits(160).to_bytes(20, "big") for _ in range(n)})
        table = b"".join(rows)
        for r in rows:
            assert oracle.searchbinary(table, len(rows), r)
        for _ in range(50):
            q = rng.getrandbits(160).to_bytes(20, "big")
            assert oracle.searchbinary(table, len(rows), q) == (q in set(rows))


def test_oracle_keccak_and_eth_against_reference_vectors(oracle):
    """The oracle's Keccak-256 / generate_binaddress_eth against the reference's (ref_golden "eth")."""
    for v in VEC["eth"]:
        x, y = oracle.pubkey(int(v["k"], 16))
        assert (x.to_bytes(32, "big") + y.to_bytes(32, "big")).hex() == v["xy"]
        assert oracle.keccak256(bytes.fromhex(v["xy"])).hex() == v["keccak"]
        assert oracle.eth_address(x, y).hex() == v["address"]


def test_oracle_second_masks_window(oracle):
    """bsgs_secondcheck's layer-2 probes (keyhunt.cpp:5151-5184): for base = key - d, S = d*G and
    S + AMP2[i] = (d - (2i+1)M2)*G, whose X is a layer-2 baby X exactly when |d - (2i+1)M2| is in
    [1, M2]: bit min(d // (2 M2), 31) is set for every d in [1, 64 M2] but the odd multiples of M2
    (there S = -AMP2[i], AddDirect's dx = 0); other bits only as FPs.  Base key 0 gives 0."""
    import random
    p = oracle.bsgs_params(1 << 22, 2)
    t = oracle.BsgsTables(p)
    key = 0x3F00DEADBEEF0123
    q = oracle.pubkey(key)
    rnd = random.Random(7)
    ds = [1, p.m2 - 1, p.m2 + 1, 2 * p.m2, 64 * p.m2] + [rnd.randrange(1, 64 * p.m2 + 1) for _ in range(60)]
    ds = [d for d in ds if d % (2 * p.m2) != p.m2]
    masks = oracle.bsgs_second_masks(t, [key - d for d in ds], q)
    for d, m in zip(ds, masks):
        assert (m >> min(d // (2 * p.m2), 31)) & 1, (d, hex(m))
    assert oracle.bsgs_second_masks(t, [0], q) == [0]


def blk_spec_bits(xb, blocks):
    """The blocked layer 1's layout, from its specification: (byte offset, bit) of the 16 bits the
    32-byte X `xb` owns in a filter of 256 shards x `blocks` 16-byte blocks."""
    base = xb[0] * blocks * 16 + ((int.from_bytes(xb[8:12], "big") * blocks) >> 32) * 16
    s = [int.from_bytes(xb[12 + 4 * q:16 + 4 * q], "big") for q in range(2)]
    for w in range(4):
        a = s[w // 2] >> (8 * (w % 2))
        for v in (a, a >> 4):
            for f in (v & 15, 16 + ((v >> 16) & 15)):
                yield base + 4 * w + (f >> 3), 1 << (f & 7)


def test_oracle_blocked_layer1_check_vs_spec_model(oracle):
    """or_blk_check (the oracle's probe of the engine's blocked layer 1) against a filter written
    from the layout's specification in Python (the same model test_blocked_layer1_bytes_match_
    layout_spec pins the GPU build to): every inserted X passes, and random X's pass at about the
    fill-implied rate only."""
    import ctypes
    rng = random.Random(5)
    blocks = 64
    model = bytearray(256 * blocks * 16)

    def words(xb):
        return blk_spec_bits(xb, blocks)

    ins = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(3000)]
    for xb in ins:
        for off, bit in words(xb):
            model[off] |= bit
    buf = ctypes.create_string_buffer(bytes(model), len(model))
    chk = oracle.lib().or_blk_check
    assert all(chk(buf, ctypes.c_uint64(blocks), xb) == 1 for xb in ins)
    rnd = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(20000)]
    hits = sum(chk(buf, ctypes.c_uint64(blocks), xb) for xb in rnd)
    # a random X passes iff all 16 of its bits are set: the model says so too
    exp = sum(all(model[o] & b for o, b in words(xb)) for xb in rnd)
    assert hits == exp and hits < 200


@pytest.mark.parametrize("blocked", [False, True], ids=["reference", "blocked"])
def test_oracle_candidates_equal_scan_candidates(oracle, blocked):
    """BsgsTables.candidates (or_bsgs_l1_candidates: the walk and the layer-1 probe alone) lists what
    scan() lists, in both layer-1 layouts: n = 2^24, k = 3 (overlapping bases) over 8 bases = 16384
    giant points, a far target, and a layer 1 made dense enough (built bits OR random ones, ~2 % of
    points pass) for a few hundred candidates."""
    from _dense_layer import dense_layer
    p = oracle.bsgs_params(1 << 24, 3)
    t = oracle.BsgsTables(p)
    blocks = (p.bits[0] * 3 + 127) // 128 if blocked else 0
    built = bytes(256 * 16 * blocks) if blocked else t.bf1.raw
    l1 = dense_layer(built, 0.02, blocked, p.hashes[0], seed=24 + blocked)
    tabs = oracle.BsgsTables.from_raw(p, l1, t.bf2.raw, t.bf3.raw, t.table_bytes(), l1_blocks=blocks)
    start = 0x6B6B6B6B0000000
    q = oracle.pubkey(start - 99991 * 2 * p.n)          # far: no base holds it
    key, via_scan = tabs.scan(start, 8, q)
    assert key is None
    cands = tabs.candidates(start, 8, q)
    assert cands == via_scan
    assert 200 <= len(cands) <= 500                     # 16384 x 2 % = 328
    assert {b for b, _ in cands} == set(range(8)) and max(a for _, a in cands) < p.cycles * 1024
    with pytest.raises(OverflowError):
        tabs.candidates(start, 8, q, cap=len(cands) - 1)
