"""Target rows for the dense -e / --rmd-batch-size tests (tests/test_gpu_endo_dense.py), in closed form.

A walk probes a point S = (x, y) under a set of image classes, each a (hash, e, s) triple: the hash of
(beta^e x, y) -- "c" hash160(02/03||X) with prefix 2 + s, "u" hash160(04||X||Y) and "eth"
Keccak(X||Y)[12:] with Y negated when s, "x" the X prefix -- reported with kind base | e << 4 | s << 6
("c": base s, no sign bit).  CLASSES lists them per case in the reference's probe order per point
(keyhunt.cpp:3476-3536, 3767-3808); -c eth -e has five distinct images, its slot 4 repeating (beta x, y)
(reported as 5 | 2 << 4, TWIN).  Rows come from the point and x * beta^e mod p alone: no lambda."""
P = 2**256 - 2**32 - 977
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
BETAS = (1, BETA, BETA * BETA % P)
ETH_BETA, TWIN = 0x15, 0x25  # eth(beta S) and its repeated slot-4 record

_C = [("c", e, s) for e in range(3) for s in range(2)]
_U = [("u", e, s) for e in range(3) for s in range(2)]
# case -> (engine/oracle mode, search, -e, classes)
CASES = {
    "compress_e": (0, 0, True, _C),
    "uncompress_e": (0, 1, True, _U),
    "both_e": (0, 2, True, _C + _U),
    "xpoint_e": (1, 2, True, [("x", e, 0) for e in range(3)]),
    "eth_e": (2, 2, True, [("eth", 0, 0), ("eth", 0, 1), ("eth", 1, 0), ("eth", 1, 1), ("eth", 2, 1)]),
    "both": (0, 2, False, [("c", 0, 0), ("c", 0, 1), ("u", 0, 0)]),
    "eth": (2, 2, False, [("eth", 0, 0)]),
}


def kind_of(cls):
    h, e, s = cls
    if h == "c":
        return s | e << 4
    return {"u": 2, "x": 3, "eth": 5}[h] | e << 4 | s << 6


def survives_without_e(cls):
    """Without -e the walk probes 02, 03 and the point's own 04 / eth / x only."""
    h, e, s = cls
    return e == 0 and (h == "c" or s == 0)


def row(oracle, cls, pt):
    h, e, s = cls
    x, y = pt
    xe = x * BETAS[e] % P
    if h == "c":
        return oracle.hash160_comp(xe, 2 + s)
    if h == "x":
        return xe.to_bytes(32, "big")[:20]
    ye = (P - y) % P if s else y
    return oracle.hash160_uncomp(xe, ye) if h == "u" else oracle.eth_address(xe, ye)


def plant(oracle, classes, slots):
    """slots: (offset, point, class index or None for every class).  Returns (rows, planted): the
    de-duplicated target rows in planting order and the (offset, kind) pairs that must be hit."""
    rows, planted = [], []
    for off, pt, c in slots:
        for cls in (classes if c is None else [classes[c]]):
            rows.append(row(oracle, cls, pt))
            planted.append((off, kind_of(cls)))
    return list(dict.fromkeys(rows)), planted


def zinv_point(centre, mult, G, t):
    """The point the reference's group of G < 1024 slots holds at slot t: its centre at G/2, else
    x = -(C.x + ((i+1)D).x), y = -+((i+1)D).y for the slots G/2 +- (i+1); mult[i] = (i+1)D."""
    half = G // 2
    if t == half:
        return centre
    i = t - half - 1 if t > half else half - t - 1
    tx, ty = mult[i]
    return (-(centre[0] + tx)) % P, (P - ty) % P if t > half else ty


def triples(hits):
    """(key, compressed, kind) per engine hit, as oracle.scan_chunk lists them."""
    return [(h.key, bool(h.compressed), int(h.kind)) for h in hits]


def check_hits(got, ref, planted, kinds):
    """The engine's hit list `got` equals the oracle's `ref` -- keys, compressed flags, kinds and order
    -- every planted (offset, kind) is among its records, every kind of `kinds` occurs, and in
    -c eth -e every eth(beta S) record has its slot-4 twin at the same offset."""
    g = triples(got)
    if g != ref:
        n = next((i for i, (a, b) in enumerate(zip(g, ref)) if a != b), min(len(g), len(ref)))
        raise AssertionError(f"{len(g)} engine hits, {len(ref)} oracle hits; first difference at record {n}: "
                             f"engine {g[n:n + 2]} (offsets {[h.offset for h in got[n:n + 2]]}), oracle {ref[n:n + 2]}")
    have = {(h.offset, int(h.kind)) for h in got}
    missing = sorted(set(planted) - have)
    assert not missing, f"{len(missing)} planted (offset, kind) not hit: {missing[:8]}"
    assert {k for _, k in have} >= set(kinds), sorted(set(kinds) - {k for _, k in have})
    if ETH_BETA in kinds:
        assert sorted(o for o, k in have if k == TWIN) == sorted(o for o, k in have if k == ETH_BETA)
        assert sum(1 for h in got if h.kind == TWIN) == sum(1 for h in got if h.kind == ETH_BETA)
