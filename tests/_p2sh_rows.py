"""Target rows for the dense KH_MODE_P2SH tests (tests/test_gpu_p2sh_dense.py), in closed form.

The image classes of tests/_endo_rows.py, (hash, e, s), take a fourth field nest: with KH_MODE_P2SH a walk
probes every compressed digest h as without the flag and then its nested form hash160(00 14 || h), the
P2SH-P2WPKH script hash (BIP-49), reported with KH_KIND_P2SH (0x80) or-ed into the plain hit's kind.  Only
"c" classes nest: a segwit key is compressed by rule.  Rows come from the oracle's hash160, SHA-256 and
RIPEMD-160 alone."""
from _endo_rows import _C, _U, kind_of, row, survives_without_e

KIND_P2SH = 0x80
MODE_ADDRESS, MODE_P2SH = 0, 0x20
COMPRESS, BOTH = 0, 2


def _nest(classes):
    return [c + (nest,) for c in classes for nest in (0, 1)]


def _flat(classes):
    return [c + (0,) for c in classes]


# case -> (search, -e, classes): KH_MODE_ADDRESS | KH_MODE_P2SH throughout
CASES = {
    "compress": (COMPRESS, False, _nest([("c", 0, 0), ("c", 0, 1)])),
    "both": (BOTH, False, _nest([("c", 0, 0), ("c", 0, 1)]) + [("u", 0, 0, 0)]),
    "compress_e": (COMPRESS, True, _nest(_C)),
    "both_e": (BOTH, True, _nest(_C) + _flat(_U)),
}
assert [len(c[2]) for c in CASES.values()] == [4, 5, 12, 18]


def nested(oracle, h):
    """hash160 of the witness script 00 14 || h."""
    return oracle.ripemd160(oracle.sha256(b"\x00\x14" + h))


def plain_row(oracle, cls, pt):
    """The un-nested row of the class: what the reference's own probes compute."""
    return row(oracle, cls[:3], pt)


def row4(oracle, cls, pt):
    r = plain_row(oracle, cls, pt)
    if not cls[3]:
        return r
    assert cls[0] == "c"
    return nested(oracle, r)


def kind4(cls):
    return kind_of(cls[:3]) | (KIND_P2SH if cls[3] else 0)


def survives4(cls):
    """Without -e: image 0 alone, plain or nested."""
    return survives_without_e(cls[:3])


def records(hits):
    """(key, compressed, kind) per engine hit, as oracle.scan_chunk lists them."""
    return [(h.key, bool(h.compressed), int(h.kind)) for h in hits]


def first_difference(got, want):
    g, w = records(got), list(want)
    if g == w:
        return None
    n = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
    return (f"{len(g)} engine hits, {len(w)} expected; first difference at record {n}: engine {g[n:n + 2]} "
            f"(offsets {[h.offset for h in got[n:n + 2]]}), expected {w[n:n + 2]}")
