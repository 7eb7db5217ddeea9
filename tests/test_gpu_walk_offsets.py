"""The sequential walks (kh_scan) pinned at every in-group offset by planted keys.

The other scan tests plant a few dozen keys in a chunk; a walk that is wrong at one of a group's 4096
(or 1024) offsets -- the drain of its deferred probes, the last pair, the centre, C + (H-1) -- passes
them unless a key happens to sit there.  Here every in-group offset o holds exactly one key,
key_o = start + g_o*G + o, with g_o a seeded permutation over the chunk's groups, so the offsets spread
over lanes and over a lane's successive groups; the chunk's first and last key are planted too.  The
hits must be exactly these keys, once each.  Expected values come from the oracle's pubkey / hashes; no
oracle scan is needed."""
import random

import pytest

pytestmark = pytest.mark.gpu

START_BIG = (1 << 67) + 0x1D2C3B4A59687       # 4096-point groups: n_keys = 2^24 = 4096 groups
N_BIG, G_BIG = 1 << 24, 4096
START_SMALL = (1 << 66) + 0x0F1E2D3C4B5A6     # 1024-point groups: 1025 of them (no multiple of 4096 keys)
N_SMALL, G_SMALL = 1025 * 1024, 1024


def _planted(start, n_keys, G, seed):
    groups = list(range(n_keys // G))
    random.Random(seed).shuffle(groups)
    assert len(groups) >= G
    offs = {groups[o] * G + o for o in range(G)} | {0, n_keys - 1}
    assert sorted({o % G for o in offs}) == list(range(G))
    return [start + o for o in sorted(offs)]


@pytest.fixture(scope="module")
def planted(oracle):
    """Keys and their target rows by kind, computed once for the module."""
    out = {}
    for name, (start, n, G, seed) in {"big": (START_BIG, N_BIG, G_BIG, 4096),
                                      "small": (START_SMALL, N_SMALL, G_SMALL, 1024)}.items():
        keys = _planted(start, n, G, seed)
        pts = [oracle.pubkey(k) for k in keys]
        rows = {"x": [x.to_bytes(32, "big")[:20] for x, _ in pts],
                "comp": [oracle.hash160_comp(x, 2 + (y & 1)) for x, y in pts]}
        if name == "small":
            rows["uncomp"] = [oracle.hash160_uncomp(x, y) for x, y in pts]
            # -l both probes the compressed and the uncompressed hash: alternate them over the offsets
            rows["both"] = [rows["comp"][i] if (k - start) % 2 == 0 else rows["uncomp"][i] for i, k in enumerate(keys)]
            rows["eth"] = [oracle.eth_address(x, y) for x, y in pts]
        out[name] = (keys, rows)
    return out


@pytest.fixture(scope="module")
def engine512():
    """512 lanes: a lane walks several groups of the chunk in turn (the default geometry gives every
    group of these chunks a lane of its own)."""
    import keyhunt_amd
    with keyhunt_amd.Engine(0, 512, 0) as e:
        yield e


@pytest.fixture(params=["default", "lanes512"])
def eng(request, engine, engine512):
    return engine if request.param == "default" else engine512


def _scan_and_check(e, keys, rows, start, n_keys, mode, search):
    e.set_targets(rows)
    got = e.scan(start, n_keys, mode=mode, search=search, cap=2 * len(keys))
    found = sorted(h.key for h in got)
    if found != keys:
        want, have = set(keys), set(found)
        G = G_BIG if n_keys == N_BIG else G_SMALL
        miss, extra = sorted(want - have), sorted(have - want)
        dup = sorted({k for k in found if found.count(k) > 1})[:12] if len(found) != len(have) else []
        raise AssertionError(f"missing {len(miss)} (offsets in group {[(k - start) % G for k in miss[:16]]}), "
                             f"extra {len(extra)} {[hex(k) for k in extra[:8]]}, twice {[(k - start) % G for k in dup]}")
    assert len(got) == len(keys)


@pytest.mark.parametrize("ref_bloom", [False, True], ids=["blocked_filter", "reference_bloom"])
@pytest.mark.parametrize("kind", ["x", "comp"], ids=["xpoint", "compress"])
def test_large_groups_every_offset(eng, planted, monkeypatch, kind, ref_bloom):
    """2^24 keys in 4096-point groups (H = 2048): xpoint with exact targets (k_walk<KM_XPOINTB>, its
    whole-wave fast path and the group at the chunk's end) and -l compress (k_walk<KM_H160CB>); with
    KH_REF_TARGET_BLOOM=1 the reference-layout probes (k_walk<KM_XPOINT>, k_walk<KM_H160C>)."""
    if ref_bloom:
        monkeypatch.setenv("KH_REF_TARGET_BLOOM", "1")
    else:
        monkeypatch.delenv("KH_REF_TARGET_BLOOM", raising=False)
    keys, rows = planted["big"]
    assert len(keys) in (G_BIG + 1, G_BIG + 2)
    _scan_and_check(eng, keys, rows[kind], START_BIG, N_BIG, 1 if kind == "x" else 0, 0)


@pytest.mark.parametrize("kind,mode,search", [("uncomp", 0, 1), ("both", 0, 2), ("eth", 2, 2), ("x", 1, 2)],
                         ids=["uncompress", "both", "eth", "xpoint"])
def test_small_groups_every_offset(eng, planted, kind, mode, search):
    """1025 x 1024 keys in the reference's 1024-point groups (H = 512): -l uncompress, -l both, -c eth
    and xpoint (a chunk that is no multiple of 4096 keys)."""
    keys, rows = planted["small"]
    assert len(keys) in (G_SMALL + 1, G_SMALL + 2)
    _scan_and_check(eng, keys, rows[kind], START_SMALL, N_SMALL, mode, search)
