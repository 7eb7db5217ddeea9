"""The kangaroo search on the GPU against the model of _kangaroo.py: placement, the table, solves that equal
the model's count for count, solves at a useful size, and the other modes' independence of it."""
import math
import os

import pytest

import _kangaroo as K
import keyhunt_amd
from conftest import DATA
from keyhunt_amd import engine as E
from test_kangaroo_model import SEEDS, W24, planted

pytestmark = pytest.mark.gpu
ORDER = K.ORDER


@pytest.fixture
def kang(engine):
    """The session's engine with the automatic launch size, before and after."""
    engine.kang_set_launch(0)
    yield engine
    engine.kang_set_launch(0)


def herd_sizes(B):
    return [1, 2, 63, 64 * B - 1, 64 * B + 1, 2 * 256 * B + 5]


# the three ranges of the placement test: a = 1; a with high limbs set; b two below the order
RANGES = [(1, 1 + W24), ((0xDEADBEEF << 200) + (0x1234 << 130) + 99, (0xDEADBEEF << 200) + (0x1234 << 130) + 99 + (1 << 40)),
          (ORDER - 2 - (1 << 30), ORDER - 2)]


def dists_for(n, W, salt):
    """Arbitrary distances below 2 W for kangaroos 0 .. n-1, none of them 0."""
    return [1 + K._h(b"dist" + bytes([salt]) + i.to_bytes(4, "little")) % (2 * W) for i in range(n)]


def check_herd(e, model):
    got = e.kang_get_herd(0, len(model.k))
    want = model.state()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if w[0] is None:
            assert g[2] == w[2], i
        else:
            assert g == w, i


@pytest.mark.parametrize("size_index", range(6))
def test_placement_equals_the_model(kang, size_index):
    a, b = RANGES[size_index % 3]
    key = a + (b - a) // 3
    B = kang.kang_setup(K.pub_of(key), a, b, 4)
    n = herd_sizes(B)[size_index]
    m = K.Herd(K.pub_of(key), a, b, 4)
    assert kang.kang_jumps() == m.jd
    d = dists_for(n, b - a, size_index)
    # in two calls, the second starting at an odd index when there is room
    cut = min(n, 33)
    kang.kang_set_herd(n, 0, d[:cut])
    if cut < n:
        kang.kang_set_herd(n, cut, d[cut:])
    m.set_herd(n, 0, d)
    check_herd(kang, m)
    assert kang.kang_seed(11, n) == n
    m.seed_herd(11, n)
    for i, st in enumerate(m.k):
        lo, hi = (1, b - a) if i & 1 else ((b - a) // 2, (b - a) // 2 + (b - a))
        assert lo <= st[1] <= hi
    check_herd(kang, m)


def test_setup_refusals(kang):
    pub = K.pub_of(12345)
    S = kang.kang_setup_status
    assert S(pub, 1, 1 + (1 << 16) - 1) == E.KH_E_RANGE           # W < 2^16
    assert S(pub, 1, 1 + (1 << 16)) == 0
    assert S(pub, 1, 1 + (1 << 192)) == E.KH_E_RANGE              # W >= 2^192
    assert S(pub, 1, (1 << 192)) == 0
    assert S(pub, ORDER - (1 << 20), ORDER) == E.KH_E_RANGE       # b reaches the order
    assert S(pub, ORDER - (1 << 20), ORDER - 2) == 0
    assert S(pub, 100000, 1) == E.KH_E_RANGE
    assert S((pub[0], pub[1] ^ 1), 1, 1 << 20) == E.KH_E_ARG      # not on the curve
    assert S(pub, 1, 1 << 20, 33) == E.KH_E_ARG
    assert S(pub, 1, 1 << 20, 4, [1] * 31 + [0]) == E.KH_E_ARG
    assert S(pub, 1, 1 << 20, 4, [1] * 31 + [1 << 128]) == E.KH_E_ARG
    assert S(pub, 1, 1 << 20, 4) == 0
    assert kang.kang_set_herd_status(4, 0, [0, 5]) == E.KH_E_ARG  # a tame at distance 0
    assert kang.kang_set_herd_status(4, 3, [5, 5]) == E.KH_E_ARG  # first + n > total
    assert kang.kang_set_herd_status(4, 1, [0, 5]) == 0           # a wild at distance 0 is Q' itself
    m = K.Herd(pub, 1, 1 << 20, 4)
    assert kang.kang_get_herd(1, 1)[0][:2] == m.qp


def test_calls_before_setup_refuse():
    with keyhunt_amd.Engine(0) as e:
        L = keyhunt_amd.lib()
        import ctypes
        n32, n64, key = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.create_string_buffer(32)
        assert L.kh_kang_step(e._ctx, 1, None, 0, ctypes.byref(n32), ctypes.byref(n64)) == E.KH_E_STATE
        assert L.kh_kang_seed(e._ctx, 0, 0) == E.KH_E_STATE
        assert L.kh_kang_solve(e._ctx, 1, key, ctypes.byref(n32), None) == E.KH_E_STATE
        assert L.kh_kang_set_herd(e._ctx, 2, 0, 0, None) == E.KH_E_STATE
        assert e.kang_geometry()[2] == 0
        # set up, then released: the same again
        e.kang_setup(K.pub_of(777777), 1, 1 << 24, 2)
        assert e.kang_seed(1, 64) == 64
        e.release_walk()
        assert L.kh_kang_step(e._ctx, 1, None, 0, ctypes.byref(n32), ctypes.byref(n64)) == E.KH_E_STATE


def stats_of(e):
    st = e.kang_solve(0)[1]
    return {f: getattr(st, f) for f in ("jumps", "dps", "same_herd", "reseeds", "stalls", "bad")}


@pytest.mark.parametrize("sign", ["t-w", "-(t+w)"])
def test_table_resolves_a_collision_of_either_sign(kang, sign):
    a, kp = 5, 0xC0FFEE
    pub = K.pub_of(a + kp)
    kang.kang_setup(pub, a, a + W24, 2)
    kang.kang_seed(1, 64)
    if sign == "t-w":
        t, w = kp + 4242, 4242
    else:
        w = 31337
        t = ORDER - kp - w
    x = 0x1234567890ABCDEF << 100
    assert kang.kang_add_dps([(x, t, 6, K.TAME)]) is None
    assert kang.kang_add_dps([(x + 1, w, 7, K.WILD)]) is None  # another x: no collision
    assert kang.kang_add_dps([(x, w, 9, K.WILD)]) == a + kp
    st = stats_of(kang)
    assert (st["dps"], st["bad"], st["same_herd"], st["reseeds"]) == (3, 0, 0, 0)
    assert kang.kang_solve(1 << 30)[0] == a + kp  # known already: nothing runs
    assert stats_of(kang)["jumps"] == 0


def test_table_same_herd_and_bad_collisions(kang):
    a, kp = 5, 0xC0FFEE
    pub = K.pub_of(a + kp)
    kang.kang_setup(pub, a, a + W24, 2)
    kang.kang_seed(3, 64)
    m = K.Herd(pub, a, a + W24, 2)
    m.seed_herd(3, 64)
    x = 0xFEDCBA << 180
    recs = [(x, 1000, 8, K.TAME), (x, 2000, 4, K.TAME)]  # fed out of order: index 4 comes first, 8 is the later one
    assert kang.kang_add_dps(recs) is None
    assert m.add_dps(recs) is None
    assert m.gen[8] == 1 and m.gen[4] == 0
    check_herd(kang, m)
    want = dict(jumps=0, dps=2, same_herd=1, reseeds=1, stalls=0, bad=0)
    assert stats_of(kang) == want == m.stats
    # a wild on the same x whose distance fits neither candidate
    bad = [(x, 77, 5, K.WILD)]
    assert kang.kang_add_dps(bad) is None and m.add_dps(bad) is None
    want.update(dps=3, bad=1)
    assert stats_of(kang) == want == m.stats
    check_herd(kang, m)


def solve_case(e, seed, spl):
    a, W = 1, W24
    key = planted(seed, a, W)
    e.kang_set_launch(spl)
    e.kang_setup(K.pub_of(key), a, a + W, 2)
    assert e.kang_seed(seed, 64) == 64
    spl_used = e.kang_geometry()[1]
    m = K.Herd(K.pub_of(key), a, a + W, 2)
    m.seed_herd(seed, 64)
    bound = 16 * math.isqrt(W)
    assert m.solve(bound, spl_used) == key
    got, st = e.kang_solve(bound)
    assert got == key
    print(f"seed {seed} spl {spl_used}: {m.stats}")
    assert {f: getattr(st, f) for f in m.stats} == m.stats
    assert st.lost == 0 and st.jumps <= bound
    check_herd(e, m)


@pytest.mark.parametrize("seed", SEEDS)
def test_solve_equals_the_model(kang, seed):
    solve_case(kang, seed, 8)


def test_solve_equals_the_model_at_the_automatic_launch_size(kang):
    solve_case(kang, SEEDS[0], 0)
    assert kang.kang_geometry()[1] == 2  # 16 * 64 * 4 = 4096 > sqrt(2^24 - 1) >= 16 * 64 * 2


HERD40, DP40 = 1 << 12, 4


def solve40(e, pub, a, b, seed=1, herd=HERD40):
    e.kang_setup(pub, a, b, DP40)
    e.kang_seed(seed, herd)
    W = b - a
    bound = 16 * math.isqrt(W) + 4 * herd * (1 << DP40)
    key, st = e.kang_solve(bound)
    print(f"W 2^{W.bit_length()}: jumps {st.jumps} = {st.jumps / math.isqrt(W):.2f} sqrt(W), dps {st.dps}")
    assert st.jumps <= bound
    assert st.bad == 0 and st.lost == 0
    return key, st


def test_solve_puzzle_63(kang):
    line = open(os.path.join(DATA, "63.pub")).read().split()[0]
    x = int(line[2:], 16)
    y = pow(x ** 3 + 7, (K.P + 1) // 4, K.P)
    if (y & 1) != (int(line[:2], 16) & 1):
        y = K.P - y
    key, _ = solve40(kang, (x, y), 0x7CCE5E0000000000, 0x7CCE5EFFFFFFFFFF)
    assert key == 0x7CCE5EFDACCF6808


A40 = (0xA5A5 << 150) + 12345


@pytest.mark.parametrize("off", [0, 1, (1 << 40), 0x123456789, (1 << 39) + 1, (1 << 40) - 77])
def test_solve_planted_keys_in_a_40_bit_range(kang, off):
    a, b = A40, A40 + (1 << 40)
    key, st = solve40(kang, K.pub_of(a + off), a, b)
    assert key == a + off
    if off == 0:
        assert st.jumps == 0 and kang.kang_geometry()[2] == 0  # found by setup: no herd, nothing launched


def test_solve_continues_across_calls(kang):
    a, b = A40, A40 + (1 << 40)
    key = a + 0x7777777777
    one, st1 = solve40(kang, K.pub_of(key), a, b, seed=9)
    assert one == key
    kang.kang_setup(K.pub_of(key), a, b, DP40)
    kang.kang_seed(9, HERD40)
    got, st = kang.kang_solve(1)  # one launch: too little
    assert got is None and 0 < st.jumps < st1.jumps
    got, st = kang.kang_solve(1 << 40)
    assert got == key
    assert (st.jumps, st.dps, st.same_herd, st.reseeds) == (st1.jumps, st1.dps, st1.same_herd, st1.reseeds)


def test_other_modes_are_independent_of_a_solve(kang, oracle):
    def others(e):
        keys = [1, 3, 7, 8, 21, 49, 76, 224, 467, 514, 1155, 2683, 5216, 10544, 26867, 51510]
        rows = []
        for k in keys:
            x, y = oracle.pubkey(k)
            rows.append(oracle.hash160_comp(x, 2 + (y & 1)))
        e.set_targets(rows)
        hits = [(h.key, h.compressed, h.kind) for h in e.scan(1, 1 << 16, E.KH_MODE_ADDRESS, E.KH_SEARCH_COMPRESS)]
        p = oracle.bsgs_params(1 << 20, 1)
        e.bsgs_setup(1 << 20, 1)
        e.bsgs_build()
        key = 0x1234567890ABCDEF
        e.bsgs_set_targets([oracle.pubkey(key)])
        return hits, e.bsgs_scan(key - 5 * 2 * p.n - 777, 8)

    with keyhunt_amd.Engine(0) as fresh:
        want = others(fresh)
    assert len(want[0]) == 16 and want[1] == [(0, 0x1234567890ABCDEF)]
    kang.kernel_time_reset()
    a, key = 1, planted(2, 1, W24)
    kang.kang_setup(K.pub_of(key), a, a + W24, 2)
    kang.kang_seed(2, 64)
    got, st = kang.kang_solve(1 << 20)
    assert got == key
    launches, ms, points = kang.kernel_time(E.TIME_KANG)
    assert launches > 0 and ms > 0 and points == st.jumps
    assert others(kang) == want
    assert others(kang) == want
