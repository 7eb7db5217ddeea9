"""The kangaroo search at the widths it exists for, against the model of _kangaroo.py: default tables, seeding
and walks at 64 to 192 bits (every limb of a jump distance, the host's 256-bit shifts and remainders across
their word boundaries), carries through every limb of the distance, distances at and above the group order,
a stall met in the middle of a launch, the placement passes of herds beyond 2^20, and planted collisions
that drive wide distances through records, sort, table and resolution.  Every precondition a case rests on
is asserted on the model, so a change of seed or table that keeps a case from its edge fails here."""
import collections
import copy

import pytest

import _kangaroo as K
from keyhunt_amd import engine as E
from test_gpu_kangaroo import check_herd, dists_for, herd_sizes, kang  # noqa: F401 (fixture)
from test_gpu_kangaroo_dense import same_records

pytestmark = pytest.mark.gpu
ORDER = K.ORDER
M32 = (1 << 32) - 1
A_HIGH = (0xDEADBEEF << 200) + (0x1234 << 130) + 99
_PUBS = {}


def pub_of(k):
    if k not in _PUBS:
        _PUBS[k] = K.pub_of(k)
    return _PUBS[k]


def carries(dist: int, d: int) -> list[int]:
    """c[k], k = 0..7: the carry that the 8 x 32-bit addition dist + d takes into limb k (c[0] = 0)."""
    return [((dist & ((1 << 32 * k) - 1)) + (d & ((1 << 32 * k) - 1))) >> (32 * k) for k in range(8)]


def limb(v: int, w: int) -> int:
    return (v >> (32 * w)) & M32


# ---- 1. default tables, seeding and walk at wide W -------------------------------------------------
BITLENS = [64, 65, 70, 127, 128, 129, 191, 192]
JB = [33, 33, 36, 64, 65, 65, 96, 97]
STEPS = (1, 2, 5, 33)  # in launches of 4: 5 crosses a launch boundary once, 33 eight times


def width(bl: int) -> int:
    """The top bit and arbitrary lower bits in every word; 2^192 - 1, the largest width accepted, at 192."""
    if bl == 192:
        return (1 << 192) - 1
    return (1 << (bl - 1)) + (K._h(b"wide" + bytes([bl])) % (1 << (bl - 1)) or 1)


def start_of(bl: int, W: int) -> int:
    """a = 1; a with bits above 2^200; b = ORDER - 2: rotated over the widths."""
    return [1, A_HIGH, ORDER - 2 - W][BITLENS.index(bl) % 3]


WideCase = collections.namedtuple("WideCase", "pub a W seeded recs walked")
_WIDE = {}


def wide_case(bl: int, n: int) -> WideCase:
    """The model seeded with n kangaroos (seed 21) in a range of bit length bl, then walked through STEPS in
    launches of 4 with dp 0; computed once per (bl, n)."""
    if (bl, n) in _WIDE:
        return _WIDE[bl, n]
    W = width(bl)
    assert W.bit_length() == bl and W & (W - 1)
    a = start_of(bl, W)
    assert 0 < a and a + W < ORDER
    pub = pub_of(a + W // 3)
    m = K.Herd(pub, a, a + W, 0)
    m.seed_herd(21, n)
    assert all(st[0] is not None for st in m.k)
    seeded = copy.deepcopy(m)
    words, into = set(), set()

    def see(index, j, dist):
        words.update(w for w in range(4) if limb(m.jd[j], w))
        into.update(k for k, c in enumerate(carries(dist, m.jd[j])) if c)

    m.on_jump = see
    recs = [m.step(s, 4) for s in STEPS]
    m.on_jump = None
    assert all(len(r) == n * s for r, s in zip(recs, STEPS))
    # the edges this width is here for
    if bl == 192:
        assert 3 in words
    if bl >= 128:
        assert 2 in words
    if bl >= 191:
        assert 3 in into
    if bl >= 127:
        assert 2 in into
    assert 1 in into and max(into) <= 3
    _WIDE[bl, n] = WideCase(pub, a, W, seeded, recs, m)
    return _WIDE[bl, n]


def test_the_widths_cover_every_word_boundary():
    assert [width(bl).bit_length() // 2 + 1 for bl in BITLENS] == JB
    assert width(192) == (1 << 192) - 1
    starts = [start_of(bl, width(bl)) for bl in BITLENS]
    assert starts[0] == 1 and starts[1] >> 200 and starts[2] + width(BITLENS[2]) == ORDER - 2


@pytest.mark.parametrize("bl", BITLENS)
def test_default_jump_table_at_wide_ranges(kang, bl):
    W = width(bl)
    a = start_of(bl, W)
    kang.kang_setup(pub_of(a + W // 3), a, a + W, 0)
    want = K.default_jumps(W)
    jb = JB[BITLENS.index(bl)]
    assert len(set(want)) == 32 and max(want).bit_length() == jb  # the model's table reaches its top bit
    assert kang.kang_jumps() == want


@pytest.mark.parametrize("bl,full", [(bl, False) for bl in BITLENS] + [(70, True), (192, True)])
def test_seed_and_walk_at_wide_ranges(kang, bl, full):
    B = kang.kang_geometry()[0]
    n = herd_sizes(B)[4 if full else 2]  # 64 B + 1: a second block of one lane; 63: short of a wave
    c = wide_case(bl, n)
    kang.kang_set_launch(4)
    kang.kang_setup(c.pub, c.a, c.a + c.W, 0)
    assert kang.kang_seed(21, n) == n
    check_herd(kang, c.seeded)
    for steps, want in zip(STEPS, c.recs):
        recs, lost = kang.kang_step(steps, n * steps)
        assert lost == 0
        same_records(recs, want)
    check_herd(kang, c.walked)


# ---- 2. carries through every limb of the distance (a table of the test's own) -------------------
EDGE_JUMPS = [(1 << 128) - 1, (1 << 128) - (1 << 32), (1 << 128) - (1 << 96), 1 << 127, (1 << 97) - 1,
              (1 << 96) + (1 << 32) - 1, 1 << 96, (1 << 96) - 1, (1 << 65) - 1, (1 << 64) + 1, 1 << 64, (1 << 64) - 1,
              (1 << 33) - 1, 1 << 32, (1 << 32) - 1, 1]
EDGE_DISTS = [(1 << 128) - 1, (1 << 160) - 1, (1 << 192) - 1, (1 << 224) - 1, (1 << 255) - 1, (1 << 256) - (1 << 140)]
CARRY_STEPS = 12
_CARRY = []


def carry_dist(i: int) -> int:
    """Limbs 4 .. k-1 all ones for k = 4 + i mod 4, the rest hashed, the top limb below 2^31; every second
    group of four has one of its low four limbs all ones as well."""
    h = K._h(b"carry-dist" + i.to_bytes(4, "little"))
    limbs = [limb(h, w) for w in range(8)]
    for w in range(4, 4 + i % 4):
        limbs[w] = M32
    limbs[7] &= (1 << 31) - 1
    if i & 4:
        limbs[(i >> 3) & 3] = M32
    return sum(v << (32 * w) for w, v in enumerate(limbs))


def carry_case(B: int):
    """(pub, a, W, jumps, dists, the model placed, its records of 12 jumps, the model walked)."""
    if _CARRY:
        return _CARRY[0]
    jumps = []
    for j in range(16):
        jumps += [(1 << 127) | (K._h(b"carry-jump" + bytes([j])) % (1 << 127)), EDGE_JUMPS[j]]
    assert len(set(jumps)) == 32 and all(0 < d < (1 << 128) for d in jumps)
    n = 2 * 64 * B + 1
    dists = [carry_dist(i) for i in range(n)]
    for q, d in enumerate(EDGE_DISTS):  # a tame and a wild at each, spread over lanes and batch slots
        dists[2 * (331 * q + 29)] = dists[2 * (331 * q + 29) + 1] = d
    limit = (1 << 256) - (1 << 140)
    assert all(0 < d <= limit and d % ORDER for d in dists)
    a, W = A_HIGH, (1 << 100) + 7
    pub = pub_of(a + W // 3)
    m = K.Herd(pub, a, a + W, 0, jumps)
    m.set_herd(n, 0, dists)
    assert all(st[0] is not None for st in m.k)
    placed = copy.deepcopy(m)
    taken, into, ripple = set(), collections.Counter(), collections.Counter()

    def see(index, j, dist):
        taken.add(j)
        c = carries(dist, jumps[j])
        into.update(k for k in range(1, 8) if c[k])
        for k in range(5, 8):
            # out of limb 3 and through the all-ones limbs 4 .. k-1 into limb k
            if all(c[4:k + 1]) and all(limb(dist, w) == M32 for w in range(4, k)):
                ripple[k] += 1

    m.on_jump = see
    recs = m.step(CARRY_STEPS, 4)
    m.on_jump = None
    assert len(recs) == n * CARRY_STEPS
    assert taken == set(range(32))
    assert all(into[k] > 0 for k in range(1, 8)), into
    assert all(ripple[k] > 0 for k in range(5, 8)), ripple
    assert max(st[1] for st in m.k) < (1 << 256)
    print("carries into limbs 1..7:", [into[k] for k in range(1, 8)], "ripples into 5..7:", [ripple[k] for k in (5, 6, 7)])
    _CARRY.append((pub, a, W, jumps, dists, placed, recs, m))
    return _CARRY[0]


def test_carries_through_every_limb_of_the_distance(kang):
    B = kang.kang_geometry()[0]
    pub, a, W, jumps, dists, placed, want, walked = carry_case(B)
    n = len(dists)
    kang.kang_set_launch(4)
    kang.kang_setup(pub, a, a + W, 0, jumps)
    assert kang.kang_jumps() == jumps
    kang.kang_set_herd(n, 0, dists)
    check_herd(kang, placed)
    recs, lost = kang.kang_step(CARRY_STEPS, n * CARRY_STEPS)
    assert lost == 0
    same_records(recs, want)
    check_herd(kang, walked)


# ---- 3. placement of distances at and above the group order -----------------------------------------
def test_placement_at_and_above_the_group_order(kang):
    a, W = A_HIGH, width(70)
    pub = pub_of(a + W // 3)
    kang.kang_setup(pub, a, a + W, 4)
    m = K.Herd(pub, a, a + W, 4)
    n = 131
    d = dists_for(n, W, 7)
    tames = {4: ORDER - 1, 40: ORDER + 1, 100: (1 << 256) - 1}
    wilds = {5: ORDER - 1, 41: ORDER, 77: ORDER + 1, 101: (1 << 256) - 1}
    for e, v in list(tames.items()) + list(wilds.items()):
        d[e] = v
    kang.kang_set_herd(n, 0, d)
    m.set_herd(n, 0, d)
    assert all(st[0] is not None for st in m.k)
    assert m.k[41][0] == m.qp and m.k[4][0] == K.neg(K.mul_g(1)) and m.k[40][0] == K.mul_g(1)
    assert m.k[100][0] == K.mul_g((1 << 256) - 1 - ORDER)
    check_herd(kang, m)
    assert [g[2] for g in kang.kang_get_herd(0, n)] == d  # as given, unreduced


def test_a_tame_at_a_multiple_of_the_order_is_refused(kang):
    a, W = 1, width(65)
    pub = pub_of(a + W // 3)
    kang.kang_setup(pub, a, a + W, 4)
    assert kang.kang_seed(3, 64) == 64
    m = K.Herd(pub, a, a + W, 4)
    m.seed_herd(3, 64)
    for bad in (0, ORDER):
        assert kang.kang_set_herd_status(64, 0, [5, 5, bad, 5]) == E.KH_E_ARG
        assert kang.kang_set_herd_status(128, 6, [bad]) == E.KH_E_ARG  # refused before the herd is resized
        assert kang.kang_geometry()[2] == 64
        check_herd(kang, m)  # nothing was placed
    assert kang.kang_set_herd_status(64, 2, [ORDER + 1, ORDER]) == 0  # the wild at n is Q' itself
    m.set_herd(64, 2, [ORDER + 1, ORDER])
    assert m.k[2][0] == K.mul_g(1) and m.k[3][0] == m.qp
    check_herd(kang, m)


# ---- 4. a stall met after moving, reported once per call -------------------------------------------
def stall_path(jd: list[int]):
    """(d, j0, i, i2): d G selects its own table entry j0 once that entry is d, (d - jd[i]) G selects i and
    (d - jd[i] - jd[i2]) G selects i2: a tame placed there stands on J[j0] after two jumps."""
    d = 1 << 100
    while True:
        d += 1
        if d in jd:
            continue
        j0 = K.mul_g(d)[0] % 32
        t = list(jd)
        t[j0] = d
        for i in range(32):
            if i == j0 or K.mul_g(d - t[i])[0] % 32 != i:
                continue
            for i2 in range(32):
                if i2 != j0 and K.mul_g(d - t[i] - t[i2])[0] % 32 == i2:
                    return d, j0, i, i2


def test_a_stall_met_after_moving_is_reported_once_per_call(kang):
    B = kang.kang_geometry()[0]
    a, W = (0xA5A5 << 150) + 12345, (1 << 191) + 12345
    jd = K.default_jumps(W)
    d, j0, i, i2 = stall_path(jd)
    jd[j0] = d
    start = d - jd[i] - jd[i2]
    assert len(set(jd)) == 32 and start > 0
    assert K.mul_g(d)[0] % 32 == j0 and K.mul_g(d - jd[i])[0] % 32 == i and K.mul_g(start)[0] % 32 == i2
    pub = pub_of(a + W // 3)
    kang.kang_set_launch(4)
    kang.kang_setup(pub, a, a + W, 32, jd)  # dp 32: no distinguished point in a few steps
    m = K.Herd(pub, a, a + W, 32, jd)
    n, T = 2 * 64 * B, 128  # two blocks of full batches
    e = (B // 2) * T + 10
    dists = [1 + K._h(b"stall-late" + k.to_bytes(4, "little")) % W for k in range(n)]
    dists[e] = start
    kang.kang_set_herd(n, 0, dists)
    m.set_herd(n, 0, dists)
    assert all(st[0] is not None for st in m.k)
    stalled = (K.mul_g(d)[0], d, e, K.TAME | K.STALL)
    # six jumps in launches of 4 and 2: it stalls in the middle of the first and the second finds it reported
    for call in range(2):
        recs, lost = kang.kang_step(6, 64)
        want = m.step(6, 4)
        assert want == [stalled] and lost == 0
        assert recs == want
        assert m.k[e] == [K.mul_g(d), d]
        check_herd(kang, m)  # the stalled one where it was, its batch neighbours moved as the model's
    assert kang.kang_add_dps(recs) is None
    assert m.add_dps(want) is None
    assert m.gen[e] == 1 and sum(m.gen) == 1 and m.stats["stalls"] == 1
    check_herd(kang, m)


# ---- 5. the placement passes and a large grid ------------------------------------------------------
N20 = (1 << 20) + 67
A70, W70 = (0xBEEF << 140) + 4321, width(70)


def sample_of(N: int, T: int) -> list[int]:
    """Kangaroos around the lane count T, the last batch slot, every multiple of the 2^20 of a placement pass
    and the herd's end, and 64 hashed ones."""
    ids = {0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 17 * T - 1, 17 * T, 31 * T - 1, 31 * T, N - 2, N - 1}
    for k in range(1 << 20, N + 1, 1 << 20):
        ids.update((k - 2, k - 1, k, k + 1))
    ids.update(K._h(b"sample" + bytes([i])) % N for i in range(64))
    return sorted(i for i in ids if 0 <= i < N)


def check_some(e, m):
    for i, w in zip(m.ids, m.state()):
        assert e.kang_get_herd(i, 1)[0] == w, i


def sampled_herd(kang, n_arg, N):
    B = kang.kang_setup(pub_of(A70 + W70 // 3), A70, A70 + W70, 32)
    assert kang.kang_seed(9, n_arg) == N
    T = 64 * -(-N // (64 * B))
    ids = sample_of(N, T)
    assert {T, 31 * T, (1 << 20) - 1, 1 << 20, N - 1} <= set(ids) and 31 * T < N
    m = K.Herd(pub_of(A70 + W70 // 3), A70, A70 + W70, 32)
    m.seed_some(9, N, ids)
    assert all(st[0] is not None for st in m.k)
    check_some(kang, m)
    spl = K.launch_steps(N, W70)
    assert kang.kang_geometry()[1] == spl >= 128
    recs, lost = kang.kang_step(3, 16)
    want = m.step(3, spl)
    assert want == []  # no stall among the sampled; with dp 32 the rest of the herd reports nothing either
    assert len(recs) + lost == 0
    check_some(kang, m)


def test_placement_passes_beyond_2_20(kang):
    sampled_herd(kang, N20, N20)


def test_placement_passes_of_the_default_herd(kang):
    """2^23 kangaroos in eight passes, the herd every search of 62 bits or more starts with."""
    sampled_herd(kang, 0, 1 << 23)


def test_head_count_of_a_large_herd(kang):
    pub = pub_of(A70 + W70 // 3)
    kang.kang_setup(pub, A70, A70 + W70, 0)
    assert kang.kang_seed(9, N20) == N20
    recs, lost = kang.kang_step(3, 100)
    assert len(recs) == 100 and lost == 3 * N20 - 100
    # whichever kangaroos took the 100 slots, each record is one the model gives
    m = K.Herd(pub, A70, A70 + W70, 0)
    m.seed_some(9, N20, sorted({r[2] for r in recs}))
    assert not collections.Counter(recs) - collections.Counter(m.step(3, 256))


@pytest.mark.parametrize("N", [64, 4096])
def test_geometry_on_both_sides_of_each_rule(kang, N):
    pub = pub_of(12345)
    seen = set()
    for rule, vs in (("dp", [N << 1, N << 5, N << 32]), ("launch", [N * 4, N * 16 * 4, N * 128 * 4])):
        for v in vs:
            pair = []
            for W in ((8 * v) ** 2, (8 * v) ** 2 - 1):
                kang.kang_setup(pub, 1, 1 + W)  # the automatic dp
                assert kang.kang_seed(1, N) == N
                _, spl, herd, dp = kang.kang_geometry()
                assert (herd, dp, spl) == (N, K.default_dp(N, W), K.launch_steps(N, W)), (rule, v, W)
                pair.append(dp if rule == "dp" else spl)
            assert pair[0] == pair[1] + 1 if rule == "dp" else pair[0] == 2 * pair[1]
            seen.add((rule, pair[0]))
    assert {("dp", 1), ("dp", 5), ("dp", 32), ("launch", 2), ("launch", 32), ("launch", 256)} == seen


def test_default_herd(kang):
    pub = pub_of(12345)
    want = {(1 << 28) - 1: 64, 1 << 28: 128, (1 << 30) - 1: 128, 1 << 38: 4096}
    for W, n in want.items():
        assert K.default_herd(W) == n
        kang.kang_setup(pub, 1, 1 + W)
        assert kang.kang_seed(2, 0) == n
    assert K.default_herd(W70) == 1 << 23


# ---- 6. planted collisions: a wide solve end to end ------------------------------------------------
SOLVES = [((0xA5A5 << 150) + 12345, (1 << 191) + 777), (ORDER - 2 - ((1 << 128) + 99), (1 << 128) + 99),
          (A_HIGH, (1 << 69) + 5)]


@pytest.mark.parametrize("lead", [0, 3])
@pytest.mark.parametrize("case", range(3))
def test_solve_a_planted_collision_in_a_wide_range(kang, case, lead):
    a, W = SOLVES[case]
    kp = W // 3 + 0x1234567
    pub = pub_of(a + kp)
    m = K.Herd(pub, a, a + W, 4)
    m.seed_herd(5, 64)
    pt, w0 = m.k[1]
    wd = w0
    for _ in range(lead):  # where the wild will be after `lead` jumps
        j = pt[0] % 32
        pt, wd = K.add(pt, m.J[j]), wd + m.jd[j]
    t = kp + wd
    m.set_herd(64, 0, [t, w0])
    assert m.k[0][0] == pt and m.k[1][1] == w0 and t >> 64
    bound = 40 * 64 * 8
    assert m.solve(bound, 8) == a + kp
    assert m.stats["jumps"] <= bound and m.stats["bad"] == 0
    print(f"case {case} lead {lead}: {m.stats}")
    kang.kang_set_launch(8)
    kang.kang_setup(pub, a, a + W, 4)
    assert kang.kang_seed(5, 64) == 64
    kang.kang_set_herd(64, 0, [t, w0])
    got, st = kang.kang_solve(bound)
    assert got == a + kp
    assert {f: getattr(st, f) for f in m.stats} == m.stats
    assert st.lost == 0 and st.bad == 0
    check_herd(kang, m)
