"""k_kang_step dense: every jump of every kangaroo against the model at herd sizes around the lane, block
and batch boundaries, the stalled kangaroos' handling, the record buffer's bound, and the search's efficiency."""
import collections
import copy
import ctypes
import hashlib
import math

import pytest

import _kangaroo as K
from keyhunt_amd import engine as E
from test_gpu_kangaroo import check_herd, herd_sizes, kang  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
ORDER = K.ORDER
A, W = (0xBEEF << 140) + 4321, (1 << 44) + 12345
KEY = A + W // 5
_PUB = []
_SEEDED = {}


def pub():
    if not _PUB:
        _PUB.append(K.pub_of(KEY))
    return _PUB[0]


def seeded(e, n, dp):
    """Engine and model both seeded with n kangaroos; the model's placement is computed once per size."""
    B = e.kang_setup(pub(), A, A + W, dp)
    assert e.kang_seed(21, n) == n
    if n not in _SEEDED:
        m = K.Herd(pub(), A, A + W, 0)
        m.seed_herd(21, n)
        _SEEDED[n] = m
    m = copy.deepcopy(_SEEDED[n])
    m.dp_bits = dp
    return m, B


def same_records(got, want):
    """The multiset of (x, dist, index, kind); a stall record of a kangaroo without a point compares no x."""
    norm = lambda r: (None if r[0] is None else r[0], r[1], r[2], r[3])
    g = collections.Counter(norm(r) for r in got)
    w = collections.Counter(norm(r) for r in want)
    assert g == w


def run_steps(e, m, steps, spl):
    n = len(m.k)
    recs, lost = e.kang_step(steps, n * steps)
    assert lost == 0
    same_records(recs, m.step(steps, spl))


@pytest.mark.parametrize("size_index", range(6))
def test_every_jump_of_every_kangaroo(kang, size_index):
    B = kang.kang_geometry()[0]
    n = herd_sizes(B)[size_index]
    kang.kang_set_launch(4)
    m, _ = seeded(kang, n, 0)
    # 5 crosses the boundary of the 4-jump launches once, 33 eight times
    for steps in (1, 2, 5, 33):
        run_steps(kang, m, steps, 4)
    check_herd(kang, m)


@pytest.mark.parametrize("size_index", [2, 4, 5])
@pytest.mark.parametrize("dp", [4, 9])
def test_only_distinguished_points_are_reported(kang, dp, size_index):
    B = kang.kang_geometry()[0]
    n = herd_sizes(B)[size_index]
    kang.kang_set_launch(8)
    m, _ = seeded(kang, n, dp)
    steps = 40 if n <= 64 * B + 1 else 24  # either way several launches of 8
    recs, lost = kang.kang_step(steps, n * steps)
    want = m.step(steps, 8)
    assert lost == 0 and len(want) > 0
    assert all(K.is_dp(r[0], dp) for r in recs)
    same_records(recs, want)
    check_herd(kang, m)


@pytest.mark.parametrize("size_index", [0, 2, 3, 5])
def test_two_calls_equal_one(kang, size_index):
    n = herd_sizes(kang.kang_geometry()[0])[size_index]
    m, _ = seeded(kang, n, 0)  # the automatic launch size
    spl = kang.kang_geometry()[1]
    r1, _ = kang.kang_step(5, n * 5)
    r2, _ = kang.kang_step(5, n * 5)
    same_records(r1 + r2, m.step(10, spl))
    check_herd(kang, m)


def test_stalled_kangaroos(kang):
    B = kang.kang_geometry()[0]
    jd = K.default_jumps(W)
    # a distance d whose point selects its own jump: entry j = x(d G) mod 32 becomes d
    d = 1 << 20
    while d in jd:
        d += 1
    j0 = K.mul_g(d)[0] % 32
    jd[j0] = d
    # the wild sits on -d G: Q' + w G = -d G, so Q' = -(d + w) G, and the key is a + k' with k' = -(d + w)
    w = 987654321
    kp = (-(d + w)) % ORDER
    target = K.pub_of((A + kp) % ORDER)
    kang.kang_set_launch(0)
    kang.kang_setup(target, A, A + W, 32, jd)  # dp 32: no distinguished point in a few steps
    m = K.Herd(target, A, A + W, 32, jd)
    assert m.qp == K.neg(K.mul_g(d + w))
    n = 2 * 64 * B  # two blocks of full batches
    T = 128
    e_tame, e_wild, e_unplaced = (B // 2) * T + 10, (B // 2) * T + 11, (B // 2) * T + 75
    dists = [1 + K._h(b"stall" + i.to_bytes(4, "little")) % W for i in range(n)]
    dists[e_tame], dists[e_wild], dists[e_unplaced] = d, w, kp  # kp G = Q': the wild has no point
    kang.kang_set_herd(n, 0, dists)
    m.set_herd(n, 0, dists)
    assert m.k[e_tame][0] == K.mul_g(d) and m.k[e_wild][0] == K.neg(K.mul_g(d)) and m.k[e_unplaced][0] is None
    before = kang.kang_get_herd(0, n)
    recs, lost = kang.kang_step(3, 64)
    want = m.step(3, kang.kang_geometry()[1])
    assert lost == 0
    same_records([r if r[2] != e_unplaced else (None,) + r[1:] for r in recs], want)
    assert sorted(r[2] for r in recs) == [e_tame, e_wild, e_unplaced]
    assert all(r[3] & K.STALL for r in recs)
    after = kang.kang_get_herd(0, n)
    for e in (e_tame, e_wild, e_unplaced):
        assert after[e] == before[e]
    check_herd(kang, m)  # every other kangaroo, the batch neighbours among them, moved as the model's
    # the table places the three afresh at generation 1
    assert kang.kang_add_dps(recs) is None
    assert m.add_dps(want) is None
    assert [m.gen[e] for e in (e_tame, e_wild, e_unplaced)] == [1, 1, 1] and sum(m.gen) == 3
    check_herd(kang, m)
    recs, lost = kang.kang_step(2, 64)
    assert recs == [] and m.step(2, 256) == []
    check_herd(kang, m)


def test_record_buffer_bound(kang):
    B = kang.kang_geometry()[0]
    n, steps, cap = 64 * B + 1, 8, 100
    kang.kang_set_launch(0)
    m, _ = seeded(kang, n, 0)
    buf = (E.KhKangDp * (cap + 64))()
    ctypes.memset(buf, 0xA5, ctypes.sizeof(buf))
    got, lost = kang.kang_step_raw(steps, buf, cap)
    assert got == cap and lost == n * steps - cap
    tail = bytes(buf)[cap * ctypes.sizeof(E.KhKangDp):]
    assert tail == b"\xa5" * len(tail)
    want = collections.Counter(m.step(steps, kang.kang_geometry()[1]))
    recs = collections.Counter(kang._dp_tuple(buf[i]) for i in range(cap))
    assert not recs - want
    check_herd(kang, m)


def test_efficiency(kang):
    """jumps / sqrt(W) over 16 fixed seeds: mean at most 3, every run at most 16 (theory 2.14)."""
    a, w, n, dp = 1, (1 << 32) - 1, 256, 4
    root = math.isqrt(w)
    ratios = []
    for seed in range(16):
        key = a + int.from_bytes(hashlib.sha256(b"efficiency" + bytes([seed])).digest(), "big") % (w + 1)
        kang.kang_setup(K.pub_of(key), a, a + w, dp)
        kang.kang_seed(seed, n)
        got, st = kang.kang_solve(16 * root)
        assert got == key and st.bad == 0 and st.lost == 0
        ratios.append(st.jumps / root)
    print("jumps/sqrt(W):", " ".join(f"{r:.2f}" for r in ratios), "mean %.3f" % (sum(ratios) / 16))
    assert max(ratios) <= 16
    assert sum(ratios) / 16 <= 3
