"""k_setup and k_refine checked lane by lane and point by point, all by exact equality.

k_setup (lane centres C_g = [Q +] s_g*G) runs through kh_setup_centres in its three forms -- uploaded
scalars, the progression s0 + g*step, the BSGS centres -(base(b) + M*(2(a0 + H) + 1)) -- and every centre
is compared with the oracle's independent double-and-add (oracle.pubkey), its affine sum
(oracle.point_add), its 1024-point group walk (oracle.walk_points, for 2^20 lanes) and, where Q = +-s*G,
the reference's AddDirect value (oracle.add_direct, pinned by tests/test_add_direct.py).  The lane scalars
are Python integers.

k_refine (the second check: 32 x-coordinates S + AMP2[i] per candidate from one batched inversion) is seen
through the layer-2 mask of those 32 points.  At the built layer's 1e-6 false-positive rate nearly every
mask is 0 whatever the x's are, so layer 2 is replaced (kh_bsgs_set_bloom) by the built bits OR'ed with
seeded random ones that pass a quarter of all x's: every one of the 32 points then decides a mask bit of
many candidates.  GPU masks = host-twin masks = the oracle's bsgs_secondcheck, through the list hook
(kh_bsgs_second_masks) and through the kernel's own index arithmetic (kh_bsgs_refine_masks).

What cannot happen, by arithmetic, and is therefore not a case here:
  * with a base < n the sum base + offset never carries out of 2^256: 2^256 - n > 1.27 * 2^128, and the
    offset stays below 2^128 + 2^97 (k_setup: b <= 2^64/a_pts, f <= 2 a_pts + 2^33) or below 2^128
    (k_refine).  The hooks pass bases raw, and the kernels' sum is right mod n for any 256-bit base
    (base + offset < 2n), so the carry-out case uses a base in [n, 2^256), which the engine never sends;
  * k_refine's offset b*2N + a*2M is at most (2^64 - 1)((2^64 - 1)/a_pts + a_pts - 1) < 2^128, so its
    bit 128 (s2) is always 0; k_setup's reaches 2^128 (a_pts = 1, 2N = 2^64 - 1, M ~ 2^59)."""
import functools
import random

import numpy as np
import pytest

from _dense_layer import dense_layer

pytestmark = pytest.mark.gpu

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P = 2**256 - 2**32 - 977
KH_E_ARG = -1
KQ = 0x5DEECE66D1234567F00DFACE                      # Q = KQ*G, the point added to every lane


def _orc():
    import oracle
    return oracle


def pairs(raw):
    return [(int.from_bytes(raw[i:i + 32], "big"), int.from_bytes(raw[i + 32:i + 64], "big"))
            for i in range(0, len(raw), 64)]


@functools.lru_cache(maxsize=None)
def pub(s):
    return _orc().pubkey(s)


def plus_q(s):
    """The reference's value of Q + s*G: AddDirect where the x's coincide, the affine sum elsewhere."""
    q, pt = pub(KQ), pub(s)
    return _orc().add_direct(q, pt) if pt[0] == q[0] else _orc().point_add(q, pt)


@pytest.fixture(scope="module")
def eng():
    import keyhunt_amd as K
    e = K.Engine(0, 512, 0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------
# k_setup, uploaded scalars
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_scalars():
    """The edge scalars of the byte comb, each between random neighbours (so that the comb's `if (v)`
    diverges inside a wave), among 4096 seeded random scalars."""
    rnd = random.Random(0x5E7)
    special = [v << (8 * j) for j in range(32) for v in (1, 2, 0x7F, 0x80, 0xFF)]
    special += [(1 << (8 * j)) - 1 for j in range(1, 33)]
    special += [1, 2, N - 1, N - 2, (N - 1) // 2, 1 << 255, int("00ff" * 16, 16), int("ff00" * 16, 16)]
    special = [s for s in special if 0 < s < N]
    assert len(special) == 160 + 31 + 8
    out, it = [], iter(special)
    for i in range(4096):
        out.append(rnd.randrange(1, N))
        if i % 16 == 7:
            s = next(it, None)
            if s is not None:
                out.append(s)
    assert next(it, None) is None and len(out) == 4096 + len(special)
    return out


@pytest.mark.parametrize("L", [1, 63, 64, 255, 256, 257, 4099, 0], ids=lambda L: f"L{L}" if L else "all")
def test_setup_scalars(eng, L):
    """Uploaded scalars (prog 0), no Q: every comb edge (single bytes 1, 2, 0x7F, 0x80, 0xFF at every
    position, 2^(8j) - 1, n - 1, n - 2, (n-1)/2, 2^255, alternating 00/FF bytes) and 4096 random ones."""
    s = mixed_scalars()
    off = 0 if L in (0, 4099) else 8 * L             # short launches start at different places of the list
    s = s[off:off + L] if L else s
    assert pairs(eng.setup_centres(len(s), scalars=s)) == [pub(x) for x in s]


@functools.lru_cache(maxsize=None)
def q_scalars():
    """Six waves: four ordinary ones holding one lane with s*G = Q or -Q each, one whole wave of such
    lanes, one ordinary wave."""
    rnd = random.Random(0xADD)
    s = [rnd.randrange(1, N) for _ in range(6 * 64)]
    for w, lane in enumerate((0, 17, 40, 63)):
        s[64 * w + lane] = KQ if w % 2 else N - KQ
    for lane in range(64):
        s[64 * 4 + lane] = KQ if lane % 3 else N - KQ
    return s


def test_setup_scalars_with_q_and_dx0_lanes(eng):
    """Q + s*G, with lanes where s*G = Q and s*G = -Q: there the reference's AddDirect(Q, s*G) takes the
    inverse of 0 as 0 and returns (-2 Q.x, -(s*G).y) -- the y of its second operand."""
    s = q_scalars()
    q = pub(KQ)
    want = [plus_q(x) for x in s]
    assert want[0] == ((-2 * q[0]) % P, q[1]) and want[64 + 17] == ((-2 * q[0]) % P, P - q[1])
    assert pairs(eng.setup_centres(len(s), scalars=s, q=q)) == want


def test_setup_all_scalars_with_q(eng):
    s = mixed_scalars()
    assert pairs(eng.setup_centres(len(s), scalars=s, q=pub(KQ))) == [plus_q(x) for x in s]


# ------------------------------------------------------------------------------------------------
# k_setup, the progression s0 + g*step
# ------------------------------------------------------------------------------------------------
S0_67 = 0x5A5A5A5A5A5A5A5A5
PROG_LS = [1, 2, 3, 255, 256, 257, (1 << 16) + 1, 1 << 18, 1 << 20]


@functools.lru_cache(maxsize=None)
def walk_xy():
    """(S0_67 + g*2048)*G for g < 2^20 as the hook's bytes, from the oracle's group walk (computed once)."""
    xs, ys = _orc().walk_points(S0_67, 1 << 10, stride=2048, need_y=True)
    x = np.frombuffer(xs, dtype=np.uint8).reshape(-1, 32)
    y = np.frombuffer(ys, dtype=np.uint8).reshape(-1, 32)
    raw = np.concatenate([x, y], axis=1).tobytes()
    assert pairs(raw[:64 * 3]) == [pub(S0_67 + g * 2048) for g in range(3)]   # the walk's own anchor
    return raw


@pytest.mark.parametrize("L", PROG_LS)
def test_setup_progression_lanes(eng, L):
    """prog 1 at every lane count where the bit loop's bound (A.L >> b) != 0 changes, up to 2^20 lanes."""
    got = eng.setup_centres(L, prog=(S0_67, 2048))
    assert got == walk_xy()[:64 * L]


@pytest.mark.parametrize("s0,step,L", [
    (0x1F2E3D4C5B6A79880123456789ABCDEF, (1 << 200) + 977, 1500),
    (0xC0FFEE << 180, N - 1, 1500),
    (0x7777777 << 100, N // 3 + 12345, 1500),            # wraps n about every third lane
    (N - 2, N - 3, 1500),                                # every sum carries out of 2^256
], ids=["step_2p200", "step_n_minus_1", "step_n_third", "carry_out"])
def test_setup_progression_wraps(eng, s0, step, L):
    want = [pub((s0 + g * step) % N) for g in range(L)]
    assert pairs(eng.setup_centres(L, prog=(s0, step))) == want


def test_setup_progression_zero_lane_and_q(eng):
    """Lane 5 of (n - 5, 1) is 0 mod n: KH_E_ARG as run_setup_prog reports it; five lanes succeed.  And
    one progression with Q."""
    r, _ = eng.setup_centres_status(8, prog=(N - 5, 1))
    assert r == KH_E_ARG
    assert pairs(eng.setup_centres(5, prog=(N - 5, 1))) == [pub(N - 5 + g) for g in range(5)]
    s0, step = 0x123456789ABCDEF0123, (1 << 130) + 3
    assert pairs(eng.setup_centres(300, prog=(s0, step), q=pub(KQ))) == [plus_q((s0 + g * step) % N) for g in range(300)]
    assert pairs(eng.setup_centres(130, prog=(KQ - 70, 1), q=pub(KQ)))[70] == plus_q(KQ)     # s*G = Q in prog 1


# ------------------------------------------------------------------------------------------------
# k_setup, the BSGS centres
# ------------------------------------------------------------------------------------------------
def centre_scalars(L, t_round, lane_pts, a_pts, m, h, start=0, two_n=0, bases=None):
    out = []
    for g in range(L):
        t0 = t_round + g * lane_pts
        b, a0 = divmod(t0, a_pts)
        base = bases[b] if bases is not None else start + b * two_n
        ck = (base + m * (2 * (a0 + h) + 1)) % N
        assert ck != 0
        out.append((N - ck) % N)
    return out


_R = random.Random(0xB565)
M60 = (37 << 64) // 1025                                 # M*(2*512 + 1) ~ 37 * 2^64
BSGS_CASES = {
    # lanes of 3 groups over bases of 10: lanes straddle bases, a0 takes every residue; t_round != 0
    "cross_bases": dict(L=700, t_round=7 * 1024 + 5, lane_pts=3 * 1024, a_pts=10 * 1024, m=4096, h=512,
                        start=0x5A5A5A5A5 << 64 | 0xFFFFFFFF00000000, two_n=2 * (1 << 22) - 8192),
    "h2048": dict(L=300, t_round=3, lane_pts=4096, a_pts=5 * 4096 + 1024, m=3 << 26, h=2048,
                  start=_R.getrandbits(200), two_n=(1 << 53) - (1 << 27)),
    # b*2N >= 2^64 from base 2 on, with the carry between the offset's limbs
    "b2n_past_2p64": dict(L=400, t_round=0, lane_pts=1024, a_pts=20 * 1024, m=4096, h=512,
                          start=_R.getrandbits(250), two_n=(1 << 63) - 4096 * 3000),
    # (2^64 - 1 - j)(2^64 - 1) + M*1025 reaches 2^128 for j <= 34 only: lanes with s2 = 1 and with s2 = 0
    "sum_past_2p128": dict(L=70, t_round=(1 << 64) - 70, lane_pts=1, a_pts=1, m=M60, h=512,
                           start=_R.getrandbits(255), two_n=(1 << 64) - 1),
    # a base just below n: the sum passes n (sc_add_small's compare-and-subtract case)
    "sum_past_n": dict(L=300, t_round=11, lane_pts=2048, a_pts=9 * 1024, m=4096, h=512, start=N - 1000,
                       two_n=1 << 23),
    # a raw base above n: the sum carries out of 2^256 in some lanes and not in others
    "sum_past_2p256": dict(L=300, t_round=0, lane_pts=4096, a_pts=3 * 4096, m=1 << 40, h=2048,
                           start=(1 << 256) - (1 << 60), two_n=1 << 54),
}


@pytest.mark.parametrize("with_q", [False, True], ids=["noq", "q"])
@pytest.mark.parametrize("name", list(BSGS_CASES))
def test_setup_bsgs_centres_continuous(eng, name, with_q):
    c = dict(BSGS_CASES[name])
    L = c.pop("L")
    s = centre_scalars(L, **c)
    if name == "sum_past_2p128":
        over = [(c["t_round"] + g) * c["two_n"] + c["m"] * 1025 >= 1 << 128 for g in range(L)]
        assert 20 < sum(over) < 50
    if name == "sum_past_2p256":
        over = [c["start"] + (g // 3) * c["two_n"] + c["m"] * (2 * (g % 3 * 4096 + 2048) + 1) >= 1 << 256 for g in range(L)]
        assert 20 < sum(over) < 280
    got = pairs(eng.setup_centres(L, bsgs=c, q=pub(KQ) if with_q else None))
    assert got == [plus_q(x) if with_q else pub(x) for x in s]


@pytest.mark.parametrize("with_q", [False, True], ids=["noq", "q"])
def test_setup_bsgs_centres_list(eng, with_q):
    """The list form over a shuffled list: random bases, bases just below n, raw bases above n and one
    whose centre is Q itself (with Q: the AddDirect value)."""
    rnd = random.Random(0x1157)
    m, h, a_pts, lane_pts, t_round = 4096, 512, 7 * 1024, 3 * 1024, 2 * 1024 + 9
    L = 500
    n_bases = (t_round + (L - 1) * lane_pts) // a_pts + 1
    bases = [0x3C3C3C3 << 64 | b * (1 << 23) for b in range(1, n_bases + 1)]
    rnd.shuffle(bases)
    bases[3], bases[40] = N - 5, N - m * 1025 - 1
    bases[77], bases[100] = (1 << 256) - 1, (1 << 256) - m * 2000
    # lane 33's centre key becomes -KQ, so that its scalar is KQ and Q + s*G meets dx = 0
    b33, a33 = divmod(t_round + 33 * lane_pts, a_pts)
    bases[b33] = (-KQ - m * (2 * (a33 + h) + 1)) % N
    c = dict(t_round=t_round, lane_pts=lane_pts, a_pts=a_pts, m=m, h=h, bases=bases)
    s = centre_scalars(L, **c)
    assert s[33] == KQ
    got = pairs(eng.setup_centres(L, bsgs=c, q=pub(KQ) if with_q else None))
    assert got == [plus_q(x) if with_q else pub(x) for x in s]
    # one base fewer: the last lane's base is outside the list, refused before any launch
    r, _ = eng.setup_centres_status(L, bsgs=dict(c, bases=bases[:-1]))
    assert r == KH_E_ARG
    r, _ = eng.setup_centres_status(2, bsgs=dict(c, t_round=(1 << 64) - 1))      # t0 leaves 64 bits
    assert r == KH_E_ARG
    r, _ = eng.setup_centres_status(1, bsgs=dict(c, t_round=0, bases=[(-m * 1025) % N]))   # centre key 0
    assert r == KH_E_ARG


# ------------------------------------------------------------------------------------------------
# k_refine with a dense layer 2
# ------------------------------------------------------------------------------------------------
KEY = 0x3F00DEADBEEF0123
GEOMS = {(1 << 22, 2): 22, (1 << 24, 3): 24}           # (n, k) -> seed of the dense layer


class Refine:
    def __init__(self, oracle, n, k):
        import keyhunt_amd as K
        self.o, self.p = oracle, oracle.bsgs_params(n, k)
        built = oracle.BsgsTables(self.p)
        self.e = K.Engine(0, 512, 0)
        info = self.e.bsgs_setup(n, k)
        self.e.bsgs_build()
        # the tables byte-equal to the oracle's first
        assert self.e.get_bloom(2) == built.bf2.raw and self.e.get_bloom(3) == built.bf3.raw
        assert self.e.get_bsgs_table() == built.table_bytes()
        self.l2 = dense_layer(built.bf2.raw, 0.25, False, info.bloom_hashes[1], GEOMS[(n, k)])
        self.e.set_bloom(2, self.l2)
        assert self.e.get_bloom(2) == self.l2
        self.tabs = oracle.BsgsTables.from_raw(self.p, built.bf1.raw, self.l2, built.bf3.raw, built.table_bytes())
        self.q = oracle.pubkey(KEY)
        self.e.bsgs_set_targets([self.q])
        self.A = self.p.cycles * 1024

    def want(self, keys):
        return self.o.bsgs_second_masks(self.tabs, keys, self.q)


@pytest.fixture(scope="module", params=list(GEOMS), ids=lambda g: f"n2p{g[0].bit_length() - 1}_k{g[1]}")
def ref(request, oracle):
    r = Refine(oracle, *request.param)
    yield r
    r.e.close()


def test_refine_dense_masks_list_hook(ref):
    """kh_bsgs_second_masks against the dense layer 2: the existing test's near, far, edge and +-AMP2
    bases, base = key and n - key (S = the AddDirect dx = 0 values), and S = +-AMP2[i] for every i."""
    rnd = random.Random(1234)
    p = ref.p
    near = [KEY - rnd.randrange(0, 2 * p.m) for _ in range(600)]
    far = [rnd.getrandbits(255) for _ in range(400)]
    edge = [KEY, KEY - 2 * p.m, KEY - 2 * p.m + 1, 1, N - 1, 0, N - KEY]
    amp = [KEY + s * p.m2 * (1 + 2 * i) for i in range(32) for s in (1, -1)]
    bases = near + far + edge + amp
    want = ref.want(bases)
    # the conditions that make the comparison mean something, on the oracle's masks alone
    fm = want[600:1000]
    pops = [bin(m).count("1") for m in fm]
    per_bit = [sum((m >> i) & 1 for m in fm) for i in range(32)]
    print(f"far masks: mean popcount {sum(pops) / 400:.2f}, range {min(pops)}-{max(pops)}, "
          f"per bit {min(per_bit)}-{max(per_bit)} of 400")
    assert 4 <= sum(pops) / 400 <= 14
    assert all(20 <= c <= 380 for c in per_bit)
    assert want[1005] == 0                               # base key 0: no point
    g, h = ref.e.bsgs_second_masks(0, bases)
    assert h == want
    assert g == want


def _refine_both(ref, idx, a_pts, t_round, start, two_n, two_m=0, n_bases=None):
    """The continuous form, and the list form over the same bases; base keys as Python integers."""
    tm = two_m or 2 * ref.p.m
    keys = []
    for i in idx:
        b, a = divmod(t_round + i, a_pts)
        keys.append((start + b * two_n + a * tm) % N)
    want = ref.want(keys)
    g, h = ref.e.bsgs_refine_masks(0, idx, a_pts, t_round, start=start, two_n=two_n, two_m=two_m)
    assert h == want and g == want
    if n_bases:
        bases = [start + b * two_n for b in range(n_bases)]
        bases = [b if b < 1 << 256 else b % N for b in bases]           # raw where it fits 256 bits
        g, h = ref.e.bsgs_refine_masks(0, idx, a_pts, t_round, bases=bases, two_m=two_m)
        assert h == want and g == want
    return keys, want


@pytest.mark.parametrize("count", [1, 63, 64, 65, 4099])
def test_refine_index_arithmetic(ref, count):
    """idx spanning 40 bases around the key with t_round != 0, in both forms, at every count around the
    block size."""
    rnd = random.Random(count)
    two_n = 2 * ref.p.n
    t_round = 3 * ref.A + 17
    start = KEY - 23 * two_n - 777
    idx = [rnd.randrange(0, 37 * ref.A) for _ in range(count)]
    keys, want = _refine_both(ref, idx, ref.A, t_round, start, two_n, n_bases=41)
    if count > 1:
        assert len({(t_round + i) // ref.A for i in idx}) >= 20
        assert sum(bin(m).count("1") for m in want) >= 4 * count


def test_refine_carries_and_zero_key(ref):
    two_m = 2 * ref.p.m
    rnd = random.Random(0xCA)
    # b*2N >= 2^64, and low64(b*2N) + a*2M carrying into the high limb for a >= 5
    two_n = (1 << 64) - 5 * two_m
    idx = [rnd.randrange(0, 30 * 4096) for _ in range(300)] + [4096 + 4, 4096 + 5, 3 * 4096 + 14, 3 * 4096 + 15]
    _refine_both(ref, idx, 4096, 9, rnd.getrandbits(250), two_n, n_bases=31)
    # a base just below n: the sum passes n for a >= 1; and a raw base above n: it carries out of 2^256
    _refine_both(ref, list(range(200)), 50, 0, N - two_m, 1 << 40, n_bases=4)
    _refine_both(ref, list(range(200)), 50, 0, (1 << 256) - 10 * two_m, two_m * 7, n_bases=4)
    # a raw 2M of 63 bits: the offset's high limb comes from a*2M, up to 2^126
    _refine_both(ref, [rnd.randrange(0, 1 << 63) for _ in range(100)], 1 << 62, 5, rnd.getrandbits(255),
                 (1 << 64) - 1, two_m=(1 << 64) - 59)
    # candidate 7's base key is 0 mod n: mask 0 on both sides
    b, a = divmod(3 + 7 * 11, 64)
    start = (-(b * (1 << 30) + a * two_m)) % N
    keys, want = _refine_both(ref, [7 * i for i in range(20)], 64, 3, start, 1 << 30, n_bases=3)
    assert keys[11] == 0 and want[11] == 0


def test_refine_hook_refuses_out_of_range(ref):
    e = ref.e
    bases = [KEY - 5, KEY - 6]
    assert e.bsgs_refine_masks_status(0, [0, 2 * ref.A], ref.A, bases=bases)[0] == KH_E_ARG      # base 2 of 2
    assert e.bsgs_refine_masks_status(0, [0, ref.A], ref.A, t_round=ref.A, bases=bases)[0] == KH_E_ARG
    assert e.bsgs_refine_masks_status(0, [5], ref.A, t_round=(1 << 64) - 3, start=1, two_n=2)[0] == KH_E_ARG
    assert e.bsgs_refine_masks_status(0, [5], 0, start=1, two_n=2)[0] == KH_E_ARG                # a_pts 0
    assert e.bsgs_refine_masks_status(1, [5], ref.A, start=1, two_n=2)[0] != 0                   # no such target
    assert e.bsgs_refine_masks_status(0, [0, 2 * ref.A - 1], ref.A, bases=bases)[0] == 0
