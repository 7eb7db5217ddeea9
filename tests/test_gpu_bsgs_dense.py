"""The BSGS giant walk pinned at every in-group offset, lane and group.

At the design rate layer 1 passes 6.6e-7 of the giant points, so the candidate lists the other BSGS
tests compare hold a handful of entries: a walk that is wrong at one of a group's 4096 offsets passes
them.  Here layer 1 is made dense: the engine's own built bytes OR'ed with seeded random bits
(tests/_dense_layer.py), installed on the device (kh_bsgs_set_bloom) and handed, byte for byte, to the
CPU oracle, which walks the reference's 1024-point groups and probes the same bytes
(BsgsTables.candidates).  About 1 % of the points then pass, every in-group offset holds several
expected candidates, and the logged (base, a) list must equal the oracle's exactly.  A true key still
passes: no built bit is cleared.

The conditions on the oracle's own list (every offset >= 2 candidates, share <= 3 %, below the 65,536
entries of the first candidate buffer except in the overflow case) are asserted before the engine's
list is looked at; they are what makes the comparison mean something, not tolerances."""
import random

import pytest

from _dense_layer import dense_layer

pytestmark = pytest.mark.gpu

SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
LANES = 512
SHARE = 0.0098            # of the giant points; 6.29 M points -> ~61,700 candidates, ~15 per offset of 4096
FAR = 99991               # the far target lies this many bases below the start

# Both starts have their low 64 bits within 2^40 below 2^64, so adding the offset b*2N + M*f (k_setup
# prog 2: list mode, overlapping bases) or b*2N + a*2M (k_refine) to the base carries out of the base's
# low limb in mid-call (the carry inside the offset sum itself needs base 2^64 / 2N: the last test):
#   n = 2^36: base 4's low limb is 2^64 - 12345, its first centre offset M*4097 carries;
#   n = 2^24: 2N = 33546240, the carry comes in base 512 of 1024.
START36 = (0x5A5A5A5A5 << 64) | ((1 << 64) - (1 << 39) - 12345)
START24 = (0x3C3C3C3 << 64) | ((1 << 64) - 512 * 33546240 - 999)


class Dense:
    """One engine with built tables of (n, k, layout), its layer 1 replaced by the dense one, and the
    oracle's tables over the same bytes."""

    def __init__(self, oracle, n, k, layout, share, seed):
        import keyhunt_amd as K
        self.oracle = oracle
        self.e = K.Engine(0, LANES, 0)
        self.p = oracle.bsgs_params(n, k)
        info = self.e.bsgs_setup(n, k, layer1=layout)
        assert info.layer1_layout == layout
        self.e.bsgs_build()
        blocked = layout == K.KH_LAYER1_BLOCKED
        self.blocks = info.bloom_bits[0] // 128 if blocked else 0
        built = self.e.get_bloom(1)
        self.l1 = dense_layer(built, share, blocked, info.bloom_hashes[0], seed)
        self.e.set_bloom(1, self.l1)
        assert self.e.get_bloom(1) == self.l1            # the hook put exactly these bytes there
        self.tabs = oracle.BsgsTables.from_raw(self.p, self.l1, self.e.get_bloom(2), self.e.get_bloom(3),
                                               self.e.get_bsgs_table(), l1_blocks=self.blocks)
        self.A = self.p.cycles * 1024                    # giant points per base
        self.G = 4096 if self.A % 4096 == 0 else 1024    # the walk's group
        self._oracle_lists = {}

    def close(self):
        self.e.close()

    def expected(self, start, n_bases, target):
        """The oracle's candidate list (computed once per (start, bases, target), never changed), with
        the conditions that make it a test checked first."""
        key = (start, n_bases, target)
        if key not in self._oracle_lists:
            oc = self.tabs.candidates(start, n_bases, self.oracle.pubkey(target), cap=1 << 18)
            assert oc == sorted(oc) and len(set(oc)) == len(oc)
            self._oracle_lists[key] = oc
        return self._oracle_lists[key]

    def check_conditions(self, oc, n_bases, overflow=False):
        points = n_bases * self.A
        per = [0] * self.G
        for _, a in oc:
            per[a % self.G] += 1
        print(f"oracle: {points} points, {len(oc)} candidates, share {100 * len(oc) / points:.3f} %, "
              f"min per offset {min(per)}")
        assert min(per) >= 2
        assert len(oc) <= 0.03 * points
        assert (len(oc) > 65536) if overflow else (len(oc) < 65536)

    def logged(self, call):
        """Run call() with candidate logging; (its result, the sorted logged (base, a, mask) list)."""
        self.e.bsgs_log_candidates(True)
        self.e.kernel_time_reset()
        res = call()
        got = sorted(self.e.bsgs_logged_candidates())
        self.e.bsgs_log_candidates(False)
        return res, got

    def base_key(self, start, b, a):
        return start + b * 2 * self.p.n + a * 2 * self.p.m

    def check_masks(self, got, keys, target, seed):
        """The logged layer-2 mask of a seeded sample of 512 candidates and of every candidate whose
        mask is set, against the oracle's bsgs_secondcheck probes."""
        pick = set(random.Random(seed).sample(range(len(got)), min(512, len(got))))
        pick |= {i for i, g in enumerate(got) if g[2]}
        pick = sorted(pick)
        om = self.oracle.bsgs_second_masks(self.tabs, [keys[i] for i in pick], self.oracle.pubkey(target))
        assert [got[i][2] for i in pick] == om

    def true_candidate(self, oc, start, base, q, key):
        """Index in the oracle's list of the first candidate of `base` that the oracle refines to key."""
        for i, (b, a) in enumerate(oc):
            if b == base and self.tabs.refine(start + b * 2 * self.p.n, a, q) == key:
                return i
        raise AssertionError("the oracle's own list must hold the true candidate")

    def walked(self):
        from keyhunt_amd.engine import TIME_BSGS
        return self.e.kernel_time(TIME_BSGS)[2]


@pytest.fixture(scope="module")
def dense(oracle):
    """(n, k, layout) -> Dense, each built once for the module."""
    made = {}

    def get(n, k, layout, share=SHARE):
        key = (n, k, layout, share)
        if key not in made:
            made[key] = Dense(oracle, n, k, layout, share, seed=100 * n.bit_length() + 2 * k + layout)
        return made[key]

    yield get
    for d in made.values():
        d.close()


N36, K16 = 1 << 36, 16    # M = 2^22, a base holds 16384 giant points = 4 groups of 4096: continuous, H = 2048
N24, K3 = 1 << 24, 3      # cycles*1024 = 2048 != aux = 1365: bases overlap, lanes restart per base, H = 512


def _diff(got_ba, oc, G):
    """What differs, for the assertion message: counts and the first few entries with their offsets."""
    g, o = set(got_ba), set(oc)
    miss, extra = sorted(o - g), sorted(g - o)
    return (f"missing {len(miss)} extra {len(extra)}; missing (base, a, offset) {[(b, a, a % G) for b, a in miss[:12]]}; "
            f"extra {[(b, a, a % G) for b, a in extra[:12]]}")


@pytest.mark.parametrize("layout", [1, 0], ids=["blocked", "reference"])
def test_continuous_one_call_every_offset(dense, layout):
    """n = 2^36, k = 16, 384 bases = 1536 groups on 512 lanes: 3 groups per lane in one round of two
    launches, so every lane steps its centre twice.  Blocked: k_walk<KM_BSGSB, 2048> (LDS table);
    reference: k_walk<KM_BSGS, 2048> (probe_pair_bsgs).  Far target: the sorted logged (base, a) list is
    the oracle's, nothing missing, nothing extra; the walk counted bases x cycles x 1024 points; the
    logged layer-2 masks are the oracle's.
    Measured (oracle, 6,291,456 points): blocked share 0.982 %, 61,766 candidates, at least 4 per offset;
    reference 0.989 %, 62,233, at least 4."""
    from keyhunt_amd.engine import TIME_BSGS, TIME_SETUP
    d = dense(N36, K16, layout)
    assert (d.p.aux, d.p.cycles, d.G) == (16384, 16, 4096)
    nb = 384
    far = START36 - FAR * 2 * d.p.n
    oc = [c for c in d.expected(START36, 385, far) if c[0] < nb] if layout == 1 else d.expected(START36, nb, far)
    d.check_conditions(oc, nb)
    d.e.bsgs_set_targets([d.oracle.pubkey(far)])
    res, got = d.logged(lambda: d.e.bsgs_scan(START36, nb))
    assert res == []
    got_ba = [(b, a) for b, a, _ in got]
    assert got_ba == oc, _diff(got_ba, oc, d.G)
    assert d.walked() == nb * d.p.cycles * 1024
    # the geometry: no calibration with explicit lanes; one lane setup of 512 lanes; 3 groups per lane
    # at two per launch
    assert d.e.bsgs_geometry() == (0, 0.0, 0.0)
    assert d.e.kernel_time(TIME_SETUP)[0::2] == (1, LANES)
    assert d.e.kernel_time(TIME_BSGS)[0] == 2
    d.check_masks(got, [d.base_key(START36, b, a) for b, a in got_ba], far, seed=layout)


@pytest.mark.parametrize("layout", [1, 0], ids=["blocked", "reference"])
def test_continuous_key_in_last_base(dense, layout):
    """The same call with a real key in the last base: found, and the candidates up to the true one are
    the oracle's (the engine logs its whole round, the true one included).
    Measured (oracle, 6,291,456 points): blocked share 0.980 %, 61,635 candidates, at least 2 per offset;
    reference 0.981 %, 61,717, at least 4."""
    d = dense(N36, K16, layout)
    nb = 384
    key = START36 + (nb - 1) * 2 * d.p.n + 2 * d.p.m * 9000 + 31337
    q = d.oracle.pubkey(key)
    oc = d.expected(START36, nb, key)
    d.check_conditions(oc, nb)
    d.e.bsgs_set_targets([q])
    res, got = d.logged(lambda: d.e.bsgs_scan(START36, nb))
    assert res == [(0, key)]
    upto = d.true_candidate(oc, START36, nb - 1, q, key) + 1
    got_ba = [(b, a) for b, a, _ in got]
    assert got_ba[:upto] == oc[:upto], _diff(got_ba[:upto], oc[:upto], d.G)
    assert got[upto - 1][2] != 0


def test_two_calls_keep_lanes(dense):
    """The 384 bases as two calls of 192 (blocked): 768 groups = 384 lanes x 2, the lanes tile the call
    and are kept, so the second call continues them -- one lane setup in all -- and the union of the
    two lists is the one-call list.  Replacing layer 1 did not invalidate the kept lanes either: the
    layer is installed again between the calls.
    Measured (oracle): the one-call list, share 0.982 %, 61,766 candidates, at least 4 per offset."""
    from keyhunt_amd.engine import TIME_SETUP
    d = dense(N36, K16, 1)
    far = START36 - FAR * 2 * d.p.n
    oc = [c for c in d.expected(START36, 385, far) if c[0] < 384]
    d.check_conditions(oc, 384)
    d.e.bsgs_set_targets([d.oracle.pubkey(far)])
    d.e.bsgs_log_candidates(True)
    d.e.kernel_time_reset()
    assert d.e.bsgs_scan(START36, 192) == []
    first = d.e.bsgs_logged_candidates()
    d.e.set_bloom(1, d.l1)
    d.e.bsgs_log_candidates(True)
    assert d.e.bsgs_scan(START36 + 192 * 2 * d.p.n, 192) == []
    second = d.e.bsgs_logged_candidates()
    d.e.bsgs_log_candidates(False)
    assert max(len(first), len(second)) < 65536
    got_ba = sorted([(b, a) for b, a, _ in first] + [(b + 192, a) for b, a, _ in second])
    assert got_ba == oc, _diff(got_ba, oc, d.G)
    assert d.e.kernel_time(TIME_SETUP)[0] == 1
    assert d.walked() == 384 * d.p.cycles * 1024


@pytest.mark.parametrize("nb", [385, 383])
def test_ragged_calls(dense, nb):
    """Calls the 512 lanes do not tile with 3 groups each (blocked).  385 bases = 1540 groups: the
    engine plans 385 lanes x 4 groups.  383 bases = 1532 groups: 511 lanes x 3 = 1533, the last
    lane-group lies past the end of the call and stays unprobed.  Same exact list; the walk counts the
    call's points only.
    Measured (oracle): 385 bases 6,307,840 points, share 0.982 %, 61,954 candidates, at least 4 per
    offset; 383 bases 6,275,072 points, 0.981 %, 61,583, at least 4."""
    d = dense(N36, K16, 1)
    far = START36 - FAR * 2 * d.p.n
    oc = [c for c in d.expected(START36, 385, far) if c[0] < nb]
    d.check_conditions(oc, nb)
    d.e.bsgs_set_targets([d.oracle.pubkey(far)])
    res, got = d.logged(lambda: d.e.bsgs_scan(START36, nb))
    assert res == []
    got_ba = [(b, a) for b, a, _ in got]
    assert got_ba == oc, _diff(got_ba, oc, d.G)
    assert d.walked() == nb * d.p.cycles * 1024


def test_list_mode_shuffled_and_host_centres(dense):
    """The 384 bases shuffled through kh_bsgs_scan_list (blocked): per-base lanes (one lane per base, 4
    groups each) whose scalars k_setup prog 2 derives on the device, and k_refine in list mode; base 4's
    centre offsets carry out of the low limb.  Then a short list with a base within 3N below the
    group order, which sends the whole call down the host-centre path.
    Measured (oracle): the shuffled list 0.982 %, 61,766 candidates, at least 4 per offset."""
    d = dense(N36, K16, 1)
    far = START36 - FAR * 2 * d.p.n
    q = d.oracle.pubkey(far)
    oc = [c for c in d.expected(START36, 385, far) if c[0] < 384]
    d.check_conditions(oc, 384)
    order = list(range(384))
    random.Random(36).shuffle(order)
    where = {b: i for i, b in enumerate(order)}          # base -> its place in the list
    exp = sorted((where[b], a) for b, a in oc)
    d.e.bsgs_set_targets([q])
    res, got = d.logged(lambda: d.e.bsgs_scan_list([START36 + b * 2 * d.p.n for b in order]))
    assert res == []
    got_ba = [(i, a) for i, a, _ in got]
    assert got_ba == exp, _diff(got_ba, exp, d.G)
    assert d.walked() == 384 * d.p.cycles * 1024
    d.check_masks(got, [d.base_key(START36, order[i], a) for i, a in got_ba], far, seed=7)
    # host centres: bases 5, 3, 4 of the run and one whose 2N keys pass the group order
    high = SECP_N - 2 * d.p.n + 777
    oh = d.expected(high, 1, far)
    bases = [5, 3, None, 4]
    exp = sorted([(bases.index(b), a) for b, a in oc if b in bases] + [(2, a) for _, a in oh])
    assert len(oh) > 100
    res, got = d.logged(lambda: d.e.bsgs_scan_list([high if b is None else START36 + b * 2 * d.p.n for b in bases]))
    assert res == []
    got_ba = [(i, a) for i, a, _ in got]
    assert got_ba == exp, _diff(got_ba, exp, d.G)
    keys = [(high + a * 2 * d.p.m) % SECP_N if bases[i] is None else d.base_key(START36, bases[i], a) for i, a in got_ba]
    d.check_masks(got, keys, far, seed=8)


@pytest.mark.parametrize("layout", [1, 0], ids=["blocked", "reference"])
def test_overlapping_bases_small_groups(dense, layout):
    """n = 2^24, k = 3 through kh_bsgs_scan: cycles*1024 = 2048 != aux = 1365, so bases overlap, lanes
    restart per base (k_setup prog 2 with b*2N), the walk uses 1024-point groups (H = 512) and the
    non-LDS table path.  1024 bases, two rounds of 512 lanes x 2 groups; the start's low limb carries in
    base 512.  Far target: exact list, walked points, masks; then a real key in the last base.
    Measured (oracle, 2,097,152 points, offsets mod 1024): blocked far 0.993 %, 20,816 candidates, at
    least 7 per offset, with the key 0.997 %, 20,918, 8; reference far 0.966 %, 20,251, 6, with the key
    0.968 %, 20,294, 6."""
    d = dense(N24, K3, layout)
    assert (d.p.aux, d.p.cycles, d.G, 2 * d.p.n) == (1365, 2, 1024, 33546240)
    nb = 1024
    far = START24 - FAR * 2 * d.p.n
    oc = d.expected(START24, nb, far)
    d.check_conditions(oc, nb)
    d.e.bsgs_set_targets([d.oracle.pubkey(far)])
    res, got = d.logged(lambda: d.e.bsgs_scan(START24, nb))
    assert res == []
    got_ba = [(b, a) for b, a, _ in got]
    assert got_ba == oc, _diff(got_ba, oc, d.G)
    assert d.walked() == nb * d.p.cycles * 1024
    d.check_masks(got, [d.base_key(START24, b, a) for b, a in got_ba], far, seed=24 + layout)
    # a real key in the last base (past the overlap with the base before it)
    key = START24 + (nb - 1) * 2 * d.p.n + 2 * d.p.m * 1100 + 4242
    q = d.oracle.pubkey(key)
    ok = d.expected(START24, nb, key)
    d.check_conditions(ok, nb)
    d.e.bsgs_set_targets([q])
    res, got = d.logged(lambda: d.e.bsgs_scan(START24, nb))
    assert res == [(0, key)]
    upto = d.true_candidate(ok, START24, nb - 1, q, key) + 1
    got_ba = [(b, a) for b, a, _ in got]
    assert got_ba[:upto] == ok[:upto], _diff(got_ba[:upto], ok[:upto], d.G)


def test_list_mode_small_groups_limb_carry(dense):
    """n = 2^24, k = 3 through kh_bsgs_scan_list (blocked): 96 bases around the low limb's carry (bases
    464..559 of the run above, shuffled).  An extra over the cases with per-offset conditions: about
    2,000 candidates, two per offset on average."""
    d = dense(N24, K3, 1)
    far = START24 - FAR * 2 * d.p.n
    run = list(range(464, 560))
    oc = [c for c in d.expected(START24, 1024, far) if c[0] in set(run)]
    order = run[:]
    random.Random(24).shuffle(order)
    where = {b: i for i, b in enumerate(order)}
    exp = sorted((where[b], a) for b, a in oc)
    assert len(exp) > 1000                               # 96 x 2048 points at ~1 %
    d.e.bsgs_set_targets([d.oracle.pubkey(far)])
    res, got = d.logged(lambda: d.e.bsgs_scan_list([START24 + b * 2 * d.p.n for b in order]))
    assert res == []
    got_ba = [(i, a) for i, a, _ in got]
    assert got_ba == exp, _diff(got_ba, exp, d.G)
    d.check_masks(got, [d.base_key(START24, order[i], a) for i, a in got_ba], far, seed=9)


def test_overflow_grows_and_redoes(dense, oracle):
    """About 2.9 % of the points pass (blocked, 192 bases = 3.1 M points, ~91,000 candidates): the round
    overflows the 65,536-entry buffer, the buffers grow and the round is walked again -- the walk
    counts its points twice -- and the list is still the oracle's exactly.
    Measured (oracle, 3,145,728 points): share 2.891 %, 90,948 candidates, at least 6 per offset."""
    d = Dense(oracle, N36, K16, 1, 0.029, seed=29)       # its own engine: the buffers start at 65,536
    try:
        nb = 192
        far = START36 - FAR * 2 * d.p.n
        oc = d.expected(START36, nb, far)
        d.check_conditions(oc, nb, overflow=True)
        d.e.bsgs_set_targets([oracle.pubkey(far)])
        res, got = d.logged(lambda: d.e.bsgs_scan(START36, nb))
        assert res == []
        got_ba = [(b, a) for b, a, _ in got]
        assert got_ba == oc, _diff(got_ba, oc, d.G)
        assert d.walked() == 2 * nb * d.p.cycles * 1024
        d.check_masks(got, [d.base_key(START36, b, a) for b, a in got_ba], far, seed=29)
    finally:
        d.close()


def test_set_bloom_argument_and_state_errors(oracle, tmp_path):
    """kh_bsgs_set_bloom: KH_E_STATE before the tables exist, KH_E_ARG for a layer other than 1 and 2 or
    another byte count; kh_bsgs_save refuses after either layer until the tables are built again."""
    import keyhunt_amd as K
    KH_E_ARG = -1
    with K.Engine(0, LANES, 0) as e:
        def status(layer, data):
            return K.lib().kh_bsgs_set_bloom(e._ctx, layer, data, len(data))
        e.bsgs_setup(1 << 20, 1, layer1=K.KH_LAYER1_REFERENCE)
        assert status(1, bytes(16)) == K.KH_E_STATE
        e.bsgs_build()
        l1 = e.get_bloom(1)
        l2, l3 = e.get_bloom(2), e.get_bloom(3)
        for layer, data in ((0, l1), (3, l1), (3, l3), (4, l1), (1, l1[:-1]), (1, l1 + b"\0"), (2, l2[:-1]),
                            (2, l2 + b"\0")):
            assert status(layer, data) == KH_E_ARG, (layer, len(data))
        assert (e.get_bloom(1), e.get_bloom(2), e.get_bloom(3)) == (l1, l2, l3)
        e.set_bloom(1, l1)
        assert K.lib().kh_bsgs_save(e._ctx, str(tmp_path).encode()) == K.KH_E_STATE
        e.bsgs_build()
        e.set_bloom(2, l2)                               # layer 2 is taken too, and save refuses as well
        assert K.lib().kh_bsgs_save(e._ctx, str(tmp_path).encode()) == K.KH_E_STATE
        e.bsgs_build()
        e.bsgs_save(str(tmp_path))
        e.bsgs_setup(1 << 20, 1, layer1=K.KH_LAYER1_REFERENCE)
        assert status(1, l1) == K.KH_E_STATE             # set up again, not built yet


def test_offset_sum_carries_out_of_its_low_limb(engine, oracle):
    """k_setup prog 2 and k_refine add b*2N and the in-base offset (M*f, a*2M) as 128-bit numbers before
    adding the base; the carry between the sum's limbs (c0) is 1 only where low64(b*2N) + offset >=
    2^64, i.e. from base 2^64 / 2N on -- whatever the start -- and only where bases overlap (with a
    power-of-two N the low limb of b*2N has room for every offset).  The smallest shape that gets there
    in seconds: n = 2^52, k = 3 (M = 3*2^26, 2N = 2^53 - 2^27, bases of 22,370,304 points overlapping by
    683): 2048 * 2N = 2^64 - 683 * 2M + 2M/3, so in base 2048 every lane centre past the first and
    every candidate from a = 683 on carries.  A key there, 4.6e10 giant points after the start, is
    found only if both sums are right (the walk has no dense layer here: the key is the check)."""
    n, k = 1 << 52, 3
    p = oracle.bsgs_params(n, k)
    A = p.cycles * 1024
    assert (p.m, p.aux, A) == (3 << 26, 22369621, 22370304)
    b = (1 << 64) // (2 * p.n)
    a = 5_000_000
    low = (b * 2 * p.n) & ((1 << 64) - 1)
    assert b == 2048 and low + 683 * 2 * p.m >= 1 << 64 > low + 682 * 2 * p.m
    assert A - p.aux < a < p.aux                         # past the overlap with base 2047, inside 2N
    start = (0x2D2D2D << 64) + 0x123456789ABCDEF
    key = start + b * 2 * p.n + a * 2 * p.m + 777
    engine.bsgs_setup(n, k, layer1=1)
    engine.bsgs_build()
    engine.bsgs_set_targets([oracle.pubkey(key)])
    assert engine.bsgs_scan(start, b + 1) == [(0, key)]
