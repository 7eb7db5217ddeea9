"""Pollard's lambda search as include/kh_gpu.h states it, in plain Python: the jump-table derivation, the
seeding rule, one jump, the distinguished-point test, the table logic and the collision's resolution.  Curve
arithmetic comes from _taproot.  Points are affine (x, y) integer pairs; a record is (x, dist, index, kind)."""
import hashlib

from _taproot import N as ORDER, P, add, mul_g

TAME, WILD, STALL = 0, 1, 0x10
JUMPS = 32


def neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def pub_of(k):
    return mul_g(k % ORDER)


def mul_g_fast(k: int):
    """k G over _taproot's byte comb in Jacobian coordinates, one inversion at the end: the dense tests place
    thousands of kangaroos.  The comb's partial sums never meet the doubling or the inverse case (k < n)."""
    import _taproot
    if not _taproot._COMB:
        mul_g(1)
    X = Y = Z = None
    for j in range(32):
        q = _taproot._COMB[j][(k >> (8 * j)) & 255]
        if q is None:
            continue
        if X is None:
            X, Y, Z = q[0], q[1], 1
            continue
        zz = Z * Z % P
        u2, s2 = q[0] * zz % P, q[1] * zz * Z % P
        h, r = (u2 - X) % P, (s2 - Y) % P
        hh = h * h % P
        hhh, v = h * hh % P, X * hh % P
        X3 = (r * r - hhh - 2 * v) % P
        Y = (r * (v - X3) - Y * hhh) % P
        X, Z = X3, Z * h % P
    if X is None:
        return None
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


def _h(msg: bytes) -> int:
    return int.from_bytes(hashlib.sha256(msg).digest(), "big")


def default_jumps(W: int) -> list[int]:
    jb = W.bit_length() // 2 + 1
    out = []
    for j in range(JUMPS):
        d = _h(b"kh-kangaroo-jump" + bytes([j, jb])) % (1 << jb)
        d = d or 1
        while d in out:
            d += 1
        out.append(d)
    return out


def seed_dist(W: int, seed: int, index: int, gen: int) -> int:
    h = _h(seed.to_bytes(8, "little") + index.to_bytes(4, "little") + gen.to_bytes(4, "little"))
    return 1 + h % W if index & 1 else W // 2 + h % (W + 1)


def isqrt_div8_fits(v: int, W: int) -> bool:
    return (8 * v) ** 2 <= W


def default_dp(n: int, W: int) -> int:
    dp = 0
    while dp < 32 and isqrt_div8_fits(n << (dp + 1), W):
        dp += 1
    return dp


def launch_steps(n: int, W: int) -> int:
    """Jumps per kangaroo per launch when none is set: the largest power of two up to 256 that keeps a launch
    of the whole herd below sqrt(W)/16 jumps."""
    s = 1
    while s < 256 and n and isqrt_div8_fits(n * s * 4, W):
        s *= 2
    return s


def default_herd(W: int) -> int:
    """The herd kh_kang_seed places for n_kangaroos = 0: sqrt(W)/128 rounded down to a power of two, at least
    64 and at most 2^23."""
    n = 64
    while n < (1 << 23) and isqrt_div8_fits(n * 32, W):
        n *= 2
    return n


def is_dp(x: int, dp_bits: int) -> bool:
    return dp_bits == 0 or (x >> (256 - dp_bits)) == 0


def resolve(t: int, w: int, a: int, pub):
    for kp in ((t - w) % ORDER, (-(t + w)) % ORDER):
        k = (a + kp) % ORDER
        if k and pub_of(k) == pub:
            return k
    return None


class Herd:
    """The herd, the table and the statistics of one search."""

    def __init__(self, pub, a: int, b: int, dp_bits: int, jumps: list[int] = None, seed: int = 0):
        self.pub, self.a, self.W, self.dp_bits, self.seed = pub, a, b - a, dp_bits, seed
        self.qp = add(pub, neg(mul_g(a))) if a else pub
        self.jd = list(jumps) if jumps is not None else default_jumps(self.W)
        self.J = [mul_g(d) for d in self.jd]
        self.k = []      # per kangaroo [point or None (it could not be placed), dist]
        self.ids = None  # seed_some: the true index of each entry of k (None: entry e is kangaroo e)
        self.on_jump = None  # called as on_jump(index, j, dist) for every jump taken, dist before the jump
        self.gen = []
        self.table = {}  # x -> (dist, index, kind)
        self.stats = dict(jumps=0, dps=0, same_herd=0, reseeds=0, stalls=0, bad=0)
        self.key = None

    # -- placement ----------------------------------------------------------------------------
    def point_at(self, index: int, dist: int):
        g = mul_g_fast(dist % ORDER)
        if not index & 1:
            return g
        if g is not None and g[0] == self.qp[0]:
            return None  # dist*G = +-Q': no point
        return add(self.qp, g)

    def set_herd(self, total: int, first: int, dists: list[int]):
        if len(self.k) != total:
            self.k = [[None, 0] for _ in range(total)]
            self.gen = [0] * total
        for i, d in enumerate(dists):
            self.k[first + i] = [self.point_at(first + i, d), d]

    def seed_herd(self, seed: int, n: int):
        self.seed, self.ids = seed, None
        self.k, self.gen = [], [0] * n
        self.table, self.key = {}, None
        self.stats = dict.fromkeys(self.stats, 0)
        self.set_herd(n, 0, [seed_dist(self.W, seed, i, 0) for i in range(n)])

    def seed_some(self, seed: int, total: int, ids: list[int]):
        """Only the kangaroos `ids` of a seeded herd of `total`, each under its true index: kangaroos do not
        depend on each other, so their placement, walk and records are those of the whole herd's.  The table
        (add_dps, solve) is not for such a herd."""
        assert all(0 <= i < total for i in ids) and len(set(ids)) == len(ids)
        self.seed_herd(seed, 0)
        self.ids = list(ids)
        self.k = [[self.point_at(i, d), d] for i in ids for d in [seed_dist(self.W, seed, i, 0)]]

    # -- the walk -----------------------------------------------------------------------------
    def step(self, steps: int, spl: int):
        """`steps` jumps of every kangaroo in launches of spl: every record, a stalled kangaroo once per call.
        A kangaroo that meets dx = 0 does not move for the rest of its launch; the next launch tries it again
        (and finds it where it was).  Per step the herd's dx are inverted together (one modular inversion and
        three multiplications each), which changes no value: the dense tests walk 10^5 .. 10^6 jumps."""
        recs, stalled_seen = [], set()
        J, jd, k = self.J, self.jd, self.k
        ix = self.ids if self.ids is not None else range(len(k))
        for lo in range(0, steps, spl):
            frozen = set()
            for _ in range(min(spl, steps - lo)):
                live, dxs = [], []
                for e, (pt, dist) in enumerate(k):
                    if e in frozen:
                        continue
                    dx = (J[pt[0] % JUMPS][0] - pt[0]) % P if pt is not None else 0
                    if dx == 0:
                        frozen.add(e)
                        if e not in stalled_seen:
                            stalled_seen.add(e)
                            recs.append((pt[0] if pt is not None else None, dist, ix[e], (ix[e] & 1) | STALL))
                        continue
                    live.append(e)
                    dxs.append(dx)
                pre, acc = [], 1
                for dx in dxs:
                    pre.append(acc)
                    acc = acc * dx % P
                inv = pow(acc, -1, P) if dxs else 1
                for i in range(len(live) - 1, -1, -1):
                    e = live[i]
                    (x, y), dist = k[e]
                    j = x % JUMPS
                    li = inv * pre[i] % P
                    inv = inv * dxs[i] % P
                    if self.on_jump is not None:
                        self.on_jump(ix[e], j, dist)
                    s = (J[j][1] - y) * li % P
                    x3 = (s * s - x - J[j][0]) % P
                    k[e] = [(x3, (s * (x - x3) - y) % P), dist + jd[j]]
                    if is_dp(x3, self.dp_bits):
                        recs.append((x3, dist + jd[j], ix[e], ix[e] & 1))
        self.stats["jumps"] += len(k) * steps
        return recs

    # -- the table ----------------------------------------------------------------------------
    def add_dps(self, recs):
        assert self.ids is None
        again = []
        for x, dist, index, kind in sorted(recs, key=lambda r: (r[2], r[1])):
            if self.key is not None:
                break
            if index in again:
                continue
            if kind & STALL:
                self.stats["stalls"] += 1
                if index < len(self.k):
                    again.append(index)
                continue
            self.stats["dps"] += 1
            o = self.table.get(x)
            if o is None:
                self.table[x] = (dist, index, kind)
            elif o[2] != kind:
                t, w = (dist, o[0]) if kind == TAME else (o[0], dist)
                k = resolve(t, w, self.a, self.pub)
                if k is None:
                    self.stats["bad"] += 1
                else:
                    self.key = k
            elif o[1] != index:
                self.stats["same_herd"] += 1
                if index < len(self.k):
                    again.append(index)
        if self.key is None and again:
            for e in again:
                self.gen[e] += 1
                d = seed_dist(self.W, self.seed, e, self.gen[e])
                self.k[e] = [self.point_at(e, d), d]
            self.stats["reseeds"] += len(again)
        return self.key

    def solve(self, max_jumps: int, spl: int):
        done = 0
        while self.key is None and done < max_jumps:
            self.add_dps(self.step(spl, spl))
            done += len(self.k) * spl
        return self.key

    def state(self):
        """(x, y, dist) per kangaroo; x and y None where the kangaroo has no point."""
        return [(st[0][0], st[0][1], st[1]) if st[0] is not None else (None, None, st[1]) for st in self.k]
