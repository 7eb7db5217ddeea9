"""Taproot key-path outputs (BIP-86: no script tree), restated from BIP-340 and BIP-341 in plain Python:
tagged hashes, lift_x, the TapTweak of an internal key and the bech32m address of the output key
(BIP-350, through _segwit.encode).  Points are affine (x, y) integer pairs, None is the point at infinity."""
import hashlib

from _segwit import BECH32M, encode

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        s = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        s = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (s * s - a[0] - b[0]) % P
    return x, (s * (a[0] - x) - a[1]) % P


def mul(k, pt=G):
    r = None
    while k:
        if k & 1:
            r = add(r, pt)
        pt = add(pt, pt)
        k >>= 1
    return r


_COMB = []


def mul_g(k):
    """k G by a byte comb, 32 additions at the most: the dense tests tweak a thousand keys."""
    if not _COMB:
        base = G
        for _ in range(32):
            row, pt = [None], None
            for _ in range(255):
                pt = add(pt, base)
                row.append(pt)
            _COMB.append(row)
            base = add(pt, base)
    r = None
    for j in range(32):
        r = add(r, _COMB[j][(k >> (8 * j)) & 255])
    return r


def tagged_hash(tag: str, msg: bytes) -> bytes:
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + msg).digest()


def lift_x(x: int):
    """BIP-340: the point of x-coordinate x with even y, or None."""
    if x >= P:
        return None
    c = (pow(x, 3, P) + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return x, y if y % 2 == 0 else P - y


def tweak(x: int) -> int:
    """t = int(hash_TapTweak(bytes(x))) for a key-path-only output (no merkle root)."""
    return int.from_bytes(tagged_hash("TapTweak", x.to_bytes(32, "big")), "big")


def output_x(x: int):
    """x(Q) of Q = lift_x(x) + t G, or None where BIP-341 fails (t >= n, x not on the curve, Q at infinity)."""
    t = tweak(x)
    pt = lift_x(x)
    if t >= N or pt is None:
        return None
    q = add(pt, mul_g(t))
    return None if q is None else q[0]


def address_of_x(qx: int) -> str:
    return encode("bc", 1, qx.to_bytes(32, "big"), BECH32M)


def bip340_key(k: int):
    """(d, P) for the secret k: P = k G, d = k if P.y is even, else n - k (what a tr(KEY) descriptor takes)."""
    pt = mul_g(k % N)
    return (k % N if pt[1] % 2 == 0 else N - k % N), pt


def key_output(k: int):
    """(output x, address, d, P) of secret k; asserts that (d + t) G has the output key's x."""
    d, pt = bip340_key(k)
    qx = output_x(pt[0])
    assert qx is not None
    assert mul_g((d + tweak(pt[0])) % N)[0] == qx
    return qx, address_of_x(qx), d, pt


def walk(start: int, stride: int, count: int):
    """The points (start + i stride) G, i < count, by repeated addition (one multiplication each end)."""
    pt, step = mul(start % N), mul(stride % N)
    for _ in range(count):
        yield pt
        pt = add(pt, step)


# published vectors: BIP-86's first receive address (m/86'/0'/0'/0/0) and BIP-341's wallet vector 0
VECTORS = [
    ("cc8a4bc64d897bddc5fbc2f670f7a8ba0b386779106cf1223c6fc5d7cd6fc115",
     "a60869f0dbcf1dc659c9cecbaf8050135ea9e8cdc487053f1dc6880949dc684c",
     "bc1p5cyxnuxmeuwuvkwfem96lqzszd02n6xdcjrs20cac6yqjjwudpxqkedrcr"),
    ("d6889cb081036e0faefa3a35157ad71086b123b2b144b649798b494c300a961d",
     "53a1f6e454df1aa2776a2814a721372d6258050de330b3c6d10ee8f4e0dda343",
     "bc1p2wsldez5mud2yam29q22wgfh9439spgduvct83k3pm50fcxa5dps59h4z5"),
]
SMALL_KEYS = {
    1: "bc1pmfr3p9j00pfxjh0zmgp99y8zftmd3s5pmedqhyptwy6lm87hf5sspknck9",
    2: "bc1pet7ep3czdu9k4wvdlz2fp5p8x2yp7t6ttyqg2c6cmh0lgeuu9lasmp9hsg",
    3: "bc1pgxxyvcmdncdxs06cudd5yvmwwahaesaj6n3eu7st7x4sw9hrchaqjy33gs",
}
