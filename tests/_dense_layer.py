"""A dense BSGS layer 1 for the tests that compare candidate lists: the built layer's bytes OR'ed with
seeded random bits, so that a chosen share of all X's passes it while every baby X still does.

The random density r is derived from the built layer as measured, so that the final layer passes the
wanted share of random X's:
  reference layout -- an X owns `hashes` bit positions (a + b*i) mod bits, spread over the shard by its
      hashes, so the layer's overall density d0 decides: share = d ** hashes with
      1 - d = (1 - d0)(1 - r)  (0.79 -> 0.90 % at 20 hashes, as the oracle measures it);
  blocked layout -- an X owns one 16-byte block and, in each of its 8 half-words, two 4-bit positions
      that coincide with probability 1/16 (kh_kernels.h kh_blk_masks).  The built bits sit 16 to an
      item in that item's block, so blocks differ in fill and the overall density is not enough
      (it underestimates the share by a third at M = 2^22).  With k built bits in a half-word, that
      half passes with probability
        g(k) = 1/16 (k + (16-k) r)/16 + 15/16 (k(k-1) + 2k(16-k) r + (16-k)(15-k) r^2) / 240,
      a block with the product over its 8 halves, and the share is the mean over all blocks; r is
      found by bisection on that.  (A layer with no built bits: (15/16 r^2 + 1/16 r)^8, 0.74 -> 0.96 %.)"""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint64)


def bit_density(layer: bytes) -> float:
    """Share of set bits (padding bits past a shard's `bits` count as clear, as they are)."""
    return float(np.bincount(np.frombuffer(layer, dtype=np.uint8), minlength=256).astype(np.uint64) @ _POP) / (8 * len(layer))


def reference_random_density(built: bytes, share: float, hashes: int) -> float:
    d_final = share ** (1.0 / hashes)
    d0 = bit_density(built)
    assert d0 < d_final, (d0, d_final)
    return 1.0 - (1.0 - d_final) / (1.0 - d0)


def blocked_share(half_counts: np.ndarray, r: float) -> float:
    """Share of random X's passing built | random(r); half_counts: (blocks, 8) built bits per half-word."""
    k = np.arange(17, dtype=np.float64)
    g = (k + (16 - k) * r) / 256 + (k * (k - 1) + 2 * k * (16 - k) * r + (16 - k) * (15 - k) * r * r) / 256
    return float(g[half_counts].prod(axis=1).mean())


def blocked_random_density(built: bytes, share: float) -> float:
    blocks = np.frombuffer(built, dtype=np.uint8).reshape(-1, 16)
    blocks = blocks[::max(1, len(blocks) >> 18)]         # 2^18 blocks evenly spread: the mean to ~0.2 %
    halves = blocks.reshape(-1, 2)
    counts = (_POP[halves[:, 0]] + _POP[halves[:, 1]]).astype(np.intp).reshape(-1, 8)
    assert blocked_share(counts, 0.0) < share
    lo, hi = 0.0, 1.0
    for _ in range(40):
        mid = (lo + hi) / 2
        if blocked_share(counts, mid) < share:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def random_bits(nbytes: int, p: float, seed: int, precision: int = 14) -> np.ndarray:
    """nbytes bytes whose bits are set independently with probability p (to 2**-precision): p's binary
    digits, least significant first, each OR (digit 1) or AND (digit 0) with a fresh random array."""
    rng = np.random.Generator(np.random.PCG64(seed))
    q = int(round(p * (1 << precision)))
    assert 0 < q < (1 << precision)
    out = np.zeros(nbytes, dtype=np.uint8)
    for i in range(precision):
        r = rng.integers(0, 256, nbytes, dtype=np.uint8)
        if (q >> i) & 1:
            out |= r
        else:
            out &= r
    return out


def dense_layer(built: bytes, share: float, blocked: bool, hashes: int, seed: int) -> bytes:
    """built | random bits of the density that makes `share` of random X's pass the result."""
    r = blocked_random_density(built, share) if blocked else reference_random_density(built, share, hashes)
    return (np.frombuffer(built, dtype=np.uint8) | random_bits(len(built), r, seed)).tobytes()
