"""The models the device probe path is tested against (tests/test_gpu_probe_path.py), pinned on the
CPU: the oracle's XXH64 against the reference's own at every input length, and the Python model of
the blocked exact-target filter against the split-block layout's specification."""
import json
import os
import random
import struct

from conftest import GOLDEN

import _probe_model as pm
from test_oracle import blk_spec_bits

VEC = json.load(open(os.path.join(GOLDEN, "ref_vectors.json")))
SEED = 0x59F2815B16F81798


def test_xxh64_every_length_vs_reference(oracle):
    """or_xxh64 with the bloom seed and the chained second hash equals the reference's XXH64 for
    lengths 0..32: the 32-byte stripe loop, the 8-byte loop, the 4-byte step and the byte tail."""
    vec = VEC["xxh64_lengths"]
    assert sorted({v["len"] for v in vec}) == list(range(33))
    for v in vec:
        buf = bytes.fromhex(v["buf"])
        assert len(buf) == v["len"]
        a = oracle.xxh64(buf, SEED)
        assert a == int(v["a"], 16), v
        assert oracle.xxh64(buf, a) == int(v["b"], 16), v


def test_bloom_keyed_on_prefix_is_xxh64_of_the_prefix(oracle):
    """oracle.Bloom's positions for a short item are (a + i * b) mod bits with the two XXH64s above, so
    the prefix filters of the GPU tests stand on the pinned hash."""
    rng = random.Random(11)
    bits, _, hashes = oracle.bloom_params(10000)
    for ln in range(1, 21):
        buf = rng.randbytes(ln)
        a = oracle.xxh64(buf, SEED)
        b = oracle.xxh64(buf, a)
        assert oracle.bloom_positions(bits, hashes, buf) == [((a + i * b) % (1 << 64)) % bits for i in range(hashes)]


def _edge_words():
    yield from (0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x11111111, 0x77777777, 0xF0F0F0F0, 0x0000FFFF, 0xABCDABCE, 0x80000001)


def test_target_block_model_vs_layer1_spec(oracle):
    """The exact-target filter uses the blocked layer 1's bit layout with (w0, w1, w2) in the places of
    the big-endian X[8..12), X[12..16), X[16..20): the model's block and masks equal the bits the
    layer-1 specification (test_oracle.blk_spec_bits) gives such an X, for edge and random words."""
    rng = random.Random(12)
    blocks = pm.tblk_blocks(oracle, 10000)
    assert blocks == 6740
    cases = [(a, b, c) for a in _edge_words() for b in _edge_words() for c in _edge_words()]
    cases += [(rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32)) for _ in range(3000)]
    # both sides of a few block boundaries
    for k in (1, 2, blocks // 2, blocks - 1):
        lo = -((-k << 32) // blocks)  # ceil(k * 2^32 / blocks): the first w0 of block k
        assert pm.block_of(lo, blocks) == k and pm.block_of(lo - 1, blocks) == k - 1
        cases += [(lo, rng.getrandbits(32), rng.getrandbits(32)), (lo - 1, rng.getrandbits(32), rng.getrandbits(32))]
    for w0, w1, w2 in cases:
        xb = bytes(8) + struct.pack(">3I", w0, w1, w2) + bytes(12)
        spec = [0, 0, 0, 0]
        blk = None
        for off, bit in blk_spec_bits(xb, blocks):
            blk = off // 16 if blk is None else blk
            assert off // 16 == blk
            spec[(off % 16) // 4] |= bit << (8 * (off % 4))
        assert blk == pm.block_of(w0, blocks)
        assert spec == pm.masks(w1, w2), (hex(w0), hex(w1), hex(w2))


def test_target_block_model_members_and_strangers(oracle):
    """Every inserted row passes; a stranger passes iff its 16 bits are all set, counted bit by bit."""
    rng = random.Random(13)
    blocks = 16
    f = pm.TargetBlockFilter(blocks)
    rows = [rng.randbytes(20) for _ in range(200)]
    for r in rows:
        f.add(r)
    assert all(f.check(r) for r in rows)
    raw = b"".join(struct.pack("<I", w) for w in f.w)
    assert len(raw) == 16 * blocks
    yes = 0
    for _ in range(5000):
        r = rng.randbytes(20)
        w = pm.words(r)
        xb = bytes(8) + struct.pack(">3I", w[0], w[1], w[2]) + bytes(12)
        exp = all(raw[off] & bit for off, bit in blk_spec_bits(xb, blocks))
        assert f.check(r) == exp
        yes += exp
    assert 0 < yes < 5000
