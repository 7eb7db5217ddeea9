"""The kangaroo search without a GPU: kh_kang_resolve (host only) against the model, the model's own solves
within the bound the method promises, the derivations the model and the library share, and the calls that
refuse without a context."""
import ctypes
import hashlib
import math

import pytest

import _kangaroo as K
import keyhunt_amd
from keyhunt_amd import engine as E

ORDER = K.ORDER
SEEDS = [1, 2, 3, 4]
W24 = (1 << 24) - 1


def planted(seed: int, a: int, W: int) -> int:
    """The key the solve tests plant for a seed: a + SHA-256("planted" || seed) mod (W + 1)."""
    return a + int.from_bytes(hashlib.sha256(b"planted" + seed.to_bytes(8, "little")).digest(), "big") % (W + 1)


@pytest.mark.parametrize("a", [1, ORDER - (1 << 40)])
@pytest.mark.parametrize("sign", ["t-w", "-(t+w)"])
def test_resolve_finds_the_key_of_either_sign(a, sign):
    kp = 0x1234567 if a == 1 else (1 << 39) + 12345
    pub = K.pub_of(a + kp)
    if sign == "t-w":
        t, w = kp + 999_999, 999_999
    else:  # the wild sits on the negated point: t = -(k' + w) mod n as a plain distance
        w = 77_777
        t = (ORDER - kp - w) % ORDER
    assert K.resolve(t, w, a, pub) == a + kp
    assert E.kang_resolve(t, w, a, pub) == a + kp


def test_resolve_refuses_a_pair_that_matches_neither():
    a, kp = 1, 0xABCDEF
    pub = K.pub_of(a + kp)
    assert K.resolve(kp + 5, 4, a, pub) is None
    assert E.kang_resolve(kp + 5, 4, a, pub) is None
    L = keyhunt_amd.lib()
    assert L.kh_kang_resolve(None, b"\0" * 32, b"\0" * 32, b"\0" * 64, ctypes.create_string_buffer(32)) == E.KH_E_ARG


def test_default_jump_table():
    for W in (W24, (1 << 40), (1 << 129) + 5, (1 << 192) - 1):
        jd = K.default_jumps(W)
        jb = W.bit_length() // 2 + 1
        assert len(jd) == 32 and len(set(jd)) == 32 and all(0 < d < (1 << jb) + 32 for d in jd)
        assert jd[0] == (int.from_bytes(hashlib.sha256(b"kh-kangaroo-jump" + bytes([0, jb])).digest(), "big") % (1 << jb) or 1)
        # the mean jump is of the order of sqrt(W): between sqrt(W)/4 and 4 sqrt(W)
        mean = sum(jd) / 32
        assert math.isqrt(W) / 4 < mean < 4 * math.isqrt(W)


def test_seeding_rule_covers_overlapping_intervals():
    W = W24
    for i in range(0, 64, 2):
        d = K.seed_dist(W, 7, i, 0)
        assert W // 2 <= d <= W // 2 + W
    for i in range(1, 64, 2):
        assert 1 <= K.seed_dist(W, 7, i, 0) <= W
    assert K.seed_dist(W, 7, 3, 0) != K.seed_dist(W, 7, 3, 1) != K.seed_dist(W, 8, 3, 1)


def test_default_dp():
    assert K.default_dp(64, W24) == 2          # 8 * 64 * 2^3 = 4096 > sqrt(2^24 - 1)
    assert K.default_dp(1 << 19, (1 << 129)) == 32
    assert K.default_dp(256, 1 << 16) == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_model_solves_within_the_bound(seed):
    a, W = 1, W24
    key = planted(seed, a, W)
    h = K.Herd(K.pub_of(key), a, a + W, 2)
    h.seed_herd(seed, 64)
    bound = 16 * math.isqrt(W)
    assert h.solve(bound, 8) == key
    print(f"seed {seed}: {h.stats}")
    assert h.stats["jumps"] <= bound
    assert h.stats["bad"] == 0


def test_calls_without_a_context_refuse():
    L = keyhunt_amd.lib()
    z32, z64 = b"\0" * 32, b"\0" * 64
    n32, n64 = ctypes.c_uint32(), ctypes.c_uint64()
    assert L.kh_kang_setup(None, z64, z32, z32, 0, None) == E.KH_E_ARG
    assert L.kh_kang_jumps(None, ctypes.create_string_buffer(1024)) == E.KH_E_ARG
    assert L.kh_kang_geometry(None, None, None, None, None) == E.KH_E_ARG
    assert L.kh_kang_set_launch(None, 0) == E.KH_E_ARG
    assert L.kh_kang_set_herd(None, 1, 0, 0, None) == E.KH_E_ARG
    assert L.kh_kang_seed(None, 0, 0) == E.KH_E_ARG
    assert L.kh_kang_step(None, 1, None, 0, ctypes.byref(n32), ctypes.byref(n64)) == E.KH_E_ARG
    assert L.kh_kang_get_herd(None, 0, 1, None, None) == E.KH_E_ARG
    assert L.kh_kang_add_dps(None, None, 0, ctypes.create_string_buffer(32), ctypes.byref(n32)) == E.KH_E_ARG
    assert L.kh_kang_solve(None, 1, ctypes.create_string_buffer(32), ctypes.byref(n32), None) == E.KH_E_ARG
    assert L.kh_kernel_time(None, 8, None, None, None) == E.KH_E_ARG
