"""A Python model of the reference's minikeys worker (thread_process_minikeys, keyhunt.cpp:3094-3259),
built on hashlib and the CPU oracle's pubkey / hash160_uncomp / h160_to_address.

A minikey is 'S' plus 21 characters of a 58-character alphabet, held as 21 raw digits 0..57.  From a
chunk's base the worker walks base+1, base+2, ... with a base-58 odometer (the top digit wraps to all
zeros), four candidates at a time.  A candidate is valid when SHA-256(22 characters || '?')[0] == 0;
its key is SHA-256(22 characters) read big-endian.  A chunk ends at the first group-of-4 boundary with
at least N valid candidates; the next chunk's base is base + 253*N (increment_minikey_N).
"""
from __future__ import annotations

import functools
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

ALPHABET = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
DIGITS = 21
SPACE = 58 ** DIGITS


def digits_of(minikey: str, alphabet: str = ALPHABET) -> list[int]:
    """The 21 raw digits of a 22-character minikey (its leading 'S' is not a digit)."""
    assert len(minikey) == 22
    return [alphabet.index(c) % 58 for c in minikey[1:]]


def value_of(digits: list[int]) -> int:
    v = 0
    for d in digits:
        v = v * 58 + d
    return v


def digits_from_value(v: int) -> list[int]:
    v %= SPACE
    out = [0] * DIGITS
    for i in range(DIGITS - 1, -1, -1):
        v, out[i] = divmod(v, 58)
    return out


def text_of(digits: list[int], alphabet: str = ALPHABET) -> str:
    return "S" + "".join(alphabet[d] for d in digits)


def candidate(base: list[int], offset: int, alphabet: str = ALPHABET) -> str:
    """Candidate number `offset` (1-based) from `base`: the odometer stepped offset times."""
    return text_of(digits_from_value(value_of(base) + offset), alphabet)


def is_valid(minikey: str) -> bool:
    return hashlib.sha256((minikey + "?").encode("latin-1")).digest()[0] == 0


def key_of(minikey: str) -> int:
    return int.from_bytes(hashlib.sha256(minikey.encode("latin-1")).digest(), "big")


def walk(base: list[int], n_candidates: int, alphabet: str = ALPHABET):
    """(offset, minikey) of candidates 1..n_candidates, stepping the odometer digit by digit as
    increment_minikey_index does (keyhunt.cpp:6520-6536)."""
    d = list(base)
    for off in range(1, n_candidates + 1):
        i = DIGITS - 1
        while True:
            if d[i] < 57:
                d[i] += 1
                break
            d[i] = 0
            if i == 0:
                break
            i -= 1
        yield off, text_of(d, alphabet)


def valid_offsets(base: list[int], n_candidates: int, alphabet: str = ALPHABET) -> list[int]:
    return [off for off, mk in walk(base, n_candidates, alphabet) if is_valid(mk)]


@functools.lru_cache(maxsize=None)
def h160_of_key(key: int) -> bytes:
    import oracle
    x, y = oracle.pubkey(key % oracle.SECP_N)
    return oracle.hash160_uncomp(x, y)


def record_of(minikey: str) -> dict:
    """What the reference prints for a hit on this minikey (keyhunt.cpp:3226-3241): the key through
    GetBase16 (no leading zeros), the uncompressed public key, the address."""
    import oracle
    key = key_of(minikey)
    x, y = oracle.pubkey(key % oracle.SECP_N)
    return {"key": "%x" % key, "pubkey": "04%064x%064x" % (x, y), "minikey": minikey,
            "address": oracle.h160_to_address(oracle.hash160_uncomp(x, y))}


def scan(base: list[int], need_valid: int, targets: set[bytes], alphabet: str = ALPHABET):
    """One engine call: walk groups of 4 until at least need_valid valid candidates have been seen.
    Returns (n_candidates, n_valid, hits) with hits = [(offset, ordinal, minikey, key)] in candidate
    order for every one of the n_valid keys whose hash160(04||X||Y) is a target."""
    assert need_valid > 0
    hits, n_valid, off = [], 0, 0
    it = walk(base, 1 << 62, alphabet)
    while n_valid < need_valid:
        for _ in range(4):
            off, mk = next(it)
            if is_valid(mk):
                if targets and h160_of_key(key_of(mk)) in targets:
                    hits.append((off, n_valid, mk, key_of(mk)))
                n_valid += 1
    return off, n_valid, hits


def minikey_n(n: int) -> tuple[list[int], int]:
    """minikeyN and minikey_n_limit (keyhunt.cpp:1298-1322): the base-58 digits of 253*n filled from
    index 20 down; the limit is one more than the digit count (the digit it then reaches is 0: the
    reference leaves it as malloc gave it, which a fresh heap returns zeroed)."""
    mn = [0] * 22
    aux, i = 253 * n, 20
    while aux and i > 0:
        aux, mn[i] = divmod(aux, 58)
        i -= 1
    return mn, 21 - i


def advance(raw: list[int], n: int) -> list[int]:
    """increment_minikey_N (keyhunt.cpp:6548-6559) on the raw base digits; a digit it leaves at 58
    (the carry out of its last step) is carried upward here, as the host does."""
    mn, limit = minikey_n(n)
    raw = list(raw)
    i, j = 20, 0
    while i > 0 and j < limit:
        raw[i] += mn[i]
        if raw[i] > 57:
            raw[i] %= 58
            raw[i - 1] += 1
        i -= 1
        j += 1
    for k in range(DIGITS - 1, 0, -1):
        if raw[k] > 57:
            raw[k] -= 58
            raw[k - 1] += 1
    raw[0] %= 58
    return raw
