"""Python model of --ptable-cache's FILE.cache, shared by the tests of the table files."""
import hashlib
import struct


def cache_model(rows: bytes) -> bytes:
    """struct bptable_cache_file (keyhunt.cpp:137-143) as build_bptable_cache fills it (186-197)."""
    m3 = len(rows) // 16
    b, pos = [], 0
    for bucket in range(256):
        while pos < m3 and rows[pos * 16] < bucket:
            pos += 1
        b.append(pos)
    b.append(m3)
    return struct.pack("<IIQ16s257Q", 0x42505443, 1, m3, hashlib.md5(rows).digest(), *b)
