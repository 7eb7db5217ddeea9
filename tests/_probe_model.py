"""Spec model of the blocked exact-target filter (keyhunt_amd/csrc/kh_kernels.h "Bit positions of the
split-block filters", kh_capi.cpp upload_tblk), written from the text with plain shifts.

A 20-byte target is its five little-endian u32 words w0..w4.  The filter has
blocks = ceil(3 * bits / 128) 16-byte blocks, bits = the reference bloom's bit count for the same item
count; a target lives in block (w0 * blocks) >> 32 and sets 16 bits there, 4 in each little-endian u32
word of the block: word k (< 4) takes s = w1 (k < 2) or w2 (k >= 2), a = s >> 8 * (k % 2), b = a >> 4
and the bits  a & 15,  16 + ((a >> 16) & 15),  b & 15,  16 + ((b >> 16) & 15).  A probe answers yes iff
every bit of the item's four masks is set in its block.
"""
import struct


def tblk_blocks(oracle, items: int) -> int:
    bits, _, _ = oracle.bloom_params(oracle.bloom_entries(items))
    return (3 * bits + 127) // 128


def words(row: bytes) -> tuple[int, int, int, int, int]:
    return struct.unpack("<5I", row)


def block_of(w0: int, blocks: int) -> int:
    return (w0 * blocks) >> 32


def masks(s0: int, s1: int) -> list[int]:
    out = []
    for k in range(4):
        s = s0 if k < 2 else s1
        a = s >> (8 * (k % 2))
        b = a >> 4
        out.append((1 << (a & 15)) | (1 << (16 + ((a >> 16) & 15))) | (1 << (b & 15)) | (1 << (16 + ((b >> 16) & 15))))
    return out


class TargetBlockFilter:
    def __init__(self, blocks: int):
        self.blocks = blocks
        self.w = [0] * (4 * blocks)

    def add(self, row: bytes) -> None:
        w = words(row)
        base = 4 * block_of(w[0], self.blocks)
        for k, m in enumerate(masks(w[1], w[2])):
            self.w[base + k] |= m

    def check(self, row: bytes) -> bool:
        w = words(row)
        base = 4 * block_of(w[0], self.blocks)
        return all(self.w[base + k] & m == m for k, m in enumerate(masks(w[1], w[2])))
