"""ctypes binding of include/kh_gpu.h (lib/libkh_gpu.so) -- the MI355X engine.

`Engine` mirrors the reference's worker seams (see include/kh_gpu.h for the keyhunt.cpp lines each
call replaces).  There is no CPU path here: if the shared library or the GPU is missing, calls
raise.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
from dataclasses import dataclass

PKG = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG)
LIB_PATH = os.environ.get("KH_LIB") or os.path.join(PKG, "lib", "libkh_gpu.so")
HEADER = os.path.join(REPO, "include", "kh_gpu.h")

KH_MODE_ADDRESS, KH_MODE_XPOINT, KH_MODE_ETH = 0, 1, 2
KH_MODE_ENDO = 0x10  # OR into mode: -e
KH_MODE_P2SH = 0x20  # OR into KH_MODE_ADDRESS: also probe the nested P2SH-P2WPKH digest of each 02/03 hash
KH_SEARCH_COMPRESS, KH_SEARCH_UNCOMPRESS, KH_SEARCH_BOTH = 0, 1, 2
KH_KIND_02, KH_KIND_03, KH_KIND_04, KH_KIND_XPOINT, KH_KIND_ETH = 0, 1, 2, 3, 5
KH_KIND_TAPROOT = 6  # taproot_scan: the point's taproot output key matched a witness program
KH_KIND_ENDO1, KH_KIND_ENDO2, KH_KIND_NEGY = 0x10, 0x20, 0x40
KH_KIND_P2SH = 0x80  # with KH_MODE_P2SH, OR'ed into KH_KIND_02/03: the nested digest matched
TIME_ADDRESS, TIME_XPOINT, TIME_BSGS, TIME_BUILD, TIME_SETUP = 0, 1, 2, 3, 4
KH_LAYER1_REFERENCE, KH_LAYER1_BLOCKED = 0, 1

ORDER_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


class KhError(RuntimeError):
    pass


class KhHit(ctypes.Structure):
    _fields_ = [("key", ctypes.c_uint8 * 32), ("offset", ctypes.c_uint64), ("kind", ctypes.c_uint32),
                ("compressed", ctypes.c_uint32)]


class KhBsgsInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("m", ctypes.c_uint64), ("m2", ctypes.c_uint64), ("m3", ctypes.c_uint64),
                ("aux", ctypes.c_uint64), ("cycles", ctypes.c_uint64), ("bloom_bits", ctypes.c_uint64 * 3),
                ("bloom_bytes", ctypes.c_uint64 * 3), ("bloom_hashes", ctypes.c_uint32 * 3),
                ("layer1_layout", ctypes.c_uint32)]


class KhBsgsFound(ctypes.Structure):
    _fields_ = [("target", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("key", ctypes.c_uint8 * 32)]


class KhSetupForm(ctypes.Structure):
    _fields_ = [("prog", ctypes.c_uint32), ("L", ctypes.c_uint32), ("scalars", ctypes.c_char_p),
                ("s0", ctypes.c_uint8 * 32), ("step", ctypes.c_uint8 * 32), ("list", ctypes.c_char_p),
                ("n_bases", ctypes.c_uint64), ("start", ctypes.c_uint8 * 32), ("t_round", ctypes.c_uint64),
                ("lane_pts", ctypes.c_uint64), ("a_pts", ctypes.c_uint64), ("two_n", ctypes.c_uint64),
                ("m", ctypes.c_uint64), ("h", ctypes.c_uint32)]


class KhMinikeyHit(ctypes.Structure):
    _fields_ = [("key", ctypes.c_uint8 * 32), ("offset", ctypes.c_uint64), ("ordinal", ctypes.c_uint64),
                ("minikey", ctypes.c_char * 24)]


class KhKangDp(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint8 * 32), ("dist", ctypes.c_uint8 * 32), ("index", ctypes.c_uint32),
                ("kind", ctypes.c_uint32)]


class KhKangStats(ctypes.Structure):
    _fields_ = [("jumps", ctypes.c_uint64), ("dps", ctypes.c_uint64), ("same_herd", ctypes.c_uint64),
                ("reseeds", ctypes.c_uint64), ("stalls", ctypes.c_uint64), ("lost", ctypes.c_uint64),
                ("bad", ctypes.c_uint64)]


KH_KANG_TAME, KH_KANG_WILD, KH_KANG_STALL = 0, 1, 0x10
KH_KANG_DP_AUTO = 0xFFFFFFFF
TIME_KANG = 8
MINIKEY_ALPHABET = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
TIME_MINI_FILTER, TIME_MINI_KEYS = 5, 6
TIME_TAP_KEYS = 7
KH_E_ARG, KH_E_STATE, KH_E_OVERFLOW, KH_E_RANGE = -1, -4, -5, -7

_lib = None


def build(jobs: int = 8) -> str:
    subprocess.run(["make", "-s", "-C", PKG, f"-j{jobs}"], check=True)
    return LIB_PATH


def header_symbols() -> list[str]:
    """Every function the C-ABI header declares."""
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char \*)\s*(kh_\w+)\s*\(", txt, re.M)))


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KhError(f"{LIB_PATH} is missing: build the HIP engine first (python -c 'import keyhunt_amd; keyhunt_amd.build()')")
    L = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    u8p = ctypes.c_char_p
    L.kh_strerror.restype = ctypes.c_char_p
    L.kh_last_error.restype = ctypes.c_char_p
    L.kh_last_error.argtypes = [P]
    L.kh_open.argtypes = [ctypes.c_int, ctypes.POINTER(P)]
    L.kh_close.argtypes = [P]
    L.kh_set_geometry.argtypes = [P, ctypes.c_uint32, ctypes.c_uint32]
    L.kh_release_walk.argtypes = [P]
    L.kh_bsgs_placement.argtypes = [P, ctypes.POINTER(ctypes.c_double * 4)]
    L.kh_bsgs_geometry.argtypes = [P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double * 2)]
    L.kh_synchronize.argtypes = [P]
    L.kh_scan_memory.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    L.kh_bsgs_set_bloom_multiplier.argtypes = [P, ctypes.c_uint32]
    L.kh_set_rmd_batch.argtypes = [P, ctypes.c_uint32]
    L.kh_set_targets.argtypes = [P, u8p, ctypes.c_uint64, ctypes.c_uint64]
    L.kh_set_vanity.argtypes = [P, u8p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]
    L.kh_scan.argtypes = [P, u8p, u8p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(KhHit),
                          ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    L.kh_bsgs_setup.argtypes = [P, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(KhBsgsInfo)]
    L.kh_bsgs_set_layer1.argtypes = [P, ctypes.c_uint32]
    L.kh_bsgs_build.argtypes = [P]
    L.kh_bsgs_save.argtypes = [P, ctypes.c_char_p]
    L.kh_bsgs_load.argtypes = [P, ctypes.c_char_p, ctypes.c_uint32]
    L.kh_targets_save.argtypes = [P, ctypes.c_char_p]
    L.kh_targets_load.argtypes = [P, ctypes.c_char_p, ctypes.c_uint32]
    L.kh_bsgs_set_targets.argtypes = [P, u8p, ctypes.c_uint32]
    L.kh_bsgs_scan.argtypes = [P, u8p, ctypes.c_uint64, ctypes.POINTER(KhBsgsFound), ctypes.c_uint32,
                               ctypes.POINTER(ctypes.c_uint32)]
    L.kh_bsgs_scan_list.argtypes = [P, u8p, ctypes.c_uint64, ctypes.POINTER(KhBsgsFound), ctypes.c_uint32,
                                    ctypes.POINTER(ctypes.c_uint32)]
    L.kh_bsgs_reset_found.argtypes = [P]
    L.kh_bsgs_candidates.argtypes = [P, ctypes.POINTER(ctypes.c_uint64)]
    L.kh_bsgs_refine_stats.argtypes = [P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.kh_bsgs_second_masks.argtypes = [P, ctypes.c_uint32, u8p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                       ctypes.POINTER(ctypes.c_uint32)]
    L.kh_bsgs_refine_masks.argtypes = [P, ctypes.c_uint32, u8p, u8p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                       ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32,
                                       ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.kh_setup_centres.argtypes = [P, ctypes.POINTER(KhSetupForm), u8p, u8p]
    L.kh_kernel_time.argtypes = [P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double),
                                 ctypes.POINTER(ctypes.c_uint64)]
    L.kh_kernel_time_reset.argtypes = [P]
    L.kh_pubkeys.argtypes = [P, u8p, ctypes.c_uint32, u8p]
    L.kh_walk_points.argtypes = [P, u8p, u8p, ctypes.c_uint64, u8p, u8p]
    L.kh_hash160.argtypes = [P, u8p, ctypes.c_uint32, u8p]
    L.kh_field_ops.argtypes = [P, u8p, u8p, ctypes.c_uint32, u8p]
    L.kh_bloom_check.argtypes = [P, ctypes.c_uint32, u8p, ctypes.c_uint32, ctypes.c_uint32, u8p]
    L.kh_bloom_check2.argtypes = [P, ctypes.c_uint32, u8p, ctypes.c_uint32, ctypes.c_uint32, u8p, u8p]
    L.kh_digests.argtypes = [P, u8p, ctypes.c_uint32, u8p]
    L.kh_digests_nested.argtypes = [P, u8p, ctypes.c_uint32, u8p]
    L.kh_filter_keys.argtypes = [P, u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    L.kh_tblk_check.argtypes = [P, u8p, ctypes.c_uint32, u8p]
    L.kh_scan_device_hits.argtypes = [P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.kh_get_bloom.argtypes = [P, ctypes.c_uint32, u8p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.kh_bsgs_set_bloom.argtypes = [P, ctypes.c_uint32, u8p, ctypes.c_uint64]
    L.kh_get_bsgs_table.argtypes = [P, u8p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.kh_bsgs_set_table.argtypes = [P, u8p, ctypes.c_uint64]
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.kh_minikeys_set_alphabet.argtypes = [P, ctypes.c_char_p]
    L.kh_minikeys_set_window.argtypes = [P, ctypes.c_uint64, ctypes.c_uint32]
    L.kh_minikeys_scan.argtypes = [P, u8p, ctypes.c_uint64, ctypes.POINTER(KhMinikeyHit), ctypes.c_uint32,
                                   ctypes.POINTER(ctypes.c_uint32), u64p, u64p]
    L.kh_minikeys_valid.argtypes = [P, u8p, ctypes.c_uint64, u64p, ctypes.c_uint64, u64p]
    L.kh_minikeys_keys.argtypes = [P, u8p, u64p, ctypes.c_uint32, u8p]
    L.kh_minikeys_queue.argtypes = [P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.kh_taproot_set_targets.argtypes = [P, u8p, ctypes.c_uint64]
    L.kh_taproot_scan.argtypes = [P, u8p, u8p, ctypes.c_uint64, ctypes.POINTER(KhHit), ctypes.c_uint32,
                                  ctypes.POINTER(ctypes.c_uint32)]
    L.kh_taproot_set_window.argtypes = [P, ctypes.c_uint64]
    L.kh_taproot_outputs.argtypes = [P, u8p, ctypes.c_uint32, u8p]
    L.kh_taproot_stats.argtypes = [P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.kh_kang_setup.argtypes = [P, u8p, u8p, u8p, ctypes.c_uint32, u8p]
    L.kh_kang_jumps.argtypes = [P, u8p]
    L.kh_kang_geometry.argtypes = [P, u32p, u32p, u32p, u32p]
    L.kh_kang_set_launch.argtypes = [P, ctypes.c_uint32]
    L.kh_kang_set_herd.argtypes = [P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u8p]
    L.kh_kang_seed.argtypes = [P, ctypes.c_uint64, ctypes.c_uint32]
    L.kh_kang_step.argtypes = [P, ctypes.c_uint32, ctypes.POINTER(KhKangDp), ctypes.c_uint32, u32p, u64p]
    L.kh_kang_get_herd.argtypes = [P, ctypes.c_uint32, ctypes.c_uint32, u8p, u8p]
    L.kh_kang_add_dps.argtypes = [P, ctypes.POINTER(KhKangDp), ctypes.c_uint32, u8p, u32p]
    L.kh_kang_resolve.argtypes = [u8p, u8p, u8p, u8p, u8p]
    L.kh_kang_solve.argtypes = [P, ctypes.c_uint64, u8p, u32p, ctypes.POINTER(KhKangStats)]
    _lib = L
    return L


def device_count() -> int:
    n = ctypes.c_int(0)
    lib().kh_device_count(ctypes.byref(n))
    return n.value


def be32(v: int) -> bytes:
    return (int(v) % (1 << 256)).to_bytes(32, "big")


def kang_resolve(tame_dist: int, wild_dist: int, start: int, pub: tuple[int, int]) -> int | None:
    """kh_kang_resolve (host only, no context): the key of a tame/wild collision, or None."""
    key = ctypes.create_string_buffer(32)
    r = lib().kh_kang_resolve(be32(tame_dist), be32(wild_dist), be32(start), be32(pub[0]) + be32(pub[1]), key)
    if r < 0:
        raise KhError(f"kh_kang_resolve: {lib().kh_strerror(r).decode()}")
    return int.from_bytes(key.raw, "big") if r else None


@dataclass
class ScanHit:
    key: int
    offset: int
    kind: int
    compressed: bool


@dataclass
class MinikeyHit:
    key: int
    offset: int
    ordinal: int
    minikey: str


class Engine:
    """One device context (kh_open).  Not thread-safe; one Engine per GPU."""

    def __init__(self, device: int = 0, lanes: int = 0, groups_per_launch: int = 0):
        self._ctx = ctypes.c_void_p()
        r = lib().kh_open(device, ctypes.byref(self._ctx))
        if r:
            raise KhError(f"kh_open({device}) failed: {lib().kh_strerror(r).decode()}")
        self.device = device
        if lanes or groups_per_launch:
            self.set_geometry(lanes, groups_per_launch)

    # -- plumbing ------------------------------------------------------------------------------
    def _chk(self, r: int, what: str) -> None:
        if r:
            raise KhError(f"{what}: {lib().kh_strerror(r).decode()} ({lib().kh_last_error(self._ctx).decode()})")

    def close(self) -> None:
        if self._ctx:
            lib().kh_close(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_geometry(self, lanes: int = 0, groups_per_launch: int = 0) -> None:
        self._chk(lib().kh_set_geometry(self._ctx, lanes, groups_per_launch), "kh_set_geometry")

    def bsgs_geometry(self) -> tuple[int, float, float]:
        """(lanes kept for large BSGS calls or 0, giant points/s of the lane count kept, of the other
        one) -- the context's placement calibration (kh_bsgs_geometry)."""
        lanes, rates = ctypes.c_uint32(), (ctypes.c_double * 2)()
        self._chk(lib().kh_bsgs_geometry(self._ctx, ctypes.byref(lanes), ctypes.byref(rates)), "kh_bsgs_geometry")
        return lanes.value, rates[0], rates[1]

    def bsgs_placement(self) -> tuple[bool, list[float]]:
        """(calibration complete, [lanes kept, lanes other, 0.0, 0.0] giant points/s)."""
        rates = (ctypes.c_double * 4)()
        r = lib().kh_bsgs_placement(self._ctx, ctypes.byref(rates))
        if r < 0:
            self._chk(r, "kh_bsgs_placement")
        return r == 1, list(rates)

    def release_walk(self) -> None:
        """Free the walks' lane arrays and inversion pad (kh_release_walk)."""
        self._chk(lib().kh_release_walk(self._ctx), "kh_release_walk")

    def set_rmd_batch(self, group: int) -> None:
        """-m rmd160 --rmd-batch-size: the reference's clamped group size (1024 = the ordinary walk)."""
        self._chk(lib().kh_set_rmd_batch(self._ctx, group), "kh_set_rmd_batch")

    def synchronize(self) -> None:
        self._chk(lib().kh_synchronize(self._ctx), "kh_synchronize")

    # -- address / rmd160 / xpoint -------------------------------------------------------------
    def set_targets(self, rows: list[bytes], bloom_items: int = 0) -> None:
        buf = b"".join(rows)
        assert all(len(r) == 20 for r in rows)
        self._chk(lib().kh_set_targets(self._ctx, buf, len(rows), bloom_items), "kh_set_targets")

    def set_vanity(self, ranges: list[tuple[bytes, bytes]], probe_len: int, bloom_items: int = 0) -> None:
        """Vanity prefixes (kh_set_vanity): hash160 ranges [A, B], the bloom keyed on A's first probe_len bytes."""
        assert all(len(a) == 20 and len(b) == 20 for a, b in ranges)
        buf = b"".join(a + b for a, b in ranges)
        self._chk(lib().kh_set_vanity(self._ctx, buf, len(ranges), probe_len, bloom_items), "kh_set_vanity")

    def targets_save(self, path: str) -> None:
        """Write the -S target file (data_<hex>.dat layout) of the current targets to path."""
        self._chk(lib().kh_targets_save(self._ctx, path.encode()), "kh_targets_save")

    def targets_load(self, path: str, skip_checksum: bool = False) -> None:
        """Targets (rows and bloom, geometry included) from a data_<hex>.dat file, instead of set_targets."""
        self._chk(lib().kh_targets_load(self._ctx, path.encode(), 1 if skip_checksum else 0), "kh_targets_load")

    def scan(self, start: int, n_keys: int, mode: int = KH_MODE_ADDRESS, search: int = KH_SEARCH_BOTH,
             stride: int = 1, cap: int = 4096, endo: bool = False) -> list[ScanHit]:
        """endo: -e (also the endomorphism images; hit kinds then carry KH_KIND_ENDO1/2, KH_KIND_NEGY).
        mode | KH_MODE_P2SH: also the nested P2SH-P2WPKH digests (hit kinds then carry KH_KIND_P2SH)."""
        hits = (KhHit * cap)()
        n = ctypes.c_uint32(0)
        r = lib().kh_scan(self._ctx, be32(start), be32(stride), n_keys, mode | (KH_MODE_ENDO if endo else 0), search,
                          hits, cap, ctypes.byref(n))
        self._chk(r, "kh_scan")
        return [ScanHit(int.from_bytes(bytes(h.key), "big"), h.offset, h.kind, bool(h.compressed))
                for h in hits[: n.value]]

    def scan_status(self, start: int, n_keys: int, mode: int = KH_MODE_ADDRESS, search: int = KH_SEARCH_BOTH,
                    stride: int = 1, cap: int = 4096) -> tuple[int, list[ScanHit]]:
        """kh_scan returning (status, hits) instead of raising: a KH_E_RANGE call (--rmd-batch-size, a
        group centred on the key 0 mod n) still returns the hits of the groups before it."""
        hits = (KhHit * cap)()
        n = ctypes.c_uint32(0)
        r = lib().kh_scan(self._ctx, be32(start), be32(stride), n_keys, mode, search, hits, cap, ctypes.byref(n))
        return r, [ScanHit(int.from_bytes(bytes(h.key), "big"), h.offset, h.kind, bool(h.compressed))
                   for h in hits[: min(n.value, cap)]]

    # -- minikeys ------------------------------------------------------------------------------
    def minikeys_set_alphabet(self, alphabet: str | None = None) -> None:
        """-8: the 58 characters raw digits map to (None = the default base-58 alphabet)."""
        assert alphabet is None or len(alphabet) == 58
        self._chk(lib().kh_minikeys_set_alphabet(self._ctx, alphabet.encode("latin-1") if alphabet else None),
                  "kh_minikeys_set_alphabet")

    def minikeys_set_window(self, candidates_per_launch: int = 0, queue_entries: int = 0) -> None:
        """Candidates per filter launch and the device queue's initial size (0, 0 = automatic)."""
        self._chk(lib().kh_minikeys_set_window(self._ctx, candidates_per_launch, queue_entries),
                  "kh_minikeys_set_window")

    def minikeys_scan_status(self, base: list[int], need_valid: int, cap: int = 4096):
        """kh_minikeys_scan returning (status, hits, n_hits, n_candidates, n_valid) instead of raising."""
        hits = (KhMinikeyHit * max(cap, 1))()
        n, nc, nv = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        r = lib().kh_minikeys_scan(self._ctx, bytes(base), need_valid, hits, cap, ctypes.byref(n), ctypes.byref(nc),
                                   ctypes.byref(nv))
        out = [MinikeyHit(int.from_bytes(bytes(h.key), "big"), h.offset, h.ordinal, h.minikey.decode("latin-1"))
               for h in hits[: min(n.value, cap)]]
        return r, out, n.value, nc.value, nv.value

    def minikeys_scan(self, base: list[int], need_valid: int, cap: int = 4096):
        """One chunk from `base` (21 raw digits): (hits in candidate order, candidates walked, valid ones)."""
        r, out, _, nc, nv = self.minikeys_scan_status(base, need_valid, cap)
        self._chk(r, "kh_minikeys_scan")
        return out, nc, nv

    def minikeys_valid(self, base: list[int], n_candidates: int, cap: int = 0) -> list[int]:
        """The valid candidates among base+1 .. base+n_candidates, ascending (the filter kernel).  With
        more than `cap` of them (0 = n_candidates / 128 + 64) the call is made a second time."""
        n = ctypes.c_uint64(0)
        cap = cap or n_candidates // 128 + 64
        buf = (ctypes.c_uint64 * cap)()
        r = lib().kh_minikeys_valid(self._ctx, bytes(base), n_candidates, buf, cap, ctypes.byref(n))
        if r == KH_E_OVERFLOW:
            cap = n.value
            buf = (ctypes.c_uint64 * cap)()
            r = lib().kh_minikeys_valid(self._ctx, bytes(base), n_candidates, buf, cap, ctypes.byref(n))
        self._chk(r, "kh_minikeys_valid")
        return list(buf[: n.value])

    def minikeys_keys(self, base: list[int], offsets: list[int]) -> list[tuple[int, bytes]]:
        """Per candidate offset (key, hash160(04||X||Y)) as the key kernel computes them."""
        n = len(offsets)
        out = ctypes.create_string_buffer(52 * n)
        self._chk(lib().kh_minikeys_keys(self._ctx, bytes(base), (ctypes.c_uint64 * n)(*offsets), n, out),
                  "kh_minikeys_keys")
        raw = out.raw
        return [(int.from_bytes(raw[52 * i:52 * i + 32], "big"), raw[52 * i + 32:52 * i + 52]) for i in range(n)]

    def minikeys_queue(self) -> tuple[int, int]:
        """(device queue entries, times the last minikeys call grew the queue and redid a window)."""
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(lib().kh_minikeys_queue(self._ctx, ctypes.byref(a), ctypes.byref(b)), "kh_minikeys_queue")
        return a.value, b.value

    # -- taproot -------------------------------------------------------------------------------
    def taproot_set_targets(self, progs: list[bytes]) -> None:
        """The 32-byte witness programs of bc1p... addresses (kept beside set_targets' rows)."""
        assert all(len(p) == 32 for p in progs)
        self._chk(lib().kh_taproot_set_targets(self._ctx, b"".join(progs), len(progs)), "kh_taproot_set_targets")

    def taproot_scan_status(self, start: int, n_keys: int, stride: int = 1, cap: int = 4096):
        """kh_taproot_scan returning (status, hits, n_hits) instead of raising."""
        hits = (KhHit * max(cap, 1))()
        n = ctypes.c_uint32(0)
        r = lib().kh_taproot_scan(self._ctx, be32(start), be32(stride), n_keys, hits, cap, ctypes.byref(n))
        return r, [ScanHit(int.from_bytes(bytes(h.key), "big"), h.offset, h.kind, bool(h.compressed))
                   for h in hits[: min(n.value, cap)]], n.value

    def taproot_scan(self, start: int, n_keys: int, stride: int = 1, cap: int = 4096) -> list[ScanHit]:
        """Keys start + i*stride whose key-path taproot output key is a program of taproot_set_targets, in
        offset order; a hit's key is the BIP-340 secret key of the internal key (n - k where P.y is odd)."""
        r, out, _ = self.taproot_scan_status(start, n_keys, stride, cap)
        self._chk(r, "kh_taproot_scan")
        return out

    def taproot_set_window(self, points: int = 0) -> None:
        """Points per window of taproot_scan (a multiple of 1024, at most 2^24; 0 = the default 2^24)."""
        self._chk(lib().kh_taproot_set_window(self._ctx, points), "kh_taproot_set_window")

    def taproot_outputs(self, points: list[tuple[int, int]]) -> list[bytes]:
        """Per point (x, y) the 32-byte output key as the tweak kernel computes it (zeros: t >= n)."""
        n = len(points)
        out = ctypes.create_string_buffer(32 * n)
        buf = b"".join(be32(x) + be32(y) for x, y in points)
        self._chk(lib().kh_taproot_outputs(self._ctx, buf, n, out), "kh_taproot_outputs")
        return [out.raw[32 * i:32 * i + 32] for i in range(n)]

    def taproot_stats(self) -> tuple[int, int]:
        """(the tweak kernel's compiled batch, filter hits the device reported in the last taproot_scan)."""
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(lib().kh_taproot_stats(self._ctx, ctypes.byref(a), ctypes.byref(b)), "kh_taproot_stats")
        return a.value, b.value

    # -- kangaroo ------------------------------------------------------------------------------
    # distinguished points travel as (x, dist, index, kind) tuples of integers
    def kang_setup_status(self, pub: tuple[int, int], start: int, end: int, dp_bits: int = KH_KANG_DP_AUTO,
                          jumps: list[int] = None) -> int:
        jb = b"".join(be32(d) for d in jumps) if jumps is not None else None
        return lib().kh_kang_setup(self._ctx, be32(pub[0]) + be32(pub[1]), be32(start), be32(end), dp_bits, jb)

    def kang_setup(self, pub: tuple[int, int], start: int, end: int, dp_bits: int = KH_KANG_DP_AUTO,
                   jumps: list[int] = None) -> int:
        """Target `pub` with its key in [start, end]; returns KH_KANG_BATCH, the kangaroos per lane."""
        self._chk(self.kang_setup_status(pub, start, end, dp_bits, jumps), "kh_kang_setup")
        return self.kang_geometry()[0]

    def kang_jumps(self) -> list[int]:
        out = ctypes.create_string_buffer(32 * 32)
        self._chk(lib().kh_kang_jumps(self._ctx, out), "kh_kang_jumps")
        return [int.from_bytes(out.raw[32 * j:32 * j + 32], "big") for j in range(32)]

    def kang_geometry(self) -> tuple[int, int, int, int]:
        """(batch, jumps per kangaroo per launch, herd size, dp_bits)."""
        v = [ctypes.c_uint32() for _ in range(4)]
        self._chk(lib().kh_kang_geometry(self._ctx, *[ctypes.byref(x) for x in v]), "kh_kang_geometry")
        return tuple(x.value for x in v)

    def kang_set_launch(self, steps_per_launch: int = 0) -> None:
        self._chk(lib().kh_kang_set_launch(self._ctx, steps_per_launch), "kh_kang_set_launch")

    def kang_set_herd_status(self, total: int, first: int, dists: list[int]) -> int:
        return lib().kh_kang_set_herd(self._ctx, total, first, len(dists), b"".join(be32(d) for d in dists))

    def kang_set_herd(self, total: int, first: int, dists: list[int]) -> None:
        self._chk(self.kang_set_herd_status(total, first, dists), "kh_kang_set_herd")

    def kang_seed(self, seed: int, n_kangaroos: int = 0) -> int:
        """Place the whole herd by the library's rule; returns the herd's size."""
        self._chk(lib().kh_kang_seed(self._ctx, seed, n_kangaroos), "kh_kang_seed")
        return self.kang_geometry()[2]

    @staticmethod
    def _dp_tuple(d: KhKangDp) -> tuple[int, int, int, int]:
        return int.from_bytes(bytes(d.x), "big"), int.from_bytes(bytes(d.dist), "big"), d.index, d.kind

    def kang_step_raw(self, steps: int, buf, cap: int) -> tuple[int, int]:
        """kh_kang_step into a caller's KhKangDp array; (records written, records lost)."""
        n, lost = ctypes.c_uint32(), ctypes.c_uint64()
        self._chk(lib().kh_kang_step(self._ctx, steps, buf, cap, ctypes.byref(n), ctypes.byref(lost)), "kh_kang_step")
        return n.value, lost.value

    def kang_step(self, steps: int, cap: int) -> tuple[list[tuple[int, int, int, int]], int]:
        buf = (KhKangDp * max(1, cap))()
        n, lost = self.kang_step_raw(steps, buf, cap)
        return [self._dp_tuple(buf[i]) for i in range(n)], lost

    def kang_get_herd(self, first: int, n: int) -> list[tuple[int, int, int]]:
        """(x, y, dist) of kangaroos first .. first+n-1."""
        xy, dist = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(32 * n)
        self._chk(lib().kh_kang_get_herd(self._ctx, first, n, xy, dist), "kh_kang_get_herd")
        f = int.from_bytes
        return [(f(xy.raw[64 * i:64 * i + 32], "big"), f(xy.raw[64 * i + 32:64 * i + 64], "big"),
                 f(dist.raw[32 * i:32 * i + 32], "big")) for i in range(n)]

    def kang_add_dps(self, dps: list[tuple[int, int, int, int]]) -> int | None:
        """Feed records to the context's table; the key once it is known, else None."""
        buf = (KhKangDp * max(1, len(dps)))()
        for i, (x, dist, index, kind) in enumerate(dps):
            buf[i].x[:] = be32(x)
            buf[i].dist[:] = be32(dist)
            buf[i].index, buf[i].kind = index, kind
        key, found = ctypes.create_string_buffer(32), ctypes.c_uint32()
        self._chk(lib().kh_kang_add_dps(self._ctx, buf, len(dps), key, ctypes.byref(found)), "kh_kang_add_dps")
        return int.from_bytes(key.raw, "big") if found.value else None

    def kang_solve(self, max_jumps: int) -> tuple[int | None, KhKangStats]:
        key, found, st = ctypes.create_string_buffer(32), ctypes.c_uint32(), KhKangStats()
        self._chk(lib().kh_kang_solve(self._ctx, max_jumps, key, ctypes.byref(found), ctypes.byref(st)), "kh_kang_solve")
        return (int.from_bytes(key.raw, "big") if found.value else None), st

    # -- BSGS ----------------------------------------------------------------------------------
    def bsgs_setup(self, n: int, k: int, layer1: int = None) -> KhBsgsInfo:
        """layer1: KH_LAYER1_BLOCKED (default) or KH_LAYER1_REFERENCE (bit-identical to the reference)."""
        if layer1 is not None:
            self._chk(lib().kh_bsgs_set_layer1(self._ctx, layer1), "kh_bsgs_set_layer1")
        info = KhBsgsInfo()
        self._chk(lib().kh_bsgs_setup(self._ctx, n, k, ctypes.byref(info)), "kh_bsgs_setup")
        return info

    def bsgs_build(self) -> None:
        self._chk(lib().kh_bsgs_build(self._ctx), "kh_bsgs_build")

    def bsgs_save(self, directory: str) -> None:
        """Write the -S table files (keyhunt_bsgs_{4,6,7}_*.blm, keyhunt_bsgs_2_*.tbl) into directory."""
        self._chk(lib().kh_bsgs_save(self._ctx, directory.encode()), "kh_bsgs_save")

    def bsgs_load(self, directory: str, skip_checksum: bool = False) -> None:
        """Load the -S table files instead of bsgs_build (after bsgs_setup)."""
        self._chk(lib().kh_bsgs_load(self._ctx, directory.encode(), 1 if skip_checksum else 0), "kh_bsgs_load")

    def bsgs_set_targets(self, points: list[tuple[int, int]]) -> None:
        buf = b"".join(be32(x) + be32(y) for x, y in points)
        self._chk(lib().kh_bsgs_set_targets(self._ctx, buf, len(points)), "kh_bsgs_set_targets")

    def bsgs_scan(self, start: int, n_bases: int, cap: int = 1024) -> list[tuple[int, int]]:
        out = (KhBsgsFound * cap)()
        n = ctypes.c_uint32(0)
        self._chk(lib().kh_bsgs_scan(self._ctx, be32(start), n_bases, out, cap, ctypes.byref(n)), "kh_bsgs_scan")
        return [(f.target, int.from_bytes(bytes(f.key), "big")) for f in out[: n.value]]

    def bsgs_scan_list(self, bases: list[int], cap: int = 1024) -> list[tuple[int, int]]:
        """Scan an arbitrary list of bases (each walks its own 2N keys)."""
        out = (KhBsgsFound * cap)()
        n = ctypes.c_uint32(0)
        buf = b"".join(be32(b) for b in bases)
        self._chk(lib().kh_bsgs_scan_list(self._ctx, buf, len(bases), out, cap, ctypes.byref(n)), "kh_bsgs_scan_list")
        return [(f.target, int.from_bytes(bytes(f.key), "big")) for f in out[: n.value]]

    def bsgs_reset_found(self) -> None:
        self._chk(lib().kh_bsgs_reset_found(self._ctx), "kh_bsgs_reset_found")

    def bsgs_candidates(self) -> int:
        c = ctypes.c_uint64()
        self._chk(lib().kh_bsgs_candidates(self._ctx, ctypes.byref(c)), "kh_bsgs_candidates")
        return c.value

    def bsgs_refine_stats(self) -> tuple[int, int]:
        """(first-level candidates, layer-2 hits of their second checks) since bsgs_setup."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(lib().kh_bsgs_refine_stats(self._ctx, ctypes.byref(a), ctypes.byref(b)), "kh_bsgs_refine_stats")
        return a.value, b.value

    def bsgs_log_candidates(self, enable: bool = True) -> None:
        self._chk(lib().kh_bsgs_log_candidates(self._ctx, int(enable)), "kh_bsgs_log_candidates")

    def bsgs_logged_candidates(self) -> list[tuple[int, int, int]]:
        """(base ordinal, a, layer-2 mask) of every first-level candidate since bsgs_log_candidates."""
        n = ctypes.c_uint64()
        lib().kh_bsgs_get_candidates(self._ctx, None, None, None, ctypes.c_uint64(0), ctypes.byref(n))
        m = max(n.value, 1)
        b, a, k = (ctypes.c_uint64 * m)(), (ctypes.c_uint32 * m)(), (ctypes.c_uint32 * m)()
        self._chk(lib().kh_bsgs_get_candidates(self._ctx, b, a, k, ctypes.c_uint64(m), ctypes.byref(n)),
                  "kh_bsgs_get_candidates")
        return [(b[i], a[i], k[i]) for i in range(n.value)]

    def bsgs_second_masks(self, target: int, base_keys: list[int]) -> tuple[list[int], list[int]]:
        """(GPU, host) layer-2 masks of bsgs_secondcheck for each base key (parity hook)."""
        n = len(base_keys)
        buf = b"".join(be32(k) for k in base_keys) or bytes(32)
        g, h = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))()
        self._chk(lib().kh_bsgs_second_masks(self._ctx, target, buf, n, g, h), "kh_bsgs_second_masks")
        return list(g[:n]), list(h[:n])

    def bsgs_refine_masks_status(self, target: int, idx: list[int], a_pts: int, t_round: int = 0, start: int = None,
                                 two_n: int = 0, bases: list[int] = None, two_m: int = 0):
        """kh_bsgs_refine_masks returning (status, GPU masks, host masks): k_refine over its own index
        arithmetic, continuous (start, two_n) or list (bases) form; two_m = 0: the tables' 2M."""
        n = len(idx)
        g, h = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))()
        lst = b"".join(be32(b) for b in bases) if bases is not None else None
        r = lib().kh_bsgs_refine_masks(self._ctx, target, be32(start) if start is not None else None, lst,
                                       len(bases) if bases is not None else 0, t_round, a_pts, two_n, two_m,
                                       (ctypes.c_uint64 * max(n, 1))(*idx), n, g, h)
        return r, list(g[:n]), list(h[:n])

    def bsgs_refine_masks(self, target: int, idx: list[int], a_pts: int, t_round: int = 0, start: int = None,
                          two_n: int = 0, bases: list[int] = None, two_m: int = 0) -> tuple[list[int], list[int]]:
        r, g, h = self.bsgs_refine_masks_status(target, idx, a_pts, t_round, start, two_n, bases, two_m)
        self._chk(r, "kh_bsgs_refine_masks")
        return g, h

    # -- measurement ---------------------------------------------------------------------------
    def kernel_time(self, kind: int) -> tuple[int, float, int]:
        la, ms, pts = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint64()
        self._chk(lib().kh_kernel_time(self._ctx, kind, ctypes.byref(la), ctypes.byref(ms), ctypes.byref(pts)),
                  "kh_kernel_time")
        return la.value, ms.value, pts.value

    def kernel_time_reset(self) -> None:
        self._chk(lib().kh_kernel_time_reset(self._ctx), "kh_kernel_time_reset")

    # -- parity hooks --------------------------------------------------------------------------
    def pubkeys(self, scalars: list[int]) -> list[tuple[int, int]]:
        buf = b"".join(be32(s) for s in scalars)
        out = ctypes.create_string_buffer(64 * len(scalars))
        self._chk(lib().kh_pubkeys(self._ctx, buf, len(scalars), out), "kh_pubkeys")
        raw = out.raw
        return [(int.from_bytes(raw[64 * i:64 * i + 32], "big"), int.from_bytes(raw[64 * i + 32:64 * i + 64], "big"))
                for i in range(len(scalars))]

    def setup_centres_status(self, L: int, scalars: list[int] = None, prog: tuple[int, int] = None,
                             bsgs: dict = None, q: tuple[int, int] = None):
        """kh_setup_centres returning (status, raw L x 64 bytes): k_setup's centres [Q +] s_g*G of L lanes.
        Exactly one form: scalars (prog 0), prog = (s0, step) (prog 1), or bsgs = dict(t_round, lane_pts,
        a_pts, m, h and either start, two_n or bases) (prog 2)."""
        f = KhSetupForm()
        f.L = L
        if scalars is not None:
            f.prog = 0
            f.scalars = b"".join(be32(s) for s in scalars)
        elif prog is not None:
            f.prog = 1
            f.s0 = (ctypes.c_uint8 * 32)(*be32(prog[0]))
            f.step = (ctypes.c_uint8 * 32)(*be32(prog[1]))
        else:
            f.prog = 2
            if bsgs.get("bases") is not None:
                f.list = b"".join(be32(b) for b in bsgs["bases"])
                f.n_bases = len(bsgs["bases"])
            f.start = (ctypes.c_uint8 * 32)(*be32(bsgs.get("start", 0)))
            f.two_n = bsgs.get("two_n", 0)
            f.t_round, f.lane_pts, f.a_pts = bsgs.get("t_round", 0), bsgs["lane_pts"], bsgs["a_pts"]
            f.m, f.h = bsgs["m"], bsgs["h"]
        out = ctypes.create_string_buffer(64 * max(L, 1))
        qb = be32(q[0]) + be32(q[1]) if q is not None else None
        r = lib().kh_setup_centres(self._ctx, ctypes.byref(f), qb, out)
        return r, out.raw

    def setup_centres(self, L: int, scalars: list[int] = None, prog: tuple[int, int] = None, bsgs: dict = None,
                      q: tuple[int, int] = None) -> bytes:
        """The centres as L x (x[32] || y[32]) big-endian bytes (see setup_centres_status)."""
        r, raw = self.setup_centres_status(L, scalars, prog, bsgs, q)
        self._chk(r, "kh_setup_centres")
        return raw

    def walk_points(self, start: int, n_points: int, stride: int = 1, need_y: bool = False):
        xs = ctypes.create_string_buffer(32 * n_points)
        ys = ctypes.create_string_buffer(32 * n_points) if need_y else None
        self._chk(lib().kh_walk_points(self._ctx, be32(start), be32(stride), n_points, xs, ys), "kh_walk_points")
        return xs.raw, (ys.raw if need_y else None)

    def hash160(self, points: list[tuple[int, int]]) -> list[tuple[bytes, bytes, bytes]]:
        buf = b"".join(be32(x) + be32(y) for x, y in points)
        out = ctypes.create_string_buffer(60 * len(points))
        self._chk(lib().kh_hash160(self._ctx, buf, len(points), out), "kh_hash160")
        raw = out.raw
        return [(raw[60 * i:60 * i + 20], raw[60 * i + 20:60 * i + 40], raw[60 * i + 40:60 * i + 60])
                for i in range(len(points))]

    def field_ops(self, a: list[int], b: list[int]) -> list[tuple[int, int, int, int, int]]:
        ba = b"".join(be32(x) for x in a)
        bb = b"".join(be32(x) for x in b)
        out = ctypes.create_string_buffer(160 * len(a))
        self._chk(lib().kh_field_ops(self._ctx, ba, bb, len(a), out), "kh_field_ops")
        raw = out.raw
        return [tuple(int.from_bytes(raw[160 * i + 32 * k:160 * i + 32 * k + 32], "big") for k in range(5))
                for i in range(len(a))]

    def bloom_check(self, layer: int, items: list[bytes]) -> list[bool]:
        ln = len(items[0])
        out = ctypes.create_string_buffer(len(items))
        self._chk(lib().kh_bloom_check(self._ctx, layer, b"".join(items), len(items), ln, out), "kh_bloom_check")
        return [b != 0 for b in out.raw]

    def bloom_check2(self, layer: int, items: list[bytes], probe_len: int = 0) -> tuple[list[bool], list[bool]]:
        """(eager, lazy) answers of the device's two probe forms (kh_bloom_check2).  probe_len 1..19
        (layer 0, 20-byte items): the filter keyed on the items' first probe_len bytes."""
        ln = probe_len or len(items[0])
        assert all(len(it) == len(items[0]) for it in items) and (not probe_len or len(items[0]) == 20)
        eager = ctypes.create_string_buffer(len(items))
        lazy = ctypes.create_string_buffer(len(items))
        self._chk(lib().kh_bloom_check2(self._ctx, layer, b"".join(items), len(items), ln, eager, lazy),
                  "kh_bloom_check2")
        return [b != 0 for b in eager.raw], [b != 0 for b in lazy.raw]

    def digests(self, points: list[tuple[int, int]]) -> list[tuple[bytes, bytes, bytes, bytes]]:
        """Per (x, y): hash160(02||X), hash160(03||X) (the walks' interleaved pair form), hash160(04||X||Y)
        and the Ethereum address (kh_digests)."""
        buf = b"".join(be32(x) + be32(y) for x, y in points)
        out = ctypes.create_string_buffer(80 * len(points))
        self._chk(lib().kh_digests(self._ctx, buf, len(points), out), "kh_digests")
        raw = out.raw
        return [tuple(raw[80 * i + 20 * k:80 * i + 20 * k + 20] for k in range(4)) for i in range(len(points))]

    def digests_nested(self, points: list[tuple[int, int]]) -> list[tuple[bytes, bytes]]:
        """Per (x, y): hash160(00 14 || hash160(02||X)) and hash160(00 14 || hash160(03||X)), the nested
        P2SH-P2WPKH digests as the KH_MODE_P2SH walks compute them (kh_digests_nested)."""
        buf = b"".join(be32(x) + be32(y) for x, y in points)
        out = ctypes.create_string_buffer(40 * len(points))
        self._chk(lib().kh_digests_nested(self._ctx, buf, len(points), out), "kh_digests_nested")
        raw = out.raw
        return [(raw[40 * i:40 * i + 20], raw[40 * i + 20:40 * i + 40]) for i in range(len(points))]

    def filter_keys(self, items: list[bytes], length: int) -> list[tuple[int, int]]:
        """Per 20-byte item the filter key pair (a, b) of its first `length` bytes (kh_filter_keys)."""
        assert all(len(it) == 20 for it in items)
        out = (ctypes.c_uint64 * (2 * len(items)))()
        self._chk(lib().kh_filter_keys(self._ctx, b"".join(items), len(items), length, out), "kh_filter_keys")
        return [(out[2 * i], out[2 * i + 1]) for i in range(len(items))]

    def tblk_check(self, items: list[bytes]) -> list[bool]:
        """The walks' probe of 20-byte items against the blocked exact-target filter (kh_tblk_check)."""
        assert all(len(it) == 20 for it in items)
        out = ctypes.create_string_buffer(len(items))
        self._chk(lib().kh_tblk_check(self._ctx, b"".join(items), len(items), out), "kh_tblk_check")
        return [b != 0 for b in out.raw]

    def scan_device_hits(self) -> tuple[int, int]:
        """(filter hits the device reported in the last scan, times that scan redid its chunk)."""
        n, redos = ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(lib().kh_scan_device_hits(self._ctx, ctypes.byref(n), ctypes.byref(redos)), "kh_scan_device_hits")
        return n.value, redos.value

    def get_bloom(self, layer: int) -> bytes:
        nb = ctypes.c_uint64()
        self._chk(lib().kh_get_bloom(self._ctx, layer, None, 0, ctypes.byref(nb)), "kh_get_bloom")
        buf = ctypes.create_string_buffer(nb.value)
        self._chk(lib().kh_get_bloom(self._ctx, layer, buf, nb.value, ctypes.byref(nb)), "kh_get_bloom")
        return buf.raw

    def set_bloom(self, layer: int, data: bytes) -> None:
        """Parity hook: replace BSGS layer 1 or 2 by `data` (get_bloom(layer)'s size and layout)."""
        self._chk(lib().kh_bsgs_set_bloom(self._ctx, layer, data, len(data)), "kh_bsgs_set_bloom")

    def get_bsgs_table(self) -> bytes:
        n = ctypes.c_uint64()
        self._chk(lib().kh_get_bsgs_table(self._ctx, None, 0, ctypes.byref(n)), "kh_get_bsgs_table")
        buf = ctypes.create_string_buffer(16 * n.value)
        self._chk(lib().kh_get_bsgs_table(self._ctx, buf, n.value, ctypes.byref(n)), "kh_get_bsgs_table")
        return buf.raw

    def set_bsgs_table(self, rows: bytes) -> None:
        """--load-ptable: use these 16-byte rows as the bP table (keyhunt.cpp:1871-1892)."""
        self._chk(lib().kh_bsgs_set_table(self._ctx, rows, len(rows) // 16), "kh_bsgs_set_table")
