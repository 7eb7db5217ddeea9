#!/usr/bin/env python3
"""Rate of -m minikeys on the GPU: one engine call (kh_minikeys_scan) with need_valid = 2^22 from a
fixed base, after a small warm-up call.  Prints one JSON line:

  candidates_per_s / valid_keys_per_s   the call's candidates and valid keys over its wall time (host
                                        clock around the call, which ends in a device synchronise)
  filter_ms, keys_ms                    device time of k_mini_filter / k_mini_keys (kh_kernel_time 5, 6)
  filter_candidates_per_s               candidates the filter launches covered over filter_ms
  keys_per_s                            queue entries the key launches took over keys_ms
  discarded_share                       candidates filtered past the stopping point / candidates filtered

With --reference SECONDS (and oracle/_ref/keyhunt built) it also runs the reference CLI at 16 threads
for that long and records the last stats line's keys/s: valid minikeys per second, which times 256 is
its candidate rate.

usage: python tools/minikeys_rate.py [--need N] [--repeat K] [--reference SECONDS]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BASE = "SG64GZqySYwBm9KxE3wH8R"
ALPHABET = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def engine_rate(need: int, repeat: int) -> dict:
    import keyhunt_amd
    base = [ALPHABET.index(c) for c in BASE[1:]]
    runs = []
    with keyhunt_amd.Engine(0) as e:
        e.set_targets([bytes(20)])
        e.minikeys_scan(base, 1 << 12)  # warm-up: code objects, queue and hit buffers
        for _ in range(repeat):
            e.kernel_time_reset()
            t0 = time.perf_counter()
            _, n_cand, n_valid = e.minikeys_scan(base, need)
            dt = time.perf_counter() - t0
            fl, fms, fpts = e.kernel_time(keyhunt_amd.TIME_MINI_FILTER)
            kl, kms, kpts = e.kernel_time(keyhunt_amd.TIME_MINI_KEYS)
            runs.append({"seconds": dt, "candidates": n_cand, "valid": n_valid,
                         "candidates_per_s": n_cand / dt, "valid_keys_per_s": n_valid / dt,
                         "filter_launches": fl, "filter_ms": fms, "filter_candidates_per_s": fpts / (fms / 1e3),
                         "keys_launches": kl, "keys_ms": kms, "keys_per_s": kpts / (kms / 1e3),
                         "discarded_share": (fpts - n_cand) / fpts})
    best = max(runs, key=lambda r: r["candidates_per_s"])
    return dict(best, need_valid=need, runs=[r["candidates_per_s"] for r in runs])


def reference_rate(seconds: int, threads: int = 16) -> dict | None:
    ref = os.path.join(REPO, "oracle", "_ref", "keyhunt")
    if not os.path.exists(ref):
        return None
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.txt"), "w").write("15azScMmHvFPAQfQafrKr48E9MqRRXSnVv\n")
        p = subprocess.run(["timeout", "-k", "10", str(seconds + 5), ref, "-m", "minikeys", "-f", "t.txt", "-C", BASE,
                            "-n", "0x100000", "-t", str(threads), "-q", "-M", "-s", "10"], cwd=td, capture_output=True)
    lines = re.findall(r"Total (\d+) keys in (\d+) seconds", p.stdout.decode("latin-1"))
    if not lines:
        return None
    total, secs = map(int, lines[-1])
    return {"threads": threads, "seconds": secs, "valid_keys_per_s": total / secs, "candidates_per_s": 256 * total / secs}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--need", type=lambda s: int(s, 0), default=1 << 22)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--reference", type=int, default=0, metavar="SECONDS")
    ap.add_argument("--no-gpu", action="store_true", help="only the reference's rate")
    a = ap.parse_args()
    out = {} if a.no_gpu else engine_rate(a.need, a.repeat)
    if a.reference:
        out["reference"] = reference_rate(a.reference)
    print(json.dumps(out))
