#!/usr/bin/env python3
"""Rate of the taproot search on the GPU: one engine call (kh_taproot_scan) over 2^22 keys from a fixed
start against one absent program, after a small warm-up call (--keys 0x1000000 is one whole default
window, --window 0x100000 four windows of 2^20).  Prints one JSON line with the best of the repeats by
keys_per_s:

  keys_per_s            the call's keys over its wall time (host clock around the call, which ends in a
                        device synchronise)
  tap_ms, tap_keys_per_s  device time of k_tap_keys (kh_kernel_time 7) and the points it took over that
  walk_ms, setup_ms     device time of the KM_DUMP walks (kind 0) and of the lane setups (kind 4)
  walk_share            (walk_ms + setup_ms) / (walk_ms + setup_ms + tap_ms): what a window spends on
                        producing its points
  batch                 the kernel's compiled batch (points per lane and inversion)

With --minikeys it also runs tools/minikeys_rate.py's measurement in the same process and reports the
ratio tap_keys_per_s / k_mini_keys' keys_per_s: the two kernels do the same shape of work per key.

usage: python tools/taproot_rate.py [--keys N] [--window W] [--repeat K] [--minikeys]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
START = 0x7A9207AB0000000000000001


def engine_rate(keys: int, window: int, repeat: int) -> dict:
    import keyhunt_amd
    runs = []
    with keyhunt_amd.Engine(0) as e:
        e.taproot_set_targets([bytes(range(32))])
        e.taproot_set_window(window)
        e.taproot_scan(START, 1 << 12)  # warm-up: code objects, tables, lanes and hit buffers
        batch, _ = e.taproot_stats()
        for _ in range(repeat):
            e.kernel_time_reset()
            t0 = time.perf_counter()
            hits = e.taproot_scan(START, keys)
            dt = time.perf_counter() - t0
            assert not hits
            tl, tms, tpts = e.kernel_time(keyhunt_amd.TIME_TAP_KEYS)
            _, wms, _ = e.kernel_time(keyhunt_amd.engine.TIME_ADDRESS)
            _, sms, _ = e.kernel_time(keyhunt_amd.engine.TIME_SETUP)
            runs.append({"seconds": dt, "keys": keys, "keys_per_s": keys / dt, "tap_launches": tl, "tap_ms": tms,
                         "tap_keys_per_s": tpts / (tms / 1e3), "walk_ms": wms, "setup_ms": sms,
                         "walk_share": (wms + sms) / (wms + sms + tms)})
    best = max(runs, key=lambda r: r["keys_per_s"])
    return dict(best, batch=batch, window=min(window or 1 << 24, keys), runs=[r["keys_per_s"] for r in runs],
                tap_runs=[r["tap_keys_per_s"] for r in runs])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=lambda s: int(s, 0), default=1 << 22)
    ap.add_argument("--window", type=lambda s: int(s, 0), default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--minikeys", action="store_true", help="also k_mini_keys' rate, and the ratio")
    a = ap.parse_args()
    out = engine_rate(a.keys, a.window, a.repeat)
    if a.minikeys:
        import minikeys_rate
        mk = minikeys_rate.engine_rate(1 << 22, a.repeat)
        out["minikeys"] = {k: mk[k] for k in ("keys_per_s", "keys_ms", "keys_launches", "valid", "candidates_per_s")}
        out["tap_over_mini_keys"] = out["tap_keys_per_s"] / mk["keys_per_s"]
    print(json.dumps(out))
