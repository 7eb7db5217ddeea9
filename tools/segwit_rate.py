#!/usr/bin/env python3
"""Rate of -m address -l compress on exact targets with and without KH_MODE_P2SH (the nested
P2SH-P2WPKH probes of --segwit), on one context and one chunk size.  Prints one JSON line.

One measurement: per mode a block of consecutive kh_scan chunks -- one untimed chunk that starts the
lanes, then --repeat timed ones that continue them -- the blocks alternating plain, p2sh, plain, ...
for --rounds rounds.  Per timed chunk two rates:

  keys_per_s          the chunk's keys over its wall time (host clock around kh_scan, which ends in a
                      device synchronise and the hit read-back)
  device_keys_per_s   the same keys over the walk launches' device time (kh_kernel_time 0, HIP events)

and per mode the median and the spread (min, max) of each over all its timed chunks.

With --builds A,B[,...] the measurement runs once per build and round in a fresh process each, the
builds alternating, so that two builds are compared under the same conditions and the run-to-run spread
of one build is seen next to the difference between two.  A build is a libkh_gpu.so (a variant of this
checkout's library, picked through KH_LIB) or a directory: another checkout with its own built
keyhunt_amd package, e.g. the parent commit's.  A build without KH_MODE_P2SH gives its plain rate only.

usage: python tools/segwit_rate.py [--keys N] [--repeat K] [--rounds R] [--builds A,B --build-rounds R]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _summary(runs: list[dict]) -> dict:
    out = {}
    for k in ("keys_per_s", "device_keys_per_s"):
        v = [r[k] for r in runs]
        out[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    out["chunks"] = len(runs)
    return out


def measure(n_keys: int, repeat: int, rounds: int, tree: str) -> dict:
    sys.path.insert(0, tree)
    import keyhunt_amd
    from keyhunt_amd import KH_MODE_ADDRESS, KH_SEARCH_COMPRESS
    modes = [("plain", KH_MODE_ADDRESS)]
    if hasattr(keyhunt_amd, "KH_MODE_P2SH"):
        modes.append(("p2sh", KH_MODE_ADDRESS | keyhunt_amd.KH_MODE_P2SH))
    rng = random.Random(20)
    start = (1 << 70) + rng.getrandbits(64)
    runs = {"plain": [], "p2sh": []}
    with keyhunt_amd.Engine(0) as e:
        e.set_targets([rng.randbytes(20) for _ in range(16)])
        nxt = start
        for _ in range(rounds):
            for name, mode in modes:
                e.scan(nxt, n_keys, mode=mode, search=KH_SEARCH_COMPRESS)  # starts the lanes (and warms up)
                nxt += n_keys
                for _ in range(repeat):
                    e.kernel_time_reset()
                    t0 = time.perf_counter()
                    hits = e.scan(nxt, n_keys, mode=mode, search=KH_SEARCH_COMPRESS)
                    dt = time.perf_counter() - t0
                    assert hits == []
                    launches, ms, pts = e.kernel_time(keyhunt_amd.engine.TIME_ADDRESS)
                    assert pts == n_keys and e.kernel_time(keyhunt_amd.engine.TIME_SETUP)[0] == 0
                    runs[name].append({"keys_per_s": n_keys / dt, "device_keys_per_s": pts / (ms / 1e3)})
                    nxt += n_keys
    out = {"lib": os.path.relpath(keyhunt_amd.LIB_PATH, REPO), "n_keys": n_keys, "repeat": repeat, "rounds": rounds}
    for name, _ in modes:
        out[name] = _summary(runs[name])
    if "p2sh" in out:
        out["p2sh_over_plain"] = (out["p2sh"]["device_keys_per_s"]["median"] /
                                  out["plain"]["device_keys_per_s"]["median"])
    return out


def compare(builds: list[str], build_rounds: int, argv: list[str]) -> dict:
    per = {b: [] for b in builds}
    for _ in range(build_rounds):
        for b in builds:
            env = dict(os.environ)
            env.pop("KH_LIB", None)
            extra = []
            if os.path.isdir(b):
                extra = ["--tree", os.path.abspath(b)]
            else:
                env["KH_LIB"] = os.path.abspath(b)
            p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv + extra, capture_output=True,
                               text=True, env=env, timeout=900)
            if p.returncode:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(p.returncode)
            per[b].append(json.loads(p.stdout.strip().splitlines()[-1]))
    med = {b: {f"{m}_{k}": [r[m][k]["median"] for r in rs] for m in ("plain", "p2sh") if m in rs[0]
               for k in ("device_keys_per_s", "keys_per_s")} for b, rs in per.items()}
    return {"builds": med, "order": "builds alternate, one fresh process per build and round", "runs": per}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=lambda s: int(s, 0), default=1 << 32)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--builds", default="")
    ap.add_argument("--build-rounds", type=int, default=2)
    ap.add_argument("--tree", default=REPO, help="the checkout whose keyhunt_amd package is measured")
    a = ap.parse_args()
    if a.builds:
        print(json.dumps(compare(a.builds.split(","), a.build_rounds,
                                 ["--keys", str(a.keys), "--repeat", str(a.repeat), "--rounds", str(a.rounds)])))
    else:
        print(json.dumps(measure(a.keys, a.repeat, a.rounds, a.tree)))
