#!/usr/bin/env python3
"""Rates of the kangaroo search on the GPU, one JSON document on stdout (and in --out FILE).

Default: on a 2^129-key range (the width of the 130-bit puzzle) with the default herd and dp_bits,
  step_jumps_per_s     kh_kang_step alone: jumps over wall time, best of 3 windows of about a second
  kernel_jumps_per_s   the same windows by k_kang_step's device time (kh_kernel_time 8)
  solve_jumps_per_s    kh_kang_solve end to end on a planted key of a 2^96-key range (step, the host table
                       and the placements afresh; the search is not run to its end), best of 3 such windows
  bsgs_points_per_s    the BSGS giant walk's points/s (kh_kernel_time 2, -n 2^44 -k 128) re-measured in the
                       same process: the yardstick a jump is set against
  steps_sweep          k_kang_step's jumps/s by device time at 16, 64, 256 and 1024 jumps per launch, three
                       interleaved rounds of short windows on the same herd, best of the three
and the herd, dp_bits, batch and jumps per launch in use.

usage: python tools/kangaroo_rate.py [--seconds S] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
A129 = 1 << 129
P = 2**256 - 2**32 - 977


def window(e, seconds, steps):
    """kang_step calls of `steps` jumps per kangaroo for about `seconds`: (jumps/s by wall, by device time)."""
    import keyhunt_amd
    n = e.kang_geometry()[2]
    e.kernel_time_reset()
    jumps, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        e.kang_step(steps, 1 << 16)
        jumps += n * steps
    dt = time.perf_counter() - t0
    _, ms, pts = e.kernel_time(keyhunt_amd.TIME_KANG)
    assert pts == jumps
    return jumps / dt, pts / (ms / 1e3)


def bsgs_rate(e):
    import keyhunt_amd
    x = int("33709eb11e0d4439a729f21c2c443dedb727528229713f0065721ba8fa46f00e", 16)
    y = pow((x * x * x + 7) % P, (P + 1) // 4, P)
    info = e.bsgs_setup(1 << 44, 128)
    e.bsgs_build()
    e.bsgs_set_targets([(x, y if not y & 1 else P - y)])
    e.bsgs_scan(1 << 124, 65536)
    best = 0.0
    for i in range(3):
        e.kernel_time_reset()
        e.bsgs_scan((1 << 124) + (i + 1) * 65536 * 2 * info.n, 65536)
        _, ms, pts = e.kernel_time(keyhunt_amd.engine.TIME_BSGS)
        best = max(best, pts / (ms / 1e3))
    return best


def rate(seconds):
    import keyhunt_amd
    with keyhunt_amd.Engine(0) as e:
        key = A129 + 0x123456789ABCDEF0123456789ABCDEF
        pub = e.pubkeys([key])[0]
        batch = e.kang_setup(pub, A129, 2 * A129 - 1)
        herd = e.kang_seed(1)
        _, spl, _, dp = e.kang_geometry()
        window(e, 0.2, spl)  # warm-up
        runs = [window(e, seconds, 4 * spl) for _ in range(3)]
        out = {"range_bits": 129, "herd": herd, "dp_bits": dp, "batch": batch, "steps_per_launch": spl,
               "step_jumps_per_s": max(r[0] for r in runs), "kernel_jumps_per_s": max(r[1] for r in runs),
               "step_runs": [r[0] for r in runs], "kernel_runs": [r[1] for r in runs]}
        sweep = {}
        for _ in range(3):
            for n in (16, 64, 256, 1024):
                e.kang_set_launch(n)
                sweep[str(n)] = max(sweep.get(str(n), 0.0), window(e, 0.3, n)[1])
        e.kang_set_launch(0)
        out["steps_sweep"] = sweep
        # end to end: a planted key in a 2^96 range, windows of the solve loop
        a72 = 1 << 96
        k72 = a72 + 0x9E3779B97F4A7C15F3
        e.kang_setup(e.pubkeys([k72])[0], a72, 2 * a72 - 1)
        herd72 = e.kang_seed(1)
        _, spl72, _, dp72 = e.kang_geometry()
        e.kang_solve(herd72 * spl72)
        sruns, before = [], e.kang_solve(0)[1].jumps
        for _ in range(3):
            t0 = time.perf_counter()
            found, st = e.kang_solve(int(out["step_jumps_per_s"] * seconds))
            dt = time.perf_counter() - t0
            assert found is None
            sruns.append((st.jumps - before) / dt)
            before = st.jumps
        out.update(solve_range_bits=96, solve_herd=herd72, solve_dp_bits=dp72, solve_jumps_per_s=max(sruns),
                   solve_runs=sruns, solve_dps=st.dps, solve_same_herd=st.same_herd, solve_lost=st.lost)
        e.release_walk()
        out["bsgs_points_per_s"] = bsgs_rate(e)
        out["jump_over_bsgs_point"] = out["bsgs_points_per_s"] / out["kernel_jumps_per_s"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=None)
    ap.add_argument("--out")
    a = ap.parse_args()
    doc = rate(a.seconds or 1.0)
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)
