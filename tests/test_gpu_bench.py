"""bench.py as a plain run on one GPU: the headline leg alone, --steps timed steps of a fixed piece of
work, and --dump-outputs files that repeat from run to run and hold what the engine itself reports
for the bases of the last timed step."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
BASES = 65536  # per step (--bases): 2^31 giant points, some 1600 first-level candidates
STEPS = 2


def _bench(out_dir):
    t = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "0", "--bases", str(BASES), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300)
    whole = time.perf_counter() - t
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {n[:-4]: np.load(os.path.join(out_dir, n)) for n in sorted(os.listdir(out_dir))}, whole


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return [_bench(tmp_path_factory.mktemp(f"dump{i}")) for i in range(2)]


def test_plain_run_is_the_headline_leg_alone(runs):
    line, _, whole = runs[0]
    assert line["metric"].startswith("Mkeys/s") and line["unit"] == "Mkeys/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u32" and line["steps"] == STEPS and line["full"] is False
    assert line["config"]["bases_per_step"] == BASES
    # value: keys of the timed steps (2N per base, N = 2^44) over their time
    assert line["value"] == pytest.approx(STEPS * BASES * (2 << 44) / (STEPS * line["ms_per_step"] / 1e3) / 1e6, rel=1e-9)
    assert 0 < STEPS * line["ms_per_step"] / 1e3 < whole
    # what --full adds is not run
    assert "secondary" not in line and "tertiary" not in line and list(line["legs"]) == ["bsgs_b125"]
    assert line["cpu_baseline"] is None and line["known_answer"] is None and line["board_sampler"] is None


def test_dumped_outputs_repeat_from_run_to_run(runs):
    (line, a, _), (_, b, _) = runs
    # no key lies in these bases: no found file, and no array without rows
    assert sorted(a) == sorted(b) == ["candidates", "counters"]
    assert line["dumped_outputs"] == {n: list(v.shape) for n, v in a.items()}
    for n in a:
        assert a[n].dtype == np.float64 and a[n].size and a[n].shape == b[n].shape and (a[n] == b[n]).all(), n
    first_base, bases, points, first_level, _, found = a["counters"].tolist()
    assert (first_base, bases, points, found) == ((STEPS - 1) * BASES, BASES, BASES * 32768, 0)
    assert first_level == len(a["candidates"]) > 0


def test_dumped_candidates_are_the_engines_for_those_bases(runs, engine):
    """The same bases walked by a context of this process: the same candidates and layer-2 masks."""
    import bench
    _, a, _ = runs[0]
    info = engine.bsgs_setup(1 << 44, 128)
    engine.bsgs_build()
    engine.bsgs_set_targets([bench.decompress(bench.PUZZLE125)])
    engine.bsgs_log_candidates(True)
    assert engine.bsgs_scan((1 << 124) + int(a["counters"][0]) * 2 * info.n, BASES) == []
    got = sorted(engine.bsgs_logged_candidates())
    engine.bsgs_log_candidates(False)
    assert [list(r) for r in got] == a["candidates"].tolist()
