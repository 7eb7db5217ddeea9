"""-m minikeys on the GPU: the filter kernel (k_mini_filter), the key kernel (k_mini_keys), the chunk
semantics of kh_minikeys_scan and bin/minikeys-amd, all compared exactly with the Python model
(tests/_minikeys_model.py) and with the reference CLI's own run (tests/golden/ref_minikeys.json).

The three bases: the reference's example (995 valid candidates in its first 2^18), one with a four-digit
carry at candidate 101 (990), and one whose top digit wraps to all zeros at its 11th candidate (1084)."""
import json
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import keyhunt_amd
from conftest import DATA, GOLDEN

import _minikeys_model as M
from test_minikeys_model import BASE_LINE, CLI, records

pytestmark = pytest.mark.gpu
REF = json.load(open(os.path.join(GOLDEN, "ref_minikeys.json")))
STDOUT = json.load(open(os.path.join(GOLDEN, "ref_stdout.json")))  # the reference's stats lines (-m rmd160)
BASES = {"example": "SG64GZqySYwBm9KxE3wH8R", "carry": "SG64GZqySYwBm9KxE2zzyG", "wrap": "Szzzzzzzzzzzzzzzzzzzzp"}
COUNTS = {"example": 995, "carry": 990, "wrap": 1084}
SPAN = 1 << 18
_valid = {}


def model_valid(name: str) -> list[int]:
    """The model's valid candidates of the first 2^18 from a base: computed once, never changed."""
    if name not in _valid:
        _valid[name] = tuple(M.valid_offsets(M.digits_of(BASES[name]), SPAN))
    return list(_valid[name])


def h160(base: list[int], off: int) -> bytes:
    return M.h160_of_key(M.key_of(M.candidate(base, off)))


@pytest.fixture(scope="module")
def eng():
    """An engine of this module's own: the window and alphabet settings stay off the shared one."""
    if keyhunt_amd.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    e = keyhunt_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture
def engine(eng):
    eng.minikeys_set_alphabet(None)
    eng.minikeys_set_window(0, 0)
    return eng


def test_model_counts():
    assert {k: len(model_valid(k)) for k in BASES} == COUNTS
    assert model_valid("example")[:3] == [204, 586, 1648]
    assert model_valid("wrap")[0] == 192 and M.candidate(M.digits_of(BASES["wrap"]), 192) == "S111111111111111111148"
    assert M.candidate(M.digits_of(BASES["carry"]), 101) == "SG64GZqySYwBm9KxE31111"


@pytest.mark.parametrize("name", list(BASES))
@pytest.mark.parametrize("window", [1, 3, 4, 63, 64, 65, 4097, SPAN])
def test_valid(engine, name, window):
    want = [o for o in model_valid(name) if o <= window]
    assert model_valid(name)
    assert engine.minikeys_valid(M.digits_of(BASES[name]), window) == want
    if window == SPAN:
        assert len(want) == COUNTS[name]


def test_valid_small_launch_windows(engine):
    """The same candidates through many launches whose edges fall inside rows of 58."""
    engine.minikeys_set_window(1000, 0)
    want = [o for o in model_valid("carry") if o <= 20001]
    assert want and engine.minikeys_valid(M.digits_of(BASES["carry"]), 20001) == want


def test_valid_permuted_alphabet(engine):
    alpha = M.ALPHABET[29:] + M.ALPHABET[:29]
    base = M.digits_of(BASES["example"])
    want = M.valid_offsets(base, 1 << 14, alpha)
    assert want and want != [o for o in model_valid("example") if o <= 1 << 14]
    engine.minikeys_set_alphabet(alpha)
    assert engine.minikeys_valid(base, 1 << 14) == want


def test_keys(engine):
    base = M.digits_of(BASES["example"])
    offs = model_valid("example")[:64]
    got = engine.minikeys_keys(base, offs)
    assert got == [(M.key_of(M.candidate(base, o)), h160(base, o)) for o in offs]
    # any candidate has a key, valid or not: those at the four-digit carry and at the top-digit wrap
    for name, around in (("carry", 101), ("wrap", 11)):
        b = M.digits_of(BASES[name])
        offs = list(range(around - 2, around + 3)) + model_valid(name)[:3]
        assert engine.minikeys_keys(b, offs) == [(M.key_of(M.candidate(b, o)), h160(b, o)) for o in offs]


@pytest.mark.parametrize("name,need,last_two", [("example", 366, (93043, 93044)), ("wrap", 20, (4926, 4928))])
def test_scan_carried_group(engine, name, need, last_two):
    """The need-th valid candidate and the next one share a group of 4: the call walks to the group's
    end, counts need + 1 valid ones and checks the extra key too (ordinal == need)."""
    base = M.digits_of(BASES[name])
    v = model_valid(name)
    assert tuple(v[need - 1:need + 1]) == last_two and (last_two[0] - 1) // 4 == (last_two[1] - 1) // 4
    targets = [h160(base, last_two[1]), h160(base, v[need + 1])]  # the extra key; the next one is not reached
    engine.set_targets(targets)
    hits, n_cand, n_valid = engine.minikeys_scan(base, need)
    want = M.scan(base, need, set(targets))
    assert want[2] and (n_cand, n_valid) == want[:2] == ((last_two[1] + 3) // 4 * 4, need + 1)
    assert [(h.offset, h.ordinal, h.minikey, h.key) for h in hits] == want[2]
    assert hits[0].ordinal == need and hits[0].offset == last_two[1]


def test_scan_known_answer(engine):
    base = M.digits_of(BASES["example"])
    engine.set_targets([M.h160_of_key(M.key_of(REF["known"]))])
    hits, n_cand, n_valid = engine.minikeys_scan(base, 5)
    assert (n_cand, n_valid) == (3000, 5)
    assert [(h.offset, h.ordinal, h.minikey) for h in hits] == [(3000, 4, REF["known"])]
    assert "%x" % hits[0].key == records(REF["keyfound"])[0]["key"]
    hits, n_cand, n_valid = engine.minikeys_scan(base, 4)
    assert (hits, n_cand, n_valid) == ([], 2024, 4)


def _all_targets():
    base = M.digits_of(BASES["example"])
    v = [o for o in model_valid("example") if o <= 1 << 16]
    assert len(v) == 244
    return base, v, [h160(base, o) for o in v]


def test_scan_every_key_a_target(engine):
    base, v, targets = _all_targets()
    engine.set_targets(targets)
    need = 244 - 1  # v[242] and v[243] are in different groups, so the 244th is not reached
    assert (v[242] - 1) // 4 != (v[243] - 1) // 4
    hits, n_cand, n_valid = engine.minikeys_scan(base, need)
    assert n_valid == need and n_cand == (v[242] + 3) // 4 * 4
    assert [(h.offset, h.ordinal) for h in hits] == [(o, i) for i, o in enumerate(v[:need])]
    assert [h.minikey for h in hits] == [M.candidate(base, o) for o in v[:need]]
    assert [h.key for h in hits] == [M.key_of(M.candidate(base, o)) for o in v[:need]]
    hits, n_cand, n_valid = engine.minikeys_scan(base, 244)
    assert (n_cand, n_valid) == ((v[243] + 3) // 4 * 4, 244)
    assert [(h.offset, h.ordinal) for h in hits] == [(o, i) for i, o in enumerate(v)]
    # the same through queue growth: 4096-candidate windows hold about 16 valid ones, the queue starts at 8
    engine.minikeys_set_window(1 << 12, 8)
    again, n_cand2, n_valid2 = engine.minikeys_scan(base, 244)
    entries, redos = engine.minikeys_queue()
    assert redos > 0 and entries > 8
    assert (again, n_cand2, n_valid2) == (hits, n_cand, n_valid)
    engine.minikeys_set_window(0, 0)
    assert engine.minikeys_scan(base, 244) == (hits, n_cand, n_valid)
    assert engine.minikeys_queue()[1] == 0


def test_scan_small_cap_overflows_with_count(engine):
    base, v, targets = _all_targets()
    engine.set_targets(targets[:2])
    r, hits, n_hits, n_cand, n_valid = engine.minikeys_scan_status(base, 4, cap=1)
    assert r == keyhunt_amd.KH_E_OVERFLOW and n_hits == 2 and [h.offset for h in hits] == v[:1]


def test_scan_argument_and_state_errors():
    with keyhunt_amd.Engine(0) as e:
        base = M.digits_of(BASES["example"])
        assert e.minikeys_scan_status(base, 4)[0] == keyhunt_amd.KH_E_STATE  # no targets
        e.set_targets([bytes(20)])
        assert e.minikeys_scan_status(base, 0)[0] == -1
        assert e.minikeys_scan_status(base[:20] + [58], 4)[0] == -1


def test_kernel_time_kinds(engine):
    base = M.digits_of(BASES["example"])
    engine.set_targets([bytes(20)])
    engine.kernel_time_reset()
    _, n_cand, n_valid = engine.minikeys_scan(base, 100)
    la, ms, pts = engine.kernel_time(keyhunt_amd.TIME_MINI_FILTER)
    assert la >= 1 and ms > 0 and pts >= n_cand
    la, ms, pts = engine.kernel_time(keyhunt_amd.TIME_MINI_KEYS)
    assert la >= 1 and ms > 0 and pts >= n_valid


def _run_cli(argv, kill_after):
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(os.path.join(DATA, "minikeys.txt"), td)
        p = subprocess.run(["timeout", "-k", "10", str(kill_after), CLI] + argv, cwd=td, capture_output=True, timeout=120)
        kf = os.path.join(td, "KEYFOUNDKEYFOUND.txt")
        return p, open(kf).read() if os.path.exists(kf) else ""


def test_cli_matches_reference_run():
    """The reference's arguments, one context: stdout from the first base line through the second one,
    and the records (the overlap target twice), equal the reference's; only that much is compared."""
    p, keyfound = _run_cli(REF["argv"] + ["-t", "1", "-s", "0", "-g", "1"], kill_after=6)
    out = p.stdout.decode("latin-1")
    assert p.returncode == 124, out[-2000:] + p.stderr.decode("latin-1")[-2000:]
    want = REF["stdout"][BASE_LINE.search(REF["stdout"]).start():]
    m = BASE_LINE.search(out)
    assert m and out[m.start():m.start() + len(want)] == want
    assert keyfound.startswith(REF["keyfound"])
    assert [r["minikey"] for r in records(REF["keyfound"])] == [REF["known"], REF["overlap"], REF["overlap"]]


def _shape(line: str) -> str:
    return re.sub(r"[MGTPEZY]keys/s", "Xkeys/s", re.sub(r"\d+", "#", line))


def test_cli_stats_line_shape():
    """The stats line (keyhunt.cpp:2904-2950) counts 1024 per step of 1024 valid minikeys: with -M a
    line of its own, otherwise rewritten in place."""
    for extra in (["-M"], ["-q"]):
        p, _ = _run_cli(["-m", "minikeys", "-f", "minikeys.txt", "-C", REF["base"], "-n", "0x100000", "-s", "1",
                         "-g", "1"] + extra, kill_after=4)
        got = re.findall(r"\r?\[\+\] Total \d+ keys in \d+ seconds: [^\r\n]*[\r\n]", p.stdout.decode("latin-1"))
        assert len(got) >= 2, p.stdout[-1000:]
        ref = STDOUT["rmd160_stats_M" if extra == ["-M"] else "rmd160_stats"]["stats_lines"]
        assert {_shape(g) for g in got} <= {_shape(r) for r in ref} | {
            _shape(r).replace("~# Xkeys/s (# keys/s)", "# keys/s") for r in ref}
        totals = [int(re.search(r"Total (\d+) keys", g).group(1)) for g in got]
        assert all(t % 1048576 == 0 for t in totals) and totals[-1] > 0
        for g in got:
            assert (g.endswith("\n") and not g.startswith("\r")) if extra == ["-M"] else (g.startswith("\r") and g.endswith("\r"))
