"""-m minikeys where natural data never goes: filter blocks that overflow their 256-entry stage, key
launches of many blocks with all eight batch slots and entries skipped in the middle of a lane's
batch, and candidates past 2^32.  Every expected value is the Python model's (tests/_minikeys_model.py).

The dense construction (pinned in tests/test_minikeys_model.py::test_dense_construction_counts): under
the alphabet ALPHABET[:8] + 'A' * 50 every candidate whose changed digits are all >= 8 spells the same
string, so one valid string makes runs of candidates valid: 157,987 of the first 2^18 from DENSE_BASE,
between 51 and 11,400 per filter block of 14,848, 16 of the 18 blocks above the stage's 256."""
import random

import pytest

import keyhunt_amd

import _minikeys_model as M
from test_minikeys_model import DENSE_ALPHA, DENSE_BASE, EXAMPLE, FILTER_BLOCK, X32, around_x32, dense_valid

pytestmark = pytest.mark.gpu
BASES = {"example": EXAMPLE, "carry": "SG64GZqySYwBm9KxE2zzyG", "wrap": "Szzzzzzzzzzzzzzzzzzzzp"}
CARRY_AT = {"example": 34, "carry": 101, "wrap": 11}  # the candidate at the base's first carry out of its last digit
SPAN = 1 << 18


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


@pytest.fixture
def dense(engine):
    engine.minikeys_set_alphabet(DENSE_ALPHA)
    return engine


# -- A. the filter's stage overflow ---------------------------------------------------------------------
def test_dense_valid_one_launch(dense):
    """One launch of 18 blocks, 16 of them past the stage; the queue starts at 2^18/200 + 1024 = 2334
    entries and grows straight to the count, more than a doubling.  Measured: 0.33 s, of which the
    model's walk of the 2^18 candidates (shared with the tests below) is 0.3 s."""
    want = dense_valid()
    assert dense.minikeys_valid(DENSE_BASE, SPAN, cap=len(want) + 64) == want
    entries, redos = dense.minikeys_queue()
    assert redos >= 1 and entries >= len(want)


def test_dense_valid_launch_edges_inside_rows(dense):
    """The same candidates through 263 launches of 1000, whose edges fall inside rows of 58, and through
    16 launches of 2^14 with a queue that starts at 8 entries: no offset lost or doubled at an edge or
    in a redone window.  Measured: 0.08 s."""
    want = dense_valid()
    dense.minikeys_set_window(1000, 0)
    assert dense.minikeys_valid(DENSE_BASE, SPAN, cap=len(want) + 64) == want
    assert dense.minikeys_queue()[1] == 0  # a queue of 1000/200 + 1024 holds any window of 1000
    dense.minikeys_set_window(1 << 14, 8)
    assert dense.minikeys_valid(DENSE_BASE, SPAN, cap=len(want) + 64) == want
    assert dense.minikeys_queue()[1] >= 1


@pytest.mark.parametrize("blocks_in", [0, 2])
@pytest.mark.parametrize("n", [FILTER_BLOCK - 1, FILTER_BLOCK, FILTER_BLOCK + 1])
def test_dense_valid_one_block_and_one_row_more(dense, n, blocks_in):
    """DENSE_BASE's last digit is 0, so candidates 1 .. 58*256 - 1 are exactly one block and candidate
    58*256 is the first of the next block's first row.  From the base itself the block holds 51 valid
    candidates; from the base + 2 blocks it holds 11,050 and overflows.  Measured: under 5 ms each."""
    shift = blocks_in * FILTER_BLOCK
    base = M.digits_from_value(M.value_of(DENSE_BASE) + shift)
    assert base[20] == 0
    want = [o - shift for o in dense_valid() if shift < o <= shift + n]
    assert (len(want) > 256) == (blocks_in == 2) and len(want) > 32
    assert dense.minikeys_valid(base, n, cap=len(want) + 64) == want


# -- B. the scan over a dense queue: entries past the limit in the middle of a lane's batch ---------------
def _dense_targets() -> list[bytes]:
    strings = sorted({M.candidate(DENSE_BASE, o, DENSE_ALPHA) for o in dense_valid() if o <= 1 << 16})
    assert len(strings) == 4
    return [M.h160_of_key(M.key_of(s)) for s in strings]


@pytest.mark.parametrize("queue", [0, 8])
@pytest.mark.parametrize("need", [4095, 4096, 4097])
def test_dense_scan(dense, need, queue):
    """One window of 2^16 candidates: 29,148 unordered queue entries, of which the key kernel computes
    the `need` (to need + 3) at or below the limit and skips the rest wherever they sit in a lane's batch
    of 8.  Every valid candidate is a hit: offsets, ordinals, minikeys and keys equal the model's.  The
    window is fixed because the host counts each hit's ordinal over the whole queue.  Measured: 0.21 s to
    0.23 s each."""
    targets = _dense_targets()
    dense.set_targets(targets)
    dense.minikeys_set_window(1 << 16, queue)
    want = M.scan(DENSE_BASE, need, set(targets), DENSE_ALPHA)
    assert len(want[2]) == want[1] and [h[1] for h in want[2]] == list(range(want[1]))
    if need == 4096:
        assert want[:2] == (32416, 4096)
    hits, n_cand, n_valid = dense.minikeys_scan(DENSE_BASE, need, cap=8192)
    assert (n_cand, n_valid) == want[:2]
    assert [(h.offset, h.ordinal, h.minikey, h.key) for h in hits] == want[2]
    entries, redos = dense.minikeys_queue()
    assert entries >= 29148 and redos >= 1  # from 2^16/200 + 1024 = 1351 entries, or from 8


# -- C. the key kernel through its hook: many blocks, all eight batch slots ----------------------------------
def _offsets(name: str, n: int) -> list[int]:
    """n candidate offsets, valid or not: drawn from [1, 2^40], with those around the base's carry, a
    few above 2^63 and a few duplicates, shuffled."""
    rng = random.Random(f"{name}-{n}")
    at = CARRY_AT[name]
    offs = list(range(at - 2, at + 3)) + [1 << 63, (1 << 63) + 58 ** 6 + 12345, (1 << 64) - 1]
    offs += [rng.randint(1, 1 << 40) for _ in range(n - len(offs) - 3)]
    offs += offs[8:11]
    rng.shuffle(offs)
    assert len(offs) == n
    return offs


def _model_keys(base: list[int], offs: list[int], alphabet: str = M.ALPHABET) -> list[tuple[int, bytes]]:
    keys = [M.key_of(M.candidate(base, o, alphabet)) for o in offs]
    return [(k, M.h160_of_key(k)) for k in keys]


@pytest.mark.parametrize("name,n", [("example", 511), ("carry", 512), ("wrap", 513), ("example", 1053), ("carry", 1053),
                                    ("wrap", 1053), ("example", 4096 + 3)])
def test_keys_many_blocks(engine, name, n):
    """511 / 512 / 513 entries: 64 lanes exactly and one over, batches of 7 and 8; 1053: 132 lanes,
    3 blocks, T = 192 and a ragged t = 5; 4099: 9 blocks.  Measured: 0.05 s (511 to 513), 0.10 s (1053)
    and 0.40 s (4099), the model's point multiplications included."""
    base = M.digits_of(BASES[name])
    offs = _offsets(name, n)
    assert engine.minikeys_keys(base, offs) == _model_keys(base, offs)


def test_keys_many_blocks_dense_alphabet(dense):
    """Under the many-to-one alphabet: 1053 offsets of the first 2^18, a handful of distinct strings.
    Measured: 0.01 s."""
    offs = random.Random("dense").sample(range(1, SPAN + 1), 1053)
    want = _model_keys(DENSE_BASE, offs, DENSE_ALPHA)
    assert 4 < len(set(want)) < 1053
    assert dense.minikeys_keys(DENSE_BASE, offs) == want


# -- D. across candidate 2^32 --------------------------------------------------------------------------------
def test_scan_across_2_to_32(engine):
    """2^24 + 2^16 valid candidates from the example base: 16 windows of 2^28 up to candidate 2^32
    exactly, then smaller ones.  The 275 valid candidates of (2^32 - 2^15, 2^32 + 2^15] are the targets:
    the filter's row and offset arithmetic, the key kernel's odometer and the host's window positions
    all pass 2^32 with 64-bit values or the hits differ.  Absolute ordinals cannot be had from the CPU;
    these are consecutive because every valid candidate of the span is a target.  Measured: 0.31 s."""
    want = around_x32()
    assert len(want) == 275 and want[0][0] > X32 - (1 << 15) and want[-1][0] <= X32 + (1 << 15)
    engine.set_targets([M.h160_of_key(M.key_of(mk)) for _, mk in want])
    need = (1 << 24) + (1 << 16)
    hits, n_cand, n_valid = engine.minikeys_scan(M.digits_of(EXAMPLE), need, cap=1024)
    assert [(h.offset, h.minikey, h.key) for h in hits] == [(o, mk, M.key_of(mk)) for o, mk in want]
    assert [h.ordinal for h in hits] == list(range(hits[0].ordinal, hits[0].ordinal + 275))
    assert abs(hits[0].ordinal - (1 << 24)) < 1 << 15  # 2^24 +- 4096 valid ones below 2^32 (sd 4088)
    assert n_cand % 4 == 0 and n_cand > X32 + (1 << 15)
    assert need <= n_valid <= need + 3
