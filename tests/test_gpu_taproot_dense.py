"""kh_taproot_scan and k_tap_keys pinned dense: every key of a chunk a target, over several lanes and
windows, with a stride, from key 1, and across the edge of the default window of 2^24 points.

tests/test_gpu_taproot.py has one dense chunk of 1024 keys (one lane, one group, one window) and plants
5 and 7 keys where a chunk has more than one window.  Here a window's KM_DUMP walk has up to four lanes
(and 2^14 at the default window), k_tap_keys runs 512 lanes and more, a ragged last window follows a full
one that sized the lanes and buffers, and every slot is checked.  Expected values come from the model of
BIP-340/341 in tests/_taproot.py alone."""
import pytest

import keyhunt_amd
from keyhunt_amd import KH_KIND_TAPROOT
import _taproot as T

pytestmark = pytest.mark.gpu

START, N_KEYS = (1 << 72) + 0x13579BDF, 4096                     # B1
START_STRIDE, STRIDE, N_STRIDE = (1 << 100) + 0x2468ACE1, 7919, 2048   # B2
START_EDGE, W_DEFAULT = (1 << 80) + 0x0F1E2D3C4B, 1 << 24        # B4


def prog(qx: int) -> bytes:
    return qx.to_bytes(32, "big")


def _model(start, stride, count):
    """Per key start + i stride, walked P += stride G by the model: (point, output key, BIP-340 key)."""
    out = []
    for i, pt in enumerate(T.walk(start, stride, count)):
        k = start + i * stride
        qx = T.output_x(pt[0])
        assert qx is not None
        out.append((pt, prog(qx), k if pt[1] % 2 == 0 else T.N - k))
    return out


@pytest.fixture(scope="module")
def dense():
    """B1's 4096 keys.  On the model alone: both Y parities occur, no tweak reaches n, and for every byte
    position some key's tweak has that byte zero (comb_mult_jac skips zero bytes; a zero lowest byte
    leaves its accumulator empty past the first step)."""
    out = _model(START, 1, N_KEYS)
    assert T.mul_g(START) == out[0][0] and T.mul_g(START + N_KEYS - 1) == out[-1][0]
    odd = sum(pt[1] & 1 for pt, _, _ in out)
    assert N_KEYS // 4 < odd < 3 * N_KEYS // 4
    tweaks = [T.tweak(pt[0]) for pt, _, _ in out]
    assert all(t < T.N for t in tweaks)
    for j in range(32):
        assert any((t >> (8 * j)) & 255 == 0 for t in tweaks), j
    assert len({p for _, p, _ in out}) == N_KEYS
    return out


@pytest.fixture(scope="module")
def dense_stride():
    out = _model(START_STRIDE, STRIDE, N_STRIDE)
    assert T.mul_g(START_STRIDE + (N_STRIDE - 1) * STRIDE) == out[-1][0]
    assert {pt[1] & 1 for pt, _, _ in out} == {0, 1}
    return out


def _scan_dense(e, model, start, stride, window):
    n = len(model)
    e.taproot_set_targets([p for _, p, _ in model])
    e.taproot_set_window(window)
    try:
        hits = e.taproot_scan(start, n, stride=stride, cap=2 * n)
    finally:
        e.taproot_set_window(0)
    assert [h.offset for h in hits] == list(range(n))
    bad = [i for i, h in enumerate(hits) if h.key != model[i][2]]
    assert not bad, (len(bad), bad[:16])
    assert all(h.kind == KH_KIND_TAPROOT and h.compressed for h in hits)


@pytest.mark.parametrize("window", [1024, 2048, 3072, 0])
def test_every_key_of_four_groups_in_windows(engine, dense, window):
    """B1: four windows of one lane, two of two lanes, a full window of three lanes and then a ragged one
    of one lane, one window of four lanes."""
    _scan_dense(engine, dense, START, 1, window)


def test_outputs_of_4096_points_in_one_call(engine, dense):
    """B1: k_tap_keys on 512 lanes (T = 512), all 32 bytes of every output key."""
    assert engine.taproot_stats()[0] * 512 == N_KEYS
    got = engine.taproot_outputs([pt for pt, _, _ in dense])
    bad = [i for i in range(N_KEYS) if got[i] != dense[i][1]]
    assert not bad, (len(bad), bad[:16])


@pytest.mark.parametrize("window", [1024, 0])
def test_every_key_with_a_stride(engine, dense_stride, window):
    """B2: 2048 keys, stride 7919, from above 2^100."""
    _scan_dense(engine, dense_stride, START_STRIDE, STRIDE, window)


def test_the_low_end(engine):
    """B3: the chunk of keys 1..1024, whose first group holds G, 2G and 3G."""
    keys = [1, 2, 3, 512, 513, 514, 1024]
    outs = {k: T.key_output(k) for k in keys + [1025]}
    assert [outs[k][1] for k in (1, 2, 3)] == list(T.SMALL_KEYS.values())
    engine.taproot_set_window(0)
    engine.taproot_set_targets([prog(outs[k][0]) for k in keys + [1025]])
    hits = engine.taproot_scan(1, 1024)
    assert [(h.offset, h.key) for h in hits] == [(k - 1, outs[k][2]) for k in keys]
    assert [h.offset for h in hits] == [0, 1, 2, 511, 512, 513, 1023]


def test_the_default_windows_edge(dense):
    """B4: one call of 2^24 + 2048 keys at the default window: a full window of 2^14 lanes, then a ragged
    one of two.  Afterwards B1's windows of 1024 on the same engine: the lanes and buffers shrink again.
    An engine of its own, so that the session's keeps its memory footprint."""
    n = W_DEFAULT + 2048
    offs = [0, 1, (1 << 23) - 1, 1 << 23, W_DEFAULT - 1024, W_DEFAULT - 1, W_DEFAULT, W_DEFAULT + 1,
            W_DEFAULT + 1023, W_DEFAULT + 1024, W_DEFAULT + 2047]
    assert offs == sorted(offs) and offs[-1] == n - 1
    outs = [T.key_output(START_EDGE + o) for o in offs]
    absent = [T.key_output(START_EDGE - 1), T.key_output(START_EDGE + n)]
    with keyhunt_amd.Engine(0) as e:
        e.taproot_set_window(0)
        e.taproot_set_targets([prog(o[0]) for o in outs + absent])
        hits = e.taproot_scan(START_EDGE, n)
        assert [(h.offset, h.key) for h in hits] == [(o, out[2]) for o, out in zip(offs, outs)]
        _scan_dense(e, dense, START, 1, 1024)
