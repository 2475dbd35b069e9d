"""The host half of the salvage decode, checked without a GPU: the argument checks of l3c_dmll_conceal (include/l3c_hip.h; every one is made
before anything is launched: fake, well-aligned pointers stand in for device memory), l3c_decode_batch_banded_p_offset on plans of
l3c_decode_plan_banded, and container.failing_bands beside check_band_crcs."""
import ctypes

import numpy as np
import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.bitcoding import container
from tests.test_native_banded_abi import INVALID, _cfg, _err, _plan_rc, _synthetic

FAKE = 0x100000
SPAN = np.dtype([('image', '<i8'), ('pix0', '<i8'), ('npix', '<i8'), ('replace', '<u4'), ('reserved', '<u4')])


def _spans(*rows):
    t = np.zeros(len(rows), dtype=SPAN)
    for i, r in enumerate(rows):
        t[i] = tuple(r) + (0,) * (5 - len(r))
    return t


def _conceal(table, B=2, HW=209, K=10, x_min=0.0, x_max=255.0, L=256, P=FAKE, spans=FAKE, sym=FAKE, host=True, n=None):
    lib = _lib.load()
    return lib.l3c_dmll_conceal(P, B, HW, K, x_min, x_max, L, table.ctypes.data if host else None, spans, len(table) if n is None else n, sym, None)


def test_the_span_table_is_the_declared_struct():
    from l3c_pytorch_amd import ops
    assert SPAN.itemsize == 32 and ops.CONCEAL_SPAN_DTYPE == SPAN
    t = ops.conceal_spans([(1, 128, 81, 5)])
    assert t.tobytes() == _spans((1, 128, 81, 5)).tobytes() and int(t['reserved'][0]) == 0
    assert _lib.load().l3c_abi_version() == 4                      # symbols were added, nothing existing changed


def test_conceal_argument_checks_precede_any_device_call():
    good = _spans((0, 0, 64, 7), (0, 128, 81, 7), (1, 64, 1, 7), (1, 128, 0, 7))
    # nothing to do is success, whatever the pointers: no span, empty spans, spans that replace nothing
    assert _conceal(good, n=0, P=None, spans=None, sym=None) == 0
    assert _conceal(_spans((1, 128, 0, 7), (0, 64, 0, 3))) == 0
    assert _conceal(_spans((0, 0, 64, 0), (1, 128, 81, 0))) == 0
    assert _conceal(good, n=-1) == INVALID and 'n_spans' in _err()
    assert _conceal(good, n=65536) == INVALID and 'n_spans' in _err()
    for kw in (dict(P=None), dict(spans=None), dict(sym=None), dict(host=False)):
        assert _conceal(good, **kw) == INVALID and 'null pointer' in _err(), kw
    assert _conceal(good, spans=FAKE + 4) == INVALID and '8-byte aligned' in _err()
    for B, HW in ((0, 209), (-1, 209), (65536, 209), (2, 0), (2, -5)):
        assert _conceal(good, B=B, HW=HW) == INVALID and 'bad shape' in _err(), (B, HW)
    for K in (0, -1, 17):
        assert _conceal(good, K=K) == INVALID and 'K out of range' in _err(), K
    for x_min, x_max, L in ((0.0, 255.0, 1), (0.0, 255.0, 32769), (1.0, 1.0, 256), (2.0, 1.0, 256)):
        assert _conceal(good, x_min=x_min, x_max=x_max, L=L) == INVALID and 'alphabet out of range' in _err()
    # every field of a span, and the error names the span
    bad = [((2, 0, 64, 7), 'image'), ((-1, 0, 64, 7), 'image'), ((0, 32, 64, 7), 'multiple of 64'), ((0, 1, 1, 7), 'multiple of 64'),
           ((0, -64, 64, 7), 'multiple of 64'), ((0, 0, -1, 7), 'outside the image'), ((0, 192, 18, 7), 'outside the image'),
           ((0, 256, 0, 7), 'outside the image'), ((0, 0, 210, 7), 'outside the image'), ((0, 0, 2 ** 62, 7), 'outside the image'),
           ((0, 0, 64, 8), 'replace'), ((0, 0, 64, 0xffffffff), 'replace'), ((0, 0, 64, 7, 1), 'reserved')]
    for row, needle in bad:
        for at in (0, 2):
            rows = [tuple(r) for r in good.tolist()]
            rows[at] = row
            assert _conceal(_spans(*rows)) == INVALID and needle in _err() and 'span {}'.format(at) in _err(), (row, _err())
    # a span is checked even where it would replace nothing
    assert _conceal(_spans((0, 0, 64, 7), (5, 0, 0, 0))) == INVALID and 'span 1' in _err()
    # K = 16 is the largest tile: it fits (the LDS check passes; the launch itself needs a device and is not reached with n_spans == 0)
    assert _conceal(good, K=16, n=0) == 0


@pytest.mark.parametrize('B,H,W,K', [(1, 64, 96, 4), (2, 64, 96, 4), (1, 136, 200, 16), (3, 320, 88, 64)])
def test_p_offset_lies_inside_the_workspace(B, H, W, K):
    lib = _lib.load()
    cfg = _cfg()
    rc, msg, blob, Hp, Wp, _ = _plan_rc(cfg, [_synthetic(cfg, H, W, K, 3 + b) for b in range(B)])
    assert rc == 0, msg
    plan = np.frombuffer(blob, dtype=np.int64)
    ws = lib.l3c_decode_batch_banded_workspace_bytes(ctypes.byref(cfg), plan.ctypes.data)
    off = lib.l3c_decode_batch_banded_p_offset(ctypes.byref(cfg), plan.ctypes.data)
    assert ws > 0 and off >= 0 and off % 16 == 0 and off % 256 == 0
    # room for B HW 12 K floats, even when the caller's pointer is only 16-byte aligned (the decode rounds it up to 256: at most 240 more)
    assert off + 240 + B * Hp * Wp * 12 * cfg.K * 4 <= ws
    assert off == lib.l3c_decode_batch_banded_p_offset(ctypes.byref(_cfg()), plan.ctypes.data)      # pure


def test_p_offset_refuses_a_bad_blob():
    lib = _lib.load()
    cfg = _cfg()
    rc, msg, blob, _, _, _ = _plan_rc(cfg, [_synthetic(cfg, 64, 96, 4, 1)])
    assert rc == 0, msg
    plan = np.frombuffer(blob, dtype=np.int64)
    po = lib.l3c_decode_batch_banded_p_offset
    assert po(ctypes.byref(cfg), None) < 0
    assert po(None, plan.ctypes.data) < 0
    bad = plan.copy()
    bad[0] ^= 1
    assert po(ctypes.byref(cfg), bad.ctypes.data) == INVALID and 'magic' in _err()
    zeros = np.zeros_like(plan)
    assert po(ctypes.byref(cfg), zeros.ctypes.data) == INVALID
    legacy = np.zeros(lib.l3c_decode_plan_bytes(ctypes.byref(cfg), 1) // 8 + 1, dtype=np.int64)
    assert po(ctypes.byref(cfg), legacy.ctypes.data) == INVALID
    wide = _cfg()
    wide.Cf = 128
    assert po(ctypes.byref(wide), plan.ctypes.data) < 0 and 'Cf' in _err()
    assert po(ctypes.byref(cfg), plan.ctypes.data) >= 0


def test_failing_bands_returns_what_check_band_crcs_raises():
    rng = np.random.RandomState(11)
    H, W, L = 88, 320, 1792
    n = container.n_bands(H * W, L)
    tables = [rng.randint(0, 1 << 32, (3, n), dtype=np.int64).astype(np.uint32) for _ in range(5)]
    frame = [container.combine_band_crcs(t, L, H * W) for t in tables]
    seals = [container.Seal(3, frame[0], 0, L, tables[0]), None, container.Seal(3, frame[2], 0), container.Seal(3, frame[3], 0, L, tables[3]),
             container.Seal(3, frame[4], 0, L, tables[4])]
    paddings = [(1, 2, 3, 2), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 4, 4), (0, 0, 0, 0)]
    words = np.stack(tables).copy()
    frame_words = np.asarray(frame, dtype=np.int64)
    assert container.failing_bands(seals, words, (H, W), paddings, 0, frame_words) == ([], {}, {})
    container.check_band_crcs(seals, words, (H, W), paddings, 0, frame_words)
    for c, j in ((1, 3), (0, 3), (2, 15), (0, 0)):
        words[0, c, j] ^= 0x10
    words[1] ^= 1                      # an unsealed file: its words are ignored
    frame_words[2] ^= 1                # a version-1 seal: the frame word alone
    words[3, 2, 0] ^= 0x80000000       # band 0 of a frame whose first rows are padding
    words[4] ^= 7                      # every band of every channel
    for signed in (False, True):       # the device hands the words out as int32
        w = words.view(np.int32) if signed else words
        failed, bands, rows = container.failing_bands(seals, w, (H, W), paddings, 0, frame_words)
        with pytest.raises(container.SealError) as e:
            container.check_band_crcs(seals, w, (H, W), paddings, 0, frame_words)
        assert e.value.reason == 'pixels' and e.value.failed == failed == [0, 2, 3, 4] and e.value.index == 0
        assert e.value.bands == bands and e.value.rows == rows
        assert bands[0] == [(0, 0), (0, 3), (1, 3), (2, 15)] and sorted(bands) == [0, 3, 4] and 2 not in bands and 1 not in bands
        assert bands[3] == [(2, 0)] and len(bands[4]) == 3 * n
        assert rows == {0: (0, 83), 3: (0, 2), 4: (0, 88)}
    # a window of bands (a region decode): first_band shifts the pairs
    failed, bands, rows = container.failing_bands(seals[:1], words[:1, :, 2:5], (H, W), paddings[:1], 2)
    assert failed == [0] and bands == {0: [(0, 3), (1, 3)]} and rows == {0: (13, 20)}
    with pytest.raises(ValueError, match='words for bands'):
        container.failing_bands(seals[:1], words[:1, :, 2:5], (H, W), paddings[:1], 15)
