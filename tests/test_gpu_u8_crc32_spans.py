"""-m gpu: l3c_u8_crc32_spans (include/l3c_hip.h, csrc/crc.hip) against zlib.crc32, word for word.

One call hashes spans of different lengths anywhere in one buffer.  With T and S the bytes one thread and one block fold
(l3c_u8_crc32_tile), the lengths are those of tests/test_gpu_u8_crc32.py -- every place the tile code changes path -- plus one span of more
than 64 full tiles, where a lane of the combine step holds more than one tile.  All-zero spans of different lengths tell a missing initial
/ final XOR, all-0xFF ones a wrong bit order; 5000 spans make the tile launch grid-stride."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROW = 4096       # bytes of a tile row: 256 threads x 16
GUARD = np.int32(np.uint32(0xA5A5A5A5).view(np.int32))


def _tile():
    from l3c_pytorch_amd import ops
    return ops.u8_crc32_tile()


def _lengths():
    T, S = _tile()
    return [0, 1, 3, 4, 5, 15, 16, 17, T - 1, T, T + 1, ROW - 1, ROW, ROW + 1, S - 1, S, S + 1, 2 * S + 7, 192, 18432, 66 * S + 5]


def _layout(lengths, rng):
    """The spans laid into a buffer in shuffled order with random gaps (multiples of 4) -> (offsets in the lengths' order, buffer bytes)."""
    offsets, at = [0] * len(lengths), 4 * int(rng.randint(0, 5))
    for k in rng.permutation(len(lengths)):
        offsets[k] = at
        at += (lengths[k] + 3) // 4 * 4 + 4 * int(rng.randint(0, 9))
    return offsets, at


def _crc(buf, offsets, lengths):
    from l3c_pytorch_amd import ops
    dev = torch.from_numpy(buf).cuda() if isinstance(buf, np.ndarray) else buf
    return ops.u8_crc32_spans(dev, offsets, lengths).cpu().numpy().view(np.uint32)


def _want(buf, offsets, lengths):
    return np.asarray([zlib.crc32(buf[o:o + n].tobytes()) for o, n in zip(offsets, lengths)], dtype=np.uint32)


def _hex(words):
    return [hex(int(v)) for v in words]


def test_mixed_lengths_in_one_call_and_the_gaps_never_reach_a_result():
    rng = np.random.RandomState(0)
    lengths = _lengths()
    offsets, total = _layout(lengths, rng)
    buf = rng.randint(0, 256, total).astype(np.uint8)
    got, want = _crc(buf, offsets, lengths), _want(buf, offsets, lengths)
    assert got.tolist() == want.tolist(), (_hex(got), _hex(want))
    inside = np.zeros(total, dtype=bool)
    for o, n in zip(offsets, lengths):
        inside[o:o + n] = True
    assert (~inside).sum() > 0
    buf[~inside] = rng.randint(0, 256, int((~inside).sum()))
    assert _crc(buf, offsets, lengths).tolist() == got.tolist()


@pytest.mark.parametrize('fill', [0, 0xFF])
def test_constant_spans_of_every_length(fill):
    rng = np.random.RandomState(1)
    lengths = _lengths()
    offsets, total = _layout(lengths, rng)
    buf = np.full(total, fill, dtype=np.uint8)
    got, want = _crc(buf, offsets, lengths), _want(buf, offsets, lengths)
    assert got.tolist() == want.tolist(), (fill, _hex(got), _hex(want))


def test_5000_short_spans_make_the_tile_launch_stride():
    rng = np.random.RandomState(2)
    lengths = [int(v) for v in rng.randint(1, 301, 5000)]
    offsets, total = _layout(lengths, rng)
    buf = rng.randint(0, 256, total).astype(np.uint8)
    assert _crc(buf, offsets, lengths).tolist() == _want(buf, offsets, lengths).tolist()


def test_overlapping_spans_and_a_span_that_ends_with_the_buffer():
    rng = np.random.RandomState(3)
    T, S = _tile()
    total = S + ROW + 20
    buf = rng.randint(0, 256, total).astype(np.uint8)
    offsets = [0, 0, 4, ROW, S, total - 5 - (total - 5) % 4, 8, total]
    lengths = [total, S + 1, S, S, ROW + 20, 0, 100, 0]
    lengths[5] = total - offsets[5]                       # ends exactly at data_bytes, as spans 0 and 4 do
    assert offsets[4] + lengths[4] == total and offsets[0] + lengths[0] == total
    assert _crc(buf, offsets, lengths).tolist() == _want(buf, offsets, lengths).tolist()


def test_one_span():
    rng = np.random.RandomState(4)
    T, S = _tile()
    for n in (0, 1, T + 1, 2 * S + 7):
        buf = rng.randint(0, 256, 8 + (n + 3) // 4 * 4).astype(np.uint8)
        assert _crc(buf, [8], [n]).tolist() == _want(buf, [8], [n]).tolist(), n


def test_uniform_spans_give_the_words_of_the_uniform_call():
    from l3c_pytorch_amd import ops
    rng = np.random.RandomState(5)
    T, S = _tile()
    for n_items, n in ((3, 2 * S + 7), (300, 192)):
        stride = (n + 3) // 4 * 4 + 4
        buf = rng.randint(0, 256, n_items * stride).astype(np.uint8)
        dev = torch.from_numpy(buf).cuda()
        uniform = ops.u8_crc32(dev, n_items, n, stride)
        spans = ops.u8_crc32_spans(dev, np.arange(n_items, dtype=np.int64) * stride, [n] * n_items)
        assert torch.equal(spans, uniform), n
        assert spans.cpu().numpy().view(np.uint32).tolist() == _want(buf, [i * stride for i in range(n_items)], [n] * n_items).tolist()


def test_guard_words_around_the_result_and_two_calls_give_the_same_words():
    from l3c_pytorch_amd import ops
    rng = np.random.RandomState(6)
    lengths = _lengths()
    offsets, total = _layout(lengths, rng)
    buf = rng.randint(0, 256, total).astype(np.uint8)
    dev = torch.from_numpy(buf).cuda()
    n = len(lengths)
    words = []
    for _ in range(2):
        store = torch.full((n + 8,), int(GUARD), dtype=torch.int32, device='cuda')
        out = ops.u8_crc32_spans(dev, offsets, lengths, out=store[4:4 + n])
        assert out.data_ptr() == store[4:].data_ptr()
        host = store.cpu().numpy()
        assert (host[:4] == GUARD).all() and (host[4 + n:] == GUARD).all()
        words.append(host[4:4 + n].view(np.uint32).tolist())
    assert words[0] == words[1] == _want(buf, offsets, lengths).tolist()


def test_arguments_are_checked_before_the_launch():
    """Fake, well-aligned pointers stand in for device memory: nothing dereferences them on these paths.  (The same cases run without a GPU
    in tests/test_crc_spans_host.py.)"""
    from tests.test_crc_spans_host import check_rejected_arguments
    check_rejected_arguments()
