"""-m gpu: l3c_u8_crc32 (include/l3c_hip.h, csrc/crc.hip) against zlib.crc32, word for word.

With T and S the bytes one thread and one block fold (l3c_u8_crc32_tile), the lengths sit around every place the kernel changes path: the
empty item, less than a dword, a partial 16-byte load, one thread's run, one 4096-byte row of a tile, one tile, several tiles with a ragged
tail, and the two frame sizes of the codec tests.  All-zero items of different lengths tell a missing initial / final XOR (their plain
remainder is 0 at every length), all-0xFF ones a wrong bit order."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROW = 4096       # bytes of a tile row: 256 threads x 16


def _tile():
    from l3c_pytorch_amd import ops
    return ops.u8_crc32_tile()


def _lengths():
    T, S = _tile()
    return [0, 1, 3, 4, 5, 15, 16, 17, T - 1, T, T + 1, ROW - 1, ROW, ROW + 1, S - 1, S, S + 1, 2 * S + 7, 192, 18432]


def _crc(items, item_bytes, stride=None):
    """items: uint8 numpy (n, stride) -> the kernel's words for the first item_bytes bytes of every row."""
    from l3c_pytorch_amd import ops
    n, stride = items.shape[0], items.shape[1] if stride is None else stride
    dev = torch.from_numpy(np.ascontiguousarray(items).reshape(-1)).cuda()
    if dev.numel() == 0:
        dev = torch.zeros(4, dtype=torch.uint8, device='cuda')
    return ops.u8_crc32(dev, n, item_bytes, stride).cpu().numpy().view(np.uint32)


def _want(items, item_bytes):
    return np.asarray([zlib.crc32(row[:item_bytes].tobytes()) for row in items], dtype=np.uint32)


def test_tile_sizes_are_what_the_header_says():
    T, S = _tile()
    assert T > 0 and S % T == 0 and S % ROW == 0 and T == 16 * (S // ROW)


def test_constant_items_of_every_length():
    for n in _lengths():
        for fill in (0, 0xFF):
            items = np.full((1, (n + 3) // 4 * 4), fill, dtype=np.uint8)
            got, want = _crc(items, n), _want(items, n)
            assert got.tolist() == want.tolist(), (n, fill, hex(got[0]), hex(want[0]))


def test_random_items_of_every_length_three_per_call():
    rng = np.random.RandomState(0)
    for n in _lengths():
        stride = (n + 3) // 4 * 4
        items = rng.randint(0, 256, (3, stride)).astype(np.uint8)
        got, want = _crc(items, n), _want(items, n)
        assert got.tolist() == want.tolist(), (n, [hex(v) for v in got], [hex(v) for v in want])


def test_300_items_in_one_call():
    rng = np.random.RandomState(1)
    T, S = _tile()
    for n in (192, T + 1, 18432):
        items = rng.randint(0, 256, (300, (n + 3) // 4 * 4)).astype(np.uint8)
        assert _crc(items, n).tolist() == _want(items, n).tolist(), n


def test_gap_bytes_between_items_never_reach_a_result():
    rng = np.random.RandomState(2)
    T, S = _tile()
    for n, stride in ((5, 8), (T - 1, T + 4), (ROW + 1, ROW + 32), (S + 1, S + 4096), (18432, 18432 + 64)):
        items = rng.randint(0, 256, (3, stride)).astype(np.uint8)
        first = _crc(items, n)
        assert first.tolist() == _want(items, n).tolist(), (n, stride)
        items[:, n:] = rng.randint(0, 256, (3, stride - n))
        assert _crc(items, n).tolist() == first.tolist(), (n, stride)


def test_two_calls_on_the_same_data_give_the_same_words():
    from l3c_pytorch_amd import ops
    T, S = _tile()
    n = 2 * S + 7
    dev = torch.from_numpy(np.random.RandomState(3).randint(0, 256, 3 * (n + 1)).astype(np.uint8)).cuda()
    a = ops.u8_crc32(dev, 3, n, n + 1)
    b = ops.u8_crc32(dev, 3, n, n + 1)
    assert torch.equal(a, b)
    host = dev.cpu().numpy().reshape(3, n + 1)
    assert a.cpu().numpy().view(np.uint32).tolist() == _want(host, n).tolist()


def test_arguments_are_checked_before_the_launch():
    from l3c_pytorch_amd import _lib
    lib = _lib.load()
    fake = 0x1000
    assert lib.l3c_u8_crc32(fake, 1, 8, 6, fake, fake, 1 << 20, None) == -1 and 'item_stride' in lib.l3c_last_error().decode()
    assert lib.l3c_u8_crc32(fake + 2, 1, 8, 8, fake, fake, 1 << 20, None) == -1 and '4-byte aligned' in lib.l3c_last_error().decode()
    assert lib.l3c_u8_crc32(fake, 1, 8, 8, fake, fake, 4, None) == -1 and 'workspace_bytes too small' in lib.l3c_last_error().decode()
    assert lib.l3c_u8_crc32_workspace_bytes(0, 8) == -1 and lib.l3c_u8_crc32_workspace_bytes(1, -1) == -1
