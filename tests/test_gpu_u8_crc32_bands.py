"""-m gpu: l3c_u8_crc32_bands (include/l3c_hip.h, csrc/crc.hip) against zlib.crc32: every band word and every frame word.

The (plane_bytes, band_bytes) pairs are the codec's (the 64x64 image at K = 64, 96x128 at K = 5, 320x88 at K = 16 and K = 1) and the lengths
around every place the kernels change path: the 16-byte load, the 1024-byte row and the 16 KiB chunk a wavefront folds, the 4096-byte row
and 128 KiB tile of l3c_u8_crc32, a last band of one dword, a band longer than the plane's rest, and more bands per plane than the 64 lanes
that combine them (one, two and four bands per lane).  Frames lie frame_stride apart with poison between them, and both outputs lie between
guard words."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROW, CHUNK = 1024, 16384       # csrc/crc_spans.h: WROW, WCHUNK
GUARD = 0x5A5AA5A5

PAIRS = [(4096, 64), (12288, 2496), (28160, 1792), (28160, 28160), (3 * 4096 + 64, 4096), (2 * 4160 + 4096, 4160),
         (2 * 131072 + 192, 131072), (131072 + 128, 131072 + 64), (68, 4), (72, 68),
         # this kernel's own lengths
         (3 * ROW + 1020, ROW), (5 * (ROW + 4), ROW + 4), (2 * CHUNK + ROW + 16, CHUNK), (CHUNK + 4, CHUNK + 4), (3 * (CHUNK + 16), CHUNK + 16),
         (4 * (CHUNK - 4), CHUNK - 4), (2 * CHUNK + 12, 2 * CHUNK + 8), (130 * 64, 64), (200 * 8 + 4, 8), (16, 16), (4, 4)]


def _run(frames, planes, plane_bytes, band_bytes, with_frame=True):
    """frames: uint8 numpy (B, stride) -> (band words (B, planes, n), frame words (B,) or None), guards checked."""
    from l3c_pytorch_amd import _lib, ops
    B, stride = frames.shape
    n = -(-plane_bytes // band_bytes)
    dev = torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)).cuda()
    bands = torch.full((B * planes * n + 8,), GUARD, dtype=torch.int32, device='cuda')
    whole = torch.full((B + 8,), GUARD, dtype=torch.int32, device='cuda')
    n_ws = _lib.load().l3c_u8_crc32_bands_workspace_bytes(B, planes, plane_bytes, band_bytes)
    assert n_ws > 0
    ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
    ops.call('l3c_u8_crc32_bands', ops.ptr(dev), B, planes, plane_bytes, band_bytes, stride, ops.ptr(bands[4:]),
             ops.ptr(whole[4:]) if with_frame else None, ops.ptr(ws), n_ws, ops.stream())
    bands, whole = bands.cpu().numpy(), whole.cpu().numpy()
    assert (bands[:4] == GUARD).all() and (bands[-4:] == GUARD).all() and (whole[:4] == GUARD).all() and (whole[-4:] == GUARD).all()
    if not with_frame:
        assert (whole == GUARD).all()
    return bands[4:-4].view(np.uint32).reshape(B, planes, n), whole[4:-4].view(np.uint32) if with_frame else None


def _want(frames, planes, plane_bytes, band_bytes):
    n = -(-plane_bytes // band_bytes)
    bands = np.zeros((frames.shape[0], planes, n), dtype=np.uint32)
    for b, row in enumerate(frames):
        for c in range(planes):
            plane = row[c * plane_bytes:(c + 1) * plane_bytes].tobytes()
            for j in range(n):
                bands[b, c, j] = zlib.crc32(plane[j * band_bytes:(j + 1) * band_bytes])
    return bands, np.asarray([zlib.crc32(row[:planes * plane_bytes].tobytes()) for row in frames], dtype=np.uint32)


def _check(got, want, what):
    bad = np.argwhere(got[0] != want[0])
    assert bad.shape[0] == 0, (what, 'bands (frame, plane, band)', bad[:8].tolist())
    if got[1] is not None:
        assert got[1].tolist() == want[1].tolist(), (what, 'frames')


@pytest.mark.parametrize('B', [1, 3])
def test_every_band_and_frame_word_is_zlibs(B):
    rng = np.random.RandomState(B)
    for plane_bytes, band_bytes in PAIRS:
        stride = 3 * plane_bytes + 36                                       # poison between the frames
        frames = rng.randint(0, 256, (B, stride)).astype(np.uint8)
        _check(_run(frames, 3, plane_bytes, band_bytes), _want(frames, 3, plane_bytes, band_bytes), (plane_bytes, band_bytes))


def test_one_plane_and_no_frame_output():
    rng = np.random.RandomState(7)
    for plane_bytes, band_bytes in ((28160, 1792), (68, 4), (2 * CHUNK + ROW + 16, CHUNK)):
        frames = rng.randint(0, 256, (2, plane_bytes + 8)).astype(np.uint8)
        _check(_run(frames, 1, plane_bytes, band_bytes), _want(frames, 1, plane_bytes, band_bytes), (plane_bytes, band_bytes))
        frames = rng.randint(0, 256, (2, 3 * plane_bytes)).astype(np.uint8)
        _check(_run(frames, 3, plane_bytes, band_bytes, with_frame=False), _want(frames, 3, plane_bytes, band_bytes), (plane_bytes, band_bytes))


def test_constant_frames_and_gap_bytes():
    """All-zero bands of two lengths tell a missing Z(length), all-0xFF a wrong bit order; the bytes between frames reach no word."""
    for fill in (0, 0xFF):
        frames = np.full((2, 3 * 12288), fill, dtype=np.uint8)
        _check(_run(frames, 3, 12288, 2496), _want(frames, 3, 12288, 2496), fill)
    rng = np.random.RandomState(9)
    frames = rng.randint(0, 256, (3, 3 * 4096 + 64)).astype(np.uint8)
    first = _run(frames, 3, 4096, 64)
    frames[:, 3 * 4096:] ^= 0xFF
    again = _run(frames, 3, 4096, 64)
    assert (first[0] == again[0]).all() and (first[1] == again[1]).all()


def test_the_wrapper_returns_the_same_words():
    from l3c_pytorch_amd import ops
    frames = np.random.RandomState(11).randint(0, 256, (2, 3 * 28160)).astype(np.uint8)
    bands, whole = ops.u8_crc32_bands(torch.from_numpy(frames.reshape(-1)).cuda(), 2, 28160, 1792)
    want = _want(frames, 3, 28160, 1792)
    assert (bands.cpu().numpy().view(np.uint32) == want[0]).all() and whole.cpu().numpy().view(np.uint32).tolist() == want[1].tolist()
