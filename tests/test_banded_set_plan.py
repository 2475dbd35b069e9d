"""Set decoding of banded `.l3c` files, the host side (no GPU): the chunk plan of l3c_decode_rgb_entries as a pure function, the slicing
below the entry limit, the argument checks of the new entry point, the workspace bound of the chunk count, and the set planner's batches."""
import ctypes
import struct

import numpy as np
import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib, ops
from l3c_pytorch_amd.bitcoding import container
from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding, band_len, n_bands
from l3c_pytorch_amd.bitcoding.set_decode import SetDecoder
from l3c_pytorch_amd.helpers import dataset_codec

# padded image shapes of a mixed set: one band; a 64-symbol last band at K = 64 (L = 128, n = 33); more than 1 MPix; and some in between
SHAPES = [(8, 8), (40, 104), (1024, 1032), (512, 768), (64, 96), (24, 40), (768, 512), (200, 328)]


def band_entries(shapes, K):
    """-> (hw per image, (pix0, len) of every band of every image in order) at the finest scale."""
    hws, pix0, lens = [], [], []
    for H, W in shapes:
        HW = H * W
        L = band_len(HW, K)
        hws.append(HW)
        for j in range(n_bands(HW, L)):
            pix0.append(j * L)
            lens.append(min(L, HW - j * L))
    return hws, np.asarray(pix0, dtype=np.int64), np.asarray(lens, dtype=np.int64)


def test_the_named_shapes_are_what_the_issue_says():
    assert n_bands(8 * 8, band_len(8 * 8, 64)) == 1
    L = band_len(40 * 104, 64)
    assert L == 128 and n_bands(40 * 104, L) == 33 and 40 * 104 - 32 * L == 64
    assert 1024 * 1032 >= 1 << 20


@pytest.mark.parametrize('K', [4, 64])
@pytest.mark.parametrize('n_chunks', [1, 2, 8, 33, 64])
def test_entries_plan_tiles_every_band(K, n_chunks):
    _, _, lens = band_entries(SHAPES, K)
    start, npix, final, table_off = ops.rgb_entries_plan(lens, n_chunks)
    S = lens.shape[0]
    assert start.shape == npix.shape == table_off.shape == (n_chunks, S) and final.shape == (S,)
    for e in range(S):
        step = 64 * -(-int(lens[e]) // (64 * n_chunks))
        nonempty = [k for k in range(n_chunks) if npix[k, e] > 0]
        assert nonempty == list(range(len(nonempty))) and nonempty, e              # the empty chunks are the trailing ones
        nxt = 0
        for k in nonempty:                                                        # the non-empty chunks tile [0, len) in order
            assert start[k, e] == nxt == k * step
            nxt += int(npix[k, e])
            assert k == nonempty[-1] or npix[k, e] % 64 == 0                       # boundaries on 64-symbol blocks, except the entry's last
        assert nxt == lens[e]
        assert final[e] == nonempty[-1]                                           # exactly one final chunk: the last non-empty one
        assert sum(1 for k in range(n_chunks) if final[e] == k) == 1
        for k in range(n_chunks):                                                 # an empty chunk's first pixel stays inside the entry
            assert 0 <= start[k, e] < lens[e]
    for k in range(n_chunks):                                                     # a step's table slots are disjoint and packed
        lo = table_off[k]
        hi = lo + npix[k] * 514
        order = np.argsort(lo, kind='stable')
        assert (lo[order][1:] >= hi[order][:-1]).all()
        assert hi.max() == npix[k].sum() * 514
    # the whole call never falls to one chunk because one band is 64 symbols long
    if n_chunks > 1:
        assert (npix[1] > 0).any()


def test_entry_slices_respect_the_limit():
    assert ops.ENTRIES_MAX == 65535
    for S, limit in [(1, 65535), (65535, 65535), (65536, 65535), (200000, 65535), (1000, 7), (5, 10 ** 9)]:
        sl = ops.entry_slices(S, limit)
        assert sl[0][0] == 0 and sl[-1][1] == S
        assert all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert all(0 < e - a <= min(limit, 65535) for a, e in sl)
    assert SetDecoder.ENTRY_LIMIT == 65535


def test_entries_entry_point_checks_its_arguments_before_any_launch():
    """Status codes and messages WITHOUT a GPU: every call is refused by its argument checks, before any HIP call.  Fake but well-aligned
    non-null pointers stand in for device memory (never dereferenced on these paths)."""
    lib = _lib.load()
    fake = 0x10000

    def err():
        return lib.l3c_last_error().decode()
    i64p = ctypes.POINTER(_lib.c_i64)
    lens = (_lib.c_i64 * 3)(128, 64, 4096)
    assert lib.l3c_decode_rgb_entries_workspace_bytes(3, lens, 8, 1) > 0
    assert lib.l3c_decode_rgb_entries_workspace_bytes(3, lens, 8, 2) > lib.l3c_decode_rgb_entries_workspace_bytes(3, lens, 8, 1)
    assert lib.l3c_decode_rgb_entries_workspace_bytes(0, lens, 8, 1) == -1
    assert lib.l3c_decode_rgb_entries_workspace_bytes(65536, lens, 8, 1) == -1
    assert lib.l3c_decode_rgb_entries_workspace_bytes(3, None, 8, 1) == -1
    assert lib.l3c_decode_rgb_entries_workspace_bytes(3, lens, 0, 1) == -1
    assert lib.l3c_decode_rgb_entries_workspace_bytes(3, lens, 8, 3) == -1
    assert lib.l3c_decode_rgb_entries_workspace_bytes(3, (_lib.c_i64 * 3)(128, 0, 64), 8, 1) == -1
    # pixbase | hw | pix0 | len of three entries: two bands of one 192-pixel image, one whole 4096-pixel image behind it
    ent = (_lib.c_i64 * 12)(0, 0, 192, 192, 192, 4096, 0, 128, 0, 128, 64, 4096)
    d = _lib.RgbEntriesDesc(fake, fake, fake, 3, 192 + 4096, fake, ctypes.cast(ent, i64p), 10, fake, fake, fake, 8, 1, 1, fake, 1 << 30)

    def rgb(**kw):
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.l3c_decode_rgb_entries(ctypes.byref(d), None, None)
    assert lib.l3c_decode_rgb_entries(None, None, None) == -1 and 'null descriptor' in err()
    assert rgb(entries_dev=None) == -1 and 'null pointer' in err()
    assert rgb(entries_dev=fake, S=70000) == -1 and '65535 entries' in err()
    assert rgb(S=0) == -1 and '65535 entries' in err()
    assert rgb(S=3, n_chunks=0) == -1 and 'chunks' in err()
    assert rgb(n_chunks=5000) == -1 and 'chunks' in err()
    assert rgb(n_chunks=8, lag=2) == -1 and 'side stream' in err()
    assert rgb(lag=3) == -1 and 'lag' in err()
    assert rgb(lag=1, window_mode=3) == -1 and 'window_mode' in err()
    assert rgb(window_mode=1, in_=fake + 2) == -1 and 'misaligned' in err()
    assert rgb(in_=fake, entries_dev=fake + 4) == -1 and 'misaligned' in err()
    assert rgb(entries_dev=fake, workspace=fake + 64) == -1 and '256-byte aligned' in err()
    assert rgb(workspace=fake, K=17) == -1 and 'bad shape' in err()
    assert rgb(K=10, total_pix=4096) == -1 and 'outside the P' in err()              # the second image ends past the buffers
    assert rgb(total_pix=192 + 4096, workspace_bytes=4096) == -1 and 'workspace too small' in err()
    d.workspace_bytes = 1 << 30
    for i, v, what in [(0, -1, 'outside the P'), (3, 0, 'outside the P'), (6, -64, 'outside its image'), (9, 0, 'outside its image'),
                       (10, 128, 'outside its image'), (7, 192, 'outside its image')]:
        old = ent[i]
        ent[i] = v
        assert rgb() == -1 and what in err(), (i, v, err())
        ent[i] = old


@pytest.mark.parametrize('K', [4, 64])
@pytest.mark.parametrize('rgb_window', ['auto', 'never'])
def test_chunk_count_keeps_the_workspace_within_the_legacy_group_decodes(K, rgb_window):
    lib = _lib.load()
    hws, _, lens = band_entries(SHAPES, K)
    pix0, npix = Bitcoding.ragged_rgb_chunk_plan(hws, rgb_window)
    for lag_legacy, lag in [(1, 1), (1, 2), (2, 2)]:
        legacy = lib.l3c_decode_rgb_ragged_workspace_bytes(len(hws), int(npix.sum(axis=1).max()), pix0.shape[0], lag_legacy)
        chunks, fits = Bitcoding.banded_rgb_chunks(hws, lens, rgb_window, lag_legacy, lag)
        ws = ops.rgb_entries_workspace_bytes(lens, chunks, lag)
        print('K', K, rgb_window, 'lags', lag_legacy, lag, 'chunks', chunks, 'workspace', ws, 'legacy', legacy)
        assert 1 <= chunks <= 256
        assert fits and ws <= legacy
        # and the tables of a step are what the plan says: the workspace covers them for every lag slot and channel
        _, npix_b, _, _ = ops.rgb_entries_plan(lens, chunks)
        assert ws >= (2 if lag == 2 else 1) * 3 * int(npix_b.sum(axis=1).max()) * 514


def test_chunk_count_says_so_where_no_count_fits_the_legacy_workspace():
    """A few tiny images: the entries workspace holds its plan arrays ((2 + 3 n) S int64 and S int32), the legacy one does not, and the
    tables are too small to make up for them.  The choice is then reported as not fitting -- never silently -- and is the count with the
    smallest workspace of all; a budget that some count meets is met with the first such count from 8 on, then from 7 down."""
    lib = _lib.load()
    hws, _, lens = band_entries([(8, 8), (8, 8)], 64)
    pix0, npix = Bitcoding.ragged_rgb_chunk_plan(hws, 'auto')
    legacy = lib.l3c_decode_rgb_ragged_workspace_bytes(len(hws), int(npix.sum(axis=1).max()), pix0.shape[0], 1)
    every = {n: ops.rgb_entries_workspace_bytes(lens, n, 1) for n in range(1, 257)}
    chunks, fits = Bitcoding.banded_rgb_chunks(hws, lens, 'auto', 1, 1)
    print('legacy', legacy, 'smallest entries workspace', min(every.values()), 'chunks', chunks, 'fits', fits)
    assert fits == (every[chunks] <= legacy)
    if not fits:
        assert min(every.values()) > legacy and every[chunks] == min(every.values())
    assert ops.rgb_entries_chunks(lens, every[8], 1) == (8, True)
    assert ops.rgb_entries_chunks(lens, every[3], 1) == (max(n for n in range(1, 9) if every[n] <= every[3]), True)
    n, fits = ops.rgb_entries_chunks(lens, min(every.values()) - 1, 1)
    assert not fits and every[n] == min(every.values())


def _banded(shape, K, n_records=4, C=5):
    """A banded file with the framing of a (padded) `shape` image written at band count K; the payloads are empty streams."""
    H, W = shape
    scales = []
    for s in reversed(range(n_records)):
        h, w = H >> s, W >> s
        L = band_len(h * w, K)
        scales.append((C if s else 3, h, w, L))
    return container.write_file((0, 0, 0, 0), scales, [[[b''] * n_bands(h * w, L) for _ in range(Cs)] for Cs, h, w, L in scales], True)


def _legacy(shape, n_records=4, C=5):
    H, W = shape
    scales = [(C if s else 3, H >> s, W >> s) for s in reversed(range(n_records))]
    return container.write_file((0, 0, 0, 0), scales, [[b''] * Cs for Cs, _, _ in scales], False)


def test_set_planner_keeps_formats_and_band_lengths_apart():
    files = {0: _banded((64, 96), 4), 1: _banded((64, 96), 64), 2: _banded((64, 96), 4), 3: _legacy((64, 96)), 4: _banded((128, 96), 4),
             5: _legacy((64, 96)), 6: _banded((64, 96), 64)}
    assert container.band_lengths(files[0]) != container.band_lengths(files[1]) and container.band_lengths(files[3]) is None
    chunks, padded = dataset_codec.plan_decode_set(files, list(range(7)), 16)
    assert sorted(map(tuple, chunks)) == [(0, 2), (1, 6), (3, 5), (4,)]
    assert [padded[chunks.index(c)] for c in ([0, 2], [4])] == [(64, 96), (128, 96)]
    for c in chunks:                                     # every batch parses as ONE decode_batch call
        container.parse_batch([files[i] for i in c])
    chunks, _ = dataset_codec.plan_decode_set(files, [0, 2, 1], 1)
    assert chunks == [[0], [2], [1]]
    # legacy sets are planned as before: by padded shape alone
    legacy = {i: _legacy(s) for i, s in enumerate([(64, 96), (32, 48), (64, 96)])}
    assert dataset_codec.plan_decode_set(legacy, [0, 1, 2], 16) == ([[0, 2], [1]], [(64, 96), (32, 48)])


def test_set_entry_parser():
    a, b = _banded((64, 96), 4), _banded((64, 96), 4)
    records, streams = container.parse_set_entry([a, b])
    assert [r[:3] for r in records] == [(5, 8, 12), (5, 16, 24), (5, 32, 48), (3, 64, 96)]
    assert [r[3] for r in records] == [band_len(h * w, 4) for _, h, w in [r[:3] for r in records]]
    for k, (C, H, W, L) in enumerate(records):
        n = n_bands(H * W, L)
        assert streams.scales[k] == (C * n, H, W) and streams.offset[k].shape == streams.nbytes[k].shape == (2, C * n)
    with pytest.raises(ValueError, match='mixes'):
        container.parse_set_entry([a, _legacy((64, 96))])
    with pytest.raises(ValueError, match='band length'):
        container.parse_set_entry([a, _banded((64, 96), 64)])
    with pytest.raises(ValueError, match='equally sized'):
        container.parse_set_entry([a, _banded((128, 96), 4)])
    with pytest.raises(ValueError, match='truncated'):
        container.parse_set_entry([a, b[:-3]])
    with pytest.raises(ValueError):
        container.parse_set_entry([a, b[:19] + struct.pack('<I', 96) + b[23:]])
