"""The band seal (seal version 2) on the host, no GPU: container.make_seal / split_seal / combine_band_crcs / check_band_crcs against bytes
built by hand with struct and zlib, and against the C side (csrc/seal.h behind l3c_seal_write_bands / l3c_seal_find_bands / l3c_seal_find).
The yardstick is zlib.crc32 throughout."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.bitcoding import container
from tests.conftest import ROOT

INVALID = -1
SEP = b'\x46\xE2\x84\x92'
PAD = (1, 2, 3, 4)


def _body(H=16, W=16, L=64, seed=0):
    """A banded file of two records: (1, H/2, W/2) in one band and the finest (3, H, W) in bands of L, payloads of a few bytes."""
    rng = np.random.RandomState(seed)
    n = container.n_bands(H * W, L)
    coarse_L = 64 * (-(-(H // 2) * (W // 2) // 64))
    finest = [[rng.randint(0, 256, 1 + (c + j) % 4).astype(np.uint8).tobytes() for j in range(n)] for c in range(3)]
    return container.write_file(PAD, [(1, H // 2, W // 2, coarse_L), (3, H, W, L)], [[[b'abc']], finest], True)


def _frame(HW, seed):
    return np.random.RandomState(seed).randint(0, 256, 3 * HW).astype(np.uint8).tobytes()


def _band_crcs(frame, HW, L):
    n = container.n_bands(HW, L)
    return np.asarray([[zlib.crc32(frame[c * HW + j * L:c * HW + min((j + 1) * L, HW)]) for j in range(n)] for c in range(3)], dtype=np.uint32)


def _by_hand(body, generation, frame_crc, model_id, crcs, L):
    n = crcs.shape[1]
    T = 20 + 12 * n
    table = b'L3CT' + struct.pack('<HHI', n, 0, L) + b''.join(struct.pack('<I', int(w)) for w in crcs.reshape(-1)) + struct.pack('<I', T) + SEP
    head = b'L3CS' + struct.pack('<BBHIQ', 2, 0, generation, frame_crc, model_id)
    return table + head + struct.pack('<I', zlib.crc32(body[6:14] + table + head))


def _sealed(H=16, W=16, L=64, seed=0):
    body, frame = _body(H, W, L, seed), _frame(H * W, seed)
    crcs = _band_crcs(frame, H * W, L)
    return body, frame, crcs, body + container.make_seal(body, 3, zlib.crc32(frame), 0x1122334455667788, crcs, L)


def _find_bands(data):
    """l3c_seal_find_bands -> (status, body bytes, (generation, frame_crc, model_id), n, L, offset of the table words in the file), message."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    body, seal, bands = ctypes.c_int64(-7), _lib.Seal(), _lib.SealBands()
    rc = lib.l3c_seal_find_bands(buf, len(data), ctypes.byref(body), ctypes.byref(seal), ctypes.byref(bands))
    at = bands.crc - ctypes.addressof(buf) if bands.crc else None
    return (rc, body.value, (seal.generation, seal.frame_crc, seal.model_id), bands.n, bands.band_len, at), lib.l3c_last_error().decode()


def test_the_layout_is_the_documented_one():
    for H, W, L in ((16, 16, 64), (16, 24, 128), (8, 8, 64)):
        body, frame, crcs, sealed = _sealed(H, W, L, H + W)
        n = container.n_bands(H * W, L)
        s = sealed[len(body):]
        assert s == _by_hand(body, 3, zlib.crc32(frame), 0x1122334455667788, crcs, L)
        assert len(s) == 20 + 12 * n + 24 == container.seal_bands_bytes(n) == _lib.load().l3c_seal_bands_bytes(n)
        assert container.is_sealed(sealed) and sealed[-24:-20] == b'L3CS' and sealed[-28:-24] == SEP and sealed[-20] == 2
        assert struct.unpack('<I', sealed[-32:-28])[0] == 20 + 12 * n                       # T: the table is found from the end
        assert sealed[len(body):len(body) + 4] == b'L3CT'
    assert _lib.load().l3c_seal_bands_bytes(0) == INVALID and _lib.load().l3c_seal_bands_bytes(1025) == INVALID


def test_split_seal_round_trips_and_version_1_is_unchanged():
    body, frame, crcs, sealed = _sealed()
    got, seal = container.split_seal(sealed)
    assert got == body and seal == container.Seal(3, zlib.crc32(frame), 0x1122334455667788, 64, crcs)
    assert seal.band_len == 64 and seal.band_crcs.dtype == np.uint32 and seal.band_crcs.shape == (3, 4) and (seal.band_crcs == crcs).all()
    view, seal2 = container.split_seal(sealed, view=True)
    assert isinstance(view, memoryview) and bytes(view) == body and seal2 == seal
    assert seal != container.Seal(3, zlib.crc32(frame), 0x1122334455667788)
    # version 1: today's bytes and objects
    v1 = container.make_seal(body, 3, 0xCAFEF00D, 7)
    head = b'L3CS' + struct.pack('<BBHIQ', 1, 0, 3, 0xCAFEF00D, 7)
    assert v1 == head + struct.pack('<I', zlib.crc32(body[6:14] + head)) and len(v1) == 24
    got, seal = container.split_seal(body + v1)
    assert got == body and seal == container.Seal(3, 0xCAFEF00D, 7) and seal.band_crcs is None and seal.band_len is None
    with pytest.raises(ValueError, match='banded'):
        container.make_seal(body[6:], 3, 1, 0, crcs, 64)                                   # a band seal on a legacy body


PAIRS = [(4096, 64), (12288, 2496), (28160, 1792), (28160, 28160), (3 * 4096 + 64, 4096), (2 * 4160 + 4096, 4160),
         (2 * 131072 + 192, 131072), (131072 + 128, 131072 + 64), (68, 4), (72, 68)]


def test_the_frame_crc_is_the_combination_of_the_band_crcs():
    for k, (HW, L) in enumerate(PAIRS):
        frame = _frame(HW, k)
        assert container.combine_band_crcs(_band_crcs(frame, HW, L), L, HW) == zlib.crc32(frame), (HW, L)
    with pytest.raises(ValueError):
        container.combine_band_crcs(np.zeros((3, 5), dtype=np.uint32), 64, 256)


def _resealed(body, table, generation, frame_crc, model_id, version=2):
    head = b'L3CS' + struct.pack('<BBHIQ', version, 0, generation, frame_crc, model_id)
    return body + table + head + struct.pack('<I', zlib.crc32(body[6:14] + table + head))


def test_every_reader_error_python_and_c_alike():
    body, frame, crcs, sealed = _sealed()
    fc, T = zlib.crc32(frame), 20 + 12 * 4
    table = sealed[len(body):len(body) + T]

    def with_T(t):                        # the length field alone changed, the check word right for the table the reader will take
        tab = table[:-8] + struct.pack('<I', t) + SEP
        end = len(body) + T
        taken = (body + tab)[max(0, end - t):end] if t <= end else b''
        head = b'L3CS' + struct.pack('<BBHIQ', 2, 0, 3, fc, 9)
        return body + tab + head + struct.pack('<I', zlib.crc32(body[6:14] + taken + head))
    legacy = struct.pack('<4H', *PAD) + struct.pack('<BHH', 1, 8, 8) + struct.pack('<I', 3) + b'abc' + SEP
    other_L = _body(16, 16, 128)
    cases = {
        'T = 0': (with_T(0), 'length field'),
        'T % 12 != 8': (with_T(T + 1), 'length field'),
        'n = 1025': (with_T(20 + 12 * 1025), 'length field'),
        'T beyond the file': (with_T(20 + 12 * 64), 'last scale separator'),
        'T in front of the last separator': (with_T(T + 12), 'last scale separator'),
        'no L3CT': (_resealed(body, b'L3CX' + table[4:], 3, fc, 9), "'L3CT'"),
        'reserved': (_resealed(body, table[:6] + b'\x01\x00' + table[8:], 3, fc, 9), 'reserved'),
        'check word': (sealed[:-1] + bytes([sealed[-1] ^ 1]), 'check word'),
        'check word (table)': (sealed[:len(body) + 14] + bytes([sealed[len(body) + 14] ^ 0x10]) + sealed[len(body) + 15:], 'check word'),
        'check word (padding)': (sealed[:8] + bytes([sealed[8] ^ 2]) + sealed[9:], 'check word'),
        'legacy body': (legacy + table + sealed[-24:], 'legacy'),
        'n field': (_resealed(body, table[:4] + struct.pack('<H', 3) + table[6:], 3, fc, 9), 'band count'),
        'L': (_resealed(body, table[:8] + struct.pack('<I', 128) + table[12:], 3, fc, 9), 'finest scale record'),
        'n of another record': (_resealed(other_L, table, 3, fc, 9), 'finest scale record'),
        'frame CRC': (_resealed(body, table, 3, fc ^ 1, 9), 'combination'),
        'table word': (_resealed(body, table[:12] + bytes([table[12] ^ 1]) + table[13:], 3, fc, 9), 'combination'),
        'flags': (body + table + b'L3CS\x02\x01' + sealed[-18:], 'flags'),
    }
    for what, (f, needle) in cases.items():
        assert container.is_sealed(f), what
        with pytest.raises(ValueError, match='invalid file: seal') as e:
            container.split_seal(f)
        assert not isinstance(e.value, container.SealError)
        got, msg = _find_bands(f)
        assert got[0] == INVALID and msg == str(e.value), (what, msg, str(e.value))
        assert needle in msg, (what, msg)


def test_check_band_crcs_names_bands_and_rows():
    # a 320 x 88 frame at K = 16: L = 1792 (20.4 rows); the image is 317 x 83, centre-padded: top 1, bottom 2
    H, W, L = 320, 88, 1792
    n = container.n_bands(H * W, L)
    assert n == 16
    table = (np.arange(3 * n, dtype=np.int64).reshape(3, n) * 2654435761 % (1 << 32)).astype(np.uint32)
    frame_crc = container.combine_band_crcs(table, L, H * W)
    seals = [None, container.Seal(3, frame_crc, 0, L, table), container.Seal(3, 77, 0), container.Seal(3, frame_crc, 0, L, table)]
    pads = [(2, 3, 1, 2)] * 4
    good = np.broadcast_to(table.astype(np.int64), (4, 3, n)).copy()
    container.check_band_crcs(seals, good, (H, W), pads, 0, [0, frame_crc, 77, frame_crc])
    container.check_band_crcs(seals, good.astype(np.uint32).view(np.int32), (H, W), pads, 0, np.asarray([0, frame_crc, 77, frame_crc]).astype(np.uint32).view(np.int32))
    bad = good.copy()
    bad[1, 1, 3] ^= 1
    bad[1, 2, 4] ^= 1
    bad[3, 0, 15] ^= 5
    with pytest.raises(container.SealError) as e:
        container.check_band_crcs(seals, bad, (H, W), pads, 0, [0, frame_crc, 78, frame_crc])
    err = e.value
    assert (err.reason, err.index, err.failed) == ('pixels', 1, [1, 2, 3]) and isinstance(err, ValueError)
    assert err.bands == {1: [(1, 3), (2, 4)], 3: [(0, 15)]}
    # bands 3..4: pixels [5376, 8960) = frame rows [61, 102) = image rows [60, 101); band 15: rows [305, 320) -> image rows [304, 317)
    assert err.rows == {1: (60, 101), 3: (304, 317)}
    # a region decode's words: bands 9..10 only
    part = good[:, :, 9:11].copy()
    container.check_band_crcs(seals, part, (H, W), pads, 9)
    part[3, 2, 1] ^= 9
    with pytest.raises(container.SealError) as e:
        container.check_band_crcs(seals, part, (H, W), pads, 9)
    assert e.value.bands == {3: [(2, 10)]} and e.value.rows == {3: (202, 223)} and e.value.failed == [3]
    # a damaged band that lies wholly in the padding rows: a 64 x 64 frame at L = 64 is a row per band; top padding 2, bottom 3
    t2 = np.arange(3 * 64, dtype=np.uint32).reshape(3, 64)
    s2 = [container.Seal(3, container.combine_band_crcs(t2, 64, 4096), 0, 64, t2)]
    w2 = t2[None].astype(np.int64).copy()
    w2[0, 0, 1] ^= 1
    w2[0, 1, 62] ^= 1
    with pytest.raises(container.SealError) as e:
        container.check_band_crcs(s2, w2, (64, 64), [(0, 0, 2, 3)])
    assert e.value.bands == {0: [(0, 1), (1, 62)]} and e.value.rows == {0: (0, 59)}          # the hull, clipped to the image
    w2 = t2[None].astype(np.int64).copy()
    w2[0, 2, 63] ^= 1
    with pytest.raises(container.SealError) as e:
        container.check_band_crcs(s2, w2, (64, 64), [(0, 0, 2, 3)])
    assert e.value.bands == {0: [(2, 63)]} and e.value.rows == {0: None}
    # every other SealError carries None
    with pytest.raises(container.SealError) as e:
        container.check_frame_crcs([container.Seal(3, 7, 0)], [8])
    assert e.value.bands is None and e.value.rows is None
    with pytest.raises(container.SealError) as e:
        container.check_seals([container.Seal(2, 7, 0)], 3, 0)
    assert e.value.bands is None and e.value.rows is None


def test_python_and_c_write_the_same_bytes_and_read_them_back():
    lib = _lib.load()
    for H, W, L, seed in ((16, 16, 64, 1), (16, 24, 128, 2), (8, 8, 64, 3), (32, 32, 64, 4)):
        body, frame, crcs, sealed = _sealed(H, W, L, seed)
        n = crcs.shape[1]
        out = ctypes.create_string_buffer(container.seal_bands_bytes(n))
        words = np.ascontiguousarray(crcs)
        assert lib.l3c_seal_write_bands(ctypes.byref(_lib.Seal(3, zlib.crc32(frame), 0x1122334455667788)), body[6:14], words.ctypes.data, n, L, out) == 0
        assert out.raw == sealed[len(body):]
        got, _ = _find_bands(sealed)
        assert got == (1, len(body), (3, zlib.crc32(frame), 0x1122334455667788), n, L, len(body) + 12)
        # a caller that knows version 1 alone: sealed, the body in front of the table
        size, seal = ctypes.c_int64(-7), _lib.Seal()
        assert lib.l3c_seal_find(sealed, len(sealed), ctypes.byref(size), ctypes.byref(seal)) == 1
        assert size.value == len(body) and (seal.generation, seal.frame_crc, seal.model_id) == (3, zlib.crc32(frame), 0x1122334455667788)
        # version 1 and unsealed files through the new entry
        v1 = body + container.make_seal(body, 3, 5, 6)
        assert _find_bands(v1)[0] == (1, len(body), (3, 5, 6), 0, 0, None)
        assert _find_bands(body)[0][:2] == (0, len(body)) and _find_bands(body)[0][3] == 0
    assert lib.l3c_seal_write_bands(None, b'x' * 8, b'x' * 12, 1, 64, ctypes.create_string_buffer(64)) == INVALID
    assert lib.l3c_seal_write_bands(ctypes.byref(_lib.Seal(3, 1, 1)), b'x' * 8, b'x' * 12, 0, 64, ctypes.create_string_buffer(64)) == INVALID
    assert lib.l3c_seal_write_bands(ctypes.byref(_lib.Seal(3, 1, 1)), b'x' * 8, b'x' * 12, 1025, 64, ctypes.create_string_buffer(64)) == INVALID


def test_kernel_entries_check_their_arguments_before_any_launch():
    lib = _lib.load()
    fake, ws = 0x1000, 1 << 30

    def said():
        return lib.l3c_last_error().decode()
    assert lib.l3c_u8_crc32_bands_workspace_bytes(1, 3, 4096, 64) > 0
    for args in ((0, 3, 4096, 64), (1, 0, 4096, 64), (1, 1025, 4096, 64), (1, 3, 0, 64), (1, 3, 4098, 64), (1, 3, 4096, 0), (1, 3, 4096, 66),
                 (1, 3, -4, 64), (1 << 40, 3, 4096, 4)):
        assert lib.l3c_u8_crc32_bands_workspace_bytes(*args) == INVALID, args
        assert lib.l3c_u8_crc32_bands(fake, args[0], args[1], args[2], args[3], 3 * 4096, fake, fake, fake, ws, None) == INVALID, args
    call = lib.l3c_u8_crc32_bands
    assert call(None, 1, 3, 4096, 64, 12288, fake, fake, fake, ws, None) == INVALID and 'null' in said()
    assert call(fake, 1, 3, 4096, 64, 12288, None, fake, fake, ws, None) == INVALID and 'null' in said()
    assert call(fake, 1, 3, 4096, 64, 12288, fake, fake, None, ws, None) == INVALID and 'null' in said()
    assert call(fake, 1, 3, 4096, 64, 12284, fake, fake, fake, ws, None) == INVALID and 'frame_stride' in said()
    assert call(fake, 2, 3, 4096, 64, 12290, fake, fake, fake, ws, None) == INVALID and 'frame_stride' in said()
    assert call(fake + 2, 1, 3, 4096, 64, 12288, fake, fake, fake, ws, None) == INVALID and '4-byte aligned' in said()
    assert call(fake, 1, 3, 4096, 64, 12288, fake + 1, fake, fake, ws, None) == INVALID and '4-byte aligned' in said()
    assert call(fake, 1, 3, 4096, 64, 12288, fake, fake + 2, fake, ws, None) == INVALID and '4-byte aligned' in said()
    assert call(fake, 1, 3, 4096, 64, 12288, fake, fake, fake + 8, ws, None) == INVALID and '16-byte aligned' in said()
    assert call(fake, 1, 3, 4096, 64, 12288, fake, fake, fake, 16, None) == INVALID and 'workspace_bytes too small' in said()
    app = lib.l3c_seal_append_bands
    assert app(None, 4096, fake, fake, fake, 4, 64, None, 0, 1, None) == INVALID and 'null' in said()
    assert app(fake, 4096, None, fake, fake, 4, 64, None, 0, 1, None) == INVALID and 'null' in said()
    assert app(fake, 4096, fake, None, fake, 4, 64, None, 0, 1, None) == INVALID and 'null' in said()
    assert app(fake, 4096, fake, fake, None, 4, 64, None, 0, 1, None) == INVALID and 'null' in said()
    assert app(fake, 4096, fake, fake, fake, 0, 64, None, 0, 1, None) == INVALID and '1..1024' in said()
    assert app(fake, 4096, fake, fake, fake, 1025, 64, None, 0, 1, None) == INVALID and '1..1024' in said()
    assert app(fake, 4096, fake, fake, fake, 4, 0, None, 0, 1, None) == INVALID and 'band_len' in said()
    assert app(fake, 4096, fake, fake, fake, 4, 64, None, 0, 0, None) == INVALID and 'batch size' in said()
    assert app(fake, 4096, fake, fake, fake, 4, 64, None, 0, 65536, None) == INVALID and 'batch size' in said()
    assert app(fake, 0, fake, fake, fake, 4, 64, None, 0, 1, None) == INVALID and 'file_stride' in said()
    assert app(fake, 4096, fake + 4, fake, fake, 4, 64, None, 0, 1, None) == INVALID and 'aligned' in said()
    assert app(fake, 4096, fake, fake + 2, fake, 4, 64, None, 0, 1, None) == INVALID and 'aligned' in said()
    assert app(fake, 4096, fake, fake, fake + 2, 4, 64, None, 0, 1, None) == INVALID and 'aligned' in said()
    assert app(fake, 4096, fake, fake, fake, 4, 64, fake + 1, 0, 1, None) == INVALID and 'aligned' in said()


def test_constructors_refuse_a_band_seal_without_bands():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    with pytest.raises(ValueError, match="seal='bands' needs banded files"):
        Bitcoding(None, bands=0, seal='bands')
    with pytest.raises(ValueError, match='seal must be'):
        Bitcoding(None, bands=4, seal='rows')


def test_band_seal_reader_survives_truncations_and_byte_changes_under_the_sanitizers(tmp_path):
    """tests/cabi/band_seal_check_main.cpp: csrc/seal.h alone, built with the address and undefined-behaviour sanitizers and run as a child
    process: every truncation and every single-byte change of a small band-sealed file in an exactly sized heap buffer, and crafted T and n
    fields (0, 1025, T beyond the file, T % 12 != 8); each call returns 1, 0 or L3C_ERR_INVALID_ARG."""
    exe = tmp_path / 'band_seal_check'
    subprocess.run(['c++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'band_seal_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith('band_seal_check: 209 truncations, 53295 single-byte changes, 49 crafted fields: '), r.stdout
