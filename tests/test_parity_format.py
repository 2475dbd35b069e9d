"""Parity bands (seal version 3) on the host, no GPU: container.make_seal(parity=) / split_seal / band_parity against bytes built by hand with
struct and zlib, and against the C side (csrc/seal.h behind l3c_seal_write_parity / l3c_seal_find_parity / l3c_seal_find_bands /
l3c_seal_find); the argument checks of l3c_band_parity and l3c_u8_xor_spans, every one made before anything is launched (fake, well-aligned
pointers stand in for device memory)."""
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
MODEL = 0x1122334455667788


def _finest(H, W, L, seed):
    """[3][n] band payloads of 0..9 bytes, empty ones among them."""
    rng = np.random.RandomState(seed)
    n = container.n_bands(H * W, L)
    return [[rng.randint(0, 256, (3 * c + 5 * j + seed) % 10).astype(np.uint8).tobytes() for j in range(n)] for c in range(3)]


def _body(H=16, W=24, L=64, seed=0):
    """A banded file of two records: (1, H/2, W/2) in one band and the finest (3, H, W) in bands of L."""
    coarse_L = 64 * (-(-(H // 2) * (W // 2) // 64))
    return container.write_file(PAD, [(1, H // 2, W // 2, coarse_L), (3, H, W, L)], [[[b'abc']], _finest(H, W, L, seed)], True)


def _band_crcs(HW, L, seed):
    frame = np.random.RandomState(seed).randint(0, 256, 3 * HW).astype(np.uint8).tobytes()
    n = container.n_bands(HW, L)
    return zlib.crc32(frame), np.asarray([[zlib.crc32(frame[c * HW + j * L:c * HW + min((j + 1) * L, HW)]) for j in range(n)] for c in range(3)],
                                         dtype=np.uint32)


def _xor_by_hand(payloads, G):
    """The parity of one channel, byte by byte in plain Python: group g = the bands j with j % m == g."""
    n = len(payloads)
    m = -(-n // G)
    res = []
    for g in range(m):
        members = [payloads[j] for j in range(n) if j % m == g]
        out = bytearray(max(len(p) for p in members))
        for p in members:
            for i, v in enumerate(p):
                out[i] ^= v
        res.append(bytes(out))
    return res


def _by_hand(body, generation, frame_crc, model_id, crcs, L, G, rows):
    n, m = crcs.shape[1], len(rows[0])
    head = b'L3CP' + struct.pack('<HH', G, m) + b''.join(struct.pack('<I', len(p)) for row in rows for p in row)
    S = 16 + 12 * m + sum(len(p) for row in rows for p in row)
    tail = struct.pack('<I', S) + SEP
    section = head + b''.join(p for row in rows for p in row) + tail
    assert len(section) == S
    T = 20 + 12 * n
    table = b'L3CT' + struct.pack('<HHI', n, 0, L) + b''.join(struct.pack('<I', int(w)) for w in crcs.reshape(-1)) + struct.pack('<I', T) + SEP
    seal = b'L3CS' + struct.pack('<BBHIQ', 3, 0, generation, frame_crc, model_id)
    return section + table + seal + struct.pack('<I', zlib.crc32(body[6:14] + head + tail + table + seal))


def _sealed(H=16, W=24, L=64, G=4, seed=0):
    body = _body(H, W, L, seed)
    fc, crcs = _band_crcs(H * W, L, seed)
    rows = [_xor_by_hand(ch, G) for ch in _finest(H, W, L, seed)]
    return body, fc, crcs, rows, body + container.make_seal(body, 3, fc, MODEL, crcs, L, parity=(G, rows))


def _find_parity(data):
    """l3c_seal_find_parity -> (status, body bytes, (generation, frame_crc, model_id), n, L, G, m, payload bytes, offset of the payloads)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    body, seal, bands, par = ctypes.c_int64(-7), _lib.Seal(), _lib.SealBands(), _lib.SealParity()
    rc = lib.l3c_seal_find_parity(buf, len(data), ctypes.byref(body), ctypes.byref(seal), ctypes.byref(bands), ctypes.byref(par))
    at = par.payloads - ctypes.addressof(buf) if par.payloads else None
    return (rc, body.value, (seal.generation, seal.frame_crc, seal.model_id), bands.n, bands.band_len, par.G, par.m, par.payload_bytes, at), \
        lib.l3c_last_error().decode()


def test_band_parity_is_the_interleaved_xor():
    rng = np.random.RandomState(5)
    for n, G in ((1, 1), (6, 1), (6, 6), (16, 3), (16, 4), (16, 16), (7, 2), (5, 4)):
        payloads = [rng.randint(0, 256, int(k)).astype(np.uint8).tobytes() for k in rng.randint(0, 40, n)]
        payloads[n // 2] = b''                                                   # a member of length 0
        got = container.band_parity(payloads, G)
        m = -(-n // G)
        assert len(got) == m == container.parity_groups(n, G) == _lib.load().l3c_band_parity_groups(n, G)
        assert got == _xor_by_hand(payloads, G), (n, G)
        for g in range(m):
            assert len(got[g]) == max(len(p) for p in payloads[g::m])
    assert container.band_parity([b'ab', b'\x01'], 1) == [b'ab', b'\x01']     # G = 1: every band is its own parity
    assert container.band_parity([b'ab', b'\x01', b''], 3) == [bytes([ord('a') ^ 1, ord('b')])]
    assert container.band_parity([b'', b''], 2) == [b'']
    # n = 16, G = 3: m = 6 groups of 3, 3, 3, 3, 2, 2 bands
    assert [len(range(g, 16, 6)) for g in range(6)] == [3, 3, 3, 3, 2, 2] and container.parity_groups(16, 3) == 6
    for n, G in ((4, 0), (4, 5), (4, -1)):
        with pytest.raises(ValueError, match='group size'):
            container.band_parity([b'x'] * n, G)
        assert _lib.load().l3c_band_parity_groups(n, G) == INVALID


def test_the_layout_is_the_documented_one():
    lib = _lib.load()
    for H, W, L, G in ((16, 24, 64, 4), (16, 16, 64, 1), (16, 16, 64, 4), (8, 8, 64, 1), (16, 24, 128, 2)):
        body, fc, crcs, rows, sealed = _sealed(H, W, L, G, H + W + G)
        n = container.n_bands(H * W, L)
        m = -(-n // G)
        s = sealed[len(body):]
        assert s == _by_hand(body, 3, fc, MODEL, crcs, L, G, rows)
        total = sum(len(p) for row in rows for p in row)
        assert len(s) == 16 + 12 * m + total + 20 + 12 * n + 24 == lib.l3c_seal_parity_bytes(n, m, total)
        assert container.parity_section_bytes([[len(p) for p in row] for row in rows]) == 16 + 12 * m + total
        assert container.is_sealed(sealed) and sealed[-24:-20] == b'L3CS' and sealed[-28:-24] == SEP and sealed[-20] == 3
        assert sealed[len(body):len(body) + 4] == b'L3CP' and sealed[len(body) - 4:len(body)] == SEP
        # the version-2 file of the same encode with the section inserted: table and seal differ in the version byte and the check word
        v2 = body + container.make_seal(body, 3, fc, MODEL, crcs, L)
        S = 16 + 12 * m + total
        assert sealed[:len(body)] == v2[:len(body)] and sealed[len(body) + S:-20] == v2[len(body):-20] and sealed[-19:-4] == v2[-19:-4]
        assert container.split_seal(v2)[0] == container.split_seal(sealed)[0] == body
    for args in ((0, 1, 0), (1025, 1, 0), (4, 0, 0), (4, 5, 0), (4, 2, -1), (4, 2, 1 << 32)):
        assert lib.l3c_seal_parity_bytes(*args) == INVALID, args


def test_split_seal_round_trips_and_versions_1_and_2_are_unchanged():
    body, fc, crcs, rows, sealed = _sealed()
    got, seal = container.split_seal(sealed)
    assert got == body and seal == container.Seal(3, fc, MODEL, 64, crcs, 4, rows)
    assert seal.parity_group == 4 and seal.parity_groups == 2 and [[bytes(p) for p in row] for row in seal.parity] == rows
    assert seal.band_len == 64 and (seal.band_crcs == crcs).all()
    view, seal_v = container.split_seal(sealed, view=True)
    assert isinstance(view, memoryview) and bytes(view) == body and seal_v == seal
    assert isinstance(seal.parity[0][0], memoryview)                                    # views of the file, not copies
    # a seal with parity is not the band seal of the same table, and differs by a payload byte
    v2_seal = container.Seal(3, fc, MODEL, 64, crcs)
    assert seal != v2_seal and v2_seal != seal
    other = [list(r) for r in rows]
    other[1][0] = bytes([other[1][0][0] ^ 1]) + other[1][0][1:]
    assert seal != container.Seal(3, fc, MODEL, 64, crcs, 4, other)
    # versions 1 and 2: today's bytes and objects
    v1 = container.make_seal(body, 3, 0xCAFEF00D, 7)
    head = b'L3CS' + struct.pack('<BBHIQ', 1, 0, 3, 0xCAFEF00D, 7)
    assert v1 == head + struct.pack('<I', zlib.crc32(body[6:14] + head))
    got, s1 = container.split_seal(body + v1)
    assert got == body and s1 == container.Seal(3, 0xCAFEF00D, 7) and s1.parity is None and s1.parity_group is None and s1.parity_groups == 0
    v2 = container.make_seal(body, 3, fc, MODEL, crcs, 64)
    T = 20 + 12 * 6
    table = b'L3CT' + struct.pack('<HHI', 6, 0, 64) + crcs.astype('<u4').tobytes() + struct.pack('<I', T) + SEP
    head = b'L3CS' + struct.pack('<BBHIQ', 2, 0, 3, fc, MODEL)
    assert v2 == table + head + struct.pack('<I', zlib.crc32(body[6:14] + table + head))
    got, s2 = container.split_seal(body + v2)
    assert got == body and s2 == v2_seal and s2.parity is None and hash is not None
    assert repr(s2) == 'Seal(generation=3, frame_crc=0x{:08x}, model_id=0x1122334455667788, band_len=64, band_crcs=<3 x 6>)'.format(fc)
    with pytest.raises(ValueError, match='band seal'):
        container.make_seal(body, 3, fc, MODEL, parity=(4, rows))
    with pytest.raises(ValueError, match='3 x 2 payloads'):
        container.make_seal(body, 3, fc, MODEL, crcs, 64, parity=(4, [r[:1] for r in rows]))
    with pytest.raises(ValueError, match='group size'):
        container.make_seal(body, 3, fc, MODEL, crcs, 64, parity=(7, rows))


def test_a_damaged_parity_payload_leaves_the_file_readable():
    body, fc, crcs, rows, sealed = _sealed()
    at = len(body) + 8 + 12 * 2
    total = sum(len(p) for row in rows for p in row)
    for k in (0, total // 2, total - 1):
        bad = bytearray(sealed)
        bad[at + k] ^= 0x5A
        got, seal = container.split_seal(bytes(bad))
        assert got == body and seal.band_len == 64 and (seal.band_crcs == crcs).all()
        assert b''.join(bytes(p) for row in seal.parity for p in row) == bytes(bad[at:at + total])
        assert _find_parity(bytes(bad))[0][:2] == (1, len(body))


def _resealed(body, section, table, fc, version=3):
    """The check word made right for a (changed) section and table."""
    m, = struct.unpack('<H', section[6:8])
    head = section[:8 + 12 * m] if 8 + 12 * m <= len(section) - 8 else b''
    seal = b'L3CS' + struct.pack('<BBHIQ', version, 0, 3, fc, 9)
    return body + section + table + seal + struct.pack('<I', zlib.crc32(body[6:14] + head + section[-8:] + table + seal))


def test_every_reader_error_python_and_c_alike():
    body, fc, crcs, rows, sealed = _sealed()          # n = 6, G = 4, m = 2
    n, m, T = 6, 2, 20 + 12 * 6
    total = sum(len(p) for row in rows for p in row)
    S = 16 + 12 * m + total
    section, table = sealed[len(body):len(body) + S], sealed[len(body) + S:len(body) + S + T]
    plen = [len(p) for row in rows for p in row]

    def with_fields(G=4, mm=m, lens=plen, Sfield=S, sig=b'L3CP'):
        payload = section[8 + 12 * m:-8]
        s = sig + struct.pack('<HH', G, mm) + b''.join(struct.pack('<I', v) for v in lens) + payload + struct.pack('<I', Sfield) + SEP
        return _resealed(body, s, table, fc)
    swapped = list(plen)
    swapped[0], swapped[1] = plen[0] + 1, plen[1] - 1
    legacy = struct.pack('<4H', *PAD) + struct.pack('<BHH', 1, 8, 8) + struct.pack('<I', 3) + b'abc' + SEP
    other = _body(16, 24, 64, seed=1)                 # the same shape, other payload lengths
    cases = {
        'S = 0': (with_fields(Sfield=0), 'last scale separator'),
        'S too small': (with_fields(Sfield=27), 'last scale separator'),
        'S beyond the file': (with_fields(Sfield=len(body) + S), 'last scale separator'),
        'S not at a separator': (with_fields(Sfield=S + 4), 'last scale separator'),
        'no L3CP': (with_fields(sig=b'L3CX'), "'L3CP'"),
        'm = 0': (with_fields(mm=0), 'too short for its 0 x 3 length fields'),
        'm too large for S': (with_fields(mm=1000), 'too short for its 1000 x 3 length fields'),
        'S is not the sum': (with_fields(lens=[plen[0] + 1] + plen[1:]), '16 + 12 m + the sum'),
        'm = 3 (the sum cannot fit)': (with_fields(mm=3), '16 + 12 m + the sum'),
        'G = 2 (m would be 3)': (with_fields(G=2), 'finest scale record'),
        'G = 0': (with_fields(G=0), 'finest scale record'),
        'G = 7 > n': (with_fields(G=7), 'finest scale record'),
        'plen is not the longest member': (with_fields(lens=swapped), "longest member's"),
        'plen of another body': (_resealed(other, section, table, fc), "longest member's"),
        'legacy body': (legacy + section + table + sealed[-24:], 'legacy file (version 3, the parity seal'),
        'check word': (sealed[:-1] + bytes([sealed[-1] ^ 1]), 'check word'),
        'check word (G)': (sealed[:len(body) + 4] + bytes([sealed[len(body) + 4] ^ 1]) + sealed[len(body) + 5:], 'check word'),
        'a changed plen byte (the length check comes first)': (sealed[:len(body) + 9] + bytes([sealed[len(body) + 9] ^ 1]) + sealed[len(body) + 10:],
                                                                '16 + 12 m + the sum'),
        'check word (two plen moved, S kept)': (body + section[:8] + struct.pack('<2I', plen[0] + 1, plen[1] - 1) + section[16:] + sealed[len(body) + S:],
                                                'check word'),
        'check word (padding)': (sealed[:8] + bytes([sealed[8] ^ 2]) + sealed[9:], 'check word'),
        'check word (table)': (sealed[:len(body) + S + 14] + bytes([sealed[len(body) + S + 14] ^ 0x10]) + sealed[len(body) + S + 15:], 'check word'),
        'flags': (sealed[:-19] + b'\x01' + sealed[-18:], 'flags'),
        # what a version-2 seal is rejected for still applies
        'T = 0': (sealed[:-32] + struct.pack('<I', 0) + sealed[-28:], 'length field'),
        'no L3CT': (_resealed(body, section, b'L3CX' + table[4:], fc), "'L3CT'"),
        'reserved': (_resealed(body, section, table[:6] + b'\x01\x00' + table[8:], fc), 'reserved'),
        'n field': (_resealed(body, section, table[:4] + struct.pack('<H', 3) + table[6:], fc), 'band count'),
        'L': (_resealed(body, section, table[:8] + struct.pack('<I', 128) + table[12:], fc), 'finest scale record'),
        'frame CRC': (_resealed(body, section, table, fc ^ 1), 'combination'),
        'a version the reader does not know': (sealed[:-20] + b'\x04' + sealed[-19:], 'unknown version'),
    }
    lib = _lib.load()
    for what, (f, needle) in cases.items():
        assert container.is_sealed(f), what
        with pytest.raises(ValueError, match='invalid file: seal') as e:
            container.split_seal(f)
        assert not isinstance(e.value, container.SealError)
        got, msg = _find_parity(f)
        assert got[0] == INVALID and msg == str(e.value), (what, msg, str(e.value))
        assert needle in msg, (what, msg)
        # the entries of versions 1 and 2 say the same
        size = ctypes.c_int64()
        assert lib.l3c_seal_find(f, len(f), ctypes.byref(size), None) == INVALID and lib.l3c_last_error().decode() == msg, what
        assert lib.l3c_seal_find_bands(f, len(f), ctypes.byref(size), None, None) == INVALID and lib.l3c_last_error().decode() == msg, what
    # a version-2 seal on a legacy file: the message of before
    v2 = body + container.make_seal(body, 3, fc, MODEL, crcs, 64)
    with pytest.raises(ValueError, match=r'legacy file \(version 2, the band seal, needs a banded file\)'):
        container.split_seal(legacy + v2[len(body):])


def test_python_and_c_write_the_same_bytes_and_read_them_back():
    lib = _lib.load()
    for H, W, L, G, seed in ((16, 24, 64, 4, 1), (16, 24, 64, 6, 2), (16, 16, 64, 1, 3), (8, 8, 64, 1, 4), (32, 32, 64, 5, 5)):
        body, fc, crcs, rows, sealed = _sealed(H, W, L, G, seed)
        n = crcs.shape[1]
        m = -(-n // G)
        payload = b''.join(p for row in rows for p in row)
        plen = np.asarray([len(p) for row in rows for p in row], dtype=np.uint32)
        out = ctypes.create_string_buffer(lib.l3c_seal_parity_bytes(n, m, len(payload)))
        words = np.ascontiguousarray(crcs)
        assert lib.l3c_seal_write_parity(ctypes.byref(_lib.Seal(3, fc, MODEL)), body[6:14], words.ctypes.data, n, L, G, plen.ctypes.data, payload, out) == 0
        assert out.raw == sealed[len(body):]
        got, _ = _find_parity(sealed)
        assert got == (1, len(body), (3, fc, MODEL), n, L, G, m, len(payload), len(body) + 8 + 12 * m)
        # callers that know versions 1 and 2 alone: sealed, the body in front of the section
        size, seal, bands = ctypes.c_int64(-7), _lib.Seal(), _lib.SealBands()
        assert lib.l3c_seal_find(sealed, len(sealed), ctypes.byref(size), ctypes.byref(seal)) == 1
        assert size.value == len(body) and (seal.generation, seal.frame_crc, seal.model_id) == (3, fc, MODEL)
        size = ctypes.c_int64(-7)
        assert lib.l3c_seal_find_bands(sealed, len(sealed), ctypes.byref(size), ctypes.byref(seal), ctypes.byref(bands)) == 1
        assert size.value == len(body) and bands.n == n and bands.band_len == L
        # versions 1 and 2 and unsealed files through the new entry
        v1 = body + container.make_seal(body, 3, 5, 6)
        assert _find_parity(v1)[0] == (1, len(body), (3, 5, 6), 0, 0, 0, 0, 0, None)
        v2 = body + container.make_seal(body, 3, fc, MODEL, crcs, L)
        assert _find_parity(v2)[0] == (1, len(body), (3, fc, MODEL), n, L, 0, 0, 0, None)
        assert _find_parity(body)[0][:2] == (0, len(body)) and _find_parity(body)[0][6] == 0
    seal = ctypes.byref(_lib.Seal(3, 1, 1))
    plen = np.zeros(3, dtype=np.uint32)
    out = ctypes.create_string_buffer(256)
    assert lib.l3c_seal_write_parity(None, b'x' * 8, b'x' * 12, 1, 64, 1, plen.ctypes.data, None, out) == INVALID
    assert lib.l3c_seal_write_parity(seal, b'x' * 8, b'x' * 12, 0, 64, 1, plen.ctypes.data, None, out) == INVALID
    assert lib.l3c_seal_write_parity(seal, b'x' * 8, b'x' * 12, 1, 64, 2, plen.ctypes.data, None, out) == INVALID
    assert lib.l3c_seal_write_parity(seal, b'x' * 8, b'x' * 12, 1, 64, 0, plen.ctypes.data, None, out) == INVALID
    plen[0] = 1
    assert lib.l3c_seal_write_parity(seal, b'x' * 8, b'x' * 12, 1, 64, 1, plen.ctypes.data, None, out) == INVALID      # payload bytes without payloads
    assert lib.l3c_abi_version() == 4                      # symbols were added, nothing existing changed


FAKE = 0x100000
SPAN = np.dtype([('offset', '<i8'), ('bytes', '<i8')])


def _said():
    return _lib.load().l3c_last_error().decode()


def _table(rows):
    t = np.zeros(len(rows), dtype=SPAN)
    for i, r in enumerate(rows):
        t[i] = r
    return t


def _xor(spans, first, slots, data=FAKE, data_bytes=4096, out=FAKE + (1 << 20), out_bytes=4096, dev=(FAKE + 8, FAKE + 16, FAKE + 24), n_groups=None,
         host=(True, True, True)):
    spans, slots, first = _table(spans), _table(slots), np.asarray(first, dtype=np.int64)
    return _lib.load().l3c_u8_xor_spans(data, data_bytes, spans.ctypes.data if host[0] else None, dev[0], len(spans),
                                        first.ctypes.data if host[1] else None, dev[1], len(slots) if n_groups is None else n_groups,
                                        slots.ctypes.data if host[2] else None, dev[2], out, out_bytes, None)


def test_xor_spans_argument_checks_precede_any_device_call():
    from l3c_pytorch_amd import ops
    assert ops.SPAN_DTYPE == SPAN
    spans, first, slots = [(0, 5), (64, 17), (128, 0)], [0, 2, 3], [(0, 17), (64, 3)]
    # nothing to do is success, whatever the pointers
    assert _xor(spans, first, slots, n_groups=0, data=None, out=None, dev=(None, None, None), host=(False, False, False)) == 0
    assert _xor(spans, first, slots, n_groups=-1) == INVALID and 'n_groups' in _said()
    assert _xor(spans, first, slots, n_groups=65536) == INVALID and 'n_groups' in _said()
    for host in ((False, True, True), (True, False, True), (True, True, False)):
        assert _xor(spans, first, slots, host=host) == INVALID and 'null pointer' in _said(), host
    for kw in (dict(data=None), dict(out=None), dict(dev=(None, FAKE, FAKE)), dict(dev=(FAKE, None, FAKE)), dict(dev=(FAKE, FAKE, None))):
        assert _xor(spans, first, slots, **kw) == INVALID and 'null pointer' in _said(), kw
    assert _xor(spans, first, slots, data=FAKE + 2) == INVALID and '4-byte aligned' in _said()
    assert _xor(spans, first, slots, out=FAKE + (1 << 20) + 1) == INVALID and '4-byte aligned' in _said()
    for dev in ((FAKE + 4, FAKE, FAKE), (FAKE, FAKE + 4, FAKE), (FAKE, FAKE, FAKE + 4)):
        assert _xor(spans, first, slots, dev=dev) == INVALID and '8-byte aligned' in _said(), dev
    assert _xor(spans, first, slots, out=FAKE + 2048) == INVALID and 'overlap' in _said()
    assert _xor(spans, first, slots, data_bytes=-1) == INVALID
    # every field of a span, a group and an output slot; the error names the table and the entry
    bad_spans = [((-4, 5), 'negative'), ((0, -1), 'negative'), ((2, 5), 'multiple of 4'), ((4092, 5), 'exceeds data_bytes'),
                 ((4096, 1), 'exceeds data_bytes'), ((4, 2 ** 63 - 5), 'overflows'), ((2 ** 62, 2 ** 61), 'exceeds data_bytes')]
    for row, needle in bad_spans:
        for at in (0, 2):
            rows = list(spans)
            rows[at] = row
            assert _xor(rows, first, slots) == INVALID and needle in _said() and 'span {}'.format(at) in _said(), (row, _said())
    for f, needle in (([1, 2, 3], 'start at 0'), ([0, 3, 2], 'descend'), ([0, 2, 4], 'exceeds n_spans'), ([0, 1, 2], 'end at n_spans')):
        assert _xor(spans, f, slots) == INVALID and needle in _said() and 'group' in _said(), (f, _said())
    bad_slots = [((-4, 5), 'negative'), ((0, -1), 'negative'), ((6, 5), 'multiple of 4'), ((4088, 5), 'exceeds out_bytes'),
                 ((4096, 0), 'exceeds out_bytes'), ((0, 4093), 'exceeds out_bytes'), ((4, 2 ** 63 - 2), 'overflows')]
    for row, needle in bad_slots:
        for at in (0, 1):
            rows = list(slots)
            rows[at] = row
            assert _xor(spans, first, rows) == INVALID and needle in _said() and 'out span {}'.format(at) in _said(), (row, _said())


def _scale(H=16, W=24, L=64, C=3, full=FAKE, nb_full=FAKE + 4096, s_full=136, last=FAKE + 8192, nb_last=FAKE + 12288, s_last=136):
    return _lib.BandedScale(full, nb_full, s_full, last, nb_last, s_last, C, H, W, L)


def _parity(scale, B=2, G=4, parity=FAKE + (1 << 20), stride=144, nbytes=FAKE + (2 << 20), null_scale=False):
    return _lib.load().l3c_band_parity(None if null_scale else ctypes.byref(scale), B, G, parity, stride, nbytes, None)


def test_band_parity_argument_checks_precede_any_device_call():
    for kw in (dict(null_scale=True), dict(parity=None), dict(nbytes=None)):
        assert _parity(_scale(), **kw) == INVALID and 'null pointer' in _said(), kw
    for kw in (dict(full=None), dict(nb_full=None), dict(last=None), dict(nb_last=None)):
        assert _parity(_scale(**kw)) == INVALID and 'null pointer' in _said(), kw
    assert _parity(_scale(C=1)) == INVALID and 'C must be 3' in _said()
    assert _parity(_scale(H=0)) == INVALID and 'C must be 3' in _said()
    for L in (0, 32, 100, -64):
        assert _parity(_scale(L=L)) == INVALID and 'band_len' in _said(), L
    assert _parity(_scale(H=1024, W=1024, L=64)) == INVALID and '1024 bands' in _said()
    for G in (0, -1, 7):                                                       # n = 6
        assert _parity(_scale(), G=G) == INVALID and 'G must be in 1..n' in _said(), G
    for B in (0, -1, 65535 // 6 + 1):                                          # G = 4: m = 2, 3 m = 6 streams per image
        assert _parity(_scale(), B=B) == INVALID and 'batch size' in _said(), B
    for kw in (dict(s_full=0), dict(s_full=138), dict(s_last=0), dict(s_last=134)):
        assert _parity(_scale(**kw)) == INVALID and 'coder strides' in _said(), kw
    for stride in (0, 128, 140, 152):                                          # too short, or no multiple of 16
        assert _parity(_scale(), stride=stride) == INVALID and 'parity_stride' in _said(), stride
    for kw in (dict(full=FAKE + 2), dict(last=FAKE + 8192 + 1), dict(nb_full=FAKE + 4098), dict(nb_last=FAKE + 12290)):
        assert _parity(_scale(**kw)) == INVALID and '4-byte aligned' in _said(), kw
    assert _parity(_scale(), nbytes=FAKE + 2) == INVALID and '4-byte aligned' in _said()
    assert _parity(_scale(), parity=FAKE + 8) == INVALID and '16-byte aligned' in _said()
    # n == 1: the full-band group is absent and not asked for
    assert _parity(_scale(H=8, W=8, full=None, nb_full=None, s_full=0), G=2) == INVALID and 'G must be in 1..n' in _said()


def test_constructor_refuses_parity_without_a_band_seal():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    for kw in (dict(bands=4, seal=True), dict(bands=4, seal=False), dict(bands=0, seal=False)):
        with pytest.raises(ValueError, match="parity needs seal='bands'"):
            Bitcoding(None, parity=4, **kw)
    for G in (-1, 1.5, 'x'):
        with pytest.raises(ValueError, match='parity must be'):
            Bitcoding(None, bands=4, seal='bands', parity=G)
    assert Bitcoding(None, bands=4, seal='bands').parity == 0 and Bitcoding(None, bands=4, seal='bands', parity=16).parity == 16


def test_repair_info_line():
    info = container.RepairInfo({0: [(0, 3)]}, {0: (61, 82)}, container.SalvageInfo({}, {}, [], [], {0: 48}, 1), [b'x'], 1)
    assert info.line() == 'repaired: rows [61, 82) restored (1 payload), every row verified'
    none = container.RepairInfo({}, {}, container.SalvageInfo({}, {}, [], [], {0: 48}, 1), [None], 0)
    assert none.line() == 'seal: ok' and none.rounds == 0
    both = container.RepairInfo({1: [(0, 3), (1, 9)]}, {1: (61, 200)}, container.SalvageInfo({0: [(0, 3), (0, 7)]}, {0: (61, 163)}, [], [], {0: 48, 1: 48}, 2),
                                [None, b'y'], 1)
    assert both.line() == ('repaired: file 1: rows [61, 200) restored (2 payloads); salvaged: file 0: rows [61, 163) concealed (2 of 48 bands), '
                           'every other row verified')


def test_parity_seal_reader_survives_truncations_and_byte_changes_under_the_sanitizers(tmp_path):
    """tests/cabi/parity_seal_check_main.cpp: csrc/seal.h alone, built with the address and undefined-behaviour sanitizers and run as a child
    process: every truncation and single-byte changes at every position of a small version-3 file in an exactly sized heap buffer, and crafted
    S, G, m and plen fields; each call returns 1, 0 or L3C_ERR_INVALID_ARG, and a changed parity payload byte never makes the file unreadable."""
    exe = tmp_path / 'parity_seal_check'
    subprocess.run(['c++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'parity_seal_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith('parity_seal_check: 356 truncations, 13172 single-byte changes (1110 in parity payloads, all readable), '
                                       '45 crafted fields: '), r.stdout
