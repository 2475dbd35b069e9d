"""R parity streams per group (the 'L3CQ' section of seal version 3) on the host, no GPU: the GF(2^8) arithmetic (container.gf_mul, rs_parity,
rs_repair_coefficients) against a bit-by-bit multiply and the known answer, container.make_seal / split_seal against bytes built by hand with
struct and zlib and against the C side (csrc/seal.h behind l3c_seal_write_parity_rs / l3c_seal_find_parity_rs and the three older entries),
and the argument checks of l3c_band_parity_rs and l3c_u8_gf_spans, every one made before anything is launched (fake, well-aligned pointers
stand in for device memory)."""
import ctypes
import itertools
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
LENS = [0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 4097, 64]


def _mul_bitwise(a, b):
    """a b mod 0x11D, bit by bit: independent of the tables in container."""
    p = 0
    for i in range(8):
        if (b >> i) & 1:
            p ^= a << i
    for i in range(14, 7, -1):
        if (p >> i) & 1:
            p ^= 0x11D << (i - 8)
    return p


def _pow(a, e):
    r = 1
    for _ in range(e):
        r = _mul_bitwise(r, a)
    return r


def _rs_by_hand(payloads, G, R):
    """[m][R] rows of one channel, byte by byte in plain Python: member k of group g is band g + k m, its point 2^k."""
    n = len(payloads)
    m = -(-n // G)
    res = []
    for g in range(m):
        members = [payloads[j] for j in range(g, n, m)]
        rows = [bytearray(max(len(p) for p in members)) for _ in range(R)]
        for k, p in enumerate(members):
            for r in range(R):
                w = _pow(_pow(2, k), r)
                for i, v in enumerate(p):
                    rows[r][i] ^= _mul_bitwise(w, v)
        res.append([bytes(row) for row in rows])
    return res


def test_gf_mul_and_the_known_answer():
    for a in range(256):
        assert container.gf_mul(a, 1) == a and container.gf_mul(a, 0) == 0 and container.gf_mul(0, a) == 0
        assert container.gf_mul(a, 2) == ((a << 1) ^ (0x11D if a & 0x80 else 0))
    rng = np.random.RandomState(0)
    for a, b in rng.randint(0, 256, (2000, 2)).tolist():
        assert container.gf_mul(a, b) == _mul_bitwise(a, b) == container.gf_mul(b, a), (a, b)
    arr = np.arange(256, dtype=np.uint8)
    for c in (0, 1, 2, 0x80, 0xFF, 0x1D):
        assert container.gf_mul(arr, np.uint8(c)).tolist() == [_mul_bitwise(a, c) for a in range(256)]
    # alpha = 2 generates all 255 non-zero elements: the points of up to 255 members are distinct
    assert len({container.gf_pow_alpha(k) for k in range(255)}) == 255 and container.gf_pow_alpha(255) == 1
    # one-byte members 0x01, 0x02, 0x80 at k = 0, 1, 2
    assert container.rs_parity([b'\x01', b'\x02', b'\x80'], 3, 4) == [[b'\x83', b'\x3F', b'\xE1', b'\x96']]
    assert _rs_by_hand([b'\x01', b'\x02', b'\x80'], 3, 4) == [[b'\x83', b'\x3F', b'\xE1', b'\x96']]


def test_rs_parity_row_0_is_band_parity_and_every_row_is_the_documented_sum():
    rng = np.random.RandomState(5)
    for n, G in ((1, 1), (6, 1), (6, 6), (16, 3), (16, 4), (16, 16), (7, 2), (5, 4)):
        payloads = [rng.randint(0, 256, int(k)).astype(np.uint8).tobytes() for k in rng.randint(0, 40, n)]
        payloads[n // 2] = b''
        assert [rows[0] for rows in container.rs_parity(payloads, G, 1)] == container.band_parity(payloads, G)
        assert all(len(rows) == 1 for rows in container.rs_parity(payloads, G, 1))
        for R in (2, 3, 4):
            got = container.rs_parity(payloads, G, R)
            assert got == _rs_by_hand(payloads, G, R), (n, G, R)
            assert [rows[0] for rows in got] == container.band_parity(payloads, G)
            assert all(len(set(len(p) for p in rows)) == 1 for rows in got)
    for R in (0, 5, -1, True, 1.5):
        with pytest.raises(ValueError, match='parity_streams'):
            container.rs_parity([b'x'] * 4, 2, R)
    with pytest.raises(ValueError, match='at most 255'):
        container.rs_parity([b'x'] * 256, 256, 2)
    assert len(container.rs_parity([b'x'] * 256, 256, 1)) == 1            # one stream: no points, no limit
    assert len(container.rs_parity([b'x'] * 300, 255, 2)) == 2
    with pytest.raises(ValueError, match='group size'):
        container.rs_parity([b'x'] * 4, 5, 2)


def test_no_window_of_consecutive_rows_is_singular_and_rows_0_and_3_can_be():
    # t = 1: x^r0 != 0.  t = 2..4 on a sample of member sets that includes the extremes
    rng = np.random.RandomState(1)
    for t in (2, 3, 4):
        sets = [tuple(range(t)), tuple(range(255 - t, 255)), (0, 85, 170, 254)[:t]] + [tuple(sorted(rng.choice(255, t, replace=False))) for _ in range(60)]
        for ks in sets:
            for r0 in range(0, 4 - t + 1):
                container.rs_repair_coefficients(ks, [], r0)
    with pytest.raises(ValueError, match='distinct members'):
        container.rs_repair_coefficients([3, 3], [1])
    with pytest.raises(ValueError, match='distinct members'):
        container.rs_repair_coefficients([3], [3])
    with pytest.raises(ValueError, match='distinct members'):
        container.rs_repair_coefficients([255], [])
    # rows {0, 3} with k = 0 and 85: x^3 = 1 for both, the 2 x 2 matrix is singular -- why only windows are used
    x0, x85 = container.gf_pow_alpha(0), container.gf_pow_alpha(85)
    assert container.gf_mul(container.gf_mul(x85, x85), x85) == 1 == container.gf_mul(container.gf_mul(x0, x0), x0)


_TIMES = np.asarray([[_mul_bitwise(a, c) for a in range(256)] for c in range(256)], dtype=np.uint8)      # _TIMES[c][a] = c a


def _combine(sources, coefs, length):
    out = np.zeros(length, dtype=np.uint8)
    for src, c in zip(sources, coefs):
        a = np.frombuffer(src, dtype=np.uint8)[:length]
        out[:len(a)] ^= _TIMES[c][a]
    return out.tobytes()


@pytest.mark.parametrize('G', [1, 3, 4, 16])
def test_every_subset_of_up_to_R_members_comes_back_from_every_window(G):
    n = 16
    rng = np.random.RandomState(G)
    payloads = [rng.randint(0, 256, LENS[(5 * j + G) % len(LENS)]).astype(np.uint8).tobytes() for j in range(n)]
    m = -(-n // G)
    subsets = 0
    for R in (2, 3, 4):
        parity = container.rs_parity(payloads, G, R)
        for g in range(m):
            members = payloads[g::m]
            for t in range(1, min(R, len(members)) + 1):
                for erased in itertools.combinations(range(len(members)), t):
                    present = [k for k in range(len(members)) if k not in erased]
                    for r0 in range(R - t + 1):
                        solved = container.rs_repair_coefficients(erased, present, r0)
                        assert len(solved) == t
                        for e, (rows, weights) in zip(erased, solved):
                            assert len(rows) == t and len(weights) == len(present)
                            got = _combine(parity[g][r0:r0 + t] + [members[k] for k in present], list(rows) + list(weights), len(members[e]))
                            assert got == members[e], (G, R, g, erased, r0, e)
                        subsets += 1
    assert subsets > 0


def _finest(H, W, L, seed):
    rng = np.random.RandomState(seed)
    n = container.n_bands(H * W, L)
    return [[rng.randint(0, 256, (3 * c + 5 * j + seed) % 10).astype(np.uint8).tobytes() for j in range(n)] for c in range(3)]


def _body(H=16, W=24, L=64, seed=0):
    coarse_L = 64 * (-(-(H // 2) * (W // 2) // 64))
    return container.write_file(PAD, [(1, H // 2, W // 2, coarse_L), (3, H, W, L)], [[[b'abc']], _finest(H, W, L, seed)], True)


def _band_crcs(HW, L, seed):
    frame = np.random.RandomState(seed).randint(0, 256, 3 * HW).astype(np.uint8).tobytes()
    n = container.n_bands(HW, L)
    return zlib.crc32(frame), np.asarray([[zlib.crc32(frame[c * HW + j * L:c * HW + min((j + 1) * L, HW)]) for j in range(n)] for c in range(3)],
                                         dtype=np.uint32)


def _by_hand(body, generation, frame_crc, model_id, crcs, L, G, R, rows):
    n, m = crcs.shape[1], len(rows[0])
    head = b'L3CQ' + struct.pack('<HHHH', G, m, R, 0) + b''.join(struct.pack('<I', len(p[0])) for row in rows for p in row)
    S = 20 + 12 * m + R * sum(len(p[0]) for row in rows for p in row)
    tail = struct.pack('<I', S) + SEP
    section = head + b''.join(q for row in rows for p in row for q in p) + tail
    assert len(section) == S
    T = 20 + 12 * n
    table = b'L3CT' + struct.pack('<HHI', n, 0, L) + b''.join(struct.pack('<I', int(w)) for w in crcs.reshape(-1)) + struct.pack('<I', T) + SEP
    seal = b'L3CS' + struct.pack('<BBHIQ', 3, 0, generation, frame_crc, model_id)
    return section + table + seal + struct.pack('<I', zlib.crc32(body[6:14] + head + tail + table + seal))


def _sealed(H=16, W=24, L=64, G=4, R=2, seed=0):
    body = _body(H, W, L, seed)
    fc, crcs = _band_crcs(H * W, L, seed)
    rows = [_rs_by_hand(ch, G, R) for ch in _finest(H, W, L, seed)]
    return body, fc, crcs, rows, body + container.make_seal(body, 3, fc, MODEL, crcs, L, parity=(G, rows))


def _find_rs(data):
    """l3c_seal_find_parity_rs -> (status, body bytes, (generation, frame_crc, model_id), n, L, G, m, R, payload bytes, offset of the payloads)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    body, seal, bands, par = ctypes.c_int64(-7), _lib.Seal(), _lib.SealBands(), _lib.SealParityRS()
    rc = lib.l3c_seal_find_parity_rs(buf, len(data), ctypes.byref(body), ctypes.byref(seal), ctypes.byref(bands), ctypes.byref(par))
    at = par.payloads - ctypes.addressof(buf) if par.payloads else None
    return (rc, body.value, (seal.generation, seal.frame_crc, seal.model_id), bands.n, bands.band_len, par.G, par.m, par.R, par.payload_bytes, at), \
        lib.l3c_last_error().decode()


def test_the_layout_is_the_documented_one_and_the_round_trip():
    lib = _lib.load()
    for H, W, L, G, R in ((16, 24, 64, 4, 2), (16, 16, 64, 1, 4), (16, 16, 64, 4, 3), (8, 8, 64, 1, 2), (16, 24, 128, 2, 4)):
        body, fc, crcs, rows, sealed = _sealed(H, W, L, G, R, H + W + G)
        n = container.n_bands(H * W, L)
        m = -(-n // G)
        s = sealed[len(body):]
        assert s == _by_hand(body, 3, fc, MODEL, crcs, L, G, R, rows)
        total = R * sum(len(p[0]) for row in rows for p in row)
        assert len(s) == 20 + 12 * m + total + 20 + 12 * n + 24 == lib.l3c_seal_parity_rs_bytes(n, m, R, total)
        assert container.parity_section_bytes([[len(p[0]) for p in row] for row in rows], R) == 20 + 12 * m + total
        assert container.is_sealed(sealed) and sealed[-24:-20] == b'L3CS' and sealed[-28:-24] == SEP and sealed[-20] == 3 and sealed[-19] == 0
        assert sealed[len(body):len(body) + 4] == b'L3CQ' and sealed[len(body) - 4:len(body)] == SEP
        # the version-2 file of the same encode with the section inserted: table and seal differ in the version byte and the check word
        v2 = body + container.make_seal(body, 3, fc, MODEL, crcs, L)
        S = 20 + 12 * m + total
        assert sealed[:len(body)] == v2[:len(body)] and sealed[len(body) + S:-20] == v2[len(body):-20] and sealed[-19:-4] == v2[-19:-4]
        got, seal = container.split_seal(sealed)
        assert got == body and seal == container.Seal(3, fc, MODEL, L, crcs, G, rows, R)
        assert seal.parity_streams == R and seal.parity_group == G and seal.parity_groups == m
        assert [[[bytes(q) for q in p] for p in row] for row in seal.parity] == rows
        assert isinstance(seal.parity[0][0], list) and isinstance(seal.parity[0][0][0], memoryview)
        view, seal_v = container.split_seal(sealed, view=True)
        assert isinstance(view, memoryview) and bytes(view) == body and seal_v == seal
        assert 'parity_streams={}'.format(R) in repr(seal)
        # not the seal of the band-sealed file, not that of the 'L3CP' file, and it differs by a byte of a row above row 0
        row0 = [[p[0] for p in row] for row in rows]
        assert seal != container.Seal(3, fc, MODEL, L, crcs) and seal != container.Seal(3, fc, MODEL, L, crcs, G, row0)
        if total:
            c, g = next((c, g) for c in range(3) for g in range(m) if len(rows[c][g][0]))
            other = [[list(p) for p in row] for row in rows]
            other[c][g][R - 1] = bytes([other[c][g][R - 1][0] ^ 1]) + other[c][g][R - 1][1:]
            assert seal != container.Seal(3, fc, MODEL, L, crcs, G, other, R)
    for args in ((0, 1, 2, 0), (1025, 1, 2, 0), (4, 0, 2, 0), (4, 5, 2, 0), (4, 2, 2, -2), (4, 2, 2, 1 << 32), (4, 2, 0, 0), (4, 2, 5, 0), (4, 2, 2, 3)):
        assert lib.l3c_seal_parity_rs_bytes(*args) == INVALID, args
    assert lib.l3c_seal_parity_rs_bytes(6, 2, 1, 10) == lib.l3c_seal_parity_bytes(6, 2, 10)


def test_one_stream_and_versions_1_and_2_are_unchanged_byte_for_byte():
    body = _body()
    fc, crcs = _band_crcs(16 * 24, 64, 0)
    finest = _finest(16, 24, 64, 0)
    xor = [container.band_parity(ch, 4) for ch in finest]
    as_lists = [[[p] for p in row] for row in xor]
    p_file = container.make_seal(body, 3, fc, MODEL, crcs, 64, parity=(4, xor))
    assert container.make_seal(body, 3, fc, MODEL, crcs, 64, parity=(4, as_lists)) == p_file and p_file[:4] == b'L3CP'
    assert [[rows[0] for rows in container.rs_parity(ch, 4, 1)] for ch in finest] == xor
    # 'L3CP' by hand, as tests/test_parity_format.py writes it
    head = b'L3CP' + struct.pack('<HH', 4, 2) + b''.join(struct.pack('<I', len(p)) for row in xor for p in row)
    S = 16 + 12 * 2 + sum(len(p) for row in xor for p in row)
    tail = struct.pack('<I', S) + SEP
    T = 20 + 12 * 6
    table = b'L3CT' + struct.pack('<HHI', 6, 0, 64) + crcs.astype('<u4').tobytes() + struct.pack('<I', T) + SEP
    seal = b'L3CS' + struct.pack('<BBHIQ', 3, 0, 3, fc, MODEL)
    assert p_file == head + b''.join(p for row in xor for p in row) + tail + table + seal + struct.pack('<I', zlib.crc32(body[6:14] + head + tail + table + seal))
    got, s = container.split_seal(body + p_file)
    assert got == body and s.parity_streams == 1 and s == container.Seal(3, fc, MODEL, 64, crcs, 4, xor) and isinstance(s.parity[0][0], memoryview)
    # versions 1 and 2
    v1 = container.make_seal(body, 3, 0xCAFEF00D, 7)
    h1 = b'L3CS' + struct.pack('<BBHIQ', 1, 0, 3, 0xCAFEF00D, 7)
    assert v1 == h1 + struct.pack('<I', zlib.crc32(body[6:14] + h1))
    s1 = container.split_seal(body + v1)[1]
    assert s1 == container.Seal(3, 0xCAFEF00D, 7) and s1.parity is None and s1.parity_streams is None
    v2 = container.make_seal(body, 3, fc, MODEL, crcs, 64)
    h2 = b'L3CS' + struct.pack('<BBHIQ', 2, 0, 3, fc, MODEL)
    assert v2 == table + h2 + struct.pack('<I', zlib.crc32(body[6:14] + table + h2))
    s2 = container.split_seal(body + v2)[1]
    assert s2.parity is None and s2.parity_streams is None
    rows2 = [_rs_by_hand(ch, 4, 2) for ch in finest]
    with pytest.raises(ValueError, match='band seal'):
        container.make_seal(body, 3, fc, MODEL, parity=(4, rows2))
    with pytest.raises(ValueError, match='row payloads of one length'):
        container.make_seal(body, 3, fc, MODEL, crcs, 64, parity=(4, [[[p[0], p[1] + b'x'] for p in row] for row in rows2]))
    with pytest.raises(ValueError, match='parity_streams'):
        container.make_seal(body, 3, fc, MODEL, crcs, 64, parity=(4, [[p * 3 for p in row] for row in rows2]))


def test_a_damaged_parity_payload_leaves_the_file_readable():
    body, fc, crcs, rows, sealed = _sealed()
    at = len(body) + 12 + 12 * 2
    total = 2 * sum(len(p[0]) for row in rows for p in row)
    for k in (0, total // 2, total - 1):
        bad = bytearray(sealed)
        bad[at + k] ^= 0x5A
        got, seal = container.split_seal(bytes(bad))
        assert got == body and seal.band_len == 64 and (seal.band_crcs == crcs).all()
        assert b''.join(bytes(q) for row in seal.parity for p in row for q in p) == bytes(bad[at:at + total])
        assert _find_rs(bytes(bad))[0][:2] == (1, len(body))


def _resealed(body, section, table, fc, version=3):
    """The check word made right for a (changed) 'L3CQ' section and table."""
    m, = struct.unpack('<H', section[6:8])
    head = section[:12 + 12 * m] if 12 + 12 * m <= len(section) - 8 else b''
    seal = b'L3CS' + struct.pack('<BBHIQ', version, 0, 3, fc, 9)
    return body + section + table + seal + struct.pack('<I', zlib.crc32(body[6:14] + head + section[-8:] + table + seal))


def test_every_reader_error_python_and_c_alike():
    body, fc, crcs, rows, sealed = _sealed()          # n = 6, G = 4, m = 2, R = 2
    n, m, R, T = 6, 2, 2, 20 + 12 * 6
    plen = [len(p[0]) for row in rows for p in row]
    S = 20 + 12 * m + R * sum(plen)
    section, table = sealed[len(body):len(body) + S], sealed[len(body) + S:len(body) + S + T]

    def with_fields(G=4, mm=m, RR=R, reserved=0, lens=plen, Sfield=S, sig=b'L3CQ'):
        payload = section[12 + 12 * m:-8]
        s = sig + struct.pack('<HHHH', G, mm, RR, reserved) + b''.join(struct.pack('<I', v) for v in lens) + payload + struct.pack('<I', Sfield) + SEP
        return _resealed(body, s, table, fc)
    swapped = list(plen)
    swapped[0], swapped[1] = plen[0] + 1, plen[1] - 1
    legacy = struct.pack('<4H', *PAD) + struct.pack('<BHH', 1, 8, 8) + struct.pack('<I', 3) + b'abc' + SEP
    other = _body(16, 24, 64, seed=1)                 # the same shape, other payload lengths
    at = len(body)
    cases = {
        'R = 0': (with_fields(RR=0), "states 0 parity streams, an 'L3CQ' section holds 2..4"),
        'R = 1 is never an L3CQ section': (with_fields(RR=1), "states 1 parity streams, an 'L3CQ' section holds 2..4"),
        'R = 5': (with_fields(RR=5), "states 5 parity streams, an 'L3CQ' section holds 2..4"),
        'R = 65535': (with_fields(RR=65535), "states 65535 parity streams"),
        'reserved': (with_fields(reserved=1), 'parity section with a non-zero reserved field'),
        'reserved high byte': (with_fields(reserved=0x100), 'parity section with a non-zero reserved field'),
        'R = 3: a wrong S': (with_fields(RR=3), '20 + 12 m + R times the sum'),
        'R = 4: a wrong S': (with_fields(RR=4), '20 + 12 m + R times the sum'),
        'S is not the sum': (with_fields(lens=[plen[0] + 1] + plen[1:]), '20 + 12 m + R times the sum'),
        'S = 0': (with_fields(Sfield=0), 'last scale separator'),
        'S too small': (with_fields(Sfield=27), 'last scale separator'),
        'S beyond the file': (with_fields(Sfield=len(body) + S), 'last scale separator'),
        'S not at a separator': (with_fields(Sfield=S + 4), 'last scale separator'),
        'an unknown section signature': (with_fields(sig=b'L3CX'), "parity section without its 'L3CP' signature"),
        'm = 0': (with_fields(mm=0), 'too short for its 0 x 3 length fields'),
        'm too large for S': (with_fields(mm=1000), 'too short for its 1000 x 3 length fields'),
        'm = 3': (with_fields(mm=3), '20 + 12 m + R times the sum'),
        'G = 2 (m would be 3)': (with_fields(G=2), 'finest scale record'),
        'G = 0': (with_fields(G=0), 'finest scale record'),
        'G = 7 > n': (with_fields(G=7), 'finest scale record'),
        'plen is not the longest member': (with_fields(lens=swapped), "longest member's"),
        'plen of another body': (_resealed(other, section, table, fc), "longest member's"),
        'legacy body': (legacy + section + table + sealed[-24:], 'legacy file (version 3, the parity seal'),
        'check word': (sealed[:-1] + bytes([sealed[-1] ^ 1]), 'check word'),
        'check word (G)': (sealed[:at + 4] + bytes([sealed[at + 4] ^ 1]) + sealed[at + 5:], 'check word'),
        'check word (R: 2 -> 3 does not fit S)': (sealed[:at + 8] + bytes([sealed[at + 8] ^ 1]) + sealed[at + 9:], '20 + 12 m + R times the sum'),
        'check word (two plen moved, S kept)': (body + section[:12] + struct.pack('<2I', plen[0] + 1, plen[1] - 1) + section[20:] + sealed[at + S:],
                                                'check word'),
        'check word (padding)': (sealed[:8] + bytes([sealed[8] ^ 2]) + sealed[9:], 'check word'),
        'check word (table)': (sealed[:at + S + 14] + bytes([sealed[at + S + 14] ^ 0x10]) + sealed[at + S + 15:], 'check word'),
        'flags': (sealed[:-19] + b'\x01' + sealed[-18:], 'flags'),
        'T = 0': (sealed[:-32] + struct.pack('<I', 0) + sealed[-28:], 'length field'),
        'no L3CT': (_resealed(body, section, b'L3CX' + table[4:], fc), "'L3CT'"),
        'n field': (_resealed(body, section, table[:4] + struct.pack('<H', 3) + table[6:], fc), 'band count'),
        'frame CRC': (_resealed(body, section, table, fc ^ 1), 'combination'),
        'a version the reader does not know': (sealed[:-20] + b'\x04' + sealed[-19:], 'unknown version'),
    }
    lib = _lib.load()
    for what, (f, needle) in cases.items():
        assert container.is_sealed(f), what
        with pytest.raises(ValueError, match='invalid file: seal') as e:
            container.split_seal(f)
        assert not isinstance(e.value, container.SealError)
        got, msg = _find_rs(f)
        assert got[0] == INVALID and msg == str(e.value), (what, msg, str(e.value))
        assert needle in msg, (what, msg)
        size = ctypes.c_int64()
        assert lib.l3c_seal_find(f, len(f), ctypes.byref(size), None) == INVALID and lib.l3c_last_error().decode() == msg, what
        assert lib.l3c_seal_find_bands(f, len(f), ctypes.byref(size), None, None) == INVALID and lib.l3c_last_error().decode() == msg, what
        assert lib.l3c_seal_find_parity(f, len(f), ctypes.byref(size), None, None, None) == INVALID and lib.l3c_last_error().decode() == msg, what


def _wide_file(n, G, R):
    """A band-sealed file of n bands of 64 (one byte each) with an 'L3CQ' section over groups of G, the section written by hand."""
    H, W = 64, n
    payloads = [[bytes([(7 * c + j) % 251]) for j in range(n)] for c in range(3)]
    body = container.write_file(PAD, [(1, 8, 8, 64), (3, H, W, 64)], [[[b'abc']], payloads], True)
    fc, crcs = _band_crcs(H * W, 64, n)
    m = -(-n // G)
    rows = [[[b'\0'] * R for _ in range(m)] for _ in range(3)]             # (payload bytes are not under the check word, nor checked)
    return body, body + _by_hand(body, 3, fc, MODEL, crcs, 64, G, R, rows), fc, crcs


def test_more_than_one_stream_needs_groups_of_at_most_255_bands():
    body, f, fc, crcs = _wide_file(512, 256, 2)
    with pytest.raises(ValueError, match='invalid file: seal parity section with more than one stream over groups of more than 255 bands') as e:
        container.split_seal(f)
    got, msg = _find_rs(f)
    assert got[0] == INVALID and msg == str(e.value)
    body, f, fc, crcs = _wide_file(512, 255, 2)                              # m = 3: groups of 171, 171, 170
    assert container.split_seal(f)[1].parity_streams == 2 and _find_rs(f)[0][:2] == (1, len(body))
    with pytest.raises(ValueError, match='at most 255'):
        container.make_seal(body, 3, fc, MODEL, crcs, 64, parity=(256, [[[b'\0', b'\0']] * 2] * 3))
    lib = _lib.load()
    plen = np.ones(6, dtype=np.uint32)
    out = ctypes.create_string_buffer(1 << 16)
    seal = ctypes.byref(_lib.Seal(3, 1, 1))
    words = np.zeros(3 * 512, dtype=np.uint32)
    assert lib.l3c_seal_write_parity_rs(seal, b'x' * 8, words.ctypes.data, 512, 64, 256, 2, plen.ctypes.data, b'x' * 12, out) == INVALID
    assert 'at most 255' in lib.l3c_last_error().decode()
    assert lib.l3c_seal_write_parity_rs(seal, b'x' * 8, words.ctypes.data, 512, 64, 256, 1, plen.ctypes.data, b'x' * 6, out) == 0


def test_python_and_c_write_the_same_bytes_and_every_entry_reads_them():
    lib = _lib.load()
    for H, W, L, G, R, seed in ((16, 24, 64, 4, 2, 1), (16, 24, 64, 6, 3, 2), (16, 16, 64, 1, 4, 3), (8, 8, 64, 1, 2, 4), (32, 32, 64, 5, 4, 5)):
        body, fc, crcs, rows, sealed = _sealed(H, W, L, G, R, seed)
        n = crcs.shape[1]
        m = -(-n // G)
        payload = b''.join(q for row in rows for p in row for q in p)
        plen = np.asarray([len(p[0]) for row in rows for p in row], dtype=np.uint32)
        out = ctypes.create_string_buffer(lib.l3c_seal_parity_rs_bytes(n, m, R, len(payload)))
        words = np.ascontiguousarray(crcs)
        assert lib.l3c_seal_write_parity_rs(ctypes.byref(_lib.Seal(3, fc, MODEL)), body[6:14], words.ctypes.data, n, L, G, R, plen.ctypes.data, payload,
                                            out) == 0
        assert out.raw == sealed[len(body):]
        got, _ = _find_rs(sealed)
        assert got == (1, len(body), (3, fc, MODEL), n, L, G, m, R, len(payload), len(body) + 12 + 12 * m)
        # callers that know versions 1 and 2, or the 'L3CP' section, alone: sealed, the body in front of the section, the band table filled
        size, seal, bands, par = ctypes.c_int64(-7), _lib.Seal(), _lib.SealBands(), _lib.SealParity(9, 9, 1, 1, 9)
        assert lib.l3c_seal_find(sealed, len(sealed), ctypes.byref(size), ctypes.byref(seal)) == 1
        assert size.value == len(body) and (seal.generation, seal.frame_crc, seal.model_id) == (3, fc, MODEL)
        size = ctypes.c_int64(-7)
        assert lib.l3c_seal_find_bands(sealed, len(sealed), ctypes.byref(size), ctypes.byref(seal), ctypes.byref(bands)) == 1
        assert size.value == len(body) and bands.n == n and bands.band_len == L
        size, bands = ctypes.c_int64(-7), _lib.SealBands()
        assert lib.l3c_seal_find_parity(sealed, len(sealed), ctypes.byref(size), ctypes.byref(seal), ctypes.byref(bands), ctypes.byref(par)) == 1
        assert size.value == len(body) and bands.n == n and bands.band_len == L
        assert (par.G, par.m, par.plen, par.payloads, par.payload_bytes) == (0, 0, None, None, 0)
        table = np.frombuffer(ctypes.string_at(bands.crc, 12 * n), dtype='<u4').reshape(3, n)
        assert (table == crcs).all()
        # one stream through the new entries: 'L3CP', R = 1
        xor = [[p[0] for p in row] for row in rows]
        p_file = body + container.make_seal(body, 3, fc, MODEL, crcs, L, parity=(G, xor))
        flat = b''.join(p for row in xor for p in row)
        out1 = ctypes.create_string_buffer(lib.l3c_seal_parity_rs_bytes(n, m, 1, len(flat)))
        assert lib.l3c_seal_write_parity_rs(ctypes.byref(_lib.Seal(3, fc, MODEL)), body[6:14], words.ctypes.data, n, L, G, 1, plen.ctypes.data, flat,
                                            out1) == 0
        assert out1.raw == p_file[len(body):]
        assert _find_rs(p_file)[0] == (1, len(body), (3, fc, MODEL), n, L, G, m, 1, len(flat), len(body) + 8 + 12 * m)
        # versions 1 and 2 and unsealed files
        v1 = body + container.make_seal(body, 3, 5, 6)
        assert _find_rs(v1)[0] == (1, len(body), (3, 5, 6), 0, 0, 0, 0, 0, 0, None)
        v2 = body + container.make_seal(body, 3, fc, MODEL, crcs, L)
        assert _find_rs(v2)[0] == (1, len(body), (3, fc, MODEL), n, L, 0, 0, 0, 0, None)
        assert _find_rs(body)[0][:2] == (0, len(body)) and _find_rs(body)[0][6] == 0
    seal = ctypes.byref(_lib.Seal(3, 1, 1))
    plen = np.zeros(3, dtype=np.uint32)
    out = ctypes.create_string_buffer(256)
    for R in (0, 5, -1):
        assert lib.l3c_seal_write_parity_rs(seal, b'x' * 8, b'x' * 12, 1, 64, 1, R, plen.ctypes.data, None, out) == INVALID
    assert lib.l3c_seal_write_parity_rs(None, b'x' * 8, b'x' * 12, 1, 64, 1, 2, plen.ctypes.data, None, out) == INVALID
    assert lib.l3c_seal_write_parity_rs(seal, b'x' * 8, b'x' * 12, 1, 64, 2, 2, plen.ctypes.data, None, out) == INVALID
    plen[0] = 1
    assert lib.l3c_seal_write_parity_rs(seal, b'x' * 8, b'x' * 12, 1, 64, 1, 2, plen.ctypes.data, None, out) == INVALID    # payload bytes without payloads
    assert lib.l3c_abi_version() == 4                      # symbols were added, nothing existing changed
    assert ctypes.sizeof(_lib.SealParity) == 32            # l3c_seal_parity keeps its layout


FAKE = 0x100000
SPAN = np.dtype([('offset', '<i8'), ('bytes', '<i8')])


def _said():
    return _lib.load().l3c_last_error().decode()


def _table(rows):
    t = np.zeros(len(rows), dtype=SPAN)
    for i, r in enumerate(rows):
        t[i] = r
    return t


def _gf(spans, first, slots, data=FAKE, data_bytes=4096, out=FAKE + (1 << 20), out_bytes=4096, dev=(FAKE + 8, FAKE + 16, FAKE + 24), n_groups=None,
        host=(True, True, True), coef_host=True, coef=FAKE + 33):
    spans, slots, first = _table(spans), _table(slots), np.asarray(first, dtype=np.int64)
    coefs = np.arange(1, len(spans) + 1, dtype=np.uint8)
    return _lib.load().l3c_u8_gf_spans(data, data_bytes, spans.ctypes.data if host[0] else None, dev[0], coefs.ctypes.data if coef_host else None, coef,
                                       len(spans), first.ctypes.data if host[1] else None, dev[1], len(slots) if n_groups is None else n_groups,
                                       slots.ctypes.data if host[2] else None, dev[2], out, out_bytes, None)


def test_gf_spans_argument_checks_precede_any_device_call():
    spans, first, slots = [(0, 5), (64, 17), (128, 0)], [0, 2, 3], [(0, 17), (64, 3)]
    # nothing to do is success, whatever the pointers
    assert _gf(spans, first, slots, n_groups=0, data=None, out=None, dev=(None, None, None), host=(False, False, False), coef_host=False, coef=None) == 0
    assert _gf(spans, first, slots, n_groups=-1) == INVALID and 'n_groups' in _said()
    assert _gf(spans, first, slots, n_groups=65536) == INVALID and 'n_groups' in _said()
    for host in ((False, True, True), (True, False, True), (True, True, False)):
        assert _gf(spans, first, slots, host=host) == INVALID and 'null pointer' in _said(), host
    for kw in (dict(data=None), dict(out=None), dict(dev=(None, FAKE, FAKE)), dict(dev=(FAKE, None, FAKE)), dict(dev=(FAKE, FAKE, None)),
               dict(coef_host=False), dict(coef=None)):
        assert _gf(spans, first, slots, **kw) == INVALID and 'null pointer' in _said(), kw
    assert _gf(spans, first, slots, data=FAKE + 2) == INVALID and '4-byte aligned' in _said()
    assert _gf(spans, first, slots, out=FAKE + (1 << 20) + 1) == INVALID and '4-byte aligned' in _said()
    for dev in ((FAKE + 4, FAKE, FAKE), (FAKE, FAKE + 4, FAKE), (FAKE, FAKE, FAKE + 4)):
        assert _gf(spans, first, slots, dev=dev) == INVALID and '8-byte aligned' in _said(), dev
    assert _gf(spans, first, slots, out=FAKE + 2048) == INVALID and 'overlap' in _said()
    assert _gf(spans, first, slots, data_bytes=-1) == INVALID
    # every field of a span, a group and an output slot, through the table checks l3c_u8_xor_spans makes
    bad_spans = [((-4, 5), 'negative'), ((0, -1), 'negative'), ((2, 5), 'multiple of 4'), ((4092, 5), 'exceeds data_bytes'),
                 ((4096, 1), 'exceeds data_bytes'), ((4, 2 ** 63 - 5), 'overflows'), ((2 ** 62, 2 ** 61), 'exceeds data_bytes')]
    for row, needle in bad_spans:
        for at in (0, 2):
            rows = list(spans)
            rows[at] = row
            assert _gf(rows, first, slots) == INVALID and needle in _said() and 'span {}'.format(at) in _said(), (row, _said())
    for f, needle in (([1, 2, 3], 'start at 0'), ([0, 3, 2], 'descend'), ([0, 2, 4], 'exceeds n_spans'), ([0, 1, 2], 'end at n_spans')):
        assert _gf(spans, f, slots) == INVALID and needle in _said() and 'group' in _said(), (f, _said())
    bad_slots = [((-4, 5), 'negative'), ((0, -1), 'negative'), ((6, 5), 'multiple of 4'), ((4088, 5), 'exceeds out_bytes'),
                 ((4096, 0), 'exceeds out_bytes'), ((0, 4093), 'exceeds out_bytes'), ((4, 2 ** 63 - 2), 'overflows')]
    for row, needle in bad_slots:
        for at in (0, 1):
            rows = list(slots)
            rows[at] = row
            assert _gf(spans, first, rows) == INVALID and needle in _said() and 'out span {}'.format(at) in _said(), (row, _said())


def _scale(H=16, W=24, L=64, C=3, full=FAKE, nb_full=FAKE + 4096, s_full=136, last=FAKE + 8192, nb_last=FAKE + 12288, s_last=136):
    return _lib.BandedScale(full, nb_full, s_full, last, nb_last, s_last, C, H, W, L)


def _parity(scale, B=2, G=4, R=2, parity=FAKE + (1 << 20), stride=144, nbytes=FAKE + (2 << 20), null_scale=False):
    return _lib.load().l3c_band_parity_rs(None if null_scale else ctypes.byref(scale), B, G, R, parity, stride, nbytes, None)


def test_band_parity_rs_argument_checks_precede_any_device_call():
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
    for R in (0, -1, 5, 256):
        assert _parity(_scale(), R=R) == INVALID and 'R must be in 1..4' in _said(), R
    # n = 512: groups of 256 bands have no 256 distinct points; one stream needs none
    assert _parity(_scale(H=64, W=512), G=256, R=2) == INVALID and 'at most 255' in _said()
    assert _parity(_scale(H=64, W=512), G=256, R=1, parity=None) == INVALID and 'null pointer' in _said()
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


def test_constructor_value_errors():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    for R in (0, 5, -1, 1.5, 'x', True):
        with pytest.raises(ValueError, match='parity_streams must be in 1..4'):
            Bitcoding(None, bands=16, seal='bands', parity=4, parity_streams=R)
    for kw in (dict(bands=16, seal='bands'), dict(bands=16, seal='bands', parity=0)):
        with pytest.raises(ValueError, match='parity_streams > 1 needs parity=G'):
            Bitcoding(None, parity_streams=2, **kw)
    with pytest.raises(ValueError, match="parity needs seal='bands'"):
        Bitcoding(None, bands=16, seal=True, parity=4, parity_streams=2)
    with pytest.raises(ValueError, match='at most 255'):
        Bitcoding(None, bands=512, seal='bands', parity=256, parity_streams=2)
    assert Bitcoding(None, bands=512, seal='bands', parity=256).parity_streams == 1          # one stream: no limit
    assert Bitcoding(None, bands=512, seal='bands', parity=255, parity_streams=4).parity_streams == 4
    assert Bitcoding(None, bands=200, seal='bands', parity=1000, parity_streams=2).parity_streams == 2     # min(G, n) = 200
    bc = Bitcoding(None, bands=16, seal='bands', parity=4, parity_streams=2)
    assert (bc.parity, bc.parity_streams) == (4, 2) and Bitcoding(None, bands=16, seal='bands', parity=4).parity_streams == 1


def test_rs_seal_reader_survives_truncations_and_byte_changes_under_the_sanitizers(tmp_path):
    """tests/cabi/parity_rs_check_main.cpp: csrc/seal.h alone, built with the address and undefined-behaviour sanitizers and run as a child
    process: every truncation and single-byte changes at every position of a small 'L3CQ' file in an exactly sized heap buffer, and crafted
    S, G, m, R, reserved and plen fields; each call returns 1, 0 or L3C_ERR_INVALID_ARG, the entry that knows 'L3CP' alone agrees, and a changed
    parity payload byte never makes the file unreadable."""
    exe = tmp_path / 'parity_rs_check'
    subprocess.run(['c++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'parity_rs_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith('parity_rs_check: 390 truncations, 14430 single-byte changes (2220 in parity payloads, all readable), '
                                       '62 crafted fields: '), r.stdout
