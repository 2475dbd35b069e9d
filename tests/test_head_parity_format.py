"""Head parity (the 'L3CH' section of seal version 3) on the host, no GPU: container.make_seal(head=...) against the section's bytes restated
by hand with struct, zlib and a bit-by-bit GF(2^8) multiply; split_seal's round trip and every rejection, word for word the C side's
(csrc/seal.h behind l3c_seal_find* / l3c_seal_find_head, and the same header alone in tests/cabi/head_seal_check_main.cpp under the address
and undefined-behaviour sanitizers); a damaged head part that never makes a file unreadable; container.heal_head on every kind of head
damage the section is there for.

The bodies: 4 scale records of C = 5 / 5 / 5 / 3 channels with n = 1 / 4 / 16 / 16 bands, random payloads, some of length 0."""
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
GEN = 3
RECORDS = [(5, 8, 8, 64), (5, 16, 16, 64), (5, 32, 32, 64), (3, 64, 64, 256)]        # n = 1, 4, 16, 16
LENS = [0, 1, 3, 4, 5, 15, 16, 17, 31, 33, 64, 100]


def _n(record):
    return -(-(record[1] * record[2]) // record[3])


def _payloads(seed):
    rng = np.random.RandomState(seed)
    return [[[rng.randint(0, 256, size=LENS[rng.randint(len(LENS))], dtype=np.uint8).tobytes() for _ in range(_n(r))] for _ in range(r[0])]
            for r in RECORDS]


def _mul(a, b):
    """a b mod 0x11D, bit by bit: independent of the tables in container."""
    p = 0
    for i in range(8):
        if (b >> i) & 1:
            p ^= a << i
    for i in range(14, 7, -1):
        if (p >> i) & 1:
            p ^= 0x11D << (i - 8)
    return p


def _rows_by_hand(payloads, G, R):
    """[m][R] rows of one channel, byte by byte: member k of group g is band g + k m, its point 2^k, row r = XOR of (2^k)^r d_k."""
    n = len(payloads)
    m = -(-n // G)
    res = []
    for g in range(m):
        members = [payloads[j] for j in range(g, n, m)]
        rows = [bytearray(max(len(p) for p in members)) for _ in range(R)]
        for k, p in enumerate(members):
            x = 1
            for _ in range(k):
                x = _mul(x, 2)
            w = 1
            for r in range(R):
                for i, v in enumerate(p):
                    rows[r][i] ^= _mul(w, v)
                w = _mul(w, x)
        res.append([bytes(row) for row in rows])
    return res


def _file(G=4, R=2, seed=0, head=True):
    """-> (body, payloads, band CRC words, frame CRC, the sealed file)."""
    payloads = _payloads(seed)
    body = container.write_file(PAD, RECORDS, payloads, True)
    n = _n(RECORDS[-1])
    crcs = np.random.RandomState(seed + 100).randint(0, 1 << 32, size=(3, n), dtype=np.uint64).astype(np.uint32)
    fc = container.combine_band_crcs(crcs, RECORDS[-1][3], RECORDS[-1][1] * RECORDS[-1][2])
    rows = [container.rs_parity(ch, G, R) for ch in payloads[-1]]
    seal = container.make_seal(body, GEN, fc, MODEL, crcs, RECORDS[-1][3], parity=(G, rows),
                               head=container.head_from_body(body, G, R) if head else None)
    return body, payloads, crcs, fc, body + seal


def _head_by_hand(body, payloads, G, R, records=None):
    """The HEAD PART restated from the layout in INTEGRATION.md ("Head parity") alone.  records (with payloads to match): a part that
    states other records than the body holds -- consistent in itself, head_check included."""
    fits = records is None
    records = RECORDS if fits else records
    meta = struct.pack('<HH', len(records), 0) + body[:14]
    at = 14
    for k, (r, chans) in enumerate(zip(records, payloads)):
        if k == len(records) - 1:
            P0 = at
        meta += struct.pack('<BHHI', *r) + b''.join(struct.pack('<I', len(p)) for ch in chans for p in ch)
        at += 9 + sum(4 + len(p) for ch in chans for p in ch) + 4
    assert at == len(body) or not fits
    meta += struct.pack('<I', zlib.crc32(body[:P0]))
    rows_bytes = b''
    for r, chans in zip(records[:-1], payloads[:-1]):
        n = _n(r)
        Gk = min(G, n)
        m = -(-n // Gk)
        rows = [_rows_by_hand(ch, Gk, R) for ch in chans]
        meta += b''.join(struct.pack('<I', zlib.crc32(p)) for ch in chans for p in ch) + struct.pack('<HH', Gk, m)
        meta += b''.join(struct.pack('<I', len(rows[c][g][0])) for c in range(r[0]) for g in range(m))
        rows_bytes += b''.join(q for c in range(r[0]) for g in range(m) for q in rows[c][g])
    return meta + rows_bytes + struct.pack('<I', zlib.crc32(meta)), len(meta), P0


def _tail_by_hand(body, payloads, crcs, fc, G, R, head_part):
    n = _n(RECORDS[-1])
    m = -(-n // G)
    rows = [_rows_by_hand(ch, G, R) for ch in payloads[-1]]
    front = b'L3CH' + struct.pack('<HHHH', G, m, R, 0) + b''.join(struct.pack('<I', len(rows[c][g][0])) for c in range(3) for g in range(m))
    finest = b''.join(q for c in range(3) for g in range(m) for q in rows[c][g])
    S = len(front) + len(finest) + len(head_part) + 8
    last8 = struct.pack('<I', S) + SEP
    table = b'L3CT' + struct.pack('<HHI', n, 0, RECORDS[-1][3]) + crcs.astype('<u4').tobytes() + struct.pack('<I', 20 + 12 * n) + SEP
    seal = b'L3CS' + struct.pack('<BBHIQ', 3, 0, GEN, fc, MODEL)
    return front + finest + head_part + last8 + table + seal + struct.pack('<I', zlib.crc32(body[6:14] + front + last8 + table + seal))


def _find_all(f):
    """Every C reader on `f` -> (rc of find_parity_rs, message, the SealParityRS, rc of find_head, the SealHead); all five entries must agree."""
    lib = _lib.load()
    size, seal, bands, rs, hd = ctypes.c_int64(), _lib.Seal(), _lib.SealBands(), _lib.SealParityRS(), _lib.SealHead()
    buf = (ctypes.c_uint8 * len(f)).from_buffer_copy(f)
    rc = lib.l3c_seal_find_parity_rs(buf, len(f), ctypes.byref(size), ctypes.byref(seal), ctypes.byref(bands), ctypes.byref(rs))
    msg = lib.l3c_last_error().decode() if rc == INVALID else ''
    p = _lib.SealParity()
    for other in (lib.l3c_seal_find(buf, len(f), ctypes.byref(size), None), lib.l3c_seal_find_bands(buf, len(f), ctypes.byref(size), None, None),
                  lib.l3c_seal_find_parity(buf, len(f), ctypes.byref(size), None, None, ctypes.byref(p))):
        assert other == rc and (rc != INVALID or lib.l3c_last_error().decode() == msg)
    rch = lib.l3c_seal_find_head(buf, len(f), ctypes.byref(hd))
    assert rch == (INVALID if rc == INVALID else rch) and (rch != INVALID or lib.l3c_last_error().decode() == msg)
    if rch == 1:
        assert p.m == 0                                        # 'L3CH' reads as the band-sealed file it contains there, R = 1 included
    return rc, msg, (rs.G, rs.m, rs.R, rs.payload_bytes, size.value), rch, (hd.at, hd.bytes, hd.check_ok, hd.n_records)


@pytest.mark.parametrize('G,R', [(4, 2), (4, 1), (16, 3), (3, 4), (1, 1)])
def test_the_section_is_the_documented_one_and_the_round_trip(G, R):
    body, payloads, crcs, fc, f = _file(G, R)
    head_part, meta_bytes, P0 = _head_by_hand(body, payloads, G, R)
    assert f[len(body):] == _tail_by_hand(body, payloads, crcs, fc, G, R, head_part)
    got, seal = container.split_seal(f)
    assert got == body and seal.head is not None and not seal.head_damaged
    assert (seal.parity_group, seal.parity_streams, seal.band_len) == (G, R, RECORDS[-1][3]) and np.array_equal(seal.band_crcs, crcs)
    m = -(-_n(RECORDS[-1]) // G)
    assert [[[bytes(q) for q in seal.rows(c, g)] for g in range(m)] for c in range(3)] == [_rows_by_hand(ch, G, R) for ch in payloads[-1]]
    h = seal.head
    assert h.records == RECORDS and h.file_header == body[:14] and h.head_crc == zlib.crc32(body[:P0]) and h.positions(3)[0] == P0
    for k, (r, chans) in enumerate(zip(RECORDS[:-1], payloads[:-1])):
        Gk = min(G, _n(r))
        assert h.groups[k] == (Gk, -(-_n(r) // Gk))
        assert h.crcs[k].tolist() == [[zlib.crc32(p) for p in ch] for ch in chans]
        assert [[[bytes(q) for q in grp] for grp in ch] for ch in h.rows[k]] == [_rows_by_hand(ch, Gk, R) for ch in chans]
    # the same seal as the 'L3CQ' / 'L3CP' file's, and that file's bytes are today's
    _, _, _, _, plain = _file(G, R, head=False)
    assert plain[len(body):len(body) + 4] == (b'L3CP' if R == 1 else b'L3CQ') and container.split_seal(plain)[1] == seal
    assert container.split_seal(plain)[1].head is None and not container.split_seal(plain)[1].head_damaged
    # the C side: every entry reads it, the finest rows and the head part's place
    rc, _, rs, rch, hd = _find_all(f)
    front = 12 + 12 * m
    finest_bytes = R * sum(len(_rows_by_hand(ch, G, 1)[g][0]) for ch in payloads[-1] for g in range(m))
    assert (rc, rs) == (1, (G, m, R, finest_bytes, len(body)))
    assert (rch, hd) == (1, (len(body) + front + finest_bytes, len(head_part), 1, 4))
    assert _find_all(plain)[3:] == (0, (0, 0, 0, 0)) and _find_all(body)[3] == 0


def test_make_seal_refuses_a_head_without_parity_or_of_another_shape():
    body, payloads, crcs, fc, _ = _file()
    head = container.head_from_body(body, 4, 2)
    with pytest.raises(ValueError, match='head needs parity'):
        container.make_seal(body, GEN, fc, MODEL, crcs, 256, head=head)
    rows = [container.rs_parity(ch, 4, 2) for ch in payloads[-1]]
    with pytest.raises(ValueError, match='one .crc, rows. pair per record but the finest'):
        container.make_seal(body, GEN, fc, MODEL, crcs, 256, parity=(4, rows), head=head[:2])
    with pytest.raises(ValueError, match='rows of one length per group'):
        container.make_seal(body, GEN, fc, MODEL, crcs, 256, parity=(4, rows), head=container.head_from_body(body, 4, 3))
    # the framing handed in by a caller that holds it (the encoder) gives the same bytes, and is checked against the body's size
    lens = [np.array([[len(p) for p in ch] for ch in rec]) for rec in payloads]
    assert container.make_seal(body, GEN, fc, MODEL, crcs, 256, parity=(4, rows), head=head, head_framing=(RECORDS, lens)) == \
        container.make_seal(body, GEN, fc, MODEL, crcs, 256, parity=(4, rows), head=head)
    lens[1] = lens[1] + 1
    with pytest.raises(ValueError, match='the framing given for the head adds up to'):
        container.make_seal(body, GEN, fc, MODEL, crcs, 256, parity=(4, rows), head=head, head_framing=(RECORDS, lens))


def _rehead(f, body, change):
    """`f` with its head part's bytes in front of the rows changed by change(bytearray) and head_check made to fit again."""
    _, seal = container.split_seal(f)
    t = container._tail(f)
    hp = bytearray(f[t.head_at:t.head_end])
    meta = bytearray(hp[:seal.head.meta_bytes])
    tail = change(meta) or b''
    rows = hp[seal.head.meta_bytes:-4]
    new = bytes(meta) + bytes(rows) + tail
    new += struct.pack('<I', zlib.crc32(bytes(meta)))
    assert len(new) == len(hp), 'the cases below keep the section length'
    return f[:t.head_at] + new + f[t.head_end:]


def _rejections():
    body, payloads, crcs, fc, f = _file()
    seal = container.split_seal(f)[1]
    h = seal.head
    # where things lie inside the head part's meta bytes
    rec_at, at = [], 18
    for r in RECORDS:
        rec_at.append(at)
        at += 9 + 4 * r[0] * _n(r)
    groups_at, at = [], at + 4
    for k, r in enumerate(RECORDS[:-1]):
        at += 4 * r[0] * _n(r)
        groups_at.append(at)
        at += 4 + 4 * r[0] * h.groups[k][1]

    def put(at, fmt, *v):
        def change(meta):
            meta[at:at + struct.calcsize(fmt)] = struct.pack(fmt, *v)
        return change
    len0 = struct.unpack_from('<I', f, container._tail(f).head_at + rec_at[1] + 9)[0]
    hplen0 = int(h.hplen[1][0, 0])
    cases = {
        'reserved': (put(2, '<H', 1), 'head with a non-zero reserved field'),
        # (a copy whose length field changed moves everything behind the payload in the body: the sum no longer ends at the section)
        'another body length': (put(rec_at[1] + 9, '<I', len0 + 1), 'head copy adds up to another body length'),
        # (a copy whose n or C changed no longer parses to the bytes head_check was taken over: damaged, not refused)
        'L patched in the copy of the finest record': (put(rec_at[3], '<BHHI', 3, 64, 64, 512), None),
        'C patched in the copy of the finest record': (put(rec_at[3], '<B', 5), None),
        'another group size': (put(groups_at[2], '<H', 3), 'head states a group size or count that is not min(G, n) and ceil(n / G)'),
        'another group count': (put(groups_at[2], '<HH', 4, 2), None),             # (m sizes hplen: the part no longer parses)
        'hplen is not the longest member': (put(groups_at[1] + 4, '<I', hplen0 + 1), "head length is not the one its fields add up to"),
    }
    files = {what: (_rehead(f, body, change), msg) for what, (change, msg) in cases.items()}
    # hplen changed with the rows' total kept: two neighbouring groups of one channel of the 32 x 32 record trade a byte
    m2 = h.groups[2][1]
    c, g = next((c, g) for c in range(RECORDS[2][0]) for g in range(m2 - 1) if h.hplen[2][c, g + 1] > 0)
    a, b = int(h.hplen[2][c, g]), int(h.hplen[2][c, g + 1])

    def trade(meta):
        at = groups_at[2] + 4 + 4 * (c * m2 + g)
        meta[at:at + 8] = struct.pack('<II', a + 1, b - 1)
    files['hplen traded between two groups'] = (_rehead(f, body, trade), "head states a payload length that is not its longest member's")
    t = container._tail(f)
    table, s20 = f[t.section_at + t.S:-24], f[-24:-4]

    def with_part(part):
        """`f` with another head part: S and the seal's check word made to fit."""
        S = t.head_at - t.section_at + len(part) + 8
        checked = f[t.section_at:t.section_at + 12 + 12 * t.m] + struct.pack('<I', S) + SEP
        return f[:t.head_at] + part + struct.pack('<I', S) + SEP + table + s20 + struct.pack('<I', zlib.crc32(body[6:14] + checked + table + s20))
    # a head part longer than its fields add up to: four bytes more in front of head_check
    files['a size other than the fields add up to'] = (with_part(f[t.head_at:t.head_end - 4] + b'\0\0\0\0' + f[t.head_end - 4:t.head_end]),
                                                       'head length is not the one its fields add up to')
    # head parts built by hand that are consistent in themselves -- every field, the rows, head_check -- and state other records than the body holds
    by_hand = lambda records, chans: with_part(_head_by_hand(body, chans, 4, 2, records)[0])          # noqa: E731
    files['another record count: one'] = (by_hand(RECORDS[-1:], payloads[-1:]), 'head states 1 scale record(s)')
    files['another record count: three'] = (by_hand(RECORDS[1:], payloads[1:]), 'head copy adds up to another body length')
    files['another n and L in the finest record'] = (by_hand(RECORDS[:-1] + [(3, 64, 64, 512)], payloads[:-1] + [[ch[:8] for ch in payloads[-1]]]),
                                                     'head copy of the finest record does not match the band table')
    files['another L in the finest record, the same n'] = (by_hand(RECORDS[:-1] + [(3, 64, 128, 512)], payloads),
                                                           'head copy of the finest record does not match the band table')
    files['another C in the finest record'] = (by_hand(RECORDS[:-1] + [(5, 64, 64, 256)], payloads[:-1] + [payloads[-1] + payloads[-1][:2]]),
                                               'head copy of the finest record does not match the band table')
    # one record only
    files['R = 0'] = (f[:t.section_at + 8] + struct.pack('<H', 0) + f[t.section_at + 10:], "states 0 parity streams, an 'L3CH' section holds 1..4")
    files['R = 5'] = (f[:t.section_at + 8] + struct.pack('<H', 5) + f[t.section_at + 10:], "states 5 parity streams, an 'L3CH' section holds 1..4")
    short = f[:t.section_at + t.S - 8] + struct.pack('<I', 27) + f[t.section_at + t.S - 4:]
    files['S too small'] = (short, 'last scale separator')
    return f, files


def test_every_rejection_python_and_c_alike():
    f, files = _rejections()
    # every message of container._check_head (csrc/seal.h: check_head) is produced by a case, and the three of the section's own header
    for needle in ('head with a non-zero reserved field', 'head states 1 scale record(s)', 'head length is not the one its fields add up to',
                   'head copy of the finest record does not match the band table', 'head copy adds up to another body length',
                   'head states a group size or count that is not min(G, n) and ceil(n / G)',
                   "head states a payload length that is not its longest member's", "an 'L3CH' section holds 1..4", 'last scale separator'):
        assert any(msg is not None and needle in msg for _, msg in files.values()), needle
    assert 'hplen traded between two groups' in files and 'another record count: three' in files
    for what, (g, needle) in files.items():
        assert container.is_sealed(g), what
        if needle is None:                                     # the part cannot be walked: damaged, never an error
            body, seal = container.split_seal(g)
            assert seal.head is None and seal.head_damaged, what
            rc, _, _, rch, hd = _find_all(g)
            assert (rc, rch, hd[2]) == (1, 1, 0), what
            continue
        with pytest.raises(ValueError, match='invalid file: seal') as e:
            container.split_seal(g)
        assert not isinstance(e.value, container.SealError) and needle in str(e.value), (what, str(e.value))
        rc, msg, _, rch, _ = _find_all(g)
        assert rc == INVALID and rch == INVALID and msg == str(e.value), (what, msg, str(e.value))
        if ' head ' in needle:                                 # heal_head refuses what split_seal refuses, in the same words
            with pytest.raises(ValueError) as e2:
                container.heal_head(g)
            assert str(e2.value) == str(e.value), what


def test_a_damaged_head_part_never_makes_the_file_unreadable():
    body, payloads, crcs, fc, f = _file()
    t = container._tail(f)
    plain = container.split_seal(_file(head=False)[4])[1]
    for at in list(range(t.head_at, t.head_end, 7)) + [t.head_end - 1]:
        g = f[:at] + bytes([f[at] ^ 0x20]) + f[at + 1:]
        got, seal = container.split_seal(g)
        assert got == body and seal == plain, at
        meta = at < t.head_at + container.split_seal(f)[1].head.meta_bytes or at >= t.head_end - 4
        assert seal.head_damaged == meta and (seal.head is None) == meta, at       # (a changed ROW byte leaves the part itself intact)
        rc, _, rs, rch, hd = _find_all(g)
        assert (rc, rch, hd[2]) == (1, 1, 0 if meta else 1), at
        assert rs[:3] == (4, 4, 2)
        healed, info = container.heal_head(g)
        assert healed is g and (info.section_damaged if meta else not info), at
    # cut to nothing: S says that no head part follows the rows
    cut = f[:t.head_at] + struct.pack('<I', t.head_at - t.section_at + 8) + SEP
    table, s20 = f[t.section_at + t.S:-24], f[-24:-4]
    checked = f[t.section_at:t.section_at + 12 + 12 * t.m] + cut[-8:]
    cut += table + s20 + struct.pack('<I', zlib.crc32(body[6:14] + checked + table + s20))
    got, seal = container.split_seal(cut)
    assert got == body and seal.head is None and seal.head_damaged and _find_all(cut)[3:] == (1, (t.head_at, 0, 0, 0))


# ---- heal_head ---------------------------------------------------------------------------------------------------------------------------


def _where(payloads):
    """Per record: (header position, [c][j] length field positions, separator position) in the body, from the payload lengths."""
    res, at = [], 14
    for r, chans in zip(RECORDS, payloads):
        header, at, fields = at, at + 9, []
        for ch in chans:
            fields.append([])
            for p in ch:
                fields[-1].append(at)
                at += 4 + len(p)
        res.append((header, fields, at))
        at += 4
    return res


def _flip(f, at, mask=0x04):
    return f[:at] + bytes([f[at] ^ mask]) + f[at + 1:]


def _complement(f, at, n):
    return f[:at] + bytes(v ^ 0xff for v in f[at:at + n]) + f[at + n:]


def _full_group(payloads, k, m):
    """(c, g) of a group of record k whose members are all non-empty."""
    return next((c, g) for c in range(len(payloads[k])) for g in range(m) if all(payloads[k][c][g::m]))


def _row_at(f, k, c, g, r, R):
    """Where row r of group (k, c, g) lies in the file: behind the head part's meta bytes, per head record in (c, g, r) order."""
    h, at = container.split_seal(f)[1].head, 0
    for kk in range(k + 1):
        for cc in range(h.hplen[kk].shape[0]):
            for gg in range(h.hplen[kk].shape[1]):
                if (kk, cc, gg) == (k, c, g):
                    return container._tail(f).head_at + h.meta_bytes + at + r * int(h.hplen[kk][cc, gg]), int(h.hplen[kk][cc, gg])
                at += R * int(h.hplen[kk][cc, gg])


def _a_payload(payloads, k, c, g, m, skip=0):
    """A non-empty band of group g of channel c of record k (the skip-th such)."""
    return [j for j in range(g, len(payloads[k][c]), m) if payloads[k][c][j]][skip]


def test_heal_head_returns_an_intact_file_as_it_came_and_ignores_files_without_a_head_section():
    body, _, _, _, f = _file()
    got, info = container.heal_head(f)
    assert got is f and isinstance(info, container.HeadInfo) and not info and info.framing_fixed == 0 and info.line() == 'head: ok'
    assert (info.repaired, info.failed, info.section_damaged) == ([], [], False)
    # the head part heal_head read and checked is what a split_seal that follows takes, unread: the same Seal, the same object as its head
    got, seal = container.split_seal(f, head=info.part)
    assert got == body and seal.head is info.part and seal == container.split_seal(f)[1] and not seal.head_damaged
    assert container.split_seal(_file(head=False)[4], head=info.part)[1].head is None        # (a file without the section has no head)
    for other in (body, _file(head=False)[4], _file(R=1, head=False)[4], b'', b'L3CB'):
        got, info = container.heal_head(other)
        assert got is other and info is None
    # damage in a finest band PAYLOAD is not the head's: the fast path still takes it
    where = _where(_payloads(0))
    g = _complement(f, where[3][1][1][2] + 4, 1)
    got, info = container.heal_head(g)
    assert got is g and not info


@pytest.mark.parametrize('what,kind', [('signature', 'file header'), ('version', 'file header'), ('padding', 'padding field'),
                                       ('coarse header', 'record header'), ('coarse length', 'length field'),
                                       ('finest header', 'record header'), ('finest length', 'length field'),
                                       ('coarse separator', 'separator'), ('finest separator', 'separator')])
def test_heal_head_rewrites_one_flipped_framing_bit(what, kind):
    body, payloads, _, _, f = _file()
    where = _where(payloads)
    at = {'signature': 1, 'version': 4, 'padding': 9, 'coarse header': where[1][0] + 2, 'coarse length': where[2][1][3][5],
          'finest header': where[3][0] + 6, 'finest length': where[3][1][2][7] + 1, 'coarse separator': where[0][2] + 3,
          'finest separator': where[3][2]}[what]
    g = _flip(f, at)
    with pytest.raises(ValueError, match='invalid file'):
        container.parse_banded(container.split_seal(g)[0])          # unreadable today, whichever of the two raises
    healed, info = container.heal_head(g)
    assert healed == f and healed is not g
    assert (info.framing, info.framing_fixed, info.repaired, info.failed, info.section_damaged) == ({kind: 1}, 1, [], [], False)
    assert info.line() == 'head: 1 {} restored'.format(kind)
    assert container.parse_banded(container.split_seal(healed)[0]).scales == RECORDS


@pytest.mark.parametrize('R', [1, 2, 3])
def test_heal_head_rebuilds_up_to_R_payloads_of_a_group_and_reports_the_rest(R):
    body, payloads, _, _, f = _file(4, R)
    where = _where(payloads)
    k, m = 2, 4                                                # the 32 x 32 record: n = 16, G = 4, m = 4, four members per group
    c, grp = _full_group(payloads, k, m)
    g, hit = f, []
    for i in range(R):                                         # R payloads of one group
        j = _a_payload(payloads, k, c, grp, m, i)
        g = _complement(g, where[k][1][c][j] + 4, len(payloads[k][c][j]))
        hit.append((k, c, j))
    j1 = _a_payload(payloads, 1, 0, 0, 1)                      # and one in another record
    g = _complement(g, where[1][1][0][j1] + 4, len(payloads[1][0][j1]))
    healed, info = container.heal_head(g)
    assert healed == f
    assert (sorted(info.repaired), info.failed, info.framing_fixed) == (sorted(hit + [(1, 0, j1)]), [], 0)
    assert info.line() == 'head: {} coarse payloads restored'.format(R + 1)
    # R + 1 of one group: reported, and everything else still fixed
    j = _a_payload(payloads, k, c, grp, m, R)
    g2 = _flip(_complement(g, where[k][1][c][j] + 4, len(payloads[k][c][j])), where[3][1][0][0])
    healed, info = container.heal_head(g2)
    assert sorted(info.failed) == sorted(hit + [(k, c, j)]) and info.repaired == [(1, 0, j1)] and info.framing == {'length field': 1}
    want = f
    for kk, cc, jj in info.failed:
        want = _complement(want, where[kk][1][cc][jj] + 4, len(payloads[kk][cc][jj]))
    assert healed == want
    assert info.line().startswith('head: 1 length field and 1 coarse payload restored; {} coarse payloads NOT restored'.format(R + 1))


def test_heal_head_takes_a_later_window_when_a_row_is_damaged_too():
    body, payloads, _, _, f = _file(4, 2)
    where = _where(payloads)
    k, m = 2, 4
    c, grp = _full_group(payloads, k, m)
    j = _a_payload(payloads, k, c, grp, m)
    row_at, size = _row_at(f, k, c, grp, 0, 2)
    assert size > 0 and f[row_at:row_at + size] == bytes(container.split_seal(f)[1].head.rows[k][c][grp][0])
    g = _complement(_complement(f, where[k][1][c][j] + 4, len(payloads[k][c][j])), row_at, size)
    healed, info = container.heal_head(g)
    assert info.repaired == [(k, c, j)] and not info.failed
    assert healed == _complement(f, row_at, size)              # the body is the original's; the damaged row stays as it is
    # with one row only there is no later window
    f1 = _file(4, 1)[4]
    at1, size1 = _row_at(f1, k, c, grp, 0, 1)
    g1 = _complement(_complement(f1, where[k][1][c][j] + 4, len(payloads[k][c][j])), at1, size1)
    assert container.heal_head(g1)[1].failed == [(k, c, j)]


def test_heal_head_fixes_a_length_field_and_the_payload_behind_it():
    body, payloads, _, _, f = _file()
    where = _where(payloads)
    k, c = 1, 2
    j = _a_payload(payloads, k, c, 0, 1)
    g = _complement(_flip(f, where[k][1][c][j], 0x80), where[k][1][c][j] + 4, len(payloads[k][c][j]))
    healed, info = container.heal_head(g)
    assert healed == f and info.framing == {'length field': 1} and info.repaired == [(k, c, j)] and not info.failed
    assert info.line() == 'head: 1 length field and 1 coarse payload restored'
    # two length fields and a payload: the example of the line in INTEGRATION.md
    g = _flip(g, where[3][1][1][4] + 2)
    assert container.heal_head(g)[1].line() == 'head: 2 length fields and 1 coarse payload restored'


def test_heal_head_leaves_a_file_alone_whose_checked_tail_is_damaged():
    _, _, _, _, f = _file()
    where = _where(_payloads(0))
    broken = _flip(f, where[1][0] + 2)
    for at in (len(f) - 30, len(f) - 10, container._tail(f).section_at + 5):        # the table, the seal, the section's G
        g = _flip(broken, at)
        got, info = container.heal_head(g)
        assert got is g and info is None
        with pytest.raises(ValueError, match='invalid file'):
            container.split_seal(g)


def test_repair_info_takes_the_head_as_a_keyword_with_a_default():
    info = container.RepairInfo({}, {}, container.SalvageInfo({}, {}, [], [], {}, 1), [None])
    assert info.head is None
    assert container.RepairInfo({}, {}, info.salvage, [None], 0, head=[container.HeadInfo()]).head[0].line() == 'head: ok'


def test_constructor_value_errors():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    with pytest.raises(ValueError, match='parity_head needs parity=G'):
        Bitcoding(None, bands=16, seal='bands', parity_head=True)
    with pytest.raises(ValueError, match='parity_head must be True or False'):
        Bitcoding(None, bands=16, seal='bands', parity=4, parity_head=1)


def test_kernel_argument_checks_precede_any_device_call():
    """Fake, well-aligned pointers stand in for device memory: every refusal comes before a launch."""
    lib = _lib.load()
    good = dict(out_full=0x10000, nbytes_full=0x20000, stride_full=64, out_last=0x30000, nbytes_last=0x40000, stride_last=64, C=5, H=16, W=16,
                band_len=64)

    def scale(**kw):
        v = dict(good, **kw)
        return _lib.BandedScale(v['out_full'], v['nbytes_full'], v['stride_full'], v['out_last'], v['nbytes_last'], v['stride_last'], v['C'],
                                v['H'], v['W'], v['band_len'])
    offs = (ctypes.c_int64 * 1)(0)

    def parity(sc, n=1, B=1, G=4, R=2, out=0x50000, stride=64, nb=0x60000, off=offs):
        arr = (_lib.BandedScale * 1)(sc)
        return lib.l3c_head_parity(arr, n, B, G, R, out, off, stride, nb, None)

    def crc(sc, n=1, B=1, out=0x50000):
        arr = (_lib.BandedScale * 1)(sc)
        return lib.l3c_band_payload_crc32(arr, n, B, out, None)
    for run, needle in [(lambda: parity(scale(), n=0), 'n_scales'), (lambda: parity(scale(), n=9), 'n_scales'), (lambda: parity(scale(), G=0), 'G must be'),
                       (lambda: parity(scale(), R=5), 'R must be'), (lambda: parity(scale(), R=0), 'R must be'), (lambda: parity(scale(), B=0), 'batch'),
                       (lambda: parity(scale(), stride=60), 'parity_stride'), (lambda: parity(scale(), stride=48), 'at least the coder strides'),
                       (lambda: parity(scale(), out=0x50004), '16-byte aligned'), (lambda: parity(scale(C=0)), 'C must be'),
                       (lambda: parity(scale(band_len=96)), 'multiple of 64'), (lambda: parity(scale(H=1024, W=1024)), 'more than 1024 bands'),
                       (lambda: parity(scale(out_last=0)), 'null pointer'), (lambda: parity(scale(stride_full=62)), 'multiples of 4'),
                       (lambda: parity(scale(out_full=0x10002)), '4-byte aligned'), (lambda: parity(scale(), off=(ctypes.c_int64 * 1)(8)), 'multiples of 16'),
                       (lambda: parity(scale(), B=70000), 'batch'), (lambda: parity(scale(C=1000), B=66), '65535'),
                       (lambda: parity(scale(H=512, W=64), G=256, R=2), 'at most 255 bands'),
                       (lambda: crc(scale(), n=0), 'n_scales'), (lambda: crc(scale(), B=0), 'batch'), (lambda: crc(scale(), out=0x50002), '4-byte aligned'),
                       (lambda: crc(scale(C=0)), 'C must be'), (lambda: crc(scale(band_len=0)), 'multiple of 64'), (lambda: crc(scale(nbytes_last=0)), 'null pointer'),
                       (lambda: crc(scale(stride_last=6)), 'multiples of 4'), (lambda: crc(scale(nbytes_full=0x20001)), '4-byte aligned')]:
        rc = run()
        assert rc == INVALID and needle in lib.l3c_last_error().decode(), (needle, lib.l3c_last_error().decode())


def test_the_c_reader_alone_agrees_and_survives_damage_under_the_sanitizers(tmp_path):
    """tests/cabi/head_seal_check_main.cpp: csrc/seal.h alone, built with the address and undefined-behaviour sanitizers and run as a child
    process on the cases of this module -- one file of [u32 size | bytes] records, each in an exactly sized heap buffer -- ; it prints what
    l3c_seal_find* and find_head return for each, which must be Python's word for word, and then walks every truncation and single-byte
    change of the intact file."""
    f, files = _rejections()
    cases = [('intact', f, None)] + [(what, g, needle) for what, (g, needle) in files.items()]
    t = container._tail(f)
    cases += [('a damaged head part', _flip(f, t.head_at + 30), None), ('an L3CQ file', _file(head=False)[4], None), ('unsealed', _file()[0], None)]
    path = tmp_path / 'cases.bin'
    path.write_bytes(b''.join(struct.pack('<I', len(g)) + g for _, g, _ in cases))
    exe = tmp_path / 'head_seal_check'
    subprocess.run(['c++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'head_seal_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split('\n')
    assert len(lines) == len(cases) + 1, r.stdout
    for (what, g, needle), line in zip(cases, lines):
        try:
            body, seal = container.split_seal(g)
            want = '1 {} {} {}'.format(len(body), 1 if seal.head is not None or seal.head_damaged else 0, 1 if seal.head is not None else 0) \
                if seal is not None else '0 {} 0 0'.format(len(g))
        except ValueError as e:
            want = '-1 ' + str(e)
        assert line == want, (what, line, want)
    assert lines[-1].startswith('head_seal_check: {} truncations, {} single-byte changes'.format(len(f), len(f))), lines[-1]
    assert lines[-1].endswith('every changed head byte left the file readable'), lines[-1]
