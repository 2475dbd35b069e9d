"""-m gpu: l3c_seal_append_parity (csrc/seal_parity.hip, planned by csrc/seal_parity_plan.h) at the sizes where its loops run more than
once: rows of several copy tiles, more than 256 copy units and length fields in a file, more than 64 check words, meta bytes of several
tiles, a head_crc quarter longer than one trip of the wave loop; two refusals (a body whose size is not what the records add up to, a group
length above its slot stride); and a caller's workspace between guards.

The machinery and the contract are those of tests/test_gpu_seal_append_parity.py: every file is body + container.make_seal(...) byte for
byte, file_bytes is its length, every byte of the slot behind it is still 0xA5, and container.split_seal and l3c_seal_find_head read it.

Every test first works out, from its own shapes and lengths alone (Shape: the arithmetic of seal_parity_plan.h's Plan and of the tail's
layout, in plain Python), that it is on the many-trip side it is named for, and that the files it expects have the sizes that arithmetic
gives."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd import _lib, ops  # noqa: E402
from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from tests.test_gpu_seal_append_parity import (FILL, MODEL_ID, _batch, _batch_of, _check, _crcs, _seal, _want,  # noqa: E402,F401
                                               _write_bodies)

THREADS = 256           # seal_parity_plan.h: the plan kernel's block, the unit scan's shares
TILE_BYTES = 4096       # TILE_DWORDS * 4: the destination bytes of a copy block
LANES = 64              # the check word's shares
TRIP_BYTES = 4096       # crc_wave.h: 4 rows of 1024 bytes per trip of wave_crc32's loop
_WANT = {}


def copy_tiles(longest):
    return ((longest + 3) // 4 + 1 + TILE_BYTES // 4 - 1) // (TILE_BYTES // 4)


class Shape(object):
    """A batch of B files: `headers` in front of the record `finest`, coarse(k, c, j) and fine(c, j) the bytes of a payload, file b with b
    filler bytes more in payload (0, 0, 0) of its first record -- and what the plan and the tail's layout make of them."""

    def __init__(self, key, seed, B, headers, finest, coarse, fine):
        self.key, self.seed, self.B, self.headers, self.finest, self.coarse, self.fine = key, seed, B, list(headers), finest, coarse, fine

    def batch(self):
        return _batch_of(self.key, self.seed, self.B, self.headers, self.finest, self.coarse, self.fine)

    @staticmethod
    def n(h):
        return container.n_bands(h[1] * h[2], h[3])

    @classmethod
    def m(cls, h, G):
        return -(-cls.n(h) // min(G, cls.n(h)))

    def payload(self, b, k, c, j):
        """The bytes of band j of channel c of record k (the finest: len(headers)) of file b."""
        return self.fine(c, j) if k == len(self.headers) else self.coarse(k, c, j) + (b if (k, c, j) == (0, 0, 0) else 0)

    def P0(self, b):
        """The body in front of the finest record: the file header and the records but the finest, each 9 header bytes, a length field
        per band, the payloads and the separator."""
        return 14 + sum(13 + 4 * h[0] * self.n(h) + sum(self.payload(b, k, c, j) for c in range(h[0]) for j in range(self.n(h)))
                        for k, h in enumerate(self.headers))

    def body_bytes(self, b):
        f = self.finest
        return self.P0(b) + 13 + 12 * self.n(f) + sum(self.fine(c, j) for c in range(3) for j in range(self.n(f)))

    def group_lens(self, b, k, G):
        """The row length of every group of record k in (c, g) order: the longest of its members { j : j % m == g }."""
        h = (self.headers + [self.finest])[k]
        n, m = self.n(h), self.m(h, G)
        return [max(self.payload(b, k, c, j) for j in range(g, n, m)) for c in range(h[0]) for g in range(m)]

    def plan(self, G, R, head):
        """units, fields, check words M and meta bytes of a file, as make_plan counts them."""
        f, hs = self.finest, self.headers if head else []
        m, n = self.m(f, G), self.n(f)
        units = 3 * m + (1 + sum(h[0] * self.m(h, G) for h in hs) if head else 0)
        fields = sum(h[0] * self.n(h) for h in hs + [f]) if head else 0
        plen_at = 8 if R == 1 and not head else 12
        M = 2 + (plen_at + 12 * m) // 4 + 2 + (20 + 12 * n) // 4 + 5
        meta = 0
        if head:
            meta = 4 + 14 + sum(9 + 4 * h[0] * self.n(h) for h in hs + [f]) + 4 + sum(4 * h[0] * self.n(h) + 4 + 4 * h[0] * self.m(h, G) for h in hs)
        return units, fields, M, meta

    def tail(self, b, G, R, head):
        """The rows of file b's tail in file order, [(offset in the tail, bytes, 'fine' / 'meta' / 'coarse')], and the tail's size: front,
        the finest groups' R rows each, with a head part the meta bytes, every head group's R rows and head_check, the section's last 8
        bytes, the band table, the seal."""
        f = self.finest
        units, _, _, meta = self.plan(G, R, head)
        at = (8 if R == 1 and not head else 12) + 12 * self.m(f, G)
        rows = []
        for ln in self.group_lens(b, len(self.headers), G):
            rows += [(at + r * ln, ln, 'fine') for r in range(R)]
            at += R * ln
        if head:
            rows.append((at, meta, 'meta'))
            at += meta
            for k in range(len(self.headers)):
                for ln in self.group_lens(b, k, G):
                    rows += [(at + r * ln, ln, 'coarse') for r in range(R)]
                    at += R * ln
            at += 4
        assert len(rows) == (units - bool(head)) * R + bool(head)
        return rows, at + 8 + 20 + 12 * self.n(f) + 24

    def stride(self, G, R, head, spare=40):
        return (max(self.body_bytes(b) + self.tail(b, G, R, head)[1] for b in range(self.B)) + 3) // 4 * 4 + spare


def want_of(shape, G, R, head):
    """container.make_seal's files of the batch, built once per case, with the synthetic CRC words they carry; their sizes are what the
    arithmetic of Shape says."""
    key = (shape.key, G, R, head)
    if key not in _WANT:
        scales, payloads, pads, bodies = shape.batch()
        n = Shape.n(shape.finest)
        frame, bands = _crcs(shape.B, n, 7 * G + R, shape.finest[3], shape.finest[1] * shape.finest[2])
        want = _want(bodies, payloads, frame, bands, shape.finest[3], G, R, head)
        assert [len(f) for f in bodies] == [shape.body_bytes(b) for b in range(shape.B)]
        assert [len(w) for w in want] == [shape.body_bytes(b) + shape.tail(b, G, R, head)[1] for b in range(shape.B)]
        _WANT[key] = (frame, bands, want)
    return _WANT[key]


def sealed(shape, G, R, head, stride, workspace=None):
    scales, payloads, pads, bodies = shape.batch()
    frame, bands, want = want_of(shape, G, R, head)
    files, file_bytes, padding = _write_bodies(scales, pads, bodies, stride)
    return _seal(scales, files, file_bytes, padding, frame, bands, G, R, head, workspace=workspace)


def guarded_workspace(shape, G, R, head, guard=4096):
    """A 16-byte aligned view of exactly l3c_seal_append_parity_workspace_bytes bytes inside a FILLed tensor -> (the tensor, the view)."""
    scales = shape.batch()[0]
    arr = ops._banded_scale_array(scales)
    n_ws = _lib.load().l3c_seal_append_parity_workspace_bytes(arr, len(arr), shape.B, G, R, int(head))
    assert n_ws > 0
    whole = torch.full((guard + n_ws + guard,), FILL, dtype=torch.uint8, device='cuda')
    ws = whole[guard:guard + n_ws]
    assert ws.data_ptr() % 16 == 0 and ws.numel() == n_ws and guard >= 4096
    return whole, ws


# ---- a. long rows -----------------------------------------------------------------------------------------------------------------------

LONG_LENS = [[4093, 4094, 4095, 4096, 4097], [8191, 8192, 8193, 0, 1], [12289, 4099, 3, 4100, 16385]]
LONG = Shape('long', 401, 4, [(2, 8, 24, 64)], (3, 16, 20, 64), lambda k, c, j: 4090 + 3 * j + c, lambda c, j: LONG_LENS[c][j])
LONG_CASES = [(1, 1, False), (1, 4, True), (2, 3, True), (5, 4, False), (5, 2, True)]


def long_rows_regime(G, R, head):
    """-> the slot stride, after the assertions that the case has rows on both sides of a tile's edge at every residue of the destination."""
    s = LONG
    assert Shape.n(s.finest) == 5 and Shape.n(s.headers[0]) == 3 and s.B == 4
    stride = s.stride(G, R, head)
    assert {(b * stride + s.body_bytes(b)) % 4 for b in range(s.B)} == {0, 1, 2, 3}              # a tail at every residue
    rows = [((b * stride + s.body_bytes(b) + off) % 4, ln, kind) for b in range(s.B) for off, ln, kind in s.tail(b, G, R, head)[0]]
    assert copy_tiles(max(ln for _, ln, _ in rows)) >= 5
    for sh in {sh for sh, _, _ in rows}:                                                          # a row past its first tile at every residue
        assert any(-(-(q + ln) // 4) > TILE_BYTES // 4 for q, ln, _ in rows if q == sh), sh
    if G == 1:                                                                                    # every band a group: every length a row
        assert {ln for _, ln, kind in rows if kind == 'fine'} == {ln for row in LONG_LENS for ln in row}
    if G <= 2:                 # a row that ends in front of the later tiles of the grid, beside one that does not: the early exit
        assert any(ln + 7 <= TILE_BYTES for _, ln, kind in rows if kind == 'fine') and any(ln > 3 * TILE_BYTES for _, ln, _ in rows)
    if R > 1:                                                                                     # row r + 1 at another residue than row r
        assert any(ln % 4 for _, ln, _ in rows if ln > TILE_BYTES)
    if head:
        assert all(s.P0(b) > 4 * TRIP_BYTES for b in range(s.B))                                  # a quarter of head_crc: more than one trip
        assert any(kind == 'coarse' and ln > TILE_BYTES for _, ln, kind in rows)
    return stride


@pytest.mark.parametrize('G,R,head', LONG_CASES)
def test_rows_of_several_tiles_at_every_residue(G, R, head):
    stride = long_rows_regime(G, R, head)
    bodies = LONG.batch()[3]
    want = want_of(LONG, G, R, head)[2]
    got, sizes = sealed(LONG, G, R, head, stride)
    _check(got, sizes, want, bodies, stride, head, 2)


# ---- b. many units, fields and check words ---------------------------------------------------------------------------------------------

MANY = Shape('many', 402, 2, [(5, 100, 192, 64)], (3, 128, 512, 64), lambda k, c, j: (7 * j + c) % 13, lambda c, j: (7 * j + c) % 13)
#             (G, R, head): units, fields, M
MANY_CASES = {(1, 1, False): (3072, 0, 6160), (3, 4, True): (1527, 4572, 4115), (1, 2, True): (4573, 4572, 6161), (255, 4, True): (26, 4572, 3104),
              (1024, 1, True): (9, 4572, 3092)}


def many_regime(G, R, head):
    s = MANY
    assert Shape.n(s.finest) == 1024 and Shape.n(s.headers[0]) == 300 and s.B == 2
    units, fields, M, meta = s.plan(G, R, head)
    assert (units, fields, M) == MANY_CASES[G, R, head]
    if G <= 3:                                                      # every thread's share: several units
        per = -(-units // THREADS)
        assert units > THREADS and per > 1
        if head:                                                    # the last thread with work has a part of a share, those behind it none
            assert units % THREADS != 0 and units % per != 0 and -(-units // per) < THREADS
        else:                                                       # 256 whole shares
            assert units == per * THREADS
    else:
        assert units < THREADS and M > 2 * LANES
    assert M > 2 * LANES and M % LANES != 0
    if head:
        assert fields > THREADS and fields % THREADS != 0 and meta > TILE_BYTES
    lens = [s.payload(0, 1, c, j) for c in range(3) for j in range(1024)]
    assert min(lens) == 0 and max(lens) == 12 and lens.count(0) > 100          # empty bands throughout
    return s.stride(G, R, head)


@pytest.mark.parametrize('G,R,head', sorted(MANY_CASES))
def test_many_units_fields_and_check_words(G, R, head):
    stride = many_regime(G, R, head)
    bodies = MANY.batch()[3]
    want = want_of(MANY, G, R, head)[2]
    got, sizes = sealed(MANY, G, R, head, stride)
    _check(got, sizes, want, bodies, stride, head, 2)


# ---- c. two refusals -------------------------------------------------------------------------------------------------------------------

def _refused_and_written(got, sizes, want, bodies, refused):
    for b, (w, body) in enumerate(zip(want, bodies)):
        if b in refused:
            assert sizes[b] == -1, (b, sizes[b])
            assert got[b, :len(body)].tobytes() == body and (got[b, len(body):] == FILL).all(), b
        else:
            assert sizes[b] == len(w) and got[b, :sizes[b]].tobytes() == w and (got[b, sizes[b]:] == FILL).all(), b


def test_a_body_that_is_not_what_the_records_add_up_to_is_refused():
    """With a head part the plan kernel adds up the file from its records: file 1 enters one byte longer than it is, file 2 four bytes
    shorter, both with room in their slots -> -1, the slots as they were.  Files 0 and 3 are written."""
    B, G, R = 4, 2, 2
    scales, payloads, pads, bodies = _batch(2, B)
    frame, bands = _crcs(B, 5, 19)
    want = _want(bodies, payloads, frame, bands, 64, G, R, True)
    stride = (max(len(w) for w in want) + 3) // 4 * 4 + 8
    assert all(len(w) + 1 <= stride for w in want)
    files, file_bytes, padding = _write_bodies(scales, pads, bodies, stride)
    file_bytes[1] += 1
    file_bytes[2] -= 4
    got, sizes = _seal(scales, files, file_bytes, padding, frame, bands, G, R, True)
    _refused_and_written(got, sizes, want, bodies, {1, 2})


@pytest.mark.parametrize('which,head', [('finest', False), ('finest', True), ('head', True)])
def test_a_group_length_above_its_slot_stride_is_refused(which, head):
    """One group of file 1 states parity_stride + 4 bytes (not the overrun marker) after the parity kernels have run -> the file becomes -1
    and its slot stays as it was; the others are written.  The group is not the last of its buffer and the file's slot has room for the
    longer rows: rows of that length would still lie inside the slot buffer and the file slot."""
    B, G, R = 4, 2, 2
    scales, payloads, pads, bodies = _batch(2, B)
    frame, bands = _crcs(B, 5, 23)
    want = _want(bodies, payloads, frame, bands, 64, G, R, head)
    spare = 512
    stride = (max(len(w) for w in want) + 3) // 4 * 4 + spare
    files, file_bytes, padding = _write_bodies(scales, pads, bodies, stride)

    def between(parity, hd):
        slots, nbytes = (parity if which == 'finest' else hd[1:])
        if which == 'finest':
            slot_stride, at = slots.shape[-1], (1, 0, 1)                   # file 1, channel 0, group 1 of (B, 3, m = 3)
            assert tuple(nbytes.shape) == (B, 3, 3)
        else:
            slot_stride, at = ops.head_parity_layout(B, scales[:-1], G, R)[2], (1,)      # record 0 (C = 1, m = 1): file 1
            assert nbytes.numel() == B * 1 + B * 2 * 1
        assert R * (slot_stride + 4) + 8 <= spare and slot_stride + 4 < 0x7fffffff
        nbytes[at] = slot_stride + 4
    got, sizes = _seal(scales, files, file_bytes, padding, frame, bands, G, R, head, between=between)
    _refused_and_written(got, sizes, want, bodies, {1})


# ---- d. the workspace ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape,G,R,head,regime', [(MANY, 3, 4, True, many_regime), (LONG, 1, 4, True, long_rows_regime)])
def test_nothing_outside_the_workspace_is_written(shape, G, R, head, regime):
    """A workspace of exactly the bytes the library asks for, between guards: the guards stay, and the files are those written with a
    workspace of the wrapper's own."""
    stride = regime(G, R, head)
    bodies = shape.batch()[3]
    want = want_of(shape, G, R, head)[2]
    whole, ws = guarded_workspace(shape, G, R, head)
    got, sizes = sealed(shape, G, R, head, stride, workspace=ws)
    whole = whole.cpu().numpy()
    assert (whole[:4096] == FILL).all() and (whole[-4096:] == FILL).all()
    assert (whole[4096:-4096] != FILL).any()                                  # (it was used)
    _check(got, sizes, want, bodies, stride, head, 2)
    plain, plain_sizes = sealed(shape, G, R, head, stride)
    assert np.array_equal(got, plain) and np.array_equal(sizes, plain_sizes)
