"""-m gpu: l3c_seal_append_parity (ops.seal_append_parity; csrc/seal_parity.hip) on synthetic coder outputs, no network: the bodies are
written by l3c_container_write_banded, the rows and CRC words come from the existing kernels (ops.band_parity_rs, ops.head_parity,
ops.band_payload_crc32), and every file must be body + container.make_seal(body, ..., parity=..., head=container.head_from_body(body, G, R))
byte for byte, with every byte at and behind its new end still the 0xA5 the slots were filled with.

The shapes are those of tests/test_seal_tail_bytes.py: a finest record of 16 x 20 pixels in n = 5 bands of L = 64 whose lengths hold empty
bands, empty parity payloads and unequal members; one or two coarse records; (G, R) in {(2, 1), (5, 1), (2, 2), (5, 4)}; head off and on.
File b of a batch carries b filler bytes in its first coarse payload, so that the tails of B = 4 files start at every residue mod 4, and
those of a batch of 16 at every residue mod 16."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd import _lib, ops  # noqa: E402
from l3c_pytorch_amd.bitcoding import container  # noqa: E402

FILL = 0xA5
FINEST = (3, 16, 20, 64)
LENS = [[0, 7, 3, 9, 2], [5, 0, 0, 1, 12], [0, 4, 0, 0, 0]]
COARSE = {1: [(1, 8, 10, 128)], 2: [(1, 4, 5, 64), (2, 8, 10, 64)]}
MODEL_ID = 0x1122334455667788
_CACHE = {}


def _record(rng, B, header, length):
    """One record on the device: its two coder groups (strides that are multiples of 4, not of 16; garbage behind every length) ->
    ((C, H, W, L, groups), payloads [b][c][j])."""
    C, H, W, L = header
    n = container.n_bands(H * W, L)
    lens = np.array([[[length(b, c, j) for j in range(n)] for c in range(C)] for b in range(B)], dtype=np.int32)
    groups, hosts = [], []
    for cols in ([slice(0, n - 1)] if n > 1 else []) + [slice(n - 1, n)]:
        nb = np.ascontiguousarray(lens[:, :, cols]).reshape(-1)
        stride = (int(nb.max()) + 3) // 4 * 4 + 4
        stride += 4 if stride % 16 == 0 else 0
        out = rng.randint(0, 256, size=(nb.size, stride), dtype=np.uint8)
        groups.append((torch.from_numpy(out).cuda(), torch.from_numpy(nb).cuda()))
        hosts.append((out, nb))

    def payload(b, c, j):
        out, nb = hosts[0] if j + 1 < n else hosts[-1]
        i = (b * C + c) * (n - 1) + j if j + 1 < n else b * C + c
        return out[i, :nb[i]].tobytes()
    return (C, H, W, L, groups), [[[payload(b, c, j) for j in range(n)] for c in range(C)] for b in range(B)]


def _batch_of(key, seed, B, headers, finest, coarse_length, finest_length):
    """The records of a batch of B files, built once per key: `headers` in front of the record `finest`; coarse_length(k, c, j) and
    finest_length(c, j): the bytes of a payload, and file b has b % 16 filler bytes more in its first coarse payload."""
    if key not in _CACHE:
        rng = np.random.RandomState(seed)
        built = [_record(rng, B, h, lambda b, c, j, k=k: coarse_length(k, c, j) + (b % 16 if (k, c, j) == (0, 0, 0) else 0))
                 for k, h in enumerate(headers)]
        built.append(_record(rng, B, finest, lambda b, c, j: finest_length(c, j)))
        scales, payloads = [s for s, _ in built], [p for _, p in built]
        pads = [(b, 2 * b, 65535 - b, 3) for b in range(B)]
        bodies = [container.write_file(pads[b], [s[:4] for s in scales], [p[b] for p in payloads], True) for b in range(B)]
        _CACHE[key] = (scales, payloads, pads, bodies)
    return _CACHE[key]


def _batch(coarse, B, finest=FINEST, lens=LENS):
    """The records of a batch of B files, built once per shape: file b has b % 16 filler bytes in its first coarse payload."""
    headers = COARSE[coarse] if finest == FINEST else [(1, 4, 4, 64)]
    return _batch_of((coarse, B, finest), 100 * coarse + B, B, headers, finest, lambda k, c, j: 1 + j + c, lambda c, j: lens[c][j])


def _write_bodies(scales, pads, bodies, stride):
    """The slots, all FILL, with the bodies written by l3c_container_write_banded -> (files (B, stride), file_bytes, padding tensor)."""
    B = len(bodies)
    arr = ops._banded_scale_array(scales)
    files = torch.full((B, stride), FILL, dtype=torch.uint8, device='cuda')
    n_ws = _lib.load().l3c_container_write_banded_workspace_bytes(arr, len(arr), B)
    ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
    padding = torch.from_numpy(np.asarray(pads, dtype=np.uint16).view(np.int16)).cuda()
    offsets = torch.arange(B, dtype=torch.int64, device='cuda') * stride
    ops.call('l3c_container_write_banded', arr, len(arr), B, ops.ptr(padding), ops.ptr(offsets, torch.int64), ops.ptr(files), ops.ptr(ws), n_ws,
             ops.stream())
    file_bytes = torch.tensor([len(f) for f in bodies], dtype=torch.int64, device='cuda')
    return files, file_bytes, padding


def _crcs(B, n, seed, L=64, HW=320):
    """Synthetic band CRC words and the frame words that go with them (a reader checks that the frame CRC is their combination)."""
    rng = np.random.RandomState(seed)
    bands = rng.randint(0, 1 << 32, size=(B, 3, n), dtype=np.uint64).astype(np.uint32)
    frame = np.array([container.combine_band_crcs(bands[b], L, HW) for b in range(B)], dtype=np.uint64).astype(np.uint32)
    return frame, bands


def _want(bodies, payloads, frame, bands, L, G, R, head):
    """The files container.make_seal writes: rows from container.rs_parity, the head part from container.head_from_body."""
    gen = _lib.load().l3c_bitstream_generation()
    n = bands.shape[2]
    res = []
    for b, body in enumerate(bodies):
        rows = [container.rs_parity(ch, min(G, n), R) for ch in payloads[-1][b]]
        hd = container.head_from_body(body, G, R) if head else None
        res.append(body + container.make_seal(body, gen, int(frame[b]), MODEL_ID, bands[b], L, parity=(min(G, n), rows), head=hd))
    return res


def _seal(scales, files, file_bytes, padding, frame, bands, G, R, head, parity_scale=None, workspace=None, between=None):
    """The existing kernels on the records, then l3c_seal_append_parity.  parity_scale: the finest record as the parity kernel is to see it.
    workspace: the caller's instead of a new one.  between(parity, hd): called on what the parity kernels returned, before the seal."""
    B = files.shape[0]
    C, H, W, L, groups = parity_scale or scales[-1]
    n = container.n_bands(H * W, L)
    parity = ops.band_parity_rs(B, H, W, L, groups, min(G, n), R)
    hd = None
    if head:
        hd = (ops.band_payload_crc32(B, scales[:-1]),) + tuple(ops.head_parity(B, scales[:-1], G, R))
    if between is not None:
        between(parity, hd)
    ops.seal_append_parity(files, file_bytes, torch.from_numpy(frame.view(np.int32)).cuda(), torch.from_numpy(bands.view(np.int32)).cuda(), scales, G, R,
                           parity, padding, MODEL_ID, hd, workspace)
    torch.cuda.synchronize()
    return files.cpu().numpy(), file_bytes.cpu().numpy()


def _find_head(f):
    buf = np.frombuffer(f, dtype=np.uint8)
    head = _lib.SealHead()
    rc = _lib.load().l3c_seal_find_head(buf.ctypes.data, buf.size, ctypes.byref(head))
    return rc, head.check_ok, head.n_records


def _check(got, sizes, want, bodies, stride, head, n_records):
    """Every file that fits its slot is make_seal's, everything behind it FILL; a file that does not fit is -1 and untouched behind its body."""
    for b, (w, body) in enumerate(zip(want, bodies)):
        if len(w) > stride:
            assert sizes[b] == -1, b
            assert got[b, :len(body)].tobytes() == body and (got[b, len(body):] == FILL).all(), b
            continue
        assert sizes[b] == len(w), (b, sizes[b], len(w))
        bad = np.nonzero(got[b, :len(w)] != np.frombuffer(w, dtype=np.uint8))[0]
        assert bad.size == 0, 'file {}: first differing byte {} of {} (body {}); {} differ'.format(b, bad[0], len(w), len(body), bad.size)
        assert (got[b, len(w):] == FILL).all(), b
        f = got[b, :sizes[b]].tobytes()
        back, seal = container.split_seal(f)
        assert bytes(back) == body and seal.parity is not None and (seal.head is not None) == bool(head) and not seal.head_damaged
        assert _find_head(f) == ((1, 1, n_records) if head else (0, 0, 0)), b


@pytest.mark.parametrize('coarse', [1, 2])
@pytest.mark.parametrize('head', [False, True])
@pytest.mark.parametrize('G,R', [(2, 1), (5, 1), (2, 2), (5, 4)])
def test_every_file_is_make_seal_byte_for_byte(G, R, head, coarse):
    B = 4
    scales, payloads, pads, bodies = _batch(coarse, B)
    frame, bands = _crcs(B, 5, 7 * G + R)
    want = _want(bodies, payloads, frame, bands, 64, G, R, head)
    assert want[0][len(bodies[0]):len(bodies[0]) + 4] == (b'L3CH' if head else b'L3CP' if R == 1 else b'L3CQ')
    stride = (max(len(w) for w in want) + 3) // 4 * 4 + 40
    assert {(b * stride + len(body)) % 4 for b, body in enumerate(bodies)} == {0, 1, 2, 3}       # a tail at every residue
    files, file_bytes, padding = _write_bodies(scales, pads, bodies, stride)
    got, sizes = _seal(scales, files, file_bytes, padding, frame, bands, G, R, head)
    _check(got, sizes, want, bodies, stride, head, coarse + 1)


@pytest.mark.parametrize('head', [False, True])
def test_tails_at_every_residue_mod_16(head):
    B, G, R = 16, 2, 2
    scales, payloads, pads, bodies = _batch(2, B)
    frame, bands = _crcs(B, 5, 3)
    want = _want(bodies, payloads, frame, bands, 64, G, R, head)
    stride = (max(len(w) for w in want) + 15) // 16 * 16 + 16
    assert {(b * stride + len(body)) % 16 for b, body in enumerate(bodies)} == set(range(16))
    files, file_bytes, padding = _write_bodies(scales, pads, bodies, stride)
    got, sizes = _seal(scales, files, file_bytes, padding, frame, bands, G, R, head)
    _check(got, sizes, want, bodies, stride, head, 3)


@pytest.mark.parametrize('head', [False, True])
def test_a_slot_without_room_becomes_minus_one_and_nothing_is_written(head):
    """The slot is one byte (with a head part, which asks for a multiple of 4: up to four) shorter than the longest file: that file is
    refused, a file that ends exactly with its slot is written, and so are the others."""
    B, G, R = 4, 5, 4
    scales, payloads, pads, bodies = _batch(1, B)
    frame, bands = _crcs(B, 5, 11)
    want = _want(bodies, payloads, frame, bands, 64, G, R, head)
    assert [len(f) - len(bodies[0]) for f in bodies] == [0, 1, 2, 3] and sorted(len(w) for w in want) == [len(w) for w in want]
    stride = (len(want[3]) - 1) // 4 * 4 if head else len(want[3]) - 1
    fits = [len(w) <= stride for w in want]
    assert fits == [True, True, True, False] and (head or len(want[2]) == stride)
    files, file_bytes, padding = _write_bodies(scales, pads, bodies, stride)
    got, sizes = _seal(scales, files, file_bytes, padding, frame, bands, G, R, head)
    _check(got, sizes, want, bodies, stride, head, 2)
    assert (sizes == -1).sum() == B - sum(fits)


@pytest.mark.parametrize('head', [False, True])
def test_an_overrun_group_and_a_refused_file_stay_refused(head):
    """File 1: a band marked L3C_AC_OVERRUN where the parity kernels read it (the finest record's, or with a head part a coarse record's)
    -> its group length is the marker, the file becomes -1 and its slot stays untouched behind the old end.  File 2 enters as -1 and stays
    -1.  Files 0 and 3 are written."""
    B, G, R = 4, 2, 2
    scales, payloads, pads, bodies = _batch(2, B)
    frame, bands = _crcs(B, 5, 13)
    want = _want(bodies, payloads, frame, bands, 64, G, R, head)
    stride = (max(len(w) for w in want) + 3) // 4 * 4 + 8
    files, file_bytes, padding = _write_bodies(scales, pads, bodies, stride)
    file_bytes[2] = -1

    def marked(scale, row):
        C, H, W, L, groups = scale
        out, nb = groups[0]
        nb = nb.clone()
        nb[row] = -1
        return (C, H, W, L, [(out, nb)] + list(groups[1:]))
    seen = list(scales)
    parity_scale = None
    if head:
        seen[1] = marked(scales[1], (1 * 2 + 1) * 1 + 0)               # record 1 (C = 2, n = 2): file 1, channel 1, band 0
    else:
        parity_scale = marked(scales[-1], (1 * 3 + 0) * 4 + 3)          # the finest record: file 1, channel 0, band 3
    got, sizes = _seal(seen, files, file_bytes, padding, frame, bands, G, R, head, parity_scale)
    assert list(sizes[[1, 2]]) == [-1, -1]
    for b in (1, 2):
        assert got[b, :len(bodies[b])].tobytes() == bodies[b] and (got[b, len(bodies[b]):] == FILL).all(), b
    for b in (0, 3):
        assert sizes[b] == len(want[b]) and got[b, :sizes[b]].tobytes() == want[b] and (got[b, sizes[b]:] == FILL).all(), b


@pytest.mark.parametrize('G,R,head', [(1, 1, False), (3, 2, False), (1, 4, True)])
def test_one_band_per_channel_has_no_full_band_group(G, R, head):
    """n = 1 on every record: out_full is NULL, every group has one member, G clamps to 1."""
    B = 4
    finest = (3, 8, 8, 64)
    scales, payloads, pads, bodies = _batch(1, B, finest, [[9], [0], [6]])
    assert all(len(s[4]) == 1 for s in scales)
    frame, bands = _crcs(B, 1, 17, HW=64)
    want = _want(bodies, payloads, frame, bands, 64, G, R, head)
    stride = (max(len(w) for w in want) + 3) // 4 * 4 + 12
    files, file_bytes, padding = _write_bodies(scales, pads, bodies, stride)
    got, sizes = _seal(scales, files, file_bytes, padding, frame, bands, G, R, head)
    _check(got, sizes, want, bodies, stride, head, 2)


def test_the_device_bodies_are_the_host_bodies():
    """What the comparisons above rest on: l3c_container_write_banded wrote container.write_file's bytes into the slots."""
    scales, _, pads, bodies = _batch(2, 4)
    files, file_bytes, _ = _write_bodies(scales, pads, bodies, 1024)
    got = files.cpu().numpy()
    for b, body in enumerate(bodies):
        assert got[b, :len(body)].tobytes() == body and (got[b, len(body):] == FILL).all()
