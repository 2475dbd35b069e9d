"""The banded half of the codec's C ABI (include/l3c_hip.h: l3c_encode_batch_banded, l3c_decode_plan_banded / l3c_decode_batch_banded,
l3c_ac_decode_bands, l3c_container_layout_banded), checked without a GPU: the size functions are pure host functions, every argument error is
reported before anything is enqueued (fake, well-aligned pointers stand in for device memory: they are never dereferenced on these paths),
and the banded planner -- the half of the decoder that reads untrusted bytes -- agrees with bitcoding/container.py on what a banded file
says and on what is not one."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.bitcoding import container
from l3c_pytorch_amd.helpers import config_parser

from tests.conftest import GOLDEN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000
INVALID, UNSUPPORTED = -1, -3


def _cfg(name='cr'):
    from l3c_pytorch_amd.native_net import net_config
    return net_config(config_parser.parse_builtin('ms', name))


def _err():
    return _lib.load().l3c_last_error().decode()


def _golden():
    with open(os.path.join(GOLDEN, 'hip_l3c_cal_64x96.l3c'), 'rb') as f:
        return f.read()


def _shapes(cfg, H, W, K):
    """The scale headers (C, H, W, L) of a banded file of an H x W image written with K bands, coarsest first."""
    return [(3 if s == 0 else cfg.C, H >> s, W >> s, container.band_len((H >> s) * (W >> s), K)) for s in reversed(range(cfg.num_scales + 1))]


def _synthetic(cfg, H, W, K, seed, padding=(0, 0, 0, 0), shapes=None, length=None):
    """A well-framed banded file of random payloads (the planner reads no payload byte); length(k, c, j, symbols) -> bytes of a payload."""
    rng = np.random.RandomState(seed)
    sh = shapes or _shapes(cfg, H, W, K)
    payloads = []
    for k, (C, h, w, L) in enumerate(sh):
        n = container.n_bands(h * w, L)
        syms = [min(L, h * w - j * L) for j in range(n)]
        payloads.append([[rng.randint(0, 256, length(k, c, j, syms[j]) if length else int(rng.randint(0, syms[j] + 2))).astype(np.uint8).tobytes()
                          for j in range(n)] for c in range(C)])
    return container.write_file(padding, sh, payloads, True)


def _offsets(files):
    return np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)


def _plan_bytes(cfg, files):
    offs = _offsets(files)
    data = np.frombuffer(b''.join(files) + b'\0' * 8, dtype=np.uint8)
    return _lib.load().l3c_decode_plan_banded_bytes(ctypes.byref(cfg), data.ctypes.data, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(files))


def _plan_rc(cfg, files, cap=None):
    """Raw l3c_decode_plan_banded_bytes + l3c_decode_plan_banded on host byte strings -> (status, message, blob bytes, H, W, paddings)."""
    lib = _lib.load()
    B = len(files)
    n = _plan_bytes(cfg, files)
    if n < 0 and cap is None:
        return n, _err(), b'', 0, 0, []
    n = cap if cap is not None else n
    offs = _offsets(files)
    data = np.frombuffer(b''.join(files) + b'\0' * 8, dtype=np.uint8)
    blob = np.zeros(n // 8, dtype=np.int64)
    H, W, pads = ctypes.c_int(), ctypes.c_int(), np.zeros((B, 4), dtype=np.uint16)
    rc = lib.l3c_decode_plan_banded(ctypes.byref(cfg), data.ctypes.data, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B, blob.ctypes.data, n,
                                    ctypes.byref(H), ctypes.byref(W), pads.ctypes.data)
    return rc, _err(), blob.tobytes(), H.value, W.value, [tuple(int(v) for v in p) for p in pads]


# ---- size functions --------------------------------------------------------------------------------------------------------------


def test_size_functions_are_pure_and_grow_with_the_shape():
    lib = _lib.load()
    a, b = _cfg(), _cfg()
    pa, pb = ctypes.byref(a), ctypes.byref(b)
    fs, ws = lib.l3c_encode_banded_file_stride, lib.l3c_encode_batch_banded_workspace_bytes
    for K in (1, 4, 64):
        assert fs(pa, 64, 96, K) == fs(pb, 64, 96, K) > 0 and fs(pa, 128, 96, K) > fs(pa, 64, 96, K) and fs(pa, 64, 192, K) > fs(pa, 64, 96, K)
        assert ws(pa, 2, 64, 96, K) == ws(pb, 2, 64, 96, K) > 0
        assert ws(pa, 3, 64, 96, K) > ws(pa, 2, 64, 96, K) and ws(pa, 2, 128, 96, K) > ws(pa, 2, 64, 96, K)
        assert ws(pa, 2, 64, 192, K) > ws(pa, 2, 64, 96, K)
    for H, W in ((64, 96), (136, 200), (24, 40), (512, 768)):
        for K in (1, 4, 7, 64, 1024):
            sh = _shapes(a, H, W, K)
            want = container.framing_bytes(sh, True)
            for C, h, w, L in sh:
                n = container.n_bands(h * w, L)
                want += C * ((n - 1) * lib.l3c_ac_max_bytes(L) + lib.l3c_ac_max_bytes(h * w - (n - 1) * L))
            assert want <= fs(pa, H, W, K) < want + 16 and fs(pa, H, W, K) % 16 == 0, (H, W, K)
    for K in (0, -1, 1025):
        assert fs(pa, 64, 96, K) == INVALID and 'bands' in _err()
        assert ws(pa, 1, 64, 96, K) == INVALID and 'bands' in _err()
    # the decode plan and workspace: functions of the files / of the plan alone
    f1, f3 = _synthetic(a, 64, 96, 4, 1), _synthetic(a, 136, 200, 4, 2)
    assert _plan_bytes(a, [f1]) == _plan_bytes(b, [f1]) > 0 and _plan_bytes(a, [f1, f1]) > _plan_bytes(a, [f1])
    assert _plan_bytes(a, [_synthetic(a, 64, 96, 64, 1)]) > _plan_bytes(a, [f1])
    dw = lib.l3c_decode_batch_banded_workspace_bytes
    blobs = []
    for files in ([f1], [f1, f1], [f3]):
        rc, msg, blob, _, _, _ = _plan_rc(a, files)
        assert rc == 0, msg
        blobs.append(np.frombuffer(blob, dtype=np.int64))
    assert dw(pa, blobs[0].ctypes.data) == dw(pb, blobs[0].ctypes.data) > 0
    assert dw(pa, blobs[1].ctypes.data) > dw(pa, blobs[0].ctypes.data) and dw(pa, blobs[2].ctypes.data) > dw(pa, blobs[0].ctypes.data)
    # outside the scope: a negative status, and the message names it
    wide = _cfg()
    wide.Cf = 128
    for fn, args in ((fs, (64, 96, 4)), (ws, (1, 64, 96, 4))):
        assert fn(ctypes.byref(wide), *args) == UNSUPPORTED and 'Cf' in _err()
        assert fn(ctypes.byref(_cfg('cr_rgb')), *args) == UNSUPPORTED and 'RGB' in _err()
        assert fn(ctypes.byref(_cfg('cr_rgb_shared')), *args) == UNSUPPORTED and 'RGB' in _err()
    assert _plan_bytes(_cfg('cr_rgb_shared'), [f1]) == UNSUPPORTED and 'RGB' in _err()
    assert dw(ctypes.byref(wide), blobs[0].ctypes.data) == UNSUPPORTED
    assert fs(pa, 60, 96, 4) < 0 and 'multiples of 2^num_scales' in _err()
    assert ws(pa, 1, 64, 100, 4) < 0 and 'multiples of 2^num_scales' in _err()
    assert ws(pa, 0, 64, 96, 4) < 0 and ws(pa, 65536, 64, 96, 4) < 0
    assert ws(pa, 64, 512, 768, 1024) == UNSUPPORTED and 'slice the batch' in _err()      # 64 images x 1024 bands


# ---- argument checks -------------------------------------------------------------------------------------------------------------


def _model(cfg):
    lib = _lib.load()
    return _lib.CodecModel(ctypes.pointer(cfg), FAKE, max(lib.l3c_net_packed_bytes(ctypes.byref(cfg)), 0), FAKE, FAKE, FAKE, -1.0, 0.08)


def _encode_desc(model, B=1, H=64, W=96, K=4):
    lib = _lib.load()
    cfg = model.cfg_host
    d = _lib.EncodeBatchDesc()
    d.model_host = ctypes.pointer(model)
    d.img, d.B, d.H, d.W, d.padding = FAKE, B, H, W, None
    d.files, d.file_bytes, d.workspace = FAKE, FAKE, FAKE
    d.file_stride = max(lib.l3c_encode_banded_file_stride(cfg, H, W, K), 0)
    d.workspace_bytes = max(lib.l3c_encode_batch_banded_workspace_bytes(cfg, B, H, W, K), 0)
    return d


def test_encode_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    enc = lambda d, K=4: lib.l3c_encode_batch_banded(ctypes.byref(d), K, None)   # noqa: E731
    cfg = _cfg()
    model = _model(cfg)
    assert lib.l3c_encode_batch_banded(None, 4, None) == INVALID and 'null descriptor' in _err()
    d = _encode_desc(model)
    d.model_host = None
    assert enc(d) == INVALID and 'null pointer' in _err()
    for field in ('img', 'files', 'file_bytes', 'workspace'):
        d = _encode_desc(model)
        setattr(d, field, None)
        assert enc(d) == INVALID and 'null pointer' in _err(), field
        d = _encode_desc(model)
        setattr(d, field, FAKE + 4)
        assert enc(d) == INVALID and '16-byte aligned' in _err(), field
    d = _encode_desc(model)
    d.padding = FAKE + 2
    assert enc(d) == INVALID and '16-byte aligned' in _err()
    for field in ('packed', 'targets_rgb', 'targets_z', 'uniform_row'):
        m = _model(cfg)
        setattr(m, field, None)
        assert enc(_encode_desc(m)) == INVALID and 'null pointer' in _err(), field
        m = _model(cfg)
        setattr(m, field, FAKE + 8)
        assert enc(_encode_desc(m)) == INVALID and '16-byte aligned' in _err(), field
    for K in (1, 4, 64):
        d = _encode_desc(model, K=K)
        d.workspace_bytes -= 1
        assert enc(d, K) == INVALID and 'workspace_bytes too small' in _err()
        d = _encode_desc(model, K=K)
        d.file_stride -= 16
        assert enc(d, K) == INVALID and 'file_stride' in _err()
    d = _encode_desc(model)
    d.file_stride += 8
    assert enc(d) == INVALID and 'file_stride' in _err()
    d = _encode_desc(model, K=1)                       # the slot and workspace of K = 1 do not hold K = 64
    assert enc(d, 64) == INVALID
    for K in (0, -3, 1025):
        assert enc(_encode_desc(model), K) == INVALID and 'bands' in _err()
    m = _model(cfg)
    m.packed_bytes = lib.l3c_net_packed_bytes(ctypes.byref(_cfg('cr_rgb_shared')))       # packed for another config
    assert enc(_encode_desc(m)) == INVALID and 'packed_bytes' in _err()
    assert enc(_encode_desc(model, H=60)) == UNSUPPORTED and 'multiples of 2^num_scales' in _err()
    assert enc(_encode_desc(model, B=0)) == INVALID and 'batch size' in _err()
    assert enc(_encode_desc(model, B=65536)) == INVALID and 'batch size' in _err()
    assert enc(_encode_desc(model, H=4096, W=2048)) == UNSUPPORTED and 'H * W * Cf * 4' in _err()
    assert enc(_encode_desc(_model(_cfg('cr_rgb')))) == UNSUPPORTED and 'RGB' in _err()


def _decode_desc(model, blob, fn='l3c_decode_batch_banded_workspace_bytes'):
    lib = _lib.load()
    d = _lib.DecodeBatchDesc()
    d.model_host = ctypes.pointer(model)
    d.files, d.plan, d.pixels, d.sym, d.workspace = FAKE, FAKE, FAKE, None, FAKE
    d.plan_host = blob.ctypes.data
    d.plan_bytes = blob.nbytes
    d.workspace_bytes = max(getattr(lib, fn)(model.cfg_host, blob.ctypes.data), 0)
    return d


def _legacy_blob(cfg, files):
    lib = _lib.load()
    n = lib.l3c_decode_plan_bytes(ctypes.byref(cfg), len(files))
    offs = _offsets(files)
    data = np.frombuffer(b''.join(files) + b'\0' * 8, dtype=np.uint8)
    blob = np.zeros(n // 8, dtype=np.int64)
    assert lib.l3c_decode_plan(ctypes.byref(cfg), data.ctypes.data, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(files), blob.ctypes.data,
                               n, None, None, None) == 0, _err()
    return blob


def test_decode_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    dec = lambda d, side=None: lib.l3c_decode_batch_banded(ctypes.byref(d), None, side)   # noqa: E731
    cfg = _cfg()
    model = _model(cfg)
    f = _synthetic(cfg, 64, 96, 4, 5)
    rc, msg, raw, _, _, _ = _plan_rc(cfg, [f])
    assert rc == 0, msg
    from l3c_pytorch_amd.native_codec import parse_plan_banded
    assert parse_plan_banded(raw)['lag'] == 1
    blob = np.frombuffer(raw, dtype=np.int64).copy()
    assert lib.l3c_decode_batch_banded(None, None, None) == INVALID and 'null descriptor' in _err()
    d = _decode_desc(model, blob)
    d.model_host = None
    assert dec(d) == INVALID and 'null pointer' in _err()
    for field in ('files', 'plan', 'plan_host', 'pixels', 'workspace'):
        d = _decode_desc(model, blob)
        setattr(d, field, None)
        assert dec(d) == INVALID and 'null pointer' in _err(), field
    for field in ('files', 'plan', 'pixels', 'sym', 'workspace'):
        d = _decode_desc(model, blob)
        setattr(d, field, FAKE + 4)
        assert dec(d) == INVALID and '16-byte aligned' in _err(), field
    d = _decode_desc(model, blob)
    d.workspace_bytes -= 1
    assert dec(d) == INVALID and 'workspace_bytes too small' in _err()
    d = _decode_desc(model, blob)
    d.plan_bytes = blob.nbytes - 8
    assert dec(d) == INVALID and 'plan_bytes too small' in _err()
    d = _decode_desc(model, blob)
    d.plan_bytes = 64
    assert dec(d) == INVALID and 'plan_bytes too small' in _err()
    bad = blob.copy()
    bad[0] ^= 1
    assert dec(_decode_desc(model, bad)) == INVALID and 'magic' in _err()
    assert lib.l3c_decode_batch_banded_workspace_bytes(ctypes.byref(cfg), bad.ctypes.data) == INVALID and 'magic' in _err()
    # a legacy blob handed to the banded decoder, and the reverse
    legacy = _legacy_blob(cfg, [_golden()])
    assert dec(_decode_desc(model, legacy, 'l3c_decode_batch_workspace_bytes')) == INVALID and 'magic' in _err() and 'l3c_decode_batch' in _err()
    assert lib.l3c_decode_batch_banded_workspace_bytes(ctypes.byref(cfg), legacy.ctypes.data) == INVALID and 'magic' in _err()
    assert lib.l3c_decode_batch(ctypes.byref(_decode_desc(model, blob)), None, None) == INVALID and 'magic' in _err()
    assert lib.l3c_decode_batch_workspace_bytes(ctypes.byref(cfg), blob.ctypes.data) == INVALID and 'magic' in _err()
    for word, value in ((2, 65536), (2, 0), (2, 2), (3, 3), (6, 7), (9, 64), (10, 3), (11, 2), (21, 8), (24, 16), (25, 0)):
        bad = blob.copy()                      # B, n_records, n_streams, the RGB band length / chunk count / lag, two offsets
        assert bad[word] != value
        bad[word] = value
        assert dec(_decode_desc(model, bad), FAKE) == INVALID and 'plan blob' in _err(), word
    other = _cfg()
    other.dec_blocks += 1                                                 # a plan made for another config
    assert dec(_decode_desc(_model(other), blob)) == INVALID and 'another config' in _err()
    m = _model(cfg)
    m.packed_bytes += 256
    assert dec(_decode_desc(m, blob)) == INVALID and 'packed_bytes' in _err()
    m = _model(cfg)
    m.uniform_row = None
    assert dec(_decode_desc(m, blob)) == INVALID and 'null pointer' in _err()
    # 16 bands per channel decode on two streams: the side stream must be one, and not the main stream
    rc, msg, raw16, _, _, _ = _plan_rc(cfg, [_synthetic(cfg, 64, 96, 64, 6)])
    assert rc == 0, msg
    assert parse_plan_banded(raw16)['lag'] == 2
    blob16 = np.frombuffer(raw16, dtype=np.int64).copy()
    assert dec(_decode_desc(model, blob16), None) == INVALID and 'side_stream' in _err()
    assert lib.l3c_decode_batch_banded(ctypes.byref(_decode_desc(model, blob16)), FAKE, FAKE) == INVALID and 'side_stream' in _err()
    assert dec(_decode_desc(_model(_cfg('cr_rgb_shared')), blob)) == UNSUPPORTED and 'RGB' in _err()


def test_kernel_entry_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    db = lambda row=FAKE, Lp=26, inp=FAKE, offs=FAKE, nb=FAKE, planes=3, n_sym=100, L=64, out=FAKE: lib.l3c_ac_decode_bands(   # noqa: E731
        row, Lp, inp, offs, nb, planes, n_sym, L, 1, out, None)
    for name in ('row', 'inp', 'offs', 'nb', 'out'):
        assert db(**{name: None}) == INVALID and 'null pointer' in _err(), name
    assert db(Lp=1) == INVALID and 'Lp out of range' in _err()
    assert db(Lp=258) == INVALID and 'Lp out of range' in _err()
    for L in (0, -64, 32, 65, 96):
        assert db(L=L) == INVALID and 'multiple of 64' in _err(), L
    assert db(planes=0) == INVALID and db(n_sym=0) == INVALID
    assert db(planes=1 << 21, n_sym=1 << 16, L=64) == INVALID and '2^31' in _err()      # 2^21 planes x 1024 bands
    assert db(inp=FAKE + 2) == INVALID and '4-byte aligned' in _err()
    sc = (_lib.BandedScale * 2)(_lib.BandedScale(None, FAKE, 0, None, FAKE, 0, 5, 8, 12, 64), _lib.BandedScale(None, None, 0, None, FAKE, 0, 3, 8, 8, 64))
    lay = lambda scales, n, B, stride, off=FAKE, size=FAKE: lib.l3c_container_layout_banded(scales, n, B, stride, off, size, None)   # noqa: E731
    assert lay(None, 2, 3, 256) == INVALID and 'null pointer' in _err()
    assert lay(sc, 2, 3, 256, off=None) == INVALID and 'null pointer' in _err()
    assert lay(sc, 2, 3, 256, size=None) == INVALID and 'null pointer' in _err()
    assert lay(sc, 2, 3, 256, off=FAKE + 8) == INVALID and '16-byte aligned' in _err()
    assert lay(sc, 2, 3, 256, size=FAKE + 8) == INVALID and '16-byte aligned' in _err()
    assert lay(sc, 0, 3, 256) == INVALID and 'scales' in _err()
    assert lay(sc, 9, 3, 256) == INVALID and 'scales' in _err()
    assert lay(sc, 2, 0, 256) == INVALID and 'batch size' in _err()
    assert lay(sc, 2, 65536, 256) == INVALID and 'batch size' in _err()
    assert lay(sc, 2, 3, 0) == INVALID and 'file_stride' in _err()
    assert lay(sc, 2, 3, 264) == INVALID and 'file_stride' in _err()
    one = lambda *a: (_lib.BandedScale * 1)(_lib.BandedScale(*a))   # noqa: E731
    assert lay(one(None, None, 0, None, FAKE, 0, 5, 8, 12, 64), 1, 3, 256) == INVALID and 'scale descriptor' in _err()      # 2 bands, no full-band lengths
    assert lay(one(None, FAKE, 0, None, None, 0, 5, 8, 12, 64), 1, 3, 256) == INVALID and 'scale descriptor' in _err()
    assert lay(one(None, FAKE, 0, None, FAKE + 2, 0, 5, 8, 12, 64), 1, 3, 256) == INVALID and '4-byte aligned' in _err()
    assert lay(one(None, FAKE, 0, None, FAKE, 0, 5, 8, 12, 96), 1, 3, 256) == INVALID and 'multiple of 64' in _err()
    assert lay(one(None, FAKE, 0, None, FAKE, 0, 5, 512, 512, 64), 1, 3, 256) == INVALID and '1024 bands' in _err()
    assert lay(one(None, FAKE, 0, None, FAKE, 0, 5, 70000, 8, 64), 1, 3, 256) == INVALID and 'u16' in _err()


# ---- the planner against container.py ----------------------------------------------------------------------------------------------


def _assert_plan_equals_parse_batch(cfg, files):
    from l3c_pytorch_amd.native_codec import PLAN_BANDED_MAGIC, parse_plan_banded
    rc, msg, raw, H, W, pads = _plan_rc(cfg, files)
    assert rc == 0, msg
    plan = parse_plan_banded(raw)
    records, framing, banded = container.parse_batch(files)
    B = len(files)
    assert banded and plan['magic'] == PLAN_BANDED_MAGIC and plan['B'] == B and plan['bytes'] == len(raw)
    assert (H, W) == tuple(records[-1][1:3]) == (plan['H'], plan['W'])
    assert pads == [tuple(p) for p in framing.padding]
    assert [r[:4] for r in plan['records']] == [tuple(r) for r in records]
    file_base = _offsets(files)[:B]
    first = 0
    for k, (C, h, w, L) in enumerate(records):
        n = container.n_bands(h * w, L)
        _, _, _, _, n_plan, at, count, mx = plan['records'][k]
        assert (n_plan, at, count) == (n, first, B * C * n)
        off = (framing.offset[k] + file_base[:, None]).reshape(B, C, n)        # positions inside the concatenated files
        nb = framing.nbytes[k].reshape(B, C, n)
        if k:                                  # every record but the coarsest: channel-major, stream (c B + b) n + j
            off, nb = off.transpose(1, 0, 2), nb.transpose(1, 0, 2)
        assert np.array_equal(plan['src_offset'][at:at + count], off.reshape(-1)), k
        assert np.array_equal(plan['nbytes'][at:at + count].astype(np.int64), nb.reshape(-1)), k
        assert mx == int(nb.max())
        entries = plan['entries'][k]
        if 0 < k < len(records) - 1:           # a bottleneck record: the ragged decoders' entry table
            pixbase, hw, pix0, npix = container.band_entry_table(B, h * w, L)
            for got, want in zip(entries, (pixbase, hw, pix0, npix, (pixbase + pix0) * ((cfg.L + 1) * 2))):
                assert got.dtype == np.int64 and np.array_equal(got, want), k
        else:
            assert entries is None
        first += count
    assert first == plan['n_streams']
    dst, nb = plan['dst_offset'], plan['nbytes'].astype(np.int64)
    assert (dst % 4 == 0).all()
    slots = (nb + 3) // 4 * 4 + 4
    assert np.array_equal(dst, np.cumsum(slots) - slots)       # back to back in stream order: no two slots overlap
    assert plan['dst_bytes'] == int(slots.sum()) and plan['files_bytes'] == sum(len(f) for f in files)
    C, h, w, L = records[-1]
    n = container.n_bands(h * w, L)
    assert plan['rgb_band_len'] == L
    assert plan['rgb_chunks'] == max(1, min(8, (h * w - (n - 1) * L) // 64))       # Bitcoding.RGB_BAND_CHUNKS' rule
    assert plan['lag'] == (2 if B * n >= 16 else 1)                                 # Bitcoding._rgb_schedule
    return plan, records


@pytest.mark.parametrize('H,W,K', [(64, 96, 1), (64, 96, 4), (64, 96, 7), (64, 96, 64), (136, 200, 4), (136, 200, 64)])
@pytest.mark.parametrize('B', [1, 3])
def test_planner_reads_banded_files_as_container_py_does(H, W, K, B):
    cfg = _cfg()
    pads = [(1, 2, 3, 4), (0, 7, 0, 5), (65535, 0, 0, 1)]
    files = [_synthetic(cfg, H, W, K, 10 * K + b, pads[b]) for b in range(B)]
    plan, records = _assert_plan_equals_parse_batch(cfg, files)
    bands = [container.n_bands(h * w, L) for _, h, w, L in records]
    if K == 1:
        assert bands == [1, 1, 1, 1] and plan['lag'] == 1
    if (H, W, K) == (64, 96, 4):
        assert records[1][3] == 128 and bands[1] == 3 and 16 * 24 - 2 * 128 == 128          # a last band equal to L
        assert plan['lag'] == 1 and bands[3] == 4                                           # B n = 4 or 12: lag 1
    if (H, W, K) == (136, 200, 4):
        assert records[0][1:] == (17, 25, 128) and 425 - 3 * 128 == 41                      # a last band below 64 and odd
    if K == 64:
        assert plan['lag'] == 2
    if (H, W, K) == (64, 96, 7):
        assert plan['lag'] == (2 if B == 3 else 1) and bands[3] == 7                        # B n = 7 and 21: either side of 16


def test_planner_takes_the_coarsest_bound_and_empty_payloads():
    cfg = _cfg()
    at_bound = lambda k, c, j, s: 2 * 128 + 64 if (k, c, j) == (0, 2, 3) else 0   # noqa: E731  (136x200, K = 4: L = 128, the 41-symbol last band)
    _assert_plan_equals_parse_batch(cfg, [_synthetic(cfg, 136, 200, 4, 3, length=at_bound)])
    over = lambda k, c, j, s: 2 * 128 + 65 if (k, c, j) == (0, 2, 3) else 0   # noqa: E731
    f = _synthetic(cfg, 136, 200, 4, 3, length=over)
    container.parse_batch([f])
    rc, msg, _, _, _, _ = _plan_rc(cfg, [f])
    assert rc == INVALID and 'invalid file' in msg and 'coarsest' in msg


def _rejected(cfg, files, what, python_too=True):
    rc, msg, _, _, _, _ = _plan_rc(cfg, files)
    assert rc == INVALID and 'invalid file' in msg, (what, rc, msg)
    rc, msg, _, _, _, _ = _plan_rc(cfg, files, cap=1 << 20)      # the planner itself, whatever the size function said
    assert rc == INVALID and 'invalid file' in msg, (what, rc, msg)
    if python_too:
        with pytest.raises(ValueError):                  # what the Python readers say of the same bytes
            container.parse_batch(files)


def _set(f, at, data):
    return f[:at] + data + f[at + len(data):]


def test_planner_rejects_broken_framing():
    """Everything container.parse_banded rejects, one mutated file per case."""
    cfg = _cfg()
    f = _synthetic(cfg, 64, 96, 7, 21)
    fr = container.parse_banded(f)
    assert _plan_rc(cfg, [f])[0] == 0
    _rejected(cfg, [_set(f, 4, b'\x02')], 'version 2')
    _rejected(cfg, [_set(f, 5, b'\x01')], 'reserved byte')
    _rejected(cfg, [_set(f, 14, b'\x00')], 'C = 0')
    _rejected(cfg, [_set(f, 15, b'\x00\x00')], 'empty scale: H = 0')
    _rejected(cfg, [_set(f, 17, b'\x00\x00')], 'empty scale: W = 0')
    _rejected(cfg, [_set(f, 19, struct.pack('<I', 0))], 'L = 0')
    _rejected(cfg, [_set(f, 19, struct.pack('<I', 96))], 'L = 96')
    _rejected(cfg, [_set(f, 19, struct.pack('<I', 63))], 'L = 63')
    _rejected(cfg, [f + b'\0'], 'one trailing byte')
    _rejected(cfg, [f[:-1]], 'one byte short')
    _rejected(cfg, [f[:14]], 'no record')
    _rejected(cfg, [f[:3]], 'three bytes')
    sep = int(fr.offset[0][-1, -1] + fr.nbytes[0][-1, -1])          # the separator behind the coarsest record
    assert f[sep:sep + 4] == container._MAGIC_VALUE_SEP
    for i in range(4):
        _rejected(cfg, [_set(f, sep + i, bytes([f[sep + i] ^ 0x10]))], 'separator byte {}'.format(i))
    for k in range(len(fr.scales)):
        for c, j in ((0, 0), (-1, -1)):
            p = int(fr.offset[k][c, j]) - 4                         # a length field of every record: its first and its last band
            _rejected(cfg, [_set(f, p, b'\xff\xff\xff\xff')], 'length field 0xFFFFFFFF in record {}'.format(k))
    p = int(fr.offset[3][-1, -1]) - 4
    n_last = int(fr.nbytes[3][-1, -1])
    _rejected(cfg, [_set(f, p, struct.pack('<I', n_last + 5))], 'the last payload runs past the end')
    # more than 1024 bands per channel: a 512 x 768 image whose RGB record says L = 64
    big = _shapes(cfg, 512, 768, 1)
    assert container.n_bands(512 * 768, 64) > 1024
    g = _synthetic(cfg, 512, 768, 1, 0, length=lambda k, c, j, s: 1)
    assert _plan_rc(cfg, [g])[0] == 0
    at = 14 + sum(9 + 5 * C + 4 for C, _, _, _ in big[:3]) + 5
    assert struct.unpack_from('<I', g, at)[0] == big[3][3]
    _rejected(cfg, [_set(g, at, struct.pack('<I', 64))], 'more than 1024 bands')
    _rejected(cfg, [f, f[:-1]], 'second file truncated')


def _records(shapes, nbytes=1):
    return container.write_file((0, 0, 0, 0), shapes, [[[b'\x55' * nbytes] * container.n_bands(h * w, L) for _ in range(C)] for C, h, w, L in shapes],
                                True)


def test_planner_rejects_what_the_model_does_not_code():
    """What Bitcoding._n_predicted, _check_coarsest and _check_header raise for: well-framed banded files of the wrong model or shape."""
    cfg = _cfg()
    sh = _shapes(cfg, 64, 96, 4)
    assert _plan_rc(cfg, [_records(sh)])[0] == 0

    def refused(f, what):
        container.parse_batch([f])                                 # the framing itself is fine
        _rejected(cfg, [f], what, python_too=False)

    refused(_records(sh[:3]), '3 records')
    refused(_records([(cfg.C, 4, 6, 64)] + sh), '5 records')
    refused(_records([(4, 8, 12, 64)] + sh[1:]), 'coarsest C = 4')
    for k in (1, 2, 3):
        C, h, w, L = sh[k]
        refused(_records(sh[:k] + [(C, h + 1, w, L)] + sh[k + 1:]), 'record {} with H + 1'.format(k))
        refused(_records(sh[:k] + [(C, h, w - 1, L)] + sh[k + 1:]), 'record {} with W - 1'.format(k))
    refused(_records(sh[:2] + [(3,) + sh[2][1:]] + sh[3:]), 'a bottleneck record with 3 channels')
    refused(_records(sh[:3] + [(cfg.C,) + sh[3][1:]]), 'an RGB record with C channels')
    # files of one batch that disagree: in a band length, in the shape
    a, b, c = _records(sh), _records(_shapes(cfg, 64, 96, 7)), _records(_shapes(cfg, 64, 104, 4))
    assert [s[3] for s in sh] != [s[3] for s in _shapes(cfg, 64, 96, 7)]
    _rejected(cfg, [a, b], 'two files of different L')
    _rejected(cfg, [b, a], 'two files of different L')
    _rejected(cfg, [a, c], 'two files of different shape')
    for files in ([a, a], [b, b], [c, c]):
        assert _plan_rc(cfg, files)[0] == 0
    # sizes outside what the network schedule supports (8192 x 8192: H * W * Cf * 4 above 32-bit addressing inside one image)
    refused(_records(_shapes(cfg, 8192, 8192, 1024), 0), '8192 x 8192')


def test_planner_answers_unsupported_for_what_is_outside_its_scope():
    cfg = _cfg()
    f = _synthetic(cfg, 64, 96, 4, 30)
    for files, word in (([_golden()], 'l3c_decode_plan'), ([_golden(), f], 'mixes'), ([f, _golden()], 'mixes')):
        for cap in (None, 1 << 20):
            rc, msg, _, _, _, _ = _plan_rc(cfg, files, cap)
            assert rc == UNSUPPORTED and 'unsupported' in msg and word in msg, (rc, msg)
    # B * n > 65535 from header bytes alone: 64 files that end behind their first record header (256 x 256 symbols in bands of 64: 1024
    # bands); the size function and the planner answer before they would need a length field
    head = b'L3CB' + struct.pack('<BB4H', 1, 0, 0, 0, 0, 0) + struct.pack('<BHHI', cfg.C, 256, 256, 64)
    assert len(head) == 23
    for cap in (None, 1 << 20):
        rc, msg, _, _, _, _ = _plan_rc(cfg, [head] * 64, cap)
        assert rc == UNSUPPORTED and 'slice the batch' in msg, (rc, msg)
        rc, msg, _, _, _, _ = _plan_rc(cfg, [head] * 63, cap)
        assert rc == INVALID and 'invalid file' in msg and 'truncated' in msg, (rc, msg)      # 64 512 streams are fine; the file is not
    from l3c_pytorch_amd.native_codec import decode_plan_banded
    with pytest.raises(_lib.L3CError, match='l3c_decode_plan'):
        decode_plan_banded(cfg, [_golden()])
    with pytest.raises(_lib.L3CError, match='mixes'):
        decode_plan_banded(cfg, [f, _golden()])
    with pytest.raises(ValueError, match='invalid file'):
        decode_plan_banded(cfg, [f[:-1]])
    blob, H, W, pads = decode_plan_banded(cfg, [f, f])
    assert (H, W, pads) == (64, 96, [(0, 0, 0, 0)] * 2) and struct.unpack('<q', blob[:8])[0] == int.from_bytes(b'L3CBPLAN', 'little')


def test_planner_survives_truncations_and_mutations_under_the_sanitizers(tmp_path):
    """tests/cabi/plan_banded_check_main.cpp: the planner header alone, built with the address and undefined-behaviour sanitizers and run as
    a child process on one synthetic 64x96 K = 7 file."""
    exe, path = tmp_path / 'plan_banded_check', tmp_path / 'k7.l3c'
    subprocess.run(['c++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'plan_banded_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    f = _synthetic(_cfg(), 64, 96, 7, 40, (3, 0, 1, 0))
    path.write_bytes(f)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 3 and lines[0].startswith('plan_banded_check: {} bytes, 64 x 96'.format(len(f))), r.stdout
    assert lines[1] == 'plan_banded_check: {} truncations refused'.format(len(f))
    assert lines[2].startswith('plan_banded_check: 10000 mutations:')
