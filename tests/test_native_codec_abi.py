"""The codec entry points of the C ABI (include/l3c_hip.h: l3c_encode_batch, l3c_decode_plan / l3c_decode_batch, l3c_container_layout),
checked without a GPU: the size functions are pure host functions, every argument error is reported before anything is enqueued (fake,
well-aligned pointers stand in for device memory: they are never dereferenced on these paths), and the planner -- the half of the decoder
that reads untrusted bytes -- agrees with bitcoding/container.py on what a file says and on what is not a file."""
import ctypes
import os
import struct

import numpy as np
import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.bitcoding import container
from l3c_pytorch_amd.helpers import config_parser

from tests.conftest import GOLDEN  # noqa: E402

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


def _plan_rc(cfg, files):
    """Raw l3c_decode_plan on host byte strings -> (status, message, blob bytes, H, W, paddings)."""
    lib = _lib.load()
    B = len(files)
    n = lib.l3c_decode_plan_bytes(ctypes.byref(cfg), B)
    assert n > 0, _err()
    offs = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    data = np.frombuffer(b''.join(files) + b'\0' * 8, dtype=np.uint8)
    blob = np.zeros(n // 8, dtype=np.int64)
    H, W, pads = ctypes.c_int(), ctypes.c_int(), np.zeros((B, 4), dtype=np.uint16)
    rc = lib.l3c_decode_plan(ctypes.byref(cfg), data.ctypes.data, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B, blob.ctypes.data, n,
                             ctypes.byref(H), ctypes.byref(W), pads.ctypes.data)
    return rc, _err(), blob.tobytes(), H.value, W.value, [tuple(int(v) for v in p) for p in pads]


def _shapes(cfg, H, W):
    S = cfg.num_scales
    return [(3 if s == 0 else cfg.C, H >> s, W >> s) for s in reversed(range(S + 1))]


def _synthetic(cfg, H, W, seed, coarsest_lengths=None, padding=(0, 0, 0, 0)):
    """A well-framed file of random payloads (the planner reads no payload byte)."""
    rng = np.random.RandomState(seed)
    scales = _shapes(cfg, H, W)
    payloads = []
    for k, (C, h, w) in enumerate(scales):
        lens = coarsest_lengths if (k == 0 and coarsest_lengths is not None) else [int(rng.randint(0, h * w + 2)) for _ in range(C)]
        payloads.append([rng.randint(0, 256, n).astype(np.uint8).tobytes() for n in lens])
    return container.write_file(padding, scales, payloads, False)


# ---- size functions --------------------------------------------------------------------------------------------------------------


def test_size_functions_are_pure_and_grow_with_the_shape():
    lib = _lib.load()
    a, b = _cfg(), _cfg()
    pa, pb = ctypes.byref(a), ctypes.byref(b)
    fs, ws, pl = lib.l3c_encode_file_stride, lib.l3c_encode_batch_workspace_bytes, lib.l3c_decode_plan_bytes
    assert fs(pa, 64, 96) == fs(pb, 64, 96) > 0 and fs(pa, 128, 96) > fs(pa, 64, 96) and fs(pa, 64, 192) > fs(pa, 64, 96)
    assert ws(pa, 2, 64, 96) == ws(pb, 2, 64, 96) > 0
    assert ws(pa, 3, 64, 96) > ws(pa, 2, 64, 96) and ws(pa, 2, 128, 96) > ws(pa, 2, 64, 96) and ws(pa, 2, 64, 192) > ws(pa, 2, 64, 96)
    assert pl(pa, 2) == pl(pb, 2) > 0 and pl(pa, 3) > pl(pa, 2)
    for H, W in ((64, 96), (136, 200), (512, 768)):
        want = 8 + sum(5 + 4 * C + 4 + C * lib.l3c_ac_max_bytes(h * w) for C, h, w in _shapes(a, H, W))
        assert fs(pa, H, W) == (want + 15) // 16 * 16
    # the decode workspace: a function of the plan alone
    rc, msg, blob, H, W, _ = _plan_rc(a, [_golden()])
    assert rc == 0, msg
    buf = np.frombuffer(blob, dtype=np.int64)
    dw = lib.l3c_decode_batch_workspace_bytes
    assert dw(pa, buf.ctypes.data) == dw(pb, buf.ctypes.data) > 0
    rc, msg, blob2, _, _, _ = _plan_rc(a, [_golden(), _golden()])
    assert dw(pa, np.frombuffer(blob2, dtype=np.int64).ctypes.data) > dw(pa, buf.ctypes.data)
    rc, msg, blob3, _, _, _ = _plan_rc(a, [_synthetic(a, 136, 200, 1)])
    assert rc == 0 and dw(pa, np.frombuffer(blob3, dtype=np.int64).ctypes.data) > dw(pa, buf.ctypes.data)
    # outside the scope: a negative status, and the message names it
    wide = _cfg()
    wide.Cf = 128
    for fn, args in ((fs, (64, 96)), (ws, (1, 64, 96)), (pl, (1,))):
        assert fn(ctypes.byref(wide), *args) == UNSUPPORTED and 'Cf' in _err()
        assert fn(ctypes.byref(_cfg('cr_rgb')), *args) == UNSUPPORTED and 'RGB' in _err()
        assert fn(ctypes.byref(_cfg('cr_rgb_shared')), *args) == UNSUPPORTED and 'RGB' in _err()
    assert dw(ctypes.byref(wide), buf.ctypes.data) == UNSUPPORTED
    assert fs(pa, 60, 96) < 0 and 'multiples of 2^num_scales' in _err()
    assert ws(pa, 1, 64, 100) < 0 and 'multiples of 2^num_scales' in _err()
    assert ws(pa, 0, 64, 96) < 0 and ws(pa, 65536, 64, 96) < 0 and pl(pa, 0) < 0 and pl(pa, 65536) < 0


# ---- argument checks -------------------------------------------------------------------------------------------------------------


def _model(cfg):
    lib = _lib.load()
    return _lib.CodecModel(ctypes.pointer(cfg), FAKE, max(lib.l3c_net_packed_bytes(ctypes.byref(cfg)), 0), FAKE, FAKE, FAKE, -1.0, 0.08)


def _encode_desc(model, B=1, H=64, W=96):
    lib = _lib.load()
    cfg = model.cfg_host
    d = _lib.EncodeBatchDesc()
    d.model_host = ctypes.pointer(model)
    d.img, d.B, d.H, d.W, d.padding = FAKE, B, H, W, None
    d.files, d.file_bytes, d.workspace = FAKE, FAKE, FAKE
    d.file_stride = max(lib.l3c_encode_file_stride(cfg, H, W), 0)
    d.workspace_bytes = max(lib.l3c_encode_batch_workspace_bytes(cfg, B, H, W), 0)
    return d


def test_encode_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    enc = lambda d: lib.l3c_encode_batch(ctypes.byref(d), None)   # noqa: E731
    cfg = _cfg()
    model = _model(cfg)
    assert lib.l3c_encode_batch(None, None) == INVALID and 'null descriptor' in _err()
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
    m = _model(cfg)
    m.cfg_host = None
    d = _encode_desc(model)
    d.model_host = ctypes.pointer(m)
    assert enc(d) == INVALID and 'null config' in _err()
    d = _encode_desc(model)
    d.workspace_bytes -= 1
    assert enc(d) == INVALID and 'workspace_bytes too small' in _err()
    d = _encode_desc(model)
    d.file_stride -= 16
    assert enc(d) == INVALID and 'file_stride' in _err()
    d = _encode_desc(model)
    d.file_stride += 8
    assert enc(d) == INVALID and 'file_stride' in _err()
    m = _model(cfg)
    m.packed_bytes = lib.l3c_net_packed_bytes(ctypes.byref(_cfg('cr_rgb_shared')))       # packed for another config
    assert enc(_encode_desc(m)) == INVALID and 'packed_bytes' in _err()
    assert enc(_encode_desc(model, H=60)) == UNSUPPORTED and 'multiples of 2^num_scales' in _err()
    assert enc(_encode_desc(model, W=100)) == UNSUPPORTED and 'multiples of 2^num_scales' in _err()
    assert enc(_encode_desc(model, B=0)) == INVALID and 'batch size' in _err()
    assert enc(_encode_desc(model, B=65536)) == INVALID and 'batch size' in _err()
    assert enc(_encode_desc(model, H=4096, W=2048)) == UNSUPPORTED and 'H * W * Cf * 4' in _err()
    rgb = _cfg('cr_rgb')
    assert enc(_encode_desc(_model(rgb))) == UNSUPPORTED and 'RGB' in _err()
    wide = _cfg()
    wide.Cf = 128
    assert enc(_encode_desc(_model(wide))) == UNSUPPORTED and 'Cf' in _err()


def _decode_desc(model, blob):
    lib = _lib.load()
    d = _lib.DecodeBatchDesc()
    d.model_host = ctypes.pointer(model)
    d.files, d.plan, d.pixels, d.sym, d.workspace = FAKE, FAKE, FAKE, None, FAKE
    d.plan_host = blob.ctypes.data
    d.plan_bytes = blob.nbytes
    d.workspace_bytes = max(lib.l3c_decode_batch_workspace_bytes(model.cfg_host, blob.ctypes.data), 0)
    return d


def test_decode_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    dec = lambda d, side=None: lib.l3c_decode_batch(ctypes.byref(d), None, side)   # noqa: E731
    cfg = _cfg()
    model = _model(cfg)
    rc, msg, raw, _, _, _ = _plan_rc(cfg, [_golden()])
    assert rc == 0, msg
    blob = np.frombuffer(raw, dtype=np.int64).copy()
    assert lib.l3c_decode_batch(None, None, None) == INVALID and 'null descriptor' in _err()
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
    assert lib.l3c_decode_batch_workspace_bytes(ctypes.byref(cfg), bad.ctypes.data) == INVALID and 'magic' in _err()
    bad = blob.copy()
    bad[2] = 65536                                                        # B
    assert dec(_decode_desc(model, bad)) == INVALID and 'plan blob' in _err()
    bad[2] = 0
    assert dec(_decode_desc(model, bad)) == INVALID and 'plan blob' in _err()
    other = _cfg()
    other.dec_blocks += 1                                                 # a plan made for another config
    assert dec(_decode_desc(_model(other), blob)) == INVALID and 'another config' in _err()
    m = _model(cfg)
    m.packed_bytes += 256
    assert dec(_decode_desc(m, blob)) == INVALID and 'packed_bytes' in _err()
    m = _model(cfg)
    m.uniform_row = None
    assert dec(_decode_desc(m, blob)) == INVALID and 'null pointer' in _err()
    # 16 images decode on two streams: the side stream must be one, and not the main stream
    rc, msg, raw16, _, _, _ = _plan_rc(cfg, [_golden()] * 16)
    assert rc == 0, msg
    blob16 = np.frombuffer(raw16, dtype=np.int64).copy()
    from l3c_pytorch_amd.native_codec import parse_plan
    assert parse_plan(raw16)['lag'] == 2 and parse_plan(raw)['lag'] == 1
    assert dec(_decode_desc(model, blob16), None) == INVALID and 'side_stream' in _err()
    assert lib.l3c_decode_batch(ctypes.byref(_decode_desc(model, blob16)), FAKE, FAKE) == INVALID and 'side_stream' in _err()
    assert dec(_decode_desc(_model(_cfg('cr_rgb_shared')), blob)) == UNSUPPORTED and 'RGB' in _err()


def test_container_layout_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    sc = (_lib.ContainerScale * 2)(_lib.ContainerScale(None, FAKE, 0, 5, 8, 8), _lib.ContainerScale(None, FAKE, 0, 3, 16, 16))
    lay = lambda scales, n, B, stride, off=FAKE, size=FAKE: lib.l3c_container_layout(scales, n, B, stride, off, size, None)   # noqa: E731
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
    bad = (_lib.ContainerScale * 1)(_lib.ContainerScale(None, None, 0, 5, 8, 8))
    assert lay(bad, 1, 3, 256) == INVALID and 'scale descriptor' in _err()
    bad = (_lib.ContainerScale * 1)(_lib.ContainerScale(None, FAKE + 2, 0, 5, 8, 8))
    assert lay(bad, 1, 3, 256) == INVALID and '4-byte aligned' in _err()
    assert lib.l3c_sym_to_u8(None, 16, FAKE, None) == INVALID and 'null pointer' in _err()
    assert lib.l3c_sym_to_u8(FAKE, 0, FAKE, None) == INVALID and 'empty' in _err()
    assert lib.l3c_sym_to_u8(FAKE + 2, 16, FAKE, None) == INVALID and '16-byte aligned' in _err()


# ---- the planner against container.py ----------------------------------------------------------------------------------------------


def _policy(HW):
    """The RGB chunk list as the feature's issue states it (Bitcoding._decode_rgb_pipelined's default)."""
    n = max(1, min(32, HW // 4096))
    step = 64 * -(-(-(-HW // n)) // 64)
    if HW >= 16384:
        return [(0, 1024), (1024, 1024)] + [(p0, min(step, HW - p0)) for p0 in range(2048, HW, step)]
    return [(p0, min(step, HW - p0)) for p0 in range(0, HW, step)]


def _assert_plan_equals_parse_batch(cfg, files):
    from l3c_pytorch_amd.native_codec import PLAN_MAGIC, parse_plan
    rc, msg, raw, H, W, pads = _plan_rc(cfg, files)
    assert rc == 0, msg
    plan = parse_plan(raw)
    records, framing, banded = container.parse_batch(files)
    B = len(files)
    assert not banded and plan['magic'] == PLAN_MAGIC and plan['B'] == B and plan['bytes'] == len(raw)
    assert (H, W) == tuple(records[-1][1:3]) == (plan['H'], plan['W'])
    assert pads == [tuple(p) for p in framing.padding]
    assert [r[:3] for r in plan['records']] == [tuple(r) for r in records]
    file_base = np.concatenate([[0], np.cumsum([len(f) for f in files])])[:B]
    first = 0
    for k, (C, h, w) in enumerate(records):
        _, _, _, at, n, mx = plan['records'][k]
        assert (at, n) == (first, B * C)
        off = framing.offset[k] + file_base[:, None]           # (B, C): positions inside the concatenated files
        nb = framing.nbytes[k]
        if k:                                                  # every record but the coarsest: channel-major, stream c * B + b
            off, nb = off.T, nb.T
        assert np.array_equal(plan['src_offset'][at:at + n], off.reshape(-1)), k
        assert np.array_equal(plan['nbytes'][at:at + n].astype(np.int64), nb.reshape(-1)), k
        assert mx == int(nb.max())
        first += n
    assert first == plan['n_streams']
    dst, nb = plan['dst_offset'], plan['nbytes'].astype(np.int64)
    assert (dst % 4 == 0).all()
    slots = (nb + 3) // 4 * 4 + 4
    assert np.array_equal(dst, np.cumsum(slots) - slots)       # back to back in stream order: no two slots overlap
    assert plan['dst_bytes'] == int(slots.sum()) and plan['files_bytes'] == sum(len(f) for f in files)
    HW = H * W
    chunks = plan['chunks']
    assert chunks == _policy(HW)
    assert chunks[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and sum(chunks[-1]) == HW
    assert all(p0 % 64 == 0 for p0, _ in chunks) and plan['max_chunk_npix'] == max(n for _, n in chunks)
    assert plan['lag'] == (2 if B >= 16 else 1)
    return plan


def test_planner_reads_the_golden_file_as_container_py_does():
    plan = _assert_plan_equals_parse_batch(_cfg(), [_golden()])
    assert (plan['H'], plan['W']) == (64, 96) and len(plan['chunks']) == 1


def test_planner_reads_a_batch_as_container_py_does():
    cfg = _cfg()
    hw = 17 * 25
    files = [_synthetic(cfg, 136, 200, 11, [0, 5, hw, 2 * hw + 64, 1], (1, 2, 3, 4)),
             _synthetic(cfg, 136, 200, 12, None, (0, 7, 0, 5)),
             _synthetic(cfg, 136, 200, 13, [3, 0, 0, 9, 2 * hw + 64], (65535, 0, 0, 1))]
    plan = _assert_plan_equals_parse_batch(cfg, files)
    assert len(plan['chunks']) == 8 and plan['chunks'][-1][1] < plan['chunks'][-2][1]      # two probes, six chunks, a shorter last one
    _assert_plan_equals_parse_batch(cfg, [files[0]] * 16)


@pytest.mark.parametrize('H,W', [(64, 96), (128, 128), (136, 200), (512, 768)])
def test_planner_chunk_list_is_the_python_policy(H, W):
    cfg = _cfg()
    f = container.write_file((0, 0, 0, 0), _shapes(cfg, H, W), [[b''] * C for C, _, _ in _shapes(cfg, H, W)], False)
    plan = _assert_plan_equals_parse_batch(cfg, [f])
    assert plan['H'] * plan['W'] in (6144, 16384, 27200, 393216)


def _rejected(cfg, files, what):
    rc, msg, _, _, _, _ = _plan_rc(cfg, files)
    assert rc == INVALID and 'invalid file' in msg, (what, rc, msg)
    with pytest.raises(ValueError):                      # what the Python readers say of the same bytes
        container.parse_batch(files)


def test_planner_rejects_every_truncation_of_the_golden_file():
    cfg, g = _cfg(), _golden()
    for n in range(len(g)):
        rc, msg, _, _, _, _ = _plan_rc(cfg, [g[:n]])
        assert rc == INVALID and 'invalid file' in msg, (n, rc, msg)
    for n in (0, 7, 8, 12, 13, 17, len(g) // 2, len(g) - 4, len(g) - 1):
        with pytest.raises(ValueError):
            container.parse_batch([g[:n]])
    _rejected(cfg, [g, g[:-1]], 'second file truncated')


def test_planner_rejects_broken_framing():
    cfg, g = _cfg(), _golden()
    fr = container.parse_containers([g])
    _rejected(cfg, [g + b'\0'], 'one trailing byte')
    _rejected(cfg, [g[:8] + b'\0' + g[9:]], 'C = 0')
    sep = int(fr.offset[0][0, -1] + fr.nbytes[0][0, -1])          # the separator behind the coarsest record
    assert g[sep:sep + 4] == container._MAGIC_VALUE_SEP
    for i in range(4):
        _rejected(cfg, [g[:sep + i] + bytes([g[sep + i] ^ 0x10]) + g[sep + i + 1:]], 'separator byte {}'.format(i))
    for k in range(len(fr.scales)):
        p = int(fr.offset[k][0, 0]) - 4                            # a length field of every record
        _rejected(cfg, [g[:p] + b'\xff\xff\xff\xff' + g[p + 4:]], 'length field 0xFFFFFFFF in record {}'.format(k))


def _records(cfg, shapes, lengths=None):
    return container.write_file((0, 0, 0, 0), shapes, [[b'\x55' * (lengths[k][c] if lengths else 1) for c in range(C)]
                                                       for k, (C, _, _) in enumerate(shapes)], False)


def test_planner_rejects_what_the_model_does_not_code():
    """What Bitcoding._n_predicted, _check_coarsest and _check_header raise for: well-framed files of the wrong model or shape."""
    cfg = _cfg()
    sh = _shapes(cfg, 64, 96)
    rc, msg, _, _, _, _ = _plan_rc(cfg, [_records(cfg, sh)])
    assert rc == 0, msg

    def refused(f, what):
        container.parse_batch([f])                                 # the framing itself is fine
        rc, msg, _, _, _, _ = _plan_rc(cfg, [f])
        assert rc == INVALID and 'invalid file' in msg, (what, rc, msg)

    refused(_records(cfg, sh[:3]), '3 records')
    refused(_records(cfg, [(cfg.C, 4, 6)] + sh), '5 records')
    refused(_records(cfg, [(4, 8, 12)] + sh[1:]), 'coarsest C = 4')
    refused(_records(cfg, [(cfg.C, 0, 12)] + sh[1:]), 'coarsest H = 0')
    over = [[2 * 8 * 12 + 64] * cfg.C, [1] * cfg.C, [1] * cfg.C, [1] * 3]
    rc, msg, _, _, _, _ = _plan_rc(cfg, [_records(cfg, sh, over)])
    assert rc == 0, msg                                            # exactly the bound
    over[0][2] += 1
    refused(_records(cfg, sh, over), 'coarsest payload one byte over the bound')
    for k in (1, 2, 3):
        C, h, w = sh[k]
        refused(_records(cfg, sh[:k] + [(C, h + 1, w)] + sh[k + 1:]), 'record {} with H + 1'.format(k))
        refused(_records(cfg, sh[:k] + [(C, h, w - 1)] + sh[k + 1:]), 'record {} with W - 1'.format(k))
    refused(_records(cfg, sh[:2] + [(3, sh[2][1], sh[2][2])] + sh[3:]), 'a bottleneck record with 3 channels')
    refused(_records(cfg, sh[:3] + [(cfg.C, 64, 96)]), 'an RGB record with C channels')
    # two files of different shape, and of the same shape
    a, b = _records(cfg, sh), _records(cfg, _shapes(cfg, 64, 104))
    _rejected(cfg, [a, b], 'two files of different shape')
    assert _plan_rc(cfg, [a, a])[0] == 0 and _plan_rc(cfg, [b, b])[0] == 0
    # sizes outside what the network schedule supports (8192 x 8192: H * W * Cf * 4 above 32-bit addressing inside one image)
    refused(_records(cfg, _shapes(cfg, 8192, 8192)), '8192 x 8192')


def test_planner_refuses_banded_files_as_unsupported():
    cfg = _cfg()
    sh = [(C, h, w, container.band_len(h * w, 4)) for C, h, w in _shapes(cfg, 64, 96)]
    f = container.write_file((0, 0, 0, 0), sh, [[[b'\x01'] * container.n_bands(h * w, L) for _ in range(C)] for C, h, w, L in sh], True)
    assert f[:4] == b'L3CB' and container.parse_batch([f])[2]
    for files in ([f], [_golden(), f]):
        rc, msg, _, _, _, _ = _plan_rc(cfg, files)
        assert rc == UNSUPPORTED and 'banded' in msg, (rc, msg)
    from l3c_pytorch_amd.native_codec import decode_plan
    with pytest.raises(_lib.L3CError, match='banded'):
        decode_plan(cfg, [f])
    with pytest.raises(ValueError, match='invalid file'):
        decode_plan(cfg, [_golden()[:-1]])
    assert struct.unpack('<q', decode_plan(cfg, [_golden()])[0][:8])[0] == int.from_bytes(b'L3C_PLAN', 'little')
