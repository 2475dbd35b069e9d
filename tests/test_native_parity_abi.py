"""The parity-sealed encode of the C ABI (include/l3c_hip.h: l3c_encode_batch_banded_parity, its two size functions and
l3c_seal_append_parity), checked without a GPU: the size functions against a restatement of the formulas the header states, the file stride
against worst-case files built with container.make_seal, every refusal before anything touches a device (fake, well-aligned pointers stand in
for device memory: they are never dereferenced on these paths), NativeCodec's argument rules, and csrc/seal_parity_plan.h as a program of its
own under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.bitcoding import container
from l3c_pytorch_amd.helpers import config_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000
INVALID, UNSUPPORTED = -1, -3
SHAPES = [(88, 320, 16), (64, 64, 1), (512, 768, 64)]
OPTS = [(4, 1, 0), (4, 2, 0), (3, 4, 1), (64, 1, 1)]


def _cfg(name='cr'):
    from l3c_pytorch_amd.native_net import net_config
    return net_config(config_parser.parse_builtin('ms', name))


def _err():
    return _lib.load().l3c_last_error().decode()


def _opts(G, R, head, reserved=0, model_id=7):
    return _lib.ParityOpts(G, R, head, reserved, model_id)


def _records(cfg, H, W, K):
    """Per record of a banded file of an H x W image written with K bands, coarsest first: (C, h, w, L, n, P), P the longest payload the
    coder can write for one of its bands."""
    ac = _lib.load().l3c_ac_max_bytes
    res = []
    for s in reversed(range(cfg.num_scales + 1)):
        h, w = H >> s, W >> s
        L = container.band_len(h * w, K)
        n = container.n_bands(h * w, L)
        res.append((3 if s == 0 else cfg.C, h, w, L, n, max(ac(L), ac(h * w - (n - 1) * L))))
    return res


def _groups(n, G):
    return -(-n // min(G, n))


def _tail(recs, G, R, head):
    """TAIL of include/l3c_hip.h, l3c_encode_banded_parity_file_stride."""
    C0, _, _, _, n0, P0 = recs[-1]
    m0 = _groups(n0, G)
    tail = (8 if R == 1 and not head else 12) + 12 * m0 + 3 * m0 * R * P0 + 8 + (20 + 12 * n0) + 24
    if head:
        meta = 4 + 14 + sum(9 + 4 * C * n for C, _, _, _, n, _ in recs) + 4 + sum(4 * C * n + 4 + 4 * C * _groups(n, G) for C, _, _, _, n, _ in recs[:-1])
        tail += meta + sum(C * _groups(n, G) * R * P for C, _, _, _, n, P in recs[:-1]) + 4
    return tail


def _scale_array(recs):
    arr = (_lib.BandedScale * len(recs))()
    for k, (C, h, w, L, _, _) in enumerate(recs):
        arr[k] = _lib.BandedScale(None, None, 0, None, None, 0, C, h, w, L)
    return arr


def _up(n, to=256):
    return -(-n // to) * to


@pytest.mark.parametrize('H,W,K', SHAPES)
def test_size_functions_are_the_formulas_the_header_states(H, W, K):
    lib = _lib.load()
    cfg = _cfg()
    ref = ctypes.byref(cfg)
    recs = _records(cfg, H, W, K)
    _, _, _, L0, n0, P0 = recs[-1]
    for G, R, head in OPTS:
        o = ctypes.byref(_opts(G, R, head))
        stride = lib.l3c_encode_banded_parity_file_stride(ref, H, W, K, o)
        assert stride == lib.l3c_encode_banded_file_stride(ref, H, W, K) + _up(_tail(recs, G, R, head), 32), (G, R, head, _err())
        for B in (1, 3):
            m0 = _groups(n0, G)
            seal_ws = lib.l3c_seal_append_parity_workspace_bytes(_scale_array(recs), len(recs), B, G, R, head)
            assert seal_ws > 0, _err()
            extra = [4 * B, 12 * B * n0, lib.l3c_u8_crc32_bands_workspace_bytes(B, 3, H * W, L0), 3 * B * m0 * R * _up(P0, 16), 12 * B * m0, seal_ws]
            if head:
                Sh = _up(max(P for _, _, _, _, _, P in recs[:-1]), 16)
                groups = sum(B * C * _groups(n, G) for C, _, _, _, n, _ in recs[:-1])
                extra += [groups * R * Sh, 4 * groups, 4 * sum(B * C * n for C, _, _, _, n, _ in recs[:-1])]
            want = lib.l3c_encode_batch_banded_workspace_bytes(ref, B, H, W, K) + sum(_up(v) for v in extra)
            assert lib.l3c_encode_batch_banded_parity_workspace_bytes(ref, B, H, W, K, o) == want, (G, R, head, B, _err())
        # pure functions of their arguments; the model id does not count
        assert lib.l3c_encode_banded_parity_file_stride(ctypes.byref(_cfg()), H, W, K, ctypes.byref(_opts(G, R, head, model_id=1 << 63))) == stride


def test_the_workspace_of_the_tail_assembler_is_its_three_parts():
    lib = _lib.load()
    recs = _records(_cfg(), 88, 320, 16)
    for G, R, head in OPTS:
        for B in (1, 5):
            units = 3 * _groups(recs[-1][4], G)
            meta = 0
            if head:
                units += 1 + sum(C * _groups(n, G) for C, _, _, _, n, _ in recs[:-1])
                meta = 4 + 14 + sum(9 + 4 * C * n for C, _, _, _, n, _ in recs) + 4 + sum(4 * C * n + 4 + 4 * C * _groups(n, G) for C, _, _, _, n, _ in recs[:-1])
                meta = _up(meta, 16) + 16
            want = _up(8 * B, 16) + _up(8 * B * units, 16) + B * meta
            assert lib.l3c_seal_append_parity_workspace_bytes(_scale_array(recs), len(recs), B, G, R, head) == want, (G, R, head, B, _err())


@pytest.mark.parametrize('G,R,head', OPTS)
def test_the_stride_holds_a_file_whose_every_payload_is_as_long_as_the_coder_can_make_it(G, R, head):
    """make_seal on a body of zero payloads of l3c_ac_max_bytes each, rows of the same length: nothing the coder writes is longer."""
    lib = _lib.load()
    cfg = _cfg()
    for H, W, K in ((88, 320, 16), (64, 64, 1)):
        ac = lib.l3c_ac_max_bytes
        recs = _records(cfg, H, W, K)
        payloads = [[[bytes(ac(min(L, h * w - j * L))) for j in range(n)] for _ in range(C)] for C, h, w, L, n, _ in recs]
        body = container.write_file((1, 2, 3, 4), [r[:4] for r in recs], payloads, True)
        assert len(body) <= lib.l3c_encode_banded_file_stride(ctypes.byref(cfg), H, W, K)

        def rows(channel, n):
            m = _groups(n, G)
            return [[bytes(max(len(p) for p in channel[g::m]))] * R for g in range(m)]
        n0, L0 = recs[-1][4], recs[-1][3]
        parity = [rows(ch, n0) for ch in payloads[-1]]
        hd = None
        if head:
            hd = [(np.zeros((C, n), dtype=np.uint32), [rows(ch, n) for ch in chans]) for (C, _, _, _, n, _), chans in zip(recs[:-1], payloads[:-1])]
        tail = container.make_seal(body, 3, 0x12345678, 7, np.zeros((3, n0), dtype=np.uint32), L0, parity=(min(G, n0), parity if R > 1 or head else
                                   [[q[0] for q in row] for row in parity]), head=hd)
        assert tail[:4] == (b'L3CH' if head else b'L3CP' if R == 1 else b'L3CQ')
        assert len(tail) == _tail(recs, G, R, head)                        # the bound is this file's tail exactly
        stride = lib.l3c_encode_banded_parity_file_stride(ctypes.byref(cfg), H, W, K, ctypes.byref(_opts(G, R, head)))
        assert len(body) + len(tail) <= stride and stride % 16 == 0


# ---- refusals, all before anything touches a device ------------------------------------------------------------------------------------


def _model(cfg):
    lib = _lib.load()
    return _lib.CodecModel(ctypes.pointer(cfg), FAKE, max(lib.l3c_net_packed_bytes(ctypes.byref(cfg)), 0), FAKE, FAKE, FAKE, -1.0, 0.08)


def _encode_desc(model, opts, B=1, H=88, W=320, K=16):
    lib = _lib.load()
    cfg = model.cfg_host
    d = _lib.EncodeBatchDesc()
    d.model_host = ctypes.pointer(model)
    d.img, d.B, d.H, d.W, d.padding = FAKE, B, H, W, None
    d.files, d.file_bytes, d.workspace = FAKE, FAKE, FAKE
    d.file_stride = max(lib.l3c_encode_banded_parity_file_stride(cfg, H, W, K, ctypes.byref(opts)), 16)
    d.workspace_bytes = max(lib.l3c_encode_batch_banded_parity_workspace_bytes(cfg, B, H, W, K, ctypes.byref(opts)), 0)
    return d


def test_the_encode_entry_refuses_before_any_launch():
    lib = _lib.load()
    cfg = _cfg()
    ref = ctypes.byref(cfg)
    model = _model(cfg)
    enc = lambda d, o, K=16: lib.l3c_encode_batch_banded_parity(ctypes.byref(d), K, ctypes.byref(o), None)   # noqa: E731
    good = _opts(4, 2, 1)
    assert lib.l3c_encode_batch_banded_parity(None, 16, ctypes.byref(good), None) == INVALID and 'null descriptor' in _err()
    assert lib.l3c_encode_batch_banded_parity(ctypes.byref(_encode_desc(model, good)), 16, None, None) == INVALID and 'opts_host' in _err()
    assert lib.l3c_encode_banded_parity_file_stride(ref, 88, 320, 16, None) == INVALID and 'opts_host' in _err()
    assert lib.l3c_encode_batch_banded_parity_workspace_bytes(ref, 1, 88, 320, 16, None) == INVALID and 'opts_host' in _err()
    for bad, word in ((_opts(4, 0, 0), 'R must be in 1..4'), (_opts(4, 5, 0), 'R must be in 1..4'), (_opts(0, 1, 0), 'G must be'),
                      (_opts(-2, 1, 0), 'G must be'), (_opts(4, 1, 2), 'head must be'), (_opts(4, 1, 0, reserved=1), 'reserved')):
        assert lib.l3c_encode_banded_parity_file_stride(ref, 88, 320, 16, ctypes.byref(bad)) == INVALID and word in _err(), word
        assert lib.l3c_encode_batch_banded_parity_workspace_bytes(ref, 1, 88, 320, 16, ctypes.byref(bad)) == INVALID and word in _err(), word
        assert enc(_encode_desc(model, good), bad) == INVALID and word in _err(), word
    # G > 255 with R > 1: 1024 bands per channel in groups of 256 (G clamps to n first: 300 on 16 bands is 16)
    wide = _opts(256, 2, 0)
    assert lib.l3c_encode_banded_parity_file_stride(ref, 512, 768, 1024, ctypes.byref(wide)) == INVALID and '255' in _err()
    assert lib.l3c_encode_batch_banded_parity_workspace_bytes(ref, 1, 512, 768, 1024, ctypes.byref(wide)) == INVALID and '255' in _err()
    d = _encode_desc(model, _opts(256, 1, 0), H=512, W=768, K=1024)
    assert enc(d, wide, 1024) == INVALID and '255' in _err()
    assert lib.l3c_encode_banded_parity_file_stride(ref, 512, 768, 1024, ctypes.byref(_opts(256, 1, 0))) > 0
    assert lib.l3c_encode_banded_parity_file_stride(ref, 88, 320, 16, ctypes.byref(_opts(300, 2, 1))) > 0
    # what l3c_encode_batch_banded refuses is refused here alike
    for field in ('img', 'files', 'file_bytes', 'workspace'):
        d = _encode_desc(model, good)
        setattr(d, field, None)
        assert enc(d, good) == INVALID and 'null pointer' in _err(), field
        d = _encode_desc(model, good)
        setattr(d, field, FAKE + 4)
        assert enc(d, good) == INVALID and '16-byte aligned' in _err(), field
    for K in (0, 1025):
        assert enc(_encode_desc(model, good), good, K) == INVALID and 'bands' in _err()
        assert lib.l3c_encode_banded_parity_file_stride(ref, 88, 320, K, ctypes.byref(good)) == INVALID and 'bands' in _err()
    assert enc(_encode_desc(model, good, H=84), good) == UNSUPPORTED and 'multiples of 2^num_scales' in _err()
    assert lib.l3c_encode_batch_banded_parity_workspace_bytes(ref, 0, 88, 320, 16, ctypes.byref(good)) == INVALID and 'batch size' in _err()
    assert lib.l3c_encode_batch_banded_parity_workspace_bytes(ref, 65536, 88, 320, 16, ctypes.byref(good)) == INVALID and 'batch size' in _err()
    assert lib.l3c_encode_banded_parity_file_stride(ctypes.byref(_cfg('cr_rgb')), 88, 320, 16, ctypes.byref(good)) == UNSUPPORTED and 'RGB' in _err()
    # a slot or a workspace that holds the band-sealed encode but not the parity
    for o in (good, _opts(4, 1, 0)):
        d = _encode_desc(model, o)
        d.file_stride -= 16
        assert enc(d, o) == INVALID and 'file_stride' in _err() and 'l3c_encode_banded_parity_file_stride' in _err()
        d = _encode_desc(model, o)
        d.file_stride = lib.l3c_encode_banded_file_stride(ref, 88, 320, 16) + _up(lib.l3c_seal_bands_bytes(16), 32)
        assert enc(d, o) == INVALID and 'file_stride' in _err()
        d = _encode_desc(model, o)
        d.workspace_bytes -= 1
        assert enc(d, o) == INVALID and 'workspace_bytes too small' in _err()
        d = _encode_desc(model, o)
        d.workspace_bytes = lib.l3c_encode_batch_banded_workspace_bytes(ref, 1, 88, 320, 16)
        assert enc(d, o) == INVALID and 'workspace_bytes too small' in _err()
    d = _encode_desc(model, _opts(4, 1, 0))                    # the slot and workspace of R = 1 do not hold R = 2 with a head part
    assert enc(d, good) == INVALID
    # the 65535 limits: 1024 bands a channel in groups of 1 are 3072 groups a file; the coarser records of such a file hold 5 (768 + 384 + 96)
    one = _opts(1, 1, 0)
    ws = lib.l3c_encode_batch_banded_parity_workspace_bytes
    assert cfg.C == 5 and [r[4] for r in _records(cfg, 512, 768, 1024)] == [96, 384, 768, 1024]
    assert ws(ref, 21, 512, 768, 1024, ctypes.byref(one)) > 0
    assert ws(ref, 22, 512, 768, 1024, ctypes.byref(one)) == UNSUPPORTED and 'slice the batch' in _err() and 'B * 3 * m' in _err()
    d = _encode_desc(model, one, B=21, H=512, W=768, K=1024)
    d.B = 22
    d.workspace_bytes = d.file_stride = 1 << 40
    assert enc(d, one, 1024) == UNSUPPORTED and 'slice the batch' in _err()
    headed = _opts(1, 1, 1)
    assert ws(ref, 10, 512, 768, 1024, ctypes.byref(headed)) > 0
    assert ws(ref, 11, 512, 768, 1024, ctypes.byref(headed)) == UNSUPPORTED and 'slice the batch' in _err() and 'head' in _err()
    d.B = 11
    assert enc(d, headed, 1024) == UNSUPPORTED and 'slice the batch' in _err()


def _seal_desc(recs, B=2, G=4, R=2, head=1):
    lib = _lib.load()
    d = _lib.SealParityDesc()
    arr = (_lib.BandedScale * len(recs))()
    for k, (C, h, w, L, n, P) in enumerate(recs):
        arr[k] = _lib.BandedScale(FAKE if n > 1 else None, FAKE if n > 1 else None, _up(P, 4), FAKE, FAKE, _up(P, 4), C, h, w, L)
    d.files, d.file_stride, d.file_bytes, d.B = FAKE, 1 << 20, FAKE, B
    d.scales_host, d.n_scales = arr, len(recs)
    d.G, d.R, d.head, d.reserved = G, R, head, 0
    d.padding, d.model_id, d.frame_crc, d.band_crc = None, 9, FAKE, FAKE
    d.parity, d.parity_stride, d.parity_nbytes = FAKE, _up(recs[-1][5], 16), FAKE
    d.head_parity, d.head_parity_stride, d.head_parity_nbytes, d.payload_crc = FAKE, _up(max(r[5] for r in recs), 16), FAKE, FAKE
    d.head_parity_offset_host = (ctypes.c_int64 * len(recs))(*[4096 * k for k in range(len(recs))])
    d.workspace = FAKE
    d.workspace_bytes = max(lib.l3c_seal_append_parity_workspace_bytes(arr, len(recs), B, G, R, head), 0)
    d._keep = arr
    return d


def test_the_tail_assembler_refuses_before_any_launch():
    lib = _lib.load()
    recs = _records(_cfg(), 88, 320, 16)
    call = lambda d: lib.l3c_seal_append_parity(ctypes.byref(d), None)   # noqa: E731
    assert lib.l3c_seal_append_parity(None, None) == INVALID and 'null descriptor' in _err()
    for field, value, word in (('R', 0, 'R must be'), ('R', 5, 'R must be'), ('G', 0, 'G must be'), ('head', 3, 'head must be'), ('reserved', 2, 'reserved'),
                               ('scales_host', None, 'null pointer'), ('n_scales', 0, 'n_scales'), ('B', 0, 'batch size'), ('B', 65536, 'batch size'),
                               ('files', None, 'null pointer'), ('file_bytes', None, 'null pointer'), ('frame_crc', None, 'null pointer'),
                               ('band_crc', None, 'null pointer'), ('parity', None, 'null pointer'), ('parity_nbytes', None, 'null pointer'),
                               ('workspace', None, 'null pointer'), ('head_parity', None, 'head part'), ('head_parity_nbytes', None, 'head part'),
                               ('payload_crc', None, 'head part'), ('head_parity_offset_host', None, 'head part'), ('file_stride', 0, 'file_stride'),
                               ('file_stride', 1002, 'multiples of 4'), ('files', FAKE + 2, 'multiples of 4'), ('file_bytes', FAKE + 4, 'element size'),
                               ('frame_crc', FAKE + 2, 'element size'), ('padding', FAKE + 1, 'element size'), ('parity', FAKE + 8, '16-byte aligned'),
                               ('head_parity', FAKE + 4, '16-byte aligned'), ('workspace', FAKE + 8, '16-byte aligned'),
                               ('parity_stride', 1000, 'multiple of 16'), ('parity_stride', 0, 'multiple of 16'), ('head_parity_stride', 24, 'multiple of 16')):
        d = _seal_desc(recs)
        setattr(d, field, value)
        assert call(d) == INVALID and word in _err(), (field, value, _err())
    d = _seal_desc(recs)
    d.workspace_bytes -= 1
    assert call(d) == INVALID and 'workspace too small' in _err()
    d = _seal_desc(recs)
    d.head_parity_offset_host = (ctypes.c_int64 * 4)(0, 8, 0, 0)
    assert call(d) == INVALID and 'offsets' in _err()
    d = _seal_desc(recs)
    d.n_scales = 9
    assert call(d) == UNSUPPORTED and '8 scale records' in _err()
    d = _seal_desc(recs[-1:], head=1)
    assert call(d) == INVALID and 'head' in _err()
    d = _seal_desc(recs[:-1])                                   # the last record is the finest: 3 channels
    assert call(d) == INVALID and '3 channels' in _err()
    big = _records(_cfg(), 512, 768, 1024)
    d = _seal_desc(big, B=22, G=1, R=1, head=0)
    d.workspace_bytes = 1 << 40
    assert call(d) == UNSUPPORTED and 'slice the batch' in _err()
    d = _seal_desc(big, B=11, G=1, R=1, head=1)
    d.workspace_bytes = 1 << 40
    assert call(d) == UNSUPPORTED and 'slice the batch' in _err()
    d = _seal_desc(big, B=1, G=256, R=2, head=0)
    assert call(d) == INVALID and '255' in _err()
    ws = lib.l3c_seal_append_parity_workspace_bytes
    assert ws(None, 4, 1, 4, 1, 0) == INVALID and ws(_seal_desc(recs)._keep, 4, 1, 4, 5, 0) == INVALID and ws(_seal_desc(big)._keep, 4, 22, 1, 1, 0) == UNSUPPORTED


def test_native_codec_takes_the_argument_rules_of_bitcoding():
    """Every rule is checked before the blueprint or a device is touched: None stands in for the blueprint."""
    from l3c_pytorch_amd.native_codec import NativeCodec
    for kw, word in ((dict(parity=4), "seal='bands'"), (dict(parity=4, seal=True, bands=16), "seal='bands'"), (dict(parity=4, seal='bands'), 'banded files'),
                     (dict(parity=-1, seal='bands', bands=16), 'parity must be'), (dict(parity=True, seal='bands', bands=16), 'parity must be'),
                     (dict(parity=2.0, seal='bands', bands=16), 'parity must be'), (dict(parity=4, parity_streams=0, seal='bands', bands=16), 'parity_streams must be'),
                     (dict(parity=4, parity_streams=5, seal='bands', bands=16), 'parity_streams must be'),
                     (dict(parity=4, parity_streams=True, seal='bands', bands=16), 'parity_streams must be'),
                     (dict(parity_streams=2, seal='bands', bands=16), 'needs parity=G'), (dict(parity_head=True, seal='bands', bands=16), 'needs parity=G'),
                     (dict(parity=4, parity_head=1, seal='bands', bands=16), 'parity_head must be'),
                     (dict(parity=300, parity_streams=2, seal='bands', bands=1024), 'at most 255')):
        with pytest.raises(ValueError, match=word):
            NativeCodec(None, **kw)


def test_the_plan_header_survives_the_sanitizers(tmp_path):
    """tests/cabi/seal_parity_plan_check_main.cpp: csrc/seal_parity_plan.h alone, built with the address and undefined-behaviour sanitizers
    and run as a child process."""
    exe = tmp_path / 'seal_parity_plan_check'
    subprocess.run(['c++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'seal_parity_plan_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith('seal_parity_plan_check: ') and lines[0].endswith(' plans checked'), r.stdout
    assert int(lines[0].split()[1]) > 3000 and lines[1] == 'seal_parity_plan_check: refusals checked'
