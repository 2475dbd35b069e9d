"""Region decode through the C ABI (include/l3c_hip.h: l3c_net_get_p_rows, l3c_decode_region_plan, l3c_decode_region), checked without a
GPU: the region planner (csrc/codec_plan_region.h) against bitcoding/region.py element for element, halo and apron against the Python rules,
every refusal with its status and message before anything is enqueued (fake, well-aligned pointers stand in for device memory: they are
never dereferenced on these paths -- this machine has no device, which proves it), and the planner header alone under the address and
undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.bitcoding import container, region
from l3c_pytorch_amd.helpers import config_parser
from l3c_pytorch_amd.native_codec import PLAN_BANDED_MAGIC, PLAN_MAGIC, REGION_MAGIC, parse_region_plan

from tests.test_gpu_region import P_CASES, boxes  # noqa: E402  (the lists only: nothing of that module runs here)
from tests.test_native_banded_abi import _cfg, _err, _model, _offsets, _synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000
INVALID, UNSUPPORTED = -1, -3
I64P = ctypes.POINTER(ctypes.c_int64)


def _legacy(cfg, H, W, seed, padding=(0, 0, 0, 0)):
    """A well-framed legacy file of random payloads."""
    rng = np.random.RandomState(seed)
    sh = [(3 if s == 0 else cfg.C, H >> s, W >> s) for s in reversed(range(cfg.num_scales + 1))]
    payloads = [[rng.randint(0, 256, int(rng.randint(0, 40))).astype(np.uint8).tobytes() for _ in range(C)] for C, _, _ in sh]
    return container.write_file(padding, sh, payloads, False)


def _plan(cfg, files):
    """The plan blob of either format -> (blob int64 array, paddings uint16 (B, 4), H, W)."""
    lib = _lib.load()
    B = len(files)
    offs = _offsets(files)
    data = np.frombuffer(b''.join(files) + b'\0' * 8, dtype=np.uint8)
    if container.is_banded(files[0]):
        n, fn = lib.l3c_decode_plan_banded_bytes(ctypes.byref(cfg), data.ctypes.data, offs.ctypes.data_as(I64P), B), lib.l3c_decode_plan_banded
    else:
        n, fn = lib.l3c_decode_plan_bytes(ctypes.byref(cfg), B), lib.l3c_decode_plan
    assert n > 0, _err()
    blob = np.zeros(n // 8, dtype=np.int64)
    H, W, pads = ctypes.c_int(), ctypes.c_int(), np.zeros((B, 4), dtype=np.uint16)
    rc = fn(ctypes.byref(cfg), data.ctypes.data, offs.ctypes.data_as(I64P), B, blob.ctypes.data, n, ctypes.byref(H), ctypes.byref(W), pads.ctypes.data)
    assert rc == 0, _err()
    return blob, pads, H.value, W.value


def _region_rc(cfg, blob, pads, box, cap=None, plan_bytes=None):
    """Raw l3c_decode_region_plan -> (status, message, region blob int64 array, l3c_region_info)."""
    lib = _lib.load()
    n = lib.l3c_decode_region_plan_bytes(ctypes.byref(cfg), blob.ctypes.data)
    if n < 0:
        return n, _err(), None, None
    n = n if cap is None else cap
    out = np.zeros(max(n, 8) // 8, dtype=np.int64)
    info = _lib.RegionInfo()
    box = tuple(box) + ((0, int(_image_size(blob, pads)[1])) if len(box) == 2 else ())
    rc = lib.l3c_decode_region_plan(ctypes.byref(cfg), blob.ctypes.data, blob.nbytes if plan_bytes is None else plan_bytes, pads.ctypes.data,
                                    ctypes.byref(_lib.RegionBox(*box)), out.ctypes.data, n, ctypes.byref(info))
    return rc, _err(), out, info


def _image_size(blob, pads):
    left, right, top, bottom = (int(v) for v in pads[0])
    return int(blob[4]) - top - bottom, int(blob[5]) - left - right       # words 4, 5 of either plan header: H, W


# ---- the planner against Python ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('padding', [(0, 0, 0, 0), (2, 3, 1, 2)])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('K', [0, 1, 16, 64])
@pytest.mark.parametrize('H,W', [(H, W) for H in (64, 320, 328, 712) for W in (88, 96)])
def test_planner_plans_what_region_py_plans(H, W, K, B, padding):
    """K = 0: legacy files.  Every box of tests/test_gpu_region.py:boxes on the unpadded image, and a one-row box at every band boundary
    of the frame; where region.parse_box refuses a box the library refuses it too."""
    cfg = _cfg()
    ms = config_parser.parse_builtin('ms', 'cr')
    files = [_synthetic(cfg, H, W, K, 10 * b + K, padding) if K else _legacy(cfg, H, W, 10 * b, padding) for b in range(B)]
    blob, pads, Hf, Wf = _plan(cfg, files)
    assert (Hf, Wf) == (H, W) and [tuple(p) for p in pads] == [padding] * B
    records, framing, banded = container.parse_batch(files)
    assert banded == bool(K)
    L = records[-1][3] if banded else H * W
    n = container.n_bands(H * W, L)
    halo, apron = region.halo_rows(ms), region.apron_rows(ms)
    left, right, top, bottom = padding
    h_img, w_img = H - top - bottom, W - left - right
    offs = _offsets(files)
    todo = list(boxes(h_img, w_img))
    for j in range(1, n):
        y = (j * L) // W - top
        if 0 <= y < h_img:
            todo.append((y, y + 1))
    planned = 0
    for box in todo:
        rc, msg, raw, info = _region_rc(cfg, blob, pads, box)
        try:
            rows, cols = region.parse_box(box, region.shared_padding(framing.padding), (H, W))
        except ValueError as e:
            assert rc == INVALID and msg == str(e), (box, rc, msg, str(e))
            continue
        assert rc == 0, (box, msg)
        planned += 1
        want = region.region_plan(H, W, L, rows, halo)
        got = parse_region_plan(raw.tobytes())
        assert got['magic'] == REGION_MAGIC and got['plan_magic'] == (PLAN_BANDED_MAGIC if banded else PLAN_MAGIC)
        assert got['bytes'] <= raw.nbytes and got['bytes'] % 16 == 0
        assert (got['B'], got['H'], got['W'], got['L'], got['n']) == (B, H, W, L, n) and got['padding'] == padding
        assert got['box'] == (rows[0] - top, rows[1] - top, cols[0] - left, cols[1] - left)
        assert (got['bands'], got['sym_rows'], got['conv_rows'], got['valid_rows']) == (want.bands, want.sym_rows, want.conv_rows, want.valid_rows)
        assert got['decoder_rows'] == region.decoder_rows(H, want.conv_rows, apron)
        j0, j1 = want.bands
        S = B * (j1 - j0)
        assert got['S'] == S
        for a, b in zip(got['entries'], region.entry_table(want, B)):
            assert a.dtype == b.dtype and np.array_equal(a, b), box
        # Python's pick of the band streams: stream (b, c n + j) of the finest record, (c, b n + j) after scale_host_channel_image_band
        pick = (np.arange(B)[:, None] * n + np.arange(j0, j1)[None, :]).reshape(-1)
        o = (framing.offset[-1] + offs[:B, None]).reshape(B, 3, n).transpose(1, 0, 2).reshape(3, B * n)[:, pick].reshape(-1)
        nb = framing.nbytes[-1].reshape(B, 3, n).transpose(1, 0, 2).reshape(3, B * n)[:, pick].reshape(-1)
        assert np.array_equal(got['src_offset'], o) and np.array_equal(got['nbytes'].astype(np.int64), nb)
        slots = (nb + 3) // 4 * 4 + 4
        assert np.array_equal(got['dst_offset'], np.cumsum(slots) - slots) and got['dst_bytes'] == int(slots.sum())
        assert got['max_nbytes'] == int(nb.max())
        length = region.entry_table(want, B)[3]
        chunks = max(1, min(8, int(length.min()) // 64)) if banded else max(1, min(32, int(length.min()) // 4096))
        assert (got['n_chunks'], got['lag']) == (chunks, 2 if S >= 16 else 1), box
        assert (got['streams_total'], got['bytes_used'], got['bytes_total']) == (3 * B * n, int(nb.sum()), int(framing.nbytes[-1].sum()))
        # l3c_region_info: the same numbers
        pair = lambda a: (int(a[0]), int(a[1]))       # noqa: E731
        assert (pair(info.bands), info.n_bands, pair(info.sym_rows), pair(info.conv_rows), pair(info.valid_rows), pair(info.decoder_rows)) == (
            want.bands, n, want.sym_rows, want.conv_rows, want.valid_rows, got['decoder_rows'])
        assert (info.frame_rows, info.n_chunks, info.lag, info.out_rows, info.out_cols) == (H, chunks, got['lag'], rows[1] - rows[0], cols[1] - cols[0])
        assert (info.streams_used, info.streams_total, info.bytes_used, info.bytes_total) == (3 * S, 3 * B * n, int(nb.sum()), got['bytes_total'])
        # the crop table: the box inside the window frames, planar in `pixels`
        bh, bw = rows[1] - rows[0], cols[1] - cols[0]
        for b, m in enumerate(got['crop']):
            assert tuple(int(v) for v in m) == (b * 3 * bh * bw, bw, bh * bw, 1, bh, bw, rows[0] - want.conv_rows[0], cols[0]), (box, b)
    assert planned >= (1 if H == 64 else len(boxes(h_img, w_img)))


def test_halo_and_apron_are_the_python_rules():
    lib = _lib.load()
    ms = config_parser.parse_builtin('ms', 'cr')

    class Ms(object):
        class dec(object):
            num_blocks = 0
    for blocks in range(1, 17):
        Ms.dec.num_blocks = blocks
        assert lib.l3c_net_halo_rows(blocks) == region.halo_rows(Ms) == 2 * (2 * blocks + 2) + 4
        assert lib.l3c_net_apron_rows(blocks) == region.apron_rows(Ms)
    assert (lib.l3c_net_halo_rows(ms.dec.num_blocks), lib.l3c_net_apron_rows(ms.dec.num_blocks)) == (40, 192)
    assert lib.l3c_net_halo_rows(-1) == INVALID and lib.l3c_net_apron_rows(65) == INVALID


# ---- refusals ----------------------------------------------------------------------------------------------------------------------


def test_region_planner_refusals():
    lib = _lib.load()
    cfg = _cfg()
    files = [_synthetic(cfg, 320, 88, 16, 3, (2, 3, 1, 2))]
    blob, pads, _, _ = _plan(cfg, files)
    for box in ((5, 5, 0, 10), (9, 4, 0, 10), (0, 318, 0, 10), (-1, 3, 0, 10), (0, 10, 0, 84), (0, 10, 5, 5), (0, 10, -1, 5),
                (-2 ** 31, 2 ** 31 - 1, 0, 10), (0, 10, -2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31, 0, 1)):
        rc, msg, _, _ = _region_rc(cfg, blob, pads, box)
        assert rc == INVALID and 'is empty or not inside the 317x83 image' in msg, (box, msg)
    # files whose padding tuples differ: the message says so, as region.shared_padding does
    two = [files[0], _synthetic(cfg, 320, 88, 16, 4, (3, 2, 2, 1))]
    blob2, pads2, _, _ = _plan(cfg, two)
    rc, msg, _, _ = _region_rc(cfg, blob2, pads2, (0, 10, 0, 10))
    with pytest.raises(ValueError) as e:
        region.shared_padding([tuple(p) for p in pads2])
    assert rc == INVALID and msg == str(e.value) and 'one padding tuple' in msg
    # a blob that fails its check
    bad = blob.copy()
    bad[0] ^= 1
    rc, msg, _, _ = _region_rc(cfg, bad, pads, (0, 10, 0, 10))
    assert rc == INVALID and 'magic' in msg
    bad = blob.copy()
    bad[2] = 2                      # B
    assert _region_rc(cfg, bad, pads, (0, 10, 0, 10))[0] == INVALID and 'plan blob' in _err()
    rc, msg, _, _ = _region_rc(cfg, blob, pads, (0, 10, 0, 10), plan_bytes=blob.nbytes - 8)
    assert rc == INVALID and 'plan_bytes too small' in msg
    other = _cfg()
    other.dec_blocks += 1
    assert _region_rc(other, blob, pads, (0, 10, 0, 10))[0] == INVALID and 'another config' in _err()
    # region_bytes too small: one byte less than this box's blob needs
    rc, msg, raw, _ = _region_rc(cfg, blob, pads, (100, 140, 0, 10))
    assert rc == 0, msg
    need = int(raw[1])
    assert _region_rc(cfg, blob, pads, (100, 140, 0, 10), cap=need)[0] == 0
    rc, msg, _, _ = _region_rc(cfg, blob, pads, (100, 140, 0, 10), cap=need - 1)
    assert rc == INVALID and 'region_bytes too small' in msg
    # null pointers
    box = _lib.RegionBox(0, 10, 0, 10)
    out = np.zeros(need // 8, dtype=np.int64)
    args = [ctypes.byref(cfg), blob.ctypes.data, blob.nbytes, pads.ctypes.data, ctypes.byref(box), out.ctypes.data, need, None]
    for i in (1, 3, 4, 5):
        a = list(args)
        a[i] = None
        assert lib.l3c_decode_region_plan(*a) == INVALID and 'null pointer' in _err(), i
    assert lib.l3c_decode_region_plan(None, *args[1:]) == INVALID
    # outside the scope
    for name in ('cr_rgb', 'cr_rgb_shared'):
        rgb = _cfg(name)
        assert lib.l3c_decode_region_plan(ctypes.byref(rgb), *args[1:]) == UNSUPPORTED and 'RGB' in _err()
        assert lib.l3c_decode_region_plan_bytes(ctypes.byref(rgb), blob.ctypes.data) == UNSUPPORTED and 'RGB' in _err()
    # (more than 65535 entries cannot be reached: both planners already refuse a batch with more band streams per channel than that)


def _rows_desc(cfg, B=1, h=160, w=44, c0=128, c1=256):
    lib = _lib.load()
    d = _lib.NetGetPRowsDesc()
    d.cfg_host = ctypes.pointer(cfg)
    d.packed, d.packed_bytes = FAKE, max(lib.l3c_net_packed_bytes(ctypes.byref(cfg)), 0)
    d.net, d.bn_q, d.B, d.h, d.w, d.fuse, d.c0, d.c1, d.P, d.workspace = 0, FAKE, B, h, w, FAKE, c0, c1, FAKE, FAKE
    d.workspace_bytes = max(lib.l3c_net_get_p_rows_workspace_bytes(ctypes.byref(cfg), B, h, w, c0, c1), 0)
    return d


def test_get_p_rows_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    cfg = _cfg()
    run = lambda d: lib.l3c_net_get_p_rows(ctypes.byref(d), None)   # noqa: E731
    ws = lib.l3c_net_get_p_rows_workspace_bytes
    assert lib.l3c_net_get_p_rows(None, None) == INVALID and 'null descriptor' in _err()
    for field in ('packed', 'bn_q', 'P', 'workspace', 'fuse'):
        d = _rows_desc(cfg)
        setattr(d, field, None)
        assert run(d) == INVALID and 'null pointer' in _err(), field
    for field in ('packed', 'bn_q', 'fuse', 'P', 'workspace'):
        d = _rows_desc(cfg)
        setattr(d, field, FAKE + 4)
        assert run(d) == INVALID and '16-byte aligned' in _err(), field
    d = _rows_desc(cfg)
    assert d.workspace_bytes > 0
    d.workspace_bytes -= 1
    assert run(d) == INVALID and 'workspace_bytes too small' in _err()
    d = _rows_desc(cfg)
    d.net = 1
    assert run(d) == INVALID and 'net must be 0' in _err()
    for c0, c1, what in ((32, 256, 'multiple of 64'), (128, 200, 'multiple of 64'), (1, 65, 'even rows'), (64, 64, 'even rows'), (0, 322, 'even rows'),
                         (-64, 64, 'even rows'), (128, 129, 'even rows')):
        d = _rows_desc(cfg)
        d.c0, d.c1 = c0, c1
        assert run(d) == INVALID and what in _err(), (c0, c1, _err())
        assert ws(ctypes.byref(cfg), 1, 160, 44, c0, c1) == INVALID and what in _err()
    d = _rows_desc(cfg)
    d.packed_bytes += 256
    assert run(d) == INVALID and 'packed_bytes' in _err()
    for name in ('cr_rgb', 'cr_rgb_shared'):
        rgb = _cfg(name)
        assert run(_rows_desc(rgb)) == UNSUPPORTED and 'RGB' in _err()
        assert ws(ctypes.byref(rgb), 1, 160, 44, 128, 256) == UNSUPPORTED
    # the frame must pass at FULL size: 2904 x 2896 leaves the Winograd kernel's 2 GB, whatever the window
    assert ws(ctypes.byref(cfg), 1, 1448, 1448, 0, 64) > 0
    assert ws(ctypes.byref(cfg), 1, 1452, 1448, 0, 64) == UNSUPPORTED and '32-bit addressing' in _err()
    d = _rows_desc(cfg, h=1452, w=1448, c0=0, c1=64)
    d.workspace_bytes = 1 << 40
    assert run(d) == UNSUPPORTED and '32-bit addressing' in _err()
    # the workspace is the window's and the apron's, not the frame's: the same window of a frame four times as tall needs no more
    assert ws(ctypes.byref(cfg), 1, 1024, 768, 1024, 1088) == ws(ctypes.byref(cfg), 1, 2048, 768, 1024, 1088) > 0
    assert ws(ctypes.byref(cfg), 1, 1024, 768, 1024, 1088) * 4 < lib.l3c_net_get_p_workspace_bytes(ctypes.byref(cfg), 1, 1024, 768)
    # the end of the frame is a legal c1, and the P_CASES of the GPU test are all legal windows
    for H, windows in P_CASES:
        for c0, c1 in windows:
            for B in (1, 2):
                assert ws(ctypes.byref(cfg), B, H // 2, 44, c0, c1) > 0, (H, c0, c1, _err())


def _region_desc(model, blob, raw, pixels=FAKE):
    lib = _lib.load()
    d = _lib.DecodeRegionDesc()
    d.model_host = ctypes.pointer(model)
    d.files, d.plan_host, d.plan, d.plan_bytes = FAKE, blob.ctypes.data, FAKE, blob.nbytes
    d.region_host, d.region, d.region_bytes = raw.ctypes.data, FAKE, int(raw[1])
    d.pixels, d.workspace = pixels, FAKE
    d.workspace_bytes = max(lib.l3c_decode_region_workspace_bytes(model.cfg_host, blob.ctypes.data, raw.ctypes.data), 0)
    return d


@pytest.mark.parametrize('K', [0, 16])
def test_decode_region_arguments_are_checked_before_any_launch(K):
    lib = _lib.load()
    dec = lambda d, side=None: lib.l3c_decode_region(ctypes.byref(d), None, side)   # noqa: E731
    cfg = _cfg()
    model = _model(cfg)
    files = [_synthetic(cfg, 320, 88, K, 7)] if K else [_legacy(cfg, 320, 88, 7)]
    blob, pads, _, _ = _plan(cfg, files)
    rc, msg, raw, info = _region_rc(cfg, blob, pads, (190, 210, 3, 50))
    assert rc == 0 and info.lag == 1, msg
    assert lib.l3c_decode_region(None, None, None) == INVALID and 'null descriptor' in _err()
    d = _region_desc(model, blob, raw)
    assert d.workspace_bytes > 0, _err()
    d.model_host = None
    assert dec(d) == INVALID and 'null pointer' in _err()
    for field in ('files', 'plan', 'plan_host', 'region', 'region_host', 'pixels', 'workspace'):
        d = _region_desc(model, blob, raw)
        setattr(d, field, None)
        assert dec(d) == INVALID and 'null pointer' in _err(), field
    for field in ('files', 'plan', 'region', 'pixels', 'workspace'):
        d = _region_desc(model, blob, raw)
        setattr(d, field, FAKE + 4)
        assert dec(d) == INVALID and '16-byte aligned' in _err(), field
    d = _region_desc(model, blob, raw)
    d.workspace_bytes -= 1
    assert dec(d) == INVALID and 'workspace_bytes too small' in _err()
    d = _region_desc(model, blob, raw)
    d.plan_bytes -= 8
    assert dec(d) == INVALID and 'plan_bytes too small' in _err()
    d = _region_desc(model, blob, raw)
    d.region_bytes -= 1
    assert dec(d) == INVALID and 'region_bytes too small' in _err()
    # a region blob is trusted only where planning its own box again gives the same blob
    words = int(raw[1]) // 8
    for word in (0, 3, 12, 13, 14, 16, 20, 26, 27, 28, 30, 43, 47, 48, words - 1, words - 6):
        bad = raw.copy()
        bad[word] ^= 4
        assert dec(_region_desc(model, blob, bad), FAKE) == INVALID and 'region blob' in _err(), word
        assert lib.l3c_decode_region_workspace_bytes(ctypes.byref(cfg), blob.ctypes.data, bad.ctypes.data) == INVALID
    # ... and only beside the plan blob it was made from
    other_files = [_synthetic(cfg, 320, 88, K, 8)] if K else [_legacy(cfg, 320, 88, 8)]
    other_blob, _, _, _ = _plan(cfg, other_files)
    if not np.array_equal(other_blob, blob):
        assert dec(_region_desc(model, other_blob, raw)) == INVALID and 'region blob' in _err()
    bad = blob.copy()
    bad[0] ^= 1
    assert dec(_region_desc(model, bad, raw)) == INVALID and 'magic' in _err()
    changed = _cfg()
    changed.dec_blocks += 1
    assert dec(_region_desc(_model(changed), blob, raw)) == INVALID and 'another config' in _err()
    m = _model(cfg)
    m.packed_bytes += 256
    assert dec(_region_desc(m, blob, raw)) == INVALID and 'packed_bytes' in _err()
    assert dec(_region_desc(_model(_cfg('cr_rgb_shared')), blob, raw)) == UNSUPPORTED and 'RGB' in _err()
    # lag 2 (16 entries or more) without a side stream of its own
    if K:
        files64 = [_synthetic(cfg, 320, 88, 64, 9)]
        blob64, pads64, _, _ = _plan(cfg, files64)
        rc, msg, raw64, info = _region_rc(cfg, blob64, pads64, (0, 320, 0, 88))
        assert rc == 0 and info.lag == 2 and info.bands[1] - info.bands[0] >= 16, msg
        assert dec(_region_desc(model, blob64, raw64), None) == INVALID and 'side_stream' in _err()
        assert lib.l3c_decode_region(ctypes.byref(_region_desc(model, blob64, raw64)), FAKE, FAKE) == INVALID and 'side_stream' in _err()


def test_region_workspace_is_sized_by_the_window():
    """2048 x 3072, K = 64: a 64-row box needs a fraction of the whole-frame decode's workspace; all rows need about as much."""
    lib = _lib.load()
    cfg = _cfg()
    blob, pads, _, _ = _plan(cfg, [_synthetic(cfg, 2048, 3072, 64, 11)])
    whole = lib.l3c_decode_batch_banded_workspace_bytes(ctypes.byref(cfg), blob.ctypes.data)
    sizes = []
    for box in ((1000, 1064, 0, 3072), (900, 1156, 0, 3072), (0, 2048, 0, 3072)):
        rc, msg, raw, info = _region_rc(cfg, blob, pads, box)
        assert rc == 0, msg
        sizes.append(lib.l3c_decode_region_workspace_bytes(ctypes.byref(cfg), blob.ctypes.data, raw.ctypes.data))
        assert sizes[-1] > 0, _err()
    print('workspace bytes: 64 rows {}, 256 rows {}, all rows {}; l3c_decode_batch_banded {}'.format(sizes[0], sizes[1], sizes[2], whole))
    assert sizes[0] < sizes[1] < sizes[2] and sizes[0] * 2 < whole, (sizes, whole)


# ---- the planner header alone, under the sanitizers ----------------------------------------------------------------------------------


def test_region_planner_survives_every_box_and_broken_blobs_under_the_sanitizers(tmp_path):
    """tests/cabi/region_plan_check_main.cpp: the planner headers alone, built with the address and undefined-behaviour sanitizers and run
    as a child process -- every (y0, y1) of a 328-row and a 712-row frame at K = 1, 16, 64, truncated and bit-flipped plan blobs, boxes of
    extreme values, bit-flipped region blobs."""
    exe = tmp_path / 'region_plan_check'
    subprocess.run(['c++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'region_plan_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3, r.stdout
    n_boxes = sum(h * (h + 1) // 2 for h in (328, 712, 328 - 3, 712 - 3, 328, 712))
    assert lines[0] == 'region_plan_check: {} boxes planned and checked'.format(n_boxes)
    assert lines[1].startswith('region_plan_check: plan blob mutations:') and lines[2].startswith('region_plan_check: 4000 extreme boxes answered')
