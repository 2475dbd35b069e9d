"""-m gpu: region decode through the C ABI (include/l3c_hip.h: l3c_net_get_p_rows, l3c_decode_region_plan + l3c_decode_region), driven through
native_codec.NativeCodec.decode_region.

The library moves integers and reruns the kernels of the Python path in the Python path's order, so every comparison is torch.equal: the
windowed P against MultiscaleNetwork.get_P_rows on ALL window rows and against l3c_net_get_p's full-frame P on the valid rows; the decoded
box against the crop of the input and against Bitcoding.decode_region on the same files, pixels and every RegionInfo field.  Shapes, files
and boxes are those of tests/test_gpu_region.py (shared: encoded once per session); outputs and workspaces sit inside canary-filled buffers."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd import _lib  # noqa: E402
from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from l3c_pytorch_amd.bitcoding.container import SealError  # noqa: E402
from tests.conftest import ROOT  # noqa: E402
from tests.test_gpu_region import HALO, P_CASES, Calls, bitcoding, blueprint, boxes, crop, encoded, images  # noqa: E402

CANARY = 0xA5
GUARD = 4096
_CODEC = {}


def codec():
    from l3c_pytorch_amd.native_codec import NativeCodec
    if 'c' not in _CODEC:
        _CODEC['c'] = NativeCodec(blueprint())
    return _CODEC['c']


def guarded(nbytes):
    """(the whole canary-filled buffer, its middle `nbytes` bytes at a 256-byte aligned address)."""
    whole = torch.full((GUARD + nbytes + GUARD,), CANARY, dtype=torch.uint8, device='cuda')
    assert whole.data_ptr() % 256 == 0
    return whole, whole[GUARD:GUARD + nbytes]


def intact(whole, nbytes):
    return bool((whole[:GUARD] == CANARY).all()) and bool((whole[GUARD + nbytes:] == CANARY).all())


def same_info(a, b):
    return a.as_dict() == b.as_dict()


# ---- 1. l3c_net_get_p_rows ----------------------------------------------------------------------------------------------------------


def get_p_rows(c, bn_q, fuse, c0, c1):
    """l3c_net_get_p_rows with the exact workspace and P inside canary-filled buffers -> P (B, c1 - c0, W, Kp)."""
    lib = _lib.load()
    B, _, h, w = bn_q.shape
    Kp = c.net.kp(0)
    ws_bytes = lib.l3c_net_get_p_rows_workspace_bytes(c._cfg_ref, B, h, w, c0, c1)
    assert ws_bytes > 0, lib.l3c_last_error()
    ws_all, ws = guarded(ws_bytes)
    p_bytes = B * (c1 - c0) * 2 * w * Kp * 4
    p_all, p = guarded(p_bytes)
    d = _lib.NetGetPRowsDesc(ctypes.pointer(c.cfg), _lib.ptr(c.net.packed), c.net.packed_bytes, 0, _lib.ptr(bn_q), B, h, w, _lib.ptr(fuse), c0, c1,
                             p.data_ptr(), ws.data_ptr(), ws_bytes)
    _lib.call('l3c_net_get_p_rows', ctypes.byref(d), _lib.stream())
    torch.cuda.synchronize()
    assert intact(ws_all, ws_bytes) and intact(p_all, p_bytes), 'l3c_net_get_p_rows wrote outside its workspace or P'
    return p.view(torch.float32).view(B, c1 - c0, 2 * w, Kp)


@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('H,windows', P_CASES)
def test_window_P_is_get_P_rows_and_the_frames_P(H, windows, B):
    """One forward pass of the Python network; on its z1 and F1 the library's windowed P equals MultiscaleNetwork.get_P_rows on every row of
    the window (the schedule is the same) and l3c_net_get_p's full-frame P on the valid rows; the first 40 rows of a cut window differ."""
    c = codec()
    net = blueprint().net
    W = 88
    out = net(images(B, H, W).float().cuda())
    bn_q, F1 = out.raw.bn_q[1].contiguous(), out.raw.F_dec[1].contiguous()
    assert tuple(bn_q.shape) == (B, 5, H // 2, W // 2) and tuple(F1.shape) == (B, H // 2, W // 2, 64)
    P_full = c.net.get_P(0, bn_q, F1.permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
    assert torch.equal(P_full, out.raw.P[0])
    for c0, c1 in windows:
        v0, v1 = (0 if c0 == 0 else c0 + HALO), (H if c1 == H else c1 - HALO)
        P = get_p_rows(c, bn_q, F1, c0, c1)
        want = net.get_P_rows(0, bn_q, F1.permute(0, 3, 1, 2), (c0, c1))
        assert tuple(P.shape) == tuple(want.shape)
        assert torch.equal(P, want), (H, B, (c0, c1), int((P != want).sum()))
        assert torch.equal(P[:, v0 - c0:v1 - c0], P_full[:, v0:v1]), (H, B, (c0, c1))
        if c0:
            assert not torch.equal(P[:, :HALO], P_full[:, c0:c0 + HALO])


# ---- 2. round trip -----------------------------------------------------------------------------------------------------------------


def decode_region_guarded(c, files, box, monkeypatch):
    """NativeCodec.decode_region with its output tensor placed inside a canary-filled buffer."""
    real = torch.empty
    held = {}

    def empty(*shape, **kw):
        if kw.get('dtype') == torch.uint8 and len(shape) == 4 and shape[1] == 3:
            n = int(np.prod(shape))
            held['whole'], mid = guarded((n + 255) // 256 * 256)
            held['n'] = n
            return mid[:n].view(*shape)
        return real(*shape, **kw)
    monkeypatch.setattr(torch, 'empty', empty)
    try:
        got, info = c.decode_region(files, box)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(torch, 'empty', real)
    w, n = held['whole'], held['n']
    assert bool((w[:GUARD] == CANARY).all()) and bool((w[GUARD + n:] == CANARY).all()), 'l3c_decode_region wrote outside `pixels`'
    return got, info


@pytest.mark.parametrize('K,B', [(16, 1), (64, 1), (64, 3)])
@pytest.mark.parametrize('H,W', [(317, 83), (328, 88)])
def test_round_trip(H, W, K, B, monkeypatch):
    x, files, padding = encoded(K, B, H, W)
    bc, c = bitcoding(K), codec()
    lags = set()
    for box in boxes(H, W):
        want, want_info = bc.decode_region(files, box)
        got, info = decode_region_guarded(c, files, box, monkeypatch)
        assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got, crop(x, box)), (box, info)
        assert torch.equal(got, want) and same_info(info, want_info), (box, info, want_info)
        lags.add(bc._rgb_schedule(B * (info.bands[1] - info.bands[0]), None)[0])
    assert lags == {1, 2}


@pytest.mark.parametrize('K,B', [(64, 1), (16, 2)])
def test_round_trip_tall(K, B, monkeypatch):
    """712x88: boxes whose decoder stage is cut on both sides, at the top only, and not at all."""
    H, W = 712, 88
    x, files, _ = encoded(K, B, H, W)
    bc, c = bitcoding(K), codec()
    for box, decoder in (((330, 360), (64, 640)), ((500, 520, 7, 80), (256, 712)), ((40, 41), (0, 320)), ((711, 712), (448, 712)), ((0, H), (0, H))):
        want, want_info = bc.decode_region(files, box)
        got, info = decode_region_guarded(c, files, box, monkeypatch)
        assert torch.equal(got, crop(x, box)) and torch.equal(got, want), (box, info)
        assert same_info(info, want_info), (box, info, want_info)
        if K == 64:
            assert info.decoder_rows == decoder, (box, info)


def test_box_and_file_refusals_match_bitcoding():
    x, files, padding = encoded(16, 1, 317, 83)
    bc, c = bitcoding(16), codec()
    for box in ((5, 5), (9, 4), (0, 318), (-1, 3), (0, 10, 0, 84), (0, 10, 5, 5), (1, 2, 3), (0, 2 ** 40)):
        with pytest.raises(ValueError) as want:
            bc.decode_region(files, box)
        with pytest.raises(ValueError) as got:
            c.decode_region(files, box)
        if max(abs(v) for v in box) < 2 ** 31:
            assert str(got.value) == str(want.value), box
    from l3c_pytorch_amd.helpers import pad
    other = bc.encode_batch(pad.pad(images(1, 317, 83).long(), fac=8, mode=blueprint().get_padding_mode())[0].cuda()).to_bytes([(3, 2, 2, 1)])
    with pytest.raises(ValueError) as want:
        bc.decode_region(files + other, (0, 10))
    with pytest.raises(ValueError) as got:
        c.decode_region(files + other, (0, 10))
    assert str(got.value) == str(want.value) and 'one padding tuple' in str(got.value)
    with pytest.raises(ValueError):
        c.decode_region([], (0, 10))
    with pytest.raises(ValueError):
        c.decode_region([files[0][:-9]], (0, 10))                  # a truncated file: the planner's message


# ---- 3. the rest is really not read ------------------------------------------------------------------------------------------------


def test_bands_outside_the_region_are_not_read():
    """The construction of tests/test_gpu_region.py: 320x88, K = 16, box (190, 210) lies in bands 9 and 10; bands 3 and 13 of every channel,
    complemented, destroy the whole decode and leave the region alone."""
    x, files, _ = encoded(16, 1, 320, 88)
    c = codec()
    box = (190, 210)
    parsed = container.parse_banded(files[0])
    offset, nbytes = parsed.offset[-1], parsed.nbytes[-1]
    damaged = np.frombuffer(files[0], dtype=np.uint8).copy()
    for ch in range(3):
        for j in (3, 13):
            a, n = int(offset[ch, j]), int(nbytes[ch, j])
            assert n > 16
            damaged[a:a + n] ^= 0xFF
    damaged = damaged.tobytes()
    got, info = c.decode_region([damaged], box)
    assert torch.equal(got, crop(x, box))
    assert info.bands == (9, 11) and info.sym_rows == (183, 210) and info.conv_rows == (128, 256) and info.valid_rows == (168, 216)
    assert info.streams_used == 6 and info.streams_total == 48
    assert info.bytes_used == int(nbytes[:, 9:11].sum()) < info.bytes_total == int(nbytes.sum())
    assert not torch.equal(c.decode_batch([damaged])[0], x)                # the test bites


# ---- 4. legacy file ----------------------------------------------------------------------------------------------------------------


def test_legacy_file():
    x, files, _ = encoded(0, 1, 320, 88)
    assert not container.is_banded(files[0])
    c, bc = codec(), bitcoding(0)
    for box, conv in (((0, 40), (0, 128)), ((300, 320, 80, 88), (0, 320))):
        got, info = c.decode_region(files, box)
        want, want_info = bc.decode_region(files, box)
        assert torch.equal(got, crop(x, box)) and torch.equal(got, want) and same_info(info, want_info), (box, info, want_info)
        assert info.conv_rows == conv and info.bands == (0, 1) and info.n_bands == 1 and info.streams_used == info.streams_total == 3


# ---- 5. sealed banded file ---------------------------------------------------------------------------------------------------------


def test_sealed_banded_file(monkeypatch):
    x, files, _ = encoded(16, 1, 320, 88, seal=True)
    assert container.is_sealed(files[0])
    c, bc = codec(), bitcoding(16)
    got, info = c.decode_region(files, (180, 200))
    assert torch.equal(got, crop(x, (180, 200)))
    assert info.sealed == 1 and info.verified == ('generation', 'model') and info.pixel_crc_checked is False
    assert same_info(info, bc.decode_region(files, (180, 200))[1])
    got, info = c.decode_region(files, (180, 200), verify=False)
    assert torch.equal(got, crop(x, (180, 200))) and info.sealed == 1 and info.verified == () and info.pixel_crc_checked is False
    body, seal = container.split_seal(files[0])
    foreign = body + container.make_seal(body, seal.generation, seal.frame_crc, seal.model_id ^ 1)       # a seal of another model
    c.model_id()                                                                                         # (computed once, outside the count)
    calls = Calls(monkeypatch)
    with pytest.raises(SealError) as e:
        c.decode_region([foreign], (180, 200))
    assert e.value.reason == 'model' and e.value.index == 0 and calls.n == 0            # before any library decode call
    c.decode_region(files, (180, 200))
    assert calls.n > 0                                                                  # the counter does see a decode that runs
    monkeypatch.undo()
    assert torch.equal(c.decode_region([foreign], (180, 200), verify=False)[0], crop(x, (180, 200)))


# ---- 6. a caller without torch -----------------------------------------------------------------------------------------------------


def test_a_caller_without_torch_region_decodes_two_boxes(tmp_path):
    """tests/cabi/codec_region_main.cpp: l3c_hip.h + libl3c_hip.so + the HIP runtime, built and run as a child process under a time limit."""
    from tests.test_gpu_native_banded import _write_weights
    exe = tmp_path / 'codec_region_main'
    libdir = os.path.join(ROOT, 'l3c-pytorch_amd', 'csrc')
    subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'codec_region_main.cpp'), '-L', libdir, '-ll3c_hip', '-Wl,-rpath,' + libdir,
                    '-o', str(exe)], check=True, timeout=180)
    c = codec()
    _write_weights(str(tmp_path / 'w.bin'), c.cfg, blueprint().net.state_dict())
    with open(tmp_path / 'tables.bin', 'wb') as f:
        f.write(b'L3CT' + struct.pack('<Iff', c.cfg.L, c.model.z_x_min, c.model.z_bin_width))
        f.write(c.targets_rgb.cpu().numpy().astype(np.float32).tobytes() + c.targets_z.cpu().numpy().astype(np.float32).tobytes())
        f.write(c.uniform_row.cpu().numpy().astype(np.int16).tobytes())
    cfg = [str(getattr(c.cfg, n)) for n, _ in _lib.NetConfig._fields_]
    r = subprocess.run([str(exe), str(tmp_path / 'w.bin'), str(tmp_path / 'tables.bin')] + cfg, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and lines[0].startswith('codec_region_main: 328 x 88, 16 bands -> '), r.stdout
    assert 'rows [190, 215) x columns [0, 88): bands 9..10 of 16, conv rows 128..255' in lines[1] and '6 of 48 streams' in lines[1]
    assert 'rows [300, 328) x columns [5, 60)' in lines[2] and 'conv rows 192..327' in lines[2] and lines[2].endswith('equal to the image')
