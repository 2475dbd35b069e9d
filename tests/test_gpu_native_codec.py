"""-m gpu: the codec as one library call per direction (include/l3c_hip.h: l3c_encode_batch, l3c_decode_plan + l3c_decode_batch;
l3c-pytorch_amd/native_codec.py).

The C schedule runs the Python schedule's entry points in the same order, so its files must equal `Bitcoding(bp).encode_batch(img)
.to_bytes(paddings)` BYTE FOR BYTE and its pixels must equal the input.  Shapes: 64x96 has one RGB chunk and no probes; 136x200
(27 200 pixels) two probes, six chunks and a short last one; 16 images switch the RGB pipeline to lag 2 and the side stream."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.conftest import GOLDEN, ROOT  # noqa: E402
from tests.golden import make_hip_bitstream as gen  # noqa: E402

_BP, _CODEC, _BC = {}, {}, {}


def blueprint(calibrated=True):
    if calibrated not in _BP:
        _BP[calibrated] = gen.blueprint('cr', calibrated)
    return _BP[calibrated]


def codec(calibrated=True):
    from l3c_pytorch_amd.native_codec import NativeCodec
    if calibrated not in _CODEC:
        _CODEC[calibrated] = NativeCodec(blueprint(calibrated))
    return _CODEC[calibrated]


def bitcoding(calibrated=True):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    if calibrated not in _BC:
        _BC[calibrated] = Bitcoding(blueprint(calibrated))
    return _BC[calibrated]


def _golden_file():
    with open(os.path.join(GOLDEN, 'hip_l3c_cal_64x96.l3c'), 'rb') as f:
        return f.read()


def _image(B, H, W, seed):
    """Smooth images with noise on top (uint8): something the calibrated model codes well below 16 bits per symbol."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    base = 128 + 90 * torch.sin(yy[None, None] / 9.0 + torch.arange(3).view(1, 3, 1, 1)) * torch.cos(xx[None, None] / 13.0 + torch.arange(B).view(B, 1, 1, 1))
    return (base + torch.randint(-12, 13, (B, 3, H, W), generator=g)).clamp(0, 255).to(torch.uint8).cuda()


_REF = {}


def reference(calibrated, B, H, W, seed, paddings):
    """(images, files of the Python path), computed once per case and shared."""
    key = (calibrated, B, H, W, seed)
    if key not in _REF:
        x = _image(B, H, W, seed)
        _REF[key] = (x, bitcoding(calibrated).encode_batch(x).to_bytes(paddings))
    return _REF[key]


PADS3 = [(1, 2, 3, 4), (0, 7, 0, 5), (6, 0, 2, 0)]


def test_golden_file_both_directions():
    img = gen.l3c_case().to(torch.uint8)
    c = codec(True)
    files = c.encode_batch(img)
    assert files == [_golden_file()]
    pixels, pads = c.decode_batch([_golden_file()])
    assert pads == [(0, 0, 0, 0)] and pixels.dtype == torch.uint8
    assert torch.equal(pixels.cpu(), img)


@pytest.mark.parametrize('calibrated', [True, False])
def test_batch_of_three_equals_the_python_path(calibrated):
    x, want = reference(calibrated, 3, 136, 200, 5, PADS3)
    c = codec(calibrated)
    dev_files, file_bytes = c.encode_device(x, PADS3)
    sizes = file_bytes.cpu().numpy()
    assert [int(n) for n in sizes] == [len(f) for f in want]
    host = dev_files.cpu().numpy()
    for b in range(3):
        assert host[b, :sizes[b]].tobytes() == want[b], 'file {}'.format(b)
    assert c.encode_batch(x, PADS3) == want
    pixels, pads = c.decode_batch(want)
    assert pads == PADS3
    assert torch.equal(pixels, x)
    py, py_pads = bitcoding(calibrated).decode_batch(want, out_dtype=torch.uint8)
    assert py_pads == PADS3 and torch.equal(pixels, py)


def test_batch_of_sixteen_on_a_side_stream():
    x = _image(16, 136, 200, 9)
    c = codec(True)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        files = c.encode_batch(x)
        pixels, pads = c.decode_batch(files)          # lag 2: the decoders run on the codec's side stream
    torch.cuda.current_stream().wait_stream(st)
    assert pads == [(0, 0, 0, 0)] * 16
    assert torch.equal(pixels, x)
    assert files[:3] == bitcoding(True).encode_batch(x[:3]).to_bytes()


def _plan_of(c, files):
    from l3c_pytorch_amd.native_codec import decode_plan
    return decode_plan(c.cfg, files)[0]


def test_workspace_contents_do_not_matter():
    x, want = reference(True, 3, 136, 200, 5, PADS3)
    c = codec(True)
    ws = torch.full((c.encode_workspace_bytes(3, 136, 200),), 0xFF, dtype=torch.uint8, device='cuda')
    dev_files, file_bytes = c.encode_device(x, PADS3, workspace=ws)
    sizes = file_bytes.cpu().numpy()
    host = dev_files.cpu().numpy()
    assert [host[b, :sizes[b]].tobytes() for b in range(3)] == want
    ws = torch.full((c.decode_workspace_bytes(_plan_of(c, want)),), 0xFF, dtype=torch.uint8, device='cuda')
    pixels, _ = c.decode_batch(want, workspace=ws)
    assert torch.equal(pixels, x)


def test_two_calls_in_flight_share_one_model():
    x1, want1 = reference(True, 3, 136, 200, 5, PADS3)
    x2 = _image(3, 136, 200, 6)
    want2 = bitcoding(True).encode_batch(x2).to_bytes()
    c = codec(True)
    n = c.encode_workspace_bytes(3, 136, 200)
    ws1, ws2 = torch.empty(n, dtype=torch.uint8, device='cuda'), torch.empty(n, dtype=torch.uint8, device='cuda')
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        f1, n1 = c.encode_device(x1, PADS3, workspace=ws1)
    with torch.cuda.stream(s2):
        f2, n2 = c.encode_device(x2, None, workspace=ws2)
    torch.cuda.synchronize()
    for f, nb, want in ((f1, n1, want1), (f2, n2, want2)):
        host, sizes = f.cpu().numpy(), nb.cpu().numpy()
        assert [host[b, :sizes[b]].tobytes() for b in range(3)] == want
    n = max(c.decode_workspace_bytes(_plan_of(c, want1)), c.decode_workspace_bytes(_plan_of(c, want2)))
    ws1, ws2 = torch.empty(n, dtype=torch.uint8, device='cuda'), torch.empty(n, dtype=torch.uint8, device='cuda')
    with torch.cuda.stream(s1):
        p1, _ = c.decode_batch(want1, workspace=ws1)
    with torch.cuda.stream(s2):
        p2, _ = c.decode_batch(want2, workspace=ws2)
    torch.cuda.synchronize()
    assert torch.equal(p1, x1) and torch.equal(p2, x2)


def test_container_layout_alone():
    from l3c_pytorch_amd import _lib
    B, Cs, stride = 5, (5, 5, 3), 4096
    rng = np.random.RandomState(3)
    nb = [rng.randint(0, 300, B * C).astype(np.uint32) for C in Cs]
    nb[1][2 * 5 + 3] = 0xFFFFFFFF                       # a stream of file 2 overran
    dev = [torch.from_numpy(n.view(np.int32)).cuda() for n in nb]
    sc = (_lib.ContainerScale * 3)(*[_lib.ContainerScale(None, d.data_ptr(), 0, C, 8, 8) for d, C in zip(dev, Cs)])
    off = torch.full((B,), -7, dtype=torch.int64, device='cuda')
    size = torch.full((B,), -7, dtype=torch.int64, device='cuda')
    _lib.call('l3c_container_layout', sc, 3, B, stride, off.data_ptr(), size.data_ptr(), _lib.stream())
    want = 8 + sum(9 + 4 * C + n.reshape(B, C).astype(np.int64).sum(axis=1) for n, C in zip(nb, Cs))
    want[2] = -1
    assert off.cpu().tolist() == [b * stride for b in range(B)]
    assert size.cpu().tolist() == want.tolist()


@pytest.mark.parametrize('n', [1, 15, 16, 17, 4099])
def test_sym_to_u8_alone(n):
    from l3c_pytorch_amd import _lib
    sym = (torch.arange(n, dtype=torch.int64) * 37 % 256).to(torch.int16).cuda()
    out = torch.full((n + 48,), 0xAA, dtype=torch.uint8, device='cuda')
    _lib.call('l3c_sym_to_u8', sym.data_ptr(), n, out.data_ptr(), _lib.stream())
    assert torch.equal(out[:n].cpu(), sym.cpu().to(torch.uint8))
    assert (out[n:] == 0xAA).all()                      # nothing behind the n-th pixel is touched
    if n == 4099:
        assert set(out[:n].cpu().tolist()) == set(range(256))


def test_memory_within_the_python_path():
    """Workspace + outputs of the native calls against the peak of the Python path, measured here: B = 4 at 768x512."""
    B, H, W = 4, 512, 768
    c, bc = codec(True), bitcoding(True)
    x = _image(B, H, W, 21)
    files = bc.encode_batch(x[:1, :, :64, :96]).to_bytes()          # weights packed, constants made: outside the measurement
    bc.decode_batch(files)
    torch.cuda.synchronize()

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        return p, out

    py_enc, enc = peak(lambda: bc.encode_batch(x))
    files = enc.to_bytes()
    del enc
    native_enc = c.encode_workspace_bytes(B, H, W) + B * c.file_stride(H, W) + B * 8
    print('encode: native workspace + outputs {} bytes, Python peak {} bytes'.format(native_enc, py_enc))
    py_dec, out = peak(lambda: bc.decode_batch(files, out_dtype=torch.uint8))
    del out
    plan = _plan_of(c, files)
    native_dec = c.decode_workspace_bytes(plan) + B * 3 * H * W + (sum(len(f) for f in files) + 20) + len(plan)
    print('decode: native workspace + files + plan + pixels {} bytes, Python peak {} bytes'.format(native_dec, py_dec))
    assert native_enc <= py_enc, (native_enc, py_enc)
    assert native_dec <= py_dec, (native_dec, py_dec)
    pixels, _ = c.decode_batch(files)
    assert torch.equal(pixels, x)


def _write_weights(path, cfg, sd):
    from l3c_pytorch_amd.native_net import param_schema
    names = param_schema(cfg)
    with open(path, 'wb') as f:
        f.write(b'L3CW' + struct.pack('<I', len(names)))
        for name, shape in names:
            t = sd[name].detach().cpu().float().contiguous().numpy()
            assert tuple(t.shape) == shape
            f.write(struct.pack('<I', len(name)) + name.encode() + struct.pack('<I', len(shape)))
            f.write(np.asarray(shape, dtype=np.int64).tobytes() + t.astype(np.float32).tobytes())


def test_a_caller_without_torch_writes_and_reads_the_committed_file(tmp_path):
    """tests/cabi/codec_main.cpp: l3c_hip.h + libl3c_hip.so + the HIP runtime, run as a child process."""
    exe = tmp_path / 'codec_main'
    libdir = os.path.join(ROOT, 'l3c-pytorch_amd', 'csrc')
    subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'codec_main.cpp'), '-L', libdir, '-ll3c_hip', '-Wl,-rpath,' + libdir,
                    '-o', str(exe)], check=True, timeout=180)
    c = codec(True)
    _write_weights(str(tmp_path / 'w.bin'), c.cfg, blueprint(True).net.state_dict())
    with open(tmp_path / 'tables.bin', 'wb') as f:
        f.write(b'L3CT' + struct.pack('<Iff', c.cfg.L, c.model.z_x_min, c.model.z_bin_width))
        f.write(c.targets_rgb.cpu().numpy().astype(np.float32).tobytes() + c.targets_z.cpu().numpy().astype(np.float32).tobytes())
        f.write(c.uniform_row.cpu().numpy().astype(np.int16).tobytes())
    img = gen.l3c_case().numpy().astype(np.uint8)
    _, _, H, W = img.shape
    with open(tmp_path / 'img.bin', 'wb') as f:
        f.write(np.asarray([H, W], dtype=np.int64).tobytes() + np.ascontiguousarray(img[0]).tobytes())
    cfg = c.cfg
    args = [str(v) for v in (cfg.num_scales, cfg.Cf, cfg.C, cfg.L, cfg.K, cfg.enc_blocks, cfg.dec_blocks, cfg.rgb_baseline, cfg.dec_skip)]
    r = subprocess.run([str(exe), 'enc', str(tmp_path / 'w.bin'), str(tmp_path / 'tables.bin'), str(tmp_path / 'img.bin'),
                        str(tmp_path / 'out.l3c')] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(tmp_path / 'out.l3c', 'rb') as f:
        assert f.read() == _golden_file()
    r = subprocess.run([str(exe), 'dec', str(tmp_path / 'w.bin'), str(tmp_path / 'tables.bin'), os.path.join(GOLDEN, 'hip_l3c_cal_64x96.l3c'),
                        str(tmp_path / 'out.raw')] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(str(tmp_path / 'out.raw'), dtype=np.uint8)
    assert raw[:16].view(np.int64).tolist() == [H, W] and raw[16:24].view(np.uint16).tolist() == [0, 0, 0, 0]
    assert np.array_equal(raw[24:].reshape(3, H, W), img[0])
