"""-m gpu: the banded codec behind the C ABI (include/l3c_hip.h: l3c_encode_batch_banded, l3c_decode_plan_banded + l3c_decode_batch_banded,
l3c_ac_decode_bands, l3c_container_layout_banded), driven through native_codec.NativeCodec(bp, bands=K).

The C schedule runs the Python schedule's entry points in the same order, so its files must equal `Bitcoding(bp, bands=K).encode_batch(img)
.to_bytes(paddings)` BYTE FOR BYTE and its pixels must equal the input.  Shapes: 136x200 with K = 4 has a coarsest scale of 425 symbols in
bands of 128 (a last band of 41) and 12 RGB bands (lag 1), with K = 64 a coarsest scale of 7 bands and 183 RGB bands (lag 2, the side
stream); 24x40 has a coarsest scale of 15 symbols; 64x96 with K = 4 a second record of three bands of 128 (a last band equal to L)."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ac as oracle_ac  # noqa: E402
from tests.conftest import GOLDEN, ROOT  # noqa: E402
from tests.golden import make_hip_bitstream as gen  # noqa: E402

_BP, _CODEC, _BC = {}, {}, {}


def blueprint(calibrated=True):
    if calibrated not in _BP:
        _BP[calibrated] = gen.blueprint('cr', calibrated)
    return _BP[calibrated]


def codec(K, calibrated=True):
    from l3c_pytorch_amd.native_codec import NativeCodec
    if (K, calibrated) not in _CODEC:
        _CODEC[K, calibrated] = NativeCodec(blueprint(calibrated), bands=K)
    return _CODEC[K, calibrated]


def bitcoding(K, calibrated=True):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    if (K, calibrated) not in _BC:
        _BC[K, calibrated] = Bitcoding(blueprint(calibrated), bands=K)
    return _BC[K, calibrated]


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


def reference(calibrated, K, B, H, W, seed, paddings):
    """(images, files of the Python path), computed once per case and shared."""
    key = (calibrated, K, B, H, W, seed)
    if key not in _REF:
        x = _image(B, H, W, seed)
        _REF[key] = (x, bitcoding(K, calibrated).encode_batch(x).to_bytes(paddings))
    return _REF[key]


PADS3 = [(1, 2, 3, 4), (0, 7, 0, 5), (6, 0, 2, 0)]


# ---- the two kernels alone ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('Lp', [26, 257])
@pytest.mark.parametrize('n_sym,band_len', [(64, 64), (65, 64), (96, 64), (128, 64), (1000, 192), (15, 64)])
def test_ac_decode_bands_alone(n_sym, band_len, Lp):
    """Random symbols per band, encoded band by band by the CPU oracle coder with the uniform row, decoded in ONE launch."""
    from l3c_pytorch_amd import _lib, ops
    from l3c_pytorch_amd.bitcoding.bitcoding import uniform_cdf_row
    planes, n = 3, -(-n_sym // band_len)
    rng = np.random.RandomState(n_sym * 7 + Lp)
    row = uniform_cdf_row(Lp - 1)
    row_np = row.numpy().view(np.uint16)
    sym = rng.randint(0, Lp - 1, (planes, n_sym)).astype(np.int16)
    sym[0, :min(n_sym, 3)] = Lp - 2                                 # the top symbol at a band's start, 0 at the end of the planes
    sym[:, -1] = 0
    payloads = [oracle_ac.encode(row_np, sym[p, j * band_len:(j + 1) * band_len]) for p in range(planes) for j in range(n)]
    buf, offs, lens = ops.pack_streams(payloads)
    row_d = row.cuda()
    PAD = 192
    out = torch.full((PAD + planes * n_sym + PAD,), -7777, dtype=torch.int16, device='cuda')
    _lib.call('l3c_ac_decode_bands', row_d.data_ptr(), Lp, buf.data_ptr(), offs.data_ptr(), lens.data_ptr(), planes, n_sym, band_len, 1,
              out.data_ptr() + 2 * PAD, _lib.stream())
    got = out.cpu().numpy()
    assert (got[:PAD] == -7777).all() and (got[-PAD:] == -7777).all()            # nothing outside the planes is touched
    assert np.array_equal(got[PAD:-PAD].reshape(planes, n_sym), sym)
    for p in range(planes):                                                      # and what l3c_ac_decode gives for every band alone
        for j in range(n):
            i, length = p * n + j, min(band_len, n_sym - j * band_len)
            alone = ops.ac_decode(row_d, buf, offs[i:i + 1], lens[i:i + 1], 1, length, True, broadcast_row=True)
            assert np.array_equal(alone.cpu().numpy().reshape(-1), got[PAD + p * n_sym + j * band_len:][:length]), (p, j)


@pytest.mark.parametrize('n', [1, 6])
def test_container_layout_banded_alone(n):
    from l3c_pytorch_amd import _lib
    B, stride = 5, 1 << 16
    shapes = [(5, 8, 8 * n, 64), (5, 16, 4 * n, 64), (3, 4, 16 * n, 64)]        # n bands of 64 symbols per channel
    rng = np.random.RandomState(3 + n)
    full = [rng.randint(0, 300, B * C * (n - 1)).astype(np.uint32) for C, _, _, _ in shapes]
    last = [rng.randint(0, 300, B * C).astype(np.uint32) for C, _, _, _ in shapes]

    def run():
        dev = [(torch.from_numpy(f.view(np.int32)).cuda() if n > 1 else None, torch.from_numpy(t.view(np.int32)).cuda()) for f, t in zip(full, last)]
        sc = (_lib.BandedScale * 3)(*[_lib.BandedScale(None, f.data_ptr() if f is not None else None, 0, None, t.data_ptr(), 0, C, H, W, L)
                                      for (f, t), (C, H, W, L) in zip(dev, shapes)])
        off = torch.full((B,), -7, dtype=torch.int64, device='cuda')
        size = torch.full((B,), -7, dtype=torch.int64, device='cuda')
        _lib.call('l3c_container_layout_banded', sc, 3, B, stride, off.data_ptr(), size.data_ptr(), _lib.stream())
        assert off.cpu().tolist() == [b * stride for b in range(B)]
        return size.cpu().tolist()

    def sums():
        w = np.full(B, 14, dtype=np.int64)
        for (C, _, _, _), f, t in zip(shapes, full, last):
            w += 9 + 4 * C * n + 4 + t.reshape(B, C).astype(np.int64).sum(axis=1)
            if n > 1:
                w += f.reshape(B, C * (n - 1)).astype(np.int64).sum(axis=1)
        return w

    want = sums()
    assert run() == want.tolist()
    # one overrun in a full band of file 1 (n == 1: there is none, a last band of another scale) and one in a last band of file 3
    if n > 1:
        full[1][1 * 5 * (n - 1) + 2 * (n - 1) + 3] = 0xFFFFFFFF
    else:
        last[0][1 * 5 + 4] = 0xFFFFFFFF
    last[2][3 * 3 + 1] = 0xFFFFFFFF
    want[1] = want[3] = -1
    assert run() == want.tolist()


# ---- files and pixels ----------------------------------------------------------------------------------------------------------------


def _files_of(c, x, pads, workspace=None):
    dev_files, file_bytes = c.encode_device(x, pads, workspace=workspace)
    sizes = file_bytes.cpu().numpy()
    host = dev_files.cpu().numpy()
    assert (sizes > 0).all() and int(sizes.max()) <= dev_files.shape[1]
    return [host[b, :sizes[b]].tobytes() for b in range(x.shape[0])]


@pytest.mark.parametrize('calibrated', [True, False])
@pytest.mark.parametrize('K', [1, 4, 64])
def test_batch_of_three_equals_the_python_path(K, calibrated):
    from l3c_pytorch_amd.native_codec import decode_plan_banded, parse_plan_banded
    x, want = reference(calibrated, K, 3, 136, 200, 5, PADS3)
    c = codec(K, calibrated)
    got = _files_of(c, x, PADS3)
    for b in range(3):
        assert got[b] == want[b], 'file {}'.format(b)
    assert c.encode_batch(x, PADS3) == want
    plan = parse_plan_banded(decode_plan_banded(c.cfg, want)[0])
    assert plan['lag'] == (2 if K == 64 else 1)
    sym = torch.full((3, 3, 136, 200), -1, dtype=torch.int16, device='cuda')
    pixels, pads = c.decode_batch(want, sym=sym)
    assert pads == PADS3 and pixels.dtype == torch.uint8
    assert torch.equal(pixels, x)
    assert torch.equal(sym, x.to(torch.int16))
    # either side reads the other's files (whatever band count the reading side would write with)
    py, py_pads = bitcoding(K, calibrated).decode_batch(got, out_dtype=torch.uint8)
    assert py_pads == PADS3 and torch.equal(py, x)
    pixels0, _ = codec(0, calibrated).decode_batch(want)
    assert torch.equal(pixels0, x)


@pytest.mark.parametrize('K', [1, 4, 64])
def test_a_coarsest_scale_of_fifteen_symbols(K):
    x, want = reference(True, K, 1, 24, 40, 8, [(0, 0, 5, 0)])
    c = codec(K)
    assert c.encode_batch(x, [(0, 0, 5, 0)]) == want
    pixels, pads = c.decode_batch(want)
    assert pads == [(0, 0, 5, 0)] and torch.equal(pixels, x)


def test_one_image_of_four_bands_runs_without_a_side_stream():
    """B = 1 at 64x96, K = 4: B n = 4 RGB bands, lag 1 -- l3c_decode_batch_banded is handed side_stream = NULL."""
    from l3c_pytorch_amd.native_codec import decode_plan_banded, parse_plan_banded
    x, want = reference(True, 4, 1, 64, 96, 12, None)
    c = codec(4)
    assert c.encode_batch(x) == want
    plan = parse_plan_banded(decode_plan_banded(c.cfg, want)[0])
    assert plan['lag'] == 1 and plan['records'][1][3:5] == (128, 3)
    side = c._side
    pixels, pads = c.decode_batch(want)
    assert c._side is side                                              # no side stream was made for it
    assert pads == [(0, 0, 0, 0)] and torch.equal(pixels, x)
    with pytest.raises(ValueError, match='mixes'):
        c.decode_batch([want[0], _golden_file()])


def test_one_band_is_the_committed_legacy_payloads():
    """An anchor that does not pass through Bitcoding's banded code: the K = 1 native file of the committed image carries exactly the
    committed legacy file's payloads, record by record."""
    from l3c_pytorch_amd.bitcoding import container
    img = gen.l3c_case().to(torch.uint8)
    legacy = _golden_file()
    data = codec(1).encode_batch(img)[0]
    p, q = container.parse_banded(data), container.parse_containers([legacy])
    assert [s[:3] for s in p.scales] == [tuple(s) for s in q.scales] and all(s[3] == 64 * -(-(s[1] * s[2]) // 64) for s in p.scales)
    for k, (C, H, W) in enumerate(q.scales):
        assert p.offset[k].shape == (C, 1)
        for ch in range(C):
            o, n = int(q.offset[k][0, ch]), int(q.nbytes[k][0, ch])
            ob, nb = int(p.offset[k][ch, 0]), int(p.nbytes[k][ch, 0])
            assert data[ob:ob + nb] == legacy[o:o + n], (k, ch)
    assert len(data) == len(legacy) + 6 + 4 * len(q.scales)
    pixels, _ = codec(1).decode_batch([data])
    assert torch.equal(pixels.cpu(), img)
    assert torch.equal(codec(1).decode_batch([legacy])[0].cpu(), img)     # and a banded codec still reads the legacy file


def _plan_of(c, files):
    from l3c_pytorch_amd.native_codec import decode_plan_banded
    return decode_plan_banded(c.cfg, files)[0]


@pytest.mark.parametrize('fill', ['ff', 'random'])
def test_workspace_contents_do_not_matter(fill):
    x, want = reference(True, 64, 3, 136, 200, 5, PADS3)
    c = codec(64)

    def workspace(n):
        if fill == 'ff':
            return torch.full((n,), 0xFF, dtype=torch.uint8, device='cuda')
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device='cuda', generator=torch.Generator('cuda').manual_seed(n))

    assert _files_of(c, x, PADS3, workspace(c.encode_workspace_bytes(3, 136, 200))) == want
    pixels, _ = c.decode_batch(want, workspace=workspace(c.decode_workspace_bytes(_plan_of(c, want))))
    assert torch.equal(pixels, x)


def test_two_calls_in_flight_share_one_model():
    x1, want1 = reference(True, 64, 3, 136, 200, 5, PADS3)
    x2 = _image(3, 136, 200, 6)
    want2 = bitcoding(64).encode_batch(x2).to_bytes()
    c = codec(64)
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
    # two decodes in flight: each with a codec of its own for the side stream its lag-2 decoders run on, one packed model
    from l3c_pytorch_amd.native_codec import NativeCodec
    c2 = NativeCodec.__new__(NativeCodec)
    c2.__dict__.update(c.__dict__)
    c2._side = None
    n = max(c.decode_workspace_bytes(_plan_of(c, want1)), c.decode_workspace_bytes(_plan_of(c, want2)))
    ws1, ws2 = torch.empty(n, dtype=torch.uint8, device='cuda'), torch.empty(n, dtype=torch.uint8, device='cuda')
    with torch.cuda.stream(s1):
        p1, _ = c.decode_batch(want1, workspace=ws1)
    with torch.cuda.stream(s2):
        p2, _ = c2.decode_batch(want2, workspace=ws2)
    torch.cuda.synchronize()
    assert c._side is not None and c2._side is not None and c._side is not c2._side and c2.net is c.net
    assert torch.equal(p1, x1) and torch.equal(p2, x2)


def test_memory_within_the_python_path():
    """Workspace + outputs of the native banded calls against the peak of Bitcoding(bands=64), measured here: B = 4 at 768x512."""
    B, H, W, K = 4, 512, 768, 64
    c, bc = codec(K), bitcoding(K)
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
    assert c.encode_batch(x[:2]) == files[:2]


# ---- a caller without torch ------------------------------------------------------------------------------------------------------------


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


def test_a_caller_without_torch_round_trips_the_committed_image(tmp_path):
    """tests/cabi/codec_banded_main.cpp: l3c_hip.h + libl3c_hip.so + the HIP runtime, run as a child process; K = 64: lag 2."""
    K = 64
    exe = tmp_path / 'codec_banded_main'
    libdir = os.path.join(ROOT, 'l3c-pytorch_amd', 'csrc')
    subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'codec_banded_main.cpp'), '-L', libdir, '-ll3c_hip', '-Wl,-rpath,' + libdir,
                    '-o', str(exe)], check=True, timeout=180)
    c = codec(K)
    _write_weights(str(tmp_path / 'w.bin'), c.cfg, blueprint(True).net.state_dict())
    with open(tmp_path / 'tables.bin', 'wb') as f:
        f.write(b'L3CT' + struct.pack('<Iff', c.cfg.L, c.model.z_x_min, c.model.z_bin_width))
        f.write(c.targets_rgb.cpu().numpy().astype(np.float32).tobytes() + c.targets_z.cpu().numpy().astype(np.float32).tobytes())
        f.write(c.uniform_row.cpu().numpy().astype(np.int16).tobytes())
    image = gen.l3c_case()
    img = image.numpy().astype(np.uint8)
    _, _, H, W = img.shape
    with open(tmp_path / 'img.bin', 'wb') as f:
        f.write(np.asarray([H, W], dtype=np.int64).tobytes() + np.ascontiguousarray(img[0]).tobytes())
    cfg = c.cfg
    args = [str(v) for v in (cfg.num_scales, cfg.Cf, cfg.C, cfg.L, cfg.K, cfg.enc_blocks, cfg.dec_blocks, cfg.rgb_baseline, cfg.dec_skip)]
    r = subprocess.run([str(exe), str(tmp_path / 'w.bin'), str(tmp_path / 'tables.bin'), str(tmp_path / 'img.bin'), str(tmp_path / 'out.l3c'),
                        str(K)] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'equal to the image' in r.stdout
    with open(tmp_path / 'out.l3c', 'rb') as f:
        assert f.read() == bitcoding(K).encode_batch(image).to_bytes()[0]
