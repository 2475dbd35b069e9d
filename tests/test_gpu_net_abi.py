"""-m gpu: the whole network as one library call each (include/l3c_hip.h: l3c_net_forward / l3c_net_get_p; l3c-pytorch_amd/native_net.py).

The C schedule runs the Python schedule's kernels with the same descriptors in the same order, so everything it writes must equal
MultiscaleNetwork BIT FOR BIT -- the bitstream contract rests on it (include/l3c_hip.h, L3C_BITSTREAM_GENERATION)."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.conftest import GOLDEN, ROOT  # noqa: E402
from tests.golden import make_hip_bitstream as gen  # noqa: E402


@pytest.fixture(scope='module')
def record():
    with open(os.path.join(GOLDEN, 'hip_bitstream.json')) as f:
        return json.load(f)


_BP = {}


def blueprint(name, calibrated=True):
    if (name, calibrated) not in _BP:
        _BP[(name, calibrated)] = gen.blueprint(name, calibrated)
    return _BP[(name, calibrated)]


_NATIVE = {}


def native(name, calibrated=True):
    from l3c_pytorch_amd.native_net import NativeNet
    if (name, calibrated) not in _NATIVE:
        _NATIVE[(name, calibrated)] = NativeNet(blueprint(name, calibrated).net)
    return _NATIVE[(name, calibrated)]


def _image(B, H, W, seed, halves=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (B, 3, H, W), generator=g).float()
    if halves:      # exact .5 values (round half to even) and other fractions, still inside [0, 255]
        frac = torch.tensor([0.0, 0.5, 0.25, -0.5])[torch.randint(0, 4, (B, 3, H, W), generator=g)]
        x = (x + frac).clamp(0, 255)
    return x.cuda()


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), '{} differs in {} of {} elements'.format(what, int((a != b).sum()), a.numel())


def _assert_forward_equal(got, want, what=''):
    S = len(want.raw.P)
    assert len(got.raw.P) == S
    _same(got.raw.sym[0], want.raw.sym[0], what + 'sym[0]')
    for s in range(S):
        _same(got.raw.sym[s + 1], want.raw.sym[s + 1], what + 'sym[{}]'.format(s + 1))
        _same(got.raw.bn_q[s + 1], want.raw.bn_q[s + 1], what + 'bn_q[{}]'.format(s + 1))
        _same(got.raw.P[s], want.raw.P[s], what + 'P[{}]'.format(s))
        if want.raw.F_enc and got.raw.F_enc[s] is not None:
            _same(got.raw.F_enc[s], want.raw.F_enc[s], what + 'F_enc[{}]'.format(s))
            _same(got.raw.F_dec[s], want.raw.F_dec[s], what + 'F_dec[{}]'.format(s))
    for s in range(S + 1):
        _same(got.S[s], want.S[s], what + 'S[{}]'.format(s))


@pytest.mark.parametrize('calibrated', [False, True])
def test_native_forward_hashes_to_the_committed_values(record, calibrated):
    want = record['forward_64x96']['calibrated' if calibrated else 'default']
    out = native('cr', calibrated).forward(gen.l3c_case().float().cuda())
    assert [gen.sha(S.cpu().numpy().astype(np.int16)) for S in out.S] == want['S']
    assert [gen.sha(P.contiguous().cpu().numpy().astype(np.float32)) for P in out.P] == want['P']


@pytest.mark.parametrize('B,H,W,halves', [(2, 512, 768, False), (3, 136, 200, True)])
def test_native_forward_equals_the_python_schedule(B, H, W, halves):
    x = _image(B, H, W, seed=H + W, halves=halves)
    want = blueprint('cr').net.forward(x)
    got = native('cr').forward(x)
    assert got.raw.F_enc[0] is not None and got.raw.F_dec[0] is not None
    _assert_forward_equal(got, want)
    # without the optional feature outputs: F_dec[0] lives in P[0]'s memory until the last layer -- same bits
    _assert_forward_equal(native('cr').forward(x, features=False), want, 'features=False: ')


def test_native_get_P_equals_the_forward_and_the_python_get_P():
    net = blueprint('cr').net
    nn = native('cr')
    x = _image(2, 136, 200, seed=7)
    out = net.forward(x)
    S = len(out.raw.P)
    for s in range(S):
        bn_q = out.raw.bn_q[s + 1]
        prev = None if s == S - 1 else out.raw.F_dec[s + 1].permute(0, 3, 1, 2)
        P, F = nn.get_P(s, bn_q, prev)
        _same(P.contiguous(), out.P[s].contiguous(), 'get_P P[{}]'.format(s))
        _same(F.contiguous(), out.raw.F_dec[s].permute(0, 3, 1, 2).contiguous(), 'get_P F[{}]'.format(s))
        Pp, Fp = net.get_P(s, bn_q, prev)
        _same(P.contiguous(), Pp.contiguous(), 'P vs MultiscaleNetwork.get_P')
        _same(F.contiguous(), Fp.contiguous(), 'F vs MultiscaleNetwork.get_P')
        if prev is not None:       # the same decoder without the fused features
            P0, F0 = nn.get_P(s, bn_q, None)
            Pp0, Fp0 = net.get_P(s, bn_q, None)
            _same(P0.contiguous(), Pp0.contiguous(), 'P without fuse')
            _same(F0.contiguous(), Fp0.contiguous(), 'F without fuse')


def test_native_get_P_of_the_rgb_shared_baseline_with_auto_recurse():
    net = blueprint('cr_rgb_shared').net
    nn = native('cr_rgb_shared')
    img = gen.rgb_case().float().cuda()
    out = net.forward(img, auto_recurse=3)
    n_total = len(out.raw.P)
    assert n_total == 4
    prev_native = prev_py = None
    for s in reversed(range(n_total)):
        bn_q = out.raw.bn_q[s + 1]
        P, F = nn.get_P(s, bn_q, prev_native, n_scales_total=n_total)
        Pp, Fp = net.get_P(s, bn_q, prev_py, n_scales_total=n_total)
        _same(P.contiguous(), out.P[s].contiguous(), 'rgb get_P vs forward P[{}]'.format(s))
        _same(F.contiguous(), out.raw.F_dec[s].permute(0, 3, 1, 2).contiguous(), 'rgb get_P vs forward F[{}]'.format(s))
        _same(P.contiguous(), Pp.contiguous(), 'rgb get_P vs MultiscaleNetwork.get_P')
        prev_native, prev_py = F, Fp


def test_encode_batch_on_the_native_forward_writes_the_committed_file():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    bp = blueprint('cr', True)
    img = gen.l3c_case()
    data = Bitcoding(bp).encode_batch(img, out=native('cr', True).forward(img.float().cuda())).to_bytes()[0]
    assert data == open(os.path.join(GOLDEN, 'hip_l3c_cal_64x96.l3c'), 'rb').read()


def test_workspace_contents_streams_and_a_shared_packed_buffer():
    nn = native('cr')
    x = _image(2, 136, 200, seed=3)
    ref = nn.forward(x)
    # a workspace full of NaNs beforehand
    ws = torch.full((nn.forward_workspace_bytes(2, 136, 200),), 0xFF, dtype=torch.uint8, device='cuda')
    _assert_forward_equal(nn.forward(x, workspace=ws), ref, 'NaN workspace: ')
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = nn.forward(x)
    torch.cuda.current_stream().wait_stream(side)
    _assert_forward_equal(got, ref, 'side stream: ')
    # two forwards in flight on two streams, one packed buffer, separate workspaces and outputs
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    x2 = _image(2, 136, 200, seed=4)
    ref2 = nn.forward(x2)
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        a = nn.forward(x)
    with torch.cuda.stream(s2):
        b = nn.forward(x2)
    torch.cuda.current_stream().wait_stream(s1)
    torch.cuda.current_stream().wait_stream(s2)
    _assert_forward_equal(a, ref, 'stream 1: ')
    _assert_forward_equal(b, ref2, 'stream 2: ')


def test_workspace_plus_outputs_within_the_python_forward_peak():
    net = blueprint('cr').net
    nn = native('cr')
    B, H, W = 4, 512, 768
    x = _image(B, H, W, seed=11)
    net.forward(x[:1, :, :64, :64])          # weights packed outside the measurement
    torch.cuda.synchronize()

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del out
        return p

    py = peak(lambda: net.forward(x))
    cfg = net.config_ms
    S, C = cfg.num_scales, cfg.q.C
    outputs = B * 3 * H * W * 2 + sum(B * C * (H >> (s + 1)) * (W >> (s + 1)) * (2 + 4) + B * (H >> s) * (W >> s) * nn.kp(s) * 4
                                      for s in range(S))
    ws = nn.forward_workspace_bytes(B, H, W)
    assert ws + outputs <= py, (ws, outputs, py)
    measured = peak(lambda: nn.forward(x, features=False))    # (+ Out.S as int64, as the Python forward holds too)
    assert measured <= py, (measured, py)


def _write_weights(path, nn, sd):
    from l3c_pytorch_amd.native_net import param_schema
    import struct
    names = param_schema(nn.cfg)
    with open(path, 'wb') as f:
        f.write(b'L3CW' + struct.pack('<I', len(names)))
        for name, shape in names:
            t = sd[name].detach().cpu().float().contiguous().numpy()
            assert tuple(t.shape) == shape
            f.write(struct.pack('<I', len(name)) + name.encode() + struct.pack('<I', len(shape)))
            f.write(np.asarray(shape, dtype=np.int64).tobytes() + t.astype(np.float32).tobytes())


@pytest.mark.parametrize('calibrated', [False, True])
def test_a_caller_without_torch_reproduces_the_committed_hashes(record, tmp_path, calibrated):
    """tests/cabi/net_forward_main.cpp: l3c_hip.h + libl3c_hip.so + the HIP runtime, run as a child process."""
    exe = tmp_path / 'net_forward_main'
    libdir = os.path.join(ROOT, 'l3c-pytorch_amd', 'csrc')
    subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'net_forward_main.cpp'), '-L', libdir, '-ll3c_hip', '-Wl,-rpath,' + libdir,
                    '-o', str(exe)], check=True, timeout=180)
    nn = native('cr', calibrated)
    _write_weights(str(tmp_path / 'w.bin'), nn, blueprint('cr', calibrated).net.state_dict())
    img = gen.l3c_case().float().numpy()
    B, _, H, W = img.shape
    with open(tmp_path / 'img.bin', 'wb') as f:
        f.write(np.asarray([B, H, W], dtype=np.int64).tobytes() + np.ascontiguousarray(img, dtype=np.float32).tobytes())
    c = nn.cfg
    args = [str(v) for v in (c.num_scales, c.Cf, c.C, c.L, c.K, c.enc_blocks, c.dec_blocks, c.rgb_baseline, c.dec_skip)]
    r = subprocess.run([str(exe), str(tmp_path / 'w.bin'), str(tmp_path / 'img.bin'), str(tmp_path)] + args,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = record['forward_64x96']['calibrated' if calibrated else 'default']
    S = []
    for s in range(c.num_scales + 1):
        S.append(gen.sha(np.fromfile(str(tmp_path / 'sym{}.bin'.format(s)), dtype=np.int16)))
    P = []
    for s in range(c.num_scales):
        p = np.fromfile(str(tmp_path / 'P{}.bin'.format(s)), dtype=np.float32).reshape(B, H >> s, W >> s, nn.kp(s))
        P.append(gen.sha(np.ascontiguousarray(p.transpose(0, 3, 1, 2))))
    assert S == want['S']
    assert P == want['P']
