"""-m gpu: the thin kernels of csrc/conv_small.hip against fp64 (tests/ref64.py) with DERIVED bounds -- n roundings * 2^-24 * sum |terms|,
elementwise, no tuned constant -- at the shapes where their loops change shape: a ragged last tile, tiles straddling two images, the
prefetching grid-stride loop of the to_q tile kernel (> 512 tiles), the direct kernel (Cf > 64), Cf < 64, the grid-stride loops of
dec_head and sym_to_bn; outputs poisoned before the launch; a batch equal, bit for bit, to its images launched one by one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ref64  # noqa: E402

CS = (1, 3, 5, 8)
LS = (2, 25, 256)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _within(got, val, bound, what):
    err = np.abs(got.astype(np.float64) - val)
    assert np.isfinite(got).all(), what
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print('{}: max error / bound = {:.3f} (max error {:.3g})'.format(what, ratio, err.max()))
    assert (err <= bound).all(), (what, ratio)


# ---- to_q + quantiser -------------------------------------------------------------------------------------------------------------


def _to_q(feat, w, b, levels):
    """l3c_to_q_quantize into poisoned outputs: sym -7, bn_q and bn NaN.  feat (B, H, W, Cf) on the device."""
    from l3c_pytorch_amd import _lib, ops
    Bn, H, W, Cf = feat.shape
    C, L = w.shape[0], levels.shape[0]
    sym = torch.full((Bn, C, H, W), -7, dtype=torch.int16, device='cuda')
    bn_q = torch.full((Bn, C, H, W), float('nan'), dtype=torch.float32, device='cuda')
    bn = torch.full((Bn, C, H, W), float('nan'), dtype=torch.float32, device='cuda')
    _lib.call('l3c_to_q_quantize', ops.ptr(feat, torch.float32), ops.ptr(w), ops.ptr(b), ops.ptr(levels), Bn, H * W, Cf, C, L, ops.ptr(sym),
              ops.ptr(bn_q), ops.ptr(bn), ops.stream())
    return sym.cpu().numpy(), bn_q.cpu().numpy(), bn.cpu().numpy()


TO_Q_SHAPES = [(1, 1, 1), (1, 15, 17), (1, 16, 16), (1, 1, 257), (3, 9, 29), (2, 256, 257)]
TO_Q_CASES = [(shape, Cf, CS[(i + j) % 4], LS[(i + 2 * j + (i + j) // 4) % 3])
              for i, shape in enumerate(TO_Q_SHAPES) for j, Cf in enumerate((16, 32, 64, 128))]


def test_to_q_cases_cover_every_C_and_L_with_both_kernels():
    for tile in (True, False):
        seen = {(C, L) for _, Cf, C, L in TO_Q_CASES if (Cf <= 64) == tile}
        assert {c for c, _ in seen} == set(CS) and {l for _, l in seen} == set(LS), seen
    assert {(C, L) for _, _, C, L in TO_Q_CASES} == {(c, l) for c in CS for l in LS}


@pytest.mark.parametrize('shape,Cf,C,L', TO_Q_CASES)
def test_to_q_quantize_vs_fp64(shape, Cf, C, L):
    """Cf <= 64: the tile kernel (256-pixel tiles; 1x257 and 15x17 end in a ragged tile, 3x9x29 has tiles straddling images, 2x256x257 is
    514 tiles on 512 blocks: the prefetch loop, and a ragged end); Cf 128: the direct kernel.  bn within (Cf + 1) * 2^-24 * (sum |f w| + |b|);
    sym and bn_q EQUAL to the reference quantiser applied to the kernel's own bn; every output element written; batch-invariant."""
    Bn, H, W = shape
    rng = np.random.RandomState(Cf * 1000 + H * 10 + W + C)
    feat = rng.randn(Bn, Cf, H, W).astype(np.float32)
    w = (rng.randn(C, Cf) * 0.6 / np.sqrt(Cf)).astype(np.float32)
    b = (rng.randn(C) * 0.1).astype(np.float32)
    levels = np.linspace(-1, 1, L).astype(np.float32)
    fd, wd, bd, ld = _dev(_nhwc(feat)), _dev(w), _dev(b), _dev(levels)
    assert fd.data_ptr() % 16 == 0
    sym, bn_q, bn = _to_q(fd, wd, bd, ld)
    val, bound = ref64.conv1x1_64(feat, w, b)
    _within(bn, val, bound, 'to_q {} Cf {} C {} L {}'.format(shape, Cf, C, L))
    want_sym, want_q = ref64.quantise_argmin(bn, levels)
    assert sym.min() >= 0 and np.array_equal(sym.astype(np.int64), want_sym)
    assert bn_q.tobytes() == want_q.tobytes()
    assert Bn * H * W < 100 or len(np.unique(sym)) > min(L, 20) // 2          # (the inputs spread over the levels)
    for i in range(Bn if Bn > 1 else 0):
        s1, q1, b1 = _to_q(fd[i:i + 1].contiguous(), wd, bd, ld)
        assert np.array_equal(s1[0], sym[i]) and q1[0].tobytes() == bn_q[i].tobytes() and b1[0].tobytes() == bn[i].tobytes(), i


@pytest.mark.parametrize('Cf', [16, 64, 128])
@pytest.mark.parametrize('L', LS)
def test_to_q_level_ties_resolve_to_the_lower_index(Cf, L):
    """bn exactly half way between two adjacent levels (zero weights, the midpoint as bias): where the two fp32 squared distances are equal
    the lower index wins, as torch.min; everywhere the reference quantiser's answer."""
    levels = np.linspace(-1, 1, L).astype(np.float32)
    C = min(8, L - 1)
    pairs = np.linspace(0, L - 2, C).astype(np.int64)
    mid = ((levels[pairs].astype(np.float64) + levels[pairs + 1]) / 2).astype(np.float32)
    feat = np.random.RandomState(L).randn(2, 5, 7, Cf).astype(np.float32)
    sym, bn_q, bn = _to_q(_dev(feat), _dev(np.zeros((C, Cf), dtype=np.float32)), _dev(mid), _dev(levels))
    assert (bn == mid.reshape(1, C, 1, 1)).all()
    want_sym, want_q = ref64.quantise_argmin(bn, levels)
    assert np.array_equal(sym.astype(np.int64), want_sym) and bn_q.tobytes() == want_q.tobytes()
    tie = np.square(mid - levels[pairs], dtype=np.float32) == np.square(mid - levels[pairs + 1], dtype=np.float32)
    assert tie.any()
    assert (sym[:, tie] == pairs[tie].reshape(1, -1, 1, 1)).all()


@pytest.mark.parametrize('Cf', [16, 64, 128])
def test_to_q_refuses_a_misaligned_feat(Cf):
    """l3c_to_q_quantize (csrc/conv_small.hip): `feat` must be 16-byte aligned -- both kernels read it with 16-byte loads, and the entry used
    to send a misaligned one to the direct kernel.  L3C_ERR_INVALID_ARG, nothing launched: the poisoned outputs stay as they were."""
    from l3c_pytorch_amd import _lib, ops
    Bn, HW, C, L = 2, 40, 5, 25
    buf = torch.randn(Bn * HW * Cf + 1, device='cuda')
    feat = buf[1:]
    assert feat.is_contiguous() and feat.data_ptr() % 16 == 4
    w, b, levels = torch.randn(C, Cf, device='cuda'), torch.randn(C, device='cuda'), torch.linspace(-1, 1, L, device='cuda')
    sym = torch.full((Bn, C, HW), -7, dtype=torch.int16, device='cuda')
    bn_q = torch.full((Bn, C, HW), float('nan'), dtype=torch.float32, device='cuda')
    bn = torch.full((Bn, C, HW), float('nan'), dtype=torch.float32, device='cuda')
    rc = _lib.load().l3c_to_q_quantize(ops.ptr(feat), ops.ptr(w), ops.ptr(b), ops.ptr(levels), Bn, HW, Cf, C, L, ops.ptr(sym), ops.ptr(bn_q),
                                       ops.ptr(bn), ops.stream())
    torch.cuda.synchronize()
    assert rc == -1, rc                                                    # L3C_ERR_INVALID_ARG
    assert b'aligned' in _lib.load().l3c_last_error()
    assert (sym == -7).all() and torch.isnan(bn_q).all() and torch.isnan(bn).all()
    with pytest.raises(_lib.L3CError):
        ops.to_q_quantize(feat.view(Bn, 5, 8, Cf), w, b, levels)


# ---- decoder head -----------------------------------------------------------------------------------------------------------------


def _dec_head(bn_q, w, b, fuse):
    from l3c_pytorch_amd import _lib, ops
    Bn, C, H, W = bn_q.shape
    Cf = w.shape[0]
    out = torch.full((Bn, H, W, Cf), float('nan'), dtype=torch.float32, device='cuda')
    _lib.call('l3c_dec_head', ops.ptr(bn_q, torch.float32), ops.ptr(w), ops.ptr(b), ops.ptr(fuse) if fuse is not None else None, Bn, H * W, C,
              Cf, ops.ptr(out), ops.stream())
    return out.cpu().numpy()


DEC_HW = [(1, 1), (3, 5), (4, 4), (1, 17), (9, 14), (200, 200)]       # HW 1, 15, 16, 17, 126, 40000 (the last grid-strides: > 2048 blocks' worth)
DEC_CASES = [(hw, Cf, CS[(i + j) % 4]) for i, hw in enumerate(DEC_HW) for j, Cf in enumerate((16, 64, 128, 256))]


@pytest.mark.parametrize('hw,Cf,C', DEC_CASES)
def test_dec_head_vs_fp64(hw, Cf, C):
    """1x1 conv C -> Cf on the quantised bottleneck, with and without the fused coarser features: within (C + 1 [+ 1]) * 2^-24 * (sum |v w| +
    |b| [+ |fuse|]); every output element written; B = 3 equals three single launches."""
    H, W = hw
    Bn = 3
    rng = np.random.RandomState(Cf + H * W + C)
    levels = np.linspace(-1, 1, 25).astype(np.float32)
    bn_q = levels[rng.randint(0, 25, size=(Bn, C, H, W))]
    w = (rng.randn(Cf, C) / np.sqrt(C)).astype(np.float32)
    b = rng.randn(Cf).astype(np.float32)
    fuse = rng.randn(Bn, Cf, H, W).astype(np.float32)
    qd, wd, bd, fd = _dev(bn_q), _dev(w), _dev(b), _dev(_nhwc(fuse))
    for f_host, f_dev in ((fuse, fd), (None, None)):
        got = _dec_head(qd, wd, bd, f_dev)
        val, bound = ref64.dec_head64(bn_q, w, b, f_host)
        _within(got, _nhwc(val), _nhwc(bound), 'dec_head {}x{} Cf {} C {} fuse {}'.format(H, W, Cf, C, f_host is not None))
        for i in range(Bn):
            one = _dec_head(qd[i:i + 1].contiguous(), wd, bd, f_dev[i:i + 1].contiguous() if f_dev is not None else None)
            assert one[0].tobytes() == got[i].tobytes(), i


# ---- RGB head ---------------------------------------------------------------------------------------------------------------------


def _rgb_head(img, w1, b1, w2, b2, w3, b3):
    from l3c_pytorch_amd import _lib, ops
    Bn, _, H, W = img.shape
    Cf = w3.shape[0]
    out = torch.full((Bn, H, W, Cf), float('nan'), dtype=torch.float32, device='cuda')
    shifted = torch.full((Bn, 3, H, W), float('nan'), dtype=torch.float32, device='cuda')
    _lib.call('l3c_rgb_head', ops.ptr(img, torch.float32), ops.ptr(w1), ops.ptr(b1), ops.ptr(w2), ops.ptr(b2), ops.ptr(w3), ops.ptr(b3), Bn, H, W,
              Cf, ops.ptr(out), ops.ptr(shifted), ops.stream())
    return out.cpu().numpy(), shifted.cpu().numpy()


@pytest.mark.parametrize('Cf', [16, 64, 128])
@pytest.mark.parametrize('H,W', [(1, 1), (8, 32), (9, 33), (33, 31), (70, 100), (129, 40)])
def test_rgb_head_vs_fp64(H, W, Cf):
    """sub_rgb_mean -> MeanShift -> conv3x3 3 -> Cf at one pixel, exactly one 8x32 tile, a tile plus one row and column, more than the four
    tiles a block walks down its column (33, 70, 129 rows): the mean-shifted image and the features within the bounds of ref64.rgb_head64
    (4 roundings per 3 -> 3 map, 28 for the 27 fused multiply-adds and the bias, the earlier stage's error carried through |w|)."""
    Bn = 3
    rng = np.random.RandomState(Cf + H * 7 + W)
    img = rng.randint(0, 256, size=(Bn, 3, H, W)).astype(np.float32)
    img[0, :, 0, 0], img[-1, :, -1, -1] = 255, 0
    mean = np.array([0.4488, 0.4371, 0.4040]) * 255
    w1 = (np.eye(3) + rng.randn(3, 3) * 0.01).astype(np.float32)
    b1 = (-mean).astype(np.float32)
    w2 = ((np.eye(3) + rng.randn(3, 3) * 0.01) / 128).astype(np.float32)
    b2 = (rng.randn(3) * 0.01).astype(np.float32)
    w3 = (rng.randn(Cf, 3, 3, 3) / np.sqrt(27)).astype(np.float32)
    b3 = rng.randn(Cf).astype(np.float32)
    dev = [_dev(a) for a in (img, w1, b1, w2, b2, w3, b3)]
    out, shifted = _rgb_head(*dev)
    z, ez, val, bound = ref64.rgb_head64(img, w1, b1, w2, b2, w3, b3)
    _within(shifted, z, ez, 'rgb_head shifted {}x{} Cf {}'.format(H, W, Cf))
    _within(out, _nhwc(val), _nhwc(bound), 'rgb_head out {}x{} Cf {}'.format(H, W, Cf))
    for i in range(Bn):
        o1, s1 = _rgb_head(dev[0][i:i + 1].contiguous(), *dev[1:])
        assert o1[0].tobytes() == out[i].tobytes() and s1[0].tobytes() == shifted[i].tobytes(), i


# ---- bicubic pyramid step ---------------------------------------------------------------------------------------------------------


def _tie_inputs(k, mean):
    """fp32 x with fl32(x + mean) == k + 0.5 exactly (x = fl32(k + .5 - mean), nudged by an ulp where the sum rounds elsewhere)."""
    want = (k + 0.5).astype(np.float32)
    x = (want - mean).astype(np.float32)
    for _ in range(4):
        s = (x + mean).astype(np.float32)
        x = np.where(s < want, np.nextafter(x, np.float32(np.inf)), np.where(s > want, np.nextafter(x, np.float32(-np.inf)), x)).astype(np.float32)
    return x


@pytest.mark.parametrize('H,W', [(32, 48), (37, 51)])
def test_bicubic_encoder_rounds_ties_to_even_and_clamps(H, W):
    """to_u8_kernel: x + mean -> clamp(0, 255) -> round half to EVEN.  Inputs whose x + mean is exactly k + 0.5 in fp32, for even and odd k
    (0.5 -> 0, 1.5 -> 2, 254.5 -> 254), inputs below 0 and above 255 (255.5 clamps before it rounds).  The uint8 image is what
    torch.round of the clamp gives; from there Pillow, as tests/test_gpu_net.py."""
    from PIL import Image
    from l3c_pytorch_amd import ops
    rng = np.random.RandomState(H)
    mean = torch.tensor([0.4488, 0.4371, 0.4040]).mul(255.).reshape(1, 3, 1, 1)
    m = mean.numpy()
    k = rng.randint(0, 255, size=(2, 3, H, W))
    k[0, :, 0, :8] = np.array([0, 1, 2, 3, 253, 254, 128, 127])
    x = _tie_inputs(k, m)
    off = rng.uniform(size=k.shape)
    off[0, :, 0, :8] = off[1, :, 0, :4] = 0.5                                          # (the hand-picked values stay)
    x = np.where(off < 0.05, (rng.uniform(-40, -0.01, size=k.shape) - m), x)            # below 0
    x = np.where(off > 0.95, (rng.uniform(255.01, 300, size=k.shape) - m), x)          # above 255
    x = x.astype(np.float32)
    x[1, :, 0, :4] = (np.array([255.5, 256.5, -0.5, -1.5], dtype=np.float32).reshape(1, 4) - m.reshape(3, 1)).astype(np.float32)
    xt = torch.from_numpy(x)
    s = (xt + mean)
    ties = (s - s.floor()) == 0.5
    inside = ties & (s > 0) & (s < 255)
    assert ties.float().mean() > 0.8 and (s < 0).any() and (s > 255).any()
    assert (inside & (s.floor() % 2 == 0)).sum() > 100 and (inside & (s.floor() % 2 == 1)).sum() > 100
    bn, sym = ops.bicubic_encoder(xt.cuda().contiguous())
    ref_u8 = s.clamp(0, 255.).round().to(torch.uint8)
    assert ref_u8[0, 0, 0, :6].tolist() == [0, 2, 2, 4, 254, 254]
    for n in range(2):
        ref = np.array(Image.fromarray(ref_u8[n].permute(1, 2, 0).numpy()).resize((int(W * 0.5), int(H * 0.5)), Image.BICUBIC))
        assert np.array_equal(sym[n].cpu().numpy().transpose(1, 2, 0), ref), (H, W)
    assert torch.equal(bn.cpu(), sym.cpu().float() - mean)


def test_to_u8_alone_on_ties_and_clamps():
    """The rounding kernel by itself (l3c_rgb_to_u8), so that a wrong tie cannot hide in the resampling that follows."""
    from l3c_pytorch_amd import _lib, ops
    mean = torch.tensor([0.4488, 0.4371, 0.4040]).mul(255.).reshape(1, 3, 1, 1)
    k = np.tile(np.arange(-2, 258).reshape(1, 1, 1, -1), (2, 3, 3, 1))
    x = torch.from_numpy(_tie_inputs(k, mean.numpy()))
    s = x + mean
    assert ((s - s.floor()) == 0.5).all()
    u8 = torch.full((2, 3, 3, 260), 77, dtype=torch.uint8, device='cuda')
    _lib.call('l3c_rgb_to_u8', ops.ptr(x.cuda().contiguous(), torch.float32), ops.rgb_mean(), 2, 3 * 260, ops.ptr(u8), ops.stream())
    assert torch.equal(u8.cpu(), s.clamp(0, 255.).round().to(torch.uint8))


# ---- sym -> bn --------------------------------------------------------------------------------------------------------------------


def test_sym_to_bn_grid_stride_bit_exact():
    """n = 2 200 000 > 8192 blocks * 256 threads: the grid-stride loop; bit-equal to quantizer.to_bn (a multiplication and an addition,
    each rounded)."""
    from l3c_pytorch_amd import ops
    from l3c_pytorch_amd.modules import quantizer
    n = 2200000
    assert n > 8192 * 256
    sym = torch.from_numpy(np.random.RandomState(0).randint(0, 25, size=n).astype(np.int16))
    got = ops.sym_to_bn(sym.cuda(), 2 / 24, -1).cpu()
    assert got.numpy().tobytes() == quantizer.to_bn(sym, -1, 1, 25).numpy().tobytes()
    sym = torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=n).astype(np.int16))
    assert torch.equal(ops.sym_to_bn(sym.cuda(), 1.0, 0).cpu(), quantizer.to_bn(sym, 0, 255, 256))
