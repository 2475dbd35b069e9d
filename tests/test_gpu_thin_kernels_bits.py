"""-m gpu: the three streaming kernels of csrc/conv_small.hip (rgb_head, to_q tile, dec_head) against their predecessors, which the
TEST-ONLY library keeps with their text unchanged (csrc/xcheck_small.hip, include/l3c_xcheck_small.h): every output equal bit for
bit (compared as integers: -0.0 is not +0.0 here), over the whole output.  Every output lies inside a larger buffer filled with a
sentinel, and the margins on both sides must still hold it afterwards.

Shapes: one pixel, every tail shorter than a thread's pixel group (dec_head: 4 pixels, rgb_head: a pixel pair, to_q: a 256-pixel tile),
one size past a block's span; rgb_head tiles that cross the right and the bottom border; dec_head on a bottleneck whose base is one
float off 16-byte alignment (the scalar-load path at an HW that would otherwise take the 16-byte one); a to_q input on which two levels
tie exactly (the first must win)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN = 64          # elements on either side of an output
F_SENTINEL = -12345.0
I_SENTINEL = -7


def _guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * MARGIN,), I_SENTINEL if dtype == torch.int16 else F_SENTINEL, dtype=dtype, device='cuda')
    return buf, buf[MARGIN:MARGIN + n].view(shape)


def _margins_untouched(buf, what):
    sentinel = I_SENTINEL if buf.dtype == torch.int16 else F_SENTINEL
    assert bool((buf[:MARGIN] == sentinel).all()) and bool((buf[-MARGIN:] == sentinel).all()), what + ': wrote outside its output'


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, what):
    _margins_untouched(got[0], what + ' (product)')
    _margins_untouched(want[0], what + ' (predecessor)')
    assert torch.equal(_bits(got[1]), _bits(want[1])), what


def _gen(seed):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return g


# ---- decoder head -----------------------------------------------------------------------------------------------------------------


def _dec_head(product, bn_q, w, b, fuse, Bn, HW, C, Cf):
    from l3c_pytorch_amd import _lib, ops
    buf, out = _guarded((Bn, HW, Cf), torch.float32)
    args = (bn_q.data_ptr(), ops.ptr(w), ops.ptr(b), ops.ptr(fuse) if fuse is not None else None, Bn, HW, C, Cf, ops.ptr(out), ops.stream())
    if product:
        _lib.call('l3c_dec_head', *args)
    else:
        _lib.call_xcheck('l3c_xcheck_dec_head', *args)
    return buf, out


def _dec_inputs(Bn, HW, C, Cf, offset=0):
    g = _gen(1000 * HW + 10 * C + Cf + Bn)
    levels = torch.linspace(-1, 1, 25)
    store = torch.zeros(Bn * C * HW + offset)
    store[offset:] = levels[torch.randint(0, 25, (Bn * C * HW,), generator=g)]
    store = store.cuda()
    bn_q = store[offset:]                                                # base pointer `offset` floats past a 16-byte boundary
    w = (torch.randn(Cf, C, generator=g) / C ** 0.5).cuda()
    b = torch.randn(Cf, generator=g).cuda()
    fuse = torch.randn(Bn, HW, Cf, generator=g).cuda()
    return store, bn_q, w, b, fuse


@pytest.mark.parametrize('HW', [1, 3, 5, 63, 64, 65, 4099])
@pytest.mark.parametrize('Bn', [1, 3])
def test_dec_head_bits(Bn, HW):
    for C, Cf in itertools.product((1, 5, 8), (16, 64)):
        _, bn_q, w, b, fuse = _dec_inputs(Bn, HW, C, Cf)
        assert bn_q.data_ptr() % 16 == 0
        for f in (fuse, None):
            what = 'dec_head B {} HW {} C {} Cf {} fuse {}'.format(Bn, HW, C, Cf, f is not None)
            _same(_dec_head(True, bn_q, w, b, f, Bn, HW, C, Cf), _dec_head(False, bn_q, w, b, f, Bn, HW, C, Cf), what)


def test_dec_head_bits_unaligned_bottleneck():
    """HW % 4 == 0 but the bottleneck starts one float past a 16-byte boundary: no 16-byte loads of it."""
    Bn, HW, C, Cf = 3, 64, 5, 64
    _, bn_q, w, b, fuse = _dec_inputs(Bn, HW, C, Cf, offset=1)
    assert bn_q.data_ptr() % 16 == 4
    for f in (fuse, None):
        _same(_dec_head(True, bn_q, w, b, f, Bn, HW, C, Cf), _dec_head(False, bn_q, w, b, f, Bn, HW, C, Cf), 'dec_head unaligned fuse {}'.format(f is not None))


# ---- RGB head ---------------------------------------------------------------------------------------------------------------------


def _rgb_head(product, t, Bn, H, W, Cf, want_shifted):
    from l3c_pytorch_amd import _lib, ops
    obuf, out = _guarded((Bn, H, W, Cf), torch.float32)
    sbuf, shifted = _guarded((Bn, 3, H, W), torch.float32)
    args = tuple(ops.ptr(a) for a in t) + (Bn, H, W, Cf, ops.ptr(out), ops.ptr(shifted) if want_shifted else None, ops.stream())
    if product:
        _lib.call('l3c_rgb_head', *args)
    else:
        _lib.call_xcheck('l3c_xcheck_rgb_head', *args)
    return (obuf, out), (sbuf, shifted)


@pytest.mark.parametrize('H,W', [(1, 1), (8, 32), (9, 33), (33, 65), (40, 70)])
@pytest.mark.parametrize('Bn', [1, 2])
def test_rgb_head_bits(Bn, H, W):
    for Cf, want_shifted in itertools.product((16, 64), (True, False)):
        g = _gen(H * 1000 + W * 10 + Cf + Bn)
        img = torch.randint(0, 256, (Bn, 3, H, W), generator=g).float()
        mean = torch.tensor([0.4488, 0.4371, 0.4040]) * 255
        w1 = torch.eye(3) + torch.randn(3, 3, generator=g) * 0.01
        w2 = (torch.eye(3) + torch.randn(3, 3, generator=g) * 0.01) / 128
        b2 = torch.randn(3, generator=g) * 0.01
        w3 = torch.randn(Cf, 3, 3, 3, generator=g) / 27 ** 0.5
        b3 = torch.randn(Cf, generator=g)
        t = [a.contiguous().cuda() for a in (img, w1, -mean, w2, b2, w3, b3)]
        what = 'rgb_head B {} {}x{} Cf {} shifted {}'.format(Bn, H, W, Cf, want_shifted)
        (got_o, got_s), (want_o, want_s) = _rgb_head(True, t, Bn, H, W, Cf, want_shifted), _rgb_head(False, t, Bn, H, W, Cf, want_shifted)
        _same(got_o, want_o, what + ': out')
        if want_shifted:
            _same(got_s, want_s, what + ': shifted_out')
        else:                                                            # absent: not a byte of the buffer it was not given
            assert bool((got_s[0] == F_SENTINEL).all()), what


# ---- to_q + quantiser -------------------------------------------------------------------------------------------------------------


def _to_q(product, feat, w, b, levels, Bn, HW, Cf, C, L, want_bn):
    from l3c_pytorch_amd import _lib, ops
    sym, bn_q, bn = _guarded((Bn, C, HW), torch.int16), _guarded((Bn, C, HW), torch.float32), _guarded((Bn, C, HW), torch.float32)
    args = (ops.ptr(feat), ops.ptr(w), ops.ptr(b), ops.ptr(levels), Bn, HW, Cf, C, L, ops.ptr(sym[1]), ops.ptr(bn_q[1]),
            ops.ptr(bn[1]) if want_bn else None, ops.stream())
    if product:
        _lib.call('l3c_to_q_quantize', *args)
    else:
        _lib.call_xcheck('l3c_xcheck_to_q_quantize', *args)
    return sym, bn_q, bn


def _to_q_same(feat, w, b, levels, Bn, HW, Cf, C, L, want_bn, what):
    got, want = _to_q(True, feat, w, b, levels, Bn, HW, Cf, C, L, want_bn), _to_q(False, feat, w, b, levels, Bn, HW, Cf, C, L, want_bn)
    _same(got[0], want[0], what + ': sym')
    _same(got[1], want[1], what + ': bn_q')
    if want_bn:
        _same(got[2], want[2], what + ': bn')
    else:
        assert bool((got[2][0] == F_SENTINEL).all()), what
    return got


@pytest.mark.parametrize('HW', [1, 255, 256, 257, 1000])
@pytest.mark.parametrize('Bn', [1, 2])
def test_to_q_bits(Bn, HW):
    for Cf, C, L, want_bn in itertools.product((32, 64), (1, 5, 8), (2, 25), (True, False)):
        g = _gen(HW * 100 + Cf + C * 7 + L + Bn)
        feat = torch.randn(Bn, HW, Cf, generator=g).cuda()
        w = (torch.randn(C, Cf, generator=g) / Cf ** 0.5).cuda()
        b = (torch.randn(C, generator=g) * 0.1).cuda()
        levels = torch.linspace(-1, 1, L).cuda()
        _to_q_same(feat, w, b, levels, Bn, HW, Cf, C, L, want_bn, 'to_q B {} HW {} Cf {} C {} L {} bn {}'.format(Bn, HW, Cf, C, L, want_bn))


def test_to_q_bits_exact_tie_first_level_wins():
    """Integer levels -12 .. 12, zero weights, bias k + 0.5: channel k sits exactly between two levels at every pixel, both distances are
    0.25 in fp32, and the lower index must be kept."""
    Bn, HW, Cf, C, L = 2, 257, 64, 5, 25
    feat = torch.randn(Bn, HW, Cf, generator=_gen(5)).cuda()
    w = torch.zeros(C, Cf).cuda()
    b = (torch.arange(C).float() - 2 + 0.5).cuda()                       # -1.5 .. 2.5
    levels = (torch.arange(L).float() - 12).cuda()
    sym, bn_q, _ = _to_q_same(feat, w, b, levels, Bn, HW, Cf, C, L, True, 'to_q tie')
    for k in range(C):
        assert bool((sym[1][:, k] == 10 + k).all()) and bool((bn_q[1][:, k] == float(k - 2)).all()), k
