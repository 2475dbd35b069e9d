"""-m gpu: the channel slices of l3c_conv_desc.  Every conv entry may read its input from channels in_coff .. in_coff + Cin of a tensor with
in_cstride channels per pixel, take its residual from res_coff / res_cstride and write its output at out_coff / out_cstride
(include/l3c_hip.h), and every kernel has address arithmetic of its own for the three.  Each case runs one layer twice through
ops.conv(..., impl=...): DENSE, as tests/test_gpu_conv.py does, and SLICED, with input, residual and output each a slice of its own wide
NaN-filled tensor -- three different strides, three different offsets.  Slicing changes addresses and not arithmetic, so the two results
are compared bit for bit; the sliced one also against an fp64 reference that never sees the wide tensors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _embed(t, cstride, coff):
    """the NHWC tensor t as channels [coff, coff + C) of a freshly allocated (B, H, W, cstride) tensor filled with NaN"""
    B, H, W, C = t.shape
    assert coff + C <= cstride
    wide = torch.full((B, H, W, cstride), NAN, dtype=torch.float32, device='cuda')
    wide[..., coff:coff + C] = t
    return wide


def _nan_out(B, H, W, cstride):
    """a NaN-filled output of the given channel stride"""
    return torch.full((B, H, W, cstride), NAN, dtype=torch.float32, device='cuda')


# (stride - C, offset) of input, residual, output.  Layout 16: what the kernels with 16-byte loads and stores admit (multiples of 4);
# layout 4: the input as in layout 16 (every MFMA kernel loads it 16 bytes at a time), residual and output at odd strides and offsets
LAYOUT16 = ((12, 8), (20, 12), (8, 4))
LAYOUT4 = ((12, 8), (7, 5), (5, 3))
LAYOUT = {'wino4': LAYOUT16, 'wino2': LAYOUT16, 'wino4w': LAYOUT16, 'poly5': LAYOUT16, 'poly5x4': LAYOUT16,
          'gemm': LAYOUT4, 'direct': LAYOUT4, 'pw': LAYOUT4}
# the project's bounds against fp64 for unit-scale data (tests/test_gpu_conv.py): 3e-5, the polyphase forms 5e-5
BOUND = {'poly5': 5e-5, 'poly5x4': 5e-5}


def _bits(t):
    return t.view(torch.int32)


def _layer_and_data(KS, stride, dil, Cin, Cout, B, H, W, relu, res, shuffle):
    """-> (layer, x NHWC on the device, residual NHWC on the device or None, fp64 reference NHWC with the epilogue applied)"""
    from l3c_pytorch_amd import ops
    g = torch.Generator().manual_seed(KS * 100003 + dil * 10007 + Cin * 1009 + Cout * 101 + B * 53 + H * 7 + W)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KS, KS, generator=g) / np.sqrt(Cin * KS * KS)
    b = torch.randn(Cout, generator=g)
    layer = ops.PackedConv(w, b, stride=stride, dilation=dil)
    Ho, Wo = layer.out_hw(H, W)
    r = torch.randn(B, Cout, Ho, Wo, generator=g) if res else None
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=stride, dilation=dil, padding=KS // 2 if dil == 1 else dil)
    assert ref.shape[2:] == (Ho, Wo)
    if relu:
        ref = ref.clamp(min=0)
    if res:
        ref = ref + r.double()
    if shuffle:
        ref = F.pixel_shuffle(ref, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()   # noqa: E731
    return layer, nhwc(x).cuda(), nhwc(r).cuda() if res else None, nhwc(ref)


def _check_sliced(impl, KS, stride, dil, Cin, Cout, B, H, W, relu=False, res=False, shuffle=False, layout=None, dense_impl=None):
    """One layer dense and sliced through ops.conv(impl=...) (`impl` 'pw': the product's dispatch of a 1x1 layer): the five assertions of
    this module.  dense_impl: the kernel the dense launch is forced to when the sliced one goes through the dispatch (impl None).
    -> (largest deviation of the sliced output from fp64, the sliced output's own channels)"""
    from l3c_pytorch_amd import ops
    layer, x, r, ref = _layer_and_data(KS, stride, dil, Cin, Cout, B, H, W, relu, res, shuffle)
    force = None if impl == 'pw' else impl
    if impl == 'pw':
        assert layer.packed_pw is not None
    elif KS == 1:
        layer.packed_pw = None          # (set aside, as tests/test_gpu_conv.py does for the implicit-GEMM 1x1 kernels)
    (ipad, ioff), (rpad, roff), (opad, ooff) = layout or LAYOUT[impl]
    co = Cout // 4 if shuffle else Cout
    Bo, Ho, Wo, _ = ref.shape
    kw = dict(relu=relu, pixel_shuffle=shuffle)
    dense = ops.conv(x, layer, residual=r, impl=dense_impl if impl is None else force, **kw)
    assert dense.shape == ref.shape

    xw, rw = _embed(x, Cin + ipad, ioff), (_embed(r, Cout + rpad, roff) if res else None)
    x_before, r_before = xw.clone(), (rw.clone() if res else None)

    def sliced(first, end):
        ow = _nan_out(end - first, Ho, Wo, co + opad)
        ops.conv(xw[first:end], layer, out=ow, in_coff=ioff, out_coff=ooff, residual=rw[first:end] if res else None, res_coff=roff,
                 impl=force, **kw)
        # 3. no NaN inside the output slice, every element outside it still NaN
        own = ow[..., ooff:ooff + co]
        assert not bool(torch.isnan(own).any()), 'NaN inside the output slice'
        assert bool(torch.isnan(ow[..., :ooff]).all()) and bool(torch.isnan(ow[..., ooff + co:]).all()), 'write outside the output slice'
        return own

    own = sliced(0, B)
    # 1. within the project's bound of fp64, epilogue included
    err = (own.cpu().double() - ref).abs().max().item()
    bound = BOUND.get(dense_impl if impl is None else impl, 3e-5)
    print('SLICED {} k{} s{} d{} {}->{} {}x{}x{}{}{}{}: max |err| vs fp64 {:.3g} (bound {:g})'.format(
        impl, KS, stride, dil, Cin, Cout, B, H, W, ' relu' if relu else '', ' res' if res else '', ' shuffle' if shuffle else '', err, bound))
    assert err < bound, err
    # 2. bit-identical to the dense launch of the same kernel
    assert torch.equal(own, dense), 'sliced != dense: {} elements differ, max |diff| {:.3g}'.format(
        int((own != dense).sum()), (own - dense).abs().max().item())
    # 4. the wide input and residual are unchanged (as bits: NaN != NaN)
    assert torch.equal(_bits(xw), _bits(x_before)), 'the input tensor was written to'
    if res:                                 # ('poly5x4' accumulates in place, residual == out: it has no residual tensor of its own)
        assert torch.equal(_bits(rw), _bits(r_before)), 'the residual tensor was written to'
    # 5. image 1 of the batch == the single-image launch on its own slice
    if B > 1:
        assert torch.equal(sliced(1, 2), own[1:2]), 'image 1 of the batch != its single-image launch'
    return err, own


def _epi(name):
    return dict(relu='relu' in name, res='res' in name, shuffle='shuffle' in name)


# (dil, Cin, Cout, B, H, W, epilogue): the smallest shapes with interior tiles, ragged tiles and a masked last channel group
WINO4_CASES = [
    (1, 64, 64, 2, 21, 37, 'relu+res'),
    (1, 16, 120, 1, 17, 33, 'res'),          # Cout not a multiple of 16: the last wavefront's channel groups are masked
    (2, 64, 64, 2, 19, 37, 'res'),
    (4, 32, 64, 1, 21, 50, 'relu'),
    (4, 64, 64, 1, 3, 5, 'res'),             # image smaller than the dilation pattern
    (1, 64, 256, 2, 10, 18, 'shuffle'),
]


@pytest.mark.parametrize('tpb', [0, 2])
@pytest.mark.parametrize('dil,Cin,Cout,B,H,W,epi', WINO4_CASES)
def test_winograd_f4_on_channel_slices(dil, Cin, Cout, B, H, W, epi, tpb):
    """l3c_conv_wino4 (csrc/conv_wino4.hip): the input through a buffer descriptor at in + in_coff whose range check is the zero padding,
    the residual through r_rsrc / rcol_b / rrow_b, the output through o_rsrc -- with the block walking its tiles as the launch picks
    (0) and two at a time."""
    from l3c_pytorch_amd import _lib
    lib = _lib.load()
    prev = lib.l3c_conv_wino4_set_tiles_per_block(tpb)
    try:
        _check_sliced('wino4', 3, 1, dil, Cin, Cout, B, H, W, **_epi(epi))
    finally:
        lib.l3c_conv_wino4_set_tiles_per_block(prev)


@pytest.mark.parametrize('dil,Cin,Cout,B,H,W,epi', [(1, 64, 64, 2, 13, 45, 'res'), (2, 64, 64, 1, 19, 37, 'relu+res')])
def test_winograd_f2_on_channel_slices(dil, Cin, Cout, B, H, W, epi):
    """l3c_conv_wino of the cross-check library (csrc/conv_wino.hip) carries the same fields through code of its own"""
    _check_sliced('wino2', 3, 1, dil, Cin, Cout, B, H, W, **_epi(epi))


def test_winograd_f4_probe_on_channel_slices():
    """l3c_conv_wino4w of the cross-check library (csrc/conv_wino4w.hip): no residual"""
    _check_sliced('wino4w', 3, 1, 1, 64, 64, 2, 17, 33, relu=True)


@pytest.mark.parametrize('impl', ['poly5', 'poly5x4'])
@pytest.mark.parametrize('Cout,B,H,W', [(64, 2, 46, 70), (120, 1, 8, 6)])
def test_polyphase_5x5_on_channel_slices(impl, Cout, B, H, W):
    """5x5 stride 2 on the F(4x4,3x3) kernel: all four phases in one launch (l3c_conv_wino4_stride2), and as four phase launches that
    accumulate in place (l3c_conv_wino4_phase with residual == out at res_coff == out_coff: ops._conv_poly5)"""
    _check_sliced(impl, 5, 2, 1, 64, Cout, B, H, W)


GEMM_CASES = [
    # KS, stride, dil, Cin, Cout, B, H, W, epilogue
    (3, 1, 1, 64, 64, 2, 13, 45, 'relu+res'),
    (3, 1, 2, 64, 64, 1, 19, 37, 'res'),
    (3, 1, 4, 64, 64, 1, 21, 50, 'relu'),
    (3, 1, 1, 64, 256, 1, 10, 34, 'shuffle'),
    (5, 2, 1, 64, 64, 2, 22, 70, ''),
    (5, 2, 1, 64, 64, 1, 9, 7, ''),           # odd size
    (1, 1, 1, 192, 120, 1, 11, 33, ''),       # 1x1: the two-chunk LDS form (conv_lds_kernel<1, 1, 64, 2>)
    (1, 1, 1, 192, 150, 2, 5, 70, ''),        # 1x1: the other form (conv_mfma_kernel)
]


@pytest.mark.parametrize('KS,stride,dil,Cin,Cout,B,H,W,epi', GEMM_CASES)
def test_implicit_gemm_on_channel_slices(KS, stride, dil, Cin, Cout, B, H, W, epi):
    """l3c_conv_mfma (csrc/conv_mfma.hip: conv_lds_kernel, conv_mfma_kernel, each with its own size_t arithmetic) with residual and output
    at odd strides and offsets: 4-byte loads and stores"""
    _check_sliced('gemm', KS, stride, dil, Cin, Cout, B, H, W, **_epi(epi))


@pytest.mark.parametrize('KS,stride,dil,Cin,Cout,B,H,W,epi', [GEMM_CASES[1], GEMM_CASES[5]])
def test_direct_conv_on_channel_slices(KS, stride, dil, Cin, Cout, B, H, W, epi):
    """l3c_conv_direct (conv_direct_kernel, the plain-VALU cross-check of the product library)"""
    _check_sliced('direct', KS, stride, dil, Cin, Cout, B, H, W, **_epi(epi))


@pytest.mark.parametrize('Cin,Cout,B,H,W', [(192, 120, 1, 11, 33), (192, 150, 2, 5, 70), (64, 33, 1, 9, 15)])
def test_pointwise_conv_on_channel_slices(Cin, Cout, B, H, W):
    """l3c_conv_pw (csrc/conv_pw.hip: piece_off and a descriptor per pixel tile for the input, 4-byte stores at any output offset),
    reached through the product's dispatch of a 1x1 layer"""
    _check_sliced('pw', 1, 1, 1, Cin, Cout, B, H, W)


def test_dispatch_follows_the_slices():
    """ops.conv with impl=None: a 3x3 layer on slices the Winograd kernel admits runs on it; the same layer with an output (and residual)
    slice at an odd offset falls back to the implicit-GEMM kernel, and so does a 5x5 stride-2 layer that would otherwise take its
    polyphase form -- the two fallback branches of the dispatch.  Which kernel ran is read off the bits: Winograd and polyphase results
    differ from the implicit-GEMM kernel's in the last places."""
    from l3c_pytorch_amd import ops
    shape3, shape5 = (3, 1, 1, 64, 64, 2, 21, 37), (5, 2, 1, 64, 64, 1, 22, 70)
    # the kernels must be distinguishable on these layers, or the test could not tell which one ran
    layer, x, r, _ = _layer_and_data(*shape3, relu=True, res=True, shuffle=False)
    wino = ops.conv(x, layer, residual=r, relu=True, impl='wino4')
    gemm = ops.conv(x, layer, residual=r, relu=True, impl='gemm')
    assert not torch.equal(wino, gemm)
    assert torch.equal(ops.conv(x, layer, residual=r, relu=True), wino)              # dense: the Winograd kernel
    layer5, x5, _, _ = _layer_and_data(*shape5, relu=False, res=False, shuffle=False)
    assert not torch.equal(ops.conv(x5, layer5, impl='poly5'), ops.conv(x5, layer5, impl='gemm'))
    assert torch.equal(ops.conv(x5, layer5), ops.conv(x5, layer5, impl='poly5'))     # dense: the polyphase form

    _check_sliced(None, *shape3, relu=True, res=True, layout=LAYOUT16, dense_impl='wino4')
    _check_sliced(None, *shape3, relu=True, res=True, layout=LAYOUT4, dense_impl='gemm')
    _check_sliced(None, *shape5, layout=LAYOUT4, dense_impl='gemm')
    _check_sliced(None, *shape5, layout=LAYOUT16, dense_impl='poly5')
