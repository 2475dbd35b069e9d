"""Tensor-level wrappers of the HIP entry points (include/l3c_hip.h).  torch is only the owner of device memory and of
the current stream here; every function enqueues kernels from libl3c_hip.so and nothing else."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, call, ptr, stream

# Optional per-launch timing of the MFMA conv kernels (bench.py's roofline leg): when PROFILE is a list, every conv launch
# appends (kernel key, algorithmic FLOPs, algorithmic HBM bytes, start event, end event), the events being recorded on the launch
# stream.
PROFILE = None
PROFILE_DETAIL = bool(os.environ.get('L3C_PROFILE_DETAIL'))   # split the keys by layer shape (development)


# ---- convolution stack ------------------------------------------------------------------------------------------------
#
# ONE dispatch (no environment switches: encoder and decoder of a file must compute bit-identical P, so the kernel a layer runs on
# is a function of the layer and the tensors alone):
#   3x3 stride 1 (dilation 1, 2, 4), Cin % 16 == 0   -> Winograd F(4x4,3x3), csrc/conv_wino4.hip
#   5x5 stride 2, even input size                     -> four 3x3 polyphase convolutions in one launch of the same kernel
#   1x1, Cin % 64 == 0, Cout <= 160, bias only        -> pointwise GEMM, csrc/conv_pw.hip
#   anything else with Cin % 16 == 0                  -> implicit GEMM, csrc/conv_mfma.hip (odd sizes, unaligned channel slices)
# `impl=` forces one kernel for the tests and probes: 'wino4', 'poly5', 'poly5x4' (four accumulating phase launches), 'gemm',
# 'direct' (plain-VALU cross-check in the product library), 'wino2' (the F(2x2,3x3) kernel of the TEST-ONLY libl3c_hip_xcheck.so).


class PackedConv(object):
    """One conv layer resident on the device: OIHW weights, bias, and the packed copies of the kernels that can run it."""

    def __init__(self, weight, bias, stride=1, dilation=1):
        _lib.require_gpu()
        lib = _lib.load()
        self.Cout, self.Cin, self.KS, _ = weight.shape
        self.stride, self.dilation = stride, dilation
        self.weight = weight.detach().to('cuda', torch.float32).contiguous()
        self.bias = bias.detach().to('cuda', torch.float32).contiguous()
        self.packed = None            # implicit GEMM (generic form)
        if self.Cin % 16 == 0:
            self.packed = torch.empty(lib.l3c_conv_packed_words(self.Cout, self.Cin, self.KS), dtype=torch.float32, device='cuda')
            call('l3c_conv_pack_weights', ptr(self.weight), self.Cout, self.Cin, self.KS, ptr(self.packed), stream())
        self.packed_wino4 = None      # G g G^T of F(4x4,3x3)
        if self.KS == 3 and stride == 1 and dilation in (1, 2, 4) and self.Cin % 16 == 0:
            self.packed_wino4 = self._pack_wino4(self.weight)
        # 5x5 stride 2 padding 2 = four 3x3 stride-1 convolutions of the input's 2x2 phases (include/l3c_hip.h, l3c_conv_wino4_stride2):
        # phase kernel w_ab[u][v] = w[2u+a][2v+b], zero where the index exceeds 4; all four in ONE launch: the phase kernels
        # concatenated along the input-channel axis
        self.packed_poly_fused = None
        if self.KS == 5 and stride == 2 and dilation == 1 and self.Cin % 16 == 0 and self.Cout % 4 == 0:
            w_cat = torch.zeros(self.Cout, 4 * self.Cin, 3, 3, dtype=torch.float32, device='cuda')
            for k, sub in enumerate(self._phase_kernels()):
                w_cat[:, k * self.Cin:(k + 1) * self.Cin, :sub.shape[2], :sub.shape[3]] = sub
            self.packed_poly_fused = self._pack_wino4(w_cat)
        self.packed_pw = None
        if self.KS == 1 and stride == 1 and self.Cin % 64 == 0 and self.Cout <= 160:
            self.packed_pw = torch.empty(lib.l3c_conv_pw_packed_words(self.Cout, self.Cin), dtype=torch.float32, device='cuda')
            call('l3c_conv_pw_pack_weights', ptr(self.weight), self.Cout, self.Cin, ptr(self.packed_pw), stream())
        self._packed_poly = self._packed_wino2 = self._zero_bias = self._packed_wino4_shuffle = None

    def _pack_wino4(self, w):
        packed = torch.empty(_lib.load().l3c_conv_wino4_packed_words(w.shape[0], w.shape[1]), dtype=torch.float32, device='cuda')
        call('l3c_conv_wino4_pack_weights', ptr(w.contiguous()), w.shape[0], w.shape[1], ptr(packed), stream())
        return packed

    def packed_wino4_shuffle(self):
        """the 64 -> 256 PixelShuffle tail on the Winograd kernel (include/l3c_hip.h, L3C_EPI_PIXEL_SHUFFLE): G g G^T of the weights in
        sub-pixel-major order -- row 64 s + oc = the layer's row 4 oc + s -- packed on first use"""
        if self._packed_wino4_shuffle is None:
            assert self.Cout == 256
            w = self.weight.reshape(64, 4, self.Cin, 3, 3).permute(1, 0, 2, 3, 4).reshape(256, self.Cin, 3, 3)
            self._packed_wino4_shuffle = self._pack_wino4(w)
        return self._packed_wino4_shuffle

    def _phase_kernels(self):
        return [self.weight[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)]

    def packed_poly(self):
        """tests only ('poly5x4'): the four phase kernels packed one by one, for l3c_conv_wino4_phase"""
        if self._packed_poly is None:
            self._packed_poly = []
            for sub in self._phase_kernels():
                wp = torch.zeros(self.Cout, self.Cin, 3, 3, dtype=torch.float32, device='cuda')
                wp[:, :, :sub.shape[2], :sub.shape[3]] = sub
                self._packed_poly.append(self._pack_wino4(wp))
            self._zero_bias = torch.zeros(self.Cout, dtype=torch.float32, device='cuda')
        return self._packed_poly

    def packed_wino2(self):
        """tests only ('wino2'): G g G^T of the F(2x2,3x3) kernel in the cross-check library"""
        if self._packed_wino2 is None:
            assert self.KS == 3 and self.stride == 1 and self.Cin % 16 == 0 and self.Cout % 4 == 0
            n = _lib.load_xcheck().l3c_conv_wino_packed_words(self.Cout, self.Cin)
            self._packed_wino2 = torch.empty(n, dtype=torch.float32, device='cuda')
            _lib.call_xcheck('l3c_conv_wino_pack_weights', ptr(self.weight), self.Cout, self.Cin, ptr(self._packed_wino2), stream())
        return self._packed_wino2

    def packed_wino4w(self):
        """tests / probes only ('wino4w'): the F(4x4,3x3) probe kernel on the 32x32x2 MFMA in the cross-check library (csrc/conv_wino4w.hip)"""
        if getattr(self, '_packed_wino4w', None) is None:
            assert self.KS == 3 and self.stride == 1 and self.dilation == 1 and self.Cin % 16 == 0 and self.Cout <= 64
            n = _lib.load_xcheck().l3c_conv_wino4w_packed_words(self.Cout, self.Cin)
            self._packed_wino4w = torch.empty(n, dtype=torch.float32, device='cuda')
            _lib.call_xcheck('l3c_conv_wino4w_pack_weights', ptr(self.weight), self.Cout, self.Cin, ptr(self._packed_wino4w), stream())
        return self._packed_wino4w

    def out_hw(self, H, W):
        pad = self.KS // 2 if self.dilation == 1 else self.dilation
        ext = (self.KS - 1) * self.dilation + 1
        return (H + 2 * pad - ext) // self.stride + 1, (W + 2 * pad - ext) // self.stride + 1


def _conv_desc(x, layer, out, in_coff, out_coff, packed_w, ks_stride_dilation, bias=None, residual=None, res_coff=0, epilogue=0):
    """The ConvDesc of one launch of `layer` on x (B,H,W,cstride) into `out`: `packed_w` the weights in the kernel's own form,
    ks_stride_dilation what that kernel is told it runs (a polyphase launch is not the layer's 5x5 stride 2)."""
    B, H, W, cstride = x.shape
    d = ConvDesc()
    d.inp, d.in_cstride, d.in_coff = ptr(x, torch.float32), cstride, in_coff
    d.packed_w, d.bias = ptr(packed_w), ptr(layer.bias if bias is None else bias)
    d.residual = ptr(residual, torch.float32) if residual is not None else None
    d.res_cstride, d.res_coff = (residual.shape[-1] if residual is not None else 0), res_coff
    d.out, d.out_cstride, d.out_coff = ptr(out, torch.float32), out.shape[-1], out_coff
    d.B, d.Hin, d.Win, d.Cin, d.Cout = B, H, W, layer.Cin, layer.Cout
    d.KS, d.stride, d.dilation = ks_stride_dilation
    d.epilogue = epilogue
    return d


def conv(x, layer, out=None, in_coff=0, out_coff=0, residual=None, res_coff=0, relu=False, pixel_shuffle=False, impl=None):
    """x: (B,H,W,cstride) pixel-major fp32.  Returns `out` ((B,Ho,Wo,Cout) freshly allocated when None).  impl: None = the
    product's dispatch (see above); a name forces one kernel (tests, probes)."""
    B, H, W, cstride = x.shape
    Ho, Wo = layer.out_hw(H, W)
    if out is None:
        out = (torch.empty(B, 2 * Ho, 2 * Wo, layer.Cout // 4, dtype=torch.float32, device=x.device) if pixel_shuffle
               else torch.empty(B, Ho, Wo, layer.Cout, dtype=torch.float32, device=x.device))
    assert impl in (None, 'wino4', 'wino2', 'wino4w', 'gemm', 'poly5', 'poly5x4', 'direct'), impl

    # The Winograd kernel stores / loads 16 bytes per lane: channel strides and offsets of the output (and residual) slices must be
    # multiples of 4, the pointers 16-byte aligned, Cout a multiple of 4 (pixel shuffle: 16); it addresses one input image with
    # 32-bit offsets (< 2 GB) and has no pixel shuffle combined with dilation, ReLU or a residual -- the preconditions
    # l3c_conv_wino4 checks.  Anything else goes to the implicit-GEMM kernel (64-bit addressing, 4-byte stores).
    def _aligned(t, coff):
        return t is None or (t.shape[-1] % 4 == 0 and coff % 4 == 0 and t.data_ptr() % 16 == 0)
    in_ok = x.data_ptr() % 16 == 0 and cstride % 4 == 0 and in_coff % 4 == 0 and H * W * cstride * 4 < 0x7ffffff0
    wino_ok = (layer.KS == 3 and layer.stride == 1 and in_ok and _aligned(out, out_coff) and _aligned(residual, res_coff) and
               layer.Cout % 4 == 0 and (not pixel_shuffle or layer.Cout == 256) and
               not (pixel_shuffle and (relu or residual is not None or layer.dilation != 1)))
    poly_ok = (layer.packed_poly_fused is not None and H % 2 == 0 and W % 2 == 0 and in_ok and _aligned(out, out_coff) and
               residual is None and not relu and not pixel_shuffle)
    if impl in ('poly5', 'poly5x4') or (impl is None and poly_ok):
        assert poly_ok, 'this layer / tensor has no polyphase form'
        return _conv_poly5(x, layer, out, in_coff, out_coff, fused=impl != 'poly5x4')
    if impl is None:
        kernel = ('wino4' if layer.packed_wino4 is not None and wino_ok else
                  'pw' if layer.packed_pw is not None and not (relu or pixel_shuffle or residual is not None) else 'gemm')
    else:
        kernel = impl
    if kernel == 'wino4w':      # probe kernel of the test-only library: 3x3 / stride 1 / dilation 1, bias (+ ReLU)
        assert layer.KS == 3 and layer.stride == 1 and layer.dilation == 1 and residual is None and not pixel_shuffle
        d = _conv_desc(x, layer, out, in_coff, out_coff, layer.packed_wino4w(), (3, 1, 1), epilogue=_lib.EPI_RELU if relu else 0)
        _lib.call_xcheck('l3c_conv_wino4w', d, int(os.environ.get('L3C_W4W_TPB', '0')), stream())
        return out
    if kernel in ('wino4', 'wino2'):
        assert wino_ok and (kernel == 'wino2' or layer.packed_wino4 is not None), 'this layer / epilogue has no Winograd form'
    if kernel == 'gemm' and layer.packed is None:
        raise _lib.L3CError('convolution outside every MFMA kernel\'s preconditions (Cin % 16 != 0)')
    packed_w = ({'wino4': layer.packed_wino4_shuffle() if (kernel == 'wino4' and pixel_shuffle) else layer.packed_wino4,
                 'pw': layer.packed_pw, 'gemm': layer.packed, 'direct': layer.weight}[kernel]
                if kernel != 'wino2' else layer.packed_wino2())
    d = _conv_desc(x, layer, out, in_coff, out_coff, packed_w, (layer.KS, layer.stride, layer.dilation), residual=residual, res_coff=res_coff,
                   epilogue=((_lib.EPI_RELU if relu else 0) | (_lib.EPI_RESIDUAL if residual is not None else 0) |
                             (_lib.EPI_PIXEL_SHUFFLE if pixel_shuffle else 0)))
    if kernel == 'wino2':
        _lib.call_xcheck('l3c_conv_wino', d, stream())
        return out
    entry = {'wino4': 'l3c_conv_wino4', 'pw': 'l3c_conv_pw', 'gemm': 'l3c_conv_mfma', 'direct': 'l3c_conv_direct'}[kernel]
    if PROFILE is None or kernel == 'direct':
        call(entry, d, stream())
        return out
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call(entry, d, stream())
    e1.record()
    key = ('conv_wino4_kernel' if kernel == 'wino4' else 'conv_lds_kernel<3,{}>'.format(layer.dilation) if layer.KS == 3 else
           'conv k{} s{} (mfma)'.format(layer.KS, layer.stride))   # 3x3: the kernel name rocprofv3 reports
    if PROFILE_DETAIL:
        key += ' {}->{} {}x{}{}{}'.format(layer.Cin, layer.Cout, Ho, Wo, ' +res' if residual is not None else '', ' shuffle' if pixel_shuffle else '')
    nbytes = 4.0 * B * (H * W * layer.Cin + Ho * Wo * layer.Cout * (2 if residual is not None else 1))   # in + out (+ residual), once
    # (sixth field: the kernel's template arguments as rocprofv3 prints them -- bench.py joins the PMC table's per-variant bytes with these)
    variant = '{},{},{},false'.format(*('true' if f else 'false' for f in (relu, residual is not None, pixel_shuffle))) if kernel == 'wino4' else ''
    PROFILE.append((key, 2.0 * B * Ho * Wo * layer.Cout * layer.Cin * layer.KS * layer.KS, nbytes, e0, e1, variant))
    return out


def _conv_poly5(x, layer, out, in_coff, out_coff, fused=True):
    """5x5 stride 2 in polyphase form on the F(4x4,3x3) kernel: all four phases in one launch, or (fused=False) four phase launches
    accumulating into `out` (the first carries the bias)."""
    B, H, W, cstride = x.shape
    e0 = e1 = None
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if fused:
        d = _conv_desc(x, layer, out, in_coff, out_coff, layer.packed_poly_fused, (5, 2, 1))
        call('l3c_conv_wino4_stride2', d, stream())
    for k, (a, b) in enumerate(() if fused else ((0, 0), (0, 1), (1, 0), (1, 1))):
        packed_w = layer.packed_poly()[k]             # (also makes layer._zero_bias)
        d = _conv_desc(x, layer, out, in_coff, out_coff, packed_w, (3, 2, 1), bias=layer.bias if k == 0 else layer._zero_bias,
                       residual=out if k else None, res_coff=out_coff if k else 0, epilogue=_lib.EPI_RESIDUAL if k else 0)
        call('l3c_conv_wino4_phase', d, a, b, stream())
    if PROFILE is not None:
        e1.record()
        nbytes = 4.0 * B * (H * W * layer.Cin + (H // 2) * (W // 2) * layer.Cout)
        PROFILE.append(('conv k5 s2 (4 F(4x4,3x3) phases)', 2.0 * B * (H // 2) * (W // 2) * layer.Cout * layer.Cin * 25, nbytes, e0, e1))
    return out


def rgb_head(img, ms1_w, ms1_b, ms2_w, ms2_b, conv_w, conv_b, want_shifted=False):
    """img (B,3,H,W) planar 0..255 -> (B,H,W,Cf) pixel-major features [, (B,3,H,W) mean-shifted image]."""
    B, _, H, W = img.shape
    Cf = conv_w.shape[0]
    out = torch.empty(B, H, W, Cf, dtype=torch.float32, device=img.device)
    shifted = torch.empty_like(img) if want_shifted else None
    call('l3c_rgb_head', ptr(img, torch.float32), ptr(ms1_w), ptr(ms1_b), ptr(ms2_w), ptr(ms2_b), ptr(conv_w),
         ptr(conv_b), B, H, W, Cf, ptr(out), ptr(shifted), stream())
    return (out, shifted) if want_shifted else out


def to_q_quantize(feat, w, b, levels, want_bn=False):
    """feat (B,H,W,Cf) -> sym int16 (B,C,H,W), bn_q fp32 (B,C,H,W) [, bn pre-quantisation].
    `feat` must start on a 16-byte boundary (every torch allocation and every whole-pixel slice of one does): the library refuses
    anything else with L3C_ERR_INVALID_ARG -- its kernels read a pixel's features with 16-byte loads."""
    B, H, W, Cf = feat.shape
    C, L = w.shape[0], levels.shape[0]
    sym = torch.empty(B, C, H, W, dtype=torch.int16, device=feat.device)
    bn_q = torch.empty(B, C, H, W, dtype=torch.float32, device=feat.device)
    bn = torch.empty_like(bn_q) if want_bn else None
    call('l3c_to_q_quantize', ptr(feat, torch.float32), ptr(w), ptr(b), ptr(levels), B, H * W, Cf, C, L, ptr(sym),
         ptr(bn_q), ptr(bn), stream())
    return (sym, bn_q, bn) if want_bn else (sym, bn_q)


def dec_head(bn_q, w, b, fuse=None):
    """bn_q (B,C,H,W) planar -> (B,H,W,Cf) pixel-major, + fuse."""
    B, C, H, W = bn_q.shape
    Cf = w.shape[0]
    out = torch.empty(B, H, W, Cf, dtype=torch.float32, device=bn_q.device)
    call('l3c_dec_head', ptr(bn_q, torch.float32), ptr(w), ptr(b), ptr(fuse, torch.float32) if fuse is not None else None,
         B, H * W, C, Cf, ptr(out), stream())
    return out


def sym_to_bn(sym, bin_width, x_min):
    bn = torch.empty(sym.shape, dtype=torch.float32, device=sym.device)
    call('l3c_sym_to_bn', ptr(sym, torch.int16), sym.numel(), float(bin_width), float(x_min), ptr(bn), stream())
    return bn


def sym_to_u8(sym):
    """l3c_sym_to_u8: int16 symbols -> uint8 tensor of the same shape (the low byte: the decoded RGB symbols as pixels)."""
    out = torch.empty(sym.shape, dtype=torch.uint8, device=sym.device)
    if sym.numel():
        call('l3c_sym_to_u8', ptr(sym, torch.int16), sym.numel(), ptr(out, torch.uint8), stream())
    return out


# ---- RGB baselines: bicubic pyramid encoder ------------------------------------------------------------------------------

_RGB_MEAN = None
_COEFFS = {}


def rgb_mean():
    """(0.4488, 0.4371, 0.4040) * 255 in fp32, as BicubicDownsamplingEnc builds it (net.py:69-70)."""
    global _RGB_MEAN
    if _RGB_MEAN is None:
        m = torch.tensor([0.4488, 0.4371, 0.4040], dtype=torch.float32).mul(255.)
        _RGB_MEAN = (ctypes.c_float * 3)(*[float(v) for v in m])
    return _RGB_MEAN


def _resample_tables(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    if key not in _COEFFS:
        from .helpers import pil_resample
        bounds, kk, ksize = pil_resample.precompute_coeffs(in_size, out_size)
        _COEFFS[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize)
    return _COEFFS[key]


def meanshift_planar(img, w, b):
    B, _, H, W = img.shape
    out = torch.empty_like(img)
    call('l3c_meanshift_planar', ptr(img, torch.float32), ptr(w), ptr(b), B, H * W, ptr(out), stream())
    return out


def bicubic_encoder(x):
    """x (B,3,H,W) fp32 planar, mean-shifted -> (bn (B,3,H/2,W/2) fp32, sym int16): round to uint8, Pillow-exact BICUBIC
    half-size resize (horizontal pass, then vertical), symbols = pixel values, bn = value - mean."""
    B, _, H, W = x.shape
    oh, ow = int(H * 0.5), int(W * 0.5)
    if oh < 1 or ow < 1:
        raise ValueError('image too small for another bicubic scale: {}x{}'.format(H, W))
    u8 = torch.empty(B, 3, H, W, dtype=torch.uint8, device=x.device)
    call('l3c_rgb_to_u8', ptr(x, torch.float32), rgb_mean(), B, H * W, ptr(u8), stream())
    bw, kw, ksw = _resample_tables(W, ow, x.device)
    tmp = torch.empty(B, 3, H, ow, dtype=torch.uint8, device=x.device)
    call('l3c_resample_u8', ptr(u8), B * 3, H, W, 0, ow, ptr(bw), ptr(kw), ksw, ptr(tmp), stream())
    bh, kh, ksh = _resample_tables(H, oh, x.device)
    down = torch.empty(B, 3, oh, ow, dtype=torch.uint8, device=x.device)
    call('l3c_resample_u8', ptr(tmp), B * 3, H, ow, 1, oh, ptr(bh), ptr(kh), ksh, ptr(down), stream())
    sym = torch.empty(B, 3, oh, ow, dtype=torch.int16, device=x.device)
    bn = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=x.device)
    call('l3c_u8_to_sym_bn', ptr(down), rgb_mean(), B, oh * ow, ptr(sym), ptr(bn), stream())
    return bn, sym


# ---- logistic-mixture head --------------------------------------------------------------------------------------------


def as_pixel_major(l):
    """(N,Kp,H,W) logical tensor -> (N,H,W,Kp) contiguous storage (free when `l` already is a permuted NHWC view)."""
    return l.permute(0, 2, 3, 1).contiguous()


def dmll_channel_params(P_nhwc, sym, C, K, rgb, c):
    """-> pi, mu, log_sigma, each (B,K,H,W)."""
    B, H, W, _ = P_nhwc.shape
    outs = [torch.empty(B, K, H, W, dtype=torch.float32, device=P_nhwc.device) for _ in range(3)]
    call('l3c_dmll_channel_params', ptr(P_nhwc, torch.float32), ptr(sym, torch.int16) if sym is not None else None,
         B, H * W, C, K, int(rgb), c, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), stream())
    return outs


def cdf_table_mixture(targets, pi, mu, log_sigma, check_monotone=True):
    """params (B,K,H,W) -> uint16 table viewed as int16 (B,H,W,Lp); also returns the not-monotone flag tensor."""
    B, K, H, W = pi.shape
    Lp = targets.shape[0]
    cdf = torch.empty(B, H, W, Lp, dtype=torch.int16, device=pi.device)
    flag = torch.zeros(1, dtype=torch.int32, device=pi.device) if check_monotone else None
    call('l3c_cdf_table_mixture', ptr(targets, torch.float32), ptr(pi, torch.float32), ptr(mu, torch.float32),
         ptr(log_sigma, torch.float32), B, H * W, K, Lp, ptr(cdf), ptr(flag), stream())
    return cdf, flag


def dmll_cdf_table(P_nhwc, sym, targets, C, K, rgb, c, pix0, npix, flag=None, window_stats=None):
    """Fused decoder head: uint16 table rows (viewed as int16, (B, npix, Lp)) of channel c for pixels [pix0, pix0 + npix) of
    every image; `flag` (int32[1], device) is set if a row is not strictly increasing (never cleared).
    window_stats (int32 (B,), device; RGB scale only): per image the miss count its decoder reported two chunks earlier -- an image
    whose count allows it gets 65-entry WINDOW rows packed from the start of its (B, npix, Lp) slot, the others full rows
    (include/l3c_hip.h, l3c_ac_decode_part); pass the same tensor to `ac_decode_part(window=...)`."""
    B, H, W, _ = P_nhwc.shape
    Lp = targets.shape[0]
    cdf = torch.empty(B, npix, Lp, dtype=torch.int16, device=P_nhwc.device)
    call('l3c_dmll_cdf_table', ptr(P_nhwc, torch.float32), ptr(sym, torch.int16) if sym is not None else None,
         ptr(targets, torch.float32), B, H * W, C, K, int(rgb), c, pix0, npix, Lp, ptr(cdf),
         ptr(flag, torch.int32) if flag is not None else None,
         ptr(window_stats, torch.int32) if window_stats is not None else None, stream())
    return cdf


def dmll_cdf_table_parts(P_nhwc, sym, targets, C, K, rgb, parts):
    """Grouped form of `dmll_cdf_table` (l3c_dmll_cdf_table_parts): parts = [(c, pix0, npix, flag or None, window_stats or None)], up to 8,
    ONE launch.  -> list of tables (int16 (B, npix, Lp)) in the order of `parts`."""
    B, H, W, _ = P_nhwc.shape
    Lp = targets.shape[0]
    arr = (_lib.TablePart * len(parts))()
    tables = []
    for i, (c, pix0, npix, flag, wstats) in enumerate(parts):
        t = torch.empty(B, npix, Lp, dtype=torch.int16, device=P_nhwc.device)
        tables.append(t)
        arr[i] = _lib.TablePart(c, pix0, npix, ptr(t), ptr(flag, torch.int32) if flag is not None else None,
                                ptr(wstats, torch.int32) if wstats is not None else None)
    call('l3c_dmll_cdf_table_parts', ptr(P_nhwc, torch.float32), ptr(sym, torch.int16) if sym is not None else None,
         ptr(targets, torch.float32), B, H * W, C, K, int(rgb), Lp, arr, len(parts), stream())
    return tables


def _run_rgb_pipeline(entry_point, desc, lag, side_stream, tensors):
    """The tail of the decode_rgb* wrappers: one library call runs the whole chunk pipeline of `desc` on (current stream, side stream).
    lag 2 decodes on `side_stream` (a torch stream) while the current stream builds the next step's tables, so the allocator must know that
    `tensors` -- everything the descriptor points to -- are in use there; lag 1 runs on the current stream alone."""
    if lag == 2:
        for t in tensors:
            t.record_stream(side_stream)
    call(entry_point, ctypes.byref(desc), torch.cuda.current_stream().cuda_stream, side_stream.cuda_stream if lag == 2 else None)


def decode_rgb(P_nhwc, targets, sym, buf, offs, lens, bounds, K, lag, window_mode, side_stream=None):
    """The whole RGB scale in one host call (l3c_decode_rgb): P (B,H,W,120), sym int16 (B,3,H,W) ZEROED (receives the symbols), the streams
    CHANNEL-major in (buf, offs int64 (3B,), lens int32 (3B,)), bounds = [(pix0, npix)] tiling H*W.  lag 2 decodes on `side_stream` (a
    torch stream) while the current stream builds the next step's tables.  -> (workspace tensor, window statistics view (3, chunks + 2, B)
    or None); the current stream is ordered after the last symbols."""
    lib = _lib.load()
    B, H, W, _ = P_nhwc.shape
    n = len(bounds)
    max_npix = max(b[1] for b in bounds)
    nbytes = lib.l3c_decode_rgb_workspace_bytes(B, max_npix, n, lag)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=P_nhwc.device)
    p0 = (_lib.c_i64 * n)(*[b[0] for b in bounds])
    np_ = (_lib.c_i64 * n)(*[b[1] for b in bounds])
    desc = _lib.RgbDecodeDesc(ptr(P_nhwc, torch.float32), ptr(targets, torch.float32), ptr(sym, torch.int16), B, H * W, K,
                              ptr(buf, torch.uint8), ptr(offs, torch.int64), ptr(lens, torch.int32), n,
                              ctypes.cast(p0, ctypes.POINTER(_lib.c_i64)), ctypes.cast(np_, ctypes.POINTER(_lib.c_i64)),
                              lag, window_mode, ptr(ws), nbytes)
    _run_rgb_pipeline('l3c_decode_rgb', desc, lag, side_stream, (P_nhwc, targets, sym, buf, offs, lens, ws))
    stats = None
    if window_mode:
        o = lib.l3c_decode_rgb_stats_offset(B, max_npix, n, lag)
        stats = ws[o:o + 3 * (n + 2) * B * 4].view(torch.int32).view(3, n + 2, B)
    return ws, stats


_PINNED_SCRATCH = {'bufs': [None] * 16, 'events': [None] * 16, 'turn': 0}


def upload_small(array):
    """numpy array -> device tensor of the same dtype through a small ring of page-locked buffers (an H2D copy from pageable memory makes the
    host wait for the stream): descriptor tables of a few KB."""
    a = np.ascontiguousarray(array)
    r = _PINNED_SCRATCH
    k = r['turn'] = (r['turn'] + 1) % len(r['bufs'])
    if r['events'][k] is not None:
        r['events'][k].synchronize()
    n = a.nbytes
    if r['bufs'][k] is None or r['bufs'][k].numel() < n:
        r['bufs'][k] = torch.empty(max(n, 1 << 18), dtype=torch.uint8, pin_memory=True)
    r['bufs'][k].numpy()[:n] = a.view(np.uint8).reshape(-1)
    dev = r['bufs'][k][:n].cuda(non_blocking=True)
    r['events'][k] = torch.cuda.Event()
    r['events'][k].record(torch.cuda.current_stream())
    return dev.view(torch.from_numpy(a[:0]).dtype).reshape(a.shape)


def ragged_rgb_plan(hws, n_regular, probe):
    """Chunk plan of a RAGGED RGB decode (l3c_decode_rgb_ragged): every image gets the same NUMBER of chunks -- two probe chunks of `probe`
    symbols (0: none) and n_regular regular ones, the image's own chunk length rounded DOWN to a multiple of 64 with the last chunk taking
    the rest -- so that all images step through the pipeline together.  hws: pixels per image.  -> (pix0, npix) int64 arrays (n_chunks, B)."""
    B = len(hws)
    n_chunks = n_regular + (2 if probe else 0)
    pix0 = np.zeros((n_chunks, B), dtype=np.int64)
    npix = np.zeros((n_chunks, B), dtype=np.int64)
    for b, hw in enumerate(hws):
        start, j = 0, 0
        if probe:
            pix0[0, b], npix[0, b], pix0[1, b], npix[1, b] = 0, probe, probe, probe
            start, j = 2 * probe, 2
        step = (hw - start) // n_regular // 64 * 64
        assert n_regular == 1 or step >= 64, 'image too small for {} chunks'.format(n_regular)
        for k in range(n_regular):
            pix0[j + k, b] = start + k * step
            npix[j + k, b] = step if k + 1 < n_regular else hw - start - k * step
    return pix0, npix


def decode_rgb_ragged(P_ragged, targets, sym_ragged, buf, offs, lens, hws, pix0, npix, K, lag, window_mode, side_stream=None):
    """The RGB scale of B images of DIFFERENT sizes in lock step (l3c_decode_rgb_ragged): P_ragged (sum HW, 120) fp32, sym_ragged int16
    (3 * sum HW,) ZEROED (image b: its three planes from element 3 * pixbase[b]), streams CHANNEL-major in (buf, offs (3B,), lens (3B,)),
    hws = pixels per image, (pix0, npix) = ragged_rgb_plan(...).  -> workspace tensor (kept alive by the caller until the stream is done)."""
    lib = _lib.load()
    B, n = len(hws), pix0.shape[0]
    hw = np.asarray(hws, dtype=np.int64)
    pixbase = np.concatenate([[0], np.cumsum(hw)[:-1]]).astype(np.int64)
    table_off = (np.cumsum(npix, axis=1) - npix) * (257 * 2)
    tables = upload_small(np.concatenate([pixbase, hw, pix0.reshape(-1), npix.reshape(-1), table_off.reshape(-1)]).astype(np.int64))
    max_total = int(npix.sum(axis=1).max())
    nbytes = lib.l3c_decode_rgb_ragged_workspace_bytes(B, max_total, n, lag)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=P_ragged.device)
    hw_c = (_lib.c_i64 * B)(*[int(v) for v in hw])
    p0_c = (_lib.c_i64 * (n * B))(*[int(v) for v in pix0.reshape(-1)])
    np_c = (_lib.c_i64 * (n * B))(*[int(v) for v in npix.reshape(-1)])
    desc = _lib.RgbRaggedDesc(ptr(P_ragged, torch.float32), ptr(targets, torch.float32), ptr(sym_ragged, torch.int16), B,
                              ctypes.cast(hw_c, ctypes.POINTER(_lib.c_i64)), K, ptr(buf, torch.uint8), ptr(offs, torch.int64),
                              ptr(lens, torch.int32), n, ctypes.cast(p0_c, ctypes.POINTER(_lib.c_i64)),
                              ctypes.cast(np_c, ctypes.POINTER(_lib.c_i64)), ptr(tables, torch.int64), lag, window_mode, ptr(ws), nbytes)
    _run_rgb_pipeline('l3c_decode_rgb_ragged', desc, lag, side_stream, (P_ragged, targets, sym_ragged, buf, offs, lens, ws, tables))
    return ws, tables


def decode_z_entries(P, targets, sym, buf, offs, lens, pixbase, hw, pix0, npix, total_pix, C, K):
    """A bottleneck scale as S ragged ENTRIES: its C channels are independent given P, so ONE ragged table launch (l3c_dmll_cdf_table_ragged,
    C parts) and ONE ragged decoder launch (l3c_ac_decode_chunks with the r_* fields) decode every entry and channel side by side.  Entry s
    (int64 arrays of S) is pixels [pix0, pix0 + npix) of an image of hw pixels that starts at pixel pixbase of P ((total_pix, 3 C K) fp32):
    a whole image of a set of DIFFERENT sizes, or one band of a banded file.  sym int16 (C * total_pix,) receives the symbols, an image's C
    planes from element C * pixbase; streams in (buf, offs (C S,), lens (C S,)) with stream (c, s) at index c S + s.
    -> tensors to keep alive until the stream is done."""
    assert C <= 8
    S = len(hw)
    Lp = targets.shape[0]
    tables = upload_small(np.concatenate([pixbase, hw, pix0, npix, (pixbase + pix0) * (Lp * 2)]).astype(np.int64))
    base = tables.data_ptr()
    max_hw, max_npix = int(np.max(hw)), int(np.max(npix))
    flag = torch.zeros(1, dtype=torch.int32, device=P.device)
    tabs = [torch.empty(total_pix * Lp, dtype=torch.int16, device=P.device) for _ in range(C)]
    batch = _lib.RaggedBatch(S, max_hw, base, base + 8 * S)
    tparts = (_lib.TablePart * C)()
    rparts = (_lib.RaggedPart * C)()
    dparts = (_lib.AcDecodePart * C)()
    for c in range(C):
        tparts[c] = _lib.TablePart(c, 0, max_npix, ptr(tabs[c]), ptr(flag, torch.int32), None)
        rparts[c] = _lib.RaggedPart(base + 16 * S, base + 24 * S, base + 32 * S)
        d = _lib.AcDecodePart(ptr(tabs[c]), Lp, ptr(buf, torch.uint8), ptr(offs[c * S:(c + 1) * S], torch.int64),
                              ptr(lens[c * S:(c + 1) * S], torch.int32), S, max_npix, ptr(flag, torch.int32), None, None, 1,
                              ptr(sym, torch.int16), 0, 0)
        d.r_npix, d.r_table_off, d.r_pixbase, d.r_hw, d.r_pix0 = base + 24 * S, base + 32 * S, base, base + 8 * S, base + 16 * S
        d.r_C, d.r_c, d.r_table_bytes = C, c, total_pix * Lp * 2
        dparts[c] = d
    call('l3c_dmll_cdf_table_ragged', ptr(P, torch.float32), None, ptr(targets, torch.float32), ctypes.byref(batch), C, K, 0, Lp,
         tparts, rparts, C, stream())
    call('l3c_ac_decode_chunks', dparts, C, stream())
    return tabs, tables, flag


def decode_rgb_banded(P_nhwc, targets, sym, buf, offs, lens, band_len, n_chunks, K, lag, window_mode, side_stream=None):
    """An RGB scale of banded files in one host call (l3c_decode_rgb_banded): P (B,H,W,120), sym int16 (B,3,H,W) ZEROED, the band streams in
    (buf, offs, lens) with stream (c, b, j) at index (c B + b) n + j.  -> workspace tensor; the current stream is ordered after the symbols."""
    lib = _lib.load()
    B, H, W, _ = P_nhwc.shape
    HW = H * W
    nbytes = lib.l3c_decode_rgb_banded_workspace_bytes(B, HW, band_len, n_chunks, lag)
    if nbytes < 0:
        raise _lib.L3CError('l3c_decode_rgb_banded_workspace_bytes: bad arguments (B={}, HW={}, L={}, chunks={})'.format(B, HW, band_len, n_chunks))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=P_nhwc.device)
    desc = _lib.RgbBandedDesc(ptr(P_nhwc, torch.float32), ptr(targets, torch.float32), ptr(sym, torch.int16), B, HW, K,
                              ptr(buf, torch.uint8), ptr(offs, torch.int64), ptr(lens, torch.int32), band_len, n_chunks, lag, window_mode,
                              ptr(ws), nbytes)
    _run_rgb_pipeline('l3c_decode_rgb_banded', desc, lag, side_stream, (P_nhwc, targets, sym, buf, offs, lens, ws))
    return ws


ENTRIES_MAX = 65535     # l3c_decode_rgb_entries / the ragged table kernel: one grid row per entry (grid.y)


def entry_slices(n_entries, limit=ENTRIES_MAX):
    """[(first, end)] slices of at most `limit` entries that cover n_entries in order."""
    limit = max(1, min(int(limit), ENTRIES_MAX))
    return [(a, min(n_entries, a + limit)) for a in range(0, n_entries, limit)]


def rgb_entries_plan(lens, n_chunks):
    """The chunk plan l3c_decode_rgb_entries writes on the device, as a pure function (tests, sizing): entry e of lens[e] symbols steps in
    step_e = 64 ceil(len_e / (64 n_chunks)); chunk k is [k step_e, min((k + 1) step_e, len_e)), empty past the entry's end.
    -> (start (n_chunks, S) relative to the entry's pix0, npix (n_chunks, S), final chunk (S,), table_off (n_chunks, S) bytes)."""
    lens = np.asarray(lens, dtype=np.int64)
    step = 64 * (-(-lens // (64 * n_chunks)))
    k = np.arange(n_chunks, dtype=np.int64)[:, None]
    start = np.minimum(k * step, lens - 1)
    npix = np.clip(lens - k * step, 0, step)
    table_off = (np.cumsum(npix, axis=1) - npix) * (257 * 2)
    return start, npix, (lens - 1) // step, table_off


def rgb_entries_workspace_bytes(lens, n_chunks, lag):
    """l3c_decode_rgb_entries_workspace_bytes of entries of `lens` symbols (no GPU needed)."""
    lens = np.ascontiguousarray(lens, dtype=np.int64)
    n = _lib.load().l3c_decode_rgb_entries_workspace_bytes(lens.shape[0], lens.ctypes.data_as(ctypes.POINTER(_lib.c_i64)), int(n_chunks), int(lag))
    if n < 0:
        raise _lib.L3CError('l3c_decode_rgb_entries_workspace_bytes: bad arguments (S={}, chunks={}, lag={})'.format(lens.shape[0], n_chunks, lag))
    return n


def rgb_entries_chunks(lens, budget_bytes, lag, lo=8, hi=256):
    """Chunks per entry of an entries RGB decode: the smallest count from `lo` on whose workspace stays within budget_bytes (the tables of
    a step shrink with the count; the per-chunk plan arrays, (2 + 3 n) S int64, grow with it).  Fewer chunks = fewer pipeline steps and
    launches.  -> (count, fits).  fits is False where NO count keeps the workspace within the budget -- a few tiny images, whose plan arrays
    outweigh their tables: a legacy decode keeps those arrays outside its workspace, an entries decode inside -- and the count is then the
    one with the smallest workspace, the counts below `lo` included."""
    best, n = None, lo
    while n <= hi:
        ws = rgb_entries_workspace_bytes(lens, n, lag)
        if ws <= budget_bytes:
            return n, True
        if best is None or ws < best[0]:
            best = (ws, n)
        n += max(1, n // 8)
    for n in range(min(lo, hi + 1) - 1, 0, -1):
        ws = rgb_entries_workspace_bytes(lens, n, lag)
        if ws <= budget_bytes:
            return n, True
        if ws < best[0]:
            best = (ws, n)
    return best[1], False


def rgb_entries_device_plan(ws, S, n_chunks):
    """The plan l3c_decode_rgb_entries wrote into its workspace `ws` (uint8 tensor of rgb_entries_workspace_bytes; S entries, n_chunks
    chunks), once the stream is done: the workspace ends with the plan arrays and, behind them, every entry's final chunk, each rounded up
    to 256 bytes.  -> (pixbase (S,), hw (S,), pix0 (n_chunks, S), npix (n_chunks, S), table_off (n_chunks, S), final chunk (S,)) numpy."""
    def up(v):
        return -(-v // 256) * 256
    n_tab = (2 + 3 * n_chunks) * S * 8
    a = ws.numel() - up(4 * S) - up(n_tab)
    t = ws[a:a + n_tab].view(torch.int64).cpu().numpy()
    final = ws[ws.numel() - up(4 * S):][:4 * S].view(torch.int32).cpu().numpy()
    per = n_chunks * S
    return (t[:S], t[S:2 * S], t[2 * S:2 * S + per].reshape(n_chunks, S), t[2 * S + per:2 * S + 2 * per].reshape(n_chunks, S),
            t[2 * S + 2 * per:].reshape(n_chunks, S), final)


def decode_rgb_entries(P_ragged, targets, sym_ragged, buf, offs_host, lens_host, pixbase, hw, pix0, length, n_chunks, K, lag, window_mode,
                       side_stream=None, limit=ENTRIES_MAX):
    """An RGB scale as S arbitrary ENTRIES in lock step (l3c_decode_rgb_entries: every band of every image of a set of banded files):
    entry e (int64 arrays of S) is pixels [pix0, pix0 + length) of an image of hw pixels at pixel pixbase of P_ragged ((total_pix, 120)
    fp32) and of sym_ragged (int16 (3 * total_pix,), ZEROED); the streams in `buf` at offs_host / lens_host, numpy (3, S): stream (c, e).
    More than `limit` entries go through the call in slices.  -> tensors to keep alive until the stream is done."""
    S = len(hw)
    total_pix = P_ragged.numel() // (12 * K)
    ent = np.stack([np.asarray(a, dtype=np.int64) for a in (pixbase, hw, pix0, length)])
    keep = []
    for a, e in entry_slices(S, limit):
        ent_h = np.ascontiguousarray(ent[:, a:e]).reshape(-1)
        nbytes = rgb_entries_workspace_bytes(ent[3, a:e], n_chunks, lag)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=P_ragged.device)
        ent_d = upload_small(ent_h)
        offs = upload_small(np.ascontiguousarray(offs_host[:, a:e], dtype=np.int64).reshape(-1))
        lens = upload_small(np.ascontiguousarray(lens_host[:, a:e], dtype=np.int32).reshape(-1))
        desc = _lib.RgbEntriesDesc(ptr(P_ragged, torch.float32), ptr(targets, torch.float32), ptr(sym_ragged, torch.int16), e - a, total_pix,
                                   ptr(ent_d, torch.int64), ent_h.ctypes.data_as(ctypes.POINTER(_lib.c_i64)), K, ptr(buf, torch.uint8),
                                   ptr(offs, torch.int64), ptr(lens, torch.int32), n_chunks, lag, window_mode, ptr(ws), nbytes)
        _run_rgb_pipeline('l3c_decode_rgb_entries', desc, lag, side_stream, (P_ragged, targets, sym_ragged, buf, offs, lens, ws, ent_d))
        keep.append((ws, ent_d, offs, lens))
    return keep


def band_intervals(iv, n_streams, n_sym, band_len):
    """l3c_ac_band_intervals: the interval buffer of n_streams streams -> [(iv, n_streams, n_sym)] groups for ac_encode_groups: the full
    bands (stream s * (n - 1) + j; absent when n == 1), then the last band of every stream."""
    lib = _lib.load()
    n = -(-n_sym // band_len)
    last = n_sym - (n - 1) * band_len
    full = (torch.empty(lib.l3c_interval_words(n_streams * (n - 1), band_len), dtype=torch.int32, device=iv.device) if n > 1 else None)
    tail = torch.empty(lib.l3c_interval_words(n_streams, last), dtype=torch.int32, device=iv.device)
    call('l3c_ac_band_intervals', ptr(iv, torch.int32), n_streams, n_sym, band_len, ptr(full), ptr(tail), stream())
    return ([(full, n_streams * (n - 1), band_len)] if n > 1 else []) + [(tail, n_streams, last)]


CONTAINER_READ_MAX_STREAMS = 65535     # l3c_container_read: one grid row per stream (grid.y)


def container_read(files_dev, src_off, dst_off, nbytes, max_nbytes, dst):
    """l3c_container_read: the streams of many raw `.l3c` files (one device buffer) -> 4-byte aligned, zero padded streams in `dst`;
    in slices of at most 65 535 streams (a banded batch easily holds more)."""
    S = nbytes.numel()
    for a in range(0, S, CONTAINER_READ_MAX_STREAMS):
        e = min(S, a + CONTAINER_READ_MAX_STREAMS)
        call('l3c_container_read', ptr(files_dev, torch.uint8), ptr(src_off[a:e], torch.int64), ptr(dst_off[a:e], torch.int64),
             ptr(nbytes[a:e], torch.int32), e - a, int(max_nbytes), ptr(dst, torch.uint8), stream())


def dmll_encode_intervals(P_nhwc, sym, targets, C, K, rgb):
    """P (B,H,W,Kp), sym int16 (B,C,H,W) -> packed interval words for the B*C streams of this scale."""
    B, H, W, _ = P_nhwc.shape
    Lp = targets.shape[0]
    n = _lib.load().l3c_interval_words(B * C, H * W)
    iv = torch.empty(n, dtype=torch.int32, device=P_nhwc.device)
    call('l3c_dmll_encode_intervals', ptr(P_nhwc, torch.float32), ptr(sym, torch.int16), ptr(targets, torch.float32),
         B, H * W, C, K, int(rgb), Lp, ptr(iv), stream())
    return iv


def dmll_nll(P_nhwc, x, C, K, rgb, x_min, x_max, L):
    """x (B,C,H,W) fp32 targets -> nll (B,C,H,W) in nats."""
    B, H, W, _ = P_nhwc.shape
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=P_nhwc.device)
    call('l3c_dmll_nll', ptr(P_nhwc, torch.float32), ptr(x, torch.float32), B, H * W, C, K, int(rgb), float(x_min),
         float(x_max), L, ptr(out), stream())
    return out


def dmll_sample(P_nhwc, u_mix, u_log, C, K, rgb):
    """P (B,H,W,Kp); u_mix (B,C,K,H,W), u_log (B,C,H,W) uniforms in (0,1) -> x fp32 (B,C,H,W), not rounded."""
    B, H, W, _ = P_nhwc.shape
    assert tuple(u_mix.shape) == (B, C, K, H, W) and tuple(u_log.shape) == (B, C, H, W), (u_mix.shape, u_log.shape)
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=P_nhwc.device)
    call('l3c_dmll_sample', ptr(P_nhwc, torch.float32), ptr(u_mix, torch.float32), ptr(u_log, torch.float32), B, H * W, C, K,
         int(rgb), ptr(out), stream())
    return out


def dmll_mean(P_nhwc, C, K, rgb, x_min, x_max, L):
    """P (B,H,W,Kp) -> int16 symbols (B,C,H,W) of the mixture's mean, channel by channel (the preview decode's estimator: l3c_dmll_mean)."""
    B, H, W, _ = P_nhwc.shape
    out = torch.empty(B, C, H, W, dtype=torch.int16, device=P_nhwc.device)
    call('l3c_dmll_mean', ptr(P_nhwc, torch.float32), B, H * W, C, K, int(rgb), float(x_min), float(x_max), int(L), ptr(out), stream())
    return out


CONCEAL_SPAN_DTYPE = np.dtype([('image', '<i8'), ('pix0', '<i8'), ('npix', '<i8'), ('replace', '<u4'), ('reserved', '<u4')])      # l3c_conceal_span


def conceal_spans(spans):
    """[(image, pix0, npix, replace mask), ...] -> the host table of l3c_dmll_conceal (CONCEAL_SPAN_DTYPE)."""
    table = np.zeros(len(spans), dtype=CONCEAL_SPAN_DTYPE)
    for i, (image, pix0, npix, replace) in enumerate(spans):
        table[i] = (image, pix0, npix, replace, 0)
    return table


def dmll_conceal(P, sym, spans, K, x_min, x_max, L):
    """l3c_dmll_conceal, in place on `sym`: P (B,H,W,12 K) fp32 or a device pointer to it, sym int16 (B,3,H,W) contiguous, spans a list of
    (image, pix0, npix, replace mask) or a CONCEAL_SPAN_DTYPE array -- pixels [pix0, pix0 + npix) of image `image`, pix0 a multiple of 64;
    the channels whose bit of the mask is set take the snapped mean of the mixture, conditioned on the channels that are kept.  The table
    is checked on the host and goes up through upload_small.  One launch, no host synchronisation; no spans: nothing is called."""
    table = spans if isinstance(spans, np.ndarray) else conceal_spans(spans)
    if table.dtype != CONCEAL_SPAN_DTYPE or table.ndim != 1:
        raise ValueError('dmll_conceal: spans must be a 1-d array of CONCEAL_SPAN_DTYPE, got {} {}'.format(table.dtype, table.shape))
    B, C, H, W = sym.shape
    if sym.dtype != torch.int16 or C != 3 or not sym.is_contiguous():
        raise ValueError('dmll_conceal: sym must be a contiguous int16 (B,3,H,W) tensor, got {} {}'.format(sym.dtype, tuple(sym.shape)))
    if isinstance(P, torch.Tensor):
        if tuple(P.shape) != (B, H, W, 12 * K):
            raise ValueError('dmll_conceal: P {} beside sym {} at K = {}'.format(tuple(P.shape), tuple(sym.shape), K))
        P = ptr(P, torch.float32)
    if not len(table):
        return sym
    table = np.ascontiguousarray(table)
    table_d = upload_small(table.view(np.int64))
    call('l3c_dmll_conceal', P, B, H * W, int(K), float(x_min), float(x_max), int(L), table.ctypes.data, ptr(table_d, torch.int64), len(table),
         ptr(sym, torch.int16), stream())
    return sym


# ---- arithmetic coder -------------------------------------------------------------------------------------------------


def intervals_from_table(cdf, sym, n_streams, n_sym, broadcast_row=False):
    """cdf int16/uint16: (n_streams*n_sym, Lp) rows, or one row (Lp,) with broadcast_row; sym int16 (n_streams, n_sym)."""
    Lp = cdf.shape[-1]
    n = _lib.load().l3c_interval_words(n_streams, n_sym)
    iv = torch.empty(n, dtype=torch.int32, device=sym.device)
    call('l3c_ac_intervals_from_table', ptr(cdf), 0 if broadcast_row else Lp, Lp, ptr(sym, torch.int16), n_streams,
         n_sym, ptr(iv), stream())
    return iv


def ac_encode(iv, n_streams, n_sym):
    """-> (out uint8 (n_streams, stride), nbytes int32 (n_streams,)) on the device.  `iv` is clobbered."""
    stride = _lib.load().l3c_ac_max_bytes(n_sym)
    out = torch.empty(n_streams, stride, dtype=torch.uint8, device=iv.device)
    nbytes = torch.empty(n_streams, dtype=torch.int32, device=iv.device)
    ws = torch.empty(_lib.load().l3c_ac_encode_workspace_bytes(n_streams), dtype=torch.uint8, device=iv.device)
    call('l3c_ac_encode', ptr(iv), n_streams, n_sym, ptr(out), stride, ptr(nbytes), ptr(ws), stream())
    return out, nbytes


def ac_encode_groups(groups):
    """groups: list of (iv, n_streams, n_sym).  ONE state launch + ONE pack launch code every stream of every group
    concurrently.  -> list of (out uint8 (n_streams, stride), nbytes int32 (n_streams,)); the iv buffers are clobbered."""
    lib = _lib.load()
    arr = (_lib.AcGroup * len(groups))()
    res = []
    total = 0
    for g, (iv, n_streams, n_sym) in enumerate(groups):
        stride = lib.l3c_ac_max_bytes(n_sym)
        out = torch.empty(n_streams, stride, dtype=torch.uint8, device=iv.device)
        nbytes = torch.empty(n_streams, dtype=torch.int32, device=iv.device)
        arr[g] = _lib.AcGroup(ptr(iv), ptr(out), ptr(nbytes), n_streams, n_sym, stride)
        res.append((out, nbytes))
        total += n_streams
    ws = torch.empty(lib.l3c_ac_encode_groups_workspace_bytes(len(groups), total), dtype=torch.uint8, device=groups[0][0].device)
    call('l3c_ac_encode_groups', arr, len(groups), ptr(ws), stream())
    return res, ws


def pack_streams(payloads, device='cuda'):
    """list of bytes -> (uint8 buffer with every stream 4-byte aligned and zero padded, offsets int64, nbytes int32)."""
    offs, pos = [], 0
    for p in payloads:
        offs.append(pos)
        pos += (len(p) + 3) // 4 * 4 + 4
    buf = np.zeros(max(pos, 4), dtype=np.uint8)
    for o, p in zip(offs, payloads):
        buf[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return (torch.from_numpy(buf).to(device), torch.tensor(offs, dtype=torch.int64, device=device),
            torch.tensor([len(p) for p in payloads], dtype=torch.int32, device=device))


def ac_decode(cdf, payload_buf, offsets, nbytes, n_streams, n_sym, monotone, broadcast_row=False):
    """-> sym int16 (n_streams, n_sym) on the device."""
    Lp = cdf.shape[-1]
    sym = torch.empty(n_streams, n_sym, dtype=torch.int16, device=payload_buf.device)
    call('l3c_ac_decode', ptr(cdf), 0 if broadcast_row else Lp, Lp, ptr(payload_buf, torch.uint8),
         ptr(offsets, torch.int64), ptr(nbytes, torch.int32), n_streams, n_sym, int(bool(monotone)), ptr(sym), stream())
    return sym


def ac_decode_state(n_streams, device='cuda'):
    """Opaque per-stream coder state carried between the chunks of l3c_ac_decode_chunk."""
    return torch.empty(n_streams * _lib.load().l3c_ac_decode_state_bytes(), dtype=torch.uint8, device=device)


def ac_decode_part(cdf, payload_buf, offsets, nbytes, n_streams, n_sym, flag, state_in, state_out, final, sym_out,
                   sym_stride, sym_offset, window=None):
    """One part of `ac_decode_chunks`: decode symbols [sym_offset, sym_offset + n_sym) of every stream from the table rows of
    that range (cdf: (n_streams * n_sym, Lp)), resuming from `state_in` (None: start of the streams) and saving into
    `state_out`; writes into `sym_out` (int16, row stride `sym_stride`).  `flag`: device int32 'table not validated'
    (None: treat as not validated).  The tuple keeps the tensors alive until the launch.
    window: None, or (stats_in, stats_out, P_nhwc, sym_all, targets, pix0, C, K, c) for a table built with `dmll_cdf_table(...,
    window_stats=stats_in)`: streams whose rows are window rows are decoded from those, a symbol outside its window from the pixel's
    full row evaluated by the decoder itself (needs P, the decoded channels `sym_all` (B, C, H, W) and the bin edges); stats_out
    (int32 (B,)) receives every stream's miss count of this chunk."""
    part = _lib.AcDecodePart(ptr(cdf), cdf.shape[-1], ptr(payload_buf, torch.uint8), ptr(offsets, torch.int64),
                             ptr(nbytes, torch.int32), n_streams, n_sym,
                             ptr(flag, torch.int32) if flag is not None else None,
                             ptr(state_in) if state_in is not None else None,
                             ptr(state_out) if state_out is not None else None, int(bool(final)),
                             ptr(sym_out, torch.int16), sym_stride, sym_offset)
    keep = (cdf, payload_buf, offsets, nbytes, flag, state_in, state_out, sym_out)
    if window is not None:
        stats_in, stats_out, P_nhwc, sym_all, targets, pix0, C, K, c = window
        part.window_stats_in, part.window_stats_out = ptr(stats_in, torch.int32), ptr(stats_out, torch.int32)
        part.P, part.sym_all, part.targets = ptr(P_nhwc, torch.float32), ptr(sym_all, torch.int16), ptr(targets, torch.float32)
        part.HW, part.pix0 = P_nhwc.shape[1] * P_nhwc.shape[2], pix0
        part.C, part.K, part.c = C, K, c
        keep += (stats_in, stats_out, P_nhwc, sym_all, targets)
    return part, keep


def ac_decode_chunks(parts):
    """1..8 independent parts (see ac_decode_part) decoded side by side in one launch pair."""
    arr = (_lib.AcDecodePart * len(parts))(*[p for p, _ in parts])
    call('l3c_ac_decode_chunks', arr, len(parts), stream())


def table_is_monotone(cdf):
    """Host-synchronising check (used by the generic torchac.decode_cdf path on user tables)."""
    Lp = cdf.shape[-1]
    flag = torch.zeros(1, dtype=torch.int32, device=cdf.device)
    call('l3c_cdf_check_monotone', ptr(cdf), cdf.numel() // Lp, Lp, ptr(flag), stream())
    return int(flag.item()) == 0


def u8_crc32_tile():
    """(bytes one thread folds, bytes one block folds) of l3c_u8_crc32."""
    t, s = ctypes.c_int(), ctypes.c_int()
    call('l3c_u8_crc32_tile', ctypes.byref(t), ctypes.byref(s))
    return t.value, s.value


def u8_crc32(data, n_items, item_bytes, item_stride=None, out=None, workspace=None):
    """l3c_u8_crc32: zlib.crc32 of the n_items runs of item_bytes bytes that start item_stride bytes apart (default: back to back) in the
    contiguous uint8 device tensor `data` -> int32 (n_items,) device tensor holding the CRC words (view it as uint32 on the host); no
    host synchronisation."""
    item_stride = item_bytes if item_stride is None else item_stride
    if data.dtype != torch.uint8 or n_items < 1 or item_bytes < 0 or data.numel() < (n_items - 1) * item_stride + item_bytes:
        raise ValueError('u8_crc32: {} items of {} bytes, {} apart, do not fit a {} tensor of {} elements'.format(
            n_items, item_bytes, item_stride, data.dtype, data.numel()))
    n_ws = _lib.load().l3c_u8_crc32_workspace_bytes(n_items, item_bytes)
    _lib.check(min(n_ws, 0))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=data.device) if workspace is None else workspace
    out = torch.empty(n_items, dtype=torch.int32, device=data.device) if out is None else out
    call('l3c_u8_crc32', ptr(data, torch.uint8), n_items, item_bytes, item_stride, ptr(out, torch.int32), ptr(ws, torch.uint8), ws.numel(), stream())
    return out


SPAN_DTYPE = np.dtype([('offset', '<i8'), ('bytes', '<i8')])      # l3c_u8_span (include/l3c_hip.h)


def u8_crc32_spans(data, offsets, lengths, out=None, workspace=None):
    """l3c_u8_crc32_spans: zlib.crc32 of data[offsets[i]:offsets[i] + lengths[i]] for every i, in one call of at most three launches -- the
    frames of a ragged group.  data: contiguous uint8 device tensor; offsets (multiples of 4), lengths: host sequences or int64 arrays of
    one length n >= 1; the spans may come in any order, overlap and leave gaps.  The table is checked on the host and goes up through
    upload_small.  -> int32 (n,) device tensor holding the CRC words (view it as uint32 on the host); no host synchronisation."""
    offsets, lengths = np.asarray(offsets), np.asarray(lengths)
    if data.dtype != torch.uint8 or not data.is_contiguous() or offsets.ndim != 1 or offsets.shape != lengths.shape or offsets.shape[0] < 1 \
            or offsets.dtype.kind not in 'iu' or lengths.dtype.kind not in 'iu':
        raise ValueError('u8_crc32_spans: a contiguous uint8 tensor and two integer sequences of one length >= 1, got {} and {} / {}'.format(
            data.dtype, offsets.shape, lengths.shape))
    table = np.empty(offsets.shape[0], dtype=SPAN_DTYPE)
    table['offset'], table['bytes'] = offsets, lengths
    n = table.shape[0]
    n_ws = _lib.load().l3c_u8_crc32_spans_workspace_bytes(table.ctypes.data, n)
    _lib.check(min(n_ws, 0))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=data.device) if workspace is None else workspace
    out = torch.empty(n, dtype=torch.int32, device=data.device) if out is None else out
    if out.dtype != torch.int32 or out.numel() != n or not out.is_contiguous():
        raise ValueError('u8_crc32_spans: out must be a contiguous int32 tensor of {} elements'.format(n))
    table_d = upload_small(table.view(np.int64))
    call('l3c_u8_crc32_spans', ptr(data, torch.uint8), data.numel(), table.ctypes.data, ptr(table_d, torch.int64), n, ptr(out, torch.int32),
         ptr(ws, torch.uint8), ws.numel(), stream())
    return out


def seal_append(files, file_bytes, frame_crc, padding=None, model_id=0):
    """l3c_seal_append: this build's seal behind every file of an encode, in place.  files uint8 (B, file_stride), file_bytes int64 (B,),
    frame_crc int32 (B,) (u8_crc32 of the padded frames), padding int16 (B, 4) device tensor or None -- all on the device."""
    B, stride = files.shape
    call('l3c_seal_append', ptr(files, torch.uint8), stride, ptr(file_bytes, torch.int64), ptr(frame_crc, torch.int32), ptr(padding, torch.int16),
         int(model_id), B, stream())


def u8_crc32_bands(frames, n_frames, plane_bytes, band_bytes, planes=3, frame_stride=None, frame_crc=True, workspace=None):
    """l3c_u8_crc32_bands: zlib.crc32 of every band of every plane of n_frames frames -- band j of a plane is its bytes
    [j band_bytes, min((j + 1) band_bytes, plane_bytes)) -- and of every frame, the bytes read once, in two launches.  frames: contiguous
    uint8 device tensor, frame f at f * frame_stride (default: back to back).  -> (int32 (n_frames, planes, n), int32 (n_frames,) or None
    with frame_crc=False) device tensors holding the CRC words (view them as uint32 on the host); no host synchronisation."""
    frame_stride = planes * plane_bytes if frame_stride is None else frame_stride
    if frames.dtype != torch.uint8 or not frames.is_contiguous() or n_frames < 1 or planes < 1 or plane_bytes < 1 or band_bytes < 1 \
            or frames.numel() < (n_frames - 1) * frame_stride + planes * plane_bytes:
        raise ValueError('u8_crc32_bands: {} frames of {} planes of {} bytes, {} apart, do not fit a {} tensor of {} elements'.format(
            n_frames, planes, plane_bytes, frame_stride, frames.dtype, frames.numel()))
    n_ws = _lib.load().l3c_u8_crc32_bands_workspace_bytes(n_frames, planes, plane_bytes, band_bytes)
    _lib.check(min(n_ws, 0))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=frames.device) if workspace is None else workspace
    n = -(-plane_bytes // band_bytes)
    bands = torch.empty((n_frames, planes, n), dtype=torch.int32, device=frames.device)
    whole = torch.empty(n_frames, dtype=torch.int32, device=frames.device) if frame_crc else None
    call('l3c_u8_crc32_bands', ptr(frames, torch.uint8), n_frames, planes, plane_bytes, band_bytes, frame_stride, ptr(bands, torch.int32),
         ptr(whole, torch.int32), ptr(ws, torch.uint8), ws.numel(), stream())
    return bands, whole


def seal_append_bands(files, file_bytes, frame_crc, band_crc, band_len, padding=None, model_id=0):
    """l3c_seal_append_bands: the band table and this build's version-2 seal behind every file of a banded encode, in place.  files uint8
    (B, file_stride), file_bytes int64 (B,), frame_crc int32 (B,) and band_crc int32 (B, 3, n) (u8_crc32_bands of the padded frames),
    padding int16 (B, 4) device tensor or None -- all on the device."""
    B, stride = files.shape
    if band_crc.dim() != 3 or band_crc.shape[0] != B or band_crc.shape[1] != 3 or not band_crc.is_contiguous():
        raise ValueError('seal_append_bands: band_crc must be a contiguous (B, 3, n) tensor, got {}'.format(tuple(band_crc.shape)))
    call('l3c_seal_append_bands', ptr(files, torch.uint8), stride, ptr(file_bytes, torch.int64), ptr(frame_crc, torch.int32),
         ptr(band_crc, torch.int32), band_crc.shape[2], int(band_len), ptr(padding, torch.int16), int(model_id), B, stream())


def banded_scale_desc(C, H, W, L, groups):
    """l3c_banded_scale of one record of a banded encode: groups = [(out, nbytes) of the full bands (absent when n == 1), of the last bands],
    the results of ac_encode_groups on band_intervals."""
    (out_f, nb_f), (out_l, nb_l) = (groups[0] if len(groups) == 2 else (None, None)), groups[-1]
    return _lib.BandedScale(ptr(out_f, torch.uint8), ptr(nb_f, torch.int32), out_f.shape[1] if out_f is not None else 0,
                            ptr(out_l, torch.uint8), ptr(nb_l, torch.int32), out_l.shape[1], C, H, W, L)


def _band_parity(name, B, H, W, L, groups, G, R, out):
    """band_parity (R None: l3c_band_parity, slots (B, 3, m, stride)) and band_parity_rs (l3c_band_parity_rs, slots (B, 3, m, R, stride))."""
    n = -(-(H * W) // L)
    m = _lib.load().l3c_band_parity_groups(n, int(G))
    _lib.check(min(m, 0))
    lead = (B, 3, m) if R is None else (B, 3, m, int(R))
    dev = groups[-1][0].device
    if out is None:
        stride = -(-max(g[0].shape[1] for g in groups) // 16) * 16
        out = (torch.empty(lead + (stride,), dtype=torch.uint8, device=dev), torch.empty((B, 3, m), dtype=torch.int32, device=dev))
    parity, nbytes = out
    if tuple(parity.shape[:-1]) != lead or tuple(nbytes.shape) != (B, 3, m):
        if R is None:
            raise ValueError('band_parity: out must be (B, 3, m, stride) and (B, 3, m) with m = {}, got {} and {}'.format(
                m, tuple(parity.shape), tuple(nbytes.shape)))
        raise ValueError('band_parity_rs: out must be (B, 3, m, R, stride) and (B, 3, m) with m = {}, R = {}, got {} and {}'.format(
            m, int(R), tuple(parity.shape), tuple(nbytes.shape)))
    desc = banded_scale_desc(3, H, W, L, groups)
    call(name, ctypes.byref(desc), B, int(G), *(() if R is None else (int(R),)), ptr(parity, torch.uint8), parity.shape[-1], ptr(nbytes, torch.int32),
         stream())
    return parity, nbytes


def band_parity(B, H, W, L, groups, G, out=None):
    """l3c_band_parity: the XOR parity of the finest record's band payloads (3 channels; `groups` as banded_scale_desc takes them), bands
    { j : j % m == g } of a channel in group g, m = ceil(n / G) -> (parity uint8 (B, 3, m, stride), nbytes int32 (B, 3, m)) on the device:
    bytes [0, nbytes) of a slot are the parity payload (the bytes behind its 4-byte-rounded length are not written), nbytes -1 where a
    member overran.  out: (parity, nbytes) tensors of the caller's instead of new ones.  No host synchronisation."""
    return _band_parity('l3c_band_parity', B, H, W, L, groups, G, None, out)


def band_parity_rs(B, H, W, L, groups, G, R, out=None):
    """l3c_band_parity_rs: band_parity with R rows per group over GF(2^8) (container.rs_parity is the reference; row 0 is band_parity's
    payload) -> (parity uint8 (B, 3, m, R, stride), nbytes int32 (B, 3, m)) on the device: one length for the R rows of a group, -1 where a
    member overran (none of the group's slots is written then).  R in 1..4; G <= 255 when R > 1.  No host synchronisation."""
    return _band_parity('l3c_band_parity_rs', B, H, W, L, groups, G, R, out)


HEAD_MAX_RECORDS = 8      # csrc/parity_plan.h: the records of one l3c_head_parity / l3c_band_payload_crc32 call


def _banded_scale_array(scales):
    """scales: [(C, H, W, L, groups)] records of a banded encode (groups as banded_scale_desc takes them) -> the l3c_banded_scale array."""
    arr = (_lib.BandedScale * len(scales))()
    for k, (C, H, W, L, groups) in enumerate(scales):
        arr[k] = banded_scale_desc(C, H, W, L, groups)
    return arr


def head_parity_layout(B, scales, G, R):
    """The slots of head_parity for those records -> (per record (C, n, m), per record its byte offset in the slot buffer, stride, bytes of
    the buffer, lengths in front of every record + their total): record k's slots are uint8 (B, C_k, m_k, R, stride) at its offset, its
    lengths int32 (B, C_k, m_k) at its place in the length array; G_k = min(G, n_k), m_k = ceil(n_k / G_k)."""
    shapes, offsets, first, at = [], [], [0], 0
    stride = -(-max(g[0].shape[1] for s in scales for g in s[4]) // 16) * 16
    for C, H, W, L, groups in scales:
        n = -(-(H * W) // L)
        m = -(-n // min(int(G), n))
        shapes.append((C, n, m))
        offsets.append(at)
        at += B * C * m * int(R) * stride
        first.append(first[-1] + B * C * m)
    return shapes, offsets, stride, at, first


def head_parity(B, scales, G, R, out=None):
    """l3c_head_parity: band_parity_rs over SEVERAL records of any C in ONE launch (the head records of a batch: every record but the
    finest).  scales: [(C, H, W, L, groups)], at most 8 -> (parity uint8 (bytes,), nbytes int32 (total,)) on the device, laid out as
    head_parity_layout says; nbytes -1 where a member overran (none of the group's slots is written then).  out: (parity, nbytes) tensors
    of the caller's, parity 16-byte aligned.  No host synchronisation."""
    shapes, offsets, stride, total, first = head_parity_layout(B, scales, G, R)
    dev = scales[0][4][-1][0].device
    if out is None:
        out = (torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(first[-1], dtype=torch.int32, device=dev))
    parity, nbytes = out
    if parity.dtype != torch.uint8 or nbytes.dtype != torch.int32 or parity.numel() != total or nbytes.numel() != first[-1] \
            or not parity.is_contiguous() or not nbytes.is_contiguous():
        raise ValueError('head_parity: out must be contiguous uint8 ({},) and int32 ({},) tensors, got {} and {}'.format(
            total, first[-1], tuple(parity.shape), tuple(nbytes.shape)))
    arr = _banded_scale_array(scales)
    offs = (ctypes.c_int64 * len(scales))(*offsets)
    call('l3c_head_parity', arr, len(scales), B, int(G), int(R), ptr(parity, torch.uint8), offs, stride, ptr(nbytes, torch.int32), stream())
    return parity, nbytes


def band_payload_crc32(B, scales, out=None):
    """l3c_band_payload_crc32: zlib.crc32 of every band payload of those records (scales as head_parity takes them), the lengths read on the
    device -> int32 (sum of B C_k n_k,) device tensor, record-major then (b, c, j); view it as uint32 on the host.  A payload of length 0 gives
    0, and so does an overrun band.  No host synchronisation."""
    total = sum(B * C * -(-(H * W) // L) for C, H, W, L, _ in scales)
    dev = scales[0][4][-1][0].device
    out = torch.empty(total, dtype=torch.int32, device=dev) if out is None else out
    if out.dtype != torch.int32 or out.numel() != total or not out.is_contiguous():
        raise ValueError('band_payload_crc32: out must be a contiguous int32 tensor of {} elements'.format(total))
    call('l3c_band_payload_crc32', _banded_scale_array(scales), len(scales), B, ptr(out, torch.int32), stream())
    return out


def seal_append_parity(files, file_bytes, frame_crc, band_crc, scales, G, R, parity, padding=None, model_id=0, head=None, workspace=None):
    """l3c_seal_append_parity: section ('L3CP' / 'L3CQ', with `head` 'L3CH'), band table and this build's version-3 seal behind every file
    of a banded encode, in place -- container.make_seal's bytes, assembled on the device.  files uint8 (B, file_stride), file_bytes int64
    (B,), frame_crc int32 (B,) and band_crc int32 (B, 3, n) (u8_crc32_bands of the padded frames); scales: [(C, H, W, L, groups)], ALL
    records of the files, coarsest first, as head_parity takes them; parity: (slots, nbytes) of band_parity_rs on the finest record with
    min(G, n) and R; head: None, or (band_payload_crc32, head_parity slots, head_parity nbytes) over scales[:-1] with G and R.  padding int16
    (B, 4) device tensor or None.  No host synchronisation."""
    B, stride = files.shape
    slots, nbytes = parity
    arr = _banded_scale_array(scales)
    n_ws = _lib.load().l3c_seal_append_parity_workspace_bytes(arr, len(scales), B, int(G), int(R), int(head is not None))
    _lib.check(min(n_ws, 0))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=files.device) if workspace is None else workspace
    d = _lib.SealParityDesc()
    d.files, d.file_stride, d.file_bytes, d.B = ptr(files, torch.uint8), stride, ptr(file_bytes, torch.int64), B
    d.scales_host, d.n_scales = arr, len(scales)
    d.G, d.R, d.head, d.reserved = int(G), int(R), int(head is not None), 0
    d.padding, d.model_id = ptr(padding, torch.int16), int(model_id)
    d.frame_crc, d.band_crc = ptr(frame_crc, torch.int32), ptr(band_crc, torch.int32)
    d.parity, d.parity_stride, d.parity_nbytes = ptr(slots, torch.uint8), slots.shape[-1], ptr(nbytes, torch.int32)
    if head is not None:
        crcs, hslots, hnbytes = head
        _, offsets, hstride, _, _ = head_parity_layout(B, scales[:-1], G, R)
        offs = (ctypes.c_int64 * len(offsets))(*offsets)
        d.head_parity, d.head_parity_offset_host, d.head_parity_stride = ptr(hslots, torch.uint8), offs, hstride
        d.head_parity_nbytes, d.payload_crc = ptr(hnbytes, torch.int32), ptr(crcs, torch.int32)
    d.workspace, d.workspace_bytes = ptr(ws, torch.uint8), ws.numel()
    call('l3c_seal_append_parity', ctypes.byref(d), stream())


def _u8_spans(name, data, offsets, lengths, coefs, group_first, out, out_offsets, out_lengths):
    """u8_xor_spans (coefs None: l3c_u8_xor_spans) and u8_gf_spans (l3c_u8_gf_spans): the span, slot and group tables, and the coefficients
    where there are any, checked and uploaded as ONE table, then the call."""
    group_first = np.ascontiguousarray(group_first, dtype=np.int64)
    n_groups = group_first.shape[0] - 1
    if n_groups <= 0:
        return out
    spans = np.zeros(len(offsets), dtype=SPAN_DTYPE)
    spans['offset'], spans['bytes'] = offsets, lengths
    slots = np.zeros(n_groups, dtype=SPAN_DTYPE)
    slots['offset'], slots['bytes'] = out_offsets, out_lengths
    parts = [spans.view(np.int64), slots.view(np.int64), group_first]            # the 8-byte tables in front, each 8-byte aligned
    if coefs is not None:
        coef = np.asarray(coefs, dtype=np.int64).reshape(-1)
        if coef.shape[0] != spans.shape[0] or (coef.size and (coef.min() < 0 or coef.max() > 255)):
            raise ValueError('u8_gf_spans: one coefficient in 0..255 per span')
        coef8 = np.zeros(-(-coef.shape[0] // 8) * 8, dtype=np.uint8)              # padded to whole words
        coef8[:coef.shape[0]] = coef
        parts.append(coef8.view(np.int64))
    if data.dtype != torch.uint8 or out.dtype != torch.uint8 or not data.is_contiguous() or not out.is_contiguous():
        raise ValueError('{}: data and out must be contiguous uint8 tensors'.format(name[4:]))
    table_d = upload_small(np.concatenate(parts))
    a, b, c = 2 * spans.shape[0], 2 * spans.shape[0] + 2 * n_groups, 2 * spans.shape[0] + 3 * n_groups + 1
    coef_args = () if coefs is None else (coef8.ctypes.data, ptr(table_d[c:], torch.int64) if a else None)
    call(name, ptr(data, torch.uint8), data.numel(), spans.ctypes.data, ptr(table_d[:a], torch.int64) if a else None, *coef_args, spans.shape[0],
         group_first.ctypes.data, ptr(table_d[b:c], torch.int64), n_groups, slots.ctypes.data, ptr(table_d[a:b], torch.int64),
         ptr(out, torch.uint8), out.numel(), stream())
    return out


def u8_xor_spans(data, offsets, lengths, group_first, out, out_offsets, out_lengths):
    """l3c_u8_xor_spans: slot g of `out` -- bytes [out_offsets[g], ...) -- receives the XOR of the spans data[offsets[k]:offsets[k] +
    lengths[k]], k in [group_first[g], group_first[g + 1]), each cut or zero-extended to out_lengths[g], then zero bytes up to
    ((out_lengths[g] + 3) // 4) * 4 + 4.  data, out: contiguous uint8 device tensors that do not overlap; the tables: host integer sequences
    (offsets multiples of 4), checked on the host, uploaded through upload_small.  No groups: nothing is launched.  No host synchronisation."""
    return _u8_spans('l3c_u8_xor_spans', data, offsets, lengths, None, group_first, out, out_offsets, out_lengths)


def u8_gf_spans(data, offsets, lengths, coefs, group_first, out, out_offsets, out_lengths):
    """l3c_u8_gf_spans: u8_xor_spans with one GF(2^8) coefficient per span (polynomial 0x11D): slot g receives the XOR over its spans k of
    coefs[k] * data[offsets[k]:offsets[k] + lengths[k]], cut or zero-extended and zero-padded as u8_xor_spans does.  coefs: host integers
    0..255, one per span; a span with coefficient 0 is not read.  No groups: nothing is launched.  No host synchronisation."""
    return _u8_spans('l3c_u8_gf_spans', data, offsets, lengths, coefs, group_first, out, out_offsets, out_lengths)


REBUILD_GROUP_DTYPE = np.dtype([('first_src', '<i8'), ('n_rows', '<i4'), ('n_members', '<i4'), ('t', '<i4'), ('reserved', '<i4'),
                                ('out', SPAN_DTYPE, (4,))])      # l3c_rebuild_group (include/l3c_hip.h)


def band_rebuild(rows, members, offsets, lengths, coefs, groups):
    """l3c_band_rebuild: every erased member of a group in one pass, in place.  rows: contiguous uint8 device tensor holding the parity rows at
    ANY byte offsets; members: contiguous uint8 device tensor that holds the member sources (offsets multiples of 4) and receives the outputs.
    offsets, lengths: one span per source; coefs: (n_src, 4) host integers 0..255, coefs[k][e] the weight of source k in output e.  groups:
    [(first_src, n_rows, n_members, [(out_offset, out_bytes)] * t)] -- the group's n_rows row sources first (spans of `rows`), then its
    n_members member sources (spans of `members`); output e is the XOR over the sources k of coefs[k][e] * source k over GF(2^8), cut or
    zero-extended to out_bytes, then zero bytes up to ((out_bytes + 3) // 4) * 4 + 4.  A slot that overlaps a member source or another slot is
    refused.  The tables are checked on the host and go up as ONE table through upload_small.  No groups: nothing is launched.  No host
    synchronisation."""
    if not groups:
        return members
    if rows.dtype != torch.uint8 or members.dtype != torch.uint8 or not rows.is_contiguous() or not members.is_contiguous():
        raise ValueError('band_rebuild: rows and members must be contiguous uint8 tensors')
    src = np.zeros(len(offsets), dtype=SPAN_DTYPE)
    src['offset'], src['bytes'] = offsets, lengths
    coef = np.asarray(coefs, dtype=np.int64).reshape(-1, 4)
    if coef.shape[0] != src.shape[0] or (coef.size and (coef.min() < 0 or coef.max() > 255)):
        raise ValueError('band_rebuild: four coefficients in 0..255 per source')
    table = np.zeros(len(groups), dtype=REBUILD_GROUP_DTYPE)
    for g, (first, n_rows, n_members, outs) in enumerate(groups):
        if not 1 <= len(outs) <= 4:
            raise ValueError('band_rebuild: group {} has {} outputs, must be 1..4'.format(g, len(outs)))
        table[g]['first_src'], table[g]['n_rows'], table[g]['n_members'], table[g]['t'] = first, n_rows, n_members, len(outs)
        for e, (at, k) in enumerate(outs):
            table[g]['out'][e] = (at, k)
    coef8 = np.zeros(-(-coef.size // 8) * 8, dtype=np.uint8)                     # padded to whole words
    coef8[:coef.size] = coef.reshape(-1)
    a, b = 2 * src.shape[0], 2 * src.shape[0] + 11 * table.shape[0]               # the 8-byte tables in front, each 8-byte aligned
    table_d = upload_small(np.concatenate([src.view(np.int64), table.view(np.int64), coef8.view(np.int64)]))
    call('l3c_band_rebuild', ptr(rows, torch.uint8), rows.numel(), ptr(members, torch.uint8), members.numel(), src.ctypes.data,
         ptr(table_d[:a], torch.int64) if a else None, coef8.ctypes.data, ptr(table_d[b:], torch.int64) if a else None, src.shape[0],
         table.ctypes.data, ptr(table_d[a:b], torch.int64), table.shape[0], stream())
    return members
