"""The network as two library calls (include/l3c_hip.h: l3c_net_forward / l3c_net_get_p).

`NativeNet(multiscale_network)` packs the module's weights once into ONE device buffer (l3c_net_pack) and then runs
MultiscaleNetwork.forward / .get_P as one call each: the library drives the same kernels with the same descriptors in the same order as
the Python schedule of modules/multiscale_network.py, so the outputs are bit-identical to it.  Outputs and workspaces are torch tensors
allocated on the current stream; nothing synchronises the host.

The product paths (MultiscaleNetwork, Bitcoding, l3c.py, test.py) still run the Python schedule; `Bitcoding.encode_batch(imgs,
out=NativeNet(net).forward(imgs))` works because the returned `Out` has the same fields.
"""
import ctypes

import torch

from . import _lib
from ._lib import NetConfig, NetForwardDesc, NetGetPDesc, call, ptr, stream
from .modules.multiscale_network import Out
from .modules.net import EncOut


def net_config(config_ms):
    """l3c_net_config of a parsed config (configs/ms/*.cf)."""
    return NetConfig(num_scales=config_ms.num_scales, Cf=config_ms.Cf, C=config_ms.q.C, L=config_ms.q.L, K=config_ms.prob.K,
                     enc_blocks=config_ms.enc.num_blocks, dec_blocks=config_ms.dec.num_blocks,
                     rgb_baseline=int(bool(config_ms.rgb_bicubic_baseline)), dec_skip=int(bool(config_ms.dec.skip)))


def param_schema(cfg):
    """[(name, shape)] in l3c_net_param order."""
    lib = _lib.load()
    n = lib.l3c_net_param_count(ctypes.byref(cfg))
    _lib.check(min(n, 0))
    name, ndim, shape = ctypes.create_string_buffer(256), ctypes.c_int(), (ctypes.c_int64 * 4)()
    out = []
    for i in range(n):
        call('l3c_net_param', ctypes.byref(cfg), i, name, 256, ctypes.byref(ndim), shape)
        out.append((name.value.decode(), tuple(shape[k] for k in range(ndim.value))))
    return out


def _size(rc):
    _lib.check(min(rc, 0))
    return rc


def _bytes(n):
    return torch.empty(max(n, 16), dtype=torch.uint8, device='cuda')


class NativeNet(object):
    def __init__(self, network):
        _lib.require_gpu()
        lib = _lib.load()
        self.config_ms = network.config_ms
        self.cfg = net_config(self.config_ms)
        self._cfg_ref = ctypes.byref(self.cfg)
        self.scales = self.config_ms.num_scales
        self._rgb = bool(self.config_ms.rgb_bicubic_baseline)
        sd = network.state_dict()
        names = param_schema(self.cfg)
        params = []
        for name, shape in names:
            t = sd[name].detach()
            if tuple(t.shape) != shape:
                raise _lib.L3CError('{}: shape {} != {}'.format(name, tuple(t.shape), shape))
            params.append(t.to('cuda', torch.float32).contiguous())
        self.packed_bytes = _size(lib.l3c_net_packed_bytes(self._cfg_ref))
        self.packed = _bytes(self.packed_bytes)
        ws_bytes = _size(lib.l3c_net_pack_workspace_bytes(self._cfg_ref))
        ws = _bytes(ws_bytes)
        arr = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
        call('l3c_net_pack', self._cfg_ref, arr, ptr(self.packed), self.packed_bytes, ptr(ws), ws_bytes, stream())
        # (params / ws go back to the caching allocator: reused only by later work on this stream, after the pack)

    def kp(self, s):
        Cp = 3 if (self._rgb or s == 0) else self.config_ms.q.C
        return (4 if Cp == 3 else 3) * Cp * self.config_ms.prob.K

    def forward_workspace_bytes(self, B, H, W):
        return _size(_lib.load().l3c_net_forward_workspace_bytes(self._cfg_ref, B, H, W))

    def get_P_workspace_bytes(self, B, h, w):
        return _size(_lib.load().l3c_net_get_p_workspace_bytes(self._cfg_ref, B, h, w))

    def forward(self, x, features=True, workspace=None):
        """x: image NCHW in [0, 255] -> Out with the fields of MultiscaleNetwork.forward.  features=False: raw.F_enc / raw.F_dec
        and EncOut.F are None (less memory).  workspace: a uint8 device tensor of at least forward_workspace_bytes (tests)."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('Expected BCHW image, got {}'.format(tuple(x.shape)))
        x = x.to('cuda', torch.float32).contiguous()
        B, _, H, W = x.shape
        S, C, Cf = self.scales, self.config_ms.q.C, self.config_ms.Cf
        dev = x.device
        sym = [torch.empty(B, 3, H, W, dtype=torch.int16, device=dev)]
        bn_q = [None]
        P, F_enc, F_dec = [], [], []
        for s in range(S):
            h, w = H >> (s + 1), W >> (s + 1)
            sym.append(torch.empty(B, C, h, w, dtype=torch.int16, device=dev))
            bn_q.append(torch.empty(B, C, h, w, dtype=torch.float32, device=dev))
            P.append(torch.empty(B, H >> s, W >> s, self.kp(s), dtype=torch.float32, device=dev))
            F_enc.append(torch.empty(B, h, w, Cf, dtype=torch.float32, device=dev) if features else None)
            F_dec.append(torch.empty(B, H >> s, W >> s, Cf, dtype=torch.float32, device=dev) if features else None)
        ws_bytes = self.forward_workspace_bytes(B, H, W)
        ws = _bytes(ws_bytes) if workspace is None else workspace
        d = NetForwardDesc()
        d.cfg_host, d.packed, d.packed_bytes = ctypes.pointer(self.cfg), ptr(self.packed), self.packed_bytes
        d.img, d.B, d.H, d.W = ptr(x), B, H, W
        for s in range(S + 1):
            d.sym[s] = ptr(sym[s])
            d.bn_q[s] = ptr(bn_q[s])
        for s in range(S):
            d.P[s], d.F_enc[s], d.F_dec[s] = ptr(P[s]), ptr(F_enc[s]), ptr(F_dec[s])
        d.workspace, d.workspace_bytes = ptr(ws), ws.numel()
        call('l3c_net_forward', ctypes.byref(d), stream())

        out = Out(targets_style='bn', auto_recursive_from=None)
        out.S.append(sym[0].long())
        out.L.append(256)
        out.bn.append(None)
        raw = out.raw
        raw.sym.append(sym[0])
        raw.bn_q.append(None)
        for s in range(S):
            raw.sym.append(sym[s + 1])
            raw.bn_q.append(bn_q[s + 1])
            raw.P.append(P[s])
            raw.F_enc.append(F_enc[s])
            raw.F_dec.append(F_dec[s])
            F = F_enc[s].permute(0, 3, 1, 2) if features else None
            out.append(EncOut(bn_q[s + 1], bn_q[s + 1], sym[s + 1].long(), self.config_ms.q.L, F), P[s].permute(0, 3, 1, 2))
        return out

    def __call__(self, x, auto_recurse=0):
        if auto_recurse:
            raise NotImplementedError('auto_recurse is only used by the RGB Shared baseline')
        return self.forward(x)

    def get_P(self, scale, bn_q, dec_F_prev=None, n_scales_total=None, workspace=None):
        """MultiscaleNetwork.get_P: (P, F) of `scale` as logical NCHW views, from the quantised bottleneck of scale + 1 and the coarser
        decoder's features.  n_scales_total (RGB baselines with auto_recurse): scales >= num_scales are the recursive applications of
        the last network, which take no fused features."""
        n_total = self.scales if n_scales_total is None else n_scales_total
        assert 0 <= scale < n_total, 'Out of range: {}'.format(scale)
        assert n_total == self.scales or self._rgb, 'recursion is only defined for the RGB baselines'
        net = min(scale, self.scales - 1)
        if self._rgb:      # the rule of MultiscaleNetwork.get_P: no fusion for recursive scales, nor for the coarsest proper one
            forward_scales = list(range(self.scales)) + [-1] * (n_total - self.scales)
            s = forward_scales[scale]
            if not self.config_ms.dec.skip or s == -1 or s == max(forward_scales):
                dec_F_prev = None
        bn_q = bn_q.to('cuda', torch.float32).contiguous()
        B, C, h, w = bn_q.shape
        Cf = self.config_ms.Cf
        fuse = dec_F_prev.permute(0, 2, 3, 1).contiguous() if dec_F_prev is not None else None
        P = torch.empty(B, 2 * h, 2 * w, self.kp(net), dtype=torch.float32, device=bn_q.device)
        F = torch.empty(B, 2 * h, 2 * w, Cf, dtype=torch.float32, device=bn_q.device)
        ws = _bytes(self.get_P_workspace_bytes(B, h, w)) if workspace is None else workspace
        d = NetGetPDesc()
        d.cfg_host, d.packed, d.packed_bytes, d.net = ctypes.pointer(self.cfg), ptr(self.packed), self.packed_bytes, net
        d.bn_q, d.B, d.h, d.w = ptr(bn_q), B, h, w
        d.fuse, d.P, d.F = ptr(fuse), ptr(P), ptr(F)
        d.workspace, d.workspace_bytes = ptr(ws), ws.numel()
        call('l3c_net_get_p', ctypes.byref(d), stream())
        return P.permute(0, 3, 1, 2), F.permute(0, 3, 1, 2)
