"""The whole-network entry points of the C ABI (include/l3c_hip.h: l3c_net_*), checked without a GPU: the parameter enumeration is
the checkpoint schema, the size functions are pure host functions, and every argument error is reported before anything is enqueued
(fake, well-aligned pointers stand in for device memory: they are never dereferenced on these paths)."""
import ctypes

import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.helpers import config_parser
from l3c_pytorch_amd.modules import schema

FAKE = 0x100000


def _cfg(name):
    from l3c_pytorch_amd.native_net import net_config
    return net_config(config_parser.parse_builtin('ms', name))


def _err():
    return _lib.load().l3c_last_error().decode()


@pytest.mark.parametrize('name', ['cr', 'cr_rgb', 'cr_rgb_shared'])
def test_param_enumeration_is_the_checkpoint_schema(name):
    from l3c_pytorch_amd.native_net import param_schema
    want = list(schema.param_schema(config_parser.parse_builtin('ms', name)).items())
    got = param_schema(_cfg(name))
    assert got == want
    lib = _lib.load()
    cfg = _cfg(name)
    buf, nd, shape = ctypes.create_string_buffer(8), ctypes.c_int(), (ctypes.c_int64 * 4)()
    assert lib.l3c_net_param(ctypes.byref(cfg), 0, buf, 8, ctypes.byref(nd), shape) == -1 and 'name_cap' in _err()
    assert lib.l3c_net_param(ctypes.byref(cfg), len(want), ctypes.create_string_buffer(256), 256, ctypes.byref(nd), shape) == -1
    assert 'out of range' in _err()


def test_size_functions_are_pure_and_grow_with_the_shape():
    lib = _lib.load()
    a, b = _cfg('cr'), _cfg('cr')
    pa, pb = ctypes.byref(a), ctypes.byref(b)
    assert lib.l3c_net_packed_bytes(pa) == lib.l3c_net_packed_bytes(pb) > 0
    assert lib.l3c_net_pack_workspace_bytes(pa) == lib.l3c_net_pack_workspace_bytes(pb) > 0
    fw = lambda c, B, H, W: lib.l3c_net_forward_workspace_bytes(c, B, H, W)   # noqa: E731
    gp = lambda c, B, h, w: lib.l3c_net_get_p_workspace_bytes(c, B, h, w)     # noqa: E731
    assert fw(pa, 2, 64, 96) == fw(pb, 2, 64, 96) > 0
    assert fw(pa, 3, 64, 96) > fw(pa, 2, 64, 96) and fw(pa, 2, 128, 96) > fw(pa, 2, 64, 96) and fw(pa, 2, 64, 192) > fw(pa, 2, 64, 96)
    assert gp(pa, 2, 16, 24) == gp(pb, 2, 16, 24) > 0
    assert gp(pa, 3, 16, 24) > gp(pa, 2, 16, 24) and gp(pa, 2, 32, 24) > gp(pa, 2, 16, 24) and gp(pa, 2, 16, 48) > gp(pa, 2, 16, 24)
    # the baselines' decoders are packed too (l3c_net_get_p covers both families)
    rgb = _cfg('cr_rgb_shared')
    assert 0 < lib.l3c_net_packed_bytes(ctypes.byref(rgb)) < lib.l3c_net_packed_bytes(pa)
    assert gp(ctypes.byref(rgb), 1, 16, 24) > 0
    # unsupported configs: a negative status from the size functions too
    wide = _cfg('cr')
    wide.Cf = 128
    assert lib.l3c_net_packed_bytes(ctypes.byref(wide)) == -3 and 'Cf' in _err()


def _forward_desc(cfg, B=1, H=64, W=96):
    lib = _lib.load()
    d = _lib.NetForwardDesc()
    d.cfg_host = ctypes.pointer(cfg)
    d.packed = FAKE
    d.packed_bytes = max(lib.l3c_net_packed_bytes(ctypes.byref(cfg)), 0)
    d.img, d.B, d.H, d.W = FAKE, B, H, W
    for s in range(cfg.num_scales + 1):
        d.sym[s] = FAKE
        d.bn_q[s] = FAKE if s else None
    for s in range(cfg.num_scales):
        d.P[s] = FAKE
    d.workspace = FAKE
    d.workspace_bytes = max(lib.l3c_net_forward_workspace_bytes(ctypes.byref(cfg), B, H, W), 0)
    return d


def _get_p_desc(cfg, net=0, B=1, h=16, w=24):
    lib = _lib.load()
    d = _lib.NetGetPDesc()
    d.cfg_host = ctypes.pointer(cfg)
    d.packed = FAKE
    d.packed_bytes = max(lib.l3c_net_packed_bytes(ctypes.byref(cfg)), 0)
    d.net, d.bn_q, d.B, d.h, d.w = net, FAKE, B, h, w
    d.fuse, d.P, d.F = None, FAKE, None
    d.workspace = FAKE
    d.workspace_bytes = max(lib.l3c_net_get_p_workspace_bytes(ctypes.byref(cfg), B, h, w), 0)
    return d


def test_forward_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    fwd = lambda d: lib.l3c_net_forward(ctypes.byref(d), None)   # noqa: E731

    # RGB baselines: no forward in the library
    d = _forward_desc(_cfg('cr_rgb'))
    assert fwd(d) == -3 and 'RGB baseline' in _err()
    # Cf != 64
    cfg = _cfg('cr')
    cfg.Cf = 32
    assert fwd(_forward_desc(cfg)) == -3 and 'Cf = 32' in _err()
    # C > 8, Kp > 160
    cfg = _cfg('cr')
    cfg.C = 9
    assert fwd(_forward_desc(cfg)) == -3 and 'C = 9' in _err()
    cfg = _cfg('cr')
    cfg.K = 20
    assert fwd(_forward_desc(cfg)) == -3 and 'Kp' in _err()
    # sides not multiples of 2^num_scales
    cfg = _cfg('cr')
    assert fwd(_forward_desc(cfg, H=60)) == -3 and 'multiples of 2^num_scales' in _err()
    assert fwd(_forward_desc(cfg, W=100)) == -3 and 'multiples of 2^num_scales' in _err()
    # one image above the 32-bit addressing limit (H * W * Cf * 4 >= 0x7ffffff0)
    assert fwd(_forward_desc(cfg, H=4096, W=2048)) == -3 and 'H * W * Cf * 4' in _err()
    # null image, null required outputs
    d = _forward_desc(cfg)
    d.img = None
    assert fwd(d) == -1 and 'null pointer' in _err()
    for field, s in (('sym', 0), ('sym', 3), ('bn_q', 1), ('P', 0), ('P', 2)):
        d = _forward_desc(cfg)
        getattr(d, field)[s] = None
        assert fwd(d) == -1 and 'null pointer' in _err(), (field, s)
    # misaligned pointers
    for field in ('img', 'packed', 'workspace'):
        d = _forward_desc(cfg)
        setattr(d, field, FAKE + 4)
        assert fwd(d) == -1 and '16-byte aligned' in _err(), field
    d = _forward_desc(cfg)
    d.F_dec[1] = FAKE + 8
    assert fwd(d) == -1 and '16-byte aligned' in _err()
    # workspace too small, wrong packed_bytes
    d = _forward_desc(cfg)
    d.workspace_bytes -= 1
    assert fwd(d) == -1 and 'workspace_bytes too small' in _err()
    d = _forward_desc(cfg)
    d.packed_bytes += 256
    assert fwd(d) == -1 and 'packed_bytes' in _err()
    # no descriptor, no config
    assert lib.l3c_net_forward(None, None) == -1 and 'null descriptor' in _err()
    d = _forward_desc(cfg)
    d.cfg_host = None
    assert fwd(d) == -1 and 'null config' in _err()


def test_get_p_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    getp = lambda d: lib.l3c_net_get_p(ctypes.byref(d), None)   # noqa: E731
    cfg = _cfg('cr')
    for net in (-1, 3):
        assert getp(_get_p_desc(cfg, net=net)) == -1 and 'net out of range' in _err()
    rgb = _cfg('cr_rgb_shared')
    assert getp(_get_p_desc(rgb, net=1)) == -1 and 'net out of range' in _err()
    d = _get_p_desc(rgb)
    d.fuse = FAKE
    assert getp(d) == -1 and 'dec_skip == 0' in _err()
    d = _get_p_desc(cfg)
    d.bn_q = None
    assert getp(d) == -1 and 'null pointer' in _err()
    d = _get_p_desc(cfg)
    d.P = None
    assert getp(d) == -1 and 'null pointer' in _err()
    d = _get_p_desc(cfg)
    d.fuse = FAKE + 4
    assert getp(d) == -1 and '16-byte aligned' in _err()
    d = _get_p_desc(cfg)
    d.workspace_bytes -= 16
    assert getp(d) == -1 and 'workspace_bytes too small' in _err()
    d = _get_p_desc(cfg)
    d.packed_bytes = lib.l3c_net_packed_bytes(ctypes.byref(rgb))     # packed for another config
    assert getp(d) == -1 and 'packed_bytes' in _err()
    wide = _cfg('cr')
    wide.Cf = 96
    assert getp(_get_p_desc(wide)) == -3 and 'Cf = 96' in _err()
    assert getp(_get_p_desc(cfg, h=2048, w=1024)) == -3 and 'H * W * Cf * 4' in _err()


def test_pack_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    cfg = _cfg('cr')
    n = lib.l3c_net_param_count(ctypes.byref(cfg))
    nb, wb = lib.l3c_net_packed_bytes(ctypes.byref(cfg)), lib.l3c_net_pack_workspace_bytes(ctypes.byref(cfg))
    params = (ctypes.c_void_p * n)(*([FAKE] * n))
    pack = lambda p, packed, pbytes, ws, wbytes: lib.l3c_net_pack(ctypes.byref(cfg), p, packed, pbytes, ws, wbytes, None)   # noqa: E731
    params[5] = None
    assert pack(params, FAKE, nb, FAKE, wb) == -1 and 'parameter 5 (heads.0.head.1.head.bias)' in _err()
    params[5] = FAKE
    assert pack(params, FAKE, nb - 256, FAKE, wb) == -1 and 'packed_bytes' in _err()
    assert pack(params, FAKE, nb, FAKE, wb - 1) == -1 and 'workspace_bytes too small' in _err()
    assert pack(params, FAKE + 4, nb, FAKE, wb) == -1 and '16-byte aligned' in _err()
    assert pack(None, FAKE, nb, FAKE, wb) == -1 and 'null pointer' in _err()
