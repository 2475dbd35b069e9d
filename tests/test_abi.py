"""The C-ABI library loads and exports every symbol include/l3c_hip.h declares (no compute without a GPU)."""
import os
import re

import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header='l3c_hip.h'):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(l3c_[a-z0-9_]+)\s*\(', src)))


def test_library_is_built_and_exports_every_declared_symbol():
    import __graft_entry__
    __graft_entry__.build()
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(_lib.PROTOTYPES) == names
    assert lib.l3c_abi_version() == _lib.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, 'include', 'l3c_hip.h')).read()
    assert lib.l3c_bitstream_generation() == int(re.search(r'#define L3C_BITSTREAM_GENERATION (\d+)', hdr).group(1)) >= 3
    # the product library holds ONE generation of convolution kernels: the F(2x2,3x3) cross-check kernel lives in the test-only
    # library (include/l3c_xcheck.h), which exports exactly what that header declares
    assert not any(n.startswith('l3c_conv_wino_') or n == 'l3c_conv_wino' for n in names)
    assert not hasattr(lib, 'l3c_conv_wino')
    x = _lib.load_xcheck()
    xnames = _declared('l3c_xcheck.h')
    assert sorted(_lib.XCHECK_PROTOTYPES) == xnames and len(xnames) == 8
    for n in xnames:
        assert hasattr(x, n), n


def test_pure_host_entry_points():
    lib = _lib.load()
    assert lib.l3c_interval_words(3, 100) == 2 * 3 * 64 * 2      # two role words per symbol
    assert lib.l3c_interval_words(48, 393216) == 393216 * 48 * 2
    assert lib.l3c_ac_max_bytes(393216) >= 2 * 393216 + 8 and lib.l3c_ac_max_bytes(393216) % 4 == 0
    assert lib.l3c_conv_packed_words(64, 64, 3) == 64 * 64 * 9
    assert lib.l3c_conv_packed_words(120, 192, 1) == 128 * 192


def test_argument_errors_are_reported_not_crashed():
    lib = _lib.load()
    rc = lib.l3c_ac_encode(None, 1, 1, None, 0, None, None, None)
    assert rc == -1 and b'null pointer' in lib.l3c_last_error()
    with pytest.raises(_lib.L3CError):
        _lib.check(rc)


def test_argument_validation_of_every_family_precedes_any_launch():
    """Status codes + messages instead of crashes, checked WITHOUT a GPU: validation happens before any HIP call.  Fake but
    well-aligned non-null pointers stand in for device memory (they are never dereferenced on these paths)."""
    import ctypes
    lib = _lib.load()
    xlib = _lib.load_xcheck()
    fake = 0x1000

    def err():
        return lib.l3c_last_error().decode()

    def xerr():
        return xlib.l3c_last_error().decode()

    # range coder
    assert lib.l3c_ac_decode(fake, 300, 300, fake, fake, fake, 1, 1, 1, fake, None) == -1 and 'Lp out of range' in err()
    assert lib.l3c_ac_decode(fake, 7, 26, fake, fake, fake, 1, 1, 1, fake, None) == -1 and 'row_stride' in err()
    assert lib.l3c_ac_decode(fake, 26, 26, fake + 2, fake, fake, 1, 1, 1, fake, None) == -1 and '4-byte aligned' in err()
    assert lib.l3c_ac_encode(fake, 0, 5, fake, 64, fake, fake, None) == -1
    assert lib.l3c_ac_encode_groups(None, 1, fake, None) == -1 and 'bad arguments' in err()
    grp = (_lib.AcGroup * 1)(_lib.AcGroup(fake, fake, fake, 4, 100, 8))        # stride smaller than l3c_ac_max_bytes(100)
    assert lib.l3c_ac_encode_groups(grp, 1, fake, None) == -1 and 'stride too small' in err()
    part = _lib.AcDecodePart(fake, 26, fake, fake, fake, 2, 10, None, fake, fake, 0, fake, 10, 0)
    assert lib.l3c_ac_decode_chunks((_lib.AcDecodePart * 1)(part), 1, None) == -1 and 'must differ' in err()
    assert lib.l3c_ac_decode_chunks((_lib.AcDecodePart * 1)(part), 9, None) == -1 and 'parts per call' in err()
    # window rows (ABI 3): only for the 256-symbol alphabet, and only with everything a missed row needs
    assert lib.l3c_dmll_cdf_table(fake, fake, fake, 1, 10, 5, 10, 0, 1, 0, 10, 26, fake, None, fake, None) == -1 and 'window rows' in err()
    wpart = _lib.AcDecodePart(fake, 257, fake, fake, fake, 2, 10, fake, None, fake, 1, fake, 10, 0)
    wpart.window_stats_in, wpart.window_stats_out = fake, fake
    wpart.C, wpart.K, wpart.c, wpart.HW, wpart.pix0 = 3, 10, 0, 100, 0
    assert lib.l3c_ac_decode_chunks((_lib.AcDecodePart * 1)(wpart), 1, None) == -1 and 'window rows' in err()      # P / targets missing
    assert lib.l3c_ac_decode_state_bytes() == 32
    # mixture head
    assert lib.l3c_dmll_nll(fake, fake, 1, 10, 3, 17, 1, 0.0, 255.0, 256, fake, None) == -1 and 'K out of range' in err()
    assert lib.l3c_dmll_nll(fake, fake, 1, 10, 5, 10, 1, 0.0, 255.0, 256, fake, None) == -1 and 'C == 3' in err()
    assert lib.l3c_dmll_cdf_table(fake, None, fake, 1, 10, 3, 10, 1, 1, 0, 10, 257, fake, None, None, None) == -1 and 'decoded so far' in err()
    assert lib.l3c_dmll_cdf_table(fake, fake, fake, 1, 10, 3, 10, 1, 1, 5, 10, 257, fake, None, None, None) == -1 and 'outside the image' in err()
    assert lib.l3c_dmll_sample(fake, fake, None, 1, 10, 3, 10, 1, fake, None) == -1 and 'null pointer' in err()
    # convolution
    assert lib.l3c_conv_pack_weights(fake, 64, 60, 3, fake, None) == -1 and 'multiple of 8' in err()
    assert lib.l3c_conv_pack_weights(fake, 64, 64, 7, fake, None) == -1 and 'KS must be' in err()
    d = _lib.ConvDesc()
    d.inp = d.packed_w = d.bias = d.out = fake
    d.B, d.Hin, d.Win, d.Cin, d.Cout, d.KS, d.stride, d.dilation = 1, 8, 8, 64, 64, 5, 1, 1
    d.in_cstride = 64
    assert xlib.l3c_conv_wino(ctypes.byref(d), None) == -1 and '3x3, stride 1 only' in xerr()
    d.KS, d.dilation = 3, 3
    assert xlib.l3c_conv_wino(ctypes.byref(d), None) == -1 and 'dilation must be' in xerr()
    d.dilation, d.Cin = 1, 60
    assert xlib.l3c_conv_wino(ctypes.byref(d), None) == -1 and 'multiple of 16' in xerr()
    d.Cin, d.out_cstride = 64, 62
    assert xlib.l3c_conv_wino(ctypes.byref(d), None) == -1 and '16-byte stores' in xerr()
    d.out_cstride, d.out = 64, fake + 4
    assert xlib.l3c_conv_wino(ctypes.byref(d), None) == -1 and '16-byte aligned' in xerr()
    d.out, d.Cout = fake, 62
    assert xlib.l3c_conv_wino(ctypes.byref(d), None) == -1 and 'multiple of 4' in xerr()
    d.Cout, d.epilogue = 64, 0x100
    assert xlib.l3c_conv_wino(ctypes.byref(d), None) == -1 and 'unknown epilogue bits' in xerr()
    assert lib.l3c_conv_mfma(ctypes.byref(d), None) == -1 and 'unknown epilogue bits' in err()      # no probe kernels in the product
    d.epilogue = 0
    assert xlib.l3c_conv_wino_set_tiles_per_block(2) == 0 and xlib.l3c_conv_wino_set_tiles_per_block(0) == 2
    assert xlib.l3c_conv_wino_packed_words(64, 64) == 16 * 64 * 64 and xlib.l3c_conv_wino_packed_words(120, 64) == 16 * 128 * 64
    # container
    sc = (_lib.ContainerScale * 1)(_lib.ContainerScale(fake, fake, 6, 5, 8, 8))
    assert lib.l3c_container_write(sc, 1, 2, fake, fake, fake, None) == -1 and '4-byte aligned' in err()
    sc = (_lib.ContainerScale * 1)(_lib.ContainerScale(fake, fake, 8, 5, 70000, 8))
    assert lib.l3c_container_write(sc, 1, 2, fake, fake, fake, None) == -1 and 'u16' in err()
    assert lib.l3c_container_write(sc, 9, 2, fake, fake, fake, None) == -1 and 'scales' in err()
    del ctypes


def test_conv_entries_refuse_bad_channel_slices():
    """The channel-slice preconditions of every conv entry (input / residual / output read or written as channels coff .. coff + C of a
    tensor with cstride channels per pixel), as refusals with their messages, WITHOUT a GPU.  Every descriptor handed in here must be
    refused: its pointers are fake.  As a second line of defence its shape (2^45 pixels) is one every entry refuses further down --
    'grid too large' / 'below 2 GB' -- should a slice check ever go missing: the assertion on the message then fails, and nothing is
    launched.  (l3c_conv_mfma checks the input slice only and l3c_conv_wino4w the input's multiples of 4 only: nothing else to assert
    there today.)"""
    import ctypes
    lib = _lib.load()
    xlib = _lib.load_xcheck()
    fake = 0x1000
    RES = _lib.EPI_RESIDUAL

    def desc(KS=3, stride=1, epilogue=RES, **over):
        d = _lib.ConvDesc()
        d.inp = d.packed_w = d.bias = d.out = d.residual = fake
        d.B = d.Hin = d.Win = 32768
        d.Cin, d.Cout, d.KS, d.stride, d.dilation, d.epilogue = 64, 64, KS, stride, 1, epilogue
        d.in_cstride, d.in_coff = 76, 8              # the layouts of tests/test_gpu_conv_slices.py
        d.res_cstride, d.res_coff = 84, 12
        d.out_cstride, d.out_coff = 72, 4
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def refused(fn, d, message, *extra, **kw):
        err = (xlib if kw.get('x') else lib).l3c_last_error
        rc = fn(ctypes.byref(d), *(extra + (None,)))
        assert rc == -1 and message in err().decode(), (fn.__name__, rc, err().decode(), message)

    IN4, OUT4, RES4 = 'input channel stride/offset must be multiples of 4', 'output channel stride/offset must be multiples of 4', \
        'residual channel stride/offset must be multiples of 4'
    IN_R, OUT_R, RES_R = 'input channel slice out of range', 'output channel slice out of range', 'residual channel slice out of range'
    # the three entries of the F(4x4,3x3) kernel and the F(2x2,3x3) kernel of the cross-check library: 16-byte loads and stores
    # (safety net behind the slice checks: 'grid too large', then 'one image of the input must stay below 2 GB' -- conv_wino4_launch in
    # csrc/conv_wino4.hip, l3c_conv_wino in csrc/conv_wino.hip)
    wino = [(lib.l3c_conv_wino4, dict(), (), False), (lib.l3c_conv_wino4_phase, dict(stride=2), (1, 0), False),
            (lib.l3c_conv_wino4_stride2, dict(KS=5, stride=2, epilogue=0), (), False), (xlib.l3c_conv_wino, dict(), (), True)]
    for fn, base, extra, x in wino:
        refused(fn, desc(in_coff=16, **base), IN_R, *extra, x=x)                    # 16 + 64 > 76
        refused(fn, desc(in_cstride=68, **base), IN_R, *extra, x=x)
        refused(fn, desc(in_cstride=78, **base), IN4, *extra, x=x)
        refused(fn, desc(in_coff=6, **base), IN4, *extra, x=x)
        refused(fn, desc(out_coff=3, **base), OUT4, *extra, x=x)
        refused(fn, desc(out_cstride=70, **base), OUT4, *extra, x=x)
        refused(fn, desc(out_coff=12, **base), OUT_R, *extra, x=x)                  # 12 + 64 > 72
        refused(fn, desc(out_cstride=60, out_coff=0, **base), OUT_R, *extra, x=x)
        if base.get('epilogue', RES) & RES:
            refused(fn, desc(res_coff=5, **base), RES4, *extra, x=x)
            refused(fn, desc(res_cstride=82, **base), RES4, *extra, x=x)
            refused(fn, desc(res_coff=24, **base), RES_R, *extra, x=x)              # 24 + 64 > 84
            refused(fn, desc(res_cstride=72, **base), RES_R, *extra, x=x)
    # pixel shuffle: the slice holds Cout / 4 channels
    refused(lib.l3c_conv_wino4, desc(Cout=256, epilogue=_lib.EPI_PIXEL_SHUFFLE, out_cstride=64, out_coff=4), OUT_R)
    refused(xlib.l3c_conv_wino, desc(Cout=256, epilogue=_lib.EPI_PIXEL_SHUFFLE, out_cstride=64, out_coff=4), OUT_R, x=True)
    # pointwise kernel: 16-byte loads, 4-byte stores (any output offset)
    # (safety net: 'grid too large' in l3c_conv_pw, csrc/conv_pw.hip -- 2^45 pixels are 2^38 tiles)
    pw = dict(KS=1, epilogue=0, Cin=192, Cout=120, in_cstride=204, out_cstride=125, out_coff=3)
    refused(lib.l3c_conv_pw, desc(**dict(pw, in_coff=16)), 'channel slice out of range')
    refused(lib.l3c_conv_pw, desc(**dict(pw, out_coff=6)), 'channel slice out of range')
    refused(lib.l3c_conv_pw, desc(**dict(pw, in_coff=6)), IN4)
    refused(lib.l3c_conv_pw, desc(**dict(pw, in_cstride=206)), IN4)
    # implicit GEMM: 16-byte loads of the input
    # (safety net: 'grid too large' in launch / launch_lds, csrc/conv_mfma.hip, ahead of every HIP call)
    for base in (dict(), dict(KS=5, stride=2, epilogue=0), dict(KS=1, epilogue=0)):
        refused(lib.l3c_conv_mfma, desc(in_coff=16, **base), IN_R)
        refused(lib.l3c_conv_mfma, desc(in_cstride=68, **base), IN_R)
        refused(lib.l3c_conv_mfma, desc(in_coff=6, **base), IN4)
        refused(lib.l3c_conv_mfma, desc(in_cstride=78, **base), IN4)
    # the 32x32x2 probe kernel of the cross-check library
    # (safety net: 'one image of the input must stay below 2 GB' in l3c_conv_wino4w, csrc/conv_wino4w.hip, right behind this check)
    refused(xlib.l3c_conv_wino4w, desc(epilogue=0, in_coff=6), IN4, 0, x=True)
    refused(xlib.l3c_conv_wino4w, desc(epilogue=0, in_cstride=78), IN4, 0, x=True)


def test_no_cpu_fallback():
    import torch
    with pytest.raises(_lib.L3CError):
        _lib.ptr(torch.zeros(4))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.L3CError):
            _lib.require_gpu()


def test_ring_decoder_prefetch_registers_untouched():
    """The ring decoder's LDS row prefetch is inline asm the compiler cannot see into; tools/check_asm_prefetch.py rebuilds
    the CFG of the compiled kernels and proves no compiler-generated instruction names a register with a read in flight."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'check_asm_prefetch.py')], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_no_store_data_hazard_in_isa():
    """gfx950: a VALU write right behind a 16-byte buffer store with a register soffset corrupts the stored data and hipcc
    inserts no wait state there (found with conv_wino.hip); tools/check_store_hazard.py scans every kernel's ISA."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'check_store_hazard.py')], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_mfma_kernels_stay_inside_their_register_budget():
    """conv_wino4_kernel holds 144 accumulators per lane at two blocks per CU: every variant the network launches must fit 256 VGPRs
    without scratch spills (the allocator once spilled 7 registers of the residual variant's epilogue); tools/check_registers.py reads the
    code-object metadata of the ISA compiled with the product flags."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'check_registers.py')], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
