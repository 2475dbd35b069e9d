"""The native codec's size functions (include/l3c_hip.h) return exactly what they returned before codec.hip's two formats were folded into
one encode plan and one decode walk: file strides, plan sizes and workspace sizes are part of the contract with callers that allocate once
and reuse, so every entry is an equality.  Needs no GPU: the size functions are pure host functions.

PARENT_ENCODE and PARENT_DECODE hold the values of the library built from commit 7ae48c5 (the parent of the refactor), printed by
`python -m tests.test_native_sizes_host` with L3C_LIB pointing at that build."""
import ctypes

import numpy as np

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.native_codec import parse_plan, parse_plan_banded

from tests.test_native_banded_abi import _cfg, _err, _golden, _legacy_blob, _plan_bytes, _plan_rc, _synthetic

SHAPES = [(1, 8, 8), (1, 64, 96), (3, 64, 96), (16, 64, 96), (1, 512, 768)]


def encode_sizes():
    lib = _lib.load()
    cfg = ctypes.byref(_cfg())
    out = {}
    for B, H, W in SHAPES:
        at = '{}x{}x{}'.format(B, H, W)
        out['file_stride ' + at] = lib.l3c_encode_file_stride(cfg, H, W)
        out['batch_ws ' + at] = lib.l3c_encode_batch_workspace_bytes(cfg, B, H, W)
        for K in (1, 4, 64) + ((1024,) if (H, W) == (512, 768) else ()):
            out['banded_file_stride {} K{}'.format(at, K)] = lib.l3c_encode_banded_file_stride(cfg, H, W, K)
            out['banded_batch_ws {} K{}'.format(at, K)] = lib.l3c_encode_batch_banded_workspace_bytes(cfg, B, H, W, K)
    for K in (0, 4):
        out['images_ws 3x64x96 K{}'.format(K)] = lib.l3c_encode_images_workspace_bytes(cfg, 3, 64, 96, K)
    return out


def decode_sizes():
    lib = _lib.load()
    cfg = _cfg()
    pc = ctypes.byref(cfg)
    out = {}
    for B, lag in ((1, 1), (16, 2)):           # 16 images: the lag-2 path
        files = [_golden()] * B
        blob = _legacy_blob(cfg, files)
        assert parse_plan(blob.tobytes())['lag'] == lag
        at = 'golden B{}'.format(B)
        out['plan_bytes ' + at] = lib.l3c_decode_plan_bytes(pc, B)
        out['batch_ws ' + at] = lib.l3c_decode_batch_workspace_bytes(pc, blob.ctypes.data)
        out['images_ws ' + at] = lib.l3c_decode_images_workspace_bytes(pc, blob.ctypes.data)
    for K, lag in ((4, 1), (16, 2)):           # 16 bands per channel: the banded lag-2 path
        files = [_synthetic(cfg, 64, 96, K, 100 + K)]
        rc, msg, raw, _, _, _ = _plan_rc(cfg, files)
        assert rc == 0, msg
        assert parse_plan_banded(raw)['lag'] == lag
        blob = np.frombuffer(raw, dtype=np.int64).copy()
        at = 'synthetic 64x96 K{}'.format(K)
        out['banded_plan_bytes ' + at] = _plan_bytes(cfg, files)
        out['banded_batch_ws ' + at] = lib.l3c_decode_batch_banded_workspace_bytes(pc, blob.ctypes.data)
        out['images_ws ' + at] = lib.l3c_decode_images_workspace_bytes(pc, blob.ctypes.data)
    return out


# commit 7ae48c5
PARENT_ENCODE = {
    'file_stride 1x8x8': 1152,
    'batch_ws 1x8x8': 103168,
    'banded_file_stride 1x8x8 K1': 1184,
    'banded_batch_ws 1x8x8 K1': 103168,
    'banded_file_stride 1x8x8 K4': 1184,
    'banded_batch_ws 1x8x8 K4': 103168,
    'banded_file_stride 1x8x8 K64': 1184,
    'banded_batch_ws 1x8x8 K64': 103168,
    'file_stride 1x64x96': 57584,
    'batch_ws 1x64x96': 9485312,
    'banded_file_stride 1x64x96 K1': 57600,
    'banded_batch_ws 1x64x96 K1': 9485312,
    'banded_file_stride 1x64x96 K4': 58688,
    'banded_batch_ws 1x64x96 K4': 9487360,
    'banded_file_stride 1x64x96 K64': 65616,
    'banded_batch_ws 1x64x96 K64': 9488896,
    'file_stride 3x64x96': 57584,
    'batch_ws 3x64x96': 28450048,
    'banded_file_stride 3x64x96 K1': 57600,
    'banded_batch_ws 3x64x96 K1': 28450048,
    'banded_file_stride 3x64x96 K4': 58688,
    'banded_batch_ws 3x64x96 K4': 28452096,
    'banded_file_stride 3x64x96 K64': 65616,
    'banded_batch_ws 3x64x96 K64': 28458240,
    'file_stride 16x64x96': 57584,
    'batch_ws 16x64x96': 151721216,
    'banded_file_stride 16x64x96 K1': 57600,
    'banded_batch_ws 16x64x96 K1': 151721216,
    'banded_file_stride 16x64x96 K4': 58688,
    'banded_batch_ws 16x64x96 K4': 151727360,
    'banded_file_stride 16x64x96 K64': 65616,
    'banded_batch_ws 16x64x96 K64': 151759104,
    'file_stride 1x512x768': 3650096,
    'batch_ws 1x512x768': 606870272,
    'banded_file_stride 1x512x768 K1': 3650112,
    'banded_batch_ws 1x512x768 K1': 606870272,
    'banded_file_stride 1x512x768 K4': 3651632,
    'banded_batch_ws 1x512x768 K4': 606872320,
    'banded_file_stride 1x512x768 K64': 3679632,
    'banded_batch_ws 1x512x768 K64': 606878976,
    'banded_file_stride 1x512x768 K1024': 3910352,
    'banded_batch_ws 1x512x768 K1024': 606945024,
    'images_ws 3x64x96 K0': 28505856,
    'images_ws 3x64x96 K4': 28507904,
}

# commit 7ae48c5
PARENT_DECODE = {
    'plan_bytes golden B1': 1360,
    'batch_ws golden B1': 13023744,
    'images_ws golden B1': 13042432,
    'plan_bytes golden B16': 6752,
    'batch_ws golden B16': 359919616,
    'images_ws golden B16': 360214784,
    'banded_plan_bytes synthetic 64x96 K4': 1984,
    'banded_batch_ws synthetic 64x96 K4': 8263424,
    'images_ws synthetic 64x96 K4': 8282112,
    'banded_plan_bytes synthetic 64x96 K16': 4240,
    'banded_batch_ws synthetic 64x96 K16': 8262400,
    'images_ws synthetic 64x96 K16': 8281088,
}


def _assert_equal(got, want):
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert want[key] > 0 and got[key] == want[key], (key, got[key], want[key], _err())


def test_encode_strides_and_workspaces_equal_the_parent_commits():
    _assert_equal(encode_sizes(), PARENT_ENCODE)


def test_decode_plan_and_workspace_sizes_equal_the_parent_commits():
    _assert_equal(decode_sizes(), PARENT_DECODE)


if __name__ == '__main__':
    for name, table in (('PARENT_ENCODE', encode_sizes()), ('PARENT_DECODE', decode_sizes())):
        print('{} = {{'.format(name))
        for key, value in table.items():
            print('    {!r}: {},'.format(key, value))
        print('}\n')
