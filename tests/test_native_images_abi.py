"""The image-table half of the codec's C ABI (include/l3c_hip.h: l3c_u8_image, l3c_image_padding, l3c_image_table_check, l3c_u8_gather /
l3c_u8_scatter, l3c_encode_images / l3c_decode_images), checked without a GPU: the padding rule is helpers/pad.py's, the size functions are
pure host functions, and every argument error -- a view one byte outside its buffer among them -- is reported before anything is enqueued
(fake, well-aligned pointers stand in for device memory: they are never dereferenced on these paths)."""
import ctypes
import os
import subprocess

import numpy as np

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.helpers import config_parser, pad
from l3c_pytorch_amd.native_codec import IMAGE_DTYPE, image_entry

from tests.conftest import GOLDEN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000
INVALID, UNSUPPORTED = -1, -3
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
NEW = ('l3c_image_padding', 'l3c_image_table_check', 'l3c_u8_gather', 'l3c_u8_scatter', 'l3c_encode_images_workspace_bytes', 'l3c_encode_images',
       'l3c_decode_images_workspace_bytes', 'l3c_decode_images')


def _cfg(name='cr'):
    from l3c_pytorch_amd.native_net import net_config
    return net_config(config_parser.parse_builtin('ms', name))


def _err():
    return _lib.load().l3c_last_error().decode()


def _golden():
    with open(os.path.join(GOLDEN, 'hip_l3c_cal_64x96.l3c'), 'rb') as f:
        return f.read()


def _table(*entries):
    t = np.zeros(len(entries), dtype=IMAGE_DTYPE)
    for k, e in enumerate(entries):
        t[k] = e
    return t


def test_every_entry_point_is_exported_and_the_record_is_the_struct():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    assert lib.l3c_abi_version() == 4                      # symbols were added, nothing existing changed
    assert ctypes.sizeof(_lib.U8Image) == IMAGE_DTYPE.itemsize == 48
    for name, _ in _lib.U8Image._fields_:
        assert getattr(_lib.U8Image, name).offset == IMAGE_DTYPE.fields[name][1], name
        assert getattr(_lib.U8Image, name).size == IMAGE_DTYPE.fields[name][0].itemsize, name


def test_image_padding_is_pad_py():
    lib = _lib.load()
    out = np.zeros(4, dtype=np.uint16)
    for fac in (8, 16):
        for h in range(1, 41):
            for w in range(1, 41):
                assert lib.l3c_image_padding(h, w, fac, out.ctypes.data) == 0
                assert tuple(int(v) for v in out) == pad.padding_for(h, w, fac), (h, w, fac)
    assert lib.l3c_image_padding(767, 511, 8, out.ctypes.data) == 0 and tuple(out) == pad.padding_for(767, 511, 8) == (0, 1, 0, 1)
    for h, w, fac in ((0, 5, 8), (5, 0, 8), (65536, 5, 8), (5, 5, 0), (-3, 5, 8)):
        assert lib.l3c_image_padding(h, w, fac, out.ctypes.data) == INVALID, (h, w, fac)
    assert lib.l3c_image_padding(5, 5, 8, None) == INVALID and 'null pointer' in _err()


def test_size_functions_are_pure_and_grow_with_the_shape():
    lib = _lib.load()
    a, b = _cfg(), _cfg()
    pa, pb = ctypes.byref(a), ctypes.byref(b)
    ws = lib.l3c_encode_images_workspace_bytes
    for K in (0, 1, 4, 64):
        inner = lib.l3c_encode_batch_banded_workspace_bytes(pa, 2, 64, 96, K) if K else lib.l3c_encode_batch_workspace_bytes(pa, 2, 64, 96)
        assert ws(pa, 2, 64, 96, K) == ws(pb, 2, 64, 96, K) >= inner + 2 * 3 * 64 * 96 + 2 * 8 > 0      # the frames and the padding array on top
        assert ws(pa, 3, 64, 96, K) > ws(pa, 2, 64, 96, K) and ws(pa, 2, 128, 96, K) > ws(pa, 2, 64, 96, K)
        assert ws(pa, 2, 64, 192, K) > ws(pa, 2, 64, 96, K)
    for K in (-1, 1025):
        assert ws(pa, 1, 64, 96, K) == INVALID and 'bands' in _err()
    assert ws(pa, 1, 60, 96, 0) < 0 and 'multiples of 2^num_scales' in _err()
    assert ws(pa, 0, 64, 96, 0) < 0 and ws(pa, 65536, 64, 96, 4) < 0
    assert ws(ctypes.byref(_cfg('cr_rgb')), 1, 64, 96, 0) == UNSUPPORTED and 'RGB' in _err()
    # decode: a function of the plan alone, either format
    from tests.test_native_banded_abi import _legacy_blob, _plan_rc, _synthetic
    dw = lib.l3c_decode_images_workspace_bytes
    legacy = _legacy_blob(a, [_golden()])
    assert dw(pa, legacy.ctypes.data) == dw(pb, legacy.ctypes.data) >= lib.l3c_decode_batch_workspace_bytes(pa, legacy.ctypes.data) + 3 * 64 * 96
    assert dw(pa, _legacy_blob(a, [_golden()] * 2).ctypes.data) > dw(pa, legacy.ctypes.data)
    sizes = []
    for H, W in ((64, 96), (136, 200)):
        rc, msg, raw, _, _, _ = _plan_rc(a, [_synthetic(a, H, W, 4, 1)])
        assert rc == 0, msg
        blob = np.frombuffer(raw, dtype=np.int64)
        sizes.append(dw(pa, blob.ctypes.data))
        assert sizes[-1] >= lib.l3c_decode_batch_banded_workspace_bytes(pa, blob.ctypes.data) + 3 * H * W
    assert sizes[1] > sizes[0] > 0
    bad = legacy.copy()
    bad[0] ^= 1
    assert dw(pa, bad.ctypes.data) == INVALID and 'magic' in _err()
    assert dw(pa, None) == INVALID and 'null pointer' in _err()


# ---- the table -------------------------------------------------------------------------------------------------------------------

RGB_8x8 = (0, 24, 1, 3, 8, 8, 0, 0)                   # offset, row_stride, chan_stride, pix_stride, h, w, top, left: 192 bytes


def _bad_tables():
    """(table, Hp, Wp, buffer_bytes, index of the offending image, word of the message) -- the third image is the bad one unless said."""
    good = (0, 24, 1, 3, 4, 4, 0, 0)                  # a 4 x 4 corner of the RGB image: inside every buffer used here

    def third(e, Hp=8, Wp=8, n=192, word=''):
        return _table(good, good, e), Hp, Wp, n, 2, word

    yield third((0, 24, 1, 3, 0, 8, 0, 0), word='h must be')
    yield third((0, 24, 1, 3, 8, 0, 0, 0), word='w must be')
    yield third((0, 24, 1, 3, 65536, 8, 0, 0), Hp=65535, word='h must be')
    yield third((0, 24, 1, 0, 8, 8, 0, 0), word='pix_stride')
    yield third((0, 24, 1, -3, 8, 8, 0, 0), word='pix_stride')
    yield third((0, 24, 1, 3, 8, 8, 1, 0), word='top + h')                 # 1 + 8 > 8
    yield third((0, 24, 1, 3, 8, 8, -1, 0), Hp=16, word='top + h')
    yield third((0, 24, 1, 3, 8, 8, 0, 1), word='left + w')
    yield third((0, 24, 1, 3, 5, 8, 4, 0), word='top + h')                 # 4 + 5 > 8
    # one byte past either end, with positive and negative chan_stride: RGB and BGR views of exactly 192 bytes
    yield third(RGB_8x8, n=191, word='ends behind')
    yield third((1, 24, 1, 3, 8, 8, 0, 0), word='ends behind')
    yield third((-1, 24, 1, 3, 8, 8, 0, 0), word='starts before')
    yield third((2, 24, -1, 3, 8, 8, 0, 0), n=191, word='ends behind')
    yield third((3, 24, -1, 3, 8, 8, 0, 0), word='ends behind')
    yield third((1, 24, -1, 3, 8, 8, 0, 0), word='starts before')
    yield third((0, 8, 64, 1, 8, 8, 0, 0), n=191, word='ends behind')      # planar
    yield third((0, 13, 104, 1, 8, 8, 0, 0), n=3 * 104 - 5 - 1, word='ends behind')     # planar with row pitch 13: the last row has no gap
    yield third((7 * 24, -24, 1, 3, 8, 8, 0, 0), n=191, word='ends behind')             # bottom-up
    yield third((7 * 24 - 1, -24, 1, 3, 8, 8, 0, 0), word='starts before')
    # strides that overflow int64
    yield third((0, I64_MAX, 1, 3, 8, 8, 0, 0), n=I64_MAX, word='overflow')
    yield third((0, I64_MIN, 1, 3, 8, 8, 0, 0), n=I64_MAX, word='overflow')
    yield third((I64_MAX, 24, 1, 3, 8, 8, 0, 0), n=I64_MAX, word='overflow')
    yield third((0, 24, I64_MAX, 3, 8, 8, 0, 0), n=I64_MAX, word='overflow')
    yield third((I64_MIN, 24, -1, 3, 8, 8, 0, 0), n=I64_MAX, word='overflow')
    yield third((I64_MAX - 100, 24, 1, 3, 8, 8, 0, 0), n=I64_MAX, word='overflow')
    yield third((0, I64_MAX // 7, I64_MAX // 2, 3, 8, 8, 0, 0), n=I64_MAX, word='overflow')
    yield _table((0, 24, 1, 3, 8, 9, 0, 0), good), 8, 8, 400, 0, 'left + w'                # the first image is the bad one


def test_table_validator_names_the_image_and_the_field():
    lib = _lib.load()
    chk = lambda t, Hp, Wp, n: lib.l3c_image_table_check(t.ctypes.data, len(t), Hp, Wp, n)   # noqa: E731
    assert chk(_table(RGB_8x8, RGB_8x8, RGB_8x8), 8, 8, 192) == 0
    assert chk(_table((2, 24, -1, 3, 8, 8, 0, 0)), 8, 8, 192) == 0                          # BGR
    assert chk(_table((2, 32, -1, 4, 8, 8, 0, 0)), 8, 8, 255) == 0                          # BGRX: the last X byte is outside every view
    assert chk(_table((0, 13, 104, 1, 8, 8, 4, 8)), 12, 16, 3 * 104 - 5) == 0               # pitch, inside a larger frame
    assert chk(_table((7 * 24, -24, 1, 3, 8, 8, 0, 0)), 8, 8, 192) == 0                     # bottom-up
    assert chk(_table(image_entry('hwc', (511, 767, 3), 0, 0, 0)), 512, 768, 511 * 767 * 3) == 0
    for t, Hp, Wp, n, k, word in _bad_tables():
        assert chk(t, Hp, Wp, n) == INVALID and 'image {}:'.format(k) in _err() and word in _err(), (t[k], _err())
    assert lib.l3c_image_table_check(None, 1, 8, 8, 192) == INVALID and 'null pointer' in _err()
    assert chk(_table(RGB_8x8), 8, 8, 192) == 0
    assert lib.l3c_image_table_check(_table(RGB_8x8).ctypes.data, 0, 8, 8, 192) == INVALID and 'batch size' in _err()


def test_kernel_entry_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    good = _table(RGB_8x8, RGB_8x8, RGB_8x8)

    def gather(src=FAKE, n=192, t=good, dev=FAKE, B=3, Hp=8, Wp=8, dst=FAKE, pads=FAKE):
        return lib.l3c_u8_gather(src, n, None if t is None else t.ctypes.data, dev, B, Hp, Wp, dst, pads, None)

    def scatter(src=FAKE, B=3, Hp=8, Wp=8, dst=FAKE, n=192, t=good, dev=FAKE):
        return lib.l3c_u8_scatter(src, B, Hp, Wp, dst, n, None if t is None else t.ctypes.data, dev, None)

    for fn in (gather, scatter):
        for name in ('src', 'dst', 't', 'dev'):
            assert fn(**{name: None}) == INVALID and 'null pointer' in _err(), (fn.__name__, name)
        for B in (0, -1, 65536):
            assert fn(B=B) == INVALID and 'batch size' in _err(), B
        for Hp, Wp in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
            assert fn(Hp=Hp, Wp=Wp) == INVALID and 'bad frame' in _err()
        assert fn(Wp=10) == INVALID and 'multiple of 4' in _err()
        assert fn(dev=FAKE + 8) == INVALID and '16-byte aligned' in _err()
        assert fn(n=0) == INVALID and 'empty buffer' in _err()
        for t, Hp, Wp, n, k, word in _bad_tables():
            assert fn(t=t, B=len(t), Hp=Hp, Wp=Wp, n=n) == INVALID and 'image {}:'.format(k) in _err() and word in _err(), (fn.__name__, t[k], _err())
        # an odd base pointer of the strided buffer is fine as such: the next check (here the table) answers
        assert fn(**{'src' if fn is gather else 'dst': FAKE + 1, 'n': 191}) == INVALID and 'image 0:' in _err()
    # misaligned frames
    assert gather(dst=FAKE + 4) == INVALID and '16-byte aligned' in _err()
    assert gather(pads=FAKE + 8) == INVALID and '16-byte aligned' in _err()
    assert scatter(src=FAKE + 4) == INVALID and '16-byte aligned' in _err()


def _model(cfg):
    lib = _lib.load()
    return _lib.CodecModel(ctypes.pointer(cfg), FAKE, max(lib.l3c_net_packed_bytes(ctypes.byref(cfg)), 0), FAKE, FAKE, FAKE, -1.0, 0.08)


def _hwc_table(sizes, Hp, Wp):
    entries, off = [], 0
    for h, w in sizes:
        left, _, top, _ = pad.padding_for(h, w, 8)
        entries.append(image_entry('hwc', (h, w, 3), off, top, left))
        off += h * w * 3
    return _table(*entries), off


def _encode_desc(model, table, n, Hp=64, Wp=96, K=0):
    lib = _lib.load()
    cfg = model.cfg_host
    d = _lib.EncodeImagesDesc()
    d.model_host = ctypes.pointer(model)
    d.src, d.src_bytes, d.images_host, d.images = FAKE, n, table.ctypes.data, FAKE
    d.B, d.Hp, d.Wp, d.bands = len(table), Hp, Wp, K
    d.files, d.file_bytes, d.workspace = FAKE, FAKE, FAKE
    d.file_stride = max(lib.l3c_encode_banded_file_stride(cfg, Hp, Wp, K) if K else lib.l3c_encode_file_stride(cfg, Hp, Wp), 0)
    d.workspace_bytes = max(lib.l3c_encode_images_workspace_bytes(cfg, len(table), Hp, Wp, K), 0)
    return d


def test_encode_images_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    enc = lambda d: lib.l3c_encode_images(ctypes.byref(d), None)   # noqa: E731
    cfg = _cfg()
    model = _model(cfg)
    table, n = _hwc_table([(61, 93), (57, 90), (64, 96)], 64, 96)
    desc = lambda **kw: _encode_desc(model, kw.pop('table', table), kw.pop('n', n), **kw)   # noqa: E731
    assert lib.l3c_encode_images(None, None) == INVALID and 'null descriptor' in _err()
    d = desc()
    d.model_host = None
    assert enc(d) == INVALID and 'null pointer' in _err()
    for field in ('src', 'images_host', 'images', 'files', 'file_bytes', 'workspace'):
        d = desc()
        setattr(d, field, None)
        assert enc(d) == INVALID and 'null pointer' in _err(), field
    for field in ('images', 'files', 'file_bytes', 'workspace'):
        d = desc()
        setattr(d, field, FAKE + 4)
        assert enc(d) == INVALID and '16-byte aligned' in _err(), field
    for K in (0, 1, 4):
        d = desc(K=K)
        d.workspace_bytes -= 1
        assert enc(d) == INVALID and 'workspace_bytes too small' in _err()
        d = desc(K=K)
        d.file_stride -= 16
        assert enc(d) == INVALID and 'file_stride' in _err()
        d = desc(K=K)
        d.src_bytes -= 1                                   # the last image's last byte
        assert enc(d) == INVALID and 'image 2:' in _err() and 'ends behind' in _err()
    for K in (-3, 1025):
        d = desc()
        d.bands = K
        assert enc(d) == INVALID and 'bands' in _err()
    d = desc()
    d.B = 0
    assert enc(d) == INVALID and 'batch size' in _err()
    assert enc(desc(Hp=60)) == UNSUPPORTED and 'multiples of 2^num_scales' in _err()
    assert enc(desc(Hp=4096, Wp=2048)) == UNSUPPORTED and 'H * W * Cf * 4' in _err()
    assert enc(_encode_desc(_model(_cfg('cr_rgb')), table, n)) == UNSUPPORTED and 'RGB' in _err()
    # the tables of _bad_tables in an 8 x 8 (or larger) frame of the codec
    for t, Hp, Wp, nb, k, word in _bad_tables():
        if Hp % 8 == 0 and Wp % 8 == 0:
            assert enc(desc(table=t, n=nb, Hp=Hp, Wp=Wp)) == INVALID and 'image {}:'.format(k) in _err() and word in _err(), (t[k], _err())
    # an image that does not fit the frame it is said to sit in
    t2, n2 = _hwc_table([(61, 93), (65, 96)], 64, 96)
    assert enc(desc(table=t2, n=n2)) == INVALID and 'image 1:' in _err() and 'top + h' in _err()


def _decode_desc(model, blob, table, n):
    lib = _lib.load()
    d = _lib.DecodeImagesDesc()
    d.model_host = ctypes.pointer(model)
    d.files, d.plan, d.dst, d.sym, d.workspace = FAKE, FAKE, FAKE, None, FAKE
    d.plan_host, d.plan_bytes = blob.ctypes.data, blob.nbytes
    d.dst_bytes, d.images_host, d.images = n, table.ctypes.data, FAKE
    d.workspace_bytes = max(lib.l3c_decode_images_workspace_bytes(model.cfg_host, blob.ctypes.data), 0)
    return d


def test_decode_images_arguments_are_checked_before_any_launch():
    from tests.test_native_banded_abi import _legacy_blob, _plan_rc, _synthetic
    lib = _lib.load()
    dec = lambda d, side=None: lib.l3c_decode_images(ctypes.byref(d), None, side)   # noqa: E731
    cfg = _cfg()
    model = _model(cfg)
    rc, msg, raw, _, _, _ = _plan_rc(cfg, [_synthetic(cfg, 64, 96, 4, 5)] * 2)
    assert rc == 0, msg
    rc, msg, raw16, _, _, _ = _plan_rc(cfg, [_synthetic(cfg, 64, 96, 64, 6)] * 2)
    assert rc == 0, msg
    table, n = _hwc_table([(61, 93), (64, 96)], 64, 96)
    assert lib.l3c_decode_images(None, None, None) == INVALID and 'null descriptor' in _err()
    for blob in (_legacy_blob(cfg, [_golden()] * 2), np.frombuffer(raw, dtype=np.int64).copy()):
        desc = lambda **kw: _decode_desc(model, kw.get('blob', blob), kw.get('table', table), kw.get('n', n))   # noqa: E731
        d = desc()
        d.model_host = None
        assert dec(d) == INVALID and 'null pointer' in _err()
        for field in ('files', 'plan', 'plan_host', 'dst', 'images_host', 'images', 'workspace'):
            d = desc()
            setattr(d, field, None)
            assert dec(d) == INVALID and 'null pointer' in _err(), field
        for field in ('files', 'plan', 'images', 'sym', 'workspace'):
            d = desc()
            setattr(d, field, FAKE + 4)
            assert dec(d) == INVALID and '16-byte aligned' in _err(), field
        d = desc()
        d.workspace_bytes -= 1
        assert dec(d) == INVALID and 'workspace_bytes too small' in _err()
        d = desc()
        d.plan_bytes = blob.nbytes - 8
        assert dec(d) == INVALID and 'plan_bytes too small' in _err()
        bad = blob.copy()
        bad[0] ^= 1
        assert dec(desc(blob=bad)) == INVALID and 'magic' in _err()
        # the table against the plan's B x H x W, before anything runs: a view one byte past the end, an image of another frame
        assert dec(desc(n=n - 1)) == INVALID and 'image 1:' in _err() and 'ends behind' in _err()
        t2, n2 = _hwc_table([(61, 93), (72, 96)], 72, 96)
        assert dec(desc(table=t2, n=n2)) == INVALID and 'image 1:' in _err() and 'top + h' in _err()
        t3, n3 = _hwc_table([(61, 93), (64, 104)], 64, 104)
        assert dec(desc(table=t3, n=n3)) == INVALID and 'image 1:' in _err() and 'left + w' in _err()
        t4 = table.copy()
        t4['chan_stride'][0] = I64_MAX
        assert dec(desc(table=t4)) == INVALID and 'image 0:' in _err() and 'overflow' in _err()
    # 16 bands per channel decode on two streams: the wrapped entry's own checks still answer before anything is enqueued
    blob16 = np.frombuffer(raw16, dtype=np.int64).copy()
    assert dec(_decode_desc(model, blob16, table, n), None) == INVALID and 'side_stream' in _err()


def test_table_validator_survives_random_and_adversarial_tables_under_the_sanitizers(tmp_path):
    """tests/cabi/image_table_check_main.cpp: csrc/image_table.h alone, built with the address and undefined-behaviour sanitizers and run
    as a child process: 4000 random small views checked against a walk over every byte they address, then int64-edge tables."""
    exe = tmp_path / 'image_table_check'
    subprocess.run(['c++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'image_table_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith('image_table_check: 4000 random tables:'), r.stdout
    assert lines[1].startswith('image_table_check: 432 adversarial tables:') and lines[1].endswith('refused')
