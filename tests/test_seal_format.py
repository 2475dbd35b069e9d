"""The seal of a `.l3c` file on the host, no GPU: container.split_seal / make_seal / is_sealed against the C side (csrc/seal.h behind
l3c_seal_find / l3c_seal_write), on the committed golden files of both checkpoints' formats and on a hand-made banded file."""
import ctypes
import glob
import os
import struct
import subprocess
import zlib

import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.bitcoding import container
from tests.conftest import GOLDEN, ROOT

INVALID = -1
SEP = b'\x46\xE2\x84\x92'


def _goldens():
    paths = sorted(glob.glob(os.path.join(GOLDEN, 'hip_*.l3c')))
    assert len(paths) >= 2
    return [open(p, 'rb').read() for p in paths]


def _banded():
    """A small banded file: two records of one channel, one band each."""
    return container.write_file((1, 2, 3, 4), [(1, 8, 8, 64), (1, 16, 16, 256)], [[[b'abc']], [[b'defgh']]], True)


def _bodies():
    return _goldens() + [_banded()]


def _find(data):
    """l3c_seal_find -> (status, body bytes, (generation, frame_crc, model_id)), message."""
    lib = _lib.load()
    body, seal = ctypes.c_int64(-7), _lib.Seal()
    rc = lib.l3c_seal_find(data, len(data), ctypes.byref(body), ctypes.byref(seal))
    return rc, body.value, (seal.generation, seal.frame_crc, seal.model_id), lib.l3c_last_error().decode()


def _write(body, generation, frame_crc, model_id):
    out = ctypes.create_string_buffer(_lib.SEAL_BYTES)
    pad8 = body[6:14] if container.is_banded(body) else body[:8]
    assert _lib.load().l3c_seal_write(ctypes.byref(_lib.Seal(generation, frame_crc, model_id)), pad8, out) == 0
    return out.raw


def test_the_layout_is_the_documented_one():
    body = _banded()
    s = container.make_seal(body, 3, 0xCAFEF00D, 0x1122334455667788)
    assert len(s) == 24 == container.SEAL_BYTES == _lib.SEAL_BYTES
    assert s[:4] == b'L3CS' and s[4] == 1 and s[5] == 0
    assert struct.unpack('<HIQ', s[6:20]) == (3, 0xCAFEF00D, 0x1122334455667788)
    assert struct.unpack('<I', s[20:])[0] == zlib.crc32(struct.pack('<4H', 1, 2, 3, 4) + s[:20])
    legacy = _goldens()[0]
    s = container.make_seal(legacy, 3, 1, 0)
    assert struct.unpack('<I', s[20:])[0] == zlib.crc32(legacy[:8] + s[:20])


def test_python_and_c_write_the_same_bytes_and_read_them_back():
    for body in _bodies():
        for gen_, crc, mid in ((3, 0, 0), (3, 0xFFFFFFFF, 1), (65535, 0x12345678, 0xFEDCBA9876543210)):
            s = container.make_seal(body, gen_, crc, mid)
            assert s == _write(body, gen_, crc, mid)
            sealed = body + s
            assert container.is_sealed(sealed)
            assert container.split_seal(sealed) == (body, container.Seal(gen_, crc, mid))
            assert _find(sealed)[:3] == (1, len(body), (gen_, crc, mid))


def test_unsealed_files_come_back_unchanged():
    for body in _bodies():
        assert body.endswith(SEP)                                    # what the recognition rule leans on
        assert not container.is_sealed(body)
        got, seal = container.split_seal(body)
        assert got is body and seal is None
        assert _find(body)[:2] == (0, len(body))
    for short in (b'', b'L3CS', b'x' * 27, SEP + b'L3CS' + b'\0' * 19):          # below 28 bytes: unsealed whatever they hold
        assert not container.is_sealed(short) and container.split_seal(short) == (short, None) and _find(short)[:2] == (0, len(short))


def test_a_shortened_sealed_file_is_unsealed_and_the_parsers_reject_its_trailing_bytes():
    for body in _bodies():
        sealed = body + container.make_seal(body, 3, 0xA1B2C3D4, 5)
        for cut in range(1, 28):
            f = sealed[:-cut]
            assert not container.is_sealed(f) and container.split_seal(f) == (f, None), cut
            assert _find(f)[:2] == (0, len(f)), cut
            if cut < 24:                                             # seal bytes left behind the last separator
                with pytest.raises(ValueError, match='invalid file'):
                    container.parse_banded(f) if container.is_banded(f) else container.count_scale_records(f)


def _damaged(sealed, at, new):
    return sealed[:at] + bytes([new]) + sealed[at + 1:]


def test_a_damaged_seal_is_invalid_never_unsealed():
    for body in _bodies():
        s = container.make_seal(body, 3, 0xA1B2C3D4, 5)
        sealed = body + s
        pad_at = 6 if container.is_banded(body) else 0

        def rewritten(version, flags):
            head = b'L3CS' + struct.pack('<BB', version, flags) + s[6:20]
            return body + head + struct.pack('<I', zlib.crc32(body[pad_at:pad_at + 8] + head))
        cases = {'unknown version': rewritten(2, 0), 'non-zero flags': rewritten(1, 1),
                 'check word': _damaged(sealed, len(sealed) - 1, sealed[-1] ^ 1),
                 'check word (crc)': _damaged(sealed, len(body) + 9, sealed[len(body) + 9] ^ 0x80),
                 'check word (padding)': _damaged(sealed, pad_at + 3, sealed[pad_at + 3] ^ 2)}
        for what, f in cases.items():
            assert container.is_sealed(f), what
            with pytest.raises(ValueError, match='invalid file: seal') as e:
                container.split_seal(f)
            rc, _, _, msg = _find(f)
            assert rc == INVALID and msg == str(e.value), (what, msg, str(e.value))
            assert what.split(' (')[0] in msg, (what, msg)


def test_seal_errors_say_what_failed_and_where():
    seals = [None, container.Seal(3, 7, 0), container.Seal(2, 7, 9)]
    with pytest.raises(container.SealError) as e:
        container.check_seals(seals, 3, lambda: 9)
    assert (e.value.reason, e.value.index) == ('generation', 2) and isinstance(e.value, ValueError)
    asked = []
    seals[2] = container.Seal(3, 7, 9)
    container.check_seals(seals[:2], 3, lambda: asked.append(1) or 8)       # no seal states a model: the id is never computed
    assert asked == []
    container.check_seals(seals, 3, 9)
    container.check_seals(seals, 3, 0)                                      # this side states none
    with pytest.raises(container.SealError) as e:
        container.check_seals(seals, 3, lambda: 8)
    assert (e.value.reason, e.value.index) == ('model', 2)
    container.check_frame_crcs(seals, [123, 7, -(1 << 32) + 7])             # words as int32 or uint32
    with pytest.raises(container.SealError) as e:
        container.check_frame_crcs(seals, [7, 7, 8])
    assert (e.value.reason, e.value.index) == ('pixels', 2)


def test_model_id_hashes_the_tensors_in_schema_order():
    import hashlib

    import numpy as np
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    from l3c_pytorch_amd.modules import schema
    cfg = config_parser.parse_builtin('ms', 'cr')
    sd = synthetic.make_state_dict(cfg, 0)
    h = hashlib.sha256()
    for key in schema.param_schema(cfg):
        h.update(np.ascontiguousarray(sd[key].numpy(), dtype='<f4').tobytes())
    want = int.from_bytes(h.digest()[:8], 'little')
    assert schema.model_id(sd, cfg) == (want or 1) != schema.model_id(synthetic.make_state_dict(cfg, 1), cfg)


def test_seal_reader_survives_truncations_and_byte_changes_under_the_sanitizers(tmp_path):
    """tests/cabi/seal_check_main.cpp: csrc/seal.h alone, built with the address and undefined-behaviour sanitizers and run as a child
    process: every truncation of a small sealed file, every single-byte change of its last 32 bytes, legacy and banded."""
    exe = tmp_path / 'seal_check'
    subprocess.run(['c++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'seal_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == 'seal_check: 124 truncations unsealed; 16320 single-byte changes: 10200 refused, 4080 unsealed', r.stdout
