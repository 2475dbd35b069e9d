"""The host half of l3c_u8_crc32_spans (include/l3c_hip.h; csrc/crc_spans.h, csrc/crc.hip), checked without a GPU: the span table's
validator and the combine arithmetic in a stand-alone program under the address and undefined-behaviour sanitizers, and every argument
error of the entry point on the loaded library -- reported before anything is launched (fake, well-aligned pointers stand in for device
memory: they are never dereferenced on these paths)."""
import ctypes
import os
import subprocess

import numpy as np

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000
INVALID = -1
I64_MAX = (1 << 63) - 1
TILE = 32 * 4096                 # block_bytes of l3c_u8_crc32_tile


def _err():
    return _lib.load().l3c_last_error().decode()


def _table(*spans):
    t = np.zeros(len(spans), dtype=ops.SPAN_DTYPE)
    for k, s in enumerate(spans):
        t[k] = s
    return t


def test_span_table_and_combine_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cabi/span_table_check_main.cpp: csrc/crc_spans.h alone, built with the address and undefined-behaviour sanitizers and run as a
    child process."""
    exe = tmp_path / 'span_table_check'
    subprocess.run(['c++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'span_table_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith('span_table_check: 15 tables refused, 300 random tables'), r.stdout
    assert lines[1].startswith('span_table_check: 70 runs replayed') and lines[1].endswith('equal to the bitwise CRC-32')


def test_the_symbols_are_exported_and_the_record_is_the_struct():
    lib = _lib.load()
    for name in ('l3c_u8_crc32_spans', 'l3c_u8_crc32_spans_workspace_bytes'):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    assert lib.l3c_abi_version() == 4                      # symbols were added, nothing existing changed
    assert ctypes.sizeof(_lib.U8Span) == ops.SPAN_DTYPE.itemsize == 16
    for name, _ in _lib.U8Span._fields_:
        assert getattr(_lib.U8Span, name).offset == ops.SPAN_DTYPE.fields[name][1], name


def test_workspace_bytes_grow_with_spans_and_tiles():
    ws = _lib.load().l3c_u8_crc32_spans_workspace_bytes

    def size(*spans):
        t = _table(*spans)
        return ws(t.ctypes.data, t.shape[0])

    one = size((0, 1))
    assert one > 0 and one % 16 == 0
    assert size((0, 0)) > 0                                 # a call of empty spans still needs the prefix and the constants
    assert size((0, 1), (0, 1)) >= one + 8 + 16 + 4 - 16    # a prefix entry, a span's constants and a tile's word more (before rounding)
    assert size((0, TILE)) == one and size((0, 5 * TILE + 1)) >= one + 4 * 5 - 16
    assert size((I64_MAX - 3, 100)) == one                  # offsets are not its business
    assert size((0, 8 * TILE), (4, 1)) == size((4, 1), (0, 8 * TILE))
    assert ws(None, 1) == INVALID and 'null table' in _err()
    assert size() == INVALID and 'n_spans' in _err()
    assert size((0, 4), (0, -1)) == INVALID and 'span 1' in _err() and 'bytes must not be negative' in _err()
    assert size((0, 4), (0, 4), (0, I64_MAX)) == INVALID and 'span 2' in _err() and '2^40 tiles' in _err()


def check_rejected_arguments():
    """Every argument l3c_u8_crc32_spans must refuse -> -1 and a message that names the span or the field."""
    lib = _lib.load()
    good = _table((0, 100), (100, 28), (64, 0))

    def run(table=good, n=None, data=FAKE, data_bytes=128, spans=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 20, host=True):
        n = table.shape[0] if n is None else n
        return lib.l3c_u8_crc32_spans(data, data_bytes, table.ctypes.data if host else None, spans, n, out, ws, ws_bytes, None)

    for kw in ({'data': None}, {'host': False}, {'spans': None}, {'out': None}, {'ws': None}):
        assert run(**kw) == INVALID and 'null pointer' in _err(), kw
    assert run(n=0) == INVALID and 'n_spans' in _err()
    assert run(n=-1) == INVALID and 'n_spans' in _err()
    assert run(data_bytes=-1) == INVALID and 'data_bytes' in _err()
    assert run(_table((0, 4), (-4, 4))) == INVALID and 'span 1' in _err() and 'offset must not be negative' in _err()
    assert run(_table((0, 4), (0, 4), (0, -1))) == INVALID and 'span 2' in _err() and 'bytes must not be negative' in _err()
    assert run(_table((0, 4), (6, 4))) == INVALID and 'span 1' in _err() and 'offset must be a multiple of 4' in _err()
    assert run(_table((0, 100), (100, 29))) == INVALID and 'span 1' in _err() and 'exceeds data_bytes' in _err()
    assert run(_table((132, 0))) == INVALID and 'span 0' in _err() and 'exceeds data_bytes' in _err()
    assert run(_table((0, 4), (I64_MAX - 3, 4)), data_bytes=I64_MAX) == INVALID and 'span 1' in _err() and 'overflows' in _err()
    assert run(_table((0, I64_MAX)), data_bytes=I64_MAX) == INVALID and 'span 0' in _err() and '2^40 tiles' in _err()
    assert run(_table((0, TILE * ((1 << 40) - 1)), (0, 1)), data_bytes=I64_MAX) == INVALID and 'span 1' in _err() and '2^40 tiles' in _err()
    assert run(data=FAKE + 2) == INVALID and 'data and crc_out must be 4-byte aligned' in _err()
    assert run(out=FAKE + 2) == INVALID and 'data and crc_out must be 4-byte aligned' in _err()
    assert run(spans=FAKE + 4) == INVALID and 'spans (the device table) must be 8-byte aligned' in _err()
    assert run(ws=FAKE + 8) == INVALID and 'workspace must be 16-byte aligned' in _err()
    need = lib.l3c_u8_crc32_spans_workspace_bytes(good.ctypes.data, good.shape[0])
    assert need > 0
    assert run(ws_bytes=need - 1) == INVALID and 'workspace_bytes too small' in _err()
    assert run(ws_bytes=0) == INVALID and 'workspace_bytes too small' in _err()


def test_arguments_are_checked_before_the_launch():
    check_rejected_arguments()
