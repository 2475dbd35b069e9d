"""Framing of a PREFIX of a `.l3c` file (container.prefix_bytes / parse_prefix: what Bitcoding.decode_preview reads), both formats, and
the argument checks of l3c_dmll_mean.  No GPU."""
import os
import struct

import numpy as np
import pytest

from tests.conftest import GOLDEN

from l3c_pytorch_amd import _lib
from l3c_pytorch_amd.bitcoding import container

SEP = b'\x46\xE2\x84\x92'


def _golden(name):
    with open(os.path.join(GOLDEN, name), 'rb') as f:
        return f.read()


def _banded_file(seed=0, first_c=5):
    """A banded file of four records (several bands per channel from the second record on) with random payloads."""
    rng = np.random.RandomState(seed)
    scales = [(first_c, 4, 6, 64), (5, 8, 12, 64), (5, 16, 24, 128), (3, 32, 48, 512)]
    payloads = [[[rng.bytes(int(rng.randint(0, 40))) for _ in range(container.n_bands(H * W, L))] for _ in range(C)] for C, H, W, L in scales]
    return container.write_file((1, 2, 3, 4), scales, payloads, True)


def _full(data):
    """The full parser's framing of one file in parse_batch's form: (records, streams, banded)."""
    return container.parse_batch([data])


FILES = [('legacy cr', lambda: _golden('hip_l3c_cal_64x96.l3c'), 4), ('legacy rgb shared', lambda: _golden('hip_rgb_shared_32x48_r3.l3c'), 5),
         ('banded', _banded_file, 4)]


@pytest.mark.parametrize('what,make,n_records', FILES, ids=[f[0] for f in FILES])
def test_every_record_boundary_and_the_cuts_around_it(what, make, n_records):
    data = make()
    records, streams, banded = _full(data)
    assert len(records) == n_records
    ends = [container.prefix_bytes(data, r) for r in range(1, n_records + 1)]
    assert ends == sorted(set(ends)) and ends[-1] == len(data)
    header = 14 if banded else 8
    for r, end in enumerate(ends, 1):
        # the boundary is where the full parser's last payload of record r ends, plus the separator
        assert end == int(streams.offset[r - 1][0, -1] + streams.nbytes[r - 1][0, -1]) + 4
        assert data[end - 4:end] == SEP
        nxt = ends[r] if r < n_records else None
        cuts = [(end, r), (end - 1, r - 1)]
        if nxt is not None:
            cuts += [(end + 1, r), ((end + nxt) // 2, r), (nxt - 1, r)]
        for cut, n_want in cuts:
            piece = data[:cut]
            if n_want == 0:
                assert cut > header
                with pytest.raises(ValueError, match='invalid file'):
                    container.parse_prefix([piece])
                with pytest.raises(ValueError, match='invalid file'):
                    container.prefix_bytes(piece, 1)
                continue
            recs, st, b, n = container.parse_prefix([piece])
            assert (n, b) == (n_want, banded) and recs == list(records[:n]) and len(st.scales) == n
            assert st.padding == streams.padding and st.scales == streams.scales[:n]
            for k in range(n):
                assert np.array_equal(st.offset[k], streams.offset[k]) and np.array_equal(st.nbytes[k], streams.nbytes[k])
                assert st.offset[k].dtype == np.int64 and st.offset[k].shape == (1, streams.scales[k][0])
            assert container.prefix_bytes(piece, n) == ends[n - 1]
            with pytest.raises(ValueError):
                container.prefix_bytes(piece, n + 1)
            # max_records caps; the data behind the cap is not looked at
            for cap in range(1, n + 1):
                assert container.parse_prefix([piece], cap)[3] == cap
                assert container.parse_prefix([data[:ends[cap - 1]] + b'\xff' * 7], cap)[3] == cap
    with pytest.raises(ValueError):
        container.prefix_bytes(data, 0)
    with pytest.raises(ValueError):
        container.parse_prefix([data], 0)


@pytest.mark.parametrize('what,make,n_records', FILES, ids=[f[0] for f in FILES])
def test_data_shorter_than_one_record_raises(what, make, n_records):
    data = make()
    first = container.prefix_bytes(data, 1)
    for cut in (0, 3, 4, 7, 8, 13, 14, 15, first // 2, first - 1):
        with pytest.raises(ValueError, match='invalid file'):
            container.parse_prefix([data[:cut]])
    assert container.parse_prefix([data[:first]])[3] == 1


def test_a_batch_takes_the_records_complete_in_every_file_and_refuses_mixtures():
    legacy = _golden('hip_l3c_cal_64x96.l3c')
    banded = _banded_file()
    e = [container.prefix_bytes(legacy, r) for r in (1, 2, 3, 4)]
    recs, st, b, n = container.parse_prefix([legacy, legacy[:e[1] + 5], legacy[:e[2]]])
    assert n == 2 and not b and st.offset[1].shape == (3, recs[1][0]) and len(st.padding) == 3
    assert np.array_equal(st.offset[1][0], st.offset[1][1])
    assert container.parse_prefix([legacy, legacy], 3)[3] == 3
    with pytest.raises(ValueError, match='mixes banded and legacy'):
        container.parse_prefix([legacy, banded])
    with pytest.raises(ValueError, match='mixes banded and legacy'):
        container.parse_prefix([banded[:container.prefix_bytes(banded, 1)], legacy])
    # other shapes (the RGB Shared file), another channel count, another band length in a kept record
    with pytest.raises(ValueError, match='equally sized'):
        container.parse_prefix([legacy, _golden('hip_rgb_shared_32x48_r3.l3c')])
    with pytest.raises(ValueError, match='equally sized'):
        container.parse_prefix([banded, _banded_file(1, first_c=4)])
    other_L = bytearray(banded)
    assert struct.unpack_from('<BHHI', other_L, 14) == (5, 4, 6, 64)
    struct.pack_into('<I', other_L, 19, 128)
    with pytest.raises(ValueError, match='band length'):
        container.parse_prefix([banded, bytes(other_L)])
    # ... but a difference behind the kept records is not looked at
    two = container.prefix_bytes(banded, 2)
    assert container.parse_prefix([banded, banded[:two] + b'\x00' * 9], 2)[3] == 2
    with pytest.raises(ValueError):
        container.parse_prefix([])


def _patched(data, at, fmt, *values):
    d = bytearray(data)
    struct.pack_into(fmt, d, at, *values)
    return bytes(d)


def test_corrupted_kept_records_raise_as_the_full_parsers_do():
    legacy = _golden('hip_l3c_cal_64x96.l3c')
    e = [0] + [container.prefix_bytes(legacy, r) for r in (1, 2, 3, 4)]
    bad = {
        'C == 0 in record 1': _patched(legacy, 8, '<B', 0),
        'C == 0 in record 2': _patched(legacy, e[1], '<B', 0),
        'separator of record 1': _patched(legacy, e[1] - 4, '<I', 0),
        'separator of record 3': _patched(legacy, e[3] - 1, '<B', 0),
    }
    for what, data in bad.items():
        with pytest.raises(ValueError, match='invalid file'):
            container.parse_prefix([data])
        with pytest.raises(ValueError, match='invalid file'):
            container.parse_containers([data])
    # a prefix that ends before the damage does not see it; one that holds it does
    assert container.parse_prefix([bad['separator of record 3'][:e[2] + 3]])[3] == 2
    assert container.parse_prefix([bad['separator of record 3']], 2)[3] == 2
    with pytest.raises(ValueError, match='separator'):
        container.parse_prefix([bad['separator of record 3'][:e[3]]])
    # a length field that points past the end of the data is a cut, not damage: the record is not kept
    assert container.parse_prefix([_patched(legacy, e[2] + 5, '<I', 1 << 30)])[3] == 2

    banded = _banded_file()
    b = [0] + [container.prefix_bytes(banded, r) for r in (1, 2, 3, 4)]
    assert b[0] == 0 and struct.unpack_from('<BHHI', banded, b[1]) == (5, 8, 12, 64)
    bad = {
        'version': (_patched(banded, 4, '<B', 2), 'version'),
        'reserved byte': (_patched(banded, 5, '<B', 1), 'reserved'),
        'C == 0': (_patched(banded, b[1], '<B', 0), 'C == 0'),
        'empty scale': (_patched(banded, b[1] + 1, '<H', 0), 'empty scale'),
        'L == 0': (_patched(banded, b[1] + 5, '<I', 0), 'band length'),
        'L not a multiple of 64': (_patched(banded, b[1] + 5, '<I', 96), 'band length'),
        'more than 1024 bands': (_patched(_patched(banded, b[1] + 1, '<HH', 600, 600), b[1] + 5, '<I', 64), 'bands per channel'),
        'separator': (_patched(banded, b[2] - 4, '<I', 0), 'separator'),
    }
    for what, (data, msg) in bad.items():
        with pytest.raises(ValueError, match='invalid file.*' + msg):
            container.parse_prefix([data])
        with pytest.raises(ValueError, match='invalid file'):
            container.parse_banded(data)
        if what not in ('version', 'reserved byte'):
            assert container.parse_prefix([data], 1)[3] == 1          # the first record is sound
    # the full parsers and their minimum of two records are as they were
    with pytest.raises(ValueError, match='1 scale record'):
        container.parse_banded(banded[:b[1]])
    with pytest.raises(ValueError, match='1 scale record'):
        container.parse_containers([legacy[:e[1]]])


def test_dmll_mean_argument_validation_precedes_any_launch():
    """Status and message, without a GPU: fake but well-aligned pointers stand in for device memory (never dereferenced here)."""
    lib = _lib.load()
    fake = 0x1000

    def err():
        return lib.l3c_last_error().decode()

    assert lib.l3c_dmll_mean(None, 1, 10, 3, 10, 1, 0.0, 255.0, 256, fake, None) == -1 and 'null pointer' in err()
    assert lib.l3c_dmll_mean(fake, 1, 10, 3, 10, 1, 0.0, 255.0, 256, None, None) == -1 and 'null pointer' in err()
    assert lib.l3c_dmll_mean(fake, 1, 10, 5, 10, 1, 0.0, 255.0, 256, fake, None) == -1 and 'C == 3' in err()
    for B, HW, C in ((0, 10, 5), (-1, 10, 5), (1, 0, 5), (1, -3, 5), (1, 10, 0), (65536, 10, 5)):
        assert lib.l3c_dmll_mean(fake, B, HW, C, 10, 0, -1.0, 1.0, 25, fake, None) == -1 and 'bad shape' in err()
    for K in (0, -1, 17):
        assert lib.l3c_dmll_mean(fake, 1, 10, 5, K, 0, -1.0, 1.0, 25, fake, None) == -1 and 'K out of range' in err()
    for x_min, x_max, L in ((-1.0, 1.0, 1), (-1.0, 1.0, 0), (-1.0, 1.0, 32769), (1.0, 1.0, 25), (2.0, 1.0, 25)):
        assert lib.l3c_dmll_mean(fake, 1, 10, 5, 10, 0, x_min, x_max, L, fake, None) == -1 and 'alphabet out of range' in err()
    assert lib.l3c_dmll_mean(fake, 1, 10, 16, 16, 0, -1.0, 1.0, 25, fake, None) == -1 and 'LDS tile' in err()
