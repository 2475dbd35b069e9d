"""Banded `.l3c` files on the host (no GPU): the band-length policy, the parser of the framing, the rejection of malformed files, and
that the legacy format is still read as before.  The payloads are made by the oracle range coder over band slices of random tables."""
import struct

import numpy as np
import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd.bitcoding.bitcoding import (_MAGIC_VALUE_SEP, BANDED_SIGNATURE, band_len, count_scale_records, is_banded, n_bands,
                                                 parse_banded, parse_containers)
from oracle import ac


def random_rows(rng, n, Lp):
    """n strictly increasing uint16 rows of Lp entries as the coder reads them: entry 0 = 0, entries 1..Lp-2 rising, entry Lp-1 = 65536 (0)."""
    w = rng.random((n, Lp - 1)) ** 4 + 1e-3
    counts = 1 + np.floor(w / w.sum(axis=1, keepdims=True) * (65536 - (Lp - 1) - Lp)).astype(np.int64)
    cdf = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(counts, axis=1)], axis=1)
    assert (cdf[:, -2] < 65536).all()
    cdf[:, -1] = 65536
    return (cdf & 0xFFFF).astype(np.uint16)


def banded_file(scales, padding=(0, 0, 0, 0), version=1, reserved=0):
    """scales: [(C, H, W, L, payloads[c][j])] coarsest first -> the bytes of a banded file."""
    out = [BANDED_SIGNATURE, struct.pack('<BB4H', version, reserved, *padding)]
    for C, H, W, L, pay in scales:
        out.append(struct.pack('<BHHI', C, H, W, L))
        for bands in pay:
            for p in bands:
                out += [struct.pack('<I', len(p)), p]
        out.append(_MAGIC_VALUE_SEP)
    return b''.join(out)


def coded_scale(rng, C, H, W, K, Lp):
    """One scale coded band by band with the oracle: -> (C, H, W, L, payloads, symbols (C, HW), rows (C, HW, Lp))."""
    HW = H * W
    L = band_len(HW, K)
    rows = random_rows(rng, C * HW, Lp).reshape(C, HW, Lp)
    sym = rng.integers(0, Lp - 1, size=(C, HW)).astype(np.int16)
    pay = [[ac.encode(rows[c, j * L:(j + 1) * L], sym[c, j * L:(j + 1) * L]) for j in range(n_bands(HW, L))] for c in range(C)]
    return C, H, W, L, pay, sym, rows


def test_band_length_policy():
    for hw, K in [(393216, 64), (98304, 64), (6144, 64), (24, 64), (200, 3), (100, 1), (4096, 1024), (393216, 7), (64, 2), (65, 2)]:
        L = band_len(hw, K)
        assert L == 64 * -(-hw // (64 * K)) and L % 64 == 0 and L >= 64
        n = n_bands(hw, L)
        assert 1 <= n <= K and (n - 1) * L < hw <= n * L
    assert band_len(393216, 64) == 6144 and n_bands(393216, 6144) == 64
    assert band_len(6144, 64) == 128 and n_bands(6144, 128) == 48          # small scales: 64-symbol blocks, fewer bands than asked for
    assert band_len(24, 64) == 64 and n_bands(24, 64) == 1                 # fewer than 64 symbols: one band
    assert band_len(393216, 1) == 393216
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError):
            band_len(1000, bad)


def test_parser_returns_every_band_of_oracle_coded_files():
    rng = np.random.default_rng(7)
    # a scale of fewer than 64 symbols (Lp 26, one band), a scale with a short last band (Lp 257: 200 = 128 + 72), a scale of equal bands
    s0 = coded_scale(rng, 2, 4, 6, 64, 26)
    s1 = coded_scale(rng, 3, 10, 20, 3, 257)
    s2 = coded_scale(rng, 1, 16, 16, 4, 257)
    assert (s0[3], s1[3], s2[3]) == (64, 128, 64)
    scales = [s0, s1, s2]
    data = banded_file([s[:5] for s in scales], padding=(1, 2, 3, 4))
    assert is_banded(data)
    p = parse_banded(data)
    assert p.padding == (1, 2, 3, 4)
    assert p.scales == [(2, 4, 6, 64), (3, 10, 20, 128), (1, 16, 16, 64)]
    for k, (C, H, W, L, pay, sym, rows) in enumerate(scales):
        n = n_bands(H * W, L)
        assert p.offset[k].shape == p.nbytes[k].shape == (C, n)
        for c in range(C):
            for j in range(n):
                o, nb = int(p.offset[k][c, j]), int(p.nbytes[k][c, j])
                assert data[o:o + nb] == pay[c][j]
                band = slice(j * L, min((j + 1) * L, H * W))
                assert np.array_equal(ac.decode(rows[c, band], data[o:o + nb]), sym[c, band])
    # the offsets are consecutive: every band's length field sits right in front of it
    assert p.offset[0][0, 0] == 14 + 9 + 4


def test_every_malformed_banded_file_raises():
    rng = np.random.default_rng(3)
    s0, s1 = coded_scale(rng, 2, 4, 6, 8, 26), coded_scale(rng, 3, 8, 12, 8, 257)
    good = [s0[:5], s1[:5]]
    parse_banded(banded_file(good))

    def bad(data, what):
        with pytest.raises(ValueError, match='invalid file'):
            parse_banded(data)
        assert what

    bad(banded_file(good, version=2), 'unknown version')
    bad(banded_file(good, reserved=1), 'reserved byte')
    bad(banded_file([(0, 4, 6, 64, [])] + good[1:]), 'C == 0')
    bad(banded_file([good[0][:3] + (0, good[0][4])] + good[1:]), 'L == 0')
    bad(banded_file([good[0][:3] + (96, good[0][4])] + good[1:]), 'L % 64 != 0')
    # n > 1024: 1025 bands of 64 symbols (H*W = 65600), every band empty
    bad(banded_file([(1, 100, 656, 64, [[b''] * 1025])] + good[1:]), 'more than 1024 bands')
    full = banded_file(good)
    bad(full[:-1], 'missing magic at the end')
    bad(full[:-30], 'payload past the end')
    bad(full[:20], 'length field past the end')
    bad(full + b'\x00', 'trailing byte')
    bad(full + b'\x00' * 16, 'trailing bytes')
    # a length field that claims more than the file holds
    p = parse_banded(full)
    o = int(p.offset[1][2, 0]) - 4
    bad(full[:o] + struct.pack('<I', 1 << 30) + full[o + 4:], 'length past the end')
    # a missing magic between scales
    o = int(p.offset[0][-1, -1] + p.nbytes[0][-1, -1])
    bad(full[:o] + b'\x00\x00\x00\x00' + full[o + 4:], 'missing magic')
    bad(banded_file(good[:1]), 'one scale record')
    # the legacy readers refuse a banded file, naming the format
    with pytest.raises(ValueError, match='banded'):
        count_scale_records(full)
    with pytest.raises(ValueError, match='banded'):
        parse_containers([full])


def test_banded_entry_points_check_their_arguments_before_any_launch():
    """Status codes and messages, WITHOUT a GPU: every call below is refused by its argument checks, before any HIP call.  Fake but
    well-aligned non-null pointers stand in for device memory (never dereferenced on these paths)."""
    import ctypes
    from l3c_pytorch_amd import _lib
    lib = _lib.load()
    fake = 0x10000

    def err():
        return lib.l3c_last_error().decode()
    # interval relayout
    assert lib.l3c_ac_band_intervals(fake, 4, 1000, 96, fake, fake, None) == -1 and 'multiple of 64' in err()
    assert lib.l3c_ac_band_intervals(fake, 4, 1000, 128, None, fake, None) == -1 and 'full bands' in err()
    assert lib.l3c_ac_band_intervals(fake + 4, 4, 1000, 128, fake, fake, None) == -1 and '16-byte aligned' in err()
    assert lib.l3c_ac_band_intervals(None, 4, 1000, 128, fake, fake, None) == -1 and 'null pointer' in err()
    # banded container
    sc = (_lib.BandedScale * 1)(_lib.BandedScale(fake, fake, 64, fake, fake, 64, 5, 8, 8, 96))
    assert lib.l3c_container_write_banded_workspace_bytes(sc, 1, 2) == -1 and 'multiple of 64' in err()
    sc[0].band_len = 64
    assert lib.l3c_container_write_banded_workspace_bytes(sc, 1, 2) == 2 * 5 * 1 * 8
    sc[0].H, sc[0].W = 256, 257                                     # 1028 bands of 64
    assert lib.l3c_container_write_banded(sc, 1, 2, fake, fake, fake, fake, 1 << 20, None) == -1 and '1024 bands' in err()
    sc[0].H, sc[0].W, sc[0].stride_last = 16, 16, 6
    assert lib.l3c_container_write_banded(sc, 1, 2, fake, fake, fake, fake, 1 << 20, None) == -1 and '4-byte aligned' in err()
    sc[0].stride_last, sc[0].out_full = 64, None
    assert lib.l3c_container_write_banded(sc, 1, 2, fake, fake, fake, fake, 1 << 20, None) == -1 and 'null pointer' in err()
    sc[0].out_full = fake
    assert lib.l3c_container_write_banded(sc, 1, 2, fake, fake, fake, fake, 8, None) == -1 and 'workspace' in err()
    assert lib.l3c_container_write_banded(sc, 9, 2, fake, fake, fake, fake, 1 << 20, None) == -1 and 'scales' in err()
    # banded RGB decode
    assert lib.l3c_decode_rgb_banded_workspace_bytes(1, 1000, 96, 4, 1) == -1
    assert lib.l3c_decode_rgb_banded_workspace_bytes(1, 1000, 128, 4, 3) == -1
    assert lib.l3c_decode_rgb_banded_workspace_bytes(2, 1000, 128, 1, 1) > 0
    d = _lib.RgbBandedDesc(fake, fake, fake, 2, 1000, 10, fake, fake, fake, 128, 1, 1, 1, fake, 1 << 30)

    def rgb(**kw):
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.l3c_decode_rgb_banded(ctypes.byref(d), None, None)
    assert rgb(band_len=100) == -1 and 'multiple of 64' in err()
    assert rgb(band_len=128, n_chunks=2) == -1 and '64 symbols per chunk' in err()        # last band: 1000 - 7 * 128 = 104 symbols
    assert rgb(n_chunks=1, lag=2) == -1 and 'side stream' in err()
    assert rgb(lag=1, window_mode=3) == -1 and 'window_mode' in err()
    assert rgb(window_mode=1, in_=fake + 2) == -1 and 'misaligned' in err()
    assert rgb(in_=fake, B=70000) == -1 and '65535 bands' in err()
    assert rgb(B=2, workspace=fake + 64) == -1 and '256-byte aligned' in err()
    assert rgb(workspace=fake, workspace_bytes=64) == -1 and 'workspace too small' in err()
    assert rgb(workspace_bytes=1 << 30, K=17) == -1 and 'bad shape' in err()
    assert rgb(K=10, P=None) == -1 and 'null pointer' in err()


def test_legacy_file_is_parsed_as_before():
    """A legacy file never starts with the signature (its first u16 is the left padding, below the padding factor) and is read by
    the legacy parser unchanged."""
    out = [struct.pack('<4H', 3, 0, 5, 0)]
    for C, H, W in [(5, 4, 6), (3, 8, 12)]:
        out.append(struct.pack('<BHH', C, H, W))
        for c in range(C):
            out += [struct.pack('<I', c + 1), bytes(c + 1)]
        out.append(_MAGIC_VALUE_SEP)
    data = b''.join(out)
    assert not is_banded(data) and struct.unpack('<H', BANDED_SIGNATURE[:2])[0] == 13132
    assert count_scale_records(data) == 2
    p = parse_containers([data])
    assert p.padding == [(3, 0, 5, 0)] and p.scales == [(5, 4, 6), (3, 8, 12)]
    assert p.nbytes[1].tolist() == [[1, 2, 3]]
    with pytest.raises(ValueError):
        parse_banded(data)
