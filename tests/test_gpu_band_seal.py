"""-m gpu: band-sealed `.l3c` files (Bitcoding(bp, bands=K, seal='bands'), NativeCodec(bp, bands=K, seal='bands'); include/l3c_hip.h "band
seals": l3c_u8_crc32_bands, l3c_seal_append_bands; container.make_seal / split_seal / check_band_crcs).

Every expectation comes from zlib.crc32 on the host and from the input pixels.  Frames are 320x88 (a 317x83 image centre-padded, or the
whole frame) at K = 16 -- bands of 1792 symbols, 20.4 rows -- and 64x64 at K = 64, a row per band."""
import struct
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from l3c_pytorch_amd.bitcoding.container import SealError  # noqa: E402
from l3c_pytorch_amd.helpers import dataset_codec, pad, synthetic  # noqa: E402
from tests.test_gpu_region import Calls, bitcoding, blueprint, crop, encoded, images  # noqa: E402

_CACHE = {}


def native(K, seal=False):
    from l3c_pytorch_amd.native_codec import NativeCodec
    if ('n', K, seal) not in _CACHE:
        _CACHE['n', K, seal] = NativeCodec(blueprint(), bands=K, seal=seal)
    return _CACHE['n', K, seal]


def frames_of(B, H, W):
    """(padded uint8 frames (B, 3, Hp, Wp) on the host, padding tuple) of the images the region tests encode."""
    x = images(B, H, W)
    fac = bitcoding(16).padding_factor()
    if H % fac or W % fac:
        padded, padding = pad.pad(x.long(), fac=fac, mode=blueprint().get_padding_mode())
        return padded.to(torch.uint8), tuple(padding)
    return x, (0, 0, 0, 0)


def band_words(frame, L):
    """zlib.crc32 of every band of a (3, H, W) uint8 numpy frame -> (3, n) uint32."""
    HW = frame.shape[1] * frame.shape[2]
    planes = [np.ascontiguousarray(p).tobytes() for p in frame]
    return np.asarray([[zlib.crc32(p[j * L:(j + 1) * L]) for j in range(container.n_bands(HW, L))] for p in planes], dtype=np.uint32)


def complemented(data, bands, channels=(0, 1, 2)):
    """The file with the streams of `bands` of `channels` of its finest record complemented."""
    body = container.split_seal(data)[0]
    parsed = container.parse_banded(body)
    offset, nbytes = parsed.offset[-1], parsed.nbytes[-1]
    out = np.frombuffer(data, dtype=np.uint8).copy()
    for c in channels:
        for j in bands:
            a, n = int(offset[c, j]), int(nbytes[c, j])
            assert n > 16
            out[a:a + n] ^= 0xFF
    return out.tobytes()


# ---- 1. structure ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('K,B,H,W', [(16, 2, 317, 83), (64, 1, 64, 64)])
def test_body_table_and_frame_word(K, B, H, W):
    _, plain, padding = encoded(K, B, H, W)
    _, sealed, _ = encoded(K, B, H, W, seal='bands')
    _, v1, _ = encoded(K, B, H, W, seal=True)
    frames, _ = frames_of(B, H, W)
    Hp, Wp = frames.shape[2:]
    L = container.band_len(Hp * Wp, K)
    n = container.n_bands(Hp * Wp, L)
    for b in range(B):
        body, seal = container.split_seal(sealed[b])
        assert body == plain[b] and sealed[b][:len(plain[b])] == plain[b]
        assert len(sealed[b]) == len(plain[b]) + 20 + 12 * n + 24
        f = frames[b].numpy()
        assert seal.band_len == L and seal.band_crcs.shape == (3, n)
        assert (seal.band_crcs == band_words(f, L)).all()
        assert seal.frame_crc == zlib.crc32(np.ascontiguousarray(f).tobytes())
        assert seal.generation == bitcoding(K).generation() and seal.model_id == bitcoding(K).model_id()
        assert v1[b] == plain[b] + container.make_seal(plain[b], seal.generation, seal.frame_crc, seal.model_id) and len(v1[b]) == len(plain[b]) + 24
    x = frames.cuda()
    assert native(K, 'bands').encode_batch(x, [padding] * B) == sealed                   # byte for byte, table and seal included
    assert native(K, True).encode_batch(x, [padding] * B) == v1
    assert native(K).encode_batch(x, [padding] * B) == plain


def test_constructors():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.native_codec import NativeCodec
    for cls in (Bitcoding, NativeCodec):
        with pytest.raises(ValueError, match="seal='bands' needs banded files"):
            cls(blueprint(), bands=0, seal='bands')


# ---- 2. each side decodes the other's files ----------------------------------------------------------------------------------------


def test_each_side_decodes_the_other_and_a_mixed_batch():
    K, B, H, W = 16, 2, 317, 83
    _, plain, padding = encoded(K, B, H, W)
    _, sealed, _ = encoded(K, B, H, W, seal='bands')
    _, v1, _ = encoded(K, B, H, W, seal=True)
    frames = frames_of(B, H, W)[0].cuda()
    files = native(K, 'bands').encode_batch(frames, [padding] * B)
    got, pads = bitcoding(K).decode_batch(files, out_dtype=torch.uint8)
    assert torch.equal(got, frames) and [tuple(p) for p in pads] == [padding] * B
    got, pads = native(K).decode_batch(sealed)
    assert torch.equal(got, frames) and pads == [padding] * B
    mixed = [plain[0], v1[1], sealed[0], sealed[1]]
    want = torch.stack([frames[0], frames[1], frames[0], frames[1]])
    assert torch.equal(bitcoding(K).decode_batch(mixed, out_dtype=torch.uint8)[0], want)
    assert torch.equal(native(K).decode_batch(mixed)[0], want)
    # ... and the mixed batch is VERIFIED: a damaged version-1 file and a damaged band-sealed file are both named
    bad = [plain[0], complemented(v1[1], [2]), sealed[0], complemented(sealed[1], [5], [0])]
    for decode in (lambda f: bitcoding(K).decode_batch(f, out_dtype=torch.uint8), native(K).decode_batch):
        with pytest.raises(SealError) as e:
            decode(bad)
        assert e.value.reason == 'pixels' and e.value.failed == [1, 3] and list(e.value.bands) == [3]
        assert (0, 5) in e.value.bands[3] and {j for _, j in e.value.bands[3]} == {5}


# ---- 3. damage is located ----------------------------------------------------------------------------------------------------------


def test_a_damaged_band_is_named_with_its_rows():
    x, sealed, _ = encoded(16, 1, 320, 88, seal='bands')
    L = 1792
    bad = complemented(sealed[0], [3], [1])                                   # band 3's stream of G only
    for codec in (bitcoding(16), native(16)):
        got = codec.decode_batch([bad], verify=False)[0].to(torch.uint8)
        differ = [(c, j) for c in range(3) for j in range(16)
                  if not torch.equal(got[0, c].reshape(-1)[j * L:(j + 1) * L], x[0, c].reshape(-1)[j * L:(j + 1) * L])]
        assert (1, 3) in differ and (0, 3) not in differ and {j for _, j in differ} == {3}
        with pytest.raises(SealError) as e:
            codec.decode_batch([bad])
        assert e.value.reason == 'pixels' and e.value.index == 0 and e.value.failed == [0]
        assert e.value.bands == {0: differ}
        assert e.value.rows == {0: (3 * L // 88, -(-4 * L // 88))} == {0: (61, 82)}
    assert torch.equal(bitcoding(16).decode_batch(sealed, out_dtype=torch.uint8)[0], x)


def test_region_decode_verifies_the_bands_it_decodes():
    x, sealed, _ = encoded(16, 1, 320, 88, seal='bands')
    bc = bitcoding(16)
    bad = complemented(sealed[0], [3, 13])
    got, info = bc.decode_region([bad], (190, 210))                           # bands 9 and 10
    assert torch.equal(got, crop(x, (190, 210)))
    assert info.pixel_crc_checked is True and info.verified == ('generation', 'model', 'bands') and info.sealed == 1
    assert info.bands == (9, 11) and info.sym_rows == (183, 224)              # the last band whole: 11 * 1792 / 88 = 224
    assert 'bands 9..10' in info.line() and 'verified' in info.line()
    with pytest.raises(SealError) as e:
        bc.decode_region([bad], (60, 70))
    assert e.value.reason == 'pixels' and e.value.bands == {0: [(0, 3), (1, 3), (2, 3)]} and e.value.rows == {0: (61, 82)}
    # verify=False: today's cut plan and today's info
    got, info = bc.decode_region([bad], (190, 210), verify=False)
    assert torch.equal(got, crop(x, (190, 210)))
    assert info.sym_rows == (183, 210) and info.pixel_crc_checked is False and info.verified == ()
    # a version-1 sealed file: the cut plan, unverified pixels, as before
    _, v1, _ = encoded(16, 1, 320, 88, seal=True)
    got, info = bc.decode_region(v1, (190, 210))
    assert info.sym_rows == (183, 210) and info.pixel_crc_checked is False and info.verified == ('generation', 'model')
    # both in one call: the whole-band plan, the band-sealed file checked, not every sealed file of the call
    got, info = bc.decode_region([v1[0], sealed[0]], (190, 210))
    assert torch.equal(got, torch.cat([crop(x, (190, 210))] * 2)) and info.sym_rows == (183, 224) and info.pixel_crc_checked is False
    assert info.verified == ('generation', 'model', 'bands') and info.sealed == 2
    # a padded image and a batch: rows of the unpadded image
    xp, sp, padding = encoded(16, 2, 317, 83, seal='bands')
    got, info = bc.decode_region(sp, (100, 140, 5, 60))
    assert torch.equal(got, crop(xp, (100, 140, 5, 60))) and info.pixel_crc_checked is True
    with pytest.raises(SealError) as e:
        bc.decode_region([sp[0], complemented(sp[1], [0], [2])], (0, 10))
    assert e.value.index == 1 and e.value.bands == {1: [(2, 0)]} and e.value.rows == {1: (0, 21 - padding[2])}
    # the native region decode treats a band-sealed file as a version-1 sealed one
    got, info = native(16).decode_region(sealed, (190, 210))
    assert torch.equal(got, crop(x, (190, 210))) and info.pixel_crc_checked is False and info.verified == ('generation', 'model')


# ---- 4. a damaged table is refused before any library call -------------------------------------------------------------------------


def test_a_changed_table_is_invalid_before_any_library_call(monkeypatch):
    _, sealed, _ = encoded(16, 1, 320, 88, seal='bands')
    f = sealed[0]
    body, seal = container.split_seal(f)
    T = 20 + 12 * 16

    def resealed(table):
        head = f[-24:-4]
        return body + table + head + struct.pack('<I', zlib.crc32(body[6:14] + table + head))
    table = f[len(body):len(body) + T]
    word = resealed(table[:12 + 4 * 20] + bytes([table[12 + 4 * 20] ^ 1]) + table[13 + 4 * 20:])
    other_L = resealed(table[:8] + struct.pack('<I', 1856) + table[12:])
    raw = f[:len(body) + 40] + bytes([f[len(body) + 40] ^ 0x80]) + f[len(body) + 41:]          # a table byte under the old check word
    calls = Calls(monkeypatch)
    for bad, needle in ((word, 'combination'), (other_L, 'finest scale record'), (raw, 'check word')):
        for decode in (bitcoding(16).decode_batch, native(16).decode_batch, lambda files: bitcoding(16).decode_region(files, (10, 20)),
                       lambda files: native(16).decode_region(files, (10, 20)), lambda files: bitcoding(16).decode_preview(files)):
            with pytest.raises(ValueError, match='invalid file: seal') as e:
                decode([bad])
            assert needle in str(e.value) and not isinstance(e.value, SealError)
    assert calls.n == 0
    bitcoding(16).decode_batch(sealed)
    assert calls.n > 0


# ---- 5. set readers and the preview ------------------------------------------------------------------------------------------------


def test_set_readers_verify_the_frame_crc_and_the_preview_strips_the_seal():
    K = 16
    xa, plain, _ = encoded(K, 1, 320, 88)
    _, v1, _ = encoded(K, 1, 320, 88, seal=True)
    _, sealed, _ = encoded(K, 1, 320, 88, seal='bands')
    xb, sealed_b, _ = encoded(K, 2, 317, 83, seal='bands')
    bc = bitcoding(K)
    files = {0: plain[0], 1: v1[0], 2: sealed[0], 3: sealed_b[0], 4: sealed_b[1]}
    want = {0: xa[0], 1: xa[0], 2: xa[0], 3: xb[0], 4: xb[1]}
    back = dataset_codec.decode_set(bc, files, list(files), banded=True, sealed=True)
    assert all(torch.equal(back[i].cuda(), want[i]) for i in files)
    files[4] = complemented(sealed_b[1], [7], [0])
    status = dataset_codec.verify_set(bc, files, list(files), banded=True)
    assert status == {0: 'unsealed', 1: 'ok', 2: 'ok', 3: 'ok', 4: 'pixels'}
    with pytest.raises(SealError) as e:
        dataset_codec.decode_set(bc, files, list(files), banded=True, sealed=True)
    assert e.value.reason == 'pixels' and e.value.failed == [4]
    a, _ = bc.decode_preview(sealed)
    b, _ = bc.decode_preview(plain)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match='cannot carry a seal'):
        bitcoding(K, 'bands').encode_batch(xa).to_host_buffer()


# ---- 6. l3c_seal_append_bands alone ------------------------------------------------------------------------------------------------


def test_seal_append_bands_alone():
    from l3c_pytorch_amd import _lib, ops
    rng = np.random.RandomState(5)
    for n, L in ((1, 64), (4, 64), (16, 1792), (64, 6144), (1024, 64)):
        need = 20 + 12 * n + 24
        assert _lib.load().l3c_seal_bands_bytes(n) == need
        stride = 200 + need
        B = 3
        pads = np.asarray([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], dtype=np.uint16)
        host = rng.randint(0, 256, (B, stride)).astype(np.uint8)
        for b in range(B):
            host[b, :14] = np.frombuffer(b'L3CB\x01\x00' + pads[b].tobytes(), dtype=np.uint8)
        sizes = np.asarray([200, 201, -1], dtype=np.int64)                   # room exactly; one byte short; an overrun file stays -1
        frame = rng.randint(0, 1 << 32, B, dtype=np.int64).astype(np.uint32)
        bands = rng.randint(0, 1 << 32, (B, 3, n), dtype=np.int64).astype(np.uint32)
        files = torch.from_numpy(host.copy()).cuda()
        file_bytes = torch.from_numpy(sizes.copy()).cuda()
        ops.seal_append_bands(files, file_bytes, torch.from_numpy(frame.view(np.int32)).cuda(), torch.from_numpy(bands.view(np.int32)).cuda(), L,
                              torch.from_numpy(pads.view(np.int16)).cuda(), 0xFEDCBA9876543210)
        got, got_sizes = files.cpu().numpy(), file_bytes.cpu().numpy()
        assert got_sizes.tolist() == [200 + need, -1, -1], (n, got_sizes)
        assert (got[1] == host[1]).all() and (got[2] == host[2]).all()       # nothing stored in a slot that is not sealed
        body = host[0, :200].tobytes()
        head = b'L3CS' + struct.pack('<BBHIQ', 2, 0, _lib.load().l3c_bitstream_generation(), int(frame[0]), 0xFEDCBA9876543210)
        table = b'L3CT' + struct.pack('<HHI', n, 0, L) + bands[0].astype('<u4').tobytes() + struct.pack('<I', 20 + 12 * n) + b'\x46\xE2\x84\x92'
        want = table + head + struct.pack('<I', zlib.crc32(body[6:14] + table + head))
        assert got[0, :200].tobytes() == body and got[0, 200:].tobytes() == want, n
        # no padding array: zeros go into the check word
        files = torch.from_numpy(host.copy()).cuda()
        file_bytes = torch.from_numpy(sizes.copy()).cuda()
        ops.seal_append_bands(files, file_bytes, torch.from_numpy(frame.view(np.int32)).cuda(), torch.from_numpy(bands.view(np.int32)).cuda(), L)
        head = b'L3CS' + struct.pack('<BBHIQ', 2, 0, _lib.load().l3c_bitstream_generation(), int(frame[0]), 0)
        assert files[0, 200:].cpu().numpy().tobytes() == table + head + struct.pack('<I', zlib.crc32(b'\0' * 8 + table + head))


# ---- 7. the CLI --------------------------------------------------------------------------------------------------------------------


def test_l3c_cli_band_seal(synthetic_l3c, tmp_path, capsys):
    """`l3c.py ... enc --bands 16 --seal-bands`, `dec` (the seal line with the number of band CRCs), `dec --region` (the checked bands); a
    damaged file: `dec` prints the damaged rows, `dec --region` outside them succeeds.  --seal-bands without --bands is refused."""
    import importlib.util
    import os
    from PIL import Image
    cfg, sd = synthetic_l3c
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = tmp_path / 'logs' / '0306_0001 cr oi' / 'ckpts'
    exp.mkdir(parents=True)
    torch.save({'net': sd}, str(exp / 'ckpt_0000000001.pt'))
    img = synthetic.make_image(190, 70, 22, 'natural')
    src, out, png = str(tmp_path / 'in.png'), str(tmp_path / 'out.l3c'), str(tmp_path / 'dec.png')
    Image.fromarray(img.permute(1, 2, 0).numpy()).save(src)
    spec = importlib.util.spec_from_file_location('l3c_cli', os.path.join(root, 'l3c.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    args = [str(tmp_path / 'logs'), '0306_0001']
    assert cli.main(args + ['enc', '--bands', '16', '--seal-bands', src, out]) == 0
    assert 'band-sealed' in capsys.readouterr().out
    data = open(out, 'rb').read()
    seal = container.split_seal(data)[1]
    assert seal.band_crcs.shape == (3, 16) and seal.band_len == 64 * 14                 # 192 x 72 padded: 13824 / 1024 = 13.5
    assert cli.main(args + ['dec', out, png]) == 0
    assert 'seal: ok (generation {}, 48 band CRCs)'.format(seal.generation) in capsys.readouterr().out
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1), img)
    assert cli.main(args + ['dec', '--region', '100:140,5:60', out, png]) == 0
    said = capsys.readouterr().out
    assert 'region rows [100, 140) x columns [5, 60): bands ' in said and 'band-sealed: generation and model checked, the CRCs of bands 8..11' in said
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1), img[:, 100:140, 5:60])
    with open(out, 'wb') as f:
        f.write(complemented(data, [2]))                                              # pixels [1792, 2688): frame rows 24..37, image rows 23..36
    assert cli.main(args + ['dec', out, png]) == 1
    said = capsys.readouterr().out
    assert 'DecodeError: seal:' in said and 'damaged rows: [23, 37)' in said and '--region' in said
    assert cli.main(args + ['dec', '--region', '100:140', out, png]) == 0
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1), img[:, 100:140])
    assert cli.main(args + ['dec', '--region', '30:50', out, png]) == 1
    assert 'DecodeError: seal:' in capsys.readouterr().out
    with pytest.raises(ValueError, match='--seal-bands needs --bands'):
        cli.main(args + ['enc', '--seal-bands', '-f', src, out])
