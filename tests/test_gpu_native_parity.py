"""-m gpu: parity-sealed files through the native codec -- NativeCodec(bp, bands=K, seal='bands', parity=G, parity_streams=R, parity_head=h)
writes, in ONE library call (l3c_encode_batch_banded_parity), the files of Bitcoding with the same arguments byte for byte; the existing
readers read them and Bitcoding.decode_repair repairs them.

The frames are those of tests/test_gpu_repair.py and tests/test_gpu_rs_repair.py: 320x88 at K = 16 -- L = 1792, n = 16 bands per channel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from l3c_pytorch_amd.helpers import pad  # noqa: E402
from tests.test_gpu_band_seal import native as band_sealed_native  # noqa: E402
from tests.test_gpu_head_repair import hurt  # noqa: E402
from tests.test_gpu_region import blueprint, images  # noqa: E402
from tests.test_gpu_rs_repair import damaged  # noqa: E402
from tests.test_gpu_salvage import NamedCalls  # noqa: E402

K = 16
CASES = [(4, 1, False), (4, 2, False), (4, 4, True), (3, 2, True), (64, 1, True)]      # (3, 2): m = 6, unequal groups; 64: G clamps to n
PADS = [(1, 2, 3, 4), (0, 7, 0, 5), (9, 0, 8, 1)]
_CACHE = {}


def native(G, R, head, bands=K):
    from l3c_pytorch_amd.native_codec import NativeCodec
    key = ('n', G, R, head, bands)
    if key not in _CACHE:
        _CACHE[key] = NativeCodec(blueprint(), bands=bands, seal='bands', parity=G, parity_streams=R, parity_head=head)
    return _CACHE[key]


def python(G, R, head, bands=K):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    key = ('p', G, R, head, bands)
    if key not in _CACHE:
        _CACHE[key] = Bitcoding(blueprint(), bands=bands, seal='bands', parity=G, parity_streams=R, parity_head=head)
    return _CACHE[key]


def native_files(G, R, head, B=1):
    """(the frames on the GPU, the native codec's files of them), encoded once per case."""
    key = ('f', G, R, head, B)
    if key not in _CACHE:
        x = images(B, 320, 88).cuda()
        _CACHE[key] = (x, native(G, R, head).encode_batch(x, PADS[:B] if B > 1 else None))
    return _CACHE[key]


def _same_files(got, want):
    assert [len(f) for f in got] == [len(f) for f in want]
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.nonzero(np.frombuffer(g, dtype=np.uint8) != np.frombuffer(w, dtype=np.uint8))[0]
        assert bad.size == 0, 'file {}: first differing byte {} of {} (body {}); {} differ'.format(
            k, bad[0], len(w), len(container.split_seal(w)[0]), bad.size)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('G,R,head', CASES)
def test_the_files_are_bitcodings_byte_for_byte(G, R, head, B):
    x, got = native_files(G, R, head, B)
    pads = PADS[:B] if B > 1 else [(0, 0, 0, 0)]
    want = python(G, R, head).encode_batch(x).to_bytes(pads)
    _same_files(got, want)
    for f in got:
        body, seal = container.split_seal(f)
        assert f[len(body):len(body) + 4] == (b'L3CH' if head else b'L3CP' if R == 1 else b'L3CQ') and f[-20] == 3
        assert (seal.parity_group, seal.parity_groups, seal.parity_streams) == (min(G, 16), -(-16 // min(G, 16)), R)
        assert (seal.head is not None) == head and not seal.head_damaged
    if B == 3:
        assert got[0] != got[1] != got[2] and [tuple(container.parse_banded(container.split_seal(f)[0]).padding) for f in got] == PADS


def test_one_band_per_channel_on_every_scale():
    x = images(1, 320, 88).cuda()
    for G, R, head in ((1, 1, False), (4, 2, True)):
        got = native(G, R, head, bands=1).encode_batch(x)
        _same_files(got, python(G, R, head, bands=1).encode_batch(x).to_bytes([(0, 0, 0, 0)]))
        seal = container.split_seal(got[0])[1]
        assert (seal.parity_group, seal.parity_groups) == (1, 1) and seal.band_crcs.shape == (3, 1)


@pytest.mark.parametrize('G,R,head', [(1, 2, True), (3, 4, True)])
def test_many_bands_on_every_scale(G, R, head):
    """bands = 440: L = 64 on every scale, n = 440 on the finest record -- more than 256 length fields in a file, and with G = 1 more than
    256 copy units: the seal's plan kernel gives a thread several of each, on the coder's own lengths and in the encoder's own slots."""
    bands = 440
    hws = [(320 >> s) * (88 >> s) for s in (3, 2, 1, 0)]
    ns = [container.n_bands(hw, container.band_len(hw, bands)) for hw in hws]
    assert [container.band_len(hw, bands) for hw in hws] == [64, 64, 64, 64] and ns == [7, 28, 110, 440]
    x = images(1, 320, 88).cuda()
    want = python(G, R, head, bands=bands).encode_batch(x).to_bytes([(0, 0, 0, 0)])
    scales = container.parse_banded(container.split_seal(want[0])[0]).scales
    assert [tuple(s) for s in scales] == [(5, 40, 11, 64), (5, 80, 22, 64), (5, 160, 44, 64), (3, 320, 88, 64)]
    fields = sum(C * n for (C, _, _, _), n in zip(scales, ns))
    units = 3 * -(-ns[3] // G) + 1 + sum(C * -(-n // G) for (C, _, _, _), n in zip(scales[:3], ns[:3]))
    assert fields == 2045 and fields > 256 and units == {1: 2046, 3: 692}[G] and units > 256
    codec = native(G, R, head, bands=bands)
    got = codec.encode_batch(x)
    _same_files(got, want)
    seal = container.split_seal(got[0])[1]
    assert (seal.parity_group, seal.parity_groups, seal.parity_streams) == (G, -(-440 // G), R) and seal.head is not None and not seal.head_damaged
    pixels, pads = codec.decode_batch(got)
    assert torch.equal(pixels, x) and [tuple(p) for p in pads] == [(0, 0, 0, 0)]


def test_the_encode_is_one_library_call_and_the_band_sealed_encode_is_unchanged(monkeypatch):
    x = images(1, 320, 88).cuda()
    codecs = [native(G, R, head) for G, R, head in CASES]
    plain = band_sealed_native(K, 'bands')
    for c in codecs + [plain]:
        c.model_id()                                            # (computed on first use: not part of an encode)
    calls = NamedCalls(monkeypatch)
    for c in codecs:
        calls.names = []
        files, file_bytes = c.encode_device(x)
        assert calls.names == ['l3c_encode_batch_banded_parity']
        assert files.is_cuda and file_bytes.is_cuda and tuple(files.shape) == (1, c.file_stride(320, 88))
    calls.names = []
    plain.encode_device(x)
    assert calls.names == ['l3c_encode_batch_banded', 'l3c_u8_crc32_bands', 'l3c_seal_append_bands']


def test_the_native_decoders_read_the_native_files():
    for G, R, head in ((4, 2, False), (4, 4, True)):
        x, files = native_files(G, R, head, 3)
        codec = native(G, R, head)
        pixels, pads = codec.decode_batch(files)
        assert torch.equal(pixels, x) and [tuple(p) for p in pads] == PADS
        pixels, pads, info = codec.decode_salvage(files)
        assert torch.equal(pixels, x) and info.concealed == {} and info.lost == [] and info.unverified == [] and info.line() == 'seal: ok'
        # ... and so does a codec that writes band-sealed files: a version-3 file reads as the band-sealed file it contains
        assert torch.equal(band_sealed_native(K, 'bands').decode_batch(files)[0], x)


def test_decode_repair_rebuilds_two_bands_of_one_group_of_a_native_file():
    x, files = native_files(4, 2, False)
    hit = damaged(files[0], streams=[(0, 3), (0, 7)])            # bands 3 and 7 of channel 0: both in group 3
    assert hit != files[0]
    with pytest.raises(container.SealError):
        native(4, 2, False).decode_batch([hit])
    got, pads, info = python(4, 2, False).decode_repair([hit])
    assert got.dtype == torch.uint8 and torch.equal(got, x) and info.repaired == {0: [(0, 3), (0, 7)]} and info.files[0] == files[0]


def test_decode_repair_heals_a_coarse_payload_of_a_native_head_file():
    x, files = native_files(4, 4, True)
    hit = hurt(files[0], payloads=[(1, 3, 5)])                  # the 80x22 record: channel 3, band 5
    assert hit != files[0]
    got, pads, info = python(4, 4, True).decode_repair([hit])
    assert torch.equal(got, x) and info.head[0].repaired == [(1, 3, 5)] and info.head[0].failed == [] and info.files[0] == files[0]


def test_encode_images_writes_bitcodings_files_of_the_padded_frames():
    """Two images of different sizes that pad to 320 x 88: gathered into frames on the device, then the one call."""
    from tests.test_gpu_native_images import _as, _chw
    shapes = [(317, 83), (320, 88)]
    imgs = [_chw(h, w, 40 + k) for k, (h, w) in enumerate(shapes)]
    pads = [pad.padding_for(h, w, 8) for h, w in shapes]
    x = torch.stack([torch.nn.functional.pad(im, p, 'constant', 0) for im, p in zip(imgs, pads)]).cuda()
    assert tuple(x.shape) == (2, 3, 320, 88) and pads[0] != (0, 0, 0, 0)
    for G, R, head in ((4, 2, False), (3, 2, True)):
        got = native(G, R, head).encode_images([_as('hwc', im) for im in imgs], layout='hwc')
        _same_files(got, python(G, R, head).encode_batch(x).to_bytes(pads))
