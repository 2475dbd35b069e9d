"""-m gpu: sealed files through the set readers (Bitcoding.decode_many / SetDecoder, dataset_codec.decode_set and verify_set with
sealed=True; INTEGRATION.md "Sealed files").

Twelve images of six shapes -- one pixel block, two that need padding, one shape twice -- written by encode_set with Bitcoding(seal=True),
legacy and bands = 4.  The set decode returns every image; the CRC word the device computed of every frame is zlib.crc32 of the padded frame
and the seal's; a file of another generation or checkpoint is refused before a single library call, under the caller's key; one flipped
payload byte in file 7 is SealError('pixels') for exactly that file in all three forms of decode_many, and 'pixels' in verify_set's report,
while the same body without its seal decodes to some pixels without a word -- which is what the seal is for.

The damaged byte is the middle byte of file 7's R stream (the method of tests/test_gpu_sealed_codec._flip_in_r_stream).  A flipped payload
byte does not always change a pixel, and a seal rightly passes a file whose pixels are right: [measured on an MI355X] of 84 single-byte
flips at 2 .. 99 % of the RGB streams of four files of this set, 6 changed no pixel, the middle byte of the R stream of the 9x17 image drawn
with seed 77 among them, while the same byte of the one drawn with seed 71 changes 202 of its 384 R pixels.  File 7 therefore holds the
image of seed 71 (_SEEDS), and the test that strips the seal asserts that the damaged body does decode to other pixels."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from l3c_pytorch_amd.bitcoding.container import SealError  # noqa: E402

SHAPES = [(8, 8), (9, 17), (64, 96), (72, 88), (24, 40), (64, 96)] * 2
ORDER = list(range(len(SHAPES)))
_SEEDS = [70 + (i + 6) % 12 for i in ORDER]      # file 7: seed 71 (see above)
_CACHE = {}


def _bc(l3c_checkpoint, bands=0, seal=False):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    if 'bp' not in _CACHE:
        cfg, sd = l3c_checkpoint(True)
        bp = MultiscaleBlueprint(cfg)
        bp.net.load_state_dict(sd, strict=True)
        bp.set_eval()
        _CACHE['bp'] = bp
    if ('bc', bands, seal) not in _CACHE:
        _CACHE['bc', bands, seal] = Bitcoding(_CACHE['bp'], bands=bands, seal=seal)
    return _CACHE['bc', bands, seal]


def _images():
    from l3c_pytorch_amd.helpers import synthetic
    if 'imgs' not in _CACHE:
        _CACHE['imgs'] = {i: synthetic.make_image(h, w, _SEEDS[i], 'natural') for i, (h, w) in enumerate(SHAPES)}
    return _CACHE['imgs']


def _files(l3c_checkpoint, bands=0):
    """{index: sealed file} of the twelve images, written once per format."""
    from l3c_pytorch_amd.helpers import dataset_codec
    if ('files', bands) not in _CACHE:
        files, _, _ = dataset_codec.encode_set(_bc(l3c_checkpoint, bands, True), _images(), ORDER, max_batch=16)
        assert all(container.is_sealed(files[i]) for i in ORDER)
        _CACHE['files', bands] = files
    return _CACHE['files', bands]


def _frame(i):
    """The padded planar frame of image i as bytes."""
    from l3c_pytorch_amd.helpers import pad
    x, _ = pad.pad(_images()[i].unsqueeze(0), 8, mode='constant')
    return np.ascontiguousarray(x[0].numpy().astype(np.uint8)).tobytes()


def _damaged(l3c_checkpoint):
    """(the files with one payload byte of file 7's finest record flipped, that file's damaged body without its seal)."""
    from tests.test_gpu_sealed_codec import _flip_in_r_stream
    files = dict(_files(l3c_checkpoint))
    body, files[7] = _flip_in_r_stream(files[7], 0)
    return files, body


def _batches(files):
    """decode_many's batches for the set, as decode_set plans them -> (batches, the caller's key of every (entry, file))."""
    from l3c_pytorch_amd.helpers import dataset_codec
    chunks, _ = dataset_codec.plan_decode_set(files, ORDER, 16)
    assert len(chunks) == 5 and sorted(len(c) for c in chunks) == [2, 2, 2, 2, 4]
    return [[files[i] for i in c] for c in chunks], {(n, k): i for n, c in enumerate(chunks) for k, i in enumerate(c)}


def _assert_images(back):
    imgs = _images()
    assert sorted(back) == ORDER
    for i in ORDER:
        assert torch.equal(back[i].cpu(), imgs[i]), i


def test_round_trip_of_a_sealed_set(l3c_checkpoint):
    from l3c_pytorch_amd.helpers import dataset_codec
    bc = _bc(l3c_checkpoint)
    _assert_images(dataset_codec.decode_set(bc, _files(l3c_checkpoint), ORDER, sealed=True))


def test_round_trip_of_a_sealed_banded_set(l3c_checkpoint):
    from l3c_pytorch_amd.helpers import dataset_codec
    files = _files(l3c_checkpoint, 4)
    assert all(container.is_banded(files[i]) for i in ORDER)
    _assert_images(dataset_codec.decode_set(_bc(l3c_checkpoint, 4), files, ORDER, sealed=True, banded=True))


def _mixed(l3c_checkpoint):
    files = _files(l3c_checkpoint)
    return {i: files[i] if i % 3 else files[i][:-container.SEAL_BYTES] for i in ORDER}


def test_round_trip_of_sealed_and_unsealed_files_in_one_set(l3c_checkpoint):
    from l3c_pytorch_amd.helpers import dataset_codec
    mixed = _mixed(l3c_checkpoint)
    assert sum(container.is_sealed(mixed[i]) for i in ORDER) == 8
    _assert_images(dataset_codec.decode_set(_bc(l3c_checkpoint), mixed, ORDER, sealed=True))


def test_the_device_words_are_zlib_of_the_padded_frame_and_the_seals(l3c_checkpoint):
    from l3c_pytorch_amd.helpers import dataset_codec
    for bands in (0, 4):
        files, info = _files(l3c_checkpoint, bands), {}
        status = dataset_codec.verify_set(_bc(l3c_checkpoint, bands), files, ORDER, banded=bool(bands), info=info)
        assert status == {i: 'ok' for i in ORDER}
        assert sorted(info['frame_crc']) == ORDER
        for i in ORDER:
            want = zlib.crc32(_frame(i))
            assert info['frame_crc'][i] == want == container.split_seal(files[i])[1].frame_crc, (bands, i, hex(info['frame_crc'][i]), hex(want))


def _forms(bc, batches):
    """The three forms of decode_many(sealed=True): ragged groups, two lanes without ragged groups, one lane."""
    return [('ragged', lambda: bc.decode_many(batches, out_dtype=torch.uint8, sealed=True)),
            ('two lanes', lambda: bc.decode_many(batches, out_dtype=torch.uint8, sealed=True, ragged=False, lanes=2)),
            ('one lane', lambda: bc.decode_many(batches, out_dtype=torch.uint8, sealed=True, lanes=1))]


def test_all_three_forms_of_decode_many_return_the_same_pixels(l3c_checkpoint):
    from l3c_pytorch_amd.helpers import pad
    bc = _bc(l3c_checkpoint)
    batches, key = _batches(_files(l3c_checkpoint))
    results = []
    for name, run in _forms(bc, batches):
        out = run()
        torch.cuda.synchronize()
        results.append(out)
        for n, (pixels, paddings) in enumerate(out):
            assert pixels.dtype == torch.uint8
            for k in range(pixels.shape[0]):
                img = pad.undo_pad(pixels[k:k + 1], *paddings[k])[0] if any(paddings[k]) else pixels[k]
                assert torch.equal(img.cpu(), _images()[key[n, k]]), (name, n, k)
    for other in results[1:]:
        for (a, pa), (b, pb) in zip(results[0], other):
            assert torch.equal(a, b) and [tuple(p) for p in pa] == [tuple(p) for p in pb]
    # the default dtype: the sealed path hashes uint8 pixels and still returns what it was asked for
    out = bc.decode_many(batches, sealed=True)
    assert all(p.dtype == torch.int64 and torch.equal(p, q.long()) for (p, _), (q, _) in zip(out, results[0]))


def test_all_three_forms_raise_the_same_error_for_a_damaged_file(l3c_checkpoint):
    bc = _bc(l3c_checkpoint)
    files, _ = _damaged(l3c_checkpoint)
    batches, key = _batches(files)
    where = [w for w, i in key.items() if i == 7]
    for name, run in _forms(bc, batches):
        with pytest.raises(SealError) as e:
            run()
        assert e.value.reason == 'pixels' and e.value.index == where[0] and e.value.failed == where, (name, e.value.index, e.value.failed)
    got = []
    with pytest.raises(SealError):                       # on_batch is handed the pixels before the call has verified them; it still raises
        bc.decode_many(batches, on_batch=lambda n, pixels, paddings: got.append(n), out_dtype=torch.uint8, sealed=True)
    assert sorted(got) == list(range(len(batches)))


def _resealed(f, generation=None, model_id=None):
    body, seal = container.split_seal(f)
    return body + container.make_seal(body, seal.generation if generation is None else generation, seal.frame_crc,
                                      seal.model_id if model_id is None else model_id)


@pytest.mark.parametrize('reason', ['generation', 'model'])
def test_another_generation_or_checkpoint_is_refused_before_any_library_call(l3c_checkpoint, reason, monkeypatch):
    from l3c_pytorch_amd.helpers import dataset_codec
    from tests.test_gpu_sealed_codec import Calls
    bc = _bc(l3c_checkpoint)
    files = dict(_files(l3c_checkpoint))
    seal = container.split_seal(files[4])[1]
    assert seal.generation == bc.generation() and seal.model_id == bc.model_id() != 0
    files[4] = _resealed(files[4], generation=seal.generation - 1) if reason == 'generation' else _resealed(files[4], model_id=seal.model_id ^ 1)
    batches, key = _batches(files)
    calls = Calls(monkeypatch)
    with pytest.raises(SealError) as e:
        dataset_codec.decode_set(bc, files, ORDER, sealed=True)
    assert e.value.reason == reason and e.value.index == 4 and e.value.failed == [4] and calls.n == 0
    with pytest.raises(SealError) as e:
        bc.decode_many(batches, sealed=True)
    assert e.value.reason == reason and key[e.value.index] == 4 and calls.n == 0
    status = dataset_codec.verify_set(bc, {4: files[4]}, [4])                  # reported from the seal alone: nothing is decoded
    assert status == {4: reason} and calls.n == 0
    monkeypatch.undo()
    calls = Calls(monkeypatch)                                                  # the counter does see a decode that runs
    assert dataset_codec.verify_set(bc, files, ORDER) == {i: reason if i == 4 else 'ok' for i in ORDER}
    assert calls.n > 0


def test_one_damaged_payload_byte_is_found_in_the_set(l3c_checkpoint):
    from l3c_pytorch_amd.helpers import dataset_codec
    bc = _bc(l3c_checkpoint)
    files, body = _damaged(l3c_checkpoint)
    with pytest.raises(SealError) as e:
        dataset_codec.decode_set(bc, files, ORDER, sealed=True)
    assert e.value.reason == 'pixels' and e.value.index == 7 and e.value.failed == [7]
    info = {}
    assert dataset_codec.verify_set(bc, files, ORDER, info=info) == {i: 'pixels' if i == 7 else 'ok' for i in ORDER}
    assert info['frame_crc'][7] != zlib.crc32(_frame(7)) and info['frame_crc'][6] == zlib.crc32(_frame(6))
    # what the seal is for: the same body without it decodes to SOME pixels of the right size, and nobody says a word
    stripped = {i: files[i][:-container.SEAL_BYTES] for i in ORDER}
    stripped[7] = body
    back = dataset_codec.decode_set(bc, stripped, ORDER)
    assert back[7].shape == _images()[7].shape and not torch.equal(back[7], _images()[7])
    for i in ORDER:
        assert i == 7 or torch.equal(back[i], _images()[i]), i


def test_verify_set_reports_unsealed_files(l3c_checkpoint):
    from l3c_pytorch_amd.helpers import dataset_codec
    mixed = _mixed(l3c_checkpoint)
    assert dataset_codec.verify_set(_bc(l3c_checkpoint), mixed, ORDER) == {i: 'ok' if i % 3 else 'unsealed' for i in ORDER}


def test_without_sealed_the_set_readers_still_refuse_a_sealed_file(l3c_checkpoint):
    from l3c_pytorch_amd.helpers import dataset_codec
    bc = _bc(l3c_checkpoint)
    files = _files(l3c_checkpoint)
    batches, _ = _batches(files)
    with pytest.raises(ValueError, match='sealed.*split_seal') as e:
        dataset_codec.decode_set(bc, files, ORDER)
    assert not isinstance(e.value, SealError)
    with pytest.raises(ValueError, match='sealed.*split_seal'):
        bc.decode_many(batches)
    with pytest.raises(ValueError, match='sealed.*split_seal'):
        bc.decode_many(batches, sealed=False, lanes=1)
