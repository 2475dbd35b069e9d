"""-m gpu: sealed `.l3c` files through both codec paths (Bitcoding(bp, seal=True), NativeCodec(bp, seal=True); include/l3c_hip.h
"sealed files": l3c_u8_crc32, l3c_seal_append, container.split_seal / make_seal).

On the calibrated 64x96 fixture and a 32x32 batch of 2, legacy and bands = 4: the body of a sealed file IS the unsealed file, the seal is
make_seal with zlib.crc32 of the padded frame and a model id hashed here, independently, in l3c_net_param order; both paths write the same
bytes and read each other's.  Then what a seal is for: a file of another generation or another checkpoint is refused before a single library
call, a damaged payload byte after the decode -- exactly when the pixels it decodes to are wrong."""
import hashlib
import struct
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from l3c_pytorch_amd.bitcoding.container import SealError  # noqa: E402
from tests.golden import make_hip_bitstream as gen  # noqa: E402
from tests.test_gpu_native_banded import _image, bitcoding, blueprint, codec  # noqa: E402

_SEALED = {}
CASES = [('fixture', 0), ('fixture', 4), ('batch', 0), ('batch', 4)]
PADS = {'fixture': [(3, 1, 0, 2)], 'batch': [(0, 0, 0, 0), (1, 2, 3, 4)]}


def sealed_codec(K):
    from l3c_pytorch_amd.native_codec import NativeCodec
    if ('n', K) not in _SEALED:
        _SEALED['n', K] = NativeCodec(blueprint(), bands=K, seal=True)
    return _SEALED['n', K]


def sealed_bitcoding(K):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    if ('b', K) not in _SEALED:
        _SEALED['b', K] = Bitcoding(blueprint(), bands=K, seal=True)
    return _SEALED['b', K]


def images(which):
    if which not in _SEALED:
        _SEALED[which] = gen.l3c_case().to(torch.uint8).cuda() if which == 'fixture' else _image(2, 32, 32, 5)
    return _SEALED[which]


def files(which, K):
    """(unsealed files of Bitcoding, sealed files of Bitcoding, sealed files of NativeCodec), computed once per case."""
    key = ('files', which, K)
    if key not in _SEALED:
        x, pads = images(which), PADS[which]
        _SEALED[key] = (bitcoding(K).encode_batch(x).to_bytes(pads), sealed_bitcoding(K).encode_batch(x).to_bytes(pads),
                        sealed_codec(K).encode_batch(x, pads))
    return _SEALED[key]


def model_id():
    """SHA-256 over the checkpoint's tensors in l3c_net_param order, hashed here and not by the package."""
    from l3c_pytorch_amd.native_net import param_schema
    sd = blueprint().net.state_dict()
    h = hashlib.sha256()
    for name, _ in param_schema(codec(0).cfg):
        h.update(sd[name].detach().cpu().float().contiguous().numpy().astype('<f4').tobytes())
    return int.from_bytes(h.digest()[:8], 'little') or 1


def generation():
    from l3c_pytorch_amd import _lib
    return _lib.load().l3c_bitstream_generation()


class Calls(object):
    """Counts every call into the library that goes through _lib.call (ops.call is the same function under another name)."""

    def __init__(self, monkeypatch):
        from l3c_pytorch_amd import _lib, native_net, ops
        self.n = 0
        real = _lib.call

        def counting(name, *args):
            self.n += 1
            return real(name, *args)
        for mod in (_lib, ops, native_net):
            monkeypatch.setattr(mod, 'call', counting)


@pytest.mark.parametrize('which,K', CASES)
def test_body_is_the_unsealed_file_and_the_seal_is_make_seal(which, K):
    plain, sealed, native = files(which, K)
    x = images(which).cpu().numpy()
    for b, (p, s) in enumerate(zip(plain, sealed)):
        assert container.is_sealed(s) and not container.is_sealed(p)
        assert s[:-24] == p
        want = container.make_seal(p, generation(), zlib.crc32(x[b].tobytes()), model_id())
        assert s[-24:] == want, (s[-24:].hex(), want.hex())
        body, seal = container.split_seal(s)
        assert body == p and seal == container.Seal(generation(), zlib.crc32(x[b].tobytes()), model_id())
    assert native == sealed                                           # byte for byte, seal included


@pytest.mark.parametrize('which,K', CASES)
def test_each_side_decodes_the_other_and_a_mixed_batch(which, K):
    plain, sealed, native = files(which, K)
    x = images(which)
    got, pads = bitcoding(K).decode_batch(native, out_dtype=torch.uint8)
    assert torch.equal(got, x) and [tuple(p) for p in pads] == PADS[which]
    got, pads = codec(K).decode_batch(sealed)
    assert torch.equal(got, x) and pads == PADS[which]
    mixed = [sealed[0]] + plain[1:] + plain[:1]                       # sealed and unsealed files of one shape in one call
    want = torch.cat([x, x[:1]])
    assert torch.equal(codec(K).decode_batch(mixed)[0], want)
    assert torch.equal(bitcoding(K).decode_batch(mixed, out_dtype=torch.uint8)[0], want)


@pytest.mark.parametrize('K', [0, 4])
def test_encode_images_and_decode_images_with_sealed_files(K):
    rng = np.random.RandomState(11 + K)
    pics = [np.ascontiguousarray(images('fixture')[0, :, :61, :90].permute(1, 2, 0).cpu().numpy()),
            np.ascontiguousarray(images('fixture')[0].permute(1, 2, 0).cpu().numpy())]
    pics[0][::7, ::5] = rng.randint(0, 256, pics[0][::7, ::5].shape)
    sealed = sealed_codec(K).encode_images(pics, layout='hwc')
    plain = codec(K).encode_images(pics, layout='hwc')
    assert all(container.is_sealed(s) and s[:-24] == p for s, p in zip(sealed, plain))
    frames = [np.pad(p.transpose(2, 0, 1), ((0, 0), (1, 2), (3, 3)), 'constant') if p.shape[0] == 61 else p.transpose(2, 0, 1) for p in pics]
    for s, f in zip(sealed, frames):
        assert f.shape == (3, 64, 96) and container.split_seal(s)[1].frame_crc == zlib.crc32(np.ascontiguousarray(f).tobytes())
    for c in (sealed_codec(K), codec(K)):
        back = c.decode_images(sealed, layout='hwc')
        assert all(np.array_equal(b.cpu().numpy(), p) for b, p in zip(back, pics))
    back = codec(K).decode_images([sealed[1], plain[0]], layout='hwc')            # sealed and unsealed in one call
    assert np.array_equal(back[0].cpu().numpy(), pics[1]) and np.array_equal(back[1].cpu().numpy(), pics[0])


def _regenerated(f, generation_):
    """The sealed file with its seal rewritten to another generation (check word made valid again)."""
    body, seal = container.split_seal(f)
    return body + container.make_seal(body, generation_, seal.frame_crc, seal.model_id)


@pytest.mark.parametrize('K', [0, 4])
def test_another_generation_is_refused_before_any_library_call(K, monkeypatch):
    old = _regenerated(files('batch', K)[1][1], 2)
    good = files('batch', K)[1][0]
    for dec in (lambda fs: codec(K).decode_batch(fs), lambda fs: bitcoding(K).decode_batch(fs), lambda fs: codec(K).decode_images(fs)):
        calls = Calls(monkeypatch)
        with pytest.raises(SealError) as e:
            dec([good, old])
        assert e.value.reason == 'generation' and e.value.index == 1 and calls.n == 0
        monkeypatch.undo()
        calls = Calls(monkeypatch)                                    # the counter does see a decode that runs
        dec([good])
        assert calls.n > 0
        monkeypatch.undo()


@pytest.mark.parametrize('K', [0, 4])
def test_another_checkpoint_is_refused_before_any_library_call(K, monkeypatch):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    from l3c_pytorch_amd.native_codec import NativeCodec
    if 'other' not in _SEALED:
        cfg = config_parser.parse_builtin('ms', 'cr')
        bp = gen.blueprint('cr', False)
        bp.net.load_state_dict(synthetic.make_state_dict(cfg, 1), strict=True)
        _SEALED['other'] = bp
    bp = _SEALED['other']
    others = (NativeCodec(bp), Bitcoding(bp))
    assert others[0].model_id() == others[1].model_id() != model_id()
    sealed = files('batch', K)[1]
    for other in others:
        calls = Calls(monkeypatch)
        with pytest.raises(SealError) as e:
            other.decode_batch(sealed)
        assert e.value.reason == 'model' and e.value.index == 0 and calls.n == 0
        monkeypatch.undo()
    # a seal that does not state its model is not refused up front: the pixels decide
    body, seal = container.split_seal(sealed[0])
    unstated = body + container.make_seal(body, seal.generation, seal.frame_crc, 0)
    assert torch.equal(codec(K).decode_batch([unstated])[0], images('batch')[:1])


def _flip_in_r_stream(f, K):
    """One payload byte in the middle of the R stream (bands: of its first band) of the RGB record flipped; never a length field."""
    body, seal = container.split_seal(f)
    if K:
        p = container.parse_banded(body)
        at, n = int(p.offset[-1][0, 0]), int(p.nbytes[-1][0, 0])
    else:
        p = container.parse_containers([body])
        at, n = int(p.offset[-1][0, 0]), int(p.nbytes[-1][0, 0])
    assert n > 8
    pos = at + n // 2
    assert struct.unpack_from('<I', body, at - 4)[0] == n
    damaged = body[:pos] + bytes([body[pos] ^ 0x10]) + body[pos + 1:]
    return damaged, damaged + f[-24:]


@pytest.mark.parametrize('which,K', CASES)
def test_a_damaged_payload_byte_raises_exactly_when_the_pixels_are_wrong(which, K):
    sealed = files(which, K)[1]
    x = images(which)[:1]
    body, damaged = _flip_in_r_stream(sealed[0], K)
    plain_pixels = codec(K).decode_batch([body])[0]                   # the damaged body, unsealed: decodes safely to SOME pixels
    wrong = not torch.equal(plain_pixels, x)
    for dec in (lambda fs, **kw: codec(K).decode_batch(fs, **kw)[0], lambda fs, **kw: bitcoding(K).decode_batch(fs, out_dtype=torch.uint8, **kw)[0]):
        if wrong:
            with pytest.raises(SealError) as e:
                dec([damaged])
            assert e.value.reason == 'pixels' and e.value.index == 0
        else:
            assert torch.equal(dec([damaged]), x)
        assert torch.equal(dec([damaged], verify=False), plain_pixels)      # verify=False: the damaged pixels, no error
    if wrong:
        with pytest.raises(SealError) as e:
            codec(K).decode_images([sealed[0], damaged] if which == 'fixture' else [damaged])
        assert e.value.reason == 'pixels' and e.value.index == (1 if which == 'fixture' else 0)


def test_the_set_readers_refuse_a_sealed_file():
    from l3c_pytorch_amd.helpers import dataset_codec
    sealed = files('batch', 0)[1]
    with pytest.raises(ValueError, match='sealed.*split_seal'):
        bitcoding(0).decode_many([sealed])
    with pytest.raises(ValueError, match='sealed.*split_seal'):
        dataset_codec.decode_set(bitcoding(0), dict(enumerate(sealed)), [0, 1])
    with pytest.raises(ValueError, match='sealed.*split_seal'):
        bitcoding(4).decode_many([files('batch', 4)[1]], banded=True)


def test_preview_strips_the_seal_and_the_packed_buffer_refuses_it():
    plain, sealed, _ = files('batch', 0)
    a, _ = bitcoding(0).decode_preview(sealed)
    b, _ = bitcoding(0).decode_preview(plain)
    assert torch.equal(a, b)
    enc = sealed_bitcoding(0).encode_batch(images('batch'))
    with pytest.raises(ValueError, match='seal'):
        enc.to_host_buffer()
    assert enc.to_bytes_host_assembled(PADS['batch']) == sealed


def test_seal_append_alone_marks_a_slot_without_room():
    """l3c_seal_append on hand-made slots: a file that leaves 24 bytes gets them, -1 stays -1, a slot without room becomes -1, and nothing
    outside a slot is stored."""
    from l3c_pytorch_amd import ops
    stride, B = 64, 4
    slots = torch.full((B * stride + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    sizes = torch.tensor([40, -1, 41, 12], dtype=torch.int64, device='cuda')
    crc = torch.tensor([0x01020304, 5, 6, -2], dtype=torch.int32, device='cuda')
    pads = torch.tensor([[1, 2, 3, 4]] * B, dtype=torch.int16, device='cuda')
    ops.seal_append(slots[:B * stride].view(B, stride), sizes, crc, pads, 0x1122334455667788)
    got, n = slots.cpu().numpy(), sizes.cpu().tolist()
    assert n == [64, -1, -1, 36]
    pad8 = struct.pack('<4H', 1, 2, 3, 4)
    for b, (at, word) in {0: (40, 0x01020304), 3: (12, 0xfffffffe)}.items():
        want = container.make_seal(pad8 + b'\0' * 8, generation(), word, 0x1122334455667788)
        assert got[b * stride + at:b * stride + at + 24].tobytes() == want
        got[b * stride + at:b * stride + at + 24] = 0xA5
    assert (got == 0xA5).all()


def test_file_api_writes_sealed_files_and_parts_and_verifies_them(tmp_path, monkeypatch):
    """Bitcoding.encode(img, pout) with seal=True: the file, and every .partN file of an auto-cropped image, is sealed; decode verifies each."""
    import os
    from l3c_pytorch_amd import auto_crop
    from l3c_pytorch_amd.helpers import synthetic
    img = synthetic.make_image(70, 90, 8, 'natural').long().unsqueeze(0)
    bc = sealed_bitcoding(0)
    whole = str(tmp_path / 'y.l3c')
    bc.encode(img, whole)
    data = open(whole, 'rb').read()
    body, seal = container.split_seal(data)
    assert seal == container.Seal(generation(), seal.frame_crc, model_id()) and container.padded_shape(body) == (72, 96)
    assert torch.equal(bitcoding(0).decode(whole).cpu(), img)
    monkeypatch.setattr(auto_crop, '_NEEDS_CROP_DIM', 40 * 40)
    p = str(tmp_path / 'x.l3c')
    bc.encode(img, p)
    parts = sorted(f for f in os.listdir(tmp_path) if f.startswith('x.l3c.part'))
    assert len(parts) == 4 and all(container.is_sealed(open(str(tmp_path / f), 'rb').read()) for f in parts)
    assert torch.equal(bitcoding(0).decode(p + '.part0').cpu(), img)
    # part 2 from another generation: the stitched decode refuses, verify=False goes through
    path = str(tmp_path / parts[2])
    with open(path, 'rb') as f:
        old = _regenerated(f.read(), 2)
    with open(path, 'wb') as f:
        f.write(old)
    with pytest.raises(SealError) as e:
        bitcoding(0).decode(p + '.part0')
    assert e.value.reason == 'generation'
    assert torch.equal(bitcoding(0).decode(p + '.part0', verify=False).cpu(), img)


def test_l3c_cli_seals_and_verifies(synthetic_l3c, tmp_path, capsys):
    """`l3c.py ... enc --seal` writes a sealed file and says so; `dec` prints `seal: ok (generation G)`, refuses a damaged file with a
    DecodeError line and status 1, and decodes it with --no-verify."""
    import importlib.util
    import os
    from PIL import Image
    from l3c_pytorch_amd.helpers import synthetic
    cfg, sd = synthetic_l3c
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = tmp_path / 'logs' / '0306_0001 cr oi' / 'ckpts'
    exp.mkdir(parents=True)
    torch.save({'net': sd}, str(exp / 'ckpt_0000000001.pt'))
    img = synthetic.make_image(45, 70, 21, 'natural')
    src, out, png = str(tmp_path / 'in.png'), str(tmp_path / 'out.l3c'), str(tmp_path / 'dec.png')
    Image.fromarray(img.permute(1, 2, 0).numpy()).save(src)
    spec = importlib.util.spec_from_file_location('l3c_cli', os.path.join(root, 'l3c.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    args = [str(tmp_path / 'logs'), '0306_0001']
    assert cli.main(args + ['enc', '--seal', src, out]) == 0
    assert 'bitstream generation {}'.format(generation()) in capsys.readouterr().out
    data = open(out, 'rb').read()
    body, seal = container.split_seal(data)
    assert seal is not None and seal.generation == generation() and seal.model_id not in (0, model_id())
    assert cli.main(args + ['dec', out, png]) == 0
    assert 'seal: ok (generation {})'.format(generation()) in capsys.readouterr().out
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1), img)
    with open(out, 'wb') as f:
        f.write(_regenerated(data, 2))
    assert cli.main(args + ['dec', out, png]) == 1
    assert 'DecodeError: seal:' in capsys.readouterr().out
    assert cli.main(args + ['dec', '--no-verify', out, png]) == 0
    assert 'seal: ok' not in capsys.readouterr().out
