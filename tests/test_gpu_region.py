"""-m gpu: region decode -- rows of a banded `.l3c` file without decoding the rest (Bitcoding.decode_region, MultiscaleNetwork.get_P_rows,
bitcoding/region.py).  First the measurement everything rests on: P of a row window equals the full frame's P BIT FOR BIT on the window's
valid rows.  Then the round trip over boxes, batches and band counts, a file whose unneeded bands are destroyed, a legacy file, a sealed
file, the refusals, and the CLI.

Frames are 320x88 (five 64-row granules) and 328x88 (a last granule of 8 rows); the 320x88 frame of the round trips is a 317x83 image,
centre-padded.  At K = 16 a band is 1792 symbols (20.4 rows), at K = 64 it is 448 (5.1 rows, 63 bands).  One image is fewer than 16 entries
(lag 1) for every box but the all-rows one; a batch of three at K = 64 is 16 entries and more (lag 2, the side stream) from 26 rows on."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd.bitcoding import container, region  # noqa: E402
from l3c_pytorch_amd.bitcoding.container import SealError  # noqa: E402
from l3c_pytorch_amd.helpers import pad, synthetic  # noqa: E402
from tests.conftest import GOLDEN  # noqa: E402
from tests.golden import make_hip_bitstream as gen  # noqa: E402

HALO = 40
_CACHE = {}


def blueprint(name='cr'):
    if ('bp', name) not in _CACHE:
        _CACHE['bp', name] = gen.blueprint(name, True)
    return _CACHE['bp', name]


def bitcoding(K, seal=False):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    if ('bc', K, seal) not in _CACHE:
        _CACHE['bc', K, seal] = Bitcoding(blueprint(), bands=K, seal=seal)
    return _CACHE['bc', K, seal]


def images(B, H, W):
    """B different uint8 images (B, 3, H, W) on the host."""
    if ('img', B, H, W) not in _CACHE:
        _CACHE['img', B, H, W] = torch.stack([synthetic.make_image(H, W, 30 + 7 * b + H, 'natural') for b in range(B)])
    return _CACHE['img', B, H, W]


def encoded(K, B, H, W, seal=False):
    """(images (B, 3, H, W) uint8 on the GPU, their files, the padding tuple), encoded once per case and shared."""
    key = ('files', K, B, H, W, seal)
    if key not in _CACHE:
        x = images(B, H, W)
        fac = bitcoding(K).padding_factor()
        padding = (0, 0, 0, 0)
        frames = x
        if H % fac or W % fac:
            frames, padding = pad.pad(x.long(), fac=fac, mode=blueprint().get_padding_mode())
        files = bitcoding(K, seal).encode_batch(frames.cuda()).to_bytes([padding] * B)
        _CACHE[key] = (x.cuda(), files, tuple(padding))
    return _CACHE[key]


def crop(x, box):
    y0, y1 = box[:2]
    x0, x1 = box[2:] if len(box) == 4 else (0, x.shape[-1])
    return x[:, :, y0:y1, x0:x1]


# ---- 1. P bits ---------------------------------------------------------------------------------------------------------------------


def _layers(net, bn, fuse, rows=None):
    """The schedule of _decoder + _prob of scale 0, layer by layer -> [(name, output rows per half-resolution row, first half-resolution
    row of the output relative to the input's, output)].  rows: the classifier runs on these full-resolution rows of the decoder's output."""
    from l3c_pytorch_amd import ops
    pk = net._prepare()
    d, pr = pk['dec'][0], pk['prob'][0]
    x = ops.dec_head(bn, d['head'][0], d['head'][1], fuse)
    outs = [('dec_head', 1, 0, x)]
    skip = x
    for i, (c1, c2) in enumerate(d['blocks']):
        t = ops.conv(x, c1, relu=True)
        outs.append(('block {} conv 1'.format(i), 1, 0, t))
        x = ops.conv(t, c2, residual=x)
        outs.append(('block {} conv 2'.format(i), 1, 0, x))
    x = ops.conv(x, d['tail'], residual=skip)
    outs.append(('body tail', 1, 0, x))
    F = ops.conv(x, d['up'], pixel_shuffle=True)
    outs.append(('up + pixel shuffle', 2, 0, F))
    first = 0
    if rows is not None:
        F, first = F[:, rows[0]:rows[1]].contiguous(), rows[0]
    B, H, W, Cf = F.shape
    cat = torch.empty(B, H, W, 3 * Cf, dtype=torch.float32, device=F.device)
    for i, a in enumerate(pr['atrous']):
        ops.conv(F, a, out=cat, out_coff=i * Cf)
        outs.append(('atrous {}'.format(a.dilation), 2, first, cat[..., i * Cf:(i + 1) * Cf].clone()))
    outs.append(('lin', 2, first, ops.conv(cat, pr['lin'])))
    return outs


def _first_differing_layer(net, bn_q, F_prev_nhwc, conv_rows, valid_rows, dec_rows):
    """Which layer's output first differs between a windowed schedule -- decoder on dec_rows, classifier on conv_rows -- and the frame's, on
    the rows that are valid at the END (they are valid in every layer before): both run layer by layer in this process."""
    (c0, c1), (v0, v1), (a0, a1) = conv_rows, valid_rows, dec_rows
    full = _layers(net, bn_q.contiguous(), F_prev_nhwc.contiguous())
    win = _layers(net, bn_q[:, :, a0 // 2:a1 // 2].contiguous(), F_prev_nhwc[:, a0 // 2:a1 // 2].contiguous(), (c0 - a0, c1 - a0))
    for (name, r, _, a), (_, _, first, b) in zip(full, win):
        a = a[:, v0 * r // 2:v1 * r // 2]
        lo = (v0 - a0) * r // 2 - first
        b = b[:, lo:lo + (v1 - v0) * r // 2]
        if not torch.equal(a, b):
            return '{}: {} of {} values differ, max |diff| {:.3e}'.format(name, int((a != b).sum()), a.numel(), float((a - b).abs().max()))
    return None


# (H, conv rows): the issue's frames -- an interior window with both edges cut, the image top, the image bottom (of 328 rows: a last granule
# of 8); their decoder stage is the whole frame (an apron of 192 rows).  712 rows: the decoder stage is cut too -- on both sides (64, 576),
# at the top only (256, 712 = the frame's end), and for a window that ends with the frame's last, short granule.
P_CASES = [(320, [(128, 256), (0, 128), (192, 320)]), (328, [(192, 328), (128, 256), (0, 128)]), (712, [(256, 384), (448, 576), (640, 712)])]


@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('H,windows', P_CASES)
def test_window_P_is_the_frames_P_bit_for_bit(H, windows, B):
    """One forward pass; get_P_rows on z1 and F1 of that pass against the pass's own P[0], torch.equal on the valid rows.

    MEASURED on an MI355X with the schedule the issue proposed -- decoder AND classifier on the conv rows alone, a halo of 40 rows: the
    valid rows are NOT the frame's.  320x88, conv rows (128, 256): the first layer whose kept rows differ is 'block 5 conv 1', the eleventh
    3x3 layer, 1958 of 67584 values, max |diff| 6.0e-07 -- last bits, from the rounding of Winograd tiles whose six input rows reach into
    the rows a cut edge changed (region.apron_rows).  get_P_rows therefore runs the decoder stage on the apron; the naive schedule's first
    differing layer is printed below for every cut window, and nothing is asserted about it."""
    net = blueprint().net
    W = 88
    out = net(images(B, H, W).float().cuda())
    P_full, bn_q, F1 = out.raw.P[0], out.raw.bn_q[1], out.raw.F_dec[1]
    assert tuple(P_full.shape[:3]) == (B, H, W) and tuple(F1.shape[:3]) == (B, H // 2, W // 2)
    apron = region.apron_rows(net.config_ms)
    assert apron == 192 and region.halo_rows(net.config_ms) == HALO
    for c0, c1 in windows:
        v0, v1 = (0 if c0 == 0 else c0 + HALO), (H if c1 == H else c1 - HALO)
        P = net.get_P_rows(0, bn_q, F1.permute(0, 3, 1, 2), (c0, c1))
        assert tuple(P.shape) == (B, c1 - c0, W, P_full.shape[3]) and P.is_contiguous()
        same = torch.equal(P[:, v0 - c0:v1 - c0], P_full[:, v0:v1])
        assert same, ((c0, c1), _first_differing_layer(net, bn_q, F1, (c0, c1), (v0, v1), region.decoder_rows(H, (c0, c1), apron)))
        if c0:      # ... and the halo is needed: the cut edge's rows are not the frame's
            assert not torch.equal(P[:, :HALO], P_full[:, c0:c0 + HALO])
        print('H={} B={} conv rows {}: decoder rows {}; decoder on the conv rows alone: {}'.format(
            H, B, (c0, c1), region.decoder_rows(H, (c0, c1), apron),
            _first_differing_layer(net, bn_q, F1, (c0, c1), (v0, v1), (c0, c1)) or 'no layer differs'))


def test_get_P_rows_refusals():
    net = blueprint().net
    out = net(images(1, 320, 88).float().cuda())
    bn_q, F1 = out.raw.bn_q[1], out.raw.F_dec[1].permute(0, 3, 1, 2)
    with pytest.raises(NotImplementedError):
        net.get_P_rows(1, out.raw.bn_q[2], out.raw.F_dec[2].permute(0, 3, 1, 2), (0, 64))
    for rows in ((0, 322), (64, 64), (1, 65), (-64, 64)):
        with pytest.raises(ValueError):
            net.get_P_rows(0, bn_q, F1, rows)
    with pytest.raises(ValueError):
        net.get_P_rows(0, bn_q, None, (0, 64))
    with pytest.raises(NotImplementedError):
        blueprint('cr_rgb_shared').net.get_P_rows(0, bn_q, None, (0, 64))


def test_full_size_dispatch_is_checked():
    """A frame whose scale-0 tensors pass 2 GB per image leaves the Winograd kernel: the windowed step refuses it (host arithmetic only)."""
    net = blueprint().net
    pk = net._prepare()
    net._check_rows_dispatch(2048, 3072, pk)
    net._check_rows_dispatch(2896, 2896, pk)                  # 2896^2 x 64 x 4 bytes: just below
    with pytest.raises(NotImplementedError):
        net._check_rows_dispatch(2904, 2896, pk)              # ... and just above 0x7ffffff0
    with pytest.raises(NotImplementedError):
        net._check_rows_dispatch(65528, 65528, pk)


# ---- 2. round trip -----------------------------------------------------------------------------------------------------------------


def boxes(H, W):
    return [(180, 200), (0, 30), (H - 30, H), (101, 102), (57, 58, 41, 42), (0, H), (150, 190, 10, 60), (H - 1, H, W - 1, W)]


@pytest.mark.parametrize('K,B', [(16, 1), (64, 1), (64, 3)])
@pytest.mark.parametrize('H,W', [(317, 83), (328, 88)])
def test_round_trip(H, W, K, B):
    """(Frames this small lie inside every box's apron: their decoder stage is the whole frame; test_round_trip_tall cuts it.)"""
    x, files, padding = encoded(K, B, H, W)
    bc = bitcoding(K)
    whole, pads = bc.decode_batch(files, out_dtype=torch.uint8)
    assert [tuple(p) for p in pads] == [padding] * B
    whole = pad.undo_pad(whole, *padding) if any(padding) else whole
    assert torch.equal(whole, x)
    lags = set()
    for box in boxes(H, W):
        got, info = bc.decode_region(files, box)
        assert got.dtype == torch.uint8 and torch.equal(got, crop(x, box)), (box, info)
        assert torch.equal(got, crop(whole, box)), (box, info)
        top = padding[2]
        assert info.sym_rows[0] <= top + box[0] and info.sym_rows[1] == top + box[1] and info.frame_rows == whole.shape[2] + padding[2] + padding[3]
        assert info.valid_rows[0] <= info.sym_rows[0] and info.sym_rows[1] <= info.valid_rows[1]
        assert info.streams_used == 3 * B * (info.bands[1] - info.bands[0]) and info.streams_total == 3 * B * info.n_bands
        assert not info.pixel_crc_checked and info.verified == () and info.sealed == 0
        lags.add(bc._rgb_schedule(B * (info.bands[1] - info.bands[0]), None)[0])
    assert lags == {1, 2}                                     # (lag 2: the all-rows box; with three images the 40-row box too)
    n_small = 3 * -(-40 * 88 // (1792 if K == 16 else 448))   # entries of a 40-row box of three images, at the least
    assert (n_small >= 16) == (K == 64)
    got, _ = bc.decode_region(files, (180, 200), out_dtype=torch.int64)
    assert got.dtype == torch.int64 and torch.equal(got, crop(x, (180, 200)).long())


@pytest.mark.parametrize('K,B', [(64, 1), (16, 2)])
def test_round_trip_tall(K, B):
    """712x88: boxes whose decoder stage is cut on both sides, at the top only, and not at all."""
    H, W = 712, 88
    x, files, _ = encoded(K, B, H, W)
    bc = bitcoding(K)
    for box, decoder in (((330, 360), (64, 640)), ((500, 520, 7, 80), (256, 712)), ((40, 41), (0, 320)), ((711, 712), (448, 712)), ((0, H), (0, H))):
        got, info = bc.decode_region(files, box)
        assert torch.equal(got, crop(x, box)), (box, info)
        if K == 64:
            assert info.decoder_rows == decoder, (box, info)
        assert info.decoder_rows[0] <= info.conv_rows[0] and info.conv_rows[1] <= info.decoder_rows[1]


def test_all_rows_of_one_image_take_lag_2():
    """(0, H) of one K = 64 image of 328x88 is 57 entries of 512 symbols: the side stream with a single image."""
    x, files, _ = encoded(64, 1, 328, 88)
    bc = bitcoding(64)
    got, info = bc.decode_region(files, (0, 328))
    assert info.bands == (0, info.n_bands) and info.n_bands == 57 and info.conv_rows == (0, 328)
    assert info.streams_used == info.streams_total and info.bytes_used == info.bytes_total
    assert bc._rgb_schedule(info.bands[1], None)[0] == 2 and torch.equal(got, x)


def test_box_errors():
    x, files, padding = encoded(16, 1, 317, 83)
    bc = bitcoding(16)
    for box in ((5, 5), (9, 4), (0, 318), (-1, 3), (0, 10, 0, 84), (0, 10, 5, 5), (1, 2, 3)):
        with pytest.raises(ValueError):
            bc.decode_region(files, box)
    other = bitcoding(16).encode_batch(pad.pad(images(1, 317, 83).long(), fac=8, mode=blueprint().get_padding_mode())[0].cuda()).to_bytes(
        [(3, 2, 2, 1)])
    with pytest.raises(ValueError):
        bc.decode_region(files + other, (0, 10))
    with pytest.raises(ValueError):
        bc.decode_region([], (0, 10))


# ---- 3. the rest is really not read ------------------------------------------------------------------------------------------------


def test_bands_outside_the_region_are_not_read():
    """K = 16, the 320x88 frame: rows [190, 210) lie in bands 9 and 10 (band 9 starts in row 183: conv rows (128, 256)).  Bands 3 and 13
    of every channel, complemented, destroy the whole decode and leave the region alone."""
    x, files, _ = encoded(16, 1, 320, 88)
    bc = bitcoding(16)
    box = (190, 210)
    parsed = container.parse_banded(files[0])
    offset, nbytes = parsed.offset[-1], parsed.nbytes[-1]                     # (3, 16) of the finest record
    assert offset.shape == (3, 16)
    damaged = np.frombuffer(files[0], dtype=np.uint8).copy()
    for c in range(3):
        for j in (3, 13):
            a, n = int(offset[c, j]), int(nbytes[c, j])
            assert n > 16
            damaged[a:a + n] ^= 0xFF
    damaged = damaged.tobytes()
    assert len(damaged) == len(files[0]) and damaged != files[0]
    got, info = bc.decode_region([damaged], box)
    assert torch.equal(got, crop(x, box))
    assert not torch.equal(bc.decode_batch([damaged], out_dtype=torch.uint8)[0], x)          # the test bites
    assert info.bands == (9, 11) and info.sym_rows == (183, 210) and info.conv_rows == (128, 256) and info.valid_rows == (168, 216)
    assert info.streams_used == 6 and info.streams_total == 48
    assert info.bytes_used == int(nbytes[:, 9:11].sum()) < info.bytes_total == int(nbytes.sum())


# ---- 4. legacy file ----------------------------------------------------------------------------------------------------------------


def test_legacy_file():
    x, files, _ = encoded(0, 1, 320, 88)
    assert not container.is_banded(files[0])
    got, info = bitcoding(0).decode_region(files, (0, 40))
    assert torch.equal(got, crop(x, (0, 40)))
    assert info.conv_rows == (0, 128) and info.bands == (0, 1) and info.n_bands == 1 and info.sym_rows == (0, 40)
    assert info.streams_used == info.streams_total == 3                       # one stream per channel: all of its bytes are "used"
    got, info = bitcoding(16).decode_region(files, (300, 320, 80, 88))          # (the decoder reads either format whatever it writes)
    assert torch.equal(got, crop(x, (300, 320, 80, 88))) and info.conv_rows == (0, 320) and info.sym_rows == (0, 320)


# ---- 5. sealed banded file ---------------------------------------------------------------------------------------------------------


class Calls(object):
    """Counts every call into the library that goes through _lib.call (ops.call is the same function under another name)."""

    def __init__(self, monkeypatch):
        from l3c_pytorch_amd import _lib, ops
        self.n = 0
        real = _lib.call

        def counting(name, *args):
            self.n += 1
            return real(name, *args)
        for mod in (_lib, ops):
            monkeypatch.setattr(mod, 'call', counting)


def test_sealed_banded_file(monkeypatch):
    x, files, _ = encoded(16, 1, 320, 88, seal=True)
    assert container.is_sealed(files[0])
    bc = bitcoding(16)
    got, info = bc.decode_region(files, (180, 200))
    assert torch.equal(got, crop(x, (180, 200)))
    assert info.sealed == 1 and info.verified == ('generation', 'model') and info.pixel_crc_checked is False
    assert 'pixel CRC not checked' in info.line()
    got, info = bc.decode_region(files, (180, 200), verify=False)
    assert torch.equal(got, crop(x, (180, 200))) and info.sealed == 1 and info.verified == () and info.pixel_crc_checked is False
    body, seal = container.split_seal(files[0])
    foreign = body + container.make_seal(body, seal.generation + 1, seal.frame_crc, seal.model_id)
    calls = Calls(monkeypatch)
    with pytest.raises(SealError) as e:
        bc.decode_region([foreign], (180, 200))
    assert e.value.reason == 'generation' and e.value.index == 0 and calls.n == 0       # before anything is enqueued
    got, _ = bc.decode_region(files, (180, 200))
    assert calls.n > 0                                                                  # the counter does see a decode that runs
    monkeypatch.undo()
    assert torch.equal(bc.decode_region([foreign], (180, 200), verify=False)[0], crop(x, (180, 200)))


# ---- 6. refusals, the one-file wrapper and the CLI ---------------------------------------------------------------------------------


def test_refusals(tmp_path):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    with open(GOLDEN + '/hip_rgb_shared_32x48_r3.l3c', 'rb') as f:
        rgb_file = f.read()
    with pytest.raises(NotImplementedError):
        Bitcoding(blueprint('cr_rgb_shared'), auto_recurse=3).decode_region([rgb_file], (0, 8))
    _, files, _ = encoded(16, 1, 320, 88)
    part = str(tmp_path / 'big.l3c.part0')
    with open(part, 'wb') as f:
        f.write(files[0])
    with pytest.raises(NotImplementedError):
        bitcoding(16).decode(part, region=(0, 8))


def test_decode_wrapper(tmp_path):
    x, files, _ = encoded(16, 1, 317, 83)
    p = str(tmp_path / 'one.l3c')
    with open(p, 'wb') as f:
        f.write(files[0])
    got, info = bitcoding(16).decode(p, region=(180, 200, 3, 50))
    assert got.dtype == torch.int64 and torch.equal(got, crop(x, (180, 200, 3, 50)).long())
    assert isinstance(info, region.RegionInfo) and info.box == (180, 200, 3, 50) and info.as_dict()['conv_rows'] == info.conv_rows


def test_l3c_cli_region(synthetic_l3c, tmp_path, capsys):
    """`l3c.py ... enc --bands 16`, then `dec --region 100:140,5:60` writes the box and prints the info line; a box outside the image is a
    DecodeError line and status 1."""
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
    assert cli.parse_region('3:9') == (3, 9) and cli.parse_region('3:9,0:4') == (3, 9, 0, 4)
    args = [str(tmp_path / 'logs'), '0306_0001']
    assert cli.main(args + ['enc', '--bands', '16', src, out]) == 0
    capsys.readouterr()
    assert cli.main(args + ['dec', '--region', '100:140,5:60', out, png]) == 0
    said = capsys.readouterr().out
    assert 'region rows [100, 140) x columns [5, 60): bands ' in said and ' of 16, ' in said and 'payload bytes of the finest record' in said
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1), img[:, 100:140, 5:60])
    assert cli.main(args + ['dec', '--region', '100:191', out, png]) == 1
    assert 'DecodeError:' in capsys.readouterr().out
