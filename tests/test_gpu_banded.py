"""-m gpu: banded `.l3c` files (Bitcoding(bands=K)) -- the band payloads are the oracle coder's bytes, bands=1 reproduces the committed
legacy payloads, the framing costs what the format says, and every path (encode_batch / decode_batch, encode / decode with auto-crop,
l3c.py) round-trips losslessly; malformed files and the legacy-only readers raise ValueError."""
import json
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ac as oracle_ac  # noqa: E402
from tests.conftest import GOLDEN  # noqa: E402
from tests.golden import make_hip_bitstream as gen  # noqa: E402

CASES = [('hip_l3c_cal_64x96.l3c', 'cr'), ('hip_rgb_shared_32x48_r3.l3c', 'cr_rgb_shared')]
_BP = {}


def blueprint(cfg):
    if cfg not in _BP:
        _BP[cfg] = gen.blueprint(cfg, True)
    return _BP[cfg]


def case(fname):
    with open(os.path.join(GOLDEN, 'hip_bitstream.json')) as f:
        meta = json.load(f)['files'][fname]
    cfg = dict(CASES)[fname]
    image = gen.l3c_case() if cfg == 'cr' else gen.rgb_case()
    return blueprint(cfg), image, meta['auto_recurse'], open(os.path.join(GOLDEN, fname), 'rb').read()


def band_payloads(data):
    from l3c_pytorch_amd.bitcoding.bitcoding import parse_banded
    p = parse_banded(data)
    return p, [[[data[o:o + n] for o, n in zip(p.offset[k][c], p.nbytes[k][c])] for c in range(C)]
               for k, (C, H, W, L) in enumerate(p.scales)]


@pytest.mark.parametrize('fname', [c[0] for c in CASES])
def test_one_band_is_the_committed_legacy_payloads(fname):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding, parse_containers
    bp, image, recurse, legacy = case(fname)
    data = Bitcoding(bp, auto_recurse=recurse, bands=1).encode_batch(image).to_bytes()[0]
    p, bands = band_payloads(data)
    q = parse_containers([legacy])
    assert [s[:3] for s in p.scales] == [tuple(s) for s in q.scales]
    for k, (C, H, W) in enumerate(q.scales):
        for c in range(C):
            o, n = int(q.offset[k][0, c]), int(q.nbytes[k][0, c])
            assert bands[k][c] == [legacy[o:o + n]], (k, c)
    dec, pads = Bitcoding(bp, auto_recurse=recurse).decode_batch([data])
    assert torch.equal(dec.cpu(), image) and pads == [(0, 0, 0, 0)]
    # bands=0 is the legacy format, byte for byte
    assert Bitcoding(bp, auto_recurse=recurse, bands=0).encode_batch(image).to_bytes()[0] == legacy


def _oracle_tables(bc, image):
    """Per scale record (coarse -> fine): (symbols (C, HW) numpy, table rows (C, HW, Lp) uint16 or the uniform row) as the legacy encoder
    codes them -- the rows built with ops from P and the symbols."""
    from l3c_pytorch_amd import ops
    from l3c_pytorch_amd.bitcoding.bitcoding import uniform_cdf_row
    out = bc.blueprint.net(image.to('cuda', torch.float32), bc.auto_recurse)
    K = bc.blueprint.net.config_ms.prob.K
    res = []
    for scale, dmll, uniform in bc.iter_scale_dmll():
        sym = out.raw.sym[scale]
        _, C, Hs, Ws = sym.shape
        s_np = sym[0].reshape(C, -1).cpu().numpy()
        if uniform:
            rows = [uniform_cdf_row(dmll.L).numpy().view(np.uint16)] * C
        else:
            rows = [ops.dmll_cdf_table(out.raw.P[scale], sym.contiguous(), bc._targets(dmll), C, K, dmll.rgb_scale, c, 0, Hs * Ws)[0]
                    .cpu().numpy().view(np.uint16) for c in range(C)]
        res.append((s_np, rows, uniform))
    return out, res


@pytest.mark.parametrize('K', [2, 7, 64])
def test_band_payloads_are_the_oracle_coders_and_decode_losslessly(K):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding, n_bands
    bp, image, recurse, legacy = case('hip_l3c_cal_64x96.l3c')
    bc = Bitcoding(bp, bands=K)
    out, tables = _oracle_tables(bc, image)
    data = bc.encode_batch(image, out=out).to_bytes()[0]
    p, bands = band_payloads(data)
    oracle_extra, E = 0, 0
    for k, (C, H, W, L) in enumerate(p.scales):
        assert L == 64 * -(-(H * W) // (64 * K))
        s_np, rows, uniform = tables[k]
        n = n_bands(H * W, L)
        E += C * (n - 1)
        for c in range(C):
            whole = oracle_ac.encode(rows[c], s_np[c])
            assert len(bands[k][c]) == n
            for j in range(n):
                sl = slice(j * L, min((j + 1) * L, H * W))
                want = oracle_ac.encode(rows[c] if uniform else rows[c][sl], s_np[c][sl])
                assert bands[k][c][j] == want, (k, c, j)
            oracle_extra += sum(len(b) for b in bands[k][c]) - len(whole)
    # the size bound (issue: framing 6 + 4 per scale + 4 per extra band, the coder's flush at most 2 bytes per extra band), first on the
    # oracle's own band bytes, then on the files
    assert oracle_extra <= 2 * E, (oracle_extra, E)
    n_scales = len(p.scales)
    print('K', K, 'extra bands', E, 'banded', len(data), 'legacy', len(legacy), 'coder extra', oracle_extra)
    assert len(data) - len(legacy) <= 6 + 4 * n_scales + 4 * E + 2 * E
    # lossless, and every scale's symbols are the legacy decode's
    dec, _ = Bitcoding(bp).decode_batch([data])
    assert torch.equal(dec.cpu(), image)
    syms = _decoded_symbols(bp, data)
    want = _decoded_symbols(bp, legacy)
    assert len(syms) == len(want) and all(torch.equal(a, b) for a, b in zip(syms, want))


def _decoded_symbols(bp, data):
    """Every scale's decoded symbols: the decoder's bottleneck input, recorded through sym_to_bn."""
    from l3c_pytorch_amd import ops
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    seen = []
    orig = ops.sym_to_bn

    def spy(sym, *a):
        seen.append(sym.clone().cpu())
        return orig(sym, *a)
    ops.sym_to_bn = spy
    try:
        dec, _ = Bitcoding(bp).decode_batch([data])
    finally:
        ops.sym_to_bn = orig
    return seen + [dec.cpu().to(torch.int16)]


def test_rgb_shared_with_recursion_round_trips_for_several_band_counts():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    bp, image, recurse, legacy = case('hip_rgb_shared_32x48_r3.l3c')
    for K in (3, 16):
        data = Bitcoding(bp, auto_recurse=recurse, bands=K).encode_batch(image).to_bytes()[0]
        for window in ('auto', 'always', 'never'):
            dec, _ = Bitcoding(bp, auto_recurse=recurse, rgb_window=window).decode_batch([data])
            assert torch.equal(dec.cpu(), image), (K, window)


def test_768x512_batch_and_single_files():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.helpers import synthetic
    bp = blueprint('cr')
    imgs = torch.stack([synthetic.make_image(512, 768, 900 + i, 'natural') for i in range(4)]).long()
    bc = Bitcoding(bp, bands=64)
    files = bc.encode_batch(imgs).to_bytes()
    dec, _ = bc.decode_batch(files)
    assert torch.equal(dec.cpu(), imgs)
    for i, f in enumerate(files):
        one, _ = bc.decode_batch([f])
        assert torch.equal(one.cpu(), dec[i:i + 1].cpu()), i
    # the files assembled on the device are the host's join of the band payloads
    assert files == bc.encode_batch(imgs).to_bytes_host_assembled()


def test_small_image_with_a_coarsest_scale_below_64_symbols():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding, parse_banded
    from l3c_pytorch_amd.helpers import synthetic
    img = synthetic.make_image(24, 40, 5, 'natural').long().unsqueeze(0)
    for K in (1, 4, 1024):
        data = Bitcoding(blueprint('cr'), bands=K).encode_batch(img).to_bytes()[0]
        p = parse_banded(data)
        assert p.scales[0][:3] == (5, 3, 5) and p.scales[0][3] == 64 and p.nbytes[0].shape == (5, 1)
        dec, _ = Bitcoding(blueprint('cr')).decode_batch([data])
        assert torch.equal(dec.cpu(), img), K


def test_file_api_with_auto_crop(tmp_path, monkeypatch):
    from l3c_pytorch_amd import auto_crop
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding, is_banded
    from l3c_pytorch_amd.helpers import synthetic
    img = synthetic.make_image(70, 90, 8, 'natural').long().unsqueeze(0)
    monkeypatch.setattr(auto_crop, '_NEEDS_CROP_DIM', 40 * 40)
    bc = Bitcoding(blueprint('cr'), bands=16)
    p = str(tmp_path / 'x.l3c')
    bc.encode(img, p)
    parts = sorted(f for f in os.listdir(tmp_path) if f.startswith('x.l3c.part'))
    assert len(parts) == 4 and all(is_banded(open(str(tmp_path / f), 'rb').read()) for f in parts)
    assert torch.equal(Bitcoding(blueprint('cr')).decode(p + '.part0').cpu(), img)
    # and one file without cropping, padded
    monkeypatch.setattr(auto_crop, '_NEEDS_CROP_DIM', 10 ** 9)
    q = str(tmp_path / 'y.l3c')
    bc.encode(img, q)
    assert is_banded(open(q, 'rb').read())
    assert torch.equal(Bitcoding(blueprint('cr')).decode(q).cpu(), img)


def test_malformed_banded_files_and_legacy_readers_raise():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding, parse_banded
    from l3c_pytorch_amd.helpers import dataset_codec
    bp, image, recurse, legacy = case('hip_l3c_cal_64x96.l3c')
    bc = Bitcoding(bp)
    data = Bitcoding(bp, bands=4).encode_batch(image).to_bytes()[0]
    p = parse_banded(data)
    h1 = int(p.offset[1][0, 0]) - 4 - 9          # the second record's header: 5 x 16 x 24, L = 128, three bands
    assert p.scales[1] == (5, 16, 24, 128)
    bad = {
        'version': data[:4] + b'\x02' + data[5:],
        'reserved': data[:5] + b'\x01' + data[6:],
        'C == 0': data[:14] + b'\x00' + data[15:],
        'L == 0': data[:19] + struct.pack('<I', 0) + data[23:],
        'L % 64': data[:19] + struct.pack('<I', 96) + data[23:],
        'n > 1024': data[:14] + struct.pack('<BHHI', 5, 1000, 1000, 64) + data[23:],
        'length past the end': data[:int(p.offset[3][0, 0]) - 4] + struct.pack('<I', len(data)) + data[int(p.offset[3][0, 0]):],
        'payload past the end': data[:-10],
        'missing magic': data[:-4] + b'\x00\x00\x00\x00',
        'trailing bytes': data + b'\x00' * 3,
        'shape the network does not predict': data[:h1] + struct.pack('<BHH', 5, 15, 24) + data[h1 + 5:],     # still three bands
    }
    for what, f in bad.items():
        with pytest.raises(ValueError):
            bc.decode_batch([f])
        assert what
    # a batch of banded files with different band lengths per scale
    other = Bitcoding(bp, bands=2).encode_batch(image).to_bytes()[0]
    with pytest.raises(ValueError, match='band length'):
        bc.decode_batch([data, other])
    with pytest.raises(ValueError, match='mixes'):
        bc.decode_batch([data, legacy])
    # the legacy-only readers name the format and never return pixels
    with pytest.raises(ValueError, match='banded'):
        bc.decode_many([[data]])
    with pytest.raises(ValueError, match='banded'):
        bc.decode_many([[legacy], [data]])
    with pytest.raises(ValueError, match='banded'):
        dataset_codec.decode_set(bc, {0: data}, [0])


def test_encode_many_writes_banded_files():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding, EncodedBatch, is_banded
    from l3c_pytorch_amd.helpers import synthetic
    a = torch.stack([synthetic.make_image(32, 48, 60 + i, 'natural') for i in range(2)]).long()
    b = synthetic.make_image(64, 40, 70, 'natural').long().unsqueeze(0)
    bc = Bitcoding(blueprint('cr'), bands=8)
    encs = bc.encode_many([a.cuda().float(), b.cuda().float()])
    files = EncodedBatch.many_to_bytes(encs)
    assert all(is_banded(f) for fs in files for f in fs)
    assert files[0] == bc.encode_batch(a).to_bytes() and files[1] == bc.encode_batch(b).to_bytes()
    assert torch.equal(bc.decode_batch(files[0])[0].cpu(), a) and torch.equal(bc.decode_batch(files[1])[0].cpu(), b)


def test_l3c_cli_bands_round_trip(synthetic_l3c, tmp_path):
    import subprocess
    import sys
    from PIL import Image
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding, is_banded
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import pad, synthetic
    cfg, sd = synthetic_l3c
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = tmp_path / 'logs' / '0306_0001 cr oi' / 'ckpts'
    exp.mkdir(parents=True)
    torch.save({'net': sd}, str(exp / 'ckpt_0000000001.pt'))
    img = synthetic.make_image(45, 70, 21, 'natural')
    src = str(tmp_path / 'in.png')
    Image.fromarray(img.permute(1, 2, 0).numpy()).save(src)

    def cli(*args):
        r = subprocess.run([sys.executable, os.path.join(root, 'l3c.py'), str(tmp_path / 'logs'), '0306_0001'] + list(args),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout
    banded, plain, png = str(tmp_path / 'b.l3c'), str(tmp_path / 'p.l3c'), str(tmp_path / 'dec.png')
    said = cli('--compare_theory', 'enc', src, banded, '--bands', '64')
    assert is_banded(open(banded, 'rb').read())
    theory = [ln for ln in said.splitlines() if ln.startswith(('theory:', 'assumed:'))]      # per-scale sizes of the banded file
    assert len(theory) == 2 and all(ln.count('|') == 3 for ln in theory), said
    cli('dec', banded, png)
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1), img)
    cli('enc', src, plain)
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(sd, strict=True)
    bp.set_eval()
    bc = Bitcoding(bp)
    padded, padding = pad.pad(img.long().unsqueeze(0), fac=bc.padding_factor(), mode=bp.get_padding_mode())
    assert open(plain, 'rb').read() == bc.encode_batch(padded).to_bytes([padding])[0]
