"""-m gpu: preview decode -- a picture from the coarse records of a `.l3c` file (Bitcoding.decode_preview / preview, l3c.py preview).
The estimator (l3c_dmll_mean: the mixture's mean, snapped to a symbol) against fp64, its exact ties and its range; the walk against the
exact decoder (records == total), against its own restatement, on prefixes of files, and against the CPU oracle's mean preview."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dmll as odmll, net as onet  # noqa: E402
from tests import ref64  # noqa: E402
from tests.golden import make_hip_bitstream as gen  # noqa: E402

_BP = {}


def blueprint(cfg):
    if cfg not in _BP:
        _BP[cfg] = gen.blueprint(cfg, True)
    return _BP[cfg]


def _mean(P, C, K, rgb):
    """ops.dmll_mean on a logical (B, Kp, H, W) numpy P -> int64 numpy symbols (B, C, H, W)."""
    from l3c_pytorch_amd import ops
    x_min, x_max, L = ref64.alphabet(rgb)
    P_nhwc = torch.from_numpy(np.ascontiguousarray(P.transpose(0, 2, 3, 1))).cuda()
    return ops.dmll_mean(P_nhwc, C, K, rgb, x_min, x_max, L).cpu().numpy().astype(np.int64)


# ---- 1. the kernel against fp64 --------------------------------------------------------------------------------------------------

EXCUSED_CAP = 0.02


@pytest.mark.parametrize('rgb', [True, False], ids=['rgb', 'z'])
def test_mean_kernel_against_fp64(rgb):
    """Channel by channel against fp64 from P, conditioned on the KERNEL's own symbols of the earlier channels (every channel is judged
    alone).  A pixel is excused iff fp64's scaled mean t is within bound / bw + 1e-6 of a rounding tie, with
        bound = sum_k (PI_BOUND + 16 u pi_k) (|mu_k| + |a_k| + |b_k|)         a, b: the two coupling terms, u = 2^-24
    (pi within PI_BOUND absolutely; per term a product, up to K additions and the coupling's own roundings, in either summation
    order); everywhere else the symbol must EQUAL clip(rint(t), 0, L-1).  The excused share is a cap, not a tolerance: 2 % per (alphabet,
    regime), pooled over the four shapes (the fp32 reference alone: at most 0.50 %)."""
    x_min, x_max, L = ref64.alphabet(rgb)
    bw = (x_max - x_min) / (L - 1)
    for regime in ref64.regimes(rgb):
        n = n_excused = 0
        for H, W in ref64.SHAPES:
            P, _, C, K = ref64.head_case(regime, rgb, H, W)
            got = _mean(P, C, K, rgb)
            assert got.shape == (2, C, H, W) and got.min() >= 0 and got.max() <= L - 1
            x = ref64.values_of(got, rgb)
            l, _ = ref64._split(P, rgb, C)
            for c in range(C):
                pi, mu, _ = ref64.params64(P, x, rgb, C, K, c)
                a, b = ref64._coupling64(l, x, rgb, c)
                t = (np.clip((pi * mu).sum(axis=1), x_min, x_max) - x_min) / bw
                bound = ((ref64.PI_BOUND + 16 * ref64.U32 * pi) * (np.abs(l[:, 1, c]) + np.abs(a) + np.abs(b))).sum(axis=1)
                excused = np.abs(np.abs(t - np.floor(t)) - 0.5) <= bound / bw + 1e-6
                want = np.clip(np.rint(t), 0, L - 1).astype(np.int64)
                wrong = (got[:, c] != want) & ~excused
                assert not wrong.any(), (regime, (H, W), c, int(wrong.sum()), got[:, c][wrong][:4], want[wrong][:4], t[wrong][:4])
                n += excused.size
                n_excused += int(excused.sum())
        print('rgb={} {}: excused {:.3%} of {}'.format(rgb, regime, n_excused / n, n))
        assert n_excused <= EXCUSED_CAP * n, (regime, n_excused, n)


# ---- 2. exact ties and the range -------------------------------------------------------------------------------------------------


def _tie_P(mu0, mu1=0.0):
    """RGB, K = 2, one pixel per entry of mu0 (the same in all three channels): logits (0, -200) -- pi is exactly (1, 0) in fp32 --,
    lambdas -200 (sigmoid exactly 0), log_sigma 0."""
    n = len(mu0)
    P = np.zeros((1, 4, 3, 2, 1, n), dtype=np.float32)
    P[:, 0, :, 1] = -200.0
    P[:, 1, :, 0] = np.asarray(mu0, dtype=np.float32)
    P[:, 1, :, 1] = mu1
    P[:, 3] = -200.0
    return P.reshape(1, 24, 1, n)


def test_exact_ties_and_the_range():
    got = _mean(_tie_P([0.5, 100.5, 101.5, 254.5]), 3, 2, True)
    assert got.shape == (1, 3, 1, 4)
    for c in range(3):
        assert got[0, c, 0].tolist() == [0, 100, 102, 254], (c, got[0, c, 0])           # ties go to even
    for rgb in (True, False):
        L = ref64.alphabet(rgb)[2]
        P, _, C, K = ref64.head_case('offrange', rgb, *ref64.SHAPES[0])
        sym = _mean(P, C, K, rgb)
        assert np.isin(sym, (0, L - 1)).all() and (sym == 0).any() and (sym == L - 1).any()
    # infinite and NaN means: the clamp takes +inf to x_max, -inf and NaN to x_min; a NaN made on the way (0 * inf) is a NaN
    inf, nan = np.inf, np.nan
    got = _mean(_tie_P([inf, -inf, nan, 300.0, -5.0, 77.0]), 3, 2, True)
    assert got.min() >= 0 and got.max() <= 255
    assert got[0, 0, 0].tolist() == [255, 0, 0, 255, 0, 77]
    got = _mean(_tie_P([10.0, 20.0, 30.0], mu1=np.asarray([inf, -inf, nan], dtype=np.float32)), 3, 2, True)
    assert got.min() >= 0 and got.max() <= 255
    lam = _tie_P([40.0, 50.0])
    lam.reshape(1, 4, 3, 2, 1, 2)[0, 3, :, :, 0, 1] = nan                                        # pixel 1: NaN lambdas
    got = _mean(lam, 3, 2, True)
    assert got[0, :, 0, 0].tolist() == [40, 40, 40] and got[0, 0, 0, 1] == 50 and got.min() >= 0 and got.max() <= 255


# ---- the cases of the walk -------------------------------------------------------------------------------------------------------


def _walk_case(name):
    """-> (Bitcoding, images (B,3,H,W) long, total records)."""
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.helpers import synthetic
    if name == 'rgb_shared':
        bc = Bitcoding(blueprint('cr_rgb_shared'), auto_recurse=3)
        imgs = gen.rgb_case()
    else:
        bc = Bitcoding(blueprint('cr'), bands=7 if name == 'banded' else 0)
        imgs = torch.cat([gen.l3c_case(), synthetic.make_image(64, 96, 5, 'natural').unsqueeze(0).long()])
    return bc, imgs, bc.n_predicted_scales() + 1


_FILES = {}


def _files(name):
    if name not in _FILES:
        bc, imgs, total = _walk_case(name)
        out = bc.blueprint.net(imgs.to('cuda', torch.float32), bc.auto_recurse)
        files = bc.encode_batch(imgs, out=out).to_bytes()
        _FILES[name] = (bc, imgs, total, out, files)
    return _FILES[name]


# ---- 3. records == total is the decoder ------------------------------------------------------------------------------------------


@pytest.mark.parametrize('name', ['legacy', 'banded'])
def test_all_records_is_the_exact_decode(name):
    from l3c_pytorch_amd.bitcoding import container
    bc, imgs, total, _, files = _files(name)
    assert total == 4 and len(files) == 2 and container.is_banded(files[0]) == (name == 'banded')
    want, pads = bc.decode_batch(files)
    got, pads_p = bc.decode_preview(files, records=total, out_dtype=torch.int64)
    assert got.dtype == want.dtype and torch.equal(got, want) and pads_p == pads
    assert torch.equal(got.cpu(), imgs)
    got8, _ = bc.decode_preview(files, records=total)
    assert got8.dtype == torch.uint8 and got8.is_cuda and torch.equal(got8.cpu().long(), imgs)
    with pytest.raises(ValueError):
        bc.decode_preview(files, records=total + 1)
    with pytest.raises(ValueError):
        bc.decode_preview(files, records=0)


# ---- 4. the walk is the composition ----------------------------------------------------------------------------------------------


def _restated(bc, out, total, records):
    """The encoder's symbols for the first `records` records, then get_P -> dmll_mean -> _next_input per estimated scale."""
    from l3c_pytorch_amd import ops
    net = bc.blueprint.net
    K = net.config_ms.prob.K
    n_pred = total - 1
    bn, F, sym = None, None, None
    for k, (scale, dmll, uniform) in enumerate(bc.iter_scale_dmll(n_pred)):
        if not uniform:
            P, F = net.get_P(scale, bn, F, n_scales_total=n_pred)
        if k < records:
            sym = out.raw.sym[scale]
        else:
            C = 3 if dmll.rgb_scale else net.config_ms.q.C
            sym = ops.dmll_mean(ops.as_pixel_major(P), C, K, dmll.rgb_scale, dmll.x_min, dmll.x_max, dmll.L)
        if scale > 0:
            bn = bc._next_input(sym, dmll)
    return sym


@pytest.mark.parametrize('name', ['legacy', 'banded', 'rgb_shared'])
def test_the_walk_is_the_composition(name):
    bc, imgs, total, out, files = _files(name)
    assert total == (5 if name == 'rgb_shared' else 4)
    default, _ = bc.decode_preview(files)
    for records in range(1, total):
        got, pads = bc.decode_preview(files, records=records, out_dtype=torch.int16)
        want = _restated(bc, out, total, records)
        assert got.shape == imgs.shape and got.dtype == torch.int16 and pads == [(0, 0, 0, 0)] * len(files)
        assert torch.equal(got, want.to(torch.int16)), (name, records, int((got != want).sum()))
        if records == total - 1:
            assert torch.equal(default.to(torch.int16), got)          # the default: everything but the finest record


# ---- 5. a prefix is enough -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('name', ['legacy', 'banded'])
def test_a_prefix_is_enough(name):
    from l3c_pytorch_amd.bitcoding import container
    bc, imgs, total, _, files = _files(name)
    for r in range(1, total):
        whole, _ = bc.decode_preview(files, records=r)
        ends = [container.prefix_bytes(f, r) for f in files]
        cut = [f[:e] for f, e in zip(files, ends)]
        stray = [f[:e + 100] for f, e in zip(files, ends)]
        assert all(e + 100 < container.prefix_bytes(f, r + 1) for f, e in zip(files, ends))       # stray: inside the next record
        for pieces in (cut, stray, [cut[0], files[1]]):
            got, _ = bc.decode_preview(pieces, records=r)
            assert torch.equal(got, whole), (name, r)
        got, _ = bc.decode_preview(cut)                                # the default on a prefix: all it holds (the finest is not in it)
        assert torch.equal(got, whole)
        for pieces in (cut, stray):
            with pytest.raises(ValueError):
                bc.decode_preview(pieces, records=r + 1)
    with pytest.raises(ValueError, match='invalid file'):
        bc.decode_preview([f[:container.prefix_bytes(f, 1) - 1] for f in files])


# ---- 6. it is a picture ----------------------------------------------------------------------------------------------------------


def _oracle_mean_sym(spec, P, C):
    x = torch.zeros(P.shape[0], C, P.shape[2], P.shape[3])
    sym = torch.zeros(x.shape, dtype=torch.int64)
    for c in range(C):
        pi, mu, _ = odmll.params_for_channel(spec, P, c, C, x)
        sym[:, c] = spec.to_sym((pi * mu).sum(dim=1))
        x[:, c] = spec.to_bn(sym[:, c])
    return sym


def _oracle_preview(out, sd, records):
    """The CPU oracle's mean preview from its forward pass `out`: the first `records` of the four records are the encoder's symbols, every
    finer scale the snapped mean of the mixture the oracle network predicts for it."""
    hp = onet.L3C_HYPER
    z = odmll.z_spec(hp.levels_range, hp.L)
    with torch.no_grad():
        bn, f, sym = out.bn[hp.num_scales], None, None
        for s in reversed(range(hp.num_scales)):
            P, f = onet.get_P(s, bn, f, sd)
            spec, C = (odmll.RGB, 3) if s == 0 else (z, hp.C)
            sym = out.S[s] if hp.num_scales - s < records else _oracle_mean_sym(spec, P, C)
            bn = spec.to_bn(sym)
    return sym


def _psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.parametrize('H,W,seed', [(64, 64, 0), (96, 128, 1)])
def test_it_is_a_picture(H, W, seed, synthetic_l3c_cal):
    """PSNR against the original of the HIP preview at records = 3, 2, 1: at least the CPU oracle's mean preview's minus 0.5 dB (a quarter
    of the smallest step between adjacent depths, 1.8 dB: a walk that drops, repeats or misorders a scale fails, the rounding-tie flips of
    two fp32 implementations pass), and strictly ordered 3 > 2 > 1 > flat grey."""
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.helpers import synthetic
    _, sd = synthetic_l3c_cal
    img = synthetic.make_image(H, W, seed, 'natural').unsqueeze(0).long()
    bc = Bitcoding(blueprint('cr'))
    data = bc.encode_batch(img).to_bytes()
    with torch.no_grad():
        oracle_out = onet.forward(img.float(), sd)
    hip, oracle = [], []
    for records in (3, 2, 1):
        got, _ = bc.decode_preview(data, records=records)
        assert tuple(got.shape) == (1, 3, H, W)
        hip.append(_psnr(got.cpu(), img))
        oracle.append(_psnr(_oracle_preview(oracle_out, sd, records), img))
    grey = _psnr(torch.full_like(img, 128), img)
    print('{}x{} seed {}: PSNR records 3 / 2 / 1: hip {} oracle {} difference {} flat grey {:.2f}'.format(
        H, W, seed, ' / '.join('{:.2f}'.format(v) for v in hip), ' / '.join('{:.2f}'.format(v) for v in oracle),
        ' / '.join('{:+.3f}'.format(a - b) for a, b in zip(hip, oracle)), grey))
    for a, b in zip(hip, oracle):
        assert a >= b - 0.5, (hip, oracle)
    assert hip[0] > hip[1] > hip[2] > grey, (hip, grey)


# ---- 7. file API and CLI ---------------------------------------------------------------------------------------------------------


def test_file_api_and_cli(synthetic_l3c, tmp_path):
    import subprocess
    import sys
    from PIL import Image
    from l3c_pytorch_amd.bitcoding import container
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import synthetic
    cfg, sd = synthetic_l3c
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = tmp_path / 'logs' / '0306_0001 cr oi' / 'ckpts'
    exp.mkdir(parents=True)
    torch.save({'net': sd}, str(exp / 'ckpt_0000000001.pt'))
    img = synthetic.make_image(45, 70, 21, 'natural')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(sd, strict=True)
    bp.set_eval()
    bc = Bitcoding(bp)
    path = str(tmp_path / 'p.l3c')
    bc.encode(img.long().unsqueeze(0), path)
    data = open(path, 'rb').read()
    assert any(container.parse_containers([data]).padding[0])                                    # 45x70 is padded
    got = bc.preview(path)
    assert tuple(got.shape) == (1, 3, 45, 70) and got.dtype == torch.uint8 and got.is_cuda
    three = container.prefix_bytes(data, 3)
    assert torch.equal(bc.preview(path, max_bytes=three), got) and torch.equal(bc.preview(path, records=3), got)
    assert tuple(bc.preview(path, max_bytes=container.prefix_bytes(data, 1) + 3).shape) == (1, 3, 45, 70)
    assert torch.equal(bc.preview(path, records=4).long(), bc.decode(path)) and torch.equal(bc.decode(path).cpu()[0], img.long())
    with pytest.raises(ValueError):
        bc.preview(path, records=4, max_bytes=three)
    with pytest.raises(NotImplementedError, match='part'):
        bc.preview(path + '.part0')
    png = str(tmp_path / 'preview.png')
    r = subprocess.run([sys.executable, os.path.join(root, 'l3c.py'), str(tmp_path / 'logs'), '0306_0001', 'preview', path, png,
                        '--bytes', str(three)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '3 of 4' in r.stdout and '{} of {} bytes'.format(three, len(data)) in r.stdout, r.stdout
    shown = torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1)
    assert tuple(shown.shape) == (3, 45, 70) and torch.equal(shown, got.cpu()[0])
